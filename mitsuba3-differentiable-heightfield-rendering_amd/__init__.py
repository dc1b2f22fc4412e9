"""MI355X-native differentiable heightfield intersector: host-side mirror of the
reference's Shape plugin interface over the C ABI of libhf.so (include/hf.h)."""
from . import build, workload  # noqa: F401
from ._capi import HfError  # noqa: F401
from .shape import (Adam, Bitmap, DirectionSample3f, Envmap, Frame3f, Heightfield, LargeSteps, ParamFlags,  # noqa: F401
                    PositionSample3f, PreliminaryIntersection3f, Ray3f, RayFlags, Receiver, RectLight, SurfaceInteraction3f, allreduce_gradient,
                    bounce_lighting, bounce_rays, caustic_film, caustic_filter_mass, caustic_lighting, caustic_rays,
                    dielectric_lighting, direct_lighting, envmap_lighting, envmap_rays, film_gaussian, glossy_lighting, glossy_rays,
                    point_lighting, rect_lighting, rect_rays, reflection_lighting, reflection_rays, refraction_lighting, reparameterize_ray, reparameterize_ray_adjoint, reparameterize_ray_tangent,
                    sky_lighting, sky_rays)
from .sensor import OrthographicCamera, PerspectiveCamera, ThinLensCamera  # noqa: F401
from .projector import Projector, projector_lighting, projector_rays  # noqa: F401
from .spot import SpotLight, spot_lighting, spot_rays  # noqa: F401
from .directional import DirectionalLight, directional_lighting, directional_rays  # noqa: F401
from .normalmap import NormalMap  # noqa: F401
from .bumpmap import BumpMap  # noqa: F401
from .specular import specular_lighting  # noqa: F401
from .medium import Medium, medium_attenuation, medium_lighting, medium_rays  # noqa: F401
