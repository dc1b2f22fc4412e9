"""The transform derivatives end to end: the silhouette of a translated heightfield through reparameterize_ray (the
visibility-discontinuous case that Discontinuous is about, modelled on tests/test_silhouette_gradient.py), and pose
recovery by Adam on a translation plus yaw (examples/inverse_pose.py)."""
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def _translate_z(th):
    import torch
    one, z = torch.ones_like(th), torch.zeros_like(th)
    return torch.stack([torch.stack([one, z, z, z]), torch.stack([z, one, z, z]), torch.stack([z, z, one, th])])


def _render_sum(hf, sg, h, rays, spp, tz):
    import torch
    shape = hf.Heightfield(heightfield=h, max_height=0.5, to_world=[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, tz]])
    ray = hf.Ray3f(rays[0:3].contiguous(), rays[3:6].contiguous(), rays[6].contiguous())
    with torch.no_grad():
        return float(sg.f_of(shape.ray_intersect(ray, hf.RayFlags.All)).double().sum()) / spp


def _gradient(hf, sg, h, rays, spp, aux=32, kappa=1e5, reparam=True):
    """dL/dtz at tz = 0 by reverse mode through to_world"""
    import torch
    shape = hf.Heightfield(heightfield=h.clone(), max_height=0.5, differentiable_to_world=True)
    th = torch.zeros((), dtype=torch.float64, requires_grad=True)
    shape.to_world = _translate_z(th)
    shape.parameters_changed(["to_world"])
    ray = hf.Ray3f(rays[0:3].contiguous(), rays[3:6].contiguous(), rays[6].contiguous())
    if reparam:
        d, det = hf.reparameterize_ray(shape, ray, num_rays=aux, kappa=kappa)
    else:
        d, det = ray.d, torch.ones(len(ray), device=h.device)
    si = shape.ray_intersect(hf.Ray3f(ray.o, d, ray.maxt), hf.RayFlags.All)
    ((sg.f_of(si) * det).sum() / spp).backward()
    return float(th.grad)


def test_translated_silhouette_through_reparameterisation(hf):
    """the field of examples/silhouette_gradient.py (a box ridge seen obliquely along +y) lifted by to_world's
    translation: the silhouette of the ridge's top edge moves over the field behind it in the image.  (A translation
    along y is a poor probe with this orthographic camera: it only shifts the image, and its derivative, -3.3, is the
    small difference of an attached term of -975 from the ridge's steep walls and a silhouette term of about +972.)
    Measured on an MI355X: FD 10200.6, attached only 8802.1 (0.863 of FD), reparameterised with 32 auxiliary rays
    10251.7 (1.005 of FD; 16 auxiliary rays at kappa 2e4: 0.998)."""
    import torch
    import silhouette_gradient as sg
    dev = torch.device("cuda")
    film, spp, eps = 160, 64, 0.01
    h, _ = sg.scene(device=dev)
    rays = sg.camera(film, spp, dev)
    fd = (_render_sum(hf, sg, h, rays, spp, eps) - _render_sum(hf, sg, h, rays, spp, -eps)) / (2 * eps)
    g_att = _gradient(hf, sg, h, rays, spp, reparam=False)
    g32 = _gradient(hf, sg, h, rays, spp, aux=32, kappa=1e5)
    print(f"translate along z: FD {fd:.3f}, attached only {g_att:.3f}, reparameterised (32 aux) {g32:.3f}")
    assert abs(fd) > 0
    assert abs(g_att - fd) > 0.1 * abs(fd), (g_att, fd)         # the attached gradient alone is clearly off
    assert abs(g32 - fd) < 0.03 * abs(fd), (g32, fd)
    assert abs(g32 - fd) < abs(g_att - fd)


def test_inverse_pose_recovers_translation_and_yaw():
    """150 Adam steps from (0.08, -0.06, 6 degrees) to the identity pose.  Measured on an MI355X: recovered to
    (2.9e-5, -1.5e-5) object units and 0.0014 degrees, loss 9.85e-4 -> 8.6e-11."""
    import torch
    import inverse_pose as ip
    assert torch.cuda.is_available()
    target, start, final, losses = ip.recover(steps=150)
    err0 = max(abs(start[0] - target[0]), abs(start[1] - target[1]))
    err = max(abs(final[0] - target[0]), abs(final[1] - target[1]))
    yaw_err = abs(final[2] - target[2])
    print(f"pose: start {start}, recovered {final}, loss {losses[0]:.3e} -> {losses[-1]:.3e}")
    assert losses[-1] < 1e-3 * losses[0], (losses[0], losses[-1])
    assert err < 5e-4 and err < 0.01 * err0, (final, target)          # translation, object units (a cell: 7.8e-3)
    assert yaw_err < math.radians(0.02), (math.degrees(yaw_err), final)
