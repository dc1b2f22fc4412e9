"""ctypes binding of include/hf.h (the C ABI of libhf.so).  No torch types cross
this boundary: device pointers are passed as integers (tensor.data_ptr())."""
import ctypes as C
import os

from . import build as _build

HF_OK, HF_EINVAL, HF_EDEVICE, HF_ENOMEM, HF_EFLAGS = 0, 1, 2, 3, 4
HF_ATTR_VERTEX, HF_ATTR_FACE = 0, 1

_fp = C.c_void_p  # device pointers


class hf_desc_t(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("max_height", C.c_float),
                ("to_world", C.c_float * 12), ("to_object", C.c_float * 12),
                ("has_to_object", C.c_int32), ("flip_normals", C.c_int32), ("device", C.c_int32)]


class hf_rays_t(C.Structure):
    _fields_ = [("o", _fp * 3), ("d", _fp * 3), ("maxt", _fp)]


class hf_pi_t(C.Structure):
    _fields_ = [("t", _fp), ("prim_uv", _fp * 2), ("prim_index", _fp)]


class hf_si_t(C.Structure):
    _fields_ = [("t", _fp), ("p", _fp * 3), ("n", _fp * 3), ("uv", _fp * 2), ("sh_n", _fp * 3),
                ("dp_du", _fp * 3), ("dp_dv", _fp * 3), ("boundary_test", _fp),
                ("sh_s", _fp * 3), ("sh_t", _fp * 3), ("wi", _fp * 3)]


class hf_si_grad_t(C.Structure):
    _fields_ = [("t", _fp), ("p", _fp * 3), ("n", _fp * 3), ("uv", _fp * 2), ("sh_n", _fp * 3),
                ("dp_du", _fp * 3), ("dp_dv", _fp * 3)]


class hf_si_tangent_t(C.Structure):
    _fields_ = [("t", _fp), ("p", _fp * 3), ("n", _fp * 3), ("uv", _fp * 2), ("sh_n", _fp * 3),
                ("dp_du", _fp * 3), ("dp_dv", _fp * 3)]


class hf_position_sample_t(C.Structure):
    _fields_ = [("p", _fp * 3), ("n", _fp * 3), ("uv", _fp * 2), ("pdf", _fp), ("prim_index", _fp), ("b", _fp * 2)]


# every symbol include/hf.h declares: name -> (restype, argtypes)
HF_MAX_LIGHTS = 8


class hf_dir_light_t(C.Structure):
    _fields_ = [("to_light", C.c_float * 3), ("irradiance", C.c_float)]


class hf_receiver_t(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("ex", C.c_float * 3), ("ey", C.c_float * 3)]


_caustic_in = [C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp]  # p, nrm, sh_n, d, t, active
# sh_n, d, t, active, weight, eta, W, H, data, rot
_reflect_in = [C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, _fp, C.c_float, C.c_uint32, C.c_uint32, _fp, C.POINTER(C.c_float * 9)]
# alpha, eta, num_rays, seed, ray_id, W, H, data, rot
_glossy_mid = [_fp, C.c_float, C.c_uint32, C.c_uint32, _fp, C.c_uint32, C.c_uint32, _fp, C.POINTER(C.c_float * 9)]
_glossy_in = [C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, _fp, *_glossy_mid]  # sh_n, d, t, active, weight, ...
HF_WRAP_CLAMP, HF_WRAP_REPEAT = 0, 1
_bitmap_in = [C.c_uint32, C.c_uint32, _fp, C.c_int]  # TW, TH, tex, wrap
_refract_mid = [_fp, C.c_float, C.c_float, C.POINTER(hf_receiver_t), *_bitmap_in]  # weight, eta, sigma_t, receiver, ...


class hf_rect_light_t(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("ex", C.c_float * 3), ("ey", C.c_float * 3), ("radiance", C.c_float)]


# weight, num_rays, seed, ray_id, light, TW, TH, tex, albedo
_rect_mid = [_fp, C.c_uint32, C.c_uint32, _fp, C.POINTER(hf_rect_light_t), C.c_uint32, C.c_uint32, _fp, C.c_float]
_rect_in = [C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp]  # n, spp, p, sh_n, d, t

HF_SENSOR_PERSPECTIVE, HF_SENSOR_ORTHOGRAPHIC = 0, 1


class hf_sensor_t(C.Structure):
    _fields_ = [("type", C.c_int32), ("film_w", C.c_uint32), ("film_h", C.c_uint32), ("crop_x", C.c_uint32),
                ("crop_y", C.c_uint32), ("crop_w", C.c_uint32), ("crop_h", C.c_uint32), ("to_world", C.c_double * 12),
                ("x_fov", C.c_double), ("near_clip", C.c_double), ("far_clip", C.c_double)]


_sensor_in = [C.POINTER(hf_sensor_t), C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, _fp]  # sensor, n, start, spp, seed, ray_id
_project_in = [C.POINTER(hf_sensor_t), C.c_size_t, C.POINTER(_fp * 3), _fp]  # sensor, n, p, active

HF_THINLENS_PAIR = 0x4C454E53


class hf_thinlens_t(C.Structure):
    _fields_ = [("base", hf_sensor_t), ("aperture_radius", C.c_double), ("focus_distance", C.c_double)]


_lens_in = [C.POINTER(hf_thinlens_t), *_sensor_in[1:]]  # lens, n, start, spp, seed, ray_id
# lens, n, start, seed, ray_id, p, active
_lens_project_in = [C.POINTER(hf_thinlens_t), C.c_size_t, C.c_uint32, C.c_uint32, _fp, C.POINTER(_fp * 3), _fp]

class hf_projector_t(C.Structure):
    _fields_ = [("to_world", C.c_double * 12), ("x_fov", C.c_double), ("scale", C.c_float)]


# n, spp, p, sh_n, d, t, weight, projector, TW, TH, tex, wrap, albedo, vis
_projector_in = [C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp,
                 C.POINTER(hf_projector_t), *_bitmap_in, C.c_float, _fp]

class hf_spot_light_t(C.Structure):
    _fields_ = [("to_world", C.c_double * 12), ("intensity", C.c_float), ("cutoff_angle", C.c_float), ("beam_width", C.c_float)]


HF_SPOT_PARAMS = 15
# n, spp, p, sh_n, d, t, weight, n_lights, lights, albedo, vis
_spot_in = [C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, C.c_uint32,
            C.POINTER(hf_spot_light_t), C.c_float, _fp]

class hf_directional_light_t(C.Structure):
    _fields_ = [("to_light", C.c_double * 3), ("irradiance", C.c_float)]


HF_DIRECTIONAL_PARAMS = 4
# n, spp, sh_n, d, t, weight, n_lights, lights, albedo, vis
_directional_in = [C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, C.c_uint32,
                   C.POINTER(hf_directional_light_t), C.c_float, _fp]

# n, spp, sh_n, d, weight, alpha, eta, n_lights, lights, vis
_specular_in = [C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, C.c_float, C.c_uint32,
                C.POINTER(hf_directional_light_t), _fp]

class hf_medium_t(C.Structure):
    _fields_ = [("top_origin", C.c_double * 3), ("top_normal", C.c_double * 3), ("sigma_t", C.c_float), ("albedo", C.c_float),
                ("g", C.c_float)]


HF_MEDIUM_PARAMS = 3
# n, spp, o, d, t, weight, medium, n_lights, lights, num_steps, seed, ray_id, vis_bits
_medium_in = [C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, C.POINTER(hf_medium_t), C.c_uint32,
              C.POINTER(hf_directional_light_t), C.c_uint32, C.c_uint32, _fp, _fp]

# n, uv, sh_n, dp_du, active, TW, TH, tex, wrap
_normalmap_in =[C.c_size_t, C.POINTER(_fp * 2), C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, *_bitmap_in]
# n, uv, sh_n, n_geo, dp_du, dp_dv, active, TW, TH, tex, wrap, scale
_bumpmap_in = [C.c_size_t, C.POINTER(_fp * 2), C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp,
               *_bitmap_in, C.c_float]

SYMBOLS = {
    # ..., out_n, mask
    "hf_bumpmap_eval": (C.c_int, [*_bumpmap_in, C.POINTER(_fp * 3), _fp, C.c_void_p]),
    # ..., dtex, duv, dsh_n, ddp_du, ddp_dv, dout_n
    "hf_bumpmap_eval_tangent": (C.c_int, [*_bumpmap_in, _fp, C.POINTER(_fp * 2), C.POINTER(_fp * 3), C.POINTER(_fp * 3),
                                          C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.c_void_p]),
    # ..., grad_out, grad_tex, grad_uv, grad_sh_n, grad_dp_du, grad_dp_dv
    "hf_bumpmap_eval_adjoint": (C.c_int, [*_bumpmap_in, C.POINTER(_fp * 3), _fp, C.POINTER(_fp * 2), C.POINTER(_fp * 3),
                                          C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.c_void_p]),
    # n, o, d, t, medium, light, k, seed, ray_id, out_o, out_d, out_maxt
    "hf_medium_rays": (C.c_int, [C.c_size_t, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.POINTER(hf_medium_t),
                                 C.POINTER(hf_directional_light_t), C.c_uint32, C.c_uint32, _fp, C.POINTER(_fp * 3),
                                 C.POINTER(_fp * 3), _fp, C.c_void_p]),
    # hf, n, spp, o, d, t, weight, medium, n_lights, lights, num_steps, seed, ray_id, image, value, vis_bits
    "hf_medium_lighting": (C.c_int, [C.c_void_p, *_medium_in[:-1], _fp, _fp, _fp, C.c_void_p]),
    "hf_medium_workspace_floats": (C.c_size_t, [C.c_uint32]),
    # ..., grad_image, grad_value, grad_weight, grad_t, grad_params, workspace
    "hf_medium_lighting_adjoint": (C.c_int, [*_medium_in, _fp, _fp, _fp, _fp, _fp, _fp, C.c_void_p]),
    # ..., dweight, dt, d_params, dimage, dvalue
    "hf_medium_lighting_tangent": (C.c_int, [*_medium_in, _fp, _fp, _fp, _fp, _fp, C.c_void_p]),
    # ..., out_n, mask
    "hf_normalmap_eval": (C.c_int, [*_normalmap_in, C.POINTER(_fp * 3), _fp, C.c_void_p]),
    # ..., dtex, duv, dsh_n, ddp_du, dout_n
    "hf_normalmap_eval_tangent": (C.c_int, [*_normalmap_in, _fp, C.POINTER(_fp * 2), C.POINTER(_fp * 3), C.POINTER(_fp * 3),
                                            C.POINTER(_fp * 3), C.c_void_p]),
    # ..., grad_out, grad_tex, grad_uv, grad_sh_n, grad_dp_du
    "hf_normalmap_eval_adjoint": (C.c_int, [*_normalmap_in, C.POINTER(_fp * 3), _fp, C.POINTER(_fp * 2), C.POINTER(_fp * 3),
                                            C.POINTER(_fp * 3), C.c_void_p]),
    "hf_directional_rays": (C.c_int, [C.c_size_t, C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3),
                                      _fp, C.POINTER(hf_directional_light_t), C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp,
                                      C.c_void_p]),
    "hf_directional_lighting": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3),
                                          C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, C.c_uint32,
                                          C.POINTER(hf_directional_light_t), C.c_float, _fp, _fp, _fp, C.c_void_p]),
    "hf_directional_workspace_floats": (C.c_size_t, [C.c_uint32]),
    # ..., grad_image, grad_value, grad_sh_n, grad_weight, grad_lights, workspace
    "hf_directional_lighting_adjoint": (C.c_int, [*_directional_in, _fp, _fp, C.POINTER(_fp * 3), _fp, _fp, _fp, C.c_void_p]),
    # ..., dsh_n, dweight, d_lights, dimage, dvalue
    "hf_directional_lighting_tangent": (C.c_int, [*_directional_in, C.POINTER(_fp * 3), _fp, _fp, _fp, _fp, C.c_void_p]),
    # ..., image, value
    "hf_specular_lighting": (C.c_int, [*_specular_in, _fp, _fp, C.c_void_p]),
    "hf_specular_workspace_floats": (C.c_size_t, [C.c_uint32]),
    # ..., grad_image, grad_value, grad_sh_n, grad_weight, grad_alpha, grad_lights, workspace
    "hf_specular_lighting_adjoint": (C.c_int, [*_specular_in, _fp, _fp, C.POINTER(_fp * 3), _fp, _fp, _fp, _fp, C.c_void_p]),
    # ..., dsh_n, dweight, dalpha, d_lights, dimage, dvalue
    "hf_specular_lighting_tangent": (C.c_int, [*_specular_in, C.POINTER(_fp * 3), _fp, _fp, _fp, _fp, _fp, C.c_void_p]),
    "hf_spot_rays": (C.c_int, [C.c_size_t, C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp,
                               C.POINTER(hf_spot_light_t), C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.c_void_p]),
    "hf_spot_lighting": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3),
                                   C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, C.c_uint32, C.POINTER(hf_spot_light_t),
                                   C.c_float, _fp, _fp, _fp, C.c_void_p]),
    "hf_spot_workspace_floats": (C.c_size_t, [C.c_uint32]),
    # ..., grad_image, grad_value, grad_sh_n, grad_p, grad_weight, grad_lights, workspace
    "hf_spot_lighting_adjoint": (C.c_int, [*_spot_in, _fp, _fp, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, _fp, C.c_void_p]),
    # ..., dsh_n, dp, dweight, d_lights, dimage, dvalue
    "hf_spot_lighting_tangent": (C.c_int, [*_spot_in, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, _fp, _fp, C.c_void_p]),
    "hf_projector_rays": (C.c_int, [C.c_size_t, C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp,
                                    C.POINTER(hf_projector_t), C.c_uint32, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3),
                                    _fp, C.c_void_p]),
    "hf_projector_lighting": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3),
                                        C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, C.POINTER(hf_projector_t), *_bitmap_in,
                                        C.c_float, _fp, _fp, _fp, C.POINTER(_fp * 2), C.c_void_p]),
    "hf_projector_workspace_floats": (C.c_size_t, []),
    # ..., grad_image, grad_value, grad_sh_n, grad_p, grad_weight, grad_tex, grad_to_world, grad_fov, grad_scale, workspace
    "hf_projector_lighting_adjoint": (C.c_int, [*_projector_in, _fp, _fp, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, _fp,
                                                _fp, _fp, _fp, C.c_void_p]),
    # ..., dsh_n, dp, dweight, dtex, d_to_world, d_fov, d_scale, dimage, dvalue
    "hf_projector_lighting_tangent": (C.c_int, [*_projector_in, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, _fp, _fp, _fp,
                                                _fp, _fp, C.c_void_p]),
    "hf_thinlens_rays": (C.c_int, [*_lens_in, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.POINTER(_fp * 2), C.c_void_p]),
    "hf_thinlens_rays_tangent": (C.c_int, [*_lens_in, _fp, _fp, _fp, _fp, C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.c_void_p]),
    "hf_thinlens_workspace_floats": (C.c_size_t, []),
    "hf_thinlens_rays_adjoint": (C.c_int, [*_lens_in, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, _fp, _fp, _fp,
                                           C.c_void_p]),
    "hf_thinlens_project": (C.c_int, [*_lens_project_in, C.POINTER(_fp * 2), _fp, _fp, C.c_void_p]),
    "hf_thinlens_project_tangent": (C.c_int, [*_lens_project_in, C.POINTER(_fp * 3), _fp, _fp, _fp, _fp, C.POINTER(_fp * 2),
                                              _fp, C.c_void_p]),
    "hf_thinlens_project_adjoint": (C.c_int, [*_lens_project_in, C.POINTER(_fp * 2), _fp, C.POINTER(_fp * 3), _fp, _fp, _fp,
                                              _fp, _fp, C.c_void_p]),
    "hf_sensor_rays": (C.c_int, [*_sensor_in, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.POINTER(_fp * 2), C.c_void_p]),
    "hf_sensor_rays_tangent": (C.c_int, [*_sensor_in, _fp, _fp, C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.c_void_p]),
    "hf_sensor_workspace_floats": (C.c_size_t, []),
    "hf_sensor_rays_adjoint": (C.c_int, [*_sensor_in, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, _fp, C.c_void_p]),
    "hf_sensor_project": (C.c_int, [*_project_in, C.POINTER(_fp * 2), _fp, _fp, C.c_void_p]),
    "hf_sensor_project_tangent": (C.c_int, [*_project_in, C.POINTER(_fp * 3), _fp, _fp, C.POINTER(_fp * 2), _fp, C.c_void_p]),
    "hf_sensor_project_adjoint": (C.c_int, [*_project_in, C.POINTER(_fp * 2), _fp, C.POINTER(_fp * 3), _fp, _fp, _fp, C.c_void_p]),
    "hf_create": (C.c_int, [C.POINTER(hf_desc_t), C.POINTER(C.c_void_p)]),
    "hf_destroy": (C.c_int, [C.c_void_p]),
    "hf_capture_reset": (C.c_int, [C.c_void_p]),
    "hf_set_ray_coherence": (C.c_int, [C.c_void_p, C.c_int]),
    "hf_get_ray_coherence": (C.c_int, [C.c_void_p]),
    "hf_set_heights": (C.c_int, [C.c_void_p, _fp, C.c_void_p]),
    "hf_set_heights_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hf_adam_step": (C.c_int, [C.c_void_p, _fp, _fp, _fp, _fp, C.c_double, C.c_double, C.c_double, C.c_double,
                               C.c_uint32, C.c_int, C.c_void_p]),
    "hf_adam_lr_t": (C.c_float, [C.c_double, C.c_double, C.c_double, C.c_uint32]),
    "hf_adam_step_scheduled": (C.c_int, [C.c_void_p, _fp, _fp, _fp, _fp, _fp, _fp, C.c_double, C.c_double, C.c_double, C.c_int,
                                         C.c_void_p]),
    "hf_set_transform": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "hf_set_face_normals": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "hf_get_face_normals": (C.c_int, [C.c_void_p]),
    "hf_shading_derivatives": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(hf_pi_t), _fp, C.POINTER(_fp * 3),
                                         C.POINTER(_fp * 3), C.c_void_p]),
    "hf_set_area_sampling": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "hf_surface_area": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "hf_area_cdf": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "hf_sample_position": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(_fp * 2), _fp, C.POINTER(hf_position_sample_t),
                                     C.c_void_p]),
    "hf_sample_position_adjoint": (C.c_int, [C.c_void_p, C.c_size_t, _fp, C.POINTER(_fp * 2), _fp, C.POINTER(_fp * 3),
                                             C.POINTER(_fp * 3), _fp, C.c_void_p]),
    "hf_sample_position_tangent": (C.c_int, [C.c_void_p, C.c_size_t, _fp, C.POINTER(_fp * 2), _fp, _fp, C.POINTER(_fp * 3),
                                             C.POINTER(_fp * 3), C.c_void_p]),
    "hf_sample_position_adjoint_transform": (C.c_int, [C.c_void_p, C.c_size_t, _fp, C.POINTER(_fp * 2), _fp,
                                                       C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, C.c_void_p]),
    "hf_sample_position_tangent_transform": (C.c_int, [C.c_void_p, C.c_size_t, _fp, C.POINTER(_fp * 2), _fp, _fp, _fp,
                                                       C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.c_void_p]),
    "hf_eval_attribute": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, _fp, _fp, C.POINTER(_fp * 3), _fp, _fp,
                                    C.POINTER(_fp * 3), C.c_void_p]),
    "hf_eval_attribute_adjoint": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, _fp, _fp, C.POINTER(_fp * 3), _fp,
                                            _fp, C.POINTER(_fp * 3), _fp, C.POINTER(_fp * 3), _fp, C.c_void_p]),
    "hf_eval_attribute_tangent": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, _fp, _fp, C.POINTER(_fp * 3), _fp,
                                            _fp, _fp, C.POINTER(_fp * 3), _fp, C.POINTER(_fp * 3), C.c_void_p]),
    "hf_eval_parameterization": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(_fp * 2), C.c_uint32, _fp, C.POINTER(hf_si_t),
                                           _fp, C.c_void_p]),
    "hf_eval_parameterization_adjoint": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(_fp * 2), C.c_uint32, _fp,
                                                   C.POINTER(hf_si_grad_t), _fp, _fp, C.c_void_p]),
    "hf_eval_parameterization_tangent": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(_fp * 2), C.c_uint32, _fp, _fp, _fp,
                                                   C.POINTER(hf_si_tangent_t), C.c_void_p]),
    "hf_bbox": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "hf_heights_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "hf_dims": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "hf_ray_intersect_preliminary": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(hf_rays_t), _fp,
                                               C.POINTER(hf_pi_t), C.c_void_p]),
    "hf_ray_test": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(hf_rays_t), _fp, _fp, C.c_void_p]),
    "hf_compute_surface_interaction": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(hf_rays_t),
                                                 C.POINTER(hf_pi_t), C.c_uint32, _fp,
                                                 C.POINTER(hf_si_t), C.c_void_p]),
    "hf_ray_intersect": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(hf_rays_t), C.c_uint32, _fp,
                                   C.POINTER(hf_pi_t), C.POINTER(hf_si_t), C.c_void_p]),
    "hf_adjoint": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(hf_rays_t), C.POINTER(hf_pi_t),
                             C.c_uint32, _fp, C.POINTER(hf_si_grad_t), _fp,
                             C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.c_void_p]),
    "hf_adjoint_rows": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(hf_rays_t), C.POINTER(hf_pi_t),
                             C.c_uint32, _fp, C.POINTER(hf_si_grad_t), _fp,
                             C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.c_void_p, C.c_void_p]),
    "hf_tangent": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(hf_rays_t), C.POINTER(hf_pi_t), C.c_uint32, _fp, _fp,
                             C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(hf_si_tangent_t), C.c_void_p]),
    "hf_adjoint_transform": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(hf_rays_t), C.POINTER(hf_pi_t), C.c_uint32, _fp,
                                       C.POINTER(hf_si_grad_t), _fp, C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.c_void_p, _fp,
                                       C.c_void_p]),
    "hf_tangent_transform": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(hf_rays_t), C.POINTER(hf_pi_t), C.c_uint32, _fp,
                                       _fp, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.POINTER(hf_si_tangent_t),
                                       C.c_void_p]),
    "hf_direct_lighting": (C.c_int, [C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.c_uint32,
                                     C.POINTER(hf_dir_light_t), C.c_float, C.POINTER(_fp), _fp, C.c_void_p]),
    "hf_direct_lighting_adjoint": (C.c_int, [C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp,
                                             C.c_uint32, C.POINTER(hf_dir_light_t), C.c_float, C.POINTER(_fp), _fp,
                                             C.POINTER(_fp * 3), C.c_void_p]),
    "hf_direct_lighting_weighted": (C.c_int, [C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp,
                                              C.c_uint32, C.POINTER(hf_dir_light_t), C.c_float, C.POINTER(_fp), _fp,
                                              C.c_void_p]),
    "hf_direct_lighting_weighted_adjoint": (C.c_int, [C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp,
                                                      _fp, C.c_uint32, C.POINTER(hf_dir_light_t), C.c_float,
                                                      C.POINTER(_fp), _fp, C.POINTER(_fp * 3), _fp, C.c_void_p]),
    "hf_direct_lighting_weighted_tangent": (C.c_int, [C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp,
                                                      _fp, C.c_uint32, C.POINTER(hf_dir_light_t), C.c_float,
                                                      C.POINTER(_fp), C.POINTER(_fp * 3), _fp, _fp, C.c_void_p]),
    "hf_point_lighting": (C.c_int, [C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.POINTER(_fp * 3),
                                    C.c_uint32, C.POINTER(hf_dir_light_t), C.c_float, C.POINTER(_fp), _fp, C.c_void_p]),
    "hf_point_lighting_adjoint": (C.c_int, [C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp,
                                            C.POINTER(_fp * 3), C.c_uint32, C.POINTER(hf_dir_light_t), C.c_float,
                                            C.POINTER(_fp), _fp, C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.c_void_p]),
    "hf_point_lighting_tangent": (C.c_int, [C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp,
                                            C.POINTER(_fp * 3), C.c_uint32, C.POINTER(hf_dir_light_t), C.c_float,
                                            C.POINTER(_fp), C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.c_void_p]),
    "hf_sky_rays": (C.c_int, [C.c_size_t, C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp,
                              C.c_uint32, C.c_uint32, _fp, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.c_void_p]),
    "hf_sky_lighting": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3),
                                  C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, C.c_uint32, C.c_uint32, _fp, C.c_float,
                                  C.c_float, _fp, _fp, C.c_void_p]),
    "hf_sky_lighting_adjoint": (C.c_int, [C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp,
                                          C.c_uint32, C.c_uint32, _fp, C.c_float, C.c_float, _fp, _fp, C.POINTER(_fp * 3),
                                          _fp, C.c_void_p]),
    "hf_sky_lighting_tangent": (C.c_int, [C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp,
                                          C.c_uint32, C.c_uint32, _fp, C.c_float, C.c_float, _fp, C.POINTER(_fp * 3), _fp,
                                          _fp, C.c_void_p]),
    "hf_caustic_rays": (C.c_int, [C.c_size_t, *_caustic_in, C.c_float, C.POINTER(hf_receiver_t), C.POINTER(_fp * 3),
                                  C.POINTER(_fp * 3), _fp, C.c_void_p]),
    "hf_caustic_lighting": (C.c_int, [C.c_void_p, C.c_size_t, *_caustic_in, _fp, C.c_float, C.c_float,
                                      C.POINTER(hf_receiver_t), C.POINTER(_fp * 2), _fp, _fp, C.c_void_p]),
    "hf_caustic_adjoint": (C.c_int, [C.c_size_t, *_caustic_in, _fp, C.c_float, C.c_float, C.POINTER(hf_receiver_t), _fp,
                                     C.POINTER(_fp * 2), _fp, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.c_void_p]),
    "hf_caustic_tangent": (C.c_int, [C.c_size_t, *_caustic_in, _fp, C.c_float, C.c_float, C.POINTER(hf_receiver_t), _fp,
                                     C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.POINTER(_fp * 2), _fp, C.c_void_p]),
    "hf_reflect_rays": (C.c_int, [C.c_size_t, *_caustic_in, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.c_void_p]),
    "hf_reflect_lighting": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, *_caustic_in, _fp, C.c_float, C.c_uint32, C.c_uint32,
                                      _fp, C.POINTER(C.c_float * 9), _fp, _fp, _fp, C.c_void_p]),
    "hf_reflect_lighting_adjoint": (C.c_int, [C.c_size_t, C.c_uint32, *_reflect_in, _fp, _fp, _fp, C.POINTER(_fp * 3), _fp, _fp,
                                              C.c_void_p]),
    "hf_reflect_lighting_tangent": (C.c_int, [C.c_size_t, C.c_uint32, *_reflect_in, _fp, C.POINTER(_fp * 3), _fp, _fp, _fp, _fp,
                                              C.c_void_p]),
    "hf_glossy_rays": (C.c_int, [C.c_size_t, *_caustic_in, _fp, C.c_uint32, C.c_uint32, _fp, C.POINTER(_fp * 3),
                                 C.POINTER(_fp * 3), _fp, C.POINTER(_fp * 3), C.c_void_p]),
    "hf_glossy_lighting": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, *_caustic_in, _fp, *_glossy_mid, _fp, _fp, _fp,
                                     C.c_void_p]),
    "hf_glossy_lighting_adjoint": (C.c_int, [C.c_size_t, C.c_uint32, *_glossy_in, _fp, _fp, _fp, C.POINTER(_fp * 3), _fp, _fp,
                                             _fp, C.c_void_p]),
    "hf_glossy_lighting_tangent": (C.c_int, [C.c_size_t, C.c_uint32, *_glossy_in, _fp, C.POINTER(_fp * 3), _fp, _fp, _fp, _fp,
                                             _fp, C.c_void_p]),
    "hf_bitmap_eval": (C.c_int, [C.c_size_t, C.POINTER(_fp * 2), _fp, *_bitmap_in, _fp, C.POINTER(_fp * 2), C.c_void_p]),
    "hf_bitmap_eval_adjoint": (C.c_int, [C.c_size_t, C.POINTER(_fp * 2), _fp, *_bitmap_in, _fp, C.POINTER(_fp * 2), _fp,
                                         C.c_void_p]),
    "hf_refract_lighting": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, *_caustic_in, *_refract_mid, _fp, _fp, _fp,
                                      C.POINTER(_fp * 2), C.c_void_p]),
    "hf_refract_lighting_adjoint": (C.c_int, [C.c_size_t, C.c_uint32, *_caustic_in, *_refract_mid, _fp, _fp, _fp,
                                              C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, C.c_void_p]),
    "hf_refract_lighting_tangent": (C.c_int, [C.c_size_t, C.c_uint32, *_caustic_in, *_refract_mid, _fp, C.POINTER(_fp * 3),
                                              C.POINTER(_fp * 3), _fp, _fp, _fp, _fp, C.c_void_p]),
    "hf_rect_light_geometry": (C.c_int, [C.POINTER(hf_rect_light_t), C.POINTER(C.c_float), C.POINTER(C.c_float * 3)]),
    "hf_rect_rays": (C.c_int, [C.c_size_t, C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp,
                               C.c_uint32, C.c_uint32, _fp, C.POINTER(hf_rect_light_t), C.POINTER(_fp * 3), C.POINTER(_fp * 3),
                               _fp, C.c_void_p]),
    "hf_rect_lighting": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3),
                                   C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, *_rect_mid, _fp, _fp, C.c_void_p]),
    "hf_rect_lighting_adjoint": (C.c_int, [*_rect_in, *_rect_mid, _fp, _fp, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp,
                                           C.c_void_p]),
    "hf_rect_lighting_tangent": (C.c_int, [*_rect_in, *_rect_mid, _fp, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, _fp,
                                           C.c_void_p]),
    "hf_envmap_table_floats":(C.c_size_t, [C.c_uint32, C.c_uint32]),
    "hf_envmap_build_table": (C.c_int, [C.c_uint32, C.c_uint32, _fp, C.c_float, _fp, C.c_void_p]),
    "hf_envmap_sample_direction": (C.c_int, [C.c_size_t, C.POINTER(_fp * 2), C.c_uint32, C.c_uint32, _fp, _fp,
                                             C.POINTER(C.c_float * 9), C.POINTER(_fp * 3), _fp, _fp, _fp, C.POINTER(_fp * 2),
                                             C.c_void_p]),
    "hf_envmap_eval": (C.c_int, [C.c_size_t, C.POINTER(_fp * 3), _fp, C.c_uint32, C.c_uint32, _fp, C.POINTER(C.c_float * 9),
                                 _fp, C.c_void_p]),
    "hf_envmap_eval_adjoint": (C.c_int, [C.c_size_t, C.POINTER(_fp * 3), _fp, C.c_uint32, C.c_uint32,
                                         C.POINTER(C.c_float * 9), _fp, _fp, C.c_void_p]),
    "hf_envmap_rays": (C.c_int, [C.c_size_t, C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3),
                                 _fp, C.c_uint32, C.c_uint32, _fp, C.c_uint32, C.c_uint32, _fp, _fp,
                                 C.POINTER(C.c_float * 9), C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, C.c_void_p]),
    "hf_envmap_lighting": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3),
                                     C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, C.c_uint32, C.c_uint32, _fp,
                                     C.c_uint32, C.c_uint32, _fp, _fp, C.POINTER(C.c_float * 9), C.c_float, _fp, _fp,
                                     C.c_void_p]),
    "hf_envmap_lighting_adjoint": (C.c_int, [C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp,
                                             C.c_uint32, C.c_uint32, _fp, C.c_uint32, C.c_uint32, _fp, _fp,
                                             C.POINTER(C.c_float * 9), C.c_float, _fp, _fp, C.POINTER(_fp * 3), _fp, _fp,
                                             C.c_void_p]),
    "hf_envmap_lighting_tangent": (C.c_int, [C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp,
                                             C.c_uint32, C.c_uint32, _fp, C.c_uint32, C.c_uint32, _fp, _fp,
                                             C.POINTER(C.c_float * 9), C.c_float, _fp, C.POINTER(_fp * 3), _fp, _fp, _fp,
                                             C.c_void_p]),
    "hf_large_steps_workspace_floats": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "hf_large_steps_apply": (C.c_int, [C.c_uint32, C.c_uint32, C.c_double, _fp, _fp, C.c_void_p]),
    "hf_large_steps_solve": (C.c_int, [C.c_uint32, C.c_uint32, C.c_double, _fp, _fp, C.c_int, C.c_uint32, C.c_float, _fp, _fp,
                                       C.c_void_p]),
    "hf_bounce_rays": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.POINTER(_fp * 3),
                                 C.POINTER(_fp * 3), _fp, C.c_uint32, C.c_uint32, _fp, C.POINTER(C.c_float * 3),
                                 C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.c_void_p]),
    "hf_bounce_lighting": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3),
                                     C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, _fp, C.c_uint32, C.c_uint32, _fp,
                                     C.c_uint32, C.POINTER(hf_dir_light_t), C.c_float, _fp, _fp, _fp, C.c_size_t,
                                     C.c_void_p]),
    "hf_bounce_lighting_adjoint": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp,
                                             _fp, C.c_uint32, C.c_uint32, _fp, C.c_uint32, C.POINTER(hf_dir_light_t),
                                             C.c_float, _fp, _fp, C.c_size_t, _fp, C.POINTER(_fp * 3), _fp, _fp,
                                             C.c_void_p]),
    "hf_bounce_lighting_tangent": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp,
                                             _fp, C.c_uint32, C.c_uint32, _fp, C.c_uint32, C.POINTER(hf_dir_light_t),
                                             C.c_float, _fp, _fp, C.c_size_t, C.POINTER(_fp * 3), _fp, _fp, _fp,
                                             C.c_void_p]),
    "hf_film_splat": (C.c_int, [C.c_size_t, C.c_uint32, C.POINTER(_fp), _fp, _fp, C.c_uint32, C.c_uint32, C.c_float, _fp, _fp,
                                C.c_void_p]),
    "hf_film_splat_adjoint": (C.c_int, [C.c_size_t, C.c_uint32, _fp, _fp, C.c_uint32, C.c_uint32, C.c_float, _fp,
                                        C.POINTER(_fp), C.c_void_p]),
    "hf_film_splat_weighted": (C.c_int, [C.c_size_t, C.c_uint32, C.POINTER(_fp), _fp, _fp, _fp, C.c_uint32, C.c_uint32,
                                         C.c_float, _fp, _fp, C.c_void_p]),
    "hf_film_splat_weighted_adjoint": (C.c_int, [C.c_size_t, C.c_uint32, C.POINTER(_fp), _fp, _fp, _fp, C.c_uint32,
                                                 C.c_uint32, C.c_float, _fp, _fp, C.POINTER(_fp), _fp, _fp, _fp,
                                                 C.c_void_p]),
    "hf_film_splat_weighted_tangent": (C.c_int, [C.c_size_t, C.c_uint32, C.POINTER(_fp), _fp, _fp, _fp, C.c_uint32,
                                                 C.c_uint32, C.c_float, C.POINTER(_fp), _fp, _fp, _fp, _fp, _fp,
                                                 C.c_void_p]),
    "hf_reparam_aux_rays": (C.c_int, [C.c_size_t, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.c_uint32, C.c_float,
                                      C.c_int, C.c_uint32, C.c_void_p, C.POINTER(_fp * 3), _fp, C.c_void_p]),
    "hf_reparam_weights": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.c_uint32,
                                     C.c_float, C.c_float, C.c_int, C.c_uint32, C.c_void_p, _fp, C.POINTER(_fp * 3), _fp, _fp,
                                     C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.POINTER(_fp * 3), _fp,
                                     C.POINTER(_fp * 3), C.c_void_p]),
    "hf_reparam_trace": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.c_uint32, C.c_float,
                                   C.c_int, C.c_uint32, C.c_void_p, C.POINTER(hf_pi_t), C.POINTER(hf_si_t), C.c_void_p]),
    "hf_reparam_trace_all": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.c_uint32, C.c_float,
                                       C.c_int, C.c_uint32, C.c_void_p, C.POINTER(hf_pi_t), C.POINTER(hf_si_t), C.c_size_t, C.c_void_p]),
    "hf_reparam_backward": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.c_uint32,
                                      C.c_float, C.c_float, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, _fp, C.c_size_t,
                                      C.POINTER(_fp * 3), _fp, _fp, C.c_void_p]),
    "hf_reparam_tangent": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.c_uint32,
                                     C.c_float, C.c_float, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, _fp, C.c_size_t,
                                     _fp, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.POINTER(_fp * 3), _fp, C.c_void_p]),
    "hf_reparam_backward_full": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(_fp * 3), C.POINTER(_fp * 3), _fp, C.c_uint32,
                                           C.c_float, C.c_float, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, _fp,
                                           C.c_size_t, C.POINTER(_fp * 3), _fp, _fp, C.POINTER(_fp * 3),
                                           C.POINTER(_fp * 3), _fp, C.c_void_p]),
    "hf_ray_intersect_preliminary_packet": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3),
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_fp * 2), C.c_void_p]),
    "hf_ray_test_packet": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(_fp * 3), C.POINTER(_fp * 3), C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "hf_allreduce_grad": (C.c_int, [_fp, C.c_size_t, C.c_void_p, C.c_void_p]),
    "hf_num_levels": (C.c_int, [C.c_void_p]),
    "hf_get_mip": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint32),
                             C.POINTER(C.c_uint32)]),
    "hf_get_node_level": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]),
    "hf_invert_affine": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "hf_grid_blocks": (C.c_int, [C.c_size_t, C.c_int]),
    "hf_last_error_string": (C.c_char_p, []),
    "hf_version": (C.c_int, []),
}

_lib = None


class HfError(RuntimeError):
    """Raised for a non-zero status from libhf (the adapter's Throw(...))."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def lib():
    """Load libhf.so; fails loudly if it is missing -- there is no fallback path."""
    global _lib
    if _lib is None:
        # HF_LIB: another build of the SAME library (scripts/vb.sh variants for A/B measurements), never a fallback
        path = os.environ.get("HF_LIB") or _build.LIB_PATH
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: build it with `python __graft_entry__.py` (hipcc, gfx950). "
                "This package has no CPU/eager fallback.")
        L = C.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != HF_OK:
        raise HfError(rc, lib().hf_last_error_string().decode())
