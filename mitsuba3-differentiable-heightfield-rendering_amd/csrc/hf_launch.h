// hf_launch.h -- host-side launch entry points implemented in hf_kernels.hip
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>
#include "../../include/hf.h"
#include "hf_device.h"

void hf_launch_build_mips(const hf_dev_field &f, float2 *mip, float4 *shear, hipStream_t stream);
// scratch block a trace launch needs (its work counters; the launcher zeroes it): hf_trace_scratch_bytes(n)
// bytes, exclusively this launch's until it has completed
size_t hf_trace_scratch_bytes(size_t n);
// mode 0: closest hit -> pi; 1: any hit -> hit; 2: closest hit + fused surface interaction
struct hf_reparam_args;
// aux (mode 2 only, may be NULL): trace auxiliary ray aux->k of every ray (k, seed, kappa, antithetic are read)
void hf_launch_trace(int mode, const hf_dev_field &f, size_t n, const hf_rays_t *rays, const uint8_t *active,
                     const hf_pi_t *pi, uint8_t *hit, const hf_si_t *si, uint32_t flags, void *scratch,
                     hipStream_t stream, const hf_reparam_args *aux = nullptr, bool lean = false, // lean: the launch is declared incoherent (hf_set_ray_coherence)
                     const float4 *vn = nullptr); // vn (mode 2): the handle's vertex normals = smooth shading
// vn (here and below): the handle's vertex normals when it shades smoothly (hf_set_face_normals), NULL = flat shading
void hf_launch_si(const hf_dev_field &f, size_t n, const hf_rays_t *rays, const hf_pi_const_t *pi,
                  const uint8_t *active, const hf_si_t *si, uint32_t flags, hipStream_t stream, const float4 *vn = nullptr);
void hf_launch_adjoint(const hf_dev_field &f, size_t n, const hf_rays_t *rays, const hf_pi_const_t *pi,
                       const uint8_t *active, const hf_si_grad_t *gs, uint32_t flags, float *grad_h,
                       float *const grad_o[3], float *const grad_d[3], uint32_t *row_band, hipStream_t stream,
                       const float4 *vn = nullptr, float *grad_to_world = nullptr, void *slab = nullptr);
// grad_to_world (12 device floats, accumulated; hf_adjoint_transform, hf_sample_position_adjoint_transform): the launch
// also writes its blocks' partial sums to `slab`, hf_xform_slab_bytes(n) bytes that no other pending launch may use,
// and adds them up.  hf_xform_slab_bytes(0): the most any launch needs.
size_t hf_xform_slab_bytes(size_t n);
// forward mode of compute_si (hf_tangent): dh / d_o / d_d may be NULL (zero tangents); d_to_world (12 device floats,
// hf_tangent_transform): the tangent of to_world, NULL = zero
void hf_launch_tangent(const hf_dev_field &f, size_t n, const hf_rays_t *rays, const hf_pi_const_t *pi,
                       const uint8_t *active, uint32_t flags, const float *dh, const float *const d_o[3],
                       const float *const d_d[3], const hf_si_tangent_t *out, hipStream_t stream, const float4 *vn = nullptr,
                       const float *d_to_world = nullptr);
// smooth shading: the vertex normals of the current heights and transform into vn (W H float4)
void hf_launch_build_normals(const hf_dev_field &f, float4 *vn, hipStream_t stream);
// hf_shading_derivatives: dn_du / dn_dv rows (NULL rows are not written); vn NULL = flat shading = zeros
void hf_launch_shading_derivatives(const hf_dev_field &f, size_t n, const hf_pi_const_t *pi, const uint8_t *active,
                                   float *const dn_du[3], float *const dn_dv[3], const float4 *vn, hipStream_t stream);
// c1 = (float)(1 - beta1), c2 = (float)(1 - beta2): the differences are Python doubles in optimizers.py:279-280,
// rounded once when they meet the float32 gradient
hipError_t hf_launch_adam(size_t n, float *h, const float *g, float *m, float *v, float lr_t, float beta1, float beta2,
                    float c1, float c2, float eps, int mask_updates, hipStream_t stream,
                    uint32_t *uniform_scratch = nullptr, const float *sched = nullptr, uint32_t *ctr = nullptr); // non-NULL: the UniformAdam variant (one device word of scratch)
struct hf_lights_dev {
    float l[HF_MAX_LIGHTS][3];
    float w[HF_MAX_LIGHTS]; // albedo/pi * irradiance
    const uint8_t *vis[HF_MAX_LIGHTS];
    uint32_t n;
    const float *weight;  // optional per-sample factor of every light's contribution (hf_direct_lighting_weighted)
    float *grad_weight;   // adjoint, optional: dL/dweight per sample
};
// p == nullptr: directional lights (lights.l = unit direction towards the light, lights.w = albedo/pi * irradiance);
// p != nullptr: point lights (lights.l = position, lights.w = albedo/pi * intensity), grad_p is then written too
void hf_launch_direct(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3], const float *t,
                      const float *const p[3], const hf_lights_dev &lights, float *image, hipStream_t stream);
void hf_launch_direct_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                              const float *t, const float *const p[3], const hf_lights_dev &lights,
                              const float *grad_image, float *const grad_sh_n[3], float *const grad_p[3],
                              hipStream_t stream);
// forward mode of the two above: dsh_n, dp (point lights only), dweight (directional only) may be NULL (zero)
void hf_launch_direct_tangent(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                              const float *t, const float *const p[3], const hf_lights_dev &lights,
                              const float *const dsh_n[3], const float *const dp[3], const float *dweight, float *dimage,
                              hipStream_t stream);
// ---- sky lighting (hf_sky_rays, hf_sky_lighting / _adjoint / _tangent): the one argument of its four kernels ----
struct hf_sky_args {
    hf_dev_field f;                          // forward only (the walk)
    size_t n;
    uint32_t spp, num_rays, seed, k;         // k: hf_sky_rays' direction
    float scale;                             // 4 albedo radiance / num_rays
    const float *p[3], *nrm[3];              // si.p, si.n (forward, rays)
    const float *sh_n[3], *d[3], *t, *weight;
    const uint32_t *ray_id;                  // optional: the id of sample i in the sample streams (NULL: i)
    float *image;                            // forward: image; tangent: dimage
    uint32_t *vis_bits;                      // forward: written (NULL: not wanted); adjoint, tangent: read
    float *out_o[3], *out_d[3], *out_maxt;   // rays
    const float *gimg; float *gn[3], *gw;    // adjoint
    const float *dn[3], *dw;                 // tangent inputs (NULL: zero)
};
// mode 0: forward, 1: adjoint, 2: tangent, 3: rays.  The forward launch is the per-lane any-hit walk with the samples
// drawn in the kernel: no work counter, no scratch block
void hf_launch_sky(int mode, const hf_sky_args &a, hipStream_t stream);
// ---- refractive caustics (hf_caustic_rays, hf_caustic_lighting / _adjoint / _tangent): the one argument of its four kernels ----
struct hf_caustic_args {
    hf_dev_field f;                          // forward only (the walk)
    size_t n;
    float eta, rcp_eta, power;               // rcp_eta = 1 / eta, rounded once on the host
    float origin[3], ex[3], ey[3], N[3];     // the receiver; N = normalize(ex x ey)
    const float *p[3], *nrm[3], *sh_n[3], *d[3], *t, *weight;
    const uint8_t *active;                   // optional (NULL: every lane)
    float *pos[2], *value;                   // forward: written; tangent: dpos, dvalue
    uint8_t *vis;                            // forward: written (NULL: not wanted); adjoint, tangent: read
    float *out_o[3], *out_d[3], *out_maxt;   // rays
    const float *gpos[2], *gvalue;           // adjoint inputs (NULL: zero)
    float *gn[3], *gp[3], *gw;               // adjoint outputs (NULL: not wanted)
    const float *dn[3], *dp[3], *dw;         // tangent inputs (NULL: zero)
};
// mode 0: forward, 1: adjoint, 2: tangent, 3: rays.  The forward launch is hf_launch_sky's: the per-lane any-hit walk,
// no work counter, no scratch block
void hf_launch_caustic(int mode, const hf_caustic_args &a, hipStream_t stream);
// ---- environment-map lighting (hf_envmap_*): the one argument of its kernels; data and table are the caller's ----
struct hf_envmap_args {
    hf_dev_field f;                          // forward only (the walk)
    size_t n;
    uint32_t spp, num_rays, seed, k;         // k: hf_envmap_rays' direction
    uint32_t W, H;                           // texels per row (the seam column included), rows
    float scale;                             // albedo / (pi num_rays)
    float rot[9];                            // row-major rotation, map space -> world (identity for NULL)
    const float *data, *table;               // [H][W] radiance; hf_envmap_table_floats(W, H) floats
    const float *p[3], *nrm[3];              // si.p, si.n (forward, rays)
    const float *sh_n[3], *d[3], *t, *weight; // d: the camera ray's direction; hf_envmap_eval: the directions to look up
    const uint32_t *ray_id;                  // optional: the id of sample i in the sample streams (NULL: i)
    float *image;                            // forward: image; tangent: dimage
    uint32_t *vis_bits;                      // forward: written (NULL: not wanted); adjoint, tangent: read
    float *out_o[3], *out_d[3], *out_maxt;   // rays; out_d: sample_direction too
    float *out_weight, *out_pdf;             // rays (optional), sample_direction
    uint32_t *out_cell;                      // sample_direction (optional)
    float *out_frac[2];                      // sample_direction (optional): the position (fx, fy) in the cell
    const float *gimg; float *gn[3], *gw;    // adjoint
    float *gdata;                            // adjoint, eval_adjoint: accumulated (lighting adjoint: NULL = not wanted)
    const float *dn[3], *dw, *ddata;         // tangent inputs (NULL: zero)
    const float *sample[2];                  // sample_direction
    const uint8_t *active;                   // eval, eval_adjoint (NULL: every lane)
    float *out; const float *gout;           // eval: values; eval_adjoint: dL/dvalue
};
// mode 0: forward, 1: adjoint, 2: tangent, 3: rays, 4: sample_direction, 5: eval, 6: eval_adjoint.  The forward launch
// is hf_launch_sky's: the per-lane any-hit walk, no work counter, no scratch block
void hf_launch_envmap(int mode, const hf_envmap_args &a, hipStream_t stream);
// ---- specular reflection of the environment map (hf_reflect_rays, hf_reflect_lighting / _adjoint / _tangent): the one
// argument of its four kernels; W, H, rot as in hf_envmap_args (env_lookup reads either) ----
struct hf_reflect_args {
    hf_dev_field f;                          // forward only (the walk)
    size_t n;
    uint32_t spp, W, H;
    float eta, rcp_eta;                      // rcp_eta = 1 / eta, rounded once on the host (0 for the mirror, eta = 0)
    float rot[9];                            // row-major rotation, map space -> world (identity for NULL)
    const float *data;                       // [H][W] radiance
    const float *p[3], *nrm[3];              // si.p, si.n (forward, rays)
    const float *sh_n[3], *d[3], *t, *weight;
    const uint8_t *active;                   // optional (NULL: every lane)
    float *image, *value;                    // forward: written (NULL: not wanted); tangent: dimage, dvalue
    uint8_t *vis;                            // forward: written (NULL: not wanted); adjoint, tangent: read
    float *out_o[3], *out_d[3], *out_maxt;   // rays
    const float *gimg, *gvalue;              // adjoint inputs (NULL: zero)
    float *gn[3], *gw, *gdata;               // adjoint outputs (NULL: not wanted); gdata is accumulated
    const float *dn[3], *dw, *ddata;         // tangent inputs (NULL: zero)
};
// mode 0: forward, 1: adjoint, 2: tangent, 3: rays.  The forward launch is hf_launch_sky's: the per-lane any-hit walk,
// no work counter, no scratch block
void hf_launch_reflect(int mode, const hf_reflect_args &a, hipStream_t stream);
// ---- glossy reflection of the environment map (hf_glossy_rays, hf_glossy_lighting / _adjoint / _tangent): the one
// argument of its four kernels; eta, rcp_eta as in hf_reflect_args (reflect_vertex reads either), W, H, rot as in
// hf_envmap_args ----
struct hf_glossy_args {
    hf_dev_field f;                          // forward only (the walk)
    size_t n;
    uint32_t spp, num_rays, seed, k;         // k: hf_glossy_rays' direction
    uint32_t W, H;
    float eta, rcp_eta;                      // rcp_eta = 1 / eta, rounded once on the host (0 for eta = 0: F = 1)
    float inv_k;                             // 1 / num_rays, rounded once on the host
    float rot[9];                            // row-major rotation, map space -> world (identity for NULL)
    const float *data;                       // [H][W] radiance
    const float *p[3], *nrm[3];              // si.p, si.n (forward, rays)
    const float *sh_n[3], *d[3], *t, *weight, *alpha;
    const uint8_t *active;                   // optional (NULL: every lane)
    const uint32_t *ray_id;                  // optional: the id of sample i in the sample streams (NULL: i)
    float *image, *value;                    // forward: written (NULL: not wanted); tangent: dimage, dvalue
    uint32_t *vis_bits;                      // forward: written (NULL: not wanted); adjoint, tangent: read
    float *out_o[3], *out_d[3], *out_maxt;   // rays
    float *out_h[3];                         // rays (optional): the microfacet normal
    const float *gimg, *gvalue;              // adjoint inputs (NULL: zero)
    float *gn[3], *gw, *ga, *gdata;          // adjoint outputs (NULL: not wanted); gdata is accumulated
    const float *dn[3], *dw, *da, *ddata;    // tangent inputs (NULL: zero)
};
// mode 0: forward, 1: adjoint, 2: tangent, 3: rays.  The forward launch is hf_launch_sky's: the per-lane any-hit walk,
// no work counter, no scratch block
void hf_launch_glossy(int mode, const hf_glossy_args &a, hipStream_t stream);
// ---- the refraction view (hf_refract_lighting / _adjoint / _tangent): the one argument of its three kernels; eta,
// rcp_eta, the receiver and the rows under hf_caustic_args' names (caustic_vertex reads either), TW, TH, wrap as in
// hf_bitmap_args (bitmap_cell reads either) ----
struct hf_refract_args {
    hf_dev_field f;                          // forward only (the walk)
    size_t n;
    uint32_t spp, TW, TH;
    int32_t wrap;                            // HF_WRAP_CLAMP / HF_WRAP_REPEAT
    float eta, rcp_eta, sigma_t;             // rcp_eta = 1 / eta, rounded once on the host
    float origin[3], ex[3], ey[3], N[3];     // the receiver; N = normalize(ex x ey)
    const float *tex;                        // [TH][TW]
    const float *p[3], *nrm[3], *sh_n[3], *d[3], *t, *weight;
    const uint8_t *active;                   // optional (NULL: every lane)
    float *image, *value;                    // forward: written (NULL: not wanted); tangent: dimage, dvalue
    uint8_t *vis;                            // forward: written (NULL: not wanted); adjoint, tangent: read
    float *pos[2];                           // forward: written (NULL: not wanted)
    const float *gimg, *gvalue;              // adjoint inputs (NULL: zero)
    float *gn[3], *gp[3], *gw, *gdata;       // adjoint outputs (NULL: not wanted); gdata (the texels') is accumulated
    const float *dn[3], *dp[3], *dw, *ddata; // tangent inputs (NULL: zero); ddata: the texels'
};
// mode 0: forward, 1: adjoint, 2: tangent.  The forward launch is hf_launch_sky's: the per-lane any-hit walk, no work
// counter, no scratch block
void hf_launch_refract(int mode, const hf_refract_args &a, hipStream_t stream);
// ---- the plane texture alone (hf_bitmap_eval / _adjoint) ----
struct hf_bitmap_args {
    size_t n;
    uint32_t TW, TH;
    int32_t wrap;
    const float *tex, *pos[2];
    const uint8_t *active;                   // optional (NULL: every lane)
    float *out, *out_grad[2];                // eval: L and (optional) Lx, Ly
    const float *gout;                       // adjoint: dL/dvalue
    float *gpos[2], *gtex;                   // adjoint outputs (NULL: not wanted); gtex is accumulated
};
void hf_launch_bitmap(bool adjoint, const hf_bitmap_args &a, hipStream_t stream);
// ---- the normal map (hf_normalmap_eval / _tangent / _adjoint): the one argument of its three kernels; TW, TH, wrap as
// in hf_bitmap_args (bitmap_cell reads either); tex is PLANAR, plane k at tex + k TW TH ----
struct hf_normalmap_args {
    size_t n;
    uint32_t TW, TH;
    int32_t wrap;
    const float *tex;                        // [3][TH][TW]
    const float *uv[2], *sh_n[3], *dp_du[3];
    const uint8_t *active;                   // optional (NULL: every lane)
    float *out_n[3];                         // forward: N; tangent: dN
    uint8_t *mask;                           // forward: written (NULL: not wanted)
    const float *dtex, *duv[2], *dn[3], *dp[3]; // tangent inputs (NULL: zero); dtex: the texels', planar
    const float *gout[3];                    // adjoint input: dL/dN
    float *gtex, *guv[2], *gn[3], *gp[3];    // adjoint outputs (NULL: not wanted); gtex is accumulated
};
// mode 0: forward, 1: adjoint, 2: tangent; one lane per sample, no grid stride, no scratch block
void hf_launch_normalmap(int mode, const hf_normalmap_args &a, hipStream_t stream);
// ---- the bump map (hf_bumpmap_eval / _tangent / _adjoint): the one argument of its three kernels; TW, TH, wrap as in
// hf_bitmap_args (bitmap_cell reads either); tex is ONE plane, exactly a hf_bitmap_eval texture ----
struct hf_bumpmap_args {
    size_t n;
    uint32_t TW, TH;
    int32_t wrap;
    float scale;                             // the gradient's multiplier (finite)
    const float *tex;                        // [TH][TW]
    const float *uv[2], *sh_n[3], *n_geo[3], *dp_du[3], *dp_dv[3];
    const uint8_t *active;                   // optional (NULL: every lane)
    float *out_n[3];                         // forward: N; tangent: dN
    uint8_t *mask;                           // forward: written (NULL: not wanted)
    const float *dtex, *duv[2], *dn[3], *dpu[3], *dpv[3]; // tangent inputs (NULL: zero); dtex: the texels'
    const float *gout[3];                    // adjoint input: dL/dN
    float *gtex, *guv[2], *gn[3], *gpu[3], *gpv[3]; // adjoint outputs (NULL: not wanted); gtex is accumulated
};
// mode 0: forward, 1: adjoint, 2: tangent; one lane per sample, no grid stride, no scratch block
void hf_launch_bumpmap(int mode, const hf_bumpmap_args &a, hipStream_t stream);
// ---- area-light lighting (hf_rect_rays, hf_rect_lighting / _adjoint / _tangent): the one argument of its four kernels;
// TW, TH, wrap as in hf_bitmap_args (bitmap_cell reads either) ----
struct hf_rect_args {
    hf_dev_field f;                          // forward only (the walk)
    size_t n;
    uint32_t spp, num_rays, seed, k;         // k: hf_rect_rays' draw
    uint32_t TW, TH;                         // 0, 0 without a texture
    int32_t wrap;                            // HF_WRAP_CLAMP (the lamp's texture has no other)
    float scale;                             // albedo radiance A / (pi num_rays), A = 4 |ex x ey|, rounded once on the host
    float center[3], ex[3], ey[3], nl[3];    // the lamp; nl = normalize(ex x ey), for the ray's masks
    double nld[3];                           // the same normal before its rounding to float, for the shading sums
    const float *tex;                        // [TH][TW], NULL: the lamp is uniform
    const float *p[3], *nrm[3];              // si.p (every mode), si.n (forward, rays)
    const float *sh_n[3], *d[3], *t, *weight;
    const uint32_t *ray_id;                  // optional: the id of sample i in the sample streams (NULL: i)
    float *image;                            // forward: image; tangent: dimage
    uint32_t *vis_bits;                      // forward: written (NULL: not wanted); adjoint, tangent: read
    float *out_o[3], *out_d[3], *out_maxt;   // rays
    const float *gimg;                       // adjoint input
    float *gn[3], *gp[3], *gw, *gdata;       // adjoint outputs (NULL: not wanted); gdata (the texels') is accumulated
    const float *dn[3], *dp[3], *dw, *ddata; // tangent inputs (NULL: zero); ddata: the texels'
};
// mode 0: forward, 1: adjoint, 2: tangent, 3: rays.  The forward launch is hf_launch_sky's: the per-lane any-hit walk,
// no work counter, no scratch block
void hf_launch_rect(int mode, const hf_rect_args &a, hipStream_t stream);
// ---- the sensor (hf_sensor_rays / _tangent / _adjoint): the one argument of its kernels; every constant is formed on
// the host in double, so it is wave-uniform ----
struct hf_sensor_args {
    size_t n;
    uint32_t start, spp, seed, crop_w, crop_x, crop_y;
    int32_t spp_shift, crop_w_shift;         // log2 where spp / crop_w is a power of two, else -1 (a division)
    uint32_t head, wide_mask;                // the 16-byte store variant only (set by the launcher): samples before the
                                             // first aligned group; the rows that share out_o[0]'s alignment
    double film_w, film_h, aspect;           // aspect = film_w / film_h
    double A[9], c[3];                       // to_world = [A | c]
    double near, tau, dtau;                  // tau = tan(x_fov pi / 360), dtau = (pi / 360) (1 + tau^2); orthographic: 1, 0
    double span;                             // far - near
    double An[3];                            // orthographic: A e_z near
    double dz[3], inv_len_z;                 // orthographic: d = A e_z / |A e_z| and 1 / |A e_z|
    const uint32_t *ray_id;                  // optional: the wavefront index of sample i (NULL: start + i)
    float *out_o[3], *out_d[3], *out_maxt;   // forward; tangent: out_do, out_dd
    float *out_pos[2];                       // forward, optional
    const float *d_tw, *d_fov;               // tangent inputs (NULL: zero)
    const float *go[3], *gd[3];              // adjoint inputs (NULL rows: zero)
    double *slab;                            // adjoint: 13 doubles per block
    float *g_tw, *g_fov;                     // adjoint outputs, accumulated (NULL: not wanted)
};
// mode 0: rays, 1: adjoint (two launches: the blocks' partial sums, their sum), 2: tangent
void hf_launch_sensor(int mode, int type, const hf_sensor_args &a, hipStream_t stream);
size_t hf_sensor_slab_doubles();             // the most any adjoint launch needs
// ---- the way back (hf_sensor_project / _tangent / _adjoint; perspective only) ----
struct hf_sensor_project_args {
    size_t n;
    double Ai[9], c[3];                      // to_world^-1's linear part (formed on the host in double), to_world's c
    double near, far, tau, dtau, aspect;
    double film_w, film_h, crop_x, crop_y, crop_w, crop_h;
    double inv_area;                         // 1 / A', A' = (2 tau)^2 / a (crop_w crop_h) / (film_w film_h)
    const float *p[3];
    const uint8_t *active;                   // optional (NULL: every lane)
    float *uv[2], *weight;                   // forward: written (weight optional); tangent: duv, dweight
    uint8_t *valid;                          // forward
    const float *dp[3], *d_tw, *d_fov;       // tangent inputs (NULL: zero)
    const float *guv[2], *gweight;           // adjoint inputs (NULL: zero)
    float *gp[3];                            // adjoint output rows, overwritten (NULL: not wanted)
    double *slab;                            // adjoint: 13 doubles per block
    float *g_tw, *g_fov;                     // adjoint outputs, accumulated (NULL: not wanted)
};
// mode 0: forward, 1: adjoint (two launches), 2: tangent
void hf_launch_sensor_project(int mode, const hf_sensor_project_args &a, hipStream_t stream);
// ---- the thin lens (hf_thinlens_rays / _tangent / _adjoint): the perspective sensor's argument (its kernels'
// layout stays as it is) and the lens's own constants behind it ----
struct hf_thinlens_args {
    hf_sensor_args s;                        // as a perspective sensor's; slab: 15 doubles per block
    double radius, focus;                    // aperture_radius r, focus_distance f
    double lens_o;                           // r (1 - near / f): o_c = lens_o D + near v
    double maxt_scale;                       // (far - near) / f
    uint32_t key;                            // tea32(seed, HF_THINLENS_PAIR).v0 (set by the launcher)
    const float *d_radius, *d_focus;         // tangent inputs (NULL: zero)
    float *g_radius, *g_focus;               // adjoint outputs, accumulated (NULL: not wanted)
};
// mode 0: rays, 1: adjoint (two launches), 2: tangent
void hf_launch_thinlens(int mode, const hf_thinlens_args &a, hipStream_t stream);
size_t hf_thinlens_slab_doubles();
// ---- the way back (hf_thinlens_project / _tangent / _adjoint) ----
struct hf_thinlens_project_args {
    hf_sensor_project_args s;                // as hf_sensor_project's; slab: 15 doubles per block
    uint32_t start, seed;                    // the lane's aperture draw: wavefront index start + i, or ray_id[i]
    uint32_t key;                            // tea32(seed, HF_THINLENS_PAIR).v0 (set by the launcher)
    const uint32_t *ray_id;
    double radius, focus;
    const float *d_radius, *d_focus;
    float *g_radius, *g_focus;
};
void hf_launch_thinlens_project(int mode, const hf_thinlens_project_args &a, hipStream_t stream);
// ---- projector lighting (hf_projector_rays, hf_projector_lighting / _adjoint / _tangent): the one argument
// of its kernels; every constant of the mapping is formed on the host in double; TW, TH, wrap as in hf_bitmap_args
// (bitmap_cell reads either) ----
struct hf_projector_args {
    hf_dev_field f;                          // forward only (the walk)
    size_t n;
    uint32_t spp, TW, TH;                    // TW, TH: read for the aspect without a texture too
    int32_t wrap;                            // HF_WRAP_CLAMP / HF_WRAP_REPEAT
    double Ai[9], c[3];                      // to_world^-1's linear part (adjugate, in double), to_world's c
    double tau, dtau, aspect;                // tan(x_fov pi / 360), (pi / 360) (1 + tau^2), TW / TH
    double albedo, cs;                       // cs = albedo scale
    float cf[3];                             // c rounded to float32: what the shadow ray takes
    const float *tex;                        // [TH][TW], NULL: uniform irradiance 1
    const float *p[3], *nrm[3];              // si.p (every mode), si.n (forward, rays)
    const float *sh_n[3], *d[3], *t, *weight;
    float *image, *value;                    // forward: written (NULL: not wanted); tangent: dimage, dvalue
    uint8_t *vis;                            // forward: written (NULL: not wanted); adjoint, tangent: read
    float *uv[2];                            // forward: written (NULL: not wanted)
    float *out_o[3], *out_d[3], *out_maxt;   // rays
    const float *gimg, *gvalue;              // adjoint inputs (NULL: zero)
    float *gn[3], *gp[3], *gw, *gdata;       // adjoint outputs (NULL: not wanted); gdata (the texels') is accumulated
    double *slab;                            // adjoint: 14 doubles per block (NULL: no reduced gradient is wanted)
    float *g_tw, *g_fov, *g_scale;           // adjoint outputs, accumulated (NULL: not wanted)
    const float *dn[3], *dp[3], *dw, *ddata; // tangent inputs (NULL: zero); ddata: the texels'
    const float *d_tw, *d_fov, *d_scale;     // tangent inputs: 12, 1, 1 device floats (NULL: zero)
};
// mode 0: forward, 1: adjoint (two launches where a reduced gradient is wanted), 2: tangent, 3: rays.  The forward launch
// is hf_launch_sky's: the per-lane any-hit walk, no work counter, no scratch block
void hf_launch_projector(int mode, const hf_projector_args &a, hipStream_t stream);
size_t hf_projector_slab_doubles();
// ---- spot lighting (hf_spot_rays, hf_spot_lighting / _adjoint / _tangent): a rig of up to HF_MAX_LIGHTS
// cone emitters in one launch.  One light of the rig, every constant formed on the host in double ----
struct hf_spot_light_dev {
    double Ai[9], c[3];                      // to_world^-1's linear part (adjugate, in double), to_world's c
    double cutoff, beam;                     // radians
    double cos_cutoff, cos_beam;
    double inv_width;                        // 1 / (cutoff - beam); 0 for a hard edge (cutoff == beam: there is no zone)
    double ci;                               // albedo / pi * intensity
    float cf[3], pad;                        // c rounded to float32: what the shadow ray takes
};
struct hf_spot_args {
    hf_dev_field f;                          // forward only (the walk)
    size_t n;
    uint32_t spp, n_lights;
    double albedo_pi;                        // albedo / pi: d value / d intensity
    double atan_c[14];                       // spot_theta's constants: 10 coefficients, tan(pi / 8), pi / 4, pi / 2, pi
    hf_spot_light_dev L[HF_MAX_LIGHTS];      // the first n_lights are read
    const float *p[3], *nrm[3];              // si.p (every mode), si.n (forward, rays)
    const float *sh_n[3], *d[3], *t, *weight;
    float *image, *value;                    // forward: written, K rows each (NULL: not wanted); tangent: dimage, dvalue
    uint8_t *vis;                            // forward: written (NULL: not wanted); adjoint, tangent: read; bit k: light k
    float *out_o[3], *out_d[3], *out_maxt;   // rays (of light 0)
    const float *gimg, *gvalue;              // adjoint inputs, K rows each (NULL: zero)
    float *gn[3], *gp[3], *gw;               // adjoint outputs (NULL: not wanted)
    double *slab;                            // adjoint: per light, 15 doubles per block (NULL: grad_lights is not wanted)
    float *g_lights;                         // adjoint output [K][15], accumulated
    const float *dn[3], *dp[3], *dw;         // tangent inputs (NULL: zero)
    const float *d_lights;                   // tangent input [K][15] device floats (NULL: zero)
};
// mode 0: forward, 1: adjoint (two launches where grad_lights is wanted), 2: tangent, 3: rays.  The forward launch is
// hf_launch_sky's: the per-lane any-hit walk, no work counter, no scratch block
void hf_launch_spot(int mode, const hf_spot_args &a, hipStream_t stream);
size_t hf_spot_slab_doubles(uint32_t n_lights);
// ---- directional lighting (hf_directional_rays, hf_directional_lighting / _adjoint / _tangent): a rig of up
// to HF_MAX_LIGHTS distant emitters in one launch.  One light of the rig, every constant formed on the host in double ----
struct hf_directional_light_dev {
    double l[3];                             // to_light / |to_light|
    double inv_len;                          // 1 / |to_light|
    double ce;                               // albedo / pi * irradiance
    float lf[3], pad;                        // l rounded to float32: the shadow ray's direction, and what decides `traced`
};
struct hf_directional_args {
    hf_dev_field f;                          // forward only (the walk)
    size_t n;
    uint32_t spp, n_lights;
    double albedo_pi;                        // albedo / pi: d value / d irradiance
    hf_directional_light_dev L[HF_MAX_LIGHTS]; // the first n_lights are read
    const float *p[3], *nrm[3];              // si.p, si.n (forward, rays: the held shadow ray)
    const float *sh_n[3], *d[3], *t, *weight;
    float *image, *value;                    // forward: written, K rows each (NULL: not wanted); tangent: dimage, dvalue
    uint8_t *vis;                            // forward: written (NULL: not wanted); adjoint, tangent: read; bit k: light k
    float *out_o[3], *out_d[3], *out_maxt;   // rays (of light 0)
    const float *gimg, *gvalue;              // adjoint inputs, K rows each (NULL: zero)
    float *gn[3], *gw;                       // adjoint outputs (NULL: not wanted)
    double *slab;                            // adjoint: per light, 4 doubles per block (NULL: grad_lights is not wanted)
    float *g_lights;                         // adjoint output [K][4], accumulated
    const float *dn[3], *dw;                 // tangent inputs (NULL: zero)
    const float *d_lights;                   // tangent input [K][4] device floats (NULL: zero)
};
// mode 0: forward, 1: adjoint (two launches where grad_lights is wanted), 2: tangent, 3: rays.  The forward launch is
// hf_launch_sky's: the per-lane any-hit walk, no work counter, no scratch block
void hf_launch_directional(int mode, const hf_directional_args &a, hipStream_t stream);
size_t hf_directional_slab_doubles(uint32_t n_lights);
// ---- specular highlights (hf_specular_lighting / _adjoint / _tangent): the GGX lobe under the directional
// rig, for all lights in one launch; nothing is traced, the directional row's visibility byte is read.  The lights are
// hf_directional_light_dev with ce = irradiance (no albedo); eta, rcp_eta as in hf_reflect_args (reflect_vertex reads them) ----
struct hf_specular_args {
    size_t n;
    uint32_t spp, n_lights;
    float eta, rcp_eta;
    hf_directional_light_dev L[HF_MAX_LIGHTS]; // the first n_lights are read
    const float *sh_n[3], *d[3], *weight, *alpha;
    const uint8_t *vis;                      // read by every mode; bit k: light k
    float *image, *value;                    // forward: written, K rows each (NULL: not wanted); tangent: dimage, dvalue
    const float *gimg, *gvalue;              // adjoint inputs, K rows each (NULL: zero)
    float *gn[3], *gw, *ga;                  // adjoint outputs (NULL: not wanted)
    double *slab;                            // adjoint: per light, 4 doubles per block (NULL: grad_lights is not wanted)
    float *g_lights;                         // adjoint output [K][4], accumulated
    const float *dn[3], *dw, *da;            // tangent inputs (NULL: zero)
    const float *d_lights;                   // tangent input [K][4] device floats (NULL: zero)
};
// mode 0: forward, 1: adjoint (two launches where grad_lights is wanted), 2: tangent
void hf_launch_specular(int mode, const hf_specular_args &a, hipStream_t stream);
size_t hf_specular_slab_doubles(uint32_t n_lights);
// ---- homogeneous medium (hf_medium_rays, hf_medium_lighting / _adjoint / _tangent): single scattering in
// the half space below a top plane under the directional rig, the shadow rays of 1..32 points of every primary ray
// traced in the kernel.  The lights are hf_directional_light_dev with ce = irradiance; every constant formed on the host
// in double ----
struct hf_medium_args {
    hf_dev_field f;                          // forward only (the walk)
    size_t n;
    uint32_t spp, n_lights, num_steps, seed;
    uint32_t k;                              // rays: the point that is materialised (of light 0)
    uint32_t on;                             // bit j: light j shines into the medium, nu_j > 0
    double N[3], top_o[3];                   // the unit top normal and a point of the top plane: h = <o - top_o, N>
    double sigma_t, albedo, g;
    double inv_nu[HF_MAX_LIGHTS];            // 1 / <l_j, N> (0 where the light does not shine in)
    hf_directional_light_dev L[HF_MAX_LIGHTS]; // the first n_lights are read
    const float *o[3], *d[3], *t, *weight;
    const uint32_t *ray_id;
    float *image, *value;                    // forward: written, J rows each (NULL: not wanted); tangent: dimage, dvalue
    uint32_t *vis_bits;                      // forward: written, J rows (NULL: not wanted); adjoint, tangent: read; bit k: point k
    float *out_o[3], *out_d[3], *out_maxt;   // rays
    const float *gimg, *gvalue;              // adjoint inputs, J rows each (NULL: zero)
    float *gw, *gt;                          // adjoint outputs (NULL: not wanted)
    double *slab;                            // adjoint: HF_MEDIUM_SUMS doubles per block (NULL: grad_params is not wanted)
    float *g_params;                         // adjoint output [HF_MEDIUM_PARAMS + n_lights], accumulated
    const float *dw, *dt;                    // tangent inputs (NULL: zero)
    const float *d_params;                   // tangent input [HF_MEDIUM_PARAMS + n_lights] device floats (NULL: zero)
};
// mode 0: forward, 1: adjoint (two launches where grad_params is wanted), 2: tangent, 3: rays.  The forward launch is
// hf_launch_sky's: the per-lane any-hit walk, no work counter, no scratch block
void hf_launch_medium(int mode, const hf_medium_args &a, hipStream_t stream);
size_t hf_medium_slab_doubles(void);
// the sampling table of a map: three launches (row sums of the cell means, conditional rows, marginal + header)
void hf_launch_envmap_build(uint32_t W, uint32_t H, const float *data, float u, float *table, hipStream_t stream);
// ---- bounce lighting (hf_bounce_rays, hf_bounce_lighting / _adjoint / _tangent): the one argument of its kernels ----
struct hf_bounce_args {
    hf_dev_field f;                          // the walks (forward, rays) and the triangles of the record (adjoint, tangent)
    size_t n, sample_stride;                 // record of direction k of sample i at [k * sample_stride + i]
    uint32_t spp, num_rays, seed, k;         // k: hf_bounce_rays' direction
    uint32_t n_lights;
    int32_t shadow;                          // hf_bounce_rays: 0 = the bounce ray, 1 = the shadow ray towards l[0]
    float scale;                             // albedo / num_rays
    float l[HF_MAX_LIGHTS][3];               // unit directions towards the lights
    float w[HF_MAX_LIGHTS];                  // albedo/pi * irradiance
    const float *p[3], *nrm[3];              // si.p, si.n (forward, rays)
    const float *sh_n[3], *d[3], *t, *weight;
    const uint32_t *ray_id;                  // optional: the id of sample i in the sample streams (NULL: i)
    float *image;                            // forward: image; tangent: dimage
    uint32_t *hit_prim;                      // forward: written (NULL: not wanted); adjoint, tangent: read
    uint8_t *lit_bits;                       // the same
    float *out_o[3], *out_d[3], *out_maxt;   // rays
    const float *gimg; float *gn[3], *gw, *gh; // adjoint (gn rows, gw, gh: NULL = not wanted; gh accumulated)
    const float *dn[3], *dw, *dh;            // tangent inputs (NULL: zero)
};
// mode 0: forward, 1: adjoint, 2: tangent, 3: rays.  The forward launch is the per-lane closest-hit and any-hit walks
// with the samples drawn in the kernel: no work counter, no scratch block
void hf_launch_bounce(int mode, const hf_bounce_args &a, hipStream_t stream);
struct hf_splat_args {
    size_t n;
    uint32_t channels, width, height;
    float alpha, bias, radius; // -1 / (2 stddev^2), exp(alpha r^2), r
    const float *pos_x, *pos_y;
    const float *values[HF_MAX_LIGHTS];   // forward: per-channel sample values
    float *image, *weight;                // forward: accumulated [channels][H*W], [H*W]
    const float *grad_image;              // adjoint: dL/d(accumulated image) [channels][H*W]
    float *grad_values[HF_MAX_LIGHTS];    // adjoint: per-channel, overwritten
};
void hf_launch_film_splat(const hf_splat_args &a, bool adjoint, hipStream_t stream);
// hf_film_splat_weighted / _adjoint / _tangent: the film of samples that move and carry a weight.  s.image / s.weight
// are the planes the forward AND the tangent accumulate into (the tangent's dimage, dweight)
struct hf_film_motion_args {
    hf_splat_args s;                      // s.values: NULL rows where the caller gave none (adjoint, tangent)
    const float *sample_weight;           // NULL: 1
    const float *grad_weight;             // adjoint: dL/d(accumulated weight) [H*W], NULL: zero
    float *grad_sample_weight, *grad_pos_x, *grad_pos_y; // adjoint: overwritten, NULL: not wanted (as s.grad_values rows)
    const float *dvalues[HF_MAX_LIGHTS];  // tangent inputs, NULL: zero
    const float *dsample_weight, *dpos_x, *dpos_y;
};
// mode 0: forward, 1: adjoint, 2: tangent
void hf_launch_film_motion(int mode, const hf_film_motion_args &a, hipStream_t stream);
struct hf_reparam_args {
    size_t n;
    const float *o[3], *d[3];
    const uint8_t *active;
    uint32_t k, seed;
    uint32_t num; size_t stride;                      // hf_launch_trace: samples k .. k + num - 1 in one launch, sample j at [j * stride + i] (num <= 1: sample k only)
    const uint32_t *ray_id;                           // optional: the id of ray i in the sample streams (NULL: i)
    float kappa, exponent;
    int antithetic, mode;
    float *aux_d[3], *aux_maxt;                       // aux-ray generation
    const float *si_t, *si_p[3], *si_bt;              // auxiliary hit
    float *Z, *dZ[3];                                 // mode 0: accumulated, mode 1: read
    const float *g_dir[3], *g_div;                    // mode 1
    float *g_p[3], *g_t;                              // mode 1 outputs
    float *g_vd[3];                                   // mode 1, optional: gradient w.r.t. V_direct (ray gradients)
};
void hf_launch_reparam_aux(const hf_reparam_args &a, hipStream_t stream);
void hf_launch_reparam_weights(const hf_reparam_args &a, hipStream_t stream);
void hf_launch_reparam_backward(const hf_dev_field &f, const hf_reparam_args &a, uint32_t num_rays, size_t stride,
                                const hf_pi_const_t *pi, float *grad_h, hipStream_t stream);
// hf_reparam_tangent: a.active / seed / kappa / exponent / antithetic / ray_id / o / d / si_bt are read; dh, d_o, d_d
// (or single rows of them), d_to_world (12 device floats) may be NULL (zero tangents); out_dir / out_div overwritten
void hf_launch_reparam_tangent(const hf_dev_field &f, const hf_reparam_args &a, uint32_t num_rays, size_t stride,
                               const hf_pi_const_t *pi, const float *dh, const float *const d_o[3],
                               const float *const d_d[3], const float *d_to_world, float *const out_dir[3],
                               float *out_div, hipStream_t stream);
// hf_reparam_backward_full: a.g_dir / g_div and what hf_launch_reparam_tangent reads; grad_h, grad_o, grad_d,
// grad_to_world may each be NULL (not wanted).  grad_h, grad_to_world accumulated, grad_o / grad_d overwritten;
// slab (with grad_to_world): as for hf_launch_adjoint
void hf_launch_reparam_backward_full(const hf_dev_field &f, const hf_reparam_args &a, uint32_t num_rays, size_t stride,
                                     const hf_pi_const_t *pi, float *grad_h, float *const grad_o[3],
                                     float *const grad_d[3], float *grad_to_world, void *slab, hipStream_t stream);
// ---- area sampling (hf_set_area_sampling) ----
#define HF_AREA_CHUNK 2048 // cells per tile of the table build: one cell row, or a 2048-cell piece of one
#define HF_AREA_SEG 64     // CDF entries per entry of the coarse search table
// the handle's area table; all device buffers are owned by the handle, NULL cdf = sampling disabled
struct hf_area_table {
    float *cdf;          // [nseg * HF_AREA_SEG]: fp32 CDF of the m triangle areas, padded with +inf
    float *coarse;       // [nseg]: cdf[64 k + 63] (the last entry for the last segment)
    double *tile;        // [3 ntiles]: tile totals, then per tile (group base, offset within the group)
    uint32_t *tile_valid;// [2 ntiles]: first nonzero entry, last nonzero entry + 1 of every tile
    hf_area_info *info;  // the distribution's scalars
    uint32_t m, nseg, ncx, ntiles;
};
// rebuild the table from the current heights and transform: three launches, no inter-workgroup waits
void hf_launch_build_area(const hf_dev_field &f, const hf_area_table &t, hipStream_t stream);
void hf_launch_sample_position(const hf_dev_field &f, const hf_area_table &t, size_t n, const float *const sample[2],
                               const uint8_t *active, const hf_position_sample_t &out, const float4 *vn, hipStream_t stream);
void hf_launch_sample_position_adjoint(const hf_dev_field &f, size_t n, const uint32_t *prim, const float *const b[2],
                                       const uint8_t *active, const float *const gp[3], const float *const gn[3],
                                       float *grad_h, const float4 *vn, hipStream_t stream,
                                       float *grad_to_world = nullptr, void *slab = nullptr);
void hf_launch_sample_position_tangent(const hf_dev_field &f, size_t n, const uint32_t *prim, const float *const b[2],
                                       const uint8_t *active, const float *dh, float *const dp[3], float *const dn[3],
                                       const float4 *vn, hipStream_t stream, const float *d_to_world = nullptr);
// ---- shape attributes (hf_eval_attribute / _adjoint / _tangent): the buffers are the caller's ----
struct hf_attr_args {
    hf_dev_field f;
    size_t n;
    const float *attr;          // [count][size] interleaved (count: W H vertices or 2 (W-1)(H-1) faces)
    const uint32_t *prim;
    const float *p[3], *t;      // si.p (vertex attributes), si.t (NULL: every active lane is a hit)
    const uint8_t *active;
    float *out[3];              // forward: size rows, overwritten
    const float *g[3];          // adjoint: size rows of dL/dvalue
    float *grad_attr;           // adjoint, accumulated (NULL: not wanted)
    float *grad_p[3];           // adjoint, overwritten (NULL rows: not wanted)
    float *grad_h;              // adjoint, accumulated (NULL: not wanted)
    const float *dattr, *dp[3], *dh; // tangent inputs (NULL: zero)
    float *dout[3];             // tangent: size rows, overwritten
};
// mode 0: forward, 1: adjoint, 2: tangent; type HF_ATTR_VERTEX / HF_ATTR_FACE, size 1 or 3 (checked by the caller)
void hf_launch_attribute(int mode, int type, uint32_t size, const hf_attr_args &a, hipStream_t stream);
// ---- eval_parameterization (hf_eval_parameterization / _adjoint / _tangent): uv = 2 device rows of n floats ----
// forward: flags without HF_RAY_FOLLOWSHAPE (the caller's translation); prim_out may be NULL
void hf_launch_param(const hf_dev_field &f, size_t n, const float *const uv[2], const uint8_t *active, const hf_si_t *si,
                     uint32_t *prim_out, uint32_t flags, hipStream_t stream, const float4 *vn);
// adjoint / tangent: flags WITH HF_RAY_FOLLOWSHAPE; grad_to_world / slab as for hf_launch_adjoint, d_to_world as for
// hf_launch_tangent (NULL: none)
void hf_launch_param_adjoint(const hf_dev_field &f, size_t n, const float *const uv[2], const uint8_t *active,
                             const hf_si_grad_t *gs, uint32_t flags, float *grad_h, hipStream_t stream, const float4 *vn,
                             float *grad_to_world = nullptr, void *slab = nullptr);
void hf_launch_param_tangent(const hf_dev_field &f, size_t n, const float *const uv[2], const uint8_t *active,
                             uint32_t flags, const float *dh, const float *d_to_world, const hf_si_tangent_t *out,
                             hipStream_t stream, const float4 *vn);
// ---- large-steps preconditioning (hf_large_steps_*): A = I + lambda L on the vertex grid; the buffers are the caller's ----
size_t hf_large_steps_scratch_floats(uint32_t W, uint32_t H);
void hf_launch_large_steps_apply(uint32_t W, uint32_t H, double lambda, const float *v, float *u, hipStream_t stream);
// conjugate gradients, 2 max_iter + 3 launches whatever the data; no host synchronisation
void hf_launch_large_steps_solve(uint32_t W, uint32_t H, double lambda, const float *u, float *v, int warm, uint32_t max_iter,
                                 float rel_tol, float *workspace, float *info, hipStream_t stream);
