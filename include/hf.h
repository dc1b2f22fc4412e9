/*
 * hf.h -- C ABI of libhf: MI355X (gfx950) differentiable heightfield intersector.
 *
 * This is the drop-in boundary for the reference's Shape plugin interface on
 * the heightfield hot path.  A Mitsuba 3.3 `Shape`
 * subclass ("heightfield" plugin) forwards whole ray
 * wavefronts through these entry points instead of running per-lane Dr.Jit
 * code / vcalls.  Plain C types only: device pointers + sizes, no torch,
 * no Dr.Jit, no C++ types.
 *
 * Conventions
 *   - All array arguments are DEVICE pointers (HIP) to SoA component arrays
 *     of `n` elements each (Dr.Jit arrays are SoA: one array per scalar
 *     component, cf. the RayHitT offsets in src/render/scene_native.inl:106-113).
 *   - Every call is asynchronous and ordered on the caller's `stream`
 *     (a hipStream_t passed as void*; NULL = default stream).  No hidden
 *     synchronisation except where stated (hf_bbox, hf_get_mip, hf_get_node_level).
 *   - `active` (uint8 per lane, NULL = all lanes active) mirrors the `Mask active`
 *     argument of the reference methods; inactive lanes produce a miss /
 *     zero-initialised record (include/mitsuba/render/interaction.h:479-499, 667-673).
 *   - Return value: HF_OK or an error code; hf_last_error_string() describes
 *     the last failure on the calling thread.  No exceptions cross the ABI;
 *     the adapter turns codes into Throw(...) (src/render/mesh.cpp:711 style).
 *   - Query functions are re-entrant on a const handle (the reference calls
 *     them concurrently from worker threads, src/render/integrator.cpp:161-200);
 *     hf_set_heights* requires that no query on the same handle is in flight
 *     on another stream (reference: dr::sync_thread() in parameters_changed,
 *     src/shapes/rectangle.cpp:131-142).
 *   - HIP graphs: the wavefront entry points (device-pointer forms), hf_set_heights and hf_adam_step may be issued
 *     on a stream that is being captured; they then allocate nothing and record / wait for no event, so one
 *     optimisation step can be captured once and replayed.  Limits, all the caller's to honour:
 *       * every captured trace launch (hf_ray_intersect*, hf_ray_test, hf_reparam_trace) reserves one of 32 scratch
 *         blocks of the handle for as long as its graph may be replayed; the 33rd is refused with HF_EINVAL.
 *         hf_capture_reset() hands the blocks back once the graphs captured so far have been destroyed;
 *       * two graphs of one handle must not be replayed concurrently with each other unless they were captured
 *         without a reset in between (distinct blocks); replays that run concurrently with other work of the same
 *         handle on other streams are ordered by the caller, as for any buffer the graph writes;
 *       * a replayed hf_set_heights / hf_adam_step does not record the handle's "built" event: after such a replay
 *         synchronise the replay's stream before hf_bbox, hf_get_mip, hf_get_node_level, the packet entry points or
 *         hf_destroy;
 *       * a captured launch snapshots the transform (to_world / to_object) by value: hf_set_transform after the
 *         capture does not reach the replays -- re-capture.
 *     The forward-mode entry points (hf_tangent, hf_direct_lighting_weighted_tangent, hf_point_lighting_tangent) are
 *     capturable as well: they reserve no scratch block, allocate nothing and never synchronise the host.
 *     Not capturable: hf_create / hf_destroy, hf_set_heights_host, hf_bbox, hf_get_mip, hf_get_node_level and the
 *     host-pointer packet entry (they synchronise); hf_set_face_normals and hf_set_area_sampling (refused with HF_EINVAL), hf_surface_area
 *     and, with smooth shading or area sampling, hf_set_transform (they synchronise).  hf_sample_position and its
 *     adjoint / tangent are capturable like the other wavefront entry points (no scratch block), and so are
 *     hf_eval_attribute and its adjoint / tangent (the attribute buffer is the caller's).  The four hf_sky_* entries
 *     are capturable too: hf_sky_lighting traces without a work counter (one workgroup per 256 samples), so unlike the
 *     other trace launches it reserves no scratch block and does not count towards the 32.
 *     The four hf_bounce_* entries are capturable in the same way, and so are the hf_envmap_* entries, the table
 *     build included (the map and its table are the caller's buffers).
 */
#ifndef HF_H
#define HF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HF_VERSION 4 /* 2: hf_reparam_* take ray_id; hf_adjoint_rows, weighted lighting, hf_capture_reset; 3: hf_adam_step_scheduled;
                        4: hf_set_ray_coherence */

/* status codes */
enum {
    HF_OK      = 0,
    HF_EINVAL  = 1,  /* bad argument (NULL pointer, width/height < 2: src/textures/bitmap.cpp:280-283) */
    HF_EDEVICE = 2,  /* HIP runtime error */
    HF_ENOMEM  = 3,  /* device allocation failed */
    HF_EFLAGS  = 4   /* DetachShape | FollowShape (src/render/mesh.cpp:709-711) */
};

/* RayFlags -- identical values to include/mitsuba/render/interaction.h:19-69 */
enum {
    HF_RAY_EMPTY         = 0x0,
    HF_RAY_MINIMAL       = 0x1,
    HF_RAY_UV            = 0x2,
    HF_RAY_DPDUV         = 0x4,
    HF_RAY_SHADINGFRAME  = 0x8,
    HF_RAY_DNGDUV        = 0x10,
    HF_RAY_DNSDUV        = 0x20,
    HF_RAY_BOUNDARYTEST  = 0x40,
    HF_RAY_FOLLOWSHAPE   = 0x80,
    HF_RAY_DETACHSHAPE   = 0x100,
    HF_RAY_ALL           = 0x2 | 0x4 | 0x8,
    HF_RAY_ALL_NONDIFF   = 0x2 | 0x4 | 0x8 | 0x100,
    /* libhf extension (not a Mitsuba RayFlags value; bits above the reference's): with HF_RAY_BOUNDARYTEST,
     * boundary_test is the reference Mesh's per-triangle SDF over ALL three edges of the hit triangle
     * (src/render/mesh.cpp:845-890, 0 on an edge .. 1 at the incentre) instead of this shape's default, the same
     * SDF restricted to SILHOUETTE edges (a deliberate extension for heightfields) */
    HF_RAY_BOUNDARY_ALL_EDGES = 0x10000
};

typedef struct hf_field hf_field_t; /* opaque handle: owns heights copy, min/max mips */
typedef void *hf_stream_t;          /* hipStream_t */

/* Plugin properties (build decision, SURVEY.md section 8a: {to_world, max_height,
 * heightfield tensor, flip_normals}); replaces the Properties-driven constructor +
 * update() of a shape plugin (src/shapes/rectangle.cpp:83-112). */
typedef struct hf_desc {
    uint32_t width;        /* vertices along object x (tensor columns), >= 2 */
    uint32_t height;       /* vertices along object y (tensor rows),    >= 2 */
    float    max_height;   /* object z = height value * max_height */
    float    to_world[12]; /* row-major 3x4 affine */
    float    to_object[12];/* inverse of to_world; used when has_to_object != 0
                              (the adapter passes Mitsuba's own m_to_object,
                              rectangle.cpp:102), else computed by hf_invert_affine */
    int32_t  has_to_object;
    int32_t  flip_normals;
    int32_t  device;       /* HIP device ordinal */
} hf_desc_t;

/* Ray3f (include/mitsuba/core/ray.h:24-82): o, d, maxt.  time/wavelengths are
 * not used by a static shape and stay on the caller's side.
 * ALIGNMENT: any float alignment works.  When every ray row and every output row of a launch is 16-byte aligned and
 * no `active` mask is given (what a device allocator hands out), the traversal kernels answer fetches of 256 rays
 * that miss the bound as a whole -- the part of an image beside the terrain -- through 16-byte loads and stores
 * (DESIGN 4.1 "wide path": -4 % on the BASELINE wavefront); results do not depend on it.
 * TEST HOOK: the environment variable HF_FORCE_GRAB=<64 .. 4096, a multiple of 64>, read at every trace launch, fixes
 * the number of rays a wave fetches at a time (otherwise chosen from the size of the launch); 256 lets launches of any
 * size take the wide path (tests/test_gpu_parity.py, tests/tools/fuzz_parity.py).  Results do not depend on it.
 * TEST HOOK: the environment variable HF_FORCE_GRID=<blocks, an integer >= 1>, read at every launch of a grid-stride
 * kernel (every entry point but the traversal: SI, adjoints, tangents, reparameterisation, Adam, area sampling, attributes,
 * parameterisation), makes the grid min(usual grid, blocks): launches of test size then go round their loops several
 * times (tests/test_gpu_grid_stride.py).  It only ever lowers the grid, so scratch and captured launches stay within
 * what they reserve; any other value is ignored.  Results do not depend on it except through the order of float
 * additions (atomic scatters, the per-block sums of dL/d(to_world)); per-lane outputs keep their bytes.
 * TEST HOOK: the environment variable HF_SENSOR_STORE=dword|wide, read at every hf_sensor_rays and hf_thinlens_rays,
 * picks the store variant of its kernel (one sample per lane and 4-byte stores, or four per lane and one 16-byte store per
 * row where the row is aligned) instead of the one the library was built to use; any other value is ignored.
 * Results do not depend on it: the two variants write the same bytes (tests/test_gpu_sensor.py, test_gpu_thinlens.py). */
typedef struct hf_rays {
    const float *o[3];
    const float *d[3];
    const float *maxt;
} hf_rays_t;

/* PreliminaryIntersection3f (interaction.h:587-691): t (+inf = miss), prim_uv,
 * prim_index = 2*(cell_y*(width-1)+cell_x)+tri.  shape_index is always
 * (uint32_t)-1 for a non-instanced shape (rectangle.cpp:222) and is not stored. */
typedef struct hf_pi {
    float    *t;
    float    *prim_uv[2];
    uint32_t *prim_index;
} hf_pi_t;

typedef struct hf_pi_const {
    const float    *t;
    const float    *prim_uv[2];
    const uint32_t *prim_index;
} hf_pi_const_t;

/* SurfaceInteraction3f fields filled by Shape::compute_surface_interaction +
 * finalize_surface_interaction (interaction.h:175-507).  Any pointer may be NULL
 * (field not wanted).  dn_du/dn_dv are not stored: zero with flat shading (the default), and
 * hf_shading_derivatives computes them with smooth shading (hf_set_face_normals); duv_dx/duv_dy are
 * zeroed by finalize.  sh_n is the face normal n with flat shading and the interpolated vertex normal
 * with smooth shading (with HF_RAY_SHADINGFRAME or HF_RAY_DNSDUV, as mesh.cpp:813-840); sh_s, sh_t
 * and wi are built on sh_n.  dp_du / dp_dv come from the texcoords with HF_RAY_DPDUV; without it they are
 * coordinate_system(n) of the face normal before flip_normals (mesh.cpp:762), and hf_adjoint / hf_tangent differentiate
 * them through n (the sign of n.z held constant).  uv is the texcoord with HF_RAY_UV or HF_RAY_DPDUV, else prim_uv. */
typedef struct hf_si {
    float *t;
    float *p[3];
    float *n[3];
    float *uv[2];
    float *sh_n[3];      /* sh_frame.n */
    float *dp_du[3];
    float *dp_dv[3];
    float *boundary_test;/* written only with HF_RAY_BOUNDARYTEST */
    float *sh_s[3];      /* sh_frame.s, sh_frame.t: HF_RAY_SHADINGFRAME (interaction.h:257-267) */
    float *sh_t[3];
    float *wi[3];
} hf_si_t;

/* Upstream gradient dL/d(si field); NULL pointer = zero gradient. */
typedef struct hf_si_grad {
    const float *t;
    const float *p[3];
    const float *n[3];
    const float *uv[2];
    const float *sh_n[3];
    const float *dp_du[3];
    const float *dp_dv[3];
} hf_si_grad_t;

/* Tangent (forward-mode derivative) of the same 18 differentiable fields; NULL pointer = row not written. */
typedef struct hf_si_tangent {
    float *t;
    float *p[3];
    float *n[3];
    float *uv[2];
    float *sh_n[3];
    float *dp_du[3];
    float *dp_dv[3];
} hf_si_tangent_t;

/* ---- lifetime / parameters ------------------------------------------------ */

/* Replaces: plugin construction + update() (src/shapes/rectangle.cpp:83-112) and the
 * OptiX blob upload optix_prepare_geometry (rectangle.cpp:328-338).  Heights start
 * as all zero; call hf_set_heights* before tracing.  Limits: width, height >= 2
 * (bitmap.cpp:280-283), at most 32768 cells per side and 2^30 vertices (HF_EINVAL beyond). */
int hf_create(const hf_desc_t *desc, hf_field_t **out);
int hf_destroy(hf_field_t *hf);
/* Returns the scratch blocks reserved by captured trace launches (HIP graphs, above) to the handle.  Call it only
 * when every graph captured from this handle so far has been destroyed or will not be replayed again.  (No
 * reference counterpart: Dr.Jit owns its kernel-launch scratch; cf. jit_free, src/shapes/rectangle.cpp:330-336.) */
int hf_capture_reset(hf_field_t *hf);

/* Replaces: parameters_changed({"heightfield"}) (pattern rectangle.cpp:131-142,
 * tensor form src/textures/bitmap.cpp:272-286) + the accel rebuild it triggers
 * (src/render/scene.cpp:343-385): copies width*height floats (row-major, row 0 at
 * object y=-1) from DEVICE memory and rebuilds the acceleration data (min/max mip pyramid and the
 * sheared bounds of its fine levels), all on `stream`. */
int hf_set_heights(hf_field_t *hf, const float *d_heights, hf_stream_t stream);
/* same from HOST memory (synchronous copy) */
int hf_set_heights_host(hf_field_t *hf, const float *h_heights, hf_stream_t stream);
/* Replaces: mitsuba.ad.Adam.step() for this parameter (src/python/python/ad/optimizers.py:263-300) followed
 * by params.update() -> parameters_changed({"heightfield"}) (src/python/python/util.py:185-232): one
 * Adam step on the caller's parameter buffer d_heights[width*height] (DEVICE, updated in place) with the
 * gradient d_grad and the moment buffers d_m, d_v (zero them before step 1; `step` counts from 1), then
 * hf_set_heights(hf, d_heights).  lr_t = lr * sqrt(1 - beta2^step) / (1 - beta1^step);
 * m = beta1 m + (1-beta1) g;  v = beta2 v + (1-beta2) g^2;  h -= lr_t m / (sqrt(v) + eps);
 * mask_updates: bit 0 (HF_ADAM_MASK_UPDATES) leaves h, m, v untouched where g == 0 (optimizers.py:282-285,
 * 293-294); bit 1 (HF_ADAM_UNIFORM) selects the 'UniformAdam' variant (optimizers.py:259, 290-291): the update
 * divides by sqrt(max over the texture of v) + eps instead of the per-texel sqrt(v) + eps (two launches).
 * The hyper-parameters are host doubles like the reference's Python scalars: the bias-correction scale is
 * evaluated in double and rounded once (optimizers.py:267-268), everything else runs in float32.
 * SERIAL PER HANDLE: the uniform variant keeps its running maximum in one device word owned by the handle, and the
 * rebuild writes the handle's acceleration data -- issue the steps of one handle on one stream (or order them yourself).
 * A NaN second moment makes the uniform step NaN everywhere (the maximum keeps it), as dr.max over a NaN does in the
 * reference; the reference holds no fixture for that case (parity unpinned).
 */
#define HF_ADAM_MASK_UPDATES 1
#define HF_ADAM_UNIFORM 2
int hf_adam_step(hf_field_t *hf, float *d_heights, const float *d_grad, float *d_m, float *d_v, double lr,
                 double beta1, double beta2, double eps, uint32_t step, int mask_updates, hf_stream_t stream);
/* hf_adam_step for CAPTURED steps (HIP graphs).  hf_adam_step bakes the step number into its launch (the bias-corrected
 * step size lr_t is a kernel argument computed on the host), so a captured step would replay step 1 for ever.  Here
 * the step sizes come from DEVICE memory: d_lr_t[k] = hf_adam_lr_t(lr, beta1, beta2, k + 1) for the steps the caller
 * intends to run (filled once, on the host, with hf_adam_step's own arithmetic: bit-identical updates), and *d_step
 * (device, zero before the first step) selects the entry and is incremented on the stream after the update -- every
 * replay of the captured step is the next Adam step.  Same mask_updates bits, same rebuild, serial per handle. */
float hf_adam_lr_t(double lr, double beta1, double beta2, uint32_t step);
int hf_adam_step_scheduled(hf_field_t *hf, float *d_heights, const float *d_grad, float *d_m, float *d_v,
                           const float *d_lr_t, uint32_t *d_step, double beta1, double beta2, double eps,
                           int mask_updates, hf_stream_t stream);

/* Replaces: m_to_world update + update() (rectangle.cpp:101-112, 131-142).  With smooth shading the vertex
 * normals are rebuilt as well: after the last hf_set_heights* (whatever its stream), and the call returns when the
 * rebuild is complete, so nothing the caller issues afterwards, on any stream, can overlap it.  In that mode the rule
 * of hf_set_heights holds: no query on this handle may be in flight on another stream. */
int hf_set_transform(hf_field_t *hf, const float to_world[12], const float *to_object_or_null);

/* Replaces: the Mesh property `face_normals` (src/render/mesh.cpp:30) and the vertex normals it switches on.
 * face_normals = 1 (the default of a new handle, unlike Mesh's): flat shading, sh_frame.n = the face normal.
 * face_normals = 0: smooth shading.  The handle then owns one vertex normal per texel (16 bytes each), angle-weighted
 * as the JIT path of Mesh::recompute_vertex_normals computes them (mesh.cpp:350-384) from the world-space vertices,
 * and rebuilt wherever they can go stale, as parameters_changed does (mesh.cpp:115-119): by this call on `stream`
 * (ordered after the last hf_set_heights*; later queries on other streams must be ordered after `stream` by the
 * caller, as for hf_set_heights), by every hf_set_heights* on its stream (graph-capturable, as before) and by
 * hf_set_transform (synchronous).  This call itself is not capturable: HF_EINVAL while `stream` is being captured.  A hit's shading normal
 * is the normalised barycentric blend of its three vertex normals, flipped after the blend by flip_normals
 * (mesh.cpp:792-840); hf_adjoint / hf_tangent differentiate it through the barycentrics and through the vertex
 * normals (which stay attached to the heights, as in test_mesh.py:540-600; detached with HF_RAY_DETACHSHAPE,
 * mesh.cpp:803-811).  boundary_test keeps its geometric (silhouette) definition in both modes, so
 * hf_reparam_backward does not depend on the mode.  Same rule as hf_set_heights: no query on this handle may be in
 * flight on another stream.  HF_ENOMEM when the normals cannot be allocated.  Flat mode runs the kernels it always
 * ran, and frees the normals. */
int hf_set_face_normals(hf_field_t *hf, int face_normals, hf_stream_t stream);
int hf_get_face_normals(const hf_field_t *hf);

/* Replaces: Shape::bbox() (include/mitsuba/render/shape.h:253; analog rectangle.cpp:114-124).
 * World-space {min xyz, max xyz}.  Synchronises `stream`-ordered height updates. */
int hf_bbox(hf_field_t *hf, float out[6]);

/* device pointer to the handle's own copy of the heights (width*height floats) */
int hf_heights_device(hf_field_t *hf, const float **out);
int hf_dims(const hf_field_t *hf, uint32_t *width, uint32_t *height);

/* ---- the hot path ------------------------------------------------------------ */
/* All of these launch on `stream` and return immediately; the calling thread's current HIP device must be the
 * handle's (HF_EDEVICE otherwise), all arrays are device memory of that device.
 *
 * Results: the closest hit is the minimum of (t, -prim_index) over the triangles the reference's fp32
 * Moeller-Trumbore arithmetic (include/mitsuba/render/mesh.h:357-380) reports as hit -- what a brute force over
 * every triangle returns, bit for bit.  That test is itself ill-conditioned for distant origins on needle terrain
 * (cells hundreds of times taller than wide: the computed barycentrics are off by half a cell from 8 object units
 * away at 4096^2, by more than a cell from 50): a few rays in 10^5 then carry a hit of fp32 noise, which this library
 * reports whenever the noise stays within its margins -- in every such case resolved against the full brute force so
 * far (profiles/r03_far_origin.txt) -- and which a BVH over the same triangles may or may not report. */

/* The `coherent` hint of Scene::ray_intersect / ray_test / ray_intersect_preliminary
 * (include/mitsuba/render/scene.h:117-146, 188-207, 237-259: "a hint that can improve performance in the first step of
 * finding the PreliminaryInteraction"; integrators pass coherent = true for camera rays, reparam.py:95 traces its
 * auxiliary rays with coherent = false).  A property of the handle, read by every trace launch that follows:
 *   HF_COHERENCE_AUTO        (default) every 64-ray batch decides for itself: packets take the beam sweep, the others
 *                            the per-lane walk; auxiliary rays (hf_reparam_trace*) as _INCOHERENT when kappa < 4e6
 *   HF_COHERENCE_INCOHERENT  = coherent false: kernels without the sweep (fewer registers, no LDS, 6-7 instead of 5
 *                            waves per SIMD).  Bounce rays -8 %, the reparameterisation backward -7 %; camera rays +25 %.
 *   HF_COHERENCE_COHERENT    = coherent true: as _AUTO, and auxiliary rays through the full kernel whatever kappa
 * The results do not depend on it (bit for bit: tests/test_gpu_parity.py).  Serial per handle like everything else.
 * (Shadow rays towards one light share a direction: hf_ray_test is 7 % slower with _INCOHERENT than with _AUTO on the bench's
 * 16.5 M shadow rays -- a caller that maps an integrator's default `coherent = false` onto this should do so for the
 * closest-hit launches only.) */
enum { HF_COHERENCE_AUTO = 0, HF_COHERENCE_INCOHERENT = 1, HF_COHERENCE_COHERENT = 2 };
int hf_set_ray_coherence(hf_field_t *hf, int coherence);
int hf_get_ray_coherence(const hf_field_t *hf);

/* Replaces: Shape::ray_intersect_preliminary(const Ray3f&, Mask)
 * (include/mitsuba/render/shape.h:137-138, wrapper shape.h:621-629; called from
 * include/mitsuba/render/kdtree.h:2509-2510 and src/render/shape.cpp:211). */
int hf_ray_intersect_preliminary(const hf_field_t *hf, size_t n, const hf_rays_t *rays,
                                 const uint8_t *active, const hf_pi_t *out,
                                 hf_stream_t stream);

/* Replaces: Shape::ray_test(const Ray3f&, Mask) (shape.h:153, 630-633;
 * semantics == ray_intersect_preliminary().is_valid(), src/render/shape.cpp:430-434). */
int hf_ray_test(const hf_field_t *hf, size_t n, const hf_rays_t *rays,
                const uint8_t *active, uint8_t *out_hit, hf_stream_t stream);

/* Replaces: Shape::compute_surface_interaction(ray, pi, ray_flags, recursion_depth=0, active)
 * (shape.h:179-183) followed by SurfaceInteraction::finalize_surface_interaction
 * (interaction.h:476-499), i.e. PreliminaryIntersection::compute_surface_interaction
 * (interaction.h:658-684). */
int hf_compute_surface_interaction(const hf_field_t *hf, size_t n, const hf_rays_t *rays,
                                   const hf_pi_const_t *pi, uint32_t ray_flags,
                                   const uint8_t *active, const hf_si_t *out,
                                   hf_stream_t stream);

/* Replaces: Shape::ray_intersect(ray, ray_flags, active) = preliminary + SI
 * (src/render/shape.cpp:436-446); one fused kernel.  out_pi may be NULL. */
int hf_ray_intersect(const hf_field_t *hf, size_t n, const hf_rays_t *rays,
                     uint32_t ray_flags, const uint8_t *active,
                     const hf_pi_t *out_pi, const hf_si_t *out_si, hf_stream_t stream);

/* Replaces: the Dr.Jit reverse-mode pass through compute_surface_interaction that
 * dr.backward_from() triggers (src/python/python/ad/integrators/prb_reparam.py:586-587):
 * every dr::gather from the parameter buffer becomes scatter_reduce(Add).
 * Accumulates dL/dheight (width*height floats, row-major) with float atomics;
 * grad_o / grad_d (3 arrays each, may be NULL) receive dL/d(ray.o), dL/d(ray.d)
 * per lane (overwritten).  grad_heights may be NULL when only ray gradients are wanted. */
int hf_adjoint(const hf_field_t *hf, size_t n, const hf_rays_t *rays,
               const hf_pi_const_t *pi, uint32_t ray_flags, const uint8_t *active,
               const hf_si_grad_t *grad_si, float *grad_heights,
               float *const grad_o[3], float *const grad_d[3], hf_stream_t stream);
/* hf_adjoint that also reports WHICH texture rows it added to: row_band (device, 2 x uint32, may be NULL) is updated
 * with atomicMin / atomicMax to {lowest row touched, highest row touched + 1}; the caller initialises it to
 * {height, 0} before the launches it wants covered.  Rows outside the band of every rank hold zeros in every rank's
 * private gradient texture, so a multi-GPU host may all-reduce rows [lo, hi) only (hf_allreduce_grad on
 * grad_heights + lo * width with count (hi - lo) * width).  (Reference: the gradient of the whole parameter buffer is
 * what dr.backward leaves in params.grad, src/python/python/ad/integrators/common.py:312-329; no band there.) */
int hf_adjoint_rows(const hf_field_t *hf, size_t n, const hf_rays_t *rays,
                    const hf_pi_const_t *pi, uint32_t ray_flags, const uint8_t *active,
                    const hf_si_grad_t *grad_si, float *grad_heights,
                    float *const grad_o[3], float *const grad_d[3], uint32_t *row_band, hf_stream_t stream);

/* Replaces: the Dr.Jit FORWARD-mode traversal of the attached surface interaction of mesh.cpp:672-903 that
 * dr.forward / dr.forward_to trigger (src/render/tests/test_mesh.py:380-422, 458-531, 674-735; the integrators'
 * render_forward, src/python/python/ad/integrators/common.py:120, 587, 977): for a perturbation of the heights
 * (dheights: width*height floats, row-major, the layout of hf_adjoint's grad_heights) and of the rays (d_o, d_d: 3
 * arrays of n floats each), the tangent of the 18 fields of hf_si_tangent_t per lane (overwritten; NULL rows are not
 * written).  Any of dheights / d_o / d_d may be NULL (zero tangent; a non-NULL d_o / d_d may have NULL rows).
 * The exact transpose of hf_adjoint, mode for mode: default = Moeller-Trumbore re-intersection with attached vertices
 * (t = replace_grad(pi.t, t_d), mesh.cpp:728-735); HF_RAY_FOLLOWSHAPE = frozen barycentrics, t = sqrt(|p-o|^2/|d|^2)
 * (mesh.cpp:748-752); HF_RAY_DETACHSHAPE = the heights contribute nothing, the rays still do.  Missed and inactive lanes
 * get exactly zero tangents.  No atomics: the result is bitwise the same from launch to launch. */
int hf_tangent(const hf_field_t *hf, size_t n, const hf_rays_t *rays, const hf_pi_const_t *pi, uint32_t ray_flags,
               const uint8_t *active, const float *dheights, const float *const d_o[3], const float *const d_d[3],
               const hf_si_tangent_t *tangent_si, hf_stream_t stream);

/* Replaces: the reverse-mode pass of the reference through Rectangle's attached to_world (src/shapes/rectangle.cpp:128,
 * 255-310: to_world is Differentiable | Discontinuous there).  hf_adjoint_rows, plus grad_to_world: 12 device floats,
 * row-major 3x4 [A | t] like hf_desc_t.to_world, ACCUMULATED with dL/d(to_world) = sum_v dL/dP_v (q_v, 1)^T over the
 * world positions P_v = A q_v + t of the vertices each hit reads, q_v = (x_v, y_v, max_height h_v) in object space: the
 * hit triangle's three, and with smooth shading also the 1-rings of its three vertex normals.  The modes as in
 * hf_adjoint: default = Moeller-Trumbore re-intersection (p stays on the ray), HF_RAY_FOLLOWSHAPE = frozen barycentrics
 * (p is glued to the shape), HF_RAY_DETACHSHAPE = no contribution; the choice of triangle is not differentiated.  No
 * float atomics on grad_to_world: the blocks' partial sums go to a scratch block of the handle's ring and one more
 * launch adds them up in a fixed order, so the result is bitwise the same from launch to launch (capturable, like the
 * trace launches; two streams may launch on one handle concurrently).  grad_heights, grad_o, grad_d and row_band may
 * each be NULL; grad_heights then equals hf_adjoint's up to the order of its float atomics, and grad_o / grad_d are
 * bitwise hf_adjoint's.  grad_to_world == NULL: exactly hf_adjoint_rows. */
int hf_adjoint_transform(const hf_field_t *hf, size_t n, const hf_rays_t *rays,
                         const hf_pi_const_t *pi, uint32_t ray_flags, const uint8_t *active,
                         const hf_si_grad_t *grad_si, float *grad_heights,
                         float *const grad_o[3], float *const grad_d[3], uint32_t *row_band,
                         float *grad_to_world, hf_stream_t stream);
/* Replaces: the forward-mode pass of the reference through Rectangle's attached to_world (rectangle.cpp:255-310).
 * hf_tangent, plus d_to_world: the tangent of to_world, 12 device floats (row-major 3x4), NULL = zero: every vertex the
 * surface interaction reads moves by dA q_v + dt besides its height tangent.  The transpose of hf_adjoint_transform,
 * mode for mode.  No atomics: bitwise the same from launch to launch.  d_to_world == NULL: exactly hf_tangent. */
int hf_tangent_transform(const hf_field_t *hf, size_t n, const hf_rays_t *rays, const hf_pi_const_t *pi,
                         uint32_t ray_flags, const uint8_t *active, const float *dheights, const float *const d_o[3],
                         const float *const d_d[3], const float *d_to_world, const hf_si_tangent_t *tangent_si,
                         hf_stream_t stream);

/* Replaces: SurfaceInteraction3f::dn_du / dn_dv of the smooth-shaded mesh under RayFlags::dNSdUV (mesh.cpp:818-829):
 * the derivatives of the shading normal with respect to the barycentrics (b1, b2) of every hit of pi, before
 * flip_normals (as the reference).  dn_du / dn_dv: 3 device arrays of n floats each (either may be NULL), overwritten.
 * Zero for misses, inactive lanes and with flat shading.  Forward only. */
int hf_shading_derivatives(const hf_field_t *hf, size_t n, const hf_pi_const_t *pi, const uint8_t *active,
                           float *const dn_du[3], float *const dn_dv[3], hf_stream_t stream);

/* ---- area sampling: the sampling side of Shape (surface_area, sample_position, pdf_position) ------------------ */

/* PositionSample3f (include/mitsuba/render/records.h) as Mesh::sample_position fills it (src/render/mesh.cpp:557-610):
 * p, n, uv and pdf are required; time stays on the caller's side and delta is always false.  prim_index (the sampled
 * triangle, prim_index order) and b (the barycentrics b1, b2 of square_to_uniform_triangle, include/mitsuba/core/
 * warp.h:153-156) may be NULL (not wanted); hf_sample_position_adjoint / _tangent take them back. */
typedef struct hf_position_sample {
    float    *p[3];
    float    *n[3];
    float    *uv[2];
    float    *pdf;
    uint32_t *prim_index;
    float    *b[2];
} hf_position_sample_t;

/* Replaces: Mesh::build_pmf / ensure_pmf_built (src/render/mesh.cpp:401-432) and the DiscreteDistribution it builds
 * (include/mitsuba/core/distr_1d.h:20-240), for the heightfield's triangles in prim_index order.  enable != 0 allocates
 * the handle's area table (4 bytes per triangle + 1/16 of that for the search) and builds it on `stream` after the last
 * hf_set_heights*; later queries on other streams must be ordered after `stream` by the caller, as for hf_set_heights.
 * From then on the table is rebuilt wherever it can go stale: by every hf_set_heights* on its stream (graph-capturable,
 * like the vertex normals) and by hf_set_transform (synchronous).  The areas do not depend on the shading mode, so
 * hf_set_face_normals does not rebuild it (hf_sample_position reads the vertex normals of the mode current at launch).
 * enable = 0 frees the table.  A handle that never enables sampling allocates nothing and runs no extra kernel.
 * Entry i of the table is the world-space area .5f * norm(cross(p1 - p0, p2 - p0)) of triangle i in fp32; its CDF is
 * a running fp64 sum, each prefix rounded to fp32, summed in one fixed association order (bitwise the same from build
 * to build; not the sequential loop's order, so a prefix may differ from compute_cdf's by an fp32 ulp).  The table is
 * DETACHED: no derivative flows through the pdf or the choice of triangle (as build_pmf).  Not capturable: HF_EINVAL
 * while `stream` is being captured.  HF_ENOMEM when the table cannot be allocated. */
int hf_set_area_sampling(hf_field_t *hf, int enable, hf_stream_t stream);
/* Replaces: Mesh::surface_area (mesh.cpp:552-555) = m_area_pmf.sum(), and pdf_position (mesh.cpp:637-640) =
 * m_area_pmf.normalization() = (float) (1.0 / sum).  Synchronous: waits for the last rebuild.  normalization may be
 * NULL.  HF_EINVAL without the table (hf_set_area_sampling). */
int hf_surface_area(hf_field_t *hf, float *area, float *normalization);
/* Read-only view of the table for tests and tools: the device pointer to the fp32 CDF (one entry per triangle; the
 * storage is padded with +inf up to a multiple of 64 entries) and its entry count; NULL / 0 without the table.  Reads
 * of it are ordered after the last rebuild by the caller. */
int hf_area_cdf(const hf_field_t *hf, const float **cdf, size_t *count);

/* Replaces: Mesh::sample_position(time, sample, active) (src/render/mesh.cpp:557-610) for n samples (sample: 2 device
 * arrays of n floats in [0, 1)).  Step by step: the triangle index is DiscreteDistribution::sample_reuse(sample.y)
 * (distr_1d.h:120-130, 167-176): the first i in [valid.x, valid.y] with !(cdf[i] < sample.y * sum), valid.y when there
 * is none (dr::binary_search), and sample.y is reused as (sample.y - cdf[i-1] norm) / (pmf[i] norm); then
 * b = square_to_uniform_triangle, p = fmadd(e0, b.x, fmadd(e1, b.y, p0)), uv the same fmadd chain over the texcoords,
 * n = normalize(cross(e0, e1)) -- with smooth shading (hf_set_face_normals(hf, 0)) the normalised barycentric blend of
 * the three vertex normals -- negated by flip_normals, pdf = norm.  Inactive lanes (active: NULL = all) are zeros in
 * every row.  Capturable (reads the table and its scalars from device memory, so a replay sees later rebuilds).
 * HF_EINVAL without the table. */
int hf_sample_position(const hf_field_t *hf, size_t n, const float *const sample[2], const uint8_t *active,
                       const hf_position_sample_t *out, hf_stream_t stream);
/* Reverse mode of hf_sample_position with respect to the heights: p and n stay attached to the heights through the
 * triangle's vertices (vertex_position / vertex_normal in the reference), the index and b do not.  For the samples
 * (prim_index, b) of a forward call, accumulates dL/dheight into grad_heights (width*height floats, float atomics) from
 * the upstream gradients grad_p / grad_n (3 device arrays of n floats each; either may be NULL = zero).  Flat shading: 3
 * heights per sample through p and the face normal; smooth shading: n also reaches the 1-rings of the three vertices
 * (up to 12 heights) through the vertex-normal VJP.  Capturable; does not need the table. */
int hf_sample_position_adjoint(const hf_field_t *hf, size_t n, const uint32_t *prim_index, const float *const b[2],
                               const uint8_t *active, const float *const grad_p[3], const float *const grad_n[3],
                               float *grad_heights, hf_stream_t stream);
/* Forward mode of the same: for the height tangent dheights (width*height floats, NULL = zero), the tangents dp / dn (3
 * device arrays of n floats each, overwritten; either may be NULL = not written) of the samples (prim_index, b).
 * Inactive lanes get zeros.  No atomics: bitwise the same from launch to launch.  Capturable; does not need the table. */
int hf_sample_position_tangent(const hf_field_t *hf, size_t n, const uint32_t *prim_index, const float *const b[2],
                               const uint8_t *active, const float *dheights, float *const dp[3], float *const dn[3],
                               hf_stream_t stream);
/* Replaces: the reverse mode of Mesh::sample_position through the attached to_world of the reference's shapes (the
 * vertex positions that sample_position gathers, mesh.cpp:557-610).  hf_sample_position_adjoint, plus grad_to_world
 * (12 device floats, accumulated, as in hf_adjoint_transform: p = P0 + b.x e0 + b.y e1 and n, flat or smooth, follow
 * the vertices; slab reduction, no float atomics on it, bitwise repeatable).  grad_heights may be NULL.
 * grad_to_world == NULL: exactly hf_sample_position_adjoint. */
int hf_sample_position_adjoint_transform(const hf_field_t *hf, size_t n, const uint32_t *prim_index,
                                         const float *const b[2], const uint8_t *active, const float *const grad_p[3],
                                         const float *const grad_n[3], float *grad_heights, float *grad_to_world,
                                         hf_stream_t stream);
/* Replaces: the forward mode of the same.  hf_sample_position_tangent, plus d_to_world (12 device floats, NULL = zero).
 * No atomics.  d_to_world == NULL: exactly hf_sample_position_tangent. */
int hf_sample_position_tangent_transform(const hf_field_t *hf, size_t n, const uint32_t *prim_index,
                                         const float *const b[2], const uint8_t *active, const float *dheights,
                                         const float *d_to_world, float *const dp[3], float *const dn[3],
                                         hf_stream_t stream);

/* ---- shape attributes: the attribute side of Shape (has_attribute, eval_attribute, eval_attribute_1 / _3) -------- */

/* Where an attribute lives (Mesh's MeshAttributeType, include/mitsuba/render/mesh.h): HF_ATTR_VERTEX, one value per grid
 * vertex, count = width*height in the heights' row-major order (vertex (i, j) = i*width + j); HF_ATTR_FACE, one value per
 * triangle, count = 2*(width-1)*(height-1) in prim_index order. */
enum { HF_ATTR_VERTEX = 0, HF_ATTR_FACE = 1 };

/* Replaces: Mesh::eval_attribute / eval_attribute_1 / eval_attribute_3 (src/render/mesh.cpp:944-1004) through
 * Mesh::interpolate_attribute (include/mitsuba/render/mesh.h:399-440) for n surface interactions, RGB variants (no
 * spectral upsampling).  attr is the caller's device buffer of count*size floats, interleaved [count][size] like Mesh's
 * FloatStorage (the attribute is a parameter, not handle state); size is 1 or 3.  Vertex attributes: the weights
 * (w, u, v) = Mesh::barycentric_coordinates (mesh.cpp:645-667), the least-squares solve from si.p (p: 3 device arrays
 * of n floats) and the world-space vertices of prim_index in the reference's operation order, then
 * fmadd(v0, w, fmadd(v1, u, v2 v)); face attributes: the row of prim_index (p is not read and may be NULL).  t (si.t,
 * may be NULL = every active lane is a hit) and active (NULL = all) select the lanes: misses (t = +inf), inactive lanes
 * and indices past the last triangle give exactly 0.  out: size device arrays of n floats, overwritten.  HF_EINVAL for a
 * bad type or size, a NULL attr, prim_index or output row, and p == NULL with HF_ATTR_VERTEX.  Capturable: no scratch
 * block, no allocation, no synchronisation; re-entrant on a const handle. */
int hf_eval_attribute(const hf_field_t *hf, size_t n, int type, uint32_t size, const float *attr,
                      const uint32_t *prim_index, const float *const p[3], const float *t, const uint8_t *active,
                      float *const out[], hf_stream_t stream);
/* Reverse mode of hf_eval_attribute (Dr.Jit AD through interpolate_attribute): for the upstream gradients grad_out
 * (size device arrays of n floats), accumulates dL/dattr into grad_attr (count*size floats, interleaved like attr)
 * and, for vertex attributes, writes dL/dp into grad_p (3 arrays of n floats, overwritten; zero for face attributes
 * and for lanes without a hit) and accumulates dL/dheight into grad_heights (width*height floats) through the three
 * vertices (vertex_position is attached to the heights whatever the ray flags; dP/dh = max_height * to_world[:, 2]).
 * Float atomics; for vertex attributes pre-summed per wave in an LDS tile first.  Face attributes carry no geometric
 * derivative.  Any of grad_attr, grad_p and grad_heights may be NULL (not wanted).  Inputs and errors as
 * hf_eval_attribute; capturable. */
int hf_eval_attribute_adjoint(const hf_field_t *hf, size_t n, int type, uint32_t size, const float *attr,
                              const uint32_t *prim_index, const float *const p[3], const float *t, const uint8_t *active,
                              const float *const grad_out[], float *grad_attr, float *const grad_p[3],
                              float *grad_heights, hf_stream_t stream);
/* Forward mode of hf_eval_attribute: for the tangents dattr (count*size floats, interleaved), dp (3 arrays of n floats,
 * the tangent of si.p) and dheights (width*height floats), each NULL = zero, the tangent of the value in dout (size
 * arrays of n floats, overwritten; 0 for lanes without a hit).  No atomics: bitwise the same from launch to launch.
 * Inputs and errors as hf_eval_attribute; capturable. */
int hf_eval_attribute_tangent(const hf_field_t *hf, size_t n, int type, uint32_t size, const float *attr,
                              const uint32_t *prim_index, const float *const p[3], const float *t, const uint8_t *active,
                              const float *dattr, const float *const dp[3], const float *dheights, float *const dout[],
                              hf_stream_t stream);

/* ---- eval_parameterization: the surface interaction at texture coordinates ---------------------------------------- */

/* Replaces: Shape::eval_parameterization(uv, ray_flags, active) (include/mitsuba/render/shape.h:361) as Mesh implements
 * it (src/render/mesh.cpp:503-545 build_parameterization, 614-635; Rectangle: src/shapes/rectangle.cpp:173-192), what
 * the area emitter calls when its radiance varies over the surface (src/emitters/area.cpp:136, 173, 211).  For n queries
 * uv (2 device arrays of n floats), the surface interaction of the point whose texcoords are uv.  Mesh traces the ray
 * o = (u, v, -1), d = (0, 0, 1) against its texcoord mesh; the heightfield's regular texcoords give the triangle in
 * closed form: cell (cx, cy) = (min(floor(u (W-1)), W-2), likewise v), fx = fma(u, W-1, -cx) clamped to [0, 1] (fy
 * likewise), tri 1 when fx + fy >= 1 (exactly), b = (fx, fy) on tri 0 and (1 - fx, 1 - fy) on tri 1 -- the highest
 * prim_index among the triangles that contain the point, as for a hit.  A lane is valid when active and 0 <= u, v <= 1
 * (NaN is not); an invalid lane gets the record of a miss (t = +inf, zeros, boundary_test 1e8 with HF_RAY_BOUNDARYTEST)
 * with wi = 0.  A valid lane's record is what hf_compute_surface_interaction gives for the UV-space ray and
 * pi = {1, b, prim_index}: ray_flags as there, t = 1, wi = sh_frame.to_local((0, 0, -1)); HF_RAY_FOLLOWSHAPE does not
 * replace t, and HF_RAY_BOUNDARYTEST is the all-edge SDF of HF_RAY_BOUNDARY_ALL_EDGES (no viewing ray).  out as in
 * hf_compute_surface_interaction (any row may be NULL); out_prim_index (n uint32, may be NULL): the triangle, 0 for
 * invalid lanes.  HF_EFLAGS for DetachShape | FollowShape.  Capturable: no scratch block, no allocation, no
 * synchronisation.  (HF_VERSION is unchanged: a caller detects the feature by the symbol.) */
int hf_eval_parameterization(const hf_field_t *hf, size_t n, const float *const uv[2], uint32_t ray_flags,
                             const uint8_t *active, const hf_si_t *out, uint32_t *out_prim_index, hf_stream_t stream);
/* Reverse mode of hf_eval_parameterization.  uv, the choice of triangle and b are detached; p, n, sh_n, dp_du and dp_dv
 * stay attached through the triangle's vertices -- to the heights, with smooth shading to the 1-rings of the vertex
 * normals, and to to_world: the FollowShape derivative of hf_adjoint with t held constant (the reference's default
 * mode re-intersects its UV-space ray with the world-space triangle, a derivative without geometric meaning: DESIGN 2).
 * grad_si.t and grad_si.uv are ignored.  Accumulates dL/dheight into grad_heights (width*height floats, float atomics;
 * may be NULL) and dL/d(to_world) into grad_to_world (12 floats, may be NULL) through the slab reduction of
 * hf_adjoint_transform (no float atomics on it: bitwise repeatable).  (prim, b) are recomputed from uv with the forward's
 * own lookup.  HF_RAY_DETACHSHAPE: no contribution.  Capturable (the slab is a scratch block, as hf_adjoint_transform). */
int hf_eval_parameterization_adjoint(const hf_field_t *hf, size_t n, const float *const uv[2], uint32_t ray_flags,
                                     const uint8_t *active, const hf_si_grad_t *grad_si, float *grad_heights,
                                     float *grad_to_world, hf_stream_t stream);
/* Forward mode of the same: for the height tangent dheights (width*height floats) and the tangent d_to_world of to_world
 * (12 floats), either NULL = zero, the tangent rows of tangent_si (overwritten; NULL rows are not written).  The t and uv
 * rows get 0; invalid lanes get 0 in every row.  No atomics: bitwise the same from launch to launch.  Capturable. */
int hf_eval_parameterization_tangent(const hf_field_t *hf, size_t n, const float *const uv[2], uint32_t ray_flags,
                                     const uint8_t *active, const float *dheights, const float *d_to_world,
                                     const hf_si_tangent_t *tangent_si, hf_stream_t stream);

/* ---- next row: minimal direct lighting on the wavefront ------- */

/* A directional emitter (src/emitters/directional.cpp:82,174): unit direction TOWARDS the light, scalar irradiance. */
#define HF_MAX_LIGHTS 8
typedef struct hf_dir_light {
    float to_light[3];
    float irradiance;
} hf_dir_light_t;

/* Replaces, for diffuse surfaces under directional lights, the emitter-sampling term of the direct
 * integrator (src/python/python/ad/integrators/direct_reparam.py:149-175: detached emitter sample, delta
 * light => MIS weight 1, attached BSDF value) with the diffuse BSDF (src/bsdfs/diffuse.cpp:135-140:
 * albedo/pi * cos_o, zero unless cos_i > 0 and cos_o > 0 in the shading frame) and the box-filter film
 * (mean of the spp samples of a pixel, sample i belongs to pixel i / spp as in
 * src/render/integrator.cpp:251-268):
 *   image[k][i / spp] = 1/spp * sum_s  albedo/pi * E_k * max(0, <sh_n, l_k>) * vis_k      (t finite, <sh_n,-d> > 0)
 * sh_n, d: 3 device arrays of n floats each (SoA, as hf_si_t.sh_n / hf_rays_t.d); t: n floats (inf = miss);
 * lights: n_lights <= HF_MAX_LIGHTS structs in HOST memory; vis: NULL or n_lights device arrays of n bytes
 * (0 = shadowed: the negated hf_ray_test result of the shadow ray towards light k); image: device,
 * n_lights * (n / spp) floats, overwritten.  n must be a multiple of spp. */
int hf_direct_lighting(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3], const float *t,
                       uint32_t n_lights, const hf_dir_light_t *lights, float albedo, const uint8_t *const *vis,
                       float *image, hf_stream_t stream);
/* Reverse mode of the above with respect to sh_n (what dr.backward propagates into si before it reaches
 * compute_surface_interaction; the cos > 0 masks and the visibility are piecewise constant):
 *   grad_sh_n[i] = 1/spp * sum_k  albedo/pi * E_k * vis_k * grad_image[k][i / spp] * l_k      (same masks)
 * grad_sh_n: 3 device arrays of n floats, overwritten; feed them to hf_adjoint as hf_si_grad_t.sh_n. */
int hf_direct_lighting_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                               const float *t, uint32_t n_lights, const hf_dir_light_t *lights, float albedo,
                               const uint8_t *const *vis, const float *grad_image, float *const grad_sh_n[3],
                               hf_stream_t stream);
/* The same pair with a per-sample WEIGHT (n floats, device): every light's contribution of sample i is multiplied by
 * weight[i] before the film -- the determinant of a reparameterised camera ray, which direct_reparam.py:164-180 /
 * prb_reparam.py:317-366 multiply the sample by.  The adjoint also returns dL/dweight (grad_weight, n floats,
 * overwritten; may be NULL), the gradient that goes on to hf_reparam_*'s divergence input.  weight == NULL: as above. */
int hf_direct_lighting_weighted(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                const float *t, const float *weight, uint32_t n_lights, const hf_dir_light_t *lights,
                                float albedo, const uint8_t *const *vis, float *image, hf_stream_t stream);
int hf_direct_lighting_weighted_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                        const float *t, const float *weight, uint32_t n_lights,
                                        const hf_dir_light_t *lights, float albedo, const uint8_t *const *vis,
                                        const float *grad_image, float *const grad_sh_n[3], float *grad_weight,
                                        hf_stream_t stream);

/* The same under POINT lights (src/emitters/point.cpp:106-123: direction d = position - si.p, radiance
 * intensity / |d|^2): sample value albedo/pi * intensity / r^2 * max(0, <sh_n, l>) with l = (position - p) / r, same
 * masks and film.  p: si.p, 3 device arrays of n floats.  The adjoint returns the gradient with respect to sh_n AND
 * to p (the light direction and the falloff depend on the hit point):
 *   grad_sh_n[i] = sum_k w_k / r^2 * l,   grad_p[i] = sum_k w_k / r^3 * (3 <sh_n, l> l - sh_n),
 *   w_k = 1/spp * albedo/pi * intensity_k * vis_k * grad_image[k][i / spp]            (same masks)
 * both overwritten; feed them to hf_adjoint as hf_si_grad_t.sh_n / .p. */
/* Forward mode of hf_direct_lighting_weighted (the transpose of its adjoint; dr.forward through the term of
 * direct_reparam.py:149-175): for tangents dsh_n (3 arrays of n floats) and dweight (n floats), either may be NULL
 * (zero), the tangent image dimage[k][i / spp] (device, n_lights * (n / spp) floats, overwritten):
 *   dimage[k][i / spp] = 1/spp * sum_s  albedo/pi * E_k * vis_k * (weight <dsh_n, l_k> + dweight <sh_n, l_k>)   (same masks) */
int hf_direct_lighting_weighted_tangent(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                        const float *t, const float *weight, uint32_t n_lights,
                                        const hf_dir_light_t *lights, float albedo, const uint8_t *const *vis,
                                        const float *const dsh_n[3], const float *dweight, float *dimage,
                                        hf_stream_t stream);

typedef struct {
    float position[3];
    float intensity; /* radiant intensity (W/sr) */
} hf_point_light_t;
int hf_point_lighting(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3], const float *t,
                      const float *const p[3], uint32_t n_lights, const hf_point_light_t *lights, float albedo,
                      const uint8_t *const *vis, float *image, hf_stream_t stream);
int hf_point_lighting_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                              const float *t, const float *const p[3], uint32_t n_lights,
                              const hf_point_light_t *lights, float albedo, const uint8_t *const *vis,
                              const float *grad_image, float *const grad_sh_n[3], float *const grad_p[3],
                              hf_stream_t stream);
/* Forward mode of hf_point_lighting (the transpose of hf_point_lighting_adjoint; the term of point.cpp:106-123 under
 * dr.forward): tangents dsh_n and dp (3 arrays of n floats each, either may be NULL = zero) give
 *   dimage[k][i / spp] = sum_s w_k / r^2 (<dsh_n, l> + <dp, 3 <sh_n, l> l - sh_n> / r),  w_k = 1/spp albedo/pi intensity_k vis_k
 * (same masks; dimage overwritten). */
int hf_point_lighting_tangent(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3], const float *t,
                              const float *const p[3], uint32_t n_lights, const hf_point_light_t *lights, float albedo,
                              const uint8_t *const *vis, const float *const dsh_n[3], const float *const dp[3],
                              float *dimage, hf_stream_t stream);

/* ---- next row (emitter sampling): sky lighting, the hemisphere visibility traced in the kernel ----
 *
 * Replaces, for diffuse surfaces under a CONSTANT environment of scalar radiance L (src/emitters/constant.cpp:117-145:
 * direction = square_to_uniform_sphere(sample), pdf 1 / (4 pi), radiance L), the emitter-sampling term of the direct
 * integrator (direct_reparam.py:150-180: detached emitter sample, MIS weight 1 here, attached BSDF value;
 * diffuse.cpp:135-140) averaged over K = num_rays emitter samples per wavefront sample, and the shadow rays it traces.
 *   samples     (r0, r1) = sample_tea_32(sample_tea_32(seed, k)[0], id_i), sample = (r0 >> 9, r1 >> 9) * 2^-23: the
 *               stream of hf_reparam_* with pair = k; id_i = i or ray_id[i] (device, n uint32, may be NULL);
 *   direction   w_k = (r cos 2 pi s.x, r sin 2 pi s.x, z), z = 1 - 2 s.y, r = sqrt(max(0, 1 - z^2)) (warp.h:250-255):
 *               world space, the same for every surface;
 *   eligible    sample i when t_i is finite and <sh_n_i, -d_i> > 0 (the masks of hf_direct_lighting); direction k of
 *               an eligible sample is TRACED when <sh_n_i, w_k> > 0;
 *   shadow ray  SurfaceInteraction::spawn_ray(w_k) (interaction.h:134-136, 161-165): origin p + n s (1 + max|p_c|)
 *               RayEpsilon with n the geometric normal, s = -1 where <n, w_k> < 0, else 1, RayEpsilon = 1500 * 2^-24
 *               (math.h:18-22); maxt = +inf -- the environment lies outside the scene, which is this one shape;
 *   visibility  vis_bits[i], one uint32: bit k is set iff direction k was traced and the any-hit walk found nothing;
 *               samples that are not eligible get 0;
 *   value_i     = weight_i * (4 albedo L / K) * sum_k bit_ik <sh_n_i, w_k>       (albedo/pi * cos * L / pdf, averaged)
 *   image[i / spp] = 1/spp * sum value_i: the box film of hf_direct_lighting, overwritten; n a multiple of spp.
 * The ray takes the float32 direction (what hf_sky_rays writes); the sums of cosines and of directions are formed from
 * the same sample's direction in double and rounded once, here and in the adjoint and the tangent.
 * An unoccluded horizontal plane has expectation albedo * L.  Visibility and the masks are piecewise constant, as in
 * the rows above: the silhouette part of the shadow gradient is hf_reparam_*'s.
 * All four entries: 1 <= num_rays <= 32 (hf_sky_rays: k < 32), n < 2^32; NULL pointers (other than those marked
 * optional), n % spp != 0, num_rays out of range and non-finite radiance / albedo are refused with HF_EINVAL before
 * anything touches a device.  p, nrm, sh_n, d: 3 device rows of n floats (hf_si_t.p / .n / .sh_n, hf_rays_t.d); t: n.
 * Callers detect the entries by their symbols (HF_VERSION is unchanged).
 *
 * hf_sky_rays materialises shadow ray k of every sample (out_o, out_d: 3 rows of n floats; out_maxt: n floats, +inf
 * for a traced lane and -1 -- a miss -- for every other, as hf_reparam_aux_rays marks inactive lanes): the two-call
 * sequence hf_sky_rays + hf_ray_test that hf_sky_lighting equals bit for bit.  Takes no field handle. */
int hf_sky_rays(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                const float *const d[3], const float *t, uint32_t k, uint32_t seed, const uint32_t *ray_id,
                float *const out_o[3], float *const out_d[3], float *out_maxt, hf_stream_t stream);
/* The fused launch: reads a sample's record once, draws its K directions, runs the per-lane any-hit walk for each
 * traced one and writes vis_bits[i] (n uint32, may be NULL = not wanted) and the film; no ray and no per-ray hit
 * byte goes to memory.  A batch of 64 samples without an eligible one (the part of an image beside the terrain) draws
 * nothing.  Every wave walks per lane, whatever hf_set_ray_coherence says: that state is neither read nor changed.
 * weight: n floats or NULL (1).  Allocates nothing, never synchronises the host. */
int hf_sky_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3], const float *const nrm[3],
                    const float *const sh_n[3], const float *const d[3], const float *t, const float *weight,
                    uint32_t num_rays, uint32_t seed, const uint32_t *ray_id, float radiance, float albedo,
                    float *image, uint32_t *vis_bits, hf_stream_t stream);
/* Reverse mode with respect to sh_n and weight.  Traces nothing: the directions are drawn again and vis_bits (as
 * hf_sky_lighting wrote it) is read.  With g = grad_image[i / spp] / spp:
 *   grad_sh_n[i] = g weight_i (4 albedo L / K) sum_k bit_ik w_k,   grad_weight[i] = g (4 albedo L / K) sum_k bit_ik <sh_n_i, w_k>
 * both overwritten (grad_weight may be NULL), exact zeros for samples that are not eligible; sums in k order, no
 * atomics: bitwise the same from launch to launch.  Takes no field handle. */
int hf_sky_lighting_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3], const float *t,
                            const float *weight, uint32_t num_rays, uint32_t seed, const uint32_t *ray_id,
                            float radiance, float albedo, const uint32_t *vis_bits, const float *grad_image,
                            float *const grad_sh_n[3], float *grad_weight, hf_stream_t stream);
/* Forward mode, the transpose of the adjoint: for tangents dsh_n (3 rows of n floats) and dweight (n floats), either
 * may be NULL (zero),
 *   dimage[i / spp] = 1/spp sum (4 albedo L / K) (weight_i sum_k bit_ik <dsh_n_i, w_k> + dweight_i sum_k bit_ik <sh_n_i, w_k>)
 * overwritten.  No atomics for any spp (a power of two <= 64: the film's shuffle tree; otherwise one lane adds the
 * samples of a pixel in order): bitwise the same from launch to launch.  Takes no field handle. */
int hf_sky_lighting_tangent(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3], const float *t,
                            const float *weight, uint32_t num_rays, uint32_t seed, const uint32_t *ray_id,
                            float radiance, float albedo, const uint32_t *vis_bits, const float *const dsh_n[3],
                            const float *dweight, float *dimage, hf_stream_t stream);

/* ---- next row: refractive caustics, light tracing through the surface ----
 *
 * The rows above end at a diffuse surface seen from a camera.  Here every wavefront sample is a LIGHT sample that arrives
 * along d, is refracted at the surface (the `dielectric` BSDF's transmission lobe in importance mode, dielectric.cpp:361)
 * and lands on a receiver plane: sunlight through a water surface onto a pool floor, a caustic lens.  World space.
 *   inputs      p, nrm (the geometric normal g), sh_n (the shading normal m), d: 3 device rows of n floats; t: n floats;
 *               weight: n floats or NULL (1); active: n bytes or NULL (every lane); wi = -d.
 *   constants   eta: the relative index as fresnel() defines it (> 1: the normal points into the less dense side);
 *               power: the flux one sample carries; receiver (HOST memory): the plane through `origin` spanned by ex and
 *               ey, N = normalize(ex x ey); film x = <X - origin, ex>, y = <X - origin, ey>, in pixels.
 *   eligible    t_i is finite, the sample is active, c_i = <m, wi> != 0 and <g, wi> c_i > 0 (both normals agree on the
 *               side; both signs of c_i are served, as fresnel() serves them);
 *   Fresnel     (F, c_t, eta_it, eta_ti) = fresnel(c_i, eta), include/mitsuba/render/fresnel.h:35-71, operation for
 *               operation in float32; cos_theta_t_sqr <= 0 is total internal reflection: nothing is transmitted;
 *   direction   wo = refract(wi, m, c_t, eta_ti) = m (<wi, m> eta_ti + c_t) - wi eta_ti (fresnel.h:311-314);
 *   consistent  <g, wo> <g, wi> < 0: the transmitted ray leaves on the other side of the true surface;
 *   receiver    s = <origin - p, N> / <wo, N>; it is REACHED when s is finite and s > 0;
 *   traced      = eligible, transmitted, consistent and reached;
 *   ray         SurfaceInteraction::spawn_ray(wo) exactly as hf_sky_rays builds it, direction wo, maxt = s: a receiver
 *               that cuts through the terrain's bound clips the walk;
 *   deposited   vis[i] = 1 iff the sample is traced and the any-hit walk of that ray finds nothing;
 *   landing     X = p + s wo, pos = (<X - origin, ex>, <X - origin, ey>);
 *   value       weight_i power (1 - F): no eta^2 factor (importance mode);
 *   every other sample: value = 0, vis = 0, pos = (-16, -16) -- outside every film by more than the filter radius of
 *               hf_film_splat_weighted (4 stddev), whose clamped footprint is then empty.
 * One square root and three divisions per sample (two in fresnel(), one for s); no transcendental, no double precision.
 * The masks and the occlusion are piecewise constant, as in the rows above: the silhouette term is out of scope.
 * pos and value are differentiated with respect to sh_n, p and weight -- through c_i, F, c_t, wo and s, with the sign
 * choices and the masks held; d and the receiver are constants.  With c = c_i, e = eta_ti, q = c e + c_t, b = <wo, N>:
 *   d c_t / d c = -|c| e^2 / |c_t|,   q' = e + d c_t / d c,   F' = a_s a_s' + a_p a_p' (0 for eta = 1),
 *   d wo = d m q + m q' <d m, wi>,   d s = -(<d p, N> + s <d wo, N>) / b,   d X = d p + wo d s + s d wo,
 *   d pos = (<d X, ex>, <d X, ey>),   d value = d weight power (1 - F) - weight power F' <d m, wi>.
 * All four entries refuse with HF_EINVAL, before anything touches a device: NULL pointers (other than those marked
 * optional), n >= 2^32, a non-finite or non-positive eta, a non-finite power, a receiver that is not finite, whose
 * ex x ey is zero or whose ex, ey are not orthogonal to within 1e-5 |ex| |ey|.  Callers detect the entries by their
 * symbols (HF_VERSION is unchanged). */
typedef struct hf_receiver {      /* HOST memory */
    float origin[3];              /* world point at film position (0, 0) */
    float ex[3], ey[3];           /* film x = <X - origin, ex>, y = <X - origin, ey>, in pixels */
} hf_receiver_t;
/* hf_caustic_rays materialises the refracted ray of every sample (out_o, out_d: 3 rows of n floats; out_maxt: n floats,
 * s for a traced lane; every other lane gets -1 -- a miss -- and a zero origin and direction): the two-call sequence
 * hf_caustic_rays + hf_ray_test that hf_caustic_lighting equals bit for bit.  Takes no field handle. */
int hf_caustic_rays(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                    const float *const d[3], const float *t, const uint8_t *active, float eta,
                    const hf_receiver_t *receiver, float *const out_o[3], float *const out_d[3], float *out_maxt,
                    hf_stream_t stream);
/* The fused launch (hf_sky_lighting's mapping: one lane per sample, one workgroup per 256 samples, no work counter):
 * reads a sample's record once, refracts, runs the per-lane any-hit walk with the ray's maxt and writes pos (2 rows of n
 * floats), value (n floats) and vis (n bytes, may be NULL = not wanted); no ray goes to memory.  A batch of 64 samples
 * without a traced lane skips the walk.  Every wave walks per lane, whatever hf_set_ray_coherence says: that state is
 * neither read nor changed.  Allocates nothing, never synchronises the host, capturable. */
int hf_caustic_lighting(const hf_field_t *hf, size_t n, const float *const p[3], const float *const nrm[3],
                        const float *const sh_n[3], const float *const d[3], const float *t, const uint8_t *active,
                        const float *weight, float eta, float power, const hf_receiver_t *receiver, float *const pos[2],
                        float *value, uint8_t *vis, hf_stream_t stream);
/* Reverse mode with respect to sh_n, p and weight.  Traces nothing: the vertex is formed again and vis (as
 * hf_caustic_lighting wrote it) is read.  grad_pos (2 rows) and grad_value may be NULL (zero); grad_sh_n, grad_p (3 rows
 * each) and grad_weight may be NULL (not wanted).  Outputs are overwritten, exact zeros where vis = 0; one lane per
 * sample, no atomics: bitwise the same from launch to launch.  Takes no field handle. */
int hf_caustic_adjoint(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                       const float *const d[3], const float *t, const uint8_t *active, const float *weight, float eta,
                       float power, const hf_receiver_t *receiver, const uint8_t *vis, const float *const grad_pos[2],
                       const float *grad_value, float *const grad_sh_n[3], float *const grad_p[3], float *grad_weight,
                       hf_stream_t stream);
/* Forward mode, the exact transpose of the adjoint: tangents dsh_n, dp (3 rows each) and dweight, each may be NULL (zero);
 * dpos (2 rows) and dvalue are overwritten (either may be NULL = not wanted), exact zeros where vis = 0. */
int hf_caustic_tangent(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                       const float *const d[3], const float *t, const uint8_t *active, const float *weight, float eta,
                       float power, const hf_receiver_t *receiver, const uint8_t *vis, const float *const dsh_n[3],
                       const float *const dp[3], const float *dweight, float *const dpos[2], float *dvalue,
                       hf_stream_t stream);

/* ---- next row: environment-map lighting, importance-sampled, the shadow rays traced in the kernel ----
 *
 * hf_sky_lighting with a direction-dependent environment: the reference's `envmap` emitter (src/emitters/envmap.cpp), one
 * channel, sampled by importance and differentiable in its texels.
 *   data        data[H][W] float32, row-major, scalar radiance, the CALLER's device buffer (W >= 2, H >= 2).  Row 0 is the
 *               map's north pole (theta = 0, local +Y); column W - 1 is the seam column, a copy of column 0
 *               (envmap.cpp:147, 249-258) -- the entries do not check it.
 *   radiance    in cell (cx, cy) at fractions (fx, fy): eval_spectrum's non-spectral branch (envmap.cpp:498-555),
 *               v0 = fma(1 - fx, v00, fx v10), v1 = fma(1 - fx, v01, fx v11), L = fma(1 - fy, v0, fy v1).
 *   direction   of uv = ((cx + fx + 1/2) / (W - 1), (cy + fy) / (H - 1)): theta = pi uv.y, phi = 2 pi uv.x, local
 *               d = (sin theta sin phi, cos theta, -sin theta cos phi) (envmap.cpp:393-397, 406), world w = R d.
 *               rot: 9 HOST floats, a row-major rotation, NULL = identity, detached.
 *   distribution piecewise constant over the (W - 1)(H - 1) bilinear cells (NOT the reference's Hierarchical2D; the sample
 *               streams differ from its PCG32 anyway):  weight_c = sin(pi (cy + 1/2) / (H - 1)) ((1 - u) m_c + u mbar),
 *               m_c = the mean of max(texel, 0) over the cell's corners, mbar = the mean of m_c, u in [0, 1] a DEFENSIVE
 *               fraction given at build time (0: proportional to luminance; > 0 keeps dark texels reachable while the
 *               texels are optimised).  Detached (direct_reparam.py:152-160).  In float32:
 *               m_c = 0.25 ((p00 + p10) + (p01 + p11)), weight_c = s ((1 - u) m_c + u mbar), s the sine evaluated in
 *               double and rounded once; one rounding per operation, nothing fused.
 *   table       hf_envmap_table_floats(W, H) = 4 + (H - 1) + (H - 1)(W - 1) floats, the caller's: header {Sigma, mbar, u,
 *               0}; the marginal M, H - 1 inclusive prefix sums of the row sums (the last is Sigma); the conditional
 *               C[cy], W - 1 inclusive prefix sums of weight_c per cell row.  A conditional entry is the fp64 running sum
 *               of the row's float32 weights in cell order, rounded once; rowsum_cy = C[cy][W - 2]; a marginal entry is
 *               the fp64 running sum of the float32 rowsums in row order, rounded once; mbar = the fp64 sum in row order of
 *               the rows' float32-rounded fp64 sums of m_c, divided by the cell count, rounded once.  Bitwise the same
 *               from build to build.
 *   draw        direction k of sample i from (s.x, s.y), the TEA stream of hf_sky_* (pair = k, id_i = i or ray_id[i]);
 *               float32, one rounding per step:  y = s.y Sigma, cy = the first row with !(M[cy] < y) (H - 2 if none),
 *               fy = clamp((y - M[cy - 1]) / rowsum_cy, 0, 1 - 2^-24) (M[-1] = 0);  x = s.x rowsum_cy, cx = the first cell
 *               with !(C[cy][cx] < x) (W - 2 if none), fx = clamp((x - C[cy][cx - 1]) / weight_c, 0, 1 - 2^-24) with
 *               weight_c RECOMPUTED from the four texels and the header.  Sigma = 0 or weight_c <= 0: the draw is INVALID,
 *               it is not traced and contributes exactly 0 (its fractions are reported as 0: a finite direction).
 *   value       pdf_uv = weight_c (W - 1)(H - 1) / Sigma, pdf_w = pdf_uv / (2 pi^2 sin theta) (envmap.cpp:403-415);
 *               E_k = L_k 2 pi^2 sin theta_k / pdf_uv;
 *               value_i = weight_i (albedo / (pi K)) sum_k bit_ik <sh_n_i, w_k> E_k;  image[i / spp] = 1/spp sum value_i.
 *   masks       hf_sky_lighting's: eligible when t is finite and <sh_n, -d> > 0; direction k is TRACED when the sample is
 *               eligible, the draw valid and <sh_n, w_k> > 0; shadow ray spawn_ray(w_k), maxt = +inf; bit k of vis_bits[i]
 *               is set iff direction k was traced and is unoccluded; the box film and spp as there.
 * The ray takes the float32 direction; the shading sums take the same draw's direction and E_k in double, rounded once.
 * Attached: sh_n, weight and data (through L_k only).  Not differentiated: visibility, the masks, the table, rot.
 * All entries: device pointers and a stream, no allocation, no host synchronisation, capturable without a scratch block.
 * NULL pointers (other than those marked optional), W < 2 or H < 2, u outside [0, 1] or not finite, num_rays outside
 * 1..32 (hf_envmap_rays: k >= 32), n % spp != 0, spp == 0, n >= 2^32 and a non-finite albedo or rot are refused with
 * HF_EINVAL before anything touches a device.  Callers detect the entries by their symbols (HF_VERSION is unchanged). */
/* the table's size in floats; 0 for W < 2 or H < 2 */
size_t hf_envmap_table_floats(uint32_t W, uint32_t H);
/* builds the table of `data` (three launches: the rows' sums of m_c, the conditional rows, the marginal and the header) */
int hf_envmap_build_table(uint32_t W, uint32_t H, const float *data, float u, float *table, hf_stream_t stream);
/* Emitter::sample_direction for caller-supplied samples (sample: 2 device rows of n floats in [0, 1)): out_d the float32
 * direction the rays take, out_weight = E, out_pdf = pdf_w (both 0 for an invalid draw), out_cell = cy (W - 1) + cx
 * (n uint32, may be NULL), out_frac = (fx, fy), the position in the cell (2 rows of n floats, may be NULL).
 * NOTE the parameter list: out_frac is an output that Emitter::sample_direction does not have (the fractions of the draw,
 * which no other output determines bit for bit), and it stands BETWEEN out_cell and stream -- a caller that passes the
 * stream right after out_cell is passing it as out_frac.  Pass NULL there when the fractions are not wanted. */
int hf_envmap_sample_direction(size_t n, const float *const sample[2], uint32_t W, uint32_t H, const float *data,
                               const float *table, const float rot[9], float *const out_d[3], float *out_weight,
                               float *out_pdf, uint32_t *out_cell, float *const out_frac[2], hf_stream_t stream);
/* Emitter::eval for world directions d (envmap.cpp:323-333, 498-509), evaluated in double and rounded once: v = R^T d, uv = (atan2(v.x, -v.z) / 2 pi,
 * acos(clamp(v.y, -1, 1)) / pi), uv.x -= 1/2 / (W - 1), uv -= floor(uv), the cell min(uint(uv (res - 1)), res - 2) and the
 * bilinear value; lanes with active[i] == 0 get 0 (active may be NULL: every lane).  The map is linear in data: called
 * with a tangent of the texels in place of data it is the tangent. */
int hf_envmap_eval(size_t n, const float *const d[3], const uint8_t *active, uint32_t W, uint32_t H, const float *data,
                   const float rot[9], float *out, hf_stream_t stream);
/* its transpose: grad_data[H][W] += grad_out[i] * (bilinear weight) on the four texels of every active lane (each product
 * formed in double and rounded once), float atomics; ACCUMULATED into, like grad_heightfield. */
int hf_envmap_eval_adjoint(size_t n, const float *const d[3], const uint8_t *active, uint32_t W, uint32_t H,
                           const float rot[9], const float *grad_out, float *grad_data, hf_stream_t stream);
/* shadow ray k of every sample, as hf_sky_rays: maxt = +inf where direction k is traced, -1 elsewhere; out_weight (n floats,
 * may be NULL) = E_k, 0 for an invalid draw.  Takes no field handle. */
int hf_envmap_rays(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                   const float *const d[3], const float *t, uint32_t k, uint32_t seed, const uint32_t *ray_id, uint32_t W,
                   uint32_t H, const float *data, const float *table, const float rot[9], float *const out_o[3],
                   float *const out_d[3], float *out_maxt, float *out_weight, hf_stream_t stream);
/* The fused launch (hf_sky_lighting's mapping: one lane per sample, one workgroup per 256 samples, no work counter): equals
 * hf_envmap_rays + hf_ray_test bit for bit in the visibility word.  weight: n floats or NULL (1); vis_bits may be NULL. */
int hf_envmap_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3], const float *const nrm[3],
                       const float *const sh_n[3], const float *const d[3], const float *t, const float *weight,
                       uint32_t num_rays, uint32_t seed, const uint32_t *ray_id, uint32_t W, uint32_t H, const float *data,
                       const float *table, const float rot[9], float albedo, float *image, uint32_t *vis_bits,
                       hf_stream_t stream);
/* Reverse mode.  Traces nothing: the directions are drawn again and vis_bits read.  With g = grad_image[i / spp] / spp,
 * c = albedo / (pi K) and G_k = E_k / L_k:
 *   grad_sh_n[i] = g weight_i c sum_k bit_ik E_k w_k,   grad_weight[i] = g c sum_k bit_ik <sh_n_i, w_k> E_k
 * overwritten (grad_weight may be NULL), sums in k order, no atomics: bitwise the same from launch to launch;
 *   grad_data[texel j of the cell of direction k] += g weight_i c bit_ik <sh_n_i, w_k> G_k b_j   (b: the bilinear weights)
 * accumulated with float atomics; grad_data ([H][W]) may be NULL.  Takes no field handle. */
int hf_envmap_lighting_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3], const float *t,
                               const float *weight, uint32_t num_rays, uint32_t seed, const uint32_t *ray_id, uint32_t W,
                               uint32_t H, const float *data, const float *table, const float rot[9], float albedo,
                               const uint32_t *vis_bits, const float *grad_image, float *const grad_sh_n[3],
                               float *grad_weight, float *grad_data, hf_stream_t stream);
/* Forward mode, the transpose of the adjoint, for tangents dsh_n (3 rows), dweight (n) and ddata ([H][W]; it enters through
 * L_k with the PRIMAL table), each may be NULL (zero); dimage overwritten.  No atomics for any spp. */
int hf_envmap_lighting_tangent(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3], const float *t,
                               const float *weight, uint32_t num_rays, uint32_t seed, const uint32_t *ray_id, uint32_t W,
                               uint32_t H, const float *data, const float *table, const float rot[9], float albedo,
                               const uint32_t *vis_bits, const float *const dsh_n[3], const float *dweight,
                               const float *ddata, float *dimage, hf_stream_t stream);

/* ---- next row: specular reflection of the environment map, the mirror ray traced in the kernel ----
 *
 * The rows above end at a Lambertian surface or refract through it.  Here every wavefront sample is MIRRORED at the surface
 * and sees the environment map: reflect(wi, m) (include/mitsuba/render/fresnel.h:282-284), the reflection lobe of the
 * `dielectric` BSDF (or of a `conductor` idealised to F = 1: eta = 0) and Emitter::eval of src/emitters/envmap.cpp.  World
 * space; the map conventions (W, H, data, rot) are hf_envmap_eval's, and nothing is sampled: no table, no seed.
 *   inputs      p, nrm (the geometric normal g), sh_n (the shading normal m), d: 3 device rows of n floats; t: n floats;
 *               weight: n floats or NULL (1), the specular reflectance; active: n bytes or NULL (every lane); wi = -d.
 *   eligible    the sample is active, t_i is finite, c = <m, wi> > 0 and <g, wi> > 0;
 *   Fresnel     F = fresnel(c, eta)[0] (fresnel.h:35-71) operation for operation in float32, as hf_caustic_lighting has
 *               it; eta == 0 is the ideal mirror: F = 1, F' = 0;
 *   direction   wr = fmsub(m, 2 c, wi) in float32;
 *   consistent  <g, wr> > 0: a reflected ray that would start below the true surface is not traced and contributes 0;
 *   traced      = eligible and consistent;
 *   ray         SurfaceInteraction::spawn_ray(wr) exactly as hf_sky_rays builds it, maxt = +inf, any-hit walk;
 *   visible     vis[i] = 1 iff the sample is traced and the walk finds nothing;
 *   radiance    L = hf_envmap_eval's value for the direction wr (the same lookup, in double, rounded once);
 *   value       value_i = (weight_i F) L in float32 where vis = 1, exactly 0 for every other sample;
 *   image       image[i / spp] = 1/spp sum value_i: the box film of the rows above, overwritten; n a multiple of spp.
 * A reflected ray that hits the terrain contributes 0: a second specular or diffuse vertex is OUT OF SCOPE.
 * Differentiated with respect to sh_n, weight and data; the masks, the visibility, the cell of the lookup and rot are held
 * (the silhouette term belongs to hf_reparam_*).  With v = R^T wr, the cell's fractions (fx, fy), texels v00 .. v11 and
 * bilinear weights b_j:
 *   Lx = (1 - fy)(v10 - v00) + fy (v11 - v01),   Ly = (1 - fx)(v01 - v00) + fx (v11 - v10),
 *   s2 = vx^2 + vz^2,   q = 1 - vy^2,
 *   dL/dv = Lx (W - 1) / (2 pi) (-vz, 0, vx) / s2 + Ly (H - 1) / pi (0, -1 / sqrt(q), 0),   G = R dL/dv,
 *   d wr = 2 (d m c + m <d m, wi>),   F' = a_s a_s' + a_p a_p' (hf_caustic_lighting's; 0 where F = 1 by total reflection),
 *   d value     = d weight F L + weight (F' <d m, wi> L + F <G, d wr>) + weight F sum_j b_j d data_j,
 *   grad_sh_n   = g weight (F' L wi + 2 F (c G + <m, G> wi)),   grad_weight = g F L,   grad_data[j] += g weight F b_j.
 * At the poles of the map (s2 < 1e-12 or q < 1e-12) G is EXACTLY ZERO.  G is formed in double from the same lookup and
 * rounded once.
 * All four entries refuse with HF_EINVAL, before anything touches a device: a NULL pointer that is not optional,
 * n >= 2^32, spp == 0 or n % spp != 0, W < 2 or H < 2, a negative or non-finite eta, a non-finite rot (rot NULL: the
 * identity).  Callers detect the entries by their symbols (HF_VERSION is unchanged). */
/* materialises the reflected ray of every sample (out_o, out_d: 3 rows of n floats; out_maxt: n floats, +inf for a traced
 * lane; every other lane gets -1 -- a miss -- and a zero origin and direction, as hf_caustic_rays does): the two-call
 * sequence hf_reflect_rays + hf_ray_test that hf_reflect_lighting equals bit for bit.  Takes no field handle. */
int hf_reflect_rays(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                    const float *const d[3], const float *t, const uint8_t *active, float *const out_o[3],
                    float *const out_d[3], float *out_maxt, hf_stream_t stream);
/* The fused launch (hf_sky_lighting's mapping: one lane per sample, one workgroup per 256 samples, no work counter):
 * reads a sample's record once, reflects, runs the per-lane any-hit walk, looks the map up and writes image (n / spp
 * floats), value (n floats) and vis (n bytes); each may be NULL (not wanted), but not all three.  No ray goes to memory.
 * A batch of 64 samples without a traced lane skips the walk.  hf_set_ray_coherence is neither read nor changed.
 * Allocates nothing, never synchronises the host, capturable. */
int hf_reflect_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3], const float *const nrm[3],
                        const float *const sh_n[3], const float *const d[3], const float *t, const uint8_t *active,
                        const float *weight, float eta, uint32_t W, uint32_t H, const float *data, const float rot[9],
                        float *image, float *value, uint8_t *vis, hf_stream_t stream);
/* Reverse mode.  Traces nothing: the vertex is formed again and vis (as hf_reflect_lighting wrote it) is read.  The
 * upstream of sample i is g = grad_image[i / spp] / spp + grad_value[i]; either may be NULL (zero).  grad_sh_n (3 rows)
 * and grad_weight are overwritten, exact zeros where vis = 0, one lane per sample, no atomics: bitwise the same from
 * launch to launch; grad_data ([H][W]) is ACCUMULATED with float atomics.  Any of the three may be NULL (not wanted).
 * Takes no field handle. */
int hf_reflect_lighting_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3], const float *t,
                                const uint8_t *active, const float *weight, float eta, uint32_t W, uint32_t H,
                                const float *data, const float rot[9], const uint8_t *vis, const float *grad_image,
                                const float *grad_value, float *const grad_sh_n[3], float *grad_weight, float *grad_data,
                                hf_stream_t stream);
/* Forward mode, the exact transpose of the adjoint, for tangents dsh_n (3 rows), dweight (n) and ddata ([H][W]), each may
 * be NULL (zero); dimage (n / spp) and dvalue (n) are overwritten, either may be NULL (not wanted), not both.  No atomics
 * for any spp (the film tree of the rows above, or one lane per pixel). */
int hf_reflect_lighting_tangent(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3], const float *t,
                                const uint8_t *active, const float *weight, float eta, uint32_t W, uint32_t H,
                                const float *data, const float rot[9], const uint8_t *vis, const float *const dsh_n[3],
                                const float *dweight, const float *ddata, float *dimage, float *dvalue, hf_stream_t stream);

/* ---- next row: glossy reflection of the environment map, a GGX lobe with a learnable roughness ----
 *
 * Between the Lambertian rows and the perfectly smooth interface of hf_reflect_*: the reflection lobe of `roughconductor`
 * / `roughdielectric` (roughconductor.cpp:242-268) with an isotropic GGX MicrofacetDistribution sampled by its visible
 * normals (include/mitsuba/render/microfacet.h).  Every wavefront sample draws K = num_rays microfacet normals, mirrors
 * wi at each, walks the K mirror rays inside one kernel and looks the map up where they escape.  World space; the map
 * conventions (W, H, data, rot) are hf_envmap_eval's; the sample stream is hf_sky_*'s TEA stream with pair = k and
 * id = i or ray_id[i]; no table is used.
 *   inputs      p, nrm (the geometric normal g), sh_n (the shading normal n), d: 3 device rows of n floats; t: n floats;
 *               weight: n floats or NULL (1), the specular reflectance; active: n bytes or NULL (every lane);
 *               alpha: n floats, the isotropic GGX roughness of every sample; wi = -d.
 *   roughness   a = max(alpha_i, 1e-4) (configure(), microfacet.h:426); a non-finite alpha_i makes the sample ineligible;
 *   eligible    the sample is active, t_i is finite, alpha_i is finite, c_i = <n, wi> > 0 and <g, wi> > 0;
 *   draw k      in float32, one rounding per operation, the same device function in every kernel of the row:
 *               (s, t) = coordinate_system(n);  wi_l = (<wi, s>, <wi, t>, <wi, n>);
 *               the visible-normal branch of MicrofacetDistribution::sample (microfacet.h:297-319):
 *                 wi_p = normalize(a wi_l.x, a wi_l.y, wi_l.z)  (v * (1 / sqrt(<v, v>)));
 *                 (sin_phi, cos_phi) = Frame3f::sincos_phi(wi_p) (frame.h:111-122): (0, 1) where fma(x, x, y y) <= 2^-22;
 *                 the GGX branch of sample_visible_11(wi_p.z, .) (microfacet.h:405-420) on the concentric disk point
 *                 (px, py) of hf_bounce_*'s draw for the TEA sample: s = (1 + wi_p.z) / 2,
 *                 y = lerp(safe_sqrt(1 - px^2), py, s), x = px, z = safe_sqrt(1 - (x^2 + y^2)),
 *                 sin_i = safe_sqrt(1 - wi_p.z^2), norm = 1 / fma(sin_i, y, wi_p.z z),
 *                 slope = (fmsub(wi_p.z, y, sin_i z), x) norm;
 *                 slope = (fmsub(cos_phi, slope.x, sin_phi slope.y) a, fmadd(sin_phi, slope.x, cos_phi slope.y) a);
 *                 h_l = normalize(-slope.x, -slope.y, 1);
 *               h = Frame(n).to_world(h_l) = fma(n, h_l.z, fma(t, h_l.y, s h_l.x));
 *   valid       every component of h is finite and <wi, h> > 0;
 *   direction   wo = fmsub(h, 2 <wi, h>, wi) in float32 (hf_reflect_lighting's expression with h for the normal);
 *   traced      direction k is traced iff the sample is eligible, the draw is valid, c_o = <n, wo> > 0 and <g, wo> > 0;
 *   ray         SurfaceInteraction::spawn_ray(wo) exactly as hf_sky_rays builds it, maxt = +inf, any-hit walk;
 *   visible     bit k of vis_bits[i] is set iff direction k is traced and the walk finds nothing;
 *   Fresnel     F_k = fresnel(<wi, h>, eta)[0] in hf_reflect_lighting's arithmetic; eta == 0: F = 1;
 *   Smith term  frame-free; smith_g1 (microfacet.h:341-365) for unit vectors and an isotropic lobe:
 *               T(c) = a^2 max(fnmadd(c, c, 1), 0) / (c c),   G1(c) = 2 / (1 + sqrt(1 + T));
 *   radiance    L_k = hf_envmap_eval's value for the direction wo_k (in double, rounded once);
 *   value       value_i = weight_i / K sum_k bit_ik (F_k G1(c_o,k)) L_k, summed in k order in float32: the weight of a
 *               visible-normal sample (roughconductor.cpp:262) times the radiance; exactly 0 for a sample without a bit;
 *   image       image[i / spp] = 1/spp sum value_i: the box film of the rows above, overwritten; n a multiple of spp.
 * OUT OF SCOPE: a reflected ray that hits the terrain contributes 0 (no second vertex, as DESIGN 4.19); anisotropy;
 * the Beckmann distribution; a complex index of refraction (weight carries the reflectance); the transmission lobe; the
 * silhouette term (it belongs to hf_reparam_*).  The per-sample deviation of the estimator grows as alpha falls (about
 * 10 at alpha = 0.1 against 1 at 0.6 under a smooth map): near-mirrors belong to hf_reflect_*.
 * Differentiated with respect to sh_n, weight, alpha and data.  Held, in world space: the drawn h_k and wo_k, hence
 * F_k, the lookup's cell and fractions, the masks and the visibility -- the detached sample with attached evaluation
 * of prb.py:213-223, as hf_bounce_*: of the ratio f cos / pdf_det the numerator D(c_h) G1(c_i) G1(c_o) F / (4 c_i) is
 * attached.  With c_h = <n, h>, q = c_h^2 (a^2 - 1) + 1, r = sqrt(1 + T), v = wi for c_i and wo for c_o:
 *   d ln D / d c_h = -4 c_h (a^2 - 1) / q,   d ln D / d a = 2 / a - 4 c_h^2 a / q,
 *   d G1 / d T = -1 / ((1 + r)^2 r),   d T / d c = -2 a^2 / c^3,   d T / d a = 2 a max(1 - c^2, 0) / c^2,
 *   dG1(c) = d G1 / d T (d T / d c <dn, v> + d T / d a da),   da = dalpha_i where alpha_i > 1e-4, else 0,
 *   dlnA_k = d ln D / d c_h <dn, h> + d ln D / d a da + dG1(c_i) / G1(c_i) - <dn, wi> / c_i,
 *   dvalue_i = dweight_i (value_i / weight_i)
 *              + weight_i / K sum_k bit_ik F_k [ L_k (G1(c_o) dlnA_k + dG1(c_o)) + G1(c_o) sum_j b_j ddata_j ].
 * The formulas take n as it comes, through the three cosines only: they are the derivative for unit n and tangential
 * dn, which the normalisation of the surface interaction supplies.
 * All four entries refuse with HF_EINVAL, before anything touches a device: a NULL pointer that is not optional (alpha
 * included), n >= 2^32, spp == 0 or n % spp != 0, num_rays outside 1..32 (hf_glossy_rays: k >= 32), W < 2 or H < 2, a
 * negative or non-finite eta, a non-finite rot (rot NULL: the identity).  They take device pointers and a stream,
 * allocate nothing, never synchronise the host and are capturable.  Callers detect the entries by their symbols
 * (HF_VERSION is unchanged). */
/* materialises mirror ray k of every sample (out_o, out_d: 3 rows of n floats; out_maxt: n floats, +inf for a traced
 * lane; every other lane gets -1 -- a miss -- and a zero origin and direction, as hf_reflect_rays): the two-call
 * sequence hf_glossy_rays + hf_ray_test that bit k of hf_glossy_lighting's vis_bits equals.  out_h (3 rows, may be NULL):
 * the microfacet normal h of an eligible sample, zero for an invalid draw.  Takes no field handle. */
int hf_glossy_rays(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                   const float *const d[3], const float *t, const uint8_t *active, const float *alpha, uint32_t k,
                   uint32_t seed, const uint32_t *ray_id, float *const out_o[3], float *const out_d[3], float *out_maxt,
                   float *const out_h[3], hf_stream_t stream);
/* The fused launch (hf_sky_lighting's mapping: one lane per sample, one workgroup per 256 samples, no work counter, a
 * wave-uniform loop over the K directions): writes image (n / spp floats), value (n floats) and vis_bits (n words);
 * each may be NULL (not wanted), but not all three.  No ray goes to memory.  A batch of 64 samples without an eligible
 * lane draws nothing.  hf_set_ray_coherence is neither read nor changed. */
int hf_glossy_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3], const float *const nrm[3],
                       const float *const sh_n[3], const float *const d[3], const float *t, const uint8_t *active,
                       const float *weight, const float *alpha, float eta, uint32_t num_rays, uint32_t seed,
                       const uint32_t *ray_id, uint32_t W, uint32_t H, const float *data, const float rot[9], float *image,
                       float *value, uint32_t *vis_bits, hf_stream_t stream);
/* Reverse mode, the exact transpose of the tangent.  Traces nothing: the draws are formed again and vis_bits (as
 * hf_glossy_lighting wrote it) is read; it takes no field handle and no p / nrm: a set bit implies the masks.  The
 * upstream of sample i is g = grad_image[i / spp] / spp + grad_value[i]; either may be NULL (zero).  grad_sh_n (3 rows),
 * grad_weight and grad_alpha are overwritten, exact zeros where no bit is set, one lane per sample, sums in k order, no
 * atomics: bitwise the same from launch to launch; grad_data ([H][W]) is ACCUMULATED with float atomics, as
 * hf_reflect_lighting_adjoint does.  Any of the four may be NULL (not wanted). */
int hf_glossy_lighting_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3], const float *t,
                               const uint8_t *active, const float *weight, const float *alpha, float eta, uint32_t num_rays,
                               uint32_t seed, const uint32_t *ray_id, uint32_t W, uint32_t H, const float *data,
                               const float rot[9], const uint32_t *vis_bits, const float *grad_image,
                               const float *grad_value, float *const grad_sh_n[3], float *grad_weight, float *grad_alpha,
                               float *grad_data, hf_stream_t stream);
/* Forward mode for tangents dsh_n (3 rows), dweight (n), dalpha (n) and ddata ([H][W]), each may be NULL (zero); dimage
 * (n / spp) and dvalue (n) are overwritten, either may be NULL (not wanted), not both.  No atomics for any spp (the film
 * tree of the rows above, or one lane per pixel). */
int hf_glossy_lighting_tangent(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3], const float *t,
                               const uint8_t *active, const float *weight, const float *alpha, float eta, uint32_t num_rays,
                               uint32_t seed, const uint32_t *ray_id, uint32_t W, uint32_t H, const float *data,
                               const float rot[9], const uint32_t *vis_bits, const float *const dsh_n[3],
                               const float *dweight, const float *dalpha, const float *ddata, float *dimage, float *dvalue,
                               hf_stream_t stream);

/* ---- next row: the refraction view, a textured plane seen through the surface ----
 *
 * The camera side of transmission, the other half of the `dielectric` BSDF that hf_reflect_* started: every wavefront
 * sample is a CAMERA sample that looks along d, is refracted at the surface (the transmission lobe in radiance mode,
 * src/bsdfs/dielectric.cpp:263-288, 358-363: the factor eta_ti^2 that hf_caustic_lighting leaves out), walked against the
 * terrain up to a receiver plane and sees the bitmap texture the plane carries (src/textures/bitmap.cpp:400, 497-520)
 * through a homogeneous absorbing medium below the surface.  A pool floor through water, a print through a glass relief.
 *   vertex      the inputs, eligible, Fresnel (fresnel.h:35-71), direction (fresnel.h:311-314), consistent, receiver,
 *               traced, ray (maxt = s), landing and pos are EXACTLY hf_caustic_lighting's, both signs of c_i included;
 *               vis[i] = 1 iff the sample is traced and the any-hit walk of that ray finds nothing.  The materialised ray
 *               is hf_caustic_rays': hf_caustic_rays + hf_ray_test equals vis bit for bit.
 *   texture     tex[TH][TW] float32, row-major, scalar, the CALLER's device buffer.  A film position of the receiver is a
 *               texel coordinate: texel (ix, iy) has its centre at pos = (ix + 0.5, iy + 0.5) -- the bitmap's
 *               fmadd(uv, res, -0.5) with uv = pos / res.  Per axis, in float32: q = pos - 0.5, i0 = floor(q), f = q - i0;
 *               the texels are wrap(i0) and wrap(i0 + 1), HF_WRAP_CLAMP: min(max(i, 0), res - 1), HF_WRAP_REPEAT: the
 *               non-negative remainder of i by res.
 *   lookup      v0 = fma(1 - fx, v00, fx v10), v1 = fma(1 - fx, v01, fx v11), L = fma(1 - fy, v0, fy v1);
 *               with the cell held  Lx = (1 - fy)(v10 - v00) + fy (v11 - v01),  Ly = (1 - fx)(v01 - v00) + fx (v11 - v10)
 *               (under clamp zero outside the texture of its own accord); b_j: the bilinear weights of the four texels.
 *               A coordinate that is not finite or has |q| >= 2^23: under clamp it reads what a float clamp of q to
 *               [-1, res] reads (the border texel, f = 0); under repeat L = 0 and every derivative is zero.
 *   value       a = weight_i (1 - F) (weight NULL: 1 - F),  b = a (eta_ti eta_ti),  T = expf(-sigma_t s) (the accurate
 *               float32 exponential; sigma_t == 0: no T at all),  value_i = (b T) L(pos) in float32 where vis = 1, exactly
 *               0 elsewhere; pos = (-16, -16) where vis = 0.
 *   image       image[i / spp] = 1/spp sum value_i: the box film of the rows above, overwritten; n a multiple of spp.
 * Differentiated with respect to sh_n, p, weight and tex; the masks, the visibility, the sign choices, the cell, d, the
 * receiver, eta and sigma_t are held.  With hf_caustic_lighting's d pos and d s and e2 = eta_ti^2:
 *   d value = d weight (1 - F) e2 T L
 *           + weight e2 T (-F' <d m, wi> L - (1 - F) sigma_t L d s + (1 - F) (Lx d pos_x + Ly d pos_y))
 *           + weight (1 - F) e2 T sum_j b_j d tex_j.
 * OUT OF SCOPE: a gradient for sigma_t, RGB, the mirror wrap, a second vertex (a transmitted ray that hits the terrain
 * contributes 0).
 * All five entries refuse with HF_EINVAL, before anything touches a device: a NULL pointer that is not optional,
 * n >= 2^32, spp == 0 or n % spp != 0, TW == 0, TH == 0 or TW TH >= 2^31, a wrap that is neither constant, a non-finite or
 * non-positive eta, a negative or non-finite sigma_t, an invalid receiver (hf_caustic_*'s checks).  Callers detect the
 * entries by their symbols (HF_VERSION is unchanged). */
#define HF_WRAP_CLAMP 0
#define HF_WRAP_REPEAT 1
/* the lookup alone, for film positions pos (2 device rows of n floats): out (n floats) = L, 0 on lanes with active[i] == 0
 * (active NULL: every lane); out_grad (2 rows: Lx, Ly; zero on inactive lanes) may be NULL (not wanted).  The map is
 * linear in tex: called with a tangent of the texels in place of tex it is the tangent, as hf_envmap_eval. */
int hf_bitmap_eval(size_t n, const float *const pos[2], const uint8_t *active, uint32_t TW, uint32_t TH, const float *tex,
                   int wrap, float *out, float *const out_grad[2], hf_stream_t stream);
/* its transpose: grad_pos (2 rows, OVERWRITTEN, zero on inactive lanes) = grad_out (Lx, Ly); grad_tex[TH][TW] +=
 * grad_out[i] b_j on the four texels of every active lane, float atomics, ACCUMULATED into.  Either may be NULL (not
 * wanted), not both. */
int hf_bitmap_eval_adjoint(size_t n, const float *const pos[2], const uint8_t *active, uint32_t TW, uint32_t TH,
                           const float *tex, int wrap, const float *grad_out, float *const grad_pos[2], float *grad_tex,
                           hf_stream_t stream);
/* The fused launch (hf_reflect_lighting's shape: one lane per sample, one workgroup per 256 samples, no work counter):
 * reads a sample's record once, refracts, runs the per-lane any-hit walk with maxt = s, looks the texture up where the ray
 * lands and writes image (n / spp floats), value (n floats), vis (n bytes) and pos (2 rows of n floats); each may be NULL
 * (not wanted), but not all four.  No ray goes to memory.  A batch of 64 samples without a traced lane skips the walk.
 * hf_set_ray_coherence is neither read nor changed.  Allocates nothing, never synchronises the host, capturable. */
int hf_refract_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3], const float *const nrm[3],
                        const float *const sh_n[3], const float *const d[3], const float *t, const uint8_t *active,
                        const float *weight, float eta, float sigma_t, const hf_receiver_t *receiver, uint32_t TW,
                        uint32_t TH, const float *tex, int wrap, float *image, float *value, uint8_t *vis,
                        float *const pos[2], hf_stream_t stream);
/* Reverse mode.  Traces nothing: the vertex is formed again and vis (as hf_refract_lighting wrote it) is read.  The
 * upstream of sample i is g = grad_image[i / spp] / spp + grad_value[i]; either may be NULL (zero).  grad_sh_n, grad_p
 * (3 rows each) and grad_weight are overwritten, exact zeros where vis = 0, one lane per sample, no atomics: bitwise the
 * same from launch to launch; grad_tex ([TH][TW]) is ACCUMULATED with float atomics.  Any of the four may be NULL (not
 * wanted).  Takes no field handle. */
int hf_refract_lighting_adjoint(size_t n, uint32_t spp, const float *const p[3], const float *const nrm[3],
                                const float *const sh_n[3], const float *const d[3], const float *t, const uint8_t *active,
                                const float *weight, float eta, float sigma_t, const hf_receiver_t *receiver, uint32_t TW,
                                uint32_t TH, const float *tex, int wrap, const uint8_t *vis, const float *grad_image,
                                const float *grad_value, float *const grad_sh_n[3], float *const grad_p[3],
                                float *grad_weight, float *grad_tex, hf_stream_t stream);
/* Forward mode, the exact transpose of the adjoint, for tangents dsh_n, dp (3 rows each), dweight (n) and dtex
 * ([TH][TW]), each may be NULL (zero); dimage (n / spp) and dvalue (n) are overwritten, either may be NULL (not wanted),
 * not both.  No atomics for any spp (the film tree of the rows above, or one lane per pixel). */
int hf_refract_lighting_tangent(size_t n, uint32_t spp, const float *const p[3], const float *const nrm[3],
                                const float *const sh_n[3], const float *const d[3], const float *t, const uint8_t *active,
                                const float *weight, float eta, float sigma_t, const hf_receiver_t *receiver, uint32_t TW,
                                uint32_t TH, const float *tex, int wrap, const uint8_t *vis, const float *const dsh_n[3],
                                const float *const dp[3], const float *dweight, const float *dtex, float *dimage,
                                float *dvalue, hf_stream_t stream);

/* ---- next row: area-light lighting, soft shadows from a rectangle emitter traced in the kernel ----
 *
 * Replaces, for diffuse surfaces under ONE one-sided `area` emitter on a `rectangle` (src/emitters/area.cpp,
 * src/shapes/rectangle.cpp: a lamp, a softbox, a light panel), the emitter-sampling term of the direct integrator
 * (direct_reparam.py:150-180: detached emitter sample, MIS weight 1 here, attached BSDF value; diffuse.cpp:135-140)
 * averaged over K = num_rays points of the lamp per wavefront sample, and the shadow rays it traces.  The direction
 * towards the lamp, the inverse-square falloff and the lamp's own cosine depend on the hit point, and the shadows have a
 * penumbra; the terrain is the RECEIVER (a heightfield that carries an emitter is the adapter's business).
 *   lamp        hf_rect_light_t, HOST memory: the rectangle's to_world as the centre and the images ex, ey of (1, 0, 0)
 *               and (0, 1, 0) (the rectangle spans [-1, 1]^2); n_l = normalize(ex x ey), A = 4 |ex x ey|
 *               (rectangle.cpp:104-108, 144-146), both formed in double on the host; radiance: the scalar L.  The lamp
 *               emits on the side of n_l only (area.cpp:128).
 *   samples     (s.x, s.y) of draw k of sample i: the TEA stream of hf_sky_* (pair = k, id_i = i or ray_id[i]);
 *   point       q_k = center + (2 s.x - 1) ex + (2 s.y - 1) ey (rectangle.cpp:152-166): uniform in area, detached;
 *   geometry    u = q_k - p, r = |u|, w = u / r, c_s = <sh_n, w>, c_l = -<n_l, w>;
 *   eligible    sample i when t_i is finite and <sh_n_i, -d_i> > 0 (the masks of hf_direct_lighting); draw k of an
 *               eligible sample is TRACED when c_s > 0, c_l > 0 and r is finite and > 0 -- decided in float32 on the
 *               signs of <sh_n, u> and <n_l, u> and on r^2;
 *   shadow ray  Interaction::spawn_ray_to(q_k) (interaction.h:141-147, 161-165): origin o = p + n s (1 + max|p_c|)
 *               RayEpsilon with n the geometric normal, s = -1 where <n, u> < 0, else 1; direction (q_k - o) / |q_k - o|;
 *               maxt = |q_k - o| (1 - ShadowEpsilon), ShadowEpsilon = 10 RayEpsilon (math.h:18-22);
 *   visibility  vis_bits[i], one uint32: bit k is set iff draw k was traced and the any-hit walk found nothing before
 *               maxt; samples that are not eligible get 0;
 *   radiance    L_k = radiance without a texture (tex == NULL; TW, TH are then not read); else radiance times the
 *               bilinear lookup of tex[TH][TW] (float32, row-major, the caller's device buffer) at the texel coordinate
 *               (s.x TW, s.y TH) by hf_bitmap_eval's rules under HF_WRAP_CLAMP (bitmap.cpp:497-520).  The coordinate is a
 *               function of the detached draw only: there are no Lx, Ly terms;
 *   value_i     = weight_i (albedo A / (pi K)) sum_k bit_ik L_k c_s c_l / r^2: albedo/pi * c_s * L / pdf with the
 *               solid-angle pdf r^2 / (A c_l) (shape.cpp:364-380), averaged;
 *   image[i / spp] = 1/spp * sum value_i: the box film of hf_direct_lighting, overwritten; n a multiple of spp.
 * The ray takes float32 quantities (what hf_rect_rays writes); every term of the shading sums -- G = c_s c_l / r^2, its
 * derivatives -- is formed from the same draw in double (the texture's lookup is float32, hf_bitmap_eval's expression),
 * the terms are added in double in k order and the sum is rounded once, in the forward, the adjoint and the tangent.
 * Differentiated with respect to sh_n, p, weight and tex.  HELD: the visibility, the masks, the draw, the lamp.  With
 * G = c_s c_l / r^2:   dG/dsh_n = w c_l / r^2,   dG/dp = (4 c_s c_l w - c_l sh_n + c_s n_l) / r^3
 * (a lamp that faces the sample, c_l = 1 and n_l = -w, gives hf_point_lighting's (3 c_s w - sh_n) / r^3).  The silhouette
 * part of the shadow gradient is hf_reparam_*'s, as in the rows above.
 * OUT OF SCOPE: a gradient for the lamp's pose or its radiance scalar, importance sampling of the texture or of the solid
 * angle, RGB, two-sided lamps, MIS with BSDF sampling, several lamps per call (call once per lamp and add the images).
 * All four entries refuse with HF_EINVAL, before anything touches a device: a NULL pointer that is not optional,
 * n >= 2^32, spp == 0 or n % spp != 0, num_rays outside 1..32 (hf_rect_rays: k >= 32), a non-finite field of the lamp, a
 * non-finite albedo, |ex x ey| == 0, and with tex != NULL: TW == 0, TH == 0 or TW TH >= 2^31.  p, nrm, sh_n, d: 3 device
 * rows of n floats; t: n.  Callers detect the entries by their symbols (HF_VERSION is unchanged). */
typedef struct hf_rect_light {
    float center[3], ex[3], ey[3];   /* the rectangle's to_world: the centre, the images of (1, 0, 0) and (0, 1, 0) */
    float radiance;                  /* scalar L; multiplies the texture if there is one */
} hf_rect_light_t;                   /* HOST memory, as hf_receiver_t */
/* the lamp alone, no wavefront: area = A and normal = n_l as the entries below form them, rounded to float (either may be
 * NULL); refuses what they refuse of a lamp.  Host only, touches no device. */
int hf_rect_light_geometry(const hf_rect_light_t *light, float *area, float normal[3]);
/* hf_rect_rays materialises shadow ray k of every sample (out_o, out_d: 3 rows of n floats; out_maxt: n floats, the
 * finite maxt above for a traced lane; a lane that is not traced gets a zero origin and direction and maxt = -1, a miss):
 * the two-call sequence hf_rect_rays + hf_ray_test that hf_rect_lighting equals bit for bit.  Takes no field handle. */
int hf_rect_rays(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                 const float *const d[3], const float *t, uint32_t k, uint32_t seed, const uint32_t *ray_id,
                 const hf_rect_light_t *light, float *const out_o[3], float *const out_d[3], float *out_maxt,
                 hf_stream_t stream);
/* The fused launch (hf_sky_lighting's shape): reads a sample's record once, draws its K points, runs the per-lane any-hit
 * walk up to maxt for each traced one and writes vis_bits[i] (n uint32, may be NULL = not wanted) and the film; no ray
 * and no per-ray hit byte goes to memory.  A batch of 64 samples without an eligible one draws nothing.
 * hf_set_ray_coherence is neither read nor changed.  weight: n floats or NULL (1).  Allocates nothing, never
 * synchronises the host, capturable. */
int hf_rect_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3], const float *const nrm[3],
                     const float *const sh_n[3], const float *const d[3], const float *t, const float *weight,
                     uint32_t num_rays, uint32_t seed, const uint32_t *ray_id, const hf_rect_light_t *light, uint32_t TW,
                     uint32_t TH, const float *tex, float albedo, float *image, uint32_t *vis_bits, hf_stream_t stream);
/* Reverse mode with respect to sh_n, p, weight and tex.  Traces nothing: the points are drawn again and vis_bits (as
 * hf_rect_lighting wrote it) is read.  With g = grad_image[i / spp] / spp and c = albedo A / (pi K):
 *   grad_sh_n[i] = g weight_i c sum_k bit_ik L_k dG/dsh_n,   grad_p[i] = g weight_i c sum_k bit_ik L_k dG/dp,
 *   grad_weight[i] = g c sum_k bit_ik L_k G
 * overwritten, exact zeros for samples that are not eligible; sums in k order, no atomics: bitwise the same from launch to
 * launch.  grad_tex[TH][TW] += g weight_i c radiance G b_j on the four texels of every visible draw: float atomics,
 * ACCUMULATED into (ignored without a texture).  grad_sh_n, grad_p (3 rows each), grad_weight and grad_tex may each be
 * NULL (not wanted).  Takes no field handle. */
int hf_rect_lighting_adjoint(size_t n, uint32_t spp, const float *const p[3], const float *const sh_n[3],
                             const float *const d[3], const float *t, const float *weight, uint32_t num_rays,
                             uint32_t seed, const uint32_t *ray_id, const hf_rect_light_t *light, uint32_t TW, uint32_t TH,
                             const float *tex, float albedo, const uint32_t *vis_bits, const float *grad_image,
                             float *const grad_sh_n[3], float *const grad_p[3], float *grad_weight, float *grad_tex,
                             hf_stream_t stream);
/* Forward mode, the exact transpose of the adjoint, for tangents dsh_n, dp (3 rows of n floats each), dweight (n) and dtex
 * ([TH][TW]; ignored without a texture), each may be NULL (zero); dimage (n / spp) is overwritten.  No atomics for any
 * spp (a power of two <= 64: the film's shuffle tree; otherwise one lane adds the samples of a pixel in order): bitwise
 * the same from launch to launch.  Takes no field handle. */
int hf_rect_lighting_tangent(size_t n, uint32_t spp, const float *const p[3], const float *const sh_n[3],
                             const float *const d[3], const float *t, const float *weight, uint32_t num_rays,
                             uint32_t seed, const uint32_t *ray_id, const hf_rect_light_t *light, uint32_t TW, uint32_t TH,
                             const float *tex, float albedo, const uint32_t *vis_bits, const float *const dsh_n[3],
                             const float *const dp[3], const float *dweight, const float *dtex, float *dimage,
                             hf_stream_t stream);

/* ---- the sensor: the primary wavefront of a perspective or an orthographic camera, differentiable ----
 *
 * Replaces Sensor::sample_ray of `perspective` (src/sensors/perspective.cpp:198-234) and `orthographic`
 * (src/sensors/orthographic.cpp:119-142) together with the wavefront's sample positions (src/render/integrator.cpp:
 * 251-268, src/python/python/ad/integrators/common.py:309-337), in one launch.
 *   sensor      hf_sensor_t, HOST memory.  to_world: row-major 3x4 [A | c] (the layout of hf_desc_t.to_world; here in
 *               double, as every real field, because the constants below are formed in double); x_fov: degrees along x
 *               (perspective only); the film's size and its crop window in pixels (crop_offset = (crop_x, crop_y),
 *               crop_size = (crop_w, crop_h); no crop: 0, 0, film_w, film_h).
 *   index       sample i of the call has the wavefront index id_i = start + i, or ray_id[i] when the device row ray_id
 *               is given (hf_reparam_*'s convention: a rank's tiles draw the samples of the unsharded wavefront);
 *   pixel       pix = id / spp, py = pix / crop_w, px = pix - py crop_w (integrator.cpp:251-268: the wavefront covers
 *               the crop window);
 *   jitter      (jx, jy) = (v0 >> 9, v1 >> 9) 2^-23 with (v0, v1) = sample_tea_32(seed, id) (random.h:76-91);
 *   pos         = (px + crop_x + jx, py + crop_y + jy): the film position in pixels of the WHOLE film (common.py:331-337),
 *               written to out_pos (2 rows, may be NULL);
 *   g           = pos / film_size: the sample s = (pos - crop_offset) / crop_size of sample_ray carried through the crop
 *               window by camera_to_sample (sensor.h:238-240, 256-259), g = (crop_offset + s crop_size) / film_size;
 *   w           = (1 - 2 g.x, (1 - 2 g.y) / a),  a = film_w / film_h (sensor.h:242, 260-261).
 * HF_SENSOR_PERSPECTIVE, with tau = tan(x_fov pi / 360) (transform.h:216-233):
 *   v = (w.x tau, w.y tau, 1): sample_to_camera's near-plane point over near (perspective.cpp:216-219),
 *   d_c = v / |v| (:222),   ray.d = A d_c, not renormalised (:225),   ray.o = c + near A v = c + ray.d near / d_c.z
 *   (:224-230),   maxt = (far - near) |v| (:227-231).
 * HF_SENSOR_ORTHOGRAPHIC (orthographic.cpp:119-142; sensor.h:266-301):
 *   o = A (w.x, w.y, near)^T + c,   d = normalize(A e_z),   maxt = far - near.
 * Everything is formed in double and rounded once to float32.  out_o, out_d: 3 rows of n floats; out_maxt: n floats.
 * One grid-stride launch; allocates nothing, never synchronises the host, capturable.  The kernel takes four consecutive
 * samples per lane and stores 16 bytes per row where the row is aligned: its grid is family 1 of
 * hf_grid_blocks for (n - head) / 4 items, head <= 3 (for n items with HF_SENSOR_STORE=dword, and below 64 samples).
 *
 * Differentiated with respect to to_world (all 12 entries, unconstrained, as the shape's) and x_fov, with
 * d tau = (pi / 360) (1 + tau^2) d fov; maxt, the jitter and the pixel are HELD.  With u = (w.x, w.y, 0):
 *   perspective   d v = u d tau,   d d_c = (d v - d_c <d_c, d v>) / |v|,   d ray.d = dA d_c + A d d_c,
 *                 d ray.o = dc + near (dA v + A d v);
 *   orthographic  d o = dA (w.x, w.y, near)^T + dc,   d d = (dA e_z - d <d, dA e_z>) / |A e_z|;  x_fov is not read.
 * hf_sensor_rays_tangent: d_to_world (12 device floats) and d_fov (1 device float), either may be NULL (zero); writes
 * out_do, out_dd (3 rows of n floats each); per lane, no atomics.  hf_sensor_rays_adjoint: the exact transpose; grad_o,
 * grad_d (3 rows of n floats, either may be NULL = zero) are reduced into grad_to_world (12 device floats) and grad_fov
 * (1 device float; the orthographic type leaves it untouched), both ACCUMULATED into, either may be NULL.  No float
 * atomics: every block stores its 13 partial sums in double to `workspace` -- hf_sensor_workspace_floats() floats of
 * device memory, 8-byte aligned, the caller's, exclusively this call's until it has completed -- and one more launch adds
 * them in a fixed order (family 2 of hf_grid_blocks): bitwise the same from launch to launch, capturable.
 * OUT OF SCOPE: the principal point offset, sample_border, the d_x / d_y of sample_ray_differential, wavelengths and
 * time.  (The thin lens is hf_thinlens_*, below.)
 *
 * hf_sensor_project is the way back, the perspective sensor's sample_direction (perspective.cpp:279-318, 334-383), for
 * points p (3 device rows of n floats) and an optional byte row `active` (NULL: every lane):
 *   ref       = to_world^-1 p; the affine inverse is formed once on the host in double (:283-284);
 *   inside_z  = active and near <= ref.z <= far (:289);
 *   g         = ((1 - ref.x / (ref.z tau)) / 2, (1 - a ref.y / (ref.z tau)) / 2): camera_to_sample in units of the whole
 *               film; s_crop = (g film_size - crop_offset) / crop_size;   valid = inside_z and s_crop in [0, 1]^2 (:299);
 *   uv        = s_crop crop_size + crop_offset = g film_size (:304, common.py:383-400): the pos of hf_sensor_rays, so the
 *               projection of a point of sample i's ray is pos_i;
 *   weight    = importance(local_d) / dist^2 = |ref| / (A' ref.z^3),   A' = (2 tau)^2 / a (crop_w crop_h) / (film_w film_h)
 *               (:317, 340-345, 372-382).
 * Written, a stated deviation from the reference's early returns: uv (2 rows) for every inside_z lane and zeros
 * elsewhere; valid (n bytes); weight (n floats, may be NULL), zero unless valid.  The derivatives of uv are taken where
 * inside_z and those of weight where valid, with respect to p (per lane), to_world and x_fov, with
 * d ref = A^-1 (dp - dA ref - dc); the masks are HELD.  hf_sensor_project_tangent: dp (3 rows), d_to_world (12 device
 * floats), d_fov (1 device float), each may be NULL (zero); writes duv (2 rows) and dweight (may be NULL).
 * hf_sensor_project_adjoint: grad_uv (2 rows) and grad_weight, either may be NULL (zero); grad_p (3 rows, may be NULL) is
 * OVERWRITTEN, grad_to_world and grad_fov are ACCUMULATED into through the workspace, as in hf_sensor_rays_adjoint.
 * An orthographic sensor is refused with HF_EINVAL: the reference has no sample_direction for it, and a point names no
 * film position of a sensor whose pixel integral is over the origins.
 * All entries refuse with HF_EINVAL, before anything touches a device: a NULL pointer that is not optional, n >= 2^32,
 * spp == 0, a crop window that is empty or not inside the film, a non-finite field, near_clip <= 0 or far_clip <=
 * near_clip, a type that is neither; perspective: x_fov outside (0, 180) or a to_world whose linear part has scale
 * (perspective.cpp:163-164; |A^T A - I| > 1e-4); without ray_id: start + n or crop_w crop_h spp beyond 2^32.  n == 0 is
 * legal.  Callers detect the entries by their symbols (HF_VERSION is unchanged). */
#define HF_SENSOR_PERSPECTIVE 0
#define HF_SENSOR_ORTHOGRAPHIC 1
typedef struct hf_sensor {          /* HOST memory, as hf_receiver_t */
    int32_t type;                   /* HF_SENSOR_* */
    uint32_t film_w, film_h;        /* the film in pixels */
    uint32_t crop_x, crop_y, crop_w, crop_h;
    double to_world[12];            /* row-major 3x4 [A | c] */
    double x_fov;                   /* degrees, along x; perspective only */
    double near_clip, far_clip;
} hf_sensor_t;
int hf_sensor_rays(const hf_sensor_t *sensor, size_t n, uint32_t start, uint32_t spp, uint32_t seed,
                   const uint32_t *ray_id, float *const out_o[3], float *const out_d[3], float *out_maxt,
                   float *const out_pos[2], hf_stream_t stream);
int hf_sensor_rays_tangent(const hf_sensor_t *sensor, size_t n, uint32_t start, uint32_t spp, uint32_t seed,
                           const uint32_t *ray_id, const float *d_to_world, const float *d_fov, float *const out_do[3],
                           float *const out_dd[3], hf_stream_t stream);
/* the adjoint's workspace in floats (a constant: the most any launch needs) */
size_t hf_sensor_workspace_floats(void);
int hf_sensor_rays_adjoint(const hf_sensor_t *sensor, size_t n, uint32_t start, uint32_t spp, uint32_t seed,
                           const uint32_t *ray_id, const float *const grad_o[3], const float *const grad_d[3],
                           float *grad_to_world, float *grad_fov, float *workspace, hf_stream_t stream);
int hf_sensor_project(const hf_sensor_t *sensor, size_t n, const float *const p[3], const uint8_t *active,
                      float *const uv[2], uint8_t *valid, float *weight, hf_stream_t stream);
int hf_sensor_project_tangent(const hf_sensor_t *sensor, size_t n, const float *const p[3], const uint8_t *active,
                              const float *const dp[3], const float *d_to_world, const float *d_fov, float *const duv[2],
                              float *dweight, hf_stream_t stream);
int hf_sensor_project_adjoint(const hf_sensor_t *sensor, size_t n, const float *const p[3], const uint8_t *active,
                              const float *const grad_uv[2], const float *grad_weight, float *const grad_p[3],
                              float *grad_to_world, float *grad_fov, float *workspace, hf_stream_t stream);

/* ---- the thin lens: the perspective sensor with a finite aperture, depth of field, differentiable ----
 *
 * Replaces Sensor::sample_ray and sample_direction of `thinlens` (src/sensors/thinlens.cpp:216-254, 305-350).  hf_sensor_t
 * and every hf_sensor_* entry stay as they are; the lens is a struct of its own around one:
 *   lens        hf_thinlens_t, HOST memory.  base: the sensor, type HF_SENSOR_PERSPECTIVE; aperture_radius r >= 0 (0 is the
 *               pinhole: the same rays as hf_sensor_rays up to the rounding of the outputs; the reference replaces 0 by an
 *               epsilon, thinlens.cpp:158-161); focus_distance f > 0.
 *   sampling    the index, the pixel, the jitter, pos, g and w are exactly hf_sensor_rays'.  The aperture sample is a second
 *               draw in the keyed convention of the lighting rows: key = sample_tea_32(seed, HF_THINLENS_PAIR).v0,
 *               (a0, a1) = sample_tea_32(key, id), s = (a >> 9) 2^-23.  The pair lies outside 0..31, so a lighting row on
 *               the same seed shares no number with the lens.
 *   D           = (D.x, D.y, 0) = square_to_uniform_disk_concentric(s) (warp.h; thinlens.cpp:235-236), evaluated in double
 *               from the exact float s, the sine and cosine taken of an argument of at most pi / 4.
 * Rays, with tau and v = (w.x tau, w.y tau, 1) as above (near_p = near v, :231-232; focus_p = f v, :239):
 *   e = f v - r D,   d_c = e / |e| (:242),   ray.d = A d_c (:245),
 *   ray.o = c + A (r (1 - near / f) D + near v) = to_world aperture_p + ray.d near / d_c.z (:244-250),
 *   maxt = (far - near) |e| / f (:247-251).
 * Everything in double, every output rounded once; one grid-stride launch in the store variants of hf_sensor_rays (the
 * same HF_SENSOR_STORE hook, the same grids); allocates nothing, never synchronises the host, capturable.
 *
 * Differentiated with respect to to_world (12), x_fov (through tau), aperture_radius and focus_distance -- an extension:
 * the reference marks all four NonDifferentiable (:171-177).  maxt, the pixel, the jitter and the disk point are HELD.
 * With u = (w.x, w.y, 0) and o_c = r (1 - near / f) D + near v:
 *   de = f u dtau + v df - D dr,   d d_c = (de - d_c <d_c, de>) / |e|,   d ray.d = dA d_c + A d d_c,
 *   d o_c = (1 - near / f) D dr + (r near / f^2) D df + near u dtau,   d ray.o = dc + dA o_c + A d o_c.
 * hf_thinlens_rays_tangent: d_to_world (12 device floats), d_fov, d_radius, d_focus (1 device float each), each may be
 * NULL (zero).  hf_thinlens_rays_adjoint: the exact transpose; grad_to_world (12), grad_fov, grad_radius, grad_focus (1
 * each) are ACCUMULATED into, each may be NULL.  15 sums per lane in double, per block to `workspace`
 * (hf_thinlens_workspace_floats() floats, 8-byte aligned, this call's until it has completed), then one fixed-order sum
 * launch: no float atomics, bitwise repeatable, capturable -- hf_sensor_rays_adjoint's pattern with rows of 15.
 *
 * hf_thinlens_project is the way back (:305-350).  Lane i uses ITS OWN aperture draw -- that of the wavefront index
 * start + i, or ray_id[i] -- so that the projection of a point of sample i's ray is pos_i:
 *   ref       = A^-1 (p - c) (:309-310);   inside_z = active and near <= ref.z <= far (:315);
 *   q         = ref - r D (:324);   F = r D + q f / q.z (:333; its z is f);
 *   g         = ((1 - F.x / (f tau)) / 2, (1 - a F.y / (f tau)) / 2),   uv = g film_size (:340);
 *   valid     = inside_z and s_crop in [0, 1]^2 (:334; the reference also tests scr.z, which says near <= f <= far);
 *   weight    = |q| / (A' q.z^3) with hf_sensor_project's A': m_normalization inv_ct^3 / dist^2 (:335, 349).
 * What is written, and the stated deviation from the reference's early returns, are hf_sensor_project's.  Derivatives
 * with respect to p (per lane), to_world, x_fov, r and f, the masks and D HELD; the tangent and the adjoint take the same
 * start, seed and ray_id; grad_p is OVERWRITTEN, the reduced gradients are ACCUMULATED into through the workspace.
 * OUT OF SCOPE: ds.p, ds.d, ds.dist and the aperture pdf of sample_direction; the d_x / d_y of
 * sample_ray_differential; wavelengths and time.
 * All entries refuse with HF_EINVAL, before anything touches a device: everything hf_sensor_rays (hf_sensor_project)
 * refuses for a perspective sensor, base.type != HF_SENSOR_PERSPECTIVE, a non-finite or negative aperture_radius, a
 * non-finite or non-positive focus_distance.  n == 0 is legal.  Callers detect the entries by their symbols (HF_VERSION
 * is unchanged). */
typedef struct hf_thinlens {        /* HOST memory */
    hf_sensor_t base;               /* type must be HF_SENSOR_PERSPECTIVE */
    double aperture_radius;         /* >= 0, finite; 0 is the pinhole */
    double focus_distance;          /* > 0, finite */
} hf_thinlens_t;
#define HF_THINLENS_PAIR 0x4C454E53u
int hf_thinlens_rays(const hf_thinlens_t *lens, size_t n, uint32_t start, uint32_t spp, uint32_t seed,
                     const uint32_t *ray_id, float *const out_o[3], float *const out_d[3], float *out_maxt,
                     float *const out_pos[2], hf_stream_t stream);
int hf_thinlens_rays_tangent(const hf_thinlens_t *lens, size_t n, uint32_t start, uint32_t spp, uint32_t seed,
                             const uint32_t *ray_id, const float *d_to_world, const float *d_fov, const float *d_radius,
                             const float *d_focus, float *const out_do[3], float *const out_dd[3], hf_stream_t stream);
size_t hf_thinlens_workspace_floats(void);
int hf_thinlens_rays_adjoint(const hf_thinlens_t *lens, size_t n, uint32_t start, uint32_t spp, uint32_t seed,
                             const uint32_t *ray_id, const float *const grad_o[3], const float *const grad_d[3],
                             float *grad_to_world, float *grad_fov, float *grad_radius, float *grad_focus, float *workspace,
                             hf_stream_t stream);
int hf_thinlens_project(const hf_thinlens_t *lens, size_t n, uint32_t start, uint32_t seed, const uint32_t *ray_id,
                        const float *const p[3], const uint8_t *active, float *const uv[2], uint8_t *valid, float *weight,
                        hf_stream_t stream);
int hf_thinlens_project_tangent(const hf_thinlens_t *lens, size_t n, uint32_t start, uint32_t seed, const uint32_t *ray_id,
                                const float *const p[3], const uint8_t *active, const float *const dp[3],
                                const float *d_to_world, const float *d_fov, const float *d_radius, const float *d_focus,
                                float *const duv[2], float *dweight, hf_stream_t stream);
int hf_thinlens_project_adjoint(const hf_thinlens_t *lens, size_t n, uint32_t start, uint32_t seed, const uint32_t *ray_id,
                                const float *const p[3], const uint8_t *active, const float *const grad_uv[2],
                                const float *grad_weight, float *const grad_p[3], float *grad_to_world, float *grad_fov,
                                float *grad_radius, float *grad_focus, float *workspace, hf_stream_t stream);

/* ---- next row: projector lighting, a structured-light emitter whose shadow ray is traced in the kernel ----
 *
 * Replaces, for diffuse surfaces under ONE `projector` emitter (src/emitters/projector.cpp, "the reciprocal counterpart
 * of the perspective camera": a pinhole that throws a bitmap onto the scene), the emitter-sampling term of the direct
 * integrator (Emitter::sample_direction, projector.cpp:204-246; attached BSDF value, diffuse.cpp:135-140) and the shadow
 * ray it traces.  The emitter is a point, so there is one draw per sample and no sample stream.
 *   projector   hf_projector_t, HOST memory.  to_world: row-major 3x4 [A | c], scale-free (hf_sensor_t's check
 *               |A^T A - I| <= 1e-4); x_fov: degrees along x, in (0, 180); scale: the reference's `scale` (:124).
 *   texture     the irradiance tex[TH][TW] (float32, row-major, the caller's device buffer) with wrap = HF_WRAP_* (the
 *               reference's bitmap default is repeat); tex == NULL: uniform irradiance 1.  The aspect a = TW / TH
 *               (:128-129), so TW and TH are read without a texture too.
 *   mapping     ref = to_world^-1 p (:210), the affine inverse formed once on the host in double;
 *               tau = tan(x_fov pi / 360);   uv = ((1 - ref.x / (ref.z tau)) / 2, (1 - a ref.y / (ref.z tau)) / 2) (:213:
 *               hf_sensor_project's g);   lit = ref.z > 0 and uv in [0, 1]^2 (:214).  The near and far planes of
 *               :148-150 do not enter sample_direction and are no parameters.
 *   lookup      I(uv): the texel coordinate (uv.x TW, uv.y TH), rounded once to float32 (hf_sensor_project's uv for a film
 *               of TW x TH), by hf_bitmap_eval's float32 expression and rules (bitmap.cpp:497-520);
 *   eligible    sample i when t_i is finite and <sh_n_i, -d_i> > 0 (the masks of hf_direct_lighting); an eligible sample
 *               is TRACED when it is lit, <sh_n, u> > 0 with u = c - p, and |u|^2 is finite and > 0 -- the last two decided
 *               in float32 with c rounded to float32, lit in double;
 *   shadow ray  Interaction::spawn_ray_to(c), hf_rect_rays' ray: origin o = p + n s (1 + max|p_c|) RayEpsilon with n the
 *               geometric normal, s = -1 where <n, u> < 0, else 1; direction (c - o) / |c - o|; maxt = |c - o| (1 -
 *               ShadowEpsilon) (interaction.h:141-147, 161-165, math.h:18-22);
 *   visibility  vis[i], one byte: 1 iff the sample was traced and the any-hit walk found nothing before maxt;
 *   value_i     = weight_i albedo scale I(uv) G,   G = <sh_n, c - p> / ref.z^3, where vis_i = 1 and exactly 0 elsewhere:
 *               spec = pi scale I / (ref.z^2 cos) with cos = ref.z / |ref| (:231-245; |ref| = |u| for the scale-free
 *               to_world) times albedo/pi <sh_n, u> / |u| (diffuse.cpp).  No square root is taken;
 *   image[i / spp] = 1/spp * sum value_i: the box film of hf_direct_lighting, overwritten; n a multiple of spp;
 *   uv          2 rows of n floats: uv of every sample with ref.z > 0, zeros elsewhere (eligible or not).
 * G, uv and every derivative sum are formed in double from the float32 inputs and rounded once (DESIGN 4.22's reasons:
 * u is a difference, ref.z^3 amplifies); the lookup is float32; the shadow ray takes float32 quantities (what
 * hf_projector_rays writes).
 * Differentiated with respect to sh_n, p, weight, tex, to_world (all 12 entries, unconstrained, hf_sensor_project's
 * convention), x_fov and scale.  HELD: the visibility, every mask, the cell of the lookup.  With z = ref.z, (Lx, Ly) the
 * lookup's slopes and b_j its four weights:
 *   d ref = A^-1 (dp - dA ref - dc),   d tau = (pi / 360) (1 + tau^2) d fov,
 *   dG = <d sh_n, u> / z^3 + <sh_n, dc - dp> / z^3 - 3 <sh_n, u> d ref.z / z^4,
 *   dI = Lx TW d uv.x + Ly TH d uv.y + sum_j b_j d tex_j,   d uv from the mapping above.
 * OUT OF SCOPE: the silhouette part of a moving shadow (hf_reparam_*'s, as in the rows above), sample_ray (light tracing
 * from the projector with importance-sampled pixels), RGB, the other fov_axis values, several projectors per call (call
 * once each and add the images).  spot.cpp is the next row's (hf_spot_lighting).
 * All entries refuse with HF_EINVAL, before anything touches a device: a NULL pointer that is not optional, n >= 2^32,
 * spp == 0 or n % spp != 0, TW == 0, TH == 0 or TW TH >= 2^31, a wrap that is neither, a non-finite field of the
 * projector, x_fov outside (0, 180), a to_world with scale, a non-finite albedo.  p, nrm, sh_n, d: 3 device rows of n
 * floats; t: n.  Callers detect the entries by their symbols (HF_VERSION is unchanged). */
typedef struct hf_projector {       /* HOST memory, as hf_sensor_t */
    double to_world[12];            /* row-major 3x4 [A | c], scale-free */
    double x_fov;                   /* degrees, along x, in (0, 180) */
    float scale;                    /* multiplies the irradiance */
} hf_projector_t;
/* hf_projector_rays materialises the shadow ray of every sample (out_o, out_d: 3 rows of n floats; out_maxt: n floats, the
 * finite maxt above for a traced lane; a lane that is not traced gets a zero origin and direction and maxt = -1, a miss):
 * the two-call sequence hf_projector_rays + hf_ray_test that hf_projector_lighting equals bit for bit.  TW, TH: for the
 * aspect.  Takes no field handle. */
int hf_projector_rays(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                      const float *const d[3], const float *t, const hf_projector_t *projector, uint32_t TW, uint32_t TH,
                      float *const out_o[3], float *const out_d[3], float *out_maxt, hf_stream_t stream);
/* The fused launch (hf_refract_lighting's shape): reads a sample's record once, maps it, looks the texture up, runs the
 * per-lane any-hit walk up to maxt where the sample is traced, and writes image (n / spp), value (n), vis (n bytes) and
 * uv (2 rows) -- each may be NULL (not wanted), not all of them; no ray and no hit byte goes to memory.  A batch of 64
 * samples without a traced one skips the walk.  hf_set_ray_coherence is neither read nor changed.  weight: n floats or
 * NULL (1).  Allocates nothing, never synchronises the host, capturable. */
int hf_projector_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3], const float *const nrm[3],
                          const float *const sh_n[3], const float *const d[3], const float *t, const float *weight,
                          const hf_projector_t *projector, uint32_t TW, uint32_t TH, const float *tex, int wrap,
                          float albedo, float *image, float *value, uint8_t *vis, float *const uv[2], hf_stream_t stream);
/* the adjoint's workspace in floats (a constant: the most any launch needs) */
size_t hf_projector_workspace_floats(void);
/* Reverse mode.  Traces nothing: vis (as hf_projector_lighting wrote it) is read.  With the upstream
 * g = grad_image[i / spp] / spp + grad_value[i] (either may be NULL = zero): grad_sh_n, grad_p (3 rows each) and
 * grad_weight are OVERWRITTEN, one lane per sample, exact zeros where vis = 0, no atomics; grad_tex[TH][TW] is ACCUMULATED
 * into on the four texels of every visible sample (float atomics; ignored without a texture); grad_to_world (12 device
 * floats), grad_fov and grad_scale (1 device float each) are ACCUMULATED into without atomics: every block stores its 14
 * partial sums in double to `workspace` -- hf_projector_workspace_floats() floats of device memory, 8-byte aligned, the
 * caller's, this call's until it has completed; needed only when one of the three is wanted -- and one more launch adds
 * them in a fixed order (hf_sensor_rays_adjoint's pattern with rows of 14; family 2 of hf_grid_blocks): bitwise the same
 * from launch to launch.  Every output may be NULL (not wanted).  Takes no field handle. */
int hf_projector_lighting_adjoint(size_t n, uint32_t spp, const float *const p[3], const float *const sh_n[3],
                                  const float *const d[3], const float *t, const float *weight,
                                  const hf_projector_t *projector, uint32_t TW, uint32_t TH, const float *tex, int wrap,
                                  float albedo, const uint8_t *vis, const float *grad_image, const float *grad_value,
                                  float *const grad_sh_n[3], float *const grad_p[3], float *grad_weight, float *grad_tex,
                                  float *grad_to_world, float *grad_fov, float *grad_scale, float *workspace,
                                  hf_stream_t stream);
/* Forward mode, the exact transpose of the adjoint, for tangents dsh_n, dp (3 rows of n floats each), dweight (n), dtex
 * ([TH][TW]; ignored without a texture), d_to_world (12 device floats), d_fov and d_scale (1 device float each), each may
 * be NULL (zero); dimage (n / spp) and / or dvalue (n) are overwritten (at least one).  No atomics for any spp (a power of
 * two <= 64: the film's shuffle tree; otherwise one lane adds the samples of a pixel in order): bitwise the same from
 * launch to launch.  Takes no field handle. */
int hf_projector_lighting_tangent(size_t n, uint32_t spp, const float *const p[3], const float *const sh_n[3],
                                  const float *const d[3], const float *t, const float *weight,
                                  const hf_projector_t *projector, uint32_t TW, uint32_t TH, const float *tex, int wrap,
                                  float albedo, const uint8_t *vis, const float *const dsh_n[3], const float *const dp[3],
                                  const float *dweight, const float *dtex, const float *d_to_world, const float *d_fov,
                                  const float *d_scale, float *dimage, float *dvalue, hf_stream_t stream);

/* ---- next row: spot lighting, a rig of up to HF_MAX_LIGHTS cone emitters whose shadow rays are traced in
 * the kernel ----
 *
 * Replaces, for diffuse surfaces under 1 <= K <= HF_MAX_LIGHTS `spot` emitters (src/emitters/spot.cpp), the
 * emitter-sampling term of the direct integrator (SpotLight::sample_direction, spot.cpp:177-212; falloff_curve,
 * :143-151; attached BSDF value, diffuse.cpp:135-140) and the K shadow rays it traces, in ONE launch with one image per
 * light: near-light photometric stereo.  A light with cutoff_angle = beam_width = 180 is the reference's point light.
 *   lights      n_lights hf_spot_light_t, HOST memory.  to_world: row-major 3x4 [A | c], scale-free (hf_sensor_t's check);
 *               intensity: W/sr on the axis; cutoff_angle, beam_width: degrees, 0 < beam_width <= cutoff_angle <= 180.
 *               The host forms A^-1, the angles in radians and their cosines once, in double.
 *   mapping     ref = A^-1 (p - c) in double from the float32 point; cos(theta) = ref.z / |ref|; the sample is in the
 *               cone when cos(theta) > cos(cutoff), in the full beam when cos(theta) >= cos(beam), in the transition zone
 *               when it is in the cone but not in the full beam;
 *   falloff     f = 1 in the full beam, (cutoff - theta) / (cutoff - beam) in the zone with theta = atan2(hypot(ref.x,
 *               ref.y), ref.z) (the acos of the cosine, better conditioned), 0 elsewhere.  cutoff == beam is a hard edge
 *               without a zone; nothing divides by the zero width;
 *   eligible    sample i when t_i is finite and <sh_n_i, -d_i> > 0 (the masks of every row); an eligible sample is TRACED
 *               towards light k when f > 0 (spot.cpp:198), <sh_n, u> > 0 with u = c - p, and |u|^2 is finite and > 0 -- the
 *               last two decided in float32 with c rounded to float32 (hf_projector_lighting's), f in double;
 *   shadow ray  Interaction::spawn_ray_to(c), hf_projector_rays' ray unchanged;
 *   vis[i]      one byte: bit k is set iff sample i was traced towards light k and the any-hit walk found nothing before
 *               maxt (HF_MAX_LIGHTS = 8 fills the byte);
 *   value[k][i] = weight_i albedo/pi intensity_k f <sh_n, u> / |u|^3 where bit k is set and exactly 0 elsewhere, formed in
 *               double and rounded once;
 *   image[k][i / spp] = 1/spp * sum value[k][i]: hf_point_lighting's layout, K images of n / spp, overwritten; n a
 *               multiple of spp.
 * Differentiated with respect to sh_n, p, weight and, per light, to_world (all 12 entries, unconstrained,
 * hf_projector_lighting's convention), intensity, cutoff_angle and beam_width (per degree): HF_SPOT_PARAMS numbers per
 * light in this order.  HELD: the visibility bits, every mask and the branch of the falloff.  With rho = hypot(ref.x,
 * ref.y) (> 0 in the zone), S = <sh_n, u>, r = |u| and du = dc - dp:
 *   d ref = A^-1 (dp - dA ref - dc),
 *   in the zone: d theta = (ref.z d rho - rho d ref.z) / |ref|^2,  d rho = (ref.x d ref.x + ref.y d ref.y) / rho,
 *                df = ((dcut - d theta) - f (dcut - dbeam)) / (cutoff - beam);   outside it df = 0, so a light with
 *                cutoff == beam has exact zeros for both angle gradients,
 *   d(S / r^3) = <d sh_n, u> / r^3 + <sh_n, du> / r^3 - 3 S <u, du> / r^5   (for dc = 0: hf_point_lighting's).
 * OUT OF SCOPE: the `texture` parameter of spot.cpp (a textured cone is hf_projector_lighting's business), sample_ray,
 * RGB, and the silhouette part of a moving shadow (hf_reparam_*'s, as in every row).
 * All entries refuse with HF_EINVAL, before anything touches a device: a NULL pointer that is not optional, n >= 2^32,
 * spp == 0 or n % spp != 0, n_lights outside 1..HF_MAX_LIGHTS, a non-finite field of a light, angles outside
 * 0 < beam_width <= cutoff_angle <= 180, a to_world with scale, a non-finite albedo.  p, nrm, sh_n, d: 3 device rows of n
 * floats; t: n.  Callers detect the entries by their symbols (HF_VERSION is unchanged). */
#define HF_SPOT_PARAMS 15           /* to_world[12], intensity, cutoff_angle, beam_width: the order of every parameter row */
typedef struct hf_spot_light {      /* HOST memory, as hf_projector_t */
    double to_world[12];            /* row-major 3x4 [A | c], scale-free */
    float intensity;                /* W/sr on the axis */
    float cutoff_angle, beam_width; /* degrees, 0 < beam_width <= cutoff_angle <= 180 */
} hf_spot_light_t;
/* hf_spot_rays materialises the shadow ray of every sample towards ONE light (out_o, out_d: 3 rows of n floats; out_maxt: n
 * floats, the finite maxt for a traced lane; a lane that is not traced gets a zero origin and direction and maxt = -1, a
 * miss): bit k of hf_spot_lighting's vis equals hf_spot_rays(light k) + hf_ray_test bit for bit.  Takes no field handle. */
int hf_spot_rays(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                 const float *const d[3], const float *t, const hf_spot_light_t *light, float *const out_o[3],
                 float *const out_d[3], float *out_maxt, hf_stream_t stream);
/* The fused launch: reads a sample's record once and holds it across a wave-uniform loop over the lights; for each light
 * it maps the point, finishes the value, runs the per-lane any-hit walk up to maxt where the sample is traced and reduces
 * the film; image (K rows of n / spp), value (K rows of n) and vis (n bytes) may each be NULL (not wanted), not all of
 * them; no ray and no hit byte goes to memory.  A batch of 64 samples with no lane traced towards light k skips that walk.
 * hf_set_ray_coherence is neither read nor changed.  weight: n floats or NULL (1).  Allocates nothing, never synchronises
 * the host, capturable. */
int hf_spot_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3], const float *const nrm[3],
                     const float *const sh_n[3], const float *const d[3], const float *t, const float *weight,
                     uint32_t n_lights, const hf_spot_light_t *lights, float albedo, float *image, float *value,
                     uint8_t *vis, hf_stream_t stream);
/* the adjoint's workspace in floats for a rig of n_lights (0 for a count outside 1..HF_MAX_LIGHTS) */
size_t hf_spot_workspace_floats(uint32_t n_lights);
/* Reverse mode.  Traces nothing: vis (as hf_spot_lighting wrote it) is read.  With the upstream of light k
 * g_k = grad_image[k][i / spp] / spp + grad_value[k][i] (either may be NULL = zero): grad_sh_n, grad_p (3 rows each) and
 * grad_weight are OVERWRITTEN, one lane per sample, the K lights summed in light order in double and rounded once, exact
 * zeros where vis = 0, no atomics; grad_lights[K][HF_SPOT_PARAMS] (device floats) is ACCUMULATED into without atomics:
 * every block stores the 15 partial sums of every light in double to `workspace` -- hf_spot_workspace_floats(n_lights)
 * floats of device memory, 8-byte aligned, the caller's, this call's until it has completed; needed only when grad_lights
 * is wanted -- and one more launch adds them in a fixed order (hf_sensor_rays_adjoint's pattern with rows of 15; family 2
 * of hf_grid_blocks): bitwise the same from launch to launch.  Every output may be NULL (not wanted).  Takes no field
 * handle. */
int hf_spot_lighting_adjoint(size_t n, uint32_t spp, const float *const p[3], const float *const sh_n[3],
                             const float *const d[3], const float *t, const float *weight, uint32_t n_lights,
                             const hf_spot_light_t *lights, float albedo, const uint8_t *vis, const float *grad_image,
                             const float *grad_value, float *const grad_sh_n[3], float *const grad_p[3], float *grad_weight,
                             float *grad_lights, float *workspace, hf_stream_t stream);
/* Forward mode, the exact transpose of the adjoint, for tangents dsh_n, dp (3 rows of n floats each), dweight (n) and
 * d_lights ([K][HF_SPOT_PARAMS] device floats), each may be NULL (zero); dimage (K rows of n / spp) and / or dvalue (K rows
 * of n) are overwritten (at least one).  No atomics for any spp (a power of two <= 64: the film's shuffle tree; otherwise
 * one lane adds the samples of a pixel in order): bitwise the same from launch to launch.  Takes no field handle. */
int hf_spot_lighting_tangent(size_t n, uint32_t spp, const float *const p[3], const float *const sh_n[3],
                             const float *const d[3], const float *t, const float *weight, uint32_t n_lights,
                             const hf_spot_light_t *lights, float albedo, const uint8_t *vis, const float *const dsh_n[3],
                             const float *const dp[3], const float *dweight, const float *d_lights, float *dimage,
                             float *dvalue, hf_stream_t stream);

/* ---- next row: directional lighting, a rig of up to HF_MAX_LIGHTS distant emitters whose shadow rays are
 * traced in the kernel ----
 *
 * Replaces, for diffuse surfaces under 1 <= K <= HF_MAX_LIGHTS `directional` emitters (src/emitters/directional.cpp), the
 * emitter-sampling term of the direct integrator (DirectionalEmitter::sample_direction, directional.cpp:150-177;
 * attached BSDF value, diffuse.cpp:135-140) and the K shadow rays it traces, in ONE launch with one image per light:
 * photometric stereo with cast shadows.  hf_direct_lighting* takes the visibility from the caller and holds the lights
 * constant; this row traces it and differentiates them.  hf_direct_lighting* itself is unchanged.
 *   lights      n_lights hf_directional_light_t, HOST memory.  to_light: towards the light (the reference's `direction`
 *               is -to_light), any finite length > 0; the host forms l = to_light / |to_light| once, in double.
 *               irradiance: W/m^2 on a surface facing the light (directional.cpp:82, 174).
 *   eligible    sample i when t_i is finite and <sh_n_i, -d_i> > 0 (the masks of every row); an eligible sample is TRACED
 *               towards light k when <sh_n, l_k> > 0, decided in float32 with l rounded to float32 -- that rounded vector
 *               is the ray's own direction (hf_spot_lighting's convention for its `front` test);
 *   shadow ray  si.spawn_ray(l_k), hf_sky_rays' ray for the direction l_k: o = p + n s (1 + max|p_c|) 1500 2^-24 with
 *               s = sign <n, l>, d = float32(l), maxt = inf;
 *   vis[i]      one byte: bit k is set iff sample i was traced towards light k and the any-hit walk found nothing
 *               (HF_MAX_LIGHTS = 8 fills the byte);
 *   value[k][i] = weight_i albedo/pi irradiance_k <sh_n_i, l_k> where bit k is set and exactly 0 elsewhere, formed in
 *               double and rounded once;
 *   image[k][i / spp] = 1/spp * sum value[k][i]: hf_point_lighting's layout, K images of n / spp, overwritten; n a
 *               multiple of spp.
 * Differentiated with respect to sh_n, weight and, per light, to_light and irradiance: HF_DIRECTIONAL_PARAMS numbers per
 * light in this order.  (directional.cpp:96 keeps the emitter's to_world non-differentiable; the direction's derivative
 * goes beyond the reference.)  HELD: the visibility bits and every mask.  The value does not depend on p: p and nrm enter
 * only the held shadow ray, so there is no grad_p and the derivative entries do not take them.  With L = |to_light|,
 * S = <sh_n, l>, c = albedo / pi:
 *   dl = (dv - l <l, dv>) / L,
 *   d value = c [ dw E S + w dE S + w E (<d sh_n, l> + <sh_n, dl>) ].
 * The gradient of to_light is orthogonal to l: scaling to_light by s leaves every output unchanged and divides that
 * gradient by s.
 * OUT OF SCOPE: sample_ray, RGB, and the silhouette part of a moving shadow (hf_reparam_*'s, as in every row).
 * All entries refuse with HF_EINVAL, before anything touches a device: a NULL pointer that is not optional, n >= 2^32,
 * spp == 0 or n % spp != 0, n_lights outside 1..HF_MAX_LIGHTS, a non-finite field of a light, |to_light| zero or
 * non-finite, a non-finite albedo.  p, nrm, sh_n, d: 3 device rows of n floats; t: n.  Callers detect the entries by
 * their symbols (HF_VERSION is unchanged). */
#define HF_DIRECTIONAL_PARAMS 4          /* to_light[3], irradiance: the order of every parameter row */
typedef struct hf_directional_light {    /* HOST memory, as hf_spot_light_t */
    double to_light[3];                  /* towards the light; any finite length > 0; the host normalises it once, in double */
    float irradiance;                    /* directional.cpp:82, 174 */
} hf_directional_light_t;
/* hf_directional_rays materialises the shadow ray of every sample towards ONE light (out_o, out_d: 3 rows of n floats;
 * out_maxt: n floats, inf for a traced lane; a lane that is not traced gets a zero origin and direction and maxt = -1, a
 * miss): bit k of hf_directional_lighting's vis equals hf_directional_rays(light k) + hf_ray_test bit for bit.  Takes no
 * field handle. */
int hf_directional_rays(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                        const float *const d[3], const float *t, const hf_directional_light_t *light,
                        float *const out_o[3], float *const out_d[3], float *out_maxt, hf_stream_t stream);
/* The fused launch: reads a sample's record once and holds it across a wave-uniform loop over the lights; for each light
 * it finishes the value, runs the per-lane any-hit walk where the sample is traced and reduces the film; image (K rows of
 * n / spp), value (K rows of n) and vis (n bytes) may each be NULL (not wanted), not all of them; no ray and no hit byte
 * goes to memory.  A batch of 64 samples with no lane traced towards light k skips that walk.  hf_set_ray_coherence is
 * neither read nor changed.  weight: n floats or NULL (1).  Allocates nothing, never synchronises the host, capturable. */
int hf_directional_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3],
                            const float *const nrm[3], const float *const sh_n[3], const float *const d[3],
                            const float *t, const float *weight, uint32_t n_lights, const hf_directional_light_t *lights,
                            float albedo, float *image, float *value, uint8_t *vis, hf_stream_t stream);
/* the adjoint's workspace in floats for a rig of n_lights (0 for a count outside 1..HF_MAX_LIGHTS) */
size_t hf_directional_workspace_floats(uint32_t n_lights);
/* Reverse mode.  Traces nothing: vis (as hf_directional_lighting wrote it) is read.  With the upstream of light k
 * g_k = grad_image[k][i / spp] / spp + grad_value[k][i] (either may be NULL = zero):
 *   grad_sh_n = sum_k g_k w c E_k l_k,   grad_weight = sum_k g_k c E_k S_k
 * (3 rows and 1 row) are OVERWRITTEN, one lane per sample, the K lights summed in light order in double and rounded once,
 * exact zeros where vis = 0, no atomics;
 *   grad_lights[k] = ( sum_i g w c E (sh_n - l S) / L ,  sum_i g w c S )
 * ([K][HF_DIRECTIONAL_PARAMS] device floats) is ACCUMULATED into without atomics: every block stores the 4 partial sums of
 * every light in double to `workspace` -- hf_directional_workspace_floats(n_lights) floats of device memory, 8-byte
 * aligned, the caller's, this call's until it has completed; needed only when grad_lights is wanted -- and one more
 * launch adds them in a fixed order (hf_spot_lighting_adjoint's pattern with rows of 4; family 2 of hf_grid_blocks):
 * bitwise the same from launch to launch.  Every output may be NULL (not wanted).  Takes no field handle. */
int hf_directional_lighting_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                    const float *t, const float *weight, uint32_t n_lights,
                                    const hf_directional_light_t *lights, float albedo, const uint8_t *vis,
                                    const float *grad_image, const float *grad_value, float *const grad_sh_n[3],
                                    float *grad_weight, float *grad_lights, float *workspace, hf_stream_t stream);
/* Forward mode, the exact transpose of the adjoint, for tangents dsh_n (3 rows of n floats), dweight (n) and d_lights
 * ([K][HF_DIRECTIONAL_PARAMS] device floats), each may be NULL (zero); dimage (K rows of n / spp) and / or dvalue (K rows
 * of n) are overwritten (at least one).  No atomics for any spp (a power of two <= 64: the film's shuffle tree; otherwise
 * one lane adds the samples of a pixel in order): bitwise the same from launch to launch.  Takes no field handle. */
int hf_directional_lighting_tangent(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                    const float *t, const float *weight, uint32_t n_lights,
                                    const hf_directional_light_t *lights, float albedo, const uint8_t *vis,
                                    const float *const dsh_n[3], const float *dweight, const float *d_lights,
                                    float *dimage, float *dvalue, hf_stream_t stream);

/* ---- the normal map: the shading normal perturbed by an RGB texture, fused and differentiable ----
 *
 * The reference's `normalmap` (src/bsdfs/normalmap.cpp:188-196) as a map of the ONE thing every lighting row consumes
 * of the surface, the shading normal: a per-texel normal field, finer than the height grid and independent of it -- the
 * unknown of photometric stereo.  The result is a new sh_n; every lighting row takes it as it takes any other.
 * Per sample i:
 *   inputs      uv (2 rows), b = sh_n (3 rows), dp_du (3 rows) of n floats, active (n bytes; NULL: every lane);
 *   texture     tex[3][TH][TW], float32, PLANAR, the caller's device buffer: plane k is exactly a hf_bitmap_eval texture;
 *               wrap = HF_WRAP_CLAMP or HF_WRAP_REPEAT;
 *   lookup      pos = (float32(u TW), float32(v TH)), each product rounded once; c_k = hf_bitmap_eval of plane k at pos,
 *               bit for bit (bitmap.cpp:497-520), k = 0, 1, 2;
 *   normal      mt = 2 c - 1, m = mt / |mt| (normalmap.cpp:189-192), in double from the three float32 lookups;
 *   base frame  a = dp_du - b <b, dp_du>, s0 = a / |a|, t0 = b x s0 (interaction.h:257-267), in double;
 *   result      N = s0 m_x + t0 m_y + b m_z, formed in double and rounded once per component; NOT renormalised: unit to
 *               rounding when b is.
 * A lane is PERTURBED when it is active, uv, b and dp_du are finite, the lookup reads something (under HF_WRAP_REPEAT a
 * coordinate beyond 2^23 texels reads nothing), |mt|^2 >= 1e-12, |dp_du|^2 > 0 and |a|^2 >= 1e-12 |dp_du|^2.  Every other
 * lane PASSES THROUGH: N = b bit for bit, its derivative is the identity on sh_n and zero for everything else.  The
 * reference's fall-back to coordinate_system(n) at dp_du = 0 is deliberately not taken: a lane without a
 * parameterisation has no tangent space to perturb in.  mask (n bytes, optional): 1 where perturbed, 0 elsewhere.
 * DEVIATION: the reference rebuilds frame.s from the world-space dp_du and the LOCAL perturbed normal, mixing spaces;
 * here everything is in world space and only N is returned, the one member of the frame a row reads.  s and t are the
 * host's business (NormalMap.perturb rebuilds them from dp_du and N) and carry no gradient, as hf_si_grad_t has none
 * for them.
 * Differentiated with respect to tex, uv (through the slopes Lx, Ly of each plane), sh_n and dp_du.  HELD: the cell, the
 * perturbed / pass-through decision, the masks.  With A = |a|, M = |mt|, dpos = (TW du, TH dv) and b_j the four bilinear
 * weights of the cell:
 *   dc_k = sum_j b_j dtex_k,j + Lx_k dpos_x + Ly_k dpos_y,
 *   dmt  = 2 dc,   dm = (dmt - m <m, dmt>) / M,
 *   da   = ddp_du - db <b, dp_du> - b (<db, dp_du> + <b, ddp_du>),
 *   ds0  = (da - s0 <s0, da>) / A,   dt0 = db x s0 + b x ds0,
 *   dN   = ds0 m_x + dt0 m_y + db m_z + s0 dm_x + t0 dm_y + b dm_z.
 * The adjoint is the exact transpose.
 * The reference's `bumpmap` is hf_bumpmap_eval (below the medium).
 * OUT OF SCOPE: the BSDF-side test cos_theta(wo) cos_theta(perturbed_wo) > 0 (normalmap.cpp:148: the rows
 * decide on <sh_n, l> as before); nearest filtering; a gradient for s or t; the mirror wrap.
 * All three entries refuse with HF_EINVAL, before anything touches a device: a NULL pointer that is not optional,
 * n >= 2^32, TW == 0 or TH == 0, TW TH >= 2^31, a wrap that is neither constant.  n == 0 is legal and launches nothing.
 * They take no field handle, allocate nothing, never synchronise the host and are capturable; one launch each, one lane
 * per sample.  Callers detect the entries by their symbols (HF_VERSION is unchanged). */
int hf_normalmap_eval(size_t n, const float *const uv[2], const float *const sh_n[3], const float *const dp_du[3],
                      const uint8_t *active, uint32_t TW, uint32_t TH, const float *tex, int wrap, float *const out_n[3],
                      uint8_t *mask, hf_stream_t stream);
/* Forward mode: dtex ([3][TH][TW], planar), duv (2 rows), dsh_n, ddp_du (3 rows each) may each be NULL (zero); dout_n
 * (3 rows) is overwritten.  Bitwise the same from launch to launch. */
int hf_normalmap_eval_tangent(size_t n, const float *const uv[2], const float *const sh_n[3], const float *const dp_du[3],
                              const uint8_t *active, uint32_t TW, uint32_t TH, const float *tex, int wrap,
                              const float *dtex, const float *const duv[2], const float *const dsh_n[3],
                              const float *const ddp_du[3], float *const dout_n[3], hf_stream_t stream);
/* Reverse mode: grad_out (3 rows) is dL/dN.  grad_tex ([3][TH][TW]) is ACCUMULATED into with float atomics, the four
 * products of hf_bitmap_eval_adjoint per plane -- at most twelve per perturbed sample: consecutive lanes of a wave that
 * share a cell add theirs up first -- in a free order: repeatable to rounding; grad_uv (2 rows), grad_sh_n and
 * grad_dp_du (3 rows each) are OVERWRITTEN, with exact zeros where nothing flows.  Each output may be NULL (not wanted),
 * not all of them. */
int hf_normalmap_eval_adjoint(size_t n, const float *const uv[2], const float *const sh_n[3], const float *const dp_du[3],
                              const uint8_t *active, uint32_t TW, uint32_t TH, const float *tex, int wrap,
                              const float *const grad_out[3], float *grad_tex, float *const grad_uv[2],
                              float *const grad_sh_n[3], float *const grad_dp_du[3], hf_stream_t stream);

/* ---- next row: specular highlights, a GGX lobe under the directional rig, nothing traced ----
 *
 * The reflection lobe of a rough dielectric or conductor surface (roughplastic.cpp:315-350, roughconductor.cpp's eval:
 * F D G / (4 cos theta_i), MicrofacetDistribution::eval and smith_g1 of microfacet.h:185-207, 341-365) under the rig of
 * hf_directional_lighting, for ALL K lights in ONE launch that reads a sample's record once.  The row traces nothing:
 * bit k of hf_directional_lighting's vis ("eligible, <sh_n, l_k> > 0, traced, unoccluded") is the mask of light k, read
 * as the directional adjoint and tangent read it.  A diffuse + specular image is hf_directional_lighting and this row:
 * one shadow walk per light, not two.  No other entry changes.
 *   lights      n_lights hf_directional_light_t, HOST memory, exactly as hf_directional_lighting takes them; the host
 *               forms l_k = to_light / |to_light| once, in double;
 *   alpha       n floats, the GGX roughness of every sample, as hf_glossy_lighting's; a = max(alpha, 1e-4);
 *   eta         the relative index of the interface (HOST float); 0 is the ideal mirror F = 1, as in the reflect and the
 *               glossy row;
 *   vis         n bytes as hf_directional_lighting wrote them (a foreign byte is legal: see below);
 *   wi = -d,  h = (wi + l) / |wi + l|,  c_i = <sh_n, wi>,  c_o = <sh_n, l>,  c_h = <sh_n, h>   (all in double from the
 *               float32 rows and the double l);
 *   value[k][i] = weight E_k F(<wi, h>, eta) D(c_h, a) G1(c_i, a) G1(c_o, a) / (4 c_i)
 *               where bit k of vis[i] is set, c_i > 0, c_o > 0 and alpha is finite, and exactly 0 everywhere else -- a
 *               lane whose bit was set by a foreign byte but whose cosines are not positive included;
 *               D = 1 / (pi a^2 (s^2 / a^2 + c_h^2)^2),  s^2 = max(1 - c_h^2, 0)   (microfacet.h:185-207, isotropic GGX);
 *   arithmetic  D and the product are formed in double and rounded once (D cancels at small a near c_h = 1).  F is the
 *               float32 Fresnel term of the reflect and glossy rows at the float32 cosine <wi, float32(h)>, G1 the
 *               float32 smith_g1 of the glossy row at float32(c_i) and float32(c_o): the same device functions;
 *   no further masks: on every lane that passes, c_h = (c_i + c_o) / |wi + l| > 0 and <wi, h> = |wi + l| / 2 > 0, so
 *               the conditions of microfacet.h:206 (D only where <n, h> > 0) and :362 (G1 only where <v, h> <v, n> > 0)
 *               hold identically; they are NOT tested, so that no rounding decides a mask;
 *   image[k][i / spp] = 1/spp * sum value[k][i]: hf_point_lighting's layout, K images of n / spp, overwritten.
 * image (K rows of n / spp) and value (K rows of n) may each be NULL (not wanted), not both.  There is no field handle,
 * no p, no nrm, no t and no visibility output.
 * Differentiated with respect to sh_n, weight, alpha (per sample; zero where the clamp a = 1e-4 is active) and, per
 * light, to_light and irradiance: HF_DIRECTIONAL_PARAMS numbers per light in that order.  HELD: vis and every mask.
 * With v = F R, R = D G1(c_i) G1(c_o) / (4 c_i), u = <wi, h>, M = |wi + l|, L = |to_light|:
 *   dv/dsh_n = v [ (dlnD/dc_h) h + (dlnG1(c_i)/dc - 1/c_i) wi + (dlnG1(c_o)/dc) l ],
 *   dv/da    = v [ dlnD/da + dlnG1(c_i)/da + dlnG1(c_o)/da ],
 *   dv/dl    = v (dlnG1(c_o)/dc) sh_n + [ v (dlnD/dc_h) (sh_n - h c_h) + R (dF/du) (wi - h u) ] / M   (dh/dl included),
 *   dl       = (dv - l <l, dv>) / L,
 *   d value  = dw E v + w dE v + w E ( <dv/dsh_n, dsh_n> + dv/da da + <dv/dl, dl> ).
 * The gradient of to_light is orthogonal to l: scaling to_light by s leaves every output unchanged and divides that
 * gradient by s.  G1 and its derivatives are float32: for a positive cosine so small (below about 1e-13) that G1 or one of
 * its derivatives leaves float32's range, that lane's dlnG1 terms count as 0 -- every derivative stays finite (the value
 * itself is finite and tends to 0 there).
 * OUT OF SCOPE: a gradient for d or eta, anisotropy, the Beckmann distribution, a complex index of refraction,
 * roughplastic's coupled diffuse term (its t_i t_o transmittance tables), RGB, a spot or projector rig.
 * All entries refuse with HF_EINVAL, before anything touches a device: a NULL pointer that is not optional (vis among
 * them), n >= 2^32, spp == 0 or n % spp != 0, n_lights outside 1..HF_MAX_LIGHTS, a non-finite field of a light,
 * |to_light| zero or non-finite, a negative or non-finite eta.  n == 0 is legal and launches nothing.  The entries
 * allocate nothing, never synchronise the host and are capturable.  Callers detect them by their symbols (HF_VERSION is
 * unchanged). */
int hf_specular_lighting(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3], const float *weight,
                         const float *alpha, float eta, uint32_t n_lights, const hf_directional_light_t *lights,
                         const uint8_t *vis, float *image, float *value, hf_stream_t stream);
/* the adjoint's workspace in floats for a rig of n_lights (0 for a count outside 1..HF_MAX_LIGHTS) */
size_t hf_specular_workspace_floats(uint32_t n_lights);
/* Reverse mode.  With the upstream of light k g_k = grad_image[k][i / spp] / spp + grad_value[k][i] (either may be NULL
 * = zero): grad_sh_n (3 rows), grad_weight and grad_alpha (1 row each) are OVERWRITTEN, one lane per sample, the K lights
 * summed in light order in double and rounded once, exact zeros where vis = 0, no atomics; grad_lights
 * ([K][HF_DIRECTIONAL_PARAMS] device floats) is ACCUMULATED into without atomics through `workspace` --
 * hf_specular_workspace_floats(n_lights) floats of device memory, 8-byte aligned, the caller's, this call's until it has
 * completed; needed only when grad_lights is wanted -- and one more launch that adds the blocks' rows in a fixed order
 * (hf_directional_lighting_adjoint's pattern; family 2 of hf_grid_blocks): bitwise the same from launch to launch.  Every
 * output may be NULL (not wanted). */
int hf_specular_lighting_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                 const float *weight, const float *alpha, float eta, uint32_t n_lights,
                                 const hf_directional_light_t *lights, const uint8_t *vis, const float *grad_image,
                                 const float *grad_value, float *const grad_sh_n[3], float *grad_weight, float *grad_alpha,
                                 float *grad_lights, float *workspace, hf_stream_t stream);
/* Forward mode, the exact transpose of the adjoint, for tangents dsh_n (3 rows of n floats), dweight (n), dalpha (n) and
 * d_lights ([K][HF_DIRECTIONAL_PARAMS] device floats), each may be NULL (zero); dimage (K rows of n / spp) and / or
 * dvalue (K rows of n) are overwritten (at least one).  No atomics for any spp: bitwise the same from launch to launch. */
int hf_specular_lighting_tangent(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                 const float *weight, const float *alpha, float eta, uint32_t n_lights,
                                 const hf_directional_light_t *lights, const uint8_t *vis, const float *const dsh_n[3],
                                 const float *dweight, const float *dalpha, const float *d_lights, float *dimage,
                                 float *dvalue, hf_stream_t stream);

/* ---- next row: a homogeneous medium, single scattering under the directional rig, the shadow rays of
 * 1..32 points of every primary ray traced in the kernel ----
 *
 * The single-scattering emitter-sampling step of prbvolpath (src/python/python/ad/integrators/prbvolpath.py) for a
 * `homogeneous` medium (src/media/homogeneous.cpp:139-175: sigma_s = albedo sigma_t) with the `hg` phase function
 * (src/phase/hg.cpp:66-69) under 1 <= J <= HF_MAX_LIGHTS `directional` emitters, for a scene whose only occluder is this
 * shape.  World space.  The medium fills the half space below a top plane; the rig of hf_directional_light_t lies
 * outside it.  Every lighting row so far ends at the surface; this one lights the space between camera, terrain and
 * light: its shadow rays start IN FREE SPACE (no spawn offset, no normal), and a sample that missed the terrain
 * (t = inf) still contributes.
 *   medium      hf_medium_t, HOST memory.  top_normal points out of the medium, any finite length > 0; the host forms
 *               N = top_normal / |top_normal| once, in double.
 *   segment     inputs o, d (3 device rows of n floats, the primary ray) and t (n floats, inf = a miss); geometry in
 *               double from the float32 rows.  h = <o - top_origin, N>, c = <d, N>.
 *                 c < 0:            u_in = max(0, h / -c), u_out = t;
 *                 c > 0 and h < 0:  u_in = 0, u_out = min(t, -h / c);
 *                 c == 0 and h < 0: u_in = 0, u_out = t;
 *                 otherwise the segment is empty.
 *               A sample is ELIGIBLE when t > 0, t is not NaN and u_out > u_in.  S = u_out - u_in (may be inf).  D, the
 *               depth of the entry point below the top: -h when u_in = 0, else exactly 0.
 *   points      K = num_steps, 1..32.  xi_k: the FIRST number of the stream (r0, r1) = sample_tea_32(sample_tea_32(seed,
 *               k)[0], id_i), r0 >> 9 scaled by 2^-23 (hf_sky_lighting's convention, id_i = i or ray_id[i]; the second
 *               number is unused).  a = 1 - exp(-sigma_t S) (1 for S = inf), tau_k = -log1p(-xi_k a), u_k = u_in +
 *               tau_k / sigma_t: distance sampling in proportion to the transmittance (medium.cpp:71) truncated to the
 *               segment and normalised; every draw is a medium interaction and moves smoothly with S and sigma_t.
 *               xi < 1, so tau_k < sigma_t S.
 *   shadow ray  light j has nu_j = <l_j, N>.  A light with nu_j <= 0 contributes exact zeros: no bit is set and nothing
 *               is walked (decided on the host).  Otherwise o_ray = fmaf(float(u_k), d, o) per component, direction
 *               float32(l_j), maxt = inf.  Interaction::spawn_ray of a medium interaction has n = 0, so offset_p adds
 *               nothing (interaction.h:136-165).
 *   vis_bits[j][i]  one uint32: bit k is set iff the sample is eligible, light j shines in and the any-hit walk from
 *               point k found nothing.
 *   value       sums in double, in k order, rounded once:
 *                 p_ij  = (1 - g^2) / (4 pi temp^(3/2)),  temp = 1 + g^2 + 2 g <l_j, -d_i>     (hg.cpp:66-69, 99)
 *                 x_ijk = (sigma_t D_i - tau_k c_i) / nu_j            (optical depth from point k up to the top)
 *                 value[j][i] = weight_i albedo a_i p_ij E_j (1/K) sum_k bit_ijk exp(-x_ijk)
 *               formed from tau_k in double, never from the rounded ray origin: only the ray is float32.
 *   image[j][i / spp] = 1/spp * sum value[j][i]: hf_directional_lighting's box film and layout, overwritten.
 * Differentiated with respect to weight, t (through which the gradient reaches the heights and to_world), sigma_t,
 * albedo, g and every light's irradiance: HF_MEDIUM_PARAMS numbers, then one per light.  HELD: the bits and the branch
 * of the segment (dS/dt = 1 where u_out = t, 0 where the ray leaves through the top).  With T = (1/K) sum bit exp(-x):
 *   a_S = sigma_t exp(-sigma_t S),  a_sigma = S exp(-sigma_t S)  (both 0 for S = inf),  da = a_S dS + a_sigma dsigma,
 *   dtau_k = xi_k / (1 - xi_k a) da,   dx = (dsigma D - dtau c) / nu,
 *   dp/dg = (-2 g temp - 3 (1 - g^2)(g + cos)) / (4 pi temp^(5/2)).
 * OUT OF SCOPE: gradients for to_light, the top plane, o and d; multiple scattering; a heterogeneous medium; RGB;
 * emission; and the silhouette part of a moving shadow (hf_reparam_*'s, as in every row).
 * All entries refuse with HF_EINVAL, before anything touches a device: a NULL pointer that is not optional, n >= 2^32,
 * spp == 0 or n % spp != 0, num_steps outside 1..32 (hf_medium_rays: k >= 32), n_lights outside 1..HF_MAX_LIGHTS,
 * sigma_t not finite or <= 0, albedo not finite, |g| >= 1 or g not finite, a zero or non-finite top_normal or
 * top_origin, a non-finite field of a light, |to_light| zero.  Callers detect the entries by their symbols (HF_VERSION
 * is unchanged). */
typedef struct hf_medium {          /* HOST memory */
    double top_origin[3];           /* a point of the top plane */
    double top_normal[3];           /* out of the medium; any finite length > 0, the host normalises it once in double: N */
    float  sigma_t, albedo, g;      /* homogeneous.cpp:139-175 (sigma_s = albedo sigma_t), hg.cpp:66-69 */
} hf_medium_t;
#define HF_MEDIUM_PARAMS 3          /* sigma_t, albedo, g: then one irradiance per light */
/* hf_medium_rays materialises shadow ray k of every sample towards ONE light (out_o, out_d: 3 rows of n floats;
 * out_maxt: n floats, inf for a traced lane; a lane that is not traced gets a zero origin and direction and maxt = -1, a
 * miss): bit k of hf_medium_lighting's vis_bits row of that light equals hf_medium_rays + hf_ray_test bit for bit.
 * Takes no field handle.  ray_id: n ids or NULL (i). */
int hf_medium_rays(size_t n, const float *const o[3], const float *const d[3], const float *t, const hf_medium_t *medium,
                   const hf_directional_light_t *light, uint32_t k, uint32_t seed, const uint32_t *ray_id,
                   float *const out_o[3], float *const out_d[3], float *out_maxt, hf_stream_t stream);
/* The fused launch (hf_sky_lighting's mapping: one lane per sample): reads a sample's o, d, t and weight once and holds
 * them across the loop over its points, the wave-uniform loop over the lights inside it; draws, walks (any hit, per lane)
 * and reduces the film; image (J rows of n / spp), value (J rows of n) and vis_bits (J rows of n uint32) may each be NULL
 * (not wanted), not all of them; no ray and no hit byte goes to memory.  A batch of 64 samples with no eligible sample
 * draws nothing.  hf_set_ray_coherence is neither read nor changed.  weight: n floats or NULL (1).  Allocates nothing,
 * never synchronises the host, capturable. */
int hf_medium_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const o[3], const float *const d[3],
                       const float *t, const float *weight, const hf_medium_t *medium, uint32_t n_lights,
                       const hf_directional_light_t *lights, uint32_t num_steps, uint32_t seed, const uint32_t *ray_id,
                       float *image, float *value, uint32_t *vis_bits, hf_stream_t stream);
/* the adjoint's workspace in floats for a rig of n_lights (0 for a count outside 1..HF_MAX_LIGHTS): a row of
 * HF_MEDIUM_PARAMS + HF_MAX_LIGHTS doubles for every block the launch can get, whatever the count */
size_t hf_medium_workspace_floats(uint32_t n_lights);
/* Reverse mode.  Traces nothing: the points are drawn again and vis_bits (as hf_medium_lighting wrote it) is read.  With
 * the upstream of light j g_j = grad_image[j][i / spp] / spp + grad_value[j][i] (either may be NULL = zero):
 *   grad_weight = sum_j g_j d value_j / d weight,   grad_t = sum_j g_j d value_j / d t
 * (n floats each) are OVERWRITTEN, one lane per sample, the lights summed in light order in double and rounded once,
 * exact zeros where no bit is set, no atomics;
 *   grad_params ([HF_MEDIUM_PARAMS + n_lights] device floats: sigma_t, albedo, g, then the irradiance of every light)
 * is ACCUMULATED into without atomics: every block stores its partial sums in double to `workspace` --
 * hf_medium_workspace_floats(n_lights) floats of device memory, 8-byte aligned, the caller's, this call's until it has
 * completed; needed only when grad_params is wanted -- and one more launch adds them in a fixed order
 * (hf_directional_lighting_adjoint's pattern; family 2 of hf_grid_blocks): bitwise the same from launch to launch.  Every
 * output may be NULL (not wanted).  Takes no field handle. */
int hf_medium_lighting_adjoint(size_t n, uint32_t spp, const float *const o[3], const float *const d[3], const float *t,
                               const float *weight, const hf_medium_t *medium, uint32_t n_lights,
                               const hf_directional_light_t *lights, uint32_t num_steps, uint32_t seed,
                               const uint32_t *ray_id, const uint32_t *vis_bits, const float *grad_image,
                               const float *grad_value, float *grad_weight, float *grad_t, float *grad_params,
                               float *workspace, hf_stream_t stream);
/* Forward mode, the exact transpose of the adjoint, for tangents dweight (n), dt (n) and d_params ([HF_MEDIUM_PARAMS +
 * n_lights] device floats), each may be NULL (zero); dimage (J rows of n / spp) and / or dvalue (J rows of n) are
 * overwritten (at least one).  No atomics for any spp: bitwise the same from launch to launch.  Takes no field handle. */
int hf_medium_lighting_tangent(size_t n, uint32_t spp, const float *const o[3], const float *const d[3], const float *t,
                               const float *weight, const hf_medium_t *medium, uint32_t n_lights,
                               const hf_directional_light_t *lights, uint32_t num_steps, uint32_t seed,
                               const uint32_t *ray_id, const uint32_t *vis_bits, const float *dweight, const float *dt,
                               const float *d_params, float *dimage, float *dvalue, hf_stream_t stream);

/* ---- the bump map: the shading normal perturbed by the slopes of a height texture, fused, differentiable ----
 *
 * The reference's `bumpmap` (src/bsdfs/bumpmap.cpp:199-222, frame()) over Texture::eval_1_grad (src/textures/bitmap.cpp:
 * 346-423, bilinear filter, identity uv transform) as a map of the shading normal: a scalar relief f(u, v) laid over the
 * height grid, one float per texel.  Whatever it perturbs a normal to is the normal of a surface: the heightfield's own
 * idea continued below the grid spacing.  The result is a new sh_n; every lighting row takes it as it takes any other.
 * Everything is in WORLD space, in double from the float32 records, and each component of N is rounded ONCE.
 * Per sample i:
 *   inputs      uv (2 rows), b = sh_n (3 rows), n_geo = si.n (3 rows), dp_du, dp_dv (3 rows each) of n floats, active
 *               (n bytes; NULL: every lane);
 *   texture     tex[TH][TW], float32, ONE plane, the caller's device buffer: exactly a hf_bitmap_eval texture;
 *               wrap = HF_WRAP_CLAMP or HF_WRAP_REPEAT;  scale: a HOST float, the gradient's multiplier (bumpmap.cpp:108);
 *   lookup      pos = (float32(u TW), float32(v TH)), each product rounded once: the normal map's positions; (Lx, Ly) in
 *               float32 is bit for bit the out_grad hf_bitmap_eval writes for pos;
 *   gradient    g = scale (TW Lx, TH Ly)   (bitmap.cpp:399-418, bumpmap.cpp:201);
 *   frame       P_u = dp_du + b (g_x - k <b, dp_du>),  P_v = dp_dv + b (g_y - k <b, dp_dv>),  k = 1 / <b, b>
 *               (bumpmap.cpp:204-205, where the normal is unit and k = 1),
 *               c = P_u x P_v,  sigma = -1 if <n_geo, c> < 0, else +1 (bumpmap.cpp:212),  N = sigma c / |c|.
 * DEVIATION in k: the reference's formula is written for a unit normal.  A float32 b is unit only to rounding, |b|^2 = 1 + e,
 * and with k = 1 the projected tangents keep a component -e <b, dp_du> along b: c leaves b's direction by about e tan(angle
 * between b and the tangents' normal), which under smooth shading put a FLAT texture 1.125 x 2^-22 from b.  With k the
 * projection is exact for the b that arrives; for a unit b nothing changes.  k is DIFFERENTIATED, not held: N does not
 * depend on the length of b but through the term b g.
 * A lane is PERTURBED when it is active, uv, b, n_geo, dp_du and dp_dv are finite, the lookup reads something (under
 * HF_WRAP_REPEAT a coordinate beyond 2^23 texels reads nothing), |b|^2 > 0, |dp_du|^2 > 0, |dp_dv|^2 > 0 and |c|^2 >= 1e-12
 * |dp_du|^2 |dp_dv|^2.  Every other lane PASSES THROUGH: N = b bit for bit, its derivative is the identity on sh_n and zero for
 * everything else.  mask (n bytes, optional): 1 where perturbed, 0 elsewhere.
 * A FLAT texture (g = 0) gives N = +-b / |b| only TO ROUNDING, not bit for bit: the cross product of the projected
 * tangents is formed anew.  This differs from the normal map, whose flat map changes no bit.
 * DEVIATION, the one the normal map makes: the reference converts N to the local frame and rebuilds s and t; here only the
 * world-space N is returned, the one member of the frame a lighting row reads.
 * Differentiated with respect to tex, uv, sh_n, dp_du and dp_dv.  HELD: the cell, the perturbed / pass-through decision,
 * sigma and n_geo.  With f = (fx, fy) the position in the cell, the texels v00, v10, v01, v11, C = v11 - v10 - v01 + v00
 * and dpos = (TW du, TH dv) -- the derivative of the SLOPES, not of the value:
 *   dLx  = -(1 - fy) dv00 + (1 - fy) dv10 - fy dv01 + fy dv11 + C dpos_y,
 *   dLy  = -(1 - fx) dv00 - fx dv10 + (1 - fx) dv01 + fx dv11 + C dpos_x,
 *   dg   = scale (TW dLx, TH dLy),
 *   dP_u = ddp_du + db (g_x - k <b, dp_du>) + b (dg_x - k (<db, dp_du> + <b, ddp_du> - 2 k <b, dp_du> <b, db>)),  dP_v likewise
 *          (for a unit b and a db orthogonal to it -- the tangent of any normalised normal -- the last term is zero),
 *   dc   = dP_u x P_v + P_u x dP_v,   dN = sigma (dc - ch <ch, dc>) / |c|,   ch = c / |c|.
 * The adjoint is the exact transpose.
 * OUT OF SCOPE: a gradient for scale (g is linear in scale tex: scale is redundant with the texels, and the reference
 * marks it NonDifferentiable); a gradient for n_geo; the BSDF-side test cos_theta(wo) cos_theta(perturbed_wo) > 0
 * (bumpmap.cpp:139-146: the rows decide on <sh_n, l> as before); nearest filtering; an RGB texture taken by its luminance;
 * a uv transform; the mirror wrap; s and t.
 * All three entries refuse with HF_EINVAL, before anything touches a device: a NULL pointer that is not optional,
 * n >= 2^32, TW == 0 or TH == 0, TW TH >= 2^31, a wrap that is neither constant, a scale that is not finite.  n == 0 is legal
 * and launches nothing.  They take no field handle, allocate nothing, never synchronise the host and are capturable; one
 * launch each, one lane per sample.  Callers detect the entries by their symbols (HF_VERSION is unchanged). */
int hf_bumpmap_eval(size_t n, const float *const uv[2], const float *const sh_n[3], const float *const n_geo[3],
                    const float *const dp_du[3], const float *const dp_dv[3], const uint8_t *active, uint32_t TW, uint32_t TH,
                    const float *tex, int wrap, float scale, float *const out_n[3], uint8_t *mask, hf_stream_t stream);
/* Forward mode: dtex ([TH][TW]), duv (2 rows), dsh_n, ddp_du, ddp_dv (3 rows each) may each be NULL (zero); dout_n (3 rows)
 * is overwritten.  Bitwise the same from launch to launch. */
int hf_bumpmap_eval_tangent(size_t n, const float *const uv[2], const float *const sh_n[3], const float *const n_geo[3],
                            const float *const dp_du[3], const float *const dp_dv[3], const uint8_t *active, uint32_t TW,
                            uint32_t TH, const float *tex, int wrap, float scale, const float *dtex,
                            const float *const duv[2], const float *const dsh_n[3], const float *const ddp_du[3],
                            const float *const ddp_dv[3], float *const dout_n[3], hf_stream_t stream);
/* Reverse mode: grad_out (3 rows) is dL/dN.  grad_tex ([TH][TW]) is ACCUMULATED into with float atomics, four per
 * perturbed sample with the slopes' weights above -- fewer where consecutive lanes of a wave share a cell: they add theirs
 * up first -- in a free order: repeatable to rounding; grad_uv (2 rows), grad_sh_n, grad_dp_du and grad_dp_dv (3 rows each)
 * are OVERWRITTEN, with exact zeros where nothing flows; a pass-through lane hands grad_out to grad_sh_n.  Each output may
 * be NULL (not wanted), not all of them. */
int hf_bumpmap_eval_adjoint(size_t n, const float *const uv[2], const float *const sh_n[3], const float *const n_geo[3],
                            const float *const dp_du[3], const float *const dp_dv[3], const uint8_t *active, uint32_t TW,
                            uint32_t TH, const float *tex, int wrap, float scale, const float *const grad_out[3],
                            float *grad_tex, float *const grad_uv[2], float *const grad_sh_n[3],
                            float *const grad_dp_du[3], float *const grad_dp_dv[3], hf_stream_t stream);

/* ---- next row: bounce lighting, one diffuse interreflection traced in the kernel ----
 *
 * The bounce of prb_reparam (src/python/python/ad/integrators/prb.py:162-226) for diffuse surfaces under directional
 * lights (src/emitters/directional.cpp), cut after the second vertex: a DETACHED BSDF sample at the first vertex
 * (diffuse.cpp:101-143: cosine-weighted direction, weight = albedo), the closest hit q of the spawned ray, and the
 * emitter-sampling term at q with its own shadow rays; Lr_ind = L * replace_grad(1, bsdf_val / bsdf_val_det)
 * (prb.py:213-223) makes the cosine at the first vertex differentiable.  Averaged over K = num_rays directions.
 *   samples     (r0, r1) = sample_tea_32(sample_tea_32(seed, k)[0], id_i), sample = (r0 >> 9, r1 >> 9) * 2^-23: the
 *               stream of hf_sky_* and hf_reparam_* with pair = k; id_i = i or ray_id[i].  A caller that uses several
 *               of these rows gives them different seeds;
 *   direction   wo = square_to_cosine_hemisphere(sample) (warp.h:54-90, 320-328: the concentric disk map, then
 *               z = safe_sqrt(1 - x^2 - y^2), evaluated as sqrt((1 - |r|) (1 + |r|)) with r the map's radius, the same
 *               number without the cancellation); w_k = s wo.x + t wo.y + sh_n wo.z with (s, t) = coordinate_system(sh_n)
 *               (vector.h:116-136).  DEVIATION: the reference rotates with the Gram-Schmidt sh_frame.s / .t of the
 *               interaction; a cosine lobe does not depend on the rotation about sh_n, so the frame is rebuilt from
 *               sh_n alone and six input rows are saved.  The sampled directions differ, their distribution does not;
 *   eligible    sample i when t_i is finite and <sh_n_i, -d_i> > 0 (the masks of hf_direct_lighting); direction k of
 *               an eligible sample is TRACED when wo.z > 0;
 *   bounce ray  SurfaceInteraction::spawn_ray(w_k) exactly as hf_sky_rays builds it (interaction.h:134-136, 161-165),
 *               maxt = +inf; its closest hit (t_q, prim_q) is hf_ray_intersect_preliminary's for that ray, bit for bit;
 *   2nd vertex  q and n_q: the p and n of hf_compute_surface_interaction for that ray and hit; n_q is the FACE normal
 *               (after flip_normals) under both shading modes of the handle: the first vertex takes the caller's sh_n,
 *               flat or smooth, but smoothing the normal of an indirect vertex is a second-order effect and would put
 *               1-rings of vertices into the fused adjoint.  front_ik = hit and <n_q, -w_k> > 0;
 *   light l     shadow ray traced when front_ik and <n_q, l_l> > 0: spawn_ray(l_l) from (q, n_q), the same offset
 *               rule, maxt = +inf; lit_ikl = traced and the any-hit walk finds nothing;
 *   value       R_ikl = albedo/pi E_l lit_ikl <n_q, l_l>,  value_il = weight_i (albedo / K) sum_k R_ikl
 *   image[l][i / spp] = 1/spp * sum value_il: the box film and per-light rows of hf_direct_lighting, overwritten, so
 *               the rows add onto that function's; n a multiple of spp;
 *   record      of direction k of sample i at [k * sample_stride + i], sample_stride >= n: hit_prim (uint32) = prim_q
 *               where the bounce ray hit, 0xFFFFFFFF where it missed or was not traced; lit_bits (uint8): bit l set
 *               iff lit_ikl.  Either pointer may be NULL in the forward (not wanted).
 * A bounce ray that misses contributes nothing: light from the environment is hf_sky_lighting's term.  The rays take
 * the float32 direction; the derivative kernels form w_k / z_k and their sums from the same sample in double and round
 * once (1 - |p|^2 cancels near the rim of the disk).  Not differentiated: visibility and the masks (piecewise
 * constant; silhouettes are hf_reparam_*'s) and to_world (no grad_to_world / d_to_world here).
 * All four entries: 1 <= num_rays <= 32 (hf_bounce_rays: k < 32), n < 2^32, 1 <= n_lights <= HF_MAX_LIGHTS (lights in
 * HOST memory); NULL pointers other than those marked optional, a NULL row of a row triple, n % spp != 0, spp == 0,
 * sample_stride < n with a record pointer given, non-finite albedo, irradiance or light direction are refused with
 * HF_EINVAL before anything touches a device; n == 0 is legal.  They allocate nothing, never synchronise the host and
 * are capturable (no work counter, no scratch block).  Callers detect the entries by their symbols (HF_VERSION is
 * unchanged).
 *
 * hf_bounce_rays materialises ray k of every sample (out_o, out_d: 3 rows of n floats; out_maxt: n floats, +inf for a
 * lane the fused kernel traces and -1 -- a miss -- for every other).  to_light == NULL: the bounce ray.  to_light = 3
 * HOST floats: the shadow ray from that bounce ray's hit towards to_light; this form traces the bounce ray. */
int hf_bounce_rays(const hf_field_t *hf, size_t n, const float *const p[3], const float *const nrm[3],
                   const float *const sh_n[3], const float *const d[3], const float *t, uint32_t k, uint32_t seed,
                   const uint32_t *ray_id, const float *to_light, float *const out_o[3], float *const out_d[3],
                   float *out_maxt, hf_stream_t stream);
/* The fused launch: reads a sample's record once, draws its K directions, walks each traced one to its closest hit per
 * lane, shades the hit under every light with a per-lane any-hit walk, and writes the two record words and the film.
 * A batch of 64 samples without an eligible one traces nothing.  Every wave walks per lane, whatever
 * hf_set_ray_coherence says.  weight: n floats or NULL (1).  image: n_lights * (n / spp) floats. */
int hf_bounce_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3], const float *const nrm[3],
                       const float *const sh_n[3], const float *const d[3], const float *t, const float *weight,
                       uint32_t num_rays, uint32_t seed, const uint32_t *ray_id, uint32_t n_lights,
                       const hf_dir_light_t *lights, float albedo, float *image, uint32_t *hit_prim, uint8_t *lit_bits,
                       size_t sample_stride, hf_stream_t stream);
/* Reverse mode.  Traces nothing: the directions are drawn again, the record is read and n_q recomputed from hit_prim
 * and the heights.  With g_l = grad_image[l][i / spp] / spp, c = albedo / K, G_ik = sum_l g_l R_ikl:
 *   grad_sh_n[i]   = weight_i c sum_k G_ik w_k / z_k        (z_k = the sampled wo.z)
 *   grad_weight[i] = c sum_k G_ik
 * both overwritten, exact zeros for samples that are not eligible, sums in k order without atomics; and for every
 * record with lit_bits != 0 the gradient gN = weight_i c albedo/pi sum_l g_l E_l lit_ikl l_l of n_q goes through the
 * flip, the normalisation and the cross product to the three heights of prim_q, ACCUMULATED into grad_heights[H W]
 * with float atomics.  grad_sh_n, grad_weight, grad_heights may each be NULL, not all of them. */
int hf_bounce_lighting_adjoint(const hf_field_t *hf, size_t n, uint32_t spp, const float *const sh_n[3],
                               const float *const d[3], const float *t, const float *weight, uint32_t num_rays,
                               uint32_t seed, const uint32_t *ray_id, uint32_t n_lights, const hf_dir_light_t *lights,
                               float albedo, const uint32_t *hit_prim, const uint8_t *lit_bits, size_t sample_stride,
                               const float *grad_image, float *const grad_sh_n[3], float *grad_weight,
                               float *grad_heights, hf_stream_t stream);
/* Forward mode, the transpose of the adjoint: for tangents dsh_n (3 rows of n floats), dweight (n floats) and dheights
 * (H W floats), each NULL = zero,
 *   dimage[l][i / spp] = 1/spp sum c (weight_i <dsh_n_i, sum_k R_ikl w_k / z_k> + dweight_i sum_k R_ikl
 *                                      + weight_i sum_k albedo/pi E_l lit_ikl <dn_q, l_l>)
 * overwritten.  No atomics for any spp (a power of two <= 64: the film's shuffle tree; otherwise one lane adds the
 * samples of a pixel in order): bitwise the same from launch to launch. */
int hf_bounce_lighting_tangent(const hf_field_t *hf, size_t n, uint32_t spp, const float *const sh_n[3],
                               const float *const d[3], const float *t, const float *weight, uint32_t num_rays,
                               uint32_t seed, const uint32_t *ray_id, uint32_t n_lights, const hf_dir_light_t *lights,
                               float albedo, const uint32_t *hit_prim, const uint8_t *lit_bits, size_t sample_stride,
                               const float *const dsh_n[3], const float *dweight, const float *dheights, float *dimage,
                               hf_stream_t stream);

/* Film with a Gaussian reconstruction filter (the reference's default rfilter, src/rfilters/gaussian.cpp:48-101:
 * w(x) = max(0, exp(-x^2 / (2 stddev^2)) - exp(-r^2 / (2 stddev^2))), r = 4 stddev), splatted as ImageBlock::put does
 * (src/render/imageblock.cpp:258-330): sample i at film position (pos_x[i], pos_y[i]) (pixel units; pixel (x, y)
 * covers [x, x+1) x [y, y+1)) adds w(x - (pos_x - 0.5)) w(y - (pos_y - 0.5)) * values[c][i] to image[c][y*width + x]
 * and the weight alone to weight[y*width + x] for every pixel within r; image and weight are ACCUMULATED (zero them
 * first), the film is image / weight (HDRFilm::develop).  values: `channels` (<= HF_MAX_LIGHTS) device arrays of n
 * floats -- e.g. the rows of hf_direct_lighting(..., spp = 1, ...), which are the per-sample values.  0 < stddev <= 1.
 * The adjoint gathers: grad_values[c][i] = sum_pixels w * grad_image[c][pixel], grad_image = dL/d(accumulated image)
 * (for a loss on the normalised film: dL/d(film) / weight); the weights do not depend on the samples' values. */
int hf_film_splat(size_t n, uint32_t channels, const float *const *values, const float *pos_x, const float *pos_y,
                  uint32_t width, uint32_t height, float stddev, float *image, float *weight, hf_stream_t stream);
int hf_film_splat_adjoint(size_t n, uint32_t channels, const float *pos_x, const float *pos_y, uint32_t width,
                          uint32_t height, float stddev, const float *grad_image, float *const *grad_values,
                          hf_stream_t stream);

/* The same film for samples that move and carry a weight: ImageBlock::put(pos, value, weight) with the position
 * attached (src/render/imageblock.cpp:264-400 evaluates the filter of src/rfilters/gaussian.cpp:48-101 analytically on
 * it), which is what a reparameterised integrator needs -- value = L det and weight = det splatted at the film position
 * of the warped ray (src/python/python/ad/integrators/common.py:383-405).  Filter and footprint are exactly
 * hf_film_splat's: x = px - (pos_x - 0.5), pixels ceil(pos - 0.5 - r) .. floor(pos - 0.5 + r) clamped to the film,
 * w(x) = max(0, e^(alpha x^2) - e^(alpha r^2)), alpha = -1 / (2 stddev^2), r = 4 stddev, f = w(x) w(y).  Its derivative:
 * w'(x) = 2 alpha x e^(alpha x^2) where w(x) > 0, else 0, and df/dpos_x = -w'(x) w(y); w is continuous at the radius,
 * so the clamped footprint has no boundary term.  All three take device pointers, launch on `stream`, allocate nothing,
 * never synchronise and can be captured; arguments are checked as for hf_film_splat.
 *
 * hf_film_splat_weighted accumulates  image[c][pix] += f values[c][i]  and  weight[pix] += f sample_weight[i]
 * (sample_weight: n floats, NULL = 1: the sums of hf_film_splat up to the order of the float atomics). */
int hf_film_splat_weighted(size_t n, uint32_t channels, const float *const *values, const float *sample_weight,
                           const float *pos_x, const float *pos_y, uint32_t width, uint32_t height, float stddev,
                           float *image, float *weight, hf_stream_t stream);
/* Reverse mode (common.py:868-970): grad_image [channels][H W] = dL/d(accumulated image), grad_weight [H W] =
 * dL/d(accumulated weight) (NULL = zero).  With G_i(pix) = sum_c values[c][i] grad_image[c][pix] + sample_weight[i]
 * grad_weight[pix]:
 *   grad_values[c][i]     = sum_pix f grad_image[c][pix]
 *   grad_sample_weight[i] = sum_pix f grad_weight[pix]
 *   grad_pos_x[i]         = sum_pix -w'(x) w(y) G_i(pix),   grad_pos_y[i] = sum_pix -w(x) w'(y) G_i(pix)
 * Every output is overwritten; any of them may be NULL (not wanted), not all.  values may be NULL unless a position
 * gradient is asked for.  A gather without atomics: bitwise the same from launch to launch. */
int hf_film_splat_weighted_adjoint(size_t n, uint32_t channels, const float *const *values, const float *sample_weight,
                                   const float *pos_x, const float *pos_y, uint32_t width, uint32_t height, float stddev,
                                   const float *grad_image, const float *grad_weight,
                                   float *const *grad_values, float *grad_sample_weight,
                                   float *grad_pos_x, float *grad_pos_y, hf_stream_t stream);
/* Forward mode (common.py:705-780, sample_pos_deriv), the exact transpose of the adjoint: tangents dvalues, dsample_weight,
 * dpos_x, dpos_y (each may be NULL = zero) give, with df = -w'(x) w(y) dpos_x[i] - w(x) w'(y) dpos_y[i],
 *   dimage[c][pix] += f dvalues[c][i] + df values[c][i],   dweight[pix] += f dsample_weight[i] + df sample_weight[i]
 * ACCUMULATED with float atomics like the primal (zero them first); a contribution that is exactly zero adds nothing. */
int hf_film_splat_weighted_tangent(size_t n, uint32_t channels, const float *const *values, const float *sample_weight,
                                   const float *pos_x, const float *pos_y, uint32_t width, uint32_t height, float stddev,
                                   const float *const *dvalues, const float *dsample_weight,
                                   const float *dpos_x, const float *dpos_y,
                                   float *dimage, float *dweight, hf_stream_t stream);

/* ---- next row: warped-area reparameterisation of rays ---------- */

/* The auxiliary-ray machinery of mitsuba.ad.reparameterize_ray (src/python/python/ad/reparam.py:10-123,
 * 224-333; Bangaru et al. 2020) for a scene that is this one shape, split into the two per-sample kernels
 * its three loops are made of; the auxiliary rays themselves are traced by hf_ray_intersect with
 * HF_RAY_ALL | HF_RAY_FOLLOWSHAPE | HF_RAY_BOUNDARYTEST (reparam.py:93-95) and the gradient of an
 * auxiliary hit reaches the heights through hf_adjoint with the same flags.
 * Random numbers: the reference draws two PCG32 floats per auxiliary ray (reparam.py:186); PCG32 lives in
 * the absent Dr.Jit, so sample (k, ray i) is sample_tea_32(key, id_i) with key = sample_tea_32(seed, pair)[0]
 * (include/mitsuba/core/random.h:76-91) -> two 23-bit floats, pair = k/2 with antithetic sampling (the even
 * iteration of a pair reuses the sample with omega_local.xy negated, reparam.py:83-85,188-190), else k.
 * id_i = i, the ray's index in the launch, or ray_id[i] (device array of n uint32, may be NULL): the index of the ray
 * in a larger wavefront of which this launch traces a part (a rank's image tiles: index = pixel * spp + sample) -- the
 * sharded launches then draw exactly the samples of the unsharded one (the reference seeds its sampler with the
 * wavefront index the same way, src/render/sampler.cpp:116-130).  All four hf_reparam_* calls of one ray take the
 * same seed and ray_id.
 *
 * hf_reparam_aux_rays: auxiliary ray k of every primary ray (o, d; d unit length): direction =
 * Frame3f(d).to_world(square_to_von_mises_fisher(sample, kappa)) (warp.h:546-583, frame.h:39-41,
 * vector.h:116-136), origin o, maxt = inf; inactive lanes get maxt = -1 (a miss). kappa > 0. */
int hf_reparam_aux_rays(size_t n, const float *const o[3], const float *const d[3], const uint8_t *active,
                        uint32_t k, float kappa, int antithetic, uint32_t seed, const uint32_t *ray_id,
                        float *const aux_d[3], float *aux_maxt, hf_stream_t stream);
/* hf_reparam_weights, mode 0 (reparam.py:97-121, first loop of backward :224-256): from the auxiliary hit
 * (si_t, si_boundary_test) the harmonic weight w = (1 / (D - 1 + B))^exponent * D and its tangential
 * gradient d_w_omega; accumulates Z[n] += w, dZ[3][n] += d_w_omega.
 * mode 1 (third loop :283-325 for the shape parameter): with the totals Z, dZ and the upstream gradients of
 * the outputs, grad_direction[3][n] and grad_divergence[n] (reparam.py:262-281: direction =
 * normalize(d + V / Z), divergence = (div - <V / Z, dZ>) / Z at V = 0), the gradient of this sample's
 * V_direct = (si.p - o) / si.t is written as upstream gradient of the auxiliary hit: grad_p[3][n] and
 * grad_t[n] (zero for misses), to be handed to hf_adjoint as hf_si_grad_t {p, t} with HF_RAY_FOLLOWSHAPE.
 * grad_vd (optional, NULL = not wanted): the gradient with respect to this sample's V_direct itself,
 * grad_vd[3][n] (zero for inactive lanes).  It is what the RAY needs (reparam.py:296-325 back-propagates to
 * ray.o and ray.d as well): for a hit, dL/d(ray.o) = [grad_o of hf_adjoint] - grad_p; for a miss V_direct is
 * ray.d itself and dL/d(ray.d) = grad_vd; dL/d(auxiliary direction) = [grad_d of hf_adjoint] is carried to
 * ray.d through Frame3f(ray.d) by the host (mirror: hf_amd.reparameterize_ray). */
int hf_reparam_weights(int mode, size_t n, const float *const o[3], const float *const d[3],
                       const uint8_t *active, uint32_t k, float kappa, float exponent, int antithetic,
                       uint32_t seed, const uint32_t *ray_id, const float *si_t, const float *const si_p[3],
                       const float *si_boundary_test,
                       float *Z, float *const dZ[3], const float *const grad_direction[3],
                       const float *grad_divergence, float *const grad_p[3], float *grad_t,
                       float *const grad_vd[3], hf_stream_t stream);
/* hf_reparam_aux_rays + hf_ray_intersect in one launch: traces auxiliary ray k of every ray (o, d) with
 * HF_RAY_ALL | HF_RAY_FOLLOWSHAPE | HF_RAY_BOUNDARYTEST (reparam.py:93-95) without materialising the auxiliary rays;
 * inactive lanes are misses.  out_pi / out_si as in hf_ray_intersect (si.wi is expressed for the auxiliary direction).
 * Bitwise the two-call sequence. */
int hf_reparam_trace(const hf_field_t *hf, size_t n, const float *const o[3], const float *const d[3],
                     const uint8_t *active, uint32_t k, float kappa, int antithetic, uint32_t seed,
                     const uint32_t *ray_id, const hf_pi_t *out_pi, const hf_si_t *out_si, hf_stream_t stream);
/* hf_reparam_trace for samples 0 .. num_rays - 1 in ONE launch: sample k of ray i goes to [k * sample_stride + i] of
 * every row of out_pi / out_si (the layout hf_reparam_backward reads).  A ray is fetched once and its samples are
 * traced back to back; and because every von Mises-Fisher sample lies within theta_max of the ray (cos theta_max =
 * 1 - 13.82 / kappa, warp.h:557-566), a batch of rays whose cones all miss the bound is answered with num_rays miss
 * records without a sample being drawn (not when out_si->wi is asked for).  Bitwise num_rays x hf_reparam_trace. */
int hf_reparam_trace_all(const hf_field_t *hf, size_t n, const float *const o[3], const float *const d[3],
                         const uint8_t *active, uint32_t num_rays, float kappa, int antithetic, uint32_t seed,
                         const uint32_t *ray_id, const hf_pi_t *out_pi, const hf_si_t *out_si, size_t sample_stride,
                         hf_stream_t stream);
/* The same backward pass in ONE kernel for the case that only the heights are differentiated (grad(ray) not wanted):
 * for every ray the weights of its num_rays samples and their sums Z, dZ (reparam.py:236-256), then for every
 * auxiliary HIT the gradient of its V_direct through the FollowShape surface interaction into grad_heights[H*W]
 * (accumulated, +=; reparam.py:296-325).  Inputs are the auxiliary hits only -- what hf_ray_intersect returned for
 * the rays of hf_reparam_aux_rays with HF_RAY_ALL | HF_RAY_FOLLOWSHAPE | HF_RAY_BOUNDARYTEST: sample k of ray i at
 * index [k * sample_stride + i] of pi->t / prim_uv / prim_index and of si_boundary_test.  The auxiliary directions are
 * regenerated from (d, k, seed); si.p and si.t are re-derived from pi with compute_surface_interaction's expressions,
 * so the result equals num_rays x (hf_reparam_weights mode 0), then num_rays x (mode 1 + hf_adjoint) up to the order
 * of the float atomics.  1 <= num_rays <= 32. */
int hf_reparam_backward(const hf_field_t *hf, size_t n, const float *const o[3], const float *const d[3],
                        const uint8_t *active, uint32_t num_rays, float kappa, float exponent, int antithetic,
                        uint32_t seed, const uint32_t *ray_id, const hf_pi_const_t *pi, const float *si_boundary_test,
                        size_t sample_stride,
                        const float *const grad_direction[3], const float *grad_divergence, float *grad_heights,
                        hf_stream_t stream);
/* Forward mode of the same reparameterisation (_ReparameterizeOp.forward(), src/python/python/ad/reparam.py:155-221;
 * src/render/tests/test_reparameterization.py:29-98 checks it), in ONE kernel from the same kept auxiliary hits as
 * hf_reparam_backward (pi and si_boundary_test at [k * sample_stride + i], as hf_reparam_trace_all writes them) and the
 * same samples (seed, ray_id, antithetic).  Tangents, any subset, NULL = zero: dheights (device H*W floats), d_o[3] /
 * d_d[3] (device rows of n floats; the arrays or single rows may be NULL), d_to_world (12 device floats, row-major 3x4).
 * The weights w_k, d_w_omega_k are detached (B = si.boundary_test for a hit, 1 for a miss); Z = sum w_k and
 * dZ = sum d_w_omega_k in sample order.  dV_k is the tangent of V_direct_k = (p - o) / t for a hit (FollowShape p with
 * detached barycentrics, t = sqrt(|p - o|^2 / |d_aux|^2), d_aux = Frame3f(d).to_world(omega_k), omega_k detached) and
 * d_d for a miss.  Writes out_direction[3][n] = V_theta = sum_k w_k dV_k / max(Z, 1e-8) and out_divergence[n] =
 * (sum_k <d_w_omega_k, dV_k> - <V_theta, dZ>) / max(Z, 1e-8), overwritten; inactive lanes get 0.  The primal outputs
 * are (d, 1).  No atomics (bitwise repeatable), no allocation, capturable.  1 <= num_rays <= 32. */
int hf_reparam_tangent(const hf_field_t *hf, size_t n, const float *const o[3], const float *const d[3],
                       const uint8_t *active, uint32_t num_rays, float kappa, float exponent, int antithetic,
                       uint32_t seed, const uint32_t *ray_id, const hf_pi_const_t *pi, const float *si_boundary_test,
                       size_t sample_stride, const float *dheights, const float *const d_o[3],
                       const float *const d_d[3], const float *d_to_world, float *const out_direction[3],
                       float *out_divergence, hf_stream_t stream);
/* Reverse mode of the same reparameterisation with respect to EVERYTHING attached -- the heights, ray.o, ray.d and
 * to_world -- in ONE kernel: the transpose of hf_reparam_tangent, from the same inputs (the kept auxiliary hits at
 * [k * sample_stride + i], the samples regenerated from (d, k, seed, ray_id, antithetic), si.p and the FollowShape
 * si.t re-derived from pi; weights detached).  Outputs, any subset, NULL = not wanted, at least one:
 *   grad_heights  H*W device floats, accumulated (+=) with float atomics, as hf_reparam_backward;
 *   grad_o[3], grad_d[3]  device rows of n floats, OVERWRITTEN; inactive lanes get exact zeros;
 *   grad_to_world  12 device floats (row-major 3x4), accumulated (+=) through the slab reduction of
 *                  hf_adjoint_transform: partial sums added in a fixed order, no float atomics.
 * With gVd the gradient of a sample's V_direct: a hit gives (gp, gt) of V_direct = (p - o) / t,
 * gp_tot = gp + gt (p - o) / (t |d_aux|^2); the vertices k of the hit triangle receive b_k gp_tot (heights: its
 * component along max_height to_world[:, 2]; to_world: b_k gp_tot (q_k, 1)^T), grad_o -= gp_tot, and d_aux receives
 * -gt t d_aux / |d_aux|^2, which goes on to ray.d through d_aux = s(d) omega.x + t(d) omega.y + d omega.z.  A miss on
 * an active lane has V_direct = ray.d: grad_d += gVd.  grad_o / grad_d / grad_to_world are bitwise repeatable.
 * Capturable, never synchronises; allocates nothing (grad_to_world leases one scratch block of the handle's ring).
 * Callers detect the entry point by its symbol (HF_VERSION is unchanged).  1 <= num_rays <= 32. */
int hf_reparam_backward_full(const hf_field_t *hf, size_t n, const float *const o[3], const float *const d[3],
                             const uint8_t *active, uint32_t num_rays, float kappa, float exponent, int antithetic,
                             uint32_t seed, const uint32_t *ray_id, const hf_pi_const_t *pi,
                             const float *si_boundary_test, size_t sample_stride,
                             const float *const grad_direction[3], const float *grad_divergence,
                             float *grad_heights, float *const grad_o[3], float *const grad_d[3],
                             float *grad_to_world, hf_stream_t stream);

/* ---- scalar / packet entry -----------------------------------------------------
 * Shape::ray_intersect_preliminary_scalar / _packet and ray_test_scalar / _packet
 * (include/mitsuba/render/shape.h:220-240, wrapper macros :594-641): the forms the scalar and LLVM
 * variants call per kd-tree leaf (include/mitsuba/render/kdtree.h:2490-2520) and from Embree's user-geometry
 * callbacks (src/render/shape.cpp:125-223) with 1, 4, 8 or 16 rays held in HOST registers.  These two entry
 * points take HOST pointers (SoA, n <= HF_PACKET_MAX), stage the packet through a per-thread pinned buffer and
 * a per-thread stream, run the same traversal kernel and return when the results are back in the host arrays
 * (synchronous, thread-safe, any number of threads).  One call costs a kernel launch and two PCIe round trips
 * (tens of microseconds): it exists so that an adapter can serve those call sites with the SAME arithmetic;
 * a renderer should hand whole wavefronts to the device entry points above.  `active` NULL = all lanes.
 * Inactive / missed lanes: t = +inf, prim_uv = 0, prim_index = 0; hit = 0. */
#define HF_PACKET_MAX 16
int hf_ray_intersect_preliminary_packet(const hf_field_t *hf, uint32_t n, const float *const h_o[3],
                                        const float *const h_d[3], const float *h_maxt, const uint8_t *h_active,
                                        float *h_t, float *const h_prim_uv[2], uint32_t *h_prim_index);
int hf_ray_test_packet(const hf_field_t *hf, uint32_t n, const float *const h_o[3], const float *const h_d[3],
                       const float *h_maxt, const uint8_t *h_active, uint8_t *h_hit);

/* ---- next row: large-steps preconditioning of the height grid (Nicolet et al. 2021) ----
 *
 * The reference's mitsuba.ad.largesteps.LargeSteps (src/python/python/ad/largesteps.py) for a heightfield: the optimiser
 * steps the latent u = (I + lambda L) v instead of the heights v, and every step solves (I + lambda L) v = u.
 *   L           the combinatorial Laplacian of the tessellation (every cell split along v10-v01), as mesh_laplacian
 *               (largesteps.py:6-28) builds it from the faces.  Vertex (i, j) -- row i, column j, index i W + j -- is
 *               adjacent to (i, j-1), (i, j+1), (i-1, j), (i+1, j), (i+1, j-1), (i-1, j+1), where they exist:
 *               (A v)_ij = v_ij + lambda (deg_ij v_ij - sum of the neighbours),  A = I + lambda L,
 *               deg the number of neighbours that exist (6 inside, 4 on an edge, 2 or 3 at the corners).  Nothing wraps
 *               or mirrors.  A is symmetric, its spectrum lies in [1, 1 + 12 lambda], 1^T A = 1^T.
 *   arithmetic  float32, one rounding per operation, nothing fused: the neighbours summed in the order listed above,
 *               then v + lambda (deg v - sum).  lambda is rounded to float32 once.
 *   solve       conjugate gradients, float32 vectors, the dot products accumulated in double (one double per block, the
 *               blocks' partials added in one fixed order: no float atomics; bitwise the same from call to call for a
 *               given grid and HF_FORCE_GRID), alpha and beta computed in double and rounded once.  Starts from v
 *               (warm != 0) or from 0 (v is write-only); ends when the recursive residual satisfies
 *               |r| <= rel_tol |u| (tested before every iteration, the first included) or after max_iter iterations.
 *               u = 0 gives v = 0 exactly, whatever the guess.  A NaN or an infinity in the input spreads; the call
 *               still ends.
 *   sum         A 1 = 1: the constant field is an eigenvector of A, and sum(u - A v) = sum(u) - sum(v).  After the last
 *               iteration (sum(u) - sum(v)) / (W H), both sums in double, is added to every v: the exact solve in that
 *               eigenspace.  It takes the mean out of the true residual (whose norm cannot grow), so that the solve
 *               keeps the sum of its right-hand side to float32 rounding, which the recursion alone does not.
 *   launches    1 + 2 max_iter + 2, the same whatever the data: the solve never synchronises with the host and can be
 *               captured in a HIP graph.  The launches after convergence return after one load of a device word.
 *   workspace   hf_large_steps_workspace_floats(W, H) floats of device memory, 16-byte aligned, the caller's; exclusively
 *               this solve's until it has completed.  (r, q, two p buffers, the blocks' partial sums, the scalars.)
 *   info        2 device floats, may be NULL: { iterations performed, the final |r| / |u| (0 for u = 0) }.
 * Free functions on caller buffers; no field handle.  Refused with HF_EINVAL before anything touches a device: NULL u, v
 * or workspace, W or H below 2 or above hf_create's limits (32768 cells per side, 2^30 vertices), lambda negative or not
 * finite, rel_tol negative or NaN, max_iter == 0, u == v, a workspace that is not 16-byte aligned.  Callers detect the
 * entries by their symbols (HF_VERSION is unchanged). */
/* the workspace of a solve in floats; 0 for W < 2 or H < 2 */
size_t hf_large_steps_workspace_floats(uint32_t W, uint32_t H);
/* u = A v (LargeSteps.to_differential); also its own adjoint and tangent */
int hf_large_steps_apply(uint32_t W, uint32_t H, double lambda, const float *v, float *u, hf_stream_t stream);
/* v ~= A^-1 u (LargeSteps.from_differential); its adjoint and tangent are the solve of the incoming gradient / tangent */
int hf_large_steps_solve(uint32_t W, uint32_t H, double lambda, const float *u, float *v, int warm, uint32_t max_iter,
                         float rel_tol, float *workspace, float *info, hf_stream_t stream);

/* ---- multi-GPU -------------------------------------------------------------------
 * Rays shard over image tiles, heights and acceleration data are replicated, every GPU accumulates a private
 * dL/dheight texture; this is the ONE collective of the path: an in-place sum all-reduce (float32) of that
 * texture over RCCL / xGMI, enqueued on `stream` (so it is ordered after the hf_adjoint launches of that stream
 * and can overlap the next wavefront's forward pass running on another stream).
 * `rccl_comm` is the caller's ncclComm_t for this rank (ncclCommInitRank by the host application), as void*.
 * RCCL is bound at first use: the ncclAllReduce already present in the process (the host's own RCCL, so that
 * the communicator and the call come from the same library), otherwise librccl.so is loaded.
 * Returns HF_EDEVICE if RCCL cannot be found or reports an error. */
int hf_allreduce_grad(float *d_grad, size_t count, void *rccl_comm, hf_stream_t stream);

/* ---- introspection (tests / tools) --------------------------------------------- */
int hf_num_levels(const hf_field_t *hf);
/* copies mip level `level` (1..num_levels) to HOST memory as (min,max) pairs,
 * row-major w x h; out may be NULL to query w,h.  Synchronises. */
int hf_get_mip(const hf_field_t *hf, int level, float *h_out, uint32_t *w, uint32_t *h);
/* copies the acceleration data of the nodes of level `level` (1..num_levels) to HOST memory exactly as stored: the
 * whole padded level, *side x *side slots with *side = 2^(num_levels - level), row-major by (iy, ix), nodes beyond
 * the grid included.  h_records: 12 floats per slot, the node record the traversal reads,
 * { a, b, c, f, lo0, hi0, lo1, hi1, lo2, hi2, lo3, hi3 }; h_minmax: 2 floats per slot, the (min, max) of the pyramid
 * at the same depth.  Either output may be NULL (both: queries *side).  Synchronises; not capturable. */
int hf_get_node_level(const hf_field_t *hf, int level, float *h_records, float *h_minmax, uint32_t *side);
/* inverse of a row-major 3x4 affine matrix (double precision, rounded to float) */
int hf_invert_affine(const float in[12], float out[12]);
/* blocks (of 256 threads) that a grid-stride launch of n items gets, HF_FORCE_GRID included.  family: 0 the flat cap
 * (adjoints, reparameterisation, Adam, area sampling, ...), 1 the cap of the streaming kernels (SI, hf_tangent, the
 * forward and tangent of attributes and of eval_parameterization, the sensor's rays, projection and their tangents), 2
 * the cap of the launches that sum dL/d(to_world), the sensor's adjoints, hf_projector_lighting_adjoint,
 * hf_spot_lighting_adjoint, hf_directional_lighting_adjoint, hf_specular_lighting_adjoint and hf_medium_lighting_adjoint among them.
 * 0 for an unknown family.  Needs no device. */
int hf_grid_blocks(size_t n, int family);
const char *hf_last_error_string(void);
int hf_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HF_H */
