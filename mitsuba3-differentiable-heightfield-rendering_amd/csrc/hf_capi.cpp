// hf_capi.cpp -- the C ABI of libhf (include/hf.h): handle management, argument
// validation, error strings.  All device work is in hf_kernels.hip.
#include <dlfcn.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <mutex>
#include <new>
#include <vector>

#include "hf_launch.h"

#define HF_NUM_SLOTS 64
struct hf_field {
    hf_dev_field dev;   // device view handed to kernels by value
    float *d_heights;   // owned copy of the heights
    float2 *d_mip;      // owned min/max pyramid
    float4 *d_shear;    // owned sheared bounds of the fine levels
    size_t mip_nodes;
    int device;
    uint32_t *d_misc;   // a few device words of the handle's own (the max of UniformAdam's second moments)
    hipEvent_t built;   // completion of the last hf_set_heights*
    // Ring of scratch blocks (the work counters of a launch), one slot per in-flight trace launch.  Every slot
    // carries the completion event of the launch that used it last: a launch that re-uses the slot first makes
    // its stream wait for that event (a device-side wait, normally long past), so two pending launches never
    // share a block, and hf_destroy waits for exactly the launches of this handle instead of the whole device.
    // Choice of the slot, launch and event record are ONE critical section (slot_lease below).
    // Blocks are allocated by hf_create (hf_trace_scratch_bytes is a constant today; a larger request re-allocates),
    // large enough for the slab of any transform-gradient launch too (hf_xform_slab_bytes(0): 240 KB), which also takes
    // its slab from this ring.
    // HIP-graph capture: a launch issued while its stream is being captured takes its block from the upper half of
    // the ring, touches no event, and keeps the block until hf_capture_reset (slot_lease).
    char *slot_buf[HF_NUM_SLOTS];
    size_t slot_cap[HF_NUM_SLOTS];
    hipEvent_t slot_done[HF_NUM_SLOTS];
    bool slot_used[HF_NUM_SLOTS];
    uint32_t next_slot, next_capture_slot;
    std::mutex *slot_mutex;
    int coherence;      // hf_set_ray_coherence: HF_COHERENCE_AUTO / _INCOHERENT (which instantiation the trace launches take)
    float4 *d_vn;       // smooth shading (hf_set_face_normals(hf, 0)): one vertex normal per texel, rebuilt with the
                        // heights and the transform; NULL = flat shading (the default), and the flat kernels run
    hf_area_table area; // area sampling (hf_set_area_sampling): the triangle-area CDF, rebuilt with the heights and the
                        // transform; area.cdf NULL = disabled (the default), and nothing of it is allocated or run
};

static bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void) hipGetLastError(); return false; }
    return st == hipStreamCaptureStatusActive;
}

// keeps the caller's current device across a call that has to work on the handle's device
struct hf_device_guard {
    int prev = -1;
    bool ok = true;
    explicit hf_device_guard(int dev) {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) cur = -1;
        if (cur != dev) {
            ok = hipSetDevice(dev) == hipSuccess;
            prev = cur;
        }
    }
    ~hf_device_guard() { if (prev >= 0) (void) hipSetDevice(prev); }
};

// Lease of one scratch block for ONE trace launch on `stream`.  The handle's slot mutex is held from the choice of
// the slot until the launch's completion event has been recorded (the destructor), so the three steps are one
// critical section: a later lease of the same slot -- from any thread, after the ring has wrapped -- always finds the
// event of the launch that used the block last and makes its stream wait for it (a device-side wait, normally long
// past).  The launch itself is asynchronous; the section costs microseconds.  (acquire / launch / record
// were three sections, and 32 other leases between a thread's acquire and its record could hand the block to a second
// launch that neither waited for the first nor kept its counters.)
// Captured launches (the stream is being captured into a HIP graph): the block comes from the upper half of the
// ring, no event is touched (an event recorded inside a capture cannot be waited for outside it), and every captured
// launch KEEPS its block for as long as the graph may be replayed: the 33rd captured trace launch of a handle is refused
// with HF_EINVAL instead of sharing work counters with the first; hf_capture_reset() returns the blocks once the
// graphs captured so far have been destroyed.
struct slot_lease {
    hf_field *m;
    hipStream_t stream;
    uint32_t slot = 0;
    void *buf = nullptr;
    const char *why = "scratch allocation failed";
    int code = HF_ENOMEM;
    std::unique_lock<std::mutex> lock;
    slot_lease(const hf_field *hf, hipStream_t st, size_t bytes)
        : m(const_cast<hf_field *>(hf)), stream(st), lock(*const_cast<hf_field *>(hf)->slot_mutex) {
        if (stream_capturing(stream)) { // no allocation, no events
            if (m->next_capture_slot >= HF_NUM_SLOTS / 2) {
                code = HF_EINVAL;
                why = "more than 32 captured trace launches on this handle (their scratch blocks stay reserved for "
                      "replays; destroy the graphs and call hf_capture_reset)";
                return;
            }
            slot = HF_NUM_SLOTS / 2 + m->next_capture_slot;
            if (m->slot_cap[slot] >= bytes) { buf = m->slot_buf[slot]; ++m->next_capture_slot; }
            return;
        }
        slot = m->next_slot++ % (HF_NUM_SLOTS / 2);
        if (m->slot_cap[slot] < bytes) { // grow: the previous user must be done before its block goes away
            if (m->slot_used[slot]) (void) hipEventSynchronize(m->slot_done[slot]);
            if (m->slot_buf[slot]) (void) hipFree(m->slot_buf[slot]);
            m->slot_buf[slot] = nullptr; m->slot_cap[slot] = 0;
            size_t cap = bytes < 65536 ? 65536 : bytes + bytes / 2;
            if (hipMalloc((void **) &m->slot_buf[slot], cap) != hipSuccess) return;
            m->slot_cap[slot] = cap;
        } else if (m->slot_used[slot]) {
            (void) hipStreamWaitEvent(stream, m->slot_done[slot], 0);
        }
        buf = m->slot_buf[slot];
    }
    ~slot_lease() {
        if (!buf || slot >= HF_NUM_SLOTS / 2) return; // nothing launched, or a captured launch
        (void) hipEventRecord(m->slot_done[slot], stream);
        m->slot_used[slot] = true;
    }
};

static thread_local char g_err[512] = "no error";

static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HF_HIP(call)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(e_ == hipErrorOutOfMemory ? HF_ENOMEM : HF_EDEVICE, "%s: %s", #call,     \
                        hipGetErrorString(e_));                                                   \
    } while (0)

// three row pointers, none of them NULL
static bool all3(const float *const p[3]) { return p && p[0] && p[1] && p[2]; }

extern "C" const char *hf_last_error_string(void) { return g_err; }
extern "C" int hf_version(void) { return HF_VERSION; }

// inverse of [A | t] = [A^-1 | -A^-1 t], adjugate formula in double
extern "C" int hf_invert_affine(const float in[12], float out[12]) {
    if (!in || !out) return fail(HF_EINVAL, "hf_invert_affine: NULL argument");
    double a[3][3], t[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) a[r][c] = in[4 * r + c];
        t[r] = in[4 * r + 3];
    }
    double c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1], c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2],
           c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0];
    double det = a[0][0] * c00 + a[0][1] * c01 + a[0][2] * c02;
    if (det == 0.0 || !isfinite(det)) return fail(HF_EINVAL, "hf_invert_affine: singular to_world");
    double inv[3][3];
    inv[0][0] = c00 / det;
    inv[0][1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) / det;
    inv[0][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / det;
    inv[1][0] = c01 / det;
    inv[1][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / det;
    inv[1][2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) / det;
    inv[2][0] = c02 / det;
    inv[2][1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) / det;
    inv[2][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / det;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out[4 * r + c] = (float) inv[r][c];
        out[4 * r + 3] = (float) -(inv[r][0] * t[0] + inv[r][1] * t[1] + inv[r][2] * t[2]);
    }
    return HF_OK;
}

static int set_transform(hf_field *hf, const float *to_world, const float *to_object) {
    memcpy(hf->dev.to_world, to_world, sizeof(float) * 12);
    if (to_object) {
        memcpy(hf->dev.to_object, to_object, sizeof(float) * 12);
        return HF_OK;
    }
    return hf_invert_affine(to_world, hf->dev.to_object);
}

static void free_area(hf_area_table &t) {
    void *bufs[5] = { t.cdf, t.coarse, t.tile, t.tile_valid, t.info };
    for (void *b : bufs)
        if (b) (void) hipFree(b);
    t = hf_area_table{};
}

// frees whatever a (possibly half-constructed) handle owns
static void release(hf_field *hf) {
    if (hf->built) (void) hipEventDestroy(hf->built);
    for (int k = 0; k < HF_NUM_SLOTS; ++k) {
        if (hf->slot_done[k]) (void) hipEventDestroy(hf->slot_done[k]);
        if (hf->slot_buf[k]) (void) hipFree(hf->slot_buf[k]);
    }
    if (hf->d_heights) (void) hipFree(hf->d_heights);
    if (hf->d_mip) (void) hipFree(hf->d_mip);
    if (hf->d_shear) (void) hipFree(hf->d_shear);
    if (hf->d_misc) (void) hipFree(hf->d_misc);
    if (hf->d_vn) (void) hipFree(hf->d_vn);
    free_area(hf->area);
    delete hf->slot_mutex;
    free(hf);
}

extern "C" int hf_create(const hf_desc_t *desc, hf_field_t **out) {
    if (!desc || !out) return fail(HF_EINVAL, "hf_create: NULL argument");
    *out = nullptr;
    if (desc->width < 2 || desc->height < 2)
        return fail(HF_EINVAL, "hf_create: heightfield resolution must be at least 2x2 (got %ux%u)", desc->width,
                    desc->height);
    if ((uint64_t) (desc->width - 1) * (desc->height - 1) >= (1ull << 31))
        return fail(HF_EINVAL, "hf_create: too many cells for a 32-bit prim_index");
    int ndev = 0;
    HF_HIP(hipGetDeviceCount(&ndev));
    if (desc->device < 0 || desc->device >= ndev)
        return fail(HF_EDEVICE, "hf_create: device %d not available (%d devices)", desc->device, ndev);
    hf_device_guard guard(desc->device); // the caller's current device is restored on return
    if (!guard.ok) return fail(HF_EDEVICE, "hf_create: cannot select device %d", desc->device);

    hf_field *hf = (hf_field *) calloc(1, sizeof(hf_field)); // zero-initialised POD
    if (!hf) return fail(HF_ENOMEM, "hf_create: host allocation failed");
    hf->device = desc->device;
    hf_dev_field &d = hf->dev;
    d.W = (int) desc->width; d.H = (int) desc->height;
    d.s = desc->max_height;
    d.sx = 2.0f / (float) (d.W - 1); d.sy = 2.0f / (float) (d.H - 1);
    d.iu = 1.0f / (float) (d.W - 1); d.iv = 1.0f / (float) (d.H - 1);
    d.hx = 0.5f * (float) (d.W - 1); d.hy = 0.5f * (float) (d.H - 1);
    d.flip = desc->flip_normals ? 1 : 0;
    int rc = set_transform(hf, desc->to_world, desc->has_to_object ? desc->to_object : nullptr);
    if (rc != HF_OK) { free(hf); return rc; }

    const int cw = d.W - 1, ch = d.H - 1;
    int top = 0;
    while ((1 << top) < cw || (1 << top) < ch) ++top;
    if (top < 1) top = 1;
    if (top > 15) { free(hf); return fail(HF_EINVAL, "hf_create: grid too large (more than 32768 cells per side)"); }
    if ((size_t) d.W * (size_t) d.H > ((size_t) 1 << 30)) { // the kernels address heights with 32-bit byte offsets
        free(hf);
        return fail(HF_EINVAL, "hf_create: grid too large (more than 2^30 vertices)");
    }
    d.top = top;
    const size_t off = hf_depth_off(top); // (4^top - 1)/3 nodes, depths 0..top-1
    hf->mip_nodes = off;
    hipError_t e = hipMalloc((void **) &hf->d_heights, sizeof(float) * (size_t) d.W * d.H);
    if (e == hipSuccess) e = hipMalloc((void **) &hf->d_mip, sizeof(float2) * off);
    if (e == hipSuccess) e = hipMalloc((void **) &hf->d_shear, sizeof(float4) * 3 * (hf_shear_records(top) + 1));
    if (e == hipSuccess) e = hipMalloc((void **) &hf->d_misc, 256);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&hf->built, hipEventDisableTiming);
    for (int k = 0; k < HF_NUM_SLOTS && e == hipSuccess; ++k) {
        e = hipEventCreateWithFlags(&hf->slot_done[k], hipEventDisableTiming);
        size_t cap = hf_trace_scratch_bytes(0) < 4096 ? 4096 : hf_trace_scratch_bytes(0);
        if (cap < hf_xform_slab_bytes(0)) cap = hf_xform_slab_bytes(0);
        if (e == hipSuccess) e = hipMalloc((void **) &hf->slot_buf[k], cap);
        if (e == hipSuccess) hf->slot_cap[k] = cap;
    }
    hf->coherence = HF_COHERENCE_AUTO;
    hf->slot_mutex = new (std::nothrow) std::mutex();
    if (e == hipSuccess && !hf->slot_mutex) e = hipErrorOutOfMemory;
    d.h = hf->d_heights;
    d.mip = hf->d_mip;
    d.shear = hf->d_shear;
    // heights start as zero; build the pyramid so the handle is always traceable
    if (e == hipSuccess) e = hipMemsetAsync(hf->d_heights, 0, sizeof(float) * (size_t) d.W * d.H, nullptr);
    if (e == hipSuccess) {
        hf_launch_build_mips(d, hf->d_mip, hf->d_shear, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(hf->built, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { // one exit for every failure after the first allocation: nothing leaks
        release(hf);
        return fail(e == hipErrorOutOfMemory ? HF_ENOMEM : HF_EDEVICE, "hf_create: %s", hipGetErrorString(e));
    }
    *out = hf;
    return HF_OK;
}

extern "C" int hf_destroy(hf_field_t *hf) {
    if (!hf) return HF_OK;
    hf_device_guard guard(hf->device);
    // wait for the work of THIS handle only (its last rebuild and the launches still holding a counter slot);
    // other streams of the host application keep running
    (void) hipEventSynchronize(hf->built);
    for (int k = 0; k < HF_NUM_SLOTS; ++k)
        if (hf->slot_used[k]) (void) hipEventSynchronize(hf->slot_done[k]);
    release(hf);
    return HF_OK;
}

extern "C" int hf_capture_reset(hf_field_t *hf) {
    if (!hf) return fail(HF_EINVAL, "hf_capture_reset: NULL handle");
    std::lock_guard<std::mutex> lock(*hf->slot_mutex);
    hf->next_capture_slot = 0;
    return HF_OK;
}

extern "C" int hf_set_heights(hf_field_t *hf, const float *d_heights, hf_stream_t stream) {
    if (!hf || !d_heights) return fail(HF_EINVAL, "hf_set_heights: NULL argument");
    hf_device_guard guard(hf->device);
    if (!guard.ok) return fail(HF_EDEVICE, "hf_set_heights: cannot select device %d", hf->device);
    hipStream_t st = (hipStream_t) stream;
    const size_t bytes = sizeof(float) * (size_t) hf->dev.W * hf->dev.H;
    if (d_heights != hf->d_heights)
        HF_HIP(hipMemcpyAsync(hf->d_heights, d_heights, bytes, hipMemcpyDeviceToDevice, st));
    hf_launch_build_mips(hf->dev, hf->d_mip, hf->d_shear, st);
    if (hf->d_vn) hf_launch_build_normals(hf->dev, hf->d_vn, st);
    if (hf->area.cdf) hf_launch_build_area(hf->dev, hf->area, st);
    HF_HIP(hipGetLastError());
    if (!stream_capturing(st)) HF_HIP(hipEventRecord(hf->built, st)); // (a captured rebuild is ordered by its graph)
    return HF_OK;
}

extern "C" int hf_adam_step(hf_field_t *hf, float *d_heights, const float *d_grad, float *d_m, float *d_v, double lr,
                            double beta1, double beta2, double eps, uint32_t step, int mask_updates,
                            hf_stream_t stream) {
    if (!hf || !d_heights || !d_grad || !d_m || !d_v) return fail(HF_EINVAL, "hf_adam_step: NULL argument");
    // optimizers.py:248-249
    if (!(beta1 >= 0. && beta1 < 1.) || !(beta2 >= 0. && beta2 < 1.) || !(lr > 0.) || !(eps > 0.) || step == 0)
        return fail(HF_EINVAL, "hf_adam_step: need 0 <= beta < 1, lr > 0, eps > 0, step >= 1");
    hf_device_guard guard(hf->device);
    if (!guard.ok) return fail(HF_EDEVICE, "hf_adam_step: cannot select device %d", hf->device);
    // lr_scale in double, rounded once, like the Python scalar the reference makes opaque (optimizers.py:267-268)
    const float lr_scale = (float) (sqrt(1.0 - pow(beta2, (double) step)) / (1.0 - pow(beta1, (double) step)));
    const float lr_t = (float) lr * lr_scale;
    // mask_updates: bit 0 = mask_updates, bit 1 = the 'uniform' variant (optimizers.py:259, 290-291)
    HF_HIP(hf_launch_adam((size_t) hf->dev.W * hf->dev.H, d_heights, d_grad, d_m, d_v, lr_t, (float) beta1, (float) beta2,
                          (float) (1.0 - beta1), (float) (1.0 - beta2), (float) eps, mask_updates & 1, (hipStream_t) stream,
                          (mask_updates & 2) ? hf->d_misc : nullptr));
    HF_HIP(hipGetLastError());
    return hf_set_heights(hf, d_heights, stream);
}

extern "C" float hf_adam_lr_t(double lr, double beta1, double beta2, uint32_t step) {
    // the arithmetic of hf_adam_step: lr_scale in double, rounded once, times the float learning rate
    const float lr_scale = (float) (sqrt(1.0 - pow(beta2, (double) step)) / (1.0 - pow(beta1, (double) step)));
    return (float) lr * lr_scale;
}

extern "C" int hf_adam_step_scheduled(hf_field_t *hf, float *d_heights, const float *d_grad, float *d_m, float *d_v,
                                      const float *d_lr_t, uint32_t *d_step, double beta1, double beta2, double eps,
                                      int mask_updates, hf_stream_t stream) {
    if (!hf || !d_heights || !d_grad || !d_m || !d_v || !d_lr_t || !d_step)
        return fail(HF_EINVAL, "hf_adam_step_scheduled: NULL argument");
    if (!(beta1 >= 0. && beta1 < 1.) || !(beta2 >= 0. && beta2 < 1.) || !(eps > 0.))
        return fail(HF_EINVAL, "hf_adam_step_scheduled: need 0 <= beta < 1, eps > 0");
    hf_device_guard guard(hf->device);
    if (!guard.ok) return fail(HF_EDEVICE, "hf_adam_step_scheduled: cannot select device %d", hf->device);
    HF_HIP(hf_launch_adam((size_t) hf->dev.W * hf->dev.H, d_heights, d_grad, d_m, d_v, 0.f, (float) beta1, (float) beta2,
                          (float) (1.0 - beta1), (float) (1.0 - beta2), (float) eps, mask_updates & 1, (hipStream_t) stream,
                          (mask_updates & 2) ? hf->d_misc : nullptr, d_lr_t, d_step));
    HF_HIP(hipGetLastError());
    return hf_set_heights(hf, d_heights, stream);
}

extern "C" int hf_set_heights_host(hf_field_t *hf, const float *h_heights, hf_stream_t stream) {
    if (!hf || !h_heights) return fail(HF_EINVAL, "hf_set_heights_host: NULL argument");
    hf_device_guard guard(hf->device);
    if (!guard.ok) return fail(HF_EDEVICE, "hf_set_heights_host: cannot select device %d", hf->device);
    hipStream_t st = (hipStream_t) stream;
    const size_t bytes = sizeof(float) * (size_t) hf->dev.W * hf->dev.H;
    HF_HIP(hipMemcpyAsync(hf->d_heights, h_heights, bytes, hipMemcpyHostToDevice, st));
    HF_HIP(hipStreamSynchronize(st)); // the host buffer may be reused by the caller
    return hf_set_heights(hf, hf->d_heights, stream);
}

extern "C" int hf_set_transform(hf_field_t *hf, const float to_world[12], const float *to_object_or_null) {
    if (!hf || !to_world) return fail(HF_EINVAL, "hf_set_transform: NULL argument");
    int rc = set_transform(hf, to_world, to_object_or_null);
    if (rc != HF_OK || (!hf->d_vn && !hf->area.cdf)) return rc;
    // Smooth shading: the vertex normals are world-space (angles are not affine-invariant) and are rebuilt here; so is
    // the area table (world-space areas).  The call takes no stream, so the rebuild is made synchronous: on the null stream after the last height update
    // (`built`, whatever stream that was on), and waited for before returning -- a query or a height update the caller
    // issues afterwards, on any stream, cannot overlap it.
    hf_device_guard guard(hf->device);
    if (!guard.ok) return fail(HF_EDEVICE, "hf_set_transform: cannot select device %d", hf->device);
    HF_HIP(hipStreamWaitEvent(nullptr, hf->built, 0));
    if (hf->d_vn) hf_launch_build_normals(hf->dev, hf->d_vn, nullptr);
    if (hf->area.cdf) hf_launch_build_area(hf->dev, hf->area, nullptr);
    HF_HIP(hipGetLastError());
    HF_HIP(hipEventRecord(hf->built, nullptr));
    HF_HIP(hipEventSynchronize(hf->built));
    return HF_OK;
}

extern "C" int hf_set_face_normals(hf_field_t *hf, int face_normals, hf_stream_t stream) {
    if (!hf) return fail(HF_EINVAL, "hf_set_face_normals: NULL handle");
    hf_device_guard guard(hf->device);
    if (!guard.ok) return fail(HF_EDEVICE, "hf_set_face_normals: cannot select device %d", hf->device);
    hipStream_t st = (hipStream_t) stream;
    // Not capturable: a captured switch would publish normals that no build has written before the first replay, and a
    // captured switch back would free a buffer the graph's kernels still reference.
    if (stream_capturing(st))
        return fail(HF_EINVAL, "hf_set_face_normals: not capturable (the stream is being captured into a HIP graph)");
    if (face_normals) { // flat: the buffer goes (hipFree waits for the work that may still read it)
        if (hf->d_vn) {
            float4 *vn = hf->d_vn;
            hf->d_vn = nullptr;
            HF_HIP(hipFree(vn));
        }
        return HF_OK;
    }
    if (hf->d_vn) return HF_OK;
    const size_t bytes = sizeof(float4) * (size_t) hf->dev.W * hf->dev.H;
    float4 *vn = nullptr;
    const hipError_t e = hipMalloc((void **) &vn, bytes);
    if (e != hipSuccess) {
        (void) hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? HF_ENOMEM : HF_EDEVICE,
                    "hf_set_face_normals: cannot allocate the vertex normals (%zu bytes): %s", bytes, hipGetErrorString(e));
    }
    // the build reads the heights the last hf_set_heights* left, whatever stream that was on
    HF_HIP(hipStreamWaitEvent(st, hf->built, 0));
    hf_launch_build_normals(hf->dev, vn, st);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) {
        (void) hipFree(vn);
        return fail(HF_EDEVICE, "hf_set_face_normals: %s", hipGetErrorString(le));
    }
    hf->d_vn = vn;
    HF_HIP(hipEventRecord(hf->built, st));
    return HF_OK;
}

extern "C" int hf_get_face_normals(const hf_field_t *hf) { return hf ? (hf->d_vn ? 0 : 1) : 1; }

static int check_device(const char *fn, const hf_field_t *hf);

extern "C" int hf_set_area_sampling(hf_field_t *hf, int enable, hf_stream_t stream) {
    if (!hf) return fail(HF_EINVAL, "hf_set_area_sampling: NULL handle");
    hf_device_guard guard(hf->device);
    if (!guard.ok) return fail(HF_EDEVICE, "hf_set_area_sampling: cannot select device %d", hf->device);
    hipStream_t st = (hipStream_t) stream;
    // Not capturable, for the reasons of hf_set_face_normals: a captured enable would publish a table no build has
    // written before the first replay, a captured disable would free buffers the graph's kernels still reference.
    if (stream_capturing(st))
        return fail(HF_EINVAL, "hf_set_area_sampling: not capturable (the stream is being captured into a HIP graph)");
    if (!enable) { // hipFree waits for the work that may still read the table
        free_area(hf->area);
        return HF_OK;
    }
    if (hf->area.cdf) return HF_OK;
    const uint32_t cw = (uint32_t) hf->dev.W - 1u, ch = (uint32_t) hf->dev.H - 1u;
    hf_area_table t = {};
    t.m = 2u * cw * ch;
    t.nseg = (t.m + HF_AREA_SEG - 1u) / HF_AREA_SEG;
    t.ncx = (cw + HF_AREA_CHUNK - 1u) / HF_AREA_CHUNK;
    t.ntiles = t.ncx * ch;
    const size_t n_cdf = (size_t) t.nseg * HF_AREA_SEG;
    hipError_t e = hipMalloc((void **) &t.cdf, sizeof(float) * n_cdf);
    if (e == hipSuccess) e = hipMalloc((void **) &t.coarse, sizeof(float) * t.nseg);
    if (e == hipSuccess) e = hipMalloc((void **) &t.tile, sizeof(double) * 3 * (size_t) t.ntiles);
    if (e == hipSuccess) e = hipMalloc((void **) &t.tile_valid, sizeof(uint32_t) * 2 * (size_t) t.ntiles);
    if (e == hipSuccess) e = hipMalloc((void **) &t.info, sizeof(hf_area_info));
    // the padding past the last entry is +inf: the segment count of hf_sample_position never counts it
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t) t.cdf, 0x7f800000, n_cdf, st);
    if (e == hipSuccess) e = hipStreamWaitEvent(st, hf->built, 0); // the heights of the last hf_set_heights*
    if (e == hipSuccess) {
        hf_launch_build_area(hf->dev, t, st);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        (void) hipGetLastError();
        (void) hipStreamSynchronize(st);
        free_area(t);
        return fail(e == hipErrorOutOfMemory ? HF_ENOMEM : HF_EDEVICE, "hf_set_area_sampling: cannot build the area table "
                    "(%u triangles): %s", t.m, hipGetErrorString(e));
    }
    hf->area = t;
    HF_HIP(hipEventRecord(hf->built, st));
    return HF_OK;
}

extern "C" int hf_surface_area(hf_field_t *hf, float *area, float *normalization) {
    if (!hf || !area) return fail(HF_EINVAL, "hf_surface_area: NULL argument");
    if (!hf->area.cdf) return fail(HF_EINVAL, "hf_surface_area: area sampling is not enabled (hf_set_area_sampling)");
    hf_device_guard guard(hf->device);
    if (!guard.ok) return fail(HF_EDEVICE, "hf_surface_area: cannot select device %d", hf->device);
    hf_area_info info;
    HF_HIP(hipEventSynchronize(hf->built));
    HF_HIP(hipMemcpy(&info, hf->area.info, sizeof(info), hipMemcpyDeviceToHost));
    *area = info.sum_f;
    if (normalization) *normalization = info.norm;
    return HF_OK;
}

extern "C" int hf_area_cdf(const hf_field_t *hf, const float **cdf, size_t *count) {
    if (!hf || !cdf || !count) return fail(HF_EINVAL, "hf_area_cdf: NULL argument");
    *cdf = hf->area.cdf;
    *count = hf->area.cdf ? hf->area.m : 0;
    return HF_OK;
}

extern "C" int hf_sample_position(const hf_field_t *hf, size_t n, const float *const sample[2], const uint8_t *active,
                                  const hf_position_sample_t *out, hf_stream_t stream) {
    if (!hf) return fail(HF_EINVAL, "hf_sample_position: NULL handle");
    if (!hf->area.cdf) return fail(HF_EINVAL, "hf_sample_position: area sampling is not enabled (hf_set_area_sampling)");
    if (!sample || !out) return fail(HF_EINVAL, "hf_sample_position: NULL argument");
    if (n == 0) return HF_OK;
    if (!sample[0] || !sample[1]) return fail(HF_EINVAL, "hf_sample_position: NULL sample array");
    if (!all3(out->p) || !all3(out->n) || !out->uv[0] || !out->uv[1] || !out->pdf)
        return fail(HF_EINVAL, "hf_sample_position: NULL output row (p, n, uv and pdf are required)");
    int rc;
    if ((rc = check_device("hf_sample_position", hf))) return rc;
    hf_launch_sample_position(hf->dev, hf->area, n, sample, active, *out, hf->d_vn, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

// the arguments both derivatives of hf_sample_position share
static int check_sample_diff(const char *fn, const hf_field_t *hf, size_t n, const uint32_t *prim, const float *const b[2]) {
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    if (n == 0) return HF_OK;
    if (!prim || !b || !b[0] || !b[1]) return fail(HF_EINVAL, "%s: NULL prim_index / b", fn);
    return check_device(fn, hf);
}

extern "C" int hf_sample_position_adjoint(const hf_field_t *hf, size_t n, const uint32_t *prim_index, const float *const b[2],
                                          const uint8_t *active, const float *const grad_p[3], const float *const grad_n[3],
                                          float *grad_heights, hf_stream_t stream) {
    int rc = check_sample_diff("hf_sample_position_adjoint", hf, n, prim_index, b);
    if (rc || n == 0) return rc;
    if (!grad_heights) return fail(HF_EINVAL, "hf_sample_position_adjoint: NULL grad_heights");
    if ((grad_p && !all3(grad_p)) || (grad_n && !all3(grad_n)))
        return fail(HF_EINVAL, "hf_sample_position_adjoint: NULL grad_p / grad_n array");
    hf_launch_sample_position_adjoint(hf->dev, n, prim_index, b, active, grad_p, grad_n, grad_heights, hf->d_vn,
                                      (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

// Replaces the reverse mode of sample_position through the reference's attached to_world: see include/hf.h
extern "C" int hf_sample_position_adjoint_transform(const hf_field_t *hf, size_t n, const uint32_t *prim_index,
                                                    const float *const b[2], const uint8_t *active,
                                                    const float *const grad_p[3], const float *const grad_n[3],
                                                    float *grad_heights, float *grad_to_world, hf_stream_t stream) {
    const char *fn = "hf_sample_position_adjoint_transform";
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    if (!grad_to_world) return hf_sample_position_adjoint(hf, n, prim_index, b, active, grad_p, grad_n, grad_heights, stream);
    int rc = check_sample_diff(fn, hf, n, prim_index, b);
    if (rc || n == 0) return rc;
    if ((grad_p && !all3(grad_p)) || (grad_n && !all3(grad_n))) return fail(HF_EINVAL, "%s: NULL grad_p / grad_n array", fn);
    {
        slot_lease lease(hf, (hipStream_t) stream, hf_xform_slab_bytes(n));
        if (!lease.buf) return fail(lease.code, "%s: %s", fn, lease.why);
        hf_launch_sample_position_adjoint(hf->dev, n, prim_index, b, active, grad_p, grad_n, grad_heights, hf->d_vn,
                                          (hipStream_t) stream, grad_to_world, lease.buf);
    }
    HF_HIP(hipGetLastError());
    return HF_OK;
}

// Replaces the forward mode of sample_position through the reference's attached to_world: see include/hf.h
extern "C" int hf_sample_position_tangent_transform(const hf_field_t *hf, size_t n, const uint32_t *prim_index,
                                                    const float *const b[2], const uint8_t *active, const float *dheights,
                                                    const float *d_to_world, float *const dp[3], float *const dn[3],
                                                    hf_stream_t stream) {
    const char *fn = "hf_sample_position_tangent_transform";
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    if (!d_to_world) return hf_sample_position_tangent(hf, n, prim_index, b, active, dheights, dp, dn, stream);
    int rc = check_sample_diff(fn, hf, n, prim_index, b);
    if (rc || n == 0) return rc;
    if ((dp && !all3(dp)) || (dn && !all3(dn))) return fail(HF_EINVAL, "%s: NULL dp / dn array", fn);
    hf_launch_sample_position_tangent(hf->dev, n, prim_index, b, active, dheights, dp, dn, hf->d_vn, (hipStream_t) stream,
                                      d_to_world);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_sample_position_tangent(const hf_field_t *hf, size_t n, const uint32_t *prim_index, const float *const b[2],
                                          const uint8_t *active, const float *dheights, float *const dp[3], float *const dn[3],
                                          hf_stream_t stream) {
    int rc = check_sample_diff("hf_sample_position_tangent", hf, n, prim_index, b);
    if (rc || n == 0) return rc;
    if ((dp && !all3(dp)) || (dn && !all3(dn))) return fail(HF_EINVAL, "hf_sample_position_tangent: NULL dp / dn array");
    hf_launch_sample_position_tangent(hf->dev, n, prim_index, b, active, dheights, dp, dn, hf->d_vn, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

// ---- shape attributes: what the three entry points share ----
static bool all_rows(const float *const *r, uint32_t size) {
    if (!r) return false;
    for (uint32_t c = 0; c < size; ++c)
        if (!r[c]) return false;
    return true;
}
static int attr_args(const char *fn, const hf_field_t *hf, size_t n, int type, uint32_t size, const float *attr,
                     const uint32_t *prim_index, const float *const p[3], const float *t, const uint8_t *active,
                     hf_attr_args &a) {
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    if (type != HF_ATTR_VERTEX && type != HF_ATTR_FACE) return fail(HF_EINVAL, "%s: bad attribute type %d", fn, type);
    if (size != 1 && size != 3) return fail(HF_EINVAL, "%s: attribute size %u (1 or 3)", fn, size);
    if (!attr || !prim_index) return fail(HF_EINVAL, "%s: NULL attr / prim_index", fn);
    if (type == HF_ATTR_VERTEX && !all3(p)) return fail(HF_EINVAL, "%s: NULL p (vertex attributes read si.p)", fn);
    a = hf_attr_args{};
    a.f = hf->dev; a.n = n; a.attr = attr; a.prim = prim_index; a.t = t; a.active = active;
    if (type == HF_ATTR_VERTEX)
        for (int c = 0; c < 3; ++c) a.p[c] = p[c];
    return n ? check_device(fn, hf) : HF_OK;
}

extern "C" int hf_eval_attribute(const hf_field_t *hf, size_t n, int type, uint32_t size, const float *attr,
                                 const uint32_t *prim_index, const float *const p[3], const float *t,
                                 const uint8_t *active, float *const out[], hf_stream_t stream) {
    hf_attr_args a;
    int rc = attr_args("hf_eval_attribute", hf, n, type, size, attr, prim_index, p, t, active, a);
    if (rc) return rc;
    if (!all_rows(out, size)) return fail(HF_EINVAL, "hf_eval_attribute: NULL output row");
    for (uint32_t c = 0; c < size; ++c) a.out[c] = out[c];
    hf_launch_attribute(0, type, size, a, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_eval_attribute_adjoint(const hf_field_t *hf, size_t n, int type, uint32_t size, const float *attr,
                                         const uint32_t *prim_index, const float *const p[3], const float *t,
                                         const uint8_t *active, const float *const grad_out[], float *grad_attr,
                                         float *const grad_p[3], float *grad_heights, hf_stream_t stream) {
    hf_attr_args a;
    int rc = attr_args("hf_eval_attribute_adjoint", hf, n, type, size, attr, prim_index, p, t, active, a);
    if (rc) return rc;
    if (!all_rows(grad_out, size)) return fail(HF_EINVAL, "hf_eval_attribute_adjoint: NULL grad_out row");
    if (grad_p && !all3(grad_p)) return fail(HF_EINVAL, "hf_eval_attribute_adjoint: NULL grad_p array");
    for (uint32_t c = 0; c < size; ++c) a.g[c] = grad_out[c];
    a.grad_attr = grad_attr;
    if (grad_p)
        for (int c = 0; c < 3; ++c) a.grad_p[c] = grad_p[c];
    a.grad_h = type == HF_ATTR_VERTEX ? grad_heights : nullptr; // (face attributes carry no geometric derivative)
    if (!a.grad_attr && !a.grad_p[0] && !a.grad_h) return HF_OK;
    hf_launch_attribute(1, type, size, a, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_eval_attribute_tangent(const hf_field_t *hf, size_t n, int type, uint32_t size, const float *attr,
                                         const uint32_t *prim_index, const float *const p[3], const float *t,
                                         const uint8_t *active, const float *dattr, const float *const dp[3],
                                         const float *dheights, float *const dout[], hf_stream_t stream) {
    hf_attr_args a;
    int rc = attr_args("hf_eval_attribute_tangent", hf, n, type, size, attr, prim_index, p, t, active, a);
    if (rc) return rc;
    if (!all_rows(dout, size)) return fail(HF_EINVAL, "hf_eval_attribute_tangent: NULL dout row");
    if (dp && !all3(dp)) return fail(HF_EINVAL, "hf_eval_attribute_tangent: NULL dp array");
    for (uint32_t c = 0; c < size; ++c) a.dout[c] = dout[c];
    a.dattr = dattr;
    if (dp && type == HF_ATTR_VERTEX)
        for (int c = 0; c < 3; ++c) a.dp[c] = dp[c];
    a.dh = dheights;
    hf_launch_attribute(2, type, size, a, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_heights_device(hf_field_t *hf, const float **out) {
    if (!hf || !out) return fail(HF_EINVAL, "hf_heights_device: NULL argument");
    *out = hf->d_heights;
    return HF_OK;
}

extern "C" int hf_dims(const hf_field_t *hf, uint32_t *width, uint32_t *height) {
    if (!hf) return fail(HF_EINVAL, "hf_dims: NULL argument");
    if (width) *width = (uint32_t) hf->dev.W;
    if (height) *height = (uint32_t) hf->dev.H;
    return HF_OK;
}

extern "C" int hf_num_levels(const hf_field_t *hf) { return hf ? hf->dev.top : 0; }

extern "C" int hf_get_mip(const hf_field_t *hf, int level, float *h_out, uint32_t *w, uint32_t *h) {
    if (!hf || level < 1 || level > hf->dev.top) return fail(HF_EINVAL, "hf_get_mip: bad level %d", level);
    const int cw = hf->dev.W - 1, ch = hf->dev.H - 1, k = hf->dev.top - level;
    const int wl = hf_level_w(cw, level), hl = hf_level_w(ch, level);
    if (w) *w = (uint32_t) wl;
    if (h) *h = (uint32_t) hl;
    if (h_out) { // existing nodes of the padded level, row-major (min,max) pairs
        hf_device_guard guard(hf->device);
        std::vector<float> tmp(2 * ((size_t) 1 << (2 * k)));
        HF_HIP(hipEventSynchronize(hf->built));
        HF_HIP(hipMemcpy(tmp.data(), hf->d_mip + hf_depth_off(k), sizeof(float) * tmp.size(), hipMemcpyDeviceToHost));
        for (int iy = 0; iy < hl; ++iy)
            for (int ix = 0; ix < wl; ++ix) {
                const size_t slot = ((size_t) iy << k) + ix;
                h_out[2 * ((size_t) iy * wl + ix) + 0] = tmp[2 * slot + 0];
                h_out[2 * ((size_t) iy * wl + ix) + 1] = tmp[2 * slot + 1];
            }
    }
    return HF_OK;
}

extern "C" int hf_get_node_level(const hf_field_t *hf, int level, float *h_records, float *h_minmax, uint32_t *side) {
    if (!hf || level < 1 || level > hf->dev.top) return fail(HF_EINVAL, "hf_get_node_level: bad level %d", level);
    const int k = hf->dev.top - level;
    const size_t slots = (size_t) 1 << (2 * k); // the whole padded level, as stored
    if (side) *side = 1u << k;
    if (h_records || h_minmax) {
        hf_device_guard guard(hf->device);
        HF_HIP(hipEventSynchronize(hf->built));
        if (h_records)
            HF_HIP(hipMemcpy(h_records, hf->d_shear + (size_t) (hf_depth_off(k) - 1u) * 3, sizeof(float4) * 3 * slots,
                             hipMemcpyDeviceToHost));
        if (h_minmax)
            HF_HIP(hipMemcpy(h_minmax, hf->d_mip + hf_depth_off(k), sizeof(float2) * slots, hipMemcpyDeviceToHost));
    }
    return HF_OK;
}

// world-space box of the 8 corners of the object-space bound (analog: rectangle.cpp:114-124)
extern "C" int hf_bbox(hf_field_t *hf, float out[6]) {
    if (!hf || !out) return fail(HF_EINVAL, "hf_bbox: NULL argument");
    float zr[2];
    hf_device_guard guard(hf->device);
    HF_HIP(hipEventSynchronize(hf->built));
    HF_HIP(hipMemcpy(zr, hf->d_mip + 1, sizeof(zr), hipMemcpyDeviceToHost));
    const hf_dev_field &d = hf->dev;
    const float lo[3] = { fmaf(0.f, d.sx, -1.f), fmaf(0.f, d.sy, -1.f), zr[0] };
    const float hi[3] = { fmaf((float) (d.W - 1), d.sx, -1.f), fmaf((float) (d.H - 1), d.sy, -1.f), zr[1] };
    for (int k = 0; k < 3; ++k) { out[k] = INFINITY; out[3 + k] = -INFINITY; }
    const float *m = d.to_world;
    for (int c = 0; c < 8; ++c) {
        const float p[3] = { (c & 1) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 4) ? hi[2] : lo[2] };
        for (int k = 0; k < 3; ++k) {
            float acc = m[4 * k + 3];
            acc = fmaf(m[4 * k + 0], p[0], acc);
            acc = fmaf(m[4 * k + 1], p[1], acc);
            acc = fmaf(m[4 * k + 2], p[2], acc);
            out[k] = fminf(out[k], acc);
            out[3 + k] = fmaxf(out[3 + k], acc);
        }
    }
    return HF_OK;
}

// the launch goes to the calling thread's current device: it must be the handle's (the query functions do
// not switch devices behind the caller's back)
static int check_device(const char *fn, const hf_field_t *hf) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != hf->device)
        return fail(HF_EDEVICE, "%s: current HIP device is %d, the heightfield lives on device %d", fn, cur, hf->device);
    return HF_OK;
}

static int check_rays(const char *fn, const hf_field_t *hf, size_t n, const hf_rays_t *rays) {
    if (!hf || !rays) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (n == 0) return HF_OK;
    if (!all3(rays->o) || !all3(rays->d)) return fail(HF_EINVAL, "%s: NULL ray component array", fn);
    if (!rays->maxt) return fail(HF_EINVAL, "%s: NULL ray maxt array", fn);
    return check_device(fn, hf);
}

static int check_flags(const char *fn, uint32_t flags) {
    if ((flags & HF_RAY_DETACHSHAPE) && (flags & HF_RAY_FOLLOWSHAPE))
        return fail(HF_EFLAGS, "%s: Invalid combination of RayFlags: DetachShape | FollowShape", fn);
    return HF_OK;
}

static int check_pi(const char *fn, size_t n, const hf_pi_const_t *pi) {
    if (!pi) return fail(HF_EINVAL, "%s: NULL pi", fn);
    if (n && (!pi->t || !pi->prim_uv[0] || !pi->prim_uv[1] || !pi->prim_index))
        return fail(HF_EINVAL, "%s: NULL preliminary-intersection array", fn);
    return HF_OK;
}

// one trace launch on a leased scratch block; a lease that fails reports as "<who>: <why>"
static int trace(const char *who, int mode, const hf_field_t *hf, size_t n, const hf_rays_t *rays, const uint8_t *active,
                 const hf_pi_t *pi, uint8_t *hit, const hf_si_t *si, uint32_t flags, hipStream_t stream,
                 const hf_reparam_args *aux, bool lean) {
    {
        slot_lease lease(hf, stream, hf_trace_scratch_bytes(n));
        if (!lease.buf) return fail(lease.code, "%s: %s", who, lease.why);
        hf_launch_trace(mode, hf->dev, n, rays, active, pi, hit, si, flags, lease.buf, stream, aux, lean, hf->d_vn);
    }
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_ray_intersect_preliminary(const hf_field_t *hf, size_t n, const hf_rays_t *rays,
                                            const uint8_t *active, const hf_pi_t *out, hf_stream_t stream) {
    int rc = check_rays("hf_ray_intersect_preliminary", hf, n, rays);
    if (rc) return rc;
    if (!out || (n && !out->t)) return fail(HF_EINVAL, "hf_ray_intersect_preliminary: NULL output");
    return trace("trace launch", 0, hf, n, rays, active, out, nullptr, nullptr, 0, (hipStream_t) stream, nullptr,
                 hf->coherence == HF_COHERENCE_INCOHERENT);
}

extern "C" int hf_ray_test(const hf_field_t *hf, size_t n, const hf_rays_t *rays, const uint8_t *active,
                           uint8_t *out_hit, hf_stream_t stream) {
    int rc = check_rays("hf_ray_test", hf, n, rays);
    if (rc) return rc;
    if (n && !out_hit) return fail(HF_EINVAL, "hf_ray_test: NULL output");
    return trace("trace launch", 1, hf, n, rays, active, nullptr, out_hit, nullptr, 0, (hipStream_t) stream, nullptr,
                 hf->coherence == HF_COHERENCE_INCOHERENT);
}

extern "C" int hf_compute_surface_interaction(const hf_field_t *hf, size_t n, const hf_rays_t *rays,
                                              const hf_pi_const_t *pi, uint32_t ray_flags, const uint8_t *active,
                                              const hf_si_t *out, hf_stream_t stream) {
    int rc = check_rays("hf_compute_surface_interaction", hf, n, rays);
    if (rc) return rc;
    if ((rc = check_flags("hf_compute_surface_interaction", ray_flags))) return rc;
    if ((rc = check_pi("hf_compute_surface_interaction", n, pi))) return rc;
    if (!out) return fail(HF_EINVAL, "hf_compute_surface_interaction: NULL output");
    hf_launch_si(hf->dev, n, rays, pi, active, out, ray_flags, (hipStream_t) stream, hf->d_vn);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_ray_intersect(const hf_field_t *hf, size_t n, const hf_rays_t *rays, uint32_t ray_flags,
                                const uint8_t *active, const hf_pi_t *out_pi, const hf_si_t *out_si,
                                hf_stream_t stream) {
    int rc = check_rays("hf_ray_intersect", hf, n, rays);
    if (rc) return rc;
    if ((rc = check_flags("hf_ray_intersect", ray_flags))) return rc;
    if (!out_si) return fail(HF_EINVAL, "hf_ray_intersect: NULL output");
    return trace("trace launch", 2, hf, n, rays, active, out_pi, nullptr, out_si, ray_flags, (hipStream_t) stream, nullptr,
                 hf->coherence == HF_COHERENCE_INCOHERENT);
}

extern "C" int hf_adjoint_rows(const hf_field_t *hf, size_t n, const hf_rays_t *rays, const hf_pi_const_t *pi,
                               uint32_t ray_flags, const uint8_t *active, const hf_si_grad_t *grad_si,
                               float *grad_heights, float *const grad_o[3], float *const grad_d[3],
                               uint32_t *row_band, hf_stream_t stream) {
    int rc = check_rays("hf_adjoint", hf, n, rays);
    if (rc) return rc;
    if ((rc = check_flags("hf_adjoint", ray_flags))) return rc;
    if ((rc = check_pi("hf_adjoint", n, pi))) return rc;
    if (!grad_si) return fail(HF_EINVAL, "hf_adjoint: NULL grad_si");
    if (grad_o && !all3(grad_o)) return fail(HF_EINVAL, "hf_adjoint: NULL grad_o array");
    if (grad_d && !all3(grad_d)) return fail(HF_EINVAL, "hf_adjoint: NULL grad_d array");
    hf_launch_adjoint(hf->dev, n, rays, pi, active, grad_si, ray_flags, grad_heights, grad_o, grad_d, row_band,
                      (hipStream_t) stream, hf->d_vn);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_adjoint(const hf_field_t *hf, size_t n, const hf_rays_t *rays, const hf_pi_const_t *pi,
                          uint32_t ray_flags, const uint8_t *active, const hf_si_grad_t *grad_si,
                          float *grad_heights, float *const grad_o[3], float *const grad_d[3],
                          hf_stream_t stream) {
    return hf_adjoint_rows(hf, n, rays, pi, ray_flags, active, grad_si, grad_heights, grad_o, grad_d, nullptr, stream);
}

extern "C" int hf_tangent(const hf_field_t *hf, size_t n, const hf_rays_t *rays, const hf_pi_const_t *pi,
                          uint32_t ray_flags, const uint8_t *active, const float *dheights, const float *const d_o[3],
                          const float *const d_d[3], const hf_si_tangent_t *tangent_si, hf_stream_t stream) {
    int rc = check_rays("hf_tangent", hf, n, rays);
    if (rc) return rc;
    if ((rc = check_flags("hf_tangent", ray_flags))) return rc;
    if ((rc = check_pi("hf_tangent", n, pi))) return rc;
    if (!tangent_si) return fail(HF_EINVAL, "hf_tangent: NULL output");
    hf_launch_tangent(hf->dev, n, rays, pi, active, ray_flags, dheights, d_o, d_d, tangent_si, (hipStream_t) stream, hf->d_vn);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

// Replaces the reverse-mode pass through the reference's attached to_world (rectangle.cpp:128, 255-310): see include/hf.h
extern "C" int hf_adjoint_transform(const hf_field_t *hf, size_t n, const hf_rays_t *rays, const hf_pi_const_t *pi,
                                    uint32_t ray_flags, const uint8_t *active, const hf_si_grad_t *grad_si,
                                    float *grad_heights, float *const grad_o[3], float *const grad_d[3],
                                    uint32_t *row_band, float *grad_to_world, hf_stream_t stream) {
    const char *fn = "hf_adjoint_transform";
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    if (!grad_to_world)
        return hf_adjoint_rows(hf, n, rays, pi, ray_flags, active, grad_si, grad_heights, grad_o, grad_d, row_band, stream);
    int rc = check_rays(fn, hf, n, rays);
    if (rc) return rc;
    if ((rc = check_flags(fn, ray_flags))) return rc;
    if ((rc = check_pi(fn, n, pi))) return rc;
    if (!grad_si) return fail(HF_EINVAL, "%s: NULL grad_si", fn);
    if (grad_o && !all3(grad_o)) return fail(HF_EINVAL, "%s: NULL grad_o array", fn);
    if (grad_d && !all3(grad_d)) return fail(HF_EINVAL, "%s: NULL grad_d array", fn);
    if (n == 0) return HF_OK;
    {
        slot_lease lease(hf, (hipStream_t) stream, hf_xform_slab_bytes(n)); // the slab: this launch's alone
        if (!lease.buf) return fail(lease.code, "%s: %s", fn, lease.why);
        hf_launch_adjoint(hf->dev, n, rays, pi, active, grad_si, ray_flags, grad_heights, grad_o, grad_d, row_band,
                          (hipStream_t) stream, hf->d_vn, grad_to_world, lease.buf);
    }
    HF_HIP(hipGetLastError());
    return HF_OK;
}

// Replaces the forward-mode pass through the reference's attached to_world (rectangle.cpp:255-310): see include/hf.h
extern "C" int hf_tangent_transform(const hf_field_t *hf, size_t n, const hf_rays_t *rays, const hf_pi_const_t *pi,
                                    uint32_t ray_flags, const uint8_t *active, const float *dheights,
                                    const float *const d_o[3], const float *const d_d[3], const float *d_to_world,
                                    const hf_si_tangent_t *tangent_si, hf_stream_t stream) {
    const char *fn = "hf_tangent_transform";
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    if (!d_to_world) return hf_tangent(hf, n, rays, pi, ray_flags, active, dheights, d_o, d_d, tangent_si, stream);
    int rc = check_rays(fn, hf, n, rays);
    if (rc) return rc;
    if ((rc = check_flags(fn, ray_flags))) return rc;
    if ((rc = check_pi(fn, n, pi))) return rc;
    if (!tangent_si) return fail(HF_EINVAL, "%s: NULL output", fn);
    hf_launch_tangent(hf->dev, n, rays, pi, active, ray_flags, dheights, d_o, d_d, tangent_si, (hipStream_t) stream,
                      hf->d_vn, d_to_world);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_shading_derivatives(const hf_field_t *hf, size_t n, const hf_pi_const_t *pi, const uint8_t *active,
                                      float *const dn_du[3], float *const dn_dv[3], hf_stream_t stream) {
    if (!hf) return fail(HF_EINVAL, "hf_shading_derivatives: NULL handle");
    int rc;
    if ((rc = check_pi("hf_shading_derivatives", n, pi))) return rc;
    if ((dn_du && !all3(dn_du)) || (dn_dv && !all3(dn_dv)))
        return fail(HF_EINVAL, "hf_shading_derivatives: NULL dn_du / dn_dv array");
    if (n == 0) return HF_OK;
    if ((rc = check_device("hf_shading_derivatives", hf))) return rc;
    hf_launch_shading_derivatives(hf->dev, n, pi, active, dn_du, dn_dv, hf->d_vn, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

// ---- eval_parameterization: the surface interaction at texture coordinates ----------------------------------------
// what the three entry points share: the handle, the flags (as hf_compute_surface_interaction), the uv rows, the device
static int check_param(const char *fn, const hf_field_t *hf, size_t n, const float *const uv[2], uint32_t ray_flags) {
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    int rc;
    if ((rc = check_flags(fn, ray_flags))) return rc;
    if (n == 0) return HF_OK;
    if (!uv || !uv[0] || !uv[1]) return fail(HF_EINVAL, "%s: NULL uv array", fn);
    return check_device(fn, hf);
}

// Replaces: Shape::eval_parameterization (include/mitsuba/render/shape.h:361) as Mesh implements it (src/render/mesh.cpp
// 503-545 build_parameterization, 614-635) and Rectangle (src/shapes/rectangle.cpp:173-192); called by the area emitter
// (src/emitters/area.cpp:136, 173, 211).  See include/hf.h.
extern "C" int hf_eval_parameterization(const hf_field_t *hf, size_t n, const float *const uv[2], uint32_t ray_flags,
                                        const uint8_t *active, const hf_si_t *out, uint32_t *out_prim_index,
                                        hf_stream_t stream) {
    const char *fn = "hf_eval_parameterization";
    int rc = check_param(fn, hf, n, uv, ray_flags);
    if (rc) return rc;
    if (!out) return fail(HF_EINVAL, "%s: NULL output", fn);
    if (n == 0) return HF_OK;
    // t stays the UV-space ray's 1 (FollowShape's |p - o| would measure from a UV-space point); boundary_test is the
    // ray-independent all-edge SDF (there is no viewing ray for the silhouette form)
    uint32_t flags = ray_flags & ~(uint32_t) HF_RAY_FOLLOWSHAPE;
    if (flags & HF_RAY_BOUNDARYTEST) flags |= HF_RAY_BOUNDARY_ALL_EDGES;
    hf_launch_param(hf->dev, n, uv, active, out, out_prim_index, flags, (hipStream_t) stream, hf->d_vn);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

// Replaces: the reverse mode of Mesh::eval_parameterization (mesh.cpp:614-635) with the barycentrics frozen (the
// FollowShape derivative with t held constant).  See include/hf.h.
extern "C" int hf_eval_parameterization_adjoint(const hf_field_t *hf, size_t n, const float *const uv[2],
                                                uint32_t ray_flags, const uint8_t *active, const hf_si_grad_t *grad_si,
                                                float *grad_heights, float *grad_to_world, hf_stream_t stream) {
    const char *fn = "hf_eval_parameterization_adjoint";
    int rc = check_param(fn, hf, n, uv, ray_flags);
    if (rc) return rc;
    if (!grad_si) return fail(HF_EINVAL, "%s: NULL grad_si", fn);
    if (n == 0) return HF_OK;
    hf_si_grad_t g = *grad_si;
    g.t = nullptr; g.uv[0] = g.uv[1] = nullptr; // t and uv are not differentiated
    const uint32_t flags = ray_flags | HF_RAY_FOLLOWSHAPE;
    if (!grad_to_world) {
        hf_launch_param_adjoint(hf->dev, n, uv, active, &g, flags, grad_heights, (hipStream_t) stream, hf->d_vn);
    } else {
        slot_lease lease(hf, (hipStream_t) stream, hf_xform_slab_bytes(n)); // the slab: this launch's alone
        if (!lease.buf) return fail(lease.code, "%s: %s", fn, lease.why);
        hf_launch_param_adjoint(hf->dev, n, uv, active, &g, flags, grad_heights, (hipStream_t) stream, hf->d_vn,
                                grad_to_world, lease.buf);
    }
    HF_HIP(hipGetLastError());
    return HF_OK;
}

// Replaces: the forward mode of the same (mesh.cpp:614-635, frozen barycentrics).  See include/hf.h.
extern "C" int hf_eval_parameterization_tangent(const hf_field_t *hf, size_t n, const float *const uv[2],
                                                uint32_t ray_flags, const uint8_t *active, const float *dheights,
                                                const float *d_to_world, const hf_si_tangent_t *tangent_si,
                                                hf_stream_t stream) {
    const char *fn = "hf_eval_parameterization_tangent";
    int rc = check_param(fn, hf, n, uv, ray_flags);
    if (rc) return rc;
    if (!tangent_si) return fail(HF_EINVAL, "%s: NULL output", fn);
    if (n == 0) return HF_OK;
    hf_launch_param_tangent(hf->dev, n, uv, active, ray_flags | HF_RAY_FOLLOWSHAPE, dheights, d_to_world, tangent_si,
                            (hipStream_t) stream, hf->d_vn);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

// ---- minimal direct lighting --------------------------------------------------
static int pack_lights(const char *who, size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                       const float *t, uint32_t n_lights, const hf_dir_light_t *lights, float albedo,
                       const uint8_t *const *vis, hf_lights_dev &L) {
    if (!sh_n || !d || !t || !lights) return fail(HF_EINVAL, "%s: NULL argument", who);
    for (int k = 0; k < 3; ++k)
        if (!sh_n[k] || !d[k]) return fail(HF_EINVAL, "%s: NULL component array", who);
    if (spp == 0 || n % spp != 0) return fail(HF_EINVAL, "%s: n (%zu) must be a multiple of spp (%u)", who, n, spp);
    if (n_lights == 0 || n_lights > HF_MAX_LIGHTS)
        return fail(HF_EINVAL, "%s: 1..%d lights supported (got %u)", who, HF_MAX_LIGHTS, n_lights);
    if ((size_t) (n / spp) * n_lights >= ((size_t) 1 << 32)) return fail(HF_EINVAL, "%s: image too large", who);
    L.n = n_lights;
    L.weight = nullptr; L.grad_weight = nullptr;
    for (uint32_t k = 0; k < HF_MAX_LIGHTS; ++k) {
        const bool on = k < n_lights;
        for (int c = 0; c < 3; ++c) L.l[k][c] = on ? lights[k].to_light[c] : 0.f;
        L.w[k] = on ? (albedo * 0.31830988618379067154f) * lights[k].irradiance : 0.f; // dr::InvPi
        L.vis[k] = (on && vis) ? vis[k] : nullptr;
    }
    return HF_OK;
}

// One body per direction of the lighting family.  point: point lights at p (hf_point_light_t has hf_dir_light_t's
// layout: three floats + one), else directional lights and p == NULL.
static int lighting(const char *who, bool point, size_t n, uint32_t spp, const float *const sh_n[3],
                    const float *const d[3], const float *t, const float *weight, const float *const p[3],
                    uint32_t n_lights, const hf_dir_light_t *lights, float albedo, const uint8_t *const *vis,
                    float *image, hipStream_t stream) {
    hf_lights_dev L;
    const int rc = pack_lights(who, n, spp, sh_n, d, t, n_lights, lights, albedo, vis, L);
    if (rc != HF_OK) return rc;
    if (point && !all3(p)) return fail(HF_EINVAL, "%s: NULL position array", who);
    if (!image) return fail(HF_EINVAL, "%s: NULL image", who);
    L.weight = weight;
    hf_launch_direct(n, spp, sh_n, d, t, p, L, image, stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

static int lighting_adjoint(const char *who, bool point, size_t n, uint32_t spp, const float *const sh_n[3],
                            const float *const d[3], const float *t, const float *weight, const float *const p[3],
                            uint32_t n_lights, const hf_dir_light_t *lights, float albedo, const uint8_t *const *vis,
                            const float *grad_image, float *const grad_sh_n[3], float *grad_weight,
                            float *const grad_p[3], hipStream_t stream) {
    hf_lights_dev L;
    const int rc = pack_lights(who, n, spp, sh_n, d, t, n_lights, lights, albedo, vis, L);
    if (rc != HF_OK) return rc;
    if (point && !all3(p)) return fail(HF_EINVAL, "%s: NULL position array", who);
    if (!grad_image || !all3(grad_sh_n) || (point && !all3(grad_p))) return fail(HF_EINVAL, "%s: NULL gradient array", who);
    L.weight = weight; L.grad_weight = grad_weight;
    hf_launch_direct_adjoint(n, spp, sh_n, d, t, p, L, grad_image, grad_sh_n, grad_p, stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

static int lighting_tangent(const char *who, bool point, size_t n, uint32_t spp, const float *const sh_n[3],
                            const float *const d[3], const float *t, const float *weight, const float *const p[3],
                            uint32_t n_lights, const hf_dir_light_t *lights, float albedo, const uint8_t *const *vis,
                            const float *const dsh_n[3], const float *const dp[3], const float *dweight, float *dimage,
                            hipStream_t stream) {
    hf_lights_dev L;
    const int rc = pack_lights(who, n, spp, sh_n, d, t, n_lights, lights, albedo, vis, L);
    if (rc != HF_OK) return rc;
    if (point && !all3(p)) return fail(HF_EINVAL, "%s: NULL position array", who);
    if (!dimage) return fail(HF_EINVAL, "%s: NULL image", who);
    if ((dsh_n && !all3(dsh_n)) || (dp && !all3(dp)))
        return fail(HF_EINVAL, "%s: NULL %s component array", who, point ? "tangent" : "dsh_n");
    L.weight = weight;
    hf_launch_direct_tangent(n, spp, sh_n, d, t, p, L, dsh_n, dp, dweight, dimage, stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}
static_assert(sizeof(hf_point_light_t) == sizeof(hf_dir_light_t), "light structs share one packing");

extern "C" int hf_direct_lighting_weighted(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                           const float *t, const float *weight, uint32_t n_lights,
                                           const hf_dir_light_t *lights, float albedo, const uint8_t *const *vis,
                                           float *image, hf_stream_t stream) {
    return lighting("hf_direct_lighting", false, n, spp, sh_n, d, t, weight, nullptr, n_lights, lights, albedo, vis, image,
                    (hipStream_t) stream);
}
extern "C" int hf_direct_lighting(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                  const float *t, uint32_t n_lights, const hf_dir_light_t *lights, float albedo,
                                  const uint8_t *const *vis, float *image, hf_stream_t stream) {
    return hf_direct_lighting_weighted(n, spp, sh_n, d, t, nullptr, n_lights, lights, albedo, vis, image, stream);
}
extern "C" int hf_direct_lighting_weighted_adjoint(size_t n, uint32_t spp, const float *const sh_n[3],
                                                   const float *const d[3], const float *t, const float *weight,
                                                   uint32_t n_lights, const hf_dir_light_t *lights, float albedo,
                                                   const uint8_t *const *vis, const float *grad_image,
                                                   float *const grad_sh_n[3], float *grad_weight, hf_stream_t stream) {
    return lighting_adjoint("hf_direct_lighting_adjoint", false, n, spp, sh_n, d, t, weight, nullptr, n_lights, lights,
                            albedo, vis, grad_image, grad_sh_n, grad_weight, nullptr, (hipStream_t) stream);
}
extern "C" int hf_direct_lighting_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                          const float *t, uint32_t n_lights, const hf_dir_light_t *lights,
                                          float albedo, const uint8_t *const *vis, const float *grad_image,
                                          float *const grad_sh_n[3], hf_stream_t stream) {
    return hf_direct_lighting_weighted_adjoint(n, spp, sh_n, d, t, nullptr, n_lights, lights, albedo, vis, grad_image,
                                               grad_sh_n, nullptr, stream);
}
extern "C" int hf_direct_lighting_weighted_tangent(size_t n, uint32_t spp, const float *const sh_n[3],
                                                   const float *const d[3], const float *t, const float *weight,
                                                   uint32_t n_lights, const hf_dir_light_t *lights, float albedo,
                                                   const uint8_t *const *vis, const float *const dsh_n[3],
                                                   const float *dweight, float *dimage, hf_stream_t stream) {
    return lighting_tangent("hf_direct_lighting_weighted_tangent", false, n, spp, sh_n, d, t, weight, nullptr, n_lights,
                            lights, albedo, vis, dsh_n, nullptr, dweight, dimage, (hipStream_t) stream);
}

extern "C" int hf_point_lighting(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                 const float *t, const float *const p[3], uint32_t n_lights,
                                 const hf_point_light_t *lights, float albedo, const uint8_t *const *vis, float *image,
                                 hf_stream_t stream) {
    return lighting("hf_point_lighting", true, n, spp, sh_n, d, t, nullptr, p, n_lights, (const hf_dir_light_t *) lights,
                    albedo, vis, image, (hipStream_t) stream);
}
extern "C" int hf_point_lighting_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                         const float *t, const float *const p[3], uint32_t n_lights,
                                         const hf_point_light_t *lights, float albedo, const uint8_t *const *vis,
                                         const float *grad_image, float *const grad_sh_n[3], float *const grad_p[3],
                                         hf_stream_t stream) {
    return lighting_adjoint("hf_point_lighting_adjoint", true, n, spp, sh_n, d, t, nullptr, p, n_lights,
                            (const hf_dir_light_t *) lights, albedo, vis, grad_image, grad_sh_n, nullptr, grad_p,
                            (hipStream_t) stream);
}
extern "C" int hf_point_lighting_tangent(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                         const float *t, const float *const p[3], uint32_t n_lights,
                                         const hf_point_light_t *lights, float albedo, const uint8_t *const *vis,
                                         const float *const dsh_n[3], const float *const dp[3], float *dimage,
                                         hf_stream_t stream) {
    return lighting_tangent("hf_point_lighting_tangent", true, n, spp, sh_n, d, t, nullptr, p, n_lights,
                            (const hf_dir_light_t *) lights, albedo, vis, dsh_n, dp, nullptr, dimage, (hipStream_t) stream);
}

// ---- lighting rows, shared: what the sky, envmap, reflect, glossy and bounce entries below check and fill alike (A: the
// row's argument block, zeroed by the caller).  All checks come before anything touches a device. ----
// the wavefront and the sample count; `dirs`: the row's word for its directions, other_null: a row's further pointers
template <class A>
static int light_args(const char *who, const char *dirs, size_t n, uint32_t spp, const float *const sh_n[3],
                      const float *const d[3], const float *t, const float *weight, uint32_t num_rays, uint32_t seed,
                      const uint32_t *ray_id, bool other_null, A &a) {
    if (!all3(sh_n) || !all3(d) || !t || other_null) return fail(HF_EINVAL, "%s: NULL argument", who);
    if (spp == 0 || n % spp != 0) return fail(HF_EINVAL, "%s: n (%zu) must be a multiple of spp (%u)", who, n, spp);
    if (num_rays == 0 || num_rays > 32) return fail(HF_EINVAL, "%s: 1..32 %s per sample (got %u)", who, dirs, num_rays);
    if (n >= ((size_t) 1 << 32)) return fail(HF_EINVAL, "%s: more than 2^32 samples", who);
    a.n = n; a.spp = spp; a.num_rays = num_rays; a.seed = seed; a.ray_id = ray_id; a.t = t; a.weight = weight;
    for (int c = 0; c < 3; ++c) { a.sh_n[c] = sh_n[c]; a.d[c] = d[c]; }
    return HF_OK;
}
// the outputs of a *_rays entry (and the two rows only it and the forward read)
template <class A>
static int light_rays_out(const char *who, const float *const p[3], const float *const nrm[3], float *const out_o[3],
                          float *const out_d[3], float *out_maxt, A &a) {
    if (!all3(p) || !all3(nrm) || !all3(out_o) || !all3(out_d) || !out_maxt) return fail(HF_EINVAL, "%s: NULL argument", who);
    a.out_maxt = out_maxt;
    for (int c = 0; c < 3; ++c) { a.p[c] = p[c]; a.nrm[c] = nrm[c]; a.out_o[c] = out_o[c]; a.out_d[c] = out_d[c]; }
    return HF_OK;
}
// of a forward entry (image_optional: a row that has other outputs)
template <class A>
static int light_forward_out(const char *who, const float *const p[3], const float *const nrm[3], float *image, A &a,
                             bool image_optional = false) {
    if (!all3(p) || !all3(nrm) || (!image && !image_optional)) return fail(HF_EINVAL, "%s: NULL argument", who);
    a.image = image;
    for (int c = 0; c < 3; ++c) { a.p[c] = p[c]; a.nrm[c] = nrm[c]; }
    return HF_OK;
}
// the tangents of sh_n and weight (NULL: zero) and the image of a tangent entry
template <class A>
static int light_tangent_io(const char *who, bool other_null, const float *const dsh_n[3], const float *dweight,
                            float *dimage, A &a, bool image_optional = false) {
    if (other_null || (!dimage && !image_optional)) return fail(HF_EINVAL, "%s: NULL argument", who);
    if (dsh_n && !all3(dsh_n)) return fail(HF_EINVAL, "%s: NULL dsh_n component array", who);
    a.image = dimage; a.dw = dweight;
    for (int c = 0; c < 3; ++c) a.dn[c] = dsh_n ? dsh_n[c] : nullptr;
    return HF_OK;
}
// The same for a row with a per-sample value beside its image (reflect, glossy).  The caller sets its visibility row
// (vis_null: it is missing; vis_name: what the row calls it).  Forward: image, value, visibility -- at least one
template <class A>
static int light_value_forward_out(const char *who, const float *const p[3], const float *const nrm[3], float *image,
                                   float *value, bool vis_null, const char *vis_name, A &a) {
    const int rc = light_forward_out(who, p, nrm, image, a, true);
    if (rc != HF_OK) return rc;
    if (!image && !value && vis_null) return fail(HF_EINVAL, "%s: image, value and %s are all NULL", who, vis_name);
    a.value = value;
    return HF_OK;
}
// adjoint: dL/dimage, dL/dvalue (NULL: zero); grad_sh_n (NULL, or rows of which any may be), weight, texels (NULL: not wanted)
template <class A>
static int light_value_adjoint_io(const char *who, bool vis_null, const float *grad_image, const float *grad_value,
                                  float *const grad_sh_n[3], float *grad_weight, float *grad_data, A &a) {
    if (vis_null) return fail(HF_EINVAL, "%s: NULL argument", who);
    if (grad_sh_n && !all3(grad_sh_n)) return fail(HF_EINVAL, "%s: NULL grad_sh_n component array", who);
    a.gimg = grad_image; a.gvalue = grad_value; a.gw = grad_weight; a.gdata = grad_data;
    for (int c = 0; c < 3; ++c) a.gn[c] = grad_sh_n ? grad_sh_n[c] : nullptr;
    return HF_OK;
}
// tangent: the tangents of sh_n, weight and the texels (NULL: zero); dimage, dvalue -- at least one
template <class A>
static int light_value_tangent_io(const char *who, bool vis_null, const float *const dsh_n[3], const float *dweight,
                                  const float *ddata, float *dimage, float *dvalue, A &a) {
    if (vis_null) return fail(HF_EINVAL, "%s: NULL argument", who);
    if (!dimage && !dvalue) return fail(HF_EINVAL, "%s: dimage and dvalue are both NULL", who);
    a.ddata = ddata; a.value = dvalue;
    return light_tangent_io(who, false, dsh_n, dweight, dimage, a, true);
}
// the interface of a reflection lobe: the relative index eta (0: F = 1, an ideal mirror), rcp_eta rounded once here
template <class A>
static int light_interface(const char *who, float eta, A &a) {
    if (!isfinite(eta) || eta < 0.f) return fail(HF_EINVAL, "%s: eta must be finite and not negative (got %g)", who, (double) eta);
    a.eta = eta; a.rcp_eta = eta > 0.f ? 1.f / eta : 0.f;
    return HF_OK;
}

// the launch of mode `mode` of a row, and what it reports
template <class A>
static int light_launch(void (*launch)(int, const A &, hipStream_t), int mode, const A &a, hf_stream_t stream) {
    launch(mode, a, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

// ---- sky lighting: constant environment, the shadow rays traced inside the lighting kernel ----
// What the four hf_sky_* entries share.  spp / num_rays / radiance / albedo: the film and the emitter of the three
// lighting entries (hf_sky_rays passes 1, k + 1, 1, 1: its k must name one of 32 directions).
static int sky_args(const char *who, size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                    const float *t, const float *weight, uint32_t num_rays, uint32_t seed, const uint32_t *ray_id,
                    float radiance, float albedo, hf_sky_args &a) {
    a = {};
    const int rc = light_args(who, "sky directions", n, spp, sh_n, d, t, weight, num_rays, seed, ray_id, false, a);
    if (rc != HF_OK) return rc;
    if (!isfinite(radiance) || !isfinite(albedo)) return fail(HF_EINVAL, "%s: radiance and albedo must be finite", who);
    a.scale = (4.f * albedo * radiance) / (float) num_rays; // albedo/pi * L / pdf, pdf = 1 / (4 pi), averaged over num_rays
    return HF_OK;
}

extern "C" int hf_sky_rays(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                           const float *const d[3], const float *t, uint32_t k, uint32_t seed, const uint32_t *ray_id,
                           float *const out_o[3], float *const out_d[3], float *out_maxt, hf_stream_t stream) {
    const char *fn = "hf_sky_rays";
    hf_sky_args a;
    if (k >= 32) return fail(HF_EINVAL, "%s: direction k must be below 32 (got %u)", fn, k);
    int rc = sky_args(fn, n, 1, sh_n, d, t, nullptr, k + 1, seed, ray_id, 1.f, 1.f, a);
    if (rc != HF_OK || (rc = light_rays_out(fn, p, nrm, out_o, out_d, out_maxt, a))) return rc;
    a.k = k;
    return light_launch(hf_launch_sky, 3, a, stream);
}

extern "C" int hf_sky_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3],
                               const float *const nrm[3], const float *const sh_n[3], const float *const d[3],
                               const float *t, const float *weight, uint32_t num_rays, uint32_t seed,
                               const uint32_t *ray_id, float radiance, float albedo, float *image, uint32_t *vis_bits,
                               hf_stream_t stream) {
    const char *fn = "hf_sky_lighting";
    hf_sky_args a;
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    int rc = sky_args(fn, n, spp, sh_n, d, t, weight, num_rays, seed, ray_id, radiance, albedo, a);
    if (rc != HF_OK || (rc = light_forward_out(fn, p, nrm, image, a))) return rc;
    if (n == 0) return HF_OK;
    if ((rc = check_device(fn, hf))) return rc;
    a.f = hf->dev; a.vis_bits = vis_bits;
    return light_launch(hf_launch_sky, 0, a, stream);
}

extern "C" int hf_sky_lighting_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                       const float *t, const float *weight, uint32_t num_rays, uint32_t seed,
                                       const uint32_t *ray_id, float radiance, float albedo, const uint32_t *vis_bits,
                                       const float *grad_image, float *const grad_sh_n[3], float *grad_weight,
                                       hf_stream_t stream) {
    const char *fn = "hf_sky_lighting_adjoint";
    hf_sky_args a;
    const int rc = sky_args(fn, n, spp, sh_n, d, t, weight, num_rays, seed, ray_id, radiance, albedo, a);
    if (rc != HF_OK) return rc;
    if (!vis_bits || !grad_image || !all3(grad_sh_n)) return fail(HF_EINVAL, "%s: NULL argument", fn);
    a.vis_bits = const_cast<uint32_t *>(vis_bits); a.gimg = grad_image; a.gw = grad_weight;
    for (int c = 0; c < 3; ++c) a.gn[c] = grad_sh_n[c];
    return light_launch(hf_launch_sky, 1, a, stream);
}

extern "C" int hf_sky_lighting_tangent(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                       const float *t, const float *weight, uint32_t num_rays, uint32_t seed,
                                       const uint32_t *ray_id, float radiance, float albedo, const uint32_t *vis_bits,
                                       const float *const dsh_n[3], const float *dweight, float *dimage,
                                       hf_stream_t stream) {
    const char *fn = "hf_sky_lighting_tangent";
    hf_sky_args a;
    int rc = sky_args(fn, n, spp, sh_n, d, t, weight, num_rays, seed, ray_id, radiance, albedo, a);
    if (rc != HF_OK || (rc = light_tangent_io(fn, !vis_bits, dsh_n, dweight, dimage, a))) return rc;
    a.vis_bits = const_cast<uint32_t *>(vis_bits);
    return light_launch(hf_launch_sky, 2, a, stream);
}

// ---- refractive caustics: light tracing through the surface, the refracted rays walked in the kernel ----
// What the hf_caustic_* entries and the refraction view (hf_refract_*) share, in the two pieces between which an entry
// checks what is its own (A: the row's argument block, zeroed by the caller): the wavefront rows and the interface ...
template <class A>
static int caustic_rows(const char *who, size_t n, const float *const p[3], const float *const nrm[3],
                        const float *const sh_n[3], const float *const d[3], const float *t, const uint8_t *active,
                        const float *weight, float eta, const hf_receiver_t *rcv, A &a) {
    if (!all3(p) || !all3(nrm) || !all3(sh_n) || !all3(d) || !t || !rcv) return fail(HF_EINVAL, "%s: NULL argument", who);
    if (n >= ((size_t) 1 << 32)) return fail(HF_EINVAL, "%s: more than 2^32 samples", who);
    if (!isfinite(eta) || !(eta > 0.f)) return fail(HF_EINVAL, "%s: eta must be finite and positive (got %g)", who, (double) eta);
    a.n = n; a.eta = eta; a.rcp_eta = 1.f / eta; a.t = t; a.active = active; a.weight = weight;
    for (int c = 0; c < 3; ++c) { a.p[c] = p[c]; a.nrm[c] = nrm[c]; a.sh_n[c] = sh_n[c]; a.d[c] = d[c]; }
    return HF_OK;
}
// ... and the receiver
template <class A>
static int caustic_receiver(const char *who, const hf_receiver_t *rcv, A &a) {
    double ex[3], ey[3], N[3], lx = 0.0, ly = 0.0, xy = 0.0, ln = 0.0;
    for (int c = 0; c < 3; ++c) {
        if (!isfinite(rcv->origin[c]) || !isfinite(rcv->ex[c]) || !isfinite(rcv->ey[c]))
            return fail(HF_EINVAL, "%s: the receiver must be finite", who);
        ex[c] = rcv->ex[c]; ey[c] = rcv->ey[c];
        lx += ex[c] * ex[c]; ly += ey[c] * ey[c]; xy += ex[c] * ey[c];
    }
    N[0] = ex[1] * ey[2] - ex[2] * ey[1]; N[1] = ex[2] * ey[0] - ex[0] * ey[2]; N[2] = ex[0] * ey[1] - ex[1] * ey[0];
    for (int c = 0; c < 3; ++c) ln += N[c] * N[c];
    if (!(ln > 0.0)) return fail(HF_EINVAL, "%s: the receiver's ex x ey is zero", who);
    if (fabs(xy) > 1e-5 * sqrt(lx * ly)) return fail(HF_EINVAL, "%s: the receiver's ex and ey are not orthogonal", who);
    for (int c = 0; c < 3; ++c) {
        a.origin[c] = rcv->origin[c]; a.ex[c] = rcv->ex[c]; a.ey[c] = rcv->ey[c]; a.N[c] = (float) (N[c] / sqrt(ln));
    }
    return HF_OK;
}
// What the four hf_caustic_* entries share: the wavefront rows, the interface, the power and the receiver
static int caustic_args(const char *who, size_t n, const float *const p[3], const float *const nrm[3],
                        const float *const sh_n[3], const float *const d[3], const float *t, const uint8_t *active,
                        const float *weight, float eta, float power, const hf_receiver_t *rcv, hf_caustic_args &a) {
    a = {};
    const int rc = caustic_rows(who, n, p, nrm, sh_n, d, t, active, weight, eta, rcv, a);
    if (rc != HF_OK) return rc;
    if (!isfinite(power)) return fail(HF_EINVAL, "%s: power must be finite", who);
    a.power = power;
    return caustic_receiver(who, rcv, a);
}

extern "C" int hf_caustic_rays(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                               const float *const d[3], const float *t, const uint8_t *active, float eta,
                               const hf_receiver_t *receiver, float *const out_o[3], float *const out_d[3],
                               float *out_maxt, hf_stream_t stream) {
    const char *fn = "hf_caustic_rays";
    hf_caustic_args a;
    const int rc = caustic_args(fn, n, p, nrm, sh_n, d, t, active, nullptr, eta, 1.f, receiver, a);
    if (rc != HF_OK) return rc;
    if (!all3(out_o) || !all3(out_d) || !out_maxt) return fail(HF_EINVAL, "%s: NULL argument", fn);
    a.out_maxt = out_maxt;
    for (int c = 0; c < 3; ++c) { a.out_o[c] = out_o[c]; a.out_d[c] = out_d[c]; }
    return light_launch(hf_launch_caustic, 3, a, stream);
}

extern "C" int hf_caustic_lighting(const hf_field_t *hf, size_t n, const float *const p[3], const float *const nrm[3],
                                   const float *const sh_n[3], const float *const d[3], const float *t,
                                   const uint8_t *active, const float *weight, float eta, float power,
                                   const hf_receiver_t *receiver, float *const pos[2], float *value, uint8_t *vis,
                                   hf_stream_t stream) {
    const char *fn = "hf_caustic_lighting";
    hf_caustic_args a;
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    int rc = caustic_args(fn, n, p, nrm, sh_n, d, t, active, weight, eta, power, receiver, a);
    if (rc != HF_OK) return rc;
    if (!pos || !pos[0] || !pos[1] || !value) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (n == 0) return HF_OK;
    if ((rc = check_device(fn, hf))) return rc;
    a.f = hf->dev; a.pos[0] = pos[0]; a.pos[1] = pos[1]; a.value = value; a.vis = vis;
    return light_launch(hf_launch_caustic, 0, a, stream);
}

extern "C" int hf_caustic_adjoint(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                                  const float *const d[3], const float *t, const uint8_t *active, const float *weight,
                                  float eta, float power, const hf_receiver_t *receiver, const uint8_t *vis,
                                  const float *const grad_pos[2], const float *grad_value, float *const grad_sh_n[3],
                                  float *const grad_p[3], float *grad_weight, hf_stream_t stream) {
    const char *fn = "hf_caustic_adjoint";
    hf_caustic_args a;
    const int rc = caustic_args(fn, n, p, nrm, sh_n, d, t, active, weight, eta, power, receiver, a);
    if (rc != HF_OK) return rc;
    if (!vis) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if ((grad_pos && (!grad_pos[0] || !grad_pos[1])) || (grad_sh_n && !all3(grad_sh_n)) || (grad_p && !all3(grad_p)))
        return fail(HF_EINVAL, "%s: NULL component array", fn);
    a.vis = const_cast<uint8_t *>(vis); a.gvalue = grad_value; a.gw = grad_weight;
    for (int c = 0; c < 2; ++c) a.gpos[c] = grad_pos ? grad_pos[c] : nullptr;
    for (int c = 0; c < 3; ++c) { a.gn[c] = grad_sh_n ? grad_sh_n[c] : nullptr; a.gp[c] = grad_p ? grad_p[c] : nullptr; }
    return light_launch(hf_launch_caustic, 1, a, stream);
}

extern "C" int hf_caustic_tangent(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                                  const float *const d[3], const float *t, const uint8_t *active, const float *weight,
                                  float eta, float power, const hf_receiver_t *receiver, const uint8_t *vis,
                                  const float *const dsh_n[3], const float *const dp[3], const float *dweight,
                                  float *const dpos[2], float *dvalue, hf_stream_t stream) {
    const char *fn = "hf_caustic_tangent";
    hf_caustic_args a;
    const int rc = caustic_args(fn, n, p, nrm, sh_n, d, t, active, weight, eta, power, receiver, a);
    if (rc != HF_OK) return rc;
    if (!vis) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if ((dsh_n && !all3(dsh_n)) || (dp && !all3(dp)) || (dpos && (!dpos[0] || !dpos[1])))
        return fail(HF_EINVAL, "%s: NULL component array", fn);
    a.vis = const_cast<uint8_t *>(vis); a.dw = dweight; a.value = dvalue;
    for (int c = 0; c < 2; ++c) a.pos[c] = dpos ? dpos[c] : nullptr;
    for (int c = 0; c < 3; ++c) { a.dn[c] = dsh_n ? dsh_n[c] : nullptr; a.dp[c] = dp ? dp[c] : nullptr; }
    return light_launch(hf_launch_caustic, 2, a, stream);
}

// ---- the refraction view: a textured receiver seen through the surface, the refracted rays walked in the kernel ----
// the plane texture of the hf_bitmap_* and hf_refract_* entries (A: a block with TW, TH, wrap and tex, zeroed by the caller)
template <class A>
static int bitmap_texture(const char *who, uint32_t TW, uint32_t TH, const float *tex, int wrap, A &a) {
    if (!tex) return fail(HF_EINVAL, "%s: NULL argument", who);
    if (TW == 0 || TH == 0 || (uint64_t) TW * TH >= ((uint64_t) 1 << 31))
        return fail(HF_EINVAL, "%s: the texture must have 1 .. 2^31 - 1 texels (got %u x %u)", who, TW, TH);
    if (wrap != HF_WRAP_CLAMP && wrap != HF_WRAP_REPEAT)
        return fail(HF_EINVAL, "%s: wrap must be HF_WRAP_CLAMP or HF_WRAP_REPEAT (got %d)", who, wrap);
    a.TW = TW; a.TH = TH; a.tex = tex; a.wrap = wrap;
    return HF_OK;
}
static int bitmap_args(const char *who, size_t n, const float *const pos[2], const uint8_t *active, uint32_t TW, uint32_t TH,
                       const float *tex, int wrap, hf_bitmap_args &a) {
    a = {};
    if (!pos || !pos[0] || !pos[1]) return fail(HF_EINVAL, "%s: NULL argument", who);
    if (n >= ((size_t) 1 << 32)) return fail(HF_EINVAL, "%s: more than 2^32 samples", who);
    a.n = n; a.pos[0] = pos[0]; a.pos[1] = pos[1]; a.active = active;
    return bitmap_texture(who, TW, TH, tex, wrap, a);
}

extern "C" int hf_bitmap_eval(size_t n, const float *const pos[2], const uint8_t *active, uint32_t TW, uint32_t TH,
                              const float *tex, int wrap, float *out, float *const out_grad[2], hf_stream_t stream) {
    const char *fn = "hf_bitmap_eval";
    hf_bitmap_args a;
    const int rc = bitmap_args(fn, n, pos, active, TW, TH, tex, wrap, a);
    if (rc != HF_OK) return rc;
    if (!out || (out_grad && (!out_grad[0] || !out_grad[1]))) return fail(HF_EINVAL, "%s: NULL argument", fn);
    a.out = out;
    for (int c = 0; c < 2; ++c) a.out_grad[c] = out_grad ? out_grad[c] : nullptr;
    if (n == 0) return HF_OK;
    hf_launch_bitmap(false, a, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_bitmap_eval_adjoint(size_t n, const float *const pos[2], const uint8_t *active, uint32_t TW, uint32_t TH,
                                      const float *tex, int wrap, const float *grad_out, float *const grad_pos[2],
                                      float *grad_tex, hf_stream_t stream) {
    const char *fn = "hf_bitmap_eval_adjoint";
    hf_bitmap_args a;
    const int rc = bitmap_args(fn, n, pos, active, TW, TH, tex, wrap, a);
    if (rc != HF_OK) return rc;
    if (!grad_out || (grad_pos && (!grad_pos[0] || !grad_pos[1]))) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (!grad_pos && !grad_tex) return fail(HF_EINVAL, "%s: grad_pos and grad_tex are both NULL", fn);
    a.gout = grad_out; a.gtex = grad_tex;
    for (int c = 0; c < 2; ++c) a.gpos[c] = grad_pos ? grad_pos[c] : nullptr;
    if (n == 0) return HF_OK;
    hf_launch_bitmap(true, a, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

// ---- the normal map: the shading normal perturbed by a planar RGB texture, one launch per entry ----
// What the three hf_normalmap_* entries share: the rows of the record and the texture
static int normalmap_args(const char *who, size_t n, const float *const uv[2], const float *const sh_n[3],
                          const float *const dp_du[3], const uint8_t *active, uint32_t TW, uint32_t TH, const float *tex,
                          int wrap, hf_normalmap_args &a) {
    a = {};
    if (!uv || !uv[0] || !uv[1] || !all3(sh_n) || !all3(dp_du)) return fail(HF_EINVAL, "%s: NULL argument", who);
    if (n >= ((size_t) 1 << 32)) return fail(HF_EINVAL, "%s: more than 2^32 samples", who);
    a.n = n; a.active = active;
    for (int c = 0; c < 2; ++c) a.uv[c] = uv[c];
    for (int c = 0; c < 3; ++c) { a.sh_n[c] = sh_n[c]; a.dp_du[c] = dp_du[c]; }
    return bitmap_texture(who, TW, TH, tex, wrap, a);
}

extern "C" int hf_normalmap_eval(size_t n, const float *const uv[2], const float *const sh_n[3], const float *const dp_du[3],
                                 const uint8_t *active, uint32_t TW, uint32_t TH, const float *tex, int wrap,
                                 float *const out_n[3], uint8_t *mask, hf_stream_t stream) {
    const char *fn = "hf_normalmap_eval";
    hf_normalmap_args a;
    const int rc = normalmap_args(fn, n, uv, sh_n, dp_du, active, TW, TH, tex, wrap, a);
    if (rc != HF_OK) return rc;
    if (!out_n || !out_n[0] || !out_n[1] || !out_n[2]) return fail(HF_EINVAL, "%s: NULL argument", fn);
    for (int c = 0; c < 3; ++c) a.out_n[c] = out_n[c];
    a.mask = mask;
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_normalmap, 0, a, stream);
}

extern "C" int hf_normalmap_eval_tangent(size_t n, const float *const uv[2], const float *const sh_n[3],
                                         const float *const dp_du[3], const uint8_t *active, uint32_t TW, uint32_t TH,
                                         const float *tex, int wrap, const float *dtex, const float *const duv[2],
                                         const float *const dsh_n[3], const float *const ddp_du[3], float *const dout_n[3],
                                         hf_stream_t stream) {
    const char *fn = "hf_normalmap_eval_tangent";
    hf_normalmap_args a;
    const int rc = normalmap_args(fn, n, uv, sh_n, dp_du, active, TW, TH, tex, wrap, a);
    if (rc != HF_OK) return rc;
    if (!dout_n || !dout_n[0] || !dout_n[1] || !dout_n[2]) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if ((duv && (!duv[0] || !duv[1])) || (dsh_n && !all3(dsh_n)) || (ddp_du && !all3(ddp_du)))
        return fail(HF_EINVAL, "%s: NULL component array", fn);
    a.dtex = dtex;
    for (int c = 0; c < 2; ++c) a.duv[c] = duv ? duv[c] : nullptr;
    for (int c = 0; c < 3; ++c) {
        a.out_n[c] = dout_n[c];
        a.dn[c] = dsh_n ? dsh_n[c] : nullptr;
        a.dp[c] = ddp_du ? ddp_du[c] : nullptr;
    }
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_normalmap, 2, a, stream);
}

extern "C" int hf_normalmap_eval_adjoint(size_t n, const float *const uv[2], const float *const sh_n[3],
                                         const float *const dp_du[3], const uint8_t *active, uint32_t TW, uint32_t TH,
                                         const float *tex, int wrap, const float *const grad_out[3], float *grad_tex,
                                         float *const grad_uv[2], float *const grad_sh_n[3], float *const grad_dp_du[3],
                                         hf_stream_t stream) {
    const char *fn = "hf_normalmap_eval_adjoint";
    hf_normalmap_args a;
    const int rc = normalmap_args(fn, n, uv, sh_n, dp_du, active, TW, TH, tex, wrap, a);
    if (rc != HF_OK) return rc;
    if (!all3(grad_out)) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if ((grad_uv && (!grad_uv[0] || !grad_uv[1])) || (grad_sh_n && !all3(grad_sh_n)) || (grad_dp_du && !all3(grad_dp_du)))
        return fail(HF_EINVAL, "%s: NULL component array", fn);
    if (!grad_tex && !grad_uv && !grad_sh_n && !grad_dp_du)
        return fail(HF_EINVAL, "%s: grad_tex, grad_uv, grad_sh_n and grad_dp_du are all NULL", fn);
    a.gtex = grad_tex;
    for (int c = 0; c < 2; ++c) a.guv[c] = grad_uv ? grad_uv[c] : nullptr;
    for (int c = 0; c < 3; ++c) {
        a.gout[c] = grad_out[c];
        a.gn[c] = grad_sh_n ? grad_sh_n[c] : nullptr;
        a.gp[c] = grad_dp_du ? grad_dp_du[c] : nullptr;
    }
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_normalmap, 1, a, stream);
}

// ---- the bump map: the shading normal perturbed by the slopes of a one-plane texture, one launch per entry ----
// What the three hf_bumpmap_* entries share: the rows of the record, the texture and the scale
static int bumpmap_args(const char *who, size_t n, const float *const uv[2], const float *const sh_n[3],
                        const float *const n_geo[3], const float *const dp_du[3], const float *const dp_dv[3],
                        const uint8_t *active, uint32_t TW, uint32_t TH, const float *tex, int wrap, float scale,
                        hf_bumpmap_args &a) {
    a = {};
    if (!uv || !uv[0] || !uv[1] || !all3(sh_n) || !all3(n_geo) || !all3(dp_du) || !all3(dp_dv))
        return fail(HF_EINVAL, "%s: NULL argument", who);
    if (n >= ((size_t) 1 << 32)) return fail(HF_EINVAL, "%s: more than 2^32 samples", who);
    if (!isfinite(scale)) return fail(HF_EINVAL, "%s: scale must be finite (got %g)", who, (double) scale);
    a.n = n; a.active = active; a.scale = scale;
    for (int c = 0; c < 2; ++c) a.uv[c] = uv[c];
    for (int c = 0; c < 3; ++c) { a.sh_n[c] = sh_n[c]; a.n_geo[c] = n_geo[c]; a.dp_du[c] = dp_du[c]; a.dp_dv[c] = dp_dv[c]; }
    return bitmap_texture(who, TW, TH, tex, wrap, a);
}

extern "C" int hf_bumpmap_eval(size_t n, const float *const uv[2], const float *const sh_n[3], const float *const n_geo[3],
                               const float *const dp_du[3], const float *const dp_dv[3], const uint8_t *active, uint32_t TW,
                               uint32_t TH, const float *tex, int wrap, float scale, float *const out_n[3], uint8_t *mask,
                               hf_stream_t stream) {
    const char *fn = "hf_bumpmap_eval";
    hf_bumpmap_args a;
    const int rc = bumpmap_args(fn, n, uv, sh_n, n_geo, dp_du, dp_dv, active, TW, TH, tex, wrap, scale, a);
    if (rc != HF_OK) return rc;
    if (!out_n || !out_n[0] || !out_n[1] || !out_n[2]) return fail(HF_EINVAL, "%s: NULL argument", fn);
    for (int c = 0; c < 3; ++c) a.out_n[c] = out_n[c];
    a.mask = mask;
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_bumpmap, 0, a, stream);
}

extern "C" int hf_bumpmap_eval_tangent(size_t n, const float *const uv[2], const float *const sh_n[3],
                                       const float *const n_geo[3], const float *const dp_du[3], const float *const dp_dv[3],
                                       const uint8_t *active, uint32_t TW, uint32_t TH, const float *tex, int wrap, float scale,
                                       const float *dtex, const float *const duv[2], const float *const dsh_n[3],
                                       const float *const ddp_du[3], const float *const ddp_dv[3], float *const dout_n[3],
                                       hf_stream_t stream) {
    const char *fn = "hf_bumpmap_eval_tangent";
    hf_bumpmap_args a;
    const int rc = bumpmap_args(fn, n, uv, sh_n, n_geo, dp_du, dp_dv, active, TW, TH, tex, wrap, scale, a);
    if (rc != HF_OK) return rc;
    if (!dout_n || !dout_n[0] || !dout_n[1] || !dout_n[2]) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if ((duv && (!duv[0] || !duv[1])) || (dsh_n && !all3(dsh_n)) || (ddp_du && !all3(ddp_du)) || (ddp_dv && !all3(ddp_dv)))
        return fail(HF_EINVAL, "%s: NULL component array", fn);
    a.dtex = dtex;
    for (int c = 0; c < 2; ++c) a.duv[c] = duv ? duv[c] : nullptr;
    for (int c = 0; c < 3; ++c) {
        a.out_n[c] = dout_n[c];
        a.dn[c] = dsh_n ? dsh_n[c] : nullptr;
        a.dpu[c] = ddp_du ? ddp_du[c] : nullptr;
        a.dpv[c] = ddp_dv ? ddp_dv[c] : nullptr;
    }
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_bumpmap, 2, a, stream);
}

extern "C" int hf_bumpmap_eval_adjoint(size_t n, const float *const uv[2], const float *const sh_n[3],
                                       const float *const n_geo[3], const float *const dp_du[3], const float *const dp_dv[3],
                                       const uint8_t *active, uint32_t TW, uint32_t TH, const float *tex, int wrap, float scale,
                                       const float *const grad_out[3], float *grad_tex, float *const grad_uv[2],
                                       float *const grad_sh_n[3], float *const grad_dp_du[3], float *const grad_dp_dv[3],
                                       hf_stream_t stream) {
    const char *fn = "hf_bumpmap_eval_adjoint";
    hf_bumpmap_args a;
    const int rc = bumpmap_args(fn, n, uv, sh_n, n_geo, dp_du, dp_dv, active, TW, TH, tex, wrap, scale, a);
    if (rc != HF_OK) return rc;
    if (!all3(grad_out)) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if ((grad_uv && (!grad_uv[0] || !grad_uv[1])) || (grad_sh_n && !all3(grad_sh_n)) || (grad_dp_du && !all3(grad_dp_du)) ||
        (grad_dp_dv && !all3(grad_dp_dv)))
        return fail(HF_EINVAL, "%s: NULL component array", fn);
    if (!grad_tex && !grad_uv && !grad_sh_n && !grad_dp_du && !grad_dp_dv)
        return fail(HF_EINVAL, "%s: grad_tex, grad_uv, grad_sh_n, grad_dp_du and grad_dp_dv are all NULL", fn);
    a.gtex = grad_tex;
    for (int c = 0; c < 2; ++c) a.guv[c] = grad_uv ? grad_uv[c] : nullptr;
    for (int c = 0; c < 3; ++c) {
        a.gout[c] = grad_out[c];
        a.gn[c] = grad_sh_n ? grad_sh_n[c] : nullptr;
        a.gpu[c] = grad_dp_du ? grad_dp_du[c] : nullptr;
        a.gpv[c] = grad_dp_dv ? grad_dp_dv[c] : nullptr;
    }
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_bumpmap, 1, a, stream);
}

// What the three hf_refract_* entries share: the caustic row's rows, interface and receiver, the film's sample count,
// the texture and the medium
static int refract_args(const char *who, size_t n, uint32_t spp, const float *const p[3], const float *const nrm[3],
                        const float *const sh_n[3], const float *const d[3], const float *t, const uint8_t *active,
                        const float *weight, float eta, float sigma_t, const hf_receiver_t *rcv, uint32_t TW, uint32_t TH,
                        const float *tex, int wrap, hf_refract_args &a) {
    a = {};
    int rc = caustic_rows(who, n, p, nrm, sh_n, d, t, active, weight, eta, rcv, a);
    if (rc != HF_OK) return rc;
    if (spp == 0 || n % spp != 0) return fail(HF_EINVAL, "%s: n (%zu) must be a multiple of spp (%u)", who, n, spp);
    if ((rc = bitmap_texture(who, TW, TH, tex, wrap, a))) return rc;
    if (!isfinite(sigma_t) || sigma_t < 0.f)
        return fail(HF_EINVAL, "%s: sigma_t must be finite and not negative (got %g)", who, (double) sigma_t);
    a.spp = spp; a.sigma_t = sigma_t;
    return caustic_receiver(who, rcv, a);
}

extern "C" int hf_refract_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3],
                                   const float *const nrm[3], const float *const sh_n[3], const float *const d[3],
                                   const float *t, const uint8_t *active, const float *weight, float eta, float sigma_t,
                                   const hf_receiver_t *receiver, uint32_t TW, uint32_t TH, const float *tex, int wrap,
                                   float *image, float *value, uint8_t *vis, float *const pos[2], hf_stream_t stream) {
    const char *fn = "hf_refract_lighting";
    hf_refract_args a;
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    int rc = refract_args(fn, n, spp, p, nrm, sh_n, d, t, active, weight, eta, sigma_t, receiver, TW, TH, tex, wrap, a);
    if (rc != HF_OK) return rc;
    if (pos && (!pos[0] || !pos[1])) return fail(HF_EINVAL, "%s: NULL pos component array", fn);
    if (!image && !value && !vis && !pos) return fail(HF_EINVAL, "%s: image, value, vis and pos are all NULL", fn);
    if (n == 0) return HF_OK;
    if ((rc = check_device(fn, hf))) return rc;
    a.f = hf->dev; a.image = image; a.value = value; a.vis = vis;
    for (int c = 0; c < 2; ++c) a.pos[c] = pos ? pos[c] : nullptr;
    return light_launch(hf_launch_refract, 0, a, stream);
}

extern "C" int hf_refract_lighting_adjoint(size_t n, uint32_t spp, const float *const p[3], const float *const nrm[3],
                                           const float *const sh_n[3], const float *const d[3], const float *t,
                                           const uint8_t *active, const float *weight, float eta, float sigma_t,
                                           const hf_receiver_t *receiver, uint32_t TW, uint32_t TH, const float *tex, int wrap,
                                           const uint8_t *vis, const float *grad_image, const float *grad_value,
                                           float *const grad_sh_n[3], float *const grad_p[3], float *grad_weight,
                                           float *grad_tex, hf_stream_t stream) {
    const char *fn = "hf_refract_lighting_adjoint";
    hf_refract_args a;
    int rc = refract_args(fn, n, spp, p, nrm, sh_n, d, t, active, weight, eta, sigma_t, receiver, TW, TH, tex, wrap, a);
    if (rc != HF_OK) return rc;
    if (grad_p && !all3(grad_p)) return fail(HF_EINVAL, "%s: NULL grad_p component array", fn);
    if ((rc = light_value_adjoint_io(fn, !vis, grad_image, grad_value, grad_sh_n, grad_weight, grad_tex, a))) return rc;
    a.vis = const_cast<uint8_t *>(vis);
    for (int c = 0; c < 3; ++c) a.gp[c] = grad_p ? grad_p[c] : nullptr;
    return light_launch(hf_launch_refract, 1, a, stream);
}

extern "C" int hf_refract_lighting_tangent(size_t n, uint32_t spp, const float *const p[3], const float *const nrm[3],
                                           const float *const sh_n[3], const float *const d[3], const float *t,
                                           const uint8_t *active, const float *weight, float eta, float sigma_t,
                                           const hf_receiver_t *receiver, uint32_t TW, uint32_t TH, const float *tex, int wrap,
                                           const uint8_t *vis, const float *const dsh_n[3], const float *const dp[3],
                                           const float *dweight, const float *dtex, float *dimage, float *dvalue,
                                           hf_stream_t stream) {
    const char *fn = "hf_refract_lighting_tangent";
    hf_refract_args a;
    int rc = refract_args(fn, n, spp, p, nrm, sh_n, d, t, active, weight, eta, sigma_t, receiver, TW, TH, tex, wrap, a);
    if (rc != HF_OK) return rc;
    if (dp && !all3(dp)) return fail(HF_EINVAL, "%s: NULL dp component array", fn);
    if ((rc = light_value_tangent_io(fn, !vis, dsh_n, dweight, dtex, dimage, dvalue, a))) return rc;
    a.vis = const_cast<uint8_t *>(vis);
    for (int c = 0; c < 3; ++c) a.dp[c] = dp ? dp[c] : nullptr;
    return light_launch(hf_launch_refract, 2, a, stream);
}

// ---- area-light lighting: a rectangle emitter, the shadow rays towards it traced in the kernel ----
// the lamp's checks and what follows from it alone: n_l = normalize(ex x ey) and A = 4 |ex x ey|, in double
static int rect_lamp(const char *who, const hf_rect_light_t *light, double nl[3], double *area) {
    if (!light) return fail(HF_EINVAL, "%s: NULL argument", who);
    for (int c = 0; c < 3; ++c)
        if (!isfinite(light->center[c]) || !isfinite(light->ex[c]) || !isfinite(light->ey[c]))
            return fail(HF_EINVAL, "%s: the light's center, ex and ey must be finite", who);
    if (!isfinite(light->radiance)) return fail(HF_EINVAL, "%s: the light's radiance must be finite", who);
    const double ex[3] = { light->ex[0], light->ex[1], light->ex[2] }, ey[3] = { light->ey[0], light->ey[1], light->ey[2] };
    const double cr[3] = { ex[1] * ey[2] - ex[2] * ey[1], ex[2] * ey[0] - ex[0] * ey[2], ex[0] * ey[1] - ex[1] * ey[0] };
    const double len = sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
    if (!(len > 0.0)) return fail(HF_EINVAL, "%s: the light's ex and ey span no area (|ex x ey| == 0)", who);
    for (int c = 0; c < 3; ++c) nl[c] = cr[c] / len;
    *area = 4.0 * len;
    return HF_OK;
}

extern "C" int hf_rect_light_geometry(const hf_rect_light_t *light, float *area, float normal[3]) {
    const char *fn = "hf_rect_light_geometry";
    double nl[3], A;
    const int rc = rect_lamp(fn, light, nl, &A);
    if (rc != HF_OK) return rc;
    if (area) *area = (float) A;
    for (int c = 0; c < 3 && normal; ++c) normal[c] = (float) nl[c];
    return HF_OK;
}

// What the four hf_rect_* entries share (hf_rect_rays passes spp 1, num_rays k + 1, no texture, albedo 1): the
// wavefront, the lamp, its texture (tex NULL: none, TW and TH are not read) and the scale of the sum
static int rect_args(const char *who, size_t n, uint32_t spp, const float *const p[3], const float *const sh_n[3],
                     const float *const d[3], const float *t, const float *weight, uint32_t num_rays, uint32_t seed,
                     const uint32_t *ray_id, const hf_rect_light_t *light, uint32_t TW, uint32_t TH, const float *tex,
                     float albedo, hf_rect_args &a) {
    a = {};
    int rc = light_args(who, "points of the light", n, spp, sh_n, d, t, weight, num_rays, seed, ray_id, !all3(p) || !light, a);
    if (rc != HF_OK) return rc;
    double A;
    if ((rc = rect_lamp(who, light, a.nld, &A))) return rc;
    if (!isfinite(albedo)) return fail(HF_EINVAL, "%s: albedo must be finite", who);
    if (tex && (rc = bitmap_texture(who, TW, TH, tex, HF_WRAP_CLAMP, a))) return rc;
    for (int c = 0; c < 3; ++c) {
        a.p[c] = p[c]; a.center[c] = light->center[c]; a.ex[c] = light->ex[c]; a.ey[c] = light->ey[c]; a.nl[c] = (float) a.nld[c];
    }
    a.scale = (float) ((double) albedo * (double) light->radiance * A / (3.141592653589793 * (double) num_rays));
    return HF_OK;
}

extern "C" int hf_rect_rays(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                            const float *const d[3], const float *t, uint32_t k, uint32_t seed, const uint32_t *ray_id,
                            const hf_rect_light_t *light, float *const out_o[3], float *const out_d[3], float *out_maxt,
                            hf_stream_t stream) {
    const char *fn = "hf_rect_rays";
    hf_rect_args a;
    if (k >= 32) return fail(HF_EINVAL, "%s: point k must be below 32 (got %u)", fn, k);
    int rc = rect_args(fn, n, 1, p, sh_n, d, t, nullptr, k + 1, seed, ray_id, light, 0, 0, nullptr, 1.f, a);
    if (rc != HF_OK || (rc = light_rays_out(fn, p, nrm, out_o, out_d, out_maxt, a))) return rc;
    a.k = k;
    return light_launch(hf_launch_rect, 3, a, stream);
}

extern "C" int hf_rect_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3],
                                const float *const nrm[3], const float *const sh_n[3], const float *const d[3],
                                const float *t, const float *weight, uint32_t num_rays, uint32_t seed,
                                const uint32_t *ray_id, const hf_rect_light_t *light, uint32_t TW, uint32_t TH,
                                const float *tex, float albedo, float *image, uint32_t *vis_bits, hf_stream_t stream) {
    const char *fn = "hf_rect_lighting";
    hf_rect_args a;
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    int rc = rect_args(fn, n, spp, p, sh_n, d, t, weight, num_rays, seed, ray_id, light, TW, TH, tex, albedo, a);
    if (rc != HF_OK || (rc = light_forward_out(fn, p, nrm, image, a))) return rc;
    if (n == 0) return HF_OK;
    if ((rc = check_device(fn, hf))) return rc;
    a.f = hf->dev; a.vis_bits = vis_bits;
    return light_launch(hf_launch_rect, 0, a, stream);
}

extern "C" int hf_rect_lighting_adjoint(size_t n, uint32_t spp, const float *const p[3], const float *const sh_n[3],
                                        const float *const d[3], const float *t, const float *weight, uint32_t num_rays,
                                        uint32_t seed, const uint32_t *ray_id, const hf_rect_light_t *light, uint32_t TW,
                                        uint32_t TH, const float *tex, float albedo, const uint32_t *vis_bits,
                                        const float *grad_image, float *const grad_sh_n[3], float *const grad_p[3],
                                        float *grad_weight, float *grad_tex, hf_stream_t stream) {
    const char *fn = "hf_rect_lighting_adjoint";
    hf_rect_args a;
    const int rc = rect_args(fn, n, spp, p, sh_n, d, t, weight, num_rays, seed, ray_id, light, TW, TH, tex, albedo, a);
    if (rc != HF_OK) return rc;
    if (!vis_bits || !grad_image) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (grad_sh_n && !all3(grad_sh_n)) return fail(HF_EINVAL, "%s: NULL grad_sh_n component array", fn);
    if (grad_p && !all3(grad_p)) return fail(HF_EINVAL, "%s: NULL grad_p component array", fn);
    a.vis_bits = const_cast<uint32_t *>(vis_bits); a.gimg = grad_image; a.gw = grad_weight; a.gdata = grad_tex;
    for (int c = 0; c < 3; ++c) { a.gn[c] = grad_sh_n ? grad_sh_n[c] : nullptr; a.gp[c] = grad_p ? grad_p[c] : nullptr; }
    return light_launch(hf_launch_rect, 1, a, stream);
}

extern "C" int hf_rect_lighting_tangent(size_t n, uint32_t spp, const float *const p[3], const float *const sh_n[3],
                                        const float *const d[3], const float *t, const float *weight, uint32_t num_rays,
                                        uint32_t seed, const uint32_t *ray_id, const hf_rect_light_t *light, uint32_t TW,
                                        uint32_t TH, const float *tex, float albedo, const uint32_t *vis_bits,
                                        const float *const dsh_n[3], const float *const dp[3], const float *dweight,
                                        const float *dtex, float *dimage, hf_stream_t stream) {
    const char *fn = "hf_rect_lighting_tangent";
    hf_rect_args a;
    int rc = rect_args(fn, n, spp, p, sh_n, d, t, weight, num_rays, seed, ray_id, light, TW, TH, tex, albedo, a);
    if (rc != HF_OK) return rc;
    if (dp && !all3(dp)) return fail(HF_EINVAL, "%s: NULL dp component array", fn);
    if ((rc = light_tangent_io(fn, !vis_bits, dsh_n, dweight, dimage, a))) return rc;
    a.vis_bits = const_cast<uint32_t *>(vis_bits); a.ddata = dtex;
    for (int c = 0; c < 3; ++c) a.dp[c] = dp ? dp[c] : nullptr;
    return light_launch(hf_launch_rect, 2, a, stream);
}

// ---- projector lighting: a pinhole that throws a texture onto the terrain, the shadow ray traced in the kernel ----
// What the four hf_projector_* entries share (hf_projector_rays passes spp 1, no texture, HF_WRAP_REPEAT, albedo 1): the
// wavefront, the projector's checks, the affine inverse (formed once, here, in double: adjugate) and the constants of
// the mapping
static int projector_args(const char *who, size_t n, uint32_t spp, const float *const p[3], const float *const sh_n[3],
                          const float *const d[3], const float *t, const float *weight, const hf_projector_t *pr,
                          uint32_t TW, uint32_t TH, const float *tex, int wrap, float albedo, hf_projector_args &a) {
    a = {};
    if (!all3(p) || !all3(sh_n) || !all3(d) || !t || !pr) return fail(HF_EINVAL, "%s: NULL argument", who);
    if (n >= ((size_t) 1 << 32)) return fail(HF_EINVAL, "%s: more than 2^32 samples", who);
    if (spp == 0 || n % spp != 0) return fail(HF_EINVAL, "%s: n (%zu) must be a multiple of spp (%u)", who, n, spp);
    if (TW == 0 || TH == 0 || (uint64_t) TW * TH >= ((uint64_t) 1 << 31))
        return fail(HF_EINVAL, "%s: the texture must have 1 .. 2^31 - 1 texels (got %u x %u)", who, TW, TH);
    if (wrap != HF_WRAP_CLAMP && wrap != HF_WRAP_REPEAT)
        return fail(HF_EINVAL, "%s: wrap must be HF_WRAP_CLAMP or HF_WRAP_REPEAT (got %d)", who, wrap);
    const double *M = pr->to_world;
    for (int j = 0; j < 12; ++j)
        if (!isfinite(M[j])) return fail(HF_EINVAL, "%s: the projector's to_world must be finite", who);
    if (!isfinite(pr->x_fov) || !isfinite(pr->scale)) return fail(HF_EINVAL, "%s: the projector's x_fov and scale must be finite", who);
    if (!(pr->x_fov > 0.0) || !(pr->x_fov < 180.0))
        return fail(HF_EINVAL, "%s: the projector's x_fov must be in (0, 180) degrees (got %g)", who, pr->x_fov);
    for (int i = 0; i < 3; ++i) // projector.cpp: has_scale(), hf_sensor_t's check
        for (int j = i; j < 3; ++j) {
            const double g = M[i] * M[j] + M[4 + i] * M[4 + j] + M[8 + i] * M[8 + j];
            if (fabs(g - (i == j ? 1.0 : 0.0)) > 1e-4)
                return fail(HF_EINVAL, "%s: scale factors in the projector's to_world are not allowed", who);
        }
    if (!isfinite(albedo)) return fail(HF_EINVAL, "%s: albedo must be finite", who);
    const double m[3][3] = { { M[0], M[1], M[2] }, { M[4], M[5], M[6] }, { M[8], M[9], M[10] } };
    const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                       m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) { // Ai[r][c] = cofactor(c, r) / det
            const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
            a.Ai[3 * r + c] = (m[r1][c1] * m[r2][c2] - m[r1][c2] * m[r2][c1]) / det;
        }
    for (int k = 0; k < 3; ++k) {
        a.c[k] = M[4 * k + 3]; a.cf[k] = (float) M[4 * k + 3];
        a.p[k] = p[k]; a.sh_n[k] = sh_n[k]; a.d[k] = d[k];
    }
    a.n = n; a.spp = spp; a.t = t; a.weight = weight;
    a.TW = TW; a.TH = TH; a.tex = tex; a.wrap = wrap;
    a.tau = tan(pr->x_fov * 3.141592653589793 / 360.0);
    a.dtau = (3.141592653589793 / 360.0) * (1.0 + a.tau * a.tau);
    a.aspect = (double) TW / (double) TH; // projector.cpp:128-129
    a.albedo = (double) albedo; a.cs = (double) albedo * (double) pr->scale;
    return HF_OK;
}

extern "C" int hf_projector_rays(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                                 const float *const d[3], const float *t, const hf_projector_t *projector, uint32_t TW,
                                 uint32_t TH, float *const out_o[3], float *const out_d[3], float *out_maxt,
                                 hf_stream_t stream) {
    const char *fn = "hf_projector_rays";
    hf_projector_args a;
    int rc = projector_args(fn, n, 1, p, sh_n, d, t, nullptr, projector, TW, TH, nullptr, HF_WRAP_REPEAT, 1.f, a);
    if (rc != HF_OK || (rc = light_rays_out(fn, p, nrm, out_o, out_d, out_maxt, a))) return rc;
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_projector, 3, a, stream);
}

extern "C" int hf_projector_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3],
                                     const float *const nrm[3], const float *const sh_n[3], const float *const d[3],
                                     const float *t, const float *weight, const hf_projector_t *projector, uint32_t TW,
                                     uint32_t TH, const float *tex, int wrap, float albedo, float *image, float *value,
                                     uint8_t *vis, float *const uv[2], hf_stream_t stream) {
    const char *fn = "hf_projector_lighting";
    hf_projector_args a;
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    int rc = projector_args(fn, n, spp, p, sh_n, d, t, weight, projector, TW, TH, tex, wrap, albedo, a);
    if (rc != HF_OK || (rc = light_forward_out(fn, p, nrm, image, a, true))) return rc;
    if (uv && (!uv[0] || !uv[1])) return fail(HF_EINVAL, "%s: NULL uv component array", fn);
    if (!image && !value && !vis && !uv) return fail(HF_EINVAL, "%s: image, value, vis and uv are all NULL", fn);
    if (n == 0) return HF_OK;
    if ((rc = check_device(fn, hf))) return rc;
    a.f = hf->dev; a.value = value; a.vis = vis;
    for (int c = 0; c < 2; ++c) a.uv[c] = uv ? uv[c] : nullptr;
    return light_launch(hf_launch_projector, 0, a, stream);
}

extern "C" size_t hf_projector_workspace_floats(void) { return 2u * hf_projector_slab_doubles(); }

extern "C" int hf_projector_lighting_adjoint(size_t n, uint32_t spp, const float *const p[3], const float *const sh_n[3],
                                             const float *const d[3], const float *t, const float *weight,
                                             const hf_projector_t *projector, uint32_t TW, uint32_t TH, const float *tex,
                                             int wrap, float albedo, const uint8_t *vis, const float *grad_image,
                                             const float *grad_value, float *const grad_sh_n[3], float *const grad_p[3],
                                             float *grad_weight, float *grad_tex, float *grad_to_world, float *grad_fov,
                                             float *grad_scale, float *workspace, hf_stream_t stream) {
    const char *fn = "hf_projector_lighting_adjoint";
    hf_projector_args a;
    int rc = projector_args(fn, n, spp, p, sh_n, d, t, weight, projector, TW, TH, tex, wrap, albedo, a);
    if (rc != HF_OK) return rc;
    if (grad_p && !all3(grad_p)) return fail(HF_EINVAL, "%s: NULL grad_p component array", fn);
    if ((rc = light_value_adjoint_io(fn, !vis, grad_image, grad_value, grad_sh_n, grad_weight, grad_tex, a))) return rc;
    const bool reduced = grad_to_world || grad_fov || grad_scale;
    if (reduced && !workspace) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (reduced && ((uintptr_t) workspace & 7u) != 0) return fail(HF_EINVAL, "%s: the workspace must be 8-byte aligned", fn);
    a.vis = const_cast<uint8_t *>(vis);
    for (int c = 0; c < 3; ++c) a.gp[c] = grad_p ? grad_p[c] : nullptr;
    a.slab = reduced ? (double *) workspace : nullptr;
    a.g_tw = grad_to_world; a.g_fov = grad_fov; a.g_scale = grad_scale;
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_projector, 1, a, stream);
}

extern "C" int hf_projector_lighting_tangent(size_t n, uint32_t spp, const float *const p[3], const float *const sh_n[3],
                                             const float *const d[3], const float *t, const float *weight,
                                             const hf_projector_t *projector, uint32_t TW, uint32_t TH, const float *tex,
                                             int wrap, float albedo, const uint8_t *vis, const float *const dsh_n[3],
                                             const float *const dp[3], const float *dweight, const float *dtex,
                                             const float *d_to_world, const float *d_fov, const float *d_scale,
                                             float *dimage, float *dvalue, hf_stream_t stream) {
    const char *fn = "hf_projector_lighting_tangent";
    hf_projector_args a;
    int rc = projector_args(fn, n, spp, p, sh_n, d, t, weight, projector, TW, TH, tex, wrap, albedo, a);
    if (rc != HF_OK) return rc;
    if (dp && !all3(dp)) return fail(HF_EINVAL, "%s: NULL dp component array", fn);
    if ((rc = light_value_tangent_io(fn, !vis, dsh_n, dweight, dtex, dimage, dvalue, a))) return rc;
    a.vis = const_cast<uint8_t *>(vis);
    for (int c = 0; c < 3; ++c) a.dp[c] = dp ? dp[c] : nullptr;
    a.d_tw = d_to_world; a.d_fov = d_fov; a.d_scale = d_scale;
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_projector, 2, a, stream);
}

// ---- spot lighting: a rig of 1..HF_MAX_LIGHTS cone emitters, the shadow rays traced in the kernel ----
// What the four hf_spot_* entries share (hf_spot_rays passes spp 1, one light, albedo 1): the wavefront, every light's
// checks, its affine inverse (formed once, here, in double: adjugate), the angles in radians and their cosines
static int spot_args(const char *who, size_t n, uint32_t spp, const float *const p[3], const float *const sh_n[3],
                     const float *const d[3], const float *t, const float *weight, uint32_t n_lights,
                     const hf_spot_light_t *lights, float albedo, hf_spot_args &a) {
    a = {};
    if (!all3(p) || !all3(sh_n) || !all3(d) || !t || !lights) return fail(HF_EINVAL, "%s: NULL argument", who);
    if (n >= ((size_t) 1 << 32)) return fail(HF_EINVAL, "%s: more than 2^32 samples", who);
    if (spp == 0 || n % spp != 0) return fail(HF_EINVAL, "%s: n (%zu) must be a multiple of spp (%u)", who, n, spp);
    if (n_lights == 0 || n_lights > HF_MAX_LIGHTS)
        return fail(HF_EINVAL, "%s: 1..%d lights supported (got %u)", who, HF_MAX_LIGHTS, n_lights);
    if (!isfinite(albedo)) return fail(HF_EINVAL, "%s: albedo must be finite", who);
    const double rad = 3.141592653589793 / 180.0;
    for (uint32_t l = 0; l < n_lights; ++l) {
        const hf_spot_light_t &s = lights[l];
        hf_spot_light_dev &o = a.L[l];
        const double *M = s.to_world;
        for (int j = 0; j < 12; ++j)
            if (!isfinite(M[j])) return fail(HF_EINVAL, "%s: light %u: to_world must be finite", who, l);
        if (!isfinite(s.intensity) || !isfinite(s.cutoff_angle) || !isfinite(s.beam_width))
            return fail(HF_EINVAL, "%s: light %u: intensity, cutoff_angle and beam_width must be finite", who, l);
        if (!(s.beam_width > 0.f) || !(s.beam_width <= s.cutoff_angle) || !(s.cutoff_angle <= 180.f))
            return fail(HF_EINVAL, "%s: light %u: 0 < beam_width <= cutoff_angle <= 180 degrees (got %g, %g)", who, l,
                        (double) s.beam_width, (double) s.cutoff_angle);
        for (int i = 0; i < 3; ++i) // spot.cpp: has_scale(), hf_sensor_t's check
            for (int j = i; j < 3; ++j) {
                const double g = M[i] * M[j] + M[4 + i] * M[4 + j] + M[8 + i] * M[8 + j];
                if (fabs(g - (i == j ? 1.0 : 0.0)) > 1e-4)
                    return fail(HF_EINVAL, "%s: light %u: scale factors in to_world are not allowed", who, l);
            }
        const double m[3][3] = { { M[0], M[1], M[2] }, { M[4], M[5], M[6] }, { M[8], M[9], M[10] } };
        const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) { // Ai[r][c] = cofactor(c, r) / det
                const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
                o.Ai[3 * r + c] = (m[r1][c1] * m[r2][c2] - m[r1][c2] * m[r2][c1]) / det;
            }
        for (int k = 0; k < 3; ++k) { o.c[k] = M[4 * k + 3]; o.cf[k] = (float) M[4 * k + 3]; }
        o.cutoff = (double) s.cutoff_angle * rad; o.beam = (double) s.beam_width * rad;
        // (180 degrees: cos(pi) rounds to -1 exactly, so cutoff = beam = 180 lights every direction but the one behind)
        o.cos_cutoff = cos(o.cutoff); o.cos_beam = cos(o.beam);
        o.inv_width = s.cutoff_angle > s.beam_width ? 1.0 / (o.cutoff - o.beam) : 0.0;
        o.ci = (double) albedo / 3.141592653589793 * (double) s.intensity;
    }
    for (int k = 0; k < 3; ++k) { a.p[k] = p[k]; a.sh_n[k] = sh_n[k]; a.d[k] = d[k]; }
    a.n = n; a.spp = spp; a.n_lights = n_lights; a.t = t; a.weight = weight;
    a.albedo_pi = (double) albedo / 3.141592653589793;
    // atan(t) / t as a polynomial in t^2 on [0, tan(pi / 8)] (Chebyshev interpolation, degree 9: 7e-16 off), then the
    // constants of the two folds
    static const double atan_c[14] = { 0.99999999999999922, -0.33333333333215148, 0.19999999977575814, -0.14285712620968255,
                                       0.11111047794231604, -0.090895137758045072, 0.076733844914957605, -0.065051346366116522,
                                       0.05022119694104614, -0.025281436432647405, 0.41421356237309503, 0.78539816339744831,
                                       1.5707963267948966, 3.141592653589793 };
    for (int j = 0; j < 14; ++j) a.atan_c[j] = atan_c[j];
    return HF_OK;
}

extern "C" int hf_spot_rays(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                            const float *const d[3], const float *t, const hf_spot_light_t *light, float *const out_o[3],
                            float *const out_d[3], float *out_maxt, hf_stream_t stream) {
    const char *fn = "hf_spot_rays";
    hf_spot_args a;
    int rc = spot_args(fn, n, 1, p, sh_n, d, t, nullptr, 1, light, 1.f, a);
    if (rc != HF_OK || (rc = light_rays_out(fn, p, nrm, out_o, out_d, out_maxt, a))) return rc;
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_spot, 3, a, stream);
}

extern "C" int hf_spot_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3],
                                const float *const nrm[3], const float *const sh_n[3], const float *const d[3],
                                const float *t, const float *weight, uint32_t n_lights, const hf_spot_light_t *lights,
                                float albedo, float *image, float *value, uint8_t *vis, hf_stream_t stream) {
    const char *fn = "hf_spot_lighting";
    hf_spot_args a;
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    int rc = spot_args(fn, n, spp, p, sh_n, d, t, weight, n_lights, lights, albedo, a);
    if (rc != HF_OK || (rc = light_forward_out(fn, p, nrm, image, a, true))) return rc;
    if (!image && !value && !vis) return fail(HF_EINVAL, "%s: image, value and vis are all NULL", fn);
    if (n == 0) return HF_OK;
    if ((rc = check_device(fn, hf))) return rc;
    a.f = hf->dev; a.value = value; a.vis = vis;
    return light_launch(hf_launch_spot, 0, a, stream);
}

extern "C" size_t hf_spot_workspace_floats(uint32_t n_lights) {
    return n_lights >= 1 && n_lights <= HF_MAX_LIGHTS ? 2u * hf_spot_slab_doubles(n_lights) : 0u;
}

extern "C" int hf_spot_lighting_adjoint(size_t n, uint32_t spp, const float *const p[3], const float *const sh_n[3],
                                        const float *const d[3], const float *t, const float *weight, uint32_t n_lights,
                                        const hf_spot_light_t *lights, float albedo, const uint8_t *vis,
                                        const float *grad_image, const float *grad_value, float *const grad_sh_n[3],
                                        float *const grad_p[3], float *grad_weight, float *grad_lights, float *workspace,
                                        hf_stream_t stream) {
    const char *fn = "hf_spot_lighting_adjoint";
    hf_spot_args a;
    int rc = spot_args(fn, n, spp, p, sh_n, d, t, weight, n_lights, lights, albedo, a);
    if (rc != HF_OK) return rc;
    if (!vis) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (grad_sh_n && !all3(grad_sh_n)) return fail(HF_EINVAL, "%s: NULL grad_sh_n component array", fn);
    if (grad_p && !all3(grad_p)) return fail(HF_EINVAL, "%s: NULL grad_p component array", fn);
    if (grad_lights && !workspace) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (grad_lights && ((uintptr_t) workspace & 7u) != 0) return fail(HF_EINVAL, "%s: the workspace must be 8-byte aligned", fn);
    a.vis = const_cast<uint8_t *>(vis);
    a.gimg = grad_image; a.gvalue = grad_value; a.gw = grad_weight;
    for (int c = 0; c < 3; ++c) { a.gn[c] = grad_sh_n ? grad_sh_n[c] : nullptr; a.gp[c] = grad_p ? grad_p[c] : nullptr; }
    a.slab = grad_lights ? (double *) workspace : nullptr;
    a.g_lights = grad_lights;
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_spot, 1, a, stream);
}

extern "C" int hf_spot_lighting_tangent(size_t n, uint32_t spp, const float *const p[3], const float *const sh_n[3],
                                        const float *const d[3], const float *t, const float *weight, uint32_t n_lights,
                                        const hf_spot_light_t *lights, float albedo, const uint8_t *vis,
                                        const float *const dsh_n[3], const float *const dp[3], const float *dweight,
                                        const float *d_lights, float *dimage, float *dvalue, hf_stream_t stream) {
    const char *fn = "hf_spot_lighting_tangent";
    hf_spot_args a;
    int rc = spot_args(fn, n, spp, p, sh_n, d, t, weight, n_lights, lights, albedo, a);
    if (rc != HF_OK) return rc;
    if (!vis) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (!dimage && !dvalue) return fail(HF_EINVAL, "%s: dimage and dvalue are both NULL", fn);
    if (dp && !all3(dp)) return fail(HF_EINVAL, "%s: NULL dp component array", fn);
    if ((rc = light_tangent_io(fn, false, dsh_n, dweight, dimage, a, true))) return rc;
    a.vis = const_cast<uint8_t *>(vis); a.value = dvalue;
    for (int c = 0; c < 3; ++c) a.dp[c] = dp ? dp[c] : nullptr;
    a.d_lights = d_lights;
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_spot, 2, a, stream);
}

// ---- directional lighting: a rig of 1..HF_MAX_LIGHTS distant emitters, the shadow rays traced in the kernel ----
// The two checks of a rig that this row and the specular row share.  The sizes of the wavefront and of the rig:
static int rig_sizes(const char *who, size_t n, uint32_t spp, uint32_t n_lights) {
    if (n >= ((size_t) 1 << 32)) return fail(HF_EINVAL, "%s: more than 2^32 samples", who);
    if (spp == 0 || n % spp != 0) return fail(HF_EINVAL, "%s: n (%zu) must be a multiple of spp (%u)", who, n, spp);
    if (n_lights == 0 || n_lights > HF_MAX_LIGHTS)
        return fail(HF_EINVAL, "%s: 1..%d lights supported (got %u)", who, HF_MAX_LIGHTS, n_lights);
    return HF_OK;
}
// ... and every light's checks and its device block, the unit direction formed once, here, in double; ce = scale * irradiance
static int rig_lights(const char *who, uint32_t n_lights, const hf_directional_light_t *lights, double scale,
                      hf_directional_light_dev *L) {
    for (uint32_t l = 0; l < n_lights; ++l) {
        const hf_directional_light_t &s = lights[l];
        hf_directional_light_dev &o = L[l];
        const double *v = s.to_light;
        if (!isfinite(v[0]) || !isfinite(v[1]) || !isfinite(v[2]) || !isfinite(s.irradiance))
            return fail(HF_EINVAL, "%s: light %u: to_light and irradiance must be finite", who, l);
        const double len = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (!(len > 0.0) || !isfinite(len) || !isfinite(1.0 / len))
            return fail(HF_EINVAL, "%s: light %u: to_light must have a finite length > 0", who, l);
        o.inv_len = 1.0 / len;
        for (int k = 0; k < 3; ++k) { o.l[k] = v[k] / len; o.lf[k] = (float) o.l[k]; }
        o.ce = scale * (double) s.irradiance;
    }
    return HF_OK;
}
// What the four hf_directional_* entries share (hf_directional_rays passes spp 1, one light, albedo 1): the wavefront, the
// rig's checks, ce = albedo / pi * irradiance
static int directional_args(const char *who, size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                            const float *t, const float *weight, uint32_t n_lights, const hf_directional_light_t *lights,
                            float albedo, hf_directional_args &a) {
    a = {};
    if (!all3(sh_n) || !all3(d) || !t || !lights) return fail(HF_EINVAL, "%s: NULL argument", who);
    int rc = rig_sizes(who, n, spp, n_lights);
    if (rc != HF_OK) return rc;
    if (!isfinite(albedo)) return fail(HF_EINVAL, "%s: albedo must be finite", who);
    if ((rc = rig_lights(who, n_lights, lights, (double) albedo / 3.141592653589793, a.L))) return rc;
    for (int k = 0; k < 3; ++k) { a.sh_n[k] = sh_n[k]; a.d[k] = d[k]; }
    a.n = n; a.spp = spp; a.n_lights = n_lights; a.t = t; a.weight = weight;
    a.albedo_pi = (double) albedo / 3.141592653589793;
    return HF_OK;
}

extern "C" int hf_directional_rays(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                                   const float *const d[3], const float *t, const hf_directional_light_t *light,
                                   float *const out_o[3], float *const out_d[3], float *out_maxt, hf_stream_t stream) {
    const char *fn = "hf_directional_rays";
    hf_directional_args a;
    int rc = directional_args(fn, n, 1, sh_n, d, t, nullptr, 1, light, 1.f, a);
    if (rc != HF_OK || (rc = light_rays_out(fn, p, nrm, out_o, out_d, out_maxt, a))) return rc;
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_directional, 3, a, stream);
}

extern "C" int hf_directional_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3],
                                       const float *const nrm[3], const float *const sh_n[3], const float *const d[3],
                                       const float *t, const float *weight, uint32_t n_lights,
                                       const hf_directional_light_t *lights, float albedo, float *image, float *value,
                                       uint8_t *vis, hf_stream_t stream) {
    const char *fn = "hf_directional_lighting";
    hf_directional_args a;
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    int rc = directional_args(fn, n, spp, sh_n, d, t, weight, n_lights, lights, albedo, a);
    if (rc != HF_OK || (rc = light_forward_out(fn, p, nrm, image, a, true))) return rc;
    if (!image && !value && !vis) return fail(HF_EINVAL, "%s: image, value and vis are all NULL", fn);
    if (n == 0) return HF_OK;
    if ((rc = check_device(fn, hf))) return rc;
    a.f = hf->dev; a.value = value; a.vis = vis;
    return light_launch(hf_launch_directional, 0, a, stream);
}

extern "C" size_t hf_directional_workspace_floats(uint32_t n_lights) {
    return n_lights >= 1 && n_lights <= HF_MAX_LIGHTS ? 2u * hf_directional_slab_doubles(n_lights) : 0u;
}

extern "C" int hf_directional_lighting_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                               const float *t, const float *weight, uint32_t n_lights,
                                               const hf_directional_light_t *lights, float albedo, const uint8_t *vis,
                                               const float *grad_image, const float *grad_value, float *const grad_sh_n[3],
                                               float *grad_weight, float *grad_lights, float *workspace,
                                               hf_stream_t stream) {
    const char *fn = "hf_directional_lighting_adjoint";
    hf_directional_args a;
    int rc = directional_args(fn, n, spp, sh_n, d, t, weight, n_lights, lights, albedo, a);
    if (rc != HF_OK) return rc;
    if (!vis) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (grad_sh_n && !all3(grad_sh_n)) return fail(HF_EINVAL, "%s: NULL grad_sh_n component array", fn);
    if (grad_lights && !workspace) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (grad_lights && ((uintptr_t) workspace & 7u) != 0) return fail(HF_EINVAL, "%s: the workspace must be 8-byte aligned", fn);
    a.vis = const_cast<uint8_t *>(vis);
    a.gimg = grad_image; a.gvalue = grad_value; a.gw = grad_weight;
    for (int c = 0; c < 3; ++c) a.gn[c] = grad_sh_n ? grad_sh_n[c] : nullptr;
    a.slab = grad_lights ? (double *) workspace : nullptr;
    a.g_lights = grad_lights;
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_directional, 1, a, stream);
}

extern "C" int hf_directional_lighting_tangent(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                               const float *t, const float *weight, uint32_t n_lights,
                                               const hf_directional_light_t *lights, float albedo, const uint8_t *vis,
                                               const float *const dsh_n[3], const float *dweight, const float *d_lights,
                                               float *dimage, float *dvalue, hf_stream_t stream) {
    const char *fn = "hf_directional_lighting_tangent";
    hf_directional_args a;
    int rc = directional_args(fn, n, spp, sh_n, d, t, weight, n_lights, lights, albedo, a);
    if (rc != HF_OK) return rc;
    if (!vis) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (!dimage && !dvalue) return fail(HF_EINVAL, "%s: dimage and dvalue are both NULL", fn);
    if ((rc = light_tangent_io(fn, false, dsh_n, dweight, dimage, a, true))) return rc;
    a.vis = const_cast<uint8_t *>(vis); a.value = dvalue;
    a.d_lights = d_lights;
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_directional, 2, a, stream);
}

// ---- specular highlights: the GGX lobe under the directional rig, the directional row's byte read ----
// What the three hf_specular_* entries share: the wavefront, the rig's checks (rig_sizes, rig_lights: ce = irradiance),
// the interface
static int specular_args(const char *who, size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                         const float *weight, const float *alpha, float eta, uint32_t n_lights,
                         const hf_directional_light_t *lights, const uint8_t *vis, hf_specular_args &a) {
    a = {};
    if (!all3(sh_n) || !all3(d) || !alpha || !lights || !vis) return fail(HF_EINVAL, "%s: NULL argument", who);
    int rc = rig_sizes(who, n, spp, n_lights);
    if (rc != HF_OK || (rc = rig_lights(who, n_lights, lights, 1.0, a.L)) || (rc = light_interface(who, eta, a))) return rc;
    for (int k = 0; k < 3; ++k) { a.sh_n[k] = sh_n[k]; a.d[k] = d[k]; }
    a.n = n; a.spp = spp; a.n_lights = n_lights; a.weight = weight; a.alpha = alpha; a.vis = vis;
    return HF_OK;
}

extern "C" int hf_specular_lighting(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                    const float *weight, const float *alpha, float eta, uint32_t n_lights,
                                    const hf_directional_light_t *lights, const uint8_t *vis, float *image, float *value,
                                    hf_stream_t stream) {
    const char *fn = "hf_specular_lighting";
    hf_specular_args a;
    const int rc = specular_args(fn, n, spp, sh_n, d, weight, alpha, eta, n_lights, lights, vis, a);
    if (rc != HF_OK) return rc;
    if (!image && !value) return fail(HF_EINVAL, "%s: image and value are both NULL", fn);
    a.image = image; a.value = value;
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_specular, 0, a, stream);
}

extern "C" size_t hf_specular_workspace_floats(uint32_t n_lights) {
    return n_lights >= 1 && n_lights <= HF_MAX_LIGHTS ? 2u * hf_specular_slab_doubles(n_lights) : 0u;
}

extern "C" int hf_specular_lighting_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                            const float *weight, const float *alpha, float eta, uint32_t n_lights,
                                            const hf_directional_light_t *lights, const uint8_t *vis,
                                            const float *grad_image, const float *grad_value, float *const grad_sh_n[3],
                                            float *grad_weight, float *grad_alpha, float *grad_lights, float *workspace,
                                            hf_stream_t stream) {
    const char *fn = "hf_specular_lighting_adjoint";
    hf_specular_args a;
    const int rc = specular_args(fn, n, spp, sh_n, d, weight, alpha, eta, n_lights, lights, vis, a);
    if (rc != HF_OK) return rc;
    if (grad_sh_n && !all3(grad_sh_n)) return fail(HF_EINVAL, "%s: NULL grad_sh_n component array", fn);
    if (grad_lights && !workspace) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (grad_lights && ((uintptr_t) workspace & 7u) != 0) return fail(HF_EINVAL, "%s: the workspace must be 8-byte aligned", fn);
    a.gimg = grad_image; a.gvalue = grad_value; a.gw = grad_weight; a.ga = grad_alpha;
    for (int c = 0; c < 3; ++c) a.gn[c] = grad_sh_n ? grad_sh_n[c] : nullptr;
    a.slab = grad_lights ? (double *) workspace : nullptr;
    a.g_lights = grad_lights;
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_specular, 1, a, stream);
}

extern "C" int hf_specular_lighting_tangent(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                            const float *weight, const float *alpha, float eta, uint32_t n_lights,
                                            const hf_directional_light_t *lights, const uint8_t *vis,
                                            const float *const dsh_n[3], const float *dweight, const float *dalpha,
                                            const float *d_lights, float *dimage, float *dvalue, hf_stream_t stream) {
    const char *fn = "hf_specular_lighting_tangent";
    hf_specular_args a;
    int rc = specular_args(fn, n, spp, sh_n, d, weight, alpha, eta, n_lights, lights, vis, a);
    if (rc != HF_OK) return rc;
    if (!dimage && !dvalue) return fail(HF_EINVAL, "%s: dimage and dvalue are both NULL", fn);
    if ((rc = light_tangent_io(fn, false, dsh_n, dweight, dimage, a, true))) return rc;
    a.value = dvalue; a.da = dalpha; a.d_lights = d_lights;
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_specular, 2, a, stream);
}

// ---- homogeneous medium: single scattering below a top plane under the directional rig, the shadow rays of
// every sample's points traced in the kernel ----
// What the four hf_medium_* entries share (hf_medium_rays passes spp 1, one light, num_steps k + 1: its k must name one
// of 32 points): the wavefront, the rig's checks (rig_sizes, rig_lights: ce = irradiance), the medium's, and the unit
// top normal and every nu_j = <l_j, N>, formed once, here, in double
static int medium_args(const char *who, size_t n, uint32_t spp, const float *const o[3], const float *const d[3],
                       const float *t, const float *weight, const hf_medium_t *medium, uint32_t n_lights,
                       const hf_directional_light_t *lights, uint32_t num_steps, uint32_t seed, const uint32_t *ray_id,
                       hf_medium_args &a) {
    a = {};
    if (!all3(o) || !all3(d) || !t || !medium || !lights) return fail(HF_EINVAL, "%s: NULL argument", who);
    int rc = rig_sizes(who, n, spp, n_lights);
    if (rc != HF_OK) return rc;
    if (num_steps == 0 || num_steps > 32) return fail(HF_EINVAL, "%s: 1..32 points per sample (got %u)", who, num_steps);
    if (!isfinite(medium->sigma_t) || !(medium->sigma_t > 0.f))
        return fail(HF_EINVAL, "%s: sigma_t must be finite and > 0 (got %g)", who, (double) medium->sigma_t);
    if (!isfinite(medium->albedo)) return fail(HF_EINVAL, "%s: albedo must be finite", who);
    if (!isfinite(medium->g) || !(fabsf(medium->g) < 1.f))
        return fail(HF_EINVAL, "%s: g must lie in (-1, 1) (got %g)", who, (double) medium->g);
    const double *v = medium->top_normal, *q = medium->top_origin;
    if (!isfinite(q[0]) || !isfinite(q[1]) || !isfinite(q[2])) return fail(HF_EINVAL, "%s: top_origin must be finite", who);
    const double len = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (!isfinite(v[0]) || !isfinite(v[1]) || !isfinite(v[2]) || !(len > 0.0) || !isfinite(len) || !isfinite(1.0 / len))
        return fail(HF_EINVAL, "%s: top_normal must have a finite length > 0", who);
    if ((rc = rig_lights(who, n_lights, lights, 1.0, a.L))) return rc;
    for (int c = 0; c < 3; ++c) { a.N[c] = v[c] / len; a.top_o[c] = q[c]; a.o[c] = o[c]; a.d[c] = d[c]; }
    for (uint32_t j = 0; j < n_lights; ++j) {
        const double nu = a.L[j].l[0] * a.N[0] + a.L[j].l[1] * a.N[1] + a.L[j].l[2] * a.N[2];
        if (nu > 0.0 && isfinite(1.0 / nu)) { a.on |= 1u << j; a.inv_nu[j] = 1.0 / nu; } // (else: the light does not shine in)
    }
    a.sigma_t = (double) medium->sigma_t; a.albedo = (double) medium->albedo; a.g = (double) medium->g;
    a.n = n; a.spp = spp; a.n_lights = n_lights; a.num_steps = num_steps; a.seed = seed; a.ray_id = ray_id;
    a.t = t; a.weight = weight;
    return HF_OK;
}

extern "C" int hf_medium_rays(size_t n, const float *const o[3], const float *const d[3], const float *t,
                              const hf_medium_t *medium, const hf_directional_light_t *light, uint32_t k, uint32_t seed,
                              const uint32_t *ray_id, float *const out_o[3], float *const out_d[3], float *out_maxt,
                              hf_stream_t stream) {
    const char *fn = "hf_medium_rays";
    hf_medium_args a;
    if (k >= 32) return fail(HF_EINVAL, "%s: k must be below 32 (got %u)", fn, k);
    const int rc = medium_args(fn, n, 1, o, d, t, nullptr, medium, 1, light, k + 1, seed, ray_id, a);
    if (rc != HF_OK) return rc;
    if (!all3(out_o) || !all3(out_d) || !out_maxt) return fail(HF_EINVAL, "%s: NULL argument", fn);
    a.k = k; a.out_maxt = out_maxt;
    for (int c = 0; c < 3; ++c) { a.out_o[c] = out_o[c]; a.out_d[c] = out_d[c]; }
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_medium, 3, a, stream);
}

extern "C" int hf_medium_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const o[3],
                                  const float *const d[3], const float *t, const float *weight, const hf_medium_t *medium,
                                  uint32_t n_lights, const hf_directional_light_t *lights, uint32_t num_steps,
                                  uint32_t seed, const uint32_t *ray_id, float *image, float *value, uint32_t *vis_bits,
                                  hf_stream_t stream) {
    const char *fn = "hf_medium_lighting";
    hf_medium_args a;
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    int rc = medium_args(fn, n, spp, o, d, t, weight, medium, n_lights, lights, num_steps, seed, ray_id, a);
    if (rc != HF_OK) return rc;
    if (!image && !value && !vis_bits) return fail(HF_EINVAL, "%s: image, value and vis_bits are all NULL", fn);
    if (n == 0) return HF_OK;
    if ((rc = check_device(fn, hf))) return rc;
    a.f = hf->dev; a.image = image; a.value = value; a.vis_bits = vis_bits;
    return light_launch(hf_launch_medium, 0, a, stream);
}

extern "C" size_t hf_medium_workspace_floats(uint32_t n_lights) {
    return n_lights >= 1 && n_lights <= HF_MAX_LIGHTS ? 2u * hf_medium_slab_doubles() : 0u;
}

extern "C" int hf_medium_lighting_adjoint(size_t n, uint32_t spp, const float *const o[3], const float *const d[3],
                                          const float *t, const float *weight, const hf_medium_t *medium,
                                          uint32_t n_lights, const hf_directional_light_t *lights, uint32_t num_steps,
                                          uint32_t seed, const uint32_t *ray_id, const uint32_t *vis_bits,
                                          const float *grad_image, const float *grad_value, float *grad_weight,
                                          float *grad_t, float *grad_params, float *workspace, hf_stream_t stream) {
    const char *fn = "hf_medium_lighting_adjoint";
    hf_medium_args a;
    const int rc = medium_args(fn, n, spp, o, d, t, weight, medium, n_lights, lights, num_steps, seed, ray_id, a);
    if (rc != HF_OK) return rc;
    if (!vis_bits) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (grad_params && !workspace) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (grad_params && ((uintptr_t) workspace & 7u) != 0) return fail(HF_EINVAL, "%s: the workspace must be 8-byte aligned", fn);
    a.vis_bits = const_cast<uint32_t *>(vis_bits);
    a.gimg = grad_image; a.gvalue = grad_value; a.gw = grad_weight; a.gt = grad_t;
    a.slab = grad_params ? (double *) workspace : nullptr;
    a.g_params = grad_params;
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_medium, 1, a, stream);
}

extern "C" int hf_medium_lighting_tangent(size_t n, uint32_t spp, const float *const o[3], const float *const d[3],
                                          const float *t, const float *weight, const hf_medium_t *medium,
                                          uint32_t n_lights, const hf_directional_light_t *lights, uint32_t num_steps,
                                          uint32_t seed, const uint32_t *ray_id, const uint32_t *vis_bits,
                                          const float *dweight, const float *dt, const float *d_params, float *dimage,
                                          float *dvalue, hf_stream_t stream) {
    const char *fn = "hf_medium_lighting_tangent";
    hf_medium_args a;
    const int rc = medium_args(fn, n, spp, o, d, t, weight, medium, n_lights, lights, num_steps, seed, ray_id, a);
    if (rc != HF_OK) return rc;
    if (!vis_bits) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (!dimage && !dvalue) return fail(HF_EINVAL, "%s: dimage and dvalue are both NULL", fn);
    a.vis_bits = const_cast<uint32_t *>(vis_bits);
    a.image = dimage; a.value = dvalue; a.dw = dweight; a.dt = dt; a.d_params = d_params;
    if (n == 0) return HF_OK;
    return light_launch(hf_launch_medium, 2, a, stream);
}

// ---- the sensor: the primary wavefront of a perspective or an orthographic camera ----
static int log2_or_minus1(uint32_t v) {
    if (v == 0 || (v & (v - 1u))) return -1;
    int s = 0;
    while ((1u << s) != v) ++s;
    return s;
}
// the checks of the sensor alone, what every hf_sensor_* entry starts with
static int sensor_checks(const char *who, const hf_sensor_t *s, size_t n) {
    if (!s) return fail(HF_EINVAL, "%s: NULL argument", who);
    if (s->type != HF_SENSOR_PERSPECTIVE && s->type != HF_SENSOR_ORTHOGRAPHIC)
        return fail(HF_EINVAL, "%s: the sensor's type must be HF_SENSOR_PERSPECTIVE or HF_SENSOR_ORTHOGRAPHIC (got %d)", who, s->type);
    const bool persp = s->type == HF_SENSOR_PERSPECTIVE;
    if ((uint64_t) n >= (1ull << 32)) return fail(HF_EINVAL, "%s: n must be below 2^32", who);
    if (s->crop_w == 0 || s->crop_h == 0 || (uint64_t) s->crop_x + s->crop_w > s->film_w ||
        (uint64_t) s->crop_y + s->crop_h > s->film_h)
        return fail(HF_EINVAL, "%s: the crop window (%u, %u, %u, %u) is empty or not inside the %u x %u film", who, s->crop_x,
                    s->crop_y, s->crop_w, s->crop_h, s->film_w, s->film_h);
    for (int j = 0; j < 12; ++j)
        if (!isfinite(s->to_world[j])) return fail(HF_EINVAL, "%s: the sensor's to_world must be finite", who);
    if (!isfinite(s->near_clip) || !isfinite(s->far_clip) || (persp && !isfinite(s->x_fov)))
        return fail(HF_EINVAL, "%s: the sensor's near_clip, far_clip and x_fov must be finite", who);
    if (!(s->near_clip > 0.0) || !(s->far_clip > s->near_clip))
        return fail(HF_EINVAL, "%s: the sensor needs 0 < near_clip < far_clip (got %g, %g)", who, s->near_clip, s->far_clip);
    const double *M = s->to_world;
    if (persp) {
        if (!(s->x_fov > 0.0) || !(s->x_fov < 180.0))
            return fail(HF_EINVAL, "%s: the sensor's x_fov must be in (0, 180) degrees (got %g)", who, s->x_fov);
        for (int i = 0; i < 3; ++i) // perspective.cpp:163-164: has_scale()
            for (int j = i; j < 3; ++j) {
                const double g = M[i] * M[j] + M[4 + i] * M[4 + j] + M[8 + i] * M[8 + j];
                if (fabs(g - (i == j ? 1.0 : 0.0)) > 1e-4)
                    return fail(HF_EINVAL, "%s: scale factors in the sensor's to_world are not allowed (perspective)", who);
            }
    }
    return HF_OK;
}
// What hf_sensor_rays and its two derivatives share: the checks of the sensor and of the wavefront, and every constant
// of the kernels, formed in double
static int sensor_args(const char *who, const hf_sensor_t *s, size_t n, uint32_t start, uint32_t spp, uint32_t seed,
                       const uint32_t *ray_id, hf_sensor_args &a) {
    a = {};
    const int rc = sensor_checks(who, s, n);
    if (rc != HF_OK) return rc;
    if (spp == 0) return fail(HF_EINVAL, "%s: spp must be at least 1", who);
    const bool persp = s->type == HF_SENSOR_PERSPECTIVE;
    const double *M = s->to_world;
    if (!ray_id) {
        const uint64_t window = (uint64_t) s->crop_w * s->crop_h;
        if ((uint64_t) start + (uint64_t) n > (1ull << 32) || window > (1ull << 32) || window * spp > (1ull << 32))
            return fail(HF_EINVAL, "%s: start + n and crop_w crop_h spp must not exceed 2^32 without ray_id", who);
    }
    a.n = n; a.start = start; a.spp = spp; a.seed = seed; a.ray_id = ray_id;
    a.crop_w = s->crop_w; a.crop_x = s->crop_x; a.crop_y = s->crop_y;
    a.spp_shift = log2_or_minus1(spp); a.crop_w_shift = log2_or_minus1(s->crop_w);
    a.film_w = (double) s->film_w; a.film_h = (double) s->film_h; a.aspect = a.film_w / a.film_h; // sensor.h:242
    for (int k = 0; k < 3; ++k) {
        for (int j = 0; j < 3; ++j) a.A[3 * k + j] = M[4 * k + j];
        a.c[k] = M[4 * k + 3];
    }
    a.near = s->near_clip; a.span = s->far_clip - s->near_clip;
    if (persp) {
        a.tau = tan(s->x_fov * 3.141592653589793 / 360.0); // transform.h:216-233: 1 / cot(fov / 2)
        a.dtau = (3.141592653589793 / 360.0) * (1.0 + a.tau * a.tau);
    } else {
        a.tau = 1.0; a.dtau = 0.0;
        const double len = sqrt(M[2] * M[2] + M[6] * M[6] + M[10] * M[10]); // orthographic.cpp:137: normalize(to_world * (0, 0, 1))
        if (!(len > 0.0) || !isfinite(len)) return fail(HF_EINVAL, "%s: the sensor's to_world has no z axis (orthographic)", who);
        for (int k = 0; k < 3; ++k) { a.dz[k] = M[4 * k + 2] / len; a.An[k] = M[4 * k + 2] * s->near_clip; }
        a.inv_len_z = 1.0 / len;
    }
    return HF_OK;
}

static int sensor_launch(int mode, const hf_sensor_t *s, const hf_sensor_args &a, hf_stream_t stream) {
    if (a.n == 0) return HF_OK;
    hf_launch_sensor(mode, s->type, a, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_sensor_rays(const hf_sensor_t *sensor, size_t n, uint32_t start, uint32_t spp, uint32_t seed,
                              const uint32_t *ray_id, float *const out_o[3], float *const out_d[3], float *out_maxt,
                              float *const out_pos[2], hf_stream_t stream) {
    const char *fn = "hf_sensor_rays";
    hf_sensor_args a;
    const int rc = sensor_args(fn, sensor, n, start, spp, seed, ray_id, a);
    if (rc != HF_OK) return rc;
    if (!all3(out_o) || !all3(out_d) || !out_maxt) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (out_pos && (!out_pos[0] || !out_pos[1])) return fail(HF_EINVAL, "%s: NULL out_pos component array", fn);
    for (int k = 0; k < 3; ++k) { a.out_o[k] = out_o[k]; a.out_d[k] = out_d[k]; }
    a.out_maxt = out_maxt;
    for (int k = 0; k < 2; ++k) a.out_pos[k] = out_pos ? out_pos[k] : nullptr;
    return sensor_launch(0, sensor, a, stream);
}

extern "C" int hf_sensor_rays_tangent(const hf_sensor_t *sensor, size_t n, uint32_t start, uint32_t spp, uint32_t seed,
                                      const uint32_t *ray_id, const float *d_to_world, const float *d_fov,
                                      float *const out_do[3], float *const out_dd[3], hf_stream_t stream) {
    const char *fn = "hf_sensor_rays_tangent";
    hf_sensor_args a;
    const int rc = sensor_args(fn, sensor, n, start, spp, seed, ray_id, a);
    if (rc != HF_OK) return rc;
    if (!all3(out_do) || !all3(out_dd)) return fail(HF_EINVAL, "%s: NULL argument", fn);
    for (int k = 0; k < 3; ++k) { a.out_o[k] = out_do[k]; a.out_d[k] = out_dd[k]; }
    a.d_tw = d_to_world; a.d_fov = d_fov;
    return sensor_launch(2, sensor, a, stream);
}

extern "C" size_t hf_sensor_workspace_floats(void) { return 2u * hf_sensor_slab_doubles(); }

extern "C" int hf_sensor_rays_adjoint(const hf_sensor_t *sensor, size_t n, uint32_t start, uint32_t spp, uint32_t seed,
                                      const uint32_t *ray_id, const float *const grad_o[3], const float *const grad_d[3],
                                      float *grad_to_world, float *grad_fov, float *workspace, hf_stream_t stream) {
    const char *fn = "hf_sensor_rays_adjoint";
    hf_sensor_args a;
    const int rc = sensor_args(fn, sensor, n, start, spp, seed, ray_id, a);
    if (rc != HF_OK) return rc;
    if (grad_o && !all3(grad_o)) return fail(HF_EINVAL, "%s: NULL grad_o component array", fn);
    if (grad_d && !all3(grad_d)) return fail(HF_EINVAL, "%s: NULL grad_d component array", fn);
    if (!workspace) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (((uintptr_t) workspace & 7u) != 0) return fail(HF_EINVAL, "%s: the workspace must be 8-byte aligned", fn);
    for (int k = 0; k < 3; ++k) { a.go[k] = grad_o ? grad_o[k] : nullptr; a.gd[k] = grad_d ? grad_d[k] : nullptr; }
    a.slab = (double *) workspace; a.g_tw = grad_to_world; a.g_fov = grad_fov;
    return sensor_launch(1, sensor, a, stream);
}

// What hf_sensor_project and its two derivatives share.  The affine inverse is formed once, here, in double (adjugate)
static int sensor_project_args(const char *who, const hf_sensor_t *s, size_t n, const float *const p[3], const uint8_t *active,
                               hf_sensor_project_args &a) {
    a = {};
    const int rc = sensor_checks(who, s, n);
    if (rc != HF_OK) return rc;
    if (s->type != HF_SENSOR_PERSPECTIVE)
        return fail(HF_EINVAL, "%s: an orthographic sensor has no sample_direction (a point names no film position there)", who);
    if (!all3(p)) return fail(HF_EINVAL, "%s: NULL argument", who);
    const double *M = s->to_world;
    const double m[3][3] = { { M[0], M[1], M[2] }, { M[4], M[5], M[6] }, { M[8], M[9], M[10] } };
    const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                       m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) { // Ai[r][c] = cofactor(c, r) / det
            const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
            a.Ai[3 * r + c] = (m[r1][c1] * m[r2][c2] - m[r1][c2] * m[r2][c1]) / det;
        }
    for (int k = 0; k < 3; ++k) a.c[k] = M[4 * k + 3];
    a.n = n; a.active = active;
    for (int k = 0; k < 3; ++k) a.p[k] = p[k];
    a.near = s->near_clip; a.far = s->far_clip;
    a.tau = tan(s->x_fov * 3.141592653589793 / 360.0);
    a.dtau = (3.141592653589793 / 360.0) * (1.0 + a.tau * a.tau);
    a.film_w = (double) s->film_w; a.film_h = (double) s->film_h; a.aspect = a.film_w / a.film_h;
    a.crop_x = (double) s->crop_x; a.crop_y = (double) s->crop_y; a.crop_w = (double) s->crop_w; a.crop_h = (double) s->crop_h;
    // importance(): A' = (2 tan(x_fov / 2))^2 / aspect (crop_w / film_w) (crop_h / film_h) (perspective.cpp:340-345)
    a.inv_area = 1.0 / ((2.0 * a.tau) * (2.0 * a.tau) / a.aspect * (a.crop_w * a.crop_h) / (a.film_w * a.film_h));
    return HF_OK;
}
static int sensor_project_launch(int mode, const hf_sensor_project_args &a, hf_stream_t stream) {
    if (a.n == 0) return HF_OK;
    hf_launch_sensor_project(mode, a, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_sensor_project(const hf_sensor_t *sensor, size_t n, const float *const p[3], const uint8_t *active,
                                 float *const uv[2], uint8_t *valid, float *weight, hf_stream_t stream) {
    const char *fn = "hf_sensor_project";
    hf_sensor_project_args a;
    const int rc = sensor_project_args(fn, sensor, n, p, active, a);
    if (rc != HF_OK) return rc;
    if (!uv || !uv[0] || !uv[1] || !valid) return fail(HF_EINVAL, "%s: NULL argument", fn);
    a.uv[0] = uv[0]; a.uv[1] = uv[1]; a.valid = valid; a.weight = weight;
    return sensor_project_launch(0, a, stream);
}

extern "C" int hf_sensor_project_tangent(const hf_sensor_t *sensor, size_t n, const float *const p[3], const uint8_t *active,
                                         const float *const dp[3], const float *d_to_world, const float *d_fov,
                                         float *const duv[2], float *dweight, hf_stream_t stream) {
    const char *fn = "hf_sensor_project_tangent";
    hf_sensor_project_args a;
    const int rc = sensor_project_args(fn, sensor, n, p, active, a);
    if (rc != HF_OK) return rc;
    if (!duv || !duv[0] || !duv[1]) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (dp && !all3(dp)) return fail(HF_EINVAL, "%s: NULL dp component array", fn);
    for (int k = 0; k < 3; ++k) a.dp[k] = dp ? dp[k] : nullptr;
    a.d_tw = d_to_world; a.d_fov = d_fov; a.uv[0] = duv[0]; a.uv[1] = duv[1]; a.weight = dweight;
    return sensor_project_launch(2, a, stream);
}

extern "C" int hf_sensor_project_adjoint(const hf_sensor_t *sensor, size_t n, const float *const p[3], const uint8_t *active,
                                         const float *const grad_uv[2], const float *grad_weight, float *const grad_p[3],
                                         float *grad_to_world, float *grad_fov, float *workspace, hf_stream_t stream) {
    const char *fn = "hf_sensor_project_adjoint";
    hf_sensor_project_args a;
    const int rc = sensor_project_args(fn, sensor, n, p, active, a);
    if (rc != HF_OK) return rc;
    if (grad_uv && (!grad_uv[0] || !grad_uv[1])) return fail(HF_EINVAL, "%s: NULL grad_uv component array", fn);
    if (grad_p && (!grad_p[0] || !grad_p[1] || !grad_p[2])) return fail(HF_EINVAL, "%s: NULL grad_p component array", fn);
    if (!workspace) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (((uintptr_t) workspace & 7u) != 0) return fail(HF_EINVAL, "%s: the workspace must be 8-byte aligned", fn);
    for (int k = 0; k < 2; ++k) a.guv[k] = grad_uv ? grad_uv[k] : nullptr;
    for (int k = 0; k < 3; ++k) a.gp[k] = grad_p ? grad_p[k] : nullptr;
    a.gweight = grad_weight; a.slab = (double *) workspace; a.g_tw = grad_to_world; a.g_fov = grad_fov;
    return sensor_project_launch(1, a, stream);
}

// ---- the thin lens: the perspective sensor with an aperture ----
// the checks of the lens alone, what every hf_thinlens_* entry starts with (the base's follow in sensor_args)
static int thinlens_checks(const char *who, const hf_thinlens_t *l) {
    if (!l) return fail(HF_EINVAL, "%s: NULL argument", who);
    if (l->base.type != HF_SENSOR_PERSPECTIVE)
        return fail(HF_EINVAL, "%s: the lens's base.type must be HF_SENSOR_PERSPECTIVE (got %d)", who, l->base.type);
    if (!isfinite(l->aperture_radius) || l->aperture_radius < 0.0)
        return fail(HF_EINVAL, "%s: aperture_radius must be finite and not negative (got %g)", who, l->aperture_radius);
    if (!isfinite(l->focus_distance) || !(l->focus_distance > 0.0))
        return fail(HF_EINVAL, "%s: focus_distance must be finite and positive (got %g)", who, l->focus_distance);
    return HF_OK;
}
static int thinlens_args(const char *who, const hf_thinlens_t *l, size_t n, uint32_t start, uint32_t spp, uint32_t seed,
                         const uint32_t *ray_id, hf_thinlens_args &a) {
    a = {};
    int rc = thinlens_checks(who, l);
    if (rc != HF_OK) return rc;
    if ((rc = sensor_args(who, &l->base, n, start, spp, seed, ray_id, a.s)) != HF_OK) return rc;
    a.radius = l->aperture_radius; a.focus = l->focus_distance;
    a.lens_o = a.radius * (1.0 - a.s.near / a.focus);
    a.maxt_scale = a.s.span / a.focus;
    return HF_OK;
}
static int thinlens_launch(int mode, const hf_thinlens_args &a, hf_stream_t stream) {
    if (a.s.n == 0) return HF_OK;
    hf_launch_thinlens(mode, a, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_thinlens_rays(const hf_thinlens_t *lens, size_t n, uint32_t start, uint32_t spp, uint32_t seed,
                                const uint32_t *ray_id, float *const out_o[3], float *const out_d[3], float *out_maxt,
                                float *const out_pos[2], hf_stream_t stream) {
    const char *fn = "hf_thinlens_rays";
    hf_thinlens_args a;
    const int rc = thinlens_args(fn, lens, n, start, spp, seed, ray_id, a);
    if (rc != HF_OK) return rc;
    if (!all3(out_o) || !all3(out_d) || !out_maxt) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (out_pos && (!out_pos[0] || !out_pos[1])) return fail(HF_EINVAL, "%s: NULL out_pos component array", fn);
    for (int k = 0; k < 3; ++k) { a.s.out_o[k] = out_o[k]; a.s.out_d[k] = out_d[k]; }
    a.s.out_maxt = out_maxt;
    for (int k = 0; k < 2; ++k) a.s.out_pos[k] = out_pos ? out_pos[k] : nullptr;
    return thinlens_launch(0, a, stream);
}

extern "C" int hf_thinlens_rays_tangent(const hf_thinlens_t *lens, size_t n, uint32_t start, uint32_t spp, uint32_t seed,
                                        const uint32_t *ray_id, const float *d_to_world, const float *d_fov,
                                        const float *d_radius, const float *d_focus, float *const out_do[3],
                                        float *const out_dd[3], hf_stream_t stream) {
    const char *fn = "hf_thinlens_rays_tangent";
    hf_thinlens_args a;
    const int rc = thinlens_args(fn, lens, n, start, spp, seed, ray_id, a);
    if (rc != HF_OK) return rc;
    if (!all3(out_do) || !all3(out_dd)) return fail(HF_EINVAL, "%s: NULL argument", fn);
    for (int k = 0; k < 3; ++k) { a.s.out_o[k] = out_do[k]; a.s.out_d[k] = out_dd[k]; }
    a.s.d_tw = d_to_world; a.s.d_fov = d_fov; a.d_radius = d_radius; a.d_focus = d_focus;
    return thinlens_launch(2, a, stream);
}

extern "C" size_t hf_thinlens_workspace_floats(void) { return 2u * hf_thinlens_slab_doubles(); }

extern "C" int hf_thinlens_rays_adjoint(const hf_thinlens_t *lens, size_t n, uint32_t start, uint32_t spp, uint32_t seed,
                                        const uint32_t *ray_id, const float *const grad_o[3], const float *const grad_d[3],
                                        float *grad_to_world, float *grad_fov, float *grad_radius, float *grad_focus,
                                        float *workspace, hf_stream_t stream) {
    const char *fn = "hf_thinlens_rays_adjoint";
    hf_thinlens_args a;
    const int rc = thinlens_args(fn, lens, n, start, spp, seed, ray_id, a);
    if (rc != HF_OK) return rc;
    if (grad_o && !all3(grad_o)) return fail(HF_EINVAL, "%s: NULL grad_o component array", fn);
    if (grad_d && !all3(grad_d)) return fail(HF_EINVAL, "%s: NULL grad_d component array", fn);
    if (!workspace) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (((uintptr_t) workspace & 7u) != 0) return fail(HF_EINVAL, "%s: the workspace must be 8-byte aligned", fn);
    for (int k = 0; k < 3; ++k) { a.s.go[k] = grad_o ? grad_o[k] : nullptr; a.s.gd[k] = grad_d ? grad_d[k] : nullptr; }
    a.s.slab = (double *) workspace; a.s.g_tw = grad_to_world; a.s.g_fov = grad_fov;
    a.g_radius = grad_radius; a.g_focus = grad_focus;
    return thinlens_launch(1, a, stream);
}

// What hf_thinlens_project and its two derivatives share
static int thinlens_project_args(const char *who, const hf_thinlens_t *l, size_t n, uint32_t start, uint32_t seed,
                                 const uint32_t *ray_id, const float *const p[3], const uint8_t *active,
                                 hf_thinlens_project_args &a) {
    a = {};
    int rc = thinlens_checks(who, l);
    if (rc != HF_OK) return rc;
    if ((rc = sensor_project_args(who, &l->base, n, p, active, a.s)) != HF_OK) return rc;
    if (!ray_id && (uint64_t) start + (uint64_t) n > (1ull << 32))
        return fail(HF_EINVAL, "%s: start + n must not exceed 2^32 without ray_id", who);
    a.start = start; a.seed = seed; a.ray_id = ray_id;
    a.radius = l->aperture_radius; a.focus = l->focus_distance;
    return HF_OK;
}
static int thinlens_project_launch(int mode, const hf_thinlens_project_args &a, hf_stream_t stream) {
    if (a.s.n == 0) return HF_OK;
    hf_launch_thinlens_project(mode, a, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_thinlens_project(const hf_thinlens_t *lens, size_t n, uint32_t start, uint32_t seed, const uint32_t *ray_id,
                                   const float *const p[3], const uint8_t *active, float *const uv[2], uint8_t *valid,
                                   float *weight, hf_stream_t stream) {
    const char *fn = "hf_thinlens_project";
    hf_thinlens_project_args a;
    const int rc = thinlens_project_args(fn, lens, n, start, seed, ray_id, p, active, a);
    if (rc != HF_OK) return rc;
    if (!uv || !uv[0] || !uv[1] || !valid) return fail(HF_EINVAL, "%s: NULL argument", fn);
    a.s.uv[0] = uv[0]; a.s.uv[1] = uv[1]; a.s.valid = valid; a.s.weight = weight;
    return thinlens_project_launch(0, a, stream);
}

extern "C" int hf_thinlens_project_tangent(const hf_thinlens_t *lens, size_t n, uint32_t start, uint32_t seed,
                                           const uint32_t *ray_id, const float *const p[3], const uint8_t *active,
                                           const float *const dp[3], const float *d_to_world, const float *d_fov,
                                           const float *d_radius, const float *d_focus, float *const duv[2], float *dweight,
                                           hf_stream_t stream) {
    const char *fn = "hf_thinlens_project_tangent";
    hf_thinlens_project_args a;
    const int rc = thinlens_project_args(fn, lens, n, start, seed, ray_id, p, active, a);
    if (rc != HF_OK) return rc;
    if (!duv || !duv[0] || !duv[1]) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (dp && !all3(dp)) return fail(HF_EINVAL, "%s: NULL dp component array", fn);
    for (int k = 0; k < 3; ++k) a.s.dp[k] = dp ? dp[k] : nullptr;
    a.s.d_tw = d_to_world; a.s.d_fov = d_fov; a.d_radius = d_radius; a.d_focus = d_focus;
    a.s.uv[0] = duv[0]; a.s.uv[1] = duv[1]; a.s.weight = dweight;
    return thinlens_project_launch(2, a, stream);
}

extern "C" int hf_thinlens_project_adjoint(const hf_thinlens_t *lens, size_t n, uint32_t start, uint32_t seed,
                                           const uint32_t *ray_id, const float *const p[3], const uint8_t *active,
                                           const float *const grad_uv[2], const float *grad_weight, float *const grad_p[3],
                                           float *grad_to_world, float *grad_fov, float *grad_radius, float *grad_focus,
                                           float *workspace, hf_stream_t stream) {
    const char *fn = "hf_thinlens_project_adjoint";
    hf_thinlens_project_args a;
    const int rc = thinlens_project_args(fn, lens, n, start, seed, ray_id, p, active, a);
    if (rc != HF_OK) return rc;
    if (grad_uv && (!grad_uv[0] || !grad_uv[1])) return fail(HF_EINVAL, "%s: NULL grad_uv component array", fn);
    if (grad_p && (!grad_p[0] || !grad_p[1] || !grad_p[2])) return fail(HF_EINVAL, "%s: NULL grad_p component array", fn);
    if (!workspace) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (((uintptr_t) workspace & 7u) != 0) return fail(HF_EINVAL, "%s: the workspace must be 8-byte aligned", fn);
    for (int k = 0; k < 2; ++k) a.s.guv[k] = grad_uv ? grad_uv[k] : nullptr;
    for (int k = 0; k < 3; ++k) a.s.gp[k] = grad_p ? grad_p[k] : nullptr;
    a.s.gweight = grad_weight; a.s.slab = (double *) workspace; a.s.g_tw = grad_to_world; a.s.g_fov = grad_fov;
    a.g_radius = grad_radius; a.g_focus = grad_focus;
    return thinlens_project_launch(1, a, stream);
}

// ---- environment-map lighting: importance-sampled latitude-longitude map, the shadow rays traced in the kernel ----
// What every entry that reads a map shares, the reflection rows' too: the checks of the map (A: a block with W, H, data
// and rot, zeroed by the caller), in two pieces because the entries check other things between them: the texels ...
template <class A>
static int envmap_texels(const char *who, uint32_t W, uint32_t H, const float *data, bool need_data, A &a) {
    if (W < 2 || H < 2) return fail(HF_EINVAL, "%s: the map must have at least 2 x 2 texels (got %u x %u)", who, W, H);
    if (need_data && !data) return fail(HF_EINVAL, "%s: NULL argument", who);
    a.W = W; a.H = H; a.data = data;
    return HF_OK;
}
// ... and the rotation (NULL: the identity)
template <class A>
static int envmap_rot(const char *who, const float rot[9], A &a) {
    for (int j = 0; j < 9; ++j) {
        a.rot[j] = rot ? rot[j] : (j % 4 == 0 ? 1.f : 0.f);
        if (!isfinite(a.rot[j])) return fail(HF_EINVAL, "%s: rot must be finite", who);
    }
    return HF_OK;
}
// the two for the hf_envmap_* entries; table: the sampling table of those that draw from it or build it (else need_table = false)
static int envmap_map(const char *who, uint32_t W, uint32_t H, const float *data, bool need_data, const float *table,
                      bool need_table, const float rot[9], hf_envmap_args &a) {
    const int rc = envmap_texels(who, W, H, data, need_data, a);
    if (rc != HF_OK) return rc;
    if (need_table && !table) return fail(HF_EINVAL, "%s: NULL argument", who);
    a.table = table;
    return envmap_rot(who, rot, a);
}
// ... and of the wavefront, for the four entries that light one (hf_envmap_rays passes spp 1, num_rays k + 1, albedo 1)
static int envmap_args(const char *who, size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                       const float *t, const float *weight, uint32_t num_rays, uint32_t seed, const uint32_t *ray_id,
                       uint32_t W, uint32_t H, const float *data, const float *table, const float rot[9], float albedo,
                       hf_envmap_args &a) {
    a = {};
    int rc = light_args(who, "directions", n, spp, sh_n, d, t, weight, num_rays, seed, ray_id, false, a);
    if (rc != HF_OK) return rc;
    if (!isfinite(albedo)) return fail(HF_EINVAL, "%s: albedo must be finite", who);
    if ((rc = envmap_map(who, W, H, data, true, table, true, rot, a))) return rc;
    a.scale = (float) ((double) albedo / (3.141592653589793 * (double) num_rays));
    return HF_OK;
}

extern "C" size_t hf_envmap_table_floats(uint32_t W, uint32_t H) {
    if (W < 2 || H < 2) return 0;
    return 4 + (size_t) (H - 1) + (size_t) (H - 1) * (size_t) (W - 1);
}

extern "C" int hf_envmap_build_table(uint32_t W, uint32_t H, const float *data, float u, float *table, hf_stream_t stream) {
    const char *fn = "hf_envmap_build_table";
    hf_envmap_args a = {};
    const int rc = envmap_map(fn, W, H, data, true, table, true, nullptr, a);
    if (rc != HF_OK) return rc;
    if (!(u >= 0.f && u <= 1.f)) return fail(HF_EINVAL, "%s: the defensive fraction must lie in [0, 1] (got %g)", fn, (double) u);
    hf_launch_envmap_build(W, H, data, u, table, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_envmap_sample_direction(size_t n, const float *const sample[2], uint32_t W, uint32_t H, const float *data,
                                          const float *table, const float rot[9], float *const out_d[3], float *out_weight,
                                          float *out_pdf, uint32_t *out_cell, float *const out_frac[2],
                                          hf_stream_t stream) {
    const char *fn = "hf_envmap_sample_direction";
    hf_envmap_args a = {};
    const int rc = envmap_map(fn, W, H, data, true, table, true, rot, a);
    if (rc != HF_OK) return rc;
    if (!sample || !sample[0] || !sample[1] || !all3(out_d) || !out_weight || !out_pdf) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (out_frac && (!out_frac[0] || !out_frac[1])) return fail(HF_EINVAL, "%s: NULL out_frac component array", fn);
    if (out_frac) { a.out_frac[0] = out_frac[0]; a.out_frac[1] = out_frac[1]; }
    a.n = n; a.sample[0] = sample[0]; a.sample[1] = sample[1]; a.out_weight = out_weight; a.out_pdf = out_pdf; a.out_cell = out_cell;
    for (int c = 0; c < 3; ++c) a.out_d[c] = out_d[c];
    return light_launch(hf_launch_envmap, 4, a, stream);
}

extern "C" int hf_envmap_eval(size_t n, const float *const d[3], const uint8_t *active, uint32_t W, uint32_t H,
                              const float *data, const float rot[9], float *out, hf_stream_t stream) {
    const char *fn = "hf_envmap_eval";
    hf_envmap_args a = {};
    const int rc = envmap_map(fn, W, H, data, true, nullptr, false, rot, a);
    if (rc != HF_OK) return rc;
    if (!all3(d) || !out) return fail(HF_EINVAL, "%s: NULL argument", fn);
    a.n = n; a.active = active; a.out = out;
    for (int c = 0; c < 3; ++c) a.d[c] = d[c];
    return light_launch(hf_launch_envmap, 5, a, stream);
}

extern "C" int hf_envmap_eval_adjoint(size_t n, const float *const d[3], const uint8_t *active, uint32_t W, uint32_t H,
                                      const float rot[9], const float *grad_out, float *grad_data, hf_stream_t stream) {
    const char *fn = "hf_envmap_eval_adjoint";
    hf_envmap_args a = {};
    const int rc = envmap_map(fn, W, H, nullptr, false, nullptr, false, rot, a); // (the map is linear: its values are not read)
    if (rc != HF_OK) return rc;
    if (!grad_data) return fail(HF_EINVAL, "%s: grad_data is NULL", fn);
    if (!all3(d) || !grad_out) return fail(HF_EINVAL, "%s: NULL argument", fn);
    a.n = n; a.active = active; a.gout = grad_out; a.gdata = grad_data;
    for (int c = 0; c < 3; ++c) a.d[c] = d[c];
    return light_launch(hf_launch_envmap, 6, a, stream);
}

extern "C" int hf_envmap_rays(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                              const float *const d[3], const float *t, uint32_t k, uint32_t seed, const uint32_t *ray_id,
                              uint32_t W, uint32_t H, const float *data, const float *table, const float rot[9],
                              float *const out_o[3], float *const out_d[3], float *out_maxt, float *out_weight,
                              hf_stream_t stream) {
    const char *fn = "hf_envmap_rays";
    hf_envmap_args a;
    if (k >= 32) return fail(HF_EINVAL, "%s: direction k must be below 32 (got %u)", fn, k);
    int rc = envmap_args(fn, n, 1, sh_n, d, t, nullptr, k + 1, seed, ray_id, W, H, data, table, rot, 1.f, a);
    if (rc != HF_OK || (rc = light_rays_out(fn, p, nrm, out_o, out_d, out_maxt, a))) return rc;
    a.k = k; a.out_weight = out_weight;
    return light_launch(hf_launch_envmap, 3, a, stream);
}

extern "C" int hf_envmap_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3],
                                  const float *const nrm[3], const float *const sh_n[3], const float *const d[3],
                                  const float *t, const float *weight, uint32_t num_rays, uint32_t seed,
                                  const uint32_t *ray_id, uint32_t W, uint32_t H, const float *data, const float *table,
                                  const float rot[9], float albedo, float *image, uint32_t *vis_bits, hf_stream_t stream) {
    const char *fn = "hf_envmap_lighting";
    hf_envmap_args a;
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    int rc = envmap_args(fn, n, spp, sh_n, d, t, weight, num_rays, seed, ray_id, W, H, data, table, rot, albedo, a);
    if (rc != HF_OK || (rc = light_forward_out(fn, p, nrm, image, a))) return rc;
    if (n == 0) return HF_OK;
    if ((rc = check_device(fn, hf))) return rc;
    a.f = hf->dev; a.vis_bits = vis_bits;
    return light_launch(hf_launch_envmap, 0, a, stream);
}

extern "C" int hf_envmap_lighting_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                          const float *t, const float *weight, uint32_t num_rays, uint32_t seed,
                                          const uint32_t *ray_id, uint32_t W, uint32_t H, const float *data,
                                          const float *table, const float rot[9], float albedo, const uint32_t *vis_bits,
                                          const float *grad_image, float *const grad_sh_n[3], float *grad_weight,
                                          float *grad_data, hf_stream_t stream) {
    const char *fn = "hf_envmap_lighting_adjoint";
    hf_envmap_args a;
    const int rc = envmap_args(fn, n, spp, sh_n, d, t, weight, num_rays, seed, ray_id, W, H, data, table, rot, albedo, a);
    if (rc != HF_OK) return rc;
    if (!vis_bits || !grad_image || !all3(grad_sh_n)) return fail(HF_EINVAL, "%s: NULL argument", fn);
    a.vis_bits = const_cast<uint32_t *>(vis_bits); a.gimg = grad_image; a.gw = grad_weight; a.gdata = grad_data;
    for (int c = 0; c < 3; ++c) a.gn[c] = grad_sh_n[c];
    return light_launch(hf_launch_envmap, 1, a, stream);
}

extern "C" int hf_envmap_lighting_tangent(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                          const float *t, const float *weight, uint32_t num_rays, uint32_t seed,
                                          const uint32_t *ray_id, uint32_t W, uint32_t H, const float *data,
                                          const float *table, const float rot[9], float albedo, const uint32_t *vis_bits,
                                          const float *const dsh_n[3], const float *dweight, const float *ddata,
                                          float *dimage, hf_stream_t stream) {
    const char *fn = "hf_envmap_lighting_tangent";
    hf_envmap_args a;
    int rc = envmap_args(fn, n, spp, sh_n, d, t, weight, num_rays, seed, ray_id, W, H, data, table, rot, albedo, a);
    if (rc != HF_OK || (rc = light_tangent_io(fn, !vis_bits, dsh_n, dweight, dimage, a))) return rc;
    a.vis_bits = const_cast<uint32_t *>(vis_bits); a.ddata = ddata;
    return light_launch(hf_launch_envmap, 2, a, stream);
}

// ---- specular reflection of the environment map: the mirror ray walked in the kernel, the map looked up ----
// What the hf_reflect_* entries share: the wavefront rows (`a` is zeroed here) ...
static int reflect_rows(const char *who, size_t n, const float *const sh_n[3], const float *const d[3], const float *t,
                        const uint8_t *active, hf_reflect_args &a) {
    a = {};
    if (!all3(sh_n) || !all3(d) || !t) return fail(HF_EINVAL, "%s: NULL argument", who);
    if (n >= ((size_t) 1 << 32)) return fail(HF_EINVAL, "%s: more than 2^32 samples", who);
    a.n = n; a.spp = 1; a.t = t; a.active = active;
    for (int c = 0; c < 3; ++c) { a.sh_n[c] = sh_n[c]; a.d[c] = d[c]; }
    return HF_OK;
}
// the map and the interface of a reflection row (glossy too), checked in the order 2 x 2, eta, rot (a NULL data: the caller's check)
template <class A>
static int reflect_map(const char *who, float eta, uint32_t W, uint32_t H, const float *data, const float rot[9], A &a) {
    int rc = envmap_texels(who, W, H, data, true, a);
    if (rc != HF_OK || (rc = light_interface(who, eta, a))) return rc;
    return envmap_rot(who, rot, a);
}
// ... and the film, the interface and the map of the three lighting entries
static int reflect_args(const char *who, size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                        const float *t, const uint8_t *active, const float *weight, float eta, uint32_t W, uint32_t H,
                        const float *data, const float rot[9], hf_reflect_args &a) {
    const int rc = reflect_rows(who, n, sh_n, d, t, active, a);
    if (rc != HF_OK) return rc;
    if (!data) return fail(HF_EINVAL, "%s: NULL argument", who);
    if (spp == 0 || n % spp != 0) return fail(HF_EINVAL, "%s: n (%zu) must be a multiple of spp (%u)", who, n, spp);
    a.spp = spp; a.weight = weight;
    return reflect_map(who, eta, W, H, data, rot, a);
}

extern "C" int hf_reflect_rays(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                               const float *const d[3], const float *t, const uint8_t *active, float *const out_o[3],
                               float *const out_d[3], float *out_maxt, hf_stream_t stream) {
    const char *fn = "hf_reflect_rays";
    hf_reflect_args a;
    int rc = reflect_rows(fn, n, sh_n, d, t, active, a);
    if (rc != HF_OK || (rc = light_rays_out(fn, p, nrm, out_o, out_d, out_maxt, a))) return rc;
    a.eta = 1.f; a.rcp_eta = 1.f; // (the direction does not depend on the interface)
    return light_launch(hf_launch_reflect, 3, a, stream);
}

extern "C" int hf_reflect_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3],
                                   const float *const nrm[3], const float *const sh_n[3], const float *const d[3],
                                   const float *t, const uint8_t *active, const float *weight, float eta, uint32_t W,
                                   uint32_t H, const float *data, const float rot[9], float *image, float *value,
                                   uint8_t *vis, hf_stream_t stream) {
    const char *fn = "hf_reflect_lighting";
    hf_reflect_args a;
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    int rc = reflect_args(fn, n, spp, sh_n, d, t, active, weight, eta, W, H, data, rot, a);
    if (rc != HF_OK || (rc = light_value_forward_out(fn, p, nrm, image, value, !vis, "vis", a))) return rc;
    if (n == 0) return HF_OK;
    if ((rc = check_device(fn, hf))) return rc;
    a.f = hf->dev; a.vis = vis;
    return light_launch(hf_launch_reflect, 0, a, stream);
}

extern "C" int hf_reflect_lighting_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                           const float *t, const uint8_t *active, const float *weight, float eta,
                                           uint32_t W, uint32_t H, const float *data, const float rot[9], const uint8_t *vis,
                                           const float *grad_image, const float *grad_value, float *const grad_sh_n[3],
                                           float *grad_weight, float *grad_data, hf_stream_t stream) {
    const char *fn = "hf_reflect_lighting_adjoint";
    hf_reflect_args a;
    int rc = reflect_args(fn, n, spp, sh_n, d, t, active, weight, eta, W, H, data, rot, a);
    if (rc != HF_OK || (rc = light_value_adjoint_io(fn, !vis, grad_image, grad_value, grad_sh_n, grad_weight, grad_data, a))) return rc;
    a.vis = const_cast<uint8_t *>(vis);
    return light_launch(hf_launch_reflect, 1, a, stream);
}

extern "C" int hf_reflect_lighting_tangent(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                           const float *t, const uint8_t *active, const float *weight, float eta,
                                           uint32_t W, uint32_t H, const float *data, const float rot[9], const uint8_t *vis,
                                           const float *const dsh_n[3], const float *dweight, const float *ddata,
                                           float *dimage, float *dvalue, hf_stream_t stream) {
    const char *fn = "hf_reflect_lighting_tangent";
    hf_reflect_args a;
    int rc = reflect_args(fn, n, spp, sh_n, d, t, active, weight, eta, W, H, data, rot, a);
    if (rc != HF_OK || (rc = light_value_tangent_io(fn, !vis, dsh_n, dweight, ddata, dimage, dvalue, a))) return rc;
    a.vis = const_cast<uint8_t *>(vis);
    return light_launch(hf_launch_reflect, 2, a, stream);
}

// ---- glossy reflection of the environment map: a GGX lobe, K mirror rays per sample walked in the kernel ----
// What the hf_glossy_* entries share: the wavefront rows and the sample stream (`a` is zeroed here; hf_glossy_rays passes
// spp 1 and num_rays k + 1) ...
static int glossy_rows(const char *who, size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                       const float *t, const uint8_t *active, const float *alpha, uint32_t num_rays, uint32_t seed,
                       const uint32_t *ray_id, hf_glossy_args &a) {
    a = {};
    const int rc = light_args(who, "mirror rays", n, spp, sh_n, d, t, nullptr, num_rays, seed, ray_id, !alpha, a);
    if (rc != HF_OK) return rc;
    a.active = active; a.alpha = alpha; a.inv_k = 1.f / (float) num_rays;
    return HF_OK;
}
// ... and the interface and the map of the three lighting entries
static int glossy_args(const char *who, size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                       const float *t, const uint8_t *active, const float *weight, const float *alpha, float eta,
                       uint32_t num_rays, uint32_t seed, const uint32_t *ray_id, uint32_t W, uint32_t H, const float *data,
                       const float rot[9], hf_glossy_args &a) {
    const int rc = glossy_rows(who, n, spp, sh_n, d, t, active, alpha, num_rays, seed, ray_id, a);
    if (rc != HF_OK) return rc;
    if (!data) return fail(HF_EINVAL, "%s: NULL argument", who);
    a.weight = weight;
    return reflect_map(who, eta, W, H, data, rot, a);
}

extern "C" int hf_glossy_rays(size_t n, const float *const p[3], const float *const nrm[3], const float *const sh_n[3],
                              const float *const d[3], const float *t, const uint8_t *active, const float *alpha, uint32_t k,
                              uint32_t seed, const uint32_t *ray_id, float *const out_o[3], float *const out_d[3],
                              float *out_maxt, float *const out_h[3], hf_stream_t stream) {
    const char *fn = "hf_glossy_rays";
    hf_glossy_args a;
    if (k >= 32) return fail(HF_EINVAL, "%s: direction k must be below 32 (got %u)", fn, k);
    int rc = glossy_rows(fn, n, 1, sh_n, d, t, active, alpha, k + 1, seed, ray_id, a);
    if (rc != HF_OK || (rc = light_rays_out(fn, p, nrm, out_o, out_d, out_maxt, a))) return rc;
    if (out_h && !all3(out_h)) return fail(HF_EINVAL, "%s: NULL out_h component array", fn);
    a.k = k; a.eta = 1.f; a.rcp_eta = 1.f; // (the direction does not depend on the interface)
    for (int c = 0; c < 3; ++c) a.out_h[c] = out_h ? out_h[c] : nullptr;
    return light_launch(hf_launch_glossy, 3, a, stream);
}

extern "C" int hf_glossy_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3],
                                  const float *const nrm[3], const float *const sh_n[3], const float *const d[3],
                                  const float *t, const uint8_t *active, const float *weight, const float *alpha, float eta,
                                  uint32_t num_rays, uint32_t seed, const uint32_t *ray_id, uint32_t W, uint32_t H,
                                  const float *data, const float rot[9], float *image, float *value, uint32_t *vis_bits,
                                  hf_stream_t stream) {
    const char *fn = "hf_glossy_lighting";
    hf_glossy_args a;
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    int rc = glossy_args(fn, n, spp, sh_n, d, t, active, weight, alpha, eta, num_rays, seed, ray_id, W, H, data, rot, a);
    if (rc != HF_OK || (rc = light_value_forward_out(fn, p, nrm, image, value, !vis_bits, "vis_bits", a))) return rc;
    if (n == 0) return HF_OK;
    if ((rc = check_device(fn, hf))) return rc;
    a.f = hf->dev; a.vis_bits = vis_bits;
    return light_launch(hf_launch_glossy, 0, a, stream);
}

extern "C" int hf_glossy_lighting_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                          const float *t, const uint8_t *active, const float *weight, const float *alpha,
                                          float eta, uint32_t num_rays, uint32_t seed, const uint32_t *ray_id, uint32_t W,
                                          uint32_t H, const float *data, const float rot[9], const uint32_t *vis_bits,
                                          const float *grad_image, const float *grad_value, float *const grad_sh_n[3],
                                          float *grad_weight, float *grad_alpha, float *grad_data, hf_stream_t stream) {
    const char *fn = "hf_glossy_lighting_adjoint";
    hf_glossy_args a;
    int rc = glossy_args(fn, n, spp, sh_n, d, t, active, weight, alpha, eta, num_rays, seed, ray_id, W, H, data, rot, a);
    if (rc != HF_OK || (rc = light_value_adjoint_io(fn, !vis_bits, grad_image, grad_value, grad_sh_n, grad_weight, grad_data, a))) return rc;
    a.vis_bits = const_cast<uint32_t *>(vis_bits); a.ga = grad_alpha;
    return light_launch(hf_launch_glossy, 1, a, stream);
}

extern "C" int hf_glossy_lighting_tangent(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                                          const float *t, const uint8_t *active, const float *weight, const float *alpha,
                                          float eta, uint32_t num_rays, uint32_t seed, const uint32_t *ray_id, uint32_t W,
                                          uint32_t H, const float *data, const float rot[9], const uint32_t *vis_bits,
                                          const float *const dsh_n[3], const float *dweight, const float *dalpha,
                                          const float *ddata, float *dimage, float *dvalue, hf_stream_t stream) {
    const char *fn = "hf_glossy_lighting_tangent";
    hf_glossy_args a;
    int rc = glossy_args(fn, n, spp, sh_n, d, t, active, weight, alpha, eta, num_rays, seed, ray_id, W, H, data, rot, a);
    if (rc != HF_OK || (rc = light_value_tangent_io(fn, !vis_bits, dsh_n, dweight, ddata, dimage, dvalue, a))) return rc;
    a.vis_bits = const_cast<uint32_t *>(vis_bits); a.da = dalpha;
    return light_launch(hf_launch_glossy, 2, a, stream);
}

// ---- bounce lighting: one diffuse interreflection, both rays traced inside the lighting kernel ----
// What the four hf_bounce_* entries share.  hf_bounce_rays passes spp 1, num_rays k + 1, albedo 1 and either no light or its one direction.
static int bounce_args(const char *who, const hf_field_t *hf, size_t n, uint32_t spp, const float *const sh_n[3],
                       const float *const d[3], const float *t, const float *weight, uint32_t num_rays, uint32_t seed,
                       const uint32_t *ray_id, uint32_t n_lights, const hf_dir_light_t *lights, float albedo,
                       hf_bounce_args &a) {
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", who);
    a = {};
    const int rc = light_args(who, "bounce directions", n, spp, sh_n, d, t, weight, num_rays, seed, ray_id, !lights, a);
    if (rc != HF_OK) return rc;
    if (n_lights == 0 || n_lights > HF_MAX_LIGHTS)
        return fail(HF_EINVAL, "%s: 1..%d lights supported (got %u)", who, HF_MAX_LIGHTS, n_lights);
    if (!isfinite(albedo)) return fail(HF_EINVAL, "%s: albedo must be finite", who);
    for (uint32_t l = 0; l < n_lights; ++l) {
        if (!isfinite(lights[l].irradiance) || !isfinite(lights[l].to_light[0]) || !isfinite(lights[l].to_light[1]) ||
            !isfinite(lights[l].to_light[2]))
            return fail(HF_EINVAL, "%s: light %u is not finite", who, l);
        for (int c = 0; c < 3; ++c) a.l[l][c] = lights[l].to_light[c];
        a.w[l] = (albedo * 0.31830988618379067154f) * lights[l].irradiance; // dr::InvPi
    }
    a.n_lights = n_lights;
    a.scale = albedo / (float) num_rays; // the BSDF weight (cosine and pdf cancel), averaged over num_rays
    return HF_OK;
}
// the record of the three lighting entries (need: the adjoint and the tangent read it)
static int bounce_record(const char *who, size_t n, const uint32_t *hit_prim, const uint8_t *lit_bits, size_t sample_stride,
                         bool need, hf_bounce_args &a) {
    if (need && (!hit_prim || !lit_bits)) return fail(HF_EINVAL, "%s: NULL record", who);
    if ((hit_prim || lit_bits) && sample_stride < n)
        return fail(HF_EINVAL, "%s: sample_stride (%zu) below n (%zu)", who, sample_stride, n);
    a.hit_prim = const_cast<uint32_t *>(hit_prim); a.lit_bits = const_cast<uint8_t *>(lit_bits); a.sample_stride = sample_stride;
    return HF_OK;
}

extern "C" int hf_bounce_rays(const hf_field_t *hf, size_t n, const float *const p[3], const float *const nrm[3],
                              const float *const sh_n[3], const float *const d[3], const float *t, uint32_t k,
                              uint32_t seed, const uint32_t *ray_id, const float *to_light, float *const out_o[3],
                              float *const out_d[3], float *out_maxt, hf_stream_t stream) {
    const char *fn = "hf_bounce_rays";
    hf_bounce_args a;
    if (k >= 32) return fail(HF_EINVAL, "%s: direction k must be below 32 (got %u)", fn, k);
    hf_dir_light_t one = { { 0.f, 0.f, 1.f }, 1.f };
    if (to_light) for (int c = 0; c < 3; ++c) one.to_light[c] = to_light[c];
    int rc = bounce_args(fn, hf, n, 1, sh_n, d, t, nullptr, k + 1, seed, ray_id, 1, &one, 1.f, a);
    if (rc != HF_OK || (rc = light_rays_out(fn, p, nrm, out_o, out_d, out_maxt, a))) return rc;
    if (n == 0) return HF_OK;
    if ((rc = check_device(fn, hf))) return rc;
    a.f = hf->dev; a.k = k; a.shadow = to_light ? 1 : 0;
    return light_launch(hf_launch_bounce, 3, a, stream);
}

extern "C" int hf_bounce_lighting(const hf_field_t *hf, size_t n, uint32_t spp, const float *const p[3],
                                  const float *const nrm[3], const float *const sh_n[3], const float *const d[3],
                                  const float *t, const float *weight, uint32_t num_rays, uint32_t seed,
                                  const uint32_t *ray_id, uint32_t n_lights, const hf_dir_light_t *lights, float albedo,
                                  float *image, uint32_t *hit_prim, uint8_t *lit_bits, size_t sample_stride,
                                  hf_stream_t stream) {
    const char *fn = "hf_bounce_lighting";
    hf_bounce_args a;
    int rc = bounce_args(fn, hf, n, spp, sh_n, d, t, weight, num_rays, seed, ray_id, n_lights, lights, albedo, a);
    if (rc != HF_OK || (rc = light_forward_out(fn, p, nrm, image, a))) return rc;
    if ((rc = bounce_record(fn, n, hit_prim, lit_bits, sample_stride, false, a))) return rc;
    if (n == 0) return HF_OK;
    if ((rc = check_device(fn, hf))) return rc;
    a.f = hf->dev;
    return light_launch(hf_launch_bounce, 0, a, stream);
}

extern "C" int hf_bounce_lighting_adjoint(const hf_field_t *hf, size_t n, uint32_t spp, const float *const sh_n[3],
                                          const float *const d[3], const float *t, const float *weight,
                                          uint32_t num_rays, uint32_t seed, const uint32_t *ray_id, uint32_t n_lights,
                                          const hf_dir_light_t *lights, float albedo, const uint32_t *hit_prim,
                                          const uint8_t *lit_bits, size_t sample_stride, const float *grad_image,
                                          float *const grad_sh_n[3], float *grad_weight, float *grad_heights,
                                          hf_stream_t stream) {
    const char *fn = "hf_bounce_lighting_adjoint";
    hf_bounce_args a;
    int rc = bounce_args(fn, hf, n, spp, sh_n, d, t, weight, num_rays, seed, ray_id, n_lights, lights, albedo, a);
    if (rc != HF_OK) return rc;
    if (!grad_image) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (grad_sh_n && !all3(grad_sh_n)) return fail(HF_EINVAL, "%s: NULL grad_sh_n component array", fn);
    if (!grad_sh_n && !grad_weight && !grad_heights) return fail(HF_EINVAL, "%s: no output", fn);
    if ((rc = bounce_record(fn, n, hit_prim, lit_bits, sample_stride, true, a))) return rc;
    if (n == 0) return HF_OK;
    if ((rc = check_device(fn, hf))) return rc;
    a.f = hf->dev; a.gimg = grad_image; a.gw = grad_weight; a.gh = grad_heights;
    for (int c = 0; c < 3; ++c) a.gn[c] = grad_sh_n ? grad_sh_n[c] : nullptr;
    return light_launch(hf_launch_bounce, 1, a, stream);
}

extern "C" int hf_bounce_lighting_tangent(const hf_field_t *hf, size_t n, uint32_t spp, const float *const sh_n[3],
                                          const float *const d[3], const float *t, const float *weight,
                                          uint32_t num_rays, uint32_t seed, const uint32_t *ray_id, uint32_t n_lights,
                                          const hf_dir_light_t *lights, float albedo, const uint32_t *hit_prim,
                                          const uint8_t *lit_bits, size_t sample_stride, const float *const dsh_n[3],
                                          const float *dweight, const float *dheights, float *dimage,
                                          hf_stream_t stream) {
    const char *fn = "hf_bounce_lighting_tangent";
    hf_bounce_args a;
    int rc = bounce_args(fn, hf, n, spp, sh_n, d, t, weight, num_rays, seed, ray_id, n_lights, lights, albedo, a);
    if (rc != HF_OK || (rc = light_tangent_io(fn, false, dsh_n, dweight, dimage, a))) return rc;
    if ((rc = bounce_record(fn, n, hit_prim, lit_bits, sample_stride, true, a))) return rc;
    if (n == 0) return HF_OK;
    if ((rc = check_device(fn, hf))) return rc;
    a.f = hf->dev; a.dh = dheights;
    return light_launch(hf_launch_bounce, 2, a, stream);
}

// ---- Gaussian reconstruction filter (film) ------------------------------------------------------
static int splat_args(const char *who, size_t n, uint32_t channels, const float *pos_x, const float *pos_y,
                      uint32_t width, uint32_t height, float stddev, hf_splat_args &a) {
    if (!pos_x || !pos_y) return fail(HF_EINVAL, "%s: NULL film positions", who);
    if (channels == 0 || channels > HF_MAX_LIGHTS) return fail(HF_EINVAL, "%s: 1..%d channels (got %u)", who, HF_MAX_LIGHTS, channels);
    if (width == 0 || height == 0 || (size_t) width * height >= ((size_t) 1 << 31)) return fail(HF_EINVAL, "%s: bad film size", who);
    if (!(stddev > 0.f) || stddev > 1.f) return fail(HF_EINVAL, "%s: stddev must be in (0, 1] pixels", who);
    if (n >= ((size_t) 1 << 32)) return fail(HF_EINVAL, "%s: more than 2^32 samples", who);
    a = {};
    a.n = n; a.channels = channels; a.width = width; a.height = height; a.pos_x = pos_x; a.pos_y = pos_y;
    a.radius = 4.f * stddev;                               // gaussian.cpp:52-53
    a.alpha = -1.f / (2.f * stddev * stddev);              // gaussian.cpp:97-99
    a.bias = expf(a.alpha * a.radius * a.radius);
    return HF_OK;
}

extern "C" int hf_film_splat(size_t n, uint32_t channels, const float *const *values, const float *pos_x,
                             const float *pos_y, uint32_t width, uint32_t height, float stddev, float *image,
                             float *weight, hf_stream_t stream) {
    hf_splat_args a;
    const int rc = splat_args("hf_film_splat", n, channels, pos_x, pos_y, width, height, stddev, a);
    if (rc != HF_OK) return rc;
    if (!values || !image || !weight) return fail(HF_EINVAL, "hf_film_splat: NULL argument");
    for (uint32_t k = 0; k < channels; ++k) {
        if (!values[k]) return fail(HF_EINVAL, "hf_film_splat: NULL channel array");
        a.values[k] = values[k];
    }
    a.image = image; a.weight = weight;
    hf_launch_film_splat(a, false, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_film_splat_adjoint(size_t n, uint32_t channels, const float *pos_x, const float *pos_y,
                                     uint32_t width, uint32_t height, float stddev, const float *grad_image,
                                     float *const *grad_values, hf_stream_t stream) {
    hf_splat_args a;
    const int rc = splat_args("hf_film_splat_adjoint", n, channels, pos_x, pos_y, width, height, stddev, a);
    if (rc != HF_OK) return rc;
    if (!grad_image || !grad_values) return fail(HF_EINVAL, "hf_film_splat_adjoint: NULL argument");
    for (uint32_t k = 0; k < channels; ++k) {
        if (!grad_values[k]) return fail(HF_EINVAL, "hf_film_splat_adjoint: NULL channel array");
        a.grad_values[k] = grad_values[k];
    }
    a.grad_image = grad_image;
    hf_launch_film_splat(a, true, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

// ---- the same film, differentiable in the sample positions, with a per-sample weight ----------------
// rows[0 .. channels) of an optional array of channel rows into out; a NULL row of a given array is refused
template <class T>
static int channel_rows(const char *who, uint32_t channels, T *const *rows, T **out) {
    for (uint32_t k = 0; rows && k < channels; ++k) {
        if (!rows[k]) return fail(HF_EINVAL, "%s: NULL channel array", who);
        out[k] = rows[k];
    }
    return HF_OK;
}

extern "C" int hf_film_splat_weighted(size_t n, uint32_t channels, const float *const *values, const float *sample_weight,
                                      const float *pos_x, const float *pos_y, uint32_t width, uint32_t height,
                                      float stddev, float *image, float *weight, hf_stream_t stream) {
    static const char *who = "hf_film_splat_weighted";
    hf_film_motion_args a = {};
    int rc = splat_args(who, n, channels, pos_x, pos_y, width, height, stddev, a.s);
    if (rc != HF_OK) return rc;
    if (!values || !image || !weight) return fail(HF_EINVAL, "%s: NULL argument", who);
    if ((rc = channel_rows(who, channels, values, a.s.values)) != HF_OK) return rc;
    a.sample_weight = sample_weight; a.s.image = image; a.s.weight = weight;
    hf_launch_film_motion(0, a, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_film_splat_weighted_adjoint(size_t n, uint32_t channels, const float *const *values,
                                              const float *sample_weight, const float *pos_x, const float *pos_y,
                                              uint32_t width, uint32_t height, float stddev, const float *grad_image,
                                              const float *grad_weight, float *const *grad_values,
                                              float *grad_sample_weight, float *grad_pos_x, float *grad_pos_y,
                                              hf_stream_t stream) {
    static const char *who = "hf_film_splat_weighted_adjoint";
    hf_film_motion_args a = {};
    int rc = splat_args(who, n, channels, pos_x, pos_y, width, height, stddev, a.s);
    if (rc != HF_OK) return rc;
    if (!grad_image) return fail(HF_EINVAL, "%s: NULL argument", who);
    if (!grad_values && !grad_sample_weight && !grad_pos_x && !grad_pos_y) return fail(HF_EINVAL, "%s: no output", who);
    if ((grad_pos_x || grad_pos_y) && !values) return fail(HF_EINVAL, "%s: a position gradient needs the values", who);
    if ((rc = channel_rows(who, channels, values, a.s.values)) != HF_OK) return rc;
    if ((rc = channel_rows(who, channels, grad_values, a.s.grad_values)) != HF_OK) return rc;
    a.sample_weight = sample_weight; a.s.grad_image = grad_image; a.grad_weight = grad_weight;
    a.grad_sample_weight = grad_sample_weight; a.grad_pos_x = grad_pos_x; a.grad_pos_y = grad_pos_y;
    hf_launch_film_motion(1, a, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_film_splat_weighted_tangent(size_t n, uint32_t channels, const float *const *values,
                                              const float *sample_weight, const float *pos_x, const float *pos_y,
                                              uint32_t width, uint32_t height, float stddev, const float *const *dvalues,
                                              const float *dsample_weight, const float *dpos_x, const float *dpos_y,
                                              float *dimage, float *dweight, hf_stream_t stream) {
    static const char *who = "hf_film_splat_weighted_tangent";
    hf_film_motion_args a = {};
    int rc = splat_args(who, n, channels, pos_x, pos_y, width, height, stddev, a.s);
    if (rc != HF_OK) return rc;
    if (!values || !dimage || !dweight) return fail(HF_EINVAL, "%s: NULL argument", who);
    if ((rc = channel_rows(who, channels, values, a.s.values)) != HF_OK) return rc;
    if ((rc = channel_rows(who, channels, dvalues, a.dvalues)) != HF_OK) return rc;
    a.sample_weight = sample_weight; a.dsample_weight = dsample_weight; a.dpos_x = dpos_x; a.dpos_y = dpos_y;
    a.s.image = dimage; a.s.weight = dweight;
    hf_launch_film_motion(2, a, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

// ---- warped-area reparameterisation --------------------------------------------

extern "C" int hf_reparam_aux_rays(size_t n, const float *const o[3], const float *const d[3], const uint8_t *active,
                                   uint32_t k, float kappa, int antithetic, uint32_t seed, const uint32_t *ray_id,
                                   float *const aux_d[3], float *aux_maxt, hf_stream_t stream) {
    if (!all3(o) || !all3(d) || !all3(aux_d) || !aux_maxt)
        return fail(HF_EINVAL, "hf_reparam_aux_rays: NULL argument");
    if (!(kappa > 0.f)) return fail(HF_EINVAL, "hf_reparam_aux_rays: kappa must be > 0");
    if (n >= ((size_t) 1 << 32)) return fail(HF_EINVAL, "hf_reparam_aux_rays: more than 2^32 rays");
    hf_reparam_args a = {};
    a.n = n; a.active = active; a.k = k; a.seed = seed; a.kappa = kappa; a.antithetic = antithetic; a.ray_id = ray_id;
    for (int c = 0; c < 3; ++c) { a.o[c] = o[c]; a.d[c] = d[c]; a.aux_d[c] = aux_d[c]; }
    a.aux_maxt = aux_maxt;
    hf_launch_reparam_aux(a, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_reparam_weights(int mode, size_t n, const float *const o[3], const float *const d[3],
                                  const uint8_t *active, uint32_t k, float kappa, float exponent, int antithetic,
                                  uint32_t seed, const uint32_t *ray_id, const float *si_t, const float *const si_p[3],
                                  const float *si_boundary_test, float *Z, float *const dZ[3],
                                  const float *const grad_direction[3], const float *grad_divergence,
                                  float *const grad_p[3], float *grad_t, float *const grad_vd[3],
                                  hf_stream_t stream) {
    if (!all3(o) || !all3(d) || !si_t || !si_boundary_test || !Z || !all3(dZ))
        return fail(HF_EINVAL, "hf_reparam_weights: NULL argument");
    if (mode != 0 && mode != 1) return fail(HF_EINVAL, "hf_reparam_weights: mode must be 0 or 1");
    if (mode == 1 && (!all3(si_p) || !all3(grad_direction) || !grad_divergence || !all3(grad_p) || !grad_t))
        return fail(HF_EINVAL, "hf_reparam_weights: mode 1 needs si_p, grad_direction, grad_divergence, grad_p, grad_t");
    if (!(kappa > 0.f)) return fail(HF_EINVAL, "hf_reparam_weights: kappa must be > 0");
    if (n >= ((size_t) 1 << 32)) return fail(HF_EINVAL, "hf_reparam_weights: more than 2^32 rays");
    hf_reparam_args a = {};
    a.n = n; a.active = active; a.k = k; a.seed = seed; a.kappa = kappa; a.exponent = exponent;
    a.antithetic = antithetic; a.mode = mode; a.ray_id = ray_id;
    a.si_t = si_t; a.si_bt = si_boundary_test; a.Z = Z; a.g_div = grad_divergence; a.g_t = grad_t;
    for (int c = 0; c < 3; ++c) {
        a.o[c] = o[c]; a.d[c] = d[c]; a.dZ[c] = dZ[c];
        a.si_p[c] = si_p ? si_p[c] : nullptr;
        a.g_dir[c] = grad_direction ? grad_direction[c] : nullptr;
        a.g_p[c] = grad_p ? grad_p[c] : nullptr;
        a.g_vd[c] = all3(grad_vd) ? grad_vd[c] : nullptr;
    }
    hf_launch_reparam_weights(a, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

// Which instantiation traces auxiliary rays: the lean one (every wave walks per lane) when the handle is set to
// incoherent rays, and in the automatic mode when kappa is below HF_AUX_LEAN_KAPPA -- the reference traces its auxiliary
// rays with coherent = false (reparam.py:95), and on the bench wavefront (camera 2.6 units from the terrain, cells of
// 1/2048 unit) the lean kernel wins up to kappa = 1.6e6 (15.7 vs 16.5 ms), ties at 6.4e6 and loses beyond (1e8, where the
// auxiliary rays are the primary ray: 13.9 vs 11.1 ms; profiles/r04_ab/r04_lean).
#ifndef HF_AUX_LEAN_KAPPA
#define HF_AUX_LEAN_KAPPA 4e6f
#endif
static bool aux_lean(const hf_field_t *hf, float kappa) {
    if (hf->coherence == HF_COHERENCE_INCOHERENT) return true;
    if (hf->coherence == HF_COHERENCE_COHERENT) return false;
    return kappa < HF_AUX_LEAN_KAPPA;
}

extern "C" int hf_set_ray_coherence(hf_field_t *hf, int coherence) {
    if (!hf) return fail(HF_EINVAL, "hf_set_ray_coherence: NULL handle");
    if (coherence != HF_COHERENCE_AUTO && coherence != HF_COHERENCE_INCOHERENT && coherence != HF_COHERENCE_COHERENT)
        return fail(HF_EINVAL, "hf_set_ray_coherence: unknown mode %d", coherence);
    hf->coherence = coherence;
    return HF_OK;
}
extern "C" int hf_get_ray_coherence(const hf_field_t *hf) { return hf ? hf->coherence : HF_COHERENCE_AUTO; }

// hf_reparam_trace (all = false: sample k) and hf_reparam_trace_all (all: samples 0 .. num - 1, stride apart)
static int reparam_trace(const char *fn, bool all, const hf_field_t *hf, size_t n, const float *const o[3],
                         const float *const d[3], const uint8_t *active, uint32_t k, uint32_t num, size_t stride,
                         float kappa, int antithetic, uint32_t seed, const uint32_t *ray_id, const hf_pi_t *out_pi,
                         const hf_si_t *out_si, hipStream_t stream) {
    if (!all3(o) || !all3(d)) return fail(HF_EINVAL, "%s: NULL argument", fn);
    hf_rays_t rays; // maxt is not read for auxiliary rays (infinity); any readable array of n floats will do
    for (int c = 0; c < 3; ++c) { rays.o[c] = o[c]; rays.d[c] = d[c]; }
    rays.maxt = o[0];
    int rc = check_rays(fn, hf, n, &rays);
    if (rc) return rc;
    if (!out_si) return fail(HF_EINVAL, "%s: NULL output", fn);
    if (!(kappa > 0.f)) return fail(HF_EINVAL, "%s: kappa must be > 0", fn);
    if (all && (num == 0 || num > 32)) return fail(HF_EINVAL, "%s: 1..32 auxiliary rays per ray (got %u)", fn, num);
    if (all && num > 1 && stride < n) return fail(HF_EINVAL, "%s: sample_stride < n", fn);
    if (n >= ((size_t) 1 << 32)) return fail(HF_EINVAL, "%s: more than 2^32 rays", fn);
    hf_reparam_args a = {};
    a.k = k; a.num = num; a.stride = stride; a.seed = seed; a.kappa = kappa; a.antithetic = antithetic; a.ray_id = ray_id;
    return trace("trace launch", 2, hf, n, &rays, active, out_pi, nullptr, out_si,
                 HF_RAY_ALL | HF_RAY_FOLLOWSHAPE | HF_RAY_BOUNDARYTEST, stream, &a, aux_lean(hf, kappa));
}

extern "C" int hf_reparam_trace(const hf_field_t *hf, size_t n, const float *const o[3], const float *const d[3],
                                const uint8_t *active, uint32_t k, float kappa, int antithetic, uint32_t seed,
                                const uint32_t *ray_id, const hf_pi_t *out_pi, const hf_si_t *out_si, hf_stream_t stream) {
    return reparam_trace("hf_reparam_trace", false, hf, n, o, d, active, k, 0, 0, kappa, antithetic, seed, ray_id, out_pi,
                         out_si, (hipStream_t) stream);
}

extern "C" int hf_reparam_trace_all(const hf_field_t *hf, size_t n, const float *const o[3], const float *const d[3],
                                    const uint8_t *active, uint32_t num_rays, float kappa, int antithetic, uint32_t seed,
                                    const uint32_t *ray_id, const hf_pi_t *out_pi, const hf_si_t *out_si, size_t sample_stride,
                                    hf_stream_t stream) {
    return reparam_trace("hf_reparam_trace_all", true, hf, n, o, d, active, 0, num_rays, sample_stride, kappa, antithetic,
                         seed, ray_id, out_pi, out_si, (hipStream_t) stream);
}

extern "C" int hf_reparam_backward(const hf_field_t *hf, size_t n, const float *const o[3], const float *const d[3],
                                   const uint8_t *active, uint32_t num_rays, float kappa, float exponent,
                                   int antithetic, uint32_t seed, const uint32_t *ray_id, const hf_pi_const_t *pi,
                                   const float *si_boundary_test, size_t sample_stride,
                                   const float *const grad_direction[3], const float *grad_divergence,
                                   float *grad_heights, hf_stream_t stream) {
    if (!hf) return fail(HF_EINVAL, "hf_reparam_backward: NULL handle");
    if (!all3(o) || !all3(d) || !si_boundary_test || !all3(grad_direction) || !grad_divergence || !grad_heights)
        return fail(HF_EINVAL, "hf_reparam_backward: NULL argument");
    int rc = check_pi("hf_reparam_backward", n, pi);
    if (rc) return rc;
    if (!(kappa > 0.f)) return fail(HF_EINVAL, "hf_reparam_backward: kappa must be > 0");
    if (num_rays == 0 || num_rays > 32) return fail(HF_EINVAL, "hf_reparam_backward: 1..32 auxiliary rays per ray (got %u)", num_rays);
    if (num_rays > 1 && sample_stride < n) return fail(HF_EINVAL, "hf_reparam_backward: sample_stride < n");
    if (n >= ((size_t) 1 << 32)) return fail(HF_EINVAL, "hf_reparam_backward: more than 2^32 rays");
    if ((rc = check_device("hf_reparam_backward", hf))) return rc;
    hf_reparam_args a = {};
    a.n = n; a.active = active; a.seed = seed; a.kappa = kappa; a.exponent = exponent; a.antithetic = antithetic;
    a.ray_id = ray_id;
    a.si_bt = si_boundary_test; a.g_div = grad_divergence;
    for (int c = 0; c < 3; ++c) { a.o[c] = o[c]; a.d[c] = d[c]; a.g_dir[c] = grad_direction[c]; }
    hf_launch_reparam_backward(hf->dev, a, num_rays, sample_stride, pi, grad_heights, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_reparam_tangent(const hf_field_t *hf, size_t n, const float *const o[3], const float *const d[3],
                                  const uint8_t *active, uint32_t num_rays, float kappa, float exponent, int antithetic,
                                  uint32_t seed, const uint32_t *ray_id, const hf_pi_const_t *pi,
                                  const float *si_boundary_test, size_t sample_stride, const float *dheights,
                                  const float *const d_o[3], const float *const d_d[3], const float *d_to_world,
                                  float *const out_direction[3], float *out_divergence, hf_stream_t stream) {
    const char *fn = "hf_reparam_tangent";
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    if (!all3(o) || !all3(d) || !si_boundary_test || !all3(out_direction) || !out_divergence)
        return fail(HF_EINVAL, "%s: NULL argument", fn);
    int rc = check_pi(fn, n, pi);
    if (rc) return rc;
    if (!(kappa > 0.f)) return fail(HF_EINVAL, "%s: kappa must be > 0", fn);
    if (num_rays == 0 || num_rays > 32) return fail(HF_EINVAL, "%s: 1..32 auxiliary rays per ray (got %u)", fn, num_rays);
    if (num_rays > 1 && sample_stride < n) return fail(HF_EINVAL, "%s: sample_stride < n", fn);
    if (n >= ((size_t) 1 << 32)) return fail(HF_EINVAL, "%s: more than 2^32 rays", fn);
    if ((rc = check_device(fn, hf))) return rc;
    hf_reparam_args a = {};
    a.n = n; a.active = active; a.seed = seed; a.kappa = kappa; a.exponent = exponent; a.antithetic = antithetic;
    a.ray_id = ray_id; a.si_bt = si_boundary_test;
    for (int c = 0; c < 3; ++c) { a.o[c] = o[c]; a.d[c] = d[c]; }
    hf_launch_reparam_tangent(hf->dev, a, num_rays, sample_stride, pi, dheights, d_o, d_d, d_to_world, out_direction,
                              out_divergence, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_reparam_backward_full(const hf_field_t *hf, size_t n, const float *const o[3], const float *const d[3],
                                        const uint8_t *active, uint32_t num_rays, float kappa, float exponent,
                                        int antithetic, uint32_t seed, const uint32_t *ray_id, const hf_pi_const_t *pi,
                                        const float *si_boundary_test, size_t sample_stride,
                                        const float *const grad_direction[3], const float *grad_divergence,
                                        float *grad_heights, float *const grad_o[3], float *const grad_d[3],
                                        float *grad_to_world, hf_stream_t stream) {
    const char *fn = "hf_reparam_backward_full";
    if (!hf) return fail(HF_EINVAL, "%s: NULL handle", fn);
    if (!all3(o) || !all3(d) || !si_boundary_test || !all3(grad_direction) || !grad_divergence)
        return fail(HF_EINVAL, "%s: NULL argument", fn);
    int rc = check_pi(fn, n, pi);
    if (rc) return rc;
    if (grad_o && !all3(grad_o)) return fail(HF_EINVAL, "%s: NULL grad_o array", fn);
    if (grad_d && !all3(grad_d)) return fail(HF_EINVAL, "%s: NULL grad_d array", fn);
    if (!grad_heights && !grad_o && !grad_d && !grad_to_world) return fail(HF_EINVAL, "%s: NULL output (every gradient)", fn);
    if (!(kappa > 0.f)) return fail(HF_EINVAL, "%s: kappa must be > 0", fn);
    if (num_rays == 0 || num_rays > 32) return fail(HF_EINVAL, "%s: 1..32 auxiliary rays per ray (got %u)", fn, num_rays);
    if (num_rays > 1 && sample_stride < n) return fail(HF_EINVAL, "%s: sample_stride < n", fn);
    if (n >= ((size_t) 1 << 32)) return fail(HF_EINVAL, "%s: more than 2^32 rays", fn);
    if ((rc = check_device(fn, hf))) return rc;
    if (n == 0) return HF_OK;
    hf_reparam_args a = {};
    a.n = n; a.active = active; a.seed = seed; a.kappa = kappa; a.exponent = exponent; a.antithetic = antithetic;
    a.ray_id = ray_id; a.si_bt = si_boundary_test; a.g_div = grad_divergence;
    for (int c = 0; c < 3; ++c) { a.o[c] = o[c]; a.d[c] = d[c]; a.g_dir[c] = grad_direction[c]; }
    if (grad_to_world) {
        slot_lease lease(hf, (hipStream_t) stream, hf_xform_slab_bytes(n)); // the slab: this launch's alone
        if (!lease.buf) return fail(lease.code, "%s: %s", fn, lease.why);
        hf_launch_reparam_backward_full(hf->dev, a, num_rays, sample_stride, pi, grad_heights, grad_o, grad_d,
                                        grad_to_world, lease.buf, (hipStream_t) stream);
    } else {
        hf_launch_reparam_backward_full(hf->dev, a, num_rays, sample_stride, pi, grad_heights, grad_o, grad_d, nullptr,
                                        nullptr, (hipStream_t) stream);
    }
    HF_HIP(hipGetLastError());
    return HF_OK;
}

// ---- scalar / packet entry: host pointers, per-thread staging ------------------------
namespace {
// layout of the staging block, in floats: 7 ray rows, t, u, v, prim (u32), then HF_PACKET_MAX bytes of mask / hit
enum { PK_ROWS = 11, PK_FLOATS = PK_ROWS * HF_PACKET_MAX, PK_BYTES = PK_FLOATS * 4 + 2 * HF_PACKET_MAX };
struct packet_stage {
    int device = -1;
    hipStream_t stream = nullptr;
    char *h = nullptr, *d = nullptr; // pinned host mirror, device block
    void release() {
        if (device < 0) return;
        hf_device_guard guard(device);
        if (stream) (void) hipStreamDestroy(stream);
        if (h) (void) hipHostFree(h);
        if (d) (void) hipFree(d);
        device = -1; stream = nullptr; h = d = nullptr;
    }
    ~packet_stage() { release(); }
};
thread_local packet_stage g_stage;

int stage_for(const char *fn, int device, packet_stage **out) {
    packet_stage &s = g_stage;
    if (s.device != device) {
        s.release();
        hipError_t e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipHostMalloc((void **) &s.h, PK_BYTES, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc((void **) &s.d, PK_BYTES);
        if (e != hipSuccess) {
            s.device = device; // so that release() frees what exists
            s.release();
            return fail(e == hipErrorOutOfMemory ? HF_ENOMEM : HF_EDEVICE, "%s: %s", fn, hipGetErrorString(e));
        }
        s.device = device;
    }
    *out = &s;
    return HF_OK;
}

// mode 0: closest hit, mode 1: any hit
int packet_trace(const char *fn, int mode, const hf_field_t *hf, uint32_t n, const float *const h_o[3],
                 const float *const h_d[3], const float *h_maxt, const uint8_t *h_active, float *h_t,
                 float *const h_uv[2], uint32_t *h_prim, uint8_t *h_hit) {
    if (!hf || !h_o || !h_d || !h_maxt) return fail(HF_EINVAL, "%s: NULL argument", fn);
    if (n == 0) return HF_OK;
    if (n > HF_PACKET_MAX) return fail(HF_EINVAL, "%s: packet of %u rays (at most %d)", fn, n, HF_PACKET_MAX);
    for (int k = 0; k < 3; ++k)
        if (!h_o[k] || !h_d[k]) return fail(HF_EINVAL, "%s: NULL ray component array", fn);
    hf_device_guard guard(hf->device);
    if (!guard.ok) return fail(HF_EDEVICE, "%s: cannot select device %d", fn, hf->device);
    packet_stage *st;
    int rc = stage_for(fn, hf->device, &st);
    if (rc) return rc;
    float *hf32 = (float *) st->h;
    for (int k = 0; k < 3; ++k) {
        memcpy(hf32 + (size_t) k * HF_PACKET_MAX, h_o[k], sizeof(float) * n);
        memcpy(hf32 + (size_t) (3 + k) * HF_PACKET_MAX, h_d[k], sizeof(float) * n);
    }
    memcpy(hf32 + 6 * HF_PACKET_MAX, h_maxt, sizeof(float) * n);
    uint8_t *hmask = (uint8_t *) (st->h + PK_FLOATS * 4), *hhit = hmask + HF_PACKET_MAX;
    for (uint32_t k = 0; k < n; ++k) hmask[k] = h_active ? h_active[k] : 1;
    float *d32 = (float *) st->d;
    uint8_t *dmask = (uint8_t *) (st->d + PK_FLOATS * 4), *dhit = dmask + HF_PACKET_MAX;
    HF_HIP(hipStreamWaitEvent(st->stream, hf->built, 0)); // the last rebuild of the acceleration data
    HF_HIP(hipMemcpyAsync(st->d, st->h, PK_BYTES, hipMemcpyHostToDevice, st->stream));
    hf_rays_t rays;
    for (int k = 0; k < 3; ++k) { rays.o[k] = d32 + (size_t) k * HF_PACKET_MAX; rays.d[k] = d32 + (size_t) (3 + k) * HF_PACKET_MAX; }
    rays.maxt = d32 + 6 * HF_PACKET_MAX;
    hf_pi_t pi;
    pi.t = d32 + 7 * HF_PACKET_MAX; pi.prim_uv[0] = d32 + 8 * HF_PACKET_MAX; pi.prim_uv[1] = d32 + 9 * HF_PACKET_MAX;
    pi.prim_index = (uint32_t *) (d32 + 10 * HF_PACKET_MAX);
    rc = trace(fn, mode, hf, n, &rays, dmask, mode == 0 ? &pi : nullptr, mode == 1 ? dhit : nullptr, nullptr, 0, st->stream,
               nullptr, false);
    if (rc) return rc;
    HF_HIP(hipMemcpyAsync(st->h, st->d, PK_BYTES, hipMemcpyDeviceToHost, st->stream));
    HF_HIP(hipStreamSynchronize(st->stream));
    if (mode == 0) {
        if (h_t) memcpy(h_t, hf32 + 7 * HF_PACKET_MAX, sizeof(float) * n);
        if (h_uv && h_uv[0]) memcpy(h_uv[0], hf32 + 8 * HF_PACKET_MAX, sizeof(float) * n);
        if (h_uv && h_uv[1]) memcpy(h_uv[1], hf32 + 9 * HF_PACKET_MAX, sizeof(float) * n);
        if (h_prim) memcpy(h_prim, hf32 + 10 * HF_PACKET_MAX, sizeof(uint32_t) * n);
    } else {
        memcpy(h_hit, hhit, n);
    }
    return HF_OK;
}
} // namespace

extern "C" int hf_ray_intersect_preliminary_packet(const hf_field_t *hf, uint32_t n, const float *const h_o[3],
                                                   const float *const h_d[3], const float *h_maxt,
                                                   const uint8_t *h_active, float *h_t, float *const h_prim_uv[2],
                                                   uint32_t *h_prim_index) {
    if (n && !h_t) return fail(HF_EINVAL, "hf_ray_intersect_preliminary_packet: NULL output");
    return packet_trace("hf_ray_intersect_preliminary_packet", 0, hf, n, h_o, h_d, h_maxt, h_active, h_t, h_prim_uv,
                        h_prim_index, nullptr);
}

extern "C" int hf_ray_test_packet(const hf_field_t *hf, uint32_t n, const float *const h_o[3],
                                  const float *const h_d[3], const float *h_maxt, const uint8_t *h_active,
                                  uint8_t *h_hit) {
    if (n && !h_hit) return fail(HF_EINVAL, "hf_ray_test_packet: NULL output");
    return packet_trace("hf_ray_test_packet", 1, hf, n, h_o, h_d, h_maxt, h_active, nullptr, nullptr, nullptr, h_hit);
}

// ---- large-steps preconditioning: u = (I + lambda L) v and its conjugate-gradient solve on the vertex grid ----
// the grid limits are hf_create's: at most 32768 cells per side and 2^30 vertices
static int large_steps_grid(const char *who, uint32_t W, uint32_t H, double lambda) {
    if (W < 2 || H < 2) return fail(HF_EINVAL, "%s: the grid must have at least 2 x 2 vertices (got %u x %u)", who, W, H);
    if (W > 32769u || H > 32769u || (size_t) W * (size_t) H > ((size_t) 1 << 30))
        return fail(HF_EINVAL, "%s: grid too large (more than 32768 cells per side or 2^30 vertices)", who);
    if (!(lambda >= 0.0) || !isfinite(lambda)) return fail(HF_EINVAL, "%s: lambda must be finite and >= 0 (got %g)", who, lambda);
    return HF_OK;
}

extern "C" size_t hf_large_steps_workspace_floats(uint32_t W, uint32_t H) {
    if (W < 2 || H < 2) return 0;
    return hf_large_steps_scratch_floats(W, H);
}

extern "C" int hf_large_steps_apply(uint32_t W, uint32_t H, double lambda, const float *v, float *u, hf_stream_t stream) {
    const char *fn = "hf_large_steps_apply";
    if (!v || !u) return fail(HF_EINVAL, "%s: NULL argument", fn);
    const int rc = large_steps_grid(fn, W, H, lambda);
    if (rc != HF_OK) return rc;
    if (v == u) return fail(HF_EINVAL, "%s: v and u must be different buffers (a block reads its neighbours' vertices)", fn);
    hf_launch_large_steps_apply(W, H, lambda, v, u, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

extern "C" int hf_large_steps_solve(uint32_t W, uint32_t H, double lambda, const float *u, float *v, int warm, uint32_t max_iter,
                                    float rel_tol, float *workspace, float *info, hf_stream_t stream) {
    const char *fn = "hf_large_steps_solve";
    if (!u || !v || !workspace) return fail(HF_EINVAL, "%s: NULL argument", fn);
    const int rc = large_steps_grid(fn, W, H, lambda);
    if (rc != HF_OK) return rc;
    if (!(rel_tol >= 0.f)) return fail(HF_EINVAL, "%s: rel_tol must be >= 0 (got %g)", fn, (double) rel_tol);
    if (max_iter == 0) return fail(HF_EINVAL, "%s: max_iter must be at least 1", fn);
    if (u == v) return fail(HF_EINVAL, "%s: u and v must be different buffers", fn);
    if ((uintptr_t) workspace % 16u) return fail(HF_EINVAL, "%s: the workspace must be 16-byte aligned", fn);
    hf_launch_large_steps_solve(W, H, lambda, u, v, warm, max_iter, rel_tol, workspace, info, (hipStream_t) stream);
    HF_HIP(hipGetLastError());
    return HF_OK;
}

// ---- multi-GPU: the one collective of the path --------------------------------------------
namespace {
typedef int (*nccl_allreduce_fn)(const void *, void *, size_t, int, int, void *, hipStream_t);
typedef const char *(*nccl_errstr_fn)(int);
nccl_allreduce_fn g_allreduce = nullptr;
nccl_errstr_fn g_nccl_errstr = nullptr;
std::once_flag g_nccl_once;
void bind_rccl() {
    // the host's own RCCL first (communicator and call must come from one library), else the system library
    void *sym = dlsym(RTLD_DEFAULT, "ncclAllReduce");
    void *lib = nullptr;
    if (!sym) {
        const char *names[] = { "librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so" };
        for (const char *nm : names)
            if ((lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL))) break;
        if (lib) sym = dlsym(lib, "ncclAllReduce");
    }
    g_allreduce = (nccl_allreduce_fn) sym;
    g_nccl_errstr = (nccl_errstr_fn) (lib ? dlsym(lib, "ncclGetErrorString") : dlsym(RTLD_DEFAULT, "ncclGetErrorString"));
}
} // namespace

extern "C" int hf_allreduce_grad(float *d_grad, size_t count, void *rccl_comm, hf_stream_t stream) {
    if (!d_grad || !rccl_comm) return fail(HF_EINVAL, "hf_allreduce_grad: NULL argument");
    if (count == 0) return HF_OK;
    std::call_once(g_nccl_once, bind_rccl);
    if (!g_allreduce) return fail(HF_EDEVICE, "hf_allreduce_grad: RCCL (ncclAllReduce) not found in the process or as librccl.so");
    // ncclFloat32 = 7, ncclSum = 0 (rccl.h: ncclDataType_t / ncclRedOp_t)
    const int rc = g_allreduce(d_grad, d_grad, count, 7, 0, rccl_comm, (hipStream_t) stream);
    if (rc != 0)
        return fail(HF_EDEVICE, "hf_allreduce_grad: ncclAllReduce failed: %s", g_nccl_errstr ? g_nccl_errstr(rc) : "error");
    return HF_OK;
}
