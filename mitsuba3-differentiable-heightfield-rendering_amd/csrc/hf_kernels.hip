// hf_kernels.hip -- gfx950 kernels of libhf + their launchers.
//
//   hf_mip_level1_kernel / hf_mip_reduce_kernel   min/max mip pyramid
//   hf_shear_kernel / hf_shear_minmax_kernel       node records of every level 1..top (hf_device.h)
//   hf_trace_kernel<MODE>                          hierarchical min/max-mip traversal:
//        MODE 0 closest hit  -> PreliminaryIntersection   (row a1)
//        MODE 1 any hit      -> ray_test                   (row a2)
//        MODE 2 closest hit + fused surface interaction    (rows a1+a4)
//        MODE 3 MODE 2 with smooth shading (hf_set_face_normals(hf, 0): interpolated vertex normals)
//   hf_si_kernel / hf_si_smooth_kernel             compute_surface_interaction (row a4), flat / smooth shading
//   hf_adjoint_kernel / hf_adjoint_smooth_kernel   reverse mode of a4, atomic scatter (row a5)
//   hf_tangent_kernel / hf_tangent_smooth_kernel   forward mode of a4
//   hf_vertex_normals_kernel, hf_shading_derivatives_kernel   smooth shading: the vertex normals, dn_du / dn_dv
//   hf_direct_kernel / hf_direct_adjoint_kernel, hf_adam_kernel     next rows
//   hf_area_reduce / _scan_tiles / _cdf_kernel     area sampling: the triangle-area CDF (hf_set_area_sampling)
//   hf_sample_position / _adjoint / _tangent_kernel  Mesh::sample_position and its two derivatives
//   hf_attr / _tangent_kernel<TYPE, SIZE>, hf_attr_adjoint_tile / _face_adjoint_kernel<SIZE>  shape attributes:
//        Mesh::eval_attribute and its two derivatives
//   hf_large_steps_stencil / _update / _cold / _sum / _finish_kernel  large-steps preconditioning: (I + lambda L) v and
//        its conjugate-gradient solve on the vertex grid (end of the file)
//
// Traversal = a walk of the implicit quadtree over the cells (the grid is mirrored so the ray direction is
// non-negative on both axes: "order space").  One visit of an inner node fetches its record -- a plane through
// the node's corner heights and, per child, the range of (z - plane) over the child: "sheared
// bounds", tight on slopes; the zero plane with plain min/max above level HF_SHEAR_TOP -- and keeps
// the children the *fat* ray segment [0,t_hi] overlaps; the children of a level-1 node are
// cells, whose two triangles are then tested.
// The 64 rays of a coherent wave (primary rays: one pixel's samples) share the upper levels: the wave's rays are
// bounded by a beam, the nodes of level HF_SUBTREE_LEVEL along the beam are enumerated front to back with the LANES
// acting as node testers (one round trip for all boxes and records, parked in the wave's LDS), and the survivors are
// box-tested per lane and their own record evaluated for all lanes at once (walk_beam).  Everything below such a node is
// a WAVE-WIDE WORK LIST (items_run, round 4): the children a lane is to visit become items (ray, node) on a stack in
// LDS -- ballot-free prefix-sum compaction -- and every round the wave pops up to 64 of them, any lane taking any
// item (the ray's constants come from the owning lane's registers by ds_bpermute), down to (ray, cell) items whose hits
// are merged per ray with a 64-bit minimum in LDS.  An incoherent wave hands the root to every lane instead: per-lane
// depth-first walk, children front to back, pending children as 4-bit-per-level mask stacks in registers, converged
// rounds (lanes walk until they hold candidate cells; the two-triangle test runs for all of them together).
// Fetches of 256 rays that miss the bound as a whole never get that far (the wide path of the kernel).  The visited
// set is a conservative superset of the cells the ray can hit; the per-triangle test and the tie rule are order
// independent, so the result equals the brute force's.
#include <stdlib.h>
#include <type_traits>
#include "hf_device.h"
#include "hf_launch.h"

#define HF_BLOCK 256
#ifndef HF_SUBTREE_LEVEL
#define HF_SUBTREE_LEVEL 4 // the beam sweep hands nodes of this level (16x16 cells) to the per-lane walk (5: +2 %, 3: the beam is too often wider than four nodes)
#endif

// ---------------------------------------------------------------------------------
// min/max mip pyramid (coarse-first, padded -- see hf_dev_field)
// ---------------------------------------------------------------------------------
// level 1: node (ix,iy) bounds cells [2ix, 2ix+1] x [2iy, 2iy+1], i.e. vertices [2ix, 2ix+2]^2
__global__ __launch_bounds__(HF_BLOCK) void hf_mip_level1_kernel(const float *__restrict__ h, int W, int H, float s,
                                                                float2 *__restrict__ out, int sh) {
    const int idx = blockIdx.x * HF_BLOCK + threadIdx.x;
    if (idx >= (1 << (2 * sh))) return;
    const int iy = idx >> sh, ix = idx & ((1 << sh) - 1);
    float mn = __builtin_inff(), mx = -__builtin_inff();
    // cells [2ix, 2ix+1] x [2iy, 2iy+1] that exist, then their vertices
    const int ci0 = 2 * iy, ci1 = min(2 * iy + 1, H - 2);
    const int cj0 = 2 * ix, cj1 = min(2 * ix + 1, W - 2);
    if (ci0 <= ci1 && cj0 <= cj1) {
        for (int i = ci0; i <= ci1 + 1; ++i)
            for (int j = cj0; j <= cj1 + 1; ++j) {
                const float z = h[(size_t) i * W + j] * s;
                mn = fminf(mn, z); mx = fmaxf(mx, z);
            }
    }
    out[idx] = make_float2(mn, mx);
}

// depth k from depth k+1: 2x2 reduce
__global__ __launch_bounds__(HF_BLOCK) void hf_mip_reduce_kernel(const float2 *__restrict__ in, float2 *__restrict__ out,
                                                                int sh) {
    const int idx = blockIdx.x * HF_BLOCK + threadIdx.x;
    if (idx >= (1 << (2 * sh))) return;
    const int iy = idx >> sh, ix = idx & ((1 << sh) - 1);
    const float2 *c = in + ((size_t) (2 * iy) << (sh + 1)) + 2 * ix;
    const float2 a = c[0], b = c[1], d = c[(size_t) 1 << (sh + 1)], e = c[((size_t) 1 << (sh + 1)) + 1];
    out[idx] = make_float2(fminf(fminf(a.x, b.x), fminf(d.x, e.x)), fmaxf(fmaxf(a.y, b.y), fmaxf(d.y, e.y)));
}

// sheared bounds of level L (see hf_device.h): one thread per (node, child), then one per node
__global__ __launch_bounds__(HF_BLOCK) void hf_shear_kernel(const float *__restrict__ h, int W, int H, float s, int L,
                                                           int sh, float4 *__restrict__ out) {
    const int idx = blockIdx.x * HF_BLOCK + threadIdx.x;
    if (idx >= (4 << (2 * sh))) return;
    const int j = idx & 3, node = idx >> 2, iy = node >> sh, ix = node & ((1 << sh) - 1);
    const int size = 1 << L, S = size >> 1, x0 = ix * size, y0 = iy * size;
    // plane through the (clamped) corner heights; any plane is valid, the ranges below are exact for it
    const int xa = min(x0, W - 1), xb = min(x0 + size, W - 1), ya = min(y0, H - 1), yb = min(y0 + size, H - 1);
    const float z00 = h[(size_t) ya * W + xa] * s, z10 = h[(size_t) ya * W + xb] * s;
    const float z01 = h[(size_t) yb * W + xa] * s, z11 = h[(size_t) yb * W + xb] * s;
    const float inv = 0.5f / (float) size;
    const float a = ((z10 - z00) + (z11 - z01)) * inv, b = ((z01 - z00) + (z11 - z10)) * inv;
    const float c = 0.25f * ((z00 + z10) + (z01 + z11));
    const float xc = (float) (x0 + S), yc = (float) (y0 + S);
    // child j: cells [cj0, cj1] x [ci0, ci1] that exist, then their vertices
    const int cj0 = x0 + (j & 1) * S, cj1 = min(cj0 + S - 1, W - 2);
    const int ci0 = y0 + (j >> 1) * S, ci1 = min(ci0 + S - 1, H - 2);
    float lo = __builtin_inff(), hi = -__builtin_inff();
    if (ci0 <= ci1 && cj0 <= cj1) {
        for (int i = ci0; i <= ci1 + 1; ++i) {
            const float row = __builtin_fmaf(b, (float) i - yc, c);
            for (int jj = cj0; jj <= cj1 + 1; ++jj) {
                const float w = h[(size_t) i * W + jj] * s - __builtin_fmaf(a, (float) jj - xc, row);
                lo = fminf(lo, w); hi = fmaxf(hi, w);
            }
        }
        // rounding of the plane evaluation above
        const float eps = 1e-6f * (__builtin_fabsf(c) + (__builtin_fabsf(a) + __builtin_fabsf(b)) * (float) size);
        lo -= eps; hi += eps;
    }
    // fourth entry of the record (see below): slope of the plane + the largest child range, over the node's four
    // threads (adjacent lanes; an absent child gives -inf)
    float rmax = hi - lo;
    rmax = fmaxf(rmax, __shfl_xor(rmax, 1));
    rmax = fmaxf(rmax, __shfl_xor(rmax, 2));
    float *rec = (float *) (out + (size_t) node * 3);
    if (j == 0) { rec[0] = a; rec[1] = b; rec[2] = c; rec[3] = __builtin_fabsf(a) + __builtin_fabsf(b) + 2.f * fmaxf(rmax, 0.f); }
    rec[4 + 2 * j] = lo; rec[5 + 2 * j] = hi;
}
// Fourth entry of the record: what the walk multiplies its xy uncertainty m by to get a z uncertainty -- the slope
// of the plane, |a|+|b| per cell, PLUS TWICE the largest sheared range of a child: the triangle test may report a hit
// up to m cells beside the walk's ray (that is what m stands for), and where the surface is far steeper than the plane
// (a needle triangle) those m cells are up to m x (|dw/dx| + |dw/dy|) up or down, each partial derivative of a triangle
// bounded by the sheared range of its cell, hence of the child that holds it.  (One range until round 4: the full brute
// force over 16.7 M cells -- found through the oracle walk once IT carried the factor two -- reports a noise hit at
// N = 4096 from 8 units away that (|a|+|b|+r) m fell short of: tests/test_gpu_band.py::
// test_walk_needle_term_regression_on_the_gpu.)
// (computed by hf_shear_kernel / hf_shear_level1_kernel with the ranges.)

// Level 1 (three quarters of all records, 201 MB at N = 4096): one thread per node -- the 3x3 vertex window is read
// once, the four children are the cells themselves, the slope factor is computed in the same pass and the record is
// written as three 16-byte stores.  Same arithmetic as hf_shear_kernel with L = 1.
// The same window also gives the node's entry of the min/max pyramid (hf_mip_level1_kernel's value: clamping only
// repeats vertices of existing cells), written when mip1 is not null.
__global__ __launch_bounds__(HF_BLOCK) void hf_shear_level1_kernel(const float *__restrict__ h, int W, int H, float s,
                                                                  int sh, float4 *__restrict__ out,
                                                                  float2 *__restrict__ mip1) {
    const int node = blockIdx.x * HF_BLOCK + threadIdx.x;
    if (node >= (1 << (2 * sh))) return;
    const int iy = node >> sh, ix = node & ((1 << sh) - 1);
    const int x0 = 2 * ix, y0 = 2 * iy;
    float z[3][3]; // vertex window, clamped to the grid (clamped entries are only used where the kernel above clamps too)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            z[i][j] = h[(size_t) min(y0 + i, H - 1) * W + min(x0 + j, W - 1)] * s;
    if (mip1) {
        float mn = __builtin_inff(), mx = -__builtin_inff();
        if (y0 <= H - 2 && x0 <= W - 2) { // at least cell (x0, y0) exists
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) { mn = fminf(mn, z[i][j]); mx = fmaxf(mx, z[i][j]); }
        }
        mip1[node] = make_float2(mn, mx);
    }
    const float z00 = z[0][0], z10 = z[0][2], z01 = z[2][0], z11 = z[2][2];
    const float inv = 0.5f / 2.f;
    const float a = ((z10 - z00) + (z11 - z01)) * inv, b = ((z01 - z00) + (z11 - z10)) * inv;
    const float c = 0.25f * ((z00 + z10) + (z01 + z11));
    const float xc = (float) (x0 + 1), yc = (float) (y0 + 1);
    const float eps = 1e-6f * (__builtin_fabsf(c) + (__builtin_fabsf(a) + __builtin_fabsf(b)) * 2.f);
    float lo[4], hi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int cj = x0 + (j & 1), ci = y0 + (j >> 1); // the child is cell (cj, ci)
        lo[j] = __builtin_inff(); hi[j] = -__builtin_inff();
        if (cj <= W - 2 && ci <= H - 2) {
#pragma unroll
            for (int di = 0; di < 2; ++di) {
                const float row = __builtin_fmaf(b, (float) (ci + di) - yc, c);
#pragma unroll
                for (int dj = 0; dj < 2; ++dj) {
                    const float w = z[(j >> 1) + di][(j & 1) + dj] - __builtin_fmaf(a, (float) (cj + dj) - xc, row);
                    lo[j] = fminf(lo[j], w); hi[j] = fmaxf(hi[j], w);
                }
            }
            lo[j] -= eps; hi[j] += eps;
        }
    }
    const float rmax = fmaxf(fmaxf(fmaxf(hi[0] - lo[0], hi[1] - lo[1]), fmaxf(hi[2] - lo[2], hi[3] - lo[3])), 0.f); // absent: -inf
    float4 *rec = out + (size_t) node * 3;
    rec[0] = make_float4(a, b, c, __builtin_fabsf(a) + __builtin_fabsf(b) + 2.f * rmax);
    rec[1] = make_float4(lo[0], hi[0], lo[1], hi[1]);
    rec[2] = make_float4(lo[2], hi[2], lo[3], hi[3]);
}

// Levels above HF_SHEAR_TOP keep plain min/max boxes, stored in the same record form with the zero plane
// (a = b = c = 0, slope factor 0: w = z, and shear_line leaves the ray's z line untouched bit for bit), so that
// the per-lane walk reads every inner node through ONE code path -- three 16-byte loads from one address.
// Children of node (ix,iy) of level L = nodes (2ix+jx, 2iy+jy) of depth k+1 of the pyramid (L >= 2).
// (a, b, c) = 0 and |a|+|b|+r = the largest child range r: the record of a min/max level.  r is the needle term of
// shear_line's z margin -- a hit reported up to m cells beside the walk's ray sits up to m x (height range) above or
// below it -- which the fitted-plane records carry too; absent children (+inf, -inf) do not count.
__device__ __forceinline__ float4 hf_minmax_plane(float2 a, float2 b, float2 d, float2 e) {
    const float r = fmaxf(fmaxf(fmaxf(a.y - a.x, b.y - b.x), fmaxf(d.y - d.x, e.y - e.x)), 0.f);
    return make_float4(0.f, 0.f, 0.f, 2.f * r);
}
__global__ __launch_bounds__(HF_BLOCK) void hf_shear_minmax_kernel(const float2 *__restrict__ child, int sh,
                                                                  float4 *__restrict__ out) {
    const int node = blockIdx.x * HF_BLOCK + threadIdx.x;
    if (node >= (1 << (2 * sh))) return;
    const int iy = node >> sh, ix = node & ((1 << sh) - 1);
    const float2 *c = child + ((size_t) (2 * iy) << (sh + 1)) + 2 * ix;
    const float2 a = c[0], b = c[1], d = c[(size_t) 1 << (sh + 1)], e = c[((size_t) 1 << (sh + 1)) + 1];
    float4 *rec = out + (size_t) node * 3;
    rec[0] = hf_minmax_plane(a, b, d, e);
    rec[1] = make_float4(a.x, a.y, b.x, b.y);
    rec[2] = make_float4(d.x, d.y, e.x, e.y);
}

// The top of the pyramid in ONE launch: depths kmax..0 (at most 64x64 nodes each) by a single workgroup, level after
// level -- the 2x2 reduce of hf_mip_reduce_kernel and, above HF_SHEAR_TOP, the record of hf_shear_minmax_kernel, both
// from depth k+1, which the previous iteration (or the previous launch, for kmax) has completed.
#define HF_MIP_TOP_DEPTH 6
__global__ __launch_bounds__(1024) void hf_mip_top_kernel(float2 *__restrict__ mip, float4 *__restrict__ shear, int top,
                                                         int kmax) {
    for (int k = kmax; k >= 0; --k) {
        const float2 *c0 = mip + hf_depth_off(k + 1);
        float2 *o = mip + hf_depth_off(k);
        const bool rec_level = (top - k) > HF_SHEAR_TOP;
        float4 *recs = shear + (size_t) (hf_depth_off(k) - 1u) * 3;
        for (int node = (int) threadIdx.x; node < (1 << (2 * k)); node += (int) blockDim.x) {
            const int iy = node >> k, ix = node & ((1 << k) - 1);
            const float2 *c = c0 + ((size_t) (2 * iy) << (k + 1)) + 2 * ix;
            const float2 a = c[0], b = c[1], d = c[(size_t) 1 << (k + 1)], e = c[((size_t) 1 << (k + 1)) + 1];
            o[node] = make_float2(fminf(fminf(a.x, b.x), fminf(d.x, e.x)), fmaxf(fmaxf(a.y, b.y), fmaxf(d.y, e.y)));
            if (rec_level) {
                float4 *rec = recs + (size_t) node * 3;
                rec[0] = hf_minmax_plane(a, b, d, e);
                rec[1] = make_float4(a.x, a.y, b.x, b.y);
                rec[2] = make_float4(d.x, d.y, e.x, e.y);
            }
        }
        __threadfence_block();
        __syncthreads();
    }
}

void hf_launch_build_mips(const hf_dev_field &f, float2 *mip, float4 *shear, hipStream_t stream) {
    const int top = f.top;
    for (int L = 1; L <= top && L <= HF_SHEAR_TOP; ++L) { // level 1: the children are the cells themselves
        const int k = top - L, n = 1 << (2 * k);
        float4 *recs = shear + (size_t) (hf_depth_off(k) - 1u) * 3;
        if (L == 1) {
            hipLaunchKernelGGL(hf_shear_level1_kernel, dim3((n + HF_BLOCK - 1) / HF_BLOCK), dim3(HF_BLOCK), 0, stream, f.h,
                               f.W, f.H, f.s, k, recs, mip + hf_depth_off(k)); // + depth top-1 of the pyramid
            continue;
        }
        hipLaunchKernelGGL(hf_shear_kernel, dim3((4 * n + HF_BLOCK - 1) / HF_BLOCK), dim3(HF_BLOCK), 0, stream, f.h, f.W,
                           f.H, f.s, L, k, recs);
    }
    (void) hipMemsetAsync(mip, 0, sizeof(float2), stream); // padding entry
    // depths <= ktop of the pyramid and their records come from one launch at the end (hf_mip_top_kernel); every level
    // it covers must be a plain min/max level (the fitted-plane levels 1..HF_SHEAR_TOP are built from the heights)
    const int ktop = max(min(HF_MIP_TOP_DEPTH, top - 1 - HF_SHEAR_TOP), -1); // -1: no such level (top <= HF_SHEAR_TOP)
    for (int k = top - 1; k > ktop; --k) {
        const int n = 1 << (2 * k), grid = (n + HF_BLOCK - 1) / HF_BLOCK;
        if (k == top - 1) {
            if (top >= 1 && HF_SHEAR_TOP >= 1) continue; // written by hf_shear_level1_kernel above
            hipLaunchKernelGGL(hf_mip_level1_kernel, dim3(grid), dim3(HF_BLOCK), 0, stream, f.h, f.W, f.H, f.s,
                               mip + hf_depth_off(k), k);
        } else
            hipLaunchKernelGGL(hf_mip_reduce_kernel, dim3(grid), dim3(HF_BLOCK), 0, stream,
                               (const float2 *) (mip + hf_depth_off(k + 1)), mip + hf_depth_off(k), k);
    }
    for (int L = HF_SHEAR_TOP + 1; L <= top; ++L) { // after the pyramid: reads depth k+1 of it
        const int k = top - L, n = 1 << (2 * k);
        if (k <= ktop) break; // the rest: hf_mip_top_kernel
        hipLaunchKernelGGL(hf_shear_minmax_kernel, dim3((n + HF_BLOCK - 1) / HF_BLOCK), dim3(HF_BLOCK), 0, stream,
                           (const float2 *) (mip + hf_depth_off(k + 1)), k, shear + (size_t) (hf_depth_off(k) - 1u) * 3);
    }
    if (ktop >= 0)
        hipLaunchKernelGGL(hf_mip_top_kernel, dim3(1), dim3(1024), 0, stream, mip, shear, top, ktop);
}

// ---------------------------------------------------------------------------------
// traversal
// ---------------------------------------------------------------------------------
#ifdef HF_WSTATS
// wave-level execution counters: WCOUNT(k) adds 1 per wave each time the enclosing code runs with any lane
__device__ __forceinline__ uint32_t *wcnt_base() {
    __shared__ uint32_t c[HF_BLOCK / 64][16];
    return c[threadIdx.x >> 6];
}
#define WCOUNT(k) do { const uint64_t e_ = __ballot(true); if ((int) (threadIdx.x & 63u) == __builtin_ctzll(e_)) wcnt_base()[k]++; } while (0)
// WLANES(k): adds the number of lanes that run the enclosing code (k = 7: low half word = visits, high = cell rounds)
#define WLANES(k, sh) do { const uint64_t e_ = __ballot(true); if ((int) (threadIdx.x & 63u) == __builtin_ctzll(e_)) wcnt_base()[k] += (uint32_t) __builtin_popcountll(e_) << (sh); } while (0)
__device__ __forceinline__ void wstats_reset() { if ((threadIdx.x & 63u) < 16u) wcnt_base()[threadIdx.x & 63u] = 0u; }
// diagnostic build (scripts/wstats.py): the counters of this batch replace the hit record
#if HF_WSTATS == 4
// ... variant 4: histogram of the lanes that run a visit (c[11..13]) / a cell round (c[8..10]): at most 8, 9..24, more
#define WHIST(base) do { const uint64_t e_ = __ballot(true); if ((int) (threadIdx.x & 63u) == __builtin_ctzll(e_)) { \
        const int n_ = __builtin_popcountll(e_); wcnt_base()[(base) + (n_ <= 8 ? 0 : n_ <= 24 ? 1 : 2)]++; } } while (0)
#define WSTATS_EXPORT(alive, best) do { if (alive) { const uint32_t *c = wcnt_base(); (best).hit = true; \
        (best).t = (float) c[8] + 1024.f * (float) c[9] + 1048576.f * (float) c[10]; \
        (best).u = (float) c[11] + 1024.f * (float) c[12] + 1048576.f * (float) c[13]; (best).v = 0.f; (best).prim = c[7]; } } while (0)
#else
#define WSTATS_EXPORT(alive, best) do { if (alive) { const uint32_t *c = wcnt_base(); (best).hit = true; \
        (best).t = (float) c[0] + 1024.f * (float) c[1] + 1048576.f * (float) c[2]; \
        (best).u = (float) c[3] + 4096.f * (float) c[4]; (best).v = (float) c[5] + 4096.f * (float) c[6]; (best).prim = c[7]; } } while (0)
#endif
#else
#define WLANES(k, sh) do { } while (0)
#define WSTATS_EXPORT(alive, best) do { } while (0)
#define WCOUNT(k) do { } while (0)
__device__ __forceinline__ void wstats_reset() { }
#endif

#ifdef HF_TSTATS
// Cycle stamps (diagnostic build, scripts/tstats.py): TSTAMP(k) adds the shader cycles since the previous stamp of the
// wave to phase k of the batch (lane 0 keeps the books in LDS; each stamp costs an s_memtime and three LDS operations);
// at the end of a batch with live lanes, lane l < 16 reports phase l in place of its hit record.
__device__ __forceinline__ uint32_t *tcnt_base() {
    __shared__ uint32_t c[HF_BLOCK / 64][16];
    return c[threadIdx.x >> 6];
}
#define TSTART() do { __builtin_amdgcn_wave_barrier(); if ((threadIdx.x & 63u) == 0u) { uint32_t *c_ = tcnt_base(); \
        const uint32_t now_ = (uint32_t) clock64(), out_ = now_ - c_[15]; /* since the last stamp of the wave's previous batch: its output phase */ \
        for (int i_ = 0; i_ < 15; ++i_) c_[i_] = 0u; c_[8] = out_; c_[15] = now_; } __builtin_amdgcn_wave_barrier(); } while (0)
#define TSTAMP(k) do { if ((threadIdx.x & 63u) == 0u) { uint32_t *c_ = tcnt_base(); const uint32_t now_ = (uint32_t) clock64(); \
        c_[k] += now_ - c_[15]; c_[15] = now_; } } while (0)
#define TSTATS_EXPORT(any_alive, valid, best) do { __builtin_amdgcn_wave_barrier(); if ((any_alive) && (valid)) { (best).hit = true; \
        (best).t = (float) tcnt_base()[threadIdx.x & 15u]; (best).u = 0.f; (best).v = 0.f; (best).prim = threadIdx.x & 63u; } } while (0)
#else
#define TSTART() do { } while (0)
#define TSTAMP(k) do { } while (0)
#endif
#ifndef HF_M0
#define HF_M0 0.00390625f // constant part of the xy margin, cells (1/64 until round 3: see setup_ray)
#endif
#ifndef HF_LINE_EPS
#define HF_LINE_EPS 1e-6f // rounding of the sheared line, per cell of the grid's side (2e-6 until round 3)
#endif
#ifndef WHIST
#define WHIST(base) do { } while (0)
#endif
// per-ray traversal constants (order space, cell units, re-based at t = tin)
struct hf_trav {
    float gxm, gxp, gym, gyp; // origin x,y  +/- the xy margin m
    float gz, dz, idx, idy, mz;
};

// four cells as (min,max) boxes in ACTUAL order j = 2*jy + jx
struct hf_quad {
    float lo[4], hi[4];
};

// Overlap mask (ACTUAL numbering j = 2*jy + jx) of the fat ray segment [0,thi] with the four
// boxes of the 2x2 block whose order-space origin is (fX,fY), box size S.
// parameter of box j.  The third coordinate of the ray is the line  gz + t dz  (+/- mz): the height
// for min/max boxes, the sheared height for sheared bounds.  Direction is >= 0 in order space, so a box's entry planes are its low
// faces and its exit planes its high faces; v_max3/v_min3 drop the NaN of 0*inf (origin of an
// axis-parallel ray exactly on a face plane).
__device__ __forceinline__ uint32_t child_mask(const hf_trav &r, bool fx, bool fy, float fX, float fY, float S,
                                               const hf_quad &q, float gz, float dz, float mz, float thi) {
    const float ex = fX - r.gxm, lx = fX + S - r.gxp; // entry / exit plane offsets of order column 0
    const float ey = fY - r.gym, ly = fY + S - r.gyp;
    // order-space offset of ACTUAL child column / row 0 and 1 (a mirrored axis swaps near and far half)
    const float sx0 = fx ? S : 0.f, sx1 = S - sx0, sy0 = fy ? S : 0.f, sy1 = S - sy0;
    const float x0lo = (ex + sx0) * r.idx, x0hi = (lx + sx0) * r.idx;
    const float x1lo = (ex + sx1) * r.idx, x1hi = (lx + sx1) * r.idx;
    const float y0lo = (ey + sy0) * r.idy, y0hi = (ly + sy0) * r.idy;
    const float y1lo = (ey + sy1) * r.idy, y1hi = (ly + sy1) * r.idy;
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float xlo = (j & 1) ? x1lo : x0lo, xhi = (j & 1) ? x1hi : x0hi;
        const float ylo = (j & 2) ? y1lo : y0lo, yhi = (j & 2) ? y1hi : y0hi;
        const float t0 = fmaxf(fmaxf(xlo, ylo), 0.f), t1 = fminf(fminf(xhi, yhi), thi);
        const float za = __builtin_fmaf(t0, dz, gz), zb = __builtin_fmaf(t1, dz, gz);
        const bool ok = (t0 <= t1) & (fminf(za, zb) - mz <= q.hi[j]) & (fmaxf(za, zb) + mz >= q.lo[j]);
        m |= ok ? (1u << j) : 0u;
    }
    return m;
}

// everything a lane needs to walk its ray: object-space ray (spec arithmetic input of the
// triangle test) + traversal constants in order space
struct hf_ray_state {
    v3 oo, od;
    float maxt, tin, thi;
    float gx, gy, m; // order-space entry point (cell units) and xy margin
    hf_trav r;
    bool fx, fy;
};

// transform to object space, clip against the inflated bound, build the traversal ray.
// returns false when the ray cannot hit (outside the bound, non-finite, bad maxt).
__device__ __forceinline__ bool setup_ray(const hf_dev_field &f, float2 zr, v3 o, v3 d, float maxt,
                                          hf_ray_state &rs) {
    hf_trav &r = rs.r;
    const v3 oo = xform_point(f.to_object, o), od = xform_vec(f.to_object, d);
    rs.oo = oo; rs.od = od; rs.maxt = maxt;
    // non-finite input or NaN/negative maxt: miss (also bounds the walk below)
    {
        const float chk = (oo.x + oo.y + oo.z) + (od.x + od.y + od.z);
        if (!(__builtin_fabsf(chk) < __builtin_inff()) || !(maxt >= 0.f)) return false;
    }
    const int cw = f.W - 1, ch = f.H - 1, top = f.top;
    const float hx = f.hx, hy = f.hy; // 0.5 (W - 1), 0.5 (H - 1)
    const float zspan = fmaxf(zr.y - zr.x, fmaxf(__builtin_fabsf(zr.x), __builtin_fabsf(zr.y)));
    const float mz0 = 1e-5f * zspan + 1e-30f;

    // The margins first: they depend on how far the ray travels to the grid (`reach`), measured with the entry into
    // the bound inflated by the fixed amounts only (1e-4 in xy, mz0 in z) -- also for a ray that misses that bound.
    const float oc[3] = { oo.x, oo.y, oo.z }, dc[3] = { od.x, od.y, od.z };
    float rr[3];
    float tin0 = 0.f;
    {
        const float lo[3] = { -1.f - 1e-4f, -1.f - 1e-4f, zr.x - mz0 };
        const float hi[3] = { 1.f + 1e-4f, 1.f + 1e-4f, zr.y + mz0 };
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            rr[k] = 1.0f / dc[k];
            if (dc[k] != 0.f) tin0 = fmaxf(tin0, fminf((lo[k] - oc[k]) * rr[k], (hi[k] - oc[k]) * rr[k]));
        }
        tin0 = tin0 - __builtin_fabsf(tin0) * 1e-6f;
        tin0 = fmaxf(tin0, 0.f);
    }
    const float reach = __builtin_fabsf(oo.x) + __builtin_fabsf(oo.y) +
                        tin0 * (__builtin_fabsf(od.x) + __builtin_fabsf(od.y)) + 2.f;
    // xy margin: covers the rounding of the walk and the NOISE OF THE TRIANGLE TEST ITSELF -- how far beside the exact
    // ray a triangle can lie and still be reported hit by the fp32 Moeller-Trumbore arithmetic -- which grows faster
    // than linearly with the distance of the origin (against float64 geometry and the brute force over all cells:
    // 0.001 cell from 3 units away, up to 1.7 cells from 50 units away on needle terrain at N = 4096).  Beyond a reach
    // of 8 units the distance term therefore grows with (reach / 8)^2 (round 3: with the linear term and a cap of 0.3
    // cell the walk missed ~1 such hit in 10^4 rays traced from 50 units away; the walk only gets slower with m);
    // up to a reach of 8 units -- most rays of the BASELINE configurations; a few reach 9.5 -- the distance term is what it was.  Capped at 8 cells so that the
    // strip a ray walks (and the time of the launch) stays bounded however far its origin.  The constant part HF_M0 is
    // pure slack on top of the distance term, which is never below 8 eps x (grid side) -- the rounding of the walk's own
    // slab arithmetic; it was 1/64 cell until round 3 and fattened every sheared slab by 3x its curvature thickness on
    // smooth terrain: at 1/256 a batch needs 4.7 instead of 5.7 cell rounds (forward -3 %, bounce rays -4 %).  Same
    // formula in the oracle's walk; the band brute force (no margins at all) and the fuzz check that it suffices.
    const float far = fmaxf(1.f, 0.125f * reach);
    const float m = HF_M0 + fminf(8.f, 4.8e-7f * reach * fmaxf(hx, hy) * (far * far));

    // clip against the object-space bound (slab test, bbox.h:302-327) inflated by what such a hit can reach: m cells in
    // xy and m x (height span) in z on top of the fixed amounts -- every node test of the walk has that needle term,
    // and without it here a ray traced from 40 units away lost a (noise) hit the brute force reports 1 % of the height
    // span above the bound (round 3, the one mismatch of 4e9 fuzz rays against the band brute force)
    float tin = 0.f, tout = maxt;
    {
        // (sx = 1 / hx: a cell.  Multiply + add, not fma and not m / hx: the two divisions cost the launch 2 %, and with
        // the fused form the fused kernel spills 6 registers instead of 2)
        const float ex = 1e-4f + m * f.sx, ey = 1e-4f + m * f.sy, ez = __builtin_fmaf(2.f * m, zspan, mz0);
        const float lo[3] = { -1.f - ex, -1.f - ey, zr.x - ez };
        const float hi[3] = { 1.f + ex, 1.f + ey, zr.y + ez };
        bool outside = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (dc[k] == 0.f) {
                outside |= (oc[k] < lo[k]) | (oc[k] > hi[k]);
            } else {
                const float t1 = (lo[k] - oc[k]) * rr[k], t2 = (hi[k] - oc[k]) * rr[k];
                tin = fmaxf(tin, fminf(t1, t2));
                tout = fminf(tout, fmaxf(t1, t2));
            }
        }
        tin = tin - __builtin_fabsf(tin) * 1e-6f;
        tin = fmaxf(tin, 0.f);
        tout = tout + __builtin_fabsf(tout) * 1e-6f;
        if (outside || !(tin <= tout)) return false;
    }

    // traversal ray in cell units, re-based at t = tin, mirrored into order space
    const bool fx = od.x < 0.f, fy = od.y < 0.f;
    const float Wp = (float) (1 << top);
    // entry point in double: keeps the walk accurate for origins far from the grid
    float gx = (float) (((double) oo.x + (double) tin * (double) od.x + 1.0) * (double) hx);
    float gy = (float) (((double) oo.y + (double) tin * (double) od.y + 1.0) * (double) hy);
    r.gz = __builtin_fmaf(tin, od.z, oo.z);
    float dx = od.x * hx, dy = od.y * hy;
    r.dz = od.z;
    if (fx) { gx = Wp - gx; dx = -dx; }
    if (fy) { gy = Wp - gy; dy = -dy; }
    // |.|: a negative-zero component (d = -up, or a -0 surviving to_object) is mirrored by neither test above and
    // would give -inf here, which flips every slab test below; canonicalised it is the +inf of an axis-parallel ray
    r.idx = 1.0f / __builtin_fabsf(dx); r.idy = 1.0f / __builtin_fabsf(dy);
    r.mz = mz0 + 4.8e-7f * (__builtin_fabsf(oo.z) + tin * __builtin_fabsf(od.z) + zspan);
    r.gxm = gx + m; r.gxp = gx - m; r.gym = gy + m; r.gyp = gy - m;
    float thi = tout - tin;
    thi = thi + thi * 1e-6f + 1e-30f;

    rs.tin = tin; rs.thi = thi; rs.gx = gx; rs.gy = gy; rs.m = m; rs.fx = fx; rs.fy = fy;
    return true;
}

// Conservative twin of setup_ray's clip: false ONLY IF setup_ray would return false for this ray (it may say true for a
// ray setup_ray rejects: that ray just takes the ordinary path).  Same formulas with v_rcp_f32 instead of the three IEEE
// divisions, every quantity that enters the decision pushed to the safe side by 1e-5 relative (the reciprocals are off
// by one ulp, the products by half an ulp each: 3e-7), a ray with a zero direction component or a non-finite one is
// "maybe".  Used by the wide path of the traversal kernels for fetches that miss the bound as a whole.
__device__ __forceinline__ bool maybe_alive(const hf_dev_field &f, float2 zr, v3 o, v3 d, float maxt) {
    const v3 oo = xform_point(f.to_object, o), od = xform_vec(f.to_object, d);
    const float chk = (oo.x + oo.y + oo.z) + (od.x + od.y + od.z);
    if (!(__builtin_fabsf(chk) < __builtin_inff()) || !(maxt >= 0.f)) return true; // (setup_ray: a miss; left to it)
    if (!(__builtin_fabsf(od.x) >= 1e-30f) || !(__builtin_fabsf(od.y) >= 1e-30f) || !(__builtin_fabsf(od.z) >= 1e-30f)) return true; // (zero / denormal: 1/d overflows)
    const float zspan = fmaxf(zr.y - zr.x, fmaxf(__builtin_fabsf(zr.x), __builtin_fabsf(zr.y)));
    const float mz0 = 1e-5f * zspan + 1e-30f;
    const float oc[3] = { oo.x, oo.y, oo.z }, dc[3] = { od.x, od.y, od.z };
    float rr[3], tin0 = 0.f;
    {
        const float lo[3] = { -1.f - 1e-4f, -1.f - 1e-4f, zr.x - mz0 };
        const float hi[3] = { 1.f + 1e-4f, 1.f + 1e-4f, zr.y + mz0 };
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            rr[k] = __builtin_amdgcn_rcpf(dc[k]);
            tin0 = fmaxf(tin0, fminf((lo[k] - oc[k]) * rr[k], (hi[k] - oc[k]) * rr[k]));
        }
        tin0 = fmaxf(tin0, 0.f) * (1.f + 1e-5f); // an UPPER bound of setup_ray's tin0
    }
    const float reach = (__builtin_fabsf(oo.x) + __builtin_fabsf(oo.y) + tin0 * (__builtin_fabsf(od.x) + __builtin_fabsf(od.y)) + 2.f) * (1.f + 1e-5f);
    const float far = fmaxf(1.f, 0.125f * reach);
    const float m = (HF_M0 + fminf(8.f, 4.8e-7f * reach * fmaxf(f.hx, f.hy) * (far * far))) * (1.f + 1e-5f); // >= setup_ray's m
    const float ex = 1e-4f + m * f.sx, ey = 1e-4f + m * f.sy, ez = __builtin_fmaf(2.f * m, zspan, mz0);
    const float lo[3] = { -1.f - ex, -1.f - ey, zr.x - ez }, hi[3] = { 1.f + ex, 1.f + ey, zr.y + ez }; // contain setup_ray's box
    float tin = 0.f, tout = maxt;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float t1 = (lo[k] - oc[k]) * rr[k], t2 = (hi[k] - oc[k]) * rr[k];
        tin = fmaxf(tin, fminf(t1, t2));
        tout = fminf(tout, fmaxf(t1, t2));
    }
    // setup_ray keeps the ray when tin (1 - 1e-6) <= tout (1 + 1e-6); here both sides carry the reciprocals' error on top
    return tin - __builtin_fabsf(tin) * 1e-5f <= tout + __builtin_fabsf(tout) * 1e-5f;
}

// All auxiliary rays of a ray at once (hf_reparam_trace_all): false ONLY IF no von Mises-Fisher sample around d can
// pass setup_ray's clip.  Every sample lies within the angle theta_max of d (warp.h:557-566 with its clamp of the
// sample at 1e-6: cos theta >= 1 - 13.82 / kappa), so at the parameter tau of the primary ray's object-space line the
// auxiliary point is at most tau x ct away from it, ct = sqrt(2) ||to_object|| tan(theta_max) (launcher); an auxiliary
// hit lies in the bound, hence at tau <= (R + |o - c|) / (|d_obj| - ct) (R: radius of the inflated bound around its
// centre c), so the primary ray has to pass the bound inflated by r_max = that tau x ct on every axis -- tested like
// maybe_alive (v_rcp_f32, decisions pushed to the safe side).  "Maybe" whenever an assumption of the bound fails: a
// direction that is not unit length (the frame is then not orthonormal), an inflation of more than a tenth of the
// bound (tiny grids, far origins), |d_obj| <= ct.
__device__ __forceinline__ bool cone_maybe_alive(const hf_dev_field &f, float2 zr, v3 o, v3 d, float ct) {
    const v3 oo = xform_point(f.to_object, o), od = xform_vec(f.to_object, d);
    const float chk = (oo.x + oo.y + oo.z) + (od.x + od.y + od.z);
    if (!(__builtin_fabsf(chk) < __builtin_inff())) return true;
    if (!(__builtin_fabsf(dot3(d, d) - 1.f) <= 1e-3f)) return true;
    if (!(__builtin_fabsf(od.x) >= 1e-30f) || !(__builtin_fabsf(od.y) >= 1e-30f) || !(__builtin_fabsf(od.z) >= 1e-30f)) return true;
    const float zspan = fmaxf(zr.y - zr.x, fmaxf(__builtin_fabsf(zr.x), __builtin_fabsf(zr.y)));
    const float mz0 = 1e-5f * zspan + 1e-30f;
    const float zc = 0.5f * (zr.x + zr.y), zh = 0.5f * (zr.y - zr.x);
    const float zcap = 0.1f * zh + 0.1f * zspan + 1e-3f; // the z inflation R allows for (x, y: 0.1)
    const float dz0 = oo.z - zc;
    const float dist = __builtin_sqrtf(__builtin_fmaf(dz0, dz0, __builtin_fmaf(oo.y, oo.y, oo.x * oo.x))) * (1.f + 1e-5f);
    const float hzc = zh + zcap;
    const float R = __builtin_sqrtf(__builtin_fmaf(hzc, hzc, 2.42f)) * (1.f + 1e-5f); // half diagonal of (1.1, 1.1, zh + zcap)
    // no auxiliary ray travels further to the bound than this (cf. setup_ray's reach): an upper bound of every sample's m
    const float reach = (__builtin_fabsf(oo.x) + __builtin_fabsf(oo.y) + 1.4143f * (dist + R) + 2.f) * (1.f + 1e-5f);
    const float far = fmaxf(1.f, 0.125f * reach);
    const float m = (HF_M0 + fminf(8.f, 4.8e-7f * reach * fmaxf(f.hx, f.hy) * (far * far))) * (1.f + 1e-5f);
    const float ex = 1e-4f + m * f.sx, ey = 1e-4f + m * f.sy, ez = __builtin_fmaf(2.f * m, zspan, mz0);
    if (!(ex <= 0.1f) || !(ey <= 0.1f) || !(ez <= zcap)) return true;
    const float den = __builtin_sqrtf(dot3(od, od)) * (1.f - 1e-5f) - ct;
    if (!(den > 0.f)) return true;
    const float rmax = (R + dist) * __builtin_amdgcn_rcpf(den) * ct * (1.f + 1e-4f);
    const float lo[3] = { -1.f - ex - rmax, -1.f - ey - rmax, zr.x - ez - rmax }, hi[3] = { 1.f + ex + rmax, 1.f + ey + rmax, zr.y + ez + rmax };
    const float oc[3] = { oo.x, oo.y, oo.z }, dc[3] = { od.x, od.y, od.z };
    float tin = 0.f, tout = __builtin_inff();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float r = __builtin_amdgcn_rcpf(dc[k]);
        const float t1 = (lo[k] - oc[k]) * r, t2 = (hi[k] - oc[k]) * r;
        tin = fmaxf(tin, fminf(t1, t2));
        tout = fminf(tout, fmaxf(t1, t2));
    }
    return tin - __builtin_fabsf(tin) * 1e-5f <= tout + __builtin_fabsf(tout) * 1e-5f;
}

// The ray in the sheared coordinate  w = z - (c + a (x - xc) + b (y - yc))  of a node whose centre is
// (xc,yc) in order space: w(t) = gz + t dz.  (a,b) are stored for actual coordinates; mirroring an
// axis into order space flips the sign of its slope.  mz grows by the slope times the xy uncertainty
// of the walk (the margin m) plus the rounding of the line itself, whose terms are as large as
// slope x grid size.
__device__ __forceinline__ void shear_line_v(const hf_trav &r, float dxo, float dyo, float eps_top, bool fx, bool fy, float a,
                                             float b, float c, float sab, float xc, float yc, float &gz, float &dz, float &mz) {
    const float ao = fx ? -a : a, bo = fy ? -b : b;
    const float ux = 0.5f * (r.gxm + r.gxp) - xc, uy = 0.5f * (r.gym + r.gyp) - yc;
    gz = __builtin_fmaf(-bo, uy, __builtin_fmaf(-ao, ux, r.gz - c));
    dz = __builtin_fmaf(-bo, dyo, __builtin_fmaf(-ao, dxo, r.dz));
    const float m = 0.5f * (r.gxm - r.gxp) + eps_top;
    mz = __builtin_fmaf(sab, m, r.mz);
}
// (dxo, dyo: the xy direction in cells per unit of t, order space; eps_top = HF_LINE_EPS x the grid's side)
__device__ __forceinline__ void shear_line(const hf_dev_field &f, const hf_ray_state &rs, bool fx, bool fy, float a,
                                           float b, float c, float sab, float xc, float yc, float &gz, float &dz,
                                           float &mz) {
    const float dxo = __builtin_fabsf(rs.od.x) * f.hx;
    const float dyo = __builtin_fabsf(rs.od.y) * f.hy;
    shear_line_v(rs.r, dxo, dyo, HF_LINE_EPS * (float) (1 << f.top), fx, fy, a, b, c, sab, xc, yc, gz, dz, mz);
}

// actual-child mask -> order-space child mask (bit k = bit (k ^ flip))
__device__ __forceinline__ uint32_t to_order(uint32_t m, bool fx, bool fy) {
    if (fx) m = ((m & 5u) << 1) | ((m >> 1) & 5u);
    if (fy) m = ((m & 3u) << 2) | ((m >> 2) & 3u);
    return m;
}

// data source of the per-lane subtree walk: heights + mips straight from global memory (L1/L2)
struct hf_src_global {
    const float2 *__restrict__ mip;
    const float4 *__restrict__ shear;
    const float *__restrict__ h;
    int top, W;
    // 32-bit byte offset from the uniform base (one scalar-base load, no 64-bit vector address maths);
    // hf_create limits the grid to 2^30 vertices
    __device__ __forceinline__ float height(int i, int j) const {
        const uint32_t off = ((uint32_t) i * (uint32_t) W + (uint32_t) j) << 2;
        return *(const float *) ((const char *) h + off);
    }
    // record of inner node (ix,iy) of level L >= 2: plane + the four child ranges (hf_device.h)
    __device__ __forceinline__ const float4 *sheared(int L, uint32_t ix, uint32_t iy) const {
        const uint32_t k = (uint32_t) (top - L);
        return shear + (size_t) (hf_depth_off((int) k) - 1u + (iy << k) + ix) * 3;
    }
};

// Per-lane depth-first walk of the subtree rooted at order-space node (X0,Y0) of level L0 >= 1
// (pending-children masks of the levels below L0 in a 4-bit-per-level register stack).
// "while-while": each lane walks until it holds a block with candidate cells (or is done); when
// every lane of the call has stopped, the candidate cells are triangle-tested together, one
// cell per lane per round -- the expensive test runs with all waiting lanes active.
// STK: the register stack of pending-children masks, 4 bits per level -- 64 bits for a walk from the root (the root of
// a 2^15-cell grid is 15 levels up), 32 bits for the walk below a hand-off node (HF_SUBTREE_LEVEL - 1 <= 8 levels)
template <typename STK>
struct hf_walk_t {
    uint32_t X, Y, cur, pend; // node (X,Y) of level L, its order-space children still to visit; candidate cells
    STK stk;                  // 4 bits per level: the ancestors' pending children
    int L;                    // level (1 while the lane holds candidate cells: they are the children of node (X,Y))
    bool fin;                 // subtree exhausted
};
typedef hf_walk_t<uint64_t> hf_walk;
__device__ __forceinline__ uint32_t stk_ctz(uint64_t v) { return (uint32_t) __builtin_ctzll(v); }
__device__ __forceinline__ uint32_t stk_ctz(uint32_t v) { return (uint32_t) __builtin_ctz(v); }
// start one level above the subtree root: a virtual parent whose only pending child is the root
template <typename STK>
__device__ __forceinline__ void walk_init(hf_walk_t<STK> &w, uint32_t X0, uint32_t Y0, int L0) {
    w.X = X0 >> 1; w.Y = Y0 >> 1; w.cur = 1u << ((X0 & 1u) | ((Y0 & 1u) << 1)); w.pend = 0u;
    w.stk = 0; w.L = L0 + 1; w.fin = false;
}
// One round of the walk for every lane of the call: walk until parked or done, then the parked blocks, then
// the candidate cells.  Lanes with w.fin set do nothing.  Returns whether this lane recorded a hit.
template <bool ANY, typename Src, typename STK>
__device__ __forceinline__ bool walk_round(const hf_dev_field &f, const Src &src, const hf_ray_state &rs,
                                           const hf_trav &r, bool fx, bool fy, uint32_t fxm, uint32_t fym,
                                           float &thi, hf_hit &best, hf_walk_t<STK> &w) {
    auto loadh = [&src](int i, int j) { return src.height(i, j); };
    bool hit_any = false;
    // ---- walk until this lane holds candidate cells or has exhausted the subtree ----
    while (!w.fin && w.pend == 0u) {
        WCOUNT(3);
        if (w.cur == 0u) {
            // Node exhausted: pop.  Every level between here and the nearest ancestor with pending children is
            // skipped at once (the masks are 4-bit fields of one register: count the empty ones); the virtual
            // parent of the subtree root holds no children, so an all-zero stack means the subtree is done.
            if (w.stk == 0) { w.fin = true; break; }
            const uint32_t z = stk_ctz(w.stk) >> 2;
            w.stk >>= 4u * z;
            w.cur = (uint32_t) w.stk & 15u; w.stk >>= 4;
            w.X >>= z + 1u; w.Y >>= z + 1u; w.L += (int) z + 1;
        }
        const uint32_t k = (uint32_t) __builtin_ctz(w.cur);
        w.cur &= w.cur - 1u;
        const uint32_t cx = 2u * w.X + (k & 1u), cy = 2u * w.Y + (k >> 1);
        const float S = (float) (1u << (w.L - 1));
        // the mask may predate a hit: re-check the child's entry against the current t_hi
        const float te = fmaxf(((float) cx * S - r.gxm) * r.idx, ((float) cy * S - r.gym) * r.idy);
        if (te > thi) continue;
        WCOUNT(5); WLANES(7, 0); WHIST(11);
        w.stk = (w.stk << 4) | (STK) w.cur;
        w.X = cx; w.Y = cy; --w.L;
        // the four children of (X,Y,L): sheared bounds on the fine levels, min/max boxes above
        const float Sc = 0.5f * S;
        const uint32_t ix = w.X ^ (fxm >> w.L), iy = w.Y ^ (fym >> w.L);
        hf_quad q;
        float gz, dz, mz;
        {   // A wave-level gather returns when its slowest lane does (an L2 / Infinity Cache round trip, not an
            // L1 hit), so the plane and the child ranges of the record are requested together: one memory round
            // trip per visit.  Levels above HF_SHEAR_TOP carry the zero plane (hf_shear_minmax_kernel).
            const float4 *rec = src.sheared(w.L, ix, iy);
            const float4 pl = rec[0], q01 = rec[1], q23 = rec[2];
            shear_line(f, rs, fx, fy, pl.x, pl.y, pl.z, pl.w, __builtin_fmaf((float) w.X, S, Sc),
                       __builtin_fmaf((float) w.Y, S, Sc), gz, dz, mz);
            q.lo[0] = q01.x; q.hi[0] = q01.y; q.lo[1] = q01.z; q.hi[1] = q01.w;
            q.lo[2] = q23.x; q.hi[2] = q23.y; q.lo[3] = q23.z; q.hi[3] = q23.w;
        }
        const uint32_t m = child_mask(r, fx, fy, (float) w.X * S, (float) w.Y * S, Sc, q, gz, dz, mz, thi);
        if (w.L == 1) {
            // the children of a level-1 node are cells: they become this lane's candidates (ACTUAL numbering
            // j = 2 jy + jx, tested in any order -- the result is order independent) and the lane stops walking
            // until the converged triangle rounds below have run
            w.pend = m;
            w.cur = 0u;
        } else {
            w.cur = to_order(m, fx, fy);
        }
    }
    if (__ballot(w.pend != 0u) == 0ull) return false; // nobody holds candidate cells: every lane of the call is done
    // ---- candidate cells, one per lane per round ----
    while (__ballot(w.pend != 0u) != 0ull) {
        WCOUNT(6);
        if (w.pend != 0u) {
            WLANES(7, 16); WHIST(8);
            const int j = __builtin_ctz(w.pend);
            w.pend &= w.pend - 1u;
            // (the lane's node (X,Y) is the level-1 node whose children the candidate cells are: actual cell = 2 * actual node + j)
            const int cxx = (int) (2u * (w.X ^ (fxm >> 1))) + (j & 1), cyy = (int) (2u * (w.Y ^ (fym >> 1))) + (j >> 1);
            const float z00 = loadh(cyy, cxx) * f.s, z10 = loadh(cyy, cxx + 1) * f.s;
            const float z01 = loadh(cyy + 1, cxx) * f.s, z11 = loadh(cyy + 1, cxx + 1) * f.s;
            if (test_cell(f, cxx, cyy, z00, z10, z01, z11, rs.oo, rs.od, rs.maxt, best)) {
                hit_any = true;
                float tb = best.t - rs.tin;
                tb = tb + __builtin_fabsf(tb) * 1e-6f + 1e-30f;
                thi = fminf(thi, tb);
                if (ANY) { w.pend = 0u; w.fin = true; }
            }
        }
    }
    return hit_any;
}

template <bool ANY, typename Src>
__device__ __forceinline__ bool walk_subtree(const hf_dev_field &f, const Src &src, const hf_ray_state &rs,
                                             const hf_trav &r, bool fx, bool fy, uint32_t fxm, uint32_t fym,
                                             uint32_t X0, uint32_t Y0, int L0, float &thi, hf_hit &best) {
    hf_walk w;
    walk_init(w, X0, Y0, L0);
    bool hit_any = false;
    do {
        hit_any |= walk_round<ANY>(f, src, rs, r, fx, fy, fxm, fym, thi, best, w);
    } while (__ballot(!w.fin) != 0ull);
    return hit_any;
}

// wave-wide minimum / maximum of an unsigned value, result scalar (DPP within rows of 16, readlane across rows);
// every lane of the wave must call these
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    uint32_t x = v;
    x = min(x, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) x, 0xB1, 0xF, 0xF, true));  // quad_perm [1,0,3,2]
    x = min(x, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) x, 0x4E, 0xF, 0xF, true));  // quad_perm [2,3,0,1]
    x = min(x, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) x, 0x141, 0xF, 0xF, true)); // row_half_mirror
    x = min(x, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) x, 0x140, 0xF, 0xF, true)); // row_mirror
    const uint32_t a = (uint32_t) __builtin_amdgcn_readlane((int) x, 0), b = (uint32_t) __builtin_amdgcn_readlane((int) x, 16);
    const uint32_t c = (uint32_t) __builtin_amdgcn_readlane((int) x, 32), d = (uint32_t) __builtin_amdgcn_readlane((int) x, 48);
    return min(min(a, b), min(c, d));
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) { return ~wave_min_u32(~v); }

// wave-wide minimum / maximum of a float, result uniform (DPP within rows of 16, readlane across rows); every lane calls
__device__ __forceinline__ float row_min_f32(float v) { // minimum over the lane's row of 16, in every lane of the row
    float x = v;
    x = fminf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, true)));  // quad_perm [1,0,3,2]
    x = fminf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xF, 0xF, true)));  // quad_perm [2,3,0,1]
    x = fminf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x141, 0xF, 0xF, true))); // row_half_mirror
    x = fminf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x140, 0xF, 0xF, true))); // row_mirror
    return x;
}
__device__ __forceinline__ float wave_min_f32(float v) {
    const int xi = __builtin_bit_cast(int, row_min_f32(v));
    const float a = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 0)), b = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 16));
    const float c = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 32)), d = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 48));
    return fminf(fminf(a, b), fminf(c, d));
}
__device__ __forceinline__ float wave_max_f32(float v) { return -wave_min_f32(-v); }
// Four row minima at once, one v_min_f32 with a DPP source per step (the compiler's own code for fminf(x, dpp(x)) is
// a v_mov_dpp, a canonicalising v_max and the v_min: 216 instructions for the sixteen reductions instead of 64).
// The four chains are interleaved, so a DPP read never follows the write of its register by less than the two
// wait states the hardware asks for; the leading s_nop covers the writes before the block.
__device__ __forceinline__ void row_min4_f32(float &a, float &b, float &c, float &d) {
    asm volatile("s_nop 1\n"
                 "v_min_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
                 "v_min_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
                 "v_min_f32_dpp %2, %2, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
                 "v_min_f32_dpp %3, %3, %3 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
                 "v_min_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"
                 "v_min_f32_dpp %1, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"
                 "v_min_f32_dpp %2, %2, %2 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"
                 "v_min_f32_dpp %3, %3, %3 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"
                 "v_min_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n"
                 "v_min_f32_dpp %1, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf\n"
                 "v_min_f32_dpp %2, %2, %2 row_half_mirror row_mask:0xf bank_mask:0xf\n"
                 "v_min_f32_dpp %3, %3, %3 row_half_mirror row_mask:0xf bank_mask:0xf\n"
                 "v_min_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n"
                 "v_min_f32_dpp %1, %1, %1 row_mirror row_mask:0xf bank_mask:0xf\n"
                 "v_min_f32_dpp %2, %2, %2 row_mirror row_mask:0xf bank_mask:0xf\n"
                 "v_min_f32_dpp %3, %3, %3 row_mirror row_mask:0xf bank_mask:0xf\n"
                 "s_nop 1\n"
                 : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}
// Sixteen wave-wide minima for the price of sixteen row reductions (DPP) and one pass through LDS: the first lane
// of each row of 16 parks its row's sixteen minima (four 16-byte writes), lane q < 16 then combines the four rows of
// quantity q.  `red` = 64 floats of the wave's own LDS.  Result: quantity q in lane q (other lanes: undefined).
__device__ __forceinline__ float wave_min16(const float (&h)[16], uint32_t lane, float *red) {
    float rm[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) rm[q] = h[q];
#pragma unroll
    for (int q = 0; q < 16; q += 4) row_min4_f32(rm[q], rm[q + 1], rm[q + 2], rm[q + 3]);
    if ((lane & 15u) == 0u) {
        float4 *dst = (float4 *) (red + (lane & 48u)); // row r -> red[16 r ..]
        dst[0] = make_float4(rm[0], rm[1], rm[2], rm[3]); dst[1] = make_float4(rm[4], rm[5], rm[6], rm[7]);
        dst[2] = make_float4(rm[8], rm[9], rm[10], rm[11]); dst[3] = make_float4(rm[12], rm[13], rm[14], rm[15]);
    }
    __builtin_amdgcn_wave_barrier();
    const uint32_t q = lane & 15u;
    const float v = fminf(fminf(red[q], red[16 + q]), fminf(red[32 + q], red[48 + q]));
    __builtin_amdgcn_wave_barrier();
    return v;
}

// ---------------------------------------------------------------------------------
// ITEM WALK (round 4): the subtrees below the beam sweep's hand-off nodes as a wave-wide work list instead of 64 private
// depth-first walks.  The per-lane walk left most of the wave idle -- a visit ran with 19 of 64 lanes, a cell round with
// 13 -- because every converged round lasts until its slowest lane has made its step, and a lane's steps are a
// dependent chain (rays that skim the surface crawl from 2x2-cell node to node).  Here a unit of work is an ITEM,
// (ray, node) or (ray, cell), on one of two stacks in the wave's LDS: the lanes that take a hand-off node push the
// children they are to visit (ballot + mbcnt prefix per child slot), and every round the wave pops up to 64 node items
// -- of any level: a visit is the same code at every level -- or up to 64 cell items.  Any lane takes any item: it
// pulls the ray's traversal constants from the owning lane's registers (ds_bpermute, no copy of the ray in LDS),
// evaluates the node's record exactly as a per-lane visit did (same shear_line / child_mask arithmetic) and pushes the
// children that pass; a cell item runs the two-triangle test and merges its hit into the ray's entry of an LDS table
// with one 64-bit minimum -- key = (t bits, ~prim_index): the closest hit, the higher primitive on a tie, what the
// brute-force loop produces (kdtree.h:2424-2448).  A crawling ray's chain is thereby spread over the idle lanes, and
// the hand-off nodes of a pass are worked off TOGETHER: items are pushed node after node and the list runs when it
// holds a wave's worth (or the pass ends), so a node that only a handful of lanes take no longer costs a walk of its
// own.  What is lost is front-to-back pruning between the children of a node and between the nodes of one run (t_hi
// takes effect at the next pop, after a cell round) -- harmless for the result (a minimum over a superset of the
// cells) and cheap while the extra items ride in lanes that would have idled.
// Round selection: cell tests when a full round of them is waiting or no node item is left, visits otherwise (so the
// cell stack never holds more than 63 + 4 x 64 items); a visit round takes fewer than 64 items when the children
// they may push (four each) would not fit the node stack -- down to one item per round, a plain depth-first walk whose
// stack grows by at most three per level -- so neither capacity is ever exceeded whatever the rays do.
#define HF_NODE_CAP (HF_ITEM_FLUSH + 4 * 64 + 12 + 20) // a candidate of the sweep pushes up to 4 x 64 items onto fewer than HF_ITEM_FLUSH waiting
                                                      // ones, and items_run needs 12 spare entries on top (one-item rounds grow the stack by up to 6)
#define HF_CELL_CAP 320
#ifndef HF_ITEM_FLUSH
#define HF_ITEM_FLUSH 32 // the list runs when it holds this many node items (or the pass ends)
#endif
struct hf_items_lds {
    unsigned long long best[64]; // per ray of the batch: (t bits << 32) | ~prim_index of its closest hit so far; all ones = none
    float2 uv[64];               // barycentrics of that hit
    // items: x | y << 4 (node / cell relative to its hand-off node, order space) | level << 8 | ray << 10 | slot << 16
    // (slot: the hand-off node's lane in the pass of the beam sweep)
    uint32_t nodes[HF_NODE_CAP + HF_CELL_CAP]; // the node stack, then the cell stack
};
__device__ __forceinline__ float bperm_f(int src4, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src4, __builtin_bit_cast(int, v)));
}
__device__ __forceinline__ uint32_t mbcnt64(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0u));
}
__device__ __forceinline__ void items_clear(hf_items_lds *q, uint32_t lane) {
    // (opaque: the pair of all-ones registers is otherwise hoisted out of the kernel's persistent loop and spilled)
    uint32_t ones = 0xFFFFFFFFu;
    asm volatile("" : "+v"(ones));
    q->best[lane] = ((unsigned long long) ones << 32) | (unsigned long long) ones;
}
// the lane's own ray: closest hit of the item walks so far -> `best` (minimum t, higher prim on a tie)
__device__ __forceinline__ void items_fold(hf_items_lds *q, uint32_t lane, hf_hit &best) {
    __builtin_amdgcn_wave_barrier();
    const unsigned long long mk = q->best[lane];
    if (mk != ~0ull) {
        const float2 uv = q->uv[lane];
        best_update(best, __builtin_bit_cast(float, (uint32_t) (mk >> 32)), uv.x, uv.y, ~(uint32_t) mk);
    }
}
// wave-wide inclusive prefix sum (DPP: shifts within rows of 16, then the row totals broadcast into the rows above)
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v) {
    int x = (int) v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, false); // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, false); // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, false); // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, false); // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false); // row_bcast:15 -> rows 1, 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false); // row_bcast:31 -> rows 2, 3
    return (uint32_t) x;
}
// Every lane pushes the children (order-space mask m4; 0: none) of its node as items of level lvc, far child first:
// onto the cell stack where cell_item, the node stack otherwise.  One prefix sum places everybody (node counts in the low
// half word, cell counts in the high one): ballot-free, 4 predicated LDS writes.  tag = ray << 10 | slot << 16.
__device__ __forceinline__ void push_children(hf_items_lds *q, uint32_t &nn, uint32_t &ncell, uint32_t m4, bool cell_item,
                                              uint32_t tag, uint32_t lvc, uint32_t x2, uint32_t y2) {
    const uint32_t c = (uint32_t) __builtin_popcount(m4);
    const uint32_t cp = cell_item ? c << 16 : c;
    const uint32_t inc = wave_scan_add(cp);
    const uint32_t tot = (uint32_t) __builtin_amdgcn_readlane((int) inc, 63);
    const uint32_t ex = inc - cp;
    // (one array: the cell stack follows the node stack, see hf_items_lds)
    uint32_t at = cell_item ? (uint32_t) HF_NODE_CAP + ncell + (ex >> 16) : nn + (ex & 0xFFFFu);
    const uint32_t base = (lvc << 8) | tag;
#pragma unroll
    for (int k = 3; k >= 0; --k)
        if ((m4 >> k) & 1u) q->nodes[at++] = (x2 + (uint32_t) (k & 1)) | ((y2 + (uint32_t) (k >> 1)) << 4) | base;
    nn += tot & 0xFFFFu; ncell += tot >> 16;
}
// Works the node stack (nn items) off.  All 64 lanes call this (wave-uniform control flow).  The hand-off node of an
// item is the node of lane `slot` of the current pass of the beam sweep: slab sb0 + slot / 4, cross coordinate nc of
// that lane (xm: slabs run along x); fx, fy: the wave's mirror flags.
static_assert(HF_ITEM_FLUSH - 1 + 4 * 64 <= HF_NODE_CAP - 12, "node stack: a candidate's children on top of the waiting items");
static_assert(63 + 4 * 64 <= HF_CELL_CAP, "cell stack: a round of level-1 visits on top of less than a round of cells");
template <bool ANY>
__device__ __forceinline__ void items_run(const hf_dev_field &f, const hf_ray_state &rs, float dxo, float dyo, bool fx, bool fy,
                                          bool xm, uint32_t sb0, uint32_t nc, uint32_t nn, float &thi, hf_items_lds *q, uint32_t lane) {
    const hf_trav &r = rs.r;
    const int top = f.top;
    const uint32_t fxm = fx ? ((1u << top) - 1u) : 0u, fym = fy ? ((1u << top) - 1u) : 0u;
    uint32_t nc_ = 0u; // cell items
    while ((nn | nc_) != 0u) { // wave-uniform
        WCOUNT(3);
        __builtin_amdgcn_wave_barrier(); // (same wave: LDS operations stay in order; this keeps the compiler from reordering them)
        if (nn != 0u && nc_ < 64u) {
            // ---- a round of visits: up to 64 node items from the top of the node stack ----
            uint32_t n = min(nn, 64u);
            {   // room for the (at most three per popped item, net) node items the round may add
                const int32_t room = (int32_t) HF_NODE_CAP - 12 - (int32_t) nn;
                n = min(n, max(room > 0 ? (uint32_t) room / 3u : 0u, 1u));
            }
            const bool mine = lane < n;
            const uint32_t it = mine ? q->nodes[nn - 1u - lane] : (lane << 10);
            nn -= n;
            const int src4 = (int) (((it >> 10) & 63u) << 2);
            const uint32_t slot = (it >> 16) & 63u;
            hf_trav rr;
            rr.gxm = bperm_f(src4, r.gxm); rr.gxp = bperm_f(src4, r.gxp); rr.gym = bperm_f(src4, r.gym); rr.gyp = bperm_f(src4, r.gyp);
            rr.gz = bperm_f(src4, r.gz); rr.dz = bperm_f(src4, r.dz); rr.idx = bperm_f(src4, r.idx); rr.idy = bperm_f(src4, r.idy);
            rr.mz = bperm_f(src4, r.mz);
            const float rdxo = bperm_f(src4, dxo), rdyo = bperm_f(src4, dyo), rthi = bperm_f(src4, thi);
            const uint32_t ck = (uint32_t) __builtin_amdgcn_ds_bpermute((int) (slot << 2), (int) nc), sk = sb0 + (slot >> 2);
            uint32_t m4 = 0u;
            const uint32_t lv = (it >> 8) & 3u, x = it & 15u, y = (it >> 4) & 15u; // lv: 1 .. HF_SUBTREE_LEVEL - 1
            if (mine) {
                const uint32_t X0 = xm ? sk : ck, Y0 = xm ? ck : sk;
                const uint32_t X = (X0 << ((uint32_t) HF_SUBTREE_LEVEL - lv)) + x, Y = (Y0 << ((uint32_t) HF_SUBTREE_LEVEL - lv)) + y;
                const float S = (float) (1u << lv), Sc = 0.5f * S;
                // the item may predate a hit: its entry against the ray's current t_hi (any hit: a ray that has hit holds -1)
                const float te = fmaxf(((float) X * S - rr.gxm) * rr.idx, ((float) Y * S - rr.gym) * rr.idy);
                if (te <= rthi && (!ANY || rthi >= 0.f)) {
                    WCOUNT(5); WLANES(7, 0); WHIST(11);
                    const uint32_t ix = X ^ (fxm >> lv), iy = Y ^ (fym >> lv);
                    const uint32_t k = (uint32_t) top - lv;
                    const float4 *rec = f.shear + (size_t) (hf_depth_off((int) k) - 1u + (iy << k) + ix) * 3;
                    const float4 pl4 = rec[0], q01 = rec[1], q23 = rec[2]; // one round trip: the three parts are requested together
                    float gz, dz, mz;
                    shear_line_v(rr, rdxo, rdyo, HF_LINE_EPS * (float) (1 << top), fx, fy, pl4.x, pl4.y, pl4.z, pl4.w,
                                 __builtin_fmaf((float) X, S, Sc), __builtin_fmaf((float) Y, S, Sc), gz, dz, mz);
                    hf_quad qd;
                    qd.lo[0] = q01.x; qd.hi[0] = q01.y; qd.lo[1] = q01.z; qd.hi[1] = q01.w;
                    qd.lo[2] = q23.x; qd.hi[2] = q23.y; qd.lo[3] = q23.z; qd.hi[3] = q23.w;
                    m4 = to_order(child_mask(rr, fx, fy, (float) X * S, (float) Y * S, Sc, qd, gz, dz, mz, rthi), fx, fy);
                }
            }
            const uint32_t tag = it & 0x3FFC00u; // ray and slot
            push_children(q, nn, nc_, m4, lv == 1u, tag, lv - 1u, 2u * x, 2u * y); // (m4 = 0 in the lanes without an item)
            TSTAMP(4); // visit rounds
        } else {
            // ---- a round of cell tests: up to 64 cell items from the top of the cell stack ----
            const uint32_t n = min(nc_, 64u);
            const bool mine = lane < n;
            const uint32_t it = mine ? q->nodes[(uint32_t) HF_NODE_CAP + nc_ - 1u - lane] : (lane << 10);
            nc_ -= n;
            const uint32_t ray = (it >> 10) & 63u, slot = (it >> 16) & 63u;
            const int src4 = (int) (ray << 2);
            const v3 oo = mk3(bperm_f(src4, rs.oo.x), bperm_f(src4, rs.oo.y), bperm_f(src4, rs.oo.z));
            const v3 od = mk3(bperm_f(src4, rs.od.x), bperm_f(src4, rs.od.y), bperm_f(src4, rs.od.z));
            const float rmaxt = bperm_f(src4, rs.maxt);
            const float rthi = ANY ? bperm_f(src4, thi) : 0.f;
            const uint32_t ck = (uint32_t) __builtin_amdgcn_ds_bpermute((int) (slot << 2), (int) nc), sk = sb0 + (slot >> 2);
            hf_hit b;
            b.hit = false; b.t = __builtin_inff(); b.u = 0.f; b.v = 0.f; b.prim = 0u;
            unsigned long long key = ~0ull;
            if (mine && (!ANY || rthi >= 0.f)) {
                WCOUNT(6); WLANES(7, 16); WHIST(8);
                const uint32_t X0 = xm ? sk : ck, Y0 = xm ? ck : sk, x = it & 15u, y = (it >> 4) & 15u;
                const int cxx = (int) (((X0 << HF_SUBTREE_LEVEL) + x) ^ fxm), cyy = (int) (((Y0 << HF_SUBTREE_LEVEL) + y) ^ fym);
                // (32-bit byte offsets from the uniform base: hf_create limits the grid to 2^30 vertices)
                const uint32_t off = ((uint32_t) cyy * (uint32_t) f.W + (uint32_t) cxx) << 2, pitch = (uint32_t) f.W << 2;
                const char *hb = (const char *) f.h;
                const float z00 = *(const float *) (hb + off) * f.s, z10 = *(const float *) (hb + off + 4u) * f.s;
                const float z01 = *(const float *) (hb + off + pitch) * f.s, z11 = *(const float *) (hb + off + pitch + 4u) * f.s;
                if (test_cell(f, cxx, cyy, z00, z10, z01, z11, oo, od, rmaxt, b)) {
                    key = ((unsigned long long) __builtin_bit_cast(uint32_t, b.t) << 32) | (unsigned long long) (~b.prim);
                    atomicMin(&q->best[ray], key);
                }
            }
            __builtin_amdgcn_wave_barrier();
            if (b.hit && q->best[ray] == key) q->uv[ray] = make_float2(b.u, b.v); // the (unique) winner's barycentrics
            __builtin_amdgcn_wave_barrier();
            // every lane: its own ray's closest hit so far bounds what is left of its segment
            const unsigned long long mk = q->best[lane];
            if (mk != ~0ull) {
                float tb = __builtin_bit_cast(float, (uint32_t) (mk >> 32)) - rs.tin;
                tb = tb + __builtin_fabsf(tb) * 1e-6f + 1e-30f;
                thi = ANY ? -1.f : fminf(thi, tb);
            }
            TSTAMP(5); // cell rounds
        }
    }
}

// Coherent wave, upper levels by BEAM SWEEP.  The row sweep above pays per enumerated node: a uniform (scalar) load of
// its box, whose latency nothing hides, a per-lane box test and a ballot -- 16.8 nodes per batch of which 4.2 are
// entered, and 7.8 rows with two wave reductions each: a fifth of a traversing batch's instructions.  Here the
// lanes of the wave act as NODE testers first: the wave's rays are bounded by a beam (wave-wide extrema of the
// per-lane slab coefficients: any lane's parameter interval in a node lies inside the beam's, any lane's height
// inside the beam's height range over it), 16 rows x 4 node slots of the hand-off level are assigned to the 64
// lanes front to back, every lane loads ITS node's box and record in one round trip (addresses do not depend on
// loaded data), tests the beam against the box and parks box + record in the wave's LDS table.  The nodes that
// survive (a ballot: bit order = front-to-back order) are then taken one by one: box and record come back from
// LDS at a uniform address, every lane tests its own fat ray against the box with the row sweep's arithmetic, the
// node's record is evaluated for all lanes at once (the first visit of the hand-off, hoisted: a node the rays only
// skim is dropped here), and the lanes with children to visit walk them.  The beam test only removes nodes that no
// lane's own test would accept, so the visited set -- and the result -- is the row sweep's.
#ifndef HF_BEAM_ROWS
#define HF_BEAM_ROWS 16 // slabs per pass (x 4 node slots per slab = the 64 lanes; fewer: the upper lanes sit the enumeration out)
#endif
// The slabs are cut across the beam's MAJOR direction (rows of the level when the rays advance faster in y, columns
// when faster in x), so that a slab holds few nodes whatever the view: at most four, or the sweep declines.
// Front-to-back either way: a monotone ray that visits slab s before s' has s' > s, and inside a slab the cross
// coordinate only grows.
#define HF_BEAM_CAND (4 * HF_BEAM_ROWS)
struct hf_beam_lds {
    struct { float4 pl, q01, q23; } e[HF_BEAM_CAND]; // record of the pass's nodes ...
    float2 box[HF_BEAM_CAND];                          // ... and their (min z, max z)
    float hdr[20];               // the beam (wave-uniform), parked here between passes instead of in registers; [16] = largest xy margin
};
enum { BM_ISN, BM_ISX, BM_ICN, BM_ICX, BM_AS, BM_BS, BM_AC, BM_BC, BM_GCLO, BM_GCHI, BM_DCN, BM_DCX, BM_ZLO, BM_ZHI, BM_DZN, BM_DZX };
// Returns false when it gives up -- an axis-parallel ray in the wave, or a beam wider than four nodes (rays that fan
// out over a long path) -- at the start or between two passes: the caller then lets every live lane walk from the
// root with the t_hi and the best hit reached so far (re-testing a cell is harmless: the result is a minimum).
template <bool ANY>
__device__ __forceinline__ bool walk_beam_impl(const hf_dev_field &f, const hf_ray_state &rs, bool alive, bool fx, bool fy,
                                               float &thi, hf_beam_lds *lds, hf_items_lds *items) {
    const hf_trav &r = rs.r;
    // (opaque copies: everything derived from the lane number or the level count is loop-invariant for the kernel's
    // persistent loop, and the compiler would compute it all at kernel entry and then spill it -- 30 registers)
    int top = f.top;
    asm volatile("" : "+s"(top));
    uint32_t lane = threadIdx.x & 63u;
    asm volatile("" : "+v"(lane));
    const uint32_t kd = (uint32_t) (top - HF_SUBTREE_LEVEL), nn = 1u << kd;
    const float S = (float) (1u << HF_SUBTREE_LEVEL), iS = 1.0f / S, lim = (float) nn - 0.5f;
    const float inf = __builtin_inff();
    const float dxo = __builtin_fabsf(rs.od.x) * f.hx, dyo = __builtin_fabsf(rs.od.y) * f.hy;
    // slab axis s / cross axis c (wave-uniform choice from the first live lane; any choice is correct)
    const int first = __builtin_ctzll(__ballot(alive));
    const bool xm = __builtin_amdgcn_readlane((int) (dxo > dyo), first) != 0;
    uint32_t smin, smax;
    {
        // ---- the beam: wave-wide extrema, all as minima (a maximum is the negated minimum of the negated value; dead
        // lanes contribute +inf) ----
        const float gsm = xm ? r.gxm : r.gym, gsp = xm ? r.gxp : r.gyp, ids = xm ? r.idx : r.idy, dso = xm ? dxo : dyo;
        const float gcm = xm ? r.gym : r.gxm, gcp = xm ? r.gyp : r.gxp, idc = xm ? r.idy : r.idx, dco = xm ? dyo : dxo;
        float h[16];
        h[BM_ISN] = ids; h[BM_ISX] = -ids; h[BM_ICN] = idc; h[BM_ICX] = -idc;
        h[BM_AS] = -(gsm * ids); h[BM_BS] = gsp * ids; h[BM_AC] = -(gcm * idc); h[BM_BC] = gcp * idc;
        h[BM_GCLO] = gcp; h[BM_GCHI] = -gcm; h[BM_DCN] = dco; h[BM_DCX] = -dco;
        h[BM_ZLO] = r.gz - r.mz; h[BM_ZHI] = -(r.gz + r.mz); h[BM_DZN] = r.dz; h[BM_DZX] = -r.dz;
#pragma unroll
        for (int q = 0; q < 16; ++q) h[q] = alive ? h[q] : inf;
        const float hv = wave_min16(h, lane, (float *) &lds->e[0]); // (the node table is not in use yet)
        // an axis-parallel ray in the wave (1/d = inf): decline
        const float isx = -__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, hv), BM_ISX));
        const float icx = -__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, hv), BM_ICX));
        if (!(isx < inf) || !(icx < inf)) return false;
        if (lane < 16u) lds->hdr[lane] = hv;
        // slabs the wave's rays can touch: [g - m, g + m + t_hi d] per lane, widened by the slack of this estimate
        const float sa = gsp - 1e-3f, sb = __builtin_fmaf(thi, dso, gsm);
        const float sb2 = sb + 1e-3f + 1e-6f * sb;
        {   // largest xy margin of the wave's rays: the needle term of the beam's box test is m x (height range of the box)
            const float mmax = wave_max_f32(alive ? rs.m : 0.f);
            if (lane == 0u) lds->hdr[16] = mmax;
        }
        smin = wave_min_u32(alive ? (uint32_t) fminf(fmaxf(sa * iS, 0.f), lim) : 0xFFFFFFFFu);
        smax = wave_max_u32(alive ? (uint32_t) fminf(fmaxf(sb2 * iS, 0.f), lim) : 0u);
    }
    TSTAMP(1); // beam set-up: sixteen wave-wide extrema, slab range
    for (uint32_t sb0 = smin; sb0 <= smax; sb0 += HF_BEAM_ROWS) { // wave-uniform
        WCOUNT(0);
        __builtin_amdgcn_wave_barrier();
        // ---- this lane's node of the pass: slab sb0 + lane / 4, slot lane % 4 of the beam's node range in that slab ----
        uint32_t nc; // the node's cross coordinate (its slab number follows from the lane)
        bool cand = false;
        {
            const float4 h0 = *(const float4 *) &lds->hdr[0], h1 = *(const float4 *) &lds->hdr[4];
            const float4 h2 = *(const float4 *) &lds->hdr[8], h3 = *(const float4 *) &lds->hdr[12];
            const float isn = h0.x, isx = -h0.y, icn = h0.z, icx = -h0.w, as = -h1.x, bs = h1.y, ac = -h1.z, bc = h1.w;
            const float gclo = h2.x, gchi = -h2.y, dcn = h2.z, dcx = -h2.w, zlo = h3.x, zhi = -h3.y, dzn = h3.z, dzx = -h3.w;
            const float T = wave_max_f32(thi);
            const uint32_t sl = sb0 + (lane >> 2);
            const float fS = (float) sl * S;
            const float t0 = fmaxf(fS * isn - as, 0.f), t1 = fminf((fS + S) * isx - bs, T);
            const float t0s = fmaxf(t0 - (1e-5f * t0 + 1e-5f), 0.f), t1s = t1 + (1e-5f * t1 + 1e-5f); // rounding of the beam's own arithmetic
            const bool in_slab = (HF_BEAM_CAND >= 64 || lane < (uint32_t) HF_BEAM_CAND) & (sl <= smax) & (t0s <= t1s);
            const float ca = __builtin_fmaf(t0s, dcn, gclo) - 1e-3f, cb = __builtin_fmaf(t1s, dcx, gchi);
            const float cb2 = cb + 1e-3f + 1e-6f * cb;
            const uint32_t c0 = (uint32_t) fminf(fmaxf(ca * iS, 0.f), lim), c1 = (uint32_t) fminf(fmaxf(cb2 * iS, 0.f), lim);
            if (__ballot(in_slab && c1 - c0 > 3u) != 0ull) return false; // a beam wider than four nodes
            const uint32_t cc = c0 + (lane & 3u);
            const bool valid = in_slab & (cc <= c1);
            const uint32_t i = xm ? sl : cc, j = xm ? cc : sl;
            nc = cc;
            if (valid) {
                const uint32_t ai = fx ? nn - 1u - i : i, aj = fy ? nn - 1u - j : j;
                const uint32_t node = (aj << kd) + ai;
                const float2 box = (f.mip + hf_depth_off((int) kd))[node];
                const float4 *rec = f.shear + ((size_t) (hf_depth_off((int) kd) - 1u) + node) * 3;
                const float4 pl = rec[0], q01 = rec[1], q23 = rec[2];
                const float fC = (float) cc * S;
                float u0 = fmaxf(fmaxf(fS * isn - as, fC * icn - ac), 0.f), u1 = fminf(fminf((fS + S) * isx - bs, (fC + S) * icx - bc), T);
                u0 = fmaxf(u0 - (1e-5f * u0 + 1e-5f), 0.f); u1 = u1 + (1e-5f * u1 + 1e-5f);
                const float za = zlo + fminf(u0 * dzn, u1 * dzn), zb = zhi + fmaxf(u0 * dzx, u1 * dzx);
                const float zs = __builtin_fmaf(2.f * lds->hdr[16], box.y - box.x, 1e-5f * (__builtin_fabsf(za) + __builtin_fabsf(zb)) + 1e-30f);
                cand = (u0 <= u1) & (za - zs <= box.y) & (zb + zs >= box.x);
                if (cand) {
                    lds->box[lane] = box;
                    lds->e[lane].pl = pl; lds->e[lane].q01 = q01; lds->e[lane].q23 = q23;
                }
            }
        }
        uint64_t cm = __ballot(cand);
        TSTAMP(2); // a pass: node assignment, box + record loads, beam test, LDS table
        __builtin_amdgcn_wave_barrier(); // the table is read below by every lane (same wave: LDS operations stay in order)
        // One loop with ONE walk site at its end: a lane that takes a node notes it (node + children packed in one
        // register: hf_create allows at most 2^11 nodes per side at this level) and the walk below runs at once.  The
        // shape matters more than it should: the same sweep with the walk inside the candidate's own branch spills 13
        // registers in the fused kernel instead of 2 (2.90-3.00 vs 2.71 ms, profiles/r03_ab/r03_v2).  Holding the nodes
        // of a pass and walking them together when a holder wants a second one was measured too: a lane that will hit in
        // its node still passes the box and record tests of the nodes behind it, so nearly every node flushes -- 2.1
        // instead of 2.2 walks, 9.2 instead of 6.8 box tests, 2.80 ms.
        // The candidates front to back: box test and record per lane, the children a lane is to visit go onto the wave's
        // work list; the list runs (items_run) when it holds a wave's worth of items or the pass ends.  (Until round 4 a
        // node was walked at once by the lanes that took it, each lane on its own: 2.2 walks per batch with half of the
        // lanes in each, every one as long as its slowest lane.)
        uint32_t nn = 0u; // node items waiting
        bool done = false;
        while (cm != 0ull) { // wave-uniform
            const uint32_t k = (uint32_t) __builtin_ctzll(cm);
            WCOUNT(1);
            const uint32_t ck = (uint32_t) __builtin_amdgcn_readlane((int) nc, (int) k), sk = sb0 + (k >> 2);
            const uint32_t ci = xm ? sk : ck, nodej = xm ? ck : sk;
            const float2 cbox = lds->box[k]; // uniform address: broadcast
            // ---- per-lane test of the node's box with the row sweep's arithmetic ----
            const float fXc = (float) ci * S, fYc = (float) nodej * S;
            const float xlo = (fXc - r.gxm) * r.idx, xhi = (fXc + S - r.gxp) * r.idx;
            const float ylo = (fYc - r.gym) * r.idy, yhi = (fYc + S - r.gyp) * r.idy;
            const float u0 = fmaxf(fmaxf(xlo, ylo), 0.f), u1 = fminf(fminf(xhi, yhi), thi);
            const float za = __builtin_fmaf(u0, r.dz, r.gz), zb = __builtin_fmaf(u1, r.dz, r.gz);
            const float bz = __builtin_fmaf(2.f * rs.m, cbox.y - cbox.x, r.mz); // needle term: 2 m x (range), see hf_shear_kernel
            const bool mine = (u0 <= u1) & (fminf(za, zb) - bz <= cbox.y) & (fmaxf(za, zb) + bz >= cbox.x);
            cm &= cm - 1ull;
            if (__ballot(mine) == 0ull) {
                // nobody overlaps this node; done when nobody can reach its slab -- or any later one -- before its t_hi
                // (a t_hi that waiting items have yet to shorten only delays this)
                const float tsk = ((float) sk * S - (xm ? r.gxm : r.gym)) * (xm ? r.idx : r.idy);
                if (__ballot(tsk <= thi) == 0ull) { done = true; cm = 0ull; }
            } else {
                WCOUNT(2);
                // the node's own record, for all lanes at once (the first visit of the hand-off, hoisted)
                const float4 pl = lds->e[k].pl, q01 = lds->e[k].q01, q23 = lds->e[k].q23;
                const float Sc = 0.5f * S;
                float gz, dz, mz;
                shear_line_v(r, dxo, dyo, HF_LINE_EPS * (float) (1 << top), fx, fy, pl.x, pl.y, pl.z, pl.w, fXc + Sc, fYc + Sc, gz, dz, mz);
                hf_quad q;
                q.lo[0] = q01.x; q.hi[0] = q01.y; q.lo[1] = q01.z; q.hi[1] = q01.w;
                q.lo[2] = q23.x; q.hi[2] = q23.y; q.lo[3] = q23.z; q.hi[3] = q23.w;
                const uint32_t m4 = child_mask(r, fx, fy, fXc, fYc, Sc, q, gz, dz, mz, thi);
                const uint32_t cur0 = mine ? to_order(m4, fx, fy) : 0u;
                if (__ballot(cur0 != 0u) != 0ull) WCOUNT(4);
                {
                    uint32_t no_cells = 0u;
                    push_children(items, nn, no_cells, cur0, false, (lane << 10) | (k << 16), (uint32_t) (HF_SUBTREE_LEVEL - 1), 0u, 0u);
                }
            }
            // ---- the work list: when it holds a wave's worth, and before the pass ends ----
            if (nn >= (uint32_t) HF_ITEM_FLUSH || (cm == 0ull && nn != 0u)) {
                TSTAMP(3); // candidates: per-lane box tests, hoisted records, pushes
                items_run<ANY>(f, rs, dxo, dyo, fx, fy, xm, sb0, nc, nn, thi, items, lane);
                nn = 0u;
                if (ANY && __ballot(thi >= 0.f) == 0ull) return true;
            }
        }
        if (done) return true;
        // done when nobody can reach the first slab of the next pass before its t_hi
        const float gsm = xm ? r.gxm : r.gym, ids = xm ? r.idx : r.idy;
        const float tsn = ((float) (sb0 + HF_BEAM_ROWS) * S - gsm) * ids;
        if (__ballot(tsn <= thi) == 0ull) break;
    }
    return true;
}

// the beam sweep with the item walk's hit table around it: cleared before, folded into `best` after (every exit)
template <bool ANY>
__device__ __forceinline__ bool walk_beam(const hf_dev_field &f, const hf_ray_state &rs, bool alive, bool fx, bool fy,
                                          hf_hit &best, float &thi, hf_beam_lds *lds, hf_items_lds *items) {
    const uint32_t lane = threadIdx.x & 63u;
    items_clear(items, lane);
    const bool done = walk_beam_impl<ANY>(f, rs, alive, fx, fy, thi, lds, items);
    items_fold(items, lane, best);
    return done;
}

// ---------------------------------------------------------------------------------
// Warped-area reparameterisation (include/hf.h; reparam.py:10-123,224-333): per-sample kernels
// ---------------------------------------------------------------------------------
__host__ __device__ __forceinline__ void tea32(uint32_t v0, uint32_t v1, uint32_t &o0, uint32_t &o1) { // random.h:76-91
    uint32_t sum = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sum += 0x9e3779b9u;
        v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + sum) ^ ((v1 >> 5) + 0xc8013ea4u);
        v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + sum) ^ ((v0 >> 5) + 0x7e95761eu);
    }
    o0 = v0; o1 = v1;
}

struct hf_aux_sample {
    v3 omega;     // square_to_von_mises_fisher(sample, kappa), xy negated on the flipped half of a pair
    float sy;     // sample.y
    v3 fs, ft;    // Frame3f(d): s, t (n = d)
};
__device__ __forceinline__ void aux_sample(const hf_reparam_args &a, size_t i, v3 d, hf_aux_sample &q) {
    const uint32_t pair = a.antithetic ? (a.k >> 1) : a.k;
    // The stream of a sample: (seed, pair) hashed TOGETHER (added, the streams of seed s, pair p and seed s + 1,
    // pair p - 1 were the same one), keyed by the ray's id -- its index in the launch, or ray_id[i] when the caller
    // says which ray of a larger wavefront this is (a rank's tiles of a partitioned wavefront: the sharded launch then
    // draws the samples of the unsharded one).
    uint32_t key, unused, r0, r1;
    tea32(a.seed, pair, key, unused);
    tea32(key, a.ray_id ? a.ray_id[i] : (uint32_t) i, r0, r1);
    const float sx = (float) (r0 >> 9) * (1.0f / 8388608.0f), sy = (float) (r1 >> 9) * (1.0f / 8388608.0f);
    // warp.h:557-566
    const float syc = fmaxf(1.f - sy, 1e-6f);
    const float cos_theta = 1.f + logf(__builtin_fmaf(1.f - syc, expf(-2.f * a.kappa), syc)) / a.kappa;
    float sn, cs;
    sincospif(2.f * sx, &sn, &cs); // sin / cos of 2 pi sx without the range reduction of a radian argument
    const float sin_theta = __builtin_sqrtf(fmaxf(1.f - cos_theta * cos_theta, 0.f));
    const bool flip = a.antithetic && ((a.k & 1u) == 0u); // reparam.py:83-85,189
    q.omega = mk3(flip ? -(cs * sin_theta) : cs * sin_theta, flip ? -(sn * sin_theta) : sn * sin_theta, cos_theta);
    q.sy = sy;
    coordinate_system(d, q.fs, q.ft);
}
// Frame3f::to_world (frame.h:39-41)
__device__ __forceinline__ v3 frame_to_world(const hf_aux_sample &q, v3 n, v3 v) {
    return mk3(__builtin_fmaf(n.x, v.z, __builtin_fmaf(q.ft.x, v.y, q.fs.x * v.x)),
               __builtin_fmaf(n.y, v.z, __builtin_fmaf(q.ft.y, v.y, q.fs.y * v.x)),
               __builtin_fmaf(n.z, v.z, __builtin_fmaf(q.ft.z, v.y, q.fs.z * v.x)));
}

// record stores are write-once streams (72 B/ray): non-temporal, so that they do not push the mip
// and height lines of concurrently traversing waves out of L2.  Address = (row + ub) + lo: uniform base, lane offset.
__device__ __forceinline__ void st(float *p, size_t ub, uint32_t lo, float v) { if (p) __builtin_nontemporal_store(v, &(p + ub)[lo]); }
typedef float f4 __attribute__((ext_vector_type(4)));
// four consecutive entries of a row per lane (the wide path): (row + ub) as 16-byte elements, lane offset l4
__device__ __forceinline__ void st4(float *p, size_t ub, uint32_t l4, f4 v) { if (p) __builtin_nontemporal_store(v, &((f4 *) (p + ub))[l4]); }
#define st3(p, ub, lo, v) do { st((p)[0], ub, lo, (v).x); st((p)[1], ub, lo, (v).y); st((p)[2], ub, lo, (v).z); } while (0)

#ifndef HF_GRAB
#define HF_GRAB 256 // most rays a wave takes from the work counter per fetch (hf_grab_for); 512 before the per-XCD counters
#endif
// Scratch block of one trace launch (zeroed by hf_launch_trace): the per-XCD work counters.
#define HF_SCR_BYTES 1024
#ifndef HF_PRIO
#define HF_PRIO 1     // s_setprio of a batch's traversal (0: off) ...
#endif
#ifndef HF_PRIO_OUT
#define HF_PRIO_OUT 0 // ... and of its output phase; the wide path runs at 0
#endif
#ifndef HF_COH_WINDOW
#define HF_COH_WINDOW 32.f // a wave is coherent when its entry points are within this many cells of the first live lane's
#endif
#ifndef HF_COH_DIR
#define HF_COH_DIR 0.05f   // ... and the xy direction ratios within this relative distance
#endif
#ifndef HF_TRACE_WAVES_FUSED
#define HF_TRACE_WAVES_FUSED 5 // ... of the fused mode: its surface-interaction tail needs ~100 registers (6 waves: 30 spills, slower)
#endif
#ifndef HF_TRACE_WAVES
#define HF_TRACE_WAVES 5 // resident waves per SIMD = workgroups per CU of the traversal kernel (96 VGPRs; 6 waves = 80 VGPRs spill 40 of them since the beam sweep: closest hit 2.76 vs 2.29 ms)
#endif
#define HF_NUM_XCD 8u // work counters per launch, one per XCD (power of two)
#define HF_COUNTER_STRIDE 16u // in counters: 128 bytes apart

// the one kernel argument (kernarg segment offset 0)
struct hf_trace_args {
    hf_dev_field f;
    size_t n;
    hf_rays_t rays;
    const uint8_t *active;
    hf_pi_t pi;
    uint8_t *hit_out;
    hf_si_t sio;
    uint32_t flags;
    uint32_t grab; // rays per fetch, a multiple of 64
    uint32_t wide; // every ray / record row is 16-byte aligned and there is no `active` mask: fetches that miss the bound as a whole take the wide path
    unsigned long long *counter;
    unsigned long long n_grabs; // ceil(n / grab)
    // fused mode only: trace auxiliary ray aux_k of every ray instead of the ray itself (hf_reparam_trace): the
    // direction is replaced by hf_reparam_aux_kernel's, maxt by infinity
    uint32_t aux_on, aux_k, aux_seed;
    float aux_kappa;
    int aux_antithetic;
    const uint32_t *aux_ray_id;
    // ... samples aux_k .. aux_k + aux_n - 1 in ONE launch (hf_reparam_trace_all): sample j of ray i is written at
    // [j * aux_stride + i] of every output row; aux_cull > 0: sqrt(2) ||to_object|| tan(theta_max) of cone_maybe_alive
    uint32_t aux_n;
    size_t aux_stride;
    float aux_cull;
    const float4 *vn; // MODE 3: the handle's vertex normals (appended: the other modes' arguments keep their offsets)
};

// member-wise copy out of the kernarg segment (constant address space)
__device__ __forceinline__ hf_dev_field load_field(const __attribute__((address_space(4))) hf_dev_field *p) {
    hf_dev_field f;
    f.h = p->h; f.mip = p->mip; f.shear = p->shear;
    f.W = p->W; f.H = p->H; f.top = p->top;
    f.s = p->s; f.sx = p->sx; f.sy = p->sy; f.iu = p->iu; f.iv = p->iv; f.hx = p->hx; f.hy = p->hy; f.flip = p->flip;
#pragma unroll
    for (int k = 0; k < 12; ++k) { f.to_world[k] = p->to_world[k]; f.to_object[k] = p->to_object[k]; }
    return f;
}

typedef const __attribute__((address_space(4))) hf_trace_args *hf_kargs_ptr;
// (member-wise: an implicit copy cannot bind an object of the constant address space)
__device__ __forceinline__ hf_rays_t load_rays(hf_kargs_ptr ka) {
    hf_rays_t r;
#pragma unroll
    for (int k = 0; k < 3; ++k) { r.o[k] = ka->rays.o[k]; r.d[k] = ka->rays.d[k]; }
    r.maxt = ka->rays.maxt;
    return r;
}
__device__ __forceinline__ hf_pi_t load_pi(hf_kargs_ptr ka) {
    hf_pi_t p;
    p.t = ka->pi.t; p.prim_uv[0] = ka->pi.prim_uv[0]; p.prim_uv[1] = ka->pi.prim_uv[1]; p.prim_index = ka->pi.prim_index;
    return p;
}
__device__ __forceinline__ hf_si_t load_si(hf_kargs_ptr ka) {
    hf_si_t d;
    d.t = ka->sio.t; d.boundary_test = ka->sio.boundary_test;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d.p[k] = ka->sio.p[k]; d.n[k] = ka->sio.n[k]; d.sh_n[k] = ka->sio.sh_n[k]; d.dp_du[k] = ka->sio.dp_du[k];
        d.dp_dv[k] = ka->sio.dp_dv[k]; d.sh_s[k] = ka->sio.sh_s[k]; d.sh_t[k] = ka->sio.sh_t[k]; d.wi[k] = ka->sio.wi[k];
    }
    d.uv[0] = ka->sio.uv[0]; d.uv[1] = ka->sio.uv[1];
    return d;
}

// compute_si_to sink of the fused trace kernel and hf_si_kernel (KA: their kernarg pointer type): a field goes to memory
// when it is final; the row pointers are read from the kernarg segment at the store
template <typename KA>
struct hf_si_sink {
    KA ka;
    size_t ub;
    uint32_t lo, flags;
    __device__ __forceinline__ void s1(float *p, float v) { st(p, ub, lo, v); }
    __device__ __forceinline__ void s3(float *p0, float *p1, float *p2, v3 v) { st(p0, ub, lo, v.x); st(p1, ub, lo, v.y); st(p2, ub, lo, v.z); }
    __device__ __forceinline__ void t(float v) { s1(ka->sio.t, v); }
    __device__ __forceinline__ void p(v3 v) { s3(ka->sio.p[0], ka->sio.p[1], ka->sio.p[2], v); }
    __device__ __forceinline__ void boundary_test(float v) { if (flags & HF_RAY_BOUNDARYTEST) s1(ka->sio.boundary_test, v); }
    __device__ __forceinline__ void uv(float a, float b) { s1(ka->sio.uv[0], a); s1(ka->sio.uv[1], b); }
    __device__ __forceinline__ void dp_du(v3 v) { s3(ka->sio.dp_du[0], ka->sio.dp_du[1], ka->sio.dp_du[2], v); }
    __device__ __forceinline__ void dp_dv(v3 v) { s3(ka->sio.dp_dv[0], ka->sio.dp_dv[1], ka->sio.dp_dv[2], v); }
    __device__ __forceinline__ void n(v3 v) {
        s3(ka->sio.n[0], ka->sio.n[1], ka->sio.n[2], v);
        s3(ka->sio.sh_n[0], ka->sio.sh_n[1], ka->sio.sh_n[2], v);
    }
    __device__ __forceinline__ void n_face(v3 v) { s3(ka->sio.n[0], ka->sio.n[1], ka->sio.n[2], v); }
    __device__ __forceinline__ void sh_n(v3 v) { s3(ka->sio.sh_n[0], ka->sio.sh_n[1], ka->sio.sh_n[2], v); }
    __device__ __forceinline__ void sh_s(v3 v) { s3(ka->sio.sh_s[0], ka->sio.sh_s[1], ka->sio.sh_s[2], v); }
    __device__ __forceinline__ void sh_t(v3 v) { s3(ka->sio.sh_t[0], ka->sio.sh_t[1], ka->sio.sh_t[2], v); }
    __device__ __forceinline__ void wi(v3 v) { s3(ka->sio.wi[0], ka->sio.wi[1], ka->sio.wi[2], v); }
};

// Persistent waves: every wave pulls `grab` consecutive rays at a time from a global
// counter (zeroed on the stream before the launch), so expensive image regions are
// spread over all CUs whatever their position in the wavefront.
// MODE 3: the fused mode with smooth shading, its own instantiations (the flat ones do not read the vertex normals).
// AUX (fused mode only): auxiliary ray a.aux_k of every ray is traced instead of the ray itself (hf_reparam_trace) -- an
// instantiation of its own, so that the sampling code costs the ordinary fused launch nothing (inline it was +1.5 %).
// LEAN (round 4): the instantiations for launches the caller declares INCOHERENT -- the `coherent = false` of
// Scene::ray_intersect / ray_test / ray_intersect_preliminary (scene.h:117-146, 188-207, 237-259: "a hint that can improve
// performance in the first step of finding the PreliminaryInteraction"; reparam.py:95 traces its auxiliary rays with it).
// No wave tries the beam sweep, so the sweep, the item walk and their 29 KB of LDS are not in the kernel: 71 VGPRs (79 with
// the sampling code) instead of 95, no spilled register, and 6 (7) waves per SIMD instead of 5.  The results are the same
// (the per-lane walk is what a wave falls back to anyway); bounce rays 3.46 -> 3.18 ms, the reparameterisation backward
// 20.4 -> 19.0 ms; a launch of coherent rays is up to 25 % slower with it (profiles/r04_ab/r04_lean).
#ifndef HF_LEAN_WAVES
#define HF_LEAN_WAVES 6
#endif
#ifndef HF_LEAN_WAVES_AUX
#define HF_LEAN_WAVES_AUX 7
#endif
template <int MODE, bool AUX = false, bool LEAN = false>
__global__ __launch_bounds__(HF_BLOCK, (LEAN ? (AUX ? HF_LEAN_WAVES_AUX : HF_LEAN_WAVES) : MODE >= 2 ? HF_TRACE_WAVES_FUSED : HF_TRACE_WAVES))
void hf_trace_kernel(hf_trace_args a) {
    const hf_dev_field &f = a.f;
    const unsigned lane = threadIdx.x & 63u;
    __shared__ hf_beam_lds s_beam[HF_BLOCK / 64]; // per wave: the beam and box + record of the pass's nodes (walk_beam)
    __shared__ hf_items_lds s_items[HF_BLOCK / 64]; // per wave: work list and hit table of the item walk (walk_items)
    // Work distribution: the wavefront is cut into grabs of `grab` consecutive rays; XCD x owns grabs x, x + 8, ...
    // and hands them out through its own counter (a single counter serves ~80 fetches/us, which capped the rays
    // that only stream at half the memory bandwidth; eight addresses are served in parallel).  A wave pulls from the
    // counter of the XCD it runs on and moves on to the next XCD's when its own is exhausted, so all XCDs finish
    // together.  Grab numbers map to rays from the middle of the wavefront outwards (even: towards the end, odd:
    // towards the front): stream-only and traversal regions of a rendered wavefront then overlap in time.
    // (launch constants are read from the kernarg segment where they are needed -- see below -- so that the only
    // scalar state alive across a walk is the band, the current grab and the position in it)
    unsigned xc, tried = 0;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xc));
    xc &= HF_NUM_XCD - 1u;
    for (;;) {
        const __attribute__((address_space(4))) hf_trace_args *kg =
            (const __attribute__((address_space(4))) hf_trace_args *) __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kg));
        unsigned long long *counter = kg->counter;
        const unsigned grab = kg->grab;
        const unsigned long long n_grabs = kg->n_grabs;
        unsigned long long g = 0;
#ifdef HF_TSTATS
        const long long tw0 = clock64(); // (wide-path stamps: before the grab number is asked for)
#endif
        if (lane == 0) g = atomicAdd(counter + (size_t) xc * HF_COUNTER_STRIDE, 1ull);
        g = ((unsigned long long) (uint32_t) __builtin_amdgcn_readfirstlane((int) (g >> 32)) << 32) |
            (unsigned long long) (uint32_t) __builtin_amdgcn_readfirstlane((int) (g & 0xffffffffull));
#ifdef HF_TSTATS
        const long long tw1 = clock64(); // ... the grab number is there
#endif
        const unsigned long long gg = g * HF_NUM_XCD + xc;
        // FOUR FRONTS (round 4): grab numbers map to rays along four fronts -- from the middle of the wavefront towards its
        // end and towards its beginning, and from both ends inwards; an XCD takes its grabs from the fronts in turn.  A
        // rendered wavefront is expensive in the middle rows of the image (the terrain) and all-miss at its top and bottom:
        // with the two fronts from the middle that the kernel had until round 4, the waves traversed first and the launch
        // ended in a phase in which all of them streamed miss records.  With fronts from the ends as well, half of the
        // grabs in flight are cheap and half expensive for the whole launch: fused -4 %, closest hit -2.7 %, any hit
        // -2.9 %; uniform launches (bounce rays) +1.6 % (four regions of the terrain in the caches instead of two) -- so the
        // LEAN instantiations, whose launches are uniform by declaration, keep the two fronts from the middle.
#ifdef HF_TWO_FRONTS
        const bool two_fronts = true;
#else
        const bool two_fronts = LEAN && !AUX; // (the auxiliary rays of a rendered wavefront are as uneven as the wavefront itself)
#endif
        unsigned long long base;
        if (!two_fronts) {
            const unsigned long long quarter = (n_grabs + 3ull) >> 2; // grabs per front (the last ones of two fronts may not exist)
            if (gg >= 4ull * quarter) {
                if (++tried == HF_NUM_XCD) break;
                xc = (xc + 1u) & (HF_NUM_XCD - 1u);
                continue;
            }
            const unsigned long long k = gg >> 2;
            const unsigned front = (unsigned) ((gg + (gg >> 5)) & 3ull); // (a permutation of the four fronts within every four grab numbers)
            const unsigned long long pos = front == 0u ? 2ull * quarter + k : front == 1u ? 2ull * quarter - 1ull - k :
                                           front == 2u ? 4ull * quarter - 1ull - k : k;
            if (pos >= n_grabs) continue; // (4 x quarter rounds n_grabs up: up to three positions beyond the wavefront)
            base = pos * grab;
        } else {
            if (gg >= n_grabs) {
                if (++tried == HF_NUM_XCD) break;
                xc = (xc + 1u) & (HF_NUM_XCD - 1u);
                continue;
            }
            base = ((gg & 1ull) ? (n_grabs >> 1) - 1ull - (gg >> 1) : (n_grabs >> 1) + (gg >> 1)) * grab;
        }
        // the ray of the batch in flight: requested one batch ahead (see below)
        v3 o = mk3(0.f, 0.f, 0.f), d = o;
        float maxt = 0.f;
#pragma unroll 1
        for (unsigned sub = 0; sub < grab; sub += 64) {
            if (!AUX && (sub & 255u) == 0u) {
                // ---- WIDE PATH: 256 rays that miss the bound as a whole (70 % of the bench wavefront) ----
                // Four rays per lane through 16-byte loads, the conservative clip (maybe_alive: false only where setup_ray
                // says false), and if nobody may enter the bound the 256 miss records go out as 16-byte stores: 37 memory
                // instructions and ~360 others per 256 rays where four ordinary batches take ~1900 -- and a quarter of the
                // memory round trips, i.e. of the time the wave holds its slot.  A fetch with any "maybe" ray takes the
                // ordinary path below (its rays are re-read: L2 hits).
                const __attribute__((address_space(4))) hf_trace_args *kw =
                    (const __attribute__((address_space(4))) hf_trace_args *) __builtin_amdgcn_kernarg_segment_ptr();
                asm volatile("" : "+s"(kw));
                const size_t ubw = base + sub;
                if (kw->wide != 0u && sub + 256u <= grab && ubw + 256u <= kw->n) { // wave-uniform
#if HF_PRIO_OUT != 0
                    __builtin_amdgcn_s_setprio(0);
#endif
                    const uint32_t l4 = lane; // lane l: rays ubw + 4 l .. 4 l + 3
                    const hf_rays_t rp = load_rays(kw);
                    const f4 ox = ((const f4 *) (rp.o[0] + ubw))[l4], oy = ((const f4 *) (rp.o[1] + ubw))[l4], oz = ((const f4 *) (rp.o[2] + ubw))[l4];
                    const f4 dx = ((const f4 *) (rp.d[0] + ubw))[l4], dy = ((const f4 *) (rp.d[1] + ubw))[l4], dz = ((const f4 *) (rp.d[2] + ubw))[l4];
                    const f4 mt = ((const f4 *) (rp.maxt + ubw))[l4];
                    bool maybe = false;
                    {
                        const hf_dev_field f0 = load_field(&kw->f);
                        const float2 zr = f0.mip[1];
#pragma unroll
                        for (int j = 0; j < 4; ++j) maybe |= maybe_alive(f0, zr, mk3(ox[j], oy[j], oz[j]), mk3(dx[j], dy[j], dz[j]), mt[j]);
                    }
#ifdef HF_TSTATS
                    asm volatile("s_waitcnt vmcnt(0)");
                    const long long tw2 = clock64(); // ... the rays are there and tested
#endif
                    if (__ballot(maybe) == 0ull) {
                        // (opaque: constant register quadruples are otherwise hoisted out of the kernel's persistent loop,
                        // spilled, and re-loaded before every store)
                        float z0 = 0.f, i0 = __builtin_inff();
                        asm volatile("" : "+v"(z0), "+v"(i0));
                        const f4 zero = { z0, z0, z0, z0 };
                        if (MODE == 1) {
                            ((uint32_t *) (kw->hit_out + ubw))[l4] = 0u;
                        } else {
                            const f4 inf4 = { i0, i0, i0, i0 };
                            const hf_pi_t pi = load_pi(kw);
                            if (pi.t) st4(pi.t, ubw, l4, inf4);
                            if (pi.prim_uv[0]) st4(pi.prim_uv[0], ubw, l4, zero);
                            if (pi.prim_uv[1]) st4(pi.prim_uv[1], ubw, l4, zero);
                            if (pi.prim_index) st4((float *) pi.prim_index, ubw, l4, zero);
                            if (MODE >= 2) { // zero-initialised record (interaction.h:479-499, 667-673), wi = -d
                                const uint32_t flags = kw->flags;
                                const hf_si_t sd = load_si(kw);
                                st4(sd.t, ubw, l4, inf4);
#pragma unroll
                                for (int c = 0; c < 3; ++c) {
                                    st4(sd.p[c], ubw, l4, zero); st4(sd.n[c], ubw, l4, zero); st4(sd.sh_n[c], ubw, l4, zero);
                                    st4(sd.dp_du[c], ubw, l4, zero); st4(sd.dp_dv[c], ubw, l4, zero);
                                    st4(sd.sh_s[c], ubw, l4, zero); st4(sd.sh_t[c], ubw, l4, zero);
                                }
                                st4(sd.uv[0], ubw, l4, zero); st4(sd.uv[1], ubw, l4, zero);
                                if (flags & HF_RAY_BOUNDARYTEST) { const float b0 = z0 + 1e8f; const f4 big = { b0, b0, b0, b0 }; st4(sd.boundary_test, ubw, l4, big); }
                                st4(sd.wi[0], ubw, l4, -dx); st4(sd.wi[1], ubw, l4, -dy); st4(sd.wi[2], ubw, l4, -dz);
                            }
                        }
#ifdef HF_TSTATS
                        if (MODE != 1 && sub == 0u) { // lane 0's four prim_uv[0] entries: cycles waiting for the grab number, for the rays + test, issuing the stores
                            const long long tw3 = clock64();
                            const hf_pi_t pq = load_pi(kw);
                            if (lane == 0u && pq.prim_uv[0]) { (pq.prim_uv[0] + ubw)[0] = (float) (tw1 - tw0); (pq.prim_uv[0] + ubw)[1] = (float) (tw2 - tw1); (pq.prim_uv[0] + ubw)[2] = (float) (tw3 - tw2); (pq.prim_uv[0] + ubw)[3] = 1.f; }
                        }
#endif
                        sub += 192u; // (+ 64 by the loop: the next fetch of the grab)
                        continue;
                    }
                }
            }
            // all 64 lanes stay in the loop body (the shared walk relies on whole-wave ballots);
            // lanes past the end of the wavefront re-read the last ray and store nothing.
            // Pointers and constants that are only needed before or after the walk are read from the kernarg
            // segment where they are used: held in scalar registers across the walk they get spilled into
            // vector-register lanes, and fetching them back costs vector instructions.
            const __attribute__((address_space(4))) hf_trace_args *ka =
                (const __attribute__((address_space(4))) hf_trace_args *) __builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(ka)); // opaque: keeps these loads inside the loop body
            const size_t n = ka->n;
            // Addressing: every array is read / written at  (pointer + ub) + lo  with the wave-uniform element
            // offset ub and a 32-bit lane offset lo -- scalar base + vector offset, no 64-bit vector arithmetic.
            const size_t ub = base + sub;
            if (ub >= n) break; // wave-uniform
            const size_t left = n - ub; // >= 1
            const bool valid = lane < left;
            const uint32_t lo = valid ? lane : (uint32_t) (left - 1);
            if ((MODE >= 2 && AUX) || (sub & 255u) == 0u) { // first batch of a fetch: nothing was requested ahead (see the end of the body; AUX never requests ahead)
                const hf_rays_t rp = load_rays(ka);
                o = mk3((rp.o[0] + ub)[lo], (rp.o[1] + ub)[lo], (rp.o[2] + ub)[lo]);
                d = mk3((rp.d[0] + ub)[lo], (rp.d[1] + ub)[lo], (rp.d[2] + ub)[lo]);
                maxt = (rp.maxt + ub)[lo];
            }
            if (MODE >= 2 && AUX) {
                // ---- all samples of all 64 rays at once: when no auxiliary ray of the batch can enter the bound (60 % of
                // the bench wavefront), the aux_n miss records go out without a single sample being drawn ----
                const float ct = ka->aux_cull;
                if (ct > 0.f) { // wave-uniform
                    bool maybe;
                    {
                        const hf_dev_field f0 = load_field(&ka->f);
                        maybe = valid && cone_maybe_alive(f0, f0.mip[1], o, d, ct);
                    }
                    if (__ballot(maybe) == 0ull) {
                        {
                            const uint32_t aux_n = ka->aux_n;
#pragma unroll 1
                            for (uint32_t ak = 0; ak < aux_n; ++ak) { // wave-uniform loop, the stores predicated inside
                                asm volatile("" : "+s"(ka)); // opaque per sample: the ~30 pointer tests stay in the loop instead of being hoisted into (spilled) scalar pairs
                                if (valid) {
                                    const uint32_t flags = ka->flags;
                                    const size_t ubo = ub + (size_t) ak * ka->aux_stride;
                                    const hf_pi_t pi = load_pi(ka);
                                    if (pi.t) (pi.t + ubo)[lo] = __builtin_inff();
                                    if (pi.prim_uv[0]) (pi.prim_uv[0] + ubo)[lo] = 0.f;
                                    if (pi.prim_uv[1]) (pi.prim_uv[1] + ubo)[lo] = 0.f;
                                    if (pi.prim_index) (pi.prim_index + ubo)[lo] = 0u;
                                    hf_si_sink<hf_kargs_ptr> out = { ka, ubo, lo, flags };
                                    si_miss_to(out, flags); // (the launcher culls only when si.wi -- minus the sample's direction -- is not asked for)
                                }
                            }
                        }
                        continue;
                    }
                }
            }
#pragma unroll 1
            for (uint32_t ak = 0;; ++ak) { // (one trip unless AUX; the trip count is read from the kernarg segment at the end of the body)
            if (MODE >= 2 && AUX) {
                asm volatile("" : "+s"(ka)); // opaque per sample: kernarg loads stay inside the loop instead of being hoisted (and spilled)
                // the ray again (an L1 / L2 hit from the second sample on): nothing of it is held across the walk
                const hf_rays_t rp = load_rays(ka);
                o = mk3((rp.o[0] + ub)[lo], (rp.o[1] + ub)[lo], (rp.o[2] + ub)[lo]);
                const v3 dr = mk3((rp.d[0] + ub)[lo], (rp.d[1] + ub)[lo], (rp.d[2] + ub)[lo]);
                hf_reparam_args sa = {};
                sa.k = ka->aux_k + ak; sa.seed = ka->aux_seed; sa.kappa = ka->aux_kappa; sa.antithetic = ka->aux_antithetic;
                sa.ray_id = ka->aux_ray_id;
                hf_aux_sample q;
                aux_sample(sa, ub + lo, dr, q);
                d = frame_to_world(q, dr, q.omega);
                maxt = __builtin_inff();
            }
            hf_hit best;
            best.hit = false; best.t = __builtin_inff(); best.u = 0.f; best.v = 0.f; best.prim = 0u;
            const uint8_t *active = ka->active;
            const bool act = valid && (active ? ((active + ub)[lo] != 0) : true);
            TSTART();
            hf_ray_state rs = {}; // fully defined on every path: undefined fields become loop-carried registers
            bool alive;
            {
                const hf_dev_field f0 = load_field(&ka->f); // to_object etc.
                alive = act && setup_ray(f0, f0.mip[1], o, d, maxt, rs); // mip[1]: the global height range
            }
            const v3 dw = d; // world-space direction: wi of the record
            const uint64_t am = __ballot(alive);
            if (am != 0ull) {
                // coherent wave?  equal direction signs, entry points and directions close to the first live lane's
                const int src = __builtin_ctzll(am);
                // (v_readlane: the result is a scalar, so everything the shared walk derives from it stays scalar)
                const bool fx0 = __builtin_amdgcn_readlane((int) rs.fx, src) != 0, fy0 = __builtin_amdgcn_readlane((int) rs.fy, src) != 0;
                const float gx0 = __shfl(rs.gx, src), gy0 = __shfl(rs.gy, src);
                const float ux = rs.r.idy, uy = rs.r.idx; // direction ratio proxy: compare idx/idy cross products
                const float ux0 = __shfl(ux, src), uy0 = __shfl(uy, src);
                const bool near = (rs.fx == fx0) & (rs.fy == fy0) & (__builtin_fabsf(rs.gx - gx0) <= HF_COH_WINDOW) &
                                  (__builtin_fabsf(rs.gy - gy0) <= HF_COH_WINDOW) &
                                  (__builtin_fabsf(ux * uy0 - uy * ux0) <= HF_COH_DIR * __builtin_fabsf(ux * uy0));
                const bool coherent = !LEAN && __ballot(alive && !near) == 0ull; // (LEAN: every wave walks per lane)
                // incoherent wave: the shared walk degenerates to handing the root to every live lane
                TSTAMP(0); // ray set-up, clip and coherence test
                // Instruction-issue priority (round 4): a wave that traverses issues ahead of the waves of its SIMD that store
                // records or stream misses -- those wait for memory most of the time, the traversal is a chain of dependent
                // loads and ~100-instruction visits.  Closest hit -2.5 %, any hit -1.3 %, fused -1 %, bounce rays -1.5 %
                // (profiles/r04_ab/r04_prio; levels 1 / 2 / 3 and a middle level for the output phase measure the same).
                __builtin_amdgcn_s_setprio(HF_PRIO);
                // (one root-walk site for both the incoherent wave and a coherent wave whose beam sweep gives up)
                float thi = alive ? rs.thi : -1.f; // dead lanes overlap nothing
                bool root = alive;
                wstats_reset();
                if (coherent && f.top > HF_SUBTREE_LEVEL)
                    root = !walk_beam<MODE == 1>(f, rs, alive, fx0, fy0, best, thi, &s_beam[threadIdx.x >> 6], &s_items[threadIdx.x >> 6]) && alive && thi >= 0.f;
                if (root) {
                    hf_src_global src;
                    src.mip = f.mip; src.shear = f.shear; src.h = f.h; src.top = f.top; src.W = f.W;
                    const uint32_t lfxm = rs.fx ? ((1u << f.top) - 1u) : 0u, lfym = rs.fy ? ((1u << f.top) - 1u) : 0u;
                    (void) walk_subtree<MODE == 1>(f, src, rs, rs.r, rs.fx, rs.fy, lfxm, lfym, 0u, 0u, f.top, thi, best);
                }
#ifdef HF_WSTATS_ROOT // (diagnostic: the counters of batches that took the per-lane walk from the root as well)
                WSTATS_EXPORT(alive, best);
#else
                if (coherent && f.top > HF_SUBTREE_LEVEL) WSTATS_EXPORT(alive, best);
#endif
                TSTAMP(7); // fold of the item walks' hit table (and whatever the stamps above do not cover)
            }
#ifdef HF_TSTATS
            TSTATS_EXPORT(am != 0ull, valid, best);
#endif
            __builtin_amdgcn_s_setprio(HF_PRIO_OUT);
            asm volatile("" : "+s"(ka)); // the ~30 output pointers: loaded here, not before the walk
            // Request the next batch's rays BEFORE this batch's records are stored: vector-memory operations
            // complete in order, so a wave that loads after its stores waits for the store acknowledgements
            // (HBM write latency) on top of its own load latency -- that serial chain, not bandwidth, bounded
            // the rays that only stream.
            const bool more = (MODE >= 2 && AUX) && ak + 1u < ka->aux_n; // further samples of this batch (AUX re-reads its rays: no request ahead)
            const size_t ubo = (MODE >= 2 && AUX) ? ub + (size_t) ak * ka->aux_stride : ub; // where this sample's records go
            if (MODE >= 2 && AUX) {
                o = mk3(0.f, 0.f, 0.f); d = o; maxt = 0.f;
            } else if (((sub + 64u) & 255u) != 0u && sub + 64 < grab && ub + 64 < n) { // (the next fetch decides about its own rays)
                const size_t ub2 = ub + 64, left2 = n - ub2;
                const uint32_t lo2 = lane < left2 ? lane : (uint32_t) (left2 - 1);
                const hf_rays_t rp = load_rays(ka);
                o = mk3((rp.o[0] + ub2)[lo2], (rp.o[1] + ub2)[lo2], (rp.o[2] + ub2)[lo2]);
                d = mk3((rp.d[0] + ub2)[lo2], (rp.d[1] + ub2)[lo2], (rp.d[2] + ub2)[lo2]);
                maxt = (rp.maxt + ub2)[lo2];
            } else { // (defined on this path too, or the old values stay live across the walk)
                o = mk3(0.f, 0.f, 0.f); d = o; maxt = 0.f;
            }
            if (valid) { // (no per-lane exit from the sample loop: its control flow stays wave-uniform)
            if (MODE == 1) {
                uint8_t *hit_out = ka->hit_out;
                (hit_out + ub)[lo] = best.hit ? 1 : 0;
            } else {
                const hf_pi_t pi = load_pi(ka);
                if (pi.t) (pi.t + ubo)[lo] = best.hit ? best.t : __builtin_inff();
                if (pi.prim_uv[0]) (pi.prim_uv[0] + ubo)[lo] = best.hit ? best.u : 0.f;
                if (pi.prim_uv[1]) (pi.prim_uv[1] + ubo)[lo] = best.hit ? best.v : 0.f;
                if (pi.prim_index) (pi.prim_index + ubo)[lo] = best.hit ? best.prim : 0u;
                if (MODE >= 2) {
                    const uint32_t flags = ka->flags;
                    hf_si_sink<hf_kargs_ptr> out = { ka, ubo, lo, flags };
                    if (best.hit) {
                        // the origin is only needed by a hit: read again (an L2 hit) rather than held across the walk
                        const hf_rays_t rp = load_rays(ka);
                        const v3 ow = mk3((rp.o[0] + ub)[lo], (rp.o[1] + ub)[lo], (rp.o[2] + ub)[lo]);
                        const hf_dev_field fl = load_field(&ka->f); // to_world etc.: not held across the walk
                        // every field is stored as soon as it is final: the record is never whole in registers
                        if constexpr (MODE == 3) compute_si_to<true>(fl, ow, dw, best.t, best.u, best.v, best.prim, flags, out, ka->vn);
                        else                     compute_si_to(fl, ow, dw, best.t, best.u, best.v, best.prim, flags, out);
                    } else {
                        si_miss_to(out, flags);
                        out.wi(neg3(dw));
                    }
                }
            }
            } // valid
            if (!more) break;
            } // samples of the batch
        }
    }
}

#ifndef HF_FLAT_GRID_CAP
#define HF_FLAT_GRID_CAP (256 * 64)
#endif
static int grid_for(size_t n, size_t cap = HF_FLAT_GRID_CAP) {
    size_t blocks = (n + HF_BLOCK - 1) / HF_BLOCK;
    // grid-stride kernels: many short blocks balance better than one resident set
    if (blocks > cap) blocks = cap;
    // TEST HOOK (include/hf.h): HF_FORCE_GRID=<blocks >= 1> lowers the grid (never raises it: the transform slab, the scratch
    // ring and captured launches stay within what they reserve), so that launches of test size go round their loops
    if (const char *e = getenv("HF_FORCE_GRID")) {
        char *end = nullptr;
        const long v = strtol(e, &end, 10);
        if (end != e && *end == '\0' && v >= 1 && (size_t) v < blocks) blocks = (size_t) v;
    }
    if (blocks < 1) blocks = 1;
    return (int) blocks;
}
// hf_si_kernel streams 148 bytes per ray and keeps nothing per block: one block per 256 rays (no grid stride up to
// 67 M rays) instead of 16384 blocks: 1.44 -> 1.24 ms on the bench wavefront (profiles/r03_ab/r03_sicap).  The adjoint
// (an LDS tile to clear per wave) is best at the default cap (r03_cap).
#ifndef HF_SI_GRID_CAP
#define HF_SI_GRID_CAP (256 * 1024)
#endif

// Rays per fetch: HF_GRAB for big wavefronts (a single counter serves ~80 fetches/us, which caps the rate of rays
// that only stream), fewer for smaller ones so that every resident wave gets about HF_FETCHES_PER_WAVE fetches: the
// launch ends when its slowest wave does, and a fetch of 256 incoherent rays is 50 us of work.  Measured with 4 / 12 /
// 24 / 48 fetches per wave (profiles/r03_ab/r03_fpw): a 4.19 M-ray wavefront (configs[2]) 0.435 / 0.393 / 0.394 /
// 0.393 ms fused, the bench's 16.5 M bounce rays 3.25 / 3.26 / 3.17 / 3.16 ms; the 67.1 M-ray wavefront takes HF_GRAB
// either way.
#ifndef HF_GRAB01
#define HF_GRAB01 512 // cap of the closest-hit / any-hit launches, which store 16 / 1 bytes per ray: 67.1 M rays in fetches of
                      // 512 instead of 256: closest hit 2.13 -> 2.10 ms, any hit 1.94 -> 1.88 ms (profiles/r03_ab/r03_g01); the fused
                      // launch loses 1 % with 512
#endif
static uint32_t hf_grab_for(size_t n, int mode) {
    // TEST HOOK (include/hf.h): HF_FORCE_GRAB=<multiple of 64> fixes the fetch size, so that small launches reach the paths
    // that depend on it -- the wide path needs fetches of 256 rays, which the rule below gives to launches of > 27 M rays
    if (const char *e = getenv("HF_FORCE_GRAB")) {
        const long v = strtol(e, nullptr, 10);
        if (v >= 64 && v <= 4096 && v % 64 == 0) return (uint32_t) v;
    }
    const size_t resident = 256 * 4 * HF_TRACE_WAVES; // waves the launch keeps on the chip (about)
#ifndef HF_FETCHES_PER_WAVE
#define HF_FETCHES_PER_WAVE 24
#endif
    size_t g = (n / (resident * HF_FETCHES_PER_WAVE) + 32) / 64 * 64; // about that many fetches per wave (rounded to whole batches)
    if (g < 64) g = 64;
    const size_t cap = mode == 2 ? (size_t) HF_GRAB : (size_t) HF_GRAB01;
    if (g > cap) g = cap;
    return (uint32_t) g;
}

size_t hf_trace_scratch_bytes(size_t n) {
    (void) n;
    return HF_SCR_BYTES;
}

void hf_launch_trace(int mode, const hf_dev_field &f, size_t n, const hf_rays_t *rays, const uint8_t *active,
                     const hf_pi_t *pi, uint8_t *hit, const hf_si_t *si, uint32_t flags, void *scratch,
                     hipStream_t stream, const hf_reparam_args *aux, bool lean, const float4 *vn) {
    if (n == 0) return;
    (void) hipMemsetAsync(scratch, 0, HF_SCR_BYTES, stream);
    const hf_pi_t p = pi ? *pi : hf_pi_t{};
    const hf_si_t sd = si ? *si : hf_si_t{};
    const uint32_t grab = hf_grab_for(n, mode);
    size_t waves = (n + grab - 1) / grab, blocks = (waves + 3) / 4;
    const size_t per_cu = lean ? ((aux && mode == 2) ? HF_LEAN_WAVES_AUX : HF_LEAN_WAVES) : mode == 2 ? HF_TRACE_WAVES_FUSED : HF_TRACE_WAVES;
    if (blocks > 256 * per_cu) blocks = 256 * per_cu; // the resident set: that many workgroups per CU
    const dim3 grid((unsigned) blocks), block(HF_BLOCK);
    hf_trace_args a;
    a.f = f; a.n = n; a.rays = *rays; a.active = active; a.pi = p; a.hit_out = hit; a.sio = sd; a.flags = flags;
    a.counter = (unsigned long long *) scratch; a.grab = grab;
    {   // the wide path reads and writes 16 bytes per lane: every row it touches must be 16-byte aligned
        uintptr_t bits = 0;
        for (int k = 0; k < 3; ++k) bits |= (uintptr_t) rays->o[k] | (uintptr_t) rays->d[k];
        bits |= (uintptr_t) rays->maxt | (uintptr_t) p.t | (uintptr_t) p.prim_uv[0] | (uintptr_t) p.prim_uv[1] | (uintptr_t) p.prim_index;
        if (mode == 1) bits |= (uintptr_t) hit << 2; // (4 bytes per lane)
        static_assert(sizeof(hf_si_t) == 28 * sizeof(float *), "hf_si_t: nothing but its 28 float * rows");
        const float *const *rows = (const float *const *) &sd;
        for (size_t k = 0; k < sizeof(sd) / sizeof(float *); ++k) bits |= (uintptr_t) rows[k];
        a.wide = (active == nullptr && (bits & 15u) == 0u && grab % 256u == 0u) ? 1u : 0u;
#ifdef HF_NO_WIDE
        a.wide = 0u;
#endif
    }
    a.n_grabs = waves;
    a.aux_on = 0u; a.aux_k = 0u; a.aux_seed = 0u; a.aux_kappa = 1.f; a.aux_antithetic = 0; a.aux_ray_id = nullptr;
    a.aux_n = 1u; a.aux_stride = 0; a.aux_cull = 0.f;
    a.vn = vn;
    if (aux && mode == 2) {
        a.aux_on = 1u; a.aux_k = aux->k; a.aux_seed = aux->seed; a.aux_kappa = aux->kappa; a.aux_antithetic = aux->antithetic;
        a.aux_ray_id = aux->ray_id;
        if (aux->num > 1u) { a.aux_n = aux->num; a.aux_stride = aux->stride; }
        // cone_maybe_alive's constant: sqrt(2) ||to_object||_2 tan(theta_max), the norm bounded by sqrt(||.||_1 ||.||_inf);
        // cos(theta_max) = 1 - 13.83 / kappa (warp.h:557-566 with the sample clamped at 1e-6: log(1e-6) = -13.8155).
        // Not when si.wi -- minus the sample's direction -- is asked for: a culled batch draws no sample.
        const double cmin = 1.0 - 13.83 / (double) aux->kappa - 1e-6;
        if (cmin > 0.7 && !sd.wi[0] && !sd.wi[1] && !sd.wi[2]) {
            double n1 = 0.0, ninf = 0.0;
            for (int c = 0; c < 3; ++c) {
                double col = 0.0, row = 0.0;
                for (int rr = 0; rr < 3; ++rr) { col += fabs((double) f.to_object[4 * rr + c]); row += fabs((double) f.to_object[4 * c + rr]); }
                n1 = col > n1 ? col : n1; ninf = row > ninf ? row : ninf;
            }
            a.aux_cull = (float) (1.41422 * sqrt(n1 * ninf) * sqrt(1.0 - cmin * cmin) / cmin * 1.001);
        }
#ifdef HF_NO_AUX_CULL
        a.aux_cull = 0.f;
#endif
    }
    // [lean][mode + aux]: the auxiliary-ray sampling exists in the fused mode only; vn: the smooth-shading instantiations
    static void (*const kernel[2][4])(hf_trace_args) = {
        { hf_trace_kernel<0>, hf_trace_kernel<1>, hf_trace_kernel<2>, hf_trace_kernel<2, true> },
        { hf_trace_kernel<0, false, true>, hf_trace_kernel<1, false, true>, hf_trace_kernel<2, false, true>, hf_trace_kernel<2, true, true> },
    };
    static void (*const smooth[2][2])(hf_trace_args) = {
        { hf_trace_kernel<3>, hf_trace_kernel<3, true> }, { hf_trace_kernel<3, false, true>, hf_trace_kernel<3, true, true> },
    };
    if (vn && mode == 2) hipLaunchKernelGGL(smooth[lean][a.aux_on], grid, block, 0, stream, a);
    else                 hipLaunchKernelGGL(kernel[lean][mode + a.aux_on], grid, block, 0, stream, a);
}

// ---------------------------------------------------------------------------------
// surface interaction from (ray, pi)
// ---------------------------------------------------------------------------------
// The one kernel argument, read from the kernarg segment where it is used (as in the traversal kernel: ~45 pointers and
// the field by value held across the loop body were spilled into vector-register lanes: 134 SGPR spills).
struct hf_si_args {
    hf_dev_field f;
    size_t n;
    hf_rays_t rays;
    hf_pi_const_t pi;
    const uint8_t *active;
    hf_si_t sio;
    uint32_t flags;
    const float4 *vn; // hf_si_smooth_kernel: the handle's vertex normals
};
typedef const __attribute__((address_space(4))) hf_si_args *hf_si_kargs;

// the body of hf_si_kernel (flat shading) and hf_si_smooth_kernel
template <bool SMOOTH>
__device__ __forceinline__ void si_body() {
    const uint32_t lane = threadIdx.x & 63u;
    const size_t stride = (size_t) gridDim.x * HF_BLOCK;
    for (size_t ub = (size_t) blockIdx.x * HF_BLOCK + (threadIdx.x & ~63u);; ub += stride) {
        hf_si_kargs ka = (hf_si_kargs) __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka)); // opaque: keeps the loads that follow where they are written
        const size_t n = ka->n;
        if (ub >= n) break; // wave-uniform
        if (lane >= n - ub) continue;
        const uint32_t lo = lane;
        const v3 o = mk3((ka->rays.o[0] + ub)[lo], (ka->rays.o[1] + ub)[lo], (ka->rays.o[2] + ub)[lo]);
        const v3 d = mk3((ka->rays.d[0] + ub)[lo], (ka->rays.d[1] + ub)[lo], (ka->rays.d[2] + ub)[lo]);
        const float t = (ka->pi.t + ub)[lo];
        const uint8_t *active = ka->active;
        const bool act = (active ? ((active + ub)[lo] != 0) : true) && (t != __builtin_inff());
        const uint32_t flags = ka->flags;
        hf_si_sink<hf_si_kargs> out = { ka, ub, lo, flags };
        if (act) {
            const float b1 = (ka->pi.prim_uv[0] + ub)[lo], b2 = (ka->pi.prim_uv[1] + ub)[lo];
            const uint32_t prim = (ka->pi.prim_index + ub)[lo];
            const hf_dev_field f = load_field(&ka->f);
            compute_si_to<SMOOTH>(f, o, d, t, b1, b2, prim, flags, out, SMOOTH ? ka->vn : nullptr);
        } else {
            si_miss_to(out, flags);
            out.wi(neg3(d));
        }
    }
}
__global__ __launch_bounds__(HF_BLOCK) void hf_si_kernel(hf_si_args a_) { (void) a_; si_body<false>(); }
__global__ __launch_bounds__(HF_BLOCK) void hf_si_smooth_kernel(hf_si_args a_) { (void) a_; si_body<true>(); }

void hf_launch_si(const hf_dev_field &f, size_t n, const hf_rays_t *rays, const hf_pi_const_t *pi,
                  const uint8_t *active, const hf_si_t *si, uint32_t flags, hipStream_t stream, const float4 *vn) {
    if (n == 0) return;
    hf_si_args a;
    a.f = f; a.n = n; a.rays = *rays; a.pi = *pi; a.active = active; a.sio = *si; a.flags = flags; a.vn = vn;
    hipLaunchKernelGGL(vn ? hf_si_smooth_kernel : hf_si_kernel, dim3(grid_for(n, HF_SI_GRID_CAP)), dim3(HF_BLOCK), 0, stream, a);
}

// ---------------------------------------------------------------------------------
// adjoint: reverse mode of compute_si, atomic scatter of dL/dheight.  The reverse sweep over compute_si_to's hit-geometry
// quantities (hf_device.h: prim_world, bary_point, uv_diff, unit_normal, follow_t, mt_terms)
// ---------------------------------------------------------------------------------
#define HF_ADJ_TILE 32 // texels per side of the per-wave LDS accumulation tile

// bitwise OR over the 64 lanes of a wave (DPP within rows of 16, readlane across the four rows)
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
    int x = (int) v;
    x |= __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true);  // quad_perm [1,0,3,2]
    x |= __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true);  // quad_perm [2,3,0,1]
    x |= __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true); // row_half_mirror
    x |= __builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, true); // row_mirror
    return (uint32_t) (__builtin_amdgcn_readlane(x, 0) | __builtin_amdgcn_readlane(x, 16) |
                       __builtin_amdgcn_readlane(x, 32) | __builtin_amdgcn_readlane(x, 48));
}

__device__ __forceinline__ uint64_t wave_or(uint64_t v) {
    return (uint64_t) wave_or((uint32_t) v) | ((uint64_t) wave_or((uint32_t) (v >> 32)) << 32);
}

// Per-wave LDS scatter tile of dL/dheight (hf_adjoint_kernel, hf_reparam_backward_kernel): TILE x TILE texels whose
// origin (ar, ac) is wave-uniform.  A lane adds its triangle's three contributions into the tile (ds_add_f32) or, outside
// it, straight to global memory, and records the tile rows it touched in a TILE-bit mask; the flush then adds the
// touched rows to global memory, 64 consecutive tile entries (64 / TILE rows) per wave-instruction.  The kernels zero
// their tile themselves (one loop): inlined from a helper, that loop reordered hf_adjoint_kernel's entry block
template <int TILE> using hf_tile_rows = std::conditional_t<(TILE > 32), uint64_t, uint32_t>;
// origin `off` texels before the first vertex of the first lane of `m` (a ballot), rows and columns
__device__ __forceinline__ void tile_anchor(uint64_t m, const int (&vr)[3], const int (&vc)[3], int off, int &ar, int &ac) {
    const int src = __builtin_ctzll(m);
    ar = __shfl(vr[0], src) - off; ac = __shfl(vc[0], src) - off;
}
// one vertex's contribution g at texel (r, c).  (Per vertex, with the loop over the three at the call site: the
// lane's vr / vc / gh arrays passed by reference are promoted to registers later and that reorders the adjoint's code)
// STRIDE: floats per texel of the global buffer (one channel of an interleaved attribute: grad_h = its base + channel)
template <int TILE, int STRIDE = 1>
__device__ __forceinline__ void tile_add(float *acc, int ar, int ac, int r, int c, float g, float *grad_h, int W,
                                         hf_tile_rows<TILE> &rows) {
    const int rr = r - ar, cc = c - ac;
    if ((unsigned) rr < (unsigned) TILE && (unsigned) cc < (unsigned) TILE) {
        atomicAdd(acc + rr * TILE + cc, g);
        rows |= (hf_tile_rows<TILE>) 1 << rr;
    } else {
        if constexpr (STRIDE == 1) atomicAdd(grad_h + (size_t) r * W + c, g);
        else atomicAdd(grad_h + ((size_t) r * W + c) * STRIDE, g);
    }
}
// (rows: this lane's mask; ORed over the wave here)
template <int TILE, int STRIDE = 1>
__device__ __forceinline__ void tile_flush(float *acc, int ar, int ac, hf_tile_rows<TILE> rows, float *grad_h, int W, int lane) {
    constexpr int R = 64 / TILE; // tile rows per wave-instruction
    rows = wave_or(rows);
#pragma unroll 1
    while (rows != 0u) { // wave-uniform
        const int k2 = stk_ctz(rows) / R;
        rows &= R == 1 ? rows - 1u : ~((((hf_tile_rows<TILE>) 1 << R) - 1u) << (R * k2));
        const int k = k2 * 64 + lane;
        const float v = acc[k];
        if (v != 0.f) {
            const int rr = ar + k / TILE, cc = ac + k % TILE;
            if constexpr (STRIDE == 1) atomicAdd(grad_h + (size_t) rr * W + cc, v);
            else atomicAdd(grad_h + ((size_t) rr * W + cc) * STRIDE, v);
            acc[k] = 0.f;
        }
    }
}

// harmonic weight of one auxiliary sample and its gradient w.r.t. the sampled direction (reparam.py:103-121)
__device__ __forceinline__ void reparam_weight(const hf_reparam_args &a, const hf_aux_sample &q, v3 d, float B,
                                               float &w, v3 &dw) {
    const float inv_vmf = 1.0f / __builtin_fmaf(q.sy, expf(-2.f * a.kappa), 1.f - q.sy);
    const float w_denom = inv_vmf - 1.f + B;
    const float w_rcp = (w_denom > 1e-4f) ? 1.0f / w_denom : 0.f;
    // (the exponent of the reference's callers is 3: three multiplications instead of exp2(y log2 x))
    w = (a.exponent == 3.f ? (w_rcp * w_rcp) * w_rcp : powf(w_rcp, a.exponent)) * inv_vmf;
    const float tmp1 = fminf(fmaxf(inv_vmf * w * w_rcp * a.kappa * a.exponent, -1e10f), 1e10f);
    const v3 tmp2 = frame_to_world(q, d, mk3(q.omega.x, q.omega.y, 0.f));
    dw = mk3(tmp1 * tmp2.x, tmp1 * tmp2.y, tmp1 * tmp2.z);
}
// Adjoint of V_direct.  The upstream gradient of direction = normalize(d + V/Z), divergence = (div - <V/Z, dZ>) / Z
// at V = 0 (reparam.py:262-281) reaches V = sum_i w_i V_direct_i and div = sum_i <d_w_omega_i, V_direct_i> of the samples
// of a ray.  vdirect_grad_ray: the part common to the samples, from (d, g_dir, g_div) and the sums Z, dZ.  dZ_of()
// yields dZ; it is called where hf_reparam_weight_kernel has always loaded dZ (loaded earlier, that kernel's code moves)
struct hf_vd_grad {
    v3 gV;       // dL/dV
    float gdivV; // dL/ddiv
};
template <typename DZ>
__device__ __forceinline__ hf_vd_grad vdirect_grad_ray(v3 d, v3 gd, float gdiv, float Zs, DZ dZ_of) {
    const float Z = fmaxf(Zs, 1e-8f), iZ = 1.0f / Z;
    const float dd = dot3(d, d), idn = 1.0f / __builtin_sqrtf(dd);
    const float pr = dot3(d, gd) / dd;
    const v3 dZ = dZ_of();
    const float c = gdiv * iZ * iZ;
    return hf_vd_grad{ mk3((gd.x - d.x * pr) * idn * iZ - c * dZ.x, (gd.y - d.y * pr) * idn * iZ - c * dZ.y,
                           (gd.z - d.z * pr) * idn * iZ - c * dZ.z),
                       gdiv * iZ };
}
// gradient w.r.t. one sample's V_direct (V_i = w V_direct, div_i = <d_w_omega, V_direct>)
__device__ __forceinline__ v3 vdirect_grad_sample(const hf_vd_grad &g, float w, v3 dw) {
    return mk3(__builtin_fmaf(w, g.gV.x, g.gdivV * dw.x), __builtin_fmaf(w, g.gV.y, g.gdivV * dw.y),
               __builtin_fmaf(w, g.gV.z, g.gdivV * dw.z));
}
// a hit's V_direct = (p - o) / t: gradients w.r.t. p and t from gVd, po = p - o
struct hf_vd_hit {
    v3 gp;
    float gt;
};
__device__ __forceinline__ hf_vd_hit vdirect_grad_hit(v3 gVd, v3 po, float t) {
    const float it = 1.0f / t;
    return hf_vd_hit{ mk3(gVd.x * it, gVd.y * it, gVd.z * it), -dot3(gVd, po) * it * it };
}

// ---- dL/d(to_world): the slab reducer (hf_adjoint_transform, hf_sample_position_adjoint_transform).  Every lane keeps
// its 12 partial sums in registers across its grid-stride loop.  At the end a block sums them (a butterfly over the
// wave's 64 lanes, then the block's four waves through LDS, in a fixed order) and stores its 12 sums to its row of a
// slab; hf_xform_sum_kernel then adds the slab's rows, in a fixed order, into the caller's 12 floats.  No float
// atomics: 16 k blocks x 12 same-address atomics would serialise, and the slab keeps the result bitwise repeatable.
// The grid of these launches is capped lower than HF_FLAT_GRID_CAP so that the slab (HF_XFORM_GRID_CAP x 48 bytes) fits
// every scratch block of the handle's ring, the ones reserved for captured launches included (hf_capi.cpp).  Measured
// on the bench wavefront (hf_adjoint_transform with the heights, median of 20): 2048 blocks 0.784 ms, 5120 0.722 ms,
// 16384 0.962 ms (profiles/transform_grad/). ----
#ifndef HF_XFORM_GRID_CAP
#define HF_XFORM_GRID_CAP 5120
#endif
size_t hf_xform_slab_bytes(size_t n) {
    return (size_t) (n ? grid_for(n, HF_XFORM_GRID_CAP) : HF_XFORM_GRID_CAP) * 12u * sizeof(float);
}
// introspection (include/hf.h): the grid a grid-stride launch of n items gets, HF_FORCE_GRID included
extern "C" int hf_grid_blocks(size_t n, int family) {
    switch (family) {
    case 0: return grid_for(n, HF_FLAT_GRID_CAP);
    case 1: return grid_for(n, HF_SI_GRID_CAP);
    case 2: return grid_for(n, HF_XFORM_GRID_CAP);
    default: return 0;
    }
}
// sum over the 64 lanes, the same in every lane (xor butterfly: each step adds two values that commute exactly)
__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
// the block's sums of M into slab row blockIdx.x; every thread of the block calls it
__device__ __forceinline__ void xform_block_store(const float M[12], float *slab) {
    __shared__ float s_red[HF_BLOCK / 64][12];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        const float v = wave_sum_f32(M[j]);
        if (lane == 0u) s_red[w][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < 12u) {
        float v = s_red[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < HF_BLOCK / 64; ++k) v += s_red[k][threadIdx.x];
        slab[(size_t) blockIdx.x * 12u + threadIdx.x] = v;
    }
}
// out[j] += sum over the slab's rows of column j: every thread sums every HF_BLOCK-th row in fp64 (a row is three
// 16-byte loads; consecutive threads read consecutive rows), then a fixed-order tree over the block through LDS.  (A
// first form, 16 threads per column striding over the rows one float at a time, took 117 us for 5120 rows.)
__global__ __launch_bounds__(HF_BLOCK) void hf_xform_sum_kernel(const float *__restrict__ slab, uint32_t rows,
                                                                 float *__restrict__ out) {
    __shared__ double s_part[HF_BLOCK][13]; // (13: the rows of 12 spread over the banks)
    const uint32_t t = threadIdx.x;
    double acc[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) acc[j] = 0.0;
    for (uint32_t b = t; b < rows; b += HF_BLOCK) {
        const float4 *r = reinterpret_cast<const float4 *>(slab + (size_t) b * 12u); // 48-byte rows of a 256-byte-aligned block
        const float4 v[3] = { r[0], r[1], r[2] };
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc[4 * k + 0] += (double) v[k].x; acc[4 * k + 1] += (double) v[k].y;
            acc[4 * k + 2] += (double) v[k].z; acc[4 * k + 3] += (double) v[k].w;
        }
    }
#pragma unroll
    for (int j = 0; j < 12; ++j) s_part[t][j] = acc[j];
    __syncthreads();
#pragma unroll
    for (uint32_t h = HF_BLOCK / 2; h > 0; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int j = 0; j < 12; ++j) s_part[t][j] += s_part[t + h][j];
        }
        __syncthreads();
    }
    if (t < 12u) out[t] += (float) s_part[0][t];
}
static void xform_sum(const float *slab, int rows, float *out, hipStream_t stream) {
    hipLaunchKernelGGL(hf_xform_sum_kernel, dim3(1), dim3(HF_BLOCK), 0, stream, slab, (uint32_t) rows, out);
}

// The one kernel argument.  ~45 pointers and the field by value do not fit the scalar register file: held across the
// loop body they were spilled into vector-register lanes (108 SGPR spills, 342 v_readlane / v_writelane).  As in the
// traversal kernel, everything is read from the kernarg segment where it is used (scalar loads that hit the constant
// cache), and every array is addressed as (pointer + wave-uniform element offset)[lane].
struct hf_adjoint_args {
    hf_dev_field f;
    size_t n;
    hf_rays_t rays;
    hf_pi_const_t pi;
    const uint8_t *active;
    hf_si_grad_t g;
    uint32_t flags;
    float *grad_h;
    float *go[3], *gd[3];
    uint32_t *row_band; // optional: {lowest texture row that received a contribution, highest + 1}, atomicMin / atomicMax
    const float4 *vn;   // hf_adjoint_smooth_kernel: the handle's vertex normals
};
typedef const __attribute__((address_space(4))) hf_adjoint_args *hf_adj_kargs;
// hf_eval_parameterization_adjoint (adjoint_body<..., PARAM>): the query uv rows follow the common arguments, whose
// rays and pi are not read
struct hf_param_adjoint_args {
    hf_adjoint_args a;
    const float *uv[2];
};
__device__ __forceinline__ hf_adj_kargs adj_kargs() {
    hf_adj_kargs ka = (hf_adj_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka)); // opaque: keeps the loads that follow where they are written
    return ka;
}
// (row + ub)[lo], 0 for an absent row: scalar base + 32-bit lane offset
__device__ __forceinline__ float ldu(const float *p, size_t ub, uint32_t lo) { return p ? (p + ub)[lo] : 0.f; }

// RAYGRAD: dL/do and dL/dd are wanted (hf_adjoint's grad_o / grad_d); without them their accumulation is dead code.
// SMOOTH (hf_adjoint_smooth_kernel): sh_n is the interpolated vertex normal.  Its gradient reaches the heights through
// the barycentrics (the Moeller-Trumbore reverse below) and through the three vertex normals: the VJP of vertex_normal
// is evaluated per hit, on the fly, and its 7 contributions per vertex (the vertex and its 1-ring: up to 12 texels per
// hit) go through the same LDS tile as the positions' three.  acc: the wave's tile (TILE x TILE floats of LDS).
// XFORM (hf_adjoint_xform_kernel, hf_adjoint_xform_smooth_kernel): also dL/d(to_world) = sum over the hit's vertices of
// dL/dP_k (q_k, 1)^T, in M across the loop, plus (smooth) the 1-rings of the three vertex normals; the block's sums
// go to its row of `slab` (xform_block_store).
// PARAM (hf_param_adjoint*_kernel, hf_eval_parameterization_adjoint): the kernel argument is an hf_param_adjoint_args; a
// lane's (prim, b) is param_lookup of its query uv instead of pi, and a lane outside the texture square does nothing.
// The flags carry HF_RAY_FOLLOWSHAPE (frozen barycentrics, never the re-intersection) and t has no gradient, so the
// FollowShape term of t is not evaluated (its ray is the UV-space one); ray gradients are not offered.
template <bool RAYGRAD, bool SMOOTH, bool XFORM = false, bool PARAM = false>
__device__ __forceinline__ void adjoint_body(float *acc, float *slab = nullptr) {
    // Wave-level pre-reduction of the scatter: the hits of one wave (one pixel's samples for
    // primary rays) fall on a few dozen vertices, so their three contributions each are first
    // summed into a 32x32-texel LDS tile anchored near the wave's first hit (ds_add_f32) and the
    // tile is then flushed row by row -- contiguous segments, one global atomic per touched texel
    // instead of three per ray.  Contributions outside the tile go straight to global memory.
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t k = lane; k < HF_ADJ_TILE * HF_ADJ_TILE; k += 64) acc[k] = 0.f;
    uint32_t row_lo = 0xFFFFFFFFu, row_hi = 0u; // rows this lane scattered to (hf_adjoint_rows)
    float M[12]; // XFORM: this lane's dL/d(to_world)
#pragma unroll
    for (int j = 0; j < 12; ++j) M[j] = 0.f;
    const size_t stride = (size_t) gridDim.x * HF_BLOCK;
    for (size_t ub = (size_t) blockIdx.x * HF_BLOCK + (threadIdx.x & ~63u);; ub += stride) { // whole waves stay in the loop (ballots below)
        hf_adj_kargs ka = adj_kargs();
        const size_t n = ka->n;
        if (ub >= n) break; // wave-uniform
        const size_t left = n - ub;
        const bool valid = lane < left;
        const uint32_t lo = valid ? lane : (uint32_t) (left - 1);
        uint32_t qprim = 0u; // PARAM: the lane's triangle and barycentrics
        float qb1 = 0.f, qb2 = 0.f;
        bool act;
        if constexpr (PARAM) {
            const auto *kp = (const __attribute__((address_space(4))) hf_param_adjoint_args *) ka;
            const float u = (kp->uv[0] + ub)[lo], v = (kp->uv[1] + ub)[lo];
            const uint8_t *active = ka->active;
            act = valid && (active ? ((active + ub)[lo] != 0) : true) && param_lookup(ka->f.W, ka->f.H, u, v, qprim, qb1, qb2);
        } else {
            const float t_in = (ka->pi.t + ub)[lo];
            const uint8_t *active = ka->active;
            act = valid && (active ? ((active + ub)[lo] != 0) : true) && (t_in != __builtin_inff());
        }
        const uint32_t flags = ka->flags;
        const bool follow = (flags & HF_RAY_FOLLOWSHAPE) != 0, detach = (flags & HF_RAY_DETACHSHAPE) != 0;
        const bool tex = (flags & (HF_RAY_UV | HF_RAY_DPDUV)) != 0;
        v3 go = mk3(0.f, 0.f, 0.f), gd = mk3(0.f, 0.f, 0.f);
        float gh[3] = { 0.f, 0.f, 0.f };
        int vr[3] = { 0, 0, 0 }, vc[3] = { 0, 0, 0 };
        bool scatter = false;
        v3 gnv[3]; // SMOOTH: dL/d(vertex normal k)
        bool smv = false; // ... to be scattered through vertex_normal_vjp
        if (act) {
            // ONE batch of requests for everything a hit needs that does not depend on other loads -- the ray, the
            // rest of pi, the 18 upstream rows -- then the three heights behind prim_index: three dependent round
            // trips per iteration (pi.t, this batch, the heights) where the loads used to trail the arithmetic (six).
            v3 o = mk3(0.f, 0.f, 0.f), d = o;
            float b1 = qb1, b2 = qb2;
            uint32_t prim = qprim;
            if constexpr (!PARAM) {
                o = mk3((ka->rays.o[0] + ub)[lo], (ka->rays.o[1] + ub)[lo], (ka->rays.o[2] + ub)[lo]);
                d = mk3((ka->rays.d[0] + ub)[lo], (ka->rays.d[1] + ub)[lo], (ka->rays.d[2] + ub)[lo]);
                b1 = (ka->pi.prim_uv[0] + ub)[lo]; b2 = (ka->pi.prim_uv[1] + ub)[lo];
                prim = (ka->pi.prim_index + ub)[lo];
            }
            const float b0 = 1.f - b1 - b2;
            const float gt = ldu(ka->g.t, ub, lo);
            v3 gp = mk3(ldu(ka->g.p[0], ub, lo), ldu(ka->g.p[1], ub, lo), ldu(ka->g.p[2], ub, lo));
            const v3 gn_a = mk3(ldu(ka->g.n[0], ub, lo), ldu(ka->g.n[1], ub, lo), ldu(ka->g.n[2], ub, lo));
            const v3 gn_b = mk3(ldu(ka->g.sh_n[0], ub, lo), ldu(ka->g.sh_n[1], ub, lo), ldu(ka->g.sh_n[2], ub, lo));
            const float guv0 = ldu(ka->g.uv[0], ub, lo), guv1 = ldu(ka->g.uv[1], ub, lo);
            v3 gu_ = mk3(0.f, 0.f, 0.f), gv_ = gu_;
            if (flags & HF_RAY_DPDUV) {
                gu_ = mk3(ldu(ka->g.dp_du[0], ub, lo), ldu(ka->g.dp_du[1], ub, lo), ldu(ka->g.dp_du[2], ub, lo));
                gv_ = mk3(ldu(ka->g.dp_dv[0], ub, lo), ldu(ka->g.dp_dv[1], ub, lo), ldu(ka->g.dp_dv[2], ub, lo));
            }
            const hf_dev_field f = load_field(&ka->f);
            v3 P[3];
            float U[3], V[3];
            int vi[3], vj[3];
            prim_world(f, prim, P, U, V, vi, vj);
            const bool sm = SMOOTH && smooth_sh(flags);
            v3 NV[3];
            if (sm) load_vn(f, ka->vn, vi, vj, NV);
            const v3 dp0 = P[1] - P[0], dp1 = P[2] - P[0];
            const v3 p = bary_point(P, b0, b1, b2);
            const v3 z3 = mk3(0.f, 0.f, 0.f);
            v3 gP0 = z3, gP1 = z3, gP2 = z3, gdp0 = z3, gdp1 = z3;

            // dp_du / dp_dv from the (constant) texcoord differences
            if (flags & HF_RAY_DPDUV) {
                const auto [du0, dv0, du1, dv1, det, inv_det] = uv_diff(U, V);
                if (det != 0.f) {
                    axpy3(dv1 * inv_det, gu_, gdp0);
                    axpy3(-dv0 * inv_det, gu_, gdp1);
                    axpy3(-du1 * inv_det, gv_, gdp0);
                    axpy3(du0 * inv_det, gv_, gdp1);
                }
            }
            // n = sh_n = +-normalize(cross(dp0, dp1))  (smooth: n only)
            {
                const auto [nn, r] = unit_normal(dp0, dp1);
                const float sgn = f.flip ? -1.f : 1.f;
                const v3 gnf = sm ? gn_a : mk3(gn_a.x + gn_b.x, gn_a.y + gn_b.y, gn_a.z + gn_b.z);
                const v3 gn = mk3(sgn * gnf.x, sgn * gnf.y, sgn * gnf.z);
                const v3 gN = dnormalize(nn, r, gn);
                axpy3(1.f, cross3(dp1, gN), gdp0);
                axpy3(1.f, cross3(gN, dp0), gdp1);
            }
            // FollowShape: t = sqrt(|p-o|^2/|d|^2) feeds p, o, d
            if (!PARAM && follow) {
                const auto [po, dd, tt] = follow_t(p, o, d);
                const float c = gt / (tt * dd);
                axpy3(c, po, gp);
                axpy3(-c, po, go);
                axpy3(-gt * tt / dd, d, gd);
            }
            // p = sum b_k P_k, uv = sum b_k uv_k
            float gb0 = dot3(gp, P[0]), gb1 = dot3(gp, P[1]), gb2 = dot3(gp, P[2]);
            if (sm) { // sh_n = +-normalize(sum b_k N_k): to the barycentrics and to the vertex normals
                const v3 ns = bary_normal(NV, b0, b1, b2);
                const float r = rsqrt_ieee(dot3(ns, ns));
                const v3 gns = dnormalize(ns * r, r, f.flip ? neg3(gn_b) : gn_b);
                gb0 += dot3(gns, NV[0]); gb1 += dot3(gns, NV[1]); gb2 += dot3(gns, NV[2]);
                gnv[0] = gns * b0; gnv[1] = gns * b1; gnv[2] = gns * b2;
            }
            if (tex) {
                gb0 += guv0 * U[0] + guv1 * V[0];
                gb1 += guv0 * U[1] + guv1 * V[1];
                gb2 += guv0 * U[2] + guv1 * V[2];
            }
            axpy3(b0, gp, gP0); axpy3(b1, gp, gP1); axpy3(b2, gp, gP2);
            float gu = gb1 - gb0, gv = gb2 - gb0;
            if (!tex) { gu += guv0; gv += guv1; }

            if (!follow) { // reverse of the differentiable Moeller-Trumbore (t_d, prim_uv_d)
                const v3 e1 = dp0, e2 = dp1;
                const auto [pvec, tvec, qvec, inv, a_u, a_v, a_t] = mt_terms(o, d, P[0], e1, e2);
                const float g_au = gu * inv, g_av = gv * inv, g_at = gt * inv;
                const float g_inv = gu * a_u + gv * a_v + gt * a_t;
                const float g_det = -g_inv * inv * inv;
                v3 ge1 = z3, ge2 = z3, gq = z3, gtv = z3, gpv = z3;
                axpy3(g_at, qvec, ge2); axpy3(g_at, e2, gq);
                axpy3(g_av, qvec, gd);  axpy3(g_av, d, gq);
                axpy3(1.f, cross3(e1, gq), gtv);
                axpy3(1.f, cross3(gq, tvec), ge1);
                axpy3(g_au, pvec, gtv); axpy3(g_au, tvec, gpv);
                axpy3(g_det, pvec, ge1); axpy3(g_det, e1, gpv);
                axpy3(1.f, cross3(e2, gpv), gd);
                axpy3(1.f, cross3(gpv, d), ge2);
                axpy3(1.f, gtv, go); axpy3(-1.f, gtv, gP0);
                axpy3(1.f, ge1, gP1); axpy3(-1.f, ge1, gP0);
                axpy3(1.f, ge2, gP2); axpy3(-1.f, ge2, gP0);
            }
            // without dPdUV, dp_du / dp_dv = coordinate_system of the normal before flip_normals (mesh.cpp:762): their
            // gradient joins the edges through n here, after the re-intersection's reverse, where fewer values are live
            if (!(flags & HF_RAY_DPDUV)) {
                const auto [nn, r] = unit_normal(dp0, dp1);
                const v3 gN = dnormalize(nn, r, coordinate_system_vjp(nn,
                    mk3(ldu(ka->g.dp_du[0], ub, lo), ldu(ka->g.dp_du[1], ub, lo), ldu(ka->g.dp_du[2], ub, lo)),
                    mk3(ldu(ka->g.dp_dv[0], ub, lo), ldu(ka->g.dp_dv[1], ub, lo), ldu(ka->g.dp_dv[2], ub, lo))));
                axpy3(1.f, cross3(dp1, gN), gdp0);
                axpy3(1.f, cross3(gN, dp0), gdp1);
            }
            axpy3(1.f, gdp0, gP1); axpy3(-1.f, gdp0, gP0);
            axpy3(1.f, gdp1, gP2); axpy3(-1.f, gdp1, gP0);

            if constexpr (XFORM) {
                if (!detach) { // P_k = [A | t] (q_k, 1)
                    v3 q[3];
                    prim_local(f, vi, vj, q);
                    xform_grad_point(M, gP0, q[0]); xform_grad_point(M, gP1, q[1]); xform_grad_point(M, gP2, q[2]);
                    if (SMOOTH && sm) vertex_normals_vjp_xform(f, vi, vj, gnv, M);
                }
            }
            if (!detach && ka->grad_h) { // dP_k/dh_k = s * (third column of to_world)
                const v3 ez = mk3(f.to_world[2], f.to_world[6], f.to_world[10]);
                gh[0] = f.s * dot3(ez, gP0); gh[1] = f.s * dot3(ez, gP1); gh[2] = f.s * dot3(ez, gP2);
                vr[0] = vi[0]; vr[1] = vi[1]; vr[2] = vi[2];
                vc[0] = vj[0]; vc[1] = vj[1]; vc[2] = vj[2];
                scatter = true;
                if (!sm) {
                    row_lo = min(row_lo, (uint32_t) min(vi[0], min(vi[1], vi[2])));
                    row_hi = max(row_hi, (uint32_t) max(vi[0], max(vi[1], vi[2])) + 1u);
                } else { // the vertex normals reach one row further: the band widens by their halo
                    row_lo = min(row_lo, (uint32_t) max(min(vi[0], min(vi[1], vi[2])) - 1, 0));
                    row_hi = max(row_hi, (uint32_t) min(max(vi[0], max(vi[1], vi[2])) + 2, f.H));
                }
                smv = sm;
            }
        }
        const uint64_t sm = __ballot(scatter);
        if (sm != 0ull) {
            float *grad_h = adj_kargs()->grad_h;
            const int W = adj_kargs()->f.W;
            int ar, ac;
            tile_anchor(sm, vr, vc, HF_ADJ_TILE / 4, ar, ac); // from the first scattering lane
            hf_tile_rows<HF_ADJ_TILE> rows = 0u;
            if (scatter)
#pragma unroll
                for (int k = 0; k < 3; ++k) tile_add<HF_ADJ_TILE>(acc, ar, ac, vr[k], vc[k], gh[k], grad_h, W, rows);
            if (SMOOTH && smv) {
                const hf_dev_field f = load_field(&adj_kargs()->f);
                vertex_normals_vjp(f, vr, vc, height_axis(f), gnv, [&](int r, int c, float g) {
                    tile_add<HF_ADJ_TILE>(acc, ar, ac, r, c, g, grad_h, W, rows);
                });
            }
            tile_flush<HF_ADJ_TILE>(acc, ar, ac, rows, grad_h, W, (int) lane);
        }
        if (RAYGRAD && valid) {
            hf_adj_kargs kb = adj_kargs();
            if (kb->go[0]) { (kb->go[0] + ub)[lo] = go.x; (kb->go[1] + ub)[lo] = go.y; (kb->go[2] + ub)[lo] = go.z; }
            if (kb->gd[0]) { (kb->gd[0] + ub)[lo] = gd.x; (kb->gd[1] + ub)[lo] = gd.y; (kb->gd[2] + ub)[lo] = gd.z; }
        }
    }
    uint32_t *band = adj_kargs()->row_band;
    if (band) {
        // Per wave that scattered at all -- and only when it WIDENS the band: 65 k waves doing two atomics each on the
        // same two words cost the launch 0.9 ms (same-address atomics serialise); a relaxed read first (a stale value
        // only costs a redundant atomic) leaves the handful of waves that see the band grow.
        const uint32_t wl = wave_min_u32(row_lo), wh = wave_max_u32(row_hi);
        if (lane == 0u && wl < wh) {
            if (wl < __hip_atomic_load(band, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(band, wl);
            if (wh > __hip_atomic_load(band + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(band + 1, wh);
        }
    }
    if constexpr (XFORM) xform_block_store(M, slab);
}
template <bool RAYGRAD>
__global__ __launch_bounds__(HF_BLOCK, 5) void hf_adjoint_kernel(hf_adjoint_args a_) {
    (void) a_;
    __shared__ float s_acc[HF_BLOCK / 64][HF_ADJ_TILE * HF_ADJ_TILE];
    adjoint_body<RAYGRAD, false>(s_acc[threadIdx.x >> 6]);
}
template <bool RAYGRAD>
__global__ __launch_bounds__(HF_BLOCK, 4) void hf_adjoint_smooth_kernel(hf_adjoint_args a_) {
    (void) a_;
    __shared__ float s_acc[HF_BLOCK / 64][HF_ADJ_TILE * HF_ADJ_TILE];
    adjoint_body<RAYGRAD, true>(s_acc[threadIdx.x >> 6]);
}
// the transform-gradient instantiations.  Flat: the bound of hf_adjoint_kernel (87 / 96 VGPRs).  Smooth: one wave
// per SIMD less than hf_adjoint_smooth_kernel -- at 128 VGPRs the 12 accumulators and the 1-ring VJP of the vertex
// normals spilled 27 / 47 registers (144 / 176 bytes of private segment per lane)
template <bool RAYGRAD>
__global__ __launch_bounds__(HF_BLOCK, 5) void hf_adjoint_xform_kernel(hf_adjoint_args a_, float *slab) {
    (void) a_;
    __shared__ float s_acc[HF_BLOCK / 64][HF_ADJ_TILE * HF_ADJ_TILE];
    adjoint_body<RAYGRAD, false, true>(s_acc[threadIdx.x >> 6], slab);
}
template <bool RAYGRAD>
__global__ __launch_bounds__(HF_BLOCK, 3) void hf_adjoint_xform_smooth_kernel(hf_adjoint_args a_, float *slab) {
    (void) a_;
    __shared__ float s_acc[HF_BLOCK / 64][HF_ADJ_TILE * HF_ADJ_TILE];
    adjoint_body<RAYGRAD, true, true>(s_acc[threadIdx.x >> 6], slab);
}

void hf_launch_adjoint(const hf_dev_field &f, size_t n, const hf_rays_t *rays, const hf_pi_const_t *pi,
                       const uint8_t *active, const hf_si_grad_t *gs, uint32_t flags, float *grad_h,
                       float *const grad_o[3], float *const grad_d[3], uint32_t *row_band, hipStream_t stream,
                       const float4 *vn, float *grad_to_world, void *slab) {
    if (n == 0) return;
    hf_adjoint_args a;
    a.f = f; a.n = n; a.rays = *rays; a.pi = *pi; a.active = active; a.g = *gs; a.flags = flags; a.grad_h = grad_h;
    a.row_band = row_band; a.vn = vn;
    for (int k = 0; k < 3; ++k) { a.go[k] = grad_o ? grad_o[k] : nullptr; a.gd[k] = grad_d ? grad_d[k] : nullptr; }
    const bool rg = grad_o || grad_d;
    if (grad_to_world) { // slab: hf_xform_slab_bytes(n), this launch's alone
        void (*kx)(hf_adjoint_args, float *) = vn ? (rg ? hf_adjoint_xform_smooth_kernel<true> : hf_adjoint_xform_smooth_kernel<false>)
                                                  : (rg ? hf_adjoint_xform_kernel<true> : hf_adjoint_xform_kernel<false>);
        const int grid = grid_for(n, HF_XFORM_GRID_CAP);
        hipLaunchKernelGGL(kx, dim3(grid), dim3(HF_BLOCK), 0, stream, a, (float *) slab);
        xform_sum((const float *) slab, grid, grad_to_world, stream);
        return;
    }
    void (*kernel)(hf_adjoint_args) = vn ? (rg ? hf_adjoint_smooth_kernel<true> : hf_adjoint_smooth_kernel<false>)
                                         : (rg ? hf_adjoint_kernel<true> : hf_adjoint_kernel<false>);
    hipLaunchKernelGGL(kernel, dim3(grid_for(n)), dim3(HF_BLOCK), 0, stream, a);
}

// ---------------------------------------------------------------------------------
// tangent: forward mode of compute_si (the transpose of hf_adjoint_kernel, term for term), no scatter.  The forward
// sweep over the same hit-geometry quantities; prim_world also yields the vertex tangents dP_k
// ---------------------------------------------------------------------------------
// Shaped like hf_si_kernel (one block per 256 rays, arguments from the kernarg segment where they are used, every row
// stored as soon as it is final): a hit lane issues one batch of independent loads (the rest of pi, o, d and the ray
// tangents), then one round trip for the three heights and three height tangents of its triangle.  A missed lane reads
// pi.t (and active) and stores zeros.
struct hf_tangent_args {
    hf_dev_field f;
    size_t n;
    hf_rays_t rays;
    hf_pi_const_t pi;
    const uint8_t *active;
    const float *dh;            // [H*W] height tangent, NULL = zero
    const float *d_o[3], *d_d[3]; // per-ray tangents, NULL rows = zero
    hf_si_tangent_t out;        // NULL rows are not written
    uint32_t flags;
    const float4 *vn;           // hf_tangent_smooth_kernel: the handle's vertex normals
};
typedef const __attribute__((address_space(4))) hf_tangent_args *hf_tan_kargs;
// hf_eval_parameterization_tangent (tangent_body<..., PARAM>): the query uv rows follow the common arguments, whose rays
// and pi are not read
struct hf_param_tangent_args {
    hf_tangent_args a;
    const float *uv[2];
};

// RAYTAN: d_o or d_d is given (without them the ray terms are dead code).
// SMOOTH (hf_tangent_smooth_kernel): sh_n is the interpolated vertex normal; its tangent takes the barycentric tangents
// and the tangents of the three vertex normals, evaluated on the fly from h and dh (vertex_normal_jvp: no atomics).
// XFORM (hf_tangent_xform_kernel, hf_tangent_xform_smooth_kernel): the vertices also move by dM (q_k, 1) for the tangent
// dM (12 device floats) of to_world, and so do the 1-rings of the vertex normals (vertex_normals_jvp_xform).
// PARAM (hf_param_tangent*_kernel, hf_eval_parameterization_tangent): the kernel argument is an hf_param_tangent_args; a
// lane's (prim, b) is param_lookup of its query uv instead of pi (outside the texture square: zero tangents).  The flags
// carry HF_RAY_FOLLOWSHAPE and t gets no tangent (0): the FollowShape t of the UV-space ray is not evaluated.
template <bool RAYTAN, bool SMOOTH, bool XFORM = false, bool PARAM = false>
__device__ __forceinline__ void tangent_body(const float *dMp = nullptr) {
    float dM[12]; // XFORM: wave-uniform
    if constexpr (XFORM) {
#pragma unroll
        for (int j = 0; j < 12; ++j) dM[j] = dMp[j];
    }
    const uint32_t lane = threadIdx.x & 63u;
    const size_t stride = (size_t) gridDim.x * HF_BLOCK;
    for (size_t ub = (size_t) blockIdx.x * HF_BLOCK + (threadIdx.x & ~63u);; ub += stride) {
        hf_tan_kargs ka = (hf_tan_kargs) __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka)); // opaque: keeps the loads that follow where they are written
        const size_t n = ka->n;
        if (ub >= n) break; // wave-uniform
        if (lane >= n - ub) continue;
        const uint32_t lo = lane;
        uint32_t qprim = 0u; // PARAM: the lane's triangle and barycentrics
        float qb1 = 0.f, qb2 = 0.f;
        bool act;
        if constexpr (PARAM) {
            const auto *kp = (const __attribute__((address_space(4))) hf_param_tangent_args *) ka;
            const float u = (kp->uv[0] + ub)[lo], v = (kp->uv[1] + ub)[lo];
            const uint8_t *active = ka->active;
            act = (active ? ((active + ub)[lo] != 0) : true) && param_lookup(ka->f.W, ka->f.H, u, v, qprim, qb1, qb2);
        } else {
            const float t_in = (ka->pi.t + ub)[lo];
            const uint8_t *active = ka->active;
            act = (active ? ((active + ub)[lo] != 0) : true) && (t_in != __builtin_inff());
        }
        const v3 z3 = mk3(0.f, 0.f, 0.f);
        if (!act) { // missed / inactive: exactly zero tangents
            st(ka->out.t, ub, lo, 0.f); st3(ka->out.p, ub, lo, z3); st3(ka->out.n, ub, lo, z3);
            st(ka->out.uv[0], ub, lo, 0.f); st(ka->out.uv[1], ub, lo, 0.f); st3(ka->out.sh_n, ub, lo, z3);
            st3(ka->out.dp_du, ub, lo, z3); st3(ka->out.dp_dv, ub, lo, z3);
            continue;
        }
        const uint32_t flags = ka->flags;
        const bool follow = (flags & HF_RAY_FOLLOWSHAPE) != 0, detach = (flags & HF_RAY_DETACHSHAPE) != 0;
        // ONE batch of independent loads: pi, the ray, the ray tangents
        float b1 = qb1, b2 = qb2;
        uint32_t prim = qprim;
        v3 o = z3, d = z3;
        if constexpr (!PARAM) {
            b1 = (ka->pi.prim_uv[0] + ub)[lo]; b2 = (ka->pi.prim_uv[1] + ub)[lo];
            prim = (ka->pi.prim_index + ub)[lo];
            o = mk3((ka->rays.o[0] + ub)[lo], (ka->rays.o[1] + ub)[lo], (ka->rays.o[2] + ub)[lo]);
            d = mk3((ka->rays.d[0] + ub)[lo], (ka->rays.d[1] + ub)[lo], (ka->rays.d[2] + ub)[lo]);
        }
        const float b0 = 1.f - b1 - b2;
        v3 dO = z3, dD = z3;
        if (RAYTAN) {
            dO = mk3(ldu(ka->d_o[0], ub, lo), ldu(ka->d_o[1], ub, lo), ldu(ka->d_o[2], ub, lo));
            dD = mk3(ldu(ka->d_d[0], ub, lo), ldu(ka->d_d[1], ub, lo), ldu(ka->d_d[2], ub, lo));
        }
        // then the three heights and their three tangents: one round trip (DetachShape: the heights carry no tangent)
        const hf_dev_field f = load_field(&ka->f);
        v3 P[3], dP[3];
        float U[3], V[3];
        int vi[3], vj[3];
        prim_world(f, prim, P, U, V, vi, vj, dP, detach ? nullptr : ka->dh);
        if constexpr (XFORM) {
            if (!detach) {
                v3 q[3];
                prim_local(f, vi, vj, q);
#pragma unroll
                for (int k = 0; k < 3; ++k) dP[k] = dP[k] + xform_point(dM, q[k]);
            }
        }
        const bool sm = SMOOTH && smooth_sh(flags);
        v3 NV[3];
        if (sm) load_vn(f, ka->vn, vi, vj, NV);
        const v3 e1 = P[1] - P[0], e2 = P[2] - P[0];
        const v3 de1 = dP[1] - dP[0], de2 = dP[2] - dP[0];
        // n = sh_n = +-normalize(cross(e1, e2))  (smooth: n only; sh_n below)
        v3 ddu = z3, ddv = z3;
        {
            const auto [nn, r] = unit_normal(e1, e2);
            const v3 dN = face_normal_jvp(e1, e2, de1, de2);
            const v3 dn = dnormalize(nn, f.flip ? -r : r, dN);
            st3(ka->out.n, ub, lo, dn);
            if (!sm) st3(ka->out.sh_n, ub, lo, dn);
            // without dPdUV, dp_du / dp_dv = coordinate_system of the normal before flip_normals (mesh.cpp:762)
            if (!(flags & HF_RAY_DPDUV)) coordinate_system_jvp(nn, f.flip ? neg3(dn) : dn, ddu, ddv);
        }
        // dp_du / dp_dv with dPdUV: linear in the edges (the texcoord differences are constant)
        {
            if (flags & HF_RAY_DPDUV) {
                const auto [du0, dv0, du1, dv1, det, inv_det] = uv_diff(U, V);
                if (det != 0.f) {
                    const float a0 = dv1 * inv_det, a1 = -dv0 * inv_det, c0 = -du1 * inv_det, c1 = du0 * inv_det;
                    ddu = mk3(a0 * de1.x + a1 * de2.x, a0 * de1.y + a1 * de2.y, a0 * de1.z + a1 * de2.z);
                    ddv = mk3(c0 * de1.x + c1 * de2.x, c0 * de1.y + c1 * de2.y, c0 * de1.z + c1 * de2.z);
                }
            }
            st3(ka->out.dp_du, ub, lo, ddu);
            st3(ka->out.dp_dv, ub, lo, ddv);
        }
        // barycentric tangents: the differentiable Moeller-Trumbore (default) or frozen (FollowShape)
        float du = 0.f, dv = 0.f, dt = 0.f;
        if (!follow) {
            const auto [pvec, tvec, qvec, inv, a_u, a_v, a_t] = mt_terms(o, d, P[0], e1, e2);
            const v3 p1 = cross3(dD, e2), p2 = cross3(d, de2);
            const v3 dpvec = mk3(p1.x + p2.x, p1.y + p2.y, p1.z + p2.z);
            const v3 dtv = dO - dP[0];
            const v3 q1 = cross3(dtv, e1), q2 = cross3(tvec, de1);
            const v3 dqvec = mk3(q1.x + q2.x, q1.y + q2.y, q1.z + q2.z);
            const float dinv = -(dot3(de1, pvec) + dot3(e1, dpvec)) * inv * inv;
            du = (dot3(dtv, pvec) + dot3(tvec, dpvec)) * inv + a_u * dinv;
            dv = (dot3(dD, qvec) + dot3(d, dqvec)) * inv + a_v * dinv;
            dt = (dot3(de2, qvec) + dot3(e2, dqvec)) * inv + a_t * dinv;
        }
        if (sm) { // sh_n = +-normalize(sum b_k N_k): d(sum b_k N_k) = du (N_1 - N_0) + dv (N_2 - N_0) + sum b_k dN_k
            const v3 ns = bary_normal(NV, b0, b1, b2);
            const float r = rsqrt_ieee(dot3(ns, ns));
            v3 dns = z3;
            axpy3(du, NV[1] - NV[0], dns);
            axpy3(dv, NV[2] - NV[0], dns);
            const float *dh = detach ? nullptr : ka->dh;
            if constexpr (XFORM) {
                if (!detach) {
                    const float bk[3] = { b0, b1, b2 };
                    vertex_normals_jvp_xform(f, vi, vj, height_axis(f), bk, dh, dM, dns);
                }
            } else if (dh) {
                const float bk[3] = { b0, b1, b2 };
                vertex_normals_jvp(f, vi, vj, height_axis(f), bk, dh, dns);
            }
            st3(ka->out.sh_n, ub, lo, dnormalize(ns * r, f.flip ? -r : r, dns));
        }
        // p = sum b_k P_k:  dp = du e1 + dv e2 + sum b_k dP_k
        const v3 dp = mk3(du * e1.x + dv * e2.x + (b0 * dP[0].x + b1 * dP[1].x + b2 * dP[2].x),
                          du * e1.y + dv * e2.y + (b0 * dP[0].y + b1 * dP[1].y + b2 * dP[2].y),
                          du * e1.z + dv * e2.z + (b0 * dP[0].z + b1 * dP[1].z + b2 * dP[2].z));
        if (!PARAM && follow) { // t = sqrt(|p - o|^2 / |d|^2)
            const auto [po, dd, tt] = follow_t(bary_point(P, b0, b1, b2), o, d);
            dt = dot3(po, dp - dO) / (tt * dd) - (tt / dd) * dot3(d, dD);
        }
        st(ka->out.t, ub, lo, dt);
        st3(ka->out.p, ub, lo, dp);
        float duv0 = du, duv1 = dv;
        if (flags & (HF_RAY_UV | HF_RAY_DPDUV)) {
            duv0 = du * (U[1] - U[0]) + dv * (U[2] - U[0]);
            duv1 = du * (V[1] - V[0]) + dv * (V[2] - V[0]);
        }
        st(ka->out.uv[0], ub, lo, duv0);
        st(ka->out.uv[1], ub, lo, duv1);
    }
}
template <bool RAYTAN>
__global__ __launch_bounds__(HF_BLOCK) void hf_tangent_kernel(hf_tangent_args a_) { (void) a_; tangent_body<RAYTAN, false>(); }
template <bool RAYTAN>
__global__ __launch_bounds__(HF_BLOCK) void hf_tangent_smooth_kernel(hf_tangent_args a_) { (void) a_; tangent_body<RAYTAN, true>(); }
template <bool RAYTAN>
__global__ __launch_bounds__(HF_BLOCK) void hf_tangent_xform_kernel(hf_tangent_args a_, const float *dM) {
    (void) a_;
    tangent_body<RAYTAN, false, true>(dM);
}
template <bool RAYTAN>
__global__ __launch_bounds__(HF_BLOCK) void hf_tangent_xform_smooth_kernel(hf_tangent_args a_, const float *dM) {
    (void) a_;
    tangent_body<RAYTAN, true, true>(dM);
}

void hf_launch_tangent(const hf_dev_field &f, size_t n, const hf_rays_t *rays, const hf_pi_const_t *pi,
                       const uint8_t *active, uint32_t flags, const float *dh, const float *const d_o[3],
                       const float *const d_d[3], const hf_si_tangent_t *out, hipStream_t stream, const float4 *vn,
                       const float *d_to_world) {
    if (n == 0) return;
    hf_tangent_args a;
    a.f = f; a.n = n; a.rays = *rays; a.pi = *pi; a.active = active; a.dh = dh; a.out = *out; a.flags = flags; a.vn = vn;
    bool raytan = false;
    for (int k = 0; k < 3; ++k) {
        a.d_o[k] = d_o ? d_o[k] : nullptr; a.d_d[k] = d_d ? d_d[k] : nullptr;
        raytan = raytan || a.d_o[k] || a.d_d[k];
    }
    const dim3 grid(grid_for(n, HF_SI_GRID_CAP)), block(HF_BLOCK);
    if (d_to_world) {
        void (*kx)(hf_tangent_args, const float *) = vn ? (raytan ? hf_tangent_xform_smooth_kernel<true> : hf_tangent_xform_smooth_kernel<false>)
                                                        : (raytan ? hf_tangent_xform_kernel<true> : hf_tangent_xform_kernel<false>);
        hipLaunchKernelGGL(kx, grid, block, 0, stream, a, d_to_world);
        return;
    }
    void (*kernel)(hf_tangent_args) = vn ? (raytan ? hf_tangent_smooth_kernel<true> : hf_tangent_smooth_kernel<false>)
                                         : (raytan ? hf_tangent_kernel<true> : hf_tangent_kernel<false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, a);
}

// ---------------------------------------------------------------------------------
// Smooth shading: the handle's vertex normals (one float4 per vertex: one 16-byte gather per vertex of a hit) and the
// forward-only dn_du / dn_dv of hf_shading_derivatives
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(HF_BLOCK) void hf_vertex_normals_kernel(hf_dev_field f, float4 *__restrict__ vn) {
    const uint32_t x = blockIdx.x * HF_BLOCK + threadIdx.x; // (W H <= 2^30, checked by hf_create)
    if (x >= (uint32_t) f.W * (uint32_t) f.H) return;
    const int i = (int) (x / (uint32_t) f.W), j = (int) (x - (uint32_t) i * (uint32_t) f.W);
    const v3 n = vertex_normal(f, i, j);
    vn[x] = make_float4(n.x, n.y, n.z, 0.f);
}

void hf_launch_build_normals(const hf_dev_field &f, float4 *vn, hipStream_t stream) {
    const uint32_t n = (uint32_t) f.W * (uint32_t) f.H;
    hipLaunchKernelGGL(hf_vertex_normals_kernel, dim3((n + HF_BLOCK - 1) / HF_BLOCK), dim3(HF_BLOCK), 0, stream, f, vn);
}

struct hf_shading_deriv_args {
    int32_t W;
    size_t n;
    hf_pi_const_t pi;
    const uint8_t *active;
    const float4 *vn; // NULL: flat shading (zeros)
    float *dn_du[3], *dn_dv[3];
};
// mesh.cpp:818-829: with N = sum b_k N_k and il = |N|^-1, n = N il,
//   dn_du = (N_1 - N_0) il - n <n, (N_1 - N_0) il>,  dn_dv = (N_2 - N_0) il - n <n, (N_2 - N_0) il>
// (derivatives with respect to the barycentrics b1, b2; not flipped by flip_normals, as in the reference)
__global__ __launch_bounds__(HF_BLOCK) void hf_shading_derivatives_kernel(hf_shading_deriv_args a) {
    const size_t stride = (size_t) gridDim.x * HF_BLOCK;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += stride) {
        v3 du = mk3(0.f, 0.f, 0.f), dv = du;
        const bool act = (a.active ? a.active[i] != 0 : true) && a.pi.t[i] != __builtin_inff();
        if (act && a.vn) {
            const float b1 = a.pi.prim_uv[0][i], b2 = a.pi.prim_uv[1][i], b0 = 1.f - b1 - b2;
            hf_dev_field f;
            f.W = a.W;
            int vi[3], vj[3];
            prim_vertex_ids(f, a.pi.prim_index[i], vi, vj);
            v3 N[3];
            load_vn(f, a.vn, vi, vj, N);
            const v3 ns = bary_normal(N, b0, b1, b2);
            const float il = rsqrt_ieee(dot3(ns, ns));
            const v3 n = ns * il;
            du = (N[1] - N[0]) * il;
            dv = (N[2] - N[0]) * il;
            du = fma3(n, -dot3(n, du), du);
            dv = fma3(n, -dot3(n, dv), dv);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (a.dn_du[c]) a.dn_du[c][i] = c == 0 ? du.x : c == 1 ? du.y : du.z;
            if (a.dn_dv[c]) a.dn_dv[c][i] = c == 0 ? dv.x : c == 1 ? dv.y : dv.z;
        }
    }
}

void hf_launch_shading_derivatives(const hf_dev_field &f, size_t n, const hf_pi_const_t *pi, const uint8_t *active,
                                   float *const dn_du[3], float *const dn_dv[3], const float4 *vn, hipStream_t stream) {
    if (n == 0) return;
    hf_shading_deriv_args a;
    a.W = f.W; a.n = n; a.pi = *pi; a.active = active; a.vn = vn;
    for (int c = 0; c < 3; ++c) { a.dn_du[c] = dn_du ? dn_du[c] : nullptr; a.dn_dv[c] = dn_dv ? dn_dv[c] : nullptr; }
    hipLaunchKernelGGL(hf_shading_derivatives_kernel, dim3(grid_for(n)), dim3(HF_BLOCK), 0, stream, a);
}

// ---------------------------------------------------------------------------------
// Backward of the warped-area reparameterisation with respect to the heights, all auxiliary samples of a ray in ONE
// pass (reparam.py:224-333 for the shape parameter): the weights of the samples and their sums Z, dZ (first loop,
// :236-256), then for every auxiliary HIT the gradient of its V_direct = (si.p - o) / si.t through the FollowShape
// surface interaction to the three heights of the hit triangle (third loop, :296-325).  Nothing but the auxiliary
// hits (pi + si.boundary_test per sample) is read: the auxiliary direction is regenerated from (d, k, seed), si.p and
// the FollowShape si.t are re-derived from pi with compute_si's helpers (bary_point, follow_t).  A ray none of whose
// samples hit does not reach the heights and is skipped after its num_rays reads of pi.t.
// Sample k of ray i sits at [k * stride + i] of every per-sample array.
// ---------------------------------------------------------------------------------
struct hf_reparam_bwd_args {
    size_t n, stride;
    const float *o[3], *d[3];
    const uint8_t *active;
    uint32_t num_rays, seed;
    float kappa, exponent;
    int antithetic;
    const uint32_t *ray_id;
    hf_pi_const_t pi;
    const float *si_bt;
    const float *g_dir[3], *g_div;
    float *grad_h;
};

#ifndef HF_RB_KEEP
#define HF_RB_KEEP 4u // samples whose direction and weight the first loop of hf_reparam_backward_kernel keeps for the third
#endif
#ifndef HF_RB_ANCHOR
#define HF_RB_ANCHOR (HF_RB_TILE * 7 / 16) // the tile starts this many texels before the first hit of the batch (rows and columns): 8 / 16 /
                                          // 24 / 32 of 64 measured 21.4 / 20.8 / 20.5 / 20.5 ms for the backward with 4 samples (profiles/r04_ab/r04_rb)
#endif
#ifndef HF_RB_TILE
#define HF_RB_TILE 64 // the auxiliary hits of a pixel spread over tens of cells: a larger tile than hf_adjoint_kernel's
#endif
// (one argument struct, read from the kernarg segment where it is used: see hf_adjoint_kernel)
struct hf_reparam_bwd_kargs {
    hf_dev_field f;
    hf_reparam_bwd_args a;
};
__global__ __launch_bounds__(HF_BLOCK, (HF_RB_TILE > 32 ? 2 : 5)) void hf_reparam_backward_kernel(hf_reparam_bwd_kargs k_) {
    (void) k_;
    typedef const __attribute__((address_space(4))) hf_reparam_bwd_kargs *kargs_t;
    kargs_t kc = (kargs_t) __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kc));
    const size_t a_n = kc->a.n;
    __shared__ float s_acc[HF_BLOCK / 64][HF_RB_TILE * HF_RB_TILE]; // per-wave accumulation tile, as in hf_adjoint_kernel
    float *acc = s_acc[threadIdx.x >> 6];
    const int lane = (int) (threadIdx.x & 63u);
    for (int k = lane; k < HF_RB_TILE * HF_RB_TILE; k += 64) acc[k] = 0.f;
    hf_reparam_args sa = {}; // what the sampling helpers read
    sa.seed = kc->a.seed; sa.kappa = kc->a.kappa; sa.exponent = kc->a.exponent; sa.antithetic = kc->a.antithetic;
    sa.ray_id = kc->a.ray_id;
    const size_t stride = (size_t) gridDim.x * HF_BLOCK;
    const size_t n_round = (a_n + HF_BLOCK - 1) / HF_BLOCK * HF_BLOCK; // whole waves stay in the loop (ballots below)
    for (size_t i_raw = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i_raw < n_round; i_raw += stride) {
        kargs_t ka = (kargs_t) __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka)); // opaque: keeps the loads that follow inside the loop body
        const bool valid = i_raw < a_n;
        const size_t i = valid ? i_raw : a_n - 1;
        const bool act = valid && (ka->a.active ? (ka->a.active[i] != 0) : true);
        uint32_t hm = 0u; // samples that hit
        for (uint32_t k = 0; k < ka->a.num_rays; ++k)
            hm |= (act && ka->a.pi.t[k * ka->a.stride + i] != __builtin_inff()) ? (1u << k) : 0u;
        if (__ballot(hm != 0u) == 0ull) continue; // wave-uniform
        v3 o = mk3(0.f, 0.f, 0.f), d = o;
        hf_vd_grad g = { o, 0.f };
        v3 kept_om[HF_RB_KEEP], kept_dw[HF_RB_KEEP];
        float kept_w[HF_RB_KEEP];
#pragma unroll
        for (uint32_t c = 0; c < HF_RB_KEEP; ++c) { kept_om[c] = o; kept_dw[c] = o; kept_w[c] = 0.f; }
        if (hm != 0u) {
            o = mk3(ka->a.o[0][i], ka->a.o[1][i], ka->a.o[2][i]);
            d = mk3(ka->a.d[0][i], ka->a.d[1][i], ka->a.d[2][i]);
            // first loop: Z = sum_k w_k, dZ = sum_k d_w_omega_k, in sample order from zero.  The first HF_RB_KEEP samples'
            // direction, weight and weight gradient are kept for the third loop (registers are free here: the tile's LDS
            // limits the kernel to two waves per SIMD), the others are drawn again there
            float Zs = 0.f;
            v3 dZ = mk3(0.f, 0.f, 0.f);
            for (uint32_t k = 0; k < ka->a.num_rays; ++k) {
                sa.k = k;
                hf_aux_sample q;
                aux_sample(sa, i, d, q);
                const float B = ((hm >> k) & 1u) ? ka->a.si_bt[k * ka->a.stride + i] : 1.0f;
                float w;
                v3 dw;
                reparam_weight(sa, q, d, B, w, dw);
                Zs += w;
                dZ.x += dw.x; dZ.y += dw.y; dZ.z += dw.z;
#pragma unroll
                for (uint32_t c = 0; c < HF_RB_KEEP; ++c)
                    if (k == c) { kept_om[c] = q.omega; kept_w[c] = w; kept_dw[c] = dw; } // (k is wave-uniform)
            }
            g = vdirect_grad_ray(d, mk3(ka->a.g_dir[0][i], ka->a.g_dir[1][i], ka->a.g_dir[2][i]), ka->a.g_div[i], Zs, [&] { return dZ; });
        }
        // third loop: the auxiliary hits, sample by sample (wave-uniform loop, lanes with a hit take part); all
        // samples of the batch go into the tile before it is flushed
        int ar = 0, ac = 0;   // tile anchor (wave-uniform), set at the first sample with a hit
        bool anchored = false;
        hf_tile_rows<HF_RB_TILE> rows = 0u;
        const uint32_t hm_any = wave_or(hm);
        for (uint32_t k = 0; k < ka->a.num_rays; ++k) {
            if (((hm_any >> k) & 1u) == 0u) continue; // wave-uniform
            const bool hit = ((hm >> k) & 1u) != 0u;
            float gh[3] = { 0.f, 0.f, 0.f };
            int vr[3] = { 0, 0, 0 }, vc[3] = { 0, 0, 0 };
            if (hit) {
                sa.k = k;
                hf_aux_sample q;
                float w;
                v3 dw;
                if (k < HF_RB_KEEP) { // wave-uniform: the values of the first loop (the same expressions on the same inputs)
                    q.omega = kept_om[0]; w = kept_w[0]; dw = kept_dw[0];
#pragma unroll
                    for (uint32_t c = 1; c < HF_RB_KEEP; ++c)
                        if (k == c) { q.omega = kept_om[c]; w = kept_w[c]; dw = kept_dw[c]; }
                    q.sy = 0.f;
                    coordinate_system(d, q.fs, q.ft);
                } else {
                    aux_sample(sa, i, d, q);
                    reparam_weight(sa, q, d, ka->a.si_bt[k * ka->a.stride + i], w, dw);
                }
                const v3 gVd = vdirect_grad_sample(g, w, dw);
                const v3 da = frame_to_world(q, d, q.omega); // the auxiliary direction (= hf_reparam_aux_kernel's)
                const float b1 = ka->a.pi.prim_uv[0][k * ka->a.stride + i], b2 = ka->a.pi.prim_uv[1][k * ka->a.stride + i];
                const float b0 = 1.f - b1 - b2;
                v3 P[3];
                float U[3], V[3];
                int vi[3], vj[3];
                prim_world(load_field(&ka->f), ka->a.pi.prim_index[k * ka->a.stride + i], P, U, V, vi, vj);
                // V_direct = (p - o) / t with the FollowShape t = sqrt(|p - o|^2 / |d_aux|^2) of compute_si
                const auto [po, dda, tt] = follow_t(bary_point(P, b0, b1, b2), o, da);
                auto [gp, gt] = vdirect_grad_hit(gVd, po, tt);
                axpy3(gt / (tt * dda), po, gp); // t's dependence on p (hf_adjoint_kernel, FollowShape branch)
                // p = sum b_k P_k with detached barycentrics; dP_k/dh_k = s * (third column of to_world)
                const v3 ez = mk3(ka->f.to_world[2], ka->f.to_world[6], ka->f.to_world[10]);
                const v3 z3 = mk3(0.f, 0.f, 0.f);
                v3 gP0 = z3, gP1 = z3, gP2 = z3;
                axpy3(b0, gp, gP0); axpy3(b1, gp, gP1); axpy3(b2, gp, gP2);
                const float fs = ka->f.s;
                gh[0] = fs * dot3(ez, gP0); gh[1] = fs * dot3(ez, gP1); gh[2] = fs * dot3(ez, gP2);
                vr[0] = vi[0]; vr[1] = vi[1]; vr[2] = vi[2];
                vc[0] = vj[0]; vc[1] = vj[1]; vc[2] = vj[2];
            }
            if (!anchored) { // wave-uniform: the first sample with a hit anchors the tile
                tile_anchor(__ballot(hit), vr, vc, HF_RB_ANCHOR, ar, ac);
                anchored = true;
            }
            if (hit)
#pragma unroll
                for (int c = 0; c < 3; ++c) tile_add<HF_RB_TILE>(acc, ar, ac, vr[c], vc[c], gh[c], ka->a.grad_h, ka->f.W, rows);
        }
        tile_flush<HF_RB_TILE>(acc, ar, ac, rows, ka->a.grad_h, ka->f.W, lane);
    }
}

void hf_launch_reparam_backward(const hf_dev_field &f, const hf_reparam_args &ra, uint32_t num_rays, size_t stride,
                                const hf_pi_const_t *pi, float *grad_h, hipStream_t stream) {
    if (ra.n == 0) return;
    hf_reparam_bwd_args a = {};
    a.n = ra.n; a.stride = stride; a.active = ra.active; a.num_rays = num_rays; a.seed = ra.seed; a.kappa = ra.kappa;
    a.exponent = ra.exponent; a.antithetic = ra.antithetic; a.ray_id = ra.ray_id;
    for (int c = 0; c < 3; ++c) { a.o[c] = ra.o[c]; a.d[c] = ra.d[c]; a.g_dir[c] = ra.g_dir[c]; }
    a.g_div = ra.g_div; a.si_bt = ra.si_bt; a.pi = *pi; a.grad_h = grad_h;
    hf_reparam_bwd_kargs k;
    k.f = f; k.a = a;
    hipLaunchKernelGGL(hf_reparam_backward_kernel, dim3(grid_for(ra.n)), dim3(HF_BLOCK), 0, stream, k);
}

// ---------------------------------------------------------------------------------
// Forward mode of the warped-area reparameterisation (reparam.py:155-221): for every ray, from its num_rays kept
// auxiliary hits, V_theta = sum_k w_k dV_k / Z and div = (sum_k <d_w_omega_k, dV_k> - <V_theta, dZ>) / Z, where dV_k is
// the tangent of V_direct_k = (p - o) / t (FollowShape p and t, detached barycentrics) for a hit and ray.d's tangent
// for a miss.  The weights are detached, so ONE pass over the samples yields Z, dZ and both numerators: every sample is
// drawn once and nothing is kept across samples.  A gather per hit and one store per output row: no atomics (bitwise
// repeatable).  Instantiated on the tangents present: DH heights, RAY ray.o / ray.d, XF to_world.
// ---------------------------------------------------------------------------------
struct hf_reparam_tan_args {
    size_t n, stride;
    const float *o[3], *d[3];
    const uint8_t *active;
    uint32_t num_rays, seed;
    float kappa, exponent;
    int antithetic;
    const uint32_t *ray_id;
    hf_pi_const_t pi;
    const float *si_bt;
    const float *dh, *d_o[3], *d_d[3], *dM; // tangents (DH, RAY, XF); rows of d_o / d_d may be NULL (zero)
    float *out_dir[3], *out_div;
};
struct hf_reparam_tan_kargs {
    hf_dev_field f;
    hf_reparam_tan_args a;
};
template <bool DH, bool RAY, bool XF>
__global__ __launch_bounds__(HF_BLOCK) void hf_reparam_tangent_kernel(hf_reparam_tan_kargs k_) {
    (void) k_;
    typedef const __attribute__((address_space(4))) hf_reparam_tan_kargs *kargs_t;
    kargs_t kc = (kargs_t) __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kc));
    const size_t a_n = kc->a.n;
    float dM[12]; // XF: wave-uniform
    if constexpr (XF) {
#pragma unroll
        for (int j = 0; j < 12; ++j) dM[j] = kc->a.dM[j];
    }
    hf_reparam_args sa = {}; // what the sampling helpers read
    sa.seed = kc->a.seed; sa.kappa = kc->a.kappa; sa.exponent = kc->a.exponent; sa.antithetic = kc->a.antithetic;
    sa.ray_id = kc->a.ray_id;
    const size_t stride = (size_t) gridDim.x * HF_BLOCK;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a_n; i += stride) {
        kargs_t ka = (kargs_t) __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka)); // opaque: keeps the loads that follow inside the loop body
        const v3 z3 = mk3(0.f, 0.f, 0.f);
        const bool act = ka->a.active ? (ka->a.active[i] != 0) : true;
        v3 Vt = z3;
        float div = 0.f;
        const size_t sst = ka->a.stride;
        const uint32_t K = ka->a.num_rays;
        uint32_t hm = 0u; // samples that hit
        if (act)
            for (uint32_t k = 0; k < K; ++k) hm |= (ka->a.pi.t[k * sst + i] != __builtin_inff()) ? (1u << k) : 0u;
        // Without a ray tangent a miss contributes dV = 0, so a ray none of whose samples hit gets exactly 0 (what the
        // sums would give: +0 * iZ) without drawing its samples; a wave of such rays skips to the stores, as
        // hf_reparam_backward_kernel skips the waves that do not reach the heights
        const bool work = act && (RAY || hm != 0u);
        if (__ballot(work) != 0ull && work) {
            const v3 d = mk3(ka->a.d[0][i], ka->a.d[1][i], ka->a.d[2][i]);
            v3 o = z3, dO = z3, dD = z3, dfs = z3, dft = z3;
            if (hm != 0u) o = mk3(ka->a.o[0][i], ka->a.o[1][i], ka->a.o[2][i]);
            if constexpr (RAY) {
                dO = mk3(ldu(ka->a.d_o[0], 0, i), ldu(ka->a.d_o[1], 0, i), ldu(ka->a.d_o[2], 0, i));
                dD = mk3(ldu(ka->a.d_d[0], 0, i), ldu(ka->a.d_d[1], 0, i), ldu(ka->a.d_d[2], 0, i));
                coordinate_system_jvp(d, dD, dfs, dft); // Frame3f(d)'s tangent: the auxiliary directions follow d
            }
            // Z = sum_k w_k, dZ = sum_k d_w_omega_k and the numerators, in sample order from zero.  The loop is written
            // for latency: the records of sample k + 1 are requested before sample k is worked on, and a hit's heights
            // (and height tangents) before its sample is drawn, so that neither load round trip waits idle
            const hf_dev_field f = load_field(&ka->f);
            const v3 ez = height_axis(f); // dP_k/dh_k
            float Zs = 0.f, gdiv = 0.f;
            v3 dZ = z3, gV = z3;
            float nbt = 1.f, nb1 = 0.f, nb2 = 0.f; // the next sample's record (a hit's)
            uint32_t nprim = 0u;
            if (hm & 1u) { nbt = ka->a.si_bt[i]; nb1 = ka->a.pi.prim_uv[0][i]; nb2 = ka->a.pi.prim_uv[1][i]; nprim = ka->a.pi.prim_index[i]; }
            for (uint32_t k = 0; k < K; ++k) {
                const bool hit = ((hm >> k) & 1u) != 0u;
                const float B = hit ? nbt : 1.0f, b1 = nb1, b2 = nb2;
                const uint32_t prim = nprim;
                if (k + 1 < K && ((hm >> (k + 1)) & 1u)) { // (k + 1 < K first: a shift by 32 is not defined)
                    const size_t ik1 = (k + 1) * sst + i;
                    nbt = ka->a.si_bt[ik1]; nb1 = ka->a.pi.prim_uv[0][ik1]; nb2 = ka->a.pi.prim_uv[1][ik1];
                    nprim = ka->a.pi.prim_index[ik1];
                }
                int vi[3], vj[3];
                float hz[3] = { 0.f, 0.f, 0.f }, dz[3] = { 0.f, 0.f, 0.f };
                if (hit) { // the three heights and their tangents: prim_world's loads, used below
                    prim_vertex_ids(f, prim, vi, vj);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const size_t idx = (size_t) vi[c] * f.W + vj[c];
                        hz[c] = f.h[idx];
                        if constexpr (DH) dz[c] = ka->a.dh[idx];
                    }
                }
                sa.k = k;
                hf_aux_sample q;
                aux_sample(sa, i, d, q);
                float w;
                v3 dw;
                reparam_weight(sa, q, d, B, w, dw);
                Zs += w;
                dZ.x += dw.x; dZ.y += dw.y; dZ.z += dw.z;
                v3 dV = dD; // miss: V_direct = ray.d (reparam.py:93-95)
                if (hit) {
                    const float b0 = 1.f - b1 - b2;
                    v3 P[3], dP[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) { // prim_world's expressions; dP_k = dh_k ez (+ dM (q_k, 1))
                        const v3 ql = grid_local(f, vi[c], vj[c], hz[c]);
                        P[c] = xform_point(f.to_world, ql);
                        dP[c] = ez * dz[c];
                        if constexpr (XF) dP[c] = dP[c] + xform_point(dM, ql);
                    }
                    const v3 da = frame_to_world(q, d, q.omega); // the auxiliary direction (= hf_reparam_aux_kernel's)
                    // V_direct = (p - o) / t with the FollowShape t = sqrt(|p - o|^2 / |d_aux|^2) of compute_si
                    const auto [po, dda, tt] = follow_t(bary_point(P, b0, b1, b2), o, da);
                    const v3 rel = ((DH || XF) ? bary_point(dP, b0, b1, b2) : z3) - dO; // (p - o)'s tangent
                    float dt = dot3(po, rel) / (tt * dda);
                    if constexpr (RAY) { // d_aux = s(d) omega.x + t(d) omega.y + d omega.z, omega detached
                        const v3 dda_v = mk3(__builtin_fmaf(dD.x, q.omega.z, __builtin_fmaf(dft.x, q.omega.y, dfs.x * q.omega.x)),
                                             __builtin_fmaf(dD.y, q.omega.z, __builtin_fmaf(dft.y, q.omega.y, dfs.y * q.omega.x)),
                                             __builtin_fmaf(dD.z, q.omega.z, __builtin_fmaf(dft.z, q.omega.y, dfs.z * q.omega.x)));
                        dt -= tt * dot3(da, dda_v) / dda;
                    }
                    const float it = 1.0f / tt, c = dt * it * it;
                    dV = mk3(rel.x * it - po.x * c, rel.y * it - po.y * c, rel.z * it - po.z * c);
                }
                gV.x += w * dV.x; gV.y += w * dV.y; gV.z += w * dV.z;
                gdiv += dot3(dw, dV);
            }
            const float iZ = 1.0f / fmaxf(Zs, 1e-8f);
            Vt = gV * iZ;
            div = (gdiv - dot3(Vt, dZ)) * iZ;
        }
        ka->a.out_dir[0][i] = Vt.x; ka->a.out_dir[1][i] = Vt.y; ka->a.out_dir[2][i] = Vt.z;
        ka->a.out_div[i] = div;
    }
}

void hf_launch_reparam_tangent(const hf_dev_field &f, const hf_reparam_args &ra, uint32_t num_rays, size_t stride,
                               const hf_pi_const_t *pi, const float *dh, const float *const d_o[3],
                               const float *const d_d[3], const float *d_to_world, float *const out_dir[3],
                               float *out_div, hipStream_t stream) {
    if (ra.n == 0) return;
    hf_reparam_tan_kargs k = {};
    hf_reparam_tan_args &a = k.a;
    k.f = f;
    a.n = ra.n; a.stride = stride; a.active = ra.active; a.num_rays = num_rays; a.seed = ra.seed; a.kappa = ra.kappa;
    a.exponent = ra.exponent; a.antithetic = ra.antithetic; a.ray_id = ra.ray_id; a.pi = *pi; a.si_bt = ra.si_bt;
    a.dh = dh; a.dM = d_to_world; a.out_div = out_div;
    bool ray = false;
    for (int c = 0; c < 3; ++c) {
        a.o[c] = ra.o[c]; a.d[c] = ra.d[c]; a.out_dir[c] = out_dir[c];
        a.d_o[c] = d_o ? d_o[c] : nullptr; a.d_d[c] = d_d ? d_d[c] : nullptr;
        ray = ray || a.d_o[c] || a.d_d[c];
    }
    void (*const table[8])(hf_reparam_tan_kargs) = {
        hf_reparam_tangent_kernel<false, false, false>, hf_reparam_tangent_kernel<true, false, false>,
        hf_reparam_tangent_kernel<false, true, false>, hf_reparam_tangent_kernel<true, true, false>,
        hf_reparam_tangent_kernel<false, false, true>, hf_reparam_tangent_kernel<true, false, true>,
        hf_reparam_tangent_kernel<false, true, true>, hf_reparam_tangent_kernel<true, true, true> };
    const int sel = (dh ? 1 : 0) | (ray ? 2 : 0) | (d_to_world ? 4 : 0);
    hipLaunchKernelGGL(table[sel], dim3(grid_for(ra.n)), dim3(HF_BLOCK), 0, stream, k);
}

// ---------------------------------------------------------------------------------
// Reverse mode of the warped-area reparameterisation with respect to everything attached (hf_reparam_backward_full):
// the transpose of hf_reparam_tangent_kernel, term for term, instantiated on the outputs wanted -- DH grad_heights,
// RAY grad_o / grad_d, XF grad_to_world.  Two passes over a ray's samples, as in hf_reparam_backward_kernel (the
// gradient of a sample's V_direct needs Z and dZ of all of them): the weights and their sums, then per sample
//   hit:  (gp, gt) of V_direct = (p - o) / t, gp_tot = gp + gt po / (t |d_aux|^2); vertex c receives b_c gp_tot (DH: its
//         component along height_axis into the scatter tile; XF: times (q_c, 1)^T into the lane's 12 sums); RAY:
//         grad_o -= gp_tot and d_aux receives -gt t d_aux / |d_aux|^2, accumulated against omega into the gradients of
//         Frame3f(d)'s s, t and d (coordinate_system_vjp is linear: applied once, after the samples);
//   miss: V_direct = ray.d, RAY: grad_d += gVd.
// Every sample is drawn in both passes and nothing is kept in between: the registers go to the sums (XF: 12, RAY: 12).
// DH: the per-wave 64 x 64 LDS tile of hf_reparam_backward_kernel, two waves per SIMD.  Without DH there is no tile
// and the launch bound asks for four.  Without RAY a wave whose rays all miss has nothing to add and skips, and so does
// a sample no lane of the wave hit; with RAY the misses carry grad_d and every lane stores its rows (inactive: zeros).
// Whole waves stay in the loop (ballots, the tile's shuffles) and no thread leaves before xform_block_store.
// ---------------------------------------------------------------------------------
struct hf_reparam_bwdf_kargs {
    hf_dev_field f;
    hf_reparam_bwd_args a; // grad_h: NULL without DH
    float *go[3], *gd[3];  // RAY: either array may be absent (NULL rows)
    float *slab;           // XF
};
template <bool DH, bool RAY, bool XF>
__global__ __launch_bounds__(HF_BLOCK, (DH ? 2 : 4)) void hf_reparam_backward_full_kernel(hf_reparam_bwdf_kargs k_) {
    (void) k_;
    typedef const __attribute__((address_space(4))) hf_reparam_bwdf_kargs *kargs_t;
    kargs_t kc = (kargs_t) __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kc));
    const size_t a_n = kc->a.n;
    constexpr int TILE = HF_RB_TILE;
    __shared__ float s_acc[DH ? HF_BLOCK / 64 : 1][DH ? TILE * TILE : 1]; // per-wave accumulation tile
    float *acc = s_acc[DH ? (threadIdx.x >> 6) : 0];
    const int lane = (int) (threadIdx.x & 63u);
    if constexpr (DH)
        for (int k = lane; k < TILE * TILE; k += 64) acc[k] = 0.f;
    float M[12]; // XF: this lane's sums of dL/d(to_world)
#pragma unroll
    for (int j = 0; j < 12; ++j) M[j] = 0.f;
    hf_reparam_args sa = {}; // what the sampling helpers read
    sa.seed = kc->a.seed; sa.kappa = kc->a.kappa; sa.exponent = kc->a.exponent; sa.antithetic = kc->a.antithetic;
    sa.ray_id = kc->a.ray_id;
    const size_t stride = (size_t) gridDim.x * HF_BLOCK;
    const size_t n_round = (a_n + HF_BLOCK - 1) / HF_BLOCK * HF_BLOCK; // whole waves stay in the loop
    for (size_t i_raw = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i_raw < n_round; i_raw += stride) {
        kargs_t ka = (kargs_t) __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka)); // opaque: keeps the loads that follow inside the loop body
        const v3 z3 = mk3(0.f, 0.f, 0.f);
        const bool valid = i_raw < a_n;
        const size_t i = valid ? i_raw : a_n - 1;
        const bool act = valid && (ka->a.active ? (ka->a.active[i] != 0) : true);
        const size_t sst = ka->a.stride;
        const uint32_t K = ka->a.num_rays;
        uint32_t hm = 0u; // samples that hit
        for (uint32_t k = 0; k < K; ++k) hm |= (act && ka->a.pi.t[k * sst + i] != __builtin_inff()) ? (1u << k) : 0u;
        const bool work = act && (RAY || hm != 0u);
        const bool wave_work = __ballot(work) != 0ull;
        if constexpr (!RAY) {
            if (!wave_work) continue; // wave-uniform: nothing reaches the heights or to_world
        }
        v3 gO = z3, gD = z3, gFs = z3, gFt = z3; // RAY: dL/do, dL/dd (direct), dL/ds, dL/dt of Frame3f(d)
        if (wave_work) {
            v3 o = z3, d = z3;
            hf_vd_grad g = { z3, 0.f };
            const hf_dev_field f = load_field(&ka->f);
            if (work) {
                d = mk3(ka->a.d[0][i], ka->a.d[1][i], ka->a.d[2][i]);
                if (hm != 0u) o = mk3(ka->a.o[0][i], ka->a.o[1][i], ka->a.o[2][i]);
                const v3 gdir = mk3(ka->a.g_dir[0][i], ka->a.g_dir[1][i], ka->a.g_dir[2][i]);
                const float gdiv = ka->a.g_div[i];
                // first pass: Z = sum_k w_k, dZ = sum_k d_w_omega_k, in sample order from zero; the boundary test of
                // sample k + 1 is requested before sample k is drawn
                float Zs = 0.f;
                v3 dZ = z3;
                float nbt = (hm & 1u) ? ka->a.si_bt[i] : 1.0f;
                for (uint32_t k = 0; k < K; ++k) {
                    const float B = nbt;
                    if (k + 1 < K) nbt = ((hm >> (k + 1)) & 1u) ? ka->a.si_bt[(k + 1) * sst + i] : 1.0f;
                    sa.k = k;
                    hf_aux_sample q;
                    aux_sample(sa, i, d, q);
                    float w;
                    v3 dw;
                    reparam_weight(sa, q, d, B, w, dw);
                    Zs += w;
                    dZ.x += dw.x; dZ.y += dw.y; dZ.z += dw.z;
                }
                g = vdirect_grad_ray(d, gdir, gdiv, Zs, [&] { return dZ; });
            }
            // second pass (wave-uniform loop): the samples' V_direct.  The records of sample k + 1 are requested before
            // sample k is worked on, and a hit's heights before its sample is drawn, as in hf_reparam_tangent_kernel
            int ar = 0, ac = 0; // tile anchor (wave-uniform), set at the first sample with a hit
            bool anchored = false;
            hf_tile_rows<TILE> rows = 0u;
            const uint32_t hm_any = RAY ? 0u : wave_or(hm);
            const v3 ez = height_axis(f); // dP_k/dh_k
            float nbt = 1.f, nb1 = 0.f, nb2 = 0.f; // the next sample's record (a hit's)
            uint32_t nprim = 0u;
            if (hm & 1u) { nbt = ka->a.si_bt[i]; nb1 = ka->a.pi.prim_uv[0][i]; nb2 = ka->a.pi.prim_uv[1][i]; nprim = ka->a.pi.prim_index[i]; }
            for (uint32_t k = 0; k < K; ++k) {
                const bool hit = ((hm >> k) & 1u) != 0u;
                const float B = hit ? nbt : 1.0f, b1 = nb1, b2 = nb2;
                const uint32_t prim = nprim;
                if (k + 1 < K && ((hm >> (k + 1)) & 1u)) { // (k + 1 < K first: a shift by 32 is not defined)
                    const size_t ik1 = (k + 1) * sst + i;
                    nbt = ka->a.si_bt[ik1]; nb1 = ka->a.pi.prim_uv[0][ik1]; nb2 = ka->a.pi.prim_uv[1][ik1];
                    nprim = ka->a.pi.prim_index[ik1];
                }
                if constexpr (!RAY) {
                    if (((hm_any >> k) & 1u) == 0u) continue; // wave-uniform: a miss adds nothing
                }
                float gh[3] = { 0.f, 0.f, 0.f };
                int vr[3] = { 0, 0, 0 }, vc[3] = { 0, 0, 0 };
                if (RAY ? work : hit) {
                    float hz[3] = { 0.f, 0.f, 0.f };
                    if (hit) { // the three heights: prim_world's loads, used below
                        prim_vertex_ids(f, prim, vr, vc);
#pragma unroll
                        for (int c = 0; c < 3; ++c) hz[c] = f.h[(size_t) vr[c] * f.W + vc[c]];
                    }
                    sa.k = k;
                    hf_aux_sample q;
                    aux_sample(sa, i, d, q);
                    float w;
                    v3 dw;
                    reparam_weight(sa, q, d, B, w, dw);
                    const v3 gVd = vdirect_grad_sample(g, w, dw);
                    if (hit) {
                        const float b0 = 1.f - b1 - b2;
                        v3 P[3], ql[3];
#pragma unroll
                        for (int c = 0; c < 3; ++c) { // prim_world's expressions
                            ql[c] = grid_local(f, vr[c], vc[c], hz[c]);
                            P[c] = xform_point(f.to_world, ql[c]);
                        }
                        const v3 da = frame_to_world(q, d, q.omega); // the auxiliary direction (= hf_reparam_aux_kernel's)
                        // V_direct = (p - o) / t with the FollowShape t = sqrt(|p - o|^2 / |d_aux|^2) of compute_si
                        const auto [po, dda, tt] = follow_t(bary_point(P, b0, b1, b2), o, da);
                        auto [gp, gt] = vdirect_grad_hit(gVd, po, tt);
                        axpy3(gt / (tt * dda), po, gp); // t's dependence on p - o: gp is now the gradient of p - o
                        if constexpr (RAY) {
                            gO = gO - gp;
                            // t's dependence on d_aux = s(d) omega.x + t(d) omega.y + d omega.z, omega detached
                            const v3 gda = da * (-gt * tt / dda);
                            axpy3(q.omega.x, gda, gFs); axpy3(q.omega.y, gda, gFt); axpy3(q.omega.z, gda, gD);
                        }
                        // p = sum b_c P_c with detached barycentrics; P_c = to_world (q_c, 1), dP_c/dh_c = ez
                        const float bc[3] = { b0, b1, b2 };
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const v3 gP = gp * bc[c];
                            if constexpr (DH) gh[c] = dot3(ez, gP);
                            if constexpr (XF) xform_grad_point(M, gP, ql[c]);
                        }
                    } else if constexpr (RAY) {
                        gD = gD + gVd; // miss: V_direct = ray.d (reparam.py:93-95)
                    }
                }
                if constexpr (DH) {
                    const uint64_t hb = __ballot(hit);
                    if (!anchored && hb != 0ull) { // wave-uniform: the first sample with a hit anchors the tile
                        tile_anchor(hb, vr, vc, HF_RB_ANCHOR, ar, ac);
                        anchored = true;
                    }
                    if (hit)
#pragma unroll
                        for (int c = 0; c < 3; ++c) tile_add<TILE>(acc, ar, ac, vr[c], vc[c], gh[c], ka->a.grad_h, f.W, rows);
                }
            }
            if constexpr (DH) tile_flush<TILE>(acc, ar, ac, rows, ka->a.grad_h, f.W, lane);
            if constexpr (RAY) {
                if (work) gD = gD + coordinate_system_vjp(d, gFs, gFt);
            }
        }
        if constexpr (RAY) {
            if (valid) { // inactive lanes: exact zeros
                if (ka->go[0]) { ka->go[0][i] = gO.x; ka->go[1][i] = gO.y; ka->go[2][i] = gO.z; }
                if (ka->gd[0]) { ka->gd[0][i] = gD.x; ka->gd[1][i] = gD.y; ka->gd[2][i] = gD.z; }
            }
        }
    }
    if constexpr (XF) xform_block_store(M, kc->slab); // every thread of the block
}

void hf_launch_reparam_backward_full(const hf_dev_field &f, const hf_reparam_args &ra, uint32_t num_rays, size_t stride,
                                     const hf_pi_const_t *pi, float *grad_h, float *const grad_o[3],
                                     float *const grad_d[3], float *grad_to_world, void *slab, hipStream_t stream) {
    if (ra.n == 0) return;
    hf_reparam_bwdf_kargs k = {};
    hf_reparam_bwd_args &a = k.a;
    k.f = f;
    a.n = ra.n; a.stride = stride; a.active = ra.active; a.num_rays = num_rays; a.seed = ra.seed; a.kappa = ra.kappa;
    a.exponent = ra.exponent; a.antithetic = ra.antithetic; a.ray_id = ra.ray_id; a.pi = *pi; a.si_bt = ra.si_bt;
    a.g_div = ra.g_div; a.grad_h = grad_h;
    for (int c = 0; c < 3; ++c) {
        a.o[c] = ra.o[c]; a.d[c] = ra.d[c]; a.g_dir[c] = ra.g_dir[c];
        k.go[c] = grad_o ? grad_o[c] : nullptr; k.gd[c] = grad_d ? grad_d[c] : nullptr;
    }
    k.slab = (float *) slab;
    void (*const table[8])(hf_reparam_bwdf_kargs) = {
        nullptr, hf_reparam_backward_full_kernel<true, false, false>,
        hf_reparam_backward_full_kernel<false, true, false>, hf_reparam_backward_full_kernel<true, true, false>,
        hf_reparam_backward_full_kernel<false, false, true>, hf_reparam_backward_full_kernel<true, false, true>,
        hf_reparam_backward_full_kernel<false, true, true>, hf_reparam_backward_full_kernel<true, true, true> };
    const int sel = (grad_h ? 1 : 0) | ((grad_o || grad_d) ? 2 : 0) | (grad_to_world ? 4 : 0);
    if (sel == 0) return; // (refused by the caller)
    const int grid = grad_to_world ? grid_for(ra.n, HF_XFORM_GRID_CAP) : grid_for(ra.n);
    hipLaunchKernelGGL(table[sel], dim3(grid), dim3(HF_BLOCK), 0, stream, k);
    if (grad_to_world) xform_sum((const float *) slab, grid, grad_to_world, stream); // slab: hf_xform_slab_bytes(n), this launch's alone
}

// ---------------------------------------------------------------------------------
// Adam step on the height texture (optimizers.py:263-300), explicit operation order (no contraction)
// ---------------------------------------------------------------------------------
// (sched, ctr): hf_adam_step_scheduled -- the step size is sched[*ctr] (a host-filled table of the bias-corrected step
// sizes, so that a captured step can be replayed: the step number is not baked into the launch); else lr_t
__global__ __launch_bounds__(HF_BLOCK) void hf_adam_kernel(size_t n, float *__restrict__ h, const float *__restrict__ g,
                                                          float *__restrict__ m, float *__restrict__ v, float lr_t,
                                                          float beta1, float beta2, float c1, float c2, float eps,
                                                          int mask_updates, const float *__restrict__ sched,
                                                          const uint32_t *__restrict__ ctr) {
    if (sched) lr_t = sched[*ctr];
    const size_t stride = (size_t) gridDim.x * HF_BLOCK;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < n; i += stride) {
        const float gi = g[i];
        if (mask_updates && gi == 0.f) continue;
        const float mt = beta1 * m[i] + c1 * gi;
        const float vt = beta2 * v[i] + c2 * (gi * gi);
        m[i] = mt; v[i] = vt;
        h[i] = h[i] - (lr_t * mt) / (__builtin_sqrtf(vt) + eps);
    }
}

// 'UniformAdam' (optimizers.py:259, 290-291: the update divides by the square root of the MAXIMUM second moment of the
// step instead of the per-element one): pass 1 updates the moments and reduces max(v) into *vmax (float bits as an
// unsigned: v >= 0), pass 2 applies  h -= lr_t m / (sqrt(max v) + eps).
__global__ __launch_bounds__(HF_BLOCK) void hf_adam_moments_kernel(size_t n, const float *__restrict__ g, float *__restrict__ m,
                                                                  float *__restrict__ v, float beta1, float beta2, float c1,
                                                                  float c2, int mask_updates, uint32_t *vmax) {
    const size_t stride = (size_t) gridDim.x * HF_BLOCK;
    float mx = 0.f;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < n; i += stride) {
        const float gi = g[i];
        float vt = v[i];
        if (!(mask_updates && gi == 0.f)) {
            m[i] = beta1 * m[i] + c1 * gi;
            vt = beta2 * vt + c2 * (gi * gi);
            v[i] = vt;
        }
        mx = (vt != vt) ? vt : fmaxf(mx, vt); // dr.max(v_t) runs over every entry, masked ones with their old value (:282-285, 290); a NaN moment is kept (fmaxf would drop it and mask a diverged run)
    }
    // (as unsigned bits: v >= 0, and a NaN -- 0x7fc00000 and up -- is larger than every finite value, so it reaches *vmax)
    const uint32_t wm = wave_max_u32(__builtin_bit_cast(uint32_t, mx) & 0x7FFFFFFFu);
    if ((threadIdx.x & 63u) == 0u && wm > __hip_atomic_load(vmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(vmax, wm);
}
__global__ __launch_bounds__(HF_BLOCK) void hf_adam_apply_uniform_kernel(size_t n, float *__restrict__ h, const float *__restrict__ g,
                                                                        const float *__restrict__ m, float lr_t, float eps,
                                                                        int mask_updates, const uint32_t *vmax,
                                                                        const float *__restrict__ sched, const uint32_t *__restrict__ ctr) {
    if (sched) lr_t = sched[*ctr];
    const float den = __builtin_sqrtf(__builtin_bit_cast(float, *vmax)) + eps;
    const size_t stride = (size_t) gridDim.x * HF_BLOCK;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < n; i += stride) {
        if (mask_updates && g[i] == 0.f) continue;
        h[i] = h[i] - (lr_t * m[i]) / den;
    }
}

__global__ void hf_counter_increment_kernel(uint32_t *ctr) { *ctr += 1u; }

hipError_t hf_launch_adam(size_t n, float *h, const float *g, float *m, float *v, float lr_t, float beta1, float beta2,
                          float c1, float c2, float eps, int mask_updates, hipStream_t stream, uint32_t *uniform_scratch,
                          const float *sched, uint32_t *ctr) {
    if (n == 0) return hipSuccess;
    if (uniform_scratch) {
        const hipError_t e = hipMemsetAsync(uniform_scratch, 0, sizeof(uint32_t), stream);
        if (e != hipSuccess) return e; // (the reduction below would start from a stale maximum)
        hipLaunchKernelGGL(hf_adam_moments_kernel, dim3(grid_for(n)), dim3(HF_BLOCK), 0, stream, n, g, m, v, beta1, beta2, c1, c2,
                           mask_updates, uniform_scratch);
        hipLaunchKernelGGL(hf_adam_apply_uniform_kernel, dim3(grid_for(n)), dim3(HF_BLOCK), 0, stream, n, h, g, m, lr_t, eps,
                           mask_updates, uniform_scratch, sched, (const uint32_t *) ctr);
    } else {
        hipLaunchKernelGGL(hf_adam_kernel, dim3(grid_for(n)), dim3(HF_BLOCK), 0, stream, n, h, g, m, v, lr_t, beta1, beta2,
                           c1, c2, eps, mask_updates, sched, (const uint32_t *) ctr);
    }
    if (sched) hipLaunchKernelGGL(hf_counter_increment_kernel, dim3(1), dim3(1), 0, stream, ctr); // the next replay's step
    return hipSuccess;
}

// ---------------------------------------------------------------------------------
// Minimal direct lighting on the wavefront (include/hf.h): one lane per sample, coalesced SoA loads,
// the box-filter film as a shuffle tree over the samples of a pixel.  Pure streaming: 28 B/sample in.
// ---------------------------------------------------------------------------------
#define HF_DPP_ADD(v, ctrl) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xF, 0xF, false))
struct hf_f3ptr { const float *p[3]; };
struct hf_f3out { float *p[3]; };

// light k seen from p: the unit direction towards it (returned) and ir = 1/|v|.  POINT: L.l[k] is the light's position and
// L.w[k] = albedo/pi * intensity; the direction towards the light and the inverse-square falloff L.w[k] ir^2 are per
// sample (src/emitters/point.cpp: d = pos - it.p, spec = intensity / |d|^2).  (The weight is left to the callers: read
// here, the adjoint's load of it would leave the branch that uses it.)
template <bool POINT>
__device__ __forceinline__ v3 light_dir(const hf_lights_dev &L, uint32_t k, v3 p, float &ir) {
    v3 l = mk3(L.l[k][0], L.l[k][1], L.l[k][2]);
    ir = 1.f;
    if (POINT) {
        const v3 v = l - p;
        ir = 1.0f / __builtin_sqrtf(dot3(v, v));
        l = v * ir;
    }
    return l;
}

// the box-filter film: sample i's value c of light k, averaged over the spp samples of its pixel into image[k * npix + pixel].
// spp a power of two: a butterfly over the g = min(spp, 64) lanes of a pixel (DPP within rows of 16, cross-lane beyond),
// then one store (the wave holds whole pixels) or atomic (several waves per pixel); otherwise one atomic per sample
// (tid: the thread's index in its workgroup, or anything equal to it modulo 64)
__device__ __forceinline__ void film_pixel(float *image, float c, uint32_t k, size_t npix, size_t i, uint32_t spp, bool in,
                                           bool pow2, uint32_t g, float inv_spp, uint32_t tid = threadIdx.x) {
    if (pow2) {
        if (g > 1u) c += HF_DPP_ADD(c, 0xB1);   // quad_perm [1,0,3,2]
        if (g > 2u) c += HF_DPP_ADD(c, 0x4E);   // quad_perm [2,3,0,1]
        if (g > 4u) c += HF_DPP_ADD(c, 0x141);  // row_half_mirror: the other quad pair
        if (g > 8u) c += HF_DPP_ADD(c, 0x140);  // row_mirror: the other half row
        if (g > 16u) c += __shfl_xor(c, 16);
        if (g > 32u) c += __shfl_xor(c, 32);
        if (in && (tid & (g - 1u)) == 0u) {
            if (spp <= 64u) image[k * npix + i / spp] = c * inv_spp;
            else            atomicAdd(&image[k * npix + i / spp], c * inv_spp);
        }
    } else if (in) {
        atomicAdd(&image[k * npix + i / spp], c * inv_spp);
    }
}

// POINT: point lights (light_dir)
template <bool POINT>
__global__ __launch_bounds__(HF_BLOCK) void hf_direct_kernel(size_t n, uint32_t spp, hf_f3ptr sn, hf_f3ptr dd,
                                                            const float *__restrict__ t, hf_f3ptr pp, hf_lights_dev L,
                                                            float *__restrict__ image) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const size_t npix = n / spp;
    const bool in = i < n;
    const size_t ii = in ? i : n - 1;
    const v3 nn = mk3(sn.p[0][ii], sn.p[1][ii], sn.p[2][ii]);
    const v3 d = mk3(dd.p[0][ii], dd.p[1][ii], dd.p[2][ii]);
    const bool lit = in && (t[ii] != __builtin_inff()) && (-dot3(nn, d) > 0.f); // hit, seen from the front (diffuse.cpp:137)
    const bool pow2 = (spp & (spp - 1u)) == 0u;
    const uint32_t g = spp < 64u ? spp : 64u; // lanes per pixel within a wave (tree path)
    const float inv_spp = 1.0f / (float) spp;
    v3 p = mk3(0.f, 0.f, 0.f);
    if (POINT) p = mk3(pp.p[0][ii], pp.p[1][ii], pp.p[2][ii]);
    for (uint32_t k = 0; k < L.n; ++k) {
        float ir;
        const v3 l = light_dir<POINT>(L, k, p, ir);
        const float wk = POINT ? L.w[k] * (ir * ir) : L.w[k];
        const float co = dot3(nn, l);
        float c = (lit && co > 0.f && (L.vis[k] ? L.vis[k][ii] != 0 : true)) ? wk * co : 0.f;
        if (L.weight) c *= L.weight[ii];
        film_pixel(image, c, k, npix, i, spp, in, pow2, g, inv_spp);
    }
}

// POINT: f = w (n.v) |v|^-3 with v = pos - p:  df/dn = w |v|^-2 l,  df/dp = w |v|^-3 (3 (n.l) l - n)
template <bool POINT>
__global__ __launch_bounds__(HF_BLOCK) void hf_direct_adjoint_kernel(size_t n, uint32_t spp, hf_f3ptr sn, hf_f3ptr dd,
                                                                    const float *__restrict__ t, hf_f3ptr pp, hf_lights_dev L,
                                                                    const float *__restrict__ gimg, hf_f3out gn, hf_f3out gp) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const size_t npix = n / spp, pix = i / spp;
    const v3 nn = mk3(sn.p[0][i], sn.p[1][i], sn.p[2][i]);
    const v3 d = mk3(dd.p[0][i], dd.p[1][i], dd.p[2][i]);
    const bool lit = (t[i] != __builtin_inff()) && (-dot3(nn, d) > 0.f);
    const float inv_spp = 1.0f / (float) spp;
    v3 g = mk3(0.f, 0.f, 0.f), gq = mk3(0.f, 0.f, 0.f);
    v3 p = mk3(0.f, 0.f, 0.f);
    if (POINT) p = mk3(pp.p[0][i], pp.p[1][i], pp.p[2][i]);
    const float wgt = L.weight ? L.weight[i] : 1.f;
    float gw = 0.f; // dL/dweight: the unweighted sample values against the image gradient
    for (uint32_t k = 0; k < L.n; ++k) {
        float ir;
        const v3 l = light_dir<POINT>(L, k, p, ir);
        const float co = dot3(nn, l);
        if (lit && co > 0.f && (L.vis[k] ? L.vis[k][i] != 0 : true)) {
            float w = (L.w[k] * inv_spp) * gimg[k * npix + pix];
            if (!POINT) gw = __builtin_fmaf(w, co, gw);
            w *= wgt;
            if (POINT) {
                w = w * (ir * ir);
                const float wp = w * ir, c3 = 3.f * co;
                gq.x = __builtin_fmaf(wp, __builtin_fmaf(c3, l.x, -nn.x), gq.x);
                gq.y = __builtin_fmaf(wp, __builtin_fmaf(c3, l.y, -nn.y), gq.y);
                gq.z = __builtin_fmaf(wp, __builtin_fmaf(c3, l.z, -nn.z), gq.z);
            }
            g.x = __builtin_fmaf(w, l.x, g.x); g.y = __builtin_fmaf(w, l.y, g.y); g.z = __builtin_fmaf(w, l.z, g.z);
        }
    }
    gn.p[0][i] = g.x; gn.p[1][i] = g.y; gn.p[2][i] = g.z;
    if (POINT) { gp.p[0][i] = gq.x; gp.p[1][i] = gq.y; gp.p[2][i] = gq.z; }
    if (!POINT && L.grad_weight) L.grad_weight[i] = gw;
}

// Forward mode of hf_direct_kernel (the transpose of hf_direct_adjoint_kernel): the tangent of every sample's value for
// tangents dsh_n (and dweight: directional lights; dp: point lights), reduced over the samples of a pixel as the primal
// film is.  NULL tangent rows are zero.  Same masks and visibility as the primal (piecewise constant).
//   directional: dc = w_k (wgt <dn, l> + co dweight)
//   point:       dc = wgt w_k |v|^-2 (<dn, l> + |v|^-1 (3 co <l, dp> - <n, dp>)),  v = pos - p
template <bool POINT>
__global__ __launch_bounds__(HF_BLOCK) void hf_direct_tangent_kernel(size_t n, uint32_t spp, hf_f3ptr sn, hf_f3ptr dd,
                                                                    const float *__restrict__ t, hf_f3ptr pp, hf_lights_dev L,
                                                                    hf_f3ptr dsn, hf_f3ptr dpp, const float *__restrict__ dweight,
                                                                    float *__restrict__ dimage) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const size_t npix = n / spp;
    const bool in = i < n;
    const size_t ii = in ? i : n - 1;
    const v3 nn = mk3(sn.p[0][ii], sn.p[1][ii], sn.p[2][ii]);
    const v3 d = mk3(dd.p[0][ii], dd.p[1][ii], dd.p[2][ii]);
    const bool lit = in && (t[ii] != __builtin_inff()) && (-dot3(nn, d) > 0.f);
    const v3 dn = dsn.p[0] ? mk3(dsn.p[0][ii], dsn.p[1][ii], dsn.p[2][ii]) : mk3(0.f, 0.f, 0.f);
    const bool pow2 = (spp & (spp - 1u)) == 0u;
    const uint32_t g = spp < 64u ? spp : 64u;
    const float inv_spp = 1.0f / (float) spp;
    const float wgt = L.weight ? L.weight[ii] : 1.f;
    const float dwgt = (!POINT && dweight) ? dweight[ii] : 0.f;
    v3 p = mk3(0.f, 0.f, 0.f), dq = mk3(0.f, 0.f, 0.f);
    if (POINT) {
        p = mk3(pp.p[0][ii], pp.p[1][ii], pp.p[2][ii]);
        if (dpp.p[0]) dq = mk3(dpp.p[0][ii], dpp.p[1][ii], dpp.p[2][ii]);
    }
    for (uint32_t k = 0; k < L.n; ++k) {
        float ir;
        const v3 l = light_dir<POINT>(L, k, p, ir);
        const float wk = POINT ? L.w[k] * (ir * ir) : L.w[k];
        const float co = dot3(nn, l);
        float c = 0.f;
        if (lit && co > 0.f && (L.vis[k] ? L.vis[k][ii] != 0 : true)) {
            float s = dot3(dn, l);
            if (POINT) s = __builtin_fmaf(ir, __builtin_fmaf(3.f * co, dot3(l, dq), -dot3(nn, dq)), s);
            c = wk * __builtin_fmaf(wgt, s, co * dwgt);
        }
        film_pixel(dimage, c, k, npix, i, spp, in, pow2, g, inv_spp); // (the primal's film)
    }
}

// ---------------------------------------------------------------------------------
// Gaussian reconstruction filter, splatted the way ImageBlock::put does (src/render/imageblock.cpp:258-330 with
// src/rfilters/gaussian.cpp:48-101): a sample at film position pos adds  w_x(px) w_y(py) value  to every pixel
// whose index lies in [ceil(pos - 0.5 - r), floor(pos - 0.5 + r)] (clamped to the film), with the windowed Gaussian
// w(x) = max(0, exp(-x^2 / (2 stddev^2)) - exp(-r^2 / (2 stddev^2))), r = 4 stddev, x = pixel index - (pos - 0.5);
// the accumulated weight goes to its own plane and the film divides by it.
// ---------------------------------------------------------------------------------

template <bool ADJOINT>
__global__ __launch_bounds__(HF_BLOCK) void hf_film_splat_kernel(hf_splat_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const float fx = a.pos_x[i] - 0.5f, fy = a.pos_y[i] - 0.5f;
    const int x0 = max((int) ceilf(fx - a.radius), 0), x1 = min((int) floorf(fx + a.radius), (int) a.width - 1);
    const int y0 = max((int) ceilf(fy - a.radius), 0), y1 = min((int) floorf(fy + a.radius), (int) a.height - 1);
    float acc[HF_MAX_LIGHTS];
    float val[HF_MAX_LIGHTS];
#pragma unroll
    for (uint32_t k = 0; k < HF_MAX_LIGHTS; ++k) {
        acc[k] = 0.f;
        val[k] = (!ADJOINT && k < a.channels) ? a.values[k][i] : 0.f;
    }
    const size_t plane = (size_t) a.width * a.height;
    for (int y = y0; y <= y1; ++y) {
        const float dy = (float) y - fy;
        const float wy = fmaxf(expf(a.alpha * (dy * dy)) - a.bias, 0.f);
        for (int x = x0; x <= x1; ++x) {
            const float dx = (float) x - fx;
            const float w = fmaxf(expf(a.alpha * (dx * dx)) - a.bias, 0.f) * wy;
            if (w == 0.f) continue;
            const size_t pix = (size_t) y * a.width + x;
            if (ADJOINT) {
#pragma unroll
                for (uint32_t k = 0; k < HF_MAX_LIGHTS; ++k)
                    if (k < a.channels) acc[k] = __builtin_fmaf(w, a.grad_image[k * plane + pix], acc[k]);
            } else {
                atomicAdd(a.weight + pix, w);
#pragma unroll
                for (uint32_t k = 0; k < HF_MAX_LIGHTS; ++k)
                    if (k < a.channels) atomicAdd(a.image + k * plane + pix, w * val[k]);
            }
        }
    }
    if (ADJOINT) {
#pragma unroll
        for (uint32_t k = 0; k < HF_MAX_LIGHTS; ++k)
            if (k < a.channels) a.grad_values[k][i] = acc[k];
    }
}

void hf_launch_film_splat(const hf_splat_args &a, bool adjoint, hipStream_t stream) {
    if (a.n == 0) return;
    const dim3 grid((unsigned) ((a.n + HF_BLOCK - 1) / HF_BLOCK)), block(HF_BLOCK);
    if (adjoint) hipLaunchKernelGGL(hf_film_splat_kernel<true>, grid, block, 0, stream, a);
    else         hipLaunchKernelGGL(hf_film_splat_kernel<false>, grid, block, 0, stream, a);
}

// ---------------------------------------------------------------------------------
// The same film for samples that MOVE and carry a weight (hf_film_splat_weighted and its two derivatives): what
// ImageBlock::put(pos, value, weight) does with the position attached (src/render/imageblock.cpp:264-400 evaluates
// the filter analytically on it), in forward mode (src/python/python/ad/integrators/common.py:705-780) and in reverse
// (common.py:868-970).  f = w(x) w(y), x = px - (pos_x - 0.5):  df/dpos_x = -w'(x) w(y), w'(x) = 2 alpha x e^(alpha x^2)
// where w(x) > 0, else 0; w is continuous at the radius, so the clamped footprint has no boundary term.
// One thread per sample; w(y), w'(y) once per row; one exponential gives w and w' of a coordinate.
// ---------------------------------------------------------------------------------

__device__ __forceinline__ void film_weight(float alpha, float bias, float x, float &w, float &dw) {
    const float e = expf(alpha * (x * x));
    w = fmaxf(e - bias, 0.f);
    dw = w > 0.f ? 2.f * alpha * x * e : 0.f;
}

// MODE 0: image += f value, weight += f sample_weight (float atomics)
// MODE 1: the gather of hf.h -- no atomics, every wanted output overwritten
// MODE 2: the transpose of MODE 1, scattered like MODE 0; a contribution that is exactly zero issues no atomic
template <int MODE>
__global__ __launch_bounds__(HF_BLOCK) void hf_film_motion_kernel(hf_film_motion_args m) {
    const hf_splat_args &a = m.s;
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const float fx = a.pos_x[i] - 0.5f, fy = a.pos_y[i] - 0.5f;
    const int x0 = max((int) ceilf(fx - a.radius), 0), x1 = min((int) floorf(fx + a.radius), (int) a.width - 1);
    const int y0 = max((int) ceilf(fy - a.radius), 0), y1 = min((int) floorf(fy + a.radius), (int) a.height - 1);
    const float sw = m.sample_weight ? m.sample_weight[i] : 1.f;
    float val[HF_MAX_LIGHTS];
    float aux[HF_MAX_LIGHTS]; // MODE 1: the sums of grad_values, MODE 2: the tangent values
#pragma unroll
    for (uint32_t k = 0; k < HF_MAX_LIGHTS; ++k) {
        val[k] = (k < a.channels && a.values[k]) ? a.values[k][i] : 0.f;
        aux[k] = (MODE == 2 && k < a.channels && m.dvalues[k]) ? m.dvalues[k][i] : 0.f;
    }
    float dsw = 0.f, dpx = 0.f, dpy = 0.f; // MODE 1: the sums of the three per-sample outputs, MODE 2: the tangents
    if (MODE == 2) {
        if (m.dsample_weight) dsw = m.dsample_weight[i];
        if (m.dpos_x) dpx = m.dpos_x[i];
        if (m.dpos_y) dpy = m.dpos_y[i];
    }
    const size_t plane = (size_t) a.width * a.height;
    for (int y = y0; y <= y1; ++y) {
        float wy, dwy;
        film_weight(a.alpha, a.bias, (float) y - fy, wy, dwy);
        if (wy == 0.f) continue; // (then w'(y) = 0 as well)
        for (int x = x0; x <= x1; ++x) {
            float wx, dwx;
            film_weight(a.alpha, a.bias, (float) x - fx, wx, dwx);
            const float f = wx * wy;
            const size_t pix = (size_t) y * a.width + x;
            if (MODE == 0) {
                if (f == 0.f) continue;
                atomicAdd(a.weight + pix, f * sw);
#pragma unroll
                for (uint32_t k = 0; k < HF_MAX_LIGHTS; ++k)
                    if (k < a.channels) atomicAdd(a.image + k * plane + pix, f * val[k]);
                continue;
            }
            if (wx == 0.f) continue;
            const float fpx = -dwx * wy, fpy = -wx * dwy; // df/dpos_x, df/dpos_y
            if (MODE == 1) {
                const float gw = m.grad_weight ? m.grad_weight[pix] : 0.f;
                float G = sw * gw;
#pragma unroll
                for (uint32_t k = 0; k < HF_MAX_LIGHTS; ++k)
                    if (k < a.channels) {
                        const float g = a.grad_image[k * plane + pix];
                        aux[k] = __builtin_fmaf(f, g, aux[k]);
                        G = __builtin_fmaf(val[k], g, G);
                    }
                dsw = __builtin_fmaf(f, gw, dsw);
                dpx = __builtin_fmaf(fpx, G, dpx);
                dpy = __builtin_fmaf(fpy, G, dpy);
            } else {
                const float df = __builtin_fmaf(fpx, dpx, fpy * dpy);
                const float cw = __builtin_fmaf(f, dsw, df * sw);
                if (cw != 0.f) atomicAdd(a.weight + pix, cw);
#pragma unroll
                for (uint32_t k = 0; k < HF_MAX_LIGHTS; ++k)
                    if (k < a.channels) {
                        const float c = __builtin_fmaf(f, aux[k], df * val[k]);
                        if (c != 0.f) atomicAdd(a.image + k * plane + pix, c);
                    }
            }
        }
    }
    if (MODE == 1) {
#pragma unroll
        for (uint32_t k = 0; k < HF_MAX_LIGHTS; ++k)
            if (k < a.channels && a.grad_values[k]) a.grad_values[k][i] = aux[k];
        if (m.grad_sample_weight) m.grad_sample_weight[i] = dsw;
        if (m.grad_pos_x) m.grad_pos_x[i] = dpx;
        if (m.grad_pos_y) m.grad_pos_y[i] = dpy;
    }
}

void hf_launch_film_motion(int mode, const hf_film_motion_args &a, hipStream_t stream) {
    if (a.s.n == 0) return;
    const dim3 grid((unsigned) ((a.s.n + HF_BLOCK - 1) / HF_BLOCK)), block(HF_BLOCK);
    if (mode == 0)      hipLaunchKernelGGL(hf_film_motion_kernel<0>, grid, block, 0, stream, a);
    else if (mode == 1) hipLaunchKernelGGL(hf_film_motion_kernel<1>, grid, block, 0, stream, a);
    else                hipLaunchKernelGGL(hf_film_motion_kernel<2>, grid, block, 0, stream, a);
}

// ---------------------------------------------------------------------------------
// Lighting rows, shared: what the sky, bounce, envmap, reflect and glossy sections below have in common -- the per-lane
// walk of a shadow or bounce ray, the f64 sine / cosine of their shading sums, the first reads of a derivative or rays
// kernel, the ray stores, the seed and the optional outputs of an adjoint, the tangent shell and the launch.  (The map
// lookup of the last three, env_texels / env_scatter4 / env_gather4, stands beside env_lookup in the envmap section.)
// Only text that is the same for every row belongs here; nothing in this block asks which row calls it (A: the row's
// argument struct, its common fields under their common names).
// ---------------------------------------------------------------------------------
// the masks of hf_direct_kernel: a hit seen from the front (diffuse.cpp:137)
__device__ __forceinline__ bool sky_eligible(float t, v3 sn, v3 d) { return (t != __builtin_inff()) && (-dot3(sn, d) > 0.f); }

// one lane's walk from the root (closest hit, or ANY hit), as an incoherent wave of hf_trace_kernel takes it.  `f`: the
// kernel's by-value argument; what setup_ray needs of it is read from the kernarg segment (`kf`) again.  `maxt`: where
// the ray ends (the overload below: a ray towards the environment, which lies outside the scene)
template <bool ANY>
__device__ __forceinline__ void light_walk(const __attribute__((address_space(4))) hf_dev_field *kf, const hf_dev_field &f, v3 o,
                                           v3 w, float maxt, bool traced, hf_hit &best) {
    best.hit = false; best.t = __builtin_inff(); best.u = 0.f; best.v = 0.f; best.prim = 0u;
    hf_ray_state rs = {}; // fully defined on every path
    bool alive;
    {
        const hf_dev_field f0 = load_field(kf);
        alive = traced && setup_ray(f0, f0.mip[1], o, w, maxt, rs);
    }
    if (alive) {
        float thi = rs.thi;
        hf_src_global src;
        src.mip = f.mip; src.shear = f.shear; src.h = f.h; src.top = f.top; src.W = f.W;
        const uint32_t lfxm = rs.fx ? ((1u << f.top) - 1u) : 0u, lfym = rs.fy ? ((1u << f.top) - 1u) : 0u;
        (void) walk_subtree<ANY>(f, src, rs, rs.r, rs.fx, rs.fy, lfxm, lfym, 0u, 0u, f.top, thi, best);
    }
}
template <bool ANY>
__device__ __forceinline__ void light_walk(const __attribute__((address_space(4))) hf_dev_field *kf, const hf_dev_field &f, v3 o,
                                           v3 w, bool traced, hf_hit &best) {
    light_walk<ANY>(kf, f, o, w, __builtin_inff(), traced, best);
}

// sin a, cos a in double for |a| <= pi / 4: two Taylor sums whose first dropped terms are 7e-12 and 4e-13 (a dozen fmas
// and few registers: the library's sincospi, correct to the last bit of a double, costs the forward kernel 25 spilled
// registers)
struct hf_sincos { double s, c; };
__device__ __forceinline__ hf_sincos light_sincos_f64(double a) {
    const double a2 = a * a;
    double ps = -1.0 / 39916800.0, pc = 1.0 / 479001600.0;
    ps = fma(ps, a2, 1.0 / 362880.0); ps = fma(ps, a2, -1.0 / 5040.0); ps = fma(ps, a2, 1.0 / 120.0);
    ps = fma(ps, a2, -1.0 / 6.0); ps = fma(ps, a2, 1.0); ps *= a;
    pc = fma(pc, a2, -1.0 / 3628800.0); pc = fma(pc, a2, 1.0 / 40320.0); pc = fma(pc, a2, -1.0 / 720.0);
    pc = fma(pc, a2, 1.0 / 24.0); pc = fma(pc, a2, -0.5); pc = fma(pc, a2, 1.0);
    return hf_sincos{ ps, pc };
}
// sin(pi x), cos(pi x) in double for x in [0, 4): the quadrant q = round(2 x) is taken off exactly, |pi t| <= pi / 4 is
// left to light_sincos_f64; no call
__device__ __forceinline__ void env_sincospi_f64(double x, double &sn, double &cs) {
    const double q = rint(2.0 * x), t = x - 0.5 * q;
    const auto [ps, pc] = light_sincos_f64(3.141592653589793 * t);
    const int qi = (int) q & 3;
    sn = qi == 0 ? ps : qi == 1 ? pc : qi == 2 ? -ps : -pc;
    cs = qi == 0 ? pc : qi == 1 ? -ps : qi == 2 ? -pc : ps;
}

// what a derivative or rays kernel reads of sample i first: the shading normal, and whether the sample is shaded at all
// (false: a miss, or seen from behind); light_id: its id in the sample streams
template <class A>
__device__ __forceinline__ bool light_sample(const A &a, size_t i, v3 &sn) {
    sn = mk3(a.sh_n[0][i], a.sh_n[1][i], a.sh_n[2][i]);
    const v3 d = mk3(a.d[0][i], a.d[1][i], a.d[2][i]);
    return sky_eligible(a.t[i], sn, d);
}
template <class A>
__device__ __forceinline__ uint32_t light_id(const A &a, size_t i) { return a.ray_id ? a.ray_id[i] : (uint32_t) i; }
// Interaction::offset_p (interaction.h:161-165) without the direction: (1 + max|p|) RayEpsilon, RayEpsilon = 1500 * 2^-24
__device__ __forceinline__ float sky_offset(v3 p) {
    return (1.f + fmaxf(fmaxf(__builtin_fabsf(p.x), __builtin_fabsf(p.y)), __builtin_fabsf(p.z))) * 8.940696716308594e-05f;
}
// origin of spawn_ray(w) (interaction.h:134-136): p moved along the geometric normal to the side w points to
__device__ __forceinline__ v3 sky_origin(v3 p, v3 gn, float mag, v3 w) {
    return fma3(gn, dot3(gn, w) < 0.f ? -mag : mag, p);
}
// a materialised ray; maxt = -1: the fused kernel does not trace it (`maxt`: where a traced ray ends, for the row whose
// rays end inside the scene)
template <class A>
__device__ __forceinline__ void light_store_ray(const A &a, size_t i, v3 o, v3 d, bool traced, float maxt = __builtin_inff()) {
    a.out_o[0][i] = o.x; a.out_o[1][i] = o.y; a.out_o[2][i] = o.z;
    a.out_d[0][i] = d.x; a.out_d[1][i] = d.y; a.out_d[2][i] = d.z;
    a.out_maxt[i] = traced ? maxt : -1.f;
}
// the same for a row whose untraced lanes get a zero origin and direction: spawn_ray(w) where the fused kernel walks it
template <class A>
__device__ __forceinline__ void light_store_spawned(const A &a, size_t i, v3 p, v3 gn, v3 w, bool traced) {
    const v3 z = mk3(0.f, 0.f, 0.f);
    light_store_ray(a, i, traced ? sky_origin(p, gn, sky_offset(p), w) : z, traced ? w : z, traced);
}
// what the adjoint of a row with an image and a per-sample value starts from: dL/dvalue of sample i (NULL: zero)
template <class A>
__device__ __forceinline__ float light_value_seed(const A &a, size_t i) {
    return (a.gimg ? a.gimg[i / a.spp] * (1.0f / (float) a.spp) : 0.f) + (a.gvalue ? a.gvalue[i] : 0.f);
}
// an adjoint's output of three optional rows, and the gradients of sh_n and weight of such a row (NULL: not wanted)
__device__ __forceinline__ void light_store3(float *const r[3], size_t i, v3 g) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (r[c]) r[c][i] = c == 0 ? g.x : c == 1 ? g.y : g.z;
}
template <class A>
__device__ __forceinline__ void light_store_grads(const A &a, size_t i, v3 gn, float gw) {
    light_store3(a.gn, i, gn);
    if (a.gw) a.gw[i] = gw;
}
// ... and of p, for the rows whose value or landing depends on it
template <class A>
__device__ __forceinline__ void light_store_grads(const A &a, size_t i, v3 gn, v3 gp, float gw) {
    light_store_grads(a, i, gn, gw);
    light_store3(a.gp, i, gp);
}

// The tangent image of a row with one channel, VALUE(a, i) the tangent of sample i's value.  PIXEL = false: one lane per
// sample and the primal's film (spp a power of two <= 64: its shuffle tree, one store per pixel; or no image wanted);
// PIXEL = true (any other spp): one lane per pixel adds its samples in order -- no atomics either way.  `value`: the
// per-sample tangents, for the rows that have them (NULL: not wanted; the literal nullptr of the rows that have none
// compiles the stores away); such a row's `image` may be NULL too
template <bool PIXEL, class A, float (*VALUE)(const A &, size_t)>
__device__ __forceinline__ void light_tangent_image(const A &a, float *value) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const uint32_t spp = a.spp;
    if (PIXEL) {
        if (i >= a.n / spp) return;
        float c = 0.f;
        for (uint32_t s = 0; s < spp; ++s) {
            const float dv = VALUE(a, i * spp + s);
            if (value) value[i * spp + s] = dv;
            c += dv;
        }
        a.image[i] = c * (1.0f / (float) spp);
    } else {
        const bool in = i < a.n;
        const float c = VALUE(a, in ? i : a.n - 1);
        if (in && value) value[i] = c;
        if (a.image) film_pixel(a.image, in ? c : 0.f, 0u, a.n / spp, i, spp, in, true, spp, 1.0f / (float) spp);
    }
}

// film_pixel reduces the samples of a pixel in a shuffle tree and stores once; any other spp takes its atomic paths,
// which want a zeroed image
static bool sky_tree_film(uint32_t spp) { return (spp & (spp - 1u)) == 0u && spp <= 64u; }

// modes 0 to 3 of a row: forward (`channels` film planes), adjoint, tangent, rays.  A NULL image (the rows with a
// per-sample value): no film to clear, and the tangent with one lane per sample
template <class A>
static void launch_light(int mode, const A &a, uint32_t channels, hipStream_t stream, void (*forward)(A), void (*adjoint)(A),
                         void (*tangent)(A), void (*tangent_pixel)(A), void (*rays)(A)) {
    if (a.n == 0) return;
    const bool tree = sky_tree_film(a.spp) || !a.image;
    const dim3 grid((unsigned) ((a.n + HF_BLOCK - 1) / HF_BLOCK)), block(HF_BLOCK);
    if (mode == 0 && !tree) (void) hipMemsetAsync(a.image, 0, sizeof(float) * (a.n / a.spp) * channels, stream);
    if (mode == 2 && !tree)
        hipLaunchKernelGGL(tangent_pixel, dim3((unsigned) ((a.n / a.spp + HF_BLOCK - 1) / HF_BLOCK)), block, 0, stream, a);
    else
        hipLaunchKernelGGL(mode == 0 ? forward : mode == 1 ? adjoint : mode == 2 ? tangent : rays, grid, block, 0, stream, a);
}

// the rows of a [3, n] argument; NULL: three NULL rows
static hf_f3ptr f3ptr(const float *const r[3]) { return r ? hf_f3ptr{ { r[0], r[1], r[2] } } : hf_f3ptr{}; }
static hf_f3out f3out(float *const r[3]) { return r ? hf_f3out{ { r[0], r[1], r[2] } } : hf_f3out{}; }

void hf_launch_direct(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3], const float *t,
                      const float *const p[3], const hf_lights_dev &lights, float *image, hipStream_t stream) {
    if (n == 0) return;
    if (!sky_tree_film(spp)) (void) hipMemsetAsync(image, 0, sizeof(float) * lights.n * (n / spp), stream); // atomic paths
    const dim3 grid((unsigned) ((n + HF_BLOCK - 1) / HF_BLOCK)), block(HF_BLOCK);
    hipLaunchKernelGGL(p ? hf_direct_kernel<true> : hf_direct_kernel<false>, grid, block, 0, stream, n, spp, f3ptr(sh_n),
                       f3ptr(d), t, f3ptr(p), lights, image);
}

void hf_launch_direct_adjoint(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                              const float *t, const float *const p[3], const hf_lights_dev &lights,
                              const float *grad_image, float *const grad_sh_n[3], float *const grad_p[3],
                              hipStream_t stream) {
    if (n == 0) return;
    const dim3 grid((unsigned) ((n + HF_BLOCK - 1) / HF_BLOCK)), block(HF_BLOCK);
    hipLaunchKernelGGL(p ? hf_direct_adjoint_kernel<true> : hf_direct_adjoint_kernel<false>, grid, block, 0, stream, n, spp,
                       f3ptr(sh_n), f3ptr(d), t, f3ptr(p), lights, grad_image, f3out(grad_sh_n), f3out(p ? grad_p : nullptr));
}

void hf_launch_direct_tangent(size_t n, uint32_t spp, const float *const sh_n[3], const float *const d[3],
                              const float *t, const float *const p[3], const hf_lights_dev &lights,
                              const float *const dsh_n[3], const float *const dp[3], const float *dweight, float *dimage,
                              hipStream_t stream) {
    if (n == 0) return;
    if (!sky_tree_film(spp)) (void) hipMemsetAsync(dimage, 0, sizeof(float) * lights.n * (n / spp), stream); // atomic paths
    const dim3 grid((unsigned) ((n + HF_BLOCK - 1) / HF_BLOCK)), block(HF_BLOCK);
    hipLaunchKernelGGL(p ? hf_direct_tangent_kernel<true> : hf_direct_tangent_kernel<false>, grid, block, 0, stream, n, spp,
                       f3ptr(sh_n), f3ptr(d), t, f3ptr(p), lights, f3ptr(dsh_n), f3ptr(dp), dweight, dimage);
}

// ---------------------------------------------------------------------------------
// Sky lighting (include/hf.h hf_sky_*): diffuse surface under a constant environment, the K = num_rays emitter
// samples of every wavefront sample drawn, traced (any hit, per lane) and reduced in ONE launch.  One lane per sample,
// `k` a scalar loop with the lanes predicated; nothing of a shadow ray goes to memory: per sample 56 B in (p, n, sh_n,
// d, t, + weight, ray_id) and one visibility word + the film contribution out.
// ---------------------------------------------------------------------------------
// direction k of the sample with stream id `id`: square_to_uniform_sphere (warp.h:250-255) of the TEA sample
// (the stream of aux_sample with pair = k)
__device__ __forceinline__ void sky_sample(uint32_t seed, uint32_t k, uint32_t id, float &sx, float &sy) {
    uint32_t key, unused, r0, r1;
    tea32(seed, k, key, unused);
    tea32(key, id, r0, r1);
    sx = (float) (r0 >> 9) * (1.0f / 8388608.0f); sy = (float) (r1 >> 9) * (1.0f / 8388608.0f);
}
__device__ __forceinline__ v3 sky_dir(uint32_t seed, uint32_t k, uint32_t id) {
    float sx, sy;
    sky_sample(seed, k, id, sx, sy);
    const float z = __builtin_fmaf(-2.f, sy, 1.f);
    const float r = __builtin_sqrtf(fmaxf(__builtin_fmaf(-z, z, 1.f), 0.f));
    float sn, cs;
    sincospif(2.f * sx, &sn, &cs);
    return mk3(r * cs, r * sn, z);
}

// The same direction in double, for the SHADING sums (the cosines of the forward, the sums of directions of the
// derivative kernels): a float direction is 1e-7 off, which is the whole error of a grazing cosine and of a gradient
// component that is small because the horizontal components of a hemisphere of unit vectors cancel; drawn and added
// in double and rounded once, what is left is the rounding of the result.  The RAYS use the float direction.
struct hf_d3 { double x, y, z; };
__device__ __forceinline__ hf_d3 sky_dir_f64(uint32_t seed, uint32_t k, uint32_t id) {
    float sx, sy;
    sky_sample(seed, k, id, sx, sy);
    const double z = 1.0 - 2.0 * (double) sy;
    const double r = sqrt(fmax(1.0 - z * z, 0.0));
    // env_sincospi_f64(2 sx), with the quadrant selected by value here: called through its references the selects are
    // compiled differently, and hf_sky_kernel grows by five instructions (by value there, hf_envmap_kernel changes)
    const double x = 2.0 * (double) sx, q = rint(2.0 * x), t = x - 0.5 * q;
    const auto [ps, pc] = light_sincos_f64(3.141592653589793 * t);
    const int qi = (int) q & 3;
    const double sn = qi == 0 ? ps : qi == 1 ? pc : qi == 2 ? -ps : -pc;
    const double cs = qi == 0 ? pc : qi == 1 ? -ps : qi == 2 ? -pc : ps;
    return hf_d3{ r * cs, r * sn, z };
}
__device__ __forceinline__ double sky_dot_f64(v3 a, hf_d3 w) { return (double) a.x * w.x + (double) a.y * w.y + (double) a.z * w.z; }

typedef const __attribute__((address_space(4))) hf_sky_args *hf_sky_kargs;

#ifndef HF_SKY_WAVES
#define HF_SKY_WAVES 6 // resident waves per SIMD (the lean any-hit instantiation's)
#endif
__global__ __launch_bounds__(HF_BLOCK, HF_SKY_WAVES) void hf_sky_kernel(hf_sky_args a) {
    const hf_dev_field &f = a.f;
    // n < 2^32 (hf_sky_lighting): the sample index is ONE register across the walk, and everything else about the
    // sample's place (the clamped index, its lane) is derived from it again where it is needed
    const size_t i64 = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const bool in = i64 < a.n;
    const uint32_t i = (uint32_t) i64;
    const uint32_t ii = in ? i : (uint32_t) (a.n - 1);
    const v3 sn = mk3(a.sh_n[0][ii], a.sh_n[1][ii], a.sh_n[2][ii]);
    bool elig;
    {
        const v3 d = mk3(a.d[0][ii], a.d[1][ii], a.d[2][ii]);
        elig = in && sky_eligible(a.t[ii], sn, d);
    }
    float acc = 0.f;    // sum over the visible directions of <sh_n, w_k> (sky_dir_f64), in k order
    uint32_t bits = 0u; // bit k: direction k was traced and is unoccluded
    if (__ballot(elig) != 0ull) { // wave-uniform: a batch without an eligible sample (the part of an image beside the terrain) draws nothing
        const v3 p = mk3(a.p[0][ii], a.p[1][ii], a.p[2][ii]);
        const v3 gn = mk3(a.nrm[0][ii], a.nrm[1][ii], a.nrm[2][ii]);
        const uint32_t id = a.ray_id ? a.ray_id[ii] : ii;
        const float mag = sky_offset(p);
        // (launch constants of the loop are read from the kernarg segment where they are used, as in hf_trace_kernel)
        hf_sky_kargs ka = (hf_sky_kargs) __builtin_amdgcn_kernarg_segment_ptr();
#pragma unroll 1
        for (uint32_t k = 0;; ++k) { // wave-uniform loop, the lanes predicated inside
            asm volatile("" : "+s"(ka)); // opaque per direction: the kernarg loads stay inside the loop
            // the cosine that is added (sky_dir_f64) first, and finished before the ray is begun (the id goes through
            // the same opaque statement): its doubles are dead when setup_ray's registers fill, one float is held across the walk
            v3 snd = sn; // (opaque: the conversions of sh_n to double are otherwise hoisted out of the loop, six registers held across the walk)
            asm volatile("" : "+v"(snd.x), "+v"(snd.y), "+v"(snd.z));
            float co = (float) sky_dot_f64(snd, sky_dir_f64(ka->seed, k, id));
            uint32_t idr = id;
            asm volatile("" : "+v"(co), "+v"(idr));
            const v3 w = sky_dir(ka->seed, k, idr);
            const bool traced = elig && dot3(sn, w) > 0.f;
            hf_hit best;
            light_walk<true>(&ka->f, f, sky_origin(p, gn, mag, w), w, traced, best);
            if (traced && !best.hit) { bits |= 1u << k; acc += co; }
            if (k + 1u >= ka->num_rays) break;
        }
    }
    // (the output pointers: loaded here, not before the walk)
    hf_sky_kargs ko = (hf_sky_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ko));
    float c = 0.f;
    if (elig) { // (eligible: in range)
        const float *weight = ko->weight;
        c = ko->scale * acc;
        if (weight) c *= weight[i];
    }
    uint32_t *vis_bits = ko->vis_bits;
    if (in && vis_bits) vis_bits[i] = bits;
    const uint32_t spp = ko->spp, g = spp < 64u ? spp : 64u;
    film_pixel(ko->image, c, 0u, ko->n / spp, i, spp, in, (spp & (spp - 1u)) == 0u, g, 1.0f / (float) spp, i);
}

// shadow ray a.k of every sample, materialised: what hf_sky_kernel traces for that direction, bit for bit
__global__ __launch_bounds__(HF_BLOCK) void hf_sky_rays_kernel(hf_sky_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    v3 sn;
    const bool elig = light_sample(a, i, sn);
    const v3 p = mk3(a.p[0][i], a.p[1][i], a.p[2][i]), gn = mk3(a.nrm[0][i], a.nrm[1][i], a.nrm[2][i]);
    const v3 w = sky_dir(a.seed, a.k, light_id(a, i));
    light_store_ray(a, i, sky_origin(p, gn, sky_offset(p), w), w, elig && dot3(sn, w) > 0.f);
}

// Reverse mode of hf_sky_kernel with respect to sh_n and weight: nothing is traced, the directions are drawn again and
// the visibility word read.  Sums in k order, no atomics.
__global__ __launch_bounds__(HF_BLOCK) void hf_sky_adjoint_kernel(hf_sky_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    v3 sn, g = mk3(0.f, 0.f, 0.f);
    float gw = 0.f;
    if (light_sample(a, i, sn)) {
        const uint32_t bits = a.vis_bits[i], id = light_id(a, i);
        double sx = 0.0, sy = 0.0, sz = 0.0, sc = 0.0;
        for (uint32_t k = 0; k < a.num_rays; ++k) {
            if ((bits >> k) & 1u) {
                const hf_d3 w = sky_dir_f64(a.seed, k, id);
                sx += w.x; sy += w.y; sz += w.z;
                sc += sky_dot_f64(sn, w);
            }
        }
        const float c = (a.gimg[i / a.spp] * (1.0f / (float) a.spp)) * a.scale;
        g = mk3((float) sx, (float) sy, (float) sz) * (a.weight ? c * a.weight[i] : c);
        gw = c * (float) sc;
    }
    a.gn[0][i] = g.x; a.gn[1][i] = g.y; a.gn[2][i] = g.z;
    if (a.gw) a.gw[i] = gw;
}

// forward mode: the tangent of sample i's value for tangents dn of sh_n and dw of weight (NULL: zero)
__device__ __forceinline__ float sky_tangent_value(const hf_sky_args &a, size_t i) {
    v3 sn;
    if (!light_sample(a, i, sn)) return 0.f;
    const uint32_t bits = a.vis_bits[i], id = light_id(a, i);
    const v3 dn = a.dn[0] ? mk3(a.dn[0][i], a.dn[1][i], a.dn[2][i]) : mk3(0.f, 0.f, 0.f);
    double sd = 0.0, sc = 0.0;
    for (uint32_t k = 0; k < a.num_rays; ++k) {
        if ((bits >> k) & 1u) {
            const hf_d3 w = sky_dir_f64(a.seed, k, id);
            sd += sky_dot_f64(dn, w);
            sc += sky_dot_f64(sn, w);
        }
    }
    return (float) ((double) a.scale * ((double) (a.weight ? a.weight[i] : 1.f) * sd + (double) (a.dw ? a.dw[i] : 0.f) * sc));
}
template <bool PIXEL>
__global__ __launch_bounds__(HF_BLOCK) void hf_sky_tangent_kernel(hf_sky_args a) {
    light_tangent_image<PIXEL, hf_sky_args, sky_tangent_value>(a, nullptr);
}

void hf_launch_sky(int mode, const hf_sky_args &a, hipStream_t stream) {
    launch_light(mode, a, 1u, stream, hf_sky_kernel, hf_sky_adjoint_kernel, hf_sky_tangent_kernel<false>,
                 hf_sky_tangent_kernel<true>, hf_sky_rays_kernel);
}

// ---------------------------------------------------------------------------------
// Refractive caustics (include/hf.h hf_caustic_*): light tracing through the surface.  Every wavefront sample is a
// light sample that arrives along d; it is refracted at the shading normal (the `dielectric` BSDF's transmission lobe
// in importance mode, dielectric.cpp:361: no eta^2), the refracted ray is walked (any hit, per lane, maxt = the
// distance to the receiver plane) and what gets through lands on the receiver.  ONE launch, one lane per sample;
// nothing of the ray goes to memory: per sample 56 B in (+ weight, active) and pos, value, one visibility byte out.
// ---------------------------------------------------------------------------------
// The specular vertex of one sample, the same text for the fused kernel, the rays kernel and the two derivatives.
// fresnel() (fresnel.h:35-71) and refract() (fresnel.h:311-314) operation for operation: the fmas below are the
// reference's fnmadd / fmadd / fmsub and nothing else fuses (the build contracts nothing).
//   dF, dq: d F / d c_i and d (c_i eta_ti + c_t) / d c_i with the side (the sign of c_i) held; only the derivative
//   kernels use them (one more division there)
struct hf_caustic_vertex {
    bool traced;                  // eligible, transmitted, consistent and on its way to the receiver
    v3 wi, wo;
    float s, b, F, q, dF, dq;     // s: distance to the receiver, b = <wo, N>, q = c_i eta_ti + c_t
    float e2;                     // eta_ti^2: the radiance-mode factor of the refraction view (the caustics carry importance)
};
template <class P>
__device__ __forceinline__ hf_caustic_vertex caustic_vertex(P a, v3 m, v3 g, v3 d, v3 p, float t, bool act) {
    hf_caustic_vertex v;
    v.wi = mk3(-d.x, -d.y, -d.z);
    const float ci = dot3(m, v.wi), gi = dot3(g, v.wi);
    bool ok = act && (__builtin_fabsf(t) < __builtin_inff()) && (ci != 0.f) && (gi * ci > 0.f);
    const float eta = a->eta, rcp_eta = a->rcp_eta;
    const bool outside = ci >= 0.f;
    const float eta_it = outside ? eta : rcp_eta, eta_ti = outside ? rcp_eta : eta;
    const float e2 = eta_ti * eta_ti;
    v.e2 = e2;
    const float ct2 = __builtin_fmaf(-__builtin_fmaf(-ci, ci, 1.f), e2, 1.f);
    ok = ok && (ct2 > 0.f); // total internal reflection: nothing is transmitted
    const float cia = __builtin_fabsf(ci), cta = __builtin_sqrtf(fmaxf(ct2, 0.f));
    const float ns = __builtin_fmaf(-eta_it, cta, cia), ds = __builtin_fmaf(eta_it, cta, cia);
    const float np = __builtin_fmaf(-eta_it, cia, cta), dp = __builtin_fmaf(eta_it, cia, cta);
    const float a_s = ns / ds, a_p = np / dp;
    const bool matched = eta == 1.f; // (the other special case, c_i = 0, is not eligible)
    v.F = matched ? 0.f : 0.5f * (a_s * a_s + a_p * a_p);
    const float ct = outside ? -cta : cta; // mulsign_neg(cos_theta_t_abs, cos_theta_i)
    v.q = __builtin_fmaf(ci, eta_ti, ct);
    v.wo = mk3(__builtin_fmaf(m.x, v.q, -(v.wi.x * eta_ti)), __builtin_fmaf(m.y, v.q, -(v.wi.y * eta_ti)),
               __builtin_fmaf(m.z, v.q, -(v.wi.z * eta_ti)));
    ok = ok && (dot3(g, v.wo) * gi < 0.f); // leaves on the other side of the true surface
    const v3 N = mk3(a->N[0], a->N[1], a->N[2]), org = mk3(a->origin[0], a->origin[1], a->origin[2]);
    v.b = dot3(v.wo, N);
    v.s = dot3(org - p, N) / v.b;
    v.traced = ok && (__builtin_fabsf(v.s) < __builtin_inff()) && (v.s > 0.f);
    // the derivatives with respect to c_i, the side held: d cta = c_i eta_ti^2 / cta
    const float sg = outside ? 1.f : -1.f, dcta = ci * e2 / cta;
    const float das = 2.f * ((eta_it * cta) * sg - cia * (eta_it * dcta)) / (ds * ds);
    const float dap = 2.f * ((eta_it * cia) * dcta - cta * (eta_it * sg)) / (dp * dp);
    v.dF = matched ? 0.f : a_s * das + a_p * dap;
    v.dq = eta_ti - sg * dcta;
    return v;
}
// where a deposited sample lands: film coordinates of p + s wo
template <class P>
__device__ __forceinline__ void caustic_landing(P a, v3 p, const hf_caustic_vertex &v, float &x, float &y) {
    const v3 r = fma3(v.wo, v.s, p) - mk3(a->origin[0], a->origin[1], a->origin[2]);
    x = dot3(r, mk3(a->ex[0], a->ex[1], a->ex[2]));
    y = dot3(r, mk3(a->ey[0], a->ey[1], a->ey[2]));
}
// The derivatives of the landing, for the rows that land on the receiver (A: hf_caustic_args or hf_refract_args).
// Forward mode: tangents dm of sh_n and dp of p, dci = <dm, wi>; d wo, d s (`ds`) and d pos = (dx, dy)
template <class A>
__device__ __forceinline__ void caustic_landing_tangent(const A &a, const hf_caustic_vertex &v, v3 m, v3 dm, v3 dp, float dci,
                                                        float &dx, float &dy, float &ds) {
    const v3 N = mk3(a.N[0], a.N[1], a.N[2]);
    const v3 dwo = fma3(m, v.dq * dci, dm * v.q);
    ds = -(dot3(dp, N) + v.s * dot3(dwo, N)) / v.b;
    const v3 dX = fma3(v.wo, ds, fma3(dwo, v.s, dp));
    dx = dot3(dX, mk3(a.ex[0], a.ex[1], a.ex[2]));
    dy = dot3(dX, mk3(a.ey[0], a.ey[1], a.ey[2]));
}
// Reverse mode, its transpose: (gx, gy) = dL/dpos, gs = dL/ds (DS: the row's value depends on s), gc = dL/dc_i through
// the value; gm, gp: the gradients of sh_n and p
template <bool DS, class A>
__device__ __forceinline__ void caustic_landing_adjoint(const A &a, const hf_caustic_vertex &v, v3 m, float gx, float gy, float gs,
                                                        float gc, v3 &gm, v3 &gp) {
    const v3 N = mk3(a.N[0], a.N[1], a.N[2]);
    const v3 gX = fma3(mk3(a.ex[0], a.ex[1], a.ex[2]), gx, mk3(a.ey[0], a.ey[1], a.ey[2]) * gy);
    const float gl = dot3(gX, v.wo);
    const float c = -(DS ? gl + gs : gl) / v.b;   // dL/ds over -b
    gp = fma3(N, c, gX);
    const v3 gwo = fma3(N, c * v.s, gX * v.s);
    const float gci = __builtin_fmaf(v.dq, dot3(m, gwo), gc);
    gm = fma3(v.wi, gci, gwo * v.q);
}
// the vertex of sample i from the rows
template <class P>
__device__ __forceinline__ hf_caustic_vertex caustic_sample(P a, size_t i, bool in, v3 &m, v3 &p) {
    m = mk3(a->sh_n[0][i], a->sh_n[1][i], a->sh_n[2][i]);
    p = mk3(a->p[0][i], a->p[1][i], a->p[2][i]);
    const v3 g = mk3(a->nrm[0][i], a->nrm[1][i], a->nrm[2][i]), d = mk3(a->d[0][i], a->d[1][i], a->d[2][i]);
    const uint8_t *active = a->active;
    return caustic_vertex(a, m, g, d, p, a->t[i], in && (active ? active[i] != 0 : true));
}

typedef const __attribute__((address_space(4))) hf_caustic_args *hf_caustic_kargs;

__global__ __launch_bounds__(HF_BLOCK, HF_SKY_WAVES) void hf_caustic_kernel(hf_caustic_args a) {
    const hf_dev_field &f = a.f;
    // hf_sky_kernel's mapping: n < 2^32, the sample index is one register across the walk
    const size_t i64 = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const bool in = i64 < a.n;
    const uint32_t i = (uint32_t) i64;
    const uint32_t ii = in ? i : (uint32_t) (a.n - 1);
    // (launch constants are read from the kernarg segment where they are used, as in hf_sky_kernel)
    hf_caustic_kargs ka = (hf_caustic_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    float x = -16.f, y = -16.f, val = 0.f; // what a sample that deposits nothing writes
    bool traced;
    hf_hit best;
    best.hit = false;
    {
        v3 m, p;
        const hf_caustic_vertex v = caustic_sample(ka, ii, in, m, p);
        traced = v.traced;
        if (__ballot(traced) != 0ull) { // wave-uniform: a batch without a traced sample walks nothing
            const v3 gn = mk3(ka->nrm[0][ii], ka->nrm[1][ii], ka->nrm[2][ii]);
            if (traced) {
                caustic_landing(ka, p, v, x, y);
                val = ka->power * (1.f - v.F);
            }
            // three floats and the index are held across the walk; the ray ends at the receiver
            light_walk<true>(&ka->f, f, sky_origin(p, gn, sky_offset(p), v.wo), v.wo, v.s, traced, best);
        }
    }
    // (the output pointers: loaded here, not before the walk)
    hf_caustic_kargs ko = (hf_caustic_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ko));
    if (!in) return;
    const bool lit = traced && !best.hit;
    const float *weight = ko->weight;
    if (lit && weight) val *= weight[i];
    ko->pos[0][i] = lit ? x : -16.f;
    ko->pos[1][i] = lit ? y : -16.f;
    ko->value[i] = lit ? val : 0.f;
    uint8_t *vis = ko->vis;
    if (vis) vis[i] = lit ? 1 : 0;
}

// the refracted ray of every sample, materialised: what hf_caustic_kernel walks, bit for bit (maxt = -1 and a zero
// origin and direction: the fused kernel does not trace the lane)
__global__ __launch_bounds__(HF_BLOCK) void hf_caustic_rays_kernel(hf_caustic_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    v3 m, p;
    const hf_caustic_vertex v = caustic_sample(&a, i, true, m, p);
    const v3 gn = mk3(a.nrm[0][i], a.nrm[1][i], a.nrm[2][i]);
    const v3 z = mk3(0.f, 0.f, 0.f);
    const v3 o = v.traced ? sky_origin(p, gn, sky_offset(p), v.wo) : z, w = v.traced ? v.wo : z;
    a.out_o[0][i] = o.x; a.out_o[1][i] = o.y; a.out_o[2][i] = o.z;
    a.out_d[0][i] = w.x; a.out_d[1][i] = w.y; a.out_d[2][i] = w.z;
    a.out_maxt[i] = v.traced ? v.s : -1.f;
}

// Reverse mode of hf_caustic_kernel with respect to sh_n, p and weight: nothing is traced, the vertex is formed again
// and the visibility byte read.  One lane per sample, every wanted output overwritten, no atomics.
__global__ __launch_bounds__(HF_BLOCK) void hf_caustic_adjoint_kernel(hf_caustic_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    v3 gm = mk3(0.f, 0.f, 0.f), gp = gm;
    float gw = 0.f;
    if (a.vis[i]) {
        v3 m, p;
        const hf_caustic_vertex v = caustic_sample(&a, i, true, m, p);
        if (v.traced) {
            const float gx = a.gpos[0] ? a.gpos[0][i] : 0.f, gy = a.gpos[1] ? a.gpos[1][i] : 0.f;
            const float gv = a.gvalue ? a.gvalue[i] : 0.f;
            const float pw = a.power * (a.weight ? a.weight[i] : 1.f);
            caustic_landing_adjoint<false>(a, v, m, gx, gy, 0.f, -(pw * v.dF) * gv, gm, gp);
            gw = a.power * (1.f - v.F) * gv;
        }
    }
    light_store_grads(a, i, gm, gp, gw);
}

// forward mode, the transpose of the above: tangents dn of sh_n, dp of p, dw of weight (NULL: zero)
__global__ __launch_bounds__(HF_BLOCK) void hf_caustic_tangent_kernel(hf_caustic_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    float dx = 0.f, dy = 0.f, dv = 0.f;
    if (a.vis[i]) {
        v3 m, p;
        const hf_caustic_vertex v = caustic_sample(&a, i, true, m, p);
        if (v.traced) {
            const v3 dm = a.dn[0] ? mk3(a.dn[0][i], a.dn[1][i], a.dn[2][i]) : mk3(0.f, 0.f, 0.f);
            const v3 dp = a.dp[0] ? mk3(a.dp[0][i], a.dp[1][i], a.dp[2][i]) : mk3(0.f, 0.f, 0.f);
            const float dw = a.dw ? a.dw[i] : 0.f;
            const float dci = dot3(dm, v.wi);
            float ds;
            caustic_landing_tangent(a, v, m, dm, dp, dci, dx, dy, ds);
            const float pw = a.power * (a.weight ? a.weight[i] : 1.f);
            dv = __builtin_fmaf(dw, a.power * (1.f - v.F), -(pw * v.dF) * dci);
        }
    }
    if (a.pos[0]) a.pos[0][i] = dx;
    if (a.pos[1]) a.pos[1][i] = dy;
    if (a.value) a.value[i] = dv;
}

void hf_launch_caustic(int mode, const hf_caustic_args &a, hipStream_t stream) {
    if (a.n == 0) return;
    const dim3 grid((unsigned) ((a.n + HF_BLOCK - 1) / HF_BLOCK)), block(HF_BLOCK);
    hipLaunchKernelGGL(mode == 0 ? hf_caustic_kernel : mode == 1 ? hf_caustic_adjoint_kernel : mode == 2 ? hf_caustic_tangent_kernel
                                                                                                          : hf_caustic_rays_kernel,
                       grid, block, 0, stream, a);
}

// ---------------------------------------------------------------------------------
// Bounce lighting (include/hf.h hf_bounce_*): one diffuse interreflection.  Every wavefront sample draws K = num_rays
// cosine-weighted directions (detached BSDF sample, prb.py:162-226; diffuse.cpp:101-143), traces each to its closest
// hit, shades that second vertex under the directional lights with shadow rays of its own and reduces into the film:
// ONE launch, one lane per sample, `k` and the light index scalar loops with the lanes predicated.  Per direction one
// primitive index and one byte of visibility go to memory and nothing else of the rays, hits or interactions.
// ---------------------------------------------------------------------------------
// square_to_cosine_hemisphere (warp.h:54-90, 320-328) of direction k's sample, local frame.  phi / pi = rp / (4 r) is at
// most 1/4 in magnitude; the other quadrant pair (phi -> pi/2 - phi) swaps sine and cosine.  z = safe_sqrt(1 - |p|^2)
// is taken as sqrt((1 - |r|) (1 + |r|)): |p| = |r| for the concentric map, r = 2 s - 1 is exact, and the difference
// 1 - px^2 - py^2 of rounded products would lose z to cancellation near the rim of the disk (2.7e-6 at z = 0.01).
// (bounce_disk: square_to_uniform_disk_concentric of that sample as (px, py, |r|); the glossy row draws on the same disk)
__device__ __forceinline__ v3 bounce_disk(uint32_t seed, uint32_t k, uint32_t id) {
    float sx, sy;
    sky_sample(seed, k, id, sx, sy);
    const float x = __builtin_fmaf(2.f, sx, -1.f), y = __builtin_fmaf(2.f, sy, -1.f);
    const bool q13 = __builtin_fabsf(x) < __builtin_fabsf(y);
    const float r = q13 ? y : x, rp = q13 ? x : y;
    const float a = (x == 0.f && y == 0.f) ? 0.f : 0.25f * rp / r;
    float sn, cs;
    sincospif(a, &sn, &cs);
    const float px = r * (q13 ? sn : cs), py = r * (q13 ? cs : sn);
    return mk3(px, py, __builtin_fabsf(r));
}
__device__ __forceinline__ v3 bounce_local(uint32_t seed, uint32_t k, uint32_t id) {
    const v3 q = bounce_disk(seed, k, id);
    const float ar = q.z;
    return mk3(q.x, q.y, __builtin_sqrtf((1.f - ar) * (1.f + ar)));
}
// Frame3f(sh_n).to_world with (s, t) = coordinate_system(sh_n)
__device__ __forceinline__ v3 bounce_world(v3 sn, v3 wo) {
    v3 s, t;
    coordinate_system(sn, s, t);
    return fma3(sn, wo.z, fma3(t, wo.y, s * wo.x));
}
// The same direction in double for the SHADING sums of the derivative kernels (w_k / z_k: 1 - |p|^2 cancels near the rim
// of the disk; see sky_dir_f64).  Returns the world direction, z = the local wo.z.  The RAYS use the float direction.
__device__ __forceinline__ hf_d3 bounce_dir_f64(v3 sn, uint32_t seed, uint32_t k, uint32_t id, double &z) {
    float sx, sy;
    sky_sample(seed, k, id, sx, sy);
    const double x = 2.0 * (double) sx - 1.0, y = 2.0 * (double) sy - 1.0;
    const bool q13 = fabs(x) < fabs(y);
    const double r = q13 ? y : x, rp = q13 ? x : y;
    const auto [ps, pc] = light_sincos_f64((x == 0.0 && y == 0.0) ? 0.0 : 0.7853981633974483 * rp / r); // (|a| <= pi / 4)
    const double px = r * (q13 ? ps : pc), py = r * (q13 ? pc : ps);
    z = sqrt((1.0 - fabs(r)) * (1.0 + fabs(r))); // (as bounce_local)
    // coordinate_system (vector.h:116-136) in double
    const double nx = sn.x, ny = sn.y, nz = sn.z, sg = nz >= 0.0 ? 1.0 : -1.0;
    const double ca = -1.0 / (sg + nz), cb = nx * ny * ca;
    const hf_d3 s = { sg * (nx * nx * ca) + 1.0, sg * cb, -sg * nx }, t = { cb, ny * ny * ca + sg, -ny };
    return hf_d3{ s.x * px + t.x * py + nx * z, s.y * px + t.y * py + ny * z, s.z * px + t.z * py + nz * z };
}

typedef const __attribute__((address_space(4))) hf_bounce_args *hf_bounce_kargs;

// the second vertex: p and the face normal of compute_si_to for the hit (prim, b1, b2), its arithmetic
__device__ __forceinline__ void bounce_vertex(const hf_dev_field &f, uint32_t prim, float b1, float b2, v3 &q, v3 &nq) {
    v3 P[3];
    float U[3], V[3];
    int vi[3], vj[3];
    prim_world(f, prim, P, U, V, vi, vj);
    q = bary_point(P, 1.f - b1 - b2, b1, b2);
    nq = unit_normal(P[1] - P[0], P[2] - P[0]).n;
    if (f.flip) nq = neg3(nq);
}

#ifndef HF_BOUNCE_WAVES
#define HF_BOUNCE_WAVES 6 // resident waves per SIMD: chosen by an A/B against 4 and 5 (profiles/bounce_lighting/)
#endif
__global__ __launch_bounds__(HF_BLOCK, HF_BOUNCE_WAVES) void hf_bounce_kernel(hf_bounce_args a) {
    // the per-light sums of a sample, in k order: a lane reads and writes its own column only (no barrier)
    __shared__ float s_acc[HF_MAX_LIGHTS][HF_BLOCK];
    const hf_dev_field &f = a.f;
    // n < 2^32 (hf_bounce_lighting): the sample index is ONE register across the walks
    const size_t i64 = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const bool in = i64 < a.n;
    const uint32_t i = (uint32_t) i64;
    const uint32_t ii = in ? i : (uint32_t) (a.n - 1);
    const v3 sn = mk3(a.sh_n[0][ii], a.sh_n[1][ii], a.sh_n[2][ii]);
    bool elig;
    {
        const v3 d = mk3(a.d[0][ii], a.d[1][ii], a.d[2][ii]);
        elig = in && sky_eligible(a.t[ii], sn, d);
    }
    for (uint32_t l = 0; l < a.n_lights; ++l) s_acc[l][threadIdx.x] = 0.f;
    const bool any = __ballot(elig) != 0ull; // wave-uniform: a batch without an eligible sample draws and traces nothing
    v3 p = mk3(0.f, 0.f, 0.f), gn = p;
    uint32_t id = 0u;
    if (any) {
        p = mk3(a.p[0][ii], a.p[1][ii], a.p[2][ii]);
        gn = mk3(a.nrm[0][ii], a.nrm[1][ii], a.nrm[2][ii]);
        id = a.ray_id ? a.ray_id[ii] : ii;
    }
    // (launch constants of the loops are read from the kernarg segment where they are used, as in hf_sky_kernel)
    hf_bounce_kargs ka = (hf_bounce_kargs) __builtin_amdgcn_kernarg_segment_ptr();
#pragma unroll 1
    for (uint32_t k = 0;; ++k) { // wave-uniform loop, the lanes predicated inside
        asm volatile("" : "+s"(ka)); // opaque per direction: the kernarg loads stay inside the loop
        uint32_t prim_out = 0xFFFFFFFFu, bits = 0u;
        if (any) {
            const v3 wo = bounce_local(ka->seed, k, id);
            const v3 w = bounce_world(sn, wo);
            bool hit;
            hf_hit best;
            {
                const bool traced = elig && wo.z > 0.f;
                light_walk<false>(&ka->f, f, sky_origin(p, gn, sky_offset(p), w), w, traced, best);
                hit = traced && best.hit;
            }
            if (__ballot(hit) != 0ull) { // (wave-uniform)
                v3 q, nq;
                {
                    const hf_dev_field fl = load_field(&ka->f); // to_world etc.: not held across the walk
                    bounce_vertex(fl, hit ? best.prim : 0u, hit ? best.u : 0.f, hit ? best.v : 0.f, q, nq);
                }
                if (hit) prim_out = best.prim;
                const bool front = hit && (-dot3(nq, w) > 0.f);
                if (__ballot(front) != 0ull) {
#pragma unroll 1
                    for (uint32_t l = 0;; ++l) { // the directional lights at q: kernarg scalars, never held in vector registers
                        asm volatile("" : "+s"(ka));
                        const v3 ll = mk3(ka->l[l][0], ka->l[l][1], ka->l[l][2]);
                        const bool ts = front && dot3(nq, ll) > 0.f;
                        hf_hit sh;
                        light_walk<true>(&ka->f, f, sky_origin(q, nq, sky_offset(q), ll), ll, ts, sh);
                        if (ts && !sh.hit) {
                            bits |= 1u << l;
                            // the cosine from the float normal in double, rounded once (the float dot3 decides the mask only)
                            const float co = (float) ((double) nq.x * (double) ll.x + (double) nq.y * (double) ll.y + (double) nq.z * (double) ll.z);
                            s_acc[l][threadIdx.x] += ka->w[l] * co;
                        }
                        if (l + 1u >= ka->n_lights) break;
                    }
                }
            }
        }
        {
            uint32_t *hit_prim = ka->hit_prim;
            uint8_t *lit_bits = ka->lit_bits;
            const size_t at = (size_t) k * ka->sample_stride + i;
            if (in && hit_prim) hit_prim[at] = prim_out;
            if (in && lit_bits) lit_bits[at] = (uint8_t) bits;
        }
        if (k + 1u >= ka->num_rays) break;
    }
    // (the output pointers: loaded here, not before the walks)
    hf_bounce_kargs ko = (hf_bounce_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ko));
    float cw = 0.f;
    if (elig) { // (eligible: in range)
        const float *weight = ko->weight;
        cw = ko->scale;
        if (weight) cw *= weight[i];
    }
    const uint32_t spp = ko->spp, g = spp < 64u ? spp : 64u, nl = ko->n_lights;
    const size_t npix = ko->n / spp;
    const bool pow2 = (spp & (spp - 1u)) == 0u;
    for (uint32_t l = 0; l < nl; ++l)
        film_pixel(ko->image, cw * s_acc[l][threadIdx.x], l, npix, i, spp, in, pow2, g, 1.0f / (float) spp, i);
}

// Ray a.k of every sample, materialised: the bounce ray (a.shadow == 0), or the shadow ray from that bounce ray's hit
// towards a.l[0] (the bounce ray is then traced here, per lane): what hf_bounce_kernel traces, bit for bit
__global__ __launch_bounds__(HF_BLOCK) void hf_bounce_rays_kernel(hf_bounce_args a) {
    const size_t i64 = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const bool in = i64 < a.n;
    const size_t i = in ? i64 : a.n - 1;
    v3 sn;
    const bool elig = light_sample(a, i, sn);
    const v3 p = mk3(a.p[0][i], a.p[1][i], a.p[2][i]), gn = mk3(a.nrm[0][i], a.nrm[1][i], a.nrm[2][i]);
    const v3 wo = bounce_local(a.seed, a.k, light_id(a, i));
    const v3 w = bounce_world(sn, wo);
    bool traced = in && elig && wo.z > 0.f;
    v3 o = sky_origin(p, gn, sky_offset(p), w), dir = w;
    if (a.shadow) {
        hf_bounce_kargs ka = (hf_bounce_kargs) __builtin_amdgcn_kernarg_segment_ptr();
        hf_hit best;
        light_walk<false>(&ka->f, a.f, o, w, traced, best);
        const bool hit = traced && best.hit;
        v3 q, nq;
        bounce_vertex(a.f, hit ? best.prim : 0u, hit ? best.u : 0.f, hit ? best.v : 0.f, q, nq);
        dir = mk3(a.l[0][0], a.l[0][1], a.l[0][2]);
        traced = hit && (-dot3(nq, w) > 0.f) && dot3(nq, dir) > 0.f;
        o = hit ? sky_origin(q, nq, sky_offset(q), dir) : mk3(0.f, 0.f, 0.f);
    }
    if (in) light_store_ray(a, i, o, dir, traced);
}

// What the derivative kernels read of one record: the triangle of hit_prim (edges, unit normal before flip_normals and
// 1 / |N|, vertex texels), from the heights as they are now.  false: a miss, or an index that names no triangle
struct hf_bounce_tri { v3 e0, e1, n; float r; int vi[3], vj[3]; };
__device__ __forceinline__ bool bounce_record(const hf_bounce_args &a, size_t at, hf_bounce_tri &tr, uint32_t &bits) {
    const uint32_t prim = a.hit_prim[at];
    bits = a.lit_bits[at];
    if (bits == 0u || prim >= 2u * (uint32_t) (a.f.W - 1) * (uint32_t) (a.f.H - 1)) return false;
    v3 P[3];
    float U[3], V[3];
    prim_world(a.f, prim, P, U, V, tr.vi, tr.vj);
    tr.e0 = P[1] - P[0]; tr.e1 = P[2] - P[0];
    const auto [n, r] = unit_normal(tr.e0, tr.e1);
    tr.n = n; tr.r = r;
    return true;
}
// The tangent of the unit normal of triangle `tr` (before flip_normals) for the height tangent dh, in double from the
// OBJECT-space edges.  The world vertices are float32: an edge P_k - P_0 is off by an ulp of |P|, 3e-6 of a cell at 40
// cells per unit, and dnormalize amplifies that by |dN| r / |dn| -- in float the tangent image misses the bound the
// dsh_n and dweight tangents keep (1.2 to 1.6 times it under a general to_world).  In object space the edges of a grid
// triangle are differences of (j gx, i gy, h s), exact in double, and to_world's linear part maps them to world once.
__device__ __forceinline__ hf_d3 bounce_dnq_f64(const hf_dev_field &f, const hf_bounce_tri &tr, const float *dh) {
    const double gx = 2.0 / (double) (f.W - 1), gy = 2.0 / (double) (f.H - 1), s = f.s;
    const double ez[3] = { f.to_world[2], f.to_world[6], f.to_world[10] }; // the height axis (height_axis / s)
    const size_t i0 = (size_t) tr.vi[0] * f.W + tr.vj[0];
    const double h0 = f.h[i0], d0 = dh[i0];
    double e[2][3], de[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const size_t idx = (size_t) tr.vi[k + 1] * f.W + tr.vj[k + 1];
        const double qx = (double) (tr.vj[k + 1] - tr.vj[0]) * gx, qy = (double) (tr.vi[k + 1] - tr.vi[0]) * gy;
        const double qz = ((double) f.h[idx] - h0) * s;
#pragma unroll
        for (int c = 0; c < 3; ++c) e[k][c] = (double) f.to_world[4 * c] * qx + (double) f.to_world[4 * c + 1] * qy + ez[c] * qz;
        de[k] = ((double) dh[idx] - d0) * s; // the edge's tangent is de[k] ez
    }
    const double N[3] = { e[0][1] * e[1][2] - e[0][2] * e[1][1], e[0][2] * e[1][0] - e[0][0] * e[1][2], e[0][0] * e[1][1] - e[0][1] * e[1][0] };
    // dN = cross(de1 ez, e2) + cross(e1, de2 ez) = cross(ez, de1 e2 - de2 e1)
    const double m[3] = { de[0] * e[1][0] - de[1] * e[0][0], de[0] * e[1][1] - de[1] * e[0][1], de[0] * e[1][2] - de[1] * e[0][2] };
    const double dN[3] = { ez[1] * m[2] - ez[2] * m[1], ez[2] * m[0] - ez[0] * m[2], ez[0] * m[1] - ez[1] * m[0] };
    const double r2 = 1.0 / (N[0] * N[0] + N[1] * N[1] + N[2] * N[2]), r = sqrt(r2);
    const double pj = (N[0] * dN[0] + N[1] * dN[1] + N[2] * dN[2]) * r2; // <n, dN> / |N|
    return hf_d3{ (dN[0] - N[0] * pj) * r, (dN[1] - N[1] * pj) * r, (dN[2] - N[2] * pj) * r };
}

// Reverse mode of hf_bounce_kernel with respect to sh_n, weight and the heights: nothing is traced, the directions are
// drawn again and the record read.  Sums in k order; float atomics on grad_heights only.
__global__ __launch_bounds__(HF_BLOCK) void hf_bounce_adjoint_kernel(hf_bounce_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    v3 sn;
    double sx = 0.0, sy = 0.0, sz = 0.0, sg = 0.0;
    const float wgt = a.weight ? a.weight[i] : 1.f;
    if (light_sample(a, i, sn)) {
        const uint32_t id = light_id(a, i);
        const size_t npix = a.n / a.spp, pix = i / a.spp;
        const float inv_spp = 1.0f / (float) a.spp;
        const v3 ez = height_axis(a.f);
        for (uint32_t k = 0; k < a.num_rays; ++k) {
            hf_bounce_tri tr;
            uint32_t bits;
            if (!bounce_record(a, (size_t) k * a.sample_stride + i, tr, bits)) continue;
            const v3 nq = a.f.flip ? neg3(tr.n) : tr.n;
            double G = 0.0, nx = 0.0, ny = 0.0, nz = 0.0; // G_ik and the gradient of n_q (before weight_i c)
#pragma unroll 1
            for (uint32_t l = 0; l < a.n_lights; ++l) { // (scalar loop: the lights are kernarg scalars, the image gradient an L1 hit)
                if (!((bits >> l) & 1u)) continue;
                const double lx = a.l[l][0], ly = a.l[l][1], lz = a.l[l][2];
                const double g = (a.gimg[l * npix + pix] * inv_spp) * a.w[l]; // g_l albedo/pi E_l
                G += g * ((double) nq.x * lx + (double) nq.y * ly + (double) nq.z * lz);
                nx += g * lx; ny += g * ly; nz += g * lz;
            }
            double z;
            const hf_d3 w = bounce_dir_f64(sn, a.seed, k, id, z);
            const double s = z > 0.0 ? G / z : 0.0; // the attached cosine over the detached one (prb.py:213-223)
            sx += s * w.x; sy += s * w.y; sz += s * w.z; sg += G;
            if (a.gh) {
                const float c = wgt * a.scale;
                v3 gN = mk3(c * (float) nx, c * (float) ny, c * (float) nz);
                if (a.f.flip) gN = neg3(gN);
                float g1, g2;
                face_normal_vjp(tr.e0, tr.e1, dnormalize(tr.n, tr.r, gN), ez, g1, g2);
                atomicAdd(a.gh + (size_t) tr.vi[0] * a.f.W + tr.vj[0], -(g1 + g2));
                atomicAdd(a.gh + (size_t) tr.vi[1] * a.f.W + tr.vj[1], g1);
                atomicAdd(a.gh + (size_t) tr.vi[2] * a.f.W + tr.vj[2], g2);
            }
        }
    }
    if (a.gn[0]) {
        const double c = (double) wgt * (double) a.scale;
        a.gn[0][i] = (float) (c * sx); a.gn[1][i] = (float) (c * sy); a.gn[2][i] = (float) (c * sz);
    }
    if (a.gw) a.gw[i] = (float) ((double) a.scale * sg);
}

// forward mode: the tangents of sample i's values under every light, for tangents dn of sh_n, dw of weight and dh of
// the heights (NULL: zero), ADDED to the lane's column acc[l * HF_BLOCK] (LDS: the light index stays a scalar loop)
__device__ __forceinline__ void bounce_tangent_values(const hf_bounce_args &a, size_t i, double *acc) {
    v3 sn;
    if (!light_sample(a, i, sn)) return;
    const uint32_t id = light_id(a, i);
    const v3 dn = a.dn[0] ? mk3(a.dn[0][i], a.dn[1][i], a.dn[2][i]) : mk3(0.f, 0.f, 0.f);
    const double wgt = a.weight ? a.weight[i] : 1.f, dw = a.dw ? a.dw[i] : 0.f;
    for (uint32_t k = 0; k < a.num_rays; ++k) {
        hf_bounce_tri tr;
        uint32_t bits;
        if (!bounce_record(a, (size_t) k * a.sample_stride + i, tr, bits)) continue;
        const v3 nq = a.f.flip ? neg3(tr.n) : tr.n;
        hf_d3 dnq = { 0.0, 0.0, 0.0 };
        if (a.dh) {
            dnq = bounce_dnq_f64(a.f, tr, a.dh);
            if (a.f.flip) dnq = hf_d3{ -dnq.x, -dnq.y, -dnq.z };
        }
        double z;
        const hf_d3 w = bounce_dir_f64(sn, a.seed, k, id, z);
        const double s = z > 0.0 ? sky_dot_f64(dn, w) / z : 0.0;
        const double f1 = wgt * s + dw; // what multiplies R_ikl
#pragma unroll 1
        for (uint32_t l = 0; l < a.n_lights; ++l) {
            if (!((bits >> l) & 1u)) continue;
            const double lx = a.l[l][0], ly = a.l[l][1], lz = a.l[l][2];
            const double co = (double) nq.x * lx + (double) nq.y * ly + (double) nq.z * lz;
            const double dco = dnq.x * lx + dnq.y * ly + dnq.z * lz;
            acc[l * HF_BLOCK] += (double) a.w[l] * (co * f1 + wgt * dco);
        }
    }
}
// PIXEL = false: one lane per sample and the primal's film (spp a power of two <= 64: its shuffle tree, one store per
// pixel and light); PIXEL = true (any other spp): one lane per pixel adds its samples in order -- no atomics either way
template <bool PIXEL>
__global__ __launch_bounds__(HF_BLOCK) void hf_bounce_tangent_kernel(hf_bounce_args a) {
    __shared__ double s_acc[HF_MAX_LIGHTS][HF_BLOCK]; // a lane reads and writes its own column only (no barrier)
    __shared__ float s_pix[PIXEL ? HF_MAX_LIGHTS : 1][HF_BLOCK];
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const uint32_t spp = a.spp;
    const size_t npix = a.n / spp;
    double *acc = &s_acc[0][threadIdx.x];
    if (PIXEL) {
        if (i >= npix) return;
        for (uint32_t l = 0; l < a.n_lights; ++l) s_pix[l][threadIdx.x] = 0.f;
        for (uint32_t s = 0; s < spp; ++s) {
            for (uint32_t l = 0; l < a.n_lights; ++l) acc[l * HF_BLOCK] = 0.0;
            bounce_tangent_values(a, i * spp + s, acc);
            for (uint32_t l = 0; l < a.n_lights; ++l) s_pix[l][threadIdx.x] += (float) ((double) a.scale * acc[l * HF_BLOCK]);
        }
        for (uint32_t l = 0; l < a.n_lights; ++l) a.image[l * npix + i] = s_pix[l][threadIdx.x] * (1.0f / (float) spp);
    } else {
        const bool in = i < a.n;
        for (uint32_t l = 0; l < a.n_lights; ++l) acc[l * HF_BLOCK] = 0.0;
        if (in) bounce_tangent_values(a, i, acc);
        for (uint32_t l = 0; l < a.n_lights; ++l)
            film_pixel(a.image, (float) ((double) a.scale * acc[l * HF_BLOCK]), l, npix, i, spp, in, true, spp, 1.0f / (float) spp);
    }
}

void hf_launch_bounce(int mode, const hf_bounce_args &a, hipStream_t stream) {
    launch_light(mode, a, a.n_lights, stream, hf_bounce_kernel, hf_bounce_adjoint_kernel, hf_bounce_tangent_kernel<false>,
                 hf_bounce_tangent_kernel<true>, hf_bounce_rays_kernel);
}

// ---- warped-area reparameterisation: per-sample kernels (helpers: above hf_adjoint_kernel) ----
__global__ __launch_bounds__(HF_BLOCK) void hf_reparam_aux_kernel(hf_reparam_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const v3 d = mk3(a.d[0][i], a.d[1][i], a.d[2][i]);
    hf_aux_sample q;
    aux_sample(a, i, d, q);
    const v3 ad = frame_to_world(q, d, q.omega);
    a.aux_d[0][i] = ad.x; a.aux_d[1][i] = ad.y; a.aux_d[2][i] = ad.z;
    a.aux_maxt[i] = (a.active && a.active[i] == 0) ? -1.f : __builtin_inff();
}

__global__ __launch_bounds__(HF_BLOCK) void hf_reparam_weight_kernel(hf_reparam_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const bool act = !(a.active && a.active[i] == 0);
    const v3 o = mk3(a.o[0][i], a.o[1][i], a.o[2][i]), d = mk3(a.d[0][i], a.d[1][i], a.d[2][i]);
    hf_aux_sample q;
    aux_sample(a, i, d, q);
    const float t = a.si_t[i];
    const bool hit = act && (t != __builtin_inff());
    const float B = hit ? a.si_bt[i] : 1.0f;
    float w;
    v3 dw;
    reparam_weight(a, q, d, B, w, dw);
    if (a.mode == 0) {
        if (!act) return;
        a.Z[i] += w;
        a.dZ[0][i] += dw.x; a.dZ[1][i] += dw.y; a.dZ[2][i] += dw.z;
        return;
    }
    v3 gp = mk3(0.f, 0.f, 0.f), gvd = mk3(0.f, 0.f, 0.f);
    float gt = 0.f;
    if (act) {
        const float Zs = a.Z[i];
        const v3 gd = mk3(a.g_dir[0][i], a.g_dir[1][i], a.g_dir[2][i]);
        const float gdiv = a.g_div[i];
        const hf_vd_grad g = vdirect_grad_ray(d, gd, gdiv, Zs, [&] { return mk3(a.dZ[0][i], a.dZ[1][i], a.dZ[2][i]); });
        const v3 gVd = vdirect_grad_sample(g, w, dw);
        gvd = gVd;
        if (hit) { // V_direct = (p - o) / t
            const hf_vd_hit h = vdirect_grad_hit(gVd, mk3(a.si_p[0][i] - o.x, a.si_p[1][i] - o.y, a.si_p[2][i] - o.z), t);
            gp = h.gp;
            gt = h.gt;
        }
    }
    a.g_p[0][i] = gp.x; a.g_p[1][i] = gp.y; a.g_p[2][i] = gp.z;
    a.g_t[i] = gt;
    if (a.g_vd[0]) { a.g_vd[0][i] = gvd.x; a.g_vd[1][i] = gvd.y; a.g_vd[2][i] = gvd.z; }
}

void hf_launch_reparam_aux(const hf_reparam_args &a, hipStream_t stream) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(hf_reparam_aux_kernel, dim3((unsigned) ((a.n + HF_BLOCK - 1) / HF_BLOCK)), dim3(HF_BLOCK), 0, stream, a);
}
void hf_launch_reparam_weights(const hf_reparam_args &a, hipStream_t stream) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(hf_reparam_weight_kernel, dim3((unsigned) ((a.n + HF_BLOCK - 1) / HF_BLOCK)), dim3(HF_BLOCK), 0, stream, a);
}

// ---------------------------------------------------------------------------------
// Area sampling (hf_set_area_sampling, hf_sample_position): the area distribution of Mesh::build_pmf over the triangles
// in prim_index order (mesh.cpp:401-432, distr_1d.h:212-240) and Mesh::sample_position (mesh.cpp:557-610).
//
// Table build: reduce -> scan of the tile totals -> scan of the tiles, three launches and no inter-workgroup waits.  A
// tile is one cell row, or a HF_AREA_CHUNK-cell piece of one; both passes over the tiles compute the areas from the
// heights (coalesced loads, cell c0 + lane + 256 k) into LDS, and every thread then owns 16 consecutive entries.  The
// fp64 sums follow ONE fixed association, nested four deep:
//     cdf[i] = (float) (G + (l + (c + r)))
// r: the running sum over the thread's entries up to i; c: the running sum of the thread totals before it in the tile;
// l: the running sum of the tile totals before it in its group (the tiles of one thread of the tile-total scan); G: the
// running sum of the group totals before it.  Each level is a sequential chain whose last partial sum is the total the
// next level adds, so the fp64 prefixes are non-decreasing across every boundary, the fp32 CDF is sorted, and its last
// entry is the total bit for bit.  Bitwise the same from build to build.
// ---------------------------------------------------------------------------------
#define HF_AREA_PER (2 * HF_AREA_CHUNK / HF_BLOCK) // entries per thread of a tile
struct hf_area_args {
    hf_dev_field f;
    hf_area_table t;
};

// the tile's areas into s_area[0 .. 2 HF_AREA_CHUNK) (zeros past the end of the row); returns the number of cells
__device__ __forceinline__ int area_tile_load(const hf_dev_field &f, uint32_t ncx, float *s_area, int &cy, int &c0) {
    const uint32_t tile = blockIdx.x;
    cy = (int) (tile / ncx);
    c0 = (int) (tile - (uint32_t) cy * ncx) * HF_AREA_CHUNK;
    const int ncell = min(HF_AREA_CHUNK, f.W - 1 - c0);
    for (int c = (int) threadIdx.x; c < HF_AREA_CHUNK; c += HF_BLOCK) {
        float a0 = 0.f, a1 = 0.f;
        if (c < ncell) {
            const int cx = c0 + c;
            const size_t r0 = (size_t) cy * f.W + cx, r1 = r0 + f.W;
            const float h00 = f.h[r0], h10 = f.h[r0 + 1], h01 = f.h[r1], h11 = f.h[r1 + 1];
            const v3 v00 = grid_world(f, cy, cx, h00), v10 = grid_world(f, cy, cx + 1, h10);
            const v3 v01 = grid_world(f, cy + 1, cx, h01), v11 = grid_world(f, cy + 1, cx + 1, h11);
            a0 = tri_area(v00, v10, v01); // tri 0 = (v00, v10, v01)
            a1 = tri_area(v11, v01, v10); // tri 1 = (v11, v01, v10)
        }
        reinterpret_cast<float2 *>(s_area)[c] = make_float2(a0, a1);
    }
    return ncell;
}
// thread t's entries s_area[16 t .. 16 t + 16): their running fp64 sum
__device__ __forceinline__ double area_thread_sum(const float *s_area) {
    double r = 0.0;
#pragma unroll
    for (int j = 0; j < HF_AREA_PER; ++j) r += (double) s_area[threadIdx.x * HF_AREA_PER + j];
    return r;
}
// s[u] <- the running sum of s[0 .. u) (one thread, sequential); returns the total
__device__ __forceinline__ double area_chain(double *s, int count) {
    double acc = 0.0;
    for (int u = 0; u < count; ++u) {
        const double v = s[u];
        s[u] = acc;
        acc += v;
    }
    return acc;
}

// pass 1: per tile, the total and the first / last + 1 entry with a non-zero area
__global__ __launch_bounds__(HF_BLOCK) void hf_area_reduce_kernel(hf_area_args a) {
    __shared__ float s_area[2 * HF_AREA_CHUNK];
    __shared__ double s_sum[HF_BLOCK];
    __shared__ uint32_t s_valid[2];
    if (threadIdx.x == 0) { s_valid[0] = 0xFFFFFFFFu; s_valid[1] = 0u; }
    int cy, c0;
    area_tile_load(a.f, a.t.ncx, s_area, cy, c0);
    __syncthreads();
    const uint32_t base = 2u * ((uint32_t) cy * (uint32_t) (a.f.W - 1) + (uint32_t) c0) + threadIdx.x * HF_AREA_PER;
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
#pragma unroll
    for (int j = 0; j < HF_AREA_PER; ++j)
        if (s_area[threadIdx.x * HF_AREA_PER + j] > 0.f) { lo = min(lo, base + j); hi = base + j + 1u; }
    s_sum[threadIdx.x] = area_thread_sum(s_area);
    if (hi != 0u) { atomicMin(&s_valid[0], lo); atomicMax(&s_valid[1], hi); }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.t.tile[blockIdx.x] = area_chain(s_sum, HF_BLOCK);
        a.t.tile_valid[2 * blockIdx.x] = s_valid[0];
        a.t.tile_valid[2 * blockIdx.x + 1] = s_valid[1];
    }
}

// pass 2 (one workgroup): per tile its group base G and its offset l in the group; the distribution's scalars
__global__ __launch_bounds__(HF_BLOCK) void hf_area_scan_tiles_kernel(hf_area_args a) {
    __shared__ double s_sum[HF_BLOCK];
    __shared__ uint32_t s_valid[2];
    if (threadIdx.x == 0) { s_valid[0] = 0xFFFFFFFFu; s_valid[1] = 0u; }
    __syncthreads();
    const uint32_t nt = a.t.ntiles, per = (nt + HF_BLOCK - 1) / HF_BLOCK;
    const uint32_t k0 = min(threadIdx.x * per, nt), k1 = min(k0 + per, nt);
    double *off = a.t.tile + nt; // (G, l) pairs
    double l = 0.0;
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (uint32_t k = k0; k < k1; ++k) {
        off[2 * k + 1] = l;
        l += a.t.tile[k];
        lo = min(lo, a.t.tile_valid[2 * k]);
        hi = max(hi, a.t.tile_valid[2 * k + 1]);
    }
    s_sum[threadIdx.x] = l;
    if (hi != 0u) { atomicMin(&s_valid[0], lo); atomicMax(&s_valid[1], hi); }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double sum = area_chain(s_sum, HF_BLOCK);
        hf_area_info *info = a.t.info;
        info->sum = sum;
        info->sum_f = (float) sum;
        info->norm = (float) (1.0 / sum);
        const bool any = s_valid[1] != 0u; // (none: the reference throws; index 0 keeps every read in bounds)
        info->valid_lo = any ? s_valid[0] : 0u;
        info->valid_hi = any ? s_valid[1] - 1u : 0u;
    }
    __syncthreads();
    const double G = s_sum[threadIdx.x];
    for (uint32_t k = k0; k < k1; ++k) off[2 * k] = G;
}

// pass 3: the CDF of every tile and the coarse table (every 64th entry), stored coalesced through LDS
__global__ __launch_bounds__(HF_BLOCK) void hf_area_cdf_kernel(hf_area_args a) {
    __shared__ float s_area[2 * HF_AREA_CHUNK];
    __shared__ double s_sum[HF_BLOCK];
    int cy, c0;
    const int ncell = area_tile_load(a.f, a.t.ncx, s_area, cy, c0);
    __syncthreads();
    s_sum[threadIdx.x] = area_thread_sum(s_area);
    __syncthreads();
    if (threadIdx.x == 0) area_chain(s_sum, HF_BLOCK);
    __syncthreads();
    const double *off = a.t.tile + a.t.ntiles;
    const double G = off[2 * blockIdx.x], l = off[2 * blockIdx.x + 1], c = s_sum[threadIdx.x];
    double r = 0.0;
#pragma unroll
    for (int j = 0; j < HF_AREA_PER; ++j) { // (each thread rewrites only its own entries)
        float *e = s_area + threadIdx.x * HF_AREA_PER + j;
        r += (double) *e;
        *e = (float) (G + (l + (c + r)));
    }
    __syncthreads();
    const uint32_t base = 2u * ((uint32_t) cy * (uint32_t) (a.f.W - 1) + (uint32_t) c0), cnt = 2u * (uint32_t) ncell;
    for (uint32_t e = threadIdx.x; e < cnt; e += HF_BLOCK) {
        const float v = s_area[e];
        const uint32_t gi = base + e;
        a.t.cdf[gi] = v;
        if ((gi & (HF_AREA_SEG - 1u)) == HF_AREA_SEG - 1u || gi == a.t.m - 1u) a.t.coarse[gi / HF_AREA_SEG] = v;
    }
}

void hf_launch_build_area(const hf_dev_field &f, const hf_area_table &t, hipStream_t stream) {
    hf_area_args a;
    a.f = f; a.t = t;
    hipLaunchKernelGGL(hf_area_reduce_kernel, dim3(t.ntiles), dim3(HF_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(hf_area_scan_tiles_kernel, dim3(1), dim3(HF_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(hf_area_cdf_kernel, dim3(t.ntiles), dim3(HF_BLOCK), 0, stream, a);
}

// Mesh::sample_position for one lane per sample.  The triangle: a binary search over the coarse table (every 64th entry,
// 2 MB at 4096^2: L2-resident) for the first segment whose last entry is not below sample.y * sum, then the 64 entries
// of that segment (256 bytes, 16 independent loads) counted against the target: the CDF is sorted, so the count is the
// first entry that is not below the target -- dr::binary_search's answer once clamped to [valid.x, valid.y].
struct hf_sample_args {
    hf_dev_field f;
    hf_area_table t;
    size_t n;
    const float *s[2];
    const uint8_t *active;
    hf_position_sample_t out;
    const float4 *vn; // smooth shading: the handle's vertex normals
};
template <bool SMOOTH>
__global__ __launch_bounds__(HF_BLOCK) void hf_sample_position_kernel(hf_sample_args a) {
    const size_t stride = (size_t) gridDim.x * HF_BLOCK;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += stride) {
        const bool act = a.active ? a.active[i] != 0 : true;
        v3 p = mk3(0.f, 0.f, 0.f), nn = p;
        float uv0 = 0.f, uv1 = 0.f, pdf = 0.f, bx = 0.f, by = 0.f;
        uint32_t idx = 0u;
        if (act) {
            const float sx = a.s[0][i], sy = a.s[1][i];
            const hf_area_info *info = a.t.info;
            const float target = sy * info->sum_f, norm = info->norm; // sample(): value *= m_sum
            uint32_t lo = 0u, hi = a.t.nseg - 1u;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (a.t.coarse[mid] < target) lo = mid + 1u; else hi = mid;
            }
            const float4 *seg = reinterpret_cast<const float4 *>(a.t.cdf + (size_t) lo * HF_AREA_SEG);
            uint32_t cnt = 0u;
#pragma unroll
            for (int q = 0; q < HF_AREA_SEG / 4; ++q) {
                const float4 v = seg[q];
                cnt += (uint32_t) (v.x < target) + (uint32_t) (v.y < target) + (uint32_t) (v.z < target) + (uint32_t) (v.w < target);
            }
            idx = min(max(lo * HF_AREA_SEG + cnt, info->valid_lo), info->valid_hi);
            idx = min(idx, a.t.m - 1u);
            const float prev = idx > 0u ? a.t.cdf[idx - 1u] : 0.f;
            v3 P[3], N[3];
            float U[3], V[3];
            int vi[3], vj[3];
            prim_world(a.f, idx, P, U, V, vi, vj);
            if (SMOOTH) load_vn(a.f, a.vn, vi, vj, N);
            // sample_reuse: (value - cdf[i-1] norm) / (pmf[i] norm), pmf[i] recomputed from the vertices as build_pmf does
            const float reused = (sy - prev * norm) / (tri_area(P[0], P[1], P[2]) * norm);
            const float t = __builtin_sqrtf(fmaxf(1.f - sx, 0.f)); // square_to_uniform_triangle (safe_sqrt)
            bx = 1.f - t;
            by = t * reused;
            const float b0 = 1.f - bx - by;
            const v3 e0 = P[1] - P[0], e1 = P[2] - P[0];
            p = mk3(__builtin_fmaf(e0.x, bx, __builtin_fmaf(e1.x, by, P[0].x)),
                    __builtin_fmaf(e0.y, bx, __builtin_fmaf(e1.y, by, P[0].y)),
                    __builtin_fmaf(e0.z, bx, __builtin_fmaf(e1.z, by, P[0].z)));
            uv0 = __builtin_fmaf(U[0], b0, __builtin_fmaf(U[1], bx, U[2] * by));
            uv1 = __builtin_fmaf(V[0], b0, __builtin_fmaf(V[1], bx, V[2] * by));
            nn = normalize3(SMOOTH ? sample_blend(N, b0, bx, by) : cross3(e0, e1));
            if (a.f.flip) nn = neg3(nn);
            pdf = norm;
        }
        a.out.p[0][i] = p.x; a.out.p[1][i] = p.y; a.out.p[2][i] = p.z;
        a.out.n[0][i] = nn.x; a.out.n[1][i] = nn.y; a.out.n[2][i] = nn.z;
        a.out.uv[0][i] = uv0; a.out.uv[1][i] = uv1;
        a.out.pdf[i] = pdf;
        if (a.out.prim_index) a.out.prim_index[i] = idx;
        if (a.out.b[0]) a.out.b[0][i] = bx;
        if (a.out.b[1]) a.out.b[1][i] = by;
    }
}

void hf_launch_sample_position(const hf_dev_field &f, const hf_area_table &t, size_t n, const float *const sample[2],
                               const uint8_t *active, const hf_position_sample_t &out, const float4 *vn, hipStream_t stream) {
    if (n == 0) return;
    hf_sample_args a;
    a.f = f; a.t = t; a.n = n; a.s[0] = sample[0]; a.s[1] = sample[1]; a.active = active; a.out = out; a.vn = vn;
    hipLaunchKernelGGL(vn ? hf_sample_position_kernel<true> : hf_sample_position_kernel<false>, dim3(grid_for(n)),
                       dim3(HF_BLOCK), 0, stream, a);
}

// Reverse and forward mode of sample_position with respect to the heights, for the forward's (prim, b): p = P0 + b1 e0
// + b2 e1 moves with the three heights along ez (the third column of to_world times max_height); n = N / |N| with
// N = cross(e0, e1) (flat) or the blend of the three vertex normals (smooth: through vertex_normals_vjp / _jvp).
struct hf_sample_diff_args {
    hf_dev_field f;
    size_t n;
    const uint32_t *prim;
    const float *b[2];
    const uint8_t *active;
    const float *gp[3], *gn[3]; // adjoint: upstream gradients (NULL rows: zero)
    float *grad_h;
    const float *dh;            // tangent: height tangent (NULL: zero)
    float *dp[3], *dn[3];       // tangent: outputs (NULL rows: not written)
    const float4 *vn;
};
// the sample's triangle and what both modes share; false for inactive lanes and out-of-range indices
__device__ __forceinline__ bool sample_diff_setup(const hf_sample_diff_args &a, size_t i, uint32_t &prim, float &bx, float &by) {
    if (a.active && a.active[i] == 0) return false;
    prim = a.prim[i];
    if (prim >= 2u * (uint32_t) (a.f.W - 1) * (uint32_t) (a.f.H - 1)) return false;
    bx = a.b[0][i]; by = a.b[1][i];
    return true;
}

// XFORM (hf_sample_adjoint_xform_kernel): also dL/d(to_world) from the world-space gradients of the three vertices
// (and, smooth, of the 1-rings), block sums to `slab` (xform_block_store); grad_h may then be NULL
template <bool SMOOTH, bool XFORM = false>
__device__ __forceinline__ void sample_adjoint_body(const hf_sample_diff_args &a, float *slab = nullptr) {
    float M[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) M[j] = 0.f;
    const size_t stride = (size_t) gridDim.x * HF_BLOCK;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += stride) {
        uint32_t prim;
        float bx, by;
        if (!sample_diff_setup(a, i, prim, bx, by)) continue;
        const hf_dev_field &f = a.f;
        v3 P[3];
        float U[3], V[3];
        int vi[3], vj[3];
        prim_world(f, prim, P, U, V, vi, vj);
        const v3 ez = height_axis(f);
        const v3 gp = a.gp[0] ? mk3(a.gp[0][i], a.gp[1][i], a.gp[2][i]) : mk3(0.f, 0.f, 0.f);
        v3 gn = a.gn[0] ? mk3(a.gn[0][i], a.gn[1][i], a.gn[2][i]) : mk3(0.f, 0.f, 0.f);
        if (f.flip) gn = neg3(gn);
        const float b0 = 1.f - bx - by, gpz = dot3(gp, ez);
        float gh[3] = { gpz * b0, gpz * bx, gpz * by };
        v3 gB[3];
        if (SMOOTH) {
            v3 N[3];
            load_vn(f, a.vn, vi, vj, N);
            const v3 B = sample_blend(N, b0, bx, by);
            const float r = rsqrt_ieee(dot3(B, B));
            const v3 g = dnormalize(B * r, r, gn);
            gB[0] = g * b0; gB[1] = g * bx; gB[2] = g * by;
        } else {
            const v3 e0 = P[1] - P[0], e1 = P[2] - P[0];
            const auto [n, r] = unit_normal(e0, e1);
            float g1, g2;
            face_normal_vjp(e0, e1, dnormalize(n, r, gn), ez, g1, g2);
            gh[1] += g1; gh[2] += g2; gh[0] -= g1 + g2;
        }
        if constexpr (XFORM) { // p = sum b_k P_k; flat n = N / |N|, N = cross(e0, e1)
            v3 gP[3] = { gp * b0, gp * bx, gp * by };
            if (!SMOOTH) {
                const v3 e0 = P[1] - P[0], e1 = P[2] - P[0];
                const auto [n, r] = unit_normal(e0, e1);
                const v3 gN = dnormalize(n, r, gn);
                const v3 ge0 = cross3(e1, gN), ge1 = cross3(gN, e0);
                gP[1] = gP[1] + ge0; gP[2] = gP[2] + ge1; gP[0] = gP[0] - (ge0 + ge1);
            }
            v3 q[3];
            prim_local(f, vi, vj, q);
#pragma unroll
            for (int k = 0; k < 3; ++k) xform_grad_point(M, gP[k], q[k]);
            if (SMOOTH) vertex_normals_vjp_xform(f, vi, vj, gB, M);
            if (!a.grad_h) continue;
        }
        float *grad_h = a.grad_h;
        auto add = [&](int r, int c, float g) { atomicAdd(grad_h + (size_t) r * f.W + c, g); };
#pragma unroll
        for (int k = 0; k < 3; ++k) add(vi[k], vj[k], gh[k]);
        if (SMOOTH) vertex_normals_vjp(f, vi, vj, ez, gB, add);
    }
    if constexpr (XFORM) xform_block_store(M, slab);
}
template <bool SMOOTH>
__global__ __launch_bounds__(HF_BLOCK) void hf_sample_adjoint_kernel(hf_sample_diff_args a) { sample_adjoint_body<SMOOTH>(a); }
template <bool SMOOTH>
__global__ __launch_bounds__(HF_BLOCK) void hf_sample_adjoint_xform_kernel(hf_sample_diff_args a, float *slab) {
    sample_adjoint_body<SMOOTH, true>(a, slab);
}

// XFORM (hf_sample_tangent_xform_kernel): the vertices also move by dM (q_k, 1) for the tangent dM (12 device floats)
// of to_world; a.dh may then be NULL
template <bool SMOOTH, bool XFORM = false>
__device__ __forceinline__ void sample_tangent_body(const hf_sample_diff_args &a, const float *dMp = nullptr) {
    float dM[12];
    if constexpr (XFORM) {
#pragma unroll
        for (int j = 0; j < 12; ++j) dM[j] = dMp[j];
    }
    const size_t stride = (size_t) gridDim.x * HF_BLOCK;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += stride) {
        uint32_t prim;
        float bx, by;
        v3 dp = mk3(0.f, 0.f, 0.f), dn = dp;
        if ((XFORM || a.dh) && sample_diff_setup(a, i, prim, bx, by)) {
            const hf_dev_field &f = a.f;
            v3 P[3], dP[3];
            float U[3], V[3];
            int vi[3], vj[3];
            prim_world(f, prim, P, U, V, vi, vj, dP, a.dh);
            if constexpr (XFORM) {
                v3 q[3];
                prim_local(f, vi, vj, q);
#pragma unroll
                for (int k = 0; k < 3; ++k) dP[k] = dP[k] + xform_point(dM, q[k]);
            }
            const float b0 = 1.f - bx - by;
            dp = mk3(dP[0].x * b0 + dP[1].x * bx + dP[2].x * by, dP[0].y * b0 + dP[1].y * bx + dP[2].y * by,
                     dP[0].z * b0 + dP[1].z * bx + dP[2].z * by);
            if (SMOOTH) {
                v3 N[3];
                load_vn(f, a.vn, vi, vj, N);
                const v3 B = sample_blend(N, b0, bx, by);
                const float r = rsqrt_ieee(dot3(B, B));
                v3 dB = mk3(0.f, 0.f, 0.f);
                const float w[3] = { b0, bx, by };
                if constexpr (XFORM) vertex_normals_jvp_xform(f, vi, vj, height_axis(f), w, a.dh, dM, dB);
                else vertex_normals_jvp(f, vi, vj, height_axis(f), w, a.dh, dB);
                dn = dnormalize(B * r, r, dB);
            } else {
                const v3 e0 = P[1] - P[0], e1 = P[2] - P[0], de0 = dP[1] - dP[0], de1 = dP[2] - dP[0];
                const auto [n, r] = unit_normal(e0, e1);
                dn = dnormalize(n, r, face_normal_jvp(e0, e1, de0, de1));
            }
            if (f.flip) dn = neg3(dn);
        }
        if (a.dp[0]) { a.dp[0][i] = dp.x; a.dp[1][i] = dp.y; a.dp[2][i] = dp.z; }
        if (a.dn[0]) { a.dn[0][i] = dn.x; a.dn[1][i] = dn.y; a.dn[2][i] = dn.z; }
    }
}
template <bool SMOOTH>
__global__ __launch_bounds__(HF_BLOCK) void hf_sample_tangent_kernel(hf_sample_diff_args a) { sample_tangent_body<SMOOTH>(a); }
template <bool SMOOTH>
__global__ __launch_bounds__(HF_BLOCK) void hf_sample_tangent_xform_kernel(hf_sample_diff_args a, const float *dM) {
    sample_tangent_body<SMOOTH, true>(a, dM);
}

static hf_sample_diff_args sample_diff_args(const hf_dev_field &f, size_t n, const uint32_t *prim, const float *const b[2],
                                            const uint8_t *active, const float4 *vn) {
    hf_sample_diff_args a = {};
    a.f = f; a.n = n; a.prim = prim; a.b[0] = b[0]; a.b[1] = b[1]; a.active = active; a.vn = vn;
    return a;
}
void hf_launch_sample_position_adjoint(const hf_dev_field &f, size_t n, const uint32_t *prim, const float *const b[2],
                                       const uint8_t *active, const float *const gp[3], const float *const gn[3],
                                       float *grad_h, const float4 *vn, hipStream_t stream, float *grad_to_world,
                                       void *slab) {
    if (n == 0 || (!gp && !gn)) return;
    hf_sample_diff_args a = sample_diff_args(f, n, prim, b, active, vn);
    for (int c = 0; c < 3; ++c) { a.gp[c] = gp ? gp[c] : nullptr; a.gn[c] = gn ? gn[c] : nullptr; }
    a.grad_h = grad_h;
    if (grad_to_world) { // slab: hf_xform_slab_bytes(n), this launch's alone
        const int grid = grid_for(n, HF_XFORM_GRID_CAP);
        hipLaunchKernelGGL(vn ? hf_sample_adjoint_xform_kernel<true> : hf_sample_adjoint_xform_kernel<false>, dim3(grid),
                           dim3(HF_BLOCK), 0, stream, a, (float *) slab);
        xform_sum((const float *) slab, grid, grad_to_world, stream);
        return;
    }
    hipLaunchKernelGGL(vn ? hf_sample_adjoint_kernel<true> : hf_sample_adjoint_kernel<false>, dim3(grid_for(n)),
                       dim3(HF_BLOCK), 0, stream, a);
}
void hf_launch_sample_position_tangent(const hf_dev_field &f, size_t n, const uint32_t *prim, const float *const b[2],
                                       const uint8_t *active, const float *dh, float *const dp[3], float *const dn[3],
                                       const float4 *vn, hipStream_t stream, const float *d_to_world) {
    if (n == 0 || (!dp && !dn)) return;
    hf_sample_diff_args a = sample_diff_args(f, n, prim, b, active, vn);
    a.dh = dh;
    for (int c = 0; c < 3; ++c) { a.dp[c] = dp ? dp[c] : nullptr; a.dn[c] = dn ? dn[c] : nullptr; }
    if (d_to_world) {
        hipLaunchKernelGGL(vn ? hf_sample_tangent_xform_kernel<true> : hf_sample_tangent_xform_kernel<false>,
                           dim3(grid_for(n)), dim3(HF_BLOCK), 0, stream, a, d_to_world);
        return;
    }
    hipLaunchKernelGGL(vn ? hf_sample_tangent_kernel<true> : hf_sample_tangent_kernel<false>, dim3(grid_for(n)),
                       dim3(HF_BLOCK), 0, stream, a);
}

// ---------------------------------------------------------------------------------
// Shape attributes (hf_eval_attribute / _adjoint / _tangent): Mesh::interpolate_attribute (mesh.h:399-440) on the
// caller's interleaved [count][SIZE] buffer, one lane per ray.  TYPE HF_ATTR_VERTEX: the barycentric blend of the three
// vertices' values with the weights of bary_coords (hf_device.h) at si.p; HF_ATTR_FACE: the row of si.prim_index.
// One instantiation per (TYPE, SIZE): no per-lane branch on either.
// ---------------------------------------------------------------------------------
// the hit of lane i: false for inactive lanes, t = +inf and out-of-range indices (every lane reads active and t)
__device__ __forceinline__ bool attr_hit(const hf_attr_args &a, size_t i, uint32_t &prim) {
    bool ok = !a.active || a.active[i] != 0;
    if (a.t) ok = ok && a.t[i] != __builtin_inff();
    if (!ok) return false;
    prim = a.prim[i];
    return prim < 2u * (uint32_t) (a.f.W - 1) * (uint32_t) (a.f.H - 1);
}
// the SIZE values of the three vertices of a hit (vertex ids from prim_world)
template <int SIZE>
__device__ __forceinline__ void attr_vertices(const float *buf, const hf_dev_field &f, const int vi[3], const int vj[3],
                                              float A[3][SIZE]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const size_t base = ((size_t) vi[k] * f.W + vj[k]) * SIZE;
#pragma unroll
        for (int c = 0; c < SIZE; ++c) A[k][c] = buf[base + c];
    }
}

template <int TYPE, int SIZE>
__global__ __launch_bounds__(HF_BLOCK) void hf_attr_kernel(hf_attr_args a) {
    const size_t stride = (size_t) gridDim.x * HF_BLOCK;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += stride) {
        float r[SIZE];
#pragma unroll
        for (int c = 0; c < SIZE; ++c) r[c] = 0.f;
        uint32_t prim;
        if (attr_hit(a, i, prim)) {
            if constexpr (TYPE == HF_ATTR_FACE) {
#pragma unroll
                for (int c = 0; c < SIZE; ++c) r[c] = a.attr[(size_t) prim * SIZE + c];
            } else {
                v3 P[3];
                float U[3], V[3], A[3][SIZE];
                int vi[3], vj[3];
                prim_world(a.f, prim, P, U, V, vi, vj);
                attr_vertices<SIZE>(a.attr, a.f, vi, vj, A);
                const hf_bary b = bary_coords(mk3(a.p[0][i], a.p[1][i], a.p[2][i]), P);
#pragma unroll
                for (int c = 0; c < SIZE; ++c) r[c] = bary_interp(b, A[0][c], A[1][c], A[2][c]);
            }
        }
#pragma unroll
        for (int c = 0; c < SIZE; ++c) a.out[c][i] = r[c];
    }
}

// Reverse mode of one vertex-attribute hit, for its upstream gradient g: the vertices (vi, vj), the weights wk = (w, u, v)
// (dL/dattr of vertex k, channel c = g[c] wk[k]), dL/dp (gp) and the three height gradients gh (when grad_p or grad_h is
// wanted; zero otherwise)
template <int SIZE>
__device__ __forceinline__ void attr_vertex_vjp(const hf_attr_args &a, size_t i, uint32_t prim, const float g[SIZE],
                                                int vi[3], int vj[3], float wk[3], float gh[3], v3 &gp) {
    const hf_dev_field &f = a.f;
    v3 P[3];
    float U[3], V[3];
    prim_world(f, prim, P, U, V, vi, vj);
    const hf_bary b = bary_coords(mk3(a.p[0][i], a.p[1][i], a.p[2][i]), P);
    wk[0] = b.w; wk[1] = b.u; wk[2] = b.v;
    gh[0] = gh[1] = gh[2] = 0.f;
    if (a.grad_p[0] || a.grad_h) {
        float A[3][SIZE];
        attr_vertices<SIZE>(a.attr, f, vi, vj, A);
        float gw = 0.f, gu = 0.f, gv = 0.f; // dL/dw, dL/du, dL/dv
#pragma unroll
        for (int c = 0; c < SIZE; ++c) { gw += g[c] * A[0][c]; gu += g[c] * A[1][c]; gv += g[c] * A[2][c]; }
        v3 gP[3];
        bary_coords_vjp(b, gu - gw, gv - gw, gp, gP); // (w = 1 - u - v)
        const v3 ez = height_axis(f);
#pragma unroll
        for (int k = 0; k < 3; ++k) gh[k] = dot3(ez, gP[k]);
    }
}

// Reverse mode of a face attribute: dL/dattr into the row of prim_index, plain float atomics (a face attribute carries no
// geometric derivative; dL/dp is zero)
template <int SIZE>
__global__ __launch_bounds__(HF_BLOCK) void hf_attr_face_adjoint_kernel(hf_attr_args a) {
    const size_t stride = (size_t) gridDim.x * HF_BLOCK;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += stride) {
        uint32_t prim;
        if (a.grad_attr && attr_hit(a, i, prim)) {
#pragma unroll
            for (int c = 0; c < SIZE; ++c) atomicAdd(a.grad_attr + (size_t) prim * SIZE + c, a.g[c][i]);
        }
        if (a.grad_p[0]) { a.grad_p[0][i] = 0.f; a.grad_p[1][i] = 0.f; a.grad_p[2][i] = 0.f; }
    }
}

// Reverse mode of a vertex attribute: dL/dattr, dL/dheight through the per-wave LDS scatter tile of hf_adjoint_kernel
// (tile_anchor / tile_add / tile_flush) and dL/dp (rows, overwritten).  One TILE x TILE plane per attribute channel and
// one for the heights, anchored near the wave's first hit: a hit adds its 3 (SIZE + 1) contributions into the planes
// (ds_add_f32), or straight to global memory outside the tile; the flush then adds each touched texel of each plane to
// global memory once.  On the bench wavefront (size 3) this takes 7.53 ms where plain float atomics took 10.06 ms and a
// 16 x 16 tile 7.83 ms (profiles/attributes/adjoint_ab.txt).
template <int SIZE, int TILE>
__global__ __launch_bounds__(HF_BLOCK) void hf_attr_adjoint_tile_kernel(hf_attr_args a) {
    constexpr int TT = TILE * TILE;
    __shared__ float s_acc[HF_BLOCK / 64][(SIZE + 1) * TT];
    float *acc = s_acc[threadIdx.x >> 6];
    const int lane = (int) (threadIdx.x & 63u);
    for (int k = lane; k < (SIZE + 1) * TT; k += 64) acc[k] = 0.f;
    const int W = a.f.W;
    const size_t stride = (size_t) gridDim.x * HF_BLOCK;
    // whole waves stay in the loop (the ballot below)
    for (size_t ub = (size_t) blockIdx.x * HF_BLOCK + (threadIdx.x & ~63u); ub < a.n; ub += stride) {
        const size_t i = ub + (size_t) lane;
        v3 gp = mk3(0.f, 0.f, 0.f);
        float g[SIZE], wk[3] = { 0.f, 0.f, 0.f }, gh[3] = { 0.f, 0.f, 0.f };
        int vr[3] = { 0, 0, 0 }, vc[3] = { 0, 0, 0 };
        uint32_t prim;
        const bool scatter = i < a.n && attr_hit(a, i, prim);
        if (scatter) {
#pragma unroll
            for (int c = 0; c < SIZE; ++c) g[c] = a.g[c][i];
            attr_vertex_vjp<SIZE>(a, i, prim, g, vr, vc, wk, gh, gp);
        }
        const uint64_t sm = __ballot(scatter);
        if (sm != 0ull) {
            int ar, ac;
            tile_anchor(sm, vr, vc, TILE / 4, ar, ac); // from the first scattering lane
            hf_tile_rows<TILE> rows = 0u;
            if (scatter) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (a.grad_attr) {
#pragma unroll
                        for (int c = 0; c < SIZE; ++c)
                            tile_add<TILE, SIZE>(acc + c * TT, ar, ac, vr[k], vc[k], g[c] * wk[k], a.grad_attr + c, W, rows);
                    }
                    if (a.grad_h) tile_add<TILE>(acc + SIZE * TT, ar, ac, vr[k], vc[k], gh[k], a.grad_h, W, rows);
                }
            }
            if (a.grad_attr) {
#pragma unroll
                for (int c = 0; c < SIZE; ++c) tile_flush<TILE, SIZE>(acc + c * TT, ar, ac, rows, a.grad_attr + c, W, lane);
            }
            if (a.grad_h) tile_flush<TILE>(acc + SIZE * TT, ar, ac, rows, a.grad_h, W, lane);
        }
        if (i < a.n && a.grad_p[0]) { a.grad_p[0][i] = gp.x; a.grad_p[1][i] = gp.y; a.grad_p[2][i] = gp.z; }
    }
}

// Forward mode: the tangent of the value for the tangents dattr (interleaved like attr), dp of si.p and dh of the
// heights (each NULL = zero).  No atomics: bitwise the same from launch to launch.
template <int TYPE, int SIZE>
__global__ __launch_bounds__(HF_BLOCK) void hf_attr_tangent_kernel(hf_attr_args a) {
    const size_t stride = (size_t) gridDim.x * HF_BLOCK;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += stride) {
        float r[SIZE];
#pragma unroll
        for (int c = 0; c < SIZE; ++c) r[c] = 0.f;
        uint32_t prim;
        if (attr_hit(a, i, prim)) {
            if constexpr (TYPE == HF_ATTR_FACE) {
                if (a.dattr) {
#pragma unroll
                    for (int c = 0; c < SIZE; ++c) r[c] = a.dattr[(size_t) prim * SIZE + c];
                }
            } else {
                v3 P[3], dP[3];
                float U[3], V[3], A[3][SIZE];
                int vi[3], vj[3];
                prim_world(a.f, prim, P, U, V, vi, vj, dP, a.dh);
                attr_vertices<SIZE>(a.attr, a.f, vi, vj, A);
                const hf_bary b = bary_coords(mk3(a.p[0][i], a.p[1][i], a.p[2][i]), P);
                const v3 dp = a.dp[0] ? mk3(a.dp[0][i], a.dp[1][i], a.dp[2][i]) : mk3(0.f, 0.f, 0.f);
                float du, dv;
                bary_coords_jvp(b, dp, dP, du, dv);
                const float dw = -du - dv;
#pragma unroll
                for (int c = 0; c < SIZE; ++c) r[c] = A[0][c] * dw + A[1][c] * du + A[2][c] * dv;
                if (a.dattr) {
                    float dA[3][SIZE];
                    attr_vertices<SIZE>(a.dattr, a.f, vi, vj, dA);
#pragma unroll
                    for (int c = 0; c < SIZE; ++c) r[c] += dA[0][c] * b.w + dA[1][c] * b.u + dA[2][c] * b.v;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < SIZE; ++c) a.dout[c][i] = r[c];
    }
}

#define HF_ATTR_TILE 32 // texels per side of the vertex adjoint's LDS planes (16: 7.83 ms, 32: 7.53 ms on the bench)
template <int TYPE, int SIZE>
static void attr_launch(int mode, const hf_attr_args &a, hipStream_t stream) {
    if (TYPE == HF_ATTR_VERTEX && mode == 1) { // grid-stride at the default cap, like hf_adjoint_kernel (a tile to clear per wave)
        void (*k)(hf_attr_args) = hf_attr_adjoint_tile_kernel<SIZE, HF_ATTR_TILE>;
        hipLaunchKernelGGL(k, dim3(grid_for(a.n)), dim3(HF_BLOCK), 0, stream, a);
        return;
    }
    void (*k)(hf_attr_args) = mode == 0 ? hf_attr_kernel<TYPE, SIZE>
                            : mode == 1 ? hf_attr_face_adjoint_kernel<SIZE> : hf_attr_tangent_kernel<TYPE, SIZE>;
    // streaming kernels with no per-block state: one block per 256 rays, as hf_si_kernel
    hipLaunchKernelGGL(k, dim3(grid_for(a.n, HF_SI_GRID_CAP)), dim3(HF_BLOCK), 0, stream, a);
}
void hf_launch_attribute(int mode, int type, uint32_t size, const hf_attr_args &a, hipStream_t stream) {
    if (a.n == 0) return;
    if (type == HF_ATTR_VERTEX) size == 1 ? attr_launch<HF_ATTR_VERTEX, 1>(mode, a, stream) : attr_launch<HF_ATTR_VERTEX, 3>(mode, a, stream);
    else                        size == 1 ? attr_launch<HF_ATTR_FACE, 1>(mode, a, stream) : attr_launch<HF_ATTR_FACE, 3>(mode, a, stream);
}

// ---------------------------------------------------------------------------------
// eval_parameterization (hf_eval_parameterization / _adjoint / _tangent): the surface interaction at texture coordinates
// (Shape::eval_parameterization, mesh.cpp:614-635).  One lane per query: the two uv rows (coalesced), the closed-form
// lookup in registers (param_lookup, hf_device.h), then the hit-geometry helpers on (prim, b) -- compute_si_to for the
// record with Mesh's UV-space ray o = (u, v, -1), d = (0, 0, 1) and t = 1, the FollowShape branches of adjoint_body /
// tangent_body for the derivatives.  Nothing is materialised between the lookup and the helpers.
// ---------------------------------------------------------------------------------
struct hf_param_args {
    hf_dev_field f;
    size_t n;
    const float *uv[2];
    const uint8_t *active;
    hf_si_t sio;
    uint32_t *prim_out; // may be NULL
    uint32_t flags;     // the caller's, without HF_RAY_FOLLOWSHAPE; with HF_RAY_BOUNDARY_ALL_EDGES under BoundaryTest
    const float4 *vn;   // hf_param_smooth_kernel: the handle's vertex normals
};
typedef const __attribute__((address_space(4))) hf_param_args *hf_param_kargs;

// Shaped like si_body (one block per 256 queries, arguments from the kernarg segment where they are used, every field
// stored as soon as it is final): two coalesced loads and the optional mask, then one round trip for the three heights
// (and three vertex normals) -- no load waits on another beyond that.  Invalid lanes get si_miss_to with wi = 0 and
// prim_index 0.
template <bool SMOOTH>
__device__ __forceinline__ void param_body() {
    const uint32_t lane = threadIdx.x & 63u;
    const size_t stride = (size_t) gridDim.x * HF_BLOCK;
    for (size_t ub = (size_t) blockIdx.x * HF_BLOCK + (threadIdx.x & ~63u);; ub += stride) {
        hf_param_kargs ka = (hf_param_kargs) __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka)); // opaque: keeps the loads that follow where they are written
        const size_t n = ka->n;
        if (ub >= n) break; // wave-uniform
        if (lane >= n - ub) continue;
        const uint32_t lo = lane;
        const float u = (ka->uv[0] + ub)[lo], v = (ka->uv[1] + ub)[lo];
        const uint8_t *active = ka->active;
        uint32_t prim = 0u;
        float b1 = 0.f, b2 = 0.f;
        const bool act = (active ? ((active + ub)[lo] != 0) : true) && param_lookup(ka->f.W, ka->f.H, u, v, prim, b1, b2);
        const uint32_t flags = ka->flags;
        hf_si_sink<hf_param_kargs> out = { ka, ub, lo, flags };
        if (act) {
            const hf_dev_field f = load_field(&ka->f);
            compute_si_to<SMOOTH>(f, mk3(u, v, -1.f), mk3(0.f, 0.f, 1.f), 1.f, b1, b2, prim, flags, out, SMOOTH ? ka->vn : nullptr);
        } else {
            prim = 0u;
            si_miss_to(out, flags);
            out.wi(mk3(0.f, 0.f, 0.f));
        }
        if (uint32_t *po = ka->prim_out) __builtin_nontemporal_store(prim, &(po + ub)[lo]);
    }
}
__global__ __launch_bounds__(HF_BLOCK) void hf_param_kernel(hf_param_args a_) { (void) a_; param_body<false>(); }
__global__ __launch_bounds__(HF_BLOCK) void hf_param_smooth_kernel(hf_param_args a_) { (void) a_; param_body<true>(); }

// the adjoint (float atomics into grad_h through the per-wave LDS tile) and the transform slab: adjoint_body's launch bounds
__global__ __launch_bounds__(HF_BLOCK, 5) void hf_param_adjoint_kernel(hf_param_adjoint_args a_) {
    (void) a_;
    __shared__ float s_acc[HF_BLOCK / 64][HF_ADJ_TILE * HF_ADJ_TILE];
    adjoint_body<false, false, false, true>(s_acc[threadIdx.x >> 6]);
}
__global__ __launch_bounds__(HF_BLOCK, 4) void hf_param_adjoint_smooth_kernel(hf_param_adjoint_args a_) {
    (void) a_;
    __shared__ float s_acc[HF_BLOCK / 64][HF_ADJ_TILE * HF_ADJ_TILE];
    adjoint_body<false, true, false, true>(s_acc[threadIdx.x >> 6]);
}
__global__ __launch_bounds__(HF_BLOCK, 5) void hf_param_adjoint_xform_kernel(hf_param_adjoint_args a_, float *slab) {
    (void) a_;
    __shared__ float s_acc[HF_BLOCK / 64][HF_ADJ_TILE * HF_ADJ_TILE];
    adjoint_body<false, false, true, true>(s_acc[threadIdx.x >> 6], slab);
}
__global__ __launch_bounds__(HF_BLOCK, 3) void hf_param_adjoint_xform_smooth_kernel(hf_param_adjoint_args a_, float *slab) {
    (void) a_;
    __shared__ float s_acc[HF_BLOCK / 64][HF_ADJ_TILE * HF_ADJ_TILE];
    adjoint_body<false, true, true, true>(s_acc[threadIdx.x >> 6], slab);
}
__global__ __launch_bounds__(HF_BLOCK) void hf_param_tangent_kernel(hf_param_tangent_args a_) {
    (void) a_;
    tangent_body<false, false, false, true>();
}
__global__ __launch_bounds__(HF_BLOCK) void hf_param_tangent_smooth_kernel(hf_param_tangent_args a_) {
    (void) a_;
    tangent_body<false, true, false, true>();
}
__global__ __launch_bounds__(HF_BLOCK) void hf_param_tangent_xform_kernel(hf_param_tangent_args a_, const float *dM) {
    (void) a_;
    tangent_body<false, false, true, true>(dM);
}
__global__ __launch_bounds__(HF_BLOCK) void hf_param_tangent_xform_smooth_kernel(hf_param_tangent_args a_, const float *dM) {
    (void) a_;
    tangent_body<false, true, true, true>(dM);
}

void hf_launch_param(const hf_dev_field &f, size_t n, const float *const uv[2], const uint8_t *active, const hf_si_t *si,
                     uint32_t *prim_out, uint32_t flags, hipStream_t stream, const float4 *vn) {
    if (n == 0) return;
    hf_param_args a;
    a.f = f; a.n = n; a.uv[0] = uv[0]; a.uv[1] = uv[1]; a.active = active; a.sio = *si; a.prim_out = prim_out;
    a.flags = flags; a.vn = vn;
    hipLaunchKernelGGL(vn ? hf_param_smooth_kernel : hf_param_kernel, dim3(grid_for(n, HF_SI_GRID_CAP)), dim3(HF_BLOCK), 0,
                       stream, a);
}

void hf_launch_param_adjoint(const hf_dev_field &f, size_t n, const float *const uv[2], const uint8_t *active,
                             const hf_si_grad_t *gs, uint32_t flags, float *grad_h, hipStream_t stream, const float4 *vn,
                             float *grad_to_world, void *slab) {
    if (n == 0) return;
    hf_param_adjoint_args p = {};
    hf_adjoint_args &a = p.a;
    a.f = f; a.n = n; a.active = active; a.g = *gs; a.flags = flags; a.grad_h = grad_h; a.vn = vn;
    p.uv[0] = uv[0]; p.uv[1] = uv[1];
    if (grad_to_world) { // slab: hf_xform_slab_bytes(n), this launch's alone
        const int grid = grid_for(n, HF_XFORM_GRID_CAP);
        hipLaunchKernelGGL(vn ? hf_param_adjoint_xform_smooth_kernel : hf_param_adjoint_xform_kernel, dim3(grid),
                           dim3(HF_BLOCK), 0, stream, p, (float *) slab);
        xform_sum((const float *) slab, grid, grad_to_world, stream);
        return;
    }
    hipLaunchKernelGGL(vn ? hf_param_adjoint_smooth_kernel : hf_param_adjoint_kernel, dim3(grid_for(n)), dim3(HF_BLOCK), 0,
                       stream, p);
}

void hf_launch_param_tangent(const hf_dev_field &f, size_t n, const float *const uv[2], const uint8_t *active,
                             uint32_t flags, const float *dh, const float *d_to_world, const hf_si_tangent_t *out,
                             hipStream_t stream, const float4 *vn) {
    if (n == 0) return;
    hf_param_tangent_args p = {};
    hf_tangent_args &a = p.a;
    a.f = f; a.n = n; a.active = active; a.dh = dh; a.out = *out; a.flags = flags; a.vn = vn;
    p.uv[0] = uv[0]; p.uv[1] = uv[1];
    const dim3 grid(grid_for(n, HF_SI_GRID_CAP)), block(HF_BLOCK);
    if (d_to_world) {
        hipLaunchKernelGGL(vn ? hf_param_tangent_xform_smooth_kernel : hf_param_tangent_xform_kernel, grid, block, 0, stream,
                           p, d_to_world);
        return;
    }
    hipLaunchKernelGGL(vn ? hf_param_tangent_smooth_kernel : hf_param_tangent_kernel, grid, block, 0, stream, p);
}

// ---------------------------------------------------------------------------------
// Environment-map lighting (include/hf.h hf_envmap_*): diffuse surface under a latitude-longitude radiance map
// (src/emitters/envmap.cpp), the K = num_rays emitter samples of every wavefront sample drawn by importance sampling of
// the map, traced (any hit, per lane) and reduced in ONE launch: hf_sky_kernel's mapping, with the draw (two binary
// searches of the caller's table, four texels, the angles and the rotation) in place of the uniform sphere.
// ---------------------------------------------------------------------------------
// the solid-angle factor of cell row cy: sin(pi (cy + 1/2) / (H - 1)), evaluated in double and rounded once
__device__ __forceinline__ float env_row_sin(uint32_t cy, uint32_t H) {
    double sn, cs;
    env_sincospi_f64(((double) cy + 0.5) / (double) (H - 1u), sn, cs);
    return (float) sn;
}
// m_c: the mean of max(texel, 0) over the four corners of cell (cx, cy); float32, this association
__device__ __forceinline__ float env_cell_mean(float v00, float v10, float v01, float v11) {
    return 0.25f * ((fmaxf(v00, 0.f) + fmaxf(v10, 0.f)) + (fmaxf(v01, 0.f) + fmaxf(v11, 0.f)));
}
// weight_c = sin_cy ((1 - u) m_c + u mbar): float32, one rounding per step, no fused step
__device__ __forceinline__ float env_cell_weight(float mc, float rs, float u, float mbar) {
    return rs * ((1.f - u) * mc + u * mbar);
}
#define HF_ENV_HEADER 4u // {Sigma, mbar, u, 0}, then the marginal (H - 1), then the conditional rows ((H - 1)(W - 1))

// thread 0 adds s[0 .. cnt) to acc in order (fp64) and, with `out`, writes every running sum rounded once
__device__ __forceinline__ double env_chain(const double *s, uint32_t cnt, double acc, float *out) {
    for (uint32_t j = 0; j < cnt; ++j) {
        acc += s[j];
        if (out) out[j] = (float) acc;
    }
    return acc;
}
// mbar from the rows' sums of m_c that pass 1 left in the marginal's slots: their fp64 sum in row order / the cell count
__device__ __forceinline__ float env_mbar(const float *table, uint32_t W, uint32_t H) {
    double s = 0.0;
    for (uint32_t r = 0; r + 1u < H; ++r) s += (double) table[HF_ENV_HEADER + r];
    return (float) (s / ((double) (W - 1u) * (double) (H - 1u)));
}
// PASS 0: the sum of m_c of every cell row -> the row's slot of the marginal (float32; read back by the next two passes)
// PASS 1: the conditional prefix sums of every cell row
template <int PASS>
__global__ __launch_bounds__(HF_BLOCK) void hf_envmap_rows_kernel(uint32_t W, uint32_t H, const float *__restrict__ data, float u,
                                                                 float *__restrict__ table) {
    __shared__ double s_val[HF_BLOCK];
    __shared__ float s_mbar;
    const uint32_t cy = blockIdx.x, ncx = W - 1u;
    if (PASS == 1 && threadIdx.x == 0) s_mbar = env_mbar(table, W, H);
    __syncthreads();
    const float mbar = PASS == 1 ? s_mbar : 0.f, rs = env_row_sin(cy, H);
    float *crow = table + HF_ENV_HEADER + (H - 1u) + (size_t) cy * ncx;
    double acc = 0.0;
    for (uint32_t c0 = 0; c0 < ncx; c0 += HF_BLOCK) {
        const uint32_t cx = c0 + threadIdx.x;
        double v = 0.0;
        if (cx < ncx) {
            const size_t r0 = (size_t) cy * W + cx, r1 = r0 + W;
            const float mc = env_cell_mean(data[r0], data[r0 + 1], data[r1], data[r1 + 1]);
            v = (double) (PASS == 0 ? mc : env_cell_weight(mc, rs, u, mbar));
        }
        s_val[threadIdx.x] = v;
        __syncthreads();
        if (threadIdx.x == 0) acc = env_chain(s_val, min(ncx - c0, (uint32_t) HF_BLOCK), acc, PASS == 1 ? crow + c0 : nullptr);
        __syncthreads();
    }
    if (PASS == 0 && threadIdx.x == 0) table[HF_ENV_HEADER + cy] = (float) acc;
}
// the marginal: the fp64 running sum, in row order, of the float32 row sums (the last conditional entry of a row), and the header
__global__ void hf_envmap_marginal_kernel(uint32_t W, uint32_t H, float u, float *__restrict__ table) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float mbar = env_mbar(table, W, H); // (before the slots are overwritten)
    const uint32_t ncx = W - 1u;
    const float *cond = table + HF_ENV_HEADER + (H - 1u);
    double acc = 0.0;
    float last = 0.f;
    for (uint32_t r = 0; r + 1u < H; ++r) {
        acc += (double) cond[(size_t) r * ncx + (ncx - 1u)];
        table[HF_ENV_HEADER + r] = last = (float) acc;
    }
    table[0] = last; table[1] = mbar; table[2] = u; table[3] = 0.f;
}

void hf_launch_envmap_build(uint32_t W, uint32_t H, const float *data, float u, float *table, hipStream_t stream) {
    hipLaunchKernelGGL(hf_envmap_rows_kernel<0>, dim3(H - 1u), dim3(HF_BLOCK), 0, stream, W, H, data, u, table);
    hipLaunchKernelGGL(hf_envmap_rows_kernel<1>, dim3(H - 1u), dim3(HF_BLOCK), 0, stream, W, H, data, u, table);
    hipLaunchKernelGGL(hf_envmap_marginal_kernel, dim3(1), dim3(64), 0, stream, W, H, u, table);
}

// ---- the draw ----
// first index in [0, n) whose entry is not below x (n - 1 if there is none): a branch-free lower bound, the trip count
// depends on n alone (wave-uniform)
__device__ __forceinline__ uint32_t env_lower_bound(const float *__restrict__ T, uint32_t n, float x) {
    uint32_t base = 0u;
    for (uint32_t len = n; len > 1u;) {
        const uint32_t half = len >> 1;
        base += (T[base + half - 1u] < x) ? half : 0u;
        len -= half;
    }
    base += (T[base] < x) ? 1u : 0u;
    return base < n ? base : n - 1u;
}
// one draw: the cell, the position in it, the cell's four texels, its weight (recomputed from the texels and the header)
struct hf_env_draw {
    uint32_t cx, cy;
    float fx, fy, wc, sigma;
    float v00, v10, v01, v11;
    bool valid;
};
#define HF_ENV_ONE_BELOW 0.99999994f // 1 - 2^-24
__device__ __forceinline__ hf_env_draw env_draw(const float *__restrict__ data, const float *__restrict__ table, uint32_t W,
                                                uint32_t H, float sx, float sy) {
    hf_env_draw r;
    const uint32_t ncx = W - 1u, ncy = H - 1u;
    const float *M = table + HF_ENV_HEADER, *C = M + ncy;
    r.sigma = table[0];
    const float mbar = table[1], u = table[2];
    const float y = sy * r.sigma;
    r.cy = env_lower_bound(M, ncy, y);
    const float *row = C + (size_t) r.cy * ncx;
    const float rowsum = row[ncx - 1u];
    r.fy = fminf(fmaxf((y - (r.cy ? M[r.cy - 1u] : 0.f)) / rowsum, 0.f), HF_ENV_ONE_BELOW);
    const float x = sx * rowsum;
    r.cx = env_lower_bound(row, ncx, x);
    const size_t r0 = (size_t) r.cy * W + r.cx, r1 = r0 + W;
    r.v00 = data[r0]; r.v10 = data[r0 + 1]; r.v01 = data[r1]; r.v11 = data[r1 + 1];
    r.wc = env_cell_weight(env_cell_mean(r.v00, r.v10, r.v01, r.v11), env_row_sin(r.cy, H), u, mbar);
    r.fx = fminf(fmaxf((x - (r.cx ? row[r.cx - 1u] : 0.f)) / r.wc, 0.f), HF_ENV_ONE_BELOW);
    r.valid = r.sigma > 0.f && r.wc > 0.f;
    if (!r.valid) { r.fx = 0.f; r.fy = 0.f; } // (a corner of the cell: an invalid draw still has a finite direction)
    return r;
}
// the rotation (row-major) of a local direction
__device__ __forceinline__ v3 env_rotate(const float *R, v3 d) {
    return mk3(__builtin_fmaf(R[2], d.z, __builtin_fmaf(R[1], d.y, R[0] * d.x)),
               __builtin_fmaf(R[5], d.z, __builtin_fmaf(R[4], d.y, R[3] * d.x)),
               __builtin_fmaf(R[8], d.z, __builtin_fmaf(R[7], d.y, R[6] * d.x)));
}
// the float32 direction of a draw (what the ray takes): uv = ((cx + fx + 1/2) / (W - 1), (cy + fy) / (H - 1)), theta = pi
// uv.y, phi = 2 pi uv.x, local (sin theta sin phi, cos theta, -sin theta cos phi) (envmap.cpp:393-397), world R d
template <typename RT>
__device__ __forceinline__ v3 env_dir(uint32_t cx, uint32_t cy, float fx, float fy, uint32_t W, uint32_t H, RT R) {
    const float ux = ((float) cx + (fx + 0.5f)) / (float) (W - 1u);
    // theta from the nearer pole: in the lower half uv.y = 1 - ((H - 1 - cy) - fy) / (H - 1), and the difference in the
    // bracket is exact where it is small, so sin theta keeps its relative precision at the south pole as at the north
    const bool south = 2u * cy + 1u >= H - 1u;
    const float uy = (south ? (float) (H - 1u - cy) - fy : (float) cy + fy) / (float) (H - 1u);
    float st, ct, sp, cp;
    sincospif(uy, &st, &ct);
    ct = south ? -ct : ct;
    sincospif(2.f * ux, &sp, &cp);
    const float rr[9] = { R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8] };
    return env_rotate(rr, mk3(st * sp, ct, -(st * cp)));
}
// the same direction in double for the shading sums, and what the emitter weight is made of: L (the bilinear radiance,
// envmap.cpp:498-555) and G = 2 pi^2 sin theta Sigma / (weight_c (W - 1)(H - 1)) = 1 / pdf_omega: E = L G.  bw: the four
// bilinear weights (v00, v10, v01, v11)
struct hf_env_shade { hf_d3 w; double L, G, bw[4]; };
template <typename RT>
__device__ __forceinline__ hf_d3 env_dir_f64(uint32_t cx, uint32_t cy, float fx, float fy, uint32_t W, uint32_t H, RT R, double &st) {
    const double ux = ((double) cx + ((double) fx + 0.5)) / (double) (W - 1u), uy = ((double) cy + (double) fy) / (double) (H - 1u);
    double ct, sp, cp;
    env_sincospi_f64(uy, st, ct);
    env_sincospi_f64(2.0 * ux, sp, cp);
    const double x = st * sp, y = ct, z = -(st * cp);
    return hf_d3{ (double) R[0] * x + (double) R[1] * y + (double) R[2] * z, (double) R[3] * x + (double) R[4] * y + (double) R[5] * z,
                  (double) R[6] * x + (double) R[7] * y + (double) R[8] * z };
}
__device__ __forceinline__ double env_inv_pdf(float wc, float sigma, double st, uint32_t W, uint32_t H) {
    return (19.739208802178716 * st * (double) sigma) / ((double) wc * ((double) (W - 1u) * (double) (H - 1u)));
}
__device__ __forceinline__ double env_bilinear(float fx, float fy, double v00, double v10, double v01, double v11) {
    const double x1 = (double) fx, x0 = 1.0 - x1, y1 = (double) fy, y0 = 1.0 - y1;
    return y0 * (x0 * v00 + x1 * v10) + y1 * (x0 * v01 + x1 * v11);
}
// E_k <sh_n, w_k> of a valid draw, in double
template <typename RT>
__device__ __forceinline__ double env_term(const hf_env_draw &r, v3 sn, uint32_t W, uint32_t H, RT R) {
    double st;
    const hf_d3 w = env_dir_f64(r.cx, r.cy, r.fx, r.fy, W, H, R, st);
    return sky_dot_f64(sn, w) * (env_bilinear(r.fx, r.fy, r.v00, r.v10, r.v01, r.v11) * env_inv_pdf(r.wc, r.sigma, st, W, H));
}

typedef const __attribute__((address_space(4))) hf_envmap_args *hf_envmap_kargs;

#ifndef HF_ENVMAP_WAVES
#define HF_ENVMAP_WAVES 6 // resident waves per SIMD
#endif
__global__ __launch_bounds__(HF_BLOCK, HF_ENVMAP_WAVES) void hf_envmap_kernel(hf_envmap_args a) {
    const hf_dev_field &f = a.f;
    const size_t i64 = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; // n < 2^32 (hf_envmap_lighting)
    const bool in = i64 < a.n;
    const uint32_t i = (uint32_t) i64;
    const uint32_t ii = in ? i : (uint32_t) (a.n - 1);
    const v3 sn = mk3(a.sh_n[0][ii], a.sh_n[1][ii], a.sh_n[2][ii]);
    bool elig;
    {
        const v3 d = mk3(a.d[0][ii], a.d[1][ii], a.d[2][ii]);
        elig = in && sky_eligible(a.t[ii], sn, d);
    }
    double acc = 0.0;   // sum over the visible directions of <sh_n, w_k> E_k, in k order
    uint32_t bits = 0u; // bit k: direction k was traced and is unoccluded
    if (__ballot(elig) != 0ull) { // wave-uniform: a batch without an eligible sample draws nothing
        const v3 p = mk3(a.p[0][ii], a.p[1][ii], a.p[2][ii]);
        const v3 gn = mk3(a.nrm[0][ii], a.nrm[1][ii], a.nrm[2][ii]);
        const uint32_t id = a.ray_id ? a.ray_id[ii] : ii;
        const float mag = sky_offset(p);
        hf_envmap_kargs ka = (hf_envmap_kargs) __builtin_amdgcn_kernarg_segment_ptr();
#pragma unroll 1
        for (uint32_t k = 0;; ++k) { // wave-uniform loop, the lanes predicated inside
            asm volatile("" : "+s"(ka)); // opaque per direction: the kernarg loads stay inside the loop
            // the draw and the term that is added first, finished before the ray is begun: the texels and the doubles are
            // dead when setup_ray's registers fill; the cell, the position in it and the term are held across the walk
            uint32_t cx, cy;
            float fx, fy;
            double co;
            bool valid;
            {
                float sx, sy;
                sky_sample(ka->seed, k, id, sx, sy);
                const hf_env_draw r = env_draw(ka->data, ka->table, ka->W, ka->H, sx, sy);
                v3 snd = sn; // (opaque: the conversions of sh_n to double are otherwise hoisted out of the loop)
                asm volatile("" : "+v"(snd.x), "+v"(snd.y), "+v"(snd.z));
                co = r.valid ? env_term(r, snd, ka->W, ka->H, ka->rot) : 0.0;
                cx = r.cx; cy = r.cy; fx = r.fx; fy = r.fy; valid = r.valid;
            }
            asm volatile("" : "+v"(cx), "+v"(cy), "+v"(fx), "+v"(fy));
            const v3 w = env_dir(cx, cy, fx, fy, ka->W, ka->H, ka->rot);
            const bool traced = elig && valid && dot3(sn, w) > 0.f;
            hf_hit best;
            light_walk<true>(&ka->f, f, sky_origin(p, gn, mag, w), w, traced, best);
            if (traced && !best.hit) { bits |= 1u << k; acc += co; }
            if (k + 1u >= ka->num_rays) break;
        }
    }
    hf_envmap_kargs ko = (hf_envmap_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ko));
    float c = 0.f;
    if (elig) { // (eligible: in range)
        const float *weight = ko->weight;
        c = (float) ((double) ko->scale * acc);
        if (weight) c *= weight[i];
    }
    uint32_t *vis_bits = ko->vis_bits;
    if (in && vis_bits) vis_bits[i] = bits;
    const uint32_t spp = ko->spp, g = spp < 64u ? spp : 64u;
    film_pixel(ko->image, c, 0u, ko->n / spp, i, spp, in, (spp & (spp - 1u)) == 0u, g, 1.0f / (float) spp, i);
}

// shadow ray a.k of every sample, materialised: what hf_envmap_kernel traces for that direction, bit for bit
__global__ __launch_bounds__(HF_BLOCK) void hf_envmap_rays_kernel(hf_envmap_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    v3 sn;
    const bool elig = light_sample(a, i, sn);
    const v3 p = mk3(a.p[0][i], a.p[1][i], a.p[2][i]), gn = mk3(a.nrm[0][i], a.nrm[1][i], a.nrm[2][i]);
    float sx, sy;
    sky_sample(a.seed, a.k, light_id(a, i), sx, sy);
    const hf_env_draw r = env_draw(a.data, a.table, a.W, a.H, sx, sy);
    const v3 w = env_dir(r.cx, r.cy, r.fx, r.fy, a.W, a.H, a.rot);
    light_store_ray(a, i, sky_origin(p, gn, sky_offset(p), w), w, elig && r.valid && dot3(sn, w) > 0.f);
    if (a.out_weight) {
        double st;
        (void) env_dir_f64(r.cx, r.cy, r.fx, r.fy, a.W, a.H, a.rot, st);
        a.out_weight[i] = r.valid ? (float) (env_bilinear(r.fx, r.fy, r.v00, r.v10, r.v01, r.v11) * env_inv_pdf(r.wc, r.sigma, st, a.W, a.H)) : 0.f;
    }
}

// Emitter::sample_direction for caller-supplied samples: direction (float32, as the rays take it), E, pdf_omega, cell
__global__ __launch_bounds__(HF_BLOCK) void hf_envmap_sample_kernel(hf_envmap_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const hf_env_draw r = env_draw(a.data, a.table, a.W, a.H, a.sample[0][i], a.sample[1][i]);
    const v3 w = env_dir(r.cx, r.cy, r.fx, r.fy, a.W, a.H, a.rot);
    double st;
    (void) env_dir_f64(r.cx, r.cy, r.fx, r.fy, a.W, a.H, a.rot, st);
    const double G = env_inv_pdf(r.wc, r.sigma, st, a.W, a.H);
    a.out_d[0][i] = w.x; a.out_d[1][i] = w.y; a.out_d[2][i] = w.z;
    a.out_weight[i] = r.valid ? (float) (env_bilinear(r.fx, r.fy, r.v00, r.v10, r.v01, r.v11) * G) : 0.f;
    a.out_pdf[i] = r.valid ? (float) (1.0 / G) : 0.f;
    if (a.out_cell) a.out_cell[i] = r.cy * (a.W - 1u) + r.cx;
    if (a.out_frac[0]) { a.out_frac[0][i] = r.fx; a.out_frac[1][i] = r.fy; }
}

// Emitter::eval (envmap.cpp:323-333, 498-509): the cell of a world direction and the position in it.  In double: a bilinear
// weight is then exact to its last float32 bit, which is what the summation bound of the adjoint's atomics rests on
// (A: hf_envmap_args, or the reflection row's block, which has the same W, H and rot)
template <class A>
__device__ __forceinline__ void env_lookup(const A &a, v3 d, uint32_t &cx, uint32_t &cy, double &fx, double &fy) {
    const auto *R = a.rot; // v = R^T d
    const double vx = (double) R[0] * d.x + (double) R[3] * d.y + (double) R[6] * d.z;
    const double vy = (double) R[1] * d.x + (double) R[4] * d.y + (double) R[7] * d.z;
    const double vz = (double) R[2] * d.x + (double) R[5] * d.y + (double) R[8] * d.z;
    double ux = atan2(vx, -vz) / 6.283185307179586 - 0.5 / (double) (a.W - 1u);
    double uy = acos(fmin(fmax(vy, -1.0), 1.0)) / 3.141592653589793;
    ux -= floor(ux); uy -= floor(uy);
    ux *= (double) (a.W - 1u); uy *= (double) (a.H - 1u);
    // (a NaN direction converts to 0: every index stays in the map)
    cx = min((uint32_t) fmax(ux, 0.0), a.W - 2u); cy = min((uint32_t) fmax(uy, 0.0), a.H - 2u);
    fx = ux - (double) cx; fy = uy - (double) cy;
}
// THE lookup of a world direction, for every kernel that evaluates the map or differentiates the evaluation: the first
// texel's index, the position in the cell and its complements, the four bilinear weights and the four texels (v00, v10,
// v01, v11; TEXELS = false: not read -- the map is linear, its adjoint needs no values), all in double
struct hf_env_texels {
    size_t r0;
    double fx, fy, gx, gy, bw[4], v[4];
    // Emitter::eval, rounded once.  Every radiance a kernel reports is THIS expression: hf_envmap_eval and the
    // reflection rows agree bit for bit because there is no second one
    __device__ __forceinline__ float value() const { return (float) (gy * (gx * v[0] + fx * v[1]) + fy * (gx * v[2] + fx * v[3])); }
};
template <bool TEXELS = true, class A>
__device__ __forceinline__ hf_env_texels env_texels(const A &a, const float *data, v3 d) {
    hf_env_texels e;
    uint32_t cx, cy;
    env_lookup(a, d, cx, cy, e.fx, e.fy);
    e.r0 = (size_t) cy * a.W + cx;
    const size_t r1 = e.r0 + a.W;
    e.gx = 1.0 - e.fx; e.gy = 1.0 - e.fy;
    e.bw[0] = e.gy * e.gx; e.bw[1] = e.gy * e.fx; e.bw[2] = e.fy * e.gx; e.bw[3] = e.fy * e.fx;
    e.v[0] = TEXELS ? (double) data[e.r0] : 0.0; e.v[1] = TEXELS ? (double) data[e.r0 + 1] : 0.0;
    e.v[2] = TEXELS ? (double) data[r1] : 0.0;   e.v[3] = TEXELS ? (double) data[r1 + 1] : 0.0;
    return e;
}
// the texel terms of a derivative, for bilinear weights bw about the texel r0 of a map with W texels per row:
// gdata += q bw (each product rounded once; four float atomics), and sum_j bw_j ddata_j in double
__device__ __forceinline__ void env_scatter4(float *gdata, uint32_t W, size_t r0, const double bw[4], double q) {
    atomicAdd(gdata + r0, (float) (q * bw[0])); atomicAdd(gdata + r0 + 1, (float) (q * bw[1]));
    atomicAdd(gdata + r0 + W, (float) (q * bw[2])); atomicAdd(gdata + r0 + W + 1, (float) (q * bw[3]));
}
__device__ __forceinline__ double env_gather4(const float *ddata, uint32_t W, size_t r0, const double bw[4]) {
    return bw[0] * (double) ddata[r0] + bw[1] * (double) ddata[r0 + 1] + bw[2] * (double) ddata[r0 + W] + bw[3] * (double) ddata[r0 + W + 1];
}
// ADJ = false: out[i] = the bilinear value, rounded once, 0 for an inactive lane;
// ADJ = true: grad_data += grad_out[i] * the bilinear weights (each product rounded once; float atomics)
template <bool ADJ>
__global__ __launch_bounds__(HF_BLOCK) void hf_envmap_eval_kernel(hf_envmap_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const bool act = a.active ? a.active[i] != 0 : true;
    if (!act) {
        if (!ADJ) a.out[i] = 0.f;
        return;
    }
    const hf_env_texels e = env_texels<!ADJ>(a, a.data, mk3(a.d[0][i], a.d[1][i], a.d[2][i]));
    if (!ADJ) a.out[i] = e.value();
    else env_scatter4(a.gdata, a.W, e.r0, e.bw, (double) a.gout[i]);
}

// what the derivative kernels need of direction k of sample i: drawn again, nothing traced
__device__ __forceinline__ hf_env_shade env_shade(const hf_envmap_args &a, uint32_t k, uint32_t id, size_t &r0) {
    float sx, sy;
    sky_sample(a.seed, k, id, sx, sy);
    const hf_env_draw r = env_draw(a.data, a.table, a.W, a.H, sx, sy);
    hf_env_shade s;
    double st;
    s.w = env_dir_f64(r.cx, r.cy, r.fx, r.fy, a.W, a.H, a.rot, st);
    s.G = env_inv_pdf(r.wc, r.sigma, st, a.W, a.H);
    s.L = env_bilinear(r.fx, r.fy, r.v00, r.v10, r.v01, r.v11);
    const double x1 = (double) r.fx, x0 = 1.0 - x1, y1 = (double) r.fy, y0 = 1.0 - y1;
    s.bw[0] = y0 * x0; s.bw[1] = y0 * x1; s.bw[2] = y1 * x0; s.bw[3] = y1 * x1;
    r0 = (size_t) r.cy * a.W + r.cx;
    return s;
}

// Reverse mode of hf_envmap_kernel with respect to sh_n, weight and the texels.  grad_sh_n / grad_weight: sums in k order,
// no atomics; grad_data: one float atomic per texel of every visible direction
__global__ __launch_bounds__(HF_BLOCK) void hf_envmap_adjoint_kernel(hf_envmap_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    v3 sn, g = mk3(0.f, 0.f, 0.f);
    float gw = 0.f;
    if (light_sample(a, i, sn)) {
        const uint32_t bits = a.vis_bits[i], id = light_id(a, i);
        const float c = (a.gimg[i / a.spp] * (1.0f / (float) a.spp)) * a.scale;
        const float cw = a.weight ? c * a.weight[i] : c;
        double sx = 0.0, sy = 0.0, sz = 0.0, sc = 0.0;
        for (uint32_t k = 0; k < a.num_rays; ++k) {
            if ((bits >> k) & 1u) {
                size_t r0;
                const hf_env_shade s = env_shade(a, k, id, r0);
                const double E = s.L * s.G, co = sky_dot_f64(sn, s.w);
                sx += s.w.x * E; sy += s.w.y * E; sz += s.w.z * E;
                sc += co * E;
                if (a.gdata) env_scatter4(a.gdata, a.W, r0, s.bw, (double) cw * (co * s.G));
            }
        }
        g = mk3((float) sx, (float) sy, (float) sz) * cw;
        gw = c * (float) sc;
    }
    a.gn[0][i] = g.x; a.gn[1][i] = g.y; a.gn[2][i] = g.z;
    if (a.gw) a.gw[i] = gw;
}

// forward mode: the tangent of sample i's value for tangents dn of sh_n, dw of weight and ddata of the texels (NULL: zero)
__device__ __forceinline__ float envmap_tangent_value(const hf_envmap_args &a, size_t i) {
    v3 sn;
    if (!light_sample(a, i, sn)) return 0.f;
    const uint32_t bits = a.vis_bits[i], id = light_id(a, i);
    const v3 dn = a.dn[0] ? mk3(a.dn[0][i], a.dn[1][i], a.dn[2][i]) : mk3(0.f, 0.f, 0.f);
    double sd = 0.0, sc = 0.0;
    for (uint32_t k = 0; k < a.num_rays; ++k) {
        if ((bits >> k) & 1u) {
            size_t r0;
            const hf_env_shade s = env_shade(a, k, id, r0);
            const double co = sky_dot_f64(sn, s.w);
            const double dL = a.ddata ? env_gather4(a.ddata, a.W, r0, s.bw) : 0.0;
            sd += (sky_dot_f64(dn, s.w) * s.L + co * dL) * s.G;
            sc += co * (s.L * s.G);
        }
    }
    return (float) ((double) a.scale * ((double) (a.weight ? a.weight[i] : 1.f) * sd + (double) (a.dw ? a.dw[i] : 0.f) * sc));
}
template <bool PIXEL>
__global__ __launch_bounds__(HF_BLOCK) void hf_envmap_tangent_kernel(hf_envmap_args a) {
    light_tangent_image<PIXEL, hf_envmap_args, envmap_tangent_value>(a, nullptr);
}

void hf_launch_envmap(int mode, const hf_envmap_args &a, hipStream_t stream) {
    if (mode <= 3) {
        launch_light(mode, a, 1u, stream, hf_envmap_kernel, hf_envmap_adjoint_kernel, hf_envmap_tangent_kernel<false>,
                     hf_envmap_tangent_kernel<true>, hf_envmap_rays_kernel);
    } else if (a.n != 0) {
        const dim3 grid((unsigned) ((a.n + HF_BLOCK - 1) / HF_BLOCK)), block(HF_BLOCK);
        hipLaunchKernelGGL(mode == 4 ? hf_envmap_sample_kernel : mode == 5 ? hf_envmap_eval_kernel<false> : hf_envmap_eval_kernel<true>,
                           grid, block, 0, stream, a);
    }
}

// ---------------------------------------------------------------------------------
// Specular reflection of the environment map (include/hf.h hf_reflect_*): every wavefront sample is mirrored at its
// shading normal (reflect(wi, m), fresnel.h:282-284; the `dielectric` reflection lobe, or an ideal mirror for eta = 0),
// the reflected ray is walked (any hit, per lane, maxt = +inf) and what escapes looks the map up (Emitter::eval of
// envmap.cpp: env_texels above, in double, the expression hf_envmap_eval_kernel rounds).  ONE launch, one lane per
// sample; nothing of the ray goes to memory.  A reflected ray that hits the terrain contributes 0: no second vertex.
// The row's own text is its vertex and the direction derivative of the lookup; the ray store, the adjoint's seed and
// outputs, the texel terms, the tangent film and the launch are the lighting rows' shared functions.
// ---------------------------------------------------------------------------------
// The specular vertex of one sample, the same text for the fused kernel, the rays kernel and the two derivatives:
// fresnel() as caustic_vertex has it (c > 0 on every lane that is used: the outside branch) and reflect().
//   dF = d F / d c (a_s a_s' + a_p a_p'; 0 for eta = 0, eta = 1 and under total internal reflection, where F = 1)
struct hf_reflect_vertex {
    v3 wi, wr;
    float c, F, dF;
};
template <class P>
__device__ __forceinline__ hf_reflect_vertex reflect_vertex(P a, v3 m, v3 d) {
    hf_reflect_vertex v;
    v.wi = mk3(-d.x, -d.y, -d.z);
    const float ci = dot3(m, v.wi);
    v.c = ci;
    const float eta = a->eta, rcp_eta = a->rcp_eta;
    const bool outside = ci >= 0.f;
    const float eta_it = outside ? eta : rcp_eta, eta_ti = outside ? rcp_eta : eta;
    const float e2 = eta_ti * eta_ti;
    const float ct2 = __builtin_fmaf(-__builtin_fmaf(-ci, ci, 1.f), e2, 1.f);
    const float cia = __builtin_fabsf(ci), cta = __builtin_sqrtf(fmaxf(ct2, 0.f));
    const float ns = __builtin_fmaf(-eta_it, cta, cia), ds = __builtin_fmaf(eta_it, cta, cia);
    const float np = __builtin_fmaf(-eta_it, cia, cta), dp = __builtin_fmaf(eta_it, cia, cta);
    const float a_s = ns / ds, a_p = np / dp;
    const bool mirror = eta == 0.f, matched = eta == 1.f;
    v.F = mirror ? 1.f : matched ? 0.f : 0.5f * (a_s * a_s + a_p * a_p);
    const float sg = outside ? 1.f : -1.f, dcta = ci * e2 / cta;
    const float das = 2.f * ((eta_it * cta) * sg - cia * (eta_it * dcta)) / (ds * ds);
    const float dap = 2.f * ((eta_it * cia) * dcta - cta * (eta_it * sg)) / (dp * dp);
    v.dF = (mirror || matched || !(ct2 > 0.f)) ? 0.f : a_s * das + a_p * dap;
    const float c2 = 2.f * ci; // reflect(wi, m) = fmsub(m, 2 <wi, m>, wi)
    v.wr = mk3(__builtin_fmaf(m.x, c2, -v.wi.x), __builtin_fmaf(m.y, c2, -v.wi.y), __builtin_fmaf(m.z, c2, -v.wi.z));
    return v;
}
// eligible (active, a finite t, both normals face the viewer) and consistent (the mirror ray leaves the true surface)
__device__ __forceinline__ bool reflect_traced(const hf_reflect_vertex &v, v3 g, float t, bool act) {
    return act && (__builtin_fabsf(t) < __builtin_inff()) && (v.c > 0.f) && (dot3(g, v.wi) > 0.f) && (dot3(g, v.wr) > 0.f);
}
// the vertex of sample i from the rows
template <class P>
__device__ __forceinline__ hf_reflect_vertex reflect_sample(P a, size_t i, v3 &m) {
    m = mk3(a->sh_n[0][i], a->sh_n[1][i], a->sh_n[2][i]);
    return reflect_vertex(a, m, mk3(a->d[0][i], a->d[1][i], a->d[2][i]));
}
// what the derivative kernels need of the lookup beyond env_texels (the radiance e.value(), the bilinear weights, the
// first texel's index): G = R dL/dv, the derivative of the radiance with respect to the world direction with the cell
// held (exactly 0 at the poles of the map); formed in double from the same lookup `e` of w, each component rounded once
__device__ __forceinline__ v3 reflect_shade(const hf_reflect_args &a, const hf_env_texels &e, v3 w) {
    const double fx = e.fx, fy = e.fy, gx = e.gx, gy = e.gy, v00 = e.v[0], v10 = e.v[1], v01 = e.v[2], v11 = e.v[3];
    const float *R = a.rot;
    const double vx = (double) R[0] * w.x + (double) R[3] * w.y + (double) R[6] * w.z;
    const double vy = (double) R[1] * w.x + (double) R[4] * w.y + (double) R[7] * w.z;
    const double vz = (double) R[2] * w.x + (double) R[5] * w.y + (double) R[8] * w.z;
    const double s2 = vx * vx + vz * vz, q = 1.0 - vy * vy;
    double lx = 0.0, ly = 0.0, lz = 0.0;
    if (!(s2 < 1e-12) && !(q < 1e-12)) {
        const double Lx = gy * (v10 - v00) + fy * (v11 - v01), Ly = gx * (v01 - v00) + fx * (v11 - v10);
        const double kx = Lx * (double) (a.W - 1u) / 6.283185307179586 / s2;
        lx = -(kx * vz); lz = kx * vx;
        ly = -(Ly * (double) (a.H - 1u) / 3.141592653589793 / sqrt(q));
    }
    return mk3((float) ((double) R[0] * lx + (double) R[1] * ly + (double) R[2] * lz),
               (float) ((double) R[3] * lx + (double) R[4] * ly + (double) R[5] * lz),
               (float) ((double) R[6] * lx + (double) R[7] * ly + (double) R[8] * lz));
}

typedef const __attribute__((address_space(4))) hf_reflect_args *hf_reflect_kargs;

#ifndef HF_REFLECT_WAVES
#define HF_REFLECT_WAVES 6 // resident waves per SIMD (the siblings')
#endif
__global__ __launch_bounds__(HF_BLOCK, HF_REFLECT_WAVES) void hf_reflect_kernel(hf_reflect_args a) {
    const hf_dev_field &f = a.f;
    // hf_sky_kernel's mapping: n < 2^32, the sample index is one register across the walk
    const size_t i64 = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const bool in = i64 < a.n;
    const uint32_t i = (uint32_t) i64;
    const uint32_t ii = in ? i : (uint32_t) (a.n - 1);
    hf_reflect_kargs ka = (hf_reflect_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    v3 wr;
    float F;
    bool traced;
    hf_hit best;
    best.hit = false;
    {
        v3 m;
        const hf_reflect_vertex v = reflect_sample(ka, ii, m);
        const v3 gn = mk3(ka->nrm[0][ii], ka->nrm[1][ii], ka->nrm[2][ii]);
        const uint8_t *active = ka->active;
        traced = reflect_traced(v, gn, ka->t[ii], in && (active ? active[ii] != 0 : true));
        wr = v.wr; F = v.F;
        if (__ballot(traced) != 0ull) { // wave-uniform: a batch without a traced sample walks nothing
            const v3 p = mk3(ka->p[0][ii], ka->p[1][ii], ka->p[2][ii]);
            // the direction, F and the index are held across the walk
            light_walk<true>(&ka->f, f, sky_origin(p, gn, sky_offset(p), wr), wr, traced, best);
        }
    }
    // (the map and the output pointers: loaded here, not before the walk; the lookup in double runs when the walk's
    // state is dead)
    hf_reflect_kargs ko = (hf_reflect_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ko));
    const bool lit = traced && !best.hit; // (traced: in range)
    float val = 0.f;
    if (lit) {
        const float *weight = ko->weight;
        const float L = env_texels(*ko, ko->data, wr).value();
        val = (weight ? weight[i] * F : F) * L;
    }
    if (in) {
        float *value = ko->value;
        uint8_t *vis = ko->vis;
        if (value) value[i] = val;
        if (vis) vis[i] = lit ? 1 : 0;
    }
    float *image = ko->image;
    if (image) {
        const uint32_t spp = ko->spp, g = spp < 64u ? spp : 64u;
        film_pixel(image, val, 0u, ko->n / spp, i, spp, in, (spp & (spp - 1u)) == 0u, g, 1.0f / (float) spp, i);
    }
}

// the reflected ray of every sample, materialised: what hf_reflect_kernel walks, bit for bit (maxt = -1 and a zero
// origin and direction: the fused kernel does not trace the lane)
__global__ __launch_bounds__(HF_BLOCK) void hf_reflect_rays_kernel(hf_reflect_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    v3 m;
    const hf_reflect_vertex v = reflect_sample(&a, i, m);
    const v3 gn = mk3(a.nrm[0][i], a.nrm[1][i], a.nrm[2][i]), p = mk3(a.p[0][i], a.p[1][i], a.p[2][i]);
    light_store_spawned(a, i, p, gn, v.wr, reflect_traced(v, gn, a.t[i], a.active ? a.active[i] != 0 : true));
}

// Reverse mode of hf_reflect_kernel with respect to sh_n, weight and the texels: nothing is traced, the vertex is
// formed again and the visibility byte read.  grad_sh_n, grad_weight: one lane per sample, overwritten, no atomics;
// grad_data: one float atomic per texel of every visible sample
__global__ __launch_bounds__(HF_BLOCK) void hf_reflect_adjoint_kernel(hf_reflect_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    v3 gm = mk3(0.f, 0.f, 0.f);
    float gw = 0.f;
    if (a.vis[i]) {
        v3 m;
        const hf_reflect_vertex v = reflect_sample(&a, i, m);
        const hf_env_texels e = env_texels(a, a.data, v.wr);
        const float L = e.value();
        const v3 G = reflect_shade(a, e, v.wr);
        const float g = light_value_seed(a, i);
        const float gwt = a.weight ? g * a.weight[i] : g;
        gw = g * (v.F * L);
        const float k = __builtin_fmaf(v.dF, L, (2.f * v.F) * dot3(m, G));
        gm = fma3(v.wi, k, G * ((2.f * v.F) * v.c)) * gwt;
        if (a.gdata) env_scatter4(a.gdata, a.W, e.r0, e.bw, (double) (gwt * v.F));
    }
    light_store_grads(a, i, gm, gw);
}

// forward mode, the transpose of the above: the tangent of sample i's value for tangents dn of sh_n, dw of weight and
// ddata of the texels (NULL: zero)
__device__ __forceinline__ float reflect_tangent_value(const hf_reflect_args &a, size_t i) {
    if (!a.vis[i]) return 0.f;
    v3 m;
    const hf_reflect_vertex v = reflect_sample(&a, i, m);
    const hf_env_texels e = env_texels(a, a.data, v.wr);
    const float L = e.value();
    const v3 G = reflect_shade(a, e, v.wr);
    const v3 dm = a.dn[0] ? mk3(a.dn[0][i], a.dn[1][i], a.dn[2][i]) : mk3(0.f, 0.f, 0.f);
    const float w = a.weight ? a.weight[i] : 1.f, dw = a.dw ? a.dw[i] : 0.f;
    const float dci = dot3(dm, v.wi);
    const float k = __builtin_fmaf(v.dF, L, (2.f * v.F) * dot3(m, G));
    float dv = __builtin_fmaf(k, dci, ((2.f * v.F) * v.c) * dot3(G, dm));
    if (a.ddata) dv += v.F * (float) env_gather4(a.ddata, a.W, e.r0, e.bw);
    return __builtin_fmaf(dw, v.F * L, w * dv);
}
// (the per-sample tangent is written too, and the image may be NULL)
template <bool PIXEL>
__global__ __launch_bounds__(HF_BLOCK) void hf_reflect_tangent_kernel(hf_reflect_args a) {
    light_tangent_image<PIXEL, hf_reflect_args, reflect_tangent_value>(a, a.value);
}

// mode 0: forward, 1: adjoint, 2: tangent, 3: rays
void hf_launch_reflect(int mode, const hf_reflect_args &a, hipStream_t stream) {
    launch_light(mode, a, 1u, stream, hf_reflect_kernel, hf_reflect_adjoint_kernel, hf_reflect_tangent_kernel<false>,
                 hf_reflect_tangent_kernel<true>, hf_reflect_rays_kernel);
}

// ---------------------------------------------------------------------------------
// Glossy reflection of the environment map (include/hf.h hf_glossy_*): the reflection lobe of a rough conductor or
// dielectric (roughconductor.cpp:242-268) with an isotropic GGX distribution sampled by its visible normals
// (microfacet.h:297-319, 405-420).  Every wavefront sample draws K = num_rays microfacet normals from the TEA stream,
// mirrors wi at each (reflect_vertex with the microfacet normal in the place of the shading normal), walks the mirror
// ray (any hit, per lane, maxt = +inf) and, where it escapes, looks the map up in double.  ONE launch, one lane per
// sample, `k` a scalar loop with the lanes predicated; nothing of a ray goes to memory.  The row's own text is its draw
// (glossy_draw, glossy_smith) and the derivative of its sums (glossy_sums); the lookup and everything around the
// kernels are the shared functions the reflect row uses.
// ---------------------------------------------------------------------------------
// Draw k of one sample, the same text for the fused kernel, the rays kernel and the two derivatives: the microfacet
// normal h (world), the mirror direction wo, the cosines <wi, h>, <n, h>, <n, wo>, F and whether the draw is valid
struct hf_glossy_draw {
    v3 h, wo;
    float cwh, ch, co, F;
    bool valid;
};
template <class P>
__device__ __forceinline__ hf_glossy_draw glossy_draw(P a, v3 n, v3 d, float al, uint32_t k, uint32_t id) {
    hf_glossy_draw g;
    v3 s, t;
    coordinate_system(n, s, t);
    const v3 wi = mk3(-d.x, -d.y, -d.z);
    const v3 wl = mk3(dot3(wi, s), dot3(wi, t), dot3(wi, n));
    // step 1: stretch wi (microfacet.h:301-305)
    const v3 wp = normalize3(mk3(al * wl.x, al * wl.y, wl.z));
    // Frame3f::sincos_phi (frame.h:111-122); Epsilon = 2^-24
    const float st2 = __builtin_fmaf(wp.x, wp.x, wp.y * wp.y), ist = rsqrt_ieee(st2); // Frame3f::sin_theta_2
    const bool pole = __builtin_fabsf(st2) <= 2.384185791015625e-07f;
    const float cphi = pole ? 1.f : fminf(fmaxf(wp.x * ist, -1.f), 1.f), sphi = pole ? 0.f : fminf(fmaxf(wp.y * ist, -1.f), 1.f);
    const float ct = wp.z;
    // step 2: sample_visible_11, the GGX branch (microfacet.h:405-420), on the disk of bounce_local
    const v3 q = bounce_disk(a->seed, k, id);
    const float sh = 0.5f * (1.f + ct);
    const float e = __builtin_sqrtf(fmaxf(__builtin_fmaf(-q.x, q.x, 1.f), 0.f));
    const float x = q.x, y = __builtin_fmaf(q.y, sh, __builtin_fmaf(-e, sh, e)); // lerp(e, p.y, s)
    const float z = __builtin_sqrtf(fmaxf(1.f - __builtin_fmaf(y, y, x * x), 0.f));
    const float si = __builtin_sqrtf(fmaxf(__builtin_fmaf(-ct, ct, 1.f), 0.f));
    const float nr = rcp_ieee(__builtin_fmaf(si, y, ct * z));
    const float slx = __builtin_fmaf(ct, y, -(si * z)) * nr, sly = x * nr;
    // step 3: rotate and unstretch; step 4: the normal
    const float rx = __builtin_fmaf(cphi, slx, -(sphi * sly)) * al, ry = __builtin_fmaf(sphi, slx, cphi * sly) * al;
    const v3 hl = normalize3(mk3(-rx, -ry, 1.f));
    g.h = fma3(n, hl.z, fma3(t, hl.y, s * hl.x)); // Frame3f(n).to_world, as bounce_world
    const hf_reflect_vertex v = reflect_vertex(a, g.h, d); // fresnel(<wi, h>, eta) and reflect(wi, h)
    g.cwh = v.c; g.wo = v.wr; g.F = v.F;
    const float inf = __builtin_inff();
    g.valid = (__builtin_fabsf(g.h.x) < inf) && (__builtin_fabsf(g.h.y) < inf) && (__builtin_fabsf(g.h.z) < inf) && (v.c > 0.f);
    g.ch = dot3(n, g.h); g.co = dot3(n, g.wo);
    return g;
}
// smith_g1 (microfacet.h:341-365) of a unit vector with cosine c to the normal, frame-free, and its derivatives:
//   T = a^2 max(1 - c^2, 0) / c^2,  G1 = 2 / (1 + sqrt(1 + T)),  dG1/dT = -1 / ((1 + r)^2 r),  dT/dc = -2 a^2 / c^3
struct hf_glossy_smith { float G, dc, da; }; // G1, dG1 / dc, dG1 / da
__device__ __forceinline__ hf_glossy_smith glossy_smith(float al, float c) {
    hf_glossy_smith s;
    const float a2 = al * al, m = fmaxf(__builtin_fmaf(-c, c, 1.f), 0.f), c2 = c * c;
    const float T = a2 * m / c2, r = __builtin_sqrtf(1.f + T), q = 1.f + r;
    s.G = 2.f / q;
    const float dT = -1.f / ((q * q) * r);
    s.dc = dT * (-2.f * a2 / (c2 * c));
    s.da = dT * (2.f * al * m / c2);
    return s;
}
// the rows of sample i that every kernel of the row reads: n, d and the roughness a = max(alpha, 1e-4)
template <class P>
__device__ __forceinline__ float glossy_sample(P a, size_t i, v3 &n, v3 &d) {
    n = mk3(a->sh_n[0][i], a->sh_n[1][i], a->sh_n[2][i]);
    d = mk3(a->d[0][i], a->d[1][i], a->d[2][i]);
    return a->alpha[i];
}
// eligible: active, a finite t, a finite roughness, both normals face the viewer
__device__ __forceinline__ bool glossy_eligible(v3 n, v3 g, v3 d, float t, float alpha, bool act) {
    const float inf = __builtin_inff();
    return act && (__builtin_fabsf(t) < inf) && (__builtin_fabsf(alpha) < inf) && (-dot3(n, d) > 0.f) && (-dot3(g, d) > 0.f);
}

typedef const __attribute__((address_space(4))) hf_glossy_args *hf_glossy_kargs;

#ifndef HF_GLOSSY_WAVES
#define HF_GLOSSY_WAVES 5 // resident waves per SIMD (96 VGPRs; why not six: profiles/glossy/registers.txt)
#endif
__global__ __launch_bounds__(HF_BLOCK, HF_GLOSSY_WAVES) void hf_glossy_kernel(hf_glossy_args a) {
    const hf_dev_field &f = a.f;
    // hf_sky_kernel's mapping: n < 2^32, the sample index is one register across the walk
    const size_t i64 = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const bool in = i64 < a.n;
    const uint32_t i = (uint32_t) i64;
    const uint32_t ii = in ? i : (uint32_t) (a.n - 1);
    bool elig;
    {
        v3 sn, d;
        const float al = glossy_sample(&a, ii, sn, d);
        const v3 gn = mk3(a.nrm[0][ii], a.nrm[1][ii], a.nrm[2][ii]);
        elig = glossy_eligible(sn, gn, d, a.t[ii], al, in && (a.active ? a.active[ii] != 0 : true));
    }
    // Two loops over the directions.  The first draws and walks and keeps only the bit; the second, when every walk is
    // over, forms the draws of the set bits again (the same device function: the same bits) and looks the map up in
    // double.  With the lookup inside the walk's loop its atan2 / acos polynomials' constants, sixty registers, are
    // hoisted in front of the loop and held across every walk (profiles/glossy/registers.txt).
    // In both loops the sample's record is read again per direction (the index goes through an opaque statement, so the
    // loads stay in the loop; they hit the cache): thirteen registers that are then not held across the walk.
    uint32_t bits = 0u; // bit k: direction k was traced and is unoccluded
    if (__ballot(elig) != 0ull) { // wave-uniform: a batch without an eligible sample draws nothing
        hf_glossy_kargs ka = (hf_glossy_kargs) __builtin_amdgcn_kernarg_segment_ptr();
#pragma unroll 1
        for (uint32_t k = 0;; ++k) { // wave-uniform loop, the lanes predicated inside
            asm volatile("" : "+s"(ka)); // opaque per direction: the kernarg loads stay inside the loop
            v3 wo, o;
            bool traced;
            {
                uint32_t ix = ii;
                asm volatile("" : "+v"(ix));
                v3 sn, d;
                const float al = fmaxf(glossy_sample(ka, ix, sn, d), 1e-4f);
                const v3 gn = mk3(ka->nrm[0][ix], ka->nrm[1][ix], ka->nrm[2][ix]);
                const uint32_t *ray_id = ka->ray_id;
                const hf_glossy_draw g = glossy_draw(ka, sn, d, al, k, ray_id ? ray_id[ix] : ix);
                traced = elig && g.valid && (g.co > 0.f) && (dot3(gn, g.wo) > 0.f);
                wo = g.wo;
                const v3 p = mk3(ka->p[0][ix], ka->p[1][ix], ka->p[2][ix]);
                o = sky_origin(p, gn, sky_offset(p), wo);
            }
            hf_hit best;
            light_walk<true>(&ka->f, f, o, wo, traced, best);
            if (traced && !best.hit) bits |= 1u << k;
            if (k + 1u >= ka->num_rays) break;
        }
    }
    // (the map and the output pointers: loaded here, not before the walks)
    hf_glossy_kargs ko = (hf_glossy_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ko));
    float acc = 0.f; // sum over the visible directions of F G1(c_o) L, in k order
    if (__ballot(bits != 0u) != 0ull) { // wave-uniform: on lit lanes only
#pragma unroll 1
        for (uint32_t k = 0; k < ko->num_rays; ++k) {
            asm volatile("" : "+s"(ko));
            if ((bits >> k) & 1u) {
                uint32_t ix = ii;
                asm volatile("" : "+v"(ix));
                v3 sn, d;
                const float al = fmaxf(glossy_sample(ko, ix, sn, d), 1e-4f);
                const uint32_t *ray_id = ko->ray_id;
                const hf_glossy_draw g = glossy_draw(ko, sn, d, al, k, ray_id ? ray_id[ix] : ix);
                acc += (g.F * glossy_smith(al, g.co).G) * env_texels(*ko, ko->data, g.wo).value();
            }
        }
    }
    float val = 0.f;
    if (bits != 0u) { // (a set bit: eligible, in range)
        const float *weight = ko->weight;
        val = ko->inv_k * acc;
        if (weight) val *= weight[i];
    }
    if (in) {
        float *value = ko->value;
        uint32_t *vis_bits = ko->vis_bits;
        if (value) value[i] = val;
        if (vis_bits) vis_bits[i] = bits;
    }
    float *image = ko->image;
    if (image) {
        const uint32_t spp = ko->spp, g = spp < 64u ? spp : 64u;
        film_pixel(image, val, 0u, ko->n / spp, i, spp, in, (spp & (spp - 1u)) == 0u, g, 1.0f / (float) spp, i);
    }
}

// mirror ray a.k of every sample, materialised: what hf_glossy_kernel walks for that direction, bit for bit (maxt = -1
// and a zero origin and direction: the fused kernel does not trace the lane); out_h: the microfacet normal, zero for an
// invalid draw or a sample that is not eligible
__global__ __launch_bounds__(HF_BLOCK) void hf_glossy_rays_kernel(hf_glossy_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    v3 sn, d;
    const float al = glossy_sample(&a, i, sn, d);
    const v3 gn = mk3(a.nrm[0][i], a.nrm[1][i], a.nrm[2][i]), p = mk3(a.p[0][i], a.p[1][i], a.p[2][i]);
    const bool elig = glossy_eligible(sn, gn, d, a.t[i], al, a.active ? a.active[i] != 0 : true);
    const hf_glossy_draw g = glossy_draw(&a, sn, d, fmaxf(al, 1e-4f), a.k, light_id(a, i));
    light_store_spawned(a, i, p, gn, g.wo, elig && g.valid && (g.co > 0.f) && (dot3(gn, g.wo) > 0.f));
    if (a.out_h[0]) {
        const v3 h = (elig && g.valid) ? g.h : mk3(0.f, 0.f, 0.f);
        a.out_h[0][i] = h.x; a.out_h[1][i] = h.y; a.out_h[2][i] = h.z;
    }
}

// The derivative of one sample with the draws held (include/hf.h): with S = sum_k F G1(c_o) L over the set bits,
//   value = weight / K S,   d value = d weight S / K + weight / K (<N, dn> + A da + sum_k F G1(c_o) sum_j b_j ddata_j).
// VISIT(F G1(c_o), lookup) is called per set bit (the texel terms of the adjoint and the tangent)
struct hf_glossy_sums { v3 N; float A, S; };
template <class V>
__device__ __forceinline__ hf_glossy_sums glossy_sums(const hf_glossy_args &a, size_t i, uint32_t bits, V visit) {
    hf_glossy_sums r;
    r.N = mk3(0.f, 0.f, 0.f); r.A = 0.f; r.S = 0.f;
    v3 sn, d;
    const float al = fmaxf(glossy_sample(&a, i, sn, d), 1e-4f);
    const uint32_t id = light_id(a, i);
    const v3 wi = mk3(-d.x, -d.y, -d.z);
    const float ci = dot3(sn, wi);
    const hf_glossy_smith gi = glossy_smith(al, ci);
    const float a2m1 = __builtin_fmaf(al, al, -1.f);
    const float ki = gi.dc / gi.G - 1.f / ci, kia = gi.da / gi.G; // d ln (G1(c_i) / c_i)
    for (uint32_t k = 0; k < a.num_rays; ++k) {
        if (!((bits >> k) & 1u)) continue;
        const hf_glossy_draw g = glossy_draw(&a, sn, d, al, k, id);
        const hf_glossy_smith go = glossy_smith(al, g.co);
        const hf_env_texels e = env_texels(a, a.data, g.wo);
        const float L = e.value();
        const float q = __builtin_fmaf(g.ch * g.ch, a2m1, 1.f);
        const float dDc = -4.f * g.ch * a2m1 / q, dDa = 2.f / al - 4.f * (g.ch * g.ch) * al / q; // d ln D
        const float FL = g.F * L;
        // L (G1(c_o) d ln A + d G1(c_o))
        r.N = fma3(g.wo, FL * go.dc, fma3(wi, (FL * go.G) * ki, fma3(g.h, (FL * go.G) * dDc, r.N)));
        r.A += FL * __builtin_fmaf(go.G, dDa + kia, go.da);
        r.S += g.F * go.G * L;
        visit(g.F * go.G, e);
    }
    return r;
}

// Reverse mode of hf_glossy_kernel with respect to sh_n, weight, alpha and the texels: nothing is traced, the draws
// are formed again and the visibility word read.  grad_sh_n, grad_weight, grad_alpha: one lane per sample, sums in k
// order, overwritten, no atomics; grad_data: one float atomic per texel of every set bit
__global__ __launch_bounds__(HF_BLOCK) void hf_glossy_adjoint_kernel(hf_glossy_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    v3 gm = mk3(0.f, 0.f, 0.f);
    float gw = 0.f, ga = 0.f;
    const uint32_t bits = a.vis_bits[i];
    if (bits != 0u) {
        const float g = light_value_seed(a, i);
        const float gk = (a.weight ? g * a.weight[i] : g) * a.inv_k;
        const hf_glossy_sums r = glossy_sums(a, i, bits, [&](float fg, const hf_env_texels &e) {
            if (a.gdata) env_scatter4(a.gdata, a.W, e.r0, e.bw, (double) (gk * fg));
        });
        gm = r.N * gk;
        ga = a.alpha[i] > 1e-4f ? r.A * gk : 0.f;
        gw = (g * a.inv_k) * r.S;
    }
    light_store_grads(a, i, gm, gw);
    if (a.ga) a.ga[i] = ga;
}

// forward mode, the transpose of the above: the tangent of sample i's value for tangents dn of sh_n, dw of weight, da of
// alpha and ddata of the texels (NULL: zero)
__device__ __forceinline__ float glossy_tangent_value(const hf_glossy_args &a, size_t i) {
    const uint32_t bits = a.vis_bits[i];
    if (bits == 0u) return 0.f;
    float dt = 0.f; // sum_k F G1(c_o) sum_j b_j ddata_j
    const hf_glossy_sums r = glossy_sums(a, i, bits, [&](float fg, const hf_env_texels &e) {
        if (a.ddata) dt += fg * (float) env_gather4(a.ddata, a.W, e.r0, e.bw);
    });
    const v3 dn = a.dn[0] ? mk3(a.dn[0][i], a.dn[1][i], a.dn[2][i]) : mk3(0.f, 0.f, 0.f);
    const float w = a.weight ? a.weight[i] : 1.f, dw = a.dw ? a.dw[i] : 0.f;
    const float da = (a.da && a.alpha[i] > 1e-4f) ? a.da[i] : 0.f;
    const float dv = __builtin_fmaf(r.A, da, dot3(r.N, dn)) + dt;
    return __builtin_fmaf(dw * a.inv_k, r.S, (w * a.inv_k) * dv);
}
// (the per-sample tangent is written too, and the image may be NULL)
template <bool PIXEL>
__global__ __launch_bounds__(HF_BLOCK) void hf_glossy_tangent_kernel(hf_glossy_args a) {
    light_tangent_image<PIXEL, hf_glossy_args, glossy_tangent_value>(a, a.value);
}

// mode 0: forward, 1: adjoint, 2: tangent, 3: rays
void hf_launch_glossy(int mode, const hf_glossy_args &a, hipStream_t stream) {
    launch_light(mode, a, 1u, stream, hf_glossy_kernel, hf_glossy_adjoint_kernel, hf_glossy_tangent_kernel<false>,
                 hf_glossy_tangent_kernel<true>, hf_glossy_rays_kernel);
}

// ---------------------------------------------------------------------------------
// The refraction view (include/hf.h hf_refract_*, hf_bitmap_*): the camera side of transmission.  Every wavefront
// sample looks along d, is refracted at its shading normal (caustic_vertex: the vertex, the masks, the ray and the
// landing are the caustic row's, function for function), walked up to the receiver (any hit, per lane, maxt = s) and
// sees the receiver's bitmap texture (bitmap.cpp:400, 497-520) through an absorbing medium:
//   value = ((weight (1 - F)) eta_ti^2) exp(-sigma_t s) L(pos)   (dielectric.cpp:358-363, radiance mode).
// ONE launch, one lane per sample, hf_reflect_kernel's shape: the lookup runs after the walk.  The row's own text is
// the texture lookup and the value's derivative; the vertex and the landing's derivatives are the caustic row's, the
// seed, the outputs, the tangent film and the launch the lighting rows' shared functions.
// ---------------------------------------------------------------------------------
// One axis of the lookup in float32: q = pos - 0.5, i0 = floor(q), f = q - i0, the texels wrap(i0) and wrap(i0 + 1).
// A coordinate that is not finite or beyond 2^23 (its floor is no int32, its fraction no fraction): under clamp the
// border texel q is nearest to with f = 0 -- what a float clamp of q to [-1, res] reads; under repeat nothing (false)
__device__ __forceinline__ uint32_t bitmap_wrap(int32_t i, uint32_t res, bool repeat) {
    if (repeat) {
        const int32_t r = i % (int32_t) res;
        return (uint32_t) (r < 0 ? r + (int32_t) res : r);
    }
    return (uint32_t) min(max(i, 0), (int32_t) res - 1);
}
__device__ __forceinline__ bool bitmap_axis(float pos, uint32_t res, bool repeat, uint32_t &i0, uint32_t &i1, float &f) {
    const float q = pos - 0.5f;
    if (!(__builtin_fabsf(q) < 8388608.f)) {
        i0 = i1 = (!repeat && q > 0.f) ? res - 1u : 0u;
        f = 0.f;
        return !repeat;
    }
    const float fl = __builtin_floorf(q);
    f = q - fl;
    i0 = bitmap_wrap((int32_t) fl, res, repeat);
    i1 = bitmap_wrap((int32_t) fl + 1, res, repeat);
    return true;
}
// THE lookup of a film position, for every kernel that evaluates the texture or differentiates the evaluation: the
// offsets of the texels v00, v10, v01, v11, the position in the cell, and whether anything is read at all
// (P: a pointer to hf_refract_args or hf_bitmap_args)
struct hf_bitmap_cell {
    size_t j[4];
    float fx, fy;
    bool ok;
    // Texture::eval_1 (bitmap.cpp:497-520).  Every radiance a kernel reports is THIS expression; linear in the texels
    __device__ __forceinline__ float value(const float *tex) const {
        const float gx = 1.f - fx, gy = 1.f - fy;
        const float v0 = __builtin_fmaf(gx, tex[j[0]], fx * tex[j[1]]), v1 = __builtin_fmaf(gx, tex[j[2]], fx * tex[j[3]]);
        return ok ? __builtin_fmaf(gy, v0, fy * v1) : 0.f;
    }
    // (Lx, Ly) = dL/dpos with the cell held
    __device__ __forceinline__ void slopes(const float *tex, float &Lx, float &Ly) const {
        const float v00 = tex[j[0]], v10 = tex[j[1]], v01 = tex[j[2]], v11 = tex[j[3]];
        Lx = ok ? (1.f - fy) * (v10 - v00) + fy * (v11 - v01) : 0.f;
        Ly = ok ? (1.f - fx) * (v01 - v00) + fx * (v11 - v10) : 0.f;
    }
    // gtex += q b_j: four float atomics
    __device__ __forceinline__ void scatter(float *gtex, float q) const {
        if (!ok) return;
        const float gx = 1.f - fx, gy = 1.f - fy;
        atomicAdd(gtex + j[0], q * (gy * gx)); atomicAdd(gtex + j[1], q * (gy * fx));
        atomicAdd(gtex + j[2], q * (fy * gx)); atomicAdd(gtex + j[3], q * (fy * fx));
    }
};
template <class P>
__device__ __forceinline__ hf_bitmap_cell bitmap_cell(P a, float x, float y) {
    hf_bitmap_cell e;
    const uint32_t TW = a->TW, TH = a->TH;
    const bool repeat = a->wrap == HF_WRAP_REPEAT;
    uint32_t x0, x1, y0, y1;
    const bool okx = bitmap_axis(x, TW, repeat, x0, x1, e.fx), oky = bitmap_axis(y, TH, repeat, y0, y1, e.fy);
    e.ok = okx && oky;
    e.j[0] = (size_t) y0 * TW + x0; e.j[1] = (size_t) y0 * TW + x1;
    e.j[2] = (size_t) y1 * TW + x0; e.j[3] = (size_t) y1 * TW + x1;
    return e;
}
// ADJ = false: out[i] = L, out_grad = (Lx, Ly), zeros for an inactive lane;
// ADJ = true: grad_pos = grad_out[i] (Lx, Ly) overwritten, grad_tex += grad_out[i] b_j (float atomics)
template <bool ADJ>
__global__ __launch_bounds__(HF_BLOCK) void hf_bitmap_eval_kernel(hf_bitmap_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    float *const sx = ADJ ? a.gpos[0] : a.out_grad[0], *const sy = ADJ ? a.gpos[1] : a.out_grad[1];
    float L = 0.f, Lx = 0.f, Ly = 0.f;
    if (a.active ? a.active[i] != 0 : true) {
        const hf_bitmap_cell e = bitmap_cell(&a, a.pos[0][i], a.pos[1][i]);
        const float g = ADJ ? a.gout[i] : 1.f;
        if (!ADJ) L = e.value(a.tex);
        if (sx) {
            e.slopes(a.tex, Lx, Ly);
            Lx *= g; Ly *= g;
        }
        if (ADJ && a.gtex) e.scatter(a.gtex, g);
    }
    if (!ADJ) a.out[i] = L;
    if (sx) { sx[i] = Lx; sy[i] = Ly; }
}
void hf_launch_bitmap(bool adjoint, const hf_bitmap_args &a, hipStream_t stream) {
    if (a.n == 0) return;
    const dim3 grid((unsigned) ((a.n + HF_BLOCK - 1) / HF_BLOCK)), block(HF_BLOCK);
    hipLaunchKernelGGL(adjoint ? hf_bitmap_eval_kernel<true> : hf_bitmap_eval_kernel<false>, grid, block, 0, stream, a);
}

typedef const __attribute__((address_space(4))) hf_refract_args *hf_refract_kargs;

// what a deposited sample carries to the lookup besides its landing: ((weight (1 - F)) eta_ti^2) exp(-sigma_t s), in
// this order; sigma_t == 0: no exponential at all
__device__ __forceinline__ float refract_throughput(const hf_caustic_vertex &v, const float *weight, size_t i, float sigma_t) {
    const float oneF = 1.f - v.F;
    const float b = (weight ? weight[i] * oneF : oneF) * v.e2;
    return sigma_t != 0.f ? b * expf(-sigma_t * v.s) : b;
}

#ifndef HF_REFRACT_WAVES
#define HF_REFRACT_WAVES 6 // resident waves per SIMD (the siblings')
#endif
__global__ __launch_bounds__(HF_BLOCK, HF_REFRACT_WAVES) void hf_refract_kernel(hf_refract_args a) {
    const hf_dev_field &f = a.f;
    // hf_sky_kernel's mapping: n < 2^32, the sample index is one register across the walk
    const size_t i64 = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const bool in = i64 < a.n;
    const uint32_t i = (uint32_t) i64;
    const uint32_t ii = in ? i : (uint32_t) (a.n - 1);
    hf_refract_kargs ka = (hf_refract_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    float x = -16.f, y = -16.f, bT = 0.f; // what a sample that sees nothing writes
    bool traced;
    hf_hit best;
    best.hit = false;
    {
        v3 m, p;
        const hf_caustic_vertex v = caustic_sample(ka, ii, in, m, p);
        traced = v.traced;
        if (__ballot(traced) != 0ull) { // wave-uniform: a batch without a traced sample walks nothing
            const v3 gn = mk3(ka->nrm[0][ii], ka->nrm[1][ii], ka->nrm[2][ii]);
            if (traced) {
                caustic_landing(ka, p, v, x, y);
                bT = refract_throughput(v, ka->weight, ii, ka->sigma_t); // (the exponential: before the walk's state is live)
            }
            // the landing, the throughput and the index are held across the walk; the ray ends at the receiver
            light_walk<true>(&ka->f, f, sky_origin(p, gn, sky_offset(p), v.wo), v.wo, v.s, traced, best);
        }
    }
    // (the texture and the output pointers: loaded here, not before the walk; the lookup runs when the walk's state is
    // dead)
    hf_refract_kargs ko = (hf_refract_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ko));
    const bool lit = traced && !best.hit; // (traced: in range)
    float val = 0.f;
    if (lit) val = bT * bitmap_cell(ko, x, y).value(ko->tex);
    if (in) {
        float *value = ko->value, *px = ko->pos[0], *py = ko->pos[1];
        uint8_t *vis = ko->vis;
        if (value) value[i] = val;
        if (vis) vis[i] = lit ? 1 : 0;
        if (px) { px[i] = lit ? x : -16.f; py[i] = lit ? y : -16.f; }
    }
    float *image = ko->image;
    if (image) {
        const uint32_t spp = ko->spp, g = spp < 64u ? spp : 64u;
        film_pixel(image, val, 0u, ko->n / spp, i, spp, in, (spp & (spp - 1u)) == 0u, g, 1.0f / (float) spp, i);
    }
}

// What the two derivative kernels form again of a visible sample: the vertex, the landing's lookup and the factors of
//   d value = dw oneF k L + A (-dF dci L + oneF (-sigma_t L ds + Lx dx + Ly dy)) + A oneF sum_j b_j dtex_j,
// k = eta_ti^2 T, A = weight k
struct hf_refract_shade {
    hf_caustic_vertex v;
    hf_bitmap_cell e;
    v3 m;
    float oneF, k, A, L, Lx, Ly;
};
__device__ __forceinline__ hf_refract_shade refract_shade(const hf_refract_args &a, size_t i) {
    hf_refract_shade s;
    v3 p;
    s.v = caustic_sample(&a, i, true, s.m, p);
    float x, y;
    caustic_landing(&a, p, s.v, x, y);
    s.e = bitmap_cell(&a, x, y);
    s.L = s.e.value(a.tex);
    s.e.slopes(a.tex, s.Lx, s.Ly);
    s.oneF = 1.f - s.v.F;
    s.k = a.sigma_t != 0.f ? s.v.e2 * expf(-a.sigma_t * s.v.s) : s.v.e2;
    s.A = a.weight ? a.weight[i] * s.k : s.k;
    return s;
}

// Reverse mode of hf_refract_kernel with respect to sh_n, p, weight and the texels: nothing is traced, the vertex is
// formed again and the visibility byte read.  grad_sh_n, grad_p, grad_weight: one lane per sample, overwritten, no
// atomics; grad_tex: one float atomic per texel of every visible sample
__global__ __launch_bounds__(HF_BLOCK) void hf_refract_adjoint_kernel(hf_refract_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    v3 gm = mk3(0.f, 0.f, 0.f), gp = gm;
    float gw = 0.f;
    if (a.vis[i]) {
        const hf_refract_shade s = refract_shade(a, i);
        if (s.v.traced) {
            const float g = light_value_seed(a, i);
            const float gA = g * s.A, gAF = gA * s.oneF;
            gw = g * ((s.oneF * s.k) * s.L);
            caustic_landing_adjoint<true>(a, s.v, s.m, gAF * s.Lx, gAF * s.Ly, -(gAF * a.sigma_t) * s.L, -(gA * s.v.dF) * s.L, gm, gp);
            if (a.gdata) s.e.scatter(a.gdata, gAF);
        }
    }
    light_store_grads(a, i, gm, gp, gw);
}

// forward mode, the transpose of the above: the tangent of sample i's value for tangents dn of sh_n, dp of p, dw of
// weight and dtex of the texels (NULL: zero)
__device__ __forceinline__ float refract_tangent_value(const hf_refract_args &a, size_t i) {
    if (!a.vis[i]) return 0.f;
    const hf_refract_shade s = refract_shade(a, i);
    if (!s.v.traced) return 0.f;
    const v3 dm = a.dn[0] ? mk3(a.dn[0][i], a.dn[1][i], a.dn[2][i]) : mk3(0.f, 0.f, 0.f);
    const v3 dp = a.dp[0] ? mk3(a.dp[0][i], a.dp[1][i], a.dp[2][i]) : mk3(0.f, 0.f, 0.f);
    const float dw = a.dw ? a.dw[i] : 0.f;
    const float dci = dot3(dm, s.v.wi);
    float dx, dy, ds;
    caustic_landing_tangent(a, s.v, s.m, dm, dp, dci, dx, dy, ds);
    float dL = __builtin_fmaf(s.Lx, dx, s.Ly * dy) - (a.sigma_t * s.L) * ds;
    if (a.ddata) dL += s.e.value(a.ddata);
    const float dv = __builtin_fmaf(s.oneF, dL, -(s.v.dF * dci) * s.L);
    return __builtin_fmaf(dw, (s.oneF * s.k) * s.L, s.A * dv);
}
// (the per-sample tangent is written too, and the image may be NULL)
template <bool PIXEL>
__global__ __launch_bounds__(HF_BLOCK) void hf_refract_tangent_kernel(hf_refract_args a) {
    light_tangent_image<PIXEL, hf_refract_args, refract_tangent_value>(a, a.value);
}

// mode 0: forward, 1: adjoint, 2: tangent (the row has no rays kernel: its ray is hf_caustic_rays')
void hf_launch_refract(int mode, const hf_refract_args &a, hipStream_t stream) {
    launch_light(mode, a, 1u, stream, hf_refract_kernel, hf_refract_adjoint_kernel, hf_refract_tangent_kernel<false>,
                 hf_refract_tangent_kernel<true>, (void (*)(hf_refract_args)) nullptr);
}

// ---------------------------------------------------------------------------------
// Area-light lighting (include/hf.h hf_rect_*): diffuse surface under a one-sided `area` emitter on a `rectangle`, the
// K = num_rays points of the lamp of every wavefront sample drawn (uniform in area, rectangle.cpp:152-166), their
// shadow rays (Interaction::spawn_ray_to, a FINITE maxt) traced (any hit, per lane) and reduced in ONE launch:
// hf_sky_kernel's mapping.  The direction, the falloff and the lamp's cosine depend on the hit point:
//   value = weight (albedo A / (pi K)) sum_k bit_k L_k c_s c_l / r^2.
// The row's own text is the lamp's point, the ray towards it and G = c_s c_l / r^2 with its derivatives; the sample
// stream, the origin, the walk, the film, the outputs, the tangent shell and the launch are the lighting rows' shared
// functions, the texture lookup and its scatter / gather the refraction view's (bitmap_cell).
// (P below: a pointer to hf_rect_args, in the kernarg segment or not)
// ---------------------------------------------------------------------------------
typedef const __attribute__((address_space(4))) hf_rect_args *hf_rect_kargs;

// The shadow ray of a draw, in float32: q = center + (2 s.x - 1) ex + (2 s.y - 1) ey, u = q - p, the origin
// offset_p(u), the direction (q - o) / |q - o| and maxt = |q - o| (1 - ShadowEpsilon), ShadowEpsilon = 10 RayEpsilon
// (math.h:22).  front: <sh_n, u> > 0, <n_l, u> < 0 (the signs of c_s and c_l) and r finite and > 0
struct hf_rect_ray { v3 o, w; float maxt; bool front; };
template <class P>
__device__ __forceinline__ hf_rect_ray rect_ray(P a, v3 p, v3 gn, v3 sn, float mag, float sx, float sy) {
    hf_rect_ray r;
    const float su = __builtin_fmaf(2.f, sx, -1.f), sv = __builtin_fmaf(2.f, sy, -1.f);
    const v3 q = mk3(__builtin_fmaf(sv, a->ey[0], __builtin_fmaf(su, a->ex[0], a->center[0])),
                     __builtin_fmaf(sv, a->ey[1], __builtin_fmaf(su, a->ex[1], a->center[1])),
                     __builtin_fmaf(sv, a->ey[2], __builtin_fmaf(su, a->ex[2], a->center[2])));
    const v3 u = q - p;
    const float r2 = dot3(u, u);
    r.front = dot3(sn, u) > 0.f && dot3(mk3(a->nl[0], a->nl[1], a->nl[2]), u) < 0.f && r2 > 0.f && r2 < __builtin_inff();
    r.o = sky_origin(p, gn, mag, u);
    const v3 dv = q - r.o;
    const float dist = __builtin_sqrtf(dot3(dv, dv));
    r.w = dv * (1.0f / dist);
    r.maxt = dist * (1.f - 8.940696716308594e-04f);
    return r;
}

// The same draw in double, for the SHADING sums (sky_dir_f64's reason: c_s and c_l graze, and u is a difference): u = q - p
// and the unnormalised cosines cs = <sh_n, u>, cl = -<n_l, u>, so that G = c_s c_l / r^2 = cs cl / r2^2 without a root
struct hf_rect_geom { hf_d3 u; double r2, cs, cl; };
template <class P>
__device__ __forceinline__ hf_rect_geom rect_geom_f64(P a, v3 p, v3 sn, float sx, float sy) {
    hf_rect_geom g;
    const double su = 2.0 * (double) sx - 1.0, sv = 2.0 * (double) sy - 1.0;
    g.u.x = ((double) a->center[0] + su * (double) a->ex[0] + sv * (double) a->ey[0]) - (double) p.x;
    g.u.y = ((double) a->center[1] + su * (double) a->ex[1] + sv * (double) a->ey[1]) - (double) p.y;
    g.u.z = ((double) a->center[2] + su * (double) a->ex[2] + sv * (double) a->ey[2]) - (double) p.z;
    g.r2 = g.u.x * g.u.x + g.u.y * g.u.y + g.u.z * g.u.z;
    g.cs = sky_dot_f64(sn, g.u);
    g.cl = -(a->nld[0] * g.u.x + a->nld[1] * g.u.y + a->nld[2] * g.u.z);
    return g;
}
// the texel coordinate of a draw: (s.x TW, s.y TH), a function of the detached draw alone
template <class P>
__device__ __forceinline__ hf_bitmap_cell rect_cell(P a, float sx, float sy) {
    return bitmap_cell(a, sx * (float) a->TW, sy * (float) a->TH);
}

#ifndef HF_RECT_WAVES
#define HF_RECT_WAVES 6 // resident waves per SIMD (the siblings')
#endif
__global__ __launch_bounds__(HF_BLOCK, HF_RECT_WAVES) void hf_rect_kernel(hf_rect_args a) {
    const hf_dev_field &f = a.f;
    // hf_sky_kernel's mapping: n < 2^32, the sample index is one register across the walk
    const size_t i64 = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const bool in = i64 < a.n;
    const uint32_t i = (uint32_t) i64;
    const uint32_t ii = in ? i : (uint32_t) (a.n - 1);
    const v3 sn = mk3(a.sh_n[0][ii], a.sh_n[1][ii], a.sh_n[2][ii]);
    bool elig;
    {
        const v3 d = mk3(a.d[0][ii], a.d[1][ii], a.d[2][ii]);
        elig = in && sky_eligible(a.t[ii], sn, d);
    }
    double acc = 0.0;   // sum over the visible points of L_k c_s c_l / r^2 (rect_geom_f64), in k order, rounded once below
    uint32_t bits = 0u; // bit k: point k was traced and is unoccluded
    if (__ballot(elig) != 0ull) { // wave-uniform: a batch without an eligible sample draws nothing
        const v3 p = mk3(a.p[0][ii], a.p[1][ii], a.p[2][ii]);
        const v3 gn = mk3(a.nrm[0][ii], a.nrm[1][ii], a.nrm[2][ii]);
        const uint32_t id = a.ray_id ? a.ray_id[ii] : ii;
        const float mag = sky_offset(p);
        // (launch constants of the loop, the lamp among them, are read from the kernarg segment where they are used)
        hf_rect_kargs ka = (hf_rect_kargs) __builtin_amdgcn_kernarg_segment_ptr();
#pragma unroll 1
        for (uint32_t k = 0;; ++k) { // wave-uniform loop, the lanes predicated inside
            asm volatile("" : "+s"(ka)); // opaque per point: the kernarg loads stay inside the loop
            // the term that is added first, in double, and finished before the ray is begun (hf_sky_kernel's order: its
            // other doubles and the texels are dead when setup_ray's registers fill, this one is held across the walk)
            v3 snd = sn, pd = p; // (opaque: their conversions to double are otherwise hoisted out of the loop)
            asm volatile("" : "+v"(snd.x), "+v"(snd.y), "+v"(snd.z), "+v"(pd.x), "+v"(pd.y), "+v"(pd.z));
            float sx, sy;
            sky_sample(ka->seed, k, id, sx, sy);
            double co;
            {
                const hf_rect_geom g = rect_geom_f64(ka, pd, snd, sx, sy);
                co = (g.cs * g.cl) / (g.r2 * g.r2);
                const float *tex = ka->tex;
                if (tex) co *= (double) rect_cell(ka, sx, sy).value(tex); // (wave-uniform)
            }
            asm volatile("" : "+v"(co), "+v"(sx), "+v"(sy));
            const hf_rect_ray r = rect_ray(ka, p, gn, sn, mag, sx, sy);
            const bool traced = elig && r.front;
            hf_hit best;
            light_walk<true>(&ka->f, f, r.o, r.w, r.maxt, traced, best);
            if (traced && !best.hit) { bits |= 1u << k; acc += co; }
            if (k + 1u >= ka->num_rays) break;
        }
    }
    // (the output pointers: loaded here, not before the walk)
    hf_rect_kargs ko = (hf_rect_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ko));
    float c = 0.f;
    if (elig) { // (eligible: in range)
        const float *weight = ko->weight;
        c = ko->scale * (float) acc;
        if (weight) c *= weight[i];
    }
    uint32_t *vis_bits = ko->vis_bits;
    if (in && vis_bits) vis_bits[i] = bits;
    const uint32_t spp = ko->spp, g = spp < 64u ? spp : 64u;
    film_pixel(ko->image, c, 0u, ko->n / spp, i, spp, in, (spp & (spp - 1u)) == 0u, g, 1.0f / (float) spp, i);
}

// shadow ray a.k of every sample, materialised: what hf_rect_kernel traces for that point, bit for bit (an untraced
// lane: a zero origin and direction, maxt = -1)
__global__ __launch_bounds__(HF_BLOCK) void hf_rect_rays_kernel(hf_rect_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    v3 sn;
    const bool elig = light_sample(a, i, sn);
    const v3 p = mk3(a.p[0][i], a.p[1][i], a.p[2][i]), gn = mk3(a.nrm[0][i], a.nrm[1][i], a.nrm[2][i]);
    float sx, sy;
    sky_sample(a.seed, a.k, light_id(a, i), sx, sy);
    const hf_rect_ray r = rect_ray(&a, p, gn, sn, sky_offset(p), sx, sy);
    const bool traced = elig && r.front;
    const v3 z = mk3(0.f, 0.f, 0.f);
    light_store_ray(a, i, traced ? r.o : z, traced ? r.w : z, traced, r.maxt);
}

// What the two derivative kernels form again of a visible point: the cell of its texel coordinate, L (1 without a
// texture), G and its derivatives with the draw, the masks and the lamp held:
//   dG/dsh_n = w c_l / r^2 = u cl / r2^2,   dG/dp = (4 c_s c_l w - c_l sh_n + c_s n_l) / r^3 = 4 cs cl u / r2^3 + (cs n_l - cl sh_n) / r2^2
struct hf_rect_shade {
    hf_bitmap_cell e;
    double L, G;
    hf_d3 Gn, Gp;
};
__device__ __forceinline__ hf_rect_shade rect_shade(const hf_rect_args &a, v3 p, v3 sn, uint32_t k, uint32_t id) {
    hf_rect_shade s;
    float sx, sy;
    sky_sample(a.seed, k, id, sx, sy);
    const hf_rect_geom g = rect_geom_f64(&a, p, sn, sx, sy);
    const double i4 = 1.0 / (g.r2 * g.r2), cc = g.cs * g.cl;
    s.G = cc * i4;
    const double gu = 4.0 * cc * i4 / g.r2;
    s.Gn = hf_d3{ g.u.x * (g.cl * i4), g.u.y * (g.cl * i4), g.u.z * (g.cl * i4) };
    s.Gp = hf_d3{ gu * g.u.x + (g.cs * a.nld[0] - g.cl * (double) sn.x) * i4, gu * g.u.y + (g.cs * a.nld[1] - g.cl * (double) sn.y) * i4,
                  gu * g.u.z + (g.cs * a.nld[2] - g.cl * (double) sn.z) * i4 };
    s.L = 1.0;
    if (a.tex) {
        s.e = rect_cell(&a, sx, sy);
        s.L = (double) s.e.value(a.tex);
    }
    return s;
}

// Reverse mode of hf_rect_kernel with respect to sh_n, p, weight and the texels: nothing is traced, the points are drawn
// again and the visibility word read.  grad_sh_n, grad_p, grad_weight: sums in k order, in double, overwritten, no
// atomics; grad_tex: four float atomics per visible point
__global__ __launch_bounds__(HF_BLOCK) void hf_rect_adjoint_kernel(hf_rect_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    v3 sn, gn = mk3(0.f, 0.f, 0.f), gp = gn;
    float gw = 0.f;
    if (light_sample(a, i, sn)) {
        const uint32_t bits = a.vis_bits[i], id = light_id(a, i);
        const v3 p = mk3(a.p[0][i], a.p[1][i], a.p[2][i]);
        const float c = (a.gimg[i / a.spp] * (1.0f / (float) a.spp)) * a.scale; // dL/d(sum) but for the weight
        const float cw = a.weight ? c * a.weight[i] : c;
        hf_d3 sgn = { 0.0, 0.0, 0.0 }, sgp = { 0.0, 0.0, 0.0 };
        double sc = 0.0;
        for (uint32_t k = 0; k < a.num_rays; ++k) {
            if ((bits >> k) & 1u) {
                const hf_rect_shade s = rect_shade(a, p, sn, k, id);
                sgn.x += s.L * s.Gn.x; sgn.y += s.L * s.Gn.y; sgn.z += s.L * s.Gn.z;
                sgp.x += s.L * s.Gp.x; sgp.y += s.L * s.Gp.y; sgp.z += s.L * s.Gp.z;
                sc += s.L * s.G;
                if (a.tex && a.gdata) s.e.scatter(a.gdata, (float) ((double) cw * s.G));
            }
        }
        gn = mk3((float) sgn.x, (float) sgn.y, (float) sgn.z) * cw;
        gp = mk3((float) sgp.x, (float) sgp.y, (float) sgp.z) * cw;
        gw = c * (float) sc;
    }
    light_store_grads(a, i, gn, gp, gw);
}

// forward mode, the transpose of the above: the tangent of sample i's value for tangents dn of sh_n, dp of p, dw of
// weight and dtex of the texels (NULL: zero)
__device__ __forceinline__ float rect_tangent_value(const hf_rect_args &a, size_t i) {
    v3 sn;
    if (!light_sample(a, i, sn)) return 0.f;
    const uint32_t bits = a.vis_bits[i], id = light_id(a, i);
    const v3 p = mk3(a.p[0][i], a.p[1][i], a.p[2][i]);
    const v3 dn = a.dn[0] ? mk3(a.dn[0][i], a.dn[1][i], a.dn[2][i]) : mk3(0.f, 0.f, 0.f);
    const v3 dp = a.dp[0] ? mk3(a.dp[0][i], a.dp[1][i], a.dp[2][i]) : mk3(0.f, 0.f, 0.f);
    double sd = 0.0, sc = 0.0;
    for (uint32_t k = 0; k < a.num_rays; ++k) {
        if ((bits >> k) & 1u) {
            const hf_rect_shade s = rect_shade(a, p, sn, k, id);
            double dG = s.L * (sky_dot_f64(dn, s.Gn) + sky_dot_f64(dp, s.Gp));
            if (a.tex && a.ddata) dG += (double) s.e.value(a.ddata) * s.G;
            sd += dG;
            sc += s.L * s.G;
        }
    }
    return (float) ((double) a.scale * ((double) (a.weight ? a.weight[i] : 1.f) * sd + (double) (a.dw ? a.dw[i] : 0.f) * sc));
}
template <bool PIXEL>
__global__ __launch_bounds__(HF_BLOCK) void hf_rect_tangent_kernel(hf_rect_args a) {
    light_tangent_image<PIXEL, hf_rect_args, rect_tangent_value>(a, nullptr);
}

void hf_launch_rect(int mode, const hf_rect_args &a, hipStream_t stream) {
    launch_light(mode, a, 1u, stream, hf_rect_kernel, hf_rect_adjoint_kernel, hf_rect_tangent_kernel<false>,
                 hf_rect_tangent_kernel<true>, hf_rect_rays_kernel);
}

// ---------------------------------------------------------------------------------
// The sensor (include/hf.h): the primary wavefront of a perspective or an orthographic camera, its tangent
// and its adjoint.  One sample per lane, consecutive lanes store consecutive floats of every row; no LDS in the rays
// and tangent kernels.  The sensor's constants come as kernel arguments (formed on the host in double), so they are
// wave-uniform; the per-sample arithmetic is double and every output is rounded once.
// ---------------------------------------------------------------------------------
struct hf_sensor_film {
    double px, py; // pos: the film position in pixels of the whole film
    double wx, wy; // w = (1 - 2 g.x, (1 - 2 g.y) / a), g = pos / film_size
};
__device__ __forceinline__ hf_sensor_film sensor_sample(const hf_sensor_args &a, size_t i) {
    const uint32_t id = a.ray_id ? a.ray_id[i] : a.start + (uint32_t) i;
    uint32_t v0, v1;
    tea32(a.seed, id, v0, v1);
    // integrator.cpp:251-268; a shift where the divisor is a power of two (wave-uniform choice)
    const uint32_t pix = a.spp_shift >= 0 ? id >> a.spp_shift : id / a.spp;
    const uint32_t row = a.crop_w_shift >= 0 ? pix >> a.crop_w_shift : pix / a.crop_w;
    const uint32_t col = pix - row * a.crop_w;
    hf_sensor_film f;
    f.px = (double) (col + a.crop_x) + (double) (v0 >> 9) * (1.0 / 8388608.0);
    f.py = (double) (row + a.crop_y) + (double) (v1 >> 9) * (1.0 / 8388608.0);
    f.wx = 1.0 - 2.0 * (f.px / a.film_w);
    f.wy = (1.0 - 2.0 * (f.py / a.film_h)) / a.aspect;
    return f;
}
// perspective: v = (w tau, 1), its length and d_c = v / |v|
struct hf_sensor_dir {
    double vx, vy, len, il, cx, cy, cz;
};
__device__ __forceinline__ hf_sensor_dir sensor_dir(const hf_sensor_args &a, const hf_sensor_film &f) {
    hf_sensor_dir q;
    q.vx = f.wx * a.tau; q.vy = f.wy * a.tau;
    q.len = __builtin_sqrt(q.vx * q.vx + q.vy * q.vy + 1.0);
    q.il = 1.0 / q.len;
    q.cx = q.vx * q.il; q.cy = q.vy * q.il; q.cz = q.il;
    return q;
}

// one sample's nine outputs, in the order of the rows: o (3), d (3), maxt, pos (2)
#define HF_SENSOR_ROWS 9
template <int TYPE>
__device__ __forceinline__ void sensor_ray(const hf_sensor_args &a, size_t i, float r[HF_SENSOR_ROWS]) {
    const hf_sensor_film f = sensor_sample(a, i);
    r[7] = (float) f.px; r[8] = (float) f.py;
    if (TYPE == HF_SENSOR_PERSPECTIVE) {
        const hf_sensor_dir q = sensor_dir(a, f);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double Av = a.A[3 * k] * q.vx + a.A[3 * k + 1] * q.vy + a.A[3 * k + 2];
            r[k] = (float) (a.c[k] + a.near * Av);
            r[3 + k] = (float) (a.A[3 * k] * q.cx + a.A[3 * k + 1] * q.cy + a.A[3 * k + 2] * q.cz);
        }
        r[6] = (float) (a.span * q.len);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r[k] = (float) (a.A[3 * k] * f.wx + a.A[3 * k + 1] * f.wy + a.An[k] + a.c[k]);
            r[3 + k] = (float) a.dz[k];
        }
        r[6] = (float) a.span;
    }
}
// (ARGS: hf_sensor_args, or the thin lens's block around one -- sensor_base is the block the store code reads)
__device__ __forceinline__ const hf_sensor_args &sensor_base(const hf_sensor_args &a) { return a; }
// the dword path: sample i to element i of every row that is wanted
template <int TYPE, class ARGS>
__device__ __forceinline__ void sensor_ray_store(const ARGS &args, size_t i) {
    const hf_sensor_args &a = sensor_base(args);
    float r[HF_SENSOR_ROWS];
    sensor_ray<TYPE>(args, i, r);
#pragma unroll
    for (int k = 0; k < 3; ++k) { a.out_o[k][i] = r[k]; a.out_d[k][i] = r[3 + k]; }
    a.out_maxt[i] = r[6];
    if (a.out_pos[0]) { a.out_pos[0][i] = r[7]; a.out_pos[1][i] = r[8]; }
}
template <int TYPE, class ARGS>
__device__ __forceinline__ void sensor_rays_dword(const ARGS &args) {
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < sensor_base(args).n; i += (size_t) gridDim.x * HF_BLOCK)
        sensor_ray_store<TYPE>(args, i);
}
// variant A: one sample per lane, a wave stores 256 contiguous bytes of every row
template <int TYPE>
__global__ __launch_bounds__(HF_BLOCK) void hf_sensor_rays_kernel(hf_sensor_args a) {
    sensor_rays_dword<TYPE>(a);
}
// variant B: four consecutive samples per lane, one 16-byte store per row.  a.head samples come before the first group,
// so that element a.head of out_o[0] is 16-byte aligned; bit k of a.wide_mask says that row k has the same alignment
// (its groups are stored as one float4), any other row takes four dword stores per group; the head and the tail (fewer
// than 4 + 4 samples) take the dword path on the first lanes of the grid.
typedef float hf_sensor_f4 __attribute__((ext_vector_type(4)));
template <int TYPE, class ARGS>
__device__ __forceinline__ void sensor_rays_wide(const ARGS &args) {
    const hf_sensor_args &a = sensor_base(args);
    float *const row[HF_SENSOR_ROWS] = { a.out_o[0], a.out_o[1], a.out_o[2], a.out_d[0], a.out_d[1], a.out_d[2], a.out_maxt,
                                         a.out_pos[0], a.out_pos[1] };
    const size_t tid = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const size_t groups = (a.n - a.head) >> 2;
    for (size_t g = tid; g < groups; g += (size_t) gridDim.x * HF_BLOCK) {
        const size_t i0 = a.head + 4 * g;
        float r[4][HF_SENSOR_ROWS];
#pragma unroll
        for (int j = 0; j < 4; ++j) sensor_ray<TYPE>(args, i0 + j, r[j]);
#pragma unroll
        for (int k = 0; k < HF_SENSOR_ROWS; ++k) {
            if (!row[k]) continue;
            if ((a.wide_mask >> k) & 1u) {
                const hf_sensor_f4 v = { r[0][k], r[1][k], r[2][k], r[3][k] };
                *reinterpret_cast<hf_sensor_f4 *>(row[k] + i0) = v;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) row[k][i0 + j] = r[j][k];
            }
        }
    }
    const size_t tail0 = a.head + 4 * groups, rest = a.head + (a.n - tail0);
    if (tid < rest) sensor_ray_store<TYPE>(args, tid < a.head ? tid : tail0 + (tid - a.head));
}
template <int TYPE>
__global__ __launch_bounds__(HF_BLOCK) void hf_sensor_rays_wide_kernel(hf_sensor_args a) {
    sensor_rays_wide<TYPE>(a);
}

template <int TYPE>
__global__ __launch_bounds__(HF_BLOCK) void hf_sensor_tangent_kernel(hf_sensor_args a) {
    double dM[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) dM[j] = a.d_tw ? (double) a.d_tw[j] : 0.0;
    const double dT = a.d_fov ? (double) a.d_fov[0] * a.dtau : 0.0;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += (size_t) gridDim.x * HF_BLOCK) {
        const hf_sensor_film f = sensor_sample(a, i);
        if (TYPE == HF_SENSOR_PERSPECTIVE) {
            const hf_sensor_dir q = sensor_dir(a, f);
            const double dvx = f.wx * dT, dvy = f.wy * dT;
            const double pr = q.cx * dvx + q.cy * dvy;
            const double ex = (dvx - q.cx * pr) * q.il, ey = (dvy - q.cy * pr) * q.il, ez = -(q.cz * pr) * q.il;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double *A = a.A + 3 * k, *dA = dM + 4 * k;
                a.out_o[k][i] = (float) (dA[3] + a.near * (dA[0] * q.vx + dA[1] * q.vy + dA[2] + A[0] * dvx + A[1] * dvy));
                a.out_d[k][i] = (float) (dA[0] * q.cx + dA[1] * q.cy + dA[2] * q.cz + A[0] * ex + A[1] * ey + A[2] * ez);
            }
        } else {
            const double pr = a.dz[0] * dM[2] + a.dz[1] * dM[6] + a.dz[2] * dM[10];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double *dA = dM + 4 * k;
                a.out_o[k][i] = (float) (dA[0] * f.wx + dA[1] * f.wy + dA[2] * a.near + dA[3]);
                a.out_d[k][i] = (float) ((dA[2] - a.dz[k] * pr) * a.inv_len_z);
            }
        }
    }
}

// The adjoint: every lane keeps its 13 sums (to_world's 12, tau's) in double across its grid-stride loop; a block adds
// them (a butterfly over the wave, then the four waves through LDS, in a fixed order) into its row of the slab, and
// hf_sensor_sum_kernel adds the rows in a fixed order: no float atomics, bitwise the same from launch to launch.
#define HF_SENSOR_SUMS 13
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
// the block's sums of M into slab row blockIdx.x; every thread of the block calls it
template <int SUMS>
__device__ __forceinline__ void sensor_block_store(const double M[SUMS], double *slab) {
    __shared__ double s_red[HF_BLOCK / 64][SUMS];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < SUMS; ++j) {
        const double v = wave_sum_f64(M[j]);
        if (lane == 0u) s_red[w][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < SUMS) {
        double v = s_red[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < HF_BLOCK / 64; ++k) v += s_red[k][threadIdx.x];
        slab[(size_t) blockIdx.x * SUMS + threadIdx.x] = v;
    }
}
template <int TYPE>
__global__ __launch_bounds__(HF_BLOCK) void hf_sensor_adjoint_kernel(hf_sensor_args a) {
    double M[HF_SENSOR_SUMS];
#pragma unroll
    for (int j = 0; j < HF_SENSOR_SUMS; ++j) M[j] = 0.0;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += (size_t) gridDim.x * HF_BLOCK) {
        const hf_sensor_film f = sensor_sample(a, i);
        double go[3], gd[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            go[k] = a.go[k] ? (double) a.go[k][i] : 0.0;
            gd[k] = a.gd[k] ? (double) a.gd[k][i] : 0.0;
        }
        if (TYPE == HF_SENSOR_PERSPECTIVE) {
            const hf_sensor_dir q = sensor_dir(a, f);
            double p[2] = { 0.0, 0.0 }, t[3] = { 0.0, 0.0, 0.0 }; // near A^T go (x, y), A^T gd
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double *A = a.A + 3 * k, no = a.near * go[k];
                M[4 * k] += no * q.vx + gd[k] * q.cx;
                M[4 * k + 1] += no * q.vy + gd[k] * q.cy;
                M[4 * k + 2] += no + gd[k] * q.cz;
                M[4 * k + 3] += go[k];
                p[0] += A[0] * no; p[1] += A[1] * no;
                t[0] += A[0] * gd[k]; t[1] += A[1] * gd[k]; t[2] += A[2] * gd[k];
            }
            const double pr = q.cx * t[0] + q.cy * t[1] + q.cz * t[2];
            M[12] += (p[0] + (t[0] - q.cx * pr) * q.il) * f.wx + (p[1] + (t[1] - q.cy * pr) * q.il) * f.wy;
        } else {
            const double pr = a.dz[0] * gd[0] + a.dz[1] * gd[1] + a.dz[2] * gd[2];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                M[4 * k] += go[k] * f.wx;
                M[4 * k + 1] += go[k] * f.wy;
                M[4 * k + 2] += go[k] * a.near + (gd[k] - a.dz[k] * pr) * a.inv_len_z;
                M[4 * k + 3] += go[k];
            }
        }
    }
    sensor_block_store<HF_SENSOR_SUMS>(M, a.slab);
}
// g_tw[j] += column j of the slab's rows, g_fov[0] += dtau * column 12: every thread adds every HF_BLOCK-th row, then a
// fixed-order tree over the block through LDS.  One block.
// (sensor_slab_sums: the columns' sums, readable by every thread of the one block once it returns)
template <int SUMS>
__device__ __forceinline__ const double *sensor_slab_sums(const double *__restrict__ slab, uint32_t rows) {
    __shared__ double s_part[HF_BLOCK][SUMS];
    const uint32_t t = threadIdx.x;
    double acc[SUMS];
#pragma unroll
    for (int j = 0; j < SUMS; ++j) acc[j] = 0.0;
    for (uint32_t b = t; b < rows; b += HF_BLOCK) {
#pragma unroll
        for (int j = 0; j < SUMS; ++j) acc[j] += slab[(size_t) b * SUMS + j];
    }
#pragma unroll
    for (int j = 0; j < SUMS; ++j) s_part[t][j] = acc[j];
    __syncthreads();
#pragma unroll
    for (uint32_t h = HF_BLOCK / 2; h > 0; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int j = 0; j < SUMS; ++j) s_part[t][j] += s_part[t + h][j];
        }
        __syncthreads();
    }
    return s_part[0];
}
__global__ __launch_bounds__(HF_BLOCK) void hf_sensor_sum_kernel(const double *__restrict__ slab, uint32_t rows, double dtau,
                                                                  float *__restrict__ g_tw, float *__restrict__ g_fov) {
    const double *const sum = sensor_slab_sums<HF_SENSOR_SUMS>(slab, rows);
    const uint32_t t = threadIdx.x;
    if (t < 12u) {
        if (g_tw) g_tw[t] += (float) sum[t];
    } else if (t == 12u && g_fov) {
        g_fov[0] += (float) (sum[12] * dtau);
    }
}
size_t hf_sensor_slab_doubles() { return (size_t) HF_XFORM_GRID_CAP * HF_SENSOR_SUMS; }

// ---- the way back: perspective sample_direction (perspective.cpp:279-318, 334-383) ----
struct hf_sensor_proj {
    bool inside, valid;  // inside_z; inside_z and s_crop in [0, 1]^2
    double x, y, z;      // ref = to_world^-1 p
    double iz, rx, ry;   // 1 / ref.z, ref.x / ref.z, ref.y / ref.z
    double u, v;         // uv: the film position in pixels of the whole film
    double r2, W;        // |ref|^2, importance(local_d) / dist^2 = |ref| / (A' ref.z^3)
};
__device__ __forceinline__ hf_sensor_proj sensor_project(const hf_sensor_project_args &a, size_t i) {
    hf_sensor_proj r;
    const double q0 = (double) a.p[0][i] - a.c[0], q1 = (double) a.p[1][i] - a.c[1], q2 = (double) a.p[2][i] - a.c[2];
    r.x = a.Ai[0] * q0 + a.Ai[1] * q1 + a.Ai[2] * q2;
    r.y = a.Ai[3] * q0 + a.Ai[4] * q1 + a.Ai[5] * q2;
    r.z = a.Ai[6] * q0 + a.Ai[7] * q1 + a.Ai[8] * q2;
    r.inside = (!a.active || a.active[i] != 0) && r.z >= a.near && r.z <= a.far; // perspective.cpp:289
    r.iz = 1.0 / r.z; r.rx = r.x * r.iz; r.ry = r.y * r.iz;
    r.u = 0.5 * (1.0 - r.rx / a.tau) * a.film_w;                                   // camera_to_sample (sensor.h:256-262)
    r.v = 0.5 * (1.0 - a.aspect * r.ry / a.tau) * a.film_h;
    const double sx = (r.u - a.crop_x) / a.crop_w, sy = (r.v - a.crop_y) / a.crop_h;
    r.valid = r.inside && sx >= 0.0 && sx <= 1.0 && sy >= 0.0 && sy <= 1.0;        // perspective.cpp:299-300
    r.r2 = r.x * r.x + r.y * r.y + r.z * r.z;
    r.W = __builtin_sqrt(r.r2) * a.inv_area * (r.iz * r.iz * r.iz);                // perspective.cpp:317, 372-382
    return r;
}
__global__ __launch_bounds__(HF_BLOCK) void hf_sensor_project_kernel(hf_sensor_project_args a) {
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += (size_t) gridDim.x * HF_BLOCK) {
        const hf_sensor_proj r = sensor_project(a, i);
        a.uv[0][i] = r.inside ? (float) r.u : 0.f;
        a.uv[1][i] = r.inside ? (float) r.v : 0.f;
        a.valid[i] = r.valid ? 1 : 0;
        if (a.weight) a.weight[i] = r.valid ? (float) r.W : 0.f;
    }
}
__global__ __launch_bounds__(HF_BLOCK) void hf_sensor_project_tangent_kernel(hf_sensor_project_args a) {
    double dM[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) dM[j] = a.d_tw ? (double) a.d_tw[j] : 0.0;
    const double dT = (a.d_fov ? (double) a.d_fov[0] * a.dtau : 0.0) / a.tau; // d tau / tau
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += (size_t) gridDim.x * HF_BLOCK) {
        const hf_sensor_proj r = sensor_project(a, i);
        double dq[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) // dp - dA ref - dc
            dq[k] = (a.dp[k] ? (double) a.dp[k][i] : 0.0) - (dM[4 * k] * r.x + dM[4 * k + 1] * r.y + dM[4 * k + 2] * r.z) - dM[4 * k + 3];
        const double dx = a.Ai[0] * dq[0] + a.Ai[1] * dq[1] + a.Ai[2] * dq[2];
        const double dy = a.Ai[3] * dq[0] + a.Ai[4] * dq[1] + a.Ai[5] * dq[2];
        const double dz = a.Ai[6] * dq[0] + a.Ai[7] * dq[1] + a.Ai[8] * dq[2];
        const double drx = (dx - r.rx * dz) * r.iz, dry = (dy - r.ry * dz) * r.iz;
        const double cu = -0.5 * a.film_w / a.tau, cv = -0.5 * a.film_h * a.aspect / a.tau;
        a.uv[0][i] = r.inside ? (float) (cu * (drx - r.rx * dT)) : 0.f;
        a.uv[1][i] = r.inside ? (float) (cv * (dry - r.ry * dT)) : 0.f;
        if (a.weight)
            a.weight[i] = r.valid ? (float) (r.W * ((r.x * dx + r.y * dy + r.z * dz) / r.r2 - 3.0 * dz * r.iz - 2.0 * dT)) : 0.f;
    }
}
__global__ __launch_bounds__(HF_BLOCK) void hf_sensor_project_adjoint_kernel(hf_sensor_project_args a) {
    double M[HF_SENSOR_SUMS];
#pragma unroll
    for (int j = 0; j < HF_SENSOR_SUMS; ++j) M[j] = 0.0;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += (size_t) gridDim.x * HF_BLOCK) {
        const hf_sensor_proj r = sensor_project(a, i);
        const double cu = -0.5 * a.film_w / a.tau, cv = -0.5 * a.film_h * a.aspect / a.tau;
        const double grx = r.inside && a.guv[0] ? cu * (double) a.guv[0][i] : 0.0;
        const double gry = r.inside && a.guv[1] ? cv * (double) a.guv[1][i] : 0.0;
        const double gW = r.valid && a.gweight ? r.W * (double) a.gweight[i] : 0.0;
        // dL/dref and dL/d(ln tau)
        const double gx = grx * r.iz + gW * r.x / r.r2;
        const double gy = gry * r.iz + gW * r.y / r.r2;
        const double gz = -(grx * r.rx + gry * r.ry) * r.iz + gW * (r.z / r.r2 - 3.0 * r.iz);
        const bool any = r.inside; // (valid implies inside: a lane outside the clip range has no derivative)
        double h[3]; // to_world^-T dL/dref = dL/dp
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            h[k] = any ? a.Ai[k] * gx + a.Ai[3 + k] * gy + a.Ai[6 + k] * gz : 0.0;
            if (a.gp[k]) a.gp[k][i] = (float) h[k];
            M[4 * k] -= h[k] * r.x; M[4 * k + 1] -= h[k] * r.y; M[4 * k + 2] -= h[k] * r.z; M[4 * k + 3] -= h[k];
        }
        M[12] -= any ? grx * r.rx + gry * r.ry + 2.0 * gW : 0.0;
    }
    sensor_block_store<HF_SENSOR_SUMS>(M, a.slab);
}

void hf_launch_sensor_project(int mode, const hf_sensor_project_args &a, hipStream_t stream) {
    if (mode == 1) {
        const int grid = grid_for(a.n, HF_XFORM_GRID_CAP);
        hipLaunchKernelGGL(hf_sensor_project_adjoint_kernel, dim3(grid), dim3(HF_BLOCK), 0, stream, a);
        // column 12 holds dL/d(ln tau): times d tau / tau per degree
        hipLaunchKernelGGL(hf_sensor_sum_kernel, dim3(1), dim3(HF_BLOCK), 0, stream, a.slab, (uint32_t) grid, a.dtau / a.tau,
                           a.g_tw, a.g_fov);
        return;
    }
    hipLaunchKernelGGL(mode == 0 ? hf_sensor_project_kernel : hf_sensor_project_tangent_kernel,
                       dim3(grid_for(a.n, HF_SI_GRID_CAP)), dim3(HF_BLOCK), 0, stream, a);
}

// Which store variant hf_sensor_rays launches.  HF_SENSOR_WIDE_DEFAULT is the one that measured faster (DESIGN 4.23,
// profiles/sensor/times.jsonl); TEST HOOK (include/hf.h): HF_SENSOR_STORE=dword|wide picks the other, so that the two can be
// timed in one process and compared bit for bit.
#ifndef HF_SENSOR_WIDE_DEFAULT
#define HF_SENSOR_WIDE_DEFAULT 1
#endif
static bool sensor_wide_store() {
    if (const char *e = getenv("HF_SENSOR_STORE")) {
        if (!strcmp(e, "wide")) return true;
        if (!strcmp(e, "dword")) return false;
    }
    return HF_SENSOR_WIDE_DEFAULT != 0;
}
// the 16-byte variant's head and wide_mask from the rows' addresses; returns the number of four-sample groups
static size_t sensor_wide_groups(hf_sensor_args &w) {
    float *const row[HF_SENSOR_ROWS] = { w.out_o[0], w.out_o[1], w.out_o[2], w.out_d[0], w.out_d[1], w.out_d[2], w.out_maxt,
                                         w.out_pos[0], w.out_pos[1] };
    const uint32_t r0 = (uint32_t) (((uintptr_t) row[0] >> 2) & 3u);
    w.head = (4u - r0) & 3u;
    for (int k = 0; k < HF_SENSOR_ROWS; ++k)
        if (row[k] && (((uintptr_t) row[k] >> 2) & 3u) == r0) w.wide_mask |= 1u << k;
    return (w.n - w.head) >> 2;
}
void hf_launch_sensor(int mode, int type, const hf_sensor_args &a, hipStream_t stream) {
    const bool persp = type == HF_SENSOR_PERSPECTIVE;
    if (mode == 1) {
        const int grid = grid_for(a.n, HF_XFORM_GRID_CAP); // the slab holds HF_XFORM_GRID_CAP rows
        hipLaunchKernelGGL(persp ? hf_sensor_adjoint_kernel<HF_SENSOR_PERSPECTIVE> : hf_sensor_adjoint_kernel<HF_SENSOR_ORTHOGRAPHIC>,
                           dim3(grid), dim3(HF_BLOCK), 0, stream, a);
        hipLaunchKernelGGL(hf_sensor_sum_kernel, dim3(1), dim3(HF_BLOCK), 0, stream, a.slab, (uint32_t) grid, a.dtau, a.g_tw,
                           persp ? a.g_fov : nullptr);
        return;
    }
    if (mode == 0 && sensor_wide_store() && a.n >= 64) {
        hf_sensor_args w = a;
        const size_t groups = sensor_wide_groups(w);
        hipLaunchKernelGGL(persp ? hf_sensor_rays_wide_kernel<HF_SENSOR_PERSPECTIVE> : hf_sensor_rays_wide_kernel<HF_SENSOR_ORTHOGRAPHIC>,
                           dim3(grid_for(groups, HF_SI_GRID_CAP)), dim3(HF_BLOCK), 0, stream, w);
        return;
    }
    const dim3 grid(grid_for(a.n, HF_SI_GRID_CAP)), block(HF_BLOCK);
    if (mode == 0)
        hipLaunchKernelGGL(persp ? hf_sensor_rays_kernel<HF_SENSOR_PERSPECTIVE> : hf_sensor_rays_kernel<HF_SENSOR_ORTHOGRAPHIC>,
                           grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL(persp ? hf_sensor_tangent_kernel<HF_SENSOR_PERSPECTIVE> : hf_sensor_tangent_kernel<HF_SENSOR_ORTHOGRAPHIC>,
                           grid, block, 0, stream, a);
}

// ---------------------------------------------------------------------------------
// The thin lens (include/hf.h): the perspective sensor with an aperture of radius r focused at the distance f
// (thinlens.cpp:216-254, 305-350).  The film sample, the store code and the reducer are the sensor's; what is new per
// sample is one more TEA draw, the concentric disk in double and e = f v - r D in place of v.  One sample per lane, the
// constants wave-uniform kernel arguments, double arithmetic, every output rounded once; 15 sums (to_world's 12, tau's,
// r's, f's) where the sensor has 13.
// ---------------------------------------------------------------------------------
#define HF_THINLENS_TYPE 2 // the TYPE of the shared store templates (no hf_sensor_t carries it)
#define HF_THINLENS_SUMS 15
__device__ __forceinline__ const hf_sensor_args &sensor_base(const hf_thinlens_args &a) { return a.s; }
// the stream of the aperture samples: sky_sample's keyed convention with a pair no lighting row draws; the key is one
// more constant formed on the host (by the launchers below)
static uint32_t thinlens_key(uint32_t seed) {
    uint32_t key, unused;
    tea32(seed, HF_THINLENS_PAIR, key, unused);
    return key;
}
// D = square_to_uniform_disk_concentric (warp.h, as bounce_disk has it) of the sample (a >> 9) 2^-23 of tea32(key, id), in
// double from the exact float: phi / pi = rp / (4 r) is at most 1/4, the other quadrant pair swaps sine and cosine
struct hf_lens_disk { double x, y; };
__device__ __forceinline__ hf_lens_disk thinlens_disk(uint32_t key, uint32_t id) {
    uint32_t a0, a1;
    tea32(key, id, a0, a1);
    const double x = 2.0 * ((double) (a0 >> 9) * (1.0 / 8388608.0)) - 1.0, y = 2.0 * ((double) (a1 >> 9) * (1.0 / 8388608.0)) - 1.0;
    const bool q13 = __builtin_fabs(x) < __builtin_fabs(y);
    const double r = q13 ? y : x, rp = q13 ? x : y;
    const double a = r == 0.0 ? 0.0 : 0.25 * rp / r; // (|rp| <= |r|: r == 0 is the centre)
    const auto [sn, cs] = light_sincos_f64(3.141592653589793 * a);
    return hf_lens_disk{ r * (q13 ? sn : cs), r * (q13 ? cs : sn) };
}
__device__ __forceinline__ uint32_t thinlens_id(const hf_sensor_args &s, size_t i) { return s.ray_id ? s.ray_id[i] : s.start + (uint32_t) i; }
// e = f v - r D (thinlens.cpp:239-242), its length and d_c = e / |e|; v = (vx, vy, 1) as the perspective sensor's
struct hf_lens_dir {
    double Dx, Dy, vx, vy, len, il, cx, cy, cz;
};
__device__ __forceinline__ hf_lens_dir thinlens_dir(const hf_thinlens_args &a, const hf_sensor_film &f, size_t i) {
    const hf_lens_disk D = thinlens_disk(a.key, thinlens_id(a.s, i));
    hf_lens_dir q;
    q.Dx = D.x; q.Dy = D.y;
    q.vx = f.wx * a.s.tau; q.vy = f.wy * a.s.tau;
    const double ex = a.focus * q.vx - a.radius * D.x, ey = a.focus * q.vy - a.radius * D.y;
    q.len = __builtin_sqrt(ex * ex + ey * ey + a.focus * a.focus);
    q.il = 1.0 / q.len;
    q.cx = ex * q.il; q.cy = ey * q.il; q.cz = a.focus * q.il;
    return q;
}
template <int TYPE>
__device__ __forceinline__ void sensor_ray(const hf_thinlens_args &a, size_t i, float r[HF_SENSOR_ROWS]) {
    const hf_sensor_film f = sensor_sample(a.s, i);
    r[7] = (float) f.px; r[8] = (float) f.py;
    const hf_lens_dir q = thinlens_dir(a, f, i);
    const double ox = a.lens_o * q.Dx + a.s.near * q.vx, oy = a.lens_o * q.Dy + a.s.near * q.vy; // o_c; its z is near
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double *A = a.s.A + 3 * k;
        r[k] = (float) (a.s.c[k] + (A[0] * ox + A[1] * oy + A[2] * a.s.near));
        r[3 + k] = (float) (A[0] * q.cx + A[1] * q.cy + A[2] * q.cz);
    }
    r[6] = (float) (a.maxt_scale * q.len);
}
__global__ __launch_bounds__(HF_BLOCK) void hf_thinlens_rays_kernel(hf_thinlens_args a) {
    sensor_rays_dword<HF_THINLENS_TYPE>(a);
}
__global__ __launch_bounds__(HF_BLOCK) void hf_thinlens_rays_wide_kernel(hf_thinlens_args a) {
    sensor_rays_wide<HF_THINLENS_TYPE>(a);
}

__global__ __launch_bounds__(HF_BLOCK) void hf_thinlens_tangent_kernel(hf_thinlens_args a) {
    double dM[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) dM[j] = a.s.d_tw ? (double) a.s.d_tw[j] : 0.0;
    const double dT = a.s.d_fov ? (double) a.s.d_fov[0] * a.s.dtau : 0.0;
    const double dr = a.d_radius ? (double) a.d_radius[0] : 0.0, df = a.d_focus ? (double) a.d_focus[0] : 0.0;
    const double near = a.s.near, oD = (1.0 - near / a.focus) * dr + (a.radius * near / (a.focus * a.focus)) * df;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.s.n; i += (size_t) gridDim.x * HF_BLOCK) {
        const hf_sensor_film f = sensor_sample(a.s, i);
        const hf_lens_dir q = thinlens_dir(a, f, i);
        // de = f u dtau + v df - D dr,   d d_c = (de - d_c <d_c, de>) / |e|
        const double dex = a.focus * f.wx * dT + q.vx * df - q.Dx * dr, dey = a.focus * f.wy * dT + q.vy * df - q.Dy * dr;
        const double pr = q.cx * dex + q.cy * dey + q.cz * df;
        const double ex = (dex - q.cx * pr) * q.il, ey = (dey - q.cy * pr) * q.il, ez = (df - q.cz * pr) * q.il;
        // o_c and d o_c = oD D + near u dtau
        const double ox = a.lens_o * q.Dx + near * q.vx, oy = a.lens_o * q.Dy + near * q.vy;
        const double dox = oD * q.Dx + near * f.wx * dT, doy = oD * q.Dy + near * f.wy * dT;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double *A = a.s.A + 3 * k, *dA = dM + 4 * k;
            a.s.out_o[k][i] = (float) (dA[3] + (dA[0] * ox + dA[1] * oy + dA[2] * near) + (A[0] * dox + A[1] * doy));
            a.s.out_d[k][i] = (float) (dA[0] * q.cx + dA[1] * q.cy + dA[2] * q.cz + A[0] * ex + A[1] * ey + A[2] * ez);
        }
    }
}
// the exact transpose; sums 0..11: to_world, 12: tau, 13: r, 14: f
__global__ __launch_bounds__(HF_BLOCK) void hf_thinlens_adjoint_kernel(hf_thinlens_args a) {
    double M[HF_THINLENS_SUMS];
#pragma unroll
    for (int j = 0; j < HF_THINLENS_SUMS; ++j) M[j] = 0.0;
    const double near = a.s.near, oR = 1.0 - near / a.focus, oF = a.radius * near / (a.focus * a.focus);
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.s.n; i += (size_t) gridDim.x * HF_BLOCK) {
        const hf_sensor_film f = sensor_sample(a.s, i);
        const hf_lens_dir q = thinlens_dir(a, f, i);
        const double ox = a.lens_o * q.Dx + near * q.vx, oy = a.lens_o * q.Dy + near * q.vy;
        double p[2] = { 0.0, 0.0 }, t[3] = { 0.0, 0.0, 0.0 }; // A^T go (x, y), A^T gd
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double *A = a.s.A + 3 * k;
            const double go = a.s.go[k] ? (double) a.s.go[k][i] : 0.0, gd = a.s.gd[k] ? (double) a.s.gd[k][i] : 0.0;
            M[4 * k] += go * ox + gd * q.cx;
            M[4 * k + 1] += go * oy + gd * q.cy;
            M[4 * k + 2] += go * near + gd * q.cz;
            M[4 * k + 3] += go;
            p[0] += A[0] * go; p[1] += A[1] * go;
            t[0] += A[0] * gd; t[1] += A[1] * gd; t[2] += A[2] * gd;
        }
        const double pr = q.cx * t[0] + q.cy * t[1] + q.cz * t[2];
        const double gx = (t[0] - q.cx * pr) * q.il, gy = (t[1] - q.cy * pr) * q.il, gz = (t[2] - q.cz * pr) * q.il; // dL/de
        const double pD = p[0] * q.Dx + p[1] * q.Dy;
        M[12] += (a.focus * gx + near * p[0]) * f.wx + (a.focus * gy + near * p[1]) * f.wy;
        M[13] += oR * pD - (gx * q.Dx + gy * q.Dy);
        M[14] += oF * pD + (gx * q.vx + gy * q.vy + gz);
    }
    sensor_block_store<HF_THINLENS_SUMS>(M, a.s.slab);
}
// g_tw[j] += column j, g_fov[0] += dtau * column 12, g_radius[0] += column 13, g_focus[0] += column 14.  One block.
__global__ __launch_bounds__(HF_BLOCK) void hf_thinlens_sum_kernel(const double *__restrict__ slab, uint32_t rows, double dtau,
                                                                    float *__restrict__ g_tw, float *__restrict__ g_fov,
                                                                    float *__restrict__ g_radius, float *__restrict__ g_focus) {
    const double *const sum = sensor_slab_sums<HF_THINLENS_SUMS>(slab, rows);
    const uint32_t t = threadIdx.x;
    if (t < 12u) {
        if (g_tw) g_tw[t] += (float) sum[t];
    } else if (t == 12u) {
        if (g_fov) g_fov[0] += (float) (sum[12] * dtau);
    } else if (t == 13u) {
        if (g_radius) g_radius[0] += (float) sum[13];
    } else if (t == 14u) {
        if (g_focus) g_focus[0] += (float) sum[14];
    }
}
size_t hf_thinlens_slab_doubles() { return (size_t) HF_XFORM_GRID_CAP * HF_THINLENS_SUMS; }

void hf_launch_thinlens(int mode, const hf_thinlens_args &args, hipStream_t stream) {
    hf_thinlens_args a = args;
    a.key = thinlens_key(a.s.seed);
    if (mode == 1) {
        const int grid = grid_for(a.s.n, HF_XFORM_GRID_CAP); // the slab holds HF_XFORM_GRID_CAP rows
        hipLaunchKernelGGL(hf_thinlens_adjoint_kernel, dim3(grid), dim3(HF_BLOCK), 0, stream, a);
        hipLaunchKernelGGL(hf_thinlens_sum_kernel, dim3(1), dim3(HF_BLOCK), 0, stream, a.s.slab, (uint32_t) grid, a.s.dtau,
                           a.s.g_tw, a.s.g_fov, a.g_radius, a.g_focus);
        return;
    }
    if (mode == 0 && sensor_wide_store() && a.s.n >= 64) {
        hf_thinlens_args w = a;
        const size_t groups = sensor_wide_groups(w.s);
        hipLaunchKernelGGL(hf_thinlens_rays_wide_kernel, dim3(grid_for(groups, HF_SI_GRID_CAP)), dim3(HF_BLOCK), 0, stream, w);
        return;
    }
    hipLaunchKernelGGL(mode == 0 ? hf_thinlens_rays_kernel : hf_thinlens_tangent_kernel, dim3(grid_for(a.s.n, HF_SI_GRID_CAP)),
                       dim3(HF_BLOCK), 0, stream, a);
}

// ---- the way back: thin-lens sample_direction (thinlens.cpp:305-350) with the lane's own aperture draw ----
struct hf_lens_proj {
    bool inside, valid;
    double x, y, z;      // ref = to_world^-1 p
    double Dx, Dy;
    double qx, qy;       // q = ref - r D (q.z = ref.z)
    double iz, mx, my;   // 1 / q.z, q.x / q.z, q.y / q.z
    double kx, ky;       // F / f = (r / f) D + m
    double u, v, r2, W;  // uv; |q|^2; |q| / (A' q.z^3)
};
__device__ __forceinline__ hf_lens_proj thinlens_project(const hf_thinlens_project_args &b, size_t i) {
    const hf_sensor_project_args &a = b.s;
    hf_lens_proj r;
    const double q0 = (double) a.p[0][i] - a.c[0], q1 = (double) a.p[1][i] - a.c[1], q2 = (double) a.p[2][i] - a.c[2];
    r.x = a.Ai[0] * q0 + a.Ai[1] * q1 + a.Ai[2] * q2;
    r.y = a.Ai[3] * q0 + a.Ai[4] * q1 + a.Ai[5] * q2;
    r.z = a.Ai[6] * q0 + a.Ai[7] * q1 + a.Ai[8] * q2;
    r.inside = (!a.active || a.active[i] != 0) && r.z >= a.near && r.z <= a.far;   // thinlens.cpp:315
    const hf_lens_disk D = thinlens_disk(b.key, b.ray_id ? b.ray_id[i] : b.start + (uint32_t) i);
    r.Dx = D.x; r.Dy = D.y;
    r.qx = r.x - b.radius * D.x; r.qy = r.y - b.radius * D.y;                      // :324
    r.iz = 1.0 / r.z; r.mx = r.qx * r.iz; r.my = r.qy * r.iz;
    r.kx = (b.radius / b.focus) * D.x + r.mx; r.ky = (b.radius / b.focus) * D.y + r.my; // :333 over f
    r.u = 0.5 * (1.0 - r.kx / a.tau) * a.film_w;
    r.v = 0.5 * (1.0 - a.aspect * r.ky / a.tau) * a.film_h;
    const double sx = (r.u - a.crop_x) / a.crop_w, sy = (r.v - a.crop_y) / a.crop_h;
    r.valid = r.inside && sx >= 0.0 && sx <= 1.0 && sy >= 0.0 && sy <= 1.0;        // :334
    r.r2 = r.qx * r.qx + r.qy * r.qy + r.z * r.z;
    r.W = __builtin_sqrt(r.r2) * a.inv_area * (r.iz * r.iz * r.iz);                // :335, 349
    return r;
}
__global__ __launch_bounds__(HF_BLOCK) void hf_thinlens_project_kernel(hf_thinlens_project_args b) {
    const hf_sensor_project_args &a = b.s;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += (size_t) gridDim.x * HF_BLOCK) {
        const hf_lens_proj r = thinlens_project(b, i);
        a.uv[0][i] = r.inside ? (float) r.u : 0.f;
        a.uv[1][i] = r.inside ? (float) r.v : 0.f;
        a.valid[i] = r.valid ? 1 : 0;
        if (a.weight) a.weight[i] = r.valid ? (float) r.W : 0.f;
    }
}
__global__ __launch_bounds__(HF_BLOCK) void hf_thinlens_project_tangent_kernel(hf_thinlens_project_args b) {
    const hf_sensor_project_args &a = b.s;
    double dM[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) dM[j] = a.d_tw ? (double) a.d_tw[j] : 0.0;
    const double dT = (a.d_fov ? (double) a.d_fov[0] * a.dtau : 0.0) / a.tau; // d tau / tau
    const double dr = b.d_radius ? (double) b.d_radius[0] : 0.0, df = b.d_focus ? (double) b.d_focus[0] : 0.0;
    const double dk = dr / b.focus - b.radius * df / (b.focus * b.focus);      // d (r / f)
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += (size_t) gridDim.x * HF_BLOCK) {
        const hf_lens_proj r = thinlens_project(b, i);
        double dq[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) // dp - dA ref - dc
            dq[k] = (a.dp[k] ? (double) a.dp[k][i] : 0.0) - (dM[4 * k] * r.x + dM[4 * k + 1] * r.y + dM[4 * k + 2] * r.z) - dM[4 * k + 3];
        // dq = d ref - D dr
        const double dx = a.Ai[0] * dq[0] + a.Ai[1] * dq[1] + a.Ai[2] * dq[2] - r.Dx * dr;
        const double dy = a.Ai[3] * dq[0] + a.Ai[4] * dq[1] + a.Ai[5] * dq[2] - r.Dy * dr;
        const double dz = a.Ai[6] * dq[0] + a.Ai[7] * dq[1] + a.Ai[8] * dq[2];
        const double dkx = dk * r.Dx + (dx - r.mx * dz) * r.iz, dky = dk * r.Dy + (dy - r.my * dz) * r.iz;
        const double cu = -0.5 * a.film_w / a.tau, cv = -0.5 * a.film_h * a.aspect / a.tau;
        a.uv[0][i] = r.inside ? (float) (cu * (dkx - r.kx * dT)) : 0.f;
        a.uv[1][i] = r.inside ? (float) (cv * (dky - r.ky * dT)) : 0.f;
        if (a.weight)
            a.weight[i] = r.valid ? (float) (r.W * ((r.qx * dx + r.qy * dy + r.z * dz) / r.r2 - 3.0 * dz * r.iz - 2.0 * dT)) : 0.f;
    }
}
// sums 0..11: to_world, 12: ln tau, 13: r, 14: f
__global__ __launch_bounds__(HF_BLOCK) void hf_thinlens_project_adjoint_kernel(hf_thinlens_project_args b) {
    const hf_sensor_project_args &a = b.s;
    double M[HF_THINLENS_SUMS];
#pragma unroll
    for (int j = 0; j < HF_THINLENS_SUMS; ++j) M[j] = 0.0;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += (size_t) gridDim.x * HF_BLOCK) {
        const hf_lens_proj r = thinlens_project(b, i);
        const double cu = -0.5 * a.film_w / a.tau, cv = -0.5 * a.film_h * a.aspect / a.tau;
        const double gkx = r.inside && a.guv[0] ? cu * (double) a.guv[0][i] : 0.0;  // dL/d(F / f)
        const double gky = r.inside && a.guv[1] ? cv * (double) a.guv[1][i] : 0.0;
        const double gW = r.valid && a.gweight ? r.W * (double) a.gweight[i] : 0.0;
        // dL/dq (= dL/dref)
        const double gx = gkx * r.iz + gW * r.qx / r.r2;
        const double gy = gky * r.iz + gW * r.qy / r.r2;
        const double gz = -(gkx * r.mx + gky * r.my) * r.iz + gW * (r.z / r.r2 - 3.0 * r.iz);
        double h[3]; // to_world^-T dL/dref = dL/dp (zero outside the clip range: every term above is)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            h[k] = r.inside ? a.Ai[k] * gx + a.Ai[3 + k] * gy + a.Ai[6 + k] * gz : 0.0;
            if (a.gp[k]) a.gp[k][i] = (float) h[k];
            M[4 * k] -= h[k] * r.x; M[4 * k + 1] -= h[k] * r.y; M[4 * k + 2] -= h[k] * r.z; M[4 * k + 3] -= h[k];
        }
        if (r.inside) {
            const double gD = gkx * r.Dx + gky * r.Dy;
            M[12] -= gkx * r.kx + gky * r.ky + 2.0 * gW;
            M[13] += gD / b.focus - (gx * r.Dx + gy * r.Dy);
            M[14] -= gD * b.radius / (b.focus * b.focus);
        }
    }
    sensor_block_store<HF_THINLENS_SUMS>(M, a.slab);
}

void hf_launch_thinlens_project(int mode, const hf_thinlens_project_args &args, hipStream_t stream) {
    hf_thinlens_project_args a = args;
    a.key = thinlens_key(a.seed);
    if (mode == 1) {
        const int grid = grid_for(a.s.n, HF_XFORM_GRID_CAP);
        hipLaunchKernelGGL(hf_thinlens_project_adjoint_kernel, dim3(grid), dim3(HF_BLOCK), 0, stream, a);
        // column 12 holds dL/d(ln tau): times d tau / tau per degree
        hipLaunchKernelGGL(hf_thinlens_sum_kernel, dim3(1), dim3(HF_BLOCK), 0, stream, a.s.slab, (uint32_t) grid,
                           a.s.dtau / a.s.tau, a.s.g_tw, a.s.g_fov, a.g_radius, a.g_focus);
        return;
    }
    hipLaunchKernelGGL(mode == 0 ? hf_thinlens_project_kernel : hf_thinlens_project_tangent_kernel,
                       dim3(grid_for(a.s.n, HF_SI_GRID_CAP)), dim3(HF_BLOCK), 0, stream, a);
}

// ---------------------------------------------------------------------------------
// Projector lighting (include/hf.h hf_projector_*): diffuse surface under a `projector` emitter, the
// reciprocal of the perspective sensor: a pinhole at to_world's c that throws the texture onto the terrain.  One draw per
// sample (the pinhole is a point): the frustum mapping p -> uv, the bilinear lookup, the shadow ray towards c
// (Interaction::spawn_ray_to, a FINITE maxt) traced (any hit, per lane) and the film in ONE launch, hf_refract_kernel's
// and hf_rect_kernel's shape:
//   value = weight albedo scale I(uv) G,   G = <sh_n, c - p> / ref.z^3.
// The row's own text is the mapping, G and their derivatives with the pose, the field of view and the scale; the masks,
// the origin, the walk, the film, the outputs, the tangent shell and the launch are the lighting rows' shared functions,
// the lookup with its scatter / gather the refraction view's (bitmap_cell), the reduction of the 14 pose numbers the
// sensor's (sensor_block_store, sensor_slab_sums).
// (P below: a pointer to hf_projector_args, in the kernarg segment or not)
// ---------------------------------------------------------------------------------
typedef const __attribute__((address_space(4))) hf_projector_args *hf_projector_kargs;

// The mapping (projector.cpp:209-214) in double from the float32 point: ref = to_world^-1 p, uv = camera_to_sample of
// ref / ref.z (hf_sensor_project's expressions in units of the whole film), lit = ref.z > 0 and uv in [0, 1]^2
struct hf_projector_map {
    double x, y, z;    // ref
    double iz, rx, ry; // 1 / ref.z, ref.x / ref.z, ref.y / ref.z
    double u, v;       // uv
    bool lit;
};
template <class P>
__device__ __forceinline__ hf_projector_map projector_map(P a, v3 p) {
    hf_projector_map m;
    const double q0 = (double) p.x - a->c[0], q1 = (double) p.y - a->c[1], q2 = (double) p.z - a->c[2];
    m.x = a->Ai[0] * q0 + a->Ai[1] * q1 + a->Ai[2] * q2;
    m.y = a->Ai[3] * q0 + a->Ai[4] * q1 + a->Ai[5] * q2;
    m.z = a->Ai[6] * q0 + a->Ai[7] * q1 + a->Ai[8] * q2;
    m.iz = 1.0 / m.z; m.rx = m.x * m.iz; m.ry = m.y * m.iz;
    m.u = 0.5 * (1.0 - m.rx / a->tau);
    m.v = 0.5 * (1.0 - a->aspect * m.ry / a->tau);
    m.lit = m.z > 0.0 && m.u >= 0.0 && m.u <= 1.0 && m.v >= 0.0 && m.v <= 1.0;
    return m;
}
// u = c - p in double, for the shading sums (G's numerator is <sh_n, u>)
template <class P>
__device__ __forceinline__ hf_d3 projector_to_c(P a, v3 p) {
    return hf_d3{ a->c[0] - (double) p.x, a->c[1] - (double) p.y, a->c[2] - (double) p.z };
}
// the texel coordinate of a lit point: (uv.x TW, uv.y TH), rounded once to float32 (hf_sensor_project's uv for a film of
// TW x TH), then hf_bitmap_eval's float32 lookup
template <class P>
__device__ __forceinline__ hf_bitmap_cell projector_cell(P a, const hf_projector_map &m) {
    return bitmap_cell(a, (float) (m.u * (double) a->TW), (float) (m.v * (double) a->TH));
}
// The float32 side, what the ray takes: u = c - p with c rounded to float32; front: <sh_n, u> > 0 and |u|^2 finite and > 0
__device__ __forceinline__ bool projector_front(v3 cf, v3 p, v3 sn) {
    const v3 u = cf - p;
    const float r2 = dot3(u, u);
    return dot3(sn, u) > 0.f && r2 > 0.f && r2 < __builtin_inff();
}
// spawn_ray_to(c) (hf_rect_rays' ray with the lamp's point at c): the origin offset_p(u), the direction (c - o) / |c - o|
// and maxt = |c - o| (1 - ShadowEpsilon)
struct hf_projector_ray { v3 o, w; float maxt; };
__device__ __forceinline__ hf_projector_ray projector_ray(v3 cf, v3 p, v3 gn, float mag) {
    hf_projector_ray r;
    r.o = sky_origin(p, gn, mag, cf - p);
    const v3 dv = cf - r.o;
    const float dist = __builtin_sqrtf(dot3(dv, dv));
    r.w = dv * (1.0f / dist);
    r.maxt = dist * (1.f - 8.940696716308594e-04f);
    return r;
}

#ifndef HF_PROJECTOR_WAVES
#define HF_PROJECTOR_WAVES 6 // resident waves per SIMD (the siblings')
#endif
__global__ __launch_bounds__(HF_BLOCK, HF_PROJECTOR_WAVES) void hf_projector_kernel(hf_projector_args a) {
    const hf_dev_field &f = a.f;
    // hf_sky_kernel's mapping: n < 2^32, the sample index is one register across the walk
    const size_t i64 = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const bool in = i64 < a.n;
    const uint32_t i = (uint32_t) i64;
    const uint32_t ii = in ? i : (uint32_t) (a.n - 1);
    hf_projector_kargs ka = (hf_projector_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    float val = 0.f; // the value of a sample that turns out visible: finished before the ray is begun, held across the walk
    bool traced;
    hf_hit best;
    best.hit = false;
    {
        const v3 sn = mk3(ka->sh_n[0][ii], ka->sh_n[1][ii], ka->sh_n[2][ii]);
        bool elig;
        {
            const v3 d = mk3(ka->d[0][ii], ka->d[1][ii], ka->d[2][ii]);
            elig = in && sky_eligible(ka->t[ii], sn, d);
        }
        const v3 p = mk3(ka->p[0][ii], ka->p[1][ii], ka->p[2][ii]);
        bool lit;
        { // the doubles and the four texel addresses are dead when setup_ray's registers fill; uv is stored here
            const hf_projector_map m = projector_map(ka, p);
            lit = m.lit;
            float *ux = ka->uv[0], *uy = ka->uv[1];
            if (in && ux) {
                const bool facing = m.z > 0.0;
                ux[i] = facing ? (float) m.u : 0.f; uy[i] = facing ? (float) m.v : 0.f;
            }
            if (elig && lit) {
                const double iz3 = m.iz * m.iz * m.iz;
                double v = ka->cs * (sky_dot_f64(sn, projector_to_c(ka, p)) * iz3);
                const float *tex = ka->tex, *weight = ka->weight;
                if (tex) v *= (double) projector_cell(ka, m).value(tex); // (wave-uniform)
                if (weight) v *= (double) weight[ii];
                val = (float) v;
            }
        }
        asm volatile("" : "+v"(val));
        const v3 cf = mk3(ka->cf[0], ka->cf[1], ka->cf[2]);
        traced = elig && lit && projector_front(cf, p, sn);
        if (__ballot(traced) != 0ull) { // wave-uniform: a batch without a traced sample walks nothing
            const v3 gn = mk3(ka->nrm[0][ii], ka->nrm[1][ii], ka->nrm[2][ii]);
            const hf_projector_ray r = projector_ray(cf, p, gn, sky_offset(p));
            light_walk<true>(&ka->f, f, r.o, r.w, r.maxt, traced, best);
        }
    }
    // (the output pointers: loaded here, not before the walk)
    hf_projector_kargs ko = (hf_projector_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ko));
    const bool seen = traced && !best.hit; // (traced: in range)
    if (!seen) val = 0.f;
    if (in) {
        float *value = ko->value;
        uint8_t *vis = ko->vis;
        if (value) value[i] = val;
        if (vis) vis[i] = seen ? 1 : 0;
    }
    float *image = ko->image;
    if (image) {
        const uint32_t spp = ko->spp, g = spp < 64u ? spp : 64u;
        film_pixel(image, val, 0u, ko->n / spp, i, spp, in, (spp & (spp - 1u)) == 0u, g, 1.0f / (float) spp, i);
    }
}

// the shadow ray of every sample, materialised: what hf_projector_kernel traces, bit for bit (an untraced lane: a zero
// origin and direction, maxt = -1)
__global__ __launch_bounds__(HF_BLOCK) void hf_projector_rays_kernel(hf_projector_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    v3 sn;
    const bool elig = light_sample(a, i, sn);
    const v3 p = mk3(a.p[0][i], a.p[1][i], a.p[2][i]), gn = mk3(a.nrm[0][i], a.nrm[1][i], a.nrm[2][i]);
    const v3 cf = mk3(a.cf[0], a.cf[1], a.cf[2]);
    const bool traced = elig && projector_map(&a, p).lit && projector_front(cf, p, sn);
    const hf_projector_ray r = projector_ray(cf, p, gn, sky_offset(p));
    const v3 z = mk3(0.f, 0.f, 0.f);
    light_store_ray(a, i, traced ? r.o : z, traced ? r.w : z, traced, r.maxt);
}

// What the two derivative kernels form again of a visible sample: the mapping, u = c - p, <sh_n, u>, G, the cell of the
// lookup, I (1 without a texture) and dI/duv = (Lx TW, Ly TH) with the cell held
struct hf_projector_shade {
    hf_projector_map m;
    hf_bitmap_cell e;
    hf_d3 u;
    double iz3, G, I, Iu, Iv;
};
__device__ __forceinline__ hf_projector_shade projector_shade(const hf_projector_args &a, v3 p, v3 sn) {
    hf_projector_shade s;
    s.m = projector_map(&a, p);
    s.u = projector_to_c(&a, p);
    s.iz3 = s.m.iz * s.m.iz * s.m.iz;
    s.G = sky_dot_f64(sn, s.u) * s.iz3;
    s.I = 1.0; s.Iu = 0.0; s.Iv = 0.0;
    if (a.tex) {
        s.e = projector_cell(&a, s.m);
        float Lx, Ly;
        s.e.slopes(a.tex, Lx, Ly);
        s.I = (double) s.e.value(a.tex);
        s.Iu = (double) Lx * (double) a.TW; s.Iv = (double) Ly * (double) a.TH;
    }
    return s;
}

// Reverse mode of hf_projector_kernel with respect to sh_n, p, weight, the texels, to_world, x_fov and scale: nothing is
// traced, the visibility byte is read.  grad_sh_n, grad_p, grad_weight: one lane per sample, overwritten, no atomics;
// grad_tex: one float atomic per texel of every visible sample; the 14 pose numbers (to_world's 12, ln tau's, scale's)
// are kept per lane in double across the grid-stride loop and reduced as the sensor's 13
#define HF_PROJECTOR_SUMS 14
__global__ __launch_bounds__(HF_BLOCK) void hf_projector_adjoint_kernel(hf_projector_args a) {
    double M[HF_PROJECTOR_SUMS];
#pragma unroll
    for (int j = 0; j < HF_PROJECTOR_SUMS; ++j) M[j] = 0.0;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += (size_t) gridDim.x * HF_BLOCK) {
        v3 gn = mk3(0.f, 0.f, 0.f), gp = gn;
        float gw = 0.f;
        if (a.vis[i]) {
            const v3 sn = mk3(a.sh_n[0][i], a.sh_n[1][i], a.sh_n[2][i]), p = mk3(a.p[0][i], a.p[1][i], a.p[2][i]);
            const hf_projector_shade s = projector_shade(a, p, sn);
            if (s.m.lit) { // (a visible sample is lit: the guard of the divisions by ref.z)
                const double g = (double) light_value_seed(a, i), w = a.weight ? (double) a.weight[i] : 1.0;
                const double gV = g * s.I * s.G; // dL/d(weight albedo scale)
                gw = (float) (gV * a.cs);
                M[13] += gV * w * a.albedo;
                const double gG = (g * w * a.cs) * s.I, gI = (g * w * a.cs) * s.G; // dL/dG, dL/dI
                // dL/d(ref.x / ref.z), dL/d(ref.y / ref.z) through uv, then dL/dref
                const double grx = gI * s.Iu * (-0.5 / a.tau), gry = gI * s.Iv * (-0.5 * a.aspect / a.tau);
                const double gx = grx * s.m.iz, gy = gry * s.m.iz;
                const double gz = -(grx * s.m.rx + gry * s.m.ry) * s.m.iz - 3.0 * gG * s.G * s.m.iz;
                const double gu = gG * s.iz3; // dL/d<sh_n, u>
                const double n3[3] = { (double) sn.x, (double) sn.y, (double) sn.z }, u3[3] = { s.u.x, s.u.y, s.u.z };
                float o_n[3], o_p[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double h = a.Ai[k] * gx + a.Ai[3 + k] * gy + a.Ai[6 + k] * gz; // to_world^-T dL/dref
                    o_n[k] = (float) (gu * u3[k]);
                    o_p[k] = (float) (h - gu * n3[k]);
                    M[4 * k] -= h * s.m.x; M[4 * k + 1] -= h * s.m.y; M[4 * k + 2] -= h * s.m.z;
                    M[4 * k + 3] += gu * n3[k] - h;
                }
                M[12] -= grx * s.m.rx + gry * s.m.ry;
                gn = mk3(o_n[0], o_n[1], o_n[2]); gp = mk3(o_p[0], o_p[1], o_p[2]);
                if (a.tex && a.gdata) s.e.scatter(a.gdata, (float) gI);
            }
        }
        light_store_grads(a, i, gn, gp, gw);
    }
    if (a.slab) sensor_block_store<HF_PROJECTOR_SUMS>(M, a.slab); // (launch-uniform: no reduced gradient is wanted)
}
// g_tw[j] += column j, g_fov[0] += column 12 times d tau / tau per degree, g_scale[0] += column 13.  One block.
__global__ __launch_bounds__(HF_BLOCK) void hf_projector_sum_kernel(const double *__restrict__ slab, uint32_t rows, double dtau,
                                                                     float *__restrict__ g_tw, float *__restrict__ g_fov,
                                                                     float *__restrict__ g_scale) {
    const double *const sum = sensor_slab_sums<HF_PROJECTOR_SUMS>(slab, rows);
    const uint32_t t = threadIdx.x;
    if (t < 12u) {
        if (g_tw) g_tw[t] += (float) sum[t];
    } else if (t == 12u) {
        if (g_fov) g_fov[0] += (float) (sum[12] * dtau);
    } else if (t == 13u) {
        if (g_scale) g_scale[0] += (float) sum[13];
    }
}
size_t hf_projector_slab_doubles() { return (size_t) HF_XFORM_GRID_CAP * HF_PROJECTOR_SUMS; }

// forward mode, the transpose of the above: the tangent of sample i's value for tangents dn of sh_n, dp of p, dw of
// weight, dtex of the texels, d_tw of to_world, d_fov and d_scale (NULL: zero)
__device__ __forceinline__ float projector_tangent_value(const hf_projector_args &a, size_t i) {
    if (!a.vis[i]) return 0.f;
    const v3 sn = mk3(a.sh_n[0][i], a.sh_n[1][i], a.sh_n[2][i]), p = mk3(a.p[0][i], a.p[1][i], a.p[2][i]);
    const hf_projector_shade s = projector_shade(a, p, sn);
    if (!s.m.lit) return 0.f;
    const v3 dn = a.dn[0] ? mk3(a.dn[0][i], a.dn[1][i], a.dn[2][i]) : mk3(0.f, 0.f, 0.f);
    const double dp[3] = { a.dp[0] ? (double) a.dp[0][i] : 0.0, a.dp[1] ? (double) a.dp[1][i] : 0.0, a.dp[2] ? (double) a.dp[2][i] : 0.0 };
    const double n3[3] = { (double) sn.x, (double) sn.y, (double) sn.z };
    const double dT = (a.d_fov ? (double) a.d_fov[0] * a.dtau : 0.0) / a.tau; // d tau / tau
    double dq[3], dnu = sky_dot_f64(dn, s.u); // dp - dA ref - dc; d<sh_n, u>
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double dA0 = 0.0, dA1 = 0.0, dA2 = 0.0, dc = 0.0;
        if (a.d_tw) { dA0 = (double) a.d_tw[4 * k]; dA1 = (double) a.d_tw[4 * k + 1]; dA2 = (double) a.d_tw[4 * k + 2]; dc = (double) a.d_tw[4 * k + 3]; }
        dq[k] = dp[k] - (dA0 * s.m.x + dA1 * s.m.y + dA2 * s.m.z) - dc;
        dnu += n3[k] * (dc - dp[k]);
    }
    const double dx = a.Ai[0] * dq[0] + a.Ai[1] * dq[1] + a.Ai[2] * dq[2];
    const double dy = a.Ai[3] * dq[0] + a.Ai[4] * dq[1] + a.Ai[5] * dq[2];
    const double dz = a.Ai[6] * dq[0] + a.Ai[7] * dq[1] + a.Ai[8] * dq[2];
    const double drx = (dx - s.m.rx * dz) * s.m.iz, dry = (dy - s.m.ry * dz) * s.m.iz;
    double dI = s.Iu * ((-0.5 / a.tau) * (drx - s.m.rx * dT)) + s.Iv * ((-0.5 * a.aspect / a.tau) * (dry - s.m.ry * dT));
    if (a.tex && a.ddata) dI += (double) s.e.value(a.ddata);
    const double dG = dnu * s.iz3 - 3.0 * s.G * dz * s.m.iz;
    const double w = a.weight ? (double) a.weight[i] : 1.0;
    const double dwc = (a.dw ? (double) a.dw[i] : 0.0) * a.cs + w * ((a.d_scale ? (double) a.d_scale[0] : 0.0) * a.albedo);
    return (float) (dwc * (s.I * s.G) + (w * a.cs) * (dI * s.G + s.I * dG));
}
// (the per-sample tangent is written too, and the image may be NULL)
template <bool PIXEL>
__global__ __launch_bounds__(HF_BLOCK) void hf_projector_tangent_kernel(hf_projector_args a) {
    light_tangent_image<PIXEL, hf_projector_args, projector_tangent_value>(a, a.value);
}

// mode 0: forward, 1: adjoint (and, where a reduced gradient is wanted, the sum of the blocks' rows), 2: tangent, 3: rays
void hf_launch_projector(int mode, const hf_projector_args &a, hipStream_t stream) {
    if (mode == 1) {
        if (a.n == 0) return;
        const int grid = grid_for(a.n, HF_XFORM_GRID_CAP); // the slab holds HF_XFORM_GRID_CAP rows
        hipLaunchKernelGGL(hf_projector_adjoint_kernel, dim3(grid), dim3(HF_BLOCK), 0, stream, a);
        // column 12 holds dL/d(ln tau): times d tau / tau per degree
        if (a.slab)
            hipLaunchKernelGGL(hf_projector_sum_kernel, dim3(1), dim3(HF_BLOCK), 0, stream, a.slab, (uint32_t) grid, a.dtau / a.tau,
                               a.g_tw, a.g_fov, a.g_scale);
        return;
    }
    launch_light(mode, a, 1u, stream, hf_projector_kernel, hf_projector_adjoint_kernel, hf_projector_tangent_kernel<false>,
                 hf_projector_tangent_kernel<true>, hf_projector_rays_kernel);
}

// ---------------------------------------------------------------------------------
// Spot lighting (include/hf.h hf_spot_*): diffuse surface under a RIG of 1..HF_MAX_LIGHTS `spot` emitters
// (src/emitters/spot.cpp), cones with a linear falloff between beam_width and cutoff_angle.  Every light is a point, so
// there is one draw per sample and light: the cone mapping p -> theta, the falloff, the shadow ray towards c
// (the projector's, Interaction::spawn_ray_to) traced (any hit, per lane) and the film, for ALL lights in ONE launch:
// the sample's record is read once and held across a wave-uniform loop over the lights (hf_sky_kernel's k loop),
//   value_k = weight albedo / pi intensity_k f_k <sh_n, u> / |u|^3,   u = c_k - p.
// The row's own text is the mapping, the falloff and their derivatives; the masks, the origin, the ray, the walk, the
// film and the launch are the lighting rows' and the projector's shared functions, the reduction of the 15 numbers of
// every light the sensor's (sensor_block_store, sensor_slab_sums).
// (LP below: a pointer to one hf_spot_light_dev, in the kernarg segment or not)
// ---------------------------------------------------------------------------------
typedef const __attribute__((address_space(4))) hf_spot_args *hf_spot_kargs;

// The mapping (spot.cpp:183-198) in double from the float32 point: ref = to_world^-1 p, cos(theta) = ref.z / |ref|, and
// falloff_curve (:143-151) with theta = atan2(hypot(ref.x, ref.y), ref.z) (spot_theta): the acos of the cosine, better
// conditioned.
// The sums are written as fma chains: the forward and the rays kernel must form the same bits
struct hf_spot_map {
    double x, y, z; // ref
    double r2;      // |ref|^2
    double f;       // the falloff of the branch the point is on: 1 in the full beam, the ramp elsewhere (the cone is `lit`'s)
    bool full, lit; // cos(theta) >= cos(beam); in the cone with f > 0
};
// theta = atan2(rho, z) for rho >= 0, in [0, pi]: t = min / max of (rho, |z|), folded once more about tan(pi / 8) with
// the same single division ((t - 1) / (t + 1) = (min - max) / (min + max)), then an odd polynomial of degree 19 whose
// error on [0, tan(pi / 8)] is 7e-16.  C: its ten coefficients, tan(pi / 8), pi / 4, pi / 2 and pi -- fourteen doubles of
// the kernarg segment, scalar operands: the library's atan2 keeps twenty-one constants in vector registers, which the
// loop over the lights hoists and then spills (43 registers of hf_spot_kernel)
template <class CP>
__device__ __forceinline__ double spot_theta(CP C, double rho, double z) {
    const double az = fabs(z), lo = fmin(rho, az), hi = fmax(rho, az);
    const bool fold = lo > C[10] * hi;
    const double t = (fold ? lo - hi : lo) / (fold ? lo + hi : hi), s = t * t;
    double q = C[9];
#pragma unroll
    for (int j = 8; j >= 0; --j) q = fma(q, s, C[j]);
    double r = q * t;
    if (fold) r += C[11];
    if (rho > az) r = C[12] - r;
    if (z < 0.0) r = C[13] - r;
    return r;
}
template <class LP, class CP>
__device__ __forceinline__ hf_spot_map spot_map(LP L, CP C, v3 p) {
    hf_spot_map m;
    const double q0 = (double) p.x - L->c[0], q1 = (double) p.y - L->c[1], q2 = (double) p.z - L->c[2];
    m.x = fma(L->Ai[0], q0, fma(L->Ai[1], q1, L->Ai[2] * q2));
    m.y = fma(L->Ai[3], q0, fma(L->Ai[4], q1, L->Ai[5] * q2));
    m.z = fma(L->Ai[6], q0, fma(L->Ai[7], q1, L->Ai[8] * q2));
    const double rho2 = fma(m.x, m.x, m.y * m.y);
    m.r2 = fma(m.z, m.z, rho2);
    const double co = m.z / sqrt(m.r2); // (NaN at the apex: in no cone)
    m.full = co >= L->cos_beam;
    m.f = 1.0;
    if (!m.full) m.f = (L->cutoff - spot_theta(C, sqrt(rho2), m.z)) * L->inv_width; // (a hard edge: inv_width = 0, no division)
    m.lit = co > L->cos_cutoff && m.f > 0.0;
    return m;
}

#ifndef HF_SPOT_WAVES
#define HF_SPOT_WAVES 6 // resident waves per SIMD (the siblings')
#endif
__global__ __launch_bounds__(HF_BLOCK, HF_SPOT_WAVES) void hf_spot_kernel(hf_spot_args a) {
    const hf_dev_field &f = a.f;
    // hf_sky_kernel's mapping: n < 2^32, the sample index is one register across the walk
    const size_t i64 = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const bool in = i64 < a.n;
    const uint32_t i = (uint32_t) i64;
    const uint32_t ii = in ? i : (uint32_t) (a.n - 1);
    hf_spot_kargs ka = (hf_spot_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    // the sample's record: read once, held across the loop over the lights
    const v3 sn = mk3(ka->sh_n[0][ii], ka->sh_n[1][ii], ka->sh_n[2][ii]);
    bool elig;
    {
        const v3 d = mk3(ka->d[0][ii], ka->d[1][ii], ka->d[2][ii]);
        elig = in && sky_eligible(ka->t[ii], sn, d);
    }
    const v3 p = mk3(ka->p[0][ii], ka->p[1][ii], ka->p[2][ii]);
    const v3 gn = mk3(ka->nrm[0][ii], ka->nrm[1][ii], ka->nrm[2][ii]);
    float wgt = 1.f;
    {
        const float *weight = ka->weight;
        if (weight) wgt = weight[ii];
    }
    uint32_t bits = 0u; // bit k: the sample was traced towards light k and nothing is in the way
#pragma unroll 1
    for (uint32_t k = 0;; ++k) { // wave-uniform loop, the lanes predicated inside
        asm volatile("" : "+s"(ka)); // opaque per light: the kernarg loads stay inside the loop
        // light k's value of a sample that turns out visible: finished and rounded before the ray is begun (the
        // projector kernel's discipline), one float held across the walk
        float val = 0.f;
        bool lit = false;
        {
            v3 pd = p, snd = sn; // (opaque: the conversions to double are otherwise hoisted out of the loop and held across the walk)
            asm volatile("" : "+v"(pd.x), "+v"(pd.y), "+v"(pd.z), "+v"(snd.x), "+v"(snd.y), "+v"(snd.z));
            if (elig) {
                const hf_spot_map m = spot_map(&ka->L[k], &ka->atan_c[0], pd);
                lit = m.lit;
                if (lit) {
                    const hf_d3 u = hf_d3{ ka->L[k].c[0] - (double) pd.x, ka->L[k].c[1] - (double) pd.y, ka->L[k].c[2] - (double) pd.z };
                    const double r2 = fma(u.x, u.x, fma(u.y, u.y, u.z * u.z));
                    val = (float) ((double) wgt * (ka->L[k].ci * m.f) * (sky_dot_f64(snd, u) / (r2 * sqrt(r2))));
                }
            }
        }
        asm volatile("" : "+v"(val));
        const v3 cf = mk3(ka->L[k].cf[0], ka->L[k].cf[1], ka->L[k].cf[2]);
        const bool traced = elig && lit && projector_front(cf, p, sn);
        hf_hit best;
        best.hit = false;
        if (__ballot(traced) != 0ull) { // wave-uniform: a batch without a sample traced towards this light skips its walk
            const hf_projector_ray r = projector_ray(cf, p, gn, sky_offset(p));
            light_walk<true>(&ka->f, f, r.o, r.w, r.maxt, traced, best);
        }
        // (the output pointers: loaded here, not before the walk)
        hf_spot_kargs ko = (hf_spot_kargs) __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ko));
        const bool seen = traced && !best.hit; // (traced: in range)
        if (!seen) val = 0.f;
        if (seen) bits |= 1u << k;
        float *value = ko->value;
        if (in && value) value[(size_t) k * ko->n + i] = val;
        float *image = ko->image;
        if (image) { // the film of light k: hf_point_lighting's layout, K images of n / spp
            const uint32_t spp = ko->spp, g = spp < 64u ? spp : 64u;
            film_pixel(image, val, k, ko->n / spp, i, spp, in, (spp & (spp - 1u)) == 0u, g, 1.0f / (float) spp, i);
        }
        if (k + 1u >= ko->n_lights) break;
    }
    hf_spot_kargs ko = (hf_spot_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ko));
    uint8_t *vis = ko->vis;
    if (in && vis) vis[i] = (uint8_t) bits;
}

// the shadow ray of every sample towards ONE light (L[0]), materialised: what hf_spot_kernel traces for it, bit for bit
// (an untraced lane: a zero origin and direction, maxt = -1)
__global__ __launch_bounds__(HF_BLOCK) void hf_spot_rays_kernel(hf_spot_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    hf_spot_kargs ka = (hf_spot_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    v3 sn;
    const bool elig = light_sample(a, i, sn);
    const v3 p = mk3(a.p[0][i], a.p[1][i], a.p[2][i]), gn = mk3(a.nrm[0][i], a.nrm[1][i], a.nrm[2][i]);
    const v3 cf = mk3(ka->L[0].cf[0], ka->L[0].cf[1], ka->L[0].cf[2]);
    const bool traced = elig && spot_map(&ka->L[0], &ka->atan_c[0], p).lit && projector_front(cf, p, sn);
    const hf_projector_ray r = projector_ray(cf, p, gn, sky_offset(p));
    const v3 z = mk3(0.f, 0.f, 0.f);
    light_store_ray(a, i, traced ? r.o : z, traced ? r.w : z, traced, r.maxt);
}

// What the two derivative kernels form again of a sample whose bit for light L is set: the mapping (the branch of the
// falloff is the one the point is on, the cone is the bit's), u = c - p, S = <sh_n, u>, |u|^-2, |u|^-3 and G = S / |u|^3
struct hf_spot_shade {
    hf_spot_map m;
    hf_d3 u;
    double S, ir2, ir3, G;
    bool ok; // the guard of the divisions: a sample that hf_spot_kernel found visible passes it
};
template <class LP, class CP>
__device__ __forceinline__ hf_spot_shade spot_shade(LP L, CP C, v3 p, v3 sn) {
    hf_spot_shade s;
    s.m = spot_map(L, C, p);
    s.u = hf_d3{ L->c[0] - (double) p.x, L->c[1] - (double) p.y, L->c[2] - (double) p.z };
    s.S = sky_dot_f64(sn, s.u);
    const double r2 = fma(s.u.x, s.u.x, fma(s.u.y, s.u.y, s.u.z * s.u.z));
    s.ir2 = 1.0 / r2; s.ir3 = s.ir2 / sqrt(r2);
    s.G = s.S * s.ir3;
    s.ok = r2 > 0.0 && s.m.r2 > 0.0 && (s.m.full || fma(s.m.x, s.m.x, s.m.y * s.m.y) > 0.0);
    return s;
}
// the upstream of light k's value of sample i: grad_image[k][i / spp] / spp + grad_value[k][i] (NULL: zero)
__device__ __forceinline__ float spot_value_seed(const hf_spot_args &a, uint32_t k, size_t i) {
    return (a.gimg ? a.gimg[(size_t) k * (a.n / a.spp) + i / a.spp] * (1.0f / (float) a.spp) : 0.f) +
           (a.gvalue ? a.gvalue[(size_t) k * a.n + i] : 0.f);
}
// Reverse mode of ONE light's value = w ci f G of one sample, for the upstream g:
//   gn = dL/dsh_n,  h = dL/dq (q = p - c, through ref = A^-1 q),  gu = dL/du (through S and |u|),  gw = dL/dweight,
//   gi = dL/dintensity, gcut, gbeam = dL/dcutoff, dL/dbeam (per radian)
struct hf_spot_grads { double gn[3], h[3], gu[3], gw, gi, gcut, gbeam; };
template <class LP>
__device__ __forceinline__ hf_spot_grads spot_light_grads(LP L, double albedo_pi, const hf_spot_shade &s, v3 sn, double g, double w) {
    hf_spot_grads o;
    const double fG = s.m.f * s.G;
    o.gw = g * L->ci * fG;
    o.gi = g * w * albedo_pi * fG;
    const double gf = (g * w * L->ci) * s.G, gG = (g * w * L->ci) * s.m.f; // dL/df, dL/dG
    double gx = 0.0, gy = 0.0, gz = 0.0;
    o.gcut = 0.0; o.gbeam = 0.0;
    if (!s.m.full) { // the zone: f = (cutoff - theta) / (cutoff - beam), theta = atan2(rho, ref.z)
        const double t = gf * L->inv_width;
        o.gcut = t * (1.0 - s.m.f); o.gbeam = t * s.m.f;
        const double rho = sqrt(fma(s.m.x, s.m.x, s.m.y * s.m.y)), ir2 = 1.0 / s.m.r2;
        const double grho = -t * s.m.z * ir2; // dL/dtheta = -t; d theta = (z d rho - rho dz) / |ref|^2
        gz = t * rho * ir2;
        gx = grho * (s.m.x / rho); gy = grho * (s.m.y / rho);
    }
    const double gS = gG * s.ir3, gr = -3.0 * gG * s.G * s.ir2; // dL/dS; dL/du through |u|: gr u
    const double n3[3] = { (double) sn.x, (double) sn.y, (double) sn.z }, u3[3] = { s.u.x, s.u.y, s.u.z };
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o.h[c] = L->Ai[c] * gx + L->Ai[3 + c] * gy + L->Ai[6 + c] * gz; // to_world^-T dL/dref
        o.gn[c] = gS * u3[c];
        o.gu[c] = gS * n3[c] + gr * u3[c];
    }
    return o;
}

// Reverse mode of hf_spot_kernel with respect to sh_n, p, weight and, per light, to_world, intensity and both angles:
// nothing is traced, the visibility byte is read.  First every sample's own gradients: one lane per sample, the lights
// of its byte summed in light order in double and rounded once, overwritten, no atomics.  Then, where grad_lights is
// wanted, light by light (wave-uniform): the 15 numbers of the light kept per lane in double across the grid-stride loop
// over the samples whose bit is set, and reduced as the sensor's 13 (K x 15 live doubles would not fit a lane)
#define HF_SPOT_SUMS 15
__global__ __launch_bounds__(HF_BLOCK) void hf_spot_adjoint_kernel(hf_spot_args a) {
    hf_spot_kargs ka = (hf_spot_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    if (a.gn[0] || a.gp[0] || a.gw) { // (launch-uniform)
        for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += (size_t) gridDim.x * HF_BLOCK) {
            const uint32_t bits = a.vis[i];
            double gn[3] = { 0.0, 0.0, 0.0 }, gp[3] = { 0.0, 0.0, 0.0 }, gw = 0.0;
            if (bits) {
                const v3 sn = mk3(a.sh_n[0][i], a.sh_n[1][i], a.sh_n[2][i]), p = mk3(a.p[0][i], a.p[1][i], a.p[2][i]);
                const double w = a.weight ? (double) a.weight[i] : 1.0;
#pragma unroll 1
                for (uint32_t k = 0; k < a.n_lights; ++k) {
                    if (!((bits >> k) & 1u)) continue;
                    const hf_spot_shade s = spot_shade(&ka->L[k], &ka->atan_c[0], p, sn);
                    if (!s.ok) continue;
                    const hf_spot_grads o = spot_light_grads(&ka->L[k], a.albedo_pi, s, sn, (double) spot_value_seed(a, k, i), w);
                    gw += o.gw;
#pragma unroll
                    for (int c = 0; c < 3; ++c) { gn[c] += o.gn[c]; gp[c] += o.h[c] - o.gu[c]; }
                }
            }
            light_store_grads(a, i, mk3((float) gn[0], (float) gn[1], (float) gn[2]), mk3((float) gp[0], (float) gp[1], (float) gp[2]),
                              (float) gw);
        }
    }
    if (!a.slab) return; // (launch-uniform: grad_lights is not wanted)
#pragma unroll 1
    for (uint32_t k = 0; k < a.n_lights; ++k) { // block-uniform
        double M[HF_SPOT_SUMS];
#pragma unroll
        for (int j = 0; j < HF_SPOT_SUMS; ++j) M[j] = 0.0;
        for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += (size_t) gridDim.x * HF_BLOCK) {
            if (!((a.vis[i] >> k) & 1u)) continue;
            const v3 sn = mk3(a.sh_n[0][i], a.sh_n[1][i], a.sh_n[2][i]), p = mk3(a.p[0][i], a.p[1][i], a.p[2][i]);
            const hf_spot_shade s = spot_shade(&ka->L[k], &ka->atan_c[0], p, sn);
            if (!s.ok) continue;
            const hf_spot_grads o = spot_light_grads(&ka->L[k], a.albedo_pi, s, sn, (double) spot_value_seed(a, k, i),
                                                     a.weight ? (double) a.weight[i] : 1.0);
#pragma unroll
            for (int c = 0; c < 3; ++c) { // q = p - c and ref = A^-1 q: d ref = A^-1 (dp - dA ref - dc); u = c - p
                M[4 * c] -= o.h[c] * s.m.x; M[4 * c + 1] -= o.h[c] * s.m.y; M[4 * c + 2] -= o.h[c] * s.m.z;
                M[4 * c + 3] += o.gu[c] - o.h[c];
            }
            M[12] += o.gi; M[13] += o.gcut; M[14] += o.gbeam;
        }
        sensor_block_store<HF_SPOT_SUMS>(M, a.slab + (size_t) k * gridDim.x * HF_SPOT_SUMS);
        __syncthreads(); // (the next light's sums go through the same LDS rows)
    }
}
// block k: g_lights[k][j] += column j of light k's rows; the angles' columns (per radian) times pi / 180: per degree
__global__ __launch_bounds__(HF_BLOCK) void hf_spot_sum_kernel(const double *__restrict__ slab, uint32_t rows, float *__restrict__ g_lights) {
    const double *const sum = sensor_slab_sums<HF_SPOT_SUMS>(slab + (size_t) blockIdx.x * rows * HF_SPOT_SUMS, rows);
    const uint32_t t = threadIdx.x;
    if (t < (uint32_t) HF_SPOT_SUMS)
        g_lights[blockIdx.x * HF_SPOT_SUMS + t] += (float) (t < 13u ? sum[t] : sum[t] * (3.141592653589793 / 180.0));
}
size_t hf_spot_slab_doubles(uint32_t n_lights) { return (size_t) HF_XFORM_GRID_CAP * HF_SPOT_SUMS * n_lights; }

// forward mode, the transpose of the above: the tangent of light k's value of sample i for tangents dn of sh_n, dp of p,
// dw of weight and row k of d_lights (NULL: zero)
template <class LP, class CP>
__device__ __forceinline__ float spot_tangent_value(const hf_spot_args &a, LP L, CP C, uint32_t k, size_t i) {
    if (!((a.vis[i] >> k) & 1u)) return 0.f;
    const v3 sn = mk3(a.sh_n[0][i], a.sh_n[1][i], a.sh_n[2][i]), p = mk3(a.p[0][i], a.p[1][i], a.p[2][i]);
    const hf_spot_shade s = spot_shade(L, C, p, sn);
    if (!s.ok) return 0.f;
    const v3 dn = a.dn[0] ? mk3(a.dn[0][i], a.dn[1][i], a.dn[2][i]) : mk3(0.f, 0.f, 0.f);
    const double dp[3] = { a.dp[0] ? (double) a.dp[0][i] : 0.0, a.dp[1] ? (double) a.dp[1][i] : 0.0, a.dp[2] ? (double) a.dp[2][i] : 0.0 };
    const double n3[3] = { (double) sn.x, (double) sn.y, (double) sn.z }, u3[3] = { s.u.x, s.u.y, s.u.z };
    const float *dl = a.d_lights ? a.d_lights + k * HF_SPOT_SUMS : nullptr;
    double dq[3], dS = sky_dot_f64(dn, s.u), udu = 0.0; // dp - dA ref - dc; d<sh_n, u>; <u, du>
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double dA0 = 0.0, dA1 = 0.0, dA2 = 0.0, dc = 0.0;
        if (dl) { dA0 = (double) dl[4 * c]; dA1 = (double) dl[4 * c + 1]; dA2 = (double) dl[4 * c + 2]; dc = (double) dl[4 * c + 3]; }
        dq[c] = dp[c] - (dA0 * s.m.x + dA1 * s.m.y + dA2 * s.m.z) - dc;
        dS += n3[c] * (dc - dp[c]);
        udu += u3[c] * (dc - dp[c]);
    }
    double df = 0.0;
    if (!s.m.full) {
        const double dx = L->Ai[0] * dq[0] + L->Ai[1] * dq[1] + L->Ai[2] * dq[2];
        const double dy = L->Ai[3] * dq[0] + L->Ai[4] * dq[1] + L->Ai[5] * dq[2];
        const double dz = L->Ai[6] * dq[0] + L->Ai[7] * dq[1] + L->Ai[8] * dq[2];
        const double rho = sqrt(fma(s.m.x, s.m.x, s.m.y * s.m.y));
        const double drho = (s.m.x * dx + s.m.y * dy) / rho;
        const double dth = (s.m.z * drho - rho * dz) / s.m.r2;
        const double dcut = dl ? (double) dl[13] * (3.141592653589793 / 180.0) : 0.0;
        const double dbeam = dl ? (double) dl[14] * (3.141592653589793 / 180.0) : 0.0;
        df = ((dcut - dth) - s.m.f * (dcut - dbeam)) * L->inv_width;
    }
    const double dG = dS * s.ir3 - 3.0 * s.G * udu * s.ir2;
    const double w = a.weight ? (double) a.weight[i] : 1.0;
    const double dwc = (a.dw ? (double) a.dw[i] : 0.0) * L->ci + w * ((dl ? (double) dl[12] : 0.0) * a.albedo_pi);
    return (float) (dwc * (s.m.f * s.G) + (w * L->ci) * (df * s.G + s.m.f * dG));
}
// light_tangent_image with a loop over the lights: PIXEL = false: one lane per sample and the primal's film (spp a power
// of two <= 64, or no image wanted); PIXEL = true: one lane per pixel adds its samples in order -- no atomics either way
template <bool PIXEL>
__global__ __launch_bounds__(HF_BLOCK) void hf_spot_tangent_kernel(hf_spot_args a) {
    hf_spot_kargs ka = (hf_spot_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const uint32_t spp = a.spp;
    const size_t npix = a.n / spp;
    if (PIXEL) {
        if (i >= npix) return;
#pragma unroll 1
        for (uint32_t k = 0; k < a.n_lights; ++k) {
            float c = 0.f;
            for (uint32_t s = 0; s < spp; ++s) {
                const float dv = spot_tangent_value(a, &ka->L[k], &ka->atan_c[0], k, i * spp + s);
                if (a.value) a.value[(size_t) k * a.n + i * spp + s] = dv;
                c += dv;
            }
            a.image[(size_t) k * npix + i] = c * (1.0f / (float) spp);
        }
    } else {
        const bool in = i < a.n;
#pragma unroll 1
        for (uint32_t k = 0; k < a.n_lights; ++k) { // wave-uniform
            const float c = spot_tangent_value(a, &ka->L[k], &ka->atan_c[0], k, in ? i : a.n - 1);
            if (in && a.value) a.value[(size_t) k * a.n + i] = c;
            if (a.image) film_pixel(a.image, in ? c : 0.f, k, npix, i, spp, in, true, spp, 1.0f / (float) spp);
        }
    }
}

// mode 0: forward, 1: adjoint (and, where grad_lights is wanted, the sum of the blocks' rows, one block per light),
// 2: tangent, 3: rays
void hf_launch_spot(int mode, const hf_spot_args &a, hipStream_t stream) {
    if (mode == 1) {
        if (a.n == 0) return;
        const int grid = grid_for(a.n, HF_XFORM_GRID_CAP); // the slab holds HF_XFORM_GRID_CAP rows per light
        hipLaunchKernelGGL(hf_spot_adjoint_kernel, dim3(grid), dim3(HF_BLOCK), 0, stream, a);
        if (a.slab)
            hipLaunchKernelGGL(hf_spot_sum_kernel, dim3(a.n_lights), dim3(HF_BLOCK), 0, stream, a.slab, (uint32_t) grid, a.g_lights);
        return;
    }
    launch_light(mode, a, a.n_lights, stream, hf_spot_kernel, hf_spot_adjoint_kernel, hf_spot_tangent_kernel<false>,
                 hf_spot_tangent_kernel<true>, hf_spot_rays_kernel);
}

// ---------------------------------------------------------------------------------
// Directional lighting (include/hf.h hf_directional_*): diffuse surface under a RIG of 1..HF_MAX_LIGHTS
// `directional` emitters (src/emitters/directional.cpp), distant lights of irradiance E_k from the unit direction l_k.
// One draw per sample and light: the shadow ray si.spawn_ray(l_k) (the sky row's ray for that direction) traced (any hit,
// per lane) and the film, for ALL lights in ONE launch: hf_spot_kernel's skeleton without the cone mapping,
//   value_k = weight albedo / pi E_k <sh_n, l_k>.
// The row's own text is that term, its derivatives (the direction's through l = v / |v|) and the reduction of the 4
// numbers of every light; the masks, the origin, the walk, the film and the launch are the lighting rows' shared
// functions, the reduction the sensor's (sensor_block_store, sensor_slab_sums).
// ---------------------------------------------------------------------------------
typedef const __attribute__((address_space(4))) hf_directional_args *hf_directional_kargs;

#ifndef HF_DIRECTIONAL_WAVES
#define HF_DIRECTIONAL_WAVES 6 // resident waves per SIMD (the siblings')
#endif
__global__ __launch_bounds__(HF_BLOCK, HF_DIRECTIONAL_WAVES) void hf_directional_kernel(hf_directional_args a) {
    const hf_dev_field &f = a.f;
    // hf_sky_kernel's mapping: n < 2^32, the sample index is one register across the walk
    const size_t i64 = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const bool in = i64 < a.n;
    const uint32_t i = (uint32_t) i64;
    const uint32_t ii = in ? i : (uint32_t) (a.n - 1);
    hf_directional_kargs ka = (hf_directional_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    // the sample's record: read once, held across the loop over the lights
    const v3 sn = mk3(ka->sh_n[0][ii], ka->sh_n[1][ii], ka->sh_n[2][ii]);
    bool elig;
    {
        const v3 d = mk3(ka->d[0][ii], ka->d[1][ii], ka->d[2][ii]);
        elig = in && sky_eligible(ka->t[ii], sn, d);
    }
    const v3 p = mk3(ka->p[0][ii], ka->p[1][ii], ka->p[2][ii]);
    const v3 gn = mk3(ka->nrm[0][ii], ka->nrm[1][ii], ka->nrm[2][ii]);
    float wgt = 1.f;
    {
        const float *weight = ka->weight;
        if (weight) wgt = weight[ii];
    }
    uint32_t bits = 0u; // bit k: the sample was traced towards light k and nothing is in the way
#pragma unroll 1
    for (uint32_t k = 0;; ++k) { // wave-uniform loop, the lanes predicated inside
        asm volatile("" : "+s"(ka)); // opaque per light: the kernarg loads stay inside the loop
        const v3 lf = mk3(ka->L[k].lf[0], ka->L[k].lf[1], ka->L[k].lf[2]);
        const bool traced = elig && dot3(sn, lf) > 0.f;
        // light k's value of a sample that turns out visible: finished and rounded before the ray is begun (the
        // projector kernel's discipline), one float held across the walk
        float val = 0.f;
        {
            v3 snd = sn; // (opaque: the conversions to double are otherwise hoisted out of the loop and held across the walk)
            asm volatile("" : "+v"(snd.x), "+v"(snd.y), "+v"(snd.z));
            if (traced) {
                const hf_d3 l = hf_d3{ ka->L[k].l[0], ka->L[k].l[1], ka->L[k].l[2] };
                val = (float) ((double) wgt * ka->L[k].ce * sky_dot_f64(snd, l));
            }
        }
        asm volatile("" : "+v"(val));
        hf_hit best;
        best.hit = false;
        if (__ballot(traced) != 0ull) // wave-uniform: a batch without a sample traced towards this light skips its walk
            light_walk<true>(&ka->f, f, sky_origin(p, gn, sky_offset(p), lf), lf, traced, best);
        // (the output pointers: loaded here, not before the walk)
        hf_directional_kargs ko = (hf_directional_kargs) __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ko));
        const bool seen = traced && !best.hit; // (traced: in range)
        if (!seen) val = 0.f;
        if (seen) bits |= 1u << k;
        float *value = ko->value;
        if (in && value) value[(size_t) k * ko->n + i] = val;
        float *image = ko->image;
        if (image) { // the film of light k: hf_point_lighting's layout, K images of n / spp
            const uint32_t spp = ko->spp, g = spp < 64u ? spp : 64u;
            film_pixel(image, val, k, ko->n / spp, i, spp, in, (spp & (spp - 1u)) == 0u, g, 1.0f / (float) spp, i);
        }
        if (k + 1u >= ko->n_lights) break;
    }
    hf_directional_kargs ko = (hf_directional_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ko));
    uint8_t *vis = ko->vis;
    if (in && vis) vis[i] = (uint8_t) bits;
}

// the shadow ray of every sample towards ONE light (L[0]), materialised: what hf_directional_kernel traces for it, bit
// for bit (an untraced lane: a zero origin and direction, maxt = -1)
__global__ __launch_bounds__(HF_BLOCK) void hf_directional_rays_kernel(hf_directional_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    v3 sn;
    const bool elig = light_sample(a, i, sn);
    const v3 p = mk3(a.p[0][i], a.p[1][i], a.p[2][i]), gn = mk3(a.nrm[0][i], a.nrm[1][i], a.nrm[2][i]);
    const v3 lf = mk3(a.L[0].lf[0], a.L[0].lf[1], a.L[0].lf[2]);
    light_store_spawned(a, i, p, gn, lf, elig && dot3(sn, lf) > 0.f);
}

// the upstream of light k's value of sample i: grad_image[k][i / spp] / spp + grad_value[k][i] (NULL: zero); A: the
// argument of a row with K images and K value rows (this row's, the specular row's)
template <class A>
__device__ __forceinline__ float directional_value_seed(const A &a, uint32_t k, size_t i) {
    return (a.gimg ? a.gimg[(size_t) k * (a.n / a.spp) + i / a.spp] * (1.0f / (float) a.spp) : 0.f) +
           (a.gvalue ? a.gvalue[(size_t) k * a.n + i] : 0.f);
}

// Reverse mode of hf_directional_kernel with respect to sh_n, weight and, per light, to_light and irradiance: nothing is
// traced, the visibility byte is read.  First every sample's own gradients: one lane per sample, the lights of its byte
// summed in light order in double and rounded once, overwritten, no atomics.  Then, where grad_lights is wanted, light by
// light (block-uniform): the 4 numbers of the light kept per lane in double across the grid-stride loop over the samples
// whose bit is set, and reduced as the sensor's 13.  With S = <sh_n, l> and L = |to_light|:
//   d value = c [ dw E S + w dE S + w E (<dsh_n, l> + <sh_n, dl>) ],   dl = (dv - l <l, dv>) / L
#define HF_DIRECTIONAL_SUMS 4
__global__ __launch_bounds__(HF_BLOCK) void hf_directional_adjoint_kernel(hf_directional_args a) {
    hf_directional_kargs ka = (hf_directional_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    if (a.gn[0] || a.gn[1] || a.gn[2] || a.gw) { // (launch-uniform)
        for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += (size_t) gridDim.x * HF_BLOCK) {
            const uint32_t bits = a.vis[i];
            double gn[3] = { 0.0, 0.0, 0.0 }, gw = 0.0;
            if (bits) {
                const v3 sn = mk3(a.sh_n[0][i], a.sh_n[1][i], a.sh_n[2][i]);
                const double w = a.weight ? (double) a.weight[i] : 1.0;
#pragma unroll 1
                for (uint32_t k = 0; k < a.n_lights; ++k) {
                    if (!((bits >> k) & 1u)) continue;
                    const hf_d3 l = hf_d3{ ka->L[k].l[0], ka->L[k].l[1], ka->L[k].l[2] };
                    const double gce = (double) directional_value_seed(a, k, i) * ka->L[k].ce;
                    gw += gce * sky_dot_f64(sn, l);
                    gn[0] += gce * w * l.x; gn[1] += gce * w * l.y; gn[2] += gce * w * l.z;
                }
            }
            light_store_grads(a, i, mk3((float) gn[0], (float) gn[1], (float) gn[2]), (float) gw);
        }
    }
    if (!a.slab) return; // (launch-uniform: grad_lights is not wanted)
#pragma unroll 1
    for (uint32_t k = 0; k < a.n_lights; ++k) { // block-uniform
        double M[HF_DIRECTIONAL_SUMS];
#pragma unroll
        for (int j = 0; j < HF_DIRECTIONAL_SUMS; ++j) M[j] = 0.0;
        const hf_d3 l = hf_d3{ ka->L[k].l[0], ka->L[k].l[1], ka->L[k].l[2] };
        const double ce_l = ka->L[k].ce * ka->L[k].inv_len;
        for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += (size_t) gridDim.x * HF_BLOCK) {
            if (!((a.vis[i] >> k) & 1u)) continue;
            const v3 sn = mk3(a.sh_n[0][i], a.sh_n[1][i], a.sh_n[2][i]);
            const double gw = (double) directional_value_seed(a, k, i) * (a.weight ? (double) a.weight[i] : 1.0);
            const double S = sky_dot_f64(sn, l), gl = gw * ce_l;
            M[0] += gl * ((double) sn.x - l.x * S); // sh_n's part orthogonal to l, over |to_light|
            M[1] += gl * ((double) sn.y - l.y * S);
            M[2] += gl * ((double) sn.z - l.z * S);
            M[3] += gw * a.albedo_pi * S;
        }
        sensor_block_store<HF_DIRECTIONAL_SUMS>(M, a.slab + (size_t) k * gridDim.x * HF_DIRECTIONAL_SUMS);
        __syncthreads(); // (the next light's sums go through the same LDS rows)
    }
}
// block k: g_lights[k][j] += column j of light k's rows
__global__ __launch_bounds__(HF_BLOCK) void hf_directional_sum_kernel(const double *__restrict__ slab, uint32_t rows,
                                                                       float *__restrict__ g_lights) {
    const double *const sum = sensor_slab_sums<HF_DIRECTIONAL_SUMS>(slab + (size_t) blockIdx.x * rows * HF_DIRECTIONAL_SUMS, rows);
    const uint32_t t = threadIdx.x;
    if (t < (uint32_t) HF_DIRECTIONAL_SUMS) g_lights[blockIdx.x * HF_DIRECTIONAL_SUMS + t] += (float) sum[t];
}
size_t hf_directional_slab_doubles(uint32_t n_lights) { return (size_t) HF_XFORM_GRID_CAP * HF_DIRECTIONAL_SUMS * n_lights; }

// forward mode, the transpose of the above: the tangent of light k's value of sample i for tangents dn of sh_n, dw of
// weight and row k of d_lights (NULL: zero)
template <class LP>
__device__ __forceinline__ float directional_tangent_value(const hf_directional_args &a, LP L, uint32_t k, size_t i) {
    if (!((a.vis[i] >> k) & 1u)) return 0.f;
    const v3 sn = mk3(a.sh_n[0][i], a.sh_n[1][i], a.sh_n[2][i]);
    const v3 dn = a.dn[0] ? mk3(a.dn[0][i], a.dn[1][i], a.dn[2][i]) : mk3(0.f, 0.f, 0.f);
    const hf_d3 l = hf_d3{ L->l[0], L->l[1], L->l[2] };
    const double S = sky_dot_f64(sn, l), w = a.weight ? (double) a.weight[i] : 1.0;
    double dS = sky_dot_f64(dn, l), dE = 0.0;
    if (a.d_lights) {
        const float *dl = a.d_lights + k * HF_DIRECTIONAL_SUMS;
        const double dv[3] = { (double) dl[0], (double) dl[1], (double) dl[2] };
        const double ldv = l.x * dv[0] + l.y * dv[1] + l.z * dv[2];
        const hf_d3 dlk = hf_d3{ (dv[0] - l.x * ldv) * L->inv_len, (dv[1] - l.y * ldv) * L->inv_len, (dv[2] - l.z * ldv) * L->inv_len };
        dS += sky_dot_f64(sn, dlk);
        dE = (double) dl[3];
    }
    const double dw = a.dw ? (double) a.dw[i] : 0.0;
    return (float) ((dw * L->ce + w * (dE * a.albedo_pi)) * S + (w * L->ce) * dS);
}
// light_tangent_image with a loop over the lights: PIXEL = false: one lane per sample and the primal's film (spp a power
// of two <= 64, or no image wanted); PIXEL = true: one lane per pixel adds its samples in order -- no atomics either way
template <bool PIXEL>
__global__ __launch_bounds__(HF_BLOCK) void hf_directional_tangent_kernel(hf_directional_args a) {
    hf_directional_kargs ka = (hf_directional_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const uint32_t spp = a.spp;
    const size_t npix = a.n / spp;
    if (PIXEL) {
        if (i >= npix) return;
#pragma unroll 1
        for (uint32_t k = 0; k < a.n_lights; ++k) {
            float c = 0.f;
            for (uint32_t s = 0; s < spp; ++s) {
                const float dv = directional_tangent_value(a, &ka->L[k], k, i * spp + s);
                if (a.value) a.value[(size_t) k * a.n + i * spp + s] = dv;
                c += dv;
            }
            a.image[(size_t) k * npix + i] = c * (1.0f / (float) spp);
        }
    } else {
        const bool in = i < a.n;
#pragma unroll 1
        for (uint32_t k = 0; k < a.n_lights; ++k) { // wave-uniform
            const float c = directional_tangent_value(a, &ka->L[k], k, in ? i : a.n - 1);
            if (in && a.value) a.value[(size_t) k * a.n + i] = c;
            if (a.image) film_pixel(a.image, in ? c : 0.f, k, npix, i, spp, in, true, spp, 1.0f / (float) spp);
        }
    }
}

// mode 0: forward, 1: adjoint (and, where grad_lights is wanted, the sum of the blocks' rows, one block per light),
// 2: tangent, 3: rays
void hf_launch_directional(int mode, const hf_directional_args &a, hipStream_t stream) {
    if (mode == 1) {
        if (a.n == 0) return;
        const int grid = grid_for(a.n, HF_XFORM_GRID_CAP); // the slab holds HF_XFORM_GRID_CAP rows per light
        hipLaunchKernelGGL(hf_directional_adjoint_kernel, dim3(grid), dim3(HF_BLOCK), 0, stream, a);
        if (a.slab)
            hipLaunchKernelGGL(hf_directional_sum_kernel, dim3(a.n_lights), dim3(HF_BLOCK), 0, stream, a.slab, (uint32_t) grid,
                               a.g_lights);
        return;
    }
    launch_light(mode, a, a.n_lights, stream, hf_directional_kernel, hf_directional_adjoint_kernel,
                 hf_directional_tangent_kernel<false>, hf_directional_tangent_kernel<true>, hf_directional_rays_kernel);
}

// ---------------------------------------------------------------------------------
// Specular highlights (include/hf.h hf_specular_*): the reflection lobe of a rough surface
// (roughplastic.cpp:315-350, roughconductor.cpp's eval: F D G / (4 cos theta_i)) under the directional rig, for ALL
// lights in ONE launch: hf_directional_kernel's skeleton without the walk.  Nothing is traced: bit k of the directional
// row's visibility byte is light k's mask.
//   value_k = weight E_k F(<wi, h>) D(c_h, a) G1(c_i, a) G1(c_o, a) / (4 c_i),   h = (wi + l_k) / |wi + l_k|.
// The row's own text is the lobe with its partial derivatives (specular_lobe, one function for the three kernels) and
// the reduction of the 4 numbers of every light; F and G1 are the glossy row's (reflect_vertex, glossy_smith), the film,
// the seed, the stores, the launch and the reduction the lighting rows' and the sensor's shared functions.
// ---------------------------------------------------------------------------------
typedef const __attribute__((address_space(4))) hf_specular_args *hf_specular_kargs;

// The lobe of one sample under one light, per unit weight and irradiance: v = F R with R = D G1(c_i) G1(c_o) / (4 c_i), D
// and the products in double; and (DERIV) its partial derivatives with every mask held:
//   N = dv/dsh_n = v [ kD h + (dlnG1(c_i)/dc - 1/c_i) wi + (dlnG1(c_o)/dc) l ],      kD = dlnD/dc_h,
//   A = dv/da    = v [ dlnD/da + dlnG1(c_i)/da + dlnG1(c_o)/da ],
//   Ld = dv/dl   = v (dlnG1(c_o)/dc) sh_n + [ v kD (sh_n - h c_h) + R dF/du (wi - h u) ] / M   (l free; dh = (dl - h <h, dl>) / M)
// with u = <wi, h>, M = |wi + l|.  A lane whose cosines are not positive: all zero.  Where both are, M > 0, c_h > 0 and
// u > 0 (microfacet.h:206, :362 hold identically and are not tested).  P: where eta, rcp_eta are read (reflect_vertex)
struct hf_specular_lobe {
    double v, N[3], A, Ld[3];
};
// d ln G1 = dG1 / G1 of glossy_smith's float32 results in double; 0 if that is not finite
__device__ __forceinline__ double specular_dln(float dg, float g) {
    const double q = (double) dg / (double) g;
    return __builtin_fabs(q) < (double) __builtin_inff() ? q : 0.0;
}
template <bool DERIV, class P>
__device__ __forceinline__ hf_specular_lobe specular_lobe(P a, v3 sn, v3 d, float al, hf_d3 l) {
    hf_specular_lobe r;
    r.v = 0.0; r.A = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) { r.N[c] = 0.0; r.Ld[c] = 0.0; }
    const hf_d3 wi = hf_d3{ -(double) d.x, -(double) d.y, -(double) d.z };
    const double ci = sky_dot_f64(sn, wi), co = sky_dot_f64(sn, l);
    if (!(ci > 0.0) || !(co > 0.0)) return r;
    const hf_d3 m = hf_d3{ wi.x + l.x, wi.y + l.y, wi.z + l.z };
    const double iM = 1.0 / sqrt(m.x * m.x + m.y * m.y + m.z * m.z);
    const hf_d3 h = hf_d3{ m.x * iM, m.y * iM, m.z * iM };
    const double ch = sky_dot_f64(sn, h);
    // F at the float32 cosine <wi, float32(h)> and G1 at the float32 cosines: the glossy row's functions
    const hf_reflect_vertex rv = reflect_vertex(a, mk3((float) h.x, (float) h.y, (float) h.z), d);
    const hf_glossy_smith gi = glossy_smith(al, (float) ci), go = glossy_smith(al, (float) co);
    // D = 1 / (pi a^2 q^2), q = s^2 / a^2 + c_h^2 (microfacet.h:185-207, isotropic GGX)
    const double ad = (double) al, ia2 = 1.0 / (ad * ad);
    const double s2 = fmax(1.0 - ch * ch, 0.0);
    const double q = s2 * ia2 + ch * ch;
    const double D = ia2 / (3.141592653589793 * (q * q));
    const double R = D * ((double) gi.G * (double) go.G) / (4.0 * ci);
    r.v = (double) rv.F * R;
    if (DERIV) {
        const double kD = -4.0 * ch * (1.0 - (s2 > 0.0 ? ia2 : 0.0)) / q;
        const double kDa = -2.0 / ad + 4.0 * s2 * ia2 / (ad * q);
        // (d ln G1: 0 where the float32 G1 or its derivative left float32's range, a cosine below about 1e-13)
        const double ki = specular_dln(gi.dc, gi.G) - 1.0 / ci, ko = specular_dln(go.dc, go.G);
        const double ka = specular_dln(gi.da, gi.G) + specular_dln(go.da, go.G);
        const double u = wi.x * h.x + wi.y * h.y + wi.z * h.z;
        const double vD = r.v * kD, vi = r.v * ki, vo = r.v * ko, RF = R * (double) rv.dF;
        r.N[0] = vD * h.x + vi * wi.x + vo * l.x;
        r.N[1] = vD * h.y + vi * wi.y + vo * l.y;
        r.N[2] = vD * h.z + vi * wi.z + vo * l.z;
        r.A = r.v * (kDa + ka);
        r.Ld[0] = vo * (double) sn.x + (vD * ((double) sn.x - h.x * ch) + RF * (wi.x - h.x * u)) * iM;
        r.Ld[1] = vo * (double) sn.y + (vD * ((double) sn.y - h.y * ch) + RF * (wi.y - h.y * u)) * iM;
        r.Ld[2] = vo * (double) sn.z + (vD * ((double) sn.z - h.z * ch) + RF * (wi.z - h.z * u)) * iM;
    }
    return r;
}
// a sample takes part when its roughness is finite (a = max(alpha, 1e-4)); its byte otherwise counts as zero
__device__ __forceinline__ bool specular_finite(float alpha) { return __builtin_fabsf(alpha) < __builtin_inff(); }

#ifndef HF_SPECULAR_WAVES
#define HF_SPECULAR_WAVES 6 // resident waves per SIMD (the siblings'; profiles/specular/registers.txt)
#endif
__global__ __launch_bounds__(HF_BLOCK, HF_SPECULAR_WAVES) void hf_specular_kernel(hf_specular_args a) {
    // hf_directional_kernel's mapping: n < 2^32, one lane per sample
    const size_t i64 = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const bool in = i64 < a.n;
    const uint32_t i = (uint32_t) i64;
    const uint32_t ii = in ? i : (uint32_t) (a.n - 1);
    hf_specular_kargs ka = (hf_specular_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    // the sample's record: read once, held across the loop over the lights
    const v3 sn = mk3(ka->sh_n[0][ii], ka->sh_n[1][ii], ka->sh_n[2][ii]);
    const v3 d = mk3(ka->d[0][ii], ka->d[1][ii], ka->d[2][ii]);
    const float alpha = ka->alpha[ii];
    float wgt = 1.f;
    {
        const float *weight = ka->weight;
        if (weight) wgt = weight[ii];
    }
    const uint32_t bits = (in && specular_finite(alpha)) ? (uint32_t) ka->vis[ii] : 0u;
    const float al = fmaxf(alpha, 1e-4f);
#pragma unroll 1
    for (uint32_t k = 0;; ++k) { // wave-uniform loop, the lanes predicated inside
        asm volatile("" : "+s"(ka)); // opaque per light: the kernarg loads stay inside the loop
        const bool lit = ((bits >> k) & 1u) != 0u;
        float val = 0.f;
        if (__ballot(lit) != 0ull) { // wave-uniform: a batch without a sample lit by this light skips its lobe
            if (lit) {
                const hf_d3 l = hf_d3{ ka->L[k].l[0], ka->L[k].l[1], ka->L[k].l[2] };
                val = (float) (((double) wgt * ka->L[k].ce) * specular_lobe<false>(ka, sn, d, al, l).v);
            }
        }
        float *value = ka->value;
        if (in && value) value[(size_t) k * ka->n + i] = val;
        float *image = ka->image;
        if (image) { // the film of light k: hf_point_lighting's layout, K images of n / spp
            const uint32_t spp = ka->spp, g = spp < 64u ? spp : 64u;
            film_pixel(image, val, k, ka->n / spp, i, spp, in, (spp & (spp - 1u)) == 0u, g, 1.0f / (float) spp, i);
        }
        if (k + 1u >= ka->n_lights) break;
    }
}

// Reverse mode of hf_specular_kernel with respect to sh_n, weight, alpha and, per light, to_light and irradiance:
// hf_directional_adjoint_kernel's two grid-stride passes.  First every sample's own gradients: the lights of its byte
// summed in light order in double and rounded once, overwritten, no atomics.  Then, where grad_lights is wanted, light by
// light (block-uniform): the 4 numbers of the light kept per lane in double across the grid-stride loop and reduced as
// the sensor's 13.  dl = (dv - l <l, dv>) / L
#define HF_SPECULAR_SUMS 4
__global__ __launch_bounds__(HF_BLOCK) void hf_specular_adjoint_kernel(hf_specular_args a) {
    hf_specular_kargs ka = (hf_specular_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    if (a.gn[0] || a.gn[1] || a.gn[2] || a.gw || a.ga) { // (launch-uniform)
        for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += (size_t) gridDim.x * HF_BLOCK) {
            const float alpha = a.alpha[i];
            const uint32_t bits = specular_finite(alpha) ? (uint32_t) a.vis[i] : 0u;
            double gn[3] = { 0.0, 0.0, 0.0 }, gw = 0.0, ga = 0.0;
            if (bits) {
                const v3 sn = mk3(a.sh_n[0][i], a.sh_n[1][i], a.sh_n[2][i]), d = mk3(a.d[0][i], a.d[1][i], a.d[2][i]);
                const double w = a.weight ? (double) a.weight[i] : 1.0;
                const float al = fmaxf(alpha, 1e-4f);
#pragma unroll 1
                for (uint32_t k = 0; k < a.n_lights; ++k) {
                    if (!((bits >> k) & 1u)) continue;
                    const hf_d3 l = hf_d3{ ka->L[k].l[0], ka->L[k].l[1], ka->L[k].l[2] };
                    const hf_specular_lobe s = specular_lobe<true>(ka, sn, d, al, l);
                    const double gE = (double) directional_value_seed(a, k, i) * ka->L[k].ce, gwE = gE * w;
                    gw += gE * s.v;
                    gn[0] += gwE * s.N[0]; gn[1] += gwE * s.N[1]; gn[2] += gwE * s.N[2];
                    ga += gwE * s.A;
                }
            }
            light_store_grads(a, i, mk3((float) gn[0], (float) gn[1], (float) gn[2]), (float) gw);
            if (a.ga) a.ga[i] = alpha > 1e-4f ? (float) ga : 0.f; // (the clamp a = 1e-4 is held)
        }
    }
    if (!a.slab) return; // (launch-uniform: grad_lights is not wanted)
#pragma unroll 1
    for (uint32_t k = 0; k < a.n_lights; ++k) { // block-uniform
        double M[HF_SPECULAR_SUMS];
#pragma unroll
        for (int j = 0; j < HF_SPECULAR_SUMS; ++j) M[j] = 0.0;
        const hf_d3 l = hf_d3{ ka->L[k].l[0], ka->L[k].l[1], ka->L[k].l[2] };
        const double E_l = ka->L[k].ce * ka->L[k].inv_len;
        for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += (size_t) gridDim.x * HF_BLOCK) {
            const float alpha = a.alpha[i];
            if (!((a.vis[i] >> k) & 1u) || !specular_finite(alpha)) continue;
            const v3 sn = mk3(a.sh_n[0][i], a.sh_n[1][i], a.sh_n[2][i]), d = mk3(a.d[0][i], a.d[1][i], a.d[2][i]);
            const hf_specular_lobe s = specular_lobe<true>(ka, sn, d, fmaxf(alpha, 1e-4f), l);
            const double gw = (double) directional_value_seed(a, k, i) * (a.weight ? (double) a.weight[i] : 1.0);
            const double lg = l.x * s.Ld[0] + l.y * s.Ld[1] + l.z * s.Ld[2], gl = gw * E_l;
            M[0] += gl * (s.Ld[0] - l.x * lg); // dv/dl's part orthogonal to l, over |to_light|
            M[1] += gl * (s.Ld[1] - l.y * lg);
            M[2] += gl * (s.Ld[2] - l.z * lg);
            M[3] += gw * s.v;
        }
        sensor_block_store<HF_SPECULAR_SUMS>(M, a.slab + (size_t) k * gridDim.x * HF_SPECULAR_SUMS);
        __syncthreads(); // (the next light's sums go through the same LDS rows)
    }
}
// block k: g_lights[k][j] += column j of light k's rows
__global__ __launch_bounds__(HF_BLOCK) void hf_specular_sum_kernel(const double *__restrict__ slab, uint32_t rows,
                                                                    float *__restrict__ g_lights) {
    const double *const sum = sensor_slab_sums<HF_SPECULAR_SUMS>(slab + (size_t) blockIdx.x * rows * HF_SPECULAR_SUMS, rows);
    const uint32_t t = threadIdx.x;
    if (t < (uint32_t) HF_SPECULAR_SUMS) g_lights[blockIdx.x * HF_SPECULAR_SUMS + t] += (float) sum[t];
}
size_t hf_specular_slab_doubles(uint32_t n_lights) { return (size_t) HF_XFORM_GRID_CAP * HF_SPECULAR_SUMS * n_lights; }

// forward mode, the transpose of the above: the tangent of light k's value of sample i for tangents dn of sh_n, dw of
// weight, da of alpha and row k of d_lights (NULL: zero)
template <class LP>
__device__ __forceinline__ float specular_tangent_value(const hf_specular_args &a, LP L, uint32_t k, size_t i) {
    const float alpha = a.alpha[i];
    if (!((a.vis[i] >> k) & 1u) || !specular_finite(alpha)) return 0.f;
    const v3 sn = mk3(a.sh_n[0][i], a.sh_n[1][i], a.sh_n[2][i]), d = mk3(a.d[0][i], a.d[1][i], a.d[2][i]);
    const hf_d3 l = hf_d3{ L->l[0], L->l[1], L->l[2] };
    const hf_specular_lobe s = specular_lobe<true>(&a, sn, d, fmaxf(alpha, 1e-4f), l);
    double dv = 0.0, dE = 0.0;
    if (a.dn[0]) dv = s.N[0] * (double) a.dn[0][i] + s.N[1] * (double) a.dn[1][i] + s.N[2] * (double) a.dn[2][i];
    if (a.da && alpha > 1e-4f) dv += s.A * (double) a.da[i];
    if (a.d_lights) {
        const float *dl = a.d_lights + k * HF_SPECULAR_SUMS;
        const double q[3] = { (double) dl[0], (double) dl[1], (double) dl[2] };
        const double lq = l.x * q[0] + l.y * q[1] + l.z * q[2];
        dv += (s.Ld[0] * (q[0] - l.x * lq) + s.Ld[1] * (q[1] - l.y * lq) + s.Ld[2] * (q[2] - l.z * lq)) * L->inv_len;
        dE = (double) dl[3];
    }
    const double w = a.weight ? (double) a.weight[i] : 1.0, dw = a.dw ? (double) a.dw[i] : 0.0;
    return (float) ((dw * L->ce + w * dE) * s.v + (w * L->ce) * dv);
}
// hf_directional_tangent_kernel's two shapes: PIXEL = false: one lane per sample and the primal's film (spp a power of
// two <= 64, or no image wanted); PIXEL = true: one lane per pixel adds its samples in order -- no atomics either way
template <bool PIXEL>
__global__ __launch_bounds__(HF_BLOCK) void hf_specular_tangent_kernel(hf_specular_args a) {
    hf_specular_kargs ka = (hf_specular_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const uint32_t spp = a.spp;
    const size_t npix = a.n / spp;
    if (PIXEL) {
        if (i >= npix) return;
#pragma unroll 1
        for (uint32_t k = 0; k < a.n_lights; ++k) {
            float c = 0.f;
            for (uint32_t s = 0; s < spp; ++s) {
                const float dv = specular_tangent_value(a, &ka->L[k], k, i * spp + s);
                if (a.value) a.value[(size_t) k * a.n + i * spp + s] = dv;
                c += dv;
            }
            a.image[(size_t) k * npix + i] = c * (1.0f / (float) spp);
        }
    } else {
        const bool in = i < a.n;
#pragma unroll 1
        for (uint32_t k = 0; k < a.n_lights; ++k) { // wave-uniform
            const float c = specular_tangent_value(a, &ka->L[k], k, in ? i : a.n - 1);
            if (in && a.value) a.value[(size_t) k * a.n + i] = c;
            if (a.image) film_pixel(a.image, in ? c : 0.f, k, npix, i, spp, in, true, spp, 1.0f / (float) spp);
        }
    }
}

// mode 0: forward, 1: adjoint (and, where grad_lights is wanted, the sum of the blocks' rows, one block per light),
// 2: tangent; the row has no rays
void hf_launch_specular(int mode, const hf_specular_args &a, hipStream_t stream) {
    if (mode == 1) {
        if (a.n == 0) return;
        const int grid = grid_for(a.n, HF_XFORM_GRID_CAP); // the slab holds HF_XFORM_GRID_CAP rows per light
        hipLaunchKernelGGL(hf_specular_adjoint_kernel, dim3(grid), dim3(HF_BLOCK), 0, stream, a);
        if (a.slab)
            hipLaunchKernelGGL(hf_specular_sum_kernel, dim3(a.n_lights), dim3(HF_BLOCK), 0, stream, a.slab, (uint32_t) grid,
                               a.g_lights);
        return;
    }
    launch_light(mode, a, a.n_lights, stream, hf_specular_kernel, hf_specular_adjoint_kernel,
                 hf_specular_tangent_kernel<false>, hf_specular_tangent_kernel<true>,
                 static_cast<void (*)(hf_specular_args)>(nullptr));
}

// ---------------------------------------------------------------------------------
// Large-steps preconditioning (include/hf.h): A = I + lambda L on the W x H vertex grid, L the combinatorial
// Laplacian of the tessellation (every cell split along v10-v01), and conjugate gradients for A v = u.
//
// Bandwidth-bound 7-point stencil.  An ITEM is 4 consecutive columns of HF_LS_ROWS consecutive rows; consecutive lanes
// own consecutive column groups, so a wave's row accesses are 16 bytes per lane, contiguous (rows of a grid whose W is
// no multiple of 4 are only 4-byte aligned: the same wide instruction, which takes dword alignment).  The rows above
// and below and the two columns beside a lane's own come as further loads of lines its neighbours fetch anyway (L1 /
// L2 hits; no LDS tile).  A group that hangs over the right edge takes the scalar path, rows below the grid are skipped,
// and a vertex's degree comes from index tests.
// Per CG iteration two launches: (a) p = r + beta p_old into the OTHER p buffer (so no block reads a halo value that
// another has replaced), q = A p, the blocks' partials of <p, q>;  (b) x += alpha p, r -= alpha q, the partials of
// <r, r>.  A partial is one double per block, from a shuffle tree and 4 LDS slots; the next launch's prologue has
// every block add them up in one order, so alpha and beta are the same in every block and a solve is bitwise
// repeatable for a fixed grid.  No float atomics.  About 11 passes over the grid per iteration:
// (a) r and p_old 1.5 times each (6 rows for 4) + p + q, (b) x, p, r, q in, x, r out.
// Around the iterations: one start launch (r = u, x = 0, or r = u - A x0 for a warm start) and two end launches (the
// exact solve in the eigenspace of the constant field, and info).  The launch count does not depend on the data: a
// device word per launch parity says that the solve has ended, and the launches that follow return after reading it.
// ---------------------------------------------------------------------------------
#define HF_LS_ROWS 4
typedef float hf_ls_f4 __attribute__((ext_vector_type(4), aligned(4)));

struct hf_ls_args {
    uint32_t W, H, G, k;                 // G: column groups per row; k: the iteration of this launch
    uint32_t nparts, max_iter;           // partials per sum = the grid of every launch of the solve
    uint64_t items;                      // G * ceil(H / HF_LS_ROWS)
    float lambda;
    double tol2;                         // rel_tol^2
    const float *in0, *in1;              // apply: v, -; residual: x0, u; (a): r, p_old
    float *out0, *out1;                  // apply: u, -; residual: r, -;  (a): p, q
    float *x, *r;                        // (b), cold start
    const float *p, *q;                  // (b)
    double *part_pq, *part_rr, *part_uu, *part_su; // nparts doubles each; su: the sum of u
    double *S;                           // { uu, rr[2], rr at convergence }
    uint32_t *flag;                      // { done[2], iterations at convergence }
    float *info;
};

// the sum of a double over the block, the same in every thread (xor butterfly, then the 4 waves' sums in order); every
// thread of the block calls it
__device__ __forceinline__ double ls_block_sum(double v) {
    __shared__ double s_ls[HF_BLOCK / 64];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    if ((threadIdx.x & 63u) == 0u) s_ls[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = s_ls[0];
#pragma unroll
    for (int j = 1; j < HF_BLOCK / 64; ++j) s += s_ls[j];
    __syncthreads(); // (the next call writes the slots again)
    return s;
}
// the sum of n partials in one fixed order, the same in every thread of every block
__device__ __forceinline__ double ls_sum_partials(const double *part, uint32_t n) {
    double s = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += HF_BLOCK) s += part[i];
    return ls_block_sum(s);
}

struct ls_row6 { float v[6]; }; // columns j0 - 1 .. j0 + 4 of a row, 0 outside the grid
__device__ __forceinline__ ls_row6 ls_load_row(const float *__restrict__ a, bool row_in, size_t off, uint32_t j0, uint32_t W) {
    ls_row6 o;
#pragma unroll
    for (int c = 0; c < 6; ++c) o.v[c] = 0.f;
    if (!row_in) return o;
    if (j0 + 4u <= W) {
        const hf_ls_f4 t = *(const hf_ls_f4 *) (a + off);
        o.v[1] = t.x; o.v[2] = t.y; o.v[3] = t.z; o.v[4] = t.w;
    } else {
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c)
            if (j0 + c < W) o.v[1 + c] = a[off + c];
    }
    if (j0 > 0u) o.v[0] = a[off - 1];
    if (j0 + 4u < W) o.v[5] = a[off + 4];
    return o;
}
__device__ __forceinline__ void ls_store4(float *a, size_t off, uint32_t j0, uint32_t W, const float v[4]) {
    if (j0 + 4u <= W) {
        hf_ls_f4 t; t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3];
        *(hf_ls_f4 *) (a + off) = t;
    } else {
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c)
            if (j0 + c < W) a[off + c] = v[c];
    }
}
__device__ __forceinline__ void ls_load4(const float *a, size_t off, uint32_t j0, uint32_t W, float v[4]) {
    if (j0 + 4u <= W) {
        const hf_ls_f4 t = *(const hf_ls_f4 *) (a + off);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) v[c] = (c < 3u && j0 + c < W) ? a[off + c] : 0.f;
    }
}
// (A v) at column c (1..4 of the rows' six) of row i: up / mid / dn are rows i - 1, i, i + 1.  The neighbours in one
// order -- left, right, up, down, (i+1, j-1), (i-1, j+1) --, one rounding per operation; a neighbour outside the grid
// was loaded as 0 and is not counted in the degree
__device__ __forceinline__ float ls_stencil(const ls_row6 &up, const ls_row6 &mid, const ls_row6 &dn, int c, uint32_t i,
                                            uint32_t j, uint32_t W, uint32_t H, float lambda) {
    const bool l = j > 0u, r = j + 1u < W, u = i > 0u, d = i + 1u < H;
    const float deg = (float) ((int) l + (int) r + (int) u + (int) d + (int) (d && l) + (int) (u && r));
    float s = mid.v[c - 1] + mid.v[c + 1];
    s = s + up.v[c];
    s = s + dn.v[c];
    s = s + dn.v[c - 1];
    s = s + up.v[c + 1];
    return mid.v[c] + lambda * (deg * mid.v[c] - s);
}

// the prologue of launch (a) of iteration k: LS_ENDED when the solve has ended (the block returns), LS_ZERO when u = 0
// (iteration 0 only: the answer is 0 exactly, whatever the guess; the block clears its part of x), else LS_GO with beta.
// Block 0 keeps the scalars that later launches read; no launch reads a word that the same launch writes.
enum { LS_ENDED = 0, LS_GO = 1, LS_ZERO = 2 };
__device__ __forceinline__ int ls_begin_iteration(const hf_ls_args &a, float &beta) {
    const uint32_t k = a.k;
    if (k > 0u && a.flag[(k - 1u) & 1u] != 0u) { // one uniform load
        if (blockIdx.x == 0 && threadIdx.x == 0) a.flag[k & 1u] = 1u;
        return LS_ENDED;
    }
    const double rr = ls_sum_partials(a.part_rr, a.nparts);
    const double uu = k == 0u ? ls_sum_partials(a.part_uu, a.nparts) : a.S[0];
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    const bool zero = k == 0u && uu == 0.0;
    // (false for a NaN or an infinite <r, r>: such a solve runs its max_iter launches and reports the NaN)
    if (zero || (rr <= a.tol2 * uu && rr < (double) __builtin_inff())) {
        if (first) { a.flag[k & 1u] = 1u; a.flag[2] = k; a.S[3] = zero ? 0.0 : rr; if (k == 0u) a.S[0] = uu; }
        return zero ? LS_ZERO : LS_ENDED;
    }
    double b = 0.0;
    if (k > 0u) { const double old = a.S[1 + ((k - 1u) & 1u)]; b = old != 0.0 ? rr / old : 0.0; }
    beta = (float) b;
    if (first) { a.S[1 + (k & 1u)] = rr; if (k == 0u) a.S[0] = uu; }
    return LS_GO;
}

enum { LS_APPLY = 0, LS_RESIDUAL = 1, LS_FIRST = 2, LS_ITER = 3 };
// LS_APPLY: out0 = A in0.  LS_RESIDUAL (warm start): out0 = in1 - A in0, partials of <r, r> and <u, u>, the flags
// cleared.  LS_FIRST / LS_ITER: launch (a), p = r (iteration 0: p_old holds nothing) / p = r + beta p_old.
template <int MODE>
__global__ __launch_bounds__(HF_BLOCK) void hf_large_steps_stencil_kernel(hf_ls_args a) {
    float beta = 0.f;
    const uint32_t W = a.W, H = a.H, G = a.G;
    if (MODE >= LS_FIRST) {
        const int go = ls_begin_iteration(a, beta);
        if (go == LS_ENDED) return;
        if (MODE == LS_FIRST && go == LS_ZERO) {
            const float z[4] = { 0.f, 0.f, 0.f, 0.f };
            for (uint64_t it = (uint64_t) blockIdx.x * HF_BLOCK + threadIdx.x; it < a.items; it += (uint64_t) gridDim.x * HF_BLOCK) {
                const uint32_t strip = (uint32_t) (it / G), j0 = 4u * (uint32_t) (it - (uint64_t) strip * G);
                for (uint32_t i = strip * HF_LS_ROWS; i < H && i < (strip + 1u) * HF_LS_ROWS; ++i)
                    ls_store4(a.x, (size_t) i * W + j0, j0, W, z);
            }
            return;
        }
    }
    if (MODE == LS_RESIDUAL && blockIdx.x == 0 && threadIdx.x < 3u) a.flag[threadIdx.x] = 0u;
    const float lambda = a.lambda;
    double acc = 0.0, acc2 = 0.0, acc3 = 0.0;
    const uint64_t stride = (uint64_t) gridDim.x * HF_BLOCK;
    for (uint64_t it = (uint64_t) blockIdx.x * HF_BLOCK + threadIdx.x; it < a.items; it += stride) {
        const uint32_t strip = (uint32_t) (it / G), j0 = 4u * (uint32_t) (it - (uint64_t) strip * G), i0 = strip * HF_LS_ROWS;
        ls_row6 P[HF_LS_ROWS + 2]; // rows i0 - 1 .. i0 + HF_LS_ROWS of what the stencil applies to
#pragma unroll
        for (int rr = 0; rr < HF_LS_ROWS + 2; ++rr) {
            const uint32_t i = i0 + (uint32_t) rr - 1u; // (wraps for the row above row 0: not < H)
            const bool in = i < H;
            const size_t off = (size_t) (in ? i : 0u) * W + j0;
            P[rr] = ls_load_row(a.in0, in, off, j0, W);
            if (MODE == LS_ITER) {
                const ls_row6 o = ls_load_row(a.in1, in, off, j0, W);
#pragma unroll
                for (int c = 0; c < 6; ++c) P[rr].v[c] = P[rr].v[c] + beta * o.v[c];
            }
        }
#pragma unroll
        for (int rr = 0; rr < HF_LS_ROWS; ++rr) {
            const uint32_t i = i0 + (uint32_t) rr;
            if (i >= H) break;
            const size_t off = (size_t) i * W + j0;
            float q[4], p[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                p[c] = P[rr + 1].v[c + 1];
                q[c] = ls_stencil(P[rr], P[rr + 1], P[rr + 2], c + 1, i, j0 + (uint32_t) c, W, H, lambda);
            }
            if (MODE == LS_APPLY) {
                ls_store4(a.out0, off, j0, W, q);
            } else if (MODE == LS_RESIDUAL) {
                float u[4];
                ls_load4(a.in1, off, j0, W, u);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const bool in = j0 + (uint32_t) c < W;
                    q[c] = u[c] - q[c];
                    acc += in ? (double) q[c] * (double) q[c] : 0.0;
                    acc2 += in ? (double) u[c] * (double) u[c] : 0.0;
                    acc3 += in ? (double) u[c] : 0.0;
                }
                ls_store4(a.out0, off, j0, W, q);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) acc += j0 + (uint32_t) c < W ? (double) p[c] * (double) q[c] : 0.0;
                ls_store4(a.out0, off, j0, W, p);
                ls_store4(a.out1, off, j0, W, q);
            }
        }
    }
    if (MODE == LS_APPLY) return;
    const double s = ls_block_sum(acc);
    if (MODE == LS_RESIDUAL) {
        const double s2 = ls_block_sum(acc2), s3 = ls_block_sum(acc3);
        if (threadIdx.x == 0) { a.part_rr[blockIdx.x] = s; a.part_uu[blockIdx.x] = s2; a.part_su[blockIdx.x] = s3; }
    } else if (threadIdx.x == 0) {
        a.part_pq[blockIdx.x] = s;
    }
}

// cold start: r = u, x = 0, the partials of <u, u> (= <r, r>), the flags cleared
__global__ __launch_bounds__(HF_BLOCK) void hf_large_steps_cold_kernel(hf_ls_args a) {
    if (blockIdx.x == 0 && threadIdx.x < 3u) a.flag[threadIdx.x] = 0u;
    const uint32_t W = a.W, H = a.H, G = a.G;
    double acc = 0.0, acc3 = 0.0;
    const uint64_t stride = (uint64_t) gridDim.x * HF_BLOCK;
    for (uint64_t it = (uint64_t) blockIdx.x * HF_BLOCK + threadIdx.x; it < a.items; it += stride) {
        const uint32_t strip = (uint32_t) (it / G), j0 = 4u * (uint32_t) (it - (uint64_t) strip * G), i0 = strip * HF_LS_ROWS;
#pragma unroll
        for (int rr = 0; rr < HF_LS_ROWS; ++rr) {
            const uint32_t i = i0 + (uint32_t) rr;
            if (i >= H) break;
            const size_t off = (size_t) i * W + j0;
            float u[4];
            const float z[4] = { 0.f, 0.f, 0.f, 0.f };
            ls_load4(a.in1, off, j0, W, u);
#pragma unroll
            for (int c = 0; c < 4; ++c) { acc += (double) u[c] * (double) u[c]; acc3 += (double) u[c]; } // (0 beyond the row's end)
            ls_store4(a.r, off, j0, W, u);
            ls_store4(a.x, off, j0, W, z);
        }
    }
    const double s = ls_block_sum(acc), s3 = ls_block_sum(acc3);
    if (threadIdx.x == 0) { a.part_rr[blockIdx.x] = s; a.part_uu[blockIdx.x] = s; a.part_su[blockIdx.x] = s3; }
}

// launch (b) of iteration k: alpha = <r, r> / <p, q>, x += alpha p, r -= alpha q, the partials of the new <r, r>
__global__ __launch_bounds__(HF_BLOCK) void hf_large_steps_update_kernel(hf_ls_args a) {
    const uint32_t k = a.k;
    if (a.flag[k & 1u] != 0u) return; // one uniform load
    const uint32_t W = a.W, H = a.H, G = a.G;
    const double pq = ls_sum_partials(a.part_pq, a.nparts);
    const double rr = a.S[1 + (k & 1u)];
    const float alpha = (float) (pq != 0.0 ? rr / pq : 0.0);
    double acc = 0.0;
    const uint64_t stride = (uint64_t) gridDim.x * HF_BLOCK;
    for (uint64_t it = (uint64_t) blockIdx.x * HF_BLOCK + threadIdx.x; it < a.items; it += stride) {
        const uint32_t strip = (uint32_t) (it / G), j0 = 4u * (uint32_t) (it - (uint64_t) strip * G), i0 = strip * HF_LS_ROWS;
#pragma unroll
        for (int rr_ = 0; rr_ < HF_LS_ROWS; ++rr_) {
            const uint32_t i = i0 + (uint32_t) rr_;
            if (i >= H) break;
            const size_t off = (size_t) i * W + j0;
            float x[4], p[4], r[4], q[4];
            ls_load4(a.x, off, j0, W, x);
            ls_load4(a.p, off, j0, W, p);
            ls_load4(a.r, off, j0, W, r);
            ls_load4(a.q, off, j0, W, q);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                x[c] = x[c] + alpha * p[c];
                r[c] = r[c] - alpha * q[c];
                acc += (double) r[c] * (double) r[c]; // (0 beyond the row's end)
            }
            ls_store4(a.x, off, j0, W, x);
            ls_store4(a.r, off, j0, W, r);
        }
    }
    const double s = ls_block_sum(acc);
    if (threadIdx.x == 0) a.part_rr[blockIdx.x] = s;
}

// After the last iteration.  A 1 = 1 and 1^T A = 1^T: the constant field is an eigenvector of A (eigenvalue 1), and the
// sum of the true residual u - A x is sum(u) - sum(x).  Adding c = (sum(u) - sum(x)) / (W H) to every x is the exact
// solve in that eigenspace: it takes the true residual's mean out (its norm cannot grow) and makes the solve keep the
// sum of its right-hand side, which rounding in the recursion does not.  Launch 1: the partials of sum(x).
__global__ __launch_bounds__(HF_BLOCK) void hf_large_steps_sum_kernel(hf_ls_args a) {
    const uint32_t W = a.W, H = a.H, G = a.G;
    double acc = 0.0;
    for (uint64_t it = (uint64_t) blockIdx.x * HF_BLOCK + threadIdx.x; it < a.items; it += (uint64_t) gridDim.x * HF_BLOCK) {
        const uint32_t strip = (uint32_t) (it / G), j0 = 4u * (uint32_t) (it - (uint64_t) strip * G);
        for (uint32_t i = strip * HF_LS_ROWS; i < H && i < (strip + 1u) * HF_LS_ROWS; ++i) {
            float x[4];
            ls_load4(a.x, (size_t) i * W + j0, j0, W, x);
            acc += ((double) x[0] + (double) x[1]) + ((double) x[2] + (double) x[3]);
        }
    }
    const double s = ls_block_sum(acc);
    if (threadIdx.x == 0) a.part_pq[blockIdx.x] = s;
}
// Launch 2: x += c (not for u = 0: the zeros stay zeros), and info = { iterations performed, |r| / |u| } (the recursive
// residual; 0 for u = 0: the answer is exact)
__global__ __launch_bounds__(HF_BLOCK) void hf_large_steps_finish_kernel(hf_ls_args a) {
    const uint32_t W = a.W, H = a.H, G = a.G;
    const double su = ls_sum_partials(a.part_su, a.nparts), sx = ls_sum_partials(a.part_pq, a.nparts);
    const double uu = a.S[0];
    if (a.info && blockIdx.x == 0) {
        const double last = ls_sum_partials(a.part_rr, a.nparts);
        if (threadIdx.x == 0) {
            const bool done = a.flag[(a.max_iter - 1u) & 1u] != 0u;
            const double rr = done ? a.S[3] : last;
            a.info[0] = (float) (done ? a.flag[2] : a.max_iter);
            a.info[1] = uu != 0.0 ? (float) __builtin_sqrt(rr / uu) : 0.f;
        }
    }
    if (uu == 0.0) return;
    const float c = (float) ((su - sx) / ((double) W * (double) H));
    for (uint64_t it = (uint64_t) blockIdx.x * HF_BLOCK + threadIdx.x; it < a.items; it += (uint64_t) gridDim.x * HF_BLOCK) {
        const uint32_t strip = (uint32_t) (it / G), j0 = 4u * (uint32_t) (it - (uint64_t) strip * G);
        for (uint32_t i = strip * HF_LS_ROWS; i < H && i < (strip + 1u) * HF_LS_ROWS; ++i) {
            const size_t off = (size_t) i * W + j0;
            float x[4];
            ls_load4(a.x, off, j0, W, x);
#pragma unroll
            for (int k = 0; k < 4; ++k) x[k] = x[k] + c;
            ls_store4(a.x, off, j0, W, x);
        }
    }
}

static void ls_shape(hf_ls_args &a, uint32_t W, uint32_t H, double lambda) {
    a.W = W; a.H = H; a.G = (W + 3u) / 4u;
    a.items = (uint64_t) a.G * ((H + HF_LS_ROWS - 1u) / HF_LS_ROWS);
    a.lambda = (float) lambda;
}
// the floats of a solve's workspace (the layout: hf_launch_large_steps_solve)
size_t hf_large_steps_scratch_floats(uint32_t W, uint32_t H) {
    const size_t n4 = ((size_t) W * H + 3u) & ~(size_t) 3u;
    return 4 * n4 + 2 * (4 * (size_t) HF_FLAT_GRID_CAP + 4) + 4;
}

void hf_launch_large_steps_apply(uint32_t W, uint32_t H, double lambda, const float *v, float *u, hipStream_t stream) {
    hf_ls_args a = {};
    ls_shape(a, W, H, lambda);
    a.in0 = v; a.out0 = u;
    hipLaunchKernelGGL(hf_large_steps_stencil_kernel<LS_APPLY>, dim3(grid_for(a.items)), dim3(HF_BLOCK), 0, stream, a);
}

// workspace (include/hf.h): r, q, p[2] of n4 = W H rounded up to 4 floats each, then as doubles the three rows of
// partials and the scalars, then the flag words.  1 + 2 max_iter + 2 launches, the same whatever the data.
void hf_launch_large_steps_solve(uint32_t W, uint32_t H, double lambda, const float *u, float *v, int warm, uint32_t max_iter,
                                 float rel_tol, float *workspace, float *info, hipStream_t stream) {
    hf_ls_args a = {};
    ls_shape(a, W, H, lambda);
    const size_t n4 = ((size_t) W * H + 3u) & ~(size_t) 3u;
    float *r = workspace, *q = r + n4, *p[2] = { q + n4, q + 2 * n4 };
    a.part_pq = (double *) (workspace + 4 * n4);
    a.part_rr = a.part_pq + HF_FLAT_GRID_CAP;
    a.part_uu = a.part_rr + HF_FLAT_GRID_CAP;
    a.part_su = a.part_uu + HF_FLAT_GRID_CAP;
    a.S = a.part_su + HF_FLAT_GRID_CAP;
    a.flag = (uint32_t *) (a.S + 4);
    a.info = info;
    a.max_iter = max_iter;
    a.tol2 = (double) rel_tol * (double) rel_tol;
    a.x = v; a.r = r;
    const dim3 grid(grid_for(a.items)), block(HF_BLOCK);
    a.nparts = grid.x;
    if (warm) {
        a.in0 = v; a.in1 = u; a.out0 = r;
        hipLaunchKernelGGL(hf_large_steps_stencil_kernel<LS_RESIDUAL>, grid, block, 0, stream, a);
    } else {
        a.in1 = u;
        hipLaunchKernelGGL(hf_large_steps_cold_kernel, grid, block, 0, stream, a);
    }
    for (uint32_t k = 0; k < max_iter; ++k) {
        a.k = k;
        a.in0 = r; a.in1 = p[(k + 1u) & 1u]; a.out0 = p[k & 1u]; a.out1 = q;
        if (k == 0) hipLaunchKernelGGL(hf_large_steps_stencil_kernel<LS_FIRST>, grid, block, 0, stream, a);
        else hipLaunchKernelGGL(hf_large_steps_stencil_kernel<LS_ITER>, grid, block, 0, stream, a);
        a.p = p[k & 1u]; a.q = q;
        hipLaunchKernelGGL(hf_large_steps_update_kernel, grid, block, 0, stream, a);
    }
    hipLaunchKernelGGL(hf_large_steps_sum_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(hf_large_steps_finish_kernel, grid, block, 0, stream, a);
}

// ---------------------------------------------------------------------------------
// The normal map (include/hf.h hf_normalmap_*): the reference's `normalmap` (normalmap.cpp:188-196) as a
// map of the shading normal alone.  One lane per sample, the record read once: the three planes of the texture are
// looked up at pos = (u TW, v TH) by the refraction view's bitmap_cell (twelve texel loads, the plane an offset), the
// tangent-space normal m = (2 c - 1) / |2 c - 1| and the base frame s0 = normalize(dp_du - b <b, dp_du>), t0 = b x s0
// are formed in double and N = s0 m_x + t0 m_y + b m_z is rounded once per component.  A lane that is not perturbed
// (inactive, a record that is not finite, no lookup, a degenerate m or frame) passes b through bit for bit.  The
// tangent and the adjoint rebuild the same lane state (normalmap_lane) and differ only in what they do with it; the
// adjoint's texel scatter is hf_bitmap_cell::scatter's products, the lanes of a wave that share a cell added up before
// the atomic (normalmap_scatter): at most twelve float atomics per perturbed sample.
// ---------------------------------------------------------------------------------
#ifndef HF_NORMALMAP_WAVES
#define HF_NORMALMAP_WAVES 8 // resident waves per SIMD of the forward kernel: it streams and walks nothing
#endif
#ifndef HF_NORMALMAP_AD_WAVES
#define HF_NORMALMAP_AD_WAVES 6 // the tangent and the adjoint hold the frame and its derivative in double: 10 VGPRs spilled at 8
#endif
// what the three kernels know of a perturbed lane: the cell, the base normal b and dp_du (u), the frame, m and the
// numbers the derivatives divide by (rA = 1 / |a|, rM = 1 / |2 c - 1|, bu = <b, dp_du>)
struct hf_normalmap_lane {
    hf_bitmap_cell e;
    float bf[3];
    double b[3], u[3], s0[3], t0[3], m[3];
    double bu, rA, rM;
};
__device__ __forceinline__ bool nm_finite(float x) { return __builtin_fabsf(x) <= 3.402823466e38f; }
__device__ __forceinline__ double nm_dot(const double *x, const double *y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }
__device__ __forceinline__ void nm_cross(const double *x, const double *y, double *o) {
    o[0] = x[1] * y[2] - x[2] * y[1];
    o[1] = x[2] * y[0] - x[0] * y[2];
    o[2] = x[0] * y[1] - x[1] * y[0];
}
// the lane's state; false: a pass-through lane (s.bf alone is then defined)
__device__ __forceinline__ bool normalmap_lane(const hf_normalmap_args &a, size_t i, hf_normalmap_lane &s) {
    float uf[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { s.bf[c] = a.sh_n[c][i]; uf[c] = a.dp_du[c][i]; }
    const float u = a.uv[0][i], v = a.uv[1][i];
    if (!(a.active ? a.active[i] != 0 : true)) return false;
    if (!(nm_finite(u) && nm_finite(v) && nm_finite(s.bf[0]) && nm_finite(s.bf[1]) && nm_finite(s.bf[2]) && nm_finite(uf[0]) &&
          nm_finite(uf[1]) && nm_finite(uf[2])))
        return false;
    // one rounding each: no contraction into bitmap_axis' pos - 0.5 can move the cell
    s.e = bitmap_cell(&a, __fmul_rn(u, (float) a.TW), __fmul_rn(v, (float) a.TH));
    if (!s.e.ok) return false;
    const size_t plane = (size_t) a.TW * a.TH;
    double mt[3], av[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        mt[k] = 2.0 * (double) s.e.value(a.tex + (size_t) k * plane) - 1.0;
        s.b[k] = (double) s.bf[k];
        s.u[k] = (double) uf[k];
    }
    s.bu = nm_dot(s.b, s.u);
#pragma unroll
    for (int c = 0; c < 3; ++c) av[c] = s.u[c] - s.b[c] * s.bu;
    const double M2 = nm_dot(mt, mt), A2 = nm_dot(av, av), U2 = nm_dot(s.u, s.u);
    if (!(M2 >= 1e-12) || !(U2 > 0.0) || !(A2 >= 1e-12 * U2)) return false;
    s.rM = 1.0 / sqrt(M2);
    s.rA = 1.0 / sqrt(A2);
#pragma unroll
    for (int c = 0; c < 3; ++c) { s.m[c] = mt[c] * s.rM; s.s0[c] = av[c] * s.rA; }
    nm_cross(s.b, s.s0, s.t0);
    return true;
}

__global__ __launch_bounds__(HF_BLOCK, HF_NORMALMAP_WAVES) void hf_normalmap_kernel(hf_normalmap_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    hf_normalmap_lane s;
    const bool pert = normalmap_lane(a, i, s);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        a.out_n[c][i] = pert ? (float) (s.s0[c] * s.m[0] + s.t0[c] * s.m[1] + s.b[c] * s.m[2]) : s.bf[c];
    if (a.mask) a.mask[i] = pert ? 1 : 0;
}

// dN of the tangents dtex, duv, dsh_n, ddp_du (each NULL: zero) with the cell and the decision held; a pass-through
// lane: dN = dsh_n
__global__ __launch_bounds__(HF_BLOCK, HF_NORMALMAP_AD_WAVES) void hf_normalmap_tangent_kernel(hf_normalmap_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    hf_normalmap_lane s;
    const bool pert = normalmap_lane(a, i, s);
    float dbf[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) dbf[c] = a.dn[c] ? a.dn[c][i] : 0.f;
    if (!pert) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.out_n[c][i] = dbf[c];
        return;
    }
    const size_t plane = (size_t) a.TW * a.TH;
    const double dpx = a.duv[0] ? (double) a.TW * (double) a.duv[0][i] : 0.0;
    const double dpy = a.duv[1] ? (double) a.TH * (double) a.duv[1][i] : 0.0;
    double db[3], du[3], dmt[3], dm[3], da[3], ds0[3], dt0[3], x0[3], x1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double dc = a.dtex ? (double) s.e.value(a.dtex + (size_t) k * plane) : 0.0;
        if (a.duv[0]) {
            float Lx, Ly;
            s.e.slopes(a.tex + (size_t) k * plane, Lx, Ly);
            dc += (double) Lx * dpx + (double) Ly * dpy;
        }
        dmt[k] = 2.0 * dc;
        db[k] = (double) dbf[k];
        du[k] = a.dp[k] ? (double) a.dp[k][i] : 0.0;
    }
    const double mdm = nm_dot(s.m, dmt), dbu = nm_dot(db, s.u) + nm_dot(s.b, du);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        dm[c] = (dmt[c] - s.m[c] * mdm) * s.rM;
        da[c] = du[c] - db[c] * s.bu - s.b[c] * dbu;
    }
    const double sda = nm_dot(s.s0, da);
#pragma unroll
    for (int c = 0; c < 3; ++c) ds0[c] = (da[c] - s.s0[c] * sda) * s.rA;
    nm_cross(db, s.s0, x0);
    nm_cross(s.b, ds0, x1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        dt0[c] = x0[c] + x1[c];
        a.out_n[c][i] = (float) (ds0[c] * s.m[0] + dt0[c] * s.m[1] + db[c] * s.m[2] + s.s0[c] * dm[0] + s.t0[c] * dm[1] +
                                 s.b[c] * dm[2]);
    }
}

// The adjoint's texel scatter: gtex[k][j] += q_k b_j for the three planes, hf_bitmap_cell::scatter's products.  On a
// coherent wavefront neighbouring lanes share a cell (the samples of a pixel, the pixels of a texel), and float atomics
// are the part of the adjoint that dominates (2.7 of 3.0 ms), so the lanes of a RUN -- consecutive perturbed
// lanes of the wave with the same cell -- add their products up in a shuffle tree first and the run's first lane issues
// the twelve atomics.  Lanes that share a cell without standing next to each other stay separate adds: the result is the
// same sum.  HF_NORMALMAP_MERGE = 0 builds the plain form, hf_bitmap_cell::scatter per lane and plane (profiles/normalmap).
#ifndef HF_NORMALMAP_MERGE
#define HF_NORMALMAP_MERGE 1
#endif
// every lane of the wave calls this (a lane past the end or a pass-through lane with pert = false: it adds nothing)
__device__ __forceinline__ void normalmap_scatter(const hf_normalmap_args &a, const hf_bitmap_cell &e, bool pert, const float *q) {
    const size_t plane = (size_t) a.TW * a.TH;
#if HF_NORMALMAP_MERGE
    const unsigned lane = __lane_id();
    // a cell is named by its first and last texel (both below 2^31)
    const unsigned long long key = pert ? ((unsigned long long) e.j[0] | ((unsigned long long) e.j[3] << 32)) : ~0ull;
    const unsigned long long before = __shfl_up(key, 1);
    const bool head = !pert || lane == 0 || before != key;
    const unsigned long long heads = __ballot(head);
    const float gx = 1.f - e.fx, gy = 1.f - e.fy;
    const float w[4] = { gy * gx, gy * e.fx, e.fy * gx, e.fy * e.fx };
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = pert ? q[k] * w[j] : 0.f;
        // after the step d a lane holds the sum of its run over [lane, lane + 2 d)
        for (unsigned d = 1; d < 64u; d <<= 1) {
            const bool join = lane + d < 64u && (((heads >> 1) >> lane) & ((1ull << d) - 1ull)) == 0ull;
            if (__ballot(join) == 0ull) break; // wave-uniform: no run is longer than d
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float o = __shfl_down(v[j], d);
                if (join) v[j] += o;
            }
        }
        if (pert && head) {
#pragma unroll
            for (int j = 0; j < 4; ++j) atomicAdd(a.gtex + (size_t) k * plane + e.j[j], v[j]);
        }
    }
#else
    if (pert) {
#pragma unroll
        for (int k = 0; k < 3; ++k) e.scatter(a.gtex + (size_t) k * plane, q[k]);
    }
#endif
}

// the transpose: grad_uv, grad_sh_n, grad_dp_du overwritten (exact zeros where nothing flows; a pass-through lane hands
// grad_out to grad_sh_n), grad_tex accumulated into with float atomics (normalmap_scatter).  No lane leaves before the
// scatter: a lane past the end reads the last sample and stores nothing
__global__ __launch_bounds__(HF_BLOCK, HF_NORMALMAP_AD_WAVES) void hf_normalmap_adjoint_kernel(hf_normalmap_args a) {
    const size_t i0 = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const bool in = i0 < a.n;
    const size_t i = in ? i0 : a.n - 1;
    hf_normalmap_lane s;
    const bool pert = normalmap_lane(a, i, s) && in;
    float gf[3], q[3] = { 0.f, 0.f, 0.f };
#pragma unroll
    for (int c = 0; c < 3; ++c) gf[c] = a.gout[c][i];
    if (!pert) {
        if (in) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (a.gn[0]) a.gn[c][i] = gf[c];
                if (a.gp[0]) a.gp[c][i] = 0.f;
            }
            if (a.guv[0]) { a.guv[0][i] = 0.f; a.guv[1][i] = 0.f; }
        }
    } else {
        const size_t plane = (size_t) a.TW * a.TH;
        double g[3], gs0[3], gt0[3], gb[3], gm[3], ga[3], x0[3], x1[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            g[c] = (double) gf[c];
            gs0[c] = g[c] * s.m[0]; gt0[c] = g[c] * s.m[1]; gb[c] = g[c] * s.m[2];
        }
        gm[0] = nm_dot(s.s0, g); gm[1] = nm_dot(s.t0, g); gm[2] = nm_dot(s.b, g);
        // t0 = b x s0
        nm_cross(s.s0, gt0, x0);
        nm_cross(gt0, s.b, x1);
#pragma unroll
        for (int c = 0; c < 3; ++c) { gb[c] += x0[c]; gs0[c] += x1[c]; }
        // s0 = a / |a|, a = u - b <b, u>
        const double sg = nm_dot(s.s0, gs0);
#pragma unroll
        for (int c = 0; c < 3; ++c) ga[c] = (gs0[c] - s.s0[c] * sg) * s.rA;
        const double gab = nm_dot(ga, s.b);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (a.gn[0]) a.gn[c][i] = (float) (gb[c] - s.bu * ga[c] - s.u[c] * gab);
            if (a.gp[0]) a.gp[c][i] = (float) (ga[c] - s.b[c] * gab);
        }
        // m = mt / |mt|, mt = 2 c - 1
        const double mg = nm_dot(s.m, gm);
        double gx = 0.0, gy = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double gc = 2.0 * (gm[k] - s.m[k] * mg) * s.rM;
            if (a.guv[0]) {
                float Lx, Ly;
                s.e.slopes(a.tex + (size_t) k * plane, Lx, Ly);
                gx += gc * (double) Lx; gy += gc * (double) Ly;
            }
            q[k] = (float) gc;
        }
        if (a.guv[0]) { a.guv[0][i] = (float) ((double) a.TW * gx); a.guv[1][i] = (float) ((double) a.TH * gy); }
    }
    if (a.gtex) normalmap_scatter(a, s.e, pert, q);
}

// mode 0: forward, 1: adjoint, 2: tangent
void hf_launch_normalmap(int mode, const hf_normalmap_args &a, hipStream_t stream) {
    if (a.n == 0) return;
    const dim3 grid((unsigned) ((a.n + HF_BLOCK - 1) / HF_BLOCK)), block(HF_BLOCK);
    hipLaunchKernelGGL(mode == 0 ? hf_normalmap_kernel : mode == 1 ? hf_normalmap_adjoint_kernel : hf_normalmap_tangent_kernel,
                       grid, block, 0, stream, a);
}

// ---------------------------------------------------------------------------------
// The bump map (include/hf.h hf_bumpmap_*): the reference's `bumpmap` (bumpmap.cpp:199-222 over
// Texture::eval_1_grad, bitmap.cpp:346-423) as a map of the shading normal alone.  One lane per sample, the record read
// once: the ONE plane of the texture is looked up at the normal map's pos = (u TW, v TH) by bitmap_cell, its slopes
// (Lx, Ly) are hf_bitmap_cell::slopes' -- the out_grad of hf_bitmap_eval, bit for bit -- and the rest is in double:
// g = scale (TW Lx, TH Ly), P_u = dp_du + b (g_x - <b, dp_du> / <b, b>), P_v likewise, c = P_u x P_v, N = sigma c / |c| with
// sigma = -1 where <n_geo, c> < 0, rounded once per component.  The division by <b, b> makes the projection exact for the
// b that arrives -- a float32 normal is unit only to rounding, and without it a flat texture leaves b's direction by
// (|b|^2 - 1) tan(angle between b and the tangents' normal).  A lane that is not perturbed (inactive, a record that is
// not finite, no lookup, b = 0, a degenerate dp_du, dp_dv or c) passes b through bit for bit.  The tangent and the adjoint rebuild
// the same lane state (bumpmap_lane); they differentiate the SLOPES, so a texel's weight is -+(1 - f), -+f and uv enters
// through the cross difference C = v11 - v10 - v01 + v00.  The adjoint's scatter (bumpmap_scatter) is four float atomics
// per run of consecutive lanes that share a cell: the run sum is normalmap_scatter's scheme.
// ---------------------------------------------------------------------------------
#ifndef HF_BUMPMAP_WAVES
#define HF_BUMPMAP_WAVES 8 // resident waves per SIMD of the forward kernel: it streams and walks nothing
#endif
#ifndef HF_BUMPMAP_AD_WAVES
#define HF_BUMPMAP_AD_WAVES 5 // the tangent and the adjoint hold both projected tangents and their derivatives in double
#endif
// what the three kernels know of a perturbed lane: the cell, the four texels' cross difference C, the base normal b,
// dp_du (u), dp_dv (v), the gradient g, the projected tangents, ch = c / |c|, rC = 1 / |c|, sigma, k = 1 / <b, b> and
// bu = k <b, dp_du>, bv = k <b, dp_dv>
struct hf_bumpmap_lane {
    hf_bitmap_cell e;
    float bf[3];
    float t[4]; // v00, v10, v01, v11
    double b[3], u[3], v[3], Pu[3], Pv[3], ch[3];
    double g[2], k, bu, bv, rC, sigma;
};
// the lane's state; false: a pass-through lane (s.bf alone is then defined)
__device__ __forceinline__ bool bumpmap_lane(const hf_bumpmap_args &a, size_t i, hf_bumpmap_lane &s) {
    float uf[3], vf[3], nf[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        s.bf[c] = a.sh_n[c][i]; nf[c] = a.n_geo[c][i]; uf[c] = a.dp_du[c][i]; vf[c] = a.dp_dv[c][i];
    }
    const float u = a.uv[0][i], v = a.uv[1][i];
    if (!(a.active ? a.active[i] != 0 : true)) return false;
    bool fin = nm_finite(u) && nm_finite(v);
#pragma unroll
    for (int c = 0; c < 3; ++c) fin = fin && nm_finite(s.bf[c]) && nm_finite(nf[c]) && nm_finite(uf[c]) && nm_finite(vf[c]);
    if (!fin) return false;
    // the normal map's positions: one rounding each
    s.e = bitmap_cell(&a, __fmul_rn(u, (float) a.TW), __fmul_rn(v, (float) a.TH));
    if (!s.e.ok) return false;
    float Lx, Ly;
    s.e.slopes(a.tex, Lx, Ly);
#pragma unroll
    for (int j = 0; j < 4; ++j) s.t[j] = a.tex[s.e.j[j]];
    s.g[0] = (double) a.scale * ((double) a.TW * (double) Lx);
    s.g[1] = (double) a.scale * ((double) a.TH * (double) Ly);
    double ng[3], c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s.b[k] = (double) s.bf[k]; s.u[k] = (double) uf[k]; s.v[k] = (double) vf[k]; ng[k] = (double) nf[k];
    }
    const double B2 = nm_dot(s.b, s.b);
    if (!(B2 > 0.0)) return false;
    s.k = 1.0 / B2;
    s.bu = nm_dot(s.b, s.u) * s.k;
    s.bv = nm_dot(s.b, s.v) * s.k;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s.Pu[k] = s.u[k] + s.b[k] * (s.g[0] - s.bu);
        s.Pv[k] = s.v[k] + s.b[k] * (s.g[1] - s.bv);
    }
    nm_cross(s.Pu, s.Pv, c);
    const double C2 = nm_dot(c, c), U2 = nm_dot(s.u, s.u), V2 = nm_dot(s.v, s.v);
    if (!(U2 > 0.0) || !(V2 > 0.0) || !(C2 >= 1e-12 * U2 * V2)) return false;
    s.rC = 1.0 / sqrt(C2);
    s.sigma = nm_dot(ng, c) < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) s.ch[k] = c[k] * s.rC;
    return true;
}

__global__ __launch_bounds__(HF_BLOCK, HF_BUMPMAP_WAVES) void hf_bumpmap_kernel(hf_bumpmap_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    hf_bumpmap_lane s;
    const bool pert = bumpmap_lane(a, i, s);
#pragma unroll
    for (int c = 0; c < 3; ++c) a.out_n[c][i] = pert ? (float) (s.sigma * s.ch[c]) : s.bf[c];
    if (a.mask) a.mask[i] = pert ? 1 : 0;
}

// dN of the tangents dtex, duv, dsh_n, ddp_du, ddp_dv (each NULL: zero) with the cell, the decision and sigma held; a
// pass-through lane: dN = dsh_n
__global__ __launch_bounds__(HF_BLOCK, HF_BUMPMAP_AD_WAVES) void hf_bumpmap_tangent_kernel(hf_bumpmap_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    hf_bumpmap_lane s;
    const bool pert = bumpmap_lane(a, i, s);
    float dbf[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) dbf[c] = a.dn[c] ? a.dn[c][i] : 0.f;
    if (!pert) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.out_n[c][i] = dbf[c];
        return;
    }
    const double fx = (double) s.e.fx, fy = (double) s.e.fy, gx = (double) (1.f - s.e.fx), gy = (double) (1.f - s.e.fy);
    double dLx = 0.0, dLy = 0.0;
    if (a.dtex) {
        const double d00 = (double) a.dtex[s.e.j[0]], d10 = (double) a.dtex[s.e.j[1]], d01 = (double) a.dtex[s.e.j[2]],
                     d11 = (double) a.dtex[s.e.j[3]];
        dLx = gy * (d10 - d00) + fy * (d11 - d01);
        dLy = gx * (d01 - d00) + fx * (d11 - d10);
    }
    if (a.duv[0]) {
        const double C = ((double) s.t[3] - (double) s.t[1]) - ((double) s.t[2] - (double) s.t[0]);
        dLx += C * ((double) a.TH * (double) a.duv[1][i]);
        dLy += C * ((double) a.TW * (double) a.duv[0][i]);
    }
    const double dg[2] = { (double) a.scale * ((double) a.TW * dLx), (double) a.scale * ((double) a.TH * dLy) };
    double db[3], du[3], dv[3], dPu[3], dPv[3], x0[3], x1[3], dc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        db[k] = (double) dbf[k];
        du[k] = a.dpu[k] ? (double) a.dpu[k][i] : 0.0;
        dv[k] = a.dpv[k] ? (double) a.dpv[k][i] : 0.0;
    }
    // d(k <b, u>) = k (<db, u> + <b, du> - 2 bu <b, db>)
    const double bdb = 2.0 * nm_dot(s.b, db);
    const double dbu = (nm_dot(db, s.u) + nm_dot(s.b, du) - s.bu * bdb) * s.k;
    const double dbv = (nm_dot(db, s.v) + nm_dot(s.b, dv) - s.bv * bdb) * s.k;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        dPu[k] = du[k] + db[k] * (s.g[0] - s.bu) + s.b[k] * (dg[0] - dbu);
        dPv[k] = dv[k] + db[k] * (s.g[1] - s.bv) + s.b[k] * (dg[1] - dbv);
    }
    nm_cross(dPu, s.Pv, x0);
    nm_cross(s.Pu, dPv, x1);
#pragma unroll
    for (int k = 0; k < 3; ++k) dc[k] = x0[k] + x1[k];
    const double cd = nm_dot(s.ch, dc);
#pragma unroll
    for (int k = 0; k < 3; ++k) a.out_n[k][i] = (float) (s.sigma * ((dc[k] - s.ch[k] * cd) * s.rC));
}

// The adjoint's texel scatter: gtex[j] += qx wx_j + qy wy_j with the SLOPES' weights wx = (-(1 - fy), 1 - fy, -fy, fy),
// wy = (-(1 - fx), -fx, 1 - fx, fx) and q = (dL/dLx, dL/dLy).  The lanes of a run -- consecutive perturbed lanes of the
// wave with the same cell -- add their four products up first (normalmap_scatter's scheme, written again here: taking the
// run sum out into a helper both maps call changed the instructions of hf_normalmap_adjoint_kernel) and the
// run's first lane issues the four atomics.  HF_BUMPMAP_MERGE = 0 builds the plain form: four atomics per perturbed lane
// (profiles/bumpmap).
#ifndef HF_BUMPMAP_MERGE
#define HF_BUMPMAP_MERGE 1
#endif
// every lane of the wave calls this (a lane past the end or a pass-through lane with pert = false: it adds nothing)
__device__ __forceinline__ void bumpmap_scatter(const hf_bumpmap_args &a, const hf_bitmap_cell &e, bool pert, float qx, float qy) {
    const float gx = 1.f - e.fx, gy = 1.f - e.fy;
    float v[4] = { -(qx * gy) - qy * gx, qx * gy - qy * e.fx, qy * gx - qx * e.fy, qx * e.fy + qy * e.fx };
#if HF_BUMPMAP_MERGE
    const unsigned lane = __lane_id();
    // a cell is named by its first and last texel (both below 2^31)
    const unsigned long long key = pert ? ((unsigned long long) e.j[0] | ((unsigned long long) e.j[3] << 32)) : ~0ull;
    const unsigned long long before = __shfl_up(key, 1);
    const bool head = !pert || lane == 0 || before != key;
    const unsigned long long heads = __ballot(head);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = pert ? v[j] : 0.f;
    // after the step d a lane holds the sum of its run over [lane, lane + 2 d)
    for (unsigned d = 1; d < 64u; d <<= 1) {
        const bool join = lane + d < 64u && (((heads >> 1) >> lane) & ((1ull << d) - 1ull)) == 0ull;
        if (__ballot(join) == 0ull) break; // wave-uniform: no run is longer than d
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float o = __shfl_down(v[j], d);
            if (join) v[j] += o;
        }
    }
    if (pert && head) {
#else
    if (pert) {
#endif
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicAdd(a.gtex + e.j[j], v[j]);
    }
}

// the transpose: grad_uv, grad_sh_n, grad_dp_du, grad_dp_dv overwritten (exact zeros where nothing flows; a pass-through
// lane hands grad_out to grad_sh_n), grad_tex accumulated into with float atomics (bumpmap_scatter).  No lane leaves before
// the scatter: a lane past the end reads the last sample and stores nothing
__global__ __launch_bounds__(HF_BLOCK, HF_BUMPMAP_AD_WAVES) void hf_bumpmap_adjoint_kernel(hf_bumpmap_args a) {
    const size_t i0 = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const bool in = i0 < a.n;
    const size_t i = in ? i0 : a.n - 1;
    hf_bumpmap_lane s;
    const bool pert = bumpmap_lane(a, i, s) && in;
    float gf[3], qx = 0.f, qy = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) gf[c] = a.gout[c][i];
    if (!pert) {
        if (in) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (a.gn[0]) a.gn[c][i] = gf[c];
                if (a.gpu[0]) a.gpu[c][i] = 0.f;
                if (a.gpv[0]) a.gpv[c][i] = 0.f;
            }
            if (a.guv[0]) { a.guv[0][i] = 0.f; a.guv[1][i] = 0.f; }
        }
    } else {
        double g[3], gc[3], gPu[3], gPv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = (double) gf[c];
        // N = sigma c / |c|
        const double cg = nm_dot(s.ch, g);
#pragma unroll
        for (int c = 0; c < 3; ++c) gc[c] = s.sigma * ((g[c] - s.ch[c] * cg) * s.rC);
        // c = P_u x P_v
        nm_cross(s.Pv, gc, gPu);
        nm_cross(gc, s.Pu, gPv);
        // P_u = u + b (g_x - k <b, u>), P_v = v + b (g_y - k <b, v>), k = 1 / <b, b>
        const double su = nm_dot(gPu, s.b), sv = nm_dot(gPv, s.b), ku = s.k * su, kv = s.k * sv;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (a.gn[0])
                a.gn[c][i] = (float) (gPu[c] * (s.g[0] - s.bu) - s.u[c] * ku + gPv[c] * (s.g[1] - s.bv) - s.v[c] * kv +
                                      2.0 * s.b[c] * (s.bu * ku + s.bv * kv));
            if (a.gpu[0]) a.gpu[c][i] = (float) (gPu[c] - s.b[c] * ku);
            if (a.gpv[0]) a.gpv[c][i] = (float) (gPv[c] - s.b[c] * kv);
        }
        // g = scale (TW Lx, TH Ly)
        const double gLx = (double) a.scale * ((double) a.TW * su), gLy = (double) a.scale * ((double) a.TH * sv);
        if (a.guv[0]) {
            const double C = ((double) s.t[3] - (double) s.t[1]) - ((double) s.t[2] - (double) s.t[0]);
            a.guv[0][i] = (float) ((double) a.TW * (C * gLy));
            a.guv[1][i] = (float) ((double) a.TH * (C * gLx));
        }
        qx = (float) gLx; qy = (float) gLy;
    }
    if (a.gtex) bumpmap_scatter(a, s.e, pert, qx, qy);
}

// mode 0: forward, 1: adjoint, 2: tangent
void hf_launch_bumpmap(int mode, const hf_bumpmap_args &a, hipStream_t stream) {
    if (a.n == 0) return;
    const dim3 grid((unsigned) ((a.n + HF_BLOCK - 1) / HF_BLOCK)), block(HF_BLOCK);
    hipLaunchKernelGGL(mode == 0 ? hf_bumpmap_kernel : mode == 1 ? hf_bumpmap_adjoint_kernel : hf_bumpmap_tangent_kernel,
                       grid, block, 0, stream, a);
}

// ---------------------------------------------------------------------------------
// Homogeneous medium (include/hf.h hf_medium_*): single scattering in the half space below a top plane
// (`homogeneous` + `hg`, src/media/homogeneous.cpp, src/phase/hg.cpp) under the directional rig, which lies outside it.
// One lane per sample; the sample's o, d, t are read once and held across the loop over its K = num_steps points, the
// wave-uniform loop over the lights inside it: point k is drawn on the segment of the primary ray inside the medium in
// proportion to the transmittance, its shadow ray starts IN FREE SPACE (no spawn offset, no normal) and is walked (any
// hit, per lane); a sample that missed the terrain (t = inf) takes part.  The geometry of the segment, the draws and the
// sums are in double; only the ray is float32.  The row's own text is the segment, the draw, the phase function and the
// sums with their derivatives; the sample stream, the walk, the ray store, the film, the launch and the reduction of
// the HF_MEDIUM_PARAMS + n_lights numbers are the lighting rows' and the sensor's shared functions.
// ---------------------------------------------------------------------------------
typedef const __attribute__((address_space(4))) hf_medium_args *hf_medium_kargs;

// the part of a primary ray inside the medium, [u_in, u_in + S]; c = <d, N>; D: the depth of its first point below the
// top; at_t: it ends at t (dS/dt = 1), not at the top plane (dS/dt = 0)
struct hf_medium_seg {
    double u_in, S, D, c;
    bool elig, at_t;
};
template <class P>
__device__ __forceinline__ hf_medium_seg medium_segment(P a, v3 o, v3 d, float tf) {
    hf_medium_seg s;
    const double h = ((double) o.x - a->top_o[0]) * a->N[0] + ((double) o.y - a->top_o[1]) * a->N[1] +
                     ((double) o.z - a->top_o[2]) * a->N[2];
    const double t = (double) tf;
    s.c = (double) d.x * a->N[0] + (double) d.y * a->N[1] + (double) d.z * a->N[2];
    double u_out = 0.0;
    bool some = false;
    s.u_in = 0.0; s.at_t = true;
    if (s.c < 0.0) {
        s.u_in = fmax(0.0, h / -s.c); u_out = t; some = true;
    } else if (h < 0.0) {
        const double top = s.c > 0.0 ? -h / s.c : __builtin_inf();
        s.at_t = t <= top; u_out = s.at_t ? t : top; some = true;
    }
    s.elig = some && tf > 0.f && u_out > s.u_in; // (t > 0: not NaN either)
    s.S = u_out - s.u_in;
    s.D = s.u_in == 0.0 ? -h : 0.0;
    return s;
}
// a = 1 - exp(-sigma_t S), 1 for S = inf
__device__ __forceinline__ double medium_a(double sigma_t, double S) { return -expm1(-sigma_t * S); }
// point k of the sample with stream id `id`: the first number of sky_sample's stream and the optical depth from the
// entry point, tau = -log1p(-xi a) < sigma_t S
__device__ __forceinline__ double medium_tau(uint32_t seed, uint32_t k, uint32_t id, double av, double &xi) {
    float sx, sy;
    sky_sample(seed, k, id, sx, sy);
    xi = (double) sx;
    return -log1p(-xi * av);
}
// the origin of point k's shadow rays: the distance rounded once, then one fma per component
__device__ __forceinline__ v3 medium_point(v3 o, v3 d, double u) {
    const float uf = (float) u;
    return mk3(__builtin_fmaf(uf, d.x, o.x), __builtin_fmaf(uf, d.y, o.y), __builtin_fmaf(uf, d.z, o.z));
}
// hg.cpp:66-69 with wi = -d, wo = l: p = (1 - g^2) / (4 pi temp^(3/2)), temp = 1 + g^2 + 2 g <l, -d>, and dp/dg
struct hf_medium_phase { double p, dg; };
__device__ __forceinline__ hf_medium_phase medium_phase(double g, v3 d, const double l[3]) {
    const double cs = -((double) d.x * l[0] + (double) d.y * l[1] + (double) d.z * l[2]);
    const double temp = 1.0 + g * g + 2.0 * g * cs, rt = sqrt(temp), q = 1.0 / (12.566370614359172 * temp * rt);
    return hf_medium_phase{ (1.0 - g * g) * q, (-2.0 * g * temp - 3.0 * (1.0 - g * g) * (g + cs)) * q / temp };
}

#ifndef HF_MEDIUM_WAVES
#define HF_MEDIUM_WAVES 4 // resident waves per SIMD: the siblings' walk plus the segment's doubles held across it
#endif
__global__ __launch_bounds__(HF_BLOCK, HF_MEDIUM_WAVES) void hf_medium_kernel(hf_medium_args a) {
    // a lane's sums and bits of every light: its own column, no other lane reads it
    __shared__ double s_acc[HF_MAX_LIGHTS][HF_BLOCK];
    __shared__ uint32_t s_bits[HF_MAX_LIGHTS][HF_BLOCK];
    const hf_dev_field &f = a.f;
    // hf_sky_kernel's mapping: n < 2^32, the sample index is one register across the walk
    const size_t i64 = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const bool in = i64 < a.n;
    const uint32_t i = (uint32_t) i64;
    const uint32_t ii = in ? i : (uint32_t) (a.n - 1);
    hf_medium_kargs ka = (hf_medium_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    // the sample's record: read once, held across the loop over the points
    const v3 o = mk3(ka->o[0][ii], ka->o[1][ii], ka->o[2][ii]);
    const v3 d = mk3(ka->d[0][ii], ka->d[1][ii], ka->d[2][ii]);
    const hf_medium_seg s = medium_segment(ka, o, d, ka->t[ii]);
    const bool elig = in && s.elig;
#pragma unroll 1
    for (uint32_t j = 0; j < ka->n_lights; ++j) { s_acc[j][threadIdx.x] = 0.0; s_bits[j][threadIdx.x] = 0u; }
    // wave-uniform: a batch without an eligible sample draws nothing; an eligible sample is traced towards every light
    // that shines in (the host's decision), so no (k, j) of such a batch is without a traced lane
    if (__ballot(elig) != 0ull) {
        uint32_t id;
        {
            const uint32_t *ray_id = ka->ray_id;
            id = ray_id ? ray_id[ii] : ii;
        }
        const double av = medium_a(ka->sigma_t, s.S);
#pragma unroll 1
        for (uint32_t k = 0;; ++k) { // wave-uniform loop, the lanes predicated inside
            asm volatile("" : "+s"(ka)); // opaque per point: the kernarg loads stay inside the loop
            double xi;
            const double tau = medium_tau(ka->seed, k, id, av, xi);
            const v3 ro = medium_point(o, d, s.u_in + tau / ka->sigma_t);
            const double depth = ka->sigma_t * s.D - tau * s.c; // sigma_t x the depth of point k below the top
#pragma unroll 1
            for (uint32_t j = 0;; ++j) { // wave-uniform
                asm volatile("" : "+s"(ka));
                if ((ka->on >> j) & 1u) {
                    const v3 lf = mk3(ka->L[j].lf[0], ka->L[j].lf[1], ka->L[j].lf[2]);
                    hf_hit best;
                    light_walk<true>(&ka->f, f, ro, lf, elig, best);
                    if (elig && !best.hit) {
                        s_bits[j][threadIdx.x] |= 1u << k;
                        s_acc[j][threadIdx.x] += exp(-(depth * ka->inv_nu[j])); // in k order
                    }
                }
                if (j + 1u >= ka->n_lights) break;
            }
            if (k + 1u >= ka->num_steps) break;
        }
    }
    // (the output pointers: loaded here, not before the walk)
    hf_medium_kargs ko = (hf_medium_kargs) __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ko));
    double scale = 0.0; // weight albedo a / K
    if (elig) {
        const float *weight = ko->weight;
        scale = ko->albedo * medium_a(ko->sigma_t, s.S) / (double) ko->num_steps;
        if (weight) scale *= (double) weight[i];
    }
#pragma unroll 1
    for (uint32_t j = 0; j < ko->n_lights; ++j) { // wave-uniform
        const uint32_t bits = s_bits[j][threadIdx.x];
        float val = 0.f;
        if (bits) { // (a bit: eligible, in range)
            const double l[3] = { ko->L[j].l[0], ko->L[j].l[1], ko->L[j].l[2] };
            val = (float) (scale * medium_phase(ko->g, d, l).p * ko->L[j].ce * s_acc[j][threadIdx.x]);
        }
        float *value = ko->value;
        if (in && value) value[(size_t) j * ko->n + i] = val;
        uint32_t *vis_bits = ko->vis_bits;
        if (in && vis_bits) vis_bits[(size_t) j * ko->n + i] = bits;
        float *image = ko->image;
        if (image) { // the film of light j: hf_directional_lighting's layout, J images of n / spp
            const uint32_t spp = ko->spp, g = spp < 64u ? spp : 64u;
            film_pixel(image, val, j, ko->n / spp, i, spp, in, (spp & (spp - 1u)) == 0u, g, 1.0f / (float) spp, i);
        }
    }
}

// shadow ray a.k of every sample towards ONE light (L[0]), materialised: what hf_medium_kernel traces for it, bit for
// bit (an untraced lane: a zero origin and direction, maxt = -1)
__global__ __launch_bounds__(HF_BLOCK) void hf_medium_rays_kernel(hf_medium_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const v3 o = mk3(a.o[0][i], a.o[1][i], a.o[2][i]), d = mk3(a.d[0][i], a.d[1][i], a.d[2][i]);
    const hf_medium_seg s = medium_segment(&a, o, d, a.t[i]);
    const bool traced = s.elig && (a.on & 1u);
    v3 ro = mk3(0.f, 0.f, 0.f), w = ro;
    if (traced) {
        double xi;
        const double tau = medium_tau(a.seed, a.k, light_id(a, i), medium_a(a.sigma_t, s.S), xi);
        ro = medium_point(o, d, s.u_in + tau / a.sigma_t);
        w = mk3(a.L[0].lf[0], a.L[0].lf[1], a.L[0].lf[2]);
    }
    light_store_ray(a, i, ro, w, traced);
}

// What the adjoint and the tangent form of sample i: the segment, a and its two partial derivatives, and per light the
// sums over the points whose bit is set, A0 = sum exp(-x_k) and A1 = sum exp(-x_k) xi_k / (1 - xi_k a) (d tau_k / d a).
// With T = A0 / K and the bits and branches held:
//   value = w albedo a p E T,   dT = -(D dsigma A0 - c da A1) / (K nu),   da = a_S dS + a_sigma dsigma
struct hf_medium_lane {
    hf_medium_seg s;
    double av, a_S, a_sigma;
    double A0[HF_MAX_LIGHTS], A1[HF_MAX_LIGHTS];
    uint32_t any;
};
// J: the lights whose sums are formed are [j0, j0 + J), a compile-time count (the arrays stay in registers)
template <int J>
__device__ __forceinline__ void medium_lane(const hf_medium_args &a, size_t i, v3 d, uint32_t j0, const uint32_t bits[J],
                                            hf_medium_lane &q) {
    q.any = 0u;
#pragma unroll
    for (int j = 0; j < J; ++j) { q.A0[j] = 0.0; q.A1[j] = 0.0; q.any |= bits[j]; }
    if (!q.any) return;
    const double S = q.s.S, eS = exp(-a.sigma_t * S);
    q.av = medium_a(a.sigma_t, S);
    q.a_S = a.sigma_t * eS;
    q.a_sigma = S < __builtin_inf() ? S * eS : 0.0;
    const uint32_t id = light_id(a, i);
#pragma unroll 1
    for (uint32_t k = 0; k < a.num_steps; ++k) {
        if (!((q.any >> k) & 1u)) continue;
        double xi;
        const double tau = medium_tau(a.seed, k, id, q.av, xi);
        const double r = xi / (1.0 - xi * q.av), depth = a.sigma_t * q.s.D - tau * q.s.c;
#pragma unroll
        for (int j = 0; j < J; ++j)
            if ((bits[j] >> k) & 1u) {
                const double e = exp(-(depth * a.inv_nu[j0 + j]));
                q.A0[j] += e; q.A1[j] += e * r;
            }
    }
}
// the upstream of light j's value of sample i: grad_image[j][i / spp] / spp + grad_value[j][i] (NULL: zero), in double
__device__ __forceinline__ double medium_value_seed(const hf_medium_args &a, uint32_t j, size_t i) {
    return (a.gimg ? (double) a.gimg[(size_t) j * (a.n / a.spp) + i / a.spp] / (double) a.spp : 0.0) +
           (a.gvalue ? (double) a.gvalue[(size_t) j * a.n + i] : 0.0);
}

// Reverse mode of hf_medium_kernel with respect to weight, t, sigma_t, albedo, g and every light's irradiance: nothing is
// traced, the points are drawn again and the bits read.  One lane per sample across a grid-stride loop: grad_weight and
// grad_t overwritten, the lights summed in light order in double and rounded once, exact zeros where no bit is set; the
// HF_MEDIUM_SUMS reduced numbers kept per lane in double and reduced as the sensor's 13: no atomics.
#define HF_MEDIUM_SUMS (HF_MEDIUM_PARAMS + HF_MAX_LIGHTS)
__global__ __launch_bounds__(HF_BLOCK) void hf_medium_adjoint_kernel(hf_medium_args a) {
    double M[HF_MEDIUM_SUMS];
#pragma unroll
    for (int j = 0; j < HF_MEDIUM_SUMS; ++j) M[j] = 0.0;
    const double inv_K = 1.0 / (double) a.num_steps;
    for (size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x; i < a.n; i += (size_t) gridDim.x * HF_BLOCK) {
        const v3 o = mk3(a.o[0][i], a.o[1][i], a.o[2][i]), d = mk3(a.d[0][i], a.d[1][i], a.d[2][i]);
        hf_medium_lane q;
        q.s = medium_segment(&a, o, d, a.t[i]);
        double gw = 0.0, ga = 0.0; // dL/dweight; dL/da
        uint32_t bits[HF_MAX_LIGHTS];
#pragma unroll
        for (int j = 0; j < HF_MAX_LIGHTS; ++j)
            bits[j] = (q.s.elig && (uint32_t) j < a.n_lights && ((a.on >> j) & 1u)) ? a.vis_bits[(size_t) j * a.n + i] : 0u;
        medium_lane<HF_MAX_LIGHTS>(a, i, d, 0u, bits, q);
        if (q.any) {
            const double w = a.weight ? (double) a.weight[i] : 1.0;
#pragma unroll
            for (int j = 0; j < HF_MAX_LIGHTS; ++j) {
                if (!bits[j]) continue;
                const hf_medium_phase ph = medium_phase(a.g, d, a.L[j].l);
                const double gj = medium_value_seed(a, j, i), E = a.L[j].ce;
                const double T = q.A0[j] * inv_K, aT = q.av * T, gwa = gj * w * aT;
                gw += gj * a.albedo * ph.p * E * aT;
                ga += gj * w * a.albedo * ph.p * E * (T + q.av * q.s.c * q.A1[j] * a.inv_nu[j] * inv_K);
                M[0] -= gj * w * a.albedo * ph.p * E * q.av * (q.s.D * q.A0[j] * a.inv_nu[j] * inv_K);
                M[1] += gwa * ph.p * E;
                M[2] += gwa * a.albedo * E * ph.dg;
                M[HF_MEDIUM_PARAMS + j] += gwa * a.albedo * ph.p;
            }
            M[0] += ga * q.a_sigma;
        }
        if (a.gw) a.gw[i] = (float) gw;
        if (a.gt) a.gt[i] = (q.any && q.s.at_t) ? (float) (ga * q.a_S) : 0.f;
    }
    if (a.slab) sensor_block_store<HF_MEDIUM_SUMS>(M, a.slab); // (launch-uniform: grad_params is wanted)
}
// one block: g_params[j] += column j of the slab's rows, j < count
__global__ __launch_bounds__(HF_BLOCK) void hf_medium_sum_kernel(const double *__restrict__ slab, uint32_t rows, uint32_t count,
                                                                  float *__restrict__ g_params) {
    const double *const sum = sensor_slab_sums<HF_MEDIUM_SUMS>(slab, rows);
    const uint32_t t = threadIdx.x;
    if (t < count) g_params[t] += (float) sum[t];
}
size_t hf_medium_slab_doubles(void) { return (size_t) HF_XFORM_GRID_CAP * HF_MEDIUM_SUMS; }

// forward mode, the transpose of the above: the tangent of light j's value of sample i for tangents dw of weight, dt of
// t and d_params (NULL: zero)
__device__ __forceinline__ float medium_tangent_value(const hf_medium_args &a, uint32_t j, size_t i) {
    if (!((a.on >> j) & 1u)) return 0.f;
    uint32_t bits[1] = { a.vis_bits[(size_t) j * a.n + i] };
    if (!bits[0]) return 0.f;
    const v3 o = mk3(a.o[0][i], a.o[1][i], a.o[2][i]), d = mk3(a.d[0][i], a.d[1][i], a.d[2][i]);
    hf_medium_lane q;
    q.s = medium_segment(&a, o, d, a.t[i]);
    if (!q.s.elig) return 0.f;
    medium_lane<1>(a, i, d, j, bits, q);
    const double *l = a.L[j].l;
    const hf_medium_phase ph = medium_phase(a.g, d, l);
    const float *dp = a.d_params;
    const double dsigma = dp ? (double) dp[0] : 0.0, dalbedo = dp ? (double) dp[1] : 0.0, dg = dp ? (double) dp[2] : 0.0;
    const double dE = dp ? (double) dp[HF_MEDIUM_PARAMS + j] : 0.0;
    const double w = a.weight ? (double) a.weight[i] : 1.0, dw = a.dw ? (double) a.dw[i] : 0.0;
    const double dS = (a.dt && q.s.at_t) ? (double) a.dt[i] : 0.0;
    const double da = q.a_S * dS + q.a_sigma * dsigma;
    const double inv_K = 1.0 / (double) a.num_steps, E = a.L[j].ce;
    const double T = q.A0[0] * inv_K;
    const double dT = -(q.s.D * dsigma * q.A0[0] - q.s.c * da * q.A1[0]) * a.inv_nu[j] * inv_K;
    const double pE = ph.p * E;
    return (float) ((dw * a.albedo + w * dalbedo) * q.av * pE * T + w * a.albedo * (da * pE * T + q.av * (ph.dg * dg * E + ph.p * dE) * T +
                                                                                    q.av * pE * dT));
}
// light_tangent_image with a loop over the lights (hf_directional_tangent_kernel's shell)
template <bool PIXEL>
__global__ __launch_bounds__(HF_BLOCK) void hf_medium_tangent_kernel(hf_medium_args a) {
    const size_t i = (size_t) blockIdx.x * HF_BLOCK + threadIdx.x;
    const uint32_t spp = a.spp;
    const size_t npix = a.n / spp;
    if (PIXEL) {
        if (i >= npix) return;
#pragma unroll 1
        for (uint32_t j = 0; j < a.n_lights; ++j) {
            float c = 0.f;
            for (uint32_t s = 0; s < spp; ++s) {
                const float dv = medium_tangent_value(a, j, i * spp + s);
                if (a.value) a.value[(size_t) j * a.n + i * spp + s] = dv;
                c += dv;
            }
            a.image[(size_t) j * npix + i] = c * (1.0f / (float) spp);
        }
    } else {
        const bool in = i < a.n;
#pragma unroll 1
        for (uint32_t j = 0; j < a.n_lights; ++j) { // wave-uniform
            const float c = medium_tangent_value(a, j, in ? i : a.n - 1);
            if (in && a.value) a.value[(size_t) j * a.n + i] = c;
            if (a.image) film_pixel(a.image, in ? c : 0.f, j, npix, i, spp, in, true, spp, 1.0f / (float) spp);
        }
    }
}

// mode 0: forward, 1: adjoint (and, where grad_params is wanted, the sum of the blocks' rows, one block), 2: tangent,
// 3: rays
void hf_launch_medium(int mode, const hf_medium_args &a, hipStream_t stream) {
    if (mode == 1) {
        if (a.n == 0) return;
        const int grid = grid_for(a.n, HF_XFORM_GRID_CAP); // the slab holds HF_XFORM_GRID_CAP rows
        hipLaunchKernelGGL(hf_medium_adjoint_kernel, dim3(grid), dim3(HF_BLOCK), 0, stream, a);
        if (a.slab)
            hipLaunchKernelGGL(hf_medium_sum_kernel, dim3(1), dim3(HF_BLOCK), 0, stream, a.slab, (uint32_t) grid,
                               (uint32_t) HF_MEDIUM_PARAMS + a.n_lights, a.g_params);
        return;
    }
    launch_light(mode, a, a.n_lights, stream, hf_medium_kernel, hf_medium_adjoint_kernel, hf_medium_tangent_kernel<false>,
                 hf_medium_tangent_kernel<true>, hf_medium_rays_kernel);
}
