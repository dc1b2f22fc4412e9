// hf_device.h -- device-side arithmetic shared by the gfx950 kernels.
//
// "Spec arithmetic": the per-triangle test, the transforms and the surface
// interaction use an explicit operation order (mul / fma placement written out,
// built with -ffp-contract=off) so that hit decisions are bit-identical to the
// CPU oracle's.  Reference semantics restated (not copied):
//   transform_affine        include/mitsuba/core/transform.h:104-111,130-138
//   moeller_trumbore        include/mitsuba/render/mesh.h:357-380
//   closest-hit tie rule    include/mitsuba/render/kdtree.h:2424-2448
//   surface interaction     src/render/mesh.cpp:672-903
//   finalize                include/mitsuba/render/interaction.h:257-267,476-499
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/hf.h" // HF_RAY_* flag bits

#define HF_MAX_LEVELS 24

struct v3 {
    float x, y, z;
};

__device__ __forceinline__ v3 mk3(float x, float y, float z) { return v3{ x, y, z }; }
__device__ __forceinline__ v3 operator-(v3 a, v3 b) { return v3{ a.x - b.x, a.y - b.y, a.z - b.z }; }
__device__ __forceinline__ v3 operator+(v3 a, v3 b) { return v3{ a.x + b.x, a.y + b.y, a.z + b.z }; }
__device__ __forceinline__ v3 operator*(v3 a, float s) { return v3{ a.x * s, a.y * s, a.z * s }; }
__device__ __forceinline__ v3 neg3(v3 a) { return v3{ -a.x, -a.y, -a.z }; }

// Dr.Jit dot(): x product first, then fmadd of y and z terms
__device__ __forceinline__ float dot3(v3 a, v3 b) {
    return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x));
}
// Dr.Jit cross(): fmsub(a.yzx, b.zxy, a.zxy * b.yzx)
__device__ __forceinline__ v3 cross3(v3 a, v3 b) {
    return v3{ __builtin_fmaf(a.y, b.z, -(a.z * b.y)),
               __builtin_fmaf(a.z, b.x, -(a.x * b.z)),
               __builtin_fmaf(a.x, b.y, -(a.y * b.x)) };
}
__device__ __forceinline__ float rcp_ieee(float x) { return 1.0f / x; }
__device__ __forceinline__ float rsqrt_ieee(float x) { return 1.0f / __builtin_sqrtf(x); }
__device__ __forceinline__ v3 normalize3(v3 v) { return v * rsqrt_ieee(dot3(v, v)); }
// y += a * x, plain mul + add (adjoint accumulation)
__device__ __forceinline__ void axpy3(float a, v3 x, v3 &y) {
    y.x += a * x.x; y.y += a * x.y; y.z += a * x.z;
}
__device__ __forceinline__ v3 fma3(v3 a, float s, v3 c) {
    return v3{ __builtin_fmaf(a.x, s, c.x), __builtin_fmaf(a.y, s, c.y), __builtin_fmaf(a.z, s, c.z) };
}

// row-major 3x4 affine; point: start from the translation column, fmadd columns 0..2
__device__ __forceinline__ v3 xform_point(const float *m, v3 p) {
    v3 r;
    r.x = __builtin_fmaf(m[2], p.z, __builtin_fmaf(m[1], p.y, __builtin_fmaf(m[0], p.x, m[3])));
    r.y = __builtin_fmaf(m[6], p.z, __builtin_fmaf(m[5], p.y, __builtin_fmaf(m[4], p.x, m[7])));
    r.z = __builtin_fmaf(m[10], p.z, __builtin_fmaf(m[9], p.y, __builtin_fmaf(m[8], p.x, m[11])));
    return r;
}
// vector: column 0 * x, then fmadd columns 1, 2
__device__ __forceinline__ v3 xform_vec(const float *m, v3 v) {
    v3 r;
    r.x = __builtin_fmaf(m[2], v.z, __builtin_fmaf(m[1], v.y, m[0] * v.x));
    r.y = __builtin_fmaf(m[6], v.z, __builtin_fmaf(m[5], v.y, m[4] * v.x));
    r.z = __builtin_fmaf(m[10], v.z, __builtin_fmaf(m[9], v.y, m[8] * v.x));
    return r;
}

// Device view of one heightfield: heights + min/max mip pyramid.
//
// Quadtree over 2^top x 2^top cells (top >= 1; cells beyond the grid do not exist).
// A node of level l covers 2^l x 2^l cells.  Levels 1..top are stored COARSE-FIRST in one
// padded array: depth k = top - l holds 2^k x 2^k nodes, row-major with pitch 2^k, at
// offset (4^k - 1)/3 + 1 (entry 0 is padding, the root is entry 1: the global range that bbox and the slab clip
// read; the beam sweep of the traversal kernel reads one depth of it, the level of its hand-off nodes, and parks
// the entries of the nodes along the beam in LDS).  Node (ix,iy) of level l holds
// (min z, max z) over the vertices of its existing cells; nodes without any existing cell hold
// (+inf, -inf) and fail every overlap test.
struct hf_dev_field {
    const float *h;    // W*H heights, row-major
    const float2 *mip; // (4^top - 1)/3 nodes
    const float4 *shear; // sheared bounds of the fine levels, 3 float4 per node (see hf_shear_rec)
    int32_t W, H;
    int32_t top;  // max(ceil(log2(max(W-1,H-1))), 1); mip[1] is the global (min,max)
    float s, sx, sy, iu, iv;
    float hx, hy; // 0.5 (W - 1), 0.5 (H - 1): cells per object unit (host-computed: a kernarg scalar instead of a hoisted -- and spilled -- vector register)
    int32_t flip;
    float to_world[12], to_object[12];
};

// number of existing nodes per row / column at level l
__host__ __device__ __forceinline__ int hf_level_w(int cells, int l) { return (cells + (1 << l) - 1) >> l; }
// offset of pyramid depth k: (4^k - 1)/3 + 1 (entry 0 is padding so that every depth >= 1 starts
// on an even index: the two children of a node that share a row are one aligned 16-byte load)
__host__ __device__ __forceinline__ uint32_t hf_depth_off(int k) { return (0x55555555u & ((1u << (2 * k)) - 1u)) + 1u; }

// Sheared bounds.  Min/max boxes are loose on steep terrain: a node on a slope spans a large
// z range although the surface stays close to a plane.  Nodes of levels 1..HF_SHEAR_TOP therefore
// also carry a plane  z = c + a (x - xc) + b (y - yc)  through their corner heights (x, y in cell
// units, (xc,yc) the node centre) and, per child, the exact range of  z - plane  over the child's
// vertices: the box test of the walk then runs in the sheared coordinate  w = z - plane, in which
// the ray is still a straight line.  Any plane is valid (the ranges are exact for the plane that is
// stored); record = { (a, b, c, f), (lo0, hi0, lo1, hi1), (lo2, hi2, lo3, hi3) }, children in
// actual order j = 2 jy + jx, absent children (+inf, -inf).  The slope factor f = |a|+|b| + 2 max_j(hi_j - lo_j)
// over the existing children (the needle term, see hf_shear_kernel in hf_kernels.hip).  Levels above HF_SHEAR_TOP
// store the zero plane and the children's min/max boxes in the same form.  Same coarse-first indexing as the
// pyramid: node (ix,iy) of level L = depth k = top - L is record  hf_depth_off(k) - 1 + (iy << k) + ix.
#ifndef HF_SHEAR_TOP
#define HF_SHEAR_TOP 5
#endif
__host__ __device__ __forceinline__ size_t hf_shear_records(int top) { // depths 0 .. top-1 (levels 1 .. top)
    return (size_t) hf_depth_off(top) - 1u;
}

struct hf_hit {
    float t, u, v;
    uint32_t prim;
    bool hit;
};

// Moeller-Trumbore with the reference's operation order and inclusive tests.
__device__ __forceinline__ bool moeller_trumbore(v3 o, v3 d, float maxt, v3 p0, v3 p1, v3 p2,
                                                 float &t, float &u, float &v) {
    v3 e1 = p1 - p0, e2 = p2 - p0;
    v3 pvec = cross3(d, e2);
    float inv_det = rcp_ieee(dot3(e1, pvec));
    v3 tvec = o - p0;
    u = dot3(tvec, pvec) * inv_det;
    bool ok = (u >= 0.f) & (u <= 1.f);
    v3 qvec = cross3(tvec, e1);
    v = dot3(d, qvec) * inv_det;
    ok = ok & (v >= 0.f) & (u + v <= 1.f);
    t = dot3(e2, qvec) * inv_det;
    ok = ok & (t >= 0.f) & (t <= maxt);
    return ok;
}

// minimum t; among exactly equal t the higher prim index (the brute-force loop's
// `t <= ray.maxt` lets the later primitive replace the earlier one)
__device__ __forceinline__ void best_update(hf_hit &b, float t, float u, float v, uint32_t prim) {
    if (!b.hit || t < b.t || (t == b.t && prim > b.prim)) {
        b.t = t; b.u = u; b.v = v; b.prim = prim; b.hit = true;
    }
}

// Both triangles of cell (cx,cy):  tri 0 = (v00, v10, v01),  tri 1 = (v11, v01, v10).
__device__ __forceinline__ bool test_cell(const hf_dev_field &f, int cx, int cy, float z00, float z10,
                                          float z01, float z11, v3 o, v3 d, float maxt, hf_hit &b) {
    const float x0 = __builtin_fmaf((float) cx, f.sx, -1.0f), x1 = __builtin_fmaf((float) (cx + 1), f.sx, -1.0f);
    const float y0 = __builtin_fmaf((float) cy, f.sy, -1.0f), y1 = __builtin_fmaf((float) (cy + 1), f.sy, -1.0f);
    const v3 v00 = mk3(x0, y0, z00), v10 = mk3(x1, y0, z10), v01 = mk3(x0, y1, z01), v11 = mk3(x1, y1, z11);
    const uint32_t prim = 2u * ((uint32_t) cy * (uint32_t) (f.W - 1) + (uint32_t) cx);
    float t, u, v;
    bool any = false;
    if (moeller_trumbore(o, d, maxt, v00, v10, v01, t, u, v)) { best_update(b, t, u, v, prim); any = true; }
    if (moeller_trumbore(o, d, maxt, v11, v01, v10, t, u, v)) { best_update(b, t, u, v, prim + 1u); any = true; }
    return any;
}

// (row, col) of the three vertices of a primitive
__device__ __forceinline__ void prim_vertex_ids(const hf_dev_field &f, uint32_t prim, int vi[3], int vj[3]) {
    const uint32_t cell = prim >> 1, cw = (uint32_t) (f.W - 1);
    const int cy = (int) (cell / cw), cx = (int) (cell - (uint32_t) cy * cw);
    if ((prim & 1u) == 0) {
        vi[0] = cy;     vj[0] = cx;
        vi[1] = cy;     vj[1] = cx + 1;
        vi[2] = cy + 1; vj[2] = cx;
    } else {
        vi[0] = cy + 1; vj[0] = cx + 1;
        vi[1] = cy + 1; vj[1] = cx;
        vi[2] = cy;     vj[2] = cx + 1;
    }
}

__device__ __forceinline__ float signf_(float x) { return x >= 0.f ? 1.f : -1.f; }
__device__ __forceinline__ float mulsign(float a, float b) { return b >= 0.f ? a : -a; }

// coordinate_system(), include/mitsuba/core/vector.h:116-136
__device__ __forceinline__ void coordinate_system(v3 n, v3 &s, v3 &t) {
    const float sign = signf_(n.z);
    const float a = -rcp_ieee(sign + n.z);
    const float b = n.x * n.y * a;
    s = mk3(mulsign(n.x * n.x * a, n.z) + 1.f, mulsign(b, n.z), mulsign(-n.x, n.z));
    t = mk3(b, __builtin_fmaf(n.y, n.y * a, sign), -n.y);
}

struct hf_si_rec {
    float t;
    v3 p, n;
    float uv0, uv1;
    v3 sh_n, dp_du, dp_dv;
    float boundary_test;
    v3 sh_s, sh_t, wi;
};

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// Which of the hit triangle's three edges (k = 0: P0-P1, 1: P1-P2, 2: P2-P0) are SILHOUETTE edges for a ray of
// object-space direction od: the neighbour across the edge does not exist (border of the grid) or faces the ray
// the other way.  A grid triangle with slopes (zx, zy) faces the ray by sign(od.z - zx od.x - zy od.y).  Interior
// edges between triangles that face the ray the same way are no visibility boundary.
__device__ __forceinline__ bool tri_faces(float zx, float zy, v3 od) {
    return __builtin_fmaf(-zy, od.y, __builtin_fmaf(-zx, od.x, od.z)) >= 0.f;
}
__device__ __forceinline__ uint32_t silhouette_edges(const hf_dev_field &f, uint32_t prim, v3 od) {
    const uint32_t cw = (uint32_t) (f.W - 1);
    const int cy = (int) ((prim >> 1) / cw), cx = (int) ((prim >> 1) - (uint32_t) cy * cw);
    const float s = f.s, isx = 1.0f / f.sx, isy = 1.0f / f.sy;
    auto hz = [&](int i, int j) { return f.h[(size_t) i * f.W + j] * s; };
    const float z00 = hz(cy, cx), z10 = hz(cy, cx + 1), z01 = hz(cy + 1, cx), z11 = hz(cy + 1, cx + 1);
    const bool f0 = tri_faces((z10 - z00) * isx, (z01 - z00) * isy, od); // tri 0 = (v00, v10, v01)
    const bool f1 = tri_faces((z11 - z01) * isx, (z11 - z10) * isy, od); // tri 1 = (v11, v01, v10)
    uint32_t m = 0;
    if ((prim & 1u) == 0) {
        if (cy == 0 || tri_faces((z10 - z00) * isx, (z10 - hz(cy - 1, cx + 1)) * isy, od) != f0) m |= 1u; // bottom
        if (f1 != f0) m |= 2u;                                                                             // diagonal
        if (cx == 0 || tri_faces((z01 - hz(cy + 1, cx - 1)) * isx, (z01 - z00) * isy, od) != f0) m |= 4u; // left
    } else {
        if (cy + 2 > f.H - 1 || tri_faces((z11 - z01) * isx, (hz(cy + 2, cx) - z01) * isy, od) != f1) m |= 1u; // top
        if (f0 != f1) m |= 2u;
        if (cx + 2 > f.W - 1 || tri_faces((hz(cy, cx + 2) - z10) * isx, (z11 - z10) * isy, od) != f1) m |= 4u; // right
    }
    return m;
}

// boundary test of the height field = the SDF of the hit point in an equilateral reference triangle
// (src/render/mesh.cpp:845-890), restricted to the silhouette edges; 1 (the incentre value) when there is none
__device__ __forceinline__ float boundary_test_flat(v3 p, v3 p0, v3 dp0, v3 dp1, uint32_t edges) {
    if (edges == 0u) return 1.0f;
    const v3 rel = p - p0;
    const float bb1 = dot3(dp0, rel), bb2 = dot3(dp1, rel);
    const float a11 = dot3(dp0, dp0), a12 = dot3(dp0, dp1), a22 = dot3(dp1, dp1);
    const float inv_det = rcp_ieee(a11 * a22 - a12 * a12);
    const float u = __builtin_fmaf(a22, bb1, -(a12 * bb2)) * inv_det;
    const float v = __builtin_fmaf(-a12, bb1, a11 * bb2) * inv_det;
    const float w = 1.f - u - v;
    const float h3 = 0.5f * __builtin_sqrtf(3.f);
    const float tpx[3] = { 0.f, 1.f, 0.5f }, tpy[3] = { 0.f, 0.f, h3 };
    const float qx = tpx[0] * w + tpx[1] * u + tpx[2] * v, qy = tpy[0] * w + tpy[1] * u + tpy[2] * v;
    float dmin = __builtin_inff();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!((edges >> k) & 1u)) continue;
        const int k1 = (k + 1) % 3;
        const float ex = tpx[k1] - tpx[k], ey = tpy[k1] - tpy[k];
        const float vx = qx - tpx[k], vy = qy - tpy[k];
        const float c = clamp01(__builtin_fmaf(vy, ey, vx * ex) / __builtin_fmaf(ey, ey, ex * ex));
        const float px = vx - ex * c, py = vy - ey * c;
        dmin = fminf(dmin, __builtin_fmaf(py, py, px * px));
    }
    float dist = __builtin_sqrtf(dmin);
    dist /= __builtin_sqrtf(3.f) / 6.f;
    return dist;
}

// ---- Hit geometry: the quantities that compute_si_to, its adjoint (hf_adjoint_kernel), its tangent
// (hf_tangent_kernel) and hf_reparam_backward_kernel share, each written once.  Every call site gets exactly the
// operations it had inline (same order, same fmas), so the results are bit for bit those of the inline forms. ----

// dP/dh of a grid vertex: the third column of to_world times max_height (a height moves its vertex along it only)
__device__ __forceinline__ v3 height_axis(const hf_dev_field &f) {
    return mk3(f.to_world[2] * f.s, f.to_world[6] * f.s, f.to_world[10] * f.s);
}

// World-space vertices + texcoords of a primitive.  With dP: also the vertices' tangents dP_k = dh_k height_axis(f)
// for the height tangent dh (nullptr: zero).  No load depends on another: the three heights and the three height
// tangents go out as one batch.
__device__ __forceinline__ void prim_world(const hf_dev_field &f, uint32_t prim, v3 P[3], float U[3], float V[3],
                                           int vi[3], int vj[3], v3 *dP = nullptr, const float *dh = nullptr) {
    prim_vertex_ids(f, prim, vi, vj);
    const v3 ez = height_axis(f); // dP_k/dh_k
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const size_t idx = (size_t) vi[k] * f.W + vj[k];
        const float dz = dh ? dh[idx] : 0.f;
        const v3 q = mk3(__builtin_fmaf((float) vj[k], f.sx, -1.0f), __builtin_fmaf((float) vi[k], f.sy, -1.0f), f.h[idx] * f.s);
        P[k] = xform_point(f.to_world, q);
        U[k] = (float) vj[k] * f.iu;
        V[k] = (float) vi[k] * f.iv;
        if (dP) dP[k] = ez * dz;
    }
}

// p = sum_k b_k P_k
__device__ __forceinline__ v3 bary_point(const v3 P[3], float b0, float b1, float b2) {
    return mk3(__builtin_fmaf(P[0].x, b0, __builtin_fmaf(P[1].x, b1, P[2].x * b2)),
               __builtin_fmaf(P[0].y, b0, __builtin_fmaf(P[1].y, b1, P[2].y * b2)),
               __builtin_fmaf(P[0].z, b0, __builtin_fmaf(P[1].z, b1, P[2].z * b2)));
}

// ---- Shape attributes (hf_eval_attribute): Mesh::barycentric_coordinates (mesh.cpp:645-667) and its two derivatives.
// The weights (w, u, v) of P0, P1, P2 are the least-squares solution of p - P0 = u du + v dv with du = P1 - P0,
// dv = P2 - P0, in the reference's operation order. ----
struct hf_bary {
    v3 rel, du, dv;        // p - P0, P1 - P0, P2 - P0
    float a11, a12, a22, inv_det;
    float w, u, v;
};
__device__ __forceinline__ hf_bary bary_coords(v3 p, const v3 P[3]) {
    hf_bary b;
    b.rel = p - P[0]; b.du = P[1] - P[0]; b.dv = P[2] - P[0];
    const float b1 = dot3(b.du, b.rel), b2 = dot3(b.dv, b.rel);
    b.a11 = dot3(b.du, b.du); b.a12 = dot3(b.du, b.dv); b.a22 = dot3(b.dv, b.dv);
    b.inv_det = rcp_ieee(b.a11 * b.a22 - b.a12 * b.a12);
    b.u = __builtin_fmaf(b.a22, b1, -(b.a12 * b2)) * b.inv_det;  // fmsub(a22, b1, a12 b2)
    b.v = __builtin_fmaf(-b.a12, b1, b.a11 * b2) * b.inv_det;    // fnmadd(a12, b1, a11 b2)
    b.w = 1.f - b.u - b.v;
    return b;
}
// Mesh::interpolate_attribute (mesh.h:409-437): fmadd(v0, w, fmadd(v1, u, v2 v))
__device__ __forceinline__ float bary_interp(const hf_bary &b, float a0, float a1, float a2) {
    return __builtin_fmaf(a0, b.w, __builtin_fmaf(a1, b.u, a2 * b.v));
}
// With M = [[a11, a12], [a12, a22]] and the residual r = rel - u du - v dv (zero for p in the triangle's plane), the
// derivatives of (u, v) are d(u, v) = M^-1 (<du, z> + <ddu, r>, <dv, z> + <ddv, r>), z = drel - u ddu - v ddv.
__device__ __forceinline__ v3 bary_residual(const hf_bary &b) {
    return mk3(b.rel.x - b.u * b.du.x - b.v * b.dv.x, b.rel.y - b.u * b.du.y - b.v * b.dv.y,
               b.rel.z - b.u * b.du.z - b.v * b.dv.z);
}
// JVP: the tangents (du, dv) of (u, v) for the tangents dp of p and dP[k] of the vertices
__device__ __forceinline__ void bary_coords_jvp(const hf_bary &b, v3 dp, const v3 dP[3], float &du_, float &dv_) {
    const v3 r = bary_residual(b);
    const v3 ddu = dP[1] - dP[0], ddv = dP[2] - dP[0];
    const v3 drel = dp - dP[0];
    const v3 z = mk3(drel.x - b.u * ddu.x - b.v * ddv.x, drel.y - b.u * ddu.y - b.v * ddv.y,
                     drel.z - b.u * ddu.z - b.v * ddv.z);
    const float r1 = dot3(b.du, z) + dot3(ddu, r), r2 = dot3(b.dv, z) + dot3(ddv, r);
    du_ = (b.a22 * r1 - b.a12 * r2) * b.inv_det;
    dv_ = (b.a11 * r2 - b.a12 * r1) * b.inv_det;
}
// VJP, its transpose: for the gradients (gu, gv) of (u, v), the gradients of p (gp) and of the vertices (gP[k]).
// With (g1, g2) = M^-1 (gu, gv) and q = g1 du + g2 dv: gp = q, gP1 = g1 r - u q, gP2 = g2 r - v q, gP0 = -(gp + gP1 + gP2)
__device__ __forceinline__ void bary_coords_vjp(const hf_bary &b, float gu, float gv, v3 &gp, v3 gP[3]) {
    const v3 r = bary_residual(b);
    const float g1 = (b.a22 * gu - b.a12 * gv) * b.inv_det, g2 = (b.a11 * gv - b.a12 * gu) * b.inv_det;
    const v3 q = mk3(g1 * b.du.x + g2 * b.dv.x, g1 * b.du.y + g2 * b.dv.y, g1 * b.du.z + g2 * b.dv.z);
    gp = q;
    gP[1] = mk3(g1 * r.x - b.u * q.x, g1 * r.y - b.u * q.y, g1 * r.z - b.u * q.z);
    gP[2] = mk3(g2 * r.x - b.v * q.x, g2 * r.y - b.v * q.y, g2 * r.z - b.v * q.z);
    gP[0] = mk3(-(q.x + gP[1].x + gP[2].x), -(q.y + gP[1].y + gP[2].y), -(q.z + gP[1].z + gP[2].z));
}

// FollowShape: t re-derived from the glued point p, tt = sqrt(|p - o|^2 / |d|^2) (mesh.cpp:748-752)
struct hf_follow {
    v3 po;    // p - o
    float dd; // |d|^2
    float tt;
};
__device__ __forceinline__ hf_follow follow_t(v3 p, v3 o, v3 d) {
    const v3 po = p - o;
    const float tt = __builtin_sqrtf(dot3(po, po) / dot3(d, d));
    return hf_follow{ po, dot3(d, d), tt }; // (|d|^2 is computed once: the second dot3(d, d) is the same value)
}

// texcoord differences of the triangle and the inverse determinant of their 2x2 matrix (dp_du / dp_dv); inv_det is
// only meaningful when det != 0
struct hf_uv_diff {
    float du0, dv0, du1, dv1, det, inv_det;
};
__device__ __forceinline__ hf_uv_diff uv_diff(const float U[3], const float V[3]) {
    const float du0 = U[1] - U[0], dv0 = V[1] - V[0], du1 = U[2] - U[0], dv1 = V[2] - V[0];
    const float det = __builtin_fmaf(du0, dv1, -(dv0 * du1));
    return hf_uv_diff{ du0, dv0, du1, dv1, det, rcp_ieee(det) };
}

// unit normal of edges e1, e2: n = N r with N = cross(e1, e2), r = 1 / |N|
struct hf_unit_normal {
    v3 n;
    float r;
};
__device__ __forceinline__ hf_unit_normal unit_normal(v3 e1, v3 e2) {
    const v3 N = cross3(e1, e2);
    const float r = rsqrt_ieee(dot3(N, N));
    return hf_unit_normal{ N * r, r };
}

// intermediates of the differentiable Moeller-Trumbore (mesh.h:357-380) for vertex p0 and edges e1, e2:
// u = a_u inv, v = a_v inv, t = a_t inv
struct hf_mt {
    v3 pvec, tvec, qvec;
    float inv, a_u, a_v, a_t;
};
__device__ __forceinline__ hf_mt mt_terms(v3 o, v3 d, v3 p0, v3 e1, v3 e2) {
    hf_mt m;
    m.pvec = cross3(d, e2);
    m.inv = rcp_ieee(dot3(e1, m.pvec));
    m.tvec = o - p0;
    m.qvec = cross3(m.tvec, e1);
    m.a_u = dot3(m.tvec, m.pvec); m.a_v = dot3(d, m.qvec); m.a_t = dot3(e2, m.qvec);
    return m;
}

// ---- Derivatives of the normals, written once for every tangent and adjoint kernel and vertex_normal_jvp / _vjp ----

// derivative of normalize at n = N r (r = |N|^-1) applied to x: (x - n <n, x>) r.  The map is symmetric, so the
// tangent (x = dN) and the adjoint (x = dL/dn) are the same formula.
__device__ __forceinline__ v3 dnormalize(v3 n, float r, v3 x) {
    const float pj = dot3(n, x);
    return mk3((x.x - n.x * pj) * r, (x.y - n.y * pj) * r, (x.z - n.z * pj) * r);
}
// Derivatives of coordinate_system(n) = (s, t), the dp_du / dp_dv of a record without HF_RAY_DPDUV (mesh.cpp:762).  The
// sign is that of the forward n.z and is held constant (nothing is differentiated through it); with a = -1/(sign + n.z),
// b = n.x n.y a: s = (sign n.x^2 a + 1, sign b, -sign n.x), t = (b, n.y^2 a + sign, -n.y), da = a^2 dn.z.
// JVP: (ds, dt) for the tangent dn.
__device__ __forceinline__ void coordinate_system_jvp(v3 n, v3 dn, v3 &ds, v3 &dt) {
    const float sign = signf_(n.z);
    const float a = -rcp_ieee(sign + n.z);
    const float da = a * a * dn.z;
    const float db = (dn.x * n.y + n.x * dn.y) * a + n.x * n.y * da;
    ds = mk3(sign * (2.f * n.x * dn.x * a + n.x * n.x * da), sign * db, -sign * dn.x);
    dt = mk3(db, 2.f * n.y * dn.y * a + n.y * n.y * da, -dn.y);
}
// VJP: dL/dn for the gradients gs = dL/ds, gt = dL/dt (the transpose of coordinate_system_jvp)
__device__ __forceinline__ v3 coordinate_system_vjp(v3 n, v3 gs, v3 gt) {
    const float sign = signf_(n.z);
    const float a = -rcp_ieee(sign + n.z);
    const float gb = sign * gs.y + gt.x;
    const float ga = sign * n.x * n.x * gs.x + n.y * n.y * gt.y + n.x * n.y * gb;
    return mk3(2.f * sign * n.x * a * gs.x + n.y * a * gb - sign * gs.z,
               n.x * a * gb + 2.f * n.y * a * gt.y - gt.z,
               a * a * ga);
}
// tangent of the face normal N = cross(e1, e2): dN = cross(de1, e2) + cross(e1, de2)
__device__ __forceinline__ v3 face_normal_jvp(v3 e1, v3 e2, v3 de1, v3 de2) {
    const v3 c1 = cross3(de1, e2), c2 = cross3(e1, de2);
    return mk3(c1.x + c2.x, c1.y + c2.y, c1.z + c2.z);
}
// its transpose for the gradient gN of N, contracted with ez = height_axis: g1 = <ez, dL/de1>, g2 = <ez, dL/de2>
__device__ __forceinline__ void face_normal_vjp(v3 e1, v3 e2, v3 gN, v3 ez, float &g1, float &g2) {
    g1 = dot3(ez, cross3(e2, gN)); g2 = dot3(ez, cross3(gN, e1));
}

// ---- Smooth shading (hf_set_face_normals(hf, 0)): angle-weighted vertex normals, the JIT path of
// Mesh::recompute_vertex_normals (mesh.cpp:350-384), and the interpolated shading normal of mesh.cpp:792-840. ----

// The shading normal is interpolated only when the reference fetches the vertex normals for it (mesh.cpp:813-815)
__device__ __forceinline__ bool smooth_sh(uint32_t flags) { return (flags & (HF_RAY_SHADINGFRAME | HF_RAY_DNSDUV)) != 0u; }

// object-space position q of grid vertex (row i, column j) with height h, and its world-space position [A | t] q: the
// expressions of prim_world
__device__ __forceinline__ v3 grid_local(const hf_dev_field &f, int i, int j, float h) {
    return mk3(__builtin_fmaf((float) j, f.sx, -1.0f), __builtin_fmaf((float) i, f.sy, -1.0f), h * f.s);
}
__device__ __forceinline__ v3 grid_world(const hf_dev_field &f, int i, int j, float h) {
    return xform_point(f.to_world, grid_local(f, i, j, h));
}

// ---- Derivatives with respect to to_world = [A | t] (row-major 3x4).  Everything attached depends on to_world only
// through the world positions P_v = A q_v + t of the vertices it reads, so dL/d(to_world) = sum_v G_v (q_v, 1)^T with
// G_v = dL/dP_v, and the tangent of P_v for a tangent dM of to_world is dM (q_v, 1) = xform_point(dM, q_v). ----

// M[r][c] += g[r] (q, 1)[c]: one vertex's world-space gradient g times its object-space position q
__device__ __forceinline__ void xform_grad_point(float M[12], v3 g, v3 q) {
    const float gr[3] = { g.x, g.y, g.z };
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        M[4 * r + 0] = __builtin_fmaf(gr[r], q.x, M[4 * r + 0]);
        M[4 * r + 1] = __builtin_fmaf(gr[r], q.y, M[4 * r + 1]);
        M[4 * r + 2] = __builtin_fmaf(gr[r], q.z, M[4 * r + 2]);
        M[4 * r + 3] += gr[r];
    }
}
// ... for a gradient g of a difference of two vertices (object-space difference dq): no translation part
__device__ __forceinline__ void xform_grad_vec(float M[12], v3 g, v3 dq) {
    const float gr[3] = { g.x, g.y, g.z };
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        M[4 * r + 0] = __builtin_fmaf(gr[r], dq.x, M[4 * r + 0]);
        M[4 * r + 1] = __builtin_fmaf(gr[r], dq.y, M[4 * r + 1]);
        M[4 * r + 2] = __builtin_fmaf(gr[r], dq.z, M[4 * r + 2]);
    }
}
// the object-space positions of a primitive's three vertices (prim_vertex_ids' rows vi, columns vj)
__device__ __forceinline__ void prim_local(const hf_dev_field &f, const int vi[3], const int vj[3], v3 q[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = grid_local(f, vi[k], vj[k], f.h[(size_t) vi[k] * f.W + vj[k]]);
}

// The 1-ring of grid vertex (i, j).  With the diagonal split of test_cell, the vertex's neighbours in counter-clockwise
// order are  E (i, j+1), N (i+1, j), NW (i+1, j-1), W (i, j-1), S (i-1, j), SE (i-1, j+1)  and its incident triangles
// are exactly (X, R[k], R[k+1 mod 6]) for the consecutive pairs that both exist: tri 0 of cell (j, i) = (X, E, N),
// tri 1 of cell (j-1, i) = (N, NW, X), tri 0 of cell (j-1, i) = (W, X, NW), tri 1 of cell (j-1, i-1) = (X, W, S),
// tri 0 of cell (j, i-1) = (S, SE, X), tri 1 of cell (j, i-1) = (E, X, SE), each rotated so that X comes first (a
// rotation keeps cross(v1 - v0, v2 - v0)).  Up to 6 triangles; border and corner vertices have fewer.  Absent
// neighbours are loaded at the vertex itself (in bounds) and never used.
struct hf_ring {
    v3 X, R[6];
    int i[7], j[7]; // texel of the vertex (index 6) and of ring vertex k
    uint32_t in;    // bit k: ring vertex k exists
};
__device__ __forceinline__ bool ring_tri(uint32_t in, int k) { return ((in >> k) & (in >> ((k + 1) % 6)) & 1u) != 0u; }
// dh (optional): per-texel height tangents, returned in dX / dR
__device__ __forceinline__ void ring_world(const hf_dev_field &f, int i, int j, hf_ring &g, const float *dh = nullptr,
                                           float *dX = nullptr, float *dR = nullptr) {
    const int di[6] = { 0, 1, 1, 0, -1, -1 }, dj[6] = { 1, 0, -1, -1, 0, 1 };
    g.in = 0u;
    g.i[6] = i; g.j[6] = j;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int ii = i + di[k], jj = j + dj[k];
        const bool ok = ii >= 0 && ii < f.H && jj >= 0 && jj < f.W;
        g.i[k] = ok ? ii : i; g.j[k] = ok ? jj : j;
        g.in |= ok ? (1u << k) : 0u;
    }
    const size_t x = (size_t) i * f.W + j;
    g.X = grid_world(f, i, j, f.h[x]);
    if (dh) *dX = dh[x];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const size_t r = (size_t) g.i[k] * f.W + g.j[k];
        g.R[k] = grid_world(f, g.i[k], g.j[k], f.h[r]);
        if (dh) dR[k] = dh[r];
    }
}
// unit edge directions u_k = (R_k - X) l_k, l_k = 1 / |R_k - X|
__device__ __forceinline__ void ring_dirs(const hf_ring &g, v3 u[6], float l[6]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const v3 e = g.R[k] - g.X;
        l[k] = rsqrt_ieee(dot3(e, e));
        u[k] = e * l[k];
    }
}
// interior angle of triangle k at X: safe_acos(dot(d0, d1))
__device__ __forceinline__ float ring_angle(float c) { return acosf(fminf(fmaxf(c, -1.f), 1.f)); }
// d safe_acos(c) / dc (0 where the clamp is active)
__device__ __forceinline__ float ring_dangle(float c) { return (c > -1.f && c < 1.f) ? -rsqrt_ieee(1.f - c * c) : 0.f; }

// m = sum_k face_normal_k * angle_k; returns |m|^-1 in rm (the vertex normal is m rm)
__device__ __forceinline__ v3 ring_sum(const hf_ring &g, const v3 u[6], float &rm) {
    v3 m = mk3(0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (!ring_tri(g.in, k)) continue;
        const int k1 = (k + 1) % 6;
        const v3 nt = unit_normal(g.R[k] - g.X, g.R[k1] - g.X).n;
        m = fma3(nt, ring_angle(dot3(u[k], u[k1])), m);
    }
    rm = rsqrt_ieee(dot3(m, m));
    return m;
}
// world-space normal of grid vertex (i, j) (before flip_normals, which the reference applies after interpolation)
__device__ __forceinline__ v3 vertex_normal(const hf_dev_field &f, int i, int j) {
    hf_ring g;
    ring_world(f, i, j, g);
    v3 u[6];
    float l[6], rm;
    ring_dirs(g, u, l);
    const v3 m = ring_sum(g, u, rm);
    return m * rm;
}

// Tangent of vertex_normal: the heights of X and of ring vertex k move by dX, dR[k]; ez = dP/dh (third column of
// to_world times max_height).  dn = (dm - n <n, dm>) / |m| with dm = sum_k dface_k angle_k + face_k dangle_k.
__device__ __forceinline__ v3 vertex_normal_jvp(const hf_ring &g, v3 ez, float dX, const float dR[6]) {
    v3 u[6];
    float l[6], rm;
    ring_dirs(g, u, l);
    const v3 m = ring_sum(g, u, rm);
    v3 dm = mk3(0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (!ring_tri(g.in, k)) continue;
        const int k1 = (k + 1) % 6;
        const v3 e1 = g.R[k] - g.X, e2 = g.R[k1] - g.X;
        const v3 de1 = ez * (dR[k] - dX), de2 = ez * (dR[k1] - dX);
        const auto [nt, r] = unit_normal(e1, e2);
        const v3 dnt = dnormalize(nt, r, face_normal_jvp(e1, e2, de1, de2));
        const float c = dot3(u[k], u[k1]);
        const v3 du1 = (de1 - u[k] * dot3(u[k], de1)) * l[k], du2 = (de2 - u[k1] * dot3(u[k1], de2)) * l[k1];
        const float dth = ring_dangle(c) * (dot3(du1, u[k1]) + dot3(u[k], du2));
        axpy3(ring_angle(c), dnt, dm);
        axpy3(dth, nt, dm);
    }
    return dnormalize(m * rm, rm, dm);
}
// Transpose of vertex_normal_jvp: for the upstream gradient gn of the vertex normal, the gradients with respect to the
// heights of X (gX) and of ring vertex k (gR[k]; zero for absent neighbours).  The position gradients are contracted
// with ez as they arise (a height moves its vertex along ez only), so no per-edge vector accumulator is live:
//   d/de_k of face_k:   cross(e_k+1, gN),  d/de_k+1: cross(gN, e_k)
//   d/de_k of angle_k:  gc l_k (u_k+1 - u_k c)  (and symmetrically), c = <u_k, u_k+1>
__device__ __forceinline__ void vertex_normal_vjp(const hf_ring &g, v3 ez, v3 gn, float &gX, float gR[6]) {
    v3 u[6];
    float l[6], rm;
    ring_dirs(g, u, l);
    const v3 m = ring_sum(g, u, rm);
    const v3 gm = dnormalize(m * rm, rm, gn);
#pragma unroll
    for (int k = 0; k < 6; ++k) gR[k] = 0.f;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (!ring_tri(g.in, k)) continue;
        const int k1 = (k + 1) % 6;
        const v3 e1 = g.R[k] - g.X, e2 = g.R[k1] - g.X;
        const auto [nt, r] = unit_normal(e1, e2);
        const float c = dot3(u[k], u[k1]), th = ring_angle(c);
        float g1, g2;
        face_normal_vjp(e1, e2, dnormalize(nt, r, gm * th), ez, g1, g2);
        const float gc = ring_dangle(c) * dot3(nt, gm);
        const float ez0 = dot3(ez, u[k]), ez1 = dot3(ez, u[k1]);
        gR[k] += g1 + gc * l[k] * (ez1 - ez0 * c);
        gR[k1] += g2 + gc * l[k1] * (ez0 - ez1 * c);
    }
    gX = 0.f;
#pragma unroll
    for (int k = 0; k < 6; ++k) gX -= gR[k];
}

// The three vertex normals of a hit (rows vi, columns vj), evaluated on the fly from the heights.  VJP: for their
// gradients gB[k], the 1 + 6 height gradients of each vertex and its existing ring neighbours go to the sink
// add(row, column, g); JVP: for the height tangent dh, acc += sum_k w[k] dN_k.
template <typename Add>
__device__ __forceinline__ void vertex_normals_vjp(const hf_dev_field &f, const int vi[3], const int vj[3], v3 ez,
                                                   const v3 gB[3], Add add) {
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
        hf_ring g;
        ring_world(f, vi[k], vj[k], g);
        float gX, gR[6];
        vertex_normal_vjp(g, ez, gB[k], gX, gR);
        add(vi[k], vj[k], gX);
#pragma unroll
        for (int q = 0; q < 6; ++q)
            if ((g.in >> q) & 1u) add(g.i[q], g.j[q], gR[q]);
    }
}
__device__ __forceinline__ void vertex_normals_jvp(const hf_dev_field &f, const int vi[3], const int vj[3], v3 ez,
                                                   const float w[3], const float *dh, v3 &acc) {
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
        hf_ring g;
        float dX, dR[6];
        ring_world(f, vi[k], vj[k], g, dh, &dX, dR);
        axpy3(w[k], vertex_normal_jvp(g, ez, dX, dR), acc);
    }
}

// World-space forms of vertex_normal_vjp / _jvp for the transform derivatives, where a vertex moves in every
// direction: the gradient / the tangent dE[k] of each edge E_k = R_k - X of the ring.  Same ring geometry (ring_dirs,
// ring_sum) and the same per-triangle terms; the height forms above keep their contraction with ez.  The VJP hands each
// triangle's two edge gradients to the sink add(k, g) as they arise (no per-edge accumulator is live).
template <typename Add>
__device__ __forceinline__ void vertex_normal_vjp_world(const hf_ring &g, v3 gn, Add add) {
    v3 u[6];
    float l[6], rm;
    ring_dirs(g, u, l);
    const v3 m = ring_sum(g, u, rm);
    const v3 gm = dnormalize(m * rm, rm, gn);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (!ring_tri(g.in, k)) continue;
        const int k1 = (k + 1) % 6;
        const v3 e1 = g.R[k] - g.X, e2 = g.R[k1] - g.X;
        const auto [nt, r] = unit_normal(e1, e2);
        const float c = dot3(u[k], u[k1]), th = ring_angle(c);
        const v3 gN = dnormalize(nt, r, gm * th);
        const float gc = ring_dangle(c) * dot3(nt, gm);
        add(k, fma3(u[k1] - u[k] * c, gc * l[k], cross3(e2, gN)));
        add(k1, fma3(u[k] - u[k1] * c, gc * l[k1], cross3(gN, e1)));
    }
}
__device__ __forceinline__ v3 vertex_normal_jvp_world(const hf_ring &g, const v3 dE[6]) {
    v3 u[6];
    float l[6], rm;
    ring_dirs(g, u, l);
    const v3 m = ring_sum(g, u, rm);
    v3 dm = mk3(0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (!ring_tri(g.in, k)) continue;
        const int k1 = (k + 1) % 6;
        const v3 e1 = g.R[k] - g.X, e2 = g.R[k1] - g.X;
        const v3 de1 = dE[k], de2 = dE[k1];
        const auto [nt, r] = unit_normal(e1, e2);
        const v3 dnt = dnormalize(nt, r, face_normal_jvp(e1, e2, de1, de2));
        const float c = dot3(u[k], u[k1]);
        const v3 du1 = (de1 - u[k] * dot3(u[k], de1)) * l[k], du2 = (de2 - u[k1] * dot3(u[k1], de2)) * l[k1];
        const float dth = ring_dangle(c) * (dot3(du1, u[k1]) + dot3(u[k], du2));
        axpy3(ring_angle(c), dnt, dm);
        axpy3(dth, nt, dm);
    }
    return dnormalize(m * rm, rm, dm);
}
// object-space edge E_k of a ring: q(R_k) - q(X) (zero for an absent neighbour, which ring_world puts at X)
__device__ __forceinline__ v3 ring_local_edge(const hf_dev_field &f, const hf_ring &g, int k) {
    const float hx = f.h[(size_t) g.i[6] * f.W + g.j[6]], hk = f.h[(size_t) g.i[k] * f.W + g.j[k]];
    return grid_local(f, g.i[k], g.j[k], hk) - grid_local(f, g.i[6], g.j[6], hx);
}
// The three vertex normals of a hit for the transform: VJP: M += sum over the rings of gE[k] (x) E_k (the normals
// do not depend on the translation); JVP: acc += sum_k w[k] dN_k for the tangent dM of to_world and the height tangent
// dh (nullptr: zero), each edge moving by dM E_k + ez (dh_k - dh_X).
__device__ __forceinline__ void vertex_normals_vjp_xform(const hf_dev_field &f, const int vi[3], const int vj[3],
                                                         const v3 gB[3], float M[12]) {
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
        hf_ring g;
        ring_world(f, vi[k], vj[k], g);
        vertex_normal_vjp_world(g, gB[k], [&](int q, v3 gE) { xform_grad_vec(M, gE, ring_local_edge(f, g, q)); });
    }
}
__device__ __forceinline__ void vertex_normals_jvp_xform(const hf_dev_field &f, const int vi[3], const int vj[3], v3 ez,
                                                         const float w[3], const float *dh, const float dM[12], v3 &acc) {
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
        hf_ring g;
        float dX = 0.f, dR[6] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
        ring_world(f, vi[k], vj[k], g, dh, &dX, dR);
        v3 dE[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) dE[q] = fma3(ez, dR[q] - dX, xform_vec(dM, ring_local_edge(f, g, q)));
        axpy3(w[k], vertex_normal_jvp_world(g, dE), acc);
    }
}

// The three vertex normals of a hit from the handle's buffer (one 16-byte load each)
__device__ __forceinline__ void load_vn(const hf_dev_field &f, const float4 *vn, const int vi[3], const int vj[3], v3 N[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 q = vn[(size_t) vi[k] * f.W + vj[k]];
        N[k] = mk3(q.x, q.y, q.z);
    }
}
// The blend of the three vertex normals, in the reference's two association orders (they round differently): the
// surface interaction's fmadd(n2, b2, fmadd(n1, b1, n0 * b0)) (mesh.cpp:818) ...
__device__ __forceinline__ v3 bary_normal(const v3 N[3], float b0, float b1, float b2) {
    return mk3(__builtin_fmaf(N[2].x, b2, __builtin_fmaf(N[1].x, b1, N[0].x * b0)),
               __builtin_fmaf(N[2].y, b2, __builtin_fmaf(N[1].y, b1, N[0].y * b0)),
               __builtin_fmaf(N[2].z, b2, __builtin_fmaf(N[1].z, b1, N[0].z * b0)));
}
// ... and sample_position's fmadd(n0, b0, fmadd(n1, bx, n2 * by)) (mesh.cpp:599-600)
__device__ __forceinline__ v3 sample_blend(const v3 N[3], float b0, float bx, float by) {
    return mk3(__builtin_fmaf(N[0].x, b0, __builtin_fmaf(N[1].x, bx, N[2].x * by)),
               __builtin_fmaf(N[0].y, b0, __builtin_fmaf(N[1].y, bx, N[2].y * by)),
               __builtin_fmaf(N[0].z, b0, __builtin_fmaf(N[1].z, bx, N[2].z * by)));
}

// Shape::compute_surface_interaction + finalize_surface_interaction for one valid hit, from the hit-geometry helpers
// above (hf_adjoint_kernel and hf_tangent_kernel differentiate the same quantities).
// SMOOTH (vn: the handle's vertex normals): sh_n is the interpolated vertex normal (mesh.cpp:813-840) when smooth_sh(flags),
// and the shading frame and wi are built on it; the sink then takes n and sh_n separately (n_face / sh_n).
// The fields are handed to `out` as soon as they are final (out.t(..), out.p(..), ...): the record sink below collects
// them into an hf_si_rec; the fused traversal kernel stores each one straight away, so that the whole record is
// never live in registers at once.
template <bool SMOOTH = false, typename Out>
__device__ __forceinline__ void compute_si_to(const hf_dev_field &f, v3 o, v3 d, float t_in, float b1, float b2,
                                              uint32_t prim, uint32_t flags, Out &out, const float4 *vn = nullptr) {
    v3 P[3];
    float U[3], V[3];
    int vi[3], vj[3];
    prim_world(f, prim, P, U, V, vi, vj);
    v3 NV[3];
    if (SMOOTH && smooth_sh(flags)) load_vn(f, vn, vi, vj, NV); // (issued with the heights)
    const float b0 = 1.f - b1 - b2;
    const v3 dp0 = P[1] - P[0], dp1 = P[2] - P[0];
    const v3 p = bary_point(P, b0, b1, b2);
    float t = t_in;
    if (flags & HF_RAY_FOLLOWSHAPE) t = follow_t(p, o, d).tt;
    out.t(t);
    out.p(p);
    if (flags & HF_RAY_BOUNDARYTEST)
        // HF_RAY_BOUNDARY_ALL_EDGES (a libhf extension bit): the reference Mesh's per-triangle SDF over all
        // three edges (mesh.cpp:845-890, values in [0, 1]) instead of the silhouette edges only
        out.boundary_test(boundary_test_flat(p, P[0], dp0, dp1, (flags & HF_RAY_BOUNDARY_ALL_EDGES) ? 7u : silhouette_edges(f, prim, xform_vec(f.to_object, d))));
    else
        out.boundary_test(0.f);
    v3 n = unit_normal(dp0, dp1).n;
    float uv0 = b1, uv1 = b2;
    v3 dp_du, dp_dv;
    coordinate_system(n, dp_du, dp_dv);
    if (flags & (HF_RAY_UV | HF_RAY_DPDUV)) {
        uv0 = __builtin_fmaf(U[2], b2, __builtin_fmaf(U[1], b1, U[0] * b0));
        uv1 = __builtin_fmaf(V[2], b2, __builtin_fmaf(V[1], b1, V[0] * b0));
        if (flags & HF_RAY_DPDUV) {
            const hf_uv_diff g = uv_diff(U, V);
            if (g.det != 0.f) {
                dp_du = mk3(__builtin_fmaf(g.dv1, dp0.x, -(g.dv0 * dp1.x)) * g.inv_det,
                            __builtin_fmaf(g.dv1, dp0.y, -(g.dv0 * dp1.y)) * g.inv_det,
                            __builtin_fmaf(g.dv1, dp0.z, -(g.dv0 * dp1.z)) * g.inv_det);
                dp_dv = mk3(__builtin_fmaf(-g.du1, dp0.x, g.du0 * dp1.x) * g.inv_det,
                            __builtin_fmaf(-g.du1, dp0.y, g.du0 * dp1.y) * g.inv_det,
                            __builtin_fmaf(-g.du1, dp0.z, g.du0 * dp1.z) * g.inv_det);
            }
        }
    }
    out.uv(uv0, uv1);
    out.dp_dv(dp_dv);
    if (f.flip) n = neg3(n);
    if constexpr (SMOOTH) {
        out.n_face(n);
        if (smooth_sh(flags)) {
            n = normalize3(bary_normal(NV, b0, b1, b2));
            if (f.flip) n = neg3(n); // (after the interpolation, mesh.cpp:837-840)
        }
        out.sh_n(n); // n is sh_n from here on
    } else {
        out.n(n); // n and sh_n
    }
    v3 sh_s = mk3(0.f, 0.f, 0.f), sh_t = mk3(0.f, 0.f, 0.f);
    if (flags & HF_RAY_SHADINGFRAME) { // initialize_sh_frame: Gram-Schmidt on dp_du
        const float nd = -dot3(n, dp_du);
        sh_s = normalize3(fma3(n, nd, dp_du));
        if (dp_du.x == 0.f && dp_du.y == 0.f && dp_du.z == 0.f) {
            v3 dummy;
            coordinate_system(n, sh_s, dummy);
        }
        sh_t = cross3(n, sh_s);
    }
    out.dp_du(dp_du);
    out.sh_s(sh_s);
    out.sh_t(sh_t);
    const v3 md = neg3(d);
    out.wi(mk3(dot3(md, sh_s), dot3(md, sh_t), dot3(md, n)));
}

// The zero-initialised record of a missed or inactive lane (interaction.h:479-499, 667-673), in compute_si_to's field
// order, up to wi: a caller that stores wi (= -d) does so itself, after this (passed in here, the negation moved within
// the fused traversal kernel's schedule).
template <typename Out>
__device__ __forceinline__ void si_miss_to(Out &out, uint32_t flags) {
    const v3 z = mk3(0.f, 0.f, 0.f);
    out.t(__builtin_inff()); out.p(z); out.boundary_test((flags & HF_RAY_BOUNDARYTEST) ? 1e8f : 0.f);
    out.uv(0.f, 0.f); out.dp_dv(z); out.n(z); out.dp_du(z); out.sh_s(z); out.sh_t(z);
}

struct hf_si_rec_sink {
    hf_si_rec &si;
    __device__ __forceinline__ void t(float v) { si.t = v; }
    __device__ __forceinline__ void p(v3 v) { si.p = v; }
    __device__ __forceinline__ void boundary_test(float v) { si.boundary_test = v; }
    __device__ __forceinline__ void uv(float a, float b) { si.uv0 = a; si.uv1 = b; }
    __device__ __forceinline__ void dp_du(v3 v) { si.dp_du = v; }
    __device__ __forceinline__ void dp_dv(v3 v) { si.dp_dv = v; }
    __device__ __forceinline__ void n(v3 v) { si.n = v; si.sh_n = v; }
    __device__ __forceinline__ void n_face(v3 v) { si.n = v; }
    __device__ __forceinline__ void sh_n(v3 v) { si.sh_n = v; }
    __device__ __forceinline__ void sh_s(v3 v) { si.sh_s = v; }
    __device__ __forceinline__ void sh_t(v3 v) { si.sh_t = v; }
    __device__ __forceinline__ void wi(v3 v) { si.wi = v; }
};
__device__ __forceinline__ void compute_si(const hf_dev_field &f, v3 o, v3 d, float t_in, float b1, float b2,
                                           uint32_t prim, uint32_t flags, hf_si_rec &si) {
    hf_si_rec_sink sink = { si };
    compute_si_to(f, o, d, t_in, b1, b2, prim, flags, sink);
}

// ---- eval_parameterization (hf_eval_parameterization and its adjoint / tangent): the triangle of the grid whose texcoords
// contain the query (u, v), in closed form.  Mesh traces the ray o = (u, v, -1), d = (0, 0, 1) against a copy of itself
// whose vertices are the texcoords (mesh.cpp:503-545, 614-635); the heightfield's texcoords are the regular grid
// (j / (W-1), i / (H-1)), so the cell is a floor and the triangle one comparison.  The domain is Moeller-Trumbore's
// inclusive one, 0 <= u, v <= 1 (NaN fails every test); ties go to the highest prim_index, as for a hit: a point on a cell
// border to the higher cell (the floor), u = 1 / v = 1 to the last cell (the min), the diagonal to tri 1 (fx + fy >= 1,
// decided exactly: 1 - fy is exact for fy >= 1/2 and 1 - fx for fx > 1/2, Sterbenz).  fx = fma(u, W-1, -cx) is rounded
// once, so float64 arithmetic on the host reproduces every value bit for bit (tests/param_ref.py).  b = (b1, b2) in the
// vertex order of prim_vertex_ids: tri 0 = (v00, v10, v01): (fx, fy); tri 1 = (v11, v01, v10): (1 - fx, 1 - fy). ----
__device__ __forceinline__ bool param_lookup(int W, int H, float u, float v, uint32_t &prim, float &b1, float &b2) {
    if (!((u >= 0.f) & (u <= 1.f) & (v >= 0.f) & (v <= 1.f))) return false;
    const float cw = (float) (W - 1), ch = (float) (H - 1);
    const float cxf = fminf(floorf(u * cw), (float) (W - 2)), cyf = fminf(floorf(v * ch), (float) (H - 2));
    const float fx = clamp01(__builtin_fmaf(u, cw, -cxf)), fy = clamp01(__builtin_fmaf(v, ch, -cyf));
    const bool tri1 = fy >= 0.5f ? fx >= 1.f - fy : fy >= 1.f - fx;
    prim = 2u * ((uint32_t) cyf * (uint32_t) (W - 1) + (uint32_t) cxf) + (tri1 ? 1u : 0u);
    b1 = tri1 ? 1.f - fx : fx;
    b2 = tri1 ? 1.f - fy : fy;
    return true;
}

// ---- Area sampling (hf_set_area_sampling): the discrete distribution of Mesh::build_pmf (mesh.cpp:401-432) over the
// triangles in prim_index order, and what Mesh::sample_position (mesh.cpp:557-610) reads of it. ----

// world-space area of the triangle (p0, p1, p2): .5f * norm(cross(p1 - p0, p2 - p0)), norm = sqrt(dot(v, v))
__device__ __forceinline__ float tri_area(v3 p0, v3 p1, v3 p2) {
    const v3 c = cross3(p1 - p0, p2 - p0);
    return 0.5f * __builtin_sqrtf(dot3(c, c));
}

// The scalars of DiscreteDistribution::compute_cdf (distr_1d.h:212-240), written by the table build on the device so
// that the sampling kernels (captured ones included) read those of the last rebuild.
struct hf_area_info {
    double sum;        // the fp64 total
    float sum_f;       // m_sum = (float) sum
    float norm;        // m_normalization = (float) (1.0 / sum)
    uint32_t valid_lo; // m_valid: first and last entry with a non-zero area
    uint32_t valid_hi;
};
