// P1 cell geometry shared by the assembly kernels (fs_assemble.hip) and, through fs_p1_cell.h, the solid-mechanics kernel files.
#pragma once
#include "fs_common.h"

// ---- P1 geometry ---------------------------------------------------------------------------
struct tet_geom {
    double g[4][3];  // gradients of the barycentric basis
    double adet;     // |det J|
};

// 16 + 8 bytes: the pad of the 32-byte record is not fetched (the gather kernels are bound by the bytes their lanes pull
// through the per-CU address path, not by HBM)
__device__ __forceinline__ void load_vertex(const double* __restrict__ xyz4, int32_t v, double (&x)[3]) {
    const double2 a = reinterpret_cast<const double2*>(xyz4)[2 * (int64_t)v];
    x[0] = a.x; x[1] = a.y; x[2] = xyz4[4 * (int64_t)v + 2];
}

__device__ __forceinline__ tet_geom tet_geometry_x(const double (&x0)[3], const double (&x1)[3], const double (&x2)[3],
                                                   const double (&x3)[3]);
__device__ __forceinline__ tet_geom tet_geometry(const double* __restrict__ xyz4, const int32_t (&v)[4]) {
    double x0[3], x1[3], x2[3], x3[3];
    load_vertex(xyz4, v[0], x0);
    load_vertex(xyz4, v[1], x1);
    load_vertex(xyz4, v[2], x2);
    load_vertex(xyz4, v[3], x3);
    return tet_geometry_x(x0, x1, x2, x3);
}
// snap: grid spacing of a uniform box mesh and its reciprocal (fs_mesh_s::box_h; 0 = general mesh).  An edge-vector component of a
// box cell is -h, 0 or +h up to the rounding of the two coordinates it is the difference of; h * rint(e / h) removes exactly that
// noise, so every cell of the same Kuhn type yields the same bits wherever it sits.
struct box_snap { double h[3], inv[3]; };
__device__ __forceinline__ tet_geom tet_geometry_e(const double (&e1)[3], const double (&e2)[3], const double (&e3)[3]);
__device__ __forceinline__ tet_geom tet_geometry_x(const double (&x0)[3], const double (&x1)[3], const double (&x2)[3],
                                                   const double (&x3)[3]) {
    const double e1[3] = {x1[0] - x0[0], x1[1] - x0[1], x1[2] - x0[2]};
    const double e2[3] = {x2[0] - x0[0], x2[1] - x0[1], x2[2] - x0[2]};
    const double e3[3] = {x3[0] - x0[0], x3[1] - x0[1], x3[2] - x0[2]};
    return tet_geometry_e(e1, e2, e3);
}
__device__ __forceinline__ tet_geom tet_geometry_snapped(const double (&x0)[3], const double (&x1)[3], const double (&x2)[3],
                                                         const double (&x3)[3], const box_snap& bx) {
    double e1[3], e2[3], e3[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        e1[d] = bx.h[d] * rint((x1[d] - x0[d]) * bx.inv[d]);
        e2[d] = bx.h[d] * rint((x2[d] - x0[d]) * bx.inv[d]);
        e3[d] = bx.h[d] * rint((x3[d] - x0[d]) * bx.inv[d]);
    }
    return tet_geometry_e(e1, e2, e3);
}
__device__ __forceinline__ tet_geom tet_geometry_box(const double* __restrict__ xyz4, const int32_t (&v)[4], const box_snap& bx);
__device__ __forceinline__ tet_geom tet_geometry_e(const double (&e1)[3], const double (&e2)[3], const double (&e3)[3]) {
    // cofactors: grad lambda_1 = (e2 x e3)/det, grad lambda_2 = (e3 x e1)/det, grad lambda_3 = (e1 x e2)/det
    const double c1[3] = {e2[1] * e3[2] - e2[2] * e3[1], e2[2] * e3[0] - e2[0] * e3[2], e2[0] * e3[1] - e2[1] * e3[0]};
    const double c2[3] = {e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]};
    const double c3[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double det = e1[0] * c1[0] + e1[1] * c1[1] + e1[2] * c1[2];
    const double inv = 1.0 / det;
    tet_geom t;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        t.g[1][d] = c1[d] * inv;
        t.g[2][d] = c2[d] * inv;
        t.g[3][d] = c3[d] * inv;
        t.g[0][d] = -(t.g[1][d] + t.g[2][d] + t.g[3][d]);
    }
    t.adet = fabs(det);
    return t;
}

// general mesh: the plain geometry; uniform box (bx.h > 0): edge vectors snapped to the grid spacing
__device__ __forceinline__ tet_geom tet_geometry_box(const double* __restrict__ xyz4, const int32_t (&v)[4], const box_snap& bx) {
    double x0[3], x1[3], x2[3], x3[3];
    load_vertex(xyz4, v[0], x0);
    load_vertex(xyz4, v[1], x1);
    load_vertex(xyz4, v[2], x2);
    load_vertex(xyz4, v[3], x3);
    return bx.h[0] > 0.0 ? tet_geometry_snapped(x0, x1, x2, x3, bx) : tet_geometry_x(x0, x1, x2, x3);
}

// ---- 2-D: CG1 on triangles
struct tri_geom {
    double g[3][2];   // gradients of the barycentric basis
    double area;
};
__device__ __forceinline__ tri_geom tri_geometry2(const double* __restrict__ xyz4, int32_t a, int32_t b, int32_t c) {
    const double2 p0 = reinterpret_cast<const double2*>(xyz4)[2 * (int64_t)a];
    const double2 p1 = reinterpret_cast<const double2*>(xyz4)[2 * (int64_t)b];
    const double2 p2 = reinterpret_cast<const double2*>(xyz4)[2 * (int64_t)c];
    const double e1x = p1.x - p0.x, e1y = p1.y - p0.y, e2x = p2.x - p0.x, e2y = p2.y - p0.y;
    const double det = e1x * e2y - e1y * e2x;
    const double inv = 1.0 / det;
    tri_geom t;
    t.g[1][0] = e2y * inv;  t.g[1][1] = -e2x * inv;
    t.g[2][0] = -e1y * inv; t.g[2][1] = e1x * inv;
    t.g[0][0] = -(t.g[1][0] + t.g[2][0]);
    t.g[0][1] = -(t.g[1][1] + t.g[2][1]);
    t.area = 0.5 * fabs(det);
    return t;
}

// the snap of a uniform box mesh (zero spacing for other meshes, or with the option "box_snap" / FS_BOX_SNAP=0 off)
box_snap make_box_snap(const fs_mesh_s* m);
