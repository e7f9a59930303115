// Mixed (u, v, p) large-deformation elasticity on CG1 (tetrahedra and triangles): the reduced Newton system of one Crank-Nicolson
// step, on the device.
//
// Stands in for the residual and derivative(F, w) of FenicsSolver/LargeDeformationSolver.py:80-135 that solve(F == 0, w, bcs, J)
// assembles at every Newton iterate.  With F = I + grad u, J = det F, cof = J F^-T, S = J (-p I + mu (B - I)) F^-T
// = mu J F - (p + mu) cof and pp = p / lambda + J^2 - 1:
//   R_u = M r_u,  r_u = (u - u0)/dt - q v - (1-q) v0                           (nodal, per component)
//   R_v = M (v - v0)/dt + q int S : grad _v + (1-q) int S0 : grad _v + follower loads int cof g . _v ds + int f . _v
//   R_p = q int pp _p + (1-q) int pp0 _p
// A P1 displacement has a constant gradient per cell and S is linear in the P1 pressure, so every volume integrand is integrated in
// closed form (cell mean of p; int phi_b = V/(d+1); M_ab = V (1 + delta_ab) / ((d+1)(d+2))).  With G_b = F^-T g_b:
//   dS g_a / du_bk [i] = mu J (G_b[k] (F g_a)_i + delta_ik g_a.g_b) - (p + mu) J (G_b[k] G_a[i] - G_b[i] G_a[k])
//   d cof g / du_bk [i] = J (G_b[k] (F^-T g)_i - G_b[i] (F^-T g)_k)
// The u rows are linear: du = dt (q dv - r_u) wherever the displacement component is free, 0 where it is Dirichlet.  Eliminating du
// leaves one 4 x 4 block per vertex (v_x, v_y, v_z, p) - on triangles (v_x, v_y, -, p) with a dummy identity slot:
//   [ J_vv + dt q J_vu     J_vp ] [dv]   [ -R_v + dt J_vu r_u ]
//   [ dt q J_pu            J_pp ] [dp] = [ -R_p + dt J_pu r_u ]
// with the J_xu columns of Dirichlet displacement components dropped.  Dirichlet rows of v and p become identity rows with a zero
// right-hand side.
//
// Kernels (no atomics: two assemblies of one state give the same bits):
//   k_ld_jacobian<TD>   one thread per STORED block sums its (cell, a, b) sources of the gather map in ascending order and rebuilds
//                       F, cof(F) and the cell mean of p per source (as k_hyper_tangent_gather does).
//   k_ld_facets<TD>     one thread per loaded facet: its follower-load vector and the u-derivative blocks, to a per-facet buffer.
//   k_ld_facet_entries  one thread per stored block that a loaded facet touches: adds dt q dcof/du over its facet sources in order.
//   k_ld_nodes<TD>      one thread per node: R_u, R_v, R_p over the cells around the node (ascending), the J_xu r_u corrections,
//                       the facet loads of the node, the reduced right-hand side, the squared full residual of the node (Dirichlet
//                       rows left out) and the identity rows of Dirichlet v / p unknowns.
//   k_ld_cells<TD> + k_ld_finish   cells with J == 0 or J not finite, and the fixed-order sum of the node residuals.  The workgroup
//                       part is p1_cell_tally (fs_p1_cell.h); k_ld_finish keeps its own order (a strided sum per thread, then a tree
//                       in LDS), which the one-thread k_cell_tally_finish would change.
#include "fs_common.h"
#include "fs_kernels.h"
#include "fs_p1_cell.h"
#include <math.h>
#include <algorithm>
#include <numeric>
#include <vector>

#define FS_LD_BLOCKS 512      // workgroups of the reductions (their partials are summed in this order)

namespace {

template <int TD>
struct ld_cell {
    double g[TD + 1][TD];     // reference gradients of the barycentric functions
    double vol;
    double F[TD][TD], FiT[TD][TD], J;
    int32_t v[TD + 1];
};

template <int TD>
__device__ __forceinline__ void ld_geometry(const int32_t* __restrict__ cells, const double* __restrict__ xyz4, int64_t c,
                                            const box_snap& bx, ld_cell<TD>& k) {
    const int4 v4 = reinterpret_cast<const int4*>(cells)[c];
    if constexpr (TD == 3) {
        const int32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
        const tet_geom t = tet_geometry_box(xyz4, v, bx);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            k.v[a] = v[a];
#pragma unroll
            for (int j = 0; j < 3; ++j) k.g[a][j] = t.g[a][j];
        }
        k.vol = t.adet * (1.0 / 6.0);
    } else {
        const tri_geom t = tri_geometry2(xyz4, v4.x, v4.y, v4.z);
        k.v[0] = v4.x; k.v[1] = v4.y; k.v[2] = v4.z;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int j = 0; j < 2; ++j) k.g[a][j] = t.g[a][j];
        k.vol = t.area;
    }
}

// F = I + sum_a u_a g_a^T, F^-T = cof / J, J
// (hyper_kin3 / hyper_kin2 of fs_hyper.hip compute the same F but group the sum over the vertices ((a0 + a1) + a2) + a3, where this
// one accumulates from 0: the two round differently, so each file keeps its own.)
template <int TD>
__device__ __forceinline__ void ld_kinematics(const double* __restrict__ u, ld_cell<TD>& k) {
    double uv[TD + 1][TD];
#pragma unroll
    for (int a = 0; a <= TD; ++a)
#pragma unroll
        for (int i = 0; i < TD; ++i) uv[a][i] = u[(int64_t)TD * k.v[a] + i];
#pragma unroll
    for (int i = 0; i < TD; ++i)
#pragma unroll
        for (int j = 0; j < TD; ++j) {
            double s = 0.0;
#pragma unroll
            for (int a = 0; a <= TD; ++a) s += uv[a][i] * k.g[a][j];
            k.F[i][j] = (i == j ? 1.0 : 0.0) + s;
        }
    if constexpr (TD == 3) {
        const auto& F = k.F;
        double c[3][3];
        c[0][0] = F[1][1] * F[2][2] - F[1][2] * F[2][1];
        c[0][1] = F[1][2] * F[2][0] - F[1][0] * F[2][2];
        c[0][2] = F[1][0] * F[2][1] - F[1][1] * F[2][0];
        c[1][0] = F[0][2] * F[2][1] - F[0][1] * F[2][2];
        c[1][1] = F[0][0] * F[2][2] - F[0][2] * F[2][0];
        c[1][2] = F[0][1] * F[2][0] - F[0][0] * F[2][1];
        c[2][0] = F[0][1] * F[1][2] - F[0][2] * F[1][1];
        c[2][1] = F[0][2] * F[1][0] - F[0][0] * F[1][2];
        c[2][2] = F[0][0] * F[1][1] - F[0][1] * F[1][0];
        k.J = F[0][0] * c[0][0] + F[0][1] * c[0][1] + F[0][2] * c[0][2];
        const double inv = 1.0 / k.J;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) k.FiT[i][j] = c[i][j] * inv;
    } else {
        const auto& F = k.F;
        k.J = F[0][0] * F[1][1] - F[0][1] * F[1][0];
        const double inv = 1.0 / k.J;
        k.FiT[0][0] = F[1][1] * inv;  k.FiT[0][1] = -F[1][0] * inv;
        k.FiT[1][0] = -F[0][1] * inv; k.FiT[1][1] = F[0][0] * inv;
    }
}

// cell mean of the P1 pressure (slot 3 of the block vector)
template <int TD>
__device__ __forceinline__ double ld_pmean(const double* __restrict__ w, const ld_cell<TD>& k) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a <= TD; ++a) s += w[4 * (int64_t)k.v[a] + 3];
    return s * (1.0 / (TD + 1));
}

template <int TD>
__device__ __forceinline__ void ld_mul_FiT(const ld_cell<TD>& k, const double* x, double* y) {
#pragma unroll
    for (int i = 0; i < TD; ++i) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < TD; ++j) s += k.FiT[i][j] * x[j];
        y[i] = s;
    }
}

// internal force V S g_a = V (mu J F g_a - (p + mu) J G_a)
template <int TD>
__device__ __forceinline__ void ld_force(const ld_cell<TD>& k, int a, double p, double mu, double* f) {
    double Ga[TD];
    ld_mul_FiT(k, k.g[a], Ga);
#pragma unroll
    for (int i = 0; i < TD; ++i) {
        double Fg = 0.0;
#pragma unroll
        for (int j = 0; j < TD; ++j) Fg += k.F[i][j] * k.g[a][j];
        f[i] = k.vol * (mu * k.J * Fg - (p + mu) * k.J * Ga[i]);
    }
}

// Kt[i][k] = d (V S g_a)_i / d u_bk
template <int TD>
__device__ __forceinline__ void ld_tangent(const ld_cell<TD>& k, int a, int b, double p, double mu, double (&Kt)[TD][TD]) {
    double Ga[TD], Gb[TD], Fga[TD];
    ld_mul_FiT(k, k.g[a], Ga);
    ld_mul_FiT(k, k.g[b], Gb);
    double gg = 0.0;
#pragma unroll
    for (int j = 0; j < TD; ++j) gg += k.g[a][j] * k.g[b][j];
#pragma unroll
    for (int i = 0; i < TD; ++i) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < TD; ++j) s += k.F[i][j] * k.g[a][j];
        Fga[i] = s;
    }
    const double mJ = mu * k.J, pJ = (p + mu) * k.J;
#pragma unroll
    for (int i = 0; i < TD; ++i)
#pragma unroll
        for (int q = 0; q < TD; ++q)
            Kt[i][q] = k.vol * (mJ * (Gb[q] * Fga[i] + (i == q ? gg : 0.0)) - pJ * (Gb[q] * Ga[i] - Gb[i] * Ga[q]));
}

struct ld_params {
    double dt, q, mu, lambda;
    double body[3];
};

// bits of the per-node Dirichlet mask (fs_ld_form.dirichlet)
__device__ __forceinline__ bool ld_u_free(const uint8_t* __restrict__ dm, int32_t node, int k) { return !((dm[node] >> k) & 1); }

// ---- the reduced Jacobian --------------------------------------------------------------------------------------------------
template <int TD>
__global__ void __launch_bounds__(FS_BLOCK) k_ld_jacobian(int64_t n_entries, const int32_t* __restrict__ ptr, const int32_t* __restrict__ src,
                                                          const int32_t* __restrict__ cells, const double* __restrict__ xyz4,
                                                          const double* __restrict__ u, const double* __restrict__ w,
                                                          const uint8_t* __restrict__ dm, const ld_params P, const box_snap bx,
                                                          int64_t plane, double* __restrict__ val) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const double q = P.q, dt = P.dt, mu = P.mu;
    const double mc = 1.0 / ((TD + 1) * (TD + 2)), ic = 1.0 / (TD + 1);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_entries; e += stride) {
        double acc[4][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
        const int32_t q1 = ptr[e + 1];
        for (int32_t s = ptr[e]; s < q1; ++s) {
            int64_t c;
            int a, b;
            p1_source<TD>(src[s], c, a, b);
            ld_cell<TD> k;
            ld_geometry<TD>(cells, xyz4, c, bx, k);
            ld_kinematics<TD>(u, k);
            const double p = ld_pmean<TD>(w, k);
            const double Mab = k.vol * (a == b ? 2.0 : 1.0) * mc;
            double Kt[TD][TD], Ga[TD], Gb[TD];
            ld_tangent<TD>(k, a, b, p, mu, Kt);
            ld_mul_FiT(k, k.g[a], Ga);
            ld_mul_FiT(k, k.g[b], Gb);
            const int32_t nb = k.v[b];
#pragma unroll
            for (int kk = 0; kk < TD; ++kk) {
                const bool fr = ld_u_free(dm, nb, kk);
#pragma unroll
                for (int i = 0; i < TD; ++i) {
                    double x = i == kk ? Mab / dt : 0.0;
                    if (fr) x += dt * q * q * Kt[i][kk];
                    acc[i][kk] += x;
                }
                if (fr) acc[3][kk] += dt * q * q * 2.0 * k.J * k.J * Gb[kk] * k.vol * ic;
            }
#pragma unroll
            for (int i = 0; i < TD; ++i) acc[i][3] += -q * k.J * Ga[i] * k.vol * ic;
            acc[3][3] += q / P.lambda * Mab;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) val[(int64_t)(i * 4 + j) * plane + e] = acc[i][j];
    }
}

// ---- follower loads ---------------------------------------------------------------------------------------------------------
// fr[f][TD]: (|facet| / TD) cof(F) g, the load of each facet vertex; fk[f][b][TD][TD]: its derivative with respect to u_b (b: local
// vertex of the facet's cell)
template <int TD>
__global__ void __launch_bounds__(FS_BLOCK) k_ld_facets(int64_t nf, const int32_t* __restrict__ fcell, const int32_t* __restrict__ fopp,
                                                        const double* __restrict__ fg, const int32_t* __restrict__ cells,
                                                        const double* __restrict__ xyz4, const double* __restrict__ u, const box_snap bx,
                                                        double* __restrict__ fr, double* __restrict__ fk) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < nf; f += stride) {
        ld_cell<TD> k;
        ld_geometry<TD>(cells, xyz4, fcell[f], bx, k);
        ld_kinematics<TD>(u, k);
        const int o = fopp[f];
        double x[TD][3];
        int t = 0;
#pragma unroll
        for (int a = 0; a <= TD; ++a) {
            if (a == o) continue;
            load_vertex(xyz4, k.v[a], x[t]);
            ++t;
        }
        double area;
        if constexpr (TD == 3) {
            const double e1[3] = {x[1][0] - x[0][0], x[1][1] - x[0][1], x[1][2] - x[0][2]};
            const double e2[3] = {x[2][0] - x[0][0], x[2][1] - x[0][1], x[2][2] - x[0][2]};
            const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
            area = 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
        } else {
            const double dx = x[1][0] - x[0][0], dy = x[1][1] - x[0][1];
            area = sqrt(dx * dx + dy * dy);
        }
        const double wJ = area * (1.0 / TD) * k.J;
        double g[TD], h[TD];
#pragma unroll
        for (int i = 0; i < TD; ++i) g[i] = fg[3 * f + i];
        ld_mul_FiT(k, g, h);
#pragma unroll
        for (int i = 0; i < TD; ++i) fr[TD * f + i] = wJ * h[i];
#pragma unroll
        for (int b = 0; b <= TD; ++b) {
            double Gb[TD];
            ld_mul_FiT(k, k.g[b], Gb);
#pragma unroll
            for (int i = 0; i < TD; ++i)
#pragma unroll
                for (int kk = 0; kk < TD; ++kk)
                    fk[(((f * (TD + 1) + b) * TD) + i) * TD + kk] = wJ * (Gb[kk] * h[i] - Gb[i] * h[kk]);
        }
    }
}

// keys of the facet sources: the stored block of (facet vertex t, cell vertex b) and the node of facet vertex t
template <int TD>
__global__ void k_ld_facet_keys(int64_t nf, int64_t nc, const int32_t* __restrict__ fcell, const int32_t* __restrict__ fopp,
                                const int32_t* __restrict__ cells, const int32_t* __restrict__ slots, int32_t* __restrict__ ekey,
                                int32_t* __restrict__ nkey) {
    constexpr int NV = TD + 1;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < nf; f += stride) {
        const int64_t c = fcell[f];
        const int o = fopp[f];
        const int4 v4 = reinterpret_cast<const int4*>(cells)[c];
        const int32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
        int t = 0;
        for (int a = 0; a < NV; ++a) {
            if (a == o) continue;
            nkey[f * TD + t] = v[a];
            for (int b = 0; b < NV; ++b) ekey[(f * TD + t) * NV + b] = slots[(int64_t)(a * NV + b) * nc + c];      // slots[ab * nc + c]
            ++t;
        }
    }
}

// entries touched by facets: += dt q dcof/du_b (the columns of Dirichlet displacement components dropped)
template <int TD>
__global__ void k_ld_facet_entries(int64_t n_touched, const int32_t* __restrict__ ent, const int32_t* __restrict__ eptr,
                                   const int32_t* __restrict__ esrc, const int32_t* __restrict__ fcell, const int32_t* __restrict__ cells,
                                   const double* __restrict__ fk, const uint8_t* __restrict__ dm, double dtq, int64_t plane,
                                   double* __restrict__ val) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_touched; t += stride) {
        double acc[TD][TD] = {};
        for (int32_t s = eptr[t]; s < eptr[t + 1]; ++s) {
            const int32_t fb = esrc[s];                 // f * (TD + 1) + b
            const int64_t f = fb / (TD + 1);
            const int b = fb - (int32_t)(f * (TD + 1));
            const int4 v4 = reinterpret_cast<const int4*>(cells)[fcell[f]];
            const int32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int kk = 0; kk < TD; ++kk) {
                if (!ld_u_free(dm, v[b], kk)) continue;
#pragma unroll
                for (int i = 0; i < TD; ++i) acc[i][kk] += dtq * fk[((int64_t)fb * TD + i) * TD + kk];
            }
        }
        const int64_t e = ent[t];
#pragma unroll
        for (int i = 0; i < TD; ++i)
#pragma unroll
            for (int kk = 0; kk < TD; ++kk) val[(int64_t)(i * 4 + kk) * plane + e] += acc[i][kk];
    }
}

// ---- residuals, right-hand side, Dirichlet rows ----------------------------------------------------------------------------
template <int TD>
__global__ void __launch_bounds__(FS_BLOCK) k_ld_nodes(int64_t n_rows, const int64_t* __restrict__ slice_ptr, const int32_t* __restrict__ sell_col,
                                                       const int32_t* __restrict__ gptr, const int32_t* __restrict__ gsrc,
                                                       const int32_t* __restrict__ cells, const double* __restrict__ xyz4,
                                                       const double* __restrict__ u, const double* __restrict__ w,
                                                       const double* __restrict__ u0, const double* __restrict__ w0,
                                                       const uint8_t* __restrict__ dm, const ld_params P, const box_snap bx,
                                                       const int32_t* __restrict__ nptr, const int32_t* __restrict__ nsrc,
                                                       const int32_t* __restrict__ fcell, const double* __restrict__ fr,
                                                       const double* __restrict__ fk, int64_t plane, double* __restrict__ val,
                                                       double* __restrict__ rhs, double* __restrict__ rn2) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const double q = P.q, dt = P.dt, mu = P.mu, il = 1.0 / P.lambda;
    const double mc = 1.0 / ((TD + 1) * (TD + 2)), ic = 1.0 / (TD + 1);
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += stride) {
        const int64_t e = p1_diag_entry(r, slice_ptr, sell_col);
        double Ru[TD] = {}, Rv[TD] = {}, Rp = 0.0, cv[TD] = {}, cp = 0.0;
        if (e >= 0) {
            for (int32_t s = gptr[e]; s < gptr[e + 1]; ++s) {
                int64_t c;
                int a, bb;
                p1_source<TD>(gsrc[s], c, a, bb);
                ld_cell<TD> k, k0;
                ld_geometry<TD>(cells, xyz4, c, bx, k);
                k0 = k;
                ld_kinematics<TD>(u, k);
                ld_kinematics<TD>(u0, k0);
                const double p = ld_pmean<TD>(w, k), p0 = ld_pmean<TD>(w0, k0);
#pragma unroll
                for (int b = 0; b <= TD; ++b) {
                    const int64_t nb = k.v[b];
                    const double Mab = k.vol * (a == b ? 2.0 : 1.0) * mc;
                    double ru[TD];
#pragma unroll
                    for (int i = 0; i < TD; ++i) {
                        const double rui = (u[TD * nb + i] - u0[TD * nb + i]) / dt - q * w[4 * nb + i] - (1.0 - q) * w0[4 * nb + i];
                        Ru[i] += Mab * rui;
                        ru[i] = ld_u_free(dm, (int32_t)nb, i) ? rui : 0.0;      // (the column of a Dirichlet component is dropped)
                        Rv[i] += Mab * (w[4 * nb + i] - w0[4 * nb + i]) / dt;
                    }
                    Rp += Mab * (q * il * w[4 * nb + 3] + (1.0 - q) * il * w0[4 * nb + 3]);
                    double Kt[TD][TD], Gb[TD];
                    ld_tangent<TD>(k, a, b, p, mu, Kt);
                    ld_mul_FiT(k, k.g[b], Gb);
#pragma unroll
                    for (int kk = 0; kk < TD; ++kk) {
#pragma unroll
                        for (int i = 0; i < TD; ++i) cv[i] += dt * q * Kt[i][kk] * ru[kk];
                        cp += dt * q * 2.0 * k.J * k.J * Gb[kk] * k.vol * ic * ru[kk];
                    }
                }
                double f[TD], f0[TD];
                ld_force<TD>(k, a, p, mu, f);
                ld_force<TD>(k0, a, p0, mu, f0);
#pragma unroll
                for (int i = 0; i < TD; ++i) Rv[i] += q * f[i] + (1.0 - q) * f0[i] + k.vol * ic * P.body[i];
                Rp += k.vol * ic * (q * (k.J * k.J - 1.0) + (1.0 - q) * (k0.J * k0.J - 1.0));
            }
        }
        // follower loads of the facets around the node
        for (int32_t s = nptr[r]; s < nptr[r + 1]; ++s) {
            const int32_t f = nsrc[s];
            const int4 v4 = reinterpret_cast<const int4*>(cells)[fcell[f]];
            const int32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int i = 0; i < TD; ++i) Rv[i] += fr[(int64_t)TD * f + i];
#pragma unroll
            for (int b = 0; b <= TD; ++b) {
                const int64_t nb = v[b];
#pragma unroll
                for (int kk = 0; kk < TD; ++kk) {
                    if (!ld_u_free(dm, (int32_t)nb, kk)) continue;
                    const double ru = (u[TD * nb + kk] - u0[TD * nb + kk]) / dt - q * w[4 * nb + kk] - (1.0 - q) * w0[4 * nb + kk];
#pragma unroll
                    for (int i = 0; i < TD; ++i) cv[i] += dt * fk[(((int64_t)f * (TD + 1) + b) * TD + i) * TD + kk] * ru;
                }
            }
        }
        const uint8_t m = dm[r];
        double r2 = 0.0;
#pragma unroll
        for (int i = 0; i < TD; ++i) {
            if (!((m >> i) & 1)) r2 += Ru[i] * Ru[i];
            const bool vd = (m >> (3 + i)) & 1;
            if (!vd) r2 += Rv[i] * Rv[i];
            rhs[4 * r + i] = vd ? 0.0 : -Rv[i] + cv[i];
        }
        const bool pd = (m >> 6) & 1;
        if (!pd) r2 += Rp * Rp;
        rhs[4 * r + 3] = pd ? 0.0 : -Rp + cp;
        if (TD == 2) rhs[4 * r + 2] = 0.0;
        rn2[r] = r2;
        // identity rows: Dirichlet v / p unknowns and the dummy slot of triangles
        const int rows = (TD == 2 ? 4 : 0) | (pd ? 8 : 0) | ((m >> 3) & 7);
        if (rows) {
            const int64_t sp0 = slice_ptr[r >> 6];
            const int width = (int)((slice_ptr[(r >> 6) + 1] - sp0) >> 6);
            const int64_t base = sp0 + (r & 63);
            for (int kk = 0; kk < width; ++kk) {
                const int64_t idx = base + (int64_t)kk * FS_SLICE;
                const int32_t col = sell_col[idx];
                if (col < 0) continue;                  // padding (stored as ~row, or a clamped DIA offset): its values stay zero
                const bool diag = col == (int32_t)r;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (!((rows >> i) & 1)) continue;
#pragma unroll
                    for (int j = 0; j < 4; ++j) val[(int64_t)(i * 4 + j) * plane + idx] = (diag && i == j) ? 1.0 : 0.0;
                }
            }
        }
    }
}

// cells with J == 0 or J not finite (partials per workgroup), and the node residuals summed per workgroup
template <int TD>
__global__ void __launch_bounds__(FS_BLOCK) k_ld_cells(int64_t nc, const int32_t* __restrict__ cells, const double* __restrict__ xyz4,
                                                       const double* __restrict__ u, const box_snap bx, int64_t n_rows,
                                                       const double* __restrict__ rn2, double* __restrict__ part_r,
                                                       int64_t* __restrict__ part) {
    int64_t n_bad[1] = {0}, first = INT64_MAX;
    double rs = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += stride) {
        ld_cell<TD> k;
        ld_geometry<TD>(cells, xyz4, c, bx, k);
        ld_kinematics<TD>(u, k);
        if (k.J == 0.0 || !isfinite(k.J)) {
            ++n_bad[0];
            first = c < first ? c : first;
        }
    }
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += stride) rs += rn2[r];
    p1_cell_tally<1, true>(n_bad, first, rs, part, part_r);
}

// one workgroup of FS_BLOCK threads: thread t sums the partials t, t + FS_BLOCK, ... in order, then a tree in LDS - a fixed order
__global__ void __launch_bounds__(FS_BLOCK) k_ld_finish(int nb, const double* __restrict__ part_r, const int64_t* __restrict__ part_n,
                                                        const int64_t* __restrict__ part_first, double* __restrict__ out_r,
                                                        int64_t* __restrict__ out_n) {
    __shared__ double sr[FS_BLOCK];
    __shared__ int64_t sn[FS_BLOCK], sf[FS_BLOCK];
    const int t = threadIdx.x;
    double tr = 0.0;
    int64_t tn = 0, tf = INT64_MAX;
    for (int b = t; b < nb; b += FS_BLOCK) {
        tr += part_r[b];
        tn += part_n[b];
        tf = part_first[b] < tf ? part_first[b] : tf;
    }
    sr[t] = tr; sn[t] = tn; sf[t] = tf;
    __syncthreads();
    for (int h = FS_BLOCK / 2; h > 0; h >>= 1) {
        if (t < h) {
            sr[t] += sr[t + h];
            sn[t] += sn[t + h];
            sf[t] = sf[t + h] < sf[t] ? sf[t + h] : sf[t];
        }
        __syncthreads();
    }
    if (t == 0) {
        out_r[0] = sr[0];
        out_n[0] = sn[0];
        out_n[1] = sf[0];
    }
}

// The facet maps and the Dirichlet mask of the last call: a time loop passes the same facets and mask at every iterate.  Keyed on
// the space's serial number (addresses are recycled after a destroy) and its node count.
struct ld_cache {
    uint64_t serial = 0;
    int64_t nn = -1;
    std::vector<int32_t> fcell, fopp;
    std::vector<uint8_t> mask;
    dbuf<int32_t> d_fcell, d_fopp, ent, eptr, esrc, nptr, nsrc;
    dbuf<uint8_t> d_mask;
    dbuf<double> fg, fr, fk, rn2, part_r, out_r;
    dbuf<int64_t> part, out_n;                  // part: (count, smallest index)[FS_LD_BLOCKS]
    int64_t n_touched = 0;
};

}  // namespace

// ---- host side -----------------------------------------------------------------------------------------------------------
extern "C" int fs_assemble_large_deformation(fs_matrix_t Jr, fs_vector_t rhs, fs_vector_t u, fs_vector_t w, fs_vector_t u0,
                                             fs_vector_t w0, const fs_ld_form* form, fs_ld_info* info) {
    FS_REFUSE_DG(Jr, "fs_assemble_large_deformation");
    FS_REQUIRE(Jr && rhs && u && w && u0 && w0 && form && info, "fs_assemble_large_deformation: null pointer");
    fs_space_s* sp = Jr->space;
    fs_mesh_s* m = sp->mesh;
    const int td = m->tdim;
    FS_REQUIRE(sp->degree == 1 && sp->ncomp == 4 && Jr->bs == 4,
               "fs_assemble_large_deformation: the matrix must live on the CG1 block-4 space (fs_space_create(mesh, CG, 1, 4))");
    FS_REQUIRE(m->n_owned == m->nv && sp->n_nodes_owned == sp->n_nodes_local,
               "fs_assemble_large_deformation: the space has ghost nodes (several ranks): not supported");
    FS_REQUIRE(sp->slots.p, "fs_assemble_large_deformation: space without slot table");
    const int64_t nn = sp->n_nodes_local;
    FS_REQUIRE(u->d.n >= td * nn && u0->d.n >= td * nn, "fs_assemble_large_deformation: displacement vectors need %d x %lld entries", td,
               (long long)nn);
    FS_REQUIRE(w->d.n >= 4 * nn && w0->d.n >= 4 * nn && rhs->d.n >= 4 * nn,
               "fs_assemble_large_deformation: block vectors need 4 x %lld entries", (long long)nn);
    FS_REQUIRE(form->dt > 0.0 && isfinite(form->dt) && form->q >= 0.0 && form->q <= 1.0,
               "fs_assemble_large_deformation: dt > 0 and 0 <= q <= 1 are required (dt = %g, q = %g)", form->dt, form->q);
    FS_REQUIRE(form->mu > 0.0 && form->lambda > 0.0 && isfinite(form->mu) && isfinite(form->lambda),
               "fs_assemble_large_deformation: mu > 0 and lambda > 0 are required (mu = %g, lambda = %g)", form->mu, form->lambda);
    FS_REQUIRE(form->dirichlet, "fs_assemble_large_deformation: the Dirichlet mask is required");
    FS_REQUIRE(form->n_facets == 0 || (form->facet_cell && form->facet_opposite && form->facet_g),
               "fs_assemble_large_deformation: facet arrays missing");
    const int64_t nf = form->n_facets;
    for (int64_t f = 0; f < nf; ++f)
        FS_REQUIRE(form->facet_cell[f] >= 0 && form->facet_cell[f] < m->nc && form->facet_opposite[f] >= 0 && form->facet_opposite[f] <= td,
                   "fs_assemble_large_deformation: facet %lld names cell %d, local vertex %d", (long long)f, form->facet_cell[f],
                   form->facet_opposite[f]);
    hipStream_t s = fs_rt().stream;
    static ld_cache C;
    const int nv_ = td + 1;
    const bool same_space = C.serial == sp->serial && C.nn == nn;
    if (!same_space) {
        C.serial = 0;                    // (set again once every buffer below has been rebuilt for this space)
        C.mask.clear();
        C.fcell.clear();
        C.fopp.clear();
    }
    if (!same_space || C.mask.size() != (size_t)nn || memcmp(C.mask.data(), form->dirichlet, (size_t)nn) != 0) {
        C.mask.assign(form->dirichlet, form->dirichlet + nn);
        FS_CHECK(C.d_mask.alloc(nn));
        FS_CHECK(C.d_mask.upload(C.mask.data(), nn, s));
    }
    const bool same_facets = same_space && C.fcell.size() == (size_t)nf &&
                             std::equal(C.fcell.begin(), C.fcell.end(), form->facet_cell) &&
                             std::equal(C.fopp.begin(), C.fopp.end(), form->facet_opposite);
    if (!same_space) {
        FS_CHECK(C.rn2.alloc(nn));
        FS_CHECK(C.part_r.alloc(FS_LD_BLOCKS));
        FS_CHECK(C.part.alloc(2 * FS_LD_BLOCKS));
        FS_CHECK(C.out_r.alloc(1));
        FS_CHECK(C.out_n.alloc(2));
    }
    if (!same_facets) {
        // sources of every touched stored block (ascending facet, then cell vertex) and of every node (ascending facet)
        C.fcell.assign(form->facet_cell, form->facet_cell + nf);
        C.fopp.assign(form->facet_opposite, form->facet_opposite + nf);
        FS_CHECK(C.d_fcell.alloc(std::max<int64_t>(nf, 1)));
        FS_CHECK(C.d_fopp.alloc(std::max<int64_t>(nf, 1)));
        FS_CHECK(C.d_fcell.upload(C.fcell.data(), nf, s));
        FS_CHECK(C.d_fopp.upload(C.fopp.data(), nf, s));
        FS_CHECK(C.fg.alloc(std::max<int64_t>(3 * nf, 1)));
        FS_CHECK(C.fr.alloc(std::max<int64_t>((int64_t)td * nf, 1)));
        FS_CHECK(C.fk.alloc(std::max<int64_t>((int64_t)nv_ * td * td * nf, 1)));
        std::vector<int32_t> ek((size_t)nf * td * nv_), nk((size_t)nf * td);
        if (nf) {
            dbuf<int32_t> d_ek, d_nk;
            FS_CHECK(d_ek.alloc((int64_t)ek.size()));
            FS_CHECK(d_nk.alloc((int64_t)nk.size()));
            if (td == 3)
                hipLaunchKernelGGL(k_ld_facet_keys<3>, dim3(fs_grid_for(nf)), dim3(FS_BLOCK), 0, s, nf, m->nc, C.d_fcell.p, C.d_fopp.p, m->cells.p, sp->slots.p, d_ek.p, d_nk.p);
            else
                hipLaunchKernelGGL(k_ld_facet_keys<2>, dim3(fs_grid_for(nf)), dim3(FS_BLOCK), 0, s, nf, m->nc, C.d_fcell.p, C.d_fopp.p, m->cells.p, sp->slots.p, d_ek.p, d_nk.p);
            FS_KERNEL_CHECK();
            FS_CHECK(d_ek.download(ek.data(), (int64_t)ek.size(), s));
            FS_CHECK(d_nk.download(nk.data(), (int64_t)nk.size(), s));
        }
        // stored blocks: sources f * (TD + 1) + b, in ascending (entry, facet, b)
        std::vector<int64_t> order(ek.size());
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return ek[x] < ek[y]; });
        std::vector<int32_t> ent, eptr, esrc;
        for (size_t i = 0; i < order.size(); ++i) {
            const int64_t o = order[i];
            FS_REQUIRE(ek[o] >= 0 && ek[o] < sp->sell_entries, "fs_assemble_large_deformation: internal error, facet block outside the pattern");
            if (ent.empty() || ent.back() != ek[o]) { ent.push_back(ek[o]); eptr.push_back((int32_t)i); }
            const int64_t f = o / (td * nv_), b = o % nv_;
            esrc.push_back((int32_t)(f * nv_ + b));
        }
        eptr.push_back((int32_t)order.size());
        C.n_touched = (int64_t)ent.size();
        // nodes: a dense pointer over all nodes
        std::vector<int32_t> cnt(nn + 1, 0), nsrc(nk.size());
        for (size_t i = 0; i < nk.size(); ++i) ++cnt[nk[i] + 1];
        for (int64_t r = 0; r < nn; ++r) cnt[r + 1] += cnt[r];
        std::vector<int32_t> fill(cnt.begin(), cnt.end() - 1);
        for (size_t i = 0; i < nk.size(); ++i) nsrc[fill[nk[i]]++] = (int32_t)(i / td);       // ascending facet within a node
        FS_CHECK(C.ent.alloc(std::max<int64_t>(C.n_touched, 1)));
        FS_CHECK(C.eptr.alloc((int64_t)eptr.size()));
        FS_CHECK(C.esrc.alloc(std::max<int64_t>((int64_t)esrc.size(), 1)));
        FS_CHECK(C.nptr.alloc(nn + 1));
        FS_CHECK(C.nsrc.alloc(std::max<int64_t>((int64_t)nsrc.size(), 1)));
        FS_CHECK(C.ent.upload(ent.data(), C.n_touched, s));
        FS_CHECK(C.eptr.upload(eptr.data(), (int64_t)eptr.size(), s));
        FS_CHECK(C.esrc.upload(esrc.data(), (int64_t)esrc.size(), s));
        FS_CHECK(C.nptr.upload(cnt.data(), nn + 1, s));
        FS_CHECK(C.nsrc.upload(nsrc.data(), (int64_t)nsrc.size(), s));
        FS_HIP(hipStreamSynchronize(s));
    }
    C.serial = sp->serial;
    C.nn = nn;
    if (nf) {
        std::vector<double> g3((size_t)3 * nf, 0.0);
        for (int64_t f = 0; f < nf; ++f)
            for (int i = 0; i < td; ++i) g3[3 * f + i] = form->facet_g[3 * f + i];
        FS_CHECK(C.fg.upload(g3.data(), 3 * nf, s));
    }
    const box_snap bx = make_box_snap(m);
    ld_params P;
    P.dt = form->dt; P.q = form->q; P.mu = form->mu; P.lambda = form->lambda;
    for (int i = 0; i < 3; ++i) P.body[i] = form->body_force[i];
    const int64_t plane = sp->sell_entries;
    const int gf = fs_grid_for(std::max<int64_t>(nf, 1));
    int rc = FS_OK;
    fs_dispatch_int<3, 2>(td, [&](auto TD) {          // (the space is one rank's: nn = n_nodes_owned, the node launch's count)
        constexpr int d = decltype(TD)::value;
        rc = p1_launch_blocks(sp, s, k_ld_jacobian<d>, u->d.p, w->d.p, C.d_mask.p, P, bx, plane, Jr->val.p);
        if (rc != FS_OK) return;
        if (nf) {
            hipLaunchKernelGGL(k_ld_facets<d>, dim3(gf), dim3(FS_BLOCK), 0, s, nf, C.d_fcell.p, C.d_fopp.p, C.fg.p, m->cells.p, m->xyz.p,
                               u->d.p, bx, C.fr.p, C.fk.p);
            hipLaunchKernelGGL(k_ld_facet_entries<d>, dim3(fs_grid_for(C.n_touched)), dim3(FS_BLOCK), 0, s, C.n_touched, C.ent.p, C.eptr.p,
                               C.esrc.p, C.d_fcell.p, m->cells.p, C.fk.p, C.d_mask.p, P.dt * P.q, plane, Jr->val.p);
        }
        rc = p1_launch_nodes(sp, s, k_ld_nodes<d>, u->d.p, w->d.p, u0->d.p, w0->d.p, C.d_mask.p, P, bx, C.nptr.p, C.nsrc.p, C.d_fcell.p, C.fr.p,
                             C.fk.p, plane, Jr->val.p, rhs->d.p, C.rn2.p);
        if (rc != FS_OK) return;
        hipLaunchKernelGGL(k_ld_cells<d>, dim3(FS_LD_BLOCKS), dim3(FS_BLOCK), 0, s, m->nc, m->cells.p, m->xyz.p, u->d.p, bx, nn, C.rn2.p,
                           C.part_r.p, C.part.p);
    });
    FS_CHECK(rc);
    FS_KERNEL_CHECK();
    hipLaunchKernelGGL(k_ld_finish, dim3(1), dim3(FS_BLOCK), 0, s, FS_LD_BLOCKS, C.part_r.p, C.part.p, C.part.p + FS_LD_BLOCKS, C.out_r.p,
                       C.out_n.p);
    FS_KERNEL_CHECK();
    double r2 = 0.0;
    int64_t nb[2] = {0, 0};
    FS_CHECK(C.out_r.download(&r2, 1, s));
    FS_CHECK(C.out_n.download(nb, 2, s));
    FS_HIP(hipStreamSynchronize(s));
    info->residual_norm = sqrt(r2);
    info->n_bad = nb[0];
    info->first_bad_cell = fs_first_cell(m, nb[0], nb[1]);
    return FS_OK;
}
