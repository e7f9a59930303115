// Taylor-Hood Navier-Stokes for libfsamd.so (gfx950): assembly of the linearised coupled system and its
// Krylov solve.  Replaces what CoupledNavierStokesSolver hands to DOLFIN/PETSc
// (FenicsSolver/CoupledNavierStokesSolver.py:288-381 forms, :215-245 action/derivative, :492-528 solve,
// SolverBase.py:615-626 NonlinearVariationalSolver):
//   J(w0) w = g(w0)   with   J = 2 nu eps(u):eps(v) + (1/dt) u.v + (grad(u) u0).v [+ (grad(u0) u).v]
//                                 - (p/rho) div v + (q/rho) div u
//                            g = f.v + (1/dt) u_prev.v [+ (grad(u0) u0).v]
// (the Newton step written for the new iterate, so Dirichlet values are applied directly).
//
// Layout: one block of 4 unknowns per P2 node (u_x, u_y, u_z, p), the matrix is a bs = 4 matrix on the CG2
// node pattern (hybrid SELL/DIA like every other operator, so the tuned SpMV applies).  The pressure is P1:
// only vertex nodes carry a pressure; the pressure slot of an edge node is a dummy unknown with a unit row.
//
// Assembly: one thread per (cell, test node a, trial node b): 14-point degree-5 rule (exact for the
// P2*P2*P1 convection integrand), the 4x4 block accumulated in registers, fp64 hardware atomics into the
// 16 value planes through the slot table.  Solve: restarted FGMRES, right preconditioner
//   [A 0; D S]^-1  with  A^-1 ~ Jacobi sweeps,  S^-1 ~ rho^2 ( (1/dt) K_p^-1 + nu M_p^-1 )  (Cahouet-Chabard),
// K_p, M_p = P1 pressure Laplacian / mass matrix solved by the library's own CG.
//
// This file is the assembly; the solve is fs_saddle_solve.inc, included at the end (one translation unit, one code object).
#include "fs_kernels.h"
#include <hipcub/hipcub.hpp>
#include <chrono>
#include <stdlib.h>
#include <cmath>
#include <vector>

// barycentric points / weights (sum 1) of the 14-point degree-5 rule
__device__ const double NS_QP[14][4] = {
    {0.0673422422100982, 0.3108859192633006, 0.3108859192633006, 0.3108859192633006},
    {0.3108859192633006, 0.0673422422100982, 0.3108859192633006, 0.3108859192633006},
    {0.3108859192633006, 0.3108859192633006, 0.0673422422100982, 0.3108859192633006},
    {0.3108859192633006, 0.3108859192633006, 0.3108859192633006, 0.0673422422100982},
    {0.7217942490673264, 0.0927352503108912, 0.0927352503108912, 0.0927352503108912},
    {0.0927352503108912, 0.7217942490673264, 0.0927352503108912, 0.0927352503108912},
    {0.0927352503108912, 0.0927352503108912, 0.7217942490673264, 0.0927352503108912},
    {0.0927352503108912, 0.0927352503108912, 0.0927352503108912, 0.7217942490673264},
    {0.0455037041256496, 0.0455037041256496, 0.4544962958743504, 0.4544962958743504},
    {0.0455037041256496, 0.4544962958743504, 0.0455037041256496, 0.4544962958743504},
    {0.0455037041256496, 0.4544962958743504, 0.4544962958743504, 0.0455037041256496},
    {0.4544962958743504, 0.0455037041256496, 0.0455037041256496, 0.4544962958743504},
    {0.4544962958743504, 0.0455037041256496, 0.4544962958743504, 0.0455037041256496},
    {0.4544962958743504, 0.4544962958743504, 0.0455037041256496, 0.0455037041256496}};
__device__ const double NS_QW[14] = {
    0.1126879257180159, 0.1126879257180159, 0.1126879257180159, 0.1126879257180159,
    0.0734930431163620, 0.0734930431163620, 0.0734930431163620, 0.0734930431163620,
    0.0425460207770815, 0.0425460207770815, 0.0425460207770815, 0.0425460207770815, 0.0425460207770815, 0.0425460207770815};
// UFC edge -> vertex pairs of the P2 edge nodes 4..9: e0=(2,3) e1=(1,3) e2=(1,2) e3=(0,3) e4=(0,2) e5=(0,1)
__device__ const int NS_EI[6] = {2, 1, 1, 0, 0, 0};
__device__ const int NS_EJ[6] = {3, 3, 2, 3, 2, 1};

__device__ __forceinline__ double sel4(int i, double a, double b, double c, double d) {
    return i == 0 ? a : (i == 1 ? b : (i == 2 ? c : d));
}

// value and physical gradient of P2 basis function n (runtime index) at barycentric point l
__device__ __forceinline__ void p2_eval(int n, const double l[4], const double gl[4][3], double* phi, double g[3]) {
    if (n < 4) {
        const double li = sel4(n, l[0], l[1], l[2], l[3]);
        const double d = 4.0 * li - 1.0;
        *phi = li * (2.0 * li - 1.0);
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = d * sel4(n, gl[0][k], gl[1][k], gl[2][k], gl[3][k]);
    } else {
        const int i = NS_EI[n - 4], j = NS_EJ[n - 4];
        const double li = sel4(i, l[0], l[1], l[2], l[3]), lj = sel4(j, l[0], l[1], l[2], l[3]);
        *phi = 4.0 * li * lj;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            g[k] = 4.0 * (li * sel4(j, gl[0][k], gl[1][k], gl[2][k], gl[3][k]) + lj * sel4(i, gl[0][k], gl[1][k], gl[2][k], gl[3][k]));
    }
}

struct ns_params {
    double nu, inv_rho, inv_dt;
    double f[3];
    double wm[3];      // ALE: the frame (mesh) velocity, subtracted from the ADVECTING velocity only (:321-329)
    int convection, newton;
    int g2;            // G2 streamline term (:334-363): 0 off, 1 delta1 = kappa1 h^2 (Re <= 1), 2 delta1 from |a|, h (and dt)
    double g2_kappa;
    fs_visc_dev V;     // non-Newtonian law (:194-213) evaluated at every quadrature point on the state w0 (fs_common.h); kind 0: off
};

// h = 2 * circumradius of the tetrahedron X (UFL's 2*Circumradius(mesh), :343):
// R = sqrt((aA+bB+cC)(aA+bB-cC)(aA-bB+cC)(-aA+bB+cC)) / (24 V), (a,A) (b,B) (c,C) the opposite edge pairs
__device__ __forceinline__ double ns_cell_h(const double (&X)[4][3], double vol) {
    auto dist = [&](int p, int q) {
        const double dx = X[p][0] - X[q][0], dy = X[p][1] - X[q][1], dz = X[p][2] - X[q][2];
        return sqrt(dx * dx + dy * dy + dz * dz);
    };
    const double aA = dist(0, 1) * dist(2, 3), bB = dist(0, 2) * dist(1, 3), cC = dist(0, 3) * dist(1, 2);
    const double prod = (aA + bB + cC) * (aA + bB - cC) * (aA - bB + cC) * (-aA + bB + cC);
    return 2.0 * sqrt(prod > 0.0 ? prod : 0.0) / (24.0 * vol);
}
// delta1 of the reference's G2 term at a point with advecting velocity a (|a|^2 = U2): kappa1 h^2 for Re <= 1, otherwise
// kappa1/2 * h/|a| (steady) or kappa1/2 / sqrt(1/dt^2 + 1/(|a|^2 h^2)) (transient, as the reference writes it).  The
// term delta1 (a.grad u)(a.grad v) vanishes with |a|: delta1 = 0 where a = 0 (UFL would divide by zero there).
__device__ __forceinline__ double ns_g2_delta(const ns_params& P, double h, double U2) {
    if (P.g2 == 1) return P.g2_kappa * h * h;
    if (U2 <= 0.0) return 0.0;
    if (P.inv_dt != 0.0) return 0.5 * P.g2_kappa / sqrt(P.inv_dt * P.inv_dt + 1.0 / (U2 * h * h));
    return 0.5 * P.g2_kappa * h / sqrt(U2);
}

// thread t = ab*nc + c : block (a, b) of cell c.  val planes [(i*4+j)*plane + slot], g [node*4 + i]
__global__ void __launch_bounds__(FS_BLOCK) k_assemble_ns(const double* __restrict__ xyz, const int32_t* __restrict__ cells,
                                                          const int32_t* __restrict__ cell_dofs,
                                                          int64_t nc, const int32_t* __restrict__ slots,
                                                          const double* __restrict__ w0, const double* __restrict__ wprev,
                                                          ns_params P, double* __restrict__ val, int64_t plane,
                                                          double* __restrict__ g) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; t < nc * 100; t += stride) {
        const int ab = (int)(t / nc);
        const int64_t c = t - (int64_t)ab * nc;
        const int a = ab / 10, b = ab - a * 10;
        const int32_t slot = slots[t];
        if (slot < 0) continue;   // row not owned (single GPU: never)
        int32_t nd[10];
#pragma unroll
        for (int n = 0; n < 10; ++n) nd[n] = cell_dofs[c * 10 + n];
        // geometry: gradients of the barycentric coordinates (vertex ids: node ids differ once ghosts exist)
        double X[4][3];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int64_t vx = cells[c * 4 + v];
            const double2 p01 = reinterpret_cast<const double2*>(xyz)[2 * vx];
            X[v][0] = p01.x; X[v][1] = p01.y; X[v][2] = xyz[4 * vx + 2];
        }
        const double e1[3] = {X[1][0] - X[0][0], X[1][1] - X[0][1], X[1][2] - X[0][2]};
        const double e2[3] = {X[2][0] - X[0][0], X[2][1] - X[0][1], X[2][2] - X[0][2]};
        const double e3[3] = {X[3][0] - X[0][0], X[3][1] - X[0][1], X[3][2] - X[0][2]};
        const double c23[3] = {e2[1] * e3[2] - e2[2] * e3[1], e2[2] * e3[0] - e2[0] * e3[2], e2[0] * e3[1] - e2[1] * e3[0]};
        const double c31[3] = {e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]};
        const double c12[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double det = e1[0] * c23[0] + e1[1] * c23[1] + e1[2] * c23[2];
        const double idet = 1.0 / det;
        double gl[4][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            gl[1][k] = c23[k] * idet;
            gl[2][k] = c31[k] * idet;
            gl[3][k] = c12[k] * idet;
            gl[0][k] = -(gl[1][k] + gl[2][k] + gl[3][k]);
        }
        const double vol = fabs(det) * (1.0 / 6.0);
        const double hcell = P.g2 ? ns_cell_h(X, vol) : 0.0;
        // state at the cell nodes
        double U0[10][3];
        if (P.convection) {
#pragma unroll
            for (int n = 0; n < 10; ++n) {
                const double2 u01 = reinterpret_cast<const double2*>(w0)[2 * (int64_t)nd[n]];
                U0[n][0] = u01.x; U0[n][1] = u01.y; U0[n][2] = w0[4 * (int64_t)nd[n] + 2];
            }
        }
        double blk[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) blk[i][j] = 0.0;
        double gv[3] = {0.0, 0.0, 0.0};
        const bool do_rhs = b == 0;
        double P0[4] = {0.0, 0.0, 0.0, 0.0}, T0[4] = {0.0, 0.0, 0.0, 0.0};
        if (P.V.kind) {
#pragma unroll
            for (int v = 0; v < 4; ++v) P0[v] = w0[4 * (int64_t)nd[v] + 3];
            if (P.V.kind == 2)
#pragma unroll
                for (int v = 0; v < 4; ++v) T0[v] = P.V.T[nd[v]];
        }
        for (int q = 0; q < 14; ++q) {
            const double l[4] = {NS_QP[q][0], NS_QP[q][1], NS_QP[q][2], NS_QP[q][3]};
            const double wv = NS_QW[q] * vol;
            const double nuq = fs_viscosity(P.V, P.nu, l[0] * P0[0] + l[1] * P0[1] + l[2] * P0[2] + l[3] * P0[3],
                                            l[0] * T0[0] + l[1] * T0[1] + l[2] * T0[2] + l[3] * T0[3]);
            double pa, pb, ga[3], gb[3];
            p2_eval(a, l, gl, &pa, ga);
            p2_eval(b, l, gl, &pb, gb);
            const double gg = ga[0] * gb[0] + ga[1] * gb[1] + ga[2] * gb[2];
            double diag = nuq * gg + P.inv_dt * pa * pb;
            double u0[3] = {0.0, 0.0, 0.0}, gu0[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
            if (P.convection) {
#pragma unroll
                for (int n = 0; n < 10; ++n) {
                    double pn, gn[3];
                    p2_eval(n, l, gl, &pn, gn);      // n is a compile-time constant here: the selects fold away
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        u0[i] += pn * U0[n][i];
#pragma unroll
                        for (int j = 0; j < 3; ++j) gu0[i][j] += U0[n][i] * gn[j];
                    }
                }
                const double av[3] = {u0[0] - P.wm[0], u0[1] - P.wm[1], u0[2] - P.wm[2]};
                const double agb = av[0] * gb[0] + av[1] * gb[1] + av[2] * gb[2];
                diag += pa * agb;
                if (P.g2) {      // F -= delta1 (a.grad u).(a.grad v) dx, the sign as the reference has it (:360-362)
                    const double aga = av[0] * ga[0] + av[1] * ga[1] + av[2] * ga[2];
                    diag -= ns_g2_delta(P, hcell, av[0] * av[0] + av[1] * av[1] + av[2] * av[2]) * aga * agb;
                }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                blk[i][i] += wv * diag;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    double v = nuq * ga[j] * gb[i];
                    if (P.convection && P.newton) v += pa * pb * gu0[i][j];
                    blk[i][j] += wv * v;
                }
            }
            if (b < 4) {   // pressure trial function psi_b = lambda_b
                const double psi = sel4(b, l[0], l[1], l[2], l[3]);
#pragma unroll
                for (int i = 0; i < 3; ++i) blk[i][3] -= wv * P.inv_rho * psi * ga[i];
            }
            if (a < 4) {   // continuity test function psi_a
                const double psi = sel4(a, l[0], l[1], l[2], l[3]);
#pragma unroll
                for (int j = 0; j < 3; ++j) blk[3][j] += wv * P.inv_rho * psi * gb[j];
            }
            if (do_rhs) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    double v = P.f[i];
                    if (P.convection && P.newton) v += gu0[i][0] * u0[0] + gu0[i][1] * u0[1] + gu0[i][2] * u0[2];
                    gv[i] += wv * pa * v;
                }
                if (wprev && P.inv_dt != 0.0) {
                    double up[3] = {0.0, 0.0, 0.0};
#pragma unroll
                    for (int n = 0; n < 10; ++n) {
                        double pn, gn[3];
                        p2_eval(n, l, gl, &pn, gn);
#pragma unroll
                        for (int i = 0; i < 3; ++i) up[i] += pn * wprev[4 * (int64_t)nd[n] + i];
                    }
#pragma unroll
                    for (int i = 0; i < 3; ++i) gv[i] += wv * P.inv_dt * pa * up[i];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i == 3 && j == 3) continue;
                if (j == 3 && b >= 4) continue;
                if (i == 3 && a >= 4) continue;
                atomicAdd(&val[(int64_t)(i * 4 + j) * plane + slot], blk[i][j]);
            }
        if (do_rhs) {
#pragma unroll
            for (int i = 0; i < 3; ++i) atomicAdd(&g[4 * (int64_t)nd[a] + i], gv[i]);
        }
    }
}

// ---- the same element, one wave per cell ---------------------------------------------------------------------------
// The kernel above (one thread per (cell, a, b), ordered pair-major; FS_NS_ASSEMBLE=pair) recomputes the state at the
// 14 points in each of the 100 threads of a cell.  Here a wave owns a cell: basis functions and state at the quadrature
// points are built once in LDS, lane ab accumulates block (a, b), and all atomics of a cell - and of its neighbours in
// the cell order, which share its rows - are issued together.  Measured on MI355X (configs[4], 477 042 cells): 24.7 ms
// against 22.4 ms for the pair-major kernel - neither the redundant flops nor the locality of the lines is the
// limit, the 544 M device-scope fp64 atomics are (22 G/s: they are resolved behind the per-XCD L2s).  The next
// step is an owner-computes gather (one wave per matrix row, no atomics), as the P1 scalar path already does.
// Occupancy: 4 waves per SIMD (127 VGPRs, 20 B of scratch) 5.9 ms; the compiler's own choice 3 waves (137 VGPRs) 6.9 ms;
// 5 waves (96 VGPRs, 132 B of scratch) 7.2 ms - configs[4], 477 042 cells.
#define NS_WPB (FS_BLOCK / 64)
struct ns_cell_lds {
    double phi[14][10];
    double gphi[14][10][3];
    double u0[14][3];
    double gu0[14][9];
    double up[14][3];
    double U0[10][3];
    double UP[10][3];
    double nuq[14];
    double P0[4], T0[4];
    int32_t nd[10];
    int32_t pad[2];
};
__global__ void __launch_bounds__(FS_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) k_assemble_ns_wave(const double* __restrict__ xyz, const int32_t* __restrict__ cells,
                                                               const int32_t* __restrict__ cell_dofs,
                                                               int64_t nc, int64_t n_rows, const int32_t* __restrict__ slots,
                                                               const double* __restrict__ w0, const double* __restrict__ wprev,
                                                               ns_params P, double* __restrict__ val, int64_t plane,
                                                               double* __restrict__ ebuf, double* __restrict__ g) {
    __shared__ ns_cell_lds S[NS_WPB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    ns_cell_lds& L = S[wave];
    const bool has_prev = wprev != nullptr && P.inv_dt != 0.0;
    for (int64_t cbase = (int64_t)blockIdx.x * NS_WPB; cbase < nc; cbase += (int64_t)gridDim.x * NS_WPB) {
        const int64_t c = cbase + wave;
        const bool act = c < nc;
        double gl[4][3], vol = 0.0, hcell = 0.0;
        if (act) {
            // node ids and nodal state -> LDS; geometry in registers (every lane, broadcast loads)
            if (lane < 10) L.nd[lane] = cell_dofs[c * 10 + lane];
            if (lane < 30) {
                const int n = lane / 3, i = lane - 3 * n;
                const int64_t node = cell_dofs[c * 10 + n];
                L.U0[n][i] = P.convection ? w0[4 * node + i] : 0.0;
                L.UP[n][i] = has_prev ? wprev[4 * node + i] : 0.0;
            } else if (lane < 34) {
                L.P0[lane - 30] = P.V.kind ? w0[4 * (int64_t)cell_dofs[c * 10 + (lane - 30)] + 3] : 0.0;
            } else if (lane < 38) {
                L.T0[lane - 34] = P.V.kind == 2 ? P.V.T[cell_dofs[c * 10 + (lane - 34)]] : 0.0;
            }
            double X[4][3];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t vx = cells[c * 4 + v];          // vertex ids: node ids differ once ghosts exist
                const double2 p01 = reinterpret_cast<const double2*>(xyz)[2 * vx];
                X[v][0] = p01.x; X[v][1] = p01.y; X[v][2] = xyz[4 * vx + 2];
            }
            const double e1[3] = {X[1][0] - X[0][0], X[1][1] - X[0][1], X[1][2] - X[0][2]};
            const double e2[3] = {X[2][0] - X[0][0], X[2][1] - X[0][1], X[2][2] - X[0][2]};
            const double e3[3] = {X[3][0] - X[0][0], X[3][1] - X[0][1], X[3][2] - X[0][2]};
            const double c23[3] = {e2[1] * e3[2] - e2[2] * e3[1], e2[2] * e3[0] - e2[0] * e3[2], e2[0] * e3[1] - e2[1] * e3[0]};
            const double c31[3] = {e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]};
            const double c12[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            const double det = e1[0] * c23[0] + e1[1] * c23[1] + e1[2] * c23[2];
            const double idet = 1.0 / det;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                gl[1][k] = c23[k] * idet;
                gl[2][k] = c31[k] * idet;
                gl[3][k] = c12[k] * idet;
                gl[0][k] = -(gl[1][k] + gl[2][k] + gl[3][k]);
            }
            vol = fabs(det) * (1.0 / 6.0);
            if (P.g2) hcell = ns_cell_h(X, vol);
            // basis functions and gradients at the 14 points
            for (int item = lane; item < 140; item += 64) {
                const int q = item / 10, n = item - 10 * q;
                const double l[4] = {NS_QP[q][0], NS_QP[q][1], NS_QP[q][2], NS_QP[q][3]};
                double pn, gn[3];
                p2_eval(n, l, gl, &pn, gn);
                L.phi[q][n] = pn;
                L.gphi[q][n][0] = gn[0]; L.gphi[q][n][1] = gn[1]; L.gphi[q][n][2] = gn[2];
            }
        }
        __syncthreads();
        if (act) {
            // state, its gradient and the previous velocity at the 14 points
            if (lane < 14)
                L.nuq[lane] = fs_viscosity(P.V, P.nu, NS_QP[lane][0] * L.P0[0] + NS_QP[lane][1] * L.P0[1] + NS_QP[lane][2] * L.P0[2] + NS_QP[lane][3] * L.P0[3],
                                           NS_QP[lane][0] * L.T0[0] + NS_QP[lane][1] * L.T0[1] + NS_QP[lane][2] * L.T0[2] + NS_QP[lane][3] * L.T0[3]);
            for (int item = lane; item < 210; item += 64) {
                double acc = 0.0;
                if (item < 42) {
                    const int q = item / 3, i = item - 3 * q;
#pragma unroll
                    for (int n = 0; n < 10; ++n) acc += L.phi[q][n] * L.U0[n][i];
                    L.u0[q][i] = acc;
                } else if (item < 168) {
                    const int it = item - 42, q = it / 9, ij = it - 9 * q, i = ij / 3, j = ij - 3 * i;
#pragma unroll
                    for (int n = 0; n < 10; ++n) acc += L.U0[n][i] * L.gphi[q][n][j];
                    L.gu0[q][ij] = acc;
                } else {
                    const int it = item - 168, q = it / 3, i = it - 3 * q;
#pragma unroll
                    for (int n = 0; n < 10; ++n) acc += L.phi[q][n] * L.UP[n][i];
                    L.up[q][i] = acc;
                }
            }
        }
        __syncthreads();
        if (act) {
            for (int ab = lane; ab < 100; ab += 64) {
                const int a = ab / 10, b = ab - 10 * a;
                // two-pass mode needs no slot: blocks of rows this rank does not own are simply never gathered
                const int32_t slot = ebuf ? 0 : slots[(int64_t)ab * nc + c];
                if (slot < 0) continue;   // row not owned
                double blk[4][4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) blk[i][j] = 0.0;
                double gv[3] = {0.0, 0.0, 0.0};
                const bool do_rhs = b == 0;
                const int bsel = b < 4 ? b : 0, asel = a < 4 ? a : 0;
                const double bmask = b < 4 ? 1.0 : 0.0, amask = a < 4 ? 1.0 : 0.0;
                for (int q = 0; q < 14; ++q) {
                    const double wv = NS_QW[q] * vol;
                    const double pa = L.phi[q][a], pb = L.phi[q][b];
                    const double ga[3] = {L.gphi[q][a][0], L.gphi[q][a][1], L.gphi[q][a][2]};
                    const double gb[3] = {L.gphi[q][b][0], L.gphi[q][b][1], L.gphi[q][b][2]};
                    const double u0[3] = {L.u0[q][0], L.u0[q][1], L.u0[q][2]};
                    const double nuq = L.nuq[q];
                    double diag = nuq * (ga[0] * gb[0] + ga[1] * gb[1] + ga[2] * gb[2]) + P.inv_dt * pa * pb;
                    if (P.convection) {
                        const double av[3] = {u0[0] - P.wm[0], u0[1] - P.wm[1], u0[2] - P.wm[2]};
                        const double agb = av[0] * gb[0] + av[1] * gb[1] + av[2] * gb[2];
                        diag += pa * agb;
                        if (P.g2) {
                            const double aga = av[0] * ga[0] + av[1] * ga[1] + av[2] * ga[2];
                            diag -= ns_g2_delta(P, hcell, av[0] * av[0] + av[1] * av[1] + av[2] * av[2]) * aga * agb;
                        }
                    }
                    const bool full = P.convection && P.newton;
                    // (the kernel is instruction-bound - counters in DESIGN.md section 3 -: the weight goes into the factors once,
                    // the nine viscous terms are 3 + 9 operations instead of 27, the Newton term 2 + 9)
                    const double wd = wv * diag, wn = wv * nuq;
                    const double wga[3] = {wn * ga[0], wn * ga[1], wn * ga[2]};
                    const double wpp = full ? wv * pa * pb : 0.0;
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        blk[i][i] += wd;
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            blk[i][j] = fma(wga[j], gb[i], blk[i][j]);
                            if (full) blk[i][j] = fma(wpp, L.gu0[q][3 * i + j], blk[i][j]);
                        }
                    }
                    // pressure trial function psi_b = lambda_b (b < 4) and continuity test function psi_a (a < 4): branch-free (a
                    // zero factor for the edge nodes) - every lane-divergent branch inside this loop is an exec-mask sequence of
                    // scalar instructions, 14 times per block
                    const double wr = wv * P.inv_rho;
                    const double wpb = wr * (NS_QP[q][bsel] * bmask), wpa = wr * (NS_QP[q][asel] * amask);
#pragma unroll
                    for (int i = 0; i < 3; ++i) blk[i][3] = fma(-wpb, ga[i], blk[i][3]);
#pragma unroll
                    for (int j = 0; j < 3; ++j) blk[3][j] = fma(wpa, gb[j], blk[3][j]);
                    if (do_rhs) {
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            double v = P.f[i];
                            if (full) v += L.gu0[q][3 * i] * u0[0] + L.gu0[q][3 * i + 1] * u0[1] + L.gu0[q][3 * i + 2] * u0[2];
                            if (has_prev) v += P.inv_dt * L.up[q][i];
                            gv[i] += wv * pa * v;
                        }
                    }
                }
                if (ebuf) {      // element block -> buffer (128 B per lane, contiguous over the wave); summed by k_ns_gather
                    double2* __restrict__ out = reinterpret_cast<double2*>(ebuf + ((int64_t)c * 100 + ab) * 16);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        out[2 * i] = make_double2(blk[i][0], blk[i][1]);
                        out[2 * i + 1] = make_double2(blk[i][2], blk[i][3]);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            if (i == 3 && j == 3) continue;
                            if (j == 3 && b >= 4) continue;
                            if (i == 3 && a >= 4) continue;
                            atomicAdd(&val[(int64_t)(i * 4 + j) * plane + slot], blk[i][j]);
                        }
                }
                if (do_rhs) {
                    const int64_t node = L.nd[a];
                    if (node < n_rows) {      // owned row
#pragma unroll
                        for (int i = 0; i < 3; ++i) atomicAdd(&g[4 * node + i], gv[i]);
                    }
                }
            }
        }
        __syncthreads();
    }
}


// ---- Taylor-Hood on TRIANGLES (the reference's own CFD example is 2-D: examples/test_cfd_solver.py:83) -------------------
// The class is dimension-free upstream (CoupledNavierStokesSolver.py:84-102, 288-381).  Here the 2-D system keeps the block-4
// layout: (u_x, u_y, -, p) per CG2 node with the third slot a dummy unknown (unit row, zero coupling), so the operator product,
// the block preconditioner and FGMRES above serve it unchanged; a 2-D mesh is small, the unused planes cost nothing that matters.
// Element: 6 P2 nodes (3 vertices, then the UFC edges e0=(1,2) e1=(0,2) e2=(0,1)), Radon's 7-point degree-5 rule (exact for
// the P2*P2*P1 convection integrand), one thread per (cell, a, b); the 4x4 element block goes to the element buffer and the
// stored blocks are summed by k_ns_gather in a fixed order (no atomics on the matrix).
__device__ const double NS_TRI_QP[7][3] = {
    {1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0},
    {0.797426985353087, 0.101286507323456, 0.101286507323456},
    {0.101286507323456, 0.797426985353087, 0.101286507323456},
    {0.101286507323456, 0.101286507323456, 0.797426985353087},
    {0.059715871789770, 0.470142064105115, 0.470142064105115},
    {0.470142064105115, 0.059715871789770, 0.470142064105115},
    {0.470142064105115, 0.470142064105115, 0.059715871789770}};
__device__ const double NS_TRI_QW[7] = {0.225, 0.125939180544827, 0.125939180544827, 0.125939180544827,
                                        0.132394152788506, 0.132394152788506, 0.132394152788506};
__device__ const int NS_TRI_EI[3] = {1, 0, 0};
__device__ const int NS_TRI_EJ[3] = {2, 2, 1};

__device__ __forceinline__ double sel3(int i, double a, double b, double c) { return i == 0 ? a : (i == 1 ? b : c); }

// value and physical gradient of P2 basis function n of a triangle at barycentric point l
__device__ __forceinline__ void p2tri_eval(int n, const double l[3], const double gl[3][2], double* phi, double g[2]) {
    if (n < 3) {
        const double li = sel3(n, l[0], l[1], l[2]);
        const double d = 4.0 * li - 1.0;
        *phi = li * (2.0 * li - 1.0);
        g[0] = d * sel3(n, gl[0][0], gl[1][0], gl[2][0]);
        g[1] = d * sel3(n, gl[0][1], gl[1][1], gl[2][1]);
    } else {
        const int i = NS_TRI_EI[n - 3], j = NS_TRI_EJ[n - 3];
        const double li = sel3(i, l[0], l[1], l[2]), lj = sel3(j, l[0], l[1], l[2]);
        *phi = 4.0 * li * lj;
        g[0] = 4.0 * (li * sel3(j, gl[0][0], gl[1][0], gl[2][0]) + lj * sel3(i, gl[0][0], gl[1][0], gl[2][0]));
        g[1] = 4.0 * (li * sel3(j, gl[0][1], gl[1][1], gl[2][1]) + lj * sel3(i, gl[0][1], gl[1][1], gl[2][1]));
    }
}

// gradients of the barycentric coordinates of triangle c, its area and (G2) h = 2 * circumradius = |e0||e1||e2| / (2 area)
__device__ __forceinline__ void ns_tri_geometry(const double* __restrict__ xyz, const int32_t* __restrict__ cells, int64_t c,
                                                double gl[3][2], double* area, double* hcell) {
    double X[3][2];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const int64_t vx = cells[c * 4 + v];
        X[v][0] = xyz[4 * vx]; X[v][1] = xyz[4 * vx + 1];
    }
    const double ax = X[1][0] - X[0][0], ay = X[1][1] - X[0][1], bx = X[2][0] - X[0][0], by = X[2][1] - X[0][1];
    const double det = ax * by - bx * ay;
    const double idet = 1.0 / det;
    gl[1][0] = by * idet;  gl[1][1] = -bx * idet;
    gl[2][0] = -ay * idet; gl[2][1] = ax * idet;
    gl[0][0] = -(gl[1][0] + gl[2][0]); gl[0][1] = -(gl[1][1] + gl[2][1]);
    *area = 0.5 * fabs(det);
    if (hcell) {
        const double cx = X[2][0] - X[1][0], cy = X[2][1] - X[1][1];
        *hcell = sqrt((ax * ax + ay * ay) * (bx * bx + by * by) * (cx * cx + cy * cy)) / (2.0 * *area);
    }
}

__global__ void __launch_bounds__(FS_BLOCK) k_assemble_ns_tri(const double* __restrict__ xyz, const int32_t* __restrict__ cells,
                                                              const int32_t* __restrict__ cell_dofs, int64_t nc, int64_t n_rows,
                                                              const double* __restrict__ w0, const double* __restrict__ wprev,
                                                              ns_params P, double* __restrict__ ebuf, double* __restrict__ g) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const bool has_prev = wprev != nullptr && P.inv_dt != 0.0;
    for (; t < nc * 36; t += stride) {
        const int64_t c = t / 36;
        const int ab = (int)(t - c * 36);
        const int a = ab / 6, b = ab - a * 6;
        int32_t nd[6];
#pragma unroll
        for (int n = 0; n < 6; ++n) nd[n] = cell_dofs[c * 6 + n];
        double gl[3][2], area, hcell = 0.0;
        ns_tri_geometry(xyz, cells, c, gl, &area, P.g2 ? &hcell : nullptr);
        double U0[6][2], UP[6][2];
#pragma unroll
        for (int n = 0; n < 6; ++n) {
            U0[n][0] = P.convection ? w0[4 * (int64_t)nd[n]] : 0.0;
            U0[n][1] = P.convection ? w0[4 * (int64_t)nd[n] + 1] : 0.0;
            UP[n][0] = has_prev ? wprev[4 * (int64_t)nd[n]] : 0.0;
            UP[n][1] = has_prev ? wprev[4 * (int64_t)nd[n] + 1] : 0.0;
        }
        double P0[3] = {0.0, 0.0, 0.0}, T0[3] = {0.0, 0.0, 0.0};
        if (P.V.kind) {
#pragma unroll
            for (int v = 0; v < 3; ++v) P0[v] = w0[4 * (int64_t)nd[v] + 3];
            if (P.V.kind == 2)
#pragma unroll
                for (int v = 0; v < 3; ++v) T0[v] = P.V.T[nd[v]];
        }
        double blk[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) blk[i][j] = 0.0;
        double gv[2] = {0.0, 0.0};
        const bool do_rhs = b == 0;
        const bool full = P.convection && P.newton;
        for (int q = 0; q < 7; ++q) {
            const double l[3] = {NS_TRI_QP[q][0], NS_TRI_QP[q][1], NS_TRI_QP[q][2]};
            const double wv = NS_TRI_QW[q] * area;
            const double nuq = fs_viscosity(P.V, P.nu, l[0] * P0[0] + l[1] * P0[1] + l[2] * P0[2], l[0] * T0[0] + l[1] * T0[1] + l[2] * T0[2]);
            double pa, pb, ga[2], gb[2];
            p2tri_eval(a, l, gl, &pa, ga);
            p2tri_eval(b, l, gl, &pb, gb);
            double diag = nuq * (ga[0] * gb[0] + ga[1] * gb[1]) + P.inv_dt * pa * pb;
            double u0[2] = {0.0, 0.0}, gu0[2][2] = {{0.0, 0.0}, {0.0, 0.0}}, up[2] = {0.0, 0.0};
#pragma unroll
            for (int n = 0; n < 6; ++n) {
                double pn, gn[2];
                p2tri_eval(n, l, gl, &pn, gn);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    u0[i] += pn * U0[n][i];
                    up[i] += pn * UP[n][i];
                    gu0[i][0] += U0[n][i] * gn[0];
                    gu0[i][1] += U0[n][i] * gn[1];
                }
            }
            if (P.convection) {
                const double av[2] = {u0[0] - P.wm[0], u0[1] - P.wm[1]};
                const double agb = av[0] * gb[0] + av[1] * gb[1];
                diag += pa * agb;
                if (P.g2) {
                    const double aga = av[0] * ga[0] + av[1] * ga[1];
                    diag -= ns_g2_delta(P, hcell, av[0] * av[0] + av[1] * av[1]) * aga * agb;
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                blk[i][i] += wv * diag;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    double v = nuq * ga[j] * gb[i];
                    if (full) v += pa * pb * gu0[i][j];
                    blk[i][j] += wv * v;
                }
            }
            if (b < 3) {   // pressure trial function psi_b = lambda_b
                const double psi = sel3(b, l[0], l[1], l[2]);
                blk[0][3] -= wv * P.inv_rho * psi * ga[0];
                blk[1][3] -= wv * P.inv_rho * psi * ga[1];
            }
            if (a < 3) {   // continuity test function psi_a
                const double psi = sel3(a, l[0], l[1], l[2]);
                blk[3][0] += wv * P.inv_rho * psi * gb[0];
                blk[3][1] += wv * P.inv_rho * psi * gb[1];
            }
            if (do_rhs) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    double v = P.f[i];
                    if (full) v += gu0[i][0] * u0[0] + gu0[i][1] * u0[1];
                    if (has_prev) v += P.inv_dt * up[i];
                    gv[i] += wv * pa * v;
                }
            }
        }
        double2* __restrict__ out = reinterpret_cast<double2*>(ebuf + t * 16);       // source index c*36 + ab = t
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            out[2 * i] = make_double2(blk[i][0], blk[i][1]);
            out[2 * i + 1] = make_double2(blk[i][2], blk[i][3]);
        }
        if (do_rhs && nd[a] < n_rows) {
            atomicAdd(&g[4 * (int64_t)nd[a]], gv[0]);
            atomicAdd(&g[4 * (int64_t)nd[a] + 1], gv[1]);
        }
    }
}

// unit diagonal on the dummy slots of the 2-D layout: u_z of every node, the pressure of edge nodes
__global__ void k_ns_dummy_rows_2d(int64_t nv, int64_t n_nodes, const int64_t* __restrict__ slice_ptr,
                                   const int32_t* __restrict__ sell_col, double* __restrict__ val, int64_t plane) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; r < n_nodes; r += stride) {
        const int64_t sp0 = slice_ptr[r >> 6];
        const int width = (int)((slice_ptr[(r >> 6) + 1] - sp0) >> 6);
        const int64_t base = sp0 + (r & 63);
        for (int k = 0; k < width; ++k) {
            const int64_t e = base + (int64_t)k * FS_SLICE;
            if (sell_col[e] == (int32_t)r) {
                val[10 * plane + e] = 1.0;
                if (r >= nv) val[15 * plane + e] = 1.0;
                break;
            }
        }
    }
}

// ---- second pass: stored block e = sum of its element blocks (fixed order: deterministic, no atomics) -------------------
__global__ void __launch_bounds__(FS_BLOCK) k_ns_gather(int64_t n_entries, const int32_t* __restrict__ ptr, const int32_t* __restrict__ src,
                                                        const double* __restrict__ ebuf, double* __restrict__ val, int64_t plane) {
    // 8 lanes per stored block: lane w reads the 16 bytes (values 2w, 2w+1) of every element block, so a block is one
    // coalesced 128-byte read
    typedef double v2d __attribute__((ext_vector_type(2)));
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; t < n_entries * 8; t += stride) {
        const int64_t e = t >> 3;
        const int w = (int)(t & 7);
        double a0 = 0.0, a1 = 0.0;
        const int32_t q1 = ptr[e + 1];
        for (int32_t q = ptr[e]; q < q1; ++q) {
            const v2d v = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(ebuf + (int64_t)src[q] * 16) + w);   // read once
            a0 += v.x;
            a1 += v.y;
        }
        val[(int64_t)(2 * w) * plane + e] = a0;
        val[(int64_t)(2 * w + 1) * plane + e] = a1;
    }
}
// unit diagonal on the dummy pressure slot of edge nodes
__global__ void k_ns_dummy_rows(int64_t nv, int64_t n_nodes, const int64_t* __restrict__ slice_ptr,
                                const int32_t* __restrict__ sell_col, double* __restrict__ val, int64_t plane) {
    int64_t r = nv + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; r < n_nodes; r += stride) {
        const int64_t sp0 = slice_ptr[r >> 6];
        const int width = (int)((slice_ptr[(r >> 6) + 1] - sp0) >> 6);
        const int64_t base = sp0 + (r & 63);
        for (int k = 0; k < width; ++k) {
            const int64_t e = base + (int64_t)k * FS_SLICE;
            if (sell_col[e] == (int32_t)r) { val[15 * plane + e] = 1.0; break; }
        }
    }
}

// After a periodic fold (fs_matrix_tie_nodes) the dummy pressure slot of a master edge node holds 2 (its own unit
// diagonal plus the slave's); the operator product treats those rows as the identity, so the stored value follows.
void fs_ns_reset_dummy_rows(fs_matrix_s* J, hipStream_t s) {
    fs_space_s* sp = J->space;
    const int64_t nv = sp->mesh->n_owned;
    if (sp->mesh->tdim == 2) {
        hipLaunchKernelGGL(k_ns_dummy_rows_2d, dim3(fs_grid_for(sp->n_nodes_owned)), dim3(FS_BLOCK), 0, s, nv, sp->n_nodes_owned,
                           sp->slice_ptr.p, sp->sell_col.p, J->val.p, sp->sell_entries);
        return;
    }
    if (sp->n_nodes_owned <= nv) return;
    hipLaunchKernelGGL(k_ns_dummy_rows, dim3(fs_grid_for(sp->n_nodes_owned - nv)), dim3(FS_BLOCK), 0, s, nv, sp->n_nodes_owned,
                       sp->slice_ptr.p, sp->sell_col.p, J->val.p, sp->sell_entries);
}

// The law a Taylor-Hood space carries (fs_space_set_viscosity_law), else the (p_ref, exponent) pair of the call
fs_visc_dev fs_space_viscosity(const fs_space_s* sp, double legacy_pref, double legacy_exp) {
    if (sp && sp->visc.kind) return sp->visc;
    fs_visc_dev V;
    if (legacy_pref > 0.0) { V.kind = 1; V.pref = legacy_pref; V.ex = legacy_exp; }
    return V;
}

extern "C" int fs_space_set_viscosity_law(fs_space_t th_space, const fs_viscosity_law* law) {
    FS_REFUSE_DG_SPACE(th_space, "fs_space_set_viscosity_law");
    FS_REQUIRE(th_space, "fs_space_set_viscosity_law: null space");
    fs_visc_dev V;
    if (law && law->kind) {
        FS_REQUIRE(th_space->degree == 2 && th_space->ncomp == 4, "fs_space_set_viscosity_law: not a Taylor-Hood space");
        FS_REQUIRE((law->kind == 1 || law->kind == 2) && law->pressure_ref > 0.0, "fs_space_set_viscosity_law: kind 1 or 2 with a positive reference pressure");
        V.kind = law->kind;
        V.pref = law->pressure_ref;
        V.ex = law->pressure_exponent;
        if (law->kind == 2) {
            FS_REQUIRE(law->temperature && law->temperature_ref != 0.0 && law->temperature->d.n >= th_space->n_nodes_local,
                       "fs_space_set_viscosity_law: kind 2 needs the CG1 temperature (one value per local node, read at the vertex nodes) and its reference");
            V.cp = law->pressure_coef;
            V.ct = law->temperature_coef;
            V.tref = law->temperature_ref;
            V.T = law->temperature->d.p;
        }
    }
    th_space->visc = V;
    return FS_OK;
}

extern "C" int fs_assemble_navier_stokes(fs_matrix_t J, fs_vector_t g, fs_vector_t w0, fs_vector_t w_prev,
                                         const fs_ns_form* form) {
    FS_REFUSE_DG(J, "fs_assemble_navier_stokes");
    FS_CHECK(fs_require_init());
    FS_REQUIRE(J && g && form, "fs_assemble_navier_stokes: null pointer");
    fs_space_s* sp = J->space;
    FS_REQUIRE(sp->degree == 2 && sp->ncomp == 4 && J->bs == 4, "fs_assemble_navier_stokes: the matrix must live on a 4-component CG2 space");
    FS_REQUIRE(sp->slots.p, "fs_assemble_navier_stokes: the space has no slot table");
    FS_REQUIRE(!form->convection || w0, "fs_assemble_navier_stokes: convection needs the state w0");
    FS_REQUIRE(g->d.n >= sp->n_dofs_owned && (!w0 || w0->d.n >= sp->n_dofs_local) && (!w_prev || w_prev->d.n >= sp->n_dofs_local),
               "fs_assemble_navier_stokes: vector too short");
    FS_REQUIRE(form->density > 0.0 && form->inv_dt >= 0.0, "fs_assemble_navier_stokes: bad density / time step");
    hipStream_t s = fs_rt().stream;
    fs_mesh_s* m = sp->mesh;
    ns_params P;
    P.nu = form->kinematic_viscosity;
    P.inv_rho = 1.0 / form->density;
    P.inv_dt = form->inv_dt;
    for (int i = 0; i < 3; ++i) P.f[i] = form->body_force[i];
    for (int i = 0; i < 3; ++i) P.wm[i] = form->convection ? form->mesh_velocity[i] : 0.0;
    P.convection = form->convection ? 1 : 0;
    P.newton = form->newton ? 1 : 0;
    FS_REQUIRE(form->g2_mode >= 0 && form->g2_mode <= 2 && (form->g2_mode == 0 || form->convection), "fs_assemble_navier_stokes: bad G2 mode");
    P.g2 = form->g2_mode;
    P.g2_kappa = form->g2_kappa1;
    FS_REQUIRE(form->viscosity_pressure_ref >= 0.0 && (form->viscosity_pressure_ref == 0.0 || w0),
               "fs_assemble_navier_stokes: the pressure-dependent viscosity needs a positive reference pressure and the state w0");
    P.V = fs_space_viscosity(sp, form->viscosity_pressure_ref, form->viscosity_pressure_exponent);
    FS_REQUIRE(P.V.kind == 0 || w0, "fs_assemble_navier_stokes: a non-Newtonian law needs the state w0");
    FS_HIP(hipMemsetAsync(g->d.p, 0, (size_t)sp->n_dofs_owned * sizeof(double), s));
    if (m->tdim == 2) {
        // triangles: element blocks -> buffer -> one sum per stored block (always two-pass), dummy u_z / edge-pressure rows
        if (!sp->gmap_ptr.p) FS_CHECK(fs_space_build_gather_map(sp, s));
        if (sp->elem_buf.n != m->nc * 36 * 16) FS_CHECK(sp->elem_buf.alloc(m->nc * 36 * 16));
        hipLaunchKernelGGL(k_assemble_ns_tri, dim3(fs_grid_for(m->nc * 36, FS_BLOCK, 1 << 16)), dim3(FS_BLOCK), 0, s, m->xyz.p, m->cells.p,
                           sp->cell_dofs, m->nc, sp->n_nodes_owned, w0 ? w0->d.p : nullptr, w_prev ? w_prev->d.p : nullptr, P,
                           sp->elem_buf.p, g->d.p);
        hipLaunchKernelGGL(k_ns_gather, dim3(fs_grid_for(sp->sell_entries * 8, FS_BLOCK, 1 << 18)), dim3(FS_BLOCK), 0, s, sp->sell_entries,
                           sp->gmap_ptr.p, sp->gmap_src.p, sp->elem_buf.p, J->val.p, sp->sell_entries);
        J->taylor_hood = true;
        hipLaunchKernelGGL(k_ns_dummy_rows_2d, dim3(fs_grid_for(sp->n_nodes_owned)), dim3(FS_BLOCK), 0, s, m->n_owned, sp->n_nodes_owned,
                           sp->slice_ptr.p, sp->sell_col.p, J->val.p, sp->sell_entries);
        FS_KERNEL_CHECK();
        FS_HIP(hipStreamSynchronize(s));
        return FS_OK;
    }
    // Element blocks -> buffer -> one sum per stored block: 25 ms with 544 M device-scope fp64 atomics became 7 ms
    // (MI355X, configs[4]) and the matrix is bit-reproducible.  FS_NS_ASSEMBLE=atomic / pair selects the one-pass
    // kernels (no 6 GB element buffer).
    static const char* mode_env = getenv("FS_NS_ASSEMBLE");
    const bool two_pass = !mode_env || (mode_env[0] != 'a' && mode_env[0] != 'p');
    if (two_pass) {
        if (!sp->gmap_ptr.p) FS_CHECK(fs_space_build_gather_map(sp, s));
        if (!sp->elem_buf.p) FS_CHECK(sp->elem_buf.alloc(m->nc * 1600));
    } else {
        FS_CHECK(J->val.zero(s));
    }
    if (!two_pass && mode_env[0] == 'p') {
        const int grid = fs_grid_for(m->nc * 100, FS_BLOCK, 1 << 16);
        hipLaunchKernelGGL(k_assemble_ns, dim3(grid), dim3(FS_BLOCK), 0, s, m->xyz.p, m->cells.p, sp->cell_dofs, m->nc, sp->slots.p,
                           w0 ? w0->d.p : nullptr, w_prev ? w_prev->d.p : nullptr, P, J->val.p, sp->sell_entries, g->d.p);
    } else {
        const int grid = (int)std::min<int64_t>((m->nc + NS_WPB - 1) / NS_WPB, 1 << 16);
        hipLaunchKernelGGL(k_assemble_ns_wave, dim3(std::max(grid, 1)), dim3(FS_BLOCK), 0, s, m->xyz.p, m->cells.p, sp->cell_dofs, m->nc,
                           sp->n_nodes_owned, sp->slots.p,
                           w0 ? w0->d.p : nullptr, w_prev ? w_prev->d.p : nullptr, P, J->val.p, sp->sell_entries,
                           two_pass ? sp->elem_buf.p : nullptr, g->d.p);
        if (two_pass)
            hipLaunchKernelGGL(k_ns_gather, dim3(fs_grid_for(sp->sell_entries * 8, FS_BLOCK, 1 << 18)), dim3(FS_BLOCK), 0, s, sp->sell_entries,
                               sp->gmap_ptr.p, sp->gmap_src.p, sp->elem_buf.p, J->val.p, sp->sell_entries);
    }
    J->taylor_hood = true;      // lets the operator product skip the structurally empty pressure planes
    hipLaunchKernelGGL(k_ns_dummy_rows, dim3(fs_grid_for(sp->n_nodes_owned - m->n_owned)), dim3(FS_BLOCK), 0, s, m->n_owned,
                       sp->n_nodes_owned, sp->slice_ptr.p, sp->sell_col.p, J->val.p, sp->sell_entries);
    FS_KERNEL_CHECK();
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

// ---- pressure boundaries: F += inner(p_b n, v) ds - nu inner((grad(u) + grad(u)^T) n, v) ds -----------------------
// (CoupledNavierStokesSolver.py:449-453 pressure Dirichlet, :459-460 pressure 'farfield')
// 6-point degree-4 triangle rule; the facet's P2 nodes as cell-local node indices, by opposite vertex
__device__ const double NS_TQ[6][3] = {{0.108103018168070, 0.445948490915965, 0.445948490915965},
                                       {0.445948490915965, 0.108103018168070, 0.445948490915965},
                                       {0.445948490915965, 0.445948490915965, 0.108103018168070},
                                       {0.816847572980459, 0.091576213509771, 0.091576213509771},
                                       {0.091576213509771, 0.816847572980459, 0.091576213509771},
                                       {0.091576213509771, 0.091576213509771, 0.816847572980459}};
__device__ const double NS_TW[6] = {0.223381589678011, 0.223381589678011, 0.223381589678011,
                                    0.109951743655322, 0.109951743655322, 0.109951743655322};
__device__ const int NS_FACE_NODES[4][6] = {{1, 2, 3, 4, 5, 6}, {0, 2, 3, 4, 7, 8}, {0, 1, 3, 5, 7, 9}, {0, 1, 2, 6, 8, 9}};

// thread t = (facet, facet node al, cell node b)
__global__ void k_ns_pressure_boundary(int64_t nf, const int32_t* __restrict__ facet_cell, const int32_t* __restrict__ facet_opp,
                                       const double* __restrict__ facet_value, double nu0, const double* __restrict__ xyz,
                                       const int32_t* __restrict__ cells, const int32_t* __restrict__ cell_dofs, int64_t nc,
                                       const int32_t* __restrict__ slots,
                                       double* __restrict__ val, int64_t plane, double* __restrict__ g,
                                       const double* __restrict__ w0, fs_visc_dev V, int vstride) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; t < nf * 60; t += stride) {
        const int64_t f = t / 60;
        const int r = (int)(t - f * 60);
        const int al = r / 10, b = r - al * 10;
        const int64_t c = facet_cell[f];
        const int o = facet_opp[f];
        const int a = NS_FACE_NODES[o][al];
        int32_t nd[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) nd[v] = cells[c * 4 + v];     // vertex ids (geometry), not node ids
        double X[4][3];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            X[v][0] = xyz[4 * (int64_t)nd[v]]; X[v][1] = xyz[4 * (int64_t)nd[v] + 1]; X[v][2] = xyz[4 * (int64_t)nd[v] + 2];
        }
        const double e1[3] = {X[1][0] - X[0][0], X[1][1] - X[0][1], X[1][2] - X[0][2]};
        const double e2[3] = {X[2][0] - X[0][0], X[2][1] - X[0][1], X[2][2] - X[0][2]};
        const double e3[3] = {X[3][0] - X[0][0], X[3][1] - X[0][1], X[3][2] - X[0][2]};
        const double c23[3] = {e2[1] * e3[2] - e2[2] * e3[1], e2[2] * e3[0] - e2[0] * e3[2], e2[0] * e3[1] - e2[1] * e3[0]};
        const double c31[3] = {e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]};
        const double c12[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double det = e1[0] * c23[0] + e1[1] * c23[1] + e1[2] * c23[2];
        const double idet = 1.0 / det;
        double gl[4][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            gl[1][k] = c23[k] * idet;
            gl[2][k] = c31[k] * idet;
            gl[3][k] = c12[k] * idet;
            gl[0][k] = -(gl[1][k] + gl[2][k] + gl[3][k]);
        }
        const double vol = fabs(det) * (1.0 / 6.0);
        double go[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) go[k] = sel4(o, gl[0][k], gl[1][k], gl[2][k], gl[3][k]);
        const double gnorm = sqrt(go[0] * go[0] + go[1] * go[1] + go[2] * go[2]);
        const double n[3] = {-go[0] / gnorm, -go[1] / gnorm, -go[2] / gnorm};   // outward
        const double area = 3.0 * vol * gnorm;
        double blk[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        double gv[3] = {0.0, 0.0, 0.0};
        // boundary pressure: one value per facet, or (vstride 3) its values at the facet's vertices - the P1 interpolant DOLFIN
        // evaluates a degree-1 Expression with - in the order of the cell's local vertices
        double pbv[3] = {0.0, 0.0, 0.0};
        if (facet_value) {
            if (vstride == 3) { pbv[0] = facet_value[3 * f]; pbv[1] = facet_value[3 * f + 1]; pbv[2] = facet_value[3 * f + 2]; }
            else pbv[0] = pbv[1] = pbv[2] = facet_value[f];
        }
        double P0[4] = {0.0, 0.0, 0.0, 0.0}, T0[4] = {0.0, 0.0, 0.0, 0.0};
        if (V.kind) {
#pragma unroll
            for (int v = 0; v < 4; ++v) P0[v] = w0[4 * (int64_t)cell_dofs[c * 10 + v] + 3];
            if (V.kind == 2)
#pragma unroll
                for (int v = 0; v < 4; ++v) T0[v] = V.T[cell_dofs[c * 10 + v]];
        }
        for (int q = 0; q < 6; ++q) {
            double l[4];
            int kk = 0;
#pragma unroll
            for (int v = 0; v < 4; ++v) l[v] = (v == o) ? 0.0 : NS_TQ[q][kk++];
            const double wv = NS_TW[q] * area;
            const double pb = NS_TQ[q][0] * pbv[0] + NS_TQ[q][1] * pbv[1] + NS_TQ[q][2] * pbv[2];
            const double nu = fs_viscosity(V, nu0, l[0] * P0[0] + l[1] * P0[1] + l[2] * P0[2] + l[3] * P0[3],
                                           l[0] * T0[0] + l[1] * T0[1] + l[2] * T0[2] + l[3] * T0[3]);
            double pa, pbf, ga[3], gb[3];
            p2_eval(a, l, gl, &pa, ga);
            p2_eval(b, l, gl, &pbf, gb);
            const double gn = gb[0] * n[0] + gb[1] * n[1] + gb[2] * n[2];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) blk[i][j] -= nu * wv * pa * ((i == j ? gn : 0.0) + gb[i] * n[j]);
                gv[i] -= wv * pb * n[i] * pa;
            }
        }
        const int32_t slot = slots[(int64_t)(a * 10 + b) * nc + c];
        if (slot < 0) continue;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) atomicAdd(&val[(int64_t)(i * 4 + j) * plane + slot], blk[i][j]);
        if (b == 0 && facet_value) {
            const int32_t node = cell_dofs[c * 10 + a];
#pragma unroll
            for (int i = 0; i < 3; ++i) atomicAdd(&g[4 * (int64_t)node + i], gv[i]);
        }
    }
}

// the same on boundary EDGES of a triangle mesh: the edge opposite local vertex o carries the P2 nodes (i, j, 3 + o) with
// i < j the other two vertices; 3-point Gauss-Legendre rule (degree 5); thread t = (facet, facet node al, cell node b)
__global__ void k_ns_pressure_boundary_tri(int64_t nf, const int32_t* __restrict__ facet_cell, const int32_t* __restrict__ facet_opp,
                                           const double* __restrict__ facet_value, double nu0, const double* __restrict__ xyz,
                                           const int32_t* __restrict__ cells, const int32_t* __restrict__ cell_dofs, int64_t nc,
                                           const int32_t* __restrict__ slots, double* __restrict__ val, int64_t plane,
                                           double* __restrict__ g, const double* __restrict__ w0, fs_visc_dev V,
                                           int vstride) {
    const double GS[3] = {0.5 - 0.5 * 0.7745966692414834, 0.5, 0.5 + 0.5 * 0.7745966692414834};
    const double GW[3] = {5.0 / 18.0, 8.0 / 18.0, 5.0 / 18.0};
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; t < nf * 18; t += stride) {
        const int64_t f = t / 18;
        const int r = (int)(t - f * 18);
        const int al = r / 6, b = r - al * 6;
        const int64_t c = facet_cell[f];
        const int o = facet_opp[f];
        const int vi = o == 0 ? 1 : 0, vj = o == 2 ? 1 : 2;          // the edge's vertices, ascending local index
        const int a = al == 0 ? vi : (al == 1 ? vj : 3 + o);
        double gl[3][2], area;
        ns_tri_geometry(xyz, cells, c, gl, &area, nullptr);
        const double gnorm = sqrt(gl[o][0] * gl[o][0] + gl[o][1] * gl[o][1]);
        const double n[2] = {-gl[o][0] / gnorm, -gl[o][1] / gnorm};     // outward
        const double len = 2.0 * area * gnorm;
        double pbv[2] = {0.0, 0.0};
        if (facet_value) {
            if (vstride == 2) { pbv[0] = facet_value[2 * f]; pbv[1] = facet_value[2 * f + 1]; }
            else pbv[0] = pbv[1] = facet_value[f];
        }
        double P0[3] = {0.0, 0.0, 0.0}, T0[3] = {0.0, 0.0, 0.0};
        if (V.kind) {
#pragma unroll
            for (int v = 0; v < 3; ++v) P0[v] = w0[4 * (int64_t)cell_dofs[c * 6 + v] + 3];
            if (V.kind == 2)
#pragma unroll
                for (int v = 0; v < 3; ++v) T0[v] = V.T[cell_dofs[c * 6 + v]];
        }
        double blk[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
        double gv[2] = {0.0, 0.0};
        for (int q = 0; q < 3; ++q) {
            double l[3] = {0.0, 0.0, 0.0};
            l[vi] = 1.0 - GS[q];
            l[vj] = GS[q];
            const double wv = GW[q] * len;
            const double pb = (1.0 - GS[q]) * pbv[0] + GS[q] * pbv[1];
            const double nu = fs_viscosity(V, nu0, l[0] * P0[0] + l[1] * P0[1] + l[2] * P0[2], l[0] * T0[0] + l[1] * T0[1] + l[2] * T0[2]);
            double pa, pbf, ga[2], gb[2];
            p2tri_eval(a, l, gl, &pa, ga);
            p2tri_eval(b, l, gl, &pbf, gb);
            const double gn = gb[0] * n[0] + gb[1] * n[1];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
#pragma unroll
                for (int j = 0; j < 2; ++j) blk[i][j] -= nu * wv * pa * ((i == j ? gn : 0.0) + gb[i] * n[j]);
                gv[i] -= wv * pb * n[i] * pa;
            }
        }
        const int32_t slot = slots[(int64_t)(a * 6 + b) * nc + c];
        if (slot < 0) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) atomicAdd(&val[(int64_t)(i * 4 + j) * plane + slot], blk[i][j]);
        if (b == 0 && facet_value) {
            const int32_t node = cell_dofs[c * 6 + a];
            atomicAdd(&g[4 * (int64_t)node], gv[0]);
            atomicAdd(&g[4 * (int64_t)node + 1], gv[1]);
        }
    }
}

extern "C" int fs_assemble_ns_pressure_boundary_nn(fs_matrix_t J, fs_vector_t g, int64_t n_facets, const int32_t* facet_cell,
                                                   const int32_t* facet_opposite, const double* facet_value,
                                                   double kinematic_viscosity, fs_vector_t w0, double nn_pref, double nn_exp,
                                                   int values_per_facet);
extern "C" int fs_assemble_ns_pressure_boundary(fs_matrix_t J, fs_vector_t g, int64_t n_facets, const int32_t* facet_cell,
                                                const int32_t* facet_opposite, const double* facet_value,
                                                double kinematic_viscosity) {
    FS_REFUSE_DG(J, "fs_assemble_ns_pressure_boundary");
    return fs_assemble_ns_pressure_boundary_nn(J, g, n_facets, facet_cell, facet_opposite, facet_value, kinematic_viscosity, nullptr, 0.0, 0.0, 1);
}
extern "C" int fs_assemble_ns_pressure_boundary_nn(fs_matrix_t J, fs_vector_t g, int64_t n_facets, const int32_t* facet_cell,
                                                   const int32_t* facet_opposite, const double* facet_value,
                                                   double kinematic_viscosity, fs_vector_t w0, double nn_pref, double nn_exp,
                                                   int values_per_facet) {
    FS_REFUSE_DG(J, "fs_assemble_ns_pressure_boundary");
    FS_CHECK(fs_require_init());
    FS_REQUIRE(J && J->space && J->space->mesh, "fs_assemble_ns_pressure_boundary: null matrix");
    const int fverts = J->space->mesh->tdim;      // vertices of a boundary facet: 3 (triangle) or 2 (edge of a 2-D mesh)
    FS_REQUIRE(values_per_facet == 1 || values_per_facet == fverts, "fs_assemble_ns_pressure_boundary: values_per_facet must be 1 or %d", fverts);
    const fs_visc_dev V = fs_space_viscosity(J->space, nn_pref, nn_exp);
    FS_REQUIRE(nn_pref >= 0.0 && (V.kind == 0 || (w0 && J && w0->d.n >= J->space->n_dofs_local)),
               "fs_assemble_ns_pressure_boundary: the pressure-dependent viscosity needs a positive reference pressure and the state w0");
    FS_REQUIRE(J && g && n_facets >= 0 && (n_facets == 0 || (facet_cell && facet_opposite)), "fs_assemble_ns_pressure_boundary: bad arguments");
    fs_space_s* sp = J->space;
    FS_REQUIRE(sp->degree == 2 && sp->ncomp == 4 && sp->slots.p, "fs_assemble_ns_pressure_boundary: not a Taylor-Hood block matrix");
    if (n_facets == 0) return FS_OK;
    fs_mesh_s* m = sp->mesh;
    for (int64_t i = 0; i < n_facets; ++i)
        FS_REQUIRE(facet_cell[i] >= 0 && facet_cell[i] < m->nc && facet_opposite[i] >= 0 && facet_opposite[i] <= fverts,
                   "fs_assemble_ns_pressure_boundary: facet %lld names cell %d / local vertex %d", (long long)i, facet_cell[i], facet_opposite[i]);
    hipStream_t s = fs_rt().stream;
    dbuf<int32_t> dc, dop;
    dbuf<double> dv;
    FS_CHECK(dc.alloc(n_facets));
    FS_CHECK(dop.alloc(n_facets));
    FS_CHECK(dc.upload(facet_cell, n_facets, s));
    FS_CHECK(dop.upload(facet_opposite, n_facets, s));
    if (facet_value) {
        FS_CHECK(dv.alloc(n_facets * values_per_facet));
        FS_CHECK(dv.upload(facet_value, n_facets * values_per_facet, s));
    }
    if (fverts == 2)
        hipLaunchKernelGGL(k_ns_pressure_boundary_tri, dim3(fs_grid_for(n_facets * 18)), dim3(FS_BLOCK), 0, s, n_facets, dc.p, dop.p,
                           facet_value ? dv.p : (const double*)nullptr, kinematic_viscosity, m->xyz.p, m->cells.p, sp->cell_dofs, m->nc,
                           sp->slots.p, J->val.p, sp->sell_entries, g->d.p, V.kind ? (const double*)w0->d.p : (const double*)nullptr,
                           V, values_per_facet);
    else
    hipLaunchKernelGGL(k_ns_pressure_boundary, dim3(fs_grid_for(n_facets * 60)), dim3(FS_BLOCK), 0, s, n_facets, dc.p, dop.p,
                       facet_value ? dv.p : (const double*)nullptr, kinematic_viscosity, m->xyz.p, m->cells.p, sp->cell_dofs, m->nc,
                       sp->slots.p, J->val.p, sp->sell_entries, g->d.p, V.kind ? (const double*)w0->d.p : (const double*)nullptr,
                       V, values_per_facet);
    FS_KERNEL_CHECK();
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

void fs_saddle_preload() {
    hipFuncAttributes attr;
    (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(k_ns_dummy_rows));
    (void)hipGetLastError();
}

#include "fs_saddle_solve.inc"     // the Krylov solve: the FGMRES kernels, both block preconditioners, the host side of fs_saddle_solve
