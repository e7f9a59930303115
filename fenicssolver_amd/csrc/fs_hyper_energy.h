// The hyperelastic energies in invariant form and the P1 kinematics their kernels share (fs_hyper_models.hip: tangent, force, energy
// and Cauchy stress; fs_hyper_dynamics.hip: the explicit marcher).  Header-only, moved here from fs_hyper_models.hip with the text
// unchanged; the formulas and the meaning of the parameter row p[4] are described at the top of that file.
#pragma once
#include "fs_common.h"
#include "fs_kernels.h"
#include "fs_p1_cell.h"
#include <math.h>
#include <type_traits>
#include <vector>

struct hm_par { double p[4]; };
struct hm_w { double w1, w2, wj, w11, w12, w1j, w22, w2j, wjj; };

// ---- the models ------------------------------------------------------------------------------------------------------------------
struct m_svk {
    static __device__ __forceinline__ void eval(const hm_par& q, double I1, double I2, double J, hm_w& w, double& psi) {
        const double mu = q.p[0], lm = q.p[1];
        psi = 0.125 * lm * (I1 - 3.0) * (I1 - 3.0) + 0.25 * mu * (I1 * I1 - 2.0 * I2 - 2.0 * I1 + 3.0);
        w.w1 = 0.25 * lm * (I1 - 3.0) + 0.5 * mu * (I1 - 1.0);
        w.w2 = -0.5 * mu;
        w.w11 = 0.25 * lm + 0.5 * mu;
        w.wj = w.w12 = w.w1j = w.w22 = w.w2j = w.wjj = 0.0;
    }
};

struct m_neo {          // the Cauchy stress of the neo-Hookean energy (its tangent, force and energy are fs_hyper.hip's)
    static __device__ __forceinline__ void eval(const hm_par& q, double I1, double I2, double J, hm_w& w, double& psi) {
        const double mu = q.p[0], lm = q.p[1], lj = log(J);
        psi = 0.5 * mu * (I1 - 3.0) - mu * lj + 0.5 * lm * lj * lj;
        w.w1 = 0.5 * mu;
        w.wj = (lm * lj - mu) / J;
        w.wjj = (lm * (1.0 - lj) + mu) / (J * J);
        w.w2 = w.w11 = w.w12 = w.w1j = w.w22 = w.w2j = 0.0;
    }
};

// a = J^-2/3 and its first two derivatives with respect to J
__device__ __forceinline__ void hm_jm23(double J, double& a, double& a1, double& a2, double& iJ) {
    const double cj = cbrt(J);
    a = 1.0 / (cj * cj);
    iJ = 1.0 / J;
    a1 = -(2.0 / 3.0) * a * iJ;
    a2 = (10.0 / 9.0) * a * iJ * iJ;
}

struct m_mooney {
    static __device__ __forceinline__ void eval(const hm_par& q, double I1, double I2, double J, hm_w& w, double& psi) {
        const double c10 = q.p[0], c01 = q.p[1], kap = q.p[2];
        double a, a1, a2, iJ;
        hm_jm23(J, a, a1, a2, iJ);
        const double b = a * a, b1 = -(4.0 / 3.0) * b * iJ, b2 = (28.0 / 9.0) * b * iJ * iJ;      // J^-4/3
        psi = c10 * (a * I1 - 3.0) + c01 * (b * I2 - 3.0) + 0.5 * kap * (J - 1.0) * (J - 1.0);
        w.w1 = c10 * a;
        w.w2 = c01 * b;
        w.wj = c10 * I1 * a1 + c01 * I2 * b1 + kap * (J - 1.0);
        w.w1j = c10 * a1;
        w.w2j = c01 * b1;
        w.wjj = c10 * I1 * a2 + c01 * I2 * b2 + kap;
        w.w11 = w.w12 = w.w22 = 0.0;
    }
};

struct m_yeoh {
    static __device__ __forceinline__ void eval(const hm_par& q, double I1, double I2, double J, hm_w& w, double& psi) {
        const double c10 = q.p[0], c20 = q.p[1], c30 = q.p[2], kap = q.p[3];
        double a, a1, a2, iJ;
        hm_jm23(J, a, a1, a2, iJ);
        const double x = a * I1 - 3.0, xj = I1 * a1;
        const double f1 = c10 + x * (2.0 * c20 + 3.0 * c30 * x), f2 = 2.0 * c20 + 6.0 * c30 * x;
        psi = x * (c10 + x * (c20 + x * c30)) + 0.5 * kap * (J - 1.0) * (J - 1.0);
        w.w1 = f1 * a;
        w.wj = f1 * xj + kap * (J - 1.0);
        w.w11 = f2 * a * a;
        w.w1j = f2 * a * xj + f1 * a1;
        w.wjj = f2 * xj * xj + f1 * I1 * a2 + kap;
        w.w2 = w.w12 = w.w22 = w.w2j = 0.0;
    }
};

// ---- kinematics --------------------------------------------------------------------------------------------------------------------
// F = I + sum_a u_a g_a^T of the cell c (plane strain: embedded, F33 = 1), its volume (area), g_a and (PAIR) g_b with a zero third
// component in 2-D.  The gradient picks are select chains on a local geometry (fs_p1_cell.h): never an index into a register array.
template <int TD, bool PAIR>
__device__ __forceinline__ void hm_cell_load(int4 v4, const double* __restrict__ xyz4, const double* __restrict__ u, const box_snap& bx,
                                             int a, int b, double (&F)[3][3], double (&ga)[3], double (&gb)[3], double& vol) {
    if constexpr (TD == 3) {
        const int32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
        const tet_geom t = tet_geometry_box(xyz4, v, bx);
        vol = t.adet * (1.0 / 6.0);
        double uv[4][3];
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int k = 0; k < 3; ++k) uv[n][k] = u[3 * (int64_t)v[n] + k];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                F[i][j] = (i == j ? 1.0 : 0.0) + (((uv[0][i] * t.g[0][j] + uv[1][i] * t.g[1][j]) + uv[2][i] * t.g[2][j]) + uv[3][i] * t.g[3][j]);
        P1_GRAD_TET(t, a, ga);
        if (PAIR) P1_GRAD_TET(t, b, gb);
    } else {
        const tri_geom t = tri_geometry2(xyz4, v4.x, v4.y, v4.z);
        vol = t.area;
        const double2 u0 = reinterpret_cast<const double2*>(u)[v4.x], u1 = reinterpret_cast<const double2*>(u)[v4.y],
                      u2 = reinterpret_cast<const double2*>(u)[v4.z];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            F[0][j] = (j == 0 ? 1.0 : 0.0) + ((u0.x * t.g[0][j] + u1.x * t.g[1][j]) + u2.x * t.g[2][j]);
            F[1][j] = (j == 1 ? 1.0 : 0.0) + ((u0.y * t.g[0][j] + u1.y * t.g[1][j]) + u2.y * t.g[2][j]);
        }
        F[0][2] = F[1][2] = F[2][0] = F[2][1] = 0.0;
        F[2][2] = 1.0;
        double g2[2];
        p1_grad(t, a, g2);
        ga[0] = g2[0]; ga[1] = g2[1]; ga[2] = 0.0;
        if (PAIR) {
            p1_grad(t, b, g2);
            gb[0] = g2[0]; gb[1] = g2[1]; gb[2] = 0.0;
        }
    }
}

// cof F, B = F F^T, I1, I2, J
struct hm_state { double cof[3][3], B[3][3], I1, I2, J; };
__device__ __forceinline__ void hm_invariants(const double (&F)[3][3], hm_state& s) {
    s.cof[0][0] = F[1][1] * F[2][2] - F[1][2] * F[2][1];
    s.cof[0][1] = F[1][2] * F[2][0] - F[1][0] * F[2][2];
    s.cof[0][2] = F[1][0] * F[2][1] - F[1][1] * F[2][0];
    s.cof[1][0] = F[0][2] * F[2][1] - F[0][1] * F[2][2];
    s.cof[1][1] = F[0][0] * F[2][2] - F[0][2] * F[2][0];
    s.cof[1][2] = F[0][1] * F[2][0] - F[0][0] * F[2][1];
    s.cof[2][0] = F[0][1] * F[1][2] - F[0][2] * F[1][1];
    s.cof[2][1] = F[0][2] * F[1][0] - F[0][0] * F[1][2];
    s.cof[2][2] = F[0][0] * F[1][1] - F[0][1] * F[1][0];
    s.J = F[0][0] * s.cof[0][0] + F[0][1] * s.cof[0][1] + F[0][2] * s.cof[0][2];
    double bb = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            s.B[i][j] = F[i][0] * F[j][0] + F[i][1] * F[j][1] + F[i][2] * F[j][2];
            bb += s.B[i][j] * s.B[i][j];
        }
    s.I1 = s.B[0][0] + s.B[1][1] + s.B[2][2];
    s.I2 = 0.5 * (s.I1 * s.I1 - bb);
}

__device__ __forceinline__ void hm_mul(const double (&A)[3][3], const double (&x)[3], double (&y)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = A[i][0] * x[0] + A[i][1] * x[1] + A[i][2] * x[2];
}

// a_1, a_2, a_3 = (dI1/dF, dI2/dF, dJ/dF) g and Fg = F g
__device__ __forceinline__ void hm_dvec(const double (&F)[3][3], const hm_state& s, const double (&g)[3], double (&Fg)[3], double (&a1)[3],
                                        double (&a2)[3], double (&a3)[3]) {
    double BFg[3];
    hm_mul(F, g, Fg);
    hm_mul(s.B, Fg, BFg);
    hm_mul(s.cof, g, a3);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a1[i] = 2.0 * Fg[i];
        a2[i] = 2.0 * (s.I1 * Fg[i] - BFg[i]);
    }
}

__device__ __forceinline__ hm_par hm_row(const double2* __restrict__ rows, int64_t c) {
    const double2 x = rows[2 * c], y = rows[2 * c + 1];
    hm_par q;
    q.p[0] = x.x; q.p[1] = x.y; q.p[2] = y.x; q.p[3] = y.y;
    return q;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static const char* hm_name(int model) {
    return model == FS_HYPER_NEO_HOOKEAN ? "neo-Hookean" : model == FS_HYPER_ST_VENANT_KIRCHHOFF ? "St Venant-Kirchhoff"
           : model == FS_HYPER_MOONEY_RIVLIN ? "Mooney-Rivlin" : "Yeoh";
}

// one parameter row against the refusals of its model; cell < 0: the constant row
static int hm_check_row(int model, const double* p, const char* who, int64_t cell) {
    char where[64] = "the material";
    if (cell >= 0) snprintf(where, sizeof where, "cell %lld (device order)", (long long)cell);
    const bool fin = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && isfinite(p[3]);
    if (model == FS_HYPER_NEO_HOOKEAN || model == FS_HYPER_ST_VENANT_KIRCHHOFF) {
        FS_REQUIRE(fin && p[0] > 0.0 && p[1] >= 0.0, "%s: %s has mu = %g, lambda = %g: mu > 0 and lambda >= 0 are required (%s)", who, where, p[0],
                   p[1], hm_name(model));
    } else if (model == FS_HYPER_MOONEY_RIVLIN) {
        FS_REQUIRE(fin && p[0] >= 0.0 && p[1] >= 0.0 && p[0] + p[1] > 0.0 && p[2] > 0.0,
                   "%s: %s has c10 = %g, c01 = %g, kappa = %g: c10 >= 0, c01 >= 0, c10 + c01 > 0 and kappa > 0 are required (Mooney-Rivlin)", who,
                   where, p[0], p[1], p[2]);
    } else {
        FS_REQUIRE(fin && p[0] > 0.0 && p[3] > 0.0,
                   "%s: %s has c10 = %g, c20 = %g, c30 = %g, kappa = %g: finite values with c10 > 0 and kappa > 0 are required (Yeoh)", who, where,
                   p[0], p[1], p[2], p[3]);
    }
    return FS_OK;
}

// the parameter row of the form (par), or its per-cell rows [nc][4] (rows non-empty), checked
static int hm_material(const fs_hyper_form* form, int64_t nc, const char* who, hm_par& par, std::vector<double>& rows) {
    const int model = form->model;
    FS_REQUIRE(model == FS_HYPER_NEO_HOOKEAN || model == FS_HYPER_ST_VENANT_KIRCHHOFF || model == FS_HYPER_MOONEY_RIVLIN || model == FS_HYPER_YEOH,
               "%s: unknown energy model %d (FS_HYPER_NEO_HOOKEAN, _ST_VENANT_KIRCHHOFF, _MOONEY_RIVLIN, _YEOH)", who, model);
    rows.clear();
    for (int k = 0; k < 4; ++k) par.p[k] = 0.0;
    if (model == FS_HYPER_NEO_HOOKEAN || model == FS_HYPER_ST_VENANT_KIRCHHOFF) {
        FS_REQUIRE(form->lame.mode == FS_COEF_NONE || form->lame.mode == FS_COEF_CELL_LAME,
                   "%s: the Lame coefficient is FS_COEF_NONE (mu / lambda) or FS_COEF_CELL_LAME", who);
        if (form->lame.mode == FS_COEF_CELL_LAME) {
            FS_REQUIRE(form->lame.data, "%s: per-cell Lame data pointer is null", who);
            rows.assign((size_t)(4 * nc), 0.0);
            for (int64_t c = 0; c < nc; ++c) {
                rows[4 * c] = form->lame.data[2 * c];
                rows[4 * c + 1] = form->lame.data[2 * c + 1];
            }
        } else {
            par.p[0] = form->mu;
            par.p[1] = form->lambda;
        }
    } else {
        FS_REQUIRE(form->cell_params.mode == FS_COEF_NONE || form->cell_params.mode == FS_COEF_CELL_HYPER,
                   "%s: the %s parameters are FS_COEF_NONE (params) or FS_COEF_CELL_HYPER (cell_params)", who, hm_name(model));
        if (form->cell_params.mode == FS_COEF_CELL_HYPER) {
            FS_REQUIRE(form->cell_params.data, "%s: per-cell parameter data pointer is null", who);
            rows.assign(form->cell_params.data, form->cell_params.data + 4 * nc);
        } else {
            for (int k = 0; k < 4; ++k) par.p[k] = form->params[k];
        }
    }
    if (rows.empty()) return hm_check_row(model, par.p, who, -1);
    for (int64_t c = 0; c < nc; ++c) FS_CHECK(hm_check_row(model, &rows[4 * c], who, c));
    return FS_OK;
}

template <class F> static inline void hm_dispatch_model(int model, F&& f) {
    if (model == FS_HYPER_ST_VENANT_KIRCHHOFF) f(m_svk{});
    else if (model == FS_HYPER_MOONEY_RIVLIN) f(m_mooney{});
    else if (model == FS_HYPER_YEOH) f(m_yeoh{});
    else f(m_neo{});
}
