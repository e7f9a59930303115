// Small-strain linear viscoelasticity (generalized Maxwell solid, Prony series) on vector CG1 spaces (tetrahedra, and triangles in
// plane strain): the per-cell history, the constitutive update and the history load, on the device.
//
// The reference lists "viscoelastic" among its solvers under development (Readme.md) and never delivers one; the model is the
// textbook one.  Elastic bulk response, relaxing deviatoric response, with e = dev eps:
//   sigma(t) = K tr(eps) I + 2 G0 [ g_inf e + sum_k g_k h_k ],   h_k(t) = int_0^t exp(-(t - s)/tau_k) de/ds ds,   g_inf = 1 - sum_k g_k.
// One step of length dt, exact for a strain history linear within the step, with x_k = dt / tau_k:
//   a_k = exp(-x_k),   b_k = -expm1(-x_k) / x_k,   h_k^{n+1} = a_k h_k^n + b_k (e^{n+1} - e^n).
// b_k: expm1 keeps full precision for every normal x > 0, so the quotient is good to a few ulp; what it cannot do is x -> 0 (0/0 at
// x = 0, and denormal x).  Below x = FS_VISCO_SERIES_X = 1e-5 the series 1 - x/2 + x^2/6 - x^3/24 is used instead: its first dropped
// term x^4/120 is below 1e-22 there, far under one ulp of b ~ 1, so the two forms agree to rounding at the switch-over.
// A step is therefore ONE linear solve  K(mu_eff, lambda_eff) u^{n+1} = f_ext - int B^T s_hist dx  with
//   mu_eff = G0 (g_inf + sum_k g_k b_k),  lambda_eff = K - 2/3 mu_eff,  s_hist = 2 G0 sum_k g_k (a_k h_k^n - b_k e^n)
// (deviatoric, constant per cell); the operator is fs_assemble_matrix with (mu_eff, lambda_eff), nothing here assembles a matrix.
//
// Kernels (no atomics anywhere: two evaluations of one state give the same bits):
//   k_visco_coef      constant material only: (a_k, b_k) of the step, once, into a 16-double table every other kernel reads with
//       uniform loads.  A per-cell material evaluates visco_ab() per cell instead - the same function on the same inputs, so a
//       per-cell array holding one constant gives the constant's bits.
//   k_visco_update    one thread per cell: strain from the P1 geometry, trial e, h_k and sigma^{n+1} from the COMMITTED (e, h_k); counts
//       the non-finite cells per workgroup (p1_cell_tally; k_cell_tally_finish sums the partials in a fixed order).
//   k_visco_gather    the history load: one thread per owned node over the cells around it (the sources of its diagonal
//       block, ascending), -V s_hist g_a with s_hist evaluated in place from the committed state and this step's (a_k, b_k).
//   k_p1_stress_force_gather (fs_p1_cell.h)  the internal force +V sigma g_a from the trial stress (the equilibrium check
//       int B^T sigma dx), by the same walk.
//
// Tensor storage follows fs_plasticity.hip: 3-D (xx, yy, zz, xy, xz, yz), plane strain (xx, yy, zz, xy) - tensor components, not
// engineering shears; plane strain keeps e_zz = -tr(eps)/3, h_k,zz and sigma_zz.  h is stored [cell][term][component].
#include "fs_common.h"
#include "fs_kernels.h"
#include "fs_p1_cell.h"
#include <math.h>

#define FS_VISCO_SERIES_X 1e-5           // below this dt/tau, b_k comes from its series (see the file header)

struct fs_visco_state_s : fs_cell_history {
    int nt = 0;                          // Prony terms
    fs_history_pair e, h, sig;           // dev eps [nc][ne], h_k [nc][nt][ne], stress [nc][ne]
    hipEvent_t ev[8] = {};               // (start, stop) of the table launch and of the three passes: created once, on first use
    ~fs_visco_state_s() {
        for (hipEvent_t e_ : ev)
            if (e_) (void)hipEventDestroy(e_);
    }
};

struct visco_terms {                     // the constant material's series, by value
    double g[FS_VISCO_MAX_TERMS];
    double tau[FS_VISCO_MAX_TERMS];
};

// (a, b) of one term.  Contraction is off so that every caller rounds alike.
__device__ __forceinline__ void visco_ab(double dt, double tau, double& a, double& b) {
#pragma clang fp contract(off)
    const double x = dt / tau;
    a = exp(-x);
    if (x < FS_VISCO_SERIES_X)
        b = 1.0 - x * (0.5 - x * ((1.0 / 6.0) - x * (1.0 / 24.0)));
    else
        b = -expm1(-x) / x;
}

__global__ void k_visco_coef(int nt, const visco_terms tm, double dt, double* __restrict__ coef) {
    const int k = threadIdx.x;
    if (blockIdx.x != 0 || k >= nt) return;
    double a, b;
    visco_ab(dt, tm.tau[k], a, b);
    coef[2 * k] = a;
    coef[2 * k + 1] = b;
}

// ---- per-cell update -------------------------------------------------------------------------------------------------------
// mat[nc][2 + 2 nt] = (G0, lambda0, g_1, tau_1, ...) with CELL, else (mu0, lambda0, tm) and the (a_k, b_k) table coef
template <int TD, bool CELL>
__global__ void __launch_bounds__(FS_BLOCK) k_visco_update(int64_t nc, const int32_t* __restrict__ cells, const double* __restrict__ xyz4,
                                                           const double* __restrict__ u, double mu0, double lambda0, int nt,
                                                           const visco_terms tm, const double* __restrict__ coef, double dt,
                                                           const double* __restrict__ mat, const box_snap bx,
                                                           const double* __restrict__ e0, const double* __restrict__ h0,
                                                           double* __restrict__ e1, double* __restrict__ h1, double* __restrict__ sig,
                                                           int64_t* __restrict__ part) {
    constexpr int NE = TD == 3 ? 6 : 4;
    int64_t n_bad[1] = {0}, first = INT64_MAX;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int ms = 2 + 2 * nt;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += stride) {
        const int4 v4 = reinterpret_cast<const int4*>(cells)[c];
        double mu = mu0, lambda = lambda0;
        const double2* mc = reinterpret_cast<const double2*>(mat + (CELL ? (int64_t)ms * c : 0));
        if (CELL) {
            const double2 m0 = mc[0];
            mu = m0.x; lambda = m0.y;
        }
        // strain of the P1 displacement, in the storage order of the file header
        double ed[NE];
        p1_strain<TD>(v4, xyz4, u, bx, ed);
        double sg[NE];
        {
#pragma clang fp contract(off)
            const double tr = ed[0] + ed[1] + ed[2];
            const double bulk = lambda + (2.0 / 3.0) * mu;
#pragma unroll
            for (int j = 0; j < 3; ++j) ed[j] -= tr * (1.0 / 3.0);
            double de[NE], acc[NE];
            const double2* ec = reinterpret_cast<const double2*>(e0 + NE * c);
#pragma unroll
            for (int j = 0; j < NE; j += 2) {
                const double2 x = ec[j >> 1];
                de[j] = ed[j] - x.x; de[j + 1] = ed[j + 1] - x.y;
                acc[j] = 0.0; acc[j + 1] = 0.0;
            }
            double gsum = 0.0;
            for (int k = 0; k < nt; ++k) {
                double g, a, b;
                if (CELL) {
                    const double2 gt = mc[1 + k];
                    g = gt.x;
                    visco_ab(dt, gt.y, a, b);
                } else {
                    g = tm.g[k];
                    a = coef[2 * k]; b = coef[2 * k + 1];
                }
                gsum += g;
                const double2* hc = reinterpret_cast<const double2*>(h0 + ((int64_t)nt * c + k) * NE);
                double2* hn = reinterpret_cast<double2*>(h1 + ((int64_t)nt * c + k) * NE);
#pragma unroll
                for (int j = 0; j < NE; j += 2) {
                    const double2 x = hc[j >> 1];
                    const double y0 = a * x.x + b * de[j], y1 = a * x.y + b * de[j + 1];
                    hn[j >> 1] = make_double2(y0, y1);
                    acc[j] += g * y0; acc[j + 1] += g * y1;
                }
            }
            const double ginf = 1.0 - gsum;
            bool ok = true;
#pragma unroll
            for (int j = 0; j < NE; ++j) {
                sg[j] = 2.0 * mu * (ginf * ed[j] + acc[j]) + (j < 3 ? bulk * tr : 0.0);
                ok = ok && isfinite(sg[j]);
            }
            if (!ok) {
                ++n_bad[0];
                first = c < first ? c : first;
            }
        }
        double2* eo = reinterpret_cast<double2*>(e1 + NE * c);
        double2* so = reinterpret_cast<double2*>(sig + NE * c);
#pragma unroll
        for (int j = 0; j < NE; j += 2) {
            eo[j >> 1] = make_double2(ed[j], ed[j + 1]);
            so[j >> 1] = make_double2(sg[j], sg[j + 1]);
        }
    }
    p1_cell_tally<1, false>(n_bad, first, 0.0, part, nullptr);
}

// ---- the history load --------------------------------------------------------------------------------------------------------
// s_hist = 2 G0 sum_k g_k (a_k h_k - b_k e) of cell c from the committed state
template <int NE, bool CELL>
__device__ __forceinline__ void visco_s_hist(int64_t c, double mu0, int nt, const visco_terms& tm, const double* __restrict__ coef, double dt,
                                             const double* __restrict__ mat, const double* __restrict__ e0, const double* __restrict__ h0,
                                             double* __restrict__ s) {
#pragma clang fp contract(off)
    const double2* mc = reinterpret_cast<const double2*>(mat + (CELL ? (int64_t)(2 + 2 * nt) * c : 0));
    const double mu = CELL ? mc[0].x : mu0;
    double ec[NE], acc[NE];
    const double2* ep = reinterpret_cast<const double2*>(e0 + NE * c);
#pragma unroll
    for (int j = 0; j < NE; j += 2) {
        const double2 x = ep[j >> 1];
        ec[j] = x.x; ec[j + 1] = x.y;
        acc[j] = 0.0; acc[j + 1] = 0.0;
    }
    for (int k = 0; k < nt; ++k) {
        double g, a, b;
        if (CELL) {
            const double2 gt = mc[1 + k];
            g = gt.x;
            visco_ab(dt, gt.y, a, b);
        } else {
            g = tm.g[k];
            a = coef[2 * k]; b = coef[2 * k + 1];
        }
        const double2* hc = reinterpret_cast<const double2*>(h0 + ((int64_t)nt * c + k) * NE);
#pragma unroll
        for (int j = 0; j < NE; j += 2) {
            const double2 x = hc[j >> 1];
            acc[j] += g * (a * x.x - b * ec[j]);
            acc[j + 1] += g * (a * x.y - b * ec[j + 1]);
        }
    }
#pragma unroll
    for (int j = 0; j < NE; ++j) s[j] = 2.0 * mu * acc[j];
}

// f = -int B^T s_hist dx
template <int TD, bool CELL, bool ADD>
__global__ void __launch_bounds__(FS_BLOCK) k_visco_gather(int64_t n_rows, const int64_t* __restrict__ slice_ptr,
                                                           const int32_t* __restrict__ sell_col, const int32_t* __restrict__ gptr,
                                                           const int32_t* __restrict__ gsrc, const int32_t* __restrict__ cells,
                                                           const double* __restrict__ xyz4, const box_snap bx, double mu0, int nt,
                                                           const visco_terms tm, const double* __restrict__ coef, double dt,
                                                           const double* __restrict__ mat, const double* __restrict__ e0,
                                                           const double* __restrict__ h0, double* __restrict__ f) {
    constexpr int NE = TD == 3 ? 6 : 4;
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; r < n_rows; r += stride) {
        double acc[TD];
#pragma unroll
        for (int i = 0; i < TD; ++i) acc[i] = 0.0;
        const int64_t e = p1_diag_entry(r, slice_ptr, sell_col);
        if (e >= 0) {
            const int32_t q1 = gptr[e + 1];
            for (int32_t q = gptr[e]; q < q1; ++q) {
                int64_t c;
                int a, b;
                p1_source<TD>(gsrc[q], c, a, b);
                const int4 v4 = reinterpret_cast<const int4*>(cells)[c];
                double s[NE], ga[TD], w[TD], vol;
                visco_s_hist<NE, CELL>(c, mu0, nt, tm, coef, dt, mat, e0, h0, s);
                p1_weighted_grad<TD>(v4, xyz4, bx, a, ga, vol);
                p1_sym_mul<TD>(s, ga, w);
#pragma unroll
                for (int i = 0; i < TD; ++i) acc[i] -= vol * w[i];
            }
        }
#pragma unroll
        for (int i = 0; i < TD; ++i) f[TD * r + i] = ADD ? f[TD * r + i] + acc[i] : acc[i];
    }
}

// ---- host side: the history object ---------------------------------------------------------------------------------------
extern "C" int fs_visco_state_create(fs_space_t space, int n_terms, fs_visco_state_t* out) {
    FS_CHECK(fs_require_init());
    FS_REQUIRE(out, "fs_visco_state_create: null pointer");
    FS_CHECK(fs_require_vector_cg1(space, "fs_visco_state_create"));
    FS_REQUIRE(n_terms >= 0 && n_terms <= FS_VISCO_MAX_TERMS, "fs_visco_state_create: %d Prony terms: 0 to FS_VISCO_MAX_TERMS = %d are "
               "supported", n_terms, FS_VISCO_MAX_TERMS);
    fs_visco_state_s* st = new fs_visco_state_s();
    st->bind(space);
    st->nt = n_terms;
    const int64_t ne = st->nc * st->ne;
    const int64_t nh = ne * (n_terms > 0 ? n_terms : 1);          // (never an empty allocation)
    int rc = FS_OK;
    if ((rc = st->e.alloc(ne)) || (rc = st->sig.alloc(ne)) || (rc = st->h.alloc(nh))) {
        delete st;
        return rc;
    }
    *out = st;
    rc = fs_visco_state_reset(st);
    if (rc != FS_OK) { delete st; *out = nullptr; }
    return rc;
}

extern "C" int fs_visco_state_destroy(fs_visco_state_t st) {
    delete st;
    return FS_OK;
}

extern "C" int fs_visco_state_reset(fs_visco_state_t st) {
    FS_REQUIRE(st, "fs_visco_state_reset: null pointer");
    hipStream_t s = fs_rt().stream;
    FS_CHECK(st->e.zero(s)); FS_CHECK(st->h.zero(s)); FS_CHECK(st->sig.zero(s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

extern "C" int fs_visco_state_commit(fs_visco_state_t st) {
    FS_REQUIRE(st, "fs_visco_state_commit: null pointer");
    hipStream_t s = fs_rt().stream;
    FS_CHECK(st->e.commit(s)); FS_CHECK(st->sig.commit(s));
    if (st->nt) FS_CHECK(st->h.commit(s));               // (without terms h is one unused record per cell)
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

extern "C" int fs_visco_state_get(fs_visco_state_t st, int which, double* e, double* h, double* stress) {
    FS_REQUIRE(st, "fs_visco_state_get: null pointer");
    FS_REQUIRE(which == FS_VISCO_COMMITTED || which == FS_VISCO_TRIAL, "fs_visco_state_get: which is FS_VISCO_COMMITTED or FS_VISCO_TRIAL");
    hipStream_t s = fs_rt().stream;
    const bool tr = which == FS_VISCO_TRIAL;
    if (e) FS_CHECK(st->e.pick(tr).download(e, st->nc * st->ne, s));
    if (h && st->nt) FS_CHECK(st->h.pick(tr).download(h, st->nc * st->ne * st->nt, s));
    if (stress) FS_CHECK(st->sig.pick(tr).download(stress, st->nc * st->ne, s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

extern "C" int fs_visco_state_set(fs_visco_state_t st, const double* e, const double* h) {
    FS_REQUIRE(st && e && (h || st->nt == 0), "fs_visco_state_set: null pointer");
    for (int64_t c = 0; c < st->nc; ++c) {
        bool ok = true;
        for (int j = 0; j < st->ne; ++j) ok = ok && isfinite(e[c * st->ne + j]);
        for (int64_t j = 0; j < (int64_t)st->ne * st->nt; ++j) ok = ok && isfinite(h[c * st->ne * st->nt + j]);
        FS_REQUIRE(ok, "fs_visco_state_set: cell %lld (device order) has a non-finite strain", (long long)c);
    }
    hipStream_t s = fs_rt().stream;
    FS_CHECK(st->e.committed.upload(e, st->nc * st->ne, s));
    if (st->nt) FS_CHECK(st->h.committed.upload(h, st->nc * st->ne * st->nt, s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

// ---- host side: the assembly ---------------------------------------------------------------------------------------------
// one material record (G0, lambda0, (g_k, tau_k)...): the message names the cell when there is one (c >= 0)
static int visco_material_ok(double mu, double lambda, int nt, const double* gt, long long c) {
    char where[64] = "";
    if (c >= 0) snprintf(where, sizeof where, "cell %lld (device order): ", c);
    FS_REQUIRE(mu > 0.0 && isfinite(mu) && isfinite(lambda) && lambda + (2.0 / 3.0) * mu > 0.0,
               "fs_assemble_viscoelastic: %smu = %g, lambda = %g: mu > 0 and a bulk modulus lambda + 2/3 mu > 0 are required", where, mu, lambda);
    double gsum = 0.0;
    for (int k = 0; k < nt; ++k) {
        const double g = gt[2 * k], tau = gt[2 * k + 1];
        FS_REQUIRE(g > 0.0 && isfinite(g) && tau > 0.0 && isfinite(tau), "fs_assemble_viscoelastic: %sProny term %d has relative modulus %g and "
                   "relaxation time %g: both must be positive", where, k, g, tau);
        gsum += g;
    }
    FS_REQUIRE(gsum < 1.0, "fs_assemble_viscoelastic: %sthe relative moduli sum to %g: sum g_k < 1 is required (g_inf = 1 - sum g_k > 0)", where,
               gsum);
    return FS_OK;
}

extern "C" int fs_assemble_viscoelastic(fs_space_t space, fs_vector_t r, fs_vector_t u, fs_visco_state_t state, const fs_visco_form* form,
                                        int what, fs_visco_info* info) {
    FS_REFUSE_DG_SPACE(space, "fs_assemble_viscoelastic");
    FS_REQUIRE(space && form && state, "fs_assemble_viscoelastic: null pointer");
    FS_REQUIRE((what & ~(FS_VISCO_LOAD | FS_VISCO_UPDATE | FS_VISCO_FORCE)) == 0, "fs_assemble_viscoelastic: unknown bits in what (%d)", what);
    FS_REQUIRE(!((what & FS_VISCO_LOAD) && (what & FS_VISCO_FORCE)), "fs_assemble_viscoelastic: FS_VISCO_LOAD and FS_VISCO_FORCE write the "
               "same vector: one of them per call");
    FS_CHECK(fs_require_solid_space(space, "fs_assemble_viscoelastic"));
    fs_space_s* sp = space;
    fs_mesh_s* m = sp->mesh;
    FS_REQUIRE(state->owns(sp, m), "fs_assemble_viscoelastic: the history belongs to another space");
    const int nt = form->n_terms;
    FS_REQUIRE(nt >= 0 && nt <= FS_VISCO_MAX_TERMS, "fs_assemble_viscoelastic: %d Prony terms: at most FS_VISCO_MAX_TERMS = %d are supported",
               nt, FS_VISCO_MAX_TERMS);
    FS_REQUIRE(nt == state->nt, "fs_assemble_viscoelastic: the form has %d Prony terms, the history was created for %d", nt, state->nt);
    FS_REQUIRE(form->dt > 0.0 && isfinite(form->dt), "fs_assemble_viscoelastic: the step length is %g: dt > 0 and finite is required", form->dt);
    FS_REQUIRE(!(what & FS_VISCO_UPDATE) || (u && u->d.n >= sp->n_dofs_local), "fs_assemble_viscoelastic: the update needs a displacement "
               "vector of the space's dofs");
    FS_REQUIRE(!(what & (FS_VISCO_LOAD | FS_VISCO_FORCE)) || (r && r->d.n >= sp->n_dofs_owned), "fs_assemble_viscoelastic: the history load "
               "and the internal force need a vector of the space's owned dofs");
    FS_REQUIRE(form->material.mode == FS_COEF_NONE || form->material.mode == FS_COEF_CELL_VISCO,
               "fs_assemble_viscoelastic: the material is FS_COEF_NONE (mu, lambda, g[], tau[]) or FS_COEF_CELL_VISCO");
    const bool cellw = form->material.mode == FS_COEF_CELL_VISCO;
    const int ms = 2 + 2 * nt;
    hipStream_t s = fs_rt().stream;
    dbuf<double> mstore, coef;
    hipEvent_t* ev = state->ev;                     // owned by the history object: an early return leaks nothing
    if (info)
        for (int i = 0; i < 8; ++i)
            if (!ev[i]) FS_HIP(hipEventCreate(&ev[i]));
#define FS_VT(I_) do { if (info) FS_HIP(hipEventRecord(ev[I_], s)); } while (0)
    visco_terms tm;
    for (int k = 0; k < FS_VISCO_MAX_TERMS; ++k) { tm.g[k] = k < nt ? form->g[k] : 0.0; tm.tau[k] = k < nt ? form->tau[k] : 1.0; }
    if (cellw) {
        FS_REQUIRE(form->material.data, "fs_assemble_viscoelastic: per-cell material data pointer is null");
        for (int64_t c = 0; c < m->nc; ++c) {
            const double* mc = form->material.data + (int64_t)ms * c;
            FS_CHECK(visco_material_ok(mc[0], mc[1], nt, mc + 2, (long long)c));
        }
        FS_CHECK(fs_upload_cell_rows(mstore, form->material.data, ms, m->nc, s));
    } else {
        double gt[2 * FS_VISCO_MAX_TERMS];
        for (int k = 0; k < nt; ++k) { gt[2 * k] = form->g[k]; gt[2 * k + 1] = form->tau[k]; }
        FS_CHECK(visco_material_ok(form->mu, form->lambda, nt, gt, -1));
        FS_CHECK(coef.alloc(2 * FS_VISCO_MAX_TERMS));
        FS_CHECK(coef.zero(s));
        if (nt) {
            FS_VT(0);
            hipLaunchKernelGGL(k_visco_coef, dim3(1), dim3(64), 0, s, nt, tm, form->dt, coef.p);
            FS_KERNEL_CHECK();
            FS_VT(1);
        }
    }
    FS_CHECK(p1_gather_map(sp, s));          // ahead of the passes, outside the events that time them
    const box_snap bx = make_box_snap(m);
    fs_cell_tally<1, false> tally;
    int rc = FS_OK;
    // 1. the history load, from the committed state
    if (what & FS_VISCO_LOAD) {
        FS_VT(2);
        fs_dispatch_int<3, 2>(m->tdim, [&](auto TD) {
            fs_dispatch_bool(cellw, [&](auto CELL) {
                fs_dispatch_bool(form->add != 0, [&](auto ADD) {
                    rc = p1_launch_nodes(sp, s, k_visco_gather<decltype(TD)::value, decltype(CELL)::value, decltype(ADD)::value>, bx, form->mu, nt, tm,
                                         coef.p, form->dt, mstore.p, state->e.committed.p, state->h.committed.p, r->d.p);
                });
            });
        });
        FS_CHECK(rc);
        FS_VT(3);
    }
    // 2. the update, once per cell
    if (what & FS_VISCO_UPDATE) {
        FS_CHECK(tally.alloc());
        FS_VT(4);
        fs_dispatch_int<3, 2>(m->tdim, [&](auto TD) {
            fs_dispatch_bool(cellw, [&](auto CELL) {
                hipLaunchKernelGGL((k_visco_update<decltype(TD)::value, decltype(CELL)::value>), dim3(tally.nb), dim3(FS_BLOCK), 0, s, m->nc, m->cells.p,
                                   m->xyz.p, u->d.p, form->mu, form->lambda, nt, tm, coef.p, form->dt, mstore.p, bx, state->e.committed.p,
                                   state->h.committed.p, state->e.trial.p, state->h.trial.p, state->sig.trial.p, tally.part.p);
            });
        });
        FS_CHECK(tally.finish(s));
        FS_VT(5);
    }
    // 3. the internal force of the trial stress
    if (what & FS_VISCO_FORCE) {
        FS_VT(6);
        fs_dispatch_int<3, 2>(m->tdim, [&](auto TD) {
            fs_dispatch_bool(form->add != 0, [&](auto ADD) {
                rc = p1_launch_nodes(sp, s, k_p1_stress_force_gather<decltype(TD)::value, decltype(ADD)::value>, state->sig.trial.p, bx, r->d.p);
            });
        });
        FS_CHECK(rc);
        FS_VT(7);
    }
#undef FS_VT
    if (info) {
        info->n_nonfinite = 0;
        info->first_nonfinite_cell = -1;
        if (what & FS_VISCO_UPDATE) {
            FS_CHECK(tally.get(s));
            info->n_nonfinite = tally.n[0];
            info->first_nonfinite_cell = fs_first_cell(m, tally.n[0], tally.n[1]);
        }
    }
    FS_HIP(hipStreamSynchronize(s));
    if (info) {
        const int bit[3] = {FS_VISCO_LOAD, FS_VISCO_UPDATE, FS_VISCO_FORCE};
        double* ms[3] = {&info->load_ms, &info->update_ms, &info->force_ms};
        float tc = 0.0f;                                 // the (a_k, b_k) table launch belongs to the passes that read it
        if (!cellw && nt) FS_HIP(hipEventElapsedTime(&tc, ev[0], ev[1]));
        for (int i = 0; i < 3; ++i) {
            float t = 0.0f;
            if (what & bit[i]) FS_HIP(hipEventElapsedTime(&t, ev[2 * i + 2], ev[2 * i + 3]));
            *ms[i] = (what & bit[i]) ? t + (i < 2 ? tc : 0.0f) : 0.0;
        }
    }
    return FS_OK;
}
