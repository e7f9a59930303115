// Small-strain von Mises (J2) plasticity with linear isotropic hardening on vector CG1 spaces (tetrahedra, and triangles in plane
// strain): the return mapping with its per-cell history, the consistent tangent and the internal force, on the device.
//
// The reference names a PlasticitySolver (Readme.md, the docstring of LinearElasticitySolver.py) and never delivers one; the model
// is the textbook radial return.  A P1 displacement has a constant strain per cell, so the cell is the integration point:
//   eps = sym grad u,  e = eps - eps_p,  sigma_tr = K tr(e) I + 2 G dev(e),  s = dev sigma_tr,  q = sqrt(3/2) |s|,
//   f = q - (sigma_y + H p);   f <= 0: elastic;   f > 0: dp = f / (3 G + H), N = s / |s|, beta = 3 G dp / q,
//   sigma = sigma_tr - 2 G dp sqrt(3/2) N,  eps_p += sqrt(3/2) dp N,  p += dp,
//   D = C - 2 G beta I_dev - 2 G (3G/(3G+H) - beta) N (x) N
//     = lambda' I (x) I + 2 mu' I_sym - c N (x) N   with  mu' = G (1 - beta),  lambda' = lambda + 2/3 G beta.
// D has the shape of the elastic operator with (mu', lambda') plus one rank-one term, so the tangent block of the linear kernel
// carries over:  K_ab[i][k] = V (lambda' g_a[i] g_b[k] + mu' g_a[k] g_b[i] + delta_ik mu' g_a . g_b) - V c (N g_a)[i] (N g_b)[k].
//
// Kernels (no atomics anywhere: two assemblies of one state give the same bits):
//   k_plastic_cells                       one thread per cell, ONCE per evaluation: strain, trial state, return mapping.  Writes the
//       trial history (eps_p, p), the returned stress and the tangent record (mu', lambda', c, N); counts the yielded and the
//       non-finite cells per workgroup (p1_cell_tally; k_cell_tally_finish sums the partials in a fixed order).
//   k_plastic_tangent_gather / _tri_gather  one thread per STORED block sums its (cell, a, b) sources of the inverse slot table in
//       ascending order - the walk of k_assemble_p1_elasticity_gather - and reads the cell's record instead of a material pair.  The
//       elastic-shaped part is accumulated by the linear kernel's expression, the rank-one part in an accumulator of its own that
//       stays +0 while no source cell has yielded: the tangent then equals fs_assemble_matrix of the linear operator bit for bit.
//   k_p1_stress_force_gather (fs_p1_cell.h)  one thread per owned node over the cells around it (the sources of its diagonal
//       block, ascending): V sigma g_a from the stored stress.
//
// Tensor storage: 3-D (xx, yy, zz, xy, xz, yz), plane strain (xx, yy, zz, xy) - tensor components, not engineering shears.
#include "fs_common.h"
#include "fs_kernels.h"
#include "fs_p1_cell.h"
#include <math.h>

#define FS_PLASTIC_REC3 10               // doubles per cell of the 3-D tangent record: mu', lambda', c, 0, N[6]
#define FS_PLASTIC_REC2 6                // plane strain: mu', lambda', c, Nxx, Nyy, Nxy

struct fs_plastic_state_s : fs_cell_history {      // ne: the stored components of eps_p and sigma
    fs_history_pair ep, p, sig;          // plastic strain [nc][ne], cumulative plastic strain [nc], returned stress [nc][ne]
    dbuf<double> rec;                    // tangent record of the last evaluation
};

// ---- per-cell return mapping ---------------------------------------------------------------------------------------------
// mat[nc][4] = (mu, lambda, sigma_y, H) with CELL, else the four constants
template <int TD, bool CELL>
__global__ void __launch_bounds__(FS_BLOCK) k_plastic_cells(int64_t nc, const int32_t* __restrict__ cells, const double* __restrict__ xyz4,
                                                            const double* __restrict__ u, double mu0, double lambda0, double sy0, double h0,
                                                            const double* __restrict__ mat, const box_snap bx,
                                                            const double* __restrict__ ep0, const double* __restrict__ p0,
                                                            double* __restrict__ ep1, double* __restrict__ p1, double* __restrict__ sig,
                                                            double* __restrict__ rec, int64_t* __restrict__ part) {
    constexpr int NE = TD == 3 ? 6 : 4;
    int64_t n[2] = {0, 0}, first = INT64_MAX;      // yielded, non-finite
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += stride) {
        const int4 v4 = reinterpret_cast<const int4*>(cells)[c];
        double mu = mu0, lambda = lambda0, sy = sy0, hm = h0;
        if (CELL) {
            const double2 m0 = reinterpret_cast<const double2*>(mat)[2 * c], m1 = reinterpret_cast<const double2*>(mat)[2 * c + 1];
            mu = m0.x; lambda = m0.y; sy = m1.x; hm = m1.y;
        }
        // elastic strain e = sym grad u - eps_p, in the storage order of the file header
        double e[NE];
        p1_strain<TD>(v4, xyz4, u, bx, e);
        double epc[NE];
#pragma unroll
        for (int k = 0; k < NE; ++k) { epc[k] = ep0[NE * c + k]; e[k] -= epc[k]; }
        const double pc = p0[c];
        const double tr = e[0] + e[1] + e[2];
        const double bulk = lambda + (2.0 / 3.0) * mu;
        double s[NE];
#pragma unroll
        for (int k = 0; k < NE; ++k) s[k] = 2.0 * mu * (k < 3 ? e[k] - tr * (1.0 / 3.0) : e[k]);
        double ss = s[0] * s[0] + s[1] * s[1] + s[2] * s[2];
#pragma unroll
        for (int k = 3; k < NE; ++k) ss += 2.0 * s[k] * s[k];
        const double sn = sqrt(ss);
        const double r32 = 1.224744871391589049;          // sqrt(3/2)
        const double q = r32 * sn;
        const double f = q - (sy + hm * pc);
        double sg[NE];
#pragma unroll
        for (int k = 0; k < NE; ++k) sg[k] = s[k] + (k < 3 ? bulk * tr : 0.0);
        double mu_t = mu, lambda_t = lambda, cn = 0.0, pn = pc;
        double N[NE];
#pragma unroll
        for (int k = 0; k < NE; ++k) N[k] = 0.0;
        if (!isfinite(f)) {
            ++n[1];
            first = c < first ? c : first;
        } else if (f > 0.0) {
            ++n[0];
            const double dp = f / (3.0 * mu + hm);
            const double beta = 3.0 * mu * dp / q;
            const double inv = 1.0 / sn;
#pragma unroll
            for (int k = 0; k < NE; ++k) {
                N[k] = s[k] * inv;
                sg[k] -= 2.0 * mu * dp * r32 * N[k];
                epc[k] += r32 * dp * N[k];
            }
            pn = pc + dp;
            mu_t = mu * (1.0 - beta);
            lambda_t = lambda + (2.0 / 3.0) * mu * beta;
            cn = 2.0 * mu * (3.0 * mu / (3.0 * mu + hm) - beta);
        }
#pragma unroll
        for (int k = 0; k < NE; ++k) { ep1[NE * c + k] = epc[k]; sig[NE * c + k] = sg[k]; }
        p1[c] = pn;
        if (TD == 3) {
            double2* rc = reinterpret_cast<double2*>(rec + FS_PLASTIC_REC3 * c);
            rc[0] = make_double2(mu_t, lambda_t);
            rc[1] = make_double2(cn, 0.0);
            rc[2] = make_double2(N[0], N[1]);
            rc[3] = make_double2(N[2], N[3]);
            rc[4] = make_double2(N[NE - 2], N[NE - 1]);
        } else {
            double2* rc = reinterpret_cast<double2*>(rec + FS_PLASTIC_REC2 * c);
            rc[0] = make_double2(mu_t, lambda_t);
            rc[1] = make_double2(cn, N[0]);
            rc[2] = make_double2(N[1], N[3]);
        }
    }
    p1_cell_tally<2, false>(n, first, 0.0, part, nullptr);
}

// ---- tangent: tetrahedra -------------------------------------------------------------------------------------------------
// Same source walk as k_assemble_p1_elasticity_gather (source index = cell * 16 + a * 4 + b, groups of four with their cell
// records fetched first).  ms0 is the linear kernel's mass term, passed as a run-time 0 so that the diagonal sum below is the
// same expression (and the same rounding) as there.  N is fetched for yielded cells only (c != 0).
template <bool ADD>
__global__ void __launch_bounds__(FS_BLOCK) k_plastic_tangent_gather(int64_t n_entries, const int32_t* __restrict__ ptr,
                                                                     const int32_t* __restrict__ src, const int32_t* __restrict__ cells,
                                                                     const double* __restrict__ xyz4, const double* __restrict__ rec,
                                                                     double ms0, int64_t plane, double* __restrict__ val, const box_snap bx) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; e < n_entries; e += stride) {
        double acc[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        double accn[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        const int32_t q1 = ptr[e + 1];
        constexpr int PF = 4;
        for (int32_t q0 = ptr[e]; q0 < q1; q0 += PF) {
          int32_t sc[PF];
          int4 vc[PF];
          double2 lc[PF], cc[PF];
#pragma unroll
          for (int w = 0; w < PF; ++w) sc[w] = q0 + w < q1 ? src[q0 + w] : -1;
#pragma unroll
          for (int w = 0; w < PF; ++w) {
            vc[w] = sc[w] >= 0 ? reinterpret_cast<const int4*>(cells)[p1_source_cell<3>(sc[w])] : make_int4(0, 0, 0, 0);
            const double2* rc = reinterpret_cast<const double2*>(rec + (int64_t)FS_PLASTIC_REC3 * (sc[w] >= 0 ? p1_source_cell<3>(sc[w]) : 0));
            lc[w] = sc[w] >= 0 ? rc[0] : make_double2(0.0, 0.0);
            cc[w] = sc[w] >= 0 ? rc[1] : make_double2(0.0, 0.0);
          }
#pragma unroll
          for (int w = 0; w < PF; ++w) {
            if (q0 + w >= q1) break;
            int64_t c;
            int a, b;
            p1_source<3>(sc[w], c, a, b);
            const int4 v4 = vc[w];
            const double mu = lc[w].x, lambda = lc[w].y;
            const int32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
            const tet_geom t = tet_geometry_box(xyz4, v, bx);
            const double vol = t.adet * (1.0 / 6.0);
            double ga[3], gb[3];
            P1_GRAD_TET(t, a, ga);
            P1_GRAD_TET(t, b, gb);
            const double gg = ga[0] * gb[0] + ga[1] * gb[1] + ga[2] * gb[2];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    double x = vol * (lambda * ga[i] * gb[j] + mu * ga[j] * gb[i]);
                    if (i == j) x += vol * mu * gg + ms0;
                    acc[i][j] += x;
                }
            if (cc[w].x != 0.0) {
                const double2* rc = reinterpret_cast<const double2*>(rec + (int64_t)FS_PLASTIC_REC3 * c);
                const double2 n01 = rc[2], n23 = rc[3], n45 = rc[4];
                const double N[6] = {n01.x, n01.y, n23.x, n23.y, n45.x, n45.y};
                double na[3], nb[3];
                p1_sym_mul<3>(N, ga, na);
                p1_sym_mul<3>(N, gb, nb);
                const double vc_ = vol * cc[w].x;
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) accn[i][j] += vc_ * na[i] * nb[j];
            }
          }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int64_t idx = (int64_t)(i * 3 + j) * plane + e;
                const double x = acc[i][j] - accn[i][j];
                val[idx] = ADD ? val[idx] + x : x;
            }
    }
}

// ---- tangent: triangles (plane strain), source index = cell * 9 + a * 3 + b, as k_assemble_tri_elasticity_gather -------------
template <bool ADD>
__global__ void __launch_bounds__(FS_BLOCK) k_plastic_tangent_tri_gather(int64_t n_entries, const int32_t* __restrict__ ptr,
                                                                         const int32_t* __restrict__ src, const int32_t* __restrict__ cells,
                                                                         const double* __restrict__ xyz4, const double* __restrict__ rec,
                                                                         double ms0, int64_t plane, double* __restrict__ val) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; e < n_entries; e += stride) {
        double acc[2][2] = {{0, 0}, {0, 0}};
        double accn[2][2] = {{0, 0}, {0, 0}};
        const int32_t q1 = ptr[e + 1];
        for (int32_t q = ptr[e]; q < q1; ++q) {
            int64_t c;
            int a, b;
            p1_source<2>(src[q], c, a, b);
            const int4 v4 = reinterpret_cast<const int4*>(cells)[c];
            const double2* rc = reinterpret_cast<const double2*>(rec + FS_PLASTIC_REC2 * c);
            const double2 ml = rc[0], cn = rc[1], n13 = rc[2];
            const double mu = ml.x, lambda = ml.y;
            const tri_geom t = tri_geometry2(xyz4, v4.x, v4.y, v4.z);
            double ga[2], gb[2];
            p1_grad(t, a, ga);
            p1_grad(t, b, gb);
            const double gg = ga[0] * gb[0] + ga[1] * gb[1];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    double x = t.area * (lambda * ga[i] * gb[j] + mu * ga[j] * gb[i]);
                    if (i == j) x += t.area * mu * gg + ms0;
                    acc[i][j] += x;
                }
            const double N[4] = {cn.y, n13.x, 0.0, n13.y};      // (Nxx, Nyy, -, Nxy): the in-plane part
            double na[2], nb[2];
            p1_sym_mul<2>(N, ga, na);
            p1_sym_mul<2>(N, gb, nb);
            const double vc_ = t.area * cn.x;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) accn[i][j] += vc_ * na[i] * nb[j];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int64_t idx = (int64_t)(i * 2 + j) * plane + e;
                const double x = acc[i][j] - accn[i][j];
                val[idx] = ADD ? val[idx] + x : x;
            }
    }
}

// ---- host side: the history object ---------------------------------------------------------------------------------------
extern "C" int fs_plastic_state_create(fs_space_t space, fs_plastic_state_t* out) {
    FS_CHECK(fs_require_init());
    FS_REQUIRE(out, "fs_plastic_state_create: null pointer");
    FS_CHECK(fs_require_vector_cg1(space, "fs_plastic_state_create"));
    fs_plastic_state_s* st = new fs_plastic_state_s();
    st->bind(space);
    const int64_t ne = st->nc * st->ne;
    int rc = FS_OK;
    if ((rc = st->ep.alloc(ne)) || (rc = st->sig.alloc(ne)) || (rc = st->p.alloc(st->nc)) ||
        (rc = st->rec.alloc(st->nc * (st->tdim == 3 ? FS_PLASTIC_REC3 : FS_PLASTIC_REC2)))) {
        delete st;
        return rc;
    }
    *out = st;
    rc = fs_plastic_state_reset(st);
    if (rc != FS_OK) { delete st; *out = nullptr; }
    return rc;
}

extern "C" int fs_plastic_state_destroy(fs_plastic_state_t st) {
    delete st;
    return FS_OK;
}

extern "C" int fs_plastic_state_reset(fs_plastic_state_t st) {
    FS_REQUIRE(st, "fs_plastic_state_reset: null pointer");
    hipStream_t s = fs_rt().stream;
    FS_CHECK(st->ep.zero(s)); FS_CHECK(st->p.zero(s)); FS_CHECK(st->sig.zero(s)); FS_CHECK(st->rec.zero(s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

extern "C" int fs_plastic_state_commit(fs_plastic_state_t st) {
    FS_REQUIRE(st, "fs_plastic_state_commit: null pointer");
    hipStream_t s = fs_rt().stream;
    FS_CHECK(st->ep.commit(s)); FS_CHECK(st->sig.commit(s)); FS_CHECK(st->p.commit(s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

extern "C" int fs_plastic_state_get(fs_plastic_state_t st, int which, double* eps_p, double* p, double* stress) {
    FS_REQUIRE(st, "fs_plastic_state_get: null pointer");
    FS_REQUIRE(which == FS_PLASTIC_COMMITTED || which == FS_PLASTIC_TRIAL, "fs_plastic_state_get: which is FS_PLASTIC_COMMITTED or FS_PLASTIC_TRIAL");
    hipStream_t s = fs_rt().stream;
    const bool tr = which == FS_PLASTIC_TRIAL;
    if (eps_p) FS_CHECK(st->ep.pick(tr).download(eps_p, st->nc * st->ne, s));
    if (p) FS_CHECK(st->p.pick(tr).download(p, st->nc, s));
    if (stress) FS_CHECK(st->sig.pick(tr).download(stress, st->nc * st->ne, s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

extern "C" int fs_plastic_state_set(fs_plastic_state_t st, const double* eps_p, const double* p) {
    FS_REQUIRE(st && eps_p && p, "fs_plastic_state_set: null pointer");
    for (int64_t c = 0; c < st->nc; ++c)
        FS_REQUIRE(p[c] >= 0.0 && isfinite(p[c]), "fs_plastic_state_set: cell %lld (device order) has cumulative plastic strain %g: p >= 0 is "
                   "required", (long long)c, p[c]);
    hipStream_t s = fs_rt().stream;
    FS_CHECK(st->ep.committed.upload(eps_p, st->nc * st->ne, s));
    FS_CHECK(st->p.committed.upload(p, st->nc, s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

// ---- host side: the assembly ---------------------------------------------------------------------------------------------
extern "C" int fs_assemble_plasticity(fs_space_t space, fs_matrix_t K, fs_vector_t r, fs_vector_t u, fs_plastic_state_t state,
                                      const fs_plastic_form* form, int what, fs_plastic_info* info) {
    FS_REFUSE_DG_SPACE(space, "fs_assemble_plasticity"); FS_REFUSE_DG(K, "fs_assemble_plasticity");
    FS_REQUIRE(space && u && form && state, "fs_assemble_plasticity: null pointer");
    FS_REQUIRE((what & ~(FS_PLASTIC_TANGENT | FS_PLASTIC_FORCE)) == 0, "fs_assemble_plasticity: unknown bits in what (%d)", what);
    const char* who = "fs_assemble_plasticity";
    FS_CHECK(fs_require_solid_space(space, who));
    fs_space_s* sp = space;
    fs_mesh_s* m = sp->mesh;
    FS_REQUIRE(state->owns(sp, m), "fs_assemble_plasticity: the history belongs to another space");
    FS_CHECK(fs_require_displacement(u, sp, who));
    FS_CHECK(fs_require_tangent_force(what & FS_PLASTIC_TANGENT, K, what & FS_PLASTIC_FORCE, r, sp, who));
    FS_REQUIRE(form->material.mode == FS_COEF_NONE || form->material.mode == FS_COEF_CELL_PLASTIC,
               "fs_assemble_plasticity: the material is FS_COEF_NONE (mu, lambda, yield_stress, hardening) or FS_COEF_CELL_PLASTIC");
    const bool cellw = form->material.mode == FS_COEF_CELL_PLASTIC;
    hipStream_t s = fs_rt().stream;
    dbuf<double> mstore;
    if (cellw) {
        FS_REQUIRE(form->material.data, "fs_assemble_plasticity: per-cell material data pointer is null");
        for (int64_t c = 0; c < m->nc; ++c) {
            const double* mc = form->material.data + 4 * c;
            FS_REQUIRE(mc[0] > 0.0 && mc[1] >= 0.0 && mc[2] > 0.0 && mc[3] >= 0.0 && isfinite(mc[0]) && isfinite(mc[1]) && isfinite(mc[2]) &&
                       isfinite(mc[3]), "fs_assemble_plasticity: cell %lld (device order) has mu = %g, lambda = %g, yield stress = %g, hardening "
                       "= %g: mu > 0, lambda >= 0, yield stress > 0 and hardening >= 0 are required", (long long)c, mc[0], mc[1], mc[2], mc[3]);
        }
        FS_CHECK(fs_upload_cell_rows(mstore, form->material.data, 4, m->nc, s));
    } else {
        FS_REQUIRE(form->mu > 0.0 && form->lambda >= 0.0 && form->yield_stress > 0.0 && form->hardening >= 0.0 && isfinite(form->mu) &&
                   isfinite(form->lambda) && isfinite(form->yield_stress) && isfinite(form->hardening),
                   "fs_assemble_plasticity: mu > 0, lambda >= 0, yield stress > 0 and hardening >= 0 are required (mu = %g, lambda = %g, yield "
                   "stress = %g, hardening = %g)", form->mu, form->lambda, form->yield_stress, form->hardening);
    }
    FS_CHECK(p1_gather_map(sp, s));          // ahead of the per-cell pass, the first launch
    const box_snap bx = make_box_snap(m);
    const double ms0 = 0.0;
    fs_cell_tally<2, false> tally;             // yielded, non-finite
    FS_CHECK(tally.alloc());
    int rc = FS_OK;
    fs_dispatch_int<3, 2>(m->tdim, [&](auto TD) {
        constexpr int td = decltype(TD)::value;
        // 1. the return mapping, once per cell
        fs_dispatch_bool(cellw, [&](auto CELL) {
            hipLaunchKernelGGL((k_plastic_cells<td, decltype(CELL)::value>), dim3(tally.nb), dim3(FS_BLOCK), 0, s, m->nc, m->cells.p, m->xyz.p, u->d.p,
                               form->mu, form->lambda, form->yield_stress, form->hardening, mstore.p, bx, state->ep.committed.p,
                               state->p.committed.p, state->ep.trial.p, state->p.trial.p, state->sig.trial.p, state->rec.p, tally.part.p);
        });
        if ((rc = tally.finish(s)) != FS_OK) return;
        fs_dispatch_bool(form->add != 0, [&](auto ADD) {
            constexpr bool a = decltype(ADD)::value;
            // 2. the tangent, per stored block (the tetrahedron's kernel takes the box snap: another name)
            if (what & FS_PLASTIC_TANGENT) {
                if constexpr (td == 3) rc = p1_launch_blocks(sp, s, k_plastic_tangent_gather<a>, state->rec.p, ms0, sp->sell_entries, K->val.p, bx);
                else rc = p1_launch_blocks(sp, s, k_plastic_tangent_tri_gather<a>, state->rec.p, ms0, sp->sell_entries, K->val.p);
            }
            // 3. the internal force, per owned node
            if (rc == FS_OK && (what & FS_PLASTIC_FORCE))
                rc = p1_launch_nodes(sp, s, k_p1_stress_force_gather<td, a>, state->sig.trial.p, bx, r->d.p);
        });
    });
    FS_CHECK(rc);
    if (info) {
        FS_CHECK(tally.get(s));
        info->n_yielded = tally.n[0];
        info->n_nonfinite = tally.n[1];
        info->first_nonfinite_cell = fs_first_cell(m, tally.n[1], tally.n[2]);
    }
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}
