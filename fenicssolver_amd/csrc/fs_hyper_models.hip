// St Venant-Kirchhoff, Mooney-Rivlin and Yeoh hyperelasticity on vector CG1 spaces (tetrahedra, and triangles in true plane strain):
// tangent, internal force, energy and inverted-cell tally behind fs_assemble_hyperelastic for every model but the neo-Hookean one
// (fs_hyper.hip keeps that: its expression order and its bits), and the Cauchy stress per cell of all four (fs_hyper_stress).
// None of the three has a counterpart in FenicsSolver/NonlinearElasticitySolver.py.
//
// The material is written once, in invariant form psi = W(I1, I2, J), I1 = tr C, I2 = 1/2 (I1^2 - tr C^2), J = det F.  With
//   dI1/dF = 2 F,   dI2/dF = 2 (I1 F - B F),   dJ/dF = cof F            (B = F F^T)
// and g_a the reference gradient of the barycentric function a, the three vectors a_p = (dI_p/dF) g_a (b_p for g_b) give
//   force     f_a[i]     = V (W_1 a_1 + W_2 a_2 + W_J a_3)[i]
//   tangent   K_ab[i][k] = V ( sum_pq W_pq a_p[i] b_q[k]
//                              + W_1 2 (g_a.g_b) d_ik
//                              + W_2 (4 Fa_i Fb_k - 2 Fb_i Fa_k + (2 I1 g_a.g_b - 2 Fa.Fb) d_ik - 2 B_ik g_a.g_b)      Fa = F g_a
//                              + W_J eps_ikm (F (g_a x g_b))_m )
//   Cauchy    sigma      = (2/J) (W_1 + W_2 I1) B - (2/J) W_2 B^2 + W_J I
// A model is a device functor that returns the nine numbers W_1, W_2, W_J, W_11, W_12, W_1J, W_22, W_2J, W_JJ (and psi); it is a
// TEMPLATE parameter of every kernel, as ADD and CELL are, so the parameter row stays in registers (a run-time switch over rows
// indexed at run time would put them in scratch).  Parameter row p[4] (constant, or one row per cell in device cell order):
//   m_svk   (mu, lambda, -, -)       psi = lambda/2 (tr E)^2 + mu E:E = lambda/8 (I1 - 3)^2 + mu/4 (I1^2 - 2 I2 - 2 I1 + 3)
//   m_mooney(c10, c01, kappa, -)     psi = c10 (J^-2/3 I1 - 3) + c01 (J^-4/3 I2 - 3) + kappa/2 (J - 1)^2
//   m_yeoh  (c10, c20, c30, kappa)   psi = sum_k ck0 (J^-2/3 I1 - 3)^k + kappa/2 (J - 1)^2
//   m_neo   (mu, lambda, -, -)       stress only: W_1 = mu/2, W_J = (lambda ln J - mu) / J
// 2-D is plane strain: F is embedded in 3 x 3 with F33 = 1 and g_a[2] = 0, the same code runs with TD = 2 and the compiler folds the
// constants; only the in-plane rows and columns of the block are formed.  psi(I) = 0 in both dimensions.
//
// Kernels (no atomics; the rules of fs_hyper.hip): the gathers RECOMPUTE the cell state per source, as the neo-Hookean gathers do.
// A per-cell pre-pass would have to store F, B, cof F and the nine W (36 doubles, 288 B) for every source to read, against the
// 4 vertex records, 4 displacements and the cell record (64 B + the parameter row) the recomputation reads; that variant was not
// built, so the choice rests on this count and not on a measured comparison.
//   k_hm_tangent<M, TD, ADD, CELL>  thread per stored block over the sources of the inverse slot table, ascending
//   k_hm_force<M, TD, ADD, CELL>    thread per owned node over the sources of its diagonal block
//   k_hm_cells<M, TD, CELL, false>  V psi and the cells with J <= 0 or J not finite -> p1_cell_tally, k_cell_tally_finish
//   k_hm_cells<M, TD, CELL, true>   sigma per cell (6 or 4 values, tensor storage of fs_p1_cell.h) and the same tally
// Resource use on gfx950 (-Rpass-analysis=kernel-resource-usage): 0 bytes of scratch and no AGPRs in every instantiation.  VGPRs
// (waves per SIMD), the range over ADD and CELL:
//                 tangent TD = 3    tangent TD = 2     force TD = 3    force TD = 2    cells TD = 3     cells TD = 2
//   m_svk         102 - 126 (4)     92 - 94 (5)        84 - 90 (5)     54 (8)          82 - 88 (5)      48 - 55 (8)
//   m_mooney      108 - 126 (4)     78 - 94 (5 - 6)    82 - 90 (5)     58 - 64 (8)     80 - 90 (5 - 6)  56 - 62 (8)
//   m_yeoh        126 (4)           90 - 94 (5)        92 - 94 (5)     58 - 62 (8)     80 - 92 (5 - 6)  54 - 62 (8)
//   m_neo         -                 -                  -               -               90 - 102 (4 - 5) 60 - 66 (7 - 8)
// The model functors, the kinematics helpers (hm_cell_load, hm_invariants, hm_dvec, hm_row) and the material checks live in
// fs_hyper_energy.h, which fs_hyper_dynamics.hip includes as well.
#include "fs_hyper_energy.h"

// ---- tangent ---------------------------------------------------------------------------------------------------------------------
template <class M, int TD, bool ADD, bool CELL>
__global__ void __launch_bounds__(FS_BLOCK) k_hm_tangent(int64_t n_entries, const int32_t* __restrict__ ptr, const int32_t* __restrict__ src,
                                                         const int32_t* __restrict__ cells, const double* __restrict__ xyz4,
                                                         const double* __restrict__ u, const hm_par par, const double2* __restrict__ rows,
                                                         int64_t plane, double* __restrict__ val, const box_snap bx) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; e < n_entries; e += stride) {
        double acc[TD][TD];
#pragma unroll
        for (int i = 0; i < TD; ++i)
#pragma unroll
            for (int k = 0; k < TD; ++k) acc[i][k] = 0.0;
        const int32_t q1 = ptr[e + 1];
        for (int32_t q = ptr[e]; q < q1; ++q) {
            int64_t c;
            int a, b;
            p1_source<TD>(src[q], c, a, b);
            const int4 v4 = reinterpret_cast<const int4*>(cells)[c];
            const hm_par mat = CELL ? hm_row(rows, c) : par;
            double F[3][3], ga[3], gb[3], vol;
            hm_cell_load<TD, true>(v4, xyz4, u, bx, a, b, F, ga, gb, vol);
            hm_state s;
            hm_invariants(F, s);
            hm_w w;
            double psi;
            M::eval(mat, s.I1, s.I2, s.J, w, psi);
            double Fa[3], Fb[3], a1[3], a2[3], a3[3], b1[3], b2[3], b3[3];
            hm_dvec(F, s, ga, Fa, a1, a2, a3);
            hm_dvec(F, s, gb, Fb, b1, b2, b3);
            const double gg = ga[0] * gb[0] + ga[1] * gb[1] + ga[2] * gb[2];
            const double ff = Fa[0] * Fb[0] + Fa[1] * Fb[1] + Fa[2] * Fb[2];
            const double cr[3] = {ga[1] * gb[2] - ga[2] * gb[1], ga[2] * gb[0] - ga[0] * gb[2], ga[0] * gb[1] - ga[1] * gb[0]};
            double wv[3];
            hm_mul(F, cr, wv);
            const double dg = 2.0 * w.w1 * gg + w.w2 * (2.0 * s.I1 * gg - 2.0 * ff);
#pragma unroll
            for (int i = 0; i < TD; ++i) {
                const double u1 = w.w11 * a1[i] + w.w12 * a2[i] + w.w1j * a3[i];
                const double u2 = w.w12 * a1[i] + w.w22 * a2[i] + w.w2j * a3[i];
                const double u3 = w.w1j * a1[i] + w.w2j * a2[i] + w.wjj * a3[i];
#pragma unroll
                for (int k = 0; k < TD; ++k) {
                    double x = u1 * b1[k] + u2 * b2[k] + u3 * b3[k];
                    x += w.w2 * (4.0 * Fa[i] * Fb[k] - 2.0 * Fb[i] * Fa[k] - 2.0 * gg * s.B[i][k]);
                    if (i == k) x += dg;
                    else x += w.wj * (((k - i + 3) % 3 == 1) ? wv[3 - i - k] : -wv[3 - i - k]);      // eps_ikm w_m, m = 3 - i - k
                    acc[i][k] += vol * x;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < TD; ++i)
#pragma unroll
            for (int k = 0; k < TD; ++k) {
                const int64_t idx = (int64_t)(i * TD + k) * plane + e;
                val[idx] = ADD ? val[idx] + acc[i][k] : acc[i][k];
            }
    }
}

// ---- internal force ----------------------------------------------------------------------------------------------------------------
template <class M, int TD, bool ADD, bool CELL>
__global__ void __launch_bounds__(FS_BLOCK) k_hm_force(int64_t n_rows, const int64_t* __restrict__ slice_ptr, const int32_t* __restrict__ sell_col,
                                                       const int32_t* __restrict__ gptr, const int32_t* __restrict__ gsrc,
                                                       const int32_t* __restrict__ cells, const double* __restrict__ xyz4,
                                                       const double* __restrict__ u, const hm_par par, const double2* __restrict__ rows,
                                                       const box_snap bx, double* __restrict__ f) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; r < n_rows; r += stride) {
        const int64_t e = p1_diag_entry(r, slice_ptr, sell_col);
        double acc[TD];
#pragma unroll
        for (int i = 0; i < TD; ++i) acc[i] = 0.0;
        if (e >= 0) {
            const int32_t q1 = gptr[e + 1];
            for (int32_t q = gptr[e]; q < q1; ++q) {
                int64_t c;
                int a, b;
                p1_source<TD>(gsrc[q], c, a, b);
                const int4 v4 = reinterpret_cast<const int4*>(cells)[c];
                const hm_par mat = CELL ? hm_row(rows, c) : par;
                double F[3][3], ga[3], gb[3], vol;
                hm_cell_load<TD, false>(v4, xyz4, u, bx, a, b, F, ga, gb, vol);
                hm_state s;
                hm_invariants(F, s);
                hm_w w;
                double psi;
                M::eval(mat, s.I1, s.I2, s.J, w, psi);
                double Fa[3], a1[3], a2[3], a3[3];
                hm_dvec(F, s, ga, Fa, a1, a2, a3);
#pragma unroll
                for (int i = 0; i < TD; ++i) acc[i] += vol * (w.w1 * a1[i] + w.w2 * a2[i] + w.wj * a3[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < TD; ++i) f[TD * r + i] = ADD ? f[TD * r + i] + acc[i] : acc[i];
    }
}

// ---- energy, Cauchy stress and inverted cells -------------------------------------------------------------------------------------
// STRESS false: part_e gets the energy partials.  STRESS true: sig[c][6 or 4] = sigma (zeros in an inverted cell; the host refuses
// the result then).  A cell counts as inverted when J <= 0 or J is not finite.
template <class M, int TD, bool CELL, bool STRESS>
__global__ void __launch_bounds__(FS_BLOCK) k_hm_cells(int64_t nc, const int32_t* __restrict__ cells, const double* __restrict__ xyz4,
                                                       const double* __restrict__ u, const hm_par par, const double2* __restrict__ rows,
                                                       const box_snap bx, double* __restrict__ part_e, int64_t* __restrict__ part,
                                                       double* __restrict__ sig) {
    constexpr int NE = TD == 3 ? 6 : 4;
    double en = 0.0;
    int64_t n_bad[1] = {0}, first = INT64_MAX;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += stride) {
        const int4 v4 = reinterpret_cast<const int4*>(cells)[c];
        const hm_par mat = CELL ? hm_row(rows, c) : par;
        double F[3][3], ga[3], gb[3], vol;
        hm_cell_load<TD, false>(v4, xyz4, u, bx, 0, 0, F, ga, gb, vol);
        hm_state s;
        hm_invariants(F, s);
        const bool bad = !(s.J > 0.0) || !isfinite(s.J);
        if (bad) {
            ++n_bad[0];
            first = c < first ? c : first;
        }
        hm_w w;
        double psi;
        M::eval(mat, s.I1, s.I2, bad ? 1.0 : s.J, w, psi);
        if (STRESS) {
            const double k1 = bad ? 0.0 : 2.0 / s.J * (w.w1 + w.w2 * s.I1), k2 = bad ? 0.0 : 2.0 / s.J * w.w2, k3 = bad ? 0.0 : w.wj;
            double B2[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) B2[i][j] = s.B[i][0] * s.B[0][j] + s.B[i][1] * s.B[1][j] + s.B[i][2] * s.B[2][j];
            double* o = sig + NE * c;
            o[0] = k1 * s.B[0][0] - k2 * B2[0][0] + k3;
            o[1] = k1 * s.B[1][1] - k2 * B2[1][1] + k3;
            o[2] = k1 * s.B[2][2] - k2 * B2[2][2] + k3;
            o[3] = k1 * s.B[0][1] - k2 * B2[0][1];
            if (TD == 3) {
                o[4] = k1 * s.B[0][2] - k2 * B2[0][2];
                o[5] = k1 * s.B[1][2] - k2 * B2[1][2];
            }
        } else if (!bad) {
            en += vol * psi;
        }
    }
    p1_cell_tally<1, !STRESS>(n_bad, first, en, part, part_e);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// the per-cell pass (energy or stress) and its tally; sig_dev: device [nc][6 or 4] for the stress
template <class M>
static int hm_cells_pass(fs_space_s* sp, fs_vector_s* u, const hm_par& par, const double2* rows, bool stress, double* sig_dev,
                         fs_hyper_info* info) {
    fs_mesh_s* m = sp->mesh;
    hipStream_t s = fs_rt().stream;
    const box_snap bx = make_box_snap(m);
    int rc = FS_OK;
    fs_dispatch_bool(stress, [&](auto ST) {
        constexpr bool st = decltype(ST)::value;
        fs_cell_tally<1, true> tally;                  // the energy is summed where no stress is asked for
        if ((rc = tally.alloc()) != FS_OK) return;
        fs_dispatch_int<3, 2>(m->tdim, [&](auto TD) {
            fs_dispatch_bool(rows != nullptr, [&](auto CELL) {
                hipLaunchKernelGGL((k_hm_cells<M, decltype(TD)::value, decltype(CELL)::value, st>), dim3(tally.nb), dim3(FS_BLOCK), 0, s, m->nc,
                                   m->cells.p, m->xyz.p, u->d.p, par, rows, bx, tally.part_sum.p, tally.part.p, sig_dev);
            });
        });
        if ((rc = tally.finish<!st>(s)) != FS_OK || (rc = tally.get<!st>(s)) != FS_OK) return;
        info->energy = tally.sum;
        info->n_inverted = tally.n[0];
        info->first_inverted_cell = fs_first_cell(m, tally.n[0], tally.n[1]);
    });
    FS_CHECK(rc);
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

template <class M>
static int hm_assemble(fs_space_s* sp, fs_matrix_s* K, fs_vector_s* r, fs_vector_s* u, const hm_par& par, const double2* rows, bool add,
                       int what, fs_hyper_info* info) {
    hipStream_t s = fs_rt().stream;
    const box_snap bx = make_box_snap(sp->mesh);
    int rc = FS_OK;
    fs_dispatch_int<3, 2>(sp->mesh->tdim, [&](auto TD) {
        fs_dispatch_bool(add, [&](auto ADD) {
            fs_dispatch_bool(rows != nullptr, [&](auto CELL) {
                constexpr int td = decltype(TD)::value;
                constexpr bool a = decltype(ADD)::value, c = decltype(CELL)::value;
                if (rc == FS_OK && (what & FS_HYPER_TANGENT))
                    rc = p1_launch_blocks(sp, s, k_hm_tangent<M, td, a, c>, u->d.p, par, rows, sp->sell_entries, K->val.p, bx);
                if (rc == FS_OK && (what & FS_HYPER_FORCE)) rc = p1_launch_nodes(sp, s, k_hm_force<M, td, a, c>, u->d.p, par, rows, bx, r->d.p);
            });
        });
    });
    FS_CHECK(rc);
    if (info) FS_CHECK((hm_cells_pass<M>(sp, u, par, rows, false, nullptr, info)));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}

// the form's material, checked: the parameter row in par, or (per-cell) the rows on the device in store and `rows` pointing at them
static int hm_material_dev(const fs_hyper_form* form, int64_t nc, const char* who, hm_par& par, dbuf<double>& store, const double2*& rows,
                           hipStream_t s) {
    std::vector<double> host_rows;
    FS_CHECK(hm_material(form, nc, who, par, host_rows));
    if (!host_rows.empty()) FS_CHECK(fs_upload_cell_rows(store, host_rows.data(), 4, nc, s));
    rows = host_rows.empty() ? nullptr : reinterpret_cast<const double2*>(store.p);
    return FS_OK;
}

// fs_assemble_hyperelastic for every model but the neo-Hookean one (the caller has checked the handles and `what`)
int fs_hyper_models_assemble(fs_space_s* sp, fs_matrix_s* K, fs_vector_s* r, fs_vector_s* u, const fs_hyper_form* form, int what,
                             fs_hyper_info* info) {
    const char* who = "fs_assemble_hyperelastic";
    hipStream_t s = fs_rt().stream;
    hm_par par;
    dbuf<double> rstore;
    const double2* rows = nullptr;
    FS_CHECK(hm_material_dev(form, sp->mesh->nc, who, par, rstore, rows, s));
    FS_REQUIRE(form->model != FS_HYPER_NEO_HOOKEAN, "%s: the neo-Hookean energy is assembled by its own kernels", who);
    FS_CHECK(p1_gather_map(sp, s));          // ahead of the first launch, also where only the energy is asked for
    int rc = FS_OK;
    hm_dispatch_model(form->model, [&](auto M) {
        using model_t = decltype(M);
        if constexpr (!std::is_same<model_t, m_neo>::value) rc = hm_assemble<model_t>(sp, K, r, u, par, rows, form->add != 0, what, info);
    });
    return rc;
}

extern "C" int fs_hyper_stress(fs_space_t space, fs_vector_t u, const fs_hyper_form* form, double* sigma, fs_hyper_info* info) {
    const char* who = "fs_hyper_stress";
    FS_REFUSE_DG_SPACE(space, who);
    FS_REQUIRE(space && u && form && sigma, "%s: null pointer", who);
    fs_space_s* sp = space;
    fs_mesh_s* m = sp->mesh;
    FS_CHECK(fs_require_vector_cg1(sp, who));          // (no gather here: the slot table is not asked for)
    FS_CHECK(fs_require_displacement(u, sp, who));
    hipStream_t s = fs_rt().stream;
    hm_par par;
    dbuf<double> rstore, sig;
    const double2* rows = nullptr;
    FS_CHECK(hm_material_dev(form, m->nc, who, par, rstore, rows, s));
    const int ne = m->tdim == 3 ? 6 : 4;
    FS_CHECK(sig.alloc((int64_t)ne * m->nc));
    fs_hyper_info local;
    int rc = FS_OK;
    hm_dispatch_model(form->model, [&](auto M) { rc = hm_cells_pass<decltype(M)>(sp, u, par, rows, true, sig.p, &local); });
    FS_CHECK(rc);
    if (info) *info = local;
    FS_REQUIRE(local.n_inverted == 0, "%s: %lld cell(s) are inverted (J <= 0 or not finite), first cell %lld: the Cauchy stress is not defined there",
               who, (long long)local.n_inverted, (long long)local.first_inverted_cell);
    FS_CHECK(sig.download(sigma, (int64_t)ne * m->nc, s));
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
}
