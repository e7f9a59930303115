// Explicit finite-strain dynamics on vector CG1 spaces (tetrahedra, triangles in true plane strain): the central-difference marcher
// of HyperelasticDynamicsSolver, on the device.  Neither the reference nor its NonlinearElasticitySolver has a transient form.
//
// The scheme is the leapfrog of fs_leapfrog.h - the one fs_dynamics_explicit.hip marches with y_n = K u_n; the formulas of the step,
// of the start and of the Dirichlet rows, the constants and the per-row helpers are there - with y_n = f_int(u_n) = dPi/du, the
// internal force of a hyperelastic energy (neo-Hookean, St Venant-Kirchhoff, Mooney-Rivlin, Yeoh: the invariant-form functors of
// fs_hyper_energy.h), the LUMPED mass m = M 1 of the reference configuration and C = eta_M diag(m).  The energy of the step
// n -> n+1 is reported as
//   E_kin = 1/2 sum_i m_i w_{n+1/2,i}^2,   Pi(u_n) = sum_cells V psi(F(u_n)):
// the potential half is taken at t_n, where the force is evaluated (the linear marcher reports 1/2 u_{n+1}^T K u_n).  All four
// energies have psi = 0 at rest in both dimensions: the neo-Hookean one is m_neo's, with F embedded in 3 x 3 in plane strain (the
// "- 3" shift of the 2-D energy of fs_hyper.hip does not appear here).
//
// With a nonlinear material there is no K to multiply: a step evaluates the force at the current displacement.  k_hdyn_step fuses
// that gather with the leapfrog update, so a step is ONE launch and fs_hyper_dyn_advance enqueues any number of them back to back.
//   k_hdyn_step<M, TD, CELL, MODE>   M the energy functor, TD = 3 / 2, CELL = one parameter row per cell: compile-time, as in
//       k_hm_force, so the parameter row stays in registers.  One thread per owned node, grid-stride over the geometry of the batch
//       driver (fs_march_grid of the rows: it depends on the node count only, so the energy partials are summed in the same order
//       however a march is split).  The thread walks the sources of its node's diagonal block exactly as k_hm_force does
//       (p1_diag_entry, gptr, gsrc: one source per incident cell, a = b), forms F, the invariants and M::eval per source and sums the
//       TD force components and the node's share V psi / (TD + 1) of Pi - psi is computed by M::eval anyway, so no per-cell energy
//       pass runs in the march.  Then, per component: the update formula, the Dirichlet row, the receiver sample, E_kin; the two
//       partials go out through fs_march_store_partials.  No atomics on floats anywhere.
//       u IS DOUBLE-BUFFERED: the gather of node r reads u_n of its neighbours while their threads, possibly in another workgroup,
//       produce u_{n+1}; the in-place update of k_dynx_update would be a race here.  The kernel reads buffer A and writes buffer B
//       and the state swaps the two per step; w and the row table are touched by their own thread only and stay in place.
//       A source with J <= 0 or J not finite makes the thread's potential partial NaN - explicitly, because St Venant-Kirchhoff
//       stays finite at J <= 0 -, so the finishing pass that counts non-finite energies reports the step (n_nonfinite,
//       first_nonfinite_step).  This is arithmetic only: no gather index depends on u.
//     MODE = HDYN_STEP   the step above
//            HDYN_START  the first step from (u_0, v_0); k_leapfrog_dirichlet (fs_leapfrog.h) has put g s_g[0] into the Dirichlet rows
//                        of u_0 before it, on the same stream
//            HDYN_FULL   v_n and a_n of the state's time point: w+ is recomputed, nothing is stored
//            HDYN_FORCE  f_int and Pi of the held state, for checks and for internal_force()
//   Per node and step: one source per incident cell (24 at an interior node of a box mesh, 6 in a rectangle mesh), each with the cell
//   record, 4 vertex records and 4 displacements through the caches (16 B + 4 x 24 B + 4 x 24 B, + 32 B with CELL) and about 330
//   fp64 flops with the model, and per component u, w, m, F read, u, w written and one flag byte: 3 x 49 B = 147 B of row traffic.
// Resource use on gfx950 (-Rpass-analysis=kernel-resource-usage): 0 bytes of scratch and no AGPRs in every instantiation.  VGPRs
// (waves per SIMD) of HDYN_STEP, CELL false - true; over the four modes the range is 90 - 161 VGPRs:
//                 TD = 3                TD = 2
//   m_neo         147 - 157 (3)         106 - 112 (4)
//   m_svk         125 - 135 (4 - 3)     94 - 102 (5 - 4)
//   m_mooney      135 - 157 (3)         100 - 122 (4)
//   m_yeoh        133 - 159 (3)         104 - 130 (4 - 3)
// The sources are walked in groups of four with the cell records of a group fetched before its arithmetic (the PF = 4 of
// k_hyper_force_gather).  Without the groups the kernel needs 68 - 120 VGPRs (4 - 7 waves) and takes twice as long on the 80^3-cell
// box (565 against 266 us, Mooney-Rivlin): the walk is bound by the chain source -> cell record -> vertices, not by occupancy.
// The row table (load, flags, receivers), the finishing pass and the batch driver: fs_march.h.  The state object and the checks the
// two leapfrog marchers share: fs_leapfrog.h.
#include "fs_hyper_energy.h"
#include "fs_leapfrog.h"
#include <mutex>

#define HDYN_STEP 0
#define HDYN_START 1
#define HDYN_FULL 2
#define HDYN_FORCE 3

// the rows of a launch; what a mode does not use is nullptr
struct hdyn_rows {
    const double* ua;                    // u_n (the gather reads it)
    double* ub;                          // STEP, START: u_{n+1}
    double* w;                           // STEP: in place; START: out; FULL: in
    const double* m;
    const double* load;
    const uint8_t* flag;
    const double* v0;                    // START
    double* o0;                          // FULL: v_n; FORCE: f_int
    double* o1;                          // FULL: a_n
    int n_rec;
    const int32_t* rec;
    double* trace;                       // STEP: this step's [n_rec] samples (nullptr: none wanted)
    double* part;                        // this launch's [2][gridDim.x] partials
};

struct fs_hyper_dyn_state_s : fs_leapfrog_state {
    dbuf<double> u[2];                   // u_n is u[cur]; a step writes u[1 - cur]
    int cur = 0;
    // the material on the device: uploaded when it changes, never per step
    int model = -1;
    hm_par par = {};
    std::vector<double> rows_host;
    dbuf<double> rows;
    dbuf<double> en;                     // _internal_force: (-, Pi)
    dbuf<unsigned long long> bad;
    fs_hyper_dyn_state_s() : fs_leapfrog_state("fs_hyper_dyn") {}
};

// ---- the kernel ----------------------------------------------------------------------------------------------------------------
template <class M, int TD, bool CELL, int MODE>
__global__ void __launch_bounds__(FS_BLOCK) k_hdyn_step(int64_t n_nodes, const int64_t* __restrict__ slice_ptr, const int32_t* __restrict__ sell_col,
                                                        const int32_t* __restrict__ gptr, const int32_t* __restrict__ gsrc,
                                                        const int32_t* __restrict__ cells, const double* __restrict__ xyz4, const hm_par par,
                                                        const double2* __restrict__ rows, const box_snap bx, const hdyn_rows R,
                                                        const fs_leapfrog_consts c, double sf, double sg) {
    __shared__ double lds4[4];
    const double* __restrict__ u = R.ua;
    double ek = 0.0, ep = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_nodes; r += stride) {
        const int64_t e = p1_diag_entry(r, slice_ptr, sell_col);
        double acc[TD];
#pragma unroll
        for (int i = 0; i < TD; ++i) acc[i] = 0.0;
        double pot = 0.0;
        bool inverted = false;
        if (e >= 0) {
            // the sources in groups of four with their cell records (and parameter rows) fetched first, as k_hyper_force_gather does: the
            // walk and the order of the sums are k_hm_force's, the loads of a group no longer wait for one another
            constexpr int PF = 4;
            const int32_t q1 = gptr[e + 1];
            for (int32_t q0 = gptr[e]; q0 < q1; q0 += PF) {
              int32_t sc[PF];
              int4 vc[PF];
              hm_par pc[PF];
#pragma unroll
              for (int k = 0; k < PF; ++k) sc[k] = q0 + k < q1 ? gsrc[q0 + k] : -1;
#pragma unroll
              for (int k = 0; k < PF; ++k) {
                vc[k] = sc[k] >= 0 ? reinterpret_cast<const int4*>(cells)[p1_source_cell<TD>(sc[k])] : make_int4(0, 0, 0, 0);
                if (CELL) pc[k] = sc[k] >= 0 ? hm_row(rows, p1_source_cell<TD>(sc[k])) : par;
              }
#pragma unroll
              for (int k = 0; k < PF; ++k) {
                if (q0 + k >= q1) break;
                int64_t cc;
                int a, b;
                p1_source<TD>(sc[k], cc, a, b);
                const int4 v4 = vc[k];
                const hm_par mat = CELL ? pc[k] : par;
                double F[3][3], ga[3], gb[3], vol;
                hm_cell_load<TD, false>(v4, xyz4, u, bx, a, b, F, ga, gb, vol);
                hm_state s;
                hm_invariants(F, s);
                inverted |= !(s.J > 0.0) || !isfinite(s.J);
                hm_w w;
                double psi;
                M::eval(mat, s.I1, s.I2, s.J, w, psi);
                double Fa[3], a1[3], a2[3], a3[3];
                hm_dvec(F, s, ga, Fa, a1, a2, a3);
#pragma unroll
                for (int i = 0; i < TD; ++i) acc[i] += vol * (w.w1 * a1[i] + w.w2 * a2[i] + w.wj * a3[i]);
                pot += vol * psi * (1.0 / (TD + 1));
              }
            }
        }
        ep += inverted ? __builtin_nan("") : pot;
#pragma unroll
        for (int i = 0; i < TD; ++i) {
            const int64_t row = TD * r + i;
            if (MODE == HDYN_FORCE) {
                R.o0[row] = acc[i];
                continue;
            }
            const double mi = R.m[row], fi = R.load[row];
            const bool dir = R.flag[row] & FS_MARCH_DIRICHLET;
            if (MODE == HDYN_FULL) {
                const double wi = R.w[row];
                const double wp = fs_leapfrog_w(c, wi, acc[i], mi, fi, sf);
                R.o0[row] = fs_leapfrog_v(wi, wp, dir);
                R.o1[row] = fs_leapfrog_a(c, wi, wp, dir);
                continue;
            }
            const double ui = u[row];
            const fs_leapfrog_row n = MODE == HDYN_START ? fs_leapfrog_start_row(c, ui, R.v0[row], acc[i], mi, fi, sf, sg, dir)
                                                         : fs_leapfrog_step_row(c, ui, R.w[row], acc[i], mi, fi, sf, sg, dir);
            R.ub[row] = n.u;
            R.w[row] = n.w;
            ek += fs_leapfrog_ekin(mi, n.w);
            if (MODE == HDYN_STEP) fs_march_sample(R.flag[row], row, n.u, R.n_rec, R.rec, R.trace);
        }
    }
    fs_march_store_partials(ek, ep, lds4, R.part);
}

// ---- host side: checks, the material, the launch ---------------------------------------------------------------------------------
static int hdyn_space_ok(const fs_space_s* sp, const char* who) {
    FS_REQUIRE(sp, "%s: null space", who);
    FS_REQUIRE(!fs_is_dg(sp), "%s: not built for DG spaces (vector CG1 spaces only)", who);
    FS_CHECK(fs_require_solid_space(sp, who));
    return fs_march_one_rank(sp, who);
}

// the form's material, checked, on the device: uploaded only when it differs from what the state holds
static int hdyn_material(fs_hyper_dyn_state_s* st, const fs_hyper_form* form, const char* who, hipStream_t s) {
    FS_REQUIRE(form, "%s: null form", who);
    const int64_t nc = st->space->mesh->nc;
    hm_par par;
    std::vector<double> host_rows;
    FS_CHECK(hm_material(form, nc, who, par, host_rows));
    if (!host_rows.empty() && (st->model != form->model || host_rows != st->rows_host)) {
        FS_CHECK(fs_upload_cell_rows(st->rows, host_rows.data(), 4, nc, s));
        FS_HIP(hipStreamSynchronize(s));
    }
    st->rows_host.swap(host_rows);
    st->par = par;
    st->model = form->model;
    return p1_gather_map(st->space, s);          // (k_hdyn_step has the marchers' grid: its launch is its own)
}

template <int MODE>
static void hdyn_launch(fs_hyper_dyn_state_s* st, const hdyn_rows& R, double sf, double sg, hipStream_t s) {
    fs_space_s* sp = st->space;
    fs_mesh_s* m = sp->mesh;
    const box_snap bx = make_box_snap(m);
    const double2* rows = st->rows_host.empty() ? nullptr : reinterpret_cast<const double2*>(st->rows.p);
    const int g = fs_march_grid(st->n);
    hm_dispatch_model(st->model, [&](auto M) {
        fs_dispatch_int<3, 2>(m->tdim, [&](auto TD) {
            fs_dispatch_bool(rows != nullptr, [&](auto CELL) {
                hipLaunchKernelGGL((k_hdyn_step<decltype(M), decltype(TD)::value, decltype(CELL)::value, MODE>), dim3(g), dim3(FS_BLOCK), 0,
                                   s, sp->n_nodes_owned, sp->slice_ptr.p, sp->sell_col.p, sp->gmap_ptr.p, sp->gmap_src.p, m->cells.p, m->xyz.p,
                                   st->par, rows, bx, R, st->c, sf, sg);
            });
        });
    });
}

static hdyn_rows hdyn_rows_of(fs_hyper_dyn_state_s* st) {
    hdyn_rows R = {};
    R.ua = st->u[st->cur].p;
    R.ub = st->u[1 - st->cur].p;
    R.w = st->w.p;
    R.m = st->m.p;
    R.load = st->load.p;
    R.flag = st->flag.p;
    R.part = st->part.p;
    return R;
}

static int hdyn_ready(const fs_hyper_dyn_state_s* st, const char* who, bool started) {
    FS_REQUIRE(st, "%s: null pointer", who);
    FS_CHECK(hdyn_space_ok(st->space, who));
    return st->ready(who, started);
}

// ---- the state object --------------------------------------------------------------------------------------------------------------
extern "C" int fs_hyper_dyn_state_create(fs_space_t space, fs_hyper_dyn_state_t* out) {
    FS_CHECK(fs_require_init());
    FS_REQUIRE(out, "fs_hyper_dyn_state_create: null pointer");
    FS_CHECK(hdyn_space_ok(space, "fs_hyper_dyn_state_create"));
    fs_hyper_dyn_state_s* st = new fs_hyper_dyn_state_s();
    st->space = space;
    hipStream_t s = fs_rt().stream;
    int rc = st->alloc(space->n_dofs_owned, {&st->u[0], &st->u[1]}, s);
    if (rc == FS_OK) rc = st->en.alloc(2);
    if (rc == FS_OK) rc = st->bad.alloc(2);
    return fs_march_create_finish("fs_hyper_dyn_state_create", st, rc, s, out);
}

extern "C" int fs_hyper_dyn_state_destroy(fs_hyper_dyn_state_t st) {
    delete st;
    return FS_OK;
}

extern "C" int fs_hyper_dyn_state_configure(fs_hyper_dyn_state_t st, double dt, double eta_m, const double* mass, const double* load,
                                            int64_t n_dirichlet, const int32_t* dirichlet_dofs, const double* dirichlet_values) {
    FS_REQUIRE(st, "fs_hyper_dyn_state_configure: null pointer");
    return st->configure("fs_hyper_dyn_state_configure", dt, eta_m, mass, load, n_dirichlet, dirichlet_dofs, dirichlet_values);
}

extern "C" int fs_hyper_dyn_state_set(fs_hyper_dyn_state_t st, const double* u, const double* w, int64_t step) {
    FS_REQUIRE(st, "fs_hyper_dyn_state_set: null pointer");
    return st->set("fs_hyper_dyn_state_set", st->u[st->cur], u, w, step);
}

extern "C" int fs_hyper_dyn_state_get(fs_hyper_dyn_state_t st, double* u, double* w, int64_t* step) {
    FS_REQUIRE(st, "fs_hyper_dyn_state_get: null pointer");
    return st->get(st->u[st->cur], u, w, step);
}

// ---- the march -------------------------------------------------------------------------------------------------------------------
extern "C" int fs_hyper_dyn_start(fs_hyper_dyn_state_t st, const fs_hyper_form* form, const double* u0, const double* v0, double load_scale0,
                                  double dirichlet_scale0, double dirichlet_scale1) {
    const char* who = "fs_hyper_dyn_start";
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(hdyn_ready(st, who, false));
    FS_CHECK(st->start_ok(who, u0, v0, load_scale0, dirichlet_scale0, dirichlet_scale1));
    hipStream_t s = fs_rt().stream;
    FS_CHECK(hdyn_material(st, form, who, s));
    FS_CHECK(st->start_fields(st->u[st->cur], u0, v0, dirichlet_scale0, s));   // the kernel below reads u[cur] behind it on s
    hdyn_rows R = hdyn_rows_of(st);
    R.v0 = st->t0.p;
    hdyn_launch<HDYN_START>(st, R, load_scale0, dirichlet_scale1, s);
    FS_KERNEL_CHECK();
    FS_HIP(hipStreamSynchronize(s));
    st->cur ^= 1;
    st->step = 1;
    return FS_OK;
}

extern "C" int fs_hyper_dyn_advance(fs_hyper_dyn_state_t st, const fs_hyper_form* form, int64_t n_steps, const double* load_scale,
                                    const double* dirichlet_scale, int64_t n_receivers, const int32_t* receiver_dofs, double* traces,
                                    double* energy, fs_march_info* info) {
    const char* who = "fs_hyper_dyn_advance";
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(hdyn_ready(st, who, true));
    hipStream_t s = fs_rt().stream;
    FS_CHECK(hdyn_material(st, form, who, s));
    auto enqueue = [&](int64_t k, double* trace, double* part) {
        hdyn_rows R = hdyn_rows_of(st);
        R.n_rec = (int)n_receivers;
        R.rec = st->rec.p;
        R.trace = trace;
        R.part = part;
        hdyn_launch<HDYN_STEP>(st, R, load_scale[k], dirichlet_scale[k], s);
        st->cur ^= 1;
        ++st->step;
        return (int)FS_OK;
    };
    return fs_march_advance(who, nullptr, st, true, n_steps, load_scale, dirichlet_scale, n_receivers, receiver_dofs, traces, energy, info,
                            enqueue);
}

extern "C" int fs_hyper_dyn_full_step(fs_hyper_dyn_state_t st, const fs_hyper_form* form, double load_scale_n, double* v_out, double* a_out) {
    const char* who = "fs_hyper_dyn_full_step";
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(hdyn_ready(st, who, true));
    FS_REQUIRE(isfinite(load_scale_n), "%s: the load factor is not finite", who);
    hipStream_t s = fs_rt().stream;
    FS_CHECK(hdyn_material(st, form, who, s));
    hdyn_rows R = hdyn_rows_of(st);
    R.o0 = st->t0.p;
    R.o1 = st->t1.p;
    hdyn_launch<HDYN_FULL>(st, R, load_scale_n, 0.0, s);
    FS_KERNEL_CHECK();
    return st->full_step_out(v_out, a_out, s);
}

extern "C" int fs_hyper_dyn_internal_force(fs_hyper_dyn_state_t st, const fs_hyper_form* form, double* f_out, double* energy_out) {
    const char* who = "fs_hyper_dyn_internal_force";
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(hdyn_ready(st, who, true));
    hipStream_t s = fs_rt().stream;
    FS_CHECK(hdyn_material(st, form, who, s));
    const int64_t n = st->n;
    hdyn_rows R = hdyn_rows_of(st);
    R.o0 = st->t0.p;
    hdyn_launch<HDYN_FORCE>(st, R, 0.0, 0.0, s);
    FS_KERNEL_CHECK();
    FS_HIP(hipMemsetAsync(st->bad.p, 0, 2 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_march_finish<>, dim3(1), dim3(FS_BLOCK), 0, s, fs_march_grid(n), st->part.p, (int64_t)0, st->en.p, st->bad.p);
    FS_KERNEL_CHECK();
    double en[2] = {0.0, 0.0};
    if (f_out) FS_CHECK(st->t0.download(f_out, n, s));
    if (energy_out) FS_CHECK(st->en.download(en, 2, s));
    FS_HIP(hipStreamSynchronize(s));
    FS_KERNEL_CHECK();
    if (energy_out) *energy_out = en[1];
    return FS_OK;
}
