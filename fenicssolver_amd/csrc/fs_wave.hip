// Explicit scalar wave propagation on scalar CG1 spaces (tetrahedra, triangles): the time marcher of WaveSolver, on the device.
//
// The reference lists "wave propagation" among its solvers under development (Readme.md) and never delivers one; the model is the
// textbook one: u_tt = div(c^2 grad u) + f, central differences in time, lumped mass.  With the assembled stiffness K (coefficient
// c^2), the lumped mass m_i = int phi_i dx, the lumped first-order absorbing boundary d_i = sum_F c |F| / dim, the load F scaled in
// time by s_f and the Dirichlet values g scaled by s_g, a step n -> n+1 is, with y = K u^n,
//   (m/dt^2 + d/(2 dt)) u^{n+1} = s_f[n] F - y + (2 m/dt^2) u^n - (m/dt^2 - d/(2 dt)) u^{n-1},   u^{n+1}_i = g_i s_g[n+1] on Dirichlet rows,
// and the march starts with a^0 = (s_f[0] F - K u^0 - d v^0) / m, u^1 = u^0 + dt v^0 + dt^2/2 a^0.  The discrete energy of the step is
//   E_kin = 1/2 sum_i m_i ((u^{n+1} - u^n)_i / dt)^2,   E_pot = 1/2 (u^{n+1})^T y.
// A step is therefore NOT a solve: one product with K - the library's own, through the dispatch of fs_spmv (fs_spmv_dev) - and one
// pass over the rows.  fs_wave_advance enqueues any number of steps back to back; the host touches nothing in between (the time
// factors of a step travel as kernel arguments).
//
// Kernels (no floating-point atomics: a march gives the same bits however it is split into calls):
//   k_wave_update   one thread per row, grid-stride over a launch geometry that depends on the number of rows only: the update
//       formula, the Dirichlet rows, the receiver samples and the per-workgroup partials of both energy halves.  Per row it reads y,
//       u^n, u^{n-1}, m, d, F (8 B each) and one flag byte and writes u^{n+1}: 57 B.  A Dirichlet row keeps g_i in the slot of F_i
//       (its load is never used); bit 0 of the flag marks it, bit 1 marks a row some receiver samples - only such a row searches the
//       receiver list.
//   k_wave_finish   one workgroup per step of a chunk of FS_WAVE_CHUNK steps: sums that step's partials in a fixed order into the
//       energy table of the call and counts the steps whose energy is not finite (integer atomics: the count and the first such
//       step do not depend on the order).  A non-finite field value makes m_i ((u^{n+1} - u^n)_i / dt)^2 and with it E_kin non-finite,
//       so this is also the check of the field.
//   k_wave_start    the first step from (u^0, v^0).
#include "fs_common.h"
#include "fs_kernels.h"
#include <math.h>
#include <mutex>

#define FS_WAVE_BLOCKS 1024              // most workgroups of the update kernel (its partials are summed in this order)
#define FS_WAVE_CHUNK 64                 // steps between two finishing passes (the partial table holds this many steps)
#define FS_WAVE_DIRICHLET 1
#define FS_WAVE_RECEIVER 2

struct fs_wave_state_s {
    fs_space_s* space = nullptr;
    int64_t n = 0;                       // rows
    double dt = 0.0;
    bool configured = false;
    int64_t step = 0;                    // the n of u^n in `u`; 0: not started
    dbuf<double> up, u, w;               // u^{n-1}, u^n, work: rotated by pointer
    dbuf<double> y;                      // K u^n
    dbuf<double> m, d, load;             // lumped mass, lumped damping, F (Dirichlet rows: g)
    dbuf<uint8_t> flag;
    std::vector<uint8_t> flag_host;      // the Dirichlet bits; the receiver bits of `receivers` on top
    std::vector<int32_t> receivers;      // the list whose bits the device flags carry now
    dbuf<int32_t> rec;
    dbuf<double> part;                   // [FS_WAVE_CHUNK][2][grid]
    hipEvent_t ev[2] = {};
    ~fs_wave_state_s() {
        for (hipEvent_t e_ : ev)
            if (e_) (void)hipEventDestroy(e_);
    }
};

static int wave_grid(int64_t n) { return fs_grid_for(n, FS_BLOCK, FS_WAVE_BLOCKS); }

// ---- the first step --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FS_BLOCK) k_wave_start(int64_t n, const double* __restrict__ y, const double* __restrict__ u0,
                                                         const double* __restrict__ v0, const double* __restrict__ m,
                                                         const double* __restrict__ d, const double* __restrict__ load,
                                                         const uint8_t* __restrict__ flag, double dt, double sf, double sg,
                                                         double* __restrict__ u1) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double fi = load[i], vi = v0[i];
        const double a0 = (sf * fi - y[i] - d[i] * vi) / m[i];
        double un = u0[i] + dt * vi + (0.5 * dt * dt) * a0;
        if (flag[i] & FS_WAVE_DIRICHLET) un = fi * sg;
        u1[i] = un;
    }
}

// ---- one step ----------------------------------------------------------------------------------------------------------------
// part: this step's [2][gridDim.x] partials; trace: this step's [n_rec] samples (nullptr: none wanted)
__global__ void __launch_bounds__(FS_BLOCK) k_wave_update(int64_t n, const double* __restrict__ y, const double* __restrict__ u,
                                                          const double* __restrict__ up, const double* __restrict__ m,
                                                          const double* __restrict__ d, const double* __restrict__ load,
                                                          const uint8_t* __restrict__ flag, double idt, double idt2, double hidt,
                                                          double sf, double sg, double* __restrict__ unew, int n_rec,
                                                          const int32_t* __restrict__ rec, double* __restrict__ trace,
                                                          double* __restrict__ part) {
    __shared__ double lds4[4];
    double ek = 0.0, ep = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double yi = y[i], ui = u[i], upi = up[i], mi = m[i], di = d[i], fi = load[i];
        const uint8_t fl = flag[i];
        const double a = mi * idt2, b = di * hidt;
        double un = (sf * fi - yi + 2.0 * a * ui - (a - b) * upi) / (a + b);
        if (fl & FS_WAVE_DIRICHLET) un = fi * sg;
        unew[i] = un;
        const double vel = (un - ui) * idt;
        ek += 0.5 * mi * vel * vel;
        ep += 0.5 * un * yi;
        if ((fl & FS_WAVE_RECEIVER) && trace)
            for (int r = 0; r < n_rec; ++r)
                if (rec[r] == (int32_t)i) trace[r] = un;
    }
    const double tk = fs_block_sum(ek, lds4);
    const double tp = fs_block_sum(ep, lds4);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = tk;
        part[gridDim.x + blockIdx.x] = tp;
    }
}

// workgroup b: step k0 + b of the call, whose partials are part[b][2][g]; bad = (steps with a non-finite energy, the first of them)
__global__ void __launch_bounds__(FS_BLOCK) k_wave_finish(int g, const double* __restrict__ part, int64_t k0, double* __restrict__ energy,
                                                          unsigned long long* __restrict__ bad) {
    __shared__ double lds4[4];
    const double* p = part + (int64_t)blockIdx.x * 2 * g;
    double ek = 0.0, ep = 0.0;
    for (int j = threadIdx.x; j < g; j += FS_BLOCK) {
        ek += p[j];
        ep += p[g + j];
    }
    const double tk = fs_block_sum(ek, lds4);
    const double tp = fs_block_sum(ep, lds4);
    if (threadIdx.x == 0) {
        const int64_t k = k0 + blockIdx.x;
        energy[2 * k] = tk;
        energy[2 * k + 1] = tp;
        if (!(isfinite(tk) && isfinite(tp))) {
            atomicAdd(&bad[0], 1ull);
            atomicMin(&bad[1], (unsigned long long)k);
        }
    }
}

// ---- host side: the state object ---------------------------------------------------------------------------------------------
static int wave_space_ok(const fs_space_s* sp, const char* who) {
    FS_REFUSE_DG_SPACE(sp, who);
    FS_REQUIRE(sp, "%s: null space", who);
    const fs_mesh_s* m = sp->mesh;
    FS_REQUIRE(sp->degree == 1 && sp->ncomp == 1, "%s: scalar CG1 spaces on tetrahedra or triangles only (this space: CG%d with %d components "
               "on a %d-D mesh)", who, sp->degree, sp->ncomp, m->tdim);
    FS_REQUIRE(fs_rt().n_ranks == 1 && m->n_owned == m->nv && sp->n_nodes_owned == sp->n_nodes_local,
               "%s: the space has ghost nodes or the communicator several ranks: not supported", who);
    return FS_OK;
}

extern "C" int fs_wave_state_create(fs_space_t space, fs_wave_state_t* out) {
    FS_CHECK(fs_require_init());
    FS_REQUIRE(out, "fs_wave_state_create: null pointer");
    FS_CHECK(wave_space_ok(space, "fs_wave_state_create"));
    fs_wave_state_s* st = new fs_wave_state_s();
    st->space = space;
    st->n = space->n_dofs_owned;
    const int64_t n = st->n;
    hipStream_t s = fs_rt().stream;
    int rc = FS_OK;
    if ((rc = st->up.alloc(n)) || (rc = st->u.alloc(n)) || (rc = st->w.alloc(n)) || (rc = st->y.alloc(n)) || (rc = st->m.alloc(n)) ||
        (rc = st->d.alloc(n)) || (rc = st->load.alloc(n)) || (rc = st->flag.alloc(n)) ||
        (rc = st->part.alloc((int64_t)FS_WAVE_CHUNK * 2 * wave_grid(n))) || (rc = st->up.zero(s)) || (rc = st->u.zero(s)) ||
        (rc = st->w.zero(s)) || (rc = st->y.zero(s)) || (rc = st->m.zero(s)) || (rc = st->d.zero(s)) || (rc = st->load.zero(s)) ||
        (rc = st->flag.zero(s))) {
        delete st;
        return rc;
    }
    for (hipEvent_t& e_ : st->ev)
        if (hipEventCreate(&e_) != hipSuccess) {
            fs_set_error("fs_wave_state_create: hipEventCreate failed");
            delete st;
            return FS_ERR_HIP;
        }
    if (hipStreamSynchronize(s) != hipSuccess) {
        fs_set_error("fs_wave_state_create: hipStreamSynchronize failed");
        delete st;
        return FS_ERR_HIP;
    }
    st->flag_host.assign((size_t)n, 0);
    *out = st;
    return FS_OK;
}

extern "C" int fs_wave_state_destroy(fs_wave_state_t st) {
    delete st;
    return FS_OK;
}

extern "C" int fs_wave_state_configure(fs_wave_state_t st, double dt, const double* mass, const double* damping, const double* load,
                                       int64_t n_dirichlet, const int32_t* dirichlet_dofs, const double* dirichlet_values) {
    FS_REQUIRE(st && mass, "fs_wave_state_configure: null pointer");
    FS_REQUIRE(dt > 0.0 && isfinite(dt), "fs_wave_state_configure: the step length is %g: dt > 0 and finite is required", dt);
    FS_REQUIRE(n_dirichlet >= 0 && (n_dirichlet == 0 || (dirichlet_dofs && dirichlet_values)), "fs_wave_state_configure: Dirichlet list: null "
               "pointer or negative count");
    const int64_t n = st->n;
    for (int64_t i = 0; i < n; ++i) {
        FS_REQUIRE(mass[i] > 0.0 && isfinite(mass[i]), "fs_wave_state_configure: the lumped mass of row %lld is %g: m_i > 0 is required",
                   (long long)i, mass[i]);
        FS_REQUIRE(!damping || (damping[i] >= 0.0 && isfinite(damping[i])), "fs_wave_state_configure: the damping of row %lld is %g: d_i >= 0 is "
                   "required", (long long)i, damping ? damping[i] : 0.0);
        FS_REQUIRE(!load || isfinite(load[i]), "fs_wave_state_configure: the load of row %lld is not finite", (long long)i);
    }
    std::vector<double> f(load ? load : nullptr, load ? load + n : nullptr);
    f.resize((size_t)n, 0.0);
    std::vector<uint8_t> fl((size_t)n, 0);
    for (int64_t j = 0; j < n_dirichlet; ++j) {
        const int32_t i = dirichlet_dofs[j];
        FS_REQUIRE(i >= 0 && i < n, "fs_wave_state_configure: Dirichlet dof %d outside the space of %lld dofs", i, (long long)n);
        FS_REQUIRE(isfinite(dirichlet_values[j]), "fs_wave_state_configure: the Dirichlet value of dof %d is not finite", i);
        fl[i] = FS_WAVE_DIRICHLET;
        f[i] = dirichlet_values[j];
    }
    hipStream_t s = fs_rt().stream;
    FS_CHECK(st->m.upload(mass, n, s));
    if (damping) FS_CHECK(st->d.upload(damping, n, s));
    else FS_CHECK(st->d.zero(s));
    FS_CHECK(st->load.upload(f.data(), n, s));
    FS_CHECK(st->flag.upload(fl.data(), n, s));
    FS_HIP(hipStreamSynchronize(s));
    st->flag_host.swap(fl);
    st->receivers.clear();
    st->dt = dt;
    st->configured = true;
    return FS_OK;
}

extern "C" int fs_wave_state_set(fs_wave_state_t st, const double* u_prev, const double* u, int64_t step) {
    FS_REQUIRE(st && u_prev && u, "fs_wave_state_set: null pointer");
    FS_REQUIRE(step >= 1, "fs_wave_state_set: the step counter is %lld: (u^{n-1}, u^n) needs n >= 1", (long long)step);
    hipStream_t s = fs_rt().stream;
    FS_CHECK(st->up.upload(u_prev, st->n, s));
    FS_CHECK(st->u.upload(u, st->n, s));
    FS_HIP(hipStreamSynchronize(s));
    st->step = step;
    return FS_OK;
}

extern "C" int fs_wave_state_get(fs_wave_state_t st, double* u_prev, double* u, int64_t* step) {
    FS_REQUIRE(st, "fs_wave_state_get: null pointer");
    hipStream_t s = fs_rt().stream;
    if (u_prev) FS_CHECK(st->up.download(u_prev, st->n, s));
    if (u) FS_CHECK(st->u.download(u, st->n, s));
    FS_HIP(hipStreamSynchronize(s));
    if (step) *step = st->step;
    return FS_OK;
}

static int wave_matrix_ok(const fs_matrix_s* K, const fs_wave_state_s* st, const char* who) {
    FS_REQUIRE(K && st, "%s: null pointer", who);
    FS_REFUSE_DG(K, who);
    FS_REQUIRE(K->space == st->space && K->bs == 1, "%s: the state belongs to another space than the matrix", who);
    FS_CHECK(wave_space_ok(K->space, who));
    FS_REQUIRE(st->configured, "%s: the state was not configured (fs_wave_state_configure)", who);
    return FS_OK;
}

extern "C" int fs_wave_start(fs_matrix_t K, fs_wave_state_t st, const double* u0, const double* v0, double load_scale0, double dirichlet_scale1) {
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(wave_matrix_ok(K, st, "fs_wave_start"));
    FS_REQUIRE(u0 && v0, "fs_wave_start: null pointer");
    hipStream_t s = fs_rt().stream;
    const int64_t n = st->n;
    FS_CHECK(st->up.upload(u0, n, s));
    FS_CHECK(st->w.upload(v0, n, s));
    FS_CHECK(fs_spmv_prepare(K, s));
    FS_CHECK(fs_spmv_dev(K, st->up.p, st->y.p, s));
    FS_KERNEL_CHECK();
    hipLaunchKernelGGL(k_wave_start, dim3(wave_grid(n)), dim3(FS_BLOCK), 0, s, n, st->y.p, st->up.p, st->w.p, st->m.p, st->d.p, st->load.p,
                       st->flag.p, st->dt, load_scale0, dirichlet_scale1, st->u.p);
    FS_KERNEL_CHECK();
    FS_HIP(hipStreamSynchronize(s));
    st->step = 1;
    return FS_OK;
}

// the receiver bits of the device flags follow the list of the call (uploaded only when the list changes)
static int wave_set_receivers(fs_wave_state_s* st, int64_t n_rec, const int32_t* dofs, hipStream_t s) {
    if ((int64_t)st->receivers.size() == n_rec && (n_rec == 0 || !memcmp(st->receivers.data(), dofs, (size_t)n_rec * sizeof(int32_t))))
        return FS_OK;
    for (int32_t i : st->receivers) st->flag_host[i] &= (uint8_t)~FS_WAVE_RECEIVER;
    st->receivers.assign(dofs, dofs + n_rec);
    for (int32_t i : st->receivers) st->flag_host[i] |= FS_WAVE_RECEIVER;
    FS_CHECK(st->flag.upload(st->flag_host.data(), st->n, s));
    if (n_rec) {
        FS_CHECK(st->rec.alloc(n_rec));
        FS_CHECK(st->rec.upload(dofs, n_rec, s));
    }
    return FS_OK;
}

extern "C" int fs_wave_advance(fs_matrix_t K, fs_wave_state_t st, int64_t n_steps, const double* load_scale, const double* dirichlet_scale,
                               int64_t n_receivers, const int32_t* receiver_dofs, double* traces, double* energy, fs_wave_info* info) {
    std::lock_guard<std::recursive_mutex> solve_lock(fs_solve_mutex());
    FS_CHECK(wave_matrix_ok(K, st, "fs_wave_advance"));
    FS_REQUIRE(st->step >= 1, "fs_wave_advance: the state holds no (u^{n-1}, u^n) yet (fs_wave_start or fs_wave_state_set)");
    FS_REQUIRE(n_steps >= 0 && (n_steps == 0 || (load_scale && dirichlet_scale)), "fs_wave_advance: %lld steps need load_scale and "
               "dirichlet_scale of that length", (long long)n_steps);
    FS_REQUIRE(n_receivers >= 0 && n_receivers <= INT32_MAX && (n_receivers == 0 || receiver_dofs), "fs_wave_advance: receiver list: null "
               "pointer or bad count");
    const int64_t n = st->n;
    for (int64_t r = 0; r < n_receivers; ++r)
        FS_REQUIRE(receiver_dofs[r] >= 0 && receiver_dofs[r] < n, "fs_wave_advance: receiver dof %d outside the space of %lld dofs",
                   receiver_dofs[r], (long long)n);
    const bool want_traces = traces && n_receivers > 0;
    hipStream_t s = fs_rt().stream;
    if (want_traces) FS_CHECK(wave_set_receivers(st, n_receivers, receiver_dofs, s));
    FS_CHECK(fs_spmv_prepare(K, s));
    dbuf<double> tr, en;
    dbuf<unsigned long long> bad;
    FS_CHECK(en.alloc(2 * n_steps));
    FS_CHECK(bad.alloc(2));
    if (want_traces) FS_CHECK(tr.alloc(n_steps * n_receivers));
    FS_HIP(hipMemsetAsync(bad.p, 0, sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(bad.p + 1, 0xff, sizeof(unsigned long long), s));
    const int g = wave_grid(n);
    const double dt = st->dt, idt = 1.0 / dt, idt2 = 1.0 / (dt * dt), hidt = 1.0 / (2.0 * dt);
    FS_HIP(hipEventRecord(st->ev[0], s));
    for (int64_t k = 0; k < n_steps; ++k) {
        const int64_t slot = k % FS_WAVE_CHUNK;
        FS_CHECK(fs_spmv_dev(K, st->u.p, st->y.p, s));
        hipLaunchKernelGGL(k_wave_update, dim3(g), dim3(FS_BLOCK), 0, s, n, st->y.p, st->u.p, st->up.p, st->m.p, st->d.p, st->load.p, st->flag.p,
                           idt, idt2, hidt, load_scale[k], dirichlet_scale[k], st->w.p, (int)n_receivers, st->rec.p,
                           want_traces ? tr.p + k * n_receivers : nullptr, st->part.p + slot * 2 * g);
        // (u^{n-1}, u^n, work) <- (u^n, u^{n+1}, u^{n-1})
        st->up.swap(st->u);
        st->u.swap(st->w);
        ++st->step;
        if (slot == FS_WAVE_CHUNK - 1 || k == n_steps - 1) {
            hipLaunchKernelGGL(k_wave_finish, dim3((int)slot + 1), dim3(FS_BLOCK), 0, s, g, st->part.p, k - slot, en.p, bad.p);
            FS_KERNEL_CHECK();
        }
    }
    FS_HIP(hipEventRecord(st->ev[1], s));
    if (!(want_traces || energy || info)) return FS_OK;        // nothing to hand back: the batch stays in flight
    unsigned long long bad_host[2] = {0, 0};
    if (info) FS_CHECK(bad.download(bad_host, 2, s));
    if (want_traces) FS_CHECK(tr.download(traces, n_steps * n_receivers, s));
    if (energy) FS_CHECK(en.download(energy, 2 * n_steps, s));
    FS_HIP(hipStreamSynchronize(s));
    FS_KERNEL_CHECK();
    if (info) {
        float ms = 0.0f;
        FS_HIP(hipEventElapsedTime(&ms, st->ev[0], st->ev[1]));
        info->device_ms = ms;
        info->n_nonfinite = (int64_t)bad_host[0];
        info->first_nonfinite_step = bad_host[0] ? (int64_t)bad_host[1] : -1;
        info->step = st->step;
    }
    return FS_OK;
}
