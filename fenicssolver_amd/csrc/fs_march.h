// Scaffolding shared by the per-row time marchers (fs_wave.hip, fs_dynamics_explicit.hip, fs_dynamics.hip, fs_hyper_dynamics.hip): everything of a marcher
// that is not its update formula.  Header-only; every translation unit keeps its own copy of the one kernel.
//
//   row table      F with the Dirichlet values g in the slots of the Dirichlet rows, one flag byte per row (bit 0: Dirichlet row, bit 1: a
//                  row some receiver samples - only such a row searches the receiver list) and the receiver list.  The receiver bits
//                  follow the list of the last call that wanted samples and are uploaded only when that list changes.
//   batch driver   fs_march_advance: n_steps steps enqueued back to back, the host touches nothing in between.  Step k leaves its
//                  [2][grid] per-workgroup partials of both energy halves in slot k % FS_MARCH_CHUNK of the partial table; after every
//                  FS_MARCH_CHUNK steps k_march_finish, one workgroup per step, sums them in a fixed order into the energy table of
//                  the call and counts the steps whose energy is not finite (integer atomics: the count and the first such step do
//                  not depend on the order).  No floating-point atomics: a march gives the same bits however it is split into calls.
//   checks         the refusals the entry points share; `who` is the entry point the message names.
// Nothing here sets fp contraction, and the device helpers do no floating-point arithmetic beyond fs_block_sum.
#pragma once
#include "fs_common.h"
#include "fs_kernels.h"
#include <math.h>
#include <string.h>

#define FS_MARCH_BLOCKS 1024             // most workgroups of a pointwise kernel (its energy partials are summed in this order)
#define FS_MARCH_CHUNK 64                // steps between two finishing passes (the partial table holds this many steps)
#define FS_MARCH_DIRICHLET 1
#define FS_MARCH_RECEIVER 2

static inline int fs_march_grid(int64_t n) { return fs_grid_for(n, FS_BLOCK, FS_MARCH_BLOCKS); }

// ---- device helpers ----------------------------------------------------------------------------------------------------------
// the tail of an energy kernel: part = this launch's [2][gridDim.x] partials
__device__ __forceinline__ void fs_march_store_partials(double ek, double ep, double* lds4, double* __restrict__ part) {
    const double tk = fs_block_sum(ek, lds4);
    const double tp = fs_block_sum(ep, lds4);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = tk;
        part[gridDim.x + blockIdx.x] = tp;
    }
}

// row i with flag byte fl took the value un; trace: this step's [n_rec] samples (nullptr: none wanted)
__device__ __forceinline__ void fs_march_sample(int fl, int64_t i, double un, int n_rec, const int32_t* __restrict__ rec,
                                                double* __restrict__ trace) {
    if ((fl & FS_MARCH_RECEIVER) && trace)
        for (int r = 0; r < n_rec; ++r)
            if (rec[r] == (int32_t)i) trace[r] = un;
}

// workgroup b: step k0 + b of the call, whose partials are part[b][2][g]; bad = (steps with a non-finite energy, the first of them)
// (a template so that only a file that launches it gets a copy)
template <int = 0>
__global__ void __launch_bounds__(FS_BLOCK) k_march_finish(int g, const double* __restrict__ part, int64_t k0, double* __restrict__ energy,
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

// ---- shared checks -----------------------------------------------------------------------------------------------------------
static inline int fs_march_one_rank(const fs_space_s* sp, const char* who) {
    const fs_mesh_s* m = sp->mesh;
    FS_REQUIRE(fs_rt().n_ranks == 1 && m->n_owned == m->nv && sp->n_nodes_owned == sp->n_nodes_local,
               "%s: the space has ghost nodes or the communicator several ranks: not supported", who);
    return FS_OK;
}

static inline int fs_march_receivers_ok(const char* who, int64_t n, int64_t n_receivers, const int32_t* receiver_dofs) {
    FS_REQUIRE(n_receivers >= 0 && n_receivers <= INT32_MAX && (n_receivers == 0 || receiver_dofs), "%s: receiver list: null pointer or bad "
               "count", who);
    for (int64_t r = 0; r < n_receivers; ++r)
        FS_REQUIRE(receiver_dofs[r] >= 0 && receiver_dofs[r] < n, "%s: receiver dof %d outside the space of %lld dofs", who, receiver_dofs[r],
                   (long long)n);
    return FS_OK;
}

// what *_state_configure checks before it touches the Dirichlet list: the pointers of the list and the per-row arrays (mass, damping,
// load: nullptr = the marcher has none)
static inline int fs_march_rows_ok(const char* who, int64_t n, const double* mass, const double* damping, const double* load,
                                   int64_t n_dirichlet, const int32_t* dirichlet_dofs, const double* dirichlet_values) {
    FS_REQUIRE(n_dirichlet >= 0 && (n_dirichlet == 0 || (dirichlet_dofs && dirichlet_values)), "%s: Dirichlet list: null pointer or negative "
               "count", who);
    for (int64_t i = 0; i < n; ++i) {
        FS_REQUIRE(!mass || (mass[i] > 0.0 && isfinite(mass[i])), "%s: the lumped mass of row %lld is %g: m_i > 0 is required", who, (long long)i,
                   mass ? mass[i] : 0.0);
        FS_REQUIRE(!damping || (damping[i] >= 0.0 && isfinite(damping[i])), "%s: the damping of row %lld is %g: d_i >= 0 is required", who,
                   (long long)i, damping ? damping[i] : 0.0);
        FS_REQUIRE(!load || isfinite(load[i]), "%s: the load of row %lld is not finite", who, (long long)i);
    }
    return FS_OK;
}

// ---- the row table -----------------------------------------------------------------------------------------------------------
struct fs_march_rows {
    int64_t n = 0;                       // rows
    dbuf<double> load;                   // F (Dirichlet rows: g)
    dbuf<uint8_t> flag;
    std::vector<uint8_t> flag_host;      // the Dirichlet bits; the receiver bits of `receivers` on top
    std::vector<int32_t> receivers;      // the list whose bits the device flags carry now
    dbuf<int32_t> rec;

    int alloc_rows(int64_t rows, hipStream_t s) {
        n = rows;
        FS_CHECK(load.alloc(n));
        FS_CHECK(load.zero(s));
        FS_CHECK(flag.alloc(n));
        FS_CHECK(flag.zero(s));
        flag_host.assign((size_t)n, 0);
        return FS_OK;
    }

    // load: nullptr = none.  Nothing is uploaded before every dof and value has passed; the uploads wait for the device.
    int configure(const char* who, const double* load_host, int64_t n_dirichlet, const int32_t* dofs, const double* vals, hipStream_t s) {
        std::vector<double> f(load_host ? load_host : nullptr, load_host ? load_host + n : nullptr);
        f.resize((size_t)n, 0.0);
        std::vector<uint8_t> fl((size_t)n, 0);
        for (int64_t j = 0; j < n_dirichlet; ++j) {
            const int32_t i = dofs[j];
            FS_REQUIRE(i >= 0 && i < n, "%s: Dirichlet dof %d outside the space of %lld dofs", who, i, (long long)n);
            FS_REQUIRE(isfinite(vals[j]), "%s: the Dirichlet value of dof %d is not finite", who, i);
            fl[i] = FS_MARCH_DIRICHLET;
            f[i] = vals[j];                   // (a dof named twice takes the last value)
        }
        FS_CHECK(load.upload(f.data(), n, s));
        FS_CHECK(flag.upload(fl.data(), n, s));
        flag_host.swap(fl);
        receivers.clear();
        return FS_OK;
    }

    // the receiver bits of the device flags follow the list of the call (uploaded only when the list changes)
    int set_receivers(int64_t n_rec, const int32_t* dofs, hipStream_t s) {
        if ((int64_t)receivers.size() == n_rec && (n_rec == 0 || !memcmp(receivers.data(), dofs, (size_t)n_rec * sizeof(int32_t)))) return FS_OK;
        for (int32_t i : receivers) flag_host[i] &= (uint8_t)~FS_MARCH_RECEIVER;
        receivers.assign(dofs, dofs + n_rec);
        for (int32_t i : receivers) flag_host[i] |= FS_MARCH_RECEIVER;
        FS_CHECK(flag.upload(flag_host.data(), n, s));
        if (n_rec) {
            FS_CHECK(rec.alloc(n_rec));
            FS_CHECK(rec.upload(dofs, n_rec, s));
        }
        return FS_OK;
    }
};

// ---- the state objects -------------------------------------------------------------------------------------------------------
template <int N>
struct fs_march_events {
    hipEvent_t ev[N] = {};
    ~fs_march_events() {
        for (hipEvent_t e_ : ev)
            if (e_) (void)hipEventDestroy(e_);
    }
};

// the end of every *_state_create.  rc: what the allocations gave; then the events and the wait for the zeroing.  A state that
// failed anywhere is deleted.
template <class State>
static inline int fs_march_create_finish(const char* who, State* st, int rc, hipStream_t s, State** out) {
    for (hipEvent_t& e_ : st->ev)
        if (rc == FS_OK && hipEventCreate(&e_) != hipSuccess) {
            fs_set_error("%s: hipEventCreate failed", who);
            rc = FS_ERR_HIP;
        }
    if (rc == FS_OK && hipStreamSynchronize(s) != hipSuccess) {
        fs_set_error("%s: hipStreamSynchronize failed", who);
        rc = FS_ERR_HIP;
    }
    if (rc != FS_OK) {
        delete st;
        return rc;
    }
    *out = st;
    return FS_OK;
}

// what the batch driver needs of a state: the two explicit marchers derive theirs from it
struct fs_march_batch_state : fs_march_rows, fs_march_events<2> {
    fs_space_s* space = nullptr;
    bool configured = false;
    int64_t step = 0;                    // the n of the fields the state holds; 0: not started
    dbuf<double> part;                   // [FS_MARCH_CHUNK][2][grid]
    int alloc_part() { return part.alloc((int64_t)FS_MARCH_CHUNK * 2 * fs_march_grid(n)); }
};

// ---- the batch driver --------------------------------------------------------------------------------------------------------
// Everything of a *_advance that is not the step.  enqueue(k, trace, part) puts the product and the update kernel of step k of the call
// on the stream - trace: that step's [n_receivers] samples or nullptr, part: its [2][grid] partials -, advances the state's fields
// and its step counter and returns FS_OK or what failed.  finite_factors: refuse time factors that are not finite.
template <class Enqueue>
static inline int fs_march_advance(const char* who, fs_matrix_s* K, fs_march_batch_state* st, bool finite_factors, int64_t n_steps,
                                   const double* load_scale, const double* dirichlet_scale, int64_t n_receivers, const int32_t* receiver_dofs,
                                   double* traces, double* energy, fs_march_info* info, Enqueue&& enqueue) {
    FS_REQUIRE(n_steps >= 0 && (n_steps == 0 || (load_scale && dirichlet_scale)), "%s: %lld steps need load_scale and dirichlet_scale of "
               "that length", who, (long long)n_steps);
    FS_CHECK(fs_march_receivers_ok(who, st->n, n_receivers, receiver_dofs));
    for (int64_t k = 0; finite_factors && k < n_steps; ++k)
        FS_REQUIRE(isfinite(load_scale[k]) && isfinite(dirichlet_scale[k]), "%s: the time factors of step %lld of the call are not finite", who,
                   (long long)k);
    const bool want_traces = traces && n_receivers > 0;
    hipStream_t s = fs_rt().stream;
    if (want_traces) FS_CHECK(st->set_receivers(n_receivers, receiver_dofs, s));
    if (K) FS_CHECK(fs_spmv_prepare(K, s));                    // (nullptr: a marcher whose step has no product)
    dbuf<double> tr, en;
    dbuf<unsigned long long> bad;
    FS_CHECK(en.alloc(2 * n_steps));
    FS_CHECK(bad.alloc(2));
    if (want_traces) FS_CHECK(tr.alloc(n_steps * n_receivers));
    FS_HIP(hipMemsetAsync(bad.p, 0, sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(bad.p + 1, 0xff, sizeof(unsigned long long), s));
    const int g = fs_march_grid(st->n);
    FS_HIP(hipEventRecord(st->ev[0], s));
    for (int64_t k = 0; k < n_steps; ++k) {
        const int64_t slot = k % FS_MARCH_CHUNK;
        FS_CHECK(enqueue(k, want_traces ? tr.p + k * n_receivers : nullptr, st->part.p + slot * 2 * g));
        if (slot == FS_MARCH_CHUNK - 1 || k == n_steps - 1) {
            hipLaunchKernelGGL(k_march_finish<>, dim3((int)slot + 1), dim3(FS_BLOCK), 0, s, g, st->part.p, k - slot, en.p, bad.p);
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
