// bsk_pgsched.hip — the three small launches around a scheduled update of the policy fit (bsk_fit_schedule_begin, bsk_fit_kl_gate,
// bsk_fit_schedule_end; definition in include/bskgpu.h).  Compiled with -ffp-contract=off: every f64 operation is rounded on its
// own, and numpy repeats all of it bit for bit (policy_ref.py: pg_schedule_ref, fit_kl_gate_ref).
//   pg_sched_begin_kernel   one thread: lr, clip, clip_vf and ent_coef of this iteration out of the iteration word by the rule
//                           (bsk_pgsched.hpp: pg_sched_value), the gate open, nothing skipped
//   fit_kl_gate_kernel      one wave, of which lane 0 walks: the two sums over a minibatch's diagnostics rows in their order - a
//                           handful of rows, 16 bytes each -, the decision (pg_kl_gate_apply) and, closed, the fit's count = 0: the
//                           step's launches behind it are then the no-op they already are with nothing accumulated
//   pg_sched_end_kernel     one thread: the iteration's row into the ring, the iteration word moves on
// No atomics, no LDS, plain stores.  The words are read by the fit's scheduled kernels (bsk_fit.hip) as uniform loads.
#include "bsk_pgsched.hpp"

namespace bsk {

__global__ void pg_sched_begin_kernel(unsigned long long* __restrict__ words, const PgSchedPairs p) {
#pragma clang fp contract(off)
    double* f = (double*)words;
    const unsigned long long it = words[PG_SCHED_ITERATION];
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = pg_sched_value(it, p.total, p.a[k], p.b[k]);
    words[PG_SCHED_GATE] = 0ull;
    words[PG_SCHED_SKIPPED] = 0ull;
    f[PG_SCHED_KL] = 0.0;
}

__global__ __launch_bounds__(64) void fit_kl_gate_kernel(const double* __restrict__ diag, int n_rows, double kl_stop,
                                                         unsigned long long* __restrict__ words, unsigned long long* __restrict__ count) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0) return;
    double S, N;
    pg_kl_gate_sums(diag, n_rows, S, N);
    unsigned long long gate = words[PG_SCHED_GATE], skipped = words[PG_SCHED_SKIPPED];
    double kl_at = ((const double*)words)[PG_SCHED_KL];
    if (pg_kl_gate_apply(S, N, kl_stop, gate, skipped, kl_at)) *count = 0ull;
    words[PG_SCHED_GATE] = gate;
    words[PG_SCHED_SKIPPED] = skipped;
    ((double*)words)[PG_SCHED_KL] = kl_at;
}

__global__ void pg_sched_end_kernel(unsigned long long* __restrict__ words, double* __restrict__ ring, int capacity) {
    const double* f = (const double*)words;
    const unsigned long long it = words[PG_SCHED_ITERATION];
    if (ring) {
        double* row = ring + (size_t)PG_SCHED_LOG_COLS * (size_t)(it % (unsigned long long)capacity);
        row[0] = (double)it;
        row[1] = f[PG_SCHED_LR];
        row[2] = f[PG_SCHED_CLIP];
        row[3] = f[PG_SCHED_CLIP_VF];
        row[4] = f[PG_SCHED_ENT_COEF];
        row[5] = (double)words[PG_SCHED_SKIPPED];
        row[6] = f[PG_SCHED_KL];
        row[7] = (double)words[PG_SCHED_GATE];
    }
    words[PG_SCHED_ITERATION] = it + 1ull;
}

hipError_t launch_pg_sched_begin(unsigned long long* words, const PgSchedPairs& pairs, hipStream_t s) {
    hipLaunchKernelGGL(pg_sched_begin_kernel, dim3(1), dim3(1), 0, s, words, pairs);
    return hipGetLastError();
}

hipError_t launch_fit_kl_gate(const double* diag, int n_rows, double kl_stop, unsigned long long* words, unsigned long long* count,
                              hipStream_t s) {
    hipLaunchKernelGGL(fit_kl_gate_kernel, dim3(1), dim3(64), 0, s, diag, n_rows, kl_stop, words, count);
    return hipGetLastError();
}

hipError_t launch_pg_sched_end(unsigned long long* words, double* ring, int capacity, hipStream_t s) {
    hipLaunchKernelGGL(pg_sched_end_kernel, dim3(1), dim3(1), 0, s, words, ring, capacity);
    return hipGetLastError();
}

}  // namespace bsk
