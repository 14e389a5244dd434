// bsk_pgsched.hpp — schedules of the policy-gradient loop's hyper-parameters and a KL stop per update, on the device
// (bsk_fit_set_schedule, bsk_fit_schedule_begin, bsk_fit_kl_gate, bsk_fit_schedule_end; definition in include/bskgpu.h; kernels in
// bsk_pgsched.hip; internal).  lr, clip, clip_vf and ent_coef "now" live in eight device words the fit owns, beside the iteration
// they were formed from and the gate of the KL stop, so that a replayed graph carries them: the scheduled instantiations of the fit's
// kernels (bsk_fit.hip) read the words where the others read their arguments.
// pg_sched_value - the rule - and pg_kl_gate_sums / pg_kl_gate_apply - the gate's walk over a minibatch's diagnostics rows and its
// decision - are plain C++: tools/pg_sched_host.cpp compiles them for the host (BSK_PGSCHED_HOST: no HIP header, no qualifier;
// bsk_rewnorm.hpp's pattern) and tests/test_pg_sched_host.py holds them to the restatement (policy_ref.py: pg_schedule_ref,
// fit_kl_gate_ref) before a GPU runs them; the C-ABI forms the words of bsk_fit_set_schedule with the same text.  Every f64
// operation is rounded on its own: no FMA.
#pragma once
#include <stdint.h>

#ifdef BSK_PGSCHED_HOST
#define BSK_PGSCHED_FN inline
#else
#include <hip/hip_runtime.h>
#define BSK_PGSCHED_FN __host__ __device__ __forceinline__
#endif

namespace bsk {

constexpr int PG_SCHED_WORDS = 8;          // BSK_FIT_SCHEDULE_WORDS: the words of the fit's schedule block
constexpr int PG_SCHED_LOG_COLS = 8;       // BSK_SCHED_LOG_COLS: the words of one row of the schedule's ring
constexpr int PG_SCHED_DIAG_COLS = 8;      // the doubles of one diagnostics row the gate reads: the loop's `log` layout
// the words of the block
enum { PG_SCHED_LR = 0, PG_SCHED_CLIP, PG_SCHED_CLIP_VF, PG_SCHED_ENT_COEF, PG_SCHED_ITERATION, PG_SCHED_GATE, PG_SCHED_SKIPPED, PG_SCHED_KL };

// What the host side holds: a pair (a, b) per word 0 .. 3, in the words' order, and the iterations the run from a to b takes
struct PgSchedPairs {
    double a[4], b[4];
    unsigned long long total;              // below 2^53: (double)total is exact
};

// The rule: a at the start (and with no run at all), b - exactly, not a + (b - a) - from `total` on, a line between
BSK_PGSCHED_FN double pg_sched_value(unsigned long long it, unsigned long long total, double a, double b) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (total == 0ull || it == 0ull) return a;
    if (it >= total) return b;
    const double frac = (double)it / (double)total;
    const double span = b - a;
    const double step = span * frac;
    return a + step;
}

// S: column 0 (kl_sum) and N: column 7 (count) of n_rows >= 1 rows of PG_SCHED_DIAG_COLS doubles, each summed ascending FROM the first row
BSK_PGSCHED_FN void pg_kl_gate_sums(const double* rows, int n_rows, double& S, double& N) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    S = rows[0];
    N = rows[PG_SCHED_DIAG_COLS - 1];
    for (int r = 1; r < n_rows; ++r) {
        S = S + rows[(size_t)PG_SCHED_DIAG_COLS * (size_t)r];
        N = N + rows[(size_t)PG_SCHED_DIAG_COLS * (size_t)r + (PG_SCHED_DIAG_COLS - 1)];
    }
}

// The decision on the three words {gate, skipped, kl_at_stop} -> whether the gate is closed behind it (the caller then drops the
// accumulation).  A closed gate stays closed; an open one closes when samples counted and the mean is not <= kl_stop - a NaN closes,
// a mean exactly at kl_stop does not -, and only that transition writes the mean.
BSK_PGSCHED_FN bool pg_kl_gate_apply(double S, double N, double kl_stop, unsigned long long& gate, unsigned long long& skipped, double& kl_at) {
    const double mean = S / N;
    if (gate == 0ull && N > 0.0 && !(mean <= kl_stop)) {
        gate = 1ull;
        kl_at = mean;
    }
    if (gate != 0ull) skipped += 1ull;
    return gate != 0ull;
}

#ifndef BSK_PGSCHED_HOST
// words 0 .. 3 out of word 4 by the rule; gate = 0, skipped = 0, kl_at_stop = +0.0: one thread
hipError_t launch_pg_sched_begin(unsigned long long* words, const PgSchedPairs& pairs, hipStream_t s);
// the gate over diag f64[n_rows][8]; closed: *count = 0 (the fit's), so that the step behind it moves nothing: one wave
hipError_t launch_fit_kl_gate(const double* diag, int n_rows, double kl_stop, unsigned long long* words, unsigned long long* count,
                              hipStream_t s);
// ring (or NULL) [iteration % capacity] = the row of the eight columns; iteration += 1: one thread
hipError_t launch_pg_sched_end(unsigned long long* words, double* ring, int capacity, hipStream_t s);
#endif

}  // namespace bsk
