// bsk_pglog.hpp — the per-iteration training log of the policy-gradient loop (bsk_pg_episodes, bsk_pg_log_update,
// bsk_pg_log_advance; definition in include/bskgpu.h; kernels in bsk_pglog.hip; internal).  Episode returns and lengths are carried
// per env from rollout to rollout in two device arrays, so that an episode of 541 steps is followed across the many collect() calls
// it spans; everything else of a row is formed from one rollout's histories.
// pg_episode_walk - one env's column of the histories, rows ascending - is plain C++: tools/pg_episodes_host.cpp compiles it for the
// host (BSK_PGLOG_HOST: no HIP header, no qualifier; bsk_shuffle.hpp's pattern) and tests/test_pg_log_host.py holds it to the
// restatement (policy_ref.py: pg_episodes_walk_ref) before a GPU runs it.  Every f64 operation is rounded on its own: no FMA.
#pragma once
#include <stdint.h>

#ifdef BSK_PGLOG_HOST
#define BSK_PGLOG_FN inline
#else
#include <hip/hip_runtime.h>
#define BSK_PGLOG_FN __device__ __forceinline__
#endif

namespace bsk {

constexpr int PG_LOG_COLS = 26;            // BSK_PG_LOG_COLS: words of one ring row
constexpr int PG_EP_WORDS = 19;            // words of one wave's partial row in the work buffer: 7 sums, 2 extremes, 10 counts
constexpr int PG_EP_SUMS = 7, PG_EP_COUNTS = 10;
constexpr int PG_EP_BATCH = 8;             // rows of every history in flight at once

// What one column (and, behind the trees, one wave) holds.  The order of the members is the order of the 19 words.
enum { PG_S_R = 0, PG_S_R2, PG_S_REW, PG_S_Y, PG_S_Y2, PG_S_E, PG_S_E2 };        // s[]: returns of ended episodes and their squares,
                                                                                // all rewards, y, y^2, e, e^2
enum { PG_N_EP = 0, PG_N_LEN, PG_N_END, PG_N_ACT = PG_N_END + 4, PG_N_SAMPLES = PG_N_ACT + 3 };    // n[]: episodes ended, their lengths,
                                                                                // ends by reason bit, steps by action, rows walked
struct PgEpisodeAcc {
    double s[PG_EP_SUMS];                  // from +0.0
    double mn, mx;                         // from NaN ("nothing yet"): the least and the greatest return of an ended episode
    long long n[PG_EP_COUNTS];             // from 0
};

// bsk_tree.hpp's rule of the episode outcomes, restated here because that header is device code only: the candidate x replaces the
// incumbent m when it is smaller (MAX: greater) or the incumbent is a NaN
template <bool MAX>
BSK_PGLOG_FN double pg_extreme_pick(double m, double x) {
    return ((MAX ? x > m : x < m) || m != m) ? x : m;
}

BSK_PGLOG_FN void pg_episode_zero(PgEpisodeAcc& a) {
    for (int c = 0; c < PG_EP_SUMS; ++c) a.s[c] = 0.0;
    a.mn = a.mx = __builtin_nan("");
    for (int c = 0; c < PG_EP_COUNTS; ++c) a.n[c] = 0;
}

// One row of one column, in the order of the definition.  R, L: the running return and length of the env's current episode.
BSK_PGLOG_FN void pg_episode_row(PgEpisodeAcc& a, double& R, int32_t& L, double rew, uint8_t why, bool with_action, int32_t action,
                                 bool with_value, double y, float value) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    R = R + rew;
    L = L + 1;
    a.s[PG_S_REW] = a.s[PG_S_REW] + rew;
    a.n[PG_N_SAMPLES] += 1;
    if (with_action) {
        a.n[PG_N_ACT] += action == 0 ? 1 : 0;
        a.n[PG_N_ACT + 1] += action == 1 ? 1 : 0;
        a.n[PG_N_ACT + 2] += action == 2 ? 1 : 0;
    }
    if (with_value) {
        const double v = (double)value;
        const double e = y - v;
        a.s[PG_S_Y] = a.s[PG_S_Y] + y;
        a.s[PG_S_Y2] = a.s[PG_S_Y2] + y * y;
        a.s[PG_S_E] = a.s[PG_S_E] + e;
        a.s[PG_S_E2] = a.s[PG_S_E2] + e * e;
    }
    if (why != 0) {
        a.s[PG_S_R] = a.s[PG_S_R] + R;
        a.s[PG_S_R2] = a.s[PG_S_R2] + R * R;
        a.mn = pg_extreme_pick<false>(a.mn, R);
        a.mx = pg_extreme_pick<true>(a.mx, R);
        a.n[PG_N_EP] += 1;
        a.n[PG_N_LEN] += L;
        a.n[PG_N_END] += (why & 0x1) ? 1 : 0;           // BSK_DONE_LENGTH, _WHEELS, _BATTERY, _ORBIT: a byte with two bits counts in both
        a.n[PG_N_END + 1] += (why & 0x2) ? 1 : 0;
        a.n[PG_N_END + 2] += (why & 0x4) ? 1 : 0;
        a.n[PG_N_END + 3] += (why & 0x8) ? 1 : 0;
        R = 0.0;
        L = 0;
    }
}

// One column: the pointers are the histories' at row 0 of that column (action NULL: not counted; value and ret both or neither),
// rows `stride` elements apart.  PG_EP_BATCH rows of every history are fetched side by side and consumed in order - the chain is
// serial by definition, the loads are not - then the tail one by one.
BSK_PGLOG_FN void pg_episode_walk(const double* reward, const uint8_t* reason, const int32_t* action, const float* value, const double* ret,
                                  int n_steps, int64_t stride, double& R, int32_t& L, PgEpisodeAcc& a) {
    const bool with_action = action != nullptr, with_value = value != nullptr;
    int t = 0;
    for (; t + PG_EP_BATCH <= n_steps; t += PG_EP_BATCH) {
        double rew[PG_EP_BATCH], y[PG_EP_BATCH];
        uint8_t why[PG_EP_BATCH];
        int32_t act[PG_EP_BATCH];
        float v[PG_EP_BATCH];
#pragma unroll
        for (int i = 0; i < PG_EP_BATCH; ++i) {
            const int64_t at = (int64_t)(t + i) * stride;
            rew[i] = reward[at];
            why[i] = reason[at];
            act[i] = with_action ? action[at] : 0;
            v[i] = with_value ? value[at] : 0.0f;
            y[i] = with_value ? ret[at] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < PG_EP_BATCH; ++i) pg_episode_row(a, R, L, rew[i], why[i], with_action, act[i], with_value, y[i], v[i]);
    }
    for (; t < n_steps; ++t) {
        const int64_t at = (int64_t)t * stride;
        pg_episode_row(a, R, L, reward[at], reason[at], with_action, with_action ? action[at] : 0, with_value, with_value ? ret[at] : 0.0,
                       with_value ? value[at] : 0.0f);
    }
}

#ifndef BSK_PGLOG_HOST
struct PgEpisodesArgs {
    const double* reward;                  // histories [n_steps][stride]
    const uint8_t* reason;
    const int32_t* action;                 // or NULL
    const float* value;                    // value and ret: both or neither
    const double* ret;
    int n_steps, n_envs;
    int64_t stride;
    double* ep_return;                     // [n_envs]: the carried state
    int32_t* ep_len;
    double* work;                          // [ceil(n_envs / 64)][PG_EP_WORDS]
    double* ring;                          // [capacity][PG_LOG_COLS]
    int capacity;
    const unsigned long long* counter;     // or NULL: slot 0
};

// the walk and the per-wave partial rows, then the join and columns 0 .. 15 of the slot's row: two launches
hipError_t launch_pg_episodes(const PgEpisodesArgs& args, hipStream_t s);
// columns 16 .. 25 of the slot's row out of diag f64[n_rows][8] and norms f64[n_norms][2] (or NULL): one wave
hipError_t launch_pg_log_update(const double* diag, int n_rows, const double* norms, int n_norms, double* ring, int capacity,
                                const unsigned long long* counter, hipStream_t s);
// gen[counter % capacity] = counter; counter += 1: one thread
hipError_t launch_pg_log_advance(unsigned long long* gen, int capacity, unsigned long long* counter, hipStream_t s);
#endif

}  // namespace bsk
