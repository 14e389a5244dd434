// bsk_rewnorm.hpp — rewards of the policy-gradient loop divided by the running standard deviation of the discounted return
// (bsk_reward_norm; definition in include/bskgpu.h; kernels in bsk_rewnorm.hip; internal): VecNormalize(norm_reward=True) of
// stable-baselines on the device.  Every env's running discounted return is carried from rollout to rollout in a device array, as
// bsk_pglog.hpp carries ep_return, since it spans the many collect() calls of an episode; the sums behind the deviation are
// carried in eight device words.
// reward_norm_walk - one env's column of the two histories, rows ascending - is plain C++: tools/reward_norm_host.cpp compiles it
// for the host (BSK_REWNORM_HOST: no HIP header, no qualifier; bsk_pglog.hpp's pattern) and tests/test_reward_norm_host.py holds it
// to the restatement (policy_ref.py: reward_norm_walk_ref) before a GPU runs it.  Every f64 operation is rounded on its own: no FMA.
#pragma once
#include <stdint.h>

#ifdef BSK_REWNORM_HOST
#define BSK_REWNORM_FN inline
#else
#include <hip/hip_runtime.h>
#define BSK_REWNORM_FN __device__ __forceinline__
#endif

namespace bsk {

constexpr int REWARD_NORM_STATE_WORDS = 8; // BSK_REWARD_NORM_STATE_WORDS: {sum, sum_sq, count, mean, var, sd, calls, 0}
constexpr int REWARD_NORM_WORK_WORDS = 3;  // words of one wave's partial row in the work buffer: a1, a2, k
constexpr int REWARD_NORM_BATCH = 8;       // rows of both histories in flight at once

// What one column (and, behind the trees, one wave) holds: the sum of the running returns, of their squares, and their number
struct RewardNormAcc {
    double a1, a2;                         // from +0.0
    long long k;                           // from 0
};

// One row of one column, in the order of the definition: the return is counted BEFORE an end resets it (VecNormalize's order)
BSK_REWNORM_FN void reward_norm_row(RewardNormAcc& a, double& R, double gamma, double rew, uint8_t why) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double carried = gamma * R;
    R = carried + rew;
    a.a1 = a.a1 + R;
    a.a2 = a.a2 + R * R;
    a.k += 1;
    if (why != 0) R = 0.0;
}

// One column: the pointers are the histories' at row 0 of that column, rows `stride` elements apart.  REWARD_NORM_BATCH rows of
// both histories are fetched side by side and consumed in order - the chain is serial by definition, the loads are not - then the
// tail one by one.
BSK_REWNORM_FN void reward_norm_walk(const double* reward, const uint8_t* reason, int n_steps, int64_t stride, double gamma, double& R,
                                     RewardNormAcc& a) {
    int t = 0;
    for (; t + REWARD_NORM_BATCH <= n_steps; t += REWARD_NORM_BATCH) {
        double rew[REWARD_NORM_BATCH];
        uint8_t why[REWARD_NORM_BATCH];
#pragma unroll
        for (int i = 0; i < REWARD_NORM_BATCH; ++i) {
            const int64_t at = (int64_t)(t + i) * stride;
            rew[i] = reward[at];
            why[i] = reason[at];
        }
#pragma unroll
        for (int i = 0; i < REWARD_NORM_BATCH; ++i) reward_norm_row(a, R, gamma, rew[i], why[i]);
    }
    for (; t < n_steps; ++t) {
        const int64_t at = (int64_t)t * stride;
        reward_norm_row(a, R, gamma, reward[at], reason[at]);
    }
}

// y = x / d, held to [-clip, clip]; a NaN passes through (both comparisons are false)
BSK_REWNORM_FN double reward_norm_scale(double x, double d, double clip) {
    const double y = x / d;
    return y > clip ? clip : (y < -clip ? -clip : y);
}

#ifndef BSK_REWNORM_HOST
struct RewardNormArgs {
    const double* reward;                  // histories [n_steps][stride]
    const uint8_t* reason;
    int n_steps, n_envs;
    int64_t stride;
    double gamma, eps, clip;
    bool update;
    double* ret_run;                       // [n_envs]: the carried returns (update only)
    double* state;                         // [REWARD_NORM_STATE_WORDS]
    double* work;                          // [ceil(n_envs / 64)][REWARD_NORM_WORK_WORDS] (update only)
    double* out;                           // [n_steps][stride]; may be `reward`
};

// update: the walk and the per-wave partial rows, the join into the state words; always: the apply.  Three launches, or one.
hipError_t launch_reward_norm(const RewardNormArgs& args, hipStream_t s);
#endif

}  // namespace bsk
