// bsk_population.hip — the fitness of a population rollout, formed on the device (bsk_population_rollout; definition in
// include/bskgpu.h):
//   fitness_row_kernel    row t of the rollout's histories AND one step of every env's value rule, one launch per env step
//   fitness_join_kernel   one wave per member: the per-member mean of the values and of the episode lengths, in a fixed order
//   outcome_row_kernel, outcome_join_kernel   bsk_population_set_outcomes: the same launch per env step with the outcome rule behind
//                         the value rule, and one wave per member for the row of counts, sum of squares, minimum and maximum
// Compiled with -ffp-contract=off (Makefile), as bsk_fork.hip is: the additions and products are the ones a numpy restatement makes.
#include "bsk_population.hpp"

#include "../../include/bskgpu.h"
#include "bsk_tree.hpp"

namespace bsk {

// The per-env rule is bsk_select_branches' (bsk_fork.hip: select_kernel), one step per launch: while alive
//   v = v + g * reward;  len += 1;  g = g * gamma;  alive ends after the first step with reason != 0 (that step's reward included)
// - product and sum each rounded on their own.  With BSK_FLAG_AUTO_RESET the env goes on stepping; its later episodes find alive = 0.
// ONE statement of it, for fitness_row_kernel and outcome_row_kernel: the history rows of env i and its step of the rule
// -> whether env i was alive BEFORE this step (false for i >= n).
__device__ __forceinline__ bool fitness_row_step(int i, const double* __restrict__ obs, const double* __restrict__ reward,
                                                 const unsigned char* __restrict__ reason, int64_t stride, int n,
                                                 double* __restrict__ obs_row, double* __restrict__ reward_row,
                                                 unsigned char* __restrict__ reason_row, const FitnessAcc& acc, double gamma, int first,
                                                 unsigned char& q) {
#pragma clang fp contract(off)
    if (i >= n) return false;
    if (obs_row) {
#pragma unroll
        for (int k = 0; k < 5; ++k) obs_row[(int64_t)k * n + i] = obs[(int64_t)k * stride + i];
    }
    const double r = reward[i];
    q = reason[i];
    if (reward_row) reward_row[i] = r;
    if (reason_row) reason_row[i] = q;
    const bool alive = first || acc.alive[i] != 0;
    if (!alive) return false;
    const double v = first ? 0.0 : acc.v[i];
    const double g = first ? 1.0 : acc.g[i];
    const int len = first ? 0 : acc.len[i];
    const double p = g * r;
    acc.v[i] = v + p;
    acc.g[i] = g * gamma;
    acc.len[i] = len + 1;
    if (first || q != 0) acc.alive[i] = q != 0 ? 0 : 1;
    return true;
}

__global__ __launch_bounds__(256) void fitness_row_kernel(const double* __restrict__ obs, const double* __restrict__ reward,
                                                          const unsigned char* __restrict__ reason, int64_t stride, int n,
                                                          double* __restrict__ obs_row, double* __restrict__ reward_row,
                                                          unsigned char* __restrict__ reason_row, const FitnessAcc acc, double gamma,
                                                          int first) {
    unsigned char q = 0;
    (void)fitness_row_step(blockIdx.x * blockDim.x + threadIdx.x, obs, reward, reason, stride, n, obs_row, reward_row, reason_row, acc,
                           gamma, first, q);
}

// The outcome rule (include/bskgpu.h, bsk_population_set_outcomes) behind the value rule, for an env that was alive before this
// step: act_n[a] += 1 and, where the step ended the episode, end_reason = the reason byte.  At step 0 the accumulators are not read
// but written whole (act_n = 0 but for the action taken, end_reason = the byte, 0 included).  An action outside 0..2 - the policy
// kernel writes none - is counted nowhere: nothing is addressed by it.
__global__ __launch_bounds__(256) void outcome_row_kernel(const double* __restrict__ obs, const double* __restrict__ reward,
                                                          const unsigned char* __restrict__ reason, const int* __restrict__ action,
                                                          int64_t stride, int n, double* __restrict__ obs_row,
                                                          double* __restrict__ reward_row, unsigned char* __restrict__ reason_row,
                                                          const FitnessAcc acc, const OutcomeAcc out, double gamma, int first) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned char q = 0;
    if (!fitness_row_step(i, obs, reward, reason, stride, n, obs_row, reward_row, reason_row, acc, gamma, first, q)) return;
    const int a = action[i];
    if (first) {
        // (the same rule as below, written as an initialisation: an action outside 0..2 matches no k and leaves three zeros)
#pragma unroll
        for (int k = 0; k < 3; ++k) out.act_n[(int64_t)k * n + i] = a == k ? 1 : 0;
        out.end_reason[i] = q;
        return;
    }
    if ((unsigned)a < 3u) out.act_n[(int64_t)a * n + i] += 1;
    if (q != 0) out.end_reason[i] = q;
}

hipError_t launch_fitness_row(const double* obs, const double* reward, const unsigned char* reason, int64_t stride, int n, double* obs_row,
                              double* reward_row, unsigned char* reason_row, const FitnessAcc& acc, double gamma, bool first,
                              hipStream_t s) {
    hipLaunchKernelGGL(fitness_row_kernel, dim3((n + 255) / 256), dim3(256), 0, s, obs, reward, reason, stride, n, obs_row, reward_row,
                       reason_row, acc, gamma, first ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_outcome_row(const double* obs, const double* reward, const unsigned char* reason, const int* action, int64_t stride, int n,
                              double* obs_row, double* reward_row, unsigned char* reason_row, const FitnessAcc& acc, const OutcomeAcc& out,
                              double gamma, bool first, hipStream_t s) {
    hipLaunchKernelGGL(outcome_row_kernel, dim3((n + 255) / 256), dim3(256), 0, s, obs, reward, reason, action, stride, n, obs_row,
                       reward_row, reason_row, acc, out, gamma, first ? 1 : 0);
    return hipGetLastError();
}

// Member m is the envs m * E .. m * E + E - 1 (E a multiple of 64).  Lane l adds its elements l, l + 64, l + 128, ... in ascending
// order, starting FROM the first (not from zero: -0.0 stays -0.0); then s[l] = s[l] + s[l + stride] for l < stride, stride = 32, 16,
// ..., 1 (fitness_tree, bsk_tree.hpp); the mean is s[0] / E.  No atomics, no dependence on the launch shape: numpy repeats it
// (policy_ref.py: population_fitness_ref).
__global__ __launch_bounds__(256) void fitness_join_kernel(const FitnessAcc acc, int n_members, int E, double* __restrict__ env_value,
                                                           int* __restrict__ env_len, double* __restrict__ fitness,
                                                           double* __restrict__ mean_len) {
#pragma clang fp contract(off)
    const int m = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));     // (wave-uniform)
    const int lane = (int)(threadIdx.x & 63u);
    if (m >= n_members) return;
    const int64_t at0 = (int64_t)m * E + lane;
    double sv = 0.0, sl = 0.0;
    for (int c = 0; c < E; c += 64) {
        const double v = acc.v[at0 + c];
        const int len = acc.len[at0 + c];
        if (env_value) env_value[at0 + c] = v;
        if (env_len) env_len[at0 + c] = len;
        sv = c == 0 ? v : sv + v;
        sl = c == 0 ? (double)len : sl + (double)len;
    }
    sv = fitness_tree(sv, lane);
    sl = fitness_tree(sl, lane);
    if (lane == 0) {
        if (fitness) fitness[m] = sv / (double)E;
        if (mean_len) mean_len[m] = sl / (double)E;
    }
}

hipError_t launch_fitness_join(const FitnessAcc& acc, int n_members, int envs_per_member, double* env_value, int* env_len,
                               double* fitness, double* mean_len, hipStream_t s) {
    if (!env_value && !env_len && !fitness && !mean_len) return hipSuccess;
    hipLaunchKernelGGL(fitness_join_kernel, dim3((n_members + 3) / 4), dim3(256), 0, s, acc, n_members, envs_per_member, env_value,
                       env_len, fitness, mean_len);
    return hipGetLastError();
}

// One wave per member (fitness_join_kernel's shape and walk: lane l takes the envs l, l + 64, ... of the member, ascending):
// row m of include/bskgpu.h.  The counts are integers until lane 0 converts them; v * v, the sum and the two extremes are f64 in
// the fitness's order.  No atomics, no dependence on the launch shape: numpy repeats it (policy_ref.py: population_outcomes_ref).
__global__ __launch_bounds__(256) void outcome_join_kernel(const FitnessAcc acc, const OutcomeAcc out, int n_members, int E,
                                                           double* __restrict__ rows) {
#pragma clang fp contract(off)
    const int m = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));     // (wave-uniform)
    const int lane = (int)(threadIdx.x & 63u);
    if (m >= n_members) return;
    const int64_t n = (int64_t)n_members * E;
    const int64_t at0 = (int64_t)m * E + lane;
    long long cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double sq = 0.0, lo = 0.0, hi = 0.0;
    for (int c = 0; c < E; c += 64) {
        const double v = acc.v[at0 + c];
        const unsigned q = out.end_reason[at0 + c];
        cnt[0] += (q & BSK_DONE_LENGTH) ? 1 : 0;
        cnt[1] += (q & BSK_DONE_WHEELS) ? 1 : 0;
        cnt[2] += (q & BSK_DONE_BATTERY) ? 1 : 0;
        cnt[3] += (q & BSK_DONE_ORBIT) ? 1 : 0;
        cnt[4] += q == 0 ? 1 : 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) cnt[5 + k] += out.act_n[k * n + at0 + c];
        const double x = v * v;
        sq = c == 0 ? x : sq + x;
        lo = c == 0 ? v : extreme_pick<false>(lo, v);
        hi = c == 0 ? v : extreme_pick<true>(hi, v);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) cnt[k] = count_tree(cnt[k], lane);
    sq = fitness_tree(sq, lane);
    lo = extreme_tree<false>(lo, lane);
    hi = extreme_tree<true>(hi, lane);
    if (lane != 0) return;
    double* row = rows + (int64_t)m * BSK_OUTCOME_COLS;
#pragma unroll
    for (int k = 0; k < 8; ++k) row[k] = (double)cnt[k];
    row[8] = sq;
    row[9] = lo;
    row[10] = hi;
}

hipError_t launch_outcome_join(const FitnessAcc& acc, const OutcomeAcc& out, int n_members, int envs_per_member, double* rows,
                               hipStream_t s) {
    hipLaunchKernelGGL(outcome_join_kernel, dim3((n_members + 3) / 4), dim3(256), 0, s, acc, out, n_members, envs_per_member, rows);
    return hipGetLastError();
}

}  // namespace bsk
