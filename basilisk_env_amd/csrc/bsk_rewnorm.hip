// bsk_rewnorm.hip — the rewards of a rollout divided by the running standard deviation of the discounted return and clipped, on
// the device (bsk_reward_norm; definition in include/bskgpu.h).  Compiled with -ffp-contract=off: every f64 operation is rounded
// on its own, and numpy repeats all of it bit for bit (policy_ref.py: reward_norm_ref).
//   reward_norm_walk_kernel   shaped like pg_episodes_kernel (bsk_pglog.hip): four waves per workgroup, wave w is the columns
//                             64 w .. 64 w + 63, a lane its env.  The lane carries its env's running discounted return in from
//                             ret_run, walks the rows ascending (bsk_rewnorm.hpp: reward_norm_walk, eight rows of both histories
//                             in flight, every load one coalesced row segment) and carries it out again; the wave joins its two
//                             sums and its count in the trees of bsk_tree.hpp and lane 0 WRITES them.  9 bytes read per sample,
//                             nothing written but 8 bytes per env and 24 per wave.  One env per lane: latency-bound, as gae_kernel.
//   reward_norm_join_kernel   one workgroup of three waves - the two sums and the count - under adv_join_kernel's rule: lane l the
//                             entries l, l + 64, ... ascending from the first, then the tree; one thread adds the totals to the
//                             carried sums and forms the eight state words.
//   reward_norm_apply_kernel  streaming, elementwise: a thread is one column below n_envs and strides over the rows, so a row
//                             segment is one coalesced load and one coalesced store and the padding is never touched; the divisor
//                             comes out of the state words once per thread.  8 bytes read and 8 written per sample.  A thread reads
//                             and writes its own element alone, so out may be the reward history.
// No atomics, no MFMA; LDS only hands the three totals to the thread that forms the state; plain stores.
#include "bsk_rewnorm.hpp"

#include "bsk_obsstats.hpp"
#include "bsk_tree.hpp"

namespace bsk {

constexpr int REWARD_NORM_APPLY_ROWS = 1024;       // rows of the apply launch's grid; a block strides over the rest

__global__ __launch_bounds__(256) void reward_norm_walk_kernel(const double* __restrict__ reward, const uint8_t* __restrict__ reason,
                                                               int n_steps, int n_envs, int64_t stride, double gamma,
                                                               double* __restrict__ ret_run, double* __restrict__ work, int waves) {
#pragma clang fp contract(off)
    const int w = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));     // (wave-uniform)
    const int lane = (int)(threadIdx.x & 63u);
    if (w >= waves) return;
    const int j = w * 64 + lane;
    RewardNormAcc a = {0.0, 0.0, 0};
    if (j < n_envs) {                      // a lane at or above n_envs reads nothing and writes nothing
        double R = ret_run[j];
        reward_norm_walk(reward + j, reason + j, n_steps, stride, gamma, R, a);
        ret_run[j] = R;
    }
    a.a1 = fitness_tree(a.a1, lane);
    a.a2 = fitness_tree(a.a2, lane);
    a.k = count_tree(a.k, lane);
    if (lane == 0) {
        double* out = work + (size_t)REWARD_NORM_WORK_WORDS * (size_t)w;
        out[0] = a.a1;
        out[1] = a.a2;
        ((long long*)out)[2] = a.k;
    }
}

__global__ __launch_bounds__(192) void reward_norm_join_kernel(const double* __restrict__ work, int waves, double eps,
                                                               double* __restrict__ state) {
#pragma clang fp contract(off)
    __shared__ double s_tot[2];
    __shared__ long long s_n;
    const int c = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63u);
    if (c < 2) {
        double s = 0.0;
        for (int w = lane; w < waves; w += 64) {
            const double v = work[(size_t)REWARD_NORM_WORK_WORDS * (size_t)w + c];
            s = w == lane ? v : s + v;
        }
        s = fitness_tree(s, lane);
        if (lane == 0) s_tot[c] = s;
    } else {
        const long long* cnt = (const long long*)work;
        long long s = 0;
        for (int w = lane; w < waves; w += 64) s += cnt[(size_t)REWARD_NORM_WORK_WORDS * (size_t)w + 2];
        s = count_tree(s, lane);
        if (lane == 0) s_n = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long* words = (unsigned long long*)state;
        const double sum = state[0] + s_tot[0];
        const double sum_sq = state[1] + s_tot[1];
        const unsigned long long count = words[2] + (unsigned long long)s_n;
        double mean, var;
        obs_moments(sum, sum_sq, count, mean, var);
        state[0] = sum;
        state[1] = sum_sq;
        words[2] = count;
        state[3] = mean;
        state[4] = var;
        state[5] = sqrt(var + eps);
        words[6] = words[6] + 1ull;
        words[7] = 0ull;
    }
}

__global__ __launch_bounds__(256) void reward_norm_apply_kernel(const double* reward, int n_steps, int n_envs, int64_t stride, double clip,
                                                                const double* __restrict__ state, double* out) {
#pragma clang fp contract(off)
    const int c = (int)(blockIdx.x * 256u + threadIdx.x);
    if (c >= n_envs) return;
    const double d = ((const unsigned long long*)state)[2] != 0ull ? state[5] : 1.0;
    for (int t = (int)blockIdx.y; t < n_steps; t += (int)gridDim.y) {
        const int64_t at = (int64_t)t * stride + c;
        out[at] = reward_norm_scale(reward[at], d, clip);
    }
}

hipError_t launch_reward_norm(const RewardNormArgs& p, hipStream_t s) {
    hipError_t e;
    if (p.update) {
        const int waves = (p.n_envs + 63) / 64;
        hipLaunchKernelGGL(reward_norm_walk_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, p.reward, p.reason, p.n_steps, p.n_envs,
                           p.stride, p.gamma, p.ret_run, p.work, waves);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(reward_norm_join_kernel, dim3(1), dim3(192), 0, s, (const double*)p.work, waves, p.eps, p.state);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const int rows = p.n_steps < REWARD_NORM_APPLY_ROWS ? p.n_steps : REWARD_NORM_APPLY_ROWS;
    hipLaunchKernelGGL(reward_norm_apply_kernel, dim3((unsigned)((p.n_envs + 255) / 256), (unsigned)rows), dim3(256), 0, s, p.reward, p.n_steps,
                       p.n_envs, p.stride, p.clip, (const double*)p.state, p.out);
    return hipGetLastError();
}

}  // namespace bsk
