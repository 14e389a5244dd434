// bsk_obsstats.hip — running statistics of the five observation rows, formed on the device, and the input normalisation of a
// policy out of them (bsk_obs_stats_*, bsk_es_apply_obs_norm; definition in include/bskgpu.h):
//   obs_stats_kernel        one lane per spacecraft, one launch per accumulate: the sums and sums of squares of every wave of 64
//   obs_stats_join_kernel   eleven waves: the ten totals and the count out of all the partial rows
//   es_obs_norm_kernel      five threads: in_scale and in_shift of the optimiser's theta out of the totals
// All of it f64 + - * / and sqrt, every operation rounded on its own: compiled with -ffp-contract=off (Makefile), as
// bsk_population.hip and bsk_es.hip are.  No atomics, and no result depends on the launch shape: numpy repeats all of it bit for
// bit (policy_ref.py: obs_stats_accumulate_ref, obs_stats_totals_ref, obs_norm_ref).
#include "bsk_obsstats.hpp"

#include "bsk_tree.hpp"

namespace bsk {

// Wave w is the spacecraft 64 w .. 64 w + 63.  A lane counts when its spacecraft exists (i < n) and is alive (no mask: all are);
// a lane that does not count brings +0.0 to all ten trees.  Lane 0 adds the wave's sums to its partial row; a wave in which no
// lane counts stores nothing.
__global__ __launch_bounds__(256) void obs_stats_kernel(const double* __restrict__ obs, int64_t stride, int n,
                                                        const unsigned char* __restrict__ alive, const ObsStats st) {
#pragma clang fp contract(off)
    const int w = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));     // (wave-uniform)
    const int lane = (int)(threadIdx.x & 63u);
    if (w >= st.waves) return;
    const int64_t i = (int64_t)w * 64 + lane;
    const bool counts = i < (int64_t)n && (!alive || alive[i] != 0);
    const unsigned long long live = __ballot(counts);
    if (live == 0ull) return;
    double s1[5], s2[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double x = counts ? obs[(int64_t)k * stride + i] : 0.0;
        const double q = x * x;
        s1[k] = fitness_tree(x, lane);
        s2[k] = fitness_tree(q, lane);
    }
    if (lane == 0) {
        double* part = st.part + (size_t)w * 10;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            part[k] = part[k] + s1[k];
            part[5 + k] = part[5 + k] + s2[k];
        }
        st.cnt[w] = st.cnt[w] + (unsigned long long)__popcll(live);
    }
}

// Wave c < 10 is column c of the partial rows: lane l adds part[w][c] for w = l, l + 64, ... ascending, starting FROM the first
// (+0.0 with no element), then the tree.  Wave 10 sums cnt the same way in integers.  The other waves of a launch do nothing.
__global__ __launch_bounds__(64) void obs_stats_join_kernel(const ObsStats st) {
#pragma clang fp contract(off)
    const int c = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));     // (wave-uniform)
    const int lane = (int)(threadIdx.x & 63u);
    if (c < 10) {
        double s = 0.0;
        for (int w = lane; w < st.waves; w += 64) {
            const double v = st.part[(size_t)w * 10 + c];
            s = w == lane ? v : s + v;
        }
        s = fitness_tree(s, lane);
        if (lane == 0) st.tot[c] = s;
    } else if (c == 10) {
        unsigned long long s = 0ull;
        for (int w = lane; w < st.waves; w += 64) s = s + st.cnt[w];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_down(s, off, 64);
            if (lane < off) s = s + o;
        }
        if (lane == 0) st.tot_n[0] = s;
    }
}

// Thread k < 5 is row k.  scale = 1 / sd, or 0 where the row has not varied (sd < std_min): such a row - the fifth at the start of
// training - is switched off instead of being multiplied by 1 / tiny; shift = 0 - mean * scale moves the mean to zero.
__global__ void es_obs_norm_kernel(const double* __restrict__ tot, const unsigned long long* __restrict__ tot_n, double std_min,
                                   double* __restrict__ theta) {
#pragma clang fp contract(off)
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const unsigned long long count = tot_n[0];
    if (k >= 5 || count == 0ull) return;
    double mean, var;
    obs_moments(tot[k], tot[5 + k], count, mean, var);
    const double sd = sqrt(var);
    const double scale = sd >= std_min ? 1.0 / sd : 0.0;
    const double shift = 0.0 - mean * scale;
    theta[k] = scale;
    theta[5 + k] = shift;
}

void obs_moments_host(double sum, double sum_sq, unsigned long long count, double* mean, double* var) {
    obs_moments(sum, sum_sq, count, *mean, *var);
}

hipError_t launch_obs_stats(const double* obs, int64_t stride, int n, const unsigned char* alive, const ObsStats& st, hipStream_t s) {
    hipLaunchKernelGGL(obs_stats_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, obs, stride, n, alive, st);
    return hipGetLastError();
}

hipError_t launch_obs_stats_join(const ObsStats& st, hipStream_t s) {
    hipLaunchKernelGGL(obs_stats_join_kernel, dim3(11), dim3(64), 0, s, st);
    return hipGetLastError();
}

hipError_t launch_es_obs_norm(const double* tot, const unsigned long long* tot_n, double std_min, double* theta, hipStream_t s) {
    hipLaunchKernelGGL(es_obs_norm_kernel, dim3(1), dim3(5), 0, s, tot, tot_n, std_min, theta);
    return hipGetLastError();
}

}  // namespace bsk
