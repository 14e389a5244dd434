// bsk_obsstats.hpp — running statistics of the observation rows, formed on the device (bsk_obsstats.hip; internal): what
// bsk_obs_stats_accumulate, the rollouts with a statistics object attached and bsk_es_apply_obs_norm launch.  Definition in
// include/bskgpu.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bsk {

// The device words of one statistics object, all zero after creation: per wave of 64 spacecraft w the sums part[w][0..4] and the
// sums of squares part[w][5..9] of the five observation rows and the number of observations cnt[w] behind them; their totals.
struct ObsStats {
    double* part;                  // [waves][10]
    unsigned long long* cnt;       // [waves]
    double* tot;                   // [10]
    unsigned long long* tot_n;     // [1]
    int waves;                     // ceil(n_cap / 64)
};

// One lane per spacecraft i < n (n <= 64 * st.waves): obs f64[5][stride] of those that count - all of them with alive == NULL,
// otherwise those with alive[i] != 0 - summed per wave in the fitness tree's order and added to part / cnt.  The totals are stale
// until launch_obs_stats_join has run behind it.
hipError_t launch_obs_stats(const double* obs, int64_t stride, int n, const unsigned char* alive, const ObsStats& st, hipStream_t s);
// Eleven waves: tot[c] and tot_n from ALL st.waves partial rows, in a fixed order
hipError_t launch_obs_stats_join(const ObsStats& st, hipStream_t s);
// Five threads: theta[k] = scale_k, theta[5 + k] = shift_k of the totals (nothing is written while tot_n == 0).  A row whose
// standard deviation is below std_min is switched off (scale 0), never multiplied by 1 / tiny: the rule of ARS (Mania et al. 2018).
hipError_t launch_es_obs_norm(const double* tot, const unsigned long long* tot_n, double std_min, double* theta, hipStream_t s);

// mean and variance of one row: var = E[x^2] - mean^2, clamped at zero (the difference of two rounded numbers can fall below it).
// One text for the observation rows (es_obs_norm_kernel) and the advantages of a minibatch (bsk_fit.hip: adv_join_kernel).
__host__ __device__ __forceinline__ void obs_moments(double sum, double sum_sq, unsigned long long count, double& mean, double& var) {
#pragma clang fp contract(off)
    const double N = (double)count;
    mean = sum / N;
    const double e2 = sum_sq / N;
    const double v = e2 - mean * mean;
    var = v > 0.0 ? v : 0.0;
}

// es_obs_norm_kernel's arithmetic on the host, compiled from the same text: mean = sum / N, var = max(sum_sq / N - mean * mean, 0)
// of one row out of its two totals and the count N > 0 (bsk_obs_stats_get)
void obs_moments_host(double sum, double sum_sq, unsigned long long count, double* mean, double* var);

}  // namespace bsk
