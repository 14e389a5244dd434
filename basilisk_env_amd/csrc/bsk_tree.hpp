// bsk_tree.hpp — the 64-lane sum every fixed-order reduction of the library ends in (internal; device code only): one text for
// the fitness of a population rollout (bsk_population.hip) and the observation statistics (bsk_obsstats.hip), so that the order of
// the additions cannot diverge between them - and its twins for the counts and the extremes of the episode outcomes
// (bsk_population.hip, bsk_es.hip).  The units are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace bsk {

// s[l] = s[l] + s[l + stride] for l < stride, stride = 32, 16, ..., 1; the sum is valid in lane 0.  The lanes at and above a
// stride keep what they had: nothing of theirs is read again.  numpy repeats it (policy_ref.py: population_fitness_ref,
// obs_stats_accumulate_ref).
__device__ __forceinline__ double fitness_tree(double s, int lane) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(s, off, 64);
        if (lane < off) s = s + o;
    }
    return s;
}

// the integer twin, for counts: exact, so its order is nobody's business
__device__ __forceinline__ long long count_tree(long long s, int lane) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const long long o = __shfl_down(s, off, 64);
        if (lane < off) s += o;
    }
    return s;
}

// The minimum (MAX: the maximum) rule of the episode outcomes (include/bskgpu.h): the candidate x replaces the incumbent m when it
// is smaller (greater) or the incumbent is a NaN - so a NaN stands for "nothing yet", and all-NaN gives a NaN
template <bool MAX>
__device__ __forceinline__ double extreme_pick(double m, double x) {
    return ((MAX ? x > m : x < m) || m != m) ? x : m;
}

// ... joined in fitness_tree's order: lane l < stride holds the incumbent, lane l + stride the candidate
template <bool MAX>
__device__ __forceinline__ double extreme_tree(double m, int lane) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(m, off, 64);
        if (lane < off) m = extreme_pick<MAX>(m, o);
    }
    return m;
}

}  // namespace bsk
