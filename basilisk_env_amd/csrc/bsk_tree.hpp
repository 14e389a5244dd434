// bsk_tree.hpp — the 64-lane sum every fixed-order reduction of the library ends in (internal; device code only): one text for
// the fitness of a population rollout (bsk_population.hip) and the observation statistics (bsk_obsstats.hip), so that the order of
// the additions cannot diverge between them.  Both units are compiled with -ffp-contract=off.
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

}  // namespace bsk
