// bsk_population.hpp — device fitness of a population rollout (bsk_population.hip; internal): what bsk_population_rollout launches
// beside the population form of the policy kernel (bsk_policy.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bsk {

// The running value of every env of a population rollout, kept between the env steps' launches (no [n_steps][n] reward history):
//   v the discounted return so far, g the next step's discount, len the steps counted, alive 1 until the first episode has ended.
struct FitnessAcc {
    double* v;                     // [n]
    double* g;                     // [n]
    int* len;                      // [n]
    unsigned char* alive;          // [n]
};

// Row t of a rollout's histories (what launch_hist_row leaves; each may be NULL) and one step of the value rule, in ONE launch.
// first: this is env step 0 of the rollout - the accumulators are not read but taken as v = 0, g = 1, len = 0, alive.
hipError_t launch_fitness_row(const double* obs, const double* reward, const unsigned char* reason, int64_t stride, int n, double* obs_row,
                              double* reward_row, unsigned char* reason_row, const FitnessAcc& acc, double gamma, bool first,
                              hipStream_t s);
// One wave per member: the fixed-order sums of include/bskgpu.h over the member's envs_per_member accumulators ->
// fitness[m], mean_len[m]; the accumulators themselves are copied to env_value / env_len on the way.  Every output may be NULL.
hipError_t launch_fitness_join(const FitnessAcc& acc, int n_members, int envs_per_member, double* env_value, int* env_len,
                               double* fitness, double* mean_len, hipStream_t s);

}  // namespace bsk
