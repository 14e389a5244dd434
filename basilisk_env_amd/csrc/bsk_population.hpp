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

// bsk_population_set_outcomes: how every env's first episode ended and which actions it took, kept beside FitnessAcc between the
// env steps' launches (no [n_steps][n] reason or action history).  Struct of arrays, as above: a wave's access is contiguous.
struct OutcomeAcc {
    int* act_n;                    // [3][n]: the steps taken under action 0, 1, 2 while alive
    unsigned char* end_reason;     // [n]: the reason byte of the step that ended the first episode; 0: still alive
};

// Row t of a rollout's histories (what launch_hist_row leaves; each may be NULL) and one step of the value rule, in ONE launch.
// first: this is env step 0 of the rollout - the accumulators are not read but taken as v = 0, g = 1, len = 0, alive.
hipError_t launch_fitness_row(const double* obs, const double* reward, const unsigned char* reason, int64_t stride, int n, double* obs_row,
                              double* reward_row, unsigned char* reason_row, const FitnessAcc& acc, double gamma, bool first,
                              hipStream_t s);
// The same launch with the outcome rule behind the value rule (ONE device function holds the value rule for both kernels):
// action is the row the policy launch of this step wrote, int32[n], every entry in 0..2.
hipError_t launch_outcome_row(const double* obs, const double* reward, const unsigned char* reason, const int* action, int64_t stride, int n,
                              double* obs_row, double* reward_row, unsigned char* reason_row, const FitnessAcc& acc, const OutcomeAcc& out,
                              double gamma, bool first, hipStream_t s);
// One wave per member: the fixed-order sums of include/bskgpu.h over the member's envs_per_member accumulators ->
// fitness[m], mean_len[m]; the accumulators themselves are copied to env_value / env_len on the way.  Every output may be NULL.
hipError_t launch_fitness_join(const FitnessAcc& acc, int n_members, int envs_per_member, double* env_value, int* env_len,
                               double* fitness, double* mean_len, hipStream_t s);

// One wave per member, behind the last step: rows f64[n_members][BSK_OUTCOME_COLS] of include/bskgpu.h out of both accumulator sets
hipError_t launch_outcome_join(const FitnessAcc& acc, const OutcomeAcc& out, int n_members, int envs_per_member, double* rows,
                               hipStream_t s);

}  // namespace bsk
