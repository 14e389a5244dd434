// bsk_es.hpp — the evolution strategy on the device (bsk_es.hip; internal): what bsk_es_ask / bsk_es_tell launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bsk_policy.hpp"

namespace bsk {

struct EsArgs {
    const unsigned long long* state;   // {seed, generation}: device words, like the policy's {seed, draw}
    double* theta;                     // [n_params], the C-ABI parameter layout
    double sigma;
    int frozen;                        // the first `frozen` parameters are neither perturbed nor moved
    int pairs;                         // n_members / 2
};

// bsk_es_set_optimizer(BSK_ES_ADAM): the moments, the running powers of beta1 / beta2 and the constants formed once on the host
struct EsAdam {
    double* m;                         // [n_params], first moment; frozen parameters keep 0
    double* v;                         // [n_params], second moment
    const double* beta_pow;            // {beta1^t, beta2^t} after t tells: device words, moved by launch_es_advance_adam
    double beta1, beta2, a1, a2;       // a1 = 1 - beta1, a2 = 1 - beta2
    double eps, weight_decay;
    double cg, lr;                     // cg = 1 / ((double)P * sigma)
};

// Adam's update of parameter j under the gradient `grad` (include/bskgpu.h, bsk_es_set_optimizer): the two moments are moved and
// stored, and the bias-corrected step is returned - (lr * (m / (1 - p1))) / (sqrt(v / (1 - p2)) + eps), every operation rounded on
// its own.  ONE text behind the evolution strategy, which ascends (theta + step), and the policy fit of bsk_fit.hip, which descends
// (theta - step); beta_pow is read here and moved on by a one-thread launch behind the update.
__device__ __forceinline__ double adam_step(const EsAdam& ad, int j, double grad) {
#pragma clang fp contract(off)
    const double p1 = ad.beta_pow[0] * ad.beta1, p2 = ad.beta_pow[1] * ad.beta2;
    const double m = ad.beta1 * ad.m[j] + ad.a1 * grad;
    const double v = ad.beta2 * ad.v[j] + (ad.a2 * grad) * grad;
    ad.m[j] = m;
    ad.v[j] = v;
    return (ad.lr * (m / (1.0 - p1))) / (sqrt(v / (1.0 - p2)) + ad.eps);
}

// bsk_es_set_sigma_adaptation(BSK_ES_SIGMA_PGPE): the step size of every parameter and the constants of its update
struct EsSigma {
    double* sigma_vec;                 // [n_params]; entries below `frozen` are carried, never read by a kernel and never moved
    double pd;                         // (double)P
    double cs;                         // lr_sigma / pd, formed once on the host
    double max_change, sigma_min, sigma_max;
};

// bsk_es_set_log: the ring of per-generation rows and the champion, all device memory (one allocation of the optimiser's)
struct EsLog {
    unsigned long long* gen;           // [capacity], the generation each row belongs to (all ones: never written)
    double* row;                       // [capacity][8]
    double* best_fitness;              // the champion: a NaN while there is none
    unsigned long long* best_generation;
    int* best_member;
    int* cand;                         // {take, b}: es_log_kernel's words for es_best_kernel
    float* best_params;                // [n_params], the C-ABI parameter layout
    const double* mean_len;            // [n_members] or nullptr: the caller's, bound by bsk_es_set_log
    int capacity;
};

// bsk_es_set_validation: the ring of the centre's rows and the validated champion, all device memory (one allocation of the
// optimiser's; the V epoch words in front of it are the caller's to read, no kernel of the optimiser does)
struct EsVal {
    unsigned long long* gen;           // [capacity], the generation each row belongs to (all ones: never written)
    double* row;                       // [capacity][4]: f_c, L_c, take, V
    double* best_fitness;              // the validated champion: a NaN while there is none
    unsigned long long* best_generation;
    int* cand;                         // {take}: es_validate_kernel's word for es_val_best_kernel
    float* best_params;                // [n_params], the C-ABI parameter layout
    const double* mean_len;            // [n_members + n_val] or nullptr: the caller's, bound by bsk_es_set_validation
    int capacity;
    int n_val;
};

// bsk_es_set_outcome_log: the ring of what the members did (one allocation of the optimiser's) and the member rows it is formed from
struct EsOutcome {
    unsigned long long* gen;           // [capacity], the generation each row belongs to (all ones: never written)
    double* row;                       // [capacity][3 * BSK_OUTCOME_COLS]: the P ranked members' totals | the first-ranked member's row | the V validation members' totals
    const double* rows;                // [n_members + n_val][BSK_OUTCOME_COLS]: the caller's, bound by bsk_es_set_outcome_log
    int capacity;
    int n_val;
};

// The members of this generation into d_params ([2 * pairs][lay.n_device], a population's device layout): one launch, every
// float written exactly once.
hipError_t launch_es_ask(const PolicyLayout& lay, const EsArgs& es, float* d_params, hipStream_t s);
// fitness f64[n_members] -> w f64[n_members / 2]: the difference of the centred-rank utilities of each pair's two members
hipError_t launch_es_rank(const double* fitness, int n_members, double* w, hipStream_t s);
// theta_j = theta_j + c * sum_i w_i * z(g, i, j) for every j >= frozen, the sum in the fixed order of include/bskgpu.h
hipError_t launch_es_tell(const EsArgs& es, int n_params, const double* w, double c, hipStream_t s);
// the same sum through Adam: g = cg * s[0] - weight_decay * theta_j, the moments, the bias-corrected step (include/bskgpu.h)
hipError_t launch_es_tell_adam(const EsArgs& es, int n_params, const double* w, const EsAdam& ad, hipStream_t s);
// BSK_ES_SIGMA_PGPE, the same four with sigma_vec[j] in the place of sigma (include/bskgpu.h): ask; the ranking that also writes
// q f64[n_members / 2], the SUM of each pair's utilities; the two updates, which leave sigma_vec moved as well (es.sigma and
// ad.cg are not read)
hipError_t launch_es_ask_sigma(const PolicyLayout& lay, const EsArgs& es, const double* sigma_vec, float* d_params, hipStream_t s);
hipError_t launch_es_rank_q(const double* fitness, int n_members, double* w, double* q, hipStream_t s);
hipError_t launch_es_tell_sigma(const EsArgs& es, int n_params, const double* w, const double* q, double lr, const EsSigma& sv, hipStream_t s);
hipError_t launch_es_tell_adam_sigma(const EsArgs& es, int n_params, const double* w, const double* q, const EsAdam& ad, const EsSigma& sv,
                                     hipStream_t s);
// The two launches of the training log, in front of the update (theta, sigma_vec and the generation word as ask read them):
// the row of this generation and the champion rule, then the champion's floats.  sigma_vec: nullptr under BSK_ES_SIGMA_FIXED.
hipError_t launch_es_log(const EsArgs& es, const double* sigma_vec, int n_params, const double* fitness, const EsLog& lg, hipStream_t s);
// Validation: (float)theta into the n_val device blocks from d_block on (the block of member n_members), one launch behind ask's ...
hipError_t launch_es_center(const PolicyLayout& lay, const double* theta, float* d_block, int n_val, hipStream_t s);
// ... and the two launches in front of the update, behind the log's: fitness f64[n_members + n_val], the centre's row and the
// champion rule on one thread, then the validated champion's floats
hipError_t launch_es_validate(const EsArgs& es, int n_params, const double* fitness, const EsVal& vl, hipStream_t s);
// The outcome ring: ONE wave in front of the update, beside the log's launches - it reads the generation word, fitness f64[n_members]
// and the member rows, and writes its own ring only
hipError_t launch_es_outcome(const EsArgs& es, const double* fitness, const EsOutcome& oc, hipStream_t s);
// generation += 1 and beta_pow *= {beta1, beta2}, one thread, behind launch_es_tell_adam on the same stream
hipError_t launch_es_advance_adam(unsigned long long* state, double* beta_pow, double beta1, double beta2, hipStream_t s);
// generation += 1, one thread, behind a tell on the same stream (a replayed graph moves on to the next generation)
hipError_t launch_es_advance(unsigned long long* state, hipStream_t s);

}  // namespace bsk
