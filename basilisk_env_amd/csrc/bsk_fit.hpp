// bsk_fit.hpp — a supervised fit of the MLP policy on the device (bsk_fit.hip; internal): what bsk_fit_accumulate / bsk_fit_step
// launch, the policy-gradient form of the block kernel (bsk_fit_accumulate_pg) and the advantage estimator in front of it (bsk_gae).
// The arithmetic is the definition in include/bskgpu.h (bsk_fit_*, bsk_gae).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bsk_es.hpp"
#include "bsk_policy.hpp"

namespace bsk {

constexpr int FIT_BLOCK_SAMPLES = POLICY_LANES;     // samples of one gradient block: one workgroup, one lane each

// One network as the fit kernel walks it: the layers of the pack map (where Wt / b lie in the device block, where W / b start in
// the C-ABI block, which is the order of the gradient) and the hidden activation.
struct FitNet {
    int n_layers;                  // 0: the network is not fitted by this launch (none, or no targets)
    int act;
    PolicyPackMap::Layer layer[POLICY_MAX_LAYERS];
};

struct FitArgs {
    const float* params;           // the policy's device layout
    FitNet a, v;
    const double* obs;             // [5][obs_stride]
    int64_t obs_stride;
    int n;
    const int32_t* label;          // [n]
    const double* target;          // [n] or NULL
    const uint8_t* alive;          // [n] or NULL
    float value_coef;
    float* dlogits;                // [3][out_stride] or NULL
    int64_t out_stride;
    float* G;                      // [n_blocks][n_params]: the block gradients, C-ABI parameter order
    double* diag;                  // [n_blocks][4]: the block's terms of the diagnostics row
    int n_params;
    int rows;                      // fit_lds_rows
    // the policy-gradient launch alone (launch_fit_blocks_pg; `label` is then the action taken, `diag` [n_blocks][8])
    const float* adv;              // [n]
    const float* logp_old;         // [n] or NULL: no ratio, no clipping
    const float* lp;               // [3][n]: the log-probabilities of the three actions, policy_logp_kernel's
    float clip_hi, clip_lo, ent_coef;      // 1.0f + (float)clip, 1.0f - (float)clip, (float)ent_coef
};

// What bsk_fit_accumulate_ppo adds to a policy-gradient launch (launch_fit_blocks_ppo: a third instantiation of the block kernel, which
// takes this beside FitArgs; `diag` is then [n_blocks][10])
struct FitVclip {
    const float* value_old;        // [n] or NULL: the plain squared error
    float clip_vf;                 // (float)clip_vf
    float* dvalue;                 // [n] or NULL: the value network's output delta of every sample
};

// The fit's schedule words (bsk_pgsched.hpp) as a scheduled launch takes them: a further element of the kernels' variadic packs, a
// type of its own beside the clip's row (const double*).  Every lane reads the same words of it: uniform loads
struct FitSched {
    const double* __restrict__ row;        // [PG_SCHED_WORDS]: lr, clip, clip_vf, ent_coef now, ...
};

// LDS rows of 64 floats the block kernel needs for this layout: the input, every hidden layer of the larger network, the output deltas
int fit_lds_rows(const PolicyLayout& lay);
FitNet fit_net(const PolicyPackMap& map, int first, const PolicyNet& net);

// One workgroup per 64 samples: forward, output deltas, backward, the block's gradient and diagnostics terms
hipError_t launch_fit_blocks(const FitArgs& args, hipStream_t s);
// The same with the policy-gradient output deltas in the cross-entropy's place, and eight diagnostics terms per block
hipError_t launch_fit_blocks_pg(const FitArgs& args, hipStream_t s);
// The same with the clipped value loss (value_old) and / or the value deltas written out (dvalue), and ten diagnostics terms per block
hipError_t launch_fit_blocks_ppo(const FitArgs& args, const FitVclip& vc, hipStream_t s);
// The two above as scheduled launches: clip_hi, clip_lo and ent_coef of `args` and clip_vf of `vc` are not read - the words at
// `sched` are, rounded as the host rounds the arguments
hipError_t launch_fit_blocks_pg_sched(const FitArgs& args, const double* sched, hipStream_t s);
hipError_t launch_fit_blocks_ppo_sched(const FitArgs& args, const FitVclip& vc, const double* sched, hipStream_t s);
// A[p] += (double)G[b][p] for b ascending, p in 10 .. n_fold - 1; the diagnostics row out of the block terms; count += row[3]
hipError_t launch_fit_fold(const float* G, const double* diag, int n_blocks, int n_params, int n_fold, double* A, double* row,
                           unsigned long long* count, hipStream_t s);
// The same over block terms of eight: the first four into `row` as above, the last four into `pg_row`
hipError_t launch_fit_fold_pg(const float* G, const double* diag, int n_blocks, int n_params, int n_fold, double* A, double* row,
                              double* pg_row, unsigned long long* count, hipStream_t s);
// The same over block terms of ten: the last two into `vclip_row`, or nowhere while it is NULL
hipError_t launch_fit_fold_ppo(const float* G, const double* diag, int n_blocks, int n_params, int n_fold, double* A, double* row,
                               double* pg_row, double* vclip_row, unsigned long long* count, hipStream_t s);
// Generalised advantage estimation over rollout histories [n_steps][stride]: one thread per env, t descending
hipError_t launch_gae(const double* reward, const uint8_t* reason, const float* value, const float* last_value, int n_steps, int n_envs,
                      int64_t stride, double gamma, double gl, float* adv, double* ret, hipStream_t s);
// bsk_adv_normalize over adv f32[rows][stride], columns below n: the partial sums of every wave of 64 columns, their join and the
// four words {mean, sd, inv, N}, then out = (float)((x - mean) * inv).  work: 4 + 3 * ceil(n / 64) words of 8 bytes
hipError_t launch_adv_normalize(const float* adv, const uint8_t* alive, int rows, int n, int64_t stride, double eps, float* out, double* work,
                                hipStream_t s);
// Adam on g = A / count + weight_decay * theta for p in 10 .. n_upd - 1 (descent; nothing while count == 0), A zeroed; then one
// thread: beta_pow and the step counter move on, count = 0.  max_norm > 0: one workgroup in front leaves {norm, scale} of the mean
// gradient in gnorm_row, and g = (A / count) * scale + weight_decay * theta; max_norm == 0: the launches and arguments without it.
// sched (the fit's schedule words, or NULL: the launches and arguments without it): ad.lr is not read, word 0 is
hipError_t launch_fit_step(double* theta, double* A, unsigned long long* count, unsigned long long* steps, int n_upd, const EsAdam& ad,
                           double max_norm, double* gnorm_row, hipStream_t s, const double* sched = nullptr);
// alive[j] = first || (alive[j] && reason[j] == 0), as bytes 1 / 0
hipError_t launch_fit_alive(const uint8_t* reason, int n, int first, uint8_t* alive, hipStream_t s);

}  // namespace bsk
