// bsk_aux.hpp — host-side entry points of the small kernels around the step kernel (bsk_aux.hip; internal).
// Kept apart from bsk_launch.hpp so that a change here does not rebuild the step kernel's 36+ instantiations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct bsk_beam_slot;              // (include/bskgpu.h)

namespace bsk {

// what a reset leaves in the output buffers of the envs it restarts (init_outputs_kernel)
struct ResetOut {
    double* obs;                   // [5][ostride]
    int64_t ostride;
    double* obs_rm;                // [n][5] or NULL
    double* reward;                // [stride]
    unsigned char* reason;         // [stride]
    unsigned char* done;           // [stride] or NULL
    double* ep_return;             // [stride] or NULL
    double inv_wheel_limit, charge_scale;
    int n_rw;
};

hipError_t launch_sample_pool(double* pool, int n_pool, int n_rw, unsigned long long seed, double mu, hipStream_t s);
hipError_t launch_reset_from_pool(double* st, int64_t stride, int nf, const double* pool, int n_pool, const unsigned char* mask,
                                  int n, int2* cnt, int* episodes, unsigned env_base, const ResetOut& ro, hipStream_t s);
// bsk_reset_from_pool_shared: slot from (env_base + env) mod envs_per_member and the low word of *epoch (NULL: 0), include/bskgpu.h
hipError_t launch_reset_from_pool_shared(double* st, int64_t stride, int nf, const double* pool, int n_pool, const unsigned char* mask,
                                         int n, int2* cnt, int* episodes, unsigned env_base, unsigned envs_per_member,
                                         const unsigned long long* epoch, const ResetOut& ro, hipStream_t s);
// first observation [|sigma_BN|, |omega|, |Omega|/limit, charge/3600/power_max, 1], zero reward / reason / done / episode
// return of freshly reset envs: all n (idx == NULL) or the m listed ones
hipError_t launch_init_outputs(const double* st, int64_t stride, const int* idx, int m, const ResetOut& ro, hipStream_t s);
// "no step since the last reset entry point" as the device sees it (bsk_aux.hip: stats_sealed): env 0's counter word and episode
// number as seal_kernel recorded them behind the reset, compared by the join kernel before it stores
struct StatsSeal {
    const unsigned long long* cnt0;     // the handle's counters (env 0's {steps | phase << 20, ticks} word first)
    const int* episodes;                // [n] or NULL (no IC pool staged)
    const unsigned long long* word;     // [3] {cnt0, episodes[0], 1} at the seal; NULL: never sealed
};
hipError_t launch_seal(const StatsSeal& seal, hipStream_t s);
// batch scalars of the last step (stats_kernel + stats_join_kernel): scratch wave_sum f64[n_waves], done_part u32[stats_done_parts()];
// have_wave_sums: the step kernel filled wave_sum[] (TailArgs::wave_sum) - the join kernel alone
hipError_t launch_stats(const double* reward, int n, const unsigned long long* done_mask, int n_waves, double* wsum,
                        unsigned* done_part, double* out_sum, long long* out_done, double* out2, bool have_wave_sums, const StatsSeal& seal,
                        hipStream_t s);
hipError_t launch_scatter_reset(double* st, int64_t stride, int nf, const double* ic, const int* idx, int m, int2* cnt,
                                hipStream_t s);

// row t of a rollout's history from the handle's output buffers (bsk_step_n at the levels whose env steps stay separate launches)
hipError_t launch_hist_row(const double* obs, const double* reward, const unsigned char* reason, int64_t stride, int n, double* obs_row,
                           double* reward_row, unsigned char* reason_row, hipStream_t s);

// bsk_fork.hip: one handle's per-env buffers as the fork kernel reads or writes them (any optional pointer may be NULL: that handle
// lacks the buffer).  `st` rows are `stride` apart, every other [stride] array is `ostride` long.
struct ForkSide {
    double* st;                    // [nf][stride]
    int64_t stride;
    int2* cnt;                     // [ostride] the whole {steps | phase << 20, ticks} word
    double* obs;                   // [5][ostride]
    int64_t ostride;
    double* reward;                // [ostride]
    unsigned char* reason;         // [ostride]
    unsigned long long* done_mask; // [ostride / 64]
    double* obs_rm;                // [n][5] or NULL
    double* ep_return;             // [ostride] or NULL (ep_return, term_return, term_len, done: BSK_FLAG_EPISODE_STATS)
    double* term_return;
    int* term_len;
    unsigned char* done;
    double* term_obs;              // [5][ostride] or NULL (no IC pool staged)
    int* episodes;                 // [ostride] or NULL
    int n;
};
// env j of dst <- env map[j] of src (map[j] outside [0, src.n): j untouched).  identity: env j of src instead of map[j], for the
// second half of an in-handle fork (src = the gather scratch).  err: raised with BSK_DEVERR_FORK_MAP on an out-of-range entry
// other than -1 (NULL: not raised).  seal_word: the destination's StatsSeal::word, whose seal the fork lifts (NULL: none).
hipError_t launch_fork(const ForkSide& src, const ForkSide& dst, int nf, const int* map, bool identity, int* err,
                       unsigned long long* seal_word, hipStream_t s);
// one action per group of `group` consecutive branches from their rollout histories (bsk_select_branches); with leaf (f32[n_branch])
// the branches no step ended also take g * leaf[b] (bsk_select_branches_boot), with NULL the kernel without that term
hipError_t launch_select(const double* reward_hist, const unsigned char* reason_hist, const int* first_action, int n_steps, int n_branch,
                         int group, double gamma, const float* leaf, double* values, double* best_value, int* best_action, hipStream_t s);
// one level of a beam search: the `width` best of every root's 3 * width candidates (bsk_beam_select); with leaf
// (f32[3 * width * n_roots]) ranked by value + boot_weight * leaf[c] of the live candidates, the keys of the kept ones into key
// (f64[n_roots * width] or NULL) (bsk_beam_select_boot), with NULL the kernel without that term
hipError_t launch_beam(const double* reward, const unsigned char* reason, int n_roots, int width, int level, double weight,
                       double boot_weight, const float* leaf, const bsk_beam_slot* in, bsk_beam_slot* out, int* map, double* key,
                       double* best_value, int* best_action, hipStream_t s);

// first-level workgroups of stats_kernel at most = entries of the `done_part` scratch
int stats_done_parts();

}  // namespace bsk
