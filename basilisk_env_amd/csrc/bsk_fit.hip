// bsk_fit.hip — a supervised fit of the MLP policy to labelled observations, on the device (bsk_fit_*; definition in
// include/bskgpu.h): cross-entropy on the action, an optional squared error on the value, Adam.
//   fit_block_kernel    one workgroup per block of 64 samples: the policy's forward pass with every layer kept, the output deltas,
//                       the backward sweep and the block's gradient G_b in the C-ABI parameter order, plus its diagnostics terms
//                       <PG = true> (bsk_fit_accumulate_pg): the output deltas of the clipped policy-gradient loss with its
//                       entropy bonus in the cross-entropy's place, and four more diagnostics terms; <false> is the supervised kernel
//                       <true, FitVclip> (bsk_fit_accumulate_ppo with d_value_old or d_dvalue): the same with PPO2's clipped value
//                       loss in the squared error's place, the value deltas written out, and two diagnostics terms more
//                       <true, [FitVclip,] FitSched> (a schedule attached, bsk_fit_set_schedule): clip, ent_coef and clip_vf from the
//                       fit's schedule words (bsk_pgsched.hpp) in the place of the arguments - uniform loads, the host's roundings
//   fit_fold_kernel     one thread per parameter: A += (double)G_b, b ascending; four threads more for the diagnostics row
//                       (<8>: eight, the policy-gradient row behind the first; <10, double*>: ten, the value-clip row behind that)
//   gae_kernel          bsk_gae: one thread per env walks its column of the rollout histories from the last step to the first
//   adv_partial_kernel, adv_join_kernel, adv_apply_kernel    bsk_adv_normalize: the mean and standard deviation of an advantage
//                       block in the fixed order of the observation statistics (bsk_tree.hpp), and (x - mean) / (sd + eps)
//   fit_gnorm_kernel    bsk_fit_set_max_grad_norm: one workgroup, the global norm of the mean gradient and the clip's scale
//   fit_adam_kernel     one thread per parameter: the mean gradient through Adam (adam_step, bsk_es.hpp: the text of the
//                       evolution strategy's update), a descent; <true>: the gradient times the clip's scale first
//                       <..., FitSched>: lr from the schedule words, in a copy of the EsAdam that goes through the same adam_step
//   fit_advance_kernel  one thread: beta_pow and the step counter move on, the count back to zero
//   fit_alive_kernel    bsk_fit_alive_mask: which envs of a collection loop are still in their first episode
// The forward pass IS policy_kernel's: policy_hidden / policy_output of bsk_policy.hpp.  Every fused multiply-add is an explicit
// fmaf and every chain has one owner that walks it in the definition's order, so neither the launch shape nor the hardware's
// scheduling enters a bit: no atomics, and no cross-lane reduction but the fixed tree of bsk_tree.hpp under the two reductions of
// the policy-gradient loop (adv_*, fit_gnorm_kernel).  Compiled with -ffp-contract=off (Makefile) for the f64 parts.
#include "bsk_fit.hpp"

#include <tuple>
#include <type_traits>

#include "../../include/bskgpu.h"
#include "bsk_obsstats.hpp"
#include "bsk_pgsched.hpp"
#include "bsk_tree.hpp"

// Measurement builds only (make fit-stamps -> variants/fit_stamps.so; tools/fit_measure.py stamps): thread 0 of every workgroup
// counts the clock ticks of the weight-gradient walks, a barrier behind each, and of the whole kernel, and the block's diagnostics
// terms [0] and [1] carry the two counts in place of the losses.  The product never compiles this in.
#ifndef BSK_FIT_STAMPS
#define BSK_FIT_STAMPS 0
#endif

namespace bsk {

// LDS: rows of 64 floats, [unit][lane] as in policy_kernel.  Row 0 - 7: the network input x (five used); then every hidden layer of
// the network in turn; then POLICY_OB rows of output deltas.  The backward sweep needs no rows of its own: the deltas of a hidden
// layer replace its activations IN PLACE once the layer above has taken its weight gradient from them.
constexpr int FIT_X_ROWS = 8;
constexpr int FIT_FOLD_BATCH = 32;     // block gradients the fold has in flight per thread
constexpr int FIT_DIAG_ROWS = 5;       // behind the rows: two doubles and an int per sample, the terms of the block's diagnostics
constexpr int FIT_PG_DIAG_ROWS = 8;    // behind those, policy-gradient launches only: four doubles more per sample
constexpr int FIT_VC_DIAG_ROWS = 4;    // behind those, launches with a FitVclip only: two doubles more per sample
constexpr int FIT_GNORM_BLOCK = 1024;  // fit_gnorm_kernel's one workgroup: sixteen waves
constexpr int ADV_BATCH = 8;           // rows of an advantage block the partial sums have in flight per lane
constexpr int ADV_APPLY_ROWS = 1024;   // rows of the apply launch's grid; a block strides over the rest

__device__ __forceinline__ int fit_row(const FitNet& net, int l) {      // the first row of layer l's INPUT; l = n_layers: the output deltas
    int r = l == 0 ? 0 : FIT_X_ROWS;
    for (int i = 1; i < l; ++i) r += net.layer[i - 1].N;
    return r;
}

// d_h[k] of the layer below, k split between the waves four at a time, for this lane's sample: the j-ascending chain
// acc = fmaf(W[j][k], d_z[j], acc) from +0.0f; then through the activation's derivative at h[k], in place.
__device__ __forceinline__ void fit_input_delta(const float* __restrict__ wt, int N, int fan_out, int K, int act, const float* dz, float* h,
                                                int lane, int wave) {
    constexpr int KB = 4;              // (K is a hidden width here: a multiple of 16)
    for (int k0 = wave * KB; k0 < K; k0 += POLICY_WAVES * KB) {
        float acc[KB];
#pragma unroll
        for (int kk = 0; kk < KB; ++kk) acc[kk] = 0.0f;
#pragma unroll 4
        for (int j = 0; j < fan_out; ++j) {
            const float d = dz[j * POLICY_LANES + lane];
#pragma unroll
            for (int kk = 0; kk < KB; ++kk) acc[kk] = __builtin_fmaf(wt[(k0 + kk) * N + j], d, acc[kk]);
        }
#pragma unroll
        for (int kk = 0; kk < KB; ++kk) {
            float* at = h + (k0 + kk) * POLICY_LANES + lane;
            const float hk = *at;
            *at = act == BSK_POLICY_TANH ? acc[kk] * __builtin_fmaf(-hk, hk, 1.0f) : (hk > 0.0f ? acc[kk] : 0.0f);
        }
    }
}

// The weight gradients of one layer: GW[j][k] = the sample-ascending chain acc = fmaf(d_z[j][s], h[k][s], acc) from +0.0f.  The
// ownership is turned round from the sweeps: a lane owns one row of the wider side - its 64 samples in registers, read from the
// LDS once - and walks the rows of the other side, which its whole half-wave reads at one address (a broadcast).  The waves split
// those rows; a side of 32 rows or fewer leaves the upper half-wave to a second one.  DZ_LANES: the lanes own d_z rows (j), else h rows (k).
template <bool DZ_LANES>
__device__ __forceinline__ void fit_weight_grad(const float* dz, int fan_out, const float* h, int K, float* __restrict__ gw, int lane, int wave) {
    const float* A = DZ_LANES ? dz : h;
    const float* B = DZ_LANES ? h : dz;
    const int n_a = DZ_LANES ? fan_out : K, n_b = DZ_LANES ? K : fan_out;
    const int span = n_a <= 32 ? 32 : 64, subs = 64 / span;
    const int sub = lane / span, al = lane % span;
    for (int a0 = 0; a0 < n_a; a0 += span) {
        const int a = a0 + al;
        const bool valid = a < n_a;
        const float4* row = (const float4*)(A + (valid ? a : 0) * POLICY_LANES);
        float4 r[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) r[i] = row[i];
        for (int b = wave * subs + sub; b < n_b; b += POLICY_WAVES * subs) {
            const float4* col = (const float4*)(B + b * POLICY_LANES);
            float acc = 0.0f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float4 q = col[i];
                if (DZ_LANES) {
                    acc = __builtin_fmaf(r[i].x, q.x, acc); acc = __builtin_fmaf(r[i].y, q.y, acc);
                    acc = __builtin_fmaf(r[i].z, q.z, acc); acc = __builtin_fmaf(r[i].w, q.w, acc);
                } else {
                    acc = __builtin_fmaf(q.x, r[i].x, acc); acc = __builtin_fmaf(q.y, r[i].y, acc);
                    acc = __builtin_fmaf(q.z, r[i].z, acc); acc = __builtin_fmaf(q.w, r[i].w, acc);
                }
            }
            if (valid) gw[DZ_LANES ? a * K + b : b * K + a] = acc;
        }
    }
}

// Gb[j]: the sample-ascending chain of plain additions of d_z[j][s] from +0.0f, one thread per unit
__device__ __forceinline__ void fit_bias_grad(const float* dz, int fan_out, float* __restrict__ gb) {
    for (int j = (int)threadIdx.x; j < fan_out; j += POLICY_BLOCK) {
        const float4* row = (const float4*)(dz + j * POLICY_LANES);
        float acc = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float4 q = row[i];
            acc = acc + q.x; acc = acc + q.y; acc = acc + q.z; acc = acc + q.w;
        }
        gb[j] = acc;
    }
}

// The forward pass of one network from the x rows, every layer kept.  -> out (wave 0): the output layer, as policy_net leaves it
__device__ __forceinline__ void fit_forward(const float* __restrict__ params, const FitNet& net, float* lds, int lane, int wave, float* out) {
    const int last = net.n_layers - 1;
    int row = 0;
    for (int l = 0; l < last; ++l) {
        const PolicyPackMap::Layer& y = net.layer[l];
        const int next = l == 0 ? FIT_X_ROWS : row + net.layer[l - 1].N;
        policy_hidden(params + y.w, params + y.b, y.K, y.N, net.act, lds + row * POLICY_LANES, lds + next * POLICY_LANES, lane, wave);
        __syncthreads();                   // (layer l + 1 reads what every wave wrote)
        row = next;
    }
    if (wave == 0) policy_output(params + net.layer[last].w, params + net.layer[last].b, net.layer[last].K, lds + row * POLICY_LANES, lane, out);
}

// The backward sweep from the output deltas (written, and a barrier passed): per layer from the last the weight and bias gradients
// into the block's row g (C-ABI order), then - a barrier on either side - the deltas of the layer below in place of its activations.
__device__ __forceinline__ void fit_backward(const float* __restrict__ params, const FitNet& net, float* lds, float* __restrict__ g, int lane,
                                             int wave, long long* walk_ticks) {
    const float* dz = lds + fit_row(net, net.n_layers) * POLICY_LANES;
    for (int l = net.n_layers - 1; l >= 0; --l) {
        const PolicyPackMap::Layer& y = net.layer[l];
        float* h = lds + fit_row(net, l) * POLICY_LANES;
#if BSK_FIT_STAMPS
        const long long t0 = clock64();
#endif
        if (y.fan_out >= y.K) fit_weight_grad<true>(dz, y.fan_out, h, y.K, g + y.src, lane, wave);
        else                  fit_weight_grad<false>(dz, y.fan_out, h, y.K, g + y.src, lane, wave);
#if BSK_FIT_STAMPS
        __syncthreads();
        *walk_ticks += clock64() - t0;
#endif
        fit_bias_grad(dz, y.fan_out, g + y.src + y.fan_out * y.K);
        if (l == 0) break;
        __syncthreads();                   // (the gradients have read h; it turns into the deltas below)
        fit_input_delta(params + y.w, y.N, y.fan_out, y.K, net.act, dz, h, lane, wave);
        __syncthreads();
        dz = h;
    }
}

// Vc: nothing, one FitVclip behind a policy-gradient launch, and / or - last - one FitSched: the fit's schedule words
// (bsk_pgsched.hpp), from which a scheduled launch takes clip, ent_coef and clip_vf in the place of its arguments, with the
// roundings the host applies to those (bsk_fit_accumulate_ppo).  Every lane reads the same words: uniform loads of a kernel
// argument that is const and __restrict__, never through the LDS.  The instantiations without a row keep the arguments they have
// always had; the clipped value loss is code of the instantiations with a FitVclip alone.
template <bool PG, typename... Vc>
__global__ __launch_bounds__(POLICY_BLOCK) void fit_block_kernel(const FitArgs p, const Vc... vclip) {
    constexpr bool VC = (std::is_same_v<Vc, FitVclip> || ... || false);
    constexpr bool SCHED = (std::is_same_v<Vc, FitSched> || ... || false);
    static_assert(PG || !(VC || SCHED), "the value clip and the schedule ride on the policy-gradient launch");
    static_assert(sizeof...(Vc) == (VC ? 1 : 0) + (SCHED ? 1 : 0), "a FitVclip first, a FitSched last, nothing else");
    float sched_hi = 0.0f, sched_lo = 0.0f, sched_ec = 0.0f, sched_cv = 0.0f;       // (SCHED alone; the others read `p` where they did)
    if constexpr (SCHED) {                 // (in front of every store of the kernel: nothing can have written the words)
        const double* __restrict__ sched = std::get<sizeof...(Vc) - 1>(std::forward_as_tuple(vclip...)).row;
        sched_hi = 1.0f + (float)sched[PG_SCHED_CLIP];
        sched_lo = 1.0f - (float)sched[PG_SCHED_CLIP];
        sched_ec = (float)sched[PG_SCHED_ENT_COEF];
        sched_cv = (float)sched[PG_SCHED_CLIP_VF];
    }
    // (everything in the dynamic region and every carve a multiple of 16 bytes: a static array in front would shift its base)
    extern __shared__ __attribute__((aligned(16))) float fit_lds[];
    double* s_nll = (double*)(fit_lds + p.rows * POLICY_LANES);
    double* s_vl = s_nll + POLICY_LANES;
    int* s_flag = (int*)(s_vl + POLICY_LANES);     // bit 0: the sample contributes; bit 1: the greedy action is its label
    double* s_pg = (double*)(s_flag + POLICY_LANES);        // (PG launches only) [4][lane]: -d, H, clipped, A * r
    double* s_vc = s_pg + 4 * POLICY_LANES;                 // (VC launches only) [2][lane]: value-clipped, the unclipped d d / 2
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t j = (int64_t)blockIdx.x * POLICY_LANES + lane;
    const bool live = j < p.n;
    float* g = p.G + (size_t)blockIdx.x * (size_t)p.n_params;
    long long walk_ticks = 0;              // (BSK_FIT_STAMPS builds only; otherwise never touched)
#if BSK_FIT_STAMPS
    const long long t_start = clock64();
#endif

    int label = -1;
    bool on = false;
    if (wave == 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const double o = live ? p.obs[(int64_t)i * p.obs_stride + j] : 0.0;       // (tail lanes read nothing)
            fit_lds[i * POLICY_LANES + lane] = __builtin_fmaf((float)o, p.params[i], p.params[5 + i]);
        }
        if (live) label = p.label[j];
        on = live && label >= 0 && label <= 2 && (!p.alive || p.alive[j] != 0);
    }
    __syncthreads();

    // the action network: cross-entropy against the label
    float out[POLICY_OB] = {0.0f, 0.0f, 0.0f, 0.0f};
    fit_forward(p.params, p.a, fit_lds, lane, wave, out);
    float* delta = fit_lds + fit_row(p.a, p.a.n_layers) * POLICY_LANES;
    if (wave == 0) {
        const float m = fmaxf(fmaxf(out[0], out[1]), out[2]);
        const float e0 = expf(out[0] - m), e1 = expf(out[1] - m), e2 = expf(out[2] - m);
        const float s = (e0 + e1) + e2;
        int a = 0;
        float best = out[0];
        if (policy_beats(out[1], best)) { best = out[1]; a = 1; }
        if (policy_beats(out[2], best)) { best = out[2]; a = 2; }
        float logp;
        float gl[3] = {0.0f, 0.0f, 0.0f};
        if constexpr (PG) {
            // the clipped surrogate's deltas (include/bskgpu.h, bsk_fit_accumulate_pg): `label` is the action taken.  p_i is the
            // supervised kernel's, from this unit's e_i and s; lp_i is READ - policy_logp_kernel's, from the launch in front, which
            // forms it in policy_kernel's own unit (bsk_policy.hpp, policy_softmax: this unit's expf and logf are not that one's)
            const float pr[3] = {e0 / s, e1 / s, e2 / s};
            float lp[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) lp[i] = live ? p.lp[(int64_t)i * p.n + j] : 0.0f;
            logp = label == 0 ? lp[0] : (label == 1 ? lp[1] : lp[2]);
            const float H = -((pr[0] * lp[0] + pr[1] * lp[1]) + pr[2] * lp[2]);
            const float A = on ? p.adv[j] : 0.0f;
            float d = 0.0f, r = 1.0f;
            bool clipped = false;
            if (p.logp_old) {                  // (workgroup-uniform)
                d = logp - (on ? p.logp_old[j] : 0.0f);
                r = expf(d);
                clipped = (A > 0.0f && r > (SCHED ? sched_hi : p.clip_hi)) || (A < 0.0f && r < (SCHED ? sched_lo : p.clip_lo));
            }
            const float ent_coef = SCHED ? sched_ec : p.ent_coef;
            const bool flat = clipped || A == 0.0f;          // c = +0.0f: the deltas are +0.0f, never the product's -0.0f
            const float c = A * r;
            if (on) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float gp = flat ? 0.0f : c * (pr[i] - (label == i ? 1.0f : 0.0f));
                    gl[i] = ent_coef == 0.0f ? gp : __builtin_fmaf(ent_coef, pr[i] * (lp[i] + H), gp);
                }
            }
            s_pg[lane] = on ? -(double)d : 0.0;
            s_pg[POLICY_LANES + lane] = on ? (double)H : 0.0;
            s_pg[2 * POLICY_LANES + lane] = on && clipped ? 1.0 : 0.0;
            s_pg[3 * POLICY_LANES + lane] = on ? (double)A * (double)r : 0.0;
        } else {
            logp = ((label == 0 ? out[0] : (label == 1 ? out[1] : out[2])) - m) - logf(s);
            if (on) {
                gl[0] = e0 / s - (label == 0 ? 1.0f : 0.0f);
                gl[1] = e1 / s - (label == 1 ? 1.0f : 0.0f);
                gl[2] = e2 / s - (label == 2 ? 1.0f : 0.0f);
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            delta[i * POLICY_LANES + lane] = gl[i];
            if (p.dlogits && live) p.dlogits[(int64_t)i * p.out_stride + j] = gl[i];
        }
        s_nll[lane] = on ? -(double)logp : 0.0;
        s_vl[lane] = 0.0;
        s_flag[lane] = (on ? 1 : 0) | (on && a == label ? 2 : 0);
    }
    __syncthreads();
    fit_backward(p.params, p.a, fit_lds, g, lane, wave, &walk_ticks);

    // the value network: squared error against the target
    if (p.v.n_layers > 0) {                // (workgroup-uniform)
        __syncthreads();                   // (the action network's last reads of the rows)
        float val[POLICY_OB] = {0.0f, 0.0f, 0.0f, 0.0f};
        fit_forward(p.params, p.v, fit_lds, lane, wave, val);
        delta = fit_lds + fit_row(p.v, p.v.n_layers) * POLICY_LANES;
        if (wave == 0) {
            if constexpr (VC) {
                const float R = on ? (float)p.target[j] : 0.0f;
                const float d = on ? val[0] - R : 0.0f;
                // PPO2's max((v - R)^2, (v_old + clamp(v - v_old, +-cv) - R)^2) (include/bskgpu.h, bsk_fit_accumulate_ppo): where
                // the clipped branch holds the max its gradient is zero; a tie is the unclipped branch's
                const FitVclip& x = std::get<0>(std::forward_as_tuple(vclip...));
                float dl = on ? p.value_coef * d : 0.0f;
                const double plain = (((double)d) * ((double)d)) * 0.5;
                double term = plain;
                bool vclipped = false;
                if (x.value_old && on) {           // (the pointer: workgroup-uniform)
                    const float cv = SCHED ? sched_cv : x.clip_vf;
                    const float vo = x.value_old[j];
                    const float dv = val[0] - vo;
                    if (!(-cv <= dv && dv <= cv)) {
                        const float vc = vo + (dv > 0.0f ? cv : -cv);
                        const float d2 = vc - R;
                        if (d2 * d2 > d * d) {
                            dl = 0.0f;
                            term = (((double)d2) * ((double)d2)) * 0.5;
                            vclipped = true;
                        }
                    }
                }
                delta[lane] = dl;
                s_vl[lane] = term;
                s_vc[lane] = vclipped ? 1.0 : 0.0;
                s_vc[POLICY_LANES + lane] = plain;
                if (x.dvalue && live) x.dvalue[j] = dl;
            } else {
                const float d = on ? val[0] - (float)p.target[j] : 0.0f;
                delta[lane] = on ? p.value_coef * d : 0.0f;
                s_vl[lane] = (((double)d) * ((double)d)) * 0.5;
            }
        }
        __syncthreads();
        fit_backward(p.params, p.v, fit_lds, g, lane, wave, &walk_ticks);
    }

    __syncthreads();
    if (threadIdx.x == 0) {                // the block's terms, sample-ascending from +0.0
        double nll = 0.0, vl = 0.0;
        int count = 0, correct = 0;
        for (int s = 0; s < POLICY_LANES; ++s) {
            nll = nll + s_nll[s];
            vl = vl + s_vl[s];
            count += s_flag[s] & 1;
            correct += (s_flag[s] >> 1) & 1;
        }
        double* row = p.diag + (VC ? 10 : (PG ? 8 : 4)) * (size_t)blockIdx.x;
        row[0] = nll;
        row[1] = vl;
#if BSK_FIT_STAMPS
        row[0] = (double)walk_ticks;
        row[1] = (double)(clock64() - t_start);
#endif
        row[2] = (double)correct;
        row[3] = (double)count;
        if constexpr (PG) {                // the policy-gradient row's terms, in the same order
            for (int k = 0; k < 4; ++k) {
                double acc = 0.0;
                for (int s = 0; s < POLICY_LANES; ++s) acc = acc + s_pg[k * POLICY_LANES + s];
                row[4 + k] = acc;
            }
        }
        if constexpr (VC) {                // the value-clip row's terms, in the same order
            for (int k = 0; k < 2; ++k) {
                double acc = 0.0;
                for (int s = 0; s < POLICY_LANES; ++s) acc = acc + s_vc[k * POLICY_LANES + s];
                row[8 + k] = acc;
            }
        }
    }
}

// W: the doubles of a block's diagnostics terms - 4, or 8 behind a policy-gradient launch, whose last four sums are pg_row's, or 10
// behind one with a FitVclip, whose last two are vclip_row's: an argument of <10, double*> alone (NULL: those two go nowhere)
template <int W, typename... Row>
__global__ __launch_bounds__(256) void fit_fold_kernel(const float* __restrict__ G, const double* __restrict__ diag, int n_blocks, int n_params,
                                                       int n_fold, double* __restrict__ A, double* __restrict__ row,
                                                       unsigned long long* __restrict__ count, double* __restrict__ pg_row,
                                                       const Row... vclip_row) {
    const int t = (int)(blockIdx.x * 256u + threadIdx.x);
    if (t < W) {                           // the diagnostics row: its four sums, block-ascending from +0.0
        double s = 0.0;
        int b = 0;
        for (; b + FIT_FOLD_BATCH <= n_blocks; b += FIT_FOLD_BATCH) {      // (fetched side by side, added in order: as below)
            double d[FIT_FOLD_BATCH];
#pragma unroll
            for (int i = 0; i < FIT_FOLD_BATCH; ++i) d[i] = diag[W * (size_t)(b + i) + t];
#pragma unroll
            for (int i = 0; i < FIT_FOLD_BATCH; ++i) s = s + d[i];
        }
        for (; b < n_blocks; ++b) s = s + diag[W * (size_t)b + t];
        if (W == 4 || t < 4) row[t] = s;
        else if (W == 8 || t < 8) pg_row[t - 4] = s;
        else if constexpr (W == 10) {
            double* const vrow[] = {vclip_row...};
            if (vrow[0]) vrow[0][t - 8] = s;
        }
        if (t == 3) *count += (unsigned long long)s;
    }
    const int p = 10 + t;
    if (p >= n_fold) return;
    // The chain is serial by definition; the loads are not.  FIT_FOLD_BATCH block values are fetched side by side and then added in
    // order: with one load per addition in flight the kernel was 1 024 dependent memory round trips long (469 us at 65 536 samples).
    const float* __restrict__ at = G + p;
    double acc = A[p];
    int b = 0;
    for (; b + FIT_FOLD_BATCH <= n_blocks; b += FIT_FOLD_BATCH) {
        float g[FIT_FOLD_BATCH];
#pragma unroll
        for (int i = 0; i < FIT_FOLD_BATCH; ++i) g[i] = at[(size_t)(b + i) * (size_t)n_params];
#pragma unroll
        for (int i = 0; i < FIT_FOLD_BATCH; ++i) acc = acc + (double)g[i];
    }
    for (; b < n_blocks; ++b) acc = acc + (double)at[(size_t)b * (size_t)n_params];
    A[p] = acc;
}

// bsk_fit_set_max_grad_norm: the global norm of the mean gradient over the parameters the step moves, and the factor that brings it
// down to max_norm (TensorFlow's clip_by_global_norm, PPO2's rule) - ONE workgroup, so that the order of the sum is the kernel's
// own.  Thread i adds g_q * g_q for q = i, i + 1024, ... ascending FROM the first (+0.0 with none); every wave joins its 64 in the
// fitness tree; thread 0 adds the sixteen wave sums ascending.  row = {norm, scale}: scale is exactly 1.0 while norm <= max_norm.
__global__ __launch_bounds__(FIT_GNORM_BLOCK) void fit_gnorm_kernel(const double* __restrict__ A, const unsigned long long* __restrict__ count,
                                                                    int n_upd, double max_norm, double* __restrict__ row) {
#pragma clang fp contract(off)
    __shared__ double s_wave[FIT_GNORM_BLOCK / 64];
    const int i = (int)threadIdx.x, lane = i & 63;
    const unsigned long long cnt = *count;
    if (cnt == 0ull) {                     // (workgroup-uniform: nothing moves, nothing is scaled)
        if (i == 0) { row[0] = 0.0; row[1] = 1.0; }
        return;
    }
    const int n = n_upd - 10;
    double s = 0.0;
    for (int q = i; q < n; q += FIT_GNORM_BLOCK) {
        const double g = A[10 + q] / (double)cnt;
        const double gg = g * g;
        s = q == i ? gg : s + gg;
    }
    s = fitness_tree(s, lane);
    if (lane == 0) s_wave[i >> 6] = s;
    __syncthreads();
    if (i == 0) {
        double S = s_wave[0];
        for (int w = 1; w < FIT_GNORM_BLOCK / 64; ++w) S = S + s_wave[w];
        const double norm = sqrt(S);
        row[0] = norm;
        row[1] = max_norm / (norm > max_norm ? norm : max_norm);
    }
}

// one parameter of the step: what every instantiation of fit_adam_kernel does with the EsAdam it ends up with
template <bool CLIP>
__device__ __forceinline__ void fit_adam_thread(double* __restrict__ theta, double* __restrict__ A, const unsigned long long* __restrict__ count,
                                                int p, const EsAdam& ad, const double* scale_row) {
    const unsigned long long cnt = *count;
    if (cnt != 0ull) {
        const double t = theta[p];
        if constexpr (CLIP) {
            theta[p] = t - adam_step(ad, p, (A[p] / (double)cnt) * scale_row[1] + ad.weight_decay * t);
        } else {
            theta[p] = t - adam_step(ad, p, A[p] / (double)cnt + ad.weight_decay * t);
        }
    }
    A[p] = 0.0;
}

// CLIP: the mean gradient times the scale fit_gnorm_kernel left, the L2 term added behind it.  <false> is the step without a clip,
// with the arguments it has always had: the clip's row is an argument of <true, const double*, ...> alone.  A FitSched - last -
// makes a scheduled step: a copy of `ad` takes its lr from the fit's schedule words (one uniform load) and goes through the same
// adam_step.
template <bool CLIP, typename... Row>
__global__ __launch_bounds__(256) void fit_adam_kernel(double* __restrict__ theta, double* __restrict__ A,
                                                       const unsigned long long* __restrict__ count, int n_upd, const EsAdam ad_in,
                                                       const Row... gnorm_row) {
    constexpr bool SCHED = (std::is_same_v<Row, FitSched> || ... || false);
    static_assert(sizeof...(Row) == (CLIP ? 1 : 0) + (SCHED ? 1 : 0), "the clip's row first, a FitSched last, nothing else");
    const int p = 10 + (int)(blockIdx.x * 256u + threadIdx.x);
    if (p >= n_upd) return;
    const double* scale_row = nullptr;
    if constexpr (CLIP) scale_row = std::get<0>(std::forward_as_tuple(gnorm_row...));
    if constexpr (SCHED) {
        EsAdam ad = ad_in;
        ad.lr = std::get<sizeof...(Row) - 1>(std::forward_as_tuple(gnorm_row...)).row[PG_SCHED_LR];
        fit_adam_thread<CLIP>(theta, A, count, p, ad, scale_row);
    } else {
        fit_adam_thread<CLIP>(theta, A, count, p, ad_in, scale_row);
    }
}

__global__ void fit_advance_kernel(unsigned long long* count, unsigned long long* steps, double* beta_pow, double beta1, double beta2) {
    if (*count != 0ull) {
        beta_pow[0] = beta_pow[0] * beta1;
        beta_pow[1] = beta_pow[1] * beta2;
        *steps += 1ull;
    }
    *count = 0ull;
}

// the alive bytes of a collection loop: one thread per env
__global__ __launch_bounds__(256) void fit_alive_kernel(const uint8_t* __restrict__ reason, int n, int first, uint8_t* __restrict__ alive) {
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    if (j < n) alive[j] = first || (alive[j] != 0 && reason[j] == 0) ? 1 : 0;        // (first: neither array is read)
}

// bsk_gae: env j's column of the histories from the last step to the first, f64, every operation rounded on its own (no FMA: the
// file's -ffp-contract=off).  A lane owns its env, so every load and store of a step is one coalesced row segment; no lane reads
// what another wrote.
__global__ __launch_bounds__(256) void gae_kernel(const double* __restrict__ reward, const uint8_t* __restrict__ reason,
                                                  const float* __restrict__ value, const float* __restrict__ last_value, int n_steps,
                                                  int n_envs, int64_t stride, double gamma, double gl, float* __restrict__ adv,
                                                  double* __restrict__ ret) {
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    if (j >= n_envs) return;
    double carry = 0.0;
    double next_v = last_value ? (double)last_value[j] : 0.0;
#pragma unroll 4
    for (int t = n_steps - 1; t >= 0; --t) {
        const int64_t at = (int64_t)t * stride + j;
        const double v = (double)value[at];
        const double rew = reward[at];
        if (reason[at] == 0) {
            const double delta = (rew + gamma * next_v) - v;
            carry = delta + gl * carry;
        } else {
            carry = rew - v;
        }
        adv[at] = (float)carry;
        if (ret) ret[at] = carry + v;
        next_v = v;
    }
}

// bsk_adv_normalize, first launch.  Wave w is the columns 64 w .. 64 w + 63 of the block, a lane its column: it walks the rows
// ascending, a1 = a1 + xd and a2 = a2 + xd * xd from +0.0 (xd = +0.0 where the sample does not count), then the wave joins in the
// fitness tree and lane 0 WRITES its partial sums and its count.  The chain is serial by definition; the loads are not:
// ADV_BATCH rows are fetched side by side and added in order, as in fit_fold_kernel.  Every load is one coalesced row segment.
__global__ __launch_bounds__(256) void adv_partial_kernel(const float* __restrict__ adv, const uint8_t* __restrict__ alive, int rows, int n,
                                                          int64_t stride, int waves, double* __restrict__ part,
                                                          unsigned long long* __restrict__ cnt) {
#pragma clang fp contract(off)
    const int w = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));     // (wave-uniform)
    const int lane = (int)(threadIdx.x & 63u);
    if (w >= waves) return;
    const int c = w * 64 + lane;
    const bool in = c < n;
    const float* __restrict__ x = adv + (in ? c : 0);
    const uint8_t* __restrict__ live = alive ? alive + (in ? c : 0) : nullptr;
    double a1 = 0.0, a2 = 0.0;
    long long k = 0;
    int t = 0;
    for (; t + ADV_BATCH <= rows; t += ADV_BATCH) {
        float v[ADV_BATCH];
        bool on[ADV_BATCH];
#pragma unroll
        for (int i = 0; i < ADV_BATCH; ++i) {
            const int64_t at = (int64_t)(t + i) * stride;
            on[i] = in && (!live || live[at] != 0);
            v[i] = in ? x[at] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < ADV_BATCH; ++i) {
            const double xd = on[i] ? (double)v[i] : 0.0;
            a1 = a1 + xd;
            a2 = a2 + xd * xd;
            k += on[i] ? 1 : 0;
        }
    }
    for (; t < rows; ++t) {
        const int64_t at = (int64_t)t * stride;
        const bool on = in && (!live || live[at] != 0);
        const double xd = on ? (double)x[at] : 0.0;
        a1 = a1 + xd;
        a2 = a2 + xd * xd;
        k += on ? 1 : 0;
    }
    a1 = fitness_tree(a1, lane);
    a2 = fitness_tree(a2, lane);
    k = count_tree(k, lane);
    if (lane == 0) {
        part[2 * (size_t)w] = a1;
        part[2 * (size_t)w + 1] = a2;
        cnt[w] = (unsigned long long)k;
    }
}

// Second launch, three waves: obs_stats_join_kernel's rule on the two columns of the partial sums and on the counts - lane l adds
// the entries w = l, l + 64, ... ascending FROM the first (+0.0 with none), then the tree - and one thread forms the four words
// {mean, sd, inv, (double)N} out of the totals; four +0.0 when nothing counts.
__global__ __launch_bounds__(192) void adv_join_kernel(const double* __restrict__ part, const unsigned long long* __restrict__ cnt, int waves,
                                                       double eps, double* __restrict__ mom) {
#pragma clang fp contract(off)
    __shared__ double s_tot[2];
    __shared__ unsigned long long s_n;
    const int c = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63u);
    if (c < 2) {
        double s = 0.0;
        for (int w = lane; w < waves; w += 64) {
            const double v = part[2 * (size_t)w + c];
            s = w == lane ? v : s + v;
        }
        s = fitness_tree(s, lane);
        if (lane == 0) s_tot[c] = s;
    } else {
        long long s = 0;
        for (int w = lane; w < waves; w += 64) s += (long long)cnt[w];
        s = count_tree(s, lane);
        if (lane == 0) s_n = (unsigned long long)s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long N = s_n;
        if (N == 0ull) {
            mom[0] = mom[1] = mom[2] = mom[3] = 0.0;
        } else {
            double mean, var;
            obs_moments(s_tot[0], s_tot[1], N, mean, var);
            const double sd = sqrt(var);
            mom[0] = mean;
            mom[1] = sd;
            mom[2] = 1.0 / (sd + eps);
            mom[3] = (double)N;
        }
    }
}

// Third launch, elementwise over the columns below n: a counting sample becomes (float)(((double)x - mean) * inv), any other +0.0f;
// nothing is written while N == 0.  A thread reads and writes its own element alone, so out may be adv.
__global__ __launch_bounds__(256) void adv_apply_kernel(const float* adv, const uint8_t* __restrict__ alive, int rows, int n, int64_t stride,
                                                        const double* __restrict__ mom, float* out) {
#pragma clang fp contract(off)
    const int c = (int)(blockIdx.x * 256u + threadIdx.x);
    if (c >= n || mom[3] == 0.0) return;
    const double mean = mom[0], inv = mom[2];
    for (int t = (int)blockIdx.y; t < rows; t += (int)gridDim.y) {
        const int64_t at = (int64_t)t * stride + c;
        const bool on = !alive || alive[at] != 0;
        out[at] = on ? (float)(((double)adv[at] - mean) * inv) : 0.0f;
    }
}

hipError_t launch_adv_normalize(const float* adv, const uint8_t* alive, int rows, int n, int64_t stride, double eps, float* out, double* work,
                                hipStream_t s) {
    const int waves = (n + 63) / 64;
    double* part = work + 4;
    unsigned long long* cnt = (unsigned long long*)(part + 2 * (size_t)waves);
    hipLaunchKernelGGL(adv_partial_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, adv, alive, rows, n, stride, waves, part, cnt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(adv_join_kernel, dim3(1), dim3(192), 0, s, (const double*)part, (const unsigned long long*)cnt, waves, eps, work);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(adv_apply_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)(rows < ADV_APPLY_ROWS ? rows : ADV_APPLY_ROWS)), dim3(256), 0,
                       s, adv, alive, rows, n, stride, (const double*)work, out);
    return hipGetLastError();
}

hipError_t launch_gae(const double* reward, const uint8_t* reason, const float* value, const float* last_value, int n_steps, int n_envs,
                      int64_t stride, double gamma, double gl, float* adv, double* ret, hipStream_t s) {
    hipLaunchKernelGGL(gae_kernel, dim3((unsigned)((n_envs + 255) / 256)), dim3(256), 0, s, reward, reason, value, last_value, n_steps,
                       n_envs, stride, gamma, gl, adv, ret);
    return hipGetLastError();
}

hipError_t launch_fit_alive(const uint8_t* reason, int n, int first, uint8_t* alive, hipStream_t s) {
    hipLaunchKernelGGL(fit_alive_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, reason, n, first, alive);
    return hipGetLastError();
}

int fit_lds_rows(const PolicyLayout& lay) {
    const PolicyNet* nets[2] = {&lay.a, &lay.v};
    int most = 0;
    for (const PolicyNet* net : nets) {
        int hidden = 0;
        for (int l = 0; l + 1 < net->n_layers; ++l) hidden += net->N[l];
        if (hidden > most) most = hidden;
    }
    return FIT_X_ROWS + most + POLICY_OB;
}

FitNet fit_net(const PolicyPackMap& map, int first, const PolicyNet& net) {
    FitNet f = {};
    f.n_layers = net.n_layers;
    f.act = net.act;
    for (int l = 0; l < net.n_layers; ++l) f.layer[l] = map.layer[first + l];
    return f;
}

template <bool PG, typename... Vc>
static hipError_t launch_fit_blocks_as(const FitArgs& args, hipStream_t s, const Vc&... vclip) {
    constexpr bool VC = (std::is_same_v<Vc, FitVclip> || ... || false);
    const size_t lds = (size_t)(args.rows + FIT_DIAG_ROWS + (PG ? FIT_PG_DIAG_ROWS : 0) + (VC ? FIT_VC_DIAG_ROWS : 0)) *
                       POLICY_LANES * sizeof(float);
    if (lds > 48 * 1024) {                 // (idempotent, and cheap beside the launch: no per-device record to keep)
        hipError_t e = hipFuncSetAttribute((const void*)&fit_block_kernel<PG, Vc...>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const unsigned n_blocks = (unsigned)((args.n + FIT_BLOCK_SAMPLES - 1) / FIT_BLOCK_SAMPLES);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(fit_block_kernel<PG, Vc...>), dim3(n_blocks), dim3(POLICY_BLOCK), lds, s, args, vclip...);
    return hipGetLastError();
}

hipError_t launch_fit_blocks(const FitArgs& args, hipStream_t s) { return launch_fit_blocks_as<false>(args, s); }
hipError_t launch_fit_blocks_pg(const FitArgs& args, hipStream_t s) { return launch_fit_blocks_as<true>(args, s); }
hipError_t launch_fit_blocks_ppo(const FitArgs& args, const FitVclip& vc, hipStream_t s) { return launch_fit_blocks_as<true>(args, s, vc); }
hipError_t launch_fit_blocks_pg_sched(const FitArgs& args, const double* sched, hipStream_t s) {
    return launch_fit_blocks_as<true>(args, s, FitSched{sched});
}
hipError_t launch_fit_blocks_ppo_sched(const FitArgs& args, const FitVclip& vc, const double* sched, hipStream_t s) {
    return launch_fit_blocks_as<true>(args, s, vc, FitSched{sched});
}

hipError_t launch_fit_fold(const float* G, const double* diag, int n_blocks, int n_params, int n_fold, double* A, double* row,
                           unsigned long long* count, hipStream_t s) {
    const int threads = n_fold - 10 > 4 ? n_fold - 10 : 4;
    hipLaunchKernelGGL(fit_fold_kernel<4>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, G, diag, n_blocks, n_params, n_fold, A,
                       row, count, (double*)nullptr);
    return hipGetLastError();
}

hipError_t launch_fit_fold_pg(const float* G, const double* diag, int n_blocks, int n_params, int n_fold, double* A, double* row,
                              double* pg_row, unsigned long long* count, hipStream_t s) {
    const int threads = n_fold - 10 > 8 ? n_fold - 10 : 8;
    hipLaunchKernelGGL(fit_fold_kernel<8>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, G, diag, n_blocks, n_params, n_fold, A,
                       row, count, pg_row);
    return hipGetLastError();
}

hipError_t launch_fit_fold_ppo(const float* G, const double* diag, int n_blocks, int n_params, int n_fold, double* A, double* row,
                               double* pg_row, double* vclip_row, unsigned long long* count, hipStream_t s) {
    const int threads = n_fold - 10 > 10 ? n_fold - 10 : 10;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(fit_fold_kernel<10, double*>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, G, diag, n_blocks,
                       n_params, n_fold, A, row, count, pg_row, vclip_row);
    return hipGetLastError();
}

hipError_t launch_fit_step(double* theta, double* A, unsigned long long* count, unsigned long long* steps, int n_upd, const EsAdam& ad,
                           double max_norm, double* gnorm_row, hipStream_t s, const double* sched) {
    if (n_upd > 10) {
        const dim3 grid((unsigned)((n_upd - 10 + 255) / 256));
        if (max_norm > 0.0) {              // one launch in front, over the range the step moves
            hipLaunchKernelGGL(fit_gnorm_kernel, dim3(1), dim3(FIT_GNORM_BLOCK), 0, s, (const double*)A, (const unsigned long long*)count, n_upd,
                               max_norm, gnorm_row);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
            if (sched)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(fit_adam_kernel<true, const double*, FitSched>), grid, dim3(256), 0, s, theta, A, count,
                                   n_upd, ad, (const double*)gnorm_row, FitSched{sched});
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(fit_adam_kernel<true, const double*>), grid, dim3(256), 0, s, theta, A, count, n_upd, ad,
                                   (const double*)gnorm_row);
        } else if (sched) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(fit_adam_kernel<false, FitSched>), grid, dim3(256), 0, s, theta, A, count, n_upd, ad,
                               FitSched{sched});
        } else {
            hipLaunchKernelGGL(fit_adam_kernel<false>, grid, dim3(256), 0, s, theta, A, count, n_upd, ad);
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(fit_advance_kernel, dim3(1), dim3(1), 0, s, count, steps, const_cast<double*>(ad.beta_pow), ad.beta1, ad.beta2);
    return hipGetLastError();
}

}  // namespace bsk
