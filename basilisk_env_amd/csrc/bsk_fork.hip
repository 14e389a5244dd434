// bsk_fork.hip — forking spacecraft states on the device and choosing among rollouts (a translation unit of its own, beside
// bsk_aux.hip; neither touches the step or rollout kernels):
//   fork_kernel     env j of one handle becomes an exact copy of env map[j] of another (or the same) handle: every buffer that
//                   decides an env's future or reports its present (bsk_fork_device, include/bskgpu.h)
//   select_kernel   discounted value of every branch of a rollout history, best branch per group of `group` (bsk_select_branches);
//                   <true>: plus a discounted leaf value for the branches no step ended (bsk_select_branches_boot)
//   beam_kernel     one level of a beam search: the `width` best of every root's 3 * width candidates (bsk_beam_select);
//                   <true>: ranked by value + discounted leaf value of the live candidates (bsk_beam_select_boot)
// Compiled with -ffp-contract=off (Makefile): select_kernel's and beam_kernel's additions and products are the ones a numpy
// restatement makes.
#include "bsk_device.hpp"
#include "bsk_aux.hpp"

#include <climits>

namespace bsk {

// One thread per destination env, 256 per workgroup (whole waves: every lane of a wave reaches the done ballot).  Destination rows
// are written coalesced; source rows are gathered at map[j], which for the planner's map (j / 3^depth) is the same or the next column
// for neighbouring lanes, and for a permutation whatever the caller asked for.  Field rows are moved eight at a time (eight loads in
// flight before the first store).  Every store is a plain vector store.
constexpr int FORK_BLOCK = 256;
__global__ __launch_bounds__(FORK_BLOCK) void fork_kernel(const ForkSide src, const ForkSide dst, int nf, const int* __restrict__ map,
                                                           int identity, int* err, unsigned long long* seal_word) {
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const bool live = j < dst.n;
    int s = -1;                                  // source env of this lane, -1: leave env j as it is
    if (live) {
        const int m = map[j];
        if (m >= 0 && m < src.n) s = identity ? j : m;
        else if (m != -1 && err) __hip_atomic_store(err, BSK_DEVERR_FORK_MAP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // the done ballot: the source's bit for mapped lanes, the old bit for -1 lanes, 0 for tail lanes (the step kernel's convention)
    bool bit = false;
    if (s >= 0) bit = ((src.done_mask[s >> 6] >> (s & 63)) & 1ull) != 0;
    else if (live) bit = ((dst.done_mask[j >> 6] >> (j & 63)) & 1ull) != 0;
    const unsigned long long word = __ballot(bit);
    if ((threadIdx.x & 63) == 0 && live) dst.done_mask[j >> 6] = word;
    // the destination's batch-scalar snapshot no longer describes its buffers: lift the seal a reset left (bsk_aux.hip: stats_sealed)
    if (j == 0 && seal_word) seal_word[2] = 0ull;
    if (s < 0) return;

    const double* __restrict__ ss = src.st;
    double* __restrict__ ds = dst.st;
    int f = 0;
    for (; f + 8 <= nf; f += 8) {
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = ss[(int64_t)(f + k) * src.stride + s];
#pragma unroll
        for (int k = 0; k < 8; ++k) ds[(int64_t)(f + k) * dst.stride + j] = v[k];
    }
    for (; f < nf; ++f) ds[(int64_t)f * dst.stride + j] = ss[(int64_t)f * src.stride + s];
    dst.cnt[j] = src.cnt[s];                     // the whole word: the FSW phase lives in bits 20+ of .x
    double o[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) o[k] = src.obs[(int64_t)k * src.ostride + s];
#pragma unroll
    for (int k = 0; k < 5; ++k) dst.obs[(int64_t)k * dst.ostride + j] = o[k];
    dst.reward[j] = src.reward[s];
    dst.reason[j] = src.reason[s];
    if (dst.obs_rm) {                            // (the same observation as the rows above, whichever layout the source keeps)
#pragma unroll
        for (int k = 0; k < 5; ++k) dst.obs_rm[(int64_t)j * 5 + k] = o[k];
    }
    if (dst.ep_return) dst.ep_return[j] = src.ep_return ? src.ep_return[s] : 0.0;
    if (dst.term_return) dst.term_return[j] = src.term_return ? src.term_return[s] : 0.0;
    if (dst.term_len) dst.term_len[j] = src.term_len ? src.term_len[s] : 0;
    if (dst.done) dst.done[j] = src.done ? src.done[s] : (unsigned char)0;
    if (dst.term_obs) {
#pragma unroll
        for (int k = 0; k < 5; ++k) dst.term_obs[(int64_t)k * dst.ostride + j] = src.term_obs ? src.term_obs[(int64_t)k * src.ostride + s] : 0.0;
    }
    if (dst.episodes) dst.episodes[j] = src.episodes ? src.episodes[s] : 0;
}

hipError_t launch_fork(const ForkSide& src, const ForkSide& dst, int nf, const int* map, bool identity, int* err,
                       unsigned long long* seal_word, hipStream_t s) {
    hipLaunchKernelGGL(fork_kernel, dim3((dst.n + FORK_BLOCK - 1) / FORK_BLOCK), dim3(FORK_BLOCK), 0, s, src, dst, nf, map, identity ? 1 : 0,
                       err, seal_word);
    return hipGetLastError();
}

// (value, index) order of the branch choice: the greater value wins, equal values go to the lower index, NaN loses to every number
// (and among NaNs the lower index wins, so that a group of NaNs picks its first branch)
__device__ __forceinline__ bool beats(double a, int ia, double b, int ib) {
    const bool na = a != a, nb = b != b;
    if (na != nb) return nb;
    if (!na && a != b) return a > b;
    return ia < ib;
}

// One wave per group of `group` consecutive branches, 64 branches per trip.  Lane l evaluates branch b of the trip:
//   v = 0, g = 1;  for t in 0 .. T-1: v = v + g * r[t][b]; g = g * gamma; stop after the first t with reason[t][b] != 0
// (that step's reward included), every operation rounded on its own - no contraction into FMAs - so that numpy's evaluation of the
// same expression gives the same bits.  The lanes' best (value, index) pairs are joined by a butterfly under the total order of
// beats(): any joining order gives the same winner.
// BOOT (bsk_select_branches_boot): a branch that no step ended also takes  v = v + g * (double)leaf[b]  with the g the loop left
// (T multiplications), product and sum each rounded on their own; a branch that ended - at the last step too - takes nothing.
// One text serves both entry points: without BOOT `leaf` is not read and the instantiation is the kernel as it was.
template <bool BOOT>
__global__ __launch_bounds__(256) void select_kernel(const double* __restrict__ rh, const unsigned char* __restrict__ qh,
                                                      const int* __restrict__ first_action, int T, int n_branch, int group, int n_groups,
                                                      double gamma, const float* __restrict__ leaf, double* __restrict__ values,
                                                      double* __restrict__ best_value, int* __restrict__ best_action) {
#pragma clang fp contract(off)
    const int g = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));     // (wave-uniform)
    const int lane = (int)(threadIdx.x & 63u);
    if (g >= n_groups) return;
    const int64_t b0 = (int64_t)g * group;
    double bv = __builtin_nan("");
    int bi = INT_MAX;
    for (int c = 0; c < group; c += 64) {
        const int i = c + lane;
        if (i >= group) continue;
        const int64_t b = b0 + i;
        double v = 0.0, w = 1.0;
        bool ended = false;
        for (int t = 0; t < T; ++t) {
            const int64_t at = (int64_t)t * n_branch + b;
            const double p = w * rh[at];
            v = v + p;
            w = w * gamma;
            if (qh[at] != 0) { ended = true; break; }
        }
        if constexpr (BOOT) {
            if (!ended) {
                const double p = w * (double)leaf[b];
                v = v + p;
            }
        }
        if (values) values[b] = v;
        if (beats(v, i, bv, bi)) { bv = v; bi = i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (beats(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
        if (best_value) best_value[g] = bv;
        best_action[g] = first_action[b0 + bi];
    }
}

// leaf: f32[n_branch] (bsk_select_branches_boot), or NULL for the kernel without the leaf term (bsk_select_branches)
hipError_t launch_select(const double* reward_hist, const unsigned char* reason_hist, const int* first_action, int n_steps, int n_branch,
                         int group, double gamma, const float* leaf, double* values, double* best_value, int* best_action, hipStream_t s) {
    const int n_groups = n_branch / group;
    if (leaf)
        hipLaunchKernelGGL(select_kernel<true>, dim3((n_groups + 3) / 4), dim3(256), 0, s, reward_hist, reason_hist, first_action, n_steps,
                           n_branch, group, n_groups, gamma, leaf, values, best_value, best_action);
    else
        hipLaunchKernelGGL(select_kernel<false>, dim3((n_groups + 3) / 4), dim3(256), 0, s, reward_hist, reason_hist, first_action, n_steps,
                           n_branch, group, n_groups, gamma, leaf, values, best_value, best_action);
    return hipGetLastError();
}

// One level of a beam search.  A workgroup takes 256 / (3 * width) whole roots, one thread per candidate, so that small widths fill
// the workgroup with roots instead of idle lanes (width 1: 85 roots, width 9: 9, width 81: 1).  Each thread builds its candidate
// from the parent slot, puts (value, valid) in LDS and counts the candidates of its root that come before it; the order is total,
// so that count is its rank and no two candidates share one.  The threads of rank < width write their slot: plain stores, one
// barrier, no atomics.  Nothing outside the 3 * width * n_roots candidates and the width * n_roots parent slots is read.
// BOOT (bsk_beam_select_boot): the candidates are ranked by a key - value + boot_weight * (double)leaf[c] for a valid candidate that
// is live after this step (product, then sum), the value itself otherwise - which takes the value's place in s_value; the slot keeps
// the value v, so the next level continues the true return.  Without BOOT key and value are one and the instantiation is the kernel
// as it was.
constexpr int BEAM_BLOCK = 256;
template <bool BOOT>
__global__ __launch_bounds__(BEAM_BLOCK) void beam_kernel(const double* __restrict__ reward, const unsigned char* __restrict__ reason,
                                                           int n_roots, int width, int level, double weight, double boot_weight,
                                                           const float* __restrict__ leaf,
                                                           const bsk_beam_slot* __restrict__ in, bsk_beam_slot* __restrict__ out,
                                                           int* __restrict__ map, double* __restrict__ key_out,
                                                           double* __restrict__ best_value, int* __restrict__ best_action) {
#pragma clang fp contract(off)
    __shared__ double s_value[BEAM_BLOCK];
    __shared__ unsigned char s_valid[BEAM_BLOCK];
    const int nc = 3 * width;                                  // candidates per root (<= 243)
    const int per = BEAM_BLOCK / nc;                           // roots per workgroup
    const int t = (int)threadIdx.x;
    const int lr = t / nc, i = t - lr * nc;                    // root within the workgroup, candidate within the root
    const int root = (int)blockIdx.x * per + lr;
    const bool active = lr < per && root < n_roots;
    const int c = active ? root * nc + i : 0;                  // (< 3 * width * n_roots < 2^31)
    double v = __builtin_nan("");                              // an invalid candidate: NaN, first -1, no flags
    int first = -1;
    unsigned flags = 0u;
    if (active) {
        const int a = i % 3;
        if (level == 0) {
            if (i < 3) {                                       // slot 0 of the root is the one real parent
                v = 0.0 + weight * reward[c];
                first = a;
                flags = BSK_BEAM_VALID | (reason[c] == 0 ? BSK_BEAM_LIVE : 0u);
            }
        } else {
            const bsk_beam_slot ps = in[c / 3];
            const bool live = (ps.flags & BSK_BEAM_LIVE) != 0u;
            if ((ps.flags & BSK_BEAM_VALID) && (live || a == 0)) {   // a finished sequence continues as one candidate
                if (live) {
                    const double p = weight * reward[c];
                    v = ps.value + p;
                } else {
                    v = ps.value;
                }
                first = ps.first;
                flags = BSK_BEAM_VALID | (live && reason[c] == 0 ? BSK_BEAM_LIVE : 0u);
            }
        }
    }
    const bool ok = flags != 0u;
    double key = v;                                            // what the candidate is ranked by (an invalid one: NaN)
    if constexpr (BOOT) {
        if ((flags & BSK_BEAM_LIVE) != 0u) {                   // (live implies valid; c < 3 * width * n_roots, the leaf's length)
            const double p = boot_weight * (double)leaf[c];
            key = v + p;
        }
    }
    s_value[t] = key;
    s_valid[t] = ok ? 1 : 0;
    __syncthreads();
    if (!active) return;
    const int base = lr * nc;
    int rank = 0;
    for (int j = 0; j < nc; ++j) {                             // candidates of this root that come before candidate i
        const bool okj = s_valid[base + j] != 0;
        const bool before = okj != ok ? okj : (ok ? beats(s_value[base + j], j, key, i) : j < i);
        rank += before ? 1 : 0;
    }
    if (rank < width) {
        const int s = root * width + rank;
        bsk_beam_slot o;
        o.value = v;
        o.first = first;
        o.flags = flags;
        out[s] = o;
        map[s] = ok ? c : -1;
        if constexpr (BOOT) {
            if (key_out) key_out[s] = key;
        }
        if (rank == 0) {
            best_value[root] = key;
            best_action[root] = first;
        }
    }
}

// leaf: f32[3 * width * n_roots] with boot_weight and key (f64[n_roots * width] or NULL) (bsk_beam_select_boot), or NULL for the
// kernel without the leaf term (bsk_beam_select)
hipError_t launch_beam(const double* reward, const unsigned char* reason, int n_roots, int width, int level, double weight,
                       double boot_weight, const float* leaf, const bsk_beam_slot* in, bsk_beam_slot* out, int* map, double* key,
                       double* best_value, int* best_action, hipStream_t s) {
    const int per = BEAM_BLOCK / (3 * width);
    if (leaf)
        hipLaunchKernelGGL(beam_kernel<true>, dim3((n_roots + per - 1) / per), dim3(BEAM_BLOCK), 0, s, reward, reason, n_roots, width, level,
                           weight, boot_weight, leaf, in, out, map, key, best_value, best_action);
    else
        hipLaunchKernelGGL(beam_kernel<false>, dim3((n_roots + per - 1) / per), dim3(BEAM_BLOCK), 0, s, reward, reason, n_roots, width, level,
                           weight, boot_weight, leaf, in, out, map, key, best_value, best_action);
    return hipGetLastError();
}

}  // namespace bsk
