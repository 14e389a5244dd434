// bsk_shuffle.hip — shuffled minibatches for the policy-gradient loop (bsk_pg_gather, bsk_pg_shuffle_advance; definition in
// include/bskgpu.h).
//   pg_gather_kernel     one thread per output position i: s = perm(q0 + i) (bsk_shuffle.hpp), then the sample's five observation
//                        words, action, advantage, old log-probability, return and old value out of the histories into position i
//                        of a contiguous minibatch.  The round keys are formed once per thread from the two state words (a uniform
//                        load, uniform arithmetic); the cycle walk is the only divergent loop.  Stores are coalesced along i; the
//                        loads are scattered by construction - up to ten reads of 4 or 8 bytes per sample, each its own cache
//                        line - so the kernel wants every wave the CU can hold in flight: 256 threads, 24 VGPRs, no LDS, eight
//                        waves per SIMD; every load of a thread is issued before its first store.
//   pg_advance_kernel    one thread: epoch += 1
// No atomics, no cross-lane traffic, plain stores: a position is written by its own thread alone.
#include "bsk_shuffle.hpp"

namespace bsk {

constexpr int PG_GATHER_BLOCK = 256;

__global__ __launch_bounds__(PG_GATHER_BLOCK) void pg_gather_kernel(const PgGatherArgs p) {
    const int i = (int)(blockIdx.x * (unsigned)PG_GATHER_BLOCK + threadIdx.x);
    if (i >= p.m) return;
    uint32_t s = (uint32_t)(p.q0 + i);             // (q0 + m <= N < 2^31: checked on the host)
    if (p.state) {                                 // (grid-uniform)
        uint32_t k[SHUFFLE_ROUNDS];
        shuffle_keys(p.state, k);
        s = shuffle_perm(s, p.N, shuffle_bits(p.N), k);
    }
    const uint32_t n = (uint32_t)p.n_envs;
    const uint32_t t = s / n, j = s - t * n;
    const int64_t at = (int64_t)t * p.stride + (int64_t)j;
    // every load first, side by side - up to ten cache lines in flight per lane -, then the stores: a store between two loads would
    // hold the second back (the compiler cannot know that no output aliases a history)
    double o[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, ret = 0.0;
    int32_t action = 0;
    float adv = 0.0f, logp = 0.0f, value = 0.0f;
    if (p.obs) {
        const double* from = p.obs + (int64_t)t * 5 * p.stride + (int64_t)j;
#pragma unroll
        for (int r = 0; r < 5; ++r) o[r] = from[(int64_t)r * p.stride];
    }
    if (p.action) action = p.action[at];
    if (p.adv) adv = p.adv[at];
    if (p.logp) logp = p.logp[at];
    if (p.ret) ret = p.ret[at];
    if (p.value) value = p.value[at];
    if (p.index_out) p.index_out[i] = (int32_t)s;
    if (p.obs) {
#pragma unroll
        for (int r = 0; r < 5; ++r) p.obs_out[(int64_t)r * p.out_stride + i] = o[r];
    }
    if (p.action) p.action_out[i] = action;
    if (p.adv) p.adv_out[i] = adv;
    if (p.logp) p.logp_out[i] = logp;
    if (p.ret) p.ret_out[i] = ret;
    if (p.value) p.value_out[i] = value;
}

__global__ void pg_advance_kernel(unsigned long long* state) { state[1] += 1ull; }

hipError_t launch_pg_gather(const PgGatherArgs& args, hipStream_t s) {
    hipLaunchKernelGGL(pg_gather_kernel, dim3((unsigned)((args.m + PG_GATHER_BLOCK - 1) / PG_GATHER_BLOCK)), dim3(PG_GATHER_BLOCK), 0, s, args);
    return hipGetLastError();
}

hipError_t launch_pg_shuffle_advance(unsigned long long* state, hipStream_t s) {
    hipLaunchKernelGGL(pg_advance_kernel, dim3(1), dim3(1), 0, s, state);
    return hipGetLastError();
}

}  // namespace bsk
