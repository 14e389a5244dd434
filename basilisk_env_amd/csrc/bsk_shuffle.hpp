// bsk_shuffle.hpp — the stateless permutation of [0, N) behind the shuffled minibatches of the policy-gradient loop (bsk_pg_gather;
// definition in include/bskgpu.h): an unbalanced Feistel network of eight rounds over 2^b >= N values, walked until it lands below
// N.  Nothing is stored: the eight round keys come from {seed, epoch} through Philox (bsk_philox.hpp), everything else is uint32
// arithmetic that numpy repeats bit for bit (policy_ref.py: pg_perm_ref).
// shuffle_perm is plain integer C++: tools/pg_perm_host.cpp compiles it for the host (BSK_SHUFFLE_HOST: no HIP header, no
// qualifier) and tests/test_pg_shuffle_host.py holds it to the restatement, walk and all, before a GPU runs it.
#pragma once
#include <stdint.h>

#ifdef BSK_SHUFFLE_HOST
#define BSK_SHUFFLE_FN inline
#else
#include <hip/hip_runtime.h>
#define BSK_SHUFFLE_FN __device__ __forceinline__
#endif

namespace bsk {

constexpr int SHUFFLE_ROUNDS = 8;          // (four leave the pairs (q, perm(q)) measurably uneven at small N: DESIGN.md)
constexpr uint32_t SHUFFLE_TAG = 0x50475348u;      // "PGSH": the third counter word of the key draws

// murmur3's finaliser: the round function's mixing
BSK_SHUFFLE_FN uint32_t shuffle_fmix(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// b = max(2, bit_length(N - 1)): the network permutes 2^b < 2 N values (1 <= N < 2^31, so b <= 31)
BSK_SHUFFLE_FN int shuffle_bits(uint32_t N) {
    int b = 0;
    for (uint32_t v = N - 1u; v != 0u; v >>= 1) ++b;
    return b < 2 ? 2 : b;
}

// perm(q) for q < N.  The walk has NO cap: the 2^b-permutation's cycle through q comes back to q < N, so it ends, and a cap would
// break the bijection.  It is the one divergent loop of the gather (mean below two trips).
BSK_SHUFFLE_FN uint32_t shuffle_perm(uint32_t q, uint32_t N, int b, const uint32_t* k) {
    const int a = b >> 1, c = b - a;
    const uint32_t mask_a = (1u << a) - 1u, mask_c = (1u << c) - 1u;
    uint32_t x = q;
    do {
        uint32_t L = x >> c, R = x & mask_c;
        uint32_t ml = mask_a, mr = mask_c;         // the masks of the widths (wl, wr) = (a, c), swapped behind every round
#pragma unroll
        for (int r = 0; r < SHUFFLE_ROUNDS; ++r) {
            const uint32_t F = shuffle_fmix(R ^ k[r]) & ml;
            const uint32_t nr = L ^ F;
            L = R;
            R = nr;
            const uint32_t t = ml; ml = mr; mr = t;
        }
        x = (L << c) | R;                          // (an even number of rounds: the widths are (a, c) again)
    } while (x >= N);
    return x;
}

#ifndef BSK_SHUFFLE_HOST
}  // namespace bsk
#include "bsk_philox.hpp"
namespace bsk {

// k[4 i .. 4 i + 3] = philox4x32_10(epoch_lo, epoch_hi, SHUFFLE_TAG, i; seed_lo, seed_hi), i = 0, 1.  state = {seed, epoch}
__device__ __forceinline__ void shuffle_keys(const unsigned long long* __restrict__ state, uint32_t* k) {
    const unsigned long long seed = state[0], epoch = state[1];
#pragma unroll
    for (unsigned i = 0; i < 2u; ++i)
        philox4x32_10((unsigned)epoch, (unsigned)(epoch >> 32), SHUFFLE_TAG, i, (unsigned)seed, (unsigned)(seed >> 32), k + 4 * i);
}

// One minibatch out of the rollout histories (bsk_pg_gather): output position i takes sample s = perm(q0 + i)
struct PgGatherArgs {
    const unsigned long long* state;       // {seed, epoch}, or NULL: s = q0 + i
    int n_envs;
    uint32_t N;                            // n_steps * n_envs
    int64_t stride, q0;
    int m;
    int64_t out_stride;
    const double* obs;                     // [n_steps][5][stride] -> obs_out [5][out_stride]
    const int32_t* action;                 // the rest [n_steps][stride] -> [m]; a NULL source has a NULL destination
    const float* adv;
    const float* logp;
    const double* ret;
    const float* value;
    double* obs_out;
    int32_t* action_out;
    float* adv_out;
    float* logp_out;
    double* ret_out;
    float* value_out;
    int32_t* index_out;                    // [m] or NULL: s itself
};

hipError_t launch_pg_gather(const PgGatherArgs& args, hipStream_t s);
// epoch += 1: one thread
hipError_t launch_pg_shuffle_advance(unsigned long long* state, hipStream_t s);
#endif

}  // namespace bsk
