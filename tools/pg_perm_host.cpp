// pg_perm_host.cpp — csrc/bsk_shuffle.hpp's shuffle_perm, the device function behind bsk_pg_gather, compiled for the HOST: the
// permutation and its uncapped cycle walk are plain integer C++, so the bijection is shown on the CPU before a GPU runs the loop
// (tests/test_pg_shuffle_host.py compares the output with policy_ref.pg_perm_keys_ref).
//   c++ -O1 -std=c++17 [-fsanitize=address,undefined] -DBSK_SHUFFLE_HOST -I basilisk_env_amd/csrc tools/pg_perm_host.cpp -o pg_perm_host
//   pg_perm_host N k0 k1 k2 k3 k4 k5 k6 k7      -> perm(0) ... perm(N - 1), one per line
// The round keys are arguments: deriving them from {seed, epoch} is Philox's part (bsk_philox.hpp), tested where it is used.
#ifndef BSK_SHUFFLE_HOST
#define BSK_SHUFFLE_HOST 1
#endif
#include <cstdio>
#include <cstdlib>

#include "bsk_shuffle.hpp"

int main(int argc, char** argv) {
    if (argc != 2 + bsk::SHUFFLE_ROUNDS) {
        std::fprintf(stderr, "usage: %s N k0 ... k7\n", argv[0]);
        return 2;
    }
    const unsigned long long n = std::strtoull(argv[1], nullptr, 0);
    if (n < 1ull || n >= (1ull << 31)) {
        std::fprintf(stderr, "N must be in 1 .. 2^31 - 1\n");
        return 2;
    }
    uint32_t k[bsk::SHUFFLE_ROUNDS];
    for (int r = 0; r < bsk::SHUFFLE_ROUNDS; ++r) k[r] = (uint32_t)std::strtoull(argv[2 + r], nullptr, 0);
    const uint32_t N = (uint32_t)n;
    const int b = bsk::shuffle_bits(N);
    for (uint32_t q = 0; q < N; ++q) std::printf("%u\n", bsk::shuffle_perm(q, N, b, k));
    return 0;
}
