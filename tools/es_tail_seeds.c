/* es_tail_seeds.c — seeds under which the evolution strategy's first draw of a parameter falls into the FAR tail of the inverse
 * normal CDF (es_inverse_normal in basilisk_env_amd/csrc/bsk_es.hip: r > 5, the E / F rationals).
 *
 * z(g, i, j) is one Philox4x32-10 call: key (seed lo, seed hi), counter (j, i, g lo, g hi), k = (w0 >> 6) * 2^26 + (w1 >> 6),
 * u = (k + 0.5) * 2^-52.  The far branch needs min(u, 1 - u) < e^-25, which is k <= K_FAR or k >= 2^52 - 1 - K_FAR with
 * K_FAR = 62545 (tests/test_es_host.py finds the same switch by bisection on the restatement): 2.8e-11 per draw, so no test
 * reaches it by chance.  This program walks seeds FIRST ... FIRST + COUNT - 1 at counter (J, 0, 0, 0) - pair 0 of generation 0,
 * what a two-member optimiser draws for parameter J in its first generation - and prints one line "seed j k" per hit.
 * tests/golden/es_tail_seeds.json records the hits the tests use.
 *
 * Host only; C99 with OpenMP:
 *     cc -O3 -fopenmp -o es_tail_seeds tools/es_tail_seeds.c
 *     ./es_tail_seeds J FIRST COUNT [K_FAR]
 * About 5e8 seeds per second on eight x86 cores: 1.5e11 seeds, where four hits are expected, take five minutes.  How deep a hit
 * lies is a matter of patience: min(k, 2^52 - 1 - k) is uniform below K_FAR, so a tenth of the hits lie below a tenth of it.
 */
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#define K_FAR_DEFAULT 62545u

/* the first two output words of Philox4x32-10 (Salmon et al. 2011; basilisk_env_amd/csrc/bsk_philox.hpp) */
static inline void philox_w01(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* w0, uint32_t* w1) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    *w0 = c0;
    *w1 = c1;
}

int main(int argc, char** argv) {
    if (argc < 4 || argc > 5) {
        fprintf(stderr, "usage: %s J FIRST COUNT [K_FAR]\n", argv[0]);
        return 2;
    }
    const uint32_t j = (uint32_t)strtoul(argv[1], NULL, 0);
    const uint64_t first = strtoull(argv[2], NULL, 0), count = strtoull(argv[3], NULL, 0);
    const uint32_t k_far = argc > 4 ? (uint32_t)strtoul(argv[4], NULL, 0) : K_FAR_DEFAULT;
    if (k_far >= (1u << 26) || count > UINT64_MAX - first) {
        fprintf(stderr, "K_FAR must be below 2^26 and FIRST + COUNT within 64 bits\n");
        return 2;
    }
    const uint32_t top = (1u << 26) - 1u;
    const int64_t n = (int64_t)count;
#pragma omp parallel for schedule(static)
    for (int64_t s = 0; s < n; ++s) {
        const uint64_t seed = first + (uint64_t)s;
        uint32_t w0, w1;
        philox_w01(j, 0u, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), &w0, &w1);
        const uint32_t hi = w0 >> 6, lo = w1 >> 6;
        if ((hi == 0u && lo <= k_far) || (hi == top && lo >= top - k_far)) {
            const uint64_t k = ((uint64_t)hi << 26) + lo;
#pragma omp critical
            {
                printf("%" PRIu64 " %" PRIu32 " %" PRIu64 "\n", seed, j, k);
                fflush(stdout);
            }
        }
    }
    return 0;
}
