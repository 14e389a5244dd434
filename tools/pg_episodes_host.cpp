// pg_episodes_host.cpp — csrc/bsk_pglog.hpp's pg_episode_walk, the per-column walk behind bsk_pg_episodes, compiled for the HOST:
// the walk is plain C++, so its batches of eight rows, its tail and its strided indexing are shown on the CPU - under the address
// and undefined-behaviour sanitizers - before a GPU runs them (tests/test_pg_log_host.py compares the output with
// policy_ref.pg_episodes_walk_ref, bit for bit).
//   c++ -O1 -std=c++17 -ffp-contract=off [-fsanitize=address,undefined] -DBSK_PGLOG_HOST -I basilisk_env_amd/csrc
//       tools/pg_episodes_host.cpp -o pg_episodes_host
//   pg_episodes_host n_steps n_envs stride with_action with_value < input      -> one line per column
// Input, whitespace-separated, floating-point numbers as the hexadecimal of their bits: per env `ep_return ep_len`, then per row and
// env `reward reason action value ret` (action, value and ret are read and dropped when switched off).  The histories are allocated
// as [n_steps - 1][stride] + [n_envs] elements exactly, so that a read past the last column of the last row is a sanitizer error.
// Output per column: the 7 sums, mn, mx (hexadecimal bits), the 10 counts, the new ep_return (bits) and ep_len.
#ifndef BSK_PGLOG_HOST
#define BSK_PGLOG_HOST 1
#endif
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bsk_pglog.hpp"

static double f64_of(uint64_t b) { double x; std::memcpy(&x, &b, 8); return x; }
static float f32_of(uint32_t b) { float x; std::memcpy(&x, &b, 4); return x; }
static uint64_t bits_of(double x) { uint64_t b; std::memcpy(&b, &x, 8); return b; }

int main(int argc, char** argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s n_steps n_envs stride with_action with_value < input\n", argv[0]);
        return 2;
    }
    const int T = std::atoi(argv[1]), N = std::atoi(argv[2]);
    const long long stride = std::atoll(argv[3]);
    const bool with_action = std::atoi(argv[4]) != 0, with_value = std::atoi(argv[5]) != 0;
    if (T < 1 || N < 1 || stride < N) {
        std::fprintf(stderr, "n_steps and n_envs must be >= 1, stride >= n_envs\n");
        return 2;
    }
    const size_t cells = (size_t)(T - 1) * (size_t)stride + (size_t)N;
    std::vector<double> reward(cells), ret(cells), R(N);
    std::vector<uint8_t> reason(cells);
    std::vector<int32_t> action(cells), L(N);
    std::vector<float> value(cells);
    for (int j = 0; j < N; ++j) {
        uint64_t r;
        int32_t l;
        if (std::scanf("%" SCNx64 " %" SCNd32, &r, &l) != 2) return 3;
        R[j] = f64_of(r);
        L[j] = l;
    }
    for (int t = 0; t < T; ++t)
        for (int j = 0; j < N; ++j) {
            uint64_t r, y;
            uint32_t v;
            unsigned why;
            int32_t a;
            if (std::scanf("%" SCNx64 " %u %" SCNd32 " %" SCNx32 " %" SCNx64, &r, &why, &a, &v, &y) != 5) return 3;
            const size_t at = (size_t)t * (size_t)stride + (size_t)j;
            reward[at] = f64_of(r);
            reason[at] = (uint8_t)why;
            action[at] = a;
            value[at] = f32_of(v);
            ret[at] = f64_of(y);
        }
    for (int j = 0; j < N; ++j) {
        bsk::PgEpisodeAcc a;
        bsk::pg_episode_zero(a);
        bsk::pg_episode_walk(reward.data() + j, reason.data() + j, with_action ? action.data() + j : nullptr,
                             with_value ? value.data() + j : nullptr, with_value ? ret.data() + j : nullptr, T, (int64_t)stride, R[j], L[j], a);
        for (int c = 0; c < bsk::PG_EP_SUMS; ++c) std::printf("%016" PRIx64 " ", bits_of(a.s[c]));
        std::printf("%016" PRIx64 " %016" PRIx64, bits_of(a.mn), bits_of(a.mx));
        for (int c = 0; c < bsk::PG_EP_COUNTS; ++c) std::printf(" %lld", a.n[c]);
        std::printf(" %016" PRIx64 " %" PRId32 "\n", bits_of(R[j]), L[j]);
    }
    return 0;
}
