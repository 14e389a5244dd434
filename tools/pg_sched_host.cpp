// pg_sched_host.cpp — csrc/bsk_pgsched.hpp's pg_sched_value, pg_kl_gate_sums and pg_kl_gate_apply - the rule behind
// bsk_fit_schedule_begin and the walk and decision behind bsk_fit_kl_gate - compiled for the HOST: they are plain C++, so the exact
// branches of the rule, the order of the gate's two sums and its comparison are shown on the CPU - under the address and
// undefined-behaviour sanitizers - before a GPU runs them (tests/test_pg_sched_host.py compares the output with
// policy_ref.pg_schedule_ref and fit_kl_gate_ref, bit for bit).
//   c++ -O1 -std=c++17 -ffp-contract=off [-fsanitize=address,undefined] -DBSK_PGSCHED_HOST -I basilisk_env_amd/csrc
//       tools/pg_sched_host.cpp -o pg_sched_host
//   pg_sched_host < input      -> one line per record
// Input, whitespace-separated records, floating-point numbers as the hexadecimal of their bits, integers in decimal:
//   v it total a b                                  -> the value (bits)
//   g kl_stop gate skipped kl_at n_rows  rows...    -> gate skipped kl_at (bits) closed S (bits) N (bits)
// where rows are n_rows * 8 numbers.  The rows are allocated as exactly that many, so that a read past the last is a sanitizer error.
#ifndef BSK_PGSCHED_HOST
#define BSK_PGSCHED_HOST 1
#endif
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bsk_pgsched.hpp"

static double f64_of(uint64_t b) { double x; std::memcpy(&x, &b, 8); return x; }
static uint64_t bits_of(double x) { uint64_t b; std::memcpy(&b, &x, 8); return b; }

int main() {
    char kind[4];
    while (std::scanf("%3s", kind) == 1) {
        if (kind[0] == 'v') {
            uint64_t it, total, a, b;
            if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNx64 " %" SCNx64, &it, &total, &a, &b) != 4) return 3;
            std::printf("%016" PRIx64 "\n", bits_of(bsk::pg_sched_value(it, total, f64_of(a), f64_of(b))));
        } else if (kind[0] == 'g') {
            uint64_t stop, gate, skipped, at;
            int n_rows;
            if (std::scanf("%" SCNx64 " %" SCNu64 " %" SCNu64 " %" SCNx64 " %d", &stop, &gate, &skipped, &at, &n_rows) != 5 || n_rows < 1) return 3;
            std::vector<double> rows((size_t)n_rows * bsk::PG_SCHED_DIAG_COLS);
            for (double& x : rows) {
                uint64_t b;
                if (std::scanf("%" SCNx64, &b) != 1) return 3;
                x = f64_of(b);
            }
            double S, N, kl_at = f64_of(at);
            unsigned long long g = gate, k = skipped;
            bsk::pg_kl_gate_sums(rows.data(), n_rows, S, N);
            const bool closed = bsk::pg_kl_gate_apply(S, N, f64_of(stop), g, k, kl_at);
            std::printf("%llu %llu %016" PRIx64 " %d %016" PRIx64 " %016" PRIx64 "\n", g, k, bits_of(kl_at), closed ? 1 : 0, bits_of(S), bits_of(N));
        } else {
            std::fprintf(stderr, "unknown record %s\n", kind);
            return 2;
        }
    }
    return 0;
}
