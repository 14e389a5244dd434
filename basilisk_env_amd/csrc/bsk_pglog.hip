// bsk_pglog.hip — a ring of per-iteration rows for the policy-gradient loop, formed on the device (bsk_pg_episodes,
// bsk_pg_log_update, bsk_pg_log_advance; definition in include/bskgpu.h).  Compiled with -ffp-contract=off: every f64 operation is
// rounded on its own, and numpy repeats all of it bit for bit (policy_ref.py: pg_episodes_ref, pg_log_update_ref).
//   pg_episodes_kernel       shaped like adv_partial_kernel (bsk_fit.hip): wave w is the columns 64 w .. 64 w + 63, a lane its env.
//                            The lane carries the return and the length of its env's running episode in from the state arrays,
//                            walks the rows ascending (bsk_pglog.hpp: pg_episode_walk, eight rows of every history in flight, every
//                            load one coalesced row segment) and carries them out again; the wave joins its 19 accumulators in the
//                            trees of bsk_tree.hpp and lane 0 WRITES them.  25 bytes read per sample, nothing written but 16 bytes
//                            per env and 152 per wave.  One env per lane means 1 024 waves at 65 536 envs, about one per SIMD:
//                            latency-bound as gae_kernel is.  Splitting the rows across waves would break the order of an episode.
//   pg_episodes_join_kernel  one workgroup of ten waves, two laps: wave c joins column c of the partial rows and then column c + 10
//                            (19 columns; a workgroup holds at most 16 waves) - adv_join_kernel's rule, lane l the entries
//                            l, l + 64, ... ascending from the first - and one thread forms columns 0 .. 15 of the slot's row.
//   pg_log_update_kernel     one wave: lane c < 8 adds column c of the diagnostics rows ascending from the first, lane 8 the norms
//   pg_log_advance_kernel    one thread
// No atomics, no MFMA; LDS only hands the 19 totals to the thread that forms the row; plain stores.
#include "bsk_pglog.hpp"

#include "bsk_obsstats.hpp"
#include "bsk_tree.hpp"

namespace bsk {

constexpr int PG_JOIN_WAVES = 10;          // ceil(PG_EP_WORDS / 2): two laps cover the 19 columns

__global__ __launch_bounds__(256) void pg_episodes_kernel(const PgEpisodesArgs p, int waves) {
#pragma clang fp contract(off)
    const int w = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));     // (wave-uniform)
    const int lane = (int)(threadIdx.x & 63u);
    if (w >= waves) return;
    const int j = w * 64 + lane;
    PgEpisodeAcc a;
    pg_episode_zero(a);
    if (j < p.n_envs) {                    // a lane at or above n_envs reads nothing and writes nothing
        double R = p.ep_return[j];
        int32_t L = p.ep_len[j];
        pg_episode_walk(p.reward + j, p.reason + j, p.action ? p.action + j : nullptr, p.value ? p.value + j : nullptr,
                        p.value ? p.ret + j : nullptr, p.n_steps, p.stride, R, L, a);
        p.ep_return[j] = R;
        p.ep_len[j] = L;
    }
#pragma unroll
    for (int c = 0; c < PG_EP_SUMS; ++c) a.s[c] = fitness_tree(a.s[c], lane);
    a.mn = extreme_tree<false>(a.mn, lane);
    a.mx = extreme_tree<true>(a.mx, lane);
#pragma unroll
    for (int c = 0; c < PG_EP_COUNTS; ++c) a.n[c] = count_tree(a.n[c], lane);
    if (lane == 0) {
        double* out = p.work + (size_t)PG_EP_WORDS * (size_t)w;
        long long* out_n = (long long*)(out + PG_EP_SUMS + 2);
#pragma unroll
        for (int c = 0; c < PG_EP_SUMS; ++c) out[c] = a.s[c];
        out[PG_EP_SUMS] = a.mn;
        out[PG_EP_SUMS + 1] = a.mx;
#pragma unroll
        for (int c = 0; c < PG_EP_COUNTS; ++c) out_n[c] = a.n[c];
    }
}

__global__ __launch_bounds__(64 * PG_JOIN_WAVES) void pg_episodes_join_kernel(const double* __restrict__ work, int waves, int with_value,
                                                                              double* __restrict__ ring, int capacity,
                                                                              const unsigned long long* __restrict__ counter) {
#pragma clang fp contract(off)
    __shared__ double s_f[PG_EP_SUMS + 2];
    __shared__ long long s_n[PG_EP_COUNTS];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63u);
    for (int c = wave; c < PG_EP_WORDS; c += PG_JOIN_WAVES) {          // (wave-uniform: two laps)
        if (c < PG_EP_SUMS) {
            double s = 0.0;
            for (int w = lane; w < waves; w += 64) {
                const double v = work[(size_t)PG_EP_WORDS * (size_t)w + c];
                s = w == lane ? v : s + v;
            }
            s = fitness_tree(s, lane);
            if (lane == 0) s_f[c] = s;
        } else if (c < PG_EP_SUMS + 2) {
            const bool greatest = c == PG_EP_SUMS + 1;
            double m = __builtin_nan("");
            for (int w = lane; w < waves; w += 64) {
                const double v = work[(size_t)PG_EP_WORDS * (size_t)w + c];
                m = greatest ? extreme_pick<true>(m, v) : extreme_pick<false>(m, v);
            }
            m = greatest ? extreme_tree<true>(m, lane) : extreme_tree<false>(m, lane);
            if (lane == 0) s_f[c] = m;
        } else {
            const long long* cnt = (const long long*)work;
            long long s = 0;
            for (int w = lane; w < waves; w += 64) s += cnt[(size_t)PG_EP_WORDS * (size_t)w + c];
            s = count_tree(s, lane);
            if (lane == 0) s_n[c - PG_EP_SUMS - 2] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* row = ring + (size_t)PG_LOG_COLS * (size_t)(counter ? *counter % (unsigned long long)capacity : 0ull);
        row[0] = (double)s_n[0];
        row[1] = s_f[0];
        row[2] = s_f[1];
        row[3] = s_f[7];
        row[4] = s_f[8];
        row[5] = (double)s_n[1];
#pragma unroll
        for (int c = 0; c < 7; ++c) row[6 + c] = (double)s_n[2 + c];          // the four ends, the three actions
        row[13] = s_f[2];
        double ev = __builtin_nan("");
        if (with_value) {
            const unsigned long long N = (unsigned long long)s_n[9];
            double mean_y, var_y, mean_e, var_e;
            obs_moments(s_f[3], s_f[4], N, mean_y, var_y);
            obs_moments(s_f[5], s_f[6], N, mean_e, var_e);
            if (var_y != 0.0) ev = 1.0 - var_e / var_y;
        }
        row[14] = ev;
        row[15] = s_f[6];
    }
}

__global__ __launch_bounds__(64) void pg_log_update_kernel(const double* __restrict__ diag, int n_rows, const double* __restrict__ norms,
                                                           int n_norms, double* __restrict__ ring, int capacity,
                                                           const unsigned long long* __restrict__ counter) {
#pragma clang fp contract(off)
    double* row = ring + (size_t)PG_LOG_COLS * (size_t)(counter ? *counter % (unsigned long long)capacity : 0ull);
    const int c = (int)threadIdx.x;
    if (c < 8) {
        double s = diag[c];
        for (int r = 1; r < n_rows; ++r) s = s + diag[8 * (size_t)r + c];
        row[16 + c] = s;
    } else if (c == 8) {
        double s = 0.0;
        long long clipped = 0;
        if (norms) {
            s = norms[0];
            clipped = norms[1] < 1.0 ? 1 : 0;
            for (int r = 1; r < n_norms; ++r) {
                s = s + norms[2 * (size_t)r];
                clipped += norms[2 * (size_t)r + 1] < 1.0 ? 1 : 0;
            }
        }
        row[24] = s;
        row[25] = (double)clipped;
    }
}

__global__ void pg_log_advance_kernel(unsigned long long* gen, int capacity, unsigned long long* counter) {
    const unsigned long long c = *counter;
    gen[c % (unsigned long long)capacity] = c;
    *counter = c + 1ull;
}

hipError_t launch_pg_episodes(const PgEpisodesArgs& args, hipStream_t s) {
    const int waves = (args.n_envs + 63) / 64;
    hipLaunchKernelGGL(pg_episodes_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, args, waves);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pg_episodes_join_kernel, dim3(1), dim3(64 * PG_JOIN_WAVES), 0, s, (const double*)args.work, waves, args.value ? 1 : 0,
                       args.ring, args.capacity, args.counter);
    return hipGetLastError();
}

hipError_t launch_pg_log_update(const double* diag, int n_rows, const double* norms, int n_norms, double* ring, int capacity,
                                const unsigned long long* counter, hipStream_t s) {
    hipLaunchKernelGGL(pg_log_update_kernel, dim3(1), dim3(64), 0, s, diag, n_rows, norms, n_norms, ring, capacity, counter);
    return hipGetLastError();
}

hipError_t launch_pg_log_advance(unsigned long long* gen, int capacity, unsigned long long* counter, hipStream_t s) {
    hipLaunchKernelGGL(pg_log_advance_kernel, dim3(1), dim3(1), 0, s, gen, capacity, counter);
    return hipGetLastError();
}

}  // namespace bsk
