// bsk_es.hip — an antithetic evolution strategy with centred-rank utilities, on the device (bsk_es_*; definition in
// include/bskgpu.h):
//   es_ask_kernel      theta +- sigma * z straight into a population's device layout, z regenerated from a counter
//   es_rank_kernel     one thread per member: how many members beat it -> the utility difference of every pair
//   es_tell_kernel     one wave per parameter: the utilities contracted with the regenerated noise in a fixed order
//   es_tell_adam_kernel     the same contraction driven through Adam with an L2 penalty
//   es_advance_kernel  the generation counter += 1 (es_advance_adam_kernel: and Adam's two running powers)
//   es_ask_sigma_kernel, es_rank_q_kernel, es_tell_sigma_kernel, es_tell_adam_sigma_kernel     the same four under
//                      BSK_ES_SIGMA_PGPE: a step size per parameter in device memory, moved by lane 0 behind a second sum
//   es_log_kernel, es_best_kernel     bsk_es_set_log: one wave for the generation's row and the champion rule, then one thread per
//                      parameter for the champion's floats - in front of the update, from what ask read
//   es_outcome_kernel  bsk_es_set_outcome_log: one wave for the generation's row of episode outcomes - in front of the update too
//   es_center_kernel, es_validate_kernel, es_val_best_kernel     bsk_es_set_validation: the centre into the V members behind
//                      ask's, then one thread for the centre's row and the validated champion's rule and one thread per parameter
//                      for its floats - in front of the update too
// The noise is never stored: z(g, i, j) is one Philox4x32-10 call and an inverse normal CDF made of f64 + - * /, sqrt and integer
// operations.  Compiled with -ffp-contract=off (Makefile), as bsk_population.hip is: every operation rounds on its own, and numpy
// repeats all of it bit for bit (policy_ref.py: es_noise_ref, es_ask_ref, es_tell_ref, es_tell_adam_ref, es_ask_sigma_ref,
// es_tell_pgpe_ref).
#include "bsk_es.hpp"

#include "../../include/bskgpu.h"
#include "bsk_philox.hpp"
#include "bsk_tree.hpp"

namespace bsk {

// c0 + c1 x + ... + c7 x^7, Horner from the highest coefficient
__device__ __forceinline__ double es_poly7(double x, double c0, double c1, double c2, double c3, double c4, double c5, double c6,
                                           double c7) {
#pragma clang fp contract(off)
    double y = c7;
    y = y * x + c6;
    y = y * x + c5;
    y = y * x + c4;
    y = y * x + c3;
    y = y * x + c2;
    y = y * x + c1;
    y = y * x + c0;
    return y;
}

// ln(p) for a positive normal p: p = m * 2^e with m in [sqrt(1/2), sqrt(2)), ln(m) = 2 atanh(s) with s = (m - 1) / (m + 1) as its
// series to s^23 (|s| < 0.1716: the first term left out is below 2^-64 of the sum)
__device__ __forceinline__ double es_log(double p) {
#pragma clang fp contract(off)
    const long long bits = __double_as_longlong(p);
    int e = (int)((bits >> 52) & 0x7ff) - 1022;
    double m = __longlong_as_double((bits & 0x000fffffffffffffll) | 0x3fe0000000000000ll);     // [0.5, 1): frexp
    if (m < 0.7071067811865476) { m = m + m; e -= 1; }
    const double s = (m - 1.0) / (m + 1.0), s2 = s * s;
    double t = 1.0 / 23.0;
#pragma unroll
    for (int k = 10; k >= 0; --k) t = t * s2 + 1.0 / (double)(2 * k + 1);
    return (double)e * 0.6931471805599453 + (2.0 * s) * t;
}

// The inverse normal CDF of u in (0, 1): Wichura's AS 241 (PPND16) with the logarithm above
__device__ __forceinline__ double es_inverse_normal(double u) {
#pragma clang fp contract(off)
    const double q = u - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        return q * es_poly7(r, 3.3871328727963666080, 1.3314166789178437745e2, 1.9715909503065514427e3, 1.3731693765509461125e4,
                            4.5921953931549871457e4, 6.7265770927008700853e4, 3.3430575583588128105e4, 2.5090809287301226727e3) /
               es_poly7(r, 1.0, 4.2313330701600911252e1, 6.8718700749205790830e2, 5.3941960214247511077e3, 2.1213794301586595867e4,
                        3.9307895800092710610e4, 2.8729085735721942674e4, 5.2264952788528545610e3);
    }
    const double p = q < 0.0 ? u : 1.0 - u;
    const double r = sqrt(-es_log(p));
    double z;
    if (r <= 5.0) {
        const double x = r - 1.6;
        z = es_poly7(x, 1.42343711074968357734, 4.63033784615654529590, 5.76949722146069140550, 3.64784832476320460504,
                     1.27045825245236838258, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4) /
            es_poly7(x, 1.0, 2.05319162663775882187, 1.67638483018380384940, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
                     1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9);
    } else {
        const double x = r - 5.0;
        z = es_poly7(x, 6.65790464350110377720, 5.46378491116411436990, 1.78482653991729133580, 2.96560571828504891230e-1,
                     2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7) /
            es_poly7(x, 1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2, 7.86869131145613259100e-4,
                     1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15);
    }
    return q < 0.0 ? -z : z;
}

// z(g, i, j): key (seed), counter (j, i, g); 52 bits of the first two words -> u = (k + 0.5) * 2^-52, exact and inside (0, 1)
__device__ __forceinline__ double es_noise(unsigned long long seed, unsigned long long g, unsigned i, unsigned j) {
    unsigned w[4];
    philox4x32_10(j, i, (unsigned)g, (unsigned)(g >> 32), (unsigned)seed, (unsigned)(seed >> 32), w);
    const unsigned long long k = ((unsigned long long)(w[0] >> 6) << 26) + (unsigned long long)(w[1] >> 6);
    return es_inverse_normal(((double)k + 0.5) * 0x1p-52);
}

// The two floats of parameter j in pair `pair` (include/bskgpu.h, ask): theta_j +- s_j * z(g, pair, j), s_j the one sigma or
// sigma_vec[j]; (float)theta_j for a frozen j.  ONE text behind ask and the champion of the training log (es_best_kernel), so
// that the two cannot diverge.  A macro and not a device function for the reason ES_PAIR_SUM gives: behind a call es_ask_kernel
// came out with other registers and another order of its two stores, and it keeps the instruction stream it had.
#define ES_PAIR_VALUES(es, sigma_vec, pair, j, plus, minus)                                                                     \
    {                                                                                                                           \
        const double t = es.theta[j];                                                                                           \
        if (j < es.frozen) {                                                                                                    \
            plus = minus = (float)t;                                                                                            \
        } else {                                                                                                                \
            const double step = (sigma_vec ? sigma_vec[j] : es.sigma) * es_noise(es.state[0], es.state[1], pair, (unsigned)j);  \
            plus = (float)(t + step);                                                                                           \
            minus = (float)(t - step);                                                                                          \
        }                                                                                                                       \
    }

// Pair blockIdx.x, float d of the device layout: policy_pack_kernel's gather with theta +- sigma * z in place of a source block.
// Both members of the pair from ONE evaluation of z; every float of both device blocks is written by exactly one thread.
// sigma_vec == nullptr (a constant where es_ask_kernel inlines this): the optimiser's one sigma; otherwise sigma_vec[j].
__device__ __forceinline__ void es_ask_pair(const EsArgs& es, const double* __restrict__ sigma_vec, float* __restrict__ dst,
                                            const PolicyPackMap& map) {
#pragma clang fp contract(off)
    const int d = (int)(blockIdx.y * blockDim.x + threadIdx.x);
    if (d >= map.n_device) return;
    const int j = policy_pack_source(map, d);
    float plus = 0.0f, minus = 0.0f;
    if (j >= 0) ES_PAIR_VALUES(es, sigma_vec, blockIdx.x, j, plus, minus)
    float* at = dst + (size_t)(2u * blockIdx.x) * (size_t)map.n_device + d;
    at[0] = plus;
    at[map.n_device] = minus;
}

__global__ __launch_bounds__(256) void es_ask_kernel(const EsArgs es, float* __restrict__ dst, const PolicyPackMap map) {
    es_ask_pair(es, nullptr, dst, map);
}

// BSK_ES_SIGMA_PGPE: one more f64 load, sigma_vec[j], beside theta[j] (frozen entries are never read)
__global__ __launch_bounds__(256) void es_ask_sigma_kernel(const EsArgs es, const double* __restrict__ sigma_vec, float* __restrict__ dst,
                                                           const PolicyPackMap map) {
    es_ask_pair(es, sigma_vec, dst, map);
}

// a (index ia) comes before b (index ib): bsk_fork.hip's beats() - the greater value, a NaN below every number, ties to the lower index
__device__ __forceinline__ bool es_beats(double a, int ia, double b, int ib) {
    const bool na = a != a, nb = b != b;
    if (na != nb) return nb;
    if (!na && a != b) return a > b;
    return ia < ib;
}

// Thread k counts the members that beat member k, the fitness staged through LDS 256 values at a time (every thread of the
// workgroup reads the same word: a broadcast); u_k = 0.5 - rank_k / max(P - 1, 1); the even thread of a pair writes u_2i - u_2i+1.
__global__ __launch_bounds__(256) void es_rank_kernel(const double* __restrict__ fitness, int P, double* __restrict__ w) {
#pragma clang fp contract(off)
    __shared__ double tile[256];
    const int k = (int)(blockIdx.x * 256u + threadIdx.x);
    const bool live = k < P;
    const double f = live ? fitness[k] : 0.0;
    int rank = 0;
    for (int base = 0; base < P; base += 256) {
        const int m = base + (int)threadIdx.x;
        __syncthreads();                   // (the previous tile's last reads)
        tile[threadIdx.x] = m < P ? fitness[m] : 0.0;
        __syncthreads();
        const int count = P - base < 256 ? P - base : 256;
        if (live)
            for (int t = 0; t < count; ++t) rank += es_beats(tile[t], base + t, f, k) ? 1 : 0;
    }
    const double u = 0.5 - (double)rank / (double)(P - 1 > 1 ? P - 1 : 1);
    const double odd = __shfl_down(u, 1, 64);       // (P is even: members 2i and 2i + 1 are neighbours in one wave)
    if (live && (k & 1) == 0) w[k >> 1] = u - odd;
}

// BSK_ES_SIGMA_PGPE: the same ranking, the even thread also writing q_i = u_2i + u_2i+1 - what the pair says about the step SIZE.
// The text a second time and not one body behind both: inlined from a shared function es_rank_kernel came out with other scalar
// instructions around its inner loop (as the comment on ES_PAIR_SUM reports of the update kernels), and it keeps the ones it had.
__global__ __launch_bounds__(256) void es_rank_q_kernel(const double* __restrict__ fitness, int P, double* __restrict__ w,
                                                        double* __restrict__ q) {
#pragma clang fp contract(off)
    __shared__ double tile[256];
    const int k = (int)(blockIdx.x * 256u + threadIdx.x);
    const bool live = k < P;
    const double f = live ? fitness[k] : 0.0;
    int rank = 0;
    for (int base = 0; base < P; base += 256) {
        const int m = base + (int)threadIdx.x;
        __syncthreads();                   // (the previous tile's last reads)
        tile[threadIdx.x] = m < P ? fitness[m] : 0.0;
        __syncthreads();
        const int count = P - base < 256 ? P - base : 256;
        if (live)
            for (int t = 0; t < count; ++t) rank += es_beats(tile[t], base + t, f, k) ? 1 : 0;
    }
    const double u = 0.5 - (double)rank / (double)(P - 1 > 1 ? P - 1 : 1);
    const double odd = __shfl_down(u, 1, 64);
    if (live && (k & 1) == 0) {
        w[k >> 1] = u - odd;
        q[k >> 1] = u + odd;
    }
}

// the fitness tree (bsk_population.hip): s[l] = s[l] + s[l + stride] for l < stride, stride = 32 ... 1
__device__ __forceinline__ double es_tree(double s, int lane) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(s, off, 64);
        if (lane < off) s = s + o;
    }
    return s;
}

// s[0] of parameter j (include/bskgpu.h, tell step 3), valid in lane 0: lane l adds w_i * z(g, i, j) over its pairs i = l, l + 64,
// ... ascending, starting FROM the first (+0.0 with no pair at all); the lanes join in the tree.  ONE text behind both update
// kernels, so that the order of the sum cannot diverge between them.  It is a macro and not a device function because
// es_tell_kernel keeps the instruction stream it had: behind a call - the structure by reference, its fields by value, the whole
// wave as a template - the same loop came out with another schedule of the Philox key's scalar instructions, every time.
#define ES_PAIR_SUM(es, w, j, lane, s)                                                \
    const unsigned long long seed = es.state[0], g = es.state[1];                     \
    double s = 0.0;                                                                   \
    for (int i = lane; i < es.pairs; i += 64) {                                       \
        const double t = w[i] * es_noise(seed, g, (unsigned)i, (unsigned)j);          \
        s = i == lane ? t : s + t;                                                    \
    }                                                                                 \
    s = es_tree(s, lane)

// One wave per parameter j >= frozen: the sum above, then lane 0 moves theta_j.  No atomics, no dependence on the launch shape.
__global__ __launch_bounds__(256) void es_tell_kernel(const EsArgs es, int n_params, const double* __restrict__ w, double c) {
#pragma clang fp contract(off)
    const int j = es.frozen + (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));     // (wave-uniform)
    const int lane = (int)(threadIdx.x & 63u);
    if (j >= n_params) return;
    ES_PAIR_SUM(es, w, j, lane, s);
    if (lane == 0) es.theta[j] = es.theta[j] + c * s;
}

// The same wave per parameter with Adam and an L2 penalty behind the sum (include/bskgpu.h: every operation on its own, plain /
// and sqrt).  beta_pow is read here and moved on by es_advance_adam_kernel behind this launch, never by this kernel.
__global__ __launch_bounds__(256) void es_tell_adam_kernel(const EsArgs es, int n_params, const double* __restrict__ w, const EsAdam ad) {
#pragma clang fp contract(off)
    const int j = es.frozen + (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));     // (wave-uniform)
    const int lane = (int)(threadIdx.x & 63u);
    if (j >= n_params) return;
    ES_PAIR_SUM(es, w, j, lane, s);
    if (lane == 0) {
        const double t = es.theta[j];
        es.theta[j] = t + adam_step(ad, j, ad.cg * s - ad.weight_decay * t);
    }
}

// BSK_ES_SIGMA_PGPE (include/bskgpu.h): ES_PAIR_SUM with a second accumulator in the same loop, r over q_i * (z * z - 1.0) from the
// SAME evaluation of z, and a second tree.  Its own text, so that the fixed-sigma kernels above keep theirs (the comment on
// ES_PAIR_SUM); the order of s is that macro's, term by term.
#define ES_PAIR_SUM_SIGMA(es, w, q, j, lane, s, r)                                    \
    const unsigned long long seed = es.state[0], g = es.state[1];                     \
    double s = 0.0, r = 0.0;                                                          \
    for (int i = lane; i < es.pairs; i += 64) {                                       \
        const double z = es_noise(seed, g, (unsigned)i, (unsigned)j);                 \
        const double t = w[i] * z;                                                    \
        const double t2 = q[i] * (z * z - 1.0);                                       \
        s = i == lane ? t : s + t;                                                    \
        r = i == lane ? t2 : r + t2;                                                  \
    }                                                                                 \
    s = es_tree(s, lane);                                                             \
    r = es_tree(r, lane)

// lane 0: sigma_vec[j] out of r[0] and sg, the value it had before this tell - a relative change of at most max_change, then the bounds
__device__ __forceinline__ void es_sigma_step(const EsSigma& sv, int j, double sg, double r) {
#pragma clang fp contract(off)
    double d = (sv.cs * r) * sg;
    const double lim = sv.max_change * sg;
    d = d > lim ? lim : (d < -lim ? -lim : d);
    double n = sg + d;
    n = n < sv.sigma_min ? sv.sigma_min : n;
    n = n > sv.sigma_max ? sv.sigma_max : n;
    sv.sigma_vec[j] = n;
}

__global__ __launch_bounds__(256) void es_tell_sigma_kernel(const EsArgs es, int n_params, const double* __restrict__ w,
                                                            const double* __restrict__ q, double lr, const EsSigma sv) {
#pragma clang fp contract(off)
    const int j = es.frozen + (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));     // (wave-uniform)
    const int lane = (int)(threadIdx.x & 63u);
    if (j >= n_params) return;
    ES_PAIR_SUM_SIGMA(es, w, q, j, lane, s, r);
    if (lane == 0) {
        const double sg = sv.sigma_vec[j];
        es.theta[j] = es.theta[j] + (lr / (sv.pd * sg)) * s;
        es_sigma_step(sv, j, sg, r);
    }
}

__global__ __launch_bounds__(256) void es_tell_adam_sigma_kernel(const EsArgs es, int n_params, const double* __restrict__ w,
                                                                 const double* __restrict__ q, const EsAdam ad, const EsSigma sv) {
#pragma clang fp contract(off)
    const int j = es.frozen + (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));     // (wave-uniform)
    const int lane = (int)(threadIdx.x & 63u);
    if (j >= n_params) return;
    ES_PAIR_SUM_SIGMA(es, w, q, j, lane, s, r);
    if (lane == 0) {
        const double sg = sv.sigma_vec[j];
        const double cg = 1.0 / (sv.pd * sg);                                                  // (ad.cg is the fixed mode's)
        const double t = es.theta[j];
        es.theta[j] = t + adam_step(ad, j, cg * s - ad.weight_decay * t);
        es_sigma_step(sv, j, sg, r);
    }
}

__global__ void es_advance_kernel(unsigned long long* state) { state[1] += 1ull; }

__global__ void es_advance_adam_kernel(unsigned long long* state, double* beta_pow, double beta1, double beta2) {
#pragma clang fp contract(off)
    beta_pow[0] = beta_pow[0] * beta1;
    beta_pow[1] = beta_pow[1] * beta2;
    state[1] += 1ull;
}

// The training log (include/bskgpu.h, bsk_es_set_log): ONE wave in front of the update.  Lane l walks members l, l + 64, ...
// ascending: its running best and worst under es_beats (the worst among the non-NaN members only), the sums of x, x * x and
// mean_len in the library's one order (from the first element, +0.0 with none), the number of non-NaN members.  The lanes join with
// __shfl_down: best and worst under the same predicate - es_beats with its index tiebreak is a strict total order, so the join's
// order does not matter - the sums in the fitness tree.  Lane 0 writes row g mod capacity and applies the champion rule; the
// candidate words {take, b} are for es_best_kernel behind this launch.  (__shfl_down past the wave's end returns the lane's own
// value: a member never beats itself, and a lane at or above the stride adds nothing.)
__global__ __launch_bounds__(64) void es_log_kernel(const unsigned long long* __restrict__ state, const double* __restrict__ fitness, int P,
                                                    const EsLog lg) {
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x;
    double bf = 0.0, wf = 0.0;
    int bi = -1, wi = -1, cnt = 0;
    double s1 = 0.0, s2 = 0.0, l1 = 0.0;
    for (int k = lane; k < P; k += 64) {
        const double f = fitness[k];
        const bool isn = f != f;
        const double x = isn ? 0.0 : f;
        const double q = x * x;
        s1 = k == lane ? x : s1 + x;
        s2 = k == lane ? q : s2 + q;
        if (lg.mean_len) {
            const double m = lg.mean_len[k];
            l1 = k == lane ? m : l1 + m;
        }
        cnt += isn ? 0 : 1;
        if (bi < 0 || es_beats(f, k, bf, bi)) { bf = f; bi = k; }
        if (!isn && (wi < 0 || es_beats(wf, wi, f, k))) { wf = f; wi = k; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double obf = __shfl_down(bf, off, 64), owf = __shfl_down(wf, off, 64);
        const int obi = __shfl_down(bi, off, 64), owi = __shfl_down(wi, off, 64), ocnt = __shfl_down(cnt, off, 64);
        if (obi >= 0 && (bi < 0 || es_beats(obf, obi, bf, bi))) { bf = obf; bi = obi; }
        if (owi >= 0 && (wi < 0 || es_beats(wf, wi, owf, owi))) { wf = owf; wi = owi; }
        if (lane < off) cnt += ocnt;
    }
    s1 = fitness_tree(s1, lane);
    s2 = fitness_tree(s2, lane);
    l1 = fitness_tree(l1, lane);
    if (lane != 0) return;
    const unsigned long long g = state[1];
    const unsigned long long slot = g % (unsigned long long)lg.capacity;
    double* row = lg.row + 8 * slot;
    row[0] = bf;
    row[1] = wi >= 0 ? wf : __longlong_as_double(0x7ff8000000000000ll);
    row[2] = s1;
    row[3] = s2;
    row[4] = (double)cnt;
    row[5] = (double)bi;
    row[6] = l1;
    row[7] = lg.mean_len ? lg.mean_len[bi] : 0.0;
    lg.gen[slot] = g;
    const double champion = *lg.best_fitness;
    const bool take = bf == bf && (champion != champion || bf > champion);
    if (take) {
        *lg.best_fitness = bf;
        *lg.best_generation = g;
        lg.best_member[0] = bi;
    }
    lg.cand[0] = take ? 1 : 0;
    lg.cand[1] = bi;
}

// One thread per parameter j, behind es_log_kernel on the same stream (the kernel boundary orders the candidate words: no atomics,
// no fence) and in front of the update: while `take`, best_params[j] = the float ask writes for member b of this generation -
// ES_PAIR_VALUES, the text of es_ask_pair, with theta, sigma_vec and the generation word as ask read them.
__global__ __launch_bounds__(256) void es_best_kernel(const EsArgs es, const double* __restrict__ sigma_vec, int n_params, const EsLog lg) {
#pragma clang fp contract(off)
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    if (j >= n_params || lg.cand[0] == 0) return;
    const int b = lg.cand[1];
    float plus, minus;
    ES_PAIR_VALUES(es, sigma_vec, (unsigned)(b >> 1), j, plus, minus)
    lg.best_params[j] = (b & 1) ? minus : plus;
}

hipError_t launch_es_log(const EsArgs& es, const double* sigma_vec, int n_params, const double* fitness, const EsLog& lg, hipStream_t s) {
    hipLaunchKernelGGL(es_log_kernel, dim3(1), dim3(64), 0, s, es.state, fitness, 2 * es.pairs, lg);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(es_best_kernel, dim3((unsigned)((n_params + 255) / 256)), dim3(256), 0, s, es, sigma_vec, n_params, lg);
    return hipGetLastError();
}

// One block of the outcome row (include/bskgpu.h, bsk_es_set_outcome_log): the totals over the `count` member rows from R on.  Lane l
// walks rows l, l + 64, ... ascending: the eight counts as integers, column 8 in the library's one order (from the first element,
// +0.0 with none), columns 9 and 10 under extreme_pick from the NaN that stands for "no member".  With count == 0 (validation off;
// wave-uniform) every entry is +0.0.
__device__ __forceinline__ void es_outcome_totals(const double* __restrict__ R, int count, int lane, double* __restrict__ dst) {
#pragma clang fp contract(off)
    if (count < 1) {
        if (lane < BSK_OUTCOME_COLS) dst[lane] = 0.0;
        return;
    }
    long long cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double sq = 0.0, lo = __longlong_as_double(0x7ff8000000000000ll), hi = lo;
    for (int k = lane; k < count; k += 64) {
        const double* r = R + (size_t)k * BSK_OUTCOME_COLS;
#pragma unroll
        for (int c = 0; c < 8; ++c) cnt[c] += (long long)r[c];
        sq = k == lane ? r[8] : sq + r[8];
        lo = extreme_pick<false>(lo, r[9]);
        hi = extreme_pick<true>(hi, r[10]);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) cnt[c] = count_tree(cnt[c], lane);
    sq = fitness_tree(sq, lane);
    lo = extreme_tree<false>(lo, lane);
    hi = extreme_tree<true>(hi, lane);
    if (lane != 0) return;
#pragma unroll
    for (int c = 0; c < 8; ++c) dst[c] = (double)cnt[c];
    dst[8] = sq;
    dst[9] = lo;
    dst[10] = hi;
}

// The outcome ring: ONE wave in front of the update.  Block A the totals over the P ranked members, block B the row of the member
// nobody beats under es_beats - found here from the fitness, as es_log_kernel finds it, and not read from the log's candidate words:
// the two records do not know each other - block C the totals over the V validation members.  It writes row g mod capacity of its
// own ring and nothing else.
__global__ __launch_bounds__(64) void es_outcome_kernel(const unsigned long long* __restrict__ state, const double* __restrict__ fitness,
                                                        int P, const EsOutcome oc) {
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x;
    const unsigned long long g = state[1];
    const unsigned long long slot = g % (unsigned long long)oc.capacity;
    double* row = oc.row + (size_t)(3 * BSK_OUTCOME_COLS) * slot;
    es_outcome_totals(oc.rows, P, lane, row);
    es_outcome_totals(oc.rows + (size_t)P * BSK_OUTCOME_COLS, oc.n_val, lane, row + 2 * BSK_OUTCOME_COLS);
    double bf = 0.0;
    int bi = -1;
    for (int k = lane; k < P; k += 64) {
        const double f = fitness[k];
        if (bi < 0 || es_beats(f, k, bf, bi)) { bf = f; bi = k; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double obf = __shfl_down(bf, off, 64);
        const int obi = __shfl_down(bi, off, 64);
        if (obi >= 0 && (bi < 0 || es_beats(obf, obi, bf, bi))) { bf = obf; bi = obi; }
    }
    const int b = __shfl(bi, 0, 64);
    if (lane < BSK_OUTCOME_COLS) row[BSK_OUTCOME_COLS + lane] = oc.rows[(size_t)b * BSK_OUTCOME_COLS + lane];
    if (lane == 0) oc.gen[slot] = g;
}

hipError_t launch_es_outcome(const EsArgs& es, const double* fitness, const EsOutcome& oc, hipStream_t s) {
    hipLaunchKernelGGL(es_outcome_kernel, dim3(1), dim3(64), 0, s, es.state, fitness, 2 * es.pairs, oc);
    return hipGetLastError();
}

// Validation on fixed episodes (include/bskgpu.h, bsk_es_set_validation).  Validation member blockIdx.x, float d of its device
// block: ask's gather (policy_pack_source) with the plain (float)theta_j in place of theta +- sigma * z - for every j, frozen or
// not, and with no sum in between, so that a -0.0 in theta stays -0.0; the padding is zero.  dst is the block of member P: every
// float of the V blocks is written by exactly one thread.
__global__ __launch_bounds__(256) void es_center_kernel(const double* __restrict__ theta, float* __restrict__ dst, const PolicyPackMap map) {
#pragma clang fp contract(off)
    const int d = (int)(blockIdx.y * blockDim.x + threadIdx.x);
    if (d >= map.n_device) return;
    const int j = policy_pack_source(map, d);
    dst[(size_t)blockIdx.x * (size_t)map.n_device + d] = j >= 0 ? (float)theta[j] : 0.0f;
}

// ONE thread, in front of the update and behind the log's two launches: the centre's score f_c = (f[P] + f[P + 1] + ...) / V, the
// sum ascending from the first value, and L_c the same over mean_len; row g mod capacity; the champion rule of es_log_kernel on
// f_c.  The candidate word is for es_val_best_kernel behind this launch.
__global__ void es_validate_kernel(const unsigned long long* __restrict__ state, const double* __restrict__ fitness, int P, const EsVal vl) {
#pragma clang fp contract(off)
    const unsigned long long g = state[1];
    const unsigned long long slot = g % (unsigned long long)vl.capacity;
    double s = fitness[P], l = vl.mean_len ? vl.mean_len[P] : 0.0;
    for (int v = 1; v < vl.n_val; ++v) {
        s = s + fitness[P + v];
        if (vl.mean_len) l = l + vl.mean_len[P + v];
    }
    const double fc = s / (double)vl.n_val;
    const double lc = vl.mean_len ? l / (double)vl.n_val : 0.0;
    const double champion = *vl.best_fitness;
    const bool take = fc == fc && (champion != champion || fc > champion);
    if (take) {
        *vl.best_fitness = fc;
        *vl.best_generation = g;
    }
    double* row = vl.row + 4 * slot;
    row[0] = fc;
    row[1] = lc;
    row[2] = take ? 1.0 : 0.0;
    row[3] = (double)vl.n_val;
    vl.gen[slot] = g;
    vl.cand[0] = take ? 1 : 0;
}

// One thread per parameter j, behind es_validate_kernel on the same stream (the kernel boundary orders the candidate word: no
// atomics, no fence) and in front of the update: while `take`, val_best_params[j] = (float)theta_j - the float es_center_kernel wrote.
__global__ __launch_bounds__(256) void es_val_best_kernel(const double* __restrict__ theta, int n_params, const EsVal vl) {
#pragma clang fp contract(off)
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    if (j >= n_params || vl.cand[0] == 0) return;
    vl.best_params[j] = (float)theta[j];
}

hipError_t launch_es_center(const PolicyLayout& lay, const double* theta, float* d_block, int n_val, hipStream_t s) {
    const PolicyPackMap map = policy_pack_map(lay);
    hipLaunchKernelGGL(es_center_kernel, dim3((unsigned)n_val, (unsigned)((lay.n_device + 255) / 256)), dim3(256), 0, s, theta, d_block, map);
    return hipGetLastError();
}

hipError_t launch_es_validate(const EsArgs& es, int n_params, const double* fitness, const EsVal& vl, hipStream_t s) {
    hipLaunchKernelGGL(es_validate_kernel, dim3(1), dim3(1), 0, s, es.state, fitness, 2 * es.pairs, vl);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(es_val_best_kernel, dim3((unsigned)((n_params + 255) / 256)), dim3(256), 0, s, es.theta, n_params, vl);
    return hipGetLastError();
}

hipError_t launch_es_ask(const PolicyLayout& lay, const EsArgs& es, float* d_params, hipStream_t s) {
    const PolicyPackMap map = policy_pack_map(lay);
    hipLaunchKernelGGL(es_ask_kernel, dim3((unsigned)es.pairs, (unsigned)((lay.n_device + 255) / 256)), dim3(256), 0, s, es, d_params, map);
    return hipGetLastError();
}

hipError_t launch_es_rank(const double* fitness, int n_members, double* w, hipStream_t s) {
    hipLaunchKernelGGL(es_rank_kernel, dim3((unsigned)((n_members + 255) / 256)), dim3(256), 0, s, fitness, n_members, w);
    return hipGetLastError();
}

hipError_t launch_es_tell(const EsArgs& es, int n_params, const double* w, double c, hipStream_t s) {
    const int moving = n_params - es.frozen;
    if (moving < 1) return hipSuccess;
    hipLaunchKernelGGL(es_tell_kernel, dim3((unsigned)((moving + 3) / 4)), dim3(256), 0, s, es, n_params, w, c);
    return hipGetLastError();
}

hipError_t launch_es_tell_adam(const EsArgs& es, int n_params, const double* w, const EsAdam& ad, hipStream_t s) {
    const int moving = n_params - es.frozen;
    if (moving < 1) return hipSuccess;
    hipLaunchKernelGGL(es_tell_adam_kernel, dim3((unsigned)((moving + 3) / 4)), dim3(256), 0, s, es, n_params, w, ad);
    return hipGetLastError();
}

hipError_t launch_es_ask_sigma(const PolicyLayout& lay, const EsArgs& es, const double* sigma_vec, float* d_params, hipStream_t s) {
    const PolicyPackMap map = policy_pack_map(lay);
    hipLaunchKernelGGL(es_ask_sigma_kernel, dim3((unsigned)es.pairs, (unsigned)((lay.n_device + 255) / 256)), dim3(256), 0, s, es, sigma_vec,
                       d_params, map);
    return hipGetLastError();
}

hipError_t launch_es_rank_q(const double* fitness, int n_members, double* w, double* q, hipStream_t s) {
    hipLaunchKernelGGL(es_rank_q_kernel, dim3((unsigned)((n_members + 255) / 256)), dim3(256), 0, s, fitness, n_members, w, q);
    return hipGetLastError();
}

hipError_t launch_es_tell_sigma(const EsArgs& es, int n_params, const double* w, const double* q, double lr, const EsSigma& sv, hipStream_t s) {
    const int moving = n_params - es.frozen;
    if (moving < 1) return hipSuccess;
    hipLaunchKernelGGL(es_tell_sigma_kernel, dim3((unsigned)((moving + 3) / 4)), dim3(256), 0, s, es, n_params, w, q, lr, sv);
    return hipGetLastError();
}

hipError_t launch_es_tell_adam_sigma(const EsArgs& es, int n_params, const double* w, const double* q, const EsAdam& ad, const EsSigma& sv,
                                     hipStream_t s) {
    const int moving = n_params - es.frozen;
    if (moving < 1) return hipSuccess;
    hipLaunchKernelGGL(es_tell_adam_sigma_kernel, dim3((unsigned)((moving + 3) / 4)), dim3(256), 0, s, es, n_params, w, q, ad, sv);
    return hipGetLastError();
}

hipError_t launch_es_advance_adam(unsigned long long* state, double* beta_pow, double beta1, double beta2, hipStream_t s) {
    hipLaunchKernelGGL(es_advance_adam_kernel, dim3(1), dim3(1), 0, s, state, beta_pow, beta1, beta2);
    return hipGetLastError();
}

hipError_t launch_es_advance(unsigned long long* state, hipStream_t s) {
    hipLaunchKernelGGL(es_advance_kernel, dim3(1), dim3(1), 0, s, state);
    return hipGetLastError();
}

}  // namespace bsk
