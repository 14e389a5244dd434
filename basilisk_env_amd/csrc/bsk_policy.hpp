// bsk_policy.hpp — the fused MLP policy (bsk_policy.hip; internal): what the C-ABI's bsk_policy_* entry points hand the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/bskgpu.h"

namespace bsk {

constexpr int POLICY_MAX_LAYERS = 4;       // three hidden layers and the output layer
constexpr int POLICY_JB = 16;              // hidden units evaluated side by side (hidden widths are multiples of it)
constexpr int POLICY_OB = 4;               // the output layer's block: 3 logits / 1 value padded with zero rows
constexpr int POLICY_HEAD = 16;            // floats in front of the first layer: in_scale[5], in_shift[5], padding

// One network as the kernel walks it.  The DEVICE layout of its parameters differs from the C-ABI's (torch's W[out][in]): per layer
// Wt[K][N] - transposed, so that the weights of POLICY_JB neighbouring units for one input k are consecutive (one scalar load) - then
// b[N]; N is the fan-out rounded up to the layer's block with zero rows.  Offsets are in floats from the start of the block.
struct PolicyNet {
    int n_layers;                  // hidden layers + 1; 0: there is no such network
    int act;                       // BSK_POLICY_RELU / BSK_POLICY_TANH of the hidden layers
    int K[POLICY_MAX_LAYERS], N[POLICY_MAX_LAYERS];
    int w[POLICY_MAX_LAYERS], b[POLICY_MAX_LAYERS];
};

struct PolicyArgs {
    const float* params;           // device layout (PolicyLayout)
    PolicyNet a, v;
    const double* obs;             // [5][obs_stride]
    int64_t obs_stride;
    int n;
    unsigned long long env_base;
    int mode;                      // BSK_POLICY_GREEDY / BSK_POLICY_SAMPLE
    const unsigned long long* rng; // {seed, draw}
    int* action;                   // [n]
    float* logp;                   // [n] or NULL
    float* value;                  // [n] or NULL
    float* logits;                 // [3][out_stride] or NULL
    int64_t out_stride;
    int width;                     // LDS floats per lane and buffer: the widest layer input (>= 5)
};

// what policy_value_kernel takes: the value network alone (bsk_policy_value)
struct PolicyValueArgs {
    const float* params;           // device layout (PolicyLayout)
    PolicyNet v;                   // n_layers >= 1
    const double* obs;             // [5][obs_stride]
    int64_t obs_stride;
    int n;
    float* value;                  // [n]
    int width;                     // the layout's width (both networks'), as PolicyArgs::width
};

// What policy_logp_kernel takes: the action network alone, and where the three log-probabilities of every spacecraft go
struct PolicyLogpArgs {
    const float* params;           // device layout (PolicyLayout)
    PolicyNet a;
    const double* obs;             // [5][obs_stride]
    int64_t obs_stride;
    int n;
    float* lp;                     // [3][n]
    int width;                     // the layout's width, as PolicyArgs::width
};

// Host side of the layout: checks a spec, counts its C-ABI parameters, and repacks them for the device.
struct PolicyLayout {
    PolicyNet a, v;
    int n_params;                  // floats of the C-ABI block: in_scale, in_shift, then per layer W[out][in], b[out]
    int n_device;                  // floats of the device block
    int width;
};
// -> NULL when the spec is a legal policy (layout filled), else what is wrong with it
const char* policy_layout(const bsk_policy_spec& spec, PolicyLayout& out);
void policy_pack(const PolicyLayout& lay, const float* params, std::vector<float>& device_block);

// the inverse: one device block -> the C-ABI block of n_params floats (the padding is dropped)
void policy_unpack(const PolicyLayout& lay, const float* device_block, float* params);

// What the pack kernel walks: per layer (action network first) where its Wt[K][N] and b[N] lie in the device block and where its
// W[fan_out][K], b[fan_out] start in the C-ABI block.
struct PolicyPackMap {
    struct Layer { int K, N, fan_out, w, b, src; };
    int n_layers;                  // of both networks together
    int n_params, n_device;
    Layer layer[2 * POLICY_MAX_LAYERS];
};
PolicyPackMap policy_pack_map(const PolicyLayout& lay);
// Where float d of a device block comes from: the index of its source in the C-ABI block, or -1 for a zero of the padding.
__device__ __forceinline__ int policy_pack_source(const PolicyPackMap& map, int d) {
    int j = d < 10 ? d : -1;
    for (int l = 0; l < map.n_layers; ++l) {
        const PolicyPackMap::Layer& y = map.layer[l];
        if (d >= y.w && d < y.w + y.K * y.N) {
            const int k = (d - y.w) / y.N, jo = (d - y.w) % y.N;
            if (jo < y.fan_out) j = y.src + jo * y.K + k;
        } else if (d >= y.b && d < y.b + y.fan_out) {
            j = y.src + y.fan_out * y.K + (d - y.b);
        }
    }
    return j;
}

// One lane per spacecraft and POLICY_WAVES waves per 64 spacecraft: the waves of a workgroup share the spacecraft and split each hidden
// layer's units between them, 16 at a time.  65 536 spacecraft are only 1 024 wave-columns, one per SIMD: with one wave each, a launch
// is as long as one wave's whole chain with nothing to hide its load latencies behind (measured: 31.8 us for relu [64, 64]); four
// waves cut the chain into four and give every SIMD four waves to switch between.  The weights are wave-uniform: a lane's 16
// neighbouring units share the input h_k, so per k a wave makes one LDS read (h_k of its 64 spacecraft), one scalar load (16
// consecutive weights of Wt[k][j0 .. j0+16), SGPR operands) and 8 independent v_pk_fma_f32 - no weight ever enters a VGPR or the
// LDS.  Activations go from layer to layer through LDS columns [unit][lane]: conflict-free, one barrier per layer.  Every unit's
// chain is evaluated by exactly one wave in the definition's order, so the split changes no bit.  (A v_mfma_f32_32x32x2_f32 form of
// the hidden layers was measured level with this one at [64, 64]: docs/KERNEL_NOTES.md.)
constexpr int POLICY_LANES = 64;
constexpr int POLICY_WAVES = 4;
constexpr int POLICY_BLOCK = POLICY_LANES * POLICY_WAVES;

__device__ __forceinline__ float policy_act(float z, int act) {
    return act == BSK_POLICY_TANH ? tanhf(z) : (z > 0.0f ? z : 0.0f);
}

// a hidden layer: hout[j] = act(b[j] + sum_k Wt[k][j] * hin[k]), k ascending; wave w takes the blocks of POLICY_JB units w, w + 4, ...
__device__ __forceinline__ void policy_hidden(const float* __restrict__ wt, const float* __restrict__ bias, int K, int N, int act,
                                              const float* hin, float* hout, int lane, int wave) {
    for (int j0 = wave * POLICY_JB; j0 < N; j0 += POLICY_WAVES * POLICY_JB) {
        float z[POLICY_JB];
#pragma unroll
        for (int jj = 0; jj < POLICY_JB; ++jj) z[jj] = bias[j0 + jj];
#pragma unroll 4
        for (int k = 0; k < K; ++k) {
            const float h = hin[k * POLICY_LANES + lane];
            const float* __restrict__ w = wt + k * N + j0;
#pragma unroll
            for (int jj = 0; jj < POLICY_JB; ++jj) z[jj] = __builtin_fmaf(w[jj], h, z[jj]);
        }
#pragma unroll
        for (int jj = 0; jj < POLICY_JB; ++jj) hout[(j0 + jj) * POLICY_LANES + lane] = policy_act(z[jj], act);
    }
}

// the output layer (linear): POLICY_OB rows, the ones beyond the fan-out are zero rows of the device layout.  Wave 0 alone evaluates
// it: it is the wave that reads the observations and stores the results.
__device__ __forceinline__ void policy_output(const float* __restrict__ wt, const float* __restrict__ bias, int K, const float* hin,
                                              int lane, float* out) {
#pragma unroll
    for (int jj = 0; jj < POLICY_OB; ++jj) out[jj] = bias[jj];
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        const float h = hin[k * POLICY_LANES + lane];
        const float* __restrict__ w = wt + k * POLICY_OB;
#pragma unroll
        for (int jj = 0; jj < POLICY_OB; ++jj) out[jj] = __builtin_fmaf(w[jj], h, out[jj]);
    }
}

// (value, index) order of the greedy choice: the greater logit wins, equal logits go to the lower index, a NaN loses to every
// number (bsk_fork.hip: beats() - the rule of bsk_select_branches)
__device__ __forceinline__ bool policy_beats(float a, float b) {      // a (the later index) displaces b (the earlier one)
    const bool na = a != a, nb = b != b;
    if (na != nb) return nb;
    return !na && a > b;
}

// Steps 5 and 6 of the definition: e_i = expf(l_i - m), s = (e_0 + e_1) + e_2 -> s, and the log-probability (l_i - m) - logf(s).
// One text for policy_kernel and policy_logp_kernel.  It must also be compiled in ONE unit: the compiler expands expf and logf into
// compensated products whose last subtraction / addition it fuses or not with the unit's contraction mode, which moves s and logp
// in their last bit - so bsk_fit.hip, built without contraction, reads these log-probabilities from policy_logp_kernel instead of
// forming them itself.
__device__ __forceinline__ float policy_softmax(const float* l, float m, float* e) {
    e[0] = expf(l[0] - m);
    e[1] = expf(l[1] - m);
    e[2] = expf(l[2] - m);
    return (e[0] + e[1]) + e[2];
}
__device__ __forceinline__ float policy_logp(float l_i, float m, float s) { return (l_i - m) - logf(s); }

hipError_t launch_policy(const PolicyArgs& args, hipStream_t s);
// the value network alone, policy_kernel's value bit for bit: reads the parameters and the observations, writes value[0 .. n)
hipError_t launch_policy_value(const PolicyValueArgs& args, hipStream_t s);
// lp[i][j] = (l_i - m) - logf(s) of spacecraft j, i = 0 .. 2: for ANY action what policy_kernel writes as the logp of its own, bit for bit
hipError_t launch_policy_logp(const PolicyLogpArgs& args, hipStream_t s);
// The population form: args.params holds one device block of n_device floats per member, spacecraft j runs member
// j / envs_per_member; envs_per_member is a multiple of 64 and args.n a multiple of envs_per_member.
hipError_t launch_policy_population(const PolicyArgs& args, int envs_per_member, int n_device, hipStream_t s);
// `count` C-ABI blocks at src (device memory) -> `count` device blocks at dst, equal to policy_pack's bit for bit; enqueue-only
hipError_t launch_policy_pack(const PolicyLayout& lay, const float* src, float* dst, int count, hipStream_t s);
// draw += 1, one thread, behind a sample-mode policy launch on the same stream (a replayed graph draws new numbers)
hipError_t launch_policy_advance(unsigned long long* rng, hipStream_t s);

}  // namespace bsk
