// bsk_policy.hpp — the fused MLP policy (bsk_policy.hip; internal): what the C-ABI's bsk_policy_* entry points hand the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

struct bsk_policy_spec;            // (include/bskgpu.h)

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

hipError_t launch_policy(const PolicyArgs& args, hipStream_t s);
// The population form: args.params holds one device block of n_device floats per member, spacecraft j runs member
// j / envs_per_member; envs_per_member is a multiple of 64 and args.n a multiple of envs_per_member.
hipError_t launch_policy_population(const PolicyArgs& args, int envs_per_member, int n_device, hipStream_t s);
// `count` C-ABI blocks at src (device memory) -> `count` device blocks at dst, equal to policy_pack's bit for bit; enqueue-only
hipError_t launch_policy_pack(const PolicyLayout& lay, const float* src, float* dst, int count, hipStream_t s);
// draw += 1, one thread, behind a sample-mode policy launch on the same stream (a replayed graph draws new numbers)
hipError_t launch_policy_advance(unsigned long long* rng, hipStream_t s);

}  // namespace bsk
