// bsk_policy.hip — a small fused MLP policy over the five observation rows (a translation unit of its own; touches neither the
// step nor the rollout kernels):
//   policy_kernel           action network (5 -> hidden... -> 3 logits) and optional value network (5 -> hidden... -> 1) for n
//                           spacecraft in one launch: greedy or sampled action, log-probability, value, logits (bsk_policy_act)
//   policy_value_kernel     the value network alone for n spacecraft: no action network, no draw counter, no action row
//                           (bsk_policy_value); it shares every device function with policy_kernel
//   policy_population_kernel  policy_kernel for a population: every envs_per_member spacecraft under a parameter block of their own
//                           (bsk_population_act); it shares every device function with policy_kernel
//   policy_pack_kernel      C-ABI parameter blocks in device memory -> the device layout (bsk_population_set_params_device)
//   policy_advance_kernel   the policy's draw counter += 1, behind a sample-mode launch
// The arithmetic is the definition in include/bskgpu.h: every layer output is ONE k-ordered chain of f32 fused multiply-adds that
// starts from the bias.  Each fmaf below is written out, so the chain does not depend on -ffp-contract.
#include "../../include/bskgpu.h"
#include "bsk_philox.hpp"
#include "bsk_policy.hpp"

namespace bsk {

__device__ __forceinline__ void policy_net(const float* __restrict__ params, const PolicyNet& net, const float* x, float* buf0,
                                           float* buf1, int lane, int wave, float* out) {
    __syncthreads();                       // (the previous network's last reads of the buffers)
    if (wave == 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) buf0[i * POLICY_LANES + lane] = x[i];
    }
    __syncthreads();
    float* hin = buf0;
    float* hout = buf1;
    const int last = net.n_layers - 1;
    for (int l = 0; l < last; ++l) {
        policy_hidden(params + net.w[l], params + net.b[l], net.K[l], net.N[l], net.act, hin, hout, lane, wave);
        __syncthreads();                   // (layer l + 1 reads what every wave wrote, and overwrites what every wave has read)
        float* t = hin; hin = hout; hout = t;
    }
    if (wave == 0) policy_output(params + net.w[last], params + net.b[last], net.K[last], hin, lane, out);
}

// One workgroup's 64 spacecraft under the parameter block `params` (workgroup-uniform): the body of both kernels below.
__device__ __forceinline__ void policy_eval(const PolicyArgs& p, const float* __restrict__ params, float* policy_lds) {
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));       // (wave-uniform: weight addresses stay scalar)
    const int64_t j = (int64_t)blockIdx.x * POLICY_LANES + lane;
    const bool live = j < p.n;
    float* buf0 = policy_lds;
    float* buf1 = policy_lds + p.width * POLICY_LANES;

    float x[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const double o = live && wave == 0 ? p.obs[(int64_t)i * p.obs_stride + j] : 0.0;       // (tail lanes read nothing)
        x[i] = __builtin_fmaf((float)o, params[i], params[5 + i]);
    }
    float l[POLICY_OB] = {0.0f, 0.0f, 0.0f, 0.0f};
    policy_net(params, p.a, x, buf0, buf1, lane, wave, l);
    float val[POLICY_OB] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (p.v.n_layers > 0) policy_net(params, p.v, x, buf0, buf1, lane, wave, val);      // (workgroup-uniform)
    if (wave != 0) return;                 // (no barrier from here on)

    const float m = fmaxf(fmaxf(l[0], l[1]), l[2]);
    float e[3];
    const float s = policy_softmax(l, m, e);
    const float e0 = e[0], e1 = e[1], e2 = e[2];
    int a = 0;
    if (p.mode == BSK_POLICY_SAMPLE) {
        const unsigned long long seed = p.rng[0], draw = p.rng[1], env = p.env_base + (unsigned long long)j;
        unsigned w[4];
        philox4x32_10((unsigned)env, (unsigned)(env >> 32), (unsigned)draw, (unsigned)(draw >> 32), (unsigned)seed, (unsigned)(seed >> 32), w);
        const float u = (float)(w[0] >> 8) * 0x1p-24f;
        const float c0 = e0 / s, c1 = c0 + e1 / s;
        a = u < c0 ? 0 : (u < c1 ? 1 : 2);
    } else {
        float best = l[0];
        if (policy_beats(l[1], best)) { best = l[1]; a = 1; }
        if (policy_beats(l[2], best)) { best = l[2]; a = 2; }
    }
    if (!live) return;
    p.action[j] = a;
    if (p.logp) p.logp[j] = policy_logp(a == 0 ? l[0] : (a == 1 ? l[1] : l[2]), m, s);
    if (p.value) p.value[j] = val[0];
    if (p.logits) {
#pragma unroll
        for (int i = 0; i < 3; ++i) p.logits[(int64_t)i * p.out_stride + j] = l[i];
    }
}

__global__ __launch_bounds__(POLICY_BLOCK) void policy_kernel(const PolicyArgs p) {
    extern __shared__ float policy_lds[];
    policy_eval(p, p.params, policy_lds);
}

// The value network alone (bsk_policy_value): policy_eval's geometry - one lane per spacecraft, POLICY_WAVES waves per 64 columns,
// activations through the LDS columns [unit][lane], the block address workgroup-uniform so that the weight loads stay scalar - and
// its device functions, so the value is the one policy_kernel writes, bit for bit.  No action network is walked, the draw counter
// is not read and no action row is written: nothing of the policy's single-stream state is touched.
__global__ __launch_bounds__(POLICY_BLOCK) void policy_value_kernel(const PolicyValueArgs p) {
    extern __shared__ float policy_lds[];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));       // (wave-uniform: weight addresses stay scalar)
    const int64_t j = (int64_t)blockIdx.x * POLICY_LANES + lane;
    const bool live = j < p.n;
    float x[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {                          // (step 1 of the definition, as policy_eval writes it)
        const double o = live && wave == 0 ? p.obs[(int64_t)i * p.obs_stride + j] : 0.0;       // (tail lanes read nothing)
        x[i] = __builtin_fmaf((float)o, p.params[i], p.params[5 + i]);
    }
    float val[POLICY_OB] = {0.0f, 0.0f, 0.0f, 0.0f};
    policy_net(p.params, p.v, x, policy_lds, policy_lds + p.width * POLICY_LANES, lane, wave, val);
    if (wave == 0 && live) p.value[j] = val[0];            // (tail lanes write nothing)
}

// The log-probabilities of all three actions (bsk_fit_accumulate_pg reads those of the actions taken): policy_eval's geometry and
// its device functions once more - the action network, then steps 5 and 6 in policy_eval's own text and this unit's own arithmetic
// mode - so that lp[a][j] is, bit for bit, the logp policy_kernel writes when it chooses a.  Touches nothing of the policy's
// single-stream state.
__global__ __launch_bounds__(POLICY_BLOCK) void policy_logp_kernel(const PolicyLogpArgs p) {
    extern __shared__ float policy_lds[];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));       // (wave-uniform: weight addresses stay scalar)
    const int64_t j = (int64_t)blockIdx.x * POLICY_LANES + lane;
    const bool live = j < p.n;
    float x[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {                          // (step 1 of the definition, as policy_eval writes it)
        const double o = live && wave == 0 ? p.obs[(int64_t)i * p.obs_stride + j] : 0.0;       // (tail lanes read nothing)
        x[i] = __builtin_fmaf((float)o, p.params[i], p.params[5 + i]);
    }
    float l[POLICY_OB] = {0.0f, 0.0f, 0.0f, 0.0f};
    policy_net(p.params, p.a, x, policy_lds, policy_lds + p.width * POLICY_LANES, lane, wave, l);
    if (wave != 0 || !live) return;                        // (no barrier from here on; tail lanes write nothing)
    const float m = fmaxf(fmaxf(l[0], l[1]), l[2]);
    float e[3];
    const float s = policy_softmax(l, m, e);
#pragma unroll
    for (int i = 0; i < 3; ++i) p.lp[(int64_t)i * p.n + j] = policy_logp(l[i], m, s);
}

// The population form (bsk_population_act): workgroup b serves the same 64 spacecraft and takes the parameter block of member
// b / wg_per_member, wg_per_member = envs_per_member / 64.  The block address depends on blockIdx alone, so it is as scalar as
// p.params is above and policy_hidden's weight loads stay one scalar load of 16 consecutive floats: nothing else differs.
__global__ __launch_bounds__(POLICY_BLOCK) void policy_population_kernel(const PolicyArgs p, int wg_per_member, int n_device) {
    extern __shared__ float policy_lds[];
    const unsigned member = blockIdx.x / (unsigned)wg_per_member;
    policy_eval(p, p.params + (size_t)member * (size_t)n_device, policy_lds);
}

// The C-ABI parameter blocks of `count` members (src, n_params floats each, DEVICE memory) -> their device layouts (dst, n_device
// floats each): what policy_pack makes on the host, bit for bit.  A gather - every float of the device block is written by exactly
// one thread, from its source element or as a zero of the padding - so there is no ordering between threads to get wrong.
__global__ __launch_bounds__(256) void policy_pack_kernel(const float* __restrict__ src, float* __restrict__ dst, const PolicyPackMap map) {
    const int d = (int)(blockIdx.y * blockDim.x + threadIdx.x);        // (members along x: there may be more than 65 535 of them)
    if (d >= map.n_device) return;
    const float* __restrict__ from = src + (size_t)blockIdx.x * (size_t)map.n_params;
    const int j = policy_pack_source(map, d);
    dst[(size_t)blockIdx.x * (size_t)map.n_device + d] = j >= 0 ? from[j] : 0.0f;
}

__global__ void policy_advance_kernel(unsigned long long* rng) { rng[1] += 1ull; }

hipError_t launch_policy(const PolicyArgs& args, hipStream_t s) {
    const size_t lds = (size_t)2 * args.width * POLICY_LANES * sizeof(float);
    hipLaunchKernelGGL(policy_kernel, dim3((unsigned)((args.n + POLICY_LANES - 1) / POLICY_LANES)), dim3(POLICY_BLOCK), lds, s, args);
    return hipGetLastError();
}

hipError_t launch_policy_value(const PolicyValueArgs& args, hipStream_t s) {
    const size_t lds = (size_t)2 * args.width * POLICY_LANES * sizeof(float);
    hipLaunchKernelGGL(policy_value_kernel, dim3((unsigned)((args.n + POLICY_LANES - 1) / POLICY_LANES)), dim3(POLICY_BLOCK), lds, s, args);
    return hipGetLastError();
}

hipError_t launch_policy_logp(const PolicyLogpArgs& args, hipStream_t s) {
    const size_t lds = (size_t)2 * args.width * POLICY_LANES * sizeof(float);
    hipLaunchKernelGGL(policy_logp_kernel, dim3((unsigned)((args.n + POLICY_LANES - 1) / POLICY_LANES)), dim3(POLICY_BLOCK), lds, s, args);
    return hipGetLastError();
}

hipError_t launch_policy_population(const PolicyArgs& args, int envs_per_member, int n_device, hipStream_t s) {
    const size_t lds = (size_t)2 * args.width * POLICY_LANES * sizeof(float);
    hipLaunchKernelGGL(policy_population_kernel, dim3((unsigned)((args.n + POLICY_LANES - 1) / POLICY_LANES)), dim3(POLICY_BLOCK), lds, s,
                       args, envs_per_member / POLICY_LANES, n_device);
    return hipGetLastError();
}

PolicyPackMap policy_pack_map(const PolicyLayout& lay) {
    PolicyPackMap map = {};
    map.n_params = lay.n_params;
    map.n_device = lay.n_device;
    const PolicyNet* nets[2] = {&lay.a, &lay.v};
    const int n_out[2] = {3, 1};
    int at = 10;
    for (int t = 0; t < 2; ++t) {
        const PolicyNet& net = *nets[t];
        for (int l = 0; l < net.n_layers; ++l) {
            PolicyPackMap::Layer& y = map.layer[map.n_layers++];
            y.K = net.K[l]; y.N = net.N[l]; y.w = net.w[l]; y.b = net.b[l];
            y.fan_out = l == net.n_layers - 1 ? n_out[t] : net.N[l];
            y.src = at;
            at += y.fan_out * y.K + y.fan_out;
        }
    }
    return map;
}

hipError_t launch_policy_pack(const PolicyLayout& lay, const float* src, float* dst, int count, hipStream_t s) {
    const PolicyPackMap map = policy_pack_map(lay);
    hipLaunchKernelGGL(policy_pack_kernel, dim3((unsigned)count, (unsigned)((lay.n_device + 255) / 256)), dim3(256), 0, s, src, dst, map);
    return hipGetLastError();
}

hipError_t launch_policy_advance(unsigned long long* rng, hipStream_t s) {
    hipLaunchKernelGGL(policy_advance_kernel, dim3(1), dim3(1), 0, s, rng);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------------------
// host side: the spec's rules, the C-ABI parameter count and the device layout
static const char* policy_net_layout(int n_hidden, const int32_t* hidden, int activation, int n_out, int out_block, int& n_params,
                                     int& n_device, int& width, PolicyNet& net) {
    if (n_hidden < 0 || n_hidden > POLICY_MAX_LAYERS - 1) return "a network has 0 to 3 hidden layers";
    if (activation != BSK_POLICY_RELU && activation != BSK_POLICY_TANH) return "activation must be BSK_POLICY_RELU or BSK_POLICY_TANH";
    net = PolicyNet{};
    net.n_layers = n_hidden + 1;
    net.act = activation;
    int K = 5;
    for (int l = 0; l <= n_hidden; ++l) {
        const bool out = l == n_hidden;
        const int fan_out = out ? n_out : hidden[l];
        if (!out && (fan_out < 16 || fan_out > 128 || fan_out % 16 != 0)) return "a hidden layer is 16 ... 128 units wide, in multiples of 16";
        const int N = out ? out_block : fan_out;
        net.K[l] = K;
        net.N[l] = N;
        net.w[l] = n_device;
        n_device += (K * N + 15) / 16 * 16;
        net.b[l] = n_device;
        n_device += (N + 15) / 16 * 16;
        n_params += K * fan_out + fan_out;
        if (K > width) width = K;
        K = fan_out;
    }
    return nullptr;
}

const char* policy_layout(const bsk_policy_spec& spec, PolicyLayout& out) {
    out = PolicyLayout{};
    out.n_params = 10;
    out.n_device = POLICY_HEAD;
    out.width = 8;
    if (const char* why = policy_net_layout(spec.n_hidden, spec.hidden, spec.activation, 3, POLICY_OB, out.n_params, out.n_device, out.width, out.a))
        return why;
    if (spec.has_value != 0 && spec.has_value != 1) return "has_value must be 0 or 1";
    if (spec.has_value)
        return policy_net_layout(spec.v_n_hidden, spec.v_hidden, spec.v_activation, 1, POLICY_OB, out.n_params, out.n_device, out.width, out.v);
    return nullptr;
}

void policy_pack(const PolicyLayout& lay, const float* params, std::vector<float>& dev) {
    dev.assign((size_t)lay.n_device, 0.0f);
    for (int i = 0; i < 10; ++i) dev[i] = params[i];
    const float* src = params + 10;
    const PolicyNet* nets[2] = {&lay.a, &lay.v};
    const int n_out[2] = {3, 1};
    for (int t = 0; t < 2; ++t) {
        const PolicyNet& net = *nets[t];
        for (int l = 0; l < net.n_layers; ++l) {
            const int K = net.K[l], N = net.N[l], fan_out = l == net.n_layers - 1 ? n_out[t] : N;
            for (int jo = 0; jo < fan_out; ++jo)
                for (int k = 0; k < K; ++k) dev[(size_t)net.w[l] + (size_t)k * N + jo] = src[(size_t)jo * K + k];
            src += (size_t)fan_out * K;
            for (int jo = 0; jo < fan_out; ++jo) dev[(size_t)net.b[l] + jo] = src[jo];
            src += fan_out;
        }
    }
}

// the inverse of policy_pack: one member's device block -> its C-ABI parameter block (n_params floats)
void policy_unpack(const PolicyLayout& lay, const float* dev, float* params) {
    for (int i = 0; i < 10; ++i) params[i] = dev[i];
    float* dst = params + 10;
    const PolicyNet* nets[2] = {&lay.a, &lay.v};
    const int n_out[2] = {3, 1};
    for (int t = 0; t < 2; ++t) {
        const PolicyNet& net = *nets[t];
        for (int l = 0; l < net.n_layers; ++l) {
            const int K = net.K[l], N = net.N[l], fan_out = l == net.n_layers - 1 ? n_out[t] : N;
            for (int jo = 0; jo < fan_out; ++jo)
                for (int k = 0; k < K; ++k) dst[(size_t)jo * K + k] = dev[(size_t)net.w[l] + (size_t)k * N + jo];
            dst += (size_t)fan_out * K;
            for (int jo = 0; jo < fan_out; ++jo) dst[jo] = dev[(size_t)net.b[l] + jo];
            dst += fan_out;
        }
    }
}

}  // namespace bsk
