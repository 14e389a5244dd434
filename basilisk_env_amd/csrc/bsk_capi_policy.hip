// bsk_capi_policy.hip — C-ABI of what drives an environment handle from the device: the fused MLP policy (bsk_policy_*), the
// population of policies (bsk_population_*) and the running observation statistics that give a policy its input normalisation
// (bsk_obs_stats_*); the evolution strategy over them (bsk_es_*) is bsk_capi_es.hip, and what the two share bsk_capi_policy.hpp.
// Host side only, as bsk_capi.hip; kernels and launch wrappers: bsk_policy.hip, bsk_population.hip, bsk_obsstats.hip.
#include <cmath>
#include <cstring>

#include "bsk_capi_policy.hpp"

using namespace bsk::capi;

namespace bsk { namespace capi {

int policy_spec_layout(const bsk_policy_spec* spec, bsk::PolicyLayout& lay) {
    if (!spec) return fail(BSK_EINVAL, "spec is NULL");
    if (spec->abi_version != BSK_ABI_VERSION || spec->struct_size != sizeof(bsk_policy_spec))
        return fail(BSK_EABI, "bsk_policy_spec abi_version / struct_size mismatch");
    if (const char* why = bsk::policy_layout(*spec, lay)) return fail(BSK_EINVAL, std::string("bsk_policy_spec: ") + why);
    return BSK_OK;
}

void free_all(std::initializer_list<void*> bufs) {
    bool any = false;
    for (void* b : bufs) any = any || b;
    if (any) (void)hipDeviceSynchronize();
    for (void* b : bufs)
        if (b) (void)hipFree(b);
}

int transfer(int device, hipMemcpyKind dir, std::initializer_list<Field> fields) {
    DeviceGuard guard(device);
    const bool get = dir == hipMemcpyDeviceToHost;
    HIP_SYNC(hipDeviceSynchronize());
    for (const Field& f : fields)
        if (f.host) HIP_COPY(hipMemcpy((void*)(get ? f.host : f.dev), get ? f.dev : f.host, f.bytes, dir));
    return BSK_OK;
}

// A rollout's scratch buffer is replaced by one of `bytes`: refused while `stream` is being captured; a queued rollout may still use
// the smaller buffer, so the device is waited for before that is freed.  The caller decides when, and records the new capacity.
int grow_scratch(void** d_buf, int* cap, size_t bytes, hipStream_t stream, const char* capture_msg) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(stream, &st));
    if (st != hipStreamCaptureStatusNone) return fail(BSK_EINVAL, capture_msg);
    if (*d_buf) {
        HIP_SYNC(hipDeviceSynchronize());
        (void)hipFree(*d_buf);
        *d_buf = nullptr;
        *cap = 0;
    }
    HIP_TRY(hipMalloc(d_buf, bytes));
    return BSK_OK;
}

} }  // namespace bsk::capi

namespace {

// the parameter blocks (left as allocated) and the draw counter {0, 0}
int store_alloc(ParamStore* p) {
    const unsigned long long rng0[2] = {0ull, 0ull};
    HIP_TRY(hipMalloc(&p->d_params, (size_t)p->n_members * (size_t)p->lay.n_device * sizeof(float)));
    HIP_TRY(hipMalloc(&p->d_rng, sizeof rng0));
    HIP_COPY(hipMemcpy(p->d_rng, rng0, sizeof rng0, hipMemcpyHostToDevice));
    return BSK_OK;
}

// every argument of a launch, checked before anything is enqueued.  envs_per_member = 0: a policy (`what` names it in the
// messages); otherwise a population, with the member rule on top
int check_act(const ParamStore* p, const char* what, int envs_per_member, const double* d_obs, int64_t obs_stride, int n, int64_t env_base,
              int mode, const int32_t* d_action, const float* d_value, const float* d_logits, int64_t out_stride) {
    if (!p || !d_obs || !d_action) return fail(BSK_EINVAL, std::string(what) + "/d_obs/d_action is NULL");
    if (n < 1 || n > (1 << 28)) return fail(BSK_EINVAL, "n must be in 1..2^28");
    if (envs_per_member != 0) {
        if (envs_per_member < 64 || envs_per_member % 64 != 0) return fail(BSK_EINVAL, "envs_per_member must be a positive multiple of 64");
        if ((int64_t)p->n_members * envs_per_member != (int64_t)n) return fail(BSK_EINVAL, "n must be n_members * envs_per_member");
    }
    if (obs_stride < n) return fail(BSK_EINVAL, "obs_stride must be >= n");
    if (env_base < 0) return fail(BSK_EINVAL, "env_base must be >= 0");
    if (mode != BSK_POLICY_GREEDY && mode != BSK_POLICY_SAMPLE) return fail(BSK_EINVAL, "mode must be BSK_POLICY_GREEDY or BSK_POLICY_SAMPLE");
    if (d_value && p->lay.v.n_layers == 0) return fail(BSK_EINVAL, std::string("d_value given, but the ") + what + " has no value network");
    if (d_logits && out_stride < n) return fail(BSK_EINVAL, "out_stride must be >= n");
    return BSK_OK;
}

// envs_per_member = 0: policy_kernel on the one block; otherwise policy_population_kernel, member m on its own block
int launch_act(ParamStore* p, int envs_per_member, const double* d_obs, int64_t obs_stride, int n, int64_t env_base, int mode,
               int32_t* d_action, float* d_logp, float* d_value, float* d_logits, int64_t out_stride, hipStream_t stream) {
    bsk::PolicyArgs a;
    a.params = p->d_params; a.a = p->lay.a; a.v = p->lay.v; a.obs = d_obs; a.obs_stride = obs_stride; a.n = n;
    a.env_base = (unsigned long long)env_base; a.mode = mode; a.rng = p->d_rng; a.action = d_action; a.logp = d_logp;
    a.value = d_value; a.logits = d_logits; a.out_stride = out_stride; a.width = p->lay.width;
    if (!d_value) a.v.n_layers = 0;            // (nobody asked for the value: its network is not evaluated)
    if (envs_per_member == 0) HIP_TRY(bsk::launch_policy(a, stream));
    else HIP_TRY(bsk::launch_policy_population(a, envs_per_member, p->lay.n_device, stream));
    if (mode == BSK_POLICY_SAMPLE) HIP_TRY(bsk::launch_policy_advance(p->d_rng, stream));
    return BSK_OK;
}

// The entry points that touch the parameters or the draw counter from the host come after everything queued on the object's device:
// it keeps no stream of its own, and the stream of its last launch may be gone with the handle that owned it.
int store_upload(ParamStore* p, const float* params) {
    const size_t nd = (size_t)p->lay.n_device;
    std::vector<float> all((size_t)p->n_members * nd), one;
    for (int m = 0; m < p->n_members; ++m) {
        bsk::policy_pack(p->lay, params + (size_t)m * (size_t)p->lay.n_params, one);
        std::memcpy(all.data() + (size_t)m * nd, one.data(), nd * sizeof(float));
    }
    HIP_SYNC(hipDeviceSynchronize());                     // (queued launches still read the old parameters)
    HIP_COPY(hipMemcpy(p->d_params, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice));
    return BSK_OK;
}

int set_rng(ParamStore* p, const char* null_msg, uint64_t seed, uint64_t draw) {
    if (!p) return fail(BSK_EINVAL, null_msg);
    const unsigned long long w[2] = {seed, draw};
    return transfer(p->device, hipMemcpyHostToDevice, {{w, p->d_rng, sizeof w}});
}

int get_rng(ParamStore* p, const char* null_msg, uint64_t* seed, uint64_t* draw) {
    if (!p) return fail(BSK_EINVAL, null_msg);
    unsigned long long w[2];
    if (int rc = transfer(p->device, hipMemcpyDeviceToHost, {{w, p->d_rng, sizeof w}})) return rc;
    if (seed) *seed = w[0];
    if (draw) *draw = w[1];
    return BSK_OK;
}

// the history outputs of a rollout, [n_steps] rows each; any may be NULL
struct RolloutHist {
    double *obs, *reward;
    uint8_t* reason;
    int32_t* action;
    float *logp, *value;
};

// The closed loop of both rollouts, enqueued on the handle's stream with no host visit in between.  Per env step: the actions of the
// current observations (into row t of the action history, or into d_act where none is kept), the step on them, and row t of the
// other histories - with one step of the value rule in the SAME launch where `acc` is given, alone otherwise (no launch for no row).
// `out` (with `acc` only): the outcome rule in that launch too, on the action row of this step.
// With a statistics object attached, the observations each launch of the policy reads are accumulated in front of it - under `acc`
// those of the envs still alive, as the previous step's launch of the value rule left them - and joined once behind the last step.
int rollout_steps(ParamStore* p, int envs_per_member, bsk_handle* h, int mode, int substeps, int n_steps, const RolloutHist& hist,
                  int32_t* d_act, const bsk::FitnessAcc* acc, double gamma, const bsk::OutcomeAcc* out = nullptr) {
    const size_t n = (size_t)h->n;
    const int n_stats = envs_per_member > 0 && p->n_counted > 0 ? p->n_counted * envs_per_member : h->n;     // (<= h->n: n_counted <= n_members)
    for (int t = 0; t < n_steps; ++t) {
        int32_t* act = hist.action ? hist.action + t * n : d_act;
        if (p->stats)
            HIP_TRY(bsk::launch_obs_stats(h->d_obs, h->ostride, n_stats, acc && t > 0 ? acc->alive : nullptr, p->stats->st, h->stream));
        int rc = launch_act(p, envs_per_member, h->d_obs, h->ostride, h->n, (int64_t)h->env_base, mode, act,
                            hist.logp ? hist.logp + t * n : nullptr, hist.value ? hist.value + t * n : nullptr, nullptr, 0, h->stream);
        if (rc) return rc;
        if ((rc = do_step(h, act, substeps, 1))) return rc;
        double* obs_row = hist.obs ? hist.obs + t * 5 * n : nullptr;
        double* reward_row = hist.reward ? hist.reward + t * n : nullptr;
        uint8_t* reason_row = hist.reason ? hist.reason + t * n : nullptr;
        if (acc && out)
            HIP_TRY(bsk::launch_outcome_row(h->d_obs, h->d_reward, h->d_reason, act, h->ostride, h->n, obs_row, reward_row, reason_row, *acc,
                                            *out, gamma, t == 0, h->stream));
        else if (acc)
            HIP_TRY(bsk::launch_fitness_row(h->d_obs, h->d_reward, h->d_reason, h->ostride, h->n, obs_row, reward_row, reason_row, *acc,
                                            gamma, t == 0, h->stream));
        else
            HIP_TRY(bsk::launch_hist_row(h->d_obs, h->d_reward, h->d_reason, h->ostride, h->n, obs_row, reward_row, reason_row, h->stream));
    }
    if (p->stats) HIP_TRY(bsk::launch_obs_stats_join(p->stats->st, h->stream));
    return BSK_OK;
}

// what a rollout refuses of an attached statistics object before anything is enqueued
int check_stats(const ParamStore* p, const bsk_handle* h) {
    if (!p->stats) return BSK_OK;
    if (p->stats->device != h->device) return fail(BSK_EINVAL, "the attached observation statistics and the handle live on different devices");
    // (a population that counts its first n_counted members only: their envs; the caller has checked that n_members divides h->n)
    const int64_t n = p->n_counted > 0 ? (int64_t)p->n_counted * (h->n / p->n_members) : (int64_t)h->n;
    if (n > p->stats->n_cap) return fail(BSK_EINVAL, "the handle's n_envs exceeds the capacity of the attached observation statistics");
    return BSK_OK;
}

int attach_stats(ParamStore* p, const char* null_msg, bsk_obs_stats* stats) {
    if (!p) return fail(BSK_EINVAL, null_msg);
    p->stats = stats;
    return BSK_OK;
}

}  // namespace

extern "C" {

int bsk_policy_n_params(const bsk_policy_spec* spec) {
    bsk::PolicyLayout lay;
    int rc = policy_spec_layout(spec, lay);
    return rc ? rc : lay.n_params;
}

int bsk_policy_create(const bsk_policy_spec* spec, const float* params, int device_id, bsk_policy** out) {
    bsk::PolicyLayout lay;
    int rc = create_begin(spec, out, lay);
    if (rc) return rc;
    if (!params) return fail(BSK_EINVAL, "params is NULL");
    return create_on_device(lay, device_id, out, bsk_policy_destroy, [&](bsk_policy* p) -> int {
        int rc = store_alloc(p);
        return rc ? rc : store_upload(p, params);
    });
}

int bsk_policy_set_params(bsk_policy* p, const float* params) {
    if (!p || !params) return fail(BSK_EINVAL, "policy/params is NULL");
    DeviceGuard guard(p->device);
    return store_upload(p, params);
}

void bsk_policy_destroy(bsk_policy* p) {
    if (!p) return;
    DeviceGuard guard(p->device);
    free_all({p->d_params, p->d_rng, p->d_act});
    delete p;
}

int bsk_policy_set_obs_stats(bsk_policy* p, bsk_obs_stats* stats) { return attach_stats(p, "policy is NULL", stats); }
int bsk_policy_set_rng(bsk_policy* p, uint64_t seed, uint64_t draw) { return set_rng(p, "policy is NULL", seed, draw); }
int bsk_policy_get_rng(bsk_policy* p, uint64_t* seed, uint64_t* draw) { return get_rng(p, "policy is NULL", seed, draw); }

int bsk_policy_act(bsk_policy* p, const double* d_obs, int64_t obs_stride, int n, int64_t env_base, int mode,
                   int32_t* d_action, float* d_logp, float* d_value, float* d_logits, int64_t out_stride, void* stream) {
    int rc = check_act(p, "policy", 0, d_obs, obs_stride, n, env_base, mode, d_action, d_value, d_logits, out_stride);
    if (rc) return rc;
    DeviceGuard guard(p->device);
    return launch_act(p, 0, d_obs, obs_stride, n, env_base, mode, d_action, d_logp, d_value, d_logits, out_stride, (hipStream_t)stream);
}

int bsk_policy_value(bsk_policy* p, const double* d_obs, int64_t obs_stride, int n, float* d_value, void* stream) {
    if (!p || !d_obs || !d_value) return fail(BSK_EINVAL, "policy/d_obs/d_value is NULL");
    if (n < 1 || n > (1 << 28)) return fail(BSK_EINVAL, "n must be in 1..2^28");
    if (obs_stride < n) return fail(BSK_EINVAL, "obs_stride must be >= n");
    if (p->lay.v.n_layers == 0) return fail(BSK_EINVAL, "bsk_policy_value: the policy has no value network");
    DeviceGuard guard(p->device);
    bsk::PolicyValueArgs a;
    a.params = p->d_params; a.v = p->lay.v; a.obs = d_obs; a.obs_stride = obs_stride; a.n = n; a.value = d_value; a.width = p->lay.width;
    HIP_TRY(bsk::launch_policy_value(a, (hipStream_t)stream));
    return BSK_OK;
}

int bsk_policy_rollout(bsk_policy* p, bsk_handle* h, int mode, int substeps, int n_steps,
                       double* d_obs_hist, double* d_reward_hist, uint8_t* d_reason_hist,
                       int32_t* d_action_hist, float* d_logp_hist, float* d_value_hist) {
    if (!p || !h) return fail(BSK_EINVAL, "policy/handle is NULL");
    if (substeps < 1 || n_steps < 1) return fail(BSK_EINVAL, "substeps and n_steps must be >= 1");
    if (p->device != h->device) return fail(BSK_EINVAL, "bsk_policy_rollout: the policy and the handle live on different devices");
    int rc = check_act(p, "policy", 0, h->d_obs, h->ostride, h->n, (int64_t)h->env_base, mode, h->d_act, d_value_hist, nullptr, 0);
    if (rc) return rc;
    if ((rc = check_steppable(h))) return rc;
    if ((rc = check_stats(p, h))) return rc;
    DeviceGuard guard(h->device);
    if (!d_action_hist && p->act_cap < h->n) {
        rc = grow_scratch((void**)&p->d_act, &p->act_cap, (size_t)h->ostride * sizeof(int), h->stream,
                          "bsk_policy_rollout: the first rollout without d_action_hist allocates the policy's scratch row and "
                          "cannot be captured; make one such call outside the capture first");
        if (rc) return rc;
        p->act_cap = (int)h->ostride;
    }
    const RolloutHist hist = {d_obs_hist, d_reward_hist, d_reason_hist, d_action_hist, d_logp_hist, d_value_hist};
    return rollout_steps(p, 0, h, mode, substeps, n_steps, hist, p->d_act, nullptr, 0.0);
}

int bsk_population_create(const bsk_policy_spec* spec, int n_members, const float* params, int device_id, bsk_population** out) {
    bsk::PolicyLayout lay;
    int rc = create_begin(spec, out, lay);
    if (rc) return rc;
    if (n_members < 1 || n_members > (1 << 22)) return fail(BSK_EINVAL, "n_members must be in 1..2^22");
    return create_on_device(lay, device_id, out, bsk_population_destroy, [&](bsk_population* p) -> int {
        p->n_members = n_members;
        int rc = store_alloc(p);
        if (rc) return rc;
        if (params) return store_upload(p, params);
        HIP_TRY(hipMemset(p->d_params, 0, (size_t)n_members * (size_t)lay.n_device * sizeof(float)));   // (all-zero members pack to all-zero device blocks)
        HIP_SYNC(hipDeviceSynchronize());
        return BSK_OK;
    });
}

void bsk_population_destroy(bsk_population* p) {
    if (!p) return;
    DeviceGuard guard(p->device);
    free_all({p->d_params, p->d_rng, p->d_scratch, p->d_out_scratch});
    delete p;
}

int bsk_population_set_params(bsk_population* p, const float* params) {
    if (!p || !params) return fail(BSK_EINVAL, "population/params is NULL");
    DeviceGuard guard(p->device);
    return store_upload(p, params);
}

int bsk_population_set_params_device(bsk_population* p, const float* d_params, int first, int count, void* stream) {
    if (!p || !d_params) return fail(BSK_EINVAL, "population/d_params is NULL");
    if (first < 0 || count < 1 || first > p->n_members - count)
        return fail(BSK_EINVAL, "first / count must name members inside the population (first >= 0, count >= 1, first + count <= n_members)");
    DeviceGuard guard(p->device);
    HIP_TRY(bsk::launch_policy_pack(p->lay, d_params, p->d_params + (size_t)first * (size_t)p->lay.n_device, count, (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream`: no copy, no synchronisation
}

int bsk_population_get_member(bsk_population* p, int member, float* params) {
    if (!p || !params) return fail(BSK_EINVAL, "population/params is NULL");
    if (member < 0 || member >= p->n_members) return fail(BSK_EINVAL, "member must be in 0..n_members-1");
    DeviceGuard guard(p->device);
    std::vector<float> dev((size_t)p->lay.n_device);
    HIP_SYNC(hipDeviceSynchronize());
    HIP_COPY(hipMemcpy(dev.data(), p->d_params + (size_t)member * dev.size(), dev.size() * sizeof(float), hipMemcpyDeviceToHost));
    bsk::policy_unpack(p->lay, dev.data(), params);
    return BSK_OK;
}
int bsk_population_set_obs_stats(bsk_population* p, bsk_obs_stats* stats) { return attach_stats(p, "population is NULL", stats); }
int bsk_population_set_outcomes(bsk_population* p, double* d_rows) {
    if (!p) return fail(BSK_EINVAL, "population is NULL");
    p->d_outcomes = d_rows;
    return BSK_OK;
}
int bsk_population_set_obs_stats_members(bsk_population* p, int n_counted) {
    if (!p) return fail(BSK_EINVAL, "population is NULL");
    if (n_counted < 1 || n_counted > p->n_members) return fail(BSK_EINVAL, "bsk_population_set_obs_stats_members: n_counted must be in 1..n_members");
    p->n_counted = n_counted;
    return BSK_OK;
}
int bsk_population_set_rng(bsk_population* p, uint64_t seed, uint64_t draw) { return set_rng(p, "population is NULL", seed, draw); }
int bsk_population_get_rng(bsk_population* p, uint64_t* seed, uint64_t* draw) { return get_rng(p, "population is NULL", seed, draw); }

int bsk_population_act(bsk_population* p, const double* d_obs, int64_t obs_stride, int n, int envs_per_member, int64_t env_base, int mode,
                       int32_t* d_action, float* d_logp, float* d_value, float* d_logits, int64_t out_stride, void* stream) {
    if (envs_per_member == 0) envs_per_member = -1;       // (0 is check_act's "a policy": a caller's 0 breaks the member rule like every other non-multiple of 64)
    int rc = check_act(p, "population", envs_per_member, d_obs, obs_stride, n, env_base, mode, d_action, d_value, d_logits, out_stride);
    if (rc) return rc;
    DeviceGuard guard(p->device);
    return launch_act(p, envs_per_member, d_obs, obs_stride, n, env_base, mode, d_action, d_logp, d_value, d_logits, out_stride,
                      (hipStream_t)stream);
}

int bsk_population_rollout(bsk_population* p, bsk_handle* h, int mode, int substeps, int n_steps, double gamma,
                           double* d_obs_hist, double* d_reward_hist, uint8_t* d_reason_hist,
                           int32_t* d_action_hist, float* d_logp_hist, float* d_value_hist,
                           double* d_env_value, int32_t* d_env_len, double* d_fitness, double* d_mean_len) {
    if (!p || !h) return fail(BSK_EINVAL, "population/handle is NULL");
    if (substeps < 1 || n_steps < 1) return fail(BSK_EINVAL, "substeps and n_steps must be >= 1");
    if (!std::isfinite(gamma)) return fail(BSK_EINVAL, "gamma must be finite");
    if (p->device != h->device) return fail(BSK_EINVAL, "bsk_population_rollout: the population and the handle live on different devices");
    if (h->n % p->n_members != 0)
        return fail(BSK_EINVAL, "bsk_population_rollout: the handle's n_envs must be n_members * envs_per_member");
    const int E = h->n / p->n_members;                    // (>= 1: h->n is)
    int rc = check_act(p, "population", E, h->d_obs, h->ostride, h->n, (int64_t)h->env_base, mode, h->d_act, d_value_hist, nullptr, 0);
    if (rc) return rc;
    if ((rc = check_steppable(h))) return rc;
    if ((rc = check_stats(p, h))) return rc;
    DeviceGuard guard(h->device);
    if (p->scratch_cap < h->n) {
        const size_t n = (size_t)h->n;                          // (a multiple of 64: every row below starts 8-byte aligned)
        rc = grow_scratch(&p->d_scratch, &p->scratch_cap, n * (8 + 8 + 4 + 4 + 1), h->stream,
                          "bsk_population_rollout: the first rollout of a size allocates the population's scratch rows and "
                          "cannot be captured; make one such call outside the capture first");
        if (rc) return rc;
        char* at = (char*)p->d_scratch;
        p->acc.v = (double*)at; at += n * 8;
        p->acc.g = (double*)at; at += n * 8;
        p->acc.len = (int*)at; at += n * 4;
        p->d_act = (int*)at; at += n * 4;
        p->acc.alive = (unsigned char*)at;
        p->scratch_cap = h->n;
    }
    const bool outcomes = p->d_outcomes != nullptr;
    if (outcomes && p->out_cap < h->n) {
        const size_t n = (size_t)h->n;
        rc = grow_scratch(&p->d_out_scratch, &p->out_cap, n * (3 * 4 + 1), h->stream,
                          "bsk_population_rollout: the first rollout of a size with outcome rows attached allocates their accumulators "
                          "and cannot be captured; make one such call outside the capture first");
        if (rc) return rc;
        p->out.act_n = (int*)p->d_out_scratch;
        p->out.end_reason = (unsigned char*)p->d_out_scratch + n * 3 * 4;
        p->out_cap = h->n;
    }
    // the history rows and the value rule in ONE launch; with no fitness output asked for and no outcome rows attached, the rows
    // alone (or nothing)
    const bool want_fitness = d_env_value || d_env_len || d_fitness || d_mean_len;
    const RolloutHist hist = {d_obs_hist, d_reward_hist, d_reason_hist, d_action_hist, d_logp_hist, d_value_hist};
    rc = rollout_steps(p, E, h, mode, substeps, n_steps, hist, p->d_act, want_fitness || outcomes ? &p->acc : nullptr, gamma,
                       outcomes ? &p->out : nullptr);
    if (rc) return rc;
    HIP_TRY(bsk::launch_fitness_join(p->acc, p->n_members, E, d_env_value, d_env_len, d_fitness, d_mean_len, h->stream));
    if (outcomes) HIP_TRY(bsk::launch_outcome_join(p->acc, p->out, p->n_members, E, p->d_outcomes, h->stream));
    return BSK_OK;
}

int bsk_obs_stats_create(int n_cap, int device_id, bsk_obs_stats** out) {
    if (!out) return fail(BSK_EINVAL, "out is NULL");
    *out = nullptr;
    if (n_cap < 1 || n_cap > (1 << 28)) return fail(BSK_EINVAL, "bsk_obs_stats_create: n_cap must be in 1..2^28");
    int rc = open_device(device_id);
    if (rc) return rc;
    DeviceGuard guard(device_id);
    bsk_obs_stats* s = new bsk_obs_stats();
    s->device = device_id;
    s->n_cap = n_cap;
    s->st.waves = (n_cap + 63) / 64;
    const hipError_t e = hipMalloc(&s->d_block, s->words() * 8);
    if (e != hipSuccess) {
        delete s;
        return fail(e == hipErrorOutOfMemory ? BSK_ENOMEM : BSK_EHIP, std::string("bsk_obs_stats_create: ") + hipGetErrorString(e));
    }
    unsigned long long* at = (unsigned long long*)s->d_block;
    s->st.part = (double*)at; at += (size_t)s->st.waves * 10;
    s->st.cnt = at; at += (size_t)s->st.waves;
    s->st.tot = (double*)at; at += 10;
    s->st.tot_n = at;
    if ((rc = bsk_obs_stats_reset(s, nullptr)) == BSK_OK) {
        g_n_syncs.fetch_add(1, std::memory_order_relaxed);
        const hipError_t e2 = hipDeviceSynchronize();
        if (e2 != hipSuccess) rc = fail(BSK_EHIP, std::string("bsk_obs_stats_create: ") + hipGetErrorString(e2));
    }
    if (rc) { bsk_obs_stats_destroy(s); return rc; }
    *out = s;
    return BSK_OK;
}

void bsk_obs_stats_destroy(bsk_obs_stats* s) {
    if (!s) return;
    DeviceGuard guard(s->device);
    free_all({s->d_block});
    delete s;
}

int bsk_obs_stats_reset(bsk_obs_stats* s, void* stream) {
    if (!s) return fail(BSK_EINVAL, "stats is NULL");
    DeviceGuard guard(s->device);
    HIP_TRY(hipMemsetAsync(s->d_block, 0, s->words() * 8, (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream`: no copy, no synchronisation
}

int bsk_obs_stats_accumulate(bsk_obs_stats* s, const double* d_obs, int64_t obs_stride, int n, const uint8_t* d_alive, void* stream) {
    if (!s || !d_obs) return fail(BSK_EINVAL, "stats/d_obs is NULL");
    if (n < 1 || n > s->n_cap) return fail(BSK_EINVAL, "bsk_obs_stats_accumulate: n must be in 1..n_cap");
    if (obs_stride < n) return fail(BSK_EINVAL, "obs_stride must be >= n");
    DeviceGuard guard(s->device);
    HIP_TRY(bsk::launch_obs_stats(d_obs, obs_stride, n, d_alive, s->st, (hipStream_t)stream));
    HIP_TRY(bsk::launch_obs_stats_join(s->st, (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream`: no copy, no synchronisation
}

int bsk_obs_stats_get(bsk_obs_stats* s, uint64_t* count, double* mean5, double* var5) {
    if (!s) return fail(BSK_EINVAL, "stats is NULL");
    DeviceGuard guard(s->device);
    unsigned long long w[11];                              // tot[10] | tot_n: neighbours in the block
    HIP_SYNC(hipDeviceSynchronize());
    HIP_COPY(hipMemcpy(w, s->st.tot, sizeof w, hipMemcpyDeviceToHost));
    if (count) *count = w[10];
    for (int k = 0; k < 5; ++k) {
        double sum, sum_sq, mean = 0.0, var = 0.0;
        std::memcpy(&sum, &w[k], 8);
        std::memcpy(&sum_sq, &w[5 + k], 8);
        if (w[10] != 0ull) bsk::obs_moments_host(sum, sum_sq, w[10], &mean, &var);
        if (mean5) mean5[k] = mean;
        if (var5) var5[k] = var;
    }
    return BSK_OK;
}

int bsk_obs_stats_totals_device(bsk_obs_stats* s, const double** d_tot10, const uint64_t** d_count) {
    if (!s || !d_tot10 || !d_count) return fail(BSK_EINVAL, "stats/d_tot10/d_count is NULL");
    *d_tot10 = s->st.tot;
    *d_count = (const uint64_t*)s->st.tot_n;
    return BSK_OK;
}

int bsk_obs_stats_get_state(bsk_obs_stats* s, double* part, uint64_t* cnt) {
    if (!s) return fail(BSK_EINVAL, "stats is NULL");
    const size_t W = (size_t)s->st.waves;
    return transfer(s->device, hipMemcpyDeviceToHost, {{part, s->st.part, W * 10 * 8}, {cnt, s->st.cnt, W * 8}});
}

int bsk_obs_stats_set_state(bsk_obs_stats* s, const double* part, const uint64_t* cnt) {
    if (!s || !part || !cnt) return fail(BSK_EINVAL, "stats/part/cnt is NULL");
    DeviceGuard guard(s->device);
    const size_t W = (size_t)s->st.waves;
    int rc = transfer(s->device, hipMemcpyHostToDevice, {{part, s->st.part, W * 10 * 8}, {cnt, s->st.cnt, W * 8}});
    if (rc) return rc;
    HIP_TRY(bsk::launch_obs_stats_join(s->st, nullptr));  // the totals are a function of the partial rows: formed again
    HIP_SYNC(hipDeviceSynchronize());
    return BSK_OK;
}
}  // extern "C"
