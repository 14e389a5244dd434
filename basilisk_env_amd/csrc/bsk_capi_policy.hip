// bsk_capi_policy.hip — C-ABI of what drives an environment handle from the device: the fused MLP policy (bsk_policy_*), the
// population of policies (bsk_population_*), the evolution strategy (bsk_es_*) and the running observation statistics that give a
// policy its input normalisation (bsk_obs_stats_*).  Host side only, as bsk_capi.hip; kernels and launch wrappers: bsk_policy.hip,
// bsk_population.hip, bsk_es.hip, bsk_obsstats.hip.
#include <cmath>
#include <cstring>
#include <initializer_list>

#include "bsk_capi.hpp"
#include "bsk_es.hpp"
#include "bsk_obsstats.hpp"
#include "bsk_policy.hpp"
#include "bsk_population.hpp"

using namespace bsk::capi;

// bsk_obs_stats_*: sums, sums of squares and counts of the observation rows (kernels: bsk_obsstats.hip)
struct bsk_obs_stats {
    int device = 0;
    int n_cap = 0;
    void* d_block = nullptr;               // ONE allocation of 8-byte words: [part | cnt | tot | tot_n]
    bsk::ObsStats st = {};
    size_t words() const { return (size_t)st.waves * 11 + 11; }
};

namespace {

// What a policy and a population are alike in: n_members parameter blocks of one spec on one device (a policy: one block) and
// one draw counter for all of them
struct ParamStore {
    bsk::PolicyLayout lay;
    int device = 0;
    int n_members = 1;
    float* d_params = nullptr;             // [n_members][lay.n_device]: one device layout of the parameters (bsk_policy.hpp) per member
    unsigned long long* d_rng = nullptr;   // {seed, draw}: read by sample-mode launches, draw advanced behind each of them
    bsk_obs_stats* stats = nullptr;        // bsk_*_set_obs_stats: what the rollouts accumulate into; not owned
    int n_counted = 0;                     // bsk_population_set_obs_stats_members: the envs of the first n_counted members feed `stats`; 0: all
};

}  // namespace

// bsk_policy_*: the fused MLP policy (kernel and layout: bsk_policy.hip)
struct bsk_policy : ParamStore {
    int* d_act = nullptr;                  // bsk_policy_rollout's scratch row of actions (d_action_hist == NULL)
    int act_cap = 0;
};

// bsk_population_*: n_members parameter blocks of one spec, member m driving envs [m * E, (m + 1) * E) (bsk_policy.hip,
// bsk_population.hip)
struct bsk_population : ParamStore {
    // bsk_population_rollout's scratch, one allocation sized for the largest handle seen: the running value of every env and a
    // row of actions (d_action_hist == NULL)
    void* d_scratch = nullptr;
    bsk::FitnessAcc acc = {};
    int* d_act = nullptr;
    int scratch_cap = 0;
};

// bsk_es_*: the evolution strategy whose candidates never leave the device (bsk_es.hip)
struct bsk_es {
    bsk::PolicyLayout lay;
    int device = 0;
    int n_members = 0;
    double sigma = 0.0, lr = 0.0;
    int frozen = 0;
    unsigned long long* d_state = nullptr; // {seed, generation}: generation advanced behind every tell
    double* d_theta = nullptr;             // [lay.n_params]
    double* d_w = nullptr;                 // [w | q], n_members / 2 each: bsk_es_tell's scratch, the difference (and, under
                                           // BSK_ES_SIGMA_PGPE, the sum) of every pair's two utilities
    // bsk_es_set_optimizer: BSK_ES_SGD until Adam is selected; then ONE allocation [m | v | beta_pow] of 2 * n_params + 2 doubles
    int optimizer = BSK_ES_SGD;
    double beta1 = 0.0, beta2 = 0.0, eps = 0.0, weight_decay = 0.0;
    double* d_adam = nullptr;
    // bsk_es_set_sigma_adaptation: BSK_ES_SIGMA_FIXED until PGPE is selected; then sigma_vec [n_params]
    int sigma_kind = BSK_ES_SIGMA_FIXED;
    double lr_sigma = 0.0, max_change = 0.0, sigma_min = 0.0, sigma_max = 0.0;
    double* d_sigma = nullptr;
    // bsk_es_set_log: off until a capacity is given; then ONE allocation of 8-byte words
    // [log_gen C | log_row 8 C | best_fitness | best_generation | best_member, - | take, b | best_params ceil(n_params / 2)]
    int log_capacity = 0;
    unsigned long long* d_log = nullptr;
    const double* d_mean_len = nullptr;    // the caller's, bound by bsk_es_set_log; may be NULL
    hipStream_t last_stream = nullptr;     // of the last ask / tell / apply_obs_norm: what bsk_es_set_log asks about a capture
    // bsk_es_set_validation: off until n_val > 0; then ONE allocation of 8-byte words
    // [val_epoch V | val_gen C | val_row 4 C | val_best_fitness | val_best_generation | take, - | val_best_params ceil(n_params / 2)]
    int n_val = 0, val_capacity = 0;
    unsigned long long* d_val = nullptr;
    const double* d_val_len = nullptr;     // the caller's, f64[n_members + n_val], bound by bsk_es_set_validation; may be NULL
};

namespace {

int policy_spec_layout(const bsk_policy_spec* spec, bsk::PolicyLayout& lay) {
    if (!spec) return fail(BSK_EINVAL, "spec is NULL");
    if (spec->abi_version != BSK_ABI_VERSION || spec->struct_size != sizeof(bsk_policy_spec))
        return fail(BSK_EABI, "bsk_policy_spec abi_version / struct_size mismatch");
    if (const char* why = bsk::policy_layout(*spec, lay)) return fail(BSK_EINVAL, std::string("bsk_policy_spec: ") + why);
    return BSK_OK;
}

// The create skeleton of the three objects.  Its head: *out = NULL, then the spec's layout ...
template <class T>
int create_begin(const bsk_policy_spec* spec, T** out, bsk::PolicyLayout& lay) {
    if (!out) return fail(BSK_EINVAL, "out is NULL");
    *out = nullptr;
    return policy_spec_layout(spec, lay);
}

// ... and, behind the caller's own argument checks, its tail: admit the device, allocate through `init`, destroy what a failure leaves
template <class T, class Init>
int create_on_device(const bsk::PolicyLayout& lay, int device_id, T** out, void (*destroy)(T*), Init init) {
    int rc = open_device(device_id);
    if (rc) return rc;
    DeviceGuard guard(device_id);
    T* obj = new T();
    obj->lay = lay;
    obj->device = device_id;
    if ((rc = init(obj))) { destroy(obj); return rc; }
    *out = obj;
    return BSK_OK;
}

// The destroy rule: what is queued on the device may still use the buffers - wait for it once if there is any, then free them
void free_all(std::initializer_list<void*> bufs) {
    bool any = false;
    for (void* b : bufs) any = any || b;
    if (any) (void)hipDeviceSynchronize();
    for (void* b : bufs)
        if (b) (void)hipFree(b);
}

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
    DeviceGuard guard(p->device);
    const unsigned long long w[2] = {seed, draw};
    HIP_SYNC(hipDeviceSynchronize());
    HIP_COPY(hipMemcpy(p->d_rng, w, sizeof w, hipMemcpyHostToDevice));
    return BSK_OK;
}

int get_rng(ParamStore* p, const char* null_msg, uint64_t* seed, uint64_t* draw) {
    if (!p) return fail(BSK_EINVAL, null_msg);
    DeviceGuard guard(p->device);
    unsigned long long w[2];
    HIP_SYNC(hipDeviceSynchronize());
    HIP_COPY(hipMemcpy(w, p->d_rng, sizeof w, hipMemcpyDeviceToHost));
    if (seed) *seed = w[0];
    if (draw) *draw = w[1];
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
// With a statistics object attached, the observations each launch of the policy reads are accumulated in front of it - under `acc`
// those of the envs still alive, as the previous step's launch of the value rule left them - and joined once behind the last step.
int rollout_steps(ParamStore* p, int envs_per_member, bsk_handle* h, int mode, int substeps, int n_steps, const RolloutHist& hist,
                  int32_t* d_act, const bsk::FitnessAcc* acc, double gamma) {
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
        if (acc)
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
    free_all({p->d_params, p->d_rng, p->d_scratch});
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
    // the history rows and the value rule in ONE launch; with no fitness output asked for, the rows alone (or nothing)
    const bool want_fitness = d_env_value || d_env_len || d_fitness || d_mean_len;
    const RolloutHist hist = {d_obs_hist, d_reward_hist, d_reason_hist, d_action_hist, d_logp_hist, d_value_hist};
    if ((rc = rollout_steps(p, E, h, mode, substeps, n_steps, hist, p->d_act, want_fitness ? &p->acc : nullptr, gamma))) return rc;
    HIP_TRY(bsk::launch_fitness_join(p->acc, p->n_members, E, d_env_value, d_env_len, d_fitness, d_mean_len, h->stream));
    return BSK_OK;
}

int bsk_es_create(const bsk_policy_spec* spec, int n_members, const float* theta, double sigma, double lr, int frozen, uint64_t seed,
                  int device_id, bsk_es** out) {
    bsk::PolicyLayout lay;
    int rc = create_begin(spec, out, lay);
    if (rc) return rc;
    if (n_members < 2 || n_members > 65536 || n_members % 2 != 0)
        return fail(BSK_EINVAL, "bsk_es_create: n_members must be even and in 2..65536 (the ranking compares every pair of members)");
    if (!std::isfinite(sigma) || !(sigma > 0.0)) return fail(BSK_EINVAL, "bsk_es_create: sigma must be finite and positive");
    if (!std::isfinite(lr)) return fail(BSK_EINVAL, "bsk_es_create: lr must be finite");
    if (frozen < 0 || frozen > lay.n_params) return fail(BSK_EINVAL, "bsk_es_create: frozen must be in 0..n_params");
    return create_on_device(lay, device_id, out, bsk_es_destroy, [&](bsk_es* es) -> int {
        es->n_members = n_members;
        es->sigma = sigma;
        es->lr = lr;
        es->frozen = frozen;
        const unsigned long long state0[2] = {seed, 0ull};
        std::vector<double> theta0((size_t)lay.n_params, 0.0);
        if (theta)
            for (int j = 0; j < lay.n_params; ++j) theta0[(size_t)j] = (double)theta[j];
        HIP_TRY(hipMalloc(&es->d_state, sizeof state0));
        HIP_TRY(hipMalloc(&es->d_theta, theta0.size() * sizeof(double)));
        HIP_TRY(hipMalloc(&es->d_w, (size_t)n_members * sizeof(double)));
        HIP_COPY(hipMemcpy(es->d_state, state0, sizeof state0, hipMemcpyHostToDevice));
        HIP_COPY(hipMemcpy(es->d_theta, theta0.data(), theta0.size() * sizeof(double), hipMemcpyHostToDevice));
        return BSK_OK;
    });
}

void bsk_es_destroy(bsk_es* es) {
    if (!es) return;
    DeviceGuard guard(es->device);
    free_all({es->d_state, es->d_theta, es->d_w, es->d_adam, es->d_sigma, es->d_log, es->d_val});
    delete es;
}

static bsk::EsArgs es_args(const bsk_es* es) {
    bsk::EsArgs a;
    a.state = es->d_state;
    a.theta = es->d_theta;
    a.sigma = es->sigma;
    a.frozen = es->frozen;
    a.pairs = es->n_members / 2;
    return a;
}

static bsk::EsSigma es_sigma(const bsk_es* es) {
    bsk::EsSigma sv;
    sv.sigma_vec = es->d_sigma;
    sv.pd = (double)es->n_members;
    sv.cs = es->lr_sigma / sv.pd;
    sv.max_change = es->max_change;
    sv.sigma_min = es->sigma_min;
    sv.sigma_max = es->sigma_max;
    return sv;
}

// the words of the log's allocation and the views of them the kernels take
static size_t es_log_words(const bsk_es* es, int capacity) { return 9 * (size_t)capacity + 4 + ((size_t)es->lay.n_params + 1) / 2; }

static bsk::EsLog es_log(const bsk_es* es) {
    const size_t C = (size_t)es->log_capacity;
    unsigned long long* tail = es->d_log + 9 * C;
    bsk::EsLog lg;
    lg.gen = es->d_log;
    lg.row = (double*)(es->d_log + C);
    lg.best_fitness = (double*)tail;
    lg.best_generation = tail + 1;
    lg.best_member = (int*)(tail + 2);
    lg.cand = (int*)(tail + 3);
    lg.best_params = (float*)(tail + 4);
    lg.mean_len = es->d_mean_len;
    lg.capacity = es->log_capacity;
    return lg;
}

// the words of the validation's allocation and the views of them the kernels take
static size_t es_val_words(const bsk_es* es, int n_val, int capacity) {
    return (size_t)n_val + 5 * (size_t)capacity + 3 + ((size_t)es->lay.n_params + 1) / 2;
}

static bsk::EsVal es_val(const bsk_es* es) {
    const size_t C = (size_t)es->val_capacity;
    unsigned long long* ring = es->d_val + (size_t)es->n_val;
    unsigned long long* tail = ring + 5 * C;
    bsk::EsVal vl;
    vl.gen = ring;
    vl.row = (double*)(ring + C);
    vl.best_fitness = (double*)tail;
    vl.best_generation = tail + 1;
    vl.cand = (int*)(tail + 2);
    vl.best_params = (float*)(tail + 3);
    vl.mean_len = es->d_val_len;
    vl.capacity = es->val_capacity;
    vl.n_val = es->n_val;
    return vl;
}

// (the optimiser serves one stream at a time: the stream of its last launch is the one a capture of its loop records)
static bool es_stream_capturing(bsk_es* es) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (es->last_stream && hipStreamIsCapturing(es->last_stream, &st) != hipSuccess) {
        (void)hipGetLastError();                          // (a stream that has been destroyed since captures nothing)
        st = hipStreamCaptureStatusNone;
        es->last_stream = nullptr;
    }
    return st != hipStreamCaptureStatusNone;
}

int bsk_es_ask(bsk_es* es, bsk_population* pop, void* stream) {
    if (!es || !pop) return fail(BSK_EINVAL, "es/population is NULL");
    if (pop->n_members != es->n_members + es->n_val)
        return fail(BSK_EINVAL, es->n_val > 0 ? "bsk_es_ask: the population's n_members differs from the optimiser's n_members + n_val (bsk_es_set_validation)"
                                              : "bsk_es_ask: the population's n_members differs from the optimiser's");
    if (std::memcmp(&pop->lay, &es->lay, sizeof(bsk::PolicyLayout)) != 0)      // (all-int, value-initialised: policy_layout)
        return fail(BSK_EINVAL, "bsk_es_ask: the population's spec differs from the optimiser's");
    if (pop->device != es->device) return fail(BSK_EINVAL, "bsk_es_ask: the optimiser and the population live on different devices");
    DeviceGuard guard(es->device);
    es->last_stream = (hipStream_t)stream;
    if (es->sigma_kind == BSK_ES_SIGMA_PGPE)
        HIP_TRY(bsk::launch_es_ask_sigma(es->lay, es_args(es), es->d_sigma, pop->d_params, (hipStream_t)stream));
    else
        HIP_TRY(bsk::launch_es_ask(es->lay, es_args(es), pop->d_params, (hipStream_t)stream));
    if (es->n_val > 0)                                    // the centre into the members behind ask's: member-major, so the launch above is the one it was
        HIP_TRY(bsk::launch_es_center(es->lay, es->d_theta, pop->d_params + (size_t)es->n_members * (size_t)es->lay.n_device, es->n_val,
                                      (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream`: no copy, no synchronisation
}

int bsk_es_tell(bsk_es* es, const double* d_fitness, void* stream) {
    if (!es || !d_fitness) return fail(BSK_EINVAL, "es/d_fitness is NULL");
    DeviceGuard guard(es->device);
    const bool pgpe = es->sigma_kind == BSK_ES_SIGMA_PGPE;
    double* d_q = es->d_w + es->n_members / 2;
    es->last_stream = (hipStream_t)stream;
    if (es->log_capacity > 0)                             // in front of the update: theta, sigma_vec and the generation as ask read them
        HIP_TRY(bsk::launch_es_log(es_args(es), pgpe ? es->d_sigma : nullptr, es->lay.n_params, d_fitness, es_log(es), (hipStream_t)stream));
    if (es->n_val > 0)                                    // behind the log's two, in front of the update too: f[P .. P + V - 1]
        HIP_TRY(bsk::launch_es_validate(es_args(es), es->lay.n_params, d_fitness, es_val(es), (hipStream_t)stream));
    if (pgpe)
        HIP_TRY(bsk::launch_es_rank_q(d_fitness, es->n_members, es->d_w, d_q, (hipStream_t)stream));
    else
        HIP_TRY(bsk::launch_es_rank(d_fitness, es->n_members, es->d_w, (hipStream_t)stream));
    if (es->optimizer == BSK_ES_ADAM) {
        const size_t np = (size_t)es->lay.n_params;
        bsk::EsAdam ad;
        ad.m = es->d_adam;
        ad.v = es->d_adam + np;
        ad.beta_pow = es->d_adam + 2 * np;
        ad.beta1 = es->beta1; ad.beta2 = es->beta2;
        ad.a1 = 1.0 - es->beta1; ad.a2 = 1.0 - es->beta2;
        ad.eps = es->eps; ad.weight_decay = es->weight_decay;
        ad.cg = 1.0 / ((double)es->n_members * es->sigma);
        ad.lr = es->lr;
        if (pgpe)
            HIP_TRY(bsk::launch_es_tell_adam_sigma(es_args(es), es->lay.n_params, es->d_w, d_q, ad, es_sigma(es), (hipStream_t)stream));
        else
            HIP_TRY(bsk::launch_es_tell_adam(es_args(es), es->lay.n_params, es->d_w, ad, (hipStream_t)stream));
        HIP_TRY(bsk::launch_es_advance_adam(es->d_state, es->d_adam + 2 * np, es->beta1, es->beta2, (hipStream_t)stream));
        return BSK_OK;
    }
    if (pgpe) {
        HIP_TRY(bsk::launch_es_tell_sigma(es_args(es), es->lay.n_params, es->d_w, d_q, es->lr, es_sigma(es), (hipStream_t)stream));
    } else {
        const double c = es->lr / ((double)es->n_members * es->sigma);
        HIP_TRY(bsk::launch_es_tell(es_args(es), es->lay.n_params, es->d_w, c, (hipStream_t)stream));
    }
    HIP_TRY(bsk::launch_es_advance(es->d_state, (hipStream_t)stream));
    return BSK_OK;
}

int bsk_es_get_state(bsk_es* es, double* theta, uint64_t* generation) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    DeviceGuard guard(es->device);
    HIP_SYNC(hipDeviceSynchronize());
    if (theta) HIP_COPY(hipMemcpy(theta, es->d_theta, (size_t)es->lay.n_params * sizeof(double), hipMemcpyDeviceToHost));
    if (generation) {
        unsigned long long w[2];
        HIP_COPY(hipMemcpy(w, es->d_state, sizeof w, hipMemcpyDeviceToHost));
        *generation = w[1];
    }
    return BSK_OK;
}

int bsk_es_set_state(bsk_es* es, const double* theta, uint64_t generation) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    DeviceGuard guard(es->device);
    const unsigned long long g = generation;
    HIP_SYNC(hipDeviceSynchronize());                     // (queued launches still read the old state)
    if (theta) HIP_COPY(hipMemcpy(es->d_theta, theta, (size_t)es->lay.n_params * sizeof(double), hipMemcpyHostToDevice));
    HIP_COPY(hipMemcpy(es->d_state + 1, &g, sizeof g, hipMemcpyHostToDevice));
    return BSK_OK;
}

int bsk_es_generation_device(bsk_es* es, const uint64_t** d_generation) {
    if (!es || !d_generation) return fail(BSK_EINVAL, "es/d_generation is NULL");
    *d_generation = (const uint64_t*)(es->d_state + 1);
    return BSK_OK;
}

int bsk_es_set_optimizer(bsk_es* es, int kind, double beta1, double beta2, double eps, double weight_decay) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    if (kind != BSK_ES_SGD && kind != BSK_ES_ADAM) return fail(BSK_EINVAL, "bsk_es_set_optimizer: kind must be BSK_ES_SGD or BSK_ES_ADAM");
    if (kind == BSK_ES_ADAM) {
        if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
            return fail(BSK_EINVAL, "bsk_es_set_optimizer: beta1 and beta2 must be in [0, 1)");
        if (!std::isfinite(eps) || !(eps > 0.0)) return fail(BSK_EINVAL, "bsk_es_set_optimizer: eps must be finite and positive");
        if (!std::isfinite(weight_decay) || weight_decay < 0.0)
            return fail(BSK_EINVAL, "bsk_es_set_optimizer: weight_decay must be finite and not negative");
    }
    DeviceGuard guard(es->device);
    HIP_SYNC(hipDeviceSynchronize());                     // (queued tells still use the old rule and the old moments)
    if (kind == BSK_ES_SGD) {
        es->optimizer = BSK_ES_SGD;
        return BSK_OK;
    }
    const size_t np = (size_t)es->lay.n_params;
    if (!es->d_adam) HIP_TRY(hipMalloc(&es->d_adam, (2 * np + 2) * sizeof(double)));
    const double one[2] = {1.0, 1.0};
    HIP_TRY(hipMemset(es->d_adam, 0, 2 * np * sizeof(double)));
    HIP_COPY(hipMemcpy(es->d_adam + 2 * np, one, sizeof one, hipMemcpyHostToDevice));
    es->optimizer = BSK_ES_ADAM;
    es->beta1 = beta1; es->beta2 = beta2; es->eps = eps; es->weight_decay = weight_decay;
    return BSK_OK;
}

int bsk_es_get_moments(bsk_es* es, double* m, double* v, double* beta_pow) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    if (es->optimizer != BSK_ES_ADAM) return fail(BSK_EINVAL, "bsk_es_get_moments: the optimiser is BSK_ES_SGD, it has no moments");
    DeviceGuard guard(es->device);
    const size_t np = (size_t)es->lay.n_params;
    HIP_SYNC(hipDeviceSynchronize());
    if (m) HIP_COPY(hipMemcpy(m, es->d_adam, np * sizeof(double), hipMemcpyDeviceToHost));
    if (v) HIP_COPY(hipMemcpy(v, es->d_adam + np, np * sizeof(double), hipMemcpyDeviceToHost));
    if (beta_pow) HIP_COPY(hipMemcpy(beta_pow, es->d_adam + 2 * np, 2 * sizeof(double), hipMemcpyDeviceToHost));
    return BSK_OK;
}

int bsk_es_set_moments(bsk_es* es, const double* m, const double* v, const double* beta_pow) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    if (es->optimizer != BSK_ES_ADAM) return fail(BSK_EINVAL, "bsk_es_set_moments: the optimiser is BSK_ES_SGD, it has no moments");
    DeviceGuard guard(es->device);
    const size_t np = (size_t)es->lay.n_params;
    HIP_SYNC(hipDeviceSynchronize());                     // (queued launches still read the old moments)
    if (m) HIP_COPY(hipMemcpy(es->d_adam, m, np * sizeof(double), hipMemcpyHostToDevice));
    if (v) HIP_COPY(hipMemcpy(es->d_adam + np, v, np * sizeof(double), hipMemcpyHostToDevice));
    if (beta_pow) HIP_COPY(hipMemcpy(es->d_adam + 2 * np, beta_pow, 2 * sizeof(double), hipMemcpyHostToDevice));
    return BSK_OK;
}

int bsk_es_set_sigma_adaptation(bsk_es* es, int kind, double lr_sigma, double max_change, double sigma_min, double sigma_max) {
    const char* const fn = "bsk_es_set_sigma_adaptation: ";
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    if (kind != BSK_ES_SIGMA_FIXED && kind != BSK_ES_SIGMA_PGPE)
        return fail(BSK_EINVAL, std::string(fn) + "kind must be BSK_ES_SIGMA_FIXED or BSK_ES_SIGMA_PGPE");
    if (kind == BSK_ES_SIGMA_PGPE) {
        if (!std::isfinite(lr_sigma) || lr_sigma < 0.0) return fail(BSK_EINVAL, std::string(fn) + "lr_sigma must be finite and not negative");
        if (!std::isfinite(max_change) || !(max_change > 0.0 && max_change < 1.0))
            return fail(BSK_EINVAL, std::string(fn) + "max_change must be inside (0, 1)");
        if (!std::isfinite(sigma_min) || !(sigma_min > 0.0)) return fail(BSK_EINVAL, std::string(fn) + "sigma_min must be finite and positive");
        if (!std::isfinite(sigma_max) || sigma_max < sigma_min)
            return fail(BSK_EINVAL, std::string(fn) + "sigma_max must be finite and not below sigma_min");
        if (es->sigma < sigma_min || es->sigma > sigma_max)
            return fail(BSK_EINVAL, std::string(fn) + "the sigma of bsk_es_create must be inside [sigma_min, sigma_max]");
    }
    DeviceGuard guard(es->device);
    HIP_SYNC(hipDeviceSynchronize());                     // (queued asks and tells still use the old rule and the old vector)
    if (kind == BSK_ES_SIGMA_FIXED) {
        es->sigma_kind = BSK_ES_SIGMA_FIXED;
        return BSK_OK;
    }
    const size_t np = (size_t)es->lay.n_params;
    if (!es->d_sigma) HIP_TRY(hipMalloc(&es->d_sigma, np * sizeof(double)));
    const std::vector<double> fill(np, es->sigma);
    HIP_COPY(hipMemcpy(es->d_sigma, fill.data(), np * sizeof(double), hipMemcpyHostToDevice));
    es->sigma_kind = BSK_ES_SIGMA_PGPE;
    es->lr_sigma = lr_sigma; es->max_change = max_change; es->sigma_min = sigma_min; es->sigma_max = sigma_max;
    return BSK_OK;
}

int bsk_es_get_sigma(bsk_es* es, double* sigma) {
    if (!es || !sigma) return fail(BSK_EINVAL, "es/sigma is NULL");
    if (es->sigma_kind != BSK_ES_SIGMA_PGPE) return fail(BSK_EINVAL, "bsk_es_get_sigma: the kind is BSK_ES_SIGMA_FIXED, there is no vector");
    DeviceGuard guard(es->device);
    HIP_SYNC(hipDeviceSynchronize());
    HIP_COPY(hipMemcpy(sigma, es->d_sigma, (size_t)es->lay.n_params * sizeof(double), hipMemcpyDeviceToHost));
    return BSK_OK;
}

int bsk_es_set_sigma(bsk_es* es, const double* sigma) {
    if (!es || !sigma) return fail(BSK_EINVAL, "es/sigma is NULL");
    if (es->sigma_kind != BSK_ES_SIGMA_PGPE) return fail(BSK_EINVAL, "bsk_es_set_sigma: the kind is BSK_ES_SIGMA_FIXED, there is no vector");
    for (int j = 0; j < es->lay.n_params; ++j)
        if (!std::isfinite(sigma[j]) || !(sigma[j] > 0.0)) return fail(BSK_EINVAL, "bsk_es_set_sigma: every entry must be finite and positive");
    DeviceGuard guard(es->device);
    HIP_SYNC(hipDeviceSynchronize());                     // (queued launches still read the old vector)
    HIP_COPY(hipMemcpy(es->d_sigma, sigma, (size_t)es->lay.n_params * sizeof(double), hipMemcpyHostToDevice));
    return BSK_OK;
}

int bsk_es_set_log(bsk_es* es, int capacity, const double* d_mean_len) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    if (capacity < 0) return fail(BSK_EINVAL, "bsk_es_set_log: capacity must not be negative");
    DeviceGuard guard(es->device);
    if (es_stream_capturing(es))
        return fail(BSK_EINVAL, "bsk_es_set_log: the optimiser's stream is being captured; it allocates and synchronises and cannot be captured");
    HIP_SYNC(hipDeviceSynchronize());                     // (queued tells still write the old log)
    if (es->d_log) {
        (void)hipFree(es->d_log);
        es->d_log = nullptr;
    }
    es->log_capacity = 0;
    es->d_mean_len = nullptr;
    if (capacity == 0) return BSK_OK;
    const size_t C = (size_t)capacity, words = es_log_words(es, capacity);
    HIP_TRY(hipMalloc(&es->d_log, words * 8));
    HIP_TRY(hipMemset(es->d_log, 0xff, C * 8));                                    // log_gen: all ones
    HIP_TRY(hipMemset(es->d_log + C, 0, (words - C) * 8));                           // log_row, best_params, the candidate words
    const unsigned long long tail[3] = {0x7ff8000000000000ull, ~0ull, 0xffffffffull};   // a NaN, all ones, member -1
    HIP_COPY(hipMemcpy(es->d_log + 9 * C, tail, sizeof tail, hipMemcpyHostToDevice));
    es->log_capacity = capacity;
    es->d_mean_len = d_mean_len;
    return BSK_OK;
}

int bsk_es_get_log(bsk_es* es, uint64_t* gen, double* rows) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    if (es->log_capacity < 1) return fail(BSK_EINVAL, "bsk_es_get_log: the optimiser has no log (bsk_es_set_log)");
    DeviceGuard guard(es->device);
    const size_t C = (size_t)es->log_capacity;
    HIP_SYNC(hipDeviceSynchronize());
    if (gen) HIP_COPY(hipMemcpy(gen, es->d_log, C * 8, hipMemcpyDeviceToHost));
    if (rows) HIP_COPY(hipMemcpy(rows, es->d_log + C, 8 * C * 8, hipMemcpyDeviceToHost));
    return BSK_OK;
}

int bsk_es_get_best(bsk_es* es, float* params, double* fitness, uint64_t* generation, int32_t* member) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    if (es->log_capacity < 1) return fail(BSK_EINVAL, "bsk_es_get_best: the optimiser has no log (bsk_es_set_log)");
    DeviceGuard guard(es->device);
    const bsk::EsLog lg = es_log(es);
    HIP_SYNC(hipDeviceSynchronize());
    if (params) HIP_COPY(hipMemcpy(params, lg.best_params, (size_t)es->lay.n_params * sizeof(float), hipMemcpyDeviceToHost));
    if (fitness) HIP_COPY(hipMemcpy(fitness, lg.best_fitness, 8, hipMemcpyDeviceToHost));
    if (generation) HIP_COPY(hipMemcpy(generation, lg.best_generation, 8, hipMemcpyDeviceToHost));
    if (member) HIP_COPY(hipMemcpy(member, lg.best_member, 4, hipMemcpyDeviceToHost));
    return BSK_OK;
}

int bsk_es_set_best(bsk_es* es, const float* params, const double* fitness, const uint64_t* generation, const int32_t* member) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    if (es->log_capacity < 1) return fail(BSK_EINVAL, "bsk_es_set_best: the optimiser has no log (bsk_es_set_log)");
    DeviceGuard guard(es->device);
    const bsk::EsLog lg = es_log(es);
    HIP_SYNC(hipDeviceSynchronize());                     // (queued tells still read and write the old champion)
    if (params) HIP_COPY(hipMemcpy(lg.best_params, params, (size_t)es->lay.n_params * sizeof(float), hipMemcpyHostToDevice));
    if (fitness) HIP_COPY(hipMemcpy(lg.best_fitness, fitness, 8, hipMemcpyHostToDevice));
    if (generation) HIP_COPY(hipMemcpy(lg.best_generation, generation, 8, hipMemcpyHostToDevice));
    if (member) HIP_COPY(hipMemcpy(lg.best_member, member, 4, hipMemcpyHostToDevice));
    return BSK_OK;
}

int bsk_es_best_device(bsk_es* es, const float** d_params) {
    if (!es || !d_params) return fail(BSK_EINVAL, "es/d_params is NULL");
    if (es->log_capacity < 1) return fail(BSK_EINVAL, "bsk_es_best_device: the optimiser has no log (bsk_es_set_log)");
    *d_params = es_log(es).best_params;
    return BSK_OK;
}

int bsk_es_set_validation(bsk_es* es, int n_val, int capacity, uint64_t epoch0, const double* d_mean_len) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    if (n_val < 0 || n_val > 16) return fail(BSK_EINVAL, "bsk_es_set_validation: n_val must be in 0..16");
    if (n_val > 0 && capacity < 1) return fail(BSK_EINVAL, "bsk_es_set_validation: capacity must be >= 1");
    DeviceGuard guard(es->device);
    if (es_stream_capturing(es))
        return fail(BSK_EINVAL, "bsk_es_set_validation: the optimiser's stream is being captured; it allocates and synchronises and cannot be captured");
    HIP_SYNC(hipDeviceSynchronize());                     // (queued asks and tells still use the old state)
    if (es->d_val) {
        (void)hipFree(es->d_val);
        es->d_val = nullptr;
    }
    es->n_val = es->val_capacity = 0;
    es->d_val_len = nullptr;
    if (n_val == 0) return BSK_OK;
    const size_t V = (size_t)n_val, C = (size_t)capacity, words = es_val_words(es, n_val, capacity);
    std::vector<unsigned long long> head(V);
    for (size_t v = 0; v < V; ++v) head[v] = epoch0 + v;
    HIP_TRY(hipMalloc(&es->d_val, words * 8));
    HIP_COPY(hipMemcpy(es->d_val, head.data(), V * 8, hipMemcpyHostToDevice));          // val_epoch
    HIP_TRY(hipMemset(es->d_val + V, 0xff, C * 8));                                      // val_gen: all ones
    HIP_TRY(hipMemset(es->d_val + V + C, 0, (words - V - C) * 8));                       // val_row, val_best_params, the candidate word
    const unsigned long long tail[2] = {0x7ff8000000000000ull, ~0ull};                   // a NaN, all ones
    HIP_COPY(hipMemcpy(es->d_val + V + 5 * C, tail, sizeof tail, hipMemcpyHostToDevice));
    HIP_SYNC(hipDeviceSynchronize());
    es->n_val = n_val;
    es->val_capacity = capacity;
    es->d_val_len = d_mean_len;
    return BSK_OK;
}

int bsk_es_get_validation_log(bsk_es* es, uint64_t* gen, double* rows) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    if (es->n_val < 1) return fail(BSK_EINVAL, "bsk_es_get_validation_log: validation is off (bsk_es_set_validation)");
    DeviceGuard guard(es->device);
    const bsk::EsVal vl = es_val(es);
    const size_t C = (size_t)es->val_capacity;
    HIP_SYNC(hipDeviceSynchronize());
    if (gen) HIP_COPY(hipMemcpy(gen, vl.gen, C * 8, hipMemcpyDeviceToHost));
    if (rows) HIP_COPY(hipMemcpy(rows, vl.row, 4 * C * 8, hipMemcpyDeviceToHost));
    return BSK_OK;
}

int bsk_es_get_validated_best(bsk_es* es, float* params, double* fitness, uint64_t* generation) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    if (es->n_val < 1) return fail(BSK_EINVAL, "bsk_es_get_validated_best: validation is off (bsk_es_set_validation)");
    DeviceGuard guard(es->device);
    const bsk::EsVal vl = es_val(es);
    HIP_SYNC(hipDeviceSynchronize());
    if (params) HIP_COPY(hipMemcpy(params, vl.best_params, (size_t)es->lay.n_params * sizeof(float), hipMemcpyDeviceToHost));
    if (fitness) HIP_COPY(hipMemcpy(fitness, vl.best_fitness, 8, hipMemcpyDeviceToHost));
    if (generation) HIP_COPY(hipMemcpy(generation, vl.best_generation, 8, hipMemcpyDeviceToHost));
    return BSK_OK;
}

int bsk_es_set_validated_best(bsk_es* es, const float* params, const double* fitness, const uint64_t* generation) {
    if (!es) return fail(BSK_EINVAL, "es is NULL");
    if (es->n_val < 1) return fail(BSK_EINVAL, "bsk_es_set_validated_best: validation is off (bsk_es_set_validation)");
    DeviceGuard guard(es->device);
    const bsk::EsVal vl = es_val(es);
    HIP_SYNC(hipDeviceSynchronize());                     // (queued tells still read and write the old champion)
    if (params) HIP_COPY(hipMemcpy(vl.best_params, params, (size_t)es->lay.n_params * sizeof(float), hipMemcpyHostToDevice));
    if (fitness) HIP_COPY(hipMemcpy(vl.best_fitness, fitness, 8, hipMemcpyHostToDevice));
    if (generation) HIP_COPY(hipMemcpy(vl.best_generation, generation, 8, hipMemcpyHostToDevice));
    return BSK_OK;
}

int bsk_es_validated_best_device(bsk_es* es, const float** d_params) {
    if (!es || !d_params) return fail(BSK_EINVAL, "es/d_params is NULL");
    if (es->n_val < 1) return fail(BSK_EINVAL, "bsk_es_validated_best_device: validation is off (bsk_es_set_validation)");
    *d_params = es_val(es).best_params;
    return BSK_OK;
}

int bsk_es_validation_epochs_device(bsk_es* es, const uint64_t** d_epochs) {
    if (!es || !d_epochs) return fail(BSK_EINVAL, "es/d_epochs is NULL");
    if (es->n_val < 1) return fail(BSK_EINVAL, "bsk_es_validation_epochs_device: validation is off (bsk_es_set_validation)");
    *d_epochs = (const uint64_t*)es->d_val;
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
    DeviceGuard guard(s->device);
    HIP_SYNC(hipDeviceSynchronize());
    if (part) HIP_COPY(hipMemcpy(part, s->st.part, (size_t)s->st.waves * 10 * 8, hipMemcpyDeviceToHost));
    if (cnt) HIP_COPY(hipMemcpy(cnt, s->st.cnt, (size_t)s->st.waves * 8, hipMemcpyDeviceToHost));
    return BSK_OK;
}

int bsk_obs_stats_set_state(bsk_obs_stats* s, const double* part, const uint64_t* cnt) {
    if (!s || !part || !cnt) return fail(BSK_EINVAL, "stats/part/cnt is NULL");
    DeviceGuard guard(s->device);
    HIP_SYNC(hipDeviceSynchronize());                     // (queued launches still read and write the old state)
    HIP_COPY(hipMemcpy(s->st.part, part, (size_t)s->st.waves * 10 * 8, hipMemcpyHostToDevice));
    HIP_COPY(hipMemcpy(s->st.cnt, cnt, (size_t)s->st.waves * 8, hipMemcpyHostToDevice));
    HIP_TRY(bsk::launch_obs_stats_join(s->st, nullptr));  // the totals are a function of the partial rows: formed again
    HIP_SYNC(hipDeviceSynchronize());
    return BSK_OK;
}

int bsk_es_apply_obs_norm(bsk_es* es, bsk_obs_stats* s, double std_min, void* stream) {
    if (!es || !s) return fail(BSK_EINVAL, "es/stats is NULL");
    if (es->frozen < 10)
        return fail(BSK_EINVAL, "bsk_es_apply_obs_norm: frozen must be >= 10 (in_scale and in_shift would be perturbed and moved by the search)");
    if (!std::isfinite(std_min) || !(std_min > 0.0)) return fail(BSK_EINVAL, "bsk_es_apply_obs_norm: std_min must be finite and positive");
    if (es->device != s->device) return fail(BSK_EINVAL, "bsk_es_apply_obs_norm: the optimiser and the statistics live on different devices");
    DeviceGuard guard(es->device);
    es->last_stream = (hipStream_t)stream;
    HIP_TRY(bsk::launch_es_obs_norm(s->st.tot, s->st.tot_n, std_min, es->d_theta, (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream`: no copy, no synchronisation
}
}  // extern "C"
