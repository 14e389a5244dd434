// bsk_capi_fit.hip — C-ABI of the supervised fit of a policy to labelled observations (bsk_fit_*): accumulate block gradients of a
// cross-entropy (and, optionally, a squared value error) from device buffers, then one Adam step into the attached policy's own
// parameters; the same with a clipped policy-gradient loss in the cross-entropy's place (bsk_fit_accumulate_pg), and the advantage
// estimator that feeds it from rollout histories (bsk_gae); PPO2's clipped value loss on top of that (bsk_fit_accumulate_ppo) and the
// shuffled minibatches it is fed (bsk_pg_gather, bsk_pg_shuffle_advance; kernels: bsk_shuffle.hip); the training log of the loop over
// them (bsk_pg_episodes, bsk_pg_log_update, bsk_pg_log_advance; kernels: bsk_pglog.hip); the rewards of a rollout scaled by the
// running deviation of the discounted return (bsk_reward_norm; kernels: bsk_rewnorm.hip); schedules of lr, clip, clip_vf and ent_coef
// and a KL stop per update, carried in eight device words of the fit (bsk_fit_set_schedule, bsk_fit_schedule_begin, bsk_fit_kl_gate,
// bsk_fit_schedule_end; kernels: bsk_pgsched.hip, and the scheduled instantiations in bsk_fit.hip).  Host side only, as bsk_capi.hip; kernels and launch wrappers: bsk_fit.hip.  The policy it reads and writes through
// its handle: bsk_capi_policy.hpp.
#include <cmath>
#include <cstring>

#include "bsk_capi_policy.hpp"
#include "bsk_fit.hpp"
#include "bsk_pglog.hpp"
#include "bsk_pgsched.hpp"
#include "bsk_rewnorm.hpp"
#include "bsk_shuffle.hpp"

using namespace bsk::capi;

// bsk_fit_*: ONE allocation of 8-byte words [theta np | m np | v np | beta_pow 2 | A np | row 4 | count | steps | pg_row 4 | gnorm_row 2 |
// vclip_row 2 | sched 8] and, from
// the first accumulate on, the scratch of the block gradients: [G n_blocks * np floats | diag n_blocks * 10 doubles | lp 3 * 64
// n_blocks floats] (a supervised launch uses the first 4 n_blocks of diag and no lp, a policy-gradient launch without the value
// clip the first 8 n_blocks)
struct bsk_fit {
    bsk_policy* policy = nullptr;          // not owned: what accumulate reads and step writes
    int device = 0;
    double lr = 0.0, beta1 = 0.0, beta2 = 0.0, eps = 0.0, weight_decay = 0.0;
    float value_coef = 0.0f;
    double max_grad_norm = 0.0;            // bsk_fit_set_max_grad_norm: 0 = no clip, and the step's launches without it
    double* d_state = nullptr;
    void* d_scratch = nullptr;
    int blocks_cap = 0;
    bool value_seen = false;               // some accumulate since the last step carried value targets: the step moves the value network
    bool scheduled = false;                // bsk_fit_set_schedule: the policy-gradient accumulates and the step read the schedule words
    bsk::PgSchedPairs pairs = {};          // ... formed from these by bsk_fit_schedule_begin
    double kl_stop = 0.0;                  // ... and bsk_fit_kl_gate closes against this (0: no gate)

    size_t np() const { return (size_t)policy->lay.n_params; }
    double* theta() const { return d_state; }
    double* m() const { return d_state + np(); }
    double* v() const { return d_state + 2 * np(); }
    double* beta_pow() const { return d_state + 3 * np(); }
    double* A() const { return d_state + 3 * np() + 2; }
    double* row() const { return d_state + 4 * np() + 2; }
    unsigned long long* count() const { return (unsigned long long*)(d_state + 4 * np() + 6); }
    unsigned long long* steps() const { return count() + 1; }
    double* pg_row() const { return d_state + 4 * np() + 8; }
    double* gnorm_row() const { return d_state + 4 * np() + 12; }          // {norm, scale} of the last clipped step
    double* vclip_row() const { return d_state + 4 * np() + 14; }          // {value-clipped samples, sum of the unclipped d d / 2}
    // the schedule block (bsk_pgsched.hpp): {lr, clip, clip_vf, ent_coef} now, iteration, gate, steps skipped, the KL that closed it
    unsigned long long* sched() const { return (unsigned long long*)(d_state + 4 * np() + 16); }
    size_t words() const { return 4 * np() + 16 + bsk::PG_SCHED_WORDS; }
    // where the action network's parameters end in the C-ABI block: all a fit without value targets folds and moves
    int action_end() const {
        const bsk::PolicyLayout& lay = policy->lay;
        return lay.v.n_layers > 0 ? bsk::policy_pack_map(lay).layer[lay.a.n_layers].src : lay.n_params;
    }
};

namespace {

bool finite_nonneg(double x) { return std::isfinite(x) && x >= 0.0; }

// (float)theta into the policy's device layout: the gather of bsk_es_set_validation's centre members
int write_policy(bsk_fit* f, hipStream_t s) {
    HIP_TRY(bsk::launch_es_center(f->policy->lay, f->theta(), f->policy->d_params, 1, s));
    return BSK_OK;
}

// the policy-gradient arguments of an accumulate (bsk_fit_accumulate_pg), already checked
struct PgLoss {
    const float* adv;
    const float* logp_old;
    float hi, lo, ec;
    // bsk_fit_accumulate_ppo's three: with neither pointer the launches are bsk_fit_accumulate_pg's
    const float* value_old;
    float clip_vf;
    float* dvalue;
};

constexpr size_t FIT_DIAG_WORDS = 10;      // doubles of diagnostics terms the scratch holds per block: the widest launch's

// bsk_fit_accumulate (pg == nullptr) and bsk_fit_accumulate_pg: the block launch in either form, then the fold
int accumulate(bsk_fit* f, const double* d_obs, int64_t obs_stride, int n, const int32_t* d_label, const double* d_value_target,
               const uint8_t* d_alive, float* d_dlogits, int64_t out_stride, const PgLoss* pg, void* stream) {
    if (n < 1 || n > (1 << 28)) return fail(BSK_EINVAL, "bsk_fit_accumulate: n must be in 1..2^28");
    if (obs_stride < n) return fail(BSK_EINVAL, "bsk_fit_accumulate: obs_stride must be >= n");
    if (d_dlogits && out_stride < n) return fail(BSK_EINVAL, "bsk_fit_accumulate: out_stride must be >= n");
    const bsk::PolicyLayout& lay = f->policy->lay;
    if (d_value_target && lay.v.n_layers == 0) return fail(BSK_EINVAL, "bsk_fit_accumulate: d_value_target given, but the policy has no value network");
    DeviceGuard guard(f->device);
    const hipStream_t s = (hipStream_t)stream;
    const int n_blocks = (n + bsk::FIT_BLOCK_SAMPLES - 1) / bsk::FIT_BLOCK_SAMPLES;
    const size_t np = f->np();
    if (f->blocks_cap < n_blocks) {
        const size_t g_bytes = ((size_t)n_blocks * np * sizeof(float) + 15) / 16 * 16;
        int rc = grow_scratch(&f->d_scratch, &f->blocks_cap, g_bytes + (size_t)n_blocks * (FIT_DIAG_WORDS * sizeof(double) + 3 * bsk::FIT_BLOCK_SAMPLES * sizeof(float)), s,
                              "bsk_fit_accumulate: the first accumulate of a size allocates the scratch of the block gradients and cannot be "
                              "captured; make one such call outside the capture first");
        if (rc) return rc;
        f->blocks_cap = n_blocks;
    }
    const size_t g_bytes = ((size_t)f->blocks_cap * np * sizeof(float) + 15) / 16 * 16;
    const bsk::PolicyPackMap map = bsk::policy_pack_map(lay);
    bsk::FitArgs a = {};
    a.params = f->policy->d_params;
    a.a = bsk::fit_net(map, 0, lay.a);
    if (d_value_target) a.v = bsk::fit_net(map, lay.a.n_layers, lay.v);
    a.obs = d_obs; a.obs_stride = obs_stride; a.n = n;
    a.label = d_label; a.target = d_value_target; a.alive = d_alive;
    a.value_coef = f->value_coef;
    a.dlogits = d_dlogits; a.out_stride = out_stride;
    a.G = (float*)f->d_scratch;
    a.diag = (double*)((char*)f->d_scratch + g_bytes);
    a.n_params = lay.n_params;
    a.rows = bsk::fit_lds_rows(lay);
    const int n_fold = d_value_target ? lay.n_params : f->action_end();
    if (pg) {
        a.adv = pg->adv; a.logp_old = pg->logp_old;
        a.clip_hi = pg->hi; a.clip_lo = pg->lo; a.ent_coef = pg->ec;
        // the log-probabilities of the three actions, formed where policy_kernel forms its logp: one launch in front
        float* lp = (float*)((char*)f->d_scratch + g_bytes + (size_t)f->blocks_cap * FIT_DIAG_WORDS * sizeof(double));
        bsk::PolicyLogpArgs la = {};
        la.params = f->policy->d_params; la.a = lay.a; la.obs = d_obs; la.obs_stride = obs_stride; la.n = n; la.lp = lp;
        la.width = lay.width;
        HIP_TRY(bsk::launch_policy_logp(la, s));
        a.lp = lp;
        const double* sched = f->scheduled ? (const double*)f->sched() : nullptr;      // (then a.clip_hi .. and vc.clip_vf are not read)
        if (pg->value_old || pg->dvalue) {
            const bsk::FitVclip vc = {pg->value_old, pg->clip_vf, pg->dvalue};
            if (sched) HIP_TRY(bsk::launch_fit_blocks_ppo_sched(a, vc, sched, s));
            else HIP_TRY(bsk::launch_fit_blocks_ppo(a, vc, s));
            HIP_TRY(bsk::launch_fit_fold_ppo(a.G, a.diag, n_blocks, lay.n_params, n_fold, f->A(), f->row(), f->pg_row(),
                                             pg->value_old ? f->vclip_row() : nullptr, f->count(), s));
        } else {
            if (sched) HIP_TRY(bsk::launch_fit_blocks_pg_sched(a, sched, s));
            else HIP_TRY(bsk::launch_fit_blocks_pg(a, s));
            HIP_TRY(bsk::launch_fit_fold_pg(a.G, a.diag, n_blocks, lay.n_params, n_fold, f->A(), f->row(), f->pg_row(), f->count(), s));
        }
    } else {
        HIP_TRY(bsk::launch_fit_blocks(a, s));
        HIP_TRY(bsk::launch_fit_fold(a.G, a.diag, n_blocks, lay.n_params, n_fold, f->A(), f->row(), f->count(), s));
    }
    if (d_value_target) f->value_seen = true;
    return BSK_OK;        // asynchronous on `stream`: no copy, no synchronisation
}

}  // namespace

extern "C" {

int bsk_fit_create(bsk_policy* p, double lr, double beta1, double beta2, double eps, double weight_decay, double value_coef, bsk_fit** out) {
    if (!out) return fail(BSK_EINVAL, "out is NULL");
    *out = nullptr;
    if (!p) return fail(BSK_EINVAL, "policy is NULL");
    if (!finite_nonneg(lr)) return fail(BSK_EINVAL, "bsk_fit_create: lr must be finite and not negative");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(BSK_EINVAL, "bsk_fit_create: beta1 and beta2 must be in [0, 1)");
    if (!std::isfinite(eps) || !(eps > 0.0)) return fail(BSK_EINVAL, "bsk_fit_create: eps must be finite and positive");
    if (!finite_nonneg(weight_decay)) return fail(BSK_EINVAL, "bsk_fit_create: weight_decay must be finite and not negative");
    if (!finite_nonneg(value_coef)) return fail(BSK_EINVAL, "bsk_fit_create: value_coef must be finite and not negative");
    DeviceGuard guard(p->device);
    bsk_fit* f = new bsk_fit();
    f->policy = p;
    f->device = p->device;
    f->lr = lr; f->beta1 = beta1; f->beta2 = beta2; f->eps = eps; f->weight_decay = weight_decay;
    f->value_coef = (float)value_coef;
    // theta := the policy's current parameters, widened; m = v = A = 0, beta_pow = {1, 1}, count = steps = 0
    const bsk::PolicyLayout& lay = p->lay;
    std::vector<float> dev((size_t)lay.n_device), params((size_t)lay.n_params);
    std::vector<double> state(f->words(), 0.0);
    int rc = transfer(p->device, hipMemcpyDeviceToHost, {{dev.data(), p->d_params, dev.size() * sizeof(float)}});
    if (rc) { delete f; return rc; }
    bsk::policy_unpack(lay, dev.data(), params.data());
    for (size_t j = 0; j < params.size(); ++j) state[j] = (double)params[j];
    state[3 * f->np()] = state[3 * f->np() + 1] = 1.0;
    state[4 * f->np() + 13] = 1.0;         // (the clip's row before the first clipped step: {+0.0, 1.0})
    auto upload = [&]() -> int {
        HIP_TRY(hipMalloc(&f->d_state, state.size() * 8));
        HIP_COPY(hipMemcpy(f->d_state, state.data(), state.size() * 8, hipMemcpyHostToDevice));
        return BSK_OK;
    };
    if ((rc = upload())) { bsk_fit_destroy(f); return rc; }
    *out = f;
    return BSK_OK;
}

void bsk_fit_destroy(bsk_fit* f) {
    if (!f) return;
    DeviceGuard guard(f->device);
    free_all({f->d_state, f->d_scratch});
    delete f;
}

int bsk_fit_accumulate(bsk_fit* f, const double* d_obs, int64_t obs_stride, int n, const int32_t* d_label, const double* d_value_target,
                       const uint8_t* d_alive, float* d_dlogits, int64_t out_stride, void* stream) {
    if (!f || !d_obs || !d_label) return fail(BSK_EINVAL, "fit/d_obs/d_label is NULL");
    return accumulate(f, d_obs, obs_stride, n, d_label, d_value_target, d_alive, d_dlogits, out_stride, nullptr, stream);
}

int bsk_fit_accumulate_pg(bsk_fit* f, const double* d_obs, int64_t obs_stride, int n, const int32_t* d_action, const float* d_adv,
                          const float* d_logp_old, double clip, double ent_coef, const double* d_value_target, const uint8_t* d_alive,
                          float* d_dlogits, int64_t out_stride, void* stream) {
    return bsk_fit_accumulate_ppo(f, d_obs, obs_stride, n, d_action, d_adv, d_logp_old, clip, ent_coef, d_value_target, nullptr, 0.0, d_alive,
                                  d_dlogits, out_stride, nullptr, stream);
}

int bsk_fit_accumulate_ppo(bsk_fit* f, const double* d_obs, int64_t obs_stride, int n, const int32_t* d_action, const float* d_adv,
                           const float* d_logp_old, double clip, double ent_coef, const double* d_value_target, const float* d_value_old,
                           double clip_vf, const uint8_t* d_alive, float* d_dlogits, int64_t out_stride, float* d_dvalue, void* stream) {
    if (!f || !d_obs || !d_action || !d_adv) return fail(BSK_EINVAL, "fit/d_obs/d_action/d_adv is NULL");
    if (d_logp_old && !(std::isfinite(clip) && clip > 0.0 && clip < 1.0))
        return fail(BSK_EINVAL, "bsk_fit_accumulate_pg: clip must be in (0, 1) when d_logp_old is given");
    if (!finite_nonneg(ent_coef)) return fail(BSK_EINVAL, "bsk_fit_accumulate_pg: ent_coef must be finite and not negative");
    if ((d_value_old || d_dvalue) && !d_value_target)
        return fail(BSK_EINVAL, "bsk_fit_accumulate_ppo: d_value_old and d_dvalue need d_value_target");
    if (d_value_old && !(std::isfinite(clip_vf) && clip_vf > 0.0))
        return fail(BSK_EINVAL, "bsk_fit_accumulate_ppo: clip_vf must be finite and positive when d_value_old is given");
    const PgLoss pg = {d_adv, d_logp_old, 1.0f + (float)clip, 1.0f - (float)clip, (float)ent_coef, d_value_old, (float)clip_vf, d_dvalue};
    return accumulate(f, d_obs, obs_stride, n, d_action, d_value_target, d_alive, d_dlogits, out_stride, &pg, stream);
}

int bsk_fit_vclip_stats_device(bsk_fit* f, const double** d_row2) {
    if (!f || !d_row2) return fail(BSK_EINVAL, "fit/d_row2 is NULL");
    *d_row2 = f->vclip_row();
    return BSK_OK;
}

int bsk_pg_gather(const uint64_t* d_state, int n_steps, int n_envs, int64_t stride, int64_t q0, int m, const double* d_obs_hist,
                  const int32_t* d_action_hist, const float* d_adv, const float* d_logp_hist, const double* d_ret, const float* d_value_hist,
                  double* d_obs_out, int64_t out_stride, int32_t* d_action_out, float* d_adv_out, float* d_logp_out, double* d_ret_out,
                  float* d_value_out, int32_t* d_index_out, void* stream) {
    if (n_steps < 1 || n_envs < 1 || stride < n_envs) return fail(BSK_EINVAL, "bsk_pg_gather: n_steps and n_envs must be >= 1, stride >= n_envs");
    const int64_t N = (int64_t)n_steps * (int64_t)n_envs;
    if (N >= ((int64_t)1 << 31)) return fail(BSK_EINVAL, "bsk_pg_gather: n_steps * n_envs must be below 2^31");
    if (q0 < 0 || m < 1 || q0 > N - (int64_t)m) return fail(BSK_EINVAL, "bsk_pg_gather: the window q0 .. q0 + m - 1 must lie inside 0 .. n_steps * n_envs - 1");
    const void* const from[6] = {d_obs_hist, d_action_hist, d_adv, d_logp_hist, d_ret, d_value_hist};
    const void* const to[6] = {d_obs_out, d_action_out, d_adv_out, d_logp_out, d_ret_out, d_value_out};
    bool any = d_index_out != nullptr;
    for (int k = 0; k < 6; ++k) {
        if ((from[k] == nullptr) != (to[k] == nullptr)) return fail(BSK_EINVAL, "bsk_pg_gather: a history and its output are given together or not at all");
        any = any || from[k];
    }
    if (!any) return fail(BSK_EINVAL, "bsk_pg_gather: nothing to write");
    if (d_obs_hist && out_stride < m) return fail(BSK_EINVAL, "bsk_pg_gather: out_stride must be >= m");
    bsk::PgGatherArgs a = {};
    a.state = (const unsigned long long*)d_state;
    a.n_envs = n_envs; a.N = (uint32_t)N; a.stride = stride; a.q0 = q0; a.m = m; a.out_stride = out_stride;
    a.obs = d_obs_hist; a.action = d_action_hist; a.adv = d_adv; a.logp = d_logp_hist; a.ret = d_ret; a.value = d_value_hist;
    a.obs_out = d_obs_out; a.action_out = d_action_out; a.adv_out = d_adv_out; a.logp_out = d_logp_out; a.ret_out = d_ret_out;
    a.value_out = d_value_out; a.index_out = d_index_out;
    HIP_TRY(bsk::launch_pg_gather(a, (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream` of the current device: no copy, no synchronisation, no allocation
}

int bsk_pg_shuffle_advance(uint64_t* d_state, void* stream) {
    if (!d_state) return fail(BSK_EINVAL, "bsk_pg_shuffle_advance: d_state is NULL");
    HIP_TRY(bsk::launch_pg_shuffle_advance((unsigned long long*)d_state, (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream` of the current device: no copy, no synchronisation, no allocation
}

size_t bsk_pg_episodes_work_bytes(int n_envs) {
    return n_envs < 1 ? 0 : 8 * (size_t)bsk::PG_EP_WORDS * (size_t)(((int64_t)n_envs + 63) / 64);
}

int bsk_pg_episodes(const double* d_reward_hist, const uint8_t* d_reason_hist, const int32_t* d_action_hist, const float* d_value_hist,
                    const double* d_ret, int n_steps, int n_envs, int64_t stride, double* d_ep_return, int32_t* d_ep_len, void* d_work,
                    double* d_ring, int capacity, const uint64_t* d_counter, void* stream) {
    if (!d_reward_hist || !d_reason_hist) return fail(BSK_EINVAL, "bsk_pg_episodes: the reward or the reason history is NULL");
    if (!d_ep_return || !d_ep_len || !d_work || !d_ring) return fail(BSK_EINVAL, "bsk_pg_episodes: d_ep_return, d_ep_len, d_work or d_ring is NULL");
    if ((d_value_hist == nullptr) != (d_ret == nullptr)) return fail(BSK_EINVAL, "bsk_pg_episodes: d_value_hist and d_ret are given together or not at all");
    if (n_steps < 1 || n_envs < 1 || stride < n_envs) return fail(BSK_EINVAL, "bsk_pg_episodes: n_steps and n_envs must be >= 1, stride >= n_envs");
    if (capacity < 1) return fail(BSK_EINVAL, "bsk_pg_episodes: capacity must be >= 1");
    if ((int64_t)n_steps > ((int64_t)1 << 31) / stride) return fail(BSK_EINVAL, "bsk_pg_episodes: n_steps * stride must not exceed 2^31");
    bsk::PgEpisodesArgs a = {};
    a.reward = d_reward_hist; a.reason = d_reason_hist; a.action = d_action_hist; a.value = d_value_hist; a.ret = d_ret;
    a.n_steps = n_steps; a.n_envs = n_envs; a.stride = stride;
    a.ep_return = d_ep_return; a.ep_len = d_ep_len; a.work = (double*)d_work;
    a.ring = d_ring; a.capacity = capacity; a.counter = (const unsigned long long*)d_counter;
    HIP_TRY(bsk::launch_pg_episodes(a, (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream` of the current device: no copy, no synchronisation, no allocation
}

int bsk_pg_log_update(const double* d_diag, int n_rows, const double* d_norms, int n_norms, double* d_ring, int capacity,
                      const uint64_t* d_counter, void* stream) {
    if (!d_diag || !d_ring) return fail(BSK_EINVAL, "bsk_pg_log_update: d_diag or d_ring is NULL");
    if (n_rows < 1 || capacity < 1) return fail(BSK_EINVAL, "bsk_pg_log_update: n_rows and capacity must be >= 1");
    if (d_norms && n_norms < 1) return fail(BSK_EINVAL, "bsk_pg_log_update: n_norms must be >= 1 when d_norms is given");
    HIP_TRY(bsk::launch_pg_log_update(d_diag, n_rows, d_norms, n_norms, d_ring, capacity, (const unsigned long long*)d_counter,
                                      (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream` of the current device: no copy, no synchronisation, no allocation
}

int bsk_pg_log_advance(uint64_t* d_gen, int capacity, uint64_t* d_counter, void* stream) {
    if (!d_gen || !d_counter) return fail(BSK_EINVAL, "bsk_pg_log_advance: d_gen or d_counter is NULL");
    if (capacity < 1) return fail(BSK_EINVAL, "bsk_pg_log_advance: capacity must be >= 1");
    HIP_TRY(bsk::launch_pg_log_advance((unsigned long long*)d_gen, capacity, (unsigned long long*)d_counter, (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream` of the current device: no copy, no synchronisation, no allocation
}

int64_t bsk_reward_norm_work_bytes(int n) { return n < 1 ? 0 : 8 * (int64_t)bsk::REWARD_NORM_WORK_WORDS * (((int64_t)n + 63) / 64); }

int bsk_reward_norm(const double* d_reward_hist, const uint8_t* d_reason_hist, int n_steps, int n_envs, int64_t stride, double gamma,
                    double eps, double clip, int update, double* d_ret_run, void* d_state, void* d_work, double* d_out, void* stream) {
    if (!d_reward_hist || !d_reason_hist || !d_state || !d_out)
        return fail(BSK_EINVAL, "bsk_reward_norm: the reward or the reason history, d_state or d_out is NULL");
    if (update && (!d_ret_run || !d_work)) return fail(BSK_EINVAL, "bsk_reward_norm: d_ret_run and d_work are required with update");
    if (n_steps < 1 || n_envs < 1 || stride < n_envs) return fail(BSK_EINVAL, "bsk_reward_norm: n_steps and n_envs must be >= 1, stride >= n_envs");
    if ((int64_t)n_steps > ((int64_t)1 << 31) / stride) return fail(BSK_EINVAL, "bsk_reward_norm: n_steps * stride must not exceed 2^31");
    if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(BSK_EINVAL, "bsk_reward_norm: gamma must be in [0, 1]");
    if (!finite_nonneg(eps)) return fail(BSK_EINVAL, "bsk_reward_norm: eps must be finite and not negative");
    if (!(clip > 0.0)) return fail(BSK_EINVAL, "bsk_reward_norm: clip must be greater than 0 (+inf: nothing is clipped)");
    bsk::RewardNormArgs a = {};
    a.reward = d_reward_hist; a.reason = d_reason_hist;
    a.n_steps = n_steps; a.n_envs = n_envs; a.stride = stride;
    a.gamma = gamma; a.eps = eps; a.clip = clip; a.update = update != 0;
    a.ret_run = d_ret_run; a.state = (double*)d_state; a.work = (double*)d_work; a.out = d_out;
    HIP_TRY(bsk::launch_reward_norm(a, (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream` of the current device: no copy, no synchronisation, no allocation
}

int bsk_fit_pg_stats_device(bsk_fit* f, const double** d_row4) {
    if (!f || !d_row4) return fail(BSK_EINVAL, "fit/d_row4 is NULL");
    *d_row4 = f->pg_row();
    return BSK_OK;
}

int bsk_gae(const double* d_reward_hist, const uint8_t* d_reason_hist, const float* d_value_hist, const float* d_last_value, int n_steps,
            int n_envs, int64_t stride, double gamma, double lambda, float* d_adv, double* d_ret, void* stream) {
    if (!d_reward_hist || !d_reason_hist || !d_value_hist || !d_adv) return fail(BSK_EINVAL, "bsk_gae: a history or d_adv is NULL");
    if (n_steps < 1 || n_envs < 1 || stride < n_envs) return fail(BSK_EINVAL, "bsk_gae: n_steps and n_envs must be >= 1, stride >= n_envs");
    if (!(gamma >= 0.0 && gamma <= 1.0) || !(lambda >= 0.0 && lambda <= 1.0)) return fail(BSK_EINVAL, "bsk_gae: gamma and lambda must be in [0, 1]");
    HIP_TRY(bsk::launch_gae(d_reward_hist, d_reason_hist, d_value_hist, d_last_value, n_steps, n_envs, stride, gamma, gamma * lambda, d_adv,
                            d_ret, (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream` of the current device: no copy, no synchronisation, no allocation
}

int bsk_fit_step(bsk_fit* f, void* stream) {
    if (!f) return fail(BSK_EINVAL, "fit is NULL");
    DeviceGuard guard(f->device);
    const hipStream_t s = (hipStream_t)stream;
    bsk::EsAdam ad = {};
    ad.m = f->m(); ad.v = f->v(); ad.beta_pow = f->beta_pow();
    ad.beta1 = f->beta1; ad.beta2 = f->beta2;
    ad.a1 = 1.0 - f->beta1; ad.a2 = 1.0 - f->beta2;
    ad.eps = f->eps; ad.weight_decay = f->weight_decay;
    ad.lr = f->lr;
    HIP_TRY(bsk::launch_fit_step(f->theta(), f->A(), f->count(), f->steps(), f->value_seen ? f->policy->lay.n_params : f->action_end(), ad,
                               f->max_grad_norm, f->gnorm_row(), s, f->scheduled ? (const double*)f->sched() : nullptr));
    f->value_seen = false;
    return write_policy(f, s);        // asynchronous on `stream`: no copy, no synchronisation
}

int bsk_fit_stats_device(bsk_fit* f, const double** d_row4) {
    if (!f || !d_row4) return fail(BSK_EINVAL, "fit/d_row4 is NULL");
    *d_row4 = f->row();
    return BSK_OK;
}

int bsk_fit_get_state(bsk_fit* f, double* theta, double* m, double* v, double* beta_pow, uint64_t* steps) {
    if (!f) return fail(BSK_EINVAL, "fit is NULL");
    const size_t bytes = f->np() * sizeof(double);
    return transfer(f->device, hipMemcpyDeviceToHost, {{theta, f->theta(), bytes}, {m, f->m(), bytes}, {v, f->v(), bytes},
                                                       {beta_pow, f->beta_pow(), 2 * sizeof(double)}, {steps, f->steps(), 8}});
}

int bsk_fit_set_state(bsk_fit* f, const double* theta, const double* m, const double* v, const double* beta_pow, uint64_t steps) {
    if (!f) return fail(BSK_EINVAL, "fit is NULL");
    const size_t bytes = f->np() * sizeof(double);
    const unsigned long long st = steps;
    int rc = transfer(f->device, hipMemcpyHostToDevice, {{theta, f->theta(), bytes}, {m, f->m(), bytes}, {v, f->v(), bytes},
                                                         {beta_pow, f->beta_pow(), 2 * sizeof(double)}, {&st, f->steps(), 8}});
    if (rc) return rc;
    DeviceGuard guard(f->device);
    // what has been accumulated since the last step belongs to the state that is replaced: A, the count and the diagnostics row
    // (contiguous words) start from zero, as behind a step
    HIP_TRY(hipMemset(f->A(), 0, (f->np() + 5) * sizeof(double)));
    HIP_TRY(hipMemset(f->pg_row(), 0, 4 * sizeof(double)));
    HIP_TRY(hipMemset(f->vclip_row(), 0, 2 * sizeof(double)));
    f->value_seen = false;
    if (theta && (rc = write_policy(f, nullptr))) return rc;          // a new theta is the policy's too: (float)theta
    HIP_SYNC(hipDeviceSynchronize());
    return BSK_OK;
}

int bsk_fit_set_lr(bsk_fit* f, double lr) {
    if (!f) return fail(BSK_EINVAL, "fit is NULL");
    if (!finite_nonneg(lr)) return fail(BSK_EINVAL, "bsk_fit_set_lr: lr must be finite and not negative");
    f->lr = lr;
    return BSK_OK;
}

// the eight words of iteration `it` with the gate open: what bsk_fit_schedule_begin leaves, formed with its own text
static void schedule_words(const bsk_fit* f, uint64_t it, uint64_t* words) {
    for (int k = 0; k < 4; ++k) {
        const double x = bsk::pg_sched_value(it, f->pairs.total, f->pairs.a[k], f->pairs.b[k]);
        std::memcpy(&words[k], &x, 8);
    }
    words[bsk::PG_SCHED_ITERATION] = it;
    words[bsk::PG_SCHED_GATE] = words[bsk::PG_SCHED_SKIPPED] = words[bsk::PG_SCHED_KL] = 0;
}

int bsk_fit_set_schedule(bsk_fit* f, const bsk_fit_schedule* sc) {
    if (!f) return fail(BSK_EINVAL, "fit is NULL");
    if (!sc) {
        f->scheduled = false;
        return BSK_OK;
    }
    for (int e = 0; e < 2; ++e) {
        if (!finite_nonneg(sc->lr[e])) return fail(BSK_EINVAL, "bsk_fit_set_schedule: lr must be finite and not negative");
        if (!(std::isfinite(sc->clip[e]) && sc->clip[e] > 0.0 && sc->clip[e] < 1.0)) return fail(BSK_EINVAL, "bsk_fit_set_schedule: clip must be in (0, 1)");
        if (!(std::isfinite(sc->clip_vf[e]) && sc->clip_vf[e] > 0.0)) return fail(BSK_EINVAL, "bsk_fit_set_schedule: clip_vf must be finite and positive");
        if (!finite_nonneg(sc->ent_coef[e])) return fail(BSK_EINVAL, "bsk_fit_set_schedule: ent_coef must be finite and not negative");
    }
    if (sc->total >= ((uint64_t)1 << 53)) return fail(BSK_EINVAL, "bsk_fit_set_schedule: total must be below 2^53");
    if (!finite_nonneg(sc->kl_stop)) return fail(BSK_EINVAL, "bsk_fit_set_schedule: kl_stop must be 0 (no stop) or finite and positive");
    const double* const from[4] = {sc->lr, sc->clip, sc->clip_vf, sc->ent_coef};          // (the words' order)
    for (int k = 0; k < 4; ++k) { f->pairs.a[k] = from[k][0]; f->pairs.b[k] = from[k][1]; }
    f->pairs.total = sc->total;
    f->kl_stop = sc->kl_stop;
    f->scheduled = true;
    return bsk_fit_set_schedule_state(f, 0);
}

int bsk_fit_set_schedule_state(bsk_fit* f, uint64_t iteration) {
    if (!f) return fail(BSK_EINVAL, "fit is NULL");
    if (!f->scheduled) return fail(BSK_EINVAL, "bsk_fit_set_schedule_state: no schedule is attached");
    uint64_t words[bsk::PG_SCHED_WORDS];
    schedule_words(f, iteration, words);
    return transfer(f->device, hipMemcpyHostToDevice, {{words, f->sched(), sizeof(words)}});
}

int bsk_fit_get_schedule_state(bsk_fit* f, uint64_t* words8) {
    if (!f || !words8) return fail(BSK_EINVAL, "fit/words8 is NULL");
    return transfer(f->device, hipMemcpyDeviceToHost, {{words8, f->sched(), 8 * bsk::PG_SCHED_WORDS}});
}

int bsk_fit_schedule_device(bsk_fit* f, const uint64_t** d_words8) {
    if (!f || !d_words8) return fail(BSK_EINVAL, "fit/d_words8 is NULL");
    *d_words8 = (const uint64_t*)f->sched();
    return BSK_OK;
}

int bsk_fit_schedule_begin(bsk_fit* f, void* stream) {
    if (!f) return fail(BSK_EINVAL, "fit is NULL");
    if (!f->scheduled) return fail(BSK_EINVAL, "bsk_fit_schedule_begin: no schedule is attached");
    DeviceGuard guard(f->device);
    HIP_TRY(bsk::launch_pg_sched_begin(f->sched(), f->pairs, (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream`: no copy, no synchronisation, no allocation
}

int bsk_fit_kl_gate(bsk_fit* f, const double* d_diag, int n_rows, void* stream) {
    if (!f || !d_diag) return fail(BSK_EINVAL, "fit/d_diag is NULL");
    if (!f->scheduled || !(f->kl_stop > 0.0)) return fail(BSK_EINVAL, "bsk_fit_kl_gate: no schedule with kl_stop > 0 is attached");
    if (n_rows < 1) return fail(BSK_EINVAL, "bsk_fit_kl_gate: n_rows must be >= 1");
    DeviceGuard guard(f->device);
    HIP_TRY(bsk::launch_fit_kl_gate(d_diag, n_rows, f->kl_stop, f->sched(), f->count(), (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream`: no copy, no synchronisation, no allocation
}

int bsk_fit_schedule_end(bsk_fit* f, double* d_ring, int capacity, void* stream) {
    if (!f) return fail(BSK_EINVAL, "fit is NULL");
    if (!f->scheduled) return fail(BSK_EINVAL, "bsk_fit_schedule_end: no schedule is attached");
    if (d_ring && capacity < 1) return fail(BSK_EINVAL, "bsk_fit_schedule_end: capacity must be >= 1 when d_ring is given");
    DeviceGuard guard(f->device);
    HIP_TRY(bsk::launch_pg_sched_end(f->sched(), d_ring, capacity, (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream`: no copy, no synchronisation, no allocation
}

int bsk_fit_set_max_grad_norm(bsk_fit* f, double max_norm) {
    if (!f) return fail(BSK_EINVAL, "fit is NULL");
    if (!finite_nonneg(max_norm)) return fail(BSK_EINVAL, "bsk_fit_set_max_grad_norm: max_norm must be 0 (off) or finite and positive");
    f->max_grad_norm = max_norm;
    return BSK_OK;
}

int bsk_fit_grad_norm_device(bsk_fit* f, const double** d_row2) {
    if (!f || !d_row2) return fail(BSK_EINVAL, "fit/d_row2 is NULL");
    *d_row2 = f->gnorm_row();
    return BSK_OK;
}

int bsk_fit_apply_obs_norm(bsk_fit* f, bsk_obs_stats* s, double std_min, void* stream) {
    if (!f || !s) return fail(BSK_EINVAL, "fit/stats is NULL");
    if (!std::isfinite(std_min) || !(std_min > 0.0)) return fail(BSK_EINVAL, "bsk_fit_apply_obs_norm: std_min must be finite and positive");
    if (f->device != s->device) return fail(BSK_EINVAL, "bsk_fit_apply_obs_norm: the fit and the statistics live on different devices");
    DeviceGuard guard(f->device);
    HIP_TRY(bsk::launch_es_obs_norm(s->st.tot, s->st.tot_n, std_min, f->theta(), (hipStream_t)stream));
    return write_policy(f, (hipStream_t)stream);        // asynchronous on `stream`: no copy, no synchronisation
}

int64_t bsk_adv_normalize_work_bytes(int n) { return n < 1 ? 0 : 8 * (4 + 3 * (((int64_t)n + 63) / 64)); }

int bsk_adv_normalize(const float* d_adv, const uint8_t* d_alive, int rows, int n, int64_t stride, double eps, float* d_out, void* d_work,
                      void* stream) {
    if (!d_adv || !d_out || !d_work) return fail(BSK_EINVAL, "bsk_adv_normalize: d_adv, d_out or d_work is NULL");
    if (rows < 1 || n < 1 || stride < n) return fail(BSK_EINVAL, "bsk_adv_normalize: rows and n must be >= 1, stride >= n");
    if ((int64_t)rows > ((int64_t)1 << 31) / stride) return fail(BSK_EINVAL, "bsk_adv_normalize: rows * stride must not exceed 2^31");
    if (!std::isfinite(eps) || !(eps > 0.0)) return fail(BSK_EINVAL, "bsk_adv_normalize: eps must be finite and positive");
    HIP_TRY(bsk::launch_adv_normalize(d_adv, d_alive, rows, n, stride, eps, d_out, (double*)d_work, (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream` of the current device: no copy, no synchronisation, no allocation
}

int bsk_fit_alive_mask(const uint8_t* d_reason, int n, int first, uint8_t* d_alive, void* stream) {
    if (!d_reason || !d_alive) return fail(BSK_EINVAL, "d_reason/d_alive is NULL");
    if (n < 1) return fail(BSK_EINVAL, "bsk_fit_alive_mask: n must be >= 1");
    HIP_TRY(bsk::launch_fit_alive(d_reason, n, first != 0, d_alive, (hipStream_t)stream));
    return BSK_OK;        // asynchronous on `stream`: no copy, no synchronisation
}

}  // extern "C"
