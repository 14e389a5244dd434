// bsk_capi.hip — C-ABI of libbskgpu.so (see include/bskgpu.h for the contract and the reference
// interfaces each entry point replaces): the environment handle.  Host side only: handle management, HBM allocation,
// uploads/downloads, launch geometry.  No CPU compute path exists here by design: without a
// gfx950 device bsk_create fails with BSK_ENODEV.  (bsk_config.hip: the configuration arithmetic; bsk_capi_policy.hip: policy,
// population and observation statistics; bsk_capi_es.hip: evolution strategy; bsk_capi.hpp: what they share.)
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>

#include "bsk_capi.hpp"
#include "bsk_rollout.hpp"

namespace bsk { namespace capi __attribute__((visibility("hidden"))) {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

std::atomic<long long> g_n_copies{0}, g_n_syncs{0};

int open_device(int device_id, hipDeviceProp_t* prop_out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(BSK_ENODEV, "no HIP device visible: libbskgpu has no CPU fallback");
    if (device_id < 0 || device_id >= ndev) return fail(BSK_ENODEV, "device_id out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(BSK_ENODEV, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    if (prop_out) *prop_out = prop;
    return BSK_OK;
}

} }  // namespace bsk::capi

using namespace bsk::capi;

namespace {

// Extra elements per field row of the state slab.  An EMPIRICAL constant, not a derived one: with the slab's rows an odd multiple of
// 256 B apart the K = 1 launch of 65 536 spacecraft is 2 - 3 % shorter than with rows at a power-of-two distance (6.20 against 6.36 us
// wall per launch; profiles/r05/stride_pad.txt, ten alternations in stride_pad_ab.txt), a micro-benchmark of the bare access pattern
// does not reproduce it (tools/micro/row_channels.hip) and the mechanism is not established.  Applied only over the range of batch
// sizes it was measured to help at (profiles/r06/stride_pad.txt, one box, alternating: 65 536 -2.7 %, 98 304 -0.5 %; 32 768 and
// 131 072 nothing either way, 4 Mi slightly slower); everywhere else the rows are N rounded up to 256 like every other per-env
// array of the handle.
#ifndef BSK_TUNABLES
#define BSK_TUNABLES 0
#endif
constexpr int SLAB_PAD_ELEMS = 32, SLAB_PAD_MIN_ENVS = 65536, SLAB_PAD_MAX_ENVS = 98304;
int slab_row_pad(int n_envs) { return (n_envs >= SLAB_PAD_MIN_ENVS && n_envs <= SLAB_PAD_MAX_ENVS) ? SLAB_PAD_ELEMS : 0; }

int ensure_stage(bsk_handle* h, size_t m) {
    if (m <= h->stage_cap) return BSK_OK;
    if (h->d_ic_stage) (void)hipFree(h->d_ic_stage);
    if (h->d_idx_stage) (void)hipFree(h->d_idx_stage);
    h->d_ic_stage = nullptr;
    h->d_idx_stage = nullptr;
    h->stage_cap = 0;
    HIP_TRY(hipMalloc(&h->d_ic_stage, m * h->nf * sizeof(double)));
    HIP_TRY(hipMalloc(&h->d_idx_stage, m * sizeof(int)));
    h->stage_cap = m;
    return BSK_OK;
}

bsk::ResetOut reset_out(const bsk_handle* h) {
    bsk::ResetOut ro;
    ro.obs = h->d_obs; ro.ostride = h->ostride; ro.obs_rm = h->d_obs_rm; ro.reward = h->d_reward; ro.reason = h->d_reason; ro.done = h->d_done;
    ro.ep_return = h->d_ep_return;
    ro.inv_wheel_limit = h->sp.obs.inv_wheel_limit; ro.charge_scale = h->sp.obs.charge_scale;
    ro.n_rw = h->cfg.n_rw;
    return ro;
}

// The batch scalars of the last step (sum of rewards, number of done envs) are formed from the reward buffer and the done
// ballots by a kernel of their own, once, when somebody asks - or just before a reset entry point overwrites the restarted
// envs' rewards with zeros (the vec env auto-resets BEFORE a training loop reads the step's statistics).
static bool note_capture(bsk_handle* h) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (!h->replayable && hipStreamIsCapturing(h->stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone) h->replayable = true;
    return h->replayable;
}

static bsk::StatsSeal stats_seal(const bsk_handle* h) {
    return bsk::StatsSeal{(const unsigned long long*)h->d_cnt, h->d_episodes, h->d_seal};
}

static int snapshot_stats(bsk_handle* h) {
    const bool replayable = note_capture(h);
    if (h->stats_fresh && !replayable) return BSK_OK;
    // (a request that is itself being captured must not freeze "the last launch wrote the wave sums" into the graph: a replay may
    // follow steps that did not - the two-level form whenever the handle is replayable)
    HIP_TRY(bsk::launch_stats(h->d_reward, h->n, h->d_done_mask, (h->n + 63) / 64, h->d_wave_sum, h->d_done_part,
                              h->d_stat_sum, h->d_stat_done, h->d_stats2, h->wave_sums_fresh && !replayable, stats_seal(h), h->stream));
    h->stats_fresh = true;
    return BSK_OK;
}

// A reset entry point has taken the snapshot and enqueued the kernels that zero the restarted envs' rewards: from here until the
// next step launch the snapshot is what bsk_get_batch_stats* report, also on a handle whose launches replay from a HIP graph
// (bsk_aux.hip: stats_sealed).
static int seal_stats(bsk_handle* h) {
    if (!h->stepped) return BSK_OK;
    HIP_TRY(bsk::launch_seal(stats_seal(h), h->stream));
    return BSK_OK;
}

// After a stream synchronisation: has a kernel raised the handle's error word?  (bsk_device.hpp: BSK_DEVERR_*)
int check_device_error(bsk_handle* h) {
    if (!h->h_err) return BSK_OK;
    const int e = *(volatile int*)h->h_err;
    if (e == 0) return BSK_OK;
    *(volatile int*)h->h_err = 0;
    if (e == bsk::BSK_DEVERR_TRI_EXCHANGE)
        return fail(BSK_EHIP, "step kernel (three-wave form): a wave waited 2^20 polls for its partner's stage value and gave up; "
                              "the results of that launch are invalid (observations were set to NaN)");
    if (e == bsk::BSK_DEVERR_FORK_MAP)
        return fail(BSK_EHIP, "bsk_fork_device: a map entry was neither -1 nor a source env index; those envs were left unchanged");
    return fail(BSK_EHIP, "step kernel raised device error " + std::to_string(e));
}
#define SYNC_CHECKED(h) do { HIP_SYNC(hipStreamSynchronize((h)->stream)); int rc_ = check_device_error(h); if (rc_) return rc_; } while (0)

void fill_buffers(bsk_handle* h, bsk::StepBuffers& b, const void* d_actions, int substeps, int act_shift, bool static_charge) {
    b.cold = h->d_cold;
    b.act = (const int*)d_actions;
    b.act_shift = act_shift;
    bsk::TailArgs& t = b.tail;
    t.obs_cfg = h->sp.obs;
    t.st = h->d_state; t.cnt = h->d_cnt; t.obs = h->d_obs; t.reward = h->d_reward; t.done_mask = h->d_done_mask; t.reason = h->d_reason;
    t.stride = h->stride; t.ostride = h->ostride; t.n = h->n; t.substeps = substeps;
    t.pool = h->d_pool; t.term_obs = h->d_term_obs; t.episodes = h->d_episodes; t.n_pool = h->n_pool; t.n_fields = h->nf;
    t.fsw_lag = h->sp.fsw_lag; t.nav_lag = h->sp.nav_lag; t.env_base = h->env_base; t.static_charge = static_charge ? 1 : 0;
    t.ep_return = h->d_ep_return; t.term_return = h->d_term_return; t.term_len = h->d_term_len; t.done = h->d_done;
    t.obs_rm = h->d_obs_rm; t.err = h->h_err; t.dbg = h->d_dbg;
    // (above 2 Mi spacecraft one workgroup joining 32 768+ wave sums AND as many done ballots is no faster than the two-level form; a
    // handle whose launches have been captured keeps the two-level form too: "the last launch wrote the wave sums" is host-side
    // knowledge, and a replayed graph steps without telling the host)
    t.wave_sum = (h->step_stats && !h->replayable && h->n <= (1 << 21)) ? h->d_wave_sum : nullptr;
}

// The form of the step kernel a launch of `substeps` sub-steps runs (bsk_handle::policy).  substeps = 0: the handle's single-wave
// form (every wave-split form needs >= 1), which bsk_kernel_info reports before the first launch.
int choose_form(const bsk_handle* h, int substeps) {
    const auto& f = h->policy;
    if (f.tri_ok && substeps >= f.tri_min_substeps && h->n <= f.tri_max_envs) return bsk::FORM_TRI;
    if (f.pair_ok && substeps >= f.pair_min_substeps && h->n <= f.pair_max_envs) return bsk::FORM_PAIR;
    // (an IC pool may be staged at any time, and its restarts rewrite r, v rows from the wave that does not hold them)
    if (f.halves_ok && f.halves_mode != 0 && substeps == 1 && h->n_pool == 0 &&
        (f.halves_mode > 0 || (h->n >= f.halves_min_envs && h->n <= f.halves_max_envs))) return bsk::FORM_HALVES;
    return h->cfg.gravity_model == BSK_GRAV_SH ? f.sh_form : bsk::FORM_SINGLE;
}

// Dispatch-timestamp sampling.  stride == 1: every launch is stamped.  stride > 1: launches
// seq % stride == 0 and 1 are stamped as a pair and only the second is counted — the first one
// absorbs the transition from un-stamped back-to-back launches (a lone stamped launch reads ~25 %
// long), the second runs under the same conditions as in an every-launch-stamped run.
int stamp_events(bsk_handle* h, hipEvent_t& e0, hipEvent_t& e1) {
    e0 = e1 = nullptr;
    if (!h->prof) return BSK_OK;
    const int ph = h->ev_seq++ % h->ev_stride;
    if (h->ev_stride == 1 || ph == 1) {
        if (h->ev_used + 2 <= (int)h->ev.size()) {
            e0 = h->ev[h->ev_used];
            e1 = h->ev[h->ev_used + 1];
            h->ev_used += 2;
        }
    } else if (ph == 0) {
        if (!h->ev_warm[0]) {
            HIP_TRY(hipEventCreate(&h->ev_warm[0]));
            HIP_TRY(hipEventCreate(&h->ev_warm[1]));
        }
        e0 = h->ev_warm[0];
        e1 = h->ev_warm[1];
    }
    return BSK_OK;
}
}  // namespace

namespace bsk { namespace capi __attribute__((visibility("hidden"))) {

int check_steppable(const bsk_handle* h) {
    if (h->cfg.gravity_model == BSK_GRAV_SH && !h->sp.sh_tab)
        return fail(BSK_EINVAL, "BSK_GRAV_SH: call bsk_set_gravity_sh before stepping");
    if ((h->cfg.flags & BSK_FLAG_AUTO_RESET) && h->n_pool == 0)
        return fail(BSK_EINVAL, "BSK_FLAG_AUTO_RESET: call bsk_set_ic_pool before stepping");
    return BSK_OK;
}

int do_step(bsk_handle* h, const void* d_actions, int substeps, int act_shift) {
    { int rc = check_steppable(h); if (rc) return rc; }
    bsk::StepBuffers b;
    const bool replayable = note_capture(h);      // (a captured launch must not freeze a host-side decision into the graph)
    fill_buffers(h, b, d_actions, substeps, act_shift,
                 !replayable && (h->sp.feat == bsk::FEAT_BARE || h->sp.feat == bsk::FEAT_LDSS) && h->charge_pos && (h->n_pool == 0 || h->pool_charge_pos));
    hipEvent_t e0, e1;
    { int rc = stamp_events(h, e0, e1); if (rc) return rc; }
    h->last = {choose_form(h, substeps), false, false};
    const bsk::StepLaunch go{h->sp, b, h->stream, e0, e1};
    bsk::KernelDesc d;
    HIP_TRY(bsk::dispatch_step(h->cfg.gravity_model, h->cfg.n_rw, h->diag, h->sp.feat, h->last.form, h->block, h->n, &go, &d));
    h->stats_fresh = false;
    h->wave_sums_fresh = b.tail.wave_sum != nullptr;
    h->stepped = true;
    return BSK_OK;
}
} }  // namespace bsk::capi

namespace {

// ------------------------------------------------------------------------------------------------------------------------------
// Forks (bsk_fork_device; kernels: bsk_fork.hip)
bsk::ForkSide fork_side(const bsk_handle* h) {
    bsk::ForkSide f;
    f.st = h->d_state; f.stride = h->stride; f.cnt = h->d_cnt; f.obs = h->d_obs; f.ostride = h->ostride; f.reward = h->d_reward;
    f.reason = h->d_reason; f.done_mask = h->d_done_mask; f.obs_rm = h->d_obs_rm; f.ep_return = h->d_ep_return;
    f.term_return = h->d_term_return; f.term_len = h->d_term_len; f.done = h->d_done; f.term_obs = h->d_term_obs;
    f.episodes = h->d_episodes; f.n = h->n;
    return f;
}

// the flags that change what a step writes or the form it runs in, never its arithmetic: free to differ between fork partners
constexpr uint32_t FORK_FREE_FLAGS = BSK_FLAG_AUTO_RESET | BSK_FLAG_EPISODE_STATS | BSK_FLAG_OBS_ROWMAJOR | BSK_FLAG_LDS_SCRATCH;

int fork_compatible(const bsk_handle* dst, const bsk_handle* src) {
    if (dst->device != src->device) return fail(BSK_EINVAL, "bsk_fork_device: the handles live on different devices");
    if (dst->cfg.n_rw != src->cfg.n_rw) return fail(BSK_EINVAL, "bsk_fork_device: the handles have different n_rw");
    bsk_config a = dst->cfg, b = src->cfg;
    a.flags &= ~FORK_FREE_FLAGS;
    b.flags &= ~FORK_FREE_FLAGS;
    if (std::memcmp(&a, &b, sizeof a) != 0)
        return fail(BSK_EINVAL, "bsk_fork_device: the handles' bsk_configs differ (beyond AUTO_RESET / EPISODE_STATS / OBS_ROWMAJOR / LDS_SCRATCH)");
    if (dst->sim_time != src->sim_time) return fail(BSK_EINVAL, "bsk_fork_device: the handles' bsk_set_sim_time values differ");
    if (dst->cfg.gravity_model == BSK_GRAV_SH && (dst->sh_cbar != src->sh_cbar || dst->sh_sbar != src->sh_sbar))
        return fail(BSK_EINVAL, "bsk_fork_device: the handles' spherical-harmonic coefficients differ");
    return BSK_OK;
}

// the in-handle fork's gather target: every buffer a handle can have (the optional ones too: a pool staged after the scratch was
// made must still be forked), laid out with the handle's strides
int ensure_fork_scratch(bsk_handle* h) {
    if (h->d_fork_block) return BSK_OK;
    const size_t S = (size_t)h->ostride;
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t sizes[] = {(size_t)h->nf * h->stride * sizeof(double), S * sizeof(int2), 5 * S * sizeof(double), S * sizeof(double), S,
                            S / 64 * sizeof(unsigned long long), 5 * S * sizeof(double), S * sizeof(double), S * sizeof(double), S * sizeof(int),
                            S, 5 * S * sizeof(double), S * sizeof(int)};
    size_t off[13], total = 0;
    for (int k = 0; k < 13; ++k) { off[k] = total; total += up(sizes[k]); }
    void* blk = nullptr;
    HIP_TRY(hipMalloc(&blk, total));
    char* p = (char*)blk;
    bsk::ForkSide& f = h->fork_scratch;
    f.st = (double*)(p + off[0]); f.stride = h->stride; f.cnt = (int2*)(p + off[1]); f.obs = (double*)(p + off[2]); f.ostride = h->ostride;
    f.reward = (double*)(p + off[3]); f.reason = (unsigned char*)(p + off[4]); f.done_mask = (unsigned long long*)(p + off[5]);
    f.obs_rm = (double*)(p + off[6]); f.ep_return = (double*)(p + off[7]); f.term_return = (double*)(p + off[8]); f.term_len = (int*)(p + off[9]);
    f.done = (unsigned char*)(p + off[10]); f.term_obs = (double*)(p + off[11]); f.episodes = (int*)(p + off[12]); f.n = h->n;
    h->d_fork_block = blk;
    return BSK_OK;
}

int do_fork(bsk_handle* dst, bsk_handle* src, const int32_t* d_map) {
    int rc = fork_compatible(dst, src);
    if (rc) return rc;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(dst->stream, &cap));
    if (src == dst) {
        // every destination receives its source's values from BEFORE the call (a permutation is a valid map): gather into the
        // scratch, then copy the mapped envs back
        if (!dst->d_fork_block && cap != hipStreamCaptureStatusNone)
            return fail(BSK_EINVAL, "bsk_fork_device: the first in-handle fork of a handle allocates its scratch and cannot be captured; "
                                    "make one in-handle fork outside the capture first");
        if ((rc = ensure_fork_scratch(dst))) return rc;
        (void)note_capture(dst);
        HIP_TRY(bsk::launch_fork(fork_side(dst), dst->fork_scratch, dst->nf, d_map, false, dst->h_err, nullptr, dst->stream));
        HIP_TRY(bsk::launch_fork(dst->fork_scratch, fork_side(dst), dst->nf, d_map, true, nullptr, dst->d_seal, dst->stream));
    } else {
        const bool two_streams = src->stream != dst->stream;
        if (two_streams) {
            if (!dst->ev_fork_in) HIP_TRY(hipEventCreateWithFlags(&dst->ev_fork_in, hipEventDisableTiming));
            if (!dst->ev_fork_out) HIP_TRY(hipEventCreateWithFlags(&dst->ev_fork_out, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(dst->ev_fork_in, src->stream));           // the fork reads what src's queued work leaves
            HIP_TRY(hipStreamWaitEvent(dst->stream, dst->ev_fork_in, 0));
        }
        (void)note_capture(dst);
        HIP_TRY(bsk::launch_fork(fork_side(src), fork_side(dst), dst->nf, d_map, false, dst->h_err, dst->d_seal, dst->stream));
        if (two_streams) {
            HIP_TRY(hipEventRecord(dst->ev_fork_out, dst->stream));          // later work on src cannot overwrite rows the fork still reads
            HIP_TRY(hipStreamWaitEvent(src->stream, dst->ev_fork_out, 0));
        }
    }
    dst->charge_pos = false;        // (a forked env may carry an empty battery: the bare levels read the charge again, as after bsk_set_state)
    dst->stats_fresh = dst->wave_sums_fresh = false;
    dst->stepped = true;
    return BSK_OK;
}
}  // namespace

static int ensure_pool_buffers(bsk_handle* h, int n_pool);

extern "C" {

const char* bsk_last_error(void) { return g_err.c_str(); }
const char* bsk_version(void) { return "bskgpu 0.1 (gfx950)"; }

int bsk_create(const bsk_config* cfg, int n_envs, int device_id, void* stream, bsk_handle** out) {
    if (!cfg || !out) return fail(BSK_EINVAL, "cfg/out is NULL");
    *out = nullptr;
    if (n_envs < 1 || n_envs > (1 << 28)) return fail(BSK_EINVAL, "n_envs must be in 1..2^28");
    int rc = validate(*cfg);
    if (rc) return rc;
    hipDeviceProp_t prop;
    if ((rc = open_device(device_id, &prop))) return rc;
    DeviceGuard guard(device_id);

    bsk_handle* h = new bsk_handle();
    h->cfg = *cfg;
    rc = build_params(*cfg, h->sp, h->cold, h->diag);
    if (rc) { delete h; return rc; }
    h->n = n_envs;
    h->nf = BSK_NF_BASE + cfg->n_rw + BSK_NF_TAIL;
    h->device = device_id;
    // Rows of N rounded up to 256 elements for everything a consumer sees (observation / reward rows, per-env arrays: a shard that
    // fills its rows is one contiguous block for the exchange step); the state slab's field rows carry slab_row_pad() more.
    h->ostride = ((int64_t)n_envs + 255) / 256 * 256;
    h->stride = h->ostride + slab_row_pad(n_envs);
#if BSK_TUNABLES
    // measurement overrides, `make tunables` builds only (variants/tunables.so; the product library never reads them):
    // extra elements per observation / reward row too; the slab's extra elements per row (multiples of 16)
    if (const char* sp = std::getenv("BSKGPU_OSTRIDE_PAD")) {
        const int v = std::atoi(sp);
        if (v > 0 && v % 16 == 0) h->ostride += v;
    }
    if (const char* sp = std::getenv("BSKGPU_STRIDE_PAD")) {
        const int v = std::atoi(sp);
        if (v >= 0 && v % 16 == 0) h->stride = ((int64_t)n_envs + 255) / 256 * 256 + v;
    }
#endif
    // 64-lane workgroups spread a small batch over more CUs (65 536 envs = 1 024 waves = 4 per CU);
    // large batches use 256 so the dispatcher has fewer workgroups to place.
    h->block = n_envs >= (1 << 20) ? 256 : 64;
#if BSK_TUNABLES
    if (const char* b = std::getenv("BSKGPU_BLOCK")) {   // measurement override: 64, 128 or 256
        const int v = std::atoi(b);
        if (v == 64 || v == 128 || v == 256) h->block = v;
    }
#endif
    // the power-system kernels carry 37.6 KB of LDS per wave: one wave per workgroup at every batch size
    if (cfg->flags & BSK_FLAG_POWER) h->block = 64;
    // both wave-split forms pay while every workgroup has a CU (and its LDS) to itself: 64 spacecraft per CU of THIS device
    // (256 CUs on a whole MI355X; fewer in a partitioned mode)
    if (prop.multiProcessorCount > 0) h->policy.pair_max_envs = h->policy.tri_max_envs = 64 * prop.multiProcessorCount;
    // the halves form doubles the waves of a launch and its kernel leaves room for two waves per SIMD: it pays while one round
    // places them all, up to 256 spacecraft per CU (65 536 on a whole MI355X: +7.7 %; 131 072 forced into the form: -18 %).
    // Measured faster from 128 per CU up (32 768: +7 %); below, 16 384 read -7 % and +4 % in two runs and stays as it was
    // (profiles/halves_k1/README.md)
    if (prop.multiProcessorCount > 0) {
        h->policy.halves_min_envs = 128 * prop.multiProcessorCount;
        h->policy.halves_max_envs = 256 * prop.multiProcessorCount;
    }
    h->policy.pair_ok = bsk::form_built(cfg->gravity_model, h->diag, h->sp.feat, bsk::FORM_PAIR);
    h->policy.tri_ok = bsk::form_built(cfg->gravity_model, h->diag, h->sp.feat, bsk::FORM_TRI);
    h->sp.pair_shift = 31;     // no swap: the hardware already places one wave 0 and one wave 1 of different workgroups on a SIMD (tools/micro/placement.hip)
#if BSK_TUNABLES
    if (const char* ps = std::getenv("BSKGPU_PAIR_SHIFT")) h->sp.pair_shift = std::max(0, std::min(31, std::atoi(ps)));
#endif
    if (const char* pv = std::getenv("BSKGPU_PAIR")) {
        const int v = std::atoi(pv);
        if (v == 0) h->policy.pair_ok = false;
        else { h->policy.pair_min_substeps = 1; h->policy.pair_max_envs = 1 << 28; }   // every launch (measurement / tests)
    }
    if (const char* tv = std::getenv("BSKGPU_TRI")) {
        const int v = std::atoi(tv);
        if (v == 0) h->policy.tri_ok = false;
        else { h->policy.tri_min_substeps = 1; h->policy.tri_max_envs = 1 << 28; }     // every launch (measurement / tests)
    }
    // the halves form is complete where the FSW chain runs on the state of one integrator step earlier (nav_lag): with nav_lag = 0
    // the observation needs the end-of-step r, v in the rotational wave on every launch
    h->policy.halves_ok = bsk::form_built(cfg->gravity_model, h->diag, h->sp.feat, bsk::FORM_HALVES, cfg->n_rw) && h->sp.nav_lag != 0;
    h->last.form = choose_form(h, 0);
    if (stream) { h->stream = (hipStream_t)stream; h->own_stream = false; }
    else {
        hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { delete h; return fail(BSK_EHIP, std::string("hipStreamCreate: ") + hipGetErrorString(e)); }
        h->own_stream = true;
    }
    const int64_t S = h->ostride;
    auto alloc = [&](void** p, size_t bytes) -> hipError_t {
        hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) e = hipMemsetAsync(*p, 0, bytes, h->stream);
        return e;
    };
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = alloc((void**)&h->d_state, (size_t)h->nf * h->stride * sizeof(double));
    if (e == hipSuccess) e = alloc((void**)&h->d_cnt, (size_t)S * sizeof(int2));
    if (e == hipSuccess) e = alloc((void**)&h->d_act, (size_t)S * sizeof(int));
    // observation rows and the reward row in ONE allocation, f64[6][stride]: a shard whose size equals its stride hands the
    // exchange step one contiguous block per rank (rccl.py: rank-major gather)
    if (e == hipSuccess) e = alloc((void**)&h->d_obs, (size_t)6 * S * sizeof(double));
    if (e == hipSuccess) h->d_reward = h->d_obs + (size_t)5 * S;
    if (e == hipSuccess) e = alloc((void**)&h->d_done_mask, (size_t)(S / 64) * sizeof(unsigned long long));
    if (e == hipSuccess) e = alloc((void**)&h->d_reason, (size_t)S);
    if (e == hipSuccess) e = alloc((void**)&h->d_stat_sum, sizeof(double));
    if (e == hipSuccess) e = alloc((void**)&h->d_stat_done, sizeof(long long));
    if (e == hipSuccess) e = alloc((void**)&h->d_stats2, 2 * sizeof(double));
    if (e == hipSuccess) e = alloc((void**)&h->d_seal, 3 * sizeof(unsigned long long));
    if (e == hipSuccess) e = alloc((void**)&h->d_wave_sum, (size_t)(S / 64) * sizeof(double));
    if (e == hipSuccess) e = alloc((void**)&h->d_done_part, (size_t)bsk::stats_done_parts() * sizeof(unsigned));
    if (e == hipSuccess) e = alloc((void**)&h->d_dbg, (size_t)(S / 64) * sizeof(unsigned long long));
    if (e == hipSuccess && (cfg->flags & BSK_FLAG_EPISODE_STATS)) {
        e = alloc((void**)&h->d_ep_return, (size_t)S * sizeof(double));
        if (e == hipSuccess) e = alloc((void**)&h->d_term_return, (size_t)S * sizeof(double));
        if (e == hipSuccess) e = alloc((void**)&h->d_term_len, (size_t)S * sizeof(int));
        if (e == hipSuccess) e = alloc((void**)&h->d_done, (size_t)S);
    }
    if (e == hipSuccess && (cfg->flags & BSK_FLAG_OBS_ROWMAJOR)) e = alloc((void**)&h->d_obs_rm, (size_t)5 * S * sizeof(double));
    if (e == hipSuccess) {
        e = hipHostMalloc((void**)&h->h_err, sizeof(int), hipHostMallocDefault);
        if (e == hipSuccess) *h->h_err = 0;
    }
    if (e == hipSuccess) e = alloc((void**)&h->d_cold, sizeof(bsk::ColdCfg));
    if (e == hipSuccess) e = hipMemcpyAsync(h->d_cold, &h->cold, sizeof(bsk::ColdCfg), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        int code = fail(e == hipErrorOutOfMemory ? BSK_ENOMEM : BSK_EHIP, std::string("device allocation: ") + hipGetErrorString(e));
        bsk_destroy(h);
        return code;
    }
    *out = h;
    return BSK_OK;
}

void bsk_destroy(bsk_handle* h) {
    if (!h) return;
    DeviceGuard guard(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (hipEvent_t ev : h->ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : h->ev_warm)
        if (ev) (void)hipEventDestroy(ev);
    void* bufs[] = {h->d_state, h->d_cnt, h->d_act, h->d_obs /* + d_reward: one block */, h->d_done_mask, h->d_reason,
                    h->d_stat_sum, h->d_stat_done, h->d_ic_stage, h->d_idx_stage, h->d_mask_stage, h->d_cold, h->d_sh_tab, h->d_sh_tab4, h->d_pool, h->d_term_obs, h->d_episodes,
                    h->d_ep_return, h->d_term_return, h->d_term_len, h->d_done, h->d_obs_rm, h->d_stats2, h->d_dbg, h->d_wave_sum, h->d_done_part, h->d_seal};
    for (void* p : bufs)
        if (p) (void)hipFree(p);
    if (h->h_err) (void)hipHostFree(h->h_err);
    for (void* p : {h->d_fork_block, (void*)h->d_map_stage})
        if (p) (void)hipFree(p);
    for (hipEvent_t ev : {h->ev_fork_in, h->ev_fork_out})
        if (ev) (void)hipEventDestroy(ev);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int bsk_set_gravity_sh(bsk_handle* h, int degree, const double* cbar, const double* sbar) {
    if (!h || !cbar || !sbar) return fail(BSK_EINVAL, "handle/cbar/sbar is NULL");
    if (h->cfg.gravity_model != BSK_GRAV_SH) return fail(BSK_EINVAL, "handle was not created with BSK_GRAV_SH");
    if (degree != h->cfg.sh_degree) return fail(BSK_EINVAL, "degree differs from bsk_config.sh_degree");
    if (cbar[0] != 1.0) return fail(BSK_EINVAL, "Cbar[0][0] must be 1 (normalised coefficients)");
    DeviceGuard guard(h->device);
    std::vector<double> tab, tab4;
    build_sh_table(degree, cbar, sbar, tab);
    const ShLayout lay = build_sh_table_dpp(degree, cbar, sbar, tab4);
    HIP_SYNC(hipStreamSynchronize(h->stream));
    if (h->d_sh_tab) { (void)hipFree(h->d_sh_tab); h->d_sh_tab = nullptr; }
    if (h->d_sh_tab4) { (void)hipFree(h->d_sh_tab4); h->d_sh_tab4 = nullptr; }
    HIP_TRY(hipMalloc(&h->d_sh_tab, tab.size() * sizeof(double)));
    HIP_COPY(hipMemcpy(h->d_sh_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&h->d_sh_tab4, tab4.size() * sizeof(double)));
    HIP_COPY(hipMemcpy(h->d_sh_tab4, tab4.data(), tab4.size() * sizeof(double), hipMemcpyHostToDevice));
    h->sh_cbar.assign(cbar, cbar + (size_t)(degree + 1) * (degree + 2) / 2);
    h->sh_sbar.assign(sbar, sbar + (size_t)(degree + 1) * (degree + 2) / 2);
    h->sp.sh_degree = degree;
    h->sp.sh_split = lay.split;
    h->sp.sh_chunk1 = lay.chunk1;
    h->sp.sh_bodies = lay.bodies;
    h->sp.sh_bodies0 = lay.bodies0;
    h->sp.sh_bodies1 = lay.bodies1;
    // Form of the harmonics kernel.  Below two 64-lane waves per SIMD (1 024 SIMDs on MI355X) each
    // spacecraft's walk is split over two cooperating waves (form 5), above that one wave walks it
    // (form 4); the two give bit-identical results.  BSKGPU_SH_FORM=1|4|5 forces a form (measurement).
    int n_cu = 256;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) n_cu = prop.multiProcessorCount;
    }
    h->policy.sh_form = (h->n < 2 * (4 * n_cu) * 64) ? bsk::FORM_SH_DPP2 : bsk::FORM_SH_DPP;
    if (const char* f = std::getenv("BSKGPU_SH_FORM")) {
        const int v = std::atoi(f);
        if (v == 1 || v == 4 || v == 5) h->policy.sh_form = v;
    }
    h->sp.sh_tab = h->policy.sh_form == bsk::FORM_SINGLE ? h->d_sh_tab : h->d_sh_tab4;
    h->last.form = h->policy.sh_form;     // (every launch of a harmonics handle runs it)
    return BSK_OK;
}

int bsk_n_fields(const bsk_handle* h) { return h ? h->nf : BSK_EINVAL; }

int bsk_reset(bsk_handle* h, const uint8_t* mask, const double* ic) {
    if (!h || !ic) return fail(BSK_EINVAL, "handle/ic is NULL");
    DeviceGuard guard(h->device);
    if (h->stepped) { int rc = snapshot_stats(h); if (rc) return rc; }   // the last step's batch scalars, before its rewards are overwritten
    const size_t row = (size_t)h->n * sizeof(double);
    const double* ic_charge = ic + (size_t)(BSK_NF_BASE + h->cfg.n_rw + BSK_T_CHARGE) * h->n;
    if (!mask) {
        h->charge_pos = true;
        for (int i = 0; i < h->n; ++i) h->charge_pos = h->charge_pos && ic_charge[i] > 0.0;
        HIP_COPY(hipMemcpy2DAsync(h->d_state, (size_t)h->stride * sizeof(double), ic, row, row, h->nf,
                                 hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemsetAsync(h->d_cnt, 0, (size_t)h->ostride * sizeof(int2), h->stream));
        HIP_TRY(bsk::launch_init_outputs(h->d_state, h->stride, nullptr, h->n, reset_out(h), h->stream));
        { int rc = seal_stats(h); if (rc) return rc; }
        HIP_SYNC(hipStreamSynchronize(h->stream));
        return BSK_OK;
    }
    std::vector<int> idx;
    for (int i = 0; i < h->n; ++i)
        if (mask[i]) { idx.push_back(i); h->charge_pos = h->charge_pos && ic_charge[i] > 0.0; }
    const size_t m = idx.size();
    if (m == 0) return BSK_OK;
    std::vector<double> compact(m * h->nf);
    for (int f = 0; f < h->nf; ++f)
        for (size_t t = 0; t < m; ++t) compact[(size_t)f * m + t] = ic[(size_t)f * h->n + idx[t]];
    int rc = ensure_stage(h, m);
    if (rc) return rc;
    HIP_COPY(hipMemcpyAsync(h->d_ic_stage, compact.data(), compact.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_COPY(hipMemcpyAsync(h->d_idx_stage, idx.data(), m * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(bsk::launch_scatter_reset(h->d_state, h->stride, h->nf, h->d_ic_stage, h->d_idx_stage, (int)m, h->d_cnt, h->stream));
    HIP_TRY(bsk::launch_init_outputs(h->d_state, h->stride, h->d_idx_stage, (int)m, reset_out(h), h->stream));
    { int rc = seal_stats(h); if (rc) return rc; }
    HIP_SYNC(hipStreamSynchronize(h->stream));
    return BSK_OK;
}

int bsk_step(bsk_handle* h, const int32_t* actions, int substeps) {
    if (!h || !actions) return fail(BSK_EINVAL, "handle/actions is NULL");
    if (substeps < 1) return fail(BSK_EINVAL, "substeps must be >= 1");
    DeviceGuard guard(h->device);
    HIP_COPY(hipMemcpyAsync(h->d_act, actions, (size_t)h->n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    return do_step(h, h->d_act, substeps, 1);
}

int bsk_step_device(bsk_handle* h, const int32_t* d_actions, int substeps) {
    if (!h || !d_actions) return fail(BSK_EINVAL, "handle/actions is NULL");
    if (substeps < 1) return fail(BSK_EINVAL, "substeps must be >= 1");
    DeviceGuard guard(h->device);
    return do_step(h, d_actions, substeps, 1);
}

int bsk_step_device_i64(bsk_handle* h, const int64_t* d_actions, int substeps) {
    if (!h || !d_actions) return fail(BSK_EINVAL, "handle/actions is NULL");
    if (substeps < 1) return fail(BSK_EINVAL, "substeps must be >= 1");
    DeviceGuard guard(h->device);
    return do_step(h, d_actions, substeps, 0);       // the kernel reads the low word of every little-endian int64
}

int bsk_step_n(bsk_handle* h, const int32_t* d_actions, int32_t constant_action, int substeps, int n_steps,
               double* d_obs_hist, double* d_reward_hist, uint8_t* d_reason_hist) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    if (substeps < 1 || n_steps < 1) return fail(BSK_EINVAL, "substeps and n_steps must be >= 1");
    if (!d_actions && (constant_action < 0 || constant_action > 2)) return fail(BSK_EINVAL, "constant_action must be 0, 1 or 2");
    if ((h->cfg.flags & BSK_FLAG_AUTO_RESET) && h->n_pool == 0)
        return fail(BSK_EINVAL, "BSK_FLAG_AUTO_RESET: call bsk_set_ic_pool before stepping");
    DeviceGuard guard(h->device);
    if (!bsk::rollout_available(h->cfg.gravity_model, h->sp.feat)) {
        // The scenario levels, the harmonics, the LDS-scratch level: the env steps stay separate launches of step_kernel (at the
        // reference's 1 800 sub-steps per env step a launch's overhead is 0.2 % of the step; the fused kernel exists where it is not),
        // each followed by a row of the history - all enqueued here, no host visit in between.  Same results by construction.
        if (!d_actions) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)h->d_act, constant_action, (size_t)h->n, h->stream));
        for (int t = 0; t < n_steps; ++t) {
            int rc = do_step(h, d_actions ? (const void*)(d_actions + (size_t)t * h->n) : (const void*)h->d_act, substeps, 1);
            if (rc) return rc;
            HIP_TRY(bsk::launch_hist_row(h->d_obs, h->d_reward, h->d_reason, h->ostride, h->n,
                                         d_obs_hist ? d_obs_hist + (size_t)t * 5 * h->n : nullptr, d_reward_hist ? d_reward_hist + (size_t)t * h->n : nullptr,
                                         d_reason_hist ? d_reason_hist + (size_t)t * h->n : nullptr, h->stream));
        }
        return BSK_OK;
    }
    bsk::StepBuffers b;
    (void)note_capture(h);
    fill_buffers(h, b, nullptr, substeps, 1, false);
    bsk::RolloutBuffers r;
    r.actions = d_actions; r.obs_hist = d_obs_hist; r.reward_hist = d_reward_hist; r.reason_hist = d_reason_hist;
    r.n_steps = n_steps; r.const_action = constant_action;
    hipEvent_t e0, e1;
    { int rc = stamp_events(h, e0, e1); if (rc) return rc; }
    h->last = {bsk::FORM_SINGLE, true, d_actions != nullptr};
    const bsk::RolloutLaunch go{{h->sp, b, h->stream, e0, e1}, r};
    bsk::KernelDesc d;
    HIP_TRY(bsk::dispatch_rollout(h->cfg.gravity_model, h->cfg.n_rw, h->diag, h->last.act, h->block, h->n, &go, &d));
    h->stats_fresh = false;
    h->wave_sums_fresh = false;
    h->stepped = true;
    return BSK_OK;
}

int bsk_get_obs(bsk_handle* h, double* obs, double* reward, uint8_t* done, uint8_t* done_reason) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    DeviceGuard guard(h->device);
    const size_t row = (size_t)h->n * sizeof(double);
    if (obs && h->n == h->ostride) {
        // a batch that fills its stride: the five observation rows are one contiguous block, and the reward row sits right behind them
        // on the device (one allocation) - one plain copy when the host arrays are laid out the same way, two otherwise
        const bool with_reward = reward == obs + 5 * (size_t)h->n;
        HIP_COPY(hipMemcpyAsync(obs, h->d_obs, (with_reward ? 6 : 5) * row, hipMemcpyDeviceToHost, h->stream));
        if (reward && !with_reward) HIP_COPY(hipMemcpyAsync(reward, h->d_reward, row, hipMemcpyDeviceToHost, h->stream));
    } else {
        if (obs)
            HIP_COPY(hipMemcpy2DAsync(obs, row, h->d_obs, (size_t)h->ostride * sizeof(double), row, 5, hipMemcpyDeviceToHost, h->stream));
        if (reward) HIP_COPY(hipMemcpyAsync(reward, h->d_reward, row, hipMemcpyDeviceToHost, h->stream));
    }
    std::vector<unsigned char> why;
    unsigned char* wp = done_reason;
    if (done && !done_reason) { why.resize(h->n); wp = why.data(); }
    if (wp) HIP_COPY(hipMemcpyAsync(wp, h->d_reason, (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
    SYNC_CHECKED(h);
    if (done)
        for (int i = 0; i < h->n; ++i) done[i] = wp[i] != 0;
    return BSK_OK;
}

int bsk_get_obs_state(bsk_handle* h, double* obs, double* reward, uint8_t* done_reason, double* state) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    DeviceGuard guard(h->device);
    const size_t row = (size_t)h->n * sizeof(double), pitch = (size_t)h->stride * sizeof(double), opitch = (size_t)h->ostride * sizeof(double);
    if (obs) HIP_COPY(hipMemcpy2DAsync(obs, row, h->d_obs, opitch, row, 5, hipMemcpyDeviceToHost, h->stream));
    if (reward) HIP_COPY(hipMemcpyAsync(reward, h->d_reward, row, hipMemcpyDeviceToHost, h->stream));
    if (done_reason) HIP_COPY(hipMemcpyAsync(done_reason, h->d_reason, (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
    if (state) HIP_COPY(hipMemcpy2DAsync(state, row, h->d_state, pitch, row, h->nf, hipMemcpyDeviceToHost, h->stream));
    SYNC_CHECKED(h);
    return BSK_OK;
}

int bsk_get_obs_rowmajor(bsk_handle* h, double* obs_n5, double* reward, uint8_t* done_reason) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    if (!h->d_obs_rm) return fail(BSK_EINVAL, "bsk_get_obs_rowmajor needs BSK_FLAG_OBS_ROWMAJOR");
    DeviceGuard guard(h->device);
    const size_t row = (size_t)h->n * sizeof(double);
    if (obs_n5) HIP_COPY(hipMemcpyAsync(obs_n5, h->d_obs_rm, 5 * row, hipMemcpyDeviceToHost, h->stream));
    if (reward) HIP_COPY(hipMemcpyAsync(reward, h->d_reward, row, hipMemcpyDeviceToHost, h->stream));
    if (done_reason) HIP_COPY(hipMemcpyAsync(done_reason, h->d_reason, (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
    SYNC_CHECKED(h);
    return BSK_OK;
}

int bsk_get_obs_device(bsk_handle* h, double** d_obs, double** d_reward, uint64_t** d_done_mask, uint8_t** d_done_reason,
                       int64_t* stride) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    if (d_obs) *d_obs = h->d_obs;
    if (d_reward) *d_reward = h->d_reward;
    if (d_done_mask) *d_done_mask = (uint64_t*)h->d_done_mask;
    if (d_done_reason) *d_done_reason = h->d_reason;
    if (stride) *stride = h->ostride;
    return BSK_OK;
}

int bsk_get_stream(bsk_handle* h, void** stream) {
    if (!h || !stream) return fail(BSK_EINVAL, "handle/stream is NULL");
    *stream = (void*)h->stream;
    return BSK_OK;
}

int bsk_get_terminal_obs_device(bsk_handle* h, double** d_term_obs, int32_t** d_episodes) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    if (d_term_obs) *d_term_obs = h->d_term_obs;
    if (d_episodes) *d_episodes = h->d_episodes;
    return BSK_OK;
}

int bsk_get_state_device(bsk_handle* h, double** d_state, int64_t* stride) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    if (d_state) *d_state = h->d_state;
    if (stride) *stride = h->stride;
    return BSK_OK;
}

int bsk_get_batch_stats(bsk_handle* h, double* reward_sum, int64_t* n_done) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    DeviceGuard guard(h->device);
    { int rc = snapshot_stats(h); if (rc) return rc; }
    double s = 0;
    long long d = 0;
    HIP_COPY(hipMemcpyAsync(&s, h->d_stat_sum, sizeof s, hipMemcpyDeviceToHost, h->stream));
    HIP_COPY(hipMemcpyAsync(&d, h->d_stat_done, sizeof d, hipMemcpyDeviceToHost, h->stream));
    SYNC_CHECKED(h);
    if (reward_sum) *reward_sum = s;
    if (n_done) *n_done = d;
    return BSK_OK;
}

int bsk_get_state(bsk_handle* h, double* state) {
    if (!h || !state) return fail(BSK_EINVAL, "handle/state is NULL");
    DeviceGuard guard(h->device);
    const size_t row = (size_t)h->n * sizeof(double);
    HIP_COPY(hipMemcpy2DAsync(state, row, h->d_state, (size_t)h->stride * sizeof(double), row, h->nf, hipMemcpyDeviceToHost, h->stream));
    SYNC_CHECKED(h);
    return BSK_OK;
}

int bsk_set_state(bsk_handle* h, const double* state) {
    if (!h || !state) return fail(BSK_EINVAL, "handle/state is NULL");
    DeviceGuard guard(h->device);
    h->charge_pos = false;       // (the observation buffers no longer describe this state: the kernel reads the charge again)
    const size_t row = (size_t)h->n * sizeof(double);
    HIP_COPY(hipMemcpy2DAsync(h->d_state, (size_t)h->stride * sizeof(double), state, row, row, h->nf, hipMemcpyHostToDevice, h->stream));
    HIP_SYNC(hipStreamSynchronize(h->stream));
    return BSK_OK;
}

int bsk_get_counters(bsk_handle* h, int32_t* steps, int32_t* ticks) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    DeviceGuard guard(h->device);
    std::vector<int2> tmp(h->n);
    HIP_COPY(hipMemcpyAsync(tmp.data(), h->d_cnt, (size_t)h->n * sizeof(int2), hipMemcpyDeviceToHost, h->stream));
    HIP_SYNC(hipStreamSynchronize(h->stream));
    for (int i = 0; i < h->n; ++i) {
        if (steps) steps[i] = tmp[i].x & 0xFFFFF;  // high bits carry the FSW phase
        if (ticks) ticks[i] = tmp[i].y;
    }
    return BSK_OK;
}

int bsk_set_counters(bsk_handle* h, const int32_t* steps, const int32_t* ticks) {
    if (!h || !steps || !ticks) return fail(BSK_EINVAL, "handle/steps/ticks is NULL");
    DeviceGuard guard(h->device);
    std::vector<int2> tmp(h->n);
    for (int i = 0; i < h->n; ++i) {
        if (steps[i] < 0 || steps[i] > 0xFFFFF || ticks[i] < 0) return fail(BSK_EINVAL, "steps must be in 0..2^20-1 and ticks >= 0");
        tmp[i].x = steps[i] | ((ticks[i] % h->cfg.fsw_every) << 20);
        tmp[i].y = ticks[i];
    }
    HIP_COPY(hipMemcpyAsync(h->d_cnt, tmp.data(), (size_t)h->n * sizeof(int2), hipMemcpyHostToDevice, h->stream));
    HIP_SYNC(hipStreamSynchronize(h->stream));
    return BSK_OK;
}

int bsk_set_ic_pool(bsk_handle* h, int n_pool, const double* ic_pool) {
    if (!h || !ic_pool) return fail(BSK_EINVAL, "handle/ic_pool is NULL");
    if (!(h->cfg.flags & BSK_FLAG_AUTO_RESET)) return fail(BSK_EINVAL, "handle was not created with BSK_FLAG_AUTO_RESET");
    if (n_pool < 1) return fail(BSK_EINVAL, "n_pool must be >= 1");
    DeviceGuard guard(h->device);
    HIP_SYNC(hipStreamSynchronize(h->stream));
    int rc = ensure_pool_buffers(h, n_pool);
    if (rc) return rc;
    HIP_COPY(hipMemcpy(h->d_pool, ic_pool, (size_t)h->nf * n_pool * sizeof(double), hipMemcpyHostToDevice));
    h->n_pool = n_pool;
    h->pool_charge_pos = true;
    for (int k = 0; k < n_pool; ++k) h->pool_charge_pos = h->pool_charge_pos && ic_pool[(size_t)(BSK_NF_BASE + h->cfg.n_rw + BSK_T_CHARGE) * n_pool + k] > 0.0;
    return BSK_OK;
}

static int ensure_pool_buffers(bsk_handle* h, int n_pool) {
    if (h->d_pool && h->pool_cap < n_pool) { (void)hipFree(h->d_pool); h->d_pool = nullptr; h->n_pool = 0; h->pool_cap = 0; }
    if (!h->d_pool) {
        HIP_TRY(hipMalloc(&h->d_pool, (size_t)h->nf * n_pool * sizeof(double)));
        h->pool_cap = n_pool;
    }
    if (!h->d_term_obs) {
        HIP_TRY(hipMalloc(&h->d_term_obs, (size_t)5 * h->ostride * sizeof(double)));
        HIP_TRY(hipMemset(h->d_term_obs, 0, (size_t)5 * h->ostride * sizeof(double)));
        HIP_TRY(hipMalloc(&h->d_episodes, (size_t)h->ostride * sizeof(int)));
        HIP_TRY(hipMemset(h->d_episodes, 0, (size_t)h->ostride * sizeof(int)));
    }
    return BSK_OK;
}

int bsk_sample_ic_pool(bsk_handle* h, int n_pool, uint64_t seed) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    if (!(h->cfg.flags & BSK_FLAG_AUTO_RESET)) return fail(BSK_EINVAL, "handle was not created with BSK_FLAG_AUTO_RESET");
    if (n_pool < 1) return fail(BSK_EINVAL, "n_pool must be >= 1");
    DeviceGuard guard(h->device);
    HIP_SYNC(hipStreamSynchronize(h->stream));
    int rc = ensure_pool_buffers(h, n_pool);
    if (rc) return rc;
    HIP_TRY(bsk::launch_sample_pool(h->d_pool, n_pool, h->cfg.n_rw, (unsigned long long)seed, h->cfg.mu, h->stream));
    HIP_SYNC(hipStreamSynchronize(h->stream));
    h->n_pool = n_pool;
    h->pool_charge_pos = true;       // the sampler draws U(8, 20) W h
    return BSK_OK;
}

int bsk_reset_from_pool(bsk_handle* h, const uint8_t* mask) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    if (h->n_pool == 0) return fail(BSK_EINVAL, "no IC pool staged (bsk_set_ic_pool / bsk_sample_ic_pool)");
    DeviceGuard guard(h->device);
    if (h->stepped) { int rc = snapshot_stats(h); if (rc) return rc; }   // the last step's batch scalars, before its rewards are overwritten
    unsigned char* d_mask = nullptr;
    if (mask) {
        if (!h->d_mask_stage) HIP_TRY(hipMalloc(&h->d_mask_stage, (size_t)h->ostride));   // kept for the handle's lifetime
        d_mask = h->d_mask_stage;
        HIP_COPY(hipMemcpyAsync(d_mask, mask, (size_t)h->n, hipMemcpyHostToDevice, h->stream));
    }
    HIP_TRY(bsk::launch_reset_from_pool(h->d_state, h->stride, h->nf, h->d_pool, h->n_pool, d_mask, h->n, h->d_cnt,
                                        h->d_episodes, h->env_base, reset_out(h), h->stream));
    h->charge_pos = (mask ? h->charge_pos : true) && h->pool_charge_pos;
    { int rc = seal_stats(h); if (rc) return rc; }
    HIP_SYNC(hipStreamSynchronize(h->stream));
    return BSK_OK;
}

int bsk_reset_from_pool_device(bsk_handle* h, const uint8_t* d_mask) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    if (h->n_pool == 0) return fail(BSK_EINVAL, "no IC pool staged (bsk_set_ic_pool / bsk_sample_ic_pool)");
    DeviceGuard guard(h->device);
    if (h->stepped) { int rc = snapshot_stats(h); if (rc) return rc; }   // the last step's batch scalars, before its rewards are overwritten
    HIP_TRY(bsk::launch_reset_from_pool(h->d_state, h->stride, h->nf, h->d_pool, h->n_pool, d_mask, h->n, h->d_cnt,
                                        h->d_episodes, h->env_base, reset_out(h), h->stream));
    h->charge_pos = (d_mask ? h->charge_pos : true) && h->pool_charge_pos;
    { int rc = seal_stats(h); if (rc) return rc; }
    return BSK_OK;       // asynchronous on the handle's stream: no host data, no copy, no synchronisation
}

int bsk_reset_from_pool_shared(bsk_handle* h, int envs_per_member, const uint64_t* d_epoch, const uint8_t* d_mask) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    if (h->n_pool == 0) return fail(BSK_EINVAL, "no IC pool staged (bsk_set_ic_pool / bsk_sample_ic_pool)");
    if (envs_per_member < 1) return fail(BSK_EINVAL, "bsk_reset_from_pool_shared: envs_per_member must be >= 1");
    DeviceGuard guard(h->device);
    if (h->stepped) { int rc = snapshot_stats(h); if (rc) return rc; }   // the last step's batch scalars, before its rewards are overwritten
    HIP_TRY(bsk::launch_reset_from_pool_shared(h->d_state, h->stride, h->nf, h->d_pool, h->n_pool, d_mask, h->n, h->d_cnt, h->d_episodes,
                                               h->env_base, (unsigned)envs_per_member, (const unsigned long long*)d_epoch, reset_out(h),
                                               h->stream));
    h->charge_pos = (d_mask ? h->charge_pos : true) && h->pool_charge_pos;
    { int rc = seal_stats(h); if (rc) return rc; }
    return BSK_OK;       // asynchronous on the handle's stream: no host data, no copy, no synchronisation
}

int bsk_get_episode_device(bsk_handle* h, double** d_ep_return, double** d_term_return, int32_t** d_term_len, uint8_t** d_done,
                           double** d_obs_rowmajor) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    if (d_ep_return) *d_ep_return = h->d_ep_return;
    if (d_term_return) *d_term_return = h->d_term_return;
    if (d_term_len) *d_term_len = h->d_term_len;
    if (d_done) *d_done = h->d_done;
    if (d_obs_rowmajor) *d_obs_rowmajor = h->d_obs_rm;
    return BSK_OK;
}

int bsk_set_halves_form(bsk_handle* h, int mode) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    if (mode < -1 || mode > 1) return fail(BSK_EINVAL, "bsk_set_halves_form: mode must be -1 (size window), 0 (never) or 1 (every launch the form is complete for)");
    h->policy.halves_mode = mode;
    return BSK_OK;
}

int bsk_set_step_stats(bsk_handle* h, int on) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    h->step_stats = on != 0;
    return BSK_OK;
}

int bsk_get_batch_stats_device(bsk_handle* h, double** d_stats2) {
    if (!h || !d_stats2) return fail(BSK_EINVAL, "handle/d_stats2 is NULL");
    DeviceGuard guard(h->device);
    { int rc = snapshot_stats(h); if (rc) return rc; }
    *d_stats2 = h->d_stats2;
    return BSK_OK;       // asynchronous: the two doubles are valid once the handle's stream has reached this point
}

int bsk_debug_words(bsk_handle* h, uint64_t* words) {
    if (!h || !words) return fail(BSK_EINVAL, "handle/words is NULL");
    DeviceGuard guard(h->device);
    HIP_COPY(hipMemcpyAsync(words, h->d_dbg, (size_t)((h->n + 63) / 64) * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    SYNC_CHECKED(h);
    return BSK_OK;
}

int bsk_debug_counters(int64_t* n_copies, int64_t* n_syncs) {
    if (n_copies) *n_copies = g_n_copies.load(std::memory_order_relaxed);
    if (n_syncs) *n_syncs = g_n_syncs.load(std::memory_order_relaxed);
    return BSK_OK;
}

int bsk_get_ic_pool(bsk_handle* h, double* ic_pool) {
    if (!h || !ic_pool) return fail(BSK_EINVAL, "handle/ic_pool is NULL");
    if (h->n_pool == 0) return fail(BSK_EINVAL, "no IC pool staged (bsk_set_ic_pool / bsk_sample_ic_pool)");
    DeviceGuard guard(h->device);
    HIP_SYNC(hipStreamSynchronize(h->stream));
    HIP_COPY(hipMemcpy(ic_pool, h->d_pool, (size_t)h->nf * h->n_pool * sizeof(double), hipMemcpyDeviceToHost));
    return BSK_OK;
}

int bsk_get_terminal_obs(bsk_handle* h, double* term_obs, int32_t* episodes) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    if (!h->d_term_obs) return fail(BSK_EINVAL, "no IC pool staged (bsk_set_ic_pool)");
    DeviceGuard guard(h->device);
    const size_t row = (size_t)h->n * sizeof(double);
    if (term_obs)
        HIP_COPY(hipMemcpy2DAsync(term_obs, row, h->d_term_obs, (size_t)h->ostride * sizeof(double), row, 5, hipMemcpyDeviceToHost, h->stream));
    if (episodes) HIP_COPY(hipMemcpyAsync(episodes, h->d_episodes, (size_t)h->n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    SYNC_CHECKED(h);
    return BSK_OK;
}

int bsk_set_sim_time(bsk_handle* h, double t) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    h->sim_time = t;
    for (int i = 0; i < 3; ++i) h->sp.pc.sun_r0[i] = h->cfg.sun_r0[i] + h->cfg.sun_v[i] * t;
    return BSK_OK;
}

int bsk_fork_device(bsk_handle* dst, bsk_handle* src, const int32_t* d_map) {
    if (!dst || !src || !d_map) return fail(BSK_EINVAL, "dst/src/d_map is NULL");
    DeviceGuard guard(dst->device);
    return do_fork(dst, src, d_map);      // asynchronous on dst's stream: no copy, no synchronisation
}

int bsk_fork(bsk_handle* dst, bsk_handle* src, const int32_t* map) {
    if (!dst || !src || !map) return fail(BSK_EINVAL, "dst/src/map is NULL");
    DeviceGuard guard(dst->device);
    if (!dst->d_map_stage) HIP_TRY(hipMalloc(&dst->d_map_stage, (size_t)dst->ostride * sizeof(int)));   // kept for the handle's lifetime
    HIP_COPY(hipMemcpyAsync(dst->d_map_stage, map, (size_t)dst->n * sizeof(int), hipMemcpyHostToDevice, dst->stream));
    int rc = do_fork(dst, src, dst->d_map_stage);
    if (rc) {
        HIP_SYNC(hipStreamSynchronize(dst->stream));     // (the pageable map must have left before the caller may free it)
        return rc;
    }
    SYNC_CHECKED(dst);
    return BSK_OK;
}

// what bsk_select_branches and bsk_select_branches_boot refuse alike, before any launch
static int check_select(const double* d_reward_hist, const uint8_t* d_reason_hist, const int32_t* d_first_action, int n_steps, int n_branch,
                        int group, const int32_t* d_best_action) {
    if (!d_reward_hist || !d_reason_hist || !d_first_action || !d_best_action)
        return fail(BSK_EINVAL, "reward_hist/reason_hist/first_action/best_action is NULL");
    if (n_steps < 1 || n_branch < 1 || group < 1) return fail(BSK_EINVAL, "n_steps, n_branch and group must be >= 1");
    if (n_branch % group != 0) return fail(BSK_EINVAL, "n_branch must be a multiple of group");
    return BSK_OK;
}

int bsk_select_branches(const double* d_reward_hist, const uint8_t* d_reason_hist, const int32_t* d_first_action, int n_steps, int n_branch,
                        int group, double gamma, double* d_values, double* d_best_value, int32_t* d_best_action, void* stream) {
    if (int rc = check_select(d_reward_hist, d_reason_hist, d_first_action, n_steps, n_branch, group, d_best_action)) return rc;
    HIP_TRY(bsk::launch_select(d_reward_hist, d_reason_hist, d_first_action, n_steps, n_branch, group, gamma, nullptr, d_values, d_best_value,
                               d_best_action, (hipStream_t)stream));
    return BSK_OK;
}

int bsk_select_branches_boot(const double* d_reward_hist, const uint8_t* d_reason_hist, const int32_t* d_first_action, int n_steps,
                             int n_branch, int group, double gamma, const float* d_leaf_value, double* d_values, double* d_best_value,
                             int32_t* d_best_action, void* stream) {
    if (int rc = check_select(d_reward_hist, d_reason_hist, d_first_action, n_steps, n_branch, group, d_best_action)) return rc;
    if (!d_leaf_value) return fail(BSK_EINVAL, "leaf_value is NULL");
    HIP_TRY(bsk::launch_select(d_reward_hist, d_reason_hist, d_first_action, n_steps, n_branch, group, gamma, d_leaf_value, d_values,
                               d_best_value, d_best_action, (hipStream_t)stream));
    return BSK_OK;
}

// what bsk_beam_select and bsk_beam_select_boot refuse alike, before any launch
static int check_beam(const double* d_reward, const uint8_t* d_reason, int n_roots, int width, int level, double weight,
                      const bsk_beam_slot* d_in, const bsk_beam_slot* d_out, const int32_t* d_map, const double* d_best_value,
                      const int32_t* d_best_action) {
    if (!d_reward || !d_reason || !d_out || !d_map || !d_best_value || !d_best_action || (!d_in && level != 0))
        return fail(BSK_EINVAL, "reward/reason/out/map/best_value/best_action is NULL, or in is NULL at a level above 0");
    if (width < 1 || width > BSK_BEAM_MAX_WIDTH) return fail(BSK_EINVAL, "width must be in 1..81");
    if (n_roots < 1 || level < 0) return fail(BSK_EINVAL, "n_roots must be >= 1 and level >= 0");
    if ((int64_t)3 * width * n_roots >= ((int64_t)1 << 31)) return fail(BSK_EINVAL, "3 * width * n_roots candidates must stay below 2^31");
    if (!std::isfinite(weight)) return fail(BSK_EINVAL, "weight must be finite");
    if (d_in == d_out) return fail(BSK_EINVAL, "in and out must be distinct slot buffers");
    return BSK_OK;
}

int bsk_beam_select(const double* d_reward, const uint8_t* d_reason, int n_roots, int width, int level, double weight,
                    const bsk_beam_slot* d_in, bsk_beam_slot* d_out, int32_t* d_map, double* d_best_value, int32_t* d_best_action,
                    void* stream) {
    if (int rc = check_beam(d_reward, d_reason, n_roots, width, level, weight, d_in, d_out, d_map, d_best_value, d_best_action)) return rc;
    HIP_TRY(bsk::launch_beam(d_reward, d_reason, n_roots, width, level, weight, 0.0, nullptr, d_in, d_out, d_map, nullptr, d_best_value,
                             d_best_action, (hipStream_t)stream));
    return BSK_OK;
}

int bsk_beam_select_boot(const double* d_reward, const uint8_t* d_reason, int n_roots, int width, int level, double weight,
                         double boot_weight, const float* d_leaf_value, const bsk_beam_slot* d_in, bsk_beam_slot* d_out, int32_t* d_map,
                         double* d_key, double* d_best_value, int32_t* d_best_action, void* stream) {
    if (int rc = check_beam(d_reward, d_reason, n_roots, width, level, weight, d_in, d_out, d_map, d_best_value, d_best_action)) return rc;
    if (!d_leaf_value) return fail(BSK_EINVAL, "leaf_value is NULL");
    if (!std::isfinite(boot_weight)) return fail(BSK_EINVAL, "boot_weight must be finite");
    HIP_TRY(bsk::launch_beam(d_reward, d_reason, n_roots, width, level, weight, boot_weight, d_leaf_value, d_in, d_out, d_map, d_key,
                             d_best_value, d_best_action, (hipStream_t)stream));
    return BSK_OK;
}
int bsk_set_env_base(bsk_handle* h, int64_t env_base) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    if (env_base < 0 || env_base > 0xFFFFFFFFll) return fail(BSK_EINVAL, "env_base must be in 0..2^32-1");
    h->env_base = (unsigned)env_base;
    return BSK_OK;
}

int bsk_sync(bsk_handle* h) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    DeviceGuard guard(h->device);
    SYNC_CHECKED(h);
    return BSK_OK;
}

int bsk_profile_begin(bsk_handle* h, int capacity) {
    if (!h || capacity < 1) return fail(BSK_EINVAL, "handle is NULL or capacity < 1");
    DeviceGuard guard(h->device);
    while ((int)h->ev.size() < 2 * capacity) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        h->ev.push_back(e);
    }
    h->ev_used = 0;
    h->ev_seq = 0;
    h->prof = true;
    return BSK_OK;
}

int bsk_profile_set_stride(bsk_handle* h, int stride) {
    if (!h || stride < 1) return fail(BSK_EINVAL, "handle is NULL or stride < 1");
    h->ev_stride = stride;
    return BSK_OK;
}

int bsk_profile_end_samples(bsk_handle* h, double* mean_kernel_ms, int* n_launches, float* samples_ms, int cap) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    DeviceGuard guard(h->device);
    h->prof = false;
    HIP_SYNC(hipStreamSynchronize(h->stream));
    double tot = 0.0;
    const int n = h->ev_used / 2;
    for (int k = 0; k < n; ++k) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev[2 * k], h->ev[2 * k + 1]));
        tot += ms;
        if (samples_ms && k < cap) samples_ms[k] = ms;
    }
    if (mean_kernel_ms) *mean_kernel_ms = n ? tot / n : 0.0;
    if (n_launches) *n_launches = n;
    h->ev_used = 0;
    return BSK_OK;
}

int bsk_profile_end(bsk_handle* h, double* mean_kernel_ms, int* n_launches) {
    return bsk_profile_end_samples(h, mean_kernel_ms, n_launches, nullptr, 0);
}

int bsk_kernel_info(bsk_handle* h, char* name, int name_cap, int* vgprs, int* lds_bytes, int* block, int* grid) {
    if (!h) return fail(BSK_EINVAL, "handle is NULL");
    DeviceGuard guard(h->device);
    const int g = h->cfg.gravity_model, form = h->last.form;
    bsk::KernelDesc d;
    if (h->last.rollout) (void)bsk::dispatch_rollout(g, h->cfg.n_rw, h->diag, h->last.act, h->block, h->n, nullptr, &d);
    else (void)bsk::dispatch_step(g, h->cfg.n_rw, h->diag, h->sp.feat, form, h->block, h->n, nullptr, &d);
    if (!d.fn) return fail(BSK_EINVAL, "no kernel variant for this config");
    hipFuncAttributes at;
    HIP_TRY(hipFuncGetAttributes(&at, d.fn));
    static const char* const GRAV[] = {"PM", "PM_J2"};                                              // BSK_GRAV_PM, _PM_J2
    static const char* const SH_FORM[] = {"", "SH/scalar", "", "", "SH/dpp", "SH/dpp2"};            // BSK_GRAV_SH, by form
    static const char* const LEVEL[] = {",lds-scratch", "", ",power", ",scenario", ",scenario/generic-facets"};  // FEAT_LDSS ..
    static const char* const SPLIT[] = {"", "", ",pair", ",tri", "", "", ",halves"};               // by form
    const char* hub = h->diag ? "diag" : "full";
    if (name && name_cap > 0 && h->last.rollout)
        std::snprintf(name, name_cap, "rollout_kernel<%s,%d,%s,%s>", GRAV[g], h->cfg.n_rw, hub, h->last.act ? "actions" : "constant");
    else if (name && name_cap > 0)
        std::snprintf(name, name_cap, "step_kernel<%s,%d,%s%s%s>", g == BSK_GRAV_SH ? SH_FORM[form] : GRAV[g], h->cfg.n_rw, hub,
                      LEVEL[h->sp.feat - bsk::FEAT_LDSS], SPLIT[form]);
    if (vgprs) *vgprs = at.numRegs;
    if (lds_bytes) *lds_bytes = (int)at.sharedSizeBytes;
    if (block) *block = d.shape.block;
    if (grid) *grid = d.shape.grid;
    return BSK_OK;
}

}  // extern "C"
