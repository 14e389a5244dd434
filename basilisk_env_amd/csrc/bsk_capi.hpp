// bsk_capi.hpp — what the translation units of the C-ABI share (bsk_capi.hip: the environment handle; bsk_capi_policy.hip: policy,
// population, observation statistics; bsk_capi_es.hip: evolution strategy - what those two share beyond this: bsk_capi_policy.hpp;
// bsk_config.hip: the configuration arithmetic).  Internal: not installed, nothing here is exported - everything that crosses a
// translation unit lives in bsk::capi, a namespace of hidden visibility.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>
#include <vector>

#include "../../include/bskgpu.h"
#include "bsk_aux.hpp"
#include "bsk_launch.hpp"

namespace bsk { namespace capi __attribute__((visibility("hidden"))) {

// bsk_last_error's string and the failure every entry point returns through (one definition of each: bsk_capi.hip)
extern thread_local std::string g_err;
int fail(int code, const std::string& msg);

// how many copies / stream synchronisations this library has issued (bsk_debug_counters: tests assert that the
// device-resident entry points issue none)
extern std::atomic<long long> g_n_copies, g_n_syncs;

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
        else prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};
// Admission of a device, for everything the library creates on one: BSK_ENODEV unless device_id names a visible gfx950 (there is
// no CPU path).  prop: where the caller wants the device's properties.
int open_device(int device_id, hipDeviceProp_t* prop = nullptr);

// bsk_capi.hip, for the rollouts of bsk_capi_policy.hip.  check_steppable: what every step refuses before anything is enqueued
// (harmonics without their table, auto-reset without a pool).  do_step: one launch of the step kernel on d_actions (act_shift 1:
// int32 actions, 0: the low words of int64 ones).
int check_steppable(const bsk_handle* h);
int do_step(bsk_handle* h, const void* d_actions, int substeps, int act_shift);

// bsk_config.hip: pure arithmetic, no HIP runtime call
int validate(const bsk_config& c);
int build_params(const bsk_config& c, bsk::StepParams& p, bsk::ColdCfg& k, bool& diag);
void build_sh_table(int d, const double* cbar, const double* sbar, std::vector<double>& tab);
// how build_sh_table_dpp cut the walk in two halves (see there)
struct ShLayout {
    int split, chunk1, bodies, bodies0, bodies1;
};
ShLayout build_sh_table_dpp(int d, const double* cbar, const double* sbar, std::vector<double>& tab);

} }  // namespace bsk::capi

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return ::bsk::capi::fail(e_ == hipErrorOutOfMemory ? BSK_ENOMEM : BSK_EHIP,                              \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                             \
    } while (0)
#define HIP_COPY(expr) do { ::bsk::capi::g_n_copies.fetch_add(1, std::memory_order_relaxed); HIP_TRY(expr); } while (0)
#define HIP_SYNC(expr) do { ::bsk::capi::g_n_syncs.fetch_add(1, std::memory_order_relaxed); HIP_TRY(expr); } while (0)

struct bsk_handle {
    bsk_config cfg;
    bsk::StepParams sp;
    bsk::ColdCfg cold;
    bool diag = false;
    bsk::ColdCfg* d_cold = nullptr;
    int n = 0, nf = 0, device = 0, block = 64;
    int64_t stride = 0;      // of the state slab's field rows (padded: bsk_create)
    int64_t ostride = 0;     // of the observation / terminal-observation rows and the size of every per-env array
    hipStream_t stream = nullptr;
    bool own_stream = false;
    double* d_state = nullptr;
    int2* d_cnt = nullptr;
    int* d_act = nullptr;
    double* d_obs = nullptr;
    double* d_reward = nullptr;
    unsigned long long* d_done_mask = nullptr;
    unsigned char* d_reason = nullptr;
    double* d_stat_sum = nullptr;
    long long* d_stat_done = nullptr;
    double* d_wave_sum = nullptr;              // stats_kernel scratch: one reward sum per 64 envs
    unsigned* d_done_part = nullptr;           // stats_kernel scratch: finished envs per first-level workgroup
    // masked-reset staging
    double* d_ic_stage = nullptr;
    int* d_idx_stage = nullptr;
    unsigned char* d_mask_stage = nullptr;
    size_t stage_cap = 0;
    double* d_sh_tab = nullptr;    // scalar-load stream (form 1)
    double* d_sh_tab4 = nullptr;   // DPP-broadcast stream (forms 4 and 5, default)
    double* d_pool = nullptr;
    double* d_term_obs = nullptr;
    int* d_episodes = nullptr;
    int n_pool = 0, pool_cap = 0;
    // profiling
    std::vector<hipEvent_t> ev;
    int ev_used = 0;
    int ev_stride = 1, ev_seq = 0;
    hipEvent_t ev_warm[2] = {nullptr, nullptr};
    bool prof = false;
    double sim_time = 0.0;
    unsigned env_base = 0;   // global index of env 0 (bsk_set_env_base)
    // device-resident surface (BSK_FLAG_EPISODE_STATS / BSK_FLAG_OBS_ROWMAJOR)
    double* d_ep_return = nullptr;
    double* d_term_return = nullptr;
    int* d_term_len = nullptr;
    unsigned char* d_done = nullptr;
    double* d_obs_rm = nullptr;
    unsigned long long* d_dbg = nullptr;   // one word per wave for probe builds (bsk_probes.hpp)
    unsigned long long* d_seal = nullptr;   // [3] what env 0's counters were behind the last reset entry point (bsk_aux.hip: stats_sealed)
    double* d_stats2 = nullptr;   // {sum of rewards, number of done envs} of the last step, as two doubles (all-reduce operand)
    bool stats_fresh = false;     // d_stat_sum / d_stat_done / d_stats2 hold the LAST STEP's batch scalars (snapshot_stats)
    bool step_stats = false;      // bsk_set_step_stats: step launches write d_wave_sum themselves (a request = the join kernel alone)
    bool wave_sums_fresh = false; // ... and the last launch that wrote rewards did so
    bool stepped = false;         // some step has run since the handle was created
    // A launch of this handle has been recorded into a HIP graph (note_capture): replays advance the device without this
    // host-side state, so from then on nothing evaluated at enqueue time is trusted - the batch scalars are formed again
    // whenever asked for (stats_fresh ignored) and the bare levels read the battery charge again (static_charge off).
    bool replayable = false;
    // error word the kernels can raise (page-locked host memory, device-visible): checked by every synchronising entry point
    int* h_err = nullptr;
    // bare levels: no spacecraft of the batch / of the reset pool started its episode with an empty battery (bsk_launch.hpp:
    // StepArgs::static_charge).  Known after a reset of the whole batch; withdrawn by bsk_set_state until the next one.
    bool charge_pos = false, pool_charge_pos = false;
    // Form policy of the step kernel (choose_form).  Pair form (bsk_device.hpp: PairLds): launches of >= pair_min_substeps sub-steps
    // of batches of <= pair_max_envs spacecraft where it is built (power / full-scenario levels, point mass or J2, diagonal hub).
    // Measured (profiles/r03/pair_form.txt): -13 % per env step up to one pair per CU (16 384 spacecraft), level with the
    // single-wave form up to three pairs per CU, 7 % slower at four (65 536).  Three-wave form (bsk_device.hpp: TriX): the pair form
    // with the dynamics wave cut into a translational and a rotational wave; full-scenario level only, preferred over the pair form
    // where both apply (profiles/r03/tri_form.txt: -16 % against the pair form up to one workgroup per CU, twice the time above).
    // Halves form (bsk_device.hpp: HalvesLds): one-sub-step launches of the bare point-mass / J2 kernels with wheels, nav_lag and no
    // IC pool, for batches of halves_min_envs..halves_max_envs spacecraft.
    // bsk_set_halves_form (halves_mode): -1 that window, 0 never, 1 every launch the form is complete for, at any size.
    // BSKGPU_PAIR / BSKGPU_TRI = 0 | 1 force a form off / on for every launch (bsk_create).  Harmonics run sh_form (bsk_set_gravity_sh).
    struct {
        bool pair_ok = false, tri_ok = false;
        int pair_min_substeps = 16, pair_max_envs = 16384;
        int tri_min_substeps = 16, tri_max_envs = 16384;
        bool halves_ok = false;
        int halves_min_envs = 1, halves_max_envs = 0;       // (bsk_create: 128 - 256 spacecraft per CU of the device)
        int halves_mode = -1;
        int sh_form = bsk::FORM_SH_DPP;
    } policy;
    // what the last launch ran (bsk_kernel_info): the step kernel in `form`, or bsk_step_n's rollout kernel (with per-step actions)
    struct { int form; bool rollout, act; } last = {bsk::FORM_SINGLE, false, false};
    // the coefficients of the last bsk_set_gravity_sh (bsk_fork_device refuses to fork between handles of different fields)
    std::vector<double> sh_cbar, sh_sbar;
    // bsk_fork_device: the in-handle fork's gather scratch (every per-env buffer a handle can have, one allocation, kept for the
    // handle's lifetime), the host map's staging buffer, and the events that order two handles' streams around a fork
    bsk::ForkSide fork_scratch = {};
    void* d_fork_block = nullptr;
    int* d_map_stage = nullptr;
    hipEvent_t ev_fork_in = nullptr, ev_fork_out = nullptr;
};
