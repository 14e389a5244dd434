"""ctypes binding of libbskgpu.so — the C-ABI declared in include/bskgpu.h.

The library is the only compute path: if it is missing, fails to load, or no gfx950 device is
visible, the product raises (:class:`BskGpuUnavailable`); there is no CPU or PyTorch fallback.
"""
import ctypes as C
import os

BSK_ABI_VERSION = 4
BSK_MAX_RW = 4
BSK_MAX_THR = 8

GRAV_PM, GRAV_PM_J2, GRAV_SH = 0, 1, 2
FLAG_SUN_THIRD_BODY, FLAG_POWER, FLAG_DESAT, FLAG_DRAG, FLAG_AUTO_RESET, FLAG_LDS_SCRATCH = 1, 2, 4, 8, 16, 32
FLAG_EPISODE_STATS, FLAG_OBS_ROWMAJOR = 64, 128
DONE_LENGTH, DONE_WHEELS, DONE_BATTERY, DONE_ORBIT = 1, 2, 4, 8

# state field offsets (include/bskgpu.h)
F_R, F_V, F_SIGMA, F_OMEGA, NF_BASE = 0, 3, 6, 9, 12
T_LEXT, T_UCMD, T_CHARGE, T_THR_REM, T_THR_LIM, T_THR_T0, T_THR_CNT, T_UPEND, T_SBR, NF_TAIL = 0, 3, 7, 8, 16, 24, 25, 26, 30, 31


def n_fields(n_rw):
    return NF_BASE + n_rw + NF_TAIL


class BskGpuUnavailable(RuntimeError):
    """libbskgpu.so cannot be used (not built, not loadable, or no gfx950 device)."""


class BskError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libbskgpu error %d: %s" % (code, msg))
        self.code = code


d, i32, u32 = C.c_double, C.c_int32, C.c_uint32


class BskConfig(C.Structure):
    """Mirror of ``struct bsk_config`` (include/bskgpu.h) — field order and types must match."""
    _fields_ = [
        ("abi_version", u32), ("struct_size", u32),
        ("dt", d), ("fsw_every", i32), ("gravity_model", i32), ("sh_degree", i32), ("n_rw", i32),
        ("flags", u32), ("max_length", i32), ("fsw_lag", i32), ("nav_lag", i32),
        ("mu", d), ("req", d), ("j2", d), ("planet_rate", d),
        ("inertia", d * 9), ("mass", d),
        ("gs", (d * 3) * BSK_MAX_RW), ("js", d * BSK_MAX_RW), ("u_max", d), ("u_min", d), ("f_coulomb", d),
        ("K", d), ("P", d), ("sigma_R0N", d * 3), ("ctrl_axes", d * 9),
        ("wheel_limit", d), ("power_max", d), ("reward_mult", d), ("failure_penalty", d), ("r_min", d),
        ("panel_normal", d * 3), ("panel_area", d), ("panel_efficiency", d), ("power_draw", d),
        ("storage_capacity", d), ("solar_flux", d),
        ("sun_r0", d * 3), ("sun_v", d * 3), ("mu_sun", d),
        ("n_thr", i32), ("thr_max_counter", i32), ("thr_pos", (d * 3) * BSK_MAX_THR), ("thr_dir", (d * 3) * BSK_MAX_THR),
        ("thr_max_thrust", d), ("thr_min_fire_time", d), ("thr_min_on_time", d), ("hs_min", d),
        ("base_density", d), ("scale_height", d), ("n_facets", i32), ("pad0_", i32),
        ("facet_area", d * 8), ("facet_cd", d * 8), ("facet_normal", (d * 3) * 8), ("facet_pos", (d * 3) * 8),
    ]

    def copy(self):
        out = BskConfig()
        C.memmove(C.byref(out), C.byref(self), C.sizeof(BskConfig))
        return out


POLICY_RELU, POLICY_TANH = 0, 1
POLICY_GREEDY, POLICY_SAMPLE = 0, 1
ES_SGD, ES_ADAM = 0, 1
ES_SIGMA_FIXED, ES_SIGMA_PGPE = 0, 1
BSK_OUTCOME_COLS = 11         # doubles per member row of bsk_population_set_outcomes (tests/test_outcomes_host.py reads the header)


class BskPolicySpec(C.Structure):
    """Mirror of ``struct bsk_policy_spec`` (include/bskgpu.h)."""
    _fields_ = [
        ("abi_version", u32), ("struct_size", u32),
        ("n_hidden", i32), ("hidden", i32 * 3), ("activation", i32),
        ("has_value", i32), ("v_n_hidden", i32), ("v_hidden", i32 * 3), ("v_activation", i32),
    ]


class BskFitSchedule(C.Structure):
    """Mirror of ``struct bsk_fit_schedule`` (include/bskgpu.h): every pair is {a, b}."""
    _fields_ = [("lr", C.c_double * 2), ("clip", C.c_double * 2), ("clip_vf", C.c_double * 2), ("ent_coef", C.c_double * 2),
                ("total", C.c_uint64), ("kl_stop", C.c_double)]


EXPORTS = [
    "bsk_default_config", "bsk_create", "bsk_destroy", "bsk_set_gravity_sh", "bsk_reset", "bsk_step",
    "bsk_step_device", "bsk_step_device_i64", "bsk_step_n", "bsk_get_episode_device", "bsk_get_batch_stats_device", "bsk_set_step_stats", "bsk_set_halves_form", "bsk_reset_from_pool_device", "bsk_debug_counters", "bsk_debug_words", "bsk_get_obs", "bsk_get_obs_rowmajor", "bsk_get_obs_device", "bsk_get_obs_state", "bsk_get_stream", "bsk_get_terminal_obs_device", "bsk_get_state_device", "bsk_get_batch_stats", "bsk_n_fields",
    "bsk_get_state", "bsk_set_state", "bsk_get_counters", "bsk_set_counters", "bsk_set_ic_pool", "bsk_sample_ic_pool", "bsk_reset_from_pool", "bsk_reset_from_pool_shared", "bsk_get_ic_pool", "bsk_get_terminal_obs", "bsk_set_env_base", "bsk_set_sim_time", "bsk_sync",
    "bsk_fork_device", "bsk_fork", "bsk_select_branches", "bsk_beam_select", "bsk_select_branches_boot", "bsk_beam_select_boot",
    "bsk_policy_n_params", "bsk_policy_create", "bsk_policy_set_params", "bsk_policy_destroy", "bsk_policy_set_rng", "bsk_policy_get_rng",
    "bsk_policy_act", "bsk_policy_value", "bsk_policy_rollout",
    "bsk_population_create", "bsk_population_destroy", "bsk_population_set_rng", "bsk_population_get_rng", "bsk_population_set_params",
    "bsk_population_set_params_device", "bsk_population_get_member", "bsk_population_act", "bsk_population_rollout",
    "bsk_population_set_outcomes", "bsk_es_set_outcome_log", "bsk_es_get_outcome_log",
    "bsk_es_create", "bsk_es_destroy", "bsk_es_ask", "bsk_es_tell", "bsk_es_get_state", "bsk_es_set_state",
    "bsk_es_generation_device", "bsk_es_set_optimizer", "bsk_es_get_moments", "bsk_es_set_moments",
    "bsk_es_set_sigma_adaptation", "bsk_es_get_sigma", "bsk_es_set_sigma",
    "bsk_es_set_log", "bsk_es_get_log", "bsk_es_get_best", "bsk_es_set_best", "bsk_es_best_device",
    "bsk_es_set_validation", "bsk_es_get_validation_log", "bsk_es_get_validated_best", "bsk_es_set_validated_best",
    "bsk_es_validated_best_device", "bsk_es_validation_epochs_device", "bsk_population_set_obs_stats_members",
    "bsk_obs_stats_create", "bsk_obs_stats_destroy", "bsk_obs_stats_accumulate", "bsk_obs_stats_get", "bsk_obs_stats_totals_device",
    "bsk_obs_stats_get_state", "bsk_obs_stats_set_state", "bsk_obs_stats_reset", "bsk_population_set_obs_stats",
    "bsk_policy_set_obs_stats", "bsk_es_apply_obs_norm",
    "bsk_fit_create", "bsk_fit_destroy", "bsk_fit_accumulate", "bsk_fit_step", "bsk_fit_stats_device", "bsk_fit_get_state",
    "bsk_fit_set_state", "bsk_fit_set_lr", "bsk_fit_alive_mask",
    "bsk_gae", "bsk_fit_accumulate_pg", "bsk_fit_pg_stats_device",
    "bsk_adv_normalize_work_bytes", "bsk_adv_normalize", "bsk_fit_set_max_grad_norm", "bsk_fit_grad_norm_device", "bsk_fit_apply_obs_norm",
    "bsk_pg_gather", "bsk_pg_shuffle_advance", "bsk_fit_accumulate_ppo", "bsk_fit_vclip_stats_device",
    "bsk_pg_episodes_work_bytes", "bsk_pg_episodes", "bsk_pg_log_update", "bsk_pg_log_advance",
    "bsk_reward_norm_work_bytes", "bsk_reward_norm",
    "bsk_fit_set_schedule", "bsk_fit_schedule_begin", "bsk_fit_kl_gate", "bsk_fit_schedule_end", "bsk_fit_schedule_device",
    "bsk_fit_get_schedule_state", "bsk_fit_set_schedule_state",
    "bsk_profile_begin", "bsk_profile_set_stride", "bsk_profile_end", "bsk_profile_end_samples", "bsk_calibrate_fp64", "bsk_kernel_info", "bsk_last_error", "bsk_version",
]


def _signatures():
    """Every export of include/bskgpu.h -> (argtypes, restype); ``rc`` is the status that all return but the two strings and the
    six destroys."""
    P, vp, rc, i, i64, u64, f64 = C.POINTER, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_uint64, C.c_double
    spec = P(BskPolicySpec)
    return {
        "bsk_last_error": ([], C.c_char_p), "bsk_version": ([], C.c_char_p),
        "bsk_default_config": ([P(BskConfig), i, i], rc), "bsk_create": ([P(BskConfig), i, i, vp, P(vp)], rc),
        "bsk_destroy": ([vp], None), "bsk_set_gravity_sh": ([vp, i, vp, vp], rc), "bsk_reset": ([vp, vp, vp], rc),
        "bsk_step": ([vp, vp, i], rc), "bsk_step_device": ([vp, vp, i], rc), "bsk_step_device_i64": ([vp, vp, i], rc),
        "bsk_step_n": ([vp, vp, C.c_int32, i, i, vp, vp, vp], rc),
        "bsk_get_episode_device": ([vp, P(vp), P(vp), P(vp), P(vp), P(vp)], rc), "bsk_get_batch_stats_device": ([vp, P(vp)], rc),
        "bsk_set_step_stats": ([vp, i], rc), "bsk_set_halves_form": ([vp, i], rc), "bsk_reset_from_pool_device": ([vp, vp], rc),
        "bsk_debug_counters": ([P(i64), P(i64)], rc), "bsk_debug_words": ([vp, vp], rc),
        "bsk_get_obs": ([vp, vp, vp, vp, vp], rc), "bsk_get_obs_rowmajor": ([vp, vp, vp, vp], rc),
        "bsk_get_obs_device": ([vp, P(vp), P(vp), P(vp), P(vp), P(i64)], rc), "bsk_get_obs_state": ([vp, vp, vp, vp, vp], rc),
        "bsk_get_stream": ([vp, P(vp)], rc), "bsk_get_terminal_obs_device": ([vp, P(vp), P(vp)], rc),
        "bsk_get_state_device": ([vp, P(vp), P(i64)], rc), "bsk_get_batch_stats": ([vp, P(f64), P(i64)], rc),
        "bsk_n_fields": ([vp], rc), "bsk_get_state": ([vp, vp], rc), "bsk_set_state": ([vp, vp], rc),
        "bsk_get_counters": ([vp, vp, vp], rc), "bsk_set_counters": ([vp, vp, vp], rc), "bsk_set_ic_pool": ([vp, i, vp], rc),
        "bsk_sample_ic_pool": ([vp, i, u64], rc), "bsk_reset_from_pool": ([vp, vp], rc),
        "bsk_reset_from_pool_shared": ([vp, i, vp, vp], rc), "bsk_get_ic_pool": ([vp, vp], rc),
        "bsk_get_terminal_obs": ([vp, vp, vp], rc), "bsk_set_env_base": ([vp, i64], rc), "bsk_set_sim_time": ([vp, f64], rc),
        "bsk_sync": ([vp], rc),
        "bsk_fork_device": ([vp, vp, vp], rc), "bsk_fork": ([vp, vp, vp], rc),
        "bsk_select_branches": ([vp, vp, vp, i, i, i, f64, vp, vp, vp, vp], rc),
        "bsk_beam_select": ([vp, vp, i, i, i, f64, vp, vp, vp, vp, vp, vp], rc),
        "bsk_select_branches_boot": ([vp, vp, vp, i, i, i, f64, vp, vp, vp, vp, vp], rc),
        "bsk_beam_select_boot": ([vp, vp, i, i, i, f64, f64, vp, vp, vp, vp, vp, vp, vp, vp], rc),
        "bsk_policy_n_params": ([spec], rc), "bsk_policy_create": ([spec, vp, i, P(vp)], rc), "bsk_policy_set_params": ([vp, vp], rc),
        "bsk_policy_destroy": ([vp], None), "bsk_policy_set_rng": ([vp, u64, u64], rc), "bsk_policy_get_rng": ([vp, P(u64), P(u64)], rc),
        "bsk_policy_act": ([vp, vp, i64, i, i64, i, vp, vp, vp, vp, i64, vp], rc),
        "bsk_policy_value": ([vp, vp, i64, i, vp, vp], rc),
        "bsk_policy_rollout": ([vp, vp, i, i, i, vp, vp, vp, vp, vp, vp], rc),
        "bsk_population_create": ([spec, i, vp, i, P(vp)], rc), "bsk_population_destroy": ([vp], None),
        "bsk_population_set_rng": ([vp, u64, u64], rc), "bsk_population_get_rng": ([vp, P(u64), P(u64)], rc),
        "bsk_population_set_params": ([vp, vp], rc), "bsk_population_set_params_device": ([vp, vp, i, i, vp], rc),
        "bsk_population_get_member": ([vp, i, vp], rc),
        "bsk_population_act": ([vp, vp, i64, i, i, i64, i, vp, vp, vp, vp, i64, vp], rc),
        "bsk_population_rollout": ([vp, vp, i, i, i, f64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp], rc),
        "bsk_es_create": ([spec, i, vp, f64, f64, i, u64, i, P(vp)], rc), "bsk_es_destroy": ([vp], None),
        "bsk_es_ask": ([vp, vp, vp], rc), "bsk_es_tell": ([vp, vp, vp], rc), "bsk_es_get_state": ([vp, vp, P(u64)], rc),
        "bsk_es_set_state": ([vp, vp, u64], rc), "bsk_es_generation_device": ([vp, P(vp)], rc),
        "bsk_es_set_optimizer": ([vp, i, f64, f64, f64, f64], rc), "bsk_es_get_moments": ([vp, vp, vp, vp], rc),
        "bsk_es_set_moments": ([vp, vp, vp, vp], rc),
        "bsk_es_set_sigma_adaptation": ([vp, i, f64, f64, f64, f64], rc), "bsk_es_get_sigma": ([vp, vp], rc),
        "bsk_es_set_sigma": ([vp, vp], rc),
        "bsk_es_set_log": ([vp, i, vp], rc), "bsk_es_get_log": ([vp, vp, vp], rc), "bsk_es_get_best": ([vp, vp, vp, vp, vp], rc),
        "bsk_es_set_best": ([vp, vp, vp, vp, vp], rc), "bsk_es_best_device": ([vp, P(vp)], rc),
        "bsk_es_set_validation": ([vp, i, i, u64, vp], rc), "bsk_es_get_validation_log": ([vp, vp, vp], rc),
        "bsk_es_get_validated_best": ([vp, vp, vp, vp], rc), "bsk_es_set_validated_best": ([vp, vp, vp, vp], rc),
        "bsk_es_validated_best_device": ([vp, P(vp)], rc), "bsk_es_validation_epochs_device": ([vp, P(vp)], rc),
        "bsk_population_set_obs_stats_members": ([vp, i], rc),
        "bsk_population_set_outcomes": ([vp, vp], rc), "bsk_es_set_outcome_log": ([vp, i, vp], rc),
        "bsk_es_get_outcome_log": ([vp, vp, vp], rc),
        "bsk_obs_stats_create": ([i, i, P(vp)], rc), "bsk_obs_stats_destroy": ([vp], None),
        "bsk_obs_stats_accumulate": ([vp, vp, i64, i, vp, vp], rc), "bsk_obs_stats_get": ([vp, P(u64), vp, vp], rc),
        "bsk_obs_stats_totals_device": ([vp, P(vp), P(vp)], rc), "bsk_obs_stats_get_state": ([vp, vp, vp], rc),
        "bsk_obs_stats_set_state": ([vp, vp, vp], rc), "bsk_obs_stats_reset": ([vp, vp], rc),
        "bsk_population_set_obs_stats": ([vp, vp], rc), "bsk_policy_set_obs_stats": ([vp, vp], rc),
        "bsk_es_apply_obs_norm": ([vp, vp, f64, vp], rc),
        "bsk_fit_create": ([vp, f64, f64, f64, f64, f64, f64, P(vp)], rc), "bsk_fit_destroy": ([vp], None),
        "bsk_fit_accumulate": ([vp, vp, i64, i, vp, vp, vp, vp, i64, vp], rc), "bsk_fit_step": ([vp, vp], rc),
        "bsk_fit_stats_device": ([vp, P(vp)], rc), "bsk_fit_get_state": ([vp, vp, vp, vp, vp, P(u64)], rc),
        "bsk_fit_set_state": ([vp, vp, vp, vp, vp, u64], rc), "bsk_fit_set_lr": ([vp, f64], rc),
        "bsk_fit_alive_mask": ([vp, i, i, vp, vp], rc),
        "bsk_gae": ([vp, vp, vp, vp, i, i, i64, f64, f64, vp, vp, vp], rc),
        "bsk_fit_accumulate_pg": ([vp, vp, i64, i, vp, vp, vp, f64, f64, vp, vp, vp, i64, vp], rc),
        "bsk_fit_pg_stats_device": ([vp, P(vp)], rc),
        "bsk_adv_normalize_work_bytes": ([i], i64), "bsk_adv_normalize": ([vp, vp, i, i, i64, f64, vp, vp, vp], rc),
        "bsk_fit_set_max_grad_norm": ([vp, f64], rc), "bsk_fit_grad_norm_device": ([vp, P(vp)], rc),
        "bsk_fit_apply_obs_norm": ([vp, vp, f64, vp], rc),
        "bsk_pg_gather": ([vp, i, i, i64, i64, i, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp], rc),
        "bsk_pg_shuffle_advance": ([vp, vp], rc),
        "bsk_fit_accumulate_ppo": ([vp, vp, i64, i, vp, vp, vp, f64, f64, vp, vp, f64, vp, vp, i64, vp, vp], rc),
        "bsk_fit_vclip_stats_device": ([vp, P(vp)], rc),
        "bsk_pg_episodes_work_bytes": ([i], C.c_size_t),
        "bsk_pg_episodes": ([vp, vp, vp, vp, vp, i, i, i64, vp, vp, vp, vp, i, vp, vp], rc),
        "bsk_pg_log_update": ([vp, i, vp, i, vp, i, vp, vp], rc), "bsk_pg_log_advance": ([vp, i, vp, vp], rc),
        "bsk_reward_norm_work_bytes": ([i], i64),
        "bsk_reward_norm": ([vp, vp, i, i, i64, f64, f64, f64, i, vp, vp, vp, vp, vp], rc),
        "bsk_fit_set_schedule": ([vp, P(BskFitSchedule)], rc), "bsk_fit_schedule_begin": ([vp, vp], rc),
        "bsk_fit_kl_gate": ([vp, vp, i, vp], rc), "bsk_fit_schedule_end": ([vp, vp, i, vp], rc),
        "bsk_fit_schedule_device": ([vp, P(vp)], rc), "bsk_fit_get_schedule_state": ([vp, vp], rc),
        "bsk_fit_set_schedule_state": ([vp, u64], rc),
        "bsk_profile_begin": ([vp, i], rc), "bsk_profile_set_stride": ([vp, i], rc), "bsk_profile_end": ([vp, P(f64), P(i)], rc),
        "bsk_profile_end_samples": ([vp, P(f64), P(i), vp, i], rc), "bsk_calibrate_fp64": ([i, i, i, P(f64), P(f64)], rc),
        "bsk_kernel_info": ([vp, C.c_char_p, i, P(i), P(i), P(i), P(i)], rc),
    }


SIGNATURES = _signatures()

_LIB = None


def lib_path():
    """In-tree library; ``BSKGPU_LIB`` overrides it (kernel A/B experiments only)."""
    return os.environ.get("BSKGPU_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libbskgpu.so")


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own ``libamdhip64.so``
    (SONAME libamdhip64.so.7, the SONAME libbskgpu.so asks for).  If libbskgpu.so were loaded
    first it would bind /opt/rocm's copy and a later ``import torch`` would bring a second runtime
    into the process: torch then sees no GPU and device pointers cannot be shared with RCCL.
    Preloading torch's copy (without importing torch) makes every import order end with one
    runtime; without torch installed the system ROCm runtime is used."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return None
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
            return cand
    except Exception:
        return None
    return None


def load():
    """Load libbskgpu.so (built in-tree by ``__graft_entry__.build()`` / csrc/Makefile)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise BskGpuUnavailable(
            "%s is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` (or `make -C "
            "basilisk_env_amd/csrc`). There is no CPU fallback for the propagator." % path)
    _share_hip_runtime_with_torch()
    try:
        lib = C.CDLL(path)
    except OSError as e:  # pragma: no cover - depends on the host
        raise BskGpuUnavailable("cannot load %s: %s" % (path, e)) from e
    for name, (argtypes, restype) in SIGNATURES.items():
        # (a BSKGPU_LIB variant built from an older tree - kernel A/B against a previous round - may predate an export)
        if hasattr(lib, name) or not os.environ.get("BSKGPU_LIB"):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argtypes, restype
    _LIB = lib
    return lib


def calibrate_fp64(device=0, waves_per_simd=2, repeats=5):
    """-> (TFLOP/s, ns per FMA wave-instruction and SIMD) this device sustains on independent fp64 FMA chains."""
    tf, ns = C.c_double(), C.c_double()
    check(load().bsk_calibrate_fp64(int(device), int(waves_per_simd), int(repeats), C.byref(tf), C.byref(ns)))
    return tf.value, ns.value


def check(rc):
    if rc != 0:
        msg = load().bsk_last_error()
        msg = msg.decode("utf-8", "replace") if msg else ""
        if rc == -2:
            raise BskGpuUnavailable("libbskgpu: %s" % msg)
        raise BskError(rc, msg)
