"""The space of ``bsk_config`` constants, for tests (tests/test_config_space_host.py, tests/test_gpu_config_space.py, and for the
halves form of the one-sub-step launch tests/test_halves_config_host.py, tests/test_gpu_halves_config.py).

``bsk_default_config`` is symmetric exactly where an indexing mistake would show (all ``js`` equal, all ``facet_cd`` 2.2, the
+/- facet pairs of equal area, two zero components in ``sigma_R0N`` and in ``panel_normal``, identity ``ctrl_axes``,
``failure_penalty = 1``), and ``build_params`` (csrc/bsk_config.hip) hands the kernels several derived copies of most constants.
This module says, for EVERY field of ``_lib.BskConfig._fields_``:

* its kind - ``abi`` (bookkeeping of the C-ABI), ``structure`` (schedules, switches and geometry that select a kernel form or a
  task order: varied by the parity, fuzz, general-inertia, forces and harmonics tests already) or ``physical``;
* for a physical constant, how to draw a legal and ASYMMETRIC value from a seeded generator (``draw``);
* the scenarios in which the field moves the outputs (``live``: level + modifiers, see ``Scenario``), each with the kernel forms
  that read a copy of the field there (``FORMS``), and the one-field change tried there (``one``; the draw unless given);
* where a draw lands among the kernel families (``family``), which the GPU tests assert through ``kernel_info()["name"]``.

``draw_config`` draws every physical constant at once; ``one_field_cases`` lists (field, scenario, forms, edit).  Ranges: every
scalar is scaled by an independent factor in [0.6, 1.6] unless the entry says otherwise; where a narrower range is used the
entry's ``note`` gives the reason.  Nothing here runs a kernel: the GPU module imports the cases, the host module checks them
against the 50-digit model and measures that each one-field change is visible to the oracle (the power of the GPU tests).
"""
import ctypes

import numpy as np

from basilisk_env_amd import _lib
from basilisk_env_amd._lib import (FLAG_DESAT, FLAG_DRAG, FLAG_LDS_SCRATCH, FLAG_POWER, FLAG_SUN_THIRD_BODY, GRAV_PM, GRAV_PM_J2,
                                   GRAV_SH)
from basilisk_env_amd.simulators.dynamics.config import AU, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
from helpers import general_hub, max_group_err, visible_sh_coefficients

LEVELS = ("bare", "ldss", "power", "full", "fullg")
GRAV_NAME = {GRAV_PM: "PM", GRAV_PM_J2: "PM_J2"}
SH_FORM_NAME = {"1": "SH/scalar", "4": "SH/dpp", "5": "SH/dpp2"}
SH_DEGREE = 8


# ---------------------------------------------------------------------------------------------------------------- levels
def apply_level(cfg, level):
    """The feature flags of a kernel level (tests/test_gpu_kernel_info.py: ``config``), with an atmosphere in which drag is live."""
    assert level in LEVELS, level
    if level == "ldss":
        cfg.flags |= FLAG_LDS_SCRATCH
    if level in ("power", "full", "fullg"):
        cfg.flags |= FLAG_POWER
    if level in ("full", "fullg"):
        cfg.flags |= FLAG_SUN_THIRD_BODY | FLAG_DRAG | (FLAG_DESAT if cfg.n_rw else 0)
        cfg.base_density, cfg.scale_height = 1e-9, 100e3
    if level == "fullg":
        generic_facets(cfg, np.random.default_rng(5))
    return cfg


def generic_facets(cfg, rng):
    """Tilted facet normals (re-normalised) and centres moved off their axes: ``build_params`` leaves the table path
    (``facet_axis == 2``) and the ``scenario/generic-facets`` kernel runs."""
    for i in range(cfg.n_facets):
        v = np.array([cfg.facet_normal[i][k] for k in range(3)]) + 0.3 * rng.normal(size=3)
        v /= np.linalg.norm(v)
        for k in range(3):
            cfg.facet_normal[i][k] = float(v[k])
            cfg.facet_pos[i][k] += float(0.05 * rng.normal())
    return cfg


def kernel_name(cfg, hub, level, form="single", sh_form=None, rollout=None):
    """What ``bsk_kernel_info`` must report for a config of this family (the literals tests/test_gpu_kernel_info.py pins)."""
    g = SH_FORM_NAME[sh_form] if cfg.gravity_model == GRAV_SH else GRAV_NAME[cfg.gravity_model]
    if rollout:
        return "rollout_kernel<%s,%d,%s,%s>" % (g, cfg.n_rw, hub, rollout)
    lvl = {"bare": "", "ldss": ",lds-scratch", "power": ",power", "full": ",scenario", "fullg": ",scenario/generic-facets"}[level]
    return "step_kernel<%s,%d,%s%s%s>" % (g, cfg.n_rw, hub, lvl, {"single": "", "pair": ",pair", "tri": ",tri", "halves": ",halves"}[form])


# ---------------------------------------------------------------------------------------------------------------- draws
def _f(rng, lo=0.6, hi=1.6):
    return float(rng.uniform(lo, hi))


def _scaled(name, lo=0.6, hi=1.6):
    def draw(cfg, rng, ctx):
        setattr(cfg, name, getattr(cfg, name) * _f(rng, lo, hi))
    return draw


def _vec_nonzero(rng, norm, floor):
    """A random vector of the given norm whose three components all exceed ``floor * norm`` in magnitude."""
    while True:
        v = rng.normal(size=3)
        v *= norm / np.linalg.norm(v)
        if np.abs(v).min() > floor * norm:
            return v


def _draw_inertia(cfg, rng, ctx):
    for k in (0, 4, 8):
        cfg.inertia[k] *= _f(rng)


def _draw_js(cfg, rng, ctx):
    # the pyramid's diagonal-hub kernels can only see EQUAL js: I - sum js g g^T has off-diagonals proportional to
    # js0-js1+js2-js3, js0-js1-js2+js3 and js0+js1-js2-js3 otherwise; on the triad it stays exactly diagonal for any js
    if ctx["n_rw"] == 4 and ctx["hub"] == "diag":
        f = _f(rng)
        while abs(f - 1.0) < 0.05:
            f = _f(rng)
        for i in range(4):
            cfg.js[i] *= f
    else:
        for i in range(ctx["n_rw"]):
            cfg.js[i] *= _f(rng)


def _draw_u_min(cfg, rng, ctx):
    cfg.u_min = float(rng.uniform(2e-3, 2e-2))        # a dead-band that small commanded torques do fall into (default 1e-5)


def _draw_sigma_r0n(cfg, rng, ctx):
    v = _vec_nonzero(rng, float(rng.uniform(0.2, 0.4)), 0.15)
    for k in range(3):
        cfg.sigma_R0N[k] = float(v[k])


def _draw_ctrl_axes(cfg, rng, ctx):
    while True:
        m = rng.normal(size=(3, 3))
        if np.linalg.cond(m) < 10.0:
            break
    for k in range(9):
        cfg.ctrl_axes[k] = float(m.flat[k])


def _draw_failure_penalty(cfg, rng, ctx):
    cfg.failure_penalty = float(rng.choice([rng.uniform(0.3, 0.8), rng.uniform(1.25, 2.0)]))


def _draw_r_min(cfg, rng, ctx):
    cfg.r_min = float(rng.uniform(6.65e6, 7.10e6))    # inside the sampled orbits' range of |r| (6 527 - 7 215 km)


def _draw_panel_normal(cfg, rng, ctx):
    v = _vec_nonzero(rng, 1.0, 0.15)
    for k in range(3):
        cfg.panel_normal[k] = float(v[k])


def _draw_sun_r0(cfg, rng, ctx):
    v = _vec_nonzero(rng, AU * float(rng.uniform(0.8, 1.2)), 0.1)
    for k in range(3):
        cfg.sun_r0[k] = float(v[k])


def _draw_sun_v(cfg, rng, ctx):
    for k in range(3):
        cfg.sun_v[k] *= _f(rng)


def _thr_spans(cfg):
    d = np.array([np.cross([cfg.thr_pos[i][k] for k in range(3)], [cfg.thr_dir[i][k] for k in range(3)]) for i in range(cfg.n_thr)])
    return np.linalg.cond(d.T @ d) < 1e3


def _draw_n_thr(cfg, rng, ctx):
    cfg.n_thr = int(rng.choice([5, 6, 7]))
    assert _thr_spans(cfg)


def _draw_thr_max_counter(cfg, rng, ctx):
    cfg.thr_max_counter = int(rng.choice([1, 2, 3, 5]))


def _draw_thr_pos(cfg, rng, ctx):
    for i in range(_lib.BSK_MAX_THR):
        for k in range(3):
            cfg.thr_pos[i][k] *= float(rng.uniform(0.85, 1.15))
    assert _thr_spans(cfg)


def _draw_thr_dir(cfg, rng, ctx):
    for i in range(_lib.BSK_MAX_THR):
        v = np.array([cfg.thr_dir[i][k] for k in range(3)]) + 0.15 * rng.normal(size=3)
        v /= np.linalg.norm(v)
        for k in range(3):
            cfg.thr_dir[i][k] = float(v[k])
    assert _thr_spans(cfg)


def _draw_thr_min_fire(cfg, rng, ctx):
    cfg.thr_min_fire_time = float(rng.uniform(0.05, 0.3))      # of a control period of 0.5 - 1 s (default 0.002 s: never reached)


def _draw_thr_min_on(cfg, rng, ctx):
    cfg.thr_min_on_time = float(rng.uniform(0.3, 0.6))


def _draw_facet_area(cfg, rng, ctx):
    for i in range(8):                  # independent factors: the +/- pairs get unequal areas, the half-difference table fills
        cfg.facet_area[i] *= _f(rng)


def _draw_facet_cd(cfg, rng, ctx):
    for i in range(8):
        cfg.facet_cd[i] *= _f(rng)


def _draw_facet_pos(cfg, rng, ctx):
    # the on-axis component only: the centres stay on their own normal axes (the table path); level "fullg" moves them off
    for i in range(cfg.n_facets):
        for k in range(3):
            cfg.facet_pos[i][k] *= _f(rng)


# one-field changes that differ from the draw (the draw's range would leave the field too weak in a short run)
def _one_r_min(cfg, rng, ctx):
    cfg.r_min = 6.8713e6                # about the median |r| of the sampled orbits: DONE_ORBIT for roughly half of a batch


def _one_mu_sun(cfg, rng, ctx):
    cfg.mu_sun *= 2.5


def _one_thr_max_counter(cfg, rng, ctx):
    cfg.thr_max_counter = 3             # (the desat scenario's own value is 1)


def _one_storage(cfg, rng, ctx):
    cfg.storage_capacity *= 0.5         # 10 W h: the batteries that start above it are clamped at once


# ---------------------------------------------------------------------------------------------------------------- forms
# the kernel forms that read a copy of a field at each level (csrc/bsk_config.hip: build_params; csrc/bsk_device.hpp)
FORMS = {
    "bare": ("single", "fullhub", "ldss", "rollout"),
    "power": ("single", "fullhub", "pair"),
    "full": ("single", "fullhub", "pair", "tri", "generic"),
    "sh": ("sh1", "sh4", "sh5"),
}


class Scenario(object):
    """A level (``bare`` / ``power`` / ``full`` / ``sh``: harmonics, bare) plus the modifiers under which some fields come alive:

    ``deadband``  gains a hundred times smaller: the commanded wheel torques fall below ``u_min`` and ``u_max`` for part of the batch
    ``failures``  a third of the spacecraft start with wheels beyond the limit, a third with an empty battery (the two overlap)
    ``epoch``     a Sun epoch offset of 40 days (``sim_time0`` / ``bsk_set_sim_time``): ``sun_v`` moves the Sun by a quarter of a radian
    ``dense``     an atmosphere a hundred times denser (1e-7 kg/m^3 at the surface, 100 km scale height): drag moves the orbit
    ``late``      every spacecraft's tick counter starts at 100 000 (2.8 h): the planet has turned by 0.73 rad under the field
    ``long``      0.5 s integrator steps, an FSW tick on every second one, and calls of 150 - 260 sub-steps (300 s in all): the Sun's tidal term moves v by 1e-8
    ``desat``     action 2 for every spacecraft, wheels 2.5 times faster, 0.5 s control period, bursts on every second FSW tick
    """

    def __init__(self, level, mods=(), n_rw=4, grav=GRAV_PM_J2):
        self.level, self.mods, self.n_rw, self.grav = level, tuple(mods), n_rw, (GRAV_SH if level == "sh" else grav)

    @property
    def name(self):
        return "+".join((self.level,) + self.mods) + "/rw%d" % self.n_rw

    @property
    def sim_time0(self):
        return 40 * 86400.0 if "epoch" in self.mods else 0.0

    @property
    def ticks0(self):
        return 100000 if "late" in self.mods else 0

    def config(self):
        cfg = default_config(self.n_rw, self.grav)
        if "long" in self.mods:
            cfg.dt, cfg.fsw_every = 0.5, 2            # (the control period stays 1 s: the attitude loop as stable as at the default rates)
        if self.level == "sh":
            cfg.sh_degree = SH_DEGREE
        else:
            apply_level(cfg, self.level)
        if "deadband" in self.mods:
            cfg.K, cfg.P = 0.07, 0.35
        if "dense" in self.mods:
            cfg.base_density = 1e-7
        if "desat" in self.mods:
            cfg.fsw_every, cfg.thr_max_counter = 5, 1
        return cfg

    def sh(self):
        return visible_sh_coefficients(SH_DEGREE, seed=3) if self.level == "sh" else (None, None)

    def ic(self, n, seed):
        ic = sample_ic_batch(n, self.n_rw, seed=seed)
        t = 12 + self.n_rw
        if "failures" in self.mods:
            if self.n_rw:
                ic[12:12 + self.n_rw, 0::3] *= 5.0
            ic[t + _lib.T_CHARGE, 1::4] = 0.0
        if "desat" in self.mods and self.n_rw:
            ic[12:12 + self.n_rw] *= 2.5
        return ic

    def schedule(self, n, seed):
        """[(actions int32[n], sub-steps)]: several calls of different lengths (not multiples of the FSW period)."""
        rng = np.random.default_rng(7000 + seed)
        ks = (23, 48, 31) if self.level != "sh" else (11, 17, 9)
        if "desat" in self.mods:
            ks = (37, 60, 45, 52)
        if "long" in self.mods:
            ks = (150, 260, 190)
        hi = 3 if (self.level == "full" and self.n_rw) else 2
        out = []
        for k in ks:
            act = rng.integers(0, hi, n).astype(np.int32)
            if "desat" in self.mods:
                act[:] = 2
            out.append((act, k))
        return out


def run_oracle(cfg, ic, schedule, sim_time0=0.0, sh=(None, None), ticks0=0, omp=False):
    """The oracle over a schedule -> per call (state, obs, reward, reason, steps, ticks), copies."""
    from oracle import oracle
    n = ic.shape[1]
    st = np.ascontiguousarray(ic.copy())
    steps, ticks = np.zeros(n, np.int32), np.full(n, ticks0, np.int32)
    out = []
    for act, k in schedule:
        obs, rew, _, why = oracle.step(cfg, st, steps, ticks, act, k, sim_time0=sim_time0, cbar=sh[0], sbar=sh[1], omp=omp)
        out.append((st.copy(), obs, rew, why, steps.copy(), ticks.copy()))
    return out


# ---------------------------------------------------------------------------------------------------------------- halves form
ODD_ACTIONS = (3, 7, 15, 16, 255, -1)      # raw integers outside {0, 1, 2}: to the oracle's guidance, as to the kernels, "not 0"


def halves_schedule(n, seed, launches=48, odd_actions=False):
    """[(actions int32[n], 1)] * launches: what the halves form of the step kernel runs (one sub-step per launch), past several FSW
    ticks of every period ``draw_halves_structure`` draws.  ``odd_actions``: a quarter of the actions come from ``ODD_ACTIONS``."""
    rng = np.random.default_rng(8000 + seed)
    out = []
    for _ in range(launches):
        act = rng.integers(0, 3, n).astype(np.int32)
        if odd_actions:
            odd = rng.random(n) < 0.25
            act[odd] = rng.choice(np.array(ODD_ACTIONS, dtype=np.int32), size=int(odd.sum()))
        out.append((act, 1))
    return out


def draw_halves_structure(cfg, rng):
    """The structure fields the halves form duplicates code for (its own phase rule, tick test and integrator constants): an FSW
    period on which every launch / every other launch / an odd share of the launches carries the hand-over, another integrator
    step, either task order, and an episode shorter than ``halves_schedule``.  ``nav_lag`` stays 1: the form needs it."""
    cfg.fsw_every = int(rng.choice([1, 2, 3, 7, 13]))
    cfg.dt = float(rng.choice([0.05, 0.1, 0.25]))
    cfg.fsw_lag = int(rng.integers(0, 2))
    cfg.nav_lag = 1
    cfg.max_length = int(rng.integers(20, 40))
    return cfg


def change(a, b, n_rw):
    """How far two runs of ``run_oracle`` are apart, in the units of the GPU tests' tolerances: the largest relative change of a
    state field group (helpers.max_group_err, GPU tolerance 1e-11), of the battery charge [W s] relative to 1e4 (GPU: 1e-7 W s),
    the largest absolute change of an observation (GPU: 1e-11), of a reward (GPU: 1e-12) and the largest share of spacecraft
    whose done reason changed, over the calls."""
    t = 12 + n_rw + _lib.T_CHARGE
    c = {"state": 0.0, "obs": 0.0, "reward": 0.0, "reason": 0.0}
    for (sa, oa, ra, wa, _, _), (sb, ob, rb, wb, _, _) in zip(a, b):
        c["state"] = max(c["state"], max(max_group_err(sa, sb, n_rw).values()), float(np.abs(sa[t] - sb[t]).max()) / 1e4)
        c["obs"] = max(c["obs"], float(np.abs(oa - ob).max()))
        c["reward"] = max(c["reward"], float(np.abs(ra - rb).max()))
        c["reason"] = max(c["reason"], float((wa != wb).mean()))
    return c


# 1 000 x the GPU tests' tolerance on the quantity: a kernel that ignores the field cannot hide inside 1e-11 (a condition, not a measurement)
LIVE = {"state": 1e-8, "obs": 1e-8, "reward": 1e-9, "reason": 0.1}


def is_live(c):
    return any(c[k] >= LIVE[k] for k in LIVE)


# ---------------------------------------------------------------------------------------------------------------- registry
def _abi(note):
    return {"kind": "abi", "note": note}


def _structure(note):
    return {"kind": "structure", "note": note}


def _phys(draw, live, note="", one=None, family="any", invariant=False):
    return {"kind": "physical", "draw": draw, "live": live, "note": note, "one": one or draw, "family": family, "invariant": invariant}


S = Scenario
_EVERY = (S("bare"), S("power"), S("full"))                 # constants of the dynamics / FSW / observation: read at every level
_POWER = (S("power"), S("full"))
_FULL = (S("full"),)
_DESAT = (S("full", ("desat",)),)

FIELDS = {
    "abi_version": _abi("checked by validate()"),
    "struct_size": _abi("checked by validate()"),
    "pad0_": _abi("padding"),
    "dt": _structure("integrator step: varied by the parity, fuzz and rollout tests, and in the halves form by "
                     "tests/test_gpu_halves_config.py (draw_halves_structure); every Scenario here keeps 0.1 s"),
    "fsw_every": _structure("FSW period: fuzz tests; in the halves form tests/test_gpu_halves_config.py (1, 2, 3, 7, 10, 13)"),
    "gravity_model": _structure("selects the kernel: every test"),
    "sh_degree": _structure("harmonics tests"),
    "n_rw": _structure("selects the kernel: every test"),
    "flags": _structure("feature level and output forms: every test"),
    "max_length": _structure("episode length: rollout and auto-reset tests"),
    "fsw_lag": _structure("task order: fuzz tests; in the halves form tests/test_gpu_halves_config.py"),
    "nav_lag": _structure("task priorities: fuzz tests"),
    "gs": _structure("wheel spin axes: a tilted axis is the general-hub family (helpers.general_hub; hub='full' here)"),
    "n_facets": _structure("facet count: tests/test_gpu_forces.py"),
    "facet_normal": _structure("facet geometry: tilted normals are the generic-facet family (level 'fullg' here; test_gpu_forces.py)"),
    "facet_pos": _structure("facet geometry: off-axis centres are the generic-facet family; draw_config scales the on-axis "
                            "component (the KB_FAD table) and level 'fullg' moves the centres off their axes"),
    "mu": _phys(_scaled("mu", 0.9, 1.1), _EVERY, "0.9 - 1.1: the sampled states stay bound orbits above the surface for the length of a test"),
    "req": _phys(_scaled("req", 0.93, 1.02), (S("bare"), S("power"), S("full")),
                 "0.93 - 1.02: the lowest sampled perigee is 6 527 km and 1.02 req = 6 506 km (inside the planet the density "
                 "overflows); read by J2 (j2k), the eclipse cone and the atmosphere's altitude"),
    "j2": _phys(_scaled("j2"), _EVERY),
    "planet_rate": _phys(_scaled("planet_rate"), (S("sh", ("late",)),), "0 outside harmonics: only the rotating field reads it, and a run of seconds "
                         "needs a late start for the rotation angle to matter"),
    "inertia": _phys(_draw_inertia, _EVERY, "the diagonal; products of inertia are the hub KIND (structure: helpers.general_hub, hub='full')"),
    "mass": _phys(_scaled("mass"), (S("full", ("dense",)),), "drag and thruster accelerations only: needs the dense atmosphere to move the orbit by 1e-8"),
    "js": _phys(_draw_js, (S("bare", n_rw=3), S("power", n_rw=3), S("full", n_rw=3), S("full", ("desat",), n_rw=3), S("bare"), S("full")),
                family="triad: per-wheel js stays 'diag'; pyramid: equal non-default js is 'diag', per-wheel js is 'full'"),
    "u_max": _phys(_scaled("u_max"), _EVERY),
    "u_min": _phys(_draw_u_min, (S("bare", ("deadband",)), S("power", ("deadband",)), S("full", ("deadband",))),
                   "drawn in 2e-3 - 2e-2 N m (default 1e-5): dead unless commanded torques fall into the band"),
    "f_coulomb": _phys(_scaled("f_coulomb"), _EVERY),
    "K": _phys(_scaled("K"), _EVERY),
    "P": _phys(_scaled("P"), _EVERY),
    "sigma_R0N": _phys(_draw_sigma_r0n, _EVERY, "all three components non-zero, norm 0.2 - 0.4"),
    "ctrl_axes": _phys(_draw_ctrl_axes, _EVERY, "a general invertible matrix (condition number < 10).  DEAD BY ALGEBRA: the wheel map "
                       "CGs^T (CGs CGs^T)^-1 C with CGs = C Gs does not depend on an invertible C; asserted invariant", invariant=True),
    "wheel_limit": _phys(_scaled("wheel_limit"), _EVERY),
    "power_max": _phys(_scaled("power_max"), _EVERY),
    "reward_mult": _phys(_scaled("reward_mult"), _EVERY),
    "failure_penalty": _phys(_draw_failure_penalty, (S("bare", ("failures",)), S("power", ("failures",)), S("full", ("failures",))),
                             "never 1; dead unless episodes fail"),
    "r_min": _phys(_draw_r_min, _EVERY, "drawn inside the batch's range of |r| (default 6.4 m: BSK_DONE_ORBIT never raised)", one=_one_r_min),
    "panel_normal": _phys(_draw_panel_normal, _POWER, "a unit vector, all three components non-zero"),
    "panel_area": _phys(_scaled("panel_area"), _POWER),
    "panel_efficiency": _phys(_scaled("panel_efficiency"), _POWER),
    "power_draw": _phys(_scaled("power_draw"), _POWER),
    "storage_capacity": _phys(_scaled("storage_capacity"), _POWER, "dead unless a battery reaches full charge", one=_one_storage),
    "solar_flux": _phys(_scaled("solar_flux"), _POWER),
    "sun_r0": _phys(_draw_sun_r0, _POWER, "any direction, 0.8 - 1.2 au, all three components non-zero"),
    "sun_v": _phys(_draw_sun_v, (S("power", ("epoch",)), S("full", ("epoch",))), "per-component factors; needs the epoch offset: 1.9e-9 within a 20 s run"),
    "mu_sun": _phys(_scaled("mu_sun"), (S("full", ("long",)),), "the tidal term moves v by 1.5e-9 per 30 % in 20 s: long calls, and the one-field change is x 2.5", one=_one_mu_sun),
    "n_thr": _phys(_draw_n_thr, _DESAT, "5, 6 or 7 (default 8); the leading thrusters of the octet still span the three torque axes"),
    "thr_max_counter": _phys(_draw_thr_max_counter, _DESAT, "1, 2, 3 or 5 (default 4)", one=_one_thr_max_counter),
    "thr_pos": _phys(_draw_thr_pos, _DESAT, "every component scaled by 0.85 - 1.15"),
    "thr_dir": _phys(_draw_thr_dir, _DESAT, "tilted by about 10 degrees, re-normalised: the z components become non-zero"),
    "thr_max_thrust": _phys(_scaled("thr_max_thrust"), _DESAT),
    "thr_min_fire_time": _phys(_draw_thr_min_fire, _DESAT, "0.05 - 0.3 s (default 0.002 s): dead unless a pulse is shorter"),
    "thr_min_on_time": _phys(_draw_thr_min_on, _DESAT, "0.3 - 0.6 s (default 0.02 s): dead unless a pulse is shorter"),
    "hs_min": _phys(_scaled("hs_min"), _DESAT),
    "base_density": _phys(_scaled("base_density"), _FULL, "around 1e-9 kg/m^3 (apply_level): at the default 1.22 / 8 km nothing is left at 500 km"),
    "scale_height": _phys(_scaled("scale_height"), _FULL, "around 100 km (apply_level)"),
    "facet_area": _phys(_draw_facet_area, _FULL, "per facet: unequal +/- pairs fill the half-difference table",
                        family="axis-aligned normals, centres on their axes: table path; level 'fullg': scenario/generic-facets"),
    "facet_cd": _phys(_draw_facet_cd, _FULL, "per facet", family="as facet_area"),
}

# drawn by draw_config although classified as structure (the part of the geometry that stays on the table path)
_EXTRA_DRAWS = {"facet_pos": _draw_facet_pos}


def physical_fields():
    return [name for name, _ in _lib.BskConfig._fields_ if FIELDS[name]["kind"] == "physical"]


def draw_config(rng, n_rw, grav, level, hub="diag"):
    """Every physical constant drawn at once -> cfg of the kernel family (grav, n_rw, hub, level)."""
    assert hub in ("diag", "full") and level in LEVELS
    cfg = default_config(n_rw, grav)
    if grav == GRAV_SH:
        cfg.sh_degree = SH_DEGREE
    apply_level(cfg, level if level != "fullg" else "full")
    ctx = {"n_rw": n_rw, "hub": hub, "level": level}
    for name in physical_fields():
        FIELDS[name]["draw"](cfg, rng, ctx)
    _draw_facet_pos(cfg, rng, ctx)
    if level == "fullg":
        generic_facets(cfg, rng)
    if hub == "full":
        general_hub(cfg, rng, inertia=True, tilt=bool(n_rw and rng.random() < 0.5))
    return cfg


def one_field_cases():
    """[(field, Scenario, forms, edit)]: ``edit(cfg)`` changes that one field of the scenario's config, in place.  For ``js`` on
    the pyramid the draw keeps the wheels equal on the diagonal hub ('single', 'pair', ...) and the per-wheel draw is the
    'fullhub' form's; every other field's edit does not depend on the form."""
    out = []
    for name in physical_fields():
        e = FIELDS[name]
        for sc in e["live"]:
            forms = FORMS[sc.level]

            def edit(cfg, form="single", _e=e, _name=name, _sc=sc):
                rng = np.random.default_rng([ord(ch) for ch in _name])
                hub = "full" if form == "fullhub" else "diag"
                _e["one"](cfg, rng, {"n_rw": _sc.n_rw, "hub": hub, "level": _sc.level})
                return cfg
            out.append((name, sc, forms, edit))
    return out


def copy_into(dst, src):
    """``dst`` becomes a byte copy of ``src`` (a cfg_edit for tests/golden/make_golden.py: run_case)."""
    ctypes.memmove(ctypes.byref(dst), ctypes.byref(src), ctypes.sizeof(_lib.BskConfig))
    return dst
