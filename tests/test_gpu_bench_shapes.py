"""GPU: every configuration bench.py times, at the size it is timed at, against the CPU oracle - every spacecraft.

The other full-size tests check invariants or a few dozen sampled envs; a bug that touches one workgroup in the middle of the
grid, one partial a wave-sum join drops, an offset past 2^31 bytes or the form switch at 64 x CU count gets past them.  Here:

- the timed path itself: a ``bench.py --dump-outputs`` child per timed configuration (headline, config 3, the scenario
  levels at K = 1 and K = 1 800, degree-70 harmonics, 4 Mi), its dump against the oracle stepped warm-up + timed times;
- 2^20 + 77 and 2^22 envs through ``step_device`` with per-env actions, int32 and int64 device tensors, step statistics on;
- ``step_n`` at the rollout leg's shapes (65 536 x 541, 4 Mi x 100), history rows included;
- the RL-loop leg (``LeoPowerAttVecEnv.step_tensors``, device sampler, device auto-reset) against the env on the oracle;
- the default form policy at its boundaries (n = 64 x CU count and one more, K = 15 and 16) and the 8 192-env shard.

Bounds: those of the existing test of the same configuration, else 1e-11 relative per field group up to ~100 ticks and
1e-10 at 1 800, rewards 1e-14 at the bare level and 1e-12 above it, battery charge 1e-7, reasons / dones / counters exact.
The oracle runs on every host core the process may use (``omp=True``); the bench children run one after another."""
import os
import subprocess
import sys

import numpy as np
import pytest

from _oracle_backend import OmpOraclePropagator as _OmpOracle
from basilisk_env_amd._lib import (FLAG_DESAT, FLAG_DRAG, FLAG_POWER, FLAG_SUN_THIRD_BODY, GRAV_PM_J2, GRAV_SH)
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.dynamics.gravity_sh import synthetic_sh_coefficients
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
from helpers import max_group_err
from oracle import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RW = 4
CHARGE = 12 + N_RW + 7                 # battery charge row of the state slab
FULL = FLAG_POWER | FLAG_SUN_THIRD_BODY | FLAG_DRAG | FLAG_DESAT
LEVELS = {"bare": 0, "power": FLAG_POWER, "full": FULL}


def _cfg(level="bare", sh=False):
    cfg = default_config(N_RW, GRAV_SH if sh else GRAV_PM_J2)
    cfg.flags |= LEVELS[level]
    if sh:
        cfg.sh_degree = 70
    return cfg


class _Oracle(object):
    """The oracle stepping ``ic`` (a copy) from zero counters; ``cbar`` / ``sbar`` for harmonics."""

    def __init__(self, cfg, ic, sh=None):
        self.cfg, self.st = cfg, np.array(ic, dtype=np.float64, order="C")
        n = self.st.shape[1]
        self.steps, self.ticks = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.kw = {"cbar": sh[0], "sbar": sh[1]} if sh else {}

    def step(self, actions, k):
        return oracle.step(self.cfg, self.st, self.steps, self.ticks, np.ascontiguousarray(actions, np.int32), k, omp=True, **self.kw)


def _check_state(got, ref, tol, tag, power=False):
    errs = max_group_err(got, ref, N_RW)
    assert max(errs.values()) < tol, (tag, errs)
    if power:
        c = np.abs(got[CHARGE] - ref[CHARGE]).max() / np.abs(ref[CHARGE]).max()
        assert c < 1e-7, (tag, "charge", c)


def _check_outputs(got, ref, obs_tol, rew_tol, tag):
    """(obs, reward, done, reason) against the oracle's: obs / reward within the bounds, done and reason exact."""
    obs, rew, done, why = got
    o_obs, o_rew, o_done, o_why = ref
    assert np.array_equal(np.asarray(why).astype(np.int64), o_why.astype(np.int64)), (tag, "reason", int((why != o_why).sum()))
    assert np.array_equal(np.asarray(done).astype(bool), o_done.astype(bool)), (tag, "done")
    assert np.abs(obs - o_obs).max() < obs_tol, (tag, "obs", np.abs(obs - o_obs).max(axis=1))
    assert np.abs(rew - o_rew).max() < rew_tol, (tag, "reward", np.abs(rew - o_rew).max())


def _done_words(done):
    """the device's done-mask words (bit i % 64 of word i / 64) of a bool per env"""
    n = done.size
    pad = np.zeros((n + 63) // 64 * 64, np.uint8)
    pad[:n] = done
    return np.packbits(pad.reshape(-1, 64), axis=1, bitorder="little").view("<u8").ravel()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the timed path, through bench.py itself
BENCH_CASES = {
    # name: (envs, extra arguments, warm-up, timed steps, state bound, obs bound, reward bound)
    # headline: 31 K = 1 launches, the last one past three FSW ticks (bounds of tests/test_gpu_bench.py)
    "headline": (65536, [], 28, 3, 1e-12, 1e-12, 1e-14),
    "config3": (131072, [], 2, 3, 1e-12, 1e-12, 1e-14),
    "power": (65536, ["--scenario", "power"], 2, 3, 1e-11, 1e-11, 1e-12),
    "full": (65536, ["--scenario", "full"], 2, 3, 1e-11, 1e-11, 1e-12),
    "full_k1800": (65536, ["--scenario", "full", "--substeps", "1800"], 0, 1, 1e-10, 1e-9, 1e-12),     # one 1 800-tick step
    "sh70": (65536, ["--gravity", "sh"], 2, 3, 1e-11, 1e-11, 1e-12),
    "large_n": (1 << 22, [], 2, 3, 1e-12, 1e-12, 1e-14),
}


@pytest.mark.parametrize("case", list(BENCH_CASES))
def test_bench_dump_matches_oracle_on_every_env(case, tmp_path):
    n, args, warm, steps, s_tol, o_tol, r_tol = BENCH_CASES[case]
    out = tmp_path / "dump"
    env = dict(os.environ, BENCH_EXTRA_FILE=str(tmp_path / "bench_extra.json"))
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs", str(n), "--steps", str(steps),
                          "--warmup", str(warm), "--dump-outputs", str(out)] + args,
                         capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    got = {k: np.load(out / (k + ".npy")) for k in ("obs", "reward", "done", "reason", "state")}
    sampled = os.path.exists(out / "env_index.npy")
    # up to 131 072 envs the whole batch fits the dump (440 B per env); at 4 Mi it is the bench's seeded sample
    assert sampled == (n > 131072), case
    ic = sample_ic_batch(n, N_RW, seed=0)
    if sampled:
        idx = np.load(out / "env_index.npy").astype(np.int64)
        assert idx.size > 100000 and np.all(np.diff(idx) > 0) and idx[-1] < n
        ic = np.ascontiguousarray(ic[:, idx])
    assert got["state"].shape == ic.shape
    level = "full" if "full" in args else "power" if "power" in args else "bare"
    sh = "sh" in args
    orc = _Oracle(_cfg(level, sh), ic, synthetic_sh_coefficients(70) if sh else None)
    del ic
    k = int(args[args.index("--substeps") + 1]) if "--substeps" in args else 1
    act = np.zeros(orc.st.shape[1], np.int32)
    for _ in range(warm + steps):
        ref = orc.step(act, k)
    _check_outputs((got["obs"], got["reward"], got["done"], got["reason"]), ref, o_tol, r_tol, case)
    _check_state(got["state"], orc.st, s_tol, case, power=level != "bare")
    # the whole slab row by row, relative to each row's largest magnitude (tests/test_gpu_bench.py's check) at the bare level
    if level == "bare" and not sh:
        scale = np.maximum(np.abs(orc.st).max(axis=1, keepdims=True), 1e-300)
        assert float((np.abs(got["state"] - orc.st) / scale).max()) < s_tol, case


# ---------------------------------------------------------------------------------------------------------------------------
# 2. large batches through the API
@pytest.mark.parametrize("n", [(1 << 20) + 77, 1 << 22])
def test_large_batch_step_device_mixed_actions_every_env(n):
    """Per-env actions on the device, int32 and int64 launches alternating, step statistics on: every env, the batch scalars
    and the done-mask words against the oracle after every K = 1 launch (12 launches: past the FSW ticks at 0 and 10)."""
    import torch
    cfg = _cfg()
    ic = sample_ic_batch(n, N_RW, seed=12)
    ic[12:12 + N_RW, ::997] = 400.0                         # wheels beyond their limit (314 rad/s): done bits in scattered words
    prop = BatchedPropagator(cfg, n)
    prop.reset(ic)
    orc = _Oracle(cfg, ic)
    del ic
    prop.set_step_stats(True)
    assert prop.kernel_info()["block"] == 256
    rng = np.random.default_rng(n)
    n_done = 0
    for t in range(12):
        a = rng.integers(0, 3, n).astype(np.int32)
        wide = t % 2 == 1
        d_act = torch.from_numpy(a.astype(np.int64) if wide else a).cuda()
        prop.step_device(d_act.data_ptr(), 1, int64=wide)
        prop.sync()
        ref = orc.step(a, 1)
        got = prop.get_obs()
        _check_outputs(got, ref, 1e-11, 1e-14, (n, t))
        rsum, ndone = prop.batch_stats()
        o_sum = float(np.sum(ref[1]))
        # every reward within 1e-14 of the oracle's, plus the summation order's rounding
        assert abs(rsum - o_sum) <= 1e-14 * n + 1e-12 * abs(o_sum), (n, t, rsum, o_sum)
        assert ndone == int(ref[2].sum()), (n, t)
        words = torch.as_tensor(prop.device_views()["done_mask"], device="cuda").cpu().numpy().view("<u8")
        assert np.array_equal(words, _done_words(ref[2].astype(bool))), (n, t)
        n_done += int(ref[2].sum())
        del d_act
    assert n_done > 0
    _check_state(prop.get_state(), orc.st, 1e-11, n)
    steps, ticks = prop.get_counters()
    assert np.array_equal(steps, orc.steps) and np.array_equal(ticks, orc.ticks)
    prop.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. rollouts at the bench's shapes
@pytest.mark.parametrize("actions", ["constant", "device"])
def test_rollout_65536_x_541_every_env_every_row(actions):
    """The rollout leg's first shape: one launch of 541 env steps (the reference's episode length + 1) for 65 536 envs; every
    row of the reward, reason and observation histories against the oracle stepped K = 1 at a time, then the state."""
    n, T = 65536, 541
    cfg = _cfg()
    ic = sample_ic_batch(n, N_RW, seed=6)
    prop = BatchedPropagator(cfg, n)
    prop.reset(ic)
    acts = np.random.default_rng(6).integers(0, 3, (T, n)).astype(np.int32) if actions == "device" else None
    h_obs, h_rew, h_why = prop.rollout(T, 1, actions=acts, constant_action=0)
    assert "rollout" in prop.kernel_info()["name"]
    orc = _Oracle(cfg, ic)
    zero = np.zeros(n, np.int32)
    for t in range(T):
        o_obs, o_rew, o_done, o_why = orc.step(zero if acts is None else acts[t], 1)
        assert np.array_equal(h_why[t], o_why), (t, int((h_why[t] != o_why).sum()))
        assert np.abs(h_rew[t] - o_rew).max() < 1e-14, (t, np.abs(h_rew[t] - o_rew).max())
        assert np.abs(h_obs[t] - o_obs).max() < 1e-11, (t, np.abs(h_obs[t] - o_obs).max(axis=1))
    assert (h_why[T - 1] & 1).all()                           # every episode ended by length at the last step
    _check_state(prop.get_state(), orc.st, 1e-11, actions)
    steps, ticks = prop.get_counters()
    assert np.array_equal(steps, orc.steps) and np.array_equal(ticks, orc.ticks)
    obs, rew, done, why = prop.get_obs()
    assert np.array_equal(obs, h_obs[T - 1]) and np.array_equal(rew, h_rew[T - 1]) and np.array_equal(why, h_why[T - 1])
    prop.close()


def test_rollout_4mi_x_100_final_state_and_sampled_history():
    """The rollout leg's second shape: 4 Mi envs x 100 steps with per-env device actions (the history is 20 GB on the device:
    its offsets pass 2^32 bytes).  Every env's final state and counters; the history rows of a seeded sample of 65 536 envs
    that holds the first 70 and the last 130."""
    import torch
    n, T = 1 << 22, 100
    cfg = _cfg()
    ic = sample_ic_batch(n, N_RW, seed=1)
    prop = BatchedPropagator(cfg, n)
    prop.reset(ic)
    orc = _Oracle(cfg, ic)
    del ic
    g = torch.Generator(device="cuda").manual_seed(100)
    act = torch.randint(0, 3, (T, n), dtype=torch.int32, device="cuda", generator=g)
    ob = torch.empty((T, 5, n), dtype=torch.float64, device="cuda")
    rw = torch.empty((T, n), dtype=torch.float64, device="cuda")
    wy = torch.empty((T, n), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    prop.step_n(T, 1, act.data_ptr(), 0, ob.data_ptr(), rw.data_ptr(), wy.data_ptr())
    prop.sync()
    assert "rollout" in prop.kernel_info()["name"]
    rng = np.random.default_rng(4)
    mid = rng.choice(np.arange(70, n - 130), size=65536 - 200, replace=False)
    idx = np.sort(np.concatenate([np.arange(70), np.arange(n - 130, n), mid]))
    it = torch.from_numpy(idx).cuda()
    s_obs, s_rew, s_why = ob[:, :, it].cpu().numpy(), rw[:, it].cpu().numpy(), wy[:, it].cpu().numpy()
    del ob, rw, wy
    for t in range(T):
        o_obs, o_rew, o_done, o_why = orc.step(act[t].cpu().numpy(), 1)
        assert np.array_equal(s_why[t], o_why[idx]), t
        assert np.abs(s_rew[t] - o_rew[idx]).max() < 1e-14, t
        assert np.abs(s_obs[t] - o_obs[:, idx]).max() < 1e-11, (t, np.abs(s_obs[t] - o_obs[:, idx]).max(axis=1))
    del act
    _check_state(prop.get_state(), orc.st, 1e-11, "4Mi")
    steps, ticks = prop.get_counters()
    assert np.array_equal(steps, orc.steps) and np.array_equal(ticks, orc.ticks)
    obs, rew, done, why = prop.get_obs()
    _check_outputs((obs, rew, done, why), (o_obs, o_rew, o_done, o_why), 1e-11, 1e-14, "4Mi last step")
    prop.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the RL-loop leg
@pytest.mark.parametrize("k,steps", [(1, 40), (1800, 2)])
def test_rl_loop_leg_against_the_oracle_env(k, steps):
    """bench.py's rl_loop: 65 536 envs of the full scenario, a device Philox pool of 4 096 ICs, device-side auto-reset, a
    linear-argmax policy on the device (int64 actions read in place) on one non-default stream.  The chosen actions are copied
    to the host so that the oracle env steps exactly the same ones (a near-tie cannot make the two sides diverge).  At K = 1
    the reference's max_length of 540 ends no episode within 40 steps: there it is 12, so that every env is restarted by the
    device three times."""
    import torch
    from basilisk_env_amd.envs import LeoPowerAttVecEnv
    n = 65536
    kw = {"n_rw": N_RW, "step_duration": 0.1 * k, "seed": 0, "device_reset_pool": 4096, "device_sampler": True}
    cfg = None
    if k == 1:
        probe = LeoPowerAttVecEnv(64, **kw)
        cfg = probe.cfg.copy()
        probe.close()
        cfg.max_length = 12
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = LeoPowerAttVecEnv(n, cfg=cfg, stream=side.cuda_stream, **kw)
        c = LeoPowerAttVecEnv(n, cfg=cfg, propagator_factory=_OmpOracle, **kw)
        ob = g.reset_tensors()
        oc = c.reset()
        assert np.abs(ob.cpu().numpy() - oc).max() < 1e-13
        gen = torch.Generator(device="cuda").manual_seed(0)
        w = torch.randn(5, 3, dtype=torch.float64, device="cuda", generator=gen)
        ret, length = np.zeros(n), np.zeros(n, np.int64)
        finished = 0
        obs_tol = 1e-10 if k == 1 else 1e-9
        for t in range(steps):
            act = (ob.reshape(n, 5) @ w).argmax(dim=1)
            assert act.dtype == torch.int64
            a = act.cpu().numpy()
            ob, rew, done, info = g.step_tensors(act)
            oc, rc, dc, _ = c.step(a)
            torch.cuda.synchronize()
            d = done.cpu().numpy()
            assert np.array_equal(d, dc), (t, int((d != dc).sum()))
            assert np.array_equal(info["reason"].cpu().numpy(), c.propagator.get_obs()[3]), t
            assert np.abs(rew.cpu().numpy() - rc).max() < 1e-12, t
            assert np.abs(ob.cpu().numpy() - oc).max() < obs_tol, (t, np.abs(ob.cpu().numpy() - oc).max(axis=(0, 2)))
            term_c, eps_c = c.propagator.get_terminal_obs()
            assert np.array_equal(info["episodes"].cpu().numpy(), eps_c), t
            ret += rc                                          # (the terminal step's reward is the episode's; its length is not)
            if d.any():
                tg = info["terminal_observation"].cpu().numpy()[d, :, 0]
                assert np.abs(tg - term_c[:, d].T).max() < obs_tol, t
                assert np.array_equal(info["episode_l"].cpu().numpy()[d], length[d]), t
                assert np.abs(info["episode_r"].cpu().numpy()[d] - ret[d]).max() < 1e-10, t
                ret[d], length[d] = 0.0, -1
            length += 1
            finished += int(d.sum())
        if k == 1:
            assert finished >= 3 * n and (eps_c >= 4).all()      # (the pool restart of reset_tensors counts one)
        s_tol = 1e-11 if k == 1 else 1e-10
        _check_state(g.propagator.get_state(), c.propagator.get_state(), s_tol, ("rl_loop", k), power=True)
        assert all(np.array_equal(x, y) for x, y in zip(g.propagator.get_counters(), c.propagator.get_counters()))
        g.close()
        c.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the default form policy at its boundaries
def _device_cus():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _form_run(level, n, k, launches, seed, tol, monkeypatch):
    for key in [v for v in os.environ if v.startswith("BSKGPU_")]:
        monkeypatch.delenv(key)                               # the default policy, no override
    cfg = _cfg(level)
    ic = sample_ic_batch(n, N_RW, seed=seed)
    prop = BatchedPropagator(cfg, n)
    prop.reset(ic)
    orc = _Oracle(cfg, ic)
    rng = np.random.default_rng(seed)
    for t in range(launches):
        a = rng.integers(0, 3, n).astype(np.int32)
        prop.step(a, k)
        ref = orc.step(a, k)
        _check_outputs(prop.get_obs(), ref, 1e-11 if k < 100 else 1e-9, 1e-12, (level, n, k, t))
    _check_state(prop.get_state(), orc.st, tol, (level, n, k), power=True)
    steps, ticks = prop.get_counters()
    assert np.array_equal(steps, orc.steps) and np.array_equal(ticks, orc.ticks)
    name = prop.kernel_info()["name"]
    prop.close()
    return name


@pytest.mark.parametrize("k", [15, 16])
@pytest.mark.parametrize("above", [False, True])
@pytest.mark.parametrize("level", ["power", "full"])
def test_default_form_at_the_switch_points(level, above, k, monkeypatch):
    """Wave-split forms run for launches of >= 16 sub-steps of batches of <= 64 spacecraft per CU of the device: the pair form
    at the power level, the three-wave form at the full level; one env more or one sub-step fewer is the single-wave form."""
    n = 64 * _device_cus() + (1 if above else 0)
    name = _form_run(level, n, k, 2, 50 + k, 1e-11, monkeypatch)
    base = "step_kernel<PM_J2,4,diag,%s" % ("power" if level == "power" else "scenario")
    split = ",pair>" if level == "power" else ",tri>"
    assert name == base + (split if (k >= 16 and not above) else ">"), name


def test_default_form_of_the_8192_env_shard_at_k1800(monkeypatch):
    """bench.py's strong_65536_total shard: 8 192 envs of the full scenario, K = 1 800, in the form the policy picks."""
    name = _form_run("full", 8192, 1800, 2, 2000, 1e-10, monkeypatch)
    assert name == "step_kernel<PM_J2,4,diag,scenario,tri>", name
