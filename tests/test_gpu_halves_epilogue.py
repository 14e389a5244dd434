"""GPU: the halves form with the launch's epilogue in the translational wave.  The rotational wave hands three values over
(|omega|^2, sum Omega_k^2, |sigma_BR|: bsk_device.hpp, HalvesLds::hand) and stores its own rows; observation, reward, reason, done
mask, counters, episode statistics and the wave sum are formed by the wave that integrated r and v.  Everything here is the form
forced on against the form forced off, bit for bit by test_gpu_halves._same, and against the CPU oracle at that file's bounds
(state 1e-12 of each row's scale, observations 1e-12, rewards 1e-14, reasons / dones / counters exact).

Shapes: n in {1, 63, 64, 65, 333}, one cell of each hub kind.  What the move can break: a done reason whose source now sits in the
other wave (WHEELS from the handed sum of squares, ORBIT from the translational wave's own |r|^2, LENGTH from the counters,
BATTERY from a charge the translational wave loads itself) alone and mixed with the others in one lane and one wave; the handed
|sigma_BR| where it is fresh in some lanes of a wave and held in others; the options that live in the epilogue; the ragged last
wave's done-mask word and wave sum.  The states are constructed so that every case is present, and each test counts what it saw."""
import numpy as np
import pytest

from basilisk_env_amd._lib import (DONE_BATTERY, DONE_LENGTH, DONE_ORBIT, DONE_WHEELS, FLAG_EPISODE_STATS, FLAG_OBS_ROWMAJOR,
                                   GRAV_PM, GRAV_PM_J2)
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
from test_gpu_halves import _against_oracle, _cfg, _done_words, _is_halves, _is_single, _Oracle, _same, make

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 333]
CELLS = [(GRAV_PM_J2, 4, "diag"), (GRAV_PM, 3, "full")]       # one cell of each hub kind
CHARGE_ROW = 7                                                # of the tail rows behind the wheel speeds (bskgpu.h: BSK_T_CHARGE)


def _lanes(n, *ks):
    return sorted({k for k in ks if 0 <= k < n})


def _pair(cfg, n, ic, stats=True):
    a, b = make(cfg, n, False), make(cfg, n, True)
    for p in (a, b):
        p.reset(ic)
        p.set_step_stats(stats)
    return a, b


def _constructed(n, n_rw, seed, battery):
    """-> cfg changes and an IC in which lanes leave the orbit band (`low`), carry a wheel beyond its limit (`fast`) and - with
    ``battery`` - an empty battery (`flat`), alone and together: lane 0 raises ORBIT (the translational wave's own |r|^2) and WHEELS
    (the rotational wave's handed sum) at once, lane 62 all three, and waves 1.. of the larger batches hold their own."""
    ic = sample_ic_batch(n, n_rw, seed=seed)
    radius = np.linalg.norm(ic[0:3], axis=0)
    low = _lanes(n, 0, 31, 62, n - 1, 130)
    fast = _lanes(n, 0, 5, 40, 62, 64 + 5, 130)
    flat = _lanes(n, 9, 40, 62, 200, 0 if n == 1 else -1) if battery else []       # (a batch of one: its only lane raises all three)
    r_min = 0.97 * float(radius.min())                     # (everything else stays above it: < 100 km of motion in 12 launches)
    ic[0:3, low] *= 0.95 * radius.min() / radius[low]
    ic[12:12 + n_rw, fast] = 400.0                         # beyond the wheel limit (314 rad/s)
    if battery:
        ic[12 + n_rw + CHARGE_ROW, flat] = 0.0
    return ic, r_min, low, fast, flat


@pytest.mark.parametrize("battery", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("grav,n_rw,hub", CELLS)
def test_every_done_reason_alone_and_mixed_in_one_wave(grav, n_rw, hub, n, battery):
    """12 launches from reset: launch 0 is the t = 0 launch (its zero-message chain), 1 - 8 have no FSW tick, 9 has the regular one.
    ``max_length`` = 9, and a masked reset of lanes 1 and 33 after launch 4 keeps them short of it: from launch 9 on LENGTH is up in
    some lanes of a wave and not in others, beside ORBIT / WHEELS / BATTERY alone and together in the constructed lanes.  Reasons
    as constructed and as the oracle's; rewards carry one penalty per WHEELS / BATTERY bit; done-mask words are the reasons'
    ballots; the batch scalars are the rewards' sum and the number of done envs."""
    cfg = _cfg(grav, n_rw, hub)
    cfg.max_length = 9
    ic, cfg.r_min, low, fast, flat = _constructed(n, n_rw, 80 + n, battery)
    a, b = _pair(cfg, n, ic)
    orc = _Oracle(cfg, ic)
    rng = np.random.default_rng(n)
    late = _lanes(n, 1, 33)
    seen = {}
    for t in range(12):
        if t == 5 and late:
            mask = np.zeros(n, np.uint8)
            mask[late] = 1
            for p in (a, b, orc):
                p.reset(ic, mask)                          # (their own initial conditions again: none of the constructed lanes)
        act = rng.integers(0, 3, n).astype(np.int32)
        a.step(act, 1)
        b.step(act, 1)
        ref = orc.step(act)
        ctx = (grav, n_rw, hub, n, battery, t)
        _same(a, b, ctx)
        _against_oracle(b, orc, ref, ctx)
        obs, rew, done, why = b.get_obs()
        why = why.astype(np.int64)
        steps_before = np.full(n, t, np.int64)
        if t >= 5:
            steps_before[late] = t - 5
        expect = np.where(steps_before >= 9, DONE_LENGTH, 0).astype(np.int64)
        expect[low] |= DONE_ORBIT
        expect[fast] |= DONE_WHEELS
        expect[flat] |= DONE_BATTERY
        assert np.array_equal(why, expect), (ctx, np.argwhere(why != expect)[:5].tolist())
        # one failure penalty per WHEELS / BATTERY bit on top of a base reward in [0, reward_mult], zero unless the action is 0
        base = rew + cfg.failure_penalty * (((why & DONE_WHEELS) != 0).astype(float) + ((why & DONE_BATTERY) != 0))
        assert (base > -1e-13).all() and (base < cfg.reward_mult + 1e-13).all(), (ctx, base.min(), base.max())
        assert (np.abs(base[act != 0]) < 1e-13).all() and (base[act == 0] > 0).all(), ctx
        words = np.zeros((n + 63) // 64, np.uint64)
        for k in np.flatnonzero(why):
            words[k >> 6] |= np.uint64(1) << np.uint64(k & 63)
        assert np.array_equal(_done_words(b), words), (ctx, "done mask")
        rsum, ndone = b.batch_stats()
        assert ndone == int(np.count_nonzero(why)) and abs(rsum - rew.sum()) < 1e-12 * max(1, n), (ctx, rsum, ndone)
        for w in np.unique(why):
            seen[int(w)] = seen.get(int(w), 0) + int((why == w).sum())
    assert _is_halves(b) and _is_single(a)
    # every case was there: each reason on its own and the mixtures, two of them (ORBIT | WHEELS) from different waves
    both = DONE_ORBIT | DONE_WHEELS | (DONE_BATTERY if battery and n == 1 else 0)
    want = {both, both | DONE_LENGTH}
    if n >= 63:
        want |= {0, DONE_LENGTH, DONE_ORBIT, DONE_WHEELS, DONE_ORBIT | DONE_LENGTH, DONE_WHEELS | DONE_LENGTH}
        if battery:
            want |= {DONE_BATTERY, DONE_BATTERY | DONE_LENGTH, DONE_WHEELS | DONE_BATTERY, DONE_ORBIT | DONE_WHEELS | DONE_BATTERY,
                     DONE_ORBIT | DONE_WHEELS | DONE_BATTERY | DONE_LENGTH}
    assert want <= set(seen), (n, battery, sorted(want - set(seen)), seen)
    a.close()
    b.close()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("grav,n_rw,hub", CELLS)
def test_handed_sigma_br_fresh_in_some_lanes_and_held_in_others(grav, n_rw, hub, n):
    """obs[0] and the reward (every action 0: the reward is a function of obs[0] alone) on launches 0, 9, 10, 11 from reset, where
    |sigma_BR| is the t = 0 chain's, the regular chain's, held, held; then a masked reset of lanes 0, 31, 63 and the last env, after
    which those lanes sit in another FSW phase than their wave: on their first launch and on either group's FSW tick the handed
    value is fresh in some lanes of a wave and held in the others."""
    cfg = _cfg(grav, n_rw, hub)
    ic = sample_ic_batch(n, n_rw, seed=90 + n)
    a, b = _pair(cfg, n, ic)
    orc = _Oracle(cfg, ic)
    act = np.zeros(n, np.int32)
    moved = _lanes(n, 0, 31, 63, n - 1)
    rest = sorted(set(range(n)) - set(moved))
    prev = None
    fresh_and_held = 0
    for t in range(26):
        if t == 12:
            mask = np.zeros(n, np.uint8)
            mask[moved] = 1
            fresh = sample_ic_batch(n, n_rw, seed=91 + n)
            for p in (a, b, orc):
                p.reset(fresh, mask)
        a.step(act, 1)
        b.step(act, 1)
        ref = orc.step(act)
        ctx = (grav, n_rw, hub, n, t)
        _same(a, b, ctx)
        obs, rew = b.get_obs()[:2]
        if t in (0, 9, 10, 11, 12, 13, 19, 20, 21, 22, 25):
            _against_oracle(b, orc, ref, ctx)
            assert np.abs(rew - cfg.reward_mult / (1.0 + obs[0] ** 2)).max() < 1e-14, ctx
        if prev is not None and t != 12:
            changed = obs[0] != prev
            # a lane's |sigma_BR| moves on its own FSW ticks only: launches 9, 19 for the lanes that kept their phase, 9 and 12 + 9
            # for the restarted ones (their t = 0 launch, 12, is left out: the reset stands between the two observations)
            assert (changed[rest] == (t in (9, 19))).all(), (ctx, "kept their phase")
            assert (changed[moved] == (t in (9, 21))).all(), (ctx, "restarted")
            if rest and changed.any() and not changed.all():
                fresh_and_held += 1
        prev = obs[0].copy()
    assert _is_halves(b)
    assert fresh_and_held >= (2 if rest else 0), fresh_and_held      # launches 19 and 21 (a batch of one env has one phase)
    a.close()
    b.close()


@pytest.mark.parametrize("option", ["episode_stats", "rowmajor", "int64", "no_step_stats"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("grav,n_rw,hub", CELLS)
def test_options_that_live_in_the_epilogue(grav, n_rw, hub, n, option):
    """Each option on its own for 12 launches across the FSW tick at launch 9, with episodes that end on the way (``max_length`` 6,
    a wheel over its limit in every 50th lane and in lane 0): episode statistics, the row-major observation copy, int64 actions
    read in place, and step statistics off (the batch scalars then come from the reward buffer, not from the launch's wave sums)."""
    import torch
    cfg = _cfg(grav, n_rw, hub)
    cfg.max_length = 6
    if option == "episode_stats":
        cfg.flags |= FLAG_EPISODE_STATS
    if option == "rowmajor":
        cfg.flags |= FLAG_OBS_ROWMAJOR
    ic = sample_ic_batch(n, n_rw, seed=70 + n)
    ic[12:12 + n_rw, ::50] = 400.0
    a, b = _pair(cfg, n, ic, stats=option != "no_step_stats")
    orc = _Oracle(cfg, ic)
    rng = np.random.default_rng(7 + n)
    wide = option == "int64"
    ended = 0
    for t in range(12):
        act = rng.integers(0, 3, n)
        d_act = torch.from_numpy(act.astype(np.int64) if wide else act.astype(np.int32)).cuda()
        for p in (a, b):
            p.step_device(d_act.data_ptr(), 1, int64=wide)
            p.sync()
        ref = orc.step(act.astype(np.int32))
        ctx = (grav, n_rw, hub, n, option, t)
        _same(a, b, ctx)
        if t in (0, 5, 6, 9, 10, 11):
            _against_oracle(b, orc, ref, ctx)
        ended += int(b.get_obs()[2].sum())
        va, vb = a.device_views(), b.device_views()
        keys = {"episode_stats": ("episode_return", "terminal_return", "terminal_length", "done"), "rowmajor": ("obs_rowmajor",)}.get(option, ())
        for key in keys:
            x, y = (torch.as_tensor(v[key], device="cuda").cpu().numpy() for v in (va, vb))
            assert np.array_equal(x, y), (ctx, key)
        if option == "rowmajor":
            rm = b.get_obs_rowmajor()
            obs, rew, done, why = b.get_obs()
            assert np.array_equal(rm[0], obs.T) and np.array_equal(rm[1], rew) and np.array_equal(rm[3], why), ctx
        if option == "episode_stats":
            done = torch.as_tensor(vb["done"], device="cuda").cpu().numpy()
            length = torch.as_tensor(vb["terminal_length"], device="cuda").cpu().numpy()
            assert np.array_equal(done.astype(bool), b.get_obs()[2]) and (length[done.astype(bool)] == t).all(), ctx
        del d_act
    assert ended >= 6 * n and _is_halves(b) and _is_single(a)        # lane 0 from the first launch, everybody from the seventh
    a.close()
    b.close()


@pytest.mark.parametrize("n", [1, 65])
def test_ragged_last_wave(n):
    """n = 1 and n = 65: the last wave holds ONE spacecraft and 63 lanes that shadow it.  Its done-mask word is bit 0 or nothing and
    its wave sum is that spacecraft's reward alone - the shadows contribute neither - on launches where it is done (a wheel over
    its limit: the failure penalty of 1 dwarfs every other reward of the batch, 64 shadows of it would show) and, in a second
    batch, on launches where it is not."""
    n_rw = 4
    cfg = _cfg(GRAV_PM_J2, n_rw, "diag")
    for over in (True, False):
        ic = sample_ic_batch(n, n_rw, seed=33 + n)
        if over:
            ic[12:12 + n_rw, n - 1] = 400.0
        a, b = _pair(cfg, n, ic)
        orc = _Oracle(cfg, ic)
        act = np.zeros(n, np.int32)
        for t in range(3):
            a.step(act, 1)
            b.step(act, 1)
            ref = orc.step(act)
            _same(a, b, (n, over, t))
            _against_oracle(b, orc, ref, (n, over, t))
            rew, done = b.get_obs()[1:3]
            words = _done_words(b)
            assert words.shape == ((n + 63) // 64,) and int(words[-1]) == (1 if over else 0), (n, over, t, words)
            assert bool(done[n - 1]) == over and (rew[n - 1] < -0.5) == over, (n, over, t)
            rsum, ndone = b.batch_stats()
            assert ndone == int(over), (n, over, t, ndone)
            # the scalars are joined from the wave sums: the first wave's 64 rewards in the butterfly's order, then the last wave's one
            assert abs(rsum - rew.sum()) < 1e-12 and (n > 1 or rsum == rew[0]), (n, over, t, rsum)
        assert _is_halves(b)
        a.close()
        b.close()
