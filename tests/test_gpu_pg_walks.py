"""GPU: the column walks of the policy-gradient loop past their first trips - bsk_gae, bsk_reward_norm, bsk_pg_episodes,
bsk_pg_log_update and bsk_adv_normalize (csrc/bsk_fit.hip: gae_kernel, adv_*_kernel; csrc/bsk_rewnorm.hip; csrc/bsk_pglog.hip;
definition in include/bskgpu.h) at the shapes of tests/_pg_walk_cases.py, and ``policy.PolicyGradient`` off the one shape every
other end-to-end test runs it at.

Everything here is an equality of bits against the numpy restatements of basilisk_env_amd/policy_ref.py, which
tests/test_pg_walk_cases_host.py holds to plain loops at these very shapes before this file runs: there is no tolerance in it.  The
shapes are the smallest at which each loop takes a trip it has not taken on a device before: a second and a third trip of the
batched row loops (T = 16, 17, 24), a second and a third trip of the apply launch's row stride (T = 1 025, 2 049), a join whose
every lane holds one, two and three partial rows (4 096, 8 192, 8 321 envs), whole and broken unrolled trips of gae_kernel around
the edges of its workgroups.  Every history has five padding columns that must never be read (NaN, reason 0xFF, action 1), every
output five that must never be written, and every output, state and work buffer guard words behind it; the histories are checked
as read only."""
import numpy as np
import pytest

from _device_bits import download as _download, same as _same
from _pg_cond_bounds import adv_case
from _pg_log_cases import diag_case
from _pg_walk_cases import (GAE_COEFS, GAE_N, GAE_T, GRID_SHAPES, LAP_SHAPES, LOG_UPDATE_NORMS, LOG_UPDATE_ROWS, LOOP, ROW_SHAPES, SEQUENCE_N,
                            STALE_N, episode_work_ref, gae_placement, gae_poisoned, gae_reach, last_wave_case, reward_padded, sequence_cases,
                            tag, walk_episode_case, walk_reward_case, waves)
from _policy_bounds import seeded_policy
from _reward_norm_cases import CLIP, EPS, GAMMA
from basilisk_env_amd import policy as P
from basilisk_env_amd._lib import FLAG_AUTO_RESET, GRAV_PM_J2
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
from test_gpu_fit import _dev
from test_gpu_pg import _PG
from test_gpu_pg_log import _Buffers as _LogBuffers, _upload

pytestmark = pytest.mark.gpu

GUARD = -7.0
PAD = 5
KEYS = ("reward", "reason", "action", "value", "ret")


def _guarded(count, dtype, fill=GUARD, words=2):
    import torch
    return torch.full((count + words,), fill, dtype=dtype, device="cuda")


# ------------------------------------------------------------------------------------------------------------------ bsk_reward_norm
class _Reward(object):
    """the state words, the running returns and the work buffer of n envs on the device, each with two guard words behind it, carried
    from call to call; a call uploads its own histories [T][n + PAD] with poisoned padding and checks them as read only"""

    def __init__(self, n, state, ret_run, work=None):
        import torch
        self.n = n
        self.state = _dev(np.r_[state.view(np.float64), [GUARD, GUARD]])
        self.R = _dev(np.r_[ret_run, [GUARD, GUARD]])
        self.work = _guarded(3 * waves(n), torch.float64) if work is None else work
        self.words = self.work.numel() - 2
        assert P.reward_norm_work_bytes(n) == 8 * 3 * waves(n) <= 8 * self.words

    def call(self, case, where, update=True, in_place=False):
        """-> out f64 (T, n)"""
        import torch
        T, n = case["reward"].shape
        stride = n + PAD
        full = reward_padded(case, stride)
        reward, reason = _dev(full["reward"]), _dev(full["reason"])
        out = None if in_place else _guarded(T * stride, torch.float64)
        torch.cuda.synchronize()
        P.reward_normalize(reward, reason, T, n, self.state[:8], None if in_place else out[:T * stride], self.R[:n] if update else None,
                           self.work[:self.words] if update else None, GAMMA, EPS, CLIP, update, stride=stride)
        torch.cuda.synchronize()
        assert _same(reason.cpu().numpy(), full["reason"]), where          # the reason history, padding included, is read only
        got = reward.cpu().numpy()
        if in_place:
            assert _same(got[:, n:], full["reward"][:, n:]), where         # the padding is nobody's
            return got[:, :n].copy()
        assert _same(got, full["reward"]), where                           # ... and so is the reward history, out of place
        flat = out.cpu().numpy()
        assert (flat[T * stride:] == GUARD).all() and (flat[:T * stride].reshape(T, stride)[:, n:] == GUARD).all(), where
        return flat[:T * stride].reshape(T, stride)[:, :n].copy()

    def host(self, where):
        """-> (state u64 (8,), ret_run f64 (n,), work u64 (words,)), the guards checked"""
        state, R, work = self.state.cpu().numpy(), self.R.cpu().numpy(), self.work.cpu().numpy()
        assert (state[8:] == GUARD).all() and (R[self.n:] == GUARD).all() and (work[self.words:] == GUARD).all(), where
        return state[:8].copy().view(np.uint64), R[:self.n].copy(), work[:self.words].copy().view(np.uint64)


def _reward_ref(case, update=1):
    return P.reward_norm_ref(case["reward"], case["reason"], GAMMA, EPS, CLIP, update, case["state"], case["ret_run"], with_work=True)


def _reward_check(run, case, where, update=True, in_place=False):
    out = run.call(case, where, update, in_place)
    want_out, want_words, want_R, want_work = _reward_ref(case, int(update))
    words, R, work = run.host(where)
    bad = np.argwhere(out.view(np.int64) != want_out.view(np.int64))
    assert _same(out, want_out), (where, "out", len(bad), bad[:4])
    assert _same(words, want_words), (where, "state", words, want_words)
    assert _same(R, want_R), (where, "ret_run")
    if update:
        assert _same(work[:want_work.size], want_work.reshape(-1)), (where, "work")
    return out, words, R, work


@pytest.mark.parametrize("n,T", ROW_SHAPES + LAP_SHAPES)
def test_reward_norm_past_one_batch_of_rows_and_one_lap_of_the_join(n, T):
    case = walk_reward_case(n, T)
    _, words, _, work = _reward_check(_Reward(n, case["state"], case["ret_run"]), case, tag(n, T))
    assert int(words[2]) == int(case["state"][2]) + T * n and int(words[6]) == 4, tag(n, T)
    assert work.reshape(-1, 3)[:, 2].astype(np.int64).sum() == T * n, tag(n, T)


@pytest.mark.parametrize("update", [True, False])
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n,T", GRID_SHAPES)
def test_reward_norm_past_the_apply_launchs_grid_of_rows(n, T, in_place, update):
    case = walk_reward_case(n, T)
    where = (tag(n, T), "in place" if in_place else "out of place", "update" if update else "frozen")
    run = _Reward(n, case["state"], case["ret_run"])
    out, words, R, work = _reward_check(run, case, where, update, in_place)
    if not update:
        assert _same(words, case["state"]) and _same(R, case["ret_run"]) and (work.view(np.float64) == GUARD).all(), where
    # (a row only a later trip of the row stride reaches holds what the restatement gives, not what it held)
    assert T <= 1024 or not _same(out[1024:], case["reward"][1024:]), where


def test_reward_norm_three_calls_of_different_length_on_one_state():
    cases = sequence_cases("reward")
    run = _Reward(SEQUENCE_N, cases[0]["state"], cases[0]["ret_run"])
    state, R = cases[0]["state"], cases[0]["ret_run"]
    for i, c in enumerate(cases):
        c = dict(c, state=state, ret_run=R)
        _, state, R, _ = _reward_check(run, c, ("call %d of the sequence" % i, c["reward"].shape))
    assert int(state[6]) == 3 + len(cases)


def test_reward_norm_does_not_read_the_stale_rows_of_a_larger_calls_work_buffer():
    big, small = (walk_reward_case(n, 9) for n in STALE_N)
    first = _Reward(STALE_N[0], big["state"], big["ret_run"])
    _, _, _, filled = _reward_check(first, big, "the call at 300 envs")
    assert waves(STALE_N[0]) == 5 and filled.reshape(5, 3)[:, 2].all()
    second = _Reward(STALE_N[1], small["state"], small["ret_run"], work=first.work)
    _, _, _, work = _reward_check(second, small, "the call at 65 envs on the work buffer of one at 300")
    assert _same(work[6:], filled[6:]) and not _same(work[:6], filled[:6])         # rows 2 .. 4 are still the larger call's


# ------------------------------------------------------------------------------------------------------------------ bsk_pg_episodes
def _episodes_check(case, keys, where, buf=None):
    """one bsk_pg_episodes into slot 0 -> the slot's columns 0 .. 15; the state, the work rows, the guards and the histories checked"""
    T, n = case["reward"].shape
    stride, W = n + PAD, waves(n)
    d, full = _upload(case, stride, keys)
    buf = _LogBuffers(n, 1, case["state"]) if buf is None else buf
    buf.episodes(d, T, stride)
    out = buf.host()
    for k in keys:                                             # the histories, padding columns included, are read only
        assert _same(d[k].cpu().numpy(), full[k]), (where, k)
    want, (want_R, want_L) = P.pg_episodes_ref(**{k: case[k] for k in tuple(keys) + ("state",)})
    row = out["rows"][0, :16].copy()
    assert _same(row, want), (where, "row", row, want)
    assert (out["rows"][0, 16:] == GUARD).all(), where          # columns 16 .. 25 are bsk_pg_log_update's
    assert _same(out["R"][:n], want_R) and _same(out["L"][:n], want_L), (where, "state")
    work, want_work = out["work"][:19 * W].view(np.uint64).reshape(W, 19), episode_work_ref(case, keys)
    assert _same(work, want_work), (where, "work", np.argwhere(work != want_work)[:4])
    return row, work


@pytest.mark.parametrize("with_value", [True, False])
@pytest.mark.parametrize("with_action", [True, False])
@pytest.mark.parametrize("n,T", ROW_SHAPES + LAP_SHAPES)
def test_pg_episodes_past_one_batch_of_rows_and_one_lap_of_the_join(n, T, with_action, with_value):
    case = walk_episode_case(n, T)
    keys = tuple(k for k in KEYS if (with_action or k != "action") and (with_value or k not in ("value", "ret")))
    where = (tag(n, T), "actions" if with_action else "no actions", "values" if with_value else "no values")
    row, _ = _episodes_check(case, keys, where)
    assert row[0] == (case["reason"] != 0).sum() > 0 and row[10:13].sum() == (T * n if with_action else 0), where
    assert np.isnan(row[14]) == (not with_value), where


def test_pg_episodes_when_only_the_tail_waves_one_env_ends_an_episode():
    case = last_wave_case()
    n, T = LAP_SHAPES[-1]
    row, work = _episodes_check(case, KEYS, tag(n, T) + ", only the last env ends an episode")
    f = work.view(np.float64)
    assert np.isnan(f[:130, 7:9]).all() and np.isfinite(f[130, 7:9]).all() and not work[:130, 9].any() and work[130, 9] == 3
    assert row[0] == 3 and _same(row[3:5], f[130, 7:9].copy()) and row[5] == work[130, 10] and row[1] == f[130, 0]


def test_pg_episodes_three_calls_of_different_length_on_one_state():
    cases = sequence_cases("episode")
    buf = _LogBuffers(SEQUENCE_N, 1, cases[0]["state"])
    state = cases[0]["state"]
    for i, c in enumerate(cases):
        c = dict(c, state=state)
        _episodes_check(c, KEYS, ("call %d of the sequence" % i, c["reward"].shape), buf)
        _, state = P.pg_episodes_ref(**{k: c[k] for k in KEYS + ("state",)})


@pytest.mark.parametrize("n_norms", LOG_UPDATE_NORMS)
@pytest.mark.parametrize("n_rows", LOG_UPDATE_ROWS)
def test_pg_log_update_over_many_rows(n_rows, n_norms):
    diag, norms = diag_case(n_rows, n_norms or 1, n_rows + (n_norms or 0))
    norms = norms if n_norms else None
    buf = _LogBuffers(1, 2, counter=5)                         # slot 1
    d_diag, d_norms = _dev(diag), None if norms is None else _dev(norms)
    buf.update(d_diag, d_norms)
    out = buf.host()
    assert _same(out["rows"][1, 16:], P.pg_log_update_ref(diag, norms)), (n_rows, n_norms)
    assert (out["rows"][1, :16] == GUARD).all() and (out["rows"][0] == GUARD).all(), (n_rows, n_norms)
    assert _same(d_diag.cpu().numpy(), diag) and (norms is None or _same(d_norms.cpu().numpy(), norms))


# ------------------------------------------------------------------------------------------------------------------ bsk_adv_normalize
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n,rows", LAP_SHAPES)
def test_adv_normalize_at_one_two_and_three_entries_per_lane_of_the_join(n, rows, masked):
    import torch
    stride, eps = n + PAD, 1e-8
    adv, alive = adv_case(rows, n, 10 * n + rows, masked=masked)
    want, mom = P.adv_normalize_ref(adv, alive, eps)
    padded = np.full((rows, stride), np.nan, np.float32)
    padded[:, :n] = adv
    d_alive = None
    if masked:
        full = np.full((rows, stride), 0xFF, np.uint8)
        full[:, :n] = alive
        d_alive = _dev(full)
    words = P.adv_normalize_work_bytes(n) // 8
    for in_place in (False, True):
        where = (tag(n, rows), "masked" if masked else "every sample", "in place" if in_place else "out of place")
        d_adv, work = _dev(padded), _guarded(words, torch.float64, -3.0, 5)
        out = None if in_place else _guarded(rows * stride, torch.float32)
        torch.cuda.synchronize()
        P.normalize_advantages(d_adv, rows, n, None if in_place else out[:rows * stride], d_alive, eps, stride, work[:words])
        torch.cuda.synchronize()
        w = work.cpu().numpy()
        assert _same(w[:4], mom) and (w[words:] == -3.0).all(), (where, w[:4], mom)
        assert mom[3] == (rows * n if alive is None else int((alive != 0).sum())), where
        got = d_adv.cpu().numpy()
        if in_place:
            assert _same(got[:, :n], want) and _same(got[:, n:], padded[:, n:]), where
        else:
            flat = out.cpu().numpy()
            block = flat[:rows * stride].reshape(rows, stride)
            assert _same(block[:, :n], want) and (block[:, n:] == GUARD).all() and (flat[rows * stride:] == GUARD).all(), where
            assert _same(got, padded), where                               # the raw estimate stays
        if masked:
            assert _same(d_alive.cpu().numpy(), full), where


# ------------------------------------------------------------------------------------------------------------------ bsk_gae
class _Gae(object):
    """the histories of one GAE case on the device, [T][n + PAD] with poisoned padding, and ``last_value`` with NaN behind it"""

    def __init__(self, reward, reason, value, last):
        T, n = reward.shape
        self.T, self.n, self.stride = T, n, n + PAD
        self.full = {}
        for k, a, fill in (("reward", reward, np.nan), ("reason", reason, 0xFF), ("value", value, np.nan)):
            self.full[k] = np.full((T, self.stride), fill, a.dtype)
            self.full[k][:, :n] = a
        self.full["last"] = np.r_[last, np.full(2, np.nan, np.float32)].astype(np.float32)
        self.d = {k: _dev(a) for k, a in self.full.items()}

    def run(self, gamma, lam, with_last, with_ret, where):
        """-> (adv f32 (T, n), ret f64 (T, n) or None); the padding and the guards behind both outputs checked"""
        import torch
        T, n, stride = self.T, self.n, self.stride
        adv, ret = _guarded(T * stride, torch.float32), _guarded(T * stride, torch.float64)
        torch.cuda.synchronize()
        P.gae(self.d["reward"], self.d["reason"], self.d["value"], self.d["last"][:n] if with_last else None, T, n, adv[:T * stride],
              ret[:T * stride] if with_ret else None, gamma, lam, stride=stride)
        torch.cuda.synchronize()
        out = []
        for flat, written in ((adv.cpu().numpy(), True), (ret.cpu().numpy(), with_ret)):
            block = flat[:T * stride].reshape(T, stride)
            assert (flat[T * stride:] == GUARD).all() and (block[:, n:] == GUARD).all(), where
            assert written or (block == GUARD).all(), where
            out.append(block[:, :n].copy() if written else None)
        return out

    def check_read_only(self, where):
        for k, a in self.full.items():
            assert _same(self.d[k].cpu().numpy(), a), (where, k)


@pytest.mark.parametrize("n", GAE_N)
@pytest.mark.parametrize("T", GAE_T)
def test_gae_over_unrolled_trips_remainders_and_workgroup_edges(T, n):
    reward, reason, value, last = gae_placement(T, n)
    dev = _Gae(reward, reason, value, last)
    reach = gae_reach(reason)
    for gamma, lam in GAE_COEFS:
        got = {}
        for with_last in (False, True):
            want_adv, want_ret = P.gae_ref(reward, reason, value, last if with_last else None, gamma, lam)
            for with_ret in (False, True):
                where = ("(T, n) = (%d, %d)" % (T, n), gamma, lam, "last_value" if with_last else "no last_value", "ret" if with_ret else "no ret")
                adv, ret = dev.run(gamma, lam, with_last, with_ret, where)
                assert _same(adv, want_adv), (where, "adv", np.argwhere(adv.view(np.int32) != want_adv.view(np.int32))[:4])
                assert ret is None or _same(ret, want_ret), (where, "ret", np.argwhere(ret.view(np.int64) != want_ret.view(np.int64))[:4])
                got[with_last] = ret if ret is not None else got.get(with_last)
        # the cut, on the device's own numbers: last_value shows behind a column's last end and nowhere else
        differ = got[False] != got[True]
        assert np.array_equal(differ, reach if gamma != 0.0 else np.zeros_like(reach)), (T, n, gamma, lam)
    dev.check_read_only((T, n))


@pytest.mark.parametrize("n", GAE_N)
@pytest.mark.parametrize("T", [9, 33])
def test_gae_a_spoilt_column_leaves_its_neighbours_bits_alone(T, n):
    reward, reason, value, last = gae_placement(T, n)
    bad_reward, bad_value, cols = gae_poisoned(reward, value)
    keep = np.setdiff1d(np.arange(n), cols)
    where = ("(T, n) = (%d, %d)" % (T, n), "one NaN or inf per wave, in columns %s" % cols)
    clean = _Gae(reward, reason, value, last).run(0.97, 0.9, True, True, where)
    dirty = _Gae(bad_reward, reason, bad_value, last).run(0.97, 0.9, True, True, where)
    want = P.gae_ref(reward, reason, value, last, 0.97, 0.9)
    for name, a, b, w in zip(("adv", "ret"), clean, dirty, want):
        assert _same(a, w), (where, name)
        assert _same(a[:, keep], b[:, keep]), (where, name, np.argwhere(a[:, keep] != b[:, keep])[:4])
    assert not np.isfinite(dirty[1][:, cols]).all(axis=0).any(), where        # (every spoilt column shows it)


# ------------------------------------------------------------------------------------------------------------------ the loop
HIST = (("reward", np.float64, 1), ("reason", np.uint8, 1), ("action", np.int32, 1), ("value", np.float32, 1), ("logp", np.float32, 1),
        ("adv", np.float32, 1), ("ret", np.float64, 1), ("reward_norm", np.float64, 1), ("obs", np.float64, 5))
MB = (("mb_action", np.int32, "action"), ("mb_logp", np.float32, "logp"), ("mb_ret", np.float64, "ret"), ("mb_value", np.float32, "value"))


def _loop(side, shuffle):
    L = LOOP
    n, T = L["n_envs"], L["n_steps"]
    spec, params = seeded_policy(L["hidden"], "relu", L["value_hidden"], seed=16)
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_AUTO_RESET
    cfg.max_length = L["max_length"]                        # (episodes end, and start again, inside and across the rollouts)
    root = BatchedPropagator(cfg, n, stream=side.cuda_stream)
    root.set_ic_pool(sample_ic_batch(23, 4, seed=73))
    root.reset(sample_ic_batch(n, 4, seed=72))
    root.step(np.zeros(n, np.int32), 1)                     # (the observation buffers hold a step's output)
    steps, ticks = root.get_counters()
    root.set_counters(steps + np.arange(n, dtype=np.int32) % 4, ticks)          # episodes end at different steps
    f = _PG(spec, params, lr=1e-2)
    f.fit.max_grad_norm = L["max_grad_norm"]
    pg = P.PolicyGradient(root, f.policy, f.fit, T, gamma=L["gamma"], lam=L["lam"], clip=0.2, ent_coef=0.01, epochs=L["epochs"],
                          minibatches=L["minibatches"], substeps=1, normalize_advantages=True, shuffle=shuffle, seed=9,
                          cliprange_vf=L["cliprange_vf"], log_capacity=L["log_capacity"], normalize_rewards=True,
                          reward_clip=L["reward_clip"], reward_eps=L["reward_eps"])
    f.policy.set_rng(3, 0)
    return root, f, pg


@pytest.mark.parametrize("shuffle", [False, True])
def test_the_loop_off_its_one_shape_holds_every_stage_to_its_restatement(shuffle):
    """200 envs - a partial last wave -, 18 steps - two batches of rows and a tail -, three minibatches of six rows, two epochs, a
    relu (32, 16) policy with a (48,) value network, everything of PPO2's update on, a ring of two rows under three iterations.
    After every iterate() each stage is held to its restatement of the loop's OWN downloaded inputs."""
    import torch
    L = LOOP
    n, T, mbs, epochs, cap = L["n_envs"], L["n_steps"], L["minibatches"], L["epochs"], L["log_capacity"]
    rows = T // mbs
    M = rows * n
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        root, f, pg = _loop(side, shuffle)
        torch.cuda.synchronize()
        bufs = pg.buffers()
        carried = 0
        for it in range(L["iterations"]):
            where = ("shuffle" if shuffle else "no shuffle", "iteration %d" % it)
            words0, run0 = pg.reward_norm_state()
            ep_R0, ep_L0, counter0 = pg.episode_state()
            epoch0 = pg.shuffle_state()[1] if shuffle else None
            assert counter0 == it and int(words0[6]) == it, where
            log = pg.iterate()
            assert log.shape == (epochs * mbs, 8) and pg.grad_norms.shape == (epochs * mbs, 2), where
            h = {k: _download(bufs[k], dt, (T + (k == "obs")) * w * n).reshape((-1, n) if w == 1 else (-1, w, n)) for k, dt, w in HIST}
            h["last_value"] = _download(bufs["last_value"], np.float32, n)
            # the rewards scaled by the running deviation, the statistics and the running returns carried from the call before
            out, words, run = P.reward_norm_ref(h["reward"], h["reason"], L["gamma"], L["reward_eps"], L["reward_clip"], 1, words0, run0)
            got_words, got_run = pg.reward_norm_state()
            assert _same(h["reward_norm"], out), (where, "reward_norm")
            assert _same(got_words, words) and _same(got_run, run), (where, "reward_state / ret_run", got_words, words)
            assert int(words[2]) == (it + 1) * T * n and not _same(out, h["reward"]), where
            # the estimator on the scaled rewards
            want_adv, want_ret = P.gae_ref(out, h["reason"], h["value"], h["last_value"], L["gamma"], L["lam"])
            assert _same(h["adv"], want_adv) and _same(h["ret"], want_ret), (where, "adv / ret")
            if not shuffle:
                normed = _download(bufs["adv_norm"], np.float32, T * n).reshape(T, n)
                for g in range(mbs):
                    want, mom = P.adv_normalize_ref(h["adv"][g * rows:(g + 1) * rows])
                    assert mom[3] == M and mom[1] > 0 and _same(normed[g * rows:(g + 1) * rows], want), (where, "adv_norm, group %d" % g)
            else:
                # the mb_* buffers hold the last minibatch of the last epoch: the permutation of the epoch word before the last advance
                seed, epoch = pg.shuffle_state()
                assert seed == 9 and epoch == epoch0 + epochs == (it + 1) * epochs, where
                mb = P.pg_gather_ref((seed, epoch - 1), n, (mbs - 1) * M, M, obs=h["obs"][:T], action=h["action"], adv=h["adv"],
                                     logp=h["logp"], ret=h["ret"], value=h["value"])
                assert _same(_download(bufs["mb_obs"], np.float64, 5 * M).reshape(5, M), mb["obs"]), (where, "mb_obs")
                for name, dt, k in MB:
                    assert _same(_download(bufs[name], dt, M), mb[k]), (where, name)
                want, mom = P.adv_normalize_ref(mb["adv"].reshape(rows, n))
                assert mom[3] == M and _same(_download(bufs["mb_adv"], np.float32, M), want.reshape(-1)), (where, "mb_adv")
                assert len(np.unique(mb["index"] // n)) > rows, where          # (the minibatch is no group of rows)
            # the newest row of the training log: the episodes of the RAW rewards, carried across the iterations, and the update's sums
            row, (ep_R, ep_L) = P.pg_episodes_ref(h["reward"], h["reason"], h["action"], h["value"], h["ret"], state=(ep_R0, ep_L0))
            raw = _download(bufs["log"], np.float64, epochs * T * 8).reshape(epochs * T, 8)
            norms = _download(bufs["grad_norm_log"], np.float64, epochs * mbs * 2).reshape(epochs * mbs, 2)
            assert _same(norms, pg.grad_norms), where
            its, table = pg.training_log()
            assert list(its) == list(range(max(0, it + 1 - cap), it + 1)), (where, its)          # the ring wraps in iteration 2
            assert _same(table[-1, :16], row), (where, "log columns 0 .. 15", table[-1, :16], row)
            assert _same(table[-1, 16:], P.pg_log_update_ref(raw, norms)), (where, "log columns 16 .. 25")
            got_R, got_L, counter = pg.episode_state()
            assert _same(got_R, ep_R) and _same(got_L, ep_L) and counter == it + 1, (where, "ep_return / ep_len")
            # episodes of five steps end inside the rollout of eighteen, in several rows, and run across its end
            ended = h["reason"] != 0
            assert ended.any(axis=1).sum() >= 3 and 0 < ended.sum() < T * n // 2 and row[0] == ended.sum(), where
            assert row[10:13].sum() == T * n and np.isfinite(row[14]) and table[-1, 23] == epochs * T * n, where
            carried += int((ep_L0 > 0).sum())
            assert (got_L > 0).any(), where
        assert carried > 0                                  # some envs came into an iteration in the middle of an episode
        assert f.fit.state()["steps"] == L["iterations"] * epochs * mbs
        pg.close()
        f.close()
        root.close()
