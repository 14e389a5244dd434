"""GPU: the reward scaling of the policy-gradient loop - bsk_reward_norm (csrc/bsk_rewnorm.hip; definition in include/bskgpu.h) and
``policy.PolicyGradient(normalize_rewards=True)``.

Everything here is an equality of bits: f64 additions, products, one division per sample and one square root in a fixed order,
which ``reward_norm_ref`` repeats (held to a plain loop, and the device's walk itself to it on the host, by
tests/test_reward_norm_host.py before this file runs it).  Shapes are the smallest at which each path is taken: 65 envs are two
waves, 4097 are 65 partial rows - the join's second entry per lane; 7 rows are a tail with no full batch of eight, 9 a tail behind
one.  Both histories have five padding columns that must never be read (NaN, reason 0xFF), the output has five that must never be
written, and the state, the running returns, the work buffer and the output have guard words behind them.

The graph test captures once, with no call before it, and replays THREE times: a capture executes nothing, and the statistics
accumulate across replays, so that is what equals three eager rounds."""
import ctypes as C

import numpy as np
import pytest

from _device_bits import download as _download, same as _same
from _policy_bounds import seeded_policy
from _reward_norm_cases import CLIP, EPS, GAMMA, SHAPES, padded, reward_case
from basilisk_env_amd import _lib
from basilisk_env_amd import policy as P
from basilisk_env_amd._lib import FLAG_AUTO_RESET, GRAV_PM_J2
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
from test_gpu_fit import _dev
from test_gpu_pg import _PG

pytestmark = pytest.mark.gpu

EINVAL = -1
GUARD = -7.0
PAD = 5
F = {name: c for c, name in enumerate(P.REWARD_NORM_STATE_FIELDS)}


class _Buffers(object):
    """the histories [T][n + PAD] with poisoned padding, and the state, the running returns, the work buffer and the output on the
    device, each with two guard words behind it; the work buffer and the output start filled with the guard value"""

    def __init__(self, case, in_place=False):
        import torch
        T, n = case["reward"].shape
        self.T, self.n, self.stride, self.W = T, n, n + PAD, (n + 63) // 64
        self.full = padded(case, self.stride)
        self.reward, self.reason = _dev(self.full["reward"]), _dev(self.full["reason"])
        self.state = _dev(np.r_[case["state"].view(np.float64), [GUARD, GUARD]])
        self.R = _dev(np.r_[case["ret_run"], [GUARD, GUARD]])
        self.work = torch.full((3 * self.W + 2,), GUARD, dtype=torch.float64, device="cuda")
        self.out = None if in_place else torch.full((T * self.stride + 2,), GUARD, dtype=torch.float64, device="cuda")
        assert P.reward_norm_work_bytes(n) == 8 * 3 * self.W
        torch.cuda.synchronize()

    def run(self, update=True, gamma=GAMMA, eps=EPS, clip=CLIP, stream=0):
        P.reward_normalize(self.reward, self.reason, self.T, self.n, self.state[:8], None if self.out is None else self.out[:self.T * self.stride],
                           self.R[:self.n] if update else None, self.work[:3 * self.W] if update else None, gamma, eps, clip, update,
                           stride=self.stride, stream=stream)

    def host(self):
        import torch
        torch.cuda.synchronize()
        T, n, stride = self.T, self.n, self.stride
        state, R, work = self.state.cpu().numpy(), self.R.cpu().numpy(), self.work.cpu().numpy()
        assert (state[8:] == GUARD).all() and (R[n:] == GUARD).all() and (work[3 * self.W:] == GUARD).all()
        assert _same(self.reason.cpu().numpy(), self.full["reason"])          # the reason history, padding included, is read only
        reward = self.reward.cpu().numpy()
        if self.out is None:
            out = reward
        else:
            flat = self.out.cpu().numpy()
            assert (flat[T * stride:] == GUARD).all()
            out = flat[:T * stride].reshape(T, stride)
            assert (out[:, n:] == GUARD).all()                     # the padding of the output is never written
            assert _same(reward, self.full["reward"])              # ... and the reward history is read only
        assert np.isnan(reward[:, n:]).all()
        return dict(out=out[:, :n].copy(), state=state[:8].copy().view(np.uint64), R=R[:n].copy(), work=work[:3 * self.W].copy().view(np.uint64))


def _ref(case, update=1, gamma=GAMMA, eps=EPS, clip=CLIP):
    return P.reward_norm_ref(case["reward"], case["reason"], gamma, eps, clip, update, case["state"], case["ret_run"], with_work=True)


def _equal(got, want, tag=None):
    out, words, R, work = want
    assert _same(got["out"], out), tag
    assert _same(got["state"], words), (tag, got["state"], words)
    assert _same(got["R"], R), tag
    if work is not None:
        assert _same(got["work"], work.reshape(-1)), tag


# ------------------------------------------------------------------------------------------------------------------ bsk_reward_norm
@pytest.mark.parametrize("n,T", SHAPES)
def test_everything_equals_the_restatement_bit_for_bit(n, T):
    case = reward_case(T, n, 10 * n + T)
    buf = _Buffers(case)
    buf.run()
    got = buf.host()
    _equal(got, _ref(case), (n, T))
    assert (case["ret_run"] != 0).all() and case["state"][:3].all()                 # (what came in was not zero)
    assert int(got["state"][F["count"]]) == int(case["state"][F["count"]]) + T * n and int(got["state"][F["calls"]]) == 4
    assert (got["work"].reshape(-1, 3)[:, 2].astype(np.int64).sum()) == T * n


@pytest.mark.parametrize("n,T", [(65, 9), (300, 7)])
def test_in_place_gives_the_same(n, T):
    case = reward_case(T, n, 10 * n + T)
    buf = _Buffers(case, in_place=True)
    buf.run()
    _equal(buf.host(), _ref(case), (n, T))


def test_without_update_the_statistics_are_frozen_and_a_fresh_state_is_the_identity_under_the_clip():
    case = reward_case(9, 130, 1)
    buf = _Buffers(case)
    buf.run(update=False)
    got = buf.host()
    _equal(got, _ref(case, update=0))
    assert _same(got["state"], case["state"]) and _same(got["R"], case["ret_run"])
    assert (got["work"].view(np.float64) == GUARD).all()           # the work buffer is not touched (and may be NULL)
    fresh = reward_case(9, 130, 1, fresh=True)
    buf = _Buffers(fresh)
    buf.run(update=False)
    got = buf.host()
    inside = np.abs(fresh["reward"]) <= CLIP
    assert inside.any() and not inside.all() and not got["state"].any()
    assert _same(got["out"][inside], fresh["reward"][inside]) and _same(got["out"][~inside], np.copysign(CLIP, fresh["reward"][~inside]))
    # ... and a fresh state that IS updated scales its first rollout by that rollout's own deviation
    buf = _Buffers(fresh)
    buf.run()
    got = buf.host()
    _equal(got, _ref(fresh))
    assert int(got["state"][F["count"]]) == 9 * 130 and int(got["state"][F["calls"]]) == 1


def test_the_branches_and_the_clip_edges():
    case = reward_case(9, 65, 2)
    for tag, change, kw in (("gamma 0", {}, dict(gamma=0.0)), ("gamma 1", {}, dict(gamma=1.0)), ("no clip", {}, dict(clip=np.inf)),
                            ("eps 0", {}, dict(eps=0.0)), ("every end", dict(reason=np.full_like(case["reason"], 8)), {}),
                            ("no end", dict(reason=np.zeros_like(case["reason"])), {})):
        c = dict(case, **change)
        buf = _Buffers(c)
        buf.run(**kw)
        got = buf.host()
        _equal(got, _ref(c, **kw), tag)
        if tag == "every end":
            assert _same(got["R"], np.zeros(65))                  # +0.0, the sign bit clear
        if tag == "no clip":
            assert (np.abs(got["out"]) > CLIP).any()
    sd = case["state"].view(np.float64)[F["sd"]]
    edge = CLIP * sd
    case["reward"][0, :8] = [edge * (1 + 2.0 ** -40), edge * (1 - 2.0 ** -40), -edge * (1 + 2.0 ** -40), -edge * (1 - 2.0 ** -40),
                             np.inf, -np.inf, np.nan, -0.0]
    buf = _Buffers(case)
    buf.run(update=False)
    got = buf.host()
    _equal(got, _ref(case, update=0), "edges")
    row = got["out"][0, :8]
    assert row[0] == CLIP and row[2] == -CLIP and 0 < row[1] < CLIP and -CLIP < row[3] < 0 and row[4] == CLIP and row[5] == -CLIP
    assert np.isnan(row[6]) and _same(row[7], np.float64(-0.0))


def test_scaling_everything_by_a_power_of_two_scales_the_deviation_and_nothing_else():
    case = reward_case(9, 300, 3)
    big = dict(case, reward=case["reward"] * 4.0, ret_run=case["ret_run"] * 4.0, state=case["state"].copy())
    big["state"].view(np.float64)[[F["sum"], F["sum_sq"]]] = case["state"].view(np.float64)[[F["sum"], F["sum_sq"]]] * np.array([4.0, 16.0])
    got = []
    for c in (case, big):
        buf = _Buffers(c)
        buf.run(eps=0.0)
        got.append(buf.host())
    assert _same(got[1]["out"], got[0]["out"]) and _same(got[1]["R"], got[0]["R"] * 4.0)
    f0, f1 = got[0]["state"].view(np.float64), got[1]["state"].view(np.float64)
    assert _same(f1[F["sd"]], f0[F["sd"]] * 4.0) and _same(f1[F["var"]], f0[F["var"]] * 16.0) and got[1]["state"][F["count"]] == got[0]["state"][F["count"]]


# ------------------------------------------------------------------------------------------------------------------ the rules
def test_bad_arguments_are_refused_before_any_launch():
    n, T = 5, 3
    case = reward_case(T, n, 40)
    buf = _Buffers(case)
    stride = buf.stride
    lib = _lib.load()
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    f64 = C.c_double
    #       0               1               2  3  4       5           6         7          8  9          10             11            12
    good = [vp(buf.reward), vp(buf.reason), T, n, stride, f64(GAMMA), f64(EPS), f64(CLIP), 1, vp(buf.R), vp(buf.state), vp(buf.work), vp(buf.out), None]
    bads = [(0, None), (1, None), (10, None), (12, None), (9, None), (11, None), (2, 0), (3, 0), (4, n - 1), (2, -1), (3, -1),
            (5, f64(-0.01)), (5, f64(1.01)), (5, f64(np.nan)), (5, f64(np.inf)), (6, f64(-1e-12)), (6, f64(np.inf)), (6, f64(np.nan)),
            (7, f64(0.0)), (7, f64(-1.0)), (7, f64(np.nan)), (7, f64(-np.inf))]
    for at, bad in bads:
        args = list(good)
        args[at] = bad
        assert lib.bsk_reward_norm(*args) == EINVAL, (at, bad)
    args = list(good)                                          # n_steps * stride beyond 2^31 (nothing is read: refused before the launch)
    args[2], args[3], args[4] = 2 ** 15, 2 ** 16, 2 ** 16 + 1
    assert lib.bsk_reward_norm(*args) == EINVAL and b"2^31" in lib.bsk_last_error()
    got = buf.host()                                           # nothing was written
    assert _same(got["state"], case["state"]) and _same(got["R"], case["ret_run"])
    assert (got["work"].view(np.float64) == GUARD).all() and (got["out"] == GUARD).all()
    # without update the running returns and the work buffer are not needed; +inf is a clip
    args = list(good)
    args[8], args[9], args[11], args[7] = 0, None, None, f64(np.inf)
    assert lib.bsk_reward_norm(*args) == 0
    _equal(buf.host(), _ref(case, update=0, clip=np.inf))
    assert lib.bsk_reward_norm(*good) == 0
    _equal(buf.host(), _ref(case))
    # the binding refuses the same with a ValueError, before the library is asked
    for kw in (dict(gamma=1.5), dict(eps=-1.0), dict(clip=0.0), dict(stride=n - 1), dict(ret_run=None), dict(work=None),
               dict(state=buf.state[:7]), dict(work=buf.work[:2]), dict(ret_run=buf.R[:n - 1]), dict(out=buf.out[:T * stride - 1])):
        a = dict(out=buf.out, ret_run=buf.R, work=buf.work, gamma=GAMMA, eps=EPS, clip=CLIP, stride=stride, state=buf.state)
        a.update(kw)
        state = a.pop("state")
        with pytest.raises(ValueError):
            P.reward_normalize(buf.reward, buf.reason, T, n, state, **a)


# ------------------------------------------------------------------------------------------------------------------ a graph
def test_a_graph_captured_with_no_call_before_it_equals_eager_rounds():
    import torch
    n, T, rounds = 300, 9, 3
    case = reward_case(T, n, 50)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        bufs = [_Buffers(case) for _ in range(2)]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        c0 = BatchedPropagator.debug_counters()
        with torch.cuda.graph(graph, stream=side):
            bufs[0].run(stream=side.cuda_stream)
        for _ in range(rounds):
            graph.replay()
        torch.cuda.synchronize()
        assert BatchedPropagator.debug_counters() == c0         # no copy, no synchronisation
        for _ in range(rounds):
            bufs[1].run(stream=side.cuda_stream)
        a, b = bufs[0].host(), bufs[1].host()
        del graph
    for k in ("out", "state", "R", "work"):
        assert _same(a[k], b[k]), k
    # ... and both are the restatement's: the same histories three times over, the statistics and the returns carried through
    c = dict(case)
    for _ in range(rounds):
        want = _ref(c)
        c = dict(c, state=want[1], ret_run=want[2])
    _equal(a, want)
    assert int(a["state"][F["calls"]]) == 3 + rounds and int(a["state"][F["count"]]) == int(case["state"][F["count"]]) + rounds * T * n


# ------------------------------------------------------------------------------------------------------------------ the loop
N_ENVS, N_STEPS, LOOP_GAMMA, LOOP_LAM, LOOP_CLIP = 65, 8, 0.97, 0.9, 2.0
HIST = (("obs", np.float64, 5), ("action", np.int32, 1), ("logp", np.float32, 1), ("value", np.float32, 1), ("reward", np.float64, 1),
        ("reason", np.uint8, 1))
NEW_KEYS = {"reward_norm", "ret_run", "reward_state", "reward_work"}


def _loop(side, spec, params, normalize):
    n, T = N_ENVS, N_STEPS
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_AUTO_RESET
    cfg.max_length = 5                                      # (episodes end, and start again, inside and across the rollouts)
    root = BatchedPropagator(cfg, n, stream=side.cuda_stream)
    root.set_ic_pool(sample_ic_batch(23, 4, seed=73))
    root.reset(sample_ic_batch(n, 4, seed=72))
    root.step(np.zeros(n, np.int32), 1)                     # (the observation buffers hold a step's output)
    steps, ticks = root.get_counters()
    root.set_counters(steps + np.arange(n, dtype=np.int32) % 4, ticks)          # episodes end at different steps
    f = _PG(spec, params, lr=1e-2)
    pg = P.PolicyGradient(root, f.policy, f.fit, T, gamma=LOOP_GAMMA, lam=LOOP_LAM, clip=0.2, ent_coef=0.01, epochs=1, minibatches=2,
                          substeps=1, log_capacity=2, normalize_rewards=normalize, reward_clip=LOOP_CLIP, reward_eps=1e-8)
    f.policy.set_rng(3, 0)
    return root, f, pg


def _histories(root, bufs):
    root.sync()
    T, n = N_STEPS, N_ENVS
    out = {k: _download(bufs[k], dt, T * w * n).reshape((T, n) if w == 1 else (T, w, n)) for k, dt, w in HIST}
    out["last_value"] = _download(bufs["last_value"], np.float32, n)
    out["adv"], out["ret"] = _download(bufs["adv"], np.float32, T * n).reshape(T, n), _download(bufs["ret"], np.float64, T * n).reshape(T, n)
    if "reward_norm" in bufs:
        out["reward_norm"] = _download(bufs["reward_norm"], np.float64, T * n).reshape(T, n)
    return out


def _close(root, f, pg):
    pg.close()
    f.close()
    root.close()


def test_the_loop_scales_its_rewards_on_the_device_end_to_end():
    import torch
    T, n = N_STEPS, N_ENVS
    spec, params = seeded_policy((16,), "relu", (16,), seed=16)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        # the loop without the option: what it always did, and none of the new buffers
        root, f, pg = _loop(side, spec, params, False)
        assert not NEW_KEYS & set(pg.buffers()) and pg.normalize_rewards is False
        for call in (pg.reward_norm_state, pg.reward_scale, lambda: pg.set_reward_norm_state(np.zeros(8, np.uint64), np.zeros(n))):
            with pytest.raises(ValueError):
                call()
        pg.collect()
        plain = _histories(root, pg.buffers())
        want_adv, want_ret = P.gae_ref(plain["reward"], plain["reason"], plain["value"], plain["last_value"], LOOP_GAMMA, LOOP_LAM)
        assert _same(plain["adv"], want_adv) and _same(plain["ret"], want_ret)
        _close(root, f, pg)
        for bad in (dict(reward_clip=0.0), dict(reward_eps=-1.0), dict(reward_clip=np.nan)):
            with pytest.raises(ValueError):
                P.PolicyGradient(None, None, None, T, **bad)

        # with it, from the same seeds
        root, f, pg = _loop(side, spec, params, True)
        bufs = pg.buffers()
        assert NEW_KEYS <= set(bufs) and pg.update_reward_stats is True
        words, R = pg.reward_norm_state()
        assert words.dtype == np.uint64 and not words.any() and not R.any() and pg.reward_scale() == 1.0
        pg.collect()
        first = _histories(root, bufs)
        for k, _, _ in HIST:
            assert _same(first[k], plain[k]), k                    # the rollout is the same, and `reward` keeps the raw rewards
        out, words, R = P.reward_norm_ref(first["reward"], first["reason"], LOOP_GAMMA, 1e-8, LOOP_CLIP, 1)
        assert _same(first["reward_norm"], out)
        want_adv, want_ret = P.gae_ref(out, first["reason"], first["value"], first["last_value"], LOOP_GAMMA, LOOP_LAM)
        assert _same(first["adv"], want_adv) and _same(first["ret"], want_ret)
        assert not _same(first["adv"], plain["adv"]) and (first["reason"] != 0).any()
        got_words, got_R = pg.reward_norm_state()
        assert _same(got_words, words) and _same(got_R, R) and R.any()
        assert pg.reward_scale() == words.view(np.float64)[F["sd"]] and 0.0 < pg.reward_scale() < 1.0        # rewards of order 1e-3
        pg.update()
        root.sync()
        # the log speaks of the RAW rewards
        row, ep_state = P.pg_episodes_ref(first["reward"], first["reason"], first["action"], first["value"], first["ret"])
        its, table = pg.training_log()
        assert list(its) == [0] and _same(table[0, :16], row) and row[0] > 0
        assert _same(table[0, 13], row[13]) and not _same(row[13], np.float64(out.sum()))

        # a second iteration carries the statistics and the running returns
        log = pg.iterate()
        assert log.shape == (2, 8)
        second = _histories(root, bufs)
        out2, words2, R2 = P.reward_norm_ref(second["reward"], second["reason"], LOOP_GAMMA, 1e-8, LOOP_CLIP, 1, words, R)
        assert _same(second["reward_norm"], out2)
        got_words, got_R = pg.reward_norm_state()
        assert _same(got_words, words2) and _same(got_R, R2) and int(words2[F["calls"]]) == 2 and int(words2[F["count"]]) == 2 * T * n
        fresh_out, _, _ = P.reward_norm_ref(second["reward"], second["reason"], LOOP_GAMMA, 1e-8, LOOP_CLIP, 1)
        assert not _same(fresh_out, out2)                          # (what was carried matters)
        row2, _ = P.pg_episodes_ref(second["reward"], second["reason"], second["action"], second["value"], second["ret"], ep_state)
        its, table = pg.training_log()
        assert list(its) == [0, 1] and _same(table[1, :16], row2)
        # frozen statistics: read at enqueue time
        pg.update_reward_stats = False
        pg.collect()
        third = _histories(root, bufs)
        got_words, got_R = pg.reward_norm_state()
        assert _same(got_words, words2) and _same(got_R, R2)
        assert _same(third["reward_norm"], P.reward_norm_ref(third["reward"], third["reason"], LOOP_GAMMA, 1e-8, LOOP_CLIP, 0, words2, R2)[0])
        with pytest.raises(ValueError):
            pg.set_reward_norm_state(words2, R2[:-1])
        _close(root, f, pg)

        # a checkpoint: a second loop from the same seeds, its state lost and put back after the first iteration, goes on bit for bit
        root, f, pg = _loop(side, spec, params, True)
        bufs = pg.buffers()
        pg.iterate()
        pg.set_reward_norm_state(np.zeros(8, np.uint64), np.zeros(n))
        lost_words, lost_R = pg.reward_norm_state()
        assert not lost_words.any() and not lost_R.any() and pg.reward_scale() == 1.0
        pg.set_reward_norm_state(words, R)
        pg.iterate()
        again = _histories(root, bufs)
        for k in ("reward", "reason", "reward_norm", "adv", "ret"):
            assert _same(again[k], second[k]), k
        got_words, got_R = pg.reward_norm_state()
        assert _same(got_words, words2) and _same(got_R, R2)
        _close(root, f, pg)
