"""GPU: bsk_fit_accumulate_ppo beyond one small network - csrc/bsk_fit.hip: fit_block_kernel<true, FitVclip> and
fit_fold_kernel<10, double*> at the shapes the supervised and the policy-gradient instantiations already run at
(tests/test_gpu_fit.py: BIT_CASES; tests/test_gpu_pg.py: PG_BIT_CASES), the two ties of the value loss, strides above n on either
side of all three accumulate forms, and the inputs of a sample that does not contribute.

Everything is an equality of bits against the numpy restatements (basilisk_env_amd/policy_ref.py), as in the files this one
extends: the networks are relu, so the forward pass is ``mlp_ref``'s bit for bit; the value deltas are ``fit_value_delta_ref``'s on
the device's OWN v, read first through d_dvalue of a launch with value_coef = 1 and targets 0; the accumulators A are read as
Adam's first moment after one step with beta1 = 0 and lr = 0, from the device's own output deltas (``_reference_moment``).  The
policy-gradient row goes through the device library's expf and logf and is held to tests/_pg_bounds.py, as in tests/test_gpu_pg.py.
The shapes, the placements and what each is there for: tests/_ppo_cases.py, whose constructions tests/test_ppo_cases_host.py checks
without a device.  The largest launch is 4 400 samples on a 16-wide network.
"""
import ctypes as C

import numpy as np
import pytest

from _device_bits import same as _same
from _fit_bounds import backward_bound
from _pg_bounds import pg_dlogits_bound, pg_stats_bound
from _policy_bounds import seeded_policy
from _ppo_cases import (CV, KINDS, NET_SEED, PPO_CASES, SEED_OF_CALL, TIE_CASES, case_values, cycle_kinds, tie_case_net, tie_place)
from basilisk_env_amd import _lib
from basilisk_env_amd import policy as P
from test_gpu_fit import _dev, _reference_moment
from test_gpu_pg import _PG, _block_sum, pg_case
from test_gpu_pg_shuffle import NAMES, _histories, _outputs, _state

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
GUARD = 3                                      # words behind d_dvalue that nobody may write
ZERO = dict(lr=0.0, beta1=0.0, weight_decay=0.0)          # m after one step is A / count, and theta stays


def _inputs(f, n, seed):
    """``pg_case``'s masked batch: two actions out of range, two dead alive bytes -> a dict of host arrays"""
    obs, actions, alive, _, adv, old, logits = pg_case(f, n, seed)
    on = (actions >= 0) & (actions <= 2) & (alive != 0)
    assert n <= 8 or (~on).sum() == 4
    return dict(obs=obs, actions=actions, alive=alive, adv=adv, old=old, logits=logits, on=on, n=n)


def _upload(x, vo=None, R=None):
    d = {k: _dev(x[k]) for k in ("obs", "actions", "alive", "adv", "old")}
    d["vo"], d["R"] = None if vo is None else _dev(vo), None if R is None else _dev(R)
    return d


def _buffers(n):
    import torch
    return (torch.full((3, n), SENTINEL, dtype=torch.float32, device="cuda"),
            torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda"))


def _ppo(f, d, n, with_old=True, with_dvalue=True):
    """one accumulate_ppo on uploaded arrays -> (dlogits (3, n), dvalue (n + GUARD,) with its guard words) on the host"""
    import torch
    dl, dv = _buffers(n)
    torch.cuda.synchronize()
    f.fit.accumulate_ppo(d["obs"], d["actions"], d["adv"], d["old"], 0.2, 0.01, d["R"], d["vo"] if with_old else None, CV if with_old else None,
                         d["alive"], dl, dv[:n] if with_dvalue else None)
    torch.cuda.synchronize()
    return dl.cpu().numpy(), dv.cpu().numpy()


def _device_values(reader, x, ref=None):
    """the device's own v of every contributing sample: value_coef = 1, targets 0, no old values - delta = 1.0f * (v - 0.0f).  The
    four masked samples get +0.0f from the launch; their v, which nothing reads, is filled in from ``ref``."""
    n = x["n"]
    _, dv = _ppo(reader, _upload(x, None, np.zeros(n)), n, with_old=False)
    v, on = dv[:n].copy(), x["on"]
    assert (dv[n:] == SENTINEL).all() and _same(v[~on], np.zeros(int((~on).sum()), np.float32))
    if ref is not None:
        assert _same(v[on], ref[on])                           # a relu network: the restatement's bits
        v[~on] = ref[~on]
    return v


def _rows(f):
    row, pg, vc = f.fit.stats(), f.fit.pg_stats(), f.fit.vclip_stats()
    return np.array([row[k] for k in P.FIT_STATS_COLUMNS] + [pg[k] for k in P.PG_STATS_COLUMNS] + [vc[k] for k in P.VCLIP_STATS_COLUMNS],
                    np.float64)


def _check_call(f, x, v, vo, R, dl, dv, relu=True, where=None):
    """what one accumulate_ppo with old values wrote: d_dvalue and the three rows against the restatement on the device's own v"""
    n, on = x["n"], x["on"]
    delta, term, clipped = P.fit_value_delta_ref(v, R, vo, CV, f.fit.value_coef)
    plain = P.fit_value_delta_ref(v, R, None, None, f.fit.value_coef)[1]
    assert _same(dv[:n][on], delta[on]), where
    assert _same(dv[:n][~on], np.zeros(int((~on).sum()), np.float32)) and (dv[n:] == SENTINEL).all(), where      # +0.0f; the guards stay
    assert _same(dl[:, ~on], np.zeros((3, int((~on).sum())), np.float32)), where
    row, pg, vrow = f.fit.stats(), f.fit.pg_stats(), f.fit.vclip_stats()
    assert row["count"] == on.sum() == n - (4 if n > 8 else 0), where
    assert _same(np.float64(row["value_loss_sum"]), np.float64(_block_sum(np.where(on, term, 0.0)))), where
    assert vrow["value_clipped"] == int((clipped & on).sum()), where
    assert _same(np.float64(vrow["value_loss_unclipped_sum"]), np.float64(_block_sum(np.where(on, plain, 0.0)))), where
    if relu:
        ref = P.fit_stats_ref(f.spec, f.params, x["obs"], x["actions"], x["alive"])
        assert row["correct"] == ref[2] and row["count"] == ref[3], where
    # the policy-gradient row: counts equal, sums within the summed per-sample bounds (tests/test_gpu_pg.py's rule)
    b = pg_dlogits_bound(x["logits"], x["actions"], x["adv"], x["old"], 0.2, 0.01, on)
    want, tol = pg_stats_bound(b, on)
    free = int((b["band"] & on).sum())
    assert free * 100 <= n and want[2] <= pg["clipped"] <= want[2] + free, where
    if free == 0:
        got = np.array([pg["kl_sum"], pg["entropy_sum"], pg["clipped"], pg["surrogate_sum"]])
        assert (np.abs(got - want) <= tol).all(), (where, got, want, tol)
    return clipped


# ------------------------------------------------------------------------------------------------------------------ A. the case table
@pytest.mark.parametrize("case", list(PPO_CASES))
def test_ppo_backward_and_accumulators_equal_the_restatement_bit_for_bit(case):
    hidden, vh, sizes = PPO_CASES[case]
    spec, params = seeded_policy(hidden, "relu", vh, seed=NET_SEED)
    f, reader = _PG(spec, params, value_coef=0.5, **ZERO), _PG(spec, params, value_coef=1.0)
    calls = []
    for k, n in enumerate(sizes):
        x = _inputs(f, n, SEED_OF_CALL + k)
        assert _same(x["logits"], P.mlp_ref(spec, params, x["obs"])[0])
        v = _device_values(reader, x, P.mlp_ref(spec, params, x["obs"])[1].reshape(-1))
        vo, R = case_values(v, wide=case == "ppo_fold33_wide")
        dl, dv = _ppo(f, _upload(x, vo, R), n)
        clipped = _check_call(f, x, v, vo, R, dl, dv, where=(case, k))
        kinds = np.array(cycle_kinds(n))[x["on"]]
        assert set(kinds) == set(KINDS) and clipped[x["on"]].sum() >= n // 5       # all five branches among the contributing samples
        calls.append((x["obs"], x["actions"], x["alive"], R, dl, dv[:n]))
    f.fit.step()
    st = f.fit.state()
    want, count = _reference_moment(spec, params, calls, 0.5)
    assert count == sum(sizes) - 4 * len(sizes) and st["steps"] == 1
    assert np.count_nonzero(want) > want.size // 10 and not want[:10].any()
    assert _same(st["m"], want)
    assert _same(st["theta"], params.astype(np.float64))             # lr = 0: nothing moved
    f.close()
    reader.close()


def test_the_ten_column_fold_without_a_value_clip_row_is_accumulate_pgs():
    """``ppo_fold33`` a second time with d_dvalue alone: fit_fold_kernel<10, double*> with a NULL vclip_row at 33 blocks.  A and the
    first two rows are accumulate_pg's on a twin, and the value-clip row keeps what the launch before left in it."""
    hidden, vh, (n,) = PPO_CASES["ppo_fold33"]
    spec, params = seeded_policy(hidden, "relu", vh, seed=NET_SEED)
    f, twin = _PG(spec, params, value_coef=0.5, **ZERO), _PG(spec, params, value_coef=0.5, **ZERO)
    x = _inputs(f, n, SEED_OF_CALL)
    v = P.mlp_ref(spec, params, x["obs"])[1].reshape(-1)
    vo, R = case_values(v)
    d = _upload(x, vo, R)
    _ppo(f, d, n)                                                    # (with old values: the value-clip row is written)
    held = f.fit.vclip_stats()
    assert held["value_clipped"] > n // 5 and held["value_loss_unclipped_sum"] > 0
    f.fit.step()
    dl, dv = _ppo(f, d, n, with_old=False)
    dl_twin = twin.accumulate_pg(x["obs"], x["actions"], x["adv"], x["old"], 0.2, 0.01, x["alive"], R)
    assert _same(dl, dl_twin) and _same(_rows(f)[:8], _rows(twin)[:8])
    assert f.fit.vclip_stats() == held and twin.fit.vclip_stats() == dict(zip(P.VCLIP_STATS_COLUMNS, (0, 0.0)))
    assert _same(dv[:n], np.where(x["on"], P.fit_value_delta_ref(v, R, None, None, 0.5)[0], np.float32(0.0))) and (dv[n:] == SENTINEL).all()
    for g in (f, twin):
        g.fit.step()
    a, b = f.fit.state(), twin.fit.state()
    assert _same(a["m"], b["m"]) and np.count_nonzero(a["m"]) > a["m"].size // 10 and (a["steps"], b["steps"]) == (2, 1)
    f.close()
    twin.close()


@pytest.mark.parametrize("activation,value_activation", [("tanh", "relu"), ("relu", "tanh")])
def test_each_network_of_a_ppo_launch_runs_its_own_activation(activation, value_activation):
    """tests/test_gpu_fit.py's test_each_network_of_a_fit_runs_its_own_activation by its own method, through accumulate_ppo with old
    values at n = 65: the relu network's slice of A is the restatement's bit for bit whichever of the two it is; a tanh action
    network lies within ``backward_bound``; a tanh value network is asked to be finite and NOT what the relu / relu restatement of
    the same floats gives."""
    n, value_coef = 65, 0.5
    spec, params = seeded_policy((32, 16), activation, (48,), seed=19, value_activation=value_activation)
    relu_relu = P.check_spec((32, 16), "relu", (48,), "relu")
    a_end = 10 + sum(o * i + o for o, i in P.layer_shapes(spec)[0])
    f, reader = _PG(spec, params, value_coef=value_coef, **ZERO), _PG(spec, params, value_coef=1.0)
    x = _inputs(f, n, 33)
    ref = P.mlp_ref(spec, params, x["obs"])[1].reshape(-1)
    v = _device_values(reader, x, ref if value_activation == "relu" else None)
    vo, R = case_values(v)
    dl, dv = _ppo(f, _upload(x, vo, R), n)
    _check_call(f, x, v, vo, R, dl, dv, relu=activation == "relu")
    row = f.fit.stats()
    f.fit.step()
    st = f.fit.state()
    m = st["m"]
    calls = [(x["obs"], x["actions"], x["alive"], R, dl, dv[:n])]
    want, count = _reference_moment(spec, params, calls, value_coef)
    plain, _ = _reference_moment(relu_relu, params, calls, value_coef)
    swapped, _ = _reference_moment(P.check_spec((32, 16), value_activation, (48,), activation), params, calls, value_coef)
    assert row["count"] == count == n - 4 and st["steps"] == 1 and not m[:10].any() and 10 < a_end < m.size
    for lo, hi in ((10, a_end), (a_end, m.size)):
        assert np.count_nonzero(want[lo:hi]) > (hi - lo) // 10 and not _same(want[lo:hi], swapped[lo:hi])
    if activation == "relu":
        assert _same(m[10:a_end], want[10:a_end])
        assert np.isfinite(m[a_end:]).all() and np.count_nonzero(m[a_end:]) > (m.size - a_end) // 10
        assert not _same(m[a_end:], plain[a_end:])
    else:
        assert _same(m[a_end:], want[a_end:])
        G64, bound = backward_bound(spec, params, x["obs"], dl)
        G64, bound = G64.sum(axis=0)[10:a_end], bound.sum(axis=0)[10:a_end]
        # (m * count is A up to the division's and the product's rounding: 2**-52 of |A| covers both)
        err, tol = np.abs(m[10:a_end] * count - G64), bound * (1.0 + 2.0 ** -20) + 2.0 ** -52 * np.abs(G64)
        print("tanh (32, 16) over a relu value network, ppo: max |A - fp64| %.3e, max bound %.3e, max ratio %.3f"
              % (err.max(), tol.max(), (err / np.maximum(tol, 1e-300)).max()))
        assert (err <= tol).all()
    assert _same(st["theta"], params.astype(np.float64))             # lr = 0: nothing moved
    f.close()
    reader.close()


# ------------------------------------------------------------------------------------------------------------------ B. the ties
@pytest.mark.parametrize("hidden,vh,n,seed", TIE_CASES)
def test_both_ties_of_the_value_loss_are_the_unclipped_branchs(hidden, vh, n, seed):
    """-cv <= dv && dv <= cv at equality, and d2 d2 == d d outside the range (tests/_ppo_cases.py: ``tie_place``), built exactly in
    f32 from the device's own v.  At least three samples in four of each kind are true ties - a condition on the construction, not a
    tolerance - and none of them may be counted as value-clipped."""
    spec, params = tie_case_net(hidden, vh, seed)
    f, reader = _PG(spec, params, value_coef=0.5, **ZERO), _PG(spec, params, value_coef=1.0)
    x = _inputs(f, n, seed)
    on = x["on"]
    v = _device_values(reader, x, P.mlp_ref(spec, params, x["obs"])[1].reshape(-1))
    vo, R, edge, peak, visible = tie_place(v)
    even = np.arange(n) % 2 == 0
    print("n %d: edge ties %d of %d (visible %d), max ties %d of %d" % (n, (edge & on).sum(), (even & on).sum(), (visible & on).sum(),
                                                                         (peak & on).sum(), (~even & on).sum()))
    assert 4 * (edge & on).sum() >= 3 * (even & on).sum() and 4 * (peak & on).sum() >= 3 * (~even & on).sum()
    assert (visible & on & (v > 0)).any() and (visible & on & (v < 0)).any()
    dl, dv = _ppo(f, _upload(x, vo, R), n)
    clipped = _check_call(f, x, v, vo, R, dl, dv, where=(hidden, vh, n))
    ties = (edge | peak) & on
    assert not clipped[ties].any()
    # directly: the row counts the samples that were placed clipped and no tie; every max tie carries its unclipped delta
    assert f.fit.vclip_stats()["value_clipped"] == int((clipped & on & ~ties).sum()) == int((clipped & on).sum())
    d = (v - R.astype(np.float32)).astype(np.float32)
    assert _same(dv[:n][peak & on], (np.float32(0.5) * d)[peak & on]) and (dv[:n][peak & on] != 0).all()
    f.fit.step()
    st = f.fit.state()
    want, count = _reference_moment(spec, params, [(x["obs"], x["actions"], x["alive"], R, dl, dv[:n])], 0.5)
    assert count == n - 4 and _same(st["m"], want) and np.count_nonzero(want) > want.size // 10
    f.close()
    reader.close()


# ------------------------------------------------------------------------------------------------------------------ C. strides
FORMS = ("accumulate", "accumulate_pg", "accumulate_ppo")


def _dense(form, f, d, dl, dv=None):
    """one accumulate of the given form through the binding, everything dense"""
    if form == "accumulate":
        f.fit.accumulate(d["obs"], d["actions"], d["R"], d["alive"], dl)
    elif form == "accumulate_pg":
        f.fit.accumulate_pg(d["obs"], d["actions"], d["adv"], d["old"], 0.2, 0.01, d["R"], d["alive"], dl)
    else:
        f.fit.accumulate_ppo(d["obs"], d["actions"], d["adv"], d["old"], 0.2, 0.01, d["R"], d["vo"], CV, d["alive"], dl, dv)


def _strided(form, f, d, obs, obs_stride, n, dl, out_stride, dv=None):
    """the same through the C ABI, which alone takes out_stride apart from obs_stride"""
    lib, h = _lib.load(), f.fit._handle()
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    if form == "accumulate":
        rc = lib.bsk_fit_accumulate(h, vp(obs), obs_stride, n, vp(d["actions"]), vp(d["R"]), vp(d["alive"]), vp(dl), out_stride, None)
    elif form == "accumulate_pg":
        rc = lib.bsk_fit_accumulate_pg(h, vp(obs), obs_stride, n, vp(d["actions"]), vp(d["adv"]), vp(d["old"]), 0.2, 0.01, vp(d["R"]),
                                       vp(d["alive"]), vp(dl), out_stride, None)
    else:
        rc = lib.bsk_fit_accumulate_ppo(h, vp(obs), obs_stride, n, vp(d["actions"]), vp(d["adv"]), vp(d["old"]), 0.2, 0.01, vp(d["R"]),
                                        vp(d["vo"]), CV, vp(d["alive"]), vp(dl), out_stride, vp(dv), None)
    assert rc == 0, lib.bsk_last_error()


@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("form", FORMS)
def test_strides_above_n_on_either_side_change_nothing(form, n):
    """obs a view of a [5][n + 3] block whose padding columns are NaN (policy_logp_kernel in front of the policy-gradient launches
    takes the same stride), dlogits a [3][n + 5] block filled with a sentinel: rows, A and the deltas are the dense call's on a twin,
    and neither padding is touched."""
    import torch
    spec, params = seeded_policy((16,), "relu", (16,), seed=NET_SEED)
    f, twin = _PG(spec, params, value_coef=0.5, **ZERO), _PG(spec, params, value_coef=0.5, **ZERO)
    x = _inputs(f, n, 70 + n)
    vo, R = case_values(P.mlp_ref(spec, params, x["obs"])[1].reshape(-1))
    d = _upload(x, vo, R)
    block = np.full((5, n + 3), np.nan)
    block[:, :n] = x["obs"]
    d_block = _dev(block)
    wide = torch.full((3, n + 5), SENTINEL, dtype=torch.float32, device="cuda")
    dl, dv = _buffers(n)
    dv_twin = torch.full_like(dv, SENTINEL)
    torch.cuda.synchronize()
    _strided(form, f, d, d_block, n + 3, n, wide, n + 5, dv if form == "accumulate_ppo" else None)
    _dense(form, twin, d, dl, dv_twin[:n] if form == "accumulate_ppo" else None)
    torch.cuda.synchronize()
    got, want = wide.cpu().numpy(), dl.cpu().numpy()
    assert _same(got[:, :n], want) and (got[:, n:] == SENTINEL).all() and np.count_nonzero(want) == 3 * (n - 4)
    assert _same(d_block.cpu().numpy(), block)                       # read only, NaN padding included
    assert _same(dv.cpu().numpy(), dv_twin.cpu().numpy()) and (dv.cpu().numpy()[n:] == SENTINEL).all()
    assert _same(_rows(f), _rows(twin)) and f.fit.stats()["count"] == n - 4 and np.isfinite(_rows(f)).all()
    for g in (f, twin):
        g.fit.step()
    a, b = f.fit.state(), twin.fit.state()
    assert _same(a["m"], b["m"]) and np.isfinite(a["m"]).all() and np.count_nonzero(a["m"]) > a["m"].size // 10
    f.close()
    twin.close()


def test_a_chunk_of_the_gathers_output_is_accumulate_ppos_d_obs_as_it_is():
    """include/bskgpu.h, bsk_pg_gather, at its word: a (T, n, stride) = (2, 70, 96) history gathered into [5][out_stride = m + 3],
    and two chunks of it - offsets 0 and 64, 64 and 76 samples - handed straight to accumulate_ppo with obs_stride = m + 3.  The state
    after the step is the one built from dense host copies of the same chunks."""
    import torch
    T, n, stride, seed, epoch = 2, 70, 96, 5, 3
    m = T * n
    padded, plain = _histories(T, n, stride, 6)
    spec, params = seeded_policy((16,), "relu", (16,), seed=NET_SEED)
    kw = dict(lr=1e-2, weight_decay=1e-3, value_coef=0.5)
    f, twin = _PG(spec, params, **kw), _PG(spec, params, **kw)
    d_hist = {k: _dev(a) for k, a in padded.items()}
    out = _outputs(m)
    torch.cuda.synchronize()
    P.pg_gather(_state(seed, epoch), T, n, 0, m, d_hist["obs"], d_hist["action"], d_hist["adv"], d_hist["logp"], d_hist["ret"], d_hist["value"],
                out["obs"], out["action"], out["adv"], out["logp"], out["ret"], out["value"], out["index"], stride=stride, out_stride=m + 3)
    torch.cuda.synchronize()
    want = P.pg_gather_ref((seed, epoch), n, 0, m, **plain)
    assert all(_same(out[k].cpu().numpy()[..., :m], want[k]) for k in NAMES)
    for lo, size in ((0, 64), (64, 76)):
        cut = slice(lo, lo + size)
        view = out["obs"][:, cut]
        assert view.stride() == (m + 3, 1)
        f.fit.accumulate_ppo(view, out["action"][cut], out["adv"][cut], out["logp"][cut], 0.2, 0.01, out["ret"][cut], out["value"][cut], CV)
        host = {k: _dev(np.ascontiguousarray(want[k][..., cut])) for k in NAMES}
        torch.cuda.synchronize()
        twin.fit.accumulate_ppo(host["obs"], host["action"], host["adv"], host["logp"], 0.2, 0.01, host["ret"], host["value"], CV)
        assert _same(_rows(f), _rows(twin)) and f.fit.stats()["count"] == size
    for g in (f, twin):
        g.fit.step()
    a, b = f.fit.state(), twin.fit.state()
    assert all(_same(a[k], b[k]) for k in ("theta", "m", "v", "beta_pow")) and a["steps"] == b["steps"] == 1
    assert not np.array_equal(a["theta"][10:], params[10:].astype(np.float64))
    assert (out["obs"].cpu().numpy()[:, m:] == -7).all()             # the padding columns of the gather's output stay
    f.close()
    twin.close()


# ------------------------------------------------------------------------------------------------------------------ D. what is not read
@pytest.mark.parametrize("form", FORMS)
def test_the_inputs_of_a_sample_that_does_not_contribute_are_not_read(form):
    """The same batch twice on twin fits, the second time with NaN in adv, logp_old, value_target and value_old at the four masked
    samples (the loop relies on it: an env past its first episode keeps stale history words).  The observations stay finite - the
    forward pass runs for every lane below n, and a NaN activation times a zero delta is NaN by definition."""
    import torch
    n = 130
    spec, params = seeded_policy((16,), "relu", (16,), seed=NET_SEED)
    fits = [_PG(spec, params, value_coef=0.5, **ZERO) for _ in range(2)]
    x = _inputs(fits[0], n, 90)
    off = ~x["on"]
    vo, R = case_values(P.mlp_ref(spec, params, x["obs"])[1].reshape(-1))
    results = []
    for f, poison in zip(fits, (False, True)):
        y = dict(x)
        if poison:
            y["adv"], y["old"], vo_, R_ = x["adv"].copy(), x["old"].copy(), vo.copy(), R.copy()
            for a in (y["adv"], y["old"], vo_, R_):
                a[off] = np.nan
                assert np.isnan(a).sum() == 4
        else:
            vo_, R_ = vo, R
        dl, dv = _buffers(n)
        torch.cuda.synchronize()
        _dense(form, f, _upload(y, vo_, R_), dl, dv[:n] if form == "accumulate_ppo" else None)
        torch.cuda.synchronize()
        rows = _rows(f)
        f.fit.step()
        results.append((rows, dl.cpu().numpy(), dv.cpu().numpy(), f.fit.state()["m"]))
    for a, b in zip(*results):
        assert _same(a, b) and np.isfinite(a).all()
    rows, dl, dv, m = results[0]
    assert rows[3] == n - 4 and np.count_nonzero(dl) == 3 * (n - 4) and np.count_nonzero(m) > m.size // 10
    assert (dv == SENTINEL).all() != (form == "accumulate_ppo")
    for f in fits:
        f.close()


# ------------------------------------------------------------------------------------------------------------------ E. three forms, one A
def test_a_supervised_a_pg_and_a_ppo_accumulate_add_into_one_accumulator():
    """tests/test_gpu_pg.py's test_a_supervised_and_a_pg_accumulate_add_into_one_accumulator with value targets and a third call:
    100 supervised samples, 70 policy-gradient ones and 65 with old values go into one A, read against ``_reference_moment`` with the
    value deltas of each call - the squared error's for the first two, the device's own d_dvalue for the third."""
    from test_gpu_fit import _batch
    spec, params = seeded_policy((16,), "relu", (16,), seed=NET_SEED)
    f = _PG(spec, params, value_coef=0.5, **ZERO)
    obs, labels, alive, targets = _batch(100, 25)
    calls = [(obs, labels, alive, targets, f.accumulate(obs, labels, alive, targets))]
    obs, actions, alive, targets, adv, old, _ = pg_case(f, 70, 26)
    calls.append((obs, actions, alive, targets, f.accumulate_pg(obs, actions, adv, old, 0.2, 0.01, alive, targets)))
    x = _inputs(f, 65, 27)
    v = P.mlp_ref(spec, params, x["obs"])[1].reshape(-1)
    vo, R = case_values(v)
    dl, dv = _ppo(f, _upload(x, vo, R), 65)
    _check_call(f, x, v, vo, R, dl, dv)
    calls.append((x["obs"], x["actions"], x["alive"], R, dl, dv[:65]))
    f.fit.step()
    st = f.fit.state()
    want, count = _reference_moment(spec, params, calls, 0.5)
    assert count == 96 + 66 + 61 and st["steps"] == 1 and _same(st["m"], want) and np.count_nonzero(want) > want.size // 10
    # (each call moved A: the step of any two of them is another)
    assert not _same(want, _reference_moment(spec, params, calls[:2], 0.5)[0])
    f.close()
