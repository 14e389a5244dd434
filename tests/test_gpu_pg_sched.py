"""GPU: schedules of lr, clip, clip_vf and ent_coef and a KL stop per update, carried in device words of the fit -
bsk_fit_set_schedule, bsk_fit_schedule_begin, bsk_fit_kl_gate, bsk_fit_schedule_end (csrc/bsk_pgsched.hip, the scheduled
instantiations of fit_block_kernel and fit_adam_kernel in csrc/bsk_fit.hip; definition in include/bskgpu.h) and
``policy.PolicyGradient(total_iterations=, lr_end=, clip_end=, kl_stop=)``.

Everything here is an equality of bits between a scheduled fit and a twin whose HOST does what the words do: a scheduled launch
rounds the words as the host rounds the arguments, so it is the unscheduled launch called with the words' values.  The rule and
the gate themselves are ``pg_schedule_ref`` and ``fit_kl_gate_ref`` (held to the device's own text on the host by
tests/test_pg_sched_host.py before this file runs it).  A scheduled fit is always CALLED with other, valid scalars than the words
hold: they are validated and not read.  Shapes: 130 samples are two full blocks of 64 and one of 2, some samples masked out; a
one-hidden-layer and a two-hidden-layer network; two accumulates per step.

The graph test captures ONE iteration and replays it three times: on a fit without the words a replay trains at the captured
constants for ever."""
import ctypes as C

import numpy as np
import pytest

from _device_bits import download as _download, same as _same
from _pg_sched_cases import CLIP, CLIP_VF, ENT, LR
from _policy_bounds import seeded_policy
from basilisk_env_amd import _hip, _lib
from basilisk_env_amd import policy as P
from basilisk_env_amd._lib import FLAG_AUTO_RESET, GRAV_PM_J2
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
from test_gpu_fit import _batch, _dev, _host
from test_gpu_pg import _PG, _lp_of

pytestmark = pytest.mark.gpu

EINVAL = -1
N = 130
NETS = {"one": ((16,), "relu", (16,)), "two": ((32, 16), "relu", (16,))}
OTHER = (0.5, 0.5, 7.0)                    # clip, ent_coef, clip_vf a scheduled fit is called with: valid, and not the words' values
PAIRS = (LR, CLIP, CLIP_VF, ENT)


def _batches(f, count, seed, shifts=None):
    """``count`` synthetic PPO batches of N samples on the device: ``test_gpu_fit._batch``'s observations, actions (two out of range)
    and alive bytes (two zero), advantages N(0, 1), old values N(0, 1) and old log-probabilities - the policy's own, from the
    device's logits, plus N(0, 0.3^2) noise or, with ``shifts``, plus that batch's constant"""
    out = []
    for k in range(count):
        obs, actions, alive, targets = _batch(N, seed + k)
        rng = np.random.default_rng(8000 + seed + k)
        lp = _lp_of(f.logits(obs), actions)
        old = lp + (rng.normal(0.0, 0.3, N) if shifts is None else shifts[k])
        host = dict(obs=obs, actions=actions, alive=alive, targets=targets, adv=rng.normal(size=N).astype(np.float32),
                    old=old.astype(np.float32), vold=rng.normal(size=N).astype(np.float32))
        out.append({name: _dev(a) for name, a in host.items()})
    return out


class _Run(object):
    """a policy with a fit, a ``log`` of diagnostics rows [rows][8] in the loop's layout and a ring for the schedule's rows"""

    def __init__(self, spec, params, max_grad_norm=0.0, ring=0):
        import torch
        self.f = _PG(spec, params, lr=LR[0])
        self.fit = self.f.fit
        if max_grad_norm:
            self.fit.max_grad_norm = max_grad_norm
        self.log = torch.zeros((8, 8), dtype=torch.float64, device="cuda")
        self.cap = ring
        self.ring = torch.full((ring, 8), -1, dtype=torch.int64, device="cuda").view(torch.float64) if ring else None          # all ones
        self.rows = (self.fit.pg_stats_ptr(), self.fit.stats_ptr())

    def warm(self, b):
        """the fit's scratch, by an accumulate in which no sample is alive: +0.0 into every accumulator, nothing into the count"""
        import torch
        dead = torch.zeros(N, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.fit.accumulate_ppo(b["obs"], b["actions"], b["adv"], b["old"], 0.2, 0.0, b["targets"], b["vold"], 0.2, dead)
        torch.cuda.synchronize()

    def accumulate(self, b, values, vold, r, stream=0):
        """one accumulate_ppo - with the old values the value-clip form of the block kernel, without them the plain PG form - and
        its two diagnostics rows into row ``r`` of the log, device to device"""
        clip, ent, cv = values
        self.fit.accumulate_ppo(b["obs"], b["actions"], b["adv"], b["old"], clip, ent, b["targets"], b["vold"] if vold else None,
                                cv if vold else None, b["alive"], stream=stream)
        for k, row in enumerate(self.rows):
            _hip.check(_hip.runtime().hipMemcpyAsync(C.c_void_p(self.log.data_ptr() + 64 * r + 32 * k), C.c_void_p(row), 32,
                                                     _hip.hipMemcpyDeviceToDevice, C.c_void_p(int(stream))), "hipMemcpyAsync")

    def iteration(self, batches, vold, values=None, gate=False, before_step=None, stream=0):
        """begin / per minibatch two accumulates (+ the gate) + step / end when ``values`` is None (a scheduled fit); the same
        accumulates and steps with ``values`` = (clip, ent_coef, clip_vf) as arguments otherwise"""
        sched = values is None
        if sched:
            self.fit.schedule_begin(stream)
        for g in range(len(batches) // 2):
            for c in range(2):
                self.accumulate(batches[2 * g + c], OTHER if sched else values, vold, 2 * g + c, stream)
            if gate:
                self.fit.kl_gate(self.log.data_ptr() + 64 * 2 * g, 2, stream)
            if before_step:
                before_step(g)
            self.fit.step(stream)
        if sched:
            self.fit.schedule_end(self.ring, self.cap, stream)

    def log_rows(self, g):
        import torch
        torch.cuda.synchronize()
        return self.log.cpu().numpy()[2 * g:2 * g + 2].copy()

    def snap(self, b):
        """theta, m, v, beta_pow, steps, the three diagnostics rows, the clip's row and the policy's device parameters as its own
        logits and values of a batch show them"""
        import torch
        torch.cuda.synchronize()
        st = self.fit.state()
        out = [st[k] for k in ("theta", "m", "v", "beta_pow")] + [np.array([st["steps"]], np.uint64)]
        out += [self.fit._row(self.fit.stats_ptr()), self.fit._row(self.fit.pg_stats_ptr()), self.fit._row(self.fit.vclip_stats_ptr(), 2),
                self.fit._row(self.fit.grad_norm_ptr(), 2)]
        res = self.f.policy.act(b["obs"], want=("logits", "value"))
        torch.cuda.synchronize()
        return out + [_host(res["logits"]), _host(res["value"])]

    def close(self):
        self.f.close()


NAMES = ("theta", "m", "v", "beta_pow", "steps", "fit row", "pg row", "vclip row", "gnorm row", "logits", "value")


def _equal(a, b, tag=None, rows=True):
    """``rows`` False: all but the three diagnostics rows, which a host-driven twin's ``set_state()`` zeroes and the gate leaves"""
    for name, x, y in zip(NAMES, a, b):
        assert _same(x, y) or (not rows and name.endswith(" row") and name != "gnorm row"), (tag, name)


def _values(it, total=4):
    """-> (lr, (clip, ent_coef, clip_vf)) of iteration ``it`` as Python floats: what a host would set and pass"""
    lr, clip, cv, ent = (float(P.pg_schedule_ref(it, total, *pair)) for pair in PAIRS)
    return lr, (clip, ent, cv)


def _words(fit):
    w = fit.schedule_words()
    return w, w.view(np.float64)


# ------------------------------------------------------------------------------------------------------------------ a constant schedule
@pytest.mark.parametrize("max_grad_norm", [0.0, 0.5])
@pytest.mark.parametrize("net", sorted(NETS))
def test_a_constant_schedule_is_invisible(net, max_grad_norm):
    spec, params = seeded_policy(*NETS[net], seed=31)
    plain, sched = (_Run(spec, params, max_grad_norm) for _ in range(2))
    batches = _batches(plain.f, 4, 100)
    values = (CLIP[0], ENT[0], CLIP_VF[0])
    sched.fit.set_schedule(0, (LR[0], LR[0]), (CLIP[0], CLIP[0]), (CLIP_VF[0], CLIP_VF[0]), (ENT[0], ENT[0]))
    assert sched.fit.schedule == (0, (LR[0], LR[0]), (CLIP[0], CLIP[0]), (CLIP_VF[0], CLIP_VF[0]), (ENT[0], ENT[0]), 0.0)
    sched.fit.lr = 0.5                                         # (not read while the schedule is attached)
    for step in range(3):
        for c in range(2):
            b = batches[(2 * step + c) % 4]
            plain.accumulate(b, values, True, c)
            sched.accumulate(b, OTHER, True, c)
        plain.fit.step()
        sched.fit.step()
        _equal(plain.snap(batches[0]), sched.snap(batches[0]), step)
    st = plain.fit.state()
    assert st["steps"] == 3 and not np.array_equal(st["theta"][10:], params[10:].astype(np.float64))
    assert plain.fit.vclip_stats()["value_clipped"] > 0 and plain.fit.pg_stats()["clipped"] > 0        # (both clips are met)
    # the words never moved: nobody called begin or end, and the values are iteration 0's
    w, f = _words(sched.fit)
    assert _same(w, P.sched_words_ref(0, 0, (LR[0],) * 2, (CLIP[0],) * 2, (CLIP_VF[0],) * 2, (ENT[0],) * 2))
    got = sched.fit.schedule_state()
    assert got["lr"] == LR[0] and got["clip"] == CLIP[0] and got["iteration"] == 0 and got["gate"] == 0
    # detached, the fit reads its arguments and its own lr again
    sched.fit.clear_schedule()
    sched.fit.lr = LR[0]
    assert sched.fit.schedule is None
    for r in (plain, sched):
        r.accumulate(batches[1], values, True, 0)
        r.fit.step()
    _equal(plain.snap(batches[0]), sched.snap(batches[0]), "detached")
    plain.close()
    sched.close()


# ------------------------------------------------------------------------------------------------------------------ an annealed one
@pytest.mark.parametrize("net,vold,max_grad_norm", [("one", True, 0.5), ("one", False, 0.0), ("two", True, 0.0), ("two", False, 0.5)])
def test_an_annealed_schedule_equals_the_host_setting_the_values(net, vold, max_grad_norm):
    spec, params = seeded_policy(*NETS[net], seed=32)
    host, sched = (_Run(spec, params, max_grad_norm, ring) for ring in (0, 3))
    batches = _batches(host.f, 4, 200)
    sched.fit.set_schedule(4, *PAIRS)
    for it in range(5):
        lr, values = _values(it)
        host.fit.lr = lr
        host.iteration(batches, vold, values)
        sched.iteration(batches, vold)
        _equal(host.snap(batches[0]), sched.snap(batches[0]), it)
        w, f = _words(sched.fit)
        assert _same(w, np.r_[P.sched_words_ref(it, 4, *PAIRS)[:4], np.array([it + 1, 0, 0, 0], np.uint64)]), (it, w)
        assert _same(f[:4], np.array([lr, values[0], values[2], values[1]]))
    assert (lr, values) == (LR[1], (CLIP[1], ENT[1], CLIP_VF[1])) and CLIP[0] + (CLIP[1] - CLIP[0]) != CLIP[1]         # exactly the ends
    assert host.fit.state()["steps"] == 10
    # the ring of three holds iterations 2, 3, 4
    import torch
    torch.cuda.synchronize()
    table = P.sched_log_table_ref(sched.ring.cpu().numpy())
    want = [[it, _values(it)[0], _values(it)[1][0], _values(it)[1][2], _values(it)[1][1], 0.0, 0.0, 0.0] for it in (2, 3, 4)]
    assert _same(table, np.array(want, np.float64))
    # a checkpoint: the iteration put back is what begin continues from
    sched.fit.set_schedule_state(2)
    assert _same(sched.fit.schedule_words(), P.sched_words_ref(2, 4, *PAIRS))
    host.fit.lr = _values(2)[0]
    host.iteration(batches, vold, _values(2)[1])
    sched.iteration(batches, vold)
    _equal(host.snap(batches[0]), sched.snap(batches[0]), "resumed")
    assert sched.fit.schedule_state()["iteration"] == 3
    host.close()
    sched.close()


# ------------------------------------------------------------------------------------------------------------------ the gate
def _constant(kl_stop):
    return (0, (LR[0],) * 2, (CLIP[0],) * 2, (CLIP_VF[0],) * 2, (ENT[0],) * 2, kl_stop)


def test_the_gate_drops_the_rest_of_an_update_and_begin_reopens_it():
    """three minibatches whose old log-probabilities lie 0.02, 0.5 and 0.02 above the policy's own: the mean KL of the second is
    read from an ungated pass, and ``kl_stop`` set just below it closes the gate there"""
    spec, params = seeded_policy(*NETS["one"], seed=33)
    probe = _Run(spec, params, 0.5)
    batches = _batches(probe.f, 6, 300, shifts=(0.02, 0.02, 0.5, 0.5, 0.02, 0.02))
    values = (CLIP[0], ENT[0], CLIP_VF[0])
    seen = []
    probe.iteration(batches, True, values, before_step=lambda g: seen.append(probe.log_rows(g)))
    means = [P.fit_kl_gate_ref(rows, 1.0)[3] for rows in seen]
    assert means[0] < 0.25 < means[1] and means[2] < 0.25 and seen[1][:, 7].sum() == 2 * (N - 4)
    probe.close()

    def host_gated(run, kl_stop, state):
        def before_step(g):
            state[:] = P.fit_kl_gate_ref(run.log_rows(g), kl_stop, *state)[:3]
            if state[0]:
                run.fit.set_state(steps=run.fit.state()["steps"])            # drops what has been accumulated
        return before_step

    # just below the mean: the second step and the third are no-ops
    below = float(np.nextafter(means[1], 0.0))
    host, sched = (_Run(spec, params, 0.5, ring) for ring in (0, 2))
    sched.fit.set_schedule(*_constant(below))
    after = []
    sched.iteration(batches, True, gate=True, before_step=lambda g: after.append((sched.fit.state(), sched.fit.schedule_words())))
    state = [0, 0, np.float64(0.0)]
    host.iteration(batches, True, values, before_step=host_gated(host, below, state))
    _equal(host.snap(batches[0]), sched.snap(batches[0]), "below", rows=False)
    assert state[:2] == [1, 2] and _same(np.float64(state[2]), np.float64(means[1]))
    w, f = _words(sched.fit)
    assert list(w[4:7]) == [1, 1, 2] and _same(f[7], np.float64(means[1]))          # iteration 1 now; closed; two steps skipped
    # (`after` was taken behind each gate, in front of its step: the first open, then closed with one and two steps skipped)
    assert [list(x[1][5:7]) for x in after] == [[0, 0], [1, 1], [1, 2]] and _same(after[1][1].view(np.float64)[7], np.float64(means[1]))
    # ... and the end wrote the closed gate's row: two steps skipped, the KL that closed it, stopped
    import torch
    torch.cuda.synchronize()
    table = P.sched_log_table_ref(sched.ring.cpu().numpy())
    assert _same(table, np.array([[0.0, LR[0], CLIP[0], CLIP_VF[0], ENT[0], 2.0, means[1], 1.0]])), table
    # (`A` has no reader on the host: that the no-op steps cleared it is shown below, where the next iteration equals the twin's,
    # whose ``set_state()`` zeroed it - `after` holds theta, m, v and steps alone)
    end = sched.fit.state()
    for k in ("theta", "m", "v", "beta_pow"):                  # nothing moved behind the step that ran before the gate closed
        assert _same(end[k], after[1][0][k]), k
    assert end["steps"] == after[1][0]["steps"] == 1 and not _same(after[0][0]["theta"], end["theta"])
    assert _same(sched.fit._row(sched.fit.grad_norm_ptr(), 2), np.array([0.0, 1.0]))         # the no-op's clip row
    # begin reopens the gate; the accumulators were cleared, so the next iteration is again the host-driven twin's
    sched.fit.schedule_begin()
    w, f = _words(sched.fit)
    assert list(w[4:7]) == [1, 0, 0] and _same(f[7], np.float64(0.0))
    sched.iteration(batches, True, gate=True)
    state[:] = [0, 0, np.float64(0.0)]
    host.iteration(batches, True, values, before_step=host_gated(host, below, state))
    _equal(host.snap(batches[0]), sched.snap(batches[0]), "reopened", rows=False)
    assert sched.fit.state()["steps"] > 1 and sched.fit.schedule_state()["iteration"] == 2
    # a row holding a NaN closes it, whatever kl_stop
    sched.fit.schedule_begin()
    rows = seen[0].copy()
    rows[1, 0] = np.nan
    d_rows = _dev(rows)
    torch.cuda.synchronize()
    sched.fit.kl_gate(d_rows, 2)
    w, f = _words(sched.fit)
    assert list(w[5:7]) == [1, 1] and np.isnan(f[7]) and P.fit_kl_gate_ref(rows, below)[:2] == (1, 1)
    sched.fit.step()                                           # (count = 0: a no-op, and the accumulators are clean for nobody)
    host.close()
    sched.close()

    # exactly at the mean: nothing closes, and the gated fit is the ungated twin
    host, sched = (_Run(spec, params, 0.5) for _ in range(2))
    sched.fit.set_schedule(*_constant(float(means[1])))
    sched.iteration(batches, True, gate=True)
    host.iteration(batches, True, values)
    _equal(host.snap(batches[0]), sched.snap(batches[0]), "at the mean")
    w, f = _words(sched.fit)
    assert list(w[4:7]) == [1, 0, 0] and _same(f[7], np.float64(0.0)) and sched.fit.state()["steps"] == 3
    host.close()
    sched.close()


def test_the_policys_own_log_probabilities_never_close_the_gate():
    """logp_old straight from bsk_policy_act, parameters unchanged: d is +0.0f for every sample, the mean KL exactly 0, and the gate
    stays open under the smallest positive ``kl_stop`` there is"""
    import torch
    spec, params = seeded_policy(*NETS["two"], seed=34)
    run = _Run(spec, params)
    b = _batches(run.f, 1, 400)[0]
    run.f.policy.set_rng(11, 4)
    res = run.f.policy.act(b["obs"], "sample", want=("logp",))
    torch.cuda.synchronize()
    run.fit.set_schedule(*_constant(5e-324))
    run.fit.schedule_begin()
    own = dict(b, actions=res["action"], old=res["logp"])
    run.accumulate(own, OTHER, True, 0)
    run.accumulate(own, OTHER, True, 1)
    run.fit.kl_gate(run.log.data_ptr(), 2)
    rows = run.log_rows(0)
    assert _same(rows[:, 0], np.zeros(2)) and rows[:, 7].sum() == 2 * (N - 2)
    assert P.fit_kl_gate_ref(rows, 5e-324)[:2] == (0, 0)
    assert list(run.fit.schedule_words()[5:7]) == [0, 0]
    run.fit.step()
    assert run.fit.state()["steps"] == 1
    run.close()


# ------------------------------------------------------------------------------------------------------------------ the rules
def test_bad_arguments_are_refused_before_any_launch():
    import torch
    spec, params = seeded_policy(*NETS["one"], seed=35)
    run = _Run(spec, params, ring=2)
    lib, h = _lib.load(), run.fit._handle()
    d_rows = _dev(np.ones((2, 8)))
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    before = run.snap(_batches(run.f, 1, 500)[0])
    c0 = BatchedPropagator.debug_counters()
    # with no schedule attached the three enqueueing calls are refused, and so is the iteration
    assert lib.bsk_fit_schedule_begin(h, None) == EINVAL and lib.bsk_fit_kl_gate(h, vp(d_rows), 2, None) == EINVAL
    assert lib.bsk_fit_schedule_end(h, vp(run.ring), 2, None) == EINVAL and lib.bsk_fit_schedule_end(h, None, 0, None) == EINVAL
    assert lib.bsk_fit_set_schedule_state(h, 1) == EINVAL and b"no schedule" in lib.bsk_last_error()

    def sc(**kw):
        a = dict(lr=LR, clip=CLIP, clip_vf=CLIP_VF, ent_coef=ENT, total=4, kl_stop=0.0)
        a.update(kw)
        return _lib.BskFitSchedule(*[(C.c_double * 2)(*a[k]) for k in ("lr", "clip", "clip_vf", "ent_coef")], a["total"], a["kl_stop"])
    nan, inf = float("nan"), float("inf")
    bads = [dict(lr=(-1e-9, 0.0)), dict(lr=(1e-3, -1.0)), dict(lr=(inf, 0.0)), dict(lr=(0.0, nan)),
            dict(clip=(0.0, 0.1)), dict(clip=(0.2, 1.0)), dict(clip=(nan, 0.1)), dict(clip=(0.2, -0.1)),
            dict(clip_vf=(0.0, 0.2)), dict(clip_vf=(0.2, -0.2)), dict(clip_vf=(inf, 0.2)), dict(clip_vf=(0.2, nan)),
            dict(ent_coef=(-0.01, 0.0)), dict(ent_coef=(0.01, inf)), dict(ent_coef=(nan, 0.0)),
            dict(total=2 ** 53), dict(total=2 ** 64 - 1), dict(kl_stop=-0.01), dict(kl_stop=inf), dict(kl_stop=nan)]
    for bad in bads:
        assert lib.bsk_fit_set_schedule(h, C.byref(sc(**bad))) == EINVAL, bad
    assert lib.bsk_fit_schedule_begin(h, None) == EINVAL       # (a refused schedule attaches nothing)
    assert BatchedPropagator.debug_counters() == c0            # nothing was copied, nothing waited for
    # attached: the gate needs kl_stop > 0, rows and n_rows >= 1; the end a capacity with its ring
    assert lib.bsk_fit_set_schedule(h, C.byref(sc(total=2 ** 53 - 1))) == 0
    c0 = BatchedPropagator.debug_counters()
    assert lib.bsk_fit_kl_gate(h, vp(d_rows), 2, None) == EINVAL and b"kl_stop" in lib.bsk_last_error()
    assert lib.bsk_fit_set_schedule(h, C.byref(sc(kl_stop=0.5))) == 0
    c0 = BatchedPropagator.debug_counters()
    assert lib.bsk_fit_kl_gate(h, None, 2, None) == EINVAL and lib.bsk_fit_kl_gate(h, vp(d_rows), 0, None) == EINVAL
    assert lib.bsk_fit_kl_gate(None, vp(d_rows), 2, None) == EINVAL
    assert lib.bsk_fit_schedule_end(h, vp(run.ring), 0, None) == EINVAL and lib.bsk_fit_schedule_end(h, vp(run.ring), -1, None) == EINVAL
    assert lib.bsk_fit_schedule_device(h, None) == EINVAL and lib.bsk_fit_get_schedule_state(h, None) == EINVAL
    assert BatchedPropagator.debug_counters() == c0
    torch.cuda.synchronize()
    assert _same(run.fit.schedule_words(), P.sched_words_ref(0, 4, *PAIRS)) and (run.ring.cpu().numpy().view(np.int64) == -1).all()
    # the scalars of an accumulate are still validated while a schedule is attached
    b = _batches(run.f, 1, 500)[0]
    for kw in (dict(clip=1.0), dict(ent_coef=-0.1), dict(clip_vf=0.0)):
        a = dict(clip=0.2, ent_coef=0.0, clip_vf=0.2)
        a.update(kw)
        with pytest.raises(ValueError):
            run.fit.accumulate_ppo(b["obs"], b["actions"], b["adv"], b["old"], a["clip"], a["ent_coef"], b["targets"], b["vold"], a["clip_vf"])
        p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
        assert lib.bsk_fit_accumulate_ppo(h, p(b["obs"]), N, N, p(b["actions"]), p(b["adv"]), p(b["old"]), a["clip"], a["ent_coef"],
                                          p(b["targets"]), p(b["vold"]), a["clip_vf"], None, None, N, None, None) == EINVAL, kw
    _equal(before, run.snap(b), "nothing moved")
    # the end with no ring is allowed; the pointer is the fit's, attached or not
    assert lib.bsk_fit_schedule_end(h, None, 0, None) == 0
    assert run.fit.schedule_state()["iteration"] == 1 and run.fit.schedule_ptr()
    # the binding refuses the same with a ValueError, before the library is asked
    for bad in (dict(total=-1), dict(lr=(1e-3,)), dict(clip=(0.2, 1.0)), dict(kl_stop=-1.0)):
        a = dict(total=4, lr=LR, clip=CLIP, clip_vf=CLIP_VF, ent_coef=ENT, kl_stop=0.0)
        a.update(bad)
        with pytest.raises(ValueError):
            run.fit.set_schedule(**a)
    for call in (lambda: run.fit.kl_gate(d_rows, 0), lambda: run.fit.kl_gate(d_rows, 3), lambda: run.fit.kl_gate(None, 1),
                 lambda: run.fit.schedule_end(run.ring, 3), lambda: run.fit.schedule_end(run.ring, 0), lambda: run.fit.set_schedule_state(-1)):
        with pytest.raises(ValueError):
            call()
    run.close()


# ------------------------------------------------------------------------------------------------------------------ a graph
@pytest.mark.parametrize("vold,max_grad_norm", [(True, 0.5), (False, 0.0)])
def test_a_graph_of_one_iteration_anneals_at_every_replay(vold, max_grad_norm):
    import torch
    rounds = 3
    spec, params = seeded_policy(*NETS["one"], seed=36)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eager, replayed = (_Run(spec, params, max_grad_norm, ring=2) for _ in range(2))
        batches = _batches(eager.f, 4, 600)
        for r in (eager, replayed):
            r.warm(batches[0])                                 # (the scratch of the block gradients; no schedule call before the capture)
            r.fit.set_schedule(4, LR, CLIP, CLIP_VF, ENT, kl_stop=1e3)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        c0 = BatchedPropagator.debug_counters()
        with torch.cuda.graph(graph, stream=side):
            replayed.iteration(batches, vold, gate=True, stream=side.cuda_stream)
        for _ in range(rounds):
            graph.replay()
        torch.cuda.synchronize()
        assert BatchedPropagator.debug_counters() == c0         # no copy, no synchronisation
        for _ in range(rounds):
            eager.iteration(batches, vold, gate=True, stream=side.cuda_stream)
        _equal(eager.snap(batches[0]), replayed.snap(batches[0]))
        a, b = (r.ring.cpu().numpy() for r in (eager, replayed))
        assert _same(a, b) and _same(eager.fit.schedule_words(), replayed.fit.schedule_words())
        assert _same(eager.log.cpu().numpy(), replayed.log.cpu().numpy())
        del graph
        # the last two rows: iterations 1 and 2, each trained at its own lr and clip
        table = P.sched_log_table_ref(b)
        want = [[it, _values(it)[0], _values(it)[1][0], _values(it)[1][2], _values(it)[1][1], 0.0, 0.0, 0.0] for it in (1, 2)]
        assert _same(table, np.array(want, np.float64)) and table[0, 1] != table[1, 1] and table[0, 2] != table[1, 2]
        assert replayed.fit.schedule_state()["iteration"] == rounds and replayed.fit.state()["steps"] == 2 * rounds
        # ... and the training is the host-driven twin's, which it cannot be at the captured constants
        host = _Run(spec, params, max_grad_norm)
        for it in range(rounds):
            lr, values = _values(it)
            host.fit.lr = lr
            host.iteration(batches, vold, values, stream=side.cuda_stream)
        _equal(host.snap(batches[0])[:5], replayed.snap(batches[0])[:5], "host")
        for r in (eager, replayed, host):
            r.close()


# ------------------------------------------------------------------------------------------------------------------ the loop
N_ENVS, N_STEPS, ITERS, LOG_CAP = 256, 8, 3, 3
HIST = (("reward", np.float64), ("reason", np.uint8), ("action", np.int32), ("value", np.float32), ("ret", np.float64), ("logp", np.float32),
        ("adv", np.float32))
TODAY = {"obs", "reward", "reason", "action", "logp", "value", "last_value", "adv", "ret", "log", "grad_norm_log", "adv_norm", "adv_work",
         "ep_return", "ep_len", "ep_work", "log_ring", "log_gen", "log_counter"}


def _loop(side, spec, params, **kw):
    """tests/test_gpu_pg_log.py's conditioned loop, with a training log of three rows: every iteration of the test stays in it"""
    n, T = N_ENVS, N_STEPS
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_AUTO_RESET
    cfg.max_length = 5
    root = BatchedPropagator(cfg, n, stream=side.cuda_stream)
    root.set_ic_pool(sample_ic_batch(23, 4, seed=73))
    root.reset(sample_ic_batch(n, 4, seed=72))
    root.step(np.zeros(n, np.int32), 1)
    steps, ticks = root.get_counters()
    root.set_counters(steps + np.arange(n, dtype=np.int32) % 4, ticks)
    f = _PG(spec, params, lr=1e-2)
    f.fit.max_grad_norm = 0.5
    stats = P.ObsStats(n)
    pg = P.PolicyGradient(root, f.policy, f.fit, T, gamma=0.97, lam=0.9, clip=0.2, ent_coef=0.01, epochs=2, minibatches=2, substeps=1,
                          normalize_advantages=True, obs_stats=stats, std_min=1e-6, log_capacity=LOG_CAP, **kw)
    f.policy.set_rng(3, 0)
    return root, f, stats, pg


def _close(root, f, stats, pg):
    pg.close()
    f.close()
    stats.close()
    root.close()


def _iterate(root, pg, bufs):
    """one iterate() -> (its log, the histories, the raw rows, the clip's rows), with the one wait checked"""
    seen, wait = [], root.sync
    root.sync = lambda: (seen.append(BatchedPropagator.debug_counters()), wait())[1]
    before = BatchedPropagator.debug_counters()
    log = pg.iterate()
    root.sync = wait
    T, n = N_STEPS, N_ENVS
    hist = {k: _download(bufs[k], dt, T * n).reshape(T, n) for k, dt in HIST}
    raw = _download(bufs["log"], np.float64, 2 * T * 8).reshape(2 * T, 8)
    return log, hist, raw, pg.grad_norms.copy(), (seen, before)


def test_the_loop_anneals_and_stops_on_the_device_end_to_end():
    import torch
    n, T, rows = N_ENVS, N_STEPS, N_STEPS // 2
    spec, params = seeded_policy((16,), "relu", (16,), seed=16)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        # every new keyword at its default: today's loop, today's buffers - and the KLs of its first iteration, to place kl_stop
        root, f, stats, pg = _loop(side, spec, params)
        torch.cuda.synchronize()
        assert set(pg.buffers()) == TODAY and pg.scheduled is False and f.fit.schedule is None and pg.kl_stop == 0.0
        with pytest.raises(ValueError):
            pg.schedule_log()
        log0, hist0, raw0, norms0, _ = _iterate(root, pg, pg.buffers())
        means = [P.fit_kl_gate_ref(raw0[rows * k:rows * (k + 1)], 1.0)[3] for k in range(4)]
        assert _same(np.float64(means[0]), np.float64(0.0)) and max(means[1:]) > 0.0        # (ratio one in front of the first step)
        kl_stop = float(np.nextafter(max(means[1:]), 0.0))
        first = 1 + int(np.argmax(means[1:]))                  # the minibatch of iteration 0 at which the gate closes
        state0 = f.fit.state()
        _close(root, f, stats, pg)
        # ... and the defaults passed explicitly are the defaults left out: the same buffers, the same run, bit for bit
        root, f, stats, pg = _loop(side, spec, params, total_iterations=None, lr_end=None, clip_end=None, cliprange_vf_end=None,
                                   ent_coef_end=None, kl_stop=0.0)
        torch.cuda.synchronize()
        assert set(pg.buffers()) == TODAY and pg.scheduled is False and f.fit.schedule is None
        log1, hist1, raw1, norms1, _ = _iterate(root, pg, pg.buffers())
        assert _same(log1, log0) and _same(raw1, raw0) and _same(norms1, norms0) and all(_same(hist1[k], hist0[k]) for k, _ in HIST)
        state1 = f.fit.state()
        assert all(_same(state1[k], state0[k]) for k in ("theta", "m", "v", "beta_pow")) and state1["steps"] == state0["steps"] == 4
        _close(root, f, stats, pg)
        for bad in (dict(lr_end=0.0), dict(total_iterations=-1), dict(total_iterations=3, clip_end=1.0), dict(kl_stop=-1.0),
                    dict(total_iterations=3, cliprange_vf_end=0.1), dict(total_iterations=3, lr_end=-1.0)):
            with pytest.raises(ValueError):
                P.PolicyGradient(None, None, type("F", (), {"lr": 1e-2})(), T, **bad)

        # the scheduled loop
        root, f, stats, pg = _loop(side, spec, params, total_iterations=ITERS, lr_end=0.0, clip_end=0.05, kl_stop=kl_stop)
        torch.cuda.synchronize()
        bufs = pg.buffers()
        assert set(bufs) == TODAY | {"sched_ring"} and pg.scheduled and pg.schedule_log().shape == (0, 8)
        assert f.fit.schedule == (ITERS, (1e-2, 0.0), (0.2, 0.05), (1.0, 1.0), (0.01, 0.01), kl_stop)
        got = []
        for it in range(ITERS):
            out = _iterate(root, pg, bufs)
            seen, before = out[4]
            assert seen and seen[0] == before                   # up to the one wait behind the loop: no copy, no synchronisation
            got.append(out[:4] + (f.fit.state(), _download(bufs["log_ring"], np.float64, LOG_CAP * 26).reshape(LOG_CAP, 26)))
        sched_log = pg.schedule_log()
        assert f.fit.schedule_state()["iteration"] == ITERS
        # iteration 0 runs at the starts: up to the minibatch that closes the gate it is the default loop's, row for row
        assert _same(got[0][2][:rows * (first + 1)], raw0[:rows * (first + 1)])
        for k, _ in HIST:
            assert _same(got[0][1][k], hist0[k]), k
        pg.close()
        assert f.fit.schedule is None                           # (close() cleared it)
        # ... and a loop whose fit was closed before it closes without a word: nothing is left to clear
        pg = P.PolicyGradient(root, f.policy, f.fit, T, epochs=1, minibatches=1, kl_stop=0.5)
        assert pg.scheduled and f.fit.schedule[5] == 0.5 and "sched_ring" not in pg.buffers()
        f.fit.close()
        _close(root, f, stats, pg)

        # the twin without a schedule: its host sets the values between iterates and applies the gate from the downloaded rows
        root, f, stats, pg = _loop(side, spec, params)
        torch.cuda.synchronize()
        bufs = pg.buffers()
        box, real = dict(k=0, state=[0, 0, np.float64(0.0)]), f.fit.step

        def gated_step(stream=0):
            root.sync()
            raw = _download(bufs["log"] + 64 * rows * box["k"], np.float64, 8 * rows).reshape(rows, 8)
            box["state"] = list(P.fit_kl_gate_ref(raw, kl_stop, *box["state"])[:3])
            if box["state"][0]:
                f.fit.set_state(steps=f.fit.state()["steps"])
            box["k"] += 1
            real(stream)
        f.fit.step = gated_step
        want_log, skipped = [], 0
        for it in range(ITERS):
            f.fit.lr = float(P.pg_schedule_ref(it, ITERS, 1e-2, 0.0))
            pg.clip = float(P.pg_schedule_ref(it, ITERS, 0.2, 0.05))
            box.update(k=0, state=[0, 0, np.float64(0.0)])
            log = pg.iterate()
            hist = {k: _download(bufs[k], dt, T * n).reshape(T, n) for k, dt in HIST}
            assert _same(log, got[it][0]), it
            for k, _ in HIST:
                assert _same(hist[k], got[it][1][k]), (it, k)
            assert _same(pg.grad_norms, got[it][3]), it
            st = f.fit.state()
            assert all(_same(st[k], got[it][4][k]) for k in ("theta", "m", "v", "beta_pow")) and st["steps"] == got[it][4]["steps"], it
            assert _same(_download(bufs["log_ring"], np.float64, LOG_CAP * 26).reshape(LOG_CAP, 26), got[it][5]), it
            gate, k, at = box["state"]
            want_log.append([it, f.fit.lr, pg.clip, 1.0, 0.01, k, at, gate])
            skipped += k
        # all three rows, iteration 0's - the one with the gate closed by construction - among them
        assert sched_log.shape == (ITERS, 8) and _same(sched_log, np.array(want_log, np.float64)), (sched_log, want_log)
        assert _same(sched_log[0, 5:], np.array([4.0 - first, max(means[1:]), 1.0]))
        assert want_log[0][5] == 4 - first and want_log[0][7] == 1 and 0 < st["steps"] == 4 * ITERS - skipped < 4 * ITERS
        assert want_log[2][1] != want_log[1][1] != want_log[0][1] and want_log[2][2] < want_log[1][2] < 0.2
        _close(root, f, stats, pg)
