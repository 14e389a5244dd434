"""CPU: what basilisk_env_amd/policy_fit.py - PolicyFit, the ten free functions of the policy-gradient loop, PolicyGradient - asks of
the C library and the HIP runtime, call by call, held against a recorded log (tests/golden/fit_binding_calls.json).

The fakes are tests/_binding_fakes.py's, as in tests/test_policy_binding_host.py, here with ``Recorder(offsets=True)``: the loop
hands its launches addresses INSIDE its buffers, and "buf#3+5120" is what pins them.  A fixed script drives every method, good
arguments and bad ones.  The log, the (type, message) of every exception the script provokes and the module's public names were
recorded from policy_fit.py as it stood before its repetitions were folded:
    PYTHONPATH=. python tests/test_fit_binding_host.py --record
writes them anew - which is right only when the sequence of C calls is MEANT to change."""
import json
import os
import types
import zlib

import numpy as np
import pytest

from _binding_fakes import FakeArray as A
from _binding_fakes import FakePropagator, Recorder, _block
from basilisk_env_amd import _hip, _lib
from basilisk_env_amd import policy as P
from basilisk_env_amd import policy_fit as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fit_binding_calls.json")
N, T = 128, 4                                  # the loop's envs and steps; 2 minibatches and 2 epochs


def _arr(a):
    return [a.dtype.str, list(a.shape), "%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes())]


def script_fit(rec, pol, pol0):
    note, raises, log = rec.note, rec.raises, rec.log
    note("PolicyFit")
    raises(F.PolicyFit, None, lr=-1.0)
    raises(F.PolicyFit, None, beta1=1.0)
    raises(F.PolicyFit, None, value_coef=np.nan)
    raises(F.PolicyFit, None, max_grad_norm=-0.5)
    fit = F.PolicyFit(pol)
    fit_c = F.PolicyFit(pol, 3e-4, 0.8, 0.9, 1e-6, 0.01, 0.25, max_grad_norm=0.5)
    fit0 = F.PolicyFit(pol0)
    log.append(["attributes", fit.lr, list(fit.adam), fit.value_coef, fit.max_grad_norm, fit.n_params, fit.device, fit.schedule,
                fit_c.lr, list(fit_c.adam), fit_c.value_coef, fit_c.max_grad_norm])
    n, stream = 96, rec.pointer("stream")
    obs, lab, tgt, liv, dl, adv, old, vold, dv = [rec.pointer(k) for k in ("obs", "lab", "tgt", "liv", "dl", "adv", "old", "vold", "dv")]
    a_obs, a_lab, a_tgt, a_liv, a_dl = A(obs, (5, n), "<f8"), A(lab, (n,), "<i4"), A(tgt, (n,), "<f8"), A(liv, (n,), "|u1"), A(dl, (3, n), "<f4")
    a_adv, a_old, a_vold, a_dv = A(adv, (n,), "<f4"), A(old, (n,), "<f4"), A(vold, (n,), "<f4"), A(dv, (n,), "<f4")
    wide = A(obs, (5, n), "<f8", (8 * 128, 8))
    kept = lambda *xs: log.append(["kept", len(fit._kept) == len(xs) and all(a is b for a, b in zip(fit._kept, xs))])      # noqa: E731

    note("accumulate")
    fit.accumulate(a_obs, a_lab)
    kept(a_obs, a_lab, None, None, None)
    fit.accumulate(wide, a_lab, a_tgt, A(liv, (n,), "|b1"), a_dl, stream=stream)
    fit.accumulate(A(obs, (5, n), "<f8", with_strides=False), a_lab, alive=a_liv)
    fit.accumulate(obs, lab, n=n)
    fit.accumulate(obs + 56, lab + 28, tgt + 56, liv + 7, dl + 28, n=n - 7, stride=128, stream=stream)
    raises(fit.accumulate, A(obs, (5, n), "<f4"), a_lab)
    raises(fit.accumulate, A(obs, (4, n), "<f8"), a_lab)
    raises(fit.accumulate, A(obs, (5, n), "<f8", (8 * n, 16)), a_lab)
    raises(fit.accumulate, obs, a_lab)
    raises(fit.accumulate, a_obs, A(lab, (n,), "<i8"))
    raises(fit.accumulate, a_obs, A(lab, (n - 1,), "<i4"))
    raises(fit.accumulate, a_obs, None)
    raises(fit.accumulate, a_obs, a_lab, A(tgt, (n + 1,), "<f8"))
    raises(fit.accumulate, a_obs, a_lab, A(tgt, (n,), "<f4"))
    raises(fit.accumulate, a_obs, a_lab, None, A(liv, (n,), "<i4"))
    raises(fit.accumulate, a_obs, a_lab, None, A(liv, (n + 1,), "|u1"))
    raises(fit.accumulate, a_obs, a_lab, None, None, A(dl, (n, 3), "<f4"))
    raises(fit.accumulate, obs, lab, n=0)
    raises(fit0.accumulate, a_obs, a_lab, a_tgt)
    raises(fit0.accumulate, obs, lab, tgt, n=n)

    note("accumulate_pg")
    fit.accumulate_pg(a_obs, a_lab, a_adv)
    kept(a_obs, a_lab, a_adv, None, None, None, None)
    fit.accumulate_pg(wide, a_lab, a_adv, a_old, 0.3, 0.01, a_tgt, a_liv, a_dl, stream=stream)
    fit.accumulate_pg(obs, lab, adv, n=n)
    fit.accumulate_pg(obs, lab, adv, None, 7.0, 0.5, n=n)                  # (clip is not read without old log-probabilities)
    fit.accumulate_pg(obs + 8, lab + 4, adv + 4, old + 4, 0.1, 0.02, tgt + 8, liv + 1, dl + 4, n - 1, 128, stream)
    raises(fit.accumulate_pg, a_obs, a_lab, None)
    raises(fit.accumulate_pg, a_obs, None, a_adv)
    raises(fit.accumulate_pg, a_obs, a_lab, A(adv, (n,), "<f8"))
    raises(fit.accumulate_pg, a_obs, a_lab, A(adv, (n + 2,), "<f4"))
    raises(fit.accumulate_pg, a_obs, a_lab, a_adv, A(old, (n,), "<f8"))
    raises(fit.accumulate_pg, a_obs, a_lab, a_adv, A(old, (n - 2,), "<f4"))
    raises(fit.accumulate_pg, a_obs, a_lab, a_adv, a_old, 1.0)
    raises(fit.accumulate_pg, a_obs, a_lab, a_adv, None, 0.2, -1.0)
    raises(fit.accumulate_pg, a_obs, a_lab, a_adv, dlogits=A(dl, (3, n + 1), "<f4"))
    raises(fit.accumulate_pg, obs, lab, adv)

    note("accumulate_ppo")
    fit.accumulate_ppo(a_obs, a_lab, a_adv)
    kept(a_obs, a_lab, a_adv, None, None, None, None, None, None)
    fit.accumulate_ppo(wide, a_lab, a_adv, a_old, 0.3, 0.01, a_tgt, a_vold, 0.25, a_liv, a_dl, a_dv, stream=stream)
    fit.accumulate_ppo(a_obs, a_lab, a_adv, value_targets=a_tgt, dvalue=a_dv)
    fit.accumulate_ppo(obs, lab, adv, n=n)
    fit.accumulate_ppo(obs, lab, adv, old, 0.2, 0.0, tgt, None, 99, n=n)          # (clip_vf is not read without old values)
    fit.accumulate_ppo(obs + 16, lab + 8, adv + 8, old + 8, 0.1, 0.02, tgt + 16, vold + 8, 0.5, liv + 2, dl + 8, dv + 8, n - 2, 128, stream)
    raises(fit.accumulate_ppo, a_obs, a_lab, None)
    raises(fit.accumulate_ppo, a_obs, a_lab, A(adv, (n - 1,), "<f4"))
    raises(fit.accumulate_ppo, a_obs, a_lab, a_adv, A(old, (n + 1,), "<f4"))
    raises(fit.accumulate_ppo, a_obs, a_lab, a_adv, a_old, 0.0)
    raises(fit.accumulate_ppo, a_obs, a_lab, a_adv, value_targets=a_tgt, value_old=A(vold, (n,), "<f8"), clip_vf=0.2)
    raises(fit.accumulate_ppo, a_obs, a_lab, a_adv, value_targets=a_tgt, value_old=A(vold, (n + 3,), "<f4"), clip_vf=0.2)
    raises(fit.accumulate_ppo, a_obs, a_lab, a_adv, value_targets=a_tgt, dvalue=A(dv, (n - 3,), "<f4"))
    raises(fit.accumulate_ppo, a_obs, a_lab, a_adv, value_old=a_vold, clip_vf=0.2)
    raises(fit.accumulate_ppo, a_obs, a_lab, a_adv, dvalue=a_dv)
    raises(fit.accumulate_ppo, a_obs, a_lab, a_adv, value_targets=a_tgt, value_old=a_vold)
    raises(fit.accumulate_ppo, a_obs, a_lab, a_adv, value_targets=a_tgt, value_old=a_vold, clip_vf=0.0)
    raises(fit.accumulate_ppo, a_obs, a_lab, a_adv, value_targets=a_tgt, value_old=a_vold, clip_vf=True)

    note("step / apply_obs_norm")
    stats = P.ObsStats(N)
    fit.step()
    fit.step(stream)
    fit.apply_obs_norm(stats)
    fit.apply_obs_norm(stats, 1e-3, stream)
    stats.close()
    raises(fit.apply_obs_norm, stats)

    note("pointers and rows")
    for name in ("stats_ptr", "pg_stats_ptr", "vclip_stats_ptr", "grad_norm_ptr", "schedule_ptr"):
        log.append([name + " ->", rec.name_of(getattr(fit, name)())])
    for name in ("stats", "pg_stats", "vclip_stats", "grad_norm"):
        row = getattr(fit, name)()
        log.append([name + " ->", [[k, type(v).__name__, v] for k, v in row.items()]])
    log.append(["_row ->", _arr(fit._row(fit.stats_ptr() + 16, 2))])

    note("state")
    st = fit.state()
    log.append(["state ->", [[k, st[k] if k == "steps" else _arr(st[k])] for k in st]])
    fit.set_state()
    fit.set_state(_block(fit.n_params, np.float32, 1.0), None, _block(fit.n_params, np.float64, 2.0), [0.5, 0.25], 9)
    fit.set_state(m=_block(fit.n_params), steps=3)
    raises(fit.set_state, _block(fit.n_params + 1))
    raises(fit.set_state, beta_pow=[0.5])

    note("lr / max_grad_norm")
    fit.lr = 0.125
    fit.max_grad_norm = 2
    fit.max_grad_norm = 0.0
    log.append(["attributes", fit.lr, fit.max_grad_norm])
    raises(setattr, fit, "lr", -1.0)
    raises(setattr, fit, "lr", np.inf)
    raises(setattr, fit, "max_grad_norm", np.nan)
    log.append(["attributes", fit.lr, fit.max_grad_norm])

    note("schedule")
    diag, ring = rec.pointer("diag"), rec.pointer("ring")
    fit.set_schedule(10, (1e-3, 0.0), (0.2, 0.1), (0.2, 0.2), (0.01, 0.0))
    log.append(["schedule", json.loads(json.dumps(fit.schedule))])
    fit.set_schedule(0, [0.5, 0.5], (0.3, 0.3), (1.0, 2.0), (0.0, 0.0), kl_stop=0.02)
    log.append(["schedule", json.loads(json.dumps(fit.schedule))])
    raises(fit.set_schedule, -1, (1e-3, 0.0), (0.2, 0.1), (0.2, 0.2), (0.01, 0.0))
    raises(fit.set_schedule, 10, (1e-3, -1.0), (0.2, 0.1), (0.2, 0.2), (0.01, 0.0))
    raises(fit.set_schedule, 10, (1e-3, 0.0), (0.2, 0.1), (0.2, 0.2), (0.01, 0.0), True)
    log.append(["schedule", json.loads(json.dumps(fit.schedule))])
    fit.schedule_begin()
    fit.schedule_begin(stream)
    fit.kl_gate(diag, 2)
    fit.kl_gate(diag + 128, np.int64(3), stream)
    fit.kl_gate(A(diag, (2, 8), "<f8"), 2, stream)
    raises(fit.kl_gate, diag, True)
    raises(fit.kl_gate, diag, 0)
    raises(fit.kl_gate, None, 2)
    raises(fit.kl_gate, A(diag, (15,), "<f8"), 2)
    raises(fit.kl_gate, A(diag, (2, 8), "<f4"), 2)
    fit.schedule_end()
    fit.schedule_end(None, 5, stream)
    fit.schedule_end(ring, 3)
    fit.schedule_end(ring + 64, np.int32(2), stream)
    fit.schedule_end(A(ring, (3, 8), "<f8"), 3, stream)
    raises(fit.schedule_end, ring, 0)
    raises(fit.schedule_end, ring, True)
    raises(fit.schedule_end, ring, 2 ** 31)
    raises(fit.schedule_end, A(ring, (23,), "<f8"), 3)
    raises(fit.schedule_end, A(ring, (3, 8), "<u8"), 3)
    log.append(["schedule_words ->", _arr(fit.schedule_words())])
    log.append(["schedule_state ->", [[k, type(v).__name__, v] for k, v in fit.schedule_state().items()]])
    fit.set_schedule_state(0)
    fit.set_schedule_state(np.uint64(2 ** 64 - 1))
    raises(fit.set_schedule_state, True)
    raises(fit.set_schedule_state, -1)
    raises(fit.set_schedule_state, 2 ** 64)
    fit.clear_schedule()
    log.append(["schedule", fit.schedule])

    note("close")
    fit.close()
    log.append(["after close", fit._kept == (), fit._p is None])
    fit.close()
    raises(fit.step)
    raises(fit.accumulate, a_obs, a_lab)
    raises(fit.accumulate, a_obs, None)            # (the argument rules come before the closed handle)
    raises(fit.stats_ptr)
    raises(fit.stats)
    fit_c.close()
    fit0.close()


def script_functions(rec):
    note, raises = rec.note, rec.raises
    S, W = T * N, 192                              # samples of a rollout; a wider stride
    stream = rec.pointer("stream")
    rew, rea, val, last, adv, ret, act, logp, out = [rec.pointer(k) for k in ("rew", "rea", "val", "last", "adv", "ret", "act", "logp", "out")]
    a_rew, a_rea, a_val, a_adv, a_ret = A(rew, (T, N), "<f8"), A(rea, (T, N), "|u1"), A(val, (T, N), "<f4"), A(adv, (T, N), "<f4"), A(ret, (T, N), "<f8")
    a_act = A(act, (T, N), "<i4")

    note("gae")
    F.gae(rew, rea, val, None, T, N, adv)
    F.gae(rew, rea, val, last, T, N, adv, ret, 0.9, 0.8, W, stream)
    F.gae(a_rew, A(rea, (T, N), "|b1"), a_val, A(last, (N,), "<f4"), T, N, a_adv, a_ret, stream=stream)
    raises(F.gae, a_rew, a_rea, a_val, None, T, N, A(adv, (T - 1, N), "<f4"))
    raises(F.gae, a_rew, a_rea, a_val, A(last, (N - 1,), "<f4"), T, N, a_adv)
    raises(F.gae, A(rew, (T, N), "<f4"), a_rea, a_val, None, T, N, a_adv)
    raises(F.gae, a_rew, a_rea, a_val, None, T, N, a_adv, stride=W)
    raises(F.gae, rew, rea, val, None, 0, N, adv)

    note("normalize_advantages")
    work, alive = rec.pointer("work"), rec.pointer("alive")
    wb = F.adv_normalize_work_bytes(N)
    F.normalize_advantages(adv, 2, N, work=work)
    F.normalize_advantages(adv + 4 * N * 2, 2, N, out, alive, 1e-6, W, work, stream)
    F.normalize_advantages(A(adv, (2, N), "<f4"), 2, N, work=A(work, (wb,), "|u1"))
    F.normalize_advantages(A(adv, (2, N), "<f4"), 2, N, A(out, (2, N), "<f4"), A(alive, (2, N), "|u1"), work=A(work, (wb // 8,), "<u8"), stream=stream)
    raises(F.normalize_advantages, adv, 2, N)
    raises(F.normalize_advantages, adv, 2, N, work=A(work, (wb - 1,), "|u1"))
    raises(F.normalize_advantages, adv, 2, N, work=A(work, (wb // 8 - 1,), "<u8"))
    raises(F.normalize_advantages, adv, 2, N, work=A(work, (wb // 4,), "<f4"))
    raises(F.normalize_advantages, A(adv, (2, N - 1), "<f4"), 2, N, work=work)
    raises(F.normalize_advantages, adv, 2, N, A(out, (N,), "<f4"), work=work)
    raises(F.normalize_advantages, adv, 2, N, alive=A(alive, (2, N), "<f4"), work=work)
    raises(F.normalize_advantages, adv, 0, N, work=work)

    note("reward_normalize")
    state, run = rec.pointer("state"), rec.pointer("run")
    rb = F.reward_norm_work_bytes(N)
    F.reward_normalize(rew, rea, T, N, state, None, run, work)
    F.reward_normalize(rew, rea, T, N, state, out, run, work, 0.9, 1e-6, 5.0, True, W, stream)
    F.reward_normalize(rew, rea, T, N, state, update=False)
    F.reward_normalize(rew + 8, rea + 1, T, N - 1, state, out + 8, None, None, update=0, stride=N, stream=stream)
    F.reward_normalize(a_rew, a_rea, T, N, A(state, (8,), "<u8"), A(out, (T, N), "<f8"), A(run, (N,), "<f8"), A(work, (rb,), "|u1"), stream=stream)
    F.reward_normalize(a_rew, a_rea, T, N, A(state, (64,), "|u1"), None, A(run, (N,), "<f8"), A(work, (rb // 8,), "<u8"))
    F.reward_normalize(a_rew, a_rea, T, N, A(state, (8,), "<i8"), update=False)
    raises(F.reward_normalize, None, rea, T, N, state, None, run, work)
    raises(F.reward_normalize, rew, rea, T, N, None, None, run, work)
    raises(F.reward_normalize, rew, rea, T, N, state, None, None, work)
    raises(F.reward_normalize, rew, rea, T, N, state, None, run)
    raises(F.reward_normalize, rew, rea, T, N, A(state, (63,), "|u1"), None, run, work)
    raises(F.reward_normalize, rew, rea, T, N, A(state, (7,), "<u8"), None, run, work)
    raises(F.reward_normalize, rew, rea, T, N, state, None, run, A(work, (rb // 8 - 1,), "<i8"))
    raises(F.reward_normalize, rew, rea, T, N, state, A(out, (T, N - 1), "<f8"), run, work)
    raises(F.reward_normalize, rew, rea, T, N, A(state, (8,), "<f4"), None, run, work)

    note("pg_gather")
    obs, words, idx = rec.pointer("obs"), rec.pointer("words"), rec.pointer("idx")
    o = [rec.pointer("mb") for _ in range(6)]
    M = 2 * N
    F.pg_gather(words, T, N, M, M, obs, act, adv, logp, ret, val, *o)
    F.pg_gather(None, T, N, 0, M, obs, act, adv, logp, ret, None, o[0], o[1], o[2], o[3], o[4], None, idx, W, M + 64, stream)
    F.pg_gather(words, T, N, 3, 5, index_out=idx)
    F.pg_gather(words + 16, T, N, 0, M, adv=adv + 4, adv_out=o[2] + 4, stream=stream)
    F.pg_gather(A(words, (2,), "<u8"), T, N, M, M, A(obs, (T, 5, N), "<f8"), a_act, a_adv, A(logp, (T, N), "<f4"), a_ret, a_val,
                A(o[0], (5, M), "<f8"), A(o[1], (M,), "<i4"), A(o[2], (M,), "<f4"), A(o[3], (M,), "<f4"), A(o[4], (M,), "<f8"),
                A(o[5], (M,), "<f4"), A(idx, (M,), "<i4"), stream=stream)
    raises(F.pg_gather, words, T, N, 0, M, obs)
    raises(F.pg_gather, words, T, N, 0, M, value_out=o[5])
    raises(F.pg_gather, words, T, N, 0, M)
    raises(F.pg_gather, A(words, (1,), "<u8"), T, N, 0, M, index_out=idx)
    raises(F.pg_gather, A(words, (2,), "<f8"), T, N, 0, M, index_out=idx)
    raises(F.pg_gather, words, T, N, 0, M, A(obs, (T, 5, N - 1), "<f8"), obs_out=o[0])
    raises(F.pg_gather, words, T, N, 0, M, obs, obs_out=A(o[0], (5, M - 1), "<f8"))
    raises(F.pg_gather, words, T, N, 0, M, action_hist=A(act, (T, N), "<f4"), action_out=o[1])
    raises(F.pg_gather, words, T, N, 0, M, index_out=A(idx, (M - 1,), "<i4"))
    raises(F.pg_gather, words, T, N, M, S, index_out=idx)

    note("pg_shuffle_advance")
    F.pg_shuffle_advance(words)
    F.pg_shuffle_advance(words + 16, stream)
    F.pg_shuffle_advance(A(words, (2,), "<u8"), stream)
    raises(F.pg_shuffle_advance, None)
    raises(F.pg_shuffle_advance, A(words, (1,), "<u8"))
    raises(F.pg_shuffle_advance, A(words, (2,), "<f8"))

    note("pg_episodes")
    epr, epl, ring, counter, gen = [rec.pointer(k) for k in ("epr", "epl", "ring", "counter", "gen")]
    eb = F.pg_episodes_work_bytes(N)
    F.pg_episodes(rew, rea, T, N, epr, epl, work, ring, 3)
    F.pg_episodes(rew, rea, T, N, epr, epl, work, ring, 3, counter, act, val, ret, W, stream)
    F.pg_episodes(rew, rea, T, N, epr, epl, work, ring + 8 * 26, 2, None, act)
    F.pg_episodes(a_rew, a_rea, T, N, A(epr, (N,), "<f8"), A(epl, (N,), "<i4"), A(work, (eb,), "|u1"), A(ring, (3, 26), "<f8"), 3,
                  A(counter, (1,), "<u8"), a_act, a_val, a_ret, stream=stream)
    F.pg_episodes(a_rew, a_rea, T, N, A(epr, (N,), "<f8"), A(epl, (N,), "<i4"), A(work, (eb // 8,), "<u8"), A(ring, (3, 26), "<f8"), 3,
                  A(counter, (), "<i8"))
    raises(F.pg_episodes, rew, None, T, N, epr, epl, work, ring, 3)
    raises(F.pg_episodes, rew, rea, T, N, epr, None, work, ring, 3)
    raises(F.pg_episodes, rew, rea, T, N, epr, epl, None, ring, 3)
    raises(F.pg_episodes, rew, rea, T, N, epr, epl, work, None, 3)
    raises(F.pg_episodes, rew, rea, T, N, epr, epl, A(work, (eb - 1,), "|u1"), ring, 3)
    raises(F.pg_episodes, rew, rea, T, N, epr, epl, A(work, (eb // 8 - 1,), "<i8"), ring, 3)
    raises(F.pg_episodes, rew, rea, T, N, epr, epl, work, A(ring, (2, 26), "<f8"), 3)
    raises(F.pg_episodes, rew, rea, T, N, epr, epl, work, ring, 3, A(counter, (0,), "<u8"))
    raises(F.pg_episodes, rew, rea, T, N, epr, A(epl, (N,), "<i8"), work, ring, 3)
    raises(F.pg_episodes, rew, rea, T, N, epr, epl, work, ring, 3, value_hist=val)

    note("pg_log_update")
    diag, norms = rec.pointer("diag"), rec.pointer("norms")
    F.pg_log_update(diag, 8, ring, 3)
    F.pg_log_update(diag, 8, ring, 3, counter, norms, 4, stream)
    F.pg_log_update(diag, 8, ring, 3, None, None, 4)                       # (n_norms is not read without norms)
    F.pg_log_update(A(diag, (8, 8), "<f8"), 8, A(ring, (3, 26), "<f8"), 3, A(counter, (1,), "<u8"), A(norms, (4, 2), "<f8"), 4, stream)
    raises(F.pg_log_update, diag, 8, ring, 3, norms=norms)
    raises(F.pg_log_update, None, 8, ring, 3)
    raises(F.pg_log_update, diag, 8, None, 3)
    raises(F.pg_log_update, A(diag, (7, 8), "<f8"), 8, ring, 3)
    raises(F.pg_log_update, diag, 8, ring, 3, norms=A(norms, (3, 2), "<f8"), n_norms=4)
    raises(F.pg_log_update, diag, 8, A(ring, (3, 25), "<f8"), 3)
    raises(F.pg_log_update, diag, 8, ring, 3, A(counter, (1,), "<f8"))
    raises(F.pg_log_update, diag, 8, ring, 3, norms=norms, n_norms=0)

    note("pg_log_advance")
    F.pg_log_advance(gen, 3, counter)
    F.pg_log_advance(gen + 8, 2, counter, stream)
    F.pg_log_advance(A(gen, (3,), "<u8"), 3, A(counter, (1,), "<i8"), stream)
    raises(F.pg_log_advance, None, 3, counter)
    raises(F.pg_log_advance, gen, 3, None)
    raises(F.pg_log_advance, A(gen, (2,), "<u8"), 3, counter)
    raises(F.pg_log_advance, gen, 3, A(counter, (0,), "<u8"))
    raises(F.pg_log_advance, A(gen, (3,), "<f8"), 3, counter)


def script_loop(rec, pol, pol0):
    note, raises, log = rec.note, rec.raises, rec.log
    prop = FakePropagator(rec, N, 0)
    prop.cfg = types.SimpleNamespace(flags=_lib.FLAG_AUTO_RESET)
    env = types.SimpleNamespace(propagator=prop)

    def loop(title, extra=None, max_grad_norm=0.0, source=prop, **kw):
        note("PolicyGradient", title)
        fit = F.PolicyFit(pol, lr=0.001, max_grad_norm=max_grad_norm)
        pg = F.PolicyGradient(source, pol, fit, T, epochs=2, minibatches=2, **kw)
        log.append(["attributes", pg.n_envs, pg.shuffle, pg.cliprange_vf, pg.log_capacity, pg.normalize_advantages, pg.normalize_rewards,
                    pg.scheduled, pg.kl_stop, json.loads(json.dumps(fit.schedule))])
        note("collect")
        pg.collect()
        note("update")
        pg.update()
        note("iterate")
        out = pg.iterate()
        log.append(["iterate ->", _arr(out), None if pg.grad_norms is None else _arr(pg.grad_norms)])
        sizes = {row[1]: row[2] for row in log if row[0] == "DeviceBuffer"}
        log.append(["buffers", [[k, rec.name_of(p), sizes[rec.name_of(p)]] for k, p in pg.buffers().items()]])
        if extra:
            note("extras")
            extra(pg, fit)
        note("close")
        pg.close()
        pg.close()
        fit.close()

    def guards(pg, fit):
        for fn, args in ((pg.schedule_log, ()), (pg.shuffle_state, ()), (pg.set_shuffle_state, (1,)), (pg.training_log, ()), (pg.episode_state, ()),
                         (pg.set_episode_state, (np.zeros(N), np.zeros(N))), (pg.reward_norm_state, ()),
                         (pg.set_reward_norm_state, (np.zeros(8, np.uint64), np.zeros(N))), (pg.reward_scale, ())):
            raises(fn, *args)

    def shuffled(pg, fit):
        log.append(["shuffle_state ->", list(pg.shuffle_state())])
        pg.set_shuffle_state(5, 2)
        pg.set_shuffle_state(np.uint64(2 ** 64 - 1))
        raises(pg.set_shuffle_state, -1)
        raises(pg.set_shuffle_state, 1, True)
        raises(pg.set_shuffle_state, 1, -1)
        raises(pg.set_shuffle_state, 1, 2 ** 64)
        raises(pg.training_log)

    def logged(pg, fit):
        log.append(["training_log ->"] + [_arr(a) for a in pg.training_log()])
        R, L, c = pg.episode_state()
        log.append(["episode_state ->", _arr(R), _arr(L), c])
        pg.set_episode_state(_block(N, np.float64, 1.0), np.arange(N), 7)
        pg.set_episode_state(list(_block(N)), np.arange(N, dtype=np.int64).reshape(2, N // 2))
        raises(pg.set_episode_state, np.zeros(N - 1), np.zeros(N))
        raises(pg.set_episode_state, np.zeros(N), np.zeros(N + 1))
        raises(pg.set_episode_state, np.zeros(N), np.zeros(N), True)
        raises(pg.set_episode_state, np.zeros(N), np.zeros(N), -1)
        raises(pg.set_episode_state, np.zeros(N), np.zeros(N), 2 ** 64)
        raises(pg.schedule_log)

    def rewards(pg, fit):
        pg.update_reward_stats = False
        note("collect, statistics frozen")
        pg.collect()
        words, R = pg.reward_norm_state()
        log.append(["reward_norm_state ->", _arr(words), _arr(R)])
        pg.set_reward_norm_state(np.arange(8, dtype=np.uint64), _block(N, np.float64))
        log.append(["reward_scale ->", pg.reward_scale()])
        raises(pg.set_reward_norm_state, np.zeros(8), np.zeros(N))
        raises(pg.set_reward_norm_state, np.zeros(7, np.uint64), np.zeros(N))
        raises(pg.set_reward_norm_state, np.zeros(8, np.uint64), np.zeros(N + 1))

    def scheduled(pg, fit):
        log.append(["schedule_log ->", _arr(pg.schedule_log())])
        log.append(["training_log ->"] + [_arr(a) for a in pg.training_log()])

    loop("plain", guards)
    loop("normalize_advantages", source=env, normalize_advantages=True)
    loop("shuffle, normalize_advantages, cliprange_vf", shuffled, shuffle=True, seed=11, normalize_advantages=True, cliprange_vf=0.2)
    loop("cliprange_vf", cliprange_vf=0.25)
    loop("log_capacity", logged, log_capacity=3)
    loop("normalize_rewards", rewards, normalize_rewards=True, reward_clip=5.0, reward_eps=1e-6)
    loop("schedule, kl_stop, log_capacity", scheduled, total_iterations=5, lr_end=0.0, kl_stop=0.02, log_capacity=3)
    stats = P.ObsStats(N)
    loop("obs_stats, max_grad_norm", max_grad_norm=0.5, obs_stats=stats, std_min=1e-3, gamma=0.9, lam=0.8, clip=0.3, ent_coef=0.0, substeps=2)
    log.append(["obs_stats detached", pol._stats is None])

    note("PolicyGradient", "refusals")
    fit = F.PolicyFit(pol)
    other = FakePropagator(rec, N, 1)
    other.cfg = prop.cfg
    plain = FakePropagator(rec, N, 0)
    plain.cfg = types.SimpleNamespace(flags=0)
    raises(F.PolicyGradient, prop, pol, fit, T, minibatches=3)
    raises(F.PolicyGradient, prop, pol, fit, T, shuffle=1)
    raises(F.PolicyGradient, prop, pol, fit, T, cliprange_vf=0.0)
    raises(F.PolicyGradient, prop, pol, fit, T, log_capacity=True)
    raises(F.PolicyGradient, prop, pol, fit, T, log_capacity=-1)
    raises(F.PolicyGradient, prop, pol, fit, T, log_capacity=2 ** 31)
    raises(F.PolicyGradient, prop, pol, fit, T, std_min=0.0)
    raises(F.PolicyGradient, prop, pol, fit, T, reward_clip=0.0)
    raises(F.PolicyGradient, prop, pol, fit, T, total_iterations=5, cliprange_vf_end=0.1)
    raises(F.PolicyGradient, prop, pol, fit, T, total_iterations=-1)
    raises(F.PolicyGradient, prop, pol, fit, T, lr_end=0.0)
    raises(F.PolicyGradient, plain, pol, fit, T)
    raises(F.PolicyGradient, prop, pol0, fit, T)
    raises(F.PolicyGradient, prop, pol, types.SimpleNamespace(policy=pol0), T)
    raises(F.PolicyGradient, other, pol, fit, T)
    small = P.ObsStats(N - 1)
    raises(F.PolicyGradient, prop, pol, fit, T, obs_stats=small)
    for obj in (small, stats, fit):
        obj.close()


def run_script(patch):
    """Drives policy_fit over the fakes; ``patch(object, name, value)`` is pytest's ``monkeypatch.setattr``."""
    rec = Recorder(offsets=True)
    patch(_lib, "load", lambda: rec.lib)
    patch(_hip, "DeviceBuffer", rec.DeviceBuffer)
    patch(_hip, "runtime", lambda: rec.rt)
    spec_v, spec = P.check_spec((16,), "tanh", (32,), "relu"), P.check_spec((16,), "relu")
    rec.sizes = {"np": P.n_params(spec)}
    pol0 = P.DevicePolicy(spec, _block(P.n_params(spec)))
    rec.sizes = {"np": P.n_params(spec_v)}
    pol = P.DevicePolicy(spec_v, _block(P.n_params(spec_v)))
    script_fit(rec, pol, pol0)
    script_functions(rec)
    script_loop(rec, pol, pol0)
    pol.close()
    pol0.close()
    return [row[:2] if row[0] == "raised" else row for row in rec.log], rec.errors          # (the texts are in the second list)


def public_names():
    """what ``basilisk_env_amd.policy_fit`` offers: no modules, and nothing that merely came along from a library"""
    names = []
    for name in dir(F):
        obj = getattr(F, name)
        if name.startswith("_") or isinstance(obj, types.ModuleType):
            continue
        if not getattr(obj, "__module__", "basilisk_env_amd").startswith("basilisk_env_amd"):
            continue
        names.append(name)
    return sorted(names)


def test_the_fit_and_the_loop_make_the_recorded_calls(monkeypatch):
    golden = json.load(open(GOLDEN))
    log, errors = run_script(monkeypatch.setattr)
    log, errors = json.loads(json.dumps(log)), json.loads(json.dumps(errors))
    assert errors == golden["exceptions"]
    for k, (got, want) in enumerate(zip(log, golden["calls"])):
        assert got == want, "entry %d: %r, recorded %r" % (k, got, want)
    assert len(log) == len(golden["calls"])
    assert ["RuntimeError", "policy fit is closed"] in errors
    destroyed = [row[1] for row in log if row[0].endswith("_destroy")]
    assert len(destroyed) == len(set(destroyed)) and sum(name.startswith("fit#") for name in destroyed) == 12


def test_every_recorded_public_name_is_still_there():
    golden = json.load(open(GOLDEN))
    missing = sorted(set(golden["public_names"]) - set(public_names()))
    assert not missing, missing
    for name in ("PolicyFit", "PolicyGradient", "gae", "normalize_advantages", "reward_normalize", "pg_gather", "pg_shuffle_advance",
                 "pg_episodes", "pg_log_update", "pg_log_advance"):
        assert name in golden["public_names"]


if __name__ == "__main__":
    import sys
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: PYTHONPATH=. python tests/test_fit_binding_host.py --record")
    with pytest.MonkeyPatch.context() as mp:
        calls, exceptions = run_script(mp.setattr)
    with open(GOLDEN, "w") as f:
        rows = lambda items: "[\n" + ",\n".join(json.dumps(x, separators=(",", ":")) for x in items) + "\n]"      # noqa: E731 - one entry per line
        f.write('{"calls": %s,\n"exceptions": %s,\n"public_names": %s}\n' % (rows(calls), rows(exceptions), json.dumps(public_names())))
    print("%d calls, %d exceptions -> %s" % (len(calls), len(exceptions), GOLDEN))
