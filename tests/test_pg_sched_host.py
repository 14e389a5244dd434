"""CPU: what the schedules and the KL stop of the policy-gradient loop state without a device - ``pg_schedule_ref`` and
``fit_kl_gate_ref`` (include/bskgpu.h, bsk_fit_set_schedule / bsk_fit_kl_gate; csrc/bsk_pgsched.hip), the argument rules
``check_pg_schedule``, and the inline functions of csrc/bsk_pgsched.hpp themselves - the text the kernels and the C-ABI run -
compiled for the HOST (tools/pg_sched_host.cpp) under the address and undefined-behaviour sanitizers and held to the restatements
bit for bit, before a GPU runs them.  No case is skipped."""
import os
import subprocess

import numpy as np
import pytest

from _device_bits import same as _same
from _pg_sched_cases import GATE_CASES, INEXACT_PAIR, SCHEDULE_CASES, gate_want
from basilisk_env_amd import _lib
from basilisk_env_amd import policy as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rule_is_exact_at_both_ends_and_a_line_between():
    kinds = set()
    for it, total, a, b, kind in SCHEDULE_CASES:
        got = P.pg_schedule_ref(it, total, a, b)
        assert isinstance(got, np.float64), (it, total)
        if kind == "a":
            assert (total == 0 or it == 0) and _same(got, np.float64(a)), (it, total, a, b)
        elif kind == "b":
            assert total > 0 and it >= total and _same(got, np.float64(b)), (it, total, a, b)
        else:
            assert 0 < it < total
            frac = np.float64(it) / np.float64(total)
            assert _same(got, np.float64(a) + (np.float64(b) - np.float64(a)) * frac), (it, total, a, b)
            assert min(a, b) <= got <= max(a, b)
        kinds.add(kind)
    assert kinds == {"a", "b", "line"}
    assert any(b > a for _, _, a, b, k in SCHEDULE_CASES if k == "line") and any(t == 1 for _, t, _, _, _ in SCHEDULE_CASES)
    assert any(t == 2 ** 31 and it == t - 1 for it, t, _, _, _ in SCHEDULE_CASES)


def test_the_last_branch_matters():
    a, b = (np.float64(x) for x in INEXACT_PAIR)
    assert a + (b - a) != b and abs((a + (b - a)) - b) <= np.spacing(a)           # off by a last place of the sum's operands
    assert _same(P.pg_schedule_ref(4, 4, a, b), b) and _same(P.pg_schedule_ref(10 ** 9, 4, a, b), b)
    # ... and PPO2's lr * (1 - (update - 1) / nupdates) is the rule with b = 0, to within the rounding of its other association
    for it in range(6):
        lr = np.float64(2.5e-4)
        ppo2 = lr * (np.float64(1.0) - np.float64(it) / np.float64(6))
        assert abs(P.pg_schedule_ref(it, 6, lr, 0.0) - ppo2) <= 2 * np.spacing(lr)
    assert P.pg_schedule_ref(6, 6, 2.5e-4, 0.0) == 0.0
    for bad in ((-1, 4), (0, 2 ** 53), (0, -1)):
        with pytest.raises(ValueError):
            P.pg_schedule_ref(bad[0], bad[1], 0.1, 0.2)


def test_the_words_of_an_iteration():
    pairs = ((1e-2, 0.0), (0.2, 0.05), (0.3, 0.9), (0.01, 0.001))
    w = P.sched_words_ref(3, 4, *pairs)
    assert w.dtype == np.uint64 and w.shape == (P.SCHED_WORDS,) == (8,) and list(w[4:]) == [3, 0, 0, 0]
    assert _same(w.view(np.float64)[:4], np.array([P.pg_schedule_ref(3, 4, *p) for p in pairs]))
    assert P.SCHED_LOG_COLUMNS == ("iteration", "lr", "clip", "clip_vf", "ent_coef", "steps_skipped", "kl_at_stop", "stopped")
    assert len(P.SCHED_STATE_FIELDS) == 8 and P.PG_LOG_COLS == 26 == len(P.PG_LOG_COLUMNS)
    ring = np.full((3, 8), np.nan)
    ring.view(np.uint64)[:] = 2 ** 64 - 1                      # memset to 0xFF: never written
    assert P.sched_log_table_ref(ring).shape == (0, 8)
    ring[2], ring[0] = np.arange(8.0) + 3, np.arange(8.0) + 4
    assert _same(P.sched_log_table_ref(ring), ring[[2, 0]])


@pytest.mark.parametrize("case", GATE_CASES, ids=[c[0] for c in GATE_CASES])
def test_the_gate(case):
    name, rows, stop, gate, skipped, at, _ = case
    want = gate_want(case)
    g, k, a, mean = P.fit_kl_gate_ref(rows, stop, gate, skipped, at)
    assert (g, k) == want[:2] and _same(np.float64(a), want[2]), (name, g, k, a, want)
    if gate == 0 and g == 1:
        assert _same(np.float64(a), np.float64(mean)) and not (mean <= stop)
    if gate == 0 and g == 0:
        assert not (rows[:, 7].sum() > 0) or mean <= stop
    junk = rows.copy()                                         # columns 1 .. 6 are not the gate's
    junk[:, 1:7] = np.nan
    assert P.fit_kl_gate_ref(junk, stop, gate, skipped, at)[:2] == (g, k)
    for bad in (rows[:, :7], rows[:0], rows[0]):
        with pytest.raises(ValueError):
            P.fit_kl_gate_ref(bad, stop)


def test_the_argument_rules():
    good = dict(total=4, lr=(1e-3, 0.0), clip=(0.2, 0.05), clip_vf=(0.2, 0.2), ent_coef=(0.01, 0.0), kl_stop=0.0)
    assert P.check_pg_schedule(**good) == (4, (1e-3, 0.0), (0.2, 0.05), (0.2, 0.2), (0.01, 0.0), 0.0)
    assert P.check_pg_schedule(0, (0, 0), (0.5, 0.5), (1, 1), (0, 0), 0.03)[5] == 0.03
    assert P.check_pg_schedule(**dict(good, total=2 ** 53 - 1))[0] == 2 ** 53 - 1
    nan, inf = float("nan"), float("inf")
    bads = [dict(total=-1), dict(total=2 ** 53), dict(total=1.0), dict(total=True), dict(total=None),
            dict(lr=(-1e-9, 0.0)), dict(lr=(1e-3, -1.0)), dict(lr=(inf, 0.0)), dict(lr=(1e-3, nan)), dict(lr=1e-3), dict(lr=(1e-3,)),
            dict(clip=(0.0, 0.1)), dict(clip=(0.2, 1.0)), dict(clip=(0.2, 0.0)), dict(clip=(nan, 0.1)), dict(clip=(0.2, -0.1)),
            dict(clip_vf=(0.0, 0.2)), dict(clip_vf=(0.2, -0.2)), dict(clip_vf=(inf, 0.2)), dict(clip_vf=(0.2, nan)),
            dict(ent_coef=(-0.01, 0.0)), dict(ent_coef=(0.01, inf)), dict(ent_coef=(nan, 0.0)), dict(ent_coef=(0.0, True)),
            dict(kl_stop=-0.01), dict(kl_stop=inf), dict(kl_stop=nan), dict(kl_stop=True)]
    for bad in bads:
        with pytest.raises(ValueError):
            P.check_pg_schedule(**dict(good, **bad))


def test_the_symbols_are_declared_and_exported():
    lib = _lib.load()
    names = ("bsk_fit_set_schedule", "bsk_fit_schedule_begin", "bsk_fit_kl_gate", "bsk_fit_schedule_end", "bsk_fit_schedule_device",
             "bsk_fit_get_schedule_state", "bsk_fit_set_schedule_state")
    with open(os.path.join(ROOT, "include", "bskgpu.h")) as f:
        header = f.read()
    for name in names:
        assert name in _lib.EXPORTS and name in _lib.SIGNATURES and hasattr(lib, name) and ("int %s(bsk_fit* f" % name) in header, name
    assert "#define BSK_FIT_SCHEDULE_WORDS 8" in header and "#define BSK_SCHED_LOG_COLS 8" in header and "#define BSK_PG_LOG_COLS 26" in header
    import ctypes as C
    assert C.sizeof(_lib.BskFitSchedule) == 80
    # refused before anything is launched: no device is needed to be told so
    assert lib.bsk_fit_set_schedule(None, None) == -1 and lib.bsk_fit_schedule_begin(None, None) == -1
    assert lib.bsk_fit_kl_gate(None, None, 1, None) == -1 and lib.bsk_fit_schedule_end(None, None, 0, None) == -1
    assert lib.bsk_fit_schedule_device(None, None) == -1 and lib.bsk_fit_get_schedule_state(None, None) == -1
    assert lib.bsk_fit_set_schedule_state(None, 0) == -1
    for name in ("set_schedule", "clear_schedule", "schedule_state", "set_schedule_state", "schedule_ptr", "schedule_begin", "kl_gate",
                 "schedule_end"):
        assert callable(getattr(P.PolicyFit, name)), name
    assert callable(P.PolicyGradient.schedule_log)
    # the Makefile builds the new file without contraction, and knows its header
    with open(os.path.join(ROOT, "basilisk_env_amd", "csrc", "Makefile")) as f:
        make = f.read()
    assert "bsk_pgsched.hip" in make and "bsk_pgsched.hpp" in make and "bsk_pgsched.o: CXXFLAGS += -ffp-contract=off" in make


def _hex(x):
    return "%016x" % int(np.array([x], np.float64).view(np.uint64)[0])


def test_the_device_functions_compiled_for_the_host_are_the_restatements(tmp_path):
    """csrc/bsk_pgsched.hpp's pg_sched_value, pg_kl_gate_sums and pg_kl_gate_apply as the kernels and the C-ABI run them, under the
    address and undefined-behaviour sanitizers of the host compiler - a stand-alone program, run as a child process: every value of
    the rule and every word the gate leaves equal the restatements', in every bit."""
    exe = tmp_path / "pg_sched_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DBSK_PGSCHED_HOST", "-I", os.path.join(ROOT, "basilisk_env_amd", "csrc"),
                           os.path.join(ROOT, "tools", "pg_sched_host.cpp"), "-o", str(exe)])
    rng = np.random.default_rng(77)
    sched = [c[:4] for c in SCHEDULE_CASES]
    for _ in range(200):                                       # ... and random ones about each branch
        total = int(rng.integers(0, 50))
        sched.append((int(rng.integers(0, 60)), total, float(rng.uniform(0, 1)), float(rng.uniform(0, 1))))
    lines = ["v %d %d %s %s" % (it, total, _hex(a), _hex(b)) for it, total, a, b in sched]
    for name, rows, stop, gate, skipped, at, _ in GATE_CASES:
        lines.append("g %s %d %d %s %d %s" % (_hex(stop), gate, skipped, _hex(at), rows.shape[0], " ".join(_hex(x) for x in rows.reshape(-1))))
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(sched) + len(GATE_CASES)
    for line, (it, total, a, b) in zip(got, sched):
        assert int(line, 16) == int(np.array([P.pg_schedule_ref(it, total, a, b)]).view(np.uint64)[0]), (it, total, a, b)
    for line, case in zip(got[len(sched):], GATE_CASES):
        name, rows, stop, gate, skipped, at, _ = case
        g, k, a, mean = P.fit_kl_gate_ref(rows, stop, gate, skipped, at)
        f = line.split()
        assert (int(f[0]), int(f[1]), int(f[3])) == (g, k, g), name
        assert int(f[2], 16) == int(np.array([a], np.float64).view(np.uint64)[0]), name
        S, N = (np.array([int(x, 16)], np.uint64).view(np.float64)[0] for x in f[4:6])
        with np.errstate(invalid="ignore", divide="ignore"):
            assert _same(np.float64(S / N), np.float64(mean)), name
