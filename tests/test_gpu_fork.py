"""GPU: forking spacecraft states on the device (bsk_fork_device / bsk_fork, csrc/bsk_fork.hip; contract in include/bskgpu.h).

A fork makes env j of one handle an exact copy of env map[j] of another (or the same) handle.  "Exact" is held bit for bit: a clone
stepped under its source's actions evolves exactly like the source - state, counters, observations, reward, reason, done bits,
terminal observations, episode counts and statistics - across kernel forms (pair / three-wave / single-wave, harmonics forms 4 and
5) and handles of different sizes.  Also: partial and in-handle maps, the host bookkeeping a fork must withdraw (static-charge
shortcut, stats seal), the auto-reset slot rule, the device path (no copy, no sync, HIP graph, two streams) and the refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from basilisk_env_amd import _hip
from basilisk_env_amd._lib import (DONE_BATTERY, FLAG_AUTO_RESET, FLAG_DESAT, FLAG_DRAG, FLAG_EPISODE_STATS, FLAG_OBS_ROWMAJOR, FLAG_POWER,
                                   FLAG_SUN_THIRD_BODY, GRAV_PM_J2, GRAV_SH, NF_BASE, T_CHARGE, BskError)
from basilisk_env_amd.envs.leoPowerAttitudeVecEnv import pool_slots
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
from helpers import visible_sh_coefficients

pytestmark = pytest.mark.gpu

SURFACE = FLAG_AUTO_RESET | FLAG_EPISODE_STATS | FLAG_OBS_ROWMAJOR
FULL = FLAG_POWER | FLAG_SUN_THIRD_BODY | FLAG_DRAG | FLAG_DESAT


def _upload(a):
    a = np.ascontiguousarray(a)
    b = _hip.DeviceBuffer(max(a.nbytes, 1), 0)
    _hip.check(_hip.runtime().hipMemcpyAsync(ctypes.c_void_p(b.ptr), ctypes.c_void_p(a.ctypes.data), a.nbytes, _hip.hipMemcpyHostToDevice,
                                             ctypes.c_void_p(0)), "hipMemcpyAsync")
    _hip.stream_sync(0)
    return b


def _download(ptr, dtype, count):
    out = np.empty(count, dtype=dtype)
    _hip.check(_hip.runtime().hipMemcpyAsync(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), out.nbytes, _hip.hipMemcpyDeviceToHost,
                                             ctypes.c_void_p(0)), "hipMemcpyAsync")
    _hip.stream_sync(0)
    return out


def _envs(p):
    """every per-env buffer of the handle, env index last (host arrays)"""
    p.sync()
    n = p.n_envs
    out = {"state": p.get_state()}
    out["steps"], out["ticks"] = p.get_counters()
    out["obs"], out["rew"], _, out["why"] = p.get_obs()
    v = p.device_views()
    mask = _download(v["done_mask"].__cuda_array_interface__["data"][0], np.uint64, (n + 63) // 64)
    j = np.arange(n)
    out["done_bit"] = (mask[j >> 6] >> (j & 63).astype(np.uint64)) & np.uint64(1)
    if "terminal_obs" in v:
        out["term_obs"], out["episodes"] = p.get_terminal_obs()
    for key, dt in (("episode_return", np.float64), ("terminal_return", np.float64), ("terminal_length", np.int32), ("done", np.uint8)):
        if key in v:
            out[key] = _download(v[key].__cuda_array_interface__["data"][0], dt, n)
    if "obs_rowmajor" in v:
        out["obs_rowmajor"] = _download(v["obs_rowmajor"].__cuda_array_interface__["data"][0], np.float64, 5 * n).reshape(n, 5).T
    return out


def _assert_clones(root, branch, idx, tag):
    """branch env j holds, bit for bit, what root env idx[j] holds (every buffer both have)"""
    a, b = _envs(root), _envs(branch)
    common = sorted(set(a) & set(b))
    assert {"state", "steps", "ticks", "obs", "rew", "why", "done_bit"} <= set(common)
    for key in common:
        assert np.array_equal(b[key], a[key][..., idx]), (tag, key)
    return common


def _pool_ic(n_rw, seed):
    return sample_ic_batch(41, n_rw, seed=seed)


def _clone_case(cfg, n_root, copies, k, monkeypatch, sh=None, root_env=None, branch_env=None, T=3):
    rng = np.random.default_rng(n_root + k)
    for kv in (root_env or {}).items():
        monkeypatch.setenv(*kv)
    root = BatchedPropagator(cfg, n_root)
    if sh:
        root.set_gravity_sh(*sh)
    for kv in (root_env or {}).items():
        monkeypatch.delenv(kv[0])
    for kv in (branch_env or {}).items():
        monkeypatch.setenv(*kv)
    branch = BatchedPropagator(cfg, n_root * copies)
    if sh:
        branch.set_gravity_sh(*sh)
    for kv in (branch_env or {}).items():
        monkeypatch.delenv(kv[0])
    pool = _pool_ic(cfg.n_rw, 7)
    for p in (root, branch):
        p.set_ic_pool(pool)
    root.reset(sample_ic_batch(n_root, cfg.n_rw, seed=11))
    # max_length 3: every episode ends at the 4th step and restarts from the pool (terminal observations, episode counts and
    # statistics are then non-trivial), and none ends during the T = 3 steps after the fork
    for _ in range(4):
        root.step(rng.integers(0, 3, n_root).astype(np.int32), k)
    assert (root.get_terminal_obs()[1] >= 1).all()
    idx = rng.permutation(np.repeat(np.arange(n_root), copies)).astype(np.int32)
    branch.fork_from(root, idx)
    _assert_clones(root, branch, idx, "fork")
    acts = rng.integers(0, 3, (T, n_root)).astype(np.int32)
    d_root, d_branch = _upload(acts), _upload(acts[:, idx])
    for t in range(T):
        root.step_device(d_root.ptr + 4 * n_root * t, k)
    branch.step_n(T, k, d_branch.ptr)
    keys = _assert_clones(root, branch, idx, "stepped")
    assert {"term_obs", "episodes", "episode_return", "terminal_return", "terminal_length", "done", "obs_rowmajor"} <= set(keys)
    names = root.kernel_info()["name"], branch.kernel_info()["name"]
    root.close()
    branch.close()
    return names


def test_clones_evolve_like_their_sources_bare_j2(monkeypatch):
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= SURFACE
    cfg.max_length = 3
    root, branch = _clone_case(cfg, 300, 3, 1, monkeypatch)
    assert root == "step_kernel<PM_J2,4,diag>" and branch.startswith("rollout_kernel<PM_J2,4,diag,actions>")


def test_clones_evolve_like_their_sources_power_pair_form(monkeypatch):
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= SURFACE | FLAG_POWER
    cfg.max_length = 3
    root, branch = _clone_case(cfg, 200, 5, 16, monkeypatch)
    assert root.endswith(",power,pair>") and branch.endswith(",power,pair>")


def test_clones_evolve_like_their_sources_full_scenario_across_forms(monkeypatch):
    """the small root runs the three-wave form, the branch (over 16 384 envs) the single-wave form: interchangeable mid-episode"""
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= SURFACE | FULL
    cfg.max_length = 3
    root, branch = _clone_case(cfg, 64, 300, 16, monkeypatch, T=2)
    assert root.endswith(",scenario,tri>") and branch.endswith(",scenario>")


@pytest.mark.parametrize("degree", [8, 70])
def test_clones_evolve_like_their_sources_harmonics_form4_to_form5(degree, monkeypatch):
    cfg = default_config(4, GRAV_SH)
    cfg.sh_degree = degree
    cfg.flags |= SURFACE
    cfg.max_length = 3
    cbar, sbar = visible_sh_coefficients(degree, seed=degree)
    root, branch = _clone_case(cfg, 70, 3, 3, monkeypatch, sh=(degree, cbar, sbar), root_env={"BSKGPU_SH_FORM": "4"},
                               branch_env={"BSKGPU_SH_FORM": "5"})
    assert "SH/dpp," in root and "SH/dpp2," in branch


def test_partial_map_leaves_unmapped_envs_alone():
    n = 200
    cfg = default_config(4, GRAV_PM_J2)
    root, dst = BatchedPropagator(cfg, n), BatchedPropagator(cfg, n)
    ic_r, ic_d = sample_ic_batch(n, 4, seed=1), sample_ic_batch(n, 4, seed=2)
    ic_r[12:16, ::3] = 400.0                      # wheels beyond their limit: done bits on both sides, at different envs
    ic_d[12:16, 1::4] = 400.0
    root.reset(ic_r)
    dst.reset(ic_d)
    root.step(np.zeros(n, np.int32), 2)
    dst.step(np.ones(n, np.int32), 2)
    before = _envs(dst)
    assert before["done_bit"].any() and not before["done_bit"].all()
    rng = np.random.default_rng(5)
    idx = rng.integers(0, n, n).astype(np.int32)
    idx[rng.random(n) < 0.4] = -1
    dst.fork_from(root, idx)
    after, src = _envs(dst), _envs(root)
    keep, m = idx < 0, idx >= 0
    for key in after:
        assert np.array_equal(after[key][..., keep], before[key][..., keep]), key
        assert np.array_equal(after[key][..., m], src[key][..., idx[m]]), key
    root.close()
    dst.close()


def test_in_handle_permutation_equals_a_host_gather():
    n = 333
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= SURFACE
    cfg.max_length = 2
    p = BatchedPropagator(cfg, n)
    p.set_ic_pool(_pool_ic(4, 3))
    p.reset(sample_ic_batch(n, 4, seed=4))
    rng = np.random.default_rng(9)
    for _ in range(4):
        p.step(rng.integers(0, 3, n).astype(np.int32), 3)
    before = _envs(p)
    rev = np.arange(n)[::-1].astype(np.int32)
    p.fork_from(p, rev)
    after = _envs(p)
    for key in after:
        assert np.array_equal(after[key], before[key][..., rev]), key
    # a second in-handle fork (the scratch exists now), overlapping: env j <- env (j + 1) mod n
    sh = ((np.arange(n) + 1) % n).astype(np.int32)
    p.fork_from(p, sh)
    again = _envs(p)
    for key in again:
        assert np.array_equal(again[key], after[key][..., sh]), key
    p.close()


def test_fork_withdraws_the_static_charge_shortcut():
    n, n_rw = 130, 3
    cfg = default_config(n_rw, GRAV_PM_J2)
    src, dst = BatchedPropagator(cfg, n), BatchedPropagator(cfg, n)
    ic = sample_ic_batch(n, n_rw, seed=22)
    dst.reset(ic)                                  # every charge > 0: the bare kernel may skip the battery test
    ic_s = ic.copy()
    ic_s[NF_BASE + n_rw + T_CHARGE, 17] = 0.0      # an empty battery at source env 17
    src.reset(ic_s)
    idx = np.full(n, -1, np.int32)
    idx[0] = 17
    dst.fork_from(src, idx)
    dst.step(np.zeros(n, np.int32), 3)
    obs, rew, done, why = dst.get_obs()
    assert why[0] & DONE_BATTERY and obs[3, 0] == 0.0 and not (why[1:] & DONE_BATTERY).any()
    src.close()
    dst.close()


def _stats_order(rew):
    """bsk_get_batch_stats' reward sum, operation for operation (csrc/bsk_aux.hip: stats_kernel + join)"""
    n = len(rew)
    nw = (n + 63) // 64
    v = np.zeros(nw * 64)
    v[:n] = rew
    v = v.reshape(nw, 64)
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, idx ^ off]
    slots = np.zeros(256)
    for w in range(nw):
        slots[w & 255] += v[w, 0]
    off = 128
    while off:
        slots[:off] += slots[off:2 * off]
        off >>= 1
    return float(slots[0])


def test_batch_stats_after_a_fork_describe_the_forked_buffers_even_after_a_sealing_reset():
    n = 500
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_AUTO_RESET
    cfg.max_length = 2
    src, dst = BatchedPropagator(cfg, n), BatchedPropagator(cfg, n)
    pool = _pool_ic(4, 5)
    for p in (src, dst):
        p.set_ic_pool(pool)
        p.reset(sample_ic_batch(n, 4, seed=6))
    for _ in range(3):
        src.step((np.arange(n) % 3).astype(np.int32), 2)    # the 3rd step ends every episode: rewards and done bits
    dst.step(np.zeros(n, np.int32), 2)
    dst.batch_stats()
    dst.reset_from_pool()                                    # seals dst's snapshot (the last step's scalars)
    idx = np.random.default_rng(1).integers(0, n, n).astype(np.int32)
    dst.fork_from(src, idx)
    s, d = dst.batch_stats()
    e = _envs(dst)
    assert d == int(e["done_bit"].sum()) > 0 and s == _stats_order(e["rew"]) and s != 0.0
    src.close()
    dst.close()


def test_forked_env_auto_resets_from_its_own_slot():
    n, nd = 96, 150
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_AUTO_RESET
    cfg.max_length = 2
    src, dst = BatchedPropagator(cfg, n), BatchedPropagator(cfg, nd)
    pool = _pool_ic(4, 8)
    for p in (src, dst):
        p.set_ic_pool(pool)
    dst.set_env_base(1000)
    src.reset(sample_ic_batch(n, 4, seed=9))
    for _ in range(4):                                       # one restart (3rd step), then one more step
        src.step(np.zeros(n, np.int32), 2)
    idx = np.random.default_rng(2).integers(0, n, nd).astype(np.int32)
    dst.fork_from(src, idx)
    eps = dst.get_terminal_obs()[1]
    assert np.array_equal(eps, src.get_terminal_obs()[1][idx]) and (eps >= 1).all()
    for _ in range(2):                                       # the 2nd of these ends every episode
        dst.step(np.zeros(nd, np.int32), 2)
    _, _, done, _ = dst.get_obs()
    assert done.all()
    st = dst.get_state()
    slots = pool_slots(1000 + np.arange(nd), eps, pool.shape[1])
    assert np.array_equal(st, pool[:, slots])
    src.close()
    dst.close()


def test_device_fork_issues_no_copy_and_no_sync():
    n = 256
    cfg = default_config(4, GRAV_PM_J2)
    src, dst = BatchedPropagator(cfg, n), BatchedPropagator(cfg, 3 * n)
    src.reset(sample_ic_batch(n, 4, seed=1))
    d_map = _upload((np.arange(3 * n) // 3).astype(np.int32))
    src.sync()
    c0 = BatchedPropagator.debug_counters()
    dst.fork_from(src, d_map.ptr)
    assert BatchedPropagator.debug_counters() == c0
    _assert_clones(src, dst, (np.arange(3 * n) // 3), "device map")
    src.close()
    dst.close()


def test_graph_of_fork_and_rollout_replays_like_eager_calls():
    import torch
    n, copies, T, k = 128, 4, 3, 5
    cfg = default_config(4, GRAV_PM_J2)
    side = torch.cuda.Stream()
    idx = np.random.default_rng(3).permutation(np.repeat(np.arange(n), copies)).astype(np.int32)
    acts = np.random.default_rng(4).integers(0, 3, (T, n * copies)).astype(np.int32)
    with torch.cuda.stream(side):
        root = BatchedPropagator(cfg, n, stream=side.cuda_stream)
        g_branch = BatchedPropagator(cfg, n * copies, stream=side.cuda_stream)
        e_branch = BatchedPropagator(cfg, n * copies, stream=side.cuda_stream)
        root.reset(sample_ic_batch(n, 4, seed=12))
        root.step(np.zeros(n, np.int32), k)
        t_map = torch.from_numpy(idx).to("cuda")
        t_act = torch.from_numpy(acts).to("cuda")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            g_branch.fork_from(root, t_map)
            g_branch.step_n(T, k, t_act.data_ptr())
        c0 = BatchedPropagator.debug_counters()
        graph.replay()
        graph.replay()                               # (a replay forks afresh: the same bits as one fork + rollout)
        assert BatchedPropagator.debug_counters() == c0
        torch.cuda.synchronize()
        e_branch.fork_from(root, t_map)
        e_branch.step_n(T, k, t_act.data_ptr())
        a, b = _envs(g_branch), _envs(e_branch)
        for key in a:
            assert np.array_equal(a[key], b[key]), key
        del graph
        for p in (root, g_branch, e_branch):
            p.close()


def test_fork_between_streams_equals_one_stream():
    n = 300
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_POWER
    src = BatchedPropagator(cfg, n)                                   # own stream
    other = BatchedPropagator(cfg, 2 * n)                             # own stream: the fork orders the two
    same = BatchedPropagator(cfg, 2 * n, stream=src.stream_ptr())     # src's stream
    src.reset(sample_ic_batch(n, 4, seed=13))
    idx = (np.arange(2 * n) % n).astype(np.int32)
    d_map = _upload(idx)
    act = (np.arange(n) % 3).astype(np.int32)
    src.step(act, 20)                       # queued on src's stream, not waited for: the fork must wait for it
    other.fork_from(src, d_map.ptr)
    same.fork_from(src, d_map.ptr)
    src.step(act, 20)                       # must not overwrite rows the fork on `other` still reads
    for p in (other, same):
        p.step(act[idx], 20)
    a, b = _envs(other), _envs(same)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    for p in (src, other, same):
        p.close()


def test_refusals():
    from basilisk_env_amd import _lib
    n = 64
    cfg = default_config(4, GRAV_PM_J2)
    a = BatchedPropagator(cfg, n)
    a.reset(sample_ic_batch(n, 4, seed=1))
    idx = np.arange(n, dtype=np.int32)
    cfg2 = default_config(4, GRAV_PM_J2)
    cfg2.dt = 0.05
    b = BatchedPropagator(cfg2, n)
    with pytest.raises(BskError) as e:
        b.fork_from(a, idx)
    assert e.value.code == -1 and "bsk_config" in str(e.value)
    c = BatchedPropagator(cfg, n)
    c.set_sim_time(60.0)
    with pytest.raises(BskError) as e:
        c.fork_from(a, idx)
    assert e.value.code == -1 and "sim_time" in str(e.value)
    # the flags that change outputs only are free to differ
    cfg3 = default_config(4, GRAV_PM_J2)
    cfg3.flags |= FLAG_EPISODE_STATS | FLAG_OBS_ROWMAJOR
    d = BatchedPropagator(cfg3, n)
    d.fork_from(a, idx)
    lib = _lib.load()
    assert lib.bsk_fork_device(d._handle(), a._handle(), None) == -1
    # harmonics: different coefficient sets
    cs = default_config(4, GRAV_SH)
    cs.sh_degree = 4
    c1, s1 = visible_sh_coefficients(4, seed=1)
    c2, s2 = visible_sh_coefficients(4, seed=2)
    h1, h2 = BatchedPropagator(cs, n), BatchedPropagator(cs, n)
    h1.set_gravity_sh(4, c1, s1)
    h2.set_gravity_sh(4, c2, s2)
    with pytest.raises(BskError) as e:
        h2.fork_from(h1, idx)
    assert e.value.code == -1 and "harmonic" in str(e.value)
    h2.set_gravity_sh(4, c1, s1)
    h2.fork_from(h1, idx)
    # an out-of-range entry: range-checked before use (the env is left alone), reported once by the next synchronising call
    before = _envs(d)
    bad = idx.copy()
    bad[5] = n + 1000
    d_bad = _upload(bad)
    d.fork_from(a, d_bad.ptr)
    with pytest.raises(BskError) as e:
        d.sync()
    assert e.value.code == -4 and "map entry" in str(e.value)
    d.sync()                                                        # once
    after = _envs(d)
    assert np.array_equal(after["state"][:, 5], before["state"][:, 5])
    for p in (a, b, c, d, h1, h2):
        p.close()


def test_c_program_forks_through_the_header_alone(tmp_path):
    """tests/c_abi/c_abi_fork.c: bsk_fork between two handles from plain C99; its printout equals the Python binding's"""
    from basilisk_env_amd import _lib
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "c_abi_fork"
    libdir = os.path.dirname(_lib.lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(root_dir, "include"),
                           os.path.join(root_dir, "tests", "c_abi", "c_abi_fork.c"), "-L", libdir, "-lbskgpu",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    n = 70
    ic = sample_ic_batch(n, 4, seed=47)
    ic_file = tmp_path / "ic.bin"
    ic.tofile(ic_file)
    got = subprocess.check_output([str(exe), str(ic_file), str(n)]).decode().split()
    cfg = default_config(4, GRAV_PM_J2)
    root, branch = BatchedPropagator(cfg, n), BatchedPropagator(cfg, 3 * n)
    root.reset(ic)
    root.step(np.zeros(n, np.int32), 7)
    branch.fork_from(root, (np.arange(3 * n) // 3).astype(np.int32))
    root.step(np.zeros(n, np.int32), 7)
    branch.step((np.arange(3 * n) % 3).astype(np.int32), 7)
    o, r, _, _ = root.get_obs()
    st = root.get_state()
    want = [o[0, 0], r[n - 1], st[9, 1]]
    ob, rb, _, _ = branch.get_obs()
    sb = branch.get_state()
    steps, ticks = branch.get_counters()
    rsum, ndone = branch.batch_stats()
    want += [ob[0, 0], ob[2, 4], rb[3 * n - 1], sb[9, 5]]
    assert [float(v) for v in got[:7]] == want
    assert [int(v) for v in got[7:9]] == [int(steps[3 * n - 1]), int(ticks[2])] and float(got[9]) == rsum and int(got[10]) == ndone
    root.close()
    branch.close()
