"""GPU: the shared-episode reset (bsk_reset_from_pool_shared; kernel in csrc/bsk_aux.hip; contract in include/bskgpu.h) and what
it is for - the members of a population scored on the same episodes.

Every check is an EQUALITY of bits: against the staged pool at the slots policy.shared_slot_ref names (held to the header's formula
in Python integers by tests/test_es_adam_host.py), against a host reset from those same initial conditions on a second handle, and
between envs that share a slot.  Shapes: (256, 64, 0) is whole members in one 256-thread workgroup; (200, 48, 70) has members that
straddle waves, an n that E does not divide, a last workgroup that is not full and a shard offset that is no multiple of E;
(256, 64, 128) a shard that starts at a member boundary; (700, 192, 5) is three workgroups, the last one partial, with an E that is no
power of two, and (700, 192, 2^32 - 300) puts the wrap of the 32-bit global index env_base + env inside the batch: envs 300 .. 699
count on from 0, and 2^32 is no multiple of 192.  Epoch 2^32 + 3 catches a read of the high word.
"""
import ctypes

import numpy as np
import pytest

from _device_bits import download as _download, same as _same
from _policy_bounds import seeded_policy
from basilisk_env_amd import _hip, _lib
from basilisk_env_amd import policy as P
from basilisk_env_amd._lib import FLAG_AUTO_RESET, FLAG_EPISODE_STATS, FLAG_OBS_ROWMAJOR, GRAV_PM_J2
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch

pytestmark = pytest.mark.gpu

N_POOL = 41
EPOCHS = (0, 1, 2 ** 32 + 3)


def _envs(p):
    """every per-env buffer of the handle, env index last (host arrays)"""
    p.sync()
    n = p.n_envs
    out = {"state": p.get_state()}
    out["steps"], out["ticks"] = p.get_counters()
    out["obs"], out["rew"], _, out["why"] = p.get_obs()
    v = p.device_views()
    if "terminal_obs" in v:                                   # (a pool is staged)
        out["term_obs"], out["episodes"] = p.get_terminal_obs()
    mask = _download(v["done_mask"].__cuda_array_interface__["data"][0], np.uint64, (n + 63) // 64)
    j = np.arange(n)
    out["done_bit"] = (mask[j >> 6] >> (j & 63).astype(np.uint64)) & np.uint64(1)
    for key, dt in (("episode_return", np.float64), ("terminal_return", np.float64), ("terminal_length", np.int32), ("done", np.uint8)):
        out[key] = _download(v[key].__cuda_array_interface__["data"][0], dt, n)
    out["obs_rowmajor"] = _download(v["obs_rowmajor"].__cuda_array_interface__["data"][0], np.float64, 5 * n).reshape(n, 5).T
    return out


RESET_WRITES = ("obs", "rew", "why", "done", "episode_return", "obs_rowmajor")


def _config(max_length=None):
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_AUTO_RESET | FLAG_EPISODE_STATS | FLAG_OBS_ROWMAJOR
    if max_length:
        cfg.max_length = max_length
    return cfg


@pytest.fixture(scope="module")
def pool():
    p = sample_ic_batch(N_POOL, 4, seed=15)
    p.setflags(write=False)
    return p


def _stepped(cfg, n, env_base, pool, ic):
    p = BatchedPropagator(cfg, n)
    p.set_env_base(env_base)
    p.set_ic_pool(pool)
    p.reset(ic)
    p.step((np.arange(n) % 3).astype(np.int32), 2)
    return p


@pytest.mark.parametrize("n,E,env_base", [(256, 64, 0), (200, 48, 70), (256, 64, 128), (700, 192, 5), (700, 192, 2 ** 32 - 300)])
def test_the_shared_reset_is_the_definition(n, E, env_base, pool):
    import torch
    cfg = _config()
    ic = sample_ic_batch(n, 4, seed=n + env_base)
    a, b = _stepped(cfg, n, env_base, pool, ic), _stepped(cfg, n, 0, pool, ic)
    assert _same(a.get_ic_pool(), pool)
    actions = ((np.arange(n) + 1) % 3).astype(np.int32)
    rng = np.random.default_rng(n + E)
    for epoch in EPOCHS:
        word = torch.tensor([epoch], dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        a.step(actions, 2)
        before = _envs(a)
        assert before["rew"].any() and before["episode_return"].any() and before["steps"].all()
        c0 = BatchedPropagator.debug_counters()
        a.reset_from_pool_shared(E, word.data_ptr())
        assert BatchedPropagator.debug_counters() == c0            # enqueue-only: no copy, no synchronisation
        after = _envs(a)
        slots = P.shared_slot_ref(n, E, epoch, N_POOL, env_base)
        want = pool[:, slots]
        assert _same(after["state"], want), epoch
        assert not after["steps"].any() and not after["ticks"].any()
        assert np.array_equal(after["episodes"], before["episodes"] + 1)
        # what a host reset from those same initial conditions leaves on a second handle (which had stepped, too)
        b.step(actions, 2)
        b.reset(want)
        host = _envs(b)
        for key in RESET_WRITES:
            assert _same(after[key], host[key]), (epoch, key)
        assert not after["rew"].any() and not after["why"].any() and not after["done"].any() and not after["episode_return"].any()
        # equal q, equal initial condition - and one member's envs are not all alike
        q = (np.arange(n) + env_base) % 2 ** 32 % E
        first = np.array([np.flatnonzero(q == x)[0] for x in q])
        assert _same(after["state"], after["state"][:, first]) and _same(after["obs"], after["obs"][:, first])
        assert len({after["state"][0, j] for j in range(E)}) > 20

        # under a device mask the unmasked envs keep every buffer's bits; the epoch word is read when the kernel runs
        a.step(actions, 2)
        before = _envs(a)
        mask = (rng.uniform(size=n) < 0.4).astype(np.uint8)
        d_mask = torch.from_numpy(mask).cuda()
        word += 1
        torch.cuda.synchronize()
        c0 = BatchedPropagator.debug_counters()
        a.reset_from_pool_shared(E, word.data_ptr(), d_mask.data_ptr())
        assert BatchedPropagator.debug_counters() == c0
        after = _envs(a)
        keep, hit = mask == 0, mask != 0
        assert keep.any() and hit.any()
        for key in before:
            assert _same(after[key][..., keep], before[key][..., keep]), (epoch, key)
        slots = P.shared_slot_ref(n, E, epoch + 1, N_POOL, env_base)
        assert _same(after["state"][:, hit], pool[:, slots][:, hit])
        assert np.array_equal(after["episodes"][hit], before["episodes"][hit] + 1) and not after["steps"][hit].any()
    # no epoch word: epoch 0
    a.reset_from_pool_shared(E)
    assert _same(_envs(a)["state"], pool[:, P.shared_slot_ref(n, E, 0, N_POOL, env_base)])
    a.close()
    b.close()


def test_identical_members_score_identically_on_shared_episodes(pool):
    """The test that fails without the feature: P identical members report P different fitness values after the plain reset,
    whose slot rule hashes the global env index - and the same value, env for env, after the shared one."""
    n_members, E, T, k, gamma = 4, 64, 8, 1, 0.99
    n = n_members * E
    spec, theta = seeded_policy((16,), "relu", None, seed=5)
    prop = _stepped(_config(max_length=6), n, 0, pool, sample_ic_batch(n, 4, seed=29))
    pop = P.PolicyPopulation(spec, np.tile(theta, (n_members, 1)))
    assert all(_same(pop.member(m), theta) for m in range(n_members))
    j = np.arange(n)
    for epoch in (None, 5):
        word = _hip.DeviceBuffer(8, 0)
        if epoch is not None:
            e = np.array([epoch], np.uint64)
            _hip.check(_hip.runtime().hipMemcpy(ctypes.c_void_p(word.ptr), ctypes.c_void_p(e.ctypes.data), 8, _hip.hipMemcpyHostToDevice), "hipMemcpy")
        prop.reset_from_pool_shared(E, None if epoch is None else word.ptr)
        out = pop.evaluate(prop, T, k, "greedy", gamma)
        word.free()
        assert _same(out["env_value"], out["env_value"][j % E]) and _same(out["env_len"], out["env_len"][j % E]), epoch
        # (a member's own envs are not all scored alike: the equality above is not that of a constant)
        assert len(set(out["env_value"][:E].tolist())) >= 2 and np.isfinite(out["env_value"]).all()
        assert (out["env_len"] >= 1).all() and (out["env_len"] <= T).all()
        for key in ("fitness", "mean_len"):
            assert out[key].shape == (n_members,) and _same(out[key], np.repeat(out[key][:1], n_members)), (epoch, key)
    # the test's own inputs: the same members after the plain reset are scored on other episodes (seed 5 does; no other tried)
    prop.reset_from_pool_device(None)
    plain = pop.evaluate(prop, T, k, "greedy", gamma)
    assert len(set(plain["fitness"].tolist())) >= 2
    assert not _same(plain["env_value"], plain["env_value"][j % E])
    prop.close()
    pop.close()


def test_refusals_come_before_any_launch(pool):
    import torch
    lib = _lib.load()
    n = 128
    ic = sample_ic_batch(n, 4, seed=3)
    staged = _stepped(_config(), n, 0, pool, ic)
    bare = BatchedPropagator(_config(), n)                    # auto-reset, but no pool staged (it cannot step either)
    bare.reset(ic)
    word = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    before = [_envs(staged), _envs(bare)]
    c0 = BatchedPropagator.debug_counters()
    for h, E, what in ((None, 64, b"NULL"), (bare._handle(), 64, b"pool"), (staged._handle(), 0, b"envs_per_member"),
                       (staged._handle(), -1, b"envs_per_member"), (staged._handle(), -2 ** 31, b"envs_per_member")):
        assert lib.bsk_reset_from_pool_shared(h, E, word.data_ptr(), None) == -1, (E, what)
        assert what in lib.bsk_last_error()
    assert BatchedPropagator.debug_counters() == c0
    with pytest.raises(_lib.BskError):
        staged.reset_from_pool_shared(0)
    for p, was in zip((staged, bare), before):
        now = _envs(p)
        for key in was:
            assert _same(now[key], was[key]), key
    # ... and the same call with legal arguments does run: one env per member, more envs per member than envs
    for E in (1, n + 7, 2 ** 31 - 1):
        staged.reset_from_pool_shared(E, word.data_ptr())
        assert _same(_envs(staged)["state"], pool[:, P.shared_slot_ref(n, E, 0, N_POOL)]), E
    staged.close()
    bare.close()
