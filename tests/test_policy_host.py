"""CPU: the policy's numpy restatements (basilisk_env_amd/policy.py) and the device-free part of its C-ABI.

``fma32`` is checked against exact rational arithmetic; the f32 chain against its own fp64 variant within the derived bound
(tests/_policy_bounds.py); sampling against the probabilities it is meant to realise; the C-ABI's spec rules against the Python ones.
"""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

from _policy_bounds import mlp_bound, observation_like, seeded_policy, softmax_bound
from basilisk_env_amd import _lib
from basilisk_env_amd import policy as P


def _round_f32(x):
    """An exact Fraction -> the nearest float32, ties to even (nothing but comparisons of exact numbers)."""
    if x == 0:
        return np.float32(0.0)
    c = np.float32(float(x))                       # (double rounding may be one step off: the neighbours are compared below)
    cands = {c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))}
    best = None
    for f in cands:
        if not np.isfinite(f):
            continue
        dist = abs(Fraction(float(f)) - x)
        even = (int(np.float32(f).view(np.int32)) & 1) == 0
        if best is None or dist < best[0] or (dist == best[0] and even and not best[2]):
            best = (dist, f, even)
    return best[1]


def test_fma32_equals_exact_rational_arithmetic():
    rng = np.random.default_rng(7)
    n = 4000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(np.float32)
    # cancellation: c is minus the ROUNDED product, so that the result is the product's rounding error alone
    a2, b2 = a[:600], b[:600]
    c2 = -(a2 * b2)
    # ties: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 lies exactly between two floats; c = 0 keeps the tie, a tiny c of either sign breaks it
    t = np.float32(1.0 + 2.0 ** -12)
    ties_a = np.array([t, t, t, -t, -t, t, np.float32(3.0), np.float32(3.0)], np.float32)
    ties_b = np.array([t, t, t, t, t, t, np.float32(1.0 + 2.0 ** -23), np.float32(1.0 + 2.0 ** -23)], np.float32)
    ties_c = np.array([0.0, 2.0 ** -60, -2.0 ** -60, 0.0, 2.0 ** -60, 1.0, 0.0, 2.0 ** -40], np.float32)
    A, B, Cc = np.concatenate([a, a2, ties_a]), np.concatenate([b, b2, ties_b]), np.concatenate([c, c2, ties_c])
    got = P.fma32(A, B, Cc)
    assert got.dtype == np.float32
    bad = 0
    for k in range(A.size):
        want = _round_f32(Fraction(float(A[k])) * Fraction(float(B[k])) + Fraction(float(Cc[k])))
        bad += int(want != got[k] or np.signbit(want) != np.signbit(got[k]) and want != 0)
    assert bad == 0
    # it is NOT what two roundings give: the cancellation cases come out as the product's error, not as zero
    assert np.count_nonzero(got[n:n + 600]) > 500 and np.count_nonzero(a2 * b2 + c2) == 0


@pytest.mark.parametrize("hidden,act,vh", [((), "relu", None), ((16,), "relu", (16,)), ((64, 64), "relu", (64, 64)),
                                           ((64, 64), "tanh", (64, 64)), ((48, 112), "tanh", None), ((128, 128, 128), "relu", None)])
def test_f32_chain_is_within_the_derived_bound_of_fp64(hidden, act, vh):
    spec, params = seeded_policy(hidden, act, vh, seed=1)
    obs = observation_like(777, seed=1)
    l32, v32 = P.mlp_ref(spec, params, obs)
    l64, v64 = P.mlp_ref(spec, params, obs, fp64=True)
    bl, el, bv, ev = mlp_bound(spec, params, obs)
    assert l32.dtype == np.float32 and l32.shape == (3, 777) and np.array_equal(l64, bl)
    assert np.all(np.abs(l32.astype(np.float64) - l64) <= el)
    print("logits: max error / bound = %.3f, max bound %.3g" % (np.max(np.abs(l32 - l64) / el), el.max()))
    if vh is None:
        assert v32 is None and v64 is None and bv is None
    else:
        assert v32.shape == (777,) and np.all(np.abs(v32.astype(np.float64) - v64) <= ev)


def test_from_torch_layers_agree_with_torch_forward():
    torch = pytest.importorskip("torch")
    nn = torch.nn
    torch.manual_seed(5)
    for act, Act in (("relu", nn.ReLU), ("tanh", nn.Tanh)):
        net = nn.Sequential(nn.Linear(5, 64), Act(), nn.Linear(64, 32), Act(), nn.Linear(32, 3))
        val = nn.Sequential(nn.Linear(5, 16), Act(), nn.Linear(16, 1))
        hidden, a, layers = P.torch_layers(net)
        vh, va, vlayers = P.torch_layers(val)
        assert (hidden, a, vh, va) == ((64, 32), act, (16,), act)
        spec = P.check_spec(hidden, a, vh, va)
        params = P.pack_params(spec, layers, vlayers)
        obs = observation_like(500, seed=2)
        with torch.no_grad():
            x = torch.from_numpy(obs.T.astype(np.float32))
            tl, tvv = net(x).numpy().T.astype(np.float64), val(x).numpy()[:, 0].astype(np.float64)
        l64, el, v64, ev = mlp_bound(spec, params, obs)       # (the bound holds for any summation order: torch's too)
        assert np.all(np.abs(tl - l64) <= el) and np.all(np.abs(tvv - v64) <= ev)
        l32, v32 = P.mlp_ref(spec, params, obs)
        assert np.all(np.abs(l32 - l64) <= el) and np.all(np.abs(v32 - v64) <= ev)
    for bad in (nn.Linear(5, 3), nn.Sequential(), nn.Sequential(nn.Linear(5, 16), nn.Sigmoid(), nn.Linear(16, 3)),
                nn.Sequential(nn.Linear(5, 16), nn.ReLU()), nn.Sequential(nn.ReLU(), nn.Linear(5, 3)),
                nn.Sequential(nn.Linear(5, 16), nn.ReLU(), nn.Linear(16, 16), nn.Tanh(), nn.Linear(16, 3)),
                nn.Sequential(nn.Linear(5, 16), nn.Linear(16, 3))):
        with pytest.raises(ValueError):
            P.torch_layers(bad)
    with pytest.raises(ValueError):                 # 5 inputs and 3 outputs are the policy's, whatever the module says
        h, a, layers = P.torch_layers(nn.Sequential(nn.Linear(4, 16), nn.ReLU(), nn.Linear(16, 3)))
        P.pack_params(P.check_spec(h, a), layers)


def test_pack_params_layout_and_spec_rules():
    spec = P.check_spec((16, 32), "relu", (16,), "tanh")
    a, v = P.layer_shapes(spec)
    assert a == [(16, 5), (32, 16), (3, 32)] and v == [(16, 5), (1, 16)]
    assert P.n_params(spec) == 10 + (80 + 16) + (512 + 32) + (96 + 3) + (80 + 16) + (16 + 1)
    k = [0]

    def layer(o, i):
        W = np.arange(k[0], k[0] + o * i, dtype=np.float32).reshape(o, i)
        b = np.arange(k[0] + o * i, k[0] + o * i + o, dtype=np.float32)
        k[0] += o * i + o
        return W, b
    layers, vlayers = [layer(o, i) for o, i in a], [layer(o, i) for o, i in v]
    p = P.pack_params(spec, layers, vlayers, in_scale=[1, 2, 3, 4, 5], in_shift=[-1, -2, -3, -4, -5])
    assert p.dtype == np.float32 and p.size == P.n_params(spec)
    assert np.array_equal(p[:10], [1, 2, 3, 4, 5, -1, -2, -3, -4, -5])
    assert np.array_equal(p[10:], np.arange(p.size - 10))          # W[out][in] row-major, then b, layer after layer, value net last
    sc, sh, la, lv = P.unpack_params(spec, p)
    assert np.array_equal(la[1][0], layers[1][0]) and np.array_equal(lv[1][1], vlayers[1][1]) and sc[4] == 5 and sh[0] == -1
    assert np.array_equal(P.pack_params(P.check_spec(()), [layer(3, 5)])[:10], [1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
    for args in (((8,),), ((144,),), ((24,),), ((16, 16, 16, 16),), ((16,), "gelu"), ((16,), "relu", (20,)), ((16,), "relu", (16,), "elu"),
                 ((16,), "relu", None, "tanh"), ((16.0,),)):
        with pytest.raises(ValueError):
            P.check_spec(*args)
    with pytest.raises(ValueError):
        P.pack_params(spec, layers)                                # the value network's layers are missing
    with pytest.raises(ValueError):
        P.pack_params(spec, layers[:2], vlayers)
    with pytest.raises(ValueError):
        P.pack_params(spec, [(W.T, b) for W, b in layers], vlayers)
    with pytest.raises(ValueError):
        P.unpack_params(spec, p[:-1])


def test_greedy_rule_ties_and_nans():
    nan = np.nan
    l = np.array([[1, 2, 2, nan, nan, nan, 0, -np.inf, 3, nan],
                  [2, 2, 1, 1, nan, nan, 0, -np.inf, nan, 5],
                  [2, 2, 2, nan, 0, nan, 0, -np.inf, 3, 5]], np.float32)
    a, _ = P.act_ref(l, "greedy")
    assert a.tolist() == [1, 0, 0, 1, 2, 0, 0, 0, 0, 1]


def test_sampling_realises_the_probabilities():
    n = 1 << 20
    logits = np.tile(np.array([[0.3], [-0.9], [1.1]], np.float32), (1, n))
    p0, c1, logp, delta, e_logp = softmax_bound(logits[:, :1])
    probs = np.array([p0[0], c1[0] - p0[0], 1.0 - c1[0]])
    a, lp = P.act_ref(logits, "sample", seed=12345, draw=0)
    assert a.dtype == np.int32 and a.min() >= 0 and a.max() <= 2
    counts = np.bincount(a, minlength=3)
    sigma = np.sqrt(n * probs * (1 - probs))
    print("sampled frequencies", counts / n, "probabilities", probs, "deviation / sigma", (counts - n * probs) / sigma)
    assert np.all(np.abs(counts - n * probs) <= 5 * sigma)
    assert np.all(np.abs(lp.astype(np.float64) - logp[a, 0]) <= e_logp[a, 0])
    a_again, _ = P.act_ref(logits, "sample", seed=12345, draw=0)
    assert np.array_equal(a, a_again)                              # a function of (seed, env, draw) alone
    a_next, _ = P.act_ref(logits, "sample", seed=12345, draw=1)
    a_seed, _ = P.act_ref(logits, "sample", seed=12346, draw=0)
    assert 0.3 < np.mean(a != a_next) < 0.8 and 0.3 < np.mean(a != a_seed) < 0.8
    # env j of a batch that starts at env_base equals env 0 of a batch that starts at env_base + j, 64-bit indices included
    for base in (0, 77, (1 << 32) - 3, (1 << 40) + 5):
        u = P.sample_uniform(8, seed=9, draw=(1 << 33) + 2, env_base=base)
        for j in range(8):
            assert u[j] == P.sample_uniform(1, seed=9, draw=(1 << 33) + 2, env_base=base + j)[0]
        assert u.dtype == np.float32 and np.all((u >= 0) & (u < 1))
    # the generator is the library's one Philox (tests/_philox_ref.py restates the IC sampler's use of it)
    from _philox_ref import philox4x32_10
    w = P.philox4x32_10([5], [0], [7], [1], [0xDEADBEEF], [0x12345678])
    assert tuple(int(x[0]) for x in w) == philox4x32_10(5, 0, 7, 1, 0xDEADBEEF, 0x12345678)


def test_policy_abi_without_a_device():
    lib = _lib.load()
    for hidden, vh in (((), None), ((16,), None), ((64, 64), (64, 64)), ((128, 128, 128), (128, 128, 128)), ((48, 112), (16,))):
        spec = P.check_spec(hidden, "relu", vh)
        cs = P.c_spec(spec)
        assert lib.bsk_policy_n_params(ctypes.byref(cs)) == P.n_params(spec)
    assert P.n_params(P.check_spec((64, 64))) == 10 + 5 * 64 + 64 + 64 * 64 + 64 + 64 * 3 + 3

    def broken(**kw):
        cs = P.c_spec(P.check_spec((32, 32), "tanh", (32,)))
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(cs, k)[v[0]] = v[1]
            else:
                setattr(cs, k, v)
        return cs
    params = np.zeros(100000, np.float32)
    out = ctypes.c_void_p()
    for kw in ({"n_hidden": 4}, {"n_hidden": -1}, {"hidden": (0, 8)}, {"hidden": (1, 136)}, {"hidden": (1, 40)}, {"activation": 2},
               {"has_value": 2}, {"v_n_hidden": 4}, {"v_hidden": (0, 15)}, {"v_activation": -1}):
        cs = broken(**kw)
        assert lib.bsk_policy_n_params(ctypes.byref(cs)) == -1, kw
        assert lib.bsk_last_error().startswith(b"bsk_policy_spec")
        assert lib.bsk_policy_create(ctypes.byref(cs), params.ctypes.data, 0, ctypes.byref(out)) == -1 and not out.value
    assert lib.bsk_policy_n_params(ctypes.byref(broken(struct_size=8))) == -5
    assert lib.bsk_policy_n_params(ctypes.byref(broken(abi_version=1))) == -5
    assert lib.bsk_policy_n_params(None) == -1
    good = broken()
    assert lib.bsk_policy_create(ctypes.byref(good), None, 0, ctypes.byref(out)) == -1
    assert lib.bsk_policy_create(ctypes.byref(good), params.ctypes.data, 0, None) == -1
    # every entry point refuses a NULL policy before it touches a device
    assert lib.bsk_policy_set_params(None, params.ctypes.data) == -1 and lib.bsk_policy_set_rng(None, 1, 0) == -1
    assert lib.bsk_policy_get_rng(None, None, None) == -1
    assert lib.bsk_policy_act(None, None, 0, 1, 0, 0, None, None, None, None, 0, None) == -1
    assert lib.bsk_policy_rollout(None, None, 0, 1, 1, None, None, None, None, None, None) == -1
    lib.bsk_policy_destroy(None)
    if not os.path.exists("/dev/kfd"):
        # a legal spec on a box without a GPU: no device, said loudly (the rule of test_product_fails_loudly_without_gpu)
        assert lib.bsk_policy_create(ctypes.byref(good), params.ctypes.data, 0, ctypes.byref(out)) == -2 and not out.value
        with pytest.raises(_lib.BskGpuUnavailable):
            P.DevicePolicy(P.check_spec((32, 32), "tanh", (32,)), params[:P.n_params(P.check_spec((32, 32), "tanh", (32,)))])
