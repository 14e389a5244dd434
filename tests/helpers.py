"""Shared helpers for the parity tests."""
import numpy as np


def field_groups(n_rw):
    g = {"r": slice(0, 3), "v": slice(3, 6), "sigma": slice(6, 9), "omega": slice(9, 12)}
    if n_rw:
        g["Omega"] = slice(12, 12 + n_rw)
        g["u"] = slice(12 + n_rw + 3, 12 + n_rw + 3 + n_rw)
        g["u_pend"] = slice(12 + n_rw + 26, 12 + n_rw + 26 + n_rw)
        g["sigma_BR_msg"] = slice(12 + n_rw + 30, 12 + n_rw + 31)
    return g


def rel_err(a, b, sl):
    """max |a-b| over the group, relative to the group's largest magnitude in b."""
    return float(np.abs(a[sl] - b[sl]).max() / max(np.abs(b[sl]).max(), 1e-300))


def max_group_err(a, b, n_rw):
    return {k: rel_err(a, b, sl) for k, sl in field_groups(n_rw).items()}


def cfg_for_case(case):
    """bsk_config of a golden case (tests/golden/make_golden.py: the recipes' cfg_edit functions)."""
    from basilisk_env_amd._lib import FLAG_DRAG, FLAG_POWER, FLAG_SUN_THIRD_BODY
    from basilisk_env_amd.simulators.dynamics.config import default_config
    cfg = default_config(case["n_rw"], case["gravity_model"])
    if case.get("cfg_edit") == "scenario_edit":
        cfg.flags |= FLAG_POWER | FLAG_SUN_THIRD_BODY | FLAG_DRAG
        cfg.base_density, cfg.scale_height = 1e-9, 100e3
    if case.get("cfg_edit") == "dense_drag_edit":
        cfg.flags |= FLAG_POWER | FLAG_SUN_THIRD_BODY | FLAG_DRAG
        cfg.dt = 1.0
        cfg.base_density, cfg.scale_height = 1e-4, 20e3
    if case.get("cfg_edit") == "desat_edit":
        from basilisk_env_amd._lib import FLAG_DESAT
        cfg.flags |= FLAG_POWER | FLAG_SUN_THIRD_BODY | FLAG_DRAG | FLAG_DESAT
    if case.get("cfg_edit") == "full_inertia_edit":
        cfg.flags |= FLAG_POWER | FLAG_SUN_THIRD_BODY | FLAG_DRAG
        cfg.base_density, cfg.scale_height = 1e-9, 100e3
        general_hub(cfg)
    if case.get("cfg_edit") == "nolag_edit":
        cfg.fsw_lag = 0
        cfg.nav_lag = 0
    if case.get("cfg_edit") == "navnow_edit":
        cfg.nav_lag = 0
    if "sh_degree" in case:
        cfg.sh_degree = case["sh_degree"]
    return cfg


def general_hub(cfg, rng=None, inertia=True, tilt=True):
    """Edit ``cfg`` so that the step kernels with a GENERAL inertia matrix run (``DIAG = false``: csrc/bsk_config.hip selects
    them whenever an off-diagonal of I_sc or of I_sc - sum Js g g^T is non-zero).  ``inertia``: a symmetric positive-definite
    I_sc with products of inertia of 1 - 20 % of the smallest diagonal entry (the reference's hub is the diagonal cuboid of
    leoPowerAttitudeSimulator.py:244-249: this is surface beyond it that the ABI accepts).  ``tilt``: one wheel's spin axis
    rotated by 3 - 15 degrees (I_sc - sum Js g g^T then has off-diagonals even with a diagonal hub).  ``rng`` None: fixed
    values (the golden case ``full_inertia_rw4``)."""
    d = min(cfg.inertia[0], cfg.inertia[4], cfg.inertia[8])
    if inertia:
        if rng is None:
            pxy, pxz, pyz = 0.075 * d, -0.055 * d, 0.11 * d
        else:
            pxy, pxz, pyz = (float(rng.uniform(0.01, 0.2) * rng.choice([-1.0, 1.0]) * d) for _ in range(3))
        cfg.inertia[1] = cfg.inertia[3] = pxy
        cfg.inertia[2] = cfg.inertia[6] = pxz
        cfg.inertia[5] = cfg.inertia[7] = pyz
        assert np.all(np.linalg.eigvalsh(np.array(list(cfg.inertia)).reshape(3, 3)) > 0.0)
    if tilt and cfg.n_rw:
        w = 1 if rng is None else int(rng.integers(0, cfg.n_rw))
        ang = np.deg2rad(9.0) if rng is None else float(rng.uniform(np.deg2rad(3.0), np.deg2rad(15.0)))
        g = np.array([cfg.gs[w][k] for k in range(3)])
        axis = np.cross(g, [0.3, -0.5, 0.8] if rng is None else rng.normal(size=3))
        axis /= np.linalg.norm(axis)
        g2 = g * np.cos(ang) + np.cross(axis, g) * np.sin(ang)
        g2 /= np.linalg.norm(g2)
        for k in range(3):
            cfg.gs[w][k] = float(g2[k])
    return cfg


def visible_sh_coefficients(degree, r0=6.9e6, harmonic_fraction=2e-3, seed=0):
    """Normalised C/S up to ``degree`` in which every degree adds about the same acceleration at radius ``r0``, so that
    an error confined to the high degrees is visible in the state (tests only; the benchmark field is
    ``gravity_sh.synthetic_sh_coefficients``, whose Kaula-rule terms at degree 70 move the state by ~1e-12).

    C00 = 1, degree 1 zero, C_lm and S_lm (S_l0 = 0) from N(0, sigma_l^2) with
    sigma_l = p (r0/Re)^l / ((l+1) sqrt(2l+1)): the (l+1) undoes the gradient's factor, sqrt(2l+1) the number of
    terms of a degree.  p is scaled so that the harmonic part |a - a_point_mass| is about ``harmonic_fraction`` of |a| at
    r0 (p = 3e-5 gives ~3e-4 at degree 70; the degrees add in quadrature)."""
    from basilisk_env_amd.simulators.dynamics.config import REQ_EARTH_KM
    from basilisk_env_amd.simulators.dynamics.gravity_sh import sh_index, sh_size
    rng = np.random.Generator(np.random.PCG64(seed))
    p = 3e-5 * (harmonic_fraction / 3e-4) * np.sqrt(69.0 / max(degree - 1, 1))
    q = r0 / (REQ_EARTH_KM * 1000.0)
    c = np.zeros(sh_size(degree))
    s = np.zeros(sh_size(degree))
    c[sh_index(0, 0)] = 1.0
    for l in range(2, degree + 1):
        sig = p * q ** l / ((l + 1) * np.sqrt(2 * l + 1))
        for m in range(l + 1):
            c[sh_index(l, m)] = rng.normal(0.0, sig)
            s[sh_index(l, m)] = rng.normal(0.0, sig) if m > 0 else 0.0
    return c, s


def visible_states(n, n_rw, r0=6.9e6, seed=0, mu=None):
    """``sample_ic_batch`` ICs with every |r| rescaled to ``r0`` and v set to the circular speed there (same direction
    of motion, v perpendicular to r): the radius at which ``visible_sh_coefficients`` balances its degrees."""
    from basilisk_env_amd.simulators.dynamics.config import MU_EARTH
    from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
    mu = MU_EARTH if mu is None else mu
    ic = sample_ic_batch(n, n_rw, seed=seed)
    r, v = ic[0:3], ic[3:6]
    r = r * (r0 / np.linalg.norm(r, axis=0))
    rhat = r / r0
    v = v - (v * rhat).sum(0) * rhat
    v = v * (np.sqrt(mu / r0) / np.linalg.norm(v, axis=0))
    ic[0:3], ic[3:6] = r, v
    return np.ascontiguousarray(ic)


def load_sh70_fixture():
    """tests/golden/sh70_field.json (written by tests/golden/make_sh70_golden.py): the degree-70 field, planet-fixed
    accelerations at ``pos`` (N, 3) -> ``acc`` (N, 3), and spacecraft ``r``, ``v`` (3, N) with their translational
    state after 1 and after 10 RK4 ticks, ``after[k]`` (6, N), starting at tick ``tick0``."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sh70_field.json")) as fh:
        doc = json.load(fh)
    sc = doc["spacecraft"]
    doc["cbar"], doc["sbar"] = np.array(doc["cbar"]), np.array(doc["sbar"])
    doc["pos"] = np.array([p["r"] for p in doc["positions"]])
    doc["acc"] = np.array([[float(v) for v in p["a"]] for p in doc["positions"]])
    doc["r"] = np.array([s["r"] for s in sc]).T.copy()
    doc["v"] = np.array([s["v"] for s in sc]).T.copy()
    doc["after"] = {int(k): np.array([[float(v) for v in s["after_ticks"][k]] for s in sc]).T.copy() for k in ("1", "10")}
    return doc


def create_each(device_id, hidden=(16,), n_members=2, n_envs=64):
    """``bsk_create``, ``bsk_policy_create``, ``bsk_population_create`` and ``bsk_es_create`` with valid arguments on ``device_id``
    -> [(name, return code, *out, bsk_last_error's text)], *out = None where the call left NULL (it goes in as a non-NULL value).
    ``hidden``: (16,) is the smallest network with a hidden layer that the library admits (16 ... 128 units, in multiples of 16) - with
    a narrower one the spec is refused, BSK_EINVAL, before the device is looked at."""
    import ctypes as C

    from basilisk_env_amd import _lib
    from basilisk_env_amd import policy as P
    from basilisk_env_amd.simulators.dynamics import default_config
    lib = _lib.load()
    cfg = default_config(4, _lib.GRAV_PM_J2)
    spec = P.check_spec(hidden)
    cs = P.c_spec(spec)
    params = np.zeros((n_members, P.n_params(spec)), np.float32)
    calls = (("bsk_create", lambda h: lib.bsk_create(C.byref(cfg), n_envs, device_id, None, C.byref(h))),
             ("bsk_policy_create", lambda h: lib.bsk_policy_create(C.byref(cs), params[0].ctypes.data, device_id, C.byref(h))),
             ("bsk_population_create", lambda h: lib.bsk_population_create(C.byref(cs), n_members, params.ctypes.data, device_id, C.byref(h))),
             ("bsk_es_create", lambda h: lib.bsk_es_create(C.byref(cs), n_members, params[0].ctypes.data, 0.1, 0.05, 10, 0, device_id, C.byref(h))))
    out = []
    for name, call in calls:
        h = C.c_void_p(0xDEAD)
        rc = call(h)
        out.append((name, rc, h.value, lib.bsk_last_error().decode()))
    return out
