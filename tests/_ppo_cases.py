"""Shapes and value placements for bsk_fit_accumulate_ppo beyond one small network (csrc/bsk_fit.hip: fit_block_kernel<true,
FitVclip>, fit_fold_kernel<10, double*>; definition in include/bskgpu.h), shared by tests/test_gpu_ppo_shapes.py and its CPU twin
tests/test_ppo_cases_host.py.  TEST CODE.

The case table takes the third instantiation of the block kernel to the shapes the other two already run at (BIT_CASES in
tests/test_gpu_fit.py, PG_BIT_CASES in tests/test_gpu_pg.py).  ``lds_rows`` restates fit_lds_rows and ``ppo_lds_bytes`` the
launch's dynamic LDS: (rows + 5 + 8 + 4) rows of 64 floats - the network rows, then the diagnostics terms of the supervised, the
policy-gradient and the value-clip launch.  Above 48 KiB the launch sets the kernel's MaxDynamicSharedMemorySize attribute first.

The placements put old values and targets around GIVEN value outputs v (the device's own on the GPU, ``mlp_ref``'s here: for relu
networks the two are the same bits).  ``place`` lands every sample well inside a branch of the value loss; ``tie_place`` lands it ON
one of the two ties the definition rules on, built exactly in f32 with cv = 0.25:
  edge tie   s = sign(v), vo = fl(v - s cv):  fl(v - vo) == s cv, the range test -cv <= dv <= cv holds with equality, the sample is
             inside and unclipped.  Where fl(vo + s cv) != v (vo was rounded: |v| well below cv) the target is v itself: d = 0, and a
             kernel that took the sample for outside would find d2 d2 > d d, count it as value-clipped and add a term to the loss.
             Where fl(vo + s cv) == v the two readings of the edge are the same function, and the target is v + s.
  max tie    vo = fl(v - s / 2), R = fl(v - s / 8):  outside the range, and d2 == -d != 0, so d2 d2 == d d.  A tie is the unclipped
             branch's: delta = value_coef d.  An fma contraction of the comparison would compare the exact d2 d2 with the rounded d d.
A sample at which the defining equality does not hold exactly in f32 falls back to ``place``'s kind for its index.
"""
import numpy as np

from _policy_bounds import observation_like, seeded_policy
from basilisk_env_amd import policy as P

CV = 0.25
KINDS = ("inside", "above_clipped", "above_unclipped", "below_clipped", "below_unclipped")
NET_SEED = 11                                  # seeded_policy's seed of every case of the table
FIT_X_ROWS, POLICY_OB, DIAG_ROWS = 8, 4, 5 + 8 + 4
LDS_NO_ATTRIBUTE = 48 * 1024                   # the dynamic LDS a launch may ask for without the function attribute

# name -> (hidden, value_hidden, sizes of the calls before one step)
PPO_CASES = {
    "ppo_w112_48_v96": ((112, 48), (96,), [130]),          # fit_weight_grad past one trip of 64 rows, both orientations; 189 rows
    "ppo_w128_48_v96": ((128, 48), (96,), [130]),          # 205 rows: the instantiation's own hipFuncSetAttribute
    "ppo_relu128x3": ((128, 128, 128), (16,), [65]),       # 413 rows: the largest carve, s_vc at its far end
    "ppo_v_wider": ((16,), (128, 128), [130]),             # rows sized by the value network
    "ppo_fold33": ((16,), (16,), [2049]),                  # the ten-column fold: a batch of 32 blocks and one
    "ppo_fold33_wide": ((16,), (16,), [2049]),             # ... with targets of order 1e12: the fold's order shows in f64
    "ppo_fold69_two_calls": ((16,), (16,), [4400, 100]),   # two full batches and a tail, then a second call into the same A
    "ppo_grow": ((16,), (16,), [29, 100]),                 # the scratch regrows between two accumulates of one step
}
LDS_ROWS = {"ppo_w112_48_v96": 189, "ppo_w128_48_v96": 205, "ppo_relu128x3": 413, "ppo_v_wider": 285, "ppo_fold33": 45,
            "ppo_fold33_wide": 45, "ppo_fold69_two_calls": 45, "ppo_grow": 45}
# the samples of ppo_fold33_wide that carry a huge target, one in each of eight blocks spread over the 33, and the targets: from
# 1e12 down to 1e9 in scrambled order, so that the squared errors (48 significant bits each) span twenty binary orders and their
# f64 sum rounds at every addition (six targets within a factor of three of each other sum exactly, in any order)
WIDE_AT = (7, 64 * 4 + 9, 64 * 8 + 2, 64 * 11 + 30, 64 * 15 + 17, 64 * 19 + 1, 64 * 27 + 40, 64 * 32)
WIDE_TARGETS = tuple(1e12 * 0.37 ** i for i in (3, 0, 5, 1, 7, 2, 6, 4))
SEED_OF_CALL = 20                              # call k of a case draws its batch under seed 20 + k


def lds_rows(hidden, value_hidden):
    """fit_lds_rows: the x rows, the hidden layers of the wider of the two networks, the output deltas"""
    return FIT_X_ROWS + max(sum(hidden), sum(value_hidden or ())) + POLICY_OB


def ppo_lds_bytes(hidden, value_hidden):
    return (lds_rows(hidden, value_hidden) + DIAG_ROWS) * 64 * 4


def masked_batch(n, seed):
    """tests/test_gpu_fit.py's ``_batch``: observations, actions (two out of range) and alive bytes (two zero) -> (obs, actions,
    alive, the mask of the contributing samples)"""
    from test_gpu_fit import _batch
    obs, actions, alive, _ = _batch(n, seed)
    on = (actions >= 0) & (actions <= 2) & (alive != 0)
    assert n <= 8 or (~on).sum() == 4
    return obs, actions, alive, on


def place(v, kinds):
    """old values and targets around the given v that put sample j into branch kinds[j]: dv = +-0.1 inside the range of
    0.25 and +-1.0 outside it; squared errors 1 against 3.06 where the clipped branch holds the max, 4 against 1.56 where not"""
    vo, R = np.empty(v.size, np.float32), np.empty(v.size, np.float64)
    for j, kind in enumerate(kinds):
        side = -1.0 if kind.startswith("below") else 1.0
        vo[j] = v[j] - np.float32(side * (0.1 if kind == "inside" else 1.0))
        R[j] = float(v[j]) + side * (-2.0 if kind.endswith("unclipped") else 1.0)
    return vo, R


def cycle_kinds(n, shift=0):
    return [KINDS[(j + shift) % len(KINDS)] for j in range(n)]


def case_values(v, wide=False):
    """the old values and targets of a call of the case table: ``place`` with the five kinds in turn (every one occurs among any
    five consecutive samples, so among the contributing ones of every call); ``wide`` plants WIDE_TARGETS"""
    vo, R = place(v, cycle_kinds(v.size))
    if wide:
        R[list(WIDE_AT)] = WIDE_TARGETS
    return vo, R


def tie_place(v):
    """-> (vo float32, R float64, edge bool, peak bool, visible bool): even samples on the edge tie, odd ones on the max tie (the
    module's docstring); ``edge`` / ``peak`` mark the samples at which the tie holds exactly in f32 - checked here, in numpy f32 -
    and ``visible`` those edge ties at which fl(vo + s cv) != v.  Every other sample is ``place``'s for its index."""
    v = np.asarray(v, np.float32).reshape(-1)
    cv = np.float32(CV)
    vo, R = place(v, cycle_kinds(v.size))
    edge, peak, visible = (np.zeros(v.size, bool) for _ in range(3))
    for j in range(v.size):
        s = np.float32(-1.0 if v[j] < 0 else 1.0)
        if j % 2 == 0:
            o = np.float32(v[j] - s * cv)
            if np.float32(v[j] - o) == s * cv:
                back = np.float32(o + s * cv)
                edge[j], visible[j] = True, back != v[j]
                vo[j], R[j] = o, float(v[j]) if visible[j] else float(v[j]) + float(s)
        else:
            o, r = np.float32(v[j] - s * np.float32(0.5)), np.float32(v[j] - s * np.float32(0.125))
            dv = np.float32(v[j] - o)
            d = np.float32(v[j] - r)
            d2 = np.float32(np.float32(o + (cv if dv > 0 else -cv)) - r)
            if not (-cv <= dv <= cv) and d2 == -d and d != 0:
                peak[j] = True
                vo[j], R[j] = o, float(r)
    return vo, R, edge, peak, visible


def block_terms(x):
    """per-sample f64 terms -> the block sums: sample-ascending within blocks of 64 from +0.0"""
    out = []
    for b in range(0, x.size, 64):
        part = 0.0
        for t in x[b:b + 64].astype(np.float64).tolist():
            part = part + t
        out.append(part)
    return out


def fold(parts, descending=False):
    total = 0.0
    for part in (reversed(parts) if descending else parts):
        total = total + part
    return total


def ref_values(hidden, value_hidden, n, seed):
    """the restatement's value outputs of a case's network on a call's observations -> (spec, params, obs, v float32 (n,))"""
    spec, params = seeded_policy(hidden, "relu", value_hidden, seed=NET_SEED)
    obs = observation_like(n, seed)
    return spec, params, obs, P.mlp_ref(spec, params, obs)[1].reshape(-1)


# the tie test: (hidden, value_hidden, n, seed of the network and of the batch)
TIE_CASES = [((16,), (16,), 65, 60), ((16,), (16,), 130, 60), ((16,), (128, 128), 130, 60)]


def tie_case_net(hidden, value_hidden, seed):
    return seeded_policy(hidden, "relu", value_hidden, seed=seed)
