"""CPU: the constructions tests/test_gpu_ppo_shapes.py runs on the device (tests/_ppo_cases.py), checked on the numpy restatement's
value outputs - for relu networks the bits the device forms - so that a case cannot pass for a reason other than the one it is there
for: the case table's LDS row counts against fit_lds_rows' formula and the 48 KiB line, the five branches among the contributing
samples of every call, the two ties of the value loss holding exactly in f32 for the seeds the GPU test uses, and the order of the
ten-column fold being visible in the bits of the sums of ``ppo_fold33_wide``."""
import numpy as np
import pytest

from _device_bits import same as _same
from _ppo_cases import (CV, KINDS, LDS_NO_ATTRIBUTE, LDS_ROWS, PPO_CASES, SEED_OF_CALL, TIE_CASES, WIDE_AT, WIDE_TARGETS, block_terms,
                        case_values, cycle_kinds, fold, lds_rows, masked_batch, ppo_lds_bytes, ref_values, tie_case_net, tie_place)
from _policy_bounds import observation_like
from basilisk_env_amd import policy as P


def test_the_case_table_reaches_the_lds_sizes_it_names():
    """fit_lds_rows = 8 + the hidden units of the wider network + 4; the third instantiation adds 5 + 8 + 4 rows of diagnostics"""
    assert lds_rows((16,), None) == 28 and lds_rows((16,), (16,)) == 28 and lds_rows((128, 128, 128), None) == 396
    for name, (hidden, vh, sizes) in PPO_CASES.items():
        assert lds_rows(hidden, vh) + 17 == LDS_ROWS[name] and ppo_lds_bytes(hidden, vh) == LDS_ROWS[name] * 256, name
        spec = P.check_spec(hidden, "relu", vh)
        a, v = P.layer_shapes(spec)
        assert lds_rows(hidden, vh) == 8 + max(sum(o for o, _ in a[:-1]), sum(o for o, _ in v[:-1])) + 4, name
    below, above = ppo_lds_bytes(*PPO_CASES["ppo_w112_48_v96"][:2]), ppo_lds_bytes(*PPO_CASES["ppo_w128_48_v96"][:2])
    assert below == 48384 <= LDS_NO_ATTRIBUTE < above == 52480          # either side of the launch's hipFuncSetAttribute
    assert ppo_lds_bytes(*PPO_CASES["ppo_relu128x3"][:2]) == 105728
    hidden, vh, _ = PPO_CASES["ppo_v_wider"]
    assert sum(vh) > sum(hidden)                                # the rows are the value network's
    # the fold: a batch of 32 blocks and one; two batches and five blocks, then two blocks; one block, then two
    blocks = {name: [-(-n // 64) for n in sizes] for name, (_, _, sizes) in PPO_CASES.items()}
    assert blocks["ppo_fold33"] == blocks["ppo_fold33_wide"] == [33] and blocks["ppo_fold69_two_calls"] == [69, 2]
    assert blocks["ppo_grow"] == [1, 2]                         # smaller first: the second call regrows the scratch
    assert len(set(b // 64 for b in WIDE_AT)) == len(WIDE_AT) == 8 and max(WIDE_AT) // 64 == 32 and max(WIDE_AT) < 2049


@pytest.mark.parametrize("name", list(PPO_CASES))
def test_every_call_of_the_table_has_all_five_branches_among_its_contributing_samples(name):
    hidden, vh, sizes = PPO_CASES[name]
    for k, n in enumerate(sizes):
        spec, params, obs, v = ref_values(hidden, vh, n, SEED_OF_CALL + k)
        batch_obs, actions, alive, on = masked_batch(n, SEED_OF_CALL + k)
        assert _same(batch_obs, obs)
        wide = name == "ppo_fold33_wide"
        vo, R = case_values(v, wide)
        delta, term, clipped = P.fit_value_delta_ref(v, R, vo, CV, 0.5)
        kinds = np.array(cycle_kinds(n))
        plain = np.ones(n, bool)
        if wide:
            plain[list(WIDE_AT)] = False
            assert on[list(WIDE_AT)].all()
        assert [k_.endswith("_clipped") for k_ in kinds[plain]] == list(clipped[plain])
        assert set(kinds[on & plain]) == set(KINDS)
        dv = (v - vo).astype(np.float64)
        assert (np.abs(np.abs(dv) - CV) > 2.0 ** -10 * CV).all()         # (no sample near an edge: the ties are another test's)
        assert (delta[on & ~clipped] != 0).all() and not delta[clipped].any()


def test_the_wide_case_cannot_pass_a_reversed_fold():
    """Eight targets from 1e12 down to 1e9 in eight blocks: the squared errors have 48 significant bits each and span twenty binary
    orders, so the f64 sum of the block terms rounds at every addition, and block-ascending and block-descending differ in bits -
    in the value loss column and in the unclipped one."""
    hidden, vh, (n,) = PPO_CASES["ppo_fold33_wide"]
    spec, params, obs, v = ref_values(hidden, vh, n, SEED_OF_CALL)
    _, _, _, on = masked_batch(n, SEED_OF_CALL)
    vo, R = case_values(v, wide=True)
    assert np.array_equal(R[list(WIDE_AT)], WIDE_TARGETS)
    _, term, clipped = P.fit_value_delta_ref(v, R, vo, CV, 0.5)
    plain = P.fit_value_delta_ref(v, R, None, None, 0.5)[1]
    for x in (np.where(on, term, 0.0), np.where(on, plain, 0.0)):
        parts = block_terms(x)
        assert len(parts) == 33
        up, down = fold(parts), fold(parts, descending=True)
        print("ascending %r, descending %r" % (up.hex(), down.hex()))
        assert up != down and abs(up - down) <= 2.0 ** -45 * up
    # ... while without the targets the two orders give the same bits: the plain case does not see the order
    vo, R = case_values(v)
    parts = block_terms(np.where(on, P.fit_value_delta_ref(v, R, vo, CV, 0.5)[1], 0.0))
    print("plain: ascending %r, descending %r" % (fold(parts).hex(), fold(parts, descending=True).hex()))


@pytest.mark.parametrize("hidden,vh,n,seed", TIE_CASES)
def test_the_ties_hold_exactly_in_f32_on_the_restatements_values(hidden, vh, n, seed):
    """At least three samples in four of each kind are true ties (a condition on the construction, not a tolerance), counted over
    the contributing samples alone; every one is checked against the restatement: unclipped, with the delta the definition gives."""
    spec, params = tie_case_net(hidden, vh, seed)
    obs = observation_like(n, seed)
    _, _, _, on = masked_batch(n, seed)
    v = P.mlp_ref(spec, params, obs)[1].reshape(-1)
    vo, R, edge, peak, visible = tie_place(v)
    even = np.arange(n) % 2 == 0
    print("n %d: edge ties %d of %d (visible %d), max ties %d of %d" % (n, (edge & on).sum(), (even & on).sum(), (visible & on).sum(),
                                                                         (peak & on).sum(), (~even & on).sum()))
    assert 4 * (edge & on).sum() >= 3 * (even & on).sum() and 4 * (peak & on).sum() >= 3 * (~even & on).sum()
    assert not (edge & ~even).any() and not (peak & even).any() and not (visible & ~edge).any()
    cv = np.float32(CV)
    dv = (v - vo).astype(np.float32)
    assert (np.abs(dv[edge]) == cv).all() and (np.abs(dv[peak]) == np.float32(0.5)).all()
    delta, term, clipped = P.fit_value_delta_ref(v, R, vo, CV, 0.5)
    d = (v - R.astype(np.float32)).astype(np.float32)
    assert not clipped[edge | peak].any()
    assert _same(delta[edge | peak], (np.float32(0.5) * d)[edge | peak]) and (d[peak] != 0).all()
    # what a kernel that read either tie the other way would give differs from the restatement
    vc = (vo + np.where(dv > 0, cv, -cv)).astype(np.float32)
    d2 = (vc - R.astype(np.float32)).astype(np.float32)
    assert _same(d2[peak], -d[peak])                            # d2 d2 >= d d would clip every max tie
    assert (visible & on).sum() >= 1 and ((d2 * d2)[visible] > (d * d)[visible]).all()          # outside would clip these edge ties
    assert (v[visible & on] > 0).any() and (v[visible & on] < 0).any()                # either side of the range test
