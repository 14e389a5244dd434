"""CPU: the cast and the layouts of tests/_crowd.py are what they claim - by the oracle alone, no kernel.

``test_presence`` runs ``_crowd.prove`` for the config of every kernel form tests/test_gpu_kernel_info.py: STEPPED pins (all three
levels, every wheel count and gravity model among them) and prints, per level, how many waves of ``mixed`` and of ``sorted`` hold each
regime.  The other two guard the harness's own indexing: every layout is a permutation / an embedding of the cast, and the oracle's
outputs for a character are the same bits in whichever layout it is run (trivially true of the oracle - so a difference is a
mistake in ``batch`` / ``batch_actions`` / ``batch_reset``)."""
import numpy as np
import pytest

import _crowd as C
import test_gpu_kernel_info as KI

CASES = list(range(len(KI.STEPPED)))
PRINTED = set()


@pytest.mark.parametrize("case", CASES, ids=[w[0] for _, w in KI.STEPPED])
def test_presence(case, capsys):
    cfg, cast = C.cast_for(case)
    first = (cast.level, cast.n_rw > 0) not in PRINTED
    PRINTED.add((cast.level, cast.n_rw > 0))
    with capsys.disabled():
        lines = C.prove(cast, verbose=first)
    assert len(lines) >= 3
    assert np.isfinite(cast.state).all() and np.isfinite(cast.spare).all() and np.isfinite(cast.filler[0]).all()
    assert (np.linalg.norm(cast.state[0:3], axis=0) > 6.3e6).all()                # no zero radius


@pytest.mark.parametrize("level_case", [0, 5, 9], ids=["bare", "power", "full"])
def test_layouts_are_permutations_or_embeddings(level_case):
    cfg, cast = C.cast_for(level_case)
    lay = cast.layouts()
    assert sorted(lay) == ["embedded", "mixed", "solo", "sorted"]
    for name in ("mixed", "sorted"):
        (n, index), = lay[name]
        assert n == C.M and np.array_equal(np.sort(index), np.arange(C.M)), name
    assert not np.array_equal(lay["mixed"][0][1], lay["sorted"][0][1])
    (n, index), = lay["embedded"]
    assert n == C.N_EMBEDDED and np.array_equal(index[C.OFFSET:C.OFFSET + C.M], np.arange(C.M))
    assert (index[:C.OFFSET] == -1).all() and (index[C.OFFSET + C.M:] == -1).all() and C.OFFSET % 64 != 0 and n % 64 != 0
    solo = [int(index[0]) for n, index in lay["solo"] if n == 1 and index.shape == (1,)]
    assert len(solo) == len(cast.slots) and [cast.slot[c] for c in solo] == list(cast.slots)
    # what a handle is given is the character's own state, counters, action and spare - wherever it sits
    for name, handles in lay.items():
        for n, index in handles:
            st, steps, ticks = cast.batch(index)
            have = index >= 0
            assert np.array_equal(st[:, have], cast.state[:, index[have]]) and np.array_equal(steps[have], cast.steps[index[have]])
            assert np.array_equal(ticks[have], cast.ticks[index[have]])
            fresh, mask = cast.batch_reset(index)
            assert np.array_equal(mask.astype(bool), have & cast.reset_mask[np.maximum(index, 0)])
            assert np.array_equal(fresh[:, have], cast.spare[:, index[have]])
            for call in range(len(C.KS)):
                assert np.array_equal(cast.batch_actions(index, call)[have], cast.actions[call][index[have]])
            # filler: sunlit, mid-episode, positive charge
            assert (ticks[~have] > 0).all() and (st[12 + cast.n_rw + 7, ~have] > 0.0).all()


@pytest.mark.parametrize("level_case", [0, 5, 9, 17], ids=["bare", "power", "full", "harmonics"])
def test_oracle_outputs_of_a_character_are_the_same_bits_in_every_layout(level_case):
    cfg, cast = C.cast_for(level_case)
    ref = cast.run_oracle()
    for name, handles in cast.layouts().items():
        for n, index in handles:
            have = index >= 0
            got = cast.run_oracle(index)
            for call, (g, r) in enumerate(zip(got, ref)):
                for k, (x, y) in enumerate(zip(g, r)):
                    x, y = x[..., have], y[..., index[have]]
                    same = np.array_equal(x.view(np.uint64), y.view(np.uint64)) if x.dtype == np.float64 else np.array_equal(x, y)
                    assert same, (name, call, k)
