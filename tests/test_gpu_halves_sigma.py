"""GPU: the halves form's attitude, integrated behind the hand-over.  The rotational wave runs the angular velocity's four stages
first, hands |omega|^2, sum Omega_k^2 and |sigma_BR| over, and only behind the form's last barrier integrates sigma from the stage
rates it kept, applies the shadow-set switch and stores the rows (csrc/bsk_device.hpp: rk4_rot_omega, rk4_rot_sigma).  Every value is
still produced by the operations of rk4_step in its order, so everything here is the form forced on against the form forced off,
bit for bit over every state row, counter and output (test_gpu_halves._same), and against the CPU oracle at the bounds
tests/test_gpu_halves_epilogue.py uses (state 1e-12 of each row's scale, observations 1e-12, rewards 1e-14, the rest exact).

Batches: tests/_halves_sigma.py (n = 65 and 130; the shadow-set switch in some lanes of a wave and not in others, a wave in which every
lane crosses, large rates, every FSW phase in one wave, ragged tails that shadow a crossing env through the deferred sigma stores);
tests/test_halves_sigma_host.py proves from the oracle alone that they hold all of that.  Cells: 4 wheels with a diagonal hub, 3
wheels with a general one; nav_lag = 1; int32 and int64 actions; 25 launches, each of them the launch before, at and after an FSW
tick of some lane."""
import numpy as np
import pytest

import _halves_sigma as H
from test_gpu_halves import OBS_TOL, REW_TOL, STATE_TOL, _is_halves, _is_single, _same, make

pytestmark = pytest.mark.gpu


def _against_oracle(p, ref, ctx):
    st, o_obs, o_rew, o_done, o_why, o_steps, o_ticks = ref
    obs, rew, done, why = p.get_obs()
    assert np.array_equal(why.astype(np.int64), o_why.astype(np.int64)), (ctx, "reason")
    assert np.array_equal(done, o_done.astype(bool)), (ctx, "done")
    assert np.abs(obs - o_obs).max() < OBS_TOL, (ctx, "obs", np.abs(obs - o_obs).max(axis=1))
    assert np.abs(rew - o_rew).max() < REW_TOL, (ctx, "reward", np.abs(rew - o_rew).max())
    scale = np.maximum(np.abs(st).max(axis=1, keepdims=True), 1e-300)
    err = np.abs(p.get_state() - st) / scale
    assert err.max() < STATE_TOL, (ctx, "state", float(err.max()), np.unravel_index(err.argmax(), err.shape))
    steps, ticks = p.get_counters()
    assert np.array_equal(steps, o_steps) and np.array_equal(ticks, o_ticks), (ctx, "counters")


@pytest.mark.parametrize("wide", [False, True], ids=["int32", "int64"])
@pytest.mark.parametrize("n", H.SIZES)
@pytest.mark.parametrize("grav,n_rw,diag", H.CELLS)
def test_attitude_behind_the_hand_over_equals_the_single_wave_form_and_the_oracle(grav, n_rw, diag, n, wide):
    import torch
    b = H.batch(grav, n_rw, diag, n)
    assert b.cfg.nav_lag == 1
    off, on = make(b.cfg, n, False), make(b.cfg, n, True)
    for p in (off, on):
        p.reset(b.state)
        p.set_counters(b.steps, b.ticks)
        p.set_step_stats(True)
    switched = np.zeros(n, bool)
    before = on.get_state()[6:9]
    for t in range(H.LAUNCHES):
        act = b.actions[t]
        d_act = torch.from_numpy(act.astype(np.int64) if wide else act).cuda()
        for p in (off, on):
            p.step_device(d_act.data_ptr(), 1, int64=wide)
            p.sync()
        ctx = (grav, n_rw, diag, n, wide, t)
        _same(off, on, ctx)
        _against_oracle(on, b.ref[t], ctx)
        after = on.get_state()[6:9]
        took = ((before * after).sum(axis=0) < 0.0) & ((before * before).sum(axis=0) > 0.81)
        assert np.array_equal(took, b.switched[t]), (ctx, "shadow-set switch", np.flatnonzero(took != b.switched[t]))
        switched |= took
        before = after
        del d_act
    assert _is_halves(on) and _is_single(off)
    # what the batch was built for was there: the switch in some lanes of the mixed wave and not in others, in every lane of the
    # all-crossing wave, in the env the ragged tail shadows
    assert switched[:64].any() and not switched[:64].all()
    assert switched[64] if n == 65 else (switched[64:128].all() and switched[128] and not switched[129])
    off.close()
    on.close()
