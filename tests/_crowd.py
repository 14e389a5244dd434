"""A cast of spacecraft that covers every regime of the step kernels, and the layouts it is run in (tests/test_crowd_host.py,
tests/test_gpu_lane_independence.py).  CPU only: nothing here runs a kernel.

A spacecraft's result is a function of its own state, counters, action and the config - not of the 63 others in its wave.  The
step kernels cooperate across a wave (ballots that choose an instantiation for the whole wave, a penumbra queue any lane may
drain, LDS exchanges between the waves of the split forms), so the claim is tested by running the SAME characters with DIFFERENT
neighbours and asking for the same bits.  This module builds the characters and proves, with the oracle alone, that they are what
they claim and that the layouts put them beside the neighbours that matter.

CAST  M = 192 characters per level, 12 slots of 16, every one finite and from a regime the suite already runs on the GPU (sampled
orbits; the ``failures`` / ``desat`` edits of tests/_config_space.py: wheels x 5, charge 0, wheels x 2.5; the band, umbra and
sunlit positions of tests/_penumbra.py; counters set as tests/_outcome_scenario.py: stagger does).  Mid-episode characters are
made by the oracle: a sampled state stepped j ticks, which leaves the FSW messages of a running episode in the state's tail.

  every level   wheels   t = 0, wheel speeds x 5: beyond the limit                              (power+: characters 0, 1 in the band)
                orbit    t = 0, |r| scaled to 10 - 60 km below r_min (6 450 km; full: 6 720 km)    
                battery  t = 0, charge 0                                                          (power+: in the umbra - stays empty)
                both     t = 0, wheels x 5 and charge 0                                           (power+: in the umbra)
                mid_a    mid-episode, ticks 1 .. 16: every FSW phase
                cross    mid-episode, |sigma| = 1 - min(0.05 dt U(2, 40), 0.2) with 0.1 rad/s along sigma: the shadow-set switch inside the schedule
                length   mid-episode, step counter one short of max_length
  bare          mid_b, mid_c (ticks 17 .. 48), spin (wheels x 2.5), fresh (t = 0, healthy), late (ticks 100 000 + j)
  power, full   mid_b (power) / burst (full, with wheels: wheels x 2.5, stepped under action 2 into a thruster burst)
                sun      t = 0, 300 km outside the planet's limb behind the planet, battery full: the upper clamp
                umbra    mid-episode, half a planet radius from the shadow axis, a charge that runs out inside the schedule: the lower clamp
                band     t = 0, in the penumbra band
                band_t   in the band of the Sun of ITS OWN time: tick counters 10 000 (1 + i mod 7) + (i mod 3)
  full          dt = 1 s, base_density = 1e-4, scale_height = 20 km (tests/test_gpu_forces.py: test_density_increment_...): the slots
                of the first wave of ``sorted`` take sampled orbits whose radial speed puts the density's exponent beyond the
                2^-6 guard per tick, those of the second wave orbits inside it; the third wave flies at 1 300 - 3 000 km, below the skip density.

LAYOUTS of the same cast, each with the index map back to it: ``mixed`` (round-robin by slot: every wave holds every slot), ``sorted``
(by slot: the wave-uniform branches go the other way), ``embedded`` (n = 333, the cast at offset 37 in benign filler) and ``solo``
(one character per slot, alone in an n = 1 handle).

SCHEDULE  12 launches of one sub-step with random per-character actions, a masked host reset of every fifth character after the
fourth (fresh states from the cast's own spare list, keyed by character), then 23 and 48 sub-steps.

PROOFS (``prove``) use the oracle only - tick by tick under the schedule's own actions, the pattern of _penumbra.assert_crowded.
They are conditions on the cast, not measurements of a kernel.  What is proven set IN EVERY LANE of some ``sorted`` wave: the t = 0
message, the density guard (full), done.  The penumbra queue's branches are wave-uniform counts: proven empty, part-full and over
capacity.  Below r_min, inside a burst, below the skip density: proven none / some (skip density: none / every lane)."""
import numpy as np

import _penumbra as P
from basilisk_env_amd import _lib
from basilisk_env_amd._lib import DONE_BATTERY, DONE_LENGTH, DONE_ORBIT, DONE_WHEELS, FLAG_DESAT, GRAV_SH
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
from oracle import oracle

PER, M = 16, 192
N_EMBEDDED, OFFSET = 333, 37
# r_min and the |r| of the characters below it: under the lowest sampled perigee (6 527 km); at the full level above the dense test
# atmosphere's lowest 280 km (further down its drag torque exceeds the wheels' and makes the attitude so sensitive that the ORACLE's own answer moves by
# more than the GPU bounds under a 1e-15 perturbation of the inputs: ``prove`` checks), with the sampled orbits taken from above 6 770 km
R_MIN = {"bare": (6.45e6, 6.39e6, 6.44e6), "power": (6.45e6, 6.39e6, 6.44e6), "full": (6.72e6, 6.66e6, 6.71e6)}
PEN_SLOTS, PEN_QCAP = 30, 192  # csrc/bsk_device.hpp
RHO_SKIP = 1e-25               # csrc/bsk_config.hip
KS = (1,) * 12 + (23, 48)      # sub-steps per launch
RESET_BEFORE = 4               # the masked reset comes after the fourth launch
SLOTS = {
    "bare": ("wheels", "orbit", "battery", "both", "mid_a", "mid_b", "cross", "spin", "fresh", "length", "late", "mid_c"),
    "power": ("wheels", "orbit", "battery", "both", "mid_a", "mid_b", "cross", "length", "sun", "umbra", "band", "band_t"),
    "full": ("wheels", "orbit", "battery", "both", "mid_a", "burst", "cross", "length", "sun", "umbra", "band", "band_t"),
}
CAST_LEVEL = {"bare": "bare", "ldss": "bare", "power": "power", "full": "full", "fullg": "full"}
T0_SLOTS = ("wheels", "orbit", "battery", "both", "fresh", "sun", "band")


def crowd_config(cfg, level):
    """The cast's edits of a form's config (in place): an r_min some characters are below, and at the full level 1 s ticks in the
    dense, thin atmosphere in which the density increment's guard and the skip density are both reached."""
    cfg.r_min = R_MIN[CAST_LEVEL[level]][0]
    if CAST_LEVEL[level] == "full":
        cfg.dt = 1.0
        cfg.base_density, cfg.scale_height = 1e-4, 20e3
    return cfg


class Cast(object):
    """state (n_fields, M), steps, ticks (M,): what each character starts from; spare (n_fields, M): its fresh state at the masked
    reset; actions (14, M); slot (M,) names; filler (state, steps, ticks) of 141 benign spacecraft for ``embedded``."""

    def __init__(self, cfg, level, sh=(None, None)):
        self.cfg, self.level, self.sh, self.n_rw = cfg, CAST_LEVEL[level], sh, cfg.n_rw
        self.slots = SLOTS[self.level]
        self.slot = np.repeat(np.array(self.slots), PER)
        self.desat = bool(cfg.flags & FLAG_DESAT) and cfg.n_rw > 0
        self._build()

    def where(self, name):
        return np.flatnonzero(self.slot == name)

    # ------------------------------------------------------------------------------------------------------------ construction
    def _prerun(self, st, js, actions, first=None):
        """each column of ``st`` stepped js[i] ticks by the oracle in ONE env step (``first``: an env step of one tick under that
        action before it, which takes the t = 0 FSW tick) -> state, steps, ticks"""
        cfg, n = self.cfg, st.shape[1]
        out, steps, ticks = st.copy(), np.zeros(n, np.int32), np.zeros(n, np.int32)
        for i in range(n):
            col, s, t = np.ascontiguousarray(st[:, i:i + 1]), np.zeros(1, np.int32), np.zeros(1, np.int32)
            k = int(js[i])
            if first is not None:
                oracle.step(cfg, col, s, t, np.array([first], np.int32), 1, cbar=self.sh[0], sbar=self.sh[1])
                k -= 1
            oracle.step(cfg, col, s, t, np.array([actions[i]], np.int32), k, cbar=self.sh[0], sbar=self.sh[1])
            out[:, i], steps[i], ticks[i] = col[:, 0], s[0], t[0]
        return out, steps, ticks

    def _build(self):
        cfg, n_rw, full = self.cfg, self.n_rw, self.level == "full"
        powered = self.level != "bare"
        tail = _lib.NF_BASE + n_rw
        rng = np.random.default_rng([17, n_rw, len(self.level)])
        pool = sample_ic_batch(8000, n_rw, seed=1900 + n_rw)
        rm = np.linalg.norm(pool[0:3], axis=0)
        d = np.abs((pool[0:3] * pool[3:6]).sum(axis=0) / rm) * cfg.dt / (cfg.scale_height if full else 1.0)
        # (full level) beyond the density guard with a margin that 83 s of orbit do not use up / well inside it; elsewhere: any
        # "near" stays clear of the penumbra band for the whole schedule (1 100 km of flight at the full level): not within 1 100 km
        # of the planet's limb as seen along the shadow axis unless well on the day side
        shat = P.sun_at(cfg, 0.0) / np.linalg.norm(P.sun_at(cfg, 0.0))
        x = pool[0:3].T @ shat
        clear = (x > 1100e3) | (np.abs(np.linalg.norm(pool[0:3].T - x[:, None] * shat, axis=1) - cfg.req) > 1100e3)
        order = {"far": iter(np.flatnonzero((d > 1.12 * 2.0 ** -6) & (rm > 6.77e6)) if full else range(0, 3000)),
                 "near": iter(np.flatnonzero((d < 0.7 * 2.0 ** -6) & (rm > 6.77e6) & clear) if full else 3000 + np.flatnonzero(clear[3000:]))}

        def take(kind, k=PER):
            return np.ascontiguousarray(pool[:, [next(order[kind]) for _ in range(k)]])

        zeros = np.zeros(PER, np.int32)
        acts01 = lambda: rng.integers(0, 2, PER)                      # noqa: E731
        state, steps, ticks = [], [], []
        for name in self.slots:
            i = np.arange(PER)
            if name in ("wheels", "orbit", "battery", "both", "fresh"):
                st, s, t = take("near" if powered and name in ("battery", "both") else "far"), zeros, zeros
                if name in ("wheels", "both") and n_rw:
                    # (_config_space.Scenario: failures; the slowest sampled wheel sets scaled further, to 1.1 of the limit)
                    st[12:12 + n_rw] *= np.maximum(5.0, 1.1 * cfg.wheel_limit / np.linalg.norm(st[12:12 + n_rw], axis=0))
                if name in ("battery", "both"):
                    if powered:                                          # in the umbra: an empty battery stays empty
                        st = self._umbra(st, rng)
                    st[tail + _lib.T_CHARGE] = 0.0
                if name == "orbit":
                    st[0:3] *= rng.uniform(R_MIN[self.level][1], R_MIN[self.level][2], PER) / np.linalg.norm(st[0:3], axis=0)
                if name == "wheels" and powered:                         # two lanes of the band in a wave that has no others
                    band = P.crowd(cfg, 2, np.zeros(2, np.int32), seed=41)
                    st[0:6, :2] = band[0:6]
            elif name in ("mid_a", "mid_b", "mid_c", "late", "length", "spin", "cross", "burst"):
                st = take("near")
                j = {"mid_a": 1 + i, "mid_b": 17 + i, "mid_c": 33 + i, "late": 7 + i, "length": 20 + i, "spin": 9 + i, "cross": 5 + i,
                     "burst": 11 + i % 3}[name]
                if name in ("spin", "burst") and n_rw:
                    st[12:12 + n_rw] *= 2.5                              # (_config_space.Scenario: desat)
                if name == "burst" and self.desat:
                    st, s, t = self._prerun(st, j, np.full(PER, 2), first=1)
                else:
                    st, s, t = self._prerun(st, j, acts01())
                if name == "late":
                    t = t + 100000
                if name == "length":
                    s = np.full(PER, cfg.max_length - 1, np.int32)
                if name == "cross":
                    shat = rng.normal(size=(3, PER))
                    shat /= np.linalg.norm(shat, axis=0)
                    st[6:9] = shat * (1.0 - np.minimum(0.05 * cfg.dt * rng.uniform(2.0, 40.0, PER), 0.2))
                    st[9:12] = 0.1 * shat
            elif name == "sun":
                st = P.move_out(cfg, P.crowd(cfg, PER, zeros, seed=42), zeros, np.ones(PER, bool))
                shat, nb, k = P.sun_at(cfg, 0.0), np.array(list(cfg.panel_normal)), 0
                while k < PER:                                           # sampled attitudes whose panel faces the Sun: the battery stays full
                    col = take("near", 1)
                    if nb @ (oracle.mrp2c(col[6:9, 0]) @ shat) > 0.3 * np.linalg.norm(shat):
                        st[6:tail, k] = col[6:tail, 0]
                        k += 1
                st[tail + _lib.T_CHARGE] = cfg.storage_capacity
                s, t = zeros, zeros
            elif name == "umbra":
                st, s, t = self._prerun(self._umbra(take("near"), rng), 2 + i, acts01())
                st[tail + _lib.T_CHARGE] = abs(cfg.power_draw) * cfg.dt * rng.uniform(3.0, 60.0, PER)
            elif name == "band":
                st, s, t = P.crowd(cfg, PER, zeros, seed=43), zeros, zeros
            elif name == "band_t":
                t = (10000 * (1 + i % 7) + i % 3).astype(np.int32)
                st, s = P.crowd(cfg, PER, t, seed=44), np.ones(PER, np.int32)
            state.append(st)
            steps.append(np.asarray(s, np.int32))
            ticks.append(np.asarray(t, np.int32))
        self.state = np.ascontiguousarray(np.concatenate(state, axis=1))
        self.steps, self.ticks = np.concatenate(steps).astype(np.int32), np.concatenate(ticks).astype(np.int32)
        self.reset_mask = (np.arange(M) % 5 == 0)
        self.spare = take("near", M)
        for c in np.flatnonzero(self.reset_mask & np.isin(self.slot, ("wheels", "orbit", "battery", "both"))):
            self.spare[:, c] = take("far", 1)[:, 0]                      # (full level: the first wave of ``sorted`` stays beyond the guard)
        if powered:                                                      # the band stays as crowded after the reset
            mine = np.flatnonzero(self.reset_mask & np.isin(self.slot, ("band", "band_t")))
            self.spare[:, mine] = P.crowd(cfg, mine.size, np.zeros(mine.size, np.int32), seed=45)
        self.actions = rng.integers(0, 3, (len(KS), M)).astype(np.int32)
        # filler: sunlit, mid-episode, positive charge
        nf = N_EMBEDDED - M
        cand = take("near", 3 * nf)
        fst, fs, ft = self._prerun(cand, 1 + np.arange(3 * nf) % 9, np.ones(3 * nf, np.int32))
        probe, ps, pt = fst.copy(), fs.copy(), ft.copy()
        lit = oracle.step(cfg, probe, ps, pt, np.ones(3 * nf, np.int32), 1, cbar=self.sh[0], sbar=self.sh[1])[0][4] == 1.0
        keep = np.flatnonzero(lit & (fst[tail + _lib.T_CHARGE] > 0.0))[:nf]
        assert keep.size == nf
        self.filler = (np.ascontiguousarray(fst[:, keep]), fs[keep], ft[keep])
        assert np.isfinite(self.state).all() and np.isfinite(self.spare).all() and (np.linalg.norm(self.state[0:3], axis=0) > 6.3e6).all()

    def _umbra(self, st, rng):
        """``st`` with r, v replaced: 6 800 - 7 400 km behind the planet, half a planet radius from the shadow axis (_penumbra.mixed)"""
        cfg, n = self.cfg, st.shape[1]
        band = P.crowd(cfg, n, np.zeros(n, np.int32), seed=int(rng.integers(1 << 20)))
        shat = P.sun_at(cfg, 0.0)
        shat = shat / np.linalg.norm(shat)
        r = band[0:3].T
        x = -(r @ shat)
        lat = r + x[:, None] * shat
        lhat = lat / np.linalg.norm(lat, axis=1)[:, None]
        st = st.copy()
        st[0:3] = (-x[:, None] * shat + 0.5 * cfg.req * lhat).T
        st[3:6] = band[3:6]
        return st

    # ------------------------------------------------------------------------------------------------------------ layouts
    def layouts(self):
        """-> {name: [(n, index (n,) int: the character in each env, -1 filler), ...]} - one handle per entry"""
        n_slots = len(self.slots)
        p = np.arange(M)
        emb = np.full(N_EMBEDDED, -1)
        emb[OFFSET:OFFSET + M] = p
        return {"mixed": [(M, (p % n_slots) * PER + p // n_slots)], "sorted": [(M, p.copy())], "embedded": [(N_EMBEDDED, emb)],
                "solo": [(1, np.array([s * PER + 1])) for s in range(n_slots)]}

    def batch(self, index, charged=None):
        """-> (state, steps, ticks) of a handle whose env e holds character index[e] (-1: the next filler spacecraft).  ``charged``:
        characters whose charge is set to half the storage capacity instead (the batch-wide switch, test (d))."""
        cast = self.state.copy()
        if charged is not None:
            cast[_lib.NF_BASE + self.n_rw + _lib.T_CHARGE, charged] = 0.5 * self.cfg.storage_capacity
        f = np.cumsum(index < 0) - 1
        pick = lambda c, fl: np.where(index >= 0, c[..., np.maximum(index, 0)], fl[..., np.maximum(f, 0)])      # noqa: E731
        return np.ascontiguousarray(pick(cast, self.filler[0])), pick(self.steps, self.filler[1]).astype(np.int32), pick(self.ticks, self.filler[2]).astype(np.int32)

    def batch_actions(self, index, call):
        return np.where(index >= 0, self.actions[call][np.maximum(index, 0)], 1).astype(np.int32)

    def batch_reset(self, index):
        """-> (fresh (n_fields, n), mask (n,) uint8) of the masked reset: every fifth CHARACTER, from its own spare state"""
        fresh = np.ascontiguousarray(self.spare[:, np.maximum(index, 0)])
        return fresh, ((index >= 0) & self.reset_mask[np.maximum(index, 0)]).astype(np.uint8)

    # ------------------------------------------------------------------------------------------------------------ oracle
    def run_oracle(self, index=None, per_tick=False, charged=None):
        """The schedule on the oracle, for a handle laid out by ``index`` (default: the cast in its own order) -> per launch
        (state, obs, reward, reason, steps, ticks, steps before, ticks before), copies.  ``per_tick``: every launch as env steps of
        one tick (the step counter held at the launch's: _penumbra.factors_per_tick) -> per tick (launch, state, obs)."""
        index = np.arange(M) if index is None else index
        st, steps, ticks = self.batch(index, charged)
        kw = {"cbar": self.sh[0], "sbar": self.sh[1]}
        out = []
        for call, k in enumerate(KS):
            if call == RESET_BEFORE:
                fresh, mask = self.batch_reset(index)
                m = mask.astype(bool)
                st[:, m], steps[m], ticks[m] = fresh[:, m], 0, 0
            act = self.batch_actions(index, call)
            s0, t0 = steps.copy(), ticks.copy()
            if per_tick:
                for _ in range(k):
                    s = s0.copy()
                    o = oracle.step(self.cfg, st, s, ticks, act, 1, **kw)
                    out.append((call, st.copy(), o[0]))
                steps = s0 + 1
            else:
                o = oracle.step(self.cfg, st, steps, ticks, act, k, **kw)
                out.append((st.copy(), o[0], o[1], o[3], steps.copy(), ticks.copy(), s0, t0))
        return out


# ---------------------------------------------------------------------------------------------------------------- proofs
def _waves(index):
    """-> list of character arrays, one per wave of 64 envs of a handle (filler left out)"""
    return [index[w:w + 64][index[w:w + 64] >= 0] for w in range(0, len(index), 64)]


def prove(cast, verbose=True):
    """Every presence condition of the module docstring, from the oracle alone -> the table that is printed (a list of lines)."""
    cfg, n_rw, lvl = cast.cfg, cast.n_rw, cast.level
    tail = _lib.NF_BASE + n_rw
    runs = cast.run_oracle()
    trace = cast.run_oracle(per_tick=True)
    n_ticks = len(trace)
    call_of = np.array([c for c, _, _ in trace])
    # ---- per launch / per tick predicates, (launches or ticks, M)
    t0 = np.array([r[7] == 0 for r in runs])                                   # at its t = 0 tick in this launch
    reason = np.array([r[3] for r in runs])
    done = reason != 0
    rad = np.array([np.linalg.norm(r[0][0:3], axis=0) for r in runs])
    assert np.abs(rad / cfg.r_min - 1.0).min() > 1e-9, "a character within 1e-9 of r_min at the end of a launch"
    below = rad < cfg.r_min
    assert np.array_equal(below, (reason & DONE_ORBIT) != 0)
    sig = np.array([s[6:9] for _, s, _ in trace])
    start_sig = [cast.state[6:9]] + [s for s in sig[:-1]]
    flipped = np.array([((a * b).sum(axis=0) < 0.0) & ((a * a).sum(axis=0) > 0.81) for a, b in zip(start_sig, sig)])
    flipped[call_of == RESET_BEFORE] &= ~cast.reset_mask                        # (a reset is no switch)
    factor = np.array([o[4] for _, _, o in trace])
    band = (factor > 0.0) & (factor < 1.0)
    charge = np.array([s[tail + _lib.T_CHARGE] for _, s, _ in trace])
    rt = np.array([np.linalg.norm(s[0:3], axis=0) for _, s, _ in trace])
    rprev = np.concatenate([np.linalg.norm(cast.state[0:3], axis=0)[None], rt[:-1]])
    # The density of a chunk's first tick is a full evaluation (Atmo::anchor), the guard acts on the others: a character counts as
    # beyond the guard in a launch of many ticks if it is at EVERY tick of it, as inside if at none - whatever the chunks are
    step_far = np.abs(rt - rprev) / cfg.scale_height > 2.0 ** -6
    far = np.array([step_far[call_of == c].all(axis=0) for c in (12, 13)])
    near = np.array([(~step_far[call_of == c]).all(axis=0) for c in (12, 13)])
    skip = cfg.base_density * np.exp(-(rt - cfg.req) / cfg.scale_height) < RHO_SKIP
    lim = np.array([r[0][tail + _lib.T_THR_LIM:tail + _lib.T_THR_LIM + 8].max(axis=0) for r in runs])
    burst = (lim > 0) & np.array([2 * (r[5] - r[0][tail + _lib.T_THR_T0]) <= l for r, l in zip(runs, lim)])   # still inside it when the launch ends
    phases = {int(t) % cfg.fsw_every for t in cast.ticks[cast.slot == "mid_a"]}

    # ---- every regime occurs
    occurs = {"t = 0": t0.any(axis=0), "mid-episode": ~t0[0], "switch": flipped.any(axis=0), "length": ((reason & DONE_LENGTH) != 0).any(axis=0),
              "orbit": below.any(axis=0)}
    if n_rw:
        occurs["wheels"] = ((reason & DONE_WHEELS) != 0).any(axis=0)
    occurs["battery"] = ((reason & DONE_BATTERY) != 0).any(axis=0)
    if lvl != "bare":
        occurs.update({"sunlit": (factor == 1.0).any(axis=0), "umbra": (factor == 0.0).any(axis=0), "penumbra": band.any(axis=0),
                       "own tick": (cast.ticks >= 10000) & band.any(axis=0), "upper clamp": (charge == cfg.storage_capacity).any(axis=0),
                       "lower clamp": (charge == 0.0).any(axis=0)})
    if lvl == "full":
        occurs.update({"beyond the guard": far.any(axis=0), "inside the guard": near.any(axis=0), "below skip density": skip.any(axis=0)})
        if cast.desat:
            occurs["burst"] = burst.any(axis=0)
    assert phases == set(range(cfg.fsw_every)), phases
    expect = {"switch": "cross", "length": "length", "orbit": "orbit", "wheels": "wheels", "battery": "battery", "sunlit": "sun", "umbra": "umbra",
              "penumbra": "band", "own tick": "band_t", "lower clamp": "umbra"}
    for name, who in occurs.items():
        assert who.any(), (lvl, name, "never occurs")
        if name in expect:                                               # ... in every character of the slot built for it that is not reset
            mine = cast.where(expect[name])
            mine = mine[~cast.reset_mask[mine]]
            assert who[mine].all(), (lvl, name, mine[~who[mine]])
    if lvl != "bare":
        assert not done[:, cast.where("band")].any() and not done[0, cast.where("sun")].any()     # healthy t = 0 characters

    # ---- conditioning: the bounds of the GPU test's comparison with the oracle (1e-11 per state group) presume characters whose
    # own sensitivity is far below them - the oracle's answer under a relative 1e-15 perturbation of the dynamic state moves by
    # less than a fifth of the bound, at every launch, in every group (the torque commands are the most sensitive: gain / u_max)
    from helpers import max_group_err
    nd, worst, rng = _lib.NF_BASE + n_rw, 0.0, np.random.default_rng(5)
    saved = cast.state
    try:
        for _ in range(3):
            cast.state = saved.copy()
            cast.state[:nd] *= 1.0 + 1e-15 * rng.normal(size=(nd, M))
            for a, b in zip(cast.run_oracle(), runs):
                worst = max(worst, max(max_group_err(a[0], b[0], n_rw).values()))
    finally:
        cast.state = saved
    assert worst < 2e-12, (lvl, "ill-conditioned character", worst)

    lay = cast.layouts()
    lines = ["%-18s %s" % ("regime", "waves holding it:  mixed  sorted   (of %d)" % len(_waves(lay["mixed"][0][1])))]
    mixed, srt = _waves(lay["mixed"][0][1]), _waves(lay["sorted"][0][1])
    for name, who in occurs.items():
        nm, ns = sum(bool(who[w].any()) for w in mixed), sum(bool(who[w].any()) for w in srt)
        lines.append("%-18s %24d %7d" % (name, nm, ns))
        assert nm == len(mixed), (lvl, name, "not in every wave of mixed")
    for w in mixed:                                                      # every slot in every wave
        assert set(cast.slot[w]) == set(cast.slots)

    # ---- mixed: in every wave a t = 0 lane beside mid-episode lanes; queued, over-capacity and far lanes
    k23 = call_of == 12

    def entries(w, sel):                                                 # queue entries a wave pushes in the ticks ``sel`` (one record)
        return int(band[sel][:, w].sum())

    first30 = np.flatnonzero(call_of == 13)[:PEN_SLOTS]
    for w in mixed:
        assert t0[0, w].any() and (~t0[0, w]).any() and t0[RESET_BEFORE, w].any() and (~t0[RESET_BEFORE, w]).any()
        if lvl != "bare":
            assert min(entries(w, call_of == c) for c in range(12)) >= 1                                    # queued, every launch
            assert entries(w, k23) > PEN_QCAP and entries(w, first30) > PEN_QCAP, (entries(w, k23), entries(w, first30))
        if lvl == "full":
            assert far[:, w].any(axis=1).all() and near[:, w].any(axis=1).all() and skip[:, w].any(axis=1).all() and (~skip[:, w]).any(axis=1).all()
            if cast.desat:
                assert burst[:12, w].any() and (burst[:12, w].any(axis=1) & (~burst[:12, w]).any(axis=1)).any()

    # ---- sorted: each ballot at zero in one wave and set in another (in every lane where the docstring says so)
    def zero_and_all(pred, what, every_lane=True, unset=None):
        """``pred`` (launches or ticks, M): some wave with no lane set and some wave with every (or some) lane set, at one time"""
        unset = ~pred if unset is None else unset
        none = any(unset[:, w].all(axis=1).any() for w in srt)
        full_ = any((pred[:, w].all(axis=1) if every_lane else pred[:, w].any(axis=1)).any() for w in srt)
        assert none and full_, (lvl, what, none, full_)

    zero_and_all(t0, "t = 0 message")
    if n_rw:
        zero_and_all(done, "done")
    zero_and_all(below, "below r_min", every_lane=False)
    if lvl != "bare":
        counts = sorted(entries(w, k23) for w in srt)
        assert counts[0] == 0 and 0 < counts[1] <= PEN_QCAP < counts[2], counts        # empty, part-full, over capacity
        lines.append("queue entries of the K = 23 record per wave of sorted: %s (capacity %d)" % (counts, PEN_QCAP))
    if lvl == "full":
        zero_and_all(far, "density guard", unset=near)
        zero_and_all(skip, "skip density")
        if cast.desat:
            zero_and_all(burst, "burst", every_lane=False)
    lines.append("the oracle under a 1e-15 perturbation of the inputs moves by %.1e of a state group at most (GPU bound 1e-11)" % worst)
    ends = sorted({int(c) for c in np.flatnonzero(done.any(axis=1))})
    lines.append("%d ticks, launches with an episode end: %s" % (n_ticks, ends))
    if verbose:
        print("\n[%s, %d wheels]\n" % (lvl, n_rw) + "\n".join(lines))
    return lines


def cast_for(case, sh_seed=3):
    """(cfg, Cast) of one entry of tests/test_gpu_kernel_info.py: STEPPED (its config with ``crowd_config``'s edits)"""
    import test_gpu_kernel_info as KI
    from helpers import visible_sh_coefficients
    (grav, n_rw, level, diag, _, _, _), _ = KI.STEPPED[case] if isinstance(case, (int, np.integer)) else case
    cfg = crowd_config(KI.config(grav, n_rw, level, diag), level)
    sh = visible_sh_coefficients(cfg.sh_degree, seed=sh_seed) if grav == GRAV_SH else (None, None)
    return cfg, Cast(cfg, level, sh)
