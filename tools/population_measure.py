#!/usr/bin/env python3
"""Cost of the population form of the policy ("Populations"): 65 536 spacecraft, `tanh [64, 64]`, K = 1.

  python tools/population_measure.py kernel
      launches, on the env's own observation buffers, blocks of WARM + COUNT evaluations: `bsk_policy_act` (action and logp), then
      `bsk_population_act` with P = 1, 64 and 1 024 members of distinct parameters; three rounds, alternating.  Run it under the
      profiler in a run of its own:  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o pop -- python tools/population_measure.py kernel
  python tools/population_measure.py stats DIR/.../pop_kernel_trace.csv
      the median kernel time of every block of that run (the blocks are recognised by their order)
  python tools/population_measure.py loop
      host clock around 200 env steps of `bsk_policy_rollout` and of `bsk_population_rollout` (with all four fitness outputs) and a
      synchronisation, after a 10-step warm-up rollout, profiler off; three runs, alternating.

A library built from an older tree (BSKGPU_LIB) has no population entry points: the blocks it cannot run are left out, and `stats`
is told so with --single-only.
"""
import csv
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

N, WARM, COUNT, ROUNDS = 65536, 10, 31, 3
MEMBERS = (1, 64, 1024)


def _members(P_mod, spec, n_members):
    rng = np.random.default_rng(7)
    a, _ = P_mod.layer_shapes(spec)
    blocks = []
    for _ in range(n_members):
        layers = [(rng.normal(0.0, np.sqrt(1.0 / i), (o, i)).astype(np.float32), rng.normal(0.0, 0.3, o).astype(np.float32)) for o, i in a]
        blocks.append(P_mod.pack_params(spec, layers, None, [2.0, 50.0, 1.5, 1.25, 0.75], [-0.5, 0.1, -0.3, -0.6, 0.2]))
    return np.stack(blocks)


def _setup():
    import torch
    from basilisk_env_amd import _lib
    from basilisk_env_amd import policy as P
    from basilisk_env_amd.envs.leoPowerAttitudeVecEnv import LeoPowerAttVecEnv
    side = torch.cuda.Stream()
    env = LeoPowerAttVecEnv(N, device_reset_pool=4096, device_sampler=True, stream=side.cuda_stream)
    env.reset_tensors()
    prop = env.propagator
    prop.step(np.zeros(N, np.int32), 1)
    spec = P.check_spec((64, 64), "tanh")
    lib = _lib.load()
    have = hasattr(lib, "bsk_population_act")
    params = _members(P, spec, max(MEMBERS))
    pol = P.DevicePolicy(spec, params[0])
    pops = {m: P.PolicyPopulation(spec, params[:m]) for m in MEMBERS} if have else {}
    return torch, lib, P, env, prop, pol, pops


def kernel():
    torch, lib, P, env, prop, pol, pops = _setup()
    v = prop.device_views()
    obs, stride, stream = v["obs"].__cuda_array_interface__["data"][0], v["stride"], C.c_void_p(prop.stream_ptr())
    act = torch.zeros(N, dtype=torch.int32, device="cuda")
    logp = torch.zeros(N, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for _ in range(WARM + COUNT):
            lib.bsk_policy_act(pol._handle(), C.c_void_p(obs), stride, N, 0, 0, act.data_ptr(), logp.data_ptr(), None, None, 0, stream)
        for m, pop in pops.items():
            for _ in range(WARM + COUNT):
                lib.bsk_population_act(pop._handle(), C.c_void_p(obs), stride, N, N // m, 0, 0, act.data_ptr(), logp.data_ptr(), None, None,
                                       0, stream)
        prop.sync()
    print("blocks per round: policy_kernel%s; %d rounds of %d + %d launches" % ("".join(", P = %d" % m for m in pops), ROUNDS, WARM, COUNT))
    env.close()


def stats(path, single_only):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "policy_kernel" in name or "policy_population_kernel" in name:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), name))
    rows.sort()
    labels = ["policy_kernel"] + ([] if single_only else ["population P = %d" % m for m in MEMBERS])
    per = WARM + COUNT
    assert len(rows) == ROUNDS * per * len(labels), (len(rows), ROUNDS * per * len(labels))
    for b, label in enumerate(labels):
        meds = []
        for rnd in range(ROUNDS):
            at = (rnd * len(labels) + b) * per
            block = rows[at:at + per]
            assert all(("population" in name) == (b > 0) for _, _, name in block)
            meds.append(statistics.median(d for _, d, _ in block[WARM:]) / 1e3)
        print("%-22s median of %d launches, us, per round: %s" % (label, COUNT, ", ".join("%.1f" % m for m in meds)))


def loop():
    torch, lib, P, env, prop, pol, pops = _setup()
    T = 200
    outs = {m: (torch.zeros(N, dtype=torch.float64, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda"),
                torch.zeros(m, dtype=torch.float64, device="cuda"), torch.zeros(m, dtype=torch.float64, device="cuda")) for m in pops}
    torch.cuda.synchronize()

    def single(steps):
        pol.rollout_device(prop, steps, 1)

    def population(m):
        def run(steps):
            ev, el, fit, ml = outs[m]
            pops[m].rollout_device(prop, steps, 1, "greedy", 0.99, d_env_value=ev.data_ptr(), d_env_len=el.data_ptr(),
                                   d_fitness=fit.data_ptr(), d_mean_len=ml.data_ptr())
        return run
    variants = [("bsk_policy_rollout", single)] + [("bsk_population_rollout P = %d" % m, population(m)) for m in pops]
    res = {name: [] for name, _ in variants}
    for _ in range(ROUNDS):
        for name, run in variants:
            run(10)
            prop.sync()
            t0 = time.perf_counter()
            run(T)
            prop.sync()
            res[name].append((time.perf_counter() - t0) / T * 1e6)
    for name, _ in variants:
        print("%-34s us per env step: %s" % (name, ", ".join("%.1f" % x for x in res[name])))
    env.close()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "kernel":
        kernel()
    elif what == "loop":
        loop()
    elif what == "stats":
        stats(sys.argv[2], "--single-only" in sys.argv)
    else:
        sys.exit(__doc__)
