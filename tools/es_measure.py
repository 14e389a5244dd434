#!/usr/bin/env python3
"""Cost of a generation of the evolution strategy ("The evolution strategy on the device"): 65 536 spacecraft,
`tanh [64, 64]`, K = 1, P = 64 and 1 024 members, a 200-step generation after a warming one.

  python tools/es_measure.py loop
      host clock around one generation and a synchronisation, profiler off; three runs, alternating:
        host    the loop as it was before the optimiser moved: `EvolutionStrategy.ask` -> `set_params` -> reset from the pool ->
                `evaluate` -> `tell`
        device  `DeviceEvolutionStrategy.run_generation`
        graph   the same call captured once into a HIP graph and replayed
        rollout reset from the pool and `rollout_device` alone: what the device loop is expected to approach
        adam    `run_generation` of an optimiser created with optimizer="adam"
        shared  `run_generation(..., shared_episodes=True)`: the reset that gives all members the same episodes
        obsnorm `run_generation(..., obs_stats=...)`: one obs_stats_kernel launch in front of every policy launch, the join and
                the normalisation behind the generation
        sigma   `run_generation` of an optimiser created with sigma_adapt="pgpe": a step size per parameter, moved by tell
        log     `run_generation` of an optimiser created with log_capacity=256: two more launches in front of the update, and the
                rollout also writes the members' mean episode lengths
        validate `run_generation` of an optimiser created with validation_members=1, on a handle of its own with the envs of one
                more member (N + N / P spacecraft): V + 1 masked resets in the place of one, the centre's launch behind ask's, two
                more launches in front of the update
  python tools/es_measure.py kernel [adam | obs | sigma | log]
      per P one warming and three measured generations of `run_generation` (`adam`: of an optimizer="adam" optimiser on shared
      episodes; `obs`: with an `ObsStats` given; `sigma`: of a sigma_adapt="pgpe" optimiser; `log`: of a log_capacity=256
      optimiser).  Run it under the profiler in a run of its own:
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o es -- python tools/es_measure.py kernel
  python tools/es_measure.py stats DIR/.../es_kernel_trace.csv
      per measured generation of that run the times of es_ask_kernel, es_rank_kernel and es_tell_kernel (or es_tell_adam_kernel;
      of a `kernel sigma` run es_ask_sigma_kernel, es_rank_q_kernel and es_tell_sigma_kernel)
      and the sum over every other kernel of the generation (the generations are recognised by the es_advance_kernel or
      es_advance_adam_kernel that ends each); of a `kernel obs` run also obs_stats_kernel, per generation and per launch; of a
      `kernel log` run also es_log_kernel and es_best_kernel
"""
import csv
import os
import sys
import time

import numpy as np

N, T, WARM_T, ROUNDS = 65536, 200, 10, 3
MEMBERS = (64, 1024)
GAMMA = 0.99


def _env(n, side):
    from basilisk_env_amd.envs.leoPowerAttitudeVecEnv import LeoPowerAttVecEnv
    env = LeoPowerAttVecEnv(n, device_reset_pool=4096, device_sampler=True, stream=side.cuda_stream)
    env.reset_tensors()
    env.propagator.step(np.zeros(n, np.int32), 1)
    return env


def _setup():
    import torch
    from basilisk_env_amd import policy as P
    side = torch.cuda.Stream()
    env = _env(N, side)
    prop = env.propagator
    spec = P.check_spec((64, 64), "tanh")
    rng = np.random.default_rng(7)
    a, _ = P.layer_shapes(spec)
    layers = [(rng.normal(0.0, np.sqrt(1.0 / i), (o, i)).astype(np.float32), rng.normal(0.0, 0.3, o).astype(np.float32)) for o, i in a]
    theta = P.pack_params(spec, layers, None, [2.0, 50.0, 1.5, 1.25, 0.75], [-0.5, 0.1, -0.3, -0.6, 0.2])
    return torch, P, side, env, prop, spec, theta


def loop():
    torch, P, side, env, prop, spec, theta = _setup()
    with torch.cuda.stream(side):
        variants, val_envs = [], []
        for m in MEMBERS:
            pop = P.PolicyPopulation(spec, n_members=m)
            host = P.EvolutionStrategy(theta, m, sigma=0.1, lr=0.05, seed=1)
            dev = P.DeviceEvolutionStrategy(spec, theta, m, sigma=0.1, lr=0.05, seed=1)
            rep = P.DeviceEvolutionStrategy(spec, theta, m, sigma=0.1, lr=0.05, seed=1)
            adam = P.DeviceEvolutionStrategy(spec, theta, m, sigma=0.1, lr=0.05, seed=1, optimizer="adam")
            shared = P.DeviceEvolutionStrategy(spec, theta, m, sigma=0.1, lr=0.05, seed=1)
            normed = P.DeviceEvolutionStrategy(spec, theta, m, sigma=0.1, lr=0.05, seed=1)
            sig = P.DeviceEvolutionStrategy(spec, theta, m, sigma=0.1, lr=0.05, seed=1, sigma_adapt="pgpe")
            logged = P.DeviceEvolutionStrategy(spec, theta, m, sigma=0.1, lr=0.05, seed=1, log_capacity=256)
            obs_stats = P.ObsStats(N)
            fit = torch.zeros(m, dtype=torch.float64, device="cuda")
            # one validation member: the same P and the same envs per member, so one member's envs more on a handle of its own
            val = P.DeviceEvolutionStrategy(spec, theta, m, sigma=0.1, lr=0.05, seed=1, validation_members=1)
            val_pop = P.PolicyPopulation(spec, n_members=m + 1)
            val_envs.append(_env(N + N // m, side))

            def host_gen(steps, pop=pop, host=host):
                pop.set_params(host.ask())
                prop.reset_from_pool_device(None)
                host.tell(pop.evaluate(prop, steps, 1, "greedy", GAMMA)["fitness"])

            def device_gen(steps, pop=pop, dev=dev):
                dev.run_generation(prop, pop, steps, 1, "greedy", GAMMA)

            def rollout_gen(steps, pop=pop, fit=fit):
                prop.reset_from_pool_device(None)
                pop.rollout_device(prop, steps, 1, "greedy", GAMMA, d_fitness=fit.data_ptr())

            def adam_gen(steps, pop=pop, adam=adam):
                adam.run_generation(prop, pop, steps, 1, "greedy", GAMMA)

            def shared_gen(steps, pop=pop, shared=shared):
                shared.run_generation(prop, pop, steps, 1, "greedy", GAMMA, shared_episodes=True)

            def obsnorm_gen(steps, pop=pop, normed=normed, obs_stats=obs_stats):
                normed.run_generation(prop, pop, steps, 1, "greedy", GAMMA, obs_stats=obs_stats)

            def sigma_gen(steps, pop=pop, sig=sig):
                sig.run_generation(prop, pop, steps, 1, "greedy", GAMMA)

            def log_gen(steps, pop=pop, logged=logged):
                logged.run_generation(prop, pop, steps, 1, "greedy", GAMMA)

            def validate_gen(steps, val=val, val_pop=val_pop, val_prop=val_envs[-1].propagator):
                val.run_generation(val_prop, val_pop, steps, 1, "greedy", GAMMA)

            rep.run_generation(prop, pop, WARM_T, 1, "greedy", GAMMA)
            prop.sync()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                rep.run_generation(prop, pop, T, 1, "greedy", GAMMA)

            def graph_gen(steps, graph=graph):
                if steps == T:
                    graph.replay()

            variants += [("host   P = %d" % m, host_gen), ("device P = %d" % m, device_gen), ("graph  P = %d" % m, graph_gen),
                         ("rollout P = %d" % m, rollout_gen), ("adam   P = %d" % m, adam_gen), ("shared P = %d" % m, shared_gen),
                         ("obsnorm P = %d" % m, obsnorm_gen), ("sigma  P = %d" % m, sigma_gen), ("log    P = %d" % m, log_gen),
                         ("validate P = %d" % m, validate_gen)]
        res = {name: [] for name, _ in variants}
        for _ in range(ROUNDS):
            for name, run in variants:
                run(WARM_T)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(T)
                torch.cuda.synchronize()
                res[name].append((time.perf_counter() - t0) * 1e6)
        for name, _ in variants:
            print("%-18s us per %d-step generation: %s" % (name, T, ", ".join("%.0f" % x for x in res[name])))
    for e in val_envs:
        e.close()
    env.close()


def kernel(adam=False, obs=False, sigma=False, log=False):
    torch, P, side, env, prop, spec, theta = _setup()
    with torch.cuda.stream(side):
        for m in MEMBERS:
            pop = P.PolicyPopulation(spec, n_members=m)
            dev = P.DeviceEvolutionStrategy(spec, theta, m, sigma=0.1, lr=0.05, seed=1, optimizer="adam" if adam else "sgd",
                                            sigma_adapt="pgpe" if sigma else None, log_capacity=256 if log else 0)
            obs_stats = P.ObsStats(N) if obs else None
            dev.run_generation(prop, pop, WARM_T, 1, "greedy", GAMMA, shared_episodes=adam, obs_stats=obs_stats)
            for _ in range(ROUNDS):
                dev.run_generation(prop, pop, T, 1, "greedy", GAMMA, shared_episodes=adam, obs_stats=obs_stats)
            prop.sync()
    print("per P in %r: one warming generation of %d steps, then %d of %d steps" % (MEMBERS, WARM_T, ROUNDS, T))
    env.close()


def stats(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    gens, cur, seen = [], {}, False
    for _, d, name in rows:
        key = next((k for k in ("es_ask_kernel", "es_rank_kernel", "es_tell_kernel", "es_advance_kernel", "obs_stats_kernel", "es_log_kernel",
                                "es_best_kernel")
                    if k in name.replace("_adam", "").replace("_sigma", "").replace("es_rank_q", "es_rank")), "rest")
        seen = seen or key == "es_ask_kernel"
        if not seen:
            continue                           # (the set-up's launches, before the first generation)
        cur[key] = cur.get(key, 0) + d
        if key == "es_advance_kernel":
            gens.append(cur)
            cur = {}
    assert len(gens) == len(MEMBERS) * (1 + ROUNDS), len(gens)
    for b, m in enumerate(MEMBERS):
        for g in gens[b * (1 + ROUNDS) + 1:(b + 1) * (1 + ROUNDS)]:
            # (tell: es_tell_kernel, or es_tell_adam_kernel in a `kernel adam` run; the *_sigma kernels and es_rank_q_kernel in a
            # `kernel sigma` run)
            print("P = %-5d ask %8.1f us, rank %7.1f us, tell %8.1f us, every other kernel of the generation %9.1f us" %
                  (m, g["es_ask_kernel"] / 1e3, g["es_rank_kernel"] / 1e3, g["es_tell_kernel"] / 1e3, g["rest"] / 1e3))
            if "obs_stats_kernel" in g:        # (a `kernel obs` run: T launches per generation, one in front of every policy launch)
                print("          obs_stats_kernel %8.1f us per generation, %.2f us per launch" %
                      (g["obs_stats_kernel"] / 1e3, g["obs_stats_kernel"] / 1e3 / T))
            if "es_log_kernel" in g:           # (a `kernel log` run: one launch of each per generation, in front of the update)
                print("          es_log_kernel %6.1f us, es_best_kernel %6.1f us" % (g["es_log_kernel"] / 1e3, g["es_best_kernel"] / 1e3))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "loop":
        loop()
    elif what == "kernel":
        kernel(adam=sys.argv[2:3] == ["adam"], obs=sys.argv[2:3] == ["obs"], sigma=sys.argv[2:3] == ["sigma"],
               log=sys.argv[2:3] == ["log"])
    elif what == "stats":
        stats(sys.argv[2])
    else:
        sys.exit(__doc__)
