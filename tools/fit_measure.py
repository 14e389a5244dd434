#!/usr/bin/env python3
"""Cost of one step of the policy fit ("Fitting the policy"): 65 536 labelled observations, `relu [64, 64]`,
one `PolicyFit.accumulate` + `step` on an otherwise idle stream, against the same loss and an Adam step in torch f32 autograd on the
same card.

  python tools/fit_measure.py time
      device events around the pair, 30 warming and 200 timed iterations one by one, the median and the 10th / 90th percentile; the
      same around `accumulate` alone and `step` alone; then torch: `F.cross_entropy(model(x * scale + shift), labels)`,
      `backward()` and `torch.optim.Adam.step()` on float32 inputs that are already on the device, timed the same way.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o fit -- python tools/fit_measure.py kernel
      (a run of its own) 60 pairs on the null stream: DIR/.../fit_kernel_stats.csv holds the mean time of
      fit_block_kernel, fit_fold_kernel, fit_adam_kernel, fit_advance_kernel and es_center_kernel apart.
  BSKGPU_LIB=basilisk_env_amd/variants/fit_stamps.so python tools/fit_measure.py stamps
      (after `make -C basilisk_env_amd/csrc fit-stamps`) the share of fit_block_kernel's clock ticks, summed over its workgroups,
      that thread 0 spends in the weight-gradient walks - the library is a measurement build whose diagnostics row carries ticks.
  python tools/fit_measure.py pg
      the policy-gradient form ("Policy gradient") with a `[64]` value network and value targets, timed as under
      `time`: `accumulate` + `step` and `accumulate` alone (the supervised pair: with BSKGPU_LIB naming a library built from the
      parent commit this is all that runs - the parent's band, re-measured in the same session), then `accumulate_pg` + `step` and
      `accumulate_pg` alone in PPO mode with the entropy bonus on, then `bsk_gae` at 32 steps of 65 536 envs against its 52 MB of
      traffic.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o pg -- python tools/fit_measure.py pg-kernel
      (a run of its own) 60 `accumulate_pg` + `step` pairs of that set-up on the null stream: the mean time of policy_logp_kernel,
      fit_block_kernel<true>, fit_fold_kernel<8> and the step's three kernels apart.
  python tools/fit_measure.py cond
      what conditions the update as PPO2 does ("Conditioning the update"), timed as under `time` on the `pg`
      set-up: `accumulate_pg` alone, `accumulate_pg` + `step` and a `step` with nothing accumulated (with BSKGPU_LIB naming a
      library built from the parent commit this is all that runs - the parent's bands, re-measured in the same session), then the
      pair and the empty step with `max_grad_norm = 0.5`, then `bsk_adv_normalize` at 8 and at 32 rows of 65 536 against the 12 bytes
      per sample it moves (4 read twice, 4 written).
  python tools/fit_measure.py shuffle
      shuffled minibatches and the clipped value loss ("Shuffled minibatches and the clipped value loss"),
      timed as under `time` on the `pg` set-up: `accumulate_pg` alone and `accumulate_pg` + `step` (with BSKGPU_LIB naming a library
      built from the parent commit this is all that runs - the parent's bands, re-measured in the same session), then
      `accumulate_ppo` with old values and a range of 0.2, alone and with the step, then `bsk_pg_gather` of 8 x 65 536 samples out
      of histories of 32 x 65 536, all six pairs, against the 128 bytes per sample it moves (64 read, 64 written) and the 8 TB/s of
      the HBM - once by the permutation (scattered reads) and once by the identity (the same bytes, coalesced), so that the
      difference is the cost of the scatter.
  python tools/fit_measure.py pglog
      the training log of the gradient loop ("A training log for the gradient loop"), timed as under `time` on
      the `pg` set-up: `accumulate_pg` alone, `accumulate_pg` + `step`, `bsk_gae` at 32 x 65 536 and `bsk_pg_gather` of 8 x 65 536
      (with BSKGPU_LIB naming a library built from the parent commit this is all that runs - the parent's bands, re-measured in the
      same session), then `bsk_pg_episodes` at 32 x 65 536 with all histories against the 25 bytes per sample it reads, beside
      `bsk_gae` at the same shape, and `bsk_pg_log_update` + `bsk_pg_log_advance` over 128 diagnostics rows and 16 norms.
  python tools/fit_measure.py rewnorm
      the reward scaling of the gradient loop ("Scaling the rewards"), timed as under `time` on the `pg`
      set-up: `accumulate_pg` + `step`, `bsk_gae` and `bsk_pg_episodes` at 32 x 65 536 (with BSKGPU_LIB naming a library built from
      the parent commit this is all that runs - the parent's bands, re-measured in the same session), then `bsk_reward_norm` at
      that shape with `update = 1` (three launches: 9 bytes per sample read by the walk, 16 moved by the apply) and with
      `update = 0` (the apply alone, against its 16 bytes per sample), out of place and in place.
  python tools/fit_measure.py sched
      schedules and the KL stop ("Schedules and a KL stop"), timed as under `time` on the `pg` set-up:
      `accumulate_ppo` (old log-probabilities, old values, a range of 0.2) + `step`, unscheduled (with BSKGPU_LIB naming a library
      built from the parent commit this is all that runs - the parent's band, re-measured in the same session), then the same pair
      with a schedule attached - the scheduled instantiations of the block and the Adam kernel -, `bsk_fit_schedule_begin` +
      `bsk_fit_schedule_end` together (into a ring of 64 rows) and one `bsk_fit_kl_gate` over 8 rows.
  python tools/fit_measure.py host [POLICY_FIT.py]
      what the HOST spends enqueuing one update ("One reader for the device arguments"): the wall time
      (`time.perf_counter`) of `PolicyGradient.update()` from the call to its return, nothing waited for in between - 4 096 envs,
      32 steps, 4 epochs of 4 minibatches, `shuffle=True, normalize_advantages=True, cliprange_vf=0.2`, `fit.max_grad_norm = 0.5`:
      PPO2's update, 468 calls into the library and the runtime.  10 warming and 100 timed calls with a `sync()` of the env between
      them, outside the timed region; the median and the 10th / 90th percentile.  With POLICY_FIT.py that file is loaded in the place
      of basilisk_env_amd/policy_fit.py - the parent commit's (`git show HEAD~1:basilisk_env_amd/policy_fit.py`) over the same
      library is the band to compare with, re-measured in the same session.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, HIDDEN, WARM, ITERS = 65536, (64, 64), 30, 200


def _setup():
    import torch
    from _policy_bounds import observation_like, seeded_policy
    from basilisk_env_amd import policy as P
    spec, params = seeded_policy(HIDDEN, "relu", seed=1)
    obs = observation_like(N, 3)
    labels = np.where(obs[3] < 0.4, 1, np.where(obs[2] > 0.7, 2, 0)).astype(np.int32)
    pol = P.DevicePolicy(spec, params)
    fit = P.PolicyFit(pol, lr=1e-3)
    return torch, P, spec, params, obs, labels, pol, fit


def _timed(torch, stream, fn):
    """-> microseconds per call: (median, p10, p90) of ITERS calls, each between two events on ``stream``"""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ITERS)]
    for a, b in ev:
        a.record(stream)
        fn()
        b.record(stream)
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) for a, b in ev]) * 1e3
    return float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))


def time_():
    torch, P, spec, params, obs, labels, pol, fit = _setup()
    side = torch.cuda.Stream()
    d_obs, d_lab = torch.from_numpy(obs).cuda(), torch.from_numpy(labels).cuda()
    torch.cuda.synchronize()
    s = side.cuda_stream
    with torch.cuda.stream(side):
        def pair():
            fit.accumulate(d_obs, d_lab, stream=s)
            fit.step(s)
        for name, fn in (("accumulate + step", pair), ("accumulate alone", lambda: fit.accumulate(d_obs, d_lab, stream=s)),
                         ("step alone", lambda: fit.step(s))):
            print("device  %-18s %8.1f us  (p10 %.1f, p90 %.1f)" % ((name,) + _timed(torch, side, fn)))
        row = fit.stats()
        print("device  last row: mean cross-entropy %.4f, correct %d of %d" % (row["nll_sum"] / row["count"], row["correct"], row["count"]))

        scale, shift, layers, _ = P.unpack_params(spec, params)
        mods = []
        for k, (W, b) in enumerate(layers):
            lin = torch.nn.Linear(W.shape[1], W.shape[0])
            with torch.no_grad():
                lin.weight.copy_(torch.from_numpy(W.copy()))
                lin.bias.copy_(torch.from_numpy(b.copy()))
            mods += [lin] + ([torch.nn.ReLU()] if k + 1 < len(layers) else [])
        model = torch.nn.Sequential(*mods).cuda()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        x = torch.from_numpy(obs.T.astype(np.float32).copy()).cuda()
        sc, sh = torch.from_numpy(scale.copy()).cuda(), torch.from_numpy(shift.copy()).cuda()
        y = d_lab.long()

        def torch_step():
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(model(x * sc + sh), y)
            loss.backward()
            opt.step()
        print("torch   %-18s %8.1f us  (p10 %.1f, p90 %.1f)" % (("f32 autograd + Adam",) + _timed(torch, side, torch_step)))
    fit.close()
    pol.close()


def kernel():
    torch, P, spec, params, obs, labels, pol, fit = _setup()
    d_obs, d_lab = torch.from_numpy(obs).cuda(), torch.from_numpy(labels).cuda()
    torch.cuda.synchronize()
    for _ in range(60):
        fit.accumulate(d_obs, d_lab)
        fit.step()
    torch.cuda.synchronize()
    fit.close()
    pol.close()


def stamps():
    if "fit_stamps" not in os.environ.get("BSKGPU_LIB", ""):
        sys.exit("run with BSKGPU_LIB=<...>/variants/fit_stamps.so (make -C basilisk_env_amd/csrc fit-stamps)")
    torch, P, spec, params, obs, labels, pol, fit = _setup()
    d_obs, d_lab = torch.from_numpy(obs).cuda(), torch.from_numpy(labels).cuda()
    torch.cuda.synchronize()
    for _ in range(3):
        fit.accumulate(d_obs, d_lab)
    row = fit.stats()
    walk, whole = row["nll_sum"], row["value_loss_sum"]
    print("stamps  fit_block_kernel, %d workgroups: weight-gradient walks %.0f of %.0f ticks of thread 0 = %.1f %%"
          % ((N + 63) // 64, walk, whole, 100.0 * walk / whole))
    fit.close()
    pol.close()


def pg(trace=False):
    import torch
    from _policy_bounds import observation_like, seeded_policy
    from basilisk_env_amd import _lib
    from basilisk_env_amd import policy as P
    spec, params = seeded_policy(HIDDEN, "relu", (64,), seed=1)
    obs = observation_like(N, 3)
    rng = np.random.default_rng(5)
    labels = np.where(obs[3] < 0.4, 1, np.where(obs[2] > 0.7, 2, 0)).astype(np.int32)
    pol = P.DevicePolicy(spec, params)
    fit = P.PolicyFit(pol, lr=1e-3)
    side = torch.cuda.Stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    d_obs, d_lab, d_tgt = dev(obs), dev(labels), dev(rng.normal(size=N))
    s = side.cuda_stream
    if trace:
        d_adv, d_old = dev(rng.normal(size=N).astype(np.float32)), dev((-1.1 + rng.normal(0.0, 0.3, N)).astype(np.float32))
        torch.cuda.synchronize()
        for _ in range(60):
            fit.accumulate_pg(d_obs, d_lab, d_adv, d_old, 0.2, 0.01, d_tgt)
            fit.step()
        torch.cuda.synchronize()
        fit.close()
        pol.close()
        return
    with torch.cuda.stream(side):
        def pair():
            fit.accumulate(d_obs, d_lab, d_tgt, stream=s)
            fit.step(s)
        for name, fn in (("accumulate + step", pair), ("accumulate alone", lambda: fit.accumulate(d_obs, d_lab, d_tgt, stream=s))):
            print("device  %-22s %8.1f us  (p10 %.1f, p90 %.1f)" % ((name,) + _timed(torch, side, fn)))
        if hasattr(_lib.load(), "bsk_fit_accumulate_pg"):
            # old log-probabilities 0.3 away from the policy's own, as in tests/test_gpu_pg.py: a good share of the samples is clipped
            res = pol.act(d_obs, "greedy", want=("logits",), stream=s)
            torch.cuda.synchronize()
            from _device_bits import download
            l = download(res["logits"].__cuda_array_interface__["data"][0], np.float32, 3 * N).reshape(3, N).astype(np.float64)
            z = l - l.max(axis=0)
            lpa = (z - np.log(np.exp(z).sum(axis=0)))[labels, np.arange(N)]
            d_adv, d_old = dev(rng.normal(size=N).astype(np.float32)), dev((lpa + rng.normal(0.0, 0.3, N)).astype(np.float32))

            def pg_pair():
                fit.accumulate_pg(d_obs, d_lab, d_adv, d_old, 0.2, 0.01, d_tgt, stream=s)
                fit.step(s)
            for name, fn in (("accumulate_pg + step", pg_pair),
                             ("accumulate_pg alone", lambda: fit.accumulate_pg(d_obs, d_lab, d_adv, d_old, 0.2, 0.01, d_tgt, stream=s))):
                print("device  %-22s %8.1f us  (p10 %.1f, p90 %.1f)" % ((name,) + _timed(torch, side, fn)))
            row = fit.pg_stats()
            print("device  last row: clipped %d of %d" % (row["clipped"], fit.stats()["count"]))
            T = 32
            d_rew, d_val = dev(rng.normal(size=(T, N))), dev(rng.normal(size=(T, N)).astype(np.float32))
            d_why = dev((rng.uniform(size=(T, N)) < 0.02).astype(np.uint8))
            d_a, d_r = torch.empty((T, N), dtype=torch.float32, device="cuda"), torch.empty((T, N), dtype=torch.float64, device="cuda")
            med, p10, p90 = _timed(torch, side, lambda: P.gae(d_rew, d_why, d_val, None, T, N, d_a, d_r, stream=s))
            print("device  %-22s %8.1f us  (p10 %.1f, p90 %.1f): %.0f GB/s of its %.1f MB" % ("bsk_gae 32 x 65536", med, p10, p90,
                                                                                          25.0 * T * N / med * 1e-3, 25.0 * T * N * 1e-6))
    fit.close()
    pol.close()


def cond():
    import torch
    from _policy_bounds import observation_like, seeded_policy
    from basilisk_env_amd import _lib
    from basilisk_env_amd import policy as P
    spec, params = seeded_policy(HIDDEN, "relu", (64,), seed=1)
    obs = observation_like(N, 3)
    rng = np.random.default_rng(5)
    labels = np.where(obs[3] < 0.4, 1, np.where(obs[2] > 0.7, 2, 0)).astype(np.int32)
    pol = P.DevicePolicy(spec, params)
    fit = P.PolicyFit(pol, lr=1e-3)
    side = torch.cuda.Stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    d_obs, d_lab, d_tgt = dev(obs), dev(labels), dev(rng.normal(size=N))
    d_adv, d_old = dev(rng.normal(size=N).astype(np.float32)), dev((-1.1 + rng.normal(0.0, 0.3, N)).astype(np.float32))
    s = side.cuda_stream
    new = hasattr(_lib.load(), "bsk_adv_normalize")
    with torch.cuda.stream(side):
        def acc():
            fit.accumulate_pg(d_obs, d_lab, d_adv, d_old, 0.2, 0.01, d_tgt, stream=s)

        def step():                        # (a step moves something only behind an accumulate: the pair, minus the accumulate alone)
            acc()
            fit.step(s)
        print("device  %-26s %8.1f us  (p10 %.1f, p90 %.1f)" % (("accumulate_pg alone",) + _timed(torch, side, acc)))
        print("device  %-26s %8.1f us  (p10 %.1f, p90 %.1f)" % (("accumulate_pg + step",) + _timed(torch, side, step)))
        print("device  %-26s %8.1f us  (p10 %.1f, p90 %.1f)" % (("step alone (count == 0)",) + _timed(torch, side, lambda: fit.step(s))))
        if new:
            fit.max_grad_norm = 0.5
            print("device  %-26s %8.1f us  (p10 %.1f, p90 %.1f)" % (("accumulate_pg + clipped step",) + _timed(torch, side, step)))
            print("device  %-26s %8.1f us  (p10 %.1f, p90 %.1f)" % (("clipped step alone (count == 0)",) + _timed(torch, side, lambda: fit.step(s))))
            print("device  last clipped step: %r" % (fit.grad_norm(),))
            for T in (8, 32):
                d_a = dev(rng.normal(size=(T, N)).astype(np.float32))
                d_o = torch.empty((T, N), dtype=torch.float32, device="cuda")
                work = torch.empty(P.adv_normalize_work_bytes(N) // 8, dtype=torch.float64, device="cuda")
                med, p10, p90 = _timed(torch, side, lambda: P.normalize_advantages(d_a, T, N, d_o, work=work, stream=s))
                print("device  %-26s %8.1f us  (p10 %.1f, p90 %.1f): %.0f GB/s of its %.1f MB" % ("bsk_adv_normalize %d x 65536" % T, med, p10, p90,
                                                                                              12.0 * T * N / med * 1e-3, 12.0 * T * N * 1e-6))
    fit.close()
    pol.close()


def shuffle():
    import torch
    from _policy_bounds import observation_like, seeded_policy
    from basilisk_env_amd import _lib
    from basilisk_env_amd import policy as P
    spec, params = seeded_policy(HIDDEN, "relu", (64,), seed=1)
    obs = observation_like(N, 3)
    rng = np.random.default_rng(5)
    labels = np.where(obs[3] < 0.4, 1, np.where(obs[2] > 0.7, 2, 0)).astype(np.int32)
    pol = P.DevicePolicy(spec, params)
    fit = P.PolicyFit(pol, lr=1e-3)
    side = torch.cuda.Stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    tgt = rng.normal(size=N)
    d_obs, d_lab, d_tgt = dev(obs), dev(labels), dev(tgt)
    d_adv, d_old = dev(rng.normal(size=N).astype(np.float32)), dev((-1.1 + rng.normal(0.0, 0.3, N)).astype(np.float32))
    s = side.cuda_stream
    new = hasattr(_lib.load(), "bsk_pg_gather")
    line = "device  %-30s %8.1f us  (p10 %.1f, p90 %.1f)"
    with torch.cuda.stream(side):
        def acc():
            fit.accumulate_pg(d_obs, d_lab, d_adv, d_old, 0.2, 0.01, d_tgt, stream=s)

        def step():
            acc()
            fit.step(s)
        print(line % (("accumulate_pg alone",) + _timed(torch, side, acc)))
        print(line % (("accumulate_pg + step",) + _timed(torch, side, step)))
        if new:
            # old values 0.3 away from the targets' scale: a good share of the samples leaves the range of 0.2
            d_vold = dev(rng.normal(0.0, 0.3, N).astype(np.float32))

            def ppo():
                fit.accumulate_ppo(d_obs, d_lab, d_adv, d_old, 0.2, 0.01, d_tgt, d_vold, 0.2, stream=s)

            def ppo_step():
                ppo()
                fit.step(s)
            print(line % (("accumulate_ppo alone",) + _timed(torch, side, ppo)))
            print(line % (("accumulate_ppo + step",) + _timed(torch, side, ppo_step)))
            ppo()
            print("device  last row: value-clipped %d of %d" % (fit.vclip_stats()["value_clipped"], fit.stats()["count"]))
            T, rows = 32, 8
            m = rows * N
            hist = dict(obs=dev(rng.normal(size=(T, 5, N))), action=dev(rng.integers(0, 3, (T, N)).astype(np.int32)),
                        adv=dev(rng.normal(size=(T, N)).astype(np.float32)), logp=dev(rng.normal(size=(T, N)).astype(np.float32)),
                        ret=dev(rng.normal(size=(T, N))), value=dev(rng.normal(size=(T, N)).astype(np.float32)))
            out = dict(obs=torch.empty((5, m), dtype=torch.float64, device="cuda"), action=torch.empty(m, dtype=torch.int32, device="cuda"),
                       adv=torch.empty(m, dtype=torch.float32, device="cuda"), logp=torch.empty(m, dtype=torch.float32, device="cuda"),
                       ret=torch.empty(m, dtype=torch.float64, device="cuda"), value=torch.empty(m, dtype=torch.float32, device="cuda"))
            state = dev(np.array([1, 0], np.int64))
            names = ("obs", "action", "adv", "logp", "ret", "value")
            print("device  histories %.0f MB, one minibatch %.0f MB" % (64.0 * T * N * 1e-6, 64.0 * m * 1e-6))
            for what, st in (("bsk_pg_gather 8 of 32 x 65536", state), ("the same by the identity", None)):
                med, p10, p90 = _timed(torch, side, lambda: P.pg_gather(st, T, N, m, m, *[hist[k] for k in names],
                                                                        *[out[k] for k in names], stream=s))
                print((line + ": %.0f GB/s of its %.1f MB, %.1f %% of 8 TB/s") % (what, med, p10, p90, 128.0 * m / med * 1e-3, 128.0 * m * 1e-6,
                                                                              100.0 * 128.0 * m / med * 1e-3 / 8000.0))
    fit.close()
    pol.close()


def pglog():
    import torch
    from _policy_bounds import observation_like, seeded_policy
    from basilisk_env_amd import _lib
    from basilisk_env_amd import policy as P
    spec, params = seeded_policy(HIDDEN, "relu", (64,), seed=1)
    obs = observation_like(N, 3)
    rng = np.random.default_rng(5)
    labels = np.where(obs[3] < 0.4, 1, np.where(obs[2] > 0.7, 2, 0)).astype(np.int32)
    pol = P.DevicePolicy(spec, params)
    fit = P.PolicyFit(pol, lr=1e-3)
    side = torch.cuda.Stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    d_obs, d_lab, d_tgt = dev(obs), dev(labels), dev(rng.normal(size=N))
    d_adv, d_old = dev(rng.normal(size=N).astype(np.float32)), dev((-1.1 + rng.normal(0.0, 0.3, N)).astype(np.float32))
    s = side.cuda_stream
    new = hasattr(_lib.load(), "bsk_pg_episodes")
    line = "device  %-34s %8.1f us  (p10 %.1f, p90 %.1f)"
    with torch.cuda.stream(side):
        def acc():
            fit.accumulate_pg(d_obs, d_lab, d_adv, d_old, 0.2, 0.01, d_tgt, stream=s)

        def step():
            acc()
            fit.step(s)
        print(line % (("accumulate_pg alone",) + _timed(torch, side, acc)))
        print(line % (("accumulate_pg + step",) + _timed(torch, side, step)))
        T, rows = 32, 8
        m = rows * N
        hist = dict(obs=dev(rng.normal(size=(T, 5, N))), action=dev(rng.integers(0, 3, (T, N)).astype(np.int32)),
                    adv=torch.empty((T, N), dtype=torch.float32, device="cuda"), logp=dev(rng.normal(size=(T, N)).astype(np.float32)),
                    ret=torch.empty((T, N), dtype=torch.float64, device="cuda"), value=dev(rng.normal(size=(T, N)).astype(np.float32)))
        d_rew = dev(rng.normal(size=(T, N)))
        d_why = dev(((rng.uniform(size=(T, N)) < 0.02) * rng.choice([1, 2, 4, 8], (T, N))).astype(np.uint8))
        gae_t = _timed(torch, side, lambda: P.gae(d_rew, d_why, hist["value"], None, T, N, hist["adv"], hist["ret"], stream=s))
        print((line + ": %.0f GB/s of its %.1f MB") % (("bsk_gae 32 x 65536",) + gae_t + (25.0 * T * N / gae_t[0] * 1e-3, 25.0 * T * N * 1e-6)))
        out = dict(obs=torch.empty((5, m), dtype=torch.float64, device="cuda"), action=torch.empty(m, dtype=torch.int32, device="cuda"),
                   adv=torch.empty(m, dtype=torch.float32, device="cuda"), logp=torch.empty(m, dtype=torch.float32, device="cuda"),
                   ret=torch.empty(m, dtype=torch.float64, device="cuda"), value=torch.empty(m, dtype=torch.float32, device="cuda"))
        state = dev(np.array([1, 0], np.int64))
        names = ("obs", "action", "adv", "logp", "ret", "value")
        print(line % (("bsk_pg_gather 8 of 32 x 65536",) + _timed(torch, side, lambda: P.pg_gather(state, T, N, m, m, *[hist[k] for k in names],
                                                                                                  *[out[k] for k in names], stream=s))))
        if new:
            cap = 64
            ep_R, ep_L = torch.zeros(N, dtype=torch.float64, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
            work = torch.zeros(P.pg_episodes_work_bytes(N) // 8, dtype=torch.float64, device="cuda")
            ring = torch.zeros(cap * P.PG_LOG_COLS, dtype=torch.float64, device="cuda")
            gen, counter = dev(np.full(cap, -1, np.int64)), dev(np.zeros(1, np.int64))
            ep_t = _timed(torch, side, lambda: P.pg_episodes(d_rew, d_why, T, N, ep_R, ep_L, work, ring, cap, counter, hist["action"],
                                                             hist["value"], hist["ret"], stream=s))
            print((line + ": %.0f GB/s of its %.1f MB") % (("bsk_pg_episodes 32 x 65536",) + ep_t + (25.0 * T * N / ep_t[0] * 1e-3, 25.0 * T * N * 1e-6)))
            gae_again = _timed(torch, side, lambda: P.gae(d_rew, d_why, hist["value"], None, T, N, hist["adv"], hist["ret"], stream=s))
            print(line % (("bsk_gae 32 x 65536 again",) + gae_again))
            print("device  bsk_pg_episodes / bsk_gae: %.2f (medians; against the second bsk_gae %.2f)" % (ep_t[0] / gae_t[0], ep_t[0] / gae_again[0]))
            d_diag, d_norms = dev(rng.normal(size=(128, 8))), dev(np.stack([rng.uniform(0.1, 1.0, 16), rng.uniform(0.5, 1.0, 16)], axis=1))

            def tail():
                P.pg_log_update(d_diag, 128, ring, cap, counter, d_norms, 16, stream=s)
                P.pg_log_advance(gen, cap, counter, s)
            print(line % (("pg_log_update + pg_log_advance",) + _timed(torch, side, tail)))
            P.pg_episodes(d_rew, d_why, T, N, ep_R, ep_L, work, ring, cap, counter, hist["action"], hist["value"], hist["ret"], stream=s)
            tail()                                             # (one whole row behind the timed ones, which wrote their halves apart)
            torch.cuda.synchronize()
            it, table = P.pg_log_table_ref(gen.cpu().numpy().view(np.uint64), ring.cpu().numpy())
            print("device  ring: %d of %d slots written, iterations %d .. %d; last row: %d episodes of mean length %.1f, explained variance %.4f"
                  % (it.size, cap, it[0], it[-1], table[-1, 0], table[-1, 5] / max(table[-1, 0], 1.0), table[-1, 14]))
    fit.close()
    pol.close()


def rewnorm():
    import torch
    from _policy_bounds import observation_like, seeded_policy
    from basilisk_env_amd import _lib
    from basilisk_env_amd import policy as P
    spec, params = seeded_policy(HIDDEN, "relu", (64,), seed=1)
    obs = observation_like(N, 3)
    rng = np.random.default_rng(5)
    labels = np.where(obs[3] < 0.4, 1, np.where(obs[2] > 0.7, 2, 0)).astype(np.int32)
    pol = P.DevicePolicy(spec, params)
    fit = P.PolicyFit(pol, lr=1e-3)
    side = torch.cuda.Stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    d_obs, d_lab, d_tgt = dev(obs), dev(labels), dev(rng.normal(size=N))
    d_adv, d_old = dev(rng.normal(size=N).astype(np.float32)), dev((-1.1 + rng.normal(0.0, 0.3, N)).astype(np.float32))
    s = side.cuda_stream
    new = hasattr(_lib.load(), "bsk_reward_norm")
    line = "device  %-34s %8.1f us  (p10 %.1f, p90 %.1f)"
    with torch.cuda.stream(side):
        def step():
            fit.accumulate_pg(d_obs, d_lab, d_adv, d_old, 0.2, 0.01, d_tgt, stream=s)
            fit.step(s)
        print(line % (("accumulate_pg + step",) + _timed(torch, side, step)))
        T = 32
        d_act, d_val = dev(rng.integers(0, 3, (T, N)).astype(np.int32)), dev(rng.normal(size=(T, N)).astype(np.float32))
        d_gae, d_ret = torch.empty((T, N), dtype=torch.float32, device="cuda"), torch.empty((T, N), dtype=torch.float64, device="cuda")
        d_rew = dev(rng.normal(size=(T, N)))
        d_why = dev(((rng.uniform(size=(T, N)) < 0.02) * rng.choice([1, 2, 4, 8], (T, N))).astype(np.uint8))
        gae_t = _timed(torch, side, lambda: P.gae(d_rew, d_why, d_val, None, T, N, d_gae, d_ret, stream=s))
        print((line + ": %.0f GB/s of its %.1f MB") % (("bsk_gae 32 x 65536",) + gae_t + (25.0 * T * N / gae_t[0] * 1e-3, 25.0 * T * N * 1e-6)))
        cap = 64
        ep_R, ep_L = torch.zeros(N, dtype=torch.float64, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
        ep_work = torch.zeros(P.pg_episodes_work_bytes(N) // 8, dtype=torch.float64, device="cuda")
        ring, counter = torch.zeros(cap * P.PG_LOG_COLS, dtype=torch.float64, device="cuda"), dev(np.zeros(1, np.int64))
        ep_t = _timed(torch, side, lambda: P.pg_episodes(d_rew, d_why, T, N, ep_R, ep_L, ep_work, ring, cap, counter, d_act, d_val, d_ret,
                                                         stream=s))
        print((line + ": %.0f GB/s of its %.1f MB") % (("bsk_pg_episodes 32 x 65536",) + ep_t + (25.0 * T * N / ep_t[0] * 1e-3, 25.0 * T * N * 1e-6)))
        if new:
            state = torch.zeros(P.REWARD_NORM_STATE_WORDS, dtype=torch.int64, device="cuda")
            ret_run = torch.zeros(N, dtype=torch.float64, device="cuda")
            work = torch.zeros(P.reward_norm_work_bytes(N) // 8, dtype=torch.float64, device="cuda")
            d_out = torch.empty((T, N), dtype=torch.float64, device="cuda")
            d_inplace = d_rew.clone()
            print("device  buffers: rewards %.1f MB, reasons %.1f MB, output %.1f MB - all inside the 256 MB last-level cache"
                  % (8.0 * T * N * 1e-6, 1.0 * T * N * 1e-6, 8.0 * T * N * 1e-6))
            up = _timed(torch, side, lambda: P.reward_normalize(d_rew, d_why, T, N, state, d_out, ret_run, work, 0.99, 1e-8, 10.0, True, stream=s))
            print((line + ": the walk reads %.1f MB, the apply moves %.1f MB") % (("bsk_reward_norm update = 1",) + up + (9.0 * T * N * 1e-6, 16.0 * T * N * 1e-6)))
            frozen = {}
            for what, out in (("bsk_reward_norm update = 0", d_out), ("the same in place", d_inplace)):
                ap = frozen[what] = _timed(torch, side, lambda: P.reward_normalize(d_rew if out is d_out else d_inplace, d_why, T, N, state, out if out is d_out else None,
                                                                    None, None, 0.99, 1e-8, 10.0, False, stream=s))
                print((line + ": %.0f GB/s of its %.1f MB, %.1f %% of 8 TB/s") % ((what,) + ap + (16.0 * T * N / ap[0] * 1e-3, 16.0 * T * N * 1e-6,
                                                                                      100.0 * 16.0 * T * N / ap[0] * 1e-3 / 8000.0)))
            ep_again = _timed(torch, side, lambda: P.pg_episodes(d_rew, d_why, T, N, ep_R, ep_L, ep_work, ring, cap, counter, d_act, d_val, d_ret,
                                                                 stream=s))
            print(line % (("bsk_pg_episodes 32 x 65536 again",) + ep_again))
            print("device  bsk_reward_norm (update = 1) / bsk_pg_episodes: %.2f; walk + join = update 1 - update 0: %.1f us"
                  % (up[0] / ep_again[0], up[0] - frozen["bsk_reward_norm update = 0"][0]))
            torch.cuda.synchronize()
            words = state.cpu().numpy().view(np.uint64)
            print("device  state: %d updating calls, %d returns, sd %.4f" % (words[6], words[2], words.view(np.float64)[5]))
    fit.close()
    pol.close()


def sched():
    import torch
    from _policy_bounds import observation_like, seeded_policy
    from basilisk_env_amd import _lib
    from basilisk_env_amd import policy as P
    spec, params = seeded_policy(HIDDEN, "relu", (64,), seed=1)
    obs = observation_like(N, 3)
    rng = np.random.default_rng(5)
    labels = np.where(obs[3] < 0.4, 1, np.where(obs[2] > 0.7, 2, 0)).astype(np.int32)
    pol = P.DevicePolicy(spec, params)
    fit = P.PolicyFit(pol, lr=1e-3)
    side = torch.cuda.Stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    d_obs, d_lab, d_tgt = dev(obs), dev(labels), dev(rng.normal(size=N))
    d_adv, d_old = dev(rng.normal(size=N).astype(np.float32)), dev((-1.1 + rng.normal(0.0, 0.3, N)).astype(np.float32))
    d_vold = dev(rng.normal(size=N).astype(np.float32))
    s = side.cuda_stream
    new = hasattr(_lib.load(), "bsk_fit_set_schedule")
    line = "device  %-40s %8.1f us  (p10 %.1f, p90 %.1f)"
    with torch.cuda.stream(side):
        def step():
            fit.accumulate_ppo(d_obs, d_lab, d_adv, d_old, 0.2, 0.01, d_tgt, d_vold, 0.2, stream=s)
            fit.step(s)
        plain = _timed(torch, side, step)
        print(line % (("accumulate_ppo + step",) + plain))
        if new:
            cap = 64
            ring = torch.full((cap, len(P.SCHED_LOG_COLUMNS)), -1, dtype=torch.int64, device="cuda").view(torch.float64)
            rows = dev(np.tile(np.array([[3.0, 60.0, 5.0, 1.0, 70.0, 30.0, 40000.0, 65536.0]]), (8, 1)))
            fit.set_schedule(10 ** 6, (1e-3, 0.0), (0.2, 0.05), (0.2, 0.2), (0.01, 0.0), kl_stop=1e3)
            with_words = _timed(torch, side, step)
            print(line % (("the same, scheduled",) + with_words))
            print("device  scheduled median - unscheduled p90: %+.1f us; the unscheduled band is %.1f us wide"
                  % (with_words[0] - plain[2], plain[2] - plain[1]))

            def around():
                fit.schedule_begin(s)
                fit.schedule_end(ring, cap, s)
            print(line % (("schedule_begin + schedule_end",) + _timed(torch, side, around)))
            print(line % (("kl_gate over 8 rows",) + _timed(torch, side, lambda: fit.kl_gate(rows, 8, s))))
            print(line % (("accumulate_ppo + step, scheduled, again",) + _timed(torch, side, step)))
            fit.clear_schedule()
            print(line % (("accumulate_ppo + step, unscheduled, again",) + _timed(torch, side, step)))
            torch.cuda.synchronize()
            fit.set_schedule(10 ** 6, (1e-3, 0.0), (0.2, 0.05), (0.2, 0.2), (0.01, 0.0), kl_stop=1e3)
            fit.set_schedule_state(WARM + ITERS)
            st = fit.schedule_state()
            print("device  words at iteration %d of 10^6: lr %.6e, clip %.6f; gate %d" % (st["iteration"], st["lr"], st["clip"], st["gate"]))
    fit.close()
    pol.close()


def host():
    import importlib.util
    import time
    if len(sys.argv) > 2:                      # (before anything imports the package's own)
        mod_spec = importlib.util.spec_from_file_location("basilisk_env_amd.policy_fit", sys.argv[2])
        sys.modules[mod_spec.name] = mod = importlib.util.module_from_spec(mod_spec)
        mod_spec.loader.exec_module(mod)
    import torch
    from _policy_bounds import seeded_policy
    from basilisk_env_amd import policy as P
    from basilisk_env_amd._lib import FLAG_AUTO_RESET, GRAV_PM_J2
    from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
    from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
    which = os.path.relpath(sys.modules["basilisk_env_amd.policy_fit"].__file__, ROOT)
    n, T, warm, iters = 4096, 32, 10, 100
    spec, params = seeded_policy(HIDDEN, "relu", (64,), seed=1)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        cfg = default_config(4, GRAV_PM_J2)
        cfg.flags |= FLAG_AUTO_RESET
        root = BatchedPropagator(cfg, n, stream=side.cuda_stream)
        root.set_ic_pool(sample_ic_batch(64, 4, seed=73))
        root.reset(sample_ic_batch(n, 4, seed=72))
        root.step(np.zeros(n, np.int32), 1)                     # (the observation buffers hold a step's output)
        pol = P.DevicePolicy(spec, params)
        fit = P.PolicyFit(pol, lr=1e-3)
        fit.max_grad_norm = 0.5
        pg = P.PolicyGradient(root, pol, fit, T, epochs=4, minibatches=4, shuffle=True, normalize_advantages=True, cliprange_vf=0.2)
        pg.collect()
        root.sync()
        t = []
        for _ in range(warm + iters):
            t0 = time.perf_counter()
            pg.update()
            t.append(time.perf_counter() - t0)
            root.sync()
        t = np.array(t[warm:]) * 1e6
        print("host    %-36s update() %8.1f us  (p10 %.1f, p90 %.1f)" % (which, np.median(t), np.percentile(t, 10), np.percentile(t, 90)))
        pg.close()
    fit.close()
    pol.close()


if __name__ == "__main__":
    {"time": time_, "kernel": kernel, "stamps": stamps, "pg": pg, "pg-kernel": lambda: pg(trace=True), "cond": cond,
     "shuffle": shuffle, "pglog": pglog, "rewnorm": rewnorm, "sched": sched, "host": host}[sys.argv[1] if len(sys.argv) > 1 else "time"]()
