#!/usr/bin/env python3
"""Role probe of the halves form: probe libraries variants/probe_halves_role{1,2}.so (make -C basilisk_env_amd/csrc probe-libs
PROBES="halves_role1:-DBSK_PROBE_HALVES_ROLE=1 halves_role2:-DBSK_PROBE_HALVES_ROLE=2"), one ROLE each.  Rotational wave (1): cycles
from its start to the hand-over (its arrival at the form's last barrier) and from the hand-over to its last instruction.
Translational wave (2): cycles waiting at that barrier and from the barrier to its last instruction.  Mean, median and the 5 % / 95 %
quantiles over the batch's workgroups, over launches without an FSW tick (phases 1 .. 8 of 10) and, apart, the launch with one.
Each library is loaded in a child process.
usage: halves_roles.py [N [LAUNCHES [SEED [DIR]]]]      (GPU box; DIR: where the two libraries are, default basilisk_env_amd/variants)"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 200
seed = int(sys.argv[3]) if len(sys.argv) > 3 else 7
here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
libdir = sys.argv[4] if len(sys.argv) > 4 else os.path.join(here, "basilisk_env_amd", "variants")
role = int(os.environ.get("HALVES_ROLE_CHILD", "0"))
names = ("rotational wave   ", "translational wave")
fields = (("start -> hand-over", "hand-over -> end"), ("waiting at the barrier", "barrier -> end"))
if role == 0:
    import subprocess
    for r in (1, 2):
        env = dict(os.environ, HALVES_ROLE_CHILD=str(r), BSKGPU_LIB=os.path.join(libdir, "probe_halves_role%d.so" % r))
        res = subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, capture_output=True, text=True)
        sys.stdout.write(res.stdout if res.returncode == 0 else "role %d failed: %s\n" % (r, res.stderr[-500:]))
        if res.returncode != 0:
            sys.exit(1)                                             # (nothing more is started on the GPU after a failure)
    sys.exit(0)
from basilisk_env_amd._lib import GRAV_PM_J2
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
cfg = default_config(4, GRAV_PM_J2)
p = BatchedPropagator(cfg, n); p.reset(sample_ic_batch(n, 4, seed=seed)); p.set_halves_form(True)
act = np.zeros(n, np.int32)
quiet, tick = [], []
for t in range(launches):
    p.step(act, 1); p.sync()
    if t < 20:
        continue                                                    # (clock ramp, code object load)
    w = p.debug_words()
    lo, hi = (w & np.uint64(0xFFFFFFFF)).astype(np.float64), (w >> np.uint64(32)).astype(np.float64)
    # with nav_lag the FSW chain runs at the head of the launch that starts at phase fsw_every - 1; launch t starts at tick t
    (tick if t % cfg.fsw_every == cfg.fsw_every - 1 else quiet if t % cfg.fsw_every not in (0, cfg.fsw_every - 1) else []).append((lo, hi))
if role == 1:
    print("%s  n %d, %d launches, seed %d" % (p.kernel_info()["name"], n, launches, seed))
for what, rows in (("no FSW tick", quiet), ("FSW tick   ", tick)):
    for k in (0, 1):
        v = np.concatenate([r[k] for r in rows])
        print("  %s %s  %-24s mean %7.0f  median %7.0f  5 %% %7.0f  95 %% %7.0f cycles   (%d words)" %
              (names[role - 1], what, fields[role - 1][k], v.mean(), np.median(v), np.quantile(v, 0.05), np.quantile(v, 0.95), v.size))
p.close()
