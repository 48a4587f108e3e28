#!/usr/bin/env python3
"""What a physics table costs: in ONE process on one MI355X, HIP-event-timed chains of dependent launches of
fpv_step - the headline kernel, the Kahan kernel (181 B), a table handle (177 B) - and fpv_step_n at k = 16 with and without a
table, interleaved over several rounds, at 2^20 and 2^23 drones.  Prints one markdown table per population.

    python tools/physics_table_cost.py [--n 1048576 8388608] [--launches 1000] [--rounds 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d prof_phys -- python tools/physics_table_cost.py --launches 200 --rounds 2

The table is randomised (mass, motor strength, drag, lags within +-20 %), the sticks are a ring of EMA-noise rows.
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from fpyv_amd import load_params, sticks  # noqa: E402
from fpyv_amd.env import DroneBatch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="*", default=[1 << 20, 1 << 23])
ap.add_argument("--launches", type=int, default=1000)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda:0")
p = load_params(fps=1000, ceiling=100.0)
R = dict(mass=(0.8, 1.2), thrust=(0.8, 1.2), drag=(0.8, 1.2), rates_lag=(0.8, 1.2), thrust_lag=(0.8, 1.2))
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for n in a.n:
    ring = 32 if n <= (1 << 21) else 4
    acts = sticks.ema_noise_device(ring, n, dev)
    kw = dict(device=dev, auto_reset=True, with_accel=False)
    legs = {"fpv_step, headline kernel (133 B)": (DroneBatch(p, n, **kw), 133, False),
            "fpv_step, Kahan rows (181 B)": (DroneBatch(p, n, kahan_position=True, **kw), 181, False),
            "fpv_step, physics table (177 B)": (DroneBatch(p, n, per_drone_physics=True, **kw), 177, False),
            "fpv_step_n k = 16, no table": (DroneBatch(p, n, **kw), None, True),
            "fpv_step_n k = 16, physics table": (DroneBatch(p, n, per_drone_physics=True, **kw), None, True)}
    for name, (b, _, _) in legs.items():
        if b.physics is not None:
            b.randomize_physics(5, **R)
    res = {k: [] for k in legs}
    for r in range(a.rounds + 1):
        for name, (b, nbytes, fused) in legs.items():
            b.reset()
            reps = max(1, a.launches // ring) if not fused else max(1, a.launches // 16 // 4)
            k16 = acts[:16] if ring >= 16 else acts.repeat(4, 1, 1)
            (b.rollout(k16) if fused else b.rollout(acts, fused=False))
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                if fused:
                    b.rollout(k16)
                else:
                    b.rollout(acts, fused=False)
            e1.record()
            torch.cuda.synchronize()
            steps = reps * (16 if fused else ring)
            if r:
                res[name].append(e0.elapsed_time(e1) * 1e3 / steps)
    print(f"\n## {n} drones (chains of {a.launches} dependent launches, {a.rounds} rounds interleaved, median; us per env-step)\n")
    print("| path | us / step | min | GB/s on its own bytes | of 8 TB/s |")
    print("|---|---:|---:|---:|---:|")
    for name, (b, nbytes, fused) in legs.items():
        med = statistics.median(res[name])
        bw = f"{nbytes * n / med / 1e3:.0f} | {nbytes * n / med / 1e3 / 8000:.1%}" if nbytes else "- | -"
        print(f"| {name} | {med:.2f} | {min(res[name]):.2f} | {bw} |", flush=True)
    del legs
    torch.cuda.empty_cache()
