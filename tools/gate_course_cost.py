#!/usr/bin/env python3
"""What a gate course costs: in ONE process on one MI355X, HIP-event-timed chains of dependent launches of fpv_step -
the headline kernel (133 B), a gate handle without (141 B) and with the observation rows (165 B) - and fpv_step_n at k = 16 with
and without a course, interleaved over several rounds, at 2^20 and 2^23 drones.  Prints one markdown table per population, next to
what the plain-order fit 4.03 us + bytes / 7.53 TB/s predicts for the single-step paths.

    python tools/gate_course_cost.py [--n 1048576 8388608] [--launches 1000] [--rounds 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d prof_gate -- python tools/gate_course_cost.py --launches 200 --rounds 2

The course is a round track of 12 gates; every drone starts at a random gate of it (the lanes of a wave read different descriptor
rows), the sticks are a ring of EMA-noise rows.
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from fpyv_amd import gates as G  # noqa: E402
from fpyv_amd import load_params, sticks  # noqa: E402
from fpyv_amd.env import DroneBatch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="*", default=[1 << 20, 1 << 23])
ap.add_argument("--launches", type=int, default=1000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--gates", type=int, default=12)
a = ap.parse_args()
dev = torch.device("cuda:0")
p = load_params(fps=1000, ceiling=100.0)
track = G.circular_track(a.gates, 8.0, 3.0, height=float(p.init_position[2]))
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for n in a.n:
    ring = 32 if n <= (1 << 21) else 4
    acts = sticks.ema_noise_device(ring, n, dev)
    start = torch.randint(0, a.gates, (n,), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    kw = dict(device=dev, auto_reset=True, with_accel=False)
    gk = dict(gates=track, gate_start=start, **kw)
    legs = {"fpv_step, headline kernel (133 B)": (DroneBatch(p, n, **kw), 133, False),
            "fpv_step, gate course without obs rows (141 B)": (DroneBatch(p, n, gate_obs=False, **gk), 141, False),
            "fpv_step, gate course with obs rows (165 B)": (DroneBatch(p, n, **gk), 165, False),
            "fpv_step_n k = 16, no course": (DroneBatch(p, n, **kw), None, True),
            "fpv_step_n k = 16, gate course with obs rows": (DroneBatch(p, n, **gk), None, True)}
    assert legs["fpv_step, gate course with obs rows (165 B)"][0].algorithmic_bytes() == 165
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
    print("| path | us / step | min | GB/s on its own bytes | of 8 TB/s | plain-order fit 4.03 us + bytes / 7.53 TB/s |")
    print("|---|---:|---:|---:|---:|---:|")
    for name, (b, nbytes, fused) in legs.items():
        med = statistics.median(res[name])
        bw = f"{nbytes * n / med / 1e3:.0f} | {nbytes * n / med / 1e3 / 8000:.1%} | {4.03 + nbytes * n / 7.53e6:.2f}" if nbytes else "- | - | -"
        print(f"| {name} | {med:.2f} | {min(res[name]):.2f} | {bw} |", flush=True)
    del legs
    torch.cuda.empty_cache()
