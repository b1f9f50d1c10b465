#!/usr/bin/env python3
"""One planning call of random-shooting MPC, two ways, in the same run: Engine.plan_shooting (emei_plan_shooting: candidates
drawn in the lanes, arg-maxed on the device, two launches) against the composition it replaces, built from the API that was there
before it — torch.randint / torch.rand for the [H, N, K(, act_dim)] candidates, evaluate_sequences, argmax, and the gather of each
env's first action.  Both plan N * K candidates of H steps from the same states (not the same candidates: the generators differ).
Method: device events around `--reps` back-to-back calls after `--warmup` untimed ones, repeated `--repeats` times, the median
reported (and the spread); the composition's pieces are timed the same way on their own.
Workloads (tools/plan_bench.py's): CartPoleSwingUp N = 4096, K = 64, H = 100; HopperRunning (RK4, freq_rate 4, dt 0.002)
N = 1024, K = 16, H = 50.  One JSON line per workload.  Run on the GPU box:
    python tools/shooting_bench.py [--reps 20] [--warmup 3] [--repeats 5]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emei_amd.engine import Engine  # noqa: E402

WORKLOADS = [
    ("CartPoleSwingUp", 4096, 64, 100, dict(freq_rate=1, real_time_scale=0.02)),
    ("HopperRunning", 1024, 16, 50, dict(freq_rate=4, real_time_scale=0.002, integrator="rk4")),
]


def timed(fn, reps, warmup):
    """seconds per call: device events around `reps` back-to-back calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / reps


def median_ms(fn, args):
    runs = [timed(fn, args.reps, args.warmup) * 1e3 for _ in range(args.repeats)]
    return statistics.median(runs), min(runs), max(runs)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shooting_bench.py needs a GPU")
    for name, N, K, H, kw in WORKLOADS:
        eng = Engine(name, N, **kw)
        eng.reset(seed=0)
        dev = eng.device
        rows = torch.arange(N, device=dev)
        seed = [0]

        def fused():
            seed[0] += 1
            return eng.plan_shooting(H, K, seed[0], discount=0.99)

        def draw():
            if eng.act_dim == 0:
                return torch.randint(0, 2, (H, N, K), device=dev, dtype=torch.uint8)
            return torch.rand((H, N, K, eng.act_dim), device=dev) * 2 - 1

        def composed():
            cand = draw()
            ret, _ = eng.evaluate_sequences(cand, 0.99)
            return cand[0, rows, ret.argmax(1)]

        fixed = draw()
        fixed_ret, _ = eng.evaluate_sequences(fixed, 0.99)
        fused_ms = median_ms(fused, args)
        comp_ms = median_ms(composed, args)
        draw_ms = median_ms(draw, args)
        eval_ms = median_ms(lambda: eng.evaluate_sequences(fixed, 0.99), args)
        pick_ms = median_ms(lambda: fixed[0, rows, fixed_ret.argmax(1)], args)
        cs = N * K * H
        print(json.dumps({
            "env": name, "N": N, "K": K, "H": H, "kw": kw, "candidate_steps": cs, "reps": args.reps, "repeats": args.repeats,
            "plan_shooting_ms": round(fused_ms[0], 4), "plan_shooting_min_max_ms": [round(fused_ms[1], 4), round(fused_ms[2], 4)],
            "composition_ms": round(comp_ms[0], 4), "composition_min_max_ms": [round(comp_ms[1], 4), round(comp_ms[2], 4)],
            "composition_over_plan_shooting": round(comp_ms[0] / fused_ms[0], 3),
            "draw_ms": round(draw_ms[0], 4), "evaluate_sequences_ms": round(eval_ms[0], 4), "argmax_gather_ms": round(pick_ms[0], 4),
            "plan_shooting_candidate_steps_per_s": float(f"{cs / (fused_ms[0] * 1e-3):.4g}"),
        }), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
