#!/usr/bin/env python3
"""Candidate-steps/s of emei_evaluate_sequences (Engine.evaluate_sequences) against the composition it replaces: a handle of
N * K envs, set_state of the start states tiled K times, one rollout of H steps (all three outputs, [H, N * K, obs_dim]
observations included, into preallocated buffers).  Both are timed over the same N * K * H candidate-steps, with device events
around `--reps` back-to-back calls after `--warmup` untimed ones.  The composition is also timed without its set_state (whose
host synchronisation is part of what it costs); that line starts each rollout where the previous one ended, so its work is not
the same where the cost of a step depends on the state (the Hopper's contacts).  The NumPy reduction a caller of the
composition still has to run is not counted.
Workloads: CartPoleSwingUp N = 4096, K = 64, H = 100; HopperRunning (RK4, freq_rate 4, dt 0.002: the env's
defaults) N = 1024, K = 16, H = 50.  One JSON line per workload.  Run on the GPU box:
    python tools/plan_bench.py [--reps 20] [--warmup 3]"""
import argparse
import json
import os
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plan_bench.py needs a GPU")
    for name, N, K, H, kw in WORKLOADS:
        eng = Engine(name, N, **kw)
        eng.reset(seed=0)
        g = torch.Generator(device=eng.device).manual_seed(0)
        if eng.act_dim == 0:
            acts = torch.randint(0, 2, (H, N, K), generator=g, device=eng.device, dtype=torch.uint8)
        else:
            acts = torch.rand((H, N, K, eng.act_dim), generator=g, device=eng.device) * 2 - 1
        plan_s = timed(lambda: eng.evaluate_sequences(acts, 0.99), args.reps, args.warmup)
        _, length = eng.evaluate_sequences(acts, 0.99)
        mean_len = float(length.double().mean())

        big = Engine(name, N * K, **kw)
        tiled = eng.get_state().repeat_interleave(K, dim=0).contiguous()
        flat = acts.view((H, N * K) + tuple(acts.shape[3:]))
        out = big.alloc_outputs(H)

        def compose():
            big.set_state(tiled)
            big.rollout(flat, out=out)

        comp_s = timed(compose, args.reps, args.warmup)
        roll_s = timed(lambda: big.rollout(flat, out=out), args.reps, args.warmup)
        cs = N * K * H
        print(json.dumps({
            "env": name, "N": N, "K": K, "H": H, "kw": kw, "candidate_steps": cs, "mean_length": round(mean_len, 2),
            "plan_ms": round(plan_s * 1e3, 4), "plan_candidate_steps_per_s": float(f"{cs / plan_s:.4g}"),
            "compose_ms": round(comp_s * 1e3, 4), "compose_candidate_steps_per_s": float(f"{cs / comp_s:.4g}"),
            "rollout_only_ms": round(roll_s * 1e3, 4), "rollout_only_candidate_steps_per_s": float(f"{cs / roll_s:.4g}"),
            "speedup_vs_compose": round(comp_s / plan_s, 2), "speedup_vs_rollout_only": round(roll_s / plan_s, 2),
        }), flush=True)
        big.close()
        eng.close()


if __name__ == "__main__":
    main()
