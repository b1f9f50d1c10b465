#!/usr/bin/env python3
"""One MPPI update of a nominal action sequence, two ways, in the same run: Engine.plan_mppi (emei_plan_mppi: candidates drawn in the
lanes that score them, every return kept, then redrawn and averaged under their weights — two launches, nothing of size H * N * K
stored) against the composition it replaces, built from the API that was there before it — sample_candidates (the same candidates,
written out), evaluate_sequences, then torch exp / sum and the weighted einsum over the float-converted candidates.  Engine.plan_shooting
alone is timed too: the difference to plan_mppi is the second pass and the 8 bytes per candidate.
Method: device events around `--reps` back-to-back calls after `--warmup` untimed ones, repeated `--repeats` times, the median
reported (and the spread); the composition's pieces are timed the same way on their own.
Workloads (tools/shooting_bench.py's, both with a nominal): CartPoleSwingUp N = 4096, K = 64, H = 100; HopperRunning (RK4,
freq_rate 4, dt 0.002) N = 1024, K = 16, H = 50, sigma 0.3.  One JSON line per workload.  Run on the GPU box:
    python tools/mppi_bench.py [--reps 20] [--warmup 3] [--repeats 5] [--only NAME]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emei_amd.engine import Engine  # noqa: E402

WORKLOADS = [
    ("CartPoleSwingUp", 4096, 64, 100, dict(freq_rate=1, real_time_scale=0.02), None),
    ("HopperRunning", 1024, 16, 50, dict(freq_rate=4, real_time_scale=0.002, integrator="rk4"), 0.3),
]
TEMPERATURE = 1.0


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
    ap.add_argument("--only", default=None, help="run the workload of this env alone")
    ap.add_argument("--fused-only", action="store_true", help="time Engine.plan_mppi alone (for a kernel trace of its two launches)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mppi_bench.py needs a GPU")
    for name, N, K, H, kw, sigma in WORKLOADS:
        if args.only and args.only != name:
            continue
        eng = Engine(name, N, **kw)
        eng.reset(seed=0)
        dev = eng.device
        if eng.act_dim == 0:
            nominal = torch.full((H, N), 0.5, device=dev)
        else:
            nominal = torch.zeros((H, N, eng.act_dim), device=dev)
        eq = "nk,hnk->hn" if eng.act_dim == 0 else "nk,hnka->hna"
        seed = [0]

        def fused():
            seed[0] += 1
            return eng.plan_mppi(H, K, seed[0], TEMPERATURE, discount=0.99, nominal=nominal, sigma=sigma)

        def shooting():
            seed[0] += 1
            return eng.plan_shooting(H, K, seed[0], discount=0.99, nominal=nominal, sigma=sigma)

        def draw():
            seed[0] += 1
            return eng.sample_candidates(H, K, seed[0], nominal=nominal, sigma=sigma)

        def weigh(cand, ret):
            w = torch.exp((ret - ret.max(1, keepdim=True).values) / TEMPERATURE)
            return (torch.einsum(eq, w, cand.to(torch.float64)) / w.sum(1)[(None, slice(None)) + (None,) * (cand.dim() - 3)]).float()

        def composed():
            cand = draw()
            ret, _ = eng.evaluate_sequences(cand, 0.99)
            return weigh(cand, ret)

        fused_ms = median_ms(fused, args)
        row = {"env": name, "N": N, "K": K, "H": H, "kw": kw, "sigma": sigma, "temperature": TEMPERATURE, "candidate_steps": N * K * H,
               "reps": args.reps, "repeats": args.repeats,
               "plan_mppi_ms": round(fused_ms[0], 4), "plan_mppi_min_max_ms": [round(fused_ms[1], 4), round(fused_ms[2], 4)]}
        if not args.fused_only:
            fixed = draw()
            fixed_ret, _ = eng.evaluate_sequences(fixed, 0.99)
            # the two ways compute the same update (the composition's soft-max has no NaN rule: the workloads give none)
            seed[0] = 0
            a = fused()[0]
            seed[0] = 0
            b = composed()
            row["max_abs_difference"] = float((a - b.view_as(a)).abs().max())
            shoot_ms = median_ms(shooting, args)
            comp_ms = median_ms(composed, args)
            draw_ms = median_ms(draw, args)
            eval_ms = median_ms(lambda: eng.evaluate_sequences(fixed, 0.99), args)
            weigh_ms = median_ms(lambda: weigh(fixed, fixed_ret), args)
            row.update({
                "plan_shooting_ms": round(shoot_ms[0], 4), "plan_shooting_min_max_ms": [round(shoot_ms[1], 4), round(shoot_ms[2], 4)],
                "composition_ms": round(comp_ms[0], 4), "composition_min_max_ms": [round(comp_ms[1], 4), round(comp_ms[2], 4)],
                "composition_over_plan_mppi": round(comp_ms[0] / fused_ms[0], 3),
                "plan_mppi_over_plan_shooting": round(fused_ms[0] / shoot_ms[0], 3),
                "sample_candidates_ms": round(draw_ms[0], 4), "evaluate_sequences_ms": round(eval_ms[0], 4),
                "exp_sum_einsum_ms": round(weigh_ms[0], 4),
            })
        print(json.dumps(row), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
