#!/usr/bin/env python3
"""One cross-entropy-method iteration, two ways, in the same run: Engine.plan_cem (emei_plan_cem: candidates drawn in the lanes that
score them, every return kept, the n_elites best per env selected on the device, redrawn and their mean / standard deviation taken —
two launches, nothing of size H * N * K stored) against the composition it replaces, built from the API that was there before it —
sample_candidates (the same candidates, written out), evaluate_sequences, torch.topk over the returns, a gather of the elites'
sequences and mean / std over them.  Engine.plan_mppi is timed at the same shape too: the difference to plan_cem is what the
selection costs over MPPI's finish pass (and what redrawing n_elites instead of all K candidates saves).
Method (tools/mppi_bench.py's): device events around `--reps` back-to-back calls after `--warmup` untimed ones, repeated `--repeats`
times, the median reported (and the spread); the composition's pieces are timed the same way on their own.
Workloads (tools/mppi_bench.py's, both with a nominal), n_elites = K / 8: CartPoleSwingUp N = 4096, K = 64, H = 100; HopperRunning
(RK4, freq_rate 4, dt 0.002) N = 1024, K = 16, H = 50, sigma 0.3.  One JSON line per workload.  Run on the GPU box:
    python tools/cem_bench.py [--reps 20] [--warmup 3] [--repeats 5] [--only NAME]"""
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
TEMPERATURE = 1.0  # of the plan_mppi call timed for comparison


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
    ap.add_argument("--fused-only", action="store_true", help="time Engine.plan_cem alone (for a kernel trace of its two launches)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cem_bench.py needs a GPU")
    for name, N, K, H, kw, sigma in WORKLOADS:
        if args.only and args.only != name:
            continue
        M = K // 8
        eng = Engine(name, N, **kw)
        eng.reset(seed=0)
        dev = eng.device
        if eng.act_dim == 0:
            nominal = torch.full((H, N), 0.5, device=dev)
        else:
            nominal = torch.zeros((H, N, eng.act_dim), device=dev)
        seed = [0]

        def fused():
            seed[0] += 1
            return eng.plan_cem(H, K, M, seed[0], discount=0.99, nominal=nominal, sigma=sigma)

        def mppi():
            seed[0] += 1
            return eng.plan_mppi(H, K, seed[0], TEMPERATURE, discount=0.99, nominal=nominal, sigma=sigma)

        def draw():
            seed[0] += 1
            return eng.sample_candidates(H, K, seed[0], nominal=nominal, sigma=sigma)

        def select(ret):
            return torch.topk(ret, M, dim=1).indices  # [N, M]

        def gather(cand, idx):
            ix = idx[(None, slice(None), slice(None)) + (None,) * (cand.dim() - 3)].expand((H, N, M) + tuple(cand.shape[3:]))
            return torch.gather(cand, 2, ix)

        def moments(elite):
            e = elite.to(torch.float64)
            return e.mean(2).float(), e.std(2, unbiased=False).float()

        def composed():
            cand = draw()
            ret, _ = eng.evaluate_sequences(cand, 0.99)
            return moments(gather(cand, select(ret)))

        fused_ms = median_ms(fused, args)
        row = {"env": name, "N": N, "K": K, "n_elites": M, "H": H, "kw": kw, "sigma": sigma, "candidate_steps": N * K * H,
               "reps": args.reps, "repeats": args.repeats,
               "plan_cem_ms": round(fused_ms[0], 4), "plan_cem_min_max_ms": [round(fused_ms[1], 4), round(fused_ms[2], 4)]}
        if not args.fused_only:
            fixed = draw()
            fixed_ret, _ = eng.evaluate_sequences(fixed, 0.99)
            fixed_idx = select(fixed_ret)
            fixed_elite = gather(fixed, fixed_idx)
            # the two ways compute the same update (topk has neither the NaN rule nor the tie rule: the workloads' returns need none)
            seed[0] = 0
            a = fused()
            seed[0] = 0
            b = composed()
            row["max_abs_difference_mean"] = float((a[0] - b[0].view_as(a[0])).abs().max())
            if a[1] is not None:
                row["max_abs_difference_std"] = float((a[1] - b[1].view_as(a[1])).abs().max())
            mppi_ms = median_ms(mppi, args)
            comp_ms = median_ms(composed, args)
            draw_ms = median_ms(draw, args)
            eval_ms = median_ms(lambda: eng.evaluate_sequences(fixed, 0.99), args)
            topk_ms = median_ms(lambda: select(fixed_ret), args)
            gather_ms = median_ms(lambda: gather(fixed, fixed_idx), args)
            mom_ms = median_ms(lambda: moments(fixed_elite), args)
            row.update({
                "plan_mppi_ms": round(mppi_ms[0], 4), "plan_mppi_min_max_ms": [round(mppi_ms[1], 4), round(mppi_ms[2], 4)],
                "composition_ms": round(comp_ms[0], 4), "composition_min_max_ms": [round(comp_ms[1], 4), round(comp_ms[2], 4)],
                "composition_over_plan_cem": round(comp_ms[0] / fused_ms[0], 3),
                "plan_cem_over_plan_mppi": round(fused_ms[0] / mppi_ms[0], 3),
                "sample_candidates_ms": round(draw_ms[0], 4), "evaluate_sequences_ms": round(eval_ms[0], 4),
                "topk_ms": round(topk_ms[0], 4), "gather_ms": round(gather_ms[0], 4), "mean_std_ms": round(mom_ms[0], 4),
            })
        print(json.dumps(row), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
