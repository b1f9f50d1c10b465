#!/usr/bin/env python3
"""MPPI with a terminal value, three ways, in the same run: Engine.plan_mppi(value=) (emei_plan_mppi_value: one lane per (env,
candidate) on one-wave blocks, the critic evaluated once per candidate in the lane after the loop, two launches) against
  composed: what the API offered before the call existed — sample_candidates materialises the [H, N, K] actions,
            evaluate_sequences(final_obs=True) scores them, the same critic is evaluated on the final rows as a user would, three
            float32 torch matmuls, discount^H * V is added where length == H (the composition cannot tell a candidate that terminated
            at its last step from one that never did), and the soft-max mean over the candidates is taken in torch;
  plain:    plan_mppi without a value, on the 256-thread plan kernel, for what the value costs.
The composition is the comparator; the one call is never its own yardstick.  The two do not compute the same thing bit for bit (float32
matmuls, the last-step rule), so only the shapes of the results are compared here; tests/test_gpu_plan_value.py holds the call to its
twin.
Method (tools/policy_plan_timing.py's): the horizon of a shape starts at --horizon and is doubled until one plan_mppi(value=) exceeds
12 ms (so that every timed window is above 10 ms), but no further than nine in ten candidates still run all H steps: a wave of a plan
kernel leaves its loop with its last live lane and a candidate that terminated takes no value, so a horizon that outlives the
candidates (CartPoleSwingUp's fair coins lose the cart after 100 to 200 steps) would time neither the steps nor the critic.  A shape
that stops below 10 ms, there or at --max-horizon, is marked "indicative".  Then, after
`--warmup` untimed runs of each route, `--repeats` rounds; every round times ONE run of each route with device events around it, the
routes alternating inside the round so that drift hits all alike.  Reported per shape: the median over the rounds and the spread
(min, max) of every route, and the ratios of the medians.  full_length_share is the share of candidates that ran all H steps.
Shapes: CartPoleSwingUp (fair coins) and HalfCheetahRunning (uniform draws), N = 256, K = 64, critic widths 64-64 and 256-256.
One JSON line per (shape, widths), one GPU process.  Run on the GPU box:
    python tools/plan_value_timing.py [--warmup 2] [--repeats 7] [--only INDEX] [--widths H1,H2]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emei_amd.engine import Engine  # noqa: E402
from emei_amd.policy import DeepValueFunction  # noqa: E402

CHEETAH = dict(freq_rate=4, real_time_scale=0.002, init_noise=0.1)
# (env, N, K, engine kwargs)
SHAPES = [
    ("CartPoleSwingUp", 256, 64, {}),
    ("HalfCheetahRunning", 256, 64, CHEETAH),
]
WIDTHS = [(64, 64), (256, 256)]
MIN_WINDOW_MS = 12.0
MIN_FULL_SHARE = 0.9  # of the candidates run all H steps, or the horizon is not doubled again


def make_value(eng, h1, h2):
    g = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=g) / s[-1] ** 0.5
    return DeepValueFunction(r(1, h2), r(1), r(h2, h1), r(h2), r(h1, eng.obs_dim), r(h1)).bind(eng)


def composed_route(eng, value, start, N, K, H, seed, temperature, discount):
    """what a user of the parent commit's API writes: the candidates in memory, their scores, the critic and the soft-max mean in torch"""
    cand = eng.sample_candidates(H, K, seed)
    ret, length, fobs = eng.evaluate_sequences(cand, discount=discount, start_state=start, final_obs=True)
    x = fobs.view(N * K, -1)
    h = torch.relu(x @ value.w1.T + value.b1)
    h = torch.relu(h @ value.w2.T + value.b2)
    v = (h @ value.w3.T + value.b3)[:, 0].view(N, K)
    ret = torch.where(length < H, ret, ret + discount ** H * v.to(torch.float64))
    best = ret.max(dim=1)
    w = torch.softmax((ret - best.values[:, None]) / temperature, dim=1)  # [N, K]
    c = cand.to(torch.float64)
    w = w[None, :, :] if c.dim() == 3 else w[None, :, :, None]
    mean = (c * w).sum(dim=2).to(torch.float32)
    return mean, best.values, best.indices.to(torch.int32), (length == H).to(torch.float32).mean()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--max-horizon", type=int, default=4096)
    ap.add_argument("--only", type=int, default=None, help="index of the one shape to run")
    ap.add_argument("--widths", default=None, metavar="H1,H2", help="the one pair of critic widths to run")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plan_value_timing.py needs a GPU")
    widths = WIDTHS
    if args.widths:
        widths = [tuple(int(v) for v in args.widths.split(","))]
        if len(widths[0]) != 2:
            raise SystemExit("--widths takes H1,H2")
    discount, temperature, seed = 0.99, 1.0, 7
    for idx, (name, N, K, kw) in enumerate(SHAPES):
        if args.only is not None and args.only != idx:
            continue
        for h1, h2 in widths:
            eng = Engine(name, N, **kw)
            eng.reset(seed=0)
            start = eng.get_state().clone()
            value = make_value(eng, h1, h2)
            H = args.horizon

            def timed(fn):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1), out

            fused = lambda: eng.plan_mppi(H, K, seed, temperature, discount=discount, start_state=start, value=value)
            plain = lambda: eng.plan_mppi(H, K, seed, temperature, discount=discount, start_state=start)
            composed = lambda: composed_route(eng, value, start, N, K, H, seed, temperature, discount)

            def full_share(h):
                cand = eng.sample_candidates(h, K, seed)
                return float((eng.evaluate_sequences(cand, discount=discount, start_state=start)[1] == h).to(torch.float32).mean())

            timed(fused)  # code objects loaded
            while timed(fused)[0] < MIN_WINDOW_MS and 2 * H <= args.max_horizon and full_share(2 * H) >= MIN_FULL_SHARE:
                H *= 2
            for _ in range(args.warmup):
                timed(fused), timed(composed), timed(plain)
            ms = {"value": [], "composed": [], "plain": []}
            for _ in range(args.repeats):
                t, a = timed(fused)
                ms["value"].append(t)
                t, b = timed(composed)
                ms["composed"].append(t)
                ms["plain"].append(timed(plain)[0])
            same_shapes = all(x.shape == y.shape and x.dtype == y.dtype for x, y in zip(a[:3], b[:3]))
            med = {k: statistics.median(v) for k, v in ms.items()}
            span = lambda k: [round(min(ms[k]), 4), round(max(ms[k]), 4)]
            print(json.dumps({
                "env": name, "n_envs": N, "n_candidates": K, "widths": [h1, h2], "horizon": H, "discount": discount, "repeats": args.repeats,
                "value_ms": round(med["value"], 4), "value_ms_min_max": span("value"),
                "composed_ms": round(med["composed"], 4), "composed_ms_min_max": span("composed"),
                "plain_ms": round(med["plain"], 4), "plain_ms_min_max": span("plain"),
                "composed_over_value": round(med["composed"] / med["value"], 3), "value_over_plain": round(med["value"] / med["plain"], 3),
                "value_minus_plain_ms": round(med["value"] - med["plain"], 4),
                "indicative": bool(med["value"] < 10.0), "same_shapes": same_shapes, "full_length_share": round(float(b[3]), 4),
            }), flush=True)
            eng.close()


if __name__ == "__main__":
    main()
