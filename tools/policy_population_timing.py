#!/usr/bin/env python3
"""A population of policies scored from the envs' current states, two ways, in the same run: Engine.evaluate_policies
(emei_evaluate_policies: one lane per (policy, env) pair, ONE launch, nothing written per step) against the loop it replaces on the API
as it was before the call existed — per member `set_state(start)`, `rollout_policy(H, member, auto_reset=False)` with its [H, N]
outputs, and the torch reduction of rewards and done codes to (return, length).  The loop is the comparator; the one call is never its
own yardstick.  Both score the same pairs from the same start (`lengths_equal` and `returns_max_rel_diff` in the output: the loop's
sum is a torch reduction, another summation order than the kernel's running sum, so the returns agree to float64 rounding, not
bit for bit; the bit-for-bit comparison is tests/test_gpu_policy_population.py's).
Method: the horizon of a shape starts at --horizon and is doubled until one call of the fused route exceeds 12 ms (so that every timed
window is above 10 ms; a shape that reaches --max-horizon below that is marked "indicative"); then, after `--warmup` untimed runs of
each route, `--repeats` rounds; every round times ONE run of each route with device events around it (the loop's host overhead is
inside its window), the two routes alternating inside the round so that drift hits both alike.  Reported per shape: the median over
the rounds and the spread (min, max) of either route, and the ratio of the medians.
Shapes: CartPoleSwingUp N = 256 and HalfCheetahRunning N = 256, P = 64 members, hidden = 0 (affine) and 64, H = 128 to start from.
One JSON line per shape.  Run on the GPU box:
    python tools/policy_population_timing.py [--warmup 2] [--repeats 7] [--only INDEX]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emei_amd.engine import Engine  # noqa: E402
from emei_amd.policy import PolicyPopulation  # noqa: E402

CHEETAH = dict(freq_rate=4, real_time_scale=0.002, init_noise=0.1)
# (env, N, P, hidden, engine kwargs)
SHAPES = [
    ("CartPoleSwingUp", 256, 64, 0, {}),
    ("CartPoleSwingUp", 256, 64, 64, {}),
    ("HalfCheetahRunning", 256, 64, 0, CHEETAH),
    ("HalfCheetahRunning", 256, 64, 64, CHEETAH),
]
MIN_WINDOW_MS = 12.0


def make_population(eng, P, hidden):
    g = torch.Generator().manual_seed(1)
    n_out = max(eng.act_dim, 1)
    r = lambda *s: torch.randn(*s, generator=g) / s[-1] ** 0.5
    if hidden == 0:
        return PolicyPopulation(r(P, n_out, eng.obs_dim), r(P, n_out)).bind(eng)
    return PolicyPopulation(r(P, n_out, hidden), r(P, n_out), r(P, hidden, eng.obs_dim), r(P, hidden)).bind(eng)


def loop_route(eng, start, members, H, discount, outs):
    """what a user of the parent commit's API writes: P launches with per-step outputs, then the reduction in torch"""
    rets, lens = [], []
    weights = (discount ** torch.arange(H, device=eng.device, dtype=torch.float64))[:, None]
    steps = torch.arange(H, device=eng.device)[:, None]
    for member in members:
        eng.set_state(start)
        _, _, rew, done = eng.rollout_policy(H, member, auto_reset=False, out=outs)
        term = (done & 1) != 0
        length = torch.where(term.any(dim=0), term.to(torch.uint8).argmax(dim=0) + 1, H)
        counted = steps < length[None, :]
        rets.append((rew.to(torch.float64) * weights * counted).sum(dim=0))
        lens.append(length.to(torch.int32))
    return torch.stack(rets), torch.stack(lens)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--horizon", type=int, default=128)
    ap.add_argument("--max-horizon", type=int, default=8192)
    ap.add_argument("--only", type=int, default=None, help="index of the one shape to run")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("policy_population_timing.py needs a GPU")
    discount = 0.99
    for idx, (name, N, P, hidden, kw) in enumerate(SHAPES):
        if args.only is not None and args.only != idx:
            continue
        eng = Engine(name, N, **kw)
        eng.reset(seed=0)
        start = eng.get_state().clone()
        pop = make_population(eng, P, hidden)
        members = [pop[p] for p in range(P)]
        H = args.horizon

        def timed(fn):
            eng.set_state(start)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), out

        fused = lambda: eng.evaluate_policies(pop, H, discount=discount)
        timed(fused)  # code objects loaded
        while timed(fused)[0] < MIN_WINDOW_MS and 2 * H <= args.max_horizon:
            H *= 2
        outs = eng.alloc_outputs(H)
        loop = lambda: loop_route(eng, start, members, H, discount, outs)
        for _ in range(args.warmup):
            timed(fused), timed(loop)
        ms = {"fused": [], "loop": []}
        for _ in range(args.repeats):
            t, a = timed(fused)
            ms["fused"].append(t)
            t, b = timed(loop)
            ms["loop"].append(t)
        same_len = bool(torch.equal(a[1], b[1]))
        rel = float(((a[0] - b[0]).abs() / b[0].abs().clamp_min(1e-3)).max())
        # the loop's sum is a torch reduction (another summation order than the kernel's running sum): agreement to rounding
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({
            "env": name, "n_envs": N, "n_policies": P, "hidden": hidden, "horizon": H, "discount": discount, "repeats": args.repeats,
            "fused_ms": round(med["fused"], 4), "fused_ms_min_max": [round(min(ms["fused"]), 4), round(max(ms["fused"]), 4)],
            "loop_ms": round(med["loop"], 4), "loop_ms_min_max": [round(min(ms["loop"]), 4), round(max(ms["loop"]), 4)],
            "loop_over_fused": round(med["loop"] / med["fused"], 3),
            "fused_us_per_step": round(1e3 * med["fused"] / H, 3), "loop_us_per_step_per_member": round(1e3 * med["loop"] / H / P, 3),
            "indicative": bool(med["fused"] < 10.0), "lengths_equal": same_len, "returns_max_rel_diff": rel,
        }), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
