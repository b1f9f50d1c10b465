#!/usr/bin/env python3
"""Receding-horizon MPPI control episodes, two ways, in the same run: Engine.mpc_mppi (emei_mpc_mppi: one wave per env plans, acts,
steps, auto-resets and shifts for all T control steps in ONE launch) against the loop it replaces, built from the API that was there
before it — per control step a clamp, plan_mppi in place (two launches), a threshold, step (one launch), a roll and a refill
(README, "MPPI").  The loop is the comparator; the fused call is never its own yardstick.  Both start every timed episode from the
same state and nominal (restored outside the timed window) and compute the same bits (tests/test_gpu_mpc.py).
Method: after `--warmup` untimed episodes of each route (code objects loaded, workspaces allocated, clocks settled), `--repeats`
rounds; every round times ONE episode of each route with device events around it (the loop's host overhead is inside its window: the
events bracket everything its T iterations enqueue), the two routes alternating inside the round so that drift hits both alike.
Reported per shape: the median over the rounds and the spread (min, max) of either route, and the ratio of the medians.
Shapes: CartPoleSwingUp N = 256 and N = 65 536, ReboundInvertedPendulumSwingUp N = 256, ReboundInvertedDoublePendulumSwingUp (the
fused call on the body kernels' controllers, body_mpc_kernels.h) N = 256 and N = 16 384; K = 64, H = 30; T = 200 (20 at the large N;
the InvertedDoublePendulum 400 and 40, so that its MPPI windows exceed 10 ms).
--planner cem: the same comparison for Engine.mpc_cem (emei_mpc_cem) against the README's CEM loop — per control step a roll, a
refill, a fresh std, ITERATIONS = 3 times (a clamp of the mean on the discrete envs, plan_cem in place: two launches, a floor of the
std on the continuous ones), and a step — with N_ELITES = 8, at the same shapes (tests/test_gpu_mpc_cem.py: the same bits).
--planner policy: the same comparison for Engine.mpc_policy (emei_mpc_policy) against the README's policy-guided loop — per control
step a new PolicyNoise under the seed 1 + t * H, plan_policy (two launches) and a step — around an MLPPolicy with HIDDEN = 64 units,
act="mean" (tests/test_gpu_mpc_policy.py: the same bits); the nominal is unused.
One JSON line per shape.  Run on the GPU box:
    python tools/mpc_timing.py [--planner mppi|cem|policy] [--warmup 2] [--repeats 7] [--only INDEX]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emei_amd.engine import _CTRL_RANGE, Engine  # noqa: E402

# (env, N, K, H, T, sigma)
SHAPES = [
    ("CartPoleSwingUp", 256, 64, 30, 200, None),
    ("CartPoleSwingUp", 65536, 64, 30, 20, None),
    ("ReboundInvertedPendulumSwingUp", 256, 64, 30, 200, 0.5),
    # (T doubled against the shapes above: at T = 200 / 20 the fused MPPI episodes are 8.2 / 6.6 ms, short of a ~10 ms window)
    ("ReboundInvertedDoublePendulumSwingUp", 256, 64, 30, 400, 0.5),
    ("ReboundInvertedDoublePendulumSwingUp", 16384, 64, 30, 40, 0.5),
]
TEMPERATURE, DISCOUNT = 0.5, 0.99
ITERATIONS, N_ELITES, SIGMA_MIN = 3, 8, 0.05  # --planner cem
HIDDEN, NOISE_STD, EPSILON = 64, 0.2, 0.2  # --planner policy


def loop_episode(eng, T, H, K, seed, nominal, sigma, refill, lo, hi):
    """the README loop, statement for statement (at the Engine level: less host work per call than through the env classes, so the
    comparator is not handicapped): what a user ran before the fused call existed"""
    for t in range(T):
        nominal = torch.roll(nominal, -1, 0)
        nominal[-1] = refill
        nominal.clamp_(lo, hi)
        eng.plan_mppi(H, K, seed + t, TEMPERATURE, discount=DISCOUNT, nominal=nominal, sigma=sigma, out=nominal)
        eng.step((nominal[0] >= 0.5).long() if eng.act_dim == 0 else nominal[0], auto_reset=True)


def cem_loop_episode(eng, T, H, K, seed, nominal, sigma, refill, lo, hi):
    """the README's CEM loop at the Engine level; the discrete envs have no std and clamp the mean as the MPPI loop does"""
    for t in range(T):
        nominal = torch.roll(nominal, -1, 0)
        nominal[-1] = refill
        std = None if eng.act_dim == 0 else torch.full_like(nominal, sigma)
        for it in range(ITERATIONS):
            nominal.clamp_(lo, hi)
            eng.plan_cem(H, K, N_ELITES, seed + ITERATIONS * t + it, discount=DISCOUNT, nominal=nominal, sigma=std, out=nominal,
                         out_sigma=std)
            if std is not None:
                std.clamp_(min=SIGMA_MIN)
        eng.step((nominal[0] >= 0.5).long() if eng.act_dim == 0 else nominal[0], auto_reset=True)


def make_policy(eng):
    """an MLPPolicy with HIDDEN units and the noise constructor of the env's kind (--planner policy)"""
    from emei_amd.policy import MLPPolicy, PolicyNoise

    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g) * 1.5 / s[-1] ** 0.5
    n_out = max(eng.act_dim, 1)
    pol = MLPPolicy(r(n_out, HIDDEN), r(n_out), r(HIDDEN, eng.obs_dim), r(HIDDEN))
    kw = dict(epsilon=EPSILON) if eng.act_dim == 0 else dict(std=NOISE_STD)
    return pol, (lambda seed: PolicyNoise(seed, **kw))


def policy_loop_episode(eng, T, H, K, seed, pol, noise):
    """the README's policy-guided loop at the Engine level"""
    for t in range(T):
        mean = eng.plan_policy(H, K, pol, noise(seed + t * H), discount=DISCOUNT, temperature=TEMPERATURE)[3]
        eng.step((mean >= 0.5).long() if eng.act_dim == 0 else mean, auto_reset=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--planner", choices=("mppi", "cem", "policy"), default="mppi")
    ap.add_argument("--only", type=int, default=None, help="index of the one shape to run")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mpc_timing.py needs a GPU")
    for idx, (name, N, K, H, T, sigma) in enumerate(SHAPES):
        if args.only is not None and args.only != idx:
            continue
        eng = Engine(name, N)
        eng.reset(seed=0)
        state0 = eng.get_state().clone()
        refill = 0.5 if eng.act_dim == 0 else 0.0
        lo, hi = (0.05, 0.95) if eng.act_dim == 0 else _CTRL_RANGE.get(name, (-1.0, 1.0))  # Engine.mpc_*'s default clamp
        nominal = torch.empty((H, N), dtype=torch.float32, device=eng.device)
        outs = eng.alloc_outputs(T)

        def restore():
            eng.reset(seed=0)
            eng.set_state(state0)
            nominal.fill_(refill)
            torch.cuda.synchronize()

        pol, noise = make_policy(eng) if args.planner == "policy" else (None, None)

        def fused():
            if args.planner == "policy":
                eng.mpc_policy(T, H, K, pol, noise(1), act="mean", temperature=TEMPERATURE, discount=DISCOUNT, auto_reset=True, out=outs)
            elif args.planner == "cem":
                eng.mpc_cem(T, H, K, N_ELITES, 1, nominal, iterations=ITERATIONS, sigma=sigma, sigma_min=SIGMA_MIN, discount=DISCOUNT,
                            refill=refill, clamp=(lo, hi), auto_reset=True, out=outs)
            else:
                eng.mpc_mppi(T, H, K, 1, TEMPERATURE, nominal, discount=DISCOUNT, sigma=sigma, refill=refill, clamp=(lo, hi),
                             auto_reset=True, out=outs)

        def loop():
            if args.planner == "policy":
                return policy_loop_episode(eng, T, H, K, 1, pol, noise)
            (cem_loop_episode if args.planner == "cem" else loop_episode)(eng, T, H, K, 1, nominal, sigma, refill, lo, hi)

        def timed(fn):
            restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(args.warmup):
            timed(fused), timed(loop)
        ms = {"fused": [], "loop": []}
        for _ in range(args.repeats):
            ms["fused"].append(timed(fused))
            ms["loop"].append(timed(loop))
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({
            "planner": args.planner, "env": name, "n_envs": N, "n_candidates": K, "horizon": H, "n_steps": T, "repeats": args.repeats,
            "fused_ms": round(med["fused"], 4), "fused_ms_min_max": [round(min(ms["fused"]), 4), round(max(ms["fused"]), 4)],
            "loop_ms": round(med["loop"], 4), "loop_ms_min_max": [round(min(ms["loop"]), 4), round(max(ms["loop"]), 4)],
            "loop_over_fused": round(med["loop"] / med["fused"], 3),
            "fused_us_per_control_step": round(1e3 * med["fused"] / T, 3), "loop_us_per_control_step": round(1e3 * med["loop"] / T, 3),
        }), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
