#!/usr/bin/env python3
"""Closed-loop policy rollouts, two ways, in the same run: Engine.rollout_policy (emei_rollout_policy: the policy is evaluated per lane
inside the rollout kernel, T steps with auto-reset in ONE launch) against the loop it replaces, the per-step route of
datasets.collect(policy=callable) — per step the callable (the SAME MLPPolicy object, evaluated in torch float64), one emei_step
launch, the host round trip `bool(done.any())` and, when an env finished, an episode_init_obs launch.  The loop is the comparator; the
fused call is never its own yardstick.  Both start every timed episode from the same state (restored outside the timed window) and
compute the same bits (tests/test_gpu_policy.py).
Method: the step count of a shape is doubled from its starting value until one fused episode exceeds 12 ms (so that every timed
window is above 10 ms); then, after `--warmup` untimed episodes of each route, `--repeats` rounds; every round times ONE episode of
each route with device events around it (the loop's host overhead is inside its window: the events bracket everything its T
iterations enqueue), the two routes alternating inside the round so that drift hits both alike.  Reported per shape: the median over
the rounds and the spread (min, max) of either route, and the ratio of the medians.
A third figure per shape, `replay_ms`: emei_rollout on the actions the fused call took, from the same start (the same trajectory, the
actions loaded instead of computed; at aligned shapes on the staged kernels) — what the in-kernel policy costs on top of the env step.
Shapes: CartPoleSwingUp N = 256 and N = 65 536, HalfCheetahRunning N = 256 and N = 16 384; one hidden layer of 64 units.
--noise: the exploration noise of emei_rollout_policy_noisy in the same method — per shape the fused NOISY launch (Gaussian std 0.1
on the continuous envs, epsilon 0.1 on the discrete ones: PolicyNoise), the fused deterministic launch and the per-step loop with the
same policy and noise objects (policy(obs, noise, t): one sample_candidates launch more per step), alternating inside every round;
the step count is sized on the noisy launch.  Reported: noisy_ms, fused_ms, loop_ms and the two ratios.
--deep H1,H2: the two-hidden-layer network of emei_rollout_policy_deep in the same method — per shape the fused DEEP launch (a
DeepMLPPolicy of widths H1, H2), the per-step loop with that same object as the callable, and the fused ONE-LAYER launch at
hidden = H1 (what the second layer adds), alternating inside every round; the step count is sized on the deep launch, starting from an
eighth of the shape's usual start (the loop of a wide net enqueues some thousand launches per step).  Reported: deep_ms, loop_ms,
one_layer_ms and the two ratios.
One JSON line per shape.  Run on the GPU box:
    python tools/policy_timing.py [--warmup 2] [--repeats 7] [--only INDEX] [--noise | --deep H1,H2]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emei_amd.engine import Engine  # noqa: E402
from emei_amd.policy import DeepMLPPolicy, MLPPolicy, PolicyNoise  # noqa: E402

# (env, N, starting T, engine kwargs)
SHAPES = [
    ("CartPoleSwingUp", 256, 1024, {}),
    ("CartPoleSwingUp", 65536, 256, {}),
    ("HalfCheetahRunning", 256, 128, dict(freq_rate=4, real_time_scale=0.002, max_episode_steps=1000, init_noise=0.1)),
    ("HalfCheetahRunning", 16384, 128, dict(freq_rate=4, real_time_scale=0.002, max_episode_steps=1000, init_noise=0.1)),
]
HIDDEN, MIN_WINDOW_MS, MAX_T = 64, 12.0, 8192


def make_policy(eng):
    g = torch.Generator().manual_seed(1)
    n_out = max(eng.act_dim, 1)
    r = lambda *s: torch.randn(*s, generator=g) / s[-1] ** 0.5
    return MLPPolicy(r(n_out, HIDDEN), r(n_out), r(HIDDEN, eng.obs_dim), r(HIDDEN)).bind(eng)


def loop_episode(eng, T, policy, outs, noise=None):
    """datasets.collect's per-step route, statement for statement, at the Engine level (noise: the callable draws step t's noise)"""
    next_obs, rew, done = outs
    cur = eng.get_obs().float()
    _, epi = eng.get_counters()
    for t in range(T):
        a = policy(cur) if noise is None else policy(cur, noise, t)
        a = (a.to(torch.float32) if eng.act_dim else a.to(torch.int64)).contiguous()
        eng.step(a, auto_reset=True, out=(next_obs[t], rew[t], done[t]))
        cur = next_obs[t]
        d = done[t] != 0
        if bool(d.any()):
            epi = epi + d.to(torch.int64)
            idx = torch.nonzero(d).reshape(-1)
            cur = cur.clone()
            cur[idx] = eng.episode_init_obs(idx, epi[idx])


def noisy_shape(args, eng, name, N, T, policy, timed):
    """--noise: one shape, the three routes alternating inside every round"""
    noise = (PolicyNoise(7, epsilon=0.1) if eng.act_dim == 0 else PolicyNoise(7, std=0.1)).bind(eng)
    box = {"outs": eng.alloc_outputs(T), "T": T}
    routes = {
        "noisy": lambda: eng.rollout_policy(box["T"], policy, auto_reset=True, out=box["outs"], noise=noise),
        "fused": lambda: eng.rollout_policy(box["T"], policy, auto_reset=True, out=box["outs"]),
        "loop": lambda: loop_episode(eng, box["T"], policy, box["outs"], noise),
    }
    timed(routes["noisy"])  # code objects loaded
    while timed(routes["noisy"]) < MIN_WINDOW_MS and 2 * box["T"] <= MAX_T:
        box["T"] *= 2
        box["outs"] = eng.alloc_outputs(box["T"])
    kernel = eng.last_kernel()
    for _ in range(args.warmup):
        for fn in routes.values():
            timed(fn)
    ms = {k: [] for k in routes}
    for _ in range(args.repeats):
        for k, fn in routes.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    row = {"env": name, "n_envs": N, "hidden": HIDDEN, "n_steps": box["T"], "repeats": args.repeats, "noise": "eps 0.1" if eng.act_dim == 0 else "std 0.1"}
    for k in routes:
        row[k + "_ms"] = round(med[k], 4)
        row[k + "_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
    row.update(noisy_over_fused=round(med["noisy"] / med["fused"], 3), loop_over_noisy=round(med["loop"] / med["noisy"], 3),
               noisy_us_per_step=round(1e3 * med["noisy"] / box["T"], 3), kernel=kernel)
    print(json.dumps(row), flush=True)


def deep_shape(args, eng, name, N, T, timed):
    """--deep: one shape, the three routes alternating inside every round"""
    h1, h2 = args.deep
    g = torch.Generator().manual_seed(1)
    n_out = max(eng.act_dim, 1)
    r = lambda *s: torch.randn(*s, generator=g) / s[-1] ** 0.5
    deep = DeepMLPPolicy(r(n_out, h2), r(n_out), r(h2, h1), r(h2), r(h1, eng.obs_dim), r(h1)).bind(eng)
    one = MLPPolicy(r(n_out, h1), r(n_out), r(h1, eng.obs_dim), r(h1)).bind(eng)
    box = {"T": max(T // 8, 8)}
    box["outs"] = eng.alloc_outputs(box["T"])
    routes = {
        "deep": lambda: eng.rollout_policy(box["T"], deep, auto_reset=True, out=box["outs"]),
        "loop": lambda: loop_episode(eng, box["T"], deep, box["outs"]),
        "one_layer": lambda: eng.rollout_policy(box["T"], one, auto_reset=True, out=box["outs"]),
    }
    timed(routes["deep"])  # code objects loaded
    while timed(routes["deep"]) < MIN_WINDOW_MS and 2 * box["T"] <= MAX_T:
        box["T"] *= 2
        box["outs"] = eng.alloc_outputs(box["T"])
    kernel = eng.last_kernel()
    for _ in range(args.warmup):
        for fn in routes.values():
            timed(fn)
    ms = {k: [] for k in routes}
    for _ in range(args.repeats):
        for k, fn in routes.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    row = {"env": name, "n_envs": N, "hidden1": h1, "hidden2": h2, "n_steps": box["T"], "repeats": args.repeats}
    for k in routes:
        row[k + "_ms"] = round(med[k], 4)
        row[k + "_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
    row.update(loop_over_deep=round(med["loop"] / med["deep"], 3), deep_over_one_layer=round(med["deep"] / med["one_layer"], 3),
               deep_us_per_step=round(1e3 * med["deep"] / box["T"], 3), kernel=kernel)
    print(json.dumps(row), flush=True)


def _widths(text):
    h1, h2 = (int(v) for v in text.split(","))
    return h1, h2


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", type=int, default=None, help="index of the one shape to run")
    ap.add_argument("--noise", action="store_true", help="time emei_rollout_policy_noisy against the deterministic launch and the noisy loop")
    ap.add_argument("--deep", type=_widths, default=None, metavar="H1,H2",
                    help="time emei_rollout_policy_deep at these widths against its per-step loop and the one-layer launch at H1")
    args = ap.parse_args()
    if args.noise and args.deep:
        raise SystemExit("--noise and --deep are separate measurements")
    if not torch.cuda.is_available():
        raise SystemExit("policy_timing.py needs a GPU")
    for idx, (name, N, T, kw) in enumerate(SHAPES):
        if args.only is not None and args.only != idx:
            continue
        eng = Engine(name, N, **kw)
        eng.reset(seed=0)
        state0 = eng.get_state().clone()
        policy = make_policy(eng)

        def restore():
            eng.reset(seed=0)
            eng.set_state(state0)
            torch.cuda.synchronize()

        def timed(fn):
            restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        if args.noise:
            noisy_shape(args, eng, name, N, T, policy, timed)
            eng.close()
            continue
        if args.deep:
            deep_shape(args, eng, name, N, T, timed)
            eng.close()
            continue
        outs = eng.alloc_outputs(T)
        fused = lambda: eng.rollout_policy(T, policy, auto_reset=True, out=outs)
        loop = lambda: loop_episode(eng, T, policy, outs)
        replay = lambda: eng.rollout(actions, auto_reset=True, out=outs)
        timed(fused)  # code objects loaded
        while timed(fused) < MIN_WINDOW_MS and 2 * T <= MAX_T:
            T *= 2
            outs = eng.alloc_outputs(T)
        kernel = eng.last_kernel()  # of the fused route (_lib.kernel_name)
        restore()
        actions = eng.rollout_policy(T, policy, auto_reset=True, out=outs)[0]
        for _ in range(args.warmup):
            timed(fused), timed(loop), timed(replay)
        ms = {"fused": [], "loop": [], "replay": []}
        for _ in range(args.repeats):
            ms["fused"].append(timed(fused))
            ms["loop"].append(timed(loop))
            ms["replay"].append(timed(replay))
        replay_kernel = eng.last_kernel()
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({
            "env": name, "n_envs": N, "hidden": HIDDEN, "n_steps": T, "repeats": args.repeats,
            "fused_ms": round(med["fused"], 4), "fused_ms_min_max": [round(min(ms["fused"]), 4), round(max(ms["fused"]), 4)],
            "loop_ms": round(med["loop"], 4), "loop_ms_min_max": [round(min(ms["loop"]), 4), round(max(ms["loop"]), 4)],
            "loop_over_fused": round(med["loop"] / med["fused"], 3),
            "replay_ms": round(med["replay"], 4), "replay_ms_min_max": [round(min(ms["replay"]), 4), round(max(ms["replay"]), 4)],
            "replay_kernel": replay_kernel,
            "fused_us_per_step": round(1e3 * med["fused"] / T, 3), "loop_us_per_step": round(1e3 * med["loop"] / T, 3),
            "kernel": kernel,
        }), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
