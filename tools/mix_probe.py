"""Measurements of the mixed-opponent path (profiles/mix_opponents/README.md).

  emit     launches pmx_emit_team_obs and pmx_emit_team_obs_mixed on byte planes, for a `rocprofv3 --kernel-trace --stats` run
           (the kernels' own durations come from the profiler) and prints the wall time per launch of each
  rollout  ticks per second of a phase-3 mixed rollout and of a default self-play rollout at the same env count
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import pmx
from pmx import trainer


def emit(args):
    N = args.envs
    env = pmx.PmxVecEnv(args.layout, N, obs_dtype="uint8", seed=1)
    env.reset(want_obs=False)
    g = torch.Generator(device="cuda").manual_seed(2)
    for _ in range(8):                                          # a few ticks: valid snapshots, agents off their starts
        env.step(torch.randint(0, 5, (N, 4), generator=g, device="cuda", dtype=torch.int8), want_obs=False)
    n_slots = 4                                                 # rotate the outputs, as bench.py's emit probe does
    team = [torch.empty((N, 2) + env.obs_shape, dtype=torch.uint8, device="cuda") for _ in range(n_slots)]
    merged = [torch.empty((N,) + env.obs_shape, dtype=torch.uint8, device="cuda") for _ in range(n_slots)]
    red = (torch.rand(N, generator=g, device="cuda") < 0.5).to(torch.uint8)
    out = {"envs": N, "layout": args.layout, "launches": args.launches}
    for name, call in (("uniform_blue", lambda k: env.emit_team_obs(False, team[k], merged[k])),
                       ("uniform_red", lambda k: env.emit_team_obs(True, team[k], merged[k])),
                       ("mixed", lambda k: env.emit_team_obs_mixed(red, team[k], merged[k]))):
        for k in range(20):
            call(k % n_slots)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(args.launches):
            call(k % n_slots)
        torch.cuda.synchronize()
        out[name + "_wall_us"] = round((time.perf_counter() - t0) / args.launches * 1e6, 2)
    print(json.dumps(out))


def rollout(args):
    out = {"envs": args.envs, "horizon": args.horizon, "layout": args.layout}
    for name, kw, idx in (("default_self", dict(opponent="self"), 0),
                          ("mixed_phase3", dict(opponent="curriculum", curriculum_scale=0.01, hard_bots=("baseline", "approxq"), mix_opponents=True), 9)):
        tr = trainer.VecMAPPOTrainer(args.layout, args.envs, horizon=args.horizon, minibatch=8192, seed=0, **kw)
        tr.update_idx = idx
        tr.rollout()                                            # warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            tr.rollout()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        times.sort()
        med = times[len(times) // 2]
        out[name] = {"ticks_per_s": round(args.horizon / med, 1), "env_steps_per_s": round(args.horizon * args.envs / med), "median_s": round(med, 4),
                     "min_s": round(times[0], 4), "max_s": round(times[-1], 4)}
        if name == "mixed_phase3":
            out["plan"] = [[m, bool(r), f, c] for m, r, f, c in tr.mix_groups]
        tr.env.close()
        del tr
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["emit", "rollout"])
    ap.add_argument("--layout", default="smallCapture")
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    {"emit": emit, "rollout": rollout}[a.what](a)
