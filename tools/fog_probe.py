"""Measurements of the fog-of-war path (profiles/fog_of_war/README.md).

  emit   launches pmx_emit_team_obs, pmx_emit_team_obs_fog, pmx_emit_team_obs_mixed and pmx_emit_team_obs_mixed_fog on byte planes,
         for a `rocprofv3 --kernel-trace --stats` run (the kernels' own durations come from the profiler), following
         tools/mix_probe.py emit, and prints the wall time per launch of each
  eval   greedy win rate of an EMA checkpoint (tools/train.py --save) against the in-kernel baselineTeam, evaluated with full
         information and under the sight rule
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import pmx
from pmx import mappo, trainer


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
    s = args.sight_range
    out = {"envs": N, "layout": args.layout, "launches": args.launches, "sight_range": s}
    full = torch.empty_like(team[0])
    env.emit_team_obs(False, full, None)
    env.emit_team_obs(False, team[0], None, sight_range=s)
    out["enemy_cells"], out["enemy_cells_seen"] = int((full[:, :, 5] != 0).sum()), int((team[0][:, :, 5] != 0).sum())
    for name, call in (("uniform", lambda k: env.emit_team_obs(False, team[k], merged[k])),
                       ("uniform_fog", lambda k: env.emit_team_obs(False, team[k], merged[k], sight_range=s)),
                       ("mixed", lambda k: env.emit_team_obs_mixed(red, team[k], merged[k])),
                       ("mixed_fog", lambda k: env.emit_team_obs_mixed(red, team[k], merged[k], sight_range=s))):
        for k in range(20):
            call(k % n_slots)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(args.launches):
            call(k % n_slots)
        torch.cuda.synchronize()
        out[name + "_wall_us"] = round((time.perf_counter() - t0) / args.launches * 1e6, 2)
    print(json.dumps(out))


def evaluate(args):
    lay = pmx.get_layout(args.layout)
    model = mappo.MAPPOAgent((8, lay.height, lay.width), 5, 2).cuda()
    model.load_state_dict(torch.load(args.checkpoint, map_location="cuda", weights_only=True))
    out = {"checkpoint": os.path.basename(args.checkpoint), "layout": args.layout, "episodes": args.episodes, "opponent": "baseline",
           "sight_range": args.sight_range}
    for name, kw in (("full", {}), ("fog", dict(fog_of_war=True, sight_range=args.sight_range))):
        mean, std, rate = trainer.evaluate_vectorized(model, args.layout, args.episodes, "baseline", seed=args.seed, **kw)
        out[name] = {"win_rate": rate, "return_mean": round(mean, 3), "return_std": round(std, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["emit", "eval"])
    ap.add_argument("--layout", default="smallCapture")
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--launches", type=int, default=520)
    ap.add_argument("--sight-range", type=int, default=5)
    ap.add_argument("--checkpoint", default="")
    ap.add_argument("--episodes", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    {"emit": emit, "eval": evaluate}[a.what](a)
