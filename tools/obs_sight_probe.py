"""Measurements of the sight rule on the four-agent planes and of pmx_agent_distances (profiles/obs_sight/README.md).

  expand   the expansion kernel's own duration (the start / stop events pmx_profile_begin attaches to the dispatch) through
           pmx_observe on ONE handle: plain, plain again, sight 5 -- launch by launch in that order, in one process, after a
           warm-up, the sweep direction fixed ("expand_alt" 0) so that the three launches of a round walk the planes the same way.
           plain_b - plain_a is the spread of repeated plain launches, sight - plain_a the cost of the rule.
  sonar    pmx_agent_distances (both forms) against pmx_episode_stats_update, the project's kernel of the same shape (one lane per
           env, snapshot words in, a few words out), interleaved launch by launch after a few ticks.

Each prints one JSON line and, with --out DIR, writes it to DIR/<what>.json.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import pmx


def _summary(v):
    v = np.array(v)
    return {"mean": round(float(v.mean()), 3), "median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3),
            "max": round(float(v.max()), 3), "std": round(float(v.std()), 3)}


def _mid_game(env, ticks=8):
    g = torch.Generator(device="cuda").manual_seed(2)
    for _ in range(ticks):                                      # agents off their starts, valid snapshots
        env.step(torch.randint(0, 5, (env.n_envs, 4), generator=g, device="cuda", dtype=torch.int8), want_obs=False)


def expand(args):
    env = pmx.PmxVecEnv(args.layout, args.envs, obs_dtype=args.dtype, seed=1, auto_reset=True)
    env.reset(want_obs=False)
    _mid_game(env)
    env.set_tuning("expand_alt", 0)

    def one(sight):
        env.set_obs_sight(sight)
        env.profile_begin(2)
        env.observe(want_legal=False)
        p = env.profile_end()
        assert p["expand_launches"] == 1 and p["rule_launches"] == 0
        return p["expand_ms"] * 1e3

    t = {"plain_a": [], "plain_b": [], "sight": []}
    for k in range(args.warmup + args.launches):
        a, b, s = one(None), one(None), one(args.sight)
        if k >= args.warmup:
            t["plain_a"].append(a), t["plain_b"].append(b), t["sight"].append(s)
    env.set_obs_sight(None)
    plain = env.observe(want_legal=False)[0].clone()
    env.set_obs_sight(args.sight)
    fog = env.observe(want_legal=False)[0]
    enemy, kept = int((plain[:, :, 5] != 0).sum()), int((fog[:, :, 5] != 0).sum())
    H, W = env.layout.height, env.layout.width
    out = {"what": "expand", "envs": args.envs, "layout": args.layout, "dtype": args.dtype, "sight": args.sight, "launches": args.launches,
           "warmup": args.warmup, "plane_bytes": int(plain.numel() * plain.element_size()), "board": [H, W],
           "enemy_cells": enemy, "hidden_share": round(1 - kept / max(enemy, 1), 4)}
    for name, v in t.items():
        out[name + "_us"] = _summary(v)
    d_rule = np.array(t["sight"]) - np.array(t["plain_a"])
    d_same = np.array(t["plain_b"]) - np.array(t["plain_a"])
    out["sight_minus_plain_us"] = _summary(d_rule)
    out["plain_minus_plain_us"] = _summary(d_same)
    return out


def sonar(args):
    N = args.envs
    env = pmx.PmxVecEnv(args.layout, N, obs_dtype="uint8", seed=1, auto_reset=False)
    env.reset(want_obs=False)
    n_slots = 4                                                 # rotate the buffers
    stats = [env.episode_stats_init(env.new_episode_stats()) for _ in range(n_slots)]
    full = [torch.empty((N, 4, 4), dtype=torch.int8, device="cuda") for _ in range(n_slots)]
    single = [torch.empty((N, 4), dtype=torch.int8, device="cuda") for _ in range(n_slots)]
    g = torch.Generator(device="cuda").manual_seed(2)
    for _ in range(8):
        env.step(torch.randint(0, 5, (N, 4), generator=g, device="cuda", dtype=torch.int8), want_obs=False)
        for s in stats:
            env.episode_stats_update(s)

    def one(f):
        env.profile_begin(2)
        f()
        p = env.profile_end()
        assert p["rule_launches"] == 1
        return p["rule_ms"] * 1e3

    t = {"agent_distances_all": [], "agent_distances_one": [], "episode_stats_update": []}
    for k in range(args.warmup + args.launches):
        i = k % n_slots
        a = one(lambda: env.agent_distances(out=full[i]))
        b = one(lambda: env.agent_distances(1, out=single[i]))
        c = one(lambda: env.episode_stats_update(stats[i]))
        if k >= args.warmup:
            t["agent_distances_all"].append(a), t["agent_distances_one"].append(b), t["episode_stats_update"].append(c)
    out = {"what": "sonar", "envs": N, "layout": args.layout, "launches": args.launches, "warmup": args.warmup,
           "all_bytes_per_env": 4 * 17 + 16, "one_bytes_per_env": 4 * 5 + 4, "stats_bytes_per_env": 4 * (43 + 41 + 45)}
    for name, v in t.items():
        out[name + "_us"] = _summary(v)
    out["ratio_all_to_episode_stats"] = round(out["agent_distances_all_us"]["mean"] / out["episode_stats_update_us"]["mean"], 3)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["expand", "sonar"])
    ap.add_argument("--layout", default="smallCapture")
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--dtype", default="float32")
    ap.add_argument("--sight", type=int, default=5)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    res = {"expand": expand, "sonar": sonar}[args.what](args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, args.what + ".json"), "w") as f:
            f.write(line + "\n")
