"""Measurements of the episode statistics and the match runner (profiles/match/README.md).

  kernel      the kernels' own durations (the start / stop events pmx_profile_begin attaches to each dispatch) of
              pmx_episode_stats_update and of pmx_belief_update -- the project's kernel of the same shape, one small launch with
              dependent snapshot loads -- interleaved launch by launch in one process after a warm-up
  throughput  wall time of play_match (a greedy network against the in-kernel baselineTeam, both colours) and of
              evaluate_vectorized(side="both") on the same model, layout, games and seed, alternating, --repeats times each; the
              network is a freshly initialised MAPPOAgent unless --checkpoint names an EMA checkpoint (tools/train.py --save)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import pmx
from pmx import mappo, trainer


def _summary(v):
    v = np.array(v)
    return {"mean": round(float(v.mean()), 3), "median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3),
            "max": round(float(v.max()), 3), "std": round(float(v.std()), 3)}


def kernel(args):
    N = args.envs
    env = pmx.PmxVecEnv(args.layout, N, obs_dtype="uint8", seed=1, auto_reset=False)
    env.reset(want_obs=False)
    g = torch.Generator(device="cuda").manual_seed(2)
    n_slots = 4                                                 # rotate the buffers
    stats = [env.episode_stats_init(env.new_episode_stats()) for _ in range(n_slots)]
    bel = [env.belief_init(env.new_belief(), 0) for _ in range(n_slots)]
    for _ in range(8):                                          # a few ticks: valid snapshots, agents off their starts
        env.step(torch.randint(0, 5, (N, 4), generator=g, device="cuda", dtype=torch.int8), want_obs=False)
        for s in stats:
            env.episode_stats_update(s)
        for b in bel:
            env.belief_update(False, b, 5)
    t = {"episode_stats_update": [], "belief_update": []}
    for k in range(args.warmup + args.launches):
        i = k % n_slots
        env.profile_begin(4)
        env.episode_stats_update(stats[i])                      # done_dev NULL: no row is ever DONE, every launch does all the work
        a = env.profile_end()
        env.profile_begin(4)
        env.belief_update(False, bel[i], 5)
        b = env.profile_end()
        assert a["rule_launches"] == 1 and b["rule_launches"] == 1
        if k >= args.warmup:
            t["episode_stats_update"].append(a["rule_ms"] * 1e3)
            t["belief_update"].append(b["rule_ms"] * 1e3)
    H = env.layout.height
    out = {"envs": N, "layout": args.layout, "launches": args.launches, "warmup": args.warmup}
    for name, v in t.items():
        out[name + "_us"] = _summary(v)
    # bytes per env: 43 words of the row and 4 x 10 snapshot words + the score word loaded, 45 words stored
    out["stats_bytes_per_env"] = 4 * (43 + 41 + 45)
    out["belief_bytes_per_env"] = 768
    out["ratio_to_belief_update"] = round(out["episode_stats_update_us"]["mean"] / out["belief_update_us"]["mean"], 3)
    out["board_rows"] = H
    print(json.dumps(out))


def throughput(args):
    dev = "cuda:0"
    lay = pmx.get_layout(args.layout)
    torch.manual_seed(args.seed)
    model = mappo.MAPPOAgent((8, lay.height, lay.width), 5, 2).to(dev)
    if args.checkpoint:
        model.load_state_dict(torch.load(args.checkpoint, map_location=dev, weights_only=True))
    kw = dict(layout=args.layout, n_envs=args.games, length=args.length, device=dev, seed=args.seed)
    a, b = trainer.MatchSide(model=model, greedy=True), trainer.MatchSide(bot="baseline")

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    timed(lambda: trainer.evaluate_vectorized(model, opponent="baseline", side="both", **kw))      # warm-up of both paths
    timed(lambda: trainer.play_match(a, b, colours="both", **kw))
    t_eval, t_match = [], []
    for _ in range(args.repeats):
        dt, ev = timed(lambda: trainer.evaluate_vectorized(model, opponent="baseline", side="both", **kw))
        t_eval.append(dt)
        dt, r = timed(lambda: trainer.play_match(a, b, colours="both", **kw))
        t_match.append(dt)
    out = {"layout": args.layout, "games": args.games, "length": args.length, "repeats": args.repeats, "checkpoint": bool(args.checkpoint),
           "evaluate_vectorized_s": [round(x, 4) for x in t_eval], "play_match_s": [round(x, 4) for x in t_match],
           "evaluate_vectorized_spread_s": round(max(t_eval) - min(t_eval), 4),
           "play_match_minus_evaluate_mean_s": round(float(np.mean(t_match) - np.mean(t_eval)), 4),
           "ticks_mean": r["ticks_mean"], "win_rate_equal": r["win_rate_a"] == ev[2], "return_diff": abs(r["return_a"] - ev[0])}
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernel", "throughput"])
    ap.add_argument("--layout", default="smallCapture")
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--launches", type=int, default=520)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--checkpoint", default="")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    {"kernel": kernel, "throughput": throughput}[args.what](args)
