"""Measurements of the game records (profiles/game_record/README.md).

  kernel      the kernels' own durations (the start / stop events pmx_profile_begin attaches to each dispatch) of
              pmx_game_record_update and of pmx_episode_stats_update -- the kernel it is modelled on -- interleaved launch by launch
              in one process after a warm-up, with the bytes each moves per env and the bandwidth that makes.  The logs hold
              --max-ticks ticks and start over when full, four of them in rotation, so that the frames written are not the ones
              just written
  throughput  wall time of play_match (a greedy network against the in-kernel baselineTeam, both colours) with record=--record and
              with record=0 on the same model, layout, games and seed, alternating, --repeats times each
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
    recs = [env.game_record_init(env.new_game_record(max_ticks=args.max_ticks)) for _ in range(n_slots)]
    for _ in range(8):                                          # a few ticks: valid snapshots, agents off their starts
        env.step(torch.randint(0, 5, (N, 4), generator=g, device="cuda", dtype=torch.int8), want_obs=False)
    t = {"game_record_update": [], "episode_stats_update": []}
    filled = [0] * n_slots
    for k in range(args.warmup + args.launches):
        i = k % n_slots
        if filled[i] == args.max_ticks:                         # start the log over, outside the timed launches
            recs[i].head[pmx._lib.RECORD_LEN].zero_()
            filled[i] = 0
        env.profile_begin(4)
        env.game_record_update(recs[i])                         # done_dev NULL: no row is ever DONE, every launch does all the work
        a = env.profile_end()
        filled[i] += 1
        env.profile_begin(4)
        env.episode_stats_update(stats[i])
        b = env.profile_end()
        assert a["rule_launches"] == 1 and b["rule_launches"] == 1
        if k >= args.warmup:
            t["game_record_update"].append(a["rule_ms"] * 1e3)
            t["episode_stats_update"].append(b["rule_ms"] * 1e3)
    assert all(int(r.head[pmx._lib.RECORD_OVERFLOW].sum()) == 0 for r in recs)
    H = env.layout.height
    fw = 12 + H
    out = {"envs": N, "layout": args.layout, "board_rows": H, "launches": args.launches, "warmup": args.warmup, "max_ticks": args.max_ticks}
    for name, v in t.items():
        out[name + "_us"] = _summary(v)
    # bytes per env.  record: 3 head words, the previous frame's 11, 4 x 10 snapshot words, the score word and 4 H food rows
    # loaded; 4 frames and 2 head words stored.  stats: 43 words of the row and 4 x 10 snapshot words + the score word loaded, 45 stored
    out["record_bytes_per_env"] = {"loaded": 4 * (3 + 11 + 41 + 4 * H), "stored": 4 * (4 * fw + 2)}
    out["stats_bytes_per_env"] = {"loaded": 4 * (43 + 41), "stored": 4 * 45}
    for name, key in (("game_record_update", "record_bytes_per_env"), ("episode_stats_update", "stats_bytes_per_env")):
        b = sum(out[key].values()) * N
        out[name + "_GBps"] = round(b / (out[name + "_us"]["median"] * 1e-6) / 1e9, 1)
    out["record_bandwidth_over_stats_bandwidth"] = round(out["game_record_update_GBps"] / out["episode_stats_update_GBps"], 3)
    print(json.dumps(out))


def throughput(args):
    dev = "cuda:0"
    lay = pmx.get_layout(args.layout)
    torch.manual_seed(args.seed)
    model = mappo.MAPPOAgent((8, lay.height, lay.width), 5, 2).to(dev)
    kw = dict(layout=args.layout, n_envs=args.games, length=args.length, device=dev, seed=args.seed, colours="both")
    a, b = trainer.MatchSide(model=model, greedy=True), trainer.MatchSide(bot="baseline")

    def timed(record):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = trainer.play_match(a, b, record=record, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    timed(0)                                                    # warm-up of both paths
    timed(args.record)
    t_plain, t_rec = [], []
    for _ in range(args.repeats):
        dt, r0 = timed(0)
        t_plain.append(dt)
        dt, r1 = timed(args.record)
        t_rec.append(dt)
    rec = r1["record"]
    out = {"layout": args.layout, "games": args.games, "length": args.length, "repeats": args.repeats, "record": args.record,
           "play_match_record_0_s": [round(x, 4) for x in t_plain], "play_match_record_k_s": [round(x, 4) for x in t_rec],
           "record_0_spread_s": round(max(t_plain) - min(t_plain), 4),
           "record_k_minus_record_0_mean_s": round(float(np.mean(t_rec) - np.mean(t_plain)), 4),
           "ticks_mean": r1["ticks_mean"], "same_scores": bool(torch.equal(r0["score"], r1["score"])),
           "record_host_bytes": int(rec.head.nbytes + rec.frames.nbytes)}
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernel", "throughput"])
    ap.add_argument("--layout", default="smallCapture")
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--launches", type=int, default=520)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--max-ticks", type=int, default=16)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--record", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    {"kernel": kernel, "throughput": throughput}[args.what](args)
