"""Measurements of the belief sets (profiles/belief/README.md), of the belief weights (profiles/belief_weights/README.md) and of the
belief evidence (profiles/belief_evidence/README.md).

  times      the kernels' own durations (the start / stop events pmx_profile_begin attaches to each dispatch) of pmx_belief_update,
             pmx_emit_team_obs_belief and pmx_emit_team_obs_fog on byte planes, interleaved launch by launch in one process after a
             warm-up, and the budget a reviewer would hold the belief emission to: the fog emission's time plus the time of 512
             more bytes per env at the fog emission's own bandwidth; also pmx_belief_weights_update and
             pmx_emit_team_obs_weighted in the same rotation, with their budgets: the set update plus 10 HW more bytes per env,
             the belief emission plus 2 HW more bytes per env, both at the fog emission's bandwidth; and the evidence forms of the
             two updates, each with its yardstick: the parent's time plus 288 + 8 H more bytes per env at that bandwidth
  tightness  over a game of in-kernel baselineTeam bots on both sides: the mean size of a hidden enemy's set and the share of
             hidden cases whose set still holds the enemy's start cell while the enemy is more than 6 cells from it (the price of
             the respawn rule), for blue learners' second slot, whose snapshot is the end-of-tick state pmx_get_state returns;
             and, from the weights, the mean share of a hidden enemy's total weight on its true cell against 1 / |set|, and the
             share of the weight on the start cell in the "start cell kept, enemy more than 6 away" cases; all of it without
             and with the belief evidence (--rules, default all three), on the same game
  eval       greedy win rate of an EMA checkpoint (tools/train.py --save) against the in-kernel baselineTeam under fog, with or
             without the belief sets (--belief) or with the belief weights (--belief-weights)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import pmx
from pmx import mappo, trainer


def times(args):
    N, s = args.envs, args.sight_range
    env = pmx.PmxVecEnv(args.layout, N, obs_dtype="uint8", seed=1)
    env.reset(want_obs=False)
    g = torch.Generator(device="cuda").manual_seed(2)
    n_slots = 4                                                 # rotate the outputs and the buffers
    bel = [env.belief_init(env.new_belief(), 0) for _ in range(n_slots)]
    wb = [env.belief_weights_init(env.new_belief(), *env.new_belief_weights(), 0) for _ in range(n_slots)]
    eb = [(env.belief_init(env.new_belief(), 0), env.belief_evidence_init(env.new_belief_evidence())) for _ in range(n_slots)]
    ewb = [(env.belief_weights_init(env.new_belief(), *env.new_belief_weights(), 0), env.belief_evidence_init(env.new_belief_evidence()))
           for _ in range(n_slots)]
    for _ in range(8):                                          # a few ticks: valid snapshots, agents off their starts, sets of many cells
        env.step(torch.randint(0, 5, (N, 4), generator=g, device="cuda", dtype=torch.int8), want_obs=False)
        for b in bel:
            env.belief_update(False, b, s, reset=env.done)
        for b in wb:
            env.belief_weights_update(False, *b, s, reset=env.done)
        for b, e in eb:
            env.belief_update(False, b, s, reset=env.done, evidence=e)
        for b, e in ewb:
            env.belief_weights_update(False, *b, s, reset=env.done, evidence=e)
    team = [torch.empty((N, 2) + env.obs_shape, dtype=torch.uint8, device="cuda") for _ in range(n_slots)]
    merged = [torch.empty((N,) + env.obs_shape, dtype=torch.uint8, device="cuda") for _ in range(n_slots)]
    t = {"update": [], "emit_belief": [], "emit_fog": [], "update_weights": [], "emit_weighted": [], "update_evidence": [],
         "update_weights_evidence": []}
    for k in range(args.warmup + args.launches):
        i = k % n_slots
        env.profile_begin(4)
        env.belief_update(False, bel[i], s)
        env.emit_team_obs(False, team[i], merged[i], belief=bel[i])
        a = env.profile_end()
        env.profile_begin(4)
        env.emit_team_obs(False, team[i], merged[i], sight_range=s)
        b = env.profile_end()
        env.profile_begin(4)
        env.belief_weights_update(False, *wb[i], s)
        env.emit_team_obs(False, team[i], merged[i], levels=wb[i][2])
        c = env.profile_end()
        env.profile_begin(4)
        env.belief_update(False, eb[i][0], s, evidence=eb[i][1])
        d = env.profile_end()
        env.profile_begin(4)
        env.belief_weights_update(False, *ewb[i][0], s, evidence=ewb[i][1])
        e = env.profile_end()
        if k >= args.warmup:
            t["update_evidence"].append(d["rule_ms"] * 1e3)
            t["update_weights_evidence"].append(e["rule_ms"] * 1e3)
            t["update_weights"].append(c["rule_ms"] * 1e3)
            t["emit_weighted"].append(c["expand_ms"] * 1e3)
            t["update"].append(a["rule_ms"] * 1e3)
            t["emit_belief"].append(a["expand_ms"] * 1e3)
            t["emit_fog"].append(b["expand_ms"] * 1e3)
    H, W = env.layout.height, env.layout.width
    out = {"envs": N, "layout": args.layout, "launches": args.launches, "warmup": args.warmup, "sight_range": s,
           "mean_set_cells": round(float(sum(bin(int(w) & 0xFFFFFFFF).count("1") for w in bel[0][:256].cpu().numpy().ravel())) / (256 * 4), 2)}
    for name, v in t.items():
        v = np.array(v)
        out[name + "_us"] = {"mean": round(float(v.mean()), 3), "median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3),
                             "max": round(float(v.max()), 3), "std": round(float(v.std()), 3)}
    fog, belief, upd = (out[k + "_us"]["mean"] for k in ("emit_fog", "emit_belief", "update"))
    stored = 3 * 8 * H * W                                      # bytes an emission stores per env (three slots of byte planes)
    out["update_share_of_fog_emission"] = round(upd / fog, 4)
    out["fog_emission_GBps"] = round(N * stored / (fog * 1e-6) / 1e9, 1)
    out["belief_emission_budget_us"] = round(fog * (1 + 512 / stored), 3)
    out["belief_emission_excess_us"] = round(belief - out["belief_emission_budget_us"], 3)
    wupd, wemit = out["update_weights_us"]["mean"], out["emit_weighted_us"]["mean"]
    per_byte = fog / stored                                     # us per byte and env at the fog emission's bandwidth
    out["weights_update_budget_us"] = round(upd + 10 * H * W * per_byte, 3)        # reads 2 * 2 * HW, writes 4 * 2 * HW + 2 * HW more bytes
    out["weights_update_excess_us"] = round(wupd - out["weights_update_budget_us"], 3)
    out["weighted_emission_budget_us"] = round(belief + 2 * H * W * per_byte, 3)
    out["weighted_emission_excess_us"] = round(wemit - out["weighted_emission_budget_us"], 3)
    extra = 144 + 144 + 2 * 4 * H                               # the evidence row read and written, two snapshots' food rows read
    for name, parent in (("update_evidence", upd), ("update_weights_evidence", wupd)):
        out[name + "_yardstick_us"] = round(parent + extra * per_byte, 3)
        out[name + "_excess_us"] = round(out[name + "_us"]["mean"] - out[name + "_yardstick_us"], 3)
    print(json.dumps(out))


def tightness(args):
    N, T, s = args.envs, args.ticks, args.sight_range
    env = pmx.PmxVecEnv(args.layout, N, length=T, obs_dtype="uint8", seed=args.seed, bots=True)
    env.reset(want_obs=False)
    lay = env.layout
    starts = lay.starts.astype(np.int64)
    codes = torch.tensor([-3, -3, -4, -4], dtype=torch.int8, device="cuda")[None].expand(N, 4).contiguous()
    H, W = lay.height, lay.width
    # the same game for both trackers: "parent" without evidence, "evidence" with the rules of --rules
    trackers = {"parent": (env.belief_weights_init(env.new_belief(), *env.new_belief_weights(), 0), None),
                "evidence": (env.belief_weights_init(env.new_belief(), *env.new_belief_weights(), 0), env.belief_evidence_init(env.new_belief_evidence()))}
    acc = {name: dict(hidden=0, cells=0, with_start=0, true_share=0.0, uniform_share=0.0, start_share=0.0) for name in trackers}
    for _ in range(T):
        env.step(codes, want_obs=False)
        st = env.get_state()
        pos = np.array([[[p.pos[i][0], p.pos[i][1]] for i in range(4)] for p in st], np.int64)
        live = ~env.done.cpu().numpy().astype(bool)
        ar = np.arange(N)
        for name, ((bel, wts, lev), evidence) in trackers.items():
            kw = {} if evidence is None else {"evidence": evidence, "rules": args.rules}
            env.belief_weights_update(False, bel, wts, lev, s, reset=env.done, **kw)   # (the sets come out as the set update leaves them)
            a = acc[name]
            words = bel[:, 1].cpu().numpy().view(np.uint32)     # blue learners' second slot: the end-of-tick state
            q = wts[:, 1].cpu().numpy().view(np.uint16).astype(np.float64).reshape(N, 2, H, W)
            for k, e in enumerate((0, 2)):
                d = np.minimum(np.abs(pos[:, e] - pos[:, 1]).sum(1), np.abs(pos[:, e] - pos[:, 3]).sum(1))
                h = live & (d > s)
                size = np.array([sum(bin(int(w)).count("1") for w in words[n, k]) for n in np.nonzero(h)[0]])
                a["hidden"] += int(h.sum())
                a["cells"] += int(size.sum())
                sx, sy = int(starts[e, 0]), int(starts[e, 1])
                has = ((words[:, k, sy] >> np.uint32(sx)) & 1).astype(bool)
                away = np.abs(pos[:, e] - starts[e]).sum(1) > 6
                a["with_start"] += int((h & has & away).sum())
                total = np.maximum(q[:, k].sum((1, 2)), 1.0)
                a["true_share"] += float((q[ar, k, pos[:, e, 1], pos[:, e, 0]] / total)[h].sum())
                a["uniform_share"] += float((1.0 / np.maximum((q[:, k] > 0).sum((1, 2)), 1))[h].sum())
                a["start_share"] += float((q[:, k, sy, sx] / total)[h & has & away].sum())
    out = {"layout": args.layout, "envs": N, "ticks": T, "sight_range": s, "rules": args.rules}
    for name, a in acc.items():
        hidden = max(a["hidden"], 1)
        out[name] = {"hidden_cases": a["hidden"], "mean_set_cells": round(a["cells"] / hidden, 2),
                     "start_cell_kept_while_far_share": round(a["with_start"] / hidden, 4),
                     "weight_share_on_true_cell": round(a["true_share"] / hidden, 4),
                     "uniform_share_one_over_set": round(a["uniform_share"] / hidden, 4),
                     "weight_share_on_start_cell_while_far": round(a["start_share"] / max(a["with_start"], 1), 4)}
    print(json.dumps(out))


def evaluate(args):
    lay = pmx.get_layout(args.layout)
    model = mappo.MAPPOAgent((8, lay.height, lay.width), 5, 2).cuda()
    model.load_state_dict(torch.load(args.checkpoint, map_location="cuda", weights_only=True))
    kw = dict(fog_of_war=True, sight_range=args.sight_range, **({"belief": True} if args.belief or args.belief_weights or args.belief_evidence else {}),
              **({"belief_weights": True} if args.belief_weights else {}), **({"belief_evidence": True} if args.belief_evidence else {}))
    mean, std, rate = trainer.evaluate_vectorized(model, args.layout, args.episodes, "baseline", seed=args.seed, **kw)
    print(json.dumps({"checkpoint": os.path.basename(args.checkpoint), "layout": args.layout, "episodes": args.episodes, "opponent": "baseline",
                      "sight_range": args.sight_range, "belief": bool(args.belief or args.belief_weights), "belief_weights": bool(args.belief_weights), "belief_evidence": bool(args.belief_evidence), "win_rate": rate, "return_mean": round(mean, 3),
                      "return_std": round(std, 3)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["times", "tightness", "eval"])
    ap.add_argument("--layout", default="smallCapture")
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--launches", type=int, default=520)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--sight-range", type=int, default=5)
    ap.add_argument("--checkpoint", default="")
    ap.add_argument("--belief", action="store_true")
    ap.add_argument("--belief-weights", action="store_true")
    ap.add_argument("--belief-evidence", action="store_true")
    ap.add_argument("--rules", type=int, default=7, help="tightness: the PMX_EVIDENCE_* bits of the second tracker")
    ap.add_argument("--episodes", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    {"times": times, "tightness": tightness, "eval": evaluate}[a.what](a)
