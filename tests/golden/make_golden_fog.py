#!/usr/bin/env python3
"""Generate tests/golden/fog_sight.npz (G11) by IMPORTING the reference (see make_golden.py, whose helpers this script uses;
like it, it runs only where the reference is present and copies nothing of it: numbers only).

Usage:
    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_fog.py

  G11 fog_sight.npz   GameState.makeObservation (capture.py:268-292) on reference GameStates rebuilt from records of existing
        fixtures -- the in_* states of scen_{small,tiny,blox}_random (every SCEN_STRIDE-th row, observer = row % 4) and the
        sub-step records of traj_{small,blox}_hunter (every TRAJ_STRIDE-th tick; record (t, i) is the state agent i's planes
        obs[t, i] were encoded from, observer i).  Per record: the source file and row / tick, the sub-step (-1: an in_* state),
        the observer, under random.seed(k) the four visibility flags (getAgentPosition(j) is not None) and the four sonar
        readings of makeObservation(observer), k, the next random.random() after the call, and per agent the Manhattan
        distance to the nearest agent of the observer's team (the reference's util.manhattanDistance).  A scen in_* state has
        no planes in its own fixture, so the reference's get_Observation(observer) of the rebuilt state is stored with it (bytes,
        one array per board).
"""
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG          # noqa: E402  (puts the reference on sys.path and chdirs to a scratch directory)
import util                       # noqa: E402  (the reference's)

OUT = MG.OUT
SOURCES = (("scen_small_random.npz", "small"), ("scen_tiny_random.npz", "tiny"), ("scen_blox_random.npz", "blox"),
           ("traj_small_hunter.npz", "small"), ("traj_blox_hunter.npz", "blox"))
SCEN_STRIDE, TRAJ_STRIDE = 3, 3
SEED0 = 1000
# shares of the recorded (observer, enemy) cases, asserted here per source and overall and again by tests/test_fog_cpu.py
MIN_SHARE = dict(hidden=0.15, visible=0.15, d5=0.01, d6=0.01)
STATE_KEYS = ("pos", "dir", "pac", "scared", "carry", "ret", "food", "caps", "score")


def shares(vis, near, observer):
    enemy = (np.arange(4)[None, :] % 2) != (observer[:, None] % 2)
    n = int(enemy.sum())
    return dict(hidden=float((~vis.astype(bool) & enemy).sum()) / n, visible=float((vis.astype(bool) & enemy).sum()) / n,
                d5=float(((near == 5) & enemy).sum()) / n, d6=float(((near == 6) & enemy).sum()) / n)


def main():
    recs = []
    planes = {}
    for s, (name, lay) in enumerate(SOURCES):
        z = np.load(os.path.join(OUT, name))
        env = MG.make_env(lay, 300)
        MG.quiet(env.reset)
        if name.startswith("scen"):
            todo = [(k, -1, k % 4, {key: z["in_" + key][k] for key in STATE_KEYS}) for k in range(0, len(z["in_pos"]), SCEN_STRIDE)]
        else:
            todo = [(t, i, i, {key: z["sub_" + key][t, i] for key in STATE_KEYS}) for t in range(0, len(z["sub_pos"]), TRAJ_STRIDE)
                    for i in range(4)]
        first = len(recs)
        for idx, sub, observer, st in todo:
            MG.inject(env, dict(st, steps=0))
            gs = env.game.state
            k = SEED0 + len(recs)
            random.seed(k)
            ob = gs.makeObservation(observer)
            nxt = random.random()
            team = [j for j in range(4) if j % 2 == observer % 2]
            near = [min(util.manhattanDistance(gs.getAgentPosition(j), gs.getAgentPosition(m)) for m in team) for j in range(4)]
            vis = [ob.getAgentPosition(j) is not None for j in range(4)]
            assert all(vis[m] for m in team) and gs.getAgentDistances() in (None, [])
            recs.append(dict(src=s, idx=idx, sub=sub, observer=observer, vis=vis, sonar=list(ob.getAgentDistances()), k=k, nxt=nxt,
                             near=near))
            if sub < 0:
                planes.setdefault(name, []).append(MG.obs_u8(env.get_Observation(observer)))
        mine = recs[first:]
        sh = shares(np.array([r["vis"] for r in mine]), np.array([r["near"] for r in mine]), np.array([r["observer"] for r in mine]))
        print(f"  {name}: records {len(mine)} shares {sh}", flush=True)
        for key, need in MIN_SHARE.items():
            assert sh[key] >= need, (name, key, sh[key], need)
    data = dict(src=np.array([r["src"] for r in recs], np.uint8), idx=np.array([r["idx"] for r in recs], np.int32),
                sub=np.array([r["sub"] for r in recs], np.int8), observer=np.array([r["observer"] for r in recs], np.uint8),
                vis=np.array([r["vis"] for r in recs], np.uint8), sonar=np.array([r["sonar"] for r in recs], np.int8),
                k=np.array([r["k"] for r in recs], np.int32), nxt=np.array([r["nxt"] for r in recs], np.float64),
                near=np.array([r["near"] for r in recs], np.uint8))
    assert (data["sonar"] == np.array([r["sonar"] for r in recs])).all()
    for name, p in planes.items():
        data["obs_" + name[:-4]] = np.stack(p)
    sh = shares(data["vis"], data["near"], data["observer"])
    for key, need in MIN_SHARE.items():
        assert sh[key] >= need, ("all", key, sh[key], need)
    meta = dict(sources=[n for n, _ in SOURCES], scen_stride=SCEN_STRIDE, traj_stride=TRAJ_STRIDE, seed0=SEED0, shares=sh,
                min_share=MIN_SHARE, sight_range=5,
                source="capture.GameState.makeObservation(observer) under random.seed(k) on GameStates rebuilt from the records; "
                       "nxt = random.random() right after; obs_scen_* = gymPacMan.get_Observation(observer) of the rebuilt in_* states")
    data["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    path = os.path.join(OUT, "fog_sight.npz")
    np.savez_compressed(path, **data)
    print(f"  fog_sight.npz: records {len(recs)} shares {sh} size={os.path.getsize(path)}", flush=True)
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
