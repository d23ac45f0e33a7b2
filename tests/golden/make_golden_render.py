#!/usr/bin/env python3
"""Generate tests/golden/G13_render.json by IMPORTING the reference (see make_golden.py, whose helpers this script uses; like it,
it runs only where the reference is present and copies nothing of it: recorded results only).

Usage:
    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_render.py

  G13 G13_render.json   str(GameState.data) (game.py:438-461, GameStateData.__str__) of reference GameStates rebuilt from sub-step
        records of the trajectory fixtures.  Per record: the source file, tick and sub-step, the state's fields (so that the test
        needs no other file) and the text.  The records are chosen, per source, to cover: a scared ghost, a Pacman facing each of
        North / East / South / West, a Pacman with direction Stop where one exists, a board with a capsule eaten, an agent on
        either half as Pacman, and the file's first and last record; the script asserts the coverage over the whole fixture.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG          # noqa: E402  (puts the reference on sys.path and chdirs to a scratch directory)

OUT = MG.OUT
SOURCES = (("traj_small_hunter.npz", "small"), ("traj_tiny_hunter.npz", "tiny"), ("traj_blox_hunter.npz", "blox"),
           ("traj_maze23_hunter.npz", "maze23"), ("traj_maze4242_hunter.npz", "maze4242"))
STATE_KEYS = ("pos", "dir", "pac", "scared", "carry", "ret", "food", "caps", "score")
PER_SOURCE = 8


def popcount(rows):
    return sum(bin(int(r)).count("1") for r in rows)


def pick(z):
    """(tick, sub-step) records of one fixture, at most PER_SOURCE, one per wanted property in this order"""
    T = len(z["sub_pos"])
    caps0 = popcount(z["init_caps"])
    recs = [(t, s) for t in range(T) for s in range(4)]
    pac, d, scared = z["sub_pac"], z["sub_dir"], z["sub_scared"]
    wants = [lambda t, s: (scared[t, s] > 0).any()]
    wants += [(lambda k: lambda t, s: ((pac[t, s] == 1) & (d[t, s] == k)).any())(k) for k in range(5)]
    wants += [lambda t, s: popcount(z["sub_caps"][t, s]) < caps0,
              lambda t, s: pac[t, s][0] == 1 or pac[t, s][2] == 1, lambda t, s: pac[t, s][1] == 1 or pac[t, s][3] == 1]
    out = [recs[0], recs[-1]]
    for w in wants:
        hit = next((r for r in recs if w(*r) and r not in out), None)
        if hit is not None and len(out) < PER_SOURCE + 2:
            out.append(hit)
    return out[:PER_SOURCE]


def main():
    records, layouts = [], {}
    for name, lay in SOURCES:
        z = np.load(os.path.join(OUT, name))
        env = MG.make_env(lay, 300)
        MG.quiet(env.reset)
        layouts[name] = MG.layout_text(lay)
        for t, s in pick(z):
            st = {k: z["sub_" + k][t, s] for k in STATE_KEYS}
            MG.inject(env, dict(st, steps=0))
            text = str(env.game.state.data)
            records.append(dict(src=name, tick=t, sub=s, text=text, **{k: np.asarray(v).tolist() for k, v in st.items()}))
    # coverage over the whole fixture
    allpac = [(r["dir"][i]) for r in records for i in range(4) if r["pac"][i]]
    assert set(allpac) >= {0, 1, 2, 3}, sorted(set(allpac))
    assert any(max(r["scared"]) > 0 for r in records)
    assert any(popcount(r["caps"]) < popcount(np.load(os.path.join(OUT, r["src"]))["init_caps"]) for r in records)
    assert any(r["pac"][0] or r["pac"][2] for r in records) and any(r["pac"][1] or r["pac"][3] for r in records)
    assert 30 <= len(records) <= 45, len(records)
    with open(os.path.join(OUT, "G13_render.json"), "w") as f:
        json.dump(dict(layouts=layouts, records=records), f, separators=(",", ":"))
    print("G13_render.json", len(records), "records")


if __name__ == "__main__":
    main()
