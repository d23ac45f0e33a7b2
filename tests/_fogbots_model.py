"""The in-kernel bots under the contest's sight rule (pmx_set_bot_sight), restated in plain Python for the tests.

_approxq_model.Model with the two features that read an enemy put under a `seen` mask, and the visibility rule itself:

    mate M = (I + 2) % 4, enemies O = (I + 1) % 4 and (I + 3) % 4
    seen(O) = min(manhattan(P[O], P[I]), manhattan(P[O], P[M])) <= sight_range, positions of the state the decision starts from

A defender counts an enemy as an invader of a successor only when it is seen; the forager counts a ghost only when it is seen.
Everything else (successors, the walk home, the draws) is the parent model's.  It is pinned by the reference's own numbers on
observations (fixture G12, tests/test_fogbots_cpu.py) and is then what the GPU tests compare the kernels with.
"""
import functools

import numpy as np

import _golden as G
from _approxq_model import (AQ_DEF, AQ_OFF, BASE_DEF, BASE_OFF, ORDER, RANDOM, REV, VEC, Model, states_from_arrays, to_pstates)

FLAG_SEEN_LO, FLAG_SEEN_HI = 4, 8


def foes(i):
    """The two enemies of agent i, lower index first (the order of the seen flags)."""
    return (1, 3) if i % 2 == 0 else (0, 2)


def seen_flags(st, i, sight):
    """(seen(lower enemy), seen(higher enemy)) for agent i deciding on state st; sight None: nothing is hidden."""
    if sight is None:
        return (True, True)
    team = (i, (i + 2) % 4)
    out = []
    for o in foes(i):
        d = min(abs(int(st["pos"][o][0]) - int(st["pos"][m][0])) + abs(int(st["pos"][o][1]) - int(st["pos"][m][1])) for m in team)
        out.append(d <= sight)
    return tuple(out)


class FogModel(Model):
    def q_features(self, st, i, a, prey=None, seen=(True, True)):
        x, y = int(st["pos"][i][0]) + VEC[a][0], int(st["pos"][i][1]) + VEC[a][1]
        g = 0
        for o, s in zip(foes(i), seen):
            if s and not st["pac"][o]:
                g += abs(int(st["pos"][o][0]) - x) + abs(int(st["pos"][o][1]) - y) <= 1
        if prey is None:
            prey = self.prey(st, i)
        eats = g == 0 and (x, y) in prey
        d = 255
        if prey:
            rows = self.cell[[p[1] for p in prey], [p[0] for p in prey]]
            d = int(self.dist[self.cell[y, x], rows].min())
        return g, eats, (None if d == 255 else d)

    def reflex_value(self, st, nx, i, a, defensive, seen=(True, True)):
        if not defensive:
            return Model.reflex_value(self, st, nx, i, a, False)
        me = (int(nx["pos"][i][0]), int(nx["pos"][i][1]))
        val, gap = (0 if nx["pac"][i] else 100), None
        for o, s in zip(foes(i), seen):
            if s and nx["pac"][o]:
                val -= 1000
                d = self.maze(me, (int(nx["pos"][o][0]), int(nx["pos"][o][1])))
                gap = d if gap is None else min(gap, d)
        if gap is not None:
            val -= 10 * gap
        return val - (100 if a == 4 else 0) - (2 if a == REV[int(st["dir"][i])] else 0)

    def evaluate(self, st, i, code, pst=None, sight=None, seen_from_successor=False):
        """Model.evaluate with the sight rule; the result also carries `seen`.  seen_from_successor (a negative control of the
        tests): visibility decided on each successor instead of on st, which the reference does not do."""
        if pst is None:
            pst = to_pstates(st.reshape(1))[0]
        seen = seen_flags(st, i, sight)
        legal = self.legal_mask(st, i)
        values = np.full(5, np.nan)
        prey = self.prey(st, i)
        out = dict(legal=legal, values=values, food_left=len(prey), home=-1, seen=seen,
                   g=np.full(5, -1), eats=np.full(5, -1), d=np.full(5, -1))
        for a in ORDER:
            if not (legal >> a) & 1:
                continue
            if code == RANDOM:
                values[a] = 0.0
            elif code == AQ_OFF:
                g, eats, d = self.q_features(st, i, a, prey, seen)
                values[a] = self.q_value(g, eats, d)
                out["g"][a], out["eats"][a], out["d"][a] = g, int(eats), (-1 if d is None else d)
            else:
                nx = self.successor(pst, i, a)
                s = seen_flags(nx, i, sight) if seen_from_successor else seen
                values[a] = float(self.reflex_value(st, nx, i, a, code in (BASE_DEF, AQ_DEF), s))
        top = np.nanmax(values)
        out["best"] = sum(1 << a for a in range(5) if values[a] == top)
        home_at = {RANDOM: -1, BASE_OFF: 0, BASE_DEF: 0, AQ_OFF: 2, AQ_DEF: 2}[code]
        if out["food_left"] <= home_at:
            out["home"] = self.home_action(pst, i, legal)
        return out

    def decide(self, st, i, code, seed, env, pst=None, sight=None):
        """-> (evaluation, action, flags as pmx_bot_query reports them on a handle with that bot sight)."""
        ev = self.evaluate(st, i, code, pst, sight)
        act, flags = self.play(ev, code, seed, env, int(st["ticks"]), i)
        if sight is not None and code != RANDOM:
            flags |= (FLAG_SEEN_LO if ev["seen"][0] else 0) | (FLAG_SEEN_HI if ev["seen"][1] else 0)
        return ev, act, flags


# ---- fixture G12 (tests/golden/fogbots.npz) ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def load_g12():
    """-> (records, meta, sources, G11's arrays).  records: G12's arrays plus src (the source of each record's G11 row);
    sources[s] = dict(name, layout rows, rows = the G11 rows of that source, states = STATE records of those rows in that order,
    observer, local = {G11 row: index into states})."""
    rec, meta = G.load("fogbots.npz")
    d11, meta11 = G.load("fog_sight.npz")
    sources = []
    for s, name in enumerate(meta11["sources"]):
        src, smeta = G.load(name)
        rows = np.nonzero(d11["src"] == s)[0]
        idx, sub = d11["idx"][rows], d11["sub"][rows]
        if name.startswith("scen"):
            f = {k: src["in_" + k][idx] for k in G.SNAP_KEYS}
        else:
            f = {k: src["sub_" + k][idx, sub] for k in G.SNAP_KEYS}
        states = states_from_arrays(*(f[k] for k in G.SNAP_KEYS), steps=np.zeros(len(rows), np.int32))
        sources.append(dict(name=name, layout=smeta["layout"], rows=rows, states=states, observer=d11["observer"][rows],
                            local={int(r): n for n, r in enumerate(rows)}))
    rec["src"] = d11["src"][rec["row"]]
    return rec, meta, sources, d11


@functools.lru_cache(maxsize=None)
def model_of(s):
    """The model of source s's board (one per layout text)."""
    return _model(tuple(load_g12()[2][s]["layout"]))


@functools.lru_cache(maxsize=None)
def _model(rows):
    return FogModel(list(rows))
