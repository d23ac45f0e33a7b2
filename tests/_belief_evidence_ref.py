"""The evidence rules of include/pmx.h ("Belief evidence") restated in numpy on boolean cell grids, on top of tests/_belief_ref.py
(sets, readings, sight) and tests/_belief_weights_ref.py (the weights, which take this model's sets unchanged).
tests/test_belief_evidence_cpu.py holds it to the golden trajectories; the GPU tests compare pmx_belief_update_evidence /
pmx_belief_weights_update_evidence with it word for word.  Vectorised over n envs.  The knobs side_swap / food_offset / contact
exist for the negative controls only."""
import numpy as np

import _belief_ref as B
import _belief_weights_ref as BW

SIDE, FOOD, CONTACT, WORDS = 1, 2, 4, 36


def init(n):
    """pmx_belief_evidence_init -> [n, 36] uint32, all zero (valid = 0)"""
    return np.zeros((n, WORDS), np.uint32)


def _xy(word):
    w = np.asarray(word).astype(np.int64)
    return np.stack([w & 0xFF, (w >> 8) & 0xFF], -1)


def _near(p, radius=1):
    return B.dist_to(p) <= radius


def update(prev, ev, P, F, red, sight, ticks, seed, env, open_g, starts, half, rules=7, reset=None, side_swap=False, food_offset=3,
           contact="previous", stats=None):
    """pmx_belief_update_evidence.  prev, P, red, sight, ticks, seed, env, open_g, starts, reset as _belief_ref.update; ev [n, 36] the
    evidence rows; F [n, 2 slots, 32] the food row words of the snapshot each learner slot is encoded from (rows >= H zero); half
    [n] or a number; rules likewise.  -> (words [n, 2, 2, 32], readings [n, 2, 2], seen [n, 2, 2], evidence rows [n, 36]).  stats (a dict): "food"
    counts the slots in which rule 2a fired, "excluded" those in which one pellet left but a distance test held the rule back."""
    n = len(prev)
    ar = np.arange(n)
    red = np.asarray(red).astype(bool)
    first = np.where(red, 0, 1)
    second = first + 2
    sight = np.broadcast_to(np.asarray(sight), (n,))
    half = np.broadcast_to(np.asarray(half), (n,))
    rules = np.broadcast_to(np.asarray(rules), (n,))                        # (a value per env is accepted too)
    P = np.asarray(P).astype(np.int64)
    F = np.asarray(F).astype(np.uint32)
    ev = np.asarray(ev).astype(np.uint32)
    starts = np.asarray(starts).astype(np.int64)
    lo = B._X[None] < half[:, None, None]                                   # columns x < half
    mine = np.where(red[:, None, None], lo, ~lo)
    valid = ev[:, 34] != 0
    # the previous snapshot of each slot: (exists, food cells, the team's two cells)
    before = [(valid, B.unpack(ev[:, :32]), _xy(ev[:, 32]), _xy(ev[:, 33])),
              (np.ones(n, bool), B.unpack(F[:, 0]), P[ar, 0, first], P[ar, 0, second])]
    out = np.zeros((n, 2, 2, 32), np.uint32)
    sonar = np.zeros((n, 2, 2), np.int64)
    seen_out = np.zeros((n, 2, 2), bool)
    for k in range(2):
        e_k = (1 - first) + 2 * k
        start_e = B.one_cell(starts[ar, e_k])
        S = B.unpack(prev[:, 1, k])
        for j in range(2):
            a_j = first + 2 * j
            Pj = P[:, j]
            pa, pe, pf, ps = Pj[ar, a_j], Pj[ar, e_k], Pj[ar, first], Pj[ar, second]
            has_prev, F_prev, qf, qs = before[j]
            qa = qs if j else qf
            moved = e_k == (a_j + 3) % 4
            S = np.where(moved[:, None, None], B._dilate(S) & open_g, S)
            E = F_prev & ~B.unpack(F[:, j]) & mine                           # 2a
            one = (rules & FOOD != 0) & has_prev & (e_k == (a_j + food_offset) % 4) & (E.sum((1, 2)) == 1)
            at = E.reshape(n, -1).argmax(1)
            c = np.stack([at % 32, at // 32], -1)
            fire = one & (B.manhattan(c, qa) > 1) & (B.manhattan(c, starts[ar, a_j]) > 1)
            S = np.where(fire[:, None, None], S & E, S)
            if stats is not None:
                stats["food"] = stats.get("food", 0) + fire.astype(np.int64)
                stats["excluded"] = stats.get("excluded", 0) + (one & ~fire).astype(np.int64)
            if contact == "previous":                                       # 3
                K = _near(qf) | _near(qs) | _near(starts[ar, first]) | _near(starts[ar, second])
            else:                                                           # the control: the team's cells now, radius 0
                K = _near(pf, 0) | _near(ps, 0)
            touch = (S & K).any((1, 2)) | ~has_prev | (rules & CONTACT == 0)
            S = S | (start_e & touch[:, None, None])
            r = B.manhattan(pa, pe) + B.noise(seed, env, ticks, 4 * a_j + e_k)
            seen = np.minimum(B.manhattan(pe, pf), B.manhattan(pe, ps)) <= sight
            hidden = S & (B.dist_to(pf) > sight[:, None, None]) & (B.dist_to(ps) > sight[:, None, None]) & B.annulus(pa, r)
            on_lo = (pe[:, 0] < half) != side_swap                          # 4
            hidden = hidden & (np.where(on_lo[:, None, None], lo, ~lo) | (rules & SIDE == 0)[:, None, None])
            S = np.where(seen[:, None, None], B.one_cell(pe), hidden)
            out[:, j, k] = B.pack(S)
            sonar[:, j, k] = r
            seen_out[:, j, k] = seen
        if reset is not None:
            rs = np.asarray(reset).astype(bool)
            out[rs, :, k] = B.pack(start_e)[rs, None]
    if reset is not None:
        sonar[np.asarray(reset).astype(bool)] = 0
    new = np.zeros((n, WORDS), np.uint32)                                   # 5: the slot-1 snapshot, reset rows too
    new[:, :32] = F[:, 1]
    new[:, 32] = (P[ar, 1, first, 0] | (P[ar, 1, first, 1] << 8)).astype(np.uint32)
    new[:, 33] = (P[ar, 1, second, 0] | (P[ar, 1, second, 1] << 8)).astype(np.uint32)
    new[:, 34] = 1
    return out, sonar, seen_out, new


class _Sets:
    """stands in for _belief_ref inside _belief_weights_ref.update: the same names, `update` returning sets computed beforehand"""

    def __init__(self, result):
        self._result = result

    def update(self, *a, **kw):
        return self._result

    def __getattr__(self, name):
        return getattr(B, name)


def weights_update(prev_w, prev_words, ev, P, F, red, sight, ticks, seed, env, open_g, starts, half, H, W, rules=7, reset=None):
    """pmx_belief_weights_update_evidence: the "Belief weights" table of _belief_weights_ref.update, unchanged, on this model's sets.
    -> (weights, levels, words, readings, seen, evidence rows)"""
    words, sonar, seen, new = update(prev_words, ev, P, F, red, sight, ticks, seed, env, open_g, starts, half, rules=rules, reset=reset)
    saved = BW.B
    BW.B = _Sets((words, sonar, seen))
    try:
        w, lev, _, _, _ = BW.update(prev_w, prev_words, P, red, sight, ticks, seed, env, open_g, starts, H, W, reset=reset)
    finally:
        BW.B = saved
    return w, lev, words, sonar, seen, new
