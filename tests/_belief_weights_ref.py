"""The weighted tracker of include/pmx.h ("Belief weights") restated in numpy on integer cell grids [n, H (y), W (x)]: neighbour sums
are padded shifts of the whole grid, with no row words, spans or shuffles.  The sets, the readings and the sight test come from
tests/_belief_ref.py and are not restated.  tests/test_belief_weights_cpu.py holds this model to the golden trajectories; the GPU
tests compare pmx_belief_weights_update / _init with it word for word.  The knobs floor / mover_offset exist for the negative
controls only."""
import numpy as np

import _belief_ref as B

RESPAWN_SHIFT = 7
LEVELS = 16
RECIP = np.array([0, 65536, 32768, 21845, 16384, 13107], np.int64)        # R[d] = floor(65536 / d)


def _neighbours(g):
    """[n, H, W] -> the sum of each cell's four neighbours, cells outside the board counting 0"""
    p = np.pad(g, ((0, 0), (1, 1), (1, 1)))
    return p[:, :-2, 1:-1] + p[:, 2:, 1:-1] + p[:, 1:-1, :-2] + p[:, 1:-1, 2:]


def degree(og):
    """deg(n) = 1 + the open 4-neighbours of n: the legal actions there, Stop included"""
    return 1 + _neighbours(og.astype(np.int64))


def bit_length(m):
    m = np.asarray(m, np.int64)
    return sum(((m >> i) > 0).astype(np.int64) for i in range(40))


def levels_of(w):
    """weights [n, 2 slots, 2 enemies, H, W] -> levels [n, 2, H, W]"""
    return np.where(w == 0, 0, 1 + (w >> 12)).max(2)


def _one_hot(n, H, W, xy, value=65535):
    g = np.zeros((n, H, W), np.int64)
    g[np.arange(n), xy[:, 1], xy[:, 0]] = value
    return g


def init(kind, open_g, starts, H, W):
    """pmx_belief_weights_init -> (set words [n, 2, 2, 32], weights [n, 2, 2, H, W], levels [n, 2, H, W])"""
    words = B.init(kind, open_g, starts)
    w = np.where(B.unpack(words)[..., :H, :W], 65535, 0).astype(np.int64)
    return words, w, levels_of(w)


def update(prev_w, prev_words, P, red, sight, ticks, seed, env, open_g, starts, H, W, reset=None, floor=True, mover_offset=3, bounds=None):
    """pmx_belief_weights_update.  prev_w [n, 2, 2, H, W] int64, prev_words [n, 2, 2, 32]; the other arguments as _belief_ref.update.
    -> (weights, levels, words, readings, seen).  bounds (a dict): the largest product, t, T and u met are recorded in it."""
    n = len(prev_w)
    ar = np.arange(n)
    words, sonar, seen = B.update(prev_words, P, red, sight, ticks, seed, env, open_g, starts, reset=reset)
    sets = B.unpack(words)[..., :H, :W]
    og = np.asarray(open_g)[:, :H, :W]
    recip = RECIP[degree(og)]
    first = np.where(np.asarray(red).astype(bool), 0, 1)
    starts = np.asarray(starts).astype(np.int64)
    out = np.zeros((n, 2, 2, H, W), np.int64)
    lo = 1 if floor else 0
    for k in range(2):
        e_k = (1 - first) + 2 * k
        q = np.asarray(prev_w)[:, 1, k].astype(np.int64)
        for j in range(2):
            a_j = first + 2 * j
            moved = e_k == (a_j + mover_offset) % 4
            prod = q * recip
            v = np.where(og, prod >> 16, 0)
            t = np.where(moved[:, None, None], np.where(og, v + _neighbours(v), 0), q)
            T = t.sum((1, 2))
            tr = t + _one_hot(n, H, W, starts[ar, e_k], 1) * (1 + (T >> RESPAWN_SHIFT))[:, None, None]
            S = sets[:, j, k]
            u = np.where(S, np.maximum(tr, lo), 0)
            b = bit_length(u.max((1, 2)))[:, None, None]
            hidden = np.where(b > 16, np.where(S, np.maximum(u >> np.maximum(b - 16, 0), lo), 0), u << np.maximum(16 - b, 0))
            q = np.where(seen[:, j, k, None, None], _one_hot(n, H, W, np.asarray(P)[ar, j, e_k].astype(np.int64)), hidden)
            out[:, j, k] = q
            if bounds is not None:
                for name, val in (("product", prod.max()), ("t", t.max()), ("T", T.max()), ("u", u.max())):
                    bounds[name] = max(bounds.get(name, 0), int(val))
        if reset is not None:
            rs = np.asarray(reset).astype(bool)
            out[rs, :, k] = _one_hot(n, H, W, starts[ar, e_k])[rs, None]
    return out, levels_of(out), words, sonar, seen
