"""The belief tracker of include/pmx.h ("Belief sets") restated in numpy, on boolean cell grids [n, 32 (y), 32 (x)] instead of the
kernel's row words and spans: the model tests/test_belief_cpu.py checks against the reference's sonar readings and the golden
trajectories, and the model the GPU tests compare pmx_belief_update / pmx_belief_init with, word for word.  Vectorised over n envs;
the knobs rule3 / mover_offset / half_width exist for the negative controls only."""
import numpy as np

SALT_SONAR = 0x534F4E41
M32 = np.uint64(0xFFFFFFFF)
_Y, _X = np.mgrid[0:32, 0:32]


def draw(seed, env, ticks, agent, salt):
    """h(salt) of include/pmx.h: lowbias32(seed ^ env * 0x9E3779B1 ^ ticks * 0x85EBCA77 ^ agent * 0xC2B2AE3D ^ salt), arrays broadcast"""
    u = lambda v: np.asarray(v).astype(np.uint64)
    x = (u(seed) ^ (u(env) * np.uint64(0x9E3779B1)) ^ (u(ticks) * np.uint64(0x85EBCA77)) ^ (u(agent) * np.uint64(0xC2B2AE3D)) ^ u(salt)) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def noise(seed, env, ticks, agent):
    """n of the sonar reading, -6 .. 6"""
    return ((draw(seed, env, ticks, agent, SALT_SONAR) * np.uint64(13)) >> np.uint64(32)).astype(np.int64) - 6


def unpack(words):
    """row words [..., 32] -> cells [..., 32, 32] (y, x)"""
    return ((np.asarray(words).astype(np.uint64)[..., None] >> np.arange(32, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def pack(cells):
    return (cells.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def open_cells(wall_rows, W, H):
    """walls [..., H] uint32 -> open cells [..., 32, 32]"""
    g = np.zeros(np.shape(wall_rows)[:-1] + (32, 32), bool)
    g[..., :H, :W] = ~unpack(wall_rows)[..., :W]
    return g


def dist_to(p):
    """Manhattan distance of every cell to p [n, 2] -> [n, 32, 32]"""
    p = np.asarray(p).astype(np.int64)
    return np.abs(_X[None] - p[:, 0, None, None]) + np.abs(_Y[None] - p[:, 1, None, None])


def one_cell(p):
    return dist_to(p) == 0


def manhattan(a, b):
    return np.abs(np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)).sum(-1)


def annulus(p, r, half_width=6):
    """the cells c with |manhattan(p, c) - r| <= half_width"""
    return np.abs(dist_to(p) - np.asarray(r).astype(np.int64)[:, None, None]) <= half_width


def init(kind, open_g, starts):
    """pmx_belief_init -> words [n, 2, 2, 32]; starts [n, 4, 2]"""
    n = len(open_g)
    out = np.zeros((n, 2, 2, 32), np.uint32)
    for k in range(2):
        g = open_g if kind else one_cell(starts[:, 2 * k]) | one_cell(starts[:, 2 * k + 1])
        out[:, :, k] = pack(g)[:, None]
    return out


def _dilate(S):
    d = S.copy()
    d[:, :, 1:] |= S[:, :, :-1]
    d[:, :, :-1] |= S[:, :, 1:]
    d[:, 1:] |= S[:, :-1]
    d[:, :-1] |= S[:, 1:]
    return d


def update(prev, P, red, sight, ticks, seed, env, open_g, starts, reset=None, rule3=True, mover_offset=3, half_width=6):
    """pmx_belief_update.  prev [n, 2, 2, 32] words; P [n, 2 slots, 4 agents, 2]: the positions in the snapshot each learner slot is
    encoded from; red [n] bool; ticks [n] the env's tick counter at the call; env [n] env indices; open_g [n, 32, 32]; starts
    [n, 4, 2]; reset [n] bool.  -> (words [n, 2, 2, 32], readings [n, 2, 2], seen [n, 2, 2])"""
    n = len(prev)
    ar = np.arange(n)
    red = np.asarray(red).astype(bool)
    first = np.where(red, 0, 1)
    second = first + 2
    sight = np.broadcast_to(np.asarray(sight), (n,))                 # (a value per env is accepted too)
    out = np.zeros((n, 2, 2, 32), np.uint32)
    sonar = np.zeros((n, 2, 2), np.int64)
    seen_out = np.zeros((n, 2, 2), bool)
    for k in range(2):
        e_k = (1 - first) + 2 * k
        S = unpack(prev[:, 1, k])
        for j in range(2):
            a_j = first + 2 * j
            Pj = np.asarray(P)[:, j].astype(np.int64)
            pa, pe, pf, ps = Pj[ar, a_j], Pj[ar, e_k], Pj[ar, first], Pj[ar, second]
            moved = e_k == (a_j + mover_offset) % 4
            S = np.where(moved[:, None, None], _dilate(S) & open_g, S)
            if rule3:
                S = S | one_cell(np.asarray(starts)[ar, e_k])
            r = manhattan(pa, pe) + noise(seed, env, ticks, 4 * a_j + e_k)
            seen = np.minimum(manhattan(pe, pf), manhattan(pe, ps)) <= sight
            hidden = S & (dist_to(pf) > sight[:, None, None]) & (dist_to(ps) > sight[:, None, None]) & annulus(pa, r, half_width)
            S = np.where(seen[:, None, None], one_cell(pe), hidden)
            out[:, j, k] = pack(S)
            sonar[:, j, k] = r
            seen_out[:, j, k] = seen
        if reset is not None:
            rs = np.asarray(reset).astype(bool)
            out[rs, :, k] = pack(one_cell(np.asarray(starts)[ar, e_k]))[rs, None]
    if reset is not None:
        sonar[np.asarray(reset).astype(bool)] = 0
    return out, sonar, seen_out
