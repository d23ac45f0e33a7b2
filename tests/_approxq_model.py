"""Plain Python restatement of what the in-kernel bots compute (action codes -2 .. -6 of include/pmx.h), for the tests.

It is pinned by the reference's own numbers (fixture G10, tests/test_approxq_cpu.py) and is then what the GPU tests compare
the kernels with.  Successors (the reflex roles and the walk home need real ones) come from the CPU checker's sub-step,
maze distances from its distance matrix; the features, the float64 Q sum, the best set, the three draws and the picks are
restated here:

    h(salt) = lowbias32(seed ^ env * 0x9E3779B1 ^ ticks * 0x85EBCA77 ^ agent * 0xC2B2AE3D ^ salt)
    explore iff h(0xA511E9B3) < 0x1999999A; exploring plays the floor(h(0) * n / 2^32)-th legal action, otherwise the
    floor(h(0x5bd1e995) * m / 2^32)-th best action (lists in the order N, S, E, W, Stop)
"""
import ctypes as C

import numpy as np

from oracle import oracle

RANDOM, BASE_OFF, BASE_DEF, AQ_OFF, AQ_DEF = -2, -3, -4, -5, -6
FLAG_HOME, FLAG_EXPLORED = 1, 2
ORDER = (0, 2, 1, 3, 4)                      # N, S, E, W, Stop as action codes
VEC = ((0, 1), (1, 0), (0, -1), (-1, 0), (0, 0))
REV = (2, 3, 0, 1, 4)
SALT_BEST, SALT_EXPLORE = 0x5bd1e995, 0xA511E9B3
W_CLOSEST, W_BIAS, W_GHOSTS, W_EATS = -3.099192562140742, -9.280875042529367, -16.6612110039328, 11.127808437648863
M32 = 0xFFFFFFFF

# pmx_state and the checker's packed state as numpy records (field for field the two ctypes structures)
_HEAD = [("pos", np.int8, (4, 2)), ("dir", np.int8, 4), ("pac", np.uint8, 4), ("scared", np.uint8, 4)]
_TAIL = [("food", np.uint32, 32), ("caps", np.uint32, 32), ("score", np.int32), ("steps", np.int32), ("ticks", np.uint32)]
STATE = np.dtype(_HEAD + [("carry", np.uint16, 4), ("ret", np.uint16, 4)] + _TAIL)
PSTATE = np.dtype(_HEAD + [("carry", np.uint8, 4), ("ret", np.uint8, 4)] + _TAIL)
assert STATE.itemsize == 304 and PSTATE.itemsize == C.sizeof(oracle.PState)


def lowbias32(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def h(seed, env, ticks, agent, salt):
    key = (int(seed) & M32) ^ ((int(env) * 0x9E3779B1) & M32)
    return lowbias32(key ^ ((int(ticks) * 0x85EBCA77) & M32) ^ ((int(agent) * 0xC2B2AE3D) & M32) ^ salt)


def pick(mask, x):
    """floor(x * n / 2^32)-th set action of mask in list order."""
    lst = [a for a in ORDER if (mask >> a) & 1]
    return lst[(x * len(lst)) >> 32]


def states_from_arrays(pos, dir, pac, scared, carry, ret, food, caps, score, steps, ticks=None):
    """Fixture columns (in_* of a golden file) -> STATE records."""
    n = len(pos)
    s = np.zeros(n, STATE)
    s["pos"], s["dir"], s["pac"], s["scared"], s["carry"], s["ret"] = pos, dir, pac, scared, carry, ret
    H = food.shape[1]
    s["food"][:, :H], s["caps"][:, :H] = food, caps
    s["score"], s["steps"] = score, steps
    if ticks is not None:
        s["ticks"] = ticks
    return s


def to_pstates(states):
    p = np.zeros(len(states), PSTATE)
    for k in PSTATE.names:
        p[k] = states[k]
    return p


class Model:
    def __init__(self, rows):
        self.env = oracle.Env(rows)
        self.W, self.H, self.walls, _, _, self.starts = oracle.parse_layout_text(rows)
        cells, dist = oracle.maze_distances(rows)
        self.index = {(int(x), int(y)): k for k, (x, y) in enumerate(cells)}
        self.dist = dist.astype(np.int64)
        self.cell = np.full((32, 32), -1, np.int64)                 # [y][x] -> row of the distance matrix
        for (x, y), k in self.index.items():
            self.cell[y, x] = k
        half = self.W // 2
        self.lo = (1 << half) - 1
        self.hi = ((1 << self.W) - 1) & ~self.lo
        self._p = oracle.PState()

    # -- pieces -------------------------------------------------------------------------------------------------
    def open(self, x, y):
        return not (int(self.walls[y]) >> x) & 1

    def legal_mask(self, st, i):
        x, y = int(st["pos"][i][0]), int(st["pos"][i][1])
        return sum(1 << a for a, (dx, dy) in enumerate(VEC) if self.open(x + dx, y + dy))

    def prey(self, st, i):
        """Pellets agent i may eat: (x, y) on the other side."""
        mask = self.hi if i % 2 == 0 else self.lo
        out = []
        for y in range(self.H):
            r = int(st["food"][y]) & mask
            while r:
                low = r & -r
                out.append((low.bit_length() - 1, y))
                r ^= low
        return out

    def maze(self, a, b):
        return int(self.dist[self.index[a], self.index[b]])

    def successor(self, pst, i, a):
        """generateSuccessor of the packed state for mover i -> PSTATE record."""
        C.memmove(C.byref(self._p), pst.tobytes(), PSTATE.itemsize)
        self.env.set_state(self._p)
        self.env.substep(i, a)
        return np.frombuffer(bytes(self.env.get_state()), PSTATE)[0]

    def home_action(self, pst, i, legal):
        start = (int(self.starts[i][0]), int(self.starts[i][1]))
        best, act = 9999, -1
        for a in ORDER:
            if (legal >> a) & 1:
                nx = self.successor(pst, i, a)
                d = self.maze(start, (int(nx["pos"][i][0]), int(nx["pos"][i][1])))
                if d < best:
                    best, act = d, a
        return act

    def q_features(self, st, i, a, prey=None):
        """(g, eats, d or None) of ApproxQLearningOffense for action a; prey: self.prey(st, i) if the caller has it."""
        x, y = int(st["pos"][i][0]) + VEC[a][0], int(st["pos"][i][1]) + VEC[a][1]
        g = 0
        for o in ((1, 3) if i % 2 == 0 else (0, 2)):
            if not st["pac"][o]:
                g += abs(int(st["pos"][o][0]) - x) + abs(int(st["pos"][o][1]) - y) <= 1
        if prey is None:
            prey = self.prey(st, i)
        eats = g == 0 and (x, y) in prey
        d = 255
        if prey:
            rows = self.cell[[p[1] for p in prey], [p[0] for p in prey]]
            d = int(self.dist[self.cell[y, x], rows].min())
        return g, eats, (None if d == 255 else d)

    def q_value(self, g, eats, d):
        q = 0
        q += (1.0 / 10.0) * W_BIAS
        q += (g / 10.0) * W_GHOSTS
        if eats:
            q += (1.0 / 10.0) * W_EATS
        if d is not None:
            q += ((float(d) / (self.W * self.H)) / 10.0) * W_CLOSEST
        return q

    def reflex_value(self, st, nx, i, a, defensive):
        me = (int(nx["pos"][i][0]), int(nx["pos"][i][1]))
        if not defensive:
            prey = self.prey(nx, i)
            return -100 * len(prey) - (min(self.maze(me, p) for p in prey) if prey else 0)
        val, gap = (0 if nx["pac"][i] else 100), None
        for o in ((1, 3) if i % 2 == 0 else (0, 2)):
            if nx["pac"][o]:
                val -= 1000
                d = self.maze(me, (int(nx["pos"][o][0]), int(nx["pos"][o][1])))
                gap = d if gap is None else min(gap, d)
        if gap is not None:
            val -= 10 * gap
        return val - (100 if a == 4 else 0) - (2 if a == REV[int(st["dir"][i])] else 0)

    # -- the bots -----------------------------------------------------------------------------------------------
    def evaluate(self, st, i, code, pst=None):
        """-> dict(legal, values [5] float64 (NaN where illegal), best mask, food_left, home action or -1, and for the
        offensive approx-Q role g / eats / d per action (-1 where illegal or absent))."""
        if pst is None:
            pst = to_pstates(st.reshape(1))[0]
        legal = self.legal_mask(st, i)
        values = np.full(5, np.nan)
        prey = self.prey(st, i)
        out = dict(legal=legal, values=values, food_left=len(prey), home=-1,
                   g=np.full(5, -1), eats=np.full(5, -1), d=np.full(5, -1))
        for a in ORDER:
            if not (legal >> a) & 1:
                continue
            if code == RANDOM:
                values[a] = 0.0
            elif code == AQ_OFF:
                g, eats, d = self.q_features(st, i, a, prey)
                values[a] = self.q_value(g, eats, d)
                out["g"][a], out["eats"][a], out["d"][a] = g, int(eats), (-1 if d is None else d)
            else:
                values[a] = float(self.reflex_value(st, self.successor(pst, i, a), i, a, code in (BASE_DEF, AQ_DEF)))
        top = np.nanmax(values)
        out["best"] = sum(1 << a for a in range(5) if values[a] == top)
        home_at = {RANDOM: -1, BASE_OFF: 0, BASE_DEF: 0, AQ_OFF: 2, AQ_DEF: 2}[code]
        if out["food_left"] <= home_at:
            out["home"] = self.home_action(pst, i, legal)
        return out

    @staticmethod
    def play(ev, code, seed, env, ticks, agent):
        """The action and flags the bot plays given its evaluation (a dict with legal / best / home)."""
        if code == RANDOM:
            return pick(ev["legal"], h(seed, env, ticks, agent, 0)), 0
        if ev["home"] >= 0:
            return int(ev["home"]), FLAG_HOME
        if code == AQ_OFF and h(seed, env, ticks, agent, SALT_EXPLORE) < 0x1999999A:
            return pick(ev["legal"], h(seed, env, ticks, agent, 0)), FLAG_EXPLORED
        return pick(int(ev["best"]), h(seed, env, ticks, agent, SALT_BEST)), 0

    def decide(self, st, i, code, seed, env, pst=None):
        ev = self.evaluate(st, i, code, pst)
        act, flags = self.play(ev, code, seed, env, int(st["ticks"]), i)
        return ev, act, flags
