"""Plain-Python model of the episode statistics (include/pmx.h, "Episode statistics"), on named per-agent fields.

The model never sees a packed word while it counts: a state is positions, isPacman flags, scared timers, carried and returned
pellets, a set of capsule cells and the score.  Only `Record.words()` packs, to compare a record with the kernel's word for word.
Test infrastructure: shared by test_episode_stats_cpu.py (fixtures, oracle-stepped states) and test_gpu_episode_stats.py."""
import numpy as np

NAMES = ("eaten", "returned", "lost", "deaths", "kills", "capsules", "pacman_steps", "stops")
WORDS = 48
ACTION_VECTORS = {0: (0, 1), 1: (1, 0), 2: (0, -1), 3: (-1, 0), 4: (0, 0)}      # 0 N, 1 E, 2 S, 3 W, 4 Stop


class State:
    """One game state on named fields; caps is a frozenset of (x, y)."""

    def __init__(self, pos, dir, pac, scared, carry, ret, caps, score):
        self.pos = [(int(p[0]), int(p[1])) for p in pos]
        self.dir = [int(v) for v in dir]
        self.pac = [int(v) for v in pac]
        self.scared = [int(v) for v in scared]
        self.carry = [int(v) for v in carry]
        self.ret = [int(v) for v in ret]
        self.caps = frozenset(caps)
        self.score = int(score)


def caps_cells(rows):
    """capsule bit rows (bit x of row y) -> [(x, y)] in the row-major order the handle fills its four slots in"""
    return [(x, y) for y, r in enumerate(rows) for x in range(32) if (int(r) >> x) & 1]


def state_of(p):
    """a packed exchange state (pmx State / oracle PState, ctypes) -> State"""
    return State([(p.pos[i][0], p.pos[i][1]) for i in range(4)], p.dir, p.pac, p.scared, p.carry, p.ret, caps_cells(p.caps), p.score)


def fixture_state(d, t=None, s=None):
    """sub-step s of tick t of a traj_*.npz fixture, or its initial state (t None) -> State"""
    if t is None:
        g = lambda k: d["init_" + k]
    else:
        g = lambda k: d["sub_" + k][t, s]
    return State(g("pos"), g("dir"), g("pac"), g("scared"), g("carry"), g("ret"), caps_cells(g("caps")), g("score"))


def dist(a, b):
    return abs(a[0] - b[0]) + abs(a[1] - b[1])


def nonmover_died(X, Y, i, position_rule=True):
    return ((position_rule and Y.pos[i] != X.pos[i]) or (X.scared[i] > 0 and Y.scared[i] == 0) or Y.carry[i] < X.carry[i])


def mover_died(X, Y, m):
    return (dist(Y.pos[m], X.pos[m]) > 1 or (Y.carry[m] < X.carry[m] and Y.ret[m] == X.ret[m])
            or (X.scared[m] >= 2 and Y.scared[m] == 0))


class Record:
    """The record of one env.  position_rule / lost_from are the negative controls' knobs: the table has True and "X"."""

    def __init__(self, state, position_rule=True, lost_from="X"):
        self.c = {n: [0, 0, 0, 0] for n in NAMES}
        self.ticks, self.done = 0, 0
        self.score = state.score
        self.last = state
        self.slots = (caps_cells_sorted(state.caps) + [None] * 4)[:4]          # a slot keeps its cell until it is eaten
        self.position_rule, self.lost_from = position_rule, lost_from
        self.mover_deaths = self.nonmover_deaths = self.pacman_deaths = 0      # (bookkeeping for the tests, not part of the record)

    def transition(self, X, Y, m):
        c = self.c
        kills = 0
        for i in range(4):
            if i != m and nonmover_died(X, Y, i, self.position_rule):
                c["deaths"][i] += 1
                c["lost"][i] += (X if self.lost_from == "X" else Y).carry[i]
                kills += 1
                self.nonmover_deaths += 1
                self.pacman_deaths += X.pac[i]
        died = mover_died(X, Y, m)
        if died:
            c["deaths"][m] += 1
            c["lost"][m] += (X if self.lost_from == "X" else Y).carry[m]
            self.mover_deaths += 1
            self.pacman_deaths += X.pac[m]
        c["kills"][m] += kills
        c["eaten"][m] += max(0, Y.carry[m] - X.carry[m])
        c["returned"][m] += Y.ret[m] - X.ret[m]
        c["capsules"][m] += len(X.caps) - len(Y.caps)
        c["pacman_steps"][m] += Y.pac[m]
        c["stops"][m] += int(not died and Y.pos[m] == X.pos[m])

    def tick(self, subs, done):
        """subs: the four states after sub-steps 0 .. 3 of one tick (the last is the state after the tick)"""
        if self.done:
            return
        X = self.last
        for m in range(4):
            self.transition(X, subs[m], m)
            X = subs[m]
        self.ticks += 1
        self.score = X.score
        self.last = X
        self.done = int(bool(done))

    def words(self):
        """the 48 int32 words of include/pmx.h"""
        w = np.zeros(WORDS, np.int64)
        for k, n in enumerate(NAMES):
            for i in range(4):
                w[8 * i + k] = self.c[n][i]
        w[32], w[33], w[34] = self.ticks, self.score, self.done
        s = self.last
        for i in range(4):
            w[36 + i] = s.pos[i][0] | s.pos[i][1] << 8 | s.dir[i] << 16 | s.pac[i] << 24
            w[40 + i] = s.scared[i] | s.carry[i] << 8 | s.ret[i] << 20
        slot = [(c[0] | c[1] << 8) if c is not None and c in s.caps else 0xFFFF for c in self.slots]
        w[44], w[45] = slot[0] | slot[1] << 16, slot[2] | slot[3] << 16
        return w.astype(np.uint32).view(np.int32)


def caps_cells_sorted(caps):
    return sorted(caps, key=lambda c: (c[1], c[0]))


def fixture_episodes(d, **knobs):
    """Every FINISHED episode of a traj_*.npz fixture -> [(Record, last tick index)] (the fixture resets after a done)"""
    out = []
    rec = Record(fixture_state(d), **knobs)
    for t in range(len(d["done"])):
        rec.tick([fixture_state(d, t, s) for s in range(4)], d["done"][t])
        if d["done"][t]:
            out.append((rec, t))
            rec = Record(fixture_state(d), **knobs)
    return out


def invariants(rec, sub_ret, sub_score):
    """the three invariants of a finished episode -> list of the broken ones"""
    c, s = rec.c, rec.last
    bad = []
    if any(c["eaten"][i] - c["returned"][i] - c["lost"][i] != s.carry[i] for i in range(4)):
        bad.append("eaten - returned - lost == carry")
    if any(c["returned"][i] != int(sub_ret[i]) for i in range(4)):
        bad.append("returned == sub_ret")
    if c["returned"][0] + c["returned"][2] - c["returned"][1] - c["returned"][3] != int(sub_score):
        bad.append("red returns - blue returns == score")
    return bad


# ---- hand-set states (the gaps of the fixtures), on a board of their own -------------------------------------------------
# red (agents 0, 2) defends x < 6, blue (1, 3) x >= 6; a capsule on each half; starts in the corners
SCENARIO_ROWS = ("%%%%%%%%%%%%",
                 "%3   ..   2%",
                 "%    ..    %",
                 "%  o .. o  %",
                 "%    ..    %",
                 "%1   ..   4%",
                 "%%%%%%%%%%%%")
_STARTS = [(1, 1), (10, 5), (1, 5), (10, 1)]


def _scn(name, actions, expect, **over):
    f = dict(pos=list(_STARTS), dir=[4] * 4, pac=[0] * 4, scared=[0] * 4, carry=[0] * 4, ret=[0] * 4)
    for k, v in over.items():
        for i, x in v.items():
            f[k][i] = x
    return dict(name=name, actions=actions, expect=expect, **f)


# expect: {(counter, agent): value} after ONE tick; every counter not named in it except pacman_steps and stops must be 0
SCENARIOS = [
    # the scared disjunct alone: agent 0 is eaten ON its own start, so neither its cell nor its (empty) carry changes
    _scn("scared_ghost_on_start_eaten", [4, 3, 4, 4], {("deaths", 0): 1, ("kills", 1): 1},
         pos={1: (2, 1)}, pac={1: 1}, scared={0: 10}),
    # the action is applied before checkDeath: the pellet is eaten and dumped with the two carried ones
    _scn("eat_and_die", [4, 1, 4, 4], {("deaths", 1): 1, ("lost", 1): 2},
         pos={0: (5, 3), 1: (4, 3)}, pac={1: 1}, carry={1: 2}),
    _scn("one_move_two_kills", [1, 4, 4, 4], {("deaths", 1): 1, ("deaths", 3): 1, ("kills", 0): 2, ("lost", 1): 1, ("lost", 3): 2},
         pos={0: (1, 2), 1: (2, 2), 3: (2, 2)}, pac={1: 1, 3: 1}, carry={1: 1, 3: 2}),
    _scn("capsule", [4, 1, 4, 4], {("capsules", 1): 1},
         pos={1: (2, 3)}, pac={1: 1}),
    # the mover's scared disjunct alone: two ticks of fear left, it steps onto the invader on its own start and is eaten there
    # (in both, the invader then stands on a ghost that is no longer scared and dies on its own Stop: a mover's death, nobody's kill)
    _scn("scared_mover_dies_on_start", [3, 4, 4, 4], {("deaths", 0): 1, ("deaths", 1): 1},
         pos={0: (2, 1), 1: (1, 1)}, pac={1: 1}, scared={0: 2}),
    # the blind spot of the header: the same with ONE tick of fear left is counted as a move
    _scn("blind_spot", [3, 4, 4, 4], {("deaths", 1): 1},
         pos={0: (2, 1), 1: (1, 1)}, pac={1: 1}, scared={0: 1}),
]


def scenario_layout():
    """(food rows, capsule rows) of SCENARIO_ROWS, bottom-up"""
    H = len(SCENARIO_ROWS)
    food, caps = np.zeros(H, np.uint32), np.zeros(H, np.uint32)
    for y in range(H):
        for x, ch in enumerate(SCENARIO_ROWS[H - 1 - y]):
            if ch == ".":
                food[y] |= np.uint32(1 << x)
            elif ch == "o":
                caps[y] |= np.uint32(1 << x)
    return food, caps


def check_expect(rec, expect):
    for n in NAMES:
        if n in ("pacman_steps", "stops"):
            continue
        for i in range(4):
            assert rec.c[n][i] == expect.get((n, i), 0), (n, i, rec.c[n][i], expect.get((n, i), 0))
