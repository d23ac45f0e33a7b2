"""Mid-game states and action streams for differential tests of the tick (a helper, not a test file).

A game that starts from the start position and plays uniformly random actions for twenty ticks never leaves home on a real
board: nothing is eaten, no capsule, no scared ghost, no death, no score, no win.  What is here starts the envs in the middle
of a game instead:

* random_states: the recipe of tests/golden/make_golden.py::random_states (with_caps=True), restated on numpy and the oracle's
  layout parser alone -- food density modes, one side cleared, 0-3 capsules biased to the border columns, agents clustered
  around a random cell, scared / carry / returned distributions, a score.  With the recipe's own step draw (recipe_steps=True)
  it reproduces the inputs of the scen_*_random fixtures, which tests/test_midgame_states_cpu.py checks;
* fixture_states: the reference-made states of a scen_*_random fixture, cycled, as test_gpu_parity._seed_states loads them;
  both leave every fifth env on the start position and cap the step counter at 250, so a length-300 game does not time out
  within a short run;
* mixed_actions: the action mix of test_gpu_parity.test_differential_vs_oracle;
* oracle_run: the oracle's record of a run (every output of every tick, the packed states at every tick) and count_events,
  which says from the oracle's states alone what the rules did in it.
"""
import ctypes as C
import functools

import numpy as np

import _golden as G
from oracle import oracle as O

T = 20
LENGTH = 300
MAX_STEPS = 250
JUNK_CODES = (-1, 5, 7, 127, -128)
ACTION_RANDOM_LEGAL = -2          # include/pmx.h PMX_ACTION_RANDOM_LEGAL

# the oracle's packed state as a numpy record (oracle.PState)
PSTATE_DTYPE = np.dtype([("pos", "i1", (4, 2)), ("dir", "i1", 4), ("pac", "u1", 4), ("scared", "u1", 4), ("carry", "u1", 4),
                         ("ret", "u1", 4), ("food", "<u4", O.MAXD), ("caps", "<u4", O.MAXD), ("score", "<i4"), ("steps", "<i4"),
                         ("ticks", "<u4")])
assert PSTATE_DTYPE.itemsize == C.sizeof(O.PState)
STATE_FIELDS = ("pos", "dir", "pac", "scared", "carry", "ret", "food", "caps", "score", "steps", "ticks")

# board name -> where its rows and its states come from
FIXTURES = {"smallCapture": "scen_small_random.npz", "tinyCapture": "scen_tiny_random.npz", "bloxCapture": "scen_blox_random.npz",
            "maze23": "scen_maze23_random.npz"}
NO_CAPSULES = ("bloxCapture",)    # scen_blox_random was made with with_caps=False and the board has none
MAZE_SEED, STATE_SEED, ACTION_SEED = 11, 21, 5


@functools.lru_cache(maxsize=None)
def board_rows(board):
    """text rows (top first) of a fixture board or of "mazeWxH" (maze_generator seed 11, as the other fused-tick tests)"""
    if board in FIXTURES:
        return tuple(G.load(FIXTURES[board])[1]["layout"])
    from pmx import maze_generator as MG
    w, h = (int(v) for v in board[4:].split("x"))
    rows = tuple(MG.generate_maze(MAZE_SEED, rows=h - 2, cols=(w - 2) // 2).split("\n"))
    assert (len(rows[0]), len(rows)) == (w, h)
    return rows


def _bit(x):
    return np.uint32(1 << x)


def _clear(x):
    return np.uint32(~(1 << x) & 0xFFFFFFFF)


def random_states(rows, n, seed, recipe_steps=False):
    """n oracle.PState drawn as make_golden.random_states(lay, n, seed, with_caps=True) draws them (same generator, same order
    of draws).  The step counter is the recipe's (0 .. 301) capped at MAX_STEPS unless recipe_steps."""
    rng = np.random.RandomState(seed)
    W, H, walls, _, _, _ = O.parse_layout_text(list(rows))
    base = O.Env(list(rows)).get_state()                       # the start position: ghosts on their starts, direction Stop
    open_cells = [(x, y) for x in range(W) for y in range(H) if not (int(walls[y]) >> x) & 1]
    half = int(W / 2)
    states = []
    for k in range(n):
        steps = int(rng.choice([0, 5, 299, 300, 301])) if rng.rand() < 0.1 else int(rng.randint(0, 300))
        # food: a random subset of the open cells, dense or sparse, sometimes none on one side (a win by the food threshold)
        p = [0.5, 0.15, 0.03, 0.9, 0.3][rng.randint(5)]
        food = np.zeros(H, np.uint32)
        for (x, y) in open_cells:
            if rng.rand() < p:
                food[y] |= _bit(x)
        if rng.rand() < 0.15:
            mask = (1 << half) - 1
            if rng.rand() < 0.5:
                food &= np.uint32(mask)
            else:
                food &= np.uint32(~mask & 0xFFFFFFFF)
        caps = np.zeros(H, np.uint32)
        for _ in range(rng.randint(0, 4)):
            x, y = open_cells[rng.randint(len(open_cells))]
            if rng.rand() < 0.3:                               # on or next to the border column
                x = half + int(rng.randint(-1, 2))
                if (int(walls[y]) >> x) & 1:
                    continue
            caps[y] |= _bit(x)
            food[y] &= _clear(x)
        # agents: clustered, so that collisions are common
        pos = [(base.pos[i][0], base.pos[i][1]) for i in range(4)]
        dirs = [base.dir[i] for i in range(4)]
        cx, cy = open_cells[rng.randint(len(open_cells))]
        for i in range(4):
            if rng.rand() < 0.15:
                continue                                       # stays on its start
            if rng.rand() < 0.7:
                near = [c for c in open_cells if abs(c[0] - cx) + abs(c[1] - cy) <= 2]
                x, y = near[rng.randint(len(near))]
            else:
                x, y = open_cells[rng.randint(len(open_cells))]
            pos[i] = (x, y)
            dirs[i] = int(rng.randint(5))
        pac = [(i in (0, 2)) != (pos[i][0] < W / 2) for i in range(4)]
        scared, carry, ret = [0] * 4, [0] * 4, [0] * 4
        for i in range(4):
            scared[i] = 0 if rng.rand() < 0.6 else int(rng.choice([1, 2, 39, 40, rng.randint(1, 41)]))
            carry[i] = 0 if rng.rand() < 0.4 else int(rng.choice([1, 2, 3, 7, 15, rng.randint(1, 20)]))
            ret[i] = int(rng.randint(0, 6))
            if not pac[i] and rng.rand() < 0.8:
                carry[i] = 0                                   # a ghost normally carries nothing; some odd ones are kept
        for i in range(4):                                     # a Pacman standing on food would have eaten it: usually cleared
            if rng.rand() < 0.7:
                food[pos[i][1]] &= _clear(pos[i][0])
        score = int(rng.randint(-8, 9))
        for _ in range(4):
            rng.randint(5)                                     # the recipe draws the scenario's four actions here
        s = O.PState()
        for i in range(4):
            s.pos[i][0], s.pos[i][1] = pos[i]
            s.dir[i], s.pac[i], s.scared[i], s.carry[i], s.ret[i] = dirs[i], int(pac[i]), scared[i], carry[i], ret[i]
        for y in range(H):
            s.food[y], s.caps[y] = int(food[y]), int(caps[y])
        s.score, s.steps = score, steps if recipe_steps else min(steps, MAX_STEPS)
        states.append(s)
    return states


def fixture_row_state(d, k, H, max_steps=MAX_STEPS):
    """row k of a scen_*.npz fixture's input states -> oracle.PState"""
    s = O.PState()
    for i in range(4):
        s.pos[i][0], s.pos[i][1] = int(d["in_pos"][k][i][0]), int(d["in_pos"][k][i][1])
        s.dir[i], s.pac[i], s.scared[i] = int(d["in_dir"][k][i]), int(d["in_pac"][k][i]), int(d["in_scared"][k][i])
        s.carry[i], s.ret[i] = int(d["in_carry"][k][i]), int(d["in_ret"][k][i])
    for y in range(H):
        s.food[y], s.caps[y] = int(d["in_food"][k][y]), int(d["in_caps"][k][y])
    s.score, s.steps = int(d["in_score"][k]), min(int(d["in_steps"][k]), max_steps)
    return s


def _copy(p):
    q = O.PState()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(O.PState))
    return q


def start_states(board, N):
    """the N states a run on `board` starts from: the fixture's rows cycled (fixture boards) or random_states (mazes); every
    fifth env keeps the start position"""
    rows = board_rows(board)
    H = len(rows)
    base = O.Env(list(rows)).get_state()
    if board in FIXTURES:
        d, _ = G.load(FIXTURES[board])
        K = len(d["actions"])
        seeded = [fixture_row_state(d, e % K, H) for e in range(N)]
    else:
        seeded = random_states(rows, N, STATE_SEED)
    return [_copy(base) if e % 5 == 4 else seeded[e] for e in range(N)]


def to_pmx_state(pmx, p, H):
    """oracle.PState -> the handle's exchange format (pmx.make_state)"""
    s = pmx.make_state([(p.pos[i][0], p.pos[i][1]) for i in range(4)], p.dir, p.pac, p.scared, p.carry, p.ret, p.food, p.caps,
                       p.score, p.steps, H)
    s.ticks = p.ticks
    return s


def load_states(pmx, env, states):
    """the same states into a handle that has been reset"""
    H = env.layout.height
    env.set_state([to_pmx_state(pmx, p, H) for p in states])


def pack_states(orc):
    """the packed state of every env of an oracle batch as one numpy record array [n]"""
    arr = (O.PState * orc.n)()
    for e in range(orc.n):
        orc.lib.orc_pack(orc.L.buf, C.byref(orc.S, e * orc.ssz), C.byref(arr[e]))
    return np.frombuffer(arr, dtype=PSTATE_DTYPE).copy()


def initial_legal(orc):
    return np.array([[orc.lib.orc_legal(orc.L.buf, C.byref(orc.S, e * orc.ssz), i) for i in range(4)] for e in range(orc.n)], np.uint8)


def mixed_actions(rng, legal, N):
    """one tick of test_differential_vs_oracle's mix: 70 % uniform over the legal moves of the masks `legal` [N, 4] (three
    redraws of an illegal one), the rest uniform over 0..4 whatever is legal; then 1 % one of the junk codes and 12 %
    PMX_ACTION_RANDOM_LEGAL, the draw the kernel makes itself"""
    a = rng.randint(0, 5, size=(N, 4)).astype(np.int8)
    pick = rng.rand(N, 4) < 0.7
    for _ in range(3):
        ill = pick & (((legal >> np.clip(a, 0, 4)) & 1) == 0)
        a[ill] = rng.randint(0, 5, size=int(ill.sum()))
    a[rng.rand(N, 4) < 0.01] = rng.choice(JUNK_CODES)
    a[rng.rand(N, 4) < 0.12] = ACTION_RANDOM_LEGAL
    return a


def _popcount(rows):
    return np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=-1).sum(-1).astype(np.int64)


def count_events(states, ticks, length):
    """What the rules did in a run, from the oracle alone.  states: the T + 1 record arrays of pack_states (before the first
    tick, after each tick); ticks: the T per-tick records of oracle_run; length: the env's length.

    Each figure is a lower bound read off states one tick apart, so what a tick does and undoes is not seen, and with
    auto_reset the state after a finishing tick is the fresh game, so board changes of such ticks are not counted:
      food      env-ticks in which an agent's carry right after its own sub-step (the tick's agent word) exceeds its carry
                before the tick
      capsule   env-ticks (not finishing) after which the board has fewer capsules
      dump      env-ticks (not finishing) after which a cell has food that had none before: a death put carried food back
      score     env-ticks with score_change != 0
      early     finishing env-ticks that began with fewer than length - 1 steps: not the timeout
      max_carry the largest carry in any state or agent word
      mixed     (tick, group of 64 envs) pairs in which between 1 and 63 envs finish
    plus, per tick, `finish_ticks` and `capsule_ticks`: whether any env finished / a capsule was seen eaten in that tick."""
    ev = dict(food=0, capsule=0, dump=0, score=0, early=0, max_carry=0, mixed=0, finish_ticks=[], capsule_ticks=[])
    for t, rec in enumerate(ticks):
        before, after = states[t], states[t + 1]
        done = rec["done"].astype(bool)
        live = ~done
        carry_own = (rec["agent"] >> 16).astype(np.int64)
        ev["food"] += int((carry_own > before["carry"]).any(1).sum())
        caps = (_popcount(after["caps"]) < _popcount(before["caps"])) & live
        ev["capsule"] += int(caps.sum())
        ev["dump"] += int((((after["food"] & ~before["food"]) != 0).any(1) & live).sum())
        ev["score"] += int((rec["score_change"] != 0).sum())
        ev["early"] += int((done & (before["steps"] < length - 1)).sum())
        ev["max_carry"] = max(ev["max_carry"], int(carry_own.max()), int(before["carry"].max()), int(after["carry"].max()))
        n = len(done)
        per_group = done[: n - n % 64].reshape(-1, 64).sum(1)
        ev["mixed"] += int(((per_group >= 1) & (per_group <= 63)).sum())
        ev["finish_ticks"].append(bool(done.any()))
        ev["capsule_ticks"].append(bool(caps.any()))
    return ev


class Run:
    """what oracle_run returns: rows, the start states, the T action arrays, the T per-tick records, the T + 1 packed states"""

    def __init__(self, rows, start, actions, ticks, states, length):
        self.rows, self.start, self.actions, self.ticks, self.states, self.length = rows, start, actions, ticks, states, length
        self.H, self.W = len(rows), len(rows[0])

    def events(self):
        return count_events(self.states, self.ticks, self.length)


@functools.lru_cache(maxsize=3)
def oracle_run(board, N, legal_reward=True, defence_reward=True, keep_obs=True):
    """T ticks of mixed_actions from start_states(board, N) through the oracle (length 300, auto_reset, seed 3): everything it
    returns at every tick (the planes as bytes: no element exceeds 1 + the board's pellets) and its packed states."""
    rows = list(board_rows(board))
    H, W = len(rows), len(rows[0])
    orc = O.BatchEnv(rows, N, length=LENGTH, legal_reward=legal_reward, defence_reward=defence_reward, auto_reset=True, seed=3)
    start = start_states(board, N)
    for e, p in enumerate(start):
        orc.set_state(e, p)
    rng = np.random.RandomState(ACTION_SEED)
    legal = initial_legal(orc)
    oobs = np.zeros((N, 4, 8, H, W), np.float32) if keep_obs else None
    actions, ticks, states = [], [], [pack_states(orc)]
    for t in range(T):
        a = mixed_actions(rng, legal, N)
        orc.tick(a, oobs)
        rec = dict(reward=orc.reward.tobytes(), done=orc.done.copy(), legal=orc.legal.copy(), score_change=orc.score_change.copy(),
                   score=orc.score.copy(), agent=orc.agent.copy())
        if keep_obs:
            assert oobs.max() <= 255 and (oobs == np.floor(oobs)).all()
            rec["obs"] = oobs.astype(np.uint8)
        actions.append(a)
        ticks.append(rec)
        states.append(pack_states(orc))
        legal = orc.legal.copy()
    return Run(tuple(rows), start, actions, ticks, states, LENGTH)
