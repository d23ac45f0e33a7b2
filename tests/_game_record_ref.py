"""Plain-numpy model of the game records (include/pmx.h, "Game records"): init and update over sequences of game states.

A state is a `Frame` on named fields (positions, directions, isPacman, timers, carried / returned pellets, capsule cells, food rows,
score); EVENT words are decided on those names, never on packed words.  Only `Log.words()` packs, to compare a log with the kernel's
word for word.  Test infrastructure: shared by test_game_record_cpu.py (fixtures, oracle-stepped states) and test_gpu_game_record.py."""
import numpy as np

HEAD_WORDS = 8
MOVE_OF = {(0, 1): 0, (1, 0): 1, (0, -1): 2, (-1, 0): 3, (0, 0): 4}     # 0 N, 1 E, 2 S, 3 W, 4 Stop
VECTORS = {v: k for k, v in MOVE_OF.items()}


class Frame:
    def __init__(self, pos, dir, pac, scared, carry, ret, caps_rows, food_rows, score, H):
        self.pos = [(int(p[0]), int(p[1])) for p in pos]
        self.dir = [int(v) for v in dir]
        self.pac = [int(v) for v in pac]
        self.scared = [int(v) for v in scared]
        self.carry = [int(v) for v in carry]
        self.ret = [int(v) for v in ret]
        self.caps = frozenset((x, y) for y in range(H) for x in range(32) if (int(caps_rows[y]) >> x) & 1)
        self.food = tuple(int(food_rows[y]) for y in range(H))
        self.score = int(score)

    def same_state(self, o):
        return (self.pos, self.dir, self.pac, self.scared, self.carry, self.ret, self.caps, self.food, self.score) == \
               (o.pos, o.dir, o.pac, o.scared, o.carry, o.ret, o.caps, o.food, o.score)


def frame_of(p, H):
    """a packed exchange state (pmx State / oracle PState, ctypes or a numpy record) -> Frame"""
    return Frame([(p.pos[i][0], p.pos[i][1]) for i in range(4)], p.dir, p.pac, p.scared, p.carry, p.ret, p.caps, p.food, p.score, H)


def frames_of_records(a, H):
    """a numpy record array of packed states (fields pos, dir, pac, scared, carry, ret, food, caps, score) -> [Frame]"""
    f = {k: a[k].tolist() for k in ("pos", "dir", "pac", "scared", "carry", "ret", "caps", "food", "score")}
    return [Frame(f["pos"][e], f["dir"][e], f["pac"][e], f["scared"][e], f["carry"][e], f["ret"][e], f["caps"][e], f["food"][e],
                  f["score"][e], H) for e in range(len(a))]


def fixture_frame(d, t=None, s=None):
    """sub-step s of tick t of a traj_*.npz fixture, or its initial state (t None) -> Frame"""
    g = (lambda k: d["init_" + k]) if t is None else (lambda k: d["sub_" + k][t, s])
    return Frame(g("pos"), g("dir"), g("pac"), g("scared"), g("carry"), g("ret"), g("caps"), g("food"), g("score"), len(d["init_food"]))


def dist(a, b):
    return abs(a[0] - b[0]) + abs(a[1] - b[1])


def died(X, Y, i, m):
    """the table of "Episode statistics": did agent i die in X -> Y, made by mover m"""
    if i != m:
        return Y.pos[i] != X.pos[i] or (X.scared[i] > 0 and Y.scared[i] == 0) or Y.carry[i] < X.carry[i]
    return dist(Y.pos[m], X.pos[m]) > 1 or (Y.carry[m] < X.carry[m] and Y.ret[m] == X.ret[m]) or (X.scared[m] >= 2 and Y.scared[m] == 0)


def death_candidates(X, m):
    """the moves d for which pos_X[m] + d is the cell of an enemy in X"""
    enemy = {X.pos[i] for i in range(4) if i % 2 != m % 2}
    return [k for v, k in MOVE_OF.items() if (X.pos[m][0] + v[0], X.pos[m][1] + v[1]) in enemy]


def event(X, Y, m):
    """EVENT of the sub-step X -> Y made by mover m, as named fields: (move, mover_died, victims, ate, capsule, returned); move 7 =
    undetermined"""
    mover_died = died(X, Y, m, m)
    if not mover_died:
        move = MOVE_OF[(Y.pos[m][0] - X.pos[m][0], Y.pos[m][1] - X.pos[m][1])]
    else:
        cand = death_candidates(X, m)
        move = cand[0] if len(cand) == 1 else 7
    victims = tuple(i for i in range(4) if i != m and died(X, Y, i, m))
    return (move, mover_died, victims, Y.carry[m] > X.carry[m], len(X.caps) > len(Y.caps), Y.ret[m] - X.ret[m])


def event_word(ev):
    move, mover_died, victims, ate, capsule, returned = ev
    return move | int(mover_died) << 3 | sum(1 << (4 + i) for i in victims) | int(ate) << 8 | int(capsule) << 9 | (returned & 0xFFF) << 10


class Log:
    """The head and the frames of one row.  Untouched frame words hold `fill` (the test's sentinel)."""

    def __init__(self, state, H, max_ticks, layout=0, fill=0):
        self.H, self.max_ticks, self.fill = H, max_ticks, fill
        self.len = self.done = self.overflow = 0
        self.layout = layout
        self.slots = (sorted(state.caps, key=lambda c: (c[1], c[0])) + [None] * 4)[:4]      # a slot keeps its cell until it is eaten
        self.frames = [(state, None)]            # (Frame, event or None)

    def update(self, subs, done):
        """subs: the four states after sub-steps 0 .. 3 of one tick"""
        if self.done or self.overflow:
            return
        if self.len == self.max_ticks:
            self.overflow = 1
            return
        X = self.frames[-1][0]
        for m in range(4):
            self.frames.append((subs[m], event(X, subs[m], m)))
            X = subs[m]
        self.len += 1
        self.done = int(bool(done))

    def head_words(self):
        w = np.zeros(HEAD_WORDS, np.int32)
        w[0], w[1], w[2], w[3] = self.len, self.done, self.overflow, self.layout
        return w

    def frame_words(self, k):
        s, ev = self.frames[k]
        w = np.zeros(12 + self.H, np.int64)
        for i in range(4):
            w[i] = s.pos[i][0] | s.pos[i][1] << 8 | s.dir[i] << 16 | s.pac[i] << 24
            w[4 + i] = s.scared[i] | s.carry[i] << 8 | s.ret[i] << 20
        slot = [(c[0] | c[1] << 8) if c is not None and c in s.caps else 0xFFFF for c in self.slots]
        w[8], w[9] = slot[0] | slot[1] << 16, slot[2] | slot[3] << 16
        w[10] = s.score & 0xFFFFFFFF
        w[11] = 0 if ev is None else event_word(ev)
        w[12:] = s.food
        return w.astype(np.uint32).view(np.int32)

    def words(self):
        """int32 [1 + 4 max_ticks, 12 + H]: the row's frames as the buffer holds them"""
        out = np.full((1 + 4 * self.max_ticks, 12 + self.H), self.fill, np.int32)
        for k in range(len(self.frames)):
            out[k] = self.frame_words(k)
        return out


def buffers(logs):
    """[Log] -> (head [8, n], frames [1 + 4 max_ticks, FW, n]), the device buffers' own order"""
    return np.stack([l.head_words() for l in logs], 1), np.stack([l.words() for l in logs], 2)
