"""Game records on the host (include/pmx.h, "Game records"): the log pmx_game_record_update keeps on the device, as numpy arrays
with the layouts the games were played on -- every sub-step's state, what happened in it, and the board as text.  No GPU here:
a saved record is read, replayed and rendered by tools/replay.py on any machine.

  GameRecord.render    GameStateData.__str__ (game.py:438-461) and Grid.__str__ (game.py:189-192) restated for frame words
"""
import json

import numpy as np

HEAD_WORDS = 8
LEN, DONE, OVERFLOW, LAYOUT = range(4)
W_SCORE, W_EVENT, W_FOOD = 10, 11, 12
MOVE_NAMES = {0: "North", 1: "East", 2: "South", 3: "West", 4: "Stop", -1: "?"}


def decode_event(word):
    """EVENT word -> (move, mover_died, victims, ate, capsule, returned); move is -1 for code 7 (undetermined)"""
    w = int(word) & 0xFFFFFFFF
    move = w & 7
    return (-1 if move == 7 else move, bool(w >> 3 & 1), tuple(i for i in range(4) if w >> (4 + i) & 1), bool(w >> 8 & 1), bool(w >> 9 & 1),
            w >> 10 & 0xFFF)


def _wall(rows, x, y):
    return rows[len(rows) - 1 - y][x] == "%"


class GameRecord:
    """head int32 [8, games], frames int32 [n_frames, 12 + H, games] (n_frames >= 1 + 4 * the longest game), layouts: the text
    rows (top row first) of every layout of the handle, meta: a JSON-able dict (first, max_ticks, length, and whatever the
    recorder adds)."""

    def __init__(self, head, frames, layouts, meta=None):
        self.head = np.ascontiguousarray(head, dtype=np.int32)
        self.frames = np.ascontiguousarray(frames, dtype=np.int32)
        self.layouts = [list(rows) for rows in layouts]
        self.meta = dict(meta or {})
        self.height, self.width = len(self.layouts[0]), len(self.layouts[0][0])
        if self.head.shape != (HEAD_WORDS, self.frames.shape[2]) or self.frames.shape[1] != W_FOOD + self.height:
            raise ValueError(f"head {self.head.shape} / frames {self.frames.shape} do not belong to a board of height {self.height}")
        if self.frames.shape[0] < 1 + 4 * int(self.head[LEN].max(initial=0)):
            raise ValueError("frames end before the longest game does")

    # -- the head ----------------------------------------------------------------------------------------------------
    @property
    def games(self):
        return self.head.shape[1]

    def length(self, g):
        """ticks recorded of game g"""
        return int(self.head[LEN, g])

    def done(self, g):
        return bool(self.head[DONE, g])

    def overflow(self, g):
        return bool(self.head[OVERFLOW, g])

    def layout(self, g):
        """the text rows of the layout game g was played on"""
        return self.layouts[int(self.head[LAYOUT, g])]

    # -- frames ------------------------------------------------------------------------------------------------------
    def frame(self, g, tick, substep=3):
        """the frame words after sub-step `substep` of tick `tick`; tick -1 is the state at init"""
        if tick == -1:
            return self.frames[0, :, g]
        if not (0 <= tick < self.length(g) and 0 <= substep < 4):
            raise IndexError(f"game {g} has ticks 0 .. {self.length(g) - 1} with sub-steps 0 .. 3, not ({tick}, {substep})")
        return self.frames[1 + 4 * tick + substep, :, g]

    def state(self, g, tick, substep=3):
        """the fields of pmx_state a frame holds: pos [4][2], dir, pac, scared, carry, ret [4], food and caps rows [H], score"""
        w = self.frame(g, tick, substep).view(np.uint32).astype(np.int64)
        a, b = w[0:4], w[4:8]
        caps = np.zeros(self.height, np.uint32)
        for word in w[8:10]:
            for slot in (word & 0xFFFF, word >> 16):
                if slot != 0xFFFF:
                    caps[slot >> 8] |= np.uint32(1 << (slot & 0xFF))
        return dict(pos=np.stack([a & 0xFF, a >> 8 & 0xFF], 1).astype(np.int8), dir=(a >> 16 & 0xFF).astype(np.int8),
                    pac=(a >> 24 & 1).astype(np.uint8), scared=(b & 0xFF).astype(np.uint8), carry=(b >> 8 & 0xFFF).astype(np.uint16),
                    ret=(b >> 20 & 0xFFF).astype(np.uint16), food=w[W_FOOD:].astype(np.uint32), caps=caps,
                    score=int(self.frame(g, tick, substep)[W_SCORE]))

    def events(self, g):
        """[(tick, mover, move, mover_died, victims, ate, capsule, returned)] for every recorded sub-step of game g"""
        n = self.length(g)
        ev = self.frames[1:1 + 4 * n, W_EVENT, g]
        return [(k // 4, k % 4) + decode_event(ev[k]) for k in range(4 * n)]

    def moves(self, g):
        """int8 [length][4]: the move each agent made in each tick (0 N, 1 E, 2 S, 3 W, 4 Stop), -1 where undetermined"""
        n = self.length(g)
        m = (self.frames[1:1 + 4 * n, W_EVENT, g] & 7).astype(np.int8).reshape(n, 4)
        m[m == 7] = -1
        return m

    def render(self, g, tick, substep=3):
        """the board after that sub-step as the reference prints a GameStateData, followed by its Score line"""
        s = self.state(g, tick, substep)
        rows = self.layout(g)
        H, W = self.height, self.width
        cell = [[("." if int(s["food"][y]) >> x & 1 else "%" if _wall(rows, x, y) else " ") for x in range(W)] for y in range(H)]
        for i in range(4):
            x, y = int(s["pos"][i][0]), int(s["pos"][i][1])
            d = int(s["dir"][i])
            cell[y][x] = ("v" if d == 0 else "^" if d == 2 else ">" if d == 3 else "<") if s["pac"][i] else "G"
        for y in range(H):
            for x in range(W):
                if int(s["caps"][y]) >> x & 1:
                    cell[y][x] = "o"
        return "\n".join("".join(r) for r in reversed(cell)) + "\nScore: %d\n" % s["score"]

    def final_score(self, g):
        return int(self.frames[4 * self.length(g), W_SCORE, g])

    # -- files -------------------------------------------------------------------------------------------------------
    def save(self, path):
        """one .npz: head, frames (cut behind the longest game) and the layouts + metadata as JSON bytes"""
        n = 1 + 4 * int(self.head[LEN].max(initial=0))
        doc = json.dumps(dict(layouts=self.layouts, meta=self.meta)).encode()
        with open(path, "wb") as f:
            np.savez_compressed(f, head=self.head, frames=self.frames[:n], doc=np.frombuffer(doc, np.uint8))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            doc = json.loads(bytes(z["doc"]).decode())
            return cls(z["head"], z["frames"], doc["layouts"], doc["meta"])
