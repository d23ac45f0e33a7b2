"""pmx_belief_update_evidence / pmx_belief_weights_update_evidence / pmx_belief_evidence_init against the numpy model
tests/_belief_evidence_ref.py (which tests/test_belief_evidence_cpu.py holds to the golden trajectories): every word of the sets, the
readings and the evidence rows at every tick of bot games with resets on three boards and a redrawn maze pool, both colours, mixed
colours and a first / count range, the rule masks 0, 1, 2, 4, 7; mask 0 against pmx_belief_update; the weighted form against the set
form and the weights model; and hand-set one-tick states for the edges."""
import numpy as np
import pytest
import torch

import _belief_evidence_ref as E
import _belief_ref as R
import _belief_weights_ref as RW
import _golden as G
from test_gpu_belief import BOT_CODES, POOL_CODES, SEED, _board_arrays, _positions, _words
from test_gpu_belief_weights import _Band, _u16

pytestmark = pytest.mark.gpu

N = 37                       # ten blocks of four envs, the last one ragged
TICKS = 90
LENGTH = 40                  # at least two resets of every env within TICKS
N_MAZES = 8
# In these short bot games pellets leave a defended half on smallCapture only (some 500 firings of the food rule in 37 envs x 90
# ticks; none on tinyCapture, bloxCapture and the maze pool, where a raider is killed or the game ends before it eats).  So a fifth
# game, "golden", replays the first GOLDEN_TICKS actions of the golden hunter trajectory on smallCapture in every env (one game, a
# noise stream per env), where pellets are eaten from tick 15 on.
GOLDEN_TICKS = 120
CODES = {"tinyCapture": BOT_CODES, "smallCapture": BOT_CODES, "bloxCapture": BOT_CODES, "mazes": POOL_CODES, "golden": BOT_CODES}


def _make(pmx, board, n):
    if board == "mazes":
        from pmx import maze_generator
        lays = [pmx.Layout.from_text(maze_generator.generate_maze(k + 1)) for k in range(N_MAZES)]
        return pmx.PmxVecEnv(lays, n, length=LENGTH, auto_reset=True, obs_dtype="uint8", seed=SEED, bots=True,
                             layout_index=np.arange(n) % N_MAZES, redraw_layouts=True)
    if board == "golden":
        return pmx.PmxVecEnv("smallCapture", n, length=300, auto_reset=True, obs_dtype="uint8", seed=SEED, bots=True)
    return pmx.PmxVecEnv(board, n, length=LENGTH, auto_reset=True, obs_dtype="uint8", seed=SEED, bots=True)


def _food(states):
    return np.array([[s.food[y] for y in range(32)] for s in states], np.uint32)


def _snapshots(sub_pos, sub_food, first):
    """(P [n, 2, 4, 2], F [n, 2, 32]) of learners of the colours `first` [n] from the states after the four sub-steps"""
    ar = np.arange(len(first))
    return np.stack([sub_pos[ar, first], sub_pos[ar, first + 2]], 1), np.stack([sub_food[ar, first], sub_food[ar, first + 2]], 1)


@pytest.mark.parametrize("board", ("tinyCapture", "smallCapture", "bloxCapture", "mazes", "golden"))
def test_every_word_reading_and_evidence_row_equals_the_model(board):
    """Two handles with one seed, as tests/test_gpu_belief.py runs them: A steps whole ticks and runs the updates, B steps agent by
    agent and supplies positions and food after every sub-step.  A finished env shows the fresh game in all four snapshots."""
    import pmx
    A, B = _make(pmx, board, N), _make(pmx, board, N)
    A.reset(want_obs=False)
    B.reset(want_obs=False)
    dev = A.device
    H, W = A.layout.height, A.layout.width
    half = W // 2
    codes = torch.tensor(CODES[board], dtype=torch.int8, device=dev)[None].expand(N, 4).contiguous()
    mixed = (torch.arange(N, device=dev) % 3 == 0).to(torch.uint8)
    # (colour, rules, first, count); the last one is the weighted form
    cases = [(True, 7, 0, N), (False, 7, 0, N), (mixed, 7, 0, N), (mixed, 7, 5, 29), (mixed, 1, 0, N), (mixed, 2, 0, N), (mixed, 4, 0, N),
             (mixed, 0, 0, N), (mixed, 7, 0, N)]
    weighted = len(cases) - 1
    open_g, starts = _board_arrays(A)
    bufs, models = [], []
    for c, (_, _, lo, cnt) in enumerate(cases):
        ev = _Band(cnt, (36,), torch.int32, dev)
        A.belief_evidence_init(ev.out, lo, cnt)
        assert (ev.out == 0).all() and ev.untouched()
        sn = torch.full((cnt, 2, 2), 99, dtype=torch.int8, device=dev)
        words = R.init(0, open_g[lo:lo + cnt], starts[lo:lo + cnt])
        if c == weighted:
            bufs.append((A.belief_weights_init(A.new_belief(cnt), *A.new_belief_weights(cnt), 0, lo, cnt), ev, sn))
            models.append([words, E.init(cnt), RW.init(0, open_g, starts, H, W)[1]])
        else:
            bufs.append((A.belief_init(A.new_belief(cnt), 0, lo, cnt), ev, sn))
            models.append([words, E.init(cnt)])
    parent = A.belief_init(A.new_belief(), 0)
    parent_sn = torch.full((N, 2, 2), 98, dtype=torch.int8, device=dev)
    stats = {}
    resets = narrower = 0
    replay = G.load("traj_small_hunter.npz")[0]["actions"] if board == "golden" else None
    for t in range(TICKS if replay is None else GOLDEN_TICKS):
        if replay is not None:
            codes = torch.tensor(replay[t], dtype=torch.int8, device=dev)[None].expand(N, 4).contiguous()
        A.step(codes, want_obs=False)
        pos, food = [], []
        for agent in range(4):
            B.step_agent(agent, codes[:, agent].contiguous(), want_obs=False)
            st = B.get_state()
            pos.append(_positions(st))
            food.append(_food(st))
        ticks = np.array([s.ticks for s in st], np.uint32)
        assert torch.equal(A.done, B.done)
        done = A.done.cpu().numpy().astype(bool)
        resets += int(done.sum())
        sub_pos, sub_food = np.stack(pos, 1), np.stack(food, 1)
        sub_pos[done], sub_food[done] = sub_pos[done, 3:], sub_food[done, 3:]          # the fresh game
        open_g, starts = _board_arrays(A)
        A.belief_update(mixed, parent, 5, reset=A.done, sonar=parent_sn)
        for c, ((colour, rules, lo, cnt), (b, ev, sn), m) in enumerate(zip(cases, bufs, models)):
            rows = slice(lo, lo + cnt)
            red = (colour.cpu().numpy().astype(bool) if isinstance(colour, torch.Tensor) else np.full(N, colour))[rows]
            P, F = _snapshots(sub_pos[rows], sub_food[rows], np.where(red, 0, 1))
            args = (P, F, red, 5, ticks[rows], SEED, np.arange(N)[rows], open_g[rows], starts[rows], half)
            if c == weighted:
                A.belief_weights_update(colour, *b, 5, reset=A.done, first=lo, count=cnt, sonar=sn, evidence=ev.out, rules=rules)
                w, lev, want, readings, seen, want_ev = E.weights_update(m[2], m[0], m[1], *args, H, W, rules=rules, reset=done[rows])
                assert (_u16(b[1]).reshape(cnt, 2, 2, H, W) == w).all(), (board, t, "weights")
                assert (b[2].cpu().numpy().reshape(cnt, 2, H, W) == lev).all(), (board, t, "levels")
                assert torch.equal(b[0], bufs[2][0]) and torch.equal(sn, bufs[2][2]), (board, t, "the weighted form's sets and readings")
                m[2] = w
                b = b[0]
            else:
                A.belief_update(colour, b, 5, reset=A.done, first=lo, count=cnt, sonar=sn, evidence=ev.out, rules=rules)
                want, readings, seen, want_ev = E.update(m[0], m[1], *args, rules=rules, reset=done[rows], stats=stats if c == 2 else None)
            bad = np.nonzero((_words(b) != want).reshape(cnt, -1).any(1))[0]
            assert len(bad) == 0, (board, t, c, bad[:8] + lo)
            assert (sn.cpu().numpy() == readings).all(), (board, t, c)
            assert (_words(ev.out) == want_ev).all() and ev.untouched(), (board, t, c)
            m[0], m[1] = want, want_ev
            if rules == 0:
                assert torch.equal(b, parent) and torch.equal(sn, parent_sn), (board, t, "mask 0 against pmx_belief_update")
            if c == 2:                                              # soundness on the envs that were not reset, and what the rules removed
                cells, pcells = R.unpack(want), R.unpack(_words(parent))
                assert not (cells & ~pcells).any()
                narrower += int((cells.sum((-1, -2)) < pcells.sum((-1, -2)))[~done].sum())
                first = np.where(red, 0, 1)
                for j in range(2):
                    for k in range(2):
                        e = P[np.arange(N), j, (1 - first) + 2 * k]
                        assert cells[np.arange(N), j, k, e[:, 1], e[:, 0]][~done].all(), (board, t, j, k)
    fired = int(np.sum(stats.get("food", 0)))
    print(f"{board}: {resets} resets, food rule fired {fired} times, held back {int(np.sum(stats.get('excluded', 0)))} times, "
          f"{narrower} sets narrower than the parent's")
    assert narrower > 100
    assert fired > 0 if replay is not None else resets >= 2 * N
    A.close()
    B.close()


# ---- hand-set one-tick states ---------------------------------------------------------------------------------------------------
def _state(pmx, pos, food, caps, H, W):
    pac = [(i in (0, 2)) != (pos[i][0] < W // 2) for i in range(4)]
    return pmx.make_state(pos, [4] * 4, pac, [0] * 4, [0] * 4, [0] * 4, food, caps, 0, 0, H)


def _hand_rows(lay):
    """-> (rows of (tag, red, S0 positions, S1 positions, pellet cell or None), the two hand-written one-cell sets)"""
    H, W = lay.height, lay.width
    half = W // 2
    s = [tuple(int(v) for v in lay.starts[i]) for i in range(4)]
    free = [(x, y) for y in range(1, H - 1) for x in range(1, W - 1) if not (int(lay.wall_rows[y]) >> x) & 1]
    dist = lambda p, q: abs(p[0] - q[0]) + abs(p[1] - q[1])
    nbs = lambda c: [f for f in free if dist(f, c) == 1]

    def far_pair(*cells, gap=8):
        """two open cells more than `gap` from every cell given, from the team's start cells' neighbourhoods and from one another"""
        ok = [f for f in free if all(dist(f, c) > gap for c in cells)]
        a = ok[0]
        return a, next(f for f in ok if dist(f, a) > 2)

    def pellet(red, cond, near=None, away=(), key=None):
        """(c, nb): an open cell c of the defended half with cond(c), more than 1 from the cells `away`, and an open neighbour of it;
        the first one, or the one with the least key"""
        mine = (lambda c: c[0] < half) if red else (lambda c: c[0] >= half)
        ok = [c for c in free if mine(c) and cond(c) and nbs(c) and all(dist(c, a) > 1 for a in away) and (near is None or dist(c, near) == 1)]
        c = min(ok, key=key) if key else ok[0]
        return c, nbs(c)[0]

    rows = []                                                       # (tag, red, S0 positions, S1 positions, pellet)

    def add(tag, red, c, nb, before=None):
        """the mover steps from nb onto c; the team stands far from both, in S0 on the cells `before` if given"""
        mover, other = (3, 1) if red else (0, 2)
        team = far_pair(c, nb, s[mover], s[other])
        p0, p1 = [None] * 4, [None] * 4
        for p, cell, (t0, t1) in ((p0, nb, before or team), (p1, c, team)):
            p[mover], p[other] = cell, s[other]
            p[0 if red else 1], p[2 if red else 3] = t0, t1
        rows.append((tag, red, p0, p1, c))

    both = (s[0], s[2], s[1], s[3])
    add("half-1", True, *pellet(True, lambda c: c[0] == half - 1, away=both))
    add("half", False, *pellet(False, lambda c: c[0] == half, away=both))
    add("top", True, *pellet(True, lambda c: True, away=both, key=lambda c: c[1]))            # the outermost rows that can hold one
    add("bottom", False, *pellet(False, lambda c: True, away=both, key=lambda c: -c[1]))
    c, nb = pellet(True, lambda c: len(nbs(c)) >= 2, away=both)
    learner = nbs(c)[1]                                             # the learner of slot 0 (agent 0) stood next to c in S0
    add("near learner", True, c, nb, before=(learner, far_pair(c, nb)[0]))
    c, nb = pellet(True, lambda c: True, near=s[0])
    add("near start", True, c, nb)
    # the two contact rows: red learners far away, no pellet leaves; the prior set of both enemies is written by hand below
    by_start = nbs(s[0])[0]
    lonely = next(f for f in free if all(dist(f, q) > 3 for q in both))
    t0, t1 = far_pair(by_start, lonely, s[1], s[3], gap=7)
    for tag in ("start only", "nowhere"):
        p = [t0, s[1], t1, s[3]]
        rows.append((tag, True, p, list(p), None))
    return rows, by_start, lonely


@pytest.mark.parametrize("board", ("bloxCapture", "maze32"))
def test_hand_set_states(board):
    """Per env two states set from outside, S0 then S1, an update after each.  The first update follows the init (valid = 0: no food
    rule, the parents' respawn rule); the second sees S0 in the evidence row.  Between the two the enemy that moves before slot 0
    (agent 3 for red learners, agent 0 for blue ones) steps onto a pellet c that S1 no longer holds:
      half-1, half     c in column half - 1 (red learners) and in column half (blue learners), the two columns at the border of `mine`;
      top, bottom      c in the outermost rows that can hold a pellet away from the start cells, rows 1 and H - 2 on maze32.  The issue
                       names rows 0 and H - 1; pmx_create refuses a layout whose border rows are not walls and pmx_set_state
                       refuses food inside a wall, so no handle can hold a pellet there.  On the 32-row board lanes 0 and 31
                       stand at the ends of the ballot and the shuffles with E = 0;
      near learner     c one step from the cell the learner of slot 0 had in S0: the rule must not fire;
      near start       c one step from that learner's start cell: likewise;
      start only       the team far away and the set before the update, written by hand, one cell next to a team start cell: it
                       touches K there only, and the enemy's start cell joins;
      nowhere          the same with a set far from all of K: the start cell does not join.
    maze32 is 32 cells wide and high: bit 31 and lane 31 exist."""
    import pmx
    if board == "maze32":
        from pmx import maze_generator
        lay = pmx.Layout.from_text(maze_generator.generate_maze(11, rows=30, cols=15))
        assert (lay.width, lay.height) == (32, 32)
    else:
        lay = pmx.get_layout(board)
    H, W = lay.height, lay.width
    half = W // 2
    rows, by_start, lonely = _hand_rows(lay)
    n = len(rows)
    env = pmx.PmxVecEnv(lay, n, length=300, auto_reset=True, obs_dtype="uint8", seed=SEED)
    env.reset(want_obs=False)
    base = env.get_state(0, 1)[0]
    base_food = np.array([base.food[y] for y in range(32)], np.uint32)
    foods = []
    for tag, red, p0, p1, c in rows:
        f0 = base_food.copy()
        if c is not None:
            f0[c[1]] |= np.uint32(1 << c[0])
        f1 = f0.copy()
        if c is not None:
            f1[c[1]] &= ~np.uint32(1 << c[0])
        foods.append((f0, f1))
    red = np.array([r[1] for r in rows])
    red_t = torch.tensor(red, dtype=torch.uint8, device=env.device)
    open_g, starts = _board_arrays(env)
    ar = np.arange(n)
    tag_row = {r[0]: i for i, r in enumerate(rows)}
    results = {}
    for rules in (7, 2, 4, 1, 0):
        bel, ev = env.belief_init(env.new_belief(), 1), env.belief_evidence_init(env.new_belief_evidence())
        m_words, m_ev = R.init(1, open_g, starts), E.init(n)
        sonar = torch.full((n, 2, 2), 99, dtype=torch.int8, device=env.device)
        for step in (0, 1):
            env.set_state([_state(pmx, r[2 + step], foods[i][step], base.caps, H, W) for i, r in enumerate(rows)])
            ticks = np.array([st.ticks for st in env.get_state()], np.uint32)
            pos = np.array([r[2 + step] for r in rows], np.int64)
            P = np.stack([pos, pos], 1)                             # no tick was run: both slots read the current state
            F = np.stack([foods[i][step] for i in range(n)])
            F = np.stack([F, F], 1)
            if step == 1:                                           # the sets S1's update starts from: every open cell, two rows by hand
                m_words = R.init(1, open_g, starts)
                for tag, cell in (("start only", by_start), ("nowhere", lonely)):
                    m_words[tag_row[tag]] = R.pack(R.one_cell(np.array([cell])))[0]
                bel.copy_(torch.from_numpy(m_words.view(np.int32)))
            assert (_words(ev)[:, 34] == step).all()                # valid = 0 after the init, 1 after an update
            env.belief_update(red_t, bel, 5, sonar=sonar, evidence=ev, rules=rules)
            m_words, readings, seen, m_ev = E.update(m_words, m_ev, P, F, red, 5, ticks, SEED, ar, open_g, starts, half, rules=rules)
            assert (_words(bel) == m_words).all(), (board, rules, step)
            assert (sonar.cpu().numpy() == readings).all(), (board, rules, step)
            assert (_words(ev) == m_ev).all(), (board, rules, step)
        results[rules] = (R.unpack(m_words), seen)
    seen, plain = results[7][1], results[0][0]
    for tag in ("half-1", "half", "top", "bottom"):
        i = tag_row[tag]
        k, c = (1, rows[i][4]) if red[i] else (0, rows[i][4])       # the enemy that moved before slot 0
        assert not seen[i, 0, k], tag
        for r in (7, 2):
            got = results[r][0][i, 0, k]
            assert got[c[1], c[0]] and got.sum() <= 2, (board, tag, r)   # the pellet's cell (and the start cell, where K is touched)
        assert plain[i, 0, k].sum() > 2, (board, tag)
    for tag in ("near learner", "near start"):
        i = tag_row[tag]
        assert (results[2][0][i] == plain[i]).all(), (board, tag)   # held back: the learner can have eaten it
    # contact: the true enemies stand on their start cells, out of sight, so the parents' sets hold the start cell in both slots
    near, far = tag_row["start only"], tag_row["nowhere"]
    for k, e in enumerate((1, 3)):
        sx, sy = (int(v) for v in lay.starts[e])
        assert plain[near, :, k, sy, sx].all() and plain[far, :, k, sy, sx].all()
        for r in (7, 4):
            assert results[r][0][near, :, k, sy, sx].all(), (board, r, k)       # the set touched K next to the team's start cell only
            assert not results[r][0][far, :, k, sy, sx].any(), (board, r, k)
    env.close()


def test_argument_errors():
    import pmx
    from pmx import _lib
    n = 5
    env = pmx.PmxVecEnv("tinyCapture", n, obs_dtype="uint8", seed=1)
    env.reset(want_obs=False)
    lib = _lib.load()
    st = _lib.stream(env.device)
    b, (w, lv), ev = env.belief_init(env.new_belief(), 0), env.new_belief_weights(), env.new_belief_evidence()
    keep = b.clone()
    INVALID = -1
    for rules in (-1, 8):
        assert lib.pmx_belief_update_evidence(env.handle, 1, None, 0, n, 5, rules, None, b.data_ptr(), None, ev.data_ptr(), st) == INVALID
        assert b"pmx_belief_update_evidence: rules" in lib.pmx_last_error()
        assert lib.pmx_belief_weights_update_evidence(env.handle, 1, None, 0, n, 5, rules, None, b.data_ptr(), None, w.data_ptr(), lv.data_ptr(),
                                                      ev.data_ptr(), st) == INVALID
        assert b"pmx_belief_weights_update_evidence: rules" in lib.pmx_last_error()
    assert lib.pmx_belief_update_evidence(env.handle, 1, None, 0, n, 5, 7, None, b.data_ptr(), None, None, st) == INVALID
    assert lib.pmx_belief_weights_update_evidence(env.handle, 1, None, 0, n, 5, 7, None, b.data_ptr(), None, w.data_ptr(), lv.data_ptr(), None, st) == INVALID
    assert lib.pmx_belief_weights_update_evidence(env.handle, 1, None, 0, n, 5, 7, None, b.data_ptr(), None, None, lv.data_ptr(), ev.data_ptr(), st) == INVALID
    assert lib.pmx_belief_update_evidence(env.handle, 1, None, 0, n, 65, 7, None, b.data_ptr(), None, ev.data_ptr(), st) == INVALID
    for first, count in ((-1, 2), (0, -1), (0, n + 1), (n, 1), (3, 3)):
        assert lib.pmx_belief_update_evidence(env.handle, 1, None, first, count, 5, 7, None, b.data_ptr(), None, ev.data_ptr(), st) == INVALID
        assert b"pmx_belief_update_evidence: envs" in lib.pmx_last_error()
        assert lib.pmx_belief_evidence_init(env.handle, first, count, ev.data_ptr(), st) == INVALID
    for first in (0, 2, n):                                        # an empty range is fine and launches nothing
        assert lib.pmx_belief_update_evidence(env.handle, 1, None, first, 0, 5, 7, None, b.data_ptr(), None, ev.data_ptr(), st) == 0
        assert lib.pmx_belief_evidence_init(env.handle, first, 0, ev.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(b, keep) and (ev == 0).all()                # none of the calls above wrote a word
    env.profile_begin(4)                                           # recorded with the rule launches, as the parents are
    env.belief_update(True, b, 5, evidence=ev)
    prof = env.profile_end()
    assert prof["rule_launches"] == 1 and prof["rule_ms"] > 0
    env.close()
