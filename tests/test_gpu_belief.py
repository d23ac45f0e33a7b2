"""pmx_belief_update / pmx_belief_init / pmx_emit_team_obs_belief against the numpy model tests/_belief_ref.py (which
tests/test_belief_cpu.py pins to the reference's sonar readings and to the golden trajectories): every word of the buffer and every
reading at every tick of bot games on three boards and a redrawn maze pool, the emission's planes against the plain emission, and
hand-set states for the edges (shuffle ends, bit 31, negative readings, the reset mask)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _belief_ref as R

pytestmark = pytest.mark.gpu

N = 67                       # a ragged last block (four envs per block)
TICKS = 150
LENGTH = 60                  # at least two resets of every env within TICKS
SEED = 9
N_MAZES = 8
BOT_CODES = (-3, -3, -4, -4)                 # baselineTeam on both sides: agents 0, 1 offensive, 2, 3 defensive
POOL_CODES = (-2, -2, -2, -2)                # the maze pool: randomTeam on both sides (the oracle's reflex bots know one layout)
# Coverage of a run, measured on the end-of-tick states: the share of (tick, env, colour, enemy) cases in which the enemy is hidden
# at sight 5, the share in which it is seen, and the respawns (an agent back on its start cell from more than one cell away in a tick
# without a reset).  The required shares are half of what the CPU oracle yields for the same bots and seeds (67 envs, 150 ticks,
# length 60; the oracle reproduces the in-kernel bots and the layout draws bit for bit):
#   tinyCapture   oracle hidden 0.5209 / seen 0.4791, 270 respawns
#   smallCapture  oracle hidden 0.5379 / seen 0.4621, 940 respawns
#   bloxCapture   oracle hidden 0.5957 / seen 0.4043,  63 respawns
#   mazes         oracle hidden 0.9927 / seen 0.0073,   1 respawn   (random walkers on 20 x 20 mazes seldom meet)
REQUIRED = {"tinyCapture": (0.2604, 0.2395), "smallCapture": (0.2689, 0.2310), "bloxCapture": (0.2978, 0.2021), "mazes": (0.4963, 0.0036)}


def _positions(states):
    return np.array([[[s.pos[i][0], s.pos[i][1]] for i in range(4)] for s in states], np.int64)


@functools.lru_cache(maxsize=None)
def _pool():
    from pmx import maze_generator
    return tuple(tuple(maze_generator.generate_maze(k + 1).split("\n")) for k in range(N_MAZES))


def _make(pmx, board, n, **kw):
    if board == "mazes":
        lays = [pmx.Layout.from_text("\n".join(r)) for r in _pool()]
        return pmx.PmxVecEnv(lays, n, length=LENGTH, auto_reset=True, obs_dtype="uint8", seed=SEED, bots=True,
                             layout_index=np.arange(n) % N_MAZES, redraw_layouts=True, **kw)
    return pmx.PmxVecEnv(board, n, length=LENGTH, auto_reset=True, obs_dtype="uint8", seed=SEED, bots=True, **kw)


def _board_arrays(env):
    """(open cells [n, 32, 32], starts [n, 4, 2]) of the layout each env is on right now"""
    idx = env.layout_indices()
    W, H = env.layout.width, env.layout.height
    open_l = np.stack([R.open_cells(l.wall_rows, W, H) for l in env.layouts])
    starts_l = np.stack([l.starts.astype(np.int64) for l in env.layouts])
    return open_l[idx], starts_l[idx]


def _words(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("board", ("tinyCapture", "smallCapture", "bloxCapture", "mazes"))
def test_every_word_and_reading_equals_the_model(board):
    """Two handles with one seed: A runs pmx_step + pmx_belief_update, B the four pmx_step_agent calls with the same codes (the
    equivalence tests/test_gpu_parity.py pins) and supplies the positions after every sub-step and the tick counter."""
    import pmx
    A, B = _make(pmx, board, N), _make(pmx, board, N)
    A.reset(want_obs=False)
    B.reset(want_obs=False)
    dev = A.device
    codes = torch.tensor(POOL_CODES if board == "mazes" else BOT_CODES, dtype=torch.int8, device=dev)[None].expand(N, 4).contiguous()
    mixed = (torch.arange(N, device=dev) % 3 == 0).to(torch.uint8)
    # (colour, sight): both uniform colours, a per-env colour, and sight 0 on one board
    cases = [(True, 5), (False, 5), (mixed, 5)] + ([(True, 0), (False, 0)] if board == "smallCapture" else [])
    env_idx = np.arange(N)
    open_g, starts = _board_arrays(A)
    bufs, sonars, models = [], [], []
    for _ in cases:
        b = A.belief_init(A.new_belief(), 0)
        bufs.append(b)
        sonars.append(torch.full((N, 2, 2), 99, dtype=torch.int8, device=dev))
        models.append(R.init(0, open_g, starts))
        assert (_words(b) == models[-1]).all()
    hidden = seen = total = respawns = resets = 0
    prev_end = _positions(B.get_state())
    for t in range(TICKS):
        A.step(codes, want_obs=False)
        sub = []
        for agent in range(4):
            B.step_agent(agent, codes[:, agent].contiguous(), want_obs=False)
            st = B.get_state()
            sub.append(_positions(st))
        ticks = np.array([s.ticks for s in st], np.uint32)
        assert torch.equal(A.done, B.done)
        done = A.done.cpu().numpy().astype(bool)
        open_g, starts = _board_arrays(A)                      # after the step: a reset env is on its new maze
        for (colour, sight), b, sn, c in zip(cases, bufs, sonars, range(len(cases))):
            A.belief_update(colour, b, sight, reset=A.done, sonar=sn)
            red = colour.cpu().numpy().astype(bool) if isinstance(colour, torch.Tensor) else np.full(N, colour)
            first = np.where(red, 0, 1)
            sub_a = np.stack(sub, 1)                           # [N, 4 sub-steps, 4 agents, 2]
            P = np.stack([sub_a[env_idx, first], sub_a[env_idx, first + 2]], 1)
            want, readings, was_seen = R.update(models[c], P, red, sight, ticks, SEED, env_idx, open_g, starts, reset=done)
            got = _words(b)
            bad = np.nonzero((got != want).reshape(N, -1).any(1))[0]
            assert len(bad) == 0, (board, t, c, bad[:8])
            assert (sn.cpu().numpy() == readings).all(), (board, t, c)
            models[c] = want
            # soundness, on the envs that were not reset: the enemy's cell is in its set, no wall cell is, one cell when seen
            cells = R.unpack(want)
            assert not (cells & ~open_g[:, None, None]).any()
            for j in range(2):
                for k in range(2):
                    e = P[env_idx, j, (1 - first) + 2 * k]
                    assert cells[env_idx, j, k, e[:, 1], e[:, 0]][~done].all(), (board, t, c, j, k)
                    assert (cells[:, j, k].sum((-1, -2)) == 1)[was_seen[:, j, k] & ~done].all()
        end = sub[3]
        for red in (True, False):
            team, foe = ((0, 2), (1, 3)) if red else ((1, 3), (0, 2))
            for e in foe:
                d = np.minimum(R.manhattan(end[:, e], end[:, team[0]]), R.manhattan(end[:, e], end[:, team[1]]))
                hidden += int((d > 5)[~done].sum())
                seen += int((d <= 5)[~done].sum())
                total += int((~done).sum())
        home = (end == starts).all(-1) & (R.manhattan(prev_end, starts) > 1)
        respawns += int(home[~done].sum())
        resets += int(done.sum())
        prev_end = end
    print(f"{board}: hidden share {hidden / total:.4f}, seen share {seen / total:.4f}, respawns {respawns}, resets {resets}")
    assert resets >= 2 * N
    need_hidden, need_seen = REQUIRED[board]
    assert hidden / total >= need_hidden and seen / total >= need_seen and respawns >= 1, (board, hidden / total, seen / total, respawns)
    A.close()
    B.close()


# ---- the emission ---------------------------------------------------------------------------------------------------------------
PAD = 2


def _bytes(t):
    return t.contiguous().view(torch.uint8)


class _Canary:
    """an output of `rows` rows with PAD rows of NaN (float planes) / 0xA5 (byte planes) before and after it"""

    def __init__(self, rows, row_shape, dtype):
        fill = 0xA5 if dtype == torch.uint8 else float("nan")
        self.buf = torch.full((rows + 2 * PAD,) + row_shape, fill, dtype=dtype, device="cuda")
        self.rows = rows
        self.out = self.buf[PAD:PAD + rows]
        self.was = _bytes(self.buf).clone()

    def untouched(self, written=None):
        written = self.rows if written is None else written
        now, per = _bytes(self.buf), _bytes(self.buf[0]).numel()
        a, b = PAD * per, (PAD + written) * per
        return torch.equal(now.flatten()[:a], self.was.flatten()[:a]) and torch.equal(now.flatten()[b:], self.was.flatten()[b:])


def _plane5(belief, red, H, W):
    """what plane 5 of the two slots must hold: [n, 2, H, W] 0 / 1, the OR of the two sets, x-flipped where red [n]"""
    cells = torch.from_numpy(R.unpack(_words(belief)).any(2)[:, :, :H, :W]).cuda()
    return torch.where(red.view(-1, 1, 1, 1).to(torch.bool), cells.flip(-1), cells)


@pytest.mark.parametrize("board", ("smallCapture", "bloxCapture"))
@pytest.mark.parametrize("dtype", ("float32", "bfloat16", "uint8"))
def test_emission_planes(dtype, board):
    import pmx
    env = pmx.PmxVecEnv(board, N, length=LENGTH, auto_reset=True, obs_dtype=dtype, seed=SEED, bots=True)
    env.reset(want_obs=False)
    dev, dt, shape = env.device, env.obs_torch_dtype, env.obs_shape
    H, W = env.layout.height, env.layout.width
    codes = torch.tensor(BOT_CODES, dtype=torch.int8, device=dev)[None].expand(N, 4).contiguous()
    colour = (torch.arange(N, device=dev) % 2).to(torch.uint8)
    uni = {red: env.belief_init(env.new_belief(), 0) for red in (True, False)}
    mix = env.belief_init(env.new_belief(), 0)
    multi = 0
    for t in range(24):
        env.step(codes, want_obs=False)
        for red in (True, False):
            env.belief_update(red, uni[red], 5, reset=env.done)
        env.belief_update(colour, mix, 5, reset=env.done)
        if t % 6 != 5:
            continue
        for red in (True, False):
            keep = uni[red].clone()
            team, merged = torch.empty((N, 2) + shape, dtype=dt, device=dev), torch.empty((N,) + shape, dtype=dt, device=dev)
            env.emit_team_obs(red, team, merged)
            bt, bm = _Canary(N, (2,) + shape, dt), _Canary(N, shape, dt)
            env.emit_team_obs(red, bt.out, bm.out, belief=uni[red])
            want5 = _plane5(uni[red], torch.full((N,), int(red), device=dev), H, W)
            multi += int((want5.sum((-1, -2)) > 2).sum())
            assert torch.equal(bt.out[:, :, 5], want5.to(dt)), (t, red)
            others = [0, 1, 2, 3, 4, 6, 7]
            assert torch.equal(_bytes(bt.out[:, :, others]), _bytes(team[:, :, others])), (t, red)
            assert torch.equal(_bytes(bm.out), _bytes(merged)), (t, red)            # the critic's input: the true enemies
            assert bt.untouched() and bm.untouched() and torch.equal(uni[red], keep), (t, red)
            bt2 = _Canary(N, (2,) + shape, dt)                                       # merged = NULL
            env.emit_team_obs(red, bt2.out, None, belief=uni[red])
            assert torch.equal(_bytes(bt2.out), _bytes(bt.out)) and bt2.untouched()
        # per-env colour, the full range and a sub-range (rows 0 .. count - 1 of the buffer belong to the envs first ..)
        keep = mix.clone()
        team, merged = torch.empty((N, 2) + shape, dtype=dt, device=dev), torch.empty((N,) + shape, dtype=dt, device=dev)
        env.emit_team_obs_mixed(colour, team, merged)
        for first, count in ((0, N), (5, 29)):
            bt, bm = _Canary(N, (2,) + shape, dt), _Canary(N, shape, dt)
            rows = mix[first:first + count].contiguous()
            env.emit_team_obs_mixed(colour, bt.out[:count], bm.out[:count], first, count, belief=rows)
            want = team[first:first + count].clone()
            want[:, :, 5] = _plane5(rows, colour[first:first + count], H, W).to(dt)
            assert torch.equal(_bytes(bt.out[:count]), _bytes(want)), (t, first)
            assert torch.equal(_bytes(bm.out[:count]), _bytes(merged[first:first + count])), (t, first)
            assert bt.untouched(count) and bm.untouched(count), (t, first)
        assert torch.equal(mix, keep)
    assert multi > N                                                                 # sets of more than a cell were emitted
    env.close()


# ---- hand-set states ------------------------------------------------------------------------------------------------------------
def _hand_states(pmx, env, base, rows):
    H, W = env.layout.height, env.layout.width
    out = []
    for pos in rows:
        pac = [(i in (0, 2)) != (pos[i][0] < W / 2) for i in range(4)]
        out.append(pmx.make_state(pos, [4] * 4, pac, [0] * 4, [0] * 4, [0] * 4, base.food, base.caps, 0, 0, H))
    return out


@pytest.mark.parametrize("board", ("bloxCapture", "maze32"))
def test_hand_set_states(board):
    """set_state + belief_init(kind 1) + one update against the model, blue learners (1, 3; enemies 0, 2) and red ones: an enemy at
    distance exactly sight and sight + 1, both enemies on one cell, an enemy on its start, agents on the outermost open cells (rows
    1 / H - 2, columns 1 / W - 2: pmx_set_state takes no wall cell and every board has a wall border, so the sets' rows 0 and H - 1
    and bits 0 and W - 1 -- bit 31 on the 32-wide board -- hold what the shuffles' ends and the shifts leave there: nothing), agents
    within a few cells of one another so that some readings have r - 6 < 0, sight 64, and a reset mask on some envs only."""
    import pmx
    if board == "maze32":
        from pmx import maze_generator
        lay = pmx.Layout.from_text(maze_generator.generate_maze(11, rows=30, cols=15))
        assert (lay.width, lay.height) == (32, 32)
    else:
        lay = pmx.get_layout(board)
    H, W = lay.height, lay.width
    s = [tuple(int(v) for v in lay.starts[i]) for i in range(4)]
    free = [(x, y) for y in range(H) for x in range(W) if not (int(lay.wall_rows[y]) >> x) & 1]
    dist = lambda p, q: abs(p[0] - q[0]) + abs(p[1] - q[1])
    near = lambda target: min(free, key=lambda c: (dist(c, target), c))          # the open cell next to a target (set_state takes no wall)
    # a learner, an enemy at exactly 5 and one at exactly 6 from it, and a second learner far from all three
    far = near((W - 2, H - 2))
    a, e5, e6 = next((a, b, c) for a in free for b in free for c in free
                     if dist(a, b) == 5 and dist(a, c) == 6 and min(dist(far, a), dist(far, b), dist(far, c)) > 8)
    mid = near((W // 2, H // 2))
    corners = [near((0, 0)), near((W - 1, H - 1)), near((W - 1, 0)), near((0, H - 1))]            # the outermost open cells
    edges = [near((W - 1, H // 2)), near((0, H // 2)), near((W // 2, H - 1)), near((W // 2, 0))]
    clump = sorted(free, key=lambda c: (dist(c, mid), c))[:4]
    rows = [
        [e5, a, s[2], far],                                        # enemy 0 at distance exactly 5 of learner 1, far from learner 3
        [e6, a, s[2], far],                                        # ... and at 6
        [e5, far, s[2], a],                                        # seen through the second team agent only
        [mid, s[1], mid, s[3]],                                    # both enemies on one cell
        [s[0], mid, s[2], clump[1]],                               # enemies on their own start cells
        corners,
        edges,
        clump,                                                     # everybody within a few cells: readings with r - 6 < 0
        [clump[3], clump[2], clump[1], clump[0]],
        [s[0], s[1], s[2], s[3]],
        [a, e5, far, s[3]],                                        # the first three rows for red learners (0, 2; enemies 1, 3)
        [a, e6, far, s[3]],
    ]
    n = len(rows)
    env = pmx.PmxVecEnv(lay, n, length=300, auto_reset=True, obs_dtype="uint8", seed=SEED)
    env.reset(want_obs=False)
    base = env.get_state(0, 1)[0]
    env.set_state(_hand_states(pmx, env, base, rows))
    ticks = np.array([st.ticks for st in env.get_state()], np.uint32)
    pos = np.array(rows, np.int64)
    P = np.stack([pos, pos], 1)                                    # no tick was run: both slots read the current state
    open_g, starts = _board_arrays(env)
    dev = env.device
    mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    mask[1::3] = 1
    neg = 0
    for red in (False, True):
        for sight, reset in ((5, None), (0, None), (64, None), (5, mask)):
            b = env.belief_init(env.new_belief(), 1)
            assert (_words(b) == R.init(1, open_g, starts)).all()
            sonar = torch.full((n, 2, 2), 99, dtype=torch.int8, device=dev)
            for rep in range(3):                                   # repeated calls: the sets only shrink towards the dilation's reach
                model = _words(b).copy()
                env.belief_update(red, b, sight, reset=reset, sonar=sonar)
                want, readings, seen = R.update(model, P, np.full(n, red), sight, ticks, SEED, np.arange(n), open_g, starts,
                                                reset=None if reset is None else reset.cpu().numpy())
                assert (_words(b) == want).all(), (board, red, sight, rep)
                assert (sonar.cpu().numpy() == readings).all(), (board, red, sight, rep)
                neg += int((readings - 6 < 0).sum())
                cells = R.unpack(want)
                if sight == 64:
                    assert (cells.sum((-1, -2)) == 1).all() and seen.all()
                if reset is None and sight == 5:                   # enemy k = 0: agent 0 for blue learners, agent 1 for red ones
                    r5, r6 = (10, 11) if red else (0, 1)
                    assert seen[r5, :, 0].all() and not seen[r6, :, 0].any() and (seen[2, :, 0].all() or red)
                    assert (cells[r5, :, 0].sum((-1, -2)) == 1).all()
    assert neg > 0
    env.close()


def test_argument_errors():
    import pmx
    from pmx import _lib
    n = 5
    env = pmx.PmxVecEnv("tinyCapture", n, obs_dtype="uint8", seed=1)
    env.reset(want_obs=False)
    lib = _lib.load()
    st = _lib.stream(env.device)
    b = env.belief_init(env.new_belief(), 0)
    keep = b.clone()
    team = _Canary(n, (2,) + env.obs_shape, torch.uint8)
    red = torch.ones(n, dtype=torch.uint8, device="cuda")
    INVALID = -1
    for sight in (-1, 65):
        assert lib.pmx_belief_update(env.handle, 1, None, 0, n, sight, None, b.data_ptr(), None, st) == INVALID
        assert b"pmx_belief_update: sight_range" in lib.pmx_last_error()
    for first, count in ((-1, 2), (0, -1), (0, n + 1), (n, 1), (3, 3)):
        assert lib.pmx_belief_update(env.handle, 1, None, first, count, 5, None, b.data_ptr(), None, st) == INVALID
        assert b"pmx_belief_update: envs" in lib.pmx_last_error()
        assert lib.pmx_belief_init(env.handle, first, count, 0, b.data_ptr(), st) == INVALID
        assert lib.pmx_emit_team_obs_mixed_belief(env.handle, red.data_ptr(), first, count, b.data_ptr(), team.out.data_ptr(), None, st) == INVALID
    assert lib.pmx_belief_init(env.handle, 0, n, 2, b.data_ptr(), st) == INVALID
    assert lib.pmx_belief_update(env.handle, 1, None, 0, n, 5, None, None, None, st) == INVALID
    assert lib.pmx_emit_team_obs_belief(env.handle, 1, None, team.out.data_ptr(), None, st) == INVALID
    for first in (0, 2, n):                                        # an empty range is fine and launches nothing
        assert lib.pmx_belief_update(env.handle, 1, None, first, 0, 5, None, b.data_ptr(), None, st) == 0
        assert lib.pmx_belief_init(env.handle, first, 0, 1, b.data_ptr(), st) == 0
        assert lib.pmx_emit_team_obs_mixed_belief(env.handle, red.data_ptr(), first, 0, b.data_ptr(), team.out.data_ptr(), None, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(b, keep) and team.untouched(0)              # none of the calls above wrote a word
    with pytest.raises(_lib.PmxError, match="pmx_belief_update"):
        env.belief_update(True, b, 65)
    env.profile_begin(4)                                           # the tracker is recorded with the rule launches
    env.belief_update(True, b, 5)
    prof = env.profile_end()
    assert prof["rule_launches"] == 1 and prof["rule_ms"] > 0
    env.close()
