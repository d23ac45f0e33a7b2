"""pmx_belief_weights_update / _init and pmx_emit_team_obs_weighted / _mixed_weighted through the C ABI against the numpy model
tests/_belief_weights_ref.py (which tests/test_belief_weights_cpu.py holds to the golden trajectories): every weight, level, set
word and reading at every tick of bot games on five boards; the shapes at which the kernel can still go wrong (ragged blocks,
first > 0, the smallest board, H == 32, W == 32, hand-set rare states, reset rows, no sonar output, canary bands, repeats, the
argument checks); and the weighted emission against the plain and the belief emission in three element types."""
import numpy as np
import pytest
import torch

import _belief_ref as B
import _belief_weights_ref as R
from test_gpu_belief import BOT_CODES, LENGTH, POOL_CODES, SEED, _board_arrays, _bytes, _Canary, _hand_states, _make, _positions, _words

pytestmark = pytest.mark.gpu

N = 96
TICKS = 150
PAD = 2
BOARD_3 = "%%%%%%%%\n%31..24%\n%%%%%%%%"                                               # 8 x 3: one corridor of six cells
BOARD_32 = "\n".join(["%" * 8, "%1.  .2%"] + ["%      %"] * 28 + ["%3.  .4%", "%" * 8])    # 8 x 32: rows 0 and 31 exist


def _u16(t):
    return t.cpu().numpy().view(np.uint16).astype(np.int64)


def _layout(pmx, board):
    from pmx import maze_generator
    if board == "maze32x16":
        lay = pmx.Layout.from_text(maze_generator.generate_maze(5, rows=14, cols=15))
        assert (lay.width, lay.height) == (32, 16)
        return lay
    if board == "board8x3":
        return pmx.Layout.from_text(BOARD_3)
    if board == "board8x32":
        return pmx.Layout.from_text(BOARD_32)
    return pmx.get_layout(board) if board != "mazes" else "mazes"


def _check(tag, env_rows, bel, wts, lev, sn, want_w, want_lev, want_words, readings, H, W):
    n = len(want_w)
    got_w, got_lev = _u16(wts).reshape(n, 2, 2, H, W), lev.cpu().numpy().astype(np.int64).reshape(n, 2, H, W)
    bad = np.nonzero((got_w != want_w).reshape(n, -1).any(1))[0]
    assert len(bad) == 0, (tag, "weights", env_rows[bad[:8]])
    bad = np.nonzero((got_lev != want_lev).reshape(n, -1).any(1))[0]
    assert len(bad) == 0, (tag, "levels", env_rows[bad[:8]])
    assert (_words(bel) == want_words).all(), (tag, "sets")
    if sn is not None:
        assert (sn.cpu().numpy() == readings).all(), (tag, "sonar")


@pytest.mark.parametrize("board", ("smallCapture", "tinyCapture", "bloxCapture", "maze32x16", "mazes"))
def test_every_weight_level_word_and_reading_equals_the_model(board):
    """Two handles with one seed, as tests/test_gpu_belief.py runs them: A steps whole ticks and runs the weighted update, B steps
    agent by agent and supplies the positions after every sub-step.  On a copy of the buffer pmx_belief_update must leave the very
    sets and readings."""
    import pmx
    lay = _layout(pmx, board)
    A, Bh = _make(pmx, lay, N), _make(pmx, lay, N)
    A.reset(want_obs=False)
    Bh.reset(want_obs=False)
    dev = A.device
    H, W = A.layout.height, A.layout.width
    codes = torch.tensor(POOL_CODES if board == "mazes" else BOT_CODES, dtype=torch.int8, device=dev)[None].expand(N, 4).contiguous()
    mixed = (torch.arange(N, device=dev) % 3 == 0).to(torch.uint8)
    cases = [(True, 5), (False, 2), (mixed, 0)] + ([(mixed, 5), (False, 0)] if board == "smallCapture" else [])
    env_idx = np.arange(N)
    open_g, starts = _board_arrays(A)
    bufs, sonars, models = [], [], []
    for _ in cases:
        bufs.append(A.belief_weights_init(A.new_belief(), *A.new_belief_weights(), 0))
        sonars.append(torch.full((N, 2, 2), 99, dtype=torch.int8, device=dev))
        words, w, lv = R.init(0, open_g, starts, H, W)
        models.append((w, words))
        _check((board, "init"), env_idx, *bufs[-1], None, w, lv, words, None, H, W)
    graded = hidden_wide = resets = 0
    for t in range(TICKS):
        A.step(codes, want_obs=False)
        sub = []
        for agent in range(4):
            Bh.step_agent(agent, codes[:, agent].contiguous(), want_obs=False)
            st = Bh.get_state()
            sub.append(_positions(st))
        ticks = np.array([s.ticks for s in st], np.uint32)
        assert torch.equal(A.done, Bh.done)
        done = A.done.cpu().numpy().astype(bool)
        resets += int(done.sum())
        open_g, starts = _board_arrays(A)
        sub_a = np.stack(sub, 1)
        for c, ((colour, sight), (bel, wts, lev), sn) in enumerate(zip(cases, bufs, sonars)):
            plain, plain_sn = bel.clone(), torch.full_like(sn, 98)
            A.belief_weights_update(colour, bel, wts, lev, sight, reset=A.done, sonar=sn)
            A.belief_update(colour, plain, sight, reset=A.done, sonar=plain_sn)
            assert torch.equal(plain, bel) and torch.equal(plain_sn, sn), (board, t, c)
            red = colour.cpu().numpy().astype(bool) if isinstance(colour, torch.Tensor) else np.full(N, colour)
            first = np.where(red, 0, 1)
            P = np.stack([sub_a[env_idx, first], sub_a[env_idx, first + 2]], 1)
            w, lv, words, readings, seen = R.update(*models[c], P, red, sight, ticks, SEED, env_idx, open_g, starts, H, W, reset=done)
            _check((board, t, c), env_idx, bel, wts, lev, sn, w, lv, words, readings, H, W)
            models[c] = (w, words)
            graded += int(((w > 0) & (w < 32768)).sum())
            hidden_wide += int((((w > 0).sum((-1, -2)) > 4) & ~seen).sum())
    print(f"{board}: {graded} weights strictly between 0 and 32768, {hidden_wide} hidden sets of more than four cells, {resets} resets")
    assert resets >= 2 * N and graded > 1000 and hidden_wide > 100
    A.close()
    Bh.close()


class _Band:
    """a tensor of `rows` rows with PAD canary rows before and after it"""

    def __init__(self, rows, row_shape, dtype, device):
        self.buf = torch.full((rows + 2 * PAD,) + row_shape, 0x5A, dtype=dtype, device=device)
        self.out = self.buf[PAD:PAD + rows]
        self.rows = rows

    def untouched(self):
        return bool((self.buf[:PAD] == 0x5A).all()) and bool((self.buf[PAD + self.rows:] == 0x5A).all())


def _hand_rows(lay, rng, sight):
    """positions [rows][4 agents] of open cells: the rare cases first (blue learners 1, 3 with enemies 0, 2; then red learners 0, 2
    with enemies 1, 3), then random ones"""
    H, W = lay.height, lay.width
    s = [tuple(int(v) for v in lay.starts[i]) for i in range(4)]
    free = [(x, y) for y in range(H) for x in range(W) if not (int(lay.wall_rows[y]) >> x) & 1]
    dist = lambda p, q: abs(p[0] - q[0]) + abs(p[1] - q[1])
    far = lambda p: max(free, key=lambda c: (dist(c, p), c))
    a = free[0]
    at = lambda d: next(c for c in free if dist(a, c) == d)
    rows = [
        [at(sight), a, far(a), a],                 # enemy 0 at distance exactly sight of both learners
        [at(sight + 1), a, far(a), a],             # ... and at sight + 1
        [s[0], far(s[0]), s[2], far(s[2])],        # enemies on their own start cells, hidden on every board wider than the sight
        [far(a), a, far(a), a],                    # both enemies on one cell
        [a, at(sight), a, far(a)],                 # the same four for red learners
        [a, at(sight + 1), a, far(a)],
        [far(s[1]), s[1], far(s[3]), s[3]],
        [a, far(a), a, far(a)],
        [s[0], s[1], s[2], s[3]],
    ]
    for _ in range(6):
        rows.append([free[i] for i in rng.randint(0, len(free), 4)])
    return rows


@pytest.mark.parametrize("board", ("board8x3", "board8x32", "bloxCapture", "maze32x16"))
def test_hand_set_states_sub_ranges_and_bands(board):
    """set_state, init (kind 1, then kind 0) and three updates from each against the model, for both colours, sight 2 / 0 / 64 and a
    reset mask; each call on a sub-range of the envs -- 1, 3, 5 rows and the rest, so first > 0 and every raggedness of the last
    block of four waves occur -- with canary bands around the three buffers; sonar_dev NULL on one range; the same call twice on
    copies gives identical bytes.  The smallest board, H == 32 (shuffle ends at rows 0 and 31) and W == 32 (bit 31) are among the
    boards; a hidden enemy whose set is a single cell is counted."""
    import pmx
    lay = _layout(pmx, board)
    H, W = lay.height, lay.width
    sight0 = 2
    rows = _hand_rows(lay, np.random.RandomState(3), sight0)
    n = len(rows)
    env = pmx.PmxVecEnv(lay, n, length=300, auto_reset=True, obs_dtype="uint8", seed=SEED)
    env.reset(want_obs=False)
    base = env.get_state(0, 1)[0]
    env.set_state(_hand_states(pmx, env, base, rows))
    ticks = np.array([st.ticks for st in env.get_state()], np.uint32)
    pos = np.array(rows, np.int64)
    P = np.stack([pos, pos], 1)
    open_g, starts = _board_arrays(env)
    dev = env.device
    mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    mask[1::3] = 1
    ranges = [(0, 1), (1, 3), (4, 5), (9, n - 9)]
    single_hidden = 0
    team = torch.empty((n, 2) + env.obs_shape, dtype=torch.uint8, device=dev)
    for red in (False, True):
        for kind in (1, 0):
            for sight, reset in ((sight0, None), (0, None), (64, None), (sight0, mask)):
                bands = [(_Band(c, (2, 2, 32), torch.int32, dev), _Band(c, (2, 2, H * W), torch.int16, dev), _Band(c, (2, H * W), torch.uint8, dev))
                         for _, c in ranges]
                model = []
                for (f, c), (b, w, l) in zip(ranges, bands):
                    env.belief_weights_init(b.out, w.out, l.out, kind, first=f, count=c)
                    words, mw, ml = R.init(kind, open_g[f:f + c], starts[f:f + c], H, W)
                    _check((board, red, kind, "init", f), np.arange(f, f + c), b.out, w.out, l.out, None, mw, ml, words, None, H, W)
                    model.append((mw, words))
                # an emission straight after the init is valid: plane 5 holds 16 on the initial cells
                lev_all = torch.cat([l.out for _, _, l in bands])
                env.emit_team_obs(red, team, None, levels=lev_all)
                want5 = lev_all.view(n, 2, H, W)
                assert torch.equal(team[:, :, 5], want5.flip(-1) if red else want5) and set(lev_all.unique().tolist()) <= {0, 16}
                for rep in range(3):
                    for i, ((f, c), (b, w, l)) in enumerate(zip(ranges, bands)):
                        sonar = None if i == 1 else torch.full((c, 2, 2), 99, dtype=torch.int8, device=dev)
                        twin = (b.out.clone(), w.out.clone(), l.out.clone())
                        env.belief_weights_update(red, b.out, w.out, l.out, sight, reset=reset, first=f, count=c, sonar=sonar)
                        env.belief_weights_update(red, *twin, sight, reset=reset, first=f, count=c)
                        assert all(torch.equal(x, y) for x, y in zip(twin, (b.out, w.out, l.out))), (board, red, kind, sight, rep, f)
                        rs = None if reset is None else reset.cpu().numpy()[f:f + c]
                        mw, ml, words, readings, seen = R.update(*model[i], P[f:f + c], np.full(c, red), sight, ticks[f:f + c], SEED,
                                                                 np.arange(f, f + c), open_g[f:f + c], starts[f:f + c], H, W, reset=rs)
                        _check((board, red, kind, sight, rep, f), np.arange(f, f + c), b.out, w.out, l.out, sonar, mw, ml, words, readings, H, W)
                        model[i] = (mw, words)
                        assert b.untouched() and w.untouched() and l.untouched(), (board, red, kind, sight, rep, f)
                        hid = ~seen if rs is None else ~seen & ~rs.astype(bool)[:, None, None]
                        single_hidden += int((((mw > 0).sum((-1, -2)) == 1) & hid).sum())
                        if sight == 64:
                            assert seen.all() and ((mw == 65535).sum((-1, -2)) == 1).all() and ((mw > 0).sum((-1, -2)) == 1).all()
    print(f"{board}: {single_hidden} hidden enemies with a set of one cell")
    assert single_hidden > 0
    env.close()


def test_argument_errors():
    import pmx
    from pmx import _lib
    n = 5
    env = pmx.PmxVecEnv("tinyCapture", n, obs_dtype="uint8", seed=1)
    env.reset(want_obs=False)
    lib = _lib.load()
    st = _lib.stream(env.device)
    b, w, l = env.belief_weights_init(env.new_belief(), *env.new_belief_weights(), 0)
    keep = (b.clone(), w.clone(), l.clone())
    team = _Canary(n, (2,) + env.obs_shape, torch.uint8)
    red = torch.ones(n, dtype=torch.uint8, device="cuda")
    bp, wp, lp, tp = b.data_ptr(), w.data_ptr(), l.data_ptr(), team.out.data_ptr()
    INVALID = -1
    for sight in (-1, 65):
        assert lib.pmx_belief_weights_update(env.handle, 1, None, 0, n, sight, None, bp, None, wp, lp, st) == INVALID
        assert b"pmx_belief_weights_update: sight_range" in lib.pmx_last_error()
    for first, count in ((-1, 2), (0, -1), (0, n + 1), (n, 1), (3, 3)):
        assert lib.pmx_belief_weights_update(env.handle, 1, None, first, count, 5, None, bp, None, wp, lp, st) == INVALID
        assert b"pmx_belief_weights_update: envs" in lib.pmx_last_error()
        assert lib.pmx_belief_weights_init(env.handle, first, count, 0, bp, wp, lp, st) == INVALID
        assert b"pmx_belief_weights_init: envs" in lib.pmx_last_error()
        assert lib.pmx_emit_team_obs_mixed_weighted(env.handle, red.data_ptr(), first, count, lp, tp, None, st) == INVALID
        assert b"pmx_emit_team_obs_mixed_weighted: envs" in lib.pmx_last_error()
    assert lib.pmx_belief_weights_init(env.handle, 0, n, 2, bp, wp, lp, st) == INVALID
    assert b"kind 2" in lib.pmx_last_error()
    for args in ((None, wp, lp), (bp, None, lp), (bp, wp, None)):
        assert lib.pmx_belief_weights_update(env.handle, 1, None, 0, n, 5, None, args[0], None, args[1], args[2], st) == INVALID
        assert b"pmx_belief_weights_update: null" in lib.pmx_last_error()
        assert lib.pmx_belief_weights_init(env.handle, 0, n, 0, *args, st) == INVALID
        assert b"pmx_belief_weights_init: null" in lib.pmx_last_error()
    assert lib.pmx_emit_team_obs_weighted(env.handle, 1, None, tp, None, st) == INVALID
    assert lib.pmx_emit_team_obs_weighted(env.handle, 1, lp, None, None, st) == INVALID
    assert lib.pmx_emit_team_obs_mixed_weighted(env.handle, None, 0, n, lp, tp, None, st) == INVALID
    assert lib.pmx_emit_team_obs_mixed_weighted(env.handle, red.data_ptr(), 0, n, None, tp, None, st) == INVALID
    for first in (0, 2, n):                                        # an empty range is fine and launches nothing
        assert lib.pmx_belief_weights_update(env.handle, 1, None, first, 0, 5, None, bp, None, wp, lp, st) == 0
        assert lib.pmx_belief_weights_init(env.handle, first, 0, 1, bp, wp, lp, st) == 0
        assert lib.pmx_emit_team_obs_mixed_weighted(env.handle, red.data_ptr(), first, 0, lp, tp, None, st) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(keep, (b, w, l))) and team.untouched(0)      # none of the calls above wrote
    with pytest.raises(_lib.PmxError, match="pmx_belief_weights_update"):
        env.belief_weights_update(True, b, w, l, 65)
    with pytest.raises(AssertionError):
        env.emit_team_obs(True, team.out, None, levels=l, belief=b)
    with pytest.raises(AssertionError):
        env.emit_team_obs(True, team.out, None, levels=l, sight_range=5)
    with pytest.raises(AssertionError):
        env.emit_team_obs(True, team.out, None, levels=l.to(torch.int8))
    env.profile_begin(4)                                           # recorded with the rule launches, as the set tracker is
    env.belief_weights_update(True, b, w, l, 5)
    prof = env.profile_end()
    assert prof["rule_launches"] == 1 and prof["rule_ms"] > 0
    env.close()


# ---- the emission ---------------------------------------------------------------------------------------------------------------
def _plane5(levels, red, H, W, dt):
    lv = levels.view(len(levels), 2, H, W)
    return torch.where(red.view(-1, 1, 1, 1).to(torch.bool), lv.flip(-1), lv).to(dt)


@pytest.mark.parametrize("board,n", (("smallCapture", 128), ("tinyCapture", 67), ("bloxCapture", 67), ("board8x3", 256)),
                         ids=("small-128", "tiny-67", "blox-67", "8x3-256"))
@pytest.mark.parametrize("dtype", ("float32", "bfloat16", "uint8"))
def test_weighted_emission(dtype, board, n):
    """n % 128 == 0 takes the XCD remap of the blocks, the others a ragged last block; H * W of tinyCapture (140) and of the 8 x 3
    board (24) is no multiple of the 16 elements of a byte vector, so plane 5 starts and ends inside vectors."""
    import pmx
    lay = _layout(pmx, board)
    env = pmx.PmxVecEnv(lay, n, length=LENGTH, auto_reset=True, obs_dtype=dtype, seed=SEED, bots=True)
    env.reset(want_obs=False)
    dev, dt, shape = env.device, env.obs_torch_dtype, env.obs_shape
    H, W = env.layout.height, env.layout.width
    codes = torch.tensor(BOT_CODES, dtype=torch.int8, device=dev)[None].expand(n, 4).contiguous()
    colour = (torch.arange(n, device=dev) % 2).to(torch.uint8)
    new = lambda: env.belief_weights_init(env.new_belief(), *env.new_belief_weights(), 0)
    uni = {red: new() for red in (True, False)}
    mix = new()
    seen_levels = set()
    for t in range(18):
        env.step(codes, want_obs=False)
        for red in (True, False):
            env.belief_weights_update(red, *uni[red], 5, reset=env.done)
        env.belief_weights_update(colour, *mix, 5, reset=env.done)
        if t % 6 != 5:
            continue
        for red in (True, False):
            bel, _, lev = uni[red]
            keep = lev.clone()
            seen_levels |= set(lev.unique().tolist())
            team, merged = torch.empty((n, 2) + shape, dtype=dt, device=dev), torch.empty((n,) + shape, dtype=dt, device=dev)
            env.emit_team_obs(red, team, merged)
            wt, wm = _Canary(n, (2,) + shape, dt), _Canary(n, shape, dt)
            env.emit_team_obs(red, wt.out, wm.out, levels=lev)
            want = team.clone()
            want[:, :, 5] = _plane5(lev, torch.full((n,), int(red), device=dev), H, W, dt)
            assert torch.equal(_bytes(wt.out), _bytes(want)), (t, red)
            assert torch.equal(_bytes(wm.out), _bytes(merged)), (t, red)            # the critic's input: the true enemies
            assert wt.untouched() and wm.untouched() and torch.equal(lev, keep), (t, red)
            wt2 = _Canary(n, (2,) + shape, dt)                                       # merged = NULL
            env.emit_team_obs(red, wt2.out, None, levels=lev)
            assert torch.equal(_bytes(wt2.out), _bytes(wt.out)) and wt2.untouched()
            # levels made of the sets, (set_0 | set_1) != 0: the output is the belief emission's, byte for byte
            cells = torch.from_numpy(B.unpack(_words(bel)).any(2)[:, :, :H, :W].reshape(n, 2, H * W)).to(dev).to(torch.uint8).contiguous()
            bt, bm = torch.empty_like(team), torch.empty_like(merged)
            env.emit_team_obs(red, bt, bm, belief=bel)
            env.emit_team_obs(red, wt.out, wm.out, levels=cells)
            assert torch.equal(_bytes(wt.out), _bytes(bt)) and torch.equal(_bytes(wm.out), _bytes(bm)), (t, red)
        bel, _, lev = mix
        team, merged = torch.empty((n, 2) + shape, dtype=dt, device=dev), torch.empty((n,) + shape, dtype=dt, device=dev)
        env.emit_team_obs_mixed(colour, team, merged)
        for first, count in ((0, n), (5, 29)):
            wt, wm = _Canary(n, (2,) + shape, dt), _Canary(n, shape, dt)
            rows = lev[first:first + count].contiguous()
            env.emit_team_obs_mixed(colour, wt.out[:count], wm.out[:count], first, count, levels=rows)
            want = team[first:first + count].clone()
            want[:, :, 5] = _plane5(rows, colour[first:first + count], H, W, dt)
            assert torch.equal(_bytes(wt.out[:count]), _bytes(want)), (t, first)
            assert torch.equal(_bytes(wm.out[:count]), _bytes(merged[first:first + count])), (t, first)
            assert wt.untouched(count) and wm.untouched(count), (t, first)
            cells = torch.from_numpy(B.unpack(_words(bel[first:first + count])).any(2)[:, :, :H, :W].reshape(count, 2, H * W)).to(dev).to(torch.uint8).contiguous()
            bt = torch.empty_like(want)
            env.emit_team_obs_mixed(colour, bt, None, first, count, belief=bel[first:first + count].contiguous())
            env.emit_team_obs_mixed(colour, wt.out[:count], None, first, count, levels=cells)
            assert torch.equal(_bytes(wt.out[:count]), _bytes(bt)), (t, first)
    if board != "board8x3":                                                           # (sight 5 covers the six-cell corridor: everybody is seen)
        assert len(seen_levels - {0, 16}) >= 3, seen_levels                          # graded levels were emitted, not only 0 and 16
    env.close()
