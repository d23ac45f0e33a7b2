"""pmx_step runs the whole tick in ONE launch (pmx_tick_fused_kernel) where a workgroup can own 64 envs from the state load to
the last plane byte; everywhere else it runs the rule and the expansion launch as before.

Against the CPU oracle on identical random actions, element for element, with the caller's buffer poisoned before every step:
the fused path forced at 64 envs (one workgroup) and 192 (three, so the reversed mapping of the alternating sweep has a
middle), on boards whose wall plane ends on a vector boundary (8 x 5), inside a vector (tinyCapture: 35 vectors exactly;
smallCapture: H*W = 154, a vector straddles planes 0 and 1) and in the HB 20 bucket (a 20 x 20 maze), with the sweep fixed and
alternating; a run in which every env finishes and auto-resets several times; the hand-off of the state and the three
snapshots to pmx_observe, pmx_emit_team_obs, pmx_step_agent and the next tick; and every case that must keep the two launches.

observe() after a step: the planes a step returns for agent i are those of the state right after agent i's own sub-step
(gymPacMan.py:149-169), so only agent 3's are the planes of the state the tick leaves.  The hand-off test therefore compares
observe() of the fused handle with agent 3's planes of the step, and all four agents' with observe() of a handle that ran the
two launches on the same actions."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

T = 20
POISON = 7
_TINY_BOARD = ["%%%%%%%%", "%1 .. 2%", "%  ..  %", "%3 .. 4%", "%%%%%%%%"]


def _pmx():
    import pmx
    return pmx


@functools.lru_cache(maxsize=None)
def _rows(board):
    pmx = _pmx()
    from pmx import maze_generator as MG
    if board == "board8x5":
        return tuple(_TINY_BOARD)
    if board.startswith("maze"):                                   # "mazeWxH": the generator mirrors `cols` columns and adds the border
        w, h = (int(v) for v in board[4:].split("x"))
        rows = tuple(MG.generate_maze(11, rows=h - 2, cols=(w - 2) // 2).split("\n"))
        assert (len(rows[0]), len(rows)) == (w, h)
        return rows
    return tuple(pmx.get_layout(board).text)


@functools.lru_cache(maxsize=None)
def _maze_pool():
    from pmx import maze_generator as MG
    return tuple(tuple(MG.generate_maze(300 + k).split("\n")) for k in range(5))


def _actions(N, seed, ticks=T):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 5, size=(N, 4)).astype(np.int8) for _ in range(ticks)]


def _record(orc, acts, N, H, W):
    """everything the oracle returns at every tick (the planes as bytes: no element exceeds 1 + the board's pellets)"""
    oobs = np.zeros((N, 4, 8, H, W), np.float32)
    out = []
    for a in acts:
        orc.tick(a, oobs)
        assert oobs.max() <= 255 and (oobs == np.floor(oobs)).all()
        out.append(dict(obs=oobs.astype(np.uint8), reward=orc.reward.tobytes(), done=orc.done.copy(), legal=orc.legal.copy(),
                        score_change=orc.score_change.copy(), score=orc.score.copy(), agent=orc.agent.copy()))
    return out


@functools.lru_cache(maxsize=None)
def _reference(board, N, length=60):
    """(actions, the oracle's results per tick) of one layout; computed once and shared by the cases of that board"""
    rows = list(_rows(board))
    acts = _actions(N, 1000 + N)
    return acts, _record(O.BatchEnv(rows, N, length=length, auto_reset=True, seed=3), acts, N, len(rows), len(rows[0]))


@functools.lru_cache(maxsize=1)
def _reference_mazes(N):
    pool = [list(r) for r in _maze_pool()]
    index = (np.arange(N) % len(pool)).astype(np.int32)
    acts = _actions(N, 77)
    return acts, index, _record(O.MultiBatchEnv(pool, index, length=60, auto_reset=True, seed=3), acts, N, 20, 20)


def _check_tick(env, a, want, fused, agents=(0, 1, 2, 3), tag=""):
    """poison, step, compare every element of every result with the oracle's; the path the step took"""
    env.obs.fill_(POISON)
    obs, rew, done, info = env.step(torch.tensor(a).cuda())
    assert env.last_step_fused() == fused, tag
    got = obs.float().cpu().numpy()
    ref = want["obs"][:, list(agents)].astype(np.float32)
    assert got.shape == ref.shape
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, f"{tag}: {len(bad)} elements differ, first (env, slot, plane, y, x) = {bad[0]}, got {got[tuple(bad[0])]}"
    assert rew.cpu().numpy().tobytes() == want["reward"], f"{tag} reward"
    assert (done.cpu().numpy() == want["done"]).all(), f"{tag} done"
    assert (info["legal_actions"].cpu().numpy() == want["legal"]).all(), f"{tag} legal"
    assert (info["score_change"].cpu().numpy() == want["score_change"]).all(), f"{tag} score_change"
    assert (info["score"].cpu().numpy() == want["score"]).all(), f"{tag} score"
    assert (info["agent"].cpu().numpy().astype(np.uint32) == want["agent"]).all(), f"{tag} agent words"


def _run(env, acts, ref, fused, agents=(0, 1, 2, 3)):
    env.set_tuning("fused_min_envs", 64)
    env.reset()
    for t, a in enumerate(acts):
        _check_tick(env, a, ref[t], fused, agents, f"t={t}")
    env.close()


# ---- the fused path, forced ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alt", [0, -1])
@pytest.mark.parametrize("N", [64, 192])
@pytest.mark.parametrize("board", ["board8x5", "tinyCapture", "smallCapture", "maze20x20"])
def test_fused_tick_matches_the_oracle(board, N, alt):
    pmx = _pmx()
    acts, ref = _reference(board, N)
    env = pmx.PmxVecEnv(pmx.Layout.from_text(list(_rows(board))), N, length=60, auto_reset=True, seed=3)
    env.set_tuning("expand_alt", alt)
    _run(env, acts, ref, True)


def test_envs_that_finish_show_the_fresh_game():
    """length=5: every env finishes and auto-resets three times within the 20 ticks; all four observations of such a tick are
    the fresh game's (gymPacMan.py:135-137), which is what the oracle returns"""
    pmx = _pmx()
    N = 192
    acts, ref = _reference("smallCapture", N, 5)
    assert sum(int(r["done"].sum()) for r in ref) >= 3 * N
    env = pmx.PmxVecEnv("smallCapture", N, length=5, auto_reset=True, seed=3)
    _run(env, acts, ref, True)


def test_default_threshold_keeps_two_launches_at_64_envs():
    pmx = _pmx()
    N = 64
    acts, ref = _reference("smallCapture", N)
    env = pmx.PmxVecEnv("smallCapture", N, length=60, auto_reset=True, seed=3)
    env.reset()
    assert env.last_step_fused() is False
    _check_tick(env, acts[0], ref[0], False)
    env.close()


# ---- hand-off to the kernels that read the state and the snapshots --------------------------------------------------------------

def _same_results(A, B, tag):
    for name in ("obs", "reward", "done", "legal", "score_change", "score", "agent"):
        assert torch.equal(getattr(A, name), getattr(B, name)), f"{tag} {name}"


@pytest.mark.parametrize("board", ["smallCapture", "maze20x20"])
def test_state_and_snapshots_reach_the_other_kernels(board):
    pmx = _pmx()
    N = 192
    lay = pmx.Layout.from_text(list(_rows(board)))
    acts = _actions(N, 4242, 2 * T + 1)
    F = pmx.PmxVecEnv(lay, N, length=12, auto_reset=True, seed=3)      # length 12: the runs below cross several resets
    P = pmx.PmxVecEnv(lay, N, length=12, auto_reset=True, seed=3)
    F.set_tuning("fused_min_envs", 64)
    P.set_tuning("fused_min_envs", N + 1)
    F.reset()
    P.reset()
    shape = (N, 2) + F.obs_shape
    for t in range(T):
        a = torch.tensor(acts[t]).cuda()
        F.obs.fill_(POISON)
        P.obs.fill_(POISON)
        F.step(a)
        P.step(a)
        assert F.last_step_fused() and not P.last_step_fused()
        _same_results(F, P, f"t={t}")
        if t in (0, 7, 12, T - 1):         # 12: the tick in which every env finishes
            for red in (1, 0):             # pmx_emit_team_obs reads the three snapshots and the state
                tf, mf = F.emit_team_obs(red, torch.full(shape, POISON, dtype=torch.float32, device="cuda"),
                                         torch.full(shape[:1] + shape[2:], POISON, dtype=torch.float32, device="cuda"))
                tp, mp = P.emit_team_obs(red, torch.full(shape, POISON, dtype=torch.float32, device="cuda"),
                                         torch.full(shape[:1] + shape[2:], POISON, dtype=torch.float32, device="cuda"))
                assert torch.equal(tf, tp) and torch.equal(mf, mp), (t, red)
            stepped = F.obs.clone()
            of, lf = F.observe()           # pmx_observe reads the state
            op, lp = P.observe()
            assert torch.equal(of, op) and torch.equal(lf, lp), t
            assert torch.equal(of[:, 3], stepped[:, 3]), t
    sf, sp = F.get_state(), P.get_state()
    assert bytes(sf) == bytes(sp)
    for t in range(T, 2 * T):              # twenty further ticks: the state write-out is complete (score, steps, ticks included)
        a = torch.tensor(acts[t]).cuda()
        F.step(a)
        P.step(a)
        assert F.last_step_fused() and not P.last_step_fused()
        _same_results(F, P, f"t={t}")
    for i in range(4):                     # pmx_step_agent reads the state the fused launch wrote
        a = torch.tensor(acts[2 * T][:, i]).cuda()
        assert torch.equal(F.step_agent(i, a), P.step_agent(i, a)), i
    assert bytes(F.get_state()) == bytes(P.get_state())
    F.close()
    P.close()


# ---- cases that keep the two launches (fused_min_envs = 64 on all of them) -------------------------------------------------------

@pytest.mark.parametrize("dtype", ["bfloat16", "uint8"])
def test_other_element_types_keep_two_launches(dtype):
    pmx = _pmx()
    N = 64
    acts, ref = _reference("smallCapture", N)
    _run(pmx.PmxVecEnv("smallCapture", N, length=60, auto_reset=True, obs_dtype=dtype, seed=3), acts, ref, False)


def test_ragged_env_count_keeps_two_launches():
    pmx = _pmx()
    N = 100
    acts, ref = _reference("smallCapture", N)
    _run(pmx.PmxVecEnv("smallCapture", N, length=60, auto_reset=True, seed=3), acts, ref, False)


def test_agent_subset_keeps_two_launches():
    pmx = _pmx()
    N = 64
    acts, ref = _reference("smallCapture", N)
    env = pmx.PmxVecEnv("smallCapture", N, length=60, auto_reset=True, obs_agents=(1, 3), seed=3)
    assert env.obs.shape[1] == 2
    _run(env, acts, ref, False, (1, 3))


def test_per_env_layouts_keep_two_launches():
    pmx = _pmx()
    N = 64
    acts, index, ref = _reference_mazes(N)
    lays = [pmx.Layout.from_text(list(r)) for r in _maze_pool()]
    _run(pmx.PmxVecEnv(lays, N, length=60, auto_reset=True, seed=3, layout_index=index), acts, ref, False)


def _redraw_index(seed, env, ticks, n):
    """include/pmx.h redraw_layouts: the counter-based draw, restated in Python."""
    M = 0xFFFFFFFF
    x = ((seed ^ ((env * 0x9E3779B1) & M)) ^ ((ticks * 0x85EBCA77) & M) ^ 0x4C41594F) & M
    x ^= x >> 16; x = (x * 0x7FEB352D) & M; x ^= x >> 15; x = (x * 0x846CA68B) & M; x ^= x >> 16
    return (x * n) >> 32


def test_redraw_layouts_keeps_two_launches():
    pmx = _pmx()
    N, seed = 64, 21
    pool = [list(r) for r in _maze_pool()]
    lays = [pmx.Layout.from_text(r) for r in pool]
    env = pmx.PmxVecEnv(lays, N, length=6, auto_reset=True, seed=seed, layout_index=(np.arange(N) % 5).astype(np.int32),
                        redraw_layouts=True)
    start = np.array([_redraw_index(seed, e, 0, 5) for e in range(N)], np.int32)      # reset() itself draws
    acts = _actions(N, 78)
    ref = _record(O.MultiBatchEnv(pool, start.copy(), length=6, auto_reset=True, seed=seed, redraw=True), acts, N, 20, 20)
    _run(env, acts, ref, False)


def test_open_profile_keeps_two_launches():
    pmx = _pmx()
    N = 64
    acts, ref = _reference("smallCapture", N)
    env = pmx.PmxVecEnv("smallCapture", N, length=60, auto_reset=True, seed=3)
    env.set_tuning("fused_min_envs", 64)
    env.reset()
    _check_tick(env, acts[0], ref[0], True, tag="before the profile")
    env.profile_begin(T + 8)
    for t in range(1, T - 1):
        _check_tick(env, acts[t], ref[t], False, tag=f"t={t}")
    p = env.profile_end()
    assert p["rule_launches"] == T - 2 and p["expand_launches"] == T - 2
    _check_tick(env, acts[T - 1], ref[T - 1], True, tag="after the profile")
    env.close()


def test_tall_board_keeps_two_launches():
    pmx = _pmx()
    N = 64
    rows = list(_rows("maze14x22"))
    assert len(rows) > 20
    acts, ref = _reference("maze14x22", N)
    _run(pmx.PmxVecEnv(pmx.Layout.from_text(rows), N, length=60, auto_reset=True, seed=3), acts, ref, False)


def test_bot_tables_keep_two_launches():
    pmx = _pmx()
    N = 64
    acts, ref = _reference("smallCapture", N)
    _run(pmx.PmxVecEnv("smallCapture", N, length=60, auto_reset=True, bots=True, seed=3), acts, ref, False)
