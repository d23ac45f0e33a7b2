"""pmx_step stores plane 0 (the walls) from extra blocks of the rule launch and starts pmx_expand_kernel behind it.

What is new with that split, against the CPU oracle on identical random actions and element for element: every byte of
the caller's buffer is written at every tick (the buffer is filled with a poison value before each step), by the kernel
that owns it (the vector that plane 0 shares with plane 1 belongs to the expansion), for boards whose wall plane ends at
different offsets into a 16-byte vector, for env counts that are ragged for the rule wave and the expansion block, for a
subset of emitted agents and for per-env layouts; and the cases that keep the full expansion (bfloat16 and uint8 planes,
redraw_layouts, an open profile, no observation pointer).  The split is used for float32 planes only (bfloat16 planes
measured slower with it); the bfloat16 cases stay, as the neighbouring path that must not change."""
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


def _actions(N, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 5, size=(N, 4)).astype(np.int8) for _ in range(T)]


def _record(orc, acts, N, H, W):
    """the oracle's planes of all four agents at every tick, as bytes (20 ticks: no element exceeds 1 + 20 pellets)"""
    oobs = np.zeros((N, 4, 8, H, W), np.float32)
    out = []
    for a in acts:
        orc.tick(a, oobs)
        assert oobs.max() <= 255 and (oobs == np.floor(oobs)).all()
        out.append(oobs.astype(np.uint8))
    return out


@functools.lru_cache(maxsize=4)
def _reference(board, N):
    """(actions, oracle planes per tick) of one layout; shared by the element types and agent subsets of that board"""
    rows = list(_rows(board))
    H, W = len(rows), len(rows[0])
    acts = _actions(N, 1000 + N)
    return acts, _record(O.BatchEnv(rows, N, length=60, auto_reset=True, seed=3), acts, N, H, W)


@functools.lru_cache(maxsize=1)
def _reference_mazes(N):
    pool = [list(r) for r in _maze_pool()]
    index = (np.arange(N) % len(pool)).astype(np.int32)
    acts = _actions(N, 77)
    return acts, index, _record(O.MultiBatchEnv(pool, index, length=60, auto_reset=True, seed=3), acts, N, 20, 20)


def _poison(env):
    env.obs.fill_(POISON)


def _check_ticks(env, acts, ref, agents=(0, 1, 2, 3)):
    """poison, step, compare all elements of all envs with the oracle's planes of the emitted agents"""
    for t, a in enumerate(acts):
        _poison(env)
        obs = env.step(torch.tensor(a).cuda())[0]
        got = obs.float().cpu().numpy()
        want = ref[t][:, list(agents)].astype(np.float32)
        assert got.shape == want.shape
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"t={t}: {len(bad)} elements differ, first (env, slot, plane, y, x) = {bad[0]}, got {got[tuple(bad[0])]}"


# 16-byte vectors of plane 0: smallCapture float32 38.5 (ends 8 bytes into a vector), bfloat16 19.25 (4 bytes); tinyCapture
# float32 35 exactly, bfloat16 17.5; 14 x 15 float32 52.5; 30 x 15 bfloat16 56.25; 8 x 5 float32 10 (less than one store
# instruction of the wall writer); 32 x 32 float32 256, the most a wave stores (four instructions); 30 x 15 float32 112.5: the
# expansion loop starts beyond its first 64 lanes' worth of vectors, inside a vector.  bfloat16 and uint8 planes keep the full
# expansion.
CASES = [("smallCapture", "float32"), ("smallCapture", "bfloat16"), ("smallCapture", "uint8"), ("tinyCapture", "float32"),
         ("tinyCapture", "bfloat16"), ("maze14x15", "float32"), ("maze30x15", "bfloat16"), ("board8x5", "float32"),
         ("maze32x32", "float32"), ("maze30x15", "float32")]


@pytest.mark.parametrize("N", [1, 70, 128])
@pytest.mark.parametrize("board,dtype", CASES)
def test_every_byte_written_every_tick(board, dtype, N):
    pmx = _pmx()
    rows = list(_rows(board))
    acts, ref = _reference(board, N)
    env = pmx.PmxVecEnv(pmx.Layout.from_text(rows), N, length=60, auto_reset=True, obs_dtype=dtype, seed=3)
    env.reset()
    _check_ticks(env, acts, ref)
    env.close()


@pytest.mark.parametrize("agents", [(1, 3), (0,)])
def test_fewer_emitted_agents(agents):
    pmx = _pmx()
    N = 70
    rows = list(_rows("smallCapture"))
    acts, ref = _reference("smallCapture", N)
    env = pmx.PmxVecEnv(pmx.Layout.from_text(rows), N, length=60, auto_reset=True, obs_agents=agents, seed=3)
    assert env.obs.shape[1] == len(agents)
    env.reset()
    _check_ticks(env, acts, ref, agents)
    env.close()


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_per_env_layouts_carry_their_own_walls(dtype):
    pmx = _pmx()
    N = 70
    acts, index, ref = _reference_mazes(N)
    walls = [ref[0][e, 0, 0].tobytes() for e in range(5)]
    assert len(set(walls)) == 5                                     # five distinct wall planes
    lays = [pmx.Layout.from_text(list(r)) for r in _maze_pool()]
    env = pmx.PmxVecEnv(lays, N, length=60, auto_reset=True, obs_dtype=dtype, seed=3, layout_index=index)
    env.reset()
    _check_ticks(env, acts, ref)
    env.close()


def _redraw_index(seed, env, ticks, n):
    """include/pmx.h redraw_layouts: the counter-based draw, restated in Python."""
    M = 0xFFFFFFFF
    x = ((seed ^ ((env * 0x9E3779B1) & M)) ^ ((ticks * 0x85EBCA77) & M) ^ 0x4C41594F) & M
    x ^= x >> 16; x = (x * 0x7FEB352D) & M; x ^= x >> 15; x = (x * 0x846CA68B) & M; x ^= x >> 16
    return (x * n) >> 32


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_redraw_keeps_the_full_expansion(dtype):
    """length=6: every env resets, and moves to another maze inside the rule kernel, three times within the 20 ticks"""
    pmx = _pmx()
    N, seed = 70, 21
    pool = [list(r) for r in _maze_pool()]
    lays = [pmx.Layout.from_text(r) for r in pool]
    index = (np.arange(N) % 5).astype(np.int32)
    env = pmx.PmxVecEnv(lays, N, length=6, auto_reset=True, obs_dtype=dtype, seed=seed, layout_index=index, redraw_layouts=True)
    env.reset()                                                     # reset() itself draws
    start = np.array([_redraw_index(seed, e, 0, 5) for e in range(N)], np.int32)
    orc = O.MultiBatchEnv(pool, start.copy(), length=6, auto_reset=True, seed=seed, redraw=True)
    acts = _actions(N, 78)
    oobs = np.zeros((N, 4, 8, 20, 20), np.float32)
    moved = np.zeros(N, np.int64)
    for t, a in enumerate(acts):
        before = orc.index.copy()
        orc.tick(a, oobs)
        moved += before != orc.index
        _poison(env)
        got = env.step(torch.tensor(a).cuda())[0].float().cpu().numpy()
        bad = np.argwhere(got != oobs)
        assert len(bad) == 0, f"t={t}: {len(bad)} elements differ, first {bad[0]}"
    assert moved.sum() > N                                          # the resets moved the envs to other mazes
    env.close()


@pytest.mark.parametrize("dtype", ["float32", "uint8"])
def test_want_obs_false_writes_nothing(dtype):
    pmx = _pmx()
    N = 70
    acts, _ = _reference("smallCapture", N)
    env = pmx.PmxVecEnv("smallCapture", N, length=60, auto_reset=True, obs_dtype=dtype, seed=3)
    env.reset()
    for a in acts[:3]:
        _poison(env)
        env.step(torch.tensor(a).cuda(), want_obs=False)
        assert bool((env.obs == POISON).all())
    env.close()


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_open_profile_does_not_change_results(dtype):
    pmx = _pmx()
    N = 70
    acts, ref = _reference("smallCapture", N)
    plain = pmx.PmxVecEnv("smallCapture", N, length=60, auto_reset=True, obs_dtype=dtype, seed=3)
    prof = pmx.PmxVecEnv("smallCapture", N, length=60, auto_reset=True, obs_dtype=dtype, seed=3)
    plain.reset()
    prof.reset()
    prof.profile_begin(T + 8)
    for t, a in enumerate(acts):
        _poison(plain)
        _poison(prof)
        x = plain.step(torch.tensor(a).cuda())[0]
        y = prof.step(torch.tensor(a).cuda())[0]
        assert torch.equal(x, y), t
        assert (y.float().cpu().numpy() == ref[t].astype(np.float32)).all(), t
    p = prof.profile_end()
    assert p["rule_launches"] == T and p["expand_launches"] == T
    plain.close()
    prof.close()
