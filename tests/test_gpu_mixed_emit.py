"""pmx_emit_team_obs_mixed (a colour per env, an env range per launch) against pmx_emit_team_obs, which
tests/test_gpu_parity.py pins to the oracle: every row of a mixed emission is, byte for byte, the same row of the uniform
emission of that env's colour.  Three element types; tinyCapture, smallCapture and one handle with a maze of odd width per
env; after a reset, after set_state of mid-game states (carried food, agents on one cell, scared ghosts) and after ticks
with valid snapshots and auto-reset envs among them; env counts and ranges around the kernel's four-env blocks and its
remap of multiples of 128."""
import functools

import numpy as np
import pytest
import torch

import _midgame as M

pytestmark = pytest.mark.gpu

SENTINEL = 9
# (n_envs, [(first, count), ...]); None = the full range.  70: a partial last block; 128: the remap; (3, 128) of 131: the remap
# inside a range; (130, 1): the last env alone
RANGES = ((1, (None,)), (5, (None,)), (70, (None,)), (128, (None,)), (131, ((3, 128), (1, 66), (130, 1))))
BOARDS = ("tinyCapture", "smallCapture", "mazes21")
N_MAZES = 8
TICKS = 6


@functools.lru_cache(maxsize=None)
def _maze_rows(k):
    """generated maze k (20 x 20, mirrored, so always of even width) with the column left of the middle doubled: 21 x 20"""
    from pmx import maze_generator
    rows = maze_generator.generate_maze(k + 1).split("\n")
    c = len(rows[0]) // 2 - 1
    rows = tuple(r[:c] + r[c] + r[c:] for r in rows)
    assert len(rows[0]) == 21 and len(rows) == 20
    return rows


@functools.lru_cache(maxsize=None)
def _start(board, N):
    """the mid-game states of N envs of `board`, every seventh three steps before its time-out (an auto-reset within TICKS)"""
    if board == "mazes21":          # env e plays maze e % N_MAZES: its states are drawn on that maze
        per = [M.random_states(_maze_rows(k), (N + N_MAZES - 1) // N_MAZES, M.STATE_SEED + k) for k in range(N_MAZES)]
        states = [per[e % N_MAZES][e // N_MAZES] for e in range(N)]
    else:
        states = M.start_states(board, N)
    states = [M._copy(s) for s in states]
    for e in range(0, N, 7):
        states[e].steps = M.LENGTH - 3
    return tuple(states)


def _env(pmx, board, N, dtype):
    if board == "mazes21":
        lay = [pmx.Layout.from_text("\n".join(_maze_rows(k))) for k in range(N_MAZES)]
        return pmx.PmxVecEnv(lay, N, length=M.LENGTH, auto_reset=True, obs_dtype=dtype, seed=3, layout_index=np.arange(N) % N_MAZES)
    return pmx.PmxVecEnv(board, N, length=M.LENGTH, auto_reset=True, obs_dtype=dtype, seed=3)


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _uniform(env, N):
    """the yardstick: {red: (team [N,2,8,H,W], merged [N,8,H,W])} of the uniform entry, and team without the merged slot checked"""
    out = {}
    for red in (False, True):
        team = torch.full((N, 2) + env.obs_shape, SENTINEL, dtype=env.obs_torch_dtype, device="cuda")
        merged = torch.full((N,) + env.obs_shape, SENTINEL, dtype=env.obs_torch_dtype, device="cuda")
        env.emit_team_obs(red, team, merged)
        out[red] = (team, merged)
    return out


def _check(env, N, ranges, colours, tag):
    uni = _uniform(env, N)
    dt, shape = env.obs_torch_dtype, env.obs_shape
    for name, red in colours.items():
        rb = red.to(torch.bool)
        want_team = torch.where(rb.view(N, 1, 1, 1, 1), uni[True][0], uni[False][0])
        want_merged = torch.where(rb.view(N, 1, 1, 1), uni[True][1], uni[False][1])
        for rng in ranges:
            first, count = (0, N) if rng is None else rng
            for with_merged in (True, False):
                # two sentinel rows on either side of the rows the call may write
                team = torch.full((count + 4, 2) + shape, SENTINEL, dtype=dt, device="cuda")
                merged = torch.full((count + 4,) + shape, SENTINEL, dtype=dt, device="cuda")
                if rng is None and with_merged:          # the defaults of the Python surface are the full range
                    env.emit_team_obs_mixed(red, team[2:2 + count], merged[2:2 + count])
                else:
                    env.emit_team_obs_mixed(red, team[2:2 + count], merged[2:2 + count] if with_merged else None, first, count)
                where = (tag, name, rng, with_merged)
                assert torch.equal(_bytes(team[2:2 + count]), _bytes(want_team[first:first + count])), where
                assert bool((team[:2] == SENTINEL).all()) and bool((team[2 + count:] == SENTINEL).all()), where
                if with_merged:
                    assert torch.equal(_bytes(merged[2:2 + count]), _bytes(want_merged[first:first + count])), where
                    assert bool((merged[:2] == SENTINEL).all()) and bool((merged[2 + count:] == SENTINEL).all()), where
                else:
                    assert bool((merged == SENTINEL).all()), where
                # mid-game, the rows do differ between the colours: the comparison above is not one of equal things.  (Not right
                # after a reset: canonicalisation is there to make a mirrored board's start look the same from either side)
                if tag != "reset" and name == "random":
                    assert not torch.equal(_bytes(uni[True][0][first:first + count]), _bytes(uni[False][0][first:first + count])), where


@pytest.mark.parametrize("board", BOARDS)
@pytest.mark.parametrize("dtype", ("float32", "bfloat16", "uint8"))
def test_mixed_rows_equal_the_uniform_emission_of_their_colour(dtype, board):
    import pmx
    for N, ranges in RANGES:
        env = _env(pmx, board, N, dtype)
        g = torch.Generator().manual_seed(100 + N)
        rand = torch.randint(0, 2, (N,), generator=g).to(torch.uint8)
        if N > 1:
            rand[0], rand[N - 1] = 1, 0                       # both colours in every handle of more than one env
        colours = {"random": rand.cuda(), "zeros": torch.zeros(N, dtype=torch.uint8, device="cuda"),
                   "ones": torch.ones(N, dtype=torch.uint8, device="cuda"), "any_nonzero": (rand * 255).cuda()}
        env.reset(want_obs=False)
        _check(env, N, ranges, colours, "reset")
        M.load_states(pmx, env, _start(board, N))
        _check(env, N, ranges, colours, "set_state")
        ga = torch.Generator(device="cuda").manual_seed(7)
        n_done = 0
        for t in range(TICKS):
            _, _, done, _ = env.step(torch.randint(0, 5, (N, 4), generator=ga, device="cuda", dtype=torch.int8), want_obs=False)
            n_done += int(done.sum())
            if t in (0, 2, TICKS - 1):                        # tick 2 is the one the timed-out envs reset in
                _check(env, N, ranges, {"random": colours["random"]}, f"tick{t}")
        assert n_done >= (N + 6) // 7 and (N < 7 or n_done < TICKS * N)      # auto-resets among the envs, not all of them
        env.close()


def test_argument_errors_and_empty_range():
    import pmx
    from pmx import _lib
    N = 5
    env = pmx.PmxVecEnv("tinyCapture", N, obs_dtype="uint8", seed=1)
    env.reset(want_obs=False)
    lib = _lib.load()
    red = torch.ones(N, dtype=torch.uint8, device="cuda")
    team = torch.full((N, 2) + env.obs_shape, SENTINEL, dtype=torch.uint8, device="cuda")
    merged = torch.full((N,) + env.obs_shape, SENTINEL, dtype=torch.uint8, device="cuda")
    st = _lib.stream(env.device)

    def rc(handle, colour, first, count, out):
        return lib.pmx_emit_team_obs_mixed(handle, colour, first, count, out, merged.data_ptr(), st)

    INVALID = -1                                               # PMX_ERR_INVALID
    assert rc(None, red.data_ptr(), 0, N, team.data_ptr()) == INVALID
    assert rc(env.handle, None, 0, N, team.data_ptr()) == INVALID
    assert rc(env.handle, red.data_ptr(), 0, N, None) == INVALID
    assert b"pmx_emit_team_obs_mixed" in lib.pmx_last_error()
    for first, count in ((-1, 2), (0, -1), (0, N + 1), (N, 1), (3, 3), (1, 2 ** 31 - 1)):
        assert rc(env.handle, red.data_ptr(), first, count, team.data_ptr()) == INVALID, (first, count)
    for first in (0, 2, N):                                    # an empty range is fine anywhere inside, and launches nothing
        assert rc(env.handle, red.data_ptr(), first, 0, team.data_ptr()) == 0
    with pytest.raises(AssertionError):
        env.emit_team_obs_mixed(red.to(torch.int32), team)      # the colour vector is bytes
    with pytest.raises(AssertionError):
        env.emit_team_obs_mixed(red, team, merged, 1, 2)        # `count` rows, not N
    env.emit_team_obs_mixed(red, team[:0], merged[:0], 2, 0)
    torch.cuda.synchronize()
    assert bool((team == SENTINEL).all()) and bool((merged == SENTINEL).all())      # none of the calls above wrote a byte
    # a tick left open by pmx_step_agent: refused like the uniform entry, and accepted again once the tick is closed
    acts = torch.full((N,), 4, dtype=torch.int8, device="cuda")
    env.step_agent(0, acts, want_obs=False)
    assert rc(env.handle, red.data_ptr(), 0, N, team.data_ptr()) == INVALID
    with pytest.raises(_lib.PmxError):
        env.emit_team_obs(True, team, merged)
    for a in (1, 2, 3):
        env.step_agent(a, acts, want_obs=False)
    assert rc(env.handle, red.data_ptr(), 0, N, team.data_ptr()) == 0
    want = torch.empty_like(team)
    env.emit_team_obs(True, want, None)
    assert torch.equal(team, want)
    env.close()
