"""pmx_emit_team_obs_fog / pmx_emit_team_obs_mixed_fog against trainer.fog_obs of the non-fog emission (which tests/test_gpu_parity.py
pins to the oracle, and tests/test_fog_cpu.py pins fog_obs to the reference's makeObservation): the learners' rows bit for bit,
the merged row untouched by the rule.  Mid-game states of three boards and of a per-env-maze batch, compared after set_state
and after each of six ticks (so the two learners read different snapshots), 128 envs (the kernel's block remap) and 37 (a ragged
last block), three element types, both colours, the per-env-colour entry over a full and a partial range; canary bands around
every output; two hand-built batches for the team rule and for an enemy that moves between the learners' sub-steps."""
import functools

import numpy as np
import pytest
import torch

import _midgame as M

pytestmark = pytest.mark.gpu

BOARDS = ("smallCapture", "tinyCapture", "bloxCapture", "mazes21")
N_MAZES = 8
TICKS = 6
PAD = 2                                                          # canary rows on either side of an output
MIXED_RANGES = ((0, None), (5, 29))
SIGHT = 5


@functools.lru_cache(maxsize=None)
def _maze_rows(k):
    """generated maze k (20 x 20) with the column left of the middle doubled: 21 x 20, an odd width (as tests/test_gpu_mixed_emit.py)"""
    from pmx import maze_generator
    rows = maze_generator.generate_maze(k + 1).split("\n")
    c = len(rows[0]) // 2 - 1
    rows = tuple(r[:c] + r[c] + r[c:] for r in rows)
    assert len(rows[0]) == 21 and len(rows) == 20
    return rows


@functools.lru_cache(maxsize=None)
def _start(board, N):
    if board == "mazes21":                                       # env e plays maze e % N_MAZES: its states are drawn on that maze
        per = [M.random_states(_maze_rows(k), (N + N_MAZES - 1) // N_MAZES, M.STATE_SEED + k) for k in range(N_MAZES)]
        states = [per[e % N_MAZES][e // N_MAZES] for e in range(N)]
    else:
        states = M.start_states(board, N)                        # the reference-made states of the board's scen_*_random fixture
    states = [M._copy(s) for s in states]
    for e in range(0, N, 7):
        states[e].steps = M.LENGTH - 3                           # an auto-reset within TICKS
    return tuple(states)


def _env(pmx, board, N, dtype):
    if board == "mazes21":
        lay = [pmx.Layout.from_text("\n".join(_maze_rows(k))) for k in range(N_MAZES)]
        return pmx.PmxVecEnv(lay, N, length=M.LENGTH, auto_reset=True, obs_dtype=dtype, seed=3, layout_index=np.arange(N) % N_MAZES)
    return pmx.PmxVecEnv(board, N, length=M.LENGTH, auto_reset=True, obs_dtype=dtype, seed=3)


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
        """the bands, and the rows from `written` on, hold what they were filled with"""
        written = self.rows if written is None else written
        now, per = _bytes(self.buf), _bytes(self.buf[0]).numel()
        a, b = PAD * per, (PAD + written) * per
        return torch.equal(now.flatten()[:a], self.was.flatten()[:a]) and torch.equal(now.flatten()[b:], self.was.flatten()[b:])


class _Shares:
    """what the compared learner rows held, from the NON-fog planes: enemy cells seen / hidden at sight 5, and at distance 5 / 6"""

    def __init__(self):
        self.enemy = self.seen = self.d5 = self.d6 = 0

    def add(self, team):
        from pmx import trainer
        n = [int((trainer.fog_obs(team, s)[..., 5, :, :] != 0).sum()) for s in (4, 5, 6)]
        self.enemy += int((team[..., 5, :, :] != 0).sum())
        self.seen += n[1]
        self.d5 += n[1] - n[0]
        self.d6 += n[2] - n[1]

    def check(self, where):
        assert self.enemy > 0, where
        assert self.seen >= 0.15 * self.enemy and self.enemy - self.seen >= 0.15 * self.enemy, (where, self.seen, self.enemy)
        assert self.d5 > 0 and self.d6 > 0, (where, self.d5, self.d6)


def _compare(env, N, colour, shares, where):
    from pmx import trainer
    dt, shape = env.obs_torch_dtype, env.obs_shape
    fog_rows = {}
    for red in (False, True):
        team = torch.empty((N, 2) + shape, dtype=dt, device="cuda")
        merged = torch.empty((N,) + shape, dtype=dt, device="cuda")
        env.emit_team_obs(red, team, merged)
        shares.add(team)
        want = trainer.fog_obs(team, SIGHT)
        ft, fm = _Canary(N, (2,) + shape, dt), _Canary(N, shape, dt)
        env.emit_team_obs(red, ft.out, fm.out, sight_range=SIGHT)
        assert torch.equal(_bytes(ft.out), _bytes(want)), (where, red)
        assert torch.equal(_bytes(fm.out), _bytes(merged)), (where, red)         # nothing is hidden from the critic
        assert ft.untouched() and fm.untouched(), (where, red)
        fog_rows[red] = (ft.out.clone(), merged)
        # merged = NULL: the learners' rows alone
        ft2 = _Canary(N, (2,) + shape, dt)
        env.emit_team_obs(red, ft2.out, None, sight_range=SIGHT)
        assert torch.equal(_bytes(ft2.out), _bytes(want)) and ft2.untouched(), (where, red)
        # sight 62 hides nothing, sight 0 keeps only an enemy on a team cell
        for sight, ref in ((62, team), (64, team), (0, trainer.fog_obs(team, 0))):
            ft3, fm3 = _Canary(N, (2,) + shape, dt), _Canary(N, shape, dt)
            env.emit_team_obs(red, ft3.out, fm3.out, sight_range=sight)
            assert torch.equal(_bytes(ft3.out), _bytes(ref)) and torch.equal(_bytes(fm3.out), _bytes(merged)), (where, red, sight)
            assert ft3.untouched() and fm3.untouched(), (where, red, sight)
        team0 = (team[:, :, 1] != 0) | (team[:, :, 4] != 0)
        assert bool(((trainer.fog_obs(team, 0)[:, :, 5] != 0) <= team0).all())
    # the per-env-colour entry: row e - first is the uniform fog row of env e's colour
    cb = colour.to(torch.bool)
    want_team = torch.where(cb.view(N, 1, 1, 1, 1), fog_rows[True][0], fog_rows[False][0])
    want_merged = torch.where(cb.view(N, 1, 1, 1), fog_rows[True][1], fog_rows[False][1])
    for first, count in MIXED_RANGES:
        count = N - first if count is None else count
        ft, fm = _Canary(N, (2,) + shape, dt), _Canary(N, shape, dt)            # N rows allocated, `count` of them written
        env.emit_team_obs_mixed(colour, ft.out[:count], fm.out[:count], first, count, sight_range=SIGHT)
        assert torch.equal(_bytes(ft.out[:count]), _bytes(want_team[first:first + count])), (where, first, count)
        assert torch.equal(_bytes(fm.out[:count]), _bytes(want_merged[first:first + count])), (where, first, count)
        assert ft.untouched(count) and fm.untouched(count), (where, first, count)
    ft = _Canary(N, (2,) + shape, dt)
    env.emit_team_obs_mixed(colour, ft.out, None, sight_range=62)
    plain = torch.empty((N, 2) + shape, dtype=dt, device="cuda")
    env.emit_team_obs_mixed(colour, plain)
    assert torch.equal(_bytes(ft.out), _bytes(plain)) and ft.untouched(), where


@pytest.mark.parametrize("board", BOARDS)
@pytest.mark.parametrize("dtype", ("float32", "bfloat16", "uint8"))
def test_fog_rows_equal_fog_obs_of_the_plain_emission(dtype, board):
    shares = _Shares()
    for N in (128, 37):                                            # the block remap of a multiple of 128; a ragged last block
        _run(dtype, board, N, shares)
    shares.check((board, dtype))


def _run(dtype, board, N, shares):
    import pmx
    env = _env(pmx, board, N, dtype)
    env.reset(want_obs=False)
    M.load_states(pmx, env, _start(board, N))
    g = torch.Generator().manual_seed(100 + N)
    colour = torch.randint(0, 2, (N,), generator=g).to(torch.uint8)
    colour[0], colour[N - 1] = 1, 0
    colour = colour.cuda()
    _compare(env, N, colour, shares, "set_state")
    rng = np.random.RandomState(M.ACTION_SEED)
    _, legal = env.observe(want_obs=False)
    legal = legal.cpu().numpy()
    n_done = 0
    for t in range(TICKS):
        a = M.mixed_actions(rng, legal, N)
        _, _, done, info = env.step(torch.from_numpy(a).cuda(), want_obs=False)
        legal = info["legal_actions"].cpu().numpy()
        n_done += int(done.sum())
        _compare(env, N, colour, shares, f"tick{t}")               # every tick: the learners' snapshots differ
    assert (N + 6) // 7 <= n_done < TICKS * N                      # auto-resets among the envs, not all of them
    env.close()


def _state(pmx, env, base, pos):
    H, W = env.layout.height, env.layout.width
    pac = [(i in (0, 2)) != (pos[i][0] < W / 2) for i in range(4)]
    return pmx.make_state(pos, [4] * 4, pac, [0] * 4, [0] * 4, [0] * 4, base.food, base.caps, 0, 0, H)


def _cells(plane):
    """[(x, y), ...] of the non-zero cells of one [H, W] plane"""
    return sorted((int(x), int(y)) for y, x in torch.nonzero(plane != 0).cpu().tolist())


@pytest.mark.parametrize("dtype", ("float32", "bfloat16", "uint8"))
def test_the_rule_is_the_teams_and_visibility_is_per_snapshot(dtype):
    """bloxCapture, by hand.  Env 0 is built for blue learners (agents 1, 3), env 1 for red ones (0, 2; their frame is x-flipped).
    Batch A, no tick: an enemy four cells from the SECOND learner and twenty from the first shows in both learners' planes, the
    other enemy in neither.  Batch B, one tick: the enemy that moves between the two learners' sub-steps starts five cells from
    the first learner and steps to six: the first learner's planes (encoded before that move) show it, the second's (after) do
    not, and the merged row, built from the first learner's snapshot, keeps both enemies."""
    import pmx
    env = pmx.PmxVecEnv("bloxCapture", 2, length=300, auto_reset=True, obs_dtype=dtype, seed=1)
    env.reset(want_obs=False)
    base = env.get_state(0, 1)[0]
    W = env.layout.width
    s0, s1, s2, s3 = [tuple(int(v) for v in env.layout.starts[i]) for i in range(4)]
    assert (s0, s1, s2, s3) == ((1, 18), (18, 18), (1, 1), (18, 1))
    shape, dt = env.obs_shape, env.obs_torch_dtype

    def emit(red):
        team = torch.empty((2, 2) + shape, dtype=dt, device="cuda")
        merged = torch.empty((2,) + shape, dtype=dt, device="cuda")
        env.emit_team_obs(red, team, merged, sight_range=SIGHT)
        return team, merged

    # A: blue env: learner 3 at (5, 7), enemy 0 at (9, 7), learner 1 and enemy 2 on their starts; red env: the same with 2 / 1 / 0 / 3
    env.set_state([_state(pmx, env, base, [(9, 7), s1, s2, (5, 7)]), _state(pmx, env, base, [s0, (9, 7), (5, 7), s3])])
    team, merged = emit(False)
    assert _cells(team[0, 0, 5]) == _cells(team[0, 1, 5]) == [(9, 7)] and _cells(merged[0, 5]) == [s2, (9, 7)]
    team, merged = emit(True)
    assert _cells(team[1, 0, 5]) == _cells(team[1, 1, 5]) == [(W - 1 - 9, 7)] and _cells(merged[1, 5]) == sorted([(W - 1 - 9, 7), (W - 1 - 18, 1)])
    # B: the first learner at (5, 7), the mover at (10, 7) stepping East, everybody else on their starts and stopping
    env.set_state([_state(pmx, env, base, [s0, (5, 7), (10, 7), s3]), _state(pmx, env, base, [(5, 7), (10, 7), s2, s3])])
    acts = torch.tensor([[4, 4, 1, 4], [4, 1, 4, 4]], dtype=torch.int8, device="cuda")
    _, _, done, info = env.step(acts, want_obs=False)
    assert not bool(done.any())
    after = env.get_state(0, 2)
    assert (after[0].pos[2][0], after[0].pos[2][1]) == (11, 7) and (after[1].pos[1][0], after[1].pos[1][1]) == (11, 7)
    team, merged = emit(False)
    assert _cells(team[0, 0, 5]) == [(10, 7)] and _cells(team[0, 1, 5]) == [] and _cells(merged[0, 5]) == sorted([s0, (10, 7)])
    team, merged = emit(True)
    assert _cells(team[1, 0, 5]) == [(W - 1 - 10, 7)] and _cells(team[1, 1, 5]) == []
    assert _cells(merged[1, 5]) == sorted([(W - 1 - 10, 7), (W - 1 - 18, 1)])
    # the same through the per-env-colour entry, and without fog nothing is hidden in either slot
    colour = torch.tensor([0, 1], dtype=torch.uint8, device="cuda")
    team = torch.empty((2, 2) + shape, dtype=dt, device="cuda")
    env.emit_team_obs_mixed(colour, team, None, sight_range=SIGHT)
    assert _cells(team[0, 0, 5]) == [(10, 7)] and _cells(team[0, 1, 5]) == [] and _cells(team[1, 0, 5]) == [(W - 1 - 10, 7)] and _cells(team[1, 1, 5]) == []
    env.emit_team_obs_mixed(colour, team)
    assert _cells(team[0, 1, 5]) == sorted([s0, (11, 7)]) and _cells(team[1, 1, 5]) == sorted([(W - 1 - 11, 7), (W - 1 - 18, 1)])
    env.close()


def test_argument_errors():
    import pmx
    from pmx import _lib
    N = 5
    env = pmx.PmxVecEnv("tinyCapture", N, obs_dtype="uint8", seed=1)
    env.reset(want_obs=False)
    lib = _lib.load()
    red = torch.ones(N, dtype=torch.uint8, device="cuda")
    team, merged = _Canary(N, (2,) + env.obs_shape, torch.uint8), _Canary(N, env.obs_shape, torch.uint8)
    st = _lib.stream(env.device)
    INVALID = -1                                                   # PMX_ERR_INVALID
    for sight in (-1, 65, 1000, -2 ** 31):
        assert lib.pmx_emit_team_obs_fog(env.handle, 1, sight, team.out.data_ptr(), merged.out.data_ptr(), st) == INVALID
        assert b"pmx_emit_team_obs_fog: sight_range" in lib.pmx_last_error()
        assert lib.pmx_emit_team_obs_mixed_fog(env.handle, red.data_ptr(), 0, N, sight, team.out.data_ptr(), merged.out.data_ptr(), st) == INVALID
        assert b"pmx_emit_team_obs_mixed_fog: sight_range" in lib.pmx_last_error()
    with pytest.raises(_lib.PmxError, match="pmx_emit_team_obs_fog"):
        env.emit_team_obs(True, team.out, merged.out, sight_range=65)
    with pytest.raises(_lib.PmxError, match="pmx_emit_team_obs_mixed_fog"):
        env.emit_team_obs_mixed(red, team.out, merged.out, sight_range=-1)
    assert lib.pmx_emit_team_obs_fog(None, 1, 5, team.out.data_ptr(), None, st) == INVALID
    assert lib.pmx_emit_team_obs_fog(env.handle, 1, 5, None, None, st) == INVALID
    assert lib.pmx_emit_team_obs_mixed_fog(env.handle, None, 0, N, 5, team.out.data_ptr(), None, st) == INVALID
    assert lib.pmx_emit_team_obs_mixed_fog(env.handle, red.data_ptr(), 0, N, 5, None, None, st) == INVALID
    for first, count in ((-1, 2), (0, -1), (0, N + 1), (N, 1), (3, 3)):
        assert lib.pmx_emit_team_obs_mixed_fog(env.handle, red.data_ptr(), first, count, 5, team.out.data_ptr(), None, st) == INVALID
        assert b"pmx_emit_team_obs_mixed_fog: envs" in lib.pmx_last_error()
    for first in (0, 2, N):                                        # an empty range is fine and launches nothing
        assert lib.pmx_emit_team_obs_mixed_fog(env.handle, red.data_ptr(), first, 0, 5, team.out.data_ptr(), None, st) == 0
    acts = torch.full((N,), 4, dtype=torch.int8, device="cuda")
    env.step_agent(0, acts, want_obs=False)                        # a tick left open: refused like the existing pair
    assert lib.pmx_emit_team_obs_fog(env.handle, 1, 5, team.out.data_ptr(), None, st) == INVALID
    assert lib.pmx_emit_team_obs_mixed_fog(env.handle, red.data_ptr(), 0, N, 5, team.out.data_ptr(), None, st) == INVALID
    torch.cuda.synchronize()
    assert team.untouched(0) and merged.untouched(0)               # none of the calls above wrote a byte
    for a in (1, 2, 3):
        env.step_agent(a, acts, want_obs=False)
    env.emit_team_obs(True, team.out, merged.out, sight_range=5)
    want = torch.empty_like(team.out)
    env.emit_team_obs_mixed(red, want, None, sight_range=5)
    assert torch.equal(team.out, want)
    # the launches are recorded by the profile like the existing ones
    env.profile_begin(8)
    env.emit_team_obs(True, team.out, merged.out, sight_range=5)
    env.emit_team_obs_mixed(red, team.out, None, sight_range=5)
    prof = env.profile_end()
    assert prof["expand_launches"] == 2 and prof["expand_ms"] > 0
    env.close()
