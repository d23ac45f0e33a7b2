"""pmx_set_obs_sight and pmx_agent_distances on the env's own four-agent surfaces (include/pmx.h, "Sight rule on the four-agent
planes").

Planes: every observation a handle with the rule writes -- observe after set_state, six step ticks with an auto-reset inside, two
ticks agent by agent, a masked reset -- equals trainer.fog_obs of a twin handle's plain planes bit for bit (tests/test_fog_cpu.py
pins fog_obs to the reference's makeObservation), at sights 5, 0, 62 and 64, with sights 4 and 6 disagreeing with 5; every other
output of every call, the state and the snapshots equal the twin's.  Three boards and a per-env-maze pool, 128 / 37 / 1 envs, three
element types, an obs_agents subset; canary bands around every output; hand-built rows.  Sonar: the 16 readings against
tests/_agent_distances_ref.py and against pmx_belief_update's."""
import ctypes as C

import numpy as np
import pytest
import torch

import _agent_distances_ref as A
import _midgame as M
from test_gpu_fog_emit import BOARDS, N_MAZES, PAD, TICKS, _Shares, _bytes, _cells, _maze_rows, _start, _state

pytestmark = pytest.mark.gpu

SIGHTS = (5, 0, 62, 64, 4, 6)                                    # compared with fog_obs; 4 and 6 must also differ from 5
STEP_OUTPUTS = ("reward", "done", "legal", "score_change", "score", "agent")
STATE_DTYPE = np.dtype([("pos", "i1", (4, 2)), ("dir", "i1", 4), ("pac", "u1", 4), ("scared", "u1", 4), ("carry", "<u2", 4),
                        ("ret", "<u2", 4), ("food", "<u4", 32), ("caps", "<u4", 32), ("score", "<i4"), ("steps", "<i4"), ("ticks", "<u4")])


class _Band:
    """a tensor of `shape` with PAD rows of 0xA5 bytes before and after it, whatever its element type"""

    def __init__(self, shape, dtype):
        per = int(np.prod(shape[1:], dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full(((shape[0] + 2 * PAD) * per,), 0xA5, dtype=torch.uint8, device="cuda")
        self.lo, self.hi = PAD * per, (PAD + shape[0]) * per
        self.out = self.raw[self.lo:self.hi].view(dtype).view(shape)

    def untouched(self):
        return bool((self.raw[:self.lo] == 0xA5).all()) and bool((self.raw[self.hi:] == 0xA5).all())


def _band_outputs(env):
    """the env's own output tensors replaced by banded ones, so that every call through the class writes between canaries"""
    bands = {}
    for name in ("obs",) + STEP_OUTPUTS:
        t = getattr(env, name)
        bands[name] = _Band(tuple(t.shape), t.dtype)
        setattr(env, name, bands[name].out)
    bands["agent_obs"] = _Band((4, env.n_envs) + env.obs_shape, env.obs_torch_dtype)
    env._agent_obs = bands["agent_obs"].out
    return bands


def _untouched(bands):
    return all(b.untouched() for b in bands.values())


def _make(pmx, board, N, dtype, obs_agents=(0, 1, 2, 3), **kw):
    if board == "mazes21":
        lay = [pmx.Layout.from_text("\n".join(_maze_rows(k))) for k in range(N_MAZES)]
        env = pmx.PmxVecEnv(lay, N, length=M.LENGTH, auto_reset=True, obs_dtype=dtype, seed=3, layout_index=np.arange(N) % N_MAZES,
                            obs_agents=obs_agents, **kw)
    else:
        env = pmx.PmxVecEnv(board, N, length=M.LENGTH, auto_reset=True, obs_dtype=dtype, seed=3, obs_agents=obs_agents, **kw)
    bands = _band_outputs(env)
    env.reset(want_obs=False)
    M.load_states(pmx, env, _start(board, N))
    return env, bands


def _state_bytes(env):
    return bytes(env.get_state())


def _snapshots(env):
    """what pmx_emit_team_obs reads (the sub-step snapshots and the state), for both colours"""
    out = []
    for red in (False, True):
        team = torch.empty((env.n_envs, 2) + env.obs_shape, dtype=env.obs_torch_dtype, device="cuda")
        merged = torch.empty((env.n_envs,) + env.obs_shape, dtype=env.obs_torch_dtype, device="cuda")
        env.emit_team_obs(red, team, merged)
        out += [team, merged]
    return out


def _same_outputs(a, b, names=STEP_OUTPUTS):
    return all(torch.equal(_bytes(getattr(a, n)), _bytes(getattr(b, n))) for n in names)


class _Differs:
    """whether sight 4 / sight 6 planes ever differed from the sight 5 planes of the same call"""

    def __init__(self):
        self.d4 = self.d6 = False

    def add(self, obs):
        self.d4 |= not torch.equal(_bytes(obs[4]), _bytes(obs[5]))
        self.d6 |= not torch.equal(_bytes(obs[6]), _bytes(obs[5]))


def _run(pmx, trainer, dtype, board, N, obs_agents, shares, differs):
    plain, pb = _make(pmx, board, N, dtype, obs_agents)
    envs = {s: _make(pmx, board, N, dtype, obs_agents) for s in SIGHTS}
    where = (board, dtype, N)
    full = envs[5][0]                                              # the handle whose every output is compared
    all_bands = [pb] + [b for _, b in envs.values()]

    def compare_planes(get, plain_obs, tag):
        got = {}
        for s, (env, _) in envs.items():
            got[s] = get(env).clone()
            assert torch.equal(_bytes(got[s]), _bytes(trainer.fog_obs(plain_obs, s))), (where, tag, s)
        assert torch.equal(_bytes(got[62]), _bytes(plain_obs)) and torch.equal(_bytes(got[64]), _bytes(plain_obs)), (where, tag)
        shares.add(plain_obs)
        differs.add(got)

    # observe after set_state: the plain planes come from the same handle with the rule off, which is the twin's call
    before = _state_bytes(full)
    plain_obs = plain.observe()[0].clone()
    off = full.observe()[0].clone()
    assert torch.equal(_bytes(off), _bytes(plain_obs)), where
    for s, (env, _) in envs.items():
        env.set_obs_sight(s)
    compare_planes(lambda e: e.observe()[0], plain_obs, "observe")
    assert _same_outputs(full, plain, ("legal",)) and _state_bytes(full) == before, where

    # six ticks of pmx_step with an auto-reset inside
    rng = np.random.RandomState(M.ACTION_SEED)
    legal = plain.legal.cpu().numpy()
    n_done = 0
    for t in range(TICKS):
        a = torch.from_numpy(M.mixed_actions(rng, legal, N)).cuda()
        plain_obs = plain.step(a)[0].clone()
        compare_planes(lambda e: e.step(a)[0], plain_obs, f"tick{t}")
        assert _same_outputs(full, plain), (where, t)
        assert _state_bytes(full) == _state_bytes(plain), (where, t)
        assert all(torch.equal(_bytes(x), _bytes(y)) for x, y in zip(_snapshots(full), _snapshots(plain))), (where, t)
        assert not full.last_step_fused()
        legal = plain.legal.cpu().numpy()
        n_done += int(plain.done.sum())
    assert (N + 6) // 7 <= n_done < TICKS * N or N == 1, where      # auto-resets among the envs, not all of them

    # two ticks agent by agent: each agent's planes right after its own sub-step, the tick outputs at agent 3
    for t in range(2):
        a = torch.from_numpy(M.mixed_actions(rng, legal, N)).cuda()
        for i in range(4):
            plain_obs = plain.step_agent(i, a[:, i].contiguous()).clone()
            compare_planes(lambda e: e.step_agent(i, a[:, i].contiguous()), plain_obs, f"agent{t}.{i}")
            assert _state_bytes(full) == _state_bytes(plain), (where, t, i)
        assert _same_outputs(full, plain), (where, t)
        legal = plain.legal.cpu().numpy()

    # a masked reset: the planes of ALL envs from their current state
    mask = (torch.arange(N) % 3 == 0).to(torch.uint8).cuda()
    plain_obs = plain.reset(mask)[0].clone()
    compare_planes(lambda e: e.reset(mask)[0], plain_obs, "reset")
    assert _same_outputs(full, plain, ("legal",)) and _state_bytes(full) == _state_bytes(plain), where

    torch.cuda.synchronize()
    assert all(_untouched(b) for b in all_bands), where
    plain.close()
    for env, _ in envs.values():
        env.close()


@pytest.mark.parametrize("board", BOARDS)
@pytest.mark.parametrize("dtype", ("float32", "bfloat16", "uint8"))
def test_planes_equal_fog_obs_of_the_twins_planes(dtype, board):
    import pmx
    from pmx import trainer
    shares, differs = _Shares(), _Differs()
    for N in (128, 37, 1):                                         # the block remap; a ragged last block; one env
        _run(pmx, trainer, dtype, board, N, (0, 1, 2, 3), shares, differs)
    shares.check((board, dtype))                                   # >= 15 % seen, >= 15 % hidden, enemies at distance 5 and at 6
    assert differs.d4 and differs.d6, (board, dtype)


@pytest.mark.parametrize("dtype", ("float32", "uint8"))
def test_planes_of_an_obs_agents_subset(dtype):
    """obs_agents 0b1010: the blue pair alone, two blocks per env (uint8: not the four-agent kernel's shape either way)"""
    import pmx
    from pmx import trainer
    shares, differs = _Shares(), _Differs()
    for N in (128, 37):
        _run(pmx, trainer, dtype, "smallCapture", N, (1, 3), shares, differs)
    shares.check(("subset", dtype))
    assert differs.d4 and differs.d6


@pytest.mark.parametrize("dtype", ("float32", "bfloat16", "uint8"))
def test_hand_built_rows(dtype):
    """bloxCapture (starts (1, 18), (18, 18), (1, 1), (18, 1)), by hand; plane 5 of agent i as a list of cells."""
    import pmx
    env = pmx.PmxVecEnv("bloxCapture", 6, length=300, auto_reset=True, obs_dtype=dtype, seed=1)
    env.reset(want_obs=False)
    base = env.get_state(0, 1)[0]
    s0, s1, s2, s3 = [tuple(int(v) for v in env.layout.starts[i]) for i in range(4)]
    assert (s0, s1, s2, s3) == ((1, 18), (18, 18), (1, 1), (18, 1))
    rows = [
        [(9, 7), s1, s2, (5, 7)],            # 0: enemy 0 four cells from agent 3, far from agent 1: seen by the mate only
        [(5, 7), (10, 7), s2, s3],           # 1: enemy 1 exactly `sight` from agent 0
        [(5, 7), (11, 7), s2, s3],           # 2: enemy 1 at sight + 1 from agent 0, further from agent 2
        [(5, 7), (9, 7), s2, (9, 7)],        # 3: both enemies on one cell, seen
        [(5, 7), (11, 7), s2, (11, 7)],      # 4: both enemies on one cell, hidden
        [(9, 7), (9, 7), s2, (10, 7)],       # 5: an enemy on the observer's cell, the other one step away
    ]
    env.set_state([_state(pmx, env, base, r) for r in rows])
    env.set_obs_sight(5)
    obs = env.observe()[0]
    p5 = lambda e, i: _cells(obs[e, i, 5])
    assert p5(0, 1) == p5(0, 3) == [(9, 7)] and p5(0, 0) == [(5, 7)] and p5(0, 2) == [(5, 7)]      # (agent 3 is four cells from 0)
    assert p5(1, 0) == p5(1, 2) == [(10, 7)]
    assert p5(2, 0) == p5(2, 2) == []
    assert p5(3, 0) == p5(3, 2) == [(9, 7)] and float(obs[3, 0, 5].sum()) == 1.0
    assert p5(4, 0) == p5(4, 2) == []
    assert p5(5, 0) == sorted([(9, 7), (10, 7)])
    env.set_obs_sight(0)
    obs = env.observe()[0]
    assert p5(5, 0) == [(9, 7)] and p5(5, 1) == [(9, 7)] and p5(1, 0) == []
    assert p5(5, 3) == [(9, 7)] and p5(5, 2) == [(9, 7)]           # the rule is the team's: the mate stands on that enemy's cell
    # every other plane is the plain call's
    env.set_obs_sight(None)
    plain = env.observe()[0].clone()
    assert _cells(plain[2, 0, 5]) == sorted([(11, 7), s3])
    env.set_obs_sight(0)
    obs = env.observe()[0]
    keep = [0, 1, 2, 3, 4, 6, 7]
    assert torch.equal(_bytes(obs[:, :, keep]), _bytes(plain[:, :, keep]))
    # the enemy that moves between agent 0's and agent 2's sub-steps: agent 1 steps from five cells to six cells from agent 0
    env.set_state([_state(pmx, env, base, [(5, 7), (10, 7), s2, s3])] * 6)
    env.set_obs_sight(5)
    acts = torch.tensor([[4, 1, 4, 4]] * 6, dtype=torch.int8, device="cuda")
    obs, _, done, _ = env.step(acts)
    assert not bool(done.any())
    after = env.get_state(0, 1)[0]
    assert (after.pos[1][0], after.pos[1][1]) == (11, 7)
    assert p5(0, 0) == [(10, 7)] and p5(0, 2) == []                # agent 0's planes are encoded before the move, agent 2's after
    assert _cells(obs[0, 1, 5]) == [] and _cells(obs[0, 3, 5]) == []   # and blue sees no red agent at six cells
    env.close()


def test_switched_off_again_is_a_handle_never_set_and_the_one_launch_tick_returns():
    import pmx
    from pmx import trainer
    N = 128
    never, nb = _make(pmx, "smallCapture", N, "float32")
    env, eb = _make(pmx, "smallCapture", N, "float32")
    for e in (never, env):
        e.set_tuning("fused_min_envs", 64)
    rng = np.random.RandomState(M.ACTION_SEED)
    legal = never.observe(want_obs=False)[1].cpu().numpy()
    want_fused = []
    for t, sight in enumerate((None, None, 5, 5, None, None)):
        env.set_obs_sight(sight)
        a = torch.from_numpy(M.mixed_actions(rng, legal, N)).cuda()
        plain_obs = never.step(a)[0]
        obs = env.step(a)[0]
        assert never.last_step_fused()
        assert env.last_step_fused() == (sight is None), t
        assert torch.equal(_bytes(obs), _bytes(plain_obs if sight is None else trainer.fog_obs(plain_obs, sight))), t
        assert _same_outputs(env, never) and _state_bytes(env) == _state_bytes(never), t
        assert all(torch.equal(_bytes(x), _bytes(y)) for x, y in zip(_snapshots(env), _snapshots(never))), t
        legal = never.legal.cpu().numpy()
    for name in ("obs",) + STEP_OUTPUTS:                             # after the rule is off again: every byte of every output
        assert torch.equal(_bytes(getattr(env, name)), _bytes(getattr(never, name))), name
    # an open profile records the sight expansion as an expand launch behind the rule launch
    env.set_obs_sight(5)
    env.profile_begin(4)
    env.step(torch.from_numpy(M.mixed_actions(rng, legal, N)).cuda())
    env.agent_distances()
    prof = env.profile_end()
    assert prof["expand_launches"] == 1 and prof["expand_ms"] > 0 and prof["rule_launches"] == 2
    torch.cuda.synchronize()
    assert _untouched(nb) and _untouched(eb)
    never.close()
    env.close()


def test_set_obs_sight_argument_errors():
    import pmx
    from pmx import _lib
    env = pmx.PmxVecEnv("tinyCapture", 3, seed=1)
    lib = _lib.load()
    for bad in (-2, 65, 1000, -2 ** 31):
        assert lib.pmx_set_obs_sight(env.handle, bad) == -1
        assert b"pmx_set_obs_sight: sight_range" in lib.pmx_last_error()
    assert lib.pmx_set_obs_sight(None, 5) == -1
    for ok in (0, 5, 64, _lib.OBS_SIGHT_OFF):
        assert lib.pmx_set_obs_sight(env.handle, ok) == 0
    with pytest.raises(_lib.PmxError, match="pmx_set_obs_sight"):
        env.set_obs_sight(65)
    env.close()


# ---- pmx_agent_distances ------------------------------------------------------------------------------------------------------------
def _np_states(env):
    return np.frombuffer(bytes(env.get_state()), dtype=STATE_DTYPE)


def test_agent_distances_against_the_model_and_the_belief_update():
    import pmx
    from pmx import _lib
    N, T, SEED = 130, 12, 3
    kw = dict(length=M.LENGTH, auto_reset=True, seed=SEED, bots=True)
    env, walk = pmx.PmxVecEnv("smallCapture", N, **kw), pmx.PmxVecEnv("smallCapture", N, **kw)   # `walk` is stepped agent by agent
    for e in (env, walk):
        e.reset(want_obs=False)
        M.load_states(pmx, e, _start("smallCapture", N))
    codes = torch.tensor([[_lib.ACTION_BASELINE_OFFENSE, _lib.ACTION_APPROXQ_OFFENSE, _lib.ACTION_BASELINE_DEFENSE, _lib.ACTION_RANDOM_LEGAL]] * N,
                         dtype=torch.int8, device="cuda")
    ar = np.arange(N)
    belief = {red: env.belief_init(env.new_belief(), 1) for red in (False, True)}
    noise_seen, n_reset = set(), 0
    for t in range(T):
        P = np.zeros((N, 4, 4, 2), np.int64)
        for a in range(4):
            walk.step_agent(a, codes[:, a].contiguous(), want_obs=False)
            st = _np_states(walk)
            P[:, a] = st["pos"]
            # the single-agent form on the current state of the open tick
            band = _Band((N, 4), torch.int8)
            got = walk.agent_distances(a, out=band.out)
            assert (got.cpu().numpy() == A.readings_agent(st["pos"], a, SEED, ar, st["ticks"])).all(), (t, a)
            assert band.untouched() and bytes(walk.get_state()) == st.tobytes(), (t, a)
        _, _, done, _ = env.step(codes, want_obs=False)
        done = done.cpu().numpy().astype(bool)
        st = _np_states(env)
        assert st.tobytes() == _np_states(walk).tobytes(), t        # the two handles play the same game
        P[done] = st["pos"][done][:, None]                          # a finished env shows the fresh game to all four agents
        n_reset += int(done.sum())
        snaps = [x.clone() for x in _snapshots(env)]
        band = _Band((N, 4, 4), torch.int8)
        r = env.agent_distances(out=band.out).cpu().numpy().astype(np.int64)
        assert (r == A.readings(P, SEED, ar, st["ticks"])).all(), t
        assert (env.agent_distances().cpu().numpy() == r).all(), t                # two runs are identical
        torch.cuda.synchronize()
        assert band.untouched(), t
        assert bytes(env.get_state()) == st.tobytes(), t                           # the handle is untouched: state ...
        assert all(torch.equal(x, y) for x, y in zip(_snapshots(env), snaps)), t   # ... and snapshots
        noise_seen |= set((r - np.abs(P - P[:, ar[:4], ar[:4]][:, :, None]).sum(-1)).ravel().tolist())
        for red in (False, True):                                                  # the very draws of pmx_belief_update
            sonar = torch.empty((N, 2, 2), dtype=torch.int8, device="cuda")
            env.belief_update(red, belief[red], 5, reset=torch.from_numpy(done.astype(np.uint8)).cuda(), sonar=sonar)
            sonar = sonar.cpu().numpy()
            first = 0 if red else 1
            for j in range(2):
                for k in range(2):
                    assert (sonar[~done, j, k] == r[~done, first + 2 * j, (1 - first) + 2 * k]).all(), (t, red, j, k)
            assert (sonar[done] == 0).all()
    assert 0 < n_reset < N * T
    assert noise_seen == set(range(-6, 7))
    env.close()
    walk.close()


def test_agent_distances_after_observe_and_reset_and_argument_errors():
    import pmx
    from pmx import _lib
    N, SEED = 37, 11
    env = pmx.PmxVecEnv("tinyCapture", N, length=M.LENGTH, seed=SEED)
    env.reset(want_obs=False)
    M.load_states(pmx, env, _start("tinyCapture", N))
    env.observe()
    st = _np_states(env)
    ar = np.arange(N)
    full = env.agent_distances().cpu().numpy()
    assert (full == A.readings(np.repeat(st["pos"][:, None], 4, 1), SEED, ar, st["ticks"])).all()
    for a in range(4):
        assert (env.agent_distances(a).cpu().numpy() == full[:, a]).all()          # on one state the two forms agree
    env.reset(want_obs=False)
    st = _np_states(env)
    assert (env.agent_distances().cpu().numpy() == A.readings(np.repeat(st["pos"][:, None], 4, 1), SEED, ar, st["ticks"])).all()
    lib = _lib.load()
    out = _Band((N, 4, 4), torch.int8)
    s = _lib.stream(env.device)
    for bad in (-2, 4, 100):
        assert lib.pmx_agent_distances(env.handle, bad, out.out.data_ptr(), s) == -1
        assert b"pmx_agent_distances: agent" in lib.pmx_last_error()
    assert lib.pmx_agent_distances(env.handle, -1, None, s) == -1
    assert lib.pmx_agent_distances(None, -1, out.out.data_ptr(), s) == -1
    assert lib.pmx_agent_distances(env.handle, -1, C.c_void_p(out.out.data_ptr() + 4), s) == -1
    assert b"aligned" in lib.pmx_last_error()
    with pytest.raises(ValueError):
        env.agent_distances(-1)
    torch.cuda.synchronize()
    assert bool((out.raw == 0xA5).all())                                            # none of the refused calls wrote a byte
    env.close()
