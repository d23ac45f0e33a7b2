"""pmx_episode_stats_init / pmx_episode_stats_update against the plain-Python model tests/_episode_stats_ref.py (which
tests/test_episode_stats_cpu.py pins to the golden trajectories and to oracle-stepped states): every word of every row after every
tick of bot games and raw-code games on three boards and a 48-maze pool, golden episodes replayed from their recorded actions, the
hand-set states of the CPU suite through pmx_set_state, and the contract of the two entry points."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _episode_stats_ref as R
import _golden as G

pytestmark = pytest.mark.gpu

TICKS = 150
LENGTH = 100                 # every env finishes (and its row freezes) inside TICKS
SEED = 11
N_MAZES = 48
# the exchange state (pmx_state, _lib.State) as a numpy record, so that a batch of states unpacks without a Python loop per field
STATE = np.dtype([("pos", np.int8, (4, 2)), ("dir", np.int8, 4), ("pac", np.uint8, 4), ("scared", np.uint8, 4), ("carry", np.uint16, 4),
                  ("ret", np.uint16, 4), ("food", np.uint32, 32), ("caps", np.uint32, 32), ("score", np.int32), ("steps", np.int32),
                  ("ticks", np.uint32)])


@functools.lru_cache(maxsize=None)
def _caps(rows):
    return tuple(R.caps_cells(rows))


def _states(env):
    """the current state of every env -> [R.State]"""
    import pmx
    assert STATE.itemsize == C.sizeof(pmx._lib.State)
    a = np.frombuffer(env.get_state(), dtype=STATE)
    f = {k: a[k].tolist() for k in ("pos", "dir", "pac", "scared", "carry", "ret", "score")}
    caps = [_caps(tuple(r)) for r in a["caps"].tolist()]
    return [R.State(f["pos"][e], f["dir"][e], f["pac"][e], f["scared"][e], f["carry"][e], f["ret"][e], caps[e], f["score"][e])
            for e in range(len(a))]


def _model_words(recs):
    return np.stack([r.words() for r in recs], 1)               # [48, n], the buffer's own order


@functools.lru_cache(maxsize=None)
def _pool():
    from pmx import maze_generator
    return tuple(maze_generator.generate_maze(k + 1) for k in range(N_MAZES))


def _make(pmx, board, n, dtype, bots):
    kw = dict(length=LENGTH, auto_reset=False, obs_dtype=dtype, seed=SEED, bots=bots)
    if board == "mazes":
        return pmx.PmxVecEnv([pmx.Layout.from_text(t) for t in _pool()], n, layout_index=np.arange(n) % N_MAZES, **kw)
    return pmx.PmxVecEnv(board, n, **kw)


# (board, envs, the four action codes or "raw", plane type, bots handle, the expected last_step_fused())
CASES = [("smallCapture", 64, "raw", "float32", False, True),            # one launch per tick: the snapshots of pmx_tick_fused_kernel
         ("tinyCapture", 65, (-3, -3, -4, -4), "uint8", True, False),      # baselineTeam on both sides, a ragged last wave
         ("bloxCapture", 320, (-5, -2, -6, -2), "float32", True, False),   # approxQTeam (red) against randomTeam, five waves
         ("mazes", 64, "raw", "uint8", False, False)]


@pytest.mark.parametrize("board, n, codes, dtype, bots, fused", CASES, ids=[c[0] for c in CASES])
def test_every_word_equals_the_model_after_every_tick(board, n, codes, dtype, bots, fused):
    """Two handles with one seed: A runs pmx_step + pmx_episode_stats_update, B the four pmx_step_agent calls with the same codes (the
    equivalence tests/test_gpu_parity.py pins) and hands its state after every sub-step to the model."""
    import pmx
    A, B = _make(pmx, board, n, dtype, bots), _make(pmx, board, n, dtype, bots)
    if fused:
        A.set_tuning("fused_min_envs", 64)
    A.reset(want_obs=False)
    B.reset(want_obs=False)
    dev = A.device
    stats = A.episode_stats_init(A.new_episode_stats())
    recs = [R.Record(s) for s in _states(B)]
    assert (stats.cpu().numpy() == _model_words(recs)).all()
    gen = torch.Generator(device="cpu").manual_seed(SEED)
    if codes != "raw":
        acts = torch.tensor(codes, dtype=torch.int8, device=dev)[None].expand(n, 4).contiguous()
    frozen = 0
    for t in range(TICKS):
        if codes == "raw":                                       # uniform over the five codes: about a third of them illegal
            acts = torch.randint(0, 5, (n, 4), generator=gen).to(device=dev, dtype=torch.int8)
        A.step(acts, want_obs=True)
        assert A.last_step_fused() == fused
        subs = []
        for agent in range(4):
            B.step_agent(agent, acts[:, agent].contiguous(), want_obs=False)
            subs.append(_states(B))
        assert torch.equal(A.done, B.done)
        done = A.done.cpu().numpy()
        frozen += sum(r.done for r in recs)
        for e, r in enumerate(recs):
            r.tick([subs[m][e] for m in range(4)], done[e])
        A.episode_stats_update(stats, A.done)
        got, want = stats.cpu().numpy(), _model_words(recs)
        bad = np.nonzero((got != want).any(0))[0]
        assert len(bad) == 0, (board, t, bad[:8], got[:, bad[0]], want[:, bad[0]])
    d = A.episode_stats_dict(stats)
    tot = {k: int(v.sum()) for k, v in d.items()}
    print(board, tot, "frozen row-ticks", frozen)
    assert tot["done"] == n and frozen > 0                       # every row finished and then stayed as it was
    assert (d["ticks"] <= LENGTH + 1).all()
    if codes == "raw":
        assert tot["stops"] > 0                                  # a Stop, or an illegal code that became one
    if board == "smallCapture":                                  # (measured: 35 eaten, 3 returned, 3 deaths, 2 kills)
        assert tot["eaten"] > 0 and tot["deaths"] > 0
    if board == "tinyCapture":                                   # (measured: 207 deaths, every one an invader stepping onto a defender)
        assert tot["deaths"] > 0
    A.close()
    B.close()


@functools.lru_cache(maxsize=None)
def _golden_episodes(name):
    d, meta = G.load(name)
    return d, meta, R.fixture_episodes(d)


@pytest.mark.parametrize("name", ("traj_small_hunter.npz", "traj_maze23_hunter.npz"))
def test_golden_episodes_replayed_from_their_actions(name):
    """env e of a 96-env batch replays finished episode e % (number of episodes) of the fixture from the recorded actions; its final
    record is the model's on the fixture's own states"""
    import pmx
    d, meta, eps = _golden_episodes(name)
    assert len(eps) >= 2
    n = 96
    starts = [0] + [t + 1 for _, t in eps[:-1]]
    spans = [(s, t + 1) for s, (_, t) in zip(starts, eps)]
    T = max(b - a for a, b in spans)
    env = pmx.PmxVecEnv(pmx.Layout(list(meta["layout"])), n, length=int(meta["length"]), auto_reset=False, obs_dtype="uint8", seed=SEED)
    env.reset(want_obs=False)
    stats = env.episode_stats_init(env.new_episode_stats())
    acts = np.full((T, n, 4), 4, np.int8)                        # Stop once the episode is over: the row is DONE by then
    for e in range(n):
        a, b = spans[e % len(eps)]
        acts[:b - a, e] = d["actions"][a:b]
    acts = torch.from_numpy(acts).to(env.device)
    for t in range(T):
        env.step(acts[t], want_obs=False)
        env.episode_stats_update(stats, env.done)
    got = stats.cpu().numpy()
    for e in range(n):
        want = eps[e % len(eps)][0].words()
        assert (got[:, e] == want).all(), (name, e, got[:, e], want)
    env.close()


def _scenario_env(pmx, n=1):
    return pmx.PmxVecEnv(pmx.Layout(list(R.SCENARIO_ROWS)), n, length=300, auto_reset=False, obs_dtype="uint8", seed=SEED)


def test_hand_set_states_through_set_state():
    """the CPU suite's scenarios, one per env: pmx_set_state, init, one step, update; the counters the CPU suite expects and the
    model's words on the handle's own sub-step states"""
    import pmx
    n = len(R.SCENARIOS)
    food, caps = R.scenario_layout()
    A, B = _scenario_env(pmx, n), _scenario_env(pmx, n)
    states = [pmx.make_state(s["pos"], s["dir"], s["pac"], s["scared"], s["carry"], s["ret"], food, caps, 0, 0, len(R.SCENARIO_ROWS))
              for s in R.SCENARIOS]
    for env in (A, B):
        env.reset(want_obs=False)
        env.set_state(states)
    stats = A.episode_stats_init(A.new_episode_stats())
    recs = [R.Record(s) for s in _states(B)]
    acts = torch.tensor([s["actions"] for s in R.SCENARIOS], dtype=torch.int8, device=A.device)
    A.step(acts, want_obs=False)
    subs = []
    for agent in range(4):
        B.step_agent(agent, acts[:, agent].contiguous(), want_obs=False)
        subs.append(_states(B))
    for e, r in enumerate(recs):
        r.tick([subs[m][e] for m in range(4)], 0)
        R.check_expect(r, R.SCENARIOS[e]["expect"])
    A.episode_stats_update(stats, A.done)
    assert (stats.cpu().numpy() == _model_words(recs)).all()
    A.close()
    B.close()


def _run(pmx, n, ticks, seed):
    env = pmx.PmxVecEnv("smallCapture", n, length=LENGTH, auto_reset=False, obs_dtype="uint8", seed=seed, bots=True)
    env.reset(want_obs=False)
    return env, torch.tensor((-3, -3, -4, -4), dtype=torch.int8, device=env.device)[None].expand(n, 4).contiguous()


def test_contract():
    import pmx
    L = pmx._lib
    n = 131
    env, acts = _run(pmx, n, 0, SEED)
    dev = env.device
    # sub-ranges between canary bands on a NaN-pattern buffer: only the range's rows are written, all 48 words of them
    PAD, first, count = 3, 37, 70
    NAN = 0x7FC00000
    inner = torch.zeros((L.STATS_WORDS, count), dtype=torch.int32, device=dev)
    whole = env.episode_stats_init(env.new_episode_stats())
    env.episode_stats_init(inner, first=first, count=count)
    assert torch.equal(inner, whole[:, first:first + count])
    st = L.stream(dev)
    call = lambda name, *a: getattr(env.lib, name)(env.handle, *a, st)
    two = torch.full((L.STATS_WORDS * 2 + 2 * PAD,), NAN, dtype=torch.int32, device=dev)      # a flat buffer: [48][2] between PAD words
    assert call("pmx_episode_stats_init", n - 2, 2, two[PAD:].data_ptr()) == 0
    assert (two[:PAD] == NAN).all() and (two[PAD + 96:] == NAN).all() and (two[PAD:PAD + 96] != NAN).all()
    assert torch.equal(two[PAD:PAD + 96].view(48, 2), whole[:, n - 2:])
    for t in range(LENGTH + 3):
        env.step(acts, want_obs=False)
        env.episode_stats_update(whole, env.done)
        env.episode_stats_update(inner, env.done, first=first, count=count)
        assert call("pmx_episode_stats_update", n - 2, 2, env.done.data_ptr(), two[PAD:].data_ptr()) == 0
    assert torch.equal(inner, whole[:, first:first + count])
    assert torch.equal(two[PAD:PAD + 96].view(48, 2), whole[:, n - 2:])
    assert (two[:PAD] == NAN).all() and (two[PAD + 96:] == NAN).all()
    d = env.episode_stats_dict(whole)
    assert bool(d["done"].all()) and d["eaten"].shape == (n, 4) and d["ticks"].shape == (n,)
    assert torch.equal(d["score"], whole[33]) and torch.equal(d["kills"][:, 2], whole[8 * 2 + L.STAT_KILLS])
    # a DONE row is bit-identical after five more steps and updates, a row that is not DONE is not
    frozen = whole.clone()
    live = env.episode_stats_init(env.new_episode_stats())
    for _ in range(5):
        env.step(acts, want_obs=False)
        env.episode_stats_update(whole, env.done)
        env.episode_stats_update(live, None)                     # done_dev NULL: DONE is never set
    assert torch.equal(whole, frozen)
    assert (live[32] == 5).all() and (live[34] == 0).all()
    # count == 0 launches nothing and is no error, at either end of the handle
    assert call("pmx_episode_stats_init", 0, 0, whole.data_ptr()) == 0 and call("pmx_episode_stats_update", n, 0, None, whole.data_ptr()) == 0
    assert torch.equal(whole, frozen)
    # errors
    INVALID, UNSUPPORTED = -1, -2
    assert env.lib.pmx_episode_stats_init(None, 0, 1, whole.data_ptr(), st) == INVALID
    assert call("pmx_episode_stats_init", 0, 1, None) == INVALID and call("pmx_episode_stats_update", 0, 1, None, None) == INVALID
    for f, c in ((-1, 1), (0, -1), (n, 1), (1, n), (2 ** 31 - 1, 2)):
        assert call("pmx_episode_stats_init", f, c, whole.data_ptr()) == INVALID, (f, c)
        assert call("pmx_episode_stats_update", f, c, None, whole.data_ptr()) == INVALID, (f, c)
    env.reset(want_obs=False)                                    # nothing stepped since: the snapshots describe no tick
    assert call("pmx_episode_stats_update", 0, n, None, whole.data_ptr()) == INVALID
    assert b"snapshots" in env.lib.pmx_last_error()
    env.step(acts, want_obs=False)
    env.set_state(env.get_state(0, 1))
    assert call("pmx_episode_stats_update", 0, n, None, whole.data_ptr()) == INVALID
    env.step(acts, want_obs=False)
    env.step_agent(0, acts[:, 0].contiguous(), want_obs=False)    # an open tick
    assert call("pmx_episode_stats_update", 0, n, None, whole.data_ptr()) == INVALID
    assert call("pmx_episode_stats_init", 0, n, whole.data_ptr()) == INVALID
    assert torch.equal(whole, frozen)
    env.close()
    auto = pmx.PmxVecEnv("smallCapture", 64, length=LENGTH, auto_reset=True, obs_dtype="uint8", seed=SEED)
    auto.reset(want_obs=False)
    buf = auto.new_episode_stats()
    with pytest.raises(L.PmxError, match="code -2"):
        auto.episode_stats_init(buf)
    auto.step(torch.full((64, 4), 4, dtype=torch.int8, device=dev), want_obs=False)
    assert auto.lib.pmx_episode_stats_update(auto.handle, 0, 64, None, buf.data_ptr(), st) == UNSUPPORTED
    assert (buf == 0).all()
    auto.close()


def test_two_runs_from_one_start_are_bit_identical():
    import pmx
    out = []
    for _ in range(2):
        env, acts = _run(pmx, 200, 0, SEED)
        stats = env.episode_stats_init(env.new_episode_stats())
        for t in range(LENGTH + 1):
            env.step(acts, want_obs=False)
            env.episode_stats_update(stats, env.done)
        out.append(stats.clone())
        env.close()
    assert torch.equal(out[0], out[1]) and bool(out[0][34].all())
