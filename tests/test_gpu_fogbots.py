"""GPU tests of the fog-bound bots (pmx_set_bot_sight), all through the C ABI.

The kernels are compared with tests/_fogbots_model.py, which tests/test_fogbots_cpu.py pins to the reference's own numbers on
observations (fixture G12); G12's values also go through the kernel directly, byte for byte.  A handle at a sight that hides
nothing, and a handle switched on and off again, must equal a handle never set on every output."""
import functools
import random

import numpy as np
import pytest
import torch

import _approxq_model as AQ
import _fogbots_model as FB
import _golden as G

pytestmark = pytest.mark.gpu

SEED = 20261
BOT_CODES = (FB.BASE_OFF, FB.BASE_DEF, FB.AQ_OFF, FB.AQ_DEF)


def _ctypes_states(states):
    import pmx
    return (pmx._lib.State * len(states)).from_buffer_copy(np.ascontiguousarray(states).tobytes())


def _numpy_states(arr):
    return np.frombuffer(bytes(arr), AQ.STATE).copy()


# ---- G12 through the query -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", range(5))
def test_g12_through_the_query(s):
    """The states of one source's kept rows in an env each, one batch per sight: after pmx_set_bot_sight, pmx_bot_query returns
    the reference's values on the observation (byte-equal), the action the model draws from the fixture's best set, the
    reference's walk home, and the seen flags."""
    import pmx
    rec, _, sources, _ = FB.load_g12()
    src = sources[s]
    mine = np.nonzero(rec["src"] == s)[0]
    rows = sorted(set(int(r) for r in rec["row"][mine]))                 # the rows the generator kept
    slot = {r: n for n, r in enumerate(rows)}
    states = src["states"][[src["local"][r] for r in rows]].copy()
    n = len(states)
    states["ticks"] = (np.arange(n, dtype=np.uint32) * 2654435761 >> 7).astype(np.uint32)      # a different draw in every env
    env = pmx.PmxVecEnv(pmx.Layout.from_text(src["layout"]), n, length=300, auto_reset=False, bots=True, seed=SEED)
    env.set_state(_ctypes_states(states))
    before = bytes(env.get_state())
    checked = 0
    for sight in (5, 1):
        env.set_bot_sight(sight)
        for agent in range(4):
            for code in BOT_CODES:
                ks = mine[(rec["sight"][mine] == sight) & (rec["agent"][mine] == agent) & (rec["code"][mine] == code)]
                if not len(ks):
                    continue
                values, action, flags = (t.cpu().numpy() for t in env.bot_query(agent, code))
                for k in ks:
                    e = slot[int(rec["row"][k])]
                    assert values[e].tobytes() == rec["values"][k].tobytes(), (s, sight, k, values[e], rec["values"][k])
                    ev = dict(legal=int(rec["legal"][k]), best=int(rec["best"][k]), home=int(rec["home"][k]))
                    act, fl = AQ.Model.play(ev, code, SEED, e, int(states["ticks"][e]), agent)
                    fl |= (FB.FLAG_SEEN_LO if rec["seen"][k][0] else 0) | (FB.FLAG_SEEN_HI if rec["seen"][k][1] else 0)
                    assert (int(action[e]), int(flags[e])) == (act, fl), (s, sight, k)
                    if not fl & (AQ.FLAG_HOME | AQ.FLAG_EXPLORED):
                        assert (int(rec["best"][k]) >> int(action[e])) & 1, (s, sight, k)
                    if rec["home"][k] >= 0:
                        assert flags[e] & AQ.FLAG_HOME and action[e] == rec["home"][k]
                    checked += 1
    assert checked == len(mine)
    assert bytes(env.get_state()) == before                              # a query changes nothing
    env.close()


# ---- three handles -----------------------------------------------------------------------------------------------------------
def _hidden_records(board, sight):
    """(states, observer) of G12's defender records on that board in which an invader is hidden at that sight."""
    rec, _, sources, _ = FB.load_g12()
    states, observers = [], []
    for s, src in enumerate(sources):
        if G.load(src["name"])[1]["layout_name"] != board:
            continue
        for k in np.nonzero((rec["src"] == s) & (rec["code"] == FB.BASE_DEF) & (rec["sight"] == 5))[0]:
            st = src["states"][src["local"][int(rec["row"][k])]]
            i = int(rec["agent"][k])
            seen = FB.seen_flags(st, i, sight)
            if any(st["pac"][o] and not v for o, v in zip(FB.foes(i), seen)):
                states.append(st)
                observers.append(i)
    return np.array(states, AQ.STATE), np.array(observers)


def _codes(rng, n_envs, first_observer=None):
    """-3 .. -6 mixed over both sides, an eighth of the slots raw actions or the random bot.  first_observer (tick 0): the agents
    in front of the record's observer stop, so that the observer decides on the record's own state, as a defender."""
    codes = rng.choice(np.array(BOT_CODES, np.int8), (n_envs, 4))
    other = rng.randint(0, 8, (n_envs, 4)) == 0
    codes[other] = rng.choice(np.array([0, 1, 2, 3, 4, FB.RANDOM], np.int8), int(other.sum()))
    if first_observer is not None:
        for e, i in enumerate(first_observer):
            codes[e, :i] = 4
            codes[e, i] = (FB.BASE_DEF, FB.AQ_DEF)[e % 2]
    return codes.astype(np.int8)


@functools.lru_cache(maxsize=None)
def _differential(board, lay_name, n_envs, n_ticks, sight):
    """Three handles with one seed and one bot sight, started from G12's hidden-invader records tiled over the envs.  A: agent
    by agent with the codes; B: the same with the explicit actions pmx_bot_query returned on A just before; C: whole pmx_step
    ticks with the codes.  Every queried value, action and flag equals the model; the three handles are equal every tick.
    Returns the number of defender queries with a hidden invader per tick."""
    import pmx
    layout = pmx.get_layout(lay_name)
    model = FB.FogModel(layout.text)
    start, observer = _hidden_records(board, sight)
    assert len(start) >= 20
    pick = np.arange(n_envs) % len(start)
    start, observer = start[pick].copy(), observer[pick]
    start["ticks"], start["steps"] = 0, 0
    mk = lambda: pmx.PmxVecEnv(layout, n_envs, length=150, auto_reset=True, bots=True, seed=SEED, obs_agents=(0,), obs_dtype="uint8")
    A, B, Cc = mk(), mk(), mk()
    for e in (A, B, Cc):
        e.reset(want_obs=False)
        e.set_state(_ctypes_states(start))
        e.set_bot_sight(sight)
    rng = np.random.RandomState(6)
    dev = A.device
    hidden_queries = []
    for t in range(n_ticks):
        codes = _codes(rng, n_envs, observer if t == 0 else None)
        codes_dev = torch.from_numpy(codes).to(dev)
        n_hidden = 0
        for agent in range(4):
            st = _numpy_states(A.get_state())
            pst = AQ.to_pstates(st)
            explicit = codes[:, agent].copy()
            for code in np.unique(codes[:, agent]):
                if code >= 0:
                    continue
                values, action, flags = (x.cpu().numpy() for x in A.bot_query(agent, int(code)))
                for e in np.nonzero(codes[:, agent] == code)[0]:
                    ev, act, fl = model.decide(st[e], agent, int(code), SEED, int(e), pst[e], sight=sight)
                    assert values[e].tobytes() == ev["values"].tobytes(), (lay_name, sight, t, agent, e, code, values[e], ev["values"])
                    assert (int(action[e]), int(flags[e])) == (act, fl), (lay_name, sight, t, agent, e, code)
                    explicit[e] = act
                    if code in (FB.BASE_DEF, FB.AQ_DEF):
                        n_hidden += any(st[e]["pac"][o] and not v for o, v in zip(FB.foes(agent), ev["seen"]))
            A.step_agent(agent, codes_dev[:, agent].contiguous(), want_obs=False)
            B.step_agent(agent, torch.from_numpy(explicit).to(dev), want_obs=False)
            if agent < 3:
                assert bytes(A.get_state()) == bytes(B.get_state()), (lay_name, sight, t, agent)
        hidden_queries.append(n_hidden)
        Cc.step(codes_dev, want_obs=False)
        sa = bytes(A.get_state())
        assert sa == bytes(B.get_state()) and sa == bytes(Cc.get_state()), (lay_name, sight, t)
        for other in (B, Cc):
            assert A.reward.cpu().numpy().tobytes() == other.reward.cpu().numpy().tobytes(), (lay_name, sight, t)
            assert torch.equal(A.done, other.done) and torch.equal(A.legal, other.legal), (lay_name, sight, t)
            assert torch.equal(A.score, other.score) and torch.equal(A.score_change, other.score_change), (lay_name, sight, t)
            assert torch.equal(A.agent, other.agent), (lay_name, sight, t)
    for e in (A, B, Cc):
        e.close()
    return hidden_queries


@pytest.mark.parametrize("board, lay, n_envs, n_ticks, sight", [("small", "smallCapture", 320, 100, 5), ("blox", "bloxCapture", 320, 100, 5),
                                                               ("small", "smallCapture", 96, 60, 1)])
def test_query_substep_and_tick_agree_with_the_model(board, lay, n_envs, n_ticks, sight):
    hidden = _differential(board, lay, n_envs, n_ticks, sight)
    print(f"{lay} sight {sight}: defender queries with a hidden invader, tick 0: {hidden[0]}, all ticks: {sum(hidden)}")
    assert len(hidden) == n_ticks
    assert hidden[0] >= 20              # by construction: tick 0 asks every record's observer on the record's own state


def test_smallest_ragged_batch():
    """N = 65: one full wave and a second one with a single live lane."""
    hidden = _differential("small", "smallCapture", 65, 6, 5)
    assert hidden[0] >= 20


# ---- a sight that hides nothing, and on / off ----------------------------------------------------------------------------------
def _lockstep(make_x, make_y, n_envs=192, n_ticks=60, board="small", lay_name="smallCapture", flags_mask=0xFF):
    """Two handles from G12's hidden-invader records, whole ticks with mixed codes: every output of every tick is equal, and so
    is what pmx_bot_query says before every tick (flags under flags_mask)."""
    import pmx
    layout = pmx.get_layout(lay_name)
    start, _ = _hidden_records(board, 5)
    start = start[np.arange(n_envs) % len(start)].copy()
    start["ticks"], start["steps"] = 0, 0
    mk = lambda: pmx.PmxVecEnv(layout, n_envs, length=40, auto_reset=True, bots=True, seed=SEED, obs_dtype="uint8")
    X, Y = mk(), mk()
    for e in (X, Y):
        e.reset(want_obs=False)
        e.set_state(_ctypes_states(start))
    make_x(X)
    make_y(Y)
    rng = np.random.RandomState(8)
    dones = 0
    for t in range(n_ticks):
        codes = torch.from_numpy(_codes(rng, n_envs)).to(X.device)
        for agent, code in ((t % 4, FB.BASE_DEF), ((t + 1) % 4, FB.AQ_OFF), ((t + 2) % 4, FB.AQ_DEF), ((t + 3) % 4, FB.BASE_OFF)):
            (vx, ax, fx), (vy, ay, fy) = X.bot_query(agent, code), Y.bot_query(agent, code)
            assert vx.cpu().numpy().tobytes() == vy.cpu().numpy().tobytes() and torch.equal(ax, ay), (t, agent, code)
            assert torch.equal(fx & flags_mask, fy & flags_mask), (t, agent, code)
        ox, rx, dx, ix = X.step(codes)
        oy, ry, dy, iy = Y.step(codes)
        assert torch.equal(ox, oy) and rx.cpu().numpy().tobytes() == ry.cpu().numpy().tobytes() and torch.equal(dx, dy), t
        for key in ("legal_actions", "score_change", "score", "agent"):
            assert torch.equal(ix[key], iy[key]), (t, key)
        assert bytes(X.get_state()) == bytes(Y.get_state()), t
        dones += int(dx.sum())
    assert dones > 0                                                      # resets were crossed
    X.close()
    Y.close()


def test_sight_64_equals_a_handle_never_set():
    """No board has a Manhattan distance above 62: at sight 64 nothing is hidden.  The flags differ by the seen bits only."""
    _lockstep(lambda e: e.set_bot_sight(64), lambda e: None, flags_mask=AQ.FLAG_HOME | AQ.FLAG_EXPLORED)
    import pmx
    env = pmx.PmxVecEnv("smallCapture", 64, bots=True, seed=1)
    env.set_bot_sight(64)
    for code in BOT_CODES:
        assert (env.bot_query(0, code)[2].cpu().numpy() & 12 == 12).all()
    assert (env.bot_query(0, FB.RANDOM)[2].cpu().numpy() == 0).all()
    env.close()


def test_on_and_off_again_equals_a_handle_never_set():
    def on_off(e):
        e.set_bot_sight(5)
        st = bytes(e.get_state())
        e.bot_query(2, FB.BASE_DEF)                                       # a sight kernel ran on this handle
        assert bytes(e.get_state()) == st
        e.set_bot_sight(None)
    _lockstep(on_off, lambda e: None)


def test_sight_five_differs_from_off():
    """The rule is not a no-op: from the hidden-invader records a defender's values differ between a handle at sight 5 and one
    never set."""
    import pmx
    start, observer = _hidden_records("small", 5)
    n = len(start)
    env = pmx.PmxVecEnv("smallCapture", n, auto_reset=False, bots=True, seed=SEED)
    env.set_state(_ctypes_states(start))
    off = [env.bot_query(i, FB.BASE_DEF)[0].cpu().numpy() for i in range(4)]
    env.set_bot_sight(5)
    on = [env.bot_query(i, FB.BASE_DEF)[0].cpu().numpy() for i in range(4)]
    for e, i in enumerate(observer):
        assert on[i][e].tobytes() != off[i][e].tobytes(), e
    env.close()


def test_argument_errors():
    import pmx
    plain = pmx.PmxVecEnv("tinyCapture", 64, bots=False, seed=3)
    bots = pmx.PmxVecEnv("tinyCapture", 64, bots=True, seed=3)
    lib = plain.lib
    assert lib.pmx_set_bot_sight(None, 5) == -1                           # PMX_ERR_INVALID
    for bad in (0, 65, -2, 1000):
        assert lib.pmx_set_bot_sight(bots.handle, bad) == -1
        assert lib.pmx_set_bot_sight(plain.handle, bad) == -1
    for ok in (1, 5, 64, -1):
        assert lib.pmx_set_bot_sight(bots.handle, ok) == 0
    assert lib.pmx_set_bot_sight(plain.handle, 5) == -2                   # PMX_ERR_UNSUPPORTED
    assert b"enable_bots" in lib.pmx_last_error()
    assert lib.pmx_set_bot_sight(plain.handle, -1) == 0
    with pytest.raises(pmx._lib.PmxError):
        plain.set_bot_sight(5)
    with pytest.raises(pmx._lib.PmxError):
        bots.set_bot_sight(0)
    plain.close()
    bots.close()


# ---- host traces -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", ["bots_small_baselineTeam_fog.json", "bots_blox_approxQTeam_fog.json"])
def test_fog_bots_stream_exact(tmp_path, fixture):
    """The host team files asked on their own observation against the reference's trace under random.seed(k): the sonar draws of
    makeObservation and the bot's own draw fall in the same places of the stdlib `random` stream."""
    import pmx
    from pmx.game_state import DIR_CODE
    g = G.load_json(fixture)
    path = tmp_path / "l.lay"
    path.write_text("\n".join(g["layout"]))
    random.seed(g["random_seed"])
    env = pmx.gymPacMan_parallel_env(layout_file=str(path), length=g["length"], self_play=False, enemieName=g["team"], fog_bots=True)
    env.reset()
    chosen = []

    def hook():
        for b in (env.agents[0], env.agents[2]):
            if getattr(b, "_recorded", False):                            # reset() keeps the instances
                continue
            b._recorded = True
            orig = b.getAction

            def wrap(gs, _o=orig):
                a = _o(gs)
                chosen.append(a)
                return a
            b.getAction = wrap
    hook()
    assert len(g["blue_actions"]) == 320 and g["hidden_turns"] >= 10
    for t, (a1, a3) in enumerate(g["blue_actions"]):
        chosen.clear()
        o, r, term, info = env.step({env.agents[1]: a1, env.agents[3]: a3})
        assert [DIR_CODE[c] for c in chosen] == g["red_actions"][t], f"tick {t}: bot actions diverged"
        assert env.game.state.data.score == g["scores"][t], t
        assert [r[env.agents[0]], r[env.agents[1]]] == g["rewards"][t], t
        done = any(term.values())
        assert done == g["dones"][t], t
        if done:
            env.reset()
            hook()
    env.close()


# ---- trainer -------------------------------------------------------------------------------------------------------------------
def test_trainer_and_evaluation_smoke(monkeypatch):
    import pmx
    from pmx import _lib, mappo, trainer
    called, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (called.append((name,) + args[1:2] if name == "pmx_set_bot_sight" else name), real(name, *args))[1])
    kw = dict(n_envs=128, horizon=4, minibatch=256, epochs=1, seed=4, opponent="baseline", fog_of_war=True)
    tr = trainer.VecMAPPOTrainer("smallCapture", fog_bots=True, **kw)
    tr.rollout()
    assert called.count(("pmx_set_bot_sight", 5)) == 1 and tr.stats["opponent"] == "baseline"
    for buf in (tr.rew_buf, tr.val_buf, tr.logp_buf):
        assert torch.isfinite(buf).all()
    lay = pmx.get_layout("smallCapture")
    torch.manual_seed(3)
    model = mappo.MAPPOAgent((8, lay.height, lay.width), 5, 2).cuda()
    called.clear()
    mean, std, rate = trainer.evaluate_vectorized(model, layout="smallCapture", n_envs=64, opponent="baseline", length=40, seed=2,
                                                  fog_of_war=True, fog_bots=True)
    assert np.isfinite(mean) and np.isfinite(std) and 0.0 <= rate <= 1.0 and called.count(("pmx_set_bot_sight", 5)) == 1
    # a trainer built without the keyword is the trainer built with fog_bots=False, and neither makes the call
    called.clear()
    torch.manual_seed(11)
    plain = trainer.VecMAPPOTrainer("smallCapture", **kw)
    plain.rollout()
    torch.manual_seed(11)
    off = trainer.VecMAPPOTrainer("smallCapture", fog_bots=False, **kw)
    off.rollout()
    assert not any(isinstance(c, tuple) for c in called)
    for name in ("obs_buf", "merged_buf", "act_buf", "logp_buf", "rew_buf", "done_buf", "val_buf"):
        a, b = getattr(plain, name), getattr(off, name)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
