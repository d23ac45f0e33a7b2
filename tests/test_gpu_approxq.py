"""GPU tests of the in-kernel approxQTeam (action codes -5 / -6), of pmx_bot_query and of the host team file.

The kernels are compared with tests/_approxq_model.py, which tests/test_approxq_cpu.py pins to the reference's own numbers
(fixture G10); the values of G10 also go through the kernel directly, byte for byte."""
import functools
import random

import numpy as np
import pytest
import torch

import _approxq_model as AQ
import _golden as G

pytestmark = pytest.mark.gpu

SEED = 20251
SNAP = ("pos", "dir", "pac", "scared", "carry", "ret", "food", "caps", "score", "steps", "ticks")


def _ctypes_states(states):
    import pmx
    return (pmx._lib.State * len(states)).from_buffer_copy(np.ascontiguousarray(states).tobytes())


def _numpy_states(arr):
    return np.frombuffer(bytes(arr), AQ.STATE).copy()


@pytest.mark.parametrize("lay", ["small", "tiny", "blox"])
def test_g10_through_the_kernel(lay):
    """Every G10 state in an env of its own: pmx_bot_query returns the reference's values (byte-equal), walks home where the
    reference does, with the reference's action, and otherwise plays what the model draws from the fixture's best set."""
    import pmx
    d, meta = G.load(f"approxq_{lay}.npz")
    n = len(d["in_pos"])
    ticks = (np.arange(n, dtype=np.uint32) * 2654435761 >> 7).astype(np.uint32)        # a different draw in every env
    states = AQ.states_from_arrays(*(d["in_" + k] for k in SNAP[:-1]), ticks=ticks)
    env = pmx.PmxVecEnv(pmx.Layout.from_text(meta["layout"]), n, length=300, auto_reset=False, bots=True, seed=SEED)
    env.set_state(_ctypes_states(states))
    before = bytes(env.get_state())
    checked = 0
    for agent in range(4):
        code = AQ.AQ_OFF if agent < 2 else AQ.AQ_DEF
        values, action, flags = (t.cpu().numpy() for t in env.bot_query(agent, code))
        for k in np.nonzero(d["agent"] == agent)[0]:
            s = int(d["state"][k])
            assert values[s].tobytes() == d["values"][k].tobytes(), (lay, k, values[s], d["values"][k])
            ev = dict(legal=int(d["legal"][k]), best=int(d["best"][k]), home=int(d["home"][k]))
            act, fl = AQ.Model.play(ev, code, SEED, s, int(ticks[s]), agent)
            assert (int(action[s]), int(flags[s])) == (act, fl), (lay, k)
            if d["home"][k] >= 0:
                assert flags[s] == AQ.FLAG_HOME and action[s] == d["home"][k]
            checked += 1
    assert checked == len(d["state"])
    assert bytes(env.get_state()) == before                                           # a query changes nothing
    env.close()


def test_bot_query_argument_errors():
    import pmx
    plain = pmx.PmxVecEnv("tinyCapture", 64, bots=False, seed=3)
    v, a, f = plain.bot_query(1, AQ.RANDOM)
    legal = plain.observe(want_obs=False)[1].cpu().numpy()
    assert ((legal[:, 1] >> a.cpu().numpy()) & 1).all() and (f.cpu().numpy() == 0).all()
    vv = v.cpu().numpy()
    assert (np.isnan(vv) == (((legal[:, 1:2] >> np.arange(5)[None]) & 1) == 0)).all() and np.nan_to_num(vv).sum() == 0
    lib = plain.lib
    assert lib.pmx_bot_query(plain.handle, 0, -5, None, None, None, None) == -2       # PMX_ERR_UNSUPPORTED
    assert lib.pmx_bot_query(plain.handle, 4, -2, None, None, None, None) == -1
    assert lib.pmx_bot_query(plain.handle, 0, -7, None, None, None, None) == -1
    assert lib.pmx_bot_query(plain.handle, 0, 0, None, None, None, None) == -1
    # elsewhere the new codes act as Stop
    acts = torch.full((64, 4), -5, dtype=torch.int8, device="cuda")
    acts[:, 2:] = -6
    s0 = _numpy_states(plain.get_state())
    plain.step(acts, want_obs=False)
    s1 = _numpy_states(plain.get_state())
    assert (s0["pos"] == s1["pos"]).all()
    plain.close()


@functools.lru_cache(maxsize=None)
def _differential(lay_name, n_envs=320, n_ticks=340):
    """Three handles with one seed.  A: agent by agent with the codes; B: the same with the explicit actions pmx_bot_query
    returned on A just before; C: whole pmx_step ticks with the codes.  Asserts the equalities as it goes; returns the red
    forager's (home, explored) flags of every decision."""
    import pmx
    layout = pmx.get_layout(lay_name)
    model = AQ.Model(layout.text)
    mk = lambda: pmx.PmxVecEnv(layout, n_envs, length=150, auto_reset=True, bots=True, seed=SEED, obs_agents=(0,), obs_dtype="uint8")
    A, B, Cc = mk(), mk(), mk()
    for e in (A, B, Cc):
        e.reset(want_obs=False)
    rng = np.random.RandomState(5)
    red_flags = []
    dev = A.device
    for t in range(n_ticks):
        codes = rng.randint(0, 5, (n_envs, 4)).astype(np.int8)
        codes[:, 0], codes[:, 2] = AQ.AQ_OFF, AQ.AQ_DEF
        codes[0::2, 1], codes[0::2, 3] = AQ.AQ_OFF, AQ.AQ_DEF
        mix = rng.randint(0, 8, (n_envs, 2))                                          # the other half of blue: raw and -2 / -3 / -4
        for j, col in enumerate((1, 3)):
            sel = np.zeros(n_envs, bool)
            sel[1::2] = True
            for m, c in ((5, AQ.RANDOM), (6, AQ.BASE_OFF), (7, AQ.BASE_DEF)):
                codes[sel & (mix[:, j] == m), col] = c
        codes_dev = torch.from_numpy(codes).to(dev)
        for agent in range(4):
            st = _numpy_states(A.get_state())
            pst = AQ.to_pstates(st)
            explicit = codes[:, agent].copy()
            for code in np.unique(codes[:, agent]):
                if code >= 0:
                    continue
                values, action, flags = (x.cpu().numpy() for x in A.bot_query(agent, int(code)))
                for e in np.nonzero(codes[:, agent] == code)[0]:
                    ev, act, fl = model.decide(st[e], agent, int(code), SEED, int(e), pst[e])
                    assert values[e].tobytes() == ev["values"].tobytes(), (lay_name, t, agent, e, code, values[e], ev["values"])
                    assert (int(action[e]), int(flags[e])) == (act, fl), (lay_name, t, agent, e, code)
                    explicit[e] = act
                if agent == 0 and code == AQ.AQ_OFF:
                    red_flags.append(flags.copy())
            A.step_agent(agent, codes_dev[:, agent].contiguous(), want_obs=False)
            B.step_agent(agent, torch.from_numpy(explicit).to(dev), want_obs=False)
            if agent < 3:
                assert bytes(A.get_state()) == bytes(B.get_state()), (lay_name, t, agent)
        Cc.step(codes_dev, want_obs=False)
        sa = bytes(A.get_state())
        assert sa == bytes(B.get_state()) and sa == bytes(Cc.get_state()), (lay_name, t)
        for other in (B, Cc):
            assert A.reward.cpu().numpy().tobytes() == other.reward.cpu().numpy().tobytes(), (lay_name, t)
            assert torch.equal(A.done, other.done) and torch.equal(A.legal, other.legal), (lay_name, t)
            assert torch.equal(A.score, other.score) and torch.equal(A.score_change, other.score_change), (lay_name, t)
        assert torch.equal(A.agent, B.agent), (lay_name, t)
        assert torch.equal(A.agent, Cc.agent), (lay_name, t)
    for e in (A, B, Cc):
        e.close()
    return np.stack(red_flags)


@pytest.mark.parametrize("lay", ["smallCapture", "tinyCapture"])
def test_query_substep_and_tick_agree_with_the_model(lay):
    flags = _differential(lay)
    assert flags.shape == (340, 320)
    assert (flags & AQ.FLAG_HOME).any() and (flags & AQ.FLAG_EXPLORED).any() and (flags == 0).any()


def test_explore_share():
    """Over the red forager's decisions that were not walks home the explored share is 0.1 within five binomial standard
    deviations: 0.1 +- 5 * sqrt(0.1 * 0.9 / n)."""
    flags = _differential("smallCapture")
    free = (flags & AQ.FLAG_HOME) == 0
    n = int(free.sum())
    share = float(((flags & AQ.FLAG_EXPLORED) != 0)[free].mean())
    print(f"explore share {share:.5f} over n = {n} decisions, bound {5 * (0.09 / n) ** 0.5:.5f}")
    assert n > 1000
    assert abs(share - 0.1) <= 5 * (0.09 / n) ** 0.5


def _write_layout(tmp_path, rows, name):
    p = tmp_path / name
    p.write_text("\n".join(rows))
    return str(p)


@pytest.mark.parametrize("fixture", ["bots_small_approxQTeam.json", "bots_tiny_approxQTeam.json"])
def test_bots_stream_exact(tmp_path, fixture):
    """The host team file against the reference's trace under random.seed(k) (same stdlib `random` call order)."""
    import pmx
    from pmx.game_state import DIR_CODE
    g = G.load_json(fixture)
    path = _write_layout(tmp_path, g["layout"], "l.lay")
    random.seed(g["random_seed"])
    env = pmx.gymPacMan_parallel_env(layout_file=path, length=g["length"], self_play=False, enemieName=g["team"])
    assert not isinstance(env.agents[0], int) and not isinstance(env.agents[2], int) and env.agents[1] == 1
    env.reset()
    chosen = []

    def hook():
        for b in (env.agents[0], env.agents[2]):
            orig = b.getAction

            def wrap(gs, _o=orig):
                a = _o(gs)
                chosen.append(a)
                return a
            b.getAction = wrap
    hook()
    assert len(g["blue_actions"]) == 320
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


def test_trainer_and_evaluation_against_approxq():
    from pmx import mappo, trainer
    torch.manual_seed(0)
    model = mappo.MAPPOAgent((8, 7, 20), 5, 2).cuda()
    mean, std, wr = trainer.evaluate_vectorized(model, layout="tinyCapture", n_envs=256, opponent="approxq", length=60)
    assert np.isfinite(mean) and np.isfinite(std) and 0.0 <= wr <= 1.0
    tr = trainer.VecMAPPOTrainer("tinyCapture", 128, horizon=8, minibatch=256, obs_dtype="bfloat16", opponent="approxq", length=40)
    tr.rollout()
    assert tr.stats["opponent"] == "approxq"
    assert (tr._acts[:, 0] == -5).all() and (tr._acts[:, 2] == -6).all()
    tr.compute_gae()
    tr.update()
    for buf in (tr.rew_buf, tr.val_buf, tr.adv_buf, tr.ret_buf, tr.logp_buf):
        assert torch.isfinite(buf).all()
    assert torch.isfinite(tr.stats["loss"]).all()
    tc = trainer.VecMAPPOTrainer("tinyCapture", 64, horizon=4, minibatch=128, obs_dtype="bfloat16", opponent="curriculum",
                                 curriculum_scale=0.01, hard_bots=("approxq",), length=40)
    tc.update_idx = 5
    seen = set()
    for _ in range(6):
        tc.rollout()
        seen.add(tc.stats["opponent"])
    assert "approxq" in seen and seen <= {"approxq", "random"}


def test_in_kernel_approxq_beats_random():
    """In-kernel approxQTeam (red) against in-kernel randomTeam (blue), one episode per env: the mean final score is positive
    (the reference's own team scores about +9 against random blue actions on this board; DESIGN.md has both figures)."""
    import pmx
    N = 1024
    env = pmx.PmxVecEnv("smallCapture", N, length=300, auto_reset=True, bots=True, seed=11, obs_agents=(0,), obs_dtype="uint8")
    env.reset(want_obs=False)
    acts = torch.empty((N, 4), dtype=torch.int8, device="cuda")
    acts[:, 0], acts[:, 2], acts[:, 1], acts[:, 3] = -5, -6, -2, -2
    alive = torch.ones(N, dtype=torch.bool, device="cuda")
    final = torch.zeros(N, dtype=torch.int32, device="cuda")
    for _ in range(301):
        _, _, done, info = env.step(acts, want_obs=False)
        d = done.to(torch.bool) & alive
        final = torch.where(d, info["score"], final)
        alive &= ~d
    assert not bool(alive.any())
    mean = float(final.double().mean())
    print(f"in-kernel approxQTeam vs randomTeam, smallCapture, {N} episodes: mean final score {mean:.3f}, "
          f"wins {float((final > 0).double().mean()):.3f}")
    assert mean > 0
    env.close()
