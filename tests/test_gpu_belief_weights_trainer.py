"""VecMAPPOTrainer(belief_weights=True) and evaluate_vectorized(belief_weights=True) on the GPU: smallCapture, 64 envs, horizon 8, two
updates.  A second handle replays the rollout's actions sub-step by sub-step and the numpy model tests/_belief_weights_ref.py is
advanced beside the learners' buffer; plane 5 of obs_buf at every stored step must be the model's levels for that env and step.
Every weighted emission is compared, as it is made, with the plain emission of the same state."""
import numpy as np
import pytest
import torch

import _belief_ref as B
import _belief_weights_ref as R

pytestmark = pytest.mark.gpu

N, T, UPDATES = 64, 8, 2
OTHERS = [0, 1, 2, 3, 4, 6, 7]
SEED = 4


def _trainer(**kw):
    from pmx import trainer
    args = dict(n_envs=N, horizon=T, minibatch=128, epochs=1, seed=SEED, opponent="self", fog_of_war=True, belief=True, belief_weights=True)
    args.update(kw)
    return trainer.VecMAPPOTrainer("smallCapture", **args)


def _flip_where(lv, red):
    return torch.where(red.view(-1, 1, 1, 1).to(torch.bool), lv.flip(-1), lv)


@pytest.mark.parametrize("variant", ["self", "mixed"])
def test_two_updates_plane_5_is_the_models_levels(variant, monkeypatch):
    """merged_buf: every merged row is compared with the plain emission of the very state it was made from (the critic's input is
    untouched by the flag), and the first tick's rows -- made before any action can differ -- with those of a run without the flag.
    Later ticks of the two runs differ by design: the policy sees levels in one and 0 / 1 in the other and acts differently."""
    import pmx
    mixed = variant == "mixed"
    tr = _trainer(**({"mix_opponents": True} if mixed else {}))
    env = tr.env
    lay = env.layout
    H, W = lay.height, lay.width
    Bh = pmx.PmxVecEnv("smallCapture", N, length=300, auto_reset=True, obs_dtype="uint8", seed=SEED * 1000003, bots=False)
    Bh.reset(want_obs=False)
    open_g = np.repeat(B.open_cells(lay.wall_rows, W, H)[None], N, 0)
    starts = np.repeat(lay.starts.astype(np.int64)[None], N, 0)
    own_b, own_w, own_l = tr._belief[0]
    words, w, lv = R.init(0, open_g, starts, H, W)
    m = {"w": w, "words": words, "lev": lv, "sub": None, "ticks": None, "checked": 0, "inits": 0, "shown": [], "emissions": 0}
    assert (own_l.cpu().numpy().reshape(N, 2, H, W) == lv).all()
    real_step, real_update, real_init = env.step, env.belief_weights_update, env.belief_weights_init
    real_uniform, real_mixed = env.emit_team_obs, env.emit_team_obs_mixed

    def step(actions, want_obs=True):
        out = real_step(actions, want_obs)
        sub = []
        for agent in range(4):
            Bh.step_agent(agent, actions[:, agent].contiguous(), want_obs=False)
            st = Bh.get_state()
            sub.append(np.array([[[s.pos[i][0], s.pos[i][1]] for i in range(4)] for s in st], np.int64))
        m["sub"], m["ticks"] = np.stack(sub, 1), np.array([s.ticks for s in st], np.uint32)
        assert torch.equal(env.done, Bh.done)
        return out

    def update(team_red, belief, weights, levels, sight_range, reset=None, **kw):
        out = real_update(team_red, belief, weights, levels, sight_range, reset=reset, **kw)
        if belief.data_ptr() == own_b.data_ptr():
            red = team_red.cpu().numpy().astype(bool) if isinstance(team_red, torch.Tensor) else np.full(N, bool(team_red))
            first = np.where(red, 0, 1)
            ar = np.arange(N)
            P = np.stack([m["sub"][ar, first], m["sub"][ar, first + 2]], 1)
            m["w"], m["lev"], m["words"], _, _ = R.update(m["w"], m["words"], P, red, sight_range, m["ticks"], SEED * 1000003, ar, open_g,
                                                         starts, H, W, reset=reset.cpu().numpy())
            assert (weights.cpu().numpy().view(np.uint16).reshape(N, 2, 2, H, W) == m["w"]).all()
            assert (levels.cpu().numpy().reshape(N, 2, H, W) == m["lev"]).all()
            assert (belief.cpu().numpy().view(np.uint32) == m["words"]).all()
            m["checked"] += 1
        return out

    def init(belief, weights, levels, kind=0, first=0, count=None):
        out = real_init(belief, weights, levels, kind, first, count)
        if belief.data_ptr() == own_b.data_ptr():
            assert kind == 1 and first == 0 and len(belief) == N
            m["words"], m["w"], m["lev"] = R.init(1, open_g, starts, H, W)
            m["inits"] += 1
        return out

    def compare(team_obs, merged, levels, red, plain):
        team, mrg = torch.empty_like(team_obs), (torch.empty_like(merged) if merged is not None else None)
        plain(team, mrg)
        assert torch.equal(team_obs[:, :, OTHERS], team[:, :, OTHERS])
        assert torch.equal(team_obs[:, :, 5], _flip_where(levels.view(-1, 2, H, W), red).to(team_obs.dtype))
        if merged is not None:
            assert torch.equal(merged, mrg)
            if levels.data_ptr() == own_l.data_ptr():
                m["shown"].append((m["lev"].copy(), red.cpu().numpy().astype(bool)))
        m["emissions"] += 1

    def uniform(team_red, team_obs, merged=None, **kw):
        assert set(kw) == {"levels"}
        out = real_uniform(team_red, team_obs, merged, **kw)
        red = torch.full((len(team_obs),), int(bool(team_red)), device=team_obs.device)
        compare(team_obs, merged, kw["levels"], red, lambda t, mm: real_uniform(team_red, t, mm))
        return out

    def mixed_emit(team_red, team_obs, merged=None, first=0, count=None, **kw):
        assert set(kw) == {"levels"}
        out = real_mixed(team_red, team_obs, merged, first, count, **kw)
        n = len(team_obs)
        compare(team_obs, merged, kw["levels"], team_red[first:first + n], lambda t, mm: real_mixed(team_red, t, mm, first, n))
        return out

    for name, fn in (("step", step), ("belief_weights_update", update), ("belief_weights_init", init), ("emit_team_obs", uniform),
                     ("emit_team_obs_mixed", mixed_emit)):
        monkeypatch.setattr(env, name, fn)
    before = tr.learner.bucket.data.clone()
    first_merged = None
    for u in range(UPDATES):
        m["shown"].clear()
        st = tr.train_update()
        for k in ("pg", "vl", "entropy", "grad_norm"):
            assert bool(torch.isfinite(torch.as_tensor(st[k])).all()), (u, k)
        assert float(st["grad_norm"]) > 0
        assert len(m["shown"]) == T + 1                                # the T stored steps and the bootstrap observation
        graded = 0
        for t in range(T):
            lev, red = m["shown"][t]
            want = np.where(red[:, None, None, None], lev[..., ::-1], lev)
            got = tr.obs_buf[t][:, :, 5].float().cpu().numpy()
            assert (got == want).all(), (u, t)
            graded += int(((want > 0) & (want < 16)).sum())
        assert graded > 0                                              # levels between 0 and 16 reached the policy
        if first_merged is None:
            first_merged = tr.merged_buf[0].clone()
    assert m["checked"] == UPDATES * T and m["emissions"] == UPDATES * (2 * T + 1)
    assert not torch.equal(before, tr.learner.bucket.data)             # the parameters moved
    Bh.close()
    env.close()
    off = _trainer(belief_weights=False, **({"mix_opponents": True} if mixed else {}))
    off.rollout()
    assert torch.equal(off.merged_buf[0], first_merged)
    off.env.close()


def test_flag_off_calls_no_new_entry_point(monkeypatch):
    """belief_weights=False (given, and by default): no symbol with `weight` in its name is called, and the two runs fill
    bit-identical rollout buffers under one seed"""
    from pmx import _lib
    called, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (called.append(name), real(name, *args))[1])
    bufs = []
    for kw in ({"belief_weights": False}, {}):
        from pmx import trainer
        args = dict(n_envs=N, horizon=T, minibatch=128, epochs=1, seed=SEED, opponent="self", fog_of_war=True, belief=True)
        args.update(kw)
        tr = trainer.VecMAPPOTrainer("smallCapture", **args)
        tr.train_update()
        bufs.append((tr.obs_buf.clone(), tr.merged_buf.clone(), tr.act_buf.clone(), tr.rew_buf.clone()))
        tr.env.close()
    assert called and not any("weight" in c for c in called)
    assert {"pmx_belief_init", "pmx_belief_update", "pmx_emit_team_obs_belief"} <= set(called)
    assert all(torch.equal(a, b) for a, b in zip(*bufs))
    called.clear()
    tr = _trainer(opponent="random")
    tr.rollout()
    assert {"pmx_belief_weights_init", "pmx_belief_weights_update", "pmx_emit_team_obs_weighted"} <= set(called)
    assert not {"pmx_belief_init", "pmx_belief_update", "pmx_emit_team_obs_belief"} & set(called)      # replaced, not run in addition
    tr.env.close()


def test_evaluate_vectorized_with_belief_weights():
    """64 episodes run and return; no claim about strength"""
    import pmx
    from pmx import mappo, trainer
    lay = pmx.get_layout("smallCapture")
    torch.manual_seed(3)
    model = mappo.MAPPOAgent((8, lay.height, lay.width), 5, 2).cuda()
    kw = dict(layout="smallCapture", n_envs=64, opponent="baseline", length=40, seed=2, fog_of_war=True, belief=True, belief_weights=True)
    for side in ("both", "blue"):
        mean, std, rate = trainer.evaluate_vectorized(model, side=side, **kw)
        assert np.isfinite(mean) and np.isfinite(std) and 0.0 <= rate <= 1.0, side
