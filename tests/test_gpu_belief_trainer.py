"""VecMAPPOTrainer(belief=True) and evaluate_vectorized(belief=True) on the GPU: smallCapture, 64 envs, 8 ticks, 2 updates, every
opponent mode, mix_opponents and the graph-replayed step once.  Every belief emission is checked, as it is made, against the plain
emission of the same state (all planes but 5 of the learners' rows, the whole merged row) and against the sets it was given; in the
self-play run a second handle replays the rollout's actions sub-step by sub-step and the learners' sets are compared with the
model tests/_belief_ref.py at every tick, across the colour changes."""
import numpy as np
import pytest
import torch

import _belief_ref as R

pytestmark = pytest.mark.gpu

N, T, UPDATES = 64, 8, 2
OTHERS = [0, 1, 2, 3, 4, 6, 7]


def _trainer(**kw):
    from pmx import trainer
    args = dict(n_envs=N, horizon=T, minibatch=128, epochs=1, seed=4, opponent="self", fog_of_war=True, belief=True)
    args.update(kw)
    return trainer.VecMAPPOTrainer("smallCapture", **args)


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _plane5(belief, red, H, W):
    cells = torch.from_numpy(R.unpack(_words(belief)).any(2)[:, :, :H, :W]).cuda()
    return torch.where(red.view(-1, 1, 1, 1).to(torch.bool), cells.flip(-1), cells)


def _check_emissions(tr, monkeypatch):
    """wrap the env's two emission methods: a belief emission is compared with the plain one of the same state"""
    env = tr.env
    H, W = env.layout.height, env.layout.width
    count = {"belief": 0, "other": 0}
    plain_uniform, plain_mixed = env.emit_team_obs, env.emit_team_obs_mixed

    def compare(team_obs, merged, belief, red, plain):
        team, mrg = torch.empty_like(team_obs), (torch.empty_like(merged) if merged is not None else None)
        plain(team, mrg)
        assert torch.equal(team_obs[:, :, OTHERS], team[:, :, OTHERS])
        assert torch.equal(team_obs[:, :, 5], _plane5(belief, red, H, W).to(team_obs.dtype))
        if merged is not None:
            assert torch.equal(merged, mrg)                        # the critic's input: byte for byte the plain call's
        count["belief"] += 1

    def uniform(team_red, team_obs, merged=None, **kw):
        out = plain_uniform(team_red, team_obs, merged, **kw)
        if "belief" in kw:
            red = torch.full((len(team_obs),), int(bool(team_red)), device=team_obs.device)
            compare(team_obs, merged, kw["belief"], red, lambda t, m: plain_uniform(team_red, t, m))
        else:
            count["other"] += 1
        return out

    def mixed(team_red, team_obs, merged=None, first=0, count_=None, **kw):
        out = plain_mixed(team_red, team_obs, merged, first, count_, **kw)
        if "belief" in kw:
            n = len(team_obs)
            compare(team_obs, merged, kw["belief"], team_red[first:first + n], lambda t, m: plain_mixed(team_red, t, m, first, n))
        else:
            count["other"] += 1
        return out

    monkeypatch.setattr(env, "emit_team_obs", uniform)
    monkeypatch.setattr(env, "emit_team_obs_mixed", mixed)
    return count


@pytest.mark.parametrize("variant", ["random", "baseline", "approxq", "pool", "curriculum", "mixed", "graph"])
def test_two_updates_with_belief(variant, monkeypatch):
    kw = {"mixed": dict(mix_opponents=True), "graph": dict(use_graph=True, opponent="random")}.get(variant, dict(opponent=variant))
    if variant == "curriculum":
        kw.update(curriculum_scale=0.0025)                         # update 0 random, update 1 a hard team
    tr = _trainer(**kw)
    count = _check_emissions(tr, monkeypatch)
    for u in range(UPDATES):
        st = tr.train_update()
        for k in ("pg", "vl", "entropy", "grad_norm"):
            assert bool(torch.isfinite(torch.as_tensor(st[k])).all()), (u, k)
        assert float(st["grad_norm"]) > 0
        # what the policy saw: plane 5 holds 0 / 1, at least one cell per slot (a set is never empty), more than the two enemies somewhere
        p5 = tr.obs_buf[:, :, :, 5]
        assert bool(((p5 == 0) | (p5 == 1)).all()) and bool((p5.flatten(3).sum(3) >= 1).all())
        assert bool((p5.flatten(3).sum(3) > 2).any())
    net = variant in ("pool", "mixed")
    assert count["other"] == 0 and count["belief"] == UPDATES * ((2 if net else 1) * T + 1)
    if variant == "graph":
        assert tr.use_graph and tr._graph_ready
    tr.env.close()


def test_self_play_sets_equal_the_model_across_colour_changes(monkeypatch):
    import pmx
    tr = _trainer(opponent="self", seed=4)
    env = tr.env
    count = _check_emissions(tr, monkeypatch)
    B = pmx.PmxVecEnv("smallCapture", N, length=300, auto_reset=True, obs_dtype="uint8", seed=4 * 1000003, bots=False)
    B.reset(want_obs=False)
    lay = env.layout
    open_g = np.repeat(R.open_cells(lay.wall_rows, lay.width, lay.height)[None], N, 0)
    starts = np.repeat(lay.starts.astype(np.int64)[None], N, 0)
    own = tr._belief[0]
    model = {"own": R.init(0, open_g, starts), "sub": None, "ticks": None, "checked": 0, "inits": 0}
    assert (_words(own) == model["own"]).all()
    real_step, real_update, real_init = env.step, env.belief_update, env.belief_init

    def step(actions, want_obs=True):
        out = real_step(actions, want_obs)
        sub = []
        for agent in range(4):
            B.step_agent(agent, actions[:, agent].contiguous(), want_obs=False)
            st = B.get_state()
            sub.append(np.array([[[s.pos[i][0], s.pos[i][1]] for i in range(4)] for s in st], np.int64))
        model["sub"], model["ticks"] = np.stack(sub, 1), np.array([s.ticks for s in st], np.uint32)
        assert torch.equal(env.done, B.done)
        return out

    def update(team_red, belief, sight_range, reset=None, **kw):
        out = real_update(team_red, belief, sight_range, reset=reset, **kw)
        if belief.data_ptr() == own.data_ptr():
            first = 0 if team_red else 1
            P = np.stack([model["sub"][:, first], model["sub"][:, first + 2]], 1)
            want, _, _ = R.update(model["own"], P, np.full(N, bool(team_red)), sight_range, model["ticks"], 4 * 1000003, np.arange(N),
                                  open_g, starts, reset=reset.cpu().numpy())
            assert (_words(belief) == want).all()
            model["own"] = want
            model["checked"] += 1
        return out

    def init(belief, kind=0, first=0, count=None):
        out = real_init(belief, kind, first, count)
        if belief.data_ptr() == own.data_ptr():
            assert kind == 1 and first == 0 and len(belief) == N
            model["own"] = R.init(1, open_g, starts)
            model["inits"] += 1
        return out

    monkeypatch.setattr(env, "step", step)
    monkeypatch.setattr(env, "belief_update", update)
    monkeypatch.setattr(env, "belief_init", init)
    colours = []
    for u in range(4):                                             # (seed 4 draws blue, red, red, blue)
        tr.rollout()
        colours.append(tr.stats["play_as_red"])
    assert model["checked"] == 4 * T and count["belief"] == 4 * (2 * T + 1)
    changes = sum(a != b for a, b in zip(colours, colours[1:]))
    assert changes >= 1 and model["inits"] == changes
    B.close()
    env.close()


def test_flag_off_calls_no_new_entry_point_and_first_tick_inputs_agree(monkeypatch):
    """belief=False: the calls are those made before the flag existed (none of the new entry points), and two such runs on one
    seed fill bit-identical buffers.  With the flag on, the first tick -- before any action differs -- feeds the critic the same
    row."""
    from pmx import _lib
    called, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (called.append(name), real(name, *args))[1])
    bufs = []
    for _ in range(2):
        tr = _trainer(belief=False, opponent="random")
        tr.train_update()
        bufs.append((tr.obs_buf.clone(), tr.merged_buf.clone(), tr.act_buf.clone(), tr.rew_buf.clone()))
        tr.env.close()
    assert not any("belief" in c for c in called)
    assert all(torch.equal(a, b) for a, b in zip(*bufs))
    tr = _trainer(opponent="random")
    tr.rollout()
    assert torch.equal(tr.merged_buf[0], bufs[0][1][0])
    assert {"pmx_belief_init", "pmx_belief_update", "pmx_emit_team_obs_belief"} <= set(called)
    tr.env.close()


def test_evaluate_vectorized_with_belief():
    import pmx
    from pmx import mappo, trainer
    lay = pmx.get_layout("smallCapture")
    torch.manual_seed(3)
    model = mappo.MAPPOAgent((8, lay.height, lay.width), 5, 2).cuda()
    kw = dict(layout="smallCapture", n_envs=64, opponent="baseline", length=40, seed=2, fog_of_war=True)
    for side in ("both", "blue", "red"):
        mean, std, rate = trainer.evaluate_vectorized(model, side=side, belief=True, **kw)
        assert np.isfinite(mean) and np.isfinite(std) and 0.0 <= rate <= 1.0, side
    mean, std, rate = trainer.evaluate_vectorized(model, side="both", belief=True, mask_illegal=True, **kw)
    assert np.isfinite(mean) and np.isfinite(std) and 0.0 <= rate <= 1.0
