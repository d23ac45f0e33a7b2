"""VecMAPPOTrainer(fog_of_war=True) and evaluate_vectorized(fog_of_war=True) on the GPU: smallCapture, 64 envs, horizon 4, one
train_update, eager and with the graph-replayed step under legal-action masks.  What the policy was fed obeys the sight rule, what
the centralised critic was fed does not, and every emission of the rollout went through the fog entry points."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, T = 64, 4


def _trainer(**kw):
    from pmx import trainer
    args = dict(n_envs=N, horizon=T, minibatch=128, epochs=1, seed=4, opponent="self", fog_of_war=True)
    args.update(kw)
    return trainer.VecMAPPOTrainer("smallCapture", **args)


@pytest.mark.parametrize("variant", ["eager", "graph_masked", "mixed"])
def test_one_update_under_fog(variant, monkeypatch):
    from pmx import _lib, trainer
    kw = {"eager": {}, "graph_masked": dict(use_graph=True, mask_illegal=True), "mixed": dict(mix_opponents=True)}[variant]
    called, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (called.append(name), real(name, *args))[1])
    tr = _trainer(**kw)
    st = tr.train_update()
    # every emission of the rollout: the learners' and the opponent network's per tick, and the bootstrap observation
    fog_name = "pmx_emit_team_obs_mixed_fog" if variant == "mixed" else "pmx_emit_team_obs_fog"
    assert called.count(fog_name) == 2 * T + 1
    assert not any(c in ("pmx_emit_team_obs", "pmx_emit_team_obs_mixed") for c in called)
    for k in ("pg", "vl", "entropy", "grad_norm"):
        assert bool(torch.isfinite(torch.as_tensor(st[k])).all()), k
    assert float(st["grad_norm"]) > 0 and st["optimizer_steps"] == T * N * 2 // 128
    if variant == "graph_masked":
        assert tr.use_graph and tr._graph_ready
        assert bool((((tr.legal_buf.long() | 0x10) >> tr.act_buf) & 1).bool().all())
    # the policy's input: no enemy cell farther than 5 from every team cell (fog_obs finds nothing left to clear) ...
    obs = tr.obs_buf
    assert torch.equal(trainer.fog_obs(obs, 5), obs)
    # ... while the critic's input keeps both enemies, so some row shows an enemy that both of its learners' rows hide (on this
    # board the starts are three cells apart in pairs, so that takes a few moves: four ticks of 64 sampled games have them)
    enemy_m = tr.merged_buf[:, :, 5] != 0                                         # [T, N, H, W]
    enemy_o = obs[:, :, :, 5] != 0                                                # [T, N, 2, H, W]
    assert bool((enemy_m.flatten(2).sum(2) >= 1).all())                           # (two enemies, on one or two cells)
    assert bool((enemy_m & ~enemy_o[:, :, 0] & ~enemy_o[:, :, 1]).any())
    assert int(enemy_o.sum()) < 2 * int(enemy_m.sum())
    # merged_buf is the non-fog merged row: the bootstrap state through the plain entry gives the same critic input
    plain = torch.empty_like(tr._boot_merged)
    team = torch.empty_like(tr._boot_obs)
    if variant == "mixed":
        tr.env.emit_team_obs_mixed(tr.team_red, team, plain)
    else:
        tr.env.emit_team_obs(tr.stats["play_as_red"], team, plain)
    assert torch.equal(tr._boot_merged, plain) and torch.equal(tr._boot_obs, trainer.fog_obs(team, 5))
    tr.env.close()


def test_ippo_critic_is_fed_the_fogged_own_observation():
    tr = _trainer(algorithm="ippo", opponent="random")
    st = tr.train_update()
    assert bool(torch.isfinite(st["grad_norm"]).all()) and bool(torch.isfinite(tr.val_buf).all())
    from pmx import trainer
    assert torch.equal(trainer.fog_obs(tr.obs_buf, 5), tr.obs_buf)
    tr.env.close()


def test_checkpoint_round_trip_and_mismatch(tmp_path):
    a = _trainer(opponent="random")
    path = str(tmp_path / "fog.pt")
    a.save_full(path)
    _trainer(opponent="random").load_full(path)
    with pytest.raises(ValueError, match="fog_of_war=True"):
        _trainer(opponent="random", fog_of_war=False).load_full(path)
    a.env.close()


def test_evaluate_vectorized_under_fog():
    import pmx
    from pmx import mappo, trainer
    lay = pmx.get_layout("smallCapture")
    torch.manual_seed(3)
    model = mappo.MAPPOAgent((8, lay.height, lay.width), 5, 2).cuda()
    kw = dict(layout="smallCapture", n_envs=64, opponent="baseline", length=40, seed=2)
    for side in ("both", "blue", "red"):
        mean, std, rate = trainer.evaluate_vectorized(model, side=side, fog_of_war=True, **kw)
        assert np.isfinite(mean) and np.isfinite(std) and 0.0 <= rate <= 1.0, side
    mean, std, rate = trainer.evaluate_vectorized(model, side="both", fog_of_war=True, mask_illegal=True, **kw)
    assert np.isfinite(mean) and np.isfinite(std) and 0.0 <= rate <= 1.0
    # a sight range that hides nothing is the evaluation without fog (the blue side through the emission-based loop)
    assert trainer.evaluate_vectorized(model, side="both", fog_of_war=True, sight_range=62, **kw) == trainer.evaluate_vectorized(model, side="both", **kw)
    assert trainer.evaluate_vectorized(model, side="blue", fog_of_war=True, sight_range=62, **kw) == trainer.evaluate_vectorized(model, **kw)
