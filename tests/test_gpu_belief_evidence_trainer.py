"""VecMAPPOTrainer(belief_evidence=True) and evaluate_vectorized(belief_evidence=True) on the GPU: smallCapture, 64 envs, horizon 8.
The kernels themselves are held to the model in tests/test_gpu_belief_evidence.py; here the flag runs through a rollout and an
update with sets and with weights, against a network opponent and in a mixed rollout, and plane 5 of every emission is compared
with the plane 5 the sets without evidence give for the same state."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, T = 64, 8
SEED = 4
EVIDENCE_CALLS = {"pmx_belief_evidence_init", "pmx_belief_update_evidence", "pmx_belief_weights_update_evidence"}


def _trainer(**kw):
    from pmx import trainer
    args = dict(n_envs=N, horizon=T, minibatch=128, epochs=1, seed=SEED, opponent="self", fog_of_war=True, belief=True, belief_evidence=True)
    args.update(kw)
    return trainer.VecMAPPOTrainer("smallCapture", **args)


@pytest.mark.parametrize("variant", ["self", "mixed"])
@pytest.mark.parametrize("weights", [False, True], ids=["sets", "weights"])
def test_an_update_with_the_flag(weights, variant, monkeypatch):
    """opponent="self" is a network opponent: the inverted-colour buffer gets evidence rows of its own"""
    from pmx import _lib
    called, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (called.append(name), real(name, *args))[1])
    tr = _trainer(belief_weights=weights, **({"mix_opponents": True} if variant == "mixed" else {}))
    before = tr.learner.bucket.data.clone()
    st = tr.train_update()
    for k in ("pg", "vl", "entropy", "grad_norm"):
        assert bool(torch.isfinite(torch.as_tensor(st[k])).all()), k
    assert float(st["grad_norm"]) > 0 and not torch.equal(before, tr.learner.bucket.data)
    update, parent = ("pmx_belief_weights_update_evidence", "pmx_belief_weights_update") if weights else ("pmx_belief_update_evidence", "pmx_belief_update")
    assert called.count(update) == 2 * T and parent not in called              # both buffers at every step, in place of the parent call
    inits = called.count("pmx_belief_weights_init" if weights else "pmx_belief_init")
    assert called.count("pmx_belief_evidence_init") == inits >= 2
    for buf in (tr._belief, tr._belief_opp):
        ev = buf[2].cpu().numpy()
        rows = (buf[1] == 0) | (buf[1] == 1)                                    # the rows the rollout updated
        assert rows.any() and (ev[rows, 34] == 1).all() and (ev[rows, 35] == 0).all()
    tr.env.close()


@pytest.mark.parametrize("variant", ["self", "mixed"])
def test_plane_5_lies_within_the_plane_5_without_evidence(variant, monkeypatch):
    """Two runs under one seed part ways after the first tick, because the policy acts on what plane 5 shows.  So the sets without
    evidence are advanced here beside the learners' buffer, on the same states, by pmx_belief_update, and every emission of the
    rollout is compared cell for cell with the emission those sets give."""
    tr = _trainer(**({"mix_opponents": True} if variant == "mixed" else {}))
    env = tr.env
    own = tr._belief[0]
    shadow = env.belief_init(env.new_belief(), 0)
    n = {"updates": 0, "emissions": 0, "fewer": 0}
    real_update, real_init, real_uniform, real_mixed = env.belief_update, env.belief_init, env.emit_team_obs, env.emit_team_obs_mixed
    mine = lambda t: own.data_ptr() <= t.data_ptr() < own.data_ptr() + own.numel() * 4

    def update(team_red, belief, sight_range, reset=None, first=0, count=None, evidence=None, **kw):
        assert evidence is not None
        out = real_update(team_red, belief, sight_range, reset=reset, first=first, count=count, evidence=evidence, **kw)
        if mine(belief):
            assert len(belief) == N
            real_update(team_red, shadow, sight_range, reset=reset)
            n["updates"] += 1
        return out

    def init(belief, kind=0, first=0, count=None):
        out = real_init(belief, kind, first, count)
        if mine(belief):
            row = (belief.data_ptr() - own.data_ptr()) // 512
            real_init(shadow[row:row + len(belief)], kind, first, count)
        return out

    def compare(team_obs, belief, plain):
        if mine(belief):
            team = torch.empty_like(team_obs)
            plain(team, shadow[:len(team_obs)])
            assert bool((team_obs[:, :, 5] <= team[:, :, 5]).all())
            assert torch.equal(team_obs[:, :, :5], team[:, :, :5]) and torch.equal(team_obs[:, :, 6:], team[:, :, 6:])
            n["fewer"] += int((team_obs[:, :, 5] < team[:, :, 5]).sum())
            n["emissions"] += 1

    def uniform(team_red, team_obs, merged=None, **kw):
        out = real_uniform(team_red, team_obs, merged, **kw)
        compare(team_obs, kw["belief"], lambda t, b: real_uniform(team_red, t, None, belief=b))
        return out

    def mixed_emit(team_red, team_obs, merged=None, first=0, count=None, **kw):
        out = real_mixed(team_red, team_obs, merged, first, count, **kw)
        compare(team_obs, kw["belief"], lambda t, b: real_mixed(team_red, t, None, first, len(t), belief=b))
        return out

    for name, fn in (("belief_update", update), ("belief_init", init), ("emit_team_obs", uniform), ("emit_team_obs_mixed", mixed_emit)):
        monkeypatch.setattr(env, name, fn)
    for _ in range(3):
        tr.rollout()
    print(f"{variant}: {n['fewer']} cells of plane 5 cleared by the evidence in {n['emissions']} emissions")
    assert n["updates"] == 3 * T and n["emissions"] == 3 * (T + 1) and n["fewer"] > 0
    env.close()


def test_flag_off_calls_no_new_entry_point(monkeypatch):
    from pmx import _lib
    called, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (called.append(name), real(name, *args))[1])
    for kw in ({"belief_evidence": False}, {"belief_evidence": False, "belief_weights": True}):
        tr = _trainer(**kw)
        tr.rollout()
        tr.env.close()
    assert called and not EVIDENCE_CALLS & set(called)


@pytest.mark.parametrize("weights", [False, True], ids=["sets", "weights"])
def test_evaluate_vectorized_with_belief_evidence(weights, monkeypatch):
    """64 episodes run and return; no claim about strength"""
    import pmx
    from pmx import _lib, mappo, trainer
    called, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (called.append(name), real(name, *args))[1])
    lay = pmx.get_layout("smallCapture")
    torch.manual_seed(3)
    model = mappo.MAPPOAgent((8, lay.height, lay.width), 5, 2).cuda()
    kw = dict(layout="smallCapture", n_envs=64, opponent="baseline", length=40, seed=2, fog_of_war=True, belief=True, belief_evidence=True,
              **({"belief_weights": True} if weights else {}))
    for side in ("both", "blue"):
        mean, std, rate = trainer.evaluate_vectorized(model, side=side, **kw)
        assert np.isfinite(mean) and np.isfinite(std) and 0.0 <= rate <= 1.0, side
    assert "pmx_belief_evidence_init" in called
    assert ("pmx_belief_weights_update_evidence" if weights else "pmx_belief_update_evidence") in called
    assert "pmx_belief_update" not in called and "pmx_belief_weights_update" not in called
