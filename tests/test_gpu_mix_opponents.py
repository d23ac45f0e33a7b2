"""Mixed-opponent rollouts on the GPU (VecMAPPOTrainer(mix_opponents=True), evaluate_vectorized(side=...)): a plan of ONE
blue group against the default trainer's rollout bit for bit, a phase-3 plan (self, pool, two hard bots and random side by
side, both colours) through a full update, and the evaluation on either colour.  tinyCapture, 64 or 96 envs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RANDOM_LEGAL = -2            # include/pmx.h PMX_ACTION_RANDOM_LEGAL


def _trainer(**kw):
    from pmx import trainer
    args = dict(n_envs=64, horizon=8, minibatch=128, epochs=1, seed=4, length=5, opponent="curriculum")
    args.update(kw)
    return trainer.VecMAPPOTrainer("tinyCapture", **args)


@pytest.mark.parametrize("opponent", ["curriculum", "baseline"])
def test_single_blue_group_rollout_equals_the_default_rollout_bit_for_bit(opponent, monkeypatch):
    """curriculum phase 1 (all random) and a fixed bot team: one blue group, so the per-env colour, reward, shaping and action
    plumbing must reproduce the default path -- same seed, same draws, same buffers.  With the flag off the new symbol is not
    called; with it on, the uniform one is not."""
    from pmx import _lib
    called, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (called.append(name), real(name, *args))[1])
    a, b = _trainer(opponent=opponent), _trainer(opponent=opponent, mix_opponents=True)
    for u in range(2):                                          # the second rollout starts from mid-game states
        del called[:]
        a.rollout()
        assert called.count("pmx_emit_team_obs") == a.T + 1 and "pmx_emit_team_obs_mixed" not in called
        del called[:]
        b.rollout()
        assert called.count("pmx_emit_team_obs_mixed") == b.T + 1 and "pmx_emit_team_obs" not in called
        assert b.mix_groups == [("random" if opponent == "curriculum" else opponent, False, 0, 64)]
        assert a.stats["opponent"] == b.mix_groups[0][0] and a.stats["play_as_red"] is False and b.stats["opponent"] == "mixed"
        for name in ("obs_buf", "merged_buf", "act_buf", "rew_buf", "done_buf", "logp_buf", "val_buf"):
            x, y = getattr(a, name), getattr(b, name)
            assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), (u, name)
        assert torch.equal(a._acts, b._acts) and torch.equal(a.prev_agent, b.prev_agent) and torch.equal(a.last_value, b.last_value)
        for k in ("rollout_reward", "episodes", "wins"):
            assert torch.equal(a.stats[k], b.stats[k]), k
        assert int(a.stats["episodes"]) >= 64 and float(a.done_buf.sum()) > 0       # games ended inside the rollout (length 5)
        assert len(torch.unique(a.rew_buf)) > 2
    a.env.close()
    b.env.close()


@pytest.mark.parametrize("variant", ["graph", "masked"])
def test_phase_three_plan_plays_every_group_and_updates(variant):
    from pmx import trainer
    kw = dict(use_graph=True) if variant == "graph" else dict(mask_illegal=True)
    N, T = 96, 4
    tr = _trainer(n_envs=N, horizon=T, length=3, minibatch=192, curriculum_scale=0.01, hard_bots=("baseline", "approxq"), mix_opponents=True, **kw)
    tr.update_idx = 9                                           # past 800 * scale = 8: self / pool / bots
    assert len(tr.opponent_pool) >= 1
    plan = trainer.mix_plan(9, 0.01, N, ("baseline", "approxq"), "curriculum")
    assert [m for m, _, _, _ in plan] == ["self", "self", "pool", "pool", "baseline", "approxq", "random"]
    # the reset state the rollout starts from, through the uniform entry
    uni = {}
    for red in (False, True):
        uni[red] = (torch.empty_like(tr.obs_buf[0]), torch.empty_like(tr.merged_buf[0]))
        tr.env.emit_team_obs(red, *uni[red])
    draws = []

    class _Rng:                                                 # the rollout's host stream: nothing but randint may be called
        def randint(self, *args):
            draws.append(args)
            return 0

    tr.np_rng = _Rng()
    st = tr.train_update()
    assert tr.mix_groups == plan and tr.update_idx == 10
    assert draws == [(1,)]                                      # one draw, the pool snapshot's index
    acts, red = tr._acts, tr.team_red
    assert red.dtype == torch.uint8 and red.shape == (N,)
    env_idx = torch.arange(N, device=acts.device)
    for mode, is_red, first, count in plan:
        inside = (env_idx >= first) & (env_idx < first + count)
        assert bool((red[inside] == int(is_red)).all())
        own, opp = ([0, 2], [1, 3]) if is_red else ([1, 3], [0, 2])
        assert bool(((acts[inside][:, own] >= 0) & (acts[inside][:, own] <= 4)).all())          # the learners' sampled actions
        if mode in trainer.BOT_TEAMS:                           # the team's codes in the opponent columns of exactly this group
            for col, code in zip(opp, trainer.BOT_TEAMS[mode]):
                assert torch.equal((acts == code).any(1), inside) and bool((acts[inside][:, col] == code).all()), mode
        elif mode == "random":
            assert bool((acts[inside][:, opp] == RANDOM_LEGAL).all())
        else:                                                   # a network opponent's sampled actions
            assert bool(((acts[inside][:, opp] >= 0) & (acts[inside][:, opp] <= 4)).all())
    rb = red.to(torch.bool)
    assert 0 < int(rb.sum()) < N
    for is_red in (False, True):
        rows = rb == is_red
        assert torch.equal(tr.obs_buf[0][rows], uni[is_red][0][rows]) and torch.equal(tr.merged_buf[0][rows], uni[is_red][1][rows])
        assert not torch.equal(tr.obs_buf[0][rows], uni[not is_red][0][rows])
    for name in ("obs_buf", "merged_buf", "logp_buf", "rew_buf", "done_buf", "val_buf", "adv_buf", "ret_buf"):
        assert bool(torch.isfinite(getattr(tr, name).float()).all()), name
    assert bool(((tr.act_buf >= 0) & (tr.act_buf <= 4)).all())
    if variant == "masked":
        assert bool((((tr.legal_buf.long() | 0x10) >> tr.act_buf) & 1).bool().all())           # only legal actions were drawn
    assert set(st["episodes_by_mode"]) == set(st["wins_by_mode"]) == {"self", "pool", "baseline", "approxq", "random"}
    assert sum(int(v) for v in st["episodes_by_mode"].values()) == int(st["episodes"]) >= N     # length 3: every env ended a game
    assert sum(int(v) for v in st["wins_by_mode"].values()) == int(st["wins"])
    assert all(0 <= int(st["wins_by_mode"][m]) <= int(st["episodes_by_mode"][m]) for m in st["episodes_by_mode"])
    assert st["opponent"] == "mixed" and st["optimizer_steps"] == T * N * 2 // 192
    assert bool(torch.isfinite(st["grad_norm"]).all()) and float(st["grad_norm"]) > 0
    if variant == "graph":
        assert tr.use_graph and tr._graph_ready                 # the replayed step ran
    tr.env.close()


class _StopModel:
    """a policy whose logits are forced to Stop"""
    training = False

    def eval(self):
        return self

    def train(self):
        return self

    def get_deterministic_action(self, obs, *, legal=None):
        return torch.full((obs.shape[0],), 4, dtype=torch.int64, device=obs.device)


def _stop_returns(n, opponent, length, seed, red):
    """What the env's reward tensors give the learner team of each env when its two agents always stop: the sum of both learners'
    (identical) team rewards up to the env's first done, and the final score -- stepped here with explicit columns."""
    import pmx
    from pmx import trainer
    env = pmx.PmxVecEnv("tinyCapture", n, length=length, auto_reset=True, obs_dtype="bfloat16", seed=seed, bots=True)
    env.reset(want_obs=False)
    acts = torch.full((n, 4), 4, dtype=torch.int8, device="cuda")
    codes = trainer.BOT_TEAMS[opponent]
    for e in range(n):
        cols = (1, 3) if red[e] else (0, 2)
        acts[e, cols[0]], acts[e, cols[1]] = codes
    ret = torch.zeros(n, dtype=torch.float64, device="cuda")
    final = torch.zeros(n, dtype=torch.int32, device="cuda")
    alive = torch.ones(n, dtype=torch.bool, device="cuda")
    team = torch.tensor([0 if r else 1 for r in red], device="cuda")
    for _ in range(length + 1):
        _, rew, done, info = env.step(acts, want_obs=False)
        r = rew.gather(1, team[:, None]).squeeze(1)
        ret += torch.where(alive, r + r, torch.zeros_like(ret))
        d = done.to(torch.bool) & alive
        final = torch.where(d, info["score"], final)
        alive &= ~d
    assert not bool(alive.any())
    env.close()
    won = torch.where(torch.tensor(list(red), device="cuda"), final > 0, final < 0)
    return float(ret.mean()), float(ret.std()), float(won.double().mean())


def test_evaluate_vectorized_sides():
    from pmx import mappo, trainer
    import pmx
    lay = pmx.get_layout("tinyCapture")
    torch.manual_seed(3)
    model = mappo.MAPPOAgent((8, lay.height, lay.width), 5, 2).cuda()
    n, length = 64, 30
    kw = dict(layout="tinyCapture", n_envs=n, opponent="baseline", length=length, seed=2)
    base = trainer.evaluate_vectorized(model, **kw)
    assert trainer.evaluate_vectorized(model, side="blue", **kw) == base         # the default value and its results
    for side in ("red", "both"):
        for mask in (False, True):
            mean, std, rate = trainer.evaluate_vectorized(model, side=side, mask_illegal=mask, **kw)
            assert np.isfinite(mean) and np.isfinite(std) and 0.0 <= rate <= 1.0, (side, mask)
    with pytest.raises(ValueError):
        trainer.evaluate_vectorized(model, side="green", **kw)
    # a policy that always stops: each colour's learner team gets what the env pays that team
    for side, red in (("red", [True] * n), ("both", [True] * (n // 2) + [False] * (n - n // 2))):
        got = trainer.evaluate_vectorized(_StopModel(), side=side, **kw)
        assert got == _stop_returns(n, "baseline", length, 2, red), side
    blue = trainer.evaluate_vectorized(_StopModel(), **kw)                     # and the untouched blue path agrees with the same count
    assert blue == _stop_returns(n, "baseline", length, 2, [False] * n)
