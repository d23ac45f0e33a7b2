"""pmx.trainer.play_match on the GPU: against the existing yardstick evaluate_vectorized, exactly (the two run the same emission,
forward and step; the envs differ in auto_reset only, which cannot act before a game's first done), and network against network:
determinism, the runner's own checks, and each side's eyes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REGIME = dict(fog_of_war=True, belief=True, belief_weights=True, belief_evidence=True)


def _agent(layout, seed):
    import pmx
    from pmx import mappo
    lay = pmx.get_layout(layout)
    torch.manual_seed(seed)
    return mappo.MAPPOAgent((8, lay.height, lay.width), 5, 2).to(DEV)


@pytest.fixture(scope="module")
def small_model():
    return _agent("smallCapture", 5)


@pytest.mark.parametrize("regime", ({}, REGIME), ids=("full_state", "fog_belief_weights_evidence"))
def test_greedy_against_baseline_equals_evaluate_vectorized(small_model, regime):
    from pmx import trainer
    kw = dict(layout="smallCapture", n_envs=128, length=60, device=DEV, seed=3)
    mean, std, win = trainer.evaluate_vectorized(small_model, opponent="baseline", side="both", **regime, **kw)
    r = trainer.play_match(trainer.MatchSide(model=small_model, greedy=True, **regime), trainer.MatchSide(bot="baseline"), colours="both", **kw)
    print("evaluate_vectorized", mean, win, "play_match", r["return_a"], r["win_rate_a"], "ticks", r["ticks_mean"])
    assert r["games"] == 128 and r["wins_a"] + r["ties"] + r["wins_b"] == 128
    assert r["win_rate_a"] == win
    assert abs(r["return_a"] - mean) <= 1e-9
    assert int(r["red"].sum()) == 64 and bool(r["red"][:64].all())


def test_sides_swapped_and_one_colour_equals_evaluate_vectorized(small_model):
    from pmx import trainer
    kw = dict(layout="smallCapture", n_envs=128, length=60, device=DEV, seed=4)
    mean, std, win = trainer.evaluate_vectorized(small_model, opponent="baseline", side="red", **kw)
    r = trainer.play_match(trainer.MatchSide(bot="baseline"), trainer.MatchSide(model=small_model, greedy=True), colours="blue", **kw)
    print("evaluate_vectorized", mean, win, "play_match", r["return_b"], r["wins_b"] / r["games"])
    assert r["wins_b"] / r["games"] == win                        # B is the network, red everywhere: a win is a final score > 0
    assert abs(r["return_b"] - mean) <= 1e-9
    assert not bool(r["red"].any()) and r["as_red"]["games"] == 0 and r["as_blue"]["games"] == 128


class _Spy:
    """a network side that, on chosen ticks, asks the env for the observation its regime's entry point writes and compares"""

    def __init__(self, model, env, red, ticks, **emit_kw):
        self.model, self.env, self.red, self.ticks, self.emit_kw = model, env, red, ticks, emit_kw
        self.training, self.t, self.checked, self.differs_from_plain = False, 0, [], []

    def eval(self):
        return self

    def logits(self, obs):
        if self.t in self.ticks:
            want = torch.empty((self.env.n_envs, 2) + self.env.obs_shape, dtype=self.env.obs_torch_dtype, device=obs.device)
            self.env.emit_team_obs_mixed(self.red, want, **self.emit_kw)
            assert torch.equal(obs.reshape(want.shape).view(torch.int16), want.view(torch.int16)), ("tick", self.t)
            plain = torch.empty_like(want)
            self.env.emit_team_obs_mixed(self.red, plain)
            self.differs_from_plain.append(not torch.equal(plain.view(torch.int16), want.view(torch.int16)))
            self.checked.append(self.t)
        self.t += 1
        return self.model.logits(obs)


def test_network_against_network():
    import pmx
    from pmx import trainer
    n = 128
    ma, mb = _agent("tinyCapture", 1), _agent("tinyCapture", 2)
    kw = dict(layout="tinyCapture", n_envs=n, length=80, device=DEV, colours="both")
    A, B = trainer.MatchSide(model=ma, fog_of_war=True, sight_range=3), trainer.MatchSide(model=mb, mask_illegal=True)
    r1, r2, r3 = (trainer.play_match(A, B, seed=s, **kw) for s in (7, 7, 8))
    assert torch.equal(r1["score"], r2["score"]) and torch.equal(r1["stats"], r2["stats"])
    assert not torch.equal(r1["stats"], r3["stats"])
    for r in (r1, r3):
        assert r["wins_a"] + r["ties"] + r["wins_b"] == r["games"] == n
        assert r["as_red"]["games"] == r["as_blue"]["games"] == n // 2
        st = r["stats"]
        # the runner's three assertions, once more from outside
        assert bool((st[34] == 1).all()) and torch.equal(st[33], r["score"])
        assert torch.equal(st[1] + st[17] - st[9] - st[25], r["score"])
        assert 1.0 <= r["ticks_mean"] <= 81.0
    # each side's eyes, on tick 0 and a mid-game tick, on an env of the test's own
    env = pmx.PmxVecEnv("tinyCapture", n, length=80, auto_reset=False, obs_dtype="bfloat16", device=DEV, seed=7)
    red = trainer.match_colours(n, "both", DEV)
    sa = _Spy(ma, env, red, (0, 30), sight_range=3)
    sb = _Spy(mb, env, 1 - red, (0, 30))
    r4 = trainer.play_match(trainer.MatchSide(model=sa, fog_of_war=True, sight_range=3), trainer.MatchSide(model=sb, mask_illegal=True), seed=7, env=env, **kw)
    assert sa.checked == [0, 30] and sb.checked == [0, 30]
    assert sa.differs_from_plain[1] and not any(sb.differs_from_plain)      # by tick 30 somebody is out of A's sight of 3
    assert torch.equal(r4["stats"], r1["stats"])                            # the spies changed nothing


def test_two_bots_and_fog_bots():
    from pmx import trainer
    r = trainer.play_match(trainer.MatchSide(bot="approxq"), trainer.MatchSide(bot="random"), layout="tinyCapture", n_envs=64, length=60,
                           device=DEV, seed=1)
    assert r["games"] == 64 and r["wins_a"] + r["ties"] + r["wins_b"] == 64
    assert sum(r["stats_b"]["eaten"]) <= sum(r["stats_a"]["eaten"])         # the random team eats no more than approxQTeam
    m = _agent("tinyCapture", 3)
    r = trainer.play_match(trainer.MatchSide(model=m, fog_of_war=True), trainer.MatchSide(bot="baseline"), layout="tinyCapture", n_envs=64,
                           length=60, device=DEV, seed=1, fog_bots=True)
    assert r["games"] == 64
