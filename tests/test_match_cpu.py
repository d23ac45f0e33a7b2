"""CPU suite: pmx.trainer.MatchSide / play_match without a GPU -- every ValueError, the colour split, the side seeds, and the loop and
its bookkeeping on a stand-in env (as tests/test_fog_cpu.py does for the trainer's flag)."""
import importlib.util
import os

import pytest
import torch

import pmx
from pmx import trainer
from pmx.trainer import MatchSide, play_match

L = pmx._lib


class _Net:
    """a stand-in policy: prefers action (row + bias) % 5"""
    training = False

    def __init__(self, bias=0):
        self.bias = bias
        self.calls = 0

    def eval(self):
        return self

    def logits(self, obs):
        self.calls += 1
        B = obs.shape[0]
        return torch.nn.functional.one_hot((torch.arange(B) + self.bias) % 5, 5).float() * 8.0

    def get_deterministic_action(self, obs, *, legal=None):
        return self.logits(obs).argmax(-1)


NET = _Net()


@pytest.mark.parametrize("kw, text", [
    (dict(), "exactly one"), (dict(model=NET, bot="baseline"), "exactly one"), (dict(bot="astar"), "bot must be one of"),
    (dict(bot="baseline", greedy=True), "a bot side takes no"), (dict(bot="random", fog_of_war=True), "a bot side takes no"),
    (dict(model=NET, belief=True), "belief=True needs fog_of_war=True"),
    (dict(model=NET, belief_weights=True, fog_of_war=True), "belief_weights=True needs fog_of_war=True and belief=True"),
    (dict(model=NET, belief_evidence=True, fog_of_war=True), "belief_evidence=True needs fog_of_war=True and belief=True"),
    (dict(model=NET, belief_evidence=True, belief=True), "needs fog_of_war=True"),
    (dict(model=NET, fog_of_war=True, sight_range=65), "sight_range must be in 0 .. 64"),
])
def test_match_side_errors(kw, text):
    with pytest.raises(ValueError, match=text):
        MatchSide(**kw)


def test_match_side_keeps_its_regime():
    s = MatchSide(model=NET, greedy=True, fog_of_war=True, sight_range=3, belief=True, belief_weights=True, belief_evidence=True)
    assert (s.greedy, s.fog_of_war, s.sight_range, s.belief, s.belief_weights, s.belief_evidence, s.bot) == (True, True, 3, True, True, True, None)
    for b in ("random", "baseline", "approxq"):
        assert MatchSide(bot=b).model is None


@pytest.mark.parametrize("a, b, kw, text", [
    (MatchSide(model=NET, greedy=True), MatchSide(model=_Net(1), greedy=True), {}, "two greedy networks"),
    (MatchSide(model=NET), MatchSide(bot="baseline"), dict(fog_bots=True), "fog_bots=True needs a bot side whose opponent has fog_of_war=True"),
    (MatchSide(model=NET, fog_of_war=True, sight_range=0), MatchSide(bot="baseline"), dict(fog_bots=True), "sight_range >= 1"),
    (MatchSide(model=NET, fog_of_war=True), MatchSide(model=_Net(1), fog_of_war=True), dict(fog_bots=True), "needs a bot side"),
    (MatchSide(model=NET), MatchSide(bot="baseline"), dict(colours="green"), "colours must be both, red or blue"),
    (NET, MatchSide(bot="baseline"), {}, "takes two MatchSide objects"),
])
def test_play_match_errors_before_anything_runs(a, b, kw, text):
    with pytest.raises(ValueError, match=text):
        play_match(a, b, device="cpu", n_envs=4, **kw)


def test_colour_split():
    assert trainer.match_colours(7, "both").tolist() == [1, 1, 1, 0, 0, 0, 0]          # n // 2 red, the split of _evaluate_sides
    assert trainer.match_colours(4, "red").tolist() == [1] * 4 and trainer.match_colours(4, "blue").tolist() == [0] * 4
    assert trainer.match_colours(4, "both").dtype == torch.uint8


def test_side_seeds():
    seen = {trainer.match_side_seed(s, k) for s in range(50) for k in (0, 1)}
    assert len(seen) == 100                                                          # distinct per side and per seed
    assert trainer.match_side_seed(5, 0) == 10 and trainer.match_side_seed(5, 1) == 11
    assert trainer.match_side_seed(2 ** 31 + 3, 1) == 7                              # 32 bits


class _StubEnv:
    """A scripted game: env e is done at tick e % 3 (0-based) with final score e - 2; red earns 1.0 and blue 0.5 per tick.  The
    statistics stand-in writes what the kernel would for such a game: TICKS, SCORE, DONE and returns that add up to the score."""
    obs_shape = (8, 7, 20)
    obs_torch_dtype = torch.float32

    def __init__(self, n, cheat=None):
        self.n_envs, self.t, self.cheat = n, 0, cheat
        self.legal = torch.full((n, 4), 31, dtype=torch.uint8)
        self.emits, self.acts, self.bot_sight, self.updates, self.closed = [], [], None, [], False

    def reset(self, want_obs=True):
        self.t = 0

    def set_bot_sight(self, s):
        self.bot_sight = s

    def new_episode_stats(self):
        return torch.zeros((L.STATS_WORDS, self.n_envs), dtype=torch.int32)

    def episode_stats_init(self, stats):
        return stats

    def emit_team_obs_mixed(self, red, team_obs, **kw):
        self.emits.append((red.tolist(), dict(kw)))
        team_obs.zero_()

    def new_belief(self):
        return torch.zeros((self.n_envs, 2, 2, 32), dtype=torch.int32)

    def belief_init(self, b, kind):
        return b

    def belief_update(self, red, b, sight, **kw):
        self.updates.append((red.tolist(), sight, sorted(kw)))

    def step(self, acts, want_obs=True):
        n = self.n_envs
        self.acts.append(acts.clone())
        e = torch.arange(n)
        self.done = (e % 3 == self.t).to(torch.uint8)
        rew = torch.tensor([[1.0, 0.5]], dtype=torch.float64).expand(n, 2).contiguous()
        self.score = (e - 2).to(torch.int32)
        self.t += 1
        return None, rew, self.done, {"score": self.score, "legal_actions": self.legal}

    def episode_stats_update(self, stats, done):
        live = stats[L.STATS_W_DONE] == 0
        stats[L.STATS_W_TICKS] += live.to(torch.int32)
        fin = live & done.to(torch.bool)
        sc = self.score if self.cheat != "score" else self.score + 1
        stats[L.STATS_W_SCORE] = torch.where(fin, sc, stats[L.STATS_W_SCORE])
        stats[8 * 0 + L.STAT_RETURNED] = torch.where(fin, self.score.clamp(min=0), stats[8 * 0 + L.STAT_RETURNED])
        stats[8 * 3 + L.STAT_RETURNED] = torch.where(fin, (-self.score).clamp(min=0) + (self.cheat == "returned"), stats[8 * 3 + L.STAT_RETURNED])
        stats[8 * 1 + L.STAT_DEATHS] = torch.where(fin, torch.full_like(self.score, 2), stats[8 * 1 + L.STAT_DEATHS])
        if self.cheat != "done":
            stats[L.STATS_W_DONE] |= fin.to(torch.int32)

    def close(self):
        self.closed = True


def test_loop_and_bookkeeping_on_a_stand_in_env():
    n = 6
    env = _StubEnv(n)
    net = _Net()
    r = play_match(MatchSide(model=net, fog_of_war=True, sight_range=4, belief=True), MatchSide(bot="baseline"), n_envs=n, length=10,
                   colours="both", device="cpu", seed=3, autocast=False, fog_bots=True, env=env)
    assert env.closed and env.bot_sight == 4 and env.t == 3 and net.calls == 3          # stopped when every game was DONE
    red = [1, 1, 1, 0, 0, 0]
    assert all(e[0] == red and set(e[1]) == {"belief"} for e in env.emits) and len(env.emits) == 3
    assert env.updates == [(red, 4, [])] * 3
    # the bot's codes sit in B's columns (blue where A is red), the network's actions in A's
    a0 = env.acts[0]
    assert a0[:3, [1, 3]].tolist() == [[-3, -4]] * 3 and a0[3:, [0, 2]].tolist() == [[-3, -4]] * 3
    assert ((a0[:3, [0, 2]] >= 0) & (a0[:3, [0, 2]] <= 4)).all() and ((a0[3:, [1, 3]] >= 0) & (a0[3:, [1, 3]] <= 4)).all()
    # games: score e - 2 = -2 -1 0 1 2 3, A red in 0..2 -> margins -2 -1 0 | -1 -2 -3
    assert (r["games"], r["wins_a"], r["ties"], r["wins_b"]) == (6, 0, 1, 5) and r["wins_a"] + r["ties"] + r["wins_b"] == r["games"]
    assert r["win_rate_a"] == 0.0 and r["margin_mean"] == pytest.approx(-1.5)
    m = torch.tensor([-2, -1, 0, -1, -2, -3], dtype=torch.float64)
    assert r["margin_sem"] == pytest.approx(float(m.std() / 6 ** 0.5))
    assert r["as_red"]["games"] == 3 and r["as_red"]["margin_mean"] == pytest.approx(-1.0) and r["as_red"]["ties"] == 1
    assert r["as_blue"]["wins_b"] == 3 and r["as_blue"]["margin_mean"] == pytest.approx(-2.0)
    assert r["ticks_mean"] == pytest.approx(2.0)                                       # ticks 1 2 3 1 2 3
    # A's return: twice its colour's reward per counted tick: red 2.0 x (1, 2, 3), blue 1.0 x (1, 2, 3)
    assert r["return_a"] == pytest.approx((2 + 4 + 6 + 1 + 2 + 3) / 6) and r["return_b"] == pytest.approx((1 + 2 + 3 + 2 + 4 + 6) / 6)
    # per-slot means: DEATHS of agent 1 is 2 in every game: A's first slot where A is blue, B's first slot where A is red
    assert r["stats_a"]["deaths"] == [pytest.approx(1.0), 0.0] and r["stats_b"]["deaths"] == [pytest.approx(1.0), 0.0]
    assert r["stats_a"]["returned"][0] == pytest.approx(0.0)                           # agent 0's returns where A is red: scores <= 0 there
    assert r["stats_b"]["returned"][0] == pytest.approx((1 + 2 + 3) / 6)               # agent 0 is B's where A is blue
    assert r["red"].tolist() == red and r["score"].tolist() == [-2, -1, 0, 1, 2, 3] and r["stats"].shape == (48, 6)


def test_sampled_sides_draw_with_their_own_seed_and_the_tick():
    calls = []
    real = trainer.mappo.sample_actions

    def spy(logits, legal=None, seed=0, counter=0, greedy=False):
        calls.append((seed, counter, greedy, legal is not None))
        return real(logits, legal, seed=seed, counter=counter, greedy=greedy)

    trainer.mappo.sample_actions = spy
    try:
        play_match(MatchSide(model=_Net()), MatchSide(model=_Net(1), mask_illegal=True), n_envs=6, length=10, colours="red", device="cpu",
                   seed=9, autocast=False, env=_StubEnv(6))
    finally:
        trainer.mappo.sample_actions = real
    assert calls == [(18, t, False, False) if k == 0 else (19, t, False, True) for t in range(3) for k in (0, 1)]


@pytest.mark.parametrize("cheat, text", [("done", "not DONE"), ("score", "SCORE differs"), ("returned", "RETURNED")])
def test_the_runner_checks_its_record(cheat, text):
    with pytest.raises(RuntimeError, match=text):
        play_match(MatchSide(model=_Net()), MatchSide(bot="random"), n_envs=6, length=10, device="cpu", autocast=False, env=_StubEnv(6, cheat))


def test_bindings_answer_without_a_gpu():
    lib = L.load()
    assert {"pmx_episode_stats_init", "pmx_episode_stats_update"} <= {p[0] for p in L.PROTOTYPES}
    assert lib.pmx_episode_stats_init(None, 0, 1, None, None) == -1 and lib.pmx_episode_stats_update(None, 0, 1, None, None, None) == -1
    assert L.STATS_WORDS == 48 and len(L.STAT_NAMES) == 8 and L.STAT_NAMES[L.STAT_KILLS] == "kills" and L.STAT_STOPS == 7


def test_cli_parses_both_sides():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("pmx_tools_match", os.path.join(root, "tools", "match.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seen = {}
    real = trainer.play_match
    trainer.play_match = lambda a, b, **kw: seen.update(a=a, b=b, kw=kw) or {"games": 0, "red": torch.zeros(1)}
    try:
        out = mod.main(["approxq", "baseline", "--games", "32", "--colours", "red", "--seed", "4", "--layout", "tinyCapture"])
    finally:
        trainer.play_match = real
    assert seen["a"].bot == "approxq" and seen["b"].bot == "baseline"
    assert seen["kw"]["n_envs"] == 32 and seen["kw"]["colours"] == "red" and seen["kw"]["seed"] == 4 and seen["kw"]["layout"] == "tinyCapture"
    assert out["games"] == 0 and "red" not in out and out["a"] == "approxq"
