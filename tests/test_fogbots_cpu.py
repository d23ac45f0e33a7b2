"""CPU suite of the fog-bound bots: tests/_fogbots_model.py against what the reference's baselineTeam / approxQTeam agents
computed on their own observations (fixture G12, tests/golden/fogbots.npz, made by tests/golden/make_golden_fogbots.py), negative
controls that show the fixture can tell the rule from its neighbours, the fixture's shares and floors, and the flag's
validation in the trainer, the evaluations and the command line on a stand-in env.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _fogbots_model as FB
import pmx
from pmx import trainer

DEFENDERS = (FB.BASE_DEF, FB.AQ_DEF)
MIN_HIDDEN_SHARE, MIN_BOTH, MIN_G_DIFFERS, MAX_DROP_SHARE = 0.05, 5, 40, 0.03


def _records(sel=None):
    rec, _, sources, _ = FB.load_g12()
    for k in (np.arange(len(rec["row"])) if sel is None else np.nonzero(sel)[0]):
        s = int(rec["src"][k])
        yield k, s, sources[s]["states"][sources[s]["local"][int(rec["row"][k])]]


def _hidden_invader(rec, d11):
    """per record: an enemy that is a Pacman and is not seen; and also one that is a Pacman and seen"""
    _, _, sources, _ = FB.load_g12()
    hid, both = np.zeros(len(rec["row"]), bool), np.zeros(len(rec["row"]), bool)
    for k, s, st in _records():
        pac = [bool(st["pac"][o]) for o in FB.foes(int(rec["agent"][k]))]
        h = any(p and not v for p, v in zip(pac, rec["seen"][k]))
        hid[k], both[k] = h, h and any(p and v for p, v in zip(pac, rec["seen"][k]))
    return hid, both


@pytest.fixture(scope="module")
def evaluated():
    """the model's evaluation of every G12 record at the record's sight, computed once"""
    rec = FB.load_g12()[0]
    return {k: FB.model_of(s).evaluate(st, int(rec["agent"][k]), int(rec["code"][k]), sight=int(rec["sight"][k])) for k, s, st in _records()}


def test_model_equals_the_reference_on_every_record(evaluated):
    rec, meta, sources, d11 = FB.load_g12()
    n = len(rec["row"])
    assert n > 9000 and set(np.unique(rec["sight"])) == {1, 5} and set(np.unique(rec["code"])) == {-3, -4, -5, -6}
    for k in range(n):
        ev = evaluated[k]
        assert ev["values"].tobytes() == rec["values"][k].tobytes(), (k, ev["values"], rec["values"][k])
        assert (ev["legal"], ev["best"], ev["home"]) == (int(rec["legal"][k]), int(rec["best"][k]), int(rec["home"][k])), k
        assert list(ev["seen"]) == [bool(v) for v in rec["seen"][k]], k
        assert ev["food_left"] == int(rec["food_left"][k]), k
        if rec["code"][k] == FB.AQ_OFF:
            legal = [a for a in range(5) if (ev["legal"] >> a) & 1]
            assert [int(ev["g"][a]) for a in legal] == [int(rec["g_obs"][k][a]) for a in legal], k


def test_seen_flags_at_sight_five_are_g11s():
    rec, _, _, d11 = FB.load_g12()
    five = rec["sight"] == 5
    for k in np.nonzero(five)[0]:
        vis = d11["vis"][rec["row"][k]]
        assert [bool(vis[o]) for o in FB.foes(int(rec["agent"][k]))] == [bool(v) for v in rec["seen"][k]], k
        assert int(rec["agent"][k]) == int(d11["observer"][rec["row"][k]])


def test_controls_equal_the_full_state_values():
    """Where the rule cannot bite -- the offensive reflex agent, and the forager at sight 5 -- the reference's values on the
    observation are the full-state model's."""
    rec = FB.load_g12()[0]
    sel = (rec["code"] == FB.BASE_OFF) | ((rec["code"] == FB.AQ_OFF) & (rec["sight"] == 5))
    assert sel.sum() >= 600
    for k, s, st in _records(sel):
        ev = FB.Model.evaluate(FB.model_of(s), st, int(rec["agent"][k]), int(rec["code"][k]))
        assert ev["values"].tobytes() == rec["values"][k].tobytes(), k


def test_full_state_model_disagrees_on_every_hidden_invader_record():
    rec, _, _, d11 = FB.load_g12()
    hid, _ = _hidden_invader(rec, d11)
    sel = hid & np.isin(rec["code"], DEFENDERS) & (rec["sight"] == 5)
    assert sel.sum() >= 2 * 428 - 20                                    # both defender codes on the 428 such rows, less the dropped ones
    for k, s, st in _records(sel):
        ev = FB.model_of(s).evaluate(st, int(rec["agent"][k]), int(rec["code"][k]), sight=None)
        assert ev["values"].tobytes() != rec["values"][k].tobytes(), k


@pytest.mark.parametrize("sight, dist", [(4, 5), (6, 6)])
def test_sight_four_and_six_disagree_on_the_boundary_rows(sight, dist):
    """A defender record whose invader is at exactly `dist` cells from the nearer team agent: seen at 5 iff dist == 5, and
    the other way round at `sight`, so the value of every action changes by the invader term."""
    rec, _, _, d11 = FB.load_g12()
    sel = np.zeros(len(rec["row"]), bool)
    for k, s, st in _records(np.isin(rec["code"], DEFENDERS) & (rec["sight"] == 5)):
        near = d11["near"][rec["row"][k]]
        sel[k] = any(st["pac"][o] and near[o] == dist for o in FB.foes(int(rec["agent"][k])))
    assert sel.sum() >= 20, sel.sum()
    for k, s, st in _records(sel):
        ev = FB.model_of(s).evaluate(st, int(rec["agent"][k]), int(rec["code"][k]), sight=sight)
        assert ev["values"].tobytes() != rec["values"][k].tobytes(), k


def test_visibility_from_the_successor_disagrees_somewhere():
    """The reference hides an enemy once, before any successor exists; deciding it per successor is a different bot."""
    rec = FB.load_g12()[0]
    n = 0
    for k, s, st in _records(np.isin(rec["code"], DEFENDERS) & (rec["sight"] == 5)):
        ev = FB.model_of(s).evaluate(st, int(rec["agent"][k]), int(rec["code"][k]), sight=5, seen_from_successor=True)
        n += ev["values"].tobytes() != rec["values"][k].tobytes()
    print(f"defender records at sight 5 on which visibility taken from the successor changes a value: {n}")
    assert n >= 1


def test_fixture_shares_and_floors():
    rec, meta, sources, d11 = FB.load_g12()
    hid, both = _hidden_invader(rec, d11)
    for s, src in enumerate(sources):
        d5 = (rec["src"] == s) & (rec["code"] == FB.BASE_DEF) & (rec["sight"] == 5)
        kept = len(set(rec["row"][d5]))
        assert kept == d5.sum() and len(src["rows"]) - kept <= MAX_DROP_SHARE * len(src["rows"]), src["name"]
        assert hid[d5].sum() >= MIN_HIDDEN_SHARE * d5.sum(), (src["name"], hid[d5].sum(), d5.sum())
        assert both[d5].sum() >= MIN_BOTH, (src["name"], both[d5].sum())
        m = meta["per_source"][src["name"]]
        assert (m["hidden"], m["both"], m["defender_records"]) == (int(hid[d5].sum()), int(both[d5].sum()), int(d5.sum()))
        # every kept row carries both defenders at sight 5 and the forager at sight 1
        for code, sight in ((FB.AQ_DEF, 5), (FB.AQ_OFF, 1)):
            assert set(rec["row"][(rec["src"] == s) & (rec["code"] == code) & (rec["sight"] == sight)]) == set(rec["row"][d5])
    f1 = (rec["code"] == FB.AQ_OFF) & (rec["sight"] == 1)
    differs = int(((rec["g_obs"] != rec["g_full"]).any(axis=1) & f1).sum())
    assert differs >= MIN_G_DIFFERS and differs == meta["g_differs"] and meta["synthesised"] == 0
    f5 = (rec["code"] == FB.AQ_OFF) & (rec["sight"] == 5)
    assert (rec["g_obs"][f5] == rec["g_full"][f5]).all()


@pytest.mark.parametrize("name", ["bots_small_baselineTeam_fog.json", "bots_blox_approxQTeam_fog.json"])
def test_traces_hold_hidden_invader_turns(name):
    import _golden as G
    g = G.load_json(name)
    # hidden_turns: the defender's turns outside the walk home with a hidden invader, the turns the host rule can change
    assert g["fog_bots"] is True and 10 <= g["hidden_turns"] <= g["hidden_turns_any_bot"]
    assert len(g["blue_actions"]) == 320 == len(g["red_actions"])


# ---- the flag on a stand-in env -----------------------------------------------------------------------------------------------
class _StubEnv:
    def __init__(self, layout, n_envs):
        from pmx.layout import get_layout
        self.layout = get_layout(layout)
        self.obs_torch_dtype = torch.float32
        self.n_envs = n_envs
        self.calls = []
        self.legal = torch.full((n_envs, 4), 31, dtype=torch.uint8)
        self.agent = torch.zeros((n_envs, 4), dtype=torch.int32)

    def reset(self):
        return torch.zeros((self.n_envs, 4, 8, self.layout.height, self.layout.width)), None

    def set_bot_sight(self, sight_range=None):
        self.calls.append(("set_bot_sight", sight_range))

    def emit_team_obs(self, team_red, team_obs, merged=None, **kw):
        team_obs.zero_()
        if merged is not None:
            merged.zero_()

    emit_team_obs_mixed = emit_team_obs

    def step(self, actions, want_obs=True):
        N = self.n_envs
        info = {"legal_actions": self.legal, "score_change": torch.zeros(N, dtype=torch.int32), "score": torch.zeros(N, dtype=torch.int32),
                "agent": self.agent}
        return None, torch.zeros((N, 2), dtype=torch.float64), torch.zeros(N, dtype=torch.uint8), info

    def close(self):
        pass


def _trainer(opponent="baseline", **kw):
    return trainer.VecMAPPOTrainer("tinyCapture", 4, horizon=2, minibatch=8, device="cpu", seed=1, use_autocast=False, opponent=opponent,
                                   curriculum_scale=0.1, total_updates=40, env=_StubEnv("tinyCapture", 4), **kw)


def test_trainer_sets_the_bot_sight_once_and_only_with_the_flag(tmp_path):
    off = _trainer(fog_of_war=True)
    assert off.fog_bots is False
    off.rollout()
    assert off.env.calls == []                                             # flag off: no new call
    on = _trainer(fog_of_war=True, fog_bots=True)
    on.rollout()
    assert on.fog_bots is True and on.env.calls == [("set_bot_sight", 5)]
    assert _trainer(fog_of_war=True, sight_range=3, fog_bots=True).env.calls == [("set_bot_sight", 3)]
    assert _trainer(opponent="curriculum", fog_of_war=True, fog_bots=True).env.calls == [("set_bot_sight", 5)]
    assert _trainer(opponent="self", fog_of_war=True, fog_bots=True).env.calls == []        # an env without bots: nothing to bind
    # nothing is recorded: a checkpoint of one loads into the other
    path = str(tmp_path / "on.pt")
    on.save_full(path)
    ck = torch.load(path, weights_only=True)
    assert "fog_bots" not in ck
    off.load_full(path)


def test_flag_validation():
    with pytest.raises(ValueError, match="fog_bots=True needs fog_of_war=True and sight_range >= 1"):
        _trainer(fog_bots=True)
    with pytest.raises(ValueError, match="fog_bots=True needs fog_of_war=True and sight_range >= 1"):
        _trainer(fog_of_war=True, sight_range=0, fog_bots=True)
    model = object()
    with pytest.raises(ValueError, match="fog_bots=True needs fog_of_war=True and sight_range >= 1"):
        trainer.evaluate_vectorized(model, fog_bots=True)
    with pytest.raises(ValueError, match="fog_bots=True needs fog_of_war=True and sight_range >= 1"):
        trainer.evaluate_vectorized(model, fog_of_war=True, sight_range=0, fog_bots=True)
    with pytest.raises(ValueError, match="fog_bots=True needs fog_of_war=True and sight_range >= 1"):
        trainer._evaluate_sides(model, "tinyCapture", 4, "baseline", 10, "cpu", 0, False, False, "blue", None, fog_bots=True)
    with pytest.raises(ValueError, match="fog_bots=True needs fog_of_war=True"):
        trainer.evaluate_vs_bots(model, fog_bots=True)
    with pytest.raises(ValueError, match="SIGHT_RANGE = 5, got sight_range=3"):
        trainer.evaluate_vs_bots(model, fog_of_war=True, sight_range=3, fog_bots=True)
    with pytest.raises(ValueError, match="no belief tracker"):
        trainer.evaluate_vs_bots(model, fog_of_war=True, belief=True, fog_bots=True)


def test_entry_point_argument_errors_without_gpu():
    lib = pmx._lib.load()
    assert "pmx_set_bot_sight" in {p[0] for p in pmx._lib.PROTOTYPES} and pmx._lib.BOT_SIGHT_OFF == -1
    for sight in (-1, 5, 0, 65):
        assert lib.pmx_set_bot_sight(None, sight) == -1
        assert b"pmx_set_bot_sight: null" in lib.pmx_last_error()


def test_cli_has_the_flags():
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    spec = importlib.util.spec_from_file_location("pmx_tools_train_fogbots", os.path.join(tools, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parser().parse_args(["--fog-of-war", "--fog-bots"]).fog_bots is True
    assert mod.parser().parse_args(["--fog-of-war"]).fog_bots is False
    spec = importlib.util.spec_from_file_location("pmx_tools_bots_time_fogbots", os.path.join(tools, "bots_time.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parser().parse_args(["--bot-sight", "5"])
    assert a.bot_sight == 5 and a.ticks == 500 and mod.parser().parse_args([]).bot_sight is None
