"""CPU suite of the fog of war: trainer.fog_obs and the host GameState.makeObservation against what the reference's
GameState.makeObservation did on the records of fixture G11 (tests/golden/fog_sight.npz, made by tests/golden/make_golden_fog.py),
the trainer's flag on a stand-in env, and the argument errors of the two new entry points.  No GPU."""
import functools
import random

import numpy as np
import pytest
import torch

import _golden as G
import pmx
from pmx import capture_agents, game_state, trainer

BOARDS = {"small": "smallCapture", "tiny": "tinyCapture", "blox": "bloxCapture"}
DTYPES = (torch.float32, torch.bfloat16, torch.uint8)


@functools.lru_cache(maxsize=None)
def _g11():
    return G.load("fog_sight.npz")


@functools.lru_cache(maxsize=None)
def _source(s):
    """source s of G11: (board, positions [n, 4, 2], reference planes [n, 8, H, W] u8, the rows of G11 that belong to it, and a
    function row -> the state's arrays)"""
    d, meta = _g11()
    name = meta["sources"][s]
    src, _ = G.load(name)
    rows = np.nonzero(d["src"] == s)[0]
    idx, sub = d["idx"][rows], d["sub"][rows]
    if name.startswith("scen"):
        assert (sub == -1).all()
        planes = d["obs_" + name[:-4]]
        fields = {k: src["in_" + k][idx] for k in G.SNAP_KEYS}
    else:
        planes = src["obs"][idx, sub]
        fields = {k: src["sub_" + k][idx, sub] for k in G.SNAP_KEYS}
    assert len(planes) == len(rows)
    board = BOARDS[G.load(name)[1]["layout_name"]]
    return board, fields, planes, rows


def _enemy(observer):
    return (np.arange(4)[None, :] % 2) != (observer[:, None] % 2)


def _expected(s, canonical, shown):
    """the source's reference planes with plane 5 rebuilt from the positions of the enemies `shown` [n, 4] says are seen"""
    d, _ = _g11()
    _, fields, planes, rows = _source(s)
    W = planes.shape[-1]
    enemy = _enemy(d["observer"][rows])
    pos = fields["pos"].astype(np.int64)
    p5 = np.zeros(planes[:, 5].shape, np.uint8)
    full = np.zeros_like(p5)
    for j in range(4):
        x = W - 1 - pos[:, j, 0] if canonical else pos[:, j, 0]
        r = np.nonzero(enemy[:, j])[0]
        full[r, pos[r, j, 1], x[r]] = 1
        r = np.nonzero(enemy[:, j] & shown[:, j].astype(bool))[0]
        p5[r, pos[r, j, 1], x[r]] = 1
    return p5, full


@pytest.mark.parametrize("canonical", (False, True), ids=("raw", "canonical"))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16", "u8"))
def test_fog_obs_clears_exactly_the_enemies_the_reference_hides(dtype, canonical):
    d, meta = _g11()
    for s in range(len(meta["sources"])):
        _, _, planes, rows = _source(s)
        x = torch.from_numpy(planes).to(dtype)
        if canonical:
            x = trainer.canonicalize_obs(x)
        p5, full = _expected(s, canonical, d["vis"][rows])
        assert torch.equal(x[:, 5], torch.from_numpy(full).to(dtype))          # (the reference's plane 5 is where the positions say)
        before = x.clone()
        out = trainer.fog_obs(x)
        assert out.dtype == dtype and out.shape == x.shape and torch.equal(x, before)       # a new tensor, the input untouched
        want = x.clone()
        want[:, 5] = torch.from_numpy(p5).to(dtype)
        assert torch.equal(out, want), meta["sources"][s]
        assert int((want[:, 5] != x[:, 5]).sum()) > 0                              # something was hidden
        # leading dimensions of any rank: [2, n / 2, 8, H, W]
        n2 = len(rows) // 2 * 2
        assert torch.equal(trainer.fog_obs(x[:n2].view((2, n2 // 2) + x.shape[1:])).view((n2,) + x.shape[1:]), want[:n2])


@pytest.mark.parametrize("sight, dist", ((4, 5), (6, 6)))
def test_sight_four_and_six_disagree_with_the_reference_on_the_boundary_records(sight, dist):
    """negative controls: an enemy at distance exactly 5 is seen (sight 4 hides it), one at exactly 6 is not (sight 6 shows it)"""
    d, meta = _g11()
    hit = 0
    for s in range(len(meta["sources"])):
        _, _, planes, rows = _source(s)
        x = torch.from_numpy(planes)
        p5, _ = _expected(s, False, d["vis"][rows])
        out = trainer.fog_obs(x, sight)
        differs = (out[:, 5] != torch.from_numpy(p5)).flatten(1).any(1).numpy()
        boundary = ((d["near"][rows] == dist) & _enemy(d["observer"][rows])).any(1)
        assert boundary.any() and differs[boundary].all(), meta["sources"][s]
        assert torch.equal(out[:, [0, 1, 2, 3, 4, 6, 7]], x[:, [0, 1, 2, 3, 4, 6, 7]])
        hit += int(boundary.sum())
    assert hit >= 20


def test_sight_zero_and_sixty_two():
    d, meta = _g11()
    for s in range(len(meta["sources"])):
        _, _, planes, rows = _source(s)
        x = torch.from_numpy(planes)
        assert torch.equal(trainer.fog_obs(x, 62), x)                                  # the longest distance on a 32 x 32 board
        z = trainer.fog_obs(x, 0)
        team = (x[:, 1] != 0) | (x[:, 4] != 0)
        assert torch.equal(z[:, 5], torch.where(team, x[:, 5], torch.zeros_like(x[:, 5])))
        assert torch.equal(z[:, [0, 1, 2, 3, 4, 6, 7]], x[:, [0, 1, 2, 3, 4, 6, 7]])
    assert trainer.SIGHT_RANGE == game_state.SIGHT_RANGE == 5


def test_fixture_shares():
    """the conditions the generator asserts, recomputed from the stored arrays: hidden and visible each at least 15 % of the
    (observer, enemy) cases, nearest-teammate distance exactly 5 and exactly 6 each at least 1 %, per source and overall"""
    d, meta = _g11()
    for rows in [np.nonzero(d["src"] == s)[0] for s in range(len(meta["sources"]))] + [np.arange(len(d["src"]))]:
        enemy = _enemy(d["observer"][rows])
        n = enemy.sum()
        vis, near = d["vis"][rows].astype(bool), d["near"][rows]
        assert (vis | enemy).all()                                                     # the own team is always seen
        assert ((near <= 5) == vis)[enemy].all()
        assert (~vis & enemy).sum() >= 0.15 * n and (vis & enemy).sum() >= 0.15 * n
        assert ((near == 5) & enemy).sum() >= 0.01 * n and ((near == 6) & enemy).sum() >= 0.01 * n


def _host_state(board, fields, r):
    lay = pmx.get_layout(board)
    st = pmx.make_state(fields["pos"][r], fields["dir"][r], fields["pac"][r], fields["scared"][r], fields["carry"][r], fields["ret"][r],
                        fields["food"][r], fields["caps"][r], fields["score"][r], 0, lay.height)
    return game_state.GameState(lay, _views(board), st, [0] * 4, None)


@functools.lru_cache(maxsize=None)
def _views(board):
    return game_state._LayoutView(pmx.get_layout(board))


def test_host_make_observation_equals_the_reference_record_by_record():
    d, meta = _g11()
    state = random.getstate()
    try:
        for s in range(len(meta["sources"])):
            board, fields, _, rows = _source(s)
            for r, row in enumerate(rows):
                gs = _host_state(board, fields, r)
                assert gs.getAgentDistances() is None                                  # a plain state has no sonar
                observer = int(d["observer"][row])
                random.seed(int(d["k"][row]))
                ob = gs.makeObservation(observer)
                nxt = random.random()
                assert [ob.getAgentPosition(j) is not None for j in range(4)] == d["vis"][row].astype(bool).tolist(), (s, row)
                assert ob.getAgentDistances() == d["sonar"][row].tolist(), (s, row)
                assert nxt == d["nxt"][row], (s, row)                                  # four draws, the reference's
                # the original is untouched, the seen agents are where they were, and the agent API reaches the same method
                assert all(gs.getAgentPosition(j) == tuple(int(v) for v in fields["pos"][r][j]) for j in range(4))
                assert all(ob.getAgentPosition(j) in (None, gs.getAgentPosition(j)) for j in range(4))
                assert all(ob.getAgentState(j).getPosition() is None for j in range(4) if not d["vis"][row][j])
                true = [abs(gs.getAgentPosition(observer)[0] - gs.getAgentPosition(j)[0]) +
                        abs(gs.getAgentPosition(observer)[1] - gs.getAgentPosition(j)[1]) for j in range(4)]
                assert all(ob.getDistanceProb(t, n) == 1.0 / 13 for t, n in zip(true, ob.getAgentDistances()))
        board, fields, _, rows = _source(0)
        gs = _host_state(board, fields, 0)
        assert gs.getDistanceProb(3, 10) == 0 and gs.getDistanceProb(3, -4) == 0 and gs.getDistanceProb(3, 9) == 1.0 / 13
        agent = capture_agents.CaptureAgent(int(d["observer"][rows[0]]))
        random.seed(int(d["k"][rows[0]]))
        ob = agent.observationFunction(gs)
        assert ob.getAgentDistances() == d["sonar"][rows[0]].tolist()
        assert game_state.SONAR_NOISE_RANGE == 13 and game_state.SONAR_NOISE_VALUES == [float(v) for v in range(-6, 7)]
    finally:
        random.setstate(state)


# ---- the trainer's flag on a stand-in env (the stand-in of tests/test_mix_opponents_cpu.py plus what a rollout calls) ------
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

    def _emit(self, name, team_obs, merged, kw):
        assert set(kw) <= {"sight_range"}
        self.calls.append((name + "_fog", kw["sight_range"]) if "sight_range" in kw else (name,))
        team_obs.zero_()
        if merged is not None:
            merged.zero_()

    def emit_team_obs(self, team_red, team_obs, merged=None, **kw):
        self._emit("emit_team_obs", team_obs, merged, kw)

    def emit_team_obs_mixed(self, team_red, team_obs, merged=None, first=0, count=None, **kw):
        self._emit("emit_team_obs_mixed", team_obs, merged, kw)

    def step(self, actions, want_obs=True):
        N = self.n_envs
        info = {"legal_actions": self.legal, "score_change": torch.zeros(N, dtype=torch.int32), "score": torch.zeros(N, dtype=torch.int32),
                "agent": self.agent}
        return None, torch.zeros((N, 2), dtype=torch.float64), torch.zeros(N, dtype=torch.uint8), info

    def close(self):
        pass


def _trainer(opponent="self", **kw):
    return trainer.VecMAPPOTrainer("tinyCapture", 4, horizon=2, minibatch=8, device="cpu", seed=1, use_autocast=False, opponent=opponent,
                                   curriculum_scale=0.1, total_updates=40, env=_StubEnv("tinyCapture", 4), **kw)


@pytest.mark.parametrize("mixed", (False, True), ids=("default", "mix_opponents"))
def test_trainer_default_makes_no_fog_call_and_writes_no_key(tmp_path, mixed):
    tr = _trainer(**({"mix_opponents": True} if mixed else {}))
    assert tr.fog_of_war is False
    tr.rollout()
    name = "emit_team_obs_mixed" if mixed else "emit_team_obs"
    assert tr.env.calls == [(name,)] * (2 * tr.T + 1)                              # learners + opponent network per tick, the bootstrap
    path = str(tmp_path / "off.pt")
    tr.save_full(path)
    ck = torch.load(path, weights_only=True)
    assert "fog_of_war" not in ck and "sight_range" not in ck
    _trainer(**({"mix_opponents": True} if mixed else {})).load_full(path)


@pytest.mark.parametrize("mixed", (False, True), ids=("default", "mix_opponents"))
def test_trainer_fog_flag_reaches_every_emission_and_the_checkpoint(tmp_path, mixed):
    kw = {"mix_opponents": True} if mixed else {}
    tr = _trainer(fog_of_war=True, **kw)
    assert tr.fog_of_war is True and tr.sight_range == 5
    tr.rollout()
    name = "emit_team_obs_mixed_fog" if mixed else "emit_team_obs_fog"
    assert tr.env.calls == [(name, 5)] * (2 * tr.T + 1)
    tr3 = _trainer(fog_of_war=True, sight_range=3, algorithm="ippo", **kw)
    tr3.rollout()
    assert tr3.env.calls == [(name, 3)] * (2 * tr3.T + 1)
    path, path_off = str(tmp_path / "on.pt"), str(tmp_path / "off.pt")
    tr.update_idx = 7
    tr.save_full(path)
    _trainer(**kw).save_full(path_off)
    ck = torch.load(path, weights_only=True)
    assert ck["fog_of_war"] == 1 and ck["sight_range"] == 5
    again = _trainer(fog_of_war=True, **kw)
    again.load_full(path)
    assert again.update_idx == 7
    with pytest.raises(ValueError, match="fog_of_war=True, sight_range=5, this trainer has fog_of_war=False"):
        _trainer(**kw).load_full(path)
    with pytest.raises(ValueError, match="fog_of_war=False, this trainer has fog_of_war=True"):
        _trainer(fog_of_war=True, **kw).load_full(path_off)
    with pytest.raises(ValueError, match="sight_range=5, this trainer has fog_of_war=True, sight_range=3"):
        _trainer(fog_of_war=True, sight_range=3, **kw).load_full(path)
    with pytest.raises(ValueError, match="sight_range"):
        _trainer(fog_of_war=True, sight_range=65)


def test_new_entry_points_argument_errors_without_gpu():
    lib = pmx._lib.load()
    assert pmx._lib.PROTOTYPES and {"pmx_emit_team_obs_fog", "pmx_emit_team_obs_mixed_fog"} <= {p[0] for p in pmx._lib.PROTOTYPES}
    assert lib.pmx_emit_team_obs_fog(None, 0, 5, None, None, None) == -1
    assert b"pmx_emit_team_obs_fog: null" in lib.pmx_last_error()
    assert lib.pmx_emit_team_obs_mixed_fog(None, None, 0, 0, 5, None, None, None) == -1
    assert b"pmx_emit_team_obs_mixed_fog: null" in lib.pmx_last_error()


def test_cli_has_the_flag():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("pmx_tools_train", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                  "tools", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parser().parse_args(["--fog-of-war"])
    assert a.fog_of_war is True and a.sight_range == 5
    a = mod.parser().parse_args(["--fog-of-war", "--sight-range", "3"])
    assert a.sight_range == 3
    assert mod.parser().parse_args([]).fog_of_war is False
