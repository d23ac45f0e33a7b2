"""CPU suite of the belief sets (include/pmx.h "Belief sets"): the numpy model tests/_belief_ref.py against the reference's sonar
readings (fixture G11) and the golden hunter trajectories, its negative controls, the trainer's flag on a stand-in env and the
argument errors of the new entry points.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import _belief_ref as R
import _golden as G
import pmx
from pmx import trainer
from test_fog_cpu import _StubEnv

BOARDS = {"small": "smallCapture", "tiny": "tinyCapture", "blox": "bloxCapture"}
TRAJ = ("traj_small_hunter.npz", "traj_blox_hunter.npz", "traj_tiny_hunter.npz")


def _records():
    """the (observer, enemy) records of G11, positions rebuilt from the source fixtures as tests/test_fog_cpu.py does:
    (observer cell [m, 2], enemy cell [m, 2], the reference's reading [m])"""
    d, meta = G.load("fog_sight.npz")
    obs_xy, en_xy, reading = [], [], []
    for s, name in enumerate(meta["sources"]):
        src, _ = G.load(name)
        rows = np.nonzero(d["src"] == s)[0]
        idx, sub = d["idx"][rows], d["sub"][rows]
        pos = (src["in_pos"][idx] if name.startswith("scen") else src["sub_pos"][idx, sub]).astype(np.int64)
        observer = d["observer"][rows].astype(np.int64)
        for e in range(4):
            m = (observer % 2) != (e % 2)
            obs_xy.append(pos[m, observer[m]])
            en_xy.append(pos[m, e])
            reading.append(d["sonar"][rows][m, e].astype(np.int64))
    return np.concatenate(obs_xy), np.concatenate(en_xy), np.concatenate(reading)


def test_noise_width_against_the_reference():
    obs_xy, en_xy, reading = _records()
    assert len(reading) > 5000
    assert sorted(set((reading - R.manhattan(obs_xy, en_xy)).tolist())) == list(range(-6, 7))
    assert (reading < 0).any()                                              # a reading may be negative, as in the reference
    ar = np.arange(len(reading))
    assert R.annulus(obs_xy, reading)[ar, en_xy[:, 1], en_xy[:, 0]].all()   # half-width 6 keeps every enemy
    assert not R.annulus(obs_xy, reading, 5)[ar, en_xy[:, 1], en_xy[:, 0]].all()


def test_the_draw_is_uniform_over_consecutive_keys():
    env, ticks = np.meshgrid(np.arange(256), np.arange(1000, 1256), indexing="ij")
    for seed, agent in ((0, 1), (12345, 14)):
        n = R.noise(seed, env.ravel(), ticks.ravel(), agent)
        values, counts = np.unique(n, return_counts=True)
        assert values.tolist() == list(range(-6, 7))
        share = counts / n.size
        assert (np.abs(share - 1 / 13) <= 0.1 / 13).all(), share


@functools.lru_cache(maxsize=None)
def _run(name, **knobs):
    """the model over one golden trajectory for both colours x sight 5, 2, 0 at once (six rows of one batch).  Returns per row:
    slots in which the set misses the enemy's true cell, seen cases whose set is not one cell, hidden cases whose set is one cell,
    slots in which a wall cell is set, and the numbers of hidden / seen cases."""
    d, meta = G.load(name)
    lay = pmx.get_layout(BOARDS[meta["layout_name"]])
    n = 6
    red = np.array([1, 1, 1, 0, 0, 0], bool)
    sight = np.array([5, 2, 0, 5, 2, 0])
    first = np.where(red, 0, 1)
    open_g = np.repeat(R.open_cells(lay.wall_rows, lay.width, lay.height)[None], n, 0)
    starts = np.repeat(lay.starts.astype(np.int64)[None], n, 0)
    assert (starts[0] == d["init_pos"]).all()
    bel = R.init(0, open_g, starts)
    lost, size, single, walls, hidden, seen_n = (np.zeros(n, np.int64) for _ in range(6))
    ar = np.arange(n)
    for t in range(len(d["actions"])):
        done = bool(d["resets"][t])
        sub = d["init_pos"][None].repeat(4, 0) if done else d["sub_pos"][t]          # a finished env shows the fresh game
        P = np.stack([sub[first], sub[first + 2]], 1)                                 # [n, 2, 4, 2]
        bel, _, seen = R.update(bel, P, red, sight, np.full(n, t + 1), 77, ar, open_g, starts, reset=np.full(n, done), **knobs)
        if done:
            continue
        cells = R.unpack(bel)                                                         # [n, 2, 2, 32, 32]
        walls += (cells & ~open_g[:, None, None]).any((-1, -2)).sum((1, 2))
        for j in range(2):
            for k in range(2):
                e = P[ar, j, (1 - first) + 2 * k]
                lost += ~cells[ar, j, k, e[:, 1], e[:, 0]]
                one = cells[:, j, k].sum((-1, -2)) == 1
                size += seen[:, j, k] & ~one
                single += ~seen[:, j, k] & one
        hidden += (~seen).sum((1, 2))
        seen_n += seen.sum((1, 2))
    return lost, size, single, walls, hidden, seen_n


@pytest.mark.parametrize("name", TRAJ)
def test_sound_on_the_golden_hunter_trajectories(name):
    _, meta = G.load(name)
    assert meta["events"]["deaths"] > 20 and meta["events"]["dones"] >= 2        # kills with respawns, resets
    lost, size, single, walls, hidden, seen = _run(name)
    assert (hidden > 50).all() and (seen[[0, 1, 3, 4]] > 50).all()            # (at sight 0 two agents on one cell is a kill: nothing is seen)
    assert (lost == 0).all(), lost              # the enemy's true cell is in its set, every slot of every tick
    assert (size == 0).all(), size              # a seen enemy's set is one cell (its own, by the line above)
    # The converse does not follow from the rules: a hidden enemy's set is one cell too right after a reset (the reset rule sets the
    # start cell while the enemy stands across the board) and wherever the annulus and the walls leave one candidate.  Such sets
    # are sound like every other (the line on `lost`); they stay a minority of the hidden cases
    assert (single > 0).any() and (2 * single < hidden).all(), (single, hidden)
    assert (walls == 0).all(), walls


def test_without_the_respawn_rule_an_enemy_is_lost():
    """control for rule 3: at sight 2 or 0 a kill happens out of sight of the tracker's team, and the set stays at the place of death"""
    lost = sum(_run(name, rule3=False)[0] for name in TRAJ)
    assert lost[[1, 2, 4, 5]].sum() > 0, lost


def test_dilating_the_wrong_enemy_loses_one():
    """control for rule 2: (a_j + 1) % 4 is the learner's other enemy, which did not move between the two snapshots"""
    lost = sum(_run(name, mover_offset=1)[0] for name in TRAJ)
    assert (lost > 0).all(), lost


# ---- the trainer's flag on the stand-in env of tests/test_fog_cpu.py -------------------------------------------------------------
class _BeliefStubEnv(_StubEnv):
    def _emit(self, name, team_obs, merged, kw):
        assert set(kw) <= {"sight_range", "belief"} and len(kw) <= 1
        if "belief" in kw:
            self.calls.append((name + "_belief", kw["belief"].data_ptr(), len(kw["belief"])))
            team_obs.zero_()
            if merged is not None:
                merged.zero_()
            return
        super()._emit(name, team_obs, merged, kw)

    def new_belief(self, count=None):
        return torch.zeros((self.n_envs if count is None else count, 2, 2, 32), dtype=torch.int32)

    def belief_init(self, belief, kind=0, first=0, count=None):
        self.calls.append(("init", belief.data_ptr(), kind, first, len(belief) if count is None else count))
        return belief

    def belief_update(self, team_red, belief, sight_range, reset=None, first=0, count=None, sonar=None):
        assert reset is not None and reset.shape == (self.n_envs,) and reset.dtype == torch.uint8
        red = team_red.tolist() if isinstance(team_red, torch.Tensor) else bool(team_red)
        self.calls.append(("update", belief.data_ptr(), red, sight_range, first, len(belief) if count is None else count))
        return belief

    def step(self, actions, want_obs=True):
        self.calls.append(("step",))
        return super().step(actions, want_obs)


def _trainer(env_cls, opponent="self", **kw):
    return trainer.VecMAPPOTrainer("tinyCapture", 4, horizon=2, minibatch=8, device="cpu", seed=1, use_autocast=False, opponent=opponent,
                                   curriculum_scale=0.1, total_updates=40, env=env_cls("tinyCapture", 4), **kw)


def test_belief_needs_fog():
    with pytest.raises(ValueError, match="belief=True needs fog_of_war=True"):
        _trainer(_BeliefStubEnv, belief=True)
    with pytest.raises(ValueError, match="evaluate_vectorized"):
        trainer.evaluate_vs_bots(None, belief=True)
    with pytest.raises(ValueError, match="fog_of_war"):
        trainer.evaluate_vectorized(None, belief=True)


@pytest.mark.parametrize("mixed", (False, True), ids=("default", "mix_opponents"))
def test_flag_off_makes_the_calls_made_before(mixed):
    """the stand-in of tests/test_fog_cpu.py has no belief method and rejects every new keyword"""
    kw = {"mix_opponents": True} if mixed else {}
    name = "emit_team_obs_mixed" if mixed else "emit_team_obs"
    tr = _trainer(_StubEnv, **kw)
    assert tr.belief is False
    tr.rollout()
    assert tr.env.calls == [(name,)] * (2 * tr.T + 1)
    tr = _trainer(_StubEnv, fog_of_war=True, **kw)
    tr.rollout()
    assert tr.env.calls == [(name + "_fog", 5)] * (2 * tr.T + 1)


def test_flag_on_one_update_per_step_and_one_init_per_reset_or_colour_change():
    tr = _trainer(_BeliefStubEnv, fog_of_war=True, belief=True, sight_range=3)
    own, opp = tr._belief[0].data_ptr(), tr._belief_opp[0].data_ptr()
    N, T = tr.N, tr.T
    assert tr.env.calls == [("init", own, 0, 0, N), ("init", opp, 0, 0, N)]              # after the constructor's reset
    colours, last = [], None
    for _ in range(6):
        tr.env.calls.clear()
        tr.rollout()
        red = tr.stats["play_as_red"]
        want = []
        if last is not None and red != last:                                              # the colour changed: every open cell
            want += [("init", own, 1, 0, N), ("init", opp, 1, 0, N)]
        for _t in range(T):
            want += [("emit_team_obs_belief", own, N), ("emit_team_obs_belief", opp, N), ("step",),
                     ("update", own, red, 3, 0, N), ("update", opp, not red, 3, 0, N)]
        want += [("emit_team_obs_belief", own, N)]                                        # the bootstrap sees the sets of the last update
        assert tr.env.calls == want
        colours.append(red)
        last = red
    assert len(set(colours)) == 2                                                         # both branches ran


def test_flag_on_bot_opponent_keeps_one_buffer_and_a_resume_starts_from_the_open_cells(tmp_path):
    tr = _trainer(_BeliefStubEnv, opponent="random", fog_of_war=True, belief=True)
    own = tr._belief[0].data_ptr()
    assert tr._belief_opp is None and tr.env.calls == [("init", own, 0, 0, tr.N)]
    tr.env.calls.clear()
    tr.rollout()
    assert tr.env.calls == ([("emit_team_obs_belief", own, tr.N), ("step",), ("update", own, False, 5, 0, tr.N)] * tr.T +
                            [("emit_team_obs_belief", own, tr.N)])
    path, path_fog = str(tmp_path / "belief.pt"), str(tmp_path / "fog.pt")
    tr.save_full(path)
    _trainer(_StubEnv, opponent="random", fog_of_war=True).save_full(path_fog)
    assert sorted(torch.load(path, weights_only=True)) == sorted(torch.load(path_fog, weights_only=True))   # the format is unchanged
    tr.env.calls.clear()
    tr.load_full(path_fog)
    assert tr.env.calls == [("init", own, 1, 0, tr.N)]


def test_flag_on_mixed_rollout_updates_the_network_range_with_the_colours_inverted():
    tr = _trainer(_BeliefStubEnv, fog_of_war=True, belief=True, mix_opponents=True)
    own, opp = tr._belief[0].data_ptr(), tr._belief_opp[0].data_ptr()
    N, T = tr.N, tr.T
    for _ in range(2):                                                                    # the plan does not change: no second init
        tr.env.calls.clear()
        tr.rollout()
        red = tr.team_red.tolist()
        assert red == [1, 1, 0, 0]
        inv = [1 - r for r in red]
        assert tr.env.calls == ([("emit_team_obs_mixed_belief", own, N), ("emit_team_obs_mixed_belief", opp, N), ("step",),
                                 ("update", own, red, 5, 0, N), ("update", opp, inv, 5, 0, N)] * T +
                                [("emit_team_obs_mixed_belief", own, N)])


def test_new_entry_points_argument_errors_without_gpu():
    lib = pmx._lib.load()
    names = {p[0] for p in pmx._lib.PROTOTYPES}
    assert {"pmx_belief_update", "pmx_belief_init", "pmx_emit_team_obs_belief", "pmx_emit_team_obs_mixed_belief"} <= names
    assert lib.pmx_belief_update(None, 0, None, 0, 0, 5, None, None, None, None) == -1
    assert b"pmx_belief_update: null" in lib.pmx_last_error()
    assert lib.pmx_belief_init(None, 0, 0, 0, None, None) == -1
    assert b"pmx_belief_init: null" in lib.pmx_last_error()
    assert lib.pmx_emit_team_obs_belief(None, 0, None, None, None, None) == -1
    assert b"pmx_emit_team_obs_belief: null" in lib.pmx_last_error()
    assert lib.pmx_emit_team_obs_mixed_belief(None, None, 0, 0, None, None, None, None) == -1
    assert b"pmx_emit_team_obs_mixed_belief: null" in lib.pmx_last_error()
    assert pmx._lib.SALT_SONAR == R.SALT_SONAR


def test_cli_has_the_flag():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("pmx_tools_train_belief", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                         "tools", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parser().parse_args(["--fog-of-war", "--belief"]).belief is True
    assert mod.parser().parse_args([]).belief is False
