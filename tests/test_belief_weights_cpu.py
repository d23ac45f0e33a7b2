"""CPU suite of the belief weights (include/pmx.h "Belief weights"): the numpy model tests/_belief_weights_ref.py on the golden hunter
trajectories tests/test_belief_cpu.py uses (both colours, sight 5 / 2 / 0, every slot of every tick), its uint32 bounds on an
adversarial board, its two negative controls, the trainer's flag on the stand-in env, and the new entry points' argument errors.
No GPU."""
import functools

import numpy as np
import pytest
import torch

import _belief_ref as B
import _belief_weights_ref as R
import _golden as G
import pmx
from pmx import trainer
from test_belief_cpu import BOARDS, TRAJ, _BeliefStubEnv
from test_fog_cpu import _StubEnv


@functools.lru_cache(maxsize=None)
def _run(name, **knobs):
    """the weighted model over one golden trajectory, six rows at once as tests/test_belief_cpu.py runs the sets.  Counts, over every
    slot of every tick of the envs not just reset: cells where support(q) differs from the set, true cells of weight 0, seen cases
    that are not one cell of 65535, hidden non-empty cases whose maximum is outside 32768 .. 65535, cells where the levels differ
    from the formula, wall cells of non-zero weight; and the hidden cases, the largest support, the uint32 bounds met."""
    d, meta = G.load(name)
    lay = pmx.get_layout(BOARDS[meta["layout_name"]])
    H, W = lay.height, lay.width
    n = 6
    red = np.array([1, 1, 1, 0, 0, 0], bool)
    sight = np.array([5, 2, 0, 5, 2, 0])
    first = np.where(red, 0, 1)
    open_g = np.repeat(B.open_cells(lay.wall_rows, W, H)[None], n, 0)
    starts = np.repeat(lay.starts.astype(np.int64)[None], n, 0)
    words, w, lev = R.init(0, open_g, starts, H, W)
    assert (lev == np.where(B.unpack(words)[..., :H, :W].any(2), 16, 0)).all()
    out = dict(support=0, lost=0, seen_bad=0, max_bad=0, level_bad=0, walls=0, hidden=0, widest=0)
    bounds = {}
    ar = np.arange(n)
    for t in range(len(d["actions"])):
        done = bool(d["resets"][t])
        sub = d["init_pos"][None].repeat(4, 0) if done else d["sub_pos"][t]
        P = np.stack([sub[first], sub[first + 2]], 1)
        w, lev, words, _, seen = R.update(w, words, P, red, sight, np.full(n, t + 1), 77, ar, open_g, starts, H, W, reset=np.full(n, done),
                                          bounds=bounds, **knobs)
        assert w.min() >= 0 and w.max() <= 65535
        sets = B.unpack(words)[..., :H, :W]
        if done:
            assert ((w > 0) == sets).all() and (w[sets] == 65535).all() and (lev == np.where(sets.any(2), 16, 0)).all()
            continue
        out["support"] += int(((w > 0) != sets).sum())
        out["walls"] += int((w * ~open_g[:, None, None, :H, :W]).astype(bool).sum())
        out["level_bad"] += int((lev != np.maximum(*(np.where(w[:, :, k] == 0, 0, 1 + w[:, :, k] // 4096) for k in range(2)))).sum())
        assert lev.max() <= R.LEVELS
        for j in range(2):
            for k in range(2):
                e = P[ar, j, (1 - first) + 2 * k]
                q, sn = w[:, j, k], seen[:, j, k]
                out["lost"] += int((q[ar, e[:, 1], e[:, 0]] == 0).sum())
                one = ((q > 0).sum((1, 2)) == 1) & (q[ar, e[:, 1], e[:, 0]] == 65535)
                out["seen_bad"] += int((sn & ~one).sum())
                top = q.max((1, 2))
                out["max_bad"] += int((~sn & (top > 0) & ((top < 32768) | (top > 65535))).sum())
                out["hidden"] += int((~sn).sum())
                out["widest"] = max(out["widest"], int((q > 0).sum((1, 2))[~sn].max(initial=0)))
    return out, bounds


def _assert_bounds(bounds):
    assert bounds["product"] < 2 ** 32 and bounds["t"] <= 5 * 65535 and bounds["T"] <= 1024 * 5 * 65535 < 2 ** 32 and bounds["u"] < 2 ** 22, bounds


@pytest.mark.parametrize("name", TRAJ)
def test_model_on_the_golden_hunter_trajectories(name):
    out, bounds = _run(name)
    assert out["hidden"] > 300 and out["widest"] > 8, out          # hidden cases with sets of many cells were weighed
    assert out["support"] == 0, out             # support(q) == the set of _belief_ref, cell for cell
    assert out["lost"] == 0, out                # the enemy's true cell has weight > 0
    assert out["seen_bad"] == 0, out            # a seen enemy's weights are one cell of 65535
    assert out["max_bad"] == 0, out             # a hidden enemy's maximum lies in 32768 .. 65535
    assert out["level_bad"] == 0, out
    assert out["walls"] == 0, out
    _assert_bounds(bounds)


def test_bounds_on_an_open_board_of_full_weights():
    """the adversarial case for the header's uint32 bounds: 32 x 32 open cells, every weight 65535, the enemy that moves and the one
    that does not, hidden from two learners in a corner (sight 0, a reading that keeps every cell)"""
    n, H, W = 2, 32, 32
    open_g = np.ones((n, 32, 32), bool)
    starts = np.repeat(np.array([[0, 0], [31, 31], [0, 31], [31, 0]], np.int64)[None], n, 0)
    words, w, _ = R.init(1, open_g, starts, H, W)
    assert (w == 65535).all()
    P = np.repeat(np.array([[0, 0], [31, 31], [1, 0], [30, 31]], np.int64)[None, None], 2, 1).repeat(n, 0)
    bounds = {}
    for red in (True, False):
        for seed in range(8):
            w2, lev, words2, _, seen = R.update(w, words, P, np.full(n, red), 0, np.array([3, 4]), seed, np.arange(n), open_g, starts, H, W,
                                                bounds=bounds)
            assert not seen.any() and w2.max() <= 65535 and ((w2 > 0) == B.unpack(words2)).all()
    _assert_bounds(bounds)
    # the case is near the bounds, not merely inside them: a corner cell (degree 3) makes the largest product, an interior cell and
    # its four neighbours (degree 5) each carry 65535 * 13107 >> 16, and the respawn term adds T >> 7 to one cell
    assert bounds["product"] == 65535 * 21845
    assert bounds["t"] >= 5 * (65535 * 13107 >> 16) and bounds["T"] > 2 ** 25 and bounds["u"] > 2 ** 18


def test_without_the_floor_of_one_the_support_leaves_the_set():
    """control for step 4 / 5: without max(., 1) a cell of the set whose weight rounds to 0 drops out of the support"""
    bad = sum(_run(name, floor=False)[0]["support"] for name in TRAJ)
    assert bad > 0


def test_moving_the_wrong_enemy_breaks_the_support():
    """control for step 2: with the random walk applied to the enemy that did not move -- and not to the one that did -- a cell the
    set has just grown into carries no weight.  The floor of 1 would hide exactly that, so the control runs without it; the line
    above shows the floor alone does not account for all of the damage: this count is larger"""
    wrong = sum(_run(name, floor=False, mover_offset=1)[0]["support"] for name in TRAJ)
    assert wrong > sum(_run(name, floor=False)[0]["support"] for name in TRAJ)


# ---- the trainer's flag on the stand-in env ---------------------------------------------------------------------------------------
class _WeightsStubEnv(_BeliefStubEnv):
    def _emit(self, name, team_obs, merged, kw):
        if "levels" in kw:
            assert set(kw) == {"levels"}
            self.calls.append((name + "_weighted", kw["levels"].data_ptr(), len(kw["levels"])))
            team_obs.zero_()
            if merged is not None:
                merged.zero_()
            return
        super()._emit(name, team_obs, merged, kw)

    def new_belief_weights(self, count=None):
        n, hw = self.n_envs if count is None else count, self.layout.height * self.layout.width
        return torch.zeros((n, 2, 2, hw), dtype=torch.int16), torch.zeros((n, 2, hw), dtype=torch.uint8)

    def belief_weights_init(self, belief, weights, levels, kind=0, first=0, count=None):
        assert len(belief) == len(weights) == len(levels)
        self.calls.append(("winit", belief.data_ptr(), weights.data_ptr(), levels.data_ptr(), kind, first, len(belief) if count is None else count))
        return belief, weights, levels

    def belief_weights_update(self, team_red, belief, weights, levels, sight_range, reset=None, first=0, count=None, sonar=None):
        assert reset is not None and reset.shape == (self.n_envs,) and len(belief) == len(weights) == len(levels)
        red = team_red.tolist() if isinstance(team_red, torch.Tensor) else bool(team_red)
        self.calls.append(("wupdate", belief.data_ptr(), levels.data_ptr(), red, sight_range, first, len(belief) if count is None else count))
        return belief, weights, levels


def _trainer(env_cls, opponent="self", **kw):
    return trainer.VecMAPPOTrainer("tinyCapture", 4, horizon=2, minibatch=8, device="cpu", seed=1, use_autocast=False, opponent=opponent,
                                   curriculum_scale=0.1, total_updates=40, env=env_cls("tinyCapture", 4), **kw)


def test_flag_combinations_that_raise():
    for kw in ({}, {"fog_of_war": True}, {"belief": True}):
        with pytest.raises(ValueError, match="belief_weights=True needs fog_of_war=True and belief=True|belief=True needs fog_of_war=True"):
            _trainer(_WeightsStubEnv, belief_weights=True, **kw)
    with pytest.raises(ValueError, match="belief_weights=True needs"):
        _trainer(_WeightsStubEnv, belief_weights=True, fog_of_war=True)
    with pytest.raises(ValueError, match=r"evaluate_vectorized\(belief_weights=True\)"):
        trainer.evaluate_vs_bots(None, belief_weights=True)
    with pytest.raises(ValueError, match="belief_weights=True needs"):
        trainer.evaluate_vectorized(None, fog_of_war=True, belief_weights=True)


@pytest.mark.parametrize("mixed", (False, True), ids=("default", "mix_opponents"))
def test_flag_off_makes_no_new_call(mixed):
    """_BeliefStubEnv has none of the new methods and rejects the new keyword: with the flag off the calls are the parent's"""
    kw = {"mix_opponents": True} if mixed else {}
    name = "emit_team_obs_mixed_belief" if mixed else "emit_team_obs_belief"
    tr = _trainer(_BeliefStubEnv, fog_of_war=True, belief=True, **kw)
    assert tr.belief_weights is False
    tr.env.calls.clear()
    tr.rollout()
    assert {c[0] for c in tr.env.calls} == {name, "step", "update"}
    tr = _trainer(_StubEnv, **kw)
    assert tr.belief_weights is False
    tr.rollout()


def test_flag_on_every_tracker_call_and_emission_is_the_weighted_form():
    tr = _trainer(_WeightsStubEnv, fog_of_war=True, belief=True, belief_weights=True, sight_range=3)
    (b, w, lv), (ob, ow, olv) = tr._belief[0], tr._belief_opp[0]
    N, T = tr.N, tr.T
    assert tr.env.calls == [("winit", b.data_ptr(), w.data_ptr(), lv.data_ptr(), 0, 0, N), ("winit", ob.data_ptr(), ow.data_ptr(), olv.data_ptr(), 0, 0, N)]
    colours, last = [], None
    for _ in range(6):
        tr.env.calls.clear()
        tr.rollout()
        red = tr.stats["play_as_red"]
        want = []
        if last is not None and red != last:                                              # the colour changed: every open cell
            want += [("winit", b.data_ptr(), w.data_ptr(), lv.data_ptr(), 1, 0, N), ("winit", ob.data_ptr(), ow.data_ptr(), olv.data_ptr(), 1, 0, N)]
        for _t in range(T):
            want += [("emit_team_obs_weighted", lv.data_ptr(), N), ("emit_team_obs_weighted", olv.data_ptr(), N), ("step",),
                     ("wupdate", b.data_ptr(), lv.data_ptr(), red, 3, 0, N), ("wupdate", ob.data_ptr(), olv.data_ptr(), not red, 3, 0, N)]
        want += [("emit_team_obs_weighted", lv.data_ptr(), N)]                            # the bootstrap observation
        assert tr.env.calls == want
        colours.append(red)
        last = red
    assert len(set(colours)) == 2


def test_flag_on_mixed_rollout_and_checkpoint(tmp_path):
    tr = _trainer(_WeightsStubEnv, fog_of_war=True, belief=True, belief_weights=True, mix_opponents=True)
    (b, w, lv), (ob, ow, olv) = tr._belief[0], tr._belief_opp[0]
    N, T = tr.N, tr.T
    tr.env.calls.clear()
    tr.rollout()
    red = tr.team_red.tolist()
    inv = [1 - r for r in red]
    assert tr.env.calls == ([("emit_team_obs_mixed_weighted", lv.data_ptr(), N), ("emit_team_obs_mixed_weighted", olv.data_ptr(), N), ("step",),
                             ("wupdate", b.data_ptr(), lv.data_ptr(), red, 5, 0, N), ("wupdate", ob.data_ptr(), olv.data_ptr(), inv, 5, 0, N)] * T +
                            [("emit_team_obs_mixed_weighted", lv.data_ptr(), N)])
    on, off = str(tmp_path / "on.pt"), str(tmp_path / "off.pt")
    tr.save_full(on)
    plain = _trainer(_BeliefStubEnv, fog_of_war=True, belief=True, mix_opponents=True)
    plain.save_full(off)
    ck_on, ck_off = torch.load(on, weights_only=True), torch.load(off, weights_only=True)
    assert ck_on["belief_weights"] == 1 and "belief_weights" not in ck_off           # written only when on
    assert sorted(set(ck_on) - {"belief_weights"}) == sorted(ck_off)                   # the buffers are not saved
    with pytest.raises(ValueError, match="belief_weights=False"):
        tr.load_full(off)
    with pytest.raises(ValueError, match="belief_weights=True"):
        plain.load_full(on)
    tr.env.calls.clear()
    tr.load_full(on)                                                                   # a resume starts from the open cells
    assert tr.env.calls == [("winit", b.data_ptr(), w.data_ptr(), lv.data_ptr(), 1, 0, N), ("winit", ob.data_ptr(), ow.data_ptr(), olv.data_ptr(), 1, 0, N)]


def test_new_entry_points_argument_errors_without_gpu():
    lib = pmx._lib.load()
    names = {p[0] for p in pmx._lib.PROTOTYPES}
    assert {"pmx_belief_weights_update", "pmx_belief_weights_init", "pmx_emit_team_obs_weighted", "pmx_emit_team_obs_mixed_weighted"} <= names
    assert lib.pmx_belief_weights_update(None, 0, None, 0, 0, 5, None, None, None, None, None, None) == -1
    assert b"pmx_belief_weights_update: null" in lib.pmx_last_error()
    assert lib.pmx_belief_weights_init(None, 0, 0, 0, None, None, None, None) == -1
    assert b"pmx_belief_weights_init: null" in lib.pmx_last_error()
    assert lib.pmx_emit_team_obs_weighted(None, 0, None, None, None, None) == -1
    assert b"pmx_emit_team_obs_weighted: null" in lib.pmx_last_error()
    assert lib.pmx_emit_team_obs_mixed_weighted(None, None, 0, 0, None, None, None, None) == -1
    assert b"pmx_emit_team_obs_mixed_weighted: null" in lib.pmx_last_error()
    assert (pmx._lib.BELIEF_RESPAWN_SHIFT, pmx._lib.BELIEF_LEVELS) == (R.RESPAWN_SHIFT, R.LEVELS) == (7, 16)


def test_cli_has_the_flag():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("pmx_tools_train_belief_weights",
                                                  os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parser().parse_args(["--fog-of-war", "--belief", "--belief-weights"]).belief_weights is True
    assert mod.parser().parse_args([]).belief_weights is False
