"""CPU suite of the belief evidence (include/pmx.h "Belief evidence"): the numpy model tests/_belief_evidence_ref.py on the golden
hunter trajectories -- sound under every rule mask, a subset of the parent model's sets, equal to it under mask 0, tighter by the
margins of the issue under mask 7 -- its negative controls, the trainer's flag on a stand-in env and the argument errors of the new
entry points.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import _belief_evidence_ref as E
import _belief_ref as R
import _golden as G
import pmx
from pmx import trainer
from test_belief_cpu import BOARDS, TRAJ, _BeliefStubEnv, _trainer
from test_belief_weights_cpu import _WeightsStubEnv
from test_fog_cpu import _StubEnv

RED = np.array([1, 1, 1, 0, 0, 0], bool)
SIGHT = np.array([5, 2, 0, 5, 2, 0])


def _pad(rows):
    out = np.zeros(rows.shape[:-1] + (32,), np.uint32)
    out[..., :rows.shape[-1]] = rows
    return out


def _snapshots(d, t, first):
    """(P [n, 2, 4, 2], F [n, 2, 32], done) of tick t for learners of the colours `first`: a finished env shows the fresh game"""
    done = bool(d["resets"][t])
    sub = d["init_pos"][None].repeat(4, 0) if done else d["sub_pos"][t]
    food = _pad(d["init_food"][None].repeat(4, 0) if done else d["sub_food"][t])
    return np.stack([sub[first], sub[first + 2]], 1), np.stack([food[first], food[first + 2]], 1), done


@functools.lru_cache(maxsize=None)
def _run(name, rules, **knobs):
    """the evidence model and the parent model side by side over one golden trajectory, both colours x sight 5, 2, 0 (six rows of one
    batch), all on the noise stream of seed 77, env 0.  Per row: slots that miss the enemy's true cell, slots with a wall cell set,
    slots that are no subset of the parent's, slots that differ from the parent's, hidden cases, their cells and far-start cases
    (the set holds the enemy's start cell while the enemy is more than 6 cells from it) for the evidence and the parent model, and
    the food rule's two counters."""
    d, meta = G.load(name)
    lay = pmx.get_layout(BOARDS[meta["layout_name"]])
    n = 6
    first = np.where(RED, 0, 1)
    open_g = np.repeat(R.open_cells(lay.wall_rows, lay.width, lay.height)[None], n, 0)
    starts = np.repeat(lay.starts.astype(np.int64)[None], n, 0)
    bel = par = R.init(0, open_g, starts)
    ev = E.init(n)
    z = lambda: np.zeros(n, np.int64)
    out = dict(lost=z(), walls=z(), not_subset=z(), differs=z(), hidden=z(), cells=z(), far=z(), par_cells=z(), par_far=z())
    stats = {}
    ar, env = np.arange(n), np.zeros(n, np.int64)
    for t in range(len(d["actions"])):
        P, F, done = _snapshots(d, t, first)
        args = (P, RED, SIGHT, np.full(n, t + 1), 77, env, open_g, starts)
        par, _, seen = R.update(par, *args, reset=np.full(n, done))
        bel, _, seen_e, ev = E.update(bel, ev, P, F, RED, SIGHT, np.full(n, t + 1), 77, env, open_g, starts, lay.width // 2, rules=rules,
                                      reset=np.full(n, done), stats=stats, **knobs)
        assert (seen == seen_e).all()
        if done:
            continue
        cells, pcells = R.unpack(bel), R.unpack(par)
        out["walls"] += (cells & ~open_g[:, None, None]).any((-1, -2)).sum((1, 2))
        out["not_subset"] += (cells & ~pcells).any((-1, -2)).sum((1, 2))
        out["differs"] += (bel != par).any(-1).sum((1, 2))
        for j in range(2):
            for k in range(2):
                e_k = (1 - first) + 2 * k
                e = P[ar, j, e_k]
                out["lost"] += ~cells[ar, j, k, e[:, 1], e[:, 0]]
                s = starts[ar, e_k]
                h = ~seen[:, j, k]
                away = R.manhattan(e, s) > 6
                out["hidden"] += h
                out["cells"] += np.where(h, cells[:, j, k].sum((-1, -2)), 0)
                out["par_cells"] += np.where(h, pcells[:, j, k].sum((-1, -2)), 0)
                out["far"] += h & away & cells[ar, j, k, s[:, 1], s[:, 0]]
                out["par_far"] += h & away & pcells[ar, j, k, s[:, 1], s[:, 0]]
    out["food"], out["excluded"] = stats.get("food", z()), stats.get("excluded", z())
    return out


@pytest.mark.parametrize("name", TRAJ)
def test_the_pacman_flag_is_the_side_and_one_pellet_leaves_per_window(name):
    d, meta = G.load(name)
    half = pmx.get_layout(BOARDS[meta["layout_name"]]).width // 2
    x = d["sub_pos"][..., 0].astype(np.int64)                               # [t, sub-step, agent]
    on_other_half = np.where(np.arange(4) % 2 == 0, x >= half, x < half)
    assert (d["sub_pac"].astype(bool) == on_other_half).all()
    lo = np.uint32((1 << half) - 1)
    most = 0
    for first in (0, 1):
        mine = lo if first == 0 else ~lo
        before = None
        for t in range(len(d["actions"])):
            _, F, done = _snapshots(d, t, np.array([first]))
            for j in range(2):
                if before is not None and not done:         # (a reset replaces the board: pellets dumped on once-empty cells go)
                    gone = before & ~F[0, j] & mine
                    most = max(most, sum(bin(int(w)).count("1") for w in gone))
                before = F[0, j]
    assert most == 1


@pytest.mark.parametrize("rules", (1, 2, 4, 7))
@pytest.mark.parametrize("name", TRAJ)
def test_sound_and_within_the_parent_sets(name, rules):
    r = _run(name, rules)
    assert (r["hidden"] > 50).all()
    assert (r["lost"] == 0).all(), r["lost"]                # the enemy's true cell is in its set, every slot of every tick
    assert (r["walls"] == 0).all(), r["walls"]
    assert (r["not_subset"] == 0).all(), r["not_subset"]
    assert (r["differs"] > 0).all(), r["differs"]           # (each rule alone removes something on every row)


@pytest.mark.parametrize("name", TRAJ)
def test_mask_0_is_the_parent_model(name):
    r = _run(name, 0)
    assert (r["differs"] == 0).all() and (r["lost"] == 0).all()
    assert (r["cells"] == r["par_cells"]).all() and (r["far"] == r["par_far"]).all()


@pytest.mark.parametrize("name", TRAJ)
def test_all_three_rules_tighten_the_sets_at_sight_5(name):
    r = _run(name, 7)
    for row in (0, 3):                                      # sight 5, red and blue learners
        print(name, "blue" if row else "red", "cells", r["cells"][row] / r["hidden"][row], "parent", r["par_cells"][row] / r["hidden"][row],
              "far", r["far"][row] / r["hidden"][row], "parent", r["par_far"][row] / r["hidden"][row], "food", r["food"][row],
              "excluded", r["excluded"][row])
        assert r["par_far"][row] > 0
        assert 4 * r["far"][row] <= r["par_far"][row]       # (the hidden cases are the same: seen does not depend on the rules)
        assert 10 * r["cells"][row] <= 9 * r["par_cells"][row]
        assert r["food"][row] > 30


def test_the_exclusion_clause_fires():
    assert sum(int(_run(name, 7)["excluded"][[0, 3]].sum()) for name in TRAJ) >= 1


def test_with_the_halves_swapped_an_enemy_is_lost():
    lost = sum(_run(name, 1, side_swap=True)["lost"] for name in TRAJ)
    assert (lost > 0).all(), lost


def test_the_food_rule_on_the_enemy_that_did_not_move_loses_it():
    lost = sum(_run(name, 2, food_offset=1)["lost"] for name in TRAJ)
    assert (lost > 0).all(), lost


def test_contact_at_radius_0_of_the_current_cells_loses_an_enemy():
    """a kill is a collision with where a team agent WAS, or one step from it: the cells it stands on now are too few"""
    lost = sum(_run(name, 4, contact="current")["lost"] for name in TRAJ)
    assert lost[[0, 3]].sum() > 0, lost


# ---- the trainer's flag on the stand-in envs of tests/test_belief_cpu.py and tests/test_belief_weights_cpu.py ---------------------
def _evidence_stub(base):
    class Stub(base):
        def new_belief_evidence(self, count=None):
            return torch.zeros((self.n_envs if count is None else count, 36), dtype=torch.int32)

        def belief_evidence_init(self, evidence, first=0, count=None):
            self.calls.append(("evidence_init", evidence.data_ptr(), first, len(evidence) if count is None else count))
            return evidence

        def belief_update(self, team_red, belief, sight_range, reset=None, first=0, count=None, sonar=None, evidence=None, rules=7):
            super().belief_update(team_red, belief, sight_range, reset=reset, first=first, count=count, sonar=sonar)
            assert evidence is not None and rules == 7 and len(evidence) == len(belief)
            self.calls[-1] += (evidence.data_ptr(),)
            return belief

        def belief_weights_update(self, team_red, belief, weights, levels, sight_range, reset=None, first=0, count=None, sonar=None,
                                  evidence=None, rules=7):
            super().belief_weights_update(team_red, belief, weights, levels, sight_range, reset=reset, first=first, count=count, sonar=sonar)
            assert evidence is not None and rules == 7 and len(evidence) == len(belief)
            self.calls[-1] += (evidence.data_ptr(),)
            return belief, weights, levels
    return Stub


def _sets_of(buf):
    return buf[0][0] if isinstance(buf[0], tuple) else buf[0]


def _pairs(calls):
    """every belief init of a call list, as ("init", sets pointer, kind, first, count), with the call that follows it, and the updates"""
    plain = lambda c: ("init", c[1]) + tuple(c[-3:])       # ("winit", sets, weights, levels, kind, first, count) likewise
    inits = [(plain(c), calls[i + 1] if i + 1 < len(calls) else None) for i, c in enumerate(calls) if c[0] in ("init", "winit")]
    return inits, [c for c in calls if c[0] in ("update", "wupdate")]


@pytest.mark.parametrize("weights", (False, True), ids=("sets", "weights"))
def test_flag_off_makes_the_calls_made_before(weights):
    """the parents' stand-ins have no evidence method and reject the new keywords"""
    stub = _WeightsStubEnv if weights else _BeliefStubEnv
    kw = {"belief_weights": True} if weights else {}
    tr = _trainer(stub, fog_of_war=True, belief=True, mix_opponents=True, **kw)
    assert tr.belief_evidence is False and tr._belief[2] is None
    tr.rollout()
    assert not any("evidence" in c[0] for c in tr.env.calls)
    assert _pairs(tr.env.calls)[1]


@pytest.mark.parametrize("mixed", (False, True), ids=("default", "mix_opponents"))
@pytest.mark.parametrize("weights", (False, True), ids=("sets", "weights"))
def test_flag_on_one_evidence_init_per_belief_init_and_evidence_at_every_update(weights, mixed):
    stub = _evidence_stub(_WeightsStubEnv if weights else _BeliefStubEnv)
    kw = dict(**({"belief_weights": True} if weights else {}), **({"mix_opponents": True} if mixed else {}))
    tr = _trainer(stub, fog_of_war=True, belief=True, belief_evidence=True, **kw)
    assert tr._belief_opp is not None
    ev_of = {_sets_of(b).data_ptr(): b[2].data_ptr() for b in (tr._belief, tr._belief_opp)}
    assert len(set(ev_of.values())) == 2
    width = {p: _sets_of(b)[0].numel() * 4 for b in (tr._belief, tr._belief_opp) for p in (_sets_of(b).data_ptr(),)}
    n_init = n_update = 0
    for i in range(6):                                      # (the constructor's calls are in the first list)
        if mixed and i:                                     # the plan of a mixed rollout does not change by itself: mark rows 1 and 2
            for b in (tr._belief, tr._belief_opp):          # as having missed the last rollout, so that a range is re-initialised
                b[1][1:3] = 2
        tr.rollout()
        inits, updates = _pairs(tr.env.calls)
        for c, nxt in inits:                                # ("init", pointer, kind, first, count): a range starts at row `first`
            base = next(p for p in ev_of if p <= c[1] < p + width[p] * tr.N)
            row = (c[1] - base) // width[base]
            assert nxt == ("evidence_init", ev_of[base] + 144 * row, c[3], c[4]), (c, nxt)
        assert sum(c[0] == "evidence_init" for c in tr.env.calls) == len(inits)
        for c in updates:                                   # ("update", pointer, red, sight, first, count, evidence pointer)
            assert c[-1] == ev_of[c[1]], c
        n_init += len(inits)
        n_update += len(updates)
        tr.env.calls.clear()
    assert n_update == 6 * 2 * tr.T and n_init > 2          # both buffers at every step; re-initialisations beyond the constructor's


def test_flag_on_a_resume_initialises_the_evidence_too(tmp_path):
    stub = _evidence_stub(_BeliefStubEnv)
    tr = _trainer(stub, opponent="random", fog_of_war=True, belief=True, belief_evidence=True)
    own, ev = tr._belief[0].data_ptr(), tr._belief[2].data_ptr()
    assert tr._belief_opp is None and tr.env.calls == [("init", own, 0, 0, tr.N), ("evidence_init", ev, 0, tr.N)]
    path, path_fog = str(tmp_path / "evidence.pt"), str(tmp_path / "fog.pt")
    tr.save_full(path)
    _trainer(_StubEnv, opponent="random", fog_of_war=True).save_full(path_fog)
    assert sorted(torch.load(path, weights_only=True)) == sorted(torch.load(path_fog, weights_only=True))   # the format is unchanged
    tr.env.calls.clear()
    tr.load_full(path_fog)
    assert tr.env.calls == [("init", own, 1, 0, tr.N), ("evidence_init", ev, 0, tr.N)]


def test_belief_evidence_needs_belief():
    with pytest.raises(ValueError, match="belief_evidence=True needs"):
        _trainer(_BeliefStubEnv, fog_of_war=True, belief_evidence=True)
    with pytest.raises(ValueError, match="belief_evidence=True needs"):
        trainer.evaluate_vectorized(None, fog_of_war=True, belief_evidence=True)


def test_new_entry_points_argument_errors_without_gpu():
    lib = pmx._lib.load()
    names = {p[0] for p in pmx._lib.PROTOTYPES}
    assert {"pmx_belief_evidence_init", "pmx_belief_update_evidence", "pmx_belief_weights_update_evidence"} <= names
    assert lib.pmx_belief_evidence_init(None, 0, 0, None, None) == -1
    assert b"pmx_belief_evidence_init: null" in lib.pmx_last_error()
    assert lib.pmx_belief_update_evidence(None, 0, None, 0, 0, 5, 7, None, None, None, None, None) == -1
    assert b"pmx_belief_update_evidence: null" in lib.pmx_last_error()
    assert lib.pmx_belief_weights_update_evidence(None, 0, None, 0, 0, 5, 7, None, None, None, None, None, None, None) == -1
    assert b"pmx_belief_weights_update_evidence: null" in lib.pmx_last_error()
    L = pmx._lib
    assert (L.EVIDENCE_SIDE, L.EVIDENCE_FOOD, L.EVIDENCE_CONTACT, L.EVIDENCE_WORDS) == (E.SIDE, E.FOOD, E.CONTACT, E.WORDS)


def test_cli_has_the_flag():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("pmx_tools_train_evidence", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                           "tools", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parser().parse_args(["--fog-of-war", "--belief", "--belief-evidence"]).belief_evidence is True
    assert mod.parser().parse_args([]).belief_evidence is False
