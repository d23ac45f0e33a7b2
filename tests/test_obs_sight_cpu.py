"""CPU suite of the sight rule on the four-agent surfaces (include/pmx.h "Sight rule on the four-agent planes"): the numpy model of
pmx_agent_distances (tests/_agent_distances_ref.py) against the reference's four readings per observation (fixture G11) and against
tests/_belief_ref.py's readings on the golden hunter trajectories, and the new symbols of the header, the binding and the drop-in
class.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import _agent_distances_ref as A
import _belief_ref as R
import _golden as G
import pmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE = list(range(-6, 7))


def _g11():
    """G11 with the four agents' cells of every row rebuilt from the source fixtures, as tests/test_belief_cpu.py rebuilds them:
    (positions [m, 4, 2], observer [m], the reference's four readings [m, 4])"""
    d, meta = G.load("fog_sight.npz")
    P = np.zeros((len(d["src"]), 4, 2), np.int64)
    for s, name in enumerate(meta["sources"]):
        src, _ = G.load(name)
        rows = np.nonzero(d["src"] == s)[0]
        idx, sub = d["idx"][rows], d["sub"][rows]
        P[rows] = (src["in_pos"][idx] if name.startswith("scen") else src["sub_pos"][idx, sub]).astype(np.int64)
    return P, d["observer"].astype(np.int64), d["sonar"].astype(np.int64)


def test_the_reference_reads_all_four_agents_with_the_models_noise_range():
    P, observer, sonar = _g11()
    assert sonar.shape == (2794, 4)
    ar = np.arange(len(P))
    n = sonar - R.manhattan(P, P[ar, observer][:, None])               # reading minus the Manhattan distance from the observer
    assert n.min() >= -6 and n.max() <= 6                               # all four targets, every row
    for i in range(4):                                                  # ... self, mate and both enemies each span the range
        assert sorted(set(n[:, i].tolist())) == NOISE, i
    values, counts = np.unique(n[ar, observer], return_counts=True)     # the self column is the bare noise
    assert values.tolist() == NOISE
    assert counts.min() >= 190 and counts.max() <= 237, counts
    # the model on those rows (any key): the same distances, a noise inside the same 13 values
    for a in range(4):
        m = observer == a
        mine = A.readings_agent(P[m], a, 77, np.nonzero(m)[0], np.full(int(m.sum()), 9))
        assert np.abs(mine - R.manhattan(P[m], P[m, a][:, None])).max() == 6
        assert np.abs(mine - sonar[m]).max() <= 12


@pytest.mark.parametrize("seed,a,i", ((0, 0, 0), (12345, 0, 2), (7, 2, 2), (3, 3, 1), (99, 1, 3)))
def test_the_models_noise_is_uniform_over_consecutive_keys(seed, a, i):
    """2^16 consecutive (env, ticks) keys for a self, a mate and enemy targets.  A uniform draw puts 65536 / 13 = 5041 keys on each
    value with a standard deviation of sqrt(65536 * 12 / 169) = 68; the band is a tenth of the share (7 deviations), the band
    tests/test_belief_cpu.py holds the enemy draws to."""
    env, ticks = np.meshgrid(np.arange(256), np.arange(1000, 1256), indexing="ij")
    P = np.zeros((env.size, 4, 2), np.int64)                            # every agent on one cell: the reading is the noise
    n = A.readings_agent(P, a, seed, env.ravel(), ticks.ravel())[:, i]
    values, counts = np.unique(n, return_counts=True)
    assert values.tolist() == NOISE
    assert (np.abs(counts / n.size - 1 / 13) <= 0.1 / 13).all(), counts
    full = A.readings(np.zeros((env.size, 4, 4, 2), np.int64), seed, env.ravel(), ticks.ravel())
    assert (full[:, a, i] == n).all()                                   # the two forms share the key


@pytest.mark.parametrize("name", ("traj_small_hunter.npz", "traj_blox_hunter.npz"))
def test_enemy_readings_are_the_belief_trackers(name):
    """r[a_j][e_k] of the model == the reading tests/_belief_ref.py's update takes for slot j and enemy k, both colours, every tick
    of a golden hunter trajectory that is not a reset (a reset row's readings are 0 in the tracker)."""
    d, meta = G.load(name)
    lay = pmx.get_layout({"small": "smallCapture", "tiny": "tinyCapture", "blox": "bloxCapture"}[meta["layout_name"]])
    red = np.array([True, False])
    first = np.where(red, 0, 1)
    ar = np.arange(2)
    open_g = np.repeat(R.open_cells(lay.wall_rows, lay.width, lay.height)[None], 2, 0)
    starts = np.repeat(lay.starts.astype(np.int64)[None], 2, 0)
    bel = R.init(0, open_g, starts)
    compared = 0
    for t in range(len(d["actions"])):
        done = bool(d["resets"][t])
        sub = d["init_pos"][None].repeat(4, 0) if done else d["sub_pos"][t]                # [4 sources, 4 agents, 2]
        P2 = np.stack([sub[first], sub[first + 2]], 1)                                     # the tracker's two slots
        ticks = np.full(2, t + 1)
        bel, sonar, _ = R.update(bel, P2, red, 5, ticks, 77, ar, open_g, starts, reset=np.full(2, done))
        mine = A.readings(np.repeat(sub[None], 2, 0), 77, ar, ticks)
        if done:
            assert (sonar == 0).all()
            continue
        for j in range(2):
            for k in range(2):
                a_j, e_k = first + 2 * j, (1 - first) + 2 * k
                assert (mine[ar, a_j, e_k] == sonar[:, j, k]).all(), (t, j, k)
                compared += 2
        # and each row of the table is the single-agent form on that source's positions
        for a in range(4):
            assert (A.readings_agent(np.repeat(sub[a][None], 2, 0), a, 77, ar, ticks) == mine[:, a]).all()
    assert compared > 400


def _header():
    return open(os.path.join(ROOT, "include", "pmx.h")).read()


def test_header_declares_the_entry_points_and_the_constant():
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+pmx_set_obs_sight\s*\(\s*pmx_env\s*\*\s*env\s*,\s*int32_t\s+sight_range\s*\)\s*;", code)
    assert re.search(r"\bint\s+pmx_agent_distances\s*\(\s*pmx_env\s*\*\s*env\s*,\s*int\s+agent\s*,\s*int8_t\s*\*\s*dist_dev\s*,\s*void\s*\*\s*stream\s*\)\s*;", code)
    assert re.search(r"^#define\s+PMX_OBS_SIGHT_OFF\s+\(-1\)\s*$", code, flags=re.M)
    assert "capture.py:268-292" in src and "capture.py:210-224" in src           # the rule table cites the reference
    assert pmx._lib.OBS_SIGHT_OFF == -1


def test_binding_has_the_prototypes_and_null_handles_are_refused():
    import ctypes as C
    protos = {n: (r, a) for n, r, a in pmx._lib.PROTOTYPES}
    assert protos["pmx_set_obs_sight"] == (C.c_int, [C.c_void_p, C.c_int32])
    assert protos["pmx_agent_distances"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p])
    lib = pmx._lib.load()
    assert lib.pmx_set_obs_sight(None, 5) == -1
    assert b"pmx_set_obs_sight: null" in lib.pmx_last_error()
    assert lib.pmx_agent_distances(None, -1, None, None) == -1
    assert b"pmx_agent_distances: null" in lib.pmx_last_error()


def test_drop_in_class_and_vec_env_have_the_keywords():
    sig = inspect.signature(pmx.gymPacMan_parallel_env.__init__).parameters
    assert sig["fog_of_war"].default is False and sig["sight_range"].default == 5
    assert sig["fog_bots"].default is False                                       # the two flags are independent keywords
    assert inspect.signature(pmx.PmxVecEnv.set_obs_sight).parameters["sight_range"].default is None
    par = inspect.signature(pmx.PmxVecEnv.agent_distances).parameters
    assert par["agent"].default is None and par["out"].default is None
