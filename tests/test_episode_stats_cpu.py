"""CPU suite: the rules of the episode statistics (include/pmx.h, "Episode statistics") as the plain-Python model of
_episode_stats_ref.py states them, on the recorded sub-step states of the ten trajectory fixtures and on hand-set states stepped by
the CPU oracle.  The GPU suite (test_gpu_episode_stats.py) holds the kernel to this model word for word."""
import numpy as np
import pytest

import _episode_stats_ref as R
import _golden as G
from oracle import oracle as O

TRAJ = G.names("traj_*.npz")
HUNTERS = [n for n in TRAJ if "hunter" in n]
_cache = {}


def _episodes(name, **knobs):
    key = (name, tuple(sorted(knobs.items())))
    if key not in _cache:
        d, _ = G.load(name)
        _cache[key] = (d, R.fixture_episodes(d, **knobs))
    return _cache[key]


def test_fixture_list():
    assert len(TRAJ) == 10 and len(HUNTERS) == 6


@pytest.mark.parametrize("name", TRAJ)
def test_invariants_on_every_finished_episode(name):
    d, eps = _episodes(name)
    for rec, t in eps:
        assert rec.done == 1 and rec.score == int(d["sub_score"][t, 3])
        assert R.invariants(rec, d["sub_ret"][t, 3], d["sub_score"][t, 3]) == [], (name, t)


def test_the_fixtures_finish_episodes():
    assert sum(len(_episodes(n)[1]) for n in TRAJ) == 21


def _whole_file(name):
    """the counters of a whole file, unfinished tail included: one Record per episode, summed"""
    d, _ = G.load(name)
    tot = {n: 0 for n in R.NAMES}
    mover = nonmover = 0
    rec = R.Record(R.fixture_state(d))
    for t in range(len(d["done"])):
        rec.tick([R.fixture_state(d, t, s) for s in range(4)], d["done"][t])
        if d["done"][t] or t == len(d["done"]) - 1:
            for n in R.NAMES:
                tot[n] += sum(rec.c[n])
            mover, nonmover = mover + rec.mover_deaths, nonmover + rec.nonmover_deaths
            rec = R.Record(R.fixture_state(d))
    return tot, mover, nonmover


def test_the_rules_find_material():
    tot, mover, nonmover = _whole_file("traj_small_hunter.npz")
    print("traj_small_hunter", tot, "mover deaths", mover, "non-mover deaths", nonmover)
    assert mover >= 50 and nonmover >= 50
    assert (tot["eaten"], tot["returned"], tot["lost"], nonmover, mover) == (189, 74, 109, 60, 72)     # reproduced here, now pinned
    assert tot["deaths"] == mover + nonmover == tot["kills"] + mover
    for name in ("traj_maze23_hunter.npz", "traj_maze4242_hunter.npz"):
        tot, _, _ = _whole_file(name)
        print(name, tot)
        assert tot["capsules"] >= 4


@pytest.mark.parametrize("name", HUNTERS)
def test_mover_death_rule_against_the_recorded_actions(name):
    """the mover died == its new cell is neither its old cell nor old cell + the recorded action's vector, on every sub-step"""
    d, _ = G.load(name)
    X = R.fixture_state(d)
    bad = []
    for t in range(len(d["done"])):
        for m in range(4):
            Y = R.fixture_state(d, t, m)
            v = R.ACTION_VECTORS[int(d["actions"][t, m])]
            moved_to = (X.pos[m][0] + v[0], X.pos[m][1] + v[1])
            by_action = Y.pos[m] not in (X.pos[m], moved_to)
            if R.mover_died(X, Y, m) != by_action:
                bad.append((t, m, X.pos[m], Y.pos[m], int(d["actions"][t, m]), X.scared[m], Y.scared[m], X.carry[m], Y.carry[m]))
            X = Y
        if d["done"][t]:
            X = R.fixture_state(d)
    assert bad == [], (name, len(bad), bad[:5])


def _pacman_deaths(name, **knobs):
    """deaths of agents that were Pacman before the transition, over a whole file (one Record per episode, the unfinished tail too)"""
    d, meta = G.load(name)
    n, rec = 0, R.Record(R.fixture_state(d), **knobs)
    for t in range(len(d["done"])):
        rec.tick([R.fixture_state(d, t, s) for s in range(4)], d["done"][t])
        if d["done"][t] or t == len(d["done"]) - 1:
            n, rec = n + rec.pacman_deaths, R.Record(R.fixture_state(d), **knobs)
    return n, meta["events"]["deaths"]


@pytest.mark.parametrize("name", TRAJ)
def test_pacman_deaths_equal_the_fixtures_own_count(name):
    """A fourth invariant, per file: the generator counted, while the reference ran, every Pacman that was sent to its start
    (meta.events.deaths: it was Pacman, is not, stands on its start, more than one step away).  The model must find exactly those."""
    n, recorded = _pacman_deaths(name)
    assert n == recorded


def test_negative_control_lost_from_the_new_state():
    """a model crediting LOST with carry_Y breaks eaten - returned - lost == carry"""
    found = []
    for name in TRAJ:
        d, eps = _episodes(name, lost_from="Y")
        for rec, t in eps:
            found += R.invariants(rec, d["sub_ret"][t, 3], d["sub_score"][t, 3])
    assert "eaten - returned - lost == carry" in found


def test_negative_control_without_the_non_mover_position_rule():
    """A model without the non-mover position rule breaks an invariant -- the death count above, and NONE of the three per-episode
    ones: measured, they hold on all 21 episodes without the rule, and they must, because a death that changes LOST empties a
    carry > 0 and the carry disjunct sees that by itself.  What the position rule alone finds are the deaths of Pacmen that carry
    nothing (32 of the 124 recorded ones on traj_small_hunter); those move DEATHS and KILLS only, which no balance contains."""
    for name in TRAJ:
        d, eps = _episodes(name, position_rule=False)
        for rec, t in eps:
            assert R.invariants(rec, d["sub_ret"][t, 3], d["sub_score"][t, 3]) == []
    n, recorded = _pacman_deaths("traj_small_hunter.npz", position_rule=False)
    assert (n, recorded) == (92, 124)
    assert sum(_pacman_deaths(name, position_rule=False)[0] != _pacman_deaths(name)[1] for name in HUNTERS) == len(HUNTERS)


def _oracle_tick(scn):
    env = O.Env(list(R.SCENARIO_ROWS), length=300)
    food, caps = R.scenario_layout()
    env.set_state_arrays(scn["pos"], scn["dir"], scn["pac"], scn["scared"], scn["carry"], scn["ret"], food, caps, 0, 0)
    rec = R.Record(R.state_of(env.get_state()))
    out = env.tick(scn["actions"])
    assert all(out["subout"][i].fault == 0 for i in range(4))
    rec.tick([R.state_of(out["sub"][s]) for s in range(4)], out["done"])
    return rec, out


@pytest.mark.parametrize("scn", R.SCENARIOS, ids=[s["name"] for s in R.SCENARIOS])
def test_hand_set_states_through_the_oracle(scn):
    rec, out = _oracle_tick(scn)
    R.check_expect(rec, scn["expect"])
    s = rec.last
    assert all(rec.c["eaten"][i] - rec.c["returned"][i] - rec.c["lost"][i] == s.carry[i] - scn["carry"][i] for i in range(4))
    assert rec.ticks == 1


def test_hand_set_states_are_what_they_claim():
    """the oracle's own record of each scenario: who was sent home, and that the disjunct under test fired ALONE"""
    by = {s["name"]: _oracle_tick(s) for s in R.SCENARIOS}
    sub = lambda name, s: R.state_of(by[name][1]["sub"][s])
    # eaten on its own start: same cell, the timer cleared (it ticked 10 -> 9 on agent 0's own Stop)
    X, Y = sub("scared_ghost_on_start_eaten", 0), sub("scared_ghost_on_start_eaten", 1)
    assert X.pos[0] == Y.pos[0] == (1, 1) and X.scared[0] == 9 and Y.scared[0] == 0 and X.carry[0] == Y.carry[0] == 0
    # eat and die: back on its start with nothing, three pellets on the board again
    Y = sub("eat_and_die", 1)
    assert Y.pos[1] == (10, 5) and Y.carry[1] == 0 and Y.pac[1] == 0
    # the capsule is gone and the red team is scared
    Y = sub("capsule", 1)
    assert len(Y.caps) == 1 and Y.scared[0] == 40 and Y.scared[2] == 40
    # the blind spot and its neighbour: both are eaten on the start cell they stepped onto
    for name, fear in (("scared_mover_dies_on_start", 2), ("blind_spot", 1)):
        Y = sub(name, 0)
        assert Y.pos[0] == (1, 1) and Y.scared[0] == 0 and Y.pos[1] == (1, 1), name
    assert by["blind_spot"][0].c["deaths"][0] == 0 and by["scared_mover_dies_on_start"][0].c["deaths"][0] == 1


def test_words_layout():
    rec, _ = _oracle_tick(R.SCENARIOS[3])         # the capsule scenario
    w = rec.words()
    assert w.shape == (48,) and w.dtype == np.int32
    assert w[8 * 1 + R.NAMES.index("capsules")] == 1 and w[32] == 1 and w[34] == 0 and w[35] == 0 and w[46] == 0 and w[47] == 0
    assert w[36 + 1] & 0xFFFF == 3 | 3 << 8 and (w[36 + 1] >> 24) & 1 == 1
    assert w[40] & 0xFF == 40 and w[42] & 0xFF == 39      # agent 0 moved before the capsule was eaten, agent 2 after it
    assert np.uint32(w[44]) == np.uint32(0xFFFF | (8 | 3 << 8) << 16) and np.uint32(w[45]) == 0xFFFFFFFF
