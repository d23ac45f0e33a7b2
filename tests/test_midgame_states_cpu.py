"""The runs tests/test_gpu_fused_tick_events.py compares the fused tick on are eventful: asserted here from the CPU oracle alone,
so it runs anywhere and a change of seeds, boards or recipe that makes the GPU comparison vacuous fails without a GPU.

Per (board, state source), 192 envs, 20 ticks of _midgame.mixed_actions, length 300: how often food was eaten, a capsule was
eaten, a death put food back on the board, the score changed, a game ended before its timeout, how much an agent carried, and
how often finishing envs were scattered inside a group of 64.  The thresholds are conditions of the test design (what a run
must contain for the comparison to mean something), far below what the runs contain; see count_events for how each figure is
counted (each is a lower bound).

Also: _midgame.random_states is the recipe that made the scen_*_random fixtures, so with the recipe's own step draw it must
reproduce their input states."""
import numpy as np
import pytest

import _golden as G
import _midgame as M
from oracle import oracle as O

N = 192
BOARDS = ["smallCapture", "tinyCapture", "bloxCapture", "maze23",
          "maze20x12", "maze20x13", "maze20x14", "maze20x16", "maze20x17", "maze20x20", "maze32x16", "maze32x20"]


@pytest.mark.parametrize("board", BOARDS)
def test_runs_are_eventful(board):
    run = M.oracle_run(board, N, keep_obs=False)
    ev = run.events()
    print(f"{board}: " + ", ".join(f"{k} {ev[k]}" for k in ("food", "capsule", "dump", "score", "early", "max_carry", "mixed")))
    assert ev["food"] >= 100, ev
    if board not in M.NO_CAPSULES:
        assert ev["capsule"] >= 3, ev
    assert ev["dump"] >= 20, ev
    assert ev["score"] >= 40, ev
    assert ev["early"] >= 5, ev
    assert ev["max_carry"] >= 15, ev
    assert ev["mixed"] >= 1, ev
    seeded = [e for e in range(N) if e % 5 != 4]
    assert max(int(run.states[0]["steps"][e]) for e in seeded) <= M.MAX_STEPS        # no timeout inside the run
    start = O.Env(list(run.rows)).get_state()
    for e in range(4, N, 5):                                                            # every fifth env: the start position
        assert bytes(run.start[e]) == bytes(start)


@pytest.mark.parametrize("board", ["smallCapture", "maze32x20"])
def test_hand_off_ticks_are_eventful(board):
    """the ticks at which test_gpu_fused_tick_events.py compares pmx_emit_team_obs and pmx_observe (0, 7 and 19): a game ends in
    one of them and a capsule is eaten in one of them"""
    ev = M.oracle_run(board, N, keep_obs=False).events()
    assert any(ev["finish_ticks"][t] for t in (0, 7, 19)) and any(ev["capsule_ticks"][t] for t in (0, 7, 19)), ev


@pytest.mark.parametrize("board,seed", [("smallCapture", 101), ("tinyCapture", 102), ("maze23", 104)])
def test_random_states_is_the_recipe_of_the_fixtures(board, seed):
    """the fixtures were made with random_states(lay, n, seed, with_caps=True); scenario k is named rand<k> (the reference
    could not run a few, which are missing)"""
    d, meta = G.load(M.FIXTURES[board])
    rows = meta["layout"]
    H = len(rows)
    ks = [int(name[4:]) for name in meta["names"]]
    states = M.random_states(rows, max(ks) + 1, seed, recipe_steps=True)
    for row, k in enumerate(ks):
        want = M.fixture_row_state(d, row, H, max_steps=10 ** 9)
        assert bytes(states[k]) == bytes(want), f"{board} rand{k}"


def test_mixed_actions_mix():
    rng = np.random.RandomState(0)
    legal = np.full((4096, 4), 0b10011, np.uint8)                  # north, east and stop are legal
    a = M.mixed_actions(rng, legal, 4096)
    share = lambda m: float(m.mean())
    assert 0.10 < share(a == M.ACTION_RANDOM_LEGAL) < 0.14
    junk = np.isin(a, M.JUNK_CODES)
    assert 0.005 < share(junk) < 0.015 and len(set(a[junk].tolist())) == 1
    plain = a[(a >= 0) & (a <= 4)]
    illegal = share(((0b10011 >> plain) & 1) == 0)
    assert 0.3 * 0.4 * 0.8 < illegal < 0.3 * 0.4 * 1.2 + 0.7 * 0.4 ** 4    # the 30 % uniform part, 2 of 5 codes illegal
