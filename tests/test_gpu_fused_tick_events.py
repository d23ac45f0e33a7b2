"""pmx_tick_fused_kernel against the CPU oracle on MID-GAME states, on every bucket and width it is instantiated or launched for.

tests/test_gpu_fused_tick.py and tests/test_gpu_fused_early_planes.py start from the start position and play twenty ticks of
uniformly random actions: on every real board nobody leaves home in them, so no food bit changes, the self plane is always 1,
the capsule planes are constant, no timer runs and no game ends but by its timeout.  Here the envs start in the middle of a
game (tests/_midgame.py: the reference-made states of the scen_*_random fixtures, or states drawn by the same recipe on generated
mazes) and play test_differential_vs_oracle's action mix, with junk codes and the in-kernel random-legal draw, which is keyed by
the env index while the alternating sweep maps the workgroups backwards.  tests/test_midgame_states_cpu.py asserts from the
oracle alone that these very runs eat food and capsules, kill carriers (the food rows then differ between the snapshot agent
0's planes are expanded from and the later ones), score, carry 15 and more, and end games by the food threshold, with
finishing envs scattered inside a workgroup.

Boards: smallCapture (HB 12, a vector straddles planes 0 and 1), tinyCapture (HB 12, 35 vectors exactly), bloxCapture and the
maze23 board (HB 20), 20 x 13 and 20 x 16 mazes (both ends of HB 16), 32 x 16 and 32 x 20 mazes (bit 31 in the wall rows and
the blue side's mask, food up to bit 30, the widest stream table, the largest LDS request the launcher accepts).  Everything a step returns is compared
exactly at every tick, with the caller's buffer poisoned before the step, and the full state of every env after ticks 4, 9, 14
and 19: the kernel writes the state from LDS in its last phase, and a wrong row there surfaces in the planes ticks later, if at
all."""
import ctypes as C

import numpy as np
import pytest
import torch

import _midgame as M

pytestmark = pytest.mark.gpu

POISON = 7
STATE_TICKS = (4, 9, 14, 19)
HANDOFF_TICKS = (0, 7, 19)
_BUCKET = {"smallCapture": 12, "tinyCapture": 12, "bloxCapture": 20, "maze23": 20, "maze20x13": 16, "maze20x16": 16,
           "maze32x16": 16, "maze32x20": 20}


def _pmx():
    import pmx
    return pmx


def _state_dtype(pmx):
    """the handle's exchange format (pmx.State) as a numpy record"""
    dt = np.dtype([("pos", "i1", (4, 2)), ("dir", "i1", 4), ("pac", "u1", 4), ("scared", "u1", 4), ("carry", "<u2", 4),
                   ("ret", "<u2", 4), ("food", "<u4", 32), ("caps", "<u4", 32), ("score", "<i4"), ("steps", "<i4"), ("ticks", "<u4")])
    assert dt.itemsize == C.sizeof(pmx._lib.State)
    return dt


def _make_env(run, N, alt=-1, fused_min=64, **kw):
    pmx = _pmx()
    env = pmx.PmxVecEnv(pmx.Layout.from_text(list(run.rows)), N, length=run.length, auto_reset=True, seed=3, **kw)
    env.set_tuning("expand_alt", alt)
    env.set_tuning("fused_min_envs", fused_min)
    env.reset()
    M.load_states(pmx, env, run.start)
    return env


def _check_tick(env, a, want, tag):
    """poison, step, compare every element of every result with the oracle's"""
    env.obs.fill_(POISON)
    obs, rew, done, info = env.step(torch.tensor(a).cuda())
    assert env.last_step_fused(), tag
    got = obs.cpu().numpy()
    ref = want["obs"].astype(np.float32)
    assert got.shape == ref.shape
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, f"{tag}: {len(bad)} elements differ, first (env, slot, plane, y, x) = {bad[0]}, got {got[tuple(bad[0])]}"
    assert rew.cpu().numpy().tobytes() == want["reward"], f"{tag} reward"
    assert (done.cpu().numpy() == want["done"]).all(), f"{tag} done"
    assert (info["legal_actions"].cpu().numpy() == want["legal"]).all(), f"{tag} legal"
    assert (info["score_change"].cpu().numpy() == want["score_change"]).all(), f"{tag} score_change"
    assert (info["score"].cpu().numpy() == want["score"]).all(), f"{tag} score"
    assert (info["agent"].cpu().numpy().astype(np.uint32) == want["agent"]).all(), f"{tag} agent words"


def _check_state(env, want, H, tag):
    """the full state of every env against the oracle's packed states"""
    got = np.frombuffer(env.get_state(), dtype=_state_dtype(_pmx()))
    for f in M.STATE_FIELDS:
        g, w = got[f], want[f]
        if f in ("food", "caps"):
            g, w = g[:, :H], w[:, :H]
        bad = np.nonzero((g != w).reshape(len(got), -1).any(1))[0]
        assert len(bad) == 0, f"{tag}: state field {f} differs for envs {bad[:10]}: {g[bad[0]]} vs {w[bad[0]]}"


def _run_against_the_oracle(run, N, alt, **kw):
    env = _make_env(run, N, alt, **kw)
    for t, a in enumerate(run.actions):
        _check_tick(env, a, run.ticks[t], f"t={t}")
        if t in STATE_TICKS:
            _check_state(env, run.states[t + 1], run.H, f"t={t}")
    env.close()


# one board's cases are neighbours, so that the two sweeps share the board's cached oracle record
_CASES = [(board, 192, alt) for board in _BUCKET for alt in (0, -1)] + [("smallCapture", 64, alt) for alt in (0, -1)]


@pytest.mark.parametrize("board,N,alt", _CASES)
def test_fused_tick_matches_the_oracle_on_mid_game_states(board, N, alt):
    run = M.oracle_run(board, N)
    H, W = run.H, run.W
    assert min(b for b in (12, 16, 20) if H <= b) == _BUCKET[board]
    if board == "smallCapture":
        assert (H * W) % 4 != 0                      # a vector straddles planes 0 and 1
    if board == "tinyCapture":
        assert H * W == 4 * 35                       # the wall plane is 35 vectors exactly
    if board in ("maze20x13", "maze20x16"):
        assert H in (13, 16)                         # both ends of the HB 16 bucket
    if board.startswith("maze32"):
        # column 31 is the border wall (bit 31 of the wall rows and of the blue side's mask); food reaches bit 30
        assert W == 32 and ((run.states[0]["food"] >> 30) & 1).any() and not (run.states[0]["food"] >> 31).any()
    _run_against_the_oracle(run, N, alt)


@pytest.mark.parametrize("alt", [0, -1])
def test_reward_switches_off(alt):
    """reward_forLegalAction=False, defenceReward=False: the other side of both switches of the reward code the fused kernel
    runs in tick_substep / tick_finish"""
    N = 192
    run = M.oracle_run("smallCapture", N, False, False)
    assert run.ticks[0]["reward"] != M.oracle_run("smallCapture", N).ticks[0]["reward"]
    _run_against_the_oracle(run, N, alt, reward_forLegalAction=False, defenceReward=False)


# ---- hand-off of the state and the three snapshots to the kernels that read them ----------------------------------------------

def _same_results(A, B, tag):
    for name in ("obs", "reward", "done", "legal", "score_change", "score", "agent"):
        assert torch.equal(getattr(A, name), getattr(B, name)), f"{tag} {name}"


@pytest.mark.parametrize("board", ["smallCapture", "maze32x20"])
def test_eventful_state_and_snapshots_reach_the_other_kernels(board):
    """a fused handle and a two-launch handle from the same loaded states, on ticks in which games end and capsules are eaten:
    pmx_emit_team_obs (the three snapshots and the state), pmx_observe (the state), the next tick, and at the end the state byte
    for byte and pmx_step_agent for all four agents"""
    N = 192
    run = M.oracle_run(board, N)
    ev = run.events()
    assert any(ev["finish_ticks"][t] for t in HANDOFF_TICKS) and any(ev["capsule_ticks"][t] for t in HANDOFF_TICKS)
    F = _make_env(run, N, fused_min=64)
    P = _make_env(run, N, fused_min=N + 1)
    shape = (N, 2) + F.obs_shape

    def poisoned(s):
        return torch.full(s, POISON, dtype=torch.float32, device="cuda")

    for t, acts in enumerate(run.actions):
        a = torch.tensor(acts).cuda()
        F.obs.fill_(POISON)
        P.obs.fill_(POISON)
        F.step(a)
        P.step(a)
        assert F.last_step_fused() and not P.last_step_fused()
        _same_results(F, P, f"t={t}")
        if t in HANDOFF_TICKS:
            for red in (1, 0):
                tf, mf = F.emit_team_obs(red, poisoned(shape), poisoned(shape[:1] + shape[2:]))
                tp, mp = P.emit_team_obs(red, poisoned(shape), poisoned(shape[:1] + shape[2:]))
                assert torch.equal(tf, tp) and torch.equal(mf, mp), (t, red)
            stepped = F.obs.clone()
            of, lf = F.observe()
            op, lp = P.observe()
            assert torch.equal(of, op) and torch.equal(lf, lp), t
            assert torch.equal(of[:, 3], stepped[:, 3]), t       # agent 3's planes of a step are those of the state it leaves
    assert bytes(F.get_state()) == bytes(P.get_state())
    rng = np.random.RandomState(9)
    for i in range(4):
        a = torch.tensor(rng.randint(0, 5, size=N).astype(np.int8)).cuda()
        assert torch.equal(F.step_agent(i, a), P.step_agent(i, a)), i
    _same_results(F, P, "after step_agent")
    assert bytes(F.get_state()) == bytes(P.get_state())
    F.close()
    P.close()
