"""pmx_tick_fused_kernel stores agent 0's planes while its rule wave still runs sub-steps 1-3, from the snapshot sub-step 0 left
in LDS, and expands them AGAIN in its last phase for the envs that turned out to finish in the tick (with auto_reset such an env
shows the fresh game to all four agents).  The other three agents' blocks are dealt to all 16 waves.

What these tests add to test_gpu_fused_tick.py:

* finishing and non-finishing envs side by side in every workgroup, which lockstep games never produce: the envs are de-phased
  with reset(mask) so that at every tick some lanes of every group of 64 finish and others do not.  A fused handle and a
  two-launch handle run the same actions and must agree on every result, and a finishing env's planes must equal the planes
  the first reset() returned for it (one layout, deterministic starts), a check that does not depend on the two-launch path;
* the state the launch leaves behind after such a run, byte for byte, twenty further ticks on;
* the CPU oracle on a board of each kind for 64 and 192 envs with both sweeps -- the wall plane ending on a vector boundary
  (8 x 5), a vector that straddles planes 0 and 1 (smallCapture), the HB 16 bucket (a 20 x 14 maze) and the HB 20 bucket with
  the largest LDS request (a 20 x 20 maze).

The caller's buffer is poisoned before every compared step; equality is exact."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

T = 20
POISON = 7
_TINY_BOARD = ["%%%%%%%%", "%1 .. 2%", "%  ..  %", "%3 .. 4%", "%%%%%%%%"]


def _pmx():
    import pmx
    return pmx


@functools.lru_cache(maxsize=None)
def _rows(board):
    pmx = _pmx()
    from pmx import maze_generator as MG
    if board == "board8x5":
        return tuple(_TINY_BOARD)
    if board.startswith("maze"):                                   # "mazeWxH": the generator mirrors `cols` columns and adds the border
        w, h = (int(v) for v in board[4:].split("x"))
        rows = tuple(MG.generate_maze(11, rows=h - 2, cols=(w - 2) // 2).split("\n"))
        assert (len(rows[0]), len(rows)) == (w, h)
        return rows
    return tuple(pmx.get_layout(board).text)


def _actions(N, seed, ticks=T):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 5, size=(N, 4)).astype(np.int8) for _ in range(ticks)]


def _record(orc, acts, N, H, W):
    """everything the oracle returns at every tick (the planes as bytes: no element exceeds 1 + the board's pellets)"""
    oobs = np.zeros((N, 4, 8, H, W), np.float32)
    out = []
    for a in acts:
        orc.tick(a, oobs)
        assert oobs.max() <= 255 and (oobs == np.floor(oobs)).all()
        out.append(dict(obs=oobs.astype(np.uint8), reward=orc.reward.tobytes(), done=orc.done.copy(), legal=orc.legal.copy(),
                        score_change=orc.score_change.copy(), score=orc.score.copy(), agent=orc.agent.copy()))
    return out


@functools.lru_cache(maxsize=None)
def _reference(board, N, length=60):
    """(actions, the oracle's results per tick) of one layout; computed once and shared by the cases of that board"""
    rows = list(_rows(board))
    acts = _actions(N, 2000 + N)
    return acts, _record(O.BatchEnv(rows, N, length=length, auto_reset=True, seed=3), acts, N, len(rows), len(rows[0]))


def _check_tick(env, a, want, tag=""):
    """poison, step, compare every element of every result with the oracle's"""
    env.obs.fill_(POISON)
    obs, rew, done, info = env.step(torch.tensor(a).cuda())
    assert env.last_step_fused(), tag
    got = obs.float().cpu().numpy()
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


# ---- boards and buckets against the CPU oracle ----------------------------------------------------------------------------------

_BUCKET = {"board8x5": 12, "smallCapture": 12, "maze20x14": 16, "maze20x20": 20}


@pytest.mark.parametrize("alt", [0, -1])
@pytest.mark.parametrize("N", [64, 192])
@pytest.mark.parametrize("board", sorted(_BUCKET))
def test_boards_and_buckets_match_the_oracle(board, N, alt):
    pmx = _pmx()
    rows = list(_rows(board))
    H, W = len(rows), len(rows[0])
    assert min(b for b in (12, 16, 20) if H <= b) == _BUCKET[board]
    if board == "board8x5":
        assert (H * W) % 4 == 0            # the wall plane ends on a 16-byte vector boundary
    if board == "smallCapture":
        assert (H * W) % 4 != 0            # a vector straddles planes 0 and 1
    acts, ref = _reference(board, N)
    env = pmx.PmxVecEnv(pmx.Layout.from_text(rows), N, length=60, auto_reset=True, seed=3)
    env.set_tuning("expand_alt", alt)
    env.set_tuning("fused_min_envs", 64)
    env.reset()
    for t, a in enumerate(acts):
        _check_tick(env, a, ref[t], f"t={t}")
    env.close()


# ---- finishing and non-finishing envs in one workgroup; the state behind them -----------------------------------------------------

def _same_results(A, B, tag):
    for name in ("obs", "reward", "done", "legal", "score_change", "score", "agent"):
        assert torch.equal(getattr(A, name), getattr(B, name)), f"{tag} {name}"


@pytest.mark.parametrize("alt", [0, -1])
def test_mixed_finishing_inside_a_workgroup(alt):
    """length=5: an env finishes every sixth tick.  reset(mask) at ticks 1..4 with the masks env % 5 == k puts the five residue
    classes out of phase, so from then on a tick finishes one class (or none) in every group of 64 envs.  Then twenty further
    ticks without poisoning, and the two handles' states byte for byte."""
    pmx = _pmx()
    N = 192
    acts = _actions(N, 515, 2 * T)
    F = pmx.PmxVecEnv("smallCapture", N, length=5, auto_reset=True, seed=3)
    P = pmx.PmxVecEnv("smallCapture", N, length=5, auto_reset=True, seed=3)
    for E in (F, P):
        E.set_tuning("expand_alt", alt)
    F.set_tuning("fused_min_envs", 64)
    P.set_tuning("fused_min_envs", N + 1)
    F.reset()
    P.reset()
    assert torch.equal(F.obs, P.obs)
    first = F.obs.clone()                  # the fresh game as all four agents see it
    residue = torch.arange(N, device="cuda") % 5
    mixed = 0
    for t in range(T):
        if 1 <= t <= 4:
            F.reset(residue == t)
            P.reset(residue == t)
        a = torch.tensor(acts[t]).cuda()
        F.obs.fill_(POISON)
        P.obs.fill_(POISON)
        F.step(a)
        P.step(a)
        assert F.last_step_fused() and not P.last_step_fused()
        _same_results(F, P, f"t={t}")
        done = F.done.bool()
        assert torch.equal(F.obs[done], first[done]), f"t={t}: a finished env does not show the fresh game"
        per_group = done.view(N // 64, 64).sum(1)
        mixed += int(((per_group > 0) & (per_group < 64)).all())
    assert mixed >= 10, mixed
    assert bytes(F.get_state()) == bytes(P.get_state())
    for t in range(T, 2 * T):
        a = torch.tensor(acts[t]).cuda()
        F.step(a)
        P.step(a)
        assert F.last_step_fused() and not P.last_step_fused()
        _same_results(F, P, f"t={t}")
    assert bytes(F.get_state()) == bytes(P.get_state())
    F.close()
    P.close()
