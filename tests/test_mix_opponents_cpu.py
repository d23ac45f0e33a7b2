"""CPU suite of mixed-opponent rollouts: the plan that spreads the curriculum's mixture over the envs of one rollout
(trainer.mix_plan), the per-env forms of the frame helpers against the scalar ones, and the checkpoint flag.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from pmx import mappo, trainer

SCALE = 0.1
PHASES = {1: 10, 2: 50, 3: 200}            # update indices inside the three phases at curriculum_scale 0.1 (thresholds 20 and 80)
N_ENVS = (1, 2, 7, 64, 4096)
HARD = (("baseline",), ("baseline", "approxq"))


def _shares(phase, hard):
    bots = {b: Fraction(5, 6) / len(hard) for b in hard}
    if phase == 1:
        return {"random": Fraction(1)}
    if phase == 2:
        return {**bots, "random": Fraction(1, 6)}
    return {"self": Fraction(2, 5), "pool": Fraction(1, 5), **{b: Fraction(2, 5) * f for b, f in bots.items()}, "random": Fraction(2, 5) * Fraction(1, 6)}


@pytest.mark.parametrize("hard", HARD, ids=("one_bot", "two_bots"))
@pytest.mark.parametrize("phase", (1, 2, 3))
@pytest.mark.parametrize("n", N_ENVS)
def test_plan_counts_ranges_shares_and_order(n, phase, hard):
    plan = trainer.mix_plan(PHASES[phase], SCALE, n, hard, "curriculum")
    assert sum(c for _, _, _, c in plan) == n
    nxt = 0
    for mode, red, first, count in plan:                       # contiguous from 0, no empty group
        assert first == nxt and count > 0 and isinstance(red, bool)
        nxt += count
    want = _shares(phase, hard)
    got = {}
    for mode, _, _, count in plan:
        got[mode] = got.get(mode, 0) + count
    assert set(got) <= set(want)
    for mode, f in want.items():                               # within one env of the stated fraction
        assert abs(got.get(mode, 0) - f * n) < 1, (mode, got.get(mode, 0), float(f * n))
    order = ["self", "pool"] + list(hard) + ["random"]
    seen = [m for m, _, _, _ in plan]
    assert seen == sorted(seen, key=order.index)               # self, pool, the hard bots in their order, random
    for mode in ("self", "pool"):                              # a red first half (count // 2) and a blue rest
        parts = [(red, c) for m, red, _, c in plan if m == mode]
        total = sum(c for _, c in parts)
        assert parts == [p for p in ((True, total // 2), (False, total - total // 2)) if p[1]]
    assert all(not red for m, red, _, _ in plan if m not in ("self", "pool"))      # bots and random: the learner is blue


def test_plan_phase_one_fixed_modes_and_ties():
    for n in N_ENVS:
        assert trainer.mix_plan(0, 1.0, n, ("baseline",), "curriculum") == [("random", False, 0, n)]
        assert trainer.mix_plan(200, 1.0, n, ("baseline",), "curriculum") == [("random", False, 0, n)]        # "up to" 200 * scale
        for idx in (0, 500, 5000):                             # a fixed mode does not look at the update index
            assert trainer.mix_plan(idx, 1.0, n, ("baseline", "approxq"), "baseline") == [("baseline", False, 0, n)]
            assert trainer.mix_plan(idx, 1.0, n, ("baseline",), "approxq") == [("approxq", False, 0, n)]
            assert trainer.mix_plan(idx, 1.0, n, ("baseline",), "random") == [("random", False, 0, n)]
    assert trainer.mix_plan(3, 1.0, 7, ("baseline",), "self") == [("self", True, 0, 3), ("self", False, 3, 4)]
    assert trainer.mix_plan(3, 1.0, 1, ("baseline",), "pool") == [("pool", False, 0, 1)]
    # phase 2, two bots, 64 envs: 26.67 + 26.67 + 10.67 -> every remainder is 2/3, the two spare envs go to the EARLIER groups
    assert trainer.mix_plan(201, 1.0, 64, ("baseline", "approxq"), "curriculum") == [("baseline", False, 0, 27), ("approxq", False, 27, 27),
                                                                                      ("random", False, 54, 10)]
    # phase 3, one bot, 64 envs: 25.6 self, 12.8 pool, 21.33 baseline, 4.27 random -> pool (.8) and self (.6) round up
    assert trainer.mix_plan(801, 1.0, 64, ("baseline",), "curriculum") == [("self", True, 0, 13), ("self", False, 13, 13), ("pool", True, 26, 6),
                                                                           ("pool", False, 32, 7), ("baseline", False, 39, 21), ("random", False, 60, 4)]


def test_plan_makes_no_draw():
    """mix_plan is a function of its arguments: it takes no generator, and numpy's and torch's global streams stay where they are."""
    np.random.seed(5)
    torch.manual_seed(5)
    s_np, s_t = np.random.get_state(), torch.get_rng_state()
    a = [trainer.mix_plan(idx, SCALE, 4096, ("baseline", "approxq"), "curriculum") for idx in (0, 50, 200)]
    b = [trainer.mix_plan(idx, SCALE, 4096, ("baseline", "approxq"), "curriculum") for idx in (0, 50, 200)]
    assert a == b
    assert all((x == y).all() if isinstance(x, np.ndarray) else x == y for x, y in zip(s_np, np.random.get_state()))
    assert torch.equal(s_t, torch.get_rng_state())


# ---- the per-env frame helpers against the scalar ones, row by row ----------------------------------------------------
@pytest.mark.parametrize("red_dtype", (torch.bool, torch.uint8))
def test_per_env_actions_equal_the_scalar_map_row_by_row(red_dtype):
    act = torch.arange(5).repeat(2)[:, None].expand(10, 2).contiguous()           # all 5 actions, both colours, [N, 2]
    red = torch.tensor([0] * 5 + [1] * 5).to(red_dtype)
    for dt in (torch.int64, torch.int8):
        out = mappo.canonicalize_action(act.to(dt), red)
        assert out.dtype == dt and out.shape == act.shape
        for e in range(10):
            assert torch.equal(out[e], mappo.canonicalize_action(act[e].to(dt), bool(red[e])))
    flat = mappo.canonicalize_action(act[:, 0].contiguous(), red)                  # a [N] tensor too
    assert flat.tolist() == [mappo.canonicalize_action(int(a), bool(r)) for a, r in zip(act[:, 0], red)]
    assert torch.equal(mappo.canonicalize_action(mappo.canonicalize_action(act, red), red), act)     # its own inverse


@pytest.mark.parametrize("red_dtype", (torch.bool, torch.uint8))
def test_per_env_masks_equal_the_scalar_map_row_by_row(red_dtype):
    bits = torch.arange(32, dtype=torch.uint8).repeat(2)                            # all 32 mask values, both colours
    bits2 = torch.stack((bits, bits.flip(0)), dim=1)                                # [64, 2]
    red = torch.tensor([0] * 32 + [1] * 32).to(red_dtype)
    out = mappo.canonicalize_legal(bits2, red)
    assert out.dtype == torch.int32 and out.shape == (64, 2)
    for e in range(64):
        assert torch.equal(out[e], mappo.canonicalize_legal(bits2[e], bool(red[e])))
        assert out[e, 0].item() == mappo.canonicalize_legal(int(bits2[e, 0]), bool(red[e]))
    # bits above the five actions are dropped, as in the scalar form
    assert torch.equal(mappo.canonicalize_legal(bits2 | 0xE0, red), out)


def test_team_columns_pick_and_write_back():
    rng = np.random.RandomState(3)
    N = 37
    x = torch.from_numpy(rng.randint(-100, 100, size=(N, 4)).astype(np.int32))
    red = torch.from_numpy(rng.randint(0, 2, size=N).astype(np.uint8))
    own, opp = mappo.team_columns(x, red), mappo.team_columns(x, red, opponents=True)
    assert own.shape == opp.shape == (N, 2)
    assert 0 < int(red.sum()) < N
    for e in range(N):
        l, o = ([0, 2], [1, 3]) if red[e] else ([1, 3], [0, 2])                      # the trainer's learner_ids / opp_ids
        assert own[e].tolist() == x[e, l].tolist() and opp[e].tolist() == x[e, o].tolist()
    assert torch.equal(mappo.team_columns(x, red.to(torch.bool)), own)
    # write-back: into the learners' columns only, then the opponents'
    y = torch.full((N, 4), -7, dtype=torch.int8)
    v = torch.from_numpy(rng.randint(0, 5, size=(N, 2)).astype(np.int64))
    assert mappo.set_team_columns(y, red, v) is y
    assert torch.equal(mappo.team_columns(y, red), v.to(torch.int8)) and bool((mappo.team_columns(y, red, opponents=True) == -7).all())
    w = torch.from_numpy(rng.randint(0, 5, size=(N, 2)).astype(np.int8))
    mappo.set_team_columns(y, red, w, opponents=True)
    assert torch.equal(mappo.team_columns(y, red), v.to(torch.int8)) and torch.equal(mappo.team_columns(y, red, opponents=True), w)
    # a slice of the rows (a group of the plan) is written in place
    z = torch.zeros((N, 4), dtype=torch.int8)
    mappo.set_team_columns(z[5:9], red[5:9], torch.ones((4, 2), dtype=torch.int8))
    assert int(z.sum()) == 8 and int(z[5:9].sum()) == 8
    # uniform colour vectors are the scalar column lists
    assert torch.equal(mappo.team_columns(x, torch.ones(N, dtype=torch.uint8)), x[:, [0, 2]])
    assert torch.equal(mappo.team_columns(x, torch.zeros(N, dtype=torch.uint8)), x[:, [1, 3]])


# ---- the checkpoint flag, on the stand-in env of tests/test_mappo_cpu.py ----------------------------------------------
class _StubEnv:
    def __init__(self, layout, n_envs):
        from pmx.layout import get_layout
        self.layout = get_layout(layout)
        self.obs_torch_dtype = torch.float32
        self.n_envs = n_envs

    def reset(self):
        return torch.zeros((self.n_envs, 4, 8, self.layout.height, self.layout.width)), None

    def close(self):
        pass


def _trainer(**kw):
    return trainer.VecMAPPOTrainer("tinyCapture", 4, horizon=2, minibatch=8, device="cpu", seed=1, use_autocast=False, opponent="curriculum",
                                   curriculum_scale=0.1, total_updates=40, env=_StubEnv("tinyCapture", 4), **kw)


def test_checkpoint_carries_the_flag_and_refuses_a_mismatch(tmp_path):
    on, off = _trainer(mix_opponents=True), _trainer()
    assert on.mix_opponents is True and off.mix_opponents is False
    p_on, p_off = str(tmp_path / "on.pt"), str(tmp_path / "off.pt")
    on.update_idx = 7
    on.save_full(p_on)
    off.save_full(p_off)
    assert torch.load(p_on, weights_only=True)["mix_opponents"] == 1
    assert "mix_opponents" not in torch.load(p_off, weights_only=True)          # the default path's file is the one it was
    again = _trainer(mix_opponents=True)
    again.load_full(p_on)
    assert again.update_idx == 7 and again.mix_opponents is True
    _trainer().load_full(p_off)
    with pytest.raises(ValueError, match="mix_opponents=True, this trainer has mix_opponents=False"):
        _trainer().load_full(p_on)
    with pytest.raises(ValueError, match="mix_opponents=False, this trainer has mix_opponents=True"):
        _trainer(mix_opponents=True).load_full(p_off)
