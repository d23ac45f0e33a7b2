"""tests/_tails_ref.py on the CPU: with every rounding switched off the hand-written references are float64 autograd of the plain
modules (nn.LayerNorm(512), nn.GELU(), nn.Linear; tokens.mean(1) and the critic head) to 1e-12 relative; with the roundings on
they move by a few bfloat16 steps and no more; and for every case of tests/test_gpu_head_tails.py the bounds made from the float32
run of the reference are missed by every negative control by a factor of 3 at least, so that the GPU test cannot pass a kernel that
drops a sample or a ragged trip.  One hard kind is restricted to the edge size: the critic's `large` tokens
(CRITIC_KIND_SIZES_OF in tests/_tails_ref.py says why)."""
import pytest
import torch

import _tails_ref as R

HEADS_PARTIAL_ROWS = 128        # PMX_HEADS_PARTIAL_ROWS of include/pmx.h; test_partial_row_cap_is_the_headers holds it to the binding
ROUNDED_STEPS = {"actor": 4, "critic": 8}       # the rounded references lie within this many bfloat16 steps of the unrounded ones


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


def test_partial_row_cap_is_the_headers():
    from pmx import _lib
    assert _lib.HEADS_PARTIAL_ROWS == HEADS_PARTIAL_ROWS


@pytest.mark.parametrize("kind", R.ACTOR_ROW_KINDS)
@pytest.mark.parametrize("B", [1, 5, 67])
def test_actor_reference_without_rounding_is_autograd(B, kind):
    c = R.cast(R.actor_case(B, 21 + B, kind, io_bf16=False))
    leaves = [c[n].clone().requires_grad_(True) for n in ("h", "lnw", "lnb", "w2", "b2")]
    y = R.actor_tail_plain(*leaves)
    want = dict(zip(("dh", "dlnw", "dlnb", "dw2", "db2"), torch.autograd.grad(y, leaves, c["dlogits"])))
    want["logits"] = y.detach()
    var, mean = torch.var_mean(c["h"], -1, unbiased=False)
    want["stats"] = torch.stack([mean, (var + R.EPS).rsqrt()], -1)
    got = R.actor_ref_of(c, rounding=False)
    for k, v in want.items():
        assert got[k].shape == v.shape and _rel(got[k], v) <= 1e-12, (k, _rel(got[k], v))
    # the backward half started from given statistics is the same function
    again = R.actor_ref_of(c, rounding=False, stats=got["stats"])
    for k in ("dh",) + R.ACTOR_PARAM_GRADS:
        assert torch.equal(again[k], got[k]), k


@pytest.mark.parametrize("kind", R.CRITIC_TOKEN_KINDS)
@pytest.mark.parametrize("B,S", [(1, 1), (5, 7), (19, 33)])
def test_critic_reference_without_rounding_is_autograd(B, S, kind):
    c = R.cast(R.critic_case(B, S, 22 + B, kind))
    leaves = [c[n].clone().requires_grad_(True) for n in ("tokens", "w1", "b1", "w2", "b2")]
    y = R.critic_tail_plain(*leaves)
    want = dict(zip(("dtokens", "dw1", "db1", "dw2", "db2"), torch.autograd.grad(y, leaves, c["dvalue"])))
    want["value"], want["pooled"] = y.detach(), c["tokens"].mean(1)
    got = R.critic_ref_of(c, rounding=False)
    for k, v in want.items():
        assert got[k].shape == v.shape and _rel(got[k], v) <= 1e-12, (k, _rel(got[k], v))
    again = R.critic_ref_of(c, rounding=False, pooled=got["pooled"])
    for k in want:
        assert torch.equal(again[k], got[k]), k


def test_rounding_moves_the_references_by_bfloat16_steps_only():
    """The switch does something, and what it does is of the size of bfloat16 rounding."""
    c = R.actor_case(200, 7)
    on, off = R.actor_ref_of(c), R.actor_ref_of(c, rounding=False)
    for k in ("logits", "dh", "dw2", "dlnw", "dlnb"):
        d = _rel(on[k], off[k])
        assert 0.0 < d < ROUNDED_STEPS["actor"] * 2.0 ** -8, (k, d)
    assert torch.equal(on["stats"], off["stats"]) and torch.equal(on["db2"], off["db2"])          # nothing is rounded on their way
    assert on["dh"].float().to(torch.bfloat16).double().equal(on["dh"])
    f32 = R.actor_case(200, 7, io_bf16=False)
    assert not R.actor_ref_of(f32)["dh"].float().to(torch.bfloat16).double().equal(R.actor_ref_of(f32)["dh"])     # float32 IO: dh unrounded
    c = R.critic_case(200, 7, 8)
    on, off = R.critic_ref_of(c), R.critic_ref_of(c, rounding=False)
    for k in ("pooled", "value", "dtokens", "dw1", "db1", "dw2"):
        d = _rel(on[k], off[k])
        assert 0.0 < d < ROUNDED_STEPS["critic"] * 2.0 ** -8, (k, d)
    assert torch.equal(on["db2"], off["db2"])
    for k in ("pooled", "dtokens"):
        assert on[k].float().to(torch.bfloat16).double().equal(on[k]), k


def test_hard_row_references_are_the_closed_forms():
    """Zero-variance rows: mean = the constant, rstd = eps**-0.5, logits = W2 gelu(LN.bias) + b2, dh = eps**-0.5 (gd - mean(gd)) with
    gd = LN.weight * dz; samples without an incoming gradient: dh, dtokens exactly zero; constant tokens pool to themselves."""
    c = R.actor_case(9, 5, "zero_var", io_bf16=False)
    ref, d = R.actor_ref_of(c, rounding=False), R.cast(c)
    hard = R.hard_row_mask(9)
    assert hard.tolist() == [False, True] * 4 + [False]
    assert torch.equal(ref["stats"][hard][:, 0], d["h"][hard][:, 0]) and _rel(ref["stats"][hard][:, 1], torch.full((4,), R.EPS ** -0.5, dtype=torch.float64)) <= 1e-12
    want = R.gelu(d["lnb"]) @ d["w2"].T + d["b2"]
    assert _rel(ref["logits"][hard], want.expand(4, 5)) <= 1e-12
    gd = d["lnw"] * (d["dlogits"][hard] @ d["w2"]) * R.gelu_grad(d["lnb"])
    assert _rel(ref["dh"][hard], R.EPS ** -0.5 * (gd - gd.mean(-1, keepdim=True))) <= 1e-10
    c = R.actor_case(9, 6, dl_kind="quarter_zero")
    zero = R.zero_sample_mask(9)
    assert zero.tolist() == [True, False, False, False, True, False, False, False, False]
    assert not R.actor_ref_of(c)["dh"][zero].any() and R.actor_ref_of(c)["dh"][~zero].any(-1).all()
    c = R.critic_case(9, 7, 7, "constant", "quarter_zero")
    ref = R.critic_ref_of(c)
    assert torch.equal(ref["pooled"][hard], c["tokens"][hard][:, 0].double())
    assert not ref["dtokens"][zero].any() and ref["dtokens"][~zero].any(-1).all()
    z = R.cast(R.actor_case(64, 9, "tails"))
    zz = torch.nn.functional.layer_norm(z["h"], (512,), z["lnw"], z["lnb"], R.EPS).abs()
    assert float(zz.min()) > 1.5 and float(zz.max()) < 8.5 and float(((zz > 3) & (zz < 8)).double().mean()) > 0.99
    far = R.actor_case(64, 9, "far_offset", io_bf16=False)["h"][R.hard_row_mask(64)]
    assert float((far.mean(-1) - 1000).abs().max()) < 1 and 0.25 < float(far.std(-1).min()) and float(far.std(-1).max()) < 1.2


def _assert_margins(tag, bnd, ctl):
    fails = []
    for what, name, margin in ctl:
        print(f"TAILCTL {tag} {name} {what}: F {bnd[name]:.3e}, misses by a factor of {margin:.1f}")
        if not margin >= R.MARGIN:
            fails.append((what, name, margin, bnd[name]))
    assert not fails, (tag, fails)


@pytest.mark.parametrize("B,kind,dl_kind,io_bf16", R.actor_cases())
def test_every_actor_control_misses_its_bound_threefold(B, kind, dl_kind, io_bf16):
    case = R.actor_case(B, R.actor_seed(B, kind, dl_kind, io_bf16), kind, dl_kind, io_bf16)
    _, bnd, ctl = R.actor_study(case, 4 * HEADS_PARTIAL_ROWS)
    assert len(ctl) == (12 if R.ragged_trip(B, 4 * HEADS_PARTIAL_ROWS) else 8)
    _assert_margins(f"actor B={B} {kind} {dl_kind} {'bf16' if io_bf16 else 'f32'}", bnd, ctl)


@pytest.mark.parametrize("B,S,kind,dv_kind", R.critic_cases())
def test_every_critic_control_misses_its_bound_threefold(B, S, kind, dv_kind):
    case = R.critic_case(B, S, R.critic_seed(B, S, kind, dv_kind), kind, dv_kind)
    _, bnd, ctl = R.critic_study(case, 4 * R.CRITIC_BLOCKS)
    assert len(ctl) == (10 if R.ragged_trip(B, 4 * R.CRITIC_BLOCKS) else 6)
    _assert_margins(f"critic B={B} S={S} {kind} {dv_kind}", bnd, ctl)


def test_the_size_tables_cross_the_edges_they_name():
    """The launchers' arithmetic restated: which sizes saturate a grid, take a ragged trip, change the weight-gradient chunking."""
    assert [R.heads_blocks(B, R.ACTOR_FWD_BLOCKS) for B in (1, 4, 5, 4095, 4096, 4097, 8195)] == [1, 1, 2, 1024, 1024, 1024, 1024]
    assert [R.heads_blocks(B, HEADS_PARTIAL_ROWS) for B in (3, 511, 512, 513, 1027)] == [1, 128, 128, 128, 128]
    assert R.ragged_trip(8195, 4096) == slice(8192, 8195) and R.ragged_trip(1027, 512) == slice(1024, 1027)
    assert R.ragged_trip(8195, 512) == slice(8192, 8195) and R.ragged_trip(4099, 2048) == slice(4096, 4099)
    assert R.ragged_trip(4096, 4096) is None and R.ragged_trip(513, 512) == slice(512, 513)
    want = {15: (16, 1), 16: (16, 1), 17: (16, 2), 19: (16, 2), 2048: (16, 128), 2049: (17, 121), 4099: (33, 125)}
    assert {B: R.wgrad_chunks(B, HEADS_PARTIAL_ROWS) for B in want} == want
    assert 2049 - 120 * 17 == 9 and 4099 - 124 * 33 == 7                       # what the last chunks hold
    assert set(want) <= set(R.CRITIC_SIZES) and {1, 3, 4, 5, 2047} <= set(R.CRITIC_SIZES)
