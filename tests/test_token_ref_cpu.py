"""tests/_token_ref.py against float64 autograd: with every rounding switched off the hand-written backward passes are the plain
formulas' gradients (1e-10 relative), so what the GPU tests compare the kernels with is the operation itself plus the kernels'
rounding points and nothing else.  Also holds every committed FFN seed to the excluded-token share the GPU test asserts."""
import pytest
import torch

import _token_ref as R


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


def _leaves(c, names):
    return [c[n].clone().requires_grad_(True) for n in names]


@pytest.mark.parametrize("T", [1, 33, 200])
def test_ffn_reference_without_rounding_is_autograd(T):
    c = R.f64(R.ffn_case(T, 11 + T))
    names = ("x", "w1", "b1", "w2", "b2", "gamma", "beta")
    leaves = _leaves(c, names)
    y = R.ffn_plain(*leaves)
    want = dict(zip(("dx", "dw1", "db1", "dw2", "db2", "dgamma", "dbeta"), torch.autograd.grad(y, leaves, c["dy"])))
    want["y"] = y.detach()
    got = R.ffn_ref_of(c, rounding=False)
    for k, v in want.items():
        assert got[k].shape == v.shape and _rel(got[k], v) <= 1e-10, (k, _rel(got[k], v))


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("T", [1, 33, 200])
def test_tok96_reference_without_rounding_is_autograd(T, with_res):
    c = R.f64(R.tok96_case(T, 12 + T))
    leaves = _leaves(c, ("a", "w", "b"))
    y = R.tok96_plain(*leaves)
    want = dict(zip(("da", "dw", "db"), torch.autograd.grad(y, leaves, c["dy"])))
    if with_res:
        want["da"] = want["da"] + c["res"]
    want["qkv"] = y.detach()
    got = R.tok96_ref_of(c, rounding=False, with_res=with_res)
    for k, v in want.items():
        assert got[k].shape == v.shape and _rel(got[k], v) <= 1e-10, (k, _rel(got[k], v))


@pytest.mark.parametrize("T", [1, 33, 200])
def test_tok32ln_reference_without_rounding_is_autograd(T):
    c = R.f64(R.tok32ln_case(T, 13 + T))
    leaves = _leaves(c, ("x", "a", "w", "b", "gamma", "beta"))
    y = R.tok32ln_plain(*leaves)
    want = dict(zip(("dx", "da", "dw", "db", "dgamma", "dbeta"), torch.autograd.grad(y, leaves, c["dy"])))
    want["y"] = y.detach()
    got = R.tok32ln_ref_of(c, rounding=False)
    for k, v in want.items():
        assert got[k].shape == v.shape and _rel(got[k], v) <= 1e-10, (k, _rel(got[k], v))


def test_rounding_moves_the_references_by_bfloat16_steps_only():
    """The switch does something, and what it does is of the size of bfloat16 rounding."""
    c = R.ffn_case(200, 7)
    on, off = R.ffn_ref_of(c), R.ffn_ref_of(c, rounding=False)
    for k in ("y", "dx", "dw1", "dw2", "db1", "db2"):
        d = _rel(on[k], off[k])
        # (a flipped ReLU mask moves dx, dw1 and db1 by a whole hidden unit's share: only the others are held to the rounding's size)
        assert 0.0 < d and (d < 4 * 2 ** -8 or k in ("dx", "dw1", "db1")), (k, d)
    assert on["y"].float().to(torch.bfloat16).double().equal(on["y"]) and on["dx"].float().to(torch.bfloat16).double().equal(on["dx"])


def test_hard_row_references_are_the_closed_forms():
    """Zero-variance rows: y = beta and dx = eps**-0.5 (gamma dy - mean(gamma dy)); dead hidden layer: dW1 = db1 = 0, dx = dz."""
    c = R.ffn_case(53, R.ffn_seed(53, "zero_var"), "zero_var")
    ref, d = R.ffn_ref_of(c, rounding=False), R.f64(c)
    hard = R.hard_row_mask(53)
    assert (ref["y"][hard] - d["beta"]).abs().max() <= 1e-12
    gd = d["gamma"] * d["dy"][hard]
    assert _rel(ref["dx"][hard], R.EPS ** -0.5 * (gd - gd.mean(-1, keepdim=True))) <= 1e-10
    assert not ref["dw1"].any() and not ref["db1"].any()                # W2 = 0: nothing flows into the hidden layer
    c = R.ffn_case(53, R.ffn_seed(53, "dead"), "dead")
    ref = R.ffn_ref_of(c)
    assert not ref["dw1"].any() and not ref["db1"].any() and not ref["dw2"].any()
    assert ref["dx"].equal(ref["dz"].float().to(torch.bfloat16).double())
    c = R.tok32ln_case(53, 5, "zero_var")
    ref, d = R.tok32ln_ref_of(c, rounding=False), R.f64(c)
    assert (ref["y"][hard] - d["beta"]).abs().max() <= 1e-12


def test_committed_ffn_seeds_keep_the_excluded_share_below_three_percent_and_the_last_token_in():
    for T, kind in R.fixed_ffn_cases():
        near = R.ffn_ref_of(R.ffn_case(T, R.ffn_seed(T, kind), kind))["near"]
        share = float(near.double().mean())
        assert share < R.MAX_EXCLUDED_SHARE and not bool(near[-1]), (T, kind, share)
