"""tests/_norm_opt_ref.py on the CPU: its float64 references against torch's own operators and autograd on small cases, and every
negative control against the bounds of its case: each must miss by MARGIN = 3 at least, or the GPU tests that rely on the bounds
would wave the same mistake through in a kernel."""
import math

import pytest
import torch
import torch.nn.functional as F

import _norm_opt_ref as R

D = torch.float64


def _close(a, b, tol=1e-11):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ---------------------------------------------------------------------------------------------------------------
# the references against torch
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,bf16", [(1, False), (7, False), (7, True), (70, True)])
def test_ln32_ref_is_layer_norm_and_its_autograd(rows, bf16):
    case = R.ln32_case(rows, 11 + rows, bf16)
    ref, _ = R.ln32_ref(case, D, stats32=False)
    x, a, w, b = (case[k].double().requires_grad_(True) for k in ("x", "a", "w", "b"))
    y = F.layer_norm(x + a, (32,), w, b, R.EPS)
    dx, da, dw, db = torch.autograd.grad(y, (x, a, w, b), case["dy"].double())
    z = (x + a).detach()
    assert _close(ref["y"], y.detach()) and _close(ref["dz"], dx) and _close(ref["dz"], da) and _close(ref["dw"], dw) and _close(ref["db"], db)
    assert _close(ref["mean"], z.mean(1)) and _close(ref["rstd"], 1 / torch.sqrt(z.var(1, unbiased=False) + R.EPS), 1e-9)
    for r, kind in case["kinds"].items():
        if kind in ("constant", "cancel"):
            assert torch.equal(ref["y"][r], case["b"].double()) and float(ref["rstd"][r]) == 1 / math.sqrt(R.EPS)


@pytest.mark.parametrize("B,groups,HW,bf16,with_res,kind", [(3, 1, 5, False, True, "rows"), (5, 3, 65, False, False, "rows"), (5, 3, 70, True, True, "rows"),
                                                            (2, 4, 193, True, True, "tails"), (3, 2, 33, False, False, "cancel")])
def test_gn8_ref_is_group_norm_gelu_and_its_autograd(B, groups, HW, bf16, with_res, kind):
    case = R.gn8_case(B, groups, HW, 5, bf16, with_res, kind)
    ref, _ = R.gn8_ref(case, D, stats32=False)
    h, w, b = (case[k].double().requires_grad_(True) for k in ("h", "w", "b"))
    res = None if case["res"] is None else case["res"].double().requires_grad_(True)
    z = F.group_norm(h, groups, w, b, R.EPS)
    y = F.gelu(z if res is None else z + res)
    leaves = (h, w, b) + (() if res is None else (res,))
    grads = torch.autograd.grad(y, leaves, case["dy"].double())
    shape = (B, groups * 8, HW)
    assert _close(ref["y"].view(shape), y.detach()) and _close(ref["dh"].view(shape), grads[0], 1e-9)
    assert _close(ref["partial"].view(B, groups * 8, 2).sum(0)[:, 0], grads[1], 1e-9) and _close(ref["partial"].view(B, groups * 8, 2).sum(0)[:, 1], grads[2])
    if res is not None:
        assert _close(ref["dres"].view(shape), grads[3])
    hh = case["h"].double().view(B * groups, -1)
    assert _close(ref["mean"], hh.mean(1)) and _close(ref["rstd"], 1 / torch.sqrt(hh.var(1, unbiased=False) + R.EPS), 1e-9)
    if kind == "tails":
        zz = (z if res is None else z + res).detach()
        assert float(zz.max()) > 11 and float(zz.min()) < -11
    if kind == "cancel":
        assert float((z + res).detach().abs().max()) < 0.05


def test_optimizer_ref_is_clip_grad_norm_adam_and_the_ema_line():
    """Two steps of torch.optim.Adam behind clip_grad_norm_ in float64, the EMA line of the trainer after each; the reference is given
    the exact norm here (its own is rounded to float32, as the kernel's is)."""
    hp = R.hp32()
    lr = 3e-4
    for kind in ("small", "large"):
        st = {k: v.double() for k, v in R.opt_state(1000, 3, kind).items()}
        st["m"], st["v"] = torch.zeros(1000, dtype=D), torch.zeros(1000, dtype=D)
        p = torch.nn.Parameter(st["p"].clone())
        opt = torch.optim.Adam([p], lr=lr, betas=(hp["b1"], hp["b2"]), eps=hp["eps"])
        ema = st["ema"].clone()
        for t in (1, 2):
            g = R.opt_state(1000, 3 + t, kind)["g"].double()
            p.grad = g.clone()
            torch.nn.utils.clip_grad_norm_([p], hp["max_norm"])
            opt.step()
            ema = ema * hp["decay"] + p.detach() * (1 - hp["decay"])
            h = dict(hp, lr_bc1=lr / (1 - hp["b1"] ** t), rsqrt_bc2=1 / math.sqrt(1 - hp["b2"] ** t))
            out, _ = R.opt_ref({**st, "g": g}, D, hp=h, norm=g.norm())
            state = opt.state[p]
            assert _close(out["g"], p.grad, 1e-7) and _close(out["m"], state["exp_avg"], 1e-7) and _close(out["v"], state["exp_avg_sq"], 1e-6)
            assert _close(out["p"], p.detach(), 1e-7) and _close(out["ema"], ema, 1e-7)
            st = {"g": g, "p": p.detach().clone(), "m": state["exp_avg"].clone(), "v": state["exp_avg_sq"].clone(), "ema": ema.clone()}


def test_optimizer_norm_and_scale_edges():
    hp = R.hp32()
    below, above = R.opt_state(4097, 1, "below"), R.opt_state(4097, 1, "above")
    assert float(R.opt_norm(below["g"])) + 1e-6 < hp["max_norm"] < float(R.opt_norm(above["g"]))
    assert torch.equal(R.opt_ref(below, torch.float32)[0]["g"], below["g"])                 # scale exactly 1
    assert not torch.equal(R.opt_ref(above, torch.float32)[0]["g"], above["g"])
    huge = R.opt_state(1025, 1, "huge")
    assert math.isinf(float(R.opt_norm(huge["g"], squares32=True))) and math.isfinite(float(R.opt_norm(huge["g"])))
    zero = R.opt_state(5, 1, "zero")
    assert float(R.opt_norm(zero["g"])) == 0.0 and bool(torch.isfinite(R.opt_ref(zero, D)[0]["p"]).all())


def test_colsum_ref():
    x = R.colsum_case(45, 96, 1)
    ref, scale = R.colsum_ref(x, D)
    want = torch.tensor([sum(float(v) for v in x[:, c]) for c in range(96)], dtype=D)
    assert _close(ref["colsum"], want) and bool((scale["colsum"] >= ref["colsum"].abs()).all())
    assert float(scale["colsum"].max() / scale["colsum"].min()) > 1e3                        # small columns beside large ones


def test_bounds_treat_zero_scales_and_nans_as_asked():
    ref, scale = torch.tensor([[0.0, 0.0], [1.0, -2.0]], dtype=D), torch.tensor([[0.0], [2.0]], dtype=D)
    assert R.excess(ref.float(), ref, scale, R.FLOOR) == 0.0
    assert R.excess(torch.tensor([[0.0, 1e-30], [1.0, -2.0]]), ref, scale, R.FLOOR) == math.inf      # an all-zero row stays exactly zero
    assert R.excess(torch.tensor([[0.0, 0.0], [math.nan, -2.0]]), ref, scale, R.FLOOR) == math.inf
    assert R.excess(torch.tensor([[0.0, 0.0], [1.0, -2.0 - 2.0 ** -7]], dtype=D), ref, scale, R.FLOOR, bf16=True) <= 1.0      # 2**-8 of 2
    assert R.excess(torch.tensor([[0.0, 0.0], [1.0, -2.0 - 2.0 ** -6]], dtype=D), ref, scale, R.FLOOR, bf16=True) > 1.9


# ---------------------------------------------------------------------------------------------------------------
# every negative control misses the bounds of its case threefold
# ---------------------------------------------------------------------------------------------------------------
def _all_miss(tag, ctl, expected):
    worst = R.worst_by_output(ctl)
    for what, x in worst.items():
        print(f"NORMNEG {tag} {what}: of its bound {x:.1f}")
    assert set(worst) == set(expected), (tag, sorted(worst))
    assert all(x >= R.MARGIN for x in worst.values()), (tag, worst)


@pytest.mark.parametrize("rows,bf16", R.ln32_cases())
def test_ln32_controls_miss(rows, bf16):
    case = R.ln32_case(rows, R.ln32_seed(rows, bf16), bf16)
    ref, scale, Fs = R.study(lambda dt: R.ln32_ref(case, dt))
    expected = set()
    if rows > 1:
        expected.add("x + a rounded to bfloat16" if bf16 else "one-pass variance in float32")
    if rows > R.LN32_BWD_TRIP:
        expected.add("rows past the first backward trip left out")
    _all_miss(f"ln32 rows={rows} bf16={bf16}", R.ln32_controls(case, ref, scale, Fs, bf16), expected)


@pytest.mark.parametrize("layout,bf16,HW", [c for c in R.gn8_cases() if c[0] == "nchw"])
def test_gn8_controls_miss(layout, bf16, HW):
    for B, groups in R.GN_SHAPES:
        for with_res in (False, True):
            case = R.gn8_case(B, groups, HW, R.gn8_seed(B, groups, HW, bf16, with_res), bf16, with_res)
            ref, scale, Fs = R.study(lambda dt: R.gn8_ref(case, dt))
            rows, expected = B * groups, set()
            if "offset" in case["kinds"].values():
                expected.add("one-pass variance in float32")
            if groups > 1:
                expected.add("weights of group row / groups")
            if 64 * R.gn_kmax(HW) > HW:
                expected.add("idle lane slots counted into the variance")
            if rows % 4:
                expected.add("last row of a partly filled block dropped")
            _all_miss(f"gn8 B={B} groups={groups} HW={HW} bf16={bf16} res={with_res}", R.gn8_controls(case, ref, scale, Fs, bf16), expected)


@pytest.mark.parametrize("n,kind", [(n, k) for n, k in R.opt_cases() if k in ("tail_mass", "huge", "large", "late_mass")])
def test_optimizer_controls_miss(n, kind):
    state = R.opt_state(n, R.opt_seed(n, kind), kind)
    ref, scale, Fs = R.study(lambda dt: R.opt_ref(state, dt))
    expected = {"tail_mass": {"the n & 3 tail left out of the norm"}, "huge": {"squares formed in float32"}}.get(kind, set())
    if n > R.OPT_UPDATE_TRIP and kind in ("large", "late_mass"):
        expected = expected | {"elements past the update's first trip unchanged"}
    _all_miss(f"opt n={n} {kind}", R.opt_controls(state, ref, scale, Fs, kind), expected)
    p = ref["p"].float()
    if n >= 1000:                                                                            # truncation is no rounding: about half the elements differ
        assert int((R.bf16_truncate(p).view(torch.int16) != p.to(torch.bfloat16).view(torch.int16)).sum()) >= n // 4
