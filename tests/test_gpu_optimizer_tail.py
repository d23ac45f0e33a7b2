"""The optimizer tail (csrc/pmx_train.hip: pmx_clip_adam_ema / pmx_clip_adam_ema_tail, i.e. pmx_sqsum_partial_kernel and
pmx_adam_ema_kernel) through the C ABI against the float64 reference of tests/_norm_opt_ref.py: per ELEMENT, at the sizes where
either launch saturates its grid and strides, with the n & 3 remainder, host and device step sizes, gradients on both sides of and a
hair off the clip threshold, squares that overflow float32, three consecutive steps at the model's size, non-finite gradients.

Grid caps of the two launches.  tests/test_gpu_norm_kernels.py::test_launcher_caps looks the literals up in the source.
    launch                       blocks of 256 threads                        one trip             csrc/pmx_train.hip
    pmx_sqsum_partial_kernel     min(max(ceil(n / 4 / 256), 1), PMX_OPT_PARTIALS = 1024), a float4 per thread and trip;
                                 the n & 3 floats behind the last float4 by block 0           1 048 576 floats     lines 1955-1957, 1889
    pmx_adam_ema_kernel          min(ceil(n / 256), 2048)                                     524 288 elements     lines 1959-1960

Reference: norm = float32(sqrt(sum g^2 in float64)); scale = min(1, max_norm / (norm + 1e-6)); then the kernel's five lines for g, m,
v, p, ema.  Bounds (none taken from the kernels' output): per element |got - ref64| <= F * scale with F = 4 x the ratio of the
reference's float32 run on the same case and output, at least 16 * 2**-24.  The scale is the value itself where the line is one
product or a sum of positive terms (g, v), and the sum of the magnitudes of the line's terms where it adds terms of either sign:
|m| + (1 - b1)(|g| + |m|) for m, |p| + |step| for p, |decay * ema| + |(1 - decay) * p| for ema.  norm_out: within 2 float32 ulps of
the reference norm.  The bfloat16 copy: p.to(torch.bfloat16) of the kernel's own p, bit for bit.  report_sums6: the float32 sums
bit for bit.  Host step sizes against sc_dev, pmx_clip_adam_ema against _tail, and _tail with each of its optional pointers NULL:
bit for bit in g, p, m, v, ema and the norm.  The negative controls that apply to a case must fail these bounds
(tests/test_norm_opt_ref_cpu.py holds each to a threefold miss).

Non-finite gradients (test_non_finite_gradient_poisons_what_the_torch_tail_poisons): before this file the kernel formed its clip
factor with fminf, which drops a NaN, so a NaN norm gave the factor 1 and poisoned the NaN elements alone (2 607 of 2 608 elements
stayed finite where PPOLearner._torch_tail and clip_grad_norm_ leave none).  The kernel now passes a NaN ratio through.

Measured on an MI355X (`NORMFIG` lines; information only: the worst |got - ref| / scale per output over every case, its F):
    g 7.853e-8 (F at its floor 9.5e-7)    m 1.553e-5 (third of three steps at n = 6 009 174, F 6.2e-5: a large m against a small step)
    v 3.070e-7 (F 1.2e-6)    p 2.703e-7 (n = 524 287, v = 0: F 1.1e-6)    ema 2.798e-7 (F 1.1e-6)    norm_out: 0 ulps in every case
    m, v, p, ema sit at F / 4 exactly on their worst cases: the kernel and the float32 run of the reference round alike there.
    negative controls: none passes; the smallest misses are 7.3e6 (elements past the update's first trip unchanged), 1.0e6 (squares in
    float32: the bound is hit at infinity's stand-in), 2.7e7 (n & 3 tail left out); truncation differs from the bfloat16 copy at
    every n >= 1 000.

Mutation check (scratch copies of the kernels, not committed): the norm kernel without its n & 3 line fails 65 cases of
test_optimizer_tail, some at every n that is no multiple of 4: up to n = 1 025 every gradient kind but `zero`; from 524 287 up
`tail_mass` always (g, v, p millions of times over their bounds), the random kinds where the two or three lost squares move
norm_out by more than its 2 ulps (3 to 7 ulps; `large` and `below` mostly), the others not: there the remainder is a millionth
of the norm, which is why `tail_mass` exists;  the update loop's stride halved fails 87 cases of test_optimizer_tail (every n from 1 023 up, every
kind) and test_three_steps_on_one_state_at_the_model_size.  The three mutations of the norm kernels and what they fail are listed in
tests/test_gpu_norm_kernels.py; none of them fails a test of this file."""
import math

import pytest
import torch

import _norm_opt_ref as R
from test_gpu_norm_kernels import Arena, _controls_fail, _hold, _libs, _nan_pattern, _st, PMX_ERR_INVALID

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
NAMES = ("g", "p", "m", "v", "ema")
REPORTS = (0.5, -1.25, 2.0, 0.125, 3.0)
SUMS0 = (1.0, 2.0, 3.0, 4.0, 5.0, 6.0)
MODEL = "model"                            # the size of MAPPOAgent((8, 18, 20), 5, 2)'s bucket, read at test time


def _model_numel():
    from pmx import mappo
    return sum(p.numel() for p in mappo.MAPPOAgent((8, 18, 20), 5, 2).parameters() if p.requires_grad)


def _cases():
    return R.opt_cases() + [(MODEL, k) for k in R.OPT_GRAD_KINDS if k != "huge"]


class TailRun:
    """One call of the optimizer tail on a copy of `state`; every buffer the kernels write sits between canary bands."""

    def __init__(self, state, hp=None, sc_dev=False, tail=True, reports=True, sums=True, bf16=True):
        self.L, self.lib = _libs()
        self.arena = arena = Arena()
        self.n = n = state["g"].numel()
        self.t = {}
        for k in NAMES:
            self.t[k] = arena(n, F32)
            self.t[k].copy_(state[k])
        self.scratch, self.norm, self.p16 = arena(R.OPT_PARTIALS, F64), arena(1, F32), arena(n, BF16)
        self.sums = arena(6, F32)
        self.sums.copy_(torch.tensor(SUMS0))
        self.reports = torch.tensor(REPORTS, device="cuda")
        hp = R.hp32() if hp is None else hp
        self.sc = torch.tensor([hp["lr_bc1"], hp["rsqrt_bc2"]], dtype=F32, device="cuda")
        scalars = (self.sc.data_ptr(), 0.0, 0.0) if sc_dev else (None, hp["lr_bc1"], hp["rsqrt_bc2"])
        self.args = [self.t[k].data_ptr() for k in ("g", "p", "m", "v", "ema")] + [n, self.scratch.data_ptr(), *scalars, hp["b1"], hp["b2"], hp["eps"],
                                                                                    hp["max_norm"], hp["decay"], self.norm.data_ptr()]
        self.fn = self.lib.pmx_clip_adam_ema
        if tail:
            self.fn = self.lib.pmx_clip_adam_ema_tail
            self.args += [self.p16.data_ptr() if bf16 else None, self.reports.data_ptr() if reports else None, self.sums.data_ptr() if sums else None]
        self.args.append(_st())

    def __call__(self):
        self.L.check(self.fn(*self.args), self.fn.__name__)
        self.arena.assert_bands_intact()
        return self

    def same_bits(self, other, what):
        for k in NAMES:
            assert torch.equal(self.t[k].view(torch.int32), other.t[k].view(torch.int32)), (what, k)
        assert torch.equal(self.norm.view(torch.int32), other.norm.view(torch.int32)), (what, "norm")


def _blocks(n):
    return min(max((n // 4 + 255) // 256, 1), R.OPT_PARTIALS)


@pytest.mark.parametrize("n,kind", _cases())
def test_optimizer_tail(n, kind):
    n = _model_numel() if n == MODEL else n
    state = R.opt_state(n, R.opt_seed(n, kind), kind, "cuda")
    ref, scale, F = R.study(lambda dt: R.opt_ref(state, dt))
    host = TailRun(state)()
    fails, tag = [], f"n={n}/{kind}"
    _hold("opt", tag, host.t, ref, scale, F, (), fails)
    _controls_fail("opt", tag, R.opt_controls(state, ref, scale, F, kind), fails)
    ulps = int(R.ulps_apart32(host.norm, R.opt_norm(state["g"]).reshape(1)))
    print(f"NORMFIG opt norm {tag} {ulps} ulps")
    assert not fails and ulps <= 2, (tag, fails, ulps)
    # the bfloat16 copy: the kernel's own p rounded to nearest even; truncation (negative control) is something else
    assert torch.equal(host.p16.view(torch.int16), host.t["p"].to(BF16).view(torch.int16))
    assert n < 1000 or not torch.equal(R.bf16_truncate(host.t["p"]).view(torch.int16), host.p16.view(torch.int16))
    # the norm launch's partial sums: one double per block, nothing behind them
    blocks = _blocks(n)
    assert bool(torch.isfinite(host.scratch[:blocks]).all()) and _nan_pattern(host.scratch[blocks:])
    # the report sums
    want = torch.tensor(SUMS0, device="cuda") + torch.cat([host.reports, host.norm])
    assert torch.equal(host.sums, want)
    # device step sizes; the entry point without the tail's extras; the extras left out one by one
    dev = TailRun(state, sc_dev=True)()
    dev.same_bits(host, "sc_dev")
    assert torch.equal(dev.p16.view(torch.int16), host.p16.view(torch.int16)) and torch.equal(dev.sums, host.sums)
    plain = TailRun(state, tail=False)()
    plain.same_bits(host, "pmx_clip_adam_ema")
    assert _nan_pattern(plain.p16) and torch.equal(plain.sums, torch.tensor(SUMS0, device="cuda"))
    bare = TailRun(state, reports=False, bf16=False)()
    bare.same_bits(host, "no reports5, no bfloat16 copy")
    assert _nan_pattern(bare.p16) and torch.equal(bare.sums, torch.tensor(SUMS0, device="cuda") + torch.cat([torch.zeros(5, device="cuda"), host.norm]))
    none = TailRun(state, sums=False)()
    none.same_bits(host, "no report sums")
    assert torch.equal(none.sums, torch.tensor(SUMS0, device="cuda"))


def test_three_steps_on_one_state_at_the_model_size():
    """g, m, v, p and ema are written back: three steps on the kernels' own state against three steps of the reference on its own,
    so that an error in what a step leaves behind compounds.  F is that of the float32 run after the same three steps."""
    n = _model_numel()
    hp, lr = R.hp32(), 3e-4
    st_k = R.opt_state(n, 5, "large", "cuda")
    st = {F64: {k: v.double() for k, v in st_k.items()}, F32: dict(st_k)}
    for t in (1, 2, 3):
        g = R.opt_state(n, 5 + t, "large" if t % 2 else "small", "cuda")["g"]
        h = R.hp32(dict(R.HP, lr_bc1=lr / (1 - hp["b1"] ** t), rsqrt_bc2=1 / math.sqrt(1 - hp["b2"] ** t)))
        outs = {}
        for dt in (F64, F32):
            outs[dt], scale = R.opt_ref({**st[dt], "g": g}, dt, hp=h)
            if dt == F64:
                scale64 = scale
            st[dt] = dict(outs[dt])
        run = TailRun({**st_k, "g": g}, hp=h)()
        st_k = {k: run.t[k].clone() for k in NAMES}
        F = {k: max(4.0 * R.ratio(outs[F32][k], outs[F64][k], scale64[k]), R.FLOOR) for k in NAMES}
        fails = []
        _hold("opt", f"n={n}/step={t}", run.t, outs[F64], scale64, F, (), fails)
        assert not fails, (t, fails)
        assert torch.equal(run.p16.view(torch.int16), run.t["p"].to(BF16).view(torch.int16))


@pytest.mark.parametrize("bad", [math.nan, math.inf])
def test_non_finite_gradient_poisons_what_the_torch_tail_poisons(bad):
    """One NaN (or +Inf) element in the gradient: the fused tail and PPOLearner._torch_tail leave the same elements of g, m, v, p, ema
    finite and report a norm that is finite in both or in neither.  clip_grad_norm_'s clamp(NaN, max=1) is NaN, so a NaN norm
    poisons every weight; an infinite norm gives scale 0, and inf * 0 poisons the one element."""
    from pmx import mappo
    res = {}
    for fused in (True, False):
        torch.manual_seed(1)
        m = torch.nn.Sequential(torch.nn.Linear(37, 53), torch.nn.Linear(53, 11)).cuda()
        L = mappo.PPOLearner(m, lr=3e-4)
        L.fused_optimizer = fused
        g = torch.Generator(device="cuda").manual_seed(100)
        L.bucket.grad.copy_(torch.randn(L.bucket.numel, device="cuda", generator=g) * 0.05)
        L.bucket.grad[1234] = bad
        if fused:
            assert L._use_fused_tail()
            L.step_count += 1
            norm = L._fused_tail().clone()
        else:
            norm = L._torch_tail()
        res[fused] = {"g": L.bucket.grad, "m": L.exp_avg, "v": L.exp_avg_sq, "p": L.bucket.data, "ema": L.ema, "norm": norm.reshape(1)}
    for k in res[True]:
        a, b = torch.isfinite(res[True][k]), torch.isfinite(res[False][k])
        assert torch.equal(a, b), (k, "finite in the fused tail:", int(a.sum()), "in the torch tail:", int(b.sum()))
    assert int(torch.isfinite(res[True]["p"]).sum()) == (0 if math.isnan(bad) else res[True]["p"].numel() - 1)


def test_bad_arguments_are_refused_and_nothing_is_written():
    state = R.opt_state(1025, 1, "small", "cuda")
    run = TailRun(state)
    for i in (0, 1, 2, 3, 4, 6):
        assert run.fn(*[None if j == i else a for j, a in enumerate(run.args)]) == PMX_ERR_INVALID, i
    for n in (0, -1):
        assert run.fn(*[n if j == 5 else a for j, a in enumerate(run.args)]) == PMX_ERR_INVALID, n
    run.arena.assert_bands_intact()
    assert all(torch.equal(run.t[k], state[k]) for k in NAMES)
    assert _nan_pattern(run.scratch) and _nan_pattern(run.norm) and _nan_pattern(run.p16) and torch.equal(run.sums, torch.tensor(SUMS0, device="cuda"))
