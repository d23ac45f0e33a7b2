"""The critic's token kernels (csrc/pmx_critic.hip: pmx_ffn_*, pmx_tok96_*, pmx_tok32ln_*, the row-sum kernel, pmx_encoder_pack;
csrc/pmx_train.hip: pmx_ln32_*) through the C ABI, against the rounding-mirrored float64 references of tests/_token_ref.py:
per ELEMENT, at the token counts where the grids saturate and the grid-stride loops take a second and a ragged third trip, on
rows that break a careless LayerNorm, with guard bands around every output.

Bounds.  bfloat16 outputs (y, qkv, dx, da): |got - ref| <= 2 * 2**-8 * max|ref| of the tensor.  float32 parameter gradients:
|got - ref| <= GRAD_FACTOR * max|ref| of the tensor, GRAD_FACTOR = 4 x the worst ratio measured on an MI355X (256 CUs) over every
case of this file (edges, looping regime, hard rows); the margin is for the matrix cores' float32 accumulation order and for the
rare token whose ReLU mask or bfloat16 rounding falls the other way in float32.  Every case also builds, from the reference alone,
the gradients without the last token and dx / da with the last token zeroed, and requires that these FAIL the same bounds.

Measured worst ratios max|got - ref| / max|ref| (MI355X, 256 CUs, every case of this file; the case that gave the worst one):
    ffn      dw1 2.429e-4 (live, 4 144)     db1 1.244e-4 (large, 4 144)    dw2 1.098e-4 (live, 4 144)    db2 4.937e-5 (large, 4 144)
             dgamma 1.419e-5 (offset, 4 144)   dbeta 1.292e-7 (65 589 tokens)
    tok96    dw 1.849e-7 (offset, 4 144)    db 1.110e-7 (131 125 tokens)      -- dy is not rounded again: float32 summation order only
    tok32ln  dw 1.810e-4 (offset, 4 144)    db 1.135e-4 (offset, 4 144)    dgamma 6.168e-6 (offset, 4 144)   dbeta 1.351e-7 (65 536 tokens)
    bfloat16 outputs, in units of 2**-8 max|ref| (bound: 2): ffn y 0.65, dx 0.90; tok96 qkv 0.99, da 0.48, da with res 0.84;
             tok32ln y 0.75, dx 0.49, da 0.52
    far_offset rows (4 144 and 53 tokens), their own table: ffn dw1 7.583e-4, db1 7.303e-4, dw2 4.335e-4, db2 4.282e-4, dgamma 1.238e-4;
             tok32ln dw 2.174e-4, db 2.062e-4, dgamma 5.690e-5; bfloat16 outputs there: ffn y 1.67 (one step of a y just above 2), dx 0.81;
             tok32ln y 0.72, dx 0.77, da 0.78
    negative controls: a zeroed last token misses the bfloat16 bound by a factor of 33 at least (65.9 x 2**-8 at 65 537 tokens), a
             dropped last token misses the weakest caught gradient bound by 3.5e-3 / 4.4e-7 at the largest sizes; no case escapes.
    excluded FFN tokens: 0 to 1.9 % (1.86 % at 4 144 N(0, 1) tokens, 1.5 to 1.6 % in the looping regime, 0.9 % zero-variance,
             under 0.05 % on the other hard rows)

FFN tokens with a float64 pre-activation within 1e-4 of zero are left out of the per-element dx check only (a float32 evaluation may
flip their ReLU mask); their share is asserted below 3 % (tests/test_token_ref_cpu.py holds the committed seeds to it on the CPU)."""
import ctypes as C
import math

import pytest
import torch

import _token_ref as R

pytestmark = pytest.mark.gpu

BF16_FACTOR = 2 * 2.0 ** -8
GRAD_FACTOR = {       # 4 x the worst measured ratio (module docstring)
    "ffn": {"dw1": 4 * 2.429e-4, "db1": 4 * 1.244e-4, "dw2": 4 * 1.098e-4, "db2": 4 * 4.937e-5, "dgamma": 4 * 1.419e-5, "dbeta": 4 * 1.292e-7},
    "tok96": {"dw": 4 * 1.849e-7, "db": 4 * 1.110e-7},
    "tok32ln": {"dw": 4 * 1.810e-4, "db": 4 * 1.135e-4, "dgamma": 4 * 6.168e-6, "dbeta": 4 * 1.351e-7},
}
# The far_offset rows (tests/_token_ref.py: rows constant at about 1000, spread 0.3 to 1.1) are not among the cases the table above
# was measured on and have a table of their own, made the same way: there the kernels hold z = x + f in float32 with an ulp of
# 6e-5 beside that spread, which moves every tenth element of bf16(dz) by one step against the float64 reference.
FAR_OFFSET_GRAD_FACTOR = {
    "ffn": {"dw1": 4 * 7.583e-4, "db1": 4 * 7.303e-4, "dw2": 4 * 4.335e-4, "db2": 4 * 4.282e-4, "dgamma": 4 * 1.238e-4},
    "tok32ln": {"dw": 4 * 2.174e-4, "db": 4 * 2.062e-4, "dgamma": 4 * 5.690e-5},
}
FAMILIES = ("ffn", "tok96", "tok32ln")
GRAD_FLOATS = {"ffn": 8416, "tok96": 3232, "tok32ln": 1120}
GRAD_SLICES = {
    "ffn": {"dw2": (0, (32, 128)), "dw1": (4096, (128, 32)), "db1": (8192, (128,)), "db2": (8320, (32,)), "dgamma": (8352, (32,)),
            "dbeta": (8384, (32,))},
    "tok96": {"dw": (0, (96, 32)), "db": (3072, (96,))},
    "tok32ln": {"dw": (0, (32, 32)), "db": (1024, (32,)), "dgamma": (1056, (32,)), "dbeta": (1088, (32,))},
}
CASE_OF = {"ffn": R.ffn_case, "tok96": R.tok96_case, "tok32ln": R.tok32ln_case}
REF_OF = {"ffn": R.ffn_ref_of, "tok96": R.tok96_ref_of, "tok32ln": R.tok32ln_ref_of}
FWD_OUT = {"ffn": "y", "tok96": "qkv", "tok32ln": "y"}
CANARY, NAN_BYTE = 0xA5, 0xFF          # 0xFFFF is a bfloat16 NaN, 0xFFFFFFFF a float32 NaN


def _libs():
    from pmx import _lib
    return _lib, _lib.load()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _fwd_blocks_cap():
    return 2 * _cus()


def _bwd_blocks_cap(fam):
    return min(_cus() if fam == "ffn" else 2 * _cus(), 512)


def _bwd_blocks(fam, T):
    return min((((T + 31) // 32) + 3) // 4, _bwd_blocks_cap(fam))


def _plain_alloc(numel, dtype):
    return torch.empty(numel, dtype=dtype, device="cuda")


class Arena:
    """Outputs cut out of larger buffers of canary bytes and prefilled with a NaN pattern."""
    PAD = 4096

    def __init__(self):
        self.items = []

    def __call__(self, numel, dtype):
        n = numel * torch.empty(0, dtype=dtype).element_size()
        buf = torch.full((self.PAD + n + self.PAD,), CANARY, dtype=torch.uint8, device="cuda")
        buf[self.PAD:self.PAD + n] = NAN_BYTE
        self.items.append((buf, n))
        return buf[self.PAD:self.PAD + n].view(dtype)

    def assert_bands_intact(self):
        for buf, n in self.items:
            assert bool((buf[:self.PAD] == CANARY).all()), "bytes in front of an output changed"
            assert bool((buf[self.PAD + n:] == CANARY).all()), "bytes behind an output changed"


class Run:
    """One family on one case through the C ABI.  mode (tok96 only): "plain" = pmx_tok96_backward, "res_null" =
    pmx_tok96_backward_res with res = NULL, "res" = with the residual gradient."""

    def __init__(self, fam, case, mode="plain", alloc=_plain_alloc):
        from pmx import mappo
        self.L, self.lib = _libs()
        self.fam, self.mode, self.alloc = fam, mode, alloc
        self.d = d = {k: v.cuda().contiguous() for k, v in case.items()}
        self.T = d["dy"].shape[0]
        if fam == "ffn":
            self.pack = mappo.pack_ffn(d["w1"], d["b1"], d["w2"], d["b2"], d["gamma"], d["beta"])
        elif fam == "tok96":
            self.pack = mappo.pack_in_proj(d["w"], d["b"])
        else:
            self.pack = mappo.pack_out_proj(d["w"], d["b"], d["gamma"], d["beta"])

    def _tokens_out(self, width=32):
        return self.alloc(max(self.T, 1) * width, torch.bfloat16).view(max(self.T, 1), width)

    def forward(self, tokens=None):
        d, lib, T = self.d, self.lib, self.T if tokens is None else tokens
        if self.fam == "ffn":
            y = self._tokens_out()
            self.L.check(lib.pmx_ffn_forward(d["x"].data_ptr(), self.pack.data_ptr(), y.data_ptr(), T, R.EPS, _st()), "pmx_ffn_forward")
        elif self.fam == "tok96":
            y = self._tokens_out(96)
            self.L.check(lib.pmx_tok96_forward(d["a"].data_ptr(), self.pack.data_ptr(), y.data_ptr(), T, _st()), "pmx_tok96_forward")
        else:
            y = self._tokens_out()
            self.L.check(lib.pmx_tok32ln_forward(d["x"].data_ptr(), d["a"].data_ptr(), self.pack.data_ptr(), y.data_ptr(), T, R.EPS, _st()),
                         "pmx_tok32ln_forward")
        return y

    def backward(self, tokens=None):
        """-> ({name: token gradient}, the whole gradient buffer [1 + GRAD_PARTIAL_ROWS][floats], pmx_last_partial_rows())"""
        d, lib, T = self.d, self.lib, self.T if tokens is None else tokens
        G = GRAD_FLOATS[self.fam]
        grad = self.alloc((1 + self.L.GRAD_PARTIAL_ROWS) * G, torch.float32).view(1 + self.L.GRAD_PARTIAL_ROWS, G)
        outs = {}
        if self.fam == "ffn":
            outs["dx"] = self._tokens_out()
            self.L.check(lib.pmx_ffn_backward(d["x"].data_ptr(), d["dy"].data_ptr(), self.pack.data_ptr(), outs["dx"].data_ptr(), grad.data_ptr(),
                                              T, R.EPS, _st()), "pmx_ffn_backward")
        elif self.fam == "tok96":
            outs["da"] = self._tokens_out()
            if self.mode == "plain":
                self.L.check(lib.pmx_tok96_backward(d["a"].data_ptr(), d["dy"].data_ptr(), self.pack.data_ptr(), outs["da"].data_ptr(),
                                                    grad.data_ptr(), T, _st()), "pmx_tok96_backward")
            else:
                res = d["res"].data_ptr() if self.mode == "res" else None
                self.L.check(lib.pmx_tok96_backward_res(d["a"].data_ptr(), d["dy"].data_ptr(), self.pack.data_ptr(), res, outs["da"].data_ptr(),
                                                        grad.data_ptr(), T, _st()), "pmx_tok96_backward_res")
        else:
            outs["dx"], outs["da"] = self._tokens_out(), self._tokens_out()
            self.L.check(lib.pmx_tok32ln_backward(d["x"].data_ptr(), d["a"].data_ptr(), d["dy"].data_ptr(), self.pack.data_ptr(),
                                                  outs["dx"].data_ptr(), outs["da"].data_ptr(), grad.data_ptr(), T, R.EPS, _st()),
                         "pmx_tok32ln_backward")
        return outs, grad, lib.pmx_last_partial_rows()


def _param_grads(fam, row0):
    return {name: row0[off:off + math.prod(shape)].view(shape) for name, (off, shape) in GRAD_SLICES[fam].items()}


def _ratio(got, ref, rows=None):
    """max |got - ref| over the tensor (over the given rows) relative to max |ref| of the WHOLE tensor; a reference that is all
    zero admits only exact zeros."""
    err = (got.double() - ref).abs()
    if rows is not None:
        err = err[rows]
    e, scale = (float(err.max()) if err.numel() else 0.0), float(ref.abs().max())
    if not math.isfinite(e):
        return math.inf
    return e / scale if scale > 0 else (0.0 if e == 0 else math.inf)


def _reference(fam, case, mode):
    kw = {"with_res": True} if mode == "res" else {}
    T = case["dy"].shape[0]
    return REF_OF[fam](case, "cuda", **kw), REF_OF[fam](case, "cuda", rows=slice(T - 1, T), **kw)


def check_case(fam, case, kind, mode="plain", forward=True, backward=True, alloc=_plain_alloc):
    """Runs the family on the case and holds every output to the bounds of the module docstring, negative controls included.
    Every figure is printed before anything is asserted.  -> (run, outputs, reference)"""
    run = Run(fam, case, mode, alloc)
    T = run.T
    ref, last = _reference(fam, case, mode)
    tag = f"{fam}{'' if mode == 'plain' else '/' + mode} T={T} kind={kind}"
    fails, got = [], {}
    factor = dict(GRAD_FACTOR[fam], **(FAR_OFFSET_GRAD_FACTOR.get(fam, {}) if kind == "far_offset" else {}))
    if forward:
        name = FWD_OUT[fam]
        got[name] = run.forward()
        r = _ratio(got[name], ref[name])
        print(f"TOKFIG {tag} {name} {r / 2 ** -8:.3f} x 2**-8")
        if not (bool(torch.isfinite(got[name]).all()) and r <= BF16_FACTOR):
            fails.append((name, r))
    if backward:
        outs, grad, rows = run.backward()
        got.update(outs)
        got["grad"], got["rows"] = grad, rows
        keep = None
        if fam == "ffn":
            share = float(ref["near"].double().mean())
            print(f"TOKFIG {tag} excluded_share {share:.5f}")
            if not share < R.MAX_EXCLUDED_SHARE:
                fails.append(("excluded share", share))
            keep = ~ref["near"]
        for name, t in outs.items():
            sel = keep if (fam == "ffn" and name == "dx") else None
            r = _ratio(t, ref[name], sel)
            print(f"TOKFIG {tag} {name} {r / 2 ** -8:.3f} x 2**-8")
            if not (bool(torch.isfinite(t).all()) and r <= BF16_FACTOR):
                fails.append((name, r))
            # negative control: the reference with its last token zeroed must fail this very check
            zeroed = ref[name].clone()
            zeroed[-1] = 0
            rn = _ratio(zeroed, ref[name], sel)
            print(f"TOKNEG {tag} {name} {rn / 2 ** -8:.3f} x 2**-8")
            if not rn > BF16_FACTOR:
                fails.append((name + ": a zeroed last token passes", rn))
        caught = False
        for name, g in _param_grads(fam, grad[0]).items():
            r = _ratio(g, ref[name])
            # negative control: the reference's gradient without the last token
            rn = _ratio(ref[name] - last[name], ref[name])
            print(f"TOKFIG {tag} {name} {r:.3e}   without the last token {rn:.3e}")
            if not (bool(torch.isfinite(g).all()) and r <= factor[name]):
                fails.append((name, r))
            caught = caught or rn > factor[name]
        if not caught:
            fails.append("no parameter gradient's bound notices a dropped last token")
    assert not fails, (tag, fails)
    return run, got, ref


def _seed(fam, T, kind):
    return R.ffn_seed(T, kind) if fam == "ffn" else 1000 + T + 7 * FAMILIES.index(fam)


# ---------------------------------------------------------------------------------------------------------------
# token-count edges: one token, the 16- and 32-token tile edges, a block whose waves 1..3 are idle, a second block
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", R.EDGE_TOKENS)
def test_every_family_at_the_tile_edges(T):
    for fam in FAMILIES:
        case = CASE_OF[fam](T, _seed(fam, T, "normal"))
        _, got, _ = check_case(fam, case, "normal")
        assert got["rows"] == _bwd_blocks(fam, T)
        if fam == "tok96":
            _, null, _ = check_case(fam, case, "normal", mode="res_null", forward=False)
            assert torch.equal(null["da"], got["da"]) and torch.equal(null["grad"][0], got["grad"][0])      # res = NULL is the plain backward
            _, res, _ = check_case(fam, case, "normal", mode="res", forward=False)
            assert torch.equal(res["grad"][0], got["grad"][0])                                                # the parameters do not see res


# ---------------------------------------------------------------------------------------------------------------
# the looping regime: the grid saturated, one wave with a second trip of one token, two trips and a ragged third
# ---------------------------------------------------------------------------------------------------------------
def _looping_tokens(cap_blocks, tokens_per_block, which):
    cap = cap_blocks * tokens_per_block
    return (cap, cap + 1, 2 * cap + 53)[which]


@pytest.mark.parametrize("which", [0, 1, 2], ids=["cap", "cap+1", "2cap+53"])
@pytest.mark.parametrize("fam", FAMILIES)
def test_forward_kernels_past_the_grid_cap(fam, which):
    T = _looping_tokens(_fwd_blocks_cap(), 64, which)
    check_case(fam, CASE_OF[fam](T, _seed(fam, T, "normal")), "normal", backward=False)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["cap", "cap+1", "2cap+53"])
@pytest.mark.parametrize("fam,mode", [("ffn", "plain"), ("tok96", "plain"), ("tok96", "res"), ("tok32ln", "plain")])
def test_backward_kernels_past_the_grid_cap(fam, mode, which):
    T = _looping_tokens(_bwd_blocks_cap(fam), 128, which)
    _, got, _ = check_case(fam, CASE_OF[fam](T, _seed(fam, T, "normal")), "normal", mode=mode, forward=False)
    assert got["rows"] == _bwd_blocks_cap(fam)                 # the grid was saturated: this case ran the regime it names


# ---------------------------------------------------------------------------------------------------------------
# hard rows
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", R.HARD_TOKENS)
@pytest.mark.parametrize("fam,kind", [("ffn", k) for k in R.ROW_KINDS[1:]] + [(f, k) for f in ("tok96", "tok32ln") for k in ("zero_var", "offset", "large")] + [("tok32ln", "far_offset")])
def test_hard_rows(fam, kind, T):
    case = CASE_OF[fam](T, _seed(fam, T, kind), kind)
    modes = ("plain", "res") if fam == "tok96" else ("plain",)
    for mode in modes:
        run, got, ref = check_case(fam, case, kind, mode=mode, forward=(mode == "plain"))
        for name in R.TOKEN_OUTS[fam]:
            if name in got:
                assert bool(torch.isfinite(got[name]).all()), name
        assert bool(torch.isfinite(got["grad"][0]).all())
    if kind == "zero_var" and fam != "tok96":
        hard = R.hard_row_mask(T).cuda()
        beta = run.d["beta"].to(torch.bfloat16)
        assert torch.equal(got["y"][hard], beta.expand(int(hard.sum()), 32))          # a constant row normalises to beta exactly
        gd = run.d["gamma"].double() * run.d["dy"].double()[hard]
        want = R.EPS ** -0.5 * (gd - gd.mean(-1, keepdim=True))
        assert float((got["dx"].double()[hard] - want).abs().max()) <= BF16_FACTOR * float(want.abs().max())
    if kind == "dead":
        g = _param_grads(fam, got["grad"][0])
        assert not bool(g["dw1"].any()) and not bool(g["db1"].any()) and not bool(g["dw2"].any())     # dH is exactly zero
        assert _ratio(got["dx"], ref["dz"]) <= 2.0 ** -8                                              # and dx is dz, rounded once


# ---------------------------------------------------------------------------------------------------------------
# guard bands, overwrite semantics, determinism, tokens == 0
# ---------------------------------------------------------------------------------------------------------------
def _nan_pattern(t):
    return bool((t.contiguous().view(torch.uint8) == NAN_BYTE).all())


@pytest.mark.parametrize("T", R.ABI_TOKENS)
@pytest.mark.parametrize("fam,mode", [("ffn", "plain"), ("tok96", "plain"), ("tok96", "res"), ("tok32ln", "plain")])
def test_outputs_are_written_in_full_and_nothing_else_is(fam, mode, T):
    case = CASE_OF[fam](T, _seed(fam, T, "normal"))
    arena = Arena()
    run, got, _ = check_case(fam, case, "normal", mode=mode, alloc=arena)
    torch.cuda.synchronize()
    arena.assert_bands_intact()
    n = got["rows"]
    assert n == _bwd_blocks(fam, T)
    for name in R.TOKEN_OUTS[fam]:
        assert bool(torch.isfinite(got[name]).all()), name
    grad = got["grad"]
    assert bool(torch.isfinite(grad[:1 + n]).all())              # row 0 was prefilled with NaN: it is overwritten, not accumulated into
    assert _nan_pattern(grad[1 + n:])                            # rows no block owns stay untouched
    again = Arena()
    run.alloc = again
    y2 = run.forward()
    outs2, grad2, n2 = run.backward()
    again.assert_bands_intact()
    assert n2 == n and torch.equal(y2.view(torch.int16), got[FWD_OUT[fam]].view(torch.int16))
    for name, t in outs2.items():
        assert torch.equal(t.view(torch.int16), got[name].view(torch.int16)), name
    assert torch.equal(grad2[:1 + n].view(torch.int32), grad[:1 + n].view(torch.int32))


@pytest.mark.parametrize("fam", FAMILIES)
def test_zero_tokens(fam):
    arena = Arena()
    run = Run(fam, CASE_OF[fam](16, 3), "res" if fam == "tok96" else "plain", arena)
    y = run.forward(tokens=0)                                    # returns OK ...
    outs, grad, n = run.backward(tokens=0)
    torch.cuda.synchronize()
    arena.assert_bands_intact()
    assert _nan_pattern(y) and all(_nan_pattern(t) for t in outs.values())          # ... and writes nothing
    assert n == 0 and not bool(grad[0].any()) and _nan_pattern(grad[1:])            # backward: row 0 zeroed, no partial rows


# ---------------------------------------------------------------------------------------------------------------
# row sums and deferral
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floats", [33, 1120, 3168, 8416])
def test_sum_partial_rows_matches_a_float64_sum(floats):
    L, lib = _libs()
    g = torch.Generator().manual_seed(floats)
    for n_rows in (1, 2, 7, 8, 9, 24, 25, 31, 32, 33, 40, 57, 64, 511, 512):
        arena = Arena()
        total = 1 + n_rows + 3                                   # three more rows behind the ones to be added
        buf = arena(total * floats, torch.float32)
        src = (torch.randn(total, floats, generator=g) * (1.0 + 10.0 * torch.rand(total, 1, generator=g))).cuda()
        buf.copy_(src.view(-1))
        L.check(lib.pmx_sum_partial_rows(buf.data_ptr(), n_rows, floats, _st()), "pmx_sum_partial_rows")
        torch.cuda.synchronize()
        arena.assert_bands_intact()
        out = buf.view(total, floats)
        assert torch.equal(out[1:], src[1:]), n_rows             # rows above n_rows, and row 1 right behind column floats - 1, untouched
        want = src[1:1 + n_rows].double().sum(0)
        bound = 1e-6 * src[1:1 + n_rows].double().abs().sum(0)
        worst = float(((out[0].double() - want).abs() / bound).max())
        print(f"TOKFIG rowsum floats={floats} n_rows={n_rows} {worst:.3f} of the bound")
        assert worst <= 1.0, (n_rows, worst)


@pytest.mark.parametrize("T", [53, 4144])
@pytest.mark.parametrize("fam", FAMILIES)
def test_deferred_row_sums_give_the_undeferred_result(fam, T):
    L, lib = _libs()
    run = Run(fam, CASE_OF[fam](T, _seed(fam, T, "normal")), "res" if fam == "tok96" else "plain", Arena())
    _, plain, n_plain = run.backward()
    lib.pmx_defer_row_sums(1)
    try:
        _, grad, n = run.backward()
    finally:
        lib.pmx_defer_row_sums(0)
    assert n == n_plain == _bwd_blocks(fam, T) and lib.pmx_last_partial_rows() == n
    assert bool(torch.isfinite(grad[1:1 + n]).all()) and _nan_pattern(grad[1 + n:])           # rows 1..n are written, no others
    assert torch.equal(grad[1:1 + n].view(torch.int32), plain[1:1 + n].view(torch.int32))
    L.check(lib.pmx_sum_partial_rows(grad.data_ptr(), n, GRAD_FLOATS[fam], _st()), "pmx_sum_partial_rows")
    assert torch.equal(grad[0].view(torch.int32), plain[0].view(torch.int32))                 # bit for bit the undeferred sums
    run.alloc.assert_bands_intact()


# ---------------------------------------------------------------------------------------------------------------
# the one-launch encoder pack
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_layers", [1, 2, 3, 4])
def test_encoder_pack_equals_the_three_stand_alone_packs(n_layers):
    from pmx import mappo
    torch.manual_seed(40 + n_layers)
    layers = [mappo.CriticEncoderLayer(d_model=32, nhead=4, dim_feedforward=128, dropout=0.0, batch_first=False).cuda() for _ in range(n_layers)]
    with torch.no_grad():
        for layer in layers:
            for p in layer.parameters():
                p.copy_(torch.randn_like(p))
    packs = mappo.encoder_packs(layers)
    assert len(packs) == n_layers
    for layer, got in zip(layers, packs):
        for u, v in zip(got, layer.packs()):
            assert u.dtype == torch.uint8 and torch.equal(u, v)


# ---------------------------------------------------------------------------------------------------------------
# pmx_ln32 past one trip of its loops (forward: 4 096 blocks x 256 rows; backward: 512 blocks x 256 rows)
# ---------------------------------------------------------------------------------------------------------------
def _ln32_inputs(rows, dtype):
    torch.manual_seed(0)
    ln = torch.nn.LayerNorm(32).cuda()
    with torch.no_grad():
        ln.weight.copy_(torch.randn(32).cuda() * 0.3 + 1.0); ln.bias.copy_(torch.randn(32).cuda() * 0.2)
    x = torch.randn(rows, 32, device="cuda").to(dtype)
    a = torch.randn(rows, 32, device="cuda").to(dtype)
    return ln, x, a


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 2e-2)])
def test_ln32_backward_on_a_ragged_third_trip(dtype, tol):
    """test_fused_add_layernorm32_matches_torch's reference and tolerances at 2 * 131 072 + 77 rows."""
    from pmx import mappo
    rows = 2 * 131072 + 77
    ln, x, a = _ln32_inputs(rows, dtype)
    x.requires_grad_(True); a.requires_grad_(True)
    g = torch.randn(rows, 32, device="cuda").to(dtype)
    y = mappo.add_layer_norm_small(x, a, ln)
    y.backward(g)
    got = (y.float(), x.grad.float(), a.grad.float(), ln.weight.grad.clone(), ln.bias.grad.clone())
    ln.zero_grad()
    x2 = x.detach().float().requires_grad_(True); a2 = a.detach().float().requires_grad_(True)
    y2 = torch.nn.functional.layer_norm(x2 + a2, (32,), ln.weight, ln.bias, ln.eps)
    y2.backward(g.float())
    ref = (y2, x2.grad, a2.grad, ln.weight.grad, ln.bias.grad)
    for name, u, v in zip(("y", "dx", "da", "dw", "db"), got, ref):
        scale = float(v.abs().max()) + 1e-6
        err = float((u - v).abs().max())
        print(f"TOKFIG ln32 {dtype} {name} {err / scale:.3e}")
        assert err <= tol * scale * (8 if name in ("dw", "db") and dtype == torch.bfloat16 else 1), name


def test_ln32_forward_on_a_second_trip():
    from pmx import mappo
    rows = 1048576 + 4099
    ln, x, a = _ln32_inputs(rows, torch.bfloat16)
    with torch.no_grad():
        y = mappo.add_layer_norm_small(x, a, ln)
        want = torch.nn.functional.layer_norm(x.float() + a.float(), (32,), ln.weight, ln.bias, ln.eps)
    assert y.dtype == torch.bfloat16
    err, scale = float((y.float() - want).abs().max()), float(want.abs().max()) + 1e-6
    print(f"TOKFIG ln32 forward y {err / scale:.3e}")
    assert err <= 2e-2 * scale
