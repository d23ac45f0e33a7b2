"""The norm kernels of csrc/pmx_train.hip through the C ABI (pmx_ln32_forward / _backward, pmx_gn8_gelu_* in NCHW, pmx_gn8cl_gelu_*
channels-last, pmx_colsum_bf16) against the float64 references of tests/_norm_opt_ref.py: per ROW and per ENTRY, statistics included,
at the row counts where the grids saturate and the grid-stride loops take a second and a ragged last trip, at every HW where the
GroupNorm launchers change their variant, with partly filled last blocks, on rows that break a careless mean, variance or GELU, in
both IO types, with NaN-prefilled outputs between canary bands.

Grid caps of the launchers.  test_launcher_caps looks the literals up in the source, so that a change of a launcher fails here
instead of silently moving the edges.
    launcher                        blocks of 256 lanes                        one trip        csrc/pmx_train.hip
    pmx_ln32_forward                min(ceil(rows / 256), 4096)                1 048 576 rows  line 405
    pmx_ln32_backward               PMX_LN32_PARTIAL_ROWS / 4 = 512, always    131 072 rows    line 421 (every wave writes its partial row)
    pmx_gn8_gelu_forward / _backward      ceil(rows / 4), a wave per (sample, group) row; no loop    lines 556, 574
        elements per lane and channel     KMAX = 3 for HW <= 192, 7 for HW <= 448, else 16 (HW <= 1024)    lines 558-559, 576-577
    pmx_gn8cl_gelu_forward / _backward    the same grid and the same HW edges                        lines 1438-1440, 1453-1455
    pmx_colsum_bf16                 PMX_COLSUM_BLOCKS = 512, always            512 * RP rows, RP = 256 / (C / 8)     lines 275-276
    (the optimizer tail's caps, lines 1955-1960, are tabulated in tests/test_gpu_optimizer_tail.py)

Bounds (tests/_norm_opt_ref.py `study` and `excess`; none is taken from the kernels' output).  float32 outputs: |got - ref64| <=
F * scale, F = 4 x the ratio the float32 run of the reference reaches against its float64 run on the same case and output, at least
16 * 2**-24.  The scale of y, dz, dh, dres is the largest |ref64| of the entry's row (a token row; a (sample, group) row of 8 * HW);
of rstd the value itself, held on its own.  Sums that may cancel are held by the sum of the magnitudes of their summands, taken
from the float64 reference entry by entry: dw and db of ln32 (the float64 sum of the 2048 partial rows), every (row, channel) pair of
the GroupNorm partials, every column of the column sum -- and mean, which is sum(z) / n: on a centred row it cancels to anything
while its float32 error stays that of the summands, so its scale is sum|z| / n, never less than |mean|.  bfloat16 outputs: per
element 2**-8 * |ref64| (what rounding to nearest moves a value by at most) + F * the row's scale; a row whose reference is all zero
must be exactly zero.  The reference forms its wavefront sums in the kernels' order (lane by lane, then the butterfly) and
multiplies by 1.0f / n as they do: on a constant group that product is one rounding off the constant, rstd = 316 magnifies it, and
only a float32 run that does the same tells how far (F grows there, by the arithmetic and not by the kernel).  The backward entry
points are given the reference's statistics rounded to float32.  Every case also requires that the negative controls which apply to
it FAIL these bounds; tests/test_norm_opt_ref_cpu.py holds each to a threefold miss on the CPU.

One deviation from the cases as first listed: the bfloat16 row "x = 256 + 2k, a = -256 + small" cannot do what it is for, since a
bfloat16 a in (-256, -128] is an integer and x + a an integer below 256, which bfloat16 holds exactly.  The row is x = 256 + 2k,
a = -64 - m / 2 instead: x + a lies on half-integers between 128 and 256, which bfloat16 does not have, and the control "x + a
rounded to bfloat16" misses its bound 5 457-fold at least.

Measured on an MI355X (`NORMFIG` lines of every case of this file; information, not the source of any bound: the worst
|got - ref| / scale per output, the case that gave it, that case's F):
    ln32     y, dz bfloat16 3.891e-3 = 0.996 x 2**-8 (rows = 131 071); mean 2.567e-7, rstd 4.169e-7 (rows = 131 073, F 1.0e-6, 1.3e-6);
             dw 1.674e-4 (rows = 65 float32, the offset rows: F 1.3e-3); db 5.847e-8; forward at 1 048 833 rows the same figures
    gn8      NCHW and channels-last give the same figures to the digit: y 3.440e-3, dh 3.117e-3, dres 2.724e-3 in bfloat16 (0.995 of
             the bound: elements just above a power of two rounded the far way); mean 1.839e-7, rstd 2.364e-7 (F at its floor);
             partial 3.473e-5 at HW = 1 (F 1.4e-4: eight numbers per group, x-hat one rounding of the mean away from +-1)
    colsum   3.961e-8 of a column's sum of magnitudes (rows = 256, C = 8)
    mean, rstd, dw, partial sit at F / 4 exactly on their worst cases: kernel and float32 run round alike there.  No float32 output
    used more than 0.33 of its bound; the bfloat16 ones reach 0.996 because 2**-8 |ref| is the exact worst case of the rounding.
    negative controls: none passes; the smallest misses are 124 (idle lane slots in the variance, HW = 1 023), 542 (one-pass
    variance, GroupNorm), 824 (ln32 rows past the first backward trip), 1 081 (row / groups), 13.9 (colsum, last row left out).

Mutation check (scratch copies of the kernels, not committed; the tests of this file and of tests/test_gpu_optimizer_tail.py run
on each):  the ln32 backward striding by gridDim.x * blockDim.x + 1 fails test_ln32 at 131 073 and 262 145 rows in both types (the
four cases past one trip);  the ln32 forward's loop cut to a single trip fails both cases of test_ln32_forward_past_its_grid_cap;
row / groups for row % groups in the NCHW forward fails all 22 NCHW cases of test_gn8_gelu, the four NCHW cases of
test_gn8_gelu_tails_and_cancelling_residual and the NCHW wrapper case;  the norm kernel without its n & 3 line fails 65 cases of
test_optimizer_tail (at every n that is no multiple of 4: the `tail_mass` gradient always, the random ones where norm_out moves by more
than 2 ulps);  the update loop's stride halved fails 87
cases of test_optimizer_tail (every n from 1 023 up) and the three-step test."""
import ctypes as C
import os

import pytest
import torch

import _norm_opt_ref as R

pytestmark = pytest.mark.gpu

LAUNCHER_CAPS = (                          # (entry point, the literal of its launcher, what tests/_norm_opt_ref.py takes it to mean)
    ("pmx_ln32_forward", "std::min<int64_t>((rows + 255) / 256, 4096)", R.LN32_FWD_BLOCKS == 4096),
    ("pmx_ln32_backward", "const unsigned grid = PMX_LN32_PARTIAL_ROWS / 4;", R.LN32_BWD_TRIP == R.LN32_PARTIAL_ROWS // 4 * 256),
    ("pmx_gn8_gelu_forward", "if (HW <= 192) PMX_GN_FWD(float, 3); else if (HW <= 448) PMX_GN_FWD(float, 7); else PMX_GN_FWD(float, 16);", True),
    ("pmx_gn8_gelu_forward", "if (HW <= 192) PMX_GN_FWD(__hip_bfloat16, 3); else if (HW <= 448) PMX_GN_FWD(__hip_bfloat16, 7); else PMX_GN_FWD(__hip_bfloat16, 16);", True),
    ("pmx_gn8_gelu_backward", "if (HW <= 192) PMX_GN_BWD(float, 3); else if (HW <= 448) PMX_GN_BWD(float, 7); else PMX_GN_BWD(float, 16);", True),
    ("pmx_gn8_gelu_backward", "if (HW <= 192) PMX_GN_BWD(__hip_bfloat16, 3); else if (HW <= 448) PMX_GN_BWD(__hip_bfloat16, 7); else PMX_GN_BWD(__hip_bfloat16, 16);", True),
    ("pmx_gn8cl_gelu_forward", "if (HW <= 192) PMX_GNCL_FWD(3); else if (HW <= 448) PMX_GNCL_FWD(7); else PMX_GNCL_FWD(16);", True),
    ("pmx_gn8cl_gelu_backward", "if (HW <= 192) PMX_GNCL_BWD(3); else if (HW <= 448) PMX_GNCL_BWD(7); else PMX_GNCL_BWD(16);", True),
    ("pmx_gn8_gelu_forward", "HW > 1024", R.GN_HW_EDGES == (192, 448, 1024)),
    ("pmx_gn8_gelu_forward", "const unsigned grid = (unsigned)((rows + 3) / 4);", True),
    ("pmx_colsum_bf16", "dim3(PMX_COLSUM_BLOCKS), dim3(256)", True),
    ("pmx_colsum_bf16", "const int RP = 256 / (C >> 3);", R.colsum_rows_per_pass(96) == 21),
    ("pmx_clip_adam_ema_tail", "if (blocks > PMX_OPT_PARTIALS) blocks = PMX_OPT_PARTIALS;", R.OPT_NORM_TRIP == R.OPT_PARTIALS * 1024),
    ("pmx_clip_adam_ema_tail", "int64_t blocks = (n / 4 + 255) / 256;", True),
    ("pmx_clip_adam_ema_tail", "if (b2k > 2048) b2k = 2048;", R.OPT_UPDATE_TRIP == 2048 * 256),
)
CANARY, NAN_BYTE = 0xA5, 0xFF              # 0xFFFF is a bfloat16 NaN, 0xFFFFFFFF a float32 NaN
PMX_OK, PMX_ERR_INVALID = 0, -1
F32, BF16 = torch.float32, torch.bfloat16


def _libs():
    from pmx import _lib
    return _lib, _lib.load()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Arena:
    """Outputs cut out of larger buffers of canary bytes and prefilled with a NaN pattern."""
    PAD = 4096

    def __init__(self):
        self.items = []

    def __call__(self, numel, dtype):
        n = max(numel, 1) * torch.empty(0, dtype=dtype).element_size()
        buf = torch.full((self.PAD + n + self.PAD,), CANARY, dtype=torch.uint8, device="cuda")
        buf[self.PAD:self.PAD + n] = NAN_BYTE
        self.items.append((buf, n))
        return buf[self.PAD:self.PAD + n].view(dtype)

    def assert_bands_intact(self):
        torch.cuda.synchronize()
        for buf, n in self.items:
            assert bool((buf[:self.PAD] == CANARY).all()), "bytes in front of an output changed"
            assert bool((buf[self.PAD + n:] == CANARY).all()), "bytes behind an output changed"


def _nan_pattern(t):
    return bool((t.contiguous().view(torch.uint8) == NAN_BYTE).all())


def _hold(fam, tag, got, ref, scale, F, bf16_outs, fails):
    """Prints the ratio of every output in `got` and notes the ones over their bound."""
    for name, t in got.items():
        r, x = R.ratio(t, ref[name], scale[name]), R.excess(t, ref[name], scale[name], F[name], name in bf16_outs)
        print(f"NORMFIG {fam} {name} {tag} {r:.3e} F {F[name]:.3e}   of its bound {x:.3f}")
        if not x <= 1.0:
            fails.append((name, r, F[name], x))


def _controls_fail(fam, tag, ctl, fails):
    for what, x in R.worst_by_output(ctl).items():
        print(f"NORMNEG {fam} {tag} {what}: of its bound {x:.1f}")
        if not x > 1.0:
            fails.append(("passes " + what, x))


def _refused(fn, args, pointers, bad_sizes):
    """Every argument list with one pointer NULL or one size out of range returns PMX_ERR_INVALID."""
    for i in pointers:
        assert fn(*[None if j == i else a for j, a in enumerate(args)]) == PMX_ERR_INVALID, (fn.__name__, "NULL argument", i)
    for i, v in bad_sizes:
        assert fn(*[v if j == i else a for j, a in enumerate(args)]) == PMX_ERR_INVALID, (fn.__name__, "argument", i, v)


def test_launcher_caps():
    L, _ = _libs()
    with open(os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "csrc", "pmx_train.hip")) as f:
        bodies = {part.split("(", 1)[0]: part for part in f.read().split('extern "C" int ')[1:]}
    for entry, literal, meaning in LAUNCHER_CAPS:
        assert literal in bodies[entry] and meaning, (entry, literal)
    assert L.LN32_PARTIAL_ROWS == R.LN32_PARTIAL_ROWS == 2048 and L.OPT_PARTIALS == R.OPT_PARTIALS == 1024 and L.COLSUM_BLOCKS == R.COLSUM_BLOCKS == 512
    with open(os.path.join(os.path.dirname(os.path.abspath(L.__file__)), os.pardir, "include", "pmx.h")) as f:
        header = f.read()
    for define in ("#define PMX_LN32_PARTIAL_ROWS 2048", "#define PMX_OPT_PARTIALS 1024", "#define PMX_COLSUM_BLOCKS 512"):
        assert define in header, define
    assert all(t + d in R.LN32_SIZES for t in (R.LN32_BWD_TRIP,) for d in (-1, 0, 1)) and R.LN32_FWD_ONLY_ROWS > R.LN32_FWD_TRIP
    assert all(e + d in R.GN_HWS for e in R.GN_HW_EDGES[:2] for d in (0, 1)) and R.GN_HW_EDGES[2] in R.GN_HWS
    assert all(t + d in R.OPT_SIZES for t in (R.OPT_UPDATE_TRIP, R.OPT_NORM_TRIP) for d in (-1, 0, 1))


# ---------------------------------------------------------------------------------------------------------------
# ln32
# ---------------------------------------------------------------------------------------------------------------
class Ln32Run:
    def __init__(self, case, alloc):
        self.L, self.lib = _libs()
        self.d = {k: v.cuda().contiguous() for k, v in case.items() if k != "kinds"}
        self.rows, self.io = case["x"].shape[0], case["x"].dtype
        self.code = 1 if self.io == BF16 else 0
        n = max(self.rows, 1)
        self.y, self.dz = alloc(n * 32, self.io).view(n, 32), alloc(n * 32, self.io).view(n, 32)
        self.mean, self.rstd = alloc(n, F32), alloc(n, F32)
        self.partial = alloc(R.LN32_PARTIAL_ROWS * 64, F32).view(R.LN32_PARTIAL_ROWS, 64)

    def fwd_args(self, rows):
        d = self.d
        return [d["x"].data_ptr(), d["a"].data_ptr(), d["w"].data_ptr(), d["b"].data_ptr(), self.y.data_ptr(), self.mean.data_ptr(), self.rstd.data_ptr(),
                rows, R.EPS, self.code, _st()]

    def bwd_args(self, mean, rstd, rows):
        d = self.d
        return [d["x"].data_ptr(), d["a"].data_ptr(), d["dy"].data_ptr(), d["w"].data_ptr(), mean.data_ptr(), rstd.data_ptr(), self.dz.data_ptr(),
                self.partial.data_ptr(), rows, self.code, _st()]


def _ln32_tag(rows, bf16):
    return f"rows={rows}/{'bf16' if bf16 else 'f32'}"


@pytest.mark.parametrize("rows,bf16", R.ln32_cases())
def test_ln32(rows, bf16):
    """Forward and backward on the case; the backward is given the reference's statistics rounded to float32."""
    case = R.ln32_case(rows, R.ln32_seed(rows, bf16), bf16)
    ref, scale, F = R.study(lambda dt: R.ln32_ref(case, dt, "cuda"))
    arena = Arena()
    run = Ln32Run(case, arena)
    run.L.check(run.lib.pmx_ln32_forward(*run.fwd_args(rows)), "pmx_ln32_forward")
    mean32, rstd32 = ref["mean"].float().contiguous(), ref["rstd"].float().contiguous()
    run.L.check(run.lib.pmx_ln32_backward(*run.bwd_args(mean32, rstd32, rows)), "pmx_ln32_backward")
    arena.assert_bands_intact()
    fails, tag = [], _ln32_tag(rows, bf16)
    assert bool(torch.isfinite(run.partial).all()), "partial rows were left unwritten"
    got = {"y": run.y, "mean": run.mean, "rstd": run.rstd, "dz": run.dz, "dw": run.partial[:, :32].double().sum(0), "db": run.partial[:, 32:].double().sum(0)}
    _hold("ln32", tag, got, ref, scale, F, ("y", "dz") if bf16 else (), fails)
    _controls_fail("ln32", tag, R.ln32_controls(case, ref, scale, F, bf16, "cuda"), fails)
    assert not fails, (tag, fails)
    busy = min((rows + 63) // 64, R.LN32_PARTIAL_ROWS)
    assert not bool(run.partial[busy:].any()), "a wavefront without a token row wrote something else than zeros"
    for r, kind in case["kinds"].items():
        if kind in ("constant", "cancel"):                                  # x + a the same in every feature: y = b exactly
            assert torch.equal(run.y[r].float(), run.d["b"].to(run.io).float())


@pytest.mark.parametrize("bf16", [True, False])
def test_ln32_forward_past_its_grid_cap(bf16):
    """4096 * 256 + 257 rows: every lane of the capped grid takes a second row, 257 of them; the reference runs in float64 here."""
    rows = R.LN32_FWD_ONLY_ROWS
    case = R.ln32_case(rows, R.ln32_seed(rows, bf16), bf16, fwd_only=True)
    ref, scale, F = R.study(lambda dt: R.ln32_ref(case, dt, "cuda", fwd_only=True))
    arena = Arena()
    L, lib = _libs()
    d = {k: case[k].cuda() for k in ("x", "a", "w", "b")}
    y, mean, rstd = arena(rows * 32, case["x"].dtype).view(rows, 32), arena(rows, F32), arena(rows, F32)
    L.check(lib.pmx_ln32_forward(d["x"].data_ptr(), d["a"].data_ptr(), d["w"].data_ptr(), d["b"].data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                 rows, R.EPS, 1 if bf16 else 0, _st()), "pmx_ln32_forward")
    arena.assert_bands_intact()
    fails, tag = [], _ln32_tag(rows, bf16) + "/forward"
    _hold("ln32", tag, {"y": y, "mean": mean, "rstd": rstd}, ref, scale, F, ("y",) if bf16 else (), fails)
    second = {k: v.clone() for k, v in ref.items()}                          # negative control: one trip only
    for v in second.values():
        v[R.LN32_FWD_TRIP:] = 0
    ctl = [("rows past the first forward trip left out", k, R.excess(second[k], ref[k], scale[k], F[k], bf16 and k == "y")) for k in ("y", "rstd")]
    _controls_fail("ln32", tag, ctl, fails)
    assert not fails, (tag, fails)


def test_ln32_zero_rows():
    arena = Arena()
    run = Ln32Run(R.ln32_case(5, 3, True), arena)
    assert run.lib.pmx_ln32_forward(*run.fwd_args(0)) == PMX_OK
    assert run.lib.pmx_ln32_backward(*run.bwd_args(run.d["w"], run.d["w"], 0)) == PMX_OK
    arena.assert_bands_intact()
    assert _nan_pattern(run.y) and _nan_pattern(run.mean) and _nan_pattern(run.rstd) and _nan_pattern(run.dz)      # nothing written ...
    assert not bool(run.partial.view(torch.int32).any())                                                          # ... but all of partial, +0.0


@pytest.mark.parametrize("bf16", [False, True])
def test_ln32_bad_arguments_are_refused_and_nothing_is_written(bf16):
    arena = Arena()
    run = Ln32Run(R.ln32_case(5, 3, bf16), arena)
    stats = torch.ones(5, device="cuda")
    _refused(run.lib.pmx_ln32_forward, run.fwd_args(5), range(7), [(7, -1)])
    _refused(run.lib.pmx_ln32_backward, run.bwd_args(stats, stats, 5), range(8), [(8, -1)])
    arena.assert_bands_intact()
    assert all(_nan_pattern(t) for t in (run.y, run.mean, run.rstd, run.dz, run.partial))


# ---------------------------------------------------------------------------------------------------------------
# gn8: NCHW in both types, channels-last in bfloat16
# ---------------------------------------------------------------------------------------------------------------
def _to_layout(t, layout):
    """[B, C, HW] -> the bytes the kernels read: as it is, or [B, HW, C]."""
    return t.cuda().contiguous() if layout == "nchw" else t.cuda().permute(0, 2, 1).contiguous()


def _from_layout(t, layout, B, Cc, HW):
    return t.view(B, Cc, HW) if layout == "nchw" else t.view(B, HW, Cc).permute(0, 2, 1)


class Gn8Run:
    def __init__(self, case, layout, alloc):
        self.L, self.lib = _libs()
        self.layout, self.io = layout, case["h"].dtype
        self.B, self.C, self.HW = case["h"].shape
        self.groups, self.rows = self.C // 8, self.B * self.C // 8
        self.h, self.dy = _to_layout(case["h"], layout), _to_layout(case["dy"], layout)
        self.res = None if case["res"] is None else _to_layout(case["res"], layout)
        self.w, self.b = case["w"].cuda(), case["b"].cuda()
        n = self.B * self.C * self.HW
        self.y, self.dh, self.dres = alloc(n, self.io), alloc(n, self.io), alloc(n, self.io)
        self.mean, self.rstd, self.partial = alloc(self.rows, F32), alloc(self.rows, F32), alloc(self.rows * 16, F32)
        self.fwd = getattr(self.lib, "pmx_gn8_gelu_forward" if layout == "nchw" else "pmx_gn8cl_gelu_forward")
        self.bwd = getattr(self.lib, "pmx_gn8_gelu_backward" if layout == "nchw" else "pmx_gn8cl_gelu_backward")
        self.code = [1 if self.io == BF16 else 0] if layout == "nchw" else []

    def fwd_args(self, HW=None):
        rp = None if self.res is None else self.res.data_ptr()
        return [self.h.data_ptr(), rp, self.w.data_ptr(), self.b.data_ptr(), self.y.data_ptr(), self.mean.data_ptr(), self.rstd.data_ptr(), self.B, self.groups,
                self.HW if HW is None else HW, R.EPS] + self.code + [_st()]

    def bwd_args(self, mean, rstd, HW=None, res=True, dres=True):
        rp = self.res.data_ptr() if res and self.res is not None else None
        dp = self.dres.data_ptr() if dres and self.res is not None else None
        return [self.h.data_ptr(), rp, self.dy.data_ptr(), self.w.data_ptr(), self.b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), self.dh.data_ptr(), dp,
                self.partial.data_ptr(), self.B, self.groups, self.HW if HW is None else HW] + self.code + [_st()]

    def outputs(self):
        shape = (self.rows, 8, self.HW)
        got = {k: _from_layout(getattr(self, k), self.layout, self.B, self.C, self.HW).reshape(shape) for k in ("y", "dh")}
        if self.res is not None:
            got["dres"] = _from_layout(self.dres, self.layout, self.B, self.C, self.HW).reshape(shape)
        got.update(mean=self.mean, rstd=self.rstd, partial=self.partial.view(self.rows, 8, 2))
        return got


def check_gn8(layout, case, tag):
    bf16 = case["h"].dtype == BF16
    ref, scale, F = R.study(lambda dt: R.gn8_ref(case, dt, "cuda"))
    arena = Arena()
    run = Gn8Run(case, layout, arena)
    run.L.check(run.fwd(*run.fwd_args()), "gn8 forward")
    run.L.check(run.bwd(*run.bwd_args(ref["mean"].float().contiguous(), ref["rstd"].float().contiguous())), "gn8 backward")
    arena.assert_bands_intact()
    fails = []
    if case["res"] is None:
        assert _nan_pattern(run.dres)
    _hold("gn8" + layout, tag, run.outputs(), ref, scale, F, ("y", "dh", "dres") if bf16 else (), fails)
    _controls_fail("gn8" + layout, tag, R.gn8_controls(case, ref, scale, F, bf16, "cuda"), fails)
    assert not fails, (tag, fails)
    return run


@pytest.mark.parametrize("layout,bf16,HW", R.gn8_cases())
def test_gn8_gelu(layout, bf16, HW):
    for B, groups in R.GN_SHAPES:
        for with_res in (False, True):
            case = R.gn8_case(B, groups, HW, R.gn8_seed(B, groups, HW, bf16, with_res), bf16, with_res)
            check_gn8(layout, case, f"B={B}/groups={groups}/HW={HW}/{'bf16' if bf16 else 'f32'}/{'res' if with_res else 'plain'}")


@pytest.mark.parametrize("layout,bf16", [("nchw", False), ("nchw", True), ("cl", True)])
@pytest.mark.parametrize("kind", ["tails", "cancel"])
def test_gn8_gelu_tails_and_cancelling_residual(kind, layout, bf16):
    for B, groups, HW in ((5, 3, 140), (7, 4, 449)):
        case = R.gn8_case(B, groups, HW, R.gn8_seed(B, groups, HW, bf16, True) + 1, bf16, True, kind)
        check_gn8(layout, case, f"B={B}/groups={groups}/HW={HW}/{'bf16' if bf16 else 'f32'}/{kind}")


@pytest.mark.parametrize("layout,bf16", [("nchw", False), ("nchw", True), ("cl", True)])
def test_gn8_bad_arguments_are_refused_and_nothing_is_written(layout, bf16):
    arena = Arena()
    run = Gn8Run(R.gn8_case(3, 2, 20, 1, bf16, True), layout, arena)
    stats = torch.ones(run.rows, device="cuda")
    _refused(run.fwd, run.fwd_args(), (0, 2, 3, 4, 5, 6), [(9, 1025), (9, 0), (9, -1), (8, 0), (7, -1)])
    _refused(run.bwd, run.bwd_args(stats, stats), (0, 2, 3, 4, 5, 6, 7, 9), [(12, 1025), (12, 0), (11, 0), (10, -1)])
    assert run.bwd(*run.bwd_args(stats, stats, dres=False)) == PMX_ERR_INVALID          # res without dres
    assert run.bwd(*run.bwd_args(stats, stats, res=False)) == PMX_ERR_INVALID           # dres without res
    arena.assert_bands_intact()
    assert all(_nan_pattern(t) for t in (run.y, run.dh, run.dres, run.mean, run.rstd, run.partial))
    assert run.fwd(*[0 if j == 7 else a for j, a in enumerate(run.fwd_args())]) == PMX_OK       # B == 0: nothing to do
    assert run.bwd(*[0 if j == 10 else a for j, a in enumerate(run.bwd_args(stats, stats))]) == PMX_OK
    arena.assert_bands_intact()
    assert all(_nan_pattern(t) for t in (run.y, run.dh, run.dres, run.mean, run.rstd, run.partial))


@pytest.mark.parametrize("channels_last", [True, False])
def test_group_norm_gelu_wrapper_picks_the_layout_and_sums_the_partials(channels_last):
    """actor_tower.group_norm_gelu on 5 samples of 24 channels (groups = 3, 15 rows: the last block is partly filled): a channels-last
    bfloat16 input goes to the NHWC kernels, an NCHW float32 one to the NCHW kernels; the weight gradients are partial.sum(0)."""
    from pmx import actor_tower
    B, groups, H, W = 5, 3, 7, 10
    bf16 = channels_last
    case = R.gn8_case(B, groups, H * W, 77, bf16, True)
    ref, scale, F = R.study(lambda dt: R.gn8_ref(case, dt, "cuda", stats32=True))
    gn = torch.nn.GroupNorm(groups, groups * 8, eps=R.EPS).cuda()
    with torch.no_grad():
        gn.weight.copy_(case["w"]); gn.bias.copy_(case["b"])
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    h, res, dy = (case[k].cuda().view(B, groups * 8, H, W).contiguous(memory_format=fmt) for k in ("h", "res", "dy"))
    h.requires_grad_(True); res.requires_grad_(True)
    y = actor_tower.group_norm_gelu(h, res, gn)
    assert type(y.grad_fn).__name__.startswith("_GN8Gelu") and y.grad_fn.cl == channels_last
    dh, dres, dw, db = torch.autograd.grad(y, (h, res, gn.weight, gn.bias), dy)
    shape = (B * groups, 8, H * W)
    got = {"y": y.detach().reshape(B, groups * 8, -1).reshape(shape), "dh": dh.reshape(B, groups * 8, -1).reshape(shape),
           "dres": dres.reshape(B, groups * 8, -1).reshape(shape)}
    fails, tag = [], f"wrapper/{'cl-bf16' if channels_last else 'nchw-f32'}"
    _hold("gn8", tag, got, ref, scale, F, ("y", "dh", "dres") if bf16 else (), fails)
    # the weight gradients: the partials of the B samples added; held against the float64 sum with the sum of the partials' scales
    wsum, wscale = ref["partial"].view(B, groups * 8, 2).sum(0), scale["partial"].view(B, groups * 8, 2).sum(0)
    for name, t, k in (("dw", dw, 0), ("db", db, 1)):
        x = R.excess(t, wsum[:, k], wscale[:, k], F["partial"])
        print(f"NORMFIG gn8 {name} {tag} of its bound {x:.3f}")
        if not x <= 1.0:
            fails.append((name, x))
    assert not fails, (tag, fails)


# ---------------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", R.COLSUM_CS)
def test_colsum_bf16(Cc):
    L, lib = _libs()
    for rows in R.colsum_sizes(Cc):
        x = R.colsum_case(rows, Cc, 17 * rows + Cc)
        ref, scale, F = R.study(lambda dt: R.colsum_ref(x.cuda(), dt))
        arena = Arena()
        xd = x.cuda() if rows else torch.zeros(1, Cc, dtype=BF16, device="cuda")
        partial = arena(R.COLSUM_BLOCKS * Cc, F32).view(R.COLSUM_BLOCKS, Cc)
        L.check(lib.pmx_colsum_bf16(xd.data_ptr(), rows, Cc, partial.data_ptr(), _st()), "pmx_colsum_bf16")
        arena.assert_bands_intact()
        assert bool(torch.isfinite(partial).all()), "partial rows were left unwritten"
        fails, tag = [], f"rows={rows}/C={Cc}"
        _hold("colsum", tag, {"colsum": partial.double().sum(0)}, ref, scale, F, (), fails)
        if rows:                                               # negative control: the last row left out, held per column
            short = R.colsum_ref(x[:-1].cuda(), torch.float64)[0]["colsum"]
            _controls_fail("colsum", tag, [("last row left out", "colsum", R.excess(short, ref["colsum"], scale["colsum"], F["colsum"]))], fails)
        else:
            assert not bool(partial.any())
        assert not fails, (tag, fails)
        busy = (rows + R.colsum_rows_per_pass(Cc) - 1) // R.colsum_rows_per_pass(Cc)
        assert not bool(partial[busy:].any())                  # blocks without a row write zeros


def test_colsum_bad_arguments_are_refused_and_nothing_is_written():
    _, lib = _libs()
    arena = Arena()
    x = torch.ones(16, 264, dtype=BF16, device="cuda")
    partial = arena(R.COLSUM_BLOCKS * 264, F32)
    for Cc in (4, 12, 264, 0, -8):
        assert lib.pmx_colsum_bf16(x.data_ptr(), 16, Cc, partial.data_ptr(), _st()) == PMX_ERR_INVALID, Cc
    assert lib.pmx_colsum_bf16(None, 16, 8, partial.data_ptr(), _st()) == PMX_ERR_INVALID
    assert lib.pmx_colsum_bf16(x.data_ptr(), 16, 8, None, _st()) == PMX_ERR_INVALID
    assert lib.pmx_colsum_bf16(x.data_ptr(), -1, 8, partial.data_ptr(), _st()) == PMX_ERR_INVALID
    arena.assert_bands_intact()
    assert _nan_pattern(partial)
