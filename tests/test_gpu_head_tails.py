"""The head-tail kernels (csrc/pmx_heads.hip: pmx_actor_tail_forward / _backward, pmx_critic_tail_forward / _backward with the
weight-gradient kernel) through the C ABI, against the rounding-mirrored float64 references of tests/_tails_ref.py: per ELEMENT and
per SAMPLE, at the batch sizes where the grids saturate and the grid-stride loops take a second and a ragged last trip, where the
weight-gradient kernel changes its chunking, on rows that break a careless LayerNorm, GELU or token sum, in both IO types, with
NaN-prefilled outputs between canary bands.

Grid caps of the launchers.  A block is 4 waves, a wave takes one sample per trip.  test_launcher_caps_are_the_tables_of_this_file
looks the literals up in the source, so that a change of a launcher fails here instead of silently moving the edges.
    launcher                     blocks at most                        samples per trip   csrc/pmx_heads.hip
    pmx_actor_tail_forward       1024                                  4096               line 384  heads_blocks(B, 1024)
    pmx_actor_tail_backward      PMX_HEADS_PARTIAL_ROWS (128)          512                line 398  heads_blocks(B, PMX_HEADS_PARTIAL_ROWS)
    pmx_critic_tail_forward      512                                   2048               line 413  heads_blocks(B, 512)
    pmx_critic_tail_backward     512                                   2048               line 430  heads_blocks(B, 512)
    its weight-gradient kernel   chunks of 16 samples, of ceil(B / PMX_HEADS_PARTIAL_ROWS) above 16 * 128      lines 433-434

Bounds (tests/_tails_ref.py `bounds`; none is taken from the kernels' output).  bfloat16 outputs (actor dh in bfloat16 mode,
critic dtokens): |got - ref| <= 2 * 2**-8 * max|ref| of THAT SAMPLE's row; a row whose reference is all zero must be exactly zero.
float32 outputs: |got - ref| <= F * max|ref| of the tensor (parameter gradients, value) or of the sample's row (logits, stats, rstd,
actor dh in float32 mode), F = 4 x the ratio the float32 run of the reference reaches against the float64 run on the same case,
at least 16 * 2**-24, computed at test time per case and output.  Widened, with the cause: the outputs behind a bf16(gelu(z)),
bf16(pre) or bf16(dh) rounding (actor logits, dw2; critic value, dw1, db1, dw2) are allowed, per element on top of F * scale, what
four such roundings that fall the other way can move them by (`_slack` and `excess` in tests/_tails_ref.py: one bfloat16 step of the
rounded quantity times the factor it meets, at the worst summand).  Such flips are discrete events of one bfloat16 step each, and
whether the float32 run of the reference meets one is luck: at B = 512 it met none (F = 2.9e-5) where the actor kernel's logits
met one (2.0e-4 of the row); at B = 2 047 likewise for the critic's value and dw2.  The bias gradients are sums that may cancel to
anything, so their scale is their largest summand if that is larger (critic db2 at B = 16: 1.5e-6 of a sum of 0.3).  `value` has
one entry per sample, which may be as close to zero as it likes, so its scale is the tensor's; `rstd` is held on its own besides
`stats`, where a large mean would hide it.  pooled:
every element a bfloat16 value within one step of the reference; value is then held against the reference evaluated on the
kernel's own pooled tokens, and the backward entry point is given the reference's.  Every case also requires that the negative
controls of the reference (last sample zeroed / dropped, last ragged trip dropped) FAIL these bounds.

Measured on an MI355X (`TAILFIG` lines of every case of this file; information, not the source of any bound: the worst ratio
|got - ref| / scale per output, the case that gave it, that case's F):
    actor    logits 1.701e-3 (B = 1 027, F 6.8e-3)     stats 1.514e-7, rstd 2.059e-7 (outlier rows, B = 4 097, F at its floor 9.5e-7)
             dh bfloat16 7.194e-3 = 1.84 x 2**-8 (B = 4 095; bound 2 x 2**-8)     dh float32 3.632e-7 (B = 8 195, F 1.5e-6)
             dw2 3.259e-4 (B = 1 027, F 1.3e-3)    db2 3.424e-7 (B = 4 097)    dlnw 2.020e-7 (B = 4 096)    dlnb 2.814e-7 (B = 4 097, F 1.1e-6)
    far_offset rows (float32 only; F follows the float32 run, no table of their own is needed): logits 4.135e-3 (F 1.6e-2),
             dh 1.198e-4 (F 1.4e-3), dw2 5.566e-4, dlnw 1.933e-5 (F 1.1e-4), dlnb 1.651e-5 (F 1.1e-4), rstd 1.272e-7
    critic   value 1.400e-4 (B = 4 099, F 5.6e-4)     dtokens 3.546e-3 = 0.91 x 2**-8 (B = 2 049)     dw1 2.130e-4, db1 1.107e-4, dw2 5.907e-5
             (constant tokens, B = 2 049, F 8.5e-4, 4.4e-4, 2.4e-4)     db2 1.307e-6 (B = 2 048, F 3.1e-6)
    The logits, dw2 and the critic's value, dw1, db1, dw2 sit at F / 4 exactly on their worst cases: the kernels and the float32 run
    of the reference flip the same roundings there.  No output used more than 0.45 of its bound except the actor's bfloat16 dh
    (0.92: one element rounded to the other neighbour where it is the row's largest and just above a power of two).
    pooled: always within one bfloat16 step; the share of elements that differ from the reference is 0.65 to 0.72 % at S = 7 from
             2 047 samples up (0.34 % where every other sample has constant or cancelling tokens), 1.25 % at worst on the 5-sample
             cases (S = 7 cancelling, S = 15), none at S = 1, 16, 17, 154, 400, 1 024: these are exact ties, sum / S on the midpoint
             of two bfloat16 values, which the kernel's float32 sum * (1 / S) leaves to one side.
    negative controls: none passes; tests/test_tails_ref_cpu.py holds each to a threefold miss at least (the smallest is 6.8).
    kinds restricted to the edge size: the critic's `large` tokens (CRITIC_KIND_SIZES_OF in tests/_tails_ref.py).

Mutation check (scratch copies, not committed): the actor backward striding by gridDim.x * 4 + 1 fails test_actor_tail at every
size from 513 up, test_actor_deferred_row_sums[1027] and the actor wrapper test; the weight-gradient kernel without its remainder
loop fails test_critic_tail at every B that is no multiple of 4 inside a chunk (1, 3, 5, 15, 17, 19, 2 047, 2 049, 4 099, all S
and kinds), two deferred cases and the critic wrapper test; pooled written unrounded fails every test_critic_tail case with S > 1
that has a pooled element off the bfloat16 grid and all three deferred cases."""
import ctypes as C
import math
import os

import pytest
import torch

import _tails_ref as R

pytestmark = pytest.mark.gpu

LAUNCHER_CAPS = (                          # (entry point, the literal of its launcher, what this file takes it to mean)
    ("pmx_actor_tail_forward", "heads_blocks(B, 1024)", R.ACTOR_FWD_BLOCKS == 1024),
    ("pmx_actor_tail_backward", "heads_blocks(B, PMX_HEADS_PARTIAL_ROWS)", True),
    ("pmx_critic_tail_forward", "heads_blocks(B, 512)", R.CRITIC_BLOCKS == 512),
    ("pmx_critic_tail_backward", "heads_blocks(B, 512)", R.CRITIC_BLOCKS == 512),
    ("pmx_critic_tail_backward", "int64_t chunk = 16;", R.WGRAD_CHUNK == 16),
    ("pmx_critic_tail_backward", "if ((B + chunk - 1) / chunk > PMX_HEADS_PARTIAL_ROWS) chunk = (B + PMX_HEADS_PARTIAL_ROWS - 1) / PMX_HEADS_PARTIAL_ROWS;", True),
)
ACTOR_SLICES = {"dw2": (0, (5, 512)), "db2": (2560, (5,)), "dlnw": (2568, (512,)), "dlnb": (3080, (512,))}
ACTOR_UNUSED = (2565, 2568)                # the 3 floats after db2
CRITIC_SLICES = {"dw1": (0, (512, 32)), "db1": (16384, (512,)), "dw2": (16896, (512,)), "db2": (17408, (1,))}
CRITIC_UNUSED = (17409, 17416)             # the 7 floats after db2
CANARY, NAN_BYTE = 0xA5, 0xFF              # 0xFFFF is a bfloat16 NaN, 0xFFFFFFFF a float32 NaN
PMX_OK, PMX_ERR_INVALID = 0, -1


def _libs():
    from pmx import _lib
    return _lib, _lib.load()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rows_cap():
    return _libs()[0].HEADS_PARTIAL_ROWS


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
        torch.cuda.synchronize()
        for buf, n in self.items:
            assert bool((buf[:self.PAD] == CANARY).all()), "bytes in front of an output changed"
            assert bool((buf[self.PAD + n:] == CANARY).all()), "bytes behind an output changed"


def _nan_pattern(t):
    return bool((t.contiguous().view(torch.uint8) == NAN_BYTE).all())


def _param_grads(slices, row0):
    return {name: row0[off:off + math.prod(shape)].view(shape) for name, (off, shape) in slices.items()}


class ActorRun:
    """The actor tail on one case through the C ABI; every output comes from `alloc`."""

    def __init__(self, case, alloc):
        self.L, self.lib = _libs()
        self.alloc = alloc
        self.d = {k: v.cuda().contiguous() for k, v in case.items()}
        self.B, self.bf = case["h"].shape[0], case["h"].dtype == torch.bfloat16

    def fwd_args(self, logits, stats, B):
        d = self.d
        return [d["h"].data_ptr(), 1 if self.bf else 0, d["lnw"].data_ptr(), d["lnb"].data_ptr(), d["w2"].data_ptr(), d["b2"].data_ptr(),
                logits.data_ptr(), None if stats is None else stats.data_ptr(), B, R.EPS, _st()]

    def bwd_args(self, stats, dh, grad, B):
        d = self.d
        return [d["h"].data_ptr(), 1 if self.bf else 0, stats.data_ptr(), d["dlogits"].data_ptr(), d["lnw"].data_ptr(), d["lnb"].data_ptr(),
                d["w2"].data_ptr(), dh.data_ptr(), grad.data_ptr(), B, _st()]

    def outputs(self):
        n = max(self.B, 1)
        return (self.alloc(n * R.NACT, torch.float32).view(n, R.NACT), self.alloc(n * 2, torch.float32).view(n, 2),
                self.alloc(n * R.HID, self.d["h"].dtype).view(n, R.HID),
                self.alloc((1 + _rows_cap()) * self.L.ACTOR_TAIL_GRAD_FLOATS, torch.float32).view(1 + _rows_cap(), -1))

    def forward(self, with_stats=True, B=None):
        logits, stats, _, _ = self.outputs()
        self.L.check(self.lib.pmx_actor_tail_forward(*self.fwd_args(logits, stats if with_stats else None, self.B if B is None else B)),
                     "pmx_actor_tail_forward")
        return logits, stats

    def backward(self, stats, B=None):
        """-> (dh, the whole gradient buffer [1 + PMX_HEADS_PARTIAL_ROWS][floats], pmx_last_partial_rows())"""
        _, _, dh, grad = self.outputs()
        self.L.check(self.lib.pmx_actor_tail_backward(*self.bwd_args(stats, dh, grad, self.B if B is None else B)), "pmx_actor_tail_backward")
        return dh, grad, self.lib.pmx_last_partial_rows()


class CriticRun:
    """The critic tail on one case through the C ABI."""

    def __init__(self, case, alloc):
        self.L, self.lib = _libs()
        self.alloc = alloc
        self.d = {k: v.cuda().contiguous() for k, v in case.items()}
        self.B, self.S = case["tokens"].shape[:2]

    def fwd_args(self, value, pooled, B, S):
        d = self.d
        return [d["tokens"].data_ptr(), d["w1"].data_ptr(), d["b1"].data_ptr(), d["w2"].data_ptr(), d["b2"].data_ptr(), value.data_ptr(),
                pooled.data_ptr(), B, S, _st()]

    def bwd_args(self, pooled, dtok, scratch, grad, B, S):
        d = self.d
        return [pooled.data_ptr(), d["dvalue"].data_ptr(), d["w1"].data_ptr(), d["b1"].data_ptr(), d["w2"].data_ptr(), dtok.data_ptr(),
                scratch.data_ptr(), grad.data_ptr(), B, S, _st()]

    def outputs(self):
        n = max(self.B, 1)
        return (self.alloc(n, torch.float32), self.alloc(n * R.DM, torch.float32).view(n, R.DM),
                self.alloc(n * self.S * R.DM, torch.bfloat16).view(n, self.S, R.DM), self.alloc(2 * n * R.HID, torch.bfloat16),
                self.alloc((1 + _rows_cap()) * self.L.CRITIC_TAIL_GRAD_FLOATS, torch.float32).view(1 + _rows_cap(), -1))

    def forward(self, B=None):
        value, pooled, _, _, _ = self.outputs()
        self.L.check(self.lib.pmx_critic_tail_forward(*self.fwd_args(value, pooled, self.B if B is None else B, self.S)), "pmx_critic_tail_forward")
        return value, pooled

    def backward(self, pooled, B=None):
        """-> (dtokens, scratch, the whole gradient buffer, pmx_last_partial_rows())"""
        _, _, dtok, scratch, grad = self.outputs()
        self.L.check(self.lib.pmx_critic_tail_backward(*self.bwd_args(pooled, dtok, scratch, grad, self.B if B is None else B, self.S)),
                     "pmx_critic_tail_backward")
        return dtok, scratch, grad, self.lib.pmx_last_partial_rows()


def _hold(fam, tag, got, ref, bnd, outs, fails):
    """Prints the ratio of every output in `got` and notes the ones over their bound."""
    for name, t in got.items():
        r, x = R.ratio(t, ref, name, outs[name]), R.excess(t, ref, name, outs[name], bnd[name])
        print(f"TAILFIG {fam} {name} {tag} {r:.3e} {bnd[name]:.3e}   of its bound {x:.3f}")
        if not x <= 1.0:
            fails.append((name, r, bnd[name], x))


def _controls_fail(fam, tag, bnd, ctl, fails):
    for what, name, x in ctl:
        print(f"TAILNEG {fam} {name} {tag} {what}: of its bound {x:.1f}")
        if not x > 1.0:
            fails.append((name + ": passes " + what, x, bnd[name]))


def _actor_tag(B, kind, dl_kind, io_bf16):
    return f"B={B}/{kind}/{dl_kind}/{'bf16' if io_bf16 else 'f32'}"


def check_actor(B, kind="normal", dl_kind="normal", io_bf16=True):
    """Both directions of the actor tail on the case, every output held to its bound, negative controls included; every figure is
    printed before anything is asserted.  -> (run, outputs, reference, bounds)"""
    case = R.actor_case(B, R.actor_seed(B, kind, dl_kind, io_bf16), kind, dl_kind, io_bf16)
    tag, outs = _actor_tag(B, kind, dl_kind, io_bf16), R.actor_outs(io_bf16)
    ref, bnd, ctl = R.actor_study(case, 4 * _rows_cap(), "cuda")
    arena = Arena()
    run = ActorRun(case, arena)
    logits, stats = run.forward()
    bare, unused = run.forward(with_stats=False)
    dh, grad, rows = run.backward(ref["stats"].float().contiguous())          # the statistics are an input of the backward
    arena.assert_bands_intact()
    fails = []
    got = {"logits": logits, "stats": stats, "rstd": stats[:, 1], "dh": dh, **_param_grads(ACTOR_SLICES, grad[0])}
    _hold("actor", tag, got, ref, bnd, outs, fails)
    _controls_fail("actor", tag, bnd, ctl, fails)
    assert not fails, (tag, fails)
    assert torch.equal(bare.view(torch.int32), logits.view(torch.int32)) and _nan_pattern(unused)       # stats_dev == NULL: the same logits
    assert rows == R.heads_blocks(B, _rows_cap())
    assert bool(torch.isfinite(grad[:1 + rows]).all()) and _nan_pattern(grad[1 + rows:])                 # rows no block owns stay untouched
    assert not bool(grad[:1 + rows, ACTOR_UNUSED[0]:ACTOR_UNUSED[1]].any())
    if dl_kind == "quarter_zero":
        assert not bool(dh[R.zero_sample_mask(B).cuda()].any())
    got["grad"], got["rows"] = grad, rows
    return run, got, ref, bnd


def _critic_tag(B, S, kind, dv_kind):
    return f"B={B}/S={S}/{kind}/{dv_kind}"


def check_critic(B, S, kind="normal", dv_kind="normal"):
    """The same for the critic tail: the pool on its own, value against the reference on the kernel's pooled tokens, the backward on
    the reference's.  -> (run, outputs, reference, bounds)"""
    case = R.critic_case(B, S, R.critic_seed(B, S, kind, dv_kind), kind, dv_kind)
    tag, outs = _critic_tag(B, S, kind, dv_kind), R.critic_outs()
    ref, bnd, ctl = R.critic_study(case, 4 * R.CRITIC_BLOCKS, "cuda")
    arena = Arena()
    run = CriticRun(case, arena)
    value, pooled = run.forward()
    dtok, scratch, grad, rows = run.backward(ref["pooled"].float().contiguous())
    arena.assert_bands_intact()
    fails = []
    # the pool
    steps = R.bf16_steps_apart(pooled, ref["pooled"])
    share = float((pooled.double() != ref["pooled"]).double().mean())
    print(f"TAILFIG critic pooled_flip_share {tag} {share:.3e} {float(steps.max()):.3f}")
    if not bool(torch.isfinite(pooled).all()) or not torch.equal(pooled.to(torch.bfloat16).float(), pooled):
        fails.append("pooled holds values that are no bfloat16")
    if not float(steps.max()) <= 1.0:
        fails.append(("pooled", float(steps.max()), "bfloat16 steps"))
    if not float(R.bf16_steps_apart(R.zero_last(ref["pooled"]), ref["pooled"]).max()) > 1.0:
        fails.append("pooled: passes last sample zeroed")
    # value, downstream of the kernel's own pool
    ref_k, bnd_k, _ = R.critic_study(case, 4 * R.CRITIC_BLOCKS, "cuda", pooled=pooled)
    _hold("critic", tag, {"value": value}, ref_k, bnd_k, outs, fails)
    got = {"dtokens": dtok, **_param_grads(CRITIC_SLICES, grad[0])}
    _hold("critic", tag, got, ref, bnd, outs, fails)
    _controls_fail("critic", tag, bnd, ctl, fails)
    assert not fails, (tag, fails)
    chunk, n_chunks = R.wgrad_chunks(B, _rows_cap())
    assert rows == (n_chunks if n_chunks > 1 else 0)
    assert bool(torch.isfinite(grad[:1 + rows]).all()) and _nan_pattern(grad[1 + rows:])
    assert not bool(grad[:1 + rows, CRITIC_UNUSED[0]:CRITIC_UNUSED[1]].any())
    assert bool(torch.isfinite(scratch).all())                                                          # dh and g of every sample were written
    if dv_kind == "quarter_zero":
        assert not bool(dtok[R.zero_sample_mask(B).cuda()].any())
    got.update(value=value, pooled=pooled, grad=grad, rows=rows)
    return run, got, ref, bnd


# ---------------------------------------------------------------------------------------------------------------
# every size edge, both IO types, every row kind at an edge size and a looped one
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,kind,dl_kind,io_bf16", R.actor_cases())
def test_actor_tail(B, kind, dl_kind, io_bf16):
    check_actor(B, kind, dl_kind, io_bf16)


@pytest.mark.parametrize("B,S,kind,dv_kind", R.critic_cases())
def test_critic_tail(B, S, kind, dv_kind):
    check_critic(B, S, kind, dv_kind)


def test_launcher_caps_are_the_tables_of_this_file():
    L, _ = _libs()
    with open(os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "csrc", "pmx_heads.hip")) as f:
        bodies = {part.split("(", 1)[0]: part for part in f.read().split('extern "C" int ')[1:]}
    for entry, literal, meaning in LAUNCHER_CAPS:
        assert literal in bodies[entry] and meaning, (entry, literal)
    assert L.HEADS_PARTIAL_ROWS == 128 and L.ACTOR_TAIL_GRAD_FLOATS == 3592 and L.CRITIC_TAIL_GRAD_FLOATS == 17416
    assert 4 * R.ACTOR_FWD_BLOCKS in R.ACTOR_SIZES and 4 * L.HEADS_PARTIAL_ROWS in R.ACTOR_SIZES and 4 * R.CRITIC_BLOCKS in R.CRITIC_SIZES
    assert R.WGRAD_CHUNK * L.HEADS_PARTIAL_ROWS in R.CRITIC_SIZES and R.WGRAD_CHUNK in R.CRITIC_SIZES


# ---------------------------------------------------------------------------------------------------------------
# B == 0, argument checks
# ---------------------------------------------------------------------------------------------------------------
def test_zero_samples():
    arena = Arena()
    run = ActorRun(R.actor_case(5, 3), arena)
    logits, stats = run.forward(B=0)                            # returns OK ...
    dh, grad, n = run.backward(stats, B=0)
    arena.assert_bands_intact()
    assert _nan_pattern(logits) and _nan_pattern(stats) and _nan_pattern(dh)        # ... and writes nothing
    assert n == 0 and not bool(grad[0].any()) and _nan_pattern(grad[1:])            # backward: row 0 zeroed, no partial rows
    run = CriticRun(R.critic_case(5, 7, 3), arena)
    value, pooled = run.forward(B=0)
    dtok, scratch, grad, n = run.backward(pooled, B=0)
    arena.assert_bands_intact()
    assert _nan_pattern(value) and _nan_pattern(pooled) and _nan_pattern(dtok) and _nan_pattern(scratch)
    assert n == 0 and not bool(grad[0].any()) and _nan_pattern(grad[1:])


def _refused(fn, args, pointers, bad_sizes):
    """Every argument list with one pointer NULL or one size out of range returns PMX_ERR_INVALID."""
    for i in pointers:
        assert fn(*[None if j == i else a for j, a in enumerate(args)]) == PMX_ERR_INVALID, (fn.__name__, "NULL argument", i)
    for i, v in bad_sizes:
        assert fn(*[v if j == i else a for j, a in enumerate(args)]) == PMX_ERR_INVALID, (fn.__name__, "argument", i, v)


def test_bad_arguments_are_refused_and_nothing_is_written():
    arena = Arena()
    run = ActorRun(R.actor_case(5, 3), arena)
    logits, stats, dh, grad = run.outputs()
    ref_stats = torch.zeros(5, 2, device="cuda")
    _refused(run.lib.pmx_actor_tail_forward, run.fwd_args(logits, stats, 5), (0, 2, 3, 4, 5, 6), [(8, -1)])      # (7, stats, may be NULL)
    _refused(run.lib.pmx_actor_tail_backward, run.bwd_args(ref_stats, dh, grad, 5), (0, 2, 3, 4, 5, 6, 7, 8), [(9, -1)])
    arena.assert_bands_intact()
    assert all(_nan_pattern(t) for t in (logits, stats, dh, grad))
    crun = CriticRun(R.critic_case(5, 7, 3), arena)
    value, pooled, dtok, scratch, grad = crun.outputs()
    ref_pooled = torch.zeros(5, 32, device="cuda")
    _refused(crun.lib.pmx_critic_tail_forward, crun.fwd_args(value, pooled, 5, 7), (0, 1, 2, 3, 4, 5, 6), [(7, -1), (8, 0), (8, -3)])
    _refused(crun.lib.pmx_critic_tail_backward, crun.bwd_args(ref_pooled, dtok, scratch, grad, 5, 7), (0, 1, 2, 3, 4, 5, 6, 7), [(8, -1), (9, 0), (9, -3)])
    arena.assert_bands_intact()
    assert all(_nan_pattern(t) for t in (value, pooled, dtok, scratch, grad))


# ---------------------------------------------------------------------------------------------------------------
# deferred row sums
# ---------------------------------------------------------------------------------------------------------------
def _deferred(lib, backward):
    lib.pmx_defer_row_sums(1)
    try:
        return backward()
    finally:
        lib.pmx_defer_row_sums(0)


def _check_deferred(fam, tag, lib, L, plain, grad, n, floats, slices, ref, bnd):
    """grad: the buffer of a deferred backward with n partial rows; plain: that of the undeferred one."""
    assert lib.pmx_last_partial_rows() == n
    if n == 0:                                                   # one chunk: the sums went straight to row 0, deferred or not
        assert torch.equal(grad[0].view(torch.int32), plain[0].view(torch.int32)) and _nan_pattern(grad[1:])
        return
    assert _nan_pattern(grad[0]) and _nan_pattern(grad[1 + n:])                                   # row 0 keeps its prefill
    assert torch.equal(grad[1:1 + n].view(torch.int32), plain[1:1 + n].view(torch.int32))
    fails = []
    _hold(fam, tag + "/rows-1..n", _param_grads(slices, grad[1:1 + n].double().sum(0)), ref, bnd, {k: "tensor" for k in slices}, fails)
    assert not fails, (tag, fails)
    L.check(lib.pmx_sum_partial_rows(grad.data_ptr(), n, floats, _st()), "pmx_sum_partial_rows")
    assert torch.equal(grad[0].view(torch.int32), plain[0].view(torch.int32))                     # bit for bit the undeferred sums
    assert _nan_pattern(grad[1 + n:])


@pytest.mark.parametrize("B", [5, 1027])
def test_actor_deferred_row_sums(B):
    run, got, ref, bnd = check_actor(B)
    stats = ref["stats"].float().contiguous()
    _, grad, n = _deferred(run.lib, lambda: run.backward(stats))
    assert n == got["rows"] == R.heads_blocks(B, _rows_cap())
    _check_deferred("actor", _actor_tag(B, "normal", "normal", True), run.lib, run.L, got["grad"], grad, n, run.L.ACTOR_TAIL_GRAD_FLOATS, ACTOR_SLICES, ref, bnd)
    run.alloc.assert_bands_intact()


@pytest.mark.parametrize("B", [16, 19, 2049])
def test_critic_deferred_row_sums(B):
    run, got, ref, bnd = check_critic(B, R.CRITIC_S)
    pooled = ref["pooled"].float().contiguous()
    _, _, grad, n = _deferred(run.lib, lambda: run.backward(pooled))
    assert n == got["rows"] == {16: 0, 19: 2, 2049: 121}[B]
    _check_deferred("critic", _critic_tag(B, R.CRITIC_S, "normal", "normal"), run.lib, run.L, got["grad"], grad, n, run.L.CRITIC_TAIL_GRAD_FLOATS, CRITIC_SLICES,
                    ref, bnd)
    run.alloc.assert_bands_intact()


# ---------------------------------------------------------------------------------------------------------------
# the autograd wrappers in the looped regime: the buffers THEY allocate
# ---------------------------------------------------------------------------------------------------------------
def test_actor_tail_wrapper_in_the_looped_regime():
    from pmx import actor_head
    B = 1027
    case = R.actor_case(B, R.actor_seed(B))
    ref, bnd, _ = R.actor_study(case, 4 * _rows_cap(), "cuda")
    d = {k: v.cuda() for k, v in case.items()}
    leaves = [d[k].requires_grad_(True) for k in ("h", "lnw", "lnb", "w2", "b2")]
    logits = actor_head._ActorTail.apply(*leaves, R.EPS)
    got = dict(zip(("dh", "dlnw", "dlnb", "dw2", "db2"), torch.autograd.grad(logits, leaves, d["dlogits"])))
    got["logits"] = logits.detach()
    fails = []
    _hold("actor", _actor_tag(B, "normal", "normal", True) + "/wrapper", got, ref, bnd, R.actor_outs(True), fails)
    assert not fails, fails
    assert all(got[k].shape == ref[k].shape for k in got)


def test_critic_tail_wrapper_in_the_looped_regime():
    from pmx import critic_kernels
    B, S = 2049, R.CRITIC_S
    case = R.critic_case(B, S, R.critic_seed(B, S))
    d = {k: v.cuda() for k, v in case.items()}
    d["w2"] = d["w2"].view(1, R.HID)
    leaves = [d[k].requires_grad_(True) for k in ("tokens", "w1", "b1", "w2", "b2")]
    value = critic_kernels._CriticTail.apply(*leaves)
    pooled = value.grad_fn.saved_tensors[0]
    assert pooled.shape == (B, R.DM) and float(R.bf16_steps_apart(pooled, R.critic_ref_of(case, "cuda")["pooled"]).max()) <= 1.0
    ref, bnd, _ = R.critic_study(case, 4 * R.CRITIC_BLOCKS, "cuda", pooled=pooled)            # the wrapper's backward starts from ITS pooled tokens
    got = dict(zip(("dtokens", "dw1", "db1", "dw2", "db2"), torch.autograd.grad(value, leaves, d["dvalue"])))
    assert got["dw2"].shape == (1, R.HID)
    got["dw2"], got["value"] = got["dw2"].view(R.HID), value.detach()
    fails = []
    _hold("critic", _critic_tag(B, S, "normal", "normal") + "/wrapper", got, ref, bnd, R.critic_outs(), fails)
    assert not fails, fails
    assert all(got[k].shape == ref[k].shape for k in got)
