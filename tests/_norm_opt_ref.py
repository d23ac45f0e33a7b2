"""References, bounds, cases and negative controls for the norm kernels and the optimizer tail of csrc/pmx_train.hip
(pmx_ln32_*, pmx_gn8_gelu_*, pmx_gn8cl_gelu_*, pmx_colsum_bf16, pmx_clip_adam_ema / _tail).  Plain torch, device-agnostic: the small
cases run on the CPU (tests/test_norm_opt_ref_cpu.py), the large ones in float64 on the GPU beside the kernels.

Every reference takes the `dtype` of its arithmetic.  float64 is THE reference; the float32 run of the same function on the same
case is what the bounds are derived from (`study`): F = 4 x the ratio the float32 run reaches against the float64 run, per case and
output, and at least FLOOR = 16 * 2**-24.  The sums the kernels form per lane and across a wavefront (`lane_sum`) are formed in that
order here too, so that the float32 run meets the rounding of a sequential float32 sum, not that of torch's pairwise one.

A reference returns (outputs, scales): |got - ref64| <= F * scale is asked of every entry (`excess`), plus one bfloat16 step of the
entry itself where the kernel stores bfloat16.  The scale of y, dz, dh, dres is the largest |ref64| of the entry's row; of rstd, and
of every line of the optimizer with one product only, the value itself; of every sum that may cancel (dw, db, the GroupNorm
partials, the column sums, the lines of the optimizer that add) the sum of the magnitudes of its summands.  `mean` is such a sum too
(sum(z) / n cancels to anything on centred rows, where its float32 error stays that of the summands), so its scale is
sum|z| / n >= |mean|, not the value itself.  A scale of zero asks for an exact zero."""
import math

import torch

EPS = float(torch.tensor(1e-5, dtype=torch.float32))        # the entry points take eps as a float32
FLOOR = 16 * 2.0 ** -24
BF16_STEP = 2.0 ** -8               # round to nearest even moves a value by at most 2**-8 of itself
MARGIN = 3.0                        # every negative control misses its bound by this factor at least

# what the launchers of csrc/pmx_train.hip cap their grids at (tests/test_gpu_norm_kernels.py::test_launcher_caps looks them up)
LN32_FWD_BLOCKS = 4096
LN32_FWD_TRIP = LN32_FWD_BLOCKS * 256                    # rows of one forward trip
LN32_PARTIAL_ROWS = 2048
LN32_BWD_TRIP = LN32_PARTIAL_ROWS // 4 * 256             # 131 072 rows of one backward trip, 64 per partial row
GN_HW_EDGES = (192, 448, 1024)                           # KMAX = 3, 7, 16 elements per lane and channel
OPT_PARTIALS = 1024
OPT_NORM_TRIP = OPT_PARTIALS * 256 * 4                   # floats of one trip of the norm launch
OPT_UPDATE_BLOCKS = 2048
OPT_UPDATE_TRIP = OPT_UPDATE_BLOCKS * 256                # elements of one trip of the update launch
COLSUM_BLOCKS = 512


# ---------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------
def row_scale(ref):
    """[rows, ...] -> the largest magnitude of every row, shaped to broadcast against ref."""
    flat = ref.abs().reshape(ref.shape[0], -1) if ref.dim() > 1 else ref.abs().reshape(-1, 1)
    m = flat.max(1).values if flat.shape[1] else flat.new_zeros(flat.shape[0])
    return m.reshape([ref.shape[0]] + [1] * (ref.dim() - 1))


def _worst(err, bound):
    """max err / bound; where the bound is zero any error is infinitely far out, none is 0."""
    if err.numel() == 0:
        return 0.0
    q = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).to(err.dtype))
    q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)
    return float(q.max())


def ratio(got, ref, scale):
    """The worst |got - ref| / scale (a NaN or an error on a zero scale counts as infinite)."""
    err = (got.to(ref.dtype).reshape(ref.shape) - ref).abs()
    return _worst(err, scale.expand_as(ref) if scale.dim() == ref.dim() else scale)


def study(fn, device="cpu"):
    """fn(dtype) -> (outputs, scales).  -> (ref64, scales64, F): the float64 run and, per output, F = max(4 x the float32 run's ratio,
    FLOOR)."""
    ref, scale = fn(torch.float64)
    ref32, _ = fn(torch.float32)
    F = {k: max(4.0 * ratio(ref32[k], ref[k], scale[k]), FLOOR) for k in ref}
    return ref, scale, F


def excess(got, ref, scale, F, bf16=False):
    """The worst |got - ref| / (F * scale [+ 2**-8 |ref| for a bfloat16 output]): <= 1 passes."""
    err = (got.to(ref.dtype).reshape(ref.shape) - ref).abs()
    bound = (F * scale).expand_as(ref).clone() if scale.dim() == ref.dim() else F * scale
    if bf16:
        bound = bound + BF16_STEP * ref.abs()
    return _worst(err, bound)


def ulps_apart32(a, b):
    """Distance of two finite float32 tensors of one sign in units of the last place."""
    return (a.float().view(torch.int32).long() - b.float().view(torch.int32).long()).abs()


def lane_sum(t):
    """[rows, n, 64] -> [rows]: every lane adds its n terms one after the other, then the 64 lanes meet in the butterfly of
    wave_sum (csrc/pmx_common.h): the order of the kernels' wavefront sums."""
    s = torch.zeros(t.shape[0], 64, dtype=t.dtype, device=t.device)
    for i in range(t.shape[1]):
        s = s + t[:, i]
    idx = torch.arange(64, device=t.device)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, idx ^ o]
    return s[:, 0]


def gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z * 0.70710678118654752))


def gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z * 0.70710678118654752)) + z * 0.3989422804014327 * torch.exp(-0.5 * z * z)


# ---------------------------------------------------------------------------------------------------------------
# ln32: y = LayerNorm(x + a) * w + b over 32 features, one lane per row
# ---------------------------------------------------------------------------------------------------------------
def ln32_ref(case, dtype, device="cpu", round_sum=False, one_pass=False, stats32=True, fwd_only=False):
    """case: x, a, dy [rows, 32] (float32 or bfloat16), w, b [32] float32.  x and a are widened exactly and added in `dtype` (never
    rounded to their own type: round_sum is the negative control that does).  Two-pass mean and biased variance, each sum taken
    feature by feature as the kernel's lane does.  The backward starts, as the kernel's does, from the float32 mean and rstd.
    -> (outputs, scales)"""
    x, a, dy, w, b = (case[k].to(device) for k in ("x", "a", "dy", "w", "b"))
    z = x.to(dtype) + a.to(dtype)
    if round_sum:
        z = z.to(x.dtype).to(dtype)
    w, b, g = w.to(dtype), b.to(dtype), dy.to(dtype)
    s, sa = torch.zeros_like(z[:, 0]), torch.zeros_like(z[:, 0])
    for j in range(32):
        s, sa = s + z[:, j], sa + z[:, j].abs()
    mean = s / 32
    if one_pass:
        q = torch.zeros_like(s)
        for j in range(32):
            q = q + z[:, j] * z[:, j]
        var = q / 32 - mean * mean
    else:
        q = torch.zeros_like(s)
        for j in range(32):
            q = q + (z[:, j] - mean) * (z[:, j] - mean)
        var = q / 32
    rstd = 1.0 / torch.sqrt(var + EPS)
    y = (z - mean[:, None]) * rstd[:, None] * w + b
    if fwd_only:
        return {"y": y, "mean": mean, "rstd": rstd}, {"y": row_scale(y), "mean": sa / 32, "rstd": rstd.abs()}
    mean0, rstd0 = mean, rstd
    if stats32:                                          # what the backward entry point is given: float32 statistics
        mean, rstd = mean.float().to(dtype), rstd.float().to(dtype)
    xh = (z - mean[:, None]) * rstd[:, None]
    gw = g * w
    c1, c2 = torch.zeros_like(s), torch.zeros_like(s)
    for j in range(32):
        c1, c2 = c1 + gw[:, j], c2 + gw[:, j] * xh[:, j]
    dz = rstd[:, None] * (gw - (c1 / 32)[:, None] - xh * (c2 / 32)[:, None])
    out = {"y": y, "mean": mean0, "rstd": rstd0, "dz": dz, "dw": (g * xh).sum(0), "db": g.sum(0)}
    scale = {"y": row_scale(y), "mean": sa / 32, "rstd": rstd0.abs(), "dz": row_scale(dz), "dw": (g * xh).abs().sum(0), "db": g.abs().sum(0)}
    return out, scale


LN32_SIZES = (1, 63, 64, 65, 255, 256, 257, LN32_BWD_TRIP - 1, LN32_BWD_TRIP, LN32_BWD_TRIP + 1, 2 * LN32_BWD_TRIP + 1)
LN32_FWD_ONLY_ROWS = LN32_FWD_TRIP + 257
LN32_ROW_KINDS = ("constant", "offset", "spike", "cancel", "bf16_sum")      # `offset` in float32 only, `bf16_sum` in bfloat16 only


def ln32_special_rows(rows):
    """The positions the hard rows go to: the first rows, the last, and both sides of every backward trip boundary."""
    pos = {r for r in range(min(rows, 5))} | {rows - 1 - r for r in range(min(rows, 5))}
    for t in range(LN32_BWD_TRIP, rows + 1, LN32_BWD_TRIP):
        pos |= {r for r in range(t - 3, t + 3) if 0 <= r < rows}
    return sorted(pos)


def ln32_case(rows, seed, bf16, fwd_only=False):
    """Random rows with the hard kinds cycled through ln32_special_rows; the gradient of those rows is 16 times the others' so that a
    row left out of dw / db shows in a sum over a quarter of a million rows.
      constant  x + a the same number in every feature: y = b exactly, rstd = 1 / sqrt(eps)
      offset    common offset 1e3, spread 0.1 (float32 only: bfloat16 has no such values)
      spike     one feature 1e4 among unit ones
      cancel    x = -a exactly
      bf16_sum  bfloat16 x = 256 + 2k, a = -64 - m / 2: x + a lies between 128 and 256 on half-integers, which bfloat16 does not
                have.  (With a = -256 + small as a bfloat16 value, x + a is an integer below 256 and rounding it changes nothing.)"""
    g = torch.Generator().manual_seed(seed)
    io = torch.bfloat16 if bf16 else torch.float32
    x, a = torch.randn(rows, 32, generator=g), 0.5 * torch.randn(rows, 32, generator=g)
    dy = None if fwd_only else torch.randn(rows, 32, generator=g)
    kinds = [k for k in LN32_ROW_KINDS if k != ("offset" if bf16 else "bf16_sum")]
    where = {}
    for i, r in enumerate(ln32_special_rows(rows) if rows else ()):
        if rows == 1:
            continue                                      # a single row stays random
        kind = kinds[i % len(kinds)]
        where[r] = kind
        if kind == "constant":
            x[r], a[r] = 1.5, 0.25
        elif kind == "offset":
            x[r], a[r] = 1e3 + 0.1 * torch.randn(32, generator=g), 0.01 * torch.randn(32, generator=g)
        elif kind == "spike":
            x[r], a[r] = 1.0, 0.0
            x[r, int(torch.randint(32, (1,), generator=g))] = 1e4
        elif kind == "cancel":
            a[r] = -x[r].to(io).float()
        else:
            x[r] = 256.0 + 2.0 * torch.randint(4, (32,), generator=g)
            a[r] = -64.0 - 0.5 * torch.randint(16, (32,), generator=g)
        if dy is not None:
            dy[r] *= 16.0
    case = {"x": x.to(io), "a": a.to(io), "w": 1.0 + 0.5 * torch.randn(32, generator=g), "b": 0.5 * torch.randn(32, generator=g), "kinds": where}
    case["dy"] = torch.zeros(rows, 32, dtype=io) if dy is None else dy.to(io)
    return case


def ln32_controls(case, ref, scale, F, bf16, device="cpu"):
    """-> [(what, output, excess)] of every negative control that applies to the case."""
    rows, ctl = case["x"].shape[0], []

    def held(what, names, mut):
        for n in names:
            ctl.append((what, n, excess(mut[n], ref[n], scale[n], F[n], bf16 and n in ("y", "dz"))))
    if "offset" in case["kinds"].values():
        held("one-pass variance in float32", ("rstd",), ln32_ref(case, torch.float32, device, one_pass=True)[0])
    if "bf16_sum" in case["kinds"].values():
        held("x + a rounded to bfloat16", ("y", "rstd"), ln32_ref(case, torch.float64, device, round_sum=True)[0])
    if rows > LN32_BWD_TRIP:
        first = {k: (v[:LN32_BWD_TRIP] if k in ("x", "a", "dy") else v) for k, v in case.items()}
        part = ln32_ref(first, torch.float64, device)[0]
        mut = {"dz": torch.cat([part["dz"], torch.zeros_like(ref["dz"][LN32_BWD_TRIP:])]), "dw": part["dw"], "db": part["db"]}
        held("rows past the first backward trip left out", ("dz", "dw", "db"), mut)
    return ctl


# ---------------------------------------------------------------------------------------------------------------
# gn8: y = gelu(GroupNorm(h) * w + b (+ res)), 8 channels per group, one wavefront per (sample, group) row
# ---------------------------------------------------------------------------------------------------------------
def gn_kmax(HW):
    return 3 if HW <= GN_HW_EDGES[0] else 7 if HW <= GN_HW_EDGES[1] else 16


def _lanes(t, HW):
    """[rows, 8, HW] -> [rows, 8 * KMAX, 64]: element e of a channel sits in lane e % 64, slots past HW hold zeros."""
    K = gn_kmax(HW)
    pad = torch.zeros(t.shape[0], 8, 64 * K, dtype=t.dtype, device=t.device)
    pad[:, :, :HW] = t
    return pad.view(t.shape[0], 8 * K, 64)


def gn8_ref(case, dtype, device="cpu", one_pass=False, div_group=False, count_pad=False, stats32=True):
    """case: h, dy (and res or None) [B, groups * 8, HW] in the IO type, NCHW order (the channels-last kernels see the same numbers
    at other addresses), w, b [groups * 8] float32.  Rows are (sample, group) pairs, row = sample * groups + group.
    Negative controls: one_pass (variance as E[h^2] - mean^2), div_group (weights of group row / groups), count_pad (the lane slots
    past HW enter the variance as (0 - mean)^2).  -> (outputs, scales); partial is [rows, 8, 2] = (sum dz * xhat, sum dz)."""
    h, dy, w, b = (case[k].to(device) for k in ("h", "dy", "w", "b"))
    B, C, HW = h.shape
    groups, rows, n = C // 8, B * C // 8, 8 * HW
    hh, g = h.to(dtype).reshape(rows, 8, HW), dy.to(dtype).reshape(rows, 8, HW)
    res = None if case.get("res") is None else case["res"].to(device).to(dtype).reshape(rows, 8, HW)
    r = torch.arange(rows, device=device)
    gi = torch.div(r, groups, rounding_mode="floor").clamp_max(groups - 1) if div_group else r % groups
    wr, br = w.to(dtype).view(groups, 8)[gi][:, :, None], b.to(dtype).view(groups, 8)[gi][:, :, None]
    inv = (torch.ones((), dtype=dtype, device=device) / n)          # the kernels multiply by 1.0f / n: on a constant group the mean is
    mean = lane_sum(_lanes(hh, HW)) * inv                           # then a float32 rounding off the constant, which rstd = 316 magnifies
    m3 = mean[:, None, None]
    if one_pass:
        var = lane_sum(_lanes(hh * hh, HW)) * inv - mean * mean
    else:
        var = lane_sum(_lanes((hh - m3) ** 2, HW)) * inv
        if count_pad:
            var = var + (64 * gn_kmax(HW) - HW) * 8 * mean * mean * inv
    rstd = 1.0 / torch.sqrt(var + EPS)
    z = (hh - m3) * rstd[:, None, None] * wr + br
    y = gelu(z if res is None else z + res)
    mean0, rstd0 = mean, rstd
    if stats32:
        mean, rstd = mean.float().to(dtype), rstd.float().to(dtype)
    xh = (hh - mean[:, None, None]) * rstd[:, None, None]
    z = xh * wr + br
    dzz = g * gelu_grad(z if res is None else z + res)
    gg = dzz * wr
    c1, c2 = lane_sum(_lanes(gg, HW)) * inv, lane_sum(_lanes(gg * xh, HW)) * inv
    dh = rstd[:, None, None] * (gg - c1[:, None, None] - xh * c2[:, None, None])
    partial = torch.stack([(dzz * xh).sum(2), dzz.sum(2)], 2)
    out = {"y": y, "mean": mean0, "rstd": rstd0, "dh": dh, "dres": dzz, "partial": partial}
    scale = {"y": row_scale(y), "mean": hh.abs().reshape(rows, -1).mean(1), "rstd": rstd0.abs(), "dh": row_scale(dh), "dres": row_scale(dzz),
             "partial": torch.stack([(dzz * xh).abs().sum(2), dzz.abs().sum(2)], 2)}
    return out, scale


GN_HWS = (1, 63, 64, 65, 140, 192, 193, 448, 449, 1023, 1024)
GN_SHAPES = ((1, 1), (3, 1), (5, 3), (2, 4), (7, 4))                 # (B, groups): 1, 3, 15, 8, 28 rows
GN_ROW_KINDS = ("normal", "constant", "hot", "offset")               # `offset` in float32 only
GN_CASE_KINDS = ("rows", "tails", "cancel")


def gn8_case(B, groups, HW, seed, bf16, with_res, kind="rows"):
    """kind `rows`: random rows of mean 0.5 (so that a variance that counts the idle lane slots shows) with the row kinds cycled
    through, the last row always random:
      constant  one number in the whole group      hot  one pixel 100 among the random ones     offset  300 + 0.5 * randn (float32)
    kind `tails`: w = +-4 so that z spans +-12: both GELU tails and the underflow of gelu''s exp term.
    kind `cancel`: res = -(the normalised, scaled value), so that z is the rounding residue around 0."""
    g = torch.Generator().manual_seed(seed)
    io = torch.bfloat16 if bf16 else torch.float32
    C, rows = groups * 8, B * groups
    h = 0.5 + torch.randn(rows, 8, HW, generator=g)
    where = {}
    if kind == "rows":
        kinds = [k for k in GN_ROW_KINDS if not (bf16 and k == "offset")]
        for r in range(rows - 1):
            where[r] = kinds[r % len(kinds)]
            if where[r] == "constant":
                h[r] = -2.75
            elif where[r] == "hot":
                h[r, int(torch.randint(8, (1,), generator=g)), int(torch.randint(HW, (1,), generator=g))] = 100.0
            elif where[r] == "offset":
                h[r] = 300.0 + 0.5 * torch.randn(8, HW, generator=g)
    w, b = 1.0 + 0.5 * torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g)      # distinct per channel: a wrong group shows
    if kind == "tails":
        w, b = 4.0 * (1 - 2 * (torch.arange(C) % 2)).float(), 0.1 * torch.randn(C, generator=g)
    case = {"h": h.view(B, C, HW).to(io), "dy": torch.randn(B, C, HW, generator=g).to(io), "w": w, "b": b, "res": None, "kinds": where}
    if kind == "cancel":
        plain = gn8_ref(case, torch.float64)[0]
        zz = (case["h"].double().view(rows, 8, HW) - plain["mean"][:, None, None]) * plain["rstd"][:, None, None]
        zz = zz * w.double().view(groups, 8).repeat(B, 1)[:, :, None] + b.double().view(groups, 8).repeat(B, 1)[:, :, None]
        case["res"] = (-zz).view(B, C, HW).to(io)
    elif with_res:
        case["res"] = torch.randn(B, C, HW, generator=g).to(io)
    return case


def gn8_controls(case, ref, scale, F, bf16, device="cpu"):
    B, C, HW = case["h"].shape
    groups, rows, ctl = C // 8, B * C // 8, []

    def held(what, names, mut):
        for n in names:
            ctl.append((what, n, excess(mut[n], ref[n], scale[n], F[n], bf16 and n in ("y", "dh", "dres"))))
    if "offset" in case["kinds"].values():
        held("one-pass variance in float32", ("rstd",), gn8_ref(case, torch.float32, device, one_pass=True)[0])
    if groups > 1 and B > 1:
        held("weights of group row / groups", ("y", "dh", "partial"), gn8_ref(case, torch.float64, device, div_group=True)[0])
    if 64 * gn_kmax(HW) > HW:
        held("idle lane slots counted into the variance", ("rstd", "y"), gn8_ref(case, torch.float64, device, count_pad=True)[0])
    if rows % 4:
        mut = {k: ref[k].clone() for k in ("y", "mean", "rstd", "dh", "partial")}
        for k in mut:
            mut[k][rows - 1] = 0
        held("last row of a partly filled block dropped", ("y", "rstd", "dh", "partial"), mut)
    return ctl


# ---------------------------------------------------------------------------------------------------------------
# column sums of a bfloat16 matrix
# ---------------------------------------------------------------------------------------------------------------
COLSUM_CS = (8, 96, 256)


def colsum_rows_per_pass(C):
    return 256 // (C // 8)


def colsum_sizes(C):
    rp = colsum_rows_per_pass(C)
    return (0, 1, rp - 1, rp, COLSUM_BLOCKS * rp + 1)


def colsum_ref(x, dtype):
    v = x.to(dtype)
    return {"colsum": v.sum(0)}, {"colsum": x.double().abs().sum(0)}


def colsum_case(rows, C, seed):
    """Columns of very different size (so that a bound by the largest column would hide the small ones), every fourth centred."""
    g = torch.Generator().manual_seed(seed)
    amp = 10.0 ** (torch.arange(C) % 5 - 2).float()
    x = torch.randn(rows, C, generator=g) * amp + amp * (torch.arange(C) % 4 != 0)
    return x.to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------
# the optimizer tail: clip by the global norm, Adam, EMA, the bfloat16 copy, the report sums
# ---------------------------------------------------------------------------------------------------------------
HP = dict(lr_bc1=3e-4 / (1 - 0.9), rsqrt_bc2=1.0 / math.sqrt(1 - 0.999), b1=0.9, b2=0.999, eps=1e-5, max_norm=0.5, decay=0.995)


def hp32(hp=HP):
    """The hyper-parameters as the float32 values the entry point receives."""
    return {k: float(torch.tensor(v, dtype=torch.float32)) for k, v in hp.items()}


def opt_norm(g, skip_tail=False, squares32=False):
    """float32(sqrt(sum g^2 in float64)).  Negative controls: the n & 3 elements behind the last float4 left out; squares in float32."""
    n = g.numel()
    gg = g[:n - (n & 3)] if skip_tail else g
    sq = (gg * gg).double() if squares32 else gg.double() ** 2
    return torch.sqrt(sq.sum()).float()


def opt_ref(state, dtype, hp=None, norm=None, keep_from=None):
    """state: g, p, m, v, ema float32 [n].  The kernel's five float32 lines in `dtype`, from the float32 norm.
    keep_from: negative control, the elements from that index on stay as they were.  -> (outputs, scales)"""
    hp = hp32() if hp is None else hp
    g, p, m, v, e = (state[k].to(dtype) for k in ("g", "p", "m", "v", "ema"))
    norm = opt_norm(state["g"]) if norm is None else norm
    one = torch.ones((), dtype=dtype, device=g.device)
    c = {k: torch.tensor(x, dtype=torch.float32).to(dtype).to(g.device) for k, x in hp.items()}
    scl = torch.minimum(c["max_norm"] / (norm.to(dtype) + torch.tensor(1e-6, dtype=torch.float32).to(dtype)), one)
    g1 = g * scl
    m1 = m + (one - c["b1"]) * (g1 - m)
    v1 = v * c["b2"] + (one - c["b2"]) * g1 * g1
    upd = c["lr_bc1"] * (m1 / (torch.sqrt(v1) * c["rsqrt_bc2"] + c["eps"]))
    p1 = p - upd
    e1 = e * c["decay"] + p1 * (one - c["decay"])
    out = {"g": g1, "m": m1, "v": v1, "p": p1, "ema": e1}
    scale = {"g": g1.abs(), "m": m.abs() + (one - c["b1"]) * (g1.abs() + m.abs()), "v": v1.abs(), "p": p.abs() + upd.abs(),
             "ema": (e * c["decay"]).abs() + (p1 * (one - c["decay"])).abs()}
    if keep_from is not None:
        for k, old in zip(("g", "p", "m", "v", "ema"), (g, p, m, v, e)):
            out[k] = torch.cat([out[k][:keep_from], old[keep_from:]])
    return out, scale


def bf16_truncate(p):
    """Negative control for the bfloat16 copy: the upper 16 bits of the float32 words."""
    return (p.float().contiguous().view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)


OPT_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, OPT_UPDATE_TRIP - 1, OPT_UPDATE_TRIP, OPT_UPDATE_TRIP + 1, OPT_NORM_TRIP - 1, OPT_NORM_TRIP,
             OPT_NORM_TRIP + 1, OPT_NORM_TRIP + 3, 2 * OPT_NORM_TRIP + 3)
OPT_GRAD_KINDS = ("small", "large", "below", "above", "zero", "tail_mass", "late_mass", "huge", "v_zero")


def opt_kind_applies(kind, n):
    return {"tail_mass": n & 3 != 0 and n > 4, "late_mass": n > OPT_UPDATE_TRIP, "huge": n == 1025}.get(kind, True)


def opt_state(n, seed, kind="small", device="cpu"):
    """A state of n elements with a gradient of the kind:
      small / large   random, norm below / above max_norm          below / above   the norm a hair (1 +- 2**-18) off max_norm: below, norm + 1e-6 < max_norm and the scale is exactly 1
      zero            all zero: every denominator is v's own        tail_mass       3.0 in the n & 3 last elements, zeros before
      late_mass       zeros in the update launch's first trip, random of norm 4 behind it
      huge            |g| = 1e20: the squares overflow float32, the float64 sum does not          v_zero   v = 0 with m != 0"""
    gen = torch.Generator(device=device).manual_seed(seed)
    rn = lambda: torch.randn(n, generator=gen, device=device)
    g, p, m, v = rn(), rn(), 0.01 * rn(), 1e-4 * torch.rand(n, generator=gen, device=device)
    ema = p + 0.01 * rn()
    nrm = float(g.double().norm())
    if kind in ("small", "v_zero"):
        g = g * (0.1 / nrm)
    elif kind == "large":
        g = g * (7.0 / nrm)
    elif kind in ("below", "above"):
        g = (g.double() * (HP["max_norm"] * (1 + (2.0 ** -18 if kind == "above" else -2.0 ** -18)) / nrm)).float()
    elif kind == "zero":
        g = torch.zeros_like(g)
    elif kind == "tail_mass":
        g = torch.zeros_like(g)
        g[n - (n & 3):] = 3.0
    elif kind == "late_mass":
        g[:OPT_UPDATE_TRIP] = 0
        g = g * (4.0 / float(g.double().norm()))
    elif kind == "huge":
        g = 1e20 * torch.sign(g)
    if kind == "v_zero":
        v = torch.zeros_like(v)
    return {"g": g, "p": p, "m": m, "v": v, "ema": ema}


def opt_controls(state, ref, scale, F, kind):
    n, ctl = state["g"].numel(), []

    def held(what, mut):
        for k in ("g", "m", "v", "p", "ema"):
            ctl.append((what, k, excess(mut[k], ref[k], scale[k], F[k])))
    if kind == "tail_mass" and n & 3:
        held("the n & 3 tail left out of the norm", opt_ref(state, torch.float64, norm=opt_norm(state["g"], skip_tail=True))[0])
    if kind == "huge":
        held("squares formed in float32", opt_ref(state, torch.float64, norm=opt_norm(state["g"], squares32=True))[0])
    if n > OPT_UPDATE_TRIP and kind in ("large", "late_mass"):
        held("elements past the update's first trip unchanged", opt_ref(state, torch.float64, keep_from=OPT_UPDATE_TRIP)[0])
    return ctl


def worst_by_output(ctl):
    """[(what, output, excess)] -> {what: the largest excess over its outputs}: a control fails if ANY output catches it."""
    best = {}
    for what, _, x in ctl:
        best[what] = max(best.get(what, 0.0), x)
    return best


# ---------------------------------------------------------------------------------------------------------------
# the cases both test files go through
# ---------------------------------------------------------------------------------------------------------------
def ln32_cases():
    return [(rows, bf16) for rows in LN32_SIZES for bf16 in (False, True)]


def ln32_seed(rows, bf16):
    return 7919 * rows + bf16


def gn8_cases():
    """(layout, bfloat16, HW): every case runs all of GN_SHAPES with and without res."""
    return [(lay, bf16, HW) for lay, bf16 in (("nchw", False), ("nchw", True), ("cl", True)) for HW in GN_HWS]


def gn8_seed(B, groups, HW, bf16, with_res):
    return ((B * 31 + groups) * 2053 + HW) * 4 + 2 * bf16 + with_res


def opt_cases(model_n=None):
    """(n, kind) for every size and every gradient kind that applies to it."""
    sizes = OPT_SIZES + ((model_n,) if model_n else ())
    return [(n, k) for n in sizes for k in OPT_GRAD_KINDS if opt_kind_applies(k, n)]


def opt_seed(n, kind):
    return 131 * n + OPT_GRAD_KINDS.index(kind)
