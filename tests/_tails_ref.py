"""Float64 references of the head-tail kernels (csrc/pmx_heads.hip) that round to bfloat16 exactly where the kernels do, the seeded
inputs the tail tests share, the negative controls and the bounds.

Rounding points, read off the kernel source (`bf_round`, `bf_pack`, the `store8<__hip_bfloat16>` stores):
  * actor tail: w2 is rounded; g = bf16(gelu(z)) in the logits and in dW2; LayerNorm (weight, bias, statistics), gelu'(z) and the
    whole input gradient stay float32; dh is rounded once at the store when the IO type is bfloat16, not at all when it is float32;
  * critic tail: pooled = bf16(sum * (1 / S)); W1, b1, w2 rounded; z = bf16(pre); g = bf16(gelu(z)) in the value and in dw2;
    dh = bf16(dv * w2 * gelu'(z)) feeds dW1, db1 and the token gradient; dtokens = bf16(W1^T dh * (1 / S)) on every token.
`rounding=False` turns every one of these off: the references are then the plain formulas, which tests/test_tails_ref_cpu.py holds
against float64 autograd.  The backward passes are written by hand because autograd cannot express these rounding points.

The references are dtype-generic: called on float32 tensors they are "the float32 run" from which the bounds are made (`bounds`)."""
import math

import torch

EPS = 1e-5
HID, NACT, DM = 512, 5, 32
FLOOR = 16 * 2.0 ** -24             # no float32 bound is tighter than 16 ulp of the scale
BF16_FACTOR = 2 * 2.0 ** -8         # the project's two-bfloat16-steps bound
FLIPS = 4                           # roundings of one output element's summands that may fall the other way in float32 (see `excess`)
MARGIN = 3.0                        # every negative control misses its bound by this factor at least (tests/test_tails_ref_cpu.py)


def _rounder(rounding):
    if rounding:
        return lambda t: t.float().to(torch.bfloat16).to(t.dtype)
    return lambda t: t


def gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z * 0.70710678118654752))


def gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z * 0.70710678118654752)) + z * 0.3989422804014327 * torch.exp(-0.5 * z * z)


def gelu_grad2(z):
    return 0.3989422804014327 * torch.exp(-0.5 * z * z) * (2.0 - z * z)


def bf16_step(t):
    """The distance from each |t| to the next bfloat16 value above it (zero where t is zero)."""
    a = t.abs()
    return torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp_min(2.0 ** -120))) - 7), torch.zeros_like(a))


def actor_tail_ref(h, dlogits, lnw, lnb, w2, b2, eps=EPS, rounding=True, io_bf16=True, stats=None):
    """logits = W2 gelu(LayerNorm_512(h)) + b2 and every gradient.  h [B][512], dlogits [B][5]; `stats` [B][2] (mean, rstd): the
    backward half then starts from the given statistics, as pmx_actor_tail_backward does."""
    r = _rounder(rounding)
    W = r(w2)
    mean = h.mean(-1, keepdim=True)
    xc = h - mean
    rstd = (xc.square().mean(-1, keepdim=True) + eps).rsqrt()
    z = xc * rstd * lnw + lnb
    out = {"logits": r(gelu(z)) @ W.T + b2, "stats": torch.cat([mean, rstd], -1), "rstd": rstd[:, 0]}
    if stats is not None:
        mean, rstd = stats[:, :1], stats[:, 1:]
    xh = (h - mean) * rstd
    z = xh * lnw + lnb
    g = r(gelu(z))
    dz = (dlogits @ W) * gelu_grad(z)
    gd = dz * lnw
    dh = rstd * (gd - gd.mean(-1, keepdim=True) - xh * (gd * xh).mean(-1, keepdim=True))
    out.update({"dh": r(dh) if io_bf16 else dh, "dw2": dlogits.T @ g, "db2": dlogits.sum(0), "dlnw": (dz * xh).sum(0), "dlnb": dz.sum(0)})
    out["_scale"] = {"db2": torch.maximum(out["db2"].abs().max(), dlogits.abs().max())}
    if rounding:                            # a flipped bf16(gelu(z)) moves g by one step: logits by step |W2|, dW2 by |dlogits| step
        sg, dl = bf16_step(g), dlogits.abs()
        out["_slack"] = {"logits": FLIPS * torch.stack([(sg * W[o].abs()).amax(-1) for o in range(NACT)], -1),
                         "dw2": FLIPS * torch.stack([(dl[:, o, None] * sg).amax(0) for o in range(NACT)])}
    return out


def critic_tail_ref(tokens, dvalue, w1, b1, w2, b2, pooled=None, rounding=True):
    """value = w2 . gelu(W1 mean_s tokens + b1) + b2 and every gradient.  tokens [B][S][32], dvalue [B], w2 [512], b2 [1]; with
    `pooled` [B][32] given, everything downstream of the pool is computed from it."""
    r = _rounder(rounding)
    B, S, _ = tokens.shape
    inv_s = 1.0 / S
    if pooled is None:
        pooled = r(tokens.sum(1) * inv_s)
    W1, bb, ww = r(w1), r(b1), r(w2)
    z = r(pooled @ W1.T + bb)
    g = r(gelu(z))
    dh = r(dvalue[:, None] * ww * gelu_grad(z))
    dtok = r((dh @ W1) * inv_s)
    out = {"pooled": pooled, "value": g @ ww + b2, "dtokens": dtok[:, None, :].expand(B, S, DM), "dw1": dh.T @ pooled, "db1": dh.sum(0),
           "dw2": dvalue @ g, "db2": dvalue.sum().reshape(1)}
    out["_scale"] = {"db2": torch.maximum(out["db2"].abs().max(), dvalue.abs().max())}
    if rounding:
        # a flipped z = bf16(pre) moves g by step(z) |gelu'(z)| and perhaps one more step of g, dh by |dv w2 gelu''(z)| step(z) and
        # perhaps one more step of dh; a flipped bf16(gelu(z)) or bf16(dh) moves that one by a step
        dv, sz = dvalue.abs()[:, None], bf16_step(z)
        a = sz * gelu_grad(z).abs() + bf16_step(g)
        sdh = dv * ww.abs() * gelu_grad2(z).abs() * sz + bf16_step(dh)
        pa = pooled.abs()
        out["_slack"] = {"value": FLIPS * (a * ww.abs()).amax(-1), "dw2": FLIPS * (dv * a).amax(0), "db1": FLIPS * sdh.amax(0),
                         "dw1": FLIPS * torch.stack([(sdh * pa[:, k, None]).amax(0) for k in range(DM)], -1)}
    return out


# the plain modules, for autograd
def actor_tail_plain(h, lnw, lnb, w2, b2, eps=EPS):
    return torch.nn.functional.linear(torch.nn.GELU()(torch.nn.functional.layer_norm(h, (HID,), lnw, lnb, eps)), w2, b2)


def critic_tail_plain(tokens, w1, b1, w2, b2):
    return torch.nn.functional.linear(torch.nn.GELU()(torch.nn.functional.linear(tokens.mean(1), w1, b1)), w2[None], b2)[:, 0]


# how an output is held: "row" = float32, per sample against that sample's largest entry; "tensor" = float32 against the tensor's
# largest entry; "bf16row" = bfloat16, two steps of that sample's largest entry.  (`value` has ONE entry per sample, which may lie
# as close to zero as it likes: its scale is the tensor's.)
ACTOR_PARAM_GRADS = ("dw2", "db2", "dlnw", "dlnb")
CRITIC_PARAM_GRADS = ("dw1", "db1", "dw2", "db2")
ACTOR_FWD_OUTS = {"logits": "row", "stats": "row", "rstd": "row"}
CRITIC_FWD_OUTS = {"value": "tensor"}


def actor_outs(io_bf16):
    return dict(ACTOR_FWD_OUTS, dh="bf16row" if io_bf16 else "row", **{k: "tensor" for k in ACTOR_PARAM_GRADS})


def critic_outs():
    return dict(CRITIC_FWD_OUTS, dtokens="bf16row", **{k: "tensor" for k in CRITIC_PARAM_GRADS})


# ---------------------------------------------------------------------------------------------------------------
# ratios and bounds
# ---------------------------------------------------------------------------------------------------------------
def _err_and_scale(got, ref, name, how):
    """-> (|got - ref| as [rows][entries], the scale of each row [rows][1]): one row for "tensor", one per sample otherwise.  The
    scale is the largest |ref| of the row; the bias gradients, sums that may cancel to anything, take their largest summand if that
    is larger (`_scale` of the reference)."""
    t = ref[name]
    rows = 1 if how == "tensor" else t.shape[0]
    err = (got.to(t.dtype) - t).abs().reshape(rows, -1)
    scale = t.abs().reshape(rows, -1).amax(1, keepdim=True)
    if name in ref.get("_scale", {}):
        scale = ref["_scale"][name].reshape(1, 1)
    return err, scale


def _worst(q, err):
    return math.inf if not bool(torch.isfinite(err).all()) else float(q.max())


def ratio(got, ref, name, how):
    """max |got - ref| relative to the scale of the tensor ("tensor") or of each sample's row ("row", "bf16row": the worst sample);
    a scale of zero admits only exact zeros; anything not finite is infinitely wrong."""
    if ref[name].numel() == 0:
        return 0.0
    err, scale = _err_and_scale(got, ref, name, how)
    e = err.amax(1, keepdim=True)
    return _worst(torch.where(scale > 0, e / scale.clamp_min(1e-300), torch.where(e > 0, math.inf, 0.0).to(e.dtype)), err)


def bounds(ref64, ref32, outs):
    """The factor F of every output of a case: 2 * 2**-8 for the bfloat16 ones; for the float32 ones 4 x the ratio the float32 run
    of the reference reaches against the float64 run, with a floor of 16 * 2**-24.  (The 4 is for the kernels' summation order --
    64 lanes, 4 waves, up to 128 partial rows against torch's -- and the few-ulp error of rsqrtf, erff and __expf.)"""
    return {k: BF16_FACTOR if how == "bf16row" else max(4.0 * ratio(ref32[k], ref64, k, how), FLOOR) for k, how in outs.items()}


def excess(got, ref, name, how, F):
    """max |got - ref| / (F * scale + slack): an output passes at 1 or below.  `slack` (`_slack` of the reference, per element) is
    what FLIPS roundings to bfloat16 that fall the other way may move the element by, each at the worst of its summands.  Why F
    alone does not do: a float32 evaluation moves a value that lies within its error of the midpoint of two bfloat16 values to
    the other one.  Those are rare, discrete events (one in 1e4 to 1e5 roundings), each worth a whole bfloat16 step; whether the
    float32 run of the reference meets one on the row that matters is luck (on an MI355X it met none in all of B = 512, F = 2.9e-5,
    where the actor kernel met one, 2.0e-4 of the row), so the size of such an event is taken from the rounding itself."""
    if ref[name].numel() == 0:
        return 0.0
    err, scale = _err_and_scale(got, ref, name, how)
    tol = (F * scale).expand_as(err)
    if name in ref.get("_slack", {}) and how != "bf16row":
        tol = tol + ref["_slack"][name].reshape(err.shape)
    return _worst(torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).to(err.dtype)), err)


def bf16_steps_apart(got, ref):
    """|got - ref| in bfloat16 steps (8 bits of precision) of the larger of the two, elementwise."""
    big = torch.maximum(got.abs(), ref.abs()).double().clamp_min(2.0 ** -120)
    step = torch.exp2(torch.floor(torch.log2(big)) - 7)
    return (got.double() - ref.double()).abs() / step


# ---------------------------------------------------------------------------------------------------------------
# negative controls, from the reference alone
# ---------------------------------------------------------------------------------------------------------------
def zero_last(t):
    """A per-sample output with its last sample zeroed."""
    out = t.clone()
    out[-1] = 0
    return out


def control_excesses(ref, bnd, last, trip, per_sample, param_grads):
    """-> [(what, output, excess)]: how far over its bound (`excess`) each wrong answer made from the reference lies: every
    per-sample output with its last sample zeroed, every parameter gradient without the last sample (`last`: the reference of that
    sample alone) and without the last ragged trip (`trip`: the reference of its samples, or None)."""
    out = [("last sample zeroed", k, excess(zero_last(ref[k]), ref, k, how, bnd[k])) for k, how in per_sample.items()]
    out += [("without the last sample", k, excess(ref[k] - last[k], ref, k, "tensor", bnd[k])) for k in param_grads]
    if trip is not None:
        out += [("without the last ragged trip", k, excess(ref[k] - trip[k], ref, k, "tensor", bnd[k])) for k in param_grads]
    return out


def ragged_trip(B, cap_samples):
    """The samples of the last, ragged trip of a grid-stride loop that covers cap_samples per trip (None: there is none)."""
    if B <= cap_samples or B % cap_samples == 0:
        return None
    return slice((B // cap_samples) * cap_samples, B)


# ---------------------------------------------------------------------------------------------------------------
# seeded inputs (CPU generator, so that the CPU test sees exactly the rows the GPU tests use)
# ---------------------------------------------------------------------------------------------------------------
ACTOR_ROW_KINDS = ("normal", "zero_var", "offset", "far_offset", "large", "outlier", "tails")
DLOGITS_KINDS = ("normal", "one_hot", "quarter_zero")
CRITIC_TOKEN_KINDS = ("normal", "constant", "large", "cancelling")
DVALUE_KINDS = ("normal", "quarter_zero")
ZERO_VAR_CONSTANTS = (0.0, 1.0, -3.0, 100.0)
# far_offset: rows at about 1000 with a spread of 0.3 to 1.1 (as in tests/_token_ref.py).  bfloat16 has a step of 4 there and would
# quantise the spread away, so the kind is float32 only.  A one-pass variance E[x^2] - mean^2 in float32 is off by tens of percent
# on these rows; on the `offset` rows (30 + 2 N(0, 1)) it would still pass.


def hard_row_mask(B):
    """The hard samples of a mixed batch: every other one, counted from the end so that the LAST sample is an ordinary one and the
    one before it hard.  (tests/_token_ref.py makes the last row hard; here a zero-variance last sample contributes exactly nothing
    to dLN.weight -- its normalised row is zero -- so a control that drops it could not be told from the truth.)  The ragged last
    trips of the looped sizes hold both sorts."""
    return (B - 1 - torch.arange(B)) % 2 == 1


def zero_sample_mask(B):
    """The samples whose incoming gradient is exactly zero in the `quarter_zero` kinds: every fourth, never the last."""
    idx = torch.arange(B)
    return (idx % 4 == 0) & (idx != B - 1)


def _uniform(g, bound, *shape):
    return (torch.rand(*shape, generator=g) * 2 - 1) * bound


def _ordinary_last(d):
    """The incoming gradient with every non-zero entry of the LAST sample pushed away from zero by one: the sample the negative
    controls drop carries a gradient of ordinary size whatever the seed drew (one that happens to weigh 0.01 is, rightly, missed
    by no bound)."""
    d = d.clone()
    d[-1] = d[-1] + torch.sign(d[-1])
    return d


def actor_case(B, seed, kind="normal", dl_kind="normal", io_bf16=True):
    """nn.LayerNorm / nn.Linear initialisation with the perturbations of test_fused_actor_tail_matches_torch (asymmetric everywhere).
    -> float32 parameters, h [B][512] in the IO type, dlogits [B][5] float32, on the CPU."""
    assert kind in ACTOR_ROW_KINDS and dl_kind in DLOGITS_KINDS and not (kind == "far_offset" and io_bf16)
    g = torch.Generator().manual_seed(seed)
    p = {"lnw": 1.0 + 0.2 * torch.randn(HID, generator=g), "lnb": 0.1 * torch.randn(HID, generator=g),
         "w2": 3.0 * _uniform(g, HID ** -0.5, NACT, HID), "b2": _uniform(g, HID ** -0.5, NACT)}
    if kind == "tails":                     # z = +-5 + 0.6 N(0, 1): [-8, -3] and [3, 8], both tails of GELU on every row
        p["lnw"] *= 0.6
        p["lnb"] += 5.0 * (1.0 - 2.0 * (torch.arange(HID) % 2))
    h = 0.2 + 1.5 * torch.randn(B, HID, generator=g)
    noise = torch.randn(B, HID, generator=g)
    idx = torch.arange(B)
    if kind == "zero_var":
        hard = torch.tensor(ZERO_VAR_CONSTANTS)[(idx // 2) % 4][:, None].expand(B, HID)
    elif kind == "offset":
        hard = 30.0 + 2.0 * noise
    elif kind == "far_offset":
        hard = 1000.0 + (0.3 + 0.8 * torch.rand(B, 1, generator=g)) * noise
    elif kind == "large":
        hard = 30.0 * h
    elif kind == "outlier":
        hard = noise.clone()
        hard[idx, torch.randint(0, HID, (B,), generator=g)] = 200.0
    else:
        hard = h
    h = torch.where(hard_row_mask(B)[:, None], hard, h)
    dl = torch.randn(B, NACT, generator=g)
    if dl_kind == "one_hot":
        dl = torch.nn.functional.one_hot(torch.randint(0, NACT, (B,), generator=g), NACT).float()
    elif dl_kind == "quarter_zero":
        dl = torch.where(zero_sample_mask(B)[:, None], torch.zeros_like(dl), dl)
    p["h"] = h.to(torch.bfloat16) if io_bf16 else h
    p["dlogits"] = _ordinary_last(dl)
    return p


def critic_case(B, S, seed, kind="normal", dv_kind="normal"):
    """The critic head's nn.Linear initialisation with the perturbations of test_fused_critic_tail_matches_torch.
    -> float32 parameters (w2 [512], b2 [1]), bfloat16 tokens [B][S][32], dvalue [B] float32, on the CPU."""
    assert kind in CRITIC_TOKEN_KINDS and dv_kind in DVALUE_KINDS
    g = torch.Generator().manual_seed(seed)
    p = {"w1": 2.0 * _uniform(g, DM ** -0.5, HID, DM), "b1": _uniform(g, DM ** -0.5, HID) + 0.1 * torch.randn(HID, generator=g),
         "w2": 4.0 * _uniform(g, HID ** -0.5, HID), "b2": _uniform(g, HID ** -0.5, 1)}
    tok = 1.2 * torch.randn(B, S, DM, generator=g) + 0.3 * torch.randn(B, 1, DM, generator=g)
    noise = torch.randn(B, S, DM, generator=g)
    if kind == "constant":
        hard = noise[:, :1].expand(B, S, DM)
    elif kind == "large":
        hard = 30.0 * tok
    elif kind == "cancelling":              # +-64 down the tokens: a float32 sum has to cancel them to leave the N(0, 1) part
        hard = 64.0 * (1.0 - 2.0 * (torch.arange(S) % 2))[None, :, None] + noise
    else:
        hard = tok
    p["tokens"] = torch.where(hard_row_mask(B)[:, None, None], hard, tok).to(torch.bfloat16)
    dv = torch.randn(B, generator=g)
    if dv_kind == "quarter_zero":
        dv = torch.where(zero_sample_mask(B), torch.zeros_like(dv), dv)
    p["dvalue"] = _ordinary_last(dv)
    return p


def cast(case, dtype=torch.float64, device="cpu"):
    return {k: v.to(device=device, dtype=dtype) for k, v in case.items()}


def actor_ref_of(case, device="cpu", dtype=torch.float64, rounding=True, rows=slice(None), stats=None):
    c = cast(case, dtype, device)
    return actor_tail_ref(c["h"][rows], c["dlogits"][rows], c["lnw"], c["lnb"], c["w2"], c["b2"], rounding=rounding,
                          io_bf16=case["h"].dtype == torch.bfloat16, stats=None if stats is None else stats.to(device=device, dtype=dtype)[rows])


def critic_ref_of(case, device="cpu", dtype=torch.float64, rounding=True, rows=slice(None), pooled=None):
    c = cast(case, dtype, device)
    return critic_tail_ref(c["tokens"][rows], c["dvalue"][rows], c["w1"], c["b1"], c["w2"], c["b2"],
                           pooled=None if pooled is None else pooled.to(device=device, dtype=dtype)[rows], rounding=rounding)


def actor_study(case, bwd_cap_samples, device="cpu"):
    """-> (float64 reference, {output: F}, control_excesses) of an actor case; bwd_cap_samples: samples per trip of the backward."""
    B = case["h"].shape[0]
    outs = actor_outs(case["h"].dtype == torch.bfloat16)
    ref = actor_ref_of(case, device)
    bnd = bounds(ref, actor_ref_of(case, device, torch.float32), outs)
    tr = ragged_trip(B, bwd_cap_samples)
    ctl = control_excesses(ref, bnd, actor_ref_of(case, device, rows=slice(B - 1, B)), None if tr is None else actor_ref_of(case, device, rows=tr),
                           {k: outs[k] for k in ("logits", "stats", "rstd", "dh")}, ACTOR_PARAM_GRADS)
    return ref, bnd, ctl


def critic_study(case, bwd_cap_samples, device="cpu", pooled=None):
    """The same for a critic case.  The float32 run is given the float64 run's pooled tokens (see critic_tail_ref); `pooled`: the
    pooled tokens to start from instead of the reference's own (the kernel's, for its value)."""
    B = case["tokens"].shape[0]
    outs = critic_outs()
    ref = critic_ref_of(case, device, pooled=pooled)
    bnd = bounds(ref, critic_ref_of(case, device, torch.float32, pooled=ref["pooled"].float()), outs)
    tr = ragged_trip(B, bwd_cap_samples)
    ctl = control_excesses(ref, bnd, critic_ref_of(case, device, rows=slice(B - 1, B), pooled=pooled),
                           None if tr is None else critic_ref_of(case, device, rows=tr, pooled=pooled),
                           {"value": "tensor", "dtokens": "bf16row"}, CRITIC_PARAM_GRADS)
    return ref, bnd, ctl


# ---------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_head_tails.py; tests/test_tails_ref_cpu.py holds every one of them to the margin of its controls
# ---------------------------------------------------------------------------------------------------------------
# literal grid caps of the launchers in csrc/pmx_heads.hip (blocks of 4 waves, one sample per wave); PMX_HEADS_PARTIAL_ROWS (128)
# caps the actor backward and the number of weight-gradient chunks and is read from the library's Python binding
ACTOR_FWD_BLOCKS, CRITIC_BLOCKS, WGRAD_CHUNK = 1024, 512, 16
ACTOR_SIZES = (1, 3, 4, 5, 511, 512, 513, 1027, 4095, 4096, 4097, 8195)
ACTOR_KIND_SIZES = (5, 4097)                # an edge size and one that loops in both directions (2nd forward trip, 9th backward)
CRITIC_S = 7
CRITIC_SIZES = (1, 3, 4, 5, 15, 16, 17, 19, 2047, 2048, 2049, 4099)
CRITIC_KIND_SIZES = (5, 2049)
# `large` tokens at the edge size only: among 2 049 samples of which every other is 30 times larger, the bfloat16 steps of the large
# samples' z and gelu(z) (`_slack`) are as large as the whole contribution of the ordinary last sample to dw1 and dw2, and the
# control that drops it misses its bound by 1.2 and 0.7 instead of 3 (tests/test_tails_ref_cpu.py prints the margins)
CRITIC_KIND_SIZES_OF = {"large": (5,)}
CRITIC_S_EDGES = (1, 15, 16, 17, 154, 400, 1024)
CRITIC_S_EDGE_B = 5


def actor_cases():
    """(B, row kind, dlogits kind, io_bf16) of every actor case."""
    out = [(B, "normal", "normal", io) for B in ACTOR_SIZES for io in (True, False)]
    out += [(B, k, "normal", k != "far_offset") for B in ACTOR_KIND_SIZES for k in ACTOR_ROW_KINDS[1:]]
    out += [(B, "normal", k, True) for B in ACTOR_KIND_SIZES for k in DLOGITS_KINDS[1:]]
    return out


def critic_cases():
    """(B, S, token kind, dvalue kind) of every critic case."""
    out = [(B, CRITIC_S, "normal", "normal") for B in CRITIC_SIZES]
    out += [(CRITIC_S_EDGE_B, S, "normal", "normal") for S in CRITIC_S_EDGES]
    out += [(B, CRITIC_S, k, "quarter_zero") for k in CRITIC_TOKEN_KINDS[1:] for B in CRITIC_KIND_SIZES_OF.get(k, CRITIC_KIND_SIZES)]
    out += [(B, CRITIC_S, "normal", "quarter_zero") for B in CRITIC_KIND_SIZES]
    return out


def actor_seed(B, kind="normal", dl_kind="normal", io_bf16=True):
    return 3000 + B + 11 * ACTOR_ROW_KINDS.index(kind) + 101 * DLOGITS_KINDS.index(dl_kind) + (0 if io_bf16 else 7)


def critic_seed(B, S, kind="normal", dv_kind="normal"):
    return 5000 + B + 13 * S + 11 * CRITIC_TOKEN_KINDS.index(kind) + 101 * DVALUE_KINDS.index(dv_kind)


def wgrad_chunks(B, partial_rows):
    """-> (samples per chunk, chunks) of pmx_critic_tail_wgrad_kernel for B samples (the launcher's arithmetic, restated)."""
    chunk = WGRAD_CHUNK
    if -(-B // chunk) > partial_rows:
        chunk = -(-B // partial_rows)
    return chunk, -(-B // chunk)


def heads_blocks(B, cap):
    return max(1, min(-(-B // 4), cap))
