"""Layer-by-layer float64 references of the fused actor tower (csrc/pmx_actor.hip), made from the kernels' OWN saved tensors: the
decoders of `save` and `scratch`, the per-layer references, the bounds, the negative controls and the seeded cases that
tests/test_gpu_tower_layers.py and tests/test_tower_layers_cpu.py share.

Why per layer: an 8-layer bfloat16 network amplifies one flipped rounding, so end to end two correct evaluations disagree by 1e-3
to 1e-2 on every parameter gradient and the suite cannot see a dropped cell.  Every reference here starts from what the kernel
itself wrote one step earlier, so that one rounding (or two, named below) lies between its input and the element it judges.

Layouts, read off the kernel source (the source is the authority; the maps below are index arithmetic written out):
  * P layout (`dump_index`), the `h` and `y` dumps of `save`: [layer][sample][tile t][half m][lane] of 4 bfloat16 = channels
    16 m + 4 (lane >> 4) .. + 3 of padded position q = WP + 16 t + (lane & 15), WP = W + 2, row = q / WP, col = q % WP; a board
    cell has 1 <= col <= W and row <= H.  `save` = h dumps of the 8 layers, y dumps of the 8 layers, then float32 statistics
    [layer][sample][group][mean, rstd] ((0, 1) for the two layers without GroupNorm).  Tile counts are the bucket's.
  * operand layout, the `dH` dumps at the head of `scratch`: [layer][sample][ks * 2 + mo][lane] of 8 bfloat16 = channel
    16 mo + (lane & 15) at padded positions WP + 32 ks + 8 (lane >> 4) + j, j = 0..7 (what the two transposing LDS reads of a lane
    return: the four positions of its row group, then the four 256 bytes on).  The one-wave kernel, both split kernels and the
    large-board instantiations (4 and 8 waves) compute the same destination from the same map, so ONE decoder serves every path.
    With an odd tile count the last key-pair block reaches 16 positions past the last tile: map cells nobody writes, zero.
  * the gradient buffer: 36 tiles [(mo * 2 + ni) * 9 + tap][lane][r] per layer = dW[16 mo + 4 (lane >> 4) + r][16 ni + (lane & 15)][tap],
    then dbias, dGN.weight, dGN.bias as [layer][32].  All layers are 32 -> 32 with zero weights for the stem's missing channels, so
    the references are too and the padding of the gradient is compared as well (exact zeros).
Every pad column, every position below the board and the tail tiles of a bucket must be exactly zero in all three dumps
(`Layout.pads_are_zero`): the next layer's convolution reads them.

Rounding points (bf_pack in the kernels): weights; h_l = bf16(conv + bias); y_l = bf16(gelu(GN(h_l) + skip)); dz_l = bf16(dY_l gelu'(z_l))
(`dgelu_quad`); dH_l = bf16(rstd (gw dz - S1 - xhat S2)) (pass 2); the next dY = bf16(skip gradient + convT(dH_l)).  dgw, dgb sum the
ROUNDED dz, dbias sums the ROUNDED dH, dW contracts the rounded dH with the rounded y_{l-1}: given the dumps these are pure float32 sums.

What each check starts from (`checks`): h_l from the decoded y_{l-1} (the observation for layer 0); the statistics and y_l from the
decoded h_l (and the decoded y_{l-2} behind a skip connection) -- one rounding each, sharper than starting both from y_{l-1}; dW_l and
dbias_l from the decoded dH_l and y_{l-1}; dH_7, dgw_7, dgb_7 from dfeat and the dumps; dH_l, dgw_l, dgb_l of l = 6, 4, 2, 0 from the
decoded dH_{l+1}; those of l = 5, 3, 1 from the decoded dH_{l+1} plus the dz of layer l + 2, which is not dumped and is taken from
the reference's own layer l + 2.  The backward references use the kernel's own saved statistics, as the kernel does.

Bounds (none comes from a kernel's output).  A bfloat16 element passes when |got - v| <= 0.5 step + F scale + slack: v the unrounded
float64 value, step the bfloat16 step at max(|got|, |v|), scale the largest |v| of that sample and layer, F = max(4 x the ratio the
float32 run of the same per-layer reference reaches against the float64 run, 16 * 2**-24).  The float32 run is given the float64
run's rounded intermediates (dY, dz), so F measures float32 arithmetic and not the luck of meeting a flipped rounding; what a flipped
upstream rounding may do is `slack`, per element (`_rounded_unc`: the steps are taken at |value| + what came from upstream, and the
float32 error of the value itself, FLOOR of its sample's largest, is added before the step): unc(dY_l) = step(dY_l) [+ unc(dz_{l+2})
for l = 5, 3, 1], unc(dz_l) = step(dz_l) + |gelu'(z_l)| unc(dY_l), and dH_l may move by rstd |gw| unc(dz_l) at its own element plus FLIPS such flips elsewhere in its group
through S1 and S2 (divided by the group's size).  unc(dY_7) = 0: dfeat is given.  So layer 7 carries one upstream rounding, layers
6, 4, 2, 0 two, and layers 5, 3, 1 accumulate those of layer l + 2: their dH is held to a few steps (measured below), still far
from what the controls do, so they are NOT left to the end-to-end tests.  The float32 sums (dW, dbias, dgw, dgb, mean, rstd) use F
alone against the tensor's largest entry or, where a sum can cancel, its largest summand; dgw and dgb also get FLIPS flips of the
worst summand.  mean is held against the largest |h| of its sample, rstd against itself.

Negative controls, all made from the reference: parameter-gradient sums without the last sample, without the last cell of the last
sample, dW without the last ragged run of the weight-gradient kernel's chunking (`wgrad_runs` restates the launcher), dW with one
tap holding its neighbour's column, every dump with one cell zeroed, and a pad left non-zero (which `pads_are_zero` must see).
tests/test_tower_layers_cpu.py holds every one to a miss by MARGIN at every case of the GPU test.

Cases: seeded on the CPU.  From B = 3 up sample 0 is all zero and sample 1 all ones with plane 1 = 5 (near-constant GroupNorm rows);
B = 2 holds the zero sample only, B = 1 neither: the LAST sample is always an ordinary one, with `_ordinary_last` on its dfeat.

Recorded figures (MI355X, the `LAYERFIG` lines of tests/test_gpu_tower_layers.py; information, not the source of any bound).  Worst
share of its bound that an output used, over the 89 cases: h and y 1.000 (an element whose unrounded value sits on the boundary
between two bfloat16 values is half a step from either), dH 0.99 (16 x 32, B = 2 049, layer 1: the layer with the most upstream
roundings), dW 0.54 (32 x 20, B = 3), dbias 0.31, dGN.weight 0.29, dGN.bias 0.27, rstd 0.26, mean 0.05.  The measured F: dW up to
1.7e-5 (32 x 20, B = 257; 3e-6 to 8e-6 on the batches of thousands), h up to 4.1e-6, y 1.3e-6, dbias 1.6e-6, dGN.weight 1.7e-6,
dH, dGN.bias, mean and rstd at the floor 9.5e-7.  Negative controls (`LAYERCTL` lines of tests/test_tower_layers_cpu.py): the
smallest miss over the 55 value cases is a factor of 4.2; on the GPU none passes.
History of the slack: written first with the steps taken at the reference's own magnitude and without the float32 error in front
of each rounding, it was exceeded once in 89 cases, by 0.8 % (dH of layer 1, 16 x 32, B = 2 049); two bfloat16 roundings of values
d apart differ by up to d + half a step at EACH, and the larger of the two may lie across a power of two, which `_rounded_unc`
now says."""

import torch
import torch.nn.functional as Fn

import _tower_ref as T
from _tails_ref import FLIPS, FLOOR, MARGIN, _ordinary_last, bf16_step, bounds, excess, gelu, gelu_grad, ratio, zero_sample_mask  # noqa: F401

NL, CH, EPS = 8, 32, 1e-5
CIN = (8, 16, 32, 32, 32, 32, 32, 32)
COUT = (16, 32, 32, 32, 32, 32, 32, 32)
GRAD_W, GRAD_B, GRAD_GNW, GRAD_GNB, GRAD_FLOATS = 0, 73728, 73984, 74240, 74496
W_PART_ROWS = 128                   # csrc/pmx_actor.hip
MI355X_CUS = 256                    # the launchers size the weight-gradient chunks from the device's CU count
DFEAT_KINDS = ("normal", "quarter_zero", "one_cell")
# dfeat is DFEAT_SIGMA N(0, 1) with the last sample's entries pushed away from zero by one (`_ordinary_last`): the sample the controls
# drop is then among the larger of its batch, as samples with a large advantage are among a PPO minibatch.  The flip slack of dgw and
# dgb is FLIPS times the LARGEST summand of the whole batch, so that a cell well below the largest is, rightly, missed by no bound.
DFEAT_SIGMA = 0.2
LAST_CELL_PUSH = 3.0                # ... and the last cell of that sample, which a control drops on its own, by this much more
SHIFTED_TAP = 3                     # the control "one tap shifted by a column": tap (1, 0) holding what tap (1, 1) should


def has_skip(l):
    """z_l = GN(h_l) + y_{l-2}: the second convolution of each residual block"""
    return l >= 3 and l % 2 == 1


def rb(t):
    return t.to(torch.bfloat16).to(t.dtype)


# ---------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------
class Layout:
    """The index maps of one board: `p_perm` / `op_perm` [32 * H * W] give, for (channel, cell) in that order, the bfloat16 element
    of a sample's P-layout / operand-layout dump that holds it; `p_pad` / `op_pad` are all the other elements of the dump."""

    def __init__(self, H, W):
        self.H, self.W, self.WP, self.HW = H, W, W + 2, H * W
        self.NT = T.bucket(T.tiles(H, W))
        assert self.NT, (H, W)
        self.KS = (self.NT + 1) // 2
        self.p_elems, self.op_elems = self.NT * 512, self.KS * 1024
        e = torch.arange(self.p_elems)
        r, lane, m, t = e % 4, (e // 4) % 64, (e // 256) % 2, e // 512
        self.p_perm, self.p_pad = self._perm(16 * m + 4 * (lane // 16) + r, self.WP + 16 * t + lane % 16)
        e = torch.arange(self.op_elems)
        j, lane, mo, ks = e % 8, (e // 8) % 64, (e // 512) % 2, e // 1024
        self.op_perm, self.op_pad = self._perm(16 * mo + lane % 16, self.WP + 32 * ks + 8 * (lane // 16) + j)
        self.save_bytes = lambda B: B * (16 * self.p_elems * 2 + NL * 4 * 2 * 4)
        self.dh_bytes = lambda B: B * NL * self.op_elems * 2

    def _perm(self, chan, q):
        row, col = q // self.WP, q % self.WP
        valid = (col >= 1) & (col <= self.W) & (row >= 1) & (row <= self.H)
        key = chan * self.HW + (row - 1) * self.W + (col - 1)
        idx = torch.nonzero(valid)[:, 0]
        order = torch.argsort(key[idx])
        # the decoder reads exactly the board's cells, each once
        assert torch.equal(key[idx][order], torch.arange(CH * self.HW)), "a layout map does not cover the board exactly once"
        return idx[order], torch.nonzero(~valid)[:, 0]

    def to(self, device):
        for k in ("p_perm", "p_pad", "op_perm", "op_pad"):
            setattr(self, k, getattr(self, k).to(device))
        return self

    # --- decoders: raw bytes (uint8 tensors) -> values ---
    def split_save(self, save, B):
        """-> (h dumps, y dumps) as bfloat16 [8][B][p_elems] views and the statistics float32 [8][B][4][2]"""
        n = NL * B * self.p_elems * 2
        assert save.numel() == self.save_bytes(B)
        hd = save[:n].view(torch.bfloat16).view(NL, B, self.p_elems)
        yd = save[n:2 * n].view(torch.bfloat16).view(NL, B, self.p_elems)
        return hd, yd, save[2 * n:].view(torch.float32).view(NL, B, 4, 2)

    def split_scratch(self, scratch, B):
        return scratch[:self.dh_bytes(B)].view(torch.bfloat16).view(NL, B, self.op_elems)

    def decode(self, dump, perm, dtype=torch.float64):
        """dump [..., elems] bfloat16 -> [..., 32, H, W] in `dtype`"""
        return dump[..., perm].to(dtype).view(dump.shape[:-1] + (CH, self.H, self.W))

    def encode(self, t, perm, elems):
        """[..., 32, H, W] -> [..., elems] bfloat16, zero wherever the kernels promise zero"""
        out = torch.zeros(t.shape[:-3] + (elems,), dtype=torch.bfloat16, device=t.device)
        out[..., perm] = t.reshape(t.shape[:-3] + (-1,)).to(torch.bfloat16)
        return out

    def decode_save(self, save, B, dtype=torch.float64):
        """-> dict h, y [8][B][32][H][W], mean, rstd [8][B][4] (the kernel's float32 values), zeros_ok"""
        hd, yd, st = self.split_save(save, B)
        return {"h": self.decode(hd, self.p_perm, dtype), "y": self.decode(yd, self.p_perm, dtype), "mean": st[..., 0].to(dtype),
                "rstd": st[..., 1].to(dtype), "pads": self.pads_are_zero(hd, self.p_pad) and self.pads_are_zero(yd, self.p_pad)}

    def decode_dh(self, scratch, B, dtype=torch.float64):
        dd = self.split_scratch(scratch, B)
        return self.decode(dd, self.op_perm, dtype), self.pads_are_zero(dd, self.op_pad)

    def encode_save(self, h, y, mean, rstd):
        B = h.shape[1]
        st = torch.stack([mean, rstd], -1).to(torch.float32).contiguous()
        parts = [self.encode(h, self.p_perm, self.p_elems), self.encode(y, self.p_perm, self.p_elems)]
        out = torch.cat([p.contiguous().view(torch.uint8).reshape(-1) for p in parts] + [st.view(torch.uint8).reshape(-1)])
        assert out.numel() == self.save_bytes(B)
        return out

    def encode_dh(self, dH):
        return self.encode(dH, self.op_perm, self.op_elems).contiguous().view(torch.uint8).reshape(-1)

    @staticmethod
    def pads_are_zero(dump, pad):
        """every element outside the board's cells is +0 or -0 (the bit pattern without the sign)"""
        return not bool((dump[..., pad].view(torch.int16) & 0x7FFF).any())


def grad_perm():
    """[32 co * 32 ci * 9 taps] -> float index within a layer's 36 tiles of the gradient buffer"""
    i = torch.arange(36 * 256)
    r, lane, tile = i % 4, (i // 4) % 64, i // 256
    k, ni, mo = tile % 9, (tile // 9) % 2, tile // 18
    key = ((16 * mo + 4 * (lane // 16) + r) * CH + 16 * ni + lane % 16) * 9 + k
    order = torch.argsort(key)
    assert torch.equal(key[order], torch.arange(CH * CH * 9))
    return order


def decode_grad(grad, dtype=torch.float64):
    """the raw gradient buffer [GRAD_FLOATS] -> dW [8][32][32][9], db, dgw, dgb [8][32]"""
    g = grad.to(dtype)
    dW = g[GRAD_W:GRAD_B].view(NL, 36 * 256)[:, grad_perm().to(g.device)].view(NL, CH, CH, 9)
    return {"dW": dW, "db": g[GRAD_B:GRAD_GNW].view(NL, CH), "dgw": g[GRAD_GNW:GRAD_GNB].view(NL, CH), "dgb": g[GRAD_GNB:].view(NL, CH)}


def encode_grad(dW, db, dgw, dgb):
    out = torch.zeros(GRAD_FLOATS, dtype=torch.float32)
    w = torch.zeros(NL, 36 * 256, dtype=torch.float32)
    w[:, grad_perm()] = dW.reshape(NL, -1).float()
    out[GRAD_W:GRAD_B] = w.reshape(-1)
    out[GRAD_B:GRAD_GNW], out[GRAD_GNW:GRAD_GNB], out[GRAD_GNB:] = db.reshape(-1).float(), dgw.reshape(-1).float(), dgb.reshape(-1).float()
    return out


def wgrad_runs(B, nt_bucket, cus=MI355X_CUS):
    """-> (samples per run, runs): the launcher's arithmetic for the weight-gradient kernels, restated.  Buckets 10 / 11 / ... up to
    11 tiles: a run is one WAVE's `per_wave` samples (4 waves per chunk); larger buckets: one wave PAIR's `per_pair` samples."""
    if nt_bucket > 11:
        pairs = min((2 * cus // NL) * 2, W_PART_ROWS)
        per = max(-(-B // pairs), 2)
    else:
        chunks = min(2 * cus // NL, W_PART_ROWS)
        per = max(-(-B // (chunks * 4)), 2)
    return per, -(-B // per)


def last_ragged_run(B, nt_bucket, cus=MI355X_CUS):
    """The samples of the last run if it is shorter than the others (None: every run is full)."""
    per, runs = wgrad_runs(B, nt_bucket, cus)
    return slice((runs - 1) * per, B) if B % per else None


# ---------------------------------------------------------------------------------------------------------------
# seeded cases
# ---------------------------------------------------------------------------------------------------------------
def tower_params(seed=0):
    """The 28 float32 parameter tensors in the kernels' order (actor_tower._tower_params): conv weights, conv biases, GroupNorm
    weights, GroupNorm biases; nn.Conv2d's initial range times 1.5, the vectors perturbed as tests/_tower_ref.model perturbs them."""
    g = torch.Generator().manual_seed(seed)
    u = lambda bound, *shape: (torch.rand(*shape, generator=g) * 2 - 1) * bound
    w = [u(1.5 * (9 * ci) ** -0.5, co, ci, 3, 3) for ci, co in zip(CIN, COUT)]
    b = [u((9 * ci) ** -0.5, co) + 0.3 * torch.randn(co, generator=g) for ci, co in zip(CIN, COUT)]
    gw = [1.0 + 0.3 * torch.randn(CH, generator=g) for _ in range(6)]
    gb = [0.3 * torch.randn(CH, generator=g) for _ in range(6)]
    return w + b + gw + gb


class Params:
    """The parameters as the kernels see them: 32 -> 32 channels in every layer, weights [8][co][ci][tap] (bfloat16-rounded
    unless rounding is off), GroupNorm weight 1 and bias 0 on the two layers without one."""

    def __init__(self, tensors, dtype=torch.float64, device="cpu", rounding=True):
        self.W = torch.zeros(NL, CH, CH, 9, dtype=dtype, device=device)
        self.b = torch.zeros(NL, CH, dtype=dtype, device=device)
        self.gw = torch.ones(NL, CH, dtype=dtype, device=device)
        self.gb = torch.zeros(NL, CH, dtype=dtype, device=device)
        for l in range(NL):
            w = tensors[l].detach().to(device=device, dtype=dtype)
            self.W[l, :COUT[l], :CIN[l]] = (rb(w) if rounding else w).reshape(COUT[l], CIN[l], 9)
            self.b[l, :COUT[l]] = tensors[8 + l].detach().to(device=device, dtype=dtype)
            if l >= 2:
                self.gw[l] = tensors[16 + l - 2].detach().to(device=device, dtype=dtype)
                self.gb[l] = tensors[22 + l - 2].detach().to(device=device, dtype=dtype)

    def to(self, dtype):
        out = object.__new__(Params)
        out.W, out.b, out.gw, out.gb = self.W.to(dtype), self.b.to(dtype), self.gw.to(dtype), self.gb.to(dtype)
        return out


def case_seed(H, W, B, kind="normal"):
    return 7000 + 100 * H + W + 13 * B + 1009 * DFEAT_KINDS.index(kind)


def tower_case(H, W, B, kind="normal", seed=None):
    """-> {"obs": float32 [B][8][H][W] planes as tests/_tower_ref.planes draws them (small integers: exact in uint8 and bfloat16),
    "dfeat": bfloat16 [B][H * W][32]}, on the CPU"""
    assert kind in DFEAT_KINDS
    g = torch.Generator().manual_seed(case_seed(H, W, B, kind) if seed is None else seed)
    o = (torch.rand(B, 8, H, W, generator=g) < 0.25).float()
    o[:, 1] *= torch.randint(1, 6, (B, 1, 1), generator=g).float()
    if B >= 2:
        o[0] = 0.0
    if B >= 3:
        o[1] = 1.0
        o[1, 1] = 5.0
    d = DFEAT_SIGMA * torch.randn(B, H * W, CH, generator=g)
    if kind == "quarter_zero":
        d = torch.where(zero_sample_mask(B)[:, None, None], torch.zeros_like(d), d)
    elif kind == "one_cell":
        keep = torch.zeros(B, H * W, 1, dtype=torch.bool)
        keep[-1, -1] = True
        d = torch.where(keep, d, torch.zeros_like(d))
    d = _ordinary_last(d)
    d[-1, -1] += LAST_CELL_PUSH * torch.sign(d[-1, -1])
    return {"obs": o, "dfeat": d.to(torch.bfloat16)}


def obs32(obs, dtype, device):
    """the observation as the kernels' map holds it: bfloat16-rounded planes in channels 0..7 of 32"""
    B, _, H, W = obs.shape
    x = torch.zeros(B, CH, H, W, dtype=dtype, device=device)
    x[:, :8] = obs.to(device).to(torch.bfloat16).to(dtype)
    return x


def dfeat_nchw(dfeat, dtype, device):
    B, HW, _ = dfeat.shape
    return dfeat.to(device=device, dtype=dtype).transpose(1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------
# the per-layer arithmetic (dtype-generic: called on float32 tensors it is "the float32 run")
# ---------------------------------------------------------------------------------------------------------------
CHUNK = 256


def unfold3x3(x):
    """x [n][32][H][W] -> [ci * 9 + tap][n * H * W]: the nine shifted copies of the zero-padded input, written out (what nn.Unfold(3,
    padding=1) returns, already in the shape of ONE matrix operand for the whole chunk)"""
    n, _, H, W = x.shape
    xp = Fn.pad(x, (1, 1, 1, 1)).transpose(0, 1)
    out = x.new_empty(CH, 9, n, H, W)
    for ky in range(3):
        for kx in range(3):
            out[:, ky * 3 + kx] = xp[:, :, ky:ky + H, kx:kx + W]
    return out.view(CH * 9, n * H * W)


def conv(x, Wm):
    """3 x 3 convolution, zero padding: x [B][32][H][W], Wm [co][ci][tap] -> [B][32][H][W]; unfold + matmul in sample chunks (no
    library convolution is involved, in any precision)"""
    out = torch.empty_like(x)
    A = Wm.reshape(CH, CH * 9)
    for i in range(0, x.shape[0], CHUNK):
        res = A @ unfold3x3(x[i:i + CHUNK])                                   # one matrix product per chunk
        out[i:i + CHUNK] = res.view(CH, -1, x.shape[2], x.shape[3]).transpose(0, 1)
    return out


def flipped(Wm):
    """the weights of the input-gradient convolution: [ci][co][8 - tap]"""
    return Wm.flip(-1).transpose(0, 1).contiguous()


def wgrad(dH, x):
    """dW[co][ci][tap] = sum over samples and positions of dH[co][pos] x[ci][pos + shift(tap)] -> [32][32][9]"""
    out = torch.zeros(CH, CH * 9, dtype=dH.dtype, device=dH.device)
    for i in range(0, x.shape[0], CHUNK):
        out += dH[i:i + CHUNK].transpose(0, 1).reshape(CH, -1) @ unfold3x3(x[i:i + CHUNK]).T
    return out.view(CH, CH, 9)


def _g(t):
    """[B][4] per group -> broadcastable over [B][32][H][W]"""
    return t.repeat_interleave(8, dim=1)[:, :, None, None]


def _c(v):
    return v[None, :, None, None]


def stats_of(h, l):
    """-> mean, rstd [B][4] of the four groups of 8 channels ((0, 1) on the layers without GroupNorm)"""
    B = h.shape[0]
    if l < 2:
        return torch.zeros(B, 4, dtype=h.dtype, device=h.device), torch.ones(B, 4, dtype=h.dtype, device=h.device)
    g = h.reshape(B, 4, -1)
    mean = g.mean(-1)
    return mean, ((g - mean[..., None]).square().mean(-1) + EPS).rsqrt()


def pre_act(h, mean, rstd, skip, P, l):
    """-> (xhat, z): z = GN(h) + skip"""
    xhat = (h - _g(mean)) * _g(rstd)
    z = xhat * _c(P.gw[l]) + _c(P.gb[l])
    return xhat, (z + skip if skip is not None else z)


def fwd_h(x, P, l):
    return conv(x, P.W[l]) + _c(P.b[l])


def fwd_y(h, mean, rstd, skip, P, l):
    return gelu(pre_act(h, mean, rstd, skip, P, l)[1])


def bwd_layer(dY, h, mean, rstd, skip, P, l, rnd=rb, dz=None):
    """One layer of the data gradient from its incoming dY: dz = rnd(dY gelu'(z)) (or the `dz` given), per-sample dgw = sum dz xhat and
    dgb = sum dz [B][32], and the unrounded dH."""
    xhat, z = pre_act(h, mean, rstd, skip, P, l)
    gp = gelu_grad(z)
    dz_v = dY * gp
    if dz is None:
        dz = rnd(dz_v)
    out = {"xhat": xhat, "gp": gp, "dz_v": dz_v, "dz": dz, "dgw": (dz * xhat).sum((2, 3)), "dgb": dz.sum((2, 3))}
    if l >= 2:
        B = h.shape[0]
        gd = _c(P.gw[l]) * dz
        S1, S2 = gd.reshape(B, 4, -1).mean(-1), (gd * xhat).reshape(B, 4, -1).mean(-1)
        out["dH_v"] = _g(rstd) * (gd - _g(S1) - xhat * _g(S2))
    else:
        out["dH_v"] = dz
    return out


def next_dy_v(dH, dz_skip, P, l):
    """the unrounded dY of layer l - 1: convT_l(dH_l) (+ the dz of layer l + 1 over the skip connection when l is 2, 4 or 6)"""
    v = conv(dH, flipped(P.W[l]))
    return v + dz_skip if dz_skip is not None else v


def chain(case, tensors, rounding=True, dtype=torch.float64, device="cpu", stats_f32=True):
    """The whole tower forward and backward from the per-layer pieces, each layer fed by the previous one: what the dumps hold if the
    kernels are right (tests/test_tower_layers_cpu.py encodes it as the dumps), and with `rounding=False` the plain network.
    `stats_f32`: the statistics pass through float32, as the kernels store them."""
    P = Params(tensors, dtype, device, rounding)
    r = rb if rounding else (lambda t: t)
    x = obs32(case["obs"], dtype, device)
    B, _, H, W = x.shape
    out = {k: [] for k in ("h", "y", "mean", "rstd")}
    for l in range(NL):
        h = r(fwd_h(out["y"][l - 1] if l else x, P, l))
        mean, rstd = stats_of(h, l)
        if rounding and stats_f32:
            mean, rstd = mean.float().to(dtype), rstd.float().to(dtype)
        y = r(fwd_y(h, mean, rstd, out["y"][l - 2] if has_skip(l) else None, P, l))
        for k, v in zip(("h", "y", "mean", "rstd"), (h, y, mean, rstd)):
            out[k].append(v)
    dY = dfeat_nchw(case["dfeat"], dtype, device).view(B, CH, H, W)
    dH, dz, dW, db, dgw, dgb = ([None] * NL for _ in range(6))
    for l in range(NL - 1, -1, -1):
        bl = bwd_layer(dY, out["h"][l], out["mean"][l], out["rstd"][l], out["y"][l - 2] if has_skip(l) else None, P, l, r)
        dH[l], dz[l], dgw[l], dgb[l] = r(bl["dH_v"]), bl["dz"], bl["dgw"].sum(0), bl["dgb"].sum(0)
        db[l], dW[l] = dH[l].sum((0, 2, 3)), wgrad(dH[l], out["y"][l - 1] if l else x)
        if l:
            dY = r(next_dy_v(dH[l], dz[l + 1] if l in (2, 4, 6) else None, P, l))
    res = {k: torch.stack(v) for k, v in out.items()}
    res.update({"dH": torch.stack(dH), "dW": torch.stack(dW), "db": torch.stack(db), "dgw": torch.stack(dgw), "dgb": torch.stack(dgb), "obs": x})
    return res


# ---------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------
class Check:
    """One output of one layer: the float64 reference `v`, how it is held and the wrong answers made from the reference.
    kind "elem": bfloat16 elements, [B][n], per sample; "sum": a float32 tensor against `scale`; "rows": float32, [rows][n], each row
    against its largest entry."""

    def __init__(self, name, kind, v, v32, scale=None, slack=None, controls=()):
        self.name, self.kind, self.v, self.scale, self.slack, self.controls = name, kind, v, scale, slack, list(controls)
        ref = {name: v}
        if scale is not None:
            ref["_scale"] = {name: scale}
        self.how = "tensor" if kind == "sum" else "row"
        self.ratio32 = ratio(v32.to(v.dtype), ref, name, self.how)
        self.F = bounds(ref, {name: v32.to(v.dtype)}, {name: self.how})[name]

    def _ref(self, got, rows=slice(None)):
        ref = {self.name: self.v[rows] if self.kind != "sum" else self.v}
        if self.scale is not None:
            ref["_scale"] = {self.name: self.scale}
        slack = self.slack
        if self.kind == "elem":
            half = 0.5 * bf16_step(torch.maximum(got.to(self.v.dtype).abs(), self.v[rows].abs()))
            slack = half if slack is None else half + slack[rows]
        if slack is not None:
            ref["_slack"] = {self.name: slack}
        return ref

    def excess(self, got, rows=slice(None)):
        """how far `got` lies over its bound: passes at 1 or below.  `rows`: the samples `got` holds, of a per-sample output (a
        control that changes the last sample is judged on that sample's row; the other rows are the reference's)"""
        got = got.reshape(self.v.shape if self.kind == "sum" else (-1,) + self.v.shape[1:])
        return excess(got, self._ref(got, rows), self.name, self.how, self.F)

    def worst_ratio(self, got):
        """max |got - v| / scale (information only)"""
        got = got.reshape(self.v.shape)
        return ratio(got, self._ref(got), self.name, self.how)


def _rounded_unc(v, upstream):
    """How far the kernel's bf16(v') may lie from the reference's bf16(v) when v' is the kernel's float32 evaluation of v from inputs
    that may themselves be off by `upstream`: |v' - v| <= upstream + FLOOR * (the sample's largest |v|), and two roundings differ by
    at most that plus half a step at each, steps taken at the larger magnitude |v| + |v' - v| (the other side of a power of two has
    twice the step)."""
    d = upstream + FLOOR * v.abs().flatten(1).amax(1).reshape(-1, 1, 1, 1)
    return d + bf16_step(v.abs() + d)


def _with_scale(t, scale):
    """[B][n] with one more column holding the row's scale: `ratio` and `excess` of tests/_tails_ref.py take a row's scale from its
    largest |reference| entry, and the column makes that at least `scale` (it is the same in what is compared, so its error is 0)"""
    return torch.cat([t, scale.reshape(-1, 1).to(t.dtype)], 1)


LAST = slice(-1, None)


def _zero_cell(t):
    """the LAST sample of [B][32][H][W], rounded to bfloat16, with its last cell zeroed -> [1][32 * H * W]"""
    out = rb(t[LAST]).clone()
    out[0, :, -1, -1] = 0
    return out.reshape(1, -1)


def _only_cell(t, b=-1):
    out = torch.zeros_like(t[b:] if b == -1 else t[b:b + 1])
    out[0, :, -1, -1] = t[b, :, -1, -1]
    return out


def checks(dec, case, tensors, device="cpu", cus=MI355X_CUS, backward=True):
    """Generator of every Check of a case, layer by layer.  `dec`: the decoded dumps {"h", "y", "dH": [8][B][32][H][W]; "mean", "rstd":
    [8][B][4]} in float64 on `device`.  Each check's reference starts from the decoded tensors named in the module docstring; the
    float32 run behind its F starts from the same tensors cast to float32."""
    f64, f32 = torch.float64, torch.float32
    P = Params(tensors, f64, device)
    P32 = P.to(f32)
    x = obs32(case["obs"], f64, device)
    B, _, H, W = x.shape
    nt = T.bucket(T.tiles(H, W))
    flat = lambda t: t.reshape(B, -1)
    for l in range(NL):
        xin = dec["y"][l - 1] if l else x
        v = fwd_h(xin, P, l)
        yield Check(f"h{l}", "elem", flat(v), flat(fwd_h(xin.to(f32), P32, l)), controls=[("one cell zeroed", _zero_cell(v))])
        h = dec["h"][l]
        mean, rstd = stats_of(h, l)
        m32, r32 = stats_of(h.to(f32), l)
        hmax = flat(h).abs().amax(1)
        yield Check(f"mean{l}", "rows", _with_scale(mean, hmax), _with_scale(m32, hmax))
        yield Check(f"rstd{l}", "rows", rstd.reshape(-1, 1), r32.reshape(-1, 1))
        skip = dec["y"][l - 2] if has_skip(l) else None
        v = fwd_y(h, mean, rstd, skip, P, l)
        v32 = fwd_y(h.to(f32), m32, r32, None if skip is None else skip.to(f32), P32, l)
        yield Check(f"y{l}", "elem", flat(v), flat(v32), controls=[("one cell zeroed", _zero_cell(v))])
    if not backward:
        return
    run = last_ragged_run(B, nt, cus)
    unc_dz = {}
    dz_ref = {}
    for l in range(NL - 1, -1, -1):
        h, mean, rstd = dec["h"][l], dec["mean"][l], dec["rstd"][l]
        skip = dec["y"][l - 2] if has_skip(l) else None
        if l == NL - 1:
            dY = dfeat_nchw(case["dfeat"], f64, device).view(B, CH, H, W)
            unc_dy = torch.zeros_like(dY)
        else:
            over = dz_ref[l + 2] if l in (1, 3, 5) else None
            dy_v = next_dy_v(dec["dH"][l + 1], over, P, l + 1)
            dY = rb(dy_v)
            unc_dy = _rounded_unc(dy_v, unc_dz[l + 2] if over is not None else 0.0)
        bl = bwd_layer(dY, h, mean, rstd, skip, P, l)
        # the float32 run, given the float64 run's roundings
        bl32 = bwd_layer(dY.to(f32), h.to(f32), mean.to(f32), rstd.to(f32), None if skip is None else skip.to(f32), P32, l, dz=bl["dz"].to(f32))
        unc = _rounded_unc(bl["dz_v"], bl["gp"].abs() * unc_dy)
        if l >= 2:
            k = _g(rstd) * _c(P.gw[l].abs()) * unc
            kg = k.reshape(B, 4, -1).amax(-1)
            xa = bl["xhat"].abs()
            slack = k + FLIPS / (8 * H * W) * _g(kg) * (1.0 + xa * _g(xa.reshape(B, 4, -1).amax(-1)))
        else:
            slack = unc
        yield Check(f"dH{l}", "elem", flat(bl["dH_v"]), flat(bl32["dH_v"]), slack=flat(slack),
                    controls=[("one cell zeroed", _zero_cell(bl["dH_v"]))])
        dz = bl["dz"]
        # (the two stem layers have no GroupNorm: the slots of the gradient buffer behind them belong to no parameter)
        for name, per, summand in (("dgw", bl["dgw"], dz * bl["xhat"]), ("dgb", bl["dgb"], dz)) if l >= 2 else ():
            tot = per.sum(0)
            big = summand.abs().amax((0, 2, 3))
            sl = FLIPS * (unc * (bl["xhat"].abs() if name == "dgw" else 1.0)).amax((0, 2, 3))
            cell = summand[-1, :, -1, -1]
            yield Check(f"{name}{l}", "sum", tot, bl32[name].sum(0), scale=torch.maximum(tot.abs().max(), big.max()), slack=sl,
                        controls=[("without the last sample", tot - per[-1]), ("without the last cell", tot - cell)])
        if l in (3, 5, 7):                      # layers 1, 3, 5 receive it over the skip connection
            unc_dz[l], dz_ref[l] = unc, dz
        for k in [k for k in unc_dz if k > l + 1]:
            del unc_dz[k], dz_ref[k]
        # the pure float32 sums, from the decoded dH and the layer's input
        dH = dec["dH"][l]
        xin = dec["y"][l - 1] if l else x
        tot = dH.sum((0, 2, 3))
        yield Check(f"db{l}", "sum", tot, dH.to(f32).sum((0, 2, 3)), scale=torch.maximum(tot.abs().max(), dH.abs().max()),
                    controls=[("without the last sample", tot - dH[-1].sum((1, 2))), ("without the last cell", tot - dH[-1, :, -1, -1])])
        dW = wgrad(dH, xin)
        ctl = [("without the last sample", dW - wgrad(dH[-1:], xin[-1:])), ("without the last cell", dW - wgrad(_only_cell(dH), xin[-1:]))]
        if run is not None:
            ctl.append(("without the last ragged run", dW - wgrad(dH[run], xin[run])))
        shifted = dW.clone()
        shifted[..., SHIFTED_TAP] = dW[..., SHIFTED_TAP + 1]
        ctl.append(("one tap shifted by a column", shifted))
        yield Check(f"dW{l}", "sum", dW, wgrad(dH.to(f32), xin.to(f32)), controls=ctl)


def got_of(name, dec, grads):
    """what the kernels gave for the check `name`: (tensor shaped like the check's reference or reshapeable to it)"""
    kind, l = name.rstrip("01234567"), int(name[-1])
    if kind in ("h", "y", "dH"):
        return dec[kind][l].reshape(dec[kind][l].shape[0], -1)
    if kind == "mean":
        return _with_scale(dec["mean"][l], dec["h"][l].reshape(dec["h"][l].shape[0], -1).abs().amax(1))
    if kind == "rstd":
        return dec["rstd"][l].reshape(-1, 1)
    return grads[kind][l]


# ---------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_tower_layers.py; tests/test_tower_layers_cpu.py holds the controls of every one of them
# ---------------------------------------------------------------------------------------------------------------
SMALL_BOARD = (11, 14)
SMALL_SIZES = (1, 2, 3, 7, 8, 9, 511, 512, 513, 1536, 1537, 2048, 2049, 4095, 4096, 4097)
MID_BOARDS = ((7, 20), (16, 14))                # buckets 10 and 16
MID_SIZES = (5, 513, 2049)
LARGE_BOARDS = ((13, 18), (18, 30), (32, 20))   # buckets 28, 36, 44
LARGE_SIZES = (1, 2, 3, 5, 257)
WIDE_BOARD, WIDE_SIZES = (16, 32), (1025, 2049)
KIND_SIZES = (5, 513, 4097)
KIND_BOARDS = MID_BOARDS + LARGE_BOARDS         # one board per other bucket, at B = 5
BOTH_TYPES_UP_TO = 513


def cases():
    """(H, W, B, dfeat kind, observation type name) of every GPU case"""
    out = []

    def add(board, B, kind="normal"):
        types = ["uint8"] if kind != "normal" or B > BOTH_TYPES_UP_TO else ["uint8", "bfloat16"] + (["float32"] if B == 5 else [])
        out.extend(board + (B, kind, t) for t in types)
    for B in SMALL_SIZES:
        add(SMALL_BOARD, B)
    for board in MID_BOARDS:
        for B in MID_SIZES:
            add(board, B)
    for board in LARGE_BOARDS:
        for B in LARGE_SIZES:
            add(board, B)
    for B in WIDE_SIZES:
        add(WIDE_BOARD, B)
    for kind in DFEAT_KINDS[1:]:
        for B in KIND_SIZES:
            add(SMALL_BOARD, B, kind)
        for board in KIND_BOARDS:
            add(board, 5, kind)
    return out


def value_cases():
    """the cases without the observation type: the values, and so the references and controls, do not depend on it"""
    seen = []
    for H, W, B, kind, _ in cases():
        if (H, W, B, kind) not in seen:
            seen.append((H, W, B, kind))
    return seen
