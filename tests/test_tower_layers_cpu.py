"""tests/_tower_layers_ref.py on the CPU: the layout maps are bijections between a board's cells and the elements of a dump that
hold them; the per-layer references chained WITHOUT rounding are float64 autograd through the plain modules to 1e-12; chained WITH
rounding they are float64 autograd through tests/_tower_ref.emulated_tower(ste=True) with the gradient rounded to bfloat16 at the
kernels' three points (dz, dH and the summed dY); and for every case of tests/test_gpu_tower_layers.py every negative control
misses its bound by MARGIN at least, with the reference's own chain encoded as the dumps, so that the GPU test cannot pass a
kernel that drops a sample, a cell or a ragged run."""

import pytest
import torch
import torch.nn.functional as F

import _tower_layers_ref as L
import _tower_ref as T
from test_gpu_any_board import BOARDS

ALL_BOARDS = BOARDS + [(7, 20), (11, 14)]


@pytest.mark.parametrize("board", ALL_BOARDS)
def test_encoders_and_decoders_are_mutually_inverse(board):
    H, W = board
    lay = L.Layout(H, W)            # (its constructor asserts that each map reads exactly the board's cells, each once)
    g = torch.Generator().manual_seed(H * 100 + W)
    for perm, pad, elems in ((lay.p_perm, lay.p_pad, lay.p_elems), (lay.op_perm, lay.op_pad, lay.op_elems)):
        assert perm.numel() == 32 * H * W and perm.numel() + pad.numel() == elems
        assert torch.equal(torch.sort(torch.cat([perm, pad]))[0], torch.arange(elems))
        t = torch.randn(2, 3, 32, H, W, generator=g).to(torch.bfloat16)
        dump = lay.encode(t, perm, elems)
        assert dump.shape == (2, 3, elems) and lay.pads_are_zero(dump, pad)
        assert torch.equal(lay.decode(dump, perm, torch.bfloat16), t)
        raw = torch.randn(2, 3, elems, generator=g).to(torch.bfloat16)
        raw[..., pad] = 0
        assert torch.equal(lay.encode(lay.decode(raw, perm, torch.bfloat16), perm, elems), raw)
        # negative control: a pad left non-zero is seen, wherever it is; a negative zero is a zero
        for i in (0, pad.numel() // 2, pad.numel() - 1):
            bad = raw.clone()
            bad[1, 2, pad[i]] = 2.0 ** -100
            assert not lay.pads_are_zero(bad, pad)
        raw[0, 0, pad[0]] = -0.0
        assert lay.pads_are_zero(raw, pad)
    # the whole buffers
    B = 3
    h, y = (torch.randn(8, B, 32, H, W, generator=g).to(torch.bfloat16) for _ in range(2))
    mean, rstd = torch.randn(8, B, 4, generator=g), torch.rand(8, B, 4, generator=g)
    dec = lay.decode_save(lay.encode_save(h, y, mean, rstd), B, torch.float32)
    assert dec["pads"] and torch.equal(dec["h"], h.float()) and torch.equal(dec["y"], y.float())
    assert torch.equal(dec["mean"], mean) and torch.equal(dec["rstd"], rstd)
    dH, ok = lay.decode_dh(lay.encode_dh(h), B, torch.bfloat16)
    assert ok and torch.equal(dH, h)


def test_gradient_buffer_round_trip():
    g = torch.Generator().manual_seed(1)
    dW, vecs = torch.randn(8, 32, 32, 9, generator=g), [torch.randn(8, 32, generator=g) for _ in range(3)]
    dec = L.decode_grad(L.encode_grad(dW, *vecs), torch.float32)
    assert torch.equal(dec["dW"], dW) and all(torch.equal(dec[k], v) for k, v in zip(("db", "dgw", "dgb"), vecs))
    # one spot of the map written out by hand: tile (mo 1, ni 0, tap 4), lane 37 (g 2, p 5), r 3 -> co 16 + 8 + 3, ci 5
    raw = torch.zeros(L.GRAD_FLOATS)
    raw[2 * 36 * 256 + ((1 * 2 + 0) * 9 + 4) * 256 + 37 * 4 + 3] = 1.0
    assert L.decode_grad(raw)["dW"][2, 27, 5, 4] == 1.0


def _agent(tensors, H, W):
    """MAPPOAgent's actor backbone in float64 with the given parameters (the plain modules)"""
    from pmx import actor_tower, mappo
    m = mappo.MAPPOAgent((8, H, W)).double()
    with torch.no_grad():
        for p, t in zip(actor_tower._tower_params(m.actor_backbone), tensors):
            p.copy_(t)
    return m, actor_tower._tower_params(m.actor_backbone)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _unpad(ch, params):
    """the chain's 32 x 32 gradients cut to the parameters' own shapes, in the parameters' order"""
    out = [ch["dW"][l, :L.COUT[l], :L.CIN[l]].reshape(L.COUT[l], L.CIN[l], 3, 3) for l in range(8)]
    out += [ch["db"][l, :L.COUT[l]] for l in range(8)] + [ch["dgw"][l] for l in range(2, 8)] + [ch["dgb"][l] for l in range(2, 8)]
    assert [o.shape for o in out] == [p.shape for p in params]
    return out


@pytest.mark.parametrize("board,B", [((11, 14), 5), ((7, 20), 3), ((13, 18), 2)])
def test_chain_without_rounding_is_autograd_through_the_plain_modules(board, B):
    H, W = board
    tensors, case = L.tower_params(3), L.tower_case(H, W, B)
    m, params = _agent(tensors, H, W)
    feat = m.actor_backbone[:-1](case["obs"].double())
    want = torch.autograd.grad((feat * L.dfeat_nchw(case["dfeat"], torch.float64, "cpu").view(B, 32, H, W)).sum(), params)
    ch = L.chain(case, tensors, rounding=False)
    assert _rel(ch["y"][7], feat.detach()) <= 1e-12
    for got, w in zip(_unpad(ch, params), want):
        assert _rel(got, w) <= 1e-12, (tuple(w.shape), _rel(got, w))
    # the padding of the 32 x 32 form carries nothing
    assert not ch["dW"][0, 16:].any() and not ch["dW"][0, :, 8:].any() and not ch["dW"][1, :, 16:].any() and not ch["db"][0, 16:].any()


class _RoundGradient(torch.autograd.Function):
    """identity whose gradient is rounded to bfloat16"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return L.rb(g)


def _emulated_with_rounded_gradients(m, obs):
    """tests/_tower_ref.emulated_tower(ste=True), line for line, with the gradient rounded where the kernels round it: on the
    convolution output (dH), on the GELU's argument (dz) and on every activation (dY, the sum over its consumers)"""
    rg = _RoundGradient.apply
    rnd = lambda x: x + (x.float().to(torch.bfloat16).to(x.dtype) - x).detach()
    bb = m.actor_backbone
    x = obs.to(bb[0].weight.dtype)

    def conv(c, x):
        return rg(rnd(F.conv2d(x, rnd(c.weight), None, padding=1) + c.bias.view(1, -1, 1, 1)))

    def act(z):
        return rg(rnd(F.gelu(rg(z))))
    x = act(conv(bb[0], x))
    x = act(conv(bb[2], x))
    for blk in (bb[4], bb[5], bb[6]):
        y = act(F.group_norm(conv(blk.conv1, x), 4, blk.gn1.weight, blk.gn1.bias, 1e-5))
        x = act(F.group_norm(conv(blk.conv2, y), 4, blk.gn2.weight, blk.gn2.bias, 1e-5) + x)
    return x


@pytest.mark.parametrize("board,B", [((11, 14), 5), ((7, 20), 3), ((13, 18), 2)])
def test_chain_with_rounding_is_autograd_through_the_emulation(board, B):
    """Both are float64 evaluations of the same roundings in another order of operations, so they agree exactly unless a value lies
    within 1e-16 of a rounding boundary; one flipped rounding would show as 1e-3 or so."""
    H, W = board
    tensors, case = L.tower_params(4), L.tower_case(H, W, B)
    m, params = _agent(tensors, H, W)
    obs = case["obs"].double()
    feat = _emulated_with_rounded_gradients(m, obs)
    with torch.no_grad():
        assert torch.equal(feat, T.emulated_tower(m, obs, ste=True))
    want = torch.autograd.grad((feat * L.dfeat_nchw(case["dfeat"], torch.float64, "cpu").view(B, 32, H, W)).sum(), params)
    ch = L.chain(case, tensors, stats_f32=False)
    assert torch.equal(ch["y"][7], feat.detach())
    for got, w in zip(_unpad(ch, params), want):
        assert _rel(got, w) <= 1e-10, (tuple(w.shape), _rel(got, w))
    # and the rounding does something
    plain = L.chain(case, tensors, rounding=False)
    assert 1e-4 < _rel(ch["dW"][4], plain["dW"][4]) < 0.2


def test_chunk_arithmetic_of_the_weight_gradient_kernels():
    """The launcher's arithmetic restated (256 CUs): 64 chunks of 4 waves, or 128 pairs of waves; at least 2 samples per run."""
    want = {1: (2, 1), 2: (2, 1), 3: (2, 2), 511: (2, 256), 512: (2, 256), 513: (3, 171), 2048: (8, 256), 2049: (9, 228), 4097: (17, 241)}
    assert {B: L.wgrad_runs(B, 11) for B in want} == want
    assert L.last_ragged_run(513, 11) is None and L.last_ragged_run(2049, 11) == slice(2043, 2049) and L.last_ragged_run(4097, 11) is None
    assert L.last_ragged_run(4095, 11) == slice(4080, 4095) and L.last_ragged_run(3, 11) == slice(2, 3)
    want = {1: (2, 1), 5: (2, 3), 257: (3, 86), 1025: (9, 114), 2049: (17, 121)}
    assert {B: L.wgrad_runs(B, 36) for B in want} == want
    assert L.last_ragged_run(257, 28) == slice(255, 257) and L.last_ragged_run(2049, 36) == slice(2040, 2049)


def test_the_case_table():
    cs = L.cases()
    assert len(cs) == len(set(cs)) and all(T.in_domain(H, W) for H, W, *_ in cs)
    assert {T.bucket(T.tiles(H, W)) for H, W, *_ in cs} == {10, 11, 16, 28, 36, 44}
    assert all(t == "uint8" for *_, B, k, t in cs if B > L.BOTH_TYPES_UP_TO or k != "normal")
    assert {(H, W, B) for H, W, B, k, t in cs if t == "float32"} == {b + (5,) for b in L.MID_BOARDS + L.LARGE_BOARDS}
    c = L.tower_case(11, 14, 9, "quarter_zero")
    assert not c["obs"][0].any() and bool((c["obs"][1, 0] == 1).all()) and bool((c["obs"][1, 1] == 5).all())
    d = c["dfeat"].float()
    assert [bool(d[i].any()) for i in range(9)] == [False, True, True, True, False, True, True, True, True] and float(d[-1].abs().min()) >= 1
    d = L.tower_case(11, 14, 9, "one_cell")["dfeat"].float()
    assert not d[:-1].any() and not d[-1, :-1].any() and float(d[-1, -1].abs().min()) >= 1


def dumps_of_the_chain(case, tensors, lay):
    """the reference's own chain, through the encoders and decoders: what the GPU test decodes if the kernels are right"""
    ch = L.chain(case, tensors)
    B = case["obs"].shape[0]
    dec = lay.decode_save(lay.encode_save(ch["h"], ch["y"], ch["mean"], ch["rstd"]), B)
    dec["dH"], ok = lay.decode_dh(lay.encode_dh(ch["dH"]), B)
    assert dec["pads"] and ok
    for k in ("h", "y", "dH"):
        assert torch.equal(dec[k], ch[k]), k
    return ch, dec, L.decode_grad(L.encode_grad(ch["dW"], ch["db"], ch["dgw"], ch["dgb"]))


@pytest.mark.parametrize("H,W,B,kind", L.value_cases())
def test_every_control_misses_its_bound(H, W, B, kind):
    case, tensors, lay = L.tower_case(H, W, B, kind), L.tower_params(), L.Layout(H, W)
    ch, dec, grads = dumps_of_the_chain(case, tensors, lay)
    smallest, fails, n = float("inf"), [], 0
    for chk in L.checks(dec, case, tensors):
        if B <= 600:                                        # the chain itself passes (the gradient buffer is float32)
            own = chk.excess(L.got_of(chk.name, dec, grads))
            assert own <= 1.0, (chk.name, own)
        for what, wrong in chk.controls:
            margin = chk.excess(wrong, L.LAST) if chk.kind == "elem" else chk.excess(wrong)
            n += 1
            smallest = min(smallest, margin)
            if not margin >= L.MARGIN:
                fails.append((chk.name, what, margin, chk.F))
    print(f"LAYERCTL {H}x{W} B={B} {kind}: {n} controls, the smallest miss is a factor of {smallest:.1f}")
    assert n >= 8 * (2 + 1 + 2 + 3) + 6 * 2 * 2 and not fails, fails
