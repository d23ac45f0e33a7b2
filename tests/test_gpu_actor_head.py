"""The first actor-head layer's kernels (csrc/pmx_actor_head.hip: pmx_actor_head_pack / _forward / _backward) through the C ABI,
per ELEMENT against the float64 reference of tests/_head_ref.py, and the model-level path that uses them (actor_head._ActorHead,
MAPPOAgent.fused_head, PPOLearner).

Bounds (derived in tests/_head_ref.py, none tuned): an output that adds n terms a_k b_k in float32 lies within
n * 2**-24 * sum |a_k b_k| of the float64 sum in any summation order; h and dfeat, stored as bfloat16, add 2**-8 |ref|.  n is
32 H W + 1 for h (the bias is one more term), 512 for dfeat, B for dw and db.  Both sums come from the reference in float64.

Data.  Features N(0, 1) rounded to bfloat16 with ONE hot cell scaled by 16 (the cell the negative control drops: on the largest
boards the worst-case float32 bound of a 20 480-term sum is wider than what 32 ordinary terms contribute, so the dropped cell is
made to matter), a float32 weight that is NOT bfloat16-representable (the pack kernel's rounding is part of the test), dh N(0, 1).
The exact case uses integers of magnitude <= 2: every partial sum stays below 2**24, so float32 is exact whatever the order and an
index error has no tolerance to hide in.

The launchers cap no grid (one block per tile / slab / quad), so there is no batch "one tile past the cap" to add."""
import ctypes as C
import functools

import pytest
import torch

import _head_ref as R

pytestmark = pytest.mark.gpu

SMALL_BOARDS, SMALL_BATCHES = [(3, 8), (5, 9), (11, 14)], [1, 3, 129, 700]
LARGE_BOARDS, LARGE_BATCHES = [(20, 20), (20, 32)], [1, 130]
CASES = [(H, W, B) for H, W in SMALL_BOARDS for B in SMALL_BATCHES] + [(H, W, B) for H, W in LARGE_BOARDS for B in LARGE_BATCHES]
BAND, CANARY, NAN_BYTE = 256, 0xA5, 0xFF          # 0xFFFF is a bfloat16 NaN, 0xFFFFFFFF a float32 NaN
OK, INVALID, UNSUPPORTED = 0, -1, -2


def _libs():
    from pmx import _lib
    return _lib, _lib.load()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _hot_cell(H, W):
    return (H * W) // 2


class _Banded:
    """nbytes of payload (prefilled with NaN bytes) between two canary bands"""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.full((2 * BAND + self.n,), CANARY, dtype=torch.uint8, device="cuda")
        self.buf[BAND:BAND + self.n] = NAN_BYTE

    @property
    def ptr(self):
        return self.buf.data_ptr() + BAND

    def view(self, dtype, shape):
        return self.buf[BAND:BAND + self.n].view(dtype).view(shape)

    def intact(self):
        return bool((self.buf[:BAND] == CANARY).all()) and bool((self.buf[BAND + self.n:] == CANARY).all())


@functools.lru_cache(maxsize=None)
def _data(H, W, B, exact):
    g = torch.Generator(device="cuda").manual_seed(1000 * H + 10 * W + B + (7 if exact else 0))
    HW, K = H * W, 32 * H * W
    if exact:
        ri = lambda *s: torch.randint(-2, 3, s, generator=g, device="cuda")
        return ri(B, HW, 32).to(torch.bfloat16), ri(512, K).float(), ri(512).float(), ri(B, 512).to(torch.bfloat16)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    feat = rn(B, HW, 32)
    feat[:, _hot_cell(H, W), :] *= 16
    return feat.to(torch.bfloat16), 0.05 * rn(512, K), rn(512), rn(B, 512).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _run(H, W, B, exact=False):
    """pack + forward + backward, twice, into NaN-prefilled buffers between canary bands -> outputs of both runs and the band check"""
    _lib, lib = _libs()
    feat, w, bias, dh = _data(H, W, B, exact)
    K = 32 * H * W
    pk, sc = C.c_int64(), C.c_int64()
    assert lib.pmx_actor_head_sizes(H, W, B, C.byref(pk), C.byref(sc)) == OK
    runs, intact = [], True
    for _ in range(2):
        pack, scratch_f, scratch_b = _Banded(pk.value), _Banded(sc.value), _Banded(sc.value)
        h, dfeat, dw, db = _Banded(B * 512 * 2), _Banded(B * K * 2), _Banded(512 * K * 4), _Banded(512 * 4)
        _lib.check(lib.pmx_actor_head_pack(w.data_ptr(), pack.ptr, H, W, _st()), "pack")
        _lib.check(lib.pmx_actor_head_forward(feat.data_ptr(), pack.ptr, bias.data_ptr(), h.ptr, scratch_f.ptr, B, H, W, _st()), "forward")
        _lib.check(lib.pmx_actor_head_backward(feat.data_ptr(), dh.data_ptr(), pack.ptr, dfeat.ptr, dw.ptr, db.ptr, scratch_b.ptr, B, H, W, _st()),
                   "backward")
        torch.cuda.synchronize()
        intact = intact and all(b.intact() for b in (pack, scratch_f, scratch_b, h, dfeat, dw, db))
        runs.append({"h": h.view(torch.bfloat16, (B, 512)).clone(), "dfeat": dfeat.view(torch.bfloat16, (B, H * W, 32)).clone(),
                     "dw": dw.view(torch.float32, (512, K)).clone(), "db": db.view(torch.float32, (512,)).clone()})
    return runs, intact


def _check(name, got, ref, bound, case):
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name} {case}: max |got - ref| / bound = {ratio:.3f}")
    assert bool((err <= bound).all()), (name, case, ratio)


def _must_fail(name, got, ref, bound, case):
    assert bool(((got.double() - ref).abs() > bound).any()), f"negative control '{name}' passed the bound at {case}"


@pytest.mark.parametrize("H,W,B", CASES)
def test_forward_within_the_summation_bound(H, W, B):
    feat, w, bias, _ = _data(H, W, B, False)
    got = _run(H, W, B)[0][0]["h"]
    ref, bound = R.forward(feat, w, bias)
    _check("h", got, ref, R.bf16_bound(ref, bound), (H, W, B))
    ref_c, bound_c = R.forward(feat, w, bias, drop_cell=_hot_cell(H, W))
    _must_fail("a cell of feat dropped", got, ref_c, R.bf16_bound(ref_c, bound_c), (H, W, B))


@pytest.mark.parametrize("H,W,B", CASES)
def test_backward_within_the_summation_bound(H, W, B):
    feat, w, _, dh = _data(H, W, B, False)
    got = _run(H, W, B)[0][0]
    ref = R.backward(feat, dh, w)
    _check("dfeat", got["dfeat"], ref["dfeat"][0], R.bf16_bound(*ref["dfeat"]), (H, W, B))
    _check("dw", got["dw"], *ref["dw"], (H, W, B))
    _check("db", got["db"], *ref["db"], (H, W, B))
    c = R.backward(feat, dh, w, drop_cell=_hot_cell(H, W))
    _must_fail("a cell of feat dropped (dw)", got["dw"], *c["dw"], (H, W, B))
    c = R.backward(feat, dh, w, drop_sample=B - 1)
    _must_fail("a sample dropped (dw)", got["dw"], *c["dw"], (H, W, B))
    _must_fail("a sample dropped (db)", got["db"], *c["db"], (H, W, B))
    c = R.backward(feat, dh, w, wrong_order=True)
    _must_fail("dw in (cell, channel) order", got["dw"], *c["dw"], (H, W, B))
    c = R.backward(feat, dh, w, drop_hidden=511)
    _must_fail("a hidden unit dropped (dfeat)", got["dfeat"], c["dfeat"][0], R.bf16_bound(*c["dfeat"]), (H, W, B))


@pytest.mark.parametrize("H,W,B", CASES)
def test_small_integers_are_exact(H, W, B):
    feat, w, bias, dh = _data(H, W, B, True)
    runs, intact = _run(H, W, B, True)
    got = runs[0]
    h, _ = R.forward(feat, w, bias)
    back = R.backward(feat, dh, w)
    assert float(h.abs().max()) < 2 ** 24 and float(back["dw"][0].abs().max()) < 2 ** 24
    assert torch.equal(got["dw"].double(), back["dw"][0]), "dw differs from the exact integer result"
    assert torch.equal(got["db"].double(), back["db"][0]), "db differs from the exact integer result"
    assert torch.equal(got["h"].double(), R.bf16(h)), "h is not the bfloat16 rounding of the exact result"
    assert torch.equal(got["dfeat"].double(), R.bf16(back["dfeat"][0])), "dfeat is not the bfloat16 rounding of the exact result"
    assert intact


@pytest.mark.parametrize("H,W,B", CASES)
def test_outputs_are_written_in_full_bands_stay_and_runs_repeat(H, W, B):
    runs, intact = _run(H, W, B)
    assert intact, "a canary band around the pack, the scratch or an output was written"
    for name, t in runs[0].items():
        assert not bool(torch.isnan(t.float()).any()), f"{name} keeps NaN prefill: not written in full"
        assert torch.equal(t.view(torch.uint8), runs[1][name].view(torch.uint8)), f"{name}: two runs differ"


def test_empty_batch_null_pointers_and_unsupported_boards():
    _lib, lib = _libs()
    H, W, B = 5, 9, 3
    feat, w, bias, dh = _data(H, W, B, False)
    K = 32 * H * W
    pk, sc = C.c_int64(), C.c_int64()
    assert lib.pmx_actor_head_sizes(H, W, B, C.byref(pk), C.byref(sc)) == OK
    pack, scratch = _Banded(pk.value), _Banded(sc.value)
    h, dfeat, dw, db = _Banded(B * 512 * 2), _Banded(B * K * 2), _Banded(512 * K * 4), _Banded(512 * 4)
    assert lib.pmx_actor_head_pack(w.data_ptr(), pack.ptr, H, W, _st()) == OK
    fwd = [feat.data_ptr(), pack.ptr, bias.data_ptr(), h.ptr, scratch.ptr]
    bwd = [feat.data_ptr(), dh.data_ptr(), pack.ptr, dfeat.ptr, dw.ptr, db.ptr, scratch.ptr]
    # B = 0: success, nothing written (every output still holds its NaN prefill)
    assert lib.pmx_actor_head_forward(*fwd, 0, H, W, _st()) == OK
    assert lib.pmx_actor_head_backward(*bwd, 0, H, W, _st()) == OK
    torch.cuda.synchronize()
    for b in (h, dfeat, dw, db, scratch):
        assert bool((b.buf[BAND:BAND + b.n] == NAN_BYTE).all()) and b.intact()
    assert lib.pmx_actor_head_forward(*fwd, -1, H, W, _st()) == INVALID
    assert lib.pmx_actor_head_backward(*bwd, -1, H, W, _st()) == INVALID
    for i in range(len(fwd)):
        a = list(fwd)
        a[i] = None
        assert lib.pmx_actor_head_forward(*a, B, H, W, _st()) == INVALID, i
    for i in range(len(bwd)):
        a = list(bwd)
        a[i] = None
        assert lib.pmx_actor_head_backward(*a, B, H, W, _st()) == INVALID, i
    assert lib.pmx_actor_head_pack(None, pack.ptr, H, W, _st()) == INVALID
    assert lib.pmx_actor_head_pack(w.data_ptr(), None, H, W, _st()) == INVALID
    for Hb, Wb in [(26, 26), (11, 7), (2, 14)]:
        assert lib.pmx_actor_head_pack(w.data_ptr(), pack.ptr, Hb, Wb, _st()) == UNSUPPORTED
        assert lib.pmx_actor_head_forward(*fwd, B, Hb, Wb, _st()) == UNSUPPORTED
        assert lib.pmx_actor_head_backward(*bwd, B, Hb, Wb, _st()) == UNSUPPORTED
    torch.cuda.synchronize()
    for b in (h, dfeat, dw, db):
        assert bool((b.buf[BAND:BAND + b.n] == NAN_BYTE).all()) and b.intact()


# ---------------------------------------------------------------------------------------------------------------
# Model level: bf16 autocast, byte planes, the same weights on both paths
# ---------------------------------------------------------------------------------------------------------------
def _model(H, W, seed):
    from pmx import mappo
    torch.manual_seed(seed)
    return mappo.MAPPOAgent((8, H, W)).cuda()


def _tail(m, h):
    from pmx import actor_head
    ln, out = m.actor_head[1], m.actor_head[3]
    return actor_head._ActorTail.apply(h, ln.weight, ln.bias, out.weight, out.bias, ln.eps)


@pytest.mark.parametrize("H,W,B", [(11, 14, 64), (5, 9, 37)])
def test_wrapper_and_logits_agree_with_the_library_path(H, W, B):
    """h of actor_head._ActorHead against the permuted-weight F.linear it replaces, on the tower's own features: within the project's
    2 bfloat16 ulps of the largest h (2 * 2**-8 max |h|).  MAPPOAgent.logits must then return EXACTLY the tail of that h (the kernels
    are deterministic, so any other operand, pack or tail input shows as a different bit) on each of its kernel branches -- with
    gradients (a pack per call) and without gradients on a frozen head_pack -- and the library path's logits everywhere else:
    fused_head off, no gradients and no frozen pack, a batch above fused_head_max_batch."""
    from pmx import actor_head, actor_tower, mappo
    m = _model(H, W, 3)
    m.fused_head_max_batch = 512         # (the class default keeps the library at every batch: DESIGN.md section 5)
    with torch.no_grad():
        m.actor_head[0].bias.copy_(0.1 * torch.randn(512, device="cuda"))
    obs = (torch.rand(B, 8, H, W, device="cuda") < 0.2).to(torch.uint8)
    lin, HW = m.actor_head[0], H * W
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        with torch.no_grad():
            feat = actor_tower.actor_tower(m.actor_backbone, obs)
            h_new = actor_head._ActorHead.apply(feat, lin.weight, lin.bias, H, W, None)
            wperm = lin.weight.view(512, 32, HW).permute(0, 2, 1).reshape(512, HW * 32)
            h_lib = torch.nn.functional.linear(feat.reshape(B, HW * 32), wperm, lin.bias)
            want_new, want_lib = _tail(m, h_new), _tail(m, h_lib)
            m.fused_head = False
            assert torch.equal(m.logits(obs), want_lib)
            m.fused_head = True
            assert torch.equal(m.logits(obs), want_lib), "no gradients, no frozen pack: the library path"
            m.head_pack = mappo.pack_actor_head(lin.weight, H, W)
            assert torch.equal(m.logits(obs), want_new), "no gradients, frozen pack: the kernels on that pack"
            m.fused_head_max_batch = B - 1
            assert torch.equal(m.logits(obs), want_lib), "above the threshold: the library path"
            m.fused_head_max_batch, m.head_pack = B, None
        lg = m.logits(obs)                                   # with gradients: a pack per call
        assert lg.requires_grad and torch.equal(lg.detach(), want_new)
    assert h_new.dtype == torch.bfloat16 and h_lib.dtype == torch.bfloat16
    err, top = float((h_new.double() - h_lib.double()).abs().max()), float(h_lib.double().abs().max())
    print(f"h ({H}, {W}, {B}): max |kernel - library| = {err:.3e}, 2 ulps of max |h| = {2 * 2.0 ** -8 * top:.3e}; "
          f"max |logits difference| = {float((want_new - want_lib).abs().max()):.3e}")
    assert err <= 2 * 2.0 ** -8 * top


@pytest.mark.parametrize("max_batch", [None, 0])
def test_learner_gradient_of_the_first_head_layer(max_batch):
    """Through PPOLearner: the flat-gradient slices of actor_head.0.weight / .bias computed by the kernels against the library path's,
    g_rel <= 2e-2 (the figure of test_bf16_shadow_weights_give_the_autocast_step); the layer is not among the bfloat16 shadows
    exactly when the step's batch takes the kernels (with the threshold at 0 it keeps its shadow and the library path)."""
    from pmx import mappo
    H, W, B = 11, 14, 256
    torch.manual_seed(4)
    obs = (torch.rand(B, 8, H, W, device="cuda") < 0.2).to(torch.uint8)
    merged = (torch.rand(B // 2, 8, H, W, device="cuda") < 0.2).to(torch.uint8)
    act = torch.randint(0, 5, (B,), device="cuda")
    old_logp, adv, ret = -torch.rand(B, device="cuda") - 1, torch.randn(B, device="cuda"), torch.randn(B, device="cuda")
    res = {}
    for fused in (True, False):
        m = _model(H, W, 9)
        m.fused_head = fused
        m.fused_head_max_batch = 512 if max_batch is None else max_batch
        L = mappo.PPOLearner(m, autocast_dtype=torch.bfloat16)
        L.update_minibatch(obs, merged, act, old_logp, adv, ret)
        shadowed = [n for _, n in L._shadow_slots]
        kernels = fused and max_batch != 0               # threshold 0: the layer keeps its shadow and the library path
        assert any(n.startswith("actor_head.0.") for n in shadowed) == (not kernels), shadowed
        sl = {}
        for name in ("actor_head.0.weight", "actor_head.0.bias"):
            i = L.bucket.names.index(name)
            sl[name] = L.bucket.grad[L._offsets[i]:L._offsets[i + 1]].clone()
        res[fused] = sl
    for name in res[True]:
        a, b = res[True][name].double(), res[False][name].double()
        g_rel = float((a - b).norm() / b.norm())
        print(f"{name}: g_rel = {g_rel:.3e}")
        assert float(b.norm()) > 0 and g_rel <= 2e-2, (name, g_rel)
