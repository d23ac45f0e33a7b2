"""tests/_head_ref.py against torch's own float64 Linear on nn.Flatten's order, and the host-only size query of the first actor-head
layer's kernels (pmx_actor_head_sizes, csrc/pmx_actor_head.hip).  No GPU."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import _head_ref as R


def _case(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    planes = torch.randn(B, 32, H, W, generator=g).to(torch.bfloat16).double()          # what the tower computes, in nn.Flatten's layout
    w = (0.05 * torch.randn(512, 32 * H * W, generator=g)).to(torch.bfloat16).float()   # already bfloat16 values: the rounding is exact
    bias = torch.randn(512, generator=g).float()
    dh = torch.randn(B, 512, generator=g).to(torch.bfloat16).double()
    return planes, w, bias, dh


@pytest.mark.parametrize("B,H,W", [(3, 3, 8), (5, 5, 9), (2, 11, 14)])
def test_reference_equals_float64_linear_on_flatten(B, H, W):
    planes, w, bias, dh = _case(B, H, W, 17 * H + W)
    x = planes.clone().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), bias.double().requires_grad_(True)
    h = F.linear(x.flatten(1), wd, bd)
    dx, dw, db = torch.autograd.grad((h * dh).sum(), [x, wd, bd])
    h = h.detach()
    feat = planes.permute(0, 2, 3, 1).reshape(B, H * W, 32)                              # [B][cell][ch]: the fused tower's output layout
    got_h, bound_h = R.forward(feat, w, bias)
    back = R.backward(feat, dh, w)
    tol = 1e-12
    assert float((got_h - h).abs().max()) <= tol * (1 + float(h.abs().max()))
    assert float((back["dfeat"][0] - dx.permute(0, 2, 3, 1).reshape(B, H * W, 32)).abs().max()) <= tol * (1 + float(dx.abs().max()))
    assert float((back["dw"][0] - dw).abs().max()) <= tol * (1 + float(dw.abs().max()))
    assert float((back["db"][0] - db).abs().max()) <= tol * (1 + float(db.abs().max()))
    assert float(bound_h.min()) > 0 and all(float(b.min()) >= 0 for _, b in back.values())


def test_index_maps_are_inverse_and_not_the_identity():
    HW = 15
    w = torch.arange(4 * 32 * HW, dtype=torch.float64).reshape(4, 32 * HW)
    wc = R.to_cell_major(w, HW)
    assert torch.equal(R.to_param_order(wc, HW), w) and not torch.equal(wc, w)
    assert float(wc[1, 7 * 32 + 5]) == float(w[1, 5 * HW + 7])


def test_negative_controls_change_the_reference():
    planes, w, bias, dh = _case(4, 3, 8, 5)
    feat = planes.permute(0, 2, 3, 1).reshape(4, 24, 32)
    h = R.forward(feat, w, bias)[0]
    assert not torch.equal(R.forward(feat, w, bias, drop_cell=23)[0], h)
    back = R.backward(feat, dh, w)
    assert not torch.equal(R.backward(feat, dh, w, drop_cell=23)["dw"][0], back["dw"][0])
    assert not torch.equal(R.backward(feat, dh, w, drop_sample=3)["db"][0], back["db"][0])
    assert not torch.equal(R.backward(feat, dh, w, wrong_order=True)["dw"][0], back["dw"][0])
    assert not torch.equal(R.backward(feat, dh, w, drop_hidden=511)["dfeat"][0], back["dfeat"][0])


def _sizes(lib, H, W, B):
    pk, sc = C.c_int64(-1), C.c_int64(-1)
    rc = lib.pmx_actor_head_sizes(H, W, B, C.byref(pk), C.byref(sc))
    return rc, pk.value, sc.value


def test_sizes_are_positive_and_monotone_in_the_batch():
    from pmx import _lib
    lib = _lib.load()
    batches = [1, 2, 3, 63, 64, 65, 127, 128, 129, 130, 255, 256, 257, 511, 512, 700, 1023, 1024, 1025, 2047, 2048, 4095, 4096, 4097, 8191, 8192,
               8193, 16383, 16384, 16385, 32768, 65536]
    for H, W in [(3, 8), (5, 9), (11, 14), (20, 20), (20, 32), (32, 20), (3, 32)]:
        K = 32 * H * W
        prev = 0
        for B in batches:
            rc, pk, sc = _sizes(lib, H, W, B)
            assert rc == 0 and pk > 0 and sc > 0, (H, W, B)
            assert pk >= 2 * 2 * 512 * K and pk % 16 == 0 and sc % 16 == 0        # two bfloat16 images of the weight at least
            assert sc >= prev, (H, W, B)
            prev = sc
        assert _sizes(lib, H, W, 1)[1] == _sizes(lib, H, W, 65536)[1]              # the pack does not depend on the batch


def test_sizes_outside_the_domain():
    from pmx import _lib
    lib = _lib.load()
    assert _sizes(lib, 26, 26, 64)[0] == -2          # PMX_ERR_UNSUPPORTED: 676 cells
    assert _sizes(lib, 11, 7, 64)[0] == -2           # W = 7
    assert _sizes(lib, 2, 14, 64)[0] == -2
    assert _sizes(lib, 11, 14, -1)[0] == -1          # PMX_ERR_INVALID
    assert lib.pmx_actor_head_sizes(11, 14, 64, None, None) == 0
    assert _sizes(lib, 11, 14, 1 << 22)[0] == 0 and _sizes(lib, 11, 14, (1 << 22) + 1)[0] == -2      # PMX_ACTOR_HEAD_MAX_BATCH


def test_model_threshold_decides_who_runs_the_layer():
    """MAPPOAgent.head_kernels_for: the class default keeps the library at every batch; a raised threshold hands the kernels every
    training batch up to it on a supported board, and nothing with fused_head off."""
    from pmx import mappo
    m = mappo.MAPPOAgent((8, 11, 14))
    assert mappo.MAPPOAgent.fused_head_max_batch == 0 and not m.head_kernels_for(512) and not m.head_kernels_for(1)
    m.fused_head_max_batch = 512
    assert m.head_kernels_for(512) and m.head_kernels_for(1) and not m.head_kernels_for(513) and not m.head_kernels_for(None)
    m.fused_head = False
    assert not m.head_kernels_for(64)
