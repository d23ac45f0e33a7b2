"""The fused actor tower (csrc/pmx_actor.hip) LAYER BY LAYER, from the tensors the kernels themselves save: one training forward
and one backward through the C ABI per case, `save` and `scratch` decoded (tests/_tower_layers_ref.py) and every layer's h, GroupNorm
statistics, y, dH, dW, dbias, dGN.weight and dGN.bias held against a float64 reference that starts from the kernel's own input to
that layer.  An 8-layer bfloat16 network amplifies one flipped rounding, so the end-to-end tests (tests/test_gpu_actor_tower.py,
tests/test_gpu_any_board.py) cannot be tighter than 3e-2 on a gradient; cut into layers, every element of every dump is held to half
a bfloat16 step plus what the named upstream roundings may move it by, and the weight and bias gradients -- pure float32 sums of
products of the dumped bfloat16 values -- to float32 accuracy.  Bounds, slack, controls and cases: see tests/_tower_layers_ref.py;
tests/test_tower_layers_cpu.py holds the references to float64 autograd and every control to a threefold miss.

Cases (the smallest that reach each path of `launch_fwd` and `launch_bwd`): 11 x 14 (bucket 11) at B = 1, 2, 3, 7, 8, 9 (4-wave split
kernels, partial blocks), 511, 512, 513 (the 2-wave split forward, the one-wave data kernel from 513), 1536, 1537 (the one-wave
forward), 2048, 2049 (the `cu_count * 2`-block cap of the one-wave kernels: a second trip; test_past_the_grid_cap_of_this_device
adds the B past the cap of a device with another CU count), 4095, 4096, 4097 (the two-wave data kernel and its 1 024-block cap; the
weight kernel at 2, 3, 9, 16, 17 samples per wave, ragged and not); 7 x 20 (bucket 10) and 16 x 14 (bucket 16) at 5, 513, 2049;
13 x 18, 18 x 30, 32 x 20 (buckets 28, 36, 44: 4 and 8 waves per sample, the pair-of-waves weight kernel) at 1, 2, 3, 5, 257; 16 x 32 at
1 025 and 2 049, where the blocks of both passes walk a second sample.  uint8 and bfloat16 planes up to 513, float32 at B = 5, uint8
alone above; the dfeat kinds `quarter_zero` and `one_cell` at 5, 513, 4 097 on 11 x 14 and at 5 on one board per other bucket.  Every
case checks all samples: the float64 reference runs on the GPU in sample chunks (B = 4 097 takes about two seconds).

Every case also requires: save and scratch cut to exactly pmx_actor_sizes between canary bands and prefilled with NaN bytes, every
element of the dumps written, pads exactly zero; the features equal to the decoded y of the last layer and bit-identical to the
inference forward's (`save == NULL`); the gradient buffer NaN-prefilled and finite afterwards; every negative control of the
reference failing its bound.

Measured on an MI355X (the `LAYERFIG` lines of this file): 89 tests in 25 s, the slowest 1.9 s (16 x 32, B = 2 049), B = 4 097 on
11 x 14 in 1.2 s.  Worst share of its bound per output: h, y 1.000; dH 0.99; dW 0.54; dbias 0.31; dGN.weight 0.29; dGN.bias 0.27; rstd
0.26; mean 0.05 (cases and the measured F in tests/_tower_layers_ref.py).  No kernel bug was found.

Mutation check (scratch copies, not committed; this file plus the tower tests of tests/test_gpu_actor_tower.py and
tests/test_gpu_any_board.py on each):
  * the weight kernel drops the last sample of wave 3 of chunk 0: 24 cases of this file fail, every one on the 10 / 11-tile boards
    with B >= 7 (dW of all 8 layers, 1e4 to 1e6 times the bound); of the existing tests three fail as well
    (test_tower_backward_matches_autograd at smallCapture 515 and tinyCapture 96, and the smallCapture sum-over-parts test);
  * `vm` zeroed for the last valid cell in pass 2 of the one-wave data kernel: the 12 cases of this file that run that kernel fail
    (B = 513 .. 4 095 on 11 x 14 and 7 x 20; dH of every layer 90 to 270 times the bound); of the existing tests one fails
    (test_tower_backward_matches_autograd[smallCapture-515]);
  * the unrounded dh summed into dbias (both data kernels): all 88 parametrised cases of this file fail (dbias 1e3 to 8e3 times the
    bound); every existing tower test still passes."""
import ctypes as C

import pytest
import torch

import _tower_layers_ref as L

pytestmark = pytest.mark.gpu

CANARY, NAN_BYTE, GUARD = 0x5A, 0xFF, 1 << 16
DTYPES = {"uint8": torch.uint8, "bfloat16": torch.bfloat16, "float32": torch.float32}
KINDS = ("h", "mean", "rstd", "y", "dH", "dgw", "dgb", "db", "dW")


def _banded(n):
    buf = torch.full((GUARD + n + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + n] = NAN_BYTE
    return buf


def _bands_intact(buf, n):
    return bool((buf[:GUARD] == CANARY).all()) and bool((buf[GUARD + n:] == CANARY).all())


def run_kernels(case, tensors, dtype):
    """One training forward, one inference forward and one backward through the C ABI -> (save, scratch, features, gradient)"""
    from pmx import _lib, actor_tower
    lib = _lib.load()
    B, _, H, W = case["obs"].shape
    lay = L.Layout(H, W)
    sv, sc, si = actor_tower._sizes(H, W, B)
    assert sv == lay.save_bytes(B) and sc >= lay.dh_bytes(B)
    pack = actor_tower.pack_params([t.cuda() for t in tensors])
    obs = case["obs"].cuda().to(dtype).contiguous()
    dfeat = case["dfeat"].cuda().contiguous()
    save, scratch, infer = _banded(sv), _banded(sc), _banded(si)
    feat = torch.full((B, H * W, 32), float("nan"), dtype=torch.bfloat16, device="cuda")
    feat_i = torch.full_like(feat, float("nan"))
    grad = torch.full((_lib.ACTOR_GRAD_FLOATS,), float("nan"), dtype=torch.float32, device="cuda")
    assert _lib.ACTOR_GRAD_FLOATS == L.GRAD_FLOATS
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    code = actor_tower._OBS_CODE[dtype]
    ptr = lambda b: b.data_ptr() + GUARD
    _lib.check(lib.pmx_actor_forward(obs.data_ptr(), code, pack.data_ptr(), feat.data_ptr(), ptr(save), None, B, H, W, st), "training forward")
    _lib.check(lib.pmx_actor_forward(obs.data_ptr(), code, pack.data_ptr(), feat_i.data_ptr(), None, ptr(infer), B, H, W, st), "inference forward")
    _lib.check(lib.pmx_actor_backward(obs.data_ptr(), code, pack.data_ptr(), ptr(save), dfeat.data_ptr(), ptr(scratch), grad.data_ptr(), B, H, W, st),
               "backward")
    torch.cuda.synchronize()
    for name, buf, n in (("save", save, sv), ("scratch", scratch, sc), ("inference scratch", infer, si)):
        assert _bands_intact(buf, n), f"written outside {name}"
    assert torch.equal(feat.view(torch.int16), feat_i.view(torch.int16)), "training and inference forward differ"
    assert bool(torch.isfinite(grad).all()), "the gradient buffer is not fully written"
    return save[GUARD:GUARD + sv], scratch[GUARD:GUARD + sc], feat, grad


def check_case(H, W, B, kind, tname):
    case, tensors = L.tower_case(H, W, B, kind), L.tower_params()
    save, scratch, feat, grad = run_kernels(case, tensors, DTYPES[tname])
    lay = L.Layout(H, W).to("cuda")
    dec = lay.decode_save(save, B)
    dec["dH"], dh_pads = lay.decode_dh(scratch, B)
    assert dec["pads"], "a pad position of the h or y dumps is not zero (or not written)"
    assert dh_pads, "a pad position of the dH dumps is not zero (or not written)"
    for k in ("h", "y", "dH", "mean", "rstd"):
        assert bool(torch.isfinite(dec[k]).all()), f"{k}: not fully written"
    assert torch.equal(feat.double().transpose(1, 2).reshape(B, 32, H, W), dec["y"][7]), "the features are not the last layer's y"
    grads = L.decode_grad(grad)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    worst, fmax, fails, passed_controls = {k: 0.0 for k in KINDS}, {k: 0.0 for k in KINDS}, [], []
    for chk in L.checks(dec, case, tensors, "cuda", cus=cus):
        k = chk.name[:-1]
        e = chk.excess(L.got_of(chk.name, dec, grads))
        worst[k], fmax[k] = max(worst[k], e), max(fmax[k], chk.F)
        if not e <= 1.0:
            fails.append((chk.name, e, chk.F))
        for what, wrong in chk.controls:
            if not (chk.excess(wrong, L.LAST) if chk.kind == "elem" else chk.excess(wrong)) > 1.0:
                passed_controls.append((chk.name, what))
    print(f"LAYERFIG {H}x{W} B={B} {kind} {tname}: excess " + " ".join(f"{k} {worst[k]:.3f}" for k in KINDS)
          + " | F " + " ".join(f"{k} {fmax[k]:.2e}" for k in KINDS))
    assert not fails, fails
    assert not passed_controls, passed_controls


@pytest.mark.parametrize("H,W,B,kind,tname", L.cases())
def test_every_layer_from_the_kernels_own_dumps(H, W, B, kind, tname):
    check_case(H, W, B, kind, tname)


def test_past_the_grid_cap_of_this_device():
    """The one-wave kernels launch at most cu_count * 2 blocks of 4 samples: on 256 CUs B = 2 049 of the table takes the second trip;
    on a device with another CU count this adds the B just past ITS cap."""
    cap = torch.cuda.get_device_properties(0).multi_processor_count * 2 * 4
    assert cap > 1536
    if cap + 1 not in L.SMALL_SIZES:
        check_case(*L.SMALL_BOARD, cap + 1, "normal", "uint8")
