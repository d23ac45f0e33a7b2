"""The actor's head after the convolutional tower (MAPPOAgent.actor_head) on the project's own kernels: the first linear layer
(csrc/pmx_actor_head.hip) and the LayerNorm - GELU - Linear tail (csrc/pmx_heads.hip), as torch.autograd.Functions."""
import ctypes as C

import torch

from . import _lib, partial_rows
from .partial_rows import row0

# row 0 of the tail's partial-row gradient buffer as (offset, numel), in the order backward returns the gradients: dLN.weight,
# dLN.bias, dW2, db2 (the comment above PMX_ACTOR_TAIL_GRAD_FLOATS in include/pmx.h)
_ACTOR_TAIL_SLICES = ((2568, 512), (3080, 512), (0, 2560), (2560, 5))


def actor_head_sizes(H, W, B):
    """-> (pack bytes, scratch bytes) of the first actor-head layer's kernels for B samples (pmx_actor_head_sizes)"""
    pk, sc = C.c_int64(), C.c_int64()
    _lib.call("pmx_actor_head_sizes", int(H), int(W), int(B), C.byref(pk), C.byref(sc))
    return pk.value, sc.value


def pack_actor_head(w, H, W):
    """The bfloat16 operand images of actor_head[0].weight (float32 [512, 32 H W], nn.Linear's own order): one kernel, one rounding."""
    wf = w.detach().contiguous()
    pack = torch.empty(actor_head_sizes(H, W, 0)[0], dtype=torch.uint8, device=wf.device)
    _lib.call("pmx_actor_head_pack", wf.data_ptr(), pack.data_ptr(), int(H), int(W), _lib.stream(wf.device))
    return pack


class _ActorHead(torch.autograd.Function):
    """h [B, 512] bf16 = Linear(32 H W -> 512)(features) on the tower's channels-last features [B, H*W, 32] bf16, through
    pmx_actor_head_forward / _backward (csrc/pmx_actor_head.hip): the weight is read in nn.Linear's (channel, cell) order and packed
    cell-major by one kernel (no permuted copy of it or of its gradient), the weight and bias gradients come back float32 in the
    parameters' own order.  `pack`: the packed weight of a caller that knows it is frozen (inference), else None."""

    @staticmethod
    def forward(ctx, feat, w, b, H, W, pack):
        feat = feat.contiguous()
        B, dev = feat.shape[0], feat.device
        if pack is None:
            pack = pack_actor_head(w, H, W)
        bf = b.detach().contiguous()
        h = torch.empty(B, 512, dtype=torch.bfloat16, device=dev)
        # scratch belongs to THIS call (see actor_tower._ActorTower.backward)
        scratch = torch.empty(actor_head_sizes(H, W, B)[1], dtype=torch.uint8, device=dev)
        _lib.call("pmx_actor_head_forward", feat.data_ptr(), pack.data_ptr(), bf.data_ptr(), h.data_ptr(), scratch.data_ptr(), B, H, W,
                  _lib.stream(dev))
        ctx.save_for_backward(feat, pack)
        ctx.board = (H, W)
        ctx.dtypes = (w.dtype, b.dtype)
        return h

    @staticmethod
    def backward(ctx, dh):
        feat, pack = ctx.saved_tensors
        H, W = ctx.board
        B, dev = feat.shape[0], feat.device
        dh = dh.to(torch.bfloat16).contiguous()
        dfeat = torch.empty_like(feat)
        alloc = torch.zeros if B == 0 else torch.empty                    # (an empty batch launches nothing)
        dw = alloc(512, 32 * H * W, dtype=torch.float32, device=dev)
        db = alloc(512, dtype=torch.float32, device=dev)
        scratch = torch.empty(actor_head_sizes(H, W, B)[1], dtype=torch.uint8, device=dev)
        _lib.call("pmx_actor_head_backward", feat.data_ptr(), dh.data_ptr(), pack.data_ptr(), dfeat.data_ptr(), dw.data_ptr(), db.data_ptr(),
                  scratch.data_ptr(), B, H, W, _lib.stream(dev))
        return dfeat, dw.to(ctx.dtypes[0]), db.to(ctx.dtypes[1]), None, None, None


class _ActorTail(torch.autograd.Function):
    """logits = Linear_5(gelu(LayerNorm_512(h))) through pmx_actor_tail_forward / _backward (csrc/pmx_heads.hip): one launch each
    way (+ a row sum) instead of LayerNorm, GELU, a skinny GEMM, their backward kernels, two bias reductions and the casts."""

    @staticmethod
    def forward(ctx, h, lnw, lnb, w2, b2, eps):
        h = h.contiguous()
        B = h.shape[0]
        logits = torch.empty(B, 5, dtype=torch.float32, device=h.device)
        stats = torch.empty(B, 2, dtype=torch.float32, device=h.device)
        _lib.call("pmx_actor_tail_forward", h.data_ptr(), 1 if h.dtype == torch.bfloat16 else 0, lnw.data_ptr(), lnb.data_ptr(), w2.data_ptr(),
                  b2.data_ptr(), logits.data_ptr(), stats.data_ptr(), B, float(eps), _lib.stream(h.device))
        ctx.save_for_backward(h, stats, lnw, lnb, w2)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        h, stats, lnw, lnb, w2 = ctx.saved_tensors
        B = h.shape[0]
        dlogits = dlogits.float().contiguous()
        dh = torch.empty_like(h)
        G = _lib.ACTOR_TAIL_GRAD_FLOATS
        grad = partial_rows.buffer(_lib.HEADS_PARTIAL_ROWS, G, h.device)
        (dlnw, dlnb, dw2, db2), wanted = row0(grad, _ACTOR_TAIL_SLICES, ctx.needs_input_grad[1:5])
        with partial_rows.OWNER.defer(_lib.load(), grad, G, wanted, family="pmx_actor_tail"):
            _lib.call("pmx_actor_tail_backward", h.data_ptr(), 1 if h.dtype == torch.bfloat16 else 0, stats.data_ptr(), dlogits.data_ptr(),
                      lnw.data_ptr(), lnb.data_ptr(), w2.data_ptr(), dh.data_ptr(), grad.data_ptr(), B, _lib.stream(h.device))
        return dh, dlnw, dlnb, dw2.view(5, 512), db2, None
