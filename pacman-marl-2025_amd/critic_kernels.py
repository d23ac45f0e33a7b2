"""The critic's hand-written kernels (csrc/pmx_critic.hip, pmx_train.hip, pmx_heads.hip, the projector in pmx_actor.hip) as
torch.autograd.Functions, the functions that choose between them and the library ops, and the parameter packs they read.

The (offset, numel) tables below are the layouts of row 0 of the partial-row gradient buffers, in the order each backward returns
its gradients; they mirror include/pmx.h: the comment at PMX_FFN_GRAD_FLOATS, the tok96 / tok32ln lines above PMX_TOK96_PACK_BYTES
and the critic-tail lines above PMX_HEADS_PARTIAL_ROWS."""
import torch
import torch.nn.functional as F

from . import _lib, actor_tower, partial_rows
from .partial_rows import row0

_FFN_SLICES = ((4096, 4096), (8192, 128), (0, 4096), (8320, 32), (8352, 32), (8384, 32))      # dw1, db1, dw2, db2, dgamma, dbeta
_TOK96_SLICES = ((0, 3072), (3072, 96))                                                        # dw, db
_TOK32_SLICES = ((0, 1024), (1024, 32), (1056, 32), (1088, 32))                                # dw, db, dgamma, dbeta
_CRITIC_TAIL_SLICES = ((0, 16384), (16384, 512), (16896, 512), (17408, 1))                     # dw1, db1, dw2, db2


def _all_f32(dtypes):
    return all(dt == torch.float32 for dt in dtypes)


def layer_norm_small(x, ln):
    """nn.LayerNorm over a SMALL last dimension as var_mean + elementwise ops.  torch's native kernel launches one
    workgroup per row (RowwiseMomentsCUDAKernel): for the critic's [H*W*B, 32] token matrix that is 630 k tiny
    workgroups and 1.7 ms per call on MI355X (45 % of the optimizer step at batch 4096)."""
    xf = x.float()
    var, mean = torch.var_mean(xf, dim=-1, unbiased=False, keepdim=True)
    return ((xf - mean) * torch.rsqrt(var + ln.eps) * ln.weight + ln.bias).to(x.dtype)


class _LN32Residual(torch.autograd.Function):
    """LayerNorm(x + a) over a 32-wide feature dimension through the fused HIP kernels pmx_ln32_forward/backward."""

    @staticmethod
    def forward(ctx, x, a, w, b, eps):
        x, a = x.contiguous(), a.contiguous()
        rows = x.numel() // 32
        y = torch.empty_like(x)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        wf, bf = w.float().contiguous(), b.float().contiguous()
        _lib.call("pmx_ln32_forward", x.data_ptr(), a.data_ptr(), wf.data_ptr(), bf.data_ptr(), y.data_ptr(), mean.data_ptr(),
                  rstd.data_ptr(), rows, float(eps), 0 if x.dtype == torch.float32 else 1, _lib.stream(x.device))
        ctx.save_for_backward(x, a, wf, mean, rstd)
        ctx.wdtype = w.dtype
        return y

    @staticmethod
    def backward(ctx, gy):
        x, a, wf, mean, rstd = ctx.saved_tensors
        gy = gy.contiguous()
        dz = torch.empty_like(x)
        partial = torch.empty(_lib.LN32_PARTIAL_ROWS, 64, dtype=torch.float32, device=x.device)
        _lib.call("pmx_ln32_backward", x.data_ptr(), a.data_ptr(), gy.data_ptr(), wf.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                  dz.data_ptr(), partial.data_ptr(), x.numel() // 32, 0 if x.dtype == torch.float32 else 1, _lib.stream(x.device))
        dwb = partial.sum(0).to(ctx.wdtype)          # gradients carry the dtype of the parameters they belong to
        return dz, dz, dwb[:32], dwb[32:], None


def add_layer_norm_small(x, a, ln):
    """LayerNorm(x + a) for the critic tokens: the fused HIP kernel on the GPU (feature dimension 32, float32 or
    bfloat16), the reduce + elementwise formulation otherwise."""
    if x.is_cuda and x.shape[-1] == 32 and x.dtype == a.dtype and x.dtype in (torch.float32, torch.bfloat16):
        return _LN32Residual.apply(x, a, ln.weight, ln.bias, ln.eps)
    return layer_norm_small(x + a, ln)


def _pack(name, nbytes, *tensors):
    """`tensors` (float32 parameters in nn.Module shapes) in a kernel family's operand layout: the pack function `name` on the
    current stream -> uint8 [nbytes]."""
    ps = [t.detach().float().contiguous() for t in tensors]
    pack = torch.empty(nbytes, dtype=torch.uint8, device=ps[0].device)
    _lib.call(name, *[t.data_ptr() for t in ps], pack.data_ptr(), _lib.stream(ps[0].device))
    return pack


def pack_ffn(w1, b1, w2, b2, gamma, beta):
    """The feed-forward half's parameters in the kernels' operand layout (pmx_ffn_pack), on the current stream."""
    return _pack("pmx_ffn_pack", _lib.FFN_PACK_BYTES, w1, b1, w2, b2, gamma, beta)


def pack_in_proj(w, b):
    return _pack("pmx_tok96_pack", _lib.TOK96_PACK_BYTES, w, b)


def pack_out_proj(w, b, gamma, beta):
    return _pack("pmx_tok32ln_pack", _lib.TOK32_PACK_BYTES, w, b, gamma, beta)


def pack_projector(w, b):
    return _pack("pmx_proj_pack", _lib.PROJ_PACK_BYTES, w, b)


def encoder_packs(layers):
    """The three parameter packs (in-projection, out-projection + norm1, feed-forward + norm2) of every given CriticEncoderLayer in
    ONE launch (pmx_encoder_pack) on the current stream -> [(pack_in, pack_out, pack_ffn), ...]."""
    n = len(layers)
    arr = (_lib.EncoderLayerParams * n)()
    keep, out = [], []
    dev = layers[0].linear1.weight.device
    for i, l in enumerate(layers):
        mha = l.self_attn
        ps = [t.detach().float().contiguous() for t in (mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias,
                                                        l.norm1.weight, l.norm1.bias, l.linear1.weight, l.linear1.bias, l.linear2.weight,
                                                        l.linear2.bias, l.norm2.weight, l.norm2.bias)]
        keep.append(ps)
        packs = tuple(torch.empty(nbytes, dtype=torch.uint8, device=dev)
                      for nbytes in (_lib.TOK96_PACK_BYTES, _lib.TOK32_PACK_BYTES, _lib.FFN_PACK_BYTES))
        for name, t in zip(("in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "norm1_w", "norm1_b", "lin1_w", "lin1_b", "lin2_w", "lin2_b",
                            "norm2_w", "norm2_b"), ps):
            setattr(arr[i], name, t.data_ptr())
        arr[i].pack_in, arr[i].pack_out, arr[i].pack_ffn = (p.data_ptr() for p in packs)
        out.append(packs)
    _lib.call("pmx_encoder_pack", n, arr, _lib.stream(dev))
    return out


class _FFNLayerNorm(torch.autograd.Function):
    """LayerNorm(x + linear2(relu(linear1(x)))) on [..., 32] bfloat16 tokens through pmx_ffn_forward / pmx_ffn_backward
    (csrc/pmx_critic.hip): one kernel each way, the 128-wide hidden activations never reach memory, backward recomputes."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, gamma, beta, eps, pack=None):
        x = x.contiguous()
        if pack is None:
            pack = pack_ffn(w1, b1, w2, b2, gamma, beta)
        y = torch.empty_like(x)
        _lib.call("pmx_ffn_forward", x.data_ptr(), pack.data_ptr(), y.data_ptr(), x.numel() // 32, float(eps), _lib.stream(x.device))
        ctx.save_for_backward(x, pack)
        ctx.eps = float(eps)
        ctx.dtypes = [t.dtype for t in (w1, b1, w2, b2, gamma, beta)]
        return y

    @staticmethod
    def backward(ctx, dy):
        x, pack = ctx.saved_tensors
        dy = dy.to(torch.bfloat16).contiguous()
        dx = torch.empty_like(x)
        grad = partial_rows.buffer(_lib.GRAD_PARTIAL_ROWS, _lib.FFN_GRAD_FLOATS, x.device)
        outs, wanted = row0(grad, _FFN_SLICES, ctx.needs_input_grad[1:7])
        with partial_rows.OWNER.defer(_lib.load(), grad, _lib.FFN_GRAD_FLOATS, wanted, _all_f32(ctx.dtypes), "pmx_ffn"):
            _lib.call("pmx_ffn_backward", x.data_ptr(), dy.data_ptr(), pack.data_ptr(), dx.data_ptr(), grad.data_ptr(), x.numel() // 32,
                      ctx.eps, _lib.stream(x.device))
        outs[0], outs[2] = outs[0].view(128, 32), outs[2].view(32, 128)
        return (dx,) + tuple(o.to(dt) for o, dt in zip(outs, ctx.dtypes)) + (None, None)


def _in_proj96_forward(ctx, a, w, b, pack):
    """The forward of both in-projection functions -> (qkv, the contiguous input it read)."""
    a = a.contiguous()
    if pack is None:
        pack = pack_in_proj(w, b)
    y = torch.empty(a.shape[:-1] + (96,), dtype=torch.bfloat16, device=a.device)
    _lib.call("pmx_tok96_forward", a.data_ptr(), pack.data_ptr(), y.data_ptr(), a.numel() // 32, _lib.stream(a.device))
    ctx.save_for_backward(a, pack)
    ctx.dtypes = (w.dtype, b.dtype)
    return y, a


def _in_proj96_backward_setup(ctx):
    """What both backwards start from -> (a, pack, the partial-row buffer, the not yet entered defer context for the kernel call,
    the row-0 views dw, db)."""
    a, pack = ctx.saved_tensors
    grad = partial_rows.buffer(_lib.GRAD_PARTIAL_ROWS, _lib.TOK96_GRAD_FLOATS, a.device)
    (dw, db), wanted = row0(grad, _TOK96_SLICES, ctx.needs_input_grad[1:3])
    deferred = partial_rows.OWNER.defer(_lib.load(), grad, _lib.TOK96_GRAD_FLOATS, wanted, _all_f32(ctx.dtypes), "pmx_tok96")
    return a, pack, grad, deferred, dw, db


def _in_proj96_grads(ctx, da, dw, db):
    return da, dw.view(96, 32).to(ctx.dtypes[0]), db.to(ctx.dtypes[1]), None


class _InProj96(torch.autograd.Function):
    """qkv = in_proj_weight a + in_proj_bias on [..., 32] bfloat16 tokens (pmx_tok96_forward / _backward)."""

    @staticmethod
    def forward(ctx, a, w, b, pack=None):
        return _in_proj96_forward(ctx, a, w, b, pack)[0]

    @staticmethod
    def backward(ctx, dy):
        a, pack, grad, deferred, dw, db = _in_proj96_backward_setup(ctx)
        dy = dy.to(torch.bfloat16).contiguous()
        da = torch.empty_like(a)
        with deferred:
            _lib.call("pmx_tok96_backward", a.data_ptr(), dy.data_ptr(), pack.data_ptr(), da.data_ptr(), grad.data_ptr(), a.numel() // 32,
                      _lib.stream(a.device))
        return _in_proj96_grads(ctx, da, dw, db)


class _InProj96Res(torch.autograd.Function):
    """_InProj96 that also hands its input back as a second output, `a_res`, for the layer's residual connection: the gradient of
    the residual branch then arrives HERE, and pmx_tok96_backward_res adds it to W^T dy inside the kernel (float32, rounded once)
    instead of autograd adding the two bfloat16 tensors with a launch of its own (one per encoder layer and optimizer step)."""

    @staticmethod
    def forward(ctx, a, w, b, pack=None):
        y, a = _in_proj96_forward(ctx, a, w, b, pack)
        return y, a.view_as(a)

    @staticmethod
    def backward(ctx, dy, dres):
        a, pack, grad, deferred, dw, db = _in_proj96_backward_setup(ctx)
        if dy is None:                                  # only the residual output was used
            grad.zero_()
            return _in_proj96_grads(ctx, dres, dw, db)
        dy = dy.to(torch.bfloat16).contiguous()
        res = None if dres is None else dres.to(torch.bfloat16).contiguous()
        da = torch.empty_like(a)
        with deferred:
            _lib.call("pmx_tok96_backward_res", a.data_ptr(), dy.data_ptr(), pack.data_ptr(), None if res is None else res.data_ptr(),
                      da.data_ptr(), grad.data_ptr(), a.numel() // 32, _lib.stream(a.device))
        return _in_proj96_grads(ctx, da, dw, db)


class _OutProjAddLN(torch.autograd.Function):
    """LayerNorm(x + out_proj.weight a + out_proj.bias) on [..., 32] bfloat16 tokens (pmx_tok32ln_forward / _backward)."""

    @staticmethod
    def forward(ctx, x, a, w, b, gamma, beta, eps, pack=None):
        x, a = x.contiguous(), a.contiguous()
        if pack is None:
            pack = pack_out_proj(w, b, gamma, beta)
        y = torch.empty_like(x)
        _lib.call("pmx_tok32ln_forward", x.data_ptr(), a.data_ptr(), pack.data_ptr(), y.data_ptr(), x.numel() // 32, float(eps),
                  _lib.stream(a.device))
        ctx.save_for_backward(x, a, pack)
        ctx.eps = float(eps)
        ctx.dtypes = [t.dtype for t in (w, b, gamma, beta)]
        return y

    @staticmethod
    def backward(ctx, dy):
        x, a, pack = ctx.saved_tensors
        dy = dy.to(torch.bfloat16).contiguous()
        dx, da = torch.empty_like(x), torch.empty_like(a)
        grad = partial_rows.buffer(_lib.GRAD_PARTIAL_ROWS, _lib.TOK32_GRAD_FLOATS, a.device)
        outs, wanted = row0(grad, _TOK32_SLICES, ctx.needs_input_grad[2:6])
        with partial_rows.OWNER.defer(_lib.load(), grad, _lib.TOK32_GRAD_FLOATS, wanted, _all_f32(ctx.dtypes), "pmx_tok32ln"):
            _lib.call("pmx_tok32ln_backward", x.data_ptr(), a.data_ptr(), dy.data_ptr(), pack.data_ptr(), dx.data_ptr(), da.data_ptr(),
                      grad.data_ptr(), x.numel() // 32, ctx.eps, _lib.stream(a.device))
        outs[0] = outs[0].view(32, 32)
        return (dx, da) + tuple(o.to(dt) for o, dt in zip(outs, ctx.dtypes)) + (None, None)


def _fused_tokens_ok(x, *weights):
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] == 32
            and all(w.dtype == torch.float32 for w in weights))


def _in_proj96_ok(x, mha):
    return _fused_tokens_ok(x, mha.in_proj_weight) and tuple(mha.in_proj_weight.shape) == (96, 32)


def in_proj96(x, mha, pack=None):
    if _in_proj96_ok(x, mha):
        return _InProj96.apply(x, mha.in_proj_weight, mha.in_proj_bias, pack)
    return token_linear(x, mha.in_proj_weight, mha.in_proj_bias)


def in_proj96_res(x, mha, pack=None):
    """-> (qkv, x_res): x_res is x, to be used for the layer's residual connection (see _InProj96Res)."""
    if _in_proj96_ok(x, mha):
        return _InProj96Res.apply(x, mha.in_proj_weight, mha.in_proj_bias, pack)
    return token_linear(x, mha.in_proj_weight, mha.in_proj_bias), x


def out_proj_add_layer_norm(x, a, proj, ln, pack=None):
    if _fused_tokens_ok(x, proj.weight) and a.dtype == torch.bfloat16 and tuple(proj.weight.shape) == (32, 32):
        return _OutProjAddLN.apply(x, a, proj.weight, proj.bias, ln.weight, ln.bias, ln.eps, pack)
    return add_layer_norm_small(x, token_linear(a, proj.weight, proj.bias), ln)


def ffn_layer_norm(x, lin1, lin2, ln, pack=None):
    """The feed-forward half of the post-LN encoder layer: the fused HIP kernels for bf16 tokens of width 32 with a 128-wide
    hidden layer on the GPU, the separate ops otherwise."""
    if (x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] == 32 and tuple(lin1.weight.shape) == (128, 32)
            and tuple(lin2.weight.shape) == (32, 128) and lin1.weight.dtype == torch.float32):
        return _FFNLayerNorm.apply(x, lin1.weight, lin1.bias, lin2.weight, lin2.bias, ln.weight, ln.bias, ln.eps, pack)
    f = token_linear(F.relu(token_linear(x, lin1.weight, lin1.bias)), lin2.weight, lin2.bias)
    return add_layer_norm_small(x, f, ln)


def attention8_forward(qkv, want_lse=False, batch_major=False):
    """softmax(q k^T / sqrt(8)) v for 4 heads of 8 on the matrix cores (pmx_attn8_forward_layout): qkv [S, B, 96] bfloat16 ->
    [S, B, 32] bfloat16 (+ log-sum-exp [B, 4, S] float32); with batch_major qkv is [B, S, 96] and the result [B, S, 32]."""
    (B, S, _) = qkv.shape if batch_major else (qkv.shape[1], qkv.shape[0], 0)
    qkv = qkv.contiguous()
    out = torch.empty(qkv.shape[0], qkv.shape[1], 32, dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty(B, 4, S, dtype=torch.float32, device=qkv.device) if want_lse else None
    _lib.call("pmx_attn8_forward_layout", qkv.data_ptr(), out.data_ptr(), lse.data_ptr() if want_lse else None, S, B,
              1 if batch_major else 0, _lib.stream(qkv.device))
    return (out, lse) if want_lse else out


class _Attention8(torch.autograd.Function):
    """Differentiable wrapper of the MFMA attention kernels (pmx_attn8_forward_layout / pmx_attn8_backward_layout)."""

    @staticmethod
    def forward(ctx, qkv, batch_major):
        out, lse = attention8_forward(qkv, want_lse=True, batch_major=batch_major)
        ctx.save_for_backward(qkv.contiguous(), out, lse)
        ctx.batch_major = batch_major
        return out

    @staticmethod
    def backward(ctx, gout):
        qkv, out, lse = ctx.saved_tensors
        B, S = lse.shape[0], lse.shape[2]
        gout = gout.contiguous().to(torch.bfloat16)
        dqkv = torch.empty_like(qkv)
        _lib.call("pmx_attn8_backward_layout", qkv.data_ptr(), out.data_ptr(), gout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), S, B,
                  1 if ctx.batch_major else 0, _lib.stream(qkv.device))
        return dqkv, None


def attention8(qkv, batch_major=False):
    return _Attention8.apply(qkv, batch_major)


class _Projector(torch.autograd.Function):
    """tokens [B, H*W, 32] bf16 = conv3x3(8 -> 32)(obs) + bias + positional table, batch-major, through pmx_proj_forward / _backward
    (csrc/pmx_actor.hip): the observation planes are read as they are (bytes), no cast, no layout copy, no library convolution."""

    @staticmethod
    def forward(ctx, obs, w, b, pe):
        obs = obs.contiguous()
        B, _, H, W = obs.shape
        pack = pack_projector(w, b)
        tok = torch.empty(B, H * W, 32, dtype=torch.bfloat16, device=obs.device)
        _lib.call("pmx_proj_forward", obs.data_ptr(), actor_tower._OBS_CODE[obs.dtype], pack.data_ptr(), pe.data_ptr(), tok.data_ptr(),
                  B, H, W, _lib.stream(obs.device))
        ctx.save_for_backward(obs)
        ctx.dtypes = (w.dtype, b.dtype)
        return tok

    @staticmethod
    def backward(ctx, dtok):
        (obs,) = ctx.saved_tensors
        B, _, H, W = obs.shape
        dev = obs.device
        dtok = dtok.to(torch.bfloat16).contiguous()
        part = torch.empty(_lib.PROJ_PARTIAL_ROWS * _lib.PROJ_GRAD_ROW_FLOATS, dtype=torch.float32, device=dev)
        dw = torch.empty(32, 8, 3, 3, dtype=torch.float32, device=dev)
        db = torch.empty(32, dtype=torch.float32, device=dev)
        _lib.call("pmx_proj_backward", obs.data_ptr(), actor_tower._OBS_CODE[obs.dtype], dtok.data_ptr(), part.data_ptr(), dw.data_ptr(),
                  db.data_ptr(), B, H, W, _lib.stream(dev))
        return None, dw.to(ctx.dtypes[0]), db.to(ctx.dtypes[1]), None


class _CriticTail(torch.autograd.Function):
    """value = Linear_1(gelu(Linear_512(mean over tokens))) through pmx_critic_tail_forward / _backward: the mean pool, both
    linears, the GELU and -- backwards -- the broadcast of the pooled gradient over the tokens and all four parameter gradients."""

    @staticmethod
    def forward(ctx, tokens, w1, b1, w2, b2):
        tokens = tokens.contiguous()
        B, S, _ = tokens.shape
        value = torch.empty(B, dtype=torch.float32, device=tokens.device)
        pooled = torch.empty(B, 32, dtype=torch.float32, device=tokens.device)
        _lib.call("pmx_critic_tail_forward", tokens.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), value.data_ptr(),
                  pooled.data_ptr(), B, S, _lib.stream(tokens.device))
        ctx.save_for_backward(pooled, w1, b1, w2)
        ctx.S = S
        return value

    @staticmethod
    def backward(ctx, dvalue):
        pooled, w1, b1, w2 = ctx.saved_tensors
        B, S, dev = pooled.shape[0], ctx.S, pooled.device
        dvalue = dvalue.float().contiguous()
        dtok = torch.empty(B, S, 32, dtype=torch.bfloat16, device=dev)
        scratch = torch.empty(2 * B * 512, dtype=torch.bfloat16, device=dev)
        grad = partial_rows.buffer(_lib.HEADS_PARTIAL_ROWS, _lib.CRITIC_TAIL_GRAD_FLOATS, dev)
        (dw1, db1, dw2, db2), wanted = row0(grad, _CRITIC_TAIL_SLICES, ctx.needs_input_grad[1:5])
        with partial_rows.OWNER.defer(_lib.load(), grad, _lib.CRITIC_TAIL_GRAD_FLOATS, wanted, family="pmx_critic_tail"):
            _lib.call("pmx_critic_tail_backward", pooled.data_ptr(), dvalue.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                      dtok.data_ptr(), scratch.data_ptr(), grad.data_ptr(), B, S, _lib.stream(dev))
        return dtok, dw1.view(512, 32), db1, dw2.view(1, 512), db2


def column_sums(t):
    """t.sum over all but the last dimension, in float32: the HIP column-sum kernel for a contiguous bfloat16 tensor on the
    GPU whose last dimension is a multiple of 8 (<= 256), torch's reduction otherwise."""
    C_ = t.shape[-1]
    if t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous() and C_ % 8 == 0 and 8 <= C_ <= 256 and t.numel() >= C_ * 4096:
        partial = torch.empty(_lib.COLSUM_BLOCKS, C_, dtype=torch.float32, device=t.device)
        _lib.call("pmx_colsum_bf16", t.data_ptr(), t.numel() // C_, C_, partial.data_ptr(), _lib.stream(t.device))
        return partial.sum(0)
    if t.dim() == 1:
        return t.float()
    return t.sum(dim=tuple(range(t.dim() - 1)), dtype=torch.float32)


class _TokenLinear(torch.autograd.Function):
    """F.linear on a token tensor [S, B, in] with the weight gradient computed as S batched GEMMs of depth B followed by
    a sum over S.  hipBLASLt's choice for the flat [S*B, in]^T x [S*B, out] product (K = 630 k rows, a 32 x 128 result)
    is a 16x32x512 tile that takes 0.4-0.6 ms per call on MI355X; eight of them were 12 % of the optimizer step."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        return F.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gx = gy.matmul(weight.to(gy.dtype)) if ctx.needs_input_grad[0] else None
        gw = torch.bmm(gy.transpose(1, 2), x.to(gy.dtype)).sum(0).to(weight.dtype) if ctx.needs_input_grad[1] else None
        gb = column_sums(gy).to(weight.dtype) if ctx.needs_input_grad[2] else None
        return gx, gw, gb


def token_linear(x, weight, bias):
    if x.dim() == 3 and torch.is_grad_enabled() and weight.requires_grad:
        if x.is_cuda and torch.is_autocast_enabled():
            dt = torch.get_autocast_gpu_dtype()
            x, weight, bias = x.to(dt), weight.to(dt), bias.to(dt)
        return _TokenLinear.apply(x, weight, bias)
    return F.linear(x, weight, bias)
