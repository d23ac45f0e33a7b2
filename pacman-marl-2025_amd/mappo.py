"""MAPPO on the vectorised env: model, PPO loss/update, flat parameter bucket, data-parallel gradient exchange.

Mirrors the training side of the reference's pacman_mappo_resnet.py for the hot path only:
  MAPPOAgent            :97-211 (+ ResidualBlock :49-67, PositionalEncoding2D :69-95); parameter names are the
                        reference's, so its state_dict checkpoints load unchanged
  ppo_loss              :571-585 (per-minibatch advantage normalisation with the unbiased std, clipped surrogate,
                        0.5*MSE value loss, entropy bonus)
  PPOLearner.update_minibatch  :587-595 (zero_grad, backward, clip_grad_norm_ 0.5, Adam eps 1e-5, EMA 0.995)
  canonicalize_action   :232-238
Differences that are design, not semantics: parameters, gradients and the EMA copy live in ONE flat fp32 buffer each
(one RCCL all-reduce per optimizer step over xGMI, one fused Adam, one lerp for the EMA); the network runs under
bf16 autocast on the GPU (MFMA through MIOpen / hipBLASLt) with fp32 master weights; fp32 on CPU for the parity tests.
"""
import contextlib
import ctypes as C
import math
import os
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils import stateless

from . import _lib, actor_tower, partial_rows
from .actor_head import _ActorHead, _ActorTail
from .actor_tower import group_norm_gelu
from .critic_kernels import (_CriticTail, _Projector, add_layer_norm_small, attention8, attention8_forward, encoder_packs, ffn_layer_norm,
                             in_proj96, in_proj96_res, out_proj_add_layer_norm, pack_ffn, pack_in_proj, pack_out_proj, token_linear)
# not called by the model: the trainer, tests and tools reach these two as mappo.<name>, like the functions above
from .actor_head import pack_actor_head  # noqa: F401
from .critic_kernels import column_sums  # noqa: F401

GAMMA, GAE_LAMBDA = 0.99, 0.95                     # pacman_mappo_resnet.py:19-20
CLIP_EPS, VF_COEF, MAX_GRAD_NORM = 0.15, 0.5, 0.5  # :21-23
LR_START, LR_END = 2e-4, 4e-5                      # :27-28
ENT_COEF_START, ENT_COEF_END = 0.02, 0.004         # :29-30
EMA_DECAY = 0.995                                  # :38
SHAPING_SCALE = 0.1                                # :34


class CriticEncoderLayer(nn.TransformerEncoderLayer):
    """The post-LN encoder layer of nn.TransformerEncoderLayer (norm_first=False, ReLU, dropout 0) with the same
    parameters and the same math, written out so that (a) the two LayerNorms over d_model = 32 use layer_norm_small and
    (b) the four projections use token_linear.  Self-attention follows nn.MultiheadAttention: packed in-projection,
    heads split as [B*h, S, d], scaled_dot_product_attention, out-projection."""

    def forward(self, src, src_mask=None, src_key_padding_mask=None, is_causal=False):
        x = src                                                       # [S, B, E]
        S, B, E = x.shape
        mha = self.self_attn
        h, d = mha.num_heads, E // mha.num_heads
        if x.is_cuda and torch.is_autocast_enabled() and x.dtype != torch.bfloat16:
            x = x.to(torch.bfloat16)
        qkv = in_proj96(x, mha) if (E == 32 and h == 4) else token_linear(x, mha.in_proj_weight, mha.in_proj_bias)
        if self.fused_ok(qkv, S):
            a = attention8(qkv) if torch.is_grad_enabled() else attention8_forward(qkv)   # hand-written MFMA attention
            x = out_proj_add_layer_norm(x, a, mha.out_proj, self.norm1)
            return ffn_layer_norm(x, self.linear1, self.linear2, self.norm2)
        q, k, v = qkv.chunk(3, dim=-1)
        q, k, v = (t.reshape(S, B * h, d).transpose(0, 1).reshape(B, h, S, d) for t in (q, k, v))
        a = F.scaled_dot_product_attention(q, k, v)                    # [B, h, S, d]
        a = a.permute(2, 0, 1, 3).reshape(S, B, E)
        a = token_linear(a, mha.out_proj.weight, mha.out_proj.bias)
        x = add_layer_norm_small(x, a, self.norm1)
        f = token_linear(F.relu(token_linear(x, self.linear1.weight, self.linear1.bias)), self.linear2.weight, self.linear2.bias)
        return add_layer_norm_small(x, f, self.norm2)

    def fused_ok(self, t, S):
        """True when the hand-written kernels take this layer's tensors: bfloat16 on the GPU, embed 32, 4 heads, S in range."""
        mha = self.self_attn
        return (t.is_cuda and t.dtype == torch.bfloat16 and mha.embed_dim == 32 and mha.num_heads == 4
                and S <= (640 if torch.is_grad_enabled() else 1024))

    def packs(self):
        """This layer's three parameter packs (in-projection, out-projection + norm1, feed-forward + norm2) on the current stream."""
        mha = self.self_attn
        return (pack_in_proj(mha.in_proj_weight, mha.in_proj_bias),
                pack_out_proj(mha.out_proj.weight, mha.out_proj.bias, self.norm1.weight, self.norm1.bias),
                pack_ffn(self.linear1.weight, self.linear1.bias, self.linear2.weight, self.linear2.bias, self.norm2.weight, self.norm2.bias))

    fold_residual_gradient = True   # development switch: False = autograd adds the in-projection's and the residual's gradients itself

    def forward_batch_major(self, x, packs=None):
        """The same layer on x [B, S, 32] bfloat16 (tokens of a sample contiguous: the memory order of a channels-last
        convolution output), hand-written kernels only; the caller has checked fused_ok.  packs: this layer's packs() made ahead."""
        mha = self.self_attn
        p_in, p_out, p_ffn = packs if packs is not None else (None, None, None)
        if torch.is_grad_enabled() and self.fold_residual_gradient:
            qkv, x = in_proj96_res(x, mha, p_in)      # the residual branch's gradient is added inside the in-projection's backward kernel
        else:
            qkv = in_proj96(x, mha, p_in)
        a = attention8(qkv, True) if torch.is_grad_enabled() else attention8_forward(qkv, batch_major=True)
        x = out_proj_add_layer_norm(x, a, mha.out_proj, self.norm1, p_out)
        return ffn_layer_norm(x, self.linear1, self.linear2, self.norm2, p_ffn)


class ResidualBlock(nn.Module):
    """conv3x3 - GroupNorm(4) - GELU - conv3x3 - GroupNorm(4) - (+x) - GELU   (pacman_mappo_resnet.py:49-67)"""

    def __init__(self, channels):
        super().__init__()
        self.conv1 = nn.Conv2d(channels, channels, 3, padding=1)
        self.gn1 = nn.GroupNorm(4, channels)
        self.act = nn.GELU()
        self.conv2 = nn.Conv2d(channels, channels, 3, padding=1)
        self.gn2 = nn.GroupNorm(4, channels)

    def forward(self, x):
        y = group_norm_gelu(self.conv1(x), None, self.gn1)
        return group_norm_gelu(self.conv2(y), x, self.gn2)


class PositionalEncoding2D(nn.Module):
    """Fixed sin/cos table: first half of the channels encodes y, second half x (pacman_mappo_resnet.py:69-95)."""

    def __init__(self, d_model, max_h=50, max_w=50):
        super().__init__()
        half = d_model // 2
        den = torch.exp(torch.arange(0, half, 2) * -(math.log(10000.0) / half))

        def table(n):
            pos = torch.arange(n).unsqueeze(1)
            t = torch.zeros(n, half)
            t[:, 0::2] = torch.sin(pos * den)
            t[:, 1::2] = torch.cos(pos * den)
            return t

        self.register_buffer("y_enc", table(max_h))
        self.register_buffer("x_enc", table(max_w))

    def table(self, H, W):
        """[H, W, d_model]"""
        return torch.cat([self.y_enc[:H, None, :].expand(H, W, -1), self.x_enc[None, :W, :].expand(H, W, -1)], dim=2)

    def forward(self, x):
        _, _, H, W = x.shape
        return x + self.table(H, W).permute(2, 0, 1).unsqueeze(0).to(x.dtype)


class MAPPOAgent(nn.Module):
    """Actor: conv 8->16->32, three residual blocks, Linear(32*H*W -> 512), LayerNorm, GELU, Linear(512 -> 5).
    Critic: conv 8->32 + 2-D positional encoding, 2 post-LN Transformer encoder layers (d=32, 4 heads, ff=128) over
    the H*W tokens, mean pool, Linear 32->512->1 (pacman_mappo_resnet.py:97-170)."""

    def __init__(self, obs_shape, action_dim=5, num_agents=2):
        super().__init__()
        self.obs_shape = tuple(obs_shape)
        C, H, W = self.obs_shape
        ch = 32
        self.actor_backbone = nn.Sequential(
            nn.Conv2d(C, 16, 3, padding=1), nn.GELU(), nn.Conv2d(16, ch, 3, padding=1), nn.GELU(),
            ResidualBlock(ch), ResidualBlock(ch), ResidualBlock(ch), nn.Flatten())
        self.actor_head = nn.Sequential(nn.Linear(ch * H * W, 512), nn.LayerNorm(512), nn.GELU(), nn.Linear(512, action_dim))
        self.d_model = 32
        self.critic_projector = nn.Sequential(nn.Conv2d(C, self.d_model, 3, padding=1))
        self.pos_encoder = PositionalEncoding2D(self.d_model)
        layer = CriticEncoderLayer(d_model=self.d_model, nhead=4, dim_feedforward=128, dropout=0.0, batch_first=False)
        self.critic_transformer = nn.TransformerEncoder(layer, num_layers=2, enable_nested_tensor=False)
        self.critic_head = nn.Sequential(nn.Linear(self.d_model, 512), nn.GELU(), nn.Linear(512, 1))
        self.apply(self._init_weights)                                   # :149-158
        nn.init.orthogonal_(self.actor_head[-1].weight, gain=0.01)
        nn.init.orthogonal_(self.critic_head[-1].weight, gain=1.0)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, (nn.Linear, nn.Conv2d)):
            nn.init.orthogonal_(m.weight, gain=math.sqrt(2))
            if m.bias is not None:
                m.bias.data.fill_(0.0)

    fused_tower = True      # use the fused actor-tower kernels where they apply (bf16 on the GPU, supported board size)
    batch_major_critic = True   # run the critic channels-last / batch-major under bf16 autocast on the GPU (no transposing copies)
    fused_loss = True       # the PPO objective and its gradient w.r.t. logits / values as one kernel on the GPU (pmx_ppo_loss)
    tower_pack = None       # packed tower parameters for inference, set by a caller that knows the weights are frozen
                            # (VecMAPPOTrainer.rollout); None = pack on every call

    fused_heads = True      # the small ends of the two heads as one kernel each way under bf16 autocast (csrc/pmx_heads.hip)

    def _fused_heads_ok(self, t):
        """The head-tail kernels take bfloat16 activations under bf16 autocast on the GPU and float32 master weights of the
        reference's shapes (they round the linears' operands to bf16 themselves, as autocast does)."""
        ah, ch = self.actor_head, self.critic_head
        return (self.fused_heads and t.is_cuda and t.dtype == torch.bfloat16 and torch.is_autocast_enabled()
                and ah[3].weight.dtype == torch.float32 and ch[0].weight.dtype == torch.float32 and ch[2].weight.dtype == torch.float32
                and tuple(ah[3].weight.shape) == (5, 512) and tuple(ch[0].weight.shape) == (512, 32) and tuple(ch[2].weight.shape) == (1, 512)
                and ah[1].weight.dtype == torch.float32)

    fused_head = True       # the first actor-head layer on the project's own matrix-core kernels under bf16 autocast (csrc/pmx_actor_head.hip)
    fused_head_max_batch = 0     # ... up to this many samples per call; above it the permuted F.linear below stays, untouched.  0: the
                                 # model keeps the library everywhere -- alone the kernels are ahead of it up to 2 048 samples, but the
                                 # replayed 512-sample optimizer step measured 4 % slower with them; a caller
                                 # that runs the layer by itself (evaluation on a frozen pack, eager steps) may raise it
    head_pack = None        # its packed weight for inference, set beside tower_pack by a caller that knows the weights are frozen

    def head_kernels_for(self, batch):
        """Whether logits() runs the first head layer on pmx_actor_head_* for a training call of `batch` samples under bf16 autocast (what
        PPOLearner asks before it decides whether the layer reads its bfloat16 shadow)."""
        _, H, W = self.obs_shape
        lin = self.actor_head[0]
        return bool(self.fused_head and self.fused_tower and batch is not None and 0 < batch <= self.fused_head_max_batch
                    and lin.in_features == 32 * H * W and lin.out_features == 512 and lin.bias is not None
                    and actor_tower.tower_supported(H, W))

    def _fused_head_ok(self, lin, HW, batch):
        """The kernels take the fused tower's features under bf16 autocast and the float32 master weight of the reference's shape, up to
        fused_head_max_batch samples.  A call without gradients takes them only on a frozen pack: packing the 5 - 13 MB weight for one
        inference call costs more than the product saves."""
        return (self.fused_head and batch <= self.fused_head_max_batch and torch.is_autocast_enabled()
                and torch.get_autocast_dtype("cuda") == torch.bfloat16
                and (torch.is_grad_enabled() or self.head_pack is not None)
                and lin.weight.dtype == torch.float32 and lin.bias is not None and lin.bias.dtype == torch.float32
                and lin.in_features == 32 * HW and lin.out_features == 512)

    def _use_fused_tower(self, obs):
        if not (self.fused_tower and obs.is_cuda and obs.dim() == 4 and obs.dtype in (torch.bfloat16, torch.uint8)):
            return False
        if self.actor_backbone[0].weight.dtype != torch.float32:
            return False
        return actor_tower.tower_supported(obs.shape[2], obs.shape[3])

    def logits(self, obs):
        if self._use_fused_tower(obs):
            # one kernel for the whole convolutional tower (csrc/pmx_actor.hip); its output is channels-last, nn.Flatten's
            # order is channel-major
            if self.tower_pack is not None and not torch.is_grad_enabled():
                feat = actor_tower.tower_forward(obs, self.tower_pack)
            else:
                feat = actor_tower.actor_tower(self.actor_backbone, obs)         # [B, H*W, 32] bf16
            # nn.Flatten's order is (channel, cell), the kernel's is (cell, channel): permute the 5 MB weight of the first
            # head layer instead of the features (160 MB per 16 384 samples, forward and again backward); autograd carries the
            # gradient back through the view
            lin = self.actor_head[0]
            HW = feat.shape[1]
            if self._fused_head_ok(lin, HW, feat.shape[0]):
                pack = self.head_pack if not torch.is_grad_enabled() else None
                h = _ActorHead.apply(feat, lin.weight, lin.bias, obs.shape[2], obs.shape[3], pack)     # [B, 512] by _fused_head_ok
            else:
                w = lin.weight.view(lin.out_features, 32, HW).permute(0, 2, 1).reshape(lin.out_features, HW * 32)
                h = F.linear(feat.reshape(feat.shape[0], HW * 32), w, lin.bias)
            if self._fused_heads_ok(h) and h.shape[1] == 512:
                ln, out = self.actor_head[1], self.actor_head[3]
                return _ActorTail.apply(h, ln.weight, ln.bias, out.weight, out.bias, ln.eps)
            return self.actor_head[1:](h)
        if obs.dtype == torch.uint8:            # byte planes are an input format of the fused tower only
            obs = obs.to(torch.bfloat16 if (obs.is_cuda and torch.is_autocast_enabled()) else torch.float32)
        if obs.is_cuda and obs.dtype == torch.bfloat16 and obs.dim() == 4:
            # channels-last end to end: MIOpen's NHWC bf16 implicit-GEMM convolutions and the NHWC GroupNorm kernels then
            # need no layout transposes; nn.Flatten still flattens in logical (C, H, W) order, one copy at the end
            obs = obs.contiguous(memory_format=torch.channels_last)
        return self.actor_head(self.actor_backbone(obs))

    fused_projector = True  # the critic's projector + positional table as one kernel under bf16 autocast (pmx_proj_forward)

    def _pe_table(self, H, W, dev):
        """The positional table [H*W, 32] float32 on `dev`, built once per board size."""
        key = (H, W, str(dev))
        cache = self.__dict__.setdefault("_pe_cache", {})
        t = cache.get(key)
        if t is None:
            t = cache[key] = self.pos_encoder.table(H, W).reshape(H * W, self.d_model).float().contiguous().to(dev)
        return t

    def _fused_projector_ok(self, merged_obs):
        conv = self.critic_projector[0]
        if not (self.fused_projector and merged_obs.dtype in (torch.uint8, torch.bfloat16, torch.float32) and merged_obs.dim() == 4
                and merged_obs.shape[1] == 8 and conv.weight.dtype == torch.float32 and tuple(conv.weight.shape) == (32, 8, 3, 3)):
            return False
        return actor_tower.tower_supported(merged_obs.shape[2], merged_obs.shape[3])

    def value(self, merged_obs):
        """merged_obs [B,8,H,W] -> [B] (pacman_mappo_resnet.py:160-170)"""
        layers = self.critic_transformer.layers
        bm = (self.batch_major_critic and merged_obs.is_cuda and torch.is_autocast_enabled()
              and torch.get_autocast_dtype("cuda") == torch.bfloat16
              and layers[0].fused_ok(merged_obs.new_empty(0, dtype=torch.bfloat16), merged_obs.shape[2] * merged_obs.shape[3]))
        if bm:
            # channels-last end to end: the projector's output [B, H, W, d] IS the token tensor [B, S, d] (no transposing copy
            # on the way in, none for its gradient on the way back) and the encoder layers run batch-major
            B, _, H, W = merged_obs.shape
            # every parameter pack of the encoder layers in one launch (they depend on nothing but the weights; six small launches sat in
            # front of the six kernels that read them).  (Making them on a side stream instead crashes hipStreamEndCapture when that
            # stream forks from the critic's side stream -- a fork inside a fork -- on ROCm 7.0.)
            dev = merged_obs.device
            layer_tuple = tuple(layers)
            all_f32 = all(p.dtype == torch.float32 for l in layer_tuple for p in l.parameters()) and len(layer_tuple) <= 4
            fused_proj = self._fused_projector_ok(merged_obs)
            lpacks = encoder_packs(layer_tuple) if all_f32 else None
            if fused_proj:
                conv = self.critic_projector[0]
                x = _Projector.apply(merged_obs, conv.weight, conv.bias, self._pe_table(H, W, dev))
            else:
                if merged_obs.dtype == torch.uint8:
                    merged_obs = merged_obs.to(torch.bfloat16)
                y = self.critic_projector(merged_obs.contiguous(memory_format=torch.channels_last))
                x = y.permute(0, 2, 3, 1)
                if not x.is_contiguous():
                    x = x.contiguous()
                x = (x + self.pos_encoder.table(H, W).to(x.dtype)).reshape(B, H * W, self.d_model)
            for k, layer in enumerate(layers):
                x = layer.forward_batch_major(x, lpacks[k] if lpacks is not None else None)
            if self.critic_transformer.norm is not None:
                x = self.critic_transformer.norm(x)
            if self._fused_heads_ok(x):
                l1, l2 = self.critic_head[0], self.critic_head[2]
                return _CriticTail.apply(x, l1.weight, l1.bias, l2.weight, l2.bias)
            return self.critic_head(x.mean(dim=1)).squeeze(-1)
        if merged_obs.dtype == torch.uint8:
            merged_obs = merged_obs.to(torch.bfloat16 if (merged_obs.is_cuda and torch.is_autocast_enabled()) else torch.float32)
        x = self.pos_encoder(self.critic_projector(merged_obs))
        x = x.flatten(2).permute(2, 0, 1)                                # [H*W, B, d]
        x = self.critic_transformer(x).mean(dim=0)
        return self.critic_head(x).squeeze(-1)

    def evaluate(self, obs, merged_obs, action, *, legal=None):
        """-> value, log_prob, entropy  (:196-205).  legal: int32 mask words (canonicalize_legal); actions outside a row's effective
        mask enter as -inf."""
        # same arithmetic as torch.distributions.Categorical(logits=...): normalise with logsumexp, probs by softmax
        logits = self.logits(obs).float()
        if legal is not None:
            logits = logits.masked_fill(~legal_bits(legal, action), float("-inf"))
        norm = logits - logits.logsumexp(dim=-1, keepdim=True)
        probs = F.softmax(norm, dim=-1)
        logp = norm.gather(1, action.view(-1, 1)).squeeze(1)
        ent = -(norm.clamp(min=torch.finfo(norm.dtype).min) * probs).sum(-1)
        return self.value(merged_obs).float(), logp, ent

    forward = evaluate      # torch.func.functional_call(model, params, (obs, merged, act)) == evaluate with those params

    @torch.no_grad()
    def act(self, obs, generator=None, *, legal=None, seed=0, counter=0):
        """Sample actions for a batch: -> action [B] int64, log_prob [B] (Categorical(logits).sample, :173-177).  With `legal` (int32
        mask words) the draw is sample_actions' counter-based one over the legal actions, keyed by (seed, counter)."""
        if legal is not None:
            return sample_actions(self.logits(obs), legal, seed=seed, counter=counter)
        logp_all = F.log_softmax(self.logits(obs).float(), dim=-1)
        a = torch.multinomial(logp_all.exp(), 1, generator=generator).squeeze(1)
        return a, logp_all.gather(1, a.view(-1, 1)).squeeze(1)

    @torch.no_grad()
    def get_deterministic_action(self, obs, *, legal=None):              # :207-211
        if legal is not None:
            return sample_actions(self.logits(obs), legal, greedy=True)[0]
        return self.logits(obs).argmax(dim=-1)


_RED_ACTION_MAP = (0, 3, 2, 1, 4)   # East <-> West for a red learner (pacman_mappo_resnet.py:232-238)


def _per_env(red, like):
    """A per-env colour vector [N] (bool / uint8) as a bool tensor that broadcasts over the leading dimension of `like`."""
    return red.to(torch.bool).view((-1,) + (1,) * (like.dim() - 1))


def canonicalize_action_per_env(action, red):
    """canonicalize_action with the colour chosen per env: action [N, ...], red [N] bool / uint8; East and West swap only in
    the rows where red is set.  (The map is its own inverse, so this also takes canonical actions back to the env's frame.)"""
    return torch.where(_per_env(red, action) & ((action == 1) | (action == 3)), 4 - action, action)


def canonicalize_legal_per_env(bits, red):
    """canonicalize_legal with the colour chosen per env: bits [N, ...] env mask bits, red [N]; int32 words."""
    w = bits.to(torch.int32) & 0x1F
    return torch.where(_per_env(red, w), (w & 0x15) | ((w & 2) << 2) | ((w & 8) >> 2), w)


def _team_column_index(red, opponents):
    # the [N, 4] agent axis seen as [N, 2, 2]: agent = 2k + c with c = 0 red, c = 1 blue
    c = red.to(torch.bool) if opponents else ~red.to(torch.bool)
    return c.to(torch.int64).view(-1, 1, 1).expand(-1, 2, 1)


def team_columns(x, red, opponents=False):
    """The learners' two columns of x [N, 4] per env -- agents (0, 2) where red [N] is set, (1, 3) elsewhere -- as [N, 2];
    opponents=True: the other team's."""
    return x.reshape(-1, 2, 2).gather(2, _team_column_index(red, opponents)).squeeze(2)


def set_team_columns(x, red, values, opponents=False):
    """The inverse of team_columns: writes values [N, 2] into the learners' (opponents') two columns of x [N, 4], in place."""
    x.view(-1, 2, 2).scatter_(2, _team_column_index(red, opponents), values.to(x.dtype).unsqueeze(2))
    return x


def canonicalize_action(action, is_red_agent):
    if isinstance(is_red_agent, torch.Tensor):                # a colour per env
        return canonicalize_action_per_env(action, is_red_agent)
    if not is_red_agent:
        return action
    if isinstance(action, torch.Tensor):
        return torch.tensor(_RED_ACTION_MAP, device=action.device, dtype=action.dtype)[action.long()]
    return _RED_ACTION_MAP[int(action)]


# bits 1 (East) and 3 (West) of a legal-action mask swapped: the mask counterpart of _RED_ACTION_MAP, as a 32-entry look-up
_RED_LEGAL_LUT = tuple((b & 0x15) | ((b & 2) << 2) | ((b & 8) >> 2) for b in range(32))
_RED_LEGAL_TENSORS = {}


def canonicalize_legal(bits, is_red_agent):
    """Env mask bits (PmxVecEnv.legal: bit a = action a legal, in the env's frame) as the int32 words the policy reads, in the
    learner's canonical frame: for a red learner East and West swap, as in canonicalize_action."""
    if isinstance(is_red_agent, torch.Tensor):                # a colour per env
        return canonicalize_legal_per_env(bits, is_red_agent)
    if isinstance(bits, torch.Tensor):
        w = bits.to(torch.int32) & 0x1F
        if not is_red_agent:
            return w
        key = _dev_key(bits.device)
        if key not in _RED_LEGAL_TENSORS:
            _RED_LEGAL_TENSORS[key] = torch.tensor(_RED_LEGAL_LUT, dtype=torch.int32, device=bits.device)
        return _RED_LEGAL_TENSORS[key][w.long()]
    b = int(bits) & 0x1F
    return _RED_LEGAL_LUT[b] if is_red_agent else b


def legal_bits(legal, action=None):
    """[B, 5] bool of a row's effective mask: the word's low five bits, Stop always, and -- as the objective counts it -- the
    stored action."""
    w = legal.long().view(-1) | 0x10
    if action is not None:
        w = w | (1 << action.long().view(-1))
    return ((w[:, None] >> torch.arange(5, device=w.device)) & 1).bool()


def _lowbias32(x):
    """lowbias32 on an int64 tensor holding uint32 values (products wrap in int64; the low 32 bits are exact)."""
    M = 0xFFFFFFFF
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & M
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & M
    return x ^ (x >> 16)


@torch.no_grad()
def sample_actions(logits, legal=None, seed=0, counter=0, greedy=False):
    """One action per row of logits [B, 5] under legal-action masks (int32 words, None = everything legal; include/pmx.h,
    pmx_policy_sample): -> (action int64 [B], log_prob float32 [B]).  The draw is a hash of (seed, row, counter), so one
    (seed, counter) on the same inputs gives the same actions.  On the GPU this is the kernel; on the CPU the same specification
    in torch, float32, with the same hash."""
    assert logits.dim() == 2 and logits.shape[1] == 5
    B = logits.shape[0]
    seed, counter = int(seed) & 0xFFFFFFFF, int(counter) & 0xFFFFFFFF
    if legal is not None:
        legal = legal.reshape(-1)
        assert legal.dtype == torch.int32 and legal.shape[0] == B and legal.device == logits.device
    if logits.is_cuda:
        if logits.dtype not in (torch.float32, torch.bfloat16):
            logits = logits.float()
        logits = logits.contiguous()
        action = torch.empty(B, dtype=torch.int64, device=logits.device)
        logp = torch.empty(B, dtype=torch.float32, device=logits.device)
        with torch.cuda.device(logits.device):
            _lib.call("pmx_policy_sample", logits.data_ptr(), 1 if logits.dtype == torch.bfloat16 else 0,
                      legal.contiguous().data_ptr() if legal is not None else None, B, seed, counter, 1 if greedy else 0,
                      action.data_ptr(), logp.data_ptr(), _lib.stream(logits.device))
        return action, logp
    z = logits.float()
    ks = torch.arange(5)
    bit = legal_bits(legal) if legal is not None else torch.ones(B, 5, dtype=torch.bool)
    z = z.masked_fill(~bit, float("-inf"))
    zmax = z.max(dim=1).values
    p = (z - zmax[:, None]).exp()
    run = [p[:, 0]]
    for k in range(1, 5):
        run.append(run[-1] + p[:, k])                     # p_0 + ... + p_k, added in that order
    total = run[4]
    if greedy:
        a = torch.where(bit & (z == zmax[:, None]), ks, 5).min(dim=1).values
    else:
        M = 0xFFFFFFFF
        rows = torch.arange(B, dtype=torch.int64)
        h = _lowbias32(seed ^ ((rows * 0x9E3779B1) & M) ^ ((counter * 0x85EBCA77) & M) ^ 0x6A09E667)
        t = (h >> 8).to(torch.float32) * 2.0 ** -24 * total
        first = torch.where(bit & (torch.stack(run, dim=1) > t[:, None]), ks, 5).min(dim=1).values
        last = torch.where(bit, ks, -1).max(dim=1).values
        a = torch.where(first < 5, first, last)
    logp = (z.gather(1, a.view(-1, 1)).squeeze(1) - zmax) - total.log()
    return a, logp


def _loss_scalar(v):
    """A clip / entropy coefficient as the (device pointer, host value) pair the objective kernels take."""
    if isinstance(v, torch.Tensor):
        assert v.is_cuda and v.dtype == torch.float32 and v.numel() == 1
        return v.data_ptr(), 0.0
    return None, float(v)


class _PPOLossMaskedFn(torch.autograd.Function):
    """pmx_ppo_loss_masked: _PPOLossFn with one int32 legal-action word per row behind the actions."""

    @staticmethod
    def forward(ctx, logits, values, act, legal, old_logp, adv, ret, clip_eps, ent_coef, vf_coef):
        logits, values = logits.contiguous(), values.contiguous()
        B, BV = logits.shape[0], values.shape[0]
        assert legal.is_cuda and legal.dtype == torch.int32 and legal.numel() == B
        stats = torch.empty(5, dtype=torch.float32, device=logits.device)
        dlogits, dvalues = torch.empty_like(logits), torch.empty_like(values)
        cp, ch = _loss_scalar(clip_eps)
        ep, eh = _loss_scalar(ent_coef)
        _lib.call("pmx_ppo_loss_masked", logits.data_ptr(), 1 if logits.dtype == torch.bfloat16 else 0, values.data_ptr(),
                  act.contiguous().data_ptr(), legal.contiguous().data_ptr(), old_logp.contiguous().data_ptr(), adv.contiguous().data_ptr(),
                  ret.contiguous().data_ptr(), B, BV, cp, ep, ch, eh, float(vf_coef), stats.data_ptr(), dlogits.data_ptr(),
                  dvalues.data_ptr(), _lib.stream(logits.device))
        ctx.save_for_backward(dlogits, dvalues)
        return stats

    @staticmethod
    def backward(ctx, gstats):
        return _PPOLossFn.backward(ctx, gstats) + (None,)


class _PPOLossFn(torch.autograd.Function):
    """pmx_ppo_loss: the objective's five scalars from the raw network outputs in one launch; the gradient with respect to the
    logits and the values is computed in the same launch and handed out (scaled) by backward."""

    @staticmethod
    def forward(ctx, logits, values, act, old_logp, adv, ret, clip_eps, ent_coef, vf_coef):
        logits, values = logits.contiguous(), values.contiguous()
        B, BV = logits.shape[0], values.shape[0]
        stats = torch.empty(5, dtype=torch.float32, device=logits.device)
        dlogits, dvalues = torch.empty_like(logits), torch.empty_like(values)

        def scalar(v):
            if isinstance(v, torch.Tensor):
                assert v.is_cuda and v.dtype == torch.float32 and v.numel() == 1
                return v.data_ptr(), 0.0
            return None, float(v)
        cp, ch = scalar(clip_eps)
        ep, eh = scalar(ent_coef)
        _lib.call("pmx_ppo_loss", logits.data_ptr(), 1 if logits.dtype == torch.bfloat16 else 0, values.data_ptr(), act.contiguous().data_ptr(),
                  old_logp.contiguous().data_ptr(), adv.contiguous().data_ptr(), ret.contiguous().data_ptr(), B, BV, cp, ep,
                  ch, eh, float(vf_coef), stats.data_ptr(), dlogits.data_ptr(), dvalues.data_ptr(), _lib.stream(logits.device))
        ctx.save_for_backward(dlogits, dvalues)
        return stats

    @staticmethod
    def backward(ctx, gstats):
        dlogits, dvalues = ctx.saved_tensors
        unit = _UNIT5.get(_dev_key(gstats.device))
        if unit is not None and gstats.data_ptr() == unit.data_ptr():
            return dlogits, dvalues, None, None, None, None, None, None, None      # d(loss) = 1: the kernel's gradients as they are
        g = gstats[4]                                     # only the total loss is an objective; the other entries are reports
        return dlogits * g.to(dlogits.dtype), dvalues * g, None, None, None, None, None, None, None


# Differentiating `loss = stats[4]` costs five small launches before the first real backward kernel (a one for the root, a zero
# 5-vector and the copy of the one into it for the select, two scalings of the kernel's gradients by it) -- 27 us on the critical
# path of a 540 us step.  The learner differentiates the 5-vector itself against this constant [0, 0, 0, 0, 1] instead
# (loss_root), and the backward above recognises it by address.
_UNIT5 = {}


def _dev_key(dev):
    return (dev.type, dev.index if dev.index is not None else (torch.cuda.current_device() if dev.type == "cuda" else 0))


def loss_root(loss):
    """(tensor to differentiate, grad_outputs) for a loss returned by ppo_loss: the fused objective's 5-vector with the unit
    gradient where the loss came from the fused kernel, the loss itself otherwise."""
    stats = getattr(loss, "_pmx_stats", None)
    if stats is None:
        return loss, None
    key = _dev_key(stats.device)
    if key not in _UNIT5:
        _UNIT5[key] = torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0], dtype=torch.float32, device=stats.device)
    return stats, _UNIT5[key]


_SIDE_STREAMS = {}


def _side_stream(dev):
    """One extra stream per device for the critic half of the optimizer step."""
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    st = _SIDE_STREAMS.get(key)
    if st is None:
        st = _SIDE_STREAMS[key] = torch.cuda.Stream(device=dev)
    return st


def _fused_loss_ok(model, obs, act, old_logp, adv, ret):
    return (MAPPOAgent.fused_loss and isinstance(model, MAPPOAgent) and obs.is_cuda and act.dtype == torch.int64
            and all(t.dtype == torch.float32 for t in (old_logp, adv, ret)) and act.shape[0] >= 2)


def ppo_loss(model, obs, merged, act, old_logp, adv, ret, clip_eps, ent_coef, vf_coef=VF_COEF, legal=None):
    """The minibatch objective of pacman_mappo_resnet.py:571-585.  Returns (loss, dict of detached scalars).  legal: one int32
    legal-action word per sample (the mask its action was drawn under); None is the reference's objective over all five logits."""
    if _fused_loss_ok(model, obs, act, old_logp, adv, ret):
        # The actor and the critic share nothing until the loss: the critic's forward runs on a side stream, so autograd
        # runs its backward there too (a node's backward uses its forward's stream) and the two halves of the step overlap.
        # At the reference's minibatch of 512 most kernels fill a fraction of the chip and the replayed step was one serial
        # chain of ~80 small launches; in the captured graph the two chains become parallel branches.
        cur = torch.cuda.current_stream(obs.device)
        side = _side_stream(obs.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            vals = model.value(merged).float()
        logits = model.logits(obs)
        cur.wait_stream(side)
        vals.record_stream(cur)
        if logits.dtype not in (torch.float32, torch.bfloat16):
            logits = logits.float()
        if legal is None:
            stats = _PPOLossFn.apply(logits, vals, act, old_logp, adv, ret, clip_eps, ent_coef, vf_coef)
        else:
            stats = _PPOLossMaskedFn.apply(logits, vals, act, legal, old_logp, adv, ret, clip_eps, ent_coef, vf_coef)
        d = stats.detach()
        loss = stats[4]
        loss._pmx_stats = stats                           # (loss_root: what the learner differentiates instead of the select)
        return loss, {"pg": d[0], "vl": d[1], "entropy": d[2], "clip_frac": d[3], "loss": d[4]}
    vals, logp, ent = model.evaluate(obs, merged, act) if legal is None else model.evaluate(obs, merged, act, legal=legal)
    if vals.shape[0] != ret.shape[0]:
        # paired minibatch: rows 2k and 2k+1 are the two learners of one env-tick and share ONE merged critic input
        # (merge_obs_for_critic is per env-tick, pacman_mappo_resnet.py:556-557 expands it per agent); the critic ran on
        # the unique inputs only and its value is used for both rows -- the same numbers, half the critic work
        assert vals.shape[0] * 2 == ret.shape[0]
        vals = vals.repeat_interleave(2)
    norm_adv = (adv - adv.mean()) / (adv.std() + 1e-8)                   # unbiased std, per minibatch (:577)
    ratio = (logp - old_logp).exp()
    pg = -torch.min(norm_adv * ratio, norm_adv * torch.clamp(ratio, 1 - clip_eps, 1 + clip_eps)).mean()
    vl = 0.5 * ((vals - ret) ** 2).mean()
    ent_mean = ent.mean()
    loss = pg + vf_coef * vl - ent_coef * ent_mean
    with torch.no_grad():
        clip_frac = ((ratio - 1).abs() > clip_eps).float().mean()
    return loss, {"pg": pg.detach(), "vl": vl.detach(), "entropy": ent_mean.detach(), "clip_frac": clip_frac,
                  "loss": loss.detach()}


class FlatBucket:
    """All parameters of a module re-homed as views into one flat fp32 buffer; same for the gradients.
    The data-parallel exchange is then ONE all-reduce of `grad` per optimizer step (2.6 M params = 10.5 MB on
    smallCapture: latency-bound on xGMI, so one message beats many).
    `names` are the parameters' names in bucket order, `offsets[i]:offsets[i + 1]` is parameter i's slice of the flat buffers."""

    def __init__(self, module):
        named = [(n, p) for n, p in module.named_parameters() if p.requires_grad]
        self.names = [n for n, _ in named]
        self.params = params = [p for _, p in named]
        self.offsets = [0]
        for p in params:
            self.offsets.append(self.offsets[-1] + p.numel())
        self.numel = self.offsets[-1]
        dev, dt = params[0].device, params[0].dtype
        self.data = torch.empty(self.numel, device=dev, dtype=dt)
        self.grad = torch.zeros(self.numel, device=dev, dtype=dt)
        for p, a, b in zip(params, self.offsets, self.offsets[1:]):
            self.data[a:b].copy_(p.data.reshape(-1))
            p.data = self.data[a:b].view_as(p)
            p.grad = self.grad[a:b].view_as(p)


class PPOLearner:
    """One optimizer step = ppo_loss -> backward into the flat gradient -> (all-reduce mean over ranks) -> clip by global
    norm 0.5 -> Adam(eps 1e-5) -> EMA 0.995 (pacman_mappo_resnet.py:587-595).  Every rank ends each step with bit-identical
    parameters because the clip and the update see the same reduced gradient."""

    def __init__(self, model, lr=LR_START, process_group=None, world_size=1, autocast_dtype=None, force_collectives=False):
        self.model = model
        self.bucket = FlatBucket(model)
        self.ema = self.bucket.data.clone()                              # EMA of the parameters (:365, :593-595)
        self.exp_avg = torch.zeros_like(self.bucket.data)
        self.exp_avg_sq = torch.zeros_like(self.bucket.data)
        self.step_count = 0
        self.lr = lr
        self.betas, self.eps = (0.9, 0.999), 1e-5                        # torch.optim.Adam defaults, eps from :366
        self.pg = process_group
        self.world_size = world_size
        # data parallel: the gradient exchange is issued when there is more than one rank -- or when a caller rehearses the
        # collective path on a one-rank group (bench.py on a one-GPU box)
        self.dp = world_size > 1 or bool(force_collectives)
        self.autocast_dtype = autocast_dtype
        self._offsets = self.bucket.offsets
        # the actor's parameters (a contiguous prefix of the bucket), then the critic's: see _grad_groups
        n, n_actor = len(self.bucket.params), 0
        while n_actor < n and self.bucket.names[n_actor].startswith("actor_"):
            n_actor += 1
        self._groups = [(0, n_actor), (n_actor, n)] if 0 < n_actor < n else [(0, n)]
        # the bfloat16 copy of the bucket and what hangs on it (_shadow_context), made on the first bf16 step on the GPU
        self._sh16 = self._shadow_slots = self._shadow_views = None
        self._bf16_fresh = False                                         # the optimizer kernel has just written _sh16
        self._opt_scratch = self._opt_norm = None                        # _fused_tail's buffers, made on its first call
        # the captured step (capture): graph(s), static inputs, device scalars, the stats it returns, running report sums
        self._graph = self._graphs = self._g_groups = None
        self._g_in = self._g_sc = self._g_stats = self._g_acc = self._g_acc_keys = self._g_batch = None

    # the second-stage row sums of the gradient reductions folded into the gradient gather (partial_rows.OWNER): eight small
    # launches less on the chains of the 512-sample step.  (A first version ran them on a third stream beside the next backward kernel
    # and LOST -- 1 380 against 1 995 steps/s: six fork / join pairs cost the captured graph more than the kernels cost the chain.)
    defer_row_sums = True

    def _grad_groups(self):
        """Index ranges [lo, hi) into bucket.params whose gradients are produced -- and, under data parallelism, reduced --
        together, in the order the backward pass is run: the actor's parameters (a contiguous prefix of the bucket that holds
        97 % of its bytes: the 4928 -> 512 head), then the critic's.  Data parallel, the actor's slice is reduced while the critic's
        backward runs.  One range when nothing is exchanged."""
        return self._groups if self.dp else [(0, len(self.bucket.params))]

    def _gather_grads(self, flat, first):
        """pmx_flatten_sum_to_f32: the float32 / bfloat16 gradients `flat` into the float32 bucket from element `first` on, in one
        launch; gradients that are still partial rows (partial_rows.OWNER) are summed on the way."""
        n = len(flat)
        owner = partial_rows.OWNER
        if any(not g.is_contiguous() for g in flat):
            owner.flush()                                    # (a copy would read rows that have not been added yet)
            flat = [g.contiguous() for g in flat]
        src = (C.c_void_p * n)(*[g.data_ptr() for g in flat])
        isb = (C.c_uint8 * n)(*[1 if g.dtype == torch.bfloat16 else 0 for g in flat])
        cnt = (C.c_int32 * n)(*[g.numel() for g in flat])
        pend = [owner.claim(g) for g in flat]
        rows = (C.c_int32 * n)(*[r for r, _ in pend])
        stride = (C.c_int32 * n)(*[f for _, f in pend])
        offs, o = [], first
        for g in flat:
            offs.append(o); o += g.numel()
        off = (C.c_int64 * n)(*offs)
        owner.settle()                                       # (raises before anything reads a row 0 that nobody will sum)
        _lib.call("pmx_flatten_sum_to_f32", n, src, isb, rows, stride, off, cnt, self.bucket.grad.data_ptr(), _lib.stream(self.bucket.grad.device))

    def _backward_group(self, loss, lo, hi, retain):
        """Gradients of bucket.params[lo:hi] into their slice of the flat float32 bucket: one gathering copy instead of
        loss.backward() (AccumulateGrad ADDS every parameter's gradient into its zeroed view of the bucket -- ~80 small kernels
        per step on this network, a quarter of the launches of the 512-sample step)."""
        params = self.bucket.params[lo:hi]
        targets = list(params)
        if self._shadow_views is not None:
            for i, v in self._shadow_views.items():
                if lo <= i < hi:
                    targets[i - lo] = v                  # the bfloat16 copy the library op multiplied by
        grad = self.bucket.grad
        # the gathering kernel applies: a float32 bucket on the GPU, gradients float32 or bfloat16 (autograd hands every gradient
        # out in its target's type).  Only then may the backward kernels leave partial rows behind for it.
        gather = grad.is_cuda and grad.dtype == torch.float32 and all(t.dtype in (torch.float32, torch.bfloat16) for t in targets)
        root, unit = loss_root(loss)
        with partial_rows.OWNER.enabled(self.defer_row_sums and gather):
            grads = torch.autograd.grad(root, targets, grad_outputs=unit, allow_unused=True, retain_graph=retain)
        flat = [g.reshape(-1) if g is not None else torch.zeros(p.numel(), dtype=grad.dtype, device=grad.device)
                for g, p in zip(grads, params)]
        if gather:
            self._gather_grads(flat, self._offsets[lo])
        else:
            partial_rows.OWNER.flush()
            torch.cat([g.to(grad.dtype) for g in flat], out=grad[self._offsets[lo]:self._offsets[hi]])

    def _reduce_slice(self, lo, hi):
        """Starts the all-reduce (mean over ranks) of the gradient slice of bucket.params[lo:hi]; returns a closure that makes the
        current stream wait for it and finishes the mean.  RCCL averages in the collective; gloo (the CPU tests) sums, and the
        division follows."""
        import torch.distributed as dist                     # optional
        sl = self.bucket.grad[self._offsets[lo]:self._offsets[hi]]
        avg = self.bucket.grad.is_cuda
        h = dist.all_reduce(sl, op=dist.ReduceOp.AVG if avg else dist.ReduceOp.SUM, group=self.pg, async_op=True)

        def finish():
            h.wait()
            if not avg:
                sl.div_(self.world_size)
        return finish

    def _backward_into_bucket(self, loss):
        """The backward pass with the gradient ending up in the flat float32 bucket and, under data parallelism, averaged over the
        ranks: group by group, each group's all-reduce in flight while the next group's backward runs."""
        groups = self._grad_groups()
        pending = []
        for k, (lo, hi) in enumerate(groups):
            self._backward_group(loss, lo, hi, retain=k + 1 < len(groups))
            if self.dp:
                pending.append(self._reduce_slice(lo, hi))
        for fin in pending:
            fin()

    def _refresh_bf16(self):
        """The bfloat16 copy follows the float32 weights (unless the optimizer kernel has just written it)."""
        if self._bf16_fresh:
            self._bf16_fresh = False
        elif self._sh16 is not None:
            with torch.no_grad():
                self._sh16.copy_(self.bucket.data)

    # parameters that only torch library ops read (the two heads' linears, the critic's projector): under bf16 autocast each of them
    # was cast to bfloat16 on use and its gradient cast back -- ~20 small kernels per step.  They are read from a bfloat16 copy of
    # the WHOLE bucket instead (one cast kernel after the optimizer step); the copy's slices take the parameters' places for the
    # forward pass and receive the gradients, which pmx_flatten_to_f32 widens into the bucket.  Same roundings as autocast's.
    SHADOWED = ("actor_head.0.", "actor_head.3.", "critic_projector.0.", "critic_head.0.", "critic_head.2.")
    # (the head-tail kernels and the projector kernel read their layers' float32 masters and round the operands themselves)
    SMALL_HEAD_LAYERS = ("actor_head.3.", "critic_head.0.", "critic_head.2.")

    def _shadowed_prefixes(self, batch=None):
        """batch: the actor samples of the step about to run, None when the caller does not say (the first head layer then keeps its
        shadow and the library path, as before the kernels existed)."""
        keep = self.SHADOWED
        if getattr(self.model, "fused_heads", False):
            keep = tuple(k for k in keep if k not in self.SMALL_HEAD_LAYERS)
        if getattr(self.model, "fused_projector", False):
            keep = tuple(k for k in keep if k != "critic_projector.0.")
        kernels = getattr(self.model, "head_kernels_for", None)
        if kernels is not None and kernels(batch):           # pmx_actor_head_pack reads the float32 master, the gradients come back float32
            keep = tuple(k for k in keep if k != "actor_head.0.")
        return keep
    shadow_weights = True

    def _shadow_context(self, batch=None):
        """Context manager under which the module's library-op parameters are their bfloat16 shadows (and a no-op when the
        shadows do not apply: CPU, float32 steps).  batch: see _shadowed_prefixes."""
        if not (self.shadow_weights and self.autocast_dtype == torch.bfloat16 and self.bucket.data.is_cuda):
            self._shadow_views = None
            return contextlib.nullcontext()
        if self._sh16 is None:
            self._sh16 = self.bucket.data.to(torch.bfloat16).requires_grad_(True)
        keep = self._shadowed_prefixes(batch)
        self._shadow_slots = [(i, n) for i, n in enumerate(self.bucket.names) if n.startswith(keep)]
        self._shadow_views, pd = {}, {}
        for i, n in self._shadow_slots:
            v = self._sh16[self._offsets[i]:self._offsets[i + 1]].view(self.bucket.params[i].shape)
            self._shadow_views[i] = v
            pd[n] = v
        return stateless._reparametrize_module(self.model, pd)

    def _loss(self, obs, merged, act, old_logp, adv, ret, clip_eps, ent_coef, legal=None):
        """ppo_loss in the learner's precision: under autocast with the bfloat16 shadow weights in place, or in plain float32."""
        if self.autocast_dtype is None:
            self._shadow_views = None
            return ppo_loss(self.model, obs, merged, act, old_logp, adv, ret, clip_eps, ent_coef, legal=legal)
        with self._shadow_context(obs.shape[0]), torch.autocast(device_type=self.bucket.data.device.type, dtype=self.autocast_dtype):
            return ppo_loss(self.model, obs, merged, act, old_logp, adv, ret, clip_eps, ent_coef, legal=legal)

    def set_lr(self, lr):
        self.lr = lr

    def _adam_step(self):
        """torch.optim.Adam's single-tensor update (no amsgrad, no weight decay) on the flat buffers."""
        self.step_count += 1
        b1, b2 = self.betas
        g, p = self.bucket.grad, self.bucket.data
        self.exp_avg.lerp_(g, 1 - b1)
        self.exp_avg_sq.mul_(b2).addcmul_(g, g, value=1 - b2)
        bc1 = 1 - b1 ** self.step_count
        bc2 = 1 - b2 ** self.step_count
        denom = (self.exp_avg_sq.sqrt() / math.sqrt(bc2)).add_(self.eps)
        p.addcdiv_(self.exp_avg, denom, value=-self.lr / bc1)

    def _torch_tail(self):
        """clip_grad_norm_(parameters, 0.5) -> Adam -> EMA as torch ops (the CPU, and what the fused tail is tested against);
        returns the gradient norm.  The norm is the 2-norm of the per-tensor 2-norms (the reference's summation order; a single
        fp32 reduction over the 2.6 M-element flat buffer is measurably less accurate on the CPU); the gradient is scaled by
        max_norm / (norm + 1e-6) if that is < 1."""
        gn = torch.linalg.vector_norm(torch.stack(torch._foreach_norm([p.grad for p in self.bucket.params])))
        self.bucket.grad.mul_(torch.clamp(MAX_GRAD_NORM / (gn + 1e-6), max=1.0))
        self._adam_step()
        self.ema.mul_(EMA_DECAY).add_(self.bucket.data, alpha=1 - EMA_DECAY)
        return gn

    fused_optimizer = True   # clip + Adam + EMA as two launches on the GPU (pmx_clip_adam_ema) instead of ~18 torch kernels

    def _fused_tail(self, scalars_dev=None, reports5=None, report_sums6=None):
        """clip_grad_norm_ -> Adam -> EMA through pmx_clip_adam_ema_tail; returns the gradient norm (a 0-dim device tensor).  With
        scalars_dev the bias-corrected step sizes are read from that device tensor (graph replay), else computed here from
        step_count, which the caller has already advanced.  The same launch refreshes the bfloat16 copy of the parameters (where
        there is one) and, given report_sums6, adds the objective's five scalars and the gradient norm to it."""
        dev = self.bucket.data.device
        if self._opt_scratch is None:
            self._opt_scratch = torch.empty(_lib.OPT_PARTIALS, dtype=torch.float64, device=dev)
            self._opt_norm = torch.zeros(1, dtype=torch.float32, device=dev)
        b1, b2 = self.betas
        if scalars_dev is None:
            bc1, bc2 = 1 - b1 ** self.step_count, 1 - b2 ** self.step_count
            sp, a, b = None, self.lr / bc1, 1.0 / math.sqrt(bc2)
        else:
            sp, a, b = scalars_dev.data_ptr(), 0.0, 0.0
        _lib.call("pmx_clip_adam_ema_tail", self.bucket.grad.data_ptr(), self.bucket.data.data_ptr(), self.exp_avg.data_ptr(),
                  self.exp_avg_sq.data_ptr(), self.ema.data_ptr(), self.bucket.numel, self._opt_scratch.data_ptr(),
                  sp, a, b, b1, b2, self.eps, MAX_GRAD_NORM, EMA_DECAY, self._opt_norm.data_ptr(),
                  self._sh16.data_ptr() if self._sh16 is not None else None,
                  reports5.data_ptr() if reports5 is not None else None,
                  report_sums6.data_ptr() if report_sums6 is not None else None, _lib.stream(dev))
        self._bf16_fresh = self._sh16 is not None
        return self._opt_norm[0]

    def _use_fused_tail(self):
        return (self.fused_optimizer and self.bucket.data.is_cuda and self.bucket.data.dtype == torch.float32
                and self.bucket.grad.is_contiguous() and self.bucket.data.is_contiguous())

    def update_minibatch(self, obs, merged, act, old_logp, adv, ret, clip_eps=CLIP_EPS, ent_coef=ENT_COEF_START, legal=None):
        loss, stats = self._loss(obs, merged, act, old_logp, adv, ret, clip_eps, ent_coef, legal)
        self._backward_into_bucket(loss)                  # (data parallel: includes the gradient all-reduce)
        if self._use_fused_tail():
            self.step_count += 1
            gn = self._fused_tail().clone()
        else:
            gn = self._torch_tail()
        self._refresh_bf16()
        stats["grad_norm"] = gn.detach()
        return stats

    def snapshot(self):
        """Copies of everything an optimizer step changes: weights, both Adam moments, the EMA, the step count."""
        return {"data": self.bucket.data.clone(), "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(),
                "ema": self.ema.clone(), "step": self.step_count}

    def restore(self, snap):
        """Back to a snapshot() (or to a checkpoint with the same keys); the bfloat16 copy follows the weights."""
        for t, k in ((self.bucket.data, "data"), (self.exp_avg, "exp_avg"), (self.exp_avg_sq, "exp_avg_sq"), (self.ema, "ema")):
            t.copy_(snap[k])
        self.step_count = int(snap["step"])
        self._refresh_bf16()

    # ---- hipGraph capture of the whole optimizer step (launch-bound at the reference's minibatch of 512) ----------
    @staticmethod
    def graph_replay_safe():
        """hipGraph replay is only trusted with ROCclr's AQL packet capture switched off, and only if the runtime can have
        read the switch: set before HIP initialised (see the package __init__, which records that at import)."""
        pkg = sys.modules.get(__name__.rsplit(".", 1)[0])
        return os.environ.get("DEBUG_CLR_GRAPH_PACKET_CAPTURE") == "0" and bool(getattr(pkg, "GRAPH_REPLAY_OK", False))

    def capture(self, batch, obs_shape, in_dtype, clip_eps=CLIP_EPS, ent_coef=ENT_COEF_START, merged_batch=None, masked=False):
        """Record zero_grad -> forward -> backward -> (all-reduce) -> clip -> Adam -> EMA for a fixed minibatch shape into
        a HIP graph.  Scalars that change between updates (lr, clip, entropy coefficient, Adam bias corrections) live in
        device tensors that the graph reads, so one capture serves the whole schedule.  masked: the graph has a seventh static
        input, `legal` (int32 [batch] legal-action words), and its objective is the masked one."""
        if not self.graph_replay_safe():
            raise RuntimeError("hipGraph replay of the optimizer step needs DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 in the environment "
                               "before HIP initialises (ROCm 7 graph packet-capture bug, DESIGN.md section 5)")
        if not self._use_fused_tail():
            raise RuntimeError("the captured optimizer step ends in the fused clip + Adam + EMA kernel (pmx_clip_adam_ema_tail): it needs "
                               "fused_optimizer and contiguous float32 buckets on the GPU")
        dev = self.bucket.data.device
        i = self._g_in = dict(obs=torch.zeros((batch,) + tuple(obs_shape), dtype=in_dtype, device=dev),
                              merged=torch.zeros((merged_batch or batch,) + tuple(obs_shape), dtype=in_dtype, device=dev),
                              act=torch.zeros(batch, dtype=torch.int64, device=dev),
                              logp=torch.zeros(batch, dtype=torch.float32, device=dev),
                              adv=torch.randn(batch, dtype=torch.float32, device=dev),
                              ret=torch.zeros(batch, dtype=torch.float32, device=dev))
        if masked:
            i["legal"] = torch.full((batch,), 0x1F, dtype=torch.int32, device=dev)
        # lr/bc1, 1/sqrt(bc2), clip_eps, ent_coef as device scalars
        self._g_sc = torch.zeros(4, dtype=torch.float32, device=dev)
        self._g_stats = None
        self._g_acc = torch.zeros(6, dtype=torch.float32, device=dev)       # sums of (pg, vl, entropy, clip_frac, loss, grad_norm)
        REPORTS = ("pg", "vl", "entropy", "clip_frac", "loss")

        # Data parallel: the collectives stay OUTSIDE the graphs (eager RCCL calls), so the step is recorded as two graphs:
        #   graph 0: forward, loss, whole backward, gradients into the bucket      | then ONE all-reduce of the whole bucket
        #   graph 1: clip, Adam, EMA, weight copies, reports
        # Both graphs share one memory pool.  Replayed steps are the launch-bound ones (small minibatches): there the actor's and the
        # critic's backward run side by side on two streams inside one graph, which buys more than reducing the actor's slice early
        # (one graph per gradient group: 1 800 against 1 300 steps/s at 512 samples on one GPU).  The eager step still reduces
        # slice by slice (_backward_into_bucket).
        n = len(self.bucket.params)

        def seg_first():
            loss, stats = self._loss(i["obs"], i["merged"], i["act"], i["logp"], i["adv"], i["ret"], self._g_sc[2], self._g_sc[3], i.get("legal"))
            self._backward_group(loss, 0, n, retain=False)
            return loss, stats

        def seg_tail(loss, stats):
            # the fused objective's 5-vector (ppo_loss leaves it on the loss): with it the optimizer kernel keeps the running sums
            s5 = getattr(loss, "_pmx_stats", None)
            in_kernel = s5 is not None and tuple(stats.keys()) == REPORTS and s5.dtype == torch.float32
            gn = self._fused_tail(self._g_sc, *((s5.detach(), self._g_acc) if in_kernel else ()))
            self._refresh_bf16()
            stats["grad_norm"] = gn
            # running sums of the step's reports, inside the graph: a caller that averages them over an update reads ONE tensor at
            # the end instead of launching an add per report and step
            self._g_acc_keys = tuple(stats.keys())
            if not in_kernel:
                self._g_acc.add_(torch.stack([stats[k].float() for k in self._g_acc_keys]))
            return stats

        def run_eager():
            out = seg_first()
            if self.dp:
                self._reduce_slice(0, n)()
            return seg_tail(*out)

        # warm up on a side stream (allocator, MIOpen solver search), restoring the optimizer state afterwards
        saved = self.snapshot()
        self._set_graph_scalars(clip_eps, ent_coef, step=1)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for _ in range(3):
                run_eager()
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize(dev)
        # Capture in THREAD-LOCAL error mode: in the default (global) mode a capture in progress forbids "unsafe" runtime calls from
        # every thread of the process -- and ProcessGroupNCCL's watchdog thread polls the events of recent collectives with
        # hipEventQuery, which then fails with hipErrorStreamCaptureUnsupported and takes the process down (seen when a capture began
        # right behind the warm-up steps' all-reduces).  This thread makes no such call while it captures; other threads' launches on
        # the capturing streams (autograd's workers) are recorded either way.  The pause lets the watchdog retire what has completed.
        if self.dp:
            time.sleep(0.25)
        tl = dict(capture_error_mode="thread_local")
        if not self.dp:
            self._graph = torch.cuda.CUDAGraph()
            self._graphs = None
            with torch.cuda.graph(self._graph, **tl):
                out = seg_first()
                self._g_stats = seg_tail(*out)
        else:
            g0, g1 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(g0, **tl):
                out = seg_first()
            with torch.cuda.graph(g1, pool=g0.pool(), **tl):
                self._g_stats = seg_tail(*out)
            self._graphs = [g0, g1]
            self._graph = None
            self._g_groups = [(0, n)]           # the gradient range the replayed step reduces (bench.py reports it)
        del out
        self.restore(saved)
        self._g_batch = batch

    def _replay(self):
        """Replays the captured step; data parallel: forward and backward, the all-reduce of the whole gradient, then the
        optimizer tail."""
        if self._graphs is None:
            self._graph.replay()
            return
        self._graphs[0].replay()
        self._reduce_slice(0, len(self.bucket.params))()
        self._graphs[1].replay()

    def _graph_scalar_values(self, clip_eps, ent_coef, step):
        b1, b2 = self.betas
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        return tuple(float(v) for v in (self.lr / bc1, 1.0 / math.sqrt(bc2), clip_eps, ent_coef))

    def _set_graph_scalars(self, clip_eps, ent_coef, step):
        """The four values travel as kernel arguments of ONE launch: stream-ordered, no host staging buffer that could be
        recycled while a copy is still in flight."""
        arr = (C.c_float * 4)(*self._graph_scalar_values(clip_eps, ent_coef, step))
        _lib.call("pmx_set_floats", self._g_sc.data_ptr(), arr, 4, _lib.stream(self._g_sc.device))

    def reset_report_sums(self):
        """Zeroes the running sums that the replayed steps keep of their reports."""
        self._g_acc.zero_()

    def report_sums(self):
        """{report: its sum over the replayed steps since reset_report_sums()} -- 0-dim views of one device tensor."""
        return {k: self._g_acc[j] for j, k in enumerate(self._g_acc_keys)}

    def update_minibatch_graph(self, obs, merged, act, old_logp, adv, ret, clip_eps=CLIP_EPS, ent_coef=ENT_COEF_START, legal=None):
        """Same step as update_minibatch, replayed from the captured graph (inputs are copied into its static buffers)."""
        i = self._g_in
        if (legal is not None) != ("legal" in i):
            raise ValueError("legal-action masks go to a graph captured with masked=True, and only to such a graph")
        i["obs"].copy_(obs); i["merged"].copy_(merged); i["act"].copy_(act)
        i["logp"].copy_(old_logp); i["adv"].copy_(adv); i["ret"].copy_(ret)
        if legal is not None:
            i["legal"].copy_(legal)
        self.step_count += 1
        self._set_graph_scalars(clip_eps, ent_coef, self.step_count)
        self._replay()
        return self._g_stats

    def update_minibatch_graph_gather(self, sources, index, rows_per_index, clip_eps=CLIP_EPS, ent_coef=ENT_COEF_START):
        """The replayed step with its minibatch assembled by ONE gather launch (pmx_gather_rows) straight into the graph's
        static inputs: sources = the flat rollout tensors {obs, merged, act, logp, adv, ret} and, for a graph captured with masks,
        legal (rows = samples; merged rows = env-ticks), index = int64 device indices, rows_per_index = {name: m} (2 for the per-learner tensors of a paired
        minibatch whose index names env-tick pairs).  Returns the graph's stats tensors (valid until the next replay)."""
        names = ("obs", "merged", "act", "logp", "adv", "ret") + (("legal",) if "legal" in self._g_in else ())
        n = len(names)
        VP, I32, I64 = C.c_void_p * n, C.c_int32 * n, C.c_int64 * n
        src, dst, idx, rb, m, nr = VP(), VP(), VP(), I32(), I32(), I64()
        for k, name in enumerate(names):
            s_t, d_t = sources[name], self._g_in[name]
            assert s_t.is_contiguous() and d_t.is_contiguous() and s_t.dtype == d_t.dtype and s_t.shape[1:] == d_t.shape[1:], name
            row = d_t[0].numel() * d_t.element_size() if d_t.dim() > 1 else d_t.element_size()
            src[k], dst[k], idx[k] = s_t.data_ptr(), d_t.data_ptr(), index.data_ptr()
            rb[k], m[k], nr[k] = row, rows_per_index[name], d_t.shape[0]
            assert index.numel() * rows_per_index[name] == d_t.shape[0], (name, index.numel(), d_t.shape)
        assert index.dtype == torch.int64 and index.is_contiguous()
        self.step_count += 1
        vals = self._graph_scalar_values(clip_eps, ent_coef, self.step_count)        # (they travel with the gather: one launch)
        arr = (C.c_float * 4)(*vals)
        _lib.call("pmx_gather_rows_set_floats", n, src, dst, idx, rb, m, nr, self._g_sc.data_ptr(), arr, 4, _lib.stream(index.device))
        self._replay()
        return self._g_stats

    def ema_state_dict(self):
        """state_dict of the EMA weights with the reference's parameter names (what :647-651 saves)."""
        sd = {k: v.clone() for k, v in self.model.state_dict().items()}
        for n, p, a, b in zip(self.bucket.names, self.bucket.params, self._offsets, self._offsets[1:]):
            sd[n] = self.ema[a:b].view_as(p).clone()
        return sd


def schedule(update, total_updates):
    """Linear lr / entropy-coefficient anneal and the clip switch (pacman_mappo_resnet.py:386-391)."""
    progress = update / total_updates
    lr = LR_START - (LR_START - LR_END) * progress
    ent = ENT_COEF_START - (ENT_COEF_START - ENT_COEF_END) * progress
    clip = 0.1 if update > 800 else CLIP_EPS
    return lr, ent, clip
