"""References shared by the any-board tests of the fused actor tower and critic projector (csrc/pmx_actor.hip): the seeded
model and synthetic planes, the rounding-exact emulation of the tower (see tests/test_gpu_actor_tower.py for what the two
references mean) and the float64 projector reference of tests/test_gpu_trainer.py::test_fused_projector_matches_torch.
Boards are (H, W); no layout is needed, the planes are synthetic [B, 8, H, W]."""
import torch
import torch.nn.functional as F


def tiles(H, W):
    """position tiles of 16 of the zero-padded board"""
    return (H * (W + 2) + 15) // 16


def bucket(nt):
    """the tile-count bucket a board runs on (csrc/pmx_actor.hip bucket_for)"""
    if nt in (10, 11):
        return nt
    for b in (16, 28, 36, 44):
        if nt <= b:
            return b
    return 0


def in_domain(H, W):
    return 8 <= W <= 32 and 3 <= H <= 32 and H * W <= 640


def _bf(x):
    return x.to(torch.bfloat16).float()


def model(H, W, seed=0):
    from pmx import mappo
    torch.manual_seed(seed)
    m = mappo.MAPPOAgent((8, H, W)).cuda()
    with torch.no_grad():                      # non-trivial biases and GroupNorm affine parameters
        for p in m.actor_backbone.parameters():
            if p.dim() == 1:
                p.add_(0.3 * torch.randn_like(p))
    return m


def planes(B, H, W, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    o = (torch.rand(B, 8, H, W, device="cuda", generator=g) < 0.25).float()
    o[:, 1] *= torch.randint(1, 6, (B, 1, 1), device="cuda", generator=g).float()     # plane 1 carries 1 + numCarrying
    return o


def emulated_tower(m, obs, ste=False):
    if ste:
        rnd = lambda x: x + (x.float().to(torch.bfloat16).to(x.dtype) - x).detach()
    else:
        rnd = _bf
    bb = m.actor_backbone
    x = obs.to(bb[0].weight.dtype)

    def conv(c, x):
        return rnd(F.conv2d(x, rnd(c.weight), None, padding=1) + c.bias.view(1, -1, 1, 1))
    x = rnd(F.gelu(conv(bb[0], x)))
    x = rnd(F.gelu(conv(bb[2], x)))
    for blk in (bb[4], bb[5], bb[6]):
        y = rnd(F.gelu(F.group_norm(conv(blk.conv1, x), 4, blk.gn1.weight, blk.gn1.bias, 1e-5)))
        x = rnd(F.gelu(F.group_norm(conv(blk.conv2, y), 4, blk.gn2.weight, blk.gn2.bias, 1e-5) + x))
    return x                                    # [B, 32, H, W]


def projector_reference(conv, pe, obs, dtok):
    """float64 with the kernel's roundings made explicit (bf16 weights, the convolution + bias rounded to bf16, then the bf16 sum
    with the bf16 table) -> (bf16-rounded tokens [B, HW, 32], dW, db)"""
    B, _, H, W = obs.shape
    bf = lambda t: t.to(torch.bfloat16).double()
    w64 = conv.weight.detach().double().requires_grad_(True)
    b64 = conv.bias.detach().double().requires_grad_(True)
    wr = w64 + (bf(w64.detach()) - w64.detach())
    y = F.conv2d(obs.double(), wr, b64, padding=1)                     # [B, 32, H, W]
    y = y + (bf(y.detach()) - y.detach())
    ref = (y.permute(0, 2, 3, 1).reshape(B, H * W, 32) + bf(pe)[None])
    dw, db = torch.autograd.grad((ref * dtok.double()).sum(), [w64, b64])
    return bf(ref.detach()), dw, db
