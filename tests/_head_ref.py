"""float64 reference of the first actor-head layer, Linear(32 H W -> 512) (pacman_mappo_resnet.py:117-119), on the operands the
kernels of csrc/pmx_actor_head.hip use: features [B][H W][32] bfloat16 in the tower's (cell, channel) order, the float32 weight in
nn.Linear's (channel, cell) column order rounded to bfloat16 once, h and dh [B][512] bfloat16.

Besides each product the functions return the sum of the absolute values of its terms: an output that adds n terms a_k b_k in
float32, in ANY order, lies within n * 2**-24 * sum |a_k b_k| of the exact sum (each of the at most n - 1 additions and the n
products -- exact here, bfloat16 x bfloat16 fits float32 -- rounds to within 2**-24 relative of a partial sum that never exceeds
sum |a_k b_k|).  The forward product counts the bias as one more term.  Outputs stored as bfloat16 add 2**-8 |ref| for the final
rounding.  Works on any device; every tensor it returns is float64."""
import torch

HID = 512
F32_EPS = 2.0 ** -24
BF16_EPS = 2.0 ** -8


def bf16(x):
    """values rounded to bfloat16 (round to nearest even, as the kernels and autocast round), as float64"""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def to_cell_major(w, HW):
    """[N][32 HW] with column ch * HW + cell (nn.Flatten's order) -> column cell * 32 + ch (the tower's order)"""
    return w.reshape(w.shape[0], 32, HW).permute(0, 2, 1).reshape(w.shape[0], HW * 32)


def to_param_order(wc, HW):
    """the inverse of to_cell_major: column cell * 32 + ch -> column ch * HW + cell"""
    return wc.reshape(wc.shape[0], HW, 32).permute(0, 2, 1).reshape(wc.shape[0], 32 * HW)


def forward(feat, w, bias, drop_cell=None):
    """h = feat . W^T + bias -> (h [B][512], bound on |float32 result - h| before the bfloat16 rounding).
    drop_cell: a NEGATIVE CONTROL that leaves out the 32 features of one cell."""
    B, HW, _ = feat.shape
    x = feat.to(torch.float64).clone()
    if drop_cell is not None:
        x[:, drop_cell, :] = 0
    x = x.reshape(B, HW * 32)
    wc = to_cell_major(bf16(w), HW)
    b = bias.to(torch.float64)
    h = x @ wc.t() + b
    mag = x.abs() @ wc.abs().t() + b.abs()
    return h, (HW * 32 + 1) * F32_EPS * mag


def backward(feat, dh, w, drop_cell=None, drop_sample=None, drop_hidden=None, wrong_order=False):
    """-> dict of (value, summation bound) for dfeat [B][HW][32], dw [512][32 HW] in the PARAMETER's order, db [512].
    Negative controls: drop_cell zeroes one cell of feat, drop_sample leaves one sample out of the batch sums, drop_hidden leaves one
    hidden unit out of dfeat, wrong_order returns dw with the (cell, channel) columns unpermuted."""
    B, HW, _ = feat.shape
    x = feat.to(torch.float64).clone()
    if drop_cell is not None:
        x[:, drop_cell, :] = 0
    x = x.reshape(B, HW * 32)
    d = dh.to(torch.float64).clone()
    wc = to_cell_major(bf16(w), HW)
    dsum = d.clone()
    if drop_sample is not None:
        dsum[drop_sample] = 0
    dfd = d.clone()
    if drop_hidden is not None:
        dfd[:, drop_hidden] = 0
    dfeat = (dfd @ wc).reshape(B, HW, 32)
    dfeat_mag = (dfd.abs() @ wc.abs()).reshape(B, HW, 32)
    dwc = dsum.t() @ x
    dwc_mag = dsum.abs().t() @ x.abs()
    order = (lambda t: t) if wrong_order else (lambda t: to_param_order(t, HW))
    return {"dfeat": (dfeat, HID * F32_EPS * dfeat_mag),
            "dw": (order(dwc), B * F32_EPS * order(dwc_mag)),
            "db": (dsum.sum(0), B * F32_EPS * dsum.abs().sum(0))}


def bf16_bound(ref, bound):
    """the bound of an output that is stored as bfloat16"""
    return bound + BF16_EPS * ref.abs()
