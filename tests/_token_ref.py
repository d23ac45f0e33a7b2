"""Float64 references of the critic's token kernels (csrc/pmx_critic.hip) that round to bfloat16 exactly where the kernels do,
and the seeded inputs the token-kernel tests share.

Rounding points, read off the kernel source:
  * weights are bfloat16 in every product (the packs hold bfloat16 fragments); biases, gamma, beta stay float32;
  * FFN: H = bf16(relu(W1 x + b1)); the ReLU mask of the backward is `H > 0` on that rounded H; dz (LayerNorm's input gradient)
    is rounded to bfloat16 for the products and for db2 but starts the dx accumulator UNROUNDED; dH = bf16(mask * W2^T bf16(dz))
    feeds db1, dW1 and dx; dgamma / dbeta use the unrounded normalised row and dy;
  * tok32ln: dx = bf16(dz), and that rounded dz is what da, dW and db see;
  * tok96: dy arrives in bfloat16; with `res` the sum W^T dy + res is formed in full precision and rounded once;
  * outputs (y, qkv, dx, da) are rounded once at the store.
`rounding=False` turns every one of these off: the references are then the plain formulas, which the CPU test holds against
float64 autograd.  The backward passes are written by hand because autograd cannot express these rounding points."""
import torch

EPS = 1e-5
NEAR_ZERO = 1e-4        # |pre-activation| below this: a float32 evaluation may flip the ReLU mask of the token


def _rounder(rounding):
    if rounding:
        return lambda t: t.float().to(torch.bfloat16).to(torch.float64)
    return lambda t: t


def _layer_norm_fwd_bwd(z, dy, gamma, eps):
    """-> xh, rstd, dz, dgamma, dbeta of LayerNorm over the last dimension (two-pass variance, as the kernels compute it)."""
    zc = z - z.mean(-1, keepdim=True)
    rstd = (zc.square().mean(-1, keepdim=True) + eps).rsqrt()
    xh = zc * rstd
    gd = gamma * dy
    dz = rstd * (gd - gd.mean(-1, keepdim=True) - xh * (gd * xh).mean(-1, keepdim=True))
    return xh, rstd, dz, (dy * xh).sum(0), dy.sum(0)


def ffn_ref(x, dy, w1, b1, w2, b2, gamma, beta, eps=EPS, rounding=True):
    """y = LayerNorm(x + W2 relu(W1 x + b1) + b2) and every gradient.  All arguments float64; x, dy hold bfloat16 values.
    `near`: per token, whether any pre-activation lies within NEAR_ZERO of zero."""
    r = _rounder(rounding)
    W1, W2 = r(w1), r(w2)
    pre = x @ W1.T + b1
    H = r(torch.relu(pre))
    z = x + H @ W2.T + b2
    xh, _, dz, dgamma, dbeta = _layer_norm_fwd_bwd(z, dy, gamma, eps)
    dzb = r(dz)
    dH = r((dzb @ W2) * (H > 0))
    return {"y": r(xh * gamma + beta), "dx": r(dz + dH @ W1), "dw1": dH.T @ x, "db1": dH.sum(0), "dw2": dzb.T @ H, "db2": dzb.sum(0),
            "dgamma": dgamma, "dbeta": dbeta, "dz": dz, "near": (pre.abs() < NEAR_ZERO).any(-1)}


def tok96_ref(a, dy, w, b, res=None, rounding=True):
    """qkv = W a + b; da = W^T dy (+ res, added before the one rounding); dw, db."""
    r = _rounder(rounding)
    W = r(w)
    da = dy @ W
    if res is not None:
        da = da + res
    return {"qkv": r(a @ W.T + b), "da": r(da), "dw": dy.T @ a, "db": dy.sum(0)}


def tok32ln_ref(x, a, dy, w, b, gamma, beta, eps=EPS, rounding=True):
    """y = LayerNorm(x + W a + b) and every gradient."""
    r = _rounder(rounding)
    W = r(w)
    z = x + a @ W.T + b
    xh, _, dz, dgamma, dbeta = _layer_norm_fwd_bwd(z, dy, gamma, eps)
    dt = r(dz)
    return {"y": r(xh * gamma + beta), "dx": dt, "da": r(dt @ W), "dw": dt.T @ a, "db": dt.sum(0), "dgamma": dgamma, "dbeta": dbeta}


# the plain formulas, for autograd
def ffn_plain(x, w1, b1, w2, b2, gamma, beta, eps=EPS):
    return torch.nn.functional.layer_norm(x + torch.relu(x @ w1.T + b1) @ w2.T + b2, (32,), gamma, beta, eps)


def tok96_plain(a, w, b):
    return a @ w.T + b


def tok32ln_plain(x, a, w, b, gamma, beta, eps=EPS):
    return torch.nn.functional.layer_norm(x + a @ w.T + b, (32,), gamma, beta, eps)


PARAM_GRADS = {"ffn": ("dw1", "db1", "dw2", "db2", "dgamma", "dbeta"), "tok96": ("dw", "db"), "tok32ln": ("dw", "db", "dgamma", "dbeta")}
TOKEN_OUTS = {"ffn": ("y", "dx"), "tok96": ("qkv", "da"), "tok32ln": ("y", "dx", "da")}


# ---------------------------------------------------------------------------------------------------------------
# seeded inputs (CPU generator, so that the CPU test sees exactly the rows the GPU tests use)
# ---------------------------------------------------------------------------------------------------------------
ROW_KINDS = ("normal", "zero_var", "offset", "large", "dead", "live", "far_offset")
# far_offset: rows constant at about 1000 whose spread comes from the projection alone (std 0.3 to 1.1), mean / std about 1000.  A
# float32 one-pass variance E[z^2] - mean^2 is off by tens of percent there, while on the `offset` rows (200 + N(0, 1), mean / std
# about 100) it stays within 1.3 * 2**-8 of the output scale, inside the 2 * 2**-8 bound: only far_offset pins the two-pass variance.
ZERO_VAR_CONSTANTS = (0.0, 1.0, -3.0, 100.0)


def _bf(t):
    return t.to(torch.bfloat16)


def hard_row_mask(T):
    """The zero-variance rows of a `zero_var` case: every other token and the last one, so that every tile mixes them with
    ordinary rows and the last token (the one the negative controls drop) is one of them."""
    idx = torch.arange(T)
    return (idx % 2 == 0) | (idx == T - 1)


def _rows(kind, T, g):
    x = torch.randn(T, 32, generator=g)
    if kind == "offset":
        x = 200.0 + x
    elif kind == "large":
        x = 30.0 * x
    elif kind == "far_offset":
        x = (1000.0 + 100.0 * x[:, :1]).expand(T, 32)
    elif kind == "zero_var":
        c = torch.tensor(ZERO_VAR_CONSTANTS)[(torch.arange(T) // 2) % 4]
        x = torch.where(hard_row_mask(T)[:, None], c[:, None].expand(T, 32), x)
    return _bf(x)


def _uniform(g, bound, *shape):
    return (torch.rand(*shape, generator=g) * 2 - 1) * bound


def ffn_case(T, seed, kind="normal"):
    """nn.Linear's default initialisation plus the existing test's perturbations (asymmetric everywhere).
    -> dict of float32 parameters and bfloat16 x, dy on the CPU."""
    g = torch.Generator().manual_seed(seed)
    p = {"w1": _uniform(g, 32 ** -0.5, 128, 32), "b1": _uniform(g, 32 ** -0.5, 128) + 0.3 * torch.randn(128, generator=g),
         "w2": _uniform(g, 128 ** -0.5, 32, 128), "b2": _uniform(g, 128 ** -0.5, 32) + 0.3 * torch.randn(32, generator=g),
         "gamma": 1.0 + 0.2 * torch.randn(32, generator=g), "beta": 0.2 * torch.randn(32, generator=g)}
    if kind == "zero_var":
        p["w2"].zero_(), p["b2"].zero_()
    elif kind == "dead":
        p["b1"] -= 50.0
    elif kind == "live":
        p["b1"] += 50.0
    elif kind == "far_offset":
        p["w2"] /= 1024.0                   # hidden activations of about 1000: keeps W2 H + b2 small beside the constant row
    p["x"] = _rows(kind, T, g)
    p["dy"] = _bf(0.1 * torch.randn(T, 32, generator=g))
    return p


def tok96_case(T, seed, kind="normal"):
    g = torch.Generator().manual_seed(seed)
    p = {"w": 0.2 * torch.randn(96, 32, generator=g), "b": 0.3 * torch.randn(96, generator=g)}
    p["a"] = _rows(kind, T, g)
    p["dy"] = _bf(0.1 * torch.randn(T, 96, generator=g))
    p["res"] = _bf(0.1 * torch.randn(T, 32, generator=g))
    return p


def tok32ln_case(T, seed, kind="normal"):
    g = torch.Generator().manual_seed(seed)
    p = {"w": 0.2 * torch.randn(32, 32, generator=g), "b": 0.3 * torch.randn(32, generator=g),
         "gamma": 1.0 + 0.2 * torch.randn(32, generator=g), "beta": 0.2 * torch.randn(32, generator=g)}
    p["x"] = _rows(kind, T, g)
    a = torch.randn(T, 32, generator=g) * (30.0 if kind == "large" else 1.0)
    if kind == "zero_var":
        p["b"].zero_()
        a = torch.where(hard_row_mask(T)[:, None], torch.zeros_like(a), a)
    p["a"] = _bf(a)
    p["dy"] = _bf(0.1 * torch.randn(T, 32, generator=g))
    return p


def f64(case, device="cpu"):
    return {k: v.to(device=device, dtype=torch.float64) for k, v in case.items()}


def ffn_ref_of(case, device="cpu", rounding=True, rows=slice(None)):
    c = f64(case, device)
    return ffn_ref(c["x"][rows], c["dy"][rows], c["w1"], c["b1"], c["w2"], c["b2"], c["gamma"], c["beta"], rounding=rounding)


def tok96_ref_of(case, device="cpu", rounding=True, rows=slice(None), with_res=False):
    c = f64(case, device)
    return tok96_ref(c["a"][rows], c["dy"][rows], c["w"], c["b"], c["res"][rows] if with_res else None, rounding=rounding)


def tok32ln_ref_of(case, device="cpu", rounding=True, rows=slice(None)):
    c = f64(case, device)
    return tok32ln_ref(c["x"][rows], c["a"][rows], c["dy"][rows], c["w"], c["b"], c["gamma"], c["beta"], rounding=rounding)


# FFN seeds of the fixed-size cases: chosen so that the share of tokens with a pre-activation within NEAR_ZERO of zero (left out
# of the per-element dx check only) stays below MAX_EXCLUDED_SHARE and the last token, the one the negative controls zero, is not
# among them; tests/test_token_ref_cpu.py holds every one of them to both.
MAX_EXCLUDED_SHARE = 0.03
EDGE_TOKENS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
HARD_TOKENS = (53, 4144)
ABI_TOKENS = (1, 17, 53, 4144)
FFN_SEEDS = {(33, "normal"): 4033, (64, "normal"): 2064, (127, "normal"): 2127, (129, "normal"): 2129}


def ffn_seed(T, kind="normal"):
    return FFN_SEEDS.get((T, kind), 1000 + T)


def fixed_ffn_cases():
    """(T, kind) of every FFN case whose size does not depend on the device."""
    out = [(T, "normal") for T in EDGE_TOKENS]
    out += [(T, k) for T in HARD_TOKENS for k in ROW_KINDS]
    out += [(T, "normal") for T in ABI_TOKENS if T not in EDGE_TOKENS and T not in HARD_TOKENS]
    return out
