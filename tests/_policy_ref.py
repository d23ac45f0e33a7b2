"""Host model of the masked policy sampler (include/pmx.h, pmx_policy_sample), independent of the product's code: the hash in
Python integers / numpy uint64, the CDF and the log-probabilities in float64 from the float32-rounded logits.

    h = lowbias32(seed ^ row * 0x9E3779B1 ^ counter * 0x85EBCA77 ^ 0x6A09E667),   u = (h >> 8) / 2^24
    action = the first legal k with cdf_k > u (the last legal k if none), cdf_k = (p_0 + ... + p_k) / total over the legal actions

The kernel and the torch path compute the same in float32, so they may differ from this model only where u falls next to a CDF
boundary: a row is AMBIGUOUS when u lies within AMBIGUOUS_BAND of an interior boundary (cdf_0 .. cdf_3; Stop is always legal, so
cdf_4 = 1 is never interior).  Four boundaries at +-1e-5 make about 8e-5 of all rows ambiguous; the tests allow leaving out at most
AMBIGUOUS_CAP of a call's rows, and test_policy_mask_cpu.py checks from this model alone that the fixed inputs stay below it.
"""
import numpy as np

M32 = 0xFFFFFFFF
AMBIGUOUS_BAND = 1e-5
AMBIGUOUS_CAP = 1e-3
# p = 1e-6 critical values of the chi-square distribution, by degrees of freedom
CHI2_CRIT = {1: 23.93, 2: 27.63, 3: 30.66, 4: 33.38}


def lowbias32(x):
    """lowbias32 of a Python int or a numpy uint64 array of 32-bit values."""
    x = x & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def draw_bits(seed, counter, B):
    """h >> 8 for rows 0 .. B-1 (numpy int64 [B])."""
    rows = np.arange(B, dtype=np.uint64)
    key = (np.uint64(seed & M32) ^ ((rows * np.uint64(0x9E3779B1)) & np.uint64(M32))
           ^ np.uint64((counter * 0x85EBCA77) & M32) ^ np.uint64(0x6A09E667))
    return (lowbias32(key) >> np.uint64(8)).astype(np.int64)


def legal_matrix(legal, B):
    """[B, 5] bool from int32 words (None: everything legal); only the low five bits count and Stop is always legal."""
    if legal is None:
        return np.ones((B, 5), dtype=bool)
    w = (np.asarray(legal).astype(np.int64) & 0x1F) | 0x10
    return ((w[:, None] >> np.arange(5)) & 1).astype(bool)


def sample(logits, legal, seed, counter):
    """logits: float32 [B, 5] (bfloat16 inputs already rounded and widened).  -> action int64 [B], logp float64 [B] of that action,
    logp_all float64 [B, 5] (-inf where masked), ambiguous bool [B]."""
    logits = np.asarray(logits)
    assert logits.dtype == np.float32
    B = logits.shape[0]
    bit = legal_matrix(legal, B)
    z = np.where(bit, logits.astype(np.float64), -np.inf)
    zmax = z.max(axis=1, keepdims=True)
    p = np.exp(z - zmax)
    total = p.sum(axis=1, keepdims=True)
    cdf = np.cumsum(p, axis=1) / total
    u = draw_bits(seed, counter, B).astype(np.float64) / 2.0 ** 24
    ks = np.arange(5)
    first = np.where(bit & (cdf > u[:, None]), ks, 5).min(axis=1)
    last = np.where(bit, ks, -1).max(axis=1)
    action = np.where(first < 5, first, last).astype(np.int64)
    logp_all = (z - zmax) - np.log(total)
    ambiguous = (np.abs(cdf[:, :4] - u[:, None]) <= AMBIGUOUS_BAND).any(axis=1)
    return action, logp_all[np.arange(B), action], logp_all, ambiguous


def greedy(logits, legal):
    """The legal action with the largest logit, the lowest index on ties."""
    logits = np.asarray(logits)
    bit = legal_matrix(legal, logits.shape[0])
    z = np.where(bit, logits.astype(np.float64), -np.inf)
    return z.argmax(axis=1).astype(np.int64)          # numpy's argmax returns the first maximum


def chi_square(actions, probs):
    """Pearson's statistic of the counts of `actions` against probs [5] over the actions with probs > 0, and the degrees of freedom."""
    probs = np.asarray(probs, dtype=np.float64)
    counts = np.bincount(np.asarray(actions), minlength=5).astype(np.float64)
    live = probs > 0
    assert counts[~live].sum() == 0, "a draw outside the support"
    n = counts.sum()
    return float((((counts[live] - n * probs[live]) ** 2) / (n * probs[live])).sum()), int(live.sum()) - 1


# ---- the fixed inputs of the sampler tests (CPU and GPU read the same ones) -------------------------------------------------
SAMPLER_SIZES = (1, 63, 64, 65, 1000, 4099)
MASK_KINDS = ("random", "only_stop", "all", "null", "zero")
LOGIT_KINDS = ("normal", "pm80", "equal")


def round_bf16(x):
    """float32 array rounded to bfloat16 (nearest even) and widened back."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).float().numpy()


def sampler_case(B, bf16, mask_kind, logit_kind):
    """-> logits float32 [B, 5] (rounded to bfloat16 when bf16), legal int32 [B] or None, seed, counter: a pure function of its
    arguments."""
    tag = SAMPLER_SIZES.index(B) * 100 + MASK_KINDS.index(mask_kind) * 10 + LOGIT_KINDS.index(logit_kind) + (5000 if bf16 else 0)
    r = np.random.RandomState(1234 + tag)
    if logit_kind == "normal":
        logits = (r.randn(B, 5) * 2.0).astype(np.float32)
    elif logit_kind == "pm80":
        logits = r.randn(B, 5).astype(np.float32)
        logits[r.rand(B, 5) < 0.3] = 80.0
        logits[r.rand(B, 5) < 0.3] = -80.0
    else:
        logits = np.full((B, 5), np.float32(r.randn()), dtype=np.float32)
    if bf16:
        logits = round_bf16(logits)
    legal = {"random": r.randint(0, 32, size=B).astype(np.int32), "only_stop": np.full(B, 0x10, dtype=np.int32),
             "all": np.full(B, 0x1F, dtype=np.int32), "null": None, "zero": np.zeros(B, dtype=np.int32)}[mask_kind]
    return logits, legal, 0xC0FFEE + tag, 7 + tag


# the distribution test: 2^20 identical rows, masks with 2, 3 and 5 legal actions
DIST_ROWS = 1 << 20
DIST_LOGITS = np.array([0.3, -1.2, 0.9, 0.1, -0.4], dtype=np.float32)
DIST_MASKS = (0x12, 0x15, 0x1F)
DIST_SEED, DIST_COUNTER = 20250101, 3


def dist_probs(mask):
    bit = legal_matrix(np.array([mask]), 1)[0]
    p = np.where(bit, np.exp(DIST_LOGITS.astype(np.float64)), 0.0)
    return p / p.sum()
