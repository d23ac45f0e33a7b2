"""CPU suite of legal-action masking: the torch paths of act / evaluate / ppo_loss under masks against
torch.distributions.Categorical on -inf-filled logits, the mask canonicalisation, mappo.sample_actions on the CPU against the host
model (tests/_policy_ref.py), and -- from the host model alone -- that the fixed inputs of the GPU tests stay inside the ambiguity
cap and the chi-square bound before any GPU run."""
import numpy as np
import pytest
import torch

import _policy_ref as R

SHAPE = (8, 7, 20)      # tinyCapture's planes


def _model():
    from pmx import mappo
    torch.manual_seed(11)
    torch.set_num_threads(2)
    return mappo.MAPPOAgent(SHAPE, 5, 2)


def _batch(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    obs = (torch.rand((B,) + SHAPE, generator=g) < 0.2).float()
    merged = (torch.rand((B // 2,) + SHAPE, generator=g) < 0.2).float()
    legal = torch.randint(0, 32, (B,), generator=g, dtype=torch.int32)
    return obs, merged, legal


def _filled(logits, legal, action=None):
    """-inf-filled logits by bit arithmetic of the test's own (Stop always legal, the stored action too)."""
    w = legal.long() | 0x10
    if action is not None:
        w = w | (1 << action)
    bit = torch.stack([(w >> k) & 1 for k in range(5)], dim=1).bool()
    return logits.masked_fill(~bit, float("-inf")), bit


def test_masked_torch_paths_equal_categorical_on_filled_logits():
    from pmx import mappo
    m = _model()
    B = 16
    obs, merged, legal = _batch(B)
    with torch.no_grad():
        raw = m.logits(obs).float()
    # act: the CPU sampler's log-probability is Categorical's of the action it drew, and the action is legal
    a, lp = m.act(obs, legal=legal, seed=3, counter=5)
    zf, bit = _filled(raw, legal)
    assert bool(bit.gather(1, a.view(-1, 1)).all())
    cat = torch.distributions.Categorical(logits=zf)
    assert torch.allclose(lp, cat.log_prob(a), rtol=0, atol=2e-6)
    a2, lp2 = m.act(obs, legal=legal, seed=3, counter=5)
    assert torch.equal(a, a2) and torch.equal(lp, lp2)
    g = m.get_deterministic_action(obs, legal=legal)
    assert torch.equal(g, zf.argmax(dim=-1))
    # evaluate: log-prob and entropy
    vals, logp, ent = m.evaluate(obs, merged, a, legal=legal)
    assert torch.allclose(logp, cat.log_prob(a), rtol=0, atol=2e-6)
    assert torch.allclose(ent, cat.entropy(), rtol=0, atol=2e-6)
    # ppo_loss: the reference's formulas on Categorical's log-prob and entropy
    old_logp, adv, ret = lp + 0.1 * torch.randn(B), torch.randn(B), torch.randn(B)
    clip_eps, ent_coef = 0.15, 0.02
    loss, st = mappo.ppo_loss(m, obs, merged, a, old_logp, adv, ret, clip_eps, ent_coef, legal=legal)
    with torch.no_grad():
        v = m.value(merged).float().repeat_interleave(2)
        na = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = (cat.log_prob(a) - old_logp).exp()
        pg = -torch.min(na * ratio, na * ratio.clamp(1 - clip_eps, 1 + clip_eps)).mean()
        want = pg + mappo.VF_COEF * 0.5 * ((v - ret) ** 2).mean() - ent_coef * cat.entropy().mean()
    assert abs(float(loss.detach()) - float(want)) <= 1e-5 * (1 + abs(float(want))), (float(loss.detach()), float(want))
    assert torch.isfinite(st["entropy"])


def test_gradients_at_masked_logits_are_exactly_zero(monkeypatch):
    from pmx import mappo
    m = _model()
    B = 16
    obs, merged, legal = _batch(B, seed=1)
    act = torch.randint(0, 5, (B,), generator=torch.Generator().manual_seed(2))
    seen = {}
    real = mappo.MAPPOAgent.logits

    def logits_with_grad(self, x):
        z = real(self, x)
        z.retain_grad()
        seen["z"] = z
        return z
    monkeypatch.setattr(mappo.MAPPOAgent, "logits", logits_with_grad)
    loss, _ = mappo.ppo_loss(m, obs, merged, act, -1.5 * torch.ones(B), torch.randn(B), torch.randn(B), 0.15, 0.02, legal=legal)
    loss.backward()
    grad = seen["z"].grad
    _, bit = _filled(grad, legal, act)
    assert bool(torch.isfinite(grad).all())
    assert (~bit).any() and float(grad[~bit].abs().max()) == 0.0
    assert float(grad[bit].abs().min()) > 0.0                  # and the legal ones do receive one
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)


def test_all_legal_mask_equals_the_unmasked_call_bit_for_bit():
    from pmx import mappo
    m = _model()
    B = 16
    obs, merged, _ = _batch(B, seed=2)
    full = torch.full((B,), 0x1F, dtype=torch.int32)
    act = torch.randint(0, 5, (B,), generator=torch.Generator().manual_seed(3))
    old_logp, adv, ret = -1.6 * torch.ones(B), torch.randn(B), torch.randn(B)
    out = []
    for legal in (None, full):
        m.zero_grad(set_to_none=True)
        kw = {} if legal is None else {"legal": legal}
        vals, logp, ent = m.evaluate(obs, merged, act, **kw)
        loss, st = mappo.ppo_loss(m, obs, merged, act, old_logp, adv, ret, 0.15, 0.02, **kw)
        loss.backward()
        out.append((vals.detach(), logp.detach(), ent.detach(), loss.detach(), [p.grad.clone() for p in m.parameters()]))
    for x, y in zip(out[0][:4], out[1][:4]):
        assert torch.equal(x, y)
    for x, y in zip(out[0][4], out[1][4]):
        assert torch.equal(x, y)
    assert torch.equal(m.get_deterministic_action(obs), m.get_deterministic_action(obs, legal=full))


def test_canonicalize_legal_swaps_east_and_west_for_red_only():
    from pmx import mappo
    bits = torch.arange(32, dtype=torch.uint8)
    blue = mappo.canonicalize_legal(bits, False)
    red = mappo.canonicalize_legal(bits, True)
    assert blue.dtype == torch.int32 and red.dtype == torch.int32
    assert torch.equal(blue, bits.to(torch.int32))
    for b in range(32):
        want = (b & 0b10101) | (((b >> 1) & 1) << 3) | (((b >> 3) & 1) << 1)
        assert int(red[b]) == want == mappo.canonicalize_legal(b, True)
        assert mappo.canonicalize_legal(b, False) == b
        # the mask of the canonical frame admits exactly the canonicalised actions
        for a in range(5):
            assert ((want >> mappo.canonicalize_action(a, True)) & 1) == ((b >> a) & 1)
    assert torch.equal(mappo.canonicalize_legal(bits.view(4, 8) | 0xE0, True), red.view(4, 8))     # only the low five bits are read


@pytest.mark.parametrize("bf16", [False, True])
def test_cpu_sampler_equals_the_host_model_off_the_ambiguous_rows(bf16):
    from pmx import mappo
    for B in (65, 1000):
        for mk in R.MASK_KINDS:
            for lk in R.LOGIT_KINDS:
                logits, legal, seed, counter = R.sampler_case(B, bf16, mk, lk)
                want_a, want_lp, _, amb = R.sample(logits, legal, seed, counter)
                t_logits = torch.from_numpy(logits).to(torch.bfloat16 if bf16 else torch.float32)
                t_legal = None if legal is None else torch.from_numpy(legal)
                a, lp = mappo.sample_actions(t_logits, t_legal, seed=seed, counter=counter)
                assert a.dtype == torch.int64 and lp.dtype == torch.float32
                keep = ~amb
                assert np.array_equal(a.numpy()[keep], want_a[keep]), (B, mk, lk)
                bit = R.legal_matrix(legal, B)
                assert bit[np.arange(B), a.numpy()].all()
                got_lp = lp.numpy().astype(np.float64)[keep]
                assert (np.abs(got_lp - want_lp[keep]) <= 2e-6 * (1 + np.abs(want_lp[keep]))).all()
                g, _ = mappo.sample_actions(t_logits, t_legal, greedy=True)
                assert np.array_equal(g.numpy(), R.greedy(logits, legal))
                b, _ = mappo.sample_actions(t_logits, t_legal, seed=seed, counter=counter + 1)
                if B == 1000 and mk in ("all", "null") and lk == "normal":
                    assert not torch.equal(a, b)


def test_fixed_sampler_inputs_stay_below_the_ambiguity_cap():
    """Every call the GPU test makes may leave out at most AMBIGUOUS_CAP of its rows; with the fixed seeds none leaves out more."""
    rows = amb_rows = 0
    for B in R.SAMPLER_SIZES:
        for bf16 in (False, True):
            for mk in R.MASK_KINDS:
                for lk in R.LOGIT_KINDS:
                    logits, legal, seed, counter = R.sampler_case(B, bf16, mk, lk)
                    a, _, _, amb = R.sample(logits, legal, seed, counter)
                    assert R.legal_matrix(legal, B)[np.arange(B), a].all()
                    assert amb.sum() <= R.AMBIGUOUS_CAP * B, (B, bf16, mk, lk, int(amb.sum()))
                    rows += B
                    amb_rows += int(amb.sum())
    assert amb_rows <= R.AMBIGUOUS_CAP * rows
    print(f"ambiguous rows: {amb_rows} of {rows}")


@pytest.mark.parametrize("mask", R.DIST_MASKS)
def test_host_model_draws_pass_the_chi_square_bound(mask):
    logits = np.broadcast_to(R.DIST_LOGITS, (R.DIST_ROWS, 5)).copy()
    a, _, _, amb = R.sample(logits, np.full(R.DIST_ROWS, mask, dtype=np.int32), R.DIST_SEED, R.DIST_COUNTER)
    stat, dof = R.chi_square(a, R.dist_probs(mask))
    assert dof == bin(mask | 0x10).count("1") - 1
    print(f"mask {mask:#x}: chi-square {stat:.2f} at {dof} degrees of freedom, ambiguous share {amb.mean():.2e}")
    assert stat < R.CHI2_CRIT[dof]
    assert amb.mean() <= R.AMBIGUOUS_CAP
