"""GPU tests of legal-action masking: pmx_policy_sample against the host model (tests/_policy_ref.py), its distribution and its
contract; pmx_ppo_loss_masked against the float64 torch objective and, under an all-legal mask, against pmx_ppo_loss bit for bit;
the trainer, the replayed step and the vectorised evaluation with mask_illegal."""
import numpy as np
import pytest
import torch

import _policy_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _stream():
    from pmx import _lib
    return _lib.stream(torch.device("cuda", torch.cuda.current_device()))


def _t(logits, bf16):
    return torch.from_numpy(logits).to(DEV).to(torch.bfloat16 if bf16 else torch.float32)


# ---- sampler against the host model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("B", R.SAMPLER_SIZES)
def test_sampler_equals_the_host_model(B, bf16):
    from pmx import mappo
    idx = np.arange(B)
    for mk in R.MASK_KINDS:
        for lk in R.LOGIT_KINDS:
            logits, legal, seed, counter = R.sampler_case(B, bf16, mk, lk)
            want_a, want_lp, _, amb = R.sample(logits, legal, seed, counter)
            z = _t(logits, bf16)
            lg = None if legal is None else torch.from_numpy(legal).to(DEV)
            a, lp = mappo.sample_actions(z, lg, seed=seed, counter=counter)
            assert a.dtype == torch.int64 and lp.dtype == torch.float32 and a.shape == (B,) and lp.shape == (B,)
            got_a, got_lp = a.cpu().numpy(), lp.cpu().numpy().astype(np.float64)
            assert R.legal_matrix(legal, B)[idx, got_a].all(), (mk, lk)                    # always legal
            assert amb.sum() <= R.AMBIGUOUS_CAP * B                                        # rows left out: only up to the cap
            keep = ~amb
            assert np.array_equal(got_a[keep], want_a[keep]), (mk, lk, np.nonzero(got_a != want_a)[0][:8])
            err = np.abs(got_lp[keep] - want_lp[keep]) / (1 + np.abs(want_lp[keep]))
            assert (err <= 2e-6).all(), (mk, lk, float(err.max()))
            a2, lp2 = mappo.sample_actions(z, lg, seed=seed, counter=counter)             # one (seed, counter): the same bits
            assert torch.equal(a, a2) and torch.equal(lp.view(torch.int32), lp2.view(torch.int32))
            if B >= 1000 and mk in ("all", "null", "random") and lk != "pm80":
                a3, _ = mappo.sample_actions(z, lg, seed=seed, counter=counter + 1)       # another counter: other draws
                assert not torch.equal(a, a3)
                a4, _ = mappo.sample_actions(z, lg, seed=seed + 1, counter=counter)
                assert not torch.equal(a, a4)
            g, glp = mappo.sample_actions(z, lg, greedy=True)
            want_g = R.greedy(logits, legal)
            assert np.array_equal(g.cpu().numpy(), want_g), (mk, lk)
            _, _, lp_all, _ = R.sample(logits, legal, 0, 0)
            gerr = np.abs(glp.cpu().numpy().astype(np.float64) - lp_all[idx, want_g]) / (1 + np.abs(lp_all[idx, want_g]))
            assert (gerr <= 2e-6).all()


@pytest.mark.parametrize("mask", R.DIST_MASKS)
def test_sampler_distribution_passes_chi_square(mask):
    from pmx import mappo
    z = torch.from_numpy(R.DIST_LOGITS).to(DEV).expand(R.DIST_ROWS, 5).contiguous()
    lg = torch.full((R.DIST_ROWS,), mask, dtype=torch.int32, device=DEV)
    a, _ = mappo.sample_actions(z, lg, seed=R.DIST_SEED, counter=R.DIST_COUNTER)
    stat, dof = R.chi_square(a.cpu().numpy(), R.dist_probs(mask))
    print(f"mask {mask:#x}: chi-square {stat:.2f} at {dof} degrees of freedom (critical {R.CHI2_CRIT[dof]})")
    assert dof == bin(mask).count("1") - 1
    assert stat < R.CHI2_CRIT[dof]


# ---- contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 65, 1000])
def test_sampler_writes_its_outputs_in_full_and_nothing_else(B):
    from pmx import _lib
    G = 64
    logits, legal, seed, counter = R.sampler_case(B, False, "random", "normal")
    z, lg = torch.from_numpy(logits).to(DEV), torch.from_numpy(legal).to(DEV)
    z0, lg0 = z.clone(), lg.clone()
    CAN_A, CAN_L = -0x0123456789ABCDEF, -12345.625
    act = torch.full((G + B + G,), CAN_A, dtype=torch.int64, device=DEV)
    lp = torch.full((G + B + G,), CAN_L, dtype=torch.float32, device=DEV)
    _lib.call("pmx_policy_sample", z.data_ptr(), 0, lg.data_ptr(), B, seed, counter, 0, act.data_ptr() + 8 * G, lp.data_ptr() + 4 * G, _stream())
    torch.cuda.synchronize()
    for t, can in ((act, CAN_A), (lp, CAN_L)):
        assert bool((t[:G] == can).all()) and bool((t[G + B:] == can).all())
        assert bool((t[G:G + B] != can).all())
    assert bool(((act[G:G + B] >= 0) & (act[G:G + B] < 5)).all())
    assert torch.equal(z, z0) and torch.equal(lg, lg0)
    # logp_dev may be NULL: the actions are the same
    act2 = torch.full((G + B + G,), CAN_A, dtype=torch.int64, device=DEV)
    _lib.call("pmx_policy_sample", z.data_ptr(), 0, lg.data_ptr(), B, seed, counter, 0, act2.data_ptr() + 8 * G, None, _stream())
    assert torch.equal(act, act2)


def test_sampler_argument_errors_and_empty_batch():
    from pmx import _lib
    lib = _lib.load()
    z = torch.zeros(4, 5, device=DEV)
    act = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    lp = torch.full((4,), -7.0, device=DEV)
    st = _stream()
    INVALID, OK = -1, 0
    assert lib.pmx_policy_sample(None, 0, None, 4, 1, 1, 0, act.data_ptr(), lp.data_ptr(), st) == INVALID
    assert lib.pmx_policy_sample(z.data_ptr(), 0, None, 4, 1, 1, 0, None, lp.data_ptr(), st) == INVALID
    assert lib.pmx_policy_sample(z.data_ptr(), 0, None, -1, 1, 1, 0, act.data_ptr(), lp.data_ptr(), st) == INVALID
    assert lib.pmx_policy_sample(z.data_ptr(), 0, None, 0, 1, 1, 0, act.data_ptr(), lp.data_ptr(), st) == OK
    torch.cuda.synchronize()
    assert bool((act == -7).all()) and bool((lp == -7.0).all())
    with pytest.raises(_lib.PmxError):
        _lib.call("pmx_policy_sample", None, 0, None, 4, 1, 1, 0, act.data_ptr(), None, st)


# ---- masked loss against the float64 torch objective -------------------------------------------------------------------------
def _loss_inputs(B, paired, dtype):
    g = torch.Generator(device=DEV).manual_seed(B * 4 + 2 * int(paired) + int(dtype == torch.bfloat16))
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    logits = (rn(B, 5) * 2).to(dtype)
    values = rn(B // 2 if paired else B)
    act = torch.randint(0, 5, (B,), device=DEV, generator=g)
    legal = torch.randint(0, 32, (B,), device=DEV, generator=g, dtype=torch.int32)      # (many words leave the stored action out)
    old_logp = torch.log_softmax(rn(B, 5), -1).gather(1, act.view(-1, 1)).squeeze(1)
    return logits, values, act, legal, old_logp, rn(B) * 3 + 0.5, rn(B)


def _masked_call(logits, values, act, legal, old_logp, adv, ret, clip_eps, ent_coef):
    """-> stats [5], dlogits, dvalues of pmx_ppo_loss_masked through its autograd function."""
    from pmx import mappo
    z, v = logits.clone().requires_grad_(True), values.clone().requires_grad_(True)
    stats = mappo._PPOLossMaskedFn.apply(z, v, act, legal, old_logp, adv, ret, clip_eps, ent_coef, mappo.VF_COEF)
    stats[4].backward()
    return stats.detach(), z.grad, v.grad


LOSS_CASES = [(2, False), (2, True), (5, False), (1023, False), (1024, False), (1024, True), (1025, False), (2 * 4099, False), (2 * 4099, True)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,paired", LOSS_CASES)
def test_masked_loss_matches_the_float64_torch_objective(B, paired, dtype):
    """Bounds of test_fused_ppo_loss_matches_the_torch_objective: scalars 2e-5; dlogits 1e-5 (float32) / 1e-2 (bfloat16) and
    dvalues 1e-5 of the largest reference gradient."""
    from pmx import mappo
    logits, values, act, legal, old_logp, adv, ret = _loss_inputs(B, paired, dtype)
    clip_eps, ent_coef = 0.15, 0.02
    w = legal.long() | 0x10 | (1 << act)
    bit = ((w[:, None] >> torch.arange(5, device=DEV)) & 1).bool()
    assert bool((~((legal.long()[:, None] >> act[:, None]) & 1).bool()).any()) or B < 5       # an action masked out in the word ...
    # the reference formulas in float64 from the same (already rounded) inputs, illegal logits at -inf
    z = logits.detach().double().requires_grad_(True)
    v = values.detach().double().requires_grad_(True)
    zm = z.masked_fill(~bit, float("-inf"))
    norm = zm - zm.logsumexp(-1, keepdim=True)
    probs = torch.softmax(zm, -1)
    logp = norm.gather(1, act.view(-1, 1)).squeeze(1)                                        # ... is treated as legal: finite
    ent = -(norm.masked_fill(~bit, 0.0) * probs).sum(-1)
    vv = v.repeat_interleave(2) if paired else v
    a = adv.double()
    na = (a - a.mean()) / (a.std() + 1e-8)
    ratio = (logp - old_logp.double()).exp()
    pg = -torch.min(na * ratio, na * torch.clamp(ratio, 1 - clip_eps, 1 + clip_eps)).mean()
    vl = 0.5 * ((vv - ret.double()) ** 2).mean()
    loss = pg + mappo.VF_COEF * vl - ent_coef * ent.mean()
    loss.backward()
    cf = ((ratio - 1).abs() > clip_eps).double().mean()
    ref = torch.stack([pg, vl, ent.mean(), cf, loss]).detach()
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(z.grad).all())
    gtol = 1e-5 if dtype == torch.float32 else 1e-2
    dev_scalars = (torch.tensor(clip_eps, device=DEV), torch.tensor(ent_coef, device=DEV))
    for ce, ec in ((clip_eps, ent_coef), dev_scalars):                                       # host and device scalars
        stats, dz, dv = _masked_call(logits, values, act, legal, old_logp, adv, ret, ce, ec)
        assert torch.allclose(stats.double(), ref, rtol=2e-5, atol=2e-5), (stats, ref)
        assert bool((dz[~bit] == 0).all()) and bool(torch.isfinite(dz).all())                # exactly 0 at masked entries
        assert float((dz.double() - z.grad).abs().max()) <= gtol * (float(z.grad.abs().max()) + 1e-12)
        assert float((dv.double() - v.grad).abs().max()) <= 1e-5 * (float(v.grad.abs().max()) + 1e-12)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,paired", LOSS_CASES)
def test_all_legal_mask_equals_the_unmasked_kernel_bit_for_bit(B, paired, dtype):
    from pmx import mappo
    logits, values, act, _, old_logp, adv, ret = _loss_inputs(B, paired, dtype)
    z, v = logits.clone().requires_grad_(True), values.clone().requires_grad_(True)
    stats = mappo._PPOLossFn.apply(z, v, act, old_logp, adv, ret, 0.15, 0.02, mappo.VF_COEF)
    stats[4].backward()
    bits = lambda t: t.detach().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
    for word in (0x1F, -1, 0x0F | (0x7F << 5)):          # every bit; only the low five are read; Stop is set whatever the word says
        legal = torch.full((B,), word, dtype=torch.int32, device=DEV)
        s2, dz2, dv2 = _masked_call(logits, values, act, legal, old_logp, adv, ret, 0.15, 0.02)
        assert torch.equal(bits(stats), bits(s2)), word
        assert torch.equal(bits(z.grad), bits(dz2)) and torch.equal(bits(v.grad), bits(dv2)), word


# ---- trainer -----------------------------------------------------------------------------------------------------------------
def _trainer(red, **kw):
    from pmx import trainer
    args = dict(n_envs=64, horizon=8, minibatch=128, epochs=2, seed=4, length=40, opponent="random", mask_illegal=True)
    args.update(kw)
    tr = trainer.VecMAPPOTrainer("tinyCapture", **args)
    mode = args["opponent"]
    tr._pick_opponent = lambda: (mode, red)
    return tr


def _host_start_masks(red):
    """[2] canonical int32 words of the learners' start cells, from the layout's walls."""
    import pmx
    lay = pmx.get_layout("tinyCapture")
    out = []
    for i in ([0, 2] if red else [1, 3]):
        x, y = (int(c) for c in lay.starts[i])
        n, e, s, w = (not lay.is_wall(x, y + 1), not lay.is_wall(x + 1, y), not lay.is_wall(x, y - 1), not lay.is_wall(x - 1, y))
        if red:
            e, w = w, e
        out.append(int(n) | int(e) << 1 | int(s) << 2 | int(w) << 3 | 0x10)
    return out


@pytest.mark.parametrize("red", [False, True])
def test_rollout_draws_only_legal_actions_and_stores_their_masks(red):
    tr = _trainer(red, opponent="self")
    tr.rollout()
    assert tr.stats["play_as_red"] == red
    legal, act = tr.legal_buf.long(), tr.act_buf
    assert bool((((legal | 0x10) >> act) & 1).bool().all())
    want = torch.tensor(_host_start_masks(red), dtype=torch.int32, device=tr.device)
    assert torch.equal(tr.legal_buf[0], want[None].expand(64, 2))
    assert bool((tr.legal_buf & 0x10).bool().all()) and bool((tr.legal_buf < 32).all())
    assert len(torch.unique(tr.legal_buf)) > 1                              # the agents moved: other cells, other masks
    assert bool(torch.isfinite(tr.logp_buf).all()) and float(tr.logp_buf.max()) <= 0.0
    # the log-probability stored is the masked one: what evaluate gives under the stored mask
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        z = tr.model.logits(tr._net_in(tr.obs_buf[3].reshape((-1,) + tr.obs_shape))).float()
    bit = ((tr.legal_buf[3].reshape(-1).long()[:, None] >> torch.arange(5, device=tr.device)) & 1).bool()
    lp = torch.log_softmax(z.masked_fill(~bit, float("-inf")), -1).gather(1, act[3].reshape(-1, 1)).squeeze(1)
    assert torch.allclose(lp, tr.logp_buf[3].reshape(-1), rtol=0, atol=5e-2)               # (bf16 inference, two passes)
    assert tr.sample_counter == 2 * tr.T                                    # learner and opponent: one call each per tick
    tr.env.close()


@pytest.mark.parametrize("variant,red", [("eager", False), ("eager", True), ("graph", True), ("gather", False), ("ippo", True),
                                         ("unpaired", False), ("float32", True)])
def test_update_under_masks_is_finite_on_every_path(variant, red):
    kw = {"eager": {}, "graph": dict(use_graph=True), "gather": dict(use_graph=True), "ippo": dict(algorithm="ippo"),
          "unpaired": dict(paired_minibatches=False), "float32": dict(use_autocast=False)}[variant]
    tr = _trainer(red, **kw)
    if variant == "graph":
        tr.graph_gather = False
    tr.rollout()
    tr.compute_gae()
    before = tr.learner.bucket.data.clone()
    tr.update(max_steps=2)
    for k in ("pg", "vl", "entropy", "loss", "grad_norm"):
        assert bool(torch.isfinite(tr.stats[k]).all()), k
    assert tr.stats["optimizer_steps"] == 2
    assert bool(torch.isfinite(tr.learner.bucket.data).all()) and not torch.equal(before, tr.learner.bucket.data)
    if variant in ("graph", "gather"):
        assert "legal" in tr.learner._g_in and tr.learner._g_in["legal"].dtype == torch.int32
    # entropy under masks is at most that of the legal actions of the widest mask
    assert 0.0 < float(tr.stats["entropy"]) <= float(np.log(5)) + 1e-3
    tr.env.close()


def test_masked_graph_step_equals_masked_eager_step():
    """test_graph_captured_step_equals_eager_step's bounds, on a masked rollout's samples: float32, three steps."""
    from pmx import mappo
    tr = _trainer(False, use_autocast=False)
    tr.rollout()
    tr.compute_gae()
    B = 128
    S = tr.T * tr.N * 2
    obs = tr.obs_buf.view((S,) + tr.obs_shape)[:B].float()
    merged = tr.merged_buf.view((S // 2,) + tr.obs_shape)[:B // 2].float()
    act, logp, legal = tr.act_buf.view(S)[:B], tr.logp_buf.view(S)[:B], tr.legal_buf.view(S)[:B]
    adv, ret = tr.adv_buf.view(S)[:B], tr.ret_buf.view(S)[:B]
    torch.manual_seed(3)
    a = mappo.MAPPOAgent(tr.obs_shape, 5, 2).cuda()
    b = mappo.MAPPOAgent(tr.obs_shape, 5, 2).cuda()
    b.load_state_dict(a.state_dict())
    la, lb = mappo.PPOLearner(a, lr=2e-4), mappo.PPOLearner(b, lr=2e-4)
    lb.capture(B, tr.obs_shape, torch.float32, merged_batch=B // 2, masked=True)
    assert torch.equal(la.bucket.data, lb.bucket.data)
    for k in range(3):
        sa = la.update_minibatch(obs, merged, act, logp, adv, ret, 0.15, 0.02, legal=legal)
        sb = lb.update_minibatch_graph(obs, merged, act, logp, adv, ret, 0.15, 0.02, legal=legal)
        assert torch.allclose(sa["loss"], sb["loss"], rtol=1e-4, atol=1e-6), k
        assert torch.allclose(sa["grad_norm"], sb["grad_norm"], rtol=1e-3), k
    assert torch.allclose(la.bucket.data, lb.bucket.data, rtol=1e-3, atol=2e-5)
    assert torch.allclose(la.ema, lb.ema, rtol=1e-3, atol=2e-5)
    with pytest.raises(ValueError):
        lb.update_minibatch_graph(obs, merged, act, logp, adv, ret, 0.15, 0.02)            # a masked graph wants its masks
    tr.env.close()


def test_flag_off_calls_neither_new_symbol(monkeypatch):
    from pmx import _lib
    names = []
    real = _lib.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", recording)
    tr = _trainer(False, mask_illegal=False, opponent="self")
    assert not hasattr(tr, "legal_buf")
    tr.rollout()
    tr.compute_gae()
    tr.update(max_steps=2)
    assert "pmx_ppo_loss" in names and "pmx_step" in names
    assert "pmx_policy_sample" not in names and "pmx_ppo_loss_masked" not in names
    names.clear()
    tr2 = _trainer(False, opponent="self")
    tr2.rollout()
    tr2.compute_gae()
    tr2.update(max_steps=2)
    assert "pmx_policy_sample" in names and "pmx_ppo_loss_masked" in names and "pmx_ppo_loss" not in names
    tr.env.close()
    tr2.env.close()


def test_checkpoint_carries_the_flag_and_the_counter(tmp_path):
    off, on = _trainer(False, mask_illegal=False), _trainer(False)
    on.rollout()
    p_off, p_on = str(tmp_path / "off.pt"), str(tmp_path / "on.pt")
    off.save_full(p_off)
    on.save_full(p_on)
    ck = torch.load(p_off, weights_only=True)
    assert "mask_illegal" not in ck and "sample_counter" not in ck
    ck = torch.load(p_on, weights_only=True)
    assert ck["mask_illegal"] == 1 and ck["sample_counter"] == on.T
    with pytest.raises(ValueError):
        off.load_full(p_on)
    with pytest.raises(ValueError):
        on.load_full(p_off)
    fresh = _trainer(False)
    fresh.load_full(p_on)
    assert fresh.sample_counter == on.T
    off.load_full(p_off)
    for t in (off, on, fresh):
        t.env.close()


def test_vectorised_evaluation_under_masks():
    from pmx import mappo, trainer
    torch.manual_seed(0)
    import pmx
    lay = pmx.get_layout("tinyCapture")
    m = mappo.MAPPOAgent((8, lay.height, lay.width), 5, 2).cuda()
    for opp in ("random", "baseline"):
        out = trainer.evaluate_vectorized(m, "tinyCapture", 256, opp, length=30, mask_illegal=True)
        assert len(out) == 3 and all(np.isfinite(x) for x in out) and 0.0 <= out[2] <= 1.0
