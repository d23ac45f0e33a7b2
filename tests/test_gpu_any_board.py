"""GPU tests of the fused actor tower and critic projector (csrc/pmx_actor.hip) on every kind of board of their domain: W in
8..32, H in 3..32, H * W <= 640 -- tile counts 2 .. 44, served by the tile-count buckets 10, 11, 16, 28, 36, 44.  Boards are
(H, W) with synthetic planes; references and bounds are those of tests/test_gpu_actor_tower.py and of
tests/test_gpu_trainer.py::test_fused_projector_matches_torch (tests/_tower_ref.py).

The boards: (3, 8) 2 tiles, the smallest board pmx_create takes; (12, 14) 12 tiles, the first count above the one-wave
kernels; (16, 14) 16 tiles, the largest of bucket 16; (13, 18) 17 tiles, the first count above 16 and the smallest of bucket
28; (16, 27) 29 and (18, 30) 36 tiles, the ends of bucket 36; (16, 32) 34 tiles, BASELINE config 5's board at the maximum
width; (17, 32) 37 and (32, 20) 44 tiles, the ends of bucket 44; (32, 18) 40 tiles, the maximum height; (20, 32) 43 tiles,
640 cells; (9, 16) runs the 11-tile kernels with another geometry than smallCapture's (a control: it has always passed)."""
import copy
import ctypes as C

import pytest
import torch

import _tower_ref as R

pytestmark = pytest.mark.gpu

SMALL = [(3, 8), (12, 14), (16, 14), (9, 16)]
LARGE = [(13, 18), (16, 27), (16, 32), (18, 30), (17, 32), (32, 18), (20, 32), (32, 20)]
BOARDS = SMALL + LARGE


def test_boards_cover_every_bucket_end():
    got = {b: R.tiles(*b) for b in BOARDS}
    assert [got[b] for b in BOARDS] == [2, 12, 16, 11, 17, 29, 34, 36, 37, 40, 43, 44]
    assert {R.bucket(n) for n in got.values()} == {11, 16, 28, 36, 44}
    assert all(R.in_domain(*b) for b in BOARDS)


_CANARY = 0x5A


@pytest.mark.parametrize("board,B", [(b, 5) for b in BOARDS] + [((16, 32), 67), ((3, 8), 1), ((20, 32), 1)])
def test_kernels_stay_inside_the_sizes_they_are_given(board, B):
    """Forward (training and inference variant) and backward through the C ABI, with save, scratch and inference scratch cut to
    exactly pmx_actor_sizes out of a buffer of canary bytes: no byte in front of or behind any of them changes, the features and
    the gradient come out finite, and an unsupported board is refused without a write."""
    import pmx
    from pmx import _lib, actor_tower
    H, W = board
    lib = _lib.load()
    assert lib.pmx_actor_supported(H, W) == 1
    sv, sc, si = actor_tower._sizes(H, W, B)
    m = R.model(H, W, seed=2)
    pack = actor_tower.pack_params(actor_tower._tower_params(m.actor_backbone))
    obs = R.planes(B, H, W, seed=3).to(torch.uint8)
    guard = 1 << 16
    bufs = {}
    for name, n in (("save", sv), ("scratch", sc), ("infer", si)):
        bufs[name] = torch.full((guard + n + guard,), _CANARY, dtype=torch.uint8, device="cuda")
    ptr = lambda name: bufs[name].data_ptr() + guard
    feat = torch.full((B, H * W, 32), float("nan"), dtype=torch.bfloat16, device="cuda")
    feat_i = torch.full_like(feat, float("nan"))
    dfeat = (torch.randn(B, H * W, 32, device="cuda") * 0.1).to(torch.bfloat16)
    grad = torch.full((_lib.ACTOR_GRAD_FLOATS,), float("nan"), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.pmx_actor_forward(obs.data_ptr(), _lib.OBS_U8, pack.data_ptr(), feat.data_ptr(), ptr("save"), None, B, H, W, st) == 0
    assert lib.pmx_actor_forward(obs.data_ptr(), _lib.OBS_U8, pack.data_ptr(), feat_i.data_ptr(), None, ptr("infer"), B, H, W, st) == 0
    assert lib.pmx_actor_backward(obs.data_ptr(), _lib.OBS_U8, pack.data_ptr(), ptr("save"), dfeat.data_ptr(), ptr("scratch"), grad.data_ptr(),
                                  B, H, W, st) == 0
    torch.cuda.synchronize()
    for name, n in (("save", sv), ("scratch", sc), ("infer", si)):
        assert bool((bufs[name][:guard] == _CANARY).all()), f"written in front of {name}"
        assert bool((bufs[name][guard + n:] == _CANARY).all()), f"written past the end of {name}"
    assert bool(torch.isfinite(feat.float()).all()) and bool(torch.isfinite(grad).all())
    assert torch.equal(feat, feat_i), "training and inference forward differ"
    # a board above 640 cells: refused, nothing written
    before = feat.clone()
    PMX_ERR_UNSUPPORTED = lib.pmx_actor_forward(obs.data_ptr(), _lib.OBS_U8, pack.data_ptr(), feat.data_ptr(), ptr("save"), None, 1, 26, 25, st)
    assert PMX_ERR_UNSUPPORTED != 0
    torch.cuda.synchronize()
    assert torch.equal(feat, before)


def _emulation(m, obs):
    """The rounding-exact emulation the forward is held to.  Up to 64 samples it is evaluated in float64 on the CPU: a float32
    evaluation carries its own accumulation-order error, which moves values across bf16 rounding boundaries just as the
    kernel's does -- two float32 evaluations of this emulation with different convolution algorithms differ from each other by
    0.4e-4 .. 1.4e-4 of the largest feature in the mean, most of the 2e-4 allowed, so against a float32 reference the outcome
    depended on the algorithm the library picked on the day.  Against float64 only the kernel's own error is measured, with
    the same bounds.  The 2 111-sample case keeps the float32 GPU evaluation (float64 on the CPU would take most of a minute)."""
    if obs.shape[0] > 64:
        return R.emulated_tower(m, obs)
    m64 = copy.deepcopy(m).cpu().double()
    return R.emulated_tower(m64, obs.cpu().double(), ste=True).float().to(obs.device)


def _check_forward(m, obs, dtype):
    from pmx import actor_tower
    B, _, H, W = obs.shape
    with torch.no_grad():
        feat = actor_tower.actor_tower(m.actor_backbone, obs.to(dtype))              # [B, HW, 32]
        got = feat.float().permute(0, 2, 1).reshape(B, 32, H, W)
        emu = _emulation(m, obs)
        exact = m.actor_backbone[:-1](obs)
    scale = emu.abs().max().item()
    err_max, err_mean = (got - emu).abs().max().item(), (got - emu).abs().mean().item()
    rel = ((got - exact).norm() / exact.norm()).item()
    print(f"forward {H}x{W} B={B} {dtype}: max {err_max / scale:.3e} mean {err_mean / scale:.3e} of the largest feature, rel {rel:.3e}")
    assert err_max <= scale * 2 ** -6, "forward differs from the rounding-exact emulation"
    assert err_mean <= scale * 2e-4
    assert rel < 3e-2, rel


@pytest.mark.parametrize("board", BOARDS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.uint8])
def test_tower_forward_matches_torch(board, dtype):
    from pmx import actor_tower
    H, W = board
    assert actor_tower.tower_supported(H, W)
    m = R.model(H, W)
    for B in (1, 5):
        obs = R.planes(B, H, W, seed=B)
        _check_forward(m, obs, dtype)
    # the model's logits through the fused path == through the library path, to bf16 accuracy
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert m._use_fused_tower(obs.to(dtype))
        a = m.logits(obs.to(torch.bfloat16)).float()
        m.fused_tower = False
        b = m.logits(obs.to(torch.bfloat16)).float()
        m.fused_tower = True
    assert ((a - b).norm() / b.norm()).item() < 5e-2


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.uint8])
def test_tower_forward_above_the_grid_cap(dtype):
    """2 111 samples of the 32 x 16 board exceed the 2 048 one-sample blocks the eight-waves-per-sample kernel launches, so some
    blocks walk two samples"""
    H, W = 16, 32
    _check_forward(R.model(H, W), R.planes(2111, H, W), dtype)


@pytest.mark.parametrize("board,B", [((16, 32), 3), ((16, 32), 67), ((20, 32), 9), ((32, 18), 9)] + [(b, 5) for b in SMALL]
                         + [((13, 18), 5), ((16, 27), 5), ((18, 30), 5), ((17, 32), 5), ((32, 20), 5)])
def test_tower_backward_matches_autograd(board, B):
    """All 28 parameter gradients within 3e-2 relative (Frobenius) of float64 CPU autograd through the straight-through emulation"""
    from pmx import actor_tower
    H, W = board
    m = R.model(H, W, seed=3)
    obs = R.planes(B, H, W, seed=4)
    g = torch.Generator(device="cuda").manual_seed(5)
    dfeat = torch.randn(B, 32, H, W, device="cuda", generator=g) * 0.1
    params = actor_tower._tower_params(m.actor_backbone)
    feat = actor_tower.actor_tower(m.actor_backbone, obs.to(torch.bfloat16))
    loss = (feat.float().permute(0, 2, 1).reshape(B, 32, H, W) * dfeat).sum()
    got = torch.autograd.grad(loss, params)
    mc = R.model(H, W, seed=3).cpu().double()
    want = torch.autograd.grad((R.emulated_tower(mc, obs.cpu(), ste=True) * dfeat.cpu().double()).sum(),
                               actor_tower._tower_params(mc.actor_backbone))
    assert len(got) == len(want) == 28
    worst = 0.0
    for p, a, b in zip(params, got, want):
        assert a.shape == b.shape and a.dtype == p.dtype
        rel = ((a.cpu().double() - b).norm() / (b.norm() + 1e-12)).item()
        worst = max(worst, rel)
    print(f"backward {H}x{W} B={B}: worst relative error {worst:.3e}")
    for p, a, b in zip(params, got, want):
        rel = ((a.cpu().double() - b).norm() / (b.norm() + 1e-12)).item()
        assert rel < 3e-2, (tuple(p.shape), rel)
    assert worst > 0.0


def test_tower_backward_of_a_large_batch_is_the_sum_over_its_parts():
    """1 300 samples of the 32 x 16 board exceed the 1 024 blocks of the data kernel (its blocks walk two samples) and give every
    pair of waves of the weight kernel a run of samples: the parameter gradients of the whole batch equal the sum of the
    gradients of its halves.  Both halves run the same kernel variant (bucket 36 has one per pass)."""
    from pmx import actor_tower
    H, W, B = 16, 32, 1300
    m = R.model(H, W, seed=11)
    obs = R.planes(B, H, W, seed=12).to(torch.uint8)
    g = torch.Generator(device="cuda").manual_seed(13)
    dfeat = (torch.randn(B, H * W, 32, device="cuda", generator=g) * 0.1).to(torch.bfloat16)
    params = actor_tower._tower_params(m.actor_backbone)

    def grads(lo, hi):
        feat = actor_tower.actor_tower(m.actor_backbone, obs[lo:hi])
        return torch.autograd.grad((feat.float() * dfeat[lo:hi].float()).sum(), params)
    whole, a, b = grads(0, B), grads(0, B // 2), grads(B // 2, B)
    for w, x, y in zip(whole, a, b):
        ref = x.double() + y.double()
        assert ((w.double() - ref).norm() / (ref.norm() + 1e-12)).item() < 2e-4        # float32 sums in another order


@pytest.mark.parametrize("board", [(16, 32), (20, 32), (3, 8), (13, 18)])
@pytest.mark.parametrize("B,dtype", [(3, torch.float32), (65, torch.uint8), (700, torch.uint8)])
def test_fused_projector_matches_torch(board, B, dtype):
    """tokens within one bf16 ulp (2^-7) of the largest, weight / bias gradients within 1e-2 of the float64 reference"""
    from pmx import mappo
    H, W = board
    torch.manual_seed(B)
    m = mappo.MAPPOAgent((8, H, W)).cuda()
    conv = m.critic_projector[0]
    with torch.no_grad():
        conv.bias.add_(0.2 * torch.randn(32, device="cuda"))
    obs = R.planes(B, H, W, seed=B + 1)
    assert m._fused_projector_ok(obs.to(dtype))
    pe = m._pe_table(H, W, obs.device)
    tok = mappo._Projector.apply(obs.to(dtype), conv.weight, conv.bias, pe)
    assert tok.shape == (B, H * W, 32) and tok.dtype == torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(B + 2)
    dt = torch.randn(B, H * W, 32, device="cuda", generator=g).to(torch.bfloat16)
    dw, db = torch.autograd.grad((tok.float() * dt.float()).sum(), [conv.weight, conv.bias])
    ref_r, dw_ref, db_ref = R.projector_reference(conv, pe, obs, dt)
    scale = float(ref_r.abs().max())
    assert float((tok.double() - ref_r).abs().max()) <= scale * 2 ** -7, float((tok.double() - ref_r).abs().max())
    assert float((dw.double() - dw_ref).abs().max()) <= 1e-2 * float(dw_ref.abs().max())
    assert float((db.double() - db_ref).abs().max()) <= 1e-2 * float(db_ref.abs().max())


def _maze_32x16(n):
    from pmx import maze_generator
    from pmx.layout import Layout
    return [Layout.from_text(maze_generator.generate_maze(3, rows=14, cols=15))] * n


@pytest.mark.parametrize("use_graph", [False, True])
def test_trainer_on_a_generated_32x16_maze_runs_the_fused_kernels(use_graph):
    """VecMAPPOTrainer on generate_maze(3, rows=14, cols=15) (BASELINE config 5's board): one full update, eager and replayed
    from a graph, with the fused tower and projector being what runs; then loss, pg, vl and the gradient norm of one fixed
    minibatch against the same minibatch on the library convolutions (fused_tower = fused_projector = False), within the
    relative bounds test_gpu_trainer.BF16_BOUNDS["sharp"] states for two bf16 paths of one model: scalars 3e-2, gradient norm
    8e-2."""
    from pmx import mappo, trainer
    tr = trainer.VecMAPPOTrainer(_maze_32x16(64), 64, horizon=4, minibatch=64, epochs=1, seed=5, length=30, opponent="random",
                                 use_graph=use_graph)
    assert tr.obs_shape == (8, 16, 32)
    model = tr.model
    o1 = tr.obs_buf[0, :1, 0]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert model._use_fused_tower(o1) and model._fused_projector_ok(tr.merged_buf[0, :1])
    st = tr.train_update()
    assert tr.use_graph == use_graph
    for k in ("pg", "vl", "entropy", "loss", "grad_norm"):
        assert torch.isfinite(st[k]).all(), k
    assert st["optimizer_steps"] == 4 * 64 * 2 // 64
    # one fixed minibatch: the first 32 env-ticks with both learners (the paired composition the trainer uses)
    S = 64
    obs = tr.obs_buf.view((-1,) + tr.obs_shape)[:S]
    merged = tr.merged_buf.view((-1,) + tr.obs_shape)[:S // 2]
    act, old_logp = tr.act_buf.view(-1)[:S], tr.logp_buf.view(-1)[:S]
    adv, ret = tr.adv_buf.view(-1)[:S], tr.ret_buf.view(-1)[:S]
    res = {}
    for fused in (True, False):
        model.fused_tower = model.fused_projector = fused
        learner = mappo.PPOLearner(model, autocast_dtype=torch.bfloat16)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert bool(model._use_fused_tower(obs)) == fused and bool(model._fused_projector_ok(merged)) == fused
            with learner._shadow_context():
                loss, stats = mappo.ppo_loss(model, obs, merged, act, old_logp, adv, ret, mappo.CLIP_EPS, mappo.ENT_COEF_START)
        learner._backward_into_bucket(loss)
        res[fused] = dict(loss=float(stats["loss"]), pg=float(stats["pg"]), vl=float(stats["vl"]),
                          grad_norm=float(learner.bucket.grad.double().norm()))
    model.fused_tower = model.fused_projector = True
    print("fused", res[True], "library", res[False])
    for k in ("loss", "pg", "vl"):
        assert abs(res[True][k] - res[False][k]) <= 3e-2 * abs(res[False][k]), (k, res[True][k], res[False][k])
    assert abs(res[True]["grad_norm"] - res[False]["grad_norm"]) <= 8e-2 * res[False]["grad_norm"], (res[True]["grad_norm"], res[False]["grad_norm"])
    tr.env.close()
