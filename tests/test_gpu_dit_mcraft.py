"""The Minecraft / dmlab DiT recipe at its own shape on the GPU: latents (32, 8, 8), patch 2 -- a 128-wide patch vector, 16 patches per frame,
max_tokens 16 -- under continuous diffusion with actions of dim 4.  From hidden 384 on the final layer's weight leaves LDS (the chunked
kernel), and the trainer's final-layer backward runs 128 columns wide.  Fixture: tests/golden/dit_mcraft.npz (the reference's own modules,
tools/make_golden_dit_mcraft.py); restatement: tests/dit_mcraft_common.forward."""
import pytest
import torch

import dit_cont_common as cc
import dit_mcraft_common as mc
from dit_mcraft_common import T, load, rel

pytestmark = pytest.mark.gpu


def build(cfg, action):
    import dfot_amd
    model = dfot_amd.DiT3D(mc.backbone_cfg(cfg, mc.DROPOUT if action else 0.0), x_shape=mc.X_SHAPE, max_tokens=mc.MAX_TOKENS,
                           external_cond_type="action", external_cond_dim=mc.COND_DIM if action else 0).cuda().eval()
    params = mc.seeded_params(cfg, action, list(model.state_dict()))
    model.load_state_dict(params, strict=True)
    return model, params


def trainer(cfg, action=True, **kw):
    import dfot_amd
    tr = dfot_amd.DiT3DTrainer(mc.backbone_cfg(cfg, mc.DROPOUT if action else 0.0), x_shape=mc.X_SHAPE, max_tokens=mc.MAX_TOKENS,
                               diffusion=dfot_amd.DiffusionConfig(is_continuous=True), external_cond_type="action",
                               external_cond_dim=mc.COND_DIM if action else 0, **kw)
    params = mc.seeded_params(cfg, action, list(tr.state_dict()))
    tr.load_state_dict(params, strict=True)
    return tr, params


def dropout_generator(drop):
    """a CUDA generator whose first draw of len(drop) uniforms reproduces the per-video dropout mask (p = 0.1)"""
    for seed in range(4096):
        cand = torch.Generator(device="cuda").manual_seed(seed)
        if torch.equal((torch.rand(len(drop), device="cuda", generator=cand) < mc.DROPOUT).cpu(), drop):
            return torch.Generator(device="cuda").manual_seed(seed)
    raise AssertionError("no seed reproduces the mask")


def test_forward_vs_reference_fixture():
    g = load("dit_mcraft.npz")
    cfg = mc.ocfg()
    x, lv = T(g["x"]).cuda(), T(g["levels"]).cuda()
    model, p = build(cfg, False)
    assert cc.digest({n: p[n] for n in map(str, g["names"])}) == str(g["digest"])
    with torch.no_grad():
        out = model(x, lv)
    print(f"hidden 384, unconditioned: rel-L2 vs the reference {rel(out.cpu(), T(g['out'])):.3e}")
    assert rel(out.cpu(), T(g["out"])) < 2e-2
    am, ap = build(cfg, True)
    assert cc.digest({n: ap[n] for n in map(str, g["act_names"])}) == str(g["act_digest"])
    cond, mask = T(g["cond"]).cuda(), T(g["mask"]).cuda()
    with torch.no_grad():
        ao = am(x, lv, cond, mask)
        au = am(x, lv)
        an = am(x, lv, cond)
    print(f"hidden 384, actions + mask: rel-L2 vs the reference {rel(ao.cpu(), T(g['act_out'])):.3e}")
    assert rel(ao.cpu(), T(g["act_out"])) < 2e-2
    # a masked video reproduces the unconditioned bits; an unmasked one does not
    assert torch.equal(ao[0], au[0]) and torch.equal(ao[1], an[1]) and not torch.equal(ao[1], au[1])


def test_forward_at_dit_b_width():
    """hidden 768, 12 heads (depth 1): the recipe's own final layer, 128 x 768 fp32 = 384 KB in chunks of 53, 53 and 22 rows"""
    cfg = mc.ocfg(hidden_size=768, depth=1, num_heads=12)
    model, p = build(cfg, False)
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(1, 8, *mc.X_SHAPE, generator=gen)
    lv = 2.5 * torch.randn(1, 8, generator=gen)
    with torch.no_grad():
        out = model(x.cuda(), lv.cuda()).cpu()
        ref = cc.forward_dit(p, cfg, x, lv)
    print(f"hidden 768: rel-L2 vs the fp32 restatement {rel(out, ref):.3e}")
    assert rel(out, ref) < 2e-2


def test_sampler_graph_equals_eager_and_window_lengths():
    import dfot_amd
    model, _ = build(mc.ocfg(), True)

    def sampler(seed, max_tokens=mc.MAX_TOKENS):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        cfg = dfot_amd.SamplerConfig(x_shape=mc.X_SHAPE, max_tokens=max_tokens,
                                     diffusion=dfot_amd.DiffusionConfig(sampling_timesteps=3, is_continuous=True), external_cond_type="action",
                                     external_cond_dim=mc.COND_DIM, external_cond_processing="mask_first")
        return dfot_amd.DFoTVideoSampler(cfg, model, lambda tag, shape: torch.randn(shape, device="cuda", generator=gen).clamp_(-20, 20))
    g = torch.Generator().manual_seed(3)
    vid = torch.randn(1, 16, *mc.X_SHAPE, generator=g).cuda()
    acts = torch.randn(1, 16, mc.COND_DIM, generator=g).cuda()
    graph = sampler(5)
    assert graph.use_graph
    og = graph._predict_videos(vid, n_context_tokens=4, conditions=acts)
    assert graph.graph_captures == 1 and graph.graph_replays > 0
    eager = sampler(5)
    eager.use_graph = False
    oe = eager._predict_videos(vid, n_context_tokens=4, conditions=acts)
    assert eager.graph_replays == 0 and torch.equal(og, oe)
    assert torch.equal(og[:, :4], vid[:, :4]) and bool(torch.isfinite(og).all())
    # every window runs at max_tokens: 8 and 16 give tokens x patches in multiples of 128, anything else is refused when the sampler is built
    sampler(0, 8)
    with pytest.raises(ValueError, match="max_tokens 12 with 16 patches per frame"):
        sampler(0, 12)


def test_training_step_vs_reference_fixture_and_autograd():
    """ContinuousDiffusion.forward + _reweight_loss + backward of the reference (fixture), then fp32 autograd through the restatement; the
    bars of tests/test_gpu_dit_cont.py::test_training_step_vs_reference_fixture_and_autograd"""
    g = load("dit_mcraft.npz")
    cfg = mc.ocfg()
    tr, params = trainer(cfg)
    xs, t, masks, noise, drop = T(g["x"]), T(g["train_t"]), T(g["train_masks"]), T(g["train_noise"]), T(g["train_dropmask"])
    acts = T(g["cond"]).clone()
    acts[:, 0] = 0  # mask_first, as the reference's training_step processes them
    gen = dropout_generator(drop)
    loss = tr.loss_and_grads(xs, t, noise, masks, conditions=acts, dropout_generator=gen)
    assert torch.equal(tr.last_cond_dropout.cpu().bool(), drop)
    ref_loss = float(g["train_loss"])
    print(f"loss {float(loss):.6f} vs the reference {ref_loss:.6f}")
    assert abs(float(loss.item()) - ref_loss) < 2e-2 * abs(ref_loss)
    grads = {n: v.cpu() for n, v in tr.grad_dict().items()}
    names = [str(n) for n in g["train_names"]]
    assert sorted(names) == sorted(grads) and cc.FREQS not in grads and cc.PHASES not in grads
    for n, ref_norm in zip(names, g["train_norms"]):
        assert abs(float(grads[n].norm()) - ref_norm) <= 3e-2 * ref_norm + 1e-7, (n, float(grads[n].norm()), ref_norm)
    stored = [k for k in g.files if k.startswith("train_grad/")]
    assert len(stored) == 4
    for key in stored:
        r = rel(grads[key.split("/", 1)[1]], T(g[key]))
        print(f"  {key.split('/', 1)[1]}: rel-L2 vs the reference {r:.2e}")
        assert r < 5e-2, key
    # two runs of one step: the same bits
    first = tr.grads.clone()
    gen.manual_seed(gen.initial_seed())
    tr.loss_and_grads(xs, t, noise, masks, conditions=acts, dropout_generator=gen)
    assert torch.equal(tr.grads, first)
    # every parameter's gradient vs fp32 autograd through the restatement, for a plain upstream gradient
    rg = torch.Generator().manual_seed(5)
    x = torch.randn(2, 8, *mc.X_SHAPE, generator=rg)
    lv = 2.5 * torch.randn(2, 8, generator=rg)
    w = torch.randn(2, 8, *mc.X_SHAPE, generator=rg)
    cond = torch.randn(2, 8, mc.COND_DIM, generator=rg)
    mask = torch.tensor([False, True])
    out = tr.forward(x, lv.cuda(), cond, mask)
    tr.backward(w)
    ps = {n: (v.clone().requires_grad_() if n not in (cc.FREQS, cc.PHASES) else v) for n, v in params.items()}
    ref = mc.forward(ps, cfg, x, lv, cond, mask)
    (ref * w).sum().backward()
    assert rel(out.cpu(), ref.detach()) < 2e-2
    eg = tr.grad_dict()
    rs = {n: rel(eg[n].cpu(), v.grad) for n, v in ps.items() if v.requires_grad}
    bad = max(rs, key=rs.get)
    print(f"worst gradient rel-L2 vs autograd {rs[bad]:.2e} at {bad}; final linear {rs['dit_base.final_layer.linear.weight']:.2e}, "
          f"patch embedding {rs['patch_embedder.proj.weight']:.2e}")
    assert rs[bad] < 5e-2


def test_training_step_matches_torch_adamw():
    from dfot_amd.diffusion import DiffusionConfig
    cfg = mc.ocfg()
    tr, params = trainer(cfg, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    gen = torch.Generator().manual_seed(4)
    xs = torch.randn(2, 8, *mc.X_SHAPE, generator=gen)
    t = torch.rand(2, 8, generator=gen)
    noise = torch.randn(2, 8, *mc.X_SHAPE, generator=gen)
    acts = torch.randn(2, 8, mc.COND_DIM, generator=gen)
    acts[:, 0] = 0
    masks = torch.ones(2, 8)
    masks[1, 0] = 0
    loss = float(tr.training_step(xs, t, noise, masks, conditions=acts, dropout_generator=torch.Generator(device="cuda").manual_seed(0)).item())
    drop = tr.last_cond_dropout.cpu().bool()
    new = {n: v.cpu() for n, v in tr.state_dict().items()}
    # torch reference: ContinuousDiffusion.forward (continuous_diffusion.py:140-167) on the restatement
    ps = {n: (v.clone().requires_grad_() if n not in (cc.FREQS, cc.PHASES) else v) for n, v in params.items()}
    logsnr, alpha, sigma, weight = DiffusionConfig(is_continuous=True).training_logsnr_tables(t)
    e5 = lambda a: a[..., None, None, None]
    x_t = e5(alpha) * xs + e5(sigma) * noise
    v = mc.forward(ps, cfg, x_t, cc.PRECOND * logsnr, acts, drop)
    per = ((e5(alpha) * v + e5(sigma) * x_t - noise) ** 2) * e5(weight)
    ref_loss = (per * e5(masks)).mean()
    ref_loss.backward()
    plist = [v_ for v_ in ps.values() if v_.requires_grad]
    torch.nn.utils.clip_grad_norm_(plist, 1.0)
    torch.optim.AdamW(plist, lr=1e-3, weight_decay=0.01, betas=(0.9, 0.99), eps=1e-8).step()
    assert abs(loss - ref_loss.item()) < 2e-2 * abs(ref_loss.item()), (loss, ref_loss.item())
    checked = 0
    for n, tt in ps.items():
        if not tt.requires_grad:
            continue
        upd, ref_upd = new[n] - params[n], tt.detach() - params[n]
        big = tt.grad.abs() > 1e-2 * tt.grad.abs().max()
        if big.any():
            r = rel(upd[big], ref_upd[big])
            assert r < 5e-2, (n, r)
            checked += int(big.sum())
    assert checked > 1000


def test_module_under_autograd_gives_input_gradient():
    """DiT3D.forward under autograd (what reconstruction guidance differentiates): d/dx and every parameter vs autograd through the restatement"""
    cfg = mc.ocfg()
    model, params = build(cfg, False)
    model.train()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(2, 8, *mc.X_SHAPE, generator=gen).cuda().requires_grad_()
    lv = (2.5 * torch.randn(2, 8, generator=gen)).cuda()
    w = torch.randn(2, 8, *mc.X_SHAPE, generator=gen).cuda()
    v = model(x, lv)
    assert v.requires_grad
    (v * w).sum().backward()
    ps = {n: (t.clone().requires_grad_() if n not in (cc.FREQS, cc.PHASES) else t) for n, t in params.items()}
    xr = x.detach().cpu().requires_grad_()
    ref = cc.forward_dit(ps, cfg, xr, lv.cpu())
    (ref * w.cpu()).sum().backward()
    rs = {n: rel(p.grad.cpu(), ps[n].grad) for n, p in model.named_parameters()}
    bad = max(rs, key=rs.get)
    print(f"autograd: worst gradient rel-L2 {rs[bad]:.2e} at {bad}; d/dx rel-L2 {rel(x.grad.cpu(), xr.grad):.2e}")
    assert rs[bad] < 5e-2 and rel(x.grad.cpu(), xr.grad) < 5e-2


def test_train_create_names_a_patch_vector_past_256():
    import dfot_amd
    from dfot_amd import capi
    cfg = cc.cont(dict(name="dit3d", variant="full", pos_emb_type="rope_3d", patch_size=4, hidden_size=128, depth=1, num_heads=4))
    with pytest.raises((capi.DfotError, ValueError), match="patch vector too long"):
        dfot_amd.DiT3DTrainer(cfg, x_shape=(32, 16, 32), max_tokens=4, diffusion=dfot_amd.DiffusionConfig(is_continuous=True))


def test_small_shape_gradients_still_match_the_stored_ones():
    """guard: at x_shape (4, 16, 8), patch 1 (a 4-wide patch vector, the 64-column backward of before) the trainer's gradients meet the
    reference's stored ones of tests/golden/dit_cont.npz as tests/test_gpu_dit_cont.py finds them"""
    import dfot_amd
    from oracle import dit as odit
    g = load("dit_cont.npz")
    params = cc.with_buffers(odit.seeded_params(odit.DiTConfig(**cc.SMALL), 2), 0)
    tr = dfot_amd.DiT3DTrainer(cc.cont(cc.dit_cfg()), x_shape=(4, 16, 8), max_tokens=5, diffusion=dfot_amd.DiffusionConfig(is_continuous=True))
    tr.load_state_dict(params, strict=True)
    loss = tr.loss_and_grads(T(g["train_xs"]), T(g["train_t"]), T(g["train_dit_noise"]), T(g["train_masks"]))
    ref_loss = float(g["train_dit_loss"])
    assert abs(float(loss.item()) - ref_loss) < 2e-2 * abs(ref_loss)
    grads = {n: v.cpu() for n, v in tr.grad_dict().items()}
    names = [str(n) for n in g["train_dit_names"]]
    assert names == list(grads)
    for n, ref_norm in zip(names, g["train_dit_norms"]):
        assert abs(float(grads[n].norm()) - ref_norm) <= 3e-2 * ref_norm + 1e-7, (n, float(grads[n].norm()), ref_norm)
    worst = 0.0
    for key in g.files:
        if key.startswith("train_dit_grad/"):
            ref = T(g[key])
            if float(ref.norm()) > 1e-6:
                worst = max(worst, rel(grads[key.split("/", 1)[1]], ref))
    print(f"small shape: worst stored-gradient rel-L2 vs the reference {worst:.2e}")
    assert worst < 5e-2
