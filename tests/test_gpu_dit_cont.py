"""The DiT family under continuous diffusion on the GPU: Fourier front end, per-frame embedding, forward parity with the reference
fixture (tools/make_golden_dit_cont.py) and the restatements (tests/dit_cont_common.py), sampler, training, ABI refusals."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dit_cont_common as cc
from dit_cont_common import T, load, rel

pytestmark = pytest.mark.gpu


def _odit():
    from oracle import dit as odit
    return odit, odit.DiTConfig(**cc.SMALL), odit.DiffDiTConfig(**cc.DIFF_TINY)


def build_dit(**kw):
    import dfot_amd
    odit, small, _ = _odit()
    params = cc.with_buffers(odit.seeded_params(small, 2), 0)
    model = dfot_amd.DiT3D(cc.cont(cc.dit_cfg()), x_shape=(4, 16, 8), max_tokens=5, **kw).cuda().eval()
    assert list(model.state_dict()) == list(params)
    model.load_state_dict(params, strict=True)
    return model, params


def build_act(g):
    import dfot_amd
    from dit_cond_common import cond_weights
    odit, small, _ = _odit()
    base = cc.with_buffers(odit.seeded_params(small, 2), 0)
    params = {**base, **cond_weights(g, "act_cond")}
    model = dfot_amd.DiT3D(cc.cont(cc.dit_cfg(0.1)), x_shape=(4, 16, 8), max_tokens=5, external_cond_type="action", external_cond_dim=3).cuda().eval()
    assert list(model.state_dict()) == [str(n) for n in g["act_names"]]
    model.load_state_dict(params, strict=True)
    return model, params


def build_diff():
    import dfot_amd
    odit, _, oc = _odit()
    params = cc.with_buffers(odit.diff_seeded_params(oc, 3), 1)
    model = dfot_amd.DifferenceDiT3D(cc.cont(cc.diff_cfg()), x_shape=(4, 16, 8), max_tokens=5).cuda().eval()
    assert list(model.state_dict()) == list(params)
    model.load_state_dict(params, strict=True)
    return model, params


def test_fourier_front_end_against_float64_cosine():
    """tap "noise_feat" vs sqrt(2) cos in float64 of the reference-formed fp32 argument: only the fp32 cosine's own error remains, so
    1e-5 holds with identical arguments; a contracted multiply-add or a fast cosine shows >= 4e-6 * sqrt(2) at the extreme levels"""
    model, p = build_dit()
    lo, hi = cc.logsnr_extremes()
    lv = torch.tensor([[lo, hi, 0.0, 3.75, -3.75], [2.999, -1.0e-3, 1.0, hi, lo]])
    x = torch.zeros(2, 5, 4, 16, 8)
    with torch.no_grad():
        model(x.cuda(), lv.cuda())
    feat = model.read_tap("noise_feat", 10).cpu().double()
    ref = cc.fourier_features(lv, p[cc.FREQS], p[cc.PHASES], torch.float64).reshape(10, 256)
    err = float((feat - ref).abs().max())
    print(f"noise_feat max-abs error {err:.3e} (largest |argument| {float(cc.fourier_argument(lv, p[cc.FREQS], p[cc.PHASES]).abs().max()):.1f} rad)")
    assert err <= 1e-5


def test_cond_emb_unconditioned_action_and_difference():
    """tap "cond_emb" (e per frame) vs the float64 restatement at rel-L2 < 1e-5, the bar of the same tap in tests/test_gpu_dit_cond.py"""
    from dit_cond_common import action_embedding_fp64
    g = load("dit_cont.npz")
    x, lv = T(g["x"]).cuda(), T(g["levels"])
    model, p = build_dit()
    with torch.no_grad():
        model(x, lv.cuda())
    e = model.read_tap("cond_emb", 10).cpu()
    want = cc.fourier_embedding(p, lv, torch.float64).reshape(10, 128)
    print(f"cond_emb unconditioned rel-L2 {rel(e, want):.3e}")
    assert rel(e, want) < 1e-5
    am, ap = build_act(g)
    cond, mask = T(g["act_cond"]), T(g["act_mask"])
    with torch.no_grad():
        am(x, lv.cuda(), cond.cuda(), mask.cuda())
    e = am.read_tap("cond_emb", 10).cpu()
    ce = action_embedding_fp64(ap, cond, "external_cond_embedding.embedding") * (~mask)[:, None, None]
    want = (cc.fourier_embedding(ap, lv, torch.float64) + ce).reshape(10, 128)
    print(f"cond_emb action + mask rel-L2 {rel(e, want):.3e}")
    assert rel(e, want) < 1e-5
    dm, dp = build_diff()
    ld = T(g["levels_d"])
    with torch.no_grad():
        dm(T(g["xd"]).cuda(), ld.cuda())
    e = dm.read_tap("cond_emb", 20).cpu()
    kind = dp["diff_embedder.embedding_table.weight"].double()[[1, 0] * 5]  # even tokens are differences (row 1)
    want = (cc.fourier_embedding(dp, ld, torch.float64) + kind[None]).reshape(20, 128)
    print(f"cond_emb difference rel-L2 {rel(e, want):.3e}")
    assert rel(e, want) < 1e-5


def test_forwards_vs_reference_fixture_and_bit_identities():
    g = load("dit_cont.npz")
    x, lv = T(g["x"]).cuda(), T(g["levels"]).cuda()
    model, p = build_dit()
    assert cc.digest(p) == str(g["digest"])
    with torch.no_grad():
        out = model(x, lv)
        alone = model(x[1:].contiguous(), lv[1:].contiguous())
    print(f"DiT3D float levels rel-L2 vs the reference {rel(out.cpu(), T(g['out'])):.3e}")
    assert rel(out.cpu(), T(g["out"])) < 2e-2
    assert torch.equal(alone[0], out[1])  # a video alone and in a batch: same bits
    am, _ = build_act(g)
    cond, mask = T(g["act_cond"]).cuda(), T(g["act_mask"]).cuda()
    with torch.no_grad():
        ao = am(x, lv, cond, mask)
        an = am(x, lv, cond)
        au = am(x, lv)
        a1 = am(x[1:].contiguous(), lv[1:].contiguous(), cond[1:].contiguous(), mask[1:].contiguous())
    print(f"DiT3D action rel-L2 vs the reference {rel(ao.cpu(), T(g['act_out'])):.3e} / {rel(an.cpu(), T(g['act_out_nomask'])):.3e}")
    assert rel(ao.cpu(), T(g["act_out"])) < 2e-2 and rel(an.cpu(), T(g["act_out_nomask"])) < 2e-2
    assert torch.equal(ao[0], au[0]) and torch.equal(ao[1], an[1]) and not torch.equal(ao[1], au[1])  # masked video == unconditioned, bit for bit
    assert torch.equal(a1[0], ao[1])
    dm, dp = build_diff()
    assert cc.digest(dp) == str(g["digest_diff"])
    with torch.no_grad():
        do = dm(T(g["xd"]).cuda(), T(g["levels_d"]).cuda())
    print(f"DifferenceDiT3D float levels rel-L2 vs the reference {rel(do.cpu(), T(g['diff_out'])):.3e}")
    assert rel(do.cpu(), T(g["diff_out"])) < 2e-2


def test_variants_2_and_3_vs_restatement():
    import dfot_amd
    import dit_fac_common as fac
    import dit_facmat_common as fm
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(2, 5, 4, 16, 8, generator=gen)
    lo, hi = cc.logsnr_extremes()
    lv = 2.5 * torch.randn(2, 5, generator=gen)
    lv[0, 0], lv[1, 4] = lo, hi
    params = cc.seeded_params(fac.key_shapes(4.0), 2)
    m2 = dfot_amd.DiT3D(cc.cont(fac.backbone_cfg(4.0)), x_shape=(4, 16, 8), max_tokens=5).cuda().eval()
    m2.load_state_dict(params, strict=True)
    with torch.no_grad():
        o2 = m2(x.cuda(), lv.cuda()).cpu()
    r2 = rel(o2, cc.forward_fac(params, x, lv))
    cc_, rr, bias, ratio, rope = fm.CASES["b"]
    params = cc.seeded_params(fm.key_shapes(bias, ratio), 3)
    m3 = dfot_amd.DiT3D(cc.cont(fm.backbone_cfg(cc_, rr, bias, ratio, rope)), x_shape=(4, 16, 8), max_tokens=5).cuda().eval()
    m3.load_state_dict(params, strict=True)
    with torch.no_grad():
        o3 = m3(x.cuda(), lv.cuda()).cpu()
    r3 = rel(o3, cc.forward_facmat(params, x, lv, cc_, rr, rope))
    print(f"float levels, variant 2 rel-L2 {r2:.3e}, variant 3 rel-L2 {r3:.3e}")
    assert r2 < 2e-2 and r3 < 2e-2
    with pytest.raises(TypeError, match="floating noise levels"), torch.no_grad():
        m2(x.cuda(), torch.zeros(2, 5, dtype=torch.long).cuda())


def test_dmlab_minecraft_geometry():
    """x_shape (32, 8, 8), patch 2, 16 tokens, hidden 128: 16 patches per frame, 256 tokens per video"""
    import dfot_amd
    from oracle import dit as odit
    ocfg = odit.DiTConfig(hidden_size=128, depth=2, num_heads=4, patch_size=2, in_channels=32, resolution=(8, 8), max_tokens=16)
    params = cc.with_buffers(odit.seeded_params(ocfg, 4), 2)
    cfg = cc.cont(dict(name="dit3d", variant="full", pos_emb_type="rope_3d", patch_size=2, hidden_size=128, depth=2, num_heads=4))
    model = dfot_amd.DiT3D(cfg, x_shape=(32, 8, 8), max_tokens=16).cuda().eval()
    model.load_state_dict(params, strict=True)
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(2, 16, 32, 8, 8, generator=gen)
    lv = 2.5 * torch.randn(2, 16, generator=gen)
    with torch.no_grad():
        out = model(x.cuda(), lv.cuda()).cpu()
        ref = cc.forward_dit(params, ocfg, x, lv)
    print(f"dmlab / Minecraft geometry rel-L2 {rel(out, ref):.3e}")
    assert rel(out, ref) < 2e-2


class ReplayList:
    strict_order = True

    def __init__(self, draws):
        self.queue = list(draws)

    def __call__(self, tag, shape):
        t = self.queue.pop(0)
        assert tuple(t.shape) == tuple(shape), (tag, tuple(t.shape), tuple(shape))
        return (t if tag == "excluded" else t.clamp(-20, 20)).cuda()


def psnr(a, b):
    mse = ((a - b) ** 2).mean().item()
    peak = (b.max() - b.min()).item()
    return 10 * math.log10(peak * peak / max(mse, 1e-20))


def _sampler(model, steps, noise_fn=None):
    import dfot_amd
    cfg = dfot_amd.SamplerConfig(x_shape=(4, 16, 8), max_tokens=5, diffusion=dfot_amd.DiffusionConfig(sampling_timesteps=steps, is_continuous=True),
                                 prediction_guidance=dict(name="vanilla", guidance_scale=1.5))
    return dfot_amd.DFoTVideoSampler(cfg, model, noise_fn)


def test_sampler_trace_vs_reference_and_graph_equals_eager():
    g = load("dit_cont.npz")
    model, _ = build_dit()
    nfn = ReplayList([T(g[f"trace_noise{i}"]) for i in range(int(g["trace_n_noise"]))])
    vid = T(g["trace_vid"]).cuda()
    out = _sampler(model, 3, nfn)._predict_videos(vid, n_context_tokens=2, conditions=None).cpu()
    assert not nfn.queue
    ref = T(g["trace_pred"])
    print(f"continuous DiT sampler trace PSNR {psnr(out, ref):.1f} dB")
    assert torch.equal(out[:, :2], ref[:, :2]) and psnr(out, ref) >= 35.0

    def seeded(seed):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        return lambda tag, shape: torch.randn(shape, device="cuda", generator=gen).clamp_(-20, 20)
    graph = _sampler(model, 6, seeded(3))
    assert graph.use_graph
    og = graph._predict_videos(vid, n_context_tokens=2, conditions=None)
    assert graph.graph_captures == 1 and graph.graph_replays > 0
    eager = _sampler(model, 6, seeded(3))
    eager.use_graph = False
    oe = eager._predict_videos(vid, n_context_tokens=2, conditions=None)
    assert eager.graph_replays == 0 and torch.equal(og, oe)


def _trainer(tag, **kw):
    import dfot_amd
    odit, small, oc = _odit()
    if tag == "dit":
        params, cfg = cc.with_buffers(odit.seeded_params(small, 2), 0), cc.cont(cc.dit_cfg())
    else:
        params, cfg = cc.with_buffers(odit.diff_seeded_params(oc, 3), 1), cc.cont(cc.diff_cfg())
    tr = dfot_amd.DiT3DTrainer(cfg, x_shape=(4, 16, 8), max_tokens=5, diffusion=dfot_amd.DiffusionConfig(is_continuous=True), **kw)
    tr.load_state_dict(params, strict=True)
    assert list(tr.state_dict()) == list(params)
    return tr, params


@pytest.mark.parametrize("tag", ["dit", "diff"])
def test_training_step_vs_reference_fixture_and_autograd(tag):
    """ContinuousDiffusion.forward + _reweight_loss + backward of the reference (fixture) and fp32 autograd through the restatement"""
    odit, small, oc = _odit()
    g = load("dit_cont.npz")
    xs, t, masks, noise = T(g["train_xs"]), T(g["train_t"]), T(g["train_masks"]), T(g[f"train_{tag}_noise"])
    tr, params = _trainer(tag)
    loss = tr.loss_and_grads(xs, t, noise, masks) if tag == "dit" else tr.difference_loss_and_grads(xs, t, noise, masks)
    ref_loss = float(g[f"train_{tag}_loss"])
    print(f"{tag}: loss {float(loss):.6f} vs the reference {ref_loss:.6f}")
    assert abs(float(loss.item()) - ref_loss) < 2e-2 * abs(ref_loss)
    grads = {n: v.cpu() for n, v in tr.grad_dict().items()}
    names = [str(n) for n in g[f"train_{tag}_names"]]
    assert names == list(grads) and cc.FREQS not in grads and cc.PHASES not in grads
    for n, ref_norm in zip(names, g[f"train_{tag}_norms"]):
        assert abs(float(grads[n].norm()) - ref_norm) <= 3e-2 * ref_norm + 1e-7, (n, float(grads[n].norm()), ref_norm)
    worst = 0.0
    for key in g.files:
        if key.startswith(f"train_{tag}_grad/"):
            ref = T(g[key])
            if float(ref.norm()) > 1e-6:
                worst = max(worst, rel(grads[key.split("/", 1)[1]], ref))
    print(f"{tag}: worst stored-gradient rel-L2 vs the reference {worst:.2e}")
    assert worst < 5e-2
    # every parameter's gradient vs fp32 autograd through the restatement, for a plain upstream gradient
    gen = torch.Generator().manual_seed(5)
    tok = 5 if tag == "dit" else 10
    x = torch.randn(2, tok, 4, 16, 8, generator=gen)
    lv = 2.5 * torch.randn(2, tok, generator=gen)
    w = torch.randn(2, tok, 4, 16, 8, generator=gen)
    out = tr.forward(x, lv.cuda())
    tr.backward(w)
    ps = {n: (v.clone().requires_grad_() if n not in (cc.FREQS, cc.PHASES) else v) for n, v in params.items()}
    ref = cc.forward_dit(ps, small, x, lv) if tag == "dit" else cc.forward_diff(ps, oc, x, lv)
    (ref * w).sum().backward()
    assert rel(out.cpu(), ref.detach()) < 2e-2
    eg = tr.grad_dict()
    rs = {n: rel(eg[n].cpu(), v.grad) for n, v in ps.items() if v.requires_grad}
    bad = max(rs, key=rs.get)
    print(f"{tag}: worst gradient rel-L2 vs autograd {rs[bad]:.2e} at {bad}")
    assert rs[bad] < 5e-2


def test_training_step_matches_torch_adamw_and_buffers_stay():
    from dfot_amd.diffusion import DiffusionConfig
    odit, small, _ = _odit()
    tr, params = _trainer("dit", lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    gen = torch.Generator().manual_seed(4)
    xs = torch.randn(2, 5, 4, 16, 8, generator=gen)
    t = torch.rand(2, 5, generator=gen)
    noise = torch.randn(2, 5, 4, 16, 8, generator=gen)
    masks = torch.ones(2, 5)
    masks[1, 0] = 0
    loss = float(tr.training_step(xs, t, noise, masks).item())
    new = {n: v.cpu() for n, v in tr.state_dict().items()}
    # torch reference: ContinuousDiffusion.forward (continuous_diffusion.py:140-167) on the restatement
    ps = {n: (v.clone().requires_grad_() if n not in (cc.FREQS, cc.PHASES) else v) for n, v in params.items()}
    logsnr, alpha, sigma, weight = DiffusionConfig(is_continuous=True).training_logsnr_tables(t)
    e5 = lambda a: a[..., None, None, None]
    x_t = e5(alpha) * xs + e5(sigma) * noise
    v = cc.forward_dit(ps, small, x_t, cc.PRECOND * logsnr)
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
    for _ in range(2):
        tr.training_step(xs, t, noise, masks)
    sd = tr.state_dict()
    assert torch.equal(sd[cc.FREQS].cpu(), params[cc.FREQS]) and torch.equal(sd[cc.PHASES].cpu(), params[cc.PHASES])
    assert not torch.equal(sd[f"{cc.EMB}.linear_1.weight"].cpu(), new[f"{cc.EMB}.linear_1.weight"])
    osd = tr.optimizer_state_dict()
    assert len(osd["state"]) == len(tr.layout) == len(params) - 2  # no optimizer state for the buffers
    with pytest.raises(TypeError, match="floating noise levels"):
        tr.forward(xs, torch.zeros(2, 5, dtype=torch.long))


def test_fourier_module_trains_through_autograd():
    odit, small, _ = _odit()
    model, params = build_dit()
    model.train()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(2, 5, 4, 16, 8, generator=gen).cuda().requires_grad_()
    lv = (2.5 * torch.randn(2, 5, generator=gen)).cuda()
    w = torch.randn(2, 5, 4, 16, 8, generator=gen).cuda()
    v = model(x, lv)
    assert v.requires_grad
    (v * w).sum().backward()
    ps = {n: (t.clone().requires_grad_() if n not in (cc.FREQS, cc.PHASES) else t) for n, t in params.items()}
    xr = x.detach().cpu().requires_grad_()
    ref = cc.forward_dit(ps, small, xr, lv.cpu())
    (ref * w.cpu()).sum().backward()
    named = dict(model.named_parameters())
    assert cc.FREQS not in named and cc.FREQS in dict(model.named_buffers())
    rs = {n: rel(p.grad.cpu(), ps[n].grad) for n, p in named.items()}
    bad = max(rs, key=rs.get)
    print(f"Fourier DiT3D autograd: worst gradient rel-L2 {rs[bad]:.2e} at {bad}; d/dx rel-L2 {rel(x.grad.cpu(), xr.grad):.2e}")
    assert rs[bad] < 5e-2 and rel(x.grad.cpu(), xr.grad) < 5e-2
    with pytest.raises(TypeError, match="floating noise levels"):
        model(x, torch.zeros(2, 5, dtype=torch.long).cuda())


def test_abi_refusals():
    from dfot_amd import capi
    from dit_cond_common import build_plain
    fm, _ = build_dit()
    dm = build_plain()
    x = torch.zeros(1, 5, 4, 16, 8).cuda()
    out = torch.empty_like(x)
    ki, kf = torch.zeros(1, 5, dtype=torch.int32).cuda(), torch.zeros(1, 5).cuda()
    with torch.no_grad():
        fm(x, kf)
        dm(x, ki)
    s = capi.stream_ptr()
    null = C.c_void_p(0)
    rc = capi.lib.dfot_dit_forward(fm._handle, capi.ptr(x), capi.ptr(ki), capi.ptr(out), 1, 5, s)
    assert rc == capi.ERR_ARG and b"dfot_dit_forward_f" in capi.lib.dfot_last_error()
    rc = capi.lib.dfot_dit_forward_f(dm._handle, capi.ptr(x), capi.ptr(kf), null, null, null, capi.ptr(out), 1, 5, s)
    assert rc == capi.ERR_ARG and b"dfot_dit_forward / dfot_dit_forward_cond" in capi.lib.dfot_last_error()
    buf = torch.empty(1000, 128).cuda()
    rc = capi.lib.dfot_dit_read_tap(fm._handle, b"emb", capi.ptr(buf), buf.numel(), s)
    assert rc == capi.ERR_ARG and b"fourier_noise" in capi.lib.dfot_last_error()
    assert capi.lib.dfot_dit_read_tap(dm._handle, b"emb", capi.ptr(buf), buf.numel(), s) == capi.OK
    tr, _ = _trainer("dit")
    tr.forward(x, kf)
    rc = capi.lib.dfot_dit_train_forward(tr._handle, capi.ptr(x), capi.ptr(ki), capi.ptr(out), 1, 5, s)
    assert rc == capi.ERR_ARG and b"dfot_dit_train_forward_f" in capi.lib.dfot_last_error()
    torch.cuda.synchronize()
