"""GPU checks of the action / label conditioned DiT family against the fixtures made from the reference's own modules
(tests/golden/dit_cond.npz, dit_cond_run.npz; tools/make_golden_dit_cond.py).

Bars: forward vs the fixtures rel-L2 < 2e-2 and sampler PSNR >= 35 dB (the bars of tests/test_gpu_dit.py for the unconditioned fixtures
of the same size: bf16 MFMA operands, fp32 accumulation); the condition-embedding kernel alone vs float64 rel-L2 < 1e-5 (fp32 arithmetic,
as the noise-level embedding check); training loss 2e-2 and gradients 5e-2 relative (the bars of the unconditioned training tests);
everything stated as "the same" is compared bit for bit."""
import math

import numpy as np
import pytest
import torch

from dit_cond_common import (MODES, T, action_embedding_fp64, base_params, build_diff, build_mode, build_plain, cond_weights, diff_cfg, dit_cfg,
                             load, rel)

pytestmark = pytest.mark.gpu


def psnr(a, b):
    mse = ((a - b) ** 2).mean().item()
    peak = (b.max() - b.min()).item()
    return 10 * math.log10(peak * peak / max(mse, 1e-20))


class ReplayList:
    strict_order = True

    def __init__(self, draws):
        self.queue = list(draws)

    def __call__(self, tag, shape):
        t = self.queue.pop(0)
        assert tuple(t.shape) == tuple(shape), (tag, tuple(t.shape), tuple(shape))
        return (t if tag == "excluded" else t.clamp(-20, 20)).cuda()


def test_conditioned_forward_exists():
    """fails before this feature: the constructor raised ValueError for any external_cond_dim != 0"""
    import dfot_amd
    model = dfot_amd.DiT3D(dit_cfg(), x_shape=(4, 16, 8), max_tokens=5, external_cond_type="action", external_cond_dim=3).cuda()
    model.init_random(0)
    x, k = torch.randn(2, 5, 4, 16, 8, device="cuda"), torch.randint(0, 1000, (2, 5), device="cuda")
    with torch.no_grad():
        out = model(x, k, torch.randn(2, 5, 3, device="cuda"))
    assert out.shape == x.shape and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("mode", list(MODES))
def test_parameter_names_and_order_equal_the_reference(mode):
    g = load("dit_cond.npz")
    model, _ = build_mode(mode, g)
    assert list(model.state_dict().keys()) == [str(n) for n in g[f"{mode}_names"]]
    from dfot_amd import trainer
    ctype, cdim, ncls, drop = MODES[mode]
    tr = trainer.DiT3DTrainer(dit_cfg(drop), (4, 16, 8), 5, external_cond_type=ctype, external_cond_num_classes=ncls, external_cond_dim=cdim)
    assert list(tr.layout) == [str(n) for n in g[f"{mode}_names"]]


def test_parameter_names_without_a_condition_are_unchanged():
    from oracle import dit as odit
    from dit_cond_common import SMALL
    assert list(build_plain().state_dict().keys()) == list(odit.param_shapes(odit.DiTConfig(**SMALL)))
    g = load("dit_cond.npz")
    model, _ = build_diff(g)
    assert list(model.state_dict().keys()) == [str(n) for n in g["diff_act_names"]]


@pytest.mark.parametrize("mode", list(MODES))
def test_forward_vs_reference_fixture(mode):
    g = load("dit_cond.npz")
    model, _ = build_mode(mode, g)
    x, k, cond, mask = T(g["x"]).cuda(), T(g["k"]).cuda(), T(g[f"{mode}_cond"]).cuda(), T(g["mask"]).cuda()
    with torch.no_grad():
        out = model(x, k, cond)
        out_m = model(x, k, cond, mask)
        out_n = model(x, k)
    r = rel(out.cpu(), T(g[f"{mode}_out"]))
    print(f"{mode}: rel-L2 vs the reference {r:.3e}")
    assert r < 2e-2
    if bool(g[f"{mode}_mask_ignored"]):  # the reference's module never sees the mask in this mode
        assert torch.equal(out_m, out)
    else:
        rm = rel(out_m.cpu(), T(g[f"{mode}_out_masked"]))
        rn = rel(out_n.cpu(), T(g[f"{mode}_out_none"]))
        print(f"{mode}: masked {rm:.3e}, no condition {rn:.3e}")
        assert rm < 2e-2 and rn < 2e-2


def test_difference_model_forward_vs_reference_fixture():
    g = load("dit_cond.npz")
    model, _ = build_diff(g)
    x, k, cond, mask = T(g["xd"]).cuda(), T(g["kd"]).cuda(), T(g["diff_act_cond"]).cuda(), T(g["mask"]).cuda()
    with torch.no_grad():
        out, out_m, out_n = model(x, k, cond), model(x, k, cond, mask), model(x, k)
    r, rm = rel(out.cpu(), T(g["diff_act_out"])), rel(out_m.cpu(), T(g["diff_act_out_masked"]))
    print(f"difference model: rel-L2 {r:.3e}, masked {rm:.3e}")
    assert r < 2e-2 and rm < 2e-2
    assert torch.equal(out_m[0], out_n[0]) and torch.equal(out_m[1], out[1])


@pytest.mark.parametrize("mode", ["act_d1", "label", "diff_act"])
def test_condition_embedding_kernel_vs_float64(mode):
    """e = noise-level embedding (+ token kind) + condition embedding of every frame (tap "cond_emb") against the engine's own
    noise-level table (checked on its own in test_gpu_dit.py) plus the condition embedding restated in float64"""
    g = load("dit_cond.npz")
    if mode == "diff_act":
        model, params = build_diff(g)
        x, k, cond = T(g["xd"]).cuda(), T(g["kd"]).cuda(), T(g["diff_act_cond"])
    else:
        model, params = build_mode(mode, g)
        x, k, cond = T(g["x"]).cuda(), T(g["k"]).cuda(), T(g[f"{mode}_cond"])
    b, t = k.shape
    with torch.no_grad():
        model(x, k, cond.cuda(), T(g["mask"]).cuda() if mode != "label" else None)
    e = model.read_tap("cond_emb", b * t).cpu().view(b, t, 128)
    emb = model.read_tap("emb", 1000).cpu().double()[k.cpu()]
    if mode == "label":
        ce = params["external_cond_embedding.embedding_table.weight"].double()[cond.long()].expand(b, t, 128)
    else:
        ce = action_embedding_fp64(params, cond, "external_cond_embedding.embedding").clone()
        ce[0] = 0  # mask = [True, False]
    if mode == "diff_act":
        kind = torch.tensor([1, 0] * (t // 2))
        emb = emb + params["diff_embedder.embedding_table.weight"].double()[kind]
    r = rel(e, emb + ce)
    rc = rel(e.double() - emb, ce)
    print(f"{mode}: e rel-L2 {r:.3e}; condition part alone {rc:.3e}")
    assert r < 1e-5 and rc < 1e-5


def test_masked_video_is_bit_identical_to_the_model_without_a_condition():
    g = load("dit_cond.npz")
    model, _ = build_mode("act_d1", g)
    plain = build_plain()
    x, k, cond = T(g["x"]).cuda(), T(g["k"]).cuda(), T(g["act_d1_cond"]).cuda()
    tt, ff = torch.tensor([True, False]).cuda(), torch.tensor([False, False]).cuda()
    with torch.no_grad():
        ref = plain(x, k)
        none = model(x, k)
        m_tf, m_ff, m_tt, m_ft = model(x, k, cond, tt), model(x, k, cond, ff), model(x, k, cond, ~ff), model(x, k, cond, ~tt)
        free = model(x, k, cond)
    assert torch.equal(none, ref)                                     # no condition given: the per-level table of the same weights
    assert torch.equal(m_tt, ref)                                     # every video masked: the per-frame table reproduces it bit for bit
    assert torch.equal(m_tf[0], ref[0]) and torch.equal(m_ft[1], ref[1])
    assert torch.equal(m_ff, free)
    # videos of one batch do not influence each other: video 1 with its condition is the same whatever video 0 does, and vice versa
    assert torch.equal(m_tf[1], free[1]) and torch.equal(m_ft[0], free[0])
    assert not torch.equal(free[0], ref[0])


@pytest.mark.parametrize("mode", list(MODES))
def test_the_condition_matters(mode):
    g = load("dit_cond.npz")
    model, _ = build_mode(mode, g)
    x, k, cond = T(g["x"]).cuda(), T(g["k"]).cuda(), T(g[f"{mode}_cond"]).cuda()
    other = (cond + 17) % 101 if mode == "label" else -cond
    with torch.no_grad():
        a, b = model(x, k, cond).cpu(), model(x, k, other).cpu()
    parity = rel(a, T(g[f"{mode}_out"]))
    moved = rel(b, a)
    print(f"{mode}: another condition moves the output by {moved:.3e}; parity error {parity:.3e}")
    assert moved > 5 * parity


def _sampler(model, noise_fn=None, steps=4, cls=None, max_tokens=5, processing="mask_first", scale=1.5):
    import dfot_amd
    cfg = dfot_amd.SamplerConfig(x_shape=(4, 16, 8), max_tokens=max_tokens,
                                 diffusion=dfot_amd.DiffusionConfig(sampling_timesteps=steps, beta_schedule="cosine", is_continuous=False),
                                 prediction_guidance=dict(name="vanilla", guidance_scale=scale), external_cond_type="action", external_cond_dim=3,
                                 external_cond_processing=processing)
    return (cls or dfot_amd.DFoTVideoSampler)(cfg, model, noise_fn)


def test_conditioned_sampler_vs_reference_fixture():
    g = load("dit_cond_run.npz")
    gm = load("dit_cond.npz")
    model, params = build_mode("act_d1", gm)
    for n, t in cond_weights(g, "cond").items():  # the run used the same condition tensors as the forward fixture's act_d1 mode
        assert torch.equal(t, params[n])
    assert list(model.state_dict().keys()) == [str(n) for n in g["names"]]
    nfn = ReplayList([T(g[f"noise{i}"]) for i in range(int(g["n_noise"]))])
    out = _sampler(model, nfn, steps=3)._predict_videos(T(g["vid"]).cuda(), n_context_tokens=2, conditions=T(g["actions"])).cpu()
    assert not nfn.queue
    p = psnr(out, T(g["pred"]))
    print(f"conditioned sampler: PSNR vs the reference's run {p:.1f} dB")
    assert p >= 35.0


def _seeded_noise(seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return lambda tag, shape: torch.randn(shape, device="cuda", generator=gen).clamp_(-20, 20)


def test_graph_step_loop_equals_eager_and_follows_the_conditions():
    g = load("dit_cond_run.npz")
    model, _ = build_mode("act_d1")
    vid, a1 = T(g["vid"]).cuda(), T(g["actions"])
    a2 = a1.flip(0) * 1.5
    graph = _sampler(model, steps=6)
    assert graph.use_graph

    def run(s, acts, seed=3):
        s.noise_fn = _seeded_noise(seed)
        return s._predict_videos(vid, n_context_tokens=2, conditions=acts)
    out1 = run(graph, a1)
    assert graph.graph_captures == 1 and graph.graph_replays > 0
    out2 = run(graph, a2)  # same shapes: the captured graph is replayed with the new conditions
    assert graph.graph_captures == 1
    eager = _sampler(model, steps=6)
    eager.use_graph = False
    e1, e2 = run(eager, a1), run(eager, a2)
    assert eager.graph_replays == 0
    assert torch.equal(out1, e1) and torch.equal(out2, e2)
    assert not torch.equal(out1, out2)
    assert torch.equal(run(graph, a1), e1)


def test_difference_sampler_with_merged_conditions():
    import dfot_amd
    gm = load("dit_cond.npz")
    model, _ = build_diff(gm)
    g = load("dit_cond_run.npz")
    vid, acts = T(g["vid"]).cuda(), T(g["actions"])
    s = _sampler(model, steps=5, cls=dfot_amd.DifferenceDFoTVideoSampler, max_tokens=10)
    s.noise_fn = _seeded_noise(5)
    out = s._sample_all_videos(vid, 2, acts)
    assert s.graph_replays > 0
    e = _sampler(model, steps=5, cls=dfot_amd.DifferenceDFoTVideoSampler, max_tokens=10)
    e.use_graph, e.noise_fn = False, _seeded_noise(5)
    ref = e._sample_all_videos(vid, 2, acts)
    assert torch.equal(out["prediction"], ref["prediction"]) and torch.equal(out["prediction_diff"], ref["prediction_diff"])
    assert torch.equal(out["prediction"][:, :2], vid[:, :2]) and bool(torch.isfinite(out["prediction"]).all())
    s.noise_fn = _seeded_noise(5)
    assert not torch.equal(s._sample_all_videos(vid, 2, -acts)["prediction"], out["prediction"])
    # the model itself on merged conditions: what one window hands it
    merged = s.merge_tensors(acts, acts).cuda()
    x, k = T(gm["xd"]).cuda(), T(gm["kd"]).cuda()
    with torch.no_grad():
        assert bool(torch.isfinite(model(x, k, merged)).all())
    with pytest.raises(ValueError, match="for noncausal models, conditions length is expected to be 10, got 5."):
        s._sample_sequence(2, conditions=acts)


def _trainer(dropout=0.1, ctype="action", ncls=None, cdim=3):
    from dfot_amd import trainer
    return trainer.DiT3DTrainer(dit_cfg(dropout), (4, 16, 8), 5, external_cond_type=ctype, external_cond_num_classes=ncls, external_cond_dim=cdim,
                                loss_weighting=dict(strategy="fused_min_snr", snr_clip=5.0, cum_snr_decay=0.96))


@pytest.mark.parametrize("tag", ["keep", "drop"])
def test_training_step_vs_reference_fixture(tag):
    g, gm = load("dit_cond_run.npz"), load("dit_cond.npz")
    params = {**base_params(), **cond_weights(gm, "act_d1_cond")}
    tr = _trainer()
    tr.load_state_dict(params, strict=True)
    drop = T(g[f"train_{tag}_dropmask"])
    # a CUDA generator whose first draw of 2 uniforms reproduces the stored mask (p = 0.1)
    gen = None
    for seed in range(4096):
        cand = torch.Generator(device="cuda").manual_seed(seed)
        if torch.equal((torch.rand(2, device="cuda", generator=cand) < 0.1).cpu(), drop):
            gen = torch.Generator(device="cuda").manual_seed(seed)
            break
    assert gen is not None
    acts = T(g["actions"]).clone()
    acts[:, 0] = 0  # mask_first, as the reference's training_step processes them
    loss = tr.loss_and_grads(T(g["train_xs"]), T(g["train_k"]), T(g[f"train_{tag}_noise"]), T(g["train_masks"]), conditions=acts,
                             dropout_generator=gen)
    assert torch.equal(tr.last_cond_dropout.cpu().bool(), drop)
    ref_loss = float(g[f"train_{tag}_loss"])
    print(f"{tag}: loss {loss.item():.6f} vs {ref_loss:.6f}")
    assert abs(loss.item() - ref_loss) < 2e-2 * abs(ref_loss)
    grads = tr.grad_dict()
    names = [str(n) for n in g[f"train_{tag}_grad_names"]]
    assert names == list(grads)
    worst = 0.0
    for n, ref_norm in zip(names, g[f"train_{tag}_norms"]):
        err = abs(float(grads[n].norm()) - ref_norm) / max(ref_norm, 1e-30)
        worst = max(worst, err)
        assert err < 5e-2, (n, float(grads[n].norm()), ref_norm)
    for key in g.files:
        if key.startswith(f"train_{tag}_grad/"):
            n = key.split("/", 1)[1]
            r = rel(grads[n].cpu(), T(g[key]))
            print(f"  {n}: rel-L2 {r:.3e}")
            assert r < 5e-2, n
    print(f"{tag}: worst gradient-norm error {worst:.3e}")
    # two runs give the same bits
    first = tr.grads.clone()
    gen.manual_seed(gen.initial_seed())
    tr.loss_and_grads(T(g["train_xs"]), T(g["train_k"]), T(g[f"train_{tag}_noise"]), T(g["train_masks"]), conditions=acts, dropout_generator=gen)
    assert torch.equal(tr.grads, first)


def test_label_training_gradients_are_reproducible_and_zero_for_unused_classes():
    gm = load("dit_cond.npz")
    tr = _trainer(0.0, "label", 101, 1)
    tr.load_state_dict({**base_params(), **cond_weights(gm, "label_cond")}, strict=True)
    gen = torch.Generator().manual_seed(0)
    xs, noise = torch.randn(2, 5, 4, 16, 8, generator=gen), torch.randn(2, 5, 4, 16, 8, generator=gen)
    k = torch.randint(0, 1000, (2, 5), generator=gen)
    labels = torch.tensor([[7], [42]])
    tr.loss_and_grads(xs, k, noise, conditions=labels)
    first = tr.grads.clone()
    table = tr.grad_dict()["external_cond_embedding.embedding_table.weight"]
    used = torch.zeros(101, dtype=torch.bool)
    used[[7, 42]] = True
    assert bool((table[~used] == 0).all()) and bool((table[used].abs().sum(1) > 0).all())
    tr.loss_and_grads(xs, k, noise, conditions=labels)
    assert torch.equal(tr.grads, first)
    # the table rows against autograd through a float64 restatement of "emb + table[label]": d loss / d row = sum over the video's
    # frames of d loss / d emb, which the noise-level embedding's last bias also receives over ALL frames
    bias = tr.grad_dict()["noise_level_pos_embedding.embedding.linear_2.bias"]
    assert rel(table[used].sum(0).cpu(), bias.cpu()) < 1e-4


def test_autograd_through_the_module_agrees_with_the_trainer():
    g, gm = load("dit_cond_run.npz"), load("dit_cond.npz")
    model, params = build_mode("act_d1", gm)
    model.eval()  # no dropout draw: the condition of every video is used
    tr = _trainer()
    tr.load_state_dict(params, strict=True)
    x, k, acts = T(g["train_xs"]).cuda(), T(g["train_k"]).cuda(), T(g["actions"]).cuda()
    d_out = torch.randn(2, 5, 4, 16, 8, generator=torch.Generator().manual_seed(1)).cuda()
    out = model(x, k, acts)
    assert out.requires_grad
    (out * d_out).sum().backward()
    ref = tr.forward(x, k, acts)
    tr.backward(d_out)
    assert torch.equal(out.detach(), ref)
    for n, p in model.named_parameters():
        assert torch.equal(p.grad, tr.view(n, tr.grads)), n
    assert float(model.state_dict()["external_cond_embedding.embedding.linear_1.weight"].abs().sum()) > 0
    assert float(dict(model.named_parameters())["external_cond_embedding.embedding.linear_1.weight"].grad.abs().sum()) > 0
    # train(): a per-video dropout draw from the module's generator; a mask is refused as the reference asserts
    model.train()
    model._dropout_generator = torch.Generator(device="cuda").manual_seed(0)
    with pytest.raises(AssertionError, match="embedding mask is only allowed during inference"):
        model(x, k, acts, torch.tensor([True, False]).cuda())


def test_argument_errors():
    import dfot_amd
    model, _ = build_mode("act_d1")
    plain = build_plain()
    x, k = torch.randn(2, 5, 4, 16, 8, device="cuda"), torch.randint(0, 1000, (2, 5), device="cuda")
    with pytest.raises(ValueError, match="built without an external condition embedding"):
        plain(x, k, torch.randn(2, 5, 3, device="cuda"))
    with pytest.raises(ValueError, match="expected"):
        model(x, k, torch.randn(2, 4, 3, device="cuda"))
    with pytest.raises(ValueError, match="external_cond_mask"):
        model(x, k, torch.randn(2, 5, 3, device="cuda"), torch.tensor([True, False, True]).cuda())
    with pytest.raises(ValueError):
        model(x, k, torch.randn(2, 5, 3))  # host tensor
    from dfot_amd import capi
    with pytest.raises(capi.DfotError):
        capi.check(capi.lib.dfot_dit_forward_cond(plain._handle, capi.ptr(x), capi.ptr(k.int()), capi.ptr(x), None, None, capi.ptr(x), 2, 5, capi.stream_ptr()))


def test_difference_training_with_conditions_is_reproducible():
    """DifferenceDFoTVideo.training_step with actions: conditions merged with themselves, every gradient finite, the condition embedding
    receives one, and two runs give the same bits (the modulation / bias / matrix-attention partial sums are added in a fixed order)"""
    from dfot_amd import trainer
    gm = load("dit_cond.npz")
    _, params = build_diff(gm)
    tr = trainer.DiT3DTrainer(diff_cfg(0.1), (4, 16, 8), 5, external_cond_type="action", external_cond_dim=3)
    assert list(tr.layout) == [str(n) for n in gm["diff_act_names"]]
    tr.load_state_dict(params, strict=True)
    gen = torch.Generator().manual_seed(2)
    frames, noise = torch.randn(2, 5, 4, 16, 8, generator=gen), torch.randn(2, 10, 4, 16, 8, generator=gen)
    k, acts = torch.randint(0, 1000, (2, 5), generator=gen), torch.randn(2, 5, 3, generator=gen)
    runs = []
    for _ in range(2):
        dg = torch.Generator(device="cuda").manual_seed(0)
        loss = tr.difference_loss_and_grads(frames, k, noise, conditions=acts, dropout_generator=dg)
        runs.append((float(loss.item()), tr.grads.clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert bool(torch.isfinite(runs[0][1]).all())
    assert float(tr.grad_dict()["external_cond_embedding.embedding.linear_1.weight"].abs().sum()) > 0
