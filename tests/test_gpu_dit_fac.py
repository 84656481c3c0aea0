"""GPU tests of the factorized-attention DiT3D (variant "factorized_attention", pos_emb_type "sinusoidal_factorized"): the temporal
attention kernel at the op level, the forward against the reference's fixture (tests/golden/dit_fac.npz, tools/make_golden_dit_fac.py),
the sampler trace, and a full-size forward against the host restatement.

Bars (all taken from the existing DiT tests): the op against an fp64 softmax rel-L2 < 1.5e-2 (tests/test_gpu_dit.py:88), the forward
against reference fixtures rel-L2 < 2e-2 (tests/test_gpu_dit.py:150), the sampler trace PSNR >= 35 dB (tests/test_gpu_dit_cond.py:187).
Every forward test fails on the parent commit, whose DiT3D constructor raises ValueError for this variant."""
import math

import pytest
import torch

import dit_fac_common as fc
from dit_fac_common import T, rel

pytestmark = pytest.mark.gpu

FIXTURE_BAR = 2e-2


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


# ---------------------------------------------------------------------------------------------------------------- the kernel
def _temporal_case(tokens, d, patches, batch, heads=2, seed=0):
    """operands as the per-frame QKV epilogue leaves them: [(b t)][heads][P][dstride] bf16, q scaled into the exp2 domain, pads zero"""
    g = torch.Generator().manual_seed(seed + 1000 * tokens + d)
    q, k, v = (torch.randn(batch * tokens, heads, patches, d, generator=g) for _ in range(3))
    ds = 64 if d <= 64 else 128
    scale = math.log2(math.e) / math.sqrt(d)

    def pad(t, mul=1.0):
        out = torch.zeros(batch * tokens, heads, patches, ds, dtype=torch.bfloat16, device="cuda")
        out[..., :d] = (t * mul).to(torch.bfloat16).cuda()
        return out
    return (q, k, v), (pad(q, scale), pad(k), pad(v))


def _run_temporal(dev, tokens, d, patches, batch, heads=2):
    from dfot_amd import capi
    o = torch.full((batch * tokens * patches, heads * d), float("nan"), dtype=torch.bfloat16, device="cuda")
    capi.check(capi.lib.dfot_op_attention_temporal(capi.ptr(dev[0]), capi.ptr(dev[1]), capi.ptr(dev[2]), capi.ptr(o), heads * d, batch, tokens,
                                                   patches, heads, d, capi.stream_ptr()))
    torch.cuda.synchronize()
    return o


def _reference(host, tokens, d, patches, batch, heads=2):
    """fp64 softmax(q k^T / sqrt(d)) v over the frames of every (video, head, patch) from the bf16-rounded operands"""
    q, k, v = (t.to(torch.bfloat16).double().reshape(batch, tokens, heads, patches, d).permute(0, 2, 3, 1, 4) for t in host)  # b h p t d
    w = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), -1)
    return (w @ v).permute(0, 3, 2, 1, 4).reshape(batch * tokens * patches, heads * d)  # (b t p), (h d)


@pytest.mark.parametrize("d", [32, 64, 72])
@pytest.mark.parametrize("tokens", [1, 2, 3, 5, 16, 17, 32])
def test_attention_temporal_vs_fp64(tokens, d):
    for patches in (128, 256):
        for batch in (1, 3):
            host, dev = _temporal_case(tokens, d, patches, batch)
            got = _run_temporal(dev, tokens, d, patches, batch).float().cpu()
            assert torch.isfinite(got).all()
            r = rel(got, _reference(host, tokens, d, patches, batch))
            print(f"temporal attention T={tokens} d={d} P={patches} B={batch}: rel-L2 {r:.2e}")
            assert r < 1.5e-2


@pytest.mark.parametrize("tokens,d", [(3, 72), (16, 64), (17, 32)])
def test_attention_temporal_patch_positions_are_independent(tokens, d):
    """perturbing q, k, v of ONE patch position (all frames, all heads) leaves every other position's output rows bitwise unchanged"""
    patches, batch, p = 128, 2, 37
    _, dev = _temporal_case(tokens, d, patches, batch)
    base = _run_temporal(dev, tokens, d, patches, batch).reshape(batch, tokens, patches, -1)
    dev2 = [t.clone() for t in dev]
    for t in dev2:
        t[:, :, p, :d] = (t[:, :, p, :d].float() * -1.5 + 0.25).to(torch.bfloat16)
    moved = _run_temporal(dev2, tokens, d, patches, batch).reshape(batch, tokens, patches, -1)
    keep = [i for i in range(patches) if i != p]
    assert torch.equal(base[:, :, keep], moved[:, :, keep])
    assert not torch.equal(base[:, :, p], moved[:, :, p])


def test_attention_temporal_invalid_shapes():
    from dfot_amd import capi
    z = torch.zeros(64 * 128 * 128, dtype=torch.bfloat16, device="cuda")
    o = torch.zeros(64 * 128 * 128, dtype=torch.bfloat16, device="cuda")

    def call(ldo, batch, tokens, patches, heads, d):
        return capi.lib.dfot_op_attention_temporal(capi.ptr(z), capi.ptr(z), capi.ptr(z), capi.ptr(o), ldo, batch, tokens, patches, heads, d,
                                                   capi.stream_ptr())
    assert call(64, 1, 4, 128, 1, 64) == capi.OK
    for args in ((64, 1, 0, 128, 1, 64), (64, 1, 33, 128, 1, 64), (64, 1, 4, 64, 1, 64), (64, 1, 4, 192, 1, 64), (66, 1, 4, 128, 1, 66),
                 (136, 1, 4, 128, 1, 136), (32, 1, 4, 128, 1, 64), (64, 0, 4, 128, 1, 64), (64, 1, 4, 128, 0, 64)):
        assert call(*args) == capi.ERR_SHAPE, args
        assert capi.lib.dfot_last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the forward
@pytest.fixture(scope="module")
def g():
    return fc.load("dit_fac.npz")


@pytest.mark.parametrize("tag,ratio", [("mlp0", 0.0), ("mlp4", 4.0)])
def test_forward_vs_reference_fixture(g, tag, ratio):
    model, params = fc.build(ratio)
    assert fc.digest(params) == str(g[f"digest_{tag}"])
    assert list(model.state_dict().keys()) == [str(n) for n in g[f"names_{tag}"]]
    x, k = T(g["x"]).cuda(), T(g["k"]).cuda()
    with torch.no_grad():
        o5 = model(x, k).cpu()
        o3 = model(x[:, :3].contiguous(), k[:, :3].contiguous()).cpu()  # T = 3 under max_tokens 5: the first rows of the temporal table
    r5, r3 = rel(o5, T(g[f"out_{tag}_t5"])), rel(o3, T(g[f"out_{tag}_t3"]))
    print(f"factorized DiT {tag}: rel-L2 vs the reference T=5 {r5:.3e}, T=3 {r3:.3e}")
    assert r5 < FIXTURE_BAR and r3 < FIXTURE_BAR


def test_temporal_path_is_live(g):
    """frame 4 alone perturbed: frames 0-3 of the output move as they do in the reference (sens_frame4, > 2x the parity bar)"""
    model, _ = fc.build(0.0)
    k = T(g["k"]).cuda()
    with torch.no_grad():
        o5, o4 = model(T(g["x"]).cuda(), k).cpu(), model(T(g["x_frame4"]).cuda(), k).cpu()
    assert rel(o4, T(g["out_mlp0_frame4"])) < FIXTURE_BAR
    moved, want = rel(o4[:, :4], o5[:, :4]), float(g["sens_frame4"])
    print(f"frames 0-3 move by {moved:.3e} (reference {want:.3e})")
    assert want > 2 * FIXTURE_BAR
    assert abs(moved - want) < FIXTURE_BAR and moved > 2 * FIXTURE_BAR


def test_conditioned_forward_vs_reference_fixture(g):
    model, params = fc.build(0.0, cond=True)
    assert fc.digest(params) == str(g["digest_act"])
    assert list(model.state_dict().keys()) == [str(n) for n in g["names_act"]]
    x, k, cond, mask = T(g["x"]).cuda(), T(g["k"]).cuda(), T(g["act_cond"]).cuda(), T(g["act_mask"]).cuda()
    with torch.no_grad():
        oa, om = model(x, k, cond).cpu(), model(x, k, cond, mask).cpu()
    ra, rm = rel(oa, T(g["out_act"])), rel(om, T(g["out_act_masked"]))
    print(f"factorized DiT, action-conditioned: rel-L2 {ra:.3e}, with the per-video mask {rm:.3e}")
    assert ra < FIXTURE_BAR and rm < FIXTURE_BAR
    assert rel(om[0], T(g["out_act_masked"])[0]) < FIXTURE_BAR  # the masked video on its own
    assert torch.equal(om[1], oa[1])  # the unmasked video is untouched by the other one's mask


def test_batch_invariance(g):
    model, _ = fc.build(4.0)
    x, k = T(g["x"]).cuda(), T(g["k"]).cuda()
    with torch.no_grad():
        both = model(x, k)
        alone = model(x[1:2].contiguous(), k[1:2].contiguous())
    assert torch.equal(both[1:2], alone)


def test_load_state_dict_is_strict_and_training_is_refused(g):
    import dfot_amd
    model, params = fc.build(0.0)
    with pytest.raises(RuntimeError):
        model.load_state_dict({n: t for n, t in params.items() if "temporal_blocks.1.attn.qkv" not in n}, strict=True)
    x = T(g["x"]).cuda().requires_grad_()
    with pytest.raises(NotImplementedError, match="inference only"):
        model(x, T(g["k"]).cuda())
    with pytest.raises(ValueError, match="no training path"):
        dfot_amd.DiT3DTrainer(fc.backbone_cfg(0.0), x_shape=(4, 16, 8), max_tokens=5)


def test_attn_timing_counts_the_temporal_launches(g):
    model, _ = fc.build(0.0)
    model.sync_weights()
    model.set_option("time_attn", 16)
    with torch.no_grad():
        model(T(g["x"]).cuda(), T(g["k"]).cuda())
    total, launches = model.attn_timing()
    model.set_option("time_attn", 0)
    assert launches == 4 and total > 0  # depth 2: two spatial + two temporal attention launches


# ---------------------------------------------------------------------------------------------------------------- the sampler
def _sampler(model, noise_fn=None, steps=3):
    import dfot_amd
    cfg = dfot_amd.SamplerConfig(x_shape=(4, 16, 8), max_tokens=5,
                                 diffusion=dfot_amd.DiffusionConfig(sampling_timesteps=steps, beta_schedule="cosine", is_continuous=False),
                                 prediction_guidance=dict(name="vanilla", guidance_scale=1.5))
    return dfot_amd.DFoTVideoSampler(cfg, model, noise_fn)


def test_sampler_trace_vs_reference_fixture(g):
    model, _ = fc.build(0.0)
    nfn = ReplayList([T(g[f"run_noise{i}"]) for i in range(int(g["run_n_noise"]))])
    out = _sampler(model, nfn)._predict_videos(T(g["run_vid"]).cuda(), n_context_tokens=2, conditions=None).cpu()
    assert not nfn.queue
    ref = T(g["run_pred"])
    p = psnr(out, ref)
    print(f"factorized DiT sampler: PSNR vs the reference's run {p:.1f} dB")
    assert torch.equal(out[:, :2], ref[:, :2])  # context tokens pass through untouched
    assert p >= 35.0


def test_graph_step_loop_equals_eager(g):
    model, _ = fc.build(0.0)
    vid = T(g["run_vid"]).cuda()

    def run(s, seed=3):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        s.noise_fn = lambda tag, shape: torch.randn(shape, device="cuda", generator=gen).clamp_(-20, 20)
        return s._predict_videos(vid, n_context_tokens=2, conditions=None)
    graph = _sampler(model, steps=6)
    assert graph.use_graph
    out = run(graph)
    assert graph.graph_captures == 1 and graph.graph_replays > 0
    eager = _sampler(model, steps=6)
    eager.use_graph = False
    ref = run(eager)
    assert eager.graph_replays == 0
    assert torch.equal(out, ref)


# ---------------------------------------------------------------------------------------------------------------- full size
def test_full_size_forward_vs_host_restatement():
    """The taichikl FacDiT-XL shape: hidden 1152, depth 28 + 28, 16 heads (d = 72), 4x32x32 latents, patch 2 (P = 256), T = 16, model batch 2,
    against dit_fac_common.forward_host run on the GPU in fp32.  Bar: rel-L2 < 2e-2 on the output (tests/test_gpu_dit.py:171)."""
    import dfot_amd
    over = dict(hidden_size=1152, depth=28, num_heads=16, patch_size=2, resolution=(32, 32), max_tokens=16)
    model = dfot_amd.DiT3D(fc.backbone_cfg(0.0, **over), x_shape=(4, 32, 32), max_tokens=16).cuda().eval()
    model.init_random(11)
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(2, 16, 4, 32, 32, generator=gen).cuda()
    k = torch.randint(0, 1000, (2, 16), generator=gen).cuda()
    with torch.no_grad():
        out = model(x, k)
        ref = fc.forward_host({n: t.detach() for n, t in model.state_dict().items()}, x, k, dtype=torch.float32, **over)
    assert torch.isfinite(out).all()
    r = rel(out.cpu(), ref.cpu())
    print(f"FacDiT-XL forward (2 x 16 x 256 tokens): rel-L2 vs the fp32 restatement {r:.3e}")
    assert r < 2e-2
