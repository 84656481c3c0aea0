"""GPU tests of FacDiT and FacMatDiT at 64 patches per frame (latents 4x16x16 at patch 2, the taichi res-128 recipes), where the per-frame
spatial attention runs csrc/attention_seq64.hip: the forward against the reference's fixture (tests/golden/dit_p64.npz,
tools/make_golden_dit_p64.py), the sampler, the attention maps, and the recipe widths against the host restatements.

Bars (all taken from the existing DiT tests): forward against reference fixtures and fp32 restatements rel-L2 < 2e-2
(tests/test_gpu_dit_fac.py FIXTURE_BAR), sampler trace PSNR >= 35 dB (tests/test_gpu_dit_cond.py:187), frame maps rel-L2 < 2e-2
(tests/test_gpu_dit_attnmap.py).  Every test fails on the parent commit, whose DiT3D constructor raises ValueError at 64 patches per
frame."""
import math

import pytest
import torch

import dit_facmat_common as fm
import dit_p64_common as pc
from dit_p64_common import FIXTURE_BAR, T, rel

pytestmark = pytest.mark.gpu


def psnr(a, b):
    mse = ((a - b) ** 2).mean().item()
    peak = (b.max() - b.min()).item()
    return 10 * math.log10(peak * peak / max(mse, 1e-20))


@pytest.fixture(scope="module")
def g():
    return pc.load(pc.FIXTURE)


def _build(tag):
    kind, case = tag.split("_")
    return pc.build_fac(pc.FAC_CASES[case]) if kind == "fac" else pc.build_mat(case)


# ---------------------------------------------------------------------------------------------------------------- the forward
@pytest.mark.parametrize("tag", ["fac_mlp0", "fac_mlp4", "mat_b", "mat_d"])
def test_forward_vs_reference_fixture(g, tag):
    model, params = _build(tag)
    assert pc.digest(params) == str(g[f"digest_{tag}"])
    assert list(model.state_dict().keys()) == [str(n) for n in g[f"names_{tag}"]]
    x, k = T(g["x"]).cuda(), T(g["k"]).cuda()
    with torch.no_grad():
        o4 = model(x, k).cpu()
        o2 = model(x[:, :2].contiguous(), k[:, :2].contiguous()).cpu()  # T = 2 under max_tokens 4: one 128-row tile per video
    r4, r2 = rel(o4, T(g[f"out_{tag}_t4"])), rel(o2, T(g[f"out_{tag}_t2"]))
    print(f"64 patches per frame, {tag}: rel-L2 vs the reference T=4 {r4:.3e}, T=2 {r2:.3e}")
    assert torch.isfinite(o4).all() and torch.isfinite(o2).all()
    assert r4 < FIXTURE_BAR and r2 < FIXTURE_BAR


@pytest.mark.parametrize("tag,sens_key", [("fac_mlp0", "sens_frame3"), ("mat_b", "sens_frame3_mat")])
def test_frame_mixing_path_is_live(g, tag, sens_key):
    """frame 3 alone perturbed: frames 0-2 of the output move as they do in the reference (> 2x the parity bar)"""
    model, _ = _build(tag)
    k = T(g["k"]).cuda()
    with torch.no_grad():
        o4, o3 = model(T(g["x"]).cuda(), k).cpu(), model(T(g["x_frame3"]).cuda(), k).cpu()
    assert rel(o3, T(g[f"out_{tag}_frame3"])) < FIXTURE_BAR
    moved, want = rel(o3[:, :3], o4[:, :3]), float(g[sens_key])
    print(f"{tag}: frames 0-2 move by {moved:.3e} (reference {want:.3e})")
    assert want > 2 * FIXTURE_BAR
    assert abs(moved - want) < FIXTURE_BAR and moved > 2 * FIXTURE_BAR


def test_conditioned_forward_vs_reference_fixture(g):
    model, params = pc.build_fac(0.0, cond=True)
    assert pc.digest(params) == str(g["digest_fac_act"])
    assert list(model.state_dict().keys()) == [str(n) for n in g["names_fac_act"]]
    x, k, cond, mask = T(g["x"]).cuda(), T(g["k"]).cuda(), T(g["act_cond"]).cuda(), T(g["act_mask"]).cuda()
    with torch.no_grad():
        oa, om = model(x, k, cond).cpu(), model(x, k, cond, mask).cpu()
    ra, rm = rel(oa, T(g["out_act"])), rel(om, T(g["out_act_masked"]))
    print(f"FacDiT at 64 patches, action-conditioned: rel-L2 {ra:.3e}, with the per-video mask {rm:.3e}")
    assert ra < FIXTURE_BAR and rm < FIXTURE_BAR
    assert torch.equal(om[1], oa[1])  # the unmasked video is untouched by the other one's mask


@pytest.mark.parametrize("tag", ["fac_mlp0", "mat_b"])
def test_odd_token_count_is_refused_by_the_engine(g, tag):
    """T = 3 under max_tokens 4: 192 rows per video are no whole 128-row tiles; the engine refuses before any launch and stays usable"""
    model, _ = _build(tag)
    x, k = T(g["x"]).cuda(), T(g["k"]).cuda()
    with torch.no_grad():
        with pytest.raises((RuntimeError, ValueError), match="multiple of 128"):
            model(x[:, :3].contiguous(), k[:, :3].contiguous())
        out = model(x, k).cpu()
    assert rel(out, T(g[f"out_{tag}_t4"])) < FIXTURE_BAR


# ---------------------------------------------------------------------------------------------------------------- the sampler
def _sampler(model, noise_fn=None, steps=4):
    import dfot_amd
    cfg = dfot_amd.SamplerConfig(x_shape=pc.X_SHAPE, max_tokens=pc.MAX_TOKENS,
                                 diffusion=dfot_amd.DiffusionConfig(sampling_timesteps=steps, beta_schedule="cosine", is_continuous=False),
                                 prediction_guidance=dict(name="vanilla", guidance_scale=1.5))
    return dfot_amd.DFoTVideoSampler(cfg, model, noise_fn)


class HostBackbone:
    """the fp64 restatement behind the backbone interface the sampler uses: model(x, levels, cond, mask) and reserve()"""

    def __init__(self, fn):
        self.fn = fn

    def reserve(self, batch):
        pass

    def __call__(self, x, levels, cond=None, mask=None):
        return self.fn(x, levels).float().contiguous()


@pytest.mark.parametrize("tag", ["fac_mlp0", "mat_b"])
def test_sampler_graph_equals_eager_and_trace_vs_host(tag):
    """4 frames from 2 context frames.  (1) the captured step loop replays and is bit-identical to the eager one; (2) with every normal draw
    replayed, the run is within the sampler bar of the same sampler driving the fp64 host restatement"""
    model, params = _build(tag)
    gen = torch.Generator().manual_seed(5)
    vid = torch.randn(pc.BATCH, pc.MAX_TOKENS, *pc.X_SHAPE, generator=gen).cuda()

    def run(s, seed=3):
        dev = torch.Generator(device="cuda").manual_seed(seed)
        s.noise_fn = lambda tag_, shape: torch.randn(shape, device="cuda", generator=dev).clamp_(-20, 20)
        return s._predict_videos(vid, n_context_tokens=2, conditions=None)
    graph = _sampler(model, steps=6)
    assert graph.use_graph
    out = run(graph)
    assert graph.graph_captures == 1 and graph.graph_replays > 0
    eager = _sampler(model, steps=6)
    eager.use_graph = False
    ref = run(eager)
    assert eager.graph_replays == 0
    assert torch.isfinite(out).all() and torch.equal(out, ref)

    draws = []

    def record(tag_, shape):
        draws.append(torch.randn(shape, generator=gen).clamp_(-20, 20))
        return draws[-1].cuda()
    got = _sampler(model, record)._predict_videos(vid, n_context_tokens=2, conditions=None).cpu()
    queue = list(draws)

    def replay(tag_, shape):
        t = queue.pop(0)
        assert tuple(t.shape) == tuple(shape), (tag_, tuple(t.shape), tuple(shape))
        return t.cuda()
    dev_params = {n: t.cuda() for n, t in params.items()}
    kind, case = tag.split("_")
    host = HostBackbone((lambda x, lv: pc.fac_host(dev_params, x, lv)) if kind == "fac" else (lambda x, lv: pc.mat_host(case, dev_params, x, lv)))
    hs = _sampler(host, replay)
    hs.use_graph = False  # (the restatement builds its tables on the host: nothing to capture)
    want = hs._predict_videos(vid, n_context_tokens=2, conditions=None).cpu()
    assert not queue
    p = psnr(got, want)
    print(f"{tag} sampler at 64 patches: PSNR vs the fp64 restatement {p:.1f} dB")
    assert torch.equal(got[:, :2], want[:, :2])  # context tokens pass through untouched
    assert p >= 35.0


# ---------------------------------------------------------------------------------------------------------------- attention maps
@pytest.mark.parametrize("variant", ["fac", "facmat"])
def test_attention_maps_vs_host(g, variant):
    model, params = _build("fac_mlp0" if variant == "fac" else "mat_b")
    x, k = T(g["x"]).cuda(), T(g["k"]).cuda()
    with torch.no_grad():
        plain = model(x, k)
        model.capture_attention()
        try:
            captured = model(x, k)
            maps = model.attention_maps()
        finally:
            model.capture_attention(False)
    assert torch.equal(plain, captured)
    want = pc.host_frame_maps(variant, {n: t.cuda() for n, t in params.items()}, x, k)
    assert list(maps) == list(want)
    for name, f in maps.items():
        w = want[name]
        assert tuple(f.shape) == tuple(w.shape)
        r = rel(f.cpu(), w.cpu())
        uniform = rel(w.cpu(), torch.full_like(w, 1.0 / w.shape[-1]).cpu())
        print(f"{variant} {name} at 64 patches: frame map rel-L2 vs the fp64 host map {r:.3e} (the map is {uniform:.3e} from uniform)")
        assert uniform > pc.CONTRAST_BAR  # the comparison can tell a wrong map from a right one
        assert r < pc.MAP_BAR
        assert (f.double().sum(-1) - 1).abs().max().item() <= 1e-4


# ---------------------------------------------------------------------------------------------------------------- recipe width
def _width_case(cfg, host, heads_note):
    import dfot_amd
    model = dfot_amd.DiT3D(cfg, x_shape=pc.X_SHAPE, max_tokens=16).cuda().eval()
    model.init_random(11)
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(2, 16, *pc.X_SHAPE, generator=gen).cuda()
    k = torch.randint(0, 1000, (2, 16), generator=gen).cuda()
    with torch.no_grad():
        out = model(x, k)
        ref = host({n: t.detach() for n, t in model.state_dict().items()}, x, k)
    assert torch.isfinite(out).all()
    r = rel(out.cpu(), ref.cpu())
    print(f"{heads_note} forward (2 x 16 x 64 tokens): rel-L2 vs the fp32 restatement {r:.3e}")
    assert r < FIXTURE_BAR


def test_recipe_width_facmat_s_64_1():
    """@FacMatDiT/S-64-1 of the res-128 ladder: embed_row_dim 384, 12 spatial heads (d = 32), embed_col_dim 64, 1 x 6 matrix heads, bias,
    temporal RoPE, depth 2 instead of 6; latents 4x16x16 at patch 2, 16 frames, batch 2"""
    over = dict(hidden_size=384, depth=2, num_heads=12, max_tokens=16)
    _width_case(fm.backbone_cfg(1, 6, True, 4.0, True, **{**pc.OVER, **over}),
                lambda p, x, k: fm.forward_host(p, x, k, 1, 6, True, dtype=torch.float32, **{**pc.OVER, **over}), "FacMatDiT-S-64-1 at 64 patches")


def test_recipe_width_facdit_s():
    """@FacDiT/S: hidden 384, 6 heads (d = 64), depth 2 instead of 6; the same shape"""
    over = dict(hidden_size=384, depth=2, num_heads=6, max_tokens=16)
    _width_case(pc.fac_cfg(4.0, **over), lambda p, x, k: pc.fac_host(p, x, k, dtype=torch.float32, **over), "FacDiT-S at 64 patches")
