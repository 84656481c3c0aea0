"""GPU tests of FacMatDiT at narrow column widths (embed_col_dim 1 .. 32, the rungs S-1-1 .. S-32-4 of the @FacMatDiT ladder), where the left
factors of the matrix blocks run csrc/facmat_narrow.hip: the matrix attention op at these widths, the forward against the reference's
fixture (tests/golden/dit_facmat_narrow.npz, tools/make_golden_dit_facmat_narrow.py), batch invariance, the action condition, the sampler,
the attention maps, a weight reload, and the odd-T refusal at 64 patches.

Bars (all taken from the existing DiT tests): matrix attention op rel-L2 < 1.5e-2 (tests/test_gpu_dit_facmat.py:19), forward against the
reference fixture rel-L2 < FIXTURE_BAR = 2e-2 (tests/dit_p64_common.py:16), sampler trace PSNR >= 35 dB (tests/test_gpu_dit_cond.py:187),
frame maps rel-L2 < MAP_BAR with the contrast assertion beside it (tests/test_gpu_dit_p64.py:180-184).

Every test that builds a model fails on the parent commit, where dfot_dit_create refuses the width ("embed_col_dim %d must be a multiple
of 64").  The matrix attention op test alone passes there: the kernel took any E with E % cc == 0 before, and the test pins that the narrow
engine path may rely on it."""
import math

import pytest
import torch

import dit_facmat_common as fm
import dit_facmat_narrow_common as nc
from dit_facmat_narrow_common import FIXTURE_BAR, T, rel

pytestmark = pytest.mark.gpu
OP_BAR = 1.5e-2  # tests/test_gpu_dit_facmat.py:19


def psnr(a, b):
    mse = ((a - b) ** 2).mean().item()
    peak = (b.max() - b.min()).item()
    return 10 * math.log10(peak * peak / max(mse, 1e-20))


@pytest.fixture(scope="module")
def g():
    return nc.load(nc.FIXTURE)


def _build(g, tag, patches=128, cond=False):
    return nc.build(tag, float(g[f"gain_{tag}"]), patches, cond)


# ---------------------------------------------------------------------------------------------------------------- the attention kernel
@pytest.mark.parametrize("e,cc", [(1, 1), (8, 1), (8, 4), (32, 1), (32, 4)])
def test_matrix_attention_at_narrow_widths_vs_fp64(e, cc):
    """dfot_op_matrix_attention_rope at E in {1, 8, 32}, cc in {1, 4} (cc divides E) against tests/test_gpu_dit_facmat.py's fp64 reference,
    with and without the rotation"""
    from dfot_amd import capi
    batch, rr, h = 2, 4, 128
    for tokens in (1, 5, 16):
        gen = torch.Generator().manual_seed(100 * e + 10 * cc + tokens)
        # unit-variance scores at any E: q, k entries ~ N(0, 1) and scale = (E/cc * h/rr)^-1/2
        z = torch.randn(batch * tokens * e, 3 * h, generator=gen).to(torch.bfloat16).float()
        for rope in (True, False):
            ref, w = fm.matrix_attention_ref(z, batch, tokens, e, h, cc, rr, rope)
            table = fm.rope_table(tokens, h // rr).cuda() if rope else None
            zd = z.to(torch.bfloat16).cuda()
            o = torch.full((batch * tokens * e, h), float("nan"), dtype=torch.bfloat16, device="cuda")
            scale = 1.0 / math.sqrt((e // cc) * (h // rr))
            capi.check(capi.lib.dfot_op_matrix_attention_rope(capi.ptr(zd), capi.ptr(o), capi.ptr(table), batch, tokens, e, h, cc, rr, scale,
                                                              capi.stream_ptr()))
            torch.cuda.synchronize()
            got = o.float().cpu()
            assert torch.isfinite(got).all()
            r = rel(got, ref)
            print(f"matrix attention E={e} cc={cc} L={tokens} rope={rope}: rel-L2 {r:.2e}")
            assert r < OP_BAR


# ---------------------------------------------------------------------------------------------------------------- the forward
@pytest.mark.parametrize("tag", list(nc.CASES))
def test_forward_vs_reference_fixture(g, tag):
    model, params = _build(g, tag)
    assert nc.digest(params) == str(g[f"digest_{tag}"])
    assert list(model.state_dict().keys()) == [str(n) for n in g[f"names_{tag}"]]
    x, k = (t.cuda() for t in nc.inputs(g))
    with torch.no_grad():
        o5 = model(x, k).cpu()
        o3 = model(x[:, :3].contiguous(), k[:, :3].contiguous()).cpu()  # T = 3 after T = 5: pad rows of the right-factor GEMM hold old frames
    r5, r3 = rel(o5, T(g[f"out_{tag}_t5"])), rel(o3, T(g[f"out_{tag}_t3"]))
    print(f"FacMatDiT {tag} {nc.CASES[tag]}: rel-L2 vs the reference T=5 {r5:.3e}, T=3 {r3:.3e}")
    assert torch.isfinite(o5).all() and torch.isfinite(o3).all()
    assert r5 < FIXTURE_BAR and r3 < FIXTURE_BAR


@pytest.mark.parametrize("tag", nc.P64_TAGS)
def test_forward_vs_reference_fixture_at_64_patches(g, tag):
    model, params = _build(g, tag, 64)
    assert nc.digest(params) == str(g[f"digest64_{tag}"])
    assert list(model.state_dict().keys()) == [str(n) for n in g[f"names64_{tag}"]]
    x, k = (t.cuda() for t in nc.inputs(g, 64))
    with torch.no_grad():
        o4 = model(x, k).cpu()
        o2 = model(x[:, :2].contiguous(), k[:, :2].contiguous()).cpu()
    r4, r2 = rel(o4, T(g[f"out64_{tag}_t4"])), rel(o2, T(g[f"out64_{tag}_t2"]))
    print(f"FacMatDiT {tag} at 64 patches: rel-L2 vs the reference T=4 {r4:.3e}, T=2 {r2:.3e}")
    assert torch.isfinite(o4).all() and torch.isfinite(o2).all()
    assert r4 < FIXTURE_BAR and r2 < FIXTURE_BAR


@pytest.mark.parametrize("tag", ["e1", "e3", "e32"])
def test_batch_invariance(g, tag):
    """a video alone gives the bits it gives in a batch of two: 5 / 15 / 160 rows of the right-factor GEMM instead of 10 / 30 / 320"""
    model, _ = _build(g, tag)
    x, k = (t.cuda() for t in nc.inputs(g))
    with torch.no_grad():
        both = model(x, k)
        alone = model(x[1:2].contiguous(), k[1:2].contiguous())
    assert torch.equal(both[1:2], alone)


def test_conditioned_forward_vs_reference_fixture(g):
    model, params = _build(g, nc.COND_TAG, cond=True)
    assert nc.digest(params) == str(g["digest_act"])
    assert list(model.state_dict().keys()) == [str(n) for n in g["names_act"]]
    x, k = (t.cuda() for t in nc.inputs(g))
    cond, mask = T(g["act_cond"]).cuda(), T(g["act_mask"]).cuda()
    with torch.no_grad():
        oa, om = model(x, k, cond).cpu(), model(x, k, cond, mask).cpu()
    ra, rm = rel(oa, T(g["out_act"])), rel(om, T(g["out_act_masked"]))
    print(f"FacMatDiT {nc.COND_TAG}, action-conditioned: rel-L2 {ra:.3e}, with the per-video mask {rm:.3e}")
    assert ra < FIXTURE_BAR and rm < FIXTURE_BAR
    assert rel(om[0], T(g["out_act_masked"])[0]) < FIXTURE_BAR  # the masked video on its own
    assert torch.equal(om[1], oa[1])  # the unmasked video is untouched by the other one's mask


def test_reload_of_a_second_state_dict_changes_the_output(g):
    """the factors the two kernels read follow load_state_dict + sync_weights: other qkv_u / proj_u alone move the output, and the first
    weights give the first bits again"""
    tag = "e8"
    model, params = _build(g, tag)
    x, k = (t.cuda() for t in nc.inputs(g))
    with torch.no_grad():
        first = model(x, k).clone()
    other = {n: t.clone() for n, t in params.items()}
    gen = torch.Generator().manual_seed(9)
    for n in other:
        if n.endswith(("attn.qkv_u", "attn.proj_u")):
            other[n] = torch.randn(other[n].shape, generator=gen) / math.sqrt(other[n].shape[0])
    model.load_state_dict(other, strict=True)
    with torch.no_grad():
        second = model(x, k).clone()
        want = nc.host(tag, {n: t.cuda() for n, t in other.items()}, x, k, dtype=torch.float32)
    assert rel(second.cpu(), first.cpu()) > 2 * FIXTURE_BAR
    assert rel(second.cpu(), want.cpu()) < FIXTURE_BAR
    model.load_state_dict(params, strict=True)
    with torch.no_grad():
        assert torch.equal(model(x, k), first)


def test_attn_timing_counts_the_spatial_launches(g):
    model, _ = _build(g, "e8")
    model.sync_weights()
    model.set_option("time_attn", 16)
    x, k = (t.cuda() for t in nc.inputs(g))
    with torch.no_grad():
        model(x, k)
    total, launches = model.attn_timing()
    model.set_option("time_attn", 0)
    assert launches == 2 and total > 0


@pytest.mark.parametrize("tag", nc.P64_TAGS)
def test_odd_token_count_at_64_patches_is_refused_and_the_handle_stays_usable(g, tag):
    model, _ = _build(g, tag, 64)
    x, k = (t.cuda() for t in nc.inputs(g, 64))
    with torch.no_grad():
        with pytest.raises((RuntimeError, ValueError), match="multiple of 128"):
            model(x[:, :3].contiguous(), k[:, :3].contiguous())
        out = model(x, k).cpu()
    assert rel(out, T(g[f"out64_{tag}_t4"])) < FIXTURE_BAR


# ---------------------------------------------------------------------------------------------------------------- the sampler
class ReplayList:
    strict_order = True

    def __init__(self, draws):
        self.queue = list(draws)

    def __call__(self, tag, shape):
        t = self.queue.pop(0)
        assert tuple(t.shape) == tuple(shape), (tag, tuple(t.shape), tuple(shape))
        return (t if tag == "excluded" else t.clamp(-20, 20)).cuda()


def _sampler(model, noise_fn=None, steps=3):
    import dfot_amd
    cfg = dfot_amd.SamplerConfig(x_shape=(4, 16, 8), max_tokens=5,
                                 diffusion=dfot_amd.DiffusionConfig(sampling_timesteps=steps, beta_schedule="cosine", is_continuous=False),
                                 prediction_guidance=dict(name="vanilla", guidance_scale=1.5))
    return dfot_amd.DFoTVideoSampler(cfg, model, noise_fn)


def test_sampler_trace_vs_reference_fixture(g):
    model, _ = _build(g, nc.TRACE_TAG)
    nfn = ReplayList([T(g[f"run_noise{i}"]) for i in range(int(g["run_n_noise"]))])
    out = _sampler(model, nfn)._predict_videos(T(g["run_vid"]).cuda(), n_context_tokens=2, conditions=None).cpu()
    assert not nfn.queue
    ref = T(g["run_pred"])
    p = psnr(out, ref)
    print(f"FacMatDiT {nc.TRACE_TAG} sampler: PSNR vs the reference's run {p:.1f} dB")
    assert torch.equal(out[:, :2], ref[:, :2])  # context tokens pass through untouched
    assert p >= 35.0


@pytest.mark.parametrize("tag", ["e1", "e8"])
def test_graph_step_loop_equals_eager(g, tag):
    """the captured step loop replays (the row workspaces are sized at reserve: nothing is allocated inside) and is bit-identical"""
    model, _ = _build(g, tag)
    vid = T(g["run_vid"]).cuda()

    def run(s, seed=3):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        s.noise_fn = lambda tag_, shape: torch.randn(shape, device="cuda", generator=gen).clamp_(-20, 20)
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


# ---------------------------------------------------------------------------------------------------------------- attention maps
@pytest.mark.parametrize("tag,patches", [("e1", 128), ("e8", 128), ("e32", 128), ("e3", 128), ("e32", 64)])
def test_attention_maps_vs_host(g, tag, patches):
    model, params = _build(g, tag, patches)
    x, k = (t.cuda() for t in nc.inputs(g, patches))
    with torch.no_grad():
        plain = model(x, k)
        model.capture_attention()
        try:
            captured = model(x, k)
            maps = model.attention_maps()
        finally:
            model.capture_attention(False)
    assert torch.equal(plain, captured)
    want = nc.host_frame_maps(tag, {n: t.cuda() for n, t in params.items()}, x, k, patches)
    assert list(maps) == list(want)
    for name, f in maps.items():
        w = want[name]
        assert tuple(f.shape) == tuple(w.shape)
        r = rel(f.cpu(), w.cpu())
        uniform = rel(w.cpu(), torch.full_like(w, 1.0 / w.shape[-1]).cpu())
        print(f"{tag} {name} at {patches} patches: frame map rel-L2 vs the fp64 host map {r:.3e} (the map is {uniform:.3e} from uniform)")
        assert uniform > nc.CONTRAST_BAR  # the comparison can tell a wrong map from a right one
        assert r < nc.MAP_BAR
        assert (f.double().sum(-1) - 1).abs().max().item() <= 1e-4
