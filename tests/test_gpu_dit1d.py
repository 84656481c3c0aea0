"""GPU tests of the DiT1D backbone (dfot_amd.DiT1D, csrc/dit1d.hip, csrc/attention_frame_causal.hip) against the reference's fixture
tests/golden/dit1d.npz (tools/make_golden_dit1d.py): the forward with and without the frame-causal mask at both head shapes, causality at
model level bit for bit, the state dict, the sampler (recorded trace, hipGraph against eager, the engine against the fp64 host
restatement), and the refusals at call time.

Bars (all taken from the existing DiT tests): forward against a reference fixture rel-L2 < 2e-2 (tests/test_gpu_dit_fac.py FIXTURE_BAR),
sampler trace PSNR >= 35 dB (tests/test_gpu_dit_cond.py:187).  Every test fails on the parent commit: dfot_amd.DiT1D does not exist."""
import math

import pytest
import torch

import dit1d_common as dc
from dit1d_common import FIXTURE_BAR, T, rel

pytestmark = pytest.mark.gpu


def psnr(a, b):
    mse = ((a - b) ** 2).mean().item()
    peak = (b.max() - b.min()).item()
    return 10 * math.log10(peak * peak / max(mse, 1e-20))


@pytest.fixture(scope="module")
def g():
    return dc.load()


@pytest.fixture(scope="module")
def inp(g):
    x, k = dc.inputs()
    assert dc.tensor_digest(x, k) == str(g["inputs_digest"])
    return x.cuda(), k.cuda()


_MODELS = {}


def model_of(g, tag, mode="video_temporal_causal", gain=None):
    gain = float(g["qk_gain"]) if gain is None else gain
    key = (tag, mode, gain)
    if key not in _MODELS:
        _MODELS[key] = dc.build(tag, gain, mode)
    return _MODELS[key]


# ---------------------------------------------------------------------------------------------------------------- the forward
@pytest.mark.parametrize("tag", list(dc.CASES))
def test_forward_vs_reference_fixture_and_the_mask_is_on(g, inp, tag):
    """Measured on MI355X when this test was written (rel-L2): see DESIGN.md, the DiT1D section."""
    model, params = model_of(g, tag)
    assert dc.digest(params) == str(g[f"digest_{tag}"])
    plain, _ = model_of(g, tag, None)
    with torch.no_grad():
        oc, on = model(*inp).cpu(), plain(*inp).cpu()
        ot = model_of(g, tag, "temporal_causal")[0](*inp).cpu()
    rc, rn = rel(oc, T(g[f"out_causal_{tag}"])), rel(on, T(g[f"out_nomask_{tag}"]))
    away = rel(oc, T(g[f"out_nomask_{tag}"]))
    print(f"DiT1D {tag}: rel-L2 vs the reference causal {rc:.3e}, no mask {rn:.3e}; causal result vs the reference's unmasked output {away:.3e} "
          f"(recorded sensitivity {float(g['sens_nomask']):.3e})")
    assert tuple(oc.shape) == tuple(inp[0].shape) and torch.isfinite(oc).all() and torch.isfinite(on).all()
    assert rc < FIXTURE_BAR and rn < FIXTURE_BAR
    assert torch.equal(ot, oc)  # temporal_causal: the same mask without context tokens
    assert float(g["sens_nomask"]) >= dc.SENS_FLOOR
    assert away > dc.SENS_FLOOR - FIXTURE_BAR  # the mask is on: the recorded sensitivity minus one bar


@pytest.mark.parametrize("tag", list(dc.CASES))
def test_model_level_causality_bit_for_bit(g, inp, tag):
    """x and noise_levels of frames >= 5 changed: frames < 5 of the output keep their bits, the later ones move"""
    model, _ = model_of(g, tag)
    x, k = inp
    x2, k2 = x.clone(), k.clone()
    x2[:, 5:] = x2[:, 5:] * -1.5 + 0.25
    k2[:, 5:] = (k2[:, 5:] + 371) % dc.TIMESTEPS
    with torch.no_grad():
        a, b = model(x, k), model(x2, k2)
        pa, pb = (model_of(g, tag, None)[0](xx, kk) for xx, kk in ((x, k), (x2, k2)))
    assert torch.equal(a[:, :5], b[:, :5])
    assert not torch.equal(a[:, 5:], b[:, 5:])
    assert not torch.equal(pa[:, :5], pb[:, :5])  # without the mask the early frames do see the later ones


def test_key_order_load_and_reload(g, inp):
    import dfot_amd
    model, params = model_of(g, "h4")
    assert list(model.state_dict().keys()) == [str(n) for n in g["names_h4"]]
    assert [" ".join(map(str, t.shape)) for t in model.state_dict().values()] == [str(s) for s in g["shapes_h4"]]
    fresh = dfot_amd.DiT1D(dc.backbone_cfg(4), x_shape=dc.X_SHAPE, max_tokens=dc.MAX_TOKENS).cuda().eval()
    n_tok = dc.MAX_TOKENS * dc.X_SHAPE[2]
    assert (fresh.pos_embed[0].double().cpu() - torch.from_numpy(dc.sincos_formula(128, n_tok))).abs().max() < 1e-6
    assert not fresh.pos_embed.requires_grad
    assert fresh.num_patches == dc.X_SHAPE[2] and fresh.max_tokens == dc.MAX_TOKENS and fresh.x_shape == dc.X_SHAPE
    with pytest.raises(RuntimeError, match="Missing key"):
        fresh.load_state_dict({n: t for n, t in params.items() if n != "pos_embed"}, strict=True)
    fresh.load_state_dict(params, strict=True)
    with torch.no_grad():
        want = model(*inp)
        assert torch.equal(fresh(*inp), want)
        # a reload of changed weights is picked up: the loaded pos_embed is used (not a recomputed table), and so is a changed matrix
        changed = dict(params, pos_embed=params["pos_embed"] * 0.5)
        fresh.load_state_dict(changed, strict=True)
        moved = fresh(*inp)
        assert rel(moved.cpu(), want.cpu()) > FIXTURE_BAR
        ref = dc.forward_host({n: t.cuda() for n, t in changed.items()}, *inp, dc.CASES["h4"]).cpu()
        assert rel(moved.cpu(), ref) < FIXTURE_BAR
        fresh.load_state_dict(params, strict=True)
        assert torch.equal(fresh(*inp), want)


def test_refusals_at_call_time_leave_the_model_usable(g, inp):
    model, _ = model_of(g, "h4")
    x, k = inp
    with torch.no_grad():
        want = model(x, k)
        with pytest.raises(ValueError, match="max_tokens"):
            model(x[:, :4].contiguous(), k[:, :4].contiguous())
        with pytest.raises(TypeError, match="continuous diffusion"):
            model(x, k.float())
        with pytest.raises(ValueError, match="external_cond"):
            model(x, k, torch.zeros(dc.BATCH, dc.MAX_TOKENS, 3, device="cuda"))
        assert torch.equal(model(x, k), want)
    for p in model.parameters():
        assert p.requires_grad == (p is not model.pos_embed)
    with pytest.raises(NotImplementedError, match="forward only"):
        model(x, k)


# ---------------------------------------------------------------------------------------------------------------- the sampler
class ReplayList:
    strict_order = True

    def __init__(self, draws):
        self.queue = list(draws)

    def __call__(self, tag, shape):
        t = self.queue.pop(0)
        assert tuple(t.shape) == tuple(shape), (tag, tuple(t.shape), tuple(shape))
        return (t if tag == "excluded" else t.clamp(-20, 20)).cuda()


class HostBackbone:
    """the fp64 restatement behind the backbone interface the sampler uses: model(x, levels, cond, mask) and reserve()"""

    def __init__(self, fn):
        self.fn = fn

    def reserve(self, batch):
        pass

    def __call__(self, x, levels, cond=None, mask=None):
        return self.fn(x, levels).float().contiguous()


def _sampler(model, steps, noise_fn=None):
    import dfot_amd
    cfg = dfot_amd.SamplerConfig(x_shape=dc.X_SHAPE, max_tokens=dc.MAX_TOKENS,
                                 diffusion=dfot_amd.DiffusionConfig(sampling_timesteps=steps, beta_schedule="cosine", is_continuous=False),
                                 prediction_guidance=dict(name="vanilla", guidance_scale=1.5))
    return dfot_amd.DFoTVideoSampler(cfg, model, noise_fn)


def _trace_draws(g):
    shapes = [tuple(int(v) for v in str(s).split()) for s in g["run_draw_shapes"]]
    draws = dc.trace_draws(shapes)
    assert dc.tensor_digest(*draws) == str(g["run_draws_digest"])
    return draws


def test_sampler_trace_vs_reference(g):
    model, params = model_of(g, "h4", gain=float(g["run_qk_gain"]))
    assert dc.digest(params) == str(g["run_digest"])
    vid = dc.trace_inputs()
    assert dc.tensor_digest(vid) == str(g["run_inputs_digest"])
    nfn = ReplayList(_trace_draws(g))
    out = _sampler(model, 3, nfn)._predict_videos(vid.cuda(), n_context_tokens=2, conditions=None).cpu()
    assert not nfn.queue
    p = psnr(out, T(g["run_pred"]))
    print(f"DiT1D sampler trace: PSNR vs the reference's run {p:.1f} dB")
    assert torch.equal(out[:, :2], vid[:, :2]) and p >= 35.0


def test_sampler_graph_equals_eager_and_engine_vs_host(g):
    model, params = model_of(g, "h4", gain=float(g["run_qk_gain"]))
    vid = dc.trace_inputs().cuda()

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

    dev_params = {n: t.cuda() for n, t in params.items()}
    host = _sampler(HostBackbone(lambda x, lv: dc.forward_host(dev_params, x, lv, dc.CASES["h4"])), 3, ReplayList(_trace_draws(g)))
    host.use_graph = False  # (the restatement builds its tables on the host: nothing to capture)
    want = host._predict_videos(vid, n_context_tokens=2, conditions=None).cpu()
    got = _sampler(model, 3, ReplayList(_trace_draws(g)))._predict_videos(vid, n_context_tokens=2, conditions=None).cpu()
    p = psnr(got, want)
    print(f"DiT1D sampler: PSNR of the engine vs the fp64 restatement behind the same sampler {p:.1f} dB")
    assert torch.equal(got[:, :2], want[:, :2]) and p >= 35.0
