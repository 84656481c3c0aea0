"""GPU checks of the pose-free U-ViT (dfot_amd.UViT3D, dfot_uvit3d_*) at the fixture's configuration (tests/uvit3d_common.TINY: the smallest
the engine accepts -- head dims 64 and 128, 128 tokens at the coarsest level).

Bars
  * whole forward vs the reference fixture: rel-L2 < 2e-2, the project's bar for the U-ViT engine against a reference fixture
    (tests/test_gpu_backbone.py:12).  The fixture keeps the reference outputs on the lattice uvit3d_common.sample(): compared there.
  * "nemb" tap vs the fp64 restatement: rel-L2 < 1e-5, the bar of the "cond_emb" tap of the DiT engine (tests/test_gpu_dit_cont.py:70,80).
  * sampler trace: PSNR >= 35 dB (tests/test_gpu_dit_cond.py:187).
  * pose-free norm kernels vs fp64.  The inference forms of these kernels had no op-level test to take a bar from (the op tests of
    tests/test_gpu_train_ops.py:642-656 cover the training kernel dfot_op_rms_film_fwd), so the bar is derived from the formats.  The kernel
    evaluates y in fp32 from exact inputs (bf16 activations, fp32 constants) and rounds once to bf16:
        |got - ref| <= 2^-8 (|ref| + d) + d,   d = 2^-18 * mag,
    2^-8 |v| = half a bf16 ulp of the value rounded; d = 64 fp32 ulps of mag, the sum of the absolute values of the terms of y (about
    ten roundings in the chain, the 64-lane + 4-chunk sum of squares of the RMS form, and a fast exponential and division inside SiLU,
    whose derivative is below 1.1); the SiLU form takes mag through the same bound since |silu'| <= 1.1.
"""
import ctypes
import math

import pytest
import torch

import uvit3d_common as uc
from uvit3d_common import T, rel

pytestmark = pytest.mark.gpu

BAR = 2e-2
TAP_BAR = 1e-5


@pytest.fixture(scope="module")
def g():
    return uc.load()


@pytest.fixture(scope="module")
def inp():
    x, levels, cond, mask = uc.inputs()
    return x.cuda(), levels.cuda(), cond.cuda(), mask.cuda()


_MODELS = {}


def model_of(tag):
    if tag not in _MODELS:
        _MODELS[tag] = uc.build(tag)
    return _MODELS[tag]


def run(model, *a):
    with torch.no_grad():
        return model(*a)


# ---------------------------------------------------------------------------------------------------------------- module
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_state_dict_names_order_and_shapes_equal_the_reference(g, tag):
    import dfot_amd
    model, _ = model_of(tag)
    names, shapes = [str(n) for n in g[f"names_{tag}"]], [str(s) for s in g[f"shapes_{tag}"]]
    sd = model.state_dict()
    assert list(sd) == names
    assert [" ".join(map(str, t.shape)) for t in sd.values()] == shapes
    assert dfot_amd.checkpoint.reference_parameter_order(model) == [n for n in names if not n.endswith((".freqs", ".phases"))]
    # a reference checkpoint (Lightning key prefix) loads through the checkpoint reader
    fresh = dfot_amd.UViT3D(uc.backbone_cfg(uc.CASES[tag][1]), x_shape=uc.X_SHAPE, max_tokens=uc.MAX_TOKENS, external_cond_dim=uc.CASES[tag][0])
    ignored = dfot_amd.load_reference_checkpoint(fresh, {"state_dict": {"diffusion_model.model." + k: v.cpu() for k, v in sd.items()}})
    assert ignored == [] and all(torch.equal(v.cpu(), fresh.state_dict()[k]) for k, v in sd.items())


def test_forward_is_refused_under_autograd_and_checks_its_arguments(inp):
    x, levels, cond, mask = inp
    model, _ = model_of("a")
    with pytest.raises(NotImplementedError, match="training and reconstruction guidance"):
        model(x, levels)
    with pytest.raises(AssertionError, match="Temporal length of U-ViT is set to 8"):
        run(model, x[:, :5], levels[:, :5])
    with pytest.raises(ValueError, match="external_cond_dim 0"):
        run(model, x, levels, cond)
    mc, _ = model_of("c")
    with pytest.raises(AssertionError, match="embedding mask should be of shape"):
        run(mc, x, levels, cond, mask[:, None])
    with pytest.raises(ValueError, match="is on cpu"):
        run(mc, x, levels, cond.cpu())


# ---------------------------------------------------------------------------------------------------------------- 1-3, 7: forward
@pytest.mark.parametrize("tag", ["a", "b", "c", "c_masked"])
def test_forward_vs_reference_fixture(g, inp, tag):
    x, levels, cond, mask = inp
    model, _ = model_of(tag[0])
    out = run(model, x, levels, None if tag == "a" else cond, mask if tag == "c_masked" else None).cpu()
    r = rel(uc.sample(out), T(g[f"out_{tag}"]))
    print(f"UViT3D {tag}: rel-L2 vs the reference fixture {r:.3e}")
    assert torch.isfinite(out).all() and r < BAR


def test_mask_bit_identities(inp):
    x, levels, cond, mask = inp
    model, _ = model_of("c")
    masked, plain, none = run(model, x, levels, cond, mask), run(model, x, levels, cond), run(model, x, levels)
    assert torch.equal(masked[0], none[0])       # the masked video runs exactly as without a condition
    assert torch.equal(masked[1], plain[1])      # the other video does not see its neighbour's mask
    assert not torch.equal(plain[0], none[0])    # ... and the condition is live
    mb, _ = model_of("b")                        # built with dropout 0: the mask is ignored (embeddings.py:385-386)
    assert torch.equal(run(mb, x, levels, cond, mask), run(mb, x, levels, cond))
    mc_train = model.train()
    try:
        mc_train._dropout_generator = torch.Generator(device="cuda").manual_seed(1)
        with pytest.raises(AssertionError, match="only allowed during inference"):
            run(model, x, levels, cond, mask)
        drawn = run(model, x, levels, cond)      # train(): one Bernoulli(0.1) per video from _dropout_generator
        draw = torch.rand(2, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) < uc.COND_DROPOUT
        for v in range(2):
            assert torch.equal(drawn[v], (none if draw[v] else plain)[v])
    finally:
        model.eval()


def test_batch_invariance(inp):
    x, levels, cond, _ = inp
    model, _ = model_of("b")
    both = run(model, x, levels, cond)
    alone = run(model, x[1:].contiguous(), levels[1:].contiguous(), cond[1:].contiguous())
    assert torch.equal(alone[0], both[1])


def test_live_frames_leave_live_outputs_bit_identical(inp):
    x, levels, cond, _ = inp
    model, _ = model_of("b")
    full = run(model, x, levels, cond)
    live = torch.ones(2, uc.MAX_TOKENS, dtype=torch.uint8, device="cuda")
    live[:, :2] = 0
    live[1, 5] = 0
    model.live_frames = live
    try:
        part = run(model, x, levels, cond)
    finally:
        model.live_frames = None
    keep = live.bool()
    assert torch.equal(part[keep], full[keep])
    assert not part[~keep].any()  # dead frames: zeros are written
    assert torch.equal(run(model, x, levels, cond), full)


# ---------------------------------------------------------------------------------------------------------------- 4: norm kernels
def _engine_cols(scale, shift):
    """(rows, C) scale and shift -> (rows, 2C) in the engine's column order: per 64 columns, 32 scale then the 32 matching shift columns"""
    rows, c = scale.shape
    return torch.stack([scale.reshape(rows, c // 32, 32), shift.reshape(rows, c // 32, 32)], dim=2).reshape(rows, 2 * c).contiguous()


def _check(name, got, ref, mag):
    d = 2.0 ** -18 * mag
    bar = 2.0 ** -8 * (ref.abs() + d) + d
    err = (got.double() - ref).abs()
    worst = float((err / bar).max())
    print(f"{name}: worst error / bar {worst:.3f}, max abs error {float(err.max()):.3e}")
    assert torch.isfinite(got).all() and worst <= 1.0


@pytest.mark.parametrize("c", [128, 256])
@pytest.mark.parametrize("side", [8, 16])
def test_gn_film_silu_pose_free_vs_float64_and_masked_pose_kernel(c, side):
    from dfot_amd import capi
    bt, pix = 2, side * side
    gen = torch.Generator().manual_seed(100 * c + side)
    h = (1.5 * torch.randn(bt * pix, c, generator=gen) + 0.3).to(torch.bfloat16)
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=gen), 0.2 * torch.randn(c, generator=gen)
    scale, shift = 0.5 * torch.randn(bt, c, generator=gen), 0.5 * torch.randn(bt, c, generator=gen)
    hd = h.double().reshape(bt, pix, 32, c // 32)
    mean = hd.mean(dim=(1, 3))
    rstd = (hd.var(dim=(1, 3), unbiased=False) + 1e-6).rsqrt()
    stats = torch.stack([mean, rstd], dim=-1).float().contiguous()  # what gn_finalize hands over: fp32 (mean, rstd) per (frame, group)
    m64, r64 = stats[..., 0].double().repeat_interleave(c // 32, dim=1)[:, None], stats[..., 1].double().repeat_interleave(c // 32, dim=1)[:, None]
    n = (h.double().reshape(bt, pix, c) - m64) * r64 * gamma.double() + beta.double()
    y = n * (1 + scale.double()[:, None]) + shift.double()[:, None]
    ref = (y * torch.sigmoid(y)).reshape(bt * pix, c)
    mag = ((((h.double().reshape(bt, pix, c) - m64).abs() * r64 * gamma.double().abs() + beta.double().abs()) * (1 + scale.double().abs()[:, None])
            + shift.double().abs()[:, None]).reshape(bt * pix, c))
    sv = _engine_cols(scale, shift)
    dev = [t.cuda() for t in (h, stats, gamma, beta, sv)]
    P, S = capi.ptr, capi.stream_ptr
    out = torch.full((bt * pix + 8, c), float("nan"), dtype=torch.bfloat16, device="cuda")
    capi.check(capi.lib.dfot_op_gn_film_silu(P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), None, P(dev[4]), None, P(out), bt, pix, c, 1, S()))
    assert torch.isnan(out[bt * pix:]).all()  # nothing written past the end
    _check(f"gn_film_silu pose-free C={c} {side}x{side}", out[:bt * pix].cpu(), ref, mag)
    # the existing kernel with every video masked does the same arithmetic and only adds the (skipped) cache loads: same bits
    fcache = torch.randn(bt * pix, 2 * c, generator=gen).to(torch.bfloat16).cuda()
    masked = torch.ones(bt, dtype=torch.uint8, device="cuda")
    out2 = torch.full_like(out, float("nan"))
    capi.check(capi.lib.dfot_op_gn_film_silu(P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), P(fcache), P(dev[4]), P(masked), P(out2), bt, pix, c, 1, S()))
    assert torch.equal(out2[:bt * pix], out[:bt * pix])
    # ... and unmasked it adds the cache: the pose path is still the pose path
    none = torch.zeros(bt, dtype=torch.uint8, device="cuda")
    capi.check(capi.lib.dfot_op_gn_film_silu(P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), P(fcache), P(dev[4]), P(none), P(out2), bt, pix, c, 1, S()))
    assert not torch.equal(out2[:bt * pix], out[:bt * pix])


@pytest.mark.parametrize("c", [128, 256])
@pytest.mark.parametrize("rows", [128, 256])
def test_rms_film_pose_free_vs_float64_and_masked_pose_kernel(c, rows):
    from dfot_amd import capi
    bt = 2
    gen = torch.Generator().manual_seed(7 * c + rows)
    x = (1.5 * torch.randn(rows, c, generator=gen)).to(torch.bfloat16)
    w = 1 + 0.2 * torch.randn(c, generator=gen)
    scale, shift = 0.5 * torch.randn(bt, c, generator=gen), 0.5 * torch.randn(bt, c, generator=gen)
    xd = x.double()
    rs = (xd.pow(2).mean(-1, keepdim=True) + 1e-6).rsqrt()
    sc = scale.double().repeat_interleave(rows // bt, dim=0)
    sh = shift.double().repeat_interleave(rows // bt, dim=0)
    ref = xd * rs * w.double() * (1 + sc) + sh
    mag = xd.abs() * rs * w.double().abs() * (1 + sc.abs()) + sh.abs()
    dev = [t.cuda() for t in (x, w, _engine_cols(scale, shift))]
    P, S = capi.ptr, capi.stream_ptr
    out = torch.full((rows + 8, c), float("nan"), dtype=torch.bfloat16, device="cuda")
    capi.check(capi.lib.dfot_op_rms_film(P(dev[0]), P(dev[1]), None, P(dev[2]), None, P(out), rows, c, rows // bt, 1, 1e-6, S()))
    assert torch.isnan(out[rows:]).all()
    _check(f"rms_film pose-free C={c} rows={rows}", out[:rows].cpu(), ref, mag)
    fcache = torch.randn(rows, 2 * c, generator=gen).to(torch.bfloat16).cuda()
    masked = torch.ones(bt, dtype=torch.uint8, device="cuda")
    out2 = torch.full_like(out, float("nan"))
    capi.check(capi.lib.dfot_op_rms_film(P(dev[0]), P(dev[1]), P(fcache), P(dev[2]), P(masked), P(out2), rows, c, rows // bt, 1, 1e-6, S()))
    assert torch.equal(out2[:rows], out[:rows])
    none = torch.zeros(bt, dtype=torch.uint8, device="cuda")
    capi.check(capi.lib.dfot_op_rms_film(P(dev[0]), P(dev[1]), P(fcache), P(dev[2]), P(none), P(out2), rows, c, rows // bt, 1, 1e-6, S()))
    assert not torch.equal(out2[:rows], out[:rows])


def test_norm_op_entry_points_refuse_bad_arguments():
    from dfot_amd import capi
    P, S, L = capi.ptr, capi.stream_ptr, capi.lib
    f, hb = torch.zeros(4096, device="cuda"), torch.zeros(4096, dtype=torch.bfloat16, device="cuda")
    assert L.dfot_op_gn_film_silu(P(hb), P(f), P(f), P(f), None, None, None, P(hb), 1, 16, 128, 1, S()) == capi.ERR_ARG
    assert L.dfot_op_gn_film_silu(P(hb), P(f), P(f), P(f), None, P(f), None, P(hb), 1, 16, 100, 1, S()) == capi.ERR_SHAPE
    assert L.dfot_op_rms_film(P(hb), None, None, P(f), None, P(hb), 16, 128, 8, 1, 1e-6, S()) == capi.ERR_ARG
    assert L.dfot_op_rms_film(P(hb), P(f), None, P(f), None, P(hb), 16, 128, 5, 1, 1e-6, S()) == capi.ERR_SHAPE
    assert b"rows_per_bt" in L.dfot_last_error()


# ---------------------------------------------------------------------------------------------------------------- 5: embedding kernel
@pytest.mark.parametrize("case", ["a", "c_masked", "c_dim3_masked"])
def test_embedding_tap_vs_float64(inp, case):
    x, levels, cond, mask = inp
    if case == "a":
        (model, p), c, m = model_of("a"), None, None
    elif case == "c_masked":
        (model, p), c, m = model_of("c"), cond, mask
    else:  # an odd condition width: rows of the first action layer are not 16-byte aligned
        (model, p), m = uc.build("c", cond_dim=3), mask
        c = torch.randn(uc.BATCH, uc.MAX_TOKENS, 3, generator=torch.Generator().manual_seed(9)).cuda()
    run(model, x, levels, c, m)
    got = model.read_nemb(uc.BATCH).cpu()
    want = uc.embedding(p, levels.cpu(), None if c is None else c.cpu(), None if m is None else m.cpu(), torch.float64).reshape(-1, got.shape[-1])
    r = rel(got, want)
    print(f"nemb {case}: rel-L2 vs float64 {r:.3e}")
    assert r < TAP_BAR
    if m is not None:  # the masked video's embedding is the noise term alone
        noise_only = uc.embedding(p, levels.cpu(), None, None, torch.float64).reshape(-1, got.shape[-1])
        assert rel(got[:uc.MAX_TOKENS], noise_only[:uc.MAX_TOKENS]) < TAP_BAR
        assert rel(got[uc.MAX_TOKENS:], noise_only[uc.MAX_TOKENS:]) > 1e-2


# ---------------------------------------------------------------------------------------------------------------- 6: sampler
class ReplayList:
    strict_order = True

    def __init__(self, draws):
        self.queue = list(draws)

    def __call__(self, tag, shape):
        t = self.queue.pop(0)
        assert tuple(t.shape) == tuple(shape), (tag, tuple(t.shape), tuple(shape))
        return (t if tag == "excluded" else t.clamp(-20, 20)).cuda()


def _sampler(model, steps, noise_fn=None):
    import dfot_amd
    cfg = dfot_amd.SamplerConfig(x_shape=uc.X_SHAPE, max_tokens=uc.MAX_TOKENS, diffusion=dfot_amd.DiffusionConfig(sampling_timesteps=steps, is_continuous=True),
                                 prediction_guidance=dict(name="vanilla", guidance_scale=1.5), external_cond_type="action", external_cond_dim=uc.COND_DIM)
    return dfot_amd.DFoTVideoSampler(cfg, model, noise_fn)


def test_sampler_trace_vs_reference_and_graph_equals_eager(g):
    model, _ = model_of("b")
    shapes = [tuple(int(v) for v in str(s).split()) for s in g["run_draw_shapes"]]
    draws = uc.trace_draws(shapes)
    assert uc.tensor_digest(*draws) == str(g["run_draws_digest"])
    vid, cond = uc.trace_inputs()
    assert uc.tensor_digest(vid, cond) == str(g["run_inputs_digest"])
    nfn = ReplayList(draws)
    out = _sampler(model, 3, nfn)._predict_videos(vid.cuda(), n_context_tokens=2, conditions=cond.cuda()).cpu()
    assert not nfn.queue
    ref = T(g["run_pred"])
    mse = ((uc.sample(out) - ref) ** 2).mean().item()
    peak = float(g["run_pred_max"]) - float(g["run_pred_min"])
    psnr = 10 * math.log10(peak * peak / max(mse, 1e-20))
    print(f"UViT3D sampler trace PSNR {psnr:.1f} dB")
    assert torch.equal(out[:, :2], vid[:, :2]) and psnr >= 35.0

    def seeded(seed):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        return lambda tag, shape: torch.randn(shape, device="cuda", generator=gen).clamp_(-20, 20)
    graph = _sampler(model, 6, seeded(3))
    assert graph.use_graph
    og = graph._predict_videos(vid.cuda(), n_context_tokens=2, conditions=cond.cuda())
    assert graph.graph_captures == 1 and graph.graph_replays > 0
    eager = _sampler(model, 6, seeded(3))
    eager.use_graph = False
    oe = eager._predict_videos(vid.cuda(), n_context_tokens=2, conditions=cond.cuda())
    assert eager.graph_replays == 0 and torch.equal(og, oe)


# ---------------------------------------------------------------------------------------------------------------- 8: C ABI errors
def test_abi_errors(inp):
    from dfot_amd import capi
    x, levels, cond, mask = inp
    L, P, S = capi.lib, capi.ptr, capi.stream_ptr
    model, params = uc.build("a")
    h = model._handle

    def err():
        return L.dfot_last_error().decode()
    w = torch.zeros(4, device="cuda")
    shape = (ctypes.c_int64 * 1)(4)
    assert L.dfot_uvit_load_weight(h, b"external_cond_embedding.linear_1.bias", P(w), shape, 1, S()) == capi.ERR_NAME and "unexpected key" in err()
    # a fresh handle with one key left out: finalize names it
    fresh = type(model)(uc.backbone_cfg(), x_shape=uc.X_SHAPE, max_tokens=uc.MAX_TOKENS, external_cond_dim=0).cuda()
    first = fresh._names[0]
    for name in fresh._names[1:]:
        t = params[name].cuda().contiguous()
        capi.check(L.dfot_uvit_load_weight(fresh._handle, name.encode(), P(t), (ctypes.c_int64 * t.ndim)(*t.shape), t.ndim, S()))
    assert L.dfot_uvit_finalize(fresh._handle, S()) == capi.ERR_STATE and f"missing key '{first}'" in err()
    out = torch.empty_like(x)
    run(model, x[:1].contiguous(), levels[:1].contiguous())  # syncs the weights and reserves a batch of 1
    assert model._reserved == 1
    assert L.dfot_uvit3d_forward(h, P(x), P(levels), None, None, P(out), 2, S()) == capi.ERR_STATE and "exceeds reserved 1" in err()
    assert L.dfot_uvit3d_forward(h, P(x), P(levels), P(cond), None, P(out), 1, S()) == capi.ERR_ARG and "cond_dim 0" in err()
    assert L.dfot_uvit3d_forward(h, None, P(levels), None, None, P(out), 1, S()) == capi.ERR_ARG
    # the two handle forms do not serve each other's forwards
    assert L.dfot_uvit_forward_cached(h, P(x), P(levels), P(out), 1, S()) == capi.ERR_STATE and "pose-free" in err()
    assert L.dfot_uvit_set_conditions(h, P(x), None, 1, S()) == capi.ERR_STATE and "pose-free" in err()
    assert L.dfot_uvit_read_tap(h, b"pose_emb0", P(out), out.numel(), S()) == capi.ERR_NAME
    assert L.dfot_uvit_read_tap(h, b"nemb", P(out), 4, S()) == capi.ERR_SHAPE
    torch.cuda.synchronize()
