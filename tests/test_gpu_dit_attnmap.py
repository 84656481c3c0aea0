"""GPU tests of the attention-map capture of the DiT3D family (DiT3D.capture_attention / attention_maps, SamplerConfig.attention_map_steps)
against the reference's maps in tests/golden/dit_attnmap.npz (tools/make_golden_dit_attnmap.py).

Bar: every captured frame map, and the one stored full map, within rel-L2 < 2e-2 of the fixture -- the project's forward-vs-reference bar
(tests/test_gpu_dit.py:150).  The fixture's own conditions (every map >= 4e-2 away from uniform and from its transpose; the bf16 host
restatement within 1e-2) are asserted by tests/test_dit_attnmap_host.py.  Every test fails on the parent commit, whose DiT3D has no
capture_attention."""
import pytest
import torch

import dit_attnmap_common as am
from dit_attnmap_common import T, rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return am.load("dit_attnmap.npz")


@pytest.fixture(scope="module")
def models(g):
    """one engine model per variant, built once"""
    return {v: am.build(v, float(g[f"gain_{v}"])) for v in am.VARIANTS}


def _inputs(g, tokens=am.TOKENS):
    return T(g["x"])[:, :tokens].contiguous().cuda(), T(g["k"])[:, :tokens].contiguous().cuda()


@pytest.mark.parametrize("variant", am.VARIANTS)
def test_frame_maps_vs_reference_fixture(g, models, variant):
    """parity of every frame-mixing block; the forward output with capture on is bit-identical to capture off, before and after"""
    import dfot_amd
    model, params = models[variant]
    assert am.fm.digest(params) == str(g[f"digest_{variant}"])
    x, k = _inputs(g)
    with torch.no_grad():
        plain = model(x, k)
        model.capture_attention()
        try:
            with pytest.raises(RuntimeError, match="no forward has run"):
                model.attention_maps()
            captured = model(x, k)
            maps = model.attention_maps()
        finally:
            model.capture_attention(False)
        after = model(x, k)
    assert torch.equal(plain, captured) and torch.equal(plain, after)
    with pytest.raises(RuntimeError, match="capture is off"):
        model.attention_maps()
    assert list(maps) == am.block_names(variant) == list(model.attention_block_names())
    for i, (name, f) in enumerate(maps.items()):
        want = T(g[f"frame_{variant}_{i}"])
        assert f.is_cuda and f.dtype == torch.float32 and tuple(f.shape) == am.map_shape(variant, 2) == tuple(want.shape)
        r = rel(f.cpu(), want)
        rows = (f.double().sum(-1) - 1).abs().max().item()
        print(f"{variant} {name}: frame map rel-L2 vs the reference {r:.3e}, rows sum to 1 within {rows:.1e}")
        assert r < am.PARITY_BAR
        assert rows <= 1e-4
    assert dfot_amd.frame_map is not None


def test_full_map_vs_reference_fixture(g, models):
    """the stored full map (block 1, video 1, head 2, T = 2) and, from the same capture, frame_map of the full maps against a frame capture"""
    import dfot_amd
    model, _ = models["full"]
    x, k = _inputs(g, am.FULL_TOKENS)
    name = am.block_names("full")[am.FULL_BLOCK]
    with torch.no_grad():
        plain = model(x, k)
        model.capture_attention([name], form="full")
        try:
            out = model(x, k)
            full = model.attention_maps()
            model.capture_attention([name], form="frame")
            model(x, k)
            frame = model.attention_maps()[name]
        finally:
            model.capture_attention(False)
    assert torch.equal(plain, out)
    assert list(full) == [name]
    n = am.FULL_TOKENS * am.PATCHES
    assert tuple(full[name].shape) == (2, am.HEADS, n, n)
    got = dfot_amd.to_hook_layout(full[name], am.FULL_TOKENS, am.HEIGHT, am.WIDTH)[am.FULL_BATCH_ROW, am.FULL_HEAD].cpu()
    r = rel(got, T(g["full_hook"]))
    print(f"full map of {name}: rel-L2 vs the reference's attn_map {r:.3e} (bf16 host restatement: {float(g['restate_full_map']):.3e})")
    assert r < am.PARITY_BAR
    assert (dfot_amd.frame_map(full[name], am.FULL_TOKENS) - frame).abs().max().item() <= 1e-4


def test_refusals_by_name(g, models):
    import dfot_amd
    full, _ = models["full"]
    with pytest.raises(ValueError, match="unknown block 'dit_base.blocks.7.attn'"):
        full.capture_attention(["dit_base.blocks.7.attn"])
    with pytest.raises(ValueError, match="unknown block 'dit_base.temporal_blocks.0.attn'"):
        full.capture_attention(["dit_base.temporal_blocks.0.attn"])
    with pytest.raises(ValueError, match="form 'both'"):
        full.capture_attention(form="both")
    for v in ("fac", "facmat"):
        model, _ = models[v]
        with pytest.raises(ValueError, match="'dit_base.blocks.0.attn' is a spatial block"):
            model.capture_attention(["dit_base.blocks.0.attn"])
        assert not model.capturing_attention
    with pytest.raises(ValueError, match="form='full' is not available on variant 'factorized_attention'"):
        models["fac"][0].capture_attention(form="full")
    # a full capture above max_bytes: 2 blocks x 5 videos... the map of ONE video is 4 heads x 640^2 x 4 B = 6.5 MB per block
    x, k = _inputs(g)
    with torch.no_grad():
        full(x, k)  # reserves batch 2
    with pytest.raises(ValueError, match=r"need \d+ bytes .* above max_bytes 1000000"):
        full.capture_attention(form="full", max_bytes=1_000_000)
    assert not full.capturing_attention
    with pytest.raises(RuntimeError, match="capture is off"):
        full.attention_maps()
    full.capture_attention(form="full", max_bytes=32 << 20)  # 2 blocks x 2 videos x 6.5 MB fit
    try:
        with pytest.raises(ValueError, match="above max_bytes"):  # ... 8 videos do not: refused when the workspace grows
            with torch.no_grad():
                full(x.repeat(4, 1, 1, 1, 1), k.repeat(4, 1))
    finally:
        full.capture_attention(False)
    cfg = dict(name="difference_dit3d", variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", merge_type="interleaved", patch_size=1,
               embed_col_dim=64, embed_row_dim=128, num_heads=4, num_col_heads=1, num_row_heads=4, depth=1, mlp_ratio=4.0, spatial_mlp_ratio=4.0,
               use_bias=True, matrix_block="matrix")
    diff = dfot_amd.DifferenceDiT3D(cfg, x_shape=(4, 16, 8), max_tokens=2).cuda()
    with pytest.raises(NotImplementedError, match="DifferenceDiT3D"):
        diff.capture_attention()
    from dfot_amd import capi
    assert capi.lib.dfot_dit_capture_attention(diff._handle, None, 0, capi.ATTN_MAP_FRAME, 0) == capi.ERR_ARG
    assert b"difference model" in capi.lib.dfot_last_error()
    trainer = dfot_amd.DiT3DTrainer(am.engine_cfg("full"), x_shape=(4, 16, 8), max_tokens=5)
    with pytest.raises(NotImplementedError, match="DiT3DTrainer is a training engine"):
        trainer.capture_attention()


def test_c_abi_state_and_selection(g, models):
    """the C entry points: DFOT_ERR_STATE until a forward has run with capture on, a subset of blocks, shape and copy"""
    import ctypes as C
    from dfot_amd import capi
    model, _ = models["fac"]
    h = model._handle
    shape, ndim = (C.c_int64 * 5)(), C.c_int()
    out = torch.zeros(2 * am.HEADS * 25, device="cuda")
    assert capi.lib.dfot_dit_attention_map_shape(h, 0, shape, C.byref(ndim)) == capi.ERR_STATE
    assert capi.lib.dfot_dit_read_attention_map(h, 0, capi.ptr(out), out.numel(), capi.stream_ptr()) == capi.ERR_STATE
    bad = (C.c_int32 * 2)(1, 0)
    assert capi.lib.dfot_dit_capture_attention(h, bad, 2, capi.ATTN_MAP_FRAME, 0) == capi.ERR_ARG
    assert capi.lib.dfot_dit_capture_attention(h, (C.c_int32 * 1)(2), 1, capi.ATTN_MAP_FRAME, 0) == capi.ERR_ARG
    model.capture_attention(["dit_base.temporal_blocks.1.attn"])
    try:
        assert capi.lib.dfot_dit_read_attention_map(h, 0, capi.ptr(out), out.numel(), capi.stream_ptr()) == capi.ERR_STATE
        x, k = _inputs(g)
        with torch.no_grad():
            model(x, k)
        capi.check(capi.lib.dfot_dit_attention_map_shape(h, 0, shape, C.byref(ndim)))
        assert [shape[i] for i in range(ndim.value)] == [2, am.HEADS, am.TOKENS, am.TOKENS]
        assert capi.lib.dfot_dit_read_attention_map(h, 0, capi.ptr(out), 10, capi.stream_ptr()) == capi.ERR_SHAPE
        assert capi.lib.dfot_dit_read_attention_map(h, 1, capi.ptr(out), out.numel(), capi.stream_ptr()) == capi.ERR_ARG
        maps = model.attention_maps()
        assert list(maps) == ["dit_base.temporal_blocks.1.attn"]
        assert rel(maps["dit_base.temporal_blocks.1.attn"].cpu(), T(g["frame_fac_1"])) < am.PARITY_BAR
    finally:
        model.capture_attention(False)


def test_sampler_collects_the_listed_steps(g, models):
    """a 3-step run with attention_map_steps=[0, 2]: maps for exactly those steps, batch rows = batch x NFE (vanilla guidance: 2 branches),
    and the sampled video bit-identical to an eager run without capture"""
    import dfot_amd
    model, _ = models["fac"]
    vid = T(g["x"]).cuda()

    def sampler(steps_listed):
        cfg = dfot_amd.SamplerConfig(x_shape=(4, 16, 8), max_tokens=5,
                                     diffusion=dfot_amd.DiffusionConfig(sampling_timesteps=3, beta_schedule="cosine", is_continuous=False),
                                     prediction_guidance=dict(name="vanilla", guidance_scale=1.5), attention_map_steps=steps_listed)
        s = dfot_amd.DFoTVideoSampler(cfg, model)
        gen = torch.Generator(device="cuda").manual_seed(5)
        s.noise_fn = lambda tag, shape: torch.randn(shape, device="cuda", generator=gen).clamp_(-20, 20)
        return s
    plain = sampler(())
    assert plain.cfg.attention_map_steps == () and plain.attention_maps == {}
    plain.use_graph = False
    want = plain._predict_videos(vid, n_context_tokens=2, conditions=None)
    assert plain.attention_maps == {}
    cap = sampler([0, 2])
    assert cap.use_graph  # the window that collects falls back to the eager loop by itself
    got = cap._predict_videos(vid, n_context_tokens=2, conditions=None)
    assert cap.graph_captures == 0
    assert torch.equal(got, want)
    assert sorted(cap.attention_maps) == [0, 2]
    for step, rec in cap.attention_maps.items():
        assert list(rec) == ["noise_levels"] + am.block_names("fac")
        assert tuple(rec["noise_levels"].shape) == (2 * 2, am.TOKENS)
        for name in am.block_names("fac"):
            f = rec[name]
            assert tuple(f.shape) == (2 * 2, am.HEADS, am.TOKENS, am.TOKENS)
            assert (f.double().sum(-1) - 1).abs().max().item() <= 1e-4
    assert not model.capturing_attention  # the sampler turned on what it needed and turned it off again
