"""GPU tests of the FacMatDiT backbone (DiT3D, variant "factorized_matrix_attention", pos_emb_type "sinusoidal_2d", use_temporal_rope):
the matrix attention kernel with the temporal RoPE at the op level, the forward against the reference's fixture
(tests/golden/dit_facmat.npz, tools/make_golden_dit_facmat.py), the sampler, and an S-64-1-width forward against the host restatement.

Bars (all taken from the existing DiT tests): the op against an fp64 softmax rel-L2 < 1.5e-2 (tests/test_gpu_dit.py:88), the forward
against reference fixtures and against the restatement rel-L2 < 2e-2 (tests/test_gpu_dit.py:150), the sampler trace PSNR >= 35 dB
(tests/test_gpu_dit_cond.py:187).  Every test here fails on the parent commit: its library exports neither op entry point and its DiT3D
constructor raises ValueError for this variant."""
import math

import pytest
import torch

import dit_facmat_common as fm
from dit_facmat_common import T, rel

pytestmark = pytest.mark.gpu

OP_BAR = 1.5e-2
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
def _run_op(z, batch, tokens, h, cc, rr, table, e=fm.OP_E):
    from dfot_amd import capi
    zd = z.to(torch.bfloat16).cuda()
    o = torch.full((batch * tokens * e, h), float("nan"), dtype=torch.bfloat16, device="cuda")
    scale = 1.0 / math.sqrt((e // cc) * (h // rr))
    capi.check(capi.lib.dfot_op_matrix_attention_rope(capi.ptr(zd), capi.ptr(o), capi.ptr(table), batch, tokens, e, h, cc, rr, scale,
                                                      capi.stream_ptr()))
    torch.cuda.synchronize()
    return o


def _run_variant1_op(z, batch, tokens, h, cc, rr, e=fm.OP_E):
    """the DifferenceDiT3D engine's own launcher (matrix_attn_kernel, no rotation)"""
    from dfot_amd import capi
    zd = z.to(torch.bfloat16).cuda()
    o = torch.full((batch * tokens * e, h), float("nan"), dtype=torch.bfloat16, device="cuda")
    capi.check(capi.lib.dfot_op_matrix_attention(capi.ptr(zd), capi.ptr(o), batch, tokens, e, h, cc, rr, 1.0 / math.sqrt((e // cc) * (h // rr)),
                                                 capi.stream_ptr()))
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("tokens", fm.OP_TOKENS)
def test_matrix_attention_rope_vs_fp64(tokens):
    """both with and without the table, at every head shape (hd in {32, 64, 72}, hn in {64, 32}); batch 2.  The fp64 side is checked not to
    be degenerate: the largest probability of a row lies in (0.05, 0.9) on average (one frame: the softmax is the constant 1)."""
    batch = 2
    for cc, rr, h in fm.OP_HEADS:
        z = fm.make_z(batch, tokens, cc, rr, h)
        for rope in (True, False):
            ref, w = fm.matrix_attention_ref(z, batch, tokens, fm.OP_E, h, cc, rr, rope)
            peak = float(w.max(-1).values.mean())
            if tokens > 1:
                assert 0.05 < peak < 0.9, peak
            table = fm.rope_table(tokens, h // rr).cuda() if rope else None
            got = _run_op(z, batch, tokens, h, cc, rr, table).float().cpu()
            assert torch.isfinite(got).all()
            r = rel(got, ref)
            print(f"matrix attention L={tokens} (cc, rr, h)={(cc, rr, h)} rope={rope}: rel-L2 {r:.2e} (mean largest probability {peak:.2f})")
            assert r < OP_BAR


def test_matrix_attention_rope_uses_the_first_rows_of_a_longer_table():
    """a shorter input under a larger max_tokens: the table has 32 rows, the call uses 5"""
    cc, rr, h = fm.OP_HEADS[2]
    z = fm.make_z(2, 5, cc, rr, h)
    long = _run_op(z, 2, 5, h, cc, rr, fm.rope_table(32, h // rr).cuda())
    exact = _run_op(z, 2, 5, h, cc, rr, fm.rope_table(5, h // rr).cuda())
    assert torch.equal(long, exact)


@pytest.mark.parametrize("tokens", [2, 10])
def test_null_table_agrees_with_the_variant1_kernel(tokens):
    """no rotation: the same z through the DifferenceDiT3D kernel; both round fp32 results to bf16, same bar as against fp64"""
    for cc, rr, h in fm.OP_HEADS:
        z = fm.make_z(2, tokens, cc, rr, h)
        new = _run_op(z, 2, tokens, h, cc, rr, None).float().cpu()
        old = _run_variant1_op(z, 2, tokens, h, cc, rr).float().cpu()
        r = rel(new, old)
        print(f"L={tokens} (cc, rr, h)={(cc, rr, h)}: new kernel vs matrix_attn_kernel rel-L2 {r:.2e}")
        assert r < OP_BAR


def test_matrix_attention_batch_rows_are_independent():
    """the second video alone gives the bits it gives in a batch of two (fixed summation order, no atomics)"""
    cc, rr, h = fm.OP_HEADS[1]
    for tokens in (5, 17):
        z = fm.make_z(2, tokens, cc, rr, h)
        table = fm.rope_table(tokens, h // rr).cuda()
        both = _run_op(z, 2, tokens, h, cc, rr, table)
        alone = _run_op(z[tokens * fm.OP_E:], 1, tokens, h, cc, rr, table)
        assert torch.equal(both[tokens * fm.OP_E:], alone)


def test_matrix_attention_invalid_shapes_launch_nothing():
    from dfot_amd import capi
    z = torch.zeros(2 * 33 * 64 * 3 * 128, dtype=torch.bfloat16, device="cuda")
    o = torch.full((2 * 33 * 64 * 128,), 7.0, dtype=torch.bfloat16, device="cuda")
    table = fm.rope_table(32, 32).cuda()

    def call(batch, tokens, e, h, cc, rr, zz=z, oo=o):
        return capi.lib.dfot_op_matrix_attention_rope(capi.ptr(zz), capi.ptr(oo), capi.ptr(table), batch, tokens, e, h, cc, rr, 0.01,
                                                      capi.stream_ptr())
    #            batch L  E   h    cc rr
    for args in ((2, 0, 64, 128, 1, 4), (2, 33, 64, 128, 1, 4), (2, -1, 64, 128, 1, 4), (2, 4, 64, 128, 3, 4), (2, 4, 64, 128, 1, 3),
                 (2, 4, 64, 120, 1, 20), (0, 4, 64, 128, 1, 4), (2, 4, 0, 128, 1, 4), (2, 4, 64, 128, 0, 4), (2, 4, 64, 128, 1, 0)):
        assert call(*args) == capi.ERR_SHAPE, args
        assert capi.lib.dfot_last_error()
    assert capi.lib.dfot_op_matrix_attention_rope(None, capi.ptr(o), None, 2, 4, 64, 128, 1, 4, 0.01, capi.stream_ptr()) == capi.ERR_ARG
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())  # nothing was launched: the output buffer is untouched
    assert call(2, 4, 64, 128, 1, 4) == capi.OK
    torch.cuda.synchronize()
    assert bool((o[: 2 * 4 * 64 * 128] == 0).all()) and bool((o[2 * 4 * 64 * 128:] == 7.0).all())  # v = 0 -> o = 0, and nothing past the end


# ---------------------------------------------------------------------------------------------------------------- the forward
@pytest.fixture(scope="module")
def g():
    return fm.load("dit_facmat.npz")


@pytest.mark.parametrize("tag", list(fm.CASES))
def test_forward_vs_reference_fixture(g, tag):
    model, params = fm.build(tag)
    assert fm.digest(params) == str(g[f"digest_{tag}"])
    assert list(model.state_dict().keys()) == [str(n) for n in g[f"names_{tag}"]]
    x, k = T(g["x"]).cuda(), T(g["k"]).cuda()
    with torch.no_grad():
        o5 = model(x, k).cpu()
        o3 = model(x[:, :3].contiguous(), k[:, :3].contiguous()).cpu()  # T = 3 (odd) under max_tokens 5: the first rows of the RoPE table
    r5, r3 = rel(o5, T(g[f"out_{tag}_t5"])), rel(o3, T(g[f"out_{tag}_t3"]))
    print(f"FacMatDiT {tag} {fm.CASES[tag]}: rel-L2 vs the reference T=5 {r5:.3e}, T=3 {r3:.3e}")
    assert r5 < FIXTURE_BAR and r3 < FIXTURE_BAR


def test_frames_are_coupled_as_in_the_reference(g):
    """frame 4 alone perturbed: frames 0-3 of the output move as they do in the reference (sens_frame4, > 2x the parity bar)"""
    model, _ = fm.build("a")
    k = T(g["k"]).cuda()
    with torch.no_grad():
        o5, o4 = model(T(g["x"]).cuda(), k).cpu(), model(T(g["x_frame4"]).cuda(), k).cpu()
    assert rel(o4, T(g["out_a_frame4"])) < FIXTURE_BAR
    moved, want = rel(o4[:, :4], o5[:, :4]), float(g["sens_frame4"])
    print(f"frames 0-3 move by {moved:.3e} (reference {want:.3e})")
    assert want > 2 * FIXTURE_BAR
    assert abs(moved - want) < FIXTURE_BAR and moved > 2 * FIXTURE_BAR


def test_conditioned_forward_vs_reference_fixture(g):
    model, params = fm.build("a", cond=True)
    assert fm.digest(params) == str(g["digest_act"])
    assert list(model.state_dict().keys()) == [str(n) for n in g["names_act"]]
    x, k, cond, mask = T(g["x"]).cuda(), T(g["k"]).cuda(), T(g["act_cond"]).cuda(), T(g["act_mask"]).cuda()
    with torch.no_grad():
        oa, om = model(x, k, cond).cpu(), model(x, k, cond, mask).cpu()
    ra, rm = rel(oa, T(g["out_act"])), rel(om, T(g["out_act_masked"]))
    print(f"FacMatDiT, action-conditioned: rel-L2 {ra:.3e}, with the per-video mask {rm:.3e}")
    assert ra < FIXTURE_BAR and rm < FIXTURE_BAR
    assert rel(om[0], T(g["out_act_masked"])[0]) < FIXTURE_BAR  # the masked video on its own
    assert torch.equal(om[1], oa[1])  # the unmasked video is untouched by the other one's mask


def test_batch_invariance(g):
    model, _ = fm.build("b")
    x, k = T(g["x"]).cuda(), T(g["k"]).cuda()
    with torch.no_grad():
        both = model(x, k)
        alone = model(x[1:2].contiguous(), k[1:2].contiguous())
    assert torch.equal(both[1:2], alone)


def test_load_state_dict_is_strict_and_training_is_refused(g):
    import dfot_amd
    model, params = fm.build("a")
    with pytest.raises(RuntimeError):
        model.load_state_dict({n: t for n, t in params.items() if "temporal_blocks.1.attn.qkv_u" not in n}, strict=True)
    x = T(g["x"]).cuda().requires_grad_()
    with pytest.raises(NotImplementedError, match="inference only"):
        model(x, T(g["k"]).cuda())
    for p in model.parameters():
        p.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="inference only"):
        model(T(g["x"]).cuda(), T(g["k"]).cuda())
    c = dfot_amd.capi.DiTConfig()
    for f, _ in c._fields_:
        setattr(c, f, getattr(model._ccfg, f))
    handle = dfot_amd.capi.C.c_void_p()
    assert dfot_amd.capi.lib.dfot_dit_train_create(dfot_amd.capi.C.byref(c), dfot_amd.capi.C.byref(handle)) == dfot_amd.capi.ERR_ARG
    assert b"variant 3" in dfot_amd.capi.lib.dfot_last_error()


def test_attn_timing_counts_as_for_the_difference_model(g):
    """the option times the spatial attention launches of every depth, as it does for variant 1 (the matrix attention is a separate kernel
    that neither variant brackets)"""
    model, _ = fm.build("a")
    model.sync_weights()
    model.set_option("time_attn", 16)
    with torch.no_grad():
        model(T(g["x"]).cuda(), T(g["k"]).cuda())
    total, launches = model.attn_timing()
    model.set_option("time_attn", 0)
    assert launches == 2 and total > 0


# ---------------------------------------------------------------------------------------------------------------- the sampler
def _sampler(model, noise_fn=None, steps=3):
    import dfot_amd
    cfg = dfot_amd.SamplerConfig(x_shape=(4, 16, 8), max_tokens=5,
                                 diffusion=dfot_amd.DiffusionConfig(sampling_timesteps=steps, beta_schedule="cosine", is_continuous=False),
                                 prediction_guidance=dict(name="vanilla", guidance_scale=1.5))
    return dfot_amd.DFoTVideoSampler(cfg, model, noise_fn)


def test_sampler_trace_vs_reference_fixture(g):
    model, _ = fm.build("a")
    nfn = ReplayList([T(g[f"run_noise{i}"]) for i in range(int(g["run_n_noise"]))])
    out = _sampler(model, nfn)._predict_videos(T(g["run_vid"]).cuda(), n_context_tokens=2, conditions=None).cpu()
    assert not nfn.queue
    ref = T(g["run_pred"])
    p = psnr(out, ref)
    print(f"FacMatDiT sampler: PSNR vs the reference's run {p:.1f} dB")
    assert torch.equal(out[:, :2], ref[:, :2])  # context tokens pass through untouched
    assert p >= 35.0


def test_graph_step_loop_equals_eager(g):
    model, _ = fm.build("a")
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


# ---------------------------------------------------------------------------------------------------------------- recipe width
def test_s64_width_forward_vs_host_restatement():
    """The @FacMatDiT/S-64-1 width at the recipes' length: embed_row_dim 384, 6 spatial and 6 row heads (hd = 64, hn = 64), depth 2, 4x32x32
    latents with patch 2 (P = 256), T = 16 (the length the register forms of variant 1 do not cover), B = 1, against
    dit_facmat_common.forward_host run on the GPU in fp32.  Bar: rel-L2 < 2e-2 on the output (tests/test_gpu_dit.py:150)."""
    import dfot_amd
    over = dict(hidden_size=384, depth=2, num_heads=6, patch_size=2, resolution=(32, 32), max_tokens=16)
    model = dfot_amd.DiT3D(fm.backbone_cfg(1, 6, False, 4.0, True, **over), x_shape=(4, 32, 32), max_tokens=16).cuda().eval()
    model.init_random(11)
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(1, 16, 4, 32, 32, generator=gen).cuda()
    k = torch.randint(0, 1000, (1, 16), generator=gen).cuda()
    with torch.no_grad():
        out = model(x, k)
        params = {n: t.detach() for n, t in model.state_dict().items()}
        ref = fm.forward_host(params, x, k, 1, 6, True, dtype=torch.float32, **over)
        plain = fm.forward_host(params, x, k, 1, 6, False, dtype=torch.float32, **over)
    assert torch.isfinite(out).all()
    r, effect = rel(out.cpu(), ref.cpu()), rel(plain.cpu(), ref.cpu())
    print(f"FacMatDiT S-64-1 width forward (1 x 16 x 256 tokens): rel-L2 vs the fp32 restatement {r:.3e}; the rotation moves the output by {effect:.3e}")
    assert r < 2e-2
