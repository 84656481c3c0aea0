"""GPU: the TiTok-KL encoder (dfot_amd.titok.TiTokEncoder) on the three configurations of tests/golden/titok_enc.npz, against the fixture
captured from the reference's own TiTok_KL source in fp32 (never against the engine itself), plus the posterior, frame independence, row
padding, repacking and the helper-level encode.

Bar: moments rel-L2 < bar(case) = 2 x rel_autocast_moments_<case>, the error the reference itself has under
torch.autocast("cpu", bfloat16) against its fp32 run (3.0e-2 / 3.8e-2 / 1.6e-2, stored in the fixture); the factor of two covers a
different rounding order, not a wrong term (the convention of tests/test_gpu_titok.py).  The fixture's own guards (tests/test_titok_enc_host.py)
show that another image, or the transposing reading of the reference's reshape, moves the moments by more than 5 x that bar.
Achieved values are printed by every test."""
import pytest
import torch

import titok_enc_common as te

pytestmark = pytest.mark.gpu

G = te.load()
CASES = ["a", "b", "c"]
_CACHE = {}


def bar(case):
    return 2.0 * float(G[f"rel_autocast_moments_{case}"])


def setup(case):
    """(params, cfg, encoder on the GPU, the fixture's frames on the GPU), built once per case"""
    if case not in _CACHE:
        import dfot_amd
        p, cfg = te.seeded_params(G, case), te.config(case)
        enc = dfot_amd.TiTokEncoder(**cfg).cuda()
        assert enc.load_reference_state_dict(p) == []
        _CACHE[case] = (p, cfg, enc, te.inputs(G, case).cuda())
    return _CACHE[case]


@pytest.mark.parametrize("case", CASES)
def test_moments_vs_reference_fixture(case):
    _, _, enc, x = setup(case)
    out = enc.encode_moments(x).cpu()
    ref = te.T(G[f"moments_{case}"])
    r = te.rel(out, ref)
    print(f"TiTok encode {case}: moments rel-L2 vs the reference fixture {r:.3e} (bar {bar(case):.3e}), max_abs {(out - ref).abs().max().item():.3e}")
    assert out.shape == ref.shape and out.dtype == torch.float32 and torch.isfinite(out).all()
    assert r < bar(case)
    other = te.rel(enc.encode_moments(te.inputs(G, case, "x2").cuda()).cpu(), te.T(G[f"moments2_{case}"]))
    print(f"TiTok encode {case}: moments of the second input rel-L2 {other:.3e}")
    assert other < bar(case)


def test_posterior_mode_and_sample():
    _, _, enc, x = setup("a")
    mom = enc.encode_moments(x)
    post = enc.encode(x)
    assert torch.equal(enc.encode(x, sample=True), mom[:, :4])                   # sample=True is the MODE, bit for bit
    assert torch.equal(post.mode(), mom[:, :4]) and torch.equal(post.mean, mom[:, :4]) and torch.equal(post.parameters, mom)
    assert post.mean.shape == post.logvar.shape == post.std.shape == (3, 4, 1, 32)
    assert torch.equal(post.logvar, mom[:, 4:].clamp(-30.0, 20.0))
    assert te.rel(post.std.cpu(), torch.exp(0.5 * post.logvar.cpu().double())) < 1e-6
    noise = torch.randn(3, 4, 1, 32, generator=torch.Generator().manual_seed(3))
    want = post.mean.cpu().double() + post.std.cpu().double() * noise.double()
    for z in (post.sample(noise.cuda()), enc.encode(x, sample=True, sample_posterior=True, noise=noise.cuda()), post.sample(noise)):
        assert z.shape == (3, 4, 1, 32) and (z.cpu().double() - want).abs().max().item() <= 1e-6 * want.abs().max().item()
    gen = torch.Generator(device="cuda").manual_seed(4)
    drawn = enc.encode(x, sample=True, sample_posterior=True, generator=gen)
    expect = torch.randn(3, 4, 1, 32, generator=torch.Generator(device="cuda").manual_seed(4), device="cuda")
    assert (drawn.cpu().double() - (post.mean.cpu().double() + post.std.cpu().double() * expect.cpu().double())).abs().max().item() <= 1e-6 * want.abs().max().item()
    for shape in ((3, 4, 32), (3, 8, 1, 32), (2, 4, 1, 32)):
        with pytest.raises(ValueError, match="noise has shape"):
            post.sample(torch.zeros(shape, device="cuda"))
        with pytest.raises(ValueError, match="noise has shape"):
            enc.encode(x, sample=True, sample_posterior=True, noise=torch.zeros(shape, device="cuda"))


def test_logvar_is_clamped():
    """conv_out's bias pushed to +-50 on the logvar channels: the raw moments keep it, the posterior clamps to [-30, 20]"""
    import dfot_amd
    p, cfg, _, x = setup("a")
    enc = dfot_amd.TiTokEncoder(**cfg).cuda()
    b = p["encoder.conv_out.bias"].clone()
    b[4:6], b[6:8] = 50.0, -50.0
    enc.load_reference_state_dict({**p, "encoder.conv_out.bias": b})
    mom, post = enc.encode_moments(x), enc.encode(x)
    assert mom[:, 4:6].min().item() > 20.0 and mom[:, 6:8].max().item() < -30.0
    assert torch.equal(post.parameters, mom)
    assert (post.logvar[:, 0:2] == 20.0).all() and (post.logvar[:, 2:4] == -30.0).all()
    assert torch.allclose(post.std[:, 0:2].cpu(), torch.full((3, 2, 1, 32), 10.0).exp(), rtol=1e-5)
    assert torch.allclose(post.std[:, 2:4].cpu(), torch.full((3, 2, 1, 32), -15.0).exp(), rtol=1e-5)


def test_frames_are_independent_bit_for_bit_and_any_count_runs():
    """49-token sequences: 1, 2 and 3 frames are 49, 98 and 147 token rows (padded to 128 / 128 / 256) and 16, 32, 48 patch rows (padded
    to 128).  A frame encodes to the same bits alone, in a batch of 3, and under vae_batch_size 1 against 2."""
    import dfot_amd
    _, _, enc, x = setup("a")
    whole = enc.encode_moments(x)
    assert whole.shape == (3, 8, 1, 32) and torch.isfinite(whole).all()
    for f in range(3):
        assert torch.equal(enc.encode_moments(x[f:f + 1]), whole[f:f + 1])
    assert torch.equal(enc.encode_moments(x[:2]), whole[:2]) and torch.equal(enc.encode_moments(x[1:]), whole[1:])
    vid = torch.stack([x, x.flip(0)], 0)[:, :2]                      # 2 videos x 2 frames
    one, two = (dfot_amd.encode_titok_frames(enc, vid, vae_batch_size=n) for n in (1, 2))
    assert one.shape == (2, 2, 4, 1, 32)
    assert torch.equal(one, two) and torch.equal(one[0], whole[:2, :4]) and torch.equal(one[1], whole[[2, 1]][:, :4])


def test_frames_are_independent_at_the_production_sequence():
    """289-token sequences (case c's module): 2 frames are 578 token rows, so the second sequence starts in the middle of a tile"""
    _, _, enc, x = setup("c")
    both = torch.cat([x, te.inputs(G, "c", "x2").cuda()], 0)
    out = enc.encode_moments(both)
    assert torch.equal(out[:1], enc.encode_moments(both[:1])) and torch.equal(out[1:], enc.encode_moments(both[1:]))
    assert te.rel(out[:1].cpu(), te.T(G["moments_c"])) < bar("c") and te.rel(out[1:].cpu(), te.T(G["moments2_c"])) < bar("c")


@pytest.mark.parametrize("name", ["latent_tokens", "encoder.patch_embed.weight", "encoder.transformer.2.attn.in_proj_weight",
                                  "encoder.conv_out.weight"])
def test_a_weight_changed_in_place_is_repacked(name):
    """whether the weight is read in fp32 as it stands (latent_tokens, conv_out) or through a packed bf16 operand (patch_embed, in_proj).
    The change is noise of half the weight's standard deviation, as in tests/test_gpu_titok.py: on the CPU restatement it moves the moments
    by 0.46 ... 0.76 (7.6 ... 12.5 x bar) while the reference's own bf16 autocast loss stays at the fixture's 3e-2 -- a larger change to
    in_proj sharpens the attention of that layer and with it every bf16 engine's error."""
    import dfot_amd
    p, cfg, _, x = setup("a")
    enc = dfot_amd.TiTokEncoder(**cfg).cuda()
    enc.load_reference_state_dict(p)
    before = enc.encode_moments(x).cpu()
    assert te.rel(before, te.T(G["moments_a"])) < bar("a")
    p2 = dict(p)
    p2[name] = p[name] + 0.5 * p[name].std() * torch.randn(p[name].shape, generator=torch.Generator().manual_seed(11))
    with torch.no_grad():
        enc.get_parameter(name).copy_(p2[name])
        ref = te.moments(p2, cfg, x.cpu())
    after = enc.encode_moments(x).cpu()
    r, moved = te.rel(after, ref), te.rel(ref, te.T(G["moments_a"]))
    print(f"TiTok encode a after an in-place change of {name}: rel-L2 vs the restatement {r:.3e}; the change moved the moments by {moved:.3e} "
          f"({moved / bar('a'):.1f} x bar)")
    assert moved > 5 * bar("a") and not torch.equal(before, after)
    assert r < bar("a")


def test_encode_titok_frames_matches_the_restatement():
    import dfot_amd
    p, cfg, enc, _ = setup("a")
    vid = torch.rand(2, 3, 3, 64, 64, generator=torch.Generator().manual_seed(12))
    out = dfot_amd.encode_titok_frames(enc, vid.cuda()).cpu()
    with torch.no_grad():
        ref = te.encode(p, cfg, vid.reshape(6, 3, 64, 64)).reshape(2, 3, 4, 1, 32)
    r = te.rel(out, ref)
    print(f"encode_titok_frames (2, 3, 3, 64, 64): rel-L2 vs the restatement {r:.3e}")
    assert out.shape == ref.shape == (2, 3, 4, 1, 32)
    assert r < bar("a")


def test_host_and_foreign_device_tensors_are_refused_before_any_launch():
    import dfot_amd
    _, cfg, enc, x = setup("a")
    for call in (enc.encode, enc.encode_moments, lambda t: dfot_amd.encode_titok_frames(enc, t[None])):
        with pytest.raises(ValueError, match="GPU only"):
            call(x.cpu())
    host = dfot_amd.TiTokEncoder(**cfg)                              # parameters still on the host
    with pytest.raises((RuntimeError, ValueError), match="cpu"):
        host.encode_moments(x)
    if torch.cuda.device_count() > 1:
        with pytest.raises((RuntimeError, ValueError), match="cuda:1"):
            enc.encode_moments(x.to("cuda:1"))
