"""GPU: the ImageVAE decoder and encoder (dfot_amd.image_vae) on the two configurations of tests/golden/image_vae.npz, against the
fixture captured from the reference's own Encoder / Decoder source and against the fp32 restatement (tests/image_vae_common.py) with the
same weights; frame independence, strict loading, and the helper-level round trip.

Bars: rel-L2 < 2e-2 on decoded frames (what tests/test_gpu_vae.py:94 holds the VideoVAE decoder to) and rel-L2 <= 2e-2 on the latent
moments (tests/test_gpu_vae_encode.py:157): bf16 GEMM operands, fp32 accumulation / streams / statistics."""
import pytest
import torch

import image_vae_common as ivc

pytestmark = pytest.mark.gpu

G = ivc.load()
_CACHE = {}


def setup(case):
    """(params, cfg, decoder, encoder, restatement frames, restatement moments), built once per case"""
    if case not in _CACHE:
        import dfot_amd
        p, cfg = ivc.seeded_params(G, case), ivc.ddconfig(case)
        dec, enc = dfot_amd.ImageVAEDecoder(**cfg).cuda(), dfot_amd.ImageVAEEncoder(**cfg).cuda()
        assert dec.load_reference_state_dict(p) == [n for n in p if n.startswith(("encoder.", "quant_conv."))]
        assert enc.load_reference_state_dict(p) == [n for n in p if n.startswith(("decoder.", "post_quant_conv."))]
        with torch.no_grad():
            frames = ivc.decode(p, cfg, ivc.T(G[f"z_{case}"]))
            moments = ivc.encode(p, cfg, 2.0 * ivc.T(G[f"y_{case}"]) - 1.0)
        _CACHE[case] = (p, cfg, dec, enc, frames, moments)
    return _CACHE[case]


@pytest.mark.parametrize("case", ["a", "b"])
def test_decode_vs_fixture_and_restatement(case):
    p, cfg, dec, _, rest, _ = setup(case)
    out = dec.decode(ivc.T(G[f"z_{case}"]).cuda()).cpu()
    ref = ivc.T(G[f"frames_{case}"])
    r_fix, r_rest = ivc.rel(out, ref), ivc.rel(out, rest)
    print(f"ImageVAE decode {case}: rel-L2 vs the reference fixture {r_fix:.3e}, vs the restatement {r_rest:.3e}, "
          f"max_abs {(out - ref).abs().max().item():.3e}")
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert r_fix < 2e-2 and r_rest < 2e-2


@pytest.mark.parametrize("case", ["a", "b"])
def test_encode_vs_fixture_and_restatement(case):
    p, cfg, _, enc, _, rest = setup(case)
    y = ivc.T(G[f"y_{case}"])
    post = enc.encode((2.0 * y - 1.0).cuda())
    mom = post.parameters.cpu()
    ref = ivc.T(G[f"moments_{case}"])
    r_fix, r_rest = ivc.rel(mom, ref), ivc.rel(mom, rest)
    print(f"ImageVAE encode {case}: moments rel-L2 vs the reference fixture {r_fix:.3e}, vs the restatement {r_rest:.3e}")
    assert mom.shape == ref.shape and torch.isfinite(mom).all()
    assert r_fix <= 2e-2 and r_rest <= 2e-2
    mean, logvar, std = ivc.posterior(ref)
    assert ivc.rel(post.mean.cpu(), mean) <= 2e-2 and torch.equal(post.mode(), post.mean)
    assert ivc.rel(post.std, torch.exp(0.5 * post.logvar)) <= 1e-6
    eps = torch.randn(mean.shape, generator=torch.Generator().manual_seed(3))
    smp = post.sample(noise=eps).cpu()
    assert smp.shape == mean.shape and ivc.rel(smp, mean + std * eps) <= 2e-2
    with pytest.raises(ValueError, match="noise has shape"):
        post.sample(noise=eps[:1])


def test_frames_are_independent_bit_for_bit():
    p, cfg, dec, enc, _, _ = setup("a")
    z = ivc.T(G["z_a"]).cuda()
    whole = dec.decode(z)
    assert torch.equal(whole, torch.cat([dec.decode(z[:2]), dec.decode(z[2:])], 0))
    x = (2.0 * ivc.T(G["y_a"]) - 1.0).cuda()
    mom = enc.encode(x).parameters
    assert torch.equal(mom, torch.cat([enc.encode(x[:2]).parameters, enc.encode(x[2:]).parameters], 0))
    # the vae.batch_size helpers: 2 videos x 2 frames in one chunk == one video per chunk
    import dfot_amd
    lat = z.reshape(2, 2, *z.shape[1:])
    assert torch.equal(dfot_amd.decode_image_latents(dec, lat, vae_batch_size=2), dfot_amd.decode_image_latents(dec, lat, vae_batch_size=1))
    vid = ivc.T(G["y_a"]).cuda().reshape(2, 2, 3, 16, 16)
    eps = torch.randn(2, 2, 4, 8, 8, generator=torch.Generator().manual_seed(4)).cuda()
    one = dfot_amd.encode_image_frames(enc, vid, vae_batch_size=2, noise=eps)
    assert torch.equal(one, dfot_amd.encode_image_frames(enc, vid, vae_batch_size=1, noise=eps))
    with pytest.raises(ValueError, match="2 frames would work"):
        dec.decode(z[:1])                                        # 64 GEMM rows: refused before any launch


def test_strict_loading_and_repacking():
    import dfot_amd
    p, cfg, _, _, _, _ = setup("a")
    dec = dfot_amd.ImageVAEDecoder(**cfg).cuda()
    own = {n: t for n, t in p.items() if n.startswith(("decoder.", "post_quant_conv."))}
    assert dec.load_reference_state_dict(own) == []
    z = ivc.T(G["z_a"]).cuda()
    first = dec.decode(z)
    ignored = dec.load_reference_state_dict({"vae." + n: t for n, t in p.items()})          # Lightning-style prefix
    assert ignored == ["vae." + n for n in p if n not in own]
    assert torch.equal(dec.decode(z), first)
    with pytest.raises(ValueError, match="keys not found"):
        dec.load_reference_state_dict({n: t for n, t in own.items() if n != "decoder.mid.attn_1.q.weight"})
    with pytest.raises(ValueError, match="size mismatch"):
        dec.load_reference_state_dict({**own, "decoder.conv_in.bias": torch.zeros(3)})
    with torch.no_grad():
        dict(dec.named_parameters())["decoder.up.1.upsample.conv.weight"].mul_(1.5)       # _version moves: the packed copy follows
    changed = dec.decode(z)
    assert not torch.equal(changed, first)
    p2 = dict(p)
    p2["decoder.up.1.upsample.conv.weight"] = p["decoder.up.1.upsample.conv.weight"] * 1.5
    with torch.no_grad():
        assert ivc.rel(changed.cpu(), ivc.decode(p2, cfg, ivc.T(G["z_a"]))) < 2e-2


def test_helper_round_trip_vs_restatement():
    import dfot_amd
    p, cfg, dec, enc, _, _ = setup("a")
    vid = ivc.T(G["y_a"]).reshape(2, 2, 3, 16, 16)
    eps = torch.randn(2, 2, 4, 8, 8, generator=torch.Generator().manual_seed(6))
    lat = dfot_amd.encode_image_frames(enc, vid.cuda(), vae_batch_size=1, noise=eps.cuda())
    out = dfot_amd.decode_image_latents(dec, lat, vae_batch_size=1)
    with torch.no_grad():
        lat_ref = ivc.encode_frames(p, cfg, vid, eps)
        out_ref = ivc.decode_latents(p, cfg, lat_ref)
    assert lat.shape == (2, 2, 4, 8, 8) and out.shape == vid.shape
    r_lat, r_out = ivc.rel(lat.cpu(), lat_ref), ivc.rel(out.cpu(), out_ref)
    print(f"ImageVAE helpers: latents rel-L2 {r_lat:.3e}, round-trip frames rel-L2 {r_out:.3e} vs the restatement")
    assert r_lat <= 2e-2 and r_out < 2e-2
    # "* 0.5 + 0.5" is applied: the helper's frames are the decoder's output of the same latents, shifted into [0, 1]
    raw = dec.decode(lat.reshape(4, 4, 8, 8))
    assert torch.equal(out.reshape(4, 3, 16, 16), raw * 0.5 + 0.5)
    # mode (no sampling) and the latent normalisation of _normalize_x
    mode = dfot_amd.encode_image_frames(enc, vid.cuda(), sample=False)
    mean, std = [0.1, -0.2, 0.3, 0.0], [1.5, 0.5, 2.0, 1.0]
    normed = dfot_amd.encode_image_frames(enc, vid.cuda(), sample=False, data_mean=mean, data_std=std)
    want = (mode - torch.tensor(mean, device="cuda").view(1, 1, 4, 1, 1)) / torch.tensor(std, device="cuda").view(1, 1, 4, 1, 1)
    assert ivc.rel(normed, want) <= 1e-6
