"""GPU: the ImageVAE decoder and encoder (dfot_amd.image_vae) with a mid attention over 32 x 32 = 1024 positions per frame.

  * case "c" of tests/golden/image_vae_1024.npz, captured from the reference's own Encoder / Decoder source, and the fp32 restatement
    (tests/image_vae_common.py) with the same weights.  Bars: rel-L2 < 2e-2 on decoded frames and <= 2e-2 on the latent moments, the
    bars of tests/test_gpu_image_vae.py.  The fixture sees the attention: a uniform average in its place moves the frames by 0.18 and
    the moments by 0.081 (stored in the file).
  * the KL-f8 recipe's own size: ch 128, ch_mult (1, 2, 4, 4), 2 res blocks, one 256 x 256 frame, seeded weights, against the fp32
    restatement evaluated with torch on the same GPU.  Bar 2e-2; a result above it is held to max(2e-2, 1.5 x the error of the SAME
    restatement under bf16 autocast against its fp32 evaluation): 1.5 for the different rounding points of two bf16 paths.
  * a decoder loaded from the diffusers layout decodes to the bits of one loaded from the reference layout; the vae.batch_size helper.
"""
import pytest
import torch

import image_vae_1024_common as c1k

pytestmark = pytest.mark.gpu

G = c1k.load()
_CACHE = {}


def setup():
    """(params, decoder, encoder, restatement frames, restatement moments) of case "c", built once"""
    if not _CACHE:
        import dfot_amd
        p = c1k.seeded_params(G)
        dec, enc = dfot_amd.ImageVAEDecoder(**c1k.CFG_C).cuda(), dfot_amd.ImageVAEEncoder(**c1k.CFG_C).cuda()
        dec.load_reference_state_dict(p)
        enc.load_reference_state_dict(p)
        with torch.no_grad():
            frames = c1k.decode(p, c1k.CFG_C, c1k.T(G["z_c"]))
            moments = c1k.encode(p, c1k.CFG_C, 2.0 * c1k.T(G["y_c"]) - 1.0)
        _CACHE["c"] = (p, dec, enc, frames, moments)
    return _CACHE["c"]


def test_fixture_sees_the_attention():
    assert float(G["uniform_attention_frames"]) >= 4e-2 and float(G["uniform_attention_moments"]) >= 4e-2


def test_decode_vs_fixture_and_restatement():
    p, dec, _, rest, _ = setup()
    out = dec.decode(c1k.T(G["z_c"]).cuda()).cpu()
    ref = c1k.T(G["frames_c"])
    r_fix, r_rest = c1k.rel(out, ref), c1k.rel(out, rest)
    print(f"ImageVAE decode c (N = 1024): rel-L2 vs the reference fixture {r_fix:.3e}, vs the restatement {r_rest:.3e}")
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert r_fix < 2e-2 and r_rest < 2e-2


def test_encode_vs_fixture_and_restatement():
    p, _, enc, _, rest = setup()
    mom = enc.encode((2.0 * c1k.T(G["y_c"]) - 1.0).cuda()).parameters.cpu()
    ref = c1k.T(G["moments_c"])
    r_fix, r_rest = c1k.rel(mom, ref), c1k.rel(mom, rest)
    print(f"ImageVAE encode c (N = 1024): moments rel-L2 vs the reference fixture {r_fix:.3e}, vs the restatement {r_rest:.3e}")
    assert mom.shape == ref.shape and torch.isfinite(mom).all()
    assert r_fix <= 2e-2 and r_rest <= 2e-2


def test_frames_are_independent_bit_for_bit():
    p, dec, enc, _, _ = setup()
    z = c1k.T(G["z_c"]).cuda()
    assert torch.equal(dec.decode(z), torch.cat([dec.decode(z[:1]), dec.decode(z[1:])], 0))
    x = (2.0 * c1k.T(G["y_c"]) - 1.0).cuda()
    assert torch.equal(enc.encode(x).parameters, torch.cat([enc.encode(x[:1]).parameters, enc.encode(x[1:]).parameters], 0))


def test_diffusers_layout_loads_to_the_same_bits_and_the_helper_decodes():
    import dfot_amd
    p, dec, _, _, _ = setup()
    z = c1k.T(G["z_c"]).cuda()
    first = dec.decode(z)
    for legacy in (False, True):
        other = dfot_amd.ImageVAEDecoder(**c1k.CFG_C).cuda()
        ignored = other.load_diffusers_state_dict(c1k.to_diffusers(p, 2, legacy))
        assert ignored == [n for n in p if n.startswith(("encoder.", "quant_conv."))]
        assert torch.equal(other.decode(z), first)
    lat = z.reshape(1, 2, 4, 32, 32)
    vid = dfot_amd.decode_image_latents(dec, lat, vae_batch_size=1)
    assert vid.shape == (1, 2, 3, 64, 64)
    assert torch.equal(vid.reshape(2, 3, 64, 64), first * 0.5 + 0.5)
    assert c1k.rel(vid.cpu().reshape(2, 3, 64, 64), c1k.T(G["frames_c"]) * 0.5 + 0.5) < 2e-2


def test_recipe_size_256x256_vs_the_restatement_on_the_gpu():
    """Measured on an MI355X (DESIGN.md section 4g''): decode 1.01e-2, encode 1.01e-2 against the fp32 restatement, under the 2e-2 bar;
    the restatement under bf16 autocast is 1.69e-2 / 1.64e-2 from its fp32 evaluation (printed for the record, not needed as a bar)."""
    import dfot_amd
    cfg = c1k.RECIPE
    p = c1k.seeded_recipe_params(cfg)
    dec, enc = dfot_amd.ImageVAEDecoder(**cfg).cuda(), dfot_amd.ImageVAEEncoder(**cfg).cuda()
    dec.load_reference_state_dict(p)
    enc.load_reference_state_dict(p)
    pg = {n: t.cuda() for n, t in p.items()}
    g = torch.Generator().manual_seed(43)
    z = torch.randn(1, 4, 32, 32, generator=g).cuda()
    x = (2.0 * torch.rand(1, 3, 256, 256, generator=g) - 1.0).cuda()
    with torch.no_grad():
        ref_frames, ref_mom = c1k.decode(pg, cfg, z), c1k.encode(pg, cfg, x)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ac_frames, ac_mom = c1k.decode(pg, cfg, z).float(), c1k.encode(pg, cfg, x).float()
    out, mom = dec.decode(z), enc.encode(x).parameters
    assert out.shape == (1, 3, 256, 256) and mom.shape == (1, 8, 32, 32)
    assert torch.isfinite(out).all() and torch.isfinite(mom).all()
    for what, got, ref, ac in (("decode", out, ref_frames, ac_frames), ("encode", mom, ref_mom, ac_mom)):
        r, r_ac = c1k.rel(got, ref), c1k.rel(ac, ref)
        bar = 2e-2 if r <= 2e-2 else max(2e-2, 1.5 * r_ac)
        print(f"ImageVAE {what} at 256x256, ch_mult (1, 2, 4, 4) x 2 res blocks: engine rel-L2 vs the fp32 restatement {r:.3e}; the "
              f"restatement under bf16 autocast vs fp32 {r_ac:.3e}; bar {bar:.3e}")
        assert r <= bar
