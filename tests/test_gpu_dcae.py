"""GPU: the DC-AE encoder and decoder (dfot_amd.dcae) on the two configurations of tests/golden/dcae.npz, against the fixture captured
from the reference's own Encoder / Decoder source (whose diffusers layers are stand-ins, unverified against the library:
tools/ref_loader.py) and against the fp32 restatement (tests/dcae_common.py) with the same weights; frame independence, strict
loading, the helper-level round trip, and one run at the stock dmlab widths.

Bars, those of tests/test_gpu_image_vae.py:5-6: rel-L2 < 2e-2 on reconstructions, <= 2e-2 on latents (bf16 GEMM operands, fp32
accumulation / streams / statistics).  Measured on an MI355X: see DESIGN.md (the DC-AE section)."""
import pytest
import torch

import dcae_common as dc

pytestmark = pytest.mark.gpu

G = dc.load()
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    """drop the cached modules and hand the cached device blocks back to the driver when this file is done, so that the test modules
    after it start from the allocator state they had without it"""
    yield
    _CACHE.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def setup(case):
    """(params, cfg, encoder, decoder, frames in [-1, 1], fixture latents, fixture reconstruction, restatement latents, restatement
    reconstruction), built once per case"""
    if case not in _CACHE:
        import dfot_amd
        p, cfg = dc.seeded_params(dc.key_shapes(G, case)), dc.config(dc.CASES[case])
        enc, dec = dfot_amd.DCAEEncoder(**cfg).cuda(), dfot_amd.DCAEDecoder(**cfg).cuda()
        assert enc.load_reference_state_dict(p) == [n for n in p if n.startswith("decoder.")]
        assert dec.load_reference_state_dict(p) == [n for n in p if n.startswith("encoder.")]
        x = 2.0 * (dc.T(G[f"y_{case}"]).float() / 255.0) - 1.0
        lat, rec = dc.T(G[f"latents_{case}"]), dc.T(G[f"recon_{case}"])
        with torch.no_grad():
            _CACHE[case] = (p, cfg, enc, dec, x, lat, rec, dc.encode(p, cfg, x), dc.decode(p, cfg, lat))
    return _CACHE[case]


@pytest.mark.parametrize("case", list(dc.CASES))
def test_encode_vs_fixture_and_restatement(case):
    _, _, enc, _, x, lat, _, rest, _ = setup(case)
    out = enc.encode(x.cuda()).cpu()
    r_fix, r_rest = dc.rel(out, lat), dc.rel(out, rest)
    print(f"DC-AE encode {case}: latents rel-L2 vs the reference fixture {r_fix:.3e}, vs the restatement {r_rest:.3e}, "
          f"max_abs {(out - lat).abs().max().item():.3e}")
    assert out.shape == lat.shape and torch.isfinite(out).all()
    assert r_fix <= 2e-2 and r_rest <= 2e-2


@pytest.mark.parametrize("case", list(dc.CASES))
def test_decode_vs_fixture_and_restatement(case):
    _, _, _, dec, _, lat, rec, _, rest = setup(case)
    out = dec.decode(lat.cuda()).cpu()
    r_fix, r_rest = dc.rel(out, rec), dc.rel(out, rest)
    print(f"DC-AE decode {case}: reconstruction rel-L2 vs the reference fixture {r_fix:.3e}, vs the restatement {r_rest:.3e}, "
          f"max_abs {(out - rec).abs().max().item():.3e}")
    assert out.shape == rec.shape and torch.isfinite(out).all()
    assert r_fix < 2e-2 and r_rest < 2e-2


@pytest.mark.parametrize("case", list(dc.CASES))
def test_frames_are_independent_bit_for_bit(case):
    """3 frames (padded to 4 inside) against 1 + 2 (padded to 2 + 2), and against the batch repeated: other tile counts, same bits"""
    _, _, enc, dec, x, lat, _, _, _ = setup(case)
    xd, zd = x.cuda(), lat.cuda()
    whole_e, whole_d = enc.encode(xd), dec.decode(zd)
    assert torch.equal(whole_e, torch.cat([enc.encode(xd[:1]), enc.encode(xd[1:])], 0))
    assert torch.equal(whole_d, torch.cat([dec.decode(zd[:1]), dec.decode(zd[1:])], 0))
    assert torch.equal(dec.decode(torch.cat([zd, zd, zd[:2]], 0))[3:6], whole_d)
    assert torch.equal(enc.encode(torch.cat([xd, xd, xd[:2]], 0))[3:6], whole_e)


def test_strict_loading_and_ignored_keys():
    import dfot_amd
    p, cfg, _, dec, _, lat, *_ = setup("f8")
    fresh = dfot_amd.DCAEDecoder(**cfg).cuda()
    assert fresh.load_reference_state_dict({"vae." + n: t for n, t in p.items()}) == ["vae." + n for n in p if n.startswith("encoder.")]
    assert torch.equal(fresh.decode(lat.cuda()), dec.decode(lat.cuda()))
    name = next(n for n in p if n.endswith("running_mean"))
    with pytest.raises(ValueError, match="keys not found"):
        fresh.load_reference_state_dict({n: t for n, t in p.items() if n != name})
    # the packed operands follow the weights: a changed BatchNorm statistic changes the result
    with torch.no_grad():
        fresh.state_dict()[name].add_(1.0)
    assert not torch.equal(fresh.decode(lat.cuda()), dec.decode(lat.cuda()))


def test_helper_round_trip_layout_and_chunking():
    import dfot_amd
    p, cfg, enc, dec, x, lat, rec, _, _ = setup("f8")
    videos = (0.5 * x + 0.5).reshape(1, 3, 3, 64, 64).repeat(3, 1, 1, 1, 1).cuda()       # b t c h w, 3 videos: chunks of 2 + 1
    videos[1] = videos[1].flip(0)
    z = dfot_amd.encode_dcae_frames(enc, videos, vae_batch_size=2)
    assert z.shape == (3, 3, 32, 8, 8)
    assert dc.rel(z[0].cpu(), lat) <= 2e-2 and dc.rel(z[1].cpu(), lat.flip(0)) <= 2e-2
    assert torch.equal(z, dfot_amd.encode_dcae_frames(enc, videos, vae_batch_size=1))
    assert torch.equal(z, dfot_amd.encode_dcae_frames(enc, videos, vae_batch_size=8))
    assert torch.equal(z[0], enc.encode(x.cuda()))                                       # 2 y - 1 fused into the pixel pack: the same bits
    zin = lat.reshape(1, 3, 32, 8, 8).repeat(3, 1, 1, 1, 1).cuda()
    y = dfot_amd.decode_dcae_latents(dec, zin, vae_batch_size=2)
    assert y.shape == (3, 3, 3, 64, 64)
    assert dc.rel(y[2].cpu(), rec * 0.5 + 0.5) < 2e-2
    assert torch.equal(y, dfot_amd.decode_dcae_latents(dec, zin, vae_batch_size=1))
    # a non-contiguous view (t b c h w transposed) addresses the same frames
    vt = videos.transpose(0, 1).contiguous().transpose(0, 1)
    assert torch.equal(z, dfot_amd.encode_dcae_frames(enc, vt, vae_batch_size=2))


def test_stock_dmlab_widths():
    """channels [128, 256, 512, 512] with 2 layers per stage, 2 frames at 64^2: the only place 512-channel 16-head attention, the K = 2048
    conv_point GEMM and the shortcut group sizes 16 / 2 run.  Reference: the fp32 restatement."""
    import dfot_amd
    cfg = dc.config(dc.STOCK)
    enc, dec = dfot_amd.DCAEEncoder(**cfg), dfot_amd.DCAEDecoder(**cfg)
    shapes = {n: tuple(t.shape) for m in (enc, dec) for n, t in m.state_dict().items()}
    p = dc.seeded_params(shapes)
    enc.load_reference_state_dict(p)
    dec.load_reference_state_dict(p)
    enc, dec = enc.cuda(), dec.cuda()
    g = torch.Generator().manual_seed(12)
    x = 2.0 * torch.rand(2, 3, 64, 64, generator=g) - 1.0
    with torch.no_grad():
        lat = dc.encode(p, cfg, x)
        rec = dc.decode(p, cfg, lat)
    z, y = enc.encode(x.cuda()).cpu(), dec.decode(lat.cuda()).cpu()
    r_lat, r_rec = dc.rel(z, lat), dc.rel(y, rec)
    print(f"DC-AE stock dmlab widths: latents rel-L2 {r_lat:.3e}, reconstruction rel-L2 {r_rec:.3e}")
    assert z.shape == (2, 32, 8, 8) and y.shape == (2, 3, 64, 64) and torch.isfinite(z).all() and torch.isfinite(y).all()
    assert r_lat <= 2e-2 and r_rec < 2e-2
    assert torch.equal(dec.decode(lat[1:].cuda()).cpu(), y[1:])       # the split-K decision does not depend on the batch
