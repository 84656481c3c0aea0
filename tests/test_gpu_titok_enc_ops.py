"""GPU: the three encoder ops of csrc/titok.hip, each against an fp64 torch computation of the same fp32 operands.

Bars (those of tests/test_gpu_titok_ops.py: from the number formats, not from these kernels):
  * fp32 outputs (token assembly, moments): 1e-5 relative (rel-L2, and per element against the row's largest magnitude);
  * the bf16 patch rows are a gather and one rounding to nearest even: BIT-equal to `F.unfold(x, 16, stride=16)` cast to bf16 (within one
    rounding, 2^-8 per element, would be the bar of a computed bf16 output; a copy has no excuse to differ)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")


@pytest.fixture(scope="module")
def capi():
    import dfot_amd  # noqa: F401
    from dfot_amd import capi as c
    assert torch.cuda.is_available()
    return c


def rel(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30)).item()


def pad128(n):
    return -(-n // 128) * 128


def f32_errors(name, got, ref):
    r = rel(got, ref)
    worst = ((got.double() - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-30)).max().item()
    print(f"{name}: fp32 rel-L2 {r:.3e}, worst element / row max {worst:.3e}")
    return r, worst


def check_f32(name, got, ref):
    r, worst = f32_errors(name, got, ref)
    assert torch.isfinite(got).all() and r < 1e-5 and worst < 1e-5


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("size", [16, 64, 128])
def test_patch_rows_vs_unfold(capi, size, frames):
    """one patch, 4 x 4 and 8 x 8 patches per frame; values out to +-10 with both signs, so round-to-nearest-even is exercised on every
    exponent in between.  The buffer is padded to whole GEMM tiles and NaN-filled: rows past frames * g^2 stay NaN."""
    g = torch.Generator().manual_seed(100 * size + frames)
    x = torch.randn(frames, 3, size, size, generator=g) * 3.0
    g2 = (size // 16) ** 2
    ref = F.unfold(x, 16, stride=16).transpose(1, 2).reshape(frames * g2, 768).to(BF)      # columns (c, dy, dx): patch_embed.weight's order
    xd = x.cuda()
    rows = torch.full((pad128(frames * g2), 768), NAN, dtype=BF, device="cuda")
    capi.check(capi.lib.dfot_op_titok_patch_rows(capi.ptr(xd), capi.ptr(rows), frames, size, capi.stream_ptr()))
    got = rows.cpu()
    assert torch.equal(got[: frames * g2].view(torch.int16), ref.view(torch.int16))
    assert torch.isnan(got[frames * g2:].float()).all()
    # the product against the reshaped convolution weight is the convolution
    w = torch.randn(8, 3, 16, 16, generator=g)
    conv = F.conv2d(x.to(BF).double(), w.double(), stride=16).reshape(frames, 8, g2).transpose(1, 2).reshape(frames * g2, 8)
    assert rel(got[: frames * g2].double() @ w.reshape(8, 768).double().T, conv) < 1e-12


def test_patch_rows_refuses_bad_shapes_before_any_launch(capi):
    x = torch.zeros(1, 3, 64, 64, device="cuda")
    rows = torch.full((128, 768), NAN, dtype=BF, device="cuda")
    for frames, size, word in ((1, 40, "image_size=40"), (1, 0, "image_size=0"), (1, -16, "image_size=-16"), (0, 64, "nframes=0")):
        rc = capi.lib.dfot_op_titok_patch_rows(capi.ptr(x), capi.ptr(rows), frames, size, capi.stream_ptr())
        assert rc == capi.ERR_SHAPE
        assert "op_titok_patch_rows" in capi.lib.dfot_last_error().decode() and word in capi.lib.dfot_last_error().decode()
    torch.cuda.synchronize()
    assert torch.isnan(rows.float()).all()                           # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------------------
def enc_tokens_operands(c, grid2, frames, pad, nlat=32):
    g = torch.Generator().manual_seed(c + 10 * grid2 + frames + pad)
    patches = torch.randn(frames * grid2, c, generator=g)
    cls, pos, lat, lpos = (torch.randn(s, generator=g) / math.sqrt(c) for s in ((1, c), (grid2 + 1, c), (nlat, c), (nlat, c)))
    gamma, beta = 1.0 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    front = torch.cat([cls.double().unsqueeze(0).expand(frames, -1, -1), patches.double().reshape(frames, grid2, c)], 1) + pos.double()[None]
    back = (lat.double() + lpos.double()).unsqueeze(0).expand(frames, -1, -1)
    ref = F.layer_norm(torch.cat([front, back], 1), (c,), gamma.double(), beta.double(), 1e-5).reshape(-1, c)
    wide = torch.cat([patches, torch.full((patches.shape[0], pad), NAN)], 1)               # columns >= C of a patch row are never read
    return [t.cuda().contiguous() for t in (wide, cls, pos, lat, lpos, gamma, beta)], ref


def run_enc_tokens(capi, dev, ldp, out, frames, grid2, nlat, c):
    return capi.lib.dfot_op_titok_enc_tokens(capi.ptr(dev[0]), ldp, *[capi.ptr(t) for t in dev[1:]], 1e-5, capi.ptr(out), frames, grid2, nlat, c,
                                             capi.stream_ptr())


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("grid2,c", [(1, 512), (16, 512), (64, 768), (256, 1024)])
def test_enc_tokens_vs_fp64(capi, grid2, c, frames, pad):
    dev, ref = enc_tokens_operands(c, grid2, frames, pad)
    rows = frames * (1 + grid2 + 32)
    out = torch.full((pad128(rows), c), NAN, device="cuda")
    capi.check(run_enc_tokens(capi, dev, c + pad, out, frames, grid2, 32, c))
    got = out.cpu()
    check_f32(f"encoder token assembly C {c} grid^2 {grid2} frames {frames} ldp {c + pad}", got[:rows], ref)
    assert torch.isnan(got[rows:]).all()                             # rows past the last sequence are not written


def test_enc_tokens_refuses_bad_shapes_before_any_launch(capi):
    dev, _ = enc_tokens_operands(512, 16, 1, 0)
    out = torch.full((128, 512), NAN, device="cuda")
    for ldp, c, word in ((512, 640, "channels=640"), (508, 512, "ldp=508"), (514, 512, "ldp=514")):
        rc = run_enc_tokens(capi, dev, ldp, out, 1, 16, 32, c)
        assert rc == capi.ERR_SHAPE
        assert "op_titok_enc_tokens" in capi.lib.dfot_last_error().decode() and word in capi.lib.dfot_last_error().decode()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("oc", [8, 24])
@pytest.mark.parametrize("c", [512, 768, 1024])
def test_moments_vs_fp64(capi, c, oc, frames, wide):
    """ldo = out_channels (8 for the recipe's token_size 4: the compact buffer the module uses) and ldo = 64.  The reference is
    conv_out on `t.reshape(F, C, 32, 1)` of the contiguous (F, 32, C) rows -- torch's own reshape, in fp64.  Reading the reshape as a
    transpose must miss the same bar by more than 100 x."""
    nlat = 32
    ldo = 64 if wide else oc
    g = torch.Generator().manual_seed(c + oc + frames + ldo)
    t = torch.randn(frames, nlat, c, generator=g)
    w, bias = torch.randn(oc, c, generator=g) / math.sqrt(c), 0.5 * torch.randn(oc, generator=g)
    td = t.double().contiguous()
    conv = lambda v: F.conv2d(v, w.double().reshape(oc, c, 1, 1), bias.double()).reshape(frames, oc, nlat).transpose(1, 2)   # noqa: E731
    ref, wrong = conv(td.reshape(frames, c, nlat, 1)), conv(td.permute(0, 2, 1).reshape(frames, c, nlat, 1))
    dev = [v.cuda().contiguous() for v in (t, w, bias)]
    out = torch.full((frames, nlat, ldo), NAN, device="cuda")
    capi.check(capi.lib.dfot_op_titok_moments(*[capi.ptr(v) for v in dev], capi.ptr(out), ldo, frames, nlat, c, oc, capi.stream_ptr()))
    got = out.cpu()
    name = f"moments C {c} out_channels {oc} frames {frames} ldo {ldo}"
    check_f32(name, got[..., :oc], ref)
    assert torch.isnan(got[..., oc:]).all()                          # columns past out_channels are not written
    r, worst = f32_errors(name + ", against the TRANSPOSING reading", got[..., :oc], wrong)
    assert r > 100 * 1e-5 and worst > 100 * 1e-5


def test_moments_refuses_bad_shapes_before_any_launch(capi):
    dev = [torch.zeros(s, device="cuda") for s in ((1, 32, 512), (130, 512), (130,))]
    out = torch.full((1, 32, 256), NAN, device="cuda")
    for ldo, nlat, c, oc, word in ((64, 32, 512, 7, "out_channels=7"), (256, 32, 512, 130, "out_channels=130"), (64, 32, 640, 8, "channels=640"),
                                   (4, 32, 512, 8, "ldo=4"), (64, 0, 512, 8, "num_latent=0")):
        rc = capi.lib.dfot_op_titok_moments(*[capi.ptr(v) for v in dev], capi.ptr(out), ldo, 1, nlat, c, oc, capi.stream_ptr())
        assert rc == capi.ERR_SHAPE
        assert "op_titok_moments" in capi.lib.dfot_last_error().decode() and word in capi.lib.dfot_last_error().decode()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
