"""GPU: the three ImageVAE ops of csrc/image_vae.hip, each against an fp64 torch computation of the same bf16-rounded operands.

Bars (taken from the existing op tests, not from these kernels):
  * fused per-frame attention: rel-L2 < 1.5e-2, the attention-op bar of tests/test_gpu_dit.py:88 (bf16 rounding of P and O);
  * stride-2 convolution and upsample-convolution: rel-L2 < 1e-5 and max abs error < 1e-3, the bar of the 3x3 convolution test
    tests/test_gpu_ops.py:106 (bf16 operands are exact in the reference, so only the fp32 summation order differs)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import dfot_amd  # noqa: F401
    from dfot_amd import capi as c
    assert torch.cuda.is_available()
    return c


def report(name, got, ref):
    err = (got.double() - ref).abs().max().item()
    rel = ((got.double() - ref).norm() / ref.norm().clamp_min(1e-12)).item()
    print(f"{name}: max_abs={err:.3e} rel_l2={rel:.3e}")
    return err, rel


def run_attention(capi, q, k, v):
    """q, k, v fp32 [frames][n][c] (bf16-representable) -> (o of the op as fp32 on the host, fp64 reference)"""
    frames, n, c = q.shape
    qd, kd, vd = (t.to(torch.bfloat16).reshape(frames * n, c).contiguous().cuda() for t in (q, k, v))
    o = torch.full((frames * n, c), float("nan"), dtype=torch.bfloat16, device="cuda")
    capi.check(capi.lib.dfot_op_ivae_attention(capi.ptr(qd), capi.ptr(kd), capi.ptr(vd), capi.ptr(o), frames, n, c, capi.stream_ptr()))
    torch.cuda.synchronize()
    q64, k64, v64 = (t.double() for t in (q, k, v))
    ref = torch.softmax(q64 @ k64.transpose(1, 2) / math.sqrt(c), -1) @ v64
    return o.float().cpu().reshape(frames, n, c), ref


def bf(t):
    return t.to(torch.bfloat16).float()


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("c", [128, 512])
def test_fused_attention(capi, n, c):
    g = torch.Generator().manual_seed(n + c)
    q, k, v = (bf(torch.randn(3, n, c, generator=g)) for _ in range(3))
    got, ref = run_attention(capi, q, k, v)
    err, rel = report(f"ivae attention frames 3 N {n} C {c}", got, ref)
    assert torch.isfinite(got).all() and rel < 1.5e-2


@pytest.mark.parametrize("mult,floor", [(8.0, 30.0), (32.0, 89.0)])
def test_fused_attention_large_scores_need_the_max_subtraction(capi, mult, floor):
    """q x 8 (and x 32): unit-normal q, k give scores / sqrt(C) of about N(0, mult^2), whose maximum over 3 x 256 x 256 entries is near
    5.3 mult: ~43 at x 8, where the raw exponentials (e^43 = 4e18) are far outside bf16 P's useful range and a softmax without the max
    subtraction loses every small probability, and ~170 at x 32, where exp of the raw score overflows fp32 outright (e^88.7).  Only
    exp(s - max) stays in range."""
    g = torch.Generator().manual_seed(5)
    n, c = 256, 512
    q, k, v = (bf(torch.randn(3, n, c, generator=g)) for _ in range(3))
    q = bf(q * mult)
    top = ((q @ k.transpose(1, 2)) / math.sqrt(c)).max().item()
    print(f"largest score / sqrt(C) at q x {mult:g}: {top:.1f}")
    assert top > floor
    got, ref = run_attention(capi, q, k, v)
    err, rel = report(f"ivae attention, q x {mult:g}", got, ref)
    assert torch.isfinite(got).all() and rel < 1.5e-2


@pytest.mark.parametrize("n", [64, 256])
def test_fused_attention_frames_do_not_mix(capi, n):
    """frame 1's k / v are far from frame 0's (another scale and offset): a read across the frame boundary shows at once"""
    g = torch.Generator().manual_seed(9 + n)
    c = 128
    q, k, v = (bf(torch.randn(3, n, c, generator=g)) for _ in range(3))
    k[1] = bf(3.0 * k[1] + 2.0)
    v[1] = bf(50.0 * v[1] - 100.0)
    got, ref = run_attention(capi, q, k, v)
    for f in range(3):
        err, rel = report(f"ivae attention N {n}, frame {f}", got[f], ref[f])
        assert rel < 1.5e-2


def test_fused_attention_refuses_other_shapes(capi):
    t = torch.zeros(128 * 128, dtype=torch.bfloat16, device="cuda")
    for n, c in ((128, 128), (64, 64), (256, 192), (64, 2048)):
        rc = capi.lib.dfot_op_ivae_attention(capi.ptr(t), capi.ptr(t), capi.ptr(t), capi.ptr(torch.empty_like(t)), 1, n, c, capi.stream_ptr())
        assert rc == capi.ERR_SHAPE
        msg = capi.lib.dfot_last_error().decode()
        assert f"N={n}" in msg and f"C={c}" in msg


def conv_operands(g, frames, h, w, cin, cout):
    x = bf(torch.randn(frames, cin, h, w, generator=g))
    wt = bf(torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin))
    bias = torch.randn(cout, generator=g)
    a = x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).cuda()                             # NHWC
    wp = wt.permute(0, 2, 3, 1).reshape(cout, 9 * cin).contiguous().to(torch.bfloat16).cuda()    # [Cout][tap][Cin]
    return x, wt, bias, a, wp


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("cout", [128, 256])
def test_stride2_conv_pads_right_and_bottom_only(capi, cout, with_bias):
    frames, h, w, cin = 8, 8, 8, 128
    g = torch.Generator().manual_seed(cout + with_bias)
    x, wt, bias, a, wp = conv_operands(g, frames, h, w, cin, cout)
    out = torch.full((frames, h // 2, w // 2, cout), float("nan"), device="cuda")
    bd = bias.cuda() if with_bias else None
    capi.check(capi.lib.dfot_op_conv3x3_s2_f32(capi.ptr(a), capi.ptr(wp), capi.ptr(bd), capi.ptr(out), frames, h, w, cin, cout, capi.stream_ptr()))
    torch.cuda.synchronize()
    b64 = bias.double() if with_bias else None
    ref = F.conv2d(F.pad(x.double(), (0, 1, 0, 1)), wt.double(), b64, stride=2).permute(0, 2, 3, 1)
    err, rel = report(f"stride-2 conv 8x8x{cin} -> 4x4x{cout} bias={with_bias}", out.cpu(), ref)
    assert torch.isfinite(out).all() and rel < 1e-5 and err < 1e-3
    # the test can tell the paddings apart: symmetric or top-left padding is far outside the bar on this input
    for pad in ((1, 1, 1, 1), (1, 0, 1, 0)):
        other = F.conv2d(F.pad(x.double(), pad), wt.double(), b64, stride=2)[:, :, : h // 2, : w // 2].permute(0, 2, 3, 1)
        assert ((other - ref).norm() / ref.norm()).item() > 0.1


@pytest.mark.parametrize("cout", [128, 256])
def test_upsample_conv(capi, cout):
    frames, h, w, cin = 2, 8, 8, 256
    g = torch.Generator().manual_seed(cout + 7)
    x, wt, bias, a, wp = conv_operands(g, frames, h, w, cin, cout)
    out = torch.full((frames, 2 * h, 2 * w, cout), float("nan"), device="cuda")
    bd = bias.cuda()
    capi.check(capi.lib.dfot_op_upconv3x3_f32(capi.ptr(a), capi.ptr(wp), capi.ptr(bd), capi.ptr(out), frames, h, w, cin, cout, capi.stream_ptr()))
    torch.cuda.synchronize()
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), wt.double(), bias.double(), padding=1).permute(0, 2, 3, 1)
    err, rel = report(f"upsample-conv 8x8x{cin} -> 16x16x{cout}", out.cpu(), ref)
    assert torch.isfinite(out).all() and rel < 1e-5 and err < 1e-3


def test_convs_refuse_bad_shapes(capi):
    t = torch.zeros(1 << 16, dtype=torch.bfloat16, device="cuda")
    o = torch.zeros(1 << 16, device="cuda")
    s = capi.stream_ptr()
    assert capi.lib.dfot_op_conv3x3_s2_f32(capi.ptr(t), capi.ptr(t), None, capi.ptr(o), 1, 7, 8, 64, 128, s) == capi.ERR_SHAPE   # odd height
    assert capi.lib.dfot_op_conv3x3_s2_f32(capi.ptr(t), capi.ptr(t), None, capi.ptr(o), 1, 8, 8, 48, 128, s) == capi.ERR_SHAPE   # Cin % 64
    assert capi.lib.dfot_op_upconv3x3_f32(capi.ptr(t), capi.ptr(t), None, capi.ptr(o), 1, 8, 8, 64, 100, s) == capi.ERR_SHAPE    # Cout % 128
    assert capi.lib.dfot_op_upconv3x3_f32(None, capi.ptr(t), None, capi.ptr(o), 1, 8, 8, 64, 128, s) == capi.ERR_ARG
