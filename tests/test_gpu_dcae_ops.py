"""GPU: the DC-AE ops of csrc/dcae.hip, each against a torch computation of the same operands in higher precision.

Bars (from the existing op tests and the number formats, not from these kernels):
  * ReLU linear attention: rel-L2 < 1.5e-2, the attention-op bar of tests/test_gpu_image_vae_ops.py (the output is bf16: one rounding is
    about 2e-3; the state and the division are fp32);
  * depthwise 3x3 + SiLU gate: rel-L2 <= 3e-3 (each bf16 output element is one rounding, <= 2^-9 relative, plus the fast SiLU
    exponential); border rows / columns separately, so that a wrong padding cannot hide in the interior's weight;
  * resampling / shortcut kernels against fp32 torch: rel-L2 <= 1e-6 (sums of at most 33 fp32 terms);
  * channel RMSNorm: the norm-op bars of tests/test_gpu_titok_ops.py: fp32 output 1e-5, bf16 output 4e-3 (rel-L2).
Measured on an MI355X: see DESIGN.md (the DC-AE section)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def capi():
    import dfot_amd  # noqa: F401
    from dfot_amd import capi as c
    assert torch.cuda.is_available()
    return c


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    """hand the module's cached device blocks (NaN- and sentinel-filled buffers among them) back to the driver when it is done, so that
    the test modules after this one start from the allocator state they had without it"""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def rel(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30)).item()


def bf(t):
    return t.to(BF).float()


SENTINEL = 64   # elements behind every output buffer that must keep their fill


def guarded(shape, dtype):
    """a NaN-filled output with a sentinel tail behind it: (the whole buffer, the output view)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + SENTINEL,), float("nan"), dtype=dtype, device="cuda")
    buf[n:] = 7.0
    return buf, buf[:n].view(shape)


def tail_ok(buf):
    return bool((buf[-SENTINEL:].float() == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------------------
def linattn_ref(qkv, frames, n, heads):
    """qkv fp32 [frames * n][96 heads] (bf16-representable) -> fp64 [frames * n][32 heads]"""
    t = qkv.double().reshape(frames, n, heads, 96)
    q, k, v = t[..., :32].relu(), t[..., 32:64].relu(), t[..., 64:]
    v1 = torch.cat([v, torch.ones_like(v[..., :1])], -1)
    s = torch.einsum("fnhj,fnhd->fhjd", k, v1)
    o = torch.einsum("fnhj,fhjd->fnhd", q, s)
    return (o[..., :32] / (o[..., 32:] + 1e-15)).reshape(frames * n, heads * 32)


def run_linattn(capi, qkv, frames, n, heads):
    dev = qkv.to(BF).cuda()
    buf, o = guarded((frames * n, heads * 32), BF)
    capi.check(capi.lib.dfot_op_dcae_linear_attention(capi.ptr(dev), 96 * heads, capi.ptr(o), 32 * heads, frames, n, heads, capi.stream_ptr()))
    torch.cuda.synchronize()
    assert tail_ok(buf)
    return o.float().cpu()


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("frames", [1, 3])
def test_linear_attention(capi, frames, heads, n):
    g = torch.Generator().manual_seed(100 * frames + 10 * heads + n)
    qkv = bf(torch.randn(frames * n, 96 * heads, generator=g))
    got, ref = run_linattn(capi, qkv, frames, n, heads), linattn_ref(qkv, frames, n, heads)
    r = rel(got, ref)
    print(f"linear attention frames {frames} heads {heads} N {n}: rel_l2={r:.3e}")
    assert torch.isfinite(got).all() and r < 1.5e-2


@pytest.mark.parametrize("n", [64, 256])
def test_linear_attention_small_denominator(capi, n):
    """head 1's q is negative in every channel but one (and tiny there): relu leaves one term, the denominator is ~1e-3 of the usual"""
    g = torch.Generator().manual_seed(n)
    frames, heads = 3, 4
    qkv = torch.randn(frames * n, 96 * heads, generator=g)
    qkv[:, 96:128] = -qkv[:, 96:128].abs() - 0.1
    qkv[:, 96 + 5] = 1e-3 * (1.0 + torch.rand(frames * n, generator=g))
    qkv = bf(qkv)
    got, ref = run_linattn(capi, qkv, frames, n, heads), linattn_ref(qkv, frames, n, heads)
    r, r1 = rel(got, ref), rel(got[:, 32:64], ref[:, 32:64])
    print(f"linear attention, small denominator, N {n}: rel_l2={r:.3e}, head 1 alone {r1:.3e}")
    assert torch.isfinite(got).all() and r < 1.5e-2 and r1 < 1.5e-2


def test_linear_attention_frame_alone_equals_frame_in_batch(capi):
    g = torch.Generator().manual_seed(3)
    n, heads = 256, 4
    qkv = bf(torch.randn(3 * n, 96 * heads, generator=g))
    qkv[n:2 * n] = bf(4.0 * qkv[n:2 * n] + 1.0)      # another scale next door: a read across the frame boundary shows
    whole = run_linattn(capi, qkv, 3, n, heads)
    for f in range(3):
        assert torch.equal(run_linattn(capi, qkv[f * n:(f + 1) * n], 1, n, heads), whole[f * n:(f + 1) * n])


def test_linear_attention_strided_rows(capi):
    """ld / ldo wider than the heads need: the columns in between are neither read as heads nor written"""
    g = torch.Generator().manual_seed(4)
    n, heads, ld, ldo = 64, 2, 256, 80
    wide = bf(torch.randn(n, ld, generator=g))
    dev = wide.to(BF).cuda()
    o = torch.full((n, ldo), 3.0, dtype=BF, device="cuda")
    capi.check(capi.lib.dfot_op_dcae_linear_attention(capi.ptr(dev), ld, capi.ptr(o), ldo, 1, n, heads, capi.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((o[:, 64:] == 3.0).all())
    assert rel(o[:, :64].float().cpu(), linattn_ref(wide[:, :192], 1, n, heads)) < 1.5e-2


# ---------------------------------------------------------------------------------------------------------------------------------
def run_dw_glu(capi, x, w, b):
    """x fp32 (F, 2 hc, H, W) bf16-representable, w (2 hc, 1, 3, 3), b (2 hc) -> the op's output as fp32 (F, hc, H, W)"""
    f, c2, h, ww = x.shape
    xd = x.permute(0, 2, 3, 1).contiguous().to(BF).cuda()
    wt, bd = w.reshape(c2, 9).t().contiguous().cuda(), b.cuda()
    buf, o = guarded((f, h, ww, c2 // 2), BF)
    capi.check(capi.lib.dfot_op_dcae_dw_glu(capi.ptr(xd), capi.ptr(wt), capi.ptr(bd), capi.ptr(o), f, h, ww, c2 // 2, capi.stream_ptr()))
    torch.cuda.synchronize()
    assert tail_ok(buf)
    return o.float().cpu().permute(0, 3, 1, 2)


def dw_glu_ref(x, w, b):
    y = F.conv2d(x.double(), w.double(), b.double(), padding=1, groups=x.shape[1])
    a, gate = y.chunk(2, dim=1)
    return a * gate * torch.sigmoid(gate)


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("c2", [512, 1024])
@pytest.mark.parametrize("size", [8, 16])
def test_dw_glu(capi, size, c2, frames):
    g = torch.Generator().manual_seed(size + c2 + frames)
    x = bf(torch.randn(frames, c2, size, size, generator=g))
    w, b = torch.randn(c2, 1, 3, 3, generator=g) / 3.0, 0.5 * torch.randn(c2, generator=g)
    got, ref = run_dw_glu(capi, x, w, b), dw_glu_ref(x, w, b)
    inner = (slice(None), slice(None), slice(1, -1), slice(1, -1))
    edge = torch.ones(size, size, dtype=torch.bool)
    edge[1:-1, 1:-1] = False
    r, r_in, r_edge = rel(got, ref), rel(got[inner], ref[inner]), rel(got[..., edge], ref[..., edge])
    print(f"dw_glu {size}x{size} 2h={c2} frames {frames}: rel_l2={r:.3e} interior {r_in:.3e} border {r_edge:.3e}")
    assert torch.isfinite(got).all() and r <= 3e-3 and r_in <= 3e-3 and r_edge <= 3e-3
    # the test can tell zero padding from replicated borders on this input
    other = F.conv2d(F.pad(x.double(), (1, 1, 1, 1), mode="replicate"), w.double(), b.double(), groups=c2)
    a, gate = other.chunk(2, dim=1)
    assert rel((a * gate * torch.sigmoid(gate))[..., edge], ref[..., edge]) > 0.1


def test_dw_glu_frame_alone_equals_frame_in_batch(capi):
    g = torch.Generator().manual_seed(8)
    x = bf(torch.randn(3, 512, 8, 8, generator=g))
    x[1] = bf(5.0 * x[1] + 2.0)
    w, b = torch.randn(512, 1, 3, 3, generator=g) / 3.0, 0.5 * torch.randn(512, generator=g)
    whole = run_dw_glu(capi, x, w, b)
    for f in range(3):
        assert torch.equal(run_dw_glu(capi, x[f:f + 1], w, b)[0], whole[f])


# ---------------------------------------------------------------------------------------------------------------------------------
def cl(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("gs", [2, 4, 8])
@pytest.mark.parametrize("shortcut", [True, False])
def test_down_shortcut_unshuffle_and_group_mean(capi, gs, shortcut):
    g = torch.Generator().manual_seed(gs)
    frames, h, w, cout = 3, 6, 10, 32
    cin, ldc = cout * gs // 4, 64                       # the convolution's output is padded to 64 channels: 8 are real
    conv, src = torch.randn(frames, cout // 4, h, w, generator=g), torch.randn(frames, cin, h, w, generator=g)
    convp = torch.full((frames, h, w, ldc), float("nan"))
    convp[..., : cout // 4] = cl(conv)
    buf, out = guarded((frames, h // 2, w // 2, cout), torch.float32)
    cd, sd = convp.cuda(), cl(src).cuda()                # (named: a temporary's memory would be reused by the next allocation)
    capi.check(capi.lib.dfot_op_dcae_down_shortcut(capi.ptr(cd), ldc, capi.ptr(sd) if shortcut else None, capi.ptr(out), frames, h, w, cin, cout, 2,
                                                   capi.stream_ptr()))
    torch.cuda.synchronize()
    ref = F.pixel_unshuffle(conv, 2)
    if shortcut:
        ref = ref + F.pixel_unshuffle(src, 2).unflatten(1, (-1, gs)).mean(dim=2)
    r = rel(out.cpu(), cl(ref))
    print(f"down shortcut group {gs} shortcut={shortcut}: rel_l2={r:.3e}")
    assert tail_ok(buf) and r <= 1e-6


@pytest.mark.parametrize("gs", [2, 4, 8])
def test_group_mean_without_resampling(capi, gs):
    """the encoder's output shortcut: factor 1"""
    g = torch.Generator().manual_seed(gs + 20)
    frames, h, w, cout, ldc = 3, 4, 5, 32, 64
    conv, src = torch.randn(frames, cout, h, w, generator=g), torch.randn(frames, cout * gs, h, w, generator=g)
    convp = torch.full((frames, h, w, ldc), float("nan"))
    convp[..., :cout] = cl(conv)
    buf, out = guarded((frames, h, w, cout), torch.float32)
    cd, sd = convp.cuda(), cl(src).cuda()
    capi.check(capi.lib.dfot_op_dcae_down_shortcut(capi.ptr(cd), ldc, capi.ptr(sd), capi.ptr(out), frames, h, w, cout * gs, cout, 1, capi.stream_ptr()))
    torch.cuda.synchronize()
    r = rel(out.cpu(), cl(conv + src.unflatten(1, (-1, gs)).mean(dim=2)))
    print(f"group mean {gs}: rel_l2={r:.3e}")
    assert tail_ok(buf) and r <= 1e-6


@pytest.mark.parametrize("rep", [2, 4, 8])
@pytest.mark.parametrize("shortcut", [True, False])
def test_up_shortcut_shuffle_and_repeat(capi, rep, shortcut):
    g = torch.Generator().manual_seed(rep + 40)
    frames, h, w, cout = 3, 5, 3, 16
    cin = 4 * cout // rep
    conv, src = torch.randn(frames, 4 * cout, h, w, generator=g), torch.randn(frames, cin, h, w, generator=g)
    buf, out = guarded((frames, 2 * h, 2 * w, cout), torch.float32)
    cd, sd = cl(conv).cuda(), cl(src).cuda()
    capi.check(capi.lib.dfot_op_dcae_up_shortcut(capi.ptr(cd), 4 * cout, capi.ptr(sd) if shortcut else None, cin, capi.ptr(out), frames, h, w, cin, cout, 2,
                                                 capi.stream_ptr()))
    torch.cuda.synchronize()
    ref = F.pixel_shuffle(conv, 2)
    if shortcut:
        ref = ref + F.pixel_shuffle(src.repeat_interleave(rep, dim=1), 2)
    r = rel(out.cpu(), cl(ref))
    print(f"up shortcut repeat {rep} shortcut={shortcut}: rel_l2={r:.3e}")
    assert tail_ok(buf) and r <= 1e-6


@pytest.mark.parametrize("rep", [2, 4, 8])
def test_repeat_without_resampling(capi, rep):
    """the decoder's input shortcut: factor 1, the latent padded to 64 channels"""
    g = torch.Generator().manual_seed(rep + 60)
    frames, h, w, cin, lds = 3, 4, 4, 32, 64
    conv, z = torch.randn(frames, cin * rep, h, w, generator=g), torch.randn(frames, cin, h, w, generator=g)
    zp = torch.full((frames, h, w, lds), float("nan"))
    zp[..., :cin] = cl(z)
    buf, out = guarded((frames, h, w, cin * rep), torch.float32)
    cd, zd = cl(conv).cuda(), zp.cuda()
    capi.check(capi.lib.dfot_op_dcae_up_shortcut(capi.ptr(cd), cin * rep, capi.ptr(zd), lds, capi.ptr(out), frames, h, w, cin, cin * rep, 1,
                                                 capi.stream_ptr()))
    torch.cuda.synchronize()
    r = rel(out.cpu(), cl(conv + z.repeat_interleave(rep, dim=1)))
    print(f"repeat {rep}: rel_l2={r:.3e}")
    assert tail_ok(buf) and r <= 1e-6


def test_final_up_block_to_three_channels(capi):
    """the decoder's conv_out: 12 real channels of a 64-wide convolution output, no shortcut, 3 output channels"""
    g = torch.Generator().manual_seed(77)
    frames, h, w = 2, 4, 4
    conv = torch.randn(frames, 12, h, w, generator=g)
    convp = torch.full((frames, h, w, 64), float("nan"))
    convp[..., :12] = cl(conv)
    buf, out = guarded((frames, 2 * h, 2 * w, 3), torch.float32)
    cd = convp.cuda()
    capi.check(capi.lib.dfot_op_dcae_up_shortcut(capi.ptr(cd), 64, None, 0, capi.ptr(out), frames, h, w, 0, 3, 2, capi.stream_ptr()))
    torch.cuda.synchronize()
    assert tail_ok(buf) and torch.equal(out.cpu(), cl(F.pixel_shuffle(conv, 2)))


# ---------------------------------------------------------------------------------------------------------------------------------
def rms_ref(x, w, b, resid, relu):
    x = x.double()
    y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-5) * w.double() + b.double()
    if resid is not None:
        y = y + resid.double()
    return y.relu() if relu else y


@pytest.mark.parametrize("channels", [64, 128, 512, 1024])
@pytest.mark.parametrize("form", ["residual", "relu_bf16", "plain_both"])
def test_rmsnorm_forms(capi, channels, form):
    g = torch.Generator().manual_seed(channels)
    rows = 131                                            # not a multiple of the 4 rows of a workgroup
    x, resid = 3.0 * torch.randn(rows, channels, generator=g), torch.randn(rows, channels, generator=g)
    w, b = 1 + 0.3 * torch.randn(channels, generator=g), 0.2 * torch.randn(channels, generator=g)
    use_resid, relu = form == "residual", form == "relu_bf16"
    want32, want16 = form != "relu_bf16", form != "residual"
    b32, o32 = guarded((rows, channels), torch.float32)
    b16, o16 = guarded((rows, channels), BF)
    xd, wd, bd, rd = x.cuda(), w.cuda(), b.cuda(), resid.cuda()
    capi.check(capi.lib.dfot_op_dcae_rmsnorm(capi.ptr(xd), capi.ptr(wd), capi.ptr(bd), 1e-5, capi.ptr(rd) if use_resid else None,
                                             capi.ptr(o32) if want32 else None, capi.ptr(o16) if want16 else None, int(relu), rows, channels,
                                             capi.stream_ptr()))
    torch.cuda.synchronize()
    ref = rms_ref(x, w, b, resid if use_resid else None, relu)
    assert tail_ok(b32) and tail_ok(b16)
    if want32:
        r = rel(o32.cpu(), ref)
        print(f"rmsnorm {form} C={channels} fp32: rel_l2={r:.3e}")
        assert r <= 1e-5
    else:
        assert torch.isnan(o32).all()                     # an output that was not asked for is not written
    if want16:
        r = rel(o16.float().cpu(), ref)
        print(f"rmsnorm {form} C={channels} bf16: rel_l2={r:.3e}")
        assert r <= 4e-3
        if relu:
            assert (o16.float() >= 0).all()
    else:
        assert torch.isnan(o16.float()).all()


def test_act_bf16(capi):
    g = torch.Generator().manual_seed(2)
    x = 3.0 * torch.randn(1000, generator=g)
    for act, fn in ((0, lambda t: t), (1, torch.relu), (2, lambda t: t * torch.sigmoid(t))):
        buf, o = guarded((1000,), BF)
        xd = x.cuda()
        capi.check(capi.lib.dfot_op_dcae_act_bf16(capi.ptr(xd), capi.ptr(o), 1000, act, capi.stream_ptr()))
        torch.cuda.synchronize()
        r = rel(o.float().cpu(), fn(x.double()))
        print(f"act {act}: rel_l2={r:.3e}")
        assert tail_ok(buf) and r <= 4e-3


# ---------------------------------------------------------------------------------------------------------------------------------
def test_invalid_shapes_launch_nothing(capi):
    L, s = capi.lib, capi.stream_ptr()
    t16 = torch.zeros(1 << 16, dtype=BF, device="cuda")
    o16 = torch.full((1 << 16,), float("nan"), dtype=BF, device="cuda")
    t32 = torch.zeros(1 << 16, device="cuda")
    o32 = torch.full((1 << 16,), float("nan"), device="cuda")
    P = capi.ptr
    for n, heads, ld, ldo in ((32, 1, 96, 32), (96, 1, 96, 32), (8192, 1, 96, 32), (64, 0, 96, 32), (64, 65, 6240, 2080), (64, 2, 96, 64), (64, 1, 100, 32),
                              (64, 1, 96, 24)):
        assert L.dfot_op_dcae_linear_attention(P(t16), ld, P(o16), ldo, 1, n, heads, s) == capi.ERR_SHAPE, (n, heads, ld, ldo)
        assert f"N={n}" in L.dfot_last_error().decode()
    assert L.dfot_op_dcae_linear_attention(P(t16), 96, P(o16), 32, 0, 64, 1, s) == capi.ERR_SHAPE
    assert L.dfot_op_dcae_linear_attention(None, 96, P(o16), 32, 1, 64, 1, s) == capi.ERR_ARG
    assert L.dfot_op_dcae_linear_attention(P(t16), 96, P(t16), 32, 1, 64, 1, s) == capi.ERR_ARG          # aliased
    assert L.dfot_op_dcae_dw_glu(P(t16), P(t32), P(t32), P(o16), 1, 8, 8, 128, s) == capi.ERR_SHAPE         # hc % 256
    assert L.dfot_op_dcae_dw_glu(P(t16), P(t32), P(t32), P(o16), 1, 0, 8, 256, s) == capi.ERR_SHAPE
    assert L.dfot_op_dcae_dw_glu(P(t16), None, P(t32), P(o16), 1, 8, 8, 256, s) == capi.ERR_ARG
    assert L.dfot_op_dcae_down_shortcut(P(t32), 64, P(t32), P(o32), 1, 7, 8, 16, 32, 2, s) == capi.ERR_SHAPE    # odd height
    assert L.dfot_op_dcae_down_shortcut(P(t32), 64, P(t32), P(o32), 1, 8, 8, 12, 32, 2, s) == capi.ERR_SHAPE    # 4 * 12 % 32
    assert L.dfot_op_dcae_down_shortcut(P(t32), 4, P(t32), P(o32), 1, 8, 8, 16, 32, 2, s) == capi.ERR_SHAPE     # ldc < cout / 4
    assert L.dfot_op_dcae_down_shortcut(P(t32), 64, P(t32), P(o32), 1, 8, 8, 16, 32, 3, s) == capi.ERR_SHAPE    # factor
    assert L.dfot_op_dcae_down_shortcut(None, 64, P(t32), P(o32), 1, 8, 8, 16, 32, 2, s) == capi.ERR_ARG
    assert L.dfot_op_dcae_up_shortcut(P(t32), 64, P(t32), 16, P(o32), 1, 8, 8, 24, 16, 2, s) == capi.ERR_SHAPE  # 64 % 24
    assert L.dfot_op_dcae_up_shortcut(P(t32), 32, P(t32), 16, P(o32), 1, 8, 8, 16, 16, 2, s) == capi.ERR_SHAPE  # ldc < 4 cout
    assert L.dfot_op_dcae_up_shortcut(P(t32), 64, P(t32), 8, P(o32), 1, 8, 8, 16, 16, 2, s) == capi.ERR_SHAPE   # lds < cin
    assert L.dfot_op_dcae_up_shortcut(P(t32), 64, P(t32), 16, None, 1, 8, 8, 16, 16, 2, s) == capi.ERR_ARG
    assert L.dfot_op_dcae_rmsnorm(P(t32), P(t32), P(t32), 1e-5, None, P(o32), None, 0, 4, 66, s) == capi.ERR_SHAPE     # C % 4
    assert L.dfot_op_dcae_rmsnorm(P(t32), P(t32), P(t32), 1e-5, None, P(o32), None, 0, 4, 4096, s) == capi.ERR_SHAPE   # C > 2048
    assert L.dfot_op_dcae_rmsnorm(P(t32), P(t32), P(t32), 1e-5, None, None, None, 0, 4, 64, s) == capi.ERR_ARG         # no output
    assert L.dfot_op_dcae_act_bf16(P(t32), P(o16), 1002, 1, s) == capi.ERR_SHAPE
    assert L.dfot_op_dcae_act_bf16(P(t32), P(o16), 1000, 3, s) == capi.ERR_SHAPE
    torch.cuda.synchronize()
    assert torch.isnan(o16.float()).all() and torch.isnan(o32).all()     # nothing was launched
