"""GPU: the VideoVAE encoder (frames -> latents, the online Kinetics-600 path: BaseVideoAlgo._encode, base_pytorch_video_algo.py:553-596;
VideoVAE.encode, algorithms/vae/video_vae/model.py:38-150,402-443).
  * the strided / causal-temporal implicit-GEMM convolution (dfot_op_conv3t_f32) against an fp64 restatement with the reference's
    padding built in torch (first frame repeated kt - 1 times in front; zero pad 1 | 1 for stride 1, 0 | 1 for stride 2) on the same
    bf16-rounded operands: fp32 accumulation is the only error source;
  * the pixel front end (exact) and the posterior kernel (clamp, sample, fused _normalize_x) against the torch formulas;
  * the whole encoder against tests/golden/vae_encode.npz, captured from the reference's own VideoVAE (rel-L2 <= 2e-2: the decoder's bar for
    the same bf16-operand / fp32-accumulate op mix and depth);
  * encode_videos: the _encode convention, chunking, and per-video independence of the GroupNorm statistics at the K600 geometry."""
import ast
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def capi():
    import dfot_amd  # noqa: F401
    from dfot_amd import capi as c
    return c


def conv_ref(x, w, bias, resid, kt, s, st):
    """fp64: x (B, T, H, W, Cin) channels-last, w (Cout, Cin, kt, 3, 3) -> (B, To, H / s, W / s, Cout), the reference's padding explicit"""
    if kt > 1:
        x = torch.cat([x[:, :1].expand(-1, kt - 1, -1, -1, -1), x], 1)        # PaddedConv3D: first frame repeated in front
    lo = 1 if s == 1 else 0                                                 # Downsample / Spatial2xTime2x3DDownsample: pad (0, 1)
    x = torch.nn.functional.pad(x, (0, 0, lo, 1, lo, 1))
    b, tp, hp, wp, _ = x.shape
    to, ho, wo = (tp - kt) // st + 1, (hp - 3) // s + 1, (wp - 3) // s + 1
    out = torch.zeros(b, to, ho, wo, w.shape[0], dtype=torch.float64, device=x.device)
    for dt in range(kt):
        for dy in range(3):
            for dx in range(3):
                sl = x[:, dt:dt + st * (to - 1) + 1:st, dy:dy + s * (ho - 1) + 1:s, dx:dx + s * (wo - 1) + 1:s]
                out += sl @ w[:, :, dt, dy, dx].t()
    if bias is not None:
        out += bias
    if resid is not None:
        out += resid
    return out


# (kt, spatial stride, time stride, B, T, H_in, W_in, Cin, Cout, bias, residual)
CONV_CASES = [
    (1, 1, 1, 1, 2, 16, 16, 64, 32, False, False),
    (1, 2, 1, 2, 9, 32, 32, 256, 128, True, False),        # Downsample (2-D, stride 2)
    (1, 2, 1, 2, 17, 128, 128, 128, 128, True, False),     # level-0 Downsample at K600 size (512x128 tiles)
    (1, 2, 2, 1, 9, 32, 32, 64, 128, True, False),         # time stride without temporal taps
    (3, 1, 1, 1, 17, 16, 16, 64, 128, True, True),
    (3, 1, 1, 2, 9, 16, 16, 512, 512, True, True),         # level-3 / mid ResnetBlock3D (split-K inside the workgroup)
    (3, 1, 1, 2, 17, 32, 32, 256, 512, True, False),       # 256x256 tiles
    (3, 1, 2, 1, 2, 16, 16, 256, 32, False, True),
    (3, 2, 2, 1, 17, 32, 32, 256, 512, True, False),       # Spatial2xTime2x3DDownsample 17 -> 9
    (3, 2, 2, 2, 9, 32, 16, 512, 512, True, True),         # 9 -> 5, non-square
    (3, 2, 2, 1, 1, 32, 32, 64, 32, False, False),         # a single frame stays one frame
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "kt{}_s{}_st{}_B{}_T{}_{}x{}_{}to{}{}{}".format(*c[:9], "_bias" if c[9] else "",
                                                                                                         "_resid" if c[10] else ""))
def test_conv3t_vs_fp64(capi, case):
    kt, s, st, b, t, h, w, ci, co, has_bias, has_res = case
    g = torch.Generator(device="cuda").manual_seed(hash(case) % 2 ** 31)
    x = torch.randn(b, t, h, w, ci, device="cuda", generator=g).to(BF)
    wt = (torch.randn(co, ci, kt, 3, 3, device="cuda", generator=g) / (kt * 9 * ci) ** 0.5).to(BF)
    wp = wt.permute(0, 2, 3, 4, 1).reshape(co, kt * 9 * ci).contiguous()        # [Cout][dt][dy][dx][Cin]
    to = (t - 1) // st + 1
    bias = torch.randn(co, device="cuda", generator=g) if has_bias else None
    resid = torch.randn(b, to, h // s, w // s, co, device="cuda", generator=g) if has_res else None
    out = torch.full((b, to, h // s, w // s, co), float("nan"), device="cuda")
    capi.check(capi.lib.dfot_op_conv3t_f32(P(x), P(wp), P(bias), P(resid), P(out), b, t, h, w, ci, co, kt, s, st, S()))
    ref = conv_ref(x.double(), wt.double(), None if bias is None else bias.double(), None if resid is None else resid.double(), kt, s, st)
    r = rel(out, ref)
    print(f"conv3t {case}: rel-L2 vs fp64 {r:.2e}")
    assert out.shape == ref.shape and torch.isfinite(out).all() and r <= 1e-4


def test_conv3t_refuses_bad_geometry(capi):
    x = torch.zeros(1, 3, 16, 16, 64, device="cuda", dtype=BF)
    wp = torch.zeros(64, 27 * 64, device="cuda", dtype=BF)
    out = torch.zeros(1, 3, 8, 8, 64, device="cuda")
    assert capi.lib.dfot_op_conv3t_f32(P(x), P(wp), None, None, P(out), 1, 3, 16, 16, 64, 64, 2, 2, 2, S()) != 0      # kt = 2
    assert capi.lib.dfot_op_conv3t_f32(P(x), P(wp), None, None, P(out), 1, 3, 16, 16, 48, 64, 3, 2, 2, S()) != 0      # Cin % 64
    assert capi.lib.dfot_op_conv3t_f32(P(x), P(wp), None, None, P(out), 1, 1, 16, 8, 64, 64, 3, 2, 1, S()) != 0       # M = 32 rows
    assert capi.lib.dfot_op_conv3t_f32(P(x), P(wp), None, None, P(out), 1, 3, 16, 16, 64, 64, 3, 3, 1, S()) != 0      # stride 3


def test_pixels_and_posterior(capi):
    g = torch.Generator(device="cuda").manual_seed(5)
    y = torch.rand(2, 5, 3, 16, 8, device="cuda", generator=g)                 # b t c h w frames in [0, 1], read through their strides
    out = torch.full((2, 5, 16, 8, 64), float("nan"), device="cuda").to(BF)
    capi.check(capi.lib.dfot_op_vae_pixels(P(y), *y.permute(0, 2, 1, 3, 4).stride(), 2.0, -1.0, P(out), 2, 5, 16, 8, S()))
    ref = torch.zeros(2, 5, 16, 8, 64, device="cuda", dtype=BF)
    ref[..., :3] = (2.0 * y - 1.0).permute(0, 1, 3, 4, 2).to(BF)
    assert torch.equal(out, ref)
    # posterior: moments [B][T][h][w][ld], logvar partly outside [-30, 20]
    b, t, h, w, zc, ld = 2, 3, 4, 8, 16, 64
    mom = torch.randn(b, t, h, w, ld, device="cuda", generator=g) * 25
    eps = torch.randn(b, t, zc, h, w, device="cuda", generator=g)
    dm, ds = torch.randn(zc, device="cuda", generator=g), torch.rand(zc, device="cuda", generator=g) * 5 + 1
    mean, logvar, std, z, zn = (torch.full((b, t, zc, h, w), float("nan"), device="cuda") for _ in range(5))
    capi.check(capi.lib.dfot_op_vae_posterior(P(mom), ld, P(eps), None, None, P(mean), P(logvar), P(std), P(z), b, t, h * w, zc, S()))
    capi.check(capi.lib.dfot_op_vae_posterior(P(mom), ld, P(eps), P(dm), P(ds), None, None, None, P(zn), b, t, h * w, zc, S()))
    m64 = mom.double().permute(0, 1, 4, 2, 3)                                 # b t c h w
    r_mean, r_lv = m64[:, :, :zc], m64[:, :, zc:2 * zc].clamp(-30.0, 20.0)
    assert (m64[:, :, zc:2 * zc] > 20).any() and (m64[:, :, zc:2 * zc] < -30).any()
    r_std = torch.exp(0.5 * r_lv)
    r_z = r_mean + r_std * eps.double()
    for got, want in ((mean, r_mean), (logvar, r_lv), (std, r_std), (z, r_z), (zn, (r_z - dm.double().view(-1, 1, 1)) / ds.double().view(-1, 1, 1))):
        assert rel(got, want) <= 1e-6, rel(got, want)


@pytest.fixture(scope="module")
def fixture_encoder():
    import dfot_amd
    from oracle import vae as ovae
    g = np.load(os.path.join(GOLDEN, "vae_encode.npz"))
    shapes = {str(n): ast.literal_eval(str(s)) for n, s in zip(g["names"], g["shapes"])}
    enc = dfot_amd.VideoVAEEncoder(hidden_size=128, z_channels=16, embed_dim=16, resolution=128, temporal_length=17).cuda()
    enc.load_reference_state_dict({n: ovae.seeded_tensor(n, s, seed=int(g["weight_seed"])) for n, s in shapes.items()})
    # the fixture's frames in [0, 1], redrawn as tools/make_golden_vae_encode.py drew them
    gen = torch.Generator().manual_seed(int(g["seed"]))
    ys = {k: torch.rand(shape, generator=gen) for k, shape in (("a", (2, 3, 17, 128, 64)), ("b", (1, 3, 1, 128, 128)))}
    return enc, g, ys


def test_encoder_vs_reference_fixture(fixture_encoder):
    enc, g, ys = fixture_encoder
    for case in ("a", "b"):
        x = (2.0 * ys[case] - 1.0).cuda()
        mom = enc._encode(x).cpu()
        ref = torch.from_numpy(g[f"moments_{case}"])
        r = rel(mom, ref)
        print(f"VideoVAE encode, case {case} {tuple(x.shape)} -> {tuple(mom.shape)}: moments rel-L2 vs the reference fixture {r:.3e}, "
              f"max_abs {(mom - ref).abs().max().item():.3e}")
        assert mom.shape == ref.shape and torch.isfinite(mom).all() and r <= 2e-2
    post = enc.encode((2.0 * ys["a"] - 1.0).cuda())
    eps = torch.from_numpy(g["eps_a"])
    smp = post.sample(noise=eps.cuda()).cpu()
    r = rel(smp, torch.from_numpy(g["sample_a"]))
    print(f"VideoVAE sample(noise = fixture eps): rel-L2 vs the reference sample {r:.3e}")
    assert smp.shape == (2, 16, 5, 16, 8) and r <= 2e-2
    assert torch.equal(post.mode(), post.mean) and post.mean.shape == post.logvar.shape == post.std.shape == (2, 16, 5, 16, 8)
    assert rel(post.std, torch.exp(0.5 * post.logvar)) <= 1e-6
    gen = torch.Generator(device="cuda").manual_seed(3)
    s1 = post.sample(generator=gen)
    assert s1.shape == (2, 16, 5, 16, 8) and torch.isfinite(s1).all()


def test_encode_videos_convention(fixture_encoder):
    import dfot_amd
    enc, g, ys = fixture_encoder
    videos = ys["a"].cuda().permute(0, 2, 1, 3, 4)                            # b t c h w in [0, 1] (a strided view: read in place)
    noise = torch.from_numpy(g["eps_a"]).permute(0, 2, 1, 3, 4).contiguous().cuda()
    two = dfot_amd.encode_videos(enc, videos, vae_batch_size=2, noise=noise)
    one = dfot_amd.encode_videos(enc, videos, vae_batch_size=1, noise=noise)
    assert two.shape == (2, 5, 16, 16, 8)
    r = rel(one, two)
    print(f"encode_videos vae_batch_size 1 vs 2: rel-L2 {r:.2e}")
    assert r <= 1e-6
    ref = torch.from_numpy(g["sample_a"]).permute(0, 2, 1, 3, 4)
    assert rel(two.cpu(), ref) <= 2e-2
    mean = [-0.284, 0.016, -0.728, -0.138, 0.941, -2.504, 0.147, -0.062, 0.833, 0.151, -0.627, 0.269, 0.268, -0.732, -1.598, 0.199]
    std = [5.591, 5.257, 7.033, 6.401, 6.091, 11.233, 5.608, 7.5, 5.277, 5.46, 5.179, 6.8, 5.474, 5.111, 7.078, 5.024]
    normed = dfot_amd.encode_videos(enc, videos, noise=noise, data_mean=mean, data_std=std)
    assert rel(normed, dfot_amd.DFoTVideoSampler._normalize_x(None, two, mean, std)) <= 1e-6
    mode = dfot_amd.encode_videos(enc, videos, sample=False)
    assert rel(mode, enc.encode((2.0 * ys["a"] - 1.0).cuda()).mean.permute(0, 2, 1, 3, 4)) <= 1e-5


def test_encode_videos_k600_geometry():
    import dfot_amd
    enc = dfot_amd.VideoVAEEncoder(z_channels=16, embed_dim=16, resolution=128, temporal_length=17).cuda()
    enc.init_random(seed=4)
    gen = torch.Generator(device="cuda").manual_seed(11)
    videos = torch.rand(2, 17, 3, 128, 128, device="cuda", generator=gen)
    noise = torch.randn(2, 5, 16, 16, 16, device="cuda", generator=gen)
    a = dfot_amd.encode_videos(enc, videos, noise=noise)
    b = dfot_amd.encode_videos(enc, videos, noise=noise)
    assert a.shape == (2, 5, 16, 16, 16) and torch.isfinite(a).all()
    assert torch.equal(a, b)
    # one video at a time == both together: no GroupNorm statistics leak across videos (or frames)
    singles = torch.cat([dfot_amd.encode_videos(enc, videos[i:i + 1], noise=noise[i:i + 1]) for i in range(2)])
    r = rel(singles, a)
    print(f"K600 geometry: one-at-a-time vs batched rel-L2 {r:.2e}")
    assert r <= 1e-6
