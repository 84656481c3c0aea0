"""GPU parity tests of the C-ABI primitives against plain PyTorch fp32 references / the CPU oracle.
Tolerances: bf16 inputs are exact in both paths (the reference consumes the same bf16-rounded values),
so GEMM/conv/attention differ only by fp32 accumulation order (+ bf16 rounding of P in attention)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import dfot_amd  # noqa: F401
    from dfot_amd import capi as c
    assert torch.cuda.is_available()
    return c


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr())


def report(name, got, ref):
    err = (got - ref).abs().max().item()
    rel = ((got - ref).norm() / ref.norm().clamp_min(1e-12)).item()
    print(f"{name}: max_abs={err:.3e} rel_l2={rel:.3e}")
    return err, rel


@pytest.mark.parametrize("dma", [0, 1, 4, 8, 9, 10, 14])
@pytest.mark.parametrize("m,n,k", [(256, 128, 64), (256, 192, 128), (1024, 576, 576), (256, 4032, 576), (768, 100, 2880),
                                   (512, 256, 192), (512, 1152, 1152)])
def test_gemm(capi, dma, m, n, k):
    g = torch.Generator().manual_seed(m + n + k)
    a = torch.randn(m, k, generator=g).bfloat16().cuda()
    w = (torch.randn(n, k, generator=g) / math.sqrt(k)).bfloat16().cuda()
    bias = torch.randn(n, generator=g).cuda()
    out = torch.full((m, n), float("nan"), device="cuda")
    capi.check(capi.lib.dfot_op_gemm(P(a), k, P(w), P(bias), P(out), m, n, k, dma, S()))
    ref = a.float() @ w.float().t() + bias
    err, rel = report(f"gemm dma={dma} {m}x{n}x{k}", out, ref)
    assert torch.isfinite(out).all()
    assert rel < 1e-5 and err < 1e-3


def test_gemm_auto_pick_at_a_ring_shape(capi):
    """M = 16384, N = 1152, K = 5760 (level-3 out-projection at model batch 8, the training dgrad shapes): the shape picker takes the
    three-stage 256x144 ring here (512 tiles = two full rounds; gemm_pick_variant) -- checked against an fp32 matmul on the GPU"""
    m, n, k = 16384, 1152, 5760
    g = torch.Generator().manual_seed(5)
    a = torch.randn(m, k, generator=g).bfloat16().cuda()
    w = (torch.randn(n, k, generator=g) / math.sqrt(k)).bfloat16().cuda()
    bias = torch.randn(n, generator=g).cuda()
    out = torch.full((m, n), float("nan"), device="cuda")
    capi.check(capi.lib.dfot_op_gemm(P(a), k, P(w), P(bias), P(out), m, n, k, -1, S()))
    ref = a.float() @ w.float().t() + bias
    err, rel = report(f"gemm auto {m}x{n}x{k}", out, ref)
    assert torch.isfinite(out).all() and rel < 1e-5 and err < 2e-3


@pytest.mark.parametrize("m,n,k", [(512, 128, 192), (1024, 100, 640)])
def test_gemm_512_row_tile(capi, m, n, k):
    g = torch.Generator().manual_seed(m + n + k)
    a = torch.randn(m, k, generator=g).bfloat16().cuda()
    w = (torch.randn(n, k, generator=g) / math.sqrt(k)).bfloat16().cuda()
    out = torch.full((m, n), float("nan"), device="cuda")
    capi.check(capi.lib.dfot_op_gemm(P(a), k, P(w), None, P(out), m, n, k, 6, S()))
    ref = a.float() @ w.float().t()
    err, rel = report(f"gemm 512x128 {m}x{n}x{k}", out, ref)
    assert rel < 1e-5 and err < 1e-3


def test_gemm_rejects_bad_shapes(capi):
    a = torch.zeros(100, 64, device="cuda", dtype=torch.bfloat16)
    out = torch.zeros(100, 64, device="cuda")
    with pytest.raises(capi.DfotError):
        capi.check(capi.lib.dfot_op_gemm(P(a), 64, P(a), None, P(out), 100, 64, 64, 1, S()))


@pytest.mark.parametrize("dma", [0, 1, 4, 8])
@pytest.mark.parametrize("bt,h,w,cin,cout", [(4, 8, 8, 128, 128), (1, 16, 16, 128, 256), (2, 8, 16, 576, 256), (4, 16, 8, 64, 100)])
def test_conv3x3(capi, dma, bt, h, w, cin, cout):
    g = torch.Generator().manual_seed(bt * 1000 + cin + cout)
    x = torch.randn(bt, cin, h, w, generator=g).bfloat16()
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)).bfloat16()
    bias = torch.randn(cout, generator=g)
    a = x.permute(0, 2, 3, 1).contiguous().cuda()                      # NHWC
    wp = wt.permute(0, 2, 3, 1).reshape(cout, 9 * cin).contiguous().cuda()  # [Cout][tap][Cin]
    out = torch.full((bt, h, w, cout), float("nan"), device="cuda")
    bd = bias.cuda()
    capi.check(capi.lib.dfot_op_conv3x3(P(a), P(wp), P(bd), P(out), bt, h, w, cin, cout, dma, S()))
    ref = F.conv2d(x.float(), wt.float(), bias, padding=1).permute(0, 2, 3, 1).cuda()
    err, rel = report(f"conv dma={dma} {bt}x{h}x{w} {cin}->{cout}", out, ref)
    assert torch.isfinite(out).all()
    assert rel < 1e-5 and err < 1e-3


@pytest.mark.parametrize("variant", [1, 0, 2, 3, 4, 5, 6, 14])
@pytest.mark.parametrize("b,heads,n,d", [(1, 2, 128, 64), (2, 9, 512, 64), (1, 3, 256, 128), (2, 9, 128, 128), (3, 5, 1024, 64), (2, 5, 512, 128)])
def test_attention(capi, variant, b, heads, n, d):
    g = torch.Generator().manual_seed(n + d + heads)
    q = torch.randn(b, heads, n, d, generator=g)
    k = torch.randn(b, heads, n, d, generator=g)
    v = torch.randn(b, heads, n, d, generator=g)
    # spike a few keys so that the running max changes mid-sequence (online-softmax rescale path)
    k[:, :, n // 2 + 3] *= 4.0
    k[:, :, n - 5] *= 6.0
    qs = (q * (math.log2(math.e) / math.sqrt(d))).bfloat16()
    kb, vb = k.bfloat16(), v.bfloat16()
    o = torch.full((b, n, heads * d), float("nan"), device="cuda", dtype=torch.bfloat16)
    qd, kd, vd = qs.cuda(), kb.cuda(), vb.cuda()  # keep the device tensors alive across the launch
    capi.check(capi.lib.dfot_op_attention(P(qd), P(kd), P(vd), P(o), heads * d, b, heads, n, d, variant, S()))
    torch.cuda.synchronize()
    s = (qs.double() @ kb.double().transpose(-1, -2)) * math.log(2.0)
    ref = (torch.softmax(s, dim=-1) @ vb.double()).permute(0, 2, 1, 3).reshape(b, n, heads * d).float()
    err, rel = report(f"attention v{variant} b{b} h{heads} n{n} d{d}", o.float().cpu(), ref)
    assert torch.isfinite(o.float()).all()
    assert rel < 1e-2 and err < 3e-2


@pytest.mark.parametrize("variant", [2, 5, 6, 14])
@pytest.mark.parametrize("b,heads,n,d", [(2, 9, 8192, 64), (2, 9, 2048, 128), (8, 9, 8192, 64), (1, 9, 8192, 64), (1, 9, 2048, 128), (4, 9, 2048, 128)])
def test_attention_production_shapes_vs_fp32_softmax(capi, variant, b, heads, n, d):
    """The launches bench.py times: level 2 = 18 (batch, head) units x N 8192 x d 64 (1152 workgroups through
    the XCD remap, 128 K/V tiles through the LDS ring), level 3 = N 2048 x d 128, and the model-batch-8 launch of the 200-frame
    plan.  Reference: fp64 softmax(QK^T)V per (batch, head) on the same bf16 q, k, v.  Bar: rel-L2 < 1e-2 (bf16 rounding of P, O)."""
    g = torch.Generator(device="cuda").manual_seed(n + d + b)
    q = torch.randn(b, heads, n, d, generator=g, device="cuda")
    k = torch.randn(b, heads, n, d, generator=g, device="cuda")
    v = torch.randn(b, heads, n, d, generator=g, device="cuda")
    k[:, :, n // 2 + 3] *= 4.0      # the running max jumps mid-sequence: deferred-rescale branch
    k[:, :, n - 5] *= 6.0
    qs = (q * (math.log2(math.e) / math.sqrt(d))).bfloat16().contiguous()
    kb, vb = k.bfloat16().contiguous(), v.bfloat16().contiguous()
    o = torch.full((b, n, heads * d), float("nan"), device="cuda", dtype=torch.bfloat16)
    if d != 64 and variant != 2:
        pytest.skip("variants 5, 6, 14 are d = 64 kernels")
    capi.check(capi.lib.dfot_op_attention(P(qs), P(kb), P(vb), P(o), heads * d, b, heads, n, d, variant, S()))
    torch.cuda.synchronize()
    assert torch.isfinite(o.float()).all()
    num = den = 0.0
    worst = 0.0
    for bi in range(b):
        for h in range(heads):
            if b > 2 and (bi * heads + h) % 7:   # the big launch: every 7th unit is enough to pin the grid mapping
                continue
            s = (qs[bi, h].double() @ kb[bi, h].double().t()) * math.log(2.0)
            ref = torch.softmax(s, dim=-1) @ vb[bi, h].double()
            got = o[bi, :, h * d:(h + 1) * d].double()
            num += (got - ref).pow(2).sum().item()
            den += ref.pow(2).sum().item()
            worst = max(worst, (got - ref).abs().max().item())
    rel = math.sqrt(num / den)
    print(f"attention production v{variant} b{b} h{heads} n{n} d{d}: rel_l2={rel:.3e} max_abs={worst:.3e}")
    assert rel < 1e-2 and worst < 3e-2


def test_ray_encode_vs_oracle(capi):
    from oracle import pose as opose
    g = np.load(os.path.join(GOLDEN, "ray_encoding.npz"))
    poses = torch.from_numpy(g["poses"])
    out = torch.empty(2, 8, 180, 8, 8, device="cuda")
    pd = poses.cuda()
    capi.check(capi.lib.dfot_ray_encode(P(pd), P(out), 2, 8, 8, S()))
    got = out.cpu()
    low = [c for c in range(180) if (c % 15) < 8]
    np.testing.assert_allclose(got[:, :, low].numpy(), g["enc8"][:, :, low], atol=2e-4)
    np.testing.assert_allclose(got.numpy(), g["enc8"], atol=3e-2)
    ref = opose.ray_encoding(poses[:1], 64)
    out = torch.empty(1, 8, 180, 64, 64, device="cuda")
    pd1 = poses[:1].contiguous().cuda()
    capi.check(capi.lib.dfot_ray_encode(P(pd1), P(out), 1, 8, 64, S()))
    np.testing.assert_allclose(out.cpu()[:, :, low].numpy(), ref[:, :, low].numpy(), atol=2e-4)


def test_sampler_step_kernels(capi):
    """dfot_hg_prepare + dfot_ddim_compose against the reference formulas in torch fp32."""
    g = torch.Generator().manual_seed(9)
    b, nfe, t, f = 2, 2, 8, 3 * 8 * 8
    x = torch.randn(b, t, f, generator=g)
    noise = torch.randn(b * nfe, t, f, generator=g)
    qa = torch.rand(b * nfe, t, generator=g)
    qb = torch.rand(b * nfe, t, generator=g)
    qb[1] = 0
    qa[1] = 1
    x_in = torch.empty(b * nfe, t, f, device="cuda")
    d = {n: v.cuda() for n, v in dict(x=x, noise=noise, qa=qa, qb=qb).items()}
    capi.check(capi.lib.dfot_hg_prepare(P(d["x"]), P(d["noise"]), P(d["qa"]), P(d["qb"]), P(x_in), b, nfe, t, f, S()))
    ref_in = qa[..., None] * x.repeat_interleave(nfe, 0) + qb[..., None] * noise
    np.testing.assert_allclose(x_in.cpu().numpy(), ref_in.numpy(), rtol=1e-6, atol=1e-6)
    v = torch.randn(b * nfe, t, f, generator=g)
    sa, s1, an, cn = (torch.rand(b * nfe, t, generator=g) for _ in range(4))
    keep = (torch.rand(b * nfe, t, generator=g) < 0.3).float()
    w = torch.tensor([-3.0, 4.0])
    gen = (torch.rand(b, t, generator=g) < 0.6)
    out = torch.empty(b, t, f, device="cuda")
    d = {n: v.cuda() for n, v in dict(x=x, xi=ref_in, v=v, sa=sa, s1=s1, an=an, cn=cn, keep=keep, w=w,
                                      gen=gen.to(torch.uint8)).items()}
    capi.check(capi.lib.dfot_ddim_compose(P(d["x"]), P(d["xi"]), P(d["v"]), P(d["sa"]), P(d["s1"]), P(d["an"]),
                                          P(d["cn"]), P(d["keep"]), P(d["w"]), P(d["gen"]), P(out), b, nfe, t, f, S()))
    e = lambda a: a[..., None]
    x0 = e(sa) * ref_in - e(s1) * v
    eps = e(sa) * v + e(s1) * ref_in
    xp = torch.where(e(keep) != 0, ref_in, x0 * e(an) + eps * e(cn))
    comp = (xp.view(b, nfe, t, f) * w.view(1, nfe, 1, 1)).sum(1)
    ref = torch.where(e(gen), comp, x)
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)
