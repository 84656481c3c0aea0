"""Op-level GPU tests of dfot_op_attention_seq64 (csrc/attention_seq64.hip): attention over sequences of exactly 64 tokens in the DiT
layout, the per-frame spatial attention of FacDiT / FacMatDiT at 64 patches per frame.

Reference: an fp64 softmax on the bf16 operands the kernel reads (q carries log2(e)/sqrt(d): softmax in base 2).  Bar: rel-L2 < 1.5e-2,
the bar of test_attention_padded (tests/test_gpu_dit.py:88) and of the temporal op (tests/test_gpu_dit_fac.py:80): bf16 probabilities and
a bf16 output.  Every test fails on the parent commit, where the symbol does not exist."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BAR = 1.5e-2
HEAD_DIMS = [32, 64, 72, 128]
LAUNCHES = [(1, 1), (3, 2), (5, 4), (32, 12)]  # (nseq, heads): odd counts, and several workgroup rounds (384 workgroups of 2 waves)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def operands(nseq, heads, d, seed=0, key_scale=None):
    """q, k, v as the per-frame QKV epilogue leaves them: [nseq][heads][64][dstride] bf16, q in the exp2 domain, pad columns zero; every
    buffer ends with its last sequence (no slack)"""
    g = torch.Generator().manual_seed(seed + 1000 * nseq + 10 * heads + d)
    q, k, v = (torch.randn(nseq, heads, 64, d, generator=g) for _ in range(3))
    if key_scale is not None:
        k = k * key_scale.view(1, 1, 64, 1)
    ds = 64 if d <= 64 else 128

    def pad(t, mul=1.0):
        out = torch.zeros(nseq, heads, 64, ds, dtype=torch.bfloat16, device="cuda")
        out[..., :d] = (t * mul).to(torch.bfloat16).cuda()
        return out
    return pad(q, math.log2(math.e) / math.sqrt(d)), pad(k), pad(v)


def run(dev, nseq, heads, d, o=None, ldo=None):
    from dfot_amd import capi
    ldo = heads * d if ldo is None else ldo
    if o is None:
        o = torch.full((nseq * 64, ldo), float("nan"), dtype=torch.bfloat16, device="cuda")
    capi.check(capi.lib.dfot_op_attention_seq64(capi.ptr(dev[0]), capi.ptr(dev[1]), capi.ptr(dev[2]), capi.ptr(o), ldo, nseq, heads, d,
                                                capi.stream_ptr()))
    torch.cuda.synchronize()
    return o


def reference(dev, nseq, heads, d):
    q, k, v = (t[..., :d].double().cpu() for t in dev)
    w = torch.softmax(q @ k.transpose(-1, -2) * math.log(2.0), -1)  # 2^s / sum 2^s
    return (w @ v).transpose(1, 2).reshape(nseq * 64, heads * d)


@pytest.mark.parametrize("d", HEAD_DIMS)
def test_vs_fp64_softmax(d):
    for nseq, heads in LAUNCHES:
        dev = operands(nseq, heads, d)
        got = run(dev, nseq, heads, d).float().cpu()
        assert torch.isfinite(got).all()
        r = rel(got, reference(dev, nseq, heads, d))
        print(f"attention_seq64 d={d} nseq={nseq} heads={heads}: rel-L2 {r:.2e}")
        assert r < BAR


@pytest.mark.parametrize("d", HEAD_DIMS)
def test_large_scores(d):
    """keys scaled by linspace(0.5, 6) along the key axis (as test_attention_d128_rows_large_launches): scores of several tens in the log2
    domain, which overflow 2^s without the row-max subtraction"""
    nseq, heads = 5, 4
    dev = operands(nseq, heads, d, seed=1, key_scale=torch.linspace(0.5, 6.0, 64))
    smax = float((dev[0][..., :d].float() @ dev[1][..., :d].float().transpose(-1, -2)).abs().max())
    got = run(dev, nseq, heads, d).float().cpu()
    assert torch.isfinite(got).all()
    r = rel(got, reference(dev, nseq, heads, d))
    print(f"attention_seq64 d={d}, large scores (max |s| = {smax:.1f} in the log2 domain): rel-L2 {r:.2e}")
    assert smax > 16.0
    assert r < BAR


@pytest.mark.parametrize("d,nseq,heads", [(32, 5, 4), (64, 4, 2), (72, 3, 2), (128, 5, 1)])
def test_sequences_are_independent(d, nseq, heads):
    """perturbing q, k, v of ONE sequence (all heads) leaves every other sequence's output rows bitwise unchanged; the last sequence run
    alone gives the bits it gives inside the batch"""
    dev = operands(nseq, heads, d, seed=2)
    base = run(dev, nseq, heads, d).reshape(nseq, 64, -1)
    s = nseq // 2
    dev2 = [t.clone() for t in dev]
    for t in dev2:
        t[s, :, :, :d] = (t[s, :, :, :d].float() * -1.5 + 0.25).to(torch.bfloat16)
    moved = run(dev2, nseq, heads, d).reshape(nseq, 64, -1)
    keep = [i for i in range(nseq) if i != s]
    assert torch.equal(base[keep], moved[keep])
    assert not torch.equal(base[s], moved[s])
    last = [t[nseq - 1:].clone() for t in dev]
    alone = run(last, 1, heads, d).reshape(1, 64, -1)
    assert torch.equal(alone[0], base[nseq - 1])


def test_only_the_live_columns_are_written():
    """d = 72 (rows of 128 elements, products over 80 / 96 columns): with ldo wider than heads * d and the whole output NaN beforehand, the
    d live columns of every head are finite and every other column keeps its NaN bits"""
    nseq, heads, d, ldo = 3, 2, 72, 2 * 72 + 24
    dev = operands(nseq, heads, d, seed=3)
    o = torch.full((nseq * 64, ldo), float("nan"), dtype=torch.bfloat16, device="cuda")
    before = o.clone()
    got = run(dev, nseq, heads, d, o=o, ldo=ldo)
    assert torch.isfinite(got[:, : heads * d].float()).all()
    assert torch.equal(got[:, heads * d:].view(torch.int16), before[:, heads * d:].view(torch.int16))
    assert rel(got[:, : heads * d].float().cpu(), reference(dev, nseq, heads, d)) < BAR
    # a neighbouring head's columns: head 0 alone, written into a buffer that holds NaN where head 1 would go
    one = [t[:, :1].contiguous() for t in dev]
    o1 = torch.full((nseq * 64, 2 * d), float("nan"), dtype=torch.bfloat16, device="cuda")
    got1 = run(one, nseq, 1, d, o=o1, ldo=2 * d)
    assert torch.equal(got1[:, :d], got[:, :d])
    assert torch.isnan(got1[:, d:].float()).all()


def test_invalid_shapes_launch_nothing():
    from dfot_amd import capi
    nseq, heads, d = 2, 2, 64
    dev = operands(nseq, heads, d, seed=4)
    o = torch.full((nseq * 64, heads * d), 3.0, dtype=torch.bfloat16, device="cuda")
    before = o.clone()
    P = capi.ptr

    def call(q, k, v, out, ldo, nseq, heads, d):
        return capi.lib.dfot_op_attention_seq64(q, k, v, out, ldo, nseq, heads, d, capi.stream_ptr())
    ok = (P(dev[0]), P(dev[1]), P(dev[2]), P(o))
    for hd in (0, 4, 136):
        assert call(*ok, 128, nseq, heads, hd) == capi.ERR_SHAPE, hd
        assert capi.lib.dfot_last_error()
    for args in ((128, 0, heads, d), (128, nseq, 0, d), (heads * d - 8, nseq, heads, d), (heads * d + 4, nseq, heads, d)):
        assert call(*ok, *args) == capi.ERR_SHAPE, args
        assert capi.lib.dfot_last_error()
    for i in range(4):
        ptrs = list(ok)
        ptrs[i] = None
        assert call(*ptrs, heads * d, nseq, heads, d) == capi.ERR_ARG, i
        assert capi.lib.dfot_last_error()
    torch.cuda.synchronize()
    assert torch.equal(o, before)
    assert call(*ok, heads * d, nseq, heads, d) == capi.OK  # the same buffers at a valid shape do launch
    torch.cuda.synchronize()
    assert not torch.equal(o, before)
