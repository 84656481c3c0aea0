"""Op-level GPU tests of dfot_op_attention_frame_causal (csrc/attention_frame_causal.hip): flash attention under the block-lower-triangular
mask of the DiT1D backbone -- query i sees key j iff j // L <= i // L -- in launch_attention_padded's layout.

Reference: an fp64 masked softmax on the bf16 operands the kernel reads (q carries log2(e)/sqrt(d): softmax in base 2).  Bar: rel-L2 <
1.5e-2, the bar of test_attention_temporal_vs_fp64 (tests/test_gpu_dit_fac.py) and test_attention_padded: bf16 probabilities and a bf16
output.  The mask must also be in the right place: at every shape the result is farther than 5 bars from the UNMASKED fp64 softmax.
Causality, batch independence and repeatability are bit-for-bit.  Every test fails on the parent commit, where the symbol does not exist."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BAR = 1.5e-2
BATCH, HEADS = 2, 2
# (L, T, d): every frame length once, every head dim once at (32, 8); N = 128 (one query tile) to 512 (four)
SHAPES = [(32, 4, 64), (32, 8, 32), (32, 8, 64), (32, 8, 72), (32, 8, 128), (16, 16, 64), (64, 4, 72), (128, 2, 32), (32, 16, 72)]


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def operands(batch, heads, n, d, seed=0, score_scale=1.5):
    """q, k, v as the QKV epilogue leaves them: [batch][heads][n][dstride] bf16, q in the exp2 domain, pad columns zero"""
    g = torch.Generator().manual_seed(seed + 1000 * n + 10 * heads + d)
    q, k, v = (torch.randn(batch, heads, n, d, generator=g) for _ in range(3))
    ds = 64 if d <= 64 else 128

    def pad(t, mul=1.0):
        out = torch.zeros(batch, heads, n, ds, dtype=torch.bfloat16, device="cuda")
        out[..., :d] = (t * mul).to(torch.bfloat16).cuda()
        return out
    return pad(q, score_scale * math.log2(math.e) / math.sqrt(d)), pad(k), pad(v)


def run(dev, n, frame_len, d, o=None, ldo=None):
    from dfot_amd import capi
    batch, heads = dev[0].shape[:2]
    ldo = heads * d if ldo is None else ldo
    if o is None:
        o = torch.full((batch * n, ldo), float("nan"), dtype=torch.bfloat16, device="cuda")
    capi.check(capi.lib.dfot_op_attention_frame_causal(capi.ptr(dev[0]), capi.ptr(dev[1]), capi.ptr(dev[2]), capi.ptr(o), ldo, batch, heads, n,
                                                       frame_len, d, capi.stream_ptr()))
    torch.cuda.synchronize()
    return o


def reference(dev, n, frame_len, d, masked=True):
    batch, heads = dev[0].shape[:2]
    q, k, v = (t[..., :d].double().cpu() for t in dev)
    s = q @ k.transpose(-1, -2) * math.log(2.0)  # 2^s / sum 2^s
    if masked:
        f = torch.arange(n) // frame_len
        s = s.masked_fill(f[None, :] > f[:, None], float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(batch * n, heads * d)


@pytest.mark.parametrize("L,T,d", SHAPES)
def test_vs_fp64_masked_softmax_and_mask_placement(L, T, d):
    n = L * T
    dev = operands(BATCH, HEADS, n, d)
    got = run(dev, n, L, d).float().cpu()
    assert torch.isfinite(got).all()
    r = rel(got, reference(dev, n, L, d))
    far = rel(got, reference(dev, n, L, d, masked=False))
    print(f"attention_frame_causal L={L} T={T} d={d}: rel-L2 vs the masked fp64 softmax {r:.2e}, vs the unmasked one {far:.2e}")
    assert r < BAR
    assert far > 5 * BAR


@pytest.mark.parametrize("L,T,d", [(32, 8, 72), (16, 16, 64), (64, 4, 32)])
def test_causality_bit_for_bit(L, T, d):
    """whatever frames > f hold -- large finite keys and values, other queries -- frames <= f keep their bits, for every f.  At L = 16 a
    wave's 32 query rows are two frames, so a decision taken per wave instead of per row (the deferred rescale) would show here"""
    n = L * T
    dev = operands(BATCH, HEADS, n, d, seed=1)
    base = run(dev, n, L, d).view(BATCH, T, L, -1)
    for f in range(T - 1):
        moved = [t.clone() for t in dev]
        sign = torch.where(torch.arange(n - (f + 1) * L, device="cuda") % 2 == 0, 1.0, -1.0).view(1, 1, -1, 1)
        moved[1][:, :, (f + 1) * L:, :d] = (1e4 * sign).to(torch.bfloat16)
        moved[2][:, :, (f + 1) * L:, :d] = (-1e4 * sign).to(torch.bfloat16)
        moved[0][:, :, (f + 1) * L:, :d] = (moved[0][:, :, (f + 1) * L:, :d].float() * -1.5 + 0.25).to(torch.bfloat16)
        out = run(moved, n, L, d).view(BATCH, T, L, -1)
        assert torch.equal(out[:, : f + 1], base[:, : f + 1]), f
        assert not torch.equal(out[:, f + 1:], base[:, f + 1:]), f


@pytest.mark.parametrize("L,T,d", [(32, 8, 72), (16, 16, 64)])
def test_batch_independence_and_repeatability(L, T, d):
    n = L * T
    dev = operands(3, HEADS, n, d, seed=2)
    full = run(dev, n, L, d)
    again = run(dev, n, L, d)
    assert torch.equal(full, again)
    alone = run([t[1:2].contiguous() for t in dev], n, L, d)
    assert torch.equal(alone, full.view(3, n, -1)[1])


def test_only_the_live_columns_are_written():
    """d = 72 with ldo wider than heads * d and the whole output NaN beforehand: the pad region keeps its NaN bits"""
    L, T, d = 32, 8, 72
    n, ldo = L * T, HEADS * 72 + 24
    dev = operands(BATCH, HEADS, n, d, seed=3)
    o = torch.full((BATCH * n, ldo), float("nan"), dtype=torch.bfloat16, device="cuda")
    before = o.clone()
    got = run(dev, n, L, d, o=o, ldo=ldo)
    assert torch.isfinite(got[:, : HEADS * d].float()).all()
    assert torch.equal(got[:, HEADS * d:].view(torch.int16), before[:, HEADS * d:].view(torch.int16))
    assert rel(got[:, : HEADS * d].float().cpu(), reference(dev, n, L, d)) < BAR
