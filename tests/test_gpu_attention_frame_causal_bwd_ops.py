"""Op-level GPU tests of dfot_op_attention_frame_causal_lse and dfot_op_attention_frame_causal_bwd (csrc/attention_frame_causal.hip,
the frame-causal instantiations of csrc/attention_bwd.hip): flash attention under the block-lower-triangular mask -- query i sees key j
iff j // L <= i // L -- with its log-sum-exp, and its backward under the contract of dfot_op_attention_bwd_lse.

Conventions of tests/test_gpu_attention_frame_causal_ops.py: B = 2, 2 heads, seeded unit-normal operands rounded to bf16, q carrying
1.5 log2(e)/sqrt(d); references in fp64 on the CPU from the bf16 values the kernels read (autograd of the masked softmax for the
gradients).  Bars are the project's own for this kernel family (tests/test_gpu_train.py, bounded-attention test; BAR of the forward test):
output rel-L2 < 1.5e-2, lse max abs error < 2e-2 in the log2 domain, each of dq, dk, dv rel-L2 < 2.5e-2.  The mask must be in the right
place: for T >= 2 every gradient is farther than 5 bars from the fp64 gradient of the UNMASKED softmax.  Causality of dq, independence of
dk / dv from earlier frames' q and d_o, batch independence and repeatability are bit-for-bit.  Every test fails on the parent commit,
where the two symbols do not exist."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BAR_O, BAR_LSE, BAR_GRAD = 1.5e-2, 2e-2, 2.5e-2
BATCH, HEADS = 2, 2
# (L, T, d): one query tile; every head-dim instantiation with its pad columns; two frames inside a wave's 32 rows; L = 64; a diagonal
# tile fully visible or fully masked per wave; a single frame (nothing masked); four query tiles
SHAPES = [(32, 4, 64), (32, 8, 32), (32, 8, 72), (32, 8, 128), (16, 16, 64), (64, 4, 72), (128, 2, 32), (128, 1, 64), (32, 16, 72)]
BITWISE_SHAPES = [(32, 8, 72), (16, 16, 64), (64, 4, 32)]


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def operands(batch, heads, n, d, seed=0, score_scale=1.5, ldo=None):
    """q, k, v as the QKV epilogue leaves them ([batch][heads][n][dstride] bf16, q in the exp2 domain, pad columns zero) and d_o compact
    [batch * n][ldo] bf16 (columns beyond heads * d zero)"""
    g = torch.Generator().manual_seed(seed + 1000 * n + 10 * heads + d)
    q, k, v = (torch.randn(batch, heads, n, d, generator=g) for _ in range(3))
    ds = 64 if d <= 64 else 128
    ldo = heads * d if ldo is None else ldo

    def pad(t, mul=1.0):
        out = torch.zeros(batch, heads, n, ds, dtype=torch.bfloat16, device="cuda")
        out[..., :d] = (t * mul).to(torch.bfloat16).cuda()
        return out
    d_o = torch.zeros(batch * n, ldo, dtype=torch.bfloat16, device="cuda")
    d_o[:, : heads * d] = torch.randn(batch * n, heads * d, generator=g).to(torch.bfloat16).cuda()
    return pad(q, score_scale * math.log2(math.e) / math.sqrt(d)), pad(k), pad(v), d_o


def forward(dev, n, frame_len, d, ldo=None):
    """dfot_op_attention_frame_causal_lse on NaN-filled outputs -> (o compact bf16, lse fp32)"""
    from dfot_amd import capi
    batch, heads = dev[0].shape[:2]
    ldo = heads * d if ldo is None else ldo
    o = torch.full((batch * n, ldo), float("nan"), dtype=torch.bfloat16, device="cuda")
    lse = torch.full((batch, heads, n), float("nan"), dtype=torch.float32, device="cuda")
    capi.check(capi.lib.dfot_op_attention_frame_causal_lse(capi.ptr(dev[0]), capi.ptr(dev[1]), capi.ptr(dev[2]), capi.ptr(o), ldo,
                                                           capi.ptr(lse), batch, heads, n, frame_len, d, capi.stream_ptr()))
    torch.cuda.synchronize()
    return o, lse


def backward(dev, o, lse, n, frame_len, d, ldo=None):
    """dfot_op_attention_frame_causal_bwd on NaN-filled outputs -> (dq, dk, dv) [batch][heads][n][dstride] bf16"""
    from dfot_amd import capi
    batch, heads = dev[0].shape[:2]
    ldo = heads * d if ldo is None else ldo
    delta = torch.full((batch, heads, n), float("nan"), dtype=torch.float32, device="cuda")
    dq, dk, dv = (torch.full_like(dev[0], float("nan")) for _ in range(3))
    capi.check(capi.lib.dfot_op_attention_frame_causal_bwd(capi.ptr(dev[0]), capi.ptr(dev[1]), capi.ptr(dev[2]), capi.ptr(o), capi.ptr(dev[3]),
                                                           ldo, capi.ptr(lse), capi.ptr(delta), capi.ptr(dq), capi.ptr(dk), capi.ptr(dv), batch,
                                                           heads, n, frame_len, d, capi.stream_ptr()))
    torch.cuda.synchronize()
    return dq, dk, dv


def run(dev, n, frame_len, d):
    o, lse = forward(dev, n, frame_len, d)
    return (o, lse) + backward(dev, o, lse, n, frame_len, d)


def reference(dev, n, frame_len, d, masked=True):
    """fp64 on the CPU from the bf16 operands: (o [batch * n][heads * d], lse in the log2 domain, dq, dk, dv [batch][heads][n][d]) under the
    kernels' contract -- dq is the gradient of the UNSCALED q (the operand divided by log2(e)/sqrt(d)), dk and dv those of k and v"""
    batch, heads = dev[0].shape[:2]
    scale = math.log2(math.e) / math.sqrt(d)
    q = (dev[0][..., :d].double().cpu() / scale).requires_grad_()
    k, v = (t[..., :d].double().cpu().requires_grad_() for t in dev[1:3])
    s = q @ k.transpose(-1, -2) / math.sqrt(d)
    if masked:
        f = torch.arange(n) // frame_len
        s = s.masked_fill(f[None, :] > f[:, None], float("-inf"))
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(batch * n, heads * d)
    o.backward(dev[3][:, : heads * d].double().cpu())
    return o.detach(), torch.logsumexp(s.detach(), -1) / math.log(2.0), q.grad, k.grad, v.grad


@functools.lru_cache(maxsize=None)
def case(L, T, d):
    """operands, the kernels' results and both fp64 references of one shape, computed once and shared (nothing below modifies them)"""
    n = L * T
    dev = operands(BATCH, HEADS, n, d)
    return dev, run(dev, n, L, d), reference(dev, n, L, d), reference(dev, n, L, d, masked=False)


@pytest.mark.parametrize("L,T,d", SHAPES)
def test_lse_forward_has_the_inference_bits_and_the_fp64_log_sum_exp(L, T, d):
    from dfot_amd import capi
    n = L * T
    dev, (o, lse, *_), (ref_o, ref_lse, *_), _ = case(L, T, d)
    plain = torch.full_like(o, float("nan"))
    capi.check(capi.lib.dfot_op_attention_frame_causal(capi.ptr(dev[0]), capi.ptr(dev[1]), capi.ptr(dev[2]), capi.ptr(plain), HEADS * d, BATCH,
                                                       HEADS, n, L, d, capi.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(o.view(torch.int16), plain.view(torch.int16))
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    r, e = rel(o.float().cpu(), ref_o), float((lse.double().cpu() - ref_lse).abs().max())
    print(f"attention_frame_causal_lse L={L} T={T} d={d}: o rel-L2 {r:.2e}, lse max abs error {e:.2e}")
    assert r < BAR_O
    assert e < BAR_LSE


@pytest.mark.parametrize("L,T,d", SHAPES)
def test_backward_vs_fp64_autograd_and_mask_placement(L, T, d):
    dev, (_, _, *got), (_, _, *want), (_, _, *unmasked) = case(L, T, d)
    ds = dev[0].shape[-1]
    for name, g, w, u in zip(("dq", "dk", "dv"), got, want, unmasked):
        g = g.float().cpu()
        assert torch.isfinite(g).all(), name
        assert not g[..., d:].any(), name  # the pad columns are written as zero
        r, far = rel(g[..., :d], w), rel(g[..., :d], u)
        print(f"attention_frame_causal_bwd L={L} T={T} d={d} (dstride {ds}) {name}: rel-L2 vs the masked fp64 autograd {r:.2e}, vs the "
              f"unmasked one {far:.2e}")
        assert r < BAR_GRAD, name
        if T >= 2:
            assert far > 5 * BAR_GRAD, name
        else:  # a single frame: nothing is masked, and the result is the unmasked gradient
            assert far < BAR_GRAD, name


def frames(t, T):
    """[batch][heads][n][c] -> [batch][heads][T][L * c]"""
    return t.reshape(t.shape[0], t.shape[1], T, -1)


@pytest.mark.parametrize("L,T,d", BITWISE_SHAPES)
def test_dq_causality_bit_for_bit(L, T, d):
    """whatever frames > f hold -- large finite keys and values, other queries, other d_o -- dq of frames <= f keeps its bits, for every
    f, and dq of the later frames does not.  At L = 16 a wave's 32 query rows are two frames"""
    n = L * T
    dev = operands(BATCH, HEADS, n, d, seed=1)
    base = frames(run(dev, n, L, d)[2], T)
    for f in range(T - 1):
        moved = [t.clone() for t in dev]
        cut = (f + 1) * L
        sign = torch.where(torch.arange(n - cut, device="cuda") % 2 == 0, 1.0, -1.0).view(1, 1, -1, 1)
        moved[1][:, :, cut:, :d] = (1e4 * sign).to(torch.bfloat16)
        moved[2][:, :, cut:, :d] = (-1e4 * sign).to(torch.bfloat16)
        moved[0][:, :, cut:, :d] = (moved[0][:, :, cut:, :d].float() * -1.5 + 0.25).to(torch.bfloat16)
        rows = moved[3].view(BATCH, n, -1)
        rows[:, cut:] = (100.0 * sign.view(1, -1, 1)).to(torch.bfloat16)
        dq = frames(run(moved, n, L, d)[2], T)
        assert torch.equal(dq[:, :, : f + 1], base[:, :, : f + 1]), f
        assert not torch.equal(dq[:, :, f + 1:], base[:, :, f + 1:]), f


@pytest.mark.parametrize("L,T,d", BITWISE_SHAPES)
def test_dk_dv_do_not_depend_on_earlier_frames_queries_bit_for_bit(L, T, d):
    """the keys of frames >= f are seen by the queries of frames >= f only, whose lse, o and delta do not depend on q and d_o of frames
    < f; inside a diagonal tile the replaced rows are selected away.  So dk and dv of frames >= f keep their bits when q and d_o of the
    earlier frames change, and dk / dv of the earlier frames change"""
    n = L * T
    dev = operands(BATCH, HEADS, n, d, seed=2)
    base = [frames(t, T) for t in run(dev, n, L, d)[3:]]
    for f in range(1, T):
        moved = [t.clone() for t in dev]
        cut = f * L
        moved[0][:, :, :cut, :d] = (moved[0][:, :, :cut, :d].float() * -1.5 + 0.25).to(torch.bfloat16)
        sign = torch.where(torch.arange(cut, device="cuda") % 2 == 0, 1.0, -1.0).view(1, -1, 1)
        moved[3].view(BATCH, n, -1)[:, :cut] = (100.0 * sign).to(torch.bfloat16)
        for name, got, want in zip(("dk", "dv"), run(moved, n, L, d)[3:], base):
            got = frames(got, T)
            assert torch.isfinite(got.float()).all(), (name, f)
            assert torch.equal(got[:, :, f:], want[:, :, f:]), (name, f)
            assert not torch.equal(got[:, :, :f], want[:, :, :f]), (name, f)


@pytest.mark.parametrize("L,T,d", [(32, 8, 72), (16, 16, 64)])
def test_batch_independence_and_repeatability(L, T, d):
    n = L * T
    dev = operands(3, HEADS, n, d, seed=3)
    full, again = run(dev, n, L, d), run(dev, n, L, d)
    for a, b in zip(full, again):  # o, lse, dq, dk, dv
        assert torch.equal(a, b)
    mid = [t[1:2].contiguous() for t in dev[:3]] + [dev[3].view(3, n, -1)[1].contiguous()]
    alone = run(mid, n, L, d)
    assert torch.equal(alone[1], full[1][1:2])  # lse
    for a, b in zip(alone[2:], full[2:]):       # dq, dk, dv
        assert torch.equal(a, b[1:2])


def test_nothing_beyond_the_live_columns_of_o_and_d_o_is_read():
    """d = 72 with a row stride wider than heads * d: NaN in the columns of o and d_o beyond heads * d reaches neither delta nor a gradient"""
    L, T, d = 32, 8, 72
    n, ldo = L * T, HEADS * 72 + 24
    dev = operands(BATCH, HEADS, n, d, seed=4, ldo=ldo)
    o, lse = forward(dev, n, L, d, ldo=ldo)
    assert torch.isnan(o[:, HEADS * d:].float()).all()  # the forward left its NaN fill there
    dev[3][:, HEADS * d:] = float("nan")
    got = backward(dev, o, lse, n, L, d, ldo=ldo)
    want = reference(dev, n, L, d)[2:]
    for name, g, w in zip(("dq", "dk", "dv"), got, want):
        assert torch.isfinite(g.float()).all(), name
        assert rel(g[..., :d].float().cpu(), w) < BAR_GRAD, name
