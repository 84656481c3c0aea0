"""GPU tests of the differentiable operator dfot_amd.attention_seq64 (ops.py: dfot::attention_seq64), the drop-in for the
F.scaled_dot_product_attention(q, k, v) that the reference's spatial DiTBlock issues per frame at 64 patches per frame.

Inputs (F, heads, 64, d); forward and the three input gradients of (o * w).sum() for a seeded w against fp64 softmax(q k^T / sqrt(d)) v on
the same input values, with the bars of tests/test_gpu_frame_causal_attention_autograd.py, whose docstring derives them (output rel-L2
< 1.5e-2, gradients < 2.5e-2: on top of the kernels' roundings the wrapper rounds q log2(e)/sqrt(d) to bf16, and for fp32 inputs k, v and
d_o as well).  fp32 inputs return fp32 output and gradients.  A non-contiguous q gives the bits of its contiguous copy; two backward passes
from one forward give equal bits; autograd through the operator gives the bits of a direct call of the two C entries on the packed
operands.  Every test fails on the parent commit, where the operator does not exist."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BAR_O, BAR_GRAD = 1.5e-2, 2.5e-2
FRAMES, HEADS = 3, 2
HEAD_DIMS = [64, 72, 128]


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def inputs(d, dtype, seed=0):
    """q, k, v, w (F, heads, 64, d): unit-normal values of `dtype`, q times 1.5 (scores of the op-level tests)"""
    g = torch.Generator().manual_seed(seed + 1000 * FRAMES + d)
    q, k, v, w = (torch.randn(FRAMES, HEADS, 64, d, generator=g) for _ in range(4))
    return tuple(t.to(dtype).cuda() for t in (1.5 * q, k, v, w))


def reference(q, k, v, w):
    """fp64 on the CPU from the values the operator was given -> (o, dq, dk, dv)"""
    q, k, v = (t.double().cpu().requires_grad_() for t in (q, k, v))
    o = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(q.shape[3]), -1) @ v
    (o * w.double().cpu()).sum().backward()
    return o.detach(), q.grad, k.grad, v.grad


def run(q, k, v, w):
    import dfot_amd
    q, k, v = (t.detach().requires_grad_() for t in (q, k, v))
    o = dfot_amd.attention_seq64(q, k, v)
    (o * w).sum().backward()
    torch.cuda.synchronize()
    return o.detach(), q.grad, k.grad, v.grad


@functools.lru_cache(maxsize=None)
def case(d, dtype):
    x = inputs(d, dtype)
    return x, run(*x), reference(*x)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_forward_and_input_gradients_vs_fp64(d, dtype):
    x, got, want = case(d, dtype)
    for name, g, r, bar in zip(("o", "dq", "dk", "dv"), got, want, (BAR_O, BAR_GRAD, BAR_GRAD, BAR_GRAD)):
        assert g.shape == x[0].shape and g.dtype == dtype, name
        assert torch.isfinite(g.float()).all(), name
        e = rel(g.float().cpu(), r)
        print(f"attention_seq64 {dtype} d={d} {name}: rel-L2 vs fp64 {e:.2e}")
        assert e < bar, name


@pytest.mark.parametrize("d", HEAD_DIMS)
def test_autograd_equals_a_direct_call_of_the_two_c_entries(d):
    """o.transpose(1, 2).reshape(F, 64, heads * d) is a view of the kernel's compact buffer; o and the gradients hold the bits that
    dfot_op_attention_seq64 and dfot_op_attention_seq64_bwd write for the packed operands"""
    from dfot_amd import capi, ops
    x, got, _ = case(d, torch.bfloat16)
    q, k, v, w = x
    o = got[0]
    assert o.transpose(1, 2).is_contiguous()
    P, ds = capi.ptr, 64 if d <= 64 else 128
    qp, kp, vp = ops._fc_pack(q, d, math.log2(math.e) / math.sqrt(d)), ops._fc_pack(k, d), ops._fc_pack(v, d)
    assert qp.shape == (FRAMES, HEADS, 64, ds) and not qp[..., d:].any()
    direct = torch.full((FRAMES * 64, HEADS * d), float("nan"), dtype=torch.bfloat16, device="cuda")
    capi.check(capi.lib.dfot_op_attention_seq64(P(qp), P(kp), P(vp), P(direct), HEADS * d, FRAMES, HEADS, d, capi.stream_ptr()))
    d_o = w.transpose(1, 2).contiguous().view(FRAMES * 64, HEADS * d)  # the gradient of (o * w).sum() w.r.t. o, compact
    grads = [torch.full((FRAMES, HEADS, 64, ds), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    capi.check(capi.lib.dfot_op_attention_seq64_bwd(P(qp), P(kp), P(vp), P(d_o), HEADS * d, P(grads[0]), P(grads[1]), P(grads[2]), FRAMES, HEADS,
                                                    d, capi.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(o.transpose(1, 2).reshape(FRAMES * 64, HEADS * d), direct)
    for g, want in zip(got[1:], grads):
        assert torch.equal(g, want[..., :d])


def test_non_contiguous_q_gives_the_bits_of_its_contiguous_copy():
    d = 72
    q, k, v, w = inputs(d, torch.bfloat16, seed=1)
    qt = q.transpose(1, 2).contiguous().transpose(1, 2)  # the (F, 64, heads, d) layout a fused QKV projection leaves
    assert not qt.is_contiguous() and torch.equal(qt, q)
    for a, b in zip(run(qt, k, v, w), run(q, k, v, w)):
        assert torch.equal(a, b)


def test_two_backward_passes_from_one_forward_give_equal_bits():
    import dfot_amd
    d = 64
    q, k, v, w = inputs(d, torch.bfloat16, seed=2)
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    loss = (dfot_amd.attention_seq64(q, k, v) * w).sum()
    first = torch.autograd.grad(loss, (q, k, v), retain_graph=True)
    second = torch.autograd.grad(loss, (q, k, v))
    for a, b in zip(first, second):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
