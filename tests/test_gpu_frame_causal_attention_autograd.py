"""GPU tests of the differentiable operator dfot_amd.frame_causal_attention (ops.py: dfot::frame_causal_attention), the drop-in for
F.scaled_dot_product_attention(q, k, v, attn_mask=<block lower triangular>) of the reference DiT1D's Attention.forward.

Inputs (B, heads, N, d); forward and the three input gradients of (o * w).sum() for a seeded w against fp64
softmax(q k^T / sqrt(d) + mask) v on the same input values, with the bars of the op-level tests (output rel-L2 < 1.5e-2, gradients
< 2.5e-2): on top of the kernels' roundings the wrapper rounds q log2(e)/sqrt(d) to bf16, a relative 2^-9 per element (measured:
2.9e-3 to 3.6e-3 at these shapes).  fp32 inputs return fp32 output and gradients; their k, v and d_o are rounded to bf16 as well
(4.0e-3 to 4.9e-3).  A non-contiguous q gives the bits of its contiguous copy; the output is compact as (B, N, heads, d); two backward passes
from one forward give equal bits.  Every test fails on the parent commit, where the operator does not exist."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BAR_O, BAR_GRAD = 1.5e-2, 2.5e-2
BATCH, HEADS = 2, 2
SHAPES = [(32, 4, 64), (16, 16, 72), (32, 8, 128)]  # (L, T, d)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def inputs(L, T, d, dtype, seed=0):
    """q, k, v, w (B, heads, N, d): unit-normal values of `dtype`, q times 1.5 (scores of the op-level tests)"""
    g = torch.Generator().manual_seed(seed + 1000 * L * T + d)
    q, k, v, w = (torch.randn(BATCH, HEADS, L * T, d, generator=g) for _ in range(4))
    return tuple(t.to(dtype).cuda() for t in (1.5 * q, k, v, w))


def reference(q, k, v, w, frame_len):
    """fp64 on the CPU from the values the operator was given -> (o, dq, dk, dv)"""
    q, k, v = (t.double().cpu().requires_grad_() for t in (q, k, v))
    n, d = q.shape[2:]
    f = torch.arange(n) // frame_len
    s = (q @ k.transpose(-1, -2) / math.sqrt(d)).masked_fill(f[None, :] > f[:, None], float("-inf"))
    o = torch.softmax(s, -1) @ v
    (o * w.double().cpu()).sum().backward()
    return o.detach(), q.grad, k.grad, v.grad


def run(q, k, v, w, frame_len):
    import dfot_amd
    q, k, v = (t.detach().requires_grad_() for t in (q, k, v))
    o = dfot_amd.frame_causal_attention(q, k, v, frame_len)
    (o * w).sum().backward()
    torch.cuda.synchronize()
    return o.detach(), q.grad, k.grad, v.grad


@functools.lru_cache(maxsize=None)
def case(L, T, d, dtype):
    x = inputs(L, T, d, dtype)
    return x, run(*x, L), reference(*x, L)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("L,T,d", SHAPES)
def test_forward_and_input_gradients_vs_fp64(L, T, d, dtype):
    x, got, want = case(L, T, d, dtype)
    for name, g, r, bar in zip(("o", "dq", "dk", "dv"), got, want, (BAR_O, BAR_GRAD, BAR_GRAD, BAR_GRAD)):
        assert g.shape == x[0].shape and g.dtype == dtype, name
        assert torch.isfinite(g.float()).all(), name
        e = rel(g.float().cpu(), r)
        print(f"frame_causal_attention {dtype} L={L} T={T} d={d} {name}: rel-L2 vs fp64 {e:.2e}")
        assert e < bar, name


def test_output_is_compact_as_the_reference_reshapes_it():
    """o.transpose(1, 2).reshape(B, N, heads * d) is a view of the kernel's compact buffer and holds what the C entry writes there"""
    import dfot_amd
    from dfot_amd import capi, ops
    L, T, d = 16, 16, 72
    n = L * T
    q, k, v, _ = inputs(L, T, d, torch.bfloat16)
    o = dfot_amd.frame_causal_attention(q, k, v, L)
    flat = o.transpose(1, 2).reshape(BATCH, n, HEADS * d)
    assert o.transpose(1, 2).is_contiguous() and flat.data_ptr() == o.data_ptr()
    qp, kp, vp = ops._fc_pack(q, d, math.log2(math.e) / math.sqrt(d)), ops._fc_pack(k, d), ops._fc_pack(v, d)
    assert qp.shape == (BATCH, HEADS, n, 128) and not qp[..., d:].any()
    direct = torch.full((BATCH * n, HEADS * d), float("nan"), dtype=torch.bfloat16, device="cuda")
    capi.check(capi.lib.dfot_op_attention_frame_causal(capi.ptr(qp), capi.ptr(kp), capi.ptr(vp), capi.ptr(direct), HEADS * d, BATCH, HEADS, n, L,
                                                       d, capi.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(flat.reshape(BATCH * n, HEADS * d), direct)


def test_non_contiguous_q_gives_the_bits_of_its_contiguous_copy():
    L, T, d = 32, 4, 64
    q, k, v, w = inputs(L, T, d, torch.bfloat16, seed=1)
    qt = q.transpose(1, 2).contiguous().transpose(1, 2)  # the (B, N, heads, d) layout a fused QKV projection leaves
    assert not qt.is_contiguous() and torch.equal(qt, q)
    for a, b in zip(run(qt, k, v, w, L), run(q, k, v, w, L)):
        assert torch.equal(a, b)


def test_two_backward_passes_from_one_forward_give_equal_bits():
    import dfot_amd
    L, T, d = 32, 4, 64
    q, k, v, w = inputs(L, T, d, torch.bfloat16, seed=2)
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    loss = (dfot_amd.frame_causal_attention(q, k, v, L) * w).sum()
    first = torch.autograd.grad(loss, (q, k, v), retain_graph=True)
    second = torch.autograd.grad(loss, (q, k, v))
    for a, b in zip(first, second):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
