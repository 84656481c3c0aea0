"""Shared by the tests of dfot_op_attention_seq64_bwd (csrc/attention_seq64_bwd.hip): the seeded cases, the fp64 reference and a host
restatement of the kernel's roundings.  No GPU is needed for anything in here.

A case is q, k, v, d_o [nseq][heads][64][d]: unit-normal values rounded to bf16 (held as fp32), q and k times `gain` (a power of two, so
the products are bf16 values too).  The yardstick is fp64 autograd through softmax(q k^T / sqrt(d)) v on exactly those values.

emulate() follows the kernel step by step in fp32 with its roundings and nothing of its summation order:
    q' = bf16(q log2(e) / sqrt(d));  S' = q' k^T;  P = exp2(S' - rowmax) / rowsum;  dP = d_o v^T;  delta = sum_j P dP;  dS = P (dP - delta)
    dv = bf16(bf16(P)^T d_o);  dq = bf16(bf16(dS) k / sqrt(d));  dk = bf16(ln 2 * bf16(dS)^T q')
`fault` swaps in one of the mistakes a kernel of this shape can make, to show that the GPU bar separates them (test_attention_seq64_bwd_host)."""
import math

import torch

BAR = 2e-2               # rel-L2 of dq, dk, dv against fp64: tests/test_gpu_train.py:52, OP_BAR of tests/test_gpu_dit_fac_train.py
HEAD_DIMS = [32, 64, 72, 96, 128]  # one per (D, DQK, DV) instantiation; d = 72 does not fill its row stride
GAINS = [1.0, 2.0]
NSEQ, HEADS = 3, 2       # odd sequence count, more than one head: the smallest launch that reaches every index path
LOG2E = math.log2(math.e)


def bf(t):
    return t.to(torch.bfloat16).float()


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def dstride(d):
    return 64 if d <= 64 else 128


def make_case(d, gain, nseq=NSEQ, heads=HEADS, seed=None):
    g = torch.Generator().manual_seed(3 + d if seed is None else seed)
    q, k, v, d_o = (bf(torch.randn(nseq, heads, 64, d, generator=g)) for _ in range(4))
    return dict(q=q * gain, k=k * gain, v=v, d_o=d_o, d=d, nseq=nseq, heads=heads)


def reference(c):
    """fp64 autograd -> (dq, dk, dv), each [nseq][heads][64][d]"""
    q, k, v = (c[n].double().requires_grad_() for n in "qkv")
    o = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(c["d"]), -1) @ v
    (o * c["d_o"].double()).sum().backward()
    return q.grad, k.grad, v.grad


def scaled_q(c):
    """what the kernel reads as q: bf16(q log2(e) / sqrt(d)), the product taken in fp32"""
    return bf(c["q"] * (LOG2E / math.sqrt(c["d"])))


def pack(c, device, ldo=None):
    """the kernel's operands on `device`: q', k, v [nseq][heads][64][dstride] bf16 with zero pad columns, and d_o [(seq*64 + row)][ldo] with
    head hd at column hd*d; columns past heads*d hold NaN"""
    d, nseq, heads = c["d"], c["nseq"], c["heads"]
    ldo = heads * d if ldo is None else ldo

    def pad(t):
        out = torch.zeros(nseq, heads, 64, dstride(d), dtype=torch.bfloat16)
        out[..., :d] = t.to(torch.bfloat16)
        return out.to(device)
    d_o = torch.full((nseq * 64, ldo), float("nan"), dtype=torch.bfloat16)
    d_o[:, : heads * d] = c["d_o"].transpose(1, 2).reshape(nseq * 64, heads * d).to(torch.bfloat16)
    return pad(scaled_q(c)), pad(c["k"]), pad(c["v"]), d_o.to(device)


def emulate(c, fault=None):
    """-> (dq, dk, dv) as the kernel rounds them.  fault: None | "no_delta" | "delta_halves_swapped" | "dk_without_ln2" | "delta_from_bf16_o"
    (delta = sum_c d_o o from a bf16 o, as launch_attention_bwd_delta forms it: a design the kernel does not use, for comparison)"""
    d = c["d"]
    qs, k, v, d_o = scaled_q(c), c["k"], c["v"], c["d_o"]
    s = qs @ k.transpose(-1, -2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    p = p / p.sum(-1, keepdim=True)
    dp = d_o @ v.transpose(-1, -2)
    delta = (p * dp).sum(-1, keepdim=True)
    if fault == "no_delta":
        delta = torch.zeros_like(delta)
    elif fault == "delta_halves_swapped":  # row i takes the delta of row i ^ 32
        delta = torch.cat([delta[..., 32:, :], delta[..., :32, :]], -2)
    elif fault == "delta_from_bf16_o":
        delta = (bf(bf(p) @ v) * d_o).sum(-1, keepdim=True)
    ds = bf(p * (dp - delta))
    dv = bf(p).transpose(-1, -2) @ d_o
    dq = ds @ k / math.sqrt(d)
    dk = ds.transpose(-1, -2) @ qs * (1.0 if fault == "dk_without_ln2" else math.log(2.0))
    return bf(dq), bf(dk), bf(dv)
