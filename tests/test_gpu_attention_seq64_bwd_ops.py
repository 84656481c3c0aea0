"""Op-level GPU tests of dfot_op_attention_seq64_bwd (csrc/attention_seq64_bwd.hip): the backward of the attention over sequences of
exactly 64 tokens, the per-frame spatial attention of FacDiT / FacMatDiT at 64 patches per frame.

Cases and reference: attention_seq64_bwd_common (bf16-rounded unit-normal q, k, v, d_o, q and k times a gain; fp64 autograd through
softmax(q k^T / sqrt(d)) v).  nseq 3 (odd), heads 2: the smallest launch that reaches every index path; d in {32, 64, 72, 96, 128} is one
per kernel instantiation.  Bar: each of dq, dk, dv rel-L2 < 2e-2, the project's bar for the flash-attention backward
(tests/test_gpu_train.py:52, OP_BAR of tests/test_gpu_dit_fac_train.py).  tests/test_attention_seq64_bwd_host.py shows on these very inputs
that a host restatement of the kernel's roundings measures 2.7e-3 to 3.3e-3 at gain 1 and 3.6e-3 to 5.3e-3 at gain 2, and what broken
kernels would measure:
    delta omitted:                                dq / dk 0.21 - 0.29 at gain 1, 1.5 - 2.1 at gain 2
    delta of row i ^ 32 (halves swapped):         dq / dk 0.29 - 0.39 at gain 1, 2.0 - 2.9 at gain 2
    dk without ln 2:                              dk 0.44
Measured on an MI355X: the kernel gives the restatement's figures to three digits (worst: dk 5.26e-3 at d = 72, gain 2).
Every test fails on the parent commit, where the symbol does not exist."""
import functools
import math

import pytest
import torch

from attention_seq64_bwd_common import BAR, GAINS, HEADS, HEAD_DIMS, NSEQ, dstride, make_case, pack, reference, rel

pytestmark = pytest.mark.gpu

NAN = float("nan")


def call(dev, outs, nseq, heads, d, ldo=None):
    from dfot_amd import capi
    P = capi.ptr
    ldo = heads * d if ldo is None else ldo
    return capi.lib.dfot_op_attention_seq64_bwd(P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), ldo, P(outs[0]), P(outs[1]), P(outs[2]), nseq, heads,
                                                d, capi.stream_ptr())


def run(dev, nseq, heads, d, ldo=None, extra=0, fill=NAN):
    """-> dq, dk, dv [nseq + extra][heads][64][dstride], `fill` wherever the kernel did not write"""
    from dfot_amd import capi
    outs = [torch.full((nseq + extra, heads, 64, dstride(d)), fill, dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    capi.check(call(dev, outs, nseq, heads, d, ldo))
    torch.cuda.synchronize()
    return outs


@functools.lru_cache(maxsize=None)
def case(d, gain):
    """(case, device operands, dq / dk / dv of one run, fp64 reference): computed once, shared, never written to"""
    c = make_case(d, gain)
    dev = pack(c, "cuda")
    return c, dev, run(dev, c["nseq"], c["heads"], d), reference(c)


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_vs_fp64_autograd(d, gain):
    """outputs start as NaN: the live columns are finite and within the bar, the pad columns are still NaN"""
    c, dev, got, want = case(d, gain)
    for name, g, r in zip(("dq", "dk", "dv"), got, want):
        live, padc = g[..., :d].float().cpu(), g[..., d:].float()
        assert torch.isfinite(live).all(), name
        assert torch.isnan(padc).all(), name
        e = rel(live, r)
        print(f"attention_seq64_bwd d={d} gain={gain} {name}: rel-L2 vs fp64 {e:.2e}")
        assert e < BAR, name


@pytest.mark.parametrize("d", [32, 72, 128])
def test_writes_nothing_past_the_end_and_leaves_its_inputs(d):
    """two sentinel sequences of 7.0 behind dq, dk, dv are untouched; q, k, v, d_o are bit-identical after the call"""
    c, dev, got, _ = case(d, 1.0)
    before = [t.clone() for t in dev]
    outs = run(dev, NSEQ, HEADS, d, extra=2, fill=7.0)
    for t, b in zip(dev, before):
        assert torch.equal(t.view(torch.int16), b.view(torch.int16))
    for o, g in zip(outs, got):
        assert (o[NSEQ:] == 7.0).all()
        assert torch.equal(o[:NSEQ, ..., :d], g[..., :d])
        assert (o[:NSEQ, ..., d:] == 7.0).all()


@pytest.mark.parametrize("d", HEAD_DIMS)
def test_reproducible_bits(d):
    """the last sequence alone gives the bits it gives in the batch of three; two runs give equal bits"""
    c, dev, got, _ = case(d, 2.0)
    again = run(dev, NSEQ, HEADS, d)
    last = [t[NSEQ - 1:].clone() for t in dev[:3]] + [dev[3][(NSEQ - 1) * 64:].clone()]
    alone = run(last, 1, HEADS, d)
    for g, a, l in zip(got, again, alone):
        assert torch.equal(g[..., :d], a[..., :d])
        assert torch.equal(l[0, ..., :d], g[NSEQ - 1, ..., :d])


def test_invalid_shapes_launch_nothing():
    from dfot_amd import capi
    nseq, heads, d = NSEQ, HEADS, 64
    c, dev, got, _ = case(d, 1.0)
    outs = [torch.full((nseq, heads, 64, 64), NAN, dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    # (ldo, nseq, heads, d): the refusal list of the launcher
    for args in ((72, nseq, heads, 36), (128, nseq, heads, 0), (128, nseq, heads, -8), (272, nseq, heads, 136), (128, 0, heads, d),
                 (128, -1, heads, d), (128, nseq, 0, d), (128, 65536, 32768, d), (heads * d - 8, nseq, heads, d), (heads * d + 4, nseq, heads, d)):
        assert call(dev, outs, args[1], args[2], args[3], ldo=args[0]) == capi.ERR_SHAPE, args
        assert capi.lib.dfot_last_error().startswith(b"attention_seq64_bwd:"), args
    P = capi.ptr
    ptrs = [P(t) for t in dev] + [P(t) for t in outs]
    for hole in range(7):
        a = list(ptrs)
        a[hole] = None
        assert capi.lib.dfot_op_attention_seq64_bwd(*a[:4], heads * d, *a[4:], nseq, heads, d, capi.stream_ptr()) == capi.ERR_ARG, hole
        assert capi.lib.dfot_last_error().startswith(b"attention_seq64_bwd:"), hole
    torch.cuda.synchronize()
    for o in outs:
        assert torch.isnan(o.float()).all()
    assert call(dev, outs, nseq, heads, d) == capi.OK  # the same buffers at a valid shape do launch
    torch.cuda.synchronize()
    for o, g in zip(outs, got):
        assert torch.equal(o, g)


@pytest.mark.parametrize("d", [64, 72])
def test_d_o_embedded_in_a_wider_row(d):
    """ldo = heads*d + 8 with the gap filled with NaN: the bits of the compact call (nothing beyond a head's d columns is read)"""
    c, dev, got, _ = case(d, 1.0)
    ldo = HEADS * d + 8
    wide = pack(c, "cuda", ldo=ldo)
    assert torch.isnan(wide[3][:, HEADS * d:].float()).all()
    for w, g in zip(run(wide, NSEQ, HEADS, d, ldo=ldo), got):
        assert torch.equal(w[..., :d], g[..., :d])


@pytest.mark.parametrize("d", [32, 72, 128])
def test_closed_form_with_zero_keys(d):
    """k = 0: every score is 0, the softmax is uniform, P = 1/64 exactly (exp2(0) = 1, the row sum 64 and its reciprocal are exact, 1/64 is
    a bf16 value).  Then
      dv[j] = (1/64) sum_q d_o[q] for every j: an fp32 sum of 64 exact products rounded once to bf16, so within 2^-8 relative of fp64;
      dq = dS k / sqrt(d) = 0 EXACTLY, whatever dS is: every product has a zero factor;
      dS[i][j] = (dP[i][j] - delta[i]) / 64 with dP[i][j] = <d_o[i], v[j]> and delta[i] the mean of dP[i][:], and
      dk[j] = sum_i dS[i][j] q[i] / sqrt(d), which is NOT zero for keys with different values: it is compared with this closed form in fp64
      under the bar of this file.
    dk is zero when moreover every key carries the same value row, v[j] = v0: then dP[i][j] = x_i = <d_o[i], v0> for every j, delta[i] = x_i
    and dS = 0 in exact arithmetic.  In fp32, delta[i] is a chain of 64 fused multiply-adds of x_i / 64, each rounding a partial sum of at
    most |x_i| to 2^-24 relative, so |dP - delta| <= 64 * 2^-24 |x_i| = 2^-18 |x_i| (the same bound covers a last-bit difference between
    the dP of the two orientations), |dS| <= 2^-24 |x_i|, and |x_i| <= d max|d_o| max|v|.  dk[j][c] = ln 2 * sum_i dS[i][j] q'[i][c] with
    |q'| = |q| log2(e) / sqrt(d) sums 64 such terms: |dk| <= 64 * 2^-24 * d * max|d_o| max|v| * max|q| / sqrt(d) = 2^-18 sqrt(d) max|v| *
    max|q| max|d_o|.  With sqrt(d) max|v| < 2^10 (here < 12 * 5) that is below 2^-8 max|q| max|d_o|, the bound asserted."""
    c = make_case(d, 1.0, seed=11 + d)
    c["k"] = torch.zeros_like(c["k"])
    q, v, d_o = (c[n].double() for n in ("q", "v", "d_o"))
    dq, dk, dv = (t[..., :d].float().cpu() for t in run(pack(c, "cuda"), NSEQ, HEADS, d))
    want_dv = d_o.mean(-2, keepdim=True).expand_as(d_o)
    assert rel(dv, want_dv) < 2.0 ** -8
    assert (dq == 0).all()
    dp = d_o @ v.transpose(-1, -2)
    ds = (dp - dp.mean(-1, keepdim=True)) / 64
    e = rel(dk, ds.transpose(-1, -2) @ q / math.sqrt(d))
    print(f"attention_seq64_bwd d={d}, k = 0: dk rel-L2 vs the closed form {e:.2e}")
    assert e < BAR
    # one value row for every key: dk = 0 up to the fp32 cancellation derived above
    c["v"] = c["v"][..., :1, :].expand_as(c["v"]).contiguous()
    assert math.sqrt(d) * float(c["v"].abs().max()) < 2.0 ** 10
    dq, dk, dv = (t[..., :d].float().cpu() for t in run(pack(c, "cuda"), NSEQ, HEADS, d))
    bound = 2.0 ** -8 * float(c["q"].abs().max()) * float(c["d_o"].abs().max())
    print(f"attention_seq64_bwd d={d}, k = 0, one value row: max |dk| {float(dk.abs().max()):.2e} (bound {bound:.2e})")
    assert (dq == 0).all()
    assert float(dk.abs().max()) <= bound
    assert rel(dv, want_dv) < 2.0 ** -8
