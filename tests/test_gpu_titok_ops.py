"""GPU: the ops of csrc/titok.hip, each against an fp64 torch computation of the same (bf16-rounded where the op takes bf16) operands.

Bars (taken from the existing op tests and the number formats, not from these kernels):
  * ragged multi-head attention: rel-L2 < 1.5e-2, the bar tests/test_gpu_dit.py (test_attention_temporal_vs_fp64) and the ImageVAE
    attention test hold (bf16 rounding of P and O);
  * fp32 outputs (LayerNorm, token assembly): 1e-5 relative (rel-L2, and per element against the row's largest magnitude);
  * bf16 outputs (LayerNorm, bias + GELU / tanh): one bf16 rounding, 2^-8 relative per element, rel-L2 < 4e-3."""
import math

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


def rel(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30)).item()


def pad128(n):
    return -(-n // 128) * 128


def mha_reference(qkv, seqs, length, heads):
    """fp64 softmax(q k^T / 8) v per sequence and head from the packed bf16 rows: [seqs * length][heads * 64]"""
    x = qkv[: seqs * length].double().reshape(seqs, length, 3, heads, 64)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    w = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
    return (w @ v).transpose(1, 2).reshape(seqs * length, heads * 64)


def run_mha(capi, qkv, seqs, length, heads):
    """qkv bf16 [rows >= seqs * length][>= 3 * heads * 64] on the host -> the op's o [seqs * length][heads * 64] (fp32, host) and
    the whole o buffer (NaN-filled before the launch: rows the op must not write stay NaN)"""
    d = qkv.cuda().contiguous()
    o = torch.full((d.shape[0], heads * 64), float("nan"), dtype=BF, device="cuda")
    capi.check(capi.lib.dfot_op_mha_packed(capi.ptr(d), d.shape[1], capi.ptr(o), seqs, length, heads, capi.stream_ptr()))
    torch.cuda.synchronize()
    return o[: seqs * length].float().cpu(), o.cpu()


@pytest.mark.parametrize("heads", [8, 12])
@pytest.mark.parametrize("seqs", [1, 3])
@pytest.mark.parametrize("length", [1, 49, 64, 97, 128, 289])
def test_mha_packed_vs_fp64(capi, length, seqs, heads):
    g = torch.Generator().manual_seed(1000 * length + 10 * seqs + heads)
    rows = pad128(seqs * length)
    qkv = torch.randn(rows, 3 * heads * 64, generator=g).to(BF)
    got, whole = run_mha(capi, qkv, seqs, length, heads)
    ref = mha_reference(qkv.float(), seqs, length, heads)
    r = rel(got, ref)
    print(f"mha_packed len {length} seqs {seqs} heads {heads}: rel-L2 {r:.3e}, max abs {(got.double() - ref).abs().max().item():.3e}")
    assert torch.isfinite(got).all() and r < 1.5e-2
    assert torch.isnan(whole[seqs * length:].float()).all()          # query rows past the last sequence are not stored


def test_mha_packed_row_stride(capi):
    """a qkv buffer wider than 3 * heads * 64 (row stride given): the extra columns are never read"""
    g = torch.Generator().manual_seed(3)
    seqs, length, heads = 2, 97, 8
    qkv = torch.randn(pad128(seqs * length), 3 * heads * 64, generator=g).to(BF)
    wide = torch.cat([qkv, torch.full((qkv.shape[0], 64), float("nan"), dtype=BF)], 1)
    a, _ = run_mha(capi, qkv, seqs, length, heads)
    b, _ = run_mha(capi, wide, seqs, length, heads)
    assert torch.equal(a, b)


@pytest.mark.parametrize("length", [49, 97, 289])
def test_mha_packed_never_reads_rows_a_sequence_does_not_own(capi, length):
    """the qkv buffer is over-allocated to the next 128 rows; the pad rows and every row of sequence 1 are NaN.  The other sequences'
    outputs stay finite and BITWISE equal to a run without the poison: no key, value or query row of another owner reaches them.  The
    same bits also come out of a launch that holds sequence 0 alone (one summation order per (len, heads))."""
    g = torch.Generator().manual_seed(length)
    seqs, heads = 3, 8
    rows = pad128(seqs * length)
    assert rows > seqs * length
    qkv = torch.randn(rows, 3 * heads * 64, generator=g).to(BF)
    clean, _ = run_mha(capi, qkv, seqs, length, heads)
    bad = qkv.clone()
    bad[seqs * length:] = float("nan")
    bad[length:2 * length] = float("nan")
    got, _ = run_mha(capi, bad, seqs, length, heads)
    keep = torch.cat([torch.arange(0, length), torch.arange(2 * length, 3 * length)])
    assert torch.isfinite(got[keep]).all()
    assert torch.equal(got[keep].view(torch.int32), clean[keep].view(torch.int32))
    assert torch.isnan(got[length:2 * length]).all()
    alone, _ = run_mha(capi, qkv[:pad128(length)], 1, length, heads)
    assert torch.equal(alone.view(torch.int32), clean[:length].view(torch.int32))


@pytest.mark.parametrize("mult,floor", [(8.0, 30.0), (32.0, 89.0)])
def test_mha_packed_large_scores_need_the_max_subtraction(capi, mult, floor):
    """q x 8 (and x 32): scores / 8 of about N(0, mult^2); at x 32 exp of the raw score overflows fp32 outright (e^88.7).  Only
    exp(s - max) stays in range -- also across key blocks, where the running max rescales the accumulator."""
    g = torch.Generator().manual_seed(5)
    seqs, length, heads = 2, 289, 8
    qkv = torch.randn(pad128(seqs * length), 3 * heads * 64, generator=g).to(BF)
    qkv[:, : heads * 64] = (qkv[:, : heads * 64].float() * mult).to(BF)
    x = qkv[: seqs * length].float().reshape(seqs, length, 3, heads, 64)
    top = (x[:, :, 0].transpose(1, 2) @ x[:, :, 1].transpose(1, 2).transpose(-1, -2) / 8.0).max().item()
    print(f"largest score / 8 at q x {mult:g}: {top:.1f}")
    assert top > floor
    got, _ = run_mha(capi, qkv, seqs, length, heads)
    r = rel(got, mha_reference(qkv.float(), seqs, length, heads))
    print(f"mha_packed, q x {mult:g}: rel-L2 {r:.3e}")
    assert torch.isfinite(got).all() and r < 1.5e-2


def test_mha_packed_refuses_bad_shapes_before_any_launch(capi):
    lmax = capi.lib.dfot_op_mha_packed_max_len()
    assert lmax >= 1057
    heads = 8
    qkv = torch.zeros(128, 3 * heads * 64, dtype=BF, device="cuda")
    o = torch.full((128, heads * 64), float("nan"), dtype=BF, device="cuda")
    for seqs, length, hd, ld, word in ((1, 0, heads, 3 * heads * 64, "len=0"), (1, lmax + 1, heads, 3 * heads * 64, f"len={lmax + 1}"),
                                       (1, 49, 0, 3 * heads * 64, "heads=0"), (1, 49, heads, 3 * heads * 64 - 8, f"ld={3 * heads * 64 - 8}")):
        rc = capi.lib.dfot_op_mha_packed(capi.ptr(qkv), ld, capi.ptr(o), seqs, length, hd, capi.stream_ptr())
        assert rc == capi.ERR_SHAPE
        assert word in capi.lib.dfot_last_error().decode()
    torch.cuda.synchronize()
    assert torch.isnan(o.float()).all()                              # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------------------
def check_f32(name, got, ref):
    r = rel(got, ref)
    worst = ((got.double() - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-30)).max().item()
    print(f"{name}: fp32 rel-L2 {r:.3e}, worst element / row max {worst:.3e}")
    assert r < 1e-5 and worst < 1e-5


def check_bf16(name, got, ref):
    """one bf16 rounding of an fp32 evaluation: |got - ref| <= 2^-8 |ref| per element, plus what the fp32 value in front of the rounding is
    allowed (the fp32 bar above: 1e-5 of the largest magnitude), which only matters where the result is tiny against its inputs"""
    r = rel(got, ref)
    floor = 1e-5 * ref.abs().max().item()
    excess = ((got.double() - ref).abs() - (2.0 ** -8) * ref.abs() - floor).max().item()
    print(f"{name}: bf16 rel-L2 {r:.3e}, worst excess over 2^-8 relative {excess:.3e}")
    assert r < 4e-3 and excess <= 0.0


@pytest.mark.parametrize("rows", [289, 867])
@pytest.mark.parametrize("c", [512, 768, 1024])
def test_layernorm_vs_fp64(capi, c, rows):
    g = torch.Generator().manual_seed(c + rows)
    x = torch.randn(rows, c, generator=g) * 3.0 + 0.5
    gamma, beta = 1.0 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    ref = F.layer_norm(x.double(), (c,), gamma.double(), beta.double(), 1e-5)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    ob = torch.full((rows, c), float("nan"), dtype=BF, device="cuda")
    of = torch.full((rows, c), float("nan"), device="cuda")
    capi.check(capi.lib.dfot_op_layernorm(capi.ptr(xd), capi.ptr(gd), capi.ptr(bd), 1e-5, capi.ptr(ob), capi.ptr(of), rows, c, 0, 0, 0,
                                          capi.stream_ptr()))
    check_f32(f"layernorm C {c} rows {rows}", of.cpu(), ref)
    check_bf16(f"layernorm C {c} rows {rows}", ob.float().cpu(), ref)
    # either output alone gives the same bits
    ob2, of2 = torch.empty_like(ob), torch.empty_like(of)
    capi.check(capi.lib.dfot_op_layernorm(capi.ptr(xd), capi.ptr(gd), capi.ptr(bd), 1e-5, capi.ptr(ob2), None, rows, c, 0, 0, 0, capi.stream_ptr()))
    capi.check(capi.lib.dfot_op_layernorm(capi.ptr(xd), capi.ptr(gd), capi.ptr(bd), 1e-5, None, capi.ptr(of2), rows, c, 0, 0, 0, capi.stream_ptr()))
    assert torch.equal(ob2, ob) and torch.equal(of2, of)


@pytest.mark.parametrize("c", [512, 768, 1024])
def test_layernorm_gather_form(capi, c):
    """ln_post's form: rows 1 .. 16 of each of 3 sequences of 49 rows -> a compact [48][C]; every other source row is NaN"""
    g = torch.Generator().manual_seed(c)
    seqs, length, first, take = 3, 49, 1, 16
    x = torch.randn(seqs, length, c, generator=g)
    gamma, beta = 1.0 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    ref = F.layer_norm(x[:, first:first + take].double(), (c,), gamma.double(), beta.double(), 1e-5).reshape(seqs * take, c)
    poisoned = torch.full_like(x, float("nan"))
    poisoned[:, first:first + take] = x[:, first:first + take]
    xd = torch.cat([poisoned.reshape(seqs * length, c), torch.full((128 - (seqs * length) % 128, c), float("nan"))]).cuda()
    gd, bd = gamma.cuda(), beta.cuda()                               # (kept alive: the op takes raw pointers)
    ob = torch.full((seqs * take, c), float("nan"), dtype=BF, device="cuda")
    of = torch.full((seqs * take, c), float("nan"), device="cuda")
    capi.check(capi.lib.dfot_op_layernorm(capi.ptr(xd), capi.ptr(gd), capi.ptr(bd), 1e-5, capi.ptr(ob), capi.ptr(of), seqs * take, c,
                                          length, first, take, capi.stream_ptr()))
    check_f32(f"layernorm gather C {c}", of.cpu(), ref)
    check_bf16(f"layernorm gather C {c}", ob.float().cpu(), ref)
    for bad in ((length, first, take + 1, seqs * take), (length, length - take + 1, take, seqs * take), (0, 1, 0, seqs * take)):
        rc = capi.lib.dfot_op_layernorm(capi.ptr(xd), capi.ptr(gd), capi.ptr(bd), 1e-5, capi.ptr(ob), None, bad[3], c, bad[0], bad[1],
                                        bad[2], capi.stream_ptr())
        assert rc == capi.ERR_SHAPE and "op_layernorm" in capi.lib.dfot_last_error().decode()
    rc = capi.lib.dfot_op_layernorm(capi.ptr(xd), capi.ptr(gd), capi.ptr(bd), 1e-5, capi.ptr(ob), None, 48, 640, 0, 0, 0, capi.stream_ptr())
    assert rc == capi.ERR_SHAPE and "channels=640" in capi.lib.dfot_last_error().decode()


@pytest.mark.parametrize("act,n", [(0, 2048), (1, 1024), (0, 3072), (1, 1536)])
def test_bias_act_vs_fp64(capi, act, n):
    """act 0: nn.GELU() (exact erf form, NOT the tanh approximation); act 1: tanh.  289 rows, inputs out to +-6"""
    g = torch.Generator().manual_seed(act + n)
    rows = 289
    x, bias = torch.randn(rows, n, generator=g) * 2.0, 0.5 * torch.randn(n, generator=g)
    t = x.double() + bias.double()
    ref = 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0))) if act == 0 else torch.tanh(t)
    xd, bd = x.cuda(), bias.cuda()                                   # (kept alive: the op takes raw pointers)
    out = torch.full((rows, n), float("nan"), dtype=BF, device="cuda")
    capi.check(capi.lib.dfot_op_bias_act_bf16(capi.ptr(xd), n, capi.ptr(bd), capi.ptr(out), rows, n, act, capi.stream_ptr()))
    check_bf16(f"bias + {'GELU-erf' if act == 0 else 'tanh'} n {n}", out.float().cpu(), ref)
    if act == 0:   # the erf form and the tanh approximation differ by up to 5e-4 near |t| = 2: the bar above tells them apart at 2^-8 relative
        approx = F.gelu(t, approximate="tanh")
        assert ((approx - ref).abs() - (2.0 ** -8) * ref.abs() - 1e-5 * ref.abs().max()).max().item() > 0
    rc = capi.lib.dfot_op_bias_act_bf16(capi.ptr(xd), n, capi.ptr(bd), capi.ptr(out), rows, n, 2, capi.stream_ptr())
    assert rc == capi.ERR_SHAPE and "act=2" in capi.lib.dfot_last_error().decode()


@pytest.mark.parametrize("c,grid2,l2norm", [(512, 16, 1), (768, 64, 1), (1024, 256, 1), (512, 16, 0)])
def test_token_assembly_vs_fp64(capi, c, grid2, l2norm):
    g = torch.Generator().manual_seed(c + grid2 + l2norm)
    frames, ts, nlat = 3, 4, 32
    z = torch.randn(frames, ts, 1, nlat, generator=g)
    ew, eb = torch.randn(c, ts, generator=g) / 2.0, 0.02 * torch.randn(c, generator=g)
    lpos, cls, mask, pos = (torch.randn(s, generator=g) / math.sqrt(c) for s in ((nlat, c), (1, c), (1, 1, c), (grid2 + 1, c)))
    gamma, beta = 1.0 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    zd = z.double()
    zn = F.normalize(zd, dim=1) if l2norm else zd
    lat = F.linear(zn.reshape(frames, ts, nlat).permute(0, 2, 1), ew.double(), eb.double()) + lpos.double()
    front = torch.cat([cls.double().unsqueeze(0).expand(frames, -1, -1), mask.double().repeat(frames, grid2, 1)], 1) + pos.double()[None]
    ref = F.layer_norm(torch.cat([front, lat], 1), (c,), gamma.double(), beta.double(), 1e-5).reshape(-1, c)
    out = torch.full((frames * (1 + grid2 + nlat), c), float("nan"), device="cuda")
    dev = [t.cuda().contiguous() for t in (z, ew, eb, lpos, cls, mask, pos, gamma, beta)]
    capi.check(capi.lib.dfot_op_titok_tokens(*[capi.ptr(t) for t in dev], 1e-5, capi.ptr(out), frames, grid2, nlat, ts, c, l2norm, capi.stream_ptr()))
    check_f32(f"token assembly C {c} grid^2 {grid2} l2norm {l2norm}", out.cpu(), ref)
    rc = capi.lib.dfot_op_titok_tokens(*[capi.ptr(t) for t in dev], 1e-5, capi.ptr(out), frames, grid2, nlat, 65, c, l2norm, capi.stream_ptr())
    assert rc == capi.ERR_SHAPE and "token_size=65" in capi.lib.dfot_last_error().decode()
