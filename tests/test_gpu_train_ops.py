"""Op-level tests of the remaining dfot_op_* entry points (the pieces the UViT training driver uvit_train.py is built from, several of
them shared with the inference engine) against float64 host references of the same rounded operands.

Every output starts as NaN: what an op must not write (row-stride padding, cond_repack columns [4 cdim, kpad), cat outside
[ccol0, ccol0 + 4C), the tail behind an output) stays NaN, what it must write is finite.  Every case runs twice on the same stream from
the same initial buffers and must give bit-identical outputs (the reductions end in the fixed-order det_sum).

Bars (u = 2^-24):
  exact       bitwise equality: the casts (torch's CPU .to(bfloat16) is the reference: round to nearest even, +-0, +-inf, fp32
              subnormals, values that overflow bf16, exact ties; NaN inputs are the canonical quiet NaN), transpose_bf16, pack_conv3,
              cond_repack, outgrad_gather, mul_cols, split_bf16, the v copy of qknorm_rope_fwd
  fp32        |got - ref| <= c u sum|terms| + u |ref|, sum|terms| evaluated like the reference on absolute values.  c is the longest chain
              of fp32 roundings an output sees (the classical gamma_n bound of an n-term sum or dot product):
                axpy 2; upsample_add, pool2_bwd 1; upsample_bwd 2 (a two-level tree of 4)
                embed_input 4 cin + 1; project_output c0 + 1; sgemm K (+1 accumulating)
                embed_input_wgrad 64 chunks + ceil(partials / 16) + 4 (rows per workgroup, then det_sum's 16-way strided sum and tree)
                colsum_bf16 128 iters + ceil(partials / 16) + 4; frame_sums ceil(pixels / nz) + ceil(nz / 16) + 4
                the MFMA wrappers gemm_f32 / conv3x3_f32 17 (1e-6, the bar of the fused-epilogue tests at K <= 1024)
                rms_film_bwd dx 64 (a C-long wave reduction inside), dw rows + 32
  bf16        |got - bf16(ref)| <= n ulp(bf16(ref)) + the fp32 bar carried through: n = 1 (pool2_bf16, sub_bf16, emb_pyramid, gemm_bf16,
              the raw / v outputs of fused_proj_train), n = 2 after RMSNorm or RoPE and for SiLU (rms_film_fwd, qknorm_rope_fwd, silu_cols,
              the q / k / SiLU outputs of fused_proj_train)
The worst error / bar ratio of each family is printed at the end of the module (-s).  A table-driven test checks every shape / pointer
refusal and that a refused call writes nothing."""
import math

import pytest
import torch
import torch.nn.functional as F

# the harness lives in train_ops_common.py, which test_gpu_train_bwd_ops.py shares; capi and worst_ratio_table are fixtures
from train_ops_common import (NAN, P, S, U, bf, bits, capi, check, exact, nan_buf, record, run, seq_bar, tail, ulp_bf16,  # noqa: F401
                              worst_ratio_table)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------- casts

def special_f32():
    """fp32 edge values: signed zeros and infinities, the canonical quiet NaN, subnormals, values that overflow bf16, exact ties between
    two bf16 neighbours (rounding to even both ways) and one bit either side of a tie"""
    f = [0.0, -0.0, math.inf, -math.inf, 1e-40, -1e-40, 2.0 ** -149, -(2.0 ** -149), 2.0 ** -127, 1.1754942e-38, 2.0 ** -126,
         3.4028235e38, -3.4028235e38, 3.3961776e38, 3.3895314e38, 1.0, -1.0, 65504.0]
    b = [0x7FC00000,                                      # NaN
         0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # 1 + 2^-8 (tie -> 1), 1 + 3 2^-8 (tie -> 1 + 2^-6), negated
         0x3F808001, 0x3F807FFF, 0x00008000, 0x00018000,  # one bit above / below a tie; subnormal ties
         0x7F7F8000, 0x7F7F7FFF, 0x477FE000]              # the tie between bf16 max and inf, just below it, a tie at 65504
    t = torch.tensor(f, dtype=torch.float32)
    return torch.cat([t, torch.tensor(b, dtype=torch.int64).to(torch.int32).view(torch.float32)])


@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (1, 0), (0, 1), (4, 8)])
def test_f32_to_bf16_cast_is_exact(capi, src_off, dst_off):
    """16-byte aligned pointers take the 8-wide kernel plus a scalar tail (n % 8 = 5); an offset of one element takes the scalar kernel"""
    gen = torch.Generator().manual_seed(1 + src_off + 3 * dst_off)
    sp = special_f32()
    x = torch.cat([sp, torch.randn(1000, generator=gen) * torch.exp2(torch.randint(-30, 30, (1000,), generator=gen).float()), sp.flip(0)])
    n = x.numel()
    assert n % 8 != 0
    src = torch.cat([torch.zeros(src_off), x, torch.zeros(3)]).cuda()
    dst = nan_buf(dst_off + n + 8, dtype=torch.bfloat16)
    got, = run(capi, lambda: capi.lib.dfot_op_f32_to_bf16(P(src[src_off:]), P(dst[dst_off:]), n, S()), [dst])
    # the device's conversion preserves fp32 subnormals (no flush to zero): the subnormal inputs above compare against torch's rounding.
    # NaN is pinned to the canonical quiet NaN 0x7FC0 (torch's vectorised CPU conversion returns 0xFFFF for it instead)
    conv = x.to(torch.bfloat16)
    bits(conv)[torch.isnan(x)] = 0x7FC0
    want = torch.full((dst_off + n + 8,), NAN, dtype=torch.bfloat16)
    want[dst_off:dst_off + n] = conv
    exact("cast", f"f32_to_bf16 src+{src_off} dst+{dst_off}", got, want)


@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (1, 0), (0, 3)])
def test_bf16_to_f32_cast_is_exact(capi, src_off, dst_off):
    gen = torch.Generator().manual_seed(7 + src_off + dst_off)
    sp = special_f32().to(torch.bfloat16)
    x = torch.cat([sp, bf(gen, 1003, scale=100.0), sp])
    n = x.numel()
    src = torch.cat([torch.zeros(src_off, dtype=torch.bfloat16), x, torch.zeros(5, dtype=torch.bfloat16)]).cuda()
    dst = nan_buf(dst_off + n + 8)
    got, = run(capi, lambda: capi.lib.dfot_op_bf16_to_f32(P(src[src_off:]), P(dst[dst_off:]), n, S()), [dst])
    want = torch.full((dst_off + n + 8,), NAN)
    want[dst_off:dst_off + n] = x.float()
    exact("cast", f"bf16_to_f32 src+{src_off} dst+{dst_off}", got, want)


def test_split_bf16_is_exact(capi):
    """hi = bf16(x), lo = bf16(x - hi): finite values over a wide range of exponents, zeros, ties"""
    gen = torch.Generator().manual_seed(3)
    sp = special_f32()
    sp = sp[torch.isfinite(sp) & (sp.abs() < 3e38)]
    x = torch.cat([sp, torch.randn(2048, generator=gen) * torch.exp2(torch.randint(-40, 40, (2048,), generator=gen).float())])
    x = x[:x.numel() // 8 * 8]
    n = x.numel()
    xd = x.cuda()
    hi, lo = nan_buf(n + 8, dtype=torch.bfloat16), nan_buf(n + 8, dtype=torch.bfloat16)
    ghi, glo = run(capi, lambda: capi.lib.dfot_op_split_bf16(P(xd), P(hi), P(lo), n, S()), [hi, lo])
    whi = x.to(torch.bfloat16)
    wlo = (x - whi.float()).to(torch.bfloat16)
    exact("split_bf16", "split_bf16 hi", ghi, tail(whi, 8))
    exact("split_bf16", "split_bf16 lo", glo, tail(wlo, 8))


# ----------------------------------------------------------------------------------------------------------- layout ops (exact)

def test_transpose_bf16_is_exact(capi):
    gen = torch.Generator().manual_seed(4)
    r, c = 192, 320
    x = bf(gen, r, c)
    xd = x.cuda()
    out = nan_buf(r * c + 64, dtype=torch.bfloat16)
    got, = run(capi, lambda: capi.lib.dfot_op_transpose_bf16(P(xd), P(out), r, c, S()), [out])
    exact("layout", "transpose_bf16 192x320", got, tail(x.t().contiguous(), 64))


@pytest.mark.parametrize("dgrad", [0, 1])
def test_pack_conv3_is_exact(capi, dgrad):
    gen = torch.Generator().manual_seed(5 + dgrad)
    co, ci = 24, 40
    w = torch.randn(co, ci, 3, 3, generator=gen)
    wd = w.cuda()
    out = nan_buf(co * ci * 9 + 16, dtype=torch.bfloat16)
    got, = run(capi, lambda: capi.lib.dfot_op_pack_conv3(P(wd), P(out), co, ci, dgrad, S()), [out])
    wf = w.view(co, ci, 9)
    # forward layout [Co][tap][Ci]; data-gradient layout [Ci][tap'][Co] with the taps mirrored (tap' = 8 - tap)
    want = wf.permute(0, 2, 1) if not dgrad else wf.flip(2).permute(1, 2, 0)
    exact("layout", f"pack_conv3 dgrad={dgrad}", got, tail(want.contiguous().to(torch.bfloat16), 16))


@pytest.mark.parametrize("bt,res,cdim,kpad", [(2, 256, 180, 768), (3, 8, 40, 164)])
def test_cond_repack_is_exact(capi, bt, res, cdim, kpad):
    """cond [BT][cdim][R][R] -> patch rows [(bt, py, px)][c * 4 + dy * 2 + dx] bf16 with row pitch kpad; columns [4 cdim, kpad) untouched
    (256 / 180 / 768: the production call)"""
    gen = torch.Generator().manual_seed(res + cdim)
    cond = torch.randn(bt, cdim, res, res, generator=gen)
    cd = cond.cuda()
    r0 = res // 2
    out = nan_buf(bt * r0 * r0, kpad, dtype=torch.bfloat16)
    got, = run(capi, lambda: capi.lib.dfot_op_cond_repack(P(cd), P(out), bt, res, cdim, kpad, S()), [out])
    want = torch.full((bt * r0 * r0, kpad), NAN, dtype=torch.bfloat16)
    want[:, :4 * cdim] = cond.view(bt, cdim, r0, 2, r0, 2).permute(0, 2, 4, 1, 3, 5).reshape(bt * r0 * r0, 4 * cdim).to(torch.bfloat16)
    exact("layout", f"cond_repack bt={bt} res={res} cdim={cdim} kpad={kpad}", got, want)


@pytest.mark.parametrize("cout,ps", [(3, 2), (2, 4), (4, 4)])
def test_outgrad_gather_is_exact(capi, cout, ps):
    """dout [BT][cout][R][R] -> dpatch [pix][64] bf16, column (co, py, px); columns >= cout ps^2 are zeroed"""
    gen = torch.Generator().manual_seed(11 + cout + ps)
    bt, res = 2, 24
    g = res // ps
    dout = torch.randn(bt, cout, res, res, generator=gen)
    dd = dout.cuda()
    pix = bt * g * g
    out = nan_buf(pix * 64 + 32, dtype=torch.bfloat16)
    got, = run(capi, lambda: capi.lib.dfot_op_outgrad_gather(P(dd), P(out), bt, res, cout, ps, S()), [out])
    want = torch.zeros(pix, 64, dtype=torch.bfloat16)
    n = cout * ps * ps
    want[:, :n] = dout.view(bt, cout, g, ps, g, ps).permute(0, 2, 4, 1, 3, 5).reshape(pix, n).to(torch.bfloat16)
    exact("layout", f"outgrad_gather cout={cout} ps={ps}", got, tail(want, 32))


def test_mul_cols_is_exact(capi):
    """dst[:, dcol0 : dcol0 + ncols] *= mask (one bf16 rounding of an exact fp32 product); the other columns untouched"""
    gen = torch.Generator().manual_seed(12)
    rows, ldd, dcol0, ncols = 37, 72, 16, 40
    blk = bf(gen, rows, ncols, scale=3.0)
    mask = (torch.rand(rows, ncols, generator=gen) > 0.3).to(torch.bfloat16) * torch.tensor(1 / 0.7).to(torch.bfloat16)
    mask[0, :8] = torch.tensor([0.0, -0.0, 1.0, 3.0, 1e-3, 7.5, -2.0, 0.5]).to(torch.bfloat16)
    dst = nan_buf(rows, ldd, dtype=torch.bfloat16)
    dst[:, dcol0:dcol0 + ncols] = blk.cuda()
    md = mask.cuda()
    got, = run(capi, lambda: capi.lib.dfot_op_mul_cols(P(dst), ldd, dcol0, P(md), rows, ncols, S()), [dst])
    want = torch.full((rows, ldd), NAN, dtype=torch.bfloat16)
    want[:, dcol0:dcol0 + ncols] = (blk.float() * mask.float()).to(torch.bfloat16)
    exact("layout", "mul_cols dcol0=16", got, want)


# ------------------------------------------------------------------------------------------------------------------- resampling

RESAMPLE = [(2, 6, 10, 4), (3, 8, 4, 12), (2, 16, 12, 128)]  # bt, fine h, fine w, c: non-square, c = 4 / 12 / 128


def pool_ref(x):
    bt, h, w, c = x.shape
    v = x.double().view(bt, h // 2, 2, w // 2, 2, c)
    return v.sum((2, 4)) / 4, v.abs().sum((2, 4)) / 4


def up(t):
    return t.repeat_interleave(2, 1).repeat_interleave(2, 2)


@pytest.mark.parametrize("bt,h,w,c", RESAMPLE)
def test_pool2_bf16(capi, bt, h, w, c):
    gen = torch.Generator().manual_seed(h * w + c)
    x = torch.randn(bt, h, w, c, generator=gen) * 2
    xd = x.cuda()
    n = bt * (h // 2) * (w // 2) * c
    out = nan_buf(n + 16, dtype=torch.bfloat16)
    got, = run(capi, lambda: capi.lib.dfot_op_pool2_bf16(P(xd), P(out), bt, h, w, c, S()), [out])
    ref, mag = pool_ref(x)
    check("pool2_bf16", f"pool2_bf16 {bt}x{h}x{w}x{c}", got, tail(ref, 16), tail(seq_bar(3, mag, ref), 16), nulp=1)


@pytest.mark.parametrize("bt,h,w,c", RESAMPLE)
def test_pool2_bwd_accumulates(capi, bt, h, w, c):
    """dx += up(dp) / 4 on the fine map (h, w): dx starts non-zero"""
    gen = torch.Generator().manual_seed(2 * h * w + c)
    dp = torch.randn(bt, h // 2, w // 2, c, generator=gen)
    dx0 = torch.randn(bt, h, w, c, generator=gen)
    dpd = dp.cuda()
    dx = torch.cat([dx0.flatten(), torch.full((16,), NAN)]).cuda()
    got, = run(capi, lambda: capi.lib.dfot_op_pool2_bwd(P(dpd), P(dx), bt, h, w, c, S()), [dx])
    ref = dx0.double() + up(dp.double()) / 4
    mag = dx0.double().abs() + up(dp.double()).abs() / 4
    check("resample_f32", f"pool2_bwd {bt}x{h}x{w}x{c}", got, tail(ref, 16), tail(seq_bar(1, mag, ref), 16))


@pytest.mark.parametrize("bt,h,w,c", RESAMPLE)
def test_upsample_add_takes_the_coarse_size(capi, bt, h, w, c):
    """out = up(t) + skip, with (h, w) the COARSE map's size"""
    gen = torch.Generator().manual_seed(3 * h * w + c)
    hc, wc = h // 2, w // 2
    t = torch.randn(bt, hc, wc, c, generator=gen)
    skip = torch.randn(bt, h, w, c, generator=gen)
    td, sd = t.cuda(), skip.cuda()
    out = nan_buf(bt * h * w * c + 16)
    got, = run(capi, lambda: capi.lib.dfot_op_upsample_add(P(td), P(sd), P(out), bt, hc, wc, c, S()), [out])
    ref = up(t.double()) + skip.double()
    mag = up(t.double()).abs() + skip.double().abs()
    check("resample_f32", f"upsample_add coarse {bt}x{hc}x{wc}x{c}", got, tail(ref, 16), tail(seq_bar(1, mag, ref), 16))


@pytest.mark.parametrize("bt,h,w,c", RESAMPLE)
def test_upsample_bwd_takes_the_fine_size(capi, bt, h, w, c):
    """ds = 2x2 block sums of dy, with (h, w) the FINE map's size"""
    gen = torch.Generator().manual_seed(4 * h * w + c)
    dy = torch.randn(bt, h, w, c, generator=gen)
    dyd = dy.cuda()
    out = nan_buf(bt * (h // 2) * (w // 2) * c + 16)
    got, = run(capi, lambda: capi.lib.dfot_op_upsample_bwd(P(dyd), P(out), bt, h, w, c, S()), [out])
    ref, mag = pool_ref(dy)
    check("resample_f32", f"upsample_bwd fine {bt}x{h}x{w}x{c}", got, tail(4 * ref, 16), tail(seq_bar(2, 4 * mag, 4 * ref), 16))


@pytest.mark.parametrize("bt,h,w,c", RESAMPLE)
def test_resampling_adjoints(capi, bt, h, w, c):
    """<pool(x), g> = <x, pool_bwd(g)> and <up(t), dy> = <t, upsample_bwd(dy)> in fp64 over the device outputs: a swapped index in one
    direction only breaks the identity"""
    gen = torch.Generator().manual_seed(5 * h * w + c)
    x, g = torch.randn(bt, h, w, c, generator=gen), torch.randn(bt, h // 2, w // 2, c, generator=gen)
    pooled = nan_buf(g.numel(), dtype=torch.bfloat16)
    dx = torch.zeros(bt, h, w, c, device="cuda")
    xd, gd = x.cuda(), g.cuda()
    capi.check(capi.lib.dfot_op_pool2_bf16(P(xd), P(pooled), bt, h, w, c, S()))
    capi.check(capi.lib.dfot_op_pool2_bwd(P(gd), P(dx), bt, h, w, c, S()))
    lhs = (pooled.cpu().double().view_as(g) * g.double()).sum().item()
    rhs = (x.double() * dx.cpu().double()).sum().item()        # dx = g / 4 exactly: rhs is <x, pool^T g> to fp64 rounding
    pr, pm = pool_ref(x)
    bar = ((ulp_bf16(pr) + 3 * U * pm) * g.double().abs()).sum().item()
    ratio = abs(lhs - rhs) / bar
    print(f"pool adjoint {bt}x{h}x{w}x{c}: {ratio:.3f}")
    record("resample_adjoint", f"pool {bt}x{h}x{w}x{c}", ratio)
    assert ratio <= 1.0
    t, dy = g, torch.randn(bt, h, w, c, generator=gen)
    zero = torch.zeros(bt, h, w, c, device="cuda")
    upt, ds = nan_buf(bt, h, w, c), nan_buf(bt, h // 2, w // 2, c)
    td, dyd = t.cuda(), dy.cuda()
    capi.check(capi.lib.dfot_op_upsample_add(P(td), P(zero), P(upt), bt, h // 2, w // 2, c, S()))
    capi.check(capi.lib.dfot_op_upsample_bwd(P(dyd), P(ds), bt, h, w, c, S()))
    lhs = (upt.cpu().double() * dy.double()).sum().item()
    rhs = (t.double() * ds.cpu().double()).sum().item()
    _, dm = pool_ref(dy)
    bar = (2 * U * 4 * dm * t.double().abs()).sum().item() + 1e-12 * abs(lhs)
    ratio = abs(lhs - rhs) / bar
    print(f"upsample adjoint {bt}x{h}x{w}x{c}: {ratio:.3f}")
    record("resample_adjoint", f"upsample {bt}x{h}x{w}x{c}", ratio)
    assert ratio <= 1.0


def test_sub_bf16(capi):
    gen = torch.Generator().manual_seed(13)
    n = 4 * 1001
    a, b = torch.randn(n, generator=gen) * 3, torch.randn(n, generator=gen)
    b[:8] = a[:8]                                                   # exact cancellation
    ad, bd = a.cuda(), b.cuda()
    out = nan_buf(n + 8, dtype=torch.bfloat16)
    got, = run(capi, lambda: capi.lib.dfot_op_sub_bf16(P(ad), P(bd), P(out), n, S()), [out])
    ref = a.double() - b.double()
    check("sub_bf16", "sub_bf16 n=4004", got, tail(ref, 8), tail(seq_bar(1, a.double().abs() + b.double().abs(), ref), 8), nulp=1)


@pytest.mark.parametrize("r0,e", [(8, 8), (64, 768)])
def test_emb_pyramid(capi, r0, e):
    """avg_pool2d by 2, 4, 8 of the level-0 embedding map (bf16 [BT][r0][r0][e]) in one pass"""
    gen = torch.Generator().manual_seed(r0 + e)
    bt = 2
    e0 = bf(gen, bt, r0, r0, e)
    ed = e0.cuda()
    outs = [nan_buf(bt * (r0 >> lv) ** 2 * e + 8, dtype=torch.bfloat16) for lv in (1, 2, 3)]
    got = run(capi, lambda: capi.lib.dfot_op_emb_pyramid(P(ed), P(outs[0]), P(outs[1]), P(outs[2]), bt, r0, e, S()), outs)
    x = e0.double()
    for lv, g in zip((1, 2, 3), got):
        k = 1 << lv
        v = x.view(bt, r0 // k, k, r0 // k, k, e)
        ref, mag = v.sum((2, 4)) / k ** 2, v.abs().sum((2, 4)) / k ** 2
        check("emb_pyramid", f"emb_pyramid r0={r0} e={e} level {lv}", g, tail(ref, 8), tail(seq_bar(k * k - 1, mag, ref), 8), nulp=1)


# ----------------------------------------------------------------------------------------------------- patch embedding / output

def patches(x, ps=2):
    """x [BT][Cin][R][R] -> [(bt, gy, gx)][(ci, py, px)] (the flatten order of a Conv2d weight)"""
    bt, cin, res, _ = x.shape
    g = res // ps
    return x.reshape(bt, cin, g, ps, g, ps).permute(0, 2, 4, 1, 3, 5).reshape(bt * g * g, cin * ps * ps)


# (bt, res, cin, c0): cin = 3 and 256 % (c0 / 4) == 0 take the register-weight kernel (grid capped at 4096 workgroups: bt = 3 at 256 runs a
# second, partial pass), the others the LDS-staged one
EMBED = [(2, 24, 3, 128), (3, 256, 3, 128), (2, 20, 3, 192), (2, 16, 4, 128), (1, 12, 3, 64)]


@pytest.mark.parametrize("bt,res,cin,c0", EMBED)
def test_embed_input(capi, bt, res, cin, c0):
    gen = torch.Generator().manual_seed(res + cin + c0)
    x = torch.randn(bt, cin, res, res, generator=gen)
    w = torch.randn(c0, cin, 2, 2, generator=gen) * 0.5
    b = torch.randn(c0, generator=gen)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    rows = bt * (res // 2) ** 2
    out = nan_buf(rows * c0 + 64)
    got, = run(capi, lambda: capi.lib.dfot_op_embed_input(P(xd), P(wd), P(bd), P(out), bt, res, cin, c0, S()), [out])
    pt, wm = patches(x.double()), w.double().view(c0, -1)
    ref = pt @ wm.t() + b.double()
    mag = pt.abs() @ wm.abs().t() + b.double().abs()
    check("embed_input", f"embed_input bt={bt} res={res} cin={cin} c0={c0}", got, tail(ref, 64), tail(seq_bar(4 * cin + 1, mag, ref), 64))


# (bt, res, c0, cout): c0 = 128 / cout = 3 takes the 16-lanes-per-pixel kernel (4096 workgroups = 65536 pixels per pass: bt = 5 at 256 has
# 81920 pixels, a second partial pass), everything else the generic one
PROJECT = [(2, 16, 128, 3), (5, 256, 128, 3), (2, 16, 64, 1), (2, 16, 256, 2), (3, 10, 64, 3), (2, 16, 128, 2)]


@pytest.mark.parametrize("bt,res,c0,cout", PROJECT)
def test_project_output(capi, bt, res, c0, cout):
    gen = torch.Generator().manual_seed(res + c0 + cout)
    r0 = res // 2
    x0 = torch.randn(bt * r0 * r0, c0, generator=gen)
    w = torch.randn(c0, cout, 2, 2, generator=gen) / math.sqrt(c0)
    b = torch.randn(cout, generator=gen)
    xd, wd, bd = x0.cuda(), w.cuda(), b.cuda()
    out = nan_buf(bt * cout * res * res + 64)
    got, = run(capi, lambda: capi.lib.dfot_op_project_output(P(xd), P(wd), P(bd), P(out), bt, res, c0, cout, S()), [out])
    wm = w.double().view(c0, cout * 4)

    def unpatch(y):  # [(bt, py, px)][(co, dy, dx)] -> [BT][cout][R][R]
        return y.view(bt, r0, r0, cout, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(bt, cout, res, res)
    ref = unpatch(x0.double() @ wm + b.double().repeat_interleave(4))
    mag = unpatch(x0.double().abs() @ wm.abs() + b.double().abs().repeat_interleave(4))
    check("project_output", f"project_output bt={bt} res={res} c0={c0} cout={cout}", got, tail(ref, 64), tail(seq_bar(c0 + 1, mag, ref), 64))


# (bt, res, cin, c0, ps): rows = bt (res / ps)^2 in the launcher's three chunk regimes -- < 131072 rows: 1 chunk of 64 rows per workgroup;
# [131072, 524288): 4; >= 524288: 16 -- each with a row count that is no multiple of 64 chunks; plus a patch of 4 (kdim 48 > 16: no
# register accumulation over chunks) and c0 = 64 (4 thread groups per workgroup)
WGRAD = [(3, 34, 3, 128, 2), (9, 250, 3, 128, 2), (34, 250, 3, 128, 2), (2, 32, 3, 64, 4), (2, 18, 4, 64, 2)]


@pytest.mark.parametrize("bt,res,cin,c0,ps", WGRAD)
def test_embed_input_wgrad(capi, bt, res, cin, c0, ps):
    gen = torch.Generator().manual_seed(bt + res + cin + c0 + ps)
    g = res // ps
    rows, kdim = bt * g * g, cin * ps * ps
    x = torch.randn(bt, cin, res, res, generator=gen)
    dx0 = torch.randn(rows, c0, generator=gen)
    xd, dd = x.cuda(), dx0.cuda()
    dw, db = nan_buf(c0 * kdim + 16), nan_buf(c0 + 16)
    gdw, gdb = run(capi, lambda: capi.lib.dfot_op_embed_input_wgrad(P(dd), P(xd), P(dw), P(db), bt, res, cin, c0, ps, S()), [dw, db])
    pt = patches(x, ps)
    ref_w, mag_w = torch.zeros(c0, kdim, dtype=torch.float64), torch.zeros(c0, kdim, dtype=torch.float64)
    ref_b, mag_b = torch.zeros(c0, dtype=torch.float64), torch.zeros(c0, dtype=torch.float64)
    for r in range(0, rows, 1 << 16):                          # fp64 in row blocks (the largest case has 531250 rows)
        gd, pd = dx0[r:r + (1 << 16)].double(), pt[r:r + (1 << 16)].double()
        ref_w += gd.t() @ pd
        mag_w += gd.abs().t() @ pd.abs()
        ref_b += gd.sum(0)
        mag_b += gd.abs().sum(0)
    if rows <= 4096:  # the patch form is the fp64 autograd gradient of conv2d(k = s = ps)
        xr, wr, br = x.double(), torch.zeros(c0, cin, ps, ps, dtype=torch.float64, requires_grad=True), torch.zeros(c0, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(xr, wr, br, stride=ps)
        y.backward(dx0.double().view(bt, g, g, c0).permute(0, 3, 1, 2))
        assert torch.allclose(wr.grad.view(c0, kdim), ref_w, rtol=1e-12, atol=1e-12) and torch.allclose(br.grad, ref_b, rtol=1e-12, atol=1e-12)
    chunks = 1 if kdim > 16 else (16 if rows >= 64 * 16 * 512 else (4 if rows >= 64 * 4 * 512 else 1))
    nsub = 256 // c0 if c0 < 256 and 256 % c0 == 0 else 1
    parts = -(-rows // (64 * chunks)) * nsub
    c = 64 * chunks + -(-parts // 16) + 4
    tag = f"embed_input_wgrad rows={rows} chunks={chunks} kdim={kdim} c0={c0}"
    check("embed_input_wgrad", tag + " dw", gdw, tail(ref_w, 16), tail(seq_bar(c, mag_w, ref_w), 16))
    check("embed_input_wgrad", tag + " db", gdb, tail(ref_b, 16), tail(seq_bar(c, mag_b, ref_b), 16))


# ------------------------------------------------------------------------------------------------------------------- reductions

def colsum_plan(rows, n, vector):
    """(iters, partial rows) of launch_colsum_bf16"""
    if not vector:
        return 1, -(-rows // 128)
    xb = -(-n // 128) if n <= 128 else -(-n // 256)
    yb = -(-rows // 128)
    iters = 1
    while iters < 16 and yb // iters * xb > 2048:
        iters *= 2
    return iters, -(-yb // iters)


# (rows, n, ld, source offset in elements): the vector path with iters 1, 2 and 4 at n = 1152 (5 column blocks), n <= 128 (16 lanes per
# row), a column block of a wider matrix (ld > n); the scalar fallback for odd n and for a source that is not 16-byte aligned
COLSUM = [(3000, 1152, 1152, 0), (63963, 1152, 1152, 0), (110001, 1152, 1160, 0), (1000, 64, 72, 0), (777, 63, 63, 0), (1500, 1152, 1160, 1)]


@pytest.mark.parametrize("rows,n,ld,off", COLSUM)
def test_colsum_bf16(capi, rows, n, ld, off):
    gen = torch.Generator().manual_seed(rows + n + off)
    src = bf(gen, rows * ld + off + 8)
    src[off:off + rows * ld].view(rows, ld)[:5, :n] = torch.tensor(1000.0).to(torch.bfloat16)  # a few large values: cancellation is not
    src[off:off + rows * ld].view(rows, ld)[5:10, :n] = torch.tensor(-1000.0).to(torch.bfloat16)  # the only error source
    sd = src.cuda()
    out = nan_buf(n + 8)
    got, = run(capi, lambda: capi.lib.dfot_op_colsum_bf16(P(sd[off:]), ld, P(out), rows, n, S()), [out])
    m = src[off:off + rows * ld].view(rows, ld)[:, :n]
    ref, mag = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for r in range(0, rows, 1 << 15):
        blk = m[r:r + (1 << 15)].double()
        ref += blk.sum(0)
        mag += blk.abs().sum(0)
    vector = n % 8 == 0 and ld % 8 == 0 and off % 8 == 0
    iters, parts = colsum_plan(rows, n, vector)
    if (rows, n) == (3000, 1152):
        assert iters == 1
    if (rows, n) == (63963, 1152):
        assert iters == 2
    if (rows, n) == (110001, 1152):
        assert iters == 4
    c = 128 * iters + -(-parts // 16) + 4
    check("colsum_bf16", f"colsum_bf16 rows={rows} n={n} ld={ld} off={off} {'vector' if vector else 'scalar'} iters={iters}", got,
          tail(ref, 8), tail(seq_bar(c, mag, ref), 8))


# (bt, pixels, n, ld): pixels < 16 (one chunk); pixels not a multiple of the chunk count; the production size (16 frames of 128^2, n = 256)
FRAME_SUMS = [(3, 9, 64, 72), (2, 1000, 256, 264), (16, 16384, 256, 256)]


@pytest.mark.parametrize("bt,pixels,n,ld", FRAME_SUMS)
def test_frame_sums_bf16(capi, bt, pixels, n, ld):
    gen = torch.Generator().manual_seed(bt + pixels + n)
    src = bf(gen, bt * pixels, ld)
    sd = src.cuda()
    out = nan_buf(bt * n + 8)
    got, = run(capi, lambda: capi.lib.dfot_op_frame_sums_bf16(P(sd), ld, P(out), bt, pixels, n, S()), [out])
    v = src[:, :n].double().view(bt, pixels, n)
    ref, mag = v.sum(1), v.abs().sum(1)
    xb = -(-(n // 8) // 256)
    nz = max(1, min(2048 // (xb * bt), pixels // 16))
    if pixels == 1000:
        assert pixels % nz != 0
    c = -(-pixels // nz) + -(-nz // 16) + 4
    check("frame_sums_bf16", f"frame_sums bt={bt} pixels={pixels} n={n} nz={nz}", got, tail(ref, 8), tail(seq_bar(c, mag, ref), 8))


def test_axpy(capi):
    """a += alpha b: both pointers 16-byte aligned with n % 4 = 3 (vector kernel + scalar tail), then a and b offset by one float (scalar)"""
    gen = torch.Generator().manual_seed(14)
    n, alpha = 1027, -0.7
    for off_a, off_b in ((0, 0), (1, 0), (0, 1)):
        a0, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        abuf = torch.cat([torch.full((off_a,), NAN), a0, torch.full((8,), NAN)]).cuda()
        bbuf = torch.cat([torch.zeros(off_b), b]).cuda()
        got, = run(capi, lambda: capi.lib.dfot_op_axpy(P(abuf[off_a:]), P(bbuf[off_b:]), alpha, n, S()), [abuf])
        al = float(torch.tensor(alpha, dtype=torch.float32))
        ref = a0.double() + al * b.double()
        mag = a0.double().abs() + abs(al) * b.double().abs()
        check("axpy", f"axpy n={n} a+{off_a} b+{off_b}", got, torch.cat([torch.full((off_a,), NAN, dtype=torch.float64), tail(ref, 8)]),
              torch.cat([torch.zeros(off_a, dtype=torch.float64), tail(seq_bar(2, mag, ref), 8)]))


# ---------------------------------------------------------------------------------------------------------------------- sgemm

def sgemm_case(capi, name, m, n, k, a_store, b_store, accumulate, ldc_pad=0, seed=0):
    """a_store / b_store: 'row' (A [M][K], B [K][N]), 'col' (the transposed storage) or 'strided' (every 2nd row and 3rd column of a
    wider buffer: neither stride is 1)"""
    gen = torch.Generator().manual_seed(seed)

    def operand(rows, cols, store):
        if store == "row":
            buf = torch.randn(rows, cols, generator=gen)
            return buf, buf.cuda(), cols, 1
        if store == "col":
            buf = torch.randn(cols, rows, generator=gen)
            return buf.t(), buf.cuda(), 1, rows
        buf = torch.randn(2 * rows, 3 * cols, generator=gen)
        return buf[::2, ::3], buf.cuda(), 6 * cols, 3
    a, ad, sa_i, sa_k = operand(m, k, a_store)
    b, bd, sb_k, sb_j = operand(k, n, b_store)
    ldc = n + ldc_pad
    c0 = torch.randn(m, n, generator=gen)
    init = torch.full((m, ldc), NAN)
    if accumulate:
        init[:, :n] = c0
    cd = init.cuda()
    got, = run(capi, lambda: capi.lib.dfot_op_sgemm(P(ad), sa_i, sa_k, P(bd), sb_k, sb_j, P(cd), ldc, m, n, k, accumulate, S()), [cd])
    ref, mag = a.double() @ b.double(), a.double().abs() @ b.double().abs()
    if accumulate:
        ref, mag = ref + c0.double(), mag + c0.double().abs()
    exp, bar = torch.full((m, ldc), NAN, dtype=torch.float64), torch.zeros(m, ldc, dtype=torch.float64)
    exp[:, :n], bar[:, :n] = ref, seq_bar(k + accumulate, mag, ref)
    check("sgemm", f"sgemm {name} {m}x{n}x{k} acc={accumulate} ldc={ldc}", got, exp, bar)


@pytest.mark.parametrize("a_store", ["row", "col", "strided"])
@pytest.mark.parametrize("b_store", ["row", "col", "strided"])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_sgemm_orientations(capi, a_store, b_store, accumulate):
    seed = 3 * ["row", "col", "strided"].index(a_store) + ["row", "col", "strided"].index(b_store)
    sgemm_case(capi, f"A {a_store} B {b_store}", 70, 93, 45, a_store, b_store, accumulate, ldc_pad=7, seed=seed)


def test_sgemm_long_k(capi):
    sgemm_case(capi, "K=4096", 67, 50, 4096, "row", "col", 0, ldc_pad=3, seed=15)


# ------------------------------------------------------------------------------------------------------------- transformer pieces

def rms64(x, w, eps=1e-6):
    """fp64 RMSNorm over the last axis (oracle.uvit.rms_norm's formula, kept in fp64) and 1 / rms"""
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    return x * r * w, r


@pytest.mark.parametrize("c", [128, 256, 576, 1152, 192, 320])
def test_rms_film_fwd(capi, c):
    """every channel count of DIT_LN_DISPATCH the UViT uses, plus two odd multiples of 64 (the one-float-per-lane kernels); rows % 4 != 0"""
    gen = torch.Generator().manual_seed(c)
    rows = 37
    x = torch.randn(rows, c, generator=gen) * 2
    w = torch.randn(c, generator=gen) * 0.3 + 1
    film = bf(gen, rows, 2 * c, scale=0.5)
    xd, wd, fd = x.cuda(), w.cuda(), film.cuda()
    out = nan_buf(rows * c + 16, dtype=torch.bfloat16)
    got, = run(capi, lambda: capi.lib.dfot_op_rms_film_fwd(P(xd), P(wd), P(fd), 1e-6, P(out), rows, c, S()), [out])
    y, _ = rms64(x.double(), w.double())
    sc, sh = film[:, :c].double(), film[:, c:].double()
    ref = y * (1 + sc) + sh
    bar = 32 * U * (y * (1 + sc)).abs() + U * sh.abs() + U * ref.abs()
    check("rms_film_fwd", f"rms_film_fwd C={c} rows={rows}", got, tail(ref, 16), tail(bar, 16), nulp=2)


def rms_film_bwd_ref(x, dxn, w, film, c):
    xr, wr, fr = x.double().requires_grad_(), w.double().requires_grad_(), film.double().requires_grad_()
    y, r = rms64(xr, wr)
    (y * (1 + fr[:, :c]) + fr[:, c:]).backward(dxn.double())
    g = dxn.double() * (1 + film[:, :c].double()) * w.double()
    xd = x.double()
    rr = r.detach()
    mag_dx = (g.abs() + xd.abs() * (g * xd).abs().mean(-1, keepdim=True) * rr ** 2) * rr
    mag_dw = (dxn.double() * (1 + film[:, :c].double())).abs().mul(xd.abs() * rr).sum(0)
    return xr.grad, wr.grad, fr.grad, mag_dx, mag_dw, (y * 1).detach()


@pytest.mark.parametrize("rows,c", [(37, 576), (300, 128)])
def test_rms_film_bwd_accumulates_dx(capi, rows, c):
    """accumulate_dx = 1: dx = dx0 + the norm's input gradient"""
    gen = torch.Generator().manual_seed(rows + c)
    x, dxn, dx0 = torch.randn(rows, c, generator=gen) * 2, torch.randn(rows, c, generator=gen), torch.randn(rows, c, generator=gen)
    w = torch.randn(c, generator=gen) * 0.3 + 1
    film = bf(gen, rows, 2 * c, scale=0.5)
    dev = [t.cuda() for t in (x, dxn, w, film)]
    dx = torch.cat([dx0.flatten(), torch.full((16,), NAN)]).cuda()
    dfilm, dw = nan_buf(rows * 2 * c + 16, dtype=torch.bfloat16), nan_buf(c + 16)
    gdx, gdf, gdw = run(capi, lambda: capi.lib.dfot_op_rms_film_bwd(P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), 1e-6, P(dx), P(dfilm), P(dw),
                                                                     rows, c, 1, S()), [dx, dfilm, dw])
    gx, gw, gf, mdx, mdw, y = rms_film_bwd_ref(x, dxn, w, film, c)
    tag = f"rms_film_bwd acc C={c} rows={rows}"
    ref = dx0.double() + gx
    check("rms_film_bwd", tag + " dx", gdx, tail(ref, 16), tail(64 * U * mdx + U * dx0.double().abs() + U * ref.abs(), 16))
    check("rms_film_bwd", tag + " dw", gdw, tail(gw, 16), tail(seq_bar(rows + 32, mdw, gw), 16))
    dfl_bar = torch.cat([8 * U * (dxn.double() * y).abs(), torch.zeros(rows, c, dtype=torch.float64)], 1)
    check("rms_film_bwd", tag + " dfilm", gdf, tail(gf, 16), tail(dfl_bar, 16), nulp=1)


@pytest.mark.parametrize("with_bf", [True, False])
def test_rms_film_bwd_res(capi, with_bf):
    """dx = dres + the norm's input gradient out of place; dres bit-untouched; dx_bf (optional) the bf16 rounding of dx"""
    gen = torch.Generator().manual_seed(16 + with_bf)
    rows, c = 41, 256
    x, dxn, dres = torch.randn(rows, c, generator=gen) * 2, torch.randn(rows, c, generator=gen), torch.randn(rows, c, generator=gen)
    w = torch.randn(c, generator=gen) * 0.3 + 1
    film = bf(gen, rows, 2 * c, scale=0.5)
    dev = [t.cuda() for t in (x, dxn, w, film, dres)]
    dx, dfilm, dw = nan_buf(rows * c + 16), nan_buf(rows * 2 * c + 16, dtype=torch.bfloat16), nan_buf(c + 16)
    dxb = nan_buf(rows * c + 16, dtype=torch.bfloat16) if with_bf else None
    outs = [dx, dfilm, dw, dev[4]] + ([dxb] if with_bf else [])
    got = run(capi, lambda: capi.lib.dfot_op_rms_film_bwd_res(P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), 1e-6, P(dev[4]), P(dx), P(dxb),
                                                               P(dfilm), P(dw), rows, c, S()), outs)
    gx, gw, gf, mdx, mdw, y = rms_film_bwd_ref(x, dxn, w, film, c)
    tag = f"rms_film_bwd_res dx_bf={with_bf}"
    ref = dres.double() + gx
    check("rms_film_bwd", tag + " dx", got[0], tail(ref, 16), tail(64 * U * mdx + U * dres.double().abs() + U * ref.abs(), 16))
    check("rms_film_bwd", tag + " dw", got[2], tail(gw, 16), tail(seq_bar(rows + 32, mdw, gw), 16))
    assert torch.equal(bits(got[3]), bits(dres)), "dres was modified"
    if with_bf:
        exact("rms_film_bwd_dx_bf", tag + " dx_bf", got[4], tail(got[0][:rows * c].to(torch.bfloat16), 16))


def rope_table(gen, ntok, d):
    ang = torch.rand(ntok, d // 2, generator=gen) * 2 * math.pi
    return torch.stack([ang.cos(), ang.sin()], -1).contiguous()  # [ntok][d/2][cos, sin]


def qk_ref(x, e, wgt, cs, mul):
    """per-head RMSNorm + RoPE of x [b][heads][ntok][d] fp64 (its fp32 error bar e carried through), through oracle.uvit.apply_rope with
    the angles of the device's (cos, sin) table; returns the reference and its bar"""
    from oracle import uvit as ouvit
    y, r = rms64(x, wgt.double())
    ang = torch.atan2(cs[..., 1].double(), cs[..., 0].double()).repeat_interleave(2, -1)
    z = ouvit.apply_rope(y, ang)
    ey = wgt.double().abs() * r * (e + x.abs() * (x.abs() * e).mean(-1, keepdim=True) * r ** 2) + 32 * U * y.abs()
    amp = cs[..., 0].double().abs() + cs[..., 1].double().abs()
    ez = torch.maximum(ey[..., 0::2], ey[..., 1::2]) * amp
    ez = torch.stack([ez, ez], -1).flatten(-2)
    return z * mul, 1.5 * ez * abs(mul) + U * (z * mul).abs()


def heads_view(x, b, ntok, heads, d):
    return x.reshape(b, ntok, heads, d).permute(0, 2, 1, 3)


@pytest.mark.parametrize("d,heads,ntok,batch", [(64, 3, 37, 2), (128, 2, 21, 3)])
def test_qknorm_rope_fwd(capi, d, heads, ntok, batch):
    """fused [rows][ld] (q | k | v head-major, ld > 7C) -> q (RMSNorm, RoPE, * qscale), k (RMSNorm, RoPE), v in [B][heads][ntok][d]"""
    gen = torch.Generator().manual_seed(d + ntok)
    c, rows = heads * d, batch * ntok
    ld = 7 * c + 8
    fused = bf(gen, rows, ld, scale=2.0)
    qw, kw = torch.rand(d, generator=gen) + 0.5, torch.rand(d, generator=gen) + 0.5
    cs = rope_table(gen, ntok, d)
    qscale = 0.3
    dev = [t.cuda() for t in (fused, qw, kw, cs)]
    q, k, v = (nan_buf(batch, heads, ntok, d, dtype=torch.bfloat16) for _ in range(3))
    gq, gk, gv = run(capi, lambda: capi.lib.dfot_op_qknorm_rope_fwd(P(dev[0]), ld, P(dev[1]), P(dev[2]), P(dev[3]), 1e-6, qscale, P(q), P(k), P(v),
                                                                    rows, ntok, heads, d, S()), [q, k, v])
    x = fused.double()
    tag = f"qknorm_rope_fwd d={d} ntok={ntok} batch={batch}"
    for i, (got, wgt, mul) in enumerate([(gq, qw, qscale), (gk, kw, 1.0)]):
        xs = heads_view(x[:, i * c:(i + 1) * c], batch, ntok, heads, d)
        ref, bar = qk_ref(xs, torch.zeros_like(xs), wgt, cs, mul)
        check("qknorm_rope_fwd", f"{tag} {'qk'[i]}", got, ref, bar, nulp=2)
    exact("qknorm_rope_fwd_v", f"{tag} v", gv, heads_view(fused[:, 2 * c:3 * c], batch, ntok, heads, d).contiguous())


def silu(x):
    return x * torch.sigmoid(x)


@pytest.mark.parametrize("d,heads,ntok", [(64, 2, 96), (128, 2, 128)])
def test_fused_proj_train(capi, d, heads, ntok):
    """one launch: fused = a w^T + bias (raw bf16 [rows][7C]), q / k / v, SiLU(mlp) into cat[:, ccol0 : ccol0 + 4C] of a wider matrix (ldcat > 5C);
    against fp64, and against the unfused path (gemm_bf16 -> qknorm_rope_fwd -> silu_cols).  The unfused path rounds the projection to
    bf16 before the norm and the SiLU, so the cross-check bar is 1 ulp + the fp64 difference that rounding makes + both fp32 bars."""
    gen = torch.Generator().manual_seed(d + ntok + 1)
    c = heads * d
    rows = 384 if d == 64 else 256
    batch = rows // ntok
    lda = c + 16
    abuf = bf(gen, rows, lda)
    a = abuf[:, 16:]
    w = bf(gen, 7 * c, c, scale=1 / math.sqrt(c))
    bias = torch.randn(7 * c, generator=gen) * 0.5
    qw, kw = torch.rand(d, generator=gen) + 0.5, torch.rand(d, generator=gen) + 0.5
    cs = rope_table(gen, ntok, d)
    qscale, ccol0, ldcat = 0.125, c, 5 * c + 24
    ad, wd, bd, qwd, kwd, csd = abuf.cuda(), w.cuda(), bias.cuda(), qw.cuda(), kw.cuda(), cs.cuda()
    a_dev = ad[:, 16:]
    fused = nan_buf(rows, 7 * c, dtype=torch.bfloat16)
    q, k, v = (nan_buf(batch, heads, ntok, d, dtype=torch.bfloat16) for _ in range(3))
    cat = nan_buf(rows, ldcat, dtype=torch.bfloat16)
    gf, gq, gk, gv, gc = run(capi, lambda: capi.lib.dfot_op_fused_proj_train(
        P(a_dev), lda, P(wd), P(bd), P(qwd), P(kwd), P(csd), 1e-6, qscale, P(fused), P(q), P(k), P(v), P(cat), ldcat, ccol0, rows, ntok, heads, d,
        S()), [fused, q, k, v, cat])
    acc = a.double() @ w.double().t() + bias.double()
    e = 1e-6 * (a.double().abs() @ w.double().abs().t() + bias.double().abs())
    tag = f"fused_proj_train d={d} ntok={ntok}"
    check("fused_proj_train", tag + " raw", gf, acc, e + 1e-6 * acc.abs(), nulp=1)
    refs = {}
    for i, (got, wgt, mul) in enumerate([(gq, qw, qscale), (gk, kw, 1.0)]):
        xs, es = (heads_view(t[:, i * c:(i + 1) * c], batch, ntok, heads, d) for t in (acc, e))
        refs["qk"[i]] = qk_ref(xs, es, wgt, cs, mul)
        check("fused_proj_train", f"{tag} {'qk'[i]}", got, *refs["qk"[i]], nulp=2)
    vv, ev = (heads_view(t[:, 2 * c:3 * c], batch, ntok, heads, d) for t in (acc, e))
    check("fused_proj_train", tag + " v", gv, vv, ev + 1e-6 * vv.abs(), nulp=1)
    h = silu(acc[:, 3 * c:])
    ecat = torch.full((rows, ldcat), NAN, dtype=torch.float64)
    bcat = torch.zeros(rows, ldcat, dtype=torch.float64)
    ecat[:, ccol0:ccol0 + 4 * c], bcat[:, ccol0:ccol0 + 4 * c] = h, 1.2 * e[:, 3 * c:] + 64 * U * h.abs()
    check("fused_proj_train", tag + " cat", gc, ecat, bcat, nulp=2)

    # the unfused path DFOT_TRAIN_FUSED_PROJ=0 selects
    ufused = nan_buf(rows, 7 * c, dtype=torch.bfloat16)
    uq, uk, uv = (nan_buf(batch, heads, ntok, d, dtype=torch.bfloat16) for _ in range(3))
    ucat = nan_buf(rows, ldcat, dtype=torch.bfloat16)
    capi.check(capi.lib.dfot_op_gemm_bf16(P(a_dev), lda, P(wd), P(bd), P(ufused), 7 * c, rows, 7 * c, c, S()))
    capi.check(capi.lib.dfot_op_qknorm_rope_fwd(P(ufused), 7 * c, P(qwd), P(kwd), P(csd), 1e-6, qscale, P(uq), P(uk), P(uv), rows, ntok, heads, d, S()))
    capi.check(capi.lib.dfot_op_silu_cols(P(ufused), 7 * c, 3 * c, None, 0, 0, P(ucat), ldcat, ccol0, rows, 4 * c, S()))
    ufh = ufused.cpu()

    def close(name, got, ugot, extra):
        """|fused - unfused| <= 1 ulp of the larger + extra"""
        g, ug = got.double(), ugot.double()
        ratio = ((g - ug).abs() / (ulp_bf16(torch.maximum(g.abs(), ug.abs())) + extra)).max().item()
        print(f"{tag} {name} fused vs unfused: {ratio:.3f}")
        record("fused_vs_unfused", f"{tag} {name}", ratio)
        assert ratio <= 1.0, name
    close("raw", gf, ufh, 2 * e + 2e-6 * acc.abs())               # the same product on two GEMM tile forms
    xr = ufh.double()                                            # the projection as the unfused path sees it
    for i, (got, ugot, wgt, mul) in enumerate([(gq, uq, qw, qscale), (gk, uk, kw, 1.0)]):
        ref_u, bar_u = qk_ref(heads_view(xr[:, i * c:(i + 1) * c], batch, ntok, heads, d), torch.zeros(batch, heads, ntok, d, dtype=torch.float64),
                              wgt, cs, mul)
        ref_f, bar_f = refs["qk"[i]]
        close("qk"[i], got, ugot.cpu(), (ref_f - ref_u).abs() + bar_f + bar_u)
    vv2 = heads_view(2 * e[:, 2 * c:3 * c] + 2e-6 * acc[:, 2 * c:3 * c].abs(), batch, ntok, heads, d)
    close("v", gv, uv.cpu(), vv2)
    hu = silu(xr[:, 3 * c:])
    gcu, gcf = ucat.cpu()[:, ccol0:ccol0 + 4 * c], gc[:, ccol0:ccol0 + 4 * c]
    close("cat", gcf, gcu, (h - hu).abs() + 1.2 * e[:, 3 * c:] + 64 * U * (h.abs() + hu.abs()))
    assert torch.isnan(ucat.cpu()[:, :ccol0].float()).all() and torch.isnan(ucat.cpu()[:, ccol0 + 4 * c:].float()).all()


@pytest.mark.parametrize("grad", [False, True])
def test_silu_cols(capi, grad):
    """dst[:, dcol0:] = SiLU(src[:, scol0:]) or grad[:, gcol0:] * SiLU'(src[:, scol0:]), column offsets on all three operands, saturated
    inputs up to |x| = 30"""
    gen = torch.Generator().manual_seed(17 + grad)
    rows, ncols = 33, 48
    lds_, scol0, ldg, gcol0, ldd, dcol0 = 96, 24, 64, 8, 80, 16
    src = bf(gen, rows, lds_, scale=4.0)
    src[0, scol0:scol0 + 8] = torch.tensor([30.0, -30.0, 20.0, -20.0, 0.0, -0.0, -1.28125, 9.0]).to(torch.bfloat16)
    g = bf(gen, rows, ldg)
    sd, gd = src.cuda(), g.cuda()
    dst = nan_buf(rows, ldd, dtype=torch.bfloat16)
    got, = run(capi, lambda: capi.lib.dfot_op_silu_cols(P(sd), lds_, scol0, P(gd) if grad else None, ldg, gcol0, P(dst), ldd, dcol0, rows, ncols,
                                                        S()), [dst])
    x = src[:, scol0:scol0 + ncols].double()
    s = torch.sigmoid(x)
    if grad:
        gg = g[:, gcol0:gcol0 + ncols].double()
        ref = gg * s * (1 + x * (1 - s))
        mag = gg.abs() * s * (1 + x.abs() * (1 - s))
    else:
        ref = x * s
        mag = ref.abs()
    exp, bar = torch.full((rows, ldd), NAN, dtype=torch.float64), torch.zeros(rows, ldd, dtype=torch.float64)
    exp[:, dcol0:dcol0 + ncols], bar[:, dcol0:dcol0 + ncols] = ref, 64 * U * mag
    check("silu_cols", f"silu_cols grad={grad}", got, exp, bar, nulp=2)


# ------------------------------------------------------------------------------------------------------- GEMM / conv wrappers

def test_gemm_bf16_wrapper(capi):
    """dfot_op_gemm_bf16's argument mapping: lda > K, ldo > N (padding untouched)"""
    gen = torch.Generator().manual_seed(18)
    m, n, k, lda, ldo = 256, 136, 128, 160, 152
    abuf, w, bias = bf(gen, m, lda), bf(gen, n, k, scale=1 / math.sqrt(k)), torch.randn(n, generator=gen)
    ad, wd, bd = abuf.cuda(), w.cuda(), bias.cuda()
    out = nan_buf(m, ldo, dtype=torch.bfloat16)
    got, = run(capi, lambda: capi.lib.dfot_op_gemm_bf16(P(ad), lda, P(wd), P(bd), P(out), ldo, m, n, k, S()), [out])
    a = abuf[:, :k].double()
    ref = a @ w.double().t() + bias.double()
    mag = a.abs() @ w.double().abs().t() + bias.double().abs()
    exp, bar = torch.full((m, ldo), NAN, dtype=torch.float64), torch.zeros(m, ldo, dtype=torch.float64)
    exp[:, :n], bar[:, :n] = ref, 1e-6 * mag + 1e-6 * ref.abs()
    check("gemm_bf16", "gemm_bf16 lda>K ldo>N", got, exp, bar, nulp=1)


def test_gemm_f32_wrapper_in_place_residual(capi):
    """dfot_op_gemm_f32 with bias = NULL and resid == out (in place), lda > K, ldo > N"""
    gen = torch.Generator().manual_seed(19)
    m, n, k, lda, ldo = 256, 200, 192, 224, 208
    abuf, w = bf(gen, m, lda), bf(gen, n, k, scale=1 / math.sqrt(k))
    resid = torch.randn(m, n, generator=gen)
    ad, wd = abuf.cuda(), w.cuda()
    out = torch.full((m, ldo), NAN)
    out[:, :n] = resid
    out = out.cuda()
    got, = run(capi, lambda: capi.lib.dfot_op_gemm_f32(P(ad), lda, P(wd), None, P(out), P(out), ldo, m, n, k, S()), [out])
    a = abuf[:, :k].double()
    ref = a @ w.double().t() + resid.double()
    mag = a.abs() @ w.double().abs().t() + resid.double().abs()
    exp, bar = torch.full((m, ldo), NAN, dtype=torch.float64), torch.zeros(m, ldo, dtype=torch.float64)
    exp[:, :n], bar[:, :n] = ref, 1e-6 * mag + 1e-6 * ref.abs()
    check("gemm_f32", "gemm_f32 resid==out bias=NULL", got, exp, bar)


def test_conv3x3_f32_wrapper(capi):
    """dfot_op_conv3x3_f32: NHWC bf16 input, weights packed by dfot_op_pack_conv3, bias and an out-of-place residual, vs F.conv2d in fp64"""
    gen = torch.Generator().manual_seed(20)
    bt, h, w_, cin, cout = 2, 8, 16, 64, 128
    a = bf(gen, bt, h, w_, cin)
    wt = torch.randn(cout, cin, 3, 3, generator=gen) / math.sqrt(9 * cin)
    bias, resid = torch.randn(cout, generator=gen), torch.randn(bt, h, w_, cout, generator=gen)
    ad, wtd, bd, rd = a.cuda(), wt.cuda(), bias.cuda(), resid.cuda()
    packed = torch.empty(cout * 9 * cin, dtype=torch.bfloat16, device="cuda")
    capi.check(capi.lib.dfot_op_pack_conv3(P(wtd), P(packed), cout, cin, 0, S()))
    y = nan_buf(bt * h * w_ * cout + 64)
    got, = run(capi, lambda: capi.lib.dfot_op_conv3x3_f32(P(ad), P(packed), P(bd), P(rd), P(y), bt, h, w_, cin, cout, S()), [y])
    xw = a.double().permute(0, 3, 1, 2)
    wb = wt.to(torch.bfloat16).double()
    ref = F.conv2d(xw, wb, padding=1).permute(0, 2, 3, 1) + bias.double() + resid.double()
    mag = F.conv2d(xw.abs(), wb.abs(), padding=1).permute(0, 2, 3, 1) + bias.double().abs() + resid.double().abs()
    check("conv3x3_f32", "conv3x3_f32 bias+resid", got, tail(ref, 64), tail(1e-6 * mag + 1e-6 * ref.abs(), 64))


# --------------------------------------------------------------------------------------------------------------------- refusals

def refusal_cases(capi):
    """name -> (expected status, call(buffers)).  Every call passes generously sized buffers (a check that is missing must not turn the
    call into an out-of-bounds launch): `f` / `f2` fp32, `h` / `h2` / `h3` bf16, each NaN-filled and 2^20 elements long"""
    L, A, SH = capi.lib, capi.ERR_ARG, capi.ERR_SHAPE
    N = None
    return {
        "pool2_bf16 c % 4": (SH, lambda b: L.dfot_op_pool2_bf16(P(b["f"]), P(b["h"]), 1, 8, 8, 6, S())),
        "pool2_bf16 odd h": (SH, lambda b: L.dfot_op_pool2_bf16(P(b["f"]), P(b["h"]), 1, 7, 8, 4, S())),
        "pool2_bf16 null": (A, lambda b: L.dfot_op_pool2_bf16(N, P(b["h"]), 1, 8, 8, 4, S())),
        "pool2_bwd c % 4": (SH, lambda b: L.dfot_op_pool2_bwd(P(b["f"]), P(b["f2"]), 1, 8, 8, 6, S())),
        "pool2_bwd odd h": (SH, lambda b: L.dfot_op_pool2_bwd(P(b["f"]), P(b["f2"]), 1, 9, 8, 4, S())),
        "pool2_bwd odd w": (SH, lambda b: L.dfot_op_pool2_bwd(P(b["f"]), P(b["f2"]), 1, 8, 5, 4, S())),
        "pool2_bwd null": (A, lambda b: L.dfot_op_pool2_bwd(P(b["f"]), N, 1, 8, 8, 4, S())),
        "upsample_add c % 4": (SH, lambda b: L.dfot_op_upsample_add(P(b["f"]), P(b["f"]), P(b["f2"]), 1, 4, 4, 6, S())),
        "upsample_add null": (A, lambda b: L.dfot_op_upsample_add(P(b["f"]), N, P(b["f2"]), 1, 4, 4, 4, S())),
        "upsample_bwd c % 4": (SH, lambda b: L.dfot_op_upsample_bwd(P(b["f"]), P(b["f2"]), 1, 8, 8, 6, S())),
        "upsample_bwd odd w": (SH, lambda b: L.dfot_op_upsample_bwd(P(b["f"]), P(b["f2"]), 1, 8, 7, 4, S())),
        "upsample_bwd null": (A, lambda b: L.dfot_op_upsample_bwd(N, P(b["f2"]), 1, 8, 8, 4, S())),
        "sub_bf16 n % 4": (SH, lambda b: L.dfot_op_sub_bf16(P(b["f"]), P(b["f"]), P(b["h"]), 6, S())),
        "sub_bf16 null": (A, lambda b: L.dfot_op_sub_bf16(P(b["f"]), N, P(b["h"]), 8, S())),
        "cond_repack kpad < 4 cdim": (SH, lambda b: L.dfot_op_cond_repack(P(b["f"]), P(b["h"]), 1, 8, 40, 156, S())),
        "cond_repack cdim % 20": (SH, lambda b: L.dfot_op_cond_repack(P(b["f"]), P(b["h"]), 1, 8, 30, 128, S())),
        "cond_repack null": (A, lambda b: L.dfot_op_cond_repack(N, P(b["h"]), 1, 8, 40, 160, S())),
        "split_bf16 misaligned": (A, lambda b: L.dfot_op_split_bf16(P(b["f"]), P(b["h"][1:]), P(b["h2"]), 64, S())),
        "split_bf16 n % 8": (A, lambda b: L.dfot_op_split_bf16(P(b["f"]), P(b["h"]), P(b["h2"]), 12, S())),
        "axpy null": (A, lambda b: L.dfot_op_axpy(P(b["f2"]), N, 1.0, 64, S())),
        "embed_input_wgrad res % ps": (SH, lambda b: L.dfot_op_embed_input_wgrad(P(b["f"]), P(b["f"]), P(b["f2"]), P(b["f3"]), 1, 10, 3, 64, 4, S())),
        "embed_input_wgrad null": (A, lambda b: L.dfot_op_embed_input_wgrad(P(b["f"]), N, P(b["f2"]), P(b["f3"]), 1, 8, 3, 64, 2, S())),
        "embed_input c0 % 4": (SH, lambda b: L.dfot_op_embed_input(P(b["f"]), P(b["f"]), P(b["f"]), P(b["f2"]), 1, 8, 3, 6, S())),
        "embed_input null": (A, lambda b: L.dfot_op_embed_input(P(b["f"]), N, P(b["f"]), P(b["f2"]), 1, 8, 3, 64, S())),
        "project_output cout > 3": (SH, lambda b: L.dfot_op_project_output(P(b["f"]), P(b["f"]), P(b["f"]), P(b["f2"]), 1, 8, 64, 4, S())),
        "project_output null": (A, lambda b: L.dfot_op_project_output(P(b["f"]), P(b["f"]), N, P(b["f2"]), 1, 8, 64, 3, S())),
        "outgrad_gather > 64 columns": (SH, lambda b: L.dfot_op_outgrad_gather(P(b["f"]), P(b["h"]), 1, 16, 5, 4, S())),
        "outgrad_gather res % ps": (SH, lambda b: L.dfot_op_outgrad_gather(P(b["f"]), P(b["h"]), 1, 10, 3, 4, S())),
        "outgrad_gather null": (A, lambda b: L.dfot_op_outgrad_gather(P(b["f"]), N, 1, 8, 3, 2, S())),
        "emb_pyramid r0 % 8": (SH, lambda b: L.dfot_op_emb_pyramid(P(b["h"]), P(b["h2"]), P(b["h2"]), P(b["h2"]), 1, 12, 8, S())),
        "emb_pyramid null": (A, lambda b: L.dfot_op_emb_pyramid(P(b["h"]), N, P(b["h2"]), P(b["h2"]), 1, 8, 8, S())),
        "transpose rows % 64": (SH, lambda b: L.dfot_op_transpose_bf16(P(b["h"]), P(b["h2"]), 100, 64, S())),
        "transpose cols % 64": (SH, lambda b: L.dfot_op_transpose_bf16(P(b["h"]), P(b["h2"]), 64, 96, S())),
        "transpose null": (A, lambda b: L.dfot_op_transpose_bf16(N, P(b["h2"]), 64, 64, S())),
        "silu_cols ncols % 8": (A, lambda b: L.dfot_op_silu_cols(P(b["h"]), 64, 0, N, 0, 0, P(b["h2"]), 64, 0, 4, 12, S())),
        "silu_cols scol0 % 8": (A, lambda b: L.dfot_op_silu_cols(P(b["h"]), 64, 4, N, 0, 0, P(b["h2"]), 64, 0, 4, 16, S())),
        "silu_cols dcol0 % 8": (A, lambda b: L.dfot_op_silu_cols(P(b["h"]), 64, 0, N, 0, 0, P(b["h2"]), 64, 4, 4, 16, S())),
        "silu_cols gcol0 % 8": (A, lambda b: L.dfot_op_silu_cols(P(b["h"]), 64, 0, P(b["h3"]), 64, 2, P(b["h2"]), 64, 0, 4, 16, S())),
        "silu_cols lds % 8": (SH, lambda b: L.dfot_op_silu_cols(P(b["h"]), 100, 0, N, 0, 0, P(b["h2"]), 64, 0, 4, 16, S())),
        "silu_cols ldg % 8": (SH, lambda b: L.dfot_op_silu_cols(P(b["h"]), 64, 0, P(b["h3"]), 60, 0, P(b["h2"]), 64, 0, 4, 16, S())),
        "silu_cols null": (A, lambda b: L.dfot_op_silu_cols(N, 64, 0, N, 0, 0, P(b["h2"]), 64, 0, 4, 16, S())),
        "mul_cols dcol0 % 8": (A, lambda b: L.dfot_op_mul_cols(P(b["h2"]), 64, 4, P(b["h"]), 4, 16, S())),
        "mul_cols ldd % 8": (SH, lambda b: L.dfot_op_mul_cols(P(b["h2"]), 100, 0, P(b["h"]), 4, 16, S())),
        "mul_cols null": (A, lambda b: L.dfot_op_mul_cols(P(b["h2"]), 64, 0, N, 4, 16, S())),
        "colsum ld < n": (SH, lambda b: L.dfot_op_colsum_bf16(P(b["h"]), 32, P(b["f2"]), 8, 64, S())),
        "colsum null": (A, lambda b: L.dfot_op_colsum_bf16(N, 64, P(b["f2"]), 8, 64, S())),
        "frame_sums n % 8": (SH, lambda b: L.dfot_op_frame_sums_bf16(P(b["h"]), 16, P(b["f2"]), 2, 16, 12, S())),
        "frame_sums ld < n": (SH, lambda b: L.dfot_op_frame_sums_bf16(P(b["h"]), 8, P(b["f2"]), 2, 16, 16, S())),
        "sgemm ldc < n": (A, lambda b: L.dfot_op_sgemm(P(b["f"]), 8, 1, P(b["f"]), 8, 1, P(b["f2"]), 4, 8, 8, 8, 0, S())),
        "sgemm k = 0": (A, lambda b: L.dfot_op_sgemm(P(b["f"]), 8, 1, P(b["f"]), 8, 1, P(b["f2"]), 8, 8, 8, 0, 0, S())),
        "rms_film_fwd channels": (SH, lambda b: L.dfot_op_rms_film_fwd(P(b["f"]), P(b["f"]), P(b["h"]), 1e-6, P(b["h2"]), 4, 100, S())),
        "rms_film_fwd null": (A, lambda b: L.dfot_op_rms_film_fwd(P(b["f"]), N, P(b["h"]), 1e-6, P(b["h2"]), 4, 128, S())),
        "rms_film_bwd channels": (SH, lambda b: L.dfot_op_rms_film_bwd(P(b["f"]), P(b["f"]), P(b["f"]), P(b["h"]), 1e-6, P(b["f2"]), P(b["h2"]),
                                                                       P(b["f3"]), 4, 100, 0, S())),
        "rms_film_bwd_res aliased": (A, lambda b: L.dfot_op_rms_film_bwd_res(P(b["f"]), P(b["f"]), P(b["f"]), P(b["h"]), 1e-6, P(b["f2"]), P(b["f2"]),
                                                                             N, P(b["h2"]), P(b["f3"]), 4, 128, S())),
        "qknorm_rope_fwd d": (A, lambda b: L.dfot_op_qknorm_rope_fwd(P(b["h"]), 576, P(b["f"]), P(b["f"]), P(b["f"]), 1e-6, 1.0, P(b["h2"]),
                                                                     P(b["h2"]), P(b["h2"]), 4, 4, 2, 96, S())),
        "fused_proj_train rows % 128": (A, lambda b: L.dfot_op_fused_proj_train(P(b["h"]), 128, P(b["h"]), P(b["f"]), P(b["f"]), P(b["f"]), P(b["f"]),
                                                                                1e-6, 1.0, P(b["h2"]), P(b["h2"]), P(b["h2"]), P(b["h2"]), P(b["h3"]),
                                                                                640, 128, 100, 100, 2, 64, S())),
        "fused_proj_train ccol0 % 8": (A, lambda b: L.dfot_op_fused_proj_train(P(b["h"]), 128, P(b["h"]), P(b["f"]), P(b["f"]), P(b["f"]), P(b["f"]),
                                                                               1e-6, 1.0, P(b["h2"]), P(b["h2"]), P(b["h2"]), P(b["h2"]), P(b["h3"]),
                                                                               640, 4, 128, 128, 2, 64, S())),
        "f32_to_bf16 null": (A, lambda b: L.dfot_op_f32_to_bf16(N, P(b["h"]), 64, S())),
        "bf16_to_f32 null": (A, lambda b: L.dfot_op_bf16_to_f32(P(b["h"]), N, 64, S())),
        "pack_conv3 null": (A, lambda b: L.dfot_op_pack_conv3(P(b["f"]), N, 8, 8, 1, S())),
        "gemm_bf16 null": (A, lambda b: L.dfot_op_gemm_bf16(N, 64, P(b["h"]), N, P(b["h2"]), 64, 64, 64, 64, S())),
        "gemm_f32 null": (A, lambda b: L.dfot_op_gemm_f32(P(b["h"]), 64, N, N, N, P(b["f2"]), 64, 64, 64, 64, S())),
        "conv3x3_f32 null": (A, lambda b: L.dfot_op_conv3x3_f32(P(b["h"]), N, N, N, P(b["f2"]), 1, 8, 8, 64, 64, S())),
    }


REFUSALS = ["pool2_bf16 c % 4", "pool2_bf16 odd h", "pool2_bf16 null", "pool2_bwd c % 4", "pool2_bwd odd h", "pool2_bwd odd w", "pool2_bwd null",
            "upsample_add c % 4", "upsample_add null", "upsample_bwd c % 4", "upsample_bwd odd w", "upsample_bwd null", "sub_bf16 n % 4",
            "sub_bf16 null", "cond_repack kpad < 4 cdim", "cond_repack cdim % 20", "cond_repack null", "split_bf16 misaligned", "split_bf16 n % 8",
            "axpy null", "embed_input_wgrad res % ps", "embed_input_wgrad null", "embed_input c0 % 4", "embed_input null",
            "project_output cout > 3", "project_output null", "outgrad_gather > 64 columns", "outgrad_gather res % ps", "outgrad_gather null",
            "emb_pyramid r0 % 8", "emb_pyramid null", "transpose rows % 64", "transpose cols % 64", "transpose null", "silu_cols ncols % 8",
            "silu_cols scol0 % 8", "silu_cols dcol0 % 8", "silu_cols gcol0 % 8", "silu_cols lds % 8", "silu_cols ldg % 8", "silu_cols null",
            "mul_cols dcol0 % 8", "mul_cols ldd % 8", "mul_cols null", "colsum ld < n", "colsum null", "frame_sums n % 8", "frame_sums ld < n",
            "sgemm ldc < n", "sgemm k = 0", "rms_film_fwd channels", "rms_film_fwd null", "rms_film_bwd channels", "rms_film_bwd_res aliased",
            "qknorm_rope_fwd d", "fused_proj_train rows % 128", "fused_proj_train ccol0 % 8", "f32_to_bf16 null", "bf16_to_f32 null",
            "pack_conv3 null", "gemm_bf16 null", "gemm_f32 null", "conv3x3_f32 null"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusal(capi, case):
    """the entry point returns the documented status and writes nothing (every buffer keeps its NaN fill)"""
    cases = refusal_cases(capi)
    assert set(cases) == set(REFUSALS)
    code, call = cases[case]
    bufs = {k: nan_buf(1 << 20) for k in ("f", "f2", "f3")}
    bufs.update({k: nan_buf(1 << 20, dtype=torch.bfloat16) for k in ("h", "h2", "h3")})
    got = call(bufs)
    torch.cuda.synchronize()
    assert got == code, f"{case}: status {got}, expected {code} ({capi.lib.dfot_last_error().decode()})"
    for k, t in bufs.items():
        assert torch.isnan(t.float()).all(), f"{case}: buffer {k} was written"
