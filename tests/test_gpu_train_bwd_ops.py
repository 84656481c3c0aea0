"""Op-level tests of the backward kernels of the pose U-ViT trainer (uvit_train.py: csrc/uvit_train.inl, wgrad.hip, attention_bwd.hip) against
float64 references of the same rounded operands, in the method of test_gpu_train_ops.py (helpers: train_ops_common.py): operands are
seeded on the CPU and rounded to the type the kernel reads, every output starts as NaN with a sentinel tail (columns and rows an op must
not write keep the fill), every call runs twice from the same initial buffers and must agree bit for bit, and the comparison is
element-wise against a bar with no element left out.  The worst error / bar ratio of each family is printed at the end (-s).

Bars (u = 2^-24):
  fp32 sums of n exact bf16 x bf16 products (conv dx: n = 9 Co, dW and db: n = pixels; wgrad_nt: n = rows; attention delta: n = d) and
        the fp32 patch-embedding data gradient (n = c0): |got - ref| <= n u sum|terms| + u |ref| -- the order-independent gamma_n bound,
        sum|terms| evaluated like the reference on absolute values.
  planted convolutions: one live input pixel makes every dW element one bf16 x bf16 product, exact in fp32, or an empty sum: compared as
        values with no tolerance (a zero may carry either sign); dx_bf against bf16(dx) bit for bit.
  bf16 outputs (dx_bf alone, dfilm, dfused): reference rounded to bf16, 2 ulp (every one of them follows a SiLU', an RMSNorm or a RoPE)
        + the fp32 bar of the value that is rounded; the v columns of dfused are a copy and compared bit for bit.
  GroupNorm backward (gn_bwd_reduce_kernel -> det_sum -> gn_bwd_apply_kernel), with xh = (x - mean) rstd, a = dy SiLU'(z) (1 + scale) gamma:
        dx = rstd (a - s1 - xh s2), s1 = mean_group(a), s2 = mean_group(a xh).  The bar is carried term by term on absolute values
        (gn_bars): 2 roundings on xh, 2 more on g = xh gamma + beta, 3 on z; SiLU' moves by at most 0.5 dz (|SiLU''| <= 1/2) plus its own
        evaluation error; the group sums carry their terms' errors plus a chain of L roundings on sum|a| (L = pixels per thread of the
        chunk + 2 (the four channels of a lane) + the LDS sum over the lane groups + log2(lanes per group) shuffles + det_sum's
        ceil(chunks / 16) + 4); 4 roundings on the three terms of dx, all on |a| + |s1| + |xh| |s2| so that cancellation is priced in.
        dgamma / dbeta the same with L = pixels per thread + lane groups + det_sum over bt * chunks rows.  Entries that compute their own
        statistics add the statistics' error: mean +- dm, rstd (1 +- rho), rho = 0.5 dvar / (var + eps) + 3 u with
        dvar = (c + 1) u E[x^2] + 2 |mean| dm + ... = c' u var (1 + mean^2 / var): E[x^2] - mean^2 in fp32 loses mean^2 / var.
  SiLU' evaluation: sg = 1 / (1 + __expf(-z)), SiLU' = sg (1 + z (1 - sg)).  __expf has no derivable constant and cannot be called alone
        through the op entry points, so the first test measures SiLU' as the kernels compute it (gamma = 0 and dy = 1 at one pixel make
        dbeta[c] = silu_grad(beta[c]) bit for bit; at z <= -4 its relative error is __expf's plus three roundings) against fp64 over
        |z| <= 20.  The error grows with |z| (the argument is scaled by log2 e in fp32), so the allowance is
        SG_C u (1 + |z|) sg (1 + |z| (1 - sg)).  Measured per range of z: [-20, 20] 1.174, [-4, 4] 2.156, [-1.4, -1.1] (SiLU''s zero
        crossing) 0.332, [-20, -4] (where __expf dominates) 0.884; SG_C = 4.4 is the worst, 2.156, with a 2x margin.
  qknorm_rope_bwd (qknorm_ref), per head with D = d, x the head's q or k, g the upstream gradient, w the norm weight:
        G = |g0 c| + |g1 s| bounds the rotated gradient (3 roundings), GW = G |w| the product gw = g w (1 more: 4 u GW);
        r = rsqrt(sum x^2 / D + eps): the D-term sum, the division, the addition and rsqrt give (D + 8) u on the argument, so
        rho_r = (D / 2 + 4) u on r; gx = sum gw x: (D + 4) u sum GW |x| for the sum plus its terms' 4 u; m = gx / D r r: 3 more and
        2 rho_r, in all (2 D + 19) u on mabs = sum GW |x| / D r^2; the output (gw - x m) r adds 2 roundings and rho_r + u for r:
          dfused: u r [(D / 2 + 11) GW + (2.5 D + 26) |x| mabs]        (D / 2 + 11 = 4 + 2 + D / 2 + 5;  2.5 D + 26 = 2 D + 19 + 3 + D / 2 + 4)
        then 2 bf16 ulp.  dqw[e] = sum over (row, head) of g x r: each term 3 u (rotation) + 2 u (two products) + rho_r + u =
        (D / 2 + 10) u G |x| r, and the sum a chain of lseq roundings on sum G |x| r, lseq = the items a lane adds in sequence
        (ceil(items / (waves * items per wave))) + 3 shuffle levels over the item groups of the 16-byte kernel + 2 for the four waves
        + det_sum's ceil(workgroups / 16) + 4:
          dqw, dkw: u (D / 2 + 10 + lseq) sum G |x| r + u |ref|
  attention o / lse / dq / dk / dv: P and dS are rounded to bf16 inside the kernels, so the project's bars of
        test_gpu_attention_frame_causal_bwd_ops.py hold: rel-L2 1.5e-2 (o), max abs 2e-2 (lse, log2 domain), rel-L2 2.5e-2 per gradient.

qknorm_rope_bwd has a 16-byte kernel (d = 64, row pitches multiples of 8) and a wave-per-item kernel; on one shape both run and must
agree within the sum of their bars.  Bitwise equality between the two is NOT promised: they add the head's squares in different orders.

A table-driven test checks every refusal: the status, and that every output keeps its NaN (the inputs of those calls are finite, so a
kernel that ran would show).  The entries that launch something before their main kernel check the whole call first:
dfot_op_attention_bwd_lse before the delta kernel, dfot_op_attention_bwd before the forward, dfot_op_conv3x3_bwd2 / dfot_op_gn_silu_bwd
before their memsets.

dfot_op_gn_silu_fwd2 refuses C = 384 (the statistics kernels take 128, 256, 512, 1024 only), as the backward does: that pair is in the
refusal table, not in the fp64 cases.

Worst error / bar per family, measured on an MI355X (the attention rows: rel-L2 or lse error over the project's bar; 0.500 on a bf16
output is one ulp of the two allowed):
  attention          0.155  (attention bounded bound 13 caller scratch o)
  attention_delta    0.026  (attention batch=1 heads=120 n=128 d=72 bwd_lse delta)
  conv3x3_bwd        0.015  (conv3x3_bwd 1x8x16 320->128 dW)
  conv3x3_dx_bf      0.000  (conv3x3_bwd 1x8x16 64->64 dx_bf)
  conv3x3_planted    0.000  (conv3x3_bwd live pixel (0, 0) of image 1 dW)
  embed_input_dgrad  0.438  (embed_input_dgrad bt=1 res=16 cin=4 c0=4)
  gn_silu_bwd        0.500  (gn_silu_bwd5 1x4160x128 film=2C dfilm_ld=2C dx_bf dfilm; fp32 outputs: dx 0.143, dgamma 0.041, dbeta 0.040)
  gn_silu_bwd_own    0.500  (gn_silu_bwd own stats film=2C offset=0.3 dfilm; fp32 outputs: dx 0.069, and 0.053 at offset 8)
  gn_silu_dx_bf      0.000  (gn_silu_bwd6 3x72x128 film=6C dfilm_ld=6C both dx_bf)
  gn_silu_fwd        0.500  (gn_silu_fwd 2x200x256 film=2C out)
  gn_stats           0.054  (gn_silu_fwd 3x72x128 film=none rstd)
  qknorm_rope_bwd    0.500  (qknorm_rope_bwd d=64 heads=9 batch=1 ntok=8200 ld=3C+0 ldo=3C+0 (vec) dfused; dqw / dkw 0.021)
  qknorm_vec_vs_one  0.004  (d=64 heads=3 batch=2 ntok=37)
  silu_grad          0.490  (measured SG_C / allowance)
  wgrad_nt           0.008  (wgrad_nt 8x8 rows=64 slices=1)
gn_stats_kernel's E[x^2] - mean^2 stays inside its derived bar at mean^2 / var = 64 (rho about 1e-4 there), so it keeps its one pass.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from train_ops_common import (NAN, P, S, U, bf, bits, capi, check, exact, nan_buf, record, run, seq_bar, tail, ulp_bf16,  # noqa: F401
                              worst_ratio_table)

pytestmark = pytest.mark.gpu

BAR_O, BAR_LSE, BAR_GRAD = 1.5e-2, 2e-2, 2.5e-2  # tests/test_gpu_attention_frame_causal_bwd_ops.py
EPS = 1e-6
# 2 x the measured worst, 2.156.  test_silu_grad_allowance printed, per range of z (MI355X, hipcc -O3):
#   [-20, 20] 1.174   [-4, 4] 2.156   [-1.4, -1.1] 0.332   [-20, -4] 0.884
SG_C = 4.4
BF, F32 = torch.bfloat16, torch.float32


def same_values(fam, name, got, exp):
    """equality as values, element for element and without tolerance (an empty sum is +0, 0 * -x is -0: a zero may carry either sign);
    exp carries the NaN sentinel where nothing may be written"""
    assert got.dtype == exp.dtype and got.shape == exp.shape
    n = torch.isnan(exp)
    assert torch.equal(torch.isnan(got), n), f"{name}: stores outside the output, or outputs missing"
    bad = (got != exp) & ~n
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        pytest.fail(f"{name}: {int(bad.sum())} elements differ, first at flat index {i}: got {got.flatten()[i].item()!r}, want {exp.flatten()[i].item()!r}")
    print(f"{name}: exact")
    record(fam, name, 0.0)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------- SiLU' allowance

def silu_parts(z):
    """sigmoid, SiLU' and the magnitude of SiLU''s terms, fp64"""
    sg = torch.sigmoid(z)
    return sg, sg * (1 + z * (1 - sg)), sg * (1 + z.abs() * (1 - sg))


def test_silu_grad_allowance(capi):
    """measures SG_C: bt = 1, gamma = 0, so z = beta exactly; dy = 1 at pixel 0 and 0 elsewhere, so dbeta[c] = silu_grad(beta[c]) with
    nothing added but zeros.  1024 values of z per call, uniform in +-20, +-4 and around SiLU''s zero crossing"""
    gen = torch.Generator().manual_seed(100)
    pix, c = 64, 1024
    x = torch.randn(1, pix, c, generator=gen)
    dy = torch.zeros(pix, c, dtype=BF)
    dy[0] = 1.0
    stats = torch.stack([torch.zeros(32), torch.ones(32)], -1).view(1, 32, 2).contiguous()
    gamma = torch.zeros(c)
    xd, dyd, sd, gd = x.cuda(), dy.cuda(), stats.cuda(), gamma.cuda()
    worst = 0.0
    for lo, hi in ((-20.0, 20.0), (-4.0, 4.0), (-1.4, -1.1), (-20.0, -4.0)):
        beta = lo + (hi - lo) * torch.rand(c, generator=gen)
        bd = beta.cuda()
        dx, dga, dbe = nan_buf(pix * c + 16), nan_buf(c + 16), nan_buf(c + 16)
        _, gga, gbe = run(capi, lambda: capi.lib.dfot_op_gn_silu_bwd5(P(xd), P(dyd), P(sd), P(gd), P(bd), None, None, P(dx), None, None, 0, P(dga),
                                                                      P(dbe), 1, pix, c, S()), [dx, dga, dbe])
        z = beta.double()
        _, sp, spm = silu_parts(z)
        assert torch.isnan(gbe[c:]).all() and torch.isfinite(gbe[:c]).all()
        r = ((gbe[:c].double() - sp).abs() / (U * (1 + z.abs()) * spm)).max().item()
        print(f"silu_grad on z in [{lo}, {hi}]: worst error = {r:.3f} u (1 + |z|) |terms|")
        worst = max(worst, r)
    print(f"measured SG_C = {worst:.3f} (allowance {SG_C})")
    record("silu_grad", "measured SG_C / allowance", worst / SG_C)
    assert worst <= SG_C


# ---------------------------------------------------------------------------------------------------------- 1. conv3x3 backward

def conv_call(capi, x, dy, wt, want_bf=False, entry2=True):
    """dx (fp32, or bf16 through dx_bf), dw, db of one call, each followed by a 16-element sentinel"""
    bt, h, w, ci = x.shape
    co = dy.shape[-1]
    xd, dyd, wd = x.cuda(), dy.cuda(), wt.cuda()
    dx = nan_buf(bt * h * w * ci + 16, dtype=BF if want_bf else F32)
    dw, db = nan_buf(co * ci * 9 + 16), nan_buf(co + 16)
    L = capi.lib
    if want_bf:
        fn = lambda: L.dfot_op_conv3x3_bwd2(P(xd), P(dyd), P(wd), None, P(dx), P(dw), P(db), bt, h, w, ci, co, S())
    elif entry2:
        fn = lambda: L.dfot_op_conv3x3_bwd2(P(xd), P(dyd), P(wd), P(dx), None, P(dw), P(db), bt, h, w, ci, co, S())
    else:
        fn = lambda: L.dfot_op_conv3x3_bwd(P(xd), P(dyd), P(wd), P(dx), P(dw), P(db), bt, h, w, ci, co, S())
    return run(capi, fn, [dx, dw, db])


def conv_ref(x, dy, wt):
    """fp64 autograd of conv2d(padding 1) on the bf16 operands (the data gradient uses bf16 weights), and sum|terms| of each gradient"""
    xd, gd = x.double().permute(0, 3, 1, 2), dy.double().permute(0, 3, 1, 2)
    wb = wt.to(BF).double()
    xr, wr, br = xd.clone().requires_grad_(), wb.clone().requires_grad_(), torch.zeros(wt.shape[0], dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, wr, br, padding=1).backward(gd)
    mdx = F.conv_transpose2d(gd.abs(), wb.abs(), padding=1).permute(0, 2, 3, 1)
    mdw = torch.nn.grad.conv2d_weight(xd.abs(), wt.shape, gd.abs(), padding=1)
    return (xr.grad.permute(0, 2, 3, 1), mdx), (wr.grad, mdw), (br.grad, gd.abs().sum((0, 2, 3)))


def conv_check(tag, got, x, dy, wt):
    bt, h, w, ci = x.shape
    co, pix = dy.shape[-1], bt * h * w
    (rdx, mdx), (rdw, mdw), (rdb, mdb) = conv_ref(x, dy, wt)
    check("conv3x3_bwd", tag + " dx", got[0], tail(rdx, 16), tail(seq_bar(9 * co, mdx, rdx), 16))
    check("conv3x3_bwd", tag + " dW", got[1], tail(rdw, 16), tail(seq_bar(pix, mdw, rdw), 16))
    check("conv3x3_bwd", tag + " db", got[2], tail(rdb, 16), tail(seq_bar(pix, mdb, rdb), 16))


# one image, guarded 64-wide tiles of the 128 x 128 tap form, split == 1 | H != W, odd bt, the 256 form with guarded edges | split > 1 and
# slices_sum_kernel | wide ci with a small image.  The data-gradient GEMM takes whole 128-row tiles, so the smallest image is 8 x 16: an
# 8 x 8 one (64 pixels) is refused (refusal table)
CONV = [(1, 8, 16, 64, 64), (3, 8, 16, 64, 192), (2, 16, 16, 128, 128), (1, 8, 16, 320, 128)]


@pytest.mark.parametrize("bt,h,w,ci,co", CONV)
def test_conv3x3_bwd(capi, bt, h, w, ci, co):
    """dx, dW, db each against fp64 (dfot_op_conv3x3_bwd), then dfot_op_conv3x3_bwd2 with dx_bf: bf16(dx) bit for bit, dW and db the same bits"""
    gen = torch.Generator().manual_seed(bt + h + w + ci + co)
    x, dy = bf(gen, bt, h, w, ci), bf(gen, bt, h, w, co)
    wt = torch.randn(co, ci, 3, 3, generator=gen) / math.sqrt(9 * ci)
    tag = f"conv3x3_bwd {bt}x{h}x{w} {ci}->{co}"
    got = conv_call(capi, x, dy, wt, entry2=False)
    conv_check(tag, got, x, dy, wt)
    got_bf = conv_call(capi, x, dy, wt, want_bf=True)
    n = bt * h * w * ci
    exact("conv3x3_dx_bf", tag + " dx_bf", got_bf[0], tail(got[0][:n].to(BF), 16))
    exact("conv3x3_dx_bf", tag + " dW (dx_bf call)", got_bf[1], got[1])
    exact("conv3x3_dx_bf", tag + " db (dx_bf call)", got_bf[2], got[2])


@pytest.mark.parametrize("img,py,px", [(1, 0, 0), (1, 0, 15), (0, 3, 0), (0, 3, 15), (1, 0, 8)])
def test_conv3x3_bwd_one_live_pixel_makes_the_weight_gradient_exact(capi, img, py, px):
    """x is non-zero at one pixel of one of two 4 x 16 images (each corner, the middle of the top edge; always on the side where the other
    image's rows are its neighbours in memory), dy is dense: dW[co][ci][ky][kx] = dy[p - (ky - 1, kx - 1)][co] x[p][ci], one exact product --
    or exactly 0 where that pixel lies outside the image.  (Two images: 128 pixels, the least the data-gradient GEMM takes)"""
    gen = torch.Generator().manual_seed(31 * py + px)
    bt, h, w, ci, co = 2, 4, 16, 64, 64
    x = torch.zeros(bt, h, w, ci, dtype=BF)
    x[img, py, px] = bf(gen, ci) + torch.tensor(0.0078125).to(BF)
    assert (x[img, py, px] != 0).all()
    dy = bf(gen, bt, h, w, co)
    wt = torch.randn(co, ci, 3, 3, generator=gen) / math.sqrt(9 * ci)
    want = torch.zeros(co, ci, 3, 3)
    outside = 0
    for ky in range(3):
        for kx in range(3):
            qy, qx = py - (ky - 1), px - (kx - 1)
            if 0 <= qy < h and 0 <= qx < w:
                want[:, :, ky, kx] = dy[img, qy, qx].float()[:, None] * x[img, py, px].float()[None, :]
            else:
                outside += 1
    assert outside == (5 if px != 8 else 3)
    ref = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), wt.shape, dy.double().permute(0, 3, 1, 2), padding=1)
    assert torch.equal(want.double(), ref)                                       # every product is exact in fp32
    got = conv_call(capi, x, dy, wt)
    same_values("conv3x3_planted", f"conv3x3_bwd live pixel ({py}, {px}) of image {img} dW", got[1], tail(want, 16))
    conv_check(f"conv3x3_bwd live pixel ({py}, {px}) of image {img}", got, x, dy, wt)


def test_conv3x3_bwd_does_not_read_the_neighbouring_image(capi):
    """rows are the pixels of consecutive images: x lives in the last row of image 0 only, dy in the first row of image 1 only.  A tap
    guard that lets a shifted row cross the image border pairs them; with the guard all of dW and dx of image 0 are exactly 0"""
    gen = torch.Generator().manual_seed(41)
    bt, h, w, ci, co = 2, 4, 16, 64, 64
    x, dy = torch.zeros(bt, h, w, ci, dtype=BF), torch.zeros(bt, h, w, co, dtype=BF)
    x[0, h - 1] = bf(gen, w, ci)
    dy[1, 0] = bf(gen, w, co)
    wt = torch.randn(co, ci, 3, 3, generator=gen) / math.sqrt(9 * ci)
    got = conv_call(capi, x, dy, wt)
    same_values("conv3x3_planted", "conv3x3_bwd image border dW", got[1], tail(torch.zeros(co, ci, 3, 3), 16))
    n0 = h * w * ci
    same_values("conv3x3_planted", "conv3x3_bwd image border dx of image 0", got[0][:n0], torch.zeros(n0))
    assert got[0][n0:2 * n0].abs().max() > 0
    conv_check("conv3x3_bwd image border", got, x, dy, wt)


# ------------------------------------------------------------------------------------------------------- 2. GroupNorm + SiLU

def gn_true_stats(x):
    """fp64 (mean, biased variance) per (image, group) of x [bt][P][C]"""
    bt, pix, c = x.shape
    v = x.double().view(bt, pix, 32, c // 32)
    m = v.mean((1, 3))
    return m, (v - m.view(bt, 1, 32, 1)).pow(2).mean((1, 3))


def gn_terms(x, gamma, beta, film, mean, rstd, dm, rho):
    """the forward's values in fp64, shaped [bt][P][32][cpg], with the bars of xh, g and z (dm, rho: what mean and rstd may be off by)"""
    bt, pix, c = x.shape
    cpg = c // 32
    X = x.double().view(bt, pix, 32, cpg)
    ga, be = gamma.double().view(32, cpg), beta.double().view(32, cpg)
    m, r = mean.double().view(bt, 1, 32, 1), rstd.double().view(bt, 1, 32, 1)
    dm, rho = torch.as_tensor(dm, dtype=torch.float64), torch.as_tensor(rho, dtype=torch.float64)
    if dm.ndim:
        dm, rho = dm.view(bt, 1, 32, 1), rho.view(bt, 1, 32, 1)
    xh = (X - m) * r
    e_xh = 2 * U * xh.abs() + r * dm + xh.abs() * rho
    g = xh * ga + be
    G = (xh * ga).abs() + be.abs()
    e_g = ga.abs() * e_xh + 2 * U * G
    if film is not None:
        sc, sh = (film[:, i * c:(i + 1) * c].double().view(bt, pix, 32, cpg) for i in (0, 1))
        mul = 1 + sc
        z = g * mul + sh
        e_z = mul.abs() * e_g + 3 * U * (G * mul.abs() + sh.abs())
    else:
        mul, z, e_z = torch.ones_like(g), g, e_g
    return dict(xh=xh, e_xh=e_xh, g=g, e_g=e_g, mul=mul, z=z, e_z=e_z, r=r, ga=ga, rho=rho)


def gn_bars(x, dy, gamma, beta, film, mean, rstd, chunk_rows, dres=None, dm=0.0, rho=0.0):
    """fp64 reference and bars of the GroupNorm + [FiLM] + SiLU backward from the statistics the kernel uses (see the module docstring).
    Returns {name: (reference, bar)} for dx [bt][P][C], dgamma, dbeta [C], dfilm [bt * P][2C]"""
    bt, pix, c = x.shape
    cpg = c // 32
    t = gn_terms(x, gamma, beta, film, mean, rstd, dm, rho)
    xh, e_xh, g, e_g, mul, z, e_z, r, ga, rho = (t[k] for k in ("xh", "e_xh", "g", "e_g", "mul", "z", "e_z", "r", "ga", "rho"))
    DY = dy.double().view(bt, pix, 32, cpg)
    _, sp, spm = silu_parts(z)
    e_sp = 0.5 * e_z + SG_C * U * (1 + z.abs()) * spm
    dz = DY * sp
    e_dz = DY.abs() * e_sp + U * dz.abs()
    dg = dz * mul
    e_dg = e_dz * mul.abs() + 2 * U * dg.abs()
    a = dg * ga
    e_a = e_dg * ga.abs() + U * a.abs()
    n = pix * cpg
    # the launcher's plan
    chunk = 512 if pix >= 4096 else 64
    assert chunk == chunk_rows
    nchunks = cdiv(pix, chunk)
    lanes = min(c // 4, 256)
    groups = 256 // lanes
    lpg = cpg // 4
    L1 = cdiv(chunk, groups) + 2 + (groups - 1) + int(math.log2(lpg)) + cdiv(nchunks, 16) + 4
    Lg = cdiv(chunk, groups) + (groups - 1) + cdiv(bt * nchunks, 16) + 4
    A, AX = a.abs(), (a * xh).abs()
    gs = lambda v: v.sum((1, 3), keepdim=True)
    s1, s2 = gs(a) / n, gs(a * xh) / n
    s1a, s2a = gs(A) / n, gs(AX) / n
    d_s1 = (gs(e_a) + L1 * U * gs(A)) / n + 2 * U * s1a
    d_s2 = (gs(e_a * xh.abs() + A * e_xh + U * AX) + L1 * U * gs(AX)) / n + 2 * U * s2a
    dx = r * (a - s1 - xh * s2)
    three = A + s1a + xh.abs() * s2a
    e_dx = r * (e_a + d_s1 + xh.abs() * d_s2 + e_xh * s2a + 4 * U * three) + rho * r * three
    if dres is not None:
        dr = dres.double().view(bt, pix, 32, cpg)
        e_dx = e_dx + U * (dr.abs() + dx.abs())
        dx = dx + dr
    e_dx = e_dx + U * dx.abs()
    dgx = dg * xh
    rga, rbe = dgx.sum((0, 1)), dg.sum((0, 1))
    e_ga = (e_dg * xh.abs() + dg.abs() * e_xh + U * dgx.abs()).sum((0, 1)) + Lg * U * dgx.abs().sum((0, 1)) + U * rga.abs()
    e_be = e_dg.sum((0, 1)) + Lg * U * dg.abs().sum((0, 1)) + U * rbe.abs()
    out = {"dx": (dx.reshape(bt, pix, c), e_dx.reshape(bt, pix, c)), "dgamma": (rga.reshape(c), e_ga.reshape(c)),
           "dbeta": (rbe.reshape(c), e_be.reshape(c))}
    if film is not None:
        dsc = dz * g
        e_dsc = e_dz * g.abs() + dz.abs() * e_g + U * dsc.abs()
        out["dfilm"] = (torch.cat([dsc.reshape(bt * pix, c), dz.reshape(bt * pix, c)], 1),
                        torch.cat([e_dsc.reshape(bt * pix, c), e_dz.reshape(bt * pix, c)], 1))
    return out


def test_gn_formula_is_the_fp64_autograd_gradient():
    """the closed form gn_bars evaluates equals fp64 autograd through group_norm -> FiLM -> SiLU when it is given the true statistics"""
    gen = torch.Generator().manual_seed(50)
    bt, pix, c = 2, 24, 128
    x = torch.randn(bt, pix, c, generator=gen) * 1.5 + 0.3
    dy = bf(gen, bt, pix, c)
    gamma, beta = torch.randn(c, generator=gen) * 0.5 + 1, torch.randn(c, generator=gen) * 0.2
    film = bf(gen, bt * pix, 2 * c, scale=0.5)
    m, var = gn_true_stats(x)
    rstd = torch.rsqrt(var + EPS)
    ref = gn_bars(x, dy, gamma, beta, film, m, rstd, 64)
    xr, gr, br = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    fr = film.double().view(bt, pix, 2 * c).requires_grad_()
    hh = F.group_norm(xr.permute(0, 2, 1), 32, gr, br, EPS).permute(0, 2, 1)
    F.silu(hh * (1 + fr[..., :c]) + fr[..., c:]).backward(dy.double())
    for name, grad in (("dx", xr.grad), ("dgamma", gr.grad), ("dbeta", br.grad), ("dfilm", fr.grad.view(bt * pix, 2 * c))):
        assert torch.allclose(ref[name][0], grad, rtol=1e-11, atol=1e-12), name


def gn_inputs(gen, bt, pix, c, film_mode, offset=0.3, scale=1.5):
    x = torch.randn(bt, pix, c, generator=gen) * scale + offset
    gamma, beta = torch.randn(c, generator=gen) * 0.5 + 1, torch.randn(c, generator=gen) * 0.2
    if film_mode == "none":
        return x, gamma, beta, None, None, 0
    fld = 2 * c if film_mode == "2C" else 6 * c
    wide = bf(gen, bt * pix, fld, scale=0.5)
    return x, gamma, beta, wide, (wide if film_mode == "2C" else wide[:, 2 * c:4 * c]), fld


def film_ptr(fd, film_mode, c):
    return None if fd is None else P(fd if film_mode == "2C" else fd[:, 2 * c:])


# 3 x 72: a partial second 64-pixel chunk, odd bt | 512: the 4-lane group shuffle | 1024: groups == 1, the 8-lane shuffle, lanes == 256 |
# 4160: 512-pixel chunks with a partial last one.  film: absent | row pitch 2C | the column block at offset 2C of a 6C-wide matrix (fwd2)
GN_FWD = [(3, 72, 128, "none"), (2, 64, 512, "2C"), (1, 64, 1024, "6C"), (1, 4160, 128, "6C"), (2, 200, 256, "2C")]


@pytest.mark.parametrize("bt,pix,c,film_mode", GN_FWD)
def test_gn_silu_fwd(capi, bt, pix, c, film_mode):
    """out = SiLU(GN32(x) [* (1 + scale) + shift]) in bf16 and stats = (mean, rstd), both element-wise against fp64: mean on an absolute bar,
    rstd on a relative one (partial sums of <= 128 pixels per workgroup, a fixed-order finalize, E[x^2] - mean^2 in fp32)"""
    gen = torch.Generator().manual_seed(bt + pix + c)
    x, gamma, beta, wide, film, fld = gn_inputs(gen, bt, pix, c, film_mode)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    fd = None if wide is None else wide.cuda()
    out, stats = nan_buf(bt * pix * c + 16, dtype=BF), nan_buf(bt * 64 + 16)
    L = capi.lib
    if film_mode == "6C":
        fn = lambda: L.dfot_op_gn_silu_fwd2(P(xd), P(gd), P(bd), film_ptr(fd, film_mode, c), fld, EPS, P(out), P(stats), bt, pix, c, S())
    else:
        fn = lambda: L.dfot_op_gn_silu_fwd(P(xd), P(gd), P(bd), film_ptr(fd, film_mode, c), EPS, P(out), P(stats), bt, pix, c, S())
    gout, gstats = run(capi, fn, [out, stats])
    m, var = gn_true_stats(x)
    rstd = torch.rsqrt(var + EPS)
    cpg = c // 32
    v = x.double().view(bt, pix, 32, cpg)
    q, absmean = v.pow(2).mean((1, 3)), v.abs().mean((1, 3))
    ppass = 256 // (c // 4)
    cs = 4 * cdiv(min(pix, 128), ppass) + 8 + cdiv(cdiv(pix, 128), 32) + 5 + 2
    dm = cs * U * absmean + U * m.abs()
    dvar = (cs + 1) * U * q + 2 * m.abs() * dm + 2 * U * m * m + U * var
    rho = 0.5 * dvar / (var + EPS) + 3 * U
    tag = f"gn_silu_fwd {bt}x{pix}x{c} film={film_mode}"
    assert torch.isnan(gstats[bt * 64:]).all() and torch.isfinite(gstats[:bt * 64]).all()
    gs = gstats[:bt * 64].double().view(bt, 32, 2)
    rm = ((gs[..., 0] - m).abs() / dm).max().item()
    rr = ((gs[..., 1] / rstd - 1).abs() / rho).max().item()
    print(f"{tag}: stats worst error / bar: mean {rm:.3f}, rstd {rr:.3f}")
    record("gn_stats", tag + " mean", rm)
    record("gn_stats", tag + " rstd", rr)
    assert rm <= 1.0 and rr <= 1.0
    t = gn_terms(x, gamma, beta, film, m, rstd, dm, rho)
    z = t["z"]
    sg = torch.sigmoid(z)
    ref = z * sg
    bar = 1.1 * t["e_z"] + SG_C * U * (1 + z.abs()) * ref.abs()                  # |SiLU'| <= 1.1; SiLU = z / (1 + __expf(-z))
    check("gn_silu_fwd", tag + " out", gout, tail(ref.reshape(bt, pix, c), 16), tail(bar.reshape(bt, pix, c), 16), nulp=2)


# (bt, P, C, film, dfilm row pitch in units of C, outputs): every film / dfilm pitch / output option once at C = 512 or 1024 and once with a
# partial chunk (P = 72, 200: 64-pixel chunks; P = 4160: 512-pixel chunks)
GN_BWD = [(3, 72, 128, "none", 0, "dx"), (3, 72, 128, "6C", 6, "both"), (2, 64, 512, "2C", 2, "dx_bf"), (2, 64, 512, "none", 0, "both"),
          (1, 64, 1024, "6C", 6, "dx"), (1, 64, 1024, "none", 0, "dx_bf"), (1, 4160, 128, "2C", 2, "dx_bf"), (2, 200, 256, "2C", 6, "dx")]


@pytest.mark.parametrize("bt,pix,c,film_mode,dfl,outs", GN_BWD)
def test_gn_silu_bwd_saved_stats(capi, bt, pix, c, film_mode, dfl, outs):
    """dfot_op_gn_silu_bwd5 (film absent or at pitch 2C) / _bwd6 (film a column block of a 6C-wide matrix) from saved statistics and a bf16
    upstream gradient.  outs: dx alone | dx_bf alone | both with dres (dres comes back unchanged, dx_bf == bf16(dx) bit for bit).  dfilm
    at pitch 2C, or the block at column 2C of a 6C-wide matrix whose other columns keep their fill"""
    gen = torch.Generator().manual_seed(2 * bt + pix + c + dfl)
    x, gamma, beta, wide, film, fld = gn_inputs(gen, bt, pix, c, film_mode)
    dy = bf(gen, bt * pix, c)
    dres = torch.randn(bt, pix, c, generator=gen) if outs == "both" else None
    m, var = gn_true_stats(x)
    stats = torch.stack([m, torch.rsqrt(var + EPS)], -1).float().contiguous()   # the saved statistics are operands: rounded to fp32
    xd, gd, bd, dyd, sd = x.cuda(), gamma.cuda(), beta.cuda(), dy.cuda(), stats.cuda()
    fd = None if wide is None else wide.cuda()
    rd = None if dres is None else dres.cuda()
    n = bt * pix * c
    dx = nan_buf(n + 16) if outs != "dx_bf" else None
    dxb = nan_buf(n + 16, dtype=BF) if outs != "dx" else None
    dfilm = nan_buf(bt * pix, dfl * c, dtype=BF) if dfl else None
    dfp = None if dfilm is None else P(dfilm if dfl == 2 else dfilm[:, 2 * c:])
    dga, dbe = nan_buf(c + 16), nan_buf(c + 16)
    L = capi.lib
    if film_mode == "6C":
        fn = lambda: L.dfot_op_gn_silu_bwd6(P(xd), P(dyd), P(sd), P(gd), P(bd), film_ptr(fd, film_mode, c), fld, P(rd), P(dx), P(dxb), dfp, dfl * c,
                                            P(dga), P(dbe), bt, pix, c, S())
    else:
        fn = lambda: L.dfot_op_gn_silu_bwd5(P(xd), P(dyd), P(sd), P(gd), P(bd), film_ptr(fd, film_mode, c), P(rd), P(dx), P(dxb), dfp, dfl * c,
                                            P(dga), P(dbe), bt, pix, c, S())
    bufs = {"dgamma": dga, "dbeta": dbe}
    for k, b in (("dx", dx), ("dx_bf", dxb), ("dfilm", dfilm), ("dres", rd)):
        if b is not None:
            bufs[k] = b
    got = dict(zip(bufs, run(capi, fn, list(bufs.values()))))
    ref = gn_bars(x, dy, gamma, beta, film, stats[..., 0], stats[..., 1], 512 if pix >= 4096 else 64, dres=dres)
    tag = f"gn_silu_bwd{6 if film_mode == '6C' else 5} {bt}x{pix}x{c} film={film_mode} dfilm_ld={dfl}C {outs}"
    for k in ("dgamma", "dbeta"):
        check("gn_silu_bwd", f"{tag} {k}", got[k], tail(ref[k][0], 16), tail(ref[k][1], 16))
    if dx is not None:
        check("gn_silu_bwd", tag + " dx", got["dx"], tail(ref["dx"][0], 16), tail(ref["dx"][1], 16))
    if outs == "dx_bf":
        check("gn_silu_bwd", tag + " dx_bf", got["dx_bf"], tail(ref["dx"][0], 16), tail(ref["dx"][1], 16), nulp=2)
    if outs == "both":
        exact("gn_silu_dx_bf", tag + " dx_bf", got["dx_bf"], tail(got["dx"][:n].to(BF), 16))
        assert torch.equal(bits(got["dres"]), bits(dres)), "dres was modified"
    if dfl:
        exp, bar = torch.full((bt * pix, dfl * c), NAN, dtype=torch.float64), torch.zeros(bt * pix, dfl * c, dtype=torch.float64)
        c0 = 0 if dfl == 2 else 2 * c
        exp[:, c0:c0 + 2 * c], bar[:, c0:c0 + 2 * c] = ref["dfilm"]
        check("gn_silu_bwd", tag + " dfilm", got["dfilm"], exp, bar, nulp=2)


@pytest.mark.parametrize("film_mode,offset", [("none", 0.3), ("2C", 0.3), ("2C", 8.0)])
def test_gn_silu_bwd_own_stats(capi, film_mode, offset):
    """dfot_op_gn_silu_bwd at C = 512: gn_stats_kernel forms E[x^2] - mean^2 in fp32 (n / 256 terms per thread, a wave sum, four waves), so
    the bar carries dm on the mean and rho = c u (1 + mean^2 / var) on rstd; x = 8 + randn makes mean^2 / var about 64"""
    gen = torch.Generator().manual_seed(60 + int(offset))
    bt, pix, c = 2, 64, 512
    x, gamma, beta, wide, film, _ = gn_inputs(gen, bt, pix, c, film_mode, offset=offset, scale=1.0 if offset > 1 else 1.5)
    dy = torch.randn(bt, pix, c, generator=gen)
    xd, gd, bd, dyd = x.cuda(), gamma.cuda(), beta.cuda(), dy.cuda()
    fd = None if wide is None else wide.cuda()
    dx, dga, dbe = nan_buf(bt * pix * c + 16), nan_buf(c + 16), nan_buf(c + 16)
    dfilm = nan_buf(bt * pix * 2 * c + 16, dtype=BF) if film is not None else None
    outs = [dx, dga, dbe] + ([dfilm] if dfilm is not None else [])
    got = run(capi, lambda: capi.lib.dfot_op_gn_silu_bwd(P(xd), P(dyd), P(gd), P(bd), P(fd), EPS, P(dx), P(dfilm), P(dga), P(dbe), bt, pix, c, S()), outs)
    m, var = gn_true_stats(x)
    cpg = c // 32
    v = x.double().view(bt, pix, 32, cpg)
    q, absmean = v.pow(2).mean((1, 3)), v.abs().mean((1, 3))
    cs = cdiv(pix * cpg, 256) + 6 + 2 + 2
    dm = cs * U * absmean + U * m.abs()
    dvar = (cs + 1) * U * q + 2 * m.abs() * dm + 2 * U * m * m + U * var
    rho = 0.5 * dvar / (var + EPS) + 3 * U
    print(f"gn_silu_bwd own stats offset {offset}: mean^2 / var up to {float((m * m / var).max()):.1f}, rho up to {float(rho.max()):.2e}")
    ref = gn_bars(x, dy, gamma, beta, film, m, torch.rsqrt(var + EPS), 64, dm=dm, rho=rho)
    tag = f"gn_silu_bwd own stats film={film_mode} offset={offset}"
    check("gn_silu_bwd_own", tag + " dx", got[0], tail(ref["dx"][0], 16), tail(ref["dx"][1], 16))
    check("gn_silu_bwd_own", tag + " dgamma", got[1], tail(ref["dgamma"][0], 16), tail(ref["dgamma"][1], 16))
    check("gn_silu_bwd_own", tag + " dbeta", got[2], tail(ref["dbeta"][0], 16), tail(ref["dbeta"][1], 16))
    if film is not None:
        check("gn_silu_bwd_own", tag + " dfilm", got[3], tail(ref["dfilm"][0], 16), tail(ref["dfilm"][1], 16), nulp=2)


# ------------------------------------------------------------------------------------------------------- 3. qknorm_rope_bwd

def qknorm_ref(fused, dq, dk, dv, qw, kw, cs, batch, ntok, heads, d, lseq):
    """fp64 autograd of sum(dq . rope(rmsnorm(q; qw))) + sum(dk . rope(rmsnorm(k; kw))) + sum(dv . v) over the first 3C columns of fused
    [rows][ld] (the rotation with the device's own (cos, sin) table), in row blocks; and the bars of the module docstring.
    Returns (dfused [rows][3C], its fp32 bar), (dqw, bar), (dkw, bar).  lseq: the longest run of sequential adds on a dqw element"""
    c, rows = heads * d, batch * ntok
    tok = torch.arange(rows) % ntok
    co, si = cs[..., 0].double()[tok].unsqueeze(1), cs[..., 1].double()[tok].unsqueeze(1)      # [rows][1][d / 2]
    gr = [t.double().permute(0, 2, 1, 3).reshape(rows, heads, d) for t in (dq, dk, dv)]        # the gradients in row layout
    grad, bar = torch.empty(rows, 3 * c, dtype=torch.float64), torch.zeros(rows, 3 * c, dtype=torch.float64)
    wref = [torch.zeros(d, dtype=torch.float64) for _ in range(2)]
    wmag = [torch.zeros(d, dtype=torch.float64) for _ in range(2)]
    ws = [qw.double().requires_grad_(), kw.double().requires_grad_()]
    for r0 in range(0, rows, 1024):
        sl = slice(r0, min(rows, r0 + 1024))
        xr = fused[sl, :3 * c].double().requires_grad_()
        parts = xr.view(-1, 3, heads, d)
        loss = (parts[:, 2] * gr[2][sl]).sum()
        for i in (0, 1):
            xi = parts[:, i]
            y = xi * torch.rsqrt(xi.pow(2).mean(-1, keepdim=True) + EPS) * ws[i]
            y0, y1 = y[..., 0::2], y[..., 1::2]
            rot = torch.stack([y0 * co[sl] - y1 * si[sl], y1 * co[sl] + y0 * si[sl]], -1).flatten(-2)
            loss = loss + (rot * gr[i][sl]).sum()
        loss.backward()
        grad[sl] = xr.grad
        with torch.no_grad():
            for i in (0, 1):
                xa = parts[:, i].detach().abs()
                r = torch.rsqrt(parts[:, i].detach().pow(2).mean(-1, keepdim=True) + EPS)
                g0, g1 = gr[i][sl][..., 0::2].abs(), gr[i][sl][..., 1::2].abs()
                G = torch.stack([g0 * co[sl].abs() + g1 * si[sl].abs(), g1 * co[sl].abs() + g0 * si[sl].abs()], -1).flatten(-2)
                GW = G * ws[i].detach().abs()
                mabs = (GW * xa).sum(-1, keepdim=True) / d * r * r
                bar[sl, i * c:(i + 1) * c] = (U * r * ((d / 2 + 11) * GW + (2.5 * d + 26) * xa * mabs)).reshape(-1, c)
                wmag[i] += (G * xa * r).sum((0, 1))
    res = [(grad, bar)]
    for i in (0, 1):
        ref = ws[i].grad
        res.append((ref, U * (d / 2 + 10 + lseq) * wmag[i] + U * ref.abs()))
    return res


def qknorm_case(capi, d, heads, batch, ntok, ld_pad, ldo_pad, seed):
    gen = torch.Generator().manual_seed(seed)
    c, rows = heads * d, batch * ntok
    ld, ldo = 3 * c + ld_pad, 3 * c + ldo_pad
    fused = torch.full((rows, ld), NAN, dtype=BF)                                               # columns [3C, ld) are never read
    fused[:, :3 * c] = bf(gen, rows, 3 * c, scale=2.0)
    dq, dk, dv = (bf(gen, batch, heads, ntok, d) for _ in range(3))                            # distinct data per batch element
    qw, kw = torch.rand(d, generator=gen) + 0.5, torch.rand(d, generator=gen) + 0.5
    ang = torch.rand(ntok, d // 2, generator=gen) * 2 * math.pi
    cs = torch.stack([ang.cos(), ang.sin()], -1).contiguous()
    dev = [t.cuda() for t in (fused, dq, dk, dv, qw, kw, cs)]
    dfused, dqw, dkw = nan_buf(rows, ldo, dtype=BF), nan_buf(d + 16), nan_buf(d + 16)
    got = run(capi, lambda: capi.lib.dfot_op_qknorm_rope_bwd(P(dev[0]), ld, P(dev[1]), P(dev[2]), P(dev[3]), P(dev[4]), P(dev[5]), P(dev[6]), EPS,
                                                             P(dfused), ldo, P(dqw), P(dkw), rows, ntok, heads, d, S()), [dfused, dqw, dkw])
    vec = d == 64 and ld % 8 == 0 and ldo % 8 == 0
    items = rows * heads
    if vec:
        wblocks = cdiv(items, 8)
        grid = cdiv(wblocks, 4) if wblocks // 4 < 2048 else 2048
        lseq = cdiv(wblocks, grid * 4) + 3
    else:
        grid = cdiv(items, 4) if items // 4 < 1024 else 1024
        lseq = cdiv(items, grid * 4)
    lseq += 2 + cdiv(grid, 16) + 4
    return got, (fused, dq, dk, dv, qw, kw, cs), vec, grid, lseq


def qknorm_check(tag, got, ops, batch, ntok, heads, d, lseq):
    fused, dq, dk, dv = ops[:4]
    c, rows = heads * d, batch * ntok
    ldo = got[0].shape[1]
    (rf, bfu), (rq, bq), (rk, bk) = qknorm_ref(*ops, batch, ntok, heads, d, lseq)
    exp, bar = torch.full((rows, ldo), NAN, dtype=torch.float64), torch.zeros(rows, ldo, dtype=torch.float64)
    exp[:, :3 * c], bar[:, :3 * c] = rf, bfu
    check("qknorm_rope_bwd", tag + " dfused", got[0], exp, bar, nulp=2)                           # columns [3C, ldo) keep their NaN
    vrows = dv.permute(0, 2, 1, 3).reshape(rows, c)
    assert torch.equal(bits(got[0][:, 2 * c:3 * c]), bits(vrows)), "the v columns are a copy"
    check("qknorm_rope_bwd", tag + " dqw", got[1], tail(rq, 16), tail(bq, 16))
    check("qknorm_rope_bwd", tag + " dkw", got[2], tail(rk, 16), tail(bk, 16))


# (d, heads, batch, ntok, ld - 3C, ldo - 3C, kernel): the 16-byte kernel with 15 items (a dead-lane tail in its only wave) | the wave-per-item
# kernel <1> chosen by either row pitch | <2> | <1> with 4680 items on 4096 waves (its grid-stride loop iterates twice) | the 16-byte
# kernel beyond its cap of 2048 workgroups (9225 item blocks on 8192 waves)
QKNORM = [(64, 3, 1, 5, 8, 8, "vec"), (64, 3, 2, 37, 4, 8, "one"), (64, 3, 2, 37, 8, 4, "one"), (128, 2, 3, 21, 2, 2, "one"),
          (64, 9, 1, 520, 4, 4, "one"), (64, 9, 1, 8200, 0, 0, "vec")]


@pytest.mark.parametrize("d,heads,batch,ntok,ld_pad,ldo_pad,kernel", QKNORM)
def test_qknorm_rope_bwd(capi, d, heads, batch, ntok, ld_pad, ldo_pad, kernel):
    got, ops, vec, grid, lseq = qknorm_case(capi, d, heads, batch, ntok, ld_pad, ldo_pad, d + heads + ntok)
    assert vec == (kernel == "vec")
    items = batch * ntok * heads
    if ntok == 5:
        assert items % 8 != 0
    if ntok == 520:
        assert not vec and items > 4096 and grid == 1024
    if ntok == 8200:
        assert vec and grid == 2048 and cdiv(items, 8) > 2048 * 4
    qknorm_check(f"qknorm_rope_bwd d={d} heads={heads} batch={batch} ntok={ntok} ld=3C+{ld_pad} ldo=3C+{ldo_pad} ({kernel})", got, ops, batch, ntok,
                 heads, d, lseq)


def test_qknorm_rope_bwd_both_d64_kernels_agree_within_their_bars(capi):
    """the same operands at row pitches 3C + 8 (16-byte kernel) and 3C + 4 (wave per item): each within its bar of fp64 (checked above for
    the second), and of each other within the sum of both bars.  Not bitwise: the kernels add a head's squares in different orders"""
    d, heads, batch, ntok = 64, 3, 2, 37
    c, rows = heads * d, batch * ntok
    res = {}
    for pad in (8, 4):
        got, ops, vec, _, lseq = qknorm_case(capi, d, heads, batch, ntok, pad, pad, 77)
        assert vec == (pad == 8)
        res[pad] = (got, lseq)
        qknorm_check(f"qknorm_rope_bwd both kernels ({'vec' if vec else 'one'})", got, ops, batch, ntok, heads, d, lseq)
    got8, got4 = res[8][0], res[4][0]
    (rf, bfu), (rq, bq), (rk, bk) = qknorm_ref(*ops, batch, ntok, heads, d, max(res[8][1], res[4][1]))
    a, b = got8[0][:, :3 * c].double(), got4[0][:, :3 * c].double()
    tol = 2 * (bfu + 2 * ulp_bf16(torch.maximum(a.abs(), b.abs())))
    ratio = ((a - b).abs() / tol).max().item()
    for x, y, bw in ((got8[1], got4[1], bq), (got8[2], got4[2], bk)):
        ratio = max(ratio, ((x[:d].double() - y[:d].double()).abs() / (2 * bw)).max().item())
    print(f"qknorm_rope_bwd 16-byte kernel vs wave-per-item kernel: worst difference / summed bars = {ratio:.3f}")
    record("qknorm_vec_vs_one", "d=64 heads=3 batch=2 ntok=37", ratio)
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------ 4. embed_input_dgrad

# (bt, res, cin, c0); the last: 300 patches, more than one workgroup of 256 and no multiple of it
EMBED_DGRAD = [(1, 2, 1, 4), (3, 6, 3, 128), (1, 16, 4, 4), (3, 16, 1, 128), (1, 6, 4, 128), (3, 2, 3, 4), (3, 20, 3, 128)]


@pytest.mark.parametrize("bt,res,cin,c0", EMBED_DGRAD)
def test_embed_input_dgrad(capi, bt, res, cin, c0):
    """dX [BT][cin][R][R] = dx0 [patch][c0] . W [c0][cin][2][2]: the fp64 autograd input gradient of conv2d(k = s = 2)"""
    gen = torch.Generator().manual_seed(bt + res + cin + c0)
    g = res // 2
    dx0 = torch.randn(bt * g * g, c0, generator=gen)
    w = torch.randn(c0, cin, 2, 2, generator=gen) * 0.5
    dd, wd = dx0.cuda(), w.cuda()
    n = bt * cin * res * res
    dx = nan_buf(n + 16)
    got, = run(capi, lambda: capi.lib.dfot_op_embed_input_dgrad(P(dd), P(wd), P(dx), bt, res, cin, c0, 2, S()), [dx])
    gy = dx0.double().view(bt, g, g, c0).permute(0, 3, 1, 2)
    xr = torch.zeros(bt, cin, res, res, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w.double(), stride=2).backward(gy)
    mag = F.conv_transpose2d(gy.abs(), w.double().abs(), stride=2)
    if bt * g * g > 256:
        assert (bt * g * g) % 256 != 0
    check("embed_input_dgrad", f"embed_input_dgrad bt={bt} res={res} cin={cin} c0={c0}", got, tail(xr.grad, 16), tail(seq_bar(c0, mag, xr.grad), 16))


# ------------------------------------------------------------------------------------------------------------- 5. wgrad_nt

@pytest.mark.parametrize("m,n,rows,slices", [(136, 72, 192, 1), (136, 72, 192, 2), (136, 72, 192, 3), (8, 8, 64, 1)])
def test_wgrad_nt_explicit_slices(capi, m, n, rows, slices):
    """out [m][n] = a^T b over the rows with ragged 128 x 128 tiles (m = 136: a second tile 8 wide) and explicit K slices; both operands are
    column blocks of wider matrices whose other columns hold NaN, which a read beyond m / n would carry into the result"""
    gen = torch.Generator().manual_seed(m + n + rows + slices)
    lda, ldb = m + 16, n + 8
    a, b = torch.full((rows, lda), NAN, dtype=BF), torch.full((rows, ldb), NAN, dtype=BF)
    a[:, :m], b[:, :n] = bf(gen, rows, m), bf(gen, rows, n)
    ad, bd = a.cuda(), b.cuda()
    out = nan_buf(m * n + 16)
    got, = run(capi, lambda: capi.lib.dfot_op_wgrad_nt(P(ad), lda, P(bd), ldb, P(out), m, n, rows, slices, S()), [out])
    av, bv = a[:, :m].double(), b[:, :n].double()
    ref, mag = av.t() @ bv, av.abs().t() @ bv.abs()
    check("wgrad_nt", f"wgrad_nt {m}x{n} rows={rows} slices={slices}", got, tail(ref, 16), tail(seq_bar(rows, mag, ref), 16))


# ----------------------------------------------------------------------------------------------------- 6. attention entries

def attn_operands(batch, heads, n, d, ldo, seed, slack=0.0, normed=False):
    """q (in the exp2 domain), k, v [batch][heads][n][dstride] bf16 with zero pad columns, d_o [batch * n][ldo] bf16 with `slack` in the
    columns beyond heads * d; host tensors.  normed: unit-RMS q and k rows, |score| <= sqrt(d) log2(e) < 13 at d = 64"""
    g = torch.Generator().manual_seed(seed + 1000 * n + 10 * heads + d)
    q, k, v = (torch.randn(batch, heads, n, d, generator=g) for _ in range(3))
    mul = 1.5
    if normed:
        q, k = (t / t.pow(2).mean(-1, keepdim=True).sqrt() for t in (q, k))
        mul = 1.0
    ds = 64 if d <= 64 else 128

    def pad(t, s=1.0):
        out = torch.zeros(batch, heads, n, ds, dtype=BF)
        out[..., :d] = (t * s).to(BF)
        return out
    d_o = torch.full((batch * n, ldo), slack, dtype=BF)
    d_o[:, :heads * d] = bf(g, batch * n, heads * d)
    return [pad(q, mul * math.log2(math.e) / math.sqrt(d)), pad(k), pad(v), d_o]


def attn_reference(ops, n, d):
    """fp64 from the bf16 operands: o [batch * n][heads * d], lse (log2 domain), dq (of the UNSCALED q), dk, dv [batch][heads][n][d]"""
    batch, heads = ops[0].shape[:2]
    scale = math.log2(math.e) / math.sqrt(d)
    q = (ops[0][..., :d].double() / scale).requires_grad_()
    k, v = (t[..., :d].double().requires_grad_() for t in ops[1:3])
    s = q @ k.transpose(-1, -2) / math.sqrt(d)
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(batch * n, heads * d)
    o.backward(ops[3][:, :heads * d].double())
    return o.detach(), torch.logsumexp(s.detach(), -1) / math.log(2.0), q.grad, k.grad, v.grad


def attn_fwd(capi, dev, n, d, ldo, bound=None, own_scratch=True):
    """dfot_op_attention_fwd_lse (bound None) or _bounded on NaN-filled o [batch * n][ldo], lse -> device tensors and host copies"""
    batch, heads = dev[0].shape[:2]
    o, lse = nan_buf(batch * n, ldo, dtype=BF), nan_buf(batch, heads, n)
    L = capi.lib
    if bound is None:
        fn = lambda: L.dfot_op_attention_fwd_lse(P(dev[0]), P(dev[1]), P(dev[2]), P(o), ldo, P(lse), batch, heads, n, d, S())
    else:
        need = int(L.dfot_op_attention_scratch_bytes(batch, heads, n, d)) if own_scratch else 0
        scratch = torch.zeros(max(need, 256), dtype=torch.uint8, device="cuda") if own_scratch else None
        fn = lambda: L.dfot_op_attention_fwd_lse_bounded(P(dev[0]), P(dev[1]), P(dev[2]), P(o), ldo, P(lse), batch, heads, n, d, float(bound),
                                                         P(scratch), need, S())
    ho, hl = run(capi, fn, [o, lse])
    return o, lse, ho, hl


def attn_bwd(capi, dev, o, lse, n, d, ldo):
    """dfot_op_attention_bwd_lse on NaN-filled delta, dq, dk, dv -> host copies"""
    batch, heads = dev[0].shape[:2]
    delta = nan_buf(batch, heads, n)
    dq, dk, dv = (torch.full_like(dev[0], NAN) for _ in range(3))
    return run(capi, lambda: capi.lib.dfot_op_attention_bwd_lse(P(dev[0]), P(dev[1]), P(dev[2]), P(o), P(dev[3]), ldo, P(lse), P(delta), P(dq), P(dk),
                                                                P(dv), batch, heads, n, d, S()), [delta, dq, dk, dv])


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def check_fwd(tag, ho, hl, ref, heads, d):
    hd = heads * d
    assert torch.isnan(ho[:, hd:].float()).all(), f"{tag}: the slack columns of o were written"
    assert torch.isfinite(ho[:, :hd].float()).all() and torch.isfinite(hl).all(), tag
    r, e = rel(ho[:, :hd].float(), ref[0]), float((hl.double() - ref[1]).abs().max())
    print(f"{tag}: o rel-L2 {r:.2e}, lse max abs error {e:.2e}")
    record("attention", tag + " o", r / BAR_O)
    record("attention", tag + " lse", e / BAR_LSE)
    assert r < BAR_O and e < BAR_LSE, tag


def check_delta(tag, hdelta, ho, ops, n, heads, d):
    """delta [batch][heads][n] = sum_c o d_o over the head's d columns, from the bf16 o the forward left: n = d exact products"""
    batch = ops[0].shape[0]
    terms = (ho[:, :heads * d].double() * ops[3][:, :heads * d].double()).view(batch, n, heads, d).permute(0, 2, 1, 3)
    ref, mag = terms.sum(-1), terms.abs().sum(-1)
    check("attention_delta", tag + " delta", hdelta, ref, seq_bar(d, mag, ref))


def check_grads(tag, got, ref, d):
    for name, g, w in zip(("dq", "dk", "dv"), got, ref[2:]):
        g = g.float()
        assert torch.isfinite(g).all(), f"{tag} {name}"
        assert not g[..., d:].any(), f"{tag} {name}: the pad columns are written as zero"
        r = rel(g[..., :d], w)
        print(f"{tag} {name}: rel-L2 {r:.2e}")
        record("attention", f"{tag} {name}", r / BAR_GRAD)
        assert r < BAR_GRAD, f"{tag} {name}"


# rows<8> (d = 64), rows<16> (d = 128), the LDS kernel (d = 72: 18 chunks per row), and heads * d / 8 = 1080 > 1024: the generic kernel
ATTN = [(2, 2, 128, 64), (2, 2, 256, 128), (2, 2, 128, 72), (1, 120, 128, 72)]


@pytest.mark.parametrize("batch,heads,n,d", ATTN)
def test_attention_fwd_lse_and_bwd_lse(capi, batch, heads, n, d):
    """o and lse of dfot_op_attention_fwd_lse, then delta (element-wise, fp32 bar) and dq / dk / dv of dfot_op_attention_bwd_lse"""
    ldo = heads * d
    ops = attn_operands(batch, heads, n, d, ldo, seed=1)
    dev = [t.cuda() for t in ops]
    ref = attn_reference(ops, n, d)
    tag = f"attention batch={batch} heads={heads} n={n} d={d}"
    o, lse, ho, hl = attn_fwd(capi, dev, n, d, ldo)
    check_fwd(tag + " fwd_lse", ho, hl, ref, heads, d)
    hdelta, *grads = attn_bwd(capi, dev, o, lse, n, d, ldo)
    check_delta(tag + " bwd_lse", hdelta, ho, ops, n, heads, d)
    check_grads(tag + " bwd_lse", grads, ref, d)


@pytest.mark.parametrize("d", [64, 72])
def test_attention_row_pitch_with_slack(capi, d):
    """ldo = heads * d + 8: the forward leaves the 8 slack columns of o NaN, and the backward gives the same bits whether the slack of o and
    d_o holds NaN or zeros"""
    batch, heads, n = 2, 2, 128
    ldo = heads * d + 8
    ops = attn_operands(batch, heads, n, d, ldo, seed=2, slack=NAN)
    dev = [t.cuda() for t in ops]
    ref = attn_reference(ops, n, d)
    tag = f"attention ldo=heads*d+8 d={d}"
    o, lse, ho, hl = attn_fwd(capi, dev, n, d, ldo)
    check_fwd(tag + " fwd_lse", ho, hl, ref, heads, d)
    with_nan = attn_bwd(capi, dev, o, lse, n, d, ldo)
    check_delta(tag + " bwd_lse", with_nan[0], ho, ops, n, heads, d)
    check_grads(tag + " bwd_lse", with_nan[1:], ref, d)
    oz, doz = o.clone(), dev[3].clone()
    oz[:, heads * d:] = 0
    doz[:, heads * d:] = 0
    with_zero = attn_bwd(capi, dev[:3] + [doz], oz, lse, n, d, ldo)
    for name, a, b in zip(("delta", "dq", "dk", "dv"), with_nan, with_zero):
        assert torch.equal(bits(a), bits(b)), f"{tag}: {name} depends on the slack columns"


def test_attention_fwd_lse_bounded(capi):
    """d = 64, n = 256: bound 13 takes the no-running-max kernel (attention_v5.hip), with the caller's scratch and with a null scratch (equal
    bits); bound inf takes the padded kernel.  o and lse of each against fp64, and the gradients dfot_op_attention_bwd_lse makes of each lse"""
    batch, heads, n, d = 2, 2, 256, 64
    ldo = heads * d
    ops = attn_operands(batch, heads, n, d, ldo, seed=3, normed=True)
    dev = [t.cuda() for t in ops]
    s2 = ops[0].double() @ ops[1].double().transpose(-1, -2)
    assert float(s2.abs().max()) < 13.0
    ref = attn_reference(ops, n, d)
    res = {}
    for name, bound, own in (("bound 13 caller scratch", 13.0, True), ("bound 13 null scratch", 13.0, False), ("bound inf", math.inf, True)):
        tag = f"attention bounded {name}"
        o, lse, ho, hl = attn_fwd(capi, dev, n, d, ldo, bound=bound, own_scratch=own)
        check_fwd(tag, ho, hl, ref, heads, d)
        res[name] = (ho, hl)
        if own:
            hdelta, *grads = attn_bwd(capi, dev, o, lse, n, d, ldo)
            check_delta(tag + " bwd_lse", hdelta, ho, ops, n, heads, d)
            check_grads(tag + " bwd_lse", grads, ref, d)
    for a, b in zip(res["bound 13 caller scratch"], res["bound 13 null scratch"]):
        assert torch.equal(bits(a), bits(b)), "the caller's scratch and the library's give different bits"


@pytest.mark.parametrize("d", [64, 72])
def test_attention_batch_elements_are_independent_bit_for_bit(capi, d):
    """a batch of 2 equals two calls with a batch of 1, for o, lse, delta, dq, dk, dv"""
    batch, heads, n = 2, 2, 128
    ldo = heads * d
    ops = attn_operands(batch, heads, n, d, ldo, seed=4)
    dev = [t.cuda() for t in ops]
    o, lse, ho, hl = attn_fwd(capi, dev, n, d, ldo)
    full = [ho.view(batch, n, ldo), hl] + attn_bwd(capi, dev, o, lse, n, d, ldo)
    for b in range(batch):
        one = [t[b:b + 1].contiguous() for t in dev[:3]] + [dev[3].view(batch, n, ldo)[b].contiguous()]
        o1, lse1, ho1, hl1 = attn_fwd(capi, one, n, d, ldo)
        alone = [ho1.view(1, n, ldo), hl1] + attn_bwd(capi, one, o1, lse1, n, d, ldo)
        for name, a, f in zip(("o", "lse", "delta", "dq", "dk", "dv"), alone, full):
            assert torch.equal(bits(a), bits(f[b:b + 1])), f"d={d} batch element {b}: {name} depends on the rest of the batch"


@pytest.mark.parametrize("d", [64, 72])
def test_attention_bwd_entry(capi, d):
    """dfot_op_attention_bwd (forward + backward in one call, temporaries its own): o, dq, dk, dv at n = 128, ldo = heads * d + 8"""
    batch, heads, n = 2, 2, 128
    ldo = heads * d + 8
    ops = attn_operands(batch, heads, n, d, ldo, seed=5)
    dev = [t.cuda() for t in ops]
    ref = attn_reference(ops, n, d)
    o = nan_buf(batch * n, ldo, dtype=BF)
    dq, dk, dv = (torch.full_like(dev[0], NAN) for _ in range(3))
    ho, *grads = run(capi, lambda: capi.lib.dfot_op_attention_bwd(P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), P(o), ldo, P(dq), P(dk), P(dv), batch,
                                                                  heads, n, d, S()), [o, dq, dk, dv])
    tag = f"attention_bwd entry d={d}"
    hd = heads * d
    assert torch.isnan(ho[:, hd:].float()).all() and torch.isfinite(ho[:, :hd].float()).all()
    r = rel(ho[:, :hd].float(), ref[0])
    record("attention", tag + " o", r / BAR_O)
    assert r < BAR_O
    check_grads(tag, grads, ref, d)


# --------------------------------------------------------------------------------------------------------------------- refusals

def refusal_cases(capi):
    """name -> (expected status, call(buffers)).  Inputs are FINITE (`xf` fp32, `xh` bf16: a kernel that ran would write finite values),
    outputs NaN-filled (`f` .. `f4` fp32, `h` .. `h4` bf16); every buffer is 2^20 elements long, so that a check that is missing does not
    turn the call into an out-of-bounds launch"""
    L, A, SH = capi.lib, capi.ERR_ARG, capi.ERR_SHAPE
    N = None

    def gn5(b, c, film=None, dfilm=None, ld=0):
        return L.dfot_op_gn_silu_bwd5(P(b["xf"]), P(b["xh"]), P(b["xf"]), P(b["xf"]), P(b["xf"]), film, N, P(b["f"]), P(b["h"]), dfilm, ld, P(b["f2"]),
                                      P(b["f3"]), 1, 64, c, S())

    def gn6(b, c, fld, dld):
        return L.dfot_op_gn_silu_bwd6(P(b["xf"]), P(b["xh"]), P(b["xf"]), P(b["xf"]), P(b["xf"]), P(b["xh"]), fld, N, P(b["f"]), P(b["h"]), P(b["h2"]), dld,
                                      P(b["f2"]), P(b["f3"]), 1, 64, c, S())

    def conv2(b, dx, dxb, ci=64, w=16):
        return L.dfot_op_conv3x3_bwd2(P(b["xh"]), P(b["xh"]), P(b["xf"]), dx, dxb, P(b["f2"]), P(b["f3"]), 1, 8, w, ci, 64, S())

    def dgrad(b, res, cin, c0, ps):
        return L.dfot_op_embed_input_dgrad(P(b["xf"]), P(b["xf"]), P(b["f"]), 2, res, cin, c0, ps, S())

    def wg(b, lda, m, rows, slices):
        return L.dfot_op_wgrad_nt(P(b["xh"]), lda, P(b["xh"]), 80, P(b["f"]), m, 72, rows, slices, S())

    def bwd_lse(b, n, d, ldo, q=True):
        return L.dfot_op_attention_bwd_lse(P(b["xh"]) if q else N, P(b["xh"]), P(b["xh"]), P(b["xh"]), P(b["xh"]), ldo, P(b["xf"]), P(b["f"]), P(b["h"]),
                                           P(b["h2"]), P(b["h3"]), 2, 2, n, d, S())

    def bwd(b, n, d, ldo, q=True):
        return L.dfot_op_attention_bwd(P(b["xh"]) if q else N, P(b["xh"]), P(b["xh"]), P(b["xh"]), P(b["h4"]), ldo, P(b["h"]), P(b["h2"]), P(b["h3"]),
                                       2, 2, n, d, S())
    return {
        "conv3x3_bwd2 dx and dx_bf": (A, lambda b: conv2(b, P(b["f"]), P(b["h"]))),
        "conv3x3_bwd2 neither dx nor dx_bf": (A, lambda b: conv2(b, N, N)),
        "conv3x3_bwd2 ci = 96": (SH, lambda b: conv2(b, P(b["f"]), N, ci=96)),
        "conv3x3_bwd2 64 pixels": (SH, lambda b: conv2(b, P(b["f"]), N, w=8)),
        "conv3x3_bwd2 64 pixels dx_bf": (SH, lambda b: conv2(b, N, P(b["h"]), w=8)),
        "conv3x3_bwd ci = 96": (SH, lambda b: L.dfot_op_conv3x3_bwd(P(b["xh"]), P(b["xh"]), P(b["xf"]), P(b["f"]), P(b["f2"]), P(b["f3"]), 1, 8, 16, 96, 64,
                                                                    S())),
        "conv3x3_bwd null dx": (A, lambda b: L.dfot_op_conv3x3_bwd(P(b["xh"]), P(b["xh"]), P(b["xf"]), N, P(b["f2"]), P(b["f3"]), 1, 8, 16, 64, 64, S())),
        "gn_silu_fwd2 C = 384": (SH, lambda b: L.dfot_op_gn_silu_fwd2(P(b["xf"]), P(b["xf"]), P(b["xf"]), N, 768, EPS, P(b["h"]), P(b["f"]), 1, 64, 384,
                                                                      S())),
        "gn_silu_fwd C = 384": (SH, lambda b: L.dfot_op_gn_silu_fwd(P(b["xf"]), P(b["xf"]), P(b["xf"]), P(b["xh"]), EPS, P(b["h"]), P(b["f"]), 1, 64, 384,
                                                                    S())),
        "gn_silu_bwd5 C = 384": (A, lambda b: gn5(b, 384)),
        "gn_silu_bwd6 C = 384": (A, lambda b: gn6(b, 384, 768, 768)),
        "gn_silu_bwd C = 384": (A, lambda b: L.dfot_op_gn_silu_bwd(P(b["xf"]), P(b["xf"]), P(b["xf"]), P(b["xf"]), N, EPS, P(b["f"]), N, P(b["f2"]),
                                                                   P(b["f3"]), 1, 64, 384, S())),
        "gn_silu_bwd5 film without dfilm": (A, lambda b: gn5(b, 128, film=P(b["xh"]))),
        "gn_silu_bwd5 dfilm_ld < 2C": (A, lambda b: gn5(b, 128, film=P(b["xh"]), dfilm=P(b["h2"]), ld=128)),
        "gn_silu_bwd6 film_ld < 2C": (A, lambda b: gn6(b, 128, 128, 256)),
        "qknorm_rope_bwd d = 96": (SH, lambda b: L.dfot_op_qknorm_rope_bwd(P(b["xh"]), 576, P(b["xh"]), P(b["xh"]), P(b["xh"]), P(b["xf"]), P(b["xf"]),
                                                                           P(b["xf"]), EPS, P(b["h"]), 576, P(b["f"]), P(b["f2"]), 8, 4, 2, 96, S())),
        "embed_input_dgrad ps = 4": (SH, lambda b: dgrad(b, 8, 3, 128, 4)),
        "embed_input_dgrad cin = 5": (SH, lambda b: dgrad(b, 8, 5, 128, 2)),
        "embed_input_dgrad c0 = 6": (SH, lambda b: dgrad(b, 8, 3, 6, 2)),
        "embed_input_dgrad odd res": (SH, lambda b: dgrad(b, 7, 3, 128, 2)),
        "embed_input_dgrad null": (A, lambda b: L.dfot_op_embed_input_dgrad(P(b["xf"]), N, P(b["f"]), 2, 8, 3, 128, 2, S())),
        "wgrad_nt slices > rows / 64": (SH, lambda b: wg(b, 144, 136, 192, 4)),
        "wgrad_nt m = 12": (SH, lambda b: wg(b, 16, 12, 192, 1)),
        "wgrad_nt rows = 100": (SH, lambda b: wg(b, 144, 136, 100, 1)),
        "wgrad_nt lda = m + 4": (SH, lambda b: wg(b, 140, 136, 192, 1)),
        "attention_bwd_lse n = 192": (SH, lambda b: bwd_lse(b, 192, 64, 128)),
        "attention_bwd_lse d = 12": (SH, lambda b: bwd_lse(b, 128, 12, 24)),
        "attention_bwd_lse ldo % 8": (SH, lambda b: bwd_lse(b, 128, 64, 132)),
        "attention_bwd_lse null": (A, lambda b: bwd_lse(b, 128, 64, 128, q=False)),
        "attention_bwd n = 192": (SH, lambda b: bwd(b, 192, 64, 128)),
        "attention_bwd d = 12": (SH, lambda b: bwd(b, 128, 12, 24)),
        "attention_bwd ldo % 8": (SH, lambda b: bwd(b, 128, 64, 132)),
        "attention_bwd null": (A, lambda b: bwd(b, 128, 64, 128, q=False)),
    }


REFUSALS = ["conv3x3_bwd2 dx and dx_bf", "conv3x3_bwd2 neither dx nor dx_bf", "conv3x3_bwd2 ci = 96", "conv3x3_bwd2 64 pixels",
            "conv3x3_bwd2 64 pixels dx_bf", "conv3x3_bwd ci = 96", "conv3x3_bwd null dx",
            "gn_silu_fwd2 C = 384", "gn_silu_fwd C = 384", "gn_silu_bwd5 C = 384", "gn_silu_bwd6 C = 384", "gn_silu_bwd C = 384",
            "gn_silu_bwd5 film without dfilm", "gn_silu_bwd5 dfilm_ld < 2C", "gn_silu_bwd6 film_ld < 2C", "qknorm_rope_bwd d = 96",
            "embed_input_dgrad ps = 4", "embed_input_dgrad cin = 5", "embed_input_dgrad c0 = 6", "embed_input_dgrad odd res", "embed_input_dgrad null",
            "wgrad_nt slices > rows / 64", "wgrad_nt m = 12", "wgrad_nt rows = 100", "wgrad_nt lda = m + 4", "attention_bwd_lse n = 192",
            "attention_bwd_lse d = 12", "attention_bwd_lse ldo % 8", "attention_bwd_lse null", "attention_bwd n = 192", "attention_bwd d = 12",
            "attention_bwd ldo % 8", "attention_bwd null"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusal(capi, case):
    """the entry point returns the documented status and writes nothing: every output buffer, delta and o included, keeps its NaN fill"""
    cases = refusal_cases(capi)
    assert set(cases) == set(REFUSALS)
    code, call = cases[case]
    gen = torch.Generator().manual_seed(9)
    bufs = {"xf": (torch.rand(1 << 20, generator=gen) + 0.5).cuda(), "xh": (torch.rand(1 << 20, generator=gen) + 0.5).to(BF).cuda()}
    outs = {k: nan_buf(1 << 20) for k in ("f", "f2", "f3", "f4")}
    outs.update({k: nan_buf(1 << 20, dtype=BF) for k in ("h", "h2", "h3", "h4")})
    bufs.update(outs)
    got = call(bufs)
    torch.cuda.synchronize()
    assert got == code, f"{case}: status {got}, expected {code} ({capi.lib.dfot_last_error().decode()})"
    for k, t in outs.items():
        assert torch.isnan(t.float()).all(), f"{case}: buffer {k} was written"
