"""The DiT block kernels at op level: every dfot_op_dit_* entry point (one launch of the inference or training engine each, through the
engine's own launcher) against the float64 restatements of tests/dit_block_common.py.

Inputs keep layout mistakes visible: the modulation table's row stride is larger than what an op touches and the op's columns start at a
non-zero offset; every frame reads a different table row with O(1) shift, scale and gate; ln_mod's noise levels include -1 and max_level + 1
(both clamped); data has a non-zero mean (1.5 randn + 0.3); outputs an op overwrites are pre-filled with NaN, outputs it accumulates into
with a known non-zero value; buffers an op writes in part are compared bit for bit outside that part; every op runs twice and the two
results have the same bits.

Bars (none taken from the kernel under test):
  bit-exact     pure data movement (gathers, the pack without rotation, padding, untouched regions) and one fp32 operation rounded to
                bf16 (da = bf16(dy * gate), final_gather): equal to torch's fp32 product cast to bf16.  f2bf is the compiler's float ->
                __bf16 conversion, round-to-nearest-even as torch's; no input class of these tests rounds differently.
  bf16 of fp32  |got - ref64| <= 2^-8 |ref64| + slack for every element; slack = 8 x the max-abs error of the float64 formula evaluated by
                torch in float32 on the same inputs.
  fp32          error against float64 (max-abs and rel-L2) at most 8 x that of the same formula evaluated by torch in float32 (e32).
  fp32 sums     |got - ref64| <= (N + 4) 2^-24 sum |terms| per element, N additions, the terms evaluated in float64 from the kernel's own
                intermediates where it has them (xhat from the fp32 stats it stored, da as it stored it).

Measured on one MI355X (kernel max-abs / rel-L2 against float64; e32 = torch float32 on the same inputs):
  ln_mod fp32 out (20 cases)            max-abs 6.1e-07 .. 1.6e-06, rel-L2 4.7e-08 .. 5.9e-08; at most 1.21 x e32's max-abs, 0.98 x its rel-L2
  ln_mod / gelu / rotated pack bf16     worst |err| / (2^-8 |ref| + slack) 0.994 / 0.988 / 0.995 (gelu: h max-abs 7.8e-03, du 1.5e-02, bf16 steps)
  ln_bwd dx (56 cases)                  max-abs 5.0e-07 .. 2.1e-06, rel-L2 4.9e-08 .. 7.8e-08; at most 2.27 x / 1.24 x e32
  ln_bwd stats (mean, rstd)             max-abs 2.9e-08 .. 7.6e-08, rel-L2 2.7e-08 .. 5.1e-08; at most 1.97 x / 1.40 x e32
  gate_combine (36 cases)               max-abs 2.2e-07 .. 8.9e-07, rel-L2 2.3e-08 .. 2.6e-08; at most 0.95 x / 0.84 x e32
  dshift | dscale planes, dmod          max-abs 1.8e-07 .. 7.5e-06, rel-L2 2.0e-08 .. 8.7e-08; worst |err| / bound 0.49 (planes), 0.35 (dmod)
  dgate planes, dmod                    max-abs 1.9e-07 .. 1.0e-05, rel-L2 2.3e-08 .. 9.9e-08; worst |err| / bound 0.31
  dbias partial rows, dbias             max-abs 0 .. 7.6e-06, rel-L2 0 .. 2.5e-08; worst |err| / bound 0.042
  patch_embed (with / without pos)      max-abs 5.0e-07 .. 5.2e-06, rel-L2 3.9e-08 .. 2.9e-07; worst |err| / bound 0.25
  patch_embed_dgrad                     max-abs 1.9e-06 .. 5.0e-05, rel-L2 1.4e-07 .. 6.2e-07; worst |err| / bound 0.052
  patch_embed_wgrad dW, db (104, 128)   max-abs 4.8e-06 .. 3.1e-05, rel-L2 4.6e-08 .. 1.4e-07; worst |err| / bound 0.025
  patch_embed_wgrad 131080 / 524296     dW max-abs 2.9e-03 / 7.6e-03, db 5.4e-03 / 2.5e-02, rel-L2 6.2e-08 .. 7.0e-08; worst |err| / blocked bound 0.003
  da, final_gather, plain pack, padding, untouched columns, run-to-run: bit-equal in every case
"""
import functools
import zlib

import pytest
import torch

import dit_block_common as bc
from dit_block_common import bits

pytestmark = pytest.mark.gpu

OFF = 64  # column of the op's first modulation entry inside a table row


def P(t):
    from dfot_amd import capi
    return capi.ptr(t)


_alive = []


def D(t):
    """device pointer of a copy of a host tensor; the copy is kept until twice() has synchronised (a temporary would be freed, and its
    memory handed to the next allocation, before the launch that reads it)"""
    _alive.append(t.cuda())
    return P(_alive[-1])


def ok(rc):
    from dfot_amd import capi
    assert rc == capi.OK, capi.lib.dfot_last_error()


def stream():
    from dfot_amd import capi
    return capi.stream_ptr()


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def data(g, *shape):
    return 1.5 * torch.randn(*shape, generator=g) + 0.3


def twice(fn):
    """runs an op twice on fresh output buffers: the kernels are deterministic, so the two results have the same bits"""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    _alive.clear()
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y)), "two runs of one op differ"
    return a


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


# ---- ln_mod and the LayerNorm backward ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ln_case(hidden, rows, per_frame):
    """x, dm, the table, the levels (a permutation of the table's rows with the first row asked for as -1 and the last as max_level + 1)"""
    g = gen("ln", hidden, rows, per_frame)
    frames = rows // per_frame
    x, dm = data(g, rows, hidden), data(g, rows, hidden)
    ldt = OFF + 3 * hidden + 32
    table = torch.randn(frames, ldt, generator=g)
    rows_of = torch.randperm(frames, generator=g)
    levels = rows_of.clone()
    levels[rows_of == 0] = -1
    levels[rows_of == frames - 1] = frames
    return x, dm, table, levels.int(), rows_of


@functools.lru_cache(maxsize=None)
def ln_reference(hidden, rows, per_frame):
    """float64 and float32 evaluations of the forward and (autograd) of its backward for dm"""
    x, dm, table, _, rows_of = ln_case(hidden, rows, per_frame)
    out = {}
    for dt in (torch.float64, torch.float32):
        xx = x.to(dt).clone().requires_grad_()  # (a copy: x.to(float32) is x itself, which the other tests share)
        sh = table[rows_of, OFF:OFF + hidden].to(dt).requires_grad_()
        sc = table[rows_of, OFF + hidden:OFF + 2 * hidden].to(dt).requires_grad_()
        m = bc.ln_mod(xx, sh, sc, per_frame)
        dx, dsh, dsc = torch.autograd.grad(m, (xx, sh, sc), dm.to(dt))
        mean = xx.detach().mean(-1)
        rstd = 1 / torch.sqrt(xx.detach().var(-1, unbiased=False) + bc.EPS)
        out[dt] = dict(m=m.detach(), dx=dx, dshift=dsh, dscale=dsc, stats=torch.stack((mean, rstd), -1))
    return out[torch.float64], out[torch.float32]


def run_ln_mod(hidden, rows, per_frame, in_place):
    from dfot_amd import capi
    x, _, table, levels, _ = ln_case(hidden, rows, per_frame)
    xin = x.cuda()
    xout = xin if in_place else nan(rows, hidden)
    obf = nan(rows, hidden, dtype=torch.bfloat16)
    ok(capi.lib.dfot_op_dit_ln_mod(P(xin), P(xout), P(obf), D(table), D(levels), table.shape[1], OFF, hidden, per_frame, rows, bc.EPS,
                                   table.shape[0] - 1, stream()))
    return xout, obf


LN_SHAPES = [(h, 21, 7) for h in bc.LN_WIDTHS] + [(h, 256, 16) for h in (128, 320, 1152)]


@pytest.mark.parametrize("hidden,rows,per_frame", LN_SHAPES)
def test_ln_mod(hidden, rows, per_frame):
    """every width of the dispatch at 21 rows (3 frames x 7: ragged against the 4-rows-per-workgroup grid), three widths at 256 rows"""
    r64, r32 = ln_reference(hidden, rows, per_frame)
    out, obf = twice(lambda: run_ln_mod(hidden, rows, per_frame, False))
    out_ip, obf_ip = run_ln_mod(hidden, rows, per_frame, True)
    assert torch.equal(bits(out), bits(out_ip)) and torch.equal(bits(obf), bits(obf_ip))  # xout == xin gives the same bits
    bc.assert_fp32_within(f"ln_mod fp32 hidden {hidden} rows {rows}", out.cpu(), r64["m"], r32["m"])
    slack = 8 * bc.errors(r32["m"], r64["m"])[0]
    bc.assert_bf16_of_fp32(f"ln_mod bf16 hidden {hidden} rows {rows}", obf.cpu(), r64["m"], slack)
    # the bf16 copy is the rounding of the fp32 output the kernel stored
    assert torch.equal(bits(obf), bits(out.bfloat16()))


def run_ln_bwd(hidden, rows, per_frame, frames_part):
    """the trainer's per-frame table: row f belongs to frame f (the rows of ln_case's table in the frames' order)"""
    from dfot_amd import capi
    x, dm, table, _, rows_of = ln_case(hidden, rows, per_frame)
    frames = rows // per_frame
    t = table[rows_of].contiguous().cuda()
    ldt = t.shape[1]
    dx, stats = nan(rows, hidden), nan(rows, 2)
    if not frames_part:
        ok(capi.lib.dfot_op_dit_ln_bwd_rows(D(dm), D(x), P(t), ldt, OFF, P(dx), P(stats), hidden, per_frame, frames, bc.EPS, stream()))
        return dx, stats
    part, dmod = sentinel(4, frames, ldt).cuda(), nan(frames, ldt)
    ok(capi.lib.dfot_op_dit_ln_bwd(D(dm), D(x), P(t), ldt, OFF, P(dx), P(stats), P(part), P(dmod), hidden, per_frame, frames, bc.EPS,
                                   stream()))
    return dx, stats, part, dmod


def sentinel(*shape):
    """a known finite, non-zero fill for buffers an op writes in part"""
    return torch.randn(*shape, generator=gen("sentinel", *shape)) + 3.0


def check_ln_rows(name, dx, stats, r64, r32):
    bc.assert_fp32_within(f"{name} dx", dx.cpu(), r64["dx"], r32["dx"])
    bc.assert_fp32_within(f"{name} stats", stats.cpu(), r64["stats"], r32["stats"])


def check_planes(name, part, dmod, col0, width, terms, per_frame):
    """part [4][frames][ldt], dmod [frames][ldt]; terms [frames][per_frame][width] float64: plane z holds the sum of rows [z per/4, (z+1)
    per/4) of every frame at columns [col0, col0 + width), nothing else of dmod_part is written, and dmod is the planes added in a fixed order"""
    frames, ldt = dmod.shape
    per = per_frame // 4
    want = sentinel(4, frames, ldt)
    inside = torch.zeros(ldt, dtype=torch.bool)
    inside[col0:col0 + width] = True
    assert torch.equal(bits(part.cpu()[:, :, ~inside]), bits(want[:, :, ~inside])), f"{name}: dmod_part written outside its columns"
    p = part.cpu()
    assert torch.equal(bits(dmod.cpu()), bits((p[0] + p[1]) + (p[2] + p[3]))), f"{name}: dmod is not the fixed-order sum of the four planes"
    chunks = terms.reshape(frames, 4, per, width)
    for z in range(4):
        bc.assert_sum_bound(f"{name} plane {z}", p[z][:, col0:col0 + width], chunks[:, z].sum(1), chunks[:, z].abs().sum(1), per)
    # the reduced value against the whole frame's sum: per additions in a chunk, then three for the planes
    bc.assert_sum_bound(f"{name} dmod", dmod.cpu()[:, col0:col0 + width], terms.sum(1), terms.abs().sum(1), per + 3)


@pytest.mark.parametrize("hidden", bc.LN_WIDTHS)
def test_ln_bwd_rows_every_width(hidden):
    r64, r32 = ln_reference(hidden, 21, 7)
    dx, stats = twice(lambda: run_ln_bwd(hidden, 21, 7, False))
    check_ln_rows(f"ln_bwd_rows hidden {hidden} rows 21", dx, stats, r64, r32)


def kernel_xhat(x, stats):
    """xhat as ln_bwd_frames forms it, from the stats the row kernel stored, in float64"""
    s = stats.cpu().double()
    return (x.double() - s[:, :1]) * s[:, 1:]


@pytest.mark.parametrize("hidden", [128, 320, 1152])
def test_ln_bwd_256_rows(hidden):
    rows, per_frame = 256, 16
    x, dm, _, _, _ = ln_case(hidden, rows, per_frame)
    r64, r32 = ln_reference(hidden, rows, per_frame)
    dx, stats, part, dmod = twice(lambda: run_ln_bwd(hidden, rows, per_frame, True))
    check_ln_rows(f"ln_bwd hidden {hidden} rows {rows}", dx, stats, r64, r32)
    frames = rows // per_frame
    terms = torch.cat((dm.double(), dm.double() * kernel_xhat(x, stats)), 1).reshape(frames, per_frame, 2 * hidden)
    check_planes(f"ln_bwd hidden {hidden} rows {rows} (dshift | dscale)", part, dmod, OFF, 2 * hidden, terms, per_frame)
    # autograd's own dshift is the same sum of dm; its dscale differs from the terms above by the rounding of the stats, held just above
    bc.assert_sum_bound(f"ln_bwd hidden {hidden} rows {rows} dshift vs autograd", dmod.cpu()[:, OFF:OFF + hidden], r64["dshift"],
                        terms[:, :, :hidden].abs().sum(1), per_frame // 4 + 3)


# ---- gate_combine, gate_bwd and the frame part of ln_bwd ---------------------------------------------------------------------
FRAME_SHAPES = [(h, p, f) for h in (64, 320, 768, 1152) for p in (4, 8, 64) for f in (1, 3, 5)]


@functools.lru_cache(maxsize=None)
def gate_case(hidden, per_frame, frames):
    g = gen("gate", hidden, per_frame, frames)
    rows = frames * per_frame
    x, dy = data(g, rows, hidden), data(g, rows, hidden)
    a = data(g, rows, hidden).bfloat16()
    table = torch.randn(frames, OFF + 3 * hidden + 32, generator=g)
    return x, dy, a, table


@pytest.mark.parametrize("hidden,per_frame,frames", FRAME_SHAPES)
def test_gate_combine(hidden, per_frame, frames):
    from dfot_amd import capi
    x, _, a, table = gate_case(hidden, per_frame, frames)
    rows, off = frames * per_frame, OFF + 2 * hidden  # the gate is the third entry of (shift | scale | gate)

    def run():
        y = nan(rows, hidden)
        ok(capi.lib.dfot_op_dit_gate_combine(D(x), P(y), D(a), D(table), table.shape[1], off, hidden, per_frame, rows, stream()))
        return (y,)
    (y,) = twice(run)
    gate = table[:, off:off + hidden]
    r64 = bc.gate_combine(x.double(), a.double(), gate.double(), per_frame)
    r32 = bc.gate_combine(x, a.float(), gate, per_frame)
    bc.assert_fp32_within(f"gate_combine hidden {hidden} per_frame {per_frame} frames {frames}", y.cpu(), r64, r32)


@pytest.mark.parametrize("hidden,per_frame,frames", FRAME_SHAPES)
def test_gate_bwd(hidden, per_frame, frames):
    from dfot_amd import capi
    _, dy, a, table = gate_case(hidden, per_frame, frames)
    rows, off, ldt = frames * per_frame, OFF + 2 * hidden, table.shape[1]

    def run():
        da = nan(rows, hidden, dtype=torch.bfloat16)
        part, dmod = sentinel(4, frames, ldt).cuda(), nan(frames, ldt)
        dbias_part, dbias = nan(4 * frames, hidden), nan(hidden)
        ok(capi.lib.dfot_op_dit_gate_bwd(D(dy), D(a), D(table), ldt, off, P(da), P(part), P(dbias_part), P(dbias), P(dmod), hidden,
                                         per_frame, frames, stream()))
        return da, part, dmod, dbias_part, dbias
    da, part, dmod, dbias_part, dbias = twice(run)
    name = f"gate_bwd hidden {hidden} per_frame {per_frame} frames {frames}"
    gate = bc.per_row(table[:, off:off + hidden], per_frame)
    assert torch.equal(bits(da.cpu()), bits((dy * gate).bfloat16())), f"{name}: da is not bf16(dy * gate)"
    # dgate: the planes, their untouched columns and the reduced table row
    terms = (dy.double() * a.double()).reshape(frames, per_frame, hidden)
    check_planes(f"{name} dgate", part, dmod, off, hidden, terms, per_frame)
    # dbias: one partial row per (frame, chunk) of da as stored, then all of them
    per = per_frame // 4
    das = da.cpu().double().reshape(frames * 4, per, hidden)
    bc.assert_sum_bound(f"{name} dbias partial rows", dbias_part.cpu(), das.sum(1), das.abs().sum(1), per)
    bc.assert_sum_bound(f"{name} dbias", dbias.cpu(), das.sum((0, 1)), das.abs().sum((0, 1)), rows)


@pytest.mark.parametrize("hidden,per_frame,frames", [s for s in FRAME_SHAPES if s[0] != 320])
def test_ln_bwd_frame_part(hidden, per_frame, frames):
    """(320 has no training engine behind it -- the trainer takes multiples of 128 -- but the op takes it: see the next test)"""
    _check_ln_bwd_frames(hidden, per_frame, frames)


@pytest.mark.parametrize("per_frame,frames", [(4, 1), (4, 3), (4, 5), (8, 1), (8, 3), (8, 5), (64, 1), (64, 3), (64, 5)])
def test_ln_bwd_frame_part_partly_live_channel_block(per_frame, frames):
    """hidden 320: the second 256-channel block of the frame reduction has 64 live threads"""
    _check_ln_bwd_frames(320, per_frame, frames)


def _check_ln_bwd_frames(hidden, per_frame, frames):
    rows = frames * per_frame
    x, dm, _, _, _ = ln_case(hidden, rows, per_frame)
    r64, r32 = ln_reference(hidden, rows, per_frame)
    dx, stats, part, dmod = twice(lambda: run_ln_bwd(hidden, rows, per_frame, True))
    name = f"ln_bwd hidden {hidden} per_frame {per_frame} frames {frames}"
    check_ln_rows(name, dx, stats, r64, r32)
    terms = torch.cat((dm.double(), dm.double() * kernel_xhat(x, stats)), 1).reshape(frames, per_frame, 2 * hidden)
    check_planes(f"{name} (dshift | dscale)", part, dmod, OFF, 2 * hidden, terms, per_frame)
    bc.assert_sum_bound(f"{name} dshift vs autograd", dmod.cpu()[:, OFF:OFF + hidden], r64["dshift"], terms[:, :, :hidden].abs().sum(1),
                        per_frame // 4 + 3)


# ---- GELU --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gelu_case(n):
    g = gen("gelu", n)
    u = torch.linspace(-8, 8, n)[torch.randperm(n, generator=g)]
    u[0], u[1], u[2], u[3], u[4] = 0.0, -0.0, 8.0, -8.0, 0.0
    u = u.bfloat16()
    dh = data(g, n).bfloat16()
    out = {}
    for dt in (torch.float64, torch.float32):
        uu = u.to(dt).requires_grad_()
        h = bc.gelu_tanh(uu)
        (du,) = torch.autograd.grad(h, uu, dh.to(dt))
        out[dt] = (h.detach(), du)
    return u, dh, out[torch.float64], out[torch.float32]


@pytest.mark.parametrize("n", [8, 8 * 257, 64 * 1536])
def test_gelu(n):
    """one thread, a ragged grid (257 threads) and an MLP-sized activation; forward only, backward only (h null) and both"""
    from dfot_amd import capi
    u, dh, (h64, du64), (h32, du32) = gelu_case(n)

    def run(fwd, bwd):
        h = nan(n, dtype=torch.bfloat16) if fwd else None
        d = dh.cuda() if bwd else None
        ok(capi.lib.dfot_op_dit_gelu(D(u), P(h), P(d), n, stream()))
        return tuple(t for t in (h, d) if t is not None)
    (h_only,) = twice(lambda: run(True, False))
    (du_only,) = twice(lambda: run(False, True))
    h_both, du_both = twice(lambda: run(True, True))
    assert torch.equal(bits(h_only), bits(h_both)) and torch.equal(bits(du_only), bits(du_both))
    bc.assert_bf16_of_fp32(f"gelu n {n} h", h_both.cpu(), h64, 8 * bc.errors(h32, h64)[0])
    bc.assert_bf16_of_fp32(f"gelu n {n} du", du_both.cpu(), du64, 8 * bc.errors(du32, du64)[0])
    print(f"gelu n {n}: h max-abs {bc.errors(h_both.cpu(), h64)[0]:.3e}, du max-abs {bc.errors(du_both.cpu(), du64)[0]:.3e}")


# ---- patch embedding: forward, data gradient, weight gradient ----------------------------------------------------------------
# (channels, patch, hidden): nsub 2 / kdim 4; nsub 4 / kdim 16; nsub 1 with hidden < 256 / kdim 12; kdim 128, hidden > 256 with a half-live
# last block; the K600 shape; kdim 256, the largest
PE_SHAPES = [(4, 1, 128), (4, 2, 64), (3, 2, 192), (32, 2, 384), (16, 1, 1152), (64, 2, 128)]
GH, GW = 2, 4  # patch grid of a frame: 13 frames = 104 rows (one whole 64-row chunk and a ragged one), 16 frames = 128 rows


@functools.lru_cache(maxsize=None)
def pe_case(c, patch, hidden, frames):
    g = gen("pe", c, patch, hidden, frames)
    kdim, rows = c * patch * patch, frames * GH * GW
    x = data(g, frames, c, GH * patch, GW * patch)
    w = torch.randn(hidden, kdim, generator=g) / kdim ** 0.5
    b, pos = 0.1 * torch.randn(hidden, generator=g), torch.randn(GH * GW, hidden, generator=g)
    dy = data(g, rows, hidden)
    dw0, db0 = sentinel(hidden, kdim), sentinel(hidden)  # what the weight gradient accumulates onto
    return x, w, b, pos, dy, dw0, db0


def run_pe(c, patch, hidden, frames):
    """the three ops on one set of inputs: out (with pos), out (without), dx, dW, db"""
    from dfot_amd import capi
    x, w, b, pos, dy, dw0, db0 = pe_case(c, patch, hidden, frames)
    rows, hh, ww = frames * GH * GW, GH * patch, GW * patch
    xd, wd, dyd = x.cuda(), w.cuda(), dy.cuda()
    out, out_nopos, dx = nan(rows, hidden), nan(rows, hidden), nan(*x.shape)
    dw, db = dw0.cuda(), db0.cuda()
    ok(capi.lib.dfot_op_dit_patch_embed(P(xd), P(wd), D(b), D(pos), P(out), c, hh, ww, patch, hidden, rows, stream()))
    ok(capi.lib.dfot_op_dit_patch_embed(P(xd), P(wd), D(b), P(None), P(out_nopos), c, hh, ww, patch, hidden, rows, stream()))
    ok(capi.lib.dfot_op_dit_patch_embed_dgrad(P(dyd), P(wd), P(dx), c, hh, ww, patch, hidden, rows, stream()))
    ok(capi.lib.dfot_op_dit_patch_embed_wgrad(P(dyd), P(xd), P(dw), P(db), c, hh, ww, patch, hidden, rows, stream()))
    return out, out_nopos, dx, dw, db


@pytest.mark.parametrize("frames", [13, 16])
@pytest.mark.parametrize("c,patch,hidden", PE_SHAPES)
def test_patch_embed_and_its_gradients(c, patch, hidden, frames):
    x, w, b, pos, dy, dw0, db0 = (t.double() for t in pe_case(c, patch, hidden, frames))
    out, out_nopos, dx, dw, db = (t.cpu() for t in twice(lambda: run_pe(c, patch, hidden, frames)))
    name = f"c {c} patch {patch} hidden {hidden} rows {frames * GH * GW}"
    kdim, rows = c * patch * patch, frames * GH * GW
    f2 = bc.F32_ULP
    # forward: kdim products onto the bias, then the positional embedding
    pat = bc.patchify(x, patch)
    absprod = pat.abs() @ w.abs().t()
    b_out = absprod + b.abs() + pos.abs().repeat(frames, 1)
    bc.assert_sum_bound(f"patch_embed {name}", out, bc.patch_embed(x, w, b, patch, pos), b_out, kdim + 1)
    bc.assert_sum_bound(f"patch_embed {name} (no pos)", out_nopos, bc.patch_embed(x, w, b, patch), absprod + b.abs(), kdim + 1)
    # gradients by autograd on the float64 forward
    xx, wv, bv = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    rdx, rdw, rdb = torch.autograd.grad(bc.patch_embed(xx, wv, bv, patch, pos), (xx, wv, bv), dy)
    # |terms| of the data gradient: the same scatter applied to |dy| |w| (autograd of the forward on magnitudes)
    xa = x.clone().requires_grad_()
    (b_dx,) = torch.autograd.grad(bc.patchify(xa, patch), xa, dy.abs() @ w.abs())
    bc.assert_sum_bound(f"patch_embed_dgrad {name}", dx, rdx, b_dx, hidden)
    b_dw = dy.abs().t() @ pat.abs() + dw0.abs()
    b_db = dy.abs().sum(0) + db0.abs()
    bc.assert_sum_bound(f"patch_embed_wgrad {name} dW", dw, dw0 + rdw, b_dw, rows + 1)
    bc.assert_sum_bound(f"patch_embed_wgrad {name} db", db, db0 + rdb, b_db, rows + 1)
    # the three ops against each other, in float64 from the kernels' outputs; tolerances from the bounds above
    out, dx, dw = out.double(), dx.double(), dw.double() - dw0
    t_out, t_dx, t_dw = (kdim + 5) * f2 * b_out, (hidden + 4) * f2 * b_dx, (rows + 5) * f2 * b_dw
    lhs, rhs = (out * dy).sum(), (x * dx).sum() + (dy * (b + pos.repeat(frames, 1))).sum()
    assert abs(float(lhs - rhs)) <= float((dy.abs() * t_out).sum() + (x.abs() * t_dx).sum()), (name, float(lhs), float(rhs))
    lhs, rhs = (dw * w).sum(), (dy * (out - b - pos.repeat(frames, 1))).sum()
    assert abs(float(lhs - rhs)) <= float((w.abs() * t_dw).sum() + (dy.abs() * t_out).sum()), (name, float(lhs), float(rhs))


@pytest.mark.parametrize("rows,chunks", [(131072 + 8, 4), (524288 + 8, 16)])
def test_patch_embed_wgrad_long_inputs(rows, chunks):
    """(4, 1, 64): at least 64 * 4 * 512 and 64 * 16 * 512 rows make a workgroup keep its sums in registers over 4 and 16 chunks of 64 rows;
    8 more rows leave the last workgroup a ragged chunk.  Inputs are drawn on the device and so is their float64 reference."""
    from dfot_amd import capi
    c, patch, hidden = 4, 1, 64
    assert (4 if rows >= 64 * 4 * 512 else 1) * (4 if rows >= 64 * 16 * 512 else 1) == chunks
    frames = rows // (GH * GW)
    g = torch.Generator(device="cuda").manual_seed(rows)
    x = 1.5 * torch.randn(frames, c, GH, GW, generator=g, device="cuda") + 0.3
    dy = 1.5 * torch.randn(rows, hidden, generator=g, device="cuda") + 0.3
    dw0, db0 = sentinel(hidden, c).cuda(), sentinel(hidden).cuda()

    def run():
        dw, db = dw0.clone(), db0.clone()
        ok(capi.lib.dfot_op_dit_patch_embed_wgrad(P(dy), P(x), P(dw), P(db), c, GH, GW, patch, hidden, rows, stream()))
        return dw, db
    dw, db = twice(run)
    pat, dyd = bc.patchify(x.double(), patch), dy.double()
    rdw, b_dw = dw0.double() + dyd.t() @ pat, dw0.double().abs() + dyd.abs().t() @ pat.abs()
    rdb, b_db = db0.double() + dyd.sum(0), db0.double().abs() + dyd.abs().sum(0)
    bc.assert_sum_bound(f"patch_embed_wgrad rows {rows} (chunks {chunks}) dW", dw.cpu(), rdw.cpu(), b_dw.cpu(), rows + 1)
    bc.assert_sum_bound(f"patch_embed_wgrad rows {rows} (chunks {chunks}) db", db.cpu(), rdb.cpu(), b_db.cpu(), rows + 1)
    # With N = every addition the bound is loose at this length (rows 2^-24 ~ 3e-2 of sum |terms|): it would pass a dropped 64-row chunk
    # (1.2e-4 of the rows).  The sum as launched is blocked, and a blocked sum's error grows with the additions one term passes through,
    # not with all of them: 64 * chunks / nsub rows per thread (nsub = 256 / hidden = 4 thread groups take alternate rows), then
    # ceil(partial rows / 16) per row group of the fixed-order reduction, its four-level tree and the accumulation onto dW.
    ny = -(-rows // (64 * chunks))
    depth = 64 * chunks // 4 + -(-ny * 4 // 16) + 4 + 1
    # (198 and 390 additions: 1.2e-5 and 2.3e-5 of sum |terms|, where a dropped chunk is 4.9e-4 and 1.2e-4 of the rows)
    assert depth in (198, 390)
    bc.assert_sum_bound(f"patch_embed_wgrad rows {rows} (chunks {chunks}) dW, blocked", dw.cpu(), rdw.cpu(), b_dw.cpu(), depth)
    bc.assert_sum_bound(f"patch_embed_wgrad rows {rows} (chunks {chunks}) db, blocked", db.cpu(), rdb.cpu(), b_db.cpu(), depth)


# ---- final gather ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,patch", [(4, 1), (3, 2), (32, 2), (64, 2)])
def test_final_gather(c, patch):
    from dfot_amd import capi
    frames = 13
    rows, oc, hh, ww = frames * GH * GW, c * patch * patch, GH * patch, GW * patch
    ocp = (oc + 63) // 64 * 64
    dout = data(gen("gather", c, patch), frames, c, hh, ww)

    def run():
        dyp = torch.zeros(rows, ocp, dtype=torch.bfloat16, device="cuda")
        dyt = torch.zeros(256, rows, dtype=torch.bfloat16, device="cuda")  # the trainer's buffer: 256 rows whatever oc is
        ok(capi.lib.dfot_op_dit_final_gather(D(dout), P(dyp), P(dyt), rows, c, hh, ww, patch, ocp, stream()))
        return dyp, dyt
    dyp, dyt = (t.cpu() for t in twice(run))
    y = torch.zeros(rows, oc, dtype=torch.float64, requires_grad=True)
    (gathered,) = torch.autograd.grad(bc.unpatchify(y, c, hh, ww, patch), y, dout.double())  # the transpose of unpatchify: a permutation
    want = gathered.float().bfloat16()
    assert torch.equal(bits(dyp[:, :oc]), bits(want)) and torch.equal(bits(dyt[:oc]), bits(want.t().contiguous()))
    assert not bool(dyp[:, oc:].any()) and not bool(dyt[oc:].any())  # the padding stays as the caller left it


# ---- qkv gradient pack -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,d", [(2, 64), (16, 72), (12, 32)])
def test_qkv_grad_pack(heads, d):
    from dfot_amd import capi
    ntok, batch = 40, 3
    dstride = 64 if d <= 64 else 128  # attention_dstride
    assert (heads, d, dstride) in ((2, 64, 64), (16, 72, 128), (12, 32, 64))
    rows = batch * ntok
    g = gen("pack", heads, d)
    dq, dk, dv = (data(g, batch, heads, ntok, dstride).bfloat16() for _ in range(3))  # the padding past d is not zero: it must not be read
    theta = 6.0 * torch.rand(ntok, d // 2, generator=g, dtype=torch.float64)  # random angle per (token, pair)
    cs = torch.stack((theta.cos(), theta.sin()), -1).float()

    def run(rope):
        out = nan(rows, 3 * heads * d, dtype=torch.bfloat16)
        ok(capi.lib.dfot_op_dit_qkv_grad_pack(D(dq), D(dk), D(dv), D(cs) if rope else P(None), P(out), rows, ntok, heads,
                                              d, dstride, stream()))
        return (out,)
    (plain,) = twice(lambda: run(False))
    assert torch.equal(bits(plain.cpu()), bits(bc.qkv_pack(dq, dk, dv, d)))  # without the rotation: a gather
    (rot,) = twice(lambda: run(True))
    rot = rot.cpu()
    hd = heads * d
    assert torch.equal(bits(rot[:, 2 * hd:]), bits(plain.cpu()[:, 2 * hd:]))  # v is never rotated
    # reference: autograd of the float64 forward rotation with the table's own (fp32) cos / sin
    refs = {}
    for dt in (torch.float64, torch.float32):
        co, si = cs[..., 0].to(dt), cs[..., 1].to(dt)
        grads = []
        for t in (dq, dk):
            xx = torch.zeros(batch, heads, ntok, d, dtype=dt, requires_grad=True)
            grads.append(torch.autograd.grad(bc.rope_rotate(xx, co, si), xx, t[..., :d].to(dt))[0])
        refs[dt] = bc.qkv_pack(grads[0], grads[1], dv.to(dt), d)[:, :2 * hd]
    slack = 8 * bc.errors(refs[torch.float32], refs[torch.float64])[0]
    bc.assert_bf16_of_fp32(f"qkv_grad_pack heads {heads} d {d} rotated", rot[:, :2 * hd], refs[torch.float64], slack)
    # adjoint identity against a float64 forward rotation of a random x: <rope(x), g> = <x, rope^T(g)>
    x = torch.randn(batch, heads, ntok, d, generator=g, dtype=torch.float64)
    fwd = bc.rope_rotate(x, cs[..., 0].double(), cs[..., 1].double())
    for which, src in enumerate((dq, dk)):
        packed = rot[:, which * hd:(which + 1) * hd].double().reshape(batch, ntok, heads, d).permute(0, 2, 1, 3)
        ref = refs[torch.float64][:, which * hd:(which + 1) * hd].reshape(batch, ntok, heads, d).permute(0, 2, 1, 3)
        lhs, rhs = (fwd * src[..., :d].double()).sum(), (x * packed).sum()
        assert abs(float(lhs - rhs)) <= float((x.abs() * (bc.BF16_HALF_ULP * ref.abs() + slack)).sum()) + 1e-9 * abs(float(lhs))
