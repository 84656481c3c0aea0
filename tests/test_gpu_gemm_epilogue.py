"""Op-level tests of every fused epilogue of the bf16 MFMA GEMM / implicit-GEMM launcher (csrc/gemm.hip) through
dfot_op_gemm_ex, against an fp64 host reference of the same bf16 operands.

Bars are elementwise:
  fp32 outputs  |got - ref| <= 1e-6 * mag + 1e-6 * |ref|, mag = the epilogue formula evaluated on absolute values
                (|A| @ |W|^T for a plain product; the MFMA is a k-ordered fp32 fma chain, ~1.5e-7 * sum|a*b| at K <= 1024)
  bf16 outputs  |got - bf16(ref)| <= n ulp(bf16(ref)) + the fp32 bar above carried through the epilogue's function,
                n = 1, or 2 after RMSNorm / RoPE / GELU
  GroupNorm partials agree with fp64 sums of the values as stored, to fp32 summation rounding.
Every output buffer starts as NaN: what the kernel must not write stays NaN, what it must write is finite.  Each
non-atomic case runs twice on the same stream and must give bit-identical outputs.  The worst error / bar ratio of each
epilogue family is printed at the end of the module (-s)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

E_F32, E_BF16, E_QKV, E_QKV_DIT = range(4)
A_DENSE, A_CONV3 = 0, 1
ALL = (0, 1, 4, 6, 8, 9, 10, 14, -1)        # every tile form, and the shape picker
NO_RING = (0, 1, 4, 6, 8, 9, 10, -1)        # GroupNorm partials, E_QKV and E_QKV_DIT: no 256x144 ring
CONV_F32 = (0, 1, 4, 6, 8, 14, -1)          # the 256x192 / 128x192 forms take dense A only
CONV_BF16 = (0, 1, 4, 6, 8, -1)
PERSISTENT = (0, 1, 9, 10, 14)              # forms of <= 12 waves without in-workgroup split-K: the persistent tile loop
NAN = float("nan")
WORST = {}


@pytest.fixture(scope="module")
def capi():
    import dfot_amd  # noqa: F401
    from dfot_amd import capi as c
    assert torch.cuda.is_available()
    return c


@pytest.fixture(scope="module", autouse=True)
def worst_ratio_table():
    yield
    print("\nworst elementwise error / bar per epilogue family:")
    for fam, (r, name) in sorted(WORST.items()):
        print(f"  {fam:14s} {r:.3f}  ({name})")


def rnd(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).bfloat16()


def nan_buf(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def desc(capi, **fields):
    """GemmDesc from keyword fields; tensors become their data pointers and are kept alive with the descriptor"""
    d = capi.GemmDesc()
    d.qscale, d.eps, d.ksplit, d.variant = 1.0, 1e-6, 1, -1
    d.keep = [v for v in fields.values() if isinstance(v, torch.Tensor)]
    for k, v in fields.items():
        setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return d


def call(capi, d):
    capi.check(capi.lib.dfot_op_gemm_ex(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def run(capi, d, outs, deterministic=True):
    """Runs the GEMM (twice unless it uses atomics), each time from the initial contents of `outs`; returns host copies"""
    init = [o.clone() for o in outs]
    res = []
    for _ in range(2 if deterministic else 1):
        for o, i in zip(outs, init):
            o.copy_(i)
        call(capi, d)
        res.append([o.cpu() for o in outs])
    if deterministic:
        for x, y in zip(*res):
            assert torch.equal(bits(x), bits(y)), "second run on the same stream differs"
    return res[0]


def ulp_bf16(x):
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


def check(fam, name, got, exp, bar, nulp=0):
    """got: host output buffer; exp: fp64 reference of the same shape, NaN where nothing may be written; bar: fp32 error bar
    (bf16 outputs: nulp > 0, the reference is rounded to bf16 first)"""
    got = got.double()
    w = ~torch.isnan(exp)
    assert torch.isnan(got[~w]).all(), f"{name}: {int((~torch.isnan(got[~w])).sum())} stores outside the output"
    assert torch.isfinite(got[w]).all(), f"{name}: {int((~torch.isfinite(got[w])).sum())} outputs missing or not finite"
    ref = exp[w]
    tol = bar[w].clamp_min(1e-30)  # (exact zeros: a conv K slice that sees padding only)
    if nulp:
        ref = ref.float().bfloat16().double()
        tol = tol + nulp * ulp_bf16(ref)
    ratio = ((got[w] - ref).abs() / tol).max().item()
    print(f"{name}: worst error / bar = {ratio:.3f}")
    if ratio > WORST.get(fam, (-1.0, ""))[0]:
        WORST[fam] = (ratio, name)
    assert ratio <= 1.0, name


def padded(x, rows, ld, col0=0):
    """fp64 [rows, ld] NaN buffer with x at columns [col0, col0 + x.shape[1])"""
    e = torch.full((rows, ld), NAN, dtype=torch.float64)
    e[:, col0:col0 + x.shape[1]] = x
    return e


def dense_operands(gen, m, n, k, apad=0, wpad=0):
    """A [m, k] and W [n, k] bf16, as column windows of wider buffers when apad / wpad > 0 (row strides lda = k + apad,
    ldw = k + wpad, the window starting at column apad / wpad): host copies, device views, row strides"""
    abuf = rnd(gen, m, k + apad)
    wbuf = rnd(gen, n, k + wpad, scale=1 / math.sqrt(k))
    a, w = abuf[:, apad:], wbuf[:, wpad:]
    da, dw = abuf.cuda(), wbuf.cuda()
    return a, w, da[:, apad:], dw[:, wpad:], k + apad, (k + wpad if wpad else 0)


def product(a, w):
    a, w = a.double(), w.double()
    return a @ w.t(), a.abs() @ w.abs().t()


def gelu(x):
    return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))


def silu(x):
    return x * torch.sigmoid(x)


def im2col(a, bt, h, w, cin):
    """NHWC image rows [bt*h*w, cin] -> [bt*h*w, 9*cin] fp64, tap-major ((dy, dx) row-major), zero padding"""
    x = F.pad(a.double().view(bt, h, w, cin), (0, 0, 1, 1, 1, 1))
    cols = [x[:, dy:dy + h, dx:dx + w, :] for dy in range(3) for dx in range(3)]
    return torch.cat(cols, -1).reshape(bt * h * w, 9 * cin)


def gn_check(fam, name, part, out, n_img, rows_per_bt, cpg, live=None):
    """gn_part[img][slot][group][sum, sumsq] against fp64 sums over 64-row slots of the values as stored"""
    slots = rows_per_bt // 64
    v = out.double().view(n_img, slots, 64, 32, cpg)
    s, s2 = v.sum((2, 4)), (v * v).sum((2, 4))
    mag = v.abs().sum((2, 4))
    exp = torch.stack([s, s2], -1)
    bar = 4e-6 * torch.stack([mag, s2], -1)
    if live is not None:
        exp[~live.bool()] = NAN
    check(fam, name, part.view(n_img, slots, 32, 2), exp, bar)


# ---------------------------------------------------------------------------------------------------- plain fp32 / bf16

PLAIN = {  # name: M, N, K, extra output columns (ldo - N), lda - K, ldw - K, bias
    "n100": (512, 100, 128, 0, 0, 0, True),
    "n264_strided": (1024, 264, 192, 24, 64, 128, True),
    "n4032_nobias": (512, 4032, 128, 0, 0, 0, False),
    "persistent": (8192, 1736, 64, 8, 0, 0, True),  # more tiles than resident workgroups: 896 .. 320 of them
}


@pytest.mark.parametrize("epi", [E_F32, E_BF16])
@pytest.mark.parametrize("case,variant", [(c, v) for c in PLAIN for v in (PERSISTENT if c == "persistent" else ALL)])
def test_plain(capi, case, epi, variant):
    m, n, k, opad, apad, wpad, has_bias = PLAIN[case]
    if epi == E_BF16 and n % 8:
        n += 4
    gen = torch.Generator().manual_seed(10 * list(PLAIN).index(case) + epi)
    a, w, da, dw, lda, ldw = dense_operands(gen, m, n, k, apad, wpad)
    bias = torch.randn(n, generator=gen) if has_bias else None
    ldo = n + opad
    out = nan_buf(m, ldo, dtype=torch.float32 if epi == E_F32 else torch.bfloat16)
    d = desc(capi, amode=A_DENSE, epi=epi, variant=variant, A=da, lda=lda, W=dw, ldw=ldw, M=m, N=n, K=k,
             bias=bias.cuda() if has_bias else 0, ldo=ldo, **({"out_f32": out} if epi == E_F32 else {"out_bf16": out}))
    got, = run(capi, d, [out])
    acc, mag = product(a, w)
    if has_bias:
        acc, mag = acc + bias.double(), mag + bias.double().abs()
    bar = padded(1e-6 * mag + 1e-6 * acc.abs(), m, ldo)
    check("plain_" + ("f32" if epi == E_F32 else "bf16"), f"plain {case} epi={epi} v={variant}", got, padded(acc, m, ldo), bar,
          nulp=0 if epi == E_F32 else 1)


@pytest.mark.parametrize("variant", ALL)
def test_f32_residual_out_of_place(capi, variant):
    m, n, k, ldo = 1024, 264, 192, 272
    gen = torch.Generator().manual_seed(11)
    a, w, da, dw, lda, ldw = dense_operands(gen, m, n, k)
    bias = torch.randn(n, generator=gen)
    resid = torch.randn(m, ldo, generator=gen) * 4
    out = nan_buf(m, ldo)
    d = desc(capi, amode=A_DENSE, epi=E_F32, variant=variant, A=da, lda=lda, W=dw, M=m, N=n, K=k, bias=bias.cuda(),
             out_f32=out, ldo=ldo, resid=resid.cuda())
    got, = run(capi, d, [out])
    acc, mag = product(a, w)
    r = resid[:, :n].double()
    ref = acc + bias.double() + r
    check("resid_f32", f"resid f32 v={variant}", got, padded(ref, m, ldo),
          padded(1e-6 * (mag + bias.double().abs() + r.abs()) + 1e-6 * ref.abs(), m, ldo))


# conv ResBlock stream (any conv tile form) and the level-2 out-projection (dense, 256x144 ring only)
BF16_RESID = [(A_CONV3, v) for v in CONV_BF16] + [(A_DENSE, 14)]


@pytest.mark.parametrize("amode,variant", BF16_RESID)
@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("act", [0, 2])
def test_bf16_residual(capi, amode, variant, inplace, act):
    gen = torch.Generator().manual_seed(12 + act)
    if amode == A_CONV3:
        bt, h, wd, cin, n = 16, 12, 8, 64, 128  # 96-pixel images: tiles straddle images
        m, k, ldo = bt * h * wd, 9 * cin, n
        a = rnd(gen, m, cin)
        w = rnd(gen, n, k, scale=1 / math.sqrt(k))
        geo = dict(amode=A_CONV3, A=a.cuda(), W=w.cuda(), M=m, N=n, K=k, H=h, Wd=wd, Cin=cin)
        cols = im2col(a, bt, h, wd, cin)
    else:
        m, n, k, ldo = 512, 576, 256, 584
        a, w, da, dw, lda, ldw = dense_operands(gen, m, n, k)
        geo = dict(amode=A_DENSE, A=da, lda=lda, W=dw, M=m, N=n, K=k)
        cols = a.double()
    bias = torch.randn(n, generator=gen)
    res = torch.full((m, ldo), NAN).bfloat16()
    res[:, :n] = rnd(gen, m, n, scale=3)
    out = res.cuda() if inplace else nan_buf(m, ldo, dtype=torch.bfloat16)
    rdev = out if inplace else res.cuda()
    d = desc(capi, epi=E_BF16, variant=variant, bias=bias.cuda(), out_bf16=out, ldo=ldo, resid_bf=rdev, act=act, **geo)
    got, = run(capi, d, [out])
    acc = cols @ w.double().t() + bias.double()
    mag = cols.abs() @ w.double().abs().t() + bias.double().abs()
    r = res[:, :n].double()
    ref = (silu(acc) if act == 2 else acc) + r
    bar = 1e-6 * (1.2 * mag + r.abs()) + 1e-6 * ref.abs()
    check("resid_bf16", f"resid_bf amode={amode} v={variant} inplace={inplace} act={act}", got, padded(ref, m, ldo),
          padded(bar, m, ldo), nulp=1)
    if not inplace:
        assert torch.equal(bits(rdev.cpu()), bits(res)), "out-of-place residual was modified"


@pytest.mark.parametrize("variant", ALL)
@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("pre_act", [False, True])
def test_activation(capi, variant, act, pre_act):
    m, n, k, ldo = 512, 264, 128, 280
    gen = torch.Generator().manual_seed(13)
    a, w, da, dw, lda, ldw = dense_operands(gen, m, n, k)
    bias = torch.randn(n, generator=gen)
    bias[::7] = 60.0  # pre-activations beyond +-40: the exp of the GELU / SiLU saturates
    bias[3::7] = -60.0
    out = nan_buf(m, ldo, dtype=torch.bfloat16)
    pre = nan_buf(m, ldo, dtype=torch.bfloat16)
    d = desc(capi, amode=A_DENSE, epi=E_BF16, variant=variant, A=da, lda=lda, W=dw, M=m, N=n, K=k, bias=bias.cuda(),
             out_bf16=out, ldo=ldo, act=act, pre_act=pre if pre_act else 0)
    got, got_pre = run(capi, d, [out, pre])
    acc, mag = product(a, w)
    acc, mag = acc + bias.double(), mag + bias.double().abs()
    ref = gelu(acc) if act == 1 else silu(acc)
    bar = 1.2e-6 * mag + 1e-6 * ref.abs()
    check("act", f"act={act} pre_act={pre_act} v={variant}", got, padded(ref, m, ldo), padded(bar, m, ldo), nulp=2)
    if pre_act:
        check("act", f"pre_act act={act} v={variant}", got_pre, padded(acc, m, ldo), padded(1e-6 * mag, m, ldo), nulp=1)
    else:
        assert torch.isnan(got_pre.float()).all()


@pytest.mark.parametrize("variant", ALL)
@pytest.mark.parametrize("epi", [E_F32, E_BF16])
@pytest.mark.parametrize("bias_rows", [96, -128])
def test_bias_rows(capi, variant, epi, bias_rows):
    m, n, k, ldo = 1024, 136, 128, 144
    gen = torch.Generator().manual_seed(14)
    a, w, da, dw, lda, ldw = dense_operands(gen, m, n, k)
    nb = bias_rows if bias_rows > 0 else m // -bias_rows
    bias = torch.randn(nb, n, generator=gen)
    rows = torch.arange(m)
    brow = rows % bias_rows if bias_rows > 0 else rows // -bias_rows
    out = nan_buf(m, ldo, dtype=torch.float32 if epi == E_F32 else torch.bfloat16)
    d = desc(capi, amode=A_DENSE, epi=epi, variant=variant, A=da, lda=lda, W=dw, M=m, N=n, K=k, bias=bias.cuda(),
             bias_rows=bias_rows, ldo=ldo, **({"out_f32": out} if epi == E_F32 else {"out_bf16": out}))
    got, = run(capi, d, [out])
    acc, mag = product(a, w)
    b = bias.double()[brow]
    ref, mag = acc + b, mag + b.abs()
    check("bias_rows", f"bias_rows={bias_rows} epi={epi} v={variant}", got, padded(ref, m, ldo),
          padded(1e-6 * mag + 1e-6 * ref.abs(), m, ldo), nulp=0 if epi == E_F32 else 1)


@pytest.mark.parametrize("variant", ALL)
@pytest.mark.parametrize("gate_rows", [48, 24])  # 16 k: one gate row per 16-row pass; else per row
@pytest.mark.parametrize("indexed", [False, True])
def test_gate(capi, variant, gate_rows, indexed):
    m, n, k, ldo, ldg = 1536, 264, 192, 264, 280
    gen = torch.Generator().manual_seed(15)
    a, w, da, dw, lda, ldw = dense_operands(gen, m, n, k)
    bias = torch.randn(n, generator=gen)
    resid = torch.randn(m, ldo, generator=gen)
    frames = m // gate_rows
    table = 7 if indexed else frames
    gate = torch.randn(table, ldg, generator=gen)
    index = torch.randint(0, table, (frames,), generator=gen, dtype=torch.int32)
    out = nan_buf(m, ldo)
    d = desc(capi, amode=A_DENSE, epi=E_F32, variant=variant, A=da, lda=lda, W=dw, M=m, N=n, K=k, bias=bias.cuda(),
             out_f32=out, ldo=ldo, resid=resid.cuda(), gate=gate.cuda(), ldg=ldg, gate_rows=gate_rows,
             gate_index=index.cuda() if indexed else 0)
    got, = run(capi, d, [out])
    acc, mag = product(a, w)
    frame = torch.arange(m) // gate_rows
    g = gate.double()[index.long()[frame] if indexed else frame][:, :n]
    r = resid.double()
    ref = r + g * (acc + bias.double())
    bar = 1e-6 * (g.abs() * (mag + bias.double().abs()) + r.abs()) + 1e-6 * ref.abs()
    check("gate", f"gate rows={gate_rows} indexed={indexed} v={variant}", got, ref, bar)


@pytest.mark.parametrize("variant", ALL)
def test_transposed_store(capi, variant):
    m, n, k, tr = 1536, 200, 128, 96  # 16 frames of 96 rows
    gen = torch.Generator().manual_seed(16)
    a, w, da, dw, lda, ldw = dense_operands(gen, m, n, k)
    out = nan_buf(m * n + 64, dtype=torch.bfloat16)  # + a tail that must stay untouched
    d = desc(capi, amode=A_DENSE, epi=E_BF16, variant=variant, A=da, lda=lda, W=dw, M=m, N=n, K=k, out_bf16=out, ldo=n,
             tr_rows=tr)
    got, = run(capi, d, [out])
    acc, mag = product(a, w)
    t = lambda x: x.view(m // tr, tr, n).transpose(1, 2).reshape(-1)  # noqa: E731  out[frame][col][row % tr]
    exp = torch.cat([t(acc), torch.full((64,), NAN, dtype=torch.float64)])
    bar = torch.cat([t(1e-6 * mag + 1e-6 * acc.abs()), torch.zeros(64, dtype=torch.float64)])
    check("tr_rows", f"tr_rows={tr} v={variant}", got, exp, bar, nulp=1)


@pytest.mark.parametrize("variant", NO_RING)
@pytest.mark.parametrize("epi", [E_F32, E_BF16])
@pytest.mark.parametrize("cpg", [4, 8])
def test_groupnorm_partials_dense(capi, variant, epi, cpg):
    m, k, rows_bt = 1536, 192, 512
    n = 32 * cpg
    gen = torch.Generator().manual_seed(17 + cpg)
    a, w, da, dw, lda, ldw = dense_operands(gen, m, n, k)
    bias = torch.randn(n, generator=gen) + 0.5  # a nonzero mean: statistics of unrounded values would drift from the stored ones
    part = nan_buf(m // 64 * 64)
    out = nan_buf(m, n, dtype=torch.float32 if epi == E_F32 else torch.bfloat16)
    d = desc(capi, amode=A_DENSE, epi=epi, variant=variant, A=da, lda=lda, W=dw, M=m, N=n, K=k, bias=bias.cuda(), ldo=n,
             gn_part=part, gn_rows_per_bt=rows_bt, gn_cpg=cpg, **({"out_f32": out} if epi == E_F32 else {"out_bf16": out}))
    got, got_part = run(capi, d, [out, part])
    acc, mag = product(a, w)
    ref, mag = acc + bias.double(), mag + bias.double().abs()
    fam = "gn_" + ("f32" if epi == E_F32 else "bf16")
    check(fam, f"gn out epi={epi} cpg={cpg} v={variant}", got, ref, 1e-6 * mag + 1e-6 * ref.abs(), nulp=0 if epi == E_F32 else 1)
    gn_check(fam, f"gn stats epi={epi} cpg={cpg} v={variant}", got_part, got, m // rows_bt, rows_bt, cpg)


@pytest.mark.parametrize("epi,variant", [(E_F32, v) for v in CONV_F32] + [(E_BF16, v) for v in CONV_BF16])
@pytest.mark.parametrize("cpg", [0, 4, 8])
def test_conv_live_images(capi, epi, variant, cpg):
    """Conv with per-image live flags (image 1 of 3 dead: no stores, no statistics); 16x32 images = whole tiles of every height"""
    if cpg and variant == 14:
        pytest.skip("the 256x144 ring has no GroupNorm partials (refused)")
    bt, h, wd, cin = 3, 16, 32, 64
    n = 32 * cpg if cpg else 192
    m, k = bt * h * wd, 9 * cin
    gen = torch.Generator().manual_seed(18 + cpg)
    a = rnd(gen, m, cin)
    w = rnd(gen, n, k, scale=1 / math.sqrt(k))
    bias = torch.randn(n, generator=gen) + 0.5
    live = torch.tensor([1, 0, 1], dtype=torch.uint8)
    out = nan_buf(m, n, dtype=torch.float32 if epi == E_F32 else torch.bfloat16)
    part = nan_buf(m // 64 * 64)
    d = desc(capi, amode=A_CONV3, epi=epi, variant=variant, A=a.cuda(), W=w.cuda(), M=m, N=n, K=k, H=h, Wd=wd, Cin=cin,
             live=live.cuda(), bias=bias.cuda(), ldo=n, gn_part=part if cpg else 0, gn_rows_per_bt=h * wd if cpg else 0,
             gn_cpg=cpg, **({"out_f32": out} if epi == E_F32 else {"out_bf16": out}))
    got, got_part = run(capi, d, [out, part])
    cols = im2col(a, bt, h, wd, cin)
    ref = cols @ w.double().t() + bias.double()
    mag = cols.abs() @ w.double().abs().t() + bias.double().abs()
    dead = live.bool().logical_not().repeat_interleave(h * wd)
    ref[dead] = NAN
    fam = "conv_" + ("f32" if epi == E_F32 else "bf16")
    check(fam, f"conv live epi={epi} cpg={cpg} v={variant}", got, ref, 1e-6 * mag + 1e-6 * ref.abs().nan_to_num(),
          nulp=0 if epi == E_F32 else 1)
    if cpg:
        gn_check(fam, f"conv gn stats epi={epi} cpg={cpg} v={variant}", got_part, got.nan_to_num(), bt, h * wd, cpg, live)
    else:
        assert torch.isnan(got_part).all()


# ---------------------------------------------------------------------------------------------------- split-K

def k_slices(nk, s):
    """the per / rem split of gemm_tile: slice i takes k-tiles [kb, kb + n)"""
    per, rem = divmod(nk, s)
    return [(i * per + min(i, rem), per + (1 if i < rem else 0)) for i in range(s)]


@pytest.mark.parametrize("amode,ksplit,variant", [(A_DENSE, s, v) for s in (2, 3) for v in ALL] +
                         [(A_CONV3, s, v) for s in (2, 4) for v in CONV_F32])
def test_split_k_slices(capi, amode, ksplit, variant):
    gen = torch.Generator().manual_seed(19 + ksplit)
    if amode == A_DENSE:
        m, n, k, ldo = 512, 264, 448, 264  # 7 k-tiles
        a, w, da, dw, lda, ldw = dense_operands(gen, m, n, k)
        geo = dict(amode=A_DENSE, A=da, lda=lda, W=dw, M=m, N=n, K=k)
        cols = a.double()
    else:
        bt, h, wd, cin, n = 16, 12, 8, 64, 128  # K = 576: 9 k-tiles
        m, k, ldo = bt * h * wd, 9 * cin, 136
        a = rnd(gen, m, cin)
        w = rnd(gen, n, k, scale=1 / math.sqrt(k))
        geo = dict(amode=A_CONV3, A=a.cuda(), W=w.cuda(), M=m, N=n, K=k, H=h, Wd=wd, Cin=cin)
        cols = im2col(a, bt, h, wd, cin)
    stride = m * ldo + 32
    out = nan_buf(ksplit * stride)
    d = desc(capi, epi=E_F32, variant=variant, out_f32=out, ldo=ldo, ksplit=ksplit, slice_stride=stride, **geo)
    got, = run(capi, d, [out])
    w64 = w.double()
    total = torch.zeros(m, n, dtype=torch.float64)
    total_mag = torch.zeros(m, n, dtype=torch.float64)
    for s, (kb, nt) in enumerate(k_slices(k // 64, ksplit)):
        ks = slice(kb * 64, (kb + nt) * 64)
        ref = cols[:, ks] @ w64[:, ks].t()
        mag = cols[:, ks].abs() @ w64[:, ks].abs().t()
        total, total_mag = total + ref, total_mag + mag
        exp = torch.full((stride,), NAN, dtype=torch.float64)
        exp[:m * ldo] = padded(ref, m, ldo).reshape(-1)
        bar = torch.zeros(stride, dtype=torch.float64)
        bar[:m * ldo] = padded(1e-6 * mag + 1e-6 * ref.abs(), m, ldo).reshape(-1)
        check("split_k", f"split-K slice {s}/{ksplit} amode={amode} v={variant}", got[s * stride:(s + 1) * stride], exp, bar)
    full = cols @ w64.t()
    sum_slices = got.double().view(ksplit, stride)[:, :m * ldo].reshape(ksplit, m, ldo)[:, :, :n].sum(0)
    check("split_k", f"split-K sum of slices amode={amode} v={variant}", sum_slices, full,
          1e-6 * total_mag + 1e-6 * full.abs())


@pytest.mark.parametrize("variant", ALL)
@pytest.mark.parametrize("ksplit", [2, 3])
def test_split_k_atomics_inplace_residual(capi, variant, ksplit):
    m, n, k, ldo = 512, 264, 448, 272
    gen = torch.Generator().manual_seed(21)
    a, w, da, dw, lda, ldw = dense_operands(gen, m, n, k)
    bias = torch.randn(n, generator=gen)
    init = torch.full((m, ldo), NAN)
    init[:, :n] = torch.randn(m, n, generator=gen) * 4
    out = init.cuda()
    d = desc(capi, amode=A_DENSE, epi=E_F32, variant=variant, A=da, lda=lda, W=dw, M=m, N=n, K=k, bias=bias.cuda(),
             out_f32=out, ldo=ldo, resid=out, ksplit=ksplit)
    got, = run(capi, d, [out], deterministic=False)  # atomics: the slice order is not fixed
    acc, mag = product(a, w)
    r = init[:, :n].double()
    ref = r + acc + bias.double()
    check("split_k_atomic", f"split-K atomics ksplit={ksplit} v={variant}", got, padded(ref, m, ldo),
          padded(1e-6 * (mag + bias.double().abs() + r.abs()) + 1e-6 * ref.abs(), m, ldo))


# ---------------------------------------------------------------------------------------------------- fused q|k|v epilogues

def rope_table(gen, ntok, d):
    ang = torch.rand(ntok, d // 2, generator=gen) * 2 * math.pi
    return torch.stack([ang.cos(), ang.sin()], -1).contiguous()  # [ntok][d/2][cos, sin]


def rope(x, cs):
    """interleaved pairs (x0, x1) -> (x0 cos - x1 sin, x1 cos + x0 sin) (rotate_half of rotary_embedding_torch); also the bar:
    |c| + |s| times the larger error of the pair"""
    c, s = cs[..., 0].double(), cs[..., 1].double()
    x0, x1 = x[..., 0::2], x[..., 1::2]
    return torch.stack([x0 * c - x1 * s, x1 * c + x0 * s], -1).flatten(-2), (c.abs() + s.abs())


def heads_view(x, b, ntok, heads, d):
    return x.reshape(b, ntok, heads, d).permute(0, 2, 1, 3)


# ntok 384: at least the tile height but no multiple of it (a 256-row tile straddles two batch elements); 96: below it (a tile
# covers several); mlp_raw: MLP half into out2 at a column offset + raw copy; qkv_only: N == split, no out2 / raw
QKV_CASES = [(64, 384, "mlp_raw"), (64, 96, "qkv_only"), (128, 384, "qkv_only"), (128, 96, "mlp_raw")]


@pytest.mark.parametrize("variant", NO_RING)
@pytest.mark.parametrize("d,ntok,form", QKV_CASES)
def test_qkv(capi, variant, d, ntok, form, m=0, k=128):
    m = m or (1536 if variant == 6 else 768)  # whole 512-row tiles and whole batch elements
    heads = 9
    c = heads * d                       # 576 / 1152 as in the model
    split = 3 * c
    n = 7 * c if form == "mlp_raw" else split
    b = m // ntok
    gen = torch.Generator().manual_seed(22 + d + ntok)
    a, w, da, dw, lda, ldw = dense_operands(gen, m, n, k)
    bias = torch.randn(n, generator=gen) * 0.5
    qw, kw = torch.rand(d, generator=gen) + 0.5, torch.rand(d, generator=gen) + 0.5
    qw[5], kw[d - 3] = 40.0, -25.0       # large norm weights
    cs = rope_table(gen, ntok, d)
    qscale = 0.125
    q, kk, v = (nan_buf(b, heads, ntok, d, dtype=torch.bfloat16) for _ in range(3))
    off2, ld2 = 64, 5 * c + 64           # out2 at a column offset of a wider buffer (the attention output sits in front of it)
    out2 = nan_buf(m, ld2, dtype=torch.bfloat16)
    ldraw = n + 16
    raw = nan_buf(m, ldraw, dtype=torch.bfloat16)
    mlp = form == "mlp_raw"
    dsc = desc(capi, amode=A_DENSE, epi=E_QKV, variant=variant, A=da, lda=lda, W=dw, M=m, N=n, K=k, bias=bias.cuda(),
               out2=out2[:, off2:] if mlp else 0, ldo2=ld2 if mlp else 0, split=split, q=q, k=kk, v=v,
               qw=qw.cuda(), kw=kw.cuda(), rope_cs=cs.cuda(), heads=heads, d=d, ntok=ntok, qscale=qscale,
               raw=raw if mlp else 0, ldraw=ldraw if mlp else 0)
    gq, gk, gv, g2, graw = run(capi, dsc, [q, kk, v, out2, raw])
    acc, mag = product(a, w)
    x, e = acc + bias.double(), 1e-6 * (mag + bias.double().abs())
    tag = f"qkv d={d} ntok={ntok} {form} v={variant}"
    for i, (got, wgt, mul) in enumerate([(gq, qw, qscale), (gk, kw, 1.0)]):
        xs = heads_view(x[:, i * c:(i + 1) * c], b, ntok, heads, d)
        es = heads_view(e[:, i * c:(i + 1) * c], b, ntok, heads, d)
        r = (xs.pow(2).mean(-1, keepdim=True) + 1e-6).sqrt()
        wd = wgt.double()
        y = xs / r * wd
        ey = wd.abs() / r * (es + xs.abs() * (xs.abs() * es).mean(-1, keepdim=True) / r ** 2)
        z, amp = rope(y, cs)
        ez = torch.maximum(ey[..., 0::2], ey[..., 1::2]) * amp
        ez = torch.stack([ez, ez], -1).flatten(-2)
        check("qkv", f"{tag} {'qk'[i]}", got, z * mul, 1.5 * ez * mul + 1e-6 * (z * mul).abs(), nulp=2)
    vv = heads_view(x[:, 2 * c:split], b, ntok, heads, d)
    check("qkv", f"{tag} v", gv, vv, heads_view(e[:, 2 * c:split], b, ntok, heads, d) + 1e-6 * vv.abs(), nulp=1)
    if mlp:
        h = silu(x[:, split:])
        check("qkv", f"{tag} silu", g2, padded(h, m, ld2, off2), padded(1.2 * e[:, split:] + 1e-6 * h.abs(), m, ld2, off2), nulp=1)
        check("qkv", f"{tag} raw", graw, padded(x, m, ldraw), padded(e + 1e-6 * x.abs(), m, ldraw), nulp=1)
    else:
        assert torch.isnan(g2.float()).all() and torch.isnan(graw.float()).all()


@pytest.mark.parametrize("d,variant", [(64, 9), (128, 1)])
def test_qkv_persistent(capi, d, variant):
    """more tiles than resident workgroups: the persistent tile loop around the epilogue (d = 128: and its LDS exchange)"""
    test_qkv(capi, variant, d, 512, "mlp_raw", m=4096, k=64)


DIT_SHAPES = [(72, 80, 4, 384), (72, 128, 4, 384), (32, 32, 6, 96)]  # d, dstride, heads, ntok


@pytest.mark.parametrize("variant", NO_RING)
@pytest.mark.parametrize("d,dstride,heads,ntok", DIT_SHAPES)
@pytest.mark.parametrize("rotary", [True, False])
def test_qkv_dit(capi, variant, d, dstride, heads, ntok, rotary):
    m, k = 1536 if variant == 6 else 768, 128
    c = heads * d
    n = 3 * c
    b = m // ntok
    gen = torch.Generator().manual_seed(23 + d + dstride)
    a, w, da, dw, lda, ldw = dense_operands(gen, m, n, k)
    bias = torch.randn(n, generator=gen)
    cs = rope_table(gen, ntok, d)
    qscale = 0.3
    q, kk, v = (nan_buf(b, heads, ntok, dstride, dtype=torch.bfloat16) for _ in range(3))
    dsc = desc(capi, amode=A_DENSE, epi=E_QKV_DIT, variant=variant, A=da, lda=lda, W=dw, M=m, N=n, K=k, bias=bias.cuda(),
               q=q, k=kk, v=v, rope_cs=cs.cuda() if rotary else 0, heads=heads, d=d, ntok=ntok, qscale=qscale, dstride=dstride)
    gq, gk, gv = run(capi, dsc, [q, kk, v])
    acc, mag = product(a, w)
    x, e = acc + bias.double(), 1e-6 * (mag + bias.double().abs())

    def pad(t):  # [b, heads, ntok, d] -> rows of dstride, pad columns NaN (never written)
        o = torch.full((b, heads, ntok, dstride), NAN, dtype=torch.float64)
        o[..., :d] = t
        return o
    tag = f"qkv_dit d={d} dstride={dstride} rope={rotary} v={variant}"
    for i, (got, mul) in enumerate([(gq, qscale), (gk, 1.0), (gv, 1.0)]):
        xs = heads_view(x[:, i * c:(i + 1) * c], b, ntok, heads, d)
        es = heads_view(e[:, i * c:(i + 1) * c], b, ntok, heads, d)
        if rotary and i < 2:
            z, amp = rope(xs, cs)
            ez = torch.maximum(es[..., 0::2], es[..., 1::2]) * amp
            ez = torch.stack([ez, ez], -1).flatten(-2)
        else:
            z, ez = xs, es
        z, ez = z * mul, ez * mul
        check("qkv_dit", f"{tag} {'qkv'[i]}", got, pad(z), pad(ez + 1e-6 * z.abs()), nulp=2 if rotary and i < 2 else 1)


# ---------------------------------------------------------------------------------------------------- launcher refusals

def _refusal_cases():
    def base(**kw):
        f = dict(amode=A_DENSE, epi=E_F32, variant=1, M=256, N=128, K=128, ldo=128)
        f.update(kw)
        return f
    return {
        "m_off_grid": base(M=200),
        "m_off_256_grid": base(M=384, variant=4),
        "k_off_grid": base(K=100),
        "resid_bf_dense_not_ring": base(epi=E_BF16, resid_bf="out"),
        "ksplit_with_gate": base(K=512, ksplit=2, gate="gate", gate_rows=16, ldg=128),
        "ksplit_out_of_place_resid": base(K=512, ksplit=2, resid="resid"),
        "tr_rows_with_bias": base(epi=E_BF16, tr_rows=64, bias="bias"),
        "gn_part_n_not_32_cpg": base(N=192, ldo=192, gn_part="gn", gn_rows_per_bt=256, gn_cpg=4),
        "qkv_split_mismatch": base(epi=E_QKV, N=576, split=576, heads=2, d=64, ntok=256, q="qkv", k="qkv", v="qkv",
                                   qw="f", kw="f", rope_cs="f"),
        "qkv_on_ring": base(epi=E_QKV, N=576, split=576, heads=3, d=64, ntok=256, q="qkv", k="qkv", v="qkv",
                            qw="f", kw="f", rope_cs="f", variant=14),
    }


@pytest.mark.parametrize("case", list(_refusal_cases()))
def test_launcher_refusals(capi, case):
    f = _refusal_cases()[case]
    f32 = torch.full((2, 256 * 256), 7.0, device="cuda")
    bfb = torch.full((256 * 256,), 3.0, device="cuda", dtype=torch.bfloat16)
    qkv = torch.full((3 * 256 * 576,), 5.0, device="cuda", dtype=torch.bfloat16)
    ops = torch.ones(256 * 1024, device="cuda", dtype=torch.bfloat16)
    named = {"out": bfb, "gate": f32[1], "resid": f32[1], "bias": f32[1], "gn": f32[1], "qkv": qkv, "f": f32[1]}
    f = {k: named[v] if isinstance(v, str) else v for k, v in f.items()}
    outs = dict(out_f32=f32[0]) if f["epi"] == E_F32 else dict(out_bf16=bfb)
    before = [f32.clone(), bfb.clone(), qkv.clone()]
    with pytest.raises(capi.DfotError):
        call(capi, desc(capi, A=ops, lda=f["K"], W=ops, **outs, **f))
    torch.cuda.synchronize()
    for x, y in zip(before, [f32, bfb, qkv]):
        assert torch.equal(bits(x), bits(y)), f"{case}: refused call wrote its output"
