"""GPU tests of the three attention-map kernels at the op level (csrc/attention_map.hip): dfot_op_attention_map (forms full / frame),
dfot_op_attention_temporal_map and dfot_op_matrix_attention_map, each against an fp64 torch softmax of the SAME bf16 q, k.

Bars: the full form and the frame form against fp64 rel-L2 < 1.5e-2 (the project's attention-op bar, tests/test_gpu_dit.py:88); the frame
form against frame_map of the op's own full output 1e-4 absolute (fp32 sums of non-negative terms <= 1); every row of A and of F sums to 1
within 1e-4; two calls give the same bits; every shape refusal returns DFOT_ERR_SHAPE.

Planted structure: the keys of frame j carry a large component along the direction the queries of frame pi(j) carry, for a cyclic (for
T >= 3 non-symmetric) permutation pi, so the expected frame map is close to the permutation matrix M[pi(j)][j] = 1: a transposed or
mis-binned map fails whatever the tolerance.  Every test fails on the parent commit, whose library exports none of the entry points."""
import math

import pytest
import torch

import dit_facmat_common as fm

pytestmark = pytest.mark.gpu

OP_BAR = 1.5e-2
SUM_BAR = 1e-4
B, HEADS = 2, 2
LN2 = math.log(2.0)


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def pi(j, tokens):
    return (j + 1) % tokens


def permutation_map(tokens):
    m = torch.zeros(tokens, tokens, dtype=torch.float64)
    for j in range(tokens):
        m[pi(j, tokens), j] = 1.0
    return m


def planted_qk(lead, tokens, rows, d, seed):
    """q, k [*lead, tokens, rows, d] fp32: unit noise + a planted direction per frame (orthonormal u_f): q of frame f carries a u_f, k of
    frame j carries a u_pi(j), a^2 / sqrt(d) = 8 nats.  Returned as bf16 in the engine's pre-scaling: q * log2(e) / sqrt(d)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(*lead, tokens, rows, d, generator=g)
    k = torch.randn(*lead, tokens, rows, d, generator=g)
    u = torch.linalg.qr(torch.randn(d, d, generator=g))[0][:tokens]  # tokens <= 32 <= d orthonormal rows
    a = math.sqrt(8.0 * math.sqrt(d))
    for f in range(tokens):
        q[..., f, :, :] += a * u[f]
        k[..., f, :, :] += a * u[pi(f, tokens)]
    return (q * (math.log2(math.e) / math.sqrt(d))).to(torch.bfloat16), k.to(torch.bfloat16)


def padded(t):
    d = t.shape[-1]
    out = torch.zeros(*t.shape[:-1], 64 if d <= 64 else 128, dtype=torch.bfloat16)
    out[..., :d] = t
    return out.cuda().contiguous()


def check_frame_map(f, want, tokens, tag):
    assert torch.isfinite(f).all()
    r = rel(f, want)
    rows = (f.double().sum(-1) - 1).abs().max().item()
    print(f"{tag}: frame map rel-L2 vs fp64 {r:.2e}, rows sum to 1 within {rows:.1e}")
    assert r < OP_BAR
    assert rows <= SUM_BAR
    if tokens > 1:  # the planted permutation, independent of the tolerance
        m = permutation_map(tokens)
        assert (want * m).sum(-1).min().item() > 0.5, "the fp64 reference does not show the planted structure"
        assert torch.equal(f.argmax(-1).cpu(), m.argmax(-1).expand(f.shape[:-1]))
        assert (f.double().cpu() * m).sum(-1).min().item() > 0.5


# ---------------------------------------------------------------------------------------------------------------- full attention
def _workspace(temporal, batch, heads, tokens, patches):
    from dfot_amd import capi
    n = capi.lib.dfot_op_attention_map_workspace_bytes(int(temporal), batch, heads, tokens, patches)
    assert n > 0 and n % 4 == 0
    return torch.full((n // 4,), float("nan"), device="cuda"), n


def _run_map(q, k, form, tokens, patches, d):
    from dfot_amd import capi
    n = tokens * patches
    side = n if form == capi.ATTN_MAP_FULL else tokens
    out = torch.full((B, HEADS, side, side), float("nan"), device="cuda")
    ws, ws_bytes = _workspace(False, B, HEADS, tokens, patches)
    capi.check(capi.lib.dfot_op_attention_map(capi.ptr(q), capi.ptr(k), capi.ptr(out), capi.ptr(ws), ws_bytes, form, B, HEADS, n, tokens, d,
                                              capi.stream_ptr()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("tokens,patches,d", [(3, 128, 32), (2, 192, 72), (1, 128, 32)])
def test_attention_map_full_and_frame_vs_fp64(tokens, patches, d):
    """T 2 x P 192: the frame boundary (row 192) lies inside the second 128-row query tile.  T 1: the expected frame map is [[1]]."""
    from dfot_amd import capi, frame_map
    n = tokens * patches
    q, k = planted_qk((B, HEADS), tokens, patches, d, seed=100 * tokens + d)
    q, k = q.reshape(B, HEADS, n, d), k.reshape(B, HEADS, n, d)
    want = torch.softmax(q.double() @ k.double().transpose(-1, -2) * LN2, -1)
    qd, kd = padded(q), padded(k)
    full = _run_map(qd, kd, capi.ATTN_MAP_FULL, tokens, patches, d)
    frame = _run_map(qd, kd, capi.ATTN_MAP_FRAME, tokens, patches, d)
    assert torch.isfinite(full).all()
    r = rel(full.cpu(), want)
    rows = (full.double().sum(-1) - 1).abs().max().item()
    print(f"T={tokens} P={patches} d={d}: full map rel-L2 vs fp64 {r:.2e}, rows sum to 1 within {rows:.1e}")
    assert r < OP_BAR
    assert rows <= SUM_BAR
    check_frame_map(frame.cpu(), frame_map(want, tokens), tokens, f"T={tokens} P={patches} d={d}")
    own = (frame - frame_map(full, tokens)).abs().max().item()
    print(f"  frame form vs frame_map(full form): max abs {own:.1e}")
    assert own <= 1e-4
    if tokens == 1:
        assert (frame - 1).abs().max().item() <= SUM_BAR and tuple(frame.shape[-2:]) == (1, 1)
    assert torch.equal(full, _run_map(qd, kd, capi.ATTN_MAP_FULL, tokens, patches, d))
    assert torch.equal(frame, _run_map(qd, kd, capi.ATTN_MAP_FRAME, tokens, patches, d))


def test_attention_map_invalid_shapes():
    from dfot_amd import capi
    z = torch.zeros(B * HEADS * 512 * 128, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(B * HEADS * 512 * 512, device="cuda")
    ws = torch.zeros(1 << 16, device="cuda")

    def call(form, n, tokens, d, batch=B, heads=HEADS):
        return capi.lib.dfot_op_attention_map(capi.ptr(z), capi.ptr(z), capi.ptr(out), capi.ptr(ws), ws.numel() * 4, form, batch, heads, n, tokens,
                                              d, capi.stream_ptr())
    assert call(capi.ATTN_MAP_FRAME, 384, 3, 32) == capi.OK
    for form in (capi.ATTN_MAP_FRAME, capi.ATTN_MAP_FULL):
        for args in ((320, 5, 32),     # N % 128
                     (384, 4, 32),     # P = 96
                     (384, 0, 32), (33 * 128, 33, 32),
                     (384, 5, 32),     # tokens does not divide N
                     (384, 3, 130), (384, 3, 6), (384, 3, 0), (0, 1, 32)):
            assert call(form, *args) == capi.ERR_SHAPE, (form, args)
            assert capi.lib.dfot_last_error()
        assert call(form, 384, 3, 32, batch=0) == capi.ERR_SHAPE
        assert call(form, 384, 3, 32, heads=0) == capi.ERR_SHAPE
    assert call(7, 384, 3, 32) == capi.ERR_ARG
    # a frame-form workspace that is too small is refused before any launch
    assert capi.lib.dfot_op_attention_map(capi.ptr(z), capi.ptr(z), capi.ptr(out), capi.ptr(ws), 16, capi.ATTN_MAP_FRAME, B, HEADS, 384, 3, 32,
                                          capi.stream_ptr()) == capi.ERR_SHAPE
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- temporal attention
def _run_temporal_map(q, k, tokens, patches, d):
    from dfot_amd import capi
    out = torch.full((B, HEADS, tokens, tokens), float("nan"), device="cuda")
    ws, ws_bytes = _workspace(True, B, HEADS, tokens, patches)
    capi.check(capi.lib.dfot_op_attention_temporal_map(capi.ptr(q), capi.ptr(k), capi.ptr(out), capi.ptr(ws), ws_bytes, B, tokens, patches, HEADS, d,
                                                       capi.stream_ptr()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("tokens,patches,d", [(32, 64, 32), (3, 128, 72), (5, 192, 64), (1, 64, 32)])
def test_attention_temporal_map_vs_fp64(tokens, patches, d):
    """operands as the per-frame QKV epilogue leaves them: [(b t)][heads][P][dstride]; the map is the mean over the patch positions of the
    T x T softmax of every (video, head, patch)"""
    q, k = planted_qk((B, HEADS), tokens, patches, d, seed=7 + 100 * tokens + d)  # b h t p d
    w = torch.softmax(torch.einsum("bhtpd,bhspd->bhpts", q.double(), k.double()) * LN2, -1).mean(2)  # b h t s
    qd, kd = (padded(t.permute(0, 2, 1, 3, 4).reshape(B * tokens, HEADS, patches, d)) for t in (q, k))
    got = _run_temporal_map(qd, kd, tokens, patches, d)
    check_frame_map(got.cpu(), w, tokens, f"temporal T={tokens} P={patches} d={d}")
    if tokens == 1:
        assert (got - 1).abs().max().item() <= SUM_BAR
    assert torch.equal(got, _run_temporal_map(qd, kd, tokens, patches, d))


def test_attention_temporal_map_invalid_shapes():
    from dfot_amd import capi
    z = torch.zeros(8 * 128 * 128, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(1 << 12, device="cuda")
    ws = torch.zeros(1 << 16, device="cuda")

    def call(batch, tokens, patches, heads, d, ws_bytes=ws.numel() * 4):
        return capi.lib.dfot_op_attention_temporal_map(capi.ptr(z), capi.ptr(z), capi.ptr(out), capi.ptr(ws), ws_bytes, batch, tokens, patches,
                                                       heads, d, capi.stream_ptr())
    assert call(1, 4, 64, 1, 64) == capi.OK
    for args in ((1, 0, 64, 1, 64), (1, 33, 64, 1, 64), (1, 4, 32, 1, 64), (1, 4, 96, 1, 64), (1, 4, 64, 1, 66), (1, 4, 64, 1, 136),
                 (0, 4, 64, 1, 64), (1, 4, 64, 0, 64), (1, 4, 64, 1, 64, 16)):
        assert call(*args) == capi.ERR_SHAPE, args
        assert capi.lib.dfot_last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- matrix attention
def _run_matrix_map(z, tokens, h, cc, rr, table, e=fm.OP_E):
    from dfot_amd import capi
    zd = z.to(torch.bfloat16).cuda()
    out = torch.full((B, cc, rr, tokens, tokens), float("nan"), device="cuda")
    scale = 1.0 / math.sqrt((e // cc) * (h // rr))
    capi.check(capi.lib.dfot_op_matrix_attention_map(capi.ptr(zd), capi.ptr(table), capi.ptr(out), B, tokens, e, h, cc, rr, scale,
                                                     capi.stream_ptr()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("tokens", [1, 5, 32])
def test_matrix_attention_map_vs_fp64(tokens):
    """z and the table as dfot_op_matrix_attention_rope takes them, with and without rope_cs, at every head shape of the forward's op test"""
    for cc, rr, h in fm.OP_HEADS:
        z = fm.make_z(B, tokens, cc, rr, h)
        for rope in (True, False):
            _, w = fm.matrix_attention_ref(z, B, tokens, fm.OP_E, h, cc, rr, rope)  # b c r l l'
            table = fm.rope_table(tokens, h // rr).cuda() if rope else None
            got = _run_matrix_map(z, tokens, h, cc, rr, table)
            assert torch.isfinite(got).all()
            r = rel(got.cpu(), w)
            rows = (got.double().sum(-1) - 1).abs().max().item()
            print(f"matrix map L={tokens} (cc, rr, h)={(cc, rr, h)} rope={rope}: rel-L2 {r:.2e}, rows sum to 1 within {rows:.1e}")
            assert r < OP_BAR and rows <= SUM_BAR
            if tokens == 1:
                assert (got - 1).abs().max().item() <= SUM_BAR
            assert torch.equal(got, _run_matrix_map(z, tokens, h, cc, rr, table))


@pytest.mark.parametrize("tokens", [5, 32])
def test_matrix_attention_map_planted_permutation(tokens):
    """no rotation (a rotation by the frame's own angle would undo the alignment): q of frame f and k of frame j with pi(j) = f share a
    planted (hn x hd) matrix, so the map is close to the permutation matrix"""
    cc, rr, h = fm.OP_HEADS[1]
    e, hn, hd = fm.OP_E, fm.OP_E // cc, h // rr
    g = torch.Generator().manual_seed(tokens)
    z = torch.randn(B, tokens, cc, hn, 3, rr, hd, generator=g)
    u = torch.randn(tokens, hn, hd, generator=g)
    u = u / u.flatten(1).norm(dim=1)[:, None, None]
    a = math.sqrt(8.0 * math.sqrt(hn * hd))
    for f in range(tokens):
        z[:, f, :, :, 0] += a * u[f][None, None, :, None, :]
        z[:, f, :, :, 1] += a * u[pi(f, tokens)][None, None, :, None, :]
    z = z.reshape(B * tokens * e, 3 * h).to(torch.bfloat16).float()
    _, w = fm.matrix_attention_ref(z, B, tokens, e, h, cc, rr, False)
    got = _run_matrix_map(z, tokens, h, cc, rr, None)
    check_frame_map(got.cpu(), w, tokens, f"matrix map planted L={tokens}")


def test_matrix_attention_map_invalid_shapes():
    from dfot_amd import capi
    z = torch.zeros(2 * 32 * 64 * 3 * 128, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(1 << 14, device="cuda")

    def call(batch, tokens, e, h, cc, rr):
        return capi.lib.dfot_op_matrix_attention_map(capi.ptr(z), None, capi.ptr(out), batch, tokens, e, h, cc, rr, 0.01, capi.stream_ptr())
    assert call(2, 4, 64, 128, 1, 4) == capi.OK
    for args in ((2, 0, 64, 128, 1, 4), (2, 33, 64, 128, 1, 4), (2, 4, 64, 128, 3, 4), (2, 4, 64, 128, 1, 3), (2, 4, 64, 120, 1, 20),
                 (0, 4, 64, 128, 1, 4)):
        assert call(*args) == capi.ERR_SHAPE, args
        assert capi.lib.dfot_last_error()
    assert capi.lib.dfot_op_matrix_attention_map(None, None, capi.ptr(out), 2, 4, 64, 128, 1, 4, 0.01, capi.stream_ptr()) == capi.ERR_ARG
    torch.cuda.synchronize()
