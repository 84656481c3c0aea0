"""The DiT1D training kernels at op level (csrc/dit1d_train.hip): dfot_op_dit1d_ln_share_train, dfot_op_dit1d_ln_share_bwd,
dfot_op_dit1d_final_bwd, dfot_op_dit1d_tok_embed_wgrad and dfot_op_dit1d_tok_embed_dgrad, each through the launcher a training engine calls,
against float64: the forward restatements of tests/dit_block_common.py / tests/dit1d_train_ops_common.py, differentiated by torch.autograd.

Fails on the parent commit: none of the five entry points exists there.

Inputs (the rules of tests/test_gpu_dit_block_ops.py): data 1.5 randn + 0.3; one table row per frame with O(1) shift and scale, the row stride
larger than what the op touches and its columns at a non-zero offset, so that a frame reading its neighbour's scale is an O(1) error; both
incoming gradients of the share_norm backward non-zero and independent, so that the DiT3D backward (the residual gradient pushed through
(1 + scale) and into dshift / dscale: O(1) wrong in all three outputs, tests/test_dit1d_train_ops_host.py) cannot pass; every output
pre-filled with NaN and followed by a guard band that must keep its bits; dmod_part pre-filled with a finite sentinel that must survive
outside the op's columns; every op runs twice and the two results have the same bits; the last frame (or the second video) alone gives the
bits it has inside the batch.

Shapes: hidden 64 (48 of a wave's 64 lanes idle), 192 (first chunk partly live), 1152 (four chunks and half of the fifth), 2048 (all eight);
16 and 32 rows per frame (one and two rows per wave of the backward's workgroup), and for the backward also 8 (two of the four waves
without a row) and 24 (waves 0, 1 take two rows, waves 2, 3 one); 3 frames; the forward also at 3 frames of 6 rows (18 rows: its last
workgroup holds two rows).  The model's ends at C 1, 4, 64 x L 16, 32 x hidden 64, 1152 with two videos of three frames: 96 / 192 rows, so
the 64-row partial sums see a partial last chunk and a video boundary inside a chunk.

Bars (none taken from the kernels): BAR = 2e-2 rel-L2 per output, the project's op bar, asserted for every output.  These kernels are pure
fp32, so every fp32 output is also held to FP32 = 1e-5 rel-L2: unit roundoff 2^-24 = 6e-8, a row statistic is a sum of <= 2048 terms in a
lane-then-butterfly tree (<= 8 + 6 additions deep), a weight gradient a serial sum of <= 64 then <= 3 terms, and the operands N and rstd
arrive rounded to fp32 -- two orders of magnitude of room over a few units of roundoff, three orders under BAR.  The per-frame planes are
held per element to (n + 4) 2^-24 sum |terms| (bc.assert_sum_bound, terms from the op's own fp32 operands), the bf16 operand per element to
2^-8 |ref| plus 8 x the max-abs error of torch's float32 evaluation.

Measured on one MI355X (rel-L2 against float64, over all cases):
  ln_share_train N / rstd               4.9e-08 .. 5.8e-08 / 3.1e-08 .. 4.5e-08; N and the bf16 operand bit-equal to dfot_op_dit1d_ln_share's
  ln_share_train bf16 operand           1.6e-03 .. 1.7e-03; worst |err| / (2^-8 |ref| + slack) 0.99
  ln_share_bwd dx / dshift / dscale     6.1e-08 .. 6.5e-08 / 4.4e-08 .. 5.1e-08 / 6.0e-08 .. 7.3e-08; planes: worst |err| / bound 0.22
  ln_share_bwd without dm, dx           5.2e-08 .. 5.5e-08
  final_bwd dx / stats / dW / db        6.0e-08 .. 1.6e-07 / 3.6e-08 .. 4.1e-08 / 1.4e-07 .. 1.7e-07 / 2.9e-08 .. 1.4e-07
  tok_embed dW / db / dx                1.3e-07 .. 1.6e-07 / 7.5e-08 .. 1.1e-07 / 6.7e-08 .. 9.2e-08
  guard bands, untouched columns, run-to-run, in place: bit-equal in every case.  The last frame alone: N, rstd, the bf16 operand, dx and
  its rows of the dmod_part planes bit-equal to the batch's.  The second video alone: dx and stats of final_bwd and dx of tok_embed
  bit-equal; dW and db are sums over every row of the batch and are not compared across batch sizes
"""
import functools
import zlib

import pytest
import torch

import dit1d_train_ops_common as tc
import dit_block_common as bc
from dit_block_common import bits

pytestmark = pytest.mark.gpu

OFF = 64
BAR = 2e-2
FP32 = 1e-5
GUARD = 512       # elements behind every output
GUARD_VALUE = 7.25
FRAMES = 3
HIDDENS = (64, 192, 1152, 2048)


def P(t):
    from dfot_amd import capi
    return capi.ptr(t)


_alive = []


def D(t):
    """device pointer of a copy of a host tensor, kept alive until twice() has synchronised"""
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


def guarded(*shape, dtype=torch.float32):
    """a NaN-filled output of `shape` with GUARD elements of GUARD_VALUE behind it (one flat allocation)"""
    n = 1
    for s in shape:
        n *= s
    t = torch.full((n + GUARD,), float("nan"), dtype=dtype, device="cuda")
    t[n:] = GUARD_VALUE
    return t


def body(t, *shape):
    """the output part of a guarded buffer; asserts the guard band kept its value"""
    n = t.numel() - GUARD
    assert bool((t[n:] == GUARD_VALUE).all()), "the guard band behind an output was written"
    return t[:n].reshape(*shape)


def sentinel(*shape):
    return torch.randn(*shape, generator=gen("sentinel", *shape)) + 3.0


def twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    _alive.clear()
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y)), "two runs of one op differ"
    return a


def check(name, got, ref64, bar=FP32):
    g = got.detach().cpu()
    assert not bool(torch.isnan(g).any()), f"{name}: an element was not written"
    k = bc.errors(g, ref64)
    print(f"{name}: max-abs {k[0]:.3e} rel-L2 {k[1]:.3e}")
    assert k[1] < BAR and k[1] < bar, (name, k)


# ---- share_norm LayerNorm: training forward and backward -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ln_case(hidden, per):
    g = gen("d1t ln", hidden, per)
    rows = FRAMES * per
    x, dres, dm = data(g, rows, hidden), data(g, rows, hidden), data(g, rows, hidden)
    table = torch.randn(FRAMES, OFF + 2 * hidden + 32, generator=g)
    x64 = x.double()
    n32, rstd32 = bc.layer_norm(x64).float(), tc.rstd_of(x64).float()  # what a forward saved: the backward's fp32 operands
    return dict(x=x, dres=dres, dm=dm, table=table, n32=n32, rstd32=rstd32)


def shift_scale(c, hidden, dt):
    return c["table"][:, OFF:OFF + hidden].to(dt), c["table"][:, OFF + hidden:OFF + 2 * hidden].to(dt)


def run_ln_train(c, hidden, per, frames=slice(None)):
    from dfot_amd import capi
    x = c["x"].reshape(FRAMES, per, hidden)[frames].reshape(-1, hidden)
    table = c["table"][frames]
    rows = x.shape[0]
    N, rstd, M = guarded(rows, hidden), guarded(rows), guarded(rows, hidden, dtype=torch.bfloat16)
    ok(capi.lib.dfot_op_dit1d_ln_share_train(D(x), P(N), P(rstd), P(M), D(table), table.shape[1], OFF, hidden, per, rows, bc.EPS, stream()))
    return N, rstd, M


@pytest.mark.parametrize("hidden,per", [(h, p) for h in HIDDENS for p in (16, 32)] + [(192, 6)])
def test_ln_share_train(hidden, per):
    from dfot_amd import capi
    c = ln_case(hidden, per)
    rows = FRAMES * per
    N, rstd, M = (body(t, *s) for t, s in zip(twice(lambda: run_ln_train(c, hidden, per)), ((rows, hidden), (rows,), (rows, hidden))))
    name = f"ln_share_train hidden {hidden} rows {FRAMES} x {per}"
    refs = {}
    for dt in (torch.float64, torch.float32):
        sh, sc = shift_scale(c, hidden, dt)
        refs[dt] = tc.ln_share(c["x"].to(dt), sh, sc, per)
    check(f"{name} N", N, refs[torch.float64][0])
    check(f"{name} rstd", rstd, tc.rstd_of(c["x"].double()))
    check(f"{name} M", M.float(), refs[torch.float64][1], bar=2.0 ** -8)
    slack = 8 * bc.errors(refs[torch.float32][1], refs[torch.float64][1])[0]
    bc.assert_bf16_of_fp32(f"{name} M", M.cpu(), refs[torch.float64][1], slack)
    # the last frame alone: the bits it has inside the batch (its own table row, not its neighbour's)
    N1, rstd1, M1 = run_ln_train(c, hidden, per, slice(FRAMES - 1, FRAMES))
    torch.cuda.synchronize()
    _alive.clear()
    assert torch.equal(bits(body(N1, per, hidden)), bits(N[-per:])) and torch.equal(bits(body(rstd1, per)), bits(rstd[-per:]))
    assert torch.equal(bits(body(M1, per, hidden)), bits(M[-per:]))
    # N is the residual base the inference kernel leaves in place: the same bits, so a trainer's forward normalises as DiT1D does
    X, A = c["x"].cuda(), torch.empty(rows, hidden, dtype=torch.bfloat16, device="cuda")
    idx = torch.empty(FRAMES, dtype=torch.int32, device="cuda")
    levels = torch.arange(FRAMES, dtype=torch.int32)
    ok(capi.lib.dfot_op_dit1d_ln_share(P(X), P(A), D(c["table"]), D(levels), P(idx), c["table"].shape[1], OFF, hidden, per, rows, bc.EPS,
                                       FRAMES - 1, stream()))
    torch.cuda.synchronize()
    _alive.clear()
    assert torch.equal(bits(X), bits(N)) and torch.equal(bits(A), bits(M))


def run_ln_bwd(c, hidden, per, with_dm=True, frames=slice(None), in_place=False):
    from dfot_amd import capi

    def pick(t):
        return t.reshape(FRAMES, per, *t.shape[1:])[frames].reshape(-1, *t.shape[1:])
    dres, dm, n32, rstd32 = (pick(c[k]) for k in ("dres", "dm", "n32", "rstd32"))
    table = c["table"][frames]
    nf, ldt = table.shape
    part = sentinel(tc.PLANES, nf, ldt).cuda()
    if in_place:
        dx = guarded(nf * per, hidden)
        dx[:nf * per * hidden] = dres.cuda().reshape(-1)
        src = P(dx)
    else:
        dx, src = guarded(nf * per, hidden), D(dres)
    ok(capi.lib.dfot_op_dit1d_ln_share_bwd(src, D(dm) if with_dm else None, D(n32), D(rstd32), D(table), ldt, OFF, P(dx), P(part), hidden, per, nf,
                                           stream()))
    return dx, part


@pytest.mark.parametrize("hidden,per", [(h, p) for h in HIDDENS for p in (16, 32)] + [(192, 8), (192, 24)])
def test_ln_share_bwd(hidden, per):
    c = ln_case(hidden, per)
    rows = FRAMES * per
    dx, part = twice(lambda: run_ln_bwd(c, hidden, per))
    dx = body(dx, rows, hidden)
    name = f"ln_share_bwd hidden {hidden} rows {FRAMES} x {per}"
    sh, sc = shift_scale(c, hidden, torch.float64)
    rdx, rdsh, rdsc = tc.ln_share_backward(c["x"].double(), sh, sc, c["dres"].double(), c["dm"].double(), per)
    check(f"{name} dx", dx, rdx)
    p = part.cpu()
    want = sentinel(*p.shape)
    inside = torch.zeros(p.shape[-1], dtype=torch.bool)
    inside[OFF:OFF + 2 * hidden] = True
    assert torch.equal(bits(p[:, :, ~inside]), bits(want[:, :, ~inside])), f"{name}: dmod_part written outside its columns"
    total = (p[0] + p[1]) + (p[2] + p[3])
    check(f"{name} dshift", total[:, OFF:OFF + hidden], rdsh)
    check(f"{name} dscale", total[:, OFF + hidden:OFF + 2 * hidden], rdsc)
    # plane z = rows [z, z + 1) per / 4 of every frame, from the op's own fp32 operands
    dm64 = c["dm"].double()
    terms = torch.cat((dm64, dm64 * c["n32"].double()), 1).reshape(FRAMES, tc.PLANES, per // tc.PLANES, 2 * hidden)
    for z in range(tc.PLANES):
        bc.assert_sum_bound(f"{name} plane {z}", p[z][:, OFF:OFF + 2 * hidden], terms[:, z].sum(1), terms[:, z].abs().sum(1), per // tc.PLANES + 3)
    # dx written over dres, and the last frame alone: the same bits
    dx_ip, part_ip = run_ln_bwd(c, hidden, per, in_place=True)
    dx1, part1 = run_ln_bwd(c, hidden, per, frames=slice(FRAMES - 1, FRAMES))
    torch.cuda.synchronize()
    _alive.clear()
    assert torch.equal(bits(body(dx_ip, rows, hidden)), bits(dx)) and torch.equal(bits(part_ip), bits(part))
    assert torch.equal(bits(body(dx1, per, hidden)), bits(dx[-per:]))
    assert torch.equal(bits(part1[:, 0, OFF:OFF + 2 * hidden]), bits(part[:, -1, OFF:OFF + 2 * hidden]))


@pytest.mark.parametrize("hidden,per", [(64, 16), (192, 32), (1152, 16), (2048, 32)])
def test_ln_share_bwd_without_modulation(hidden, per):
    """dm == NULL, the final layer's LayerNorm: dn = dres; the table and dmod_part are not touched (a null table is accepted)"""
    from dfot_amd import capi
    c = ln_case(hidden, per)
    rows = FRAMES * per
    dx, part = twice(lambda: run_ln_bwd(c, hidden, per, with_dm=False))
    rdx, _, _ = tc.ln_share_backward(c["x"].double(), None, None, c["dres"].double(), None, per)
    check(f"ln_share_bwd (no dm) hidden {hidden} rows {FRAMES} x {per} dx", body(dx, rows, hidden), rdx)
    assert torch.equal(bits(part.cpu()), bits(sentinel(*part.shape)))
    dx0 = guarded(rows, hidden)
    ok(capi.lib.dfot_op_dit1d_ln_share_bwd(D(c["dres"]), None, D(c["n32"]), D(c["rstd32"]), None, 0, 0, P(dx0), None, hidden, per, FRAMES, stream()))
    torch.cuda.synchronize()
    _alive.clear()
    assert torch.equal(bits(dx0), bits(dx))


# ---- the two ends of the model ---------------------------------------------------------------------------------------------------
VIDEOS, T = 2, 3
END_CASES = [(C, L, h) for C in (1, 4, 64) for L in (16, 32) for h in (64, 1152)]


@functools.lru_cache(maxsize=None)
def end_case(C, L, hidden):
    g = gen("d1t ends", C, L, hidden)
    frames, rows = VIDEOS * T, VIDEOS * T * L
    return dict(X=data(g, rows, hidden), fw=torch.randn(C, hidden, generator=g) / hidden ** 0.5, fb=0.1 * torch.randn(C, generator=g),
                dout=data(g, frames, C, L), x=data(g, frames, C, L), w=torch.randn(hidden, C, generator=g) / C ** 0.5,
                b=0.1 * torch.randn(hidden, generator=g), pos=torch.randn(T * L, hidden, generator=g), dX0=data(g, rows, hidden))


def run_final_bwd(c, C, L, hidden, videos=slice(None)):
    from dfot_amd import capi
    X = c["X"].reshape(VIDEOS, T * L, hidden)[videos].reshape(-1, hidden)
    dout = c["dout"].reshape(VIDEOS, T, C, L)[videos].reshape(-1, C, L)
    rows = X.shape[0]
    dx, stats, dW, db = guarded(rows, hidden), guarded(rows, 2), guarded(C, hidden), guarded(C)
    part = guarded(tc.part_floats(rows, C, hidden, C))
    ok(capi.lib.dfot_op_dit1d_final_bwd(D(dout), D(X), D(c["fw"]), P(dx), P(stats), P(part), P(dW), P(db), hidden, C, L, rows, bc.EPS, stream()))
    return dx, stats, dW, db, part


@pytest.mark.parametrize("C,L,hidden", END_CASES)
def test_final_bwd(C, L, hidden):
    c = end_case(C, L, hidden)
    frames, rows = VIDEOS * T, VIDEOS * T * L
    dx, stats, dW, db, part = twice(lambda: run_final_bwd(c, C, L, hidden))
    dx, stats, dW, db = body(dx, rows, hidden), body(stats, rows, 2), body(dW, C, hidden), body(db, C)
    body(part, tc.part_floats(rows, C, hidden, C))
    X, fw, fb = c["X"].double().requires_grad_(), c["fw"].double().requires_grad_(), c["fb"].double().requires_grad_()
    rdx, rdw, rdb = torch.autograd.grad(tc.final_forward(X, fw, fb, frames, L), (X, fw, fb), c["dout"].double())
    name = f"final_bwd C {C} L {L} hidden {hidden}"
    check(f"{name} dx", dx, rdx)
    check(f"{name} stats", stats, torch.stack((X.detach().mean(-1), tc.rstd_of(X.detach())), -1))
    check(f"{name} dW", dW, rdw)
    check(f"{name} db", db, rdb)
    dx1, stats1, _, _, _ = run_final_bwd(c, C, L, hidden, slice(1, 2))  # the second video alone
    torch.cuda.synchronize()
    _alive.clear()
    assert torch.equal(bits(body(dx1, T * L, hidden)), bits(dx[T * L:])) and torch.equal(bits(body(stats1, T * L, 2)), bits(stats[T * L:]))


def run_tok_embed_bwd(c, C, L, hidden, videos=slice(None)):
    from dfot_amd import capi
    dX0 = c["dX0"].reshape(VIDEOS, T * L, hidden)[videos].reshape(-1, hidden)
    x = c["x"].reshape(VIDEOS, T, C, L)[videos].reshape(-1, C, L)
    rows = dX0.shape[0]
    dW, db, dx = guarded(hidden, C), guarded(hidden), guarded(rows // L, C, L)
    part = guarded(tc.part_floats(rows, C, hidden, hidden))
    ok(capi.lib.dfot_op_dit1d_tok_embed_wgrad(D(dX0), D(x), P(part), P(dW), P(db), C, L, hidden, rows, stream()))
    ok(capi.lib.dfot_op_dit1d_tok_embed_dgrad(D(dX0), D(c["w"]), P(dx), C, L, hidden, rows, stream()))
    return dW, db, dx, part


@pytest.mark.parametrize("C,L,hidden", END_CASES)
def test_tok_embed_bwd(C, L, hidden):
    c = end_case(C, L, hidden)
    frames, rows = VIDEOS * T, VIDEOS * T * L
    dW, db, dx, part = twice(lambda: run_tok_embed_bwd(c, C, L, hidden))
    dW, db, dx = body(dW, hidden, C), body(db, hidden), body(dx, frames, C, L)
    body(part, tc.part_floats(rows, C, hidden, hidden))
    x, w, b = c["x"].double().requires_grad_(), c["w"].double().requires_grad_(), c["b"].double().requires_grad_()
    rdx, rdw, rdb = torch.autograd.grad(tc.tok_embed_forward(x, w, b, c["pos"].double(), VIDEOS), (x, w, b), c["dX0"].double())
    name = f"tok_embed_bwd C {C} L {L} hidden {hidden}"
    check(f"{name} dW", dW, rdw)
    check(f"{name} db", db, rdb)
    check(f"{name} dx", dx, rdx)
    _, _, dx1, _ = run_tok_embed_bwd(c, C, L, hidden, slice(1, 2))  # the second video alone
    torch.cuda.synchronize()
    _alive.clear()
    assert torch.equal(bits(body(dx1, T, C, L)), bits(dx[T:]))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_invalid_shapes_and_null_pointers_launch_nothing():
    from dfot_amd import capi
    lib, S, A = capi.lib, capi.ERR_SHAPE, capi.ERR_ARG
    hidden, per, C, L = 128, 16, 4, 16
    rows, ldt = FRAMES * per, OFF + 2 * hidden
    z = torch.zeros(rows * hidden, device="cuda")
    outs = [torch.full((rows * hidden,), float("nan"), device="cuda") for _ in range(5)]
    zp, o = P(z), [P(t) for t in outs]
    s = stream()
    calls = [
        (lib.dfot_op_dit1d_ln_share_train(zp, o[0], o[1], o[2], zp, ldt, OFF, 96, per, rows, bc.EPS, s), S),
        (lib.dfot_op_dit1d_ln_share_train(zp, o[0], o[1], o[2], zp, ldt, OFF, hidden, per, rows + 1, bc.EPS, s), S),
        (lib.dfot_op_dit1d_ln_share_train(zp, o[0], o[1], o[2], zp, ldt - 4, OFF, hidden, per, rows, bc.EPS, s), A),
        (lib.dfot_op_dit1d_ln_share_train(zp, o[0], None, o[2], zp, ldt, OFF, hidden, per, rows, bc.EPS, s), A),
        (lib.dfot_op_dit1d_ln_share_bwd(zp, zp, zp, zp, zp, ldt, OFF, o[0], o[1], hidden, 6, FRAMES, s), S),
        (lib.dfot_op_dit1d_ln_share_bwd(zp, zp, zp, zp, zp, ldt, OFF, o[0], o[1], 2112, per, FRAMES, s), S),
        (lib.dfot_op_dit1d_ln_share_bwd(zp, zp, zp, zp, zp, ldt, OFF, o[0], o[1], hidden, per, 0, s), S),
        (lib.dfot_op_dit1d_ln_share_bwd(zp, zp, zp, zp, zp, ldt, OFF + 2, o[0], o[1], hidden, per, FRAMES, s), A),
        (lib.dfot_op_dit1d_ln_share_bwd(zp, zp, zp, zp, zp, ldt, OFF, o[0], None, hidden, per, FRAMES, s), A),
        (lib.dfot_op_dit1d_ln_share_bwd(zp, None, zp, None, zp, ldt, OFF, o[0], o[1], hidden, per, FRAMES, s), A),
        (lib.dfot_op_dit1d_final_bwd(zp, zp, zp, o[0], o[1], o[2], o[3], o[4], hidden, 65, L, rows, bc.EPS, s), S),
        (lib.dfot_op_dit1d_final_bwd(zp, zp, zp, o[0], o[1], o[2], o[3], o[4], hidden, C, L, rows + 8, bc.EPS, s), S),
        (lib.dfot_op_dit1d_final_bwd(zp, zp, zp, o[0], o[1], o[2], o[3], o[4], hidden, C, L, rows, 0.0, s), A),
        (lib.dfot_op_dit1d_final_bwd(zp, zp, zp, o[0], o[1], None, o[3], o[4], hidden, C, L, rows, bc.EPS, s), A),
        (lib.dfot_op_dit1d_tok_embed_wgrad(zp, zp, o[0], o[1], o[2], 0, L, hidden, rows, s), S),
        (lib.dfot_op_dit1d_tok_embed_wgrad(zp, zp, o[0], o[1], o[2], C, L, hidden + 32, rows, s), S),
        (lib.dfot_op_dit1d_tok_embed_wgrad(zp, zp, o[0], None, o[2], C, L, hidden, rows, s), A),
        (lib.dfot_op_dit1d_tok_embed_dgrad(zp, zp, o[0], C, 0, hidden, rows, s), S),
        (lib.dfot_op_dit1d_tok_embed_dgrad(zp, zp, o[0], C, L, hidden, -rows, s), S),
        (lib.dfot_op_dit1d_tok_embed_dgrad(zp, None, o[0], C, L, hidden, rows, s), A),
    ]
    for i, (rc, want) in enumerate(calls):
        assert rc == want, (i, rc, lib.dfot_last_error())
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs) and bool((z == 0).all())  # nothing was launched
    # the same buffers with valid arguments: zero gradients in, zeros out (and nothing past the live part)
    ok(lib.dfot_op_dit1d_ln_share_bwd(zp, zp, zp, zp, zp, ldt, OFF, o[0], o[1], hidden, per, FRAMES, s))
    torch.cuda.synchronize()
    assert bool((outs[0] == 0).all())
    live = outs[1][:tc.PLANES * FRAMES * ldt].reshape(tc.PLANES, FRAMES, ldt)
    assert bool((live[:, :, OFF:] == 0).all()) and bool(torch.isnan(live[:, :, :OFF]).all()) and bool(torch.isnan(outs[1][live.numel():]).all())
