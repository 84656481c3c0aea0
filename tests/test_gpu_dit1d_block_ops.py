"""The DiT1D forward's own kernels at op level: dfot_op_dit1d_tok_embed (the channel-major frame read), dfot_op_dit1d_ln_share (LN(x) written
back in place as the residual base, its modulated bf16 copy, the `c < hidden` guard of a lane's chunks) and dfot_op_dit1d_final (the direct
(B, T, C, 1, L) write), each through the launcher the engine's forward calls, against the float64 restatements of tests/dit_block_common.py.

Input rules and bars are those of tests/test_gpu_dit_block_ops.py: table row stride larger than the op's columns at a non-zero offset, a
different table row for every frame, noise levels that include -1 and max_level + 1, data 1.5 randn + 0.3, NaN in every output before the
launch, two runs with the same bits; fp32 outputs within 8 x the error of the same formula in torch float32 (e32), bf16 outputs within
2^-8 |ref| + 8 x e32's max-abs, fp32 dot products within (N + 4) 2^-24 sum |terms| per element.

Measured on one MI355X (kernel max-abs / rel-L2 against float64; e32 = torch float32 on the same inputs):
  d1_tok_embed (8 cases)                max-abs 8.6e-07 .. 2.7e-06, rel-L2 4.2e-08 .. 1.2e-07; worst |err| / bound 0.33
  d1_ln_share LN(x) in place            max-abs 4.0e-07 .. 6.6e-07, rel-L2 5.1e-08 .. 5.3e-08; at most 1.35 x e32's max-abs, 1.01 x its rel-L2
  d1_ln_share modulated bf16            worst |err| / (2^-8 |ref| + slack) 0.995
  d1_final                              max-abs 3.9e-07 .. 5.8e-07, rel-L2 9.1e-08 .. 1.1e-07; worst |err| / bound 0.008
"""
import functools
import zlib

import pytest
import torch

import dit_block_common as bc
from dit_block_common import bits

pytestmark = pytest.mark.gpu

OFF = 64
# (C, L, T, hidden): a wave covers 256 channels per chunk: hidden 128 = half of the first chunk live; 320 = a quarter of the second;
# 1152 = four chunks and half of a fifth; 2048 = all eight
SHAPES = [(4, 32, 4, 128), (16, 32, 3, 320), (64, 16, 2, 1152), (4, 128, 1, 2048)]
CASES = [(*s, b) for s in SHAPES for b in (2, 3)]


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


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    _alive.clear()
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y)), "two runs of one op differ"
    return a


@functools.lru_cache(maxsize=None)
def case(C, L, T, hidden, batch):
    g = gen("d1", C, L, T, hidden, batch)
    frames = batch * T
    x = data(g, batch, T, C, 1, L)
    w = torch.randn(hidden, C, generator=g) / C ** 0.5
    b = 0.1 * torch.randn(hidden, generator=g)
    pos = torch.randn(T * L, hidden, generator=g)  # random per token: a wrong token index is a wrong row
    X = data(g, frames * L, hidden)                # a residual stream for ln_share and final
    table = torch.randn(frames, OFF + 2 * hidden + 32, generator=g)
    rows_of = torch.randperm(frames, generator=g)
    levels = rows_of.clone()
    levels[rows_of == 0] = -1
    levels[rows_of == frames - 1] = frames
    fw = torch.randn(C, hidden, generator=g) / hidden ** 0.5
    fb = 0.1 * torch.randn(C, generator=g)
    return dict(x=x, w=w, b=b, pos=pos, X=X, table=table, rows_of=rows_of, levels=levels.int(), fw=fw, fb=fb)


@pytest.mark.parametrize("C,L,T,hidden,batch", CASES)
def test_tok_embed(C, L, T, hidden, batch):
    from dfot_amd import capi
    c = case(C, L, T, hidden, batch)
    rows = batch * T * L

    def run():
        X = nan(rows, hidden)
        ok(capi.lib.dfot_op_dit1d_tok_embed(D(c["x"]), D(c["w"]), D(c["b"]), D(c["pos"]), P(X), C, L, T * L, hidden, rows,
                                            stream()))
        return (X,)
    (X,) = twice(run)
    x, w, b, pos = (c[k].double() for k in ("x", "w", "b", "pos"))
    ref = bc.d1_tok_embed(x[..., 0, :], w, b, pos)
    terms = bc.d1_tok_embed(x[..., 0, :].abs(), w.abs(), b.abs(), pos.abs())  # sum |w x| + |b| + |pos|
    bc.assert_sum_bound(f"d1_tok_embed C {C} L {L} T {T} hidden {hidden} batch {batch}", X.cpu(), ref, terms, C + 1)


@pytest.mark.parametrize("C,L,T,hidden,batch", CASES)
def test_ln_share(C, L, T, hidden, batch):
    from dfot_amd import capi
    c = case(C, L, T, hidden, batch)
    frames, rows = batch * T, batch * T * L
    table = c["table"]

    def run():
        X, A = c["X"].cuda(), nan(rows, hidden, dtype=torch.bfloat16)
        idx = torch.full((frames,), -7, dtype=torch.int32, device="cuda")
        ok(capi.lib.dfot_op_dit1d_ln_share(P(X), P(A), D(table), D(c["levels"]), P(idx), table.shape[1], OFF, hidden, L, rows, bc.EPS,
                                           frames - 1, stream()))
        return X, A, idx
    X, A, idx = twice(run)
    assert torch.equal(idx.cpu().long(), c["rows_of"])  # -1 and frames are clamped onto rows 0 and frames - 1
    name = f"d1_ln_share L {L} T {T} hidden {hidden} batch {batch}"
    refs = {}
    for dt in (torch.float64, torch.float32):
        ln = bc.layer_norm(c["X"].to(dt))
        sh, sc = table[c["rows_of"], OFF:OFF + hidden].to(dt), table[c["rows_of"], OFF + hidden:OFF + 2 * hidden].to(dt)
        refs[dt] = (ln, bc.modulate(ln, bc.per_row(sh, L), bc.per_row(sc, L)))
    bc.assert_fp32_within(f"{name} LN(x) in place", X.cpu(), refs[torch.float64][0], refs[torch.float32][0])
    slack = 8 * bc.errors(refs[torch.float32][1], refs[torch.float64][1])[0]
    bc.assert_bf16_of_fp32(f"{name} modulated bf16", A.cpu(), refs[torch.float64][1], slack)


@pytest.mark.parametrize("C,L,T,hidden,batch", CASES)
def test_final(C, L, T, hidden, batch):
    from dfot_amd import capi
    c = case(C, L, T, hidden, batch)
    rows = batch * T * L

    def run():
        out = nan(batch, T, C, 1, L)
        ok(capi.lib.dfot_op_dit1d_final(D(c["X"]), D(c["fw"]), D(c["fb"]), P(out), hidden, C, L, rows, bc.EPS, stream()))
        return (out,)
    (out,) = twice(run)
    X, fw, fb = c["X"].double(), c["fw"].double(), c["fb"].double()
    ref = bc.d1_final(X, fw, fb, batch, T, L)
    terms = (bc.layer_norm(X).abs() @ fw.abs().t() + fb.abs()).reshape(batch, T, L, C).permute(0, 1, 3, 2).unsqueeze(-2)
    assert out.shape == ref.shape == (batch, T, C, 1, L)
    bc.assert_sum_bound(f"d1_final C {C} L {L} T {T} hidden {hidden} batch {batch}", out.cpu(), ref, terms, hidden)
