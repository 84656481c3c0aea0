"""Host-side checks of the DiT1D training kernels' entry points (csrc/dit1d_train.hip; no GPU): every entry point is declared, bound with
the same arity, exported and documented; the closed forms the kernels implement agree with float64 autograd of an independent formulation to
1e-12; the DiT3D-style LayerNorm backward (one incoming gradient, the residual gradient routed through (1 + scale) and into dshift / dscale)
is NOT that closed form; and the argument refusals that are decided before any HIP call return the named error.

Fails on the parent commit: it has no dfot_op_dit1d_ln_share_train / _ln_share_bwd / _final_bwd / _tok_embed_wgrad / _tok_embed_dgrad."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import dit1d_train_ops_common as tc
import dit_block_common as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = {  # name -> argument count
    "dfot_op_dit1d_ln_share_train": 12, "dfot_op_dit1d_ln_share_bwd": 13, "dfot_op_dit1d_final_bwd": 14, "dfot_op_dit1d_tok_embed_wgrad": 10,
    "dfot_op_dit1d_tok_embed_dgrad": 8,
}
TIGHT = dict(rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_entry_points_are_declared_bound_and_exported(name):
    from dfot_amd import capi
    text = open(os.path.join(ROOT, "include", "dfot_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, f"{name} is not declared in include/dfot_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == ENTRY_POINTS[name] and args[-1] == "void* stream"
    res, bound = capi.SIGNATURES[name]
    assert res is C.c_int and len(bound) == len(args)
    for a, b in zip(args, bound):
        want = C.c_void_p if "*" in a else C.c_int64 if a.startswith("int64_t") else C.c_float if a.startswith("float") else C.c_int
        assert b is want, (name, a, b)
    assert getattr(capi.lib, name) is not None
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _rand(*shape, seed=0, scale=1.5, shift=0.3):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return scale * torch.randn(*shape, generator=g, dtype=torch.float64) + shift


def _share_case():
    per, frames, hidden = 8, 3, 192
    x = _rand(frames * per, hidden)
    sh, sc = _rand(frames, hidden, seed=1, scale=1.0, shift=0.0), _rand(frames, hidden, seed=2, scale=1.0, shift=0.0)
    return per, frames, hidden, x, sh, sc, _rand(frames * per, hidden, seed=3), _rand(frames * per, hidden, seed=4)


def test_ln_share_reference_is_torch_layer_norm_and_its_modulation():
    per, frames, hidden, x, sh, sc, _, _ = _share_case()
    n, m = tc.ln_share(x, sh, sc, per)
    want = F.layer_norm(x, (hidden,), eps=bc.EPS)
    torch.testing.assert_close(n, want, **TIGHT)
    torch.testing.assert_close(m, (want.reshape(frames, per, hidden) * (1 + sc[:, None]) + sh[:, None]).reshape(-1, hidden), **TIGHT)


def _closed_form(x, sc, dres, dm, per):
    """what d1_ln_share_bwd_kernel computes, from the saved n and rstd"""
    n, rstd = bc.layer_norm(x), tc.rstd_of(x)[:, None]
    dn = dres if dm is None else dres + dm * (1 + bc.per_row(sc, per))
    dx = rstd * (dn - dn.mean(-1, keepdim=True) - n * (dn * n).mean(-1, keepdim=True))
    if dm is None:
        return dx, None, None
    frames = x.shape[0] // per
    return dx, dm.reshape(frames, per, -1).sum(1), (dm * n).reshape(frames, per, -1).sum(1)


def test_ln_share_backward_by_autograd_is_the_closed_form():
    """the block as the reference composes it -- x_out = n + gate * f(m), here with f = identity-like linear probes: autograd of <dres, n> +
    <dm, m> through torch's own F.layer_norm -- against dn = dres + dm (1 + scale), dshift = sum dm, dscale = sum dm n"""
    per, frames, hidden, x, sh, sc, dres, dm = _share_case()
    xx, s1, s2 = x.clone().requires_grad_(), sh.clone().requires_grad_(), sc.clone().requires_grad_()
    n = F.layer_norm(xx, (hidden,), eps=bc.EPS)
    m = n * (1 + s2.repeat_interleave(per, 0)) + s1.repeat_interleave(per, 0)
    want = torch.autograd.grad((dres * n).sum() + (dm * m).sum(), (xx, s1, s2))
    for got, ref in zip(_closed_form(x, sc, dres, dm, per), want):
        torch.testing.assert_close(got, ref, **TIGHT)
    for got, ref in zip(tc.ln_share_backward(x, sh, sc, dres, dm, per), want):  # the restatement the GPU tests differentiate
        torch.testing.assert_close(got, ref, **TIGHT)
    # dm == None: a plain LayerNorm backward
    (want_dx,) = torch.autograd.grad(F.layer_norm(xx, (hidden,), eps=bc.EPS), xx, dres)
    torch.testing.assert_close(_closed_form(x, sc, dres, None, per)[0], want_dx, **TIGHT)
    torch.testing.assert_close(tc.ln_share_backward(x, None, None, dres, None, per)[0], want_dx, **TIGHT)


def test_the_dit3d_layer_norm_backward_is_a_different_function():
    """The DiT3D blocks add onto the modulated row, so their LayerNorm backward takes ONE gradient down every path.  Fed dres + dm it misses
    all three outputs of the share_norm backward by O(1): what the 2e-2 bar of the GPU tests has to tell apart is not subtle."""
    per, frames, hidden, x, sh, sc, dres, dm = _share_case()
    dx, dsh, dsc = _closed_form(x, sc, dres, dm, per)
    g = dres + dm
    wrong_dx, _, _ = _closed_form(x, sc, torch.zeros_like(g), g, per)
    n = bc.layer_norm(x)
    wrong_dsh, wrong_dsc = g.reshape(frames, per, -1).sum(1), (g * n).reshape(frames, per, -1).sum(1)
    rel = [float((a - b).norm() / b.norm()) for a, b in ((wrong_dx, dx), (wrong_dsh, dsh), (wrong_dsc, dsc))]
    print("DiT3D-style backward against the share_norm backward, rel-L2 of dx, dshift, dscale:", rel)
    assert min(rel) > 0.3, rel
    # ... and a backward that normalises with the neighbouring row's n and rstd: smaller (only the two projection terms and the row's scale
    # move), still more than five times the 2e-2 bar
    shifted_dx, _, _ = _closed_form(x.roll(1, 0), sc, dres, dm, per)
    rel = float((shifted_dx - dx).norm() / dx.norm())
    print("neighbouring row's statistics, rel-L2 of dx:", rel)
    assert rel > 5 * 2e-2, rel


@pytest.mark.parametrize("c,l", [(1, 16), (4, 32)])
def test_final_and_token_embedding_backward_closed_forms(c, l):
    """d nf = dout W through the LayerNorm backward, dW = sum_rows dout nf, db = sum dout; dW = sum_rows dX0 x, db = sum dX0, dx = dX0 W --
    with rows <-> (frame, c, l) across a video boundary -- against autograd of the restatements of tests/dit_block_common.py"""
    videos, t, hidden = 2, 3, 64
    frames, rows = videos * t, videos * t * l
    x = _rand(rows, hidden).requires_grad_()
    w, b = (_rand(c, hidden, seed=1, shift=0.0) / 8).requires_grad_(), _rand(c, seed=2).requires_grad_()
    dout = _rand(frames, c, l, seed=3)
    out = tc.final_forward(x, w, b, frames, l)
    for f in range(frames):  # the restatement against torch's own modules, row by row
        torch.testing.assert_close(out[f], F.linear(F.layer_norm(x[f * l:(f + 1) * l], (hidden,), eps=bc.EPS), w, b).t(), **TIGHT)
    dx, dw, db = torch.autograd.grad(out, (x, w, b), dout)
    with torch.no_grad():
        drow = tc.frames_to_rows(dout)
        n, rstd = bc.layer_norm(x), tc.rstd_of(x)[:, None]
        dn = drow @ w
        torch.testing.assert_close(dx, rstd * (dn - dn.mean(-1, keepdim=True) - n * (dn * n).mean(-1, keepdim=True)), **TIGHT)
        torch.testing.assert_close(dw, drow.t() @ n, **TIGHT)
        torch.testing.assert_close(db, drow.sum(0), **TIGHT)
    xin = _rand(frames, c, l, seed=4).requires_grad_()
    ew, eb, pos = _rand(hidden, c, seed=5).requires_grad_(), _rand(hidden, seed=6).requires_grad_(), _rand(t * l, hidden, seed=7)
    d0 = _rand(rows, hidden, seed=8)
    gx, gw, gb = torch.autograd.grad(tc.tok_embed_forward(xin, ew, eb, pos, videos), (xin, ew, eb), d0)
    with torch.no_grad():
        torch.testing.assert_close(gw, d0.t() @ tc.frames_to_rows(xin), **TIGHT)
        torch.testing.assert_close(gb, d0.sum(0), **TIGHT)
        torch.testing.assert_close(tc.frames_to_rows(gx), d0 @ ew, **TIGHT)


# ---- refusals decided on the host: no pointer is dereferenced and no HIP call is made before them ----
def _refused(rc, code, text):
    from dfot_amd import capi
    msg = (capi.lib.dfot_last_error() or b"").decode()
    assert rc == code and text in msg, (rc, msg)


def test_refusals_by_name():
    from dfot_amd import capi
    lib, p, null = capi.lib, C.c_void_p(4096), C.c_void_p(0)
    S, A = capi.ERR_SHAPE, capi.ERR_ARG
    _refused(lib.dfot_op_dit1d_ln_share_train(p, p, p, p, p, 512, 64, 96, 16, 32, 1e-6, null), S, "ln_share_train: hidden 96 must be a multiple of 64")
    _refused(lib.dfot_op_dit1d_ln_share_train(p, p, p, p, p, 8192, 64, 2112, 16, 32, 1e-6, null), S, "hidden 2112 must be a multiple of 64, <= 2048")
    _refused(lib.dfot_op_dit1d_ln_share_train(p, p, p, p, p, 512, 64, 128, 16, 40, 1e-6, null), S, "40 rows of 16 per frame")
    _refused(lib.dfot_op_dit1d_ln_share_train(p, p, p, p, p, 64 + 2 * 128 - 4, 64, 128, 16, 32, 1e-6, null), A, "ln_share_train: table row of 316")
    _refused(lib.dfot_op_dit1d_ln_share_train(p, p, p, p, p, 512, 64, 128, 16, 32, 0.0, null), A, "eps 0")
    _refused(lib.dfot_op_dit1d_ln_share_bwd(p, p, p, p, p, 512, 64, p, p, 128, 6, 2, null), S, "ln_share_bwd: rows_per_frame 6 must be a multiple of 4")
    _refused(lib.dfot_op_dit1d_ln_share_bwd(p, p, p, p, p, 512, 64, p, p, 128, 16, 0, null), S, "ln_share_bwd: 0 frames")
    _refused(lib.dfot_op_dit1d_ln_share_bwd(p, p, p, p, p, 512, 64, p, p, 192 + 2048, 16, 2, null), S, "hidden 2240 must be a multiple of 64, <= 2048")
    _refused(lib.dfot_op_dit1d_ln_share_bwd(p, p, p, p, p, 128, 64, p, p, 128, 16, 2, null), A, "ln_share_bwd: table row of 128")
    _refused(lib.dfot_op_dit1d_ln_share_bwd(p, p, p, p, p, 512, 64, p, p, 2048, 1 << 20, 2, null), S, "rows x hidden must stay below 2^31")
    _refused(lib.dfot_op_dit1d_final_bwd(p, p, p, p, p, p, p, p, 128, 65, 16, 32, 1e-6, null), S, "final_bwd: in_channels 65 must be in [1, 64]")
    _refused(lib.dfot_op_dit1d_final_bwd(p, p, p, p, p, p, p, p, 128, 4, 16, 40, 1e-6, null), S, "final_bwd: 40 rows of 16 per frame")
    _refused(lib.dfot_op_dit1d_final_bwd(p, p, p, p, p, p, p, p, 100, 4, 16, 32, 1e-6, null), S, "final_bwd: hidden 100")
    _refused(lib.dfot_op_dit1d_tok_embed_wgrad(p, p, p, p, p, 0, 16, 128, 32, null), S, "tok_embed_wgrad: in_channels 0")
    _refused(lib.dfot_op_dit1d_tok_embed_wgrad(p, p, p, p, p, 4, 16, 128, 0, null), S, "tok_embed_wgrad: 0 rows")
    _refused(lib.dfot_op_dit1d_tok_embed_dgrad(p, p, p, 4, 0, 128, 32, null), S, "tok_embed_dgrad: 32 rows of 0 per frame")
    _refused(lib.dfot_op_dit1d_tok_embed_dgrad(p, p, p, 4, 16, 2112, 32, null), S, "tok_embed_dgrad: hidden 2112")


def test_null_pointers_are_refused():
    from dfot_amd import capi
    lib, p, null = capi.lib, C.c_void_p(4096), C.c_void_p(0)
    calls = {
        "ln_share_train": (5, lambda a: lib.dfot_op_dit1d_ln_share_train(*a, 512, 64, 128, 16, 32, 1e-6, null)),
        "final_bwd": (8, lambda a: lib.dfot_op_dit1d_final_bwd(*a, 128, 4, 16, 32, 1e-6, null)),
        "tok_embed_wgrad": (5, lambda a: lib.dfot_op_dit1d_tok_embed_wgrad(*a, 4, 16, 128, 32, null)),
        "tok_embed_dgrad": (3, lambda a: lib.dfot_op_dit1d_tok_embed_dgrad(*a, 4, 16, 128, 32, null)),
    }
    for name, (n, call) in calls.items():
        for missing in range(n):
            rc = call([null if i == missing else p for i in range(n)])
            msg = (lib.dfot_last_error() or b"").decode()
            assert rc == capi.ERR_ARG and msg.startswith(f"dit1d {name}: null argument"), (name, missing, rc, msg)

    def bwd(a):  # dres, dm, N, rstd, table | dx, dmod_part
        return lib.dfot_op_dit1d_ln_share_bwd(*a[:5], 512, 64, *a[5:], 128, 16, 2, null)
    for missing in (0, 2, 3, 4, 5, 6):  # with dm given, everything else is needed
        assert bwd([null if i == missing else p for i in range(7)]) == capi.ERR_ARG, missing
        assert (lib.dfot_last_error() or b"").decode().startswith("dit1d ln_share_bwd: null argument")
    for missing in (0, 2, 3, 5):  # without dm, the table and dmod_part are not
        assert bwd([null if i in (1, 4, 6, missing) else p for i in range(7)]) == capi.ERR_ARG, missing
