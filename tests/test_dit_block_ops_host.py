"""Host-side checks of the DiT / DiT1D block op entry points (no GPU): every entry point is declared, bound with the same arity and
exported; every float64 restatement of tests/dit_block_common.py agrees with an independent float64 formulation to 1e-12; and the argument
refusals that are decided before any HIP call return the named error."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import dit_block_common as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = {  # name -> argument count
    "dfot_op_dit_ln_mod": 13, "dfot_op_dit_gate_combine": 10, "dfot_op_dit_gate_bwd": 14, "dfot_op_dit_ln_bwd": 14, "dfot_op_dit_ln_bwd_rows": 12,
    "dfot_op_dit_gelu": 5, "dfot_op_dit_patch_embed": 12, "dfot_op_dit_patch_embed_dgrad": 10, "dfot_op_dit_patch_embed_wgrad": 11,
    "dfot_op_dit_final_gather": 10, "dfot_op_dit_qkv_grad_pack": 11, "dfot_op_dit1d_tok_embed": 11, "dfot_op_dit1d_ln_share": 13,
    "dfot_op_dit1d_final": 10,
}


def _declared_args(name):
    text = open(os.path.join(ROOT, "include", "dfot_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, f"{name} is not declared in include/dfot_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_entry_points_are_declared_bound_and_exported(name):
    from dfot_amd import capi
    args = _declared_args(name)
    assert len(args) == ENTRY_POINTS[name] and args[-1] == "void* stream"
    res, bound = capi.SIGNATURES[name]
    assert res is C.c_int and len(bound) == len(args)
    for a, b in zip(args, bound):  # pointers are bound as pointers, 64-bit integers as 64-bit, floats as floats
        want = C.c_void_p if "*" in a else C.c_int64 if a.startswith("int64_t") else C.c_float if a.startswith("float") else C.c_int
        assert b is want, (name, a, b)
    assert getattr(capi.lib, name) is not None  # exported by the built library
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _rand(*shape, seed=0, scale=1.5, shift=0.3):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return scale * torch.randn(*shape, generator=g, dtype=torch.float64) + shift


TIGHT = dict(rtol=1e-12, atol=1e-12)


def test_ln_mod_reference_is_torch_layer_norm_modulated():
    x, sh, sc = _rand(21, 320), _rand(3, 320, seed=1, scale=1.0, shift=0.0), _rand(3, 320, seed=2, scale=1.0, shift=0.0)
    want = F.layer_norm(x, (320,), eps=bc.EPS).reshape(3, 7, 320) * (1 + sc[:, None]) + sh[:, None]
    torch.testing.assert_close(bc.ln_mod(x, sh, sc, 7), want.reshape(21, 320), **TIGHT)


def test_ln_mod_backward_by_autograd_is_the_closed_form():
    """dx = rstd (g - mean g - xhat mean(g xhat)), g = dm (1 + scale); dshift = sum_rows dm; dscale = sum_rows dm xhat"""
    rows_per_frame, frames, hidden = 8, 3, 192
    x = _rand(frames * rows_per_frame, hidden).requires_grad_()
    sh = _rand(frames, hidden, seed=1, scale=1.0, shift=0.0).requires_grad_()
    sc = _rand(frames, hidden, seed=2, scale=1.0, shift=0.0).requires_grad_()
    dm = _rand(frames * rows_per_frame, hidden, seed=3)
    dx, dsh, dsc = torch.autograd.grad(bc.ln_mod(x, sh, sc, rows_per_frame), (x, sh, sc), dm)
    with torch.no_grad():
        mean = x.mean(-1, keepdim=True)
        rstd = 1 / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + bc.EPS)
        xhat = (x - mean) * rstd
        g = dm * (1 + bc.per_row(sc, rows_per_frame))
        torch.testing.assert_close(dx, rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True)), **TIGHT)
        torch.testing.assert_close(dsh, dm.reshape(frames, rows_per_frame, hidden).sum(1), **TIGHT)
        torch.testing.assert_close(dsc, (dm * xhat).reshape(frames, rows_per_frame, hidden).sum(1), **TIGHT)


def test_gate_combine_reference_and_its_gradients():
    rows_per_frame, frames, hidden = 4, 3, 64
    x, a = _rand(12, hidden), _rand(12, hidden, seed=1).requires_grad_()
    gate = _rand(frames, hidden, seed=2, scale=1.0, shift=0.0).requires_grad_()
    y = bc.gate_combine(x, a, gate, rows_per_frame)
    want = torch.stack([x[r] + gate[r // rows_per_frame] * a[r] for r in range(12)])
    torch.testing.assert_close(y, want, **TIGHT)
    dy = _rand(12, hidden, seed=3)
    da, dgate = torch.autograd.grad(y, (a, gate), dy)
    torch.testing.assert_close(da, torch.stack([dy[r] * gate[r // rows_per_frame] for r in range(12)]).detach(), **TIGHT)
    torch.testing.assert_close(dgate, torch.einsum("frc,frc->fc", dy.reshape(3, 4, hidden), a.detach().reshape(3, 4, hidden)), **TIGHT)


def test_gelu_reference_is_torch_tanh_gelu_and_its_derivative():
    x = torch.linspace(-8, 8, 4001, dtype=torch.float64).requires_grad_()
    torch.testing.assert_close(bc.gelu_tanh(x), F.gelu(x, approximate="tanh"), **TIGHT)
    (g,) = torch.autograd.grad(bc.gelu_tanh(x).sum(), x)
    with torch.no_grad():  # d/dx [x s], s = sigmoid(2 t), t = sqrt(2 / pi) (x + 0.044715 x^3)
        k = (2 / torch.pi) ** 0.5
        s = torch.sigmoid(2 * k * (x + 0.044715 * x ** 3))
        torch.testing.assert_close(g, s + x * 2 * s * (1 - s) * k * (1 + 3 * 0.044715 * x ** 2), **TIGHT)


@pytest.mark.parametrize("c,patch,hidden", [(4, 1, 16), (3, 2, 24), (8, 2, 32)])
def test_patch_embed_reference_is_conv2d_and_its_gradients_are_the_transposed_convolution(c, patch, hidden):
    frames, gh, gw = 5, 2, 4
    x = _rand(frames, c, gh * patch, gw * patch).requires_grad_()
    w = (_rand(hidden, c * patch * patch, seed=1, shift=0.0) / (c * patch * patch) ** 0.5).requires_grad_()
    b, pos = _rand(hidden, seed=2, scale=0.1).requires_grad_(), _rand(gh * gw, hidden, seed=3)
    out = bc.patch_embed(x, w, b, patch, pos)
    conv = F.conv2d(x, w.reshape(hidden, c, patch, patch), b, stride=patch)  # [frames][hidden][gh][gw]
    want = conv.permute(0, 2, 3, 1).reshape(frames * gh * gw, hidden) + pos.repeat(frames, 1)
    torch.testing.assert_close(out, want, **TIGHT)
    dy = _rand(frames * gh * gw, hidden, seed=4)
    dx, dw, db = torch.autograd.grad(out, (x, w, b), dy)
    dyc = dy.reshape(frames, gh, gw, hidden).permute(0, 3, 1, 2)
    torch.testing.assert_close(dx, F.conv_transpose2d(dyc, w.detach().reshape(hidden, c, patch, patch), stride=patch), **TIGHT)
    torch.testing.assert_close(dw, dy.t() @ bc.patchify(x.detach(), patch), **TIGHT)
    torch.testing.assert_close(db, dy.sum(0), **TIGHT)


def test_unpatchify_reference_places_every_element_and_inverts_by_its_own_adjoint():
    c, patch, gh, gw, frames = 3, 2, 2, 4, 2
    h, w = gh * patch, gw * patch
    y = _rand(frames * gh * gw, patch * patch * c)
    out = bc.unpatchify(y, c, h, w, patch)
    for f in range(frames):
        for g in range(gh * gw):
            for o in range(patch * patch * c):  # o = (p, q, channel), channel fastest
                ch, pq = o % c, o // c
                assert out[f, ch, (g // gw) * patch + pq // patch, (g % gw) * patch + pq % patch] == y[f * gh * gw + g, o]
    yy = y.clone().requires_grad_()
    dout = _rand(frames, c, h, w, seed=1)
    (gathered,) = torch.autograd.grad(bc.unpatchify(yy, c, h, w, patch), yy, dout)  # what final_gather computes
    assert torch.equal(bc.unpatchify(gathered, c, h, w, patch), dout)


def test_rope_rotation_reference_is_a_complex_product_and_its_transpose_the_inverse_rotation():
    b, heads, ntok, d = 2, 3, 5, 8
    x = _rand(b, heads, ntok, d)
    th = _rand(ntok, d // 2, seed=1, scale=2.0, shift=0.0)
    y = bc.rope_rotate(x, th.cos(), th.sin())
    want = torch.view_as_real(torch.view_as_complex(x.reshape(b, heads, ntok, d // 2, 2).contiguous()) * torch.polar(torch.ones_like(th), th))
    torch.testing.assert_close(y, want.flatten(-2), **TIGHT)
    xx = x.clone().requires_grad_()
    g = _rand(b, heads, ntok, d, seed=2)
    (gx,) = torch.autograd.grad(bc.rope_rotate(xx, th.cos(), th.sin()), xx, g)
    torch.testing.assert_close(gx, bc.rope_rotate(g, (-th).cos(), (-th).sin()), **TIGHT)


def test_qkv_pack_reference_column_order():
    b, heads, ntok, d, dstride = 2, 3, 4, 8, 16
    dq, dk, dv = (_rand(b, heads, ntok, dstride, seed=s) for s in range(3))
    out = bc.qkv_pack(dq, dk, dv, d)
    assert out.shape == (b * ntok, 3 * heads * d)
    for which, src in enumerate((dq, dk, dv)):
        for bb in range(b):
            for hh in range(heads):
                for t in range(ntok):
                    assert torch.equal(out[bb * ntok + t, (which * heads + hh) * d:(which * heads + hh + 1) * d], src[bb, hh, t, :d])


def test_dit1d_references():
    bsz, t, c, l, hidden = 2, 3, 4, 16, 64
    x, w, b, pos = _rand(bsz, t, c, l), _rand(hidden, c, seed=1), _rand(hidden, seed=2), _rand(t * l, hidden, seed=3)
    emb = bc.d1_tok_embed(x, w, b, pos)
    for bb in range(bsz):
        for tt in range(t):
            for ll in (0, 5, l - 1):
                want = w @ x[bb, tt, :, ll] + b + pos[tt * l + ll]
                torch.testing.assert_close(emb[(bb * t + tt) * l + ll], want, **TIGHT)
    fw, fb = _rand(c, hidden, seed=4) / 8, _rand(c, seed=5)
    out = bc.d1_final(emb, fw, fb, bsz, t, l)
    assert out.shape == (bsz, t, c, 1, l)
    lin = F.linear(F.layer_norm(emb, (hidden,), eps=bc.EPS), fw, fb)
    for bb in range(bsz):
        for tt in range(t):
            torch.testing.assert_close(out[bb, tt, :, 0, :], lin[(bb * t + tt) * l:(bb * t + tt + 1) * l].t(), **TIGHT)


# ---- refusals decided on the host: no pointer is dereferenced and no HIP call is made before them ----
def _refused(rc, code, text):
    from dfot_amd import capi
    msg = (capi.lib.dfot_last_error() or b"").decode()
    assert rc == code and text in msg, (rc, msg)


def test_refusals_by_name():
    from dfot_amd import capi
    lib, p, null = capi.lib, C.c_void_p(4096), C.c_void_p(0)  # p: a non-null address that is never dereferenced
    # a width with no LayerNorm instance
    _refused(lib.dfot_op_dit_ln_mod(p, p, p, p, p, 64 + 3 * 704, 64, 704, 8, 16, 1e-6, 4, null), capi.ERR_SHAPE, "hidden size 704 has no LayerNorm kernel instance")
    _refused(lib.dfot_op_dit_ln_bwd_rows(p, p, p, 64 + 3 * 704, 64, p, p, 704, 8, 2, 1e-6, null), capi.ERR_SHAPE, "hidden size 704 has no LayerNorm kernel instance")
    _refused(lib.dfot_op_dit_ln_bwd(p, p, p, 64 + 3 * 704, 64, p, p, p, p, 704, 8, 2, 1e-6, null), capi.ERR_SHAPE, "hidden size 704 has no LayerNorm kernel instance")
    # the frame reductions split a frame's rows into four chunks
    _refused(lib.dfot_op_dit_gate_bwd(p, p, p, 512, 64, p, p, p, p, p, 128, 6, 2, null), capi.ERR_ARG, "gate_bwd: 6 rows per frame must be a multiple of 4")
    _refused(lib.dfot_op_dit_ln_bwd(p, p, p, 512, 64, p, p, p, p, 128, 7, 2, 1e-6, null), capi.ERR_ARG, "ln_bwd: 7 rows per frame must be a multiple of 4")
    _refused(lib.dfot_op_dit_gate_combine(p, p, p, p, 512, 64, 130, 4, 8, null), capi.ERR_SHAPE, "gate_combine: hidden 130 must be a positive multiple of 4")
    # the pack moves 8 columns per thread
    _refused(lib.dfot_op_dit_qkv_grad_pack(p, p, p, null, p, 40, 40, 2, 60, 64, null), capi.ERR_SHAPE, "head dim 60")
    _refused(lib.dfot_op_dit_qkv_grad_pack(p, p, p, null, p, 40, 40, 2, 64, 60, null), capi.ERR_ARG, "head stride 60")
    # the patch vector
    for fn, args in ((lib.dfot_op_dit_patch_embed, (p, p, p, null, p)), (lib.dfot_op_dit_patch_embed_dgrad, (p, p, p)),
                     (lib.dfot_op_dit_patch_embed_wgrad, (p, p, p, p))):
        _refused(fn(*args, 65, 4, 8, 2, 128, 8, null), capi.ERR_SHAPE, "patch vector too long (patch_size^2 * channels = 260, at most 256)")
    _refused(lib.dfot_op_dit_final_gather(p, p, p, 8, 65, 4, 8, 2, 320, null), capi.ERR_SHAPE, "patch vector too long")
    _refused(lib.dfot_op_dit_final_gather(p, p, p, 8, 3, 4, 8, 2, 8, null), capi.ERR_ARG, "row stride 8 of dyp is shorter than the 12 outputs")
    _refused(lib.dfot_op_dit_patch_embed(p, p, p, null, p, 4, 4, 8, 2, 128, 9, null), capi.ERR_SHAPE, "9 rows are no whole number of 8-patch frames")
    _refused(lib.dfot_op_dit_gelu(p, p, p, 12, null), capi.ERR_SHAPE, "gelu: 12 elements")
    # table rows too short for the columns the op touches
    _refused(lib.dfot_op_dit_ln_mod(p, p, p, p, p, 64 + 2 * 128 - 4, 64, 128, 8, 16, 1e-6, 4, null), capi.ERR_ARG, "ln_mod: table row of 316")
    _refused(lib.dfot_op_dit_gate_bwd(p, p, p, 128, 64, p, p, p, p, p, 128, 8, 2, null), capi.ERR_ARG, "gate_bwd: table row of 128")
    # DiT1D
    _refused(lib.dfot_op_dit1d_ln_share(p, p, p, p, p, 512, 64, 96, 16, 32, 1e-6, 4, null), capi.ERR_SHAPE, "hidden 96 must be a multiple of 64")
    _refused(lib.dfot_op_dit1d_final(p, p, p, p, 2112, 4, 16, 32, 1e-6, null), capi.ERR_SHAPE, "hidden 2112 must be a multiple of 64, <= 2048")
    _refused(lib.dfot_op_dit1d_tok_embed(p, p, p, p, p, 65, 16, 32, 128, 64, null), capi.ERR_SHAPE, "in_channels 65 must be in [1, 64]")
    _refused(lib.dfot_op_dit1d_tok_embed(p, p, p, p, p, 4, 16, 40, 128, 80, null), capi.ERR_SHAPE, "80 rows in sequences of 40 tokens, 16 per frame")


def test_null_pointers_are_refused():
    from dfot_amd import capi
    lib, p, null = capi.lib, C.c_void_p(4096), C.c_void_p(0)
    calls = {
        "ln_mod": lambda a: lib.dfot_op_dit_ln_mod(*a, 512, 64, 128, 8, 16, 1e-6, 4, null),
        "gate_combine": lambda a: lib.dfot_op_dit_gate_combine(*a, 512, 64, 128, 8, 16, null),
        "gelu": lambda a: lib.dfot_op_dit_gelu(a[0], null, null, 8, null),
        "patch_embed_dgrad": lambda a: lib.dfot_op_dit_patch_embed_dgrad(*a, 4, 4, 8, 2, 128, 8, null),
        "patch_embed_wgrad": lambda a: lib.dfot_op_dit_patch_embed_wgrad(*a, 4, 4, 8, 2, 128, 8, null),
        "final_gather": lambda a: lib.dfot_op_dit_final_gather(*a, 8, 4, 4, 8, 2, 64, null),
        "dit1d final": lambda a: lib.dfot_op_dit1d_final(*a, 128, 4, 16, 32, 1e-6, null),
    }
    counts = {"ln_mod": 5, "gate_combine": 4, "gelu": 1, "patch_embed_dgrad": 3, "patch_embed_wgrad": 4, "final_gather": 3, "dit1d final": 4}
    for name, n in counts.items():
        for missing in range(n):
            args = [null if i == missing else p for i in range(n)]
            rc = calls[name](args)
            msg = (lib.dfot_last_error() or b"").decode()
            assert rc == capi.ERR_ARG and msg.startswith(f"{name}: null argument"), (name, missing, rc, msg)
    assert lib.dfot_op_dit_gelu(p, null, null, 8, null) == capi.ERR_ARG  # u given, neither output
    assert lib.dfot_op_dit_gate_bwd(p, p, p, 512, 64, p, p, null, p, p, 128, 8, 2, null) == capi.ERR_ARG
    assert lib.dfot_op_dit_ln_bwd(p, p, p, 512, 64, p, null, p, p, 128, 8, 2, 1e-6, null) == capi.ERR_ARG
    assert lib.dfot_op_dit_qkv_grad_pack(p, p, null, null, p, 40, 40, 2, 64, 64, null) == capi.ERR_ARG
    assert lib.dfot_op_dit_patch_embed(p, p, null, null, p, 4, 4, 8, 2, 128, 8, null) == capi.ERR_ARG
    assert lib.dfot_op_dit1d_tok_embed(p, p, p, null, p, 4, 16, 32, 128, 64, null) == capi.ERR_ARG
    assert lib.dfot_op_dit1d_ln_share(p, p, p, p, null, 512, 64, 128, 16, 32, 1e-6, 4, null) == capi.ERR_ARG
