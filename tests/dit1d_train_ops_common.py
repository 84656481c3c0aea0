"""Restatements for the op-level tests of the DiT1D training kernels (csrc/dit1d_train.hip), on top of tests/dit_block_common.py: the
share_norm LayerNorm, whose backward is taken by torch.autograd (nothing here restates a gradient by hand), and the (frame, c, l) <-> row
maps of the model's two ends.  Written on the tensors' own dtype: float64 is the yardstick."""
import torch

import dit_block_common as bc

PLANES = 4     # planes of dmod_part
SUM_ROWS = 64  # rows per partial sum of the two weight gradients (the size of the `part` workspaces)


def ln_share(x, shift, scale, rows_per_frame, eps=bc.EPS):
    """share_norm (dit_model.py:248-271): n = LayerNorm(x) is the residual base, m = n (1 + scale) + shift the GEMM operand"""
    n = bc.layer_norm(x, eps)
    return n, bc.modulate(n, bc.per_row(shift, rows_per_frame), bc.per_row(scale, rows_per_frame))


def ln_share_backward(x, shift, scale, dres, dm, rows_per_frame, eps=bc.EPS):
    """autograd of <dres, n> + <dm, m>: dres arrives over the residual path, dm from the GEMM that consumed m.  dm None: the final layer's
    LayerNorm (no modulation).  Returns dx, dshift, dscale (the last two None without dm)."""
    xx = x.clone().requires_grad_()
    if dm is None:
        (dx,) = torch.autograd.grad(bc.layer_norm(xx, eps), xx, dres)
        return dx, None, None
    sh, sc = shift.clone().requires_grad_(), scale.clone().requires_grad_()
    n, m = ln_share(xx, sh, sc, rows_per_frame, eps)
    return torch.autograd.grad((n, m), (xx, sh, sc), (dres, dm))


def rstd_of(x, eps=bc.EPS):
    return 1 / torch.sqrt(x.var(-1, unbiased=False) + eps)


def frames_to_rows(t):
    """[frames][C][L] -> [frames * L][C]: the value of every channel at a token row"""
    return t.permute(0, 2, 1).reshape(-1, t.shape[1])


def final_forward(x, w, b, frames, l, eps=bc.EPS):
    """dit1d_common's final layer on rows: x [frames * L][hidden] -> [frames][C][L]"""
    return bc.d1_final(x, w, b, 1, frames, l, eps)[0, :, :, 0, :]


def tok_embed_forward(x, w, b, pos, videos):
    """x [frames][C][L] -> rows [frames * L][hidden]; pos [n][hidden], n = frames / videos * L"""
    f, c, l = x.shape
    return bc.d1_tok_embed(x.reshape(videos, f // videos, c, l), w, b, pos)


def part_floats(rows, c, hidden, nb):
    return -(-rows // SUM_ROWS) * (c * hidden + nb)
