"""Restatements of the DiT / DiT1D block operations, one plain torch function each, for the op-level tests of the dfot_op_dit_* and
dfot_op_dit1d_* entry points.  Every formula is the reference module's own Python (modulate, LayerNorm without affine, PatchEmbed as a
Conv2d with kernel = stride = patch, tanh-GELU, the interleaved RoPE rotation, unpatchify, the DiT1D x_embedder and final_layer), written
on the tensors' own dtype: the tests evaluate it in float64 as the yardstick and once more in float32 to learn what fp32 arithmetic alone
costs on the same inputs.  Backward references are torch.autograd on these forwards; nothing here restates a gradient by hand."""
import math

import torch

EPS = 1e-6
# the widths the LayerNorm dispatch instantiates: hidden = 128 k for k = 1..10, 12, 16 and 64 k for k = 1, 3, 5, 7, 9
LN_WIDTHS = [128 * k for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16)] + [64 * k for k in (1, 3, 5, 7, 9)]
BF16_HALF_ULP = 2.0 ** -8   # round-to-nearest bf16: |bf16(v) - v| <= 2^-8 |v|
F32_ULP = 2.0 ** -24


def per_row(t, rows_per_frame):
    """[frames][n] -> [frames * rows_per_frame][n]: a frame's value for each of its rows"""
    return t.repeat_interleave(rows_per_frame, dim=0)


def modulate(x, shift, scale):
    return x * (1 + scale) + shift


def layer_norm(x, eps=EPS):
    """nn.LayerNorm(hidden, elementwise_affine=False, eps): biased variance over the last axis"""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps)


def ln_mod(x, shift, scale, rows_per_frame, eps=EPS):
    """x [rows][hidden], shift / scale [frames][hidden] -> modulate(LayerNorm(x), shift, scale)"""
    return modulate(layer_norm(x, eps), per_row(shift, rows_per_frame), per_row(scale, rows_per_frame))


def gate_combine(x, a, gate, rows_per_frame):
    """x + gate * a, gate [frames][hidden]"""
    return x + per_row(gate, rows_per_frame) * a


def gelu_tanh(x):
    """nn.GELU(approximate="tanh")"""
    return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))


def patchify(x, patch):
    """x [frames][c][h][w] -> [frames * gh * gw][c * patch * patch] in the Conv2d weight's own flattening (channel, py, px)"""
    f, c, h, w = x.shape
    gh, gw = h // patch, w // patch
    return x.reshape(f, c, gh, patch, gw, patch).permute(0, 2, 4, 1, 3, 5).reshape(f * gh * gw, c * patch * patch)


def patch_embed(x, w, b, patch, pos=None):
    """PatchEmbed: Conv2d(c, hidden, kernel = stride = patch) then 'b d gh gw -> (b gh gw) d'; w [hidden][c * patch * patch]; pos [gh * gw][hidden]"""
    out = patchify(x, patch) @ w.t() + b
    if pos is not None:
        out = out + pos.repeat(x.shape[0], 1)
    return out


def unpatchify(y, c, h, w, patch):
    """'b (h w) (p q c) -> b (h p) (w q) c' then channels first: y [frames * gh * gw][patch * patch * c] -> [frames][c][h][w]"""
    gh, gw = h // patch, w // patch
    f = y.shape[0] // (gh * gw)
    return y.reshape(f, gh, gw, patch, patch, c).permute(0, 5, 1, 3, 2, 4).reshape(f, c, h, w)


def rope_rotate(x, cos, sin):
    """x [..., d] in interleaved pairs, cos / sin [..., d / 2]: x * cos + rotate_half(x) * sin, rotate_half((x0, x1)) = (-x1, x0)"""
    x0, x1 = x[..., 0::2], x[..., 1::2]
    return torch.stack((x0 * cos - x1 * sin, x1 * cos + x0 * sin), -1).flatten(-2)


def qkv_pack(dq, dk, dv, d):
    """[b][heads][ntok][dstride] x 3 -> [b * ntok][3 * heads * d]: q | k | v, head-major, the first d of every dstride"""
    def flat(t):
        b, heads, ntok, _ = t.shape
        return t[..., :d].permute(0, 2, 1, 3).reshape(b * ntok, heads * d)
    return torch.cat((flat(dq), flat(dk), flat(dv)), 1)


def d1_tok_embed(x, w, b, pos):
    """x [B][T][C][L] -> 'b t c l -> b (t l) c', Linear(C, hidden), + pos_embed [T * L][hidden]; returns [B * T * L][hidden]"""
    bsz, t, c, l = x.shape
    tok = x.permute(0, 1, 3, 2).reshape(bsz, t * l, c)
    return (tok @ w.t() + b + pos).reshape(bsz * t * l, -1)


def d1_final(x, w, b, bsz, t, l, eps=EPS):
    """Sequential(LayerNorm, Linear(hidden, C)) then 'b (t l) c -> b t c l' and unsqueeze(-2): x [B * T * L][hidden] -> [B][T][C][1][L]"""
    y = layer_norm(x, eps) @ w.t() + b
    return y.reshape(bsz, t, l, -1).permute(0, 1, 3, 2).unsqueeze(-2)


# ---- bars -------------------------------------------------------------------------------------------------------------------
def errors(got, ref):
    ref = ref.detach()
    d = got.detach().double() - ref
    return float(d.abs().max()), float(d.norm() / ref.norm().clamp_min(1e-300))


def assert_fp32_within(name, got, ref64, ref32, factor=8.0):
    """fp32 outputs without a long sum: the kernel's error against float64 is at most `factor` times the error of the same formula
    evaluated by torch in float32 on the same inputs (max-abs and rel-L2).  Prints both."""
    k = errors(got, ref64)
    e = errors(ref32, ref64)
    print(f"{name}: kernel max-abs {k[0]:.3e} rel-L2 {k[1]:.3e} | torch fp32 max-abs {e[0]:.3e} rel-L2 {e[1]:.3e}")
    assert not bool(torch.isnan(got).any()), f"{name}: an element was not written"
    assert k[0] <= factor * e[0] and k[1] <= factor * e[1], (name, k, e)
    return k


def assert_bf16_of_fp32(name, got, ref64, slack):
    """bf16 outputs of an fp32 computation: every element within the half-ulp of round-to-nearest bf16 plus the fp32 allowance `slack`"""
    g = got.double()
    assert not bool(torch.isnan(g).any()), f"{name}: an element was not written"
    excess = (g - ref64).abs() - (BF16_HALF_ULP * ref64.abs() + slack)
    print(f"{name}: bf16 max |err| / (2^-8 |ref| + slack) = {float(((g - ref64).abs() / (BF16_HALF_ULP * ref64.abs() + slack)).max()):.3f}")
    assert float(excess.max()) <= 0.0, (name, float(excess.max()))


def assert_sum_bound(name, got, ref64, abs_terms, n_add):
    """fp32 sums: |got - ref64| <= (n_add + 4) * 2^-24 * sum |terms|, elementwise (abs_terms = the float64 sum of the terms' magnitudes)"""
    g = got.double()
    assert not bool(torch.isnan(g).any()), f"{name}: an element was not written"
    bound = (n_add + 4) * F32_ULP * abs_terms
    ratio = ((g - ref64).abs() / bound.clamp_min(1e-300)).max()
    k = errors(got, ref64)
    print(f"{name}: max-abs {k[0]:.3e} rel-L2 {k[1]:.3e}; max |err| / bound = {float(ratio):.3f} (N = {n_add})")
    assert bool(((g - ref64).abs() <= bound).all()), (name, float(ratio))
    return k


def bits(t):
    """integer view for bit-for-bit comparisons (NaN sentinels and signed zeros included)"""
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)
