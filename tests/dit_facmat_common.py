"""Shared helpers of tests/test_dit_facmat_host.py, tests/test_gpu_dit_facmat.py and tools/make_golden_dit_facmat.py (not a test module):
the FacMatDiT backbone, DiT3D with variant "factorized_matrix_attention", pos_emb_type "sinusoidal_2d" and use_temporal_rope.

  * key_shapes        the reference module's state-dict keys and shapes, in its registration order
  * seeded_params     weights drawn per key from a seed derived from the key's name and shape (so a fixture stores a digest, not tensors)
  * forward_host      a torch restatement of the forward in any float dtype (fp32 / fp64), citing the reference lines it restates
  * matrix_attention_ref   the matrix attention core alone on a (q|k|v) matrix in the engine's layout (the op-level fp64 reference)
"""
import hashlib
import math

import torch
import torch.nn.functional as F

from dit_fac_common import COND_DIM, COND_DROPOUT, EPS, NOISE_DIM, T, _ada_ln, _dit_block, digest, load, rel, spatial_table  # noqa: F401

# the tiny configuration of the fixture: embed_row_dim 128, embed_col_dim 64, depth 2, 4 spatial heads, patch 1, latents 4x16x8 (P = 128),
# max_tokens 5, mlp_ratio 4 in the matrix blocks
TINY = dict(hidden_size=128, embed_col_dim=64, depth=2, num_heads=4, patch_size=1, in_channels=4, resolution=(16, 8), max_tokens=5,
            mlp_ratio=4.0)
ROPE_THETA = 10000.0

# the models of the fixture: tag -> (num_col_heads, num_row_heads, use_bias, spatial_mlp_ratio, use_temporal_rope).  Every value of every
# key occurs with and without the rotation; "a" is also the model of the conditioned case, the frame-coupling case and the sampler trace
CASES = {
    "a": (1, 4, False, 0.0, True),
    "b": (2, 2, True, 4.0, True),
    "c": (1, 4, True, 0.0, False),
    "d": (2, 2, False, 4.0, False),
}


def backbone_cfg(cc, rr, use_bias, spatial_mlp_ratio, rope, dropout=0.0, **over):
    c = {**TINY, **over}
    cfg = dict(name="dit3d", variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", use_temporal_rope=rope,
               patch_size=c["patch_size"], hidden_size=None, embed_col_dim=c["embed_col_dim"], embed_row_dim=c["hidden_size"],
               num_heads=c["num_heads"], num_col_heads=cc, num_row_heads=rr, depth=c["depth"], mlp_ratio=c["mlp_ratio"],
               spatial_mlp_ratio=spatial_mlp_ratio, use_bias=use_bias, matrix_block="matrix", flatten_matrix_rope=False,
               matrix_multi_token=False, fixed_u=None, use_gradient_checkpointing=False)
    if dropout:
        cfg["external_cond_dropout"] = dropout
    return cfg


def key_shapes(use_bias, spatial_mlp_ratio, cond_dim=0, cond_dropout=0.0, **over):
    """[(state-dict key, shape)] in the order the reference's DiT3D registers them (dit3d.py:45-83 -> base_backbone.py:35-62 for the two
    embeddings, then patch_embedder, then DiTBase: blocks (DiTBlock), temporal_blocks (MatrixDiTBlock: norm1, attn.qkv_u / proj_u / qkv_v /
    proj_v [/ qkv_bias / proj_bias], norm2, mlp), final_layer -- dit_base.py:156-228, dit_blocks.py:266-287, 579-601).  The RoPE table is a
    non-persistent buffer and has no key."""
    c = {**TINY, **over}
    h, e, ps, ch = c["hidden_size"], c["embed_col_dim"], c["patch_size"], c["in_channels"]
    pn = (c["resolution"][0] // ps) * (c["resolution"][1] // ps)
    out = []

    def linear(name, o, i):
        out.extend([(f"{name}.weight", (o, i)), (f"{name}.bias", (o,))])
    linear("noise_level_pos_embedding.embedding.linear_1", h, NOISE_DIM)
    linear("noise_level_pos_embedding.embedding.linear_2", h, h)
    if cond_dim:
        pre = "external_cond_embedding" + (".embedding" if cond_dropout > 0 else "")
        linear(f"{pre}.linear_1", h, cond_dim)
        linear(f"{pre}.linear_2", h, h)
    out.extend([("patch_embedder.proj.weight", (h, ch, ps, ps)), ("patch_embedder.proj.bias", (h,))])

    def mlp(pre, ratio):
        if ratio:
            linear(f"{pre}.norm2.modulation.1", 3 * h, h)
            linear(f"{pre}.mlp.fc1", int(h * ratio), h)
            linear(f"{pre}.mlp.fc2", h, int(h * ratio))
    for i in range(c["depth"]):
        pre = f"dit_base.blocks.{i}"
        linear(f"{pre}.norm1.modulation.1", 3 * h, h)
        linear(f"{pre}.attn.qkv", 3 * h, h)
        linear(f"{pre}.attn.proj", h, h)
        mlp(pre, spatial_mlp_ratio)
    for i in range(c["depth"]):
        pre = f"dit_base.temporal_blocks.{i}"
        linear(f"{pre}.norm1.modulation.1", 3 * h, h)
        out.extend([(f"{pre}.attn.qkv_u", (pn, e)), (f"{pre}.attn.proj_u", (e, pn)), (f"{pre}.attn.qkv_v", (h, 3 * h)),
                    (f"{pre}.attn.proj_v", (h, h))])
        if use_bias:
            out.extend([(f"{pre}.attn.qkv_bias", (e, 3 * h)), (f"{pre}.attn.proj_bias", (pn, h))])
        mlp(pre, c["mlp_ratio"])
    linear("dit_base.final_layer.norm_final.modulation.1", 2 * h, h)
    linear("dit_base.final_layer.linear", ps * ps * ch, h)
    return out


def seeded_params(keys):
    """every tensor from its own generator, seeded by sha256(name, shape): biases (the matrix biases included) ~ N(0, 0.05^2), weights ~
    N(0, 1/fan_in) -- the matrix factors are stored (in, out), fan-in = rows -- modulation weights at half gain.  Nothing is zero: the
    reference's zero-initialised modulations and final projection would hide the blocks."""
    out = {}
    for name, shape in keys:
        seed = int.from_bytes(hashlib.sha256(f"{name}{tuple(shape)}".encode()).digest()[:7], "little")
        g = torch.Generator().manual_seed(seed)
        leaf = name.rsplit(".", 1)[-1]
        if leaf in ("bias", "qkv_bias", "proj_bias"):
            out[name] = 0.05 * torch.randn(shape, generator=g)
        elif leaf in ("qkv_u", "proj_u", "qkv_v", "proj_v"):
            out[name] = torch.randn(shape, generator=g) / math.sqrt(shape[0])
        else:
            gain = 0.5 if ".modulation." in name else 1.0
            out[name] = gain * torch.randn(shape, generator=g) / math.sqrt(math.prod(shape[1:]))
    return out


def rope_angles(tokens, dim, dtype=torch.float32, device="cpu"):
    """RotaryEmbeddingND.get_freqs for one axis (embeddings.py:193-202): angle[t][2i] = angle[t][2i+1] = t * theta^(-2i/dim); the reference
    evaluates it in fp32, the op-level fp64 reference passes dtype=torch.float64"""
    freqs = 1.0 / (ROPE_THETA ** (torch.arange(0, dim, 2, device=device)[: dim // 2].to(dtype) / dim))
    return (torch.arange(tokens, dtype=dtype, device=device)[:, None] * freqs[None]).repeat_interleave(2, dim=-1)  # [tokens][dim]


def rope_table(tokens, dim):
    """the engine's table for dfot_op_matrix_attention_rope: fp32 [tokens][dim/2][2] = (cos, sin), from float64 angles"""
    ang = rope_angles(tokens, dim, torch.float64)[:, 0::2]
    return torch.stack([ang.cos(), ang.sin()], -1).float().contiguous()


def rotate(x, ang):
    """RotaryEmbeddingND.forward (embeddings.py:204-215) on [..., l, n, d] with ang [l][d]: x cos + rotate_half(x) sin, rotate_half on
    interleaved pairs (x1, x2) -> (-x2, x1)"""
    x2 = x.reshape(*x.shape[:-1], -1, 2)
    half = torch.stack((-x2[..., 1], x2[..., 0]), dim=-1).flatten(-2)
    return x * ang.cos()[:, None, :] + half * ang.sin()[:, None, :]


def matrix_attention_core(qkv, cc, rr, rope, rope_dtype=torch.float32):
    """MatrixAttention.forward between the two factor products (dit_blocks.py:308-342, multi_token False): qkv [b, l, E, 3h] -> [b, l, E, h]"""
    b, l, e, h3 = qkv.shape
    h = h3 // 3
    hn, hd = e // cc, h // rr
    q, k, v = qkv.reshape(b, l, cc, hn, 3, rr, hd).permute(4, 0, 2, 5, 1, 3, 6)  # k b c r l n d
    if rope:
        ang = rope_angles(l, hd, rope_dtype, qkv.device).to(qkv.dtype)
        q, k = rotate(q, ang), rotate(k, ang)
    w = torch.softmax(torch.einsum("bcrlnd,bcrknd->bcrlk", q * (hn * hd) ** -0.5, k), dim=-1)
    o = torch.einsum("bcrlk,bcrknd->bcrlnd", w, v)
    return o.permute(0, 3, 1, 4, 2, 5).reshape(b, l, e, h), w  # b l (c n) (r d)


def matrix_attention_ref(z, batch, tokens, e, h, cc, rr, rope):
    """fp64 reference of the op: z [batch*tokens*e][3h] (any float dtype, used as given) -> (o [batch*tokens*e][h], probabilities)"""
    o, w = matrix_attention_core(z.double().reshape(batch, tokens, e, 3 * h), cc, rr, rope, torch.float64)
    return o.reshape(batch * tokens * e, h), w


# the op-level cases of tests/test_gpu_dit_facmat.py: E = 64, (num_col_heads, num_row_heads, h) -> hd in {32, 64, 72}, hn in {64, 32}
OP_E = 64
OP_HEADS = [(1, 4, 128), (2, 2, 128), (1, 2, 144)]
OP_TOKENS = [1, 2, 3, 5, 10, 16, 17, 32]


def make_z(batch, tokens, cc, rr, h, seed=0):
    """(q|k|v) [batch*tokens*E][3h], unit normal and rounded to bf16 (returned as fp32): with scale = (hn*hd)^-1/2 the scores have unit
    variance, so the softmax over 2 .. 32 frames is neither flat nor one-hot"""
    g = torch.Generator().manual_seed(seed + 1000 * tokens + 10 * h + cc)
    return torch.randn(batch * tokens * OP_E, 3 * h, generator=g).to(torch.bfloat16).float()


def _matrix_block(p, pre, x, c, b, t, cc, rr, rope, has_mlp):
    """MatrixDiTBlock on (b t) p c (dit_blocks.py:626-652): x, gate = norm1(x, c); x = x + gate * attn(x as b t p c)"""
    m, gate = _ada_ln(p, f"{pre}.norm1", x, c, 3)
    pn, h = m.shape[1:]
    qkv = torch.einsum("nm,blnd,dk->blmk", p[f"{pre}.attn.qkv_u"], m.reshape(b, t, pn, h), p[f"{pre}.attn.qkv_v"])  # matrix_mul
    if f"{pre}.attn.qkv_bias" in p:
        qkv = qkv + p[f"{pre}.attn.qkv_bias"]
    o, _ = matrix_attention_core(qkv, cc, rr, rope)
    a = torch.einsum("nm,blnd,dk->blmk", p[f"{pre}.attn.proj_u"], o, p[f"{pre}.attn.proj_v"])
    if f"{pre}.attn.proj_bias" in p:
        a = a + p[f"{pre}.attn.proj_bias"]
    x = m + gate * a.reshape(b * t, pn, h)
    if has_mlp:
        m, gate = _ada_ln(p, f"{pre}.norm2", x, c, 3)
        hid = F.gelu(F.linear(m, p[f"{pre}.mlp.fc1.weight"], p[f"{pre}.mlp.fc1.bias"]), approximate="tanh")
        x = m + gate * F.linear(hid, p[f"{pre}.mlp.fc2.weight"], p[f"{pre}.mlp.fc2.bias"])
    return x


def forward_host(params, x, k, cc, rr, rope, cond=None, mask=None, dtype=torch.float64, **over):
    """DiT3D.forward (dit3d.py:153-192) with DiTBase variant "factorized_matrix_attention", sinusoidal_2d (dit_base.py:356-362, 389-419).
    x [B,T,C,H,W], k [B,T] integer levels, cond [B,T,cond_dim] actions or None, mask [B] bool (videos that run without the condition)."""
    c = {**TINY, **over}
    p = {n: t.to(device=x.device, dtype=dtype) for n, t in params.items()}
    b, t, ch, hh, ww = x.shape
    ps, h, heads = c["patch_size"], c["hidden_size"], c["num_heads"]
    gh, gw = hh // ps, ww // ps
    pn = gh * gw
    x = x.to(dtype)
    half = NOISE_DIM // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32, device=x.device) / half)
    a = (k[..., None].float() * freqs).to(dtype)
    pre = "noise_level_pos_embedding.embedding"
    emb = F.linear(F.silu(F.linear(torch.cat([a.cos(), a.sin()], -1), p[f"{pre}.linear_1.weight"], p[f"{pre}.linear_1.bias"])),
                   p[f"{pre}.linear_2.weight"], p[f"{pre}.linear_2.bias"])  # [B,T,h]
    if cond is not None:  # emb + external_cond_embedding(cond, mask) (dit3d.py:170-175; embeddings.py:364-387: masked videos get zeros)
        pre = next(n for n in p if n.startswith("external_cond_embedding")).rsplit(".linear_1", 1)[0]
        ce = F.linear(F.silu(F.linear(cond.to(dtype), p[f"{pre}.linear_1.weight"], p[f"{pre}.linear_1.bias"])),
                      p[f"{pre}.linear_2.weight"], p[f"{pre}.linear_2.bias"])
        if mask is not None:
            ce = ce * (~mask.to(ce.device))[:, None, None].to(dtype)
        emb = emb + ce
    tok = F.conv2d(x.reshape(b * t, ch, hh, ww), p["patch_embedder.proj.weight"], p["patch_embedder.proj.bias"], stride=ps)
    tok = tok.flatten(2).transpose(1, 2) + spatial_table((gh, gw), h).to(x.device, dtype)[None]  # (B*T, P, h)  dit_base.py:356-362
    cs = emb.reshape(b * t, 1, h).expand(b * t, pn, h)
    for i in range(c["depth"]):
        tok = _dit_block(p, f"dit_base.blocks.{i}", tok, cs, heads, f"dit_base.blocks.{i}.mlp.fc1.weight" in p)  # dit_base.py:392-394
        tok = _matrix_block(p, f"dit_base.temporal_blocks.{i}", tok, cs, b, t, cc, rr, rope,                    # dit_base.py:397-406
                            f"dit_base.temporal_blocks.{i}.mlp.fc1.weight" in p)
    tok = _ada_ln(p, "dit_base.final_layer.norm_final", tok, cs, 2)
    out = F.linear(tok, p["dit_base.final_layer.linear.weight"], p["dit_base.final_layer.linear.bias"])
    out = out.reshape(b * t, gh, gw, ps, ps, ch).permute(0, 1, 3, 2, 4, 5).reshape(b * t, gh * ps, gw * ps, ch)  # dit3d.py:137-151
    return out.permute(0, 3, 1, 2).reshape(b, t, ch, hh, ww)


def case_params(tag, cond=False):
    cc, rr, bias, ratio, rope = CASES[tag]
    return seeded_params(key_shapes(bias, ratio, COND_DIM if cond else 0, COND_DROPOUT if cond else 0.0))


def build(tag, cond=False):
    """the engine's DiT3D at a fixture case with the seeded weights, eval() as the reference's module was"""
    import dfot_amd
    cc, rr, bias, ratio, rope = CASES[tag]
    kw = dict(external_cond_type="action", external_cond_dim=COND_DIM) if cond else {}
    params = case_params(tag, cond)
    model = dfot_amd.DiT3D(backbone_cfg(cc, rr, bias, ratio, rope, COND_DROPOUT if cond else 0.0), x_shape=(4, 16, 8), max_tokens=5, **kw).cuda().eval()
    model.load_state_dict(params, strict=True)
    return model, params
