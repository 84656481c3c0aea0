"""Shared helpers of tests/test_dit_fac_host.py, tests/test_gpu_dit_fac.py and tools/make_golden_dit_fac.py (not a test module): the
factorized-attention DiT3D (variant "factorized_attention", pos_emb_type "sinusoidal_factorized").

  * key_shapes        the reference module's state-dict keys and shapes, in its registration order
  * seeded_params     weights drawn per key from a seed derived from the key's name and shape (so a fixture stores a digest, not tensors)
  * forward_host      a torch restatement of the forward in any float dtype (fp32 / fp64), citing the reference lines it restates
"""
import hashlib
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the tiny configuration of the fixture: hidden 128, depth 2, 4 heads, patch 1, latents 4x16x8 (P = 128), max_tokens 5
TINY = dict(hidden_size=128, depth=2, num_heads=4, patch_size=1, in_channels=4, resolution=(16, 8), max_tokens=5, mlp_ratio=4.0)
NOISE_DIM = 256
EPS = 1e-6
COND_DIM, COND_DROPOUT = 3, 0.1  # the conditioned case of the fixture


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def backbone_cfg(spatial_mlp_ratio, dropout=0.0, **over):
    c = {**TINY, **over}
    cfg = dict(name="dit3d", variant="factorized_attention", pos_emb_type="sinusoidal_factorized", patch_size=c["patch_size"],
               hidden_size=c["hidden_size"], depth=c["depth"], num_heads=c["num_heads"], mlp_ratio=c["mlp_ratio"],
               spatial_mlp_ratio=spatial_mlp_ratio, use_gradient_checkpointing=False)
    if dropout:
        cfg["external_cond_dropout"] = dropout
    return cfg


def key_shapes(spatial_mlp_ratio, cond_dim=0, cond_dropout=0.0, **over):
    """[(state-dict key, shape)] in the order the reference's DiT3D registers them (dit3d.py:45-83 -> base_backbone.py:35-62 for the two
    embeddings, then patch_embedder, then DiTBase: blocks, temporal_blocks, final_layer -- dit_base.py:156-228)"""
    c = {**TINY, **over}
    h, ps, ch = c["hidden_size"], c["patch_size"], c["in_channels"]
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

    def block(pre, ratio):
        linear(f"{pre}.norm1.modulation.1", 3 * h, h)
        linear(f"{pre}.attn.qkv", 3 * h, h)
        linear(f"{pre}.attn.proj", h, h)
        if ratio:
            linear(f"{pre}.norm2.modulation.1", 3 * h, h)
            linear(f"{pre}.mlp.fc1", int(h * ratio), h)
            linear(f"{pre}.mlp.fc2", h, int(h * ratio))
    for i in range(c["depth"]):
        block(f"dit_base.blocks.{i}", spatial_mlp_ratio)
    for i in range(c["depth"]):
        block(f"dit_base.temporal_blocks.{i}", c["mlp_ratio"])
    linear("dit_base.final_layer.norm_final.modulation.1", 2 * h, h)
    linear("dit_base.final_layer.linear", ps * ps * ch, h)
    return out


def seeded_params(keys):
    """every tensor from its own generator, seeded by sha256(name, shape): biases ~ N(0, 0.05^2), weights ~ N(0, 1/fan_in), modulation
    weights at half gain.  Nothing is zero: the reference's zero-initialised modulations and final projection would hide both blocks."""
    out = {}
    for name, shape in keys:
        seed = int.from_bytes(hashlib.sha256(f"{name}{tuple(shape)}".encode()).digest()[:7], "little")
        g = torch.Generator().manual_seed(seed)
        if name.endswith(".bias"):
            out[name] = 0.05 * torch.randn(shape, generator=g)
        else:
            gain = 0.5 if ".modulation." in name else 1.0
            out[name] = gain * torch.randn(shape, generator=g) / math.sqrt(math.prod(shape[1:]))
    return out


def digest(params):
    h = hashlib.sha256()
    for k in params:
        h.update(k.encode())
        h.update(params[k].contiguous().numpy().tobytes())
    return h.hexdigest()


def sincos_1d(embed_dim, pos):
    """get_1d_sincos_pos_embed_from_grid (dit_base.py:552-572): [sin | cos] of pos * 10000^(-i / (embed_dim / 2)), float64"""
    omega = 1.0 / 10000 ** (np.arange(embed_dim // 2, dtype=np.float64) / (embed_dim / 2.0))
    ang = np.einsum("m,d->md", np.asarray(pos, dtype=np.float32).reshape(-1), omega)
    return np.concatenate([np.sin(ang), np.cos(ang)], axis=1)


def temporal_table(max_tokens, hidden):
    """SinusoidalPositionalEmbedding(hidden, (max_tokens,)) (dit_base.py:268-271, 528-549): one axis, all channels"""
    return torch.from_numpy(sincos_1d(hidden, np.arange(max_tokens))).float()


def spatial_table(grid, hidden):
    """SinusoidalPositionalEmbedding(hidden, grid) (dit_base.py:264-267): np.meshgrid's default "xy" indexing -> flattened entry m takes
    position m % grid[0] for the first half of the channels and m // grid[0] for the second"""
    m = np.arange(grid[0] * grid[1])
    return torch.from_numpy(np.concatenate([sincos_1d(hidden // 2, m % grid[0]), sincos_1d(hidden // 2, m // grid[0])], axis=1)).float()


def _ada_ln(p, pre, x, c, chunks):
    """AdaLayerNormZero / the final AdaLN (dit_blocks.py:378-405, 512-542): LayerNorm(x) * (1 + scale) + shift [, gate]"""
    mod = F.linear(F.silu(c), p[f"{pre}.modulation.1.weight"], p[f"{pre}.modulation.1.bias"]).chunk(chunks, dim=-1)
    m = F.layer_norm(x, x.shape[-1:], None, None, EPS) * (1 + mod[1]) + mod[0]
    return (m, mod[2]) if chunks == 3 else m


def _dit_block(p, pre, x, c, heads, has_mlp):
    """DiTBlock on (sequences, tokens, C) without RoPE (dit_blocks.py:408-470): x, gate = norm(x, c); x = x + gate * f(x)"""
    m, gate = _ada_ln(p, f"{pre}.norm1", x, c, 3)
    s, n, ch = m.shape
    d = ch // heads
    qkv = F.linear(m, p[f"{pre}.attn.qkv.weight"], p[f"{pre}.attn.qkv.bias"]).reshape(s, n, 3, heads, d).permute(2, 0, 3, 1, 4)
    w = torch.softmax(qkv[0] @ qkv[1].transpose(-2, -1) / math.sqrt(d), dim=-1)
    o = (w @ qkv[2]).transpose(1, 2).reshape(s, n, ch)
    x = m + gate * F.linear(o, p[f"{pre}.attn.proj.weight"], p[f"{pre}.attn.proj.bias"])
    if has_mlp:
        m, gate = _ada_ln(p, f"{pre}.norm2", x, c, 3)
        hid = F.gelu(F.linear(m, p[f"{pre}.mlp.fc1.weight"], p[f"{pre}.mlp.fc1.bias"]), approximate="tanh")
        x = m + gate * F.linear(hid, p[f"{pre}.mlp.fc2.weight"], p[f"{pre}.mlp.fc2.bias"])
    return x


def forward_host(params, x, k, cond=None, mask=None, dtype=torch.float64, **over):
    """DiT3D.forward (dit3d.py:146-192) with DiTBase variant "factorized_attention", sinusoidal_factorized (dit_base.py:364-417).
    x [B,T,C,H,W], k [B,T] integer levels, cond [B,T,cond_dim] actions or None, mask [B] bool (videos that run without the condition)."""
    c = {**TINY, **over}
    p = {n: t.to(device=x.device, dtype=dtype) for n, t in params.items()}
    b, t, ch, hh, ww = x.shape
    ps, h, heads = c["patch_size"], c["hidden_size"], c["num_heads"]
    gh, gw = hh // ps, ww // ps
    pn = gh * gw
    x = x.to(dtype)
    # noise-level embedding: Timesteps(256, flip_sin_to_cos=True, downscale_freq_shift=0) -> Linear -> SiLU -> Linear (embeddings.py)
    half = NOISE_DIM // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32, device=x.device) / half)
    a = (k[..., None].float() * freqs).to(dtype)
    pre = "noise_level_pos_embedding.embedding"
    emb = F.linear(F.silu(F.linear(torch.cat([a.cos(), a.sin()], -1), p[f"{pre}.linear_1.weight"], p[f"{pre}.linear_1.bias"])),
                   p[f"{pre}.linear_2.weight"], p[f"{pre}.linear_2.bias"])  # [B,T,h]
    if cond is not None:  # emb + external_cond_embedding(cond, mask) (dit3d.py:171-173; embeddings.py:364-387: masked videos get zeros)
        pre = next(n for n in p if n.startswith("external_cond_embedding")).rsplit(".linear_1", 1)[0]
        ce = F.linear(F.silu(F.linear(cond.to(dtype), p[f"{pre}.linear_1.weight"], p[f"{pre}.linear_1.bias"])),
                      p[f"{pre}.linear_2.weight"], p[f"{pre}.linear_2.bias"])
        if mask is not None:
            ce = ce * (~mask.to(ce.device))[:, None, None].to(dtype)
        emb = emb + ce
    tok = F.conv2d(x.reshape(b * t, ch, hh, ww), p["patch_embedder.proj.weight"], p["patch_embedder.proj.bias"], stride=ps)
    tok = tok.flatten(2).transpose(1, 2) + spatial_table((gh, gw), h).to(x.device, dtype)[None]  # (B*T, P, h)  dit_base.py:366-372
    cs = emb.reshape(b * t, 1, h).expand(b * t, pn, h)  # the conditioning of a token is its frame's, on either axis
    ct = cs.reshape(b, t, pn, h).transpose(1, 2).reshape(b * pn, t, h)
    tpos = temporal_table(c["max_tokens"], h).to(x.device, dtype)[None, :t]
    for i in range(c["depth"]):
        tok = _dit_block(p, f"dit_base.blocks.{i}", tok, cs, heads, f"dit_base.blocks.{i}.mlp.fc1.weight" in p)  # dit_base.py:391-393
        tok = tok.reshape(b, t, pn, h).transpose(1, 2).reshape(b * pn, t, h)  # "(b t) p c -> (b p) t c"        dit_base.py:405-406
        if i == 0:
            tok = tok + tpos  # temporal_pos_emb after the first spatial block                                   dit_base.py:407-408
        tok = _dit_block(p, f"dit_base.temporal_blocks.{i}", tok, ct, heads, f"dit_base.temporal_blocks.{i}.mlp.fc1.weight" in p)
        tok = tok.reshape(b, pn, t, h).transpose(1, 2).reshape(b * t, pn, h)  # "(b p) t c -> (b t) p c"        dit_base.py:411
    tok = _ada_ln(p, "dit_base.final_layer.norm_final", tok, cs, 2)
    out = F.linear(tok, p["dit_base.final_layer.linear.weight"], p["dit_base.final_layer.linear.bias"])
    out = out.reshape(b * t, gh, gw, ps, ps, ch).permute(0, 1, 3, 2, 4, 5).reshape(b * t, gh * ps, gw * ps, ch)  # dit3d.py:129-144
    return out.permute(0, 3, 1, 2).reshape(b, t, ch, hh, ww)


def build(spatial_mlp_ratio, cond=False):
    """the engine's DiT3D at the fixture's configuration with the seeded weights, eval() as the reference's module was"""
    import dfot_amd
    kw = dict(external_cond_type="action", external_cond_dim=COND_DIM) if cond else {}
    keys = key_shapes(spatial_mlp_ratio, COND_DIM if cond else 0, COND_DROPOUT if cond else 0.0)
    params = seeded_params(keys)
    model = dfot_amd.DiT3D(backbone_cfg(spatial_mlp_ratio, COND_DROPOUT if cond else 0.0), x_shape=(4, 16, 8), max_tokens=5, **kw).cuda().eval()
    model.load_state_dict(params, strict=True)
    return model, params
