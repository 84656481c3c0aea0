"""Shared helpers of tests/test_dit_mcraft_host.py, tests/test_gpu_dit_mcraft.py and tools/make_golden_dit_mcraft.py (not a test module):
the Minecraft / dmlab recipe's geometry -- latents (32, 8, 8), patch 2 (a 128-wide patch vector, 16 patches per frame), max_tokens 16,
DiT3D "full" / rope_3d under continuous diffusion, actions of dim 4 with dropout 0.1.

  * FIX               the fixture's model (hidden 384, depth 2, 6 heads: a 196 KB final weight, the smallest width past the LDS-resident
                      final-layer kernel); ocfg(**over) other widths of the same geometry
  * seeded_params     oracle.dit.seeded_params + the Fourier buffers (+ seeded condition-embedding tensors, drawn exactly as
                      tools/make_golden_dit_cond.cond_params draws them for the reference module's keys)
  * forward           the continuous restatement (dit_cont_common.forward_dit) with the action embedding added per frame and dropped per
                      masked video, as the reference's RandomDropoutCondEmbedding does in eval mode
"""
import math

import torch

import dit_cont_common as cc
from dit_cond_common import T, load, rel  # noqa: F401

X_SHAPE = (32, 8, 8)
PATCH = 2
MAX_TOKENS = 16
COND_DIM = 4
DROPOUT = 0.1
FIX = dict(hidden_size=384, depth=2, num_heads=6)
COND = "external_cond_embedding.embedding"
COND_KEYS = ("linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias")


def ocfg(**over):
    from oracle import dit as odit
    kw = dict(FIX, **over)
    return odit.DiTConfig(patch_size=PATCH, in_channels=X_SHAPE[0], resolution=X_SHAPE[1:], max_tokens=MAX_TOKENS, **kw)


def backbone_cfg(cfg, dropout=0.0):
    out = cc.cont(dict(name="dit3d", variant="full", pos_emb_type="rope_3d", patch_size=PATCH, hidden_size=cfg.hidden_size, depth=cfg.depth,
                       num_heads=cfg.num_heads, mlp_ratio=4.0))
    if dropout:
        out["external_cond_dropout"] = dropout
    return out


def cond_seeded(hidden, dim=COND_DIM, seed=12):
    """the draws of tools/make_golden_dit_cond.cond_params for TimestepEmbedding(dim -> hidden -> hidden), in state-dict order"""
    g = torch.Generator().manual_seed(seed)
    shapes = {"linear_1.weight": (hidden, dim), "linear_1.bias": (hidden,), "linear_2.weight": (hidden, hidden), "linear_2.bias": (hidden,)}
    out = {}
    for k in COND_KEYS:
        s = shapes[k]
        out[f"{COND}.{k}"] = 0.05 * torch.randn(s, generator=g) if k.endswith(".bias") else torch.randn(s, generator=g) / math.sqrt(s[1])
    return out


def seeded_params(cfg, action=False, names=None):
    """names: a state-dict key order to return the tensors in (the reference module's, or the engine's)"""
    from oracle import dit as odit
    p = cc.with_buffers(odit.seeded_params(cfg, 4), 2)
    if action:
        p.update(cond_seeded(cfg.hidden_size))
    if names is not None:
        assert sorted(names) == sorted(p), sorted(set(names) ^ set(p))[:4]
        p = {n: p[n] for n in names}
    return p


def forward(params, cfg, x, levels, cond=None, mask=None, dtype=torch.float32):
    """eval forward: emb = Fourier embedding (+ action embedding, zeroed for the videos of `mask`)"""
    from oracle import dit as odit
    import torch.nn.functional as F

    def emb(p, _cfg, k):
        e = cc.fourier_embedding(p, k, dtype)
        if cond is not None:
            w = lambda n: p[f"{COND}.{n}"].to(dtype)
            ce = F.linear(F.silu(F.linear(cond.to(dtype), w("linear_1.weight"), w("linear_1.bias"))), w("linear_2.weight"), w("linear_2.bias"))
            if mask is not None:
                ce = ce * (~mask.bool()).to(dtype)[:, None, None]
            e = e + ce
        return e
    keep = odit.noise_level_embedding
    odit.noise_level_embedding = emb
    try:
        p = {k: (v if k in (cc.FREQS, cc.PHASES) else v.to(dtype)) for k, v in params.items()}
        return odit.forward(p, cfg, x.to(dtype), levels)
    finally:
        odit.noise_level_embedding = keep


def final_layer_fp64(x, mod, w, b, channels, height, width, patch, eps=1e-6):
    """float64 restatement of the DiT final layer (oracle.dit.forward's last four lines): x [rows][hidden], mod [frames][2 * hidden] =
    (shift | scale) of each frame, w [patch * patch * channels][hidden], b -> [frames][channels][height][width]"""
    import torch.nn.functional as F
    x, mod, w, b = x.double(), mod.double(), w.double(), b.double()
    frames, hidden = mod.shape[0], x.shape[1]
    gh, gw = height // patch, width // patch
    shift, scale = mod[:, None, :hidden], mod[:, None, hidden:]
    m = F.layer_norm(x, (hidden,), None, None, eps).reshape(frames, gh * gw, hidden) * (1 + scale) + shift
    out = F.linear(m, w, b).reshape(frames, gh, gw, patch, patch, channels).permute(0, 1, 3, 2, 4, 5).reshape(frames, height, width, channels)
    return out.permute(0, 3, 1, 2).contiguous()
