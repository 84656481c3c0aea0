"""Shared helpers of tests/test_titok_enc_host.py, tests/test_gpu_titok_enc.py and tests/test_gpu_titok_enc_ops.py (not a test module): the
encoder half of TiTok_KL, the 1-D token autoencoder of the taichi recipes (frames -> 32 latent tokens of 4 channels).

  * CASES / config     the three configurations of tests/golden/titok_enc.npz (tools/make_golden_titok_enc.py)
  * seeded_params      the fixture's encoder weights, re-created from the stored key names and shapes (oracle.vae.seeded_tensor, with the q / k
                       rows of every in_proj_weight and patch_embed.weight multiplied by the gains the file records: see the tool's docstring)
  * inputs             the fixture's frames, re-drawn from the stored seeds and checked against the stored sum and sampled values
  * moments / encode   an fp32 (any float dtype) torch restatement, functional over a state dict with the reference's key names:
        TiTokEncoder.forward                  algorithms/vae/tiktok_kl/blocks_kl.py:140-166  (the blocks are titok_common.attention_block)
        TiTok_KL.encode                       algorithms/vae/tiktok_kl/titok_kl.py:78-98
        DiagonalGaussianDistribution          algorithms/vae/common/distribution.py
    `reading="transpose"` is the WRONG reading of the reference's `reshape(batch, width, num_latent_tokens, 1)` (a permute), kept so that
    the tests can show the fixture tells the two apart.
"""
import ast
import os

import numpy as np
import torch
import torch.nn.functional as F

import titok_common as tc
from oracle import vae as ovae

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = tc.CASES
PRESETS = tc.PRESETS
T, rel = tc.T, tc.rel


def config(case):
    c = CASES[case]
    return dict(image_size=c["image_size"], token_size=4, vit_enc_model_size=c["size"], vit_enc_patch_size=16, num_latent_tokens=32)


def load():
    with np.load(os.path.join(GOLDEN, "titok_enc.npz")) as g:
        return {k: g[k] for k in g.files}


def key_shapes(g, case):
    return {str(n): ast.literal_eval(str(s)) for n, s in zip(g[f"names_{case}"], g[f"shapes_{case}"])}


def seeded_tensor(name, shape, qk_gain, patch_gain):
    t = ovae.seeded_tensor(name, shape)
    if name.startswith("encoder.transformer.") and name.endswith(".attn.in_proj_weight"):
        t = t.clone()
        t[: 2 * t.shape[1]] *= qk_gain
    elif name == "encoder.patch_embed.weight":
        t = t * patch_gain
    return t


def seeded_params(g, case):
    qk, pe = float(g["qk_gain"]), float(g["patch_gain"])
    return {n: seeded_tensor(n, s, qk, pe) for n, s in key_shapes(g, case).items()}


def inputs(g, case, tag="x"):
    """the fixture's frames (`x`) or its second, independent input (`x2`): re-drawn, and checked against what the file records"""
    c = CASES[case]
    x = torch.rand(c["frames"], 3, c["image_size"], c["image_size"], generator=torch.Generator().manual_seed(int(g[f"{tag}_seed_{case}"])))
    flat = x.reshape(-1)
    idx = torch.linspace(0, flat.numel() - 1, 8).long()
    assert np.array_equal(flat[idx].numpy(), g[f"{tag}_probe_{case}"]), "torch.rand no longer draws the fixture's input"
    assert abs(float(flat.double().sum()) - float(g[f"{tag}_sum_{case}"])) <= 1e-9 * flat.numel()
    return x


def moments(p, cfg, x, reading="reshape"):
    """TiTokEncoder.forward: frames (F, 3, S, S) -> moments (F, 2 * token_size, 1, num_latent)"""
    width, layers, heads = PRESETS[cfg["vit_enc_model_size"]]
    nlat, ts = cfg["num_latent_tokens"], cfg["token_size"]
    n = x.shape[0]
    h = F.conv2d(x, p["encoder.patch_embed.weight"], p["encoder.patch_embed.bias"], stride=16)
    h = h.reshape(n, width, -1).permute(0, 2, 1)                                           # (F, grid^2, C)
    h = torch.cat([p["encoder.class_embedding"].unsqueeze(0).expand(n, -1, -1), h], dim=1)
    h = h + p["encoder.positional_embedding"][: h.shape[1]]
    lat = (p["latent_tokens"] + p["encoder.latent_token_positional_embedding"]).unsqueeze(0).expand(n, -1, -1)
    h = tc._ln(p, "encoder.ln_pre", torch.cat([h, lat], dim=1))
    for i in range(layers):
        h = tc.attention_block(p, f"encoder.transformer.{i}", h, heads)
    t = tc._ln(p, "encoder.ln_post", h[:, h.shape[1] - nlat:]).contiguous()                # (F, num_latent, C)
    if reading == "reshape":        # the reference: each frame's num_latent x C block read as C x num_latent, nothing moved
        t = t.reshape(n, width, nlat, 1)
    else:                           # what the comment in the reference ("fake 2D shape") suggests, and what it does NOT do
        t = t.permute(0, 2, 1).reshape(n, width, nlat, 1)
    return F.conv2d(t, p["encoder.conv_out.weight"], p["encoder.conv_out.bias"]).reshape(n, 2 * ts, 1, nlat)


def posterior(mom):
    """DiagonalGaussianDistribution: (mean, logvar clamped to [-30, 20], std)"""
    mean, logvar = mom.chunk(2, dim=1)
    logvar = logvar.clamp(-30.0, 20.0)
    return mean, logvar, torch.exp(0.5 * logvar)


def encode(p, cfg, x):
    """TiTok_KL.encode(x, sample=True): the mode"""
    return posterior(moments(p, cfg, x))[0]
