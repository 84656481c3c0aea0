"""Shared helpers of tests/test_image_vae_host.py, tests/test_gpu_image_vae.py and tests/test_gpu_image_vae_ops.py (not a test module):
the per-frame ImageVAE (Stable-Diffusion-style 2-D autoencoder) of the DMLab / Minecraft latent recipes.

  * CASES / ddconfig   the two configurations of tests/golden/image_vae.npz (tools/make_golden_image_vae.py)
  * seeded_params      the fixture's weights, re-created from the stored key names and shapes (oracle.vae.seeded_tensor)
  * encode / decode    an fp32 (any float dtype) torch restatement, functional over a state dict with the reference's key names:
        Encoder.forward / Decoder.forward      algorithms/vae/image_vae/model.py:103-125, 215-245
        ImageVAE.encode / decode               algorithms/vae/image_vae/trainer.py:334-343  (1x1 quant_conv / post_quant_conv)
        ResnetBlock2D.forward                  algorithms/vae/common/modules/resnet.py:42-58
        AttnBlock.forward                      algorithms/vae/common/modules/attention.py:58-83
        Upsample / Downsample                  algorithms/vae/common/modules/updownsample.py:10-45
        Normalize = GroupNorm(32, eps 1e-6), nonlinearity = x * sigmoid(x)     normalize.py, ops.py
  * encode_frames / decode_latents   BaseVideoAlgo._encode / _decode for an ImageVAE (base_pytorch_video_algo.py:553-629)
"""
import ast
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vae as ovae

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"a": dict(ch_mult=(1, 2), resolution=16, frames=4), "b": dict(ch_mult=(1, 2, 2), resolution=64, frames=2)}


def ddconfig(case):
    c = CASES[case]
    return dict(ch=128, out_ch=3, ch_mult=c["ch_mult"], num_res_blocks=1, z_channels=4, embed_dim=4, resolution=c["resolution"],
                attn_resolutions=())


def load():
    return np.load(os.path.join(GOLDEN, "image_vae.npz"))


def key_shapes(g, case):
    return {str(n): ast.literal_eval(str(s)) for n, s in zip(g[f"names_{case}"], g[f"shapes_{case}"])}


def seeded_params(g, case):
    return {n: ovae.seeded_tensor(n, s) for n, s in key_shapes(g, case).items()}


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _conv(p, name, x, stride=1, padding=1):
    return F.conv2d(x, p[name + ".weight"], p[name + ".bias"], stride=stride, padding=padding)


def _norm(p, name, x):
    return F.group_norm(x, 32, p[name + ".weight"], p[name + ".bias"], eps=1e-6)


def _silu(x):
    return x * torch.sigmoid(x)


def resnet_block(p, name, x):
    h = _conv(p, name + ".conv1", _silu(_norm(p, name + ".norm1", x)))
    h = _conv(p, name + ".conv2", _silu(_norm(p, name + ".norm2", h)))
    if name + ".nin_shortcut.weight" in p:
        x = _conv(p, name + ".nin_shortcut", x, padding=0)
    return x + h


def attn_block(p, name, x):
    h = _norm(p, name + ".norm", x)
    q, k, v = (_conv(p, f"{name}.{n}", h, padding=0) for n in ("q", "k", "v"))
    b, c, hh, ww = q.shape
    q, k, v = q.reshape(b, c, hh * ww).permute(0, 2, 1), k.reshape(b, c, hh * ww), v.reshape(b, c, hh * ww)
    w = torch.softmax(torch.bmm(q, k) * (int(c) ** -0.5), dim=2)
    o = torch.bmm(v, w.permute(0, 2, 1)).reshape(b, c, hh, ww)
    return x + _conv(p, name + ".proj_out", o, padding=0)


def _mid(p, root, h):
    h = resnet_block(p, f"{root}.mid.block_1", h)
    h = attn_block(p, f"{root}.mid.attn_1", h)
    return resnet_block(p, f"{root}.mid.block_2", h)


def encode(p, cfg, x):
    """x (F, 3, H, W) in [-1, 1] -> moments (F, 2 * embed_dim, h, w) = quant_conv(Encoder(x))"""
    levels = len(cfg["ch_mult"])
    h = _conv(p, "encoder.conv_in", x)
    for lvl in range(levels):
        for i in range(cfg["num_res_blocks"]):
            h = resnet_block(p, f"encoder.down.{lvl}.block.{i}", h)
        if lvl != levels - 1:
            h = _conv(p, f"encoder.down.{lvl}.downsample.conv", F.pad(h, (0, 1, 0, 1)), stride=2, padding=0)
    h = _mid(p, "encoder", h)
    h = _conv(p, "encoder.conv_out", _silu(_norm(p, "encoder.norm_out", h)))
    return _conv(p, "quant_conv", h, padding=0)


def decode(p, cfg, z):
    """z (F, embed_dim, h, w) -> frames (F, out_ch, H, W) = Decoder(post_quant_conv(z))"""
    levels = len(cfg["ch_mult"])
    h = _conv(p, "decoder.conv_in", _conv(p, "post_quant_conv", z, padding=0))
    h = _mid(p, "decoder", h)
    for lvl in reversed(range(levels)):
        for i in range(cfg["num_res_blocks"] + 1):
            h = resnet_block(p, f"decoder.up.{lvl}.block.{i}", h)
        if lvl != 0:
            h = _conv(p, f"decoder.up.{lvl}.upsample.conv", F.interpolate(h, scale_factor=2.0, mode="nearest"))
    return _conv(p, "decoder.conv_out", _silu(_norm(p, "decoder.norm_out", h)))


def posterior(moments):
    """DiagonalGaussianDistribution (algorithms/vae/common/distribution.py): mean, logvar clamped to [-30, 20], std"""
    mean, logvar = torch.chunk(moments, 2, dim=1)
    logvar = torch.clamp(logvar, -30.0, 20.0)
    return mean, logvar, torch.exp(0.5 * logvar)


def decode_latents(p, cfg, latents):
    """_decode for an ImageVAE: latents (b t c h w) -> frames (b t c h w) in [0, 1]"""
    b, t = latents.shape[:2]
    y = decode(p, cfg, latents.reshape(b * t, *latents.shape[2:])) * 0.5 + 0.5
    return y.reshape(b, t, *y.shape[1:])


def encode_frames(p, cfg, videos, eps=None):
    """_encode for an ImageVAE: frames (b t c h w) in [0, 1] -> latents (b t c h w) = mean (+ std * eps)"""
    b, t = videos.shape[:2]
    mean, _, std = posterior(encode(p, cfg, 2.0 * videos.reshape(b * t, *videos.shape[2:]) - 1.0))
    z = mean if eps is None else mean + std * eps.reshape(mean.shape)
    return z.reshape(b, t, *z.shape[1:])
