"""Shared helpers of tests/test_titok_host.py, tests/test_gpu_titok.py and tests/test_gpu_titok_ops.py (not a test module): the decoder half
of TiTok_KL, the 1-D token autoencoder of the taichi recipes (32 latent tokens of 4 channels per frame).

  * CASES / config     the three configurations of tests/golden/titok.npz (tools/make_golden_titok.py)
  * seeded_params      the fixture's decoder weights, re-created from the stored key names and shapes (oracle.vae.seeded_tensor, with
                       decoder.ffn.2.weight multiplied by the gain the file records: see the tool's docstring for why)
  * decode and its stages   an fp32 (any float dtype) torch restatement, functional over a state dict with the reference's key names:
        TiTok_KL.decode                       algorithms/vae/tiktok_kl/titok_kl.py:100-109
        TiTokDecoder.forward                  algorithms/vae/tiktok_kl/blocks_kl.py:219-245
        ResidualAttentionBlock.forward        algorithms/vae/tiktok_kl/blocks_kl.py:39-88  (nn.MultiheadAttention, nn.GELU() = erf form)
        Decoder / ResnetBlock / UpsamplingBlock   algorithms/vae/tiktok_kl/maskgit_vqgan.py:53-90, 122-154, 197-245
  * decode_latents     BaseVideoAlgo._decode for a TiTok_KL (base_pytorch_video_algo.py:611-617): no rescaling
"""
import ast
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vae as ovae

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"a": dict(size="small", image_size=64, frames=3), "b": dict(size="base", image_size=128, frames=2),
         "c": dict(size="small", image_size=256, frames=1)}
PRESETS = {"small": (512, 8, 8), "base": (768, 12, 12), "large": (1024, 24, 16)}      # width, layers, heads
LOGIT_CASES = ("a", "b")
PIXEL_UP = ((4, 512, 512), (3, 512, 256), (2, 256, 256), (1, 256, 128), (0, 128, 128))  # maskgit_vqgan.Decoder: (block index, in, out), run order


def config(case):
    c = CASES[case]
    return dict(image_size=c["image_size"], token_size=4, use_l2_norm=True, vit_dec_model_size=c["size"], vit_dec_patch_size=16,
                num_latent_tokens=32)


def load():
    """the fixture as one mapping: titok.npz plus the large arrays of cases b and c, which have files of their own (size)"""
    out = {}
    for fn in ("titok.npz", "titok_b.npz", "titok_b_logits.npz", "titok_c.npz"):
        with np.load(os.path.join(GOLDEN, fn)) as g:
            out.update({k: g[k] for k in g.files})
    return out


def key_shapes(g, case):
    return {str(n): ast.literal_eval(str(s)) for n, s in zip(g[f"names_{case}"], g[f"shapes_{case}"])}


def seeded_tensor(name, shape, gain):
    t = ovae.seeded_tensor(name, shape)
    return t * gain if name == "decoder.ffn.2.weight" else t


def seeded_params(g, case):
    gain = float(g["ffn2_gain"])
    return {n: seeded_tensor(n, s, gain) for n, s in key_shapes(g, case).items()}


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _ln(p, name, x):
    return F.layer_norm(x, x.shape[-1:], p[name + ".weight"], p[name + ".bias"], 1e-5)


def attention_block(p, name, x, heads):
    """ResidualAttentionBlock on x (N, L, C): nn.MultiheadAttention packs q | k | v in in_proj_weight [3C, C]; heads of C / heads = 64"""
    n, l, c = x.shape
    h = _ln(p, name + ".ln_1", x)
    qkv = F.linear(h, p[name + ".attn.in_proj_weight"], p[name + ".attn.in_proj_bias"])
    q, k, v = (t.reshape(n, l, heads, c // heads).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
    w = torch.softmax(q @ k.transpose(-1, -2) / (c // heads) ** 0.5, dim=-1)
    o = (w @ v).transpose(1, 2).reshape(n, l, c)
    x = x + F.linear(o, p[name + ".attn.out_proj.weight"], p[name + ".attn.out_proj.bias"])
    h = F.gelu(F.linear(_ln(p, name + ".ln_2", x), p[name + ".mlp.c_fc.weight"], p[name + ".mlp.c_fc.bias"]))     # exact (erf) GELU
    return x + F.linear(h, p[name + ".mlp.c_proj.weight"], p[name + ".mlp.c_proj.bias"])


def tokens(p, cfg, z):
    """steps 1-2: z (F, token_size, 1, 32) -> ln_pre of [cls | grid^2 mask tokens | latent tokens]  (F, L, C)"""
    grid2 = (cfg["image_size"] // cfg["vit_dec_patch_size"]) ** 2
    if cfg["use_l2_norm"]:
        z = F.normalize(z, dim=1)
    n, c, hh, ww = z.shape
    x = F.linear(z.reshape(n, c * hh, ww).permute(0, 2, 1), p["decoder.decoder_embed.weight"], p["decoder.decoder_embed.bias"])
    x = x + p["decoder.latent_token_positional_embedding"][: x.shape[1]]
    mask = torch.cat([p["decoder.class_embedding"].unsqueeze(0).expand(n, -1, -1), p["decoder.mask_token"].repeat(n, grid2, 1)], dim=1)
    mask = mask + p["decoder.positional_embedding"][None, : grid2 + 1]
    return _ln(p, "decoder.ln_pre", torch.cat([mask, x], dim=1))


def logits(p, cfg, z):
    """TiTokDecoder.forward: z -> (F, 1024, grid, grid)"""
    width, layers, heads = PRESETS[cfg["vit_dec_model_size"]]
    grid = cfg["image_size"] // cfg["vit_dec_patch_size"]
    x = tokens(p, cfg, z)
    for i in range(layers):
        x = attention_block(p, f"decoder.transformer.{i}", x, heads)
    x = _ln(p, "decoder.ln_post", x[:, 1:1 + grid * grid])
    x = x.permute(0, 2, 1).reshape(x.shape[0], width, grid, grid)
    x = torch.tanh(F.conv2d(x, p["decoder.ffn.0.weight"], p["decoder.ffn.0.bias"]))
    return F.conv2d(x, p["decoder.ffn.2.weight"], p["decoder.ffn.2.bias"])


def pixel_input(p, lg):
    """softmax over the 1024 channels, then pixel_quantize_conv (1x1, 1024 -> 256)"""
    return F.conv2d(lg.softmax(1), p["pixel_quantize_conv.weight"], p["pixel_quantize_conv.bias"])


def _gn_silu(p, name, x):
    return F.silu(F.group_norm(x, 32, p[name + ".weight"], p[name + ".bias"], eps=1e-6))


def resnet_block(p, name, x):
    """maskgit_vqgan.ResnetBlock: bias-free convolutions; with a channel change the block returns h + nin_shortcut(h), h the conv2 output
    (the block's input is dropped, :87-90)"""
    h = F.conv2d(_gn_silu(p, name + ".norm1", x), p[name + ".conv1.weight"], None, padding=1)
    h = F.conv2d(_gn_silu(p, name + ".norm2", h), p[name + ".conv2.weight"], None, padding=1)
    if name + ".nin_shortcut.weight" in p:
        x = F.conv2d(h, p[name + ".nin_shortcut.weight"], None)
    return h + x


def pixel_decode(p, lat):
    """maskgit_vqgan.Decoder.forward: (F, 256, g, g) -> (F, 3, 16 g, 16 g)"""
    h = F.conv2d(lat, p["pixel_decoder.conv_in.weight"], p["pixel_decoder.conv_in.bias"], padding=1)
    for i in range(2):
        h = resnet_block(p, f"pixel_decoder.mid.{i}", h)
    for idx, _, _ in PIXEL_UP:
        for j in range(2):
            h = resnet_block(p, f"pixel_decoder.up.{idx}.block.{j}", h)
        if idx != 0:
            h = F.conv2d(F.interpolate(h, scale_factor=2.0, mode="nearest"), p[f"pixel_decoder.up.{idx}.upsample_conv.weight"],
                         p[f"pixel_decoder.up.{idx}.upsample_conv.bias"], padding=1)
    return F.conv2d(_gn_silu(p, "pixel_decoder.norm_out", h), p["pixel_decoder.conv_out.weight"], p["pixel_decoder.conv_out.bias"], padding=1)


def decode(p, cfg, z):
    """TiTok_KL.decode: z (F, token_size, 1, 32) -> frames (F, 3, image_size, image_size)"""
    return pixel_decode(p, pixel_input(p, logits(p, cfg, z)))


def decode_latents(p, cfg, latents):
    """_decode for a TiTok_KL: latents (b t c 1 32) -> frames (b t 3 H W), as decode returns them (no rescaling)"""
    b, t = latents.shape[:2]
    y = decode(p, cfg, latents.reshape(b * t, *latents.shape[2:]))
    return y.reshape(b, t, *y.shape[1:])
