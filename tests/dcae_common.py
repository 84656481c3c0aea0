"""Shared helpers of tests/test_dcae_host.py, tests/test_gpu_dcae.py and tests/test_gpu_dcae_ops.py (not a test module): the DC-AE
autoencoder of the dmlab / Minecraft latents (algorithms/vae/dc_ae/autoencoder_dc_model.py).

  * CASES / config     the two configurations of tests/golden/dcae.npz (tools/make_golden_dcae.py) and the stock dmlab widths
  * seeded_tensor / seeded_params   the fixture's weights, re-created from the stored key names and shapes (one generator per key)
  * encode / decode    a torch restatement in any float dtype, functional over a state dict with the reference's key names, written for
                       this project from the model's description:
        Encoder.forward / Decoder.forward            :360-372, 452-465
        ResBlock.forward                             :126-138   (BatchNorm2d in eval mode: running statistics)
        DCDownBlock2d / DCUpBlock2d                  :226-240, 268-283
        SanaMultiscaleLinearAttention (linear)       :86-95 and the processor of diffusers 0.32.2 ([q | k | v] in 96-channel groups)
        GLUMBConv, RMSNorm                           diffusers 0.32.2
    ``mistake`` switches one deliberate error on (the sensitivities the fixture records): "heads", "shortcut", "batch_stats", "gate"
  * encode_frames / decode_latents   BaseVideoAlgo._encode / _decode for this model (base_pytorch_video_algo.py:588-604)
  * bn_fold            BatchNorm2d(eval) folded into the bias-free convolution in front of it
"""
import ast
import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FRAMES = 3
CASES = {
    "f8": dict(channels=(64, 64, 128, 128), enc_layers=(0, 2, 1, 1), dec_layers=(0, 1, 2, 2),
               norms=("batch_norm", "batch_norm", "batch_norm", "rms_norm"), acts=("relu", "relu", "relu", "silu"), size=64),
    "f16": dict(channels=(64, 64, 128, 128, 256), enc_layers=(0, 1, 1, 1, 1), dec_layers=(0, 1, 1, 1, 1),
                norms=("batch_norm", "batch_norm", "rms_norm", "rms_norm", "rms_norm"), acts=("relu", "relu", "silu", "silu", "silu"), size=128),
}
STOCK = dict(channels=(128, 256, 512, 512), enc_layers=(0, 2, 2, 2), dec_layers=(0, 2, 2, 2),
             norms=("batch_norm", "batch_norm", "batch_norm", "rms_norm"), acts=("relu", "relu", "relu", "silu"), size=64)
MISTAKES = ("heads", "shortcut", "batch_stats", "gate")
BAR = 2e-2   # the parity bar of tests/test_gpu_dcae.py (tests/test_gpu_image_vae.py:5-6)


def config(c):
    """the reference's config keys for one of the dicts above (block pattern of the stock configs: EfficientViT from stage 3 on)"""
    n = len(c["channels"])
    types = ["ResBlock"] * min(3, n) + ["EfficientViTBlock"] * max(0, n - 3)
    return dict(in_channels=3, latent_channels=32, attention_head_dim=32,
                encoder_block_types=list(types), decoder_block_types=list(types),
                encoder_block_out_channels=list(c["channels"]), decoder_block_out_channels=list(c["channels"]),
                encoder_layers_per_block=list(c["enc_layers"]), decoder_layers_per_block=list(c["dec_layers"]),
                encoder_qkv_multiscales=[[] for _ in range(n)], decoder_qkv_multiscales=[[] for _ in range(n)],
                decoder_norm_types=list(c["norms"]), decoder_act_fns=list(c["acts"]),
                downsample_block_type="pixel_unshuffle", upsample_block_type="pixel_shuffle", scaling_factor=0.2889)


def load():
    return np.load(os.path.join(GOLDEN, "dcae.npz"))


def key_shapes(g, case):
    return {str(n): ast.literal_eval(str(s)) for n, s in zip(g[f"names_{case}"], g[f"shapes_{case}"])}


def seeded_tensor(name, shape, seed=83):
    """order-independent seeded weights, one generator per key: N(0, 1 / fan_in) weights, norm weights 1 + 0.2 N, norm biases 0.1 N,
    convolution biases 0.02 N, BatchNorm running_mean 0.2 N, running_var in [0.5, 1.5), num_batches_tracked = 7"""
    g = torch.Generator().manual_seed((zlib.crc32(name.encode()) + 1000003 * seed) % (2 ** 31))
    shape = tuple(shape)
    if name.endswith("num_batches_tracked"):
        return torch.tensor(7, dtype=torch.long)
    if name.endswith("running_var"):
        return 0.5 + torch.rand(shape, generator=g)
    if name.endswith("running_mean"):
        return 0.2 * torch.randn(shape, generator=g)
    norm = ".norm." in name or ".norm_out." in name
    if name.endswith("bias"):
        return (0.1 if norm else 0.02) * torch.randn(shape, generator=g)
    if len(shape) == 1:
        return 1.0 + 0.2 * torch.randn(shape, generator=g)
    fan_in = 1
    for d in shape[1:]:
        fan_in *= d
    return torch.randn(shape, generator=g) / (fan_in ** 0.5)


def seeded_params(shapes):
    return {n: seeded_tensor(n, s) for n, s in shapes.items()}


def digest(params):
    """crc32 over the fp32 bytes of every tensor in key order: the fixture stores it, the tests compare"""
    crc = 0
    for n in params:
        crc = zlib.crc32(params[n].detach().to(torch.float32).contiguous().numpy().tobytes(), crc)
    return crc


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def cast(p, dtype):
    return {n: (t.to(dtype) if t.is_floating_point() else t) for n, t in p.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
def _act(name, x):
    return F.relu(x) if name == "relu" else x * torch.sigmoid(x)


def rms_norm(p, name, x):
    """channel RMSNorm of an NCHW map: weight and bias, eps 1e-5"""
    xc = x.movedim(1, -1)
    y = xc * torch.rsqrt(xc.pow(2).mean(-1, keepdim=True) + 1e-5) * p[name + ".weight"] + p[name + ".bias"]
    return y.movedim(-1, 1)


def res_block(p, name, x, norm, act, mistake=None):
    h = F.conv2d(x, p[name + ".conv1.weight"], p[name + ".conv1.bias"], padding=1)
    h = F.conv2d(_act(act, h), p[name + ".conv2.weight"], None, padding=1)
    if norm == "rms_norm":
        h = rms_norm(p, name + ".norm", h)
    else:
        h = F.batch_norm(h, p[name + ".norm.running_mean"], p[name + ".norm.running_var"], p[name + ".norm.weight"], p[name + ".norm.bias"],
                         mistake == "batch_stats", 0.0, 1e-5)
    return x + h


def linear_attention(p, name, x, mistake=None):
    b, c, hh, ww = x.shape
    xc = x.movedim(1, -1)
    q, k, v = (F.linear(xc, p[f"{name}.to_{n}.weight"]).movedim(-1, 1).reshape(b, c, hh * ww) for n in "qkv")
    if mistake == "heads":      # channels [32 g, 32 g + 32) of each projection
        q, k, v = (t.reshape(b, c // 32, 32, hh * ww) for t in (q, k, v))
    else:                       # the reference: 96-channel groups of the concatenation [q | k | v]
        q, k, v = torch.cat([q, k, v], 1).reshape(b, c // 32, 96, hh * ww).chunk(3, dim=2)
    q, k = F.relu(q), F.relu(k)
    v1 = F.pad(v, (0, 0, 0, 1), value=1.0)
    o = (v1 @ k.transpose(-1, -2)) @ q
    o = (o[:, :, :-1] / (o[:, :, -1:] + 1e-15)).reshape(b, c, hh, ww)
    o = F.linear(o.movedim(1, -1), p[name + ".to_out.weight"]).movedim(-1, 1)
    return x + rms_norm(p, name + ".norm_out", o)


def glumbconv(p, name, x, mistake=None):
    h = F.conv2d(x, p[name + ".conv_inverted.weight"], p[name + ".conv_inverted.bias"])
    h = _act("silu", h)
    h = F.conv2d(h, p[name + ".conv_depth.weight"], p[name + ".conv_depth.bias"], padding=1, groups=h.shape[1])
    a, gate = torch.chunk(h, 2, dim=1)
    if mistake == "gate":
        a, gate = gate, a
    h = F.conv2d(a * _act("silu", gate), p[name + ".conv_point.weight"], None)
    return x + rms_norm(p, name + ".norm", h)


def block(p, name, kind, x, norm, act, mistake=None):
    if kind == "ResBlock":
        return res_block(p, name, x, norm, act, mistake)
    return glumbconv(p, name + ".conv_out", linear_attention(p, name + ".attn", x, mistake), mistake)


def down_block(p, name, x, cout, shortcut=True):
    y = F.pixel_unshuffle(F.conv2d(x, p[name + ".conv.weight"], p[name + ".conv.bias"], padding=1), 2)
    if shortcut:
        y = y + F.pixel_unshuffle(x, 2).unflatten(1, (cout, -1)).mean(dim=2)
    return y


def up_block(p, name, x, cout, shortcut=True):
    y = F.pixel_shuffle(F.conv2d(x, p[name + ".conv.weight"], p[name + ".conv.bias"], padding=1), 2)
    if shortcut:
        y = y + F.pixel_shuffle(x.repeat_interleave(4 * cout // x.shape[1], dim=1), 2)
    return y


def encode(p, cfg, x, mistake=None):
    """x (F, 3, S, S) in [-1, 1] -> latents (F, latent_channels, S / r, S / r)"""
    ch, layers, types = cfg["encoder_block_out_channels"], cfg["encoder_layers_per_block"], cfg["encoder_block_types"]
    sc = mistake != "shortcut"
    h = down_block(p, "encoder.conv_in", x, ch[1], shortcut=False)
    for i in range(len(ch)):
        for j in range(layers[i]):
            h = block(p, f"encoder.down_blocks.{i}.{j}", types[i], h, "rms_norm", "silu", mistake)
        if i < len(ch) - 1 and layers[i] > 0:
            h = down_block(p, f"encoder.down_blocks.{i}.{layers[i]}", h, ch[i + 1], sc)
    y = F.conv2d(h, p["encoder.conv_out.weight"], p["encoder.conv_out.bias"], padding=1)
    return y + h.unflatten(1, (cfg["latent_channels"], -1)).mean(dim=2) if sc else y


def decode(p, cfg, z, mistake=None):
    """z (F, latent_channels, h, w) -> frames (F, 3, h r, w r)"""
    ch, layers, types = cfg["decoder_block_out_channels"], cfg["decoder_layers_per_block"], cfg["decoder_block_types"]
    sc = mistake != "shortcut"
    h = F.conv2d(z, p["decoder.conv_in.weight"], p["decoder.conv_in.bias"], padding=1)
    if sc:
        h = h + z.repeat_interleave(ch[-1] // cfg["latent_channels"], dim=1)
    for i in reversed(range(len(ch))):
        j0 = 0
        if i < len(ch) - 1 and layers[i] > 0:
            h = up_block(p, f"decoder.up_blocks.{i}.0", h, ch[i], sc)
            j0 = 1
        for j in range(layers[i]):
            h = block(p, f"decoder.up_blocks.{i}.{j0 + j}", types[i], h, cfg["decoder_norm_types"][i], cfg["decoder_act_fns"][i], mistake)
    h = F.relu(rms_norm(p, "decoder.norm_out", h))
    return up_block(p, "decoder.conv_out", h, cfg["in_channels"], shortcut=False)


def encode_frames(p, cfg, videos):
    """_encode: frames (b t c h w) in [0, 1] -> latents (b t c h w); scaling_factor is not applied"""
    b, t = videos.shape[:2]
    z = encode(p, cfg, 2.0 * videos.reshape(b * t, *videos.shape[2:]) - 1.0)
    return z.reshape(b, t, *z.shape[1:])


def decode_latents(p, cfg, latents):
    """_decode: latents (b t c h w) -> frames (b t c h w) in [0, 1]"""
    b, t = latents.shape[:2]
    y = decode(p, cfg, latents.reshape(b * t, *latents.shape[2:])) * 0.5 + 0.5
    return y.reshape(b, t, *y.shape[1:])


def bn_fold(w, gamma, beta, mean, var, eps=1e-5):
    """BatchNorm2d(eval) after a bias-free convolution w [co][ci][k][k]: (w', b') with bn(conv(x, w)) = conv(x, w') + b'"""
    s = gamma / torch.sqrt(var + eps)
    return w * s.reshape(-1, 1, 1, 1), beta - mean * s
