"""Shared helpers of tests/test_gpu_image_vae_1024.py and tests/test_image_vae_diffusers_host.py (not a test module): the ImageVAE
with a mid attention over 1024 positions per frame, and the diffusers key layout.  The restatement, the seeded weights and the metrics
are the functions of tests/image_vae_common.py.

  * CASE "c"       the configuration of tests/golden/image_vae_1024.npz (tools/make_golden_image_vae_1024.py): ch 128, ch_mult (1, 2),
                   one res block, resolution 64, 2 frames -> mid attention at 32 x 32 = 1024 positions, C = 256
  * RECIPE         the KL-f8 autoencoder of the taichikl recipes (configurations/algorithm/vae/image_vae.yaml's ddconfig) at 256 x 256
  * to_diffusers   the reference's key names -> the diffusers ``AutoencoderKL`` names, written independently of the product's map
"""
import os
import re

import numpy as np

import image_vae_common as ivc
from image_vae_common import T, decode, encode, rel  # noqa: F401
from oracle import vae as ovae

CASE = "c"
CFG_C = dict(ch=128, out_ch=3, ch_mult=(1, 2), num_res_blocks=1, z_channels=4, embed_dim=4, resolution=64, attn_resolutions=())
RECIPE = dict(ch=128, out_ch=3, ch_mult=(1, 2, 4, 4), num_res_blocks=2, z_channels=4, embed_dim=4, resolution=256, attn_resolutions=())


def load():
    return np.load(os.path.join(ivc.GOLDEN, "image_vae_1024.npz"))


def seeded_params(g):
    return ivc.seeded_params(g, CASE)


def param_shapes(cfg):
    """the reference's state-dict names and shapes for a ddconfig (Encoder / Decoder of model.py:18-245 + the two 1x1 quant convolutions)"""
    ch, mult, nres, z, e = cfg["ch"], cfg["ch_mult"], cfg["num_res_blocks"], cfg["z_channels"], cfg["embed_dim"]
    chans = [ch * m for m in mult]
    out = {}

    def conv(n, ci, co, k):
        out[n + ".weight"], out[n + ".bias"] = (co, ci, k, k), (co,)

    def norm(n, c):
        out[n + ".weight"], out[n + ".bias"] = (c,), (c,)

    def res(n, ci, co):
        norm(n + ".norm1", ci), conv(n + ".conv1", ci, co, 3), norm(n + ".norm2", co), conv(n + ".conv2", co, co, 3)
        if ci != co:
            conv(n + ".nin_shortcut", ci, co, 1)

    def mid(root, c):
        res(f"{root}.mid.block_1", c, c)
        norm(f"{root}.mid.attn_1.norm", c)
        for n in ("q", "k", "v", "proj_out"):
            conv(f"{root}.mid.attn_1.{n}", c, c, 1)
        res(f"{root}.mid.block_2", c, c)

    conv("encoder.conv_in", 3, ch, 3)
    cin = ch
    for lvl, c in enumerate(chans):
        for i in range(nres):
            res(f"encoder.down.{lvl}.block.{i}", cin, c)
            cin = c
        if lvl != len(chans) - 1:
            conv(f"encoder.down.{lvl}.downsample.conv", c, c, 3)
    mid("encoder", chans[-1])
    norm("encoder.norm_out", chans[-1])
    conv("encoder.conv_out", chans[-1], 2 * z, 3)
    conv("decoder.conv_in", z, chans[-1], 3)
    mid("decoder", chans[-1])
    cin = chans[-1]
    for lvl in reversed(range(len(chans))):
        for i in range(nres + 1):
            res(f"decoder.up.{lvl}.block.{i}", cin, chans[lvl])
            cin = chans[lvl]
        if lvl != 0:
            conv(f"decoder.up.{lvl}.upsample.conv", cin, cin, 3)
    norm("decoder.norm_out", chans[0])
    conv("decoder.conv_out", chans[0], cfg["out_ch"], 3)
    conv("quant_conv", 2 * z, 2 * e, 1)
    conv("post_quant_conv", e, z, 1)
    return out


def seeded_recipe_params(cfg):
    return {n: ovae.seeded_tensor(n, s) for n, s in param_shapes(cfg).items()}


_ATTN = {"q": "to_q", "k": "to_k", "v": "to_v", "proj_out": "to_out.0", "norm": "group_norm"}
_ATTN_LEGACY = {"q": "query", "k": "key", "v": "value", "proj_out": "proj_attn", "norm": "group_norm"}


def to_diffusers_name(name, levels, legacy=False):
    """one reference (ldm) key -> its diffusers ``AutoencoderKL`` name"""
    name = name.replace(".nin_shortcut.", ".conv_shortcut.")
    name = re.sub(r"^(encoder|decoder)\.norm_out\.", r"\1.conv_norm_out.", name)
    name = re.sub(r"\.mid\.block_([12])\.", lambda m: f".mid_block.resnets.{int(m.group(1)) - 1}.", name)
    m = re.match(r"^(encoder|decoder)\.mid\.attn_1\.(\w+)\.(weight|bias)$", name)
    if m:
        return f"{m.group(1)}.mid_block.attentions.0.{(_ATTN_LEGACY if legacy else _ATTN)[m.group(2)]}.{m.group(3)}"
    name = re.sub(r"^encoder\.down\.(\d+)\.block\.(\d+)\.", r"encoder.down_blocks.\1.resnets.\2.", name)
    name = re.sub(r"^encoder\.down\.(\d+)\.downsample\.conv\.", r"encoder.down_blocks.\1.downsamplers.0.conv.", name)
    name = re.sub(r"^decoder\.up\.(\d+)\.block\.(\d+)\.", lambda m: f"decoder.up_blocks.{levels - 1 - int(m.group(1))}.resnets.{m.group(2)}.", name)
    return re.sub(r"^decoder\.up\.(\d+)\.upsample\.conv\.", lambda m: f"decoder.up_blocks.{levels - 1 - int(m.group(1))}.upsamplers.0.conv.", name)


def to_diffusers(params, levels, legacy=False):
    """a reference state dict in the diffusers layout: renamed, the attention projections as Linear weights [C, C]"""
    out = {}
    for n, t in params.items():
        d = to_diffusers_name(n, levels, legacy)
        if ".attentions.0." in d and d.endswith(".weight") and t.ndim == 4:
            t = t.reshape(t.shape[0], t.shape[1])
        out[d] = t
    return out
