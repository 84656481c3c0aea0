"""Shared helpers of tests/test_dit_attnmap_host.py, tests/test_gpu_dit_attnmap.py and tools/make_golden_dit_attnmap.py (not a test
module): the three tiny DiT3D models whose attention maps the fixture tests/golden/dit_attnmap.npz stores -- hidden 128, depth 2, 4 heads,
latents 4x16x8, patch 1 (P = 128), max_tokens 5 -- with the seeded weights of the existing fixtures and a gain on the q / k weights of the
frame-mixing blocks (small random weights give near-uniform maps, which would hide a wrong frame binning or a swapped axis).

  full     variant "full", rope_3d: oracle.dit.seeded_params(FULL_CFG, FULL_SEED); blocks dit_base.blocks.{i}.attn
  fac      variant "factorized_attention": dit_fac_common, spatial_mlp_ratio 0; blocks dit_base.temporal_blocks.{i}.attn
  facmat   variant "factorized_matrix_attention" with the temporal RoPE: dit_facmat_common case "a"; blocks dit_base.temporal_blocks.{i}.attn
"""
import torch

import dit_fac_common as fc
import dit_facmat_common as fm
from dit_fac_common import T, load, rel  # noqa: F401
from oracle import dit as odit

VARIANTS = ("full", "fac", "facmat")
TOKENS, HEIGHT, WIDTH, PATCHES, HEADS, HIDDEN, DEPTH = 5, 16, 8, 128, 4, 128, 2
FULL_CFG = odit.DiTConfig(hidden_size=HIDDEN, depth=DEPTH, num_heads=HEADS, patch_size=1, in_channels=4, resolution=(HEIGHT, WIDTH), max_tokens=TOKENS)
FULL_SEED = 11
FACMAT_CASE = "a"
FULL_TOKENS, FULL_BATCH_ROW, FULL_HEAD, FULL_BLOCK = 2, 1, 2, 1  # the one stored full map: block 1, video 1, head 2 of a T = 2 forward
PARITY_BAR = 2e-2      # the project's forward-vs-reference bar (tests/test_gpu_dit.py:150)
CONTRAST_BAR = 4e-2    # twice the parity bar: every stored frame map differs by this much from uniform and from its transpose
RESTATE_BAR = 1e-2     # half the parity bar: the bf16 host restatement against the fp32 maps, measured by the tool on the CPU


def block_names(variant):
    stem = "dit_base.blocks" if variant == "full" else "dit_base.temporal_blocks"
    return [f"{stem}.{i}.attn" for i in range(DEPTH)]


def seeded(variant, gain):
    """the variant's seeded weights with the q and k projections of its frame-mixing blocks scaled by `gain` (scores scale by gain^2)"""
    if variant == "full":
        params = odit.seeded_params(FULL_CFG, FULL_SEED)
    elif variant == "fac":
        params = fc.seeded_params(fc.key_shapes(0.0))
    else:
        params = fm.case_params(FACMAT_CASE)
    for name in block_names(variant):
        if variant == "facmat":
            params[f"{name}.qkv_v"][:, : 2 * HIDDEN] *= gain  # (in, out) factor: the q | k columns
        else:
            params[f"{name}.qkv.weight"][: 2 * HIDDEN] *= gain
            params[f"{name}.qkv.bias"][: 2 * HIDDEN] *= gain
    return params


def engine_cfg(variant):
    if variant == "full":
        return dict(variant="full", pos_emb_type="rope_3d", patch_size=1, hidden_size=HIDDEN, depth=DEPTH, num_heads=HEADS)
    if variant == "fac":
        return fc.backbone_cfg(0.0)
    cc, rr, bias, ratio, rope = fm.CASES[FACMAT_CASE]
    return fm.backbone_cfg(cc, rr, bias, ratio, rope)


def build(variant, gain, cls=None):
    """the engine's model at the fixture's configuration and weights, eval() as the reference's module was"""
    import dfot_amd
    params = seeded(variant, gain)
    model = (cls or dfot_amd.DiT3D)(engine_cfg(variant), x_shape=(4, HEIGHT, WIDTH), max_tokens=TOKENS).cuda().eval()
    model.load_state_dict(params, strict=True)
    return model, params


def map_shape(variant, batch, tokens=TOKENS):
    if variant == "facmat":
        cc, rr = fm.CASES[FACMAT_CASE][:2]
        return (batch, cc, rr, tokens, tokens)
    return (batch, HEADS, tokens, tokens)


def contrast(f):
    """(rel-L2 of a frame map [..., T, T] against the uniform map, against its own transpose)"""
    t = f.shape[-1]
    return rel(f, torch.full_like(f, 1.0 / t)), rel(f, f.transpose(-1, -2))
