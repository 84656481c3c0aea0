"""Shared helpers of tests/test_dit_p64_host.py, tests/test_gpu_dit_p64.py and tools/make_golden_dit_p64.py (not a test module): FacDiT and
FacMatDiT at 64 patches per frame, the shape of the taichi res-128 recipes (KL-f8 latents 4x16x16, patch 2).  Everything about the two
models themselves -- key order, seeded weights, the host restatements -- is tests/dit_fac_common.py / tests/dit_facmat_common.py with the
geometry below passed as **over."""
import torch

import dit_fac_common as fc
import dit_facmat_common as fm
from dit_fac_common import COND_DIM, COND_DROPOUT, T, digest, load, rel  # noqa: F401

# the fixture's geometry: hidden 128, depth 2, 4 heads (d = 32) from the TINY configurations; latents 4x16x16 at patch 2 = 64 patches
X_SHAPE = (4, 16, 16)
MAX_TOKENS, BATCH = 4, 2
OVER = dict(patch_size=2, resolution=(16, 16), max_tokens=MAX_TOKENS)
FIXTURE = "dit_p64.npz"
FIXTURE_BAR = 2e-2  # tests/test_gpu_dit_fac.py

FAC_CASES = {"mlp0": 0.0, "mlp4": 4.0}  # tag -> spatial_mlp_ratio
MAT_CASES = ("b", "d")  # of dit_facmat_common.CASES: b = use_bias + temporal RoPE, d = neither; both embed_col_dim 64


def fac_keys(ratio, cond=False, **over):
    return fc.key_shapes(ratio, COND_DIM if cond else 0, COND_DROPOUT if cond else 0.0, **{**OVER, **over})


def mat_keys(tag, **over):
    cc, rr, bias, ratio, rope = fm.CASES[tag]
    return fm.key_shapes(bias, ratio, **{**OVER, **over})


def fac_cfg(ratio, cond=False, **over):
    return fc.backbone_cfg(ratio, COND_DROPOUT if cond else 0.0, **{**OVER, **over})


def mat_cfg(tag, **over):
    cc, rr, bias, ratio, rope = fm.CASES[tag]
    return fm.backbone_cfg(cc, rr, bias, ratio, rope, **{**OVER, **over})


def fac_host(params, x, k, cond=None, mask=None, dtype=torch.float64, **over):
    return fc.forward_host(params, x, k, cond, mask, dtype=dtype, **{**OVER, **over})


def mat_host(tag, params, x, k, dtype=torch.float64, **over):
    cc, rr, bias, ratio, rope = fm.CASES[tag]
    return fm.forward_host(params, x, k, cc, rr, rope, dtype=dtype, **{**OVER, **over})


# ---- attention maps: the frame maps of the frame-mixing blocks, from the host restatements -----------------------------------------
# The maps are those of fac mlp0 / facmat b with the seeded weights as they are: tools/make_golden_dit_attnmap.py raises a gain on the q / k
# weights until every map clears CONTRAST_BAR, and for these two variants it stopped at gain 1; so it is here (the host test asserts the
# contrast: >= 0.14 for FacDiT, >= 0.9 for FacMatDiT).
MAP_BAR = 2e-2       # dit_attnmap_common.PARITY_BAR, the bar of tests/test_gpu_dit_attnmap.py
CONTRAST_BAR = 4e-2  # dit_attnmap_common.CONTRAST_BAR: every host map differs by this much from uniform and from its transpose


def host_frame_maps(variant, params, x, k, dtype=torch.float64):
    """{block name: frame map} of the restated forward.  Every attention of both restatements goes through torch.softmax, spatial block
    then frame-mixing block per depth, so the maps are the odd-numbered softmax results of one forward: FacDiT [(b p)][heads][T][T],
    averaged over the patch positions; FacMatDiT [b][col heads][row heads][T][T] as it is."""
    seen, real = [], torch.softmax

    def recording(*a, **kw):
        seen.append(real(*a, **kw))
        return seen[-1]
    torch.softmax = recording
    try:
        fac_host(params, x, k, dtype=dtype) if variant == "fac" else mat_host("b", params, x, k, dtype=dtype)
    finally:
        torch.softmax = real
    depth = fc.TINY["depth"]
    assert len(seen) == 2 * depth
    out = {}
    for i in range(depth):
        w = seen[2 * i + 1]
        if variant == "fac":
            w = w.reshape(x.shape[0], -1, *w.shape[1:]).mean(1)
        out[f"dit_base.temporal_blocks.{i}.attn"] = w
    return out


def build_fac(ratio, cond=False):
    """the engine's FacDiT at the fixture's geometry with the seeded weights"""
    import dfot_amd
    kw = dict(external_cond_type="action", external_cond_dim=COND_DIM) if cond else {}
    params = fc.seeded_params(fac_keys(ratio, cond))
    model = dfot_amd.DiT3D(fac_cfg(ratio, cond), x_shape=X_SHAPE, max_tokens=MAX_TOKENS, **kw).cuda().eval()
    model.load_state_dict(params, strict=True)
    return model, params


def build_mat(tag):
    """the engine's FacMatDiT at the fixture's geometry with the seeded weights"""
    import dfot_amd
    params = fm.seeded_params(mat_keys(tag))
    model = dfot_amd.DiT3D(mat_cfg(tag), x_shape=X_SHAPE, max_tokens=MAX_TOKENS).cuda().eval()
    model.load_state_dict(params, strict=True)
    return model, params
