"""Shared helpers of tests/test_dit_facmat_narrow_host.py, tests/test_gpu_dit_facmat_narrow.py, tests/test_gpu_facmat_narrow_ops.py and
tools/make_golden_dit_facmat_narrow.py (not a test module): FacMatDiT at narrow column widths, 1 <= embed_col_dim <= 32 -- the rungs
S-1-1 .. S-32-4 of the @FacMatDiT ladder, whose left factors run csrc/facmat_narrow.hip instead of the factor GEMMs.

Everything about the model itself -- key order, seeded weights, the host restatement -- is tests/dit_facmat_common.py with the width (and, at
64 patches per frame, the geometry of tests/dit_p64_common.py) passed through its **over hooks.  Here: the cases, the gain on the q / k
columns of the matrix blocks' right factor, the builders, the frame maps of the restatement, and the fp64 references of the two ops."""
import torch

import dit_facmat_common as fm
import dit_p64_common as pc
from dit_fac_common import COND_DIM, COND_DROPOUT, T, digest, load, rel  # noqa: F401

FIXTURE = "dit_facmat_narrow.npz"
FIXTURE_BAR = pc.FIXTURE_BAR    # 2e-2, tests/dit_p64_common.py:16
MAP_BAR = pc.MAP_BAR            # 2e-2
CONTRAST_BAR = pc.CONTRAST_BAR  # 4e-2
RR = 4                          # row heads of every case (embed_row_dim 128: row head dim 32)

# tag -> (embed_col_dim, num_col_heads, use_bias, use_temporal_rope).  At batch 2 the right-factor GEMM has frames * E = 10, 80, 160, 320, 30
# rows at T = 5: whole 128-row tiles in no case; the matrix biases differ per e, so an e-index or pad-row mistake shows
CASES = {
    "e1": (1, 1, True, True),
    "e8": (8, 1, True, True),
    "e16": (16, 1, False, False),
    "e32": (32, 4, True, True),
    "e3": (3, 1, True, False),
}
SPATIAL_MLP_RATIO = {"e1": 0.0, "e8": 4.0, "e16": 0.0, "e32": 4.0, "e3": 0.0}
P64_TAGS = ("e8", "e32")  # also at 64 patches per frame (latents 4x16x16 at patch 2, max_tokens 4)
COND_TAG = "e8"           # the action-conditioned case
TRACE_TAG = "e8"          # the sampler trace
GAINS = (1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0)  # tools/make_golden_dit_attnmap.py's ladder, continued

# geometry: 128 patches = tests/dit_facmat_common.TINY as it is (latents 4x16x8, patch 1, max_tokens 5); 64 patches = dit_p64_common.OVER
GEOM = {128: dict(over={}, x_shape=(4, 16, 8), max_tokens=5), 64: dict(over=dict(pc.OVER), x_shape=pc.X_SHAPE, max_tokens=pc.MAX_TOKENS)}


def over(tag, patches=128):
    return {**GEOM[patches]["over"], "embed_col_dim": CASES[tag][0]}


def keys(tag, patches=128, cond=False):
    return fm.key_shapes(CASES[tag][2], SPATIAL_MLP_RATIO[tag], COND_DIM if cond else 0, COND_DROPOUT if cond else 0.0, **over(tag, patches))


def cfg(tag, patches=128, cond=False):
    e, cc, bias, rope = CASES[tag]
    return fm.backbone_cfg(cc, RR, bias, SPATIAL_MLP_RATIO[tag], rope, COND_DROPOUT if cond else 0.0, **over(tag, patches))


def seeded(tag, gain, patches=128, cond=False):
    """the seeded weights of dit_facmat_common with the q | k columns of every matrix block's right factor scaled by `gain` (the scores
    scale by gain^2), the rule of tests/dit_attnmap_common.seeded: small random weights give near-uniform frame maps, and at E = 1 a score
    is one h/rr-long dot product"""
    params = fm.seeded_params(keys(tag, patches, cond))
    h = fm.TINY["hidden_size"]
    for i in range(fm.TINY["depth"]):
        params[f"dit_base.temporal_blocks.{i}.attn.qkv_v"][:, : 2 * h] *= gain
    return params


def host(tag, params, x, k, cond=None, mask=None, patches=128, dtype=torch.float64):
    e, cc, bias, rope = CASES[tag]
    return fm.forward_host(params, x, k, cc, RR, rope, cond, mask, dtype=dtype, **over(tag, patches))


def host_frame_maps(tag, params, x, k, patches=128, dtype=torch.float64):
    """{block name: frame map [b][col heads][row heads][T][T]} of the restated forward: the odd-numbered softmax results (spatial block, then
    matrix block per depth), as tests/dit_p64_common.host_frame_maps"""
    seen, real = [], torch.softmax

    def recording(*a, **kw):
        seen.append(real(*a, **kw))
        return seen[-1]
    torch.softmax = recording
    try:
        host(tag, params, x, k, patches=patches, dtype=dtype)
    finally:
        torch.softmax = real
    depth = fm.TINY["depth"]
    assert len(seen) == 2 * depth
    return {f"dit_base.temporal_blocks.{i}.attn": seen[2 * i + 1] for i in range(depth)}


def contrast(w):
    """(rel-L2 of a frame map against the uniform map, against its own transpose)"""
    return rel(w, torch.full_like(w, 1.0 / w.shape[-1])), rel(w, w.transpose(-1, -2))


def inputs(g, patches=128):
    return (T(g["x"]), T(g["k"])) if patches == 128 else (T(g["x64"]), T(g["k64"]))


def build(tag, gain, patches=128, cond=False):
    """the engine's DiT3D at a fixture case with the seeded weights, eval() as the reference's module was"""
    import dfot_amd
    kw = dict(external_cond_type="action", external_cond_dim=COND_DIM) if cond else {}
    params = seeded(tag, gain, patches, cond)
    geo = GEOM[patches]
    model = dfot_amd.DiT3D(cfg(tag, patches, cond), x_shape=geo["x_shape"], max_tokens=geo["max_tokens"], **kw).cuda().eval()
    model.load_state_dict(params, strict=True)
    return model, params


# ---- the two ops: fp64 references on bf16-rounded operands ---------------------------------------------------------------------------
OP_FRAMES, OP_P, OP_H, OP_E = (1, 3, 10), (64, 128, 384), (128, 384, 1152), (1, 3, 8, 16, 32)


def op_operands(frames, p, h, e, seed=0):
    """(m [frames][P][h], u_contract [E][P], o [frames][E][h], u_expand [P][E]) unit normal (u scaled to unit-variance sums), rounded to bf16"""
    g = torch.Generator().manual_seed(seed + 7 * frames + 11 * p + 13 * h + 17 * e)
    bf = lambda t: t.to(torch.bfloat16)  # noqa: E731
    return (bf(torch.randn(frames, p, h, generator=g)), bf(torch.randn(e, p, generator=g) / p ** 0.5),
            bf(torch.randn(frames, e, h, generator=g)), bf(torch.randn(p, e, generator=g) / e ** 0.5))


def contract_ref(m, u):
    """w[f][e][d] = sum_p u[e][p] m[f][p][d] in fp64"""
    return torch.einsum("ep,fpd->fed", u.double(), m.double())


def expand_ref(o, u):
    """s[f][p][d] = sum_e u[p][e] o[f][e][d] in fp64"""
    return torch.einsum("pe,fed->fpd", u.double(), o.double())
