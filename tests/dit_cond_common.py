"""Shared helpers of tests/test_dit_cond_host.py and tests/test_gpu_dit_cond.py (not a test module): fixture access, model construction
for every condition mode of tests/golden/dit_cond.npz, and an fp64 restatement of the condition embedding."""
import os

import numpy as np
import torch

from conftest import GOLDEN

SMALL = dict(hidden_size=128, depth=2, num_heads=4, patch_size=1, in_channels=4, resolution=(16, 8), max_tokens=5)
DIFF_TINY = dict(hidden_size=128, depth=2, num_heads=4, in_channels=4, resolution=(16, 8), embed_col_dim=64, num_row_heads=4)
# mode -> (external_cond_type, external_cond_dim, num_classes, external_cond_dropout): as tools/make_golden_dit_cond.py
MODES = {"act_d0": ("action", 3, None, 0.0), "act_d1": ("action", 3, None, 0.1), "label": ("label", 1, 101, 0.0)}


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def cond_weights(g, prefix):
    """the condition-embedding tensors stored under '<prefix>/<state-dict key>'"""
    return {k[len(prefix) + 1:]: T(g[k]) for k in g.files if k.startswith(prefix + "/")}


def dit_cfg(dropout=0.0):
    cfg = dict(name="dit3d", variant="full", pos_emb_type="rope_3d", patch_size=1, hidden_size=128, depth=2, num_heads=4, mlp_ratio=4.0)
    if dropout:
        cfg["external_cond_dropout"] = dropout
    return cfg


def diff_cfg(dropout=0.0):
    cfg = dict(name="difference_dit3d", variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", merge_type="interleaved",
               patch_size=1, embed_col_dim=64, embed_row_dim=128, num_heads=4, num_col_heads=1, num_row_heads=4, depth=2, mlp_ratio=4.0,
               spatial_mlp_ratio=4.0, use_bias=True, matrix_block="matrix")
    if dropout:
        cfg["external_cond_dropout"] = dropout
    return cfg


def base_params(seed=2):
    from oracle import dit as odit
    return odit.seeded_params(odit.DiTConfig(**SMALL), seed)


def build_mode(mode, g=None):
    """the engine's DiT3D for one fixture mode, loaded with the shared seeded weights + the fixture's condition tensors; eval() as the
    reference's modules were when the fixtures were made (train() draws the per-video dropout of the condition embedding)"""
    import dfot_amd
    g = g if g is not None else load("dit_cond.npz")
    ctype, cdim, ncls, drop = MODES[mode]
    model = dfot_amd.DiT3D(dit_cfg(drop), x_shape=(4, 16, 8), max_tokens=5, external_cond_type=ctype, external_cond_num_classes=ncls,
                           external_cond_dim=cdim).cuda().eval()
    params = {**base_params(), **cond_weights(g, f"{mode}_cond")}
    model.load_state_dict(params, strict=True)
    return model, params


def build_plain():
    import dfot_amd
    model = dfot_amd.DiT3D(dit_cfg(), x_shape=(4, 16, 8), max_tokens=5).cuda()
    model.load_state_dict(base_params(), strict=True)
    return model


def build_diff(g=None):
    import dfot_amd
    from oracle import dit as odit
    g = g if g is not None else load("dit_cond.npz")
    model = dfot_amd.DifferenceDiT3D(diff_cfg(0.1), x_shape=(4, 16, 8), max_tokens=5, external_cond_type="action", external_cond_dim=3).cuda().eval()
    params = {**odit.diff_seeded_params(odit.DiffDiTConfig(**DIFF_TINY), 3), **cond_weights(g, "diff_act_cond")}
    model.load_state_dict(params, strict=True)
    return model, params


def action_embedding_fp64(w, cond, prefix="external_cond_embedding"):
    """Linear -> SiLU -> Linear of the reference's TimestepEmbedding in float64"""
    p = {k: v.double() for k, v in w.items()}
    h = torch.nn.functional.silu(cond.double() @ p[f"{prefix}.linear_1.weight"].T + p[f"{prefix}.linear_1.bias"])
    return h @ p[f"{prefix}.linear_2.weight"].T + p[f"{prefix}.linear_2.bias"]
