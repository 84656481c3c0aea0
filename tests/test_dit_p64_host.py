"""Host checks (no GPU) of the 64-patches-per-frame fixture tests/golden/dit_p64.npz (tools/make_golden_dit_p64.py) and of the refusals
around that shape: the torch restatements of dit_fac_common / dit_facmat_common at the fixture's geometry against every output the
reference produced; the patch-count rule of DiT3D, DifferenceDiT3D and the two trainers by name; the new op's declaration and binding.

Bar of the restatements: both sides are fp32 torch on the same weights, so they differ by summation order only.  When the fixture was made
the largest relative L2 over all outputs was 2.2e-7 (stored as host_rel); the assertion allows 1e-6 (the bar of tests/test_dit_fac_host.py),
still 1e4 times below the 2e-2 bar the GPU engine is held to."""
import os
import re

import numpy as np
import pytest
import torch

import dit_fac_common as fc
import dit_facmat_common as fm
import dit_p64_common as pc
from dit_p64_common import T, rel

HOST_BAR = 1e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return pc.load(pc.FIXTURE)


def _case(g, tag):
    """(seeded weights, fp32 / fp64 host forward) of a fixture model, the digest checked"""
    kind, case = tag.split("_")
    if kind == "fac":
        keys = pc.fac_keys(pc.FAC_CASES[case])
        params = fc.seeded_params(keys)
        host = lambda x, k, dtype: pc.fac_host(params, x, k, dtype=dtype)  # noqa: E731
    else:
        keys = pc.mat_keys(case)
        params = fm.seeded_params(keys)
        host = lambda x, k, dtype: pc.mat_host(case, params, x, k, dtype=dtype)  # noqa: E731
    assert pc.digest(params) == str(g[f"digest_{tag}"])
    assert [n for n, _ in keys] == [str(n) for n in g[f"names_{tag}"]]
    assert [" ".join(map(str, s)) for _, s in keys] == [str(s) for s in g[f"shapes_{tag}"]]
    return params, host


def test_fixture_is_small_and_measured_the_restatement_below_the_bar(g):
    assert os.path.getsize(os.path.join(fc.GOLDEN, pc.FIXTURE)) < 1 << 20
    assert float(g["host_rel"]) < HOST_BAR / 2
    assert tuple(g["x"].shape) == (pc.BATCH, pc.MAX_TOKENS, *pc.X_SHAPE) and tuple(g["k"].shape) == (pc.BATCH, pc.MAX_TOKENS)
    assert (pc.X_SHAPE[1] // pc.OVER["patch_size"]) * (pc.X_SHAPE[2] // pc.OVER["patch_size"]) == 64


@pytest.mark.parametrize("tag", ["fac_mlp0", "fac_mlp4", "mat_b", "mat_d"])
def test_restatement_vs_reference_outputs(g, tag):
    _, host = _case(g, tag)
    x, k = T(g["x"]), T(g["k"])
    with torch.no_grad():
        for name, xx, kk in ((f"out_{tag}_t4", x, k), (f"out_{tag}_t2", x[:, :2], k[:, :2])):
            r = rel(host(xx, kk, torch.float32), T(g[name]))
            print(f"{name}: restatement rel-L2 {r:.2e}")
            assert r < HOST_BAR
        assert rel(host(x, k, torch.float64).float(), T(g[f"out_{tag}_t4"])) < HOST_BAR


@pytest.mark.parametrize("tag,sens_key", [("fac_mlp0", "sens_frame3"), ("mat_b", "sens_frame3_mat")])
def test_restatement_frame3_sensitivity(g, tag, sens_key):
    _, host = _case(g, tag)
    with torch.no_grad():
        o4 = host(T(g["x"]), T(g["k"]), torch.float32)
        o3 = host(T(g["x_frame3"]), T(g["k"]), torch.float32)
    assert rel(o3, T(g[f"out_{tag}_frame3"])) < HOST_BAR
    assert torch.equal(T(g["x_frame3"])[:, :3], T(g["x"])[:, :3]) and not torch.equal(T(g["x_frame3"])[:, 3], T(g["x"])[:, 3])
    moved = rel(o3[:, :3], o4[:, :3])
    np.testing.assert_allclose(moved, float(g[sens_key]), rtol=1e-4)
    assert moved > 2 * pc.FIXTURE_BAR  # the frame-mixing path is live: frames 0-2 move by more than twice the GPU parity bar


def test_restatement_conditioned(g):
    keys = pc.fac_keys(0.0, cond=True)
    params = fc.seeded_params(keys)
    assert pc.digest(params) == str(g["digest_fac_act"])
    assert [n for n, _ in keys] == [str(n) for n in g["names_fac_act"]]
    x, k, cond, mask = T(g["x"]), T(g["k"]), T(g["act_cond"]), T(g["act_mask"])
    with torch.no_grad():
        assert rel(pc.fac_host(params, x, k, cond, dtype=torch.float32), T(g["out_act"])) < HOST_BAR
        om = pc.fac_host(params, x, k, cond, mask, dtype=torch.float32)
        assert rel(om, T(g["out_act_masked"])) < HOST_BAR
        plain = pc.fac_host(params, x, k, dtype=torch.float32)
        assert rel(om[0], plain[0]) < HOST_BAR and rel(om[1], T(g["out_act"])[1]) < HOST_BAR


@pytest.mark.parametrize("variant", ["fac", "facmat"])
def test_host_frame_maps_are_maps_and_far_from_uniform(g, variant):
    """what tests/test_gpu_dit_p64.py compares the captured maps with: rows sum to 1, the shape is the engine's, and every map is more than
    twice the parity bar away from the uniform map and from its own transpose (a wrong binning or a swapped axis would show)"""
    params, real = _case(g, "fac_mlp0" if variant == "fac" else "mat_b")[0], torch.softmax
    with torch.no_grad():
        maps = pc.host_frame_maps(variant, params, T(g["x"]), T(g["k"]))
    cc, rr = fm.CASES["b"][:2]
    want = (pc.BATCH, cc, rr, pc.MAX_TOKENS, pc.MAX_TOKENS) if variant == "facmat" else (pc.BATCH, 4, pc.MAX_TOKENS, pc.MAX_TOKENS)
    assert list(maps) == [f"dit_base.temporal_blocks.{i}.attn" for i in range(2)]
    for name, w in maps.items():
        assert tuple(w.shape) == want and w.dtype == torch.float64
        assert (w.sum(-1) - 1).abs().max().item() < 1e-12
        assert rel(w, torch.full_like(w, 1.0 / pc.MAX_TOKENS)) > pc.CONTRAST_BAR, name
        assert rel(w, w.transpose(-1, -2)) > pc.CONTRAST_BAR, name
    assert torch.softmax is real  # the recorder is gone


# ---------------------------------------------------------------------------------------------------------------- refusals by name
@pytest.mark.parametrize("cfg", [pc.fac_cfg(0.0), pc.mat_cfg("b")], ids=["fac", "facmat"])
def test_dit3d_refuses_an_odd_max_tokens_at_64_patches(cfg):
    import dfot_amd
    for mt, rows in ((5, 320), (15, 960)):
        with pytest.raises(ValueError, match=rf"max_tokens {mt} × 64 patches per frame = {rows} rows per window; the row tiles need a multiple of 128"):
            dfot_amd.DiT3D(cfg, x_shape=pc.X_SHAPE, max_tokens=mt)


@pytest.mark.parametrize("kind", ["fac", "facmat"])
@pytest.mark.parametrize("x_shape,patches", [((4, 8, 8), 16), ((4, 16, 8), 32), ((4, 32, 24), 192)])
def test_dit3d_refuses_other_patch_counts(kind, x_shape, patches):
    import dfot_amd
    over = dict(resolution=x_shape[1:])
    cfg = pc.fac_cfg(0.0, **over) if kind == "fac" else pc.mat_cfg("b", **over)
    with pytest.raises(ValueError, match=rf"gives {patches} patches per frame; .* need a multiple of 128"):
        dfot_amd.DiT3D(cfg, x_shape=x_shape, max_tokens=4)


def test_difference_dit3d_refuses_64_patches():
    import __graft_entry__ as ge
    ge.build()
    import dfot_amd
    cfg = dict(name="difference_dit3d", variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", merge_type="interleaved", patch_size=2,
               embed_col_dim=64, embed_row_dim=128, num_heads=4, num_col_heads=1, num_row_heads=4, depth=1, mlp_ratio=4.0, spatial_mlp_ratio=4.0,
               use_bias=True, matrix_block="matrix")
    with pytest.raises(RuntimeError, match="factorized matrix variant: 64 patches per frame must be a multiple of 128$"):
        dfot_amd.DifferenceDiT3D(cfg, x_shape=pc.X_SHAPE, max_tokens=2)


def test_trainers_refuse_64_patches_in_the_wording_they_had():
    import dfot_amd
    with pytest.raises(ValueError, match=r"64 patches per frame; the per-frame attention kernels need a multiple of 128 \(the 64-patch recipes are "
                                         r"not supported\)"):
        dfot_amd.FacDiTTrainer(pc.fac_cfg(0.0), x_shape=pc.X_SHAPE, max_tokens=16)
    with pytest.raises(ValueError, match=r"64 patches per frame; the per-frame kernels need a multiple of 128 \(the 64-patch recipes are not "
                                         r"supported\)"):
        dfot_amd.FacMatDiTTrainer(pc.mat_cfg("b"), x_shape=pc.X_SHAPE, max_tokens=16)


def test_header_and_capi_declare_the_new_op():
    import __graft_entry__ as ge
    ge.build()
    from dfot_amd import capi
    hdr = open(os.path.join(ROOT, "include", "dfot_hip.h")).read()
    name = "dfot_op_attention_seq64"
    assert re.search(r"\b" + name + r"\s*\(", hdr)
    assert name in capi.SIGNATURES and hasattr(capi.lib, name)
    assert len(capi.SIGNATURES[name][1]) == 9
    # refusals come before any device work, so they need no GPU: null pointers, then a head dim that is no multiple of 8
    assert capi.lib.dfot_op_attention_seq64(None, None, None, None, 64, 1, 1, 64, None) == capi.ERR_ARG
    assert b"attention_seq64" in capi.lib.dfot_last_error()
