"""Host checks (no GPU) of the FacMatDiT backbone (DiT3D, variant "factorized_matrix_attention", pos_emb_type "sinusoidal_2d",
use_temporal_rope): the constructor's acceptance and refusals, the trainer's refusal, and the fixture tests/golden/dit_facmat.npz
(tools/make_golden_dit_facmat.py) against the torch restatement tests/dit_facmat_common.forward_host, which the GPU tests use at sizes
the fixture does not cover.

Bar of the restatement: both sides are fp32 torch on the same weights, so they differ by summation order only.  When the fixture was
made the largest relative L2 over all outputs was 2.9e-7 (stored as host_rel; the sibling restatement of tests/test_dit_fac_host.py
measured 2.4e-7); the assertion allows 1e-6, the bar of tests/test_dit_fac_host.py:15, about three times the measured value and 1e4 times
below the 2e-2 bar the GPU engine is held to.

The constructor and trainer tests fail on the parent commit: its DiT3D raises "unsupported DiT variant 'factorized_matrix_attention'" for
the recipe, its capi.DiTConfig has no use_temporal_rope field, and its DiT3DTrainer builds the difference model from this configuration."""
import ctypes

import numpy as np
import pytest
import torch

import dit_facmat_common as fm
from dit_facmat_common import T, rel

HOST_BAR = 1e-6


@pytest.fixture(scope="module")
def g():
    return fm.load("dit_facmat.npz")


def _cfg(**over):
    return {**fm.backbone_cfg(1, 4, False, 0.0, True), **over}


# ---------------------------------------------------------------------------------------------------------------- the constructor
def _engine_config(cfg, x_shape=(4, 16, 8), max_tokens=5):
    """DiT3D._configure on a bare instance: everything the constructor does before it touches the engine (no GPU needed)"""
    from dfot_amd import capi
    import dfot_amd
    c = capi.DiTConfig()
    c.patch_size = int(cfg["patch_size"])
    c.in_channels, c.height, c.width = x_shape
    model = dfot_amd.DiT3D.__new__(dfot_amd.DiT3D)
    model.x_shape = tuple(x_shape)
    dfot_amd.DiT3D._configure(model, c, cfg, max_tokens)
    return c


def test_constructor_accepts_the_recipe():
    c = _engine_config(_cfg())
    assert (c.variant, c.hidden_size, c.max_tokens, c.use_temporal_rope) == (3, 128, 5, 1)  # max_tokens is NOT doubled
    assert (c.embed_col_dim, c.num_col_heads, c.num_row_heads, c.use_bias) == (64, 1, 4, 0)
    assert (c.mlp_hidden, c.temporal_mlp_hidden) == (0, 512)
    c = _engine_config(fm.backbone_cfg(2, 2, True, 4.0, False))
    assert (c.variant, c.use_temporal_rope, c.use_bias, c.mlp_hidden, c.num_col_heads, c.num_row_heads) == (3, 0, 1, 512, 2, 2)
    # the @FacMatDiT/S-64-1 and XL-64-1 shortcuts at 32x32 latents, patch 2, 16 frames
    for row, heads, rr, depth in ((384, 6, 6, 6), (1152, 16, 16, 28)):
        c = _engine_config(_cfg(embed_row_dim=row, num_heads=heads, num_row_heads=rr, depth=depth, patch_size=2, spatial_mlp_ratio=4.0),
                           x_shape=(4, 32, 32), max_tokens=16)
        assert (c.variant, c.hidden_size, c.max_tokens, c.mlp_hidden) == (3, row, 16, 4 * row)
    # flatten_matrix_rope is only refused together with the rotation it would change
    assert _engine_config(_cfg(use_temporal_rope=False, flatten_matrix_rope=True)).use_temporal_rope == 0


def test_config_struct_ends_with_use_temporal_rope():
    from dfot_amd import capi
    assert capi.DiTConfig._fields_[-1][0] == "use_temporal_rope"
    assert capi.DiTConfig.use_temporal_rope.offset == ctypes.sizeof(capi.DiTConfig) - 4
    assert capi.DiTConfig().use_temporal_rope == 0  # every existing caller leaves it zero


@pytest.mark.parametrize("over,key", [
    (dict(matrix_multi_token=True), "matrix_multi_token"),
    (dict(flatten_matrix_rope=True), "flatten_matrix_rope"),
    (dict(fixed_u="identity"), "fixed_u"),
    (dict(matrix_block="matrix_cross"), "matrix_block"),
])
def test_unsupported_keys_are_refused_by_name(over, key):
    import dfot_amd
    with pytest.raises(ValueError, match=key):
        dfot_amd.DiT3D(_cfg(**over), x_shape=(4, 16, 8), max_tokens=5)


def test_unsupported_shapes_are_refused():
    import dfot_amd
    with pytest.raises(ValueError, match="multiple of 128"):  # 8x8 patches per frame = 64
        dfot_amd.DiT3D(_cfg(patch_size=2), x_shape=(4, 16, 16), max_tokens=5)
    with pytest.raises(ValueError, match="max_tokens 33"):
        dfot_amd.DiT3D(_cfg(), x_shape=(4, 16, 8), max_tokens=33)
    with pytest.raises(ValueError, match="sinusoidal_2d"):
        dfot_amd.DiT3D(_cfg(pos_emb_type="rope_3d"), x_shape=(4, 16, 8), max_tokens=5)
    # the sentence the other variants' refusals are matched against (tests/test_dit_fac_host.py:90) is still there
    with pytest.raises(ValueError, match="factorized_attention.*sinusoidal_factorized"):
        dfot_amd.DiT3D(_cfg(variant="full_matrix_attention"), x_shape=(4, 16, 8), max_tokens=5)


def test_trainer_refuses_the_rope_model_and_keeps_the_difference_model():
    import dfot_amd
    with pytest.raises(ValueError, match="no training path"):
        dfot_amd.DiT3DTrainer(_cfg(), x_shape=(4, 16, 8), max_tokens=5)


# ---------------------------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("tag,count", [("a", 46), ("b", 62), ("c", 50), ("d", 58)])
def test_key_list_and_order_equal_the_reference(g, tag, count):
    cc, rr, bias, ratio, rope = fm.CASES[tag]
    keys = fm.key_shapes(bias, ratio)
    assert [n for n, _ in keys] == [str(n) for n in g[f"names_{tag}"]]
    assert [" ".join(map(str, s)) for _, s in keys] == [str(s) for s in g[f"shapes_{tag}"]]
    assert len(keys) == count
    assert not any("rope" in n or "freqs" in n for n, _ in keys)  # the table is not a parameter
    assert fm.digest(fm.case_params(tag)) == str(g[f"digest_{tag}"])


def test_fixture_measured_the_restatement_below_the_bar(g):
    print(f"restatement vs the reference when the fixture was made: rel-L2 {float(g['host_rel']):.2e}")
    assert float(g["host_rel"]) < HOST_BAR / 2


@pytest.mark.parametrize("tag", list(fm.CASES))
def test_restatement_vs_reference_outputs(g, tag):
    cc, rr, bias, ratio, rope = fm.CASES[tag]
    params = fm.case_params(tag)
    x, k = T(g["x"]), T(g["k"])
    with torch.no_grad():
        for name, xx, kk in ((f"out_{tag}_t5", x, k), (f"out_{tag}_t3", x[:, :3], k[:, :3])):
            r = rel(fm.forward_host(params, xx, kk, cc, rr, rope, dtype=torch.float32), T(g[name]))
            print(f"{name}: restatement rel-L2 {r:.2e}")
            assert r < HOST_BAR
        r64 = rel(fm.forward_host(params, x, k, cc, rr, rope, dtype=torch.float64).float(), T(g[f"out_{tag}_t5"]))
        assert r64 < HOST_BAR


def test_rotation_and_frame_coupling_are_visible_in_the_fixture(g):
    cc, rr, bias, ratio, rope = fm.CASES["a"]
    params = fm.case_params("a")
    with torch.no_grad():
        o5 = fm.forward_host(params, T(g["x"]), T(g["k"]), cc, rr, True, dtype=torch.float32)
        plain = fm.forward_host(params, T(g["x"]), T(g["k"]), cc, rr, False, dtype=torch.float32)
        o4 = fm.forward_host(params, T(g["x_frame4"]), T(g["k"]), cc, rr, True, dtype=torch.float32)
    # a forward that skipped the rotation would miss the GPU parity bar (2e-2) by a factor of two
    np.testing.assert_allclose(rel(plain, o5), float(g["rope_effect"]), rtol=1e-4)
    assert float(g["rope_effect"]) > 2e-2
    assert rel(o4, T(g["out_a_frame4"])) < HOST_BAR
    assert torch.equal(T(g["x_frame4"])[:, :4], T(g["x"])[:, :4])
    moved = rel(o4[:, :4], o5[:, :4])
    np.testing.assert_allclose(moved, float(g["sens_frame4"]), rtol=1e-4)
    assert moved > 2 * 2e-2  # frames 0-3 move by more than twice the GPU parity bar


def test_restatement_conditioned(g):
    cc, rr, bias, ratio, rope = fm.CASES["a"]
    params = fm.case_params("a", cond=True)
    assert fm.digest(params) == str(g["digest_act"])
    assert [n for n in params] == [str(n) for n in g["names_act"]]
    x, k, cond, mask = T(g["x"]), T(g["k"]), T(g["act_cond"]), T(g["act_mask"])
    with torch.no_grad():
        assert rel(fm.forward_host(params, x, k, cc, rr, rope, cond, dtype=torch.float32), T(g["out_act"])) < HOST_BAR
        om = fm.forward_host(params, x, k, cc, rr, rope, cond, mask, dtype=torch.float32)
        assert rel(om, T(g["out_act_masked"])) < HOST_BAR
        plain = fm.forward_host(params, x, k, cc, rr, rope, dtype=torch.float32)
        assert rel(om[0], plain[0]) < HOST_BAR and rel(om[1], T(g["out_act"])[1]) < HOST_BAR


@pytest.mark.parametrize("dim", [32, 64, 72])
def test_engine_rope_table_equals_the_reference_angles(dim):
    """the (cos, sin) table the engine builds in float64 against the reference's fp32 angles: positions <= 31, so they agree to fp32 rounding"""
    ang = fm.rope_angles(32, dim)  # fp32, as the reference
    table = fm.rope_table(32, dim)
    assert tuple(table.shape) == (32, dim // 2, 2)
    assert torch.allclose(table[..., 0], ang[:, 0::2].cos(), atol=4e-6) and torch.allclose(table[..., 1], ang[:, 1::2].sin(), atol=4e-6)
    assert torch.equal(table[0, :, 0], torch.ones(dim // 2)) and torch.equal(table[0, :, 1], torch.zeros(dim // 2))


@pytest.mark.parametrize("tokens", [t for t in fm.OP_TOKENS if t >= 3])
def test_fp64_reference_with_rope_differs_from_the_one_without(tokens):
    """the op-level fp64 reference of tests/test_gpu_dit_facmat.py: with the rotation it differs from the plain one by rel-L2 >= 0.1 at
    L >= 3 -- otherwise a rotation that does nothing would pass the op test"""
    for cc, rr, h in fm.OP_HEADS:
        z = fm.make_z(2, tokens, cc, rr, h)
        with_rope, _ = fm.matrix_attention_ref(z, 2, tokens, fm.OP_E, h, cc, rr, True)
        plain, w = fm.matrix_attention_ref(z, 2, tokens, fm.OP_E, h, cc, rr, False)
        r = rel(with_rope, plain)
        print(f"L={tokens} (cc, rr, h)={(cc, rr, h)}: rope vs plain rel-L2 {r:.3f}, mean largest probability {float(w.max(-1).values.mean()):.3f}")
        assert r >= 0.1
