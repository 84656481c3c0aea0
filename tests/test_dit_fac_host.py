"""Host checks (no GPU) of the factorized-attention DiT3D fixture tests/golden/dit_fac.npz (tools/make_golden_dit_fac.py): the torch
restatement tests/dit_fac_common.forward_host, which the GPU tests use at sizes the fixture does not cover, against every output the
reference produced; the state-dict key list and order; the temporal sinusoidal table.

Bar of the restatement: both sides are fp32 torch on the same weights, so they differ by summation order only.  When the fixture was made
the largest relative L2 over all outputs was 2.4e-7 (stored as host_rel); the assertion allows 1e-6, about four times that and still 1e4
times below the 2e-2 bar the GPU engine is held to."""
import numpy as np
import pytest
import torch

import dit_fac_common as fc
from dit_fac_common import T, rel

HOST_BAR = 1e-6


@pytest.fixture(scope="module")
def g():
    return fc.load("dit_fac.npz")


def params_for(g, tag, ratio, cond=False):
    keys = fc.key_shapes(ratio, fc.COND_DIM if cond else 0, fc.COND_DROPOUT if cond else 0.0)
    params = fc.seeded_params(keys)
    assert fc.digest(params) == str(g[f"digest_{tag}"])
    return params


@pytest.mark.parametrize("tag,ratio,cond,count", [("mlp0", 0.0, False, 46), ("mlp4", 4.0, False, 58), ("act", 0.0, True, 50)])
def test_key_list_and_order_equal_the_reference(g, tag, ratio, cond, count):
    keys = fc.key_shapes(ratio, fc.COND_DIM if cond else 0, fc.COND_DROPOUT if cond else 0.0)
    assert [n for n, _ in keys] == [str(n) for n in g[f"names_{tag}"]]
    assert [" ".join(map(str, s)) for _, s in keys] == [str(s) for s in g[f"shapes_{tag}"]]
    assert len(keys) == count


def test_fixture_measured_the_restatement_below_the_bar(g):
    assert float(g["host_rel"]) < HOST_BAR / 2


@pytest.mark.parametrize("tag,ratio", [("mlp0", 0.0), ("mlp4", 4.0)])
def test_restatement_vs_reference_outputs(g, tag, ratio):
    params = params_for(g, tag, ratio)
    x, k = T(g["x"]), T(g["k"])
    with torch.no_grad():
        for name, xx, kk in ((f"out_{tag}_t5", x, k), (f"out_{tag}_t3", x[:, :3], k[:, :3])):
            r = rel(fc.forward_host(params, xx, kk, dtype=torch.float32), T(g[name]))
            print(f"{name}: restatement rel-L2 {r:.2e}")
            assert r < HOST_BAR
        r64 = rel(fc.forward_host(params, x, k, dtype=torch.float64).float(), T(g[f"out_{tag}_t5"]))
        assert r64 < HOST_BAR


def test_restatement_frame4_sensitivity(g):
    params = params_for(g, "mlp0", 0.0)
    with torch.no_grad():
        o5 = fc.forward_host(params, T(g["x"]), T(g["k"]), dtype=torch.float32)
        o4 = fc.forward_host(params, T(g["x_frame4"]), T(g["k"]), dtype=torch.float32)
    assert rel(o4, T(g["out_mlp0_frame4"])) < HOST_BAR
    assert torch.equal(T(g["x_frame4"])[:, :4], T(g["x"])[:, :4])
    moved = rel(o4[:, :4], o5[:, :4])
    np.testing.assert_allclose(moved, float(g["sens_frame4"]), rtol=1e-4)
    assert moved > 2 * 2e-2  # the temporal path is live: frames 0-3 move by more than twice the GPU parity bar


def test_restatement_conditioned(g):
    params = params_for(g, "act", 0.0, cond=True)
    x, k, cond, mask = T(g["x"]), T(g["k"]), T(g["act_cond"]), T(g["act_mask"])
    with torch.no_grad():
        assert rel(fc.forward_host(params, x, k, cond, dtype=torch.float32), T(g["out_act"])) < HOST_BAR
        om = fc.forward_host(params, x, k, cond, mask, dtype=torch.float32)
        assert rel(om, T(g["out_act_masked"])) < HOST_BAR
        # the masked video runs without its condition, the other one with it
        plain = fc.forward_host(params, x, k, dtype=torch.float32)
        assert rel(om[0], plain[0]) < HOST_BAR and rel(om[1], T(g["out_act"])[1]) < HOST_BAR


@pytest.mark.parametrize("t", [3, 5])
def test_temporal_table_equals_the_reference(g, t):
    table = fc.temporal_table(5, 128)
    assert torch.equal(table[:t], T(g["tpos_t5"])[:t])


def test_unsupported_configurations_are_refused_by_name():
    """constructor checks that run before the engine is touched (no GPU needed)"""
    import dfot_amd
    for over in (dict(variant="factorized_encoder"), dict(variant="full_matrix_attention"), dict(pos_emb_type="rope_3d"),
                 dict(pos_emb_type="sinusoidal_3d")):
        with pytest.raises(ValueError, match="factorized_attention.*sinusoidal_factorized"):
            dfot_amd.DiT3D({**fc.backbone_cfg(0.0), **over}, x_shape=(4, 16, 8), max_tokens=5)
    with pytest.raises(ValueError, match="multiple of 128"):  # 8x8 patches per frame = 64
        dfot_amd.DiT3D(fc.backbone_cfg(0.0, patch_size=2), x_shape=(4, 16, 16), max_tokens=5)
    with pytest.raises(ValueError, match="32 frames"):
        dfot_amd.DiT3D(fc.backbone_cfg(0.0), x_shape=(4, 16, 8), max_tokens=33)
