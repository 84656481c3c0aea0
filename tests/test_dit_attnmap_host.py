"""Host (no GPU) tests of the attention-map read-out: the conditions the fixture tests/golden/dit_attnmap.npz must meet to catch the
likely mistakes, the two pure-torch helpers against what the reference stored, and the C ABI's declarations and bindings."""
import os
import re

import torch

import dit_attnmap_common as am
from conftest import ROOT
from dit_attnmap_common import T, rel


def _fixture():
    return am.load("dit_attnmap.npz")


def _frame_maps(g):
    for v in am.VARIANTS:
        for i in range(am.DEPTH):
            yield f"frame_{v}_{i}", v, T(g[f"frame_{v}_{i}"])
    yield "full_hook_frame", None, T(g["full_hook_frame"])


def test_fixture_is_small_and_complete():
    path = os.path.join(ROOT, "tests", "golden", "dit_attnmap.npz")
    assert os.path.getsize(path) < 512 * 1024
    g = _fixture()
    for name, v, f in _frame_maps(g):
        if v is not None:
            assert tuple(f.shape) == am.map_shape(v, 2), name
        assert float((f.double().sum(-1) - 1).abs().max()) < 1e-5, name  # rows of a frame map sum to 1
    assert tuple(g["full_hook"].shape) == (am.FULL_TOKENS, am.HEIGHT, am.WIDTH, am.FULL_TOKENS * am.PATCHES)


def test_fixture_maps_are_far_from_uniform_and_from_their_transpose():
    """rel-L2 >= 4e-2 (twice the GPU parity bar) both ways, for every stored frame map: a uniform map, a wrong frame binning or a swapped
    query / key axis cannot pass the parity test"""
    g = _fixture()
    for name, _, f in _frame_maps(g):
        uniform, transposed = am.contrast(f)
        print(f"{name}: rel-L2 against uniform {uniform:.3e}, against the transpose {transposed:.3e}")
        assert uniform >= am.CONTRAST_BAR and transposed >= am.CONTRAST_BAR, name


def test_bf16_restatement_figures_leave_half_the_bar():
    """measured by the tool on the CPU: the forward restated with the engine's bf16 roundings stays within 1e-2 of the fp32 maps"""
    g = _fixture()
    for key in [f"restate_{v}" for v in am.VARIANTS] + ["restate_full_map"]:
        print(f"{key}: {float(g[key]):.3e}")
        assert 0 < float(g[key]) <= am.RESTATE_BAR, key


def test_seeded_weights_match_the_fixture_digests():
    g = _fixture()
    for v in am.VARIANTS:
        assert am.fm.digest(am.seeded(v, float(g[f"gain_{v}"]))) == str(g[f"digest_{v}"]), v


def test_frame_map_and_hook_layout_against_what_the_reference_stored():
    import dfot_amd
    g = _fixture()
    hook = T(g["full_hook"])  # (t, h, w, N) of one head, as Attention.forward stored it
    n = hook.shape[-1]
    full = hook.reshape(n, n)
    assert torch.equal(dfot_amd.to_hook_layout(full[None, None], am.FULL_TOKENS, am.HEIGHT, am.WIDTH)[0, 0], hook)
    f = dfot_amd.frame_map(full.double(), am.FULL_TOKENS)
    assert rel(f, T(g["full_hook_frame"])) < 1e-6
    # the definition, spelled out: (1/P) sum over the query rows of frame tq and the key columns of frame tk
    p = am.PATCHES
    for tq in range(am.FULL_TOKENS):
        for tk in range(am.FULL_TOKENS):
            want = full[tq * p:(tq + 1) * p, tk * p:(tk + 1) * p].double().sum() / p
            assert abs(float(f[tq, tk] - want)) < 1e-9
    # leading axes pass through; a map whose N is not a multiple of tokens is refused
    batch = torch.rand(2, 3, 12, 12)
    assert tuple(dfot_amd.frame_map(batch, 4).shape) == (2, 3, 4, 4)
    assert torch.allclose(dfot_amd.frame_map(batch, 1)[..., 0, 0], batch.sum((-1, -2)) / 12)
    for bad in (lambda: dfot_amd.frame_map(batch, 5), lambda: dfot_amd.to_hook_layout(batch, 2, 3, 3)):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError("expected ValueError")


def test_header_and_capi_declare_the_new_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from dfot_amd import capi
    hdr = open(os.path.join(ROOT, "include", "dfot_hip.h")).read()
    names = ("dfot_op_attention_map", "dfot_op_attention_map_workspace_bytes", "dfot_op_attention_temporal_map", "dfot_op_matrix_attention_map",
             "dfot_dit_capture_attention", "dfot_dit_attention_map_shape", "dfot_dit_read_attention_map")
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in capi.SIGNATURES and hasattr(capi.lib, name), name
    assert len(capi.SIGNATURES["dfot_op_attention_map"][1]) == 12
    assert len(capi.SIGNATURES["dfot_op_attention_temporal_map"][1]) == 11
    assert len(capi.SIGNATURES["dfot_op_matrix_attention_map"][1]) == 11
    assert (capi.ATTN_MAP_OFF, capi.ATTN_MAP_FRAME, capi.ATTN_MAP_FULL) == (-1, 0, 1)
    for text in ("DFOT_ATTN_MAP_OFF = -1", "DFOT_ATTN_MAP_FRAME = 0", "DFOT_ATTN_MAP_FULL = 1"):
        assert text in hdr
    # the workspace query needs no GPU
    assert capi.lib.dfot_op_attention_map_workspace_bytes(0, 2, 2, 3, 128) == 4 * 2 * 2 * (384 // 32) * 3
    assert capi.lib.dfot_op_attention_map_workspace_bytes(1, 2, 2, 32, 64) == 4 * 2 * 2 * 1 * 32 * 32
    assert capi.lib.dfot_op_attention_map_workspace_bytes(0, 0, 2, 3, 128) == 0


def test_sampler_config_default_changes_nothing():
    import dfot_amd
    assert dfot_amd.SamplerConfig().attention_map_steps == ()
