"""Host checks (no GPU) of the DiT1D fixture tests/golden/dit1d.npz (tools/make_golden_dit1d.py) and of the refusals around the backbone:
the torch restatement dit1d_common.forward_host against every output the reference produced, the recorded sensitivities of the wrong masks
and of the wrong residual base, the sin-cos table, every constructor refusal by name, the new C symbols and their argument checks.

Bar of the restatement: fp64 against fp32 outputs of the same arithmetic, 1e-5 (the fp32 run in the tool gave host_rel, stored).  The
sensitivities are properties of the weights: each must reach dit1d_common.SENS_FLOOR = 0.1 = 5 x the 2e-2 parity bar of the GPU forward,
so that an engine with a wrong mask or residual base stays at least four bars away from passing; forward_host reproduces each to 1e-3."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dit1d_common as dc
from dit1d_common import T, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_BAR = 1e-5


@pytest.fixture(scope="module")
def g():
    return dc.load()


@pytest.fixture(scope="module")
def host_outputs(g):
    """fp64 forward_host of both cases under every variation, computed once"""
    x, k = dc.inputs()
    assert dc.tensor_digest(x, k) == str(g["inputs_digest"])
    out = {}
    with torch.no_grad():
        for tag, heads in dc.CASES.items():
            params = dc.seeded_params(dc.key_shapes(heads), float(g["qk_gain"]))
            assert dc.digest(params) == str(g[f"digest_{tag}"])
            out[tag, "causal"] = dc.forward_host(params, x, k, heads)
            for name, kw in dc.SENSITIVITIES.items():
                out[tag, name] = dc.forward_host(params, x, k, heads, **kw)
    return out


def test_fixture_is_small_and_holds_what_the_tests_need(g):
    assert os.path.getsize(os.path.join(dc.GOLDEN, dc.FIXTURE)) < 1 << 20
    assert float(g["host_rel"]) < HOST_BAR
    assert int(g["same_modes"]) == 1  # temporal_causal and video_temporal_causal: one mask without context tokens
    for tag in dc.CASES:
        assert tuple(g[f"out_causal_{tag}"].shape) == tuple(g[f"out_nomask_{tag}"].shape) == (dc.BATCH, dc.MAX_TOKENS, *dc.X_SHAPE)


@pytest.mark.parametrize("tag", list(dc.CASES))
def test_key_shapes_equal_the_reference_key_list(g, tag):
    keys = dc.key_shapes(dc.CASES[tag])
    assert [n for n, _ in keys] == [str(n) for n in g[f"names_{tag}"]]
    assert [" ".join(map(str, s)) for _, s in keys] == [str(s) for s in g[f"shapes_{tag}"]]
    assert keys[0][0] == "pos_embed" and keys[-1][0] == "final_layer.1.bias"


@pytest.mark.parametrize("tag", list(dc.CASES))
def test_restatement_vs_reference_outputs(g, host_outputs, tag):
    rc = rel(host_outputs[tag, "causal"], T(g[f"out_causal_{tag}"]))
    rn = rel(host_outputs[tag, "sens_nomask"], T(g[f"out_nomask_{tag}"]))
    print(f"{tag}: fp64 restatement vs the reference rel-L2 causal {rc:.2e}, no mask {rn:.2e} (fp32 in the tool: {float(g['host_rel']):.2e})")
    assert rc < HOST_BAR and rn < HOST_BAR


@pytest.mark.parametrize("name", list(dc.SENSITIVITIES))
def test_sensitivities_reach_the_floor_and_are_reproduced(g, host_outputs, name):
    want = float(g[name])
    got = min(rel(host_outputs[tag, name], T(g[f"out_causal_{tag}"])) for tag in dc.CASES)
    print(f"{name}: recorded {want:.4f}, forward_host {got:.4f}")
    assert want >= dc.SENS_FLOOR
    assert abs(got - want) < 1e-3


def test_sincos_table_equals_the_formula(g):
    """what a fresh model's pos_embed holds: the backbone's table, the [sin | cos] formula and the reference's own function agree"""
    import dfot_amd
    from dfot_amd.dit1d_backbone import sincos_pos_embed_1d
    hidden, tokens = int(g["sincos_hidden"]), int(g["sincos_tokens"])
    ref = np.asarray(g["sincos"])
    assert ref.shape == (tokens, hidden)
    assert np.abs(dc.sincos_formula(hidden, tokens) - ref).max() < 1e-12
    table = sincos_pos_embed_1d(hidden, tokens)
    assert tuple(table.shape) == (1, tokens, hidden) and table.dtype == torch.float32
    assert (table[0].double() - torch.from_numpy(ref)).abs().max() < 1e-7  # fp32 rounding of values in [-1, 1]
    big = sincos_pos_embed_1d(128, dc.MAX_TOKENS * dc.X_SHAPE[2])[0].double().numpy()
    assert np.abs(big - dc.sincos_formula(128, dc.MAX_TOKENS * dc.X_SHAPE[2])).max() < 1e-7
    assert np.abs(big[:, :64] - np.sin(np.arange(256)[:, None] * 10000.0 ** (-np.arange(64) / 64.0))).max() < 1e-6  # [sin | ...
    # a fresh model (built on the host: the engine handle is created at the first weight sync) holds that table, frozen, under the
    # reference's key list
    fresh = dfot_amd.DiT1D(dc.backbone_cfg(4), x_shape=dc.X_SHAPE, max_tokens=dc.MAX_TOKENS)
    assert tuple(fresh.pos_embed.shape) == (1, dc.MAX_TOKENS * dc.X_SHAPE[2], 128) and not fresh.pos_embed.requires_grad
    assert np.abs(fresh.pos_embed[0].double().numpy() - dc.sincos_formula(128, dc.MAX_TOKENS * dc.X_SHAPE[2])).max() < 1e-7
    assert list(fresh.state_dict().keys()) == [str(n) for n in g["names_h4"]]
    assert [" ".join(map(str, t.shape)) for t in fresh.state_dict().values()] == [str(s) for s in g["shapes_h4"]]
    assert all(p.requires_grad for n, p in fresh.named_parameters() if n != "pos_embed")
    assert fresh.num_patches == dc.X_SHAPE[2] and fresh.max_tokens == dc.MAX_TOKENS and fresh.x_shape == dc.X_SHAPE


REFUSALS = [
    (dict(merge_mode="separate_norm"), {}, "merge_mode"),
    (dict(merge_mode="reproduce"), {}, "merge_mode"),
    (dict(use_rotary_emb=True), {}, "use_rotary_emb"),
    (dict(qk_norm=True), {}, "qk_norm"),
    (dict(learn_sigma=True), {}, "learn_sigma"),
    (dict(causal_attn_mode="full_causal"), {}, "causal_attn_mode"),
    ({}, dict(external_cond_dim=3), r"external_cond_dim.*reference's own DiT1D constructor fails"),
    ({}, dict(x_shape=(4, 2, 32)), r"x_shape\[1\]"),
    ({}, dict(x_shape=(4, 1, 48)), r"L = x_shape\[2\] = 48"),
    ({}, dict(x_shape=(4, 1, 8)), r"L = x_shape\[2\] = 8"),
    ({}, dict(max_tokens=3), r"max_tokens \* L = 3 x 32 = 96"),
    (dict(num_heads=32), {}, "head dim"),          # 128 / 32 = 4: no multiple of 8
    (dict(hidden_size=256, num_heads=1), {}, "head dim"),  # 256 > 128
    (dict(hidden_size=96), {}, "hidden_size=96"),          # no multiple of 64
    (dict(hidden_size=4096, num_heads=32), {}, "hidden_size=4096"),
    (dict(mlp_ratio=0.3), {}, "mlp_ratio=0.3"),            # 38 columns: no multiple of 64
    ({}, dict(x_shape=(65, 1, 32)), r"x_shape\[0\] = 65"),
]


@pytest.mark.parametrize("cfg_over,ctor_over,match", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_constructor_refusals_name_the_key(cfg_over, ctor_over, match):
    import dfot_amd
    kw = dict(x_shape=dc.X_SHAPE, max_tokens=dc.MAX_TOKENS)
    kw.update(ctor_over)
    with pytest.raises(ValueError, match=match):
        dfot_amd.DiT1D(dc.backbone_cfg(4, **cfg_over), **kw)


def test_forward_is_a_torch_operator_with_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import dfot_amd  # noqa: F401  (registers the operators)
    assert hasattr(torch.ops.dfot, "dit1d_forward")
    with FakeTensorMode():
        z = torch.empty(3, 8, 4, 1, 32)
        assert torch.ops.dfot.dit1d_forward(z, torch.empty(3, 8, dtype=torch.long), 0).shape == z.shape


def test_header_and_capi_declare_the_new_symbols():
    import __graft_entry__ as ge
    ge.build()
    from dfot_amd import capi
    hdr = open(os.path.join(ROOT, "include", "dfot_hip.h")).read()
    names = ["dfot_op_attention_frame_causal"] + ["dfot_dit1d_" + n for n in (
        "create", "destroy", "num_params", "param_name", "param_shape", "load_weight", "finalize", "reserve", "workspace_bytes", "forward")]
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in capi.SIGNATURES and hasattr(capi.lib, name), name
    assert len(capi.SIGNATURES["dfot_op_attention_frame_causal"][1]) == 11
    assert C.sizeof(capi.DiT1DConfig) == 40 and "dfot_dit1d_config" in hdr


def test_bad_arguments_are_refused_before_any_device_work():
    """none of these touches the GPU: null pointers, then (with host addresses that are never dereferenced) a bad frame_len, n, d, ldo"""
    from dfot_amd import capi
    op = capi.lib.dfot_op_attention_frame_causal
    assert op(None, None, None, None, 64, 1, 2, 256, 32, 32, None) == capi.ERR_ARG
    assert b"attention_frame_causal" in capi.lib.dfot_last_error()
    buf = C.create_string_buffer(64)
    p = C.c_void_p(C.addressof(buf))
    assert op(p, p, p, None, 64, 1, 2, 256, 32, 32, None) == capi.ERR_ARG
    for ldo, n, frame_len, d, word in ((64, 256, 48, 32, b"frame_len"), (64, 256, 8, 32, b"frame_len"), (64, 256, 256, 32, b"frame_len"),
                                       (64, 192, 32, 32, b"N=192"), (64, 0, 32, 32, b"N=0"), (64, 256, 32, 36, b"head dim"),
                                       (256, 256, 32, 136, b"head dim"), (68, 256, 32, 32, b"row stride"), (32, 256, 32, 32, b"row stride")):
        assert op(p, p, p, p, ldo, 1, 2, n, frame_len, d, None) == capi.ERR_SHAPE, (ldo, n, frame_len, d)
        assert word in capi.lib.dfot_last_error(), capi.lib.dfot_last_error()
    h = C.c_void_p()
    assert capi.lib.dfot_dit1d_create(None, C.byref(h)) == capi.ERR_ARG
    cfg = capi.DiT1DConfig(hidden=128, depth=2, heads=4, mlp_hidden=512, in_channels=4, tokens_per_frame=48, max_tokens=8, timesteps=1000,
                           causal=1, eps=1e-6)
    assert capi.lib.dfot_dit1d_create(C.byref(cfg), C.byref(h)) == capi.ERR_SHAPE and b"tokens_per_frame" in capi.lib.dfot_last_error()
    cfg.tokens_per_frame, cfg.max_tokens = 32, 3
    assert capi.lib.dfot_dit1d_create(C.byref(cfg), C.byref(h)) == capi.ERR_SHAPE and b"multiple of 128" in capi.lib.dfot_last_error()
    assert not h.value
    assert capi.lib.dfot_dit1d_forward(None, None, None, None, 1, 8, None) == capi.ERR_ARG
    assert capi.lib.dfot_dit1d_reserve(None, 1) == capi.ERR_ARG
    assert capi.lib.dfot_dit1d_num_params(None) == 0 and capi.lib.dfot_dit1d_destroy(None) == capi.OK
