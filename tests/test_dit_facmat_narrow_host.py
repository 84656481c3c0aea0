"""Host checks (no GPU) of the narrow-width FacMatDiT fixture tests/golden/dit_facmat_narrow.npz (tools/make_golden_dit_facmat_narrow.py)
and of the declarations and refusals around the narrow path: the restatement dit_facmat_common.forward_host(..., embed_col_dim=E) against
every output the reference produced, the key list and order, the contrast of every host frame map, the two new ops in the header and in
capi with their refusals, and the widths that stay refused.

Bar of the restatement: both sides are fp32 torch on the same weights and differ by summation order only; the tool measured 2.8e-7 (stored
as host_rel); the assertion allows 1e-6, the bar of tests/test_dit_facmat_host.py:22."""
import os
import re

import pytest
import torch

import dit_fac_common as fc
import dit_facmat_narrow_common as nc
from dit_facmat_narrow_common import T, rel

HOST_BAR = 1e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return nc.load(nc.FIXTURE)


def _params(g, tag, patches=128, cond=False):
    """the seeded weights of a fixture model; digest, key list, order and shapes checked against what the reference registered"""
    keys = nc.keys(tag, patches, cond)
    params = nc.seeded(tag, float(g[f"gain_{tag}"]), patches, cond)
    sfx = "act" if cond else tag
    pre = "64" if patches == 64 else ""
    assert nc.digest(params) == str(g[f"digest{pre}_{sfx}"])
    assert [n for n, _ in keys] == [str(n) for n in g[f"names{pre}_{sfx}"]]
    if not cond:
        assert [" ".join(map(str, s)) for _, s in keys] == [str(s) for s in g[f"shapes{pre}_{sfx}"]]
    return params


def test_fixture_is_small_and_measured_the_restatement_below_the_bar(g):
    assert os.path.getsize(os.path.join(fc.GOLDEN, nc.FIXTURE)) < 1 << 20
    assert float(g["host_rel"]) < HOST_BAR / 2
    assert tuple(g["x"].shape) == (2, 5, 4, 16, 8) and tuple(g["x64"].shape) == (2, 4, 4, 16, 16)
    assert not any(n.endswith(("weight", "bias", "qkv_u", "proj_u")) for n in g.files if n not in ("act_mask",))  # no stored weights
    for tag, (e, cc, bias, rope) in nc.CASES.items():  # the right-factor GEMM's row count is a whole 128-row tile in no case
        assert (2 * 5 * e) % 128 and (2 * 3 * e) % 128 and e % cc == 0 and 1 <= e <= 32


@pytest.mark.parametrize("tag", list(nc.CASES))
def test_restatement_vs_reference_outputs(g, tag):
    params = _params(g, tag)
    x, k = nc.inputs(g)
    with torch.no_grad():
        for name, xx, kk in ((f"out_{tag}_t5", x, k), (f"out_{tag}_t3", x[:, :3], k[:, :3])):
            r = rel(nc.host(tag, params, xx, kk, dtype=torch.float32), T(g[name]))
            print(f"{name}: restatement rel-L2 {r:.2e}")
            assert r < HOST_BAR
        assert rel(nc.host(tag, params, x, k).float(), T(g[f"out_{tag}_t5"])) < HOST_BAR


@pytest.mark.parametrize("tag", nc.P64_TAGS)
def test_restatement_vs_reference_outputs_at_64_patches(g, tag):
    params = _params(g, tag, 64)
    x, k = nc.inputs(g, 64)
    with torch.no_grad():
        for name, xx, kk in ((f"out64_{tag}_t4", x, k), (f"out64_{tag}_t2", x[:, :2], k[:, :2])):
            r = rel(nc.host(tag, params, xx, kk, patches=64, dtype=torch.float32), T(g[name]))
            print(f"{name}: restatement rel-L2 {r:.2e}")
            assert r < HOST_BAR


def test_restatement_conditioned(g):
    tag = nc.COND_TAG
    params = _params(g, tag, cond=True)
    x, k = nc.inputs(g)
    cond, mask = T(g["act_cond"]), T(g["act_mask"])
    with torch.no_grad():
        assert rel(nc.host(tag, params, x, k, cond, dtype=torch.float32), T(g["out_act"])) < HOST_BAR
        om = nc.host(tag, params, x, k, cond, mask, dtype=torch.float32)
        assert rel(om, T(g["out_act_masked"])) < HOST_BAR
        plain = nc.host(tag, params, x, k, dtype=torch.float32)
        assert rel(om[0], plain[0]) < HOST_BAR and rel(om[1], T(g["out_act"])[1]) < HOST_BAR
        assert rel(T(g["out_act"])[0], plain[0]) > 2 * nc.FIXTURE_BAR  # the condition moves the output by more than the GPU parity bar


@pytest.mark.parametrize("tag", ["e1", "e8"])
def test_key_list_and_order_equal_the_reference(g, tag):
    """the reference's registration order at E = 1 and E = 8, with the factor shapes (P, E) / (E, P) and the per-e bias rows"""
    e = nc.CASES[tag][0]
    names, shapes = [str(n) for n in g[f"names_{tag}"]], [str(s) for s in g[f"shapes_{tag}"]]
    assert [n for n, _ in nc.keys(tag)] == names
    by = dict(zip(names, shapes))
    pre = "dit_base.temporal_blocks.1.attn"
    assert by[f"{pre}.qkv_u"] == f"128 {e}" and by[f"{pre}.proj_u"] == f"{e} 128"
    assert by[f"{pre}.qkv_bias"] == f"{e} 384" and by[f"{pre}.proj_bias"] == "128 128"
    assert names.index(f"{pre}.qkv_u") < names.index(f"{pre}.proj_u") < names.index(f"{pre}.qkv_v") < names.index(f"{pre}.proj_v")


@pytest.mark.parametrize("tag,patches", [(t, 128) for t in nc.CASES] + [(t, 64) for t in nc.P64_TAGS])
def test_host_frame_maps_are_maps_and_far_from_uniform(g, tag, patches):
    """the condition the tool chose the gain by: every host map is CONTRAST_BAR (twice the map parity bar) from the uniform map and from
    its own transpose, so the GPU comparison can tell a wrong map from a right one -- at E = 1 a score is one 32-long dot product"""
    params = _params(g, tag, patches)
    x, k = nc.inputs(g, patches)
    real = torch.softmax
    with torch.no_grad():
        maps = nc.host_frame_maps(tag, params, x, k, patches)
    tokens = x.shape[1]
    assert list(maps) == [f"dit_base.temporal_blocks.{i}.attn" for i in range(2)]
    for name, w in maps.items():
        assert tuple(w.shape) == (2, nc.CASES[tag][1], nc.RR, tokens, tokens) and w.dtype == torch.float64
        assert (w.sum(-1) - 1).abs().max().item() < 1e-12
        uniform, transposed = nc.contrast(w)
        print(f"{tag} at {patches} patches, {name}: {uniform:.3e} from uniform, {transposed:.3e} from its transpose")
        assert uniform > nc.CONTRAST_BAR and transposed > nc.CONTRAST_BAR, name
    assert torch.softmax is real  # the recorder is gone


# ---------------------------------------------------------------------------------------------------------------- declarations, refusals
OPS = ("dfot_op_facmat_contract", "dfot_op_facmat_expand")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    from dfot_amd import capi
    return capi


def test_header_and_capi_declare_the_two_ops(capi):
    hdr = open(os.path.join(ROOT, "include", "dfot_hip.h")).read()
    for name in OPS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == 8  # (in, u, out, frames, P, h, E, stream)
        assert name in capi.SIGNATURES and hasattr(capi.lib, name)
        assert len(capi.SIGNATURES[name][1]) == 8


def test_ops_refuse_null_pointers_and_widths_outside_1_to_32_without_a_device(capi):
    """every refusal comes before any device work: the pointers below are never dereferenced"""
    import ctypes as C
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 15) & ~15
    a, u, o = C.c_void_p(base), C.c_void_p(base + 1024), C.c_void_p(base + 2048)
    for name in OPS:
        fn, short = getattr(capi.lib, name), name[len("dfot_op_"):].encode()
        for args in ((None, u, o), (a, None, o), (a, u, None)):
            assert fn(*args, 2, 64, 128, 8, None) == capi.ERR_ARG
            assert short in capi.lib.dfot_last_error() and b"null" in capi.lib.dfot_last_error()
        assert fn(C.c_void_p(base + 2), u, o, 2, 64, 128, 8, None) == capi.ERR_ARG  # 16-byte accesses
        assert short in capi.lib.dfot_last_error()
        for e in (0, 33, 48, -1, 64):
            assert fn(a, u, o, 2, 64, 128, e, None) == capi.ERR_SHAPE, e
            msg = capi.lib.dfot_last_error()
            assert short in msg and b"embed_col_dim" in msg and str(e).encode() in msg
        #            frames P    h
        for shape in ((0, 64, 128), (2, 0, 128), (2, 96, 128), (2, 32, 128), (2, 64, 0), (2, 64, 96), (2, 64, 2112)):
            assert fn(a, u, o, *shape, 8, None) == capi.ERR_SHAPE, shape
            assert short in capi.lib.dfot_last_error()


@pytest.mark.parametrize("e", [0, 33, 48, 63, 96])
def test_dit3d_surfaces_the_engines_sentence_for_a_refused_width(capi, e):
    """widths between the two accepted sets: dfot_dit_create's message, naming both sets, through the exception DiT3D raises for create
    failures (the check precedes every allocation, so it needs no device)"""
    import dfot_amd
    cfg = nc.fm.backbone_cfg(1, nc.RR, True, 0.0, True, embed_col_dim=e)
    with pytest.raises(RuntimeError, match=rf"embed_col_dim {e} must be 1 to 32 \(the narrow factor kernels\) or a multiple of 64 \(the factor GEMMs\)"):
        dfot_amd.DiT3D(cfg, x_shape=(4, 16, 8), max_tokens=5)


def test_difference_model_keeps_its_width_rule(capi):
    import dfot_amd
    cfg = dict(name="difference_dit3d", variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", merge_type="interleaved", patch_size=1,
               embed_col_dim=8, embed_row_dim=128, num_heads=4, num_col_heads=1, num_row_heads=4, depth=1, mlp_ratio=4.0, spatial_mlp_ratio=4.0,
               use_bias=True, matrix_block="matrix")
    with pytest.raises(RuntimeError, match="embed_col_dim 8 must be a multiple of 64$"):
        dfot_amd.DifferenceDiT3D(cfg, x_shape=(4, 16, 8), max_tokens=2)


def test_trainer_still_refuses_a_narrow_width(capi):
    import dfot_amd
    with pytest.raises((RuntimeError, ValueError), match="embed_col_dim 8 must be 64 or 128"):
        dfot_amd.FacMatDiTTrainer(nc.cfg("e8"), x_shape=(4, 16, 8), max_tokens=5)
