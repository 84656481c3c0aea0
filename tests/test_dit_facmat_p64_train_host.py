"""Host checks (no GPU) of FacMatDiT training at 64 patches per frame (latents 4x16x16 at patch 2, the taichi res-128 facmat-s-*-bias
recipes): the two new C-ABI symbols, FacMatDiTTrainer's configuration and refusals at that shape, the refusals of the new op (raised before
anything touches the device), and the fixture tests/golden/dit_facmat_p64_train.npz (tools/make_golden_dit_facmat_p64_train.py: the
reference's own training loss and autograd) against the host restatement tests/dit_facmat_p64_train_common.host_loss_and_grads, which the
GPU tests use for the cases and shapes the fixture does not cover.

Bars of the restatement, those of tests/test_dit_fac_p64_train_host.py for the same comparison at the same geometry: both sides are fp32
torch autograd on the same weights and the same recorded noise, so they differ by summation order only.  The stored host_rel must be below
5e-6 and host_loss_rel below 1e-6 (test_dit_fac_p64_train_host.py:193); when the fixture was made they were 1.0e-6 and 0.  The re-run
allows 4x the stored values, but not less than 1e-6 for a gradient and 1.2e-7 (one fp32 ulp) for the loss (ibid. :28, :201-210).

Every test here fails on the parent commit: its library exports neither symbol, its FacMatDiTTrainer has no allow_p64 keyword and refuses
64 patches per frame without naming one, and the fixture does not exist."""
import ctypes as C
import os
import re

import pytest
import torch

import dit_facmat_common as fm
import dit_facmat_p64_train_common as ft
import dit_p64_common as pc
from conftest import ROOT
from dit_facmat_common import T, rel

GRAD_FLOOR, LOSS_FLOOR = 1e-6, 1.2e-7  # tests/test_dit_fac_p64_train_host.py:28
NEW = {"dfot_op_facmat_factor_wgrad": 8, "dfot_facmat_train_create_p64": 2}


@pytest.fixture(scope="module")
def g():
    return fm.load(ft.FIXTURE)


# ---------------------------------------------------------------------------------------------------------------- symbols
def test_new_symbols_are_declared_exported_and_bound_with_one_arity():
    from dfot_amd import capi
    hdr = open(os.path.join(ROOT, "include", "dfot_hip.h")).read()
    for name, arity in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == arity, name
        assert name in capi.SIGNATURES and hasattr(capi.lib, name), name
        assert len(capi.SIGNATURES[name][1]) == arity, name
    # the two create entries take the same arguments
    assert capi.SIGNATURES["dfot_facmat_train_create_p64"] == capi.SIGNATURES["dfot_facmat_train_create"]
    kh = open(os.path.join(ROOT, "diffusion-forcing-transformer_amd", "csrc", "kernels.h")).read()
    assert re.search(r"\bint\s+launch_facmat_factor_wgrad\s*\(", kh)


# ---------------------------------------------------------------------------------------------------------------- configuration
def _configured(cfg, max_tokens, x_shape=pc.X_SHAPE, allow_p64=True):
    """FacMatDiTTrainer._configure on a bare instance carrying the constructor's allow_p64 keyword: what the constructor does before it
    touches the engine"""
    import dfot_amd
    from dfot_amd import capi
    c = capi.DiTConfigF()
    c.depth, c.num_heads, c.patch_size = int(cfg["depth"]), int(cfg["num_heads"]), int(cfg["patch_size"])
    c.in_channels, c.height, c.width = x_shape
    c.noise_dim, c.timesteps, c.rope_theta, c.eps = 256, 1000, 10000.0, 1e-6
    tr = dfot_amd.FacMatDiTTrainer.__new__(dfot_amd.FacMatDiTTrainer)
    if allow_p64 is not None:  # None: the class default, an instance the constructor has not seen
        tr.allow_p64 = allow_p64
    dfot_amd.FacMatDiTTrainer._configure(tr, c, cfg, max_tokens)
    tr._ccfg = c
    return tr, c


@pytest.mark.parametrize("max_tokens", [4, 16])
def test_configure_accepts_64_patches_at_an_even_max_tokens(max_tokens):
    _, c = _configured(ft.cfg("b"), max_tokens)
    assert (c.variant, c.hidden_size, c.max_tokens, c.use_temporal_rope, c.use_bias) == (3, 128, max_tokens, 1, 1)
    assert (c.embed_col_dim, c.num_col_heads, c.num_row_heads, c.mlp_hidden, c.temporal_mlp_hidden) == (64, 2, 2, 512, 512)
    assert (c.height // c.patch_size) * (c.width // c.patch_size) == 64
    _, c = _configured(ft.cfg("e128"), max_tokens)
    assert (c.variant, c.embed_col_dim, c.num_col_heads, c.num_row_heads, c.use_bias, c.use_temporal_rope, c.mlp_hidden) == (3, 128, 1, 4, 0, 0, 0)
    # the recipes' own widths: @FacMatDiT/group_S with use_bias, 16 frames (train_dfot_facmat-s-128-1-bias_*.sh)
    _, c = _configured(dict(variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", patch_size=2, embed_row_dim=384, depth=6,
                            num_heads=6, num_row_heads=6, embed_col_dim=128, num_col_heads=1, mlp_ratio=4.0, spatial_mlp_ratio=4.0,
                            use_bias=True, use_temporal_rope=True), 16)
    assert (c.variant, c.hidden_size, c.max_tokens, c.embed_col_dim, c.mlp_hidden, c.temporal_mlp_hidden) == (3, 384, 16, 128, 1536, 1536)


def test_without_the_keyword_64_patches_are_refused_as_before():
    """training at 64 patches is switched on by allow_p64=True; the default keeps the refusal and its words
    (tests/test_dit_fac_p64_train_host.py:121-123, tests/test_dit_facmat_train_host.py:91), then names the keyword"""
    import dfot_amd
    want = ("variant 'factorized_matrix_attention': x_shape (4, 16, 16) with patch_size 2 gives 64 patches per frame; the per-frame kernels "
            "need a multiple of 128 (the 64-patch recipes are not supported) by default: FacMatDiTTrainer(..., allow_p64=True) trains them "
            "(even max_tokens, even T)")
    for allow in (False, None):
        with pytest.raises(ValueError) as err:
            _configured(ft.cfg("b"), 16, allow_p64=allow)
        assert str(err.value) == want
    with pytest.raises(ValueError) as err:
        dfot_amd.FacMatDiTTrainer(ft.cfg("b"), x_shape=pc.X_SHAPE, max_tokens=4)
    assert str(err.value) == want
    assert dfot_amd.FacMatDiTTrainer.allow_p64 is False


def test_configure_refuses_an_odd_max_tokens_by_name():
    import dfot_amd
    want = ("variant 'factorized_matrix_attention': x_shape (4, 16, 16) with patch_size 2 gives 64 patches per frame; the per-frame kernels "
            "need a multiple of 128 (the 64-patch recipes are not supported) in training; inference takes 64 patches with an even max_tokens "
            "only: max_tokens 5 × 64 patches per frame = 320 rows per window; the row tiles need a multiple of 128")
    with pytest.raises(ValueError) as err:
        _configured(ft.cfg("b"), 5)
    assert str(err.value) == want
    for kw in ({}, dict(allow_p64=True)):  # the constructor refuses before it creates an engine handle, with or without the keyword
        with pytest.raises(ValueError) as err:
            dfot_amd.FacMatDiTTrainer(ft.cfg("b"), x_shape=pc.X_SHAPE, max_tokens=5, **kw)
        assert str(err.value) == want


def test_other_patch_counts_and_unsupported_keys_stay_refused_with_the_keyword():
    import dfot_amd
    with pytest.raises(ValueError, match=r"gives 32 patches per frame; .* need a multiple of 128 \(or exactly 64 with an even max_tokens\)"):
        _configured(fm.backbone_cfg(2, 2, True, 4.0, True, **{**pc.OVER, "resolution": (16, 8)}), 4, x_shape=(4, 16, 8))
    for over, key in ((dict(matrix_multi_token=True), "matrix_multi_token"), (dict(flatten_matrix_rope=True), "flatten_matrix_rope"),
                      (dict(fixed_u="identity"), "fixed_u"), (dict(use_fourier_noise_embedding=True), "use_fourier_noise_embedding")):
        with pytest.raises(ValueError, match=key):  # the -mtoken / -flrope / -identityu recipes and continuous diffusion
            dfot_amd.FacMatDiTTrainer({**ft.cfg("b"), **over}, x_shape=pc.X_SHAPE, max_tokens=4, allow_p64=True)


def test_an_odd_token_count_is_refused_by_name_before_any_launch():
    """forward / loss_and_grads / training_step on a bare configured instance: the check comes first, so no engine is needed to see it"""
    tr, _ = _configured(ft.cfg("b"), 4)
    x = torch.zeros(2, 3, *pc.X_SHAPE)
    k = torch.zeros(2, 3, dtype=torch.long)
    for call in (lambda: tr.forward(x, k), lambda: tr.loss_and_grads(x, k, x), lambda: tr.training_step(x, k, x)):
        with pytest.raises(ValueError, match=r"FacMatDiTTrainer at 64 patches per frame takes an even number of tokens: 3 tokens × 64 patches = 192 rows"):
            call()
    # at a multiple of 128 patches any T passes this check (it then fails later, on the engine this bare instance lacks)
    tr, _ = _configured(fm.backbone_cfg(*fm.CASES["b"]), 5, x_shape=(4, 16, 8))
    tr._check_tokens(3)


# ---------------------------------------------------------------------------------------------------------------- op refusals
def test_factor_wgrad_refuses_bad_arguments_before_any_device_work():
    from dfot_amd import capi
    op = capi.lib.dfot_op_facmat_factor_wgrad
    buf = C.create_string_buffer(64)
    p = C.c_void_p(C.addressof(buf))  # a host address: never dereferenced
    for hole in range(3):  # a, b | out
        ptrs = [p] * 3
        ptrs[hole] = None
        assert op(*ptrs, 2, 64, 64, 128, None) == capi.ERR_ARG, hole
        assert capi.lib.dfot_last_error().startswith(b"op_facmat_factor_wgrad:")
    #            frames ra  rb   hd
    for args in ((2, 32, 64, 128), (2, 64, 32, 128), (2, 96, 64, 128), (2, 64, 192, 128), (2, 256, 64, 128), (2, 0, 64, 128), (2, 64, -64, 128),
                 (2, 64, 64, 64), (2, 64, 64, 192), (2, 64, 64, 0), (2, 64, 64, -128), (0, 64, 64, 128), (-1, 64, 64, 128)):
        assert op(p, p, p, *args, None) == capi.ERR_SHAPE, args
        assert capi.lib.dfot_last_error().startswith(b"op_facmat_factor_wgrad:"), capi.lib.dfot_last_error()


# ---------------------------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("tag", ft.TRAIN_CASES)
def test_fixture_names_and_digest(g, tag):
    keys = ft.keys(tag)
    assert [n for n, _ in keys] == [str(n) for n in g[f"{tag}_names"]]
    assert fm.digest(ft.case_params(tag)) == str(g[f"{tag}_digest"])
    assert len(g[f"{tag}_norms"]) == len(keys) and float(g[f"{tag}_norms"].min()) > 0  # every parameter has a gradient in the reference
    e = 128 if tag == "e128" else 64
    shapes = dict(keys)
    assert shapes["dit_base.temporal_blocks.0.attn.qkv_u"] == (64, e) and shapes["dit_base.temporal_blocks.1.attn.proj_u"] == (e, 64)
    stored = [k_ for k_ in g.files if k_.startswith(f"{tag}_grad/")]
    assert any(".temporal_blocks." in k_ for k_ in stored) and any("dit_base.blocks." in k_ for k_ in stored)
    assert all(g[k_].size <= 4096 for k_ in stored)
    if tag == "b":  # the 64 x 64 left factors' gradients are small enough to be stored whole
        assert f"{tag}_grad/dit_base.temporal_blocks.0.attn.qkv_u" in stored and f"{tag}_grad/dit_base.temporal_blocks.1.attn.proj_u" in stored
    assert float(T(g["masks"]).sum()) == 7.0 and tuple(g["xs"].shape) == (2, 4, 4, 16, 16)
    assert all(isinstance(g[k_], __import__("numpy").ndarray) for k_ in g.files)  # data only


def test_fixture_measured_the_restatement(g):
    print(f"restatement vs the reference when the fixture was made: gradients {float(g['host_rel']):.2e}, loss {float(g['host_loss_rel']):.2e}")
    assert float(g["host_rel"]) < 5e-6 and float(g["host_loss_rel"]) < 1e-6  # tests/test_dit_fac_p64_train_host.py:193


@pytest.mark.parametrize("tag", ft.TRAIN_CASES)
def test_restatement_reproduces_the_reference_loss_and_gradients(g, tag):
    loss, grads = ft.host_loss_and_grads(tag, T(g["xs"]), T(g["k"]), T(g[f"{tag}_noise"]), T(g["masks"]))
    ref_loss = float(g[f"{tag}_loss"])
    dl = abs(float(loss) - ref_loss) / abs(ref_loss)
    bar = max(4 * float(g["host_rel"]), GRAD_FLOOR)
    worst = 0.0
    for n, ref_norm in zip((str(n) for n in g[f"{tag}_names"]), g[f"{tag}_norms"]):
        assert abs(float(grads[n].norm()) - ref_norm) <= bar * ref_norm, n
    for key in g.files:
        if key.startswith(f"{tag}_grad/"):
            worst = max(worst, rel(grads[key.split("/", 1)[1]], T(g[key])))
    print(f"{tag}: restatement loss deviation {dl:.2e}, worst stored-gradient rel-L2 {worst:.2e}")
    assert dl <= max(4 * float(g["host_loss_rel"]), LOSS_FLOOR)
    assert worst <= bar
