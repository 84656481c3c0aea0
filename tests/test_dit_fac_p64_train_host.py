"""Host checks (no GPU) of FacDiT training at 64 patches per frame (latents 4x16x16 at patch 2, the taichi res-128 recipes): the three
new C-ABI symbols, FacDiTTrainer's configuration and refusals at that shape, the refusals of the two new ops (raised before anything touches
the device), and the fixture tests/golden/dit_fac_p64_train.npz (tools/make_golden_dit_fac_p64_train.py: the reference's own training loss
and autograd) against the host restatement tests/dit_fac_p64_train_common.host_loss_and_grads, which the GPU tests use for the cases and
shapes the fixture does not cover.

Bar of the restatement, the one of tests/test_dit_fac_train_host.py for the same comparison: both sides are fp32 torch autograd on the same
weights and the same recorded noise, so they differ by summation order only.  When the fixture was made the largest gradient rel-L2 was
2.2e-7 and the loss deviation 1.0e-7 (stored as host_rel / host_loss_rel).  The assertions allow 4x the stored values, but not less than
1e-6 for a gradient and 1.2e-7 (one fp32 ulp) for the loss: a weight gradient is a sum over the 512 token rows of the batch, and another
thread count reorders it.

Every test here fails on the parent commit: its library exports none of the three symbols, its FacDiTTrainer refuses 64 patches per
frame at every max_tokens (it has no allow_p64 keyword) and the fixture does not exist."""
import ctypes as C
import os
import re

import pytest
import torch

import dit_fac_common as fc
import dit_fac_p64_train_common as ft
import dit_p64_common as pc
from conftest import ROOT
from dit_fac_common import T, rel

GRAD_FLOOR, LOSS_FLOOR = 1e-6, 1.2e-7  # tests/test_dit_fac_train_host.py
NEW = {"dfot_op_attention_temporal_bwd_p64": 13, "dfot_op_attention_seq64_bwd_packed": 11, "dfot_facdit_train_set_seq64_packed": 2}


@pytest.fixture(scope="module")
def g():
    return fc.load(ft.FIXTURE)


# ---------------------------------------------------------------------------------------------------------------- symbols
def test_new_symbols_are_declared_exported_and_bound_with_one_arity():
    from dfot_amd import capi
    hdr = open(os.path.join(ROOT, "include", "dfot_hip.h")).read()
    for name, arity in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == arity, name
        assert name in capi.SIGNATURES and hasattr(capi.lib, name), name
        assert len(capi.SIGNATURES[name][1]) == arity, name
    kh = open(os.path.join(ROOT, "diffusion-forcing-transformer_amd", "csrc", "kernels.h")).read()
    m = re.search(r"\bint\s+launch_attention_seq64_bwd_packed\s*\(([^)]*)\)", kh)
    assert m and len(m.group(1).split(",")) == 11
    # the three-buffer form keeps its 12 arguments
    assert len(capi.SIGNATURES["dfot_op_attention_seq64_bwd"][1]) == 12 and len(capi.SIGNATURES["dfot_op_attention_temporal_bwd"][1]) == 14


# ---------------------------------------------------------------------------------------------------------------- configuration
def _configured(cfg, max_tokens, x_shape=pc.X_SHAPE, allow_p64=True):
    """FacDiTTrainer._configure on a bare instance carrying the constructor's allow_p64 keyword: what the constructor does before it
    touches the engine"""
    import dfot_amd
    from dfot_amd import capi
    c = capi.DiTConfigF()
    c.depth, c.num_heads, c.patch_size = int(cfg["depth"]), int(cfg["num_heads"]), int(cfg["patch_size"])
    c.in_channels, c.height, c.width = x_shape
    c.noise_dim, c.timesteps, c.rope_theta, c.eps = 256, 1000, 10000.0, 1e-6
    tr = dfot_amd.FacDiTTrainer.__new__(dfot_amd.FacDiTTrainer)
    if allow_p64 is not None:  # None: the class default, an instance the constructor has not seen
        tr.allow_p64 = allow_p64
    dfot_amd.FacDiTTrainer._configure(tr, c, cfg, max_tokens)
    tr._ccfg = c
    return tr, c


@pytest.mark.parametrize("max_tokens", [4, 16])
def test_configure_accepts_64_patches_at_an_even_max_tokens(max_tokens):
    _, c = _configured(pc.fac_cfg(0.0), max_tokens)
    assert (c.variant, c.hidden_size, c.max_tokens, c.mlp_hidden, c.temporal_mlp_hidden) == (2, 128, max_tokens, 0, 512)
    assert (c.height // c.patch_size) * (c.width // c.patch_size) == 64
    _, c = _configured(pc.fac_cfg(4.0), max_tokens)
    assert (c.variant, c.mlp_hidden, c.temporal_mlp_hidden) == (2, 512, 512)
    # the recipe's own widths: @FacDiT/S, 16 frames (train_dfot_facdit-s[-mlp]_taichikl_16_res128_ru.sh)
    _, c = _configured(dict(variant="factorized_attention", pos_emb_type="sinusoidal_factorized", patch_size=2, hidden_size=384, depth=6,
                            num_heads=6, mlp_ratio=4.0, spatial_mlp_ratio=4.0), 16)
    assert (c.variant, c.hidden_size, c.max_tokens, c.mlp_hidden, c.temporal_mlp_hidden) == (2, 384, 16, 1536, 1536)


def test_without_the_keyword_64_patches_are_refused_as_before():
    """training at 64 patches is switched on by allow_p64=True; the default keeps the refusal and its words (tests/test_dit_p64_host.py)"""
    import dfot_amd
    want = ("variant 'factorized_attention': x_shape (4, 16, 16) with patch_size 2 gives 64 patches per frame; the per-frame attention kernels "
            "need a multiple of 128 (the 64-patch recipes are not supported) by default: FacDiTTrainer(..., allow_p64=True) trains them (even "
            "max_tokens, even T)")  # the words it had, then the keyword
    for allow in (False, None):
        with pytest.raises(ValueError) as err:
            _configured(pc.fac_cfg(0.0), 16, allow_p64=allow)
        assert str(err.value) == want
    with pytest.raises(ValueError) as err:
        dfot_amd.FacDiTTrainer(pc.fac_cfg(0.0), x_shape=pc.X_SHAPE, max_tokens=4)
    assert str(err.value) == want
    assert dfot_amd.FacDiTTrainer.allow_p64 is False


def test_configure_refuses_an_odd_max_tokens_in_todays_words():
    import dfot_amd
    want = ("variant 'factorized_attention': x_shape (4, 16, 16) with patch_size 2 gives 64 patches per frame; the per-frame attention kernels "
            "need a multiple of 128 (the 64-patch recipes are not supported) in training; inference takes 64 patches with an even max_tokens "
            "only: max_tokens 5 × 64 patches per frame = 320 rows per window; the row tiles need a multiple of 128")
    with pytest.raises(ValueError) as err:
        _configured(pc.fac_cfg(0.0), 5)
    assert str(err.value) == want
    for kw in ({}, dict(allow_p64=True)):  # the constructor refuses before it creates an engine handle, with or without the keyword
        with pytest.raises(ValueError) as err:
            dfot_amd.FacDiTTrainer(pc.fac_cfg(0.0), x_shape=pc.X_SHAPE, max_tokens=5, **kw)
        assert str(err.value) == want
    with pytest.raises(ValueError) as err:  # ... in the inference class's words
        dfot_amd.DiT3D(pc.fac_cfg(0.0), x_shape=pc.X_SHAPE, max_tokens=5)
    assert str(err.value) == want


def test_other_patch_counts_and_the_matrix_trainer_stay_refused():
    import dfot_amd
    with pytest.raises(ValueError, match=r"gives 32 patches per frame; .* need a multiple of 128 \(or exactly 64 with an even max_tokens\)"):
        _configured(pc.fac_cfg(0.0, resolution=(16, 8)), 4, x_shape=(4, 16, 8))
    with pytest.raises(ValueError, match=r"64 patches per frame; the per-frame kernels need a multiple of 128 \(the 64-patch recipes are not "
                                         r"supported\)"):
        dfot_amd.FacMatDiTTrainer(pc.mat_cfg("b"), x_shape=pc.X_SHAPE, max_tokens=4)


def test_an_odd_token_count_is_refused_by_name_before_any_launch():
    """forward / loss_and_grads / training_step on a bare configured instance: the check comes first, so no engine is needed to see it"""
    tr, _ = _configured(pc.fac_cfg(0.0), 4)
    x = torch.zeros(2, 3, *pc.X_SHAPE)
    k = torch.zeros(2, 3, dtype=torch.long)
    for call in (lambda: tr.forward(x, k), lambda: tr.loss_and_grads(x, k, x), lambda: tr.training_step(x, k, x)):
        with pytest.raises(ValueError, match=r"64 patches per frame takes an even number of tokens: 3 tokens × 64 patches = 192 rows"):
            call()
    # at a multiple of 128 patches any T passes this check (it then fails later, on the engine this bare instance lacks)
    tr, _ = _configured(fc.backbone_cfg(0.0), 5, x_shape=(4, 16, 8))
    tr._check_tokens(3)


# ---------------------------------------------------------------------------------------------------------------- op refusals
def test_packed_backward_refuses_bad_arguments_before_any_device_work():
    from dfot_amd import capi
    op = capi.lib.dfot_op_attention_seq64_bwd_packed
    buf = C.create_string_buffer(64)
    p = C.c_void_p(C.addressof(buf))  # a host address: never dereferenced
    for hole in range(5):  # q, k, v, d_o | dqkv
        ptrs = [p] * 5
        ptrs[hole] = None
        assert op(*ptrs[:4], 64, ptrs[4], 192, 1, 2, 32, None) == capi.ERR_ARG, hole
        assert capi.lib.dfot_last_error().startswith(b"attention_seq64_bwd_packed:")
    #            ldo  ldg  nseq   heads  d
    for args in ((72, 216, 1, 2, 36), (64, 192, 1, 2, 0), (272, 816, 1, 2, 136), (64, 192, 0, 2, 32), (64, 192, 1, 0, 32), (64, 192, -1, 2, 32),
                 (64, 192, 65536, 32768, 32), (56, 192, 1, 2, 32), (68, 192, 1, 2, 32), (64, 184, 1, 2, 32), (64, 196, 1, 2, 32),
                 (64, 0, 1, 2, 32), (64, 128, 1, 2, 32)):
        assert op(p, p, p, p, args[0], p, *args[1:], None) == capi.ERR_SHAPE, args
        assert capi.lib.dfot_last_error().startswith(b"attention_seq64_bwd_packed:"), capi.lib.dfot_last_error()


def test_temporal_backward_p64_refuses_bad_arguments_before_any_device_work():
    from dfot_amd import capi
    op = capi.lib.dfot_op_attention_temporal_bwd_p64
    buf = C.create_string_buffer(64)
    p = C.c_void_p(C.addressof(buf))
    for hole in range(7):  # q, k, v, d_o | dq, dk, dv
        ptrs = [p] * 7
        ptrs[hole] = None
        assert op(*ptrs[:4], 128, *ptrs[4:], 2, 4, 2, 64, None) == capi.ERR_ARG, hole
    #            ldo  batch  T  heads d
    for args in ((128, 2, 0, 2, 64), (128, 2, 33, 2, 64), (72, 2, 4, 2, 36), (272, 2, 4, 2, 136), (120, 2, 4, 2, 64), (132, 2, 4, 2, 64),
                 (128, 0, 4, 2, 64), (128, 2, 4, 0, 64), (128, 65536, 4, 2, 64), (128, 2, -1, 2, 64)):
        assert op(p, p, p, p, args[0], p, p, p, *args[1:], None) == capi.ERR_SHAPE, args
        assert capi.lib.dfot_last_error().startswith(b"temporal attention backward:")
    # the documented op keeps refusing 64 patches
    assert capi.lib.dfot_op_attention_temporal_bwd(p, p, p, p, 128, p, p, p, 2, 4, 64, 2, 64, None) == capi.ERR_SHAPE
    assert b"64 patches per frame must be a multiple of 128" in capi.lib.dfot_last_error()


# ---------------------------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("tag", list(ft.TRAIN_CASES))
def test_fixture_names_and_digest(g, tag):
    keys = pc.fac_keys(ft.TRAIN_CASES[tag])
    assert [n for n, _ in keys] == [str(n) for n in g[f"{tag}_names"]]
    assert fc.digest(ft.case_params(tag)) == str(g[f"{tag}_digest"])
    assert len(g[f"{tag}_norms"]) == len(keys) and float(g[f"{tag}_norms"].min()) > 0  # every parameter has a gradient in the reference
    stored = [k_ for k_ in g.files if k_.startswith(f"{tag}_grad/")]
    assert any(".temporal_blocks." in k_ for k_ in stored) and any("dit_base.blocks." in k_ for k_ in stored)
    assert all(g[k_].size <= 4096 for k_ in stored)
    assert float(T(g["masks"]).sum()) == 7.0 and tuple(g["xs"].shape) == (2, 4, 4, 16, 16)
    assert all(isinstance(g[k_], __import__("numpy").ndarray) for k_ in g.files)  # data only


def test_fixture_measured_the_restatement(g):
    print(f"restatement vs the reference when the fixture was made: gradients {float(g['host_rel']):.2e}, loss {float(g['host_loss_rel']):.2e}")
    assert float(g["host_rel"]) < 5e-6 and float(g["host_loss_rel"]) < 1e-6


@pytest.mark.parametrize("tag", list(ft.TRAIN_CASES))
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
