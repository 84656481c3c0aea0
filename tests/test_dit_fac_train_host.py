"""Host checks (no GPU) of FacDiT training (DiT3D, variant "factorized_attention"): the two new C-ABI symbols, FacDiTTrainer's
configuration and refusals (raised before anything touches the device), the trainer's parameter order (csrc/dit_model.h through
tests/dit_model_dump.cpp), and the fixture tests/golden/dit_fac_train.npz (tools/make_golden_dit_fac_train.py: the reference's own
training loss and autograd) against the host restatement tests/dit_fac_train_common.host_loss_and_grads, which the GPU tests use for the
cases and shapes the fixture does not cover.

Bar of the restatement: both sides are fp32 torch autograd on the same weights and the same recorded noise, so they differ by summation
order only.  When the fixture was made the largest gradient rel-L2 was 1.7e-7 and the loss deviation 0 (stored as host_rel /
host_loss_rel).  The assertions allow 4x the stored values, as tests/test_dit_facmat_train_host.py does, but not less than 1e-6 for a
gradient and 1.2e-7 (one fp32 ulp) for the loss: a weight gradient is a sum over the 1280 token rows of the batch, and another thread count
reorders it, eps * sqrt(1280) = 6e-8 * 36 = 2e-6 at worst for one element and less in the norm.  Either way 1e4 times below the 5e-2 /
2e-2 bars the GPU engine is held to.

Every test here fails on the parent commit: its library exports neither symbol, its package has no FacDiTTrainer and the fixture does not
exist."""
import os
import re
import shutil
import subprocess

import pytest
import torch

import dit_fac_common as fc
import dit_fac_train_common as ft
from conftest import ROOT
from dit_fac_common import T, rel

GRAD_FLOOR, LOSS_FLOOR = 1e-6, 1.2e-7


@pytest.fixture(scope="module")
def g():
    return fc.load("dit_fac_train.npz")


# ---------------------------------------------------------------------------------------------------------------- symbols
def test_new_symbols_are_declared_exported_and_bound():
    from dfot_amd import capi
    hdr = open(os.path.join(ROOT, "include", "dfot_hip.h")).read()
    for name in ("dfot_op_attention_temporal_bwd", "dfot_facdit_train_create"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in capi.SIGNATURES and hasattr(capi.lib, name), name
    assert len(capi.SIGNATURES["dfot_op_attention_temporal_bwd"][1]) == 14
    assert capi.SIGNATURES["dfot_facdit_train_create"][1][0]._type_ is capi.DiTConfigF


def test_trainer_is_exported_and_subclasses_the_dit_trainer():
    import dfot_amd
    assert issubclass(dfot_amd.FacDiTTrainer, dfot_amd.DiT3DTrainer)
    for m in ("forward", "backward", "loss_and_grads", "training_step", "accumulate", "enable_ema", "optimizer_state_dict", "load_optimizer_state_dict"):
        assert hasattr(dfot_amd.FacDiTTrainer, m)


def _configured(cfg, x_shape=(4, 16, 8), max_tokens=5):
    """FacDiTTrainer._configure on a bare instance: what the constructor does before it touches the engine"""
    import dfot_amd
    from dfot_amd import capi
    c = capi.DiTConfigF()
    c.depth, c.num_heads, c.patch_size = int(cfg["depth"]), int(cfg["num_heads"]), int(cfg["patch_size"])
    c.in_channels, c.height, c.width = x_shape
    c.noise_dim, c.timesteps, c.rope_theta, c.eps = 256, 1000, 10000.0, 1e-6
    tr = dfot_amd.FacDiTTrainer.__new__(dfot_amd.FacDiTTrainer)
    dfot_amd.FacDiTTrainer._configure(tr, c, cfg, max_tokens)
    return c


def test_configure_maps_the_two_mlp_ratios_and_ignores_gradient_checkpointing():
    c = _configured(fc.backbone_cfg(0.0))
    assert (c.variant, c.hidden_size, c.max_tokens, c.mlp_hidden, c.temporal_mlp_hidden) == (2, 128, 5, 0, 512)
    c = _configured({**fc.backbone_cfg(4.0), "use_gradient_checkpointing": True})
    assert (c.variant, c.mlp_hidden, c.temporal_mlp_hidden) == (2, 512, 512)
    c = _configured({**fc.backbone_cfg(2.0), "mlp_ratio": 0.0})
    assert (c.mlp_hidden, c.temporal_mlp_hidden) == (256, 0)
    # @DiT/XL widths at the taichikl shape (train_dfot_facdit-xl_taichikl_16_ru.sh): 4x32x32 latents, patch 2, 16 frames
    c = _configured(dict(variant="factorized_attention", pos_emb_type="sinusoidal_factorized", patch_size=2, hidden_size=1152, depth=28,
                         num_heads=16, mlp_ratio=4.0, spatial_mlp_ratio=4.0), x_shape=(4, 32, 32), max_tokens=16)
    assert (c.variant, c.hidden_size, c.max_tokens, c.mlp_hidden, c.temporal_mlp_hidden) == (2, 1152, 16, 4608, 4608)


def test_unsupported_configurations_are_refused_by_name():
    """in the wording of dit_backbone.DiT3D._configure (the code is shared: dit_backbone.configure_fac)"""
    import dfot_amd
    with pytest.raises(ValueError, match="use_fourier_noise_embedding"):
        dfot_amd.FacDiTTrainer({**fc.backbone_cfg(0.0), "use_fourier_noise_embedding": True}, x_shape=(4, 16, 8), max_tokens=5)
    with pytest.raises(ValueError, match=r"64 patches per frame.*multiple of 128 \(the 64-patch recipes are not supported\)"):
        dfot_amd.FacDiTTrainer(fc.backbone_cfg(0.0, patch_size=2), x_shape=(4, 16, 16), max_tokens=5)  # 8x8 patches: the res-128 recipes
    with pytest.raises(ValueError, match="max_tokens 33 exceeds the temporal attention kernel's 32 frames"):
        dfot_amd.FacDiTTrainer(fc.backbone_cfg(0.0), x_shape=(4, 16, 8), max_tokens=33)
    with pytest.raises(ValueError, match="sinusoidal_factorized"):
        dfot_amd.FacDiTTrainer({**fc.backbone_cfg(0.0), "pos_emb_type": "rope_3d"}, x_shape=(4, 16, 8), max_tokens=5)
    with pytest.raises(ValueError, match="factorized_attention"):
        dfot_amd.FacDiTTrainer(dict(variant="full", pos_emb_type="rope_3d", patch_size=1, hidden_size=128, depth=1, num_heads=4),
                               x_shape=(4, 16, 8), max_tokens=5)
    # the same two shape refusals, word for word, from the inference class
    for kw, shape, tokens in ((dict(patch_size=2), (4, 16, 16), 5), ({}, (4, 16, 8), 33)):
        msgs = []
        for cls in (dfot_amd.FacDiTTrainer, dfot_amd.DiT3D):
            with pytest.raises(ValueError) as err:
                cls(fc.backbone_cfg(0.0, **kw), x_shape=shape, max_tokens=tokens)
            msgs.append(str(err.value))
        assert msgs[0] == msgs[1]
    # DiT3DTrainer's own refusal of the recipe is unchanged
    with pytest.raises(ValueError, match="no training path"):
        dfot_amd.DiT3DTrainer(fc.backbone_cfg(0.0), x_shape=(4, 16, 8), max_tokens=5)


# ---------------------------------------------------------------------------------------------------------------- parameter order
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """tests/dit_model_dump.cpp, compiled once: the inventory of csrc/dit_model.h that dfot_facdit_train_create binds its storage to"""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (CXX, c++, g++, clang++)"
    work = tmp_path_factory.mktemp("dit_fac_train")
    exe = str(work / "dit_model_dump")
    subprocess.run([cxx, "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "diffusion-forcing-transformer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "dit_model_dump.cpp"), "-o", exe], check=True)

    def run(c):
        from dfot_amd import capi
        fields = {name: getattr(c, name) for name, _ in capi.DiTConfig._fields_ + capi.DiTConfigF._fields_}
        text = subprocess.run([exe, str(work)] + [f"{k}={v}" for k, v in fields.items()], check=True, capture_output=True, text=True).stdout
        head, *lines = text.splitlines()
        geom = {k: int(v) for k, v in (item.split("=") for item in head[2:].split())}
        return geom, [(line.split()[0], int(line.split()[-2]), int(line.split()[-1])) for line in lines]
    return run


@pytest.mark.parametrize("tag", list(ft.TRAIN_CASES))
def test_trainer_parameter_order_equals_the_reference_parameters(g, dump, tag):
    """the flat buffers hold the reference's parameters in the reference's order: all spatial blocks, then all temporal blocks"""
    geom, entries = dump(_configured(fc.backbone_cfg(ft.TRAIN_CASES[tag])))
    assert geom["fac"] == 1 and geom["facmat"] == 0 and geom["P"] == 128
    names = [str(n) for n in g[f"{tag}_names"]]
    assert [n for n, _, _ in entries] == names
    assert all(off >= 0 and off % 4 == 0 for _, _, off in entries)  # every tensor is a parameter with a 16-byte aligned slot
    first_temporal = next(i for i, n in enumerate(names) if n.startswith("dit_base.temporal_blocks."))
    assert all(n.startswith("dit_base.blocks.") for n in names[first_temporal - 1:first_temporal])


# ---------------------------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("tag", list(ft.TRAIN_CASES))
def test_fixture_names_and_digest(g, tag):
    keys = fc.key_shapes(ft.TRAIN_CASES[tag])
    assert [n for n, _ in keys] == [str(n) for n in g[f"{tag}_names"]]
    assert fc.digest(ft.case_params(tag)) == str(g[f"{tag}_digest"])
    assert len(g[f"{tag}_norms"]) == len(keys) and float(g[f"{tag}_norms"].min()) > 0  # every parameter has a gradient in the reference
    stored = [k_ for k_ in g.files if k_.startswith(f"{tag}_grad/")]
    assert any(".temporal_blocks." in k_ for k_ in stored) and all(g[k_].size <= 4096 for k_ in stored)
    assert float(T(g["masks"]).sum()) == 9.0 and tuple(g["xs"].shape) == (2, 5, 4, 16, 8)
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
