"""Host checks (no GPU) of UViT3D training: the four per-frame FiLM entry points (declared, exported, bound), UViT3DTrainer's refusals (raised by
name before anything touches the device) and the fixture tests/golden/uvit3d_train.npz (tools/make_golden_uvit3d_train.py: the reference's own
UViT3D under its continuous-diffusion training loss and autograd) against the host restatement
tests/uvit3d_train_common.host_loss_and_grads, which the GPU tests use for what the fixture does not cover.

Bar of the restatement: both sides are fp32 torch autograd on the same weights and the same seeded noise, so they differ by summation order
only.  When the fixture was made the largest gradient rel-L2 was 7.5e-7 and the loss deviation 0 (stored as host_rel / host_loss_rel).  The
assertions allow 2x the stored values, but not less than 1e-6 for a gradient and 1.2e-7 (one fp32 ulp) for the loss, the floors of
tests/test_dit_fac_train_host.py for the same purpose: a stored deviation of exactly 0 cannot be held across thread counts, since a weight
gradient is a sum over the batch's rows (65536 pixels at level 0) that another thread count reorders.  Either way 1e4 times below the bars
the GPU engine is held to.

Every test here fails on the parent commit: its library exports none of the symbols, its package has no UViT3DTrainer and the fixture does not
exist."""
import os
import re

import numpy as np
import pytest
import torch

import uvit3d_common as uc
import uvit3d_train_common as ut
from conftest import ROOT
from uvit3d_common import T, rel

GRAD_FLOOR, LOSS_FLOOR = 1e-6, 1.2e-7
OPS = {"dfot_op_gn_silu_fwd_frame": 12, "dfot_op_gn_silu_bwd_frame": 18, "dfot_op_rms_film_fwd_frame": 10, "dfot_op_rms_film_bwd_frame": 16}


@pytest.fixture(scope="module")
def g():
    return uc.load("uvit3d_train.npz")


def test_frame_ops_are_declared_exported_and_bound():
    from dfot_amd import capi
    hdr = open(os.path.join(ROOT, "include", "dfot_hip.h")).read()
    for name, nargs in OPS.items():
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in capi.SIGNATURES and hasattr(capi.lib, name), name
        assert len(capi.SIGNATURES[name][1]) == nargs, name


def test_trainer_is_exported_with_the_pose_trainers_methods():
    import dfot_amd
    from dfot_amd import uvit_train
    assert dfot_amd.UViT3DTrainer is uvit_train.UViT3DTrainer
    for m in ("forward", "backward", "loss_and_grads", "accumulate", "optimizer_step", "enable_ema", "ema_state_dict", "load_ema_state_dict",
              "optimizer_state_dict", "load_optimizer_state_dict", "grad_norm", "state_dict"):
        assert getattr(dfot_amd.UViT3DTrainer, m) is getattr(uvit_train.UViT3DPoseTrainer, m), m  # one implementation serves both trainers
    assert isinstance(uvit_train.ROW_FILM, bool)


def _cfg(**over):
    return {**uc.TINY, "resolution": uc.X_SHAPE[-1], "max_tokens": uc.MAX_TOKENS, "in_channels": uc.X_SHAPE[0], **over}


@pytest.mark.parametrize("over,match", [
    (dict(channels=[128, 256, 512, 1024], num_heads=4), r"head dim 1024/4 = 256 at level 3"),          # the stock u_vit3d.yaml's 4 heads
    (dict(use_fourier_noise_embedding=False), r"only the Fourier noise-level embedding"),
    (dict(pos_emb_type="learned_1d"), r"pos_emb_type 'learned_1d' is not built"),
    (dict(block_types=["ResBlock", "ResBlock", "AxialTransformerBlock", "TransformerBlock"]), r"'AxialTransformerBlock' is not built"),
    (dict(cond_dim=1025), r"cond_dim 1025 is outside the engine's limit"),
    (dict(emb_channels=2048), r"emb_channels 2048 is outside the engine's limit"),
    (dict(max_tokens=3), r"3 x 4 x 4 tokens at the coarsest level must be a multiple of 128"),
    (dict(patch_size=4), r"patch size 2"),
])
def test_unsupported_configurations_are_refused_by_name(over, match):
    """without a device: the constructor refuses before it creates a tensor (the parameters are never looked at)"""
    import dfot_amd
    with pytest.raises(ValueError, match=match):
        dfot_amd.UViT3DTrainer({}, _cfg(**over))


def test_parameter_inventory_is_checked_against_cond_dim_and_dropout():
    import dfot_amd
    keys = dict(uc.key_shapes(*uc.CASES["b"]))  # dropout 0: no ".embedding" infix
    with pytest.raises(ValueError, match=r"external_cond_embedding\.embedding\.linear_1\.weight"):
        dfot_amd.UViT3DTrainer(keys, _cfg(cond_dim=uc.COND_DIM, external_cond_dropout=0.1))
    with pytest.raises(ValueError, match=r"cond_dim 0"):
        dfot_amd.UViT3DTrainer(keys, _cfg())


# ---------------------------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("tag", ut.TRAIN_CASES)
def test_fixture_names_and_digests(g, tag):
    keys = uc.key_shapes(*uc.CASES[tag])
    assert [n for n, _ in keys if n not in (uc.FREQS, uc.PHASES)] == [str(n) for n in g[f"{tag}_names"]]
    assert uc.digest(uc.case_params(tag)) == str(g[f"{tag}_digest"])
    assert len(g[f"{tag}_norms"]) == len(keys) - 2 and float(g[f"{tag}_norms"].min()) > 0  # every parameter has a gradient in the reference
    stored = [k_ for k_ in g.files if k_.startswith(f"{tag}_grad/")]
    assert stored and all(g[k_].size <= 4096 for k_ in stored)
    assert all(isinstance(g[k_], np.ndarray) for k_ in g.files)  # data only


def test_fixture_inputs_are_the_seeded_ones(g):
    xs, t, masks, cond = ut.train_inputs()
    assert uc.tensor_digest(xs, t, cond) == str(g["inputs_digest"])
    assert torch.equal(T(g["masks"]), masks) and float(masks.sum()) == uc.BATCH * uc.MAX_TOKENS - 1
    noise = ut.train_noise()
    assert int(g["noise_seed"]) == ut.NOISE_SEED and tuple(g["noise_shape"]) == tuple(noise.shape)
    assert uc.tensor_digest(noise) == str(g["noise_digest"])
    assert torch.equal(T(g["c_drop"]), ut.DROP)


def test_fixture_measured_the_restatement(g):
    print(f"restatement vs the reference when the fixture was made: gradients {float(g['host_rel']):.2e}, loss {float(g['host_loss_rel']):.2e}")
    assert float(g["host_rel"]) < 5e-6 and float(g["host_loss_rel"]) < 1e-6


@pytest.mark.parametrize("tag", ut.TRAIN_CASES)
def test_restatement_reproduces_the_reference_loss_and_gradients(g, tag):
    loss, grads = ut.host_loss_and_grads(tag)
    ref_loss = float(g[f"{tag}_loss"])
    dl = abs(float(loss) - ref_loss) / abs(ref_loss)
    bar = max(2 * float(g["host_rel"]), GRAD_FLOOR)
    for n, ref_norm in zip((str(n) for n in g[f"{tag}_names"]), g[f"{tag}_norms"]):
        assert abs(float(grads[n].norm()) - ref_norm) <= bar * ref_norm, n
    worst = 0.0
    for key in g.files:
        if key.startswith(f"{tag}_grad/"):
            worst = max(worst, rel(grads[key.split("/", 1)[1]], T(g[key])))
    print(f"{tag}: restatement loss deviation {dl:.2e}, worst stored-gradient rel-L2 {worst:.2e}")
    assert dl <= max(2 * float(g["host_loss_rel"]), LOSS_FLOOR)
    assert worst <= bar
