"""CPU: the torch restatement of the ImageVAE (tests/image_vae_common.py) against the fixture captured from the reference's own Encoder /
Decoder source (tests/golden/image_vae.npz, tools/make_golden_image_vae.py), the product modules' state-dict inventory and constructor
refusals, and the C ABI declarations of the three new ops.

Bar of the restatement: the one tests/test_oracle_vae.py:27 holds the VideoVAE restatement to (rtol 1e-3, atol 2e-4).  Measured here on
the CPU: max |restatement - fixture| = 0 for A and B, decoded frames and moments (the restatement issues the same torch calls)."""
import os
import re

import pytest
import torch

import image_vae_common as ivc
from conftest import ROOT

G = ivc.load()


@pytest.mark.parametrize("case", ["a", "b"])
def test_restatement_vs_reference_fixture(case):
    p, cfg = ivc.seeded_params(G, case), ivc.ddconfig(case)
    with torch.no_grad():
        frames = ivc.decode(p, cfg, ivc.T(G[f"z_{case}"]))
        moments = ivc.encode(p, cfg, 2.0 * ivc.T(G[f"y_{case}"]) - 1.0)
    for got, key in ((frames, "frames"), (moments, "moments")):
        ref = ivc.T(G[f"{key}_{case}"])
        print(f"case {case} {key}: max abs diff {(got - ref).abs().max().item():.3e}, rel-L2 {ivc.rel(got, ref):.3e}")
        assert got.shape == ref.shape
        torch.testing.assert_close(got, ref, rtol=1e-3, atol=2e-4)
    c = ivc.CASES[case]
    assert frames.shape == (c["frames"], 3, c["resolution"], c["resolution"])


@pytest.mark.parametrize("case", ["a", "b"])
def test_product_modules_register_the_reference_keys(case):
    import dfot_amd
    shapes = ivc.key_shapes(G, case)
    dec = dfot_amd.ImageVAEDecoder(**ivc.ddconfig(case))           # constructing a module does not touch the GPU
    enc = dfot_amd.ImageVAEEncoder(**ivc.ddconfig(case))
    own_d = {n: tuple(t.shape) for n, t in dec.named_parameters()}
    own_e = {n: tuple(t.shape) for n, t in enc.named_parameters()}
    assert own_d == {n: s for n, s in shapes.items() if n.startswith(("decoder.", "post_quant_conv."))}
    assert own_e == {n: s for n, s in shapes.items() if n.startswith(("encoder.", "quant_conv."))}
    assert not set(own_d) & set(own_e) and set(own_d) | set(own_e) == set(shapes)
    if case == "b":   # the level without a channel change has no nin_shortcut
        assert not any("up.1.block.0.nin_shortcut" in n for n in own_d) and any("up.0.block.0.nin_shortcut" in n for n in own_d)


@pytest.mark.parametrize("cls", ["ImageVAEDecoder", "ImageVAEEncoder"])
def test_constructor_refusals(cls):
    import dfot_amd
    make = getattr(dfot_amd, cls)
    base = ivc.ddconfig("a")
    make(**base, dropout=0.0, in_channels=3, double_z=True)         # the reference's remaining ddconfig keys are accepted
    with pytest.raises(NotImplementedError, match="attn_resolutions"):
        make(**{**base, "attn_resolutions": (16,)})
    with pytest.raises(NotImplementedError, match="use_linear_attn"):
        make(**base, use_linear_attn=True)
    with pytest.raises(NotImplementedError, match="attn_type"):
        make(**base, attn_type="none")
    with pytest.raises(NotImplementedError, match="resamp_with_conv"):
        make(**base, resamp_with_conv=False)
    with pytest.raises(ValueError, match="width 384"):
        make(**{**base, "ch_mult": (1, 3)})
    with pytest.raises(ValueError, match="width 64"):
        make(**{**base, "ch": 64})
    if cls == "ImageVAEDecoder":
        with pytest.raises(NotImplementedError, match="tanh_out"):
            make(**base, tanh_out=True)
        with pytest.raises(NotImplementedError, match="give_pre_end"):
            make(**base, give_pre_end=True)


def test_call_time_refusals_before_any_launch():
    import dfot_amd
    dec = dfot_amd.ImageVAEDecoder(**ivc.ddconfig("a"))
    enc = dfot_amd.ImageVAEEncoder(**ivc.ddconfig("a"))
    with pytest.raises(ValueError, match="GPU only"):
        dec.decode(torch.zeros(4, 4, 8, 8))
    with pytest.raises(ValueError, match="GPU only"):
        enc.encode(torch.zeros(4, 3, 16, 16))
    with pytest.raises(ValueError, match=r"\(F, 4, h, w\)"):
        dec.decode(torch.zeros(4, 5, 8, 8))
    # 3 frames of 8x8 are 192 GEMM rows: the message names the frame count that works
    with pytest.raises(ValueError, match="4 frames would work"):
        dec._check_rows(3, 8, 8, "latents")
    with pytest.raises(ValueError, match="supported"):
        dec._check_rows(2, 4, 4, "latents")
    dec._check_rows(1, 16, 16, "latents")


def test_header_declares_and_capi_binds_the_new_ops():
    from dfot_amd import capi
    header = open(os.path.join(ROOT, "include", "dfot_hip.h")).read()
    for name in ("dfot_op_ivae_attention", "dfot_op_conv3x3_s2_f32", "dfot_op_upconv3x3_f32"):
        assert re.search(rf"\bint {name}\(", header), name
        assert name in capi.SIGNATURES and hasattr(capi.lib, name)
    assert len(capi.SIGNATURES["dfot_op_ivae_attention"][1]) == 8
    assert len(capi.SIGNATURES["dfot_op_conv3x3_s2_f32"][1]) == len(capi.SIGNATURES["dfot_op_upconv3x3_f32"][1]) == 10
