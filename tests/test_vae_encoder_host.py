"""CPU: the VideoVAE encoder module's state-dict inventory against the fixture captured from the reference's own VideoVAE
(tests/golden/vae_encode.npz, tools/make_golden_vae_encode.py), and the options / shapes it refuses before any launch."""
import ast
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN


def _encoder(**kw):
    import dfot_amd
    return dfot_amd.VideoVAEEncoder(hidden_size=128, z_channels=16, embed_dim=16, resolution=128, temporal_length=17, **kw)


def test_encoder_registers_the_reference_keys():
    """names, shapes and order == the reference VideoVAE's encoder.* + quant_conv.* state dict (108 tensors, 94.7 M values)"""
    g = np.load(os.path.join(GOLDEN, "vae_encode.npz"))
    ref = [(str(n), ast.literal_eval(str(s))) for n, s in zip(g["names"], g["shapes"])]
    enc = _encoder()   # constructing it does not touch the GPU
    own = [(n, tuple(t.shape)) for n, t in enc.named_parameters()]
    assert own == ref
    assert len(own) == 108 and sum(t.numel() for t in enc.parameters()) == 94_732_224
    # the two name forms: nn.Conv2d modules (4-D .weight) and PaddedConv3D (5-D .conv.weight)
    shapes = dict(own)
    assert shapes["encoder.conv_in.weight"] == (128, 3, 3, 3)
    assert shapes["encoder.down.1.block.0.nin_shortcut.weight"] == (256, 128, 1, 1)
    assert shapes["encoder.down.0.downsample.conv.weight"] == (128, 128, 3, 3)
    assert shapes["encoder.down.1.downsample.conv.conv.weight"] == (256, 256, 3, 3, 3)
    assert shapes["encoder.down.2.block.0.nin_shortcut.conv.weight"] == (512, 256, 1, 1, 1)
    assert shapes["quant_conv.conv.weight"] == (32, 32, 1, 1, 1)


def test_encoder_loads_a_reference_checkpoint_and_returns_the_other_keys():
    enc = _encoder()
    sd = {"vae." + n: torch.full(tuple(t.shape), 0.5) for n, t in enc.named_parameters()}
    sd["vae.decoder.conv_in.conv.weight"] = torch.zeros(1)
    sd["vae.post_quant_conv.conv.bias"] = torch.zeros(16)
    sd["vae.loss.logvar"] = torch.zeros(())
    ignored = enc.load_reference_state_dict(sd)
    assert sorted(ignored) == ["vae.decoder.conv_in.conv.weight", "vae.loss.logvar", "vae.post_quant_conv.conv.bias"]
    assert all(bool((t == 0.5).all()) for t in enc.parameters())
    with pytest.raises(ValueError):   # strict on its own keys
        enc.load_reference_state_dict({"encoder.conv_in.weight": torch.zeros(128, 3, 3, 3)})
    with pytest.raises(ValueError):
        enc.load_reference_state_dict(dict(sd, **{"vae.encoder.conv_in.weight": torch.zeros(128, 3, 3)}))


@pytest.mark.parametrize("kw", [dict(is_causal=False), dict(attn_resolutions=(16,)), dict(encoder_attention="AttnBlock"),
                                dict(encoder_conv_in="PaddedConv3D"), dict(encoder_mid_resnet="ResnetBlock2D"),
                                dict(encoder_resnet_blocks=("ResnetBlock2D", "ResnetBlock2D", "ResnetBlock3D", "ResnetBlock1D")),
                                dict(encoder_spatial_downsample=("Downsample", "SpatialDownsample2x", "Spatial2xTime2x3DDownsample", "")),
                                dict(encoder_spatial_downsample=("Downsample", "Downsample", "Spatial2xTime2x3DDownsample", "Downsample")),
                                dict(encoder_temporal_downsample=("", "", "TimeDownsampleRes2x", ""))])
def test_unsupported_options_raise(kw):
    with pytest.raises(NotImplementedError):
        _encoder(**kw)


def test_bad_inputs_raise_before_any_launch():
    import dfot_amd
    enc = _encoder()
    enc.check_input_shape(2, 17, 128, 128)
    enc.check_input_shape(1, 1, 128, 64)
    for t in (2, 4, 16, 21):                      # T = 4k + 1 <= temporal_length only
        with pytest.raises(ValueError, match="frames"):
            enc.check_input_shape(1, t, 128, 128)
    with pytest.raises(ValueError, match="spatial factor"):
        enc.check_input_shape(1, 17, 100, 128)
    with pytest.raises(ValueError, match=r"\(1, 3, 1, 64, 64\).*M = 64"):   # the 8x8 frames of the mid attention: half a tile
        enc.check_input_shape(1, 1, 64, 64)
    with pytest.raises(ValueError, match="M = "):
        enc.check_input_shape(1, 5, 136, 128)
    with pytest.raises(ValueError, match="GPU"):   # host tensors
        enc.encode(torch.zeros(1, 3, 1, 128, 128))
    with pytest.raises(ValueError, match="GPU"):
        dfot_amd.encode_videos(enc, torch.zeros(1, 1, 3, 128, 128))
    with pytest.raises(ValueError):
        dfot_amd.encode_videos(enc, torch.zeros(1, 1, 3, 128, 128), shape="b c t h w")
