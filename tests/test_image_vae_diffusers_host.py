"""CPU: ingestion of diffusers-layout ``AutoencoderKL`` checkpoints by dfot_amd.image_vae (diffusers_to_reference_keys,
ddconfig_from_diffusers, load_diffusers_state_dict, load_diffusers_checkpoint), the mid attention's row rule, and the restatement
against the 1024-position fixture.

The key table below is written out literally from the format's public layout (the library is not installed where this suite runs, so
it cannot be executed against it); tests/image_vae_1024_common.to_diffusers_name is a second, independent statement of the same map."""
import json
import os

import pytest
import torch

import image_vae_1024_common as c1k

LEVELS = 2
CFG = c1k.CFG_C

# diffusers name -> reference (ldm) name, for ch_mult (1, 2) with one res block; every entry stands for its .weight and .bias
TABLE = {
    "encoder.conv_in": "encoder.conv_in",
    "encoder.down_blocks.0.resnets.0.norm1": "encoder.down.0.block.0.norm1",
    "encoder.down_blocks.0.resnets.0.conv1": "encoder.down.0.block.0.conv1",
    "encoder.down_blocks.0.resnets.0.norm2": "encoder.down.0.block.0.norm2",
    "encoder.down_blocks.0.resnets.0.conv2": "encoder.down.0.block.0.conv2",
    "encoder.down_blocks.0.downsamplers.0.conv": "encoder.down.0.downsample.conv",
    "encoder.down_blocks.1.resnets.0.norm1": "encoder.down.1.block.0.norm1",
    "encoder.down_blocks.1.resnets.0.conv1": "encoder.down.1.block.0.conv1",
    "encoder.down_blocks.1.resnets.0.norm2": "encoder.down.1.block.0.norm2",
    "encoder.down_blocks.1.resnets.0.conv2": "encoder.down.1.block.0.conv2",
    "encoder.down_blocks.1.resnets.0.conv_shortcut": "encoder.down.1.block.0.nin_shortcut",
    "encoder.mid_block.resnets.0.norm1": "encoder.mid.block_1.norm1",
    "encoder.mid_block.resnets.0.conv1": "encoder.mid.block_1.conv1",
    "encoder.mid_block.resnets.0.norm2": "encoder.mid.block_1.norm2",
    "encoder.mid_block.resnets.0.conv2": "encoder.mid.block_1.conv2",
    "encoder.mid_block.attentions.0.group_norm": "encoder.mid.attn_1.norm",
    "encoder.mid_block.attentions.0.to_q": "encoder.mid.attn_1.q",
    "encoder.mid_block.attentions.0.to_k": "encoder.mid.attn_1.k",
    "encoder.mid_block.attentions.0.to_v": "encoder.mid.attn_1.v",
    "encoder.mid_block.attentions.0.to_out.0": "encoder.mid.attn_1.proj_out",
    "encoder.mid_block.resnets.1.norm1": "encoder.mid.block_2.norm1",
    "encoder.mid_block.resnets.1.conv1": "encoder.mid.block_2.conv1",
    "encoder.mid_block.resnets.1.norm2": "encoder.mid.block_2.norm2",
    "encoder.mid_block.resnets.1.conv2": "encoder.mid.block_2.conv2",
    "encoder.conv_norm_out": "encoder.norm_out",
    "encoder.conv_out": "encoder.conv_out",
    "quant_conv": "quant_conv",
    "post_quant_conv": "post_quant_conv",
    "decoder.conv_in": "decoder.conv_in",
    "decoder.mid_block.resnets.0.norm1": "decoder.mid.block_1.norm1",
    "decoder.mid_block.resnets.0.conv1": "decoder.mid.block_1.conv1",
    "decoder.mid_block.resnets.0.norm2": "decoder.mid.block_1.norm2",
    "decoder.mid_block.resnets.0.conv2": "decoder.mid.block_1.conv2",
    "decoder.mid_block.attentions.0.group_norm": "decoder.mid.attn_1.norm",
    "decoder.mid_block.attentions.0.to_q": "decoder.mid.attn_1.q",
    "decoder.mid_block.attentions.0.to_k": "decoder.mid.attn_1.k",
    "decoder.mid_block.attentions.0.to_v": "decoder.mid.attn_1.v",
    "decoder.mid_block.attentions.0.to_out.0": "decoder.mid.attn_1.proj_out",
    "decoder.mid_block.resnets.1.norm1": "decoder.mid.block_2.norm1",
    "decoder.mid_block.resnets.1.conv1": "decoder.mid.block_2.conv1",
    "decoder.mid_block.resnets.1.norm2": "decoder.mid.block_2.norm2",
    "decoder.mid_block.resnets.1.conv2": "decoder.mid.block_2.conv2",
    # diffusers counts the up blocks from the coarsest: up_blocks.0 is the reference's up.1 (the level that upsamples)
    "decoder.up_blocks.0.resnets.0.norm1": "decoder.up.1.block.0.norm1",
    "decoder.up_blocks.0.resnets.0.conv1": "decoder.up.1.block.0.conv1",
    "decoder.up_blocks.0.resnets.0.norm2": "decoder.up.1.block.0.norm2",
    "decoder.up_blocks.0.resnets.0.conv2": "decoder.up.1.block.0.conv2",
    "decoder.up_blocks.0.resnets.1.norm1": "decoder.up.1.block.1.norm1",
    "decoder.up_blocks.0.resnets.1.conv1": "decoder.up.1.block.1.conv1",
    "decoder.up_blocks.0.resnets.1.norm2": "decoder.up.1.block.1.norm2",
    "decoder.up_blocks.0.resnets.1.conv2": "decoder.up.1.block.1.conv2",
    "decoder.up_blocks.0.upsamplers.0.conv": "decoder.up.1.upsample.conv",
    "decoder.up_blocks.1.resnets.0.norm1": "decoder.up.0.block.0.norm1",
    "decoder.up_blocks.1.resnets.0.conv1": "decoder.up.0.block.0.conv1",
    "decoder.up_blocks.1.resnets.0.norm2": "decoder.up.0.block.0.norm2",
    "decoder.up_blocks.1.resnets.0.conv2": "decoder.up.0.block.0.conv2",
    "decoder.up_blocks.1.resnets.0.conv_shortcut": "decoder.up.0.block.0.nin_shortcut",
    "decoder.up_blocks.1.resnets.1.norm1": "decoder.up.0.block.1.norm1",
    "decoder.up_blocks.1.resnets.1.conv1": "decoder.up.0.block.1.conv1",
    "decoder.up_blocks.1.resnets.1.norm2": "decoder.up.0.block.1.norm2",
    "decoder.up_blocks.1.resnets.1.conv2": "decoder.up.0.block.1.conv2",
    "decoder.conv_norm_out": "decoder.norm_out",
    "decoder.conv_out": "decoder.conv_out",
}
LEGACY = {"to_q": "query", "to_k": "key", "to_v": "value", "to_out.0": "proj_attn"}

SD_VAE_FT_EMA = {   # config.json of stabilityai/sd-vae-ft-ema
    "_class_name": "AutoencoderKL", "act_fn": "silu", "block_out_channels": [128, 256, 512, 512],
    "down_block_types": ["DownEncoderBlock2D"] * 4, "in_channels": 3, "latent_channels": 4, "layers_per_block": 2, "norm_num_groups": 32,
    "out_channels": 3, "sample_size": 256, "up_block_types": ["UpDecoderBlock2D"] * 4,
}


def spell(d, legacy):
    """a TABLE key with the attention projections in the legacy spelling where asked"""
    for new, old in LEGACY.items():
        if legacy and d.endswith(".attentions.0." + new):
            return d[: -len(new)] + old
    return d


def own_shapes():
    import dfot_amd
    dec, enc = dfot_amd.ImageVAEDecoder(**CFG), dfot_amd.ImageVAEEncoder(**CFG)      # constructing a module does not touch the GPU
    return {n: tuple(t.shape) for m in (dec, enc) for n, t in m.named_parameters()}


def diffusers_state(legacy=False):
    """a state dict in the diffusers layout with the shapes of the two-level configuration, built from the literal TABLE"""
    shapes = own_shapes()
    state = {}
    for d, r in TABLE.items():
        d = spell(d, legacy)
        for leaf in ("weight", "bias"):
            s = shapes[f"{r}.{leaf}"]
            if ".attentions.0." in d and leaf == "weight" and len(s) == 4:
                s = s[:2]                                                            # a Linear there
            state[f"{d}.{leaf}"] = torch.randn(s, generator=torch.Generator().manual_seed(len(state)))
    return state


def test_restatement_vs_the_1024_position_fixture():
    g = c1k.load()
    p = c1k.seeded_params(g)
    assert p.keys() == c1k.param_shapes(CFG).keys() and all(tuple(p[n].shape) == s for n, s in c1k.param_shapes(CFG).items())
    with torch.no_grad():
        frames = c1k.decode(p, CFG, c1k.T(g["z_c"]))
        moments = c1k.encode(p, CFG, 2.0 * c1k.T(g["y_c"]) - 1.0)
    torch.testing.assert_close(frames, c1k.T(g["frames_c"]), rtol=1e-3, atol=2e-4)       # the bar of tests/test_image_vae_host.py
    torch.testing.assert_close(moments, c1k.T(g["moments_c"]), rtol=1e-3, atol=2e-4)
    assert float(g["uniform_attention_frames"]) >= 4e-2 and float(g["uniform_attention_moments"]) >= 4e-2


@pytest.mark.parametrize("legacy", [False, True])
def test_literal_key_table_maps_onto_the_modules_keys_with_nothing_left_over(legacy):
    import dfot_amd
    shapes = own_shapes()
    assert TABLE["decoder.up_blocks.0.resnets.0.conv1"] == "decoder.up.1.block.0.conv1"
    assert TABLE["decoder.up_blocks.0.upsamplers.0.conv"] == "decoder.up.1.upsample.conv"
    state = diffusers_state(legacy)
    assert ("decoder.mid_block.attentions.0.query.weight" in state) == legacy
    out = dfot_amd.diffusers_to_reference_keys(state, LEVELS)
    assert {n: tuple(t.shape) for n, t in out.items()} == shapes                        # every key, no other, Linear -> 1x1 conv shapes
    assert len(out) == len(state) == 2 * len(TABLE)
    for d, r in TABLE.items():                                                          # and each tensor went where the table says
        d = spell(d, legacy)
        for leaf in ("weight", "bias"):
            assert torch.equal(out[f"{r}.{leaf}"].reshape(-1), state[f"{d}.{leaf}"].reshape(-1)), d
    # the other way: the helper's independent statement of the map gives the table's left column back
    assert {c1k.to_diffusers_name(f"{r}.weight", LEVELS, legacy): r for r in TABLE.values()} == {f"{spell(d, legacy)}.weight": r
                                                                                                  for d, r in TABLE.items()}


def test_linear_projections_become_1x1_convolutions():
    import dfot_amd
    state = diffusers_state()
    w = state["decoder.mid_block.attentions.0.to_out.0.weight"]
    assert w.shape == (256, 256)
    out = dfot_amd.diffusers_to_reference_keys(state, LEVELS)
    got = out["decoder.mid.attn_1.proj_out.weight"]
    assert got.shape == (256, 256, 1, 1) and torch.equal(got[:, :, 0, 0], w)             # [out, in] stays [out, in]
    assert out["decoder.mid.attn_1.norm.weight"].shape == (256,) and out["decoder.mid.attn_1.proj_out.bias"].shape == (256,)
    # a checkpoint that already stores 1x1 convolutions passes through
    state["decoder.mid_block.attentions.0.to_out.0.weight"] = w.reshape(256, 256, 1, 1)
    assert torch.equal(dfot_amd.diffusers_to_reference_keys(state, LEVELS)["decoder.mid.attn_1.proj_out.weight"], got)


def test_strict_loading_names_the_key():
    import dfot_amd
    state = diffusers_state()
    dec = dfot_amd.ImageVAEDecoder(**CFG)
    ignored = dec.load_diffusers_state_dict(state)
    assert ignored and all(n.startswith(("encoder.", "quant_conv.")) for n in ignored)
    assert torch.equal(dict(dec.named_parameters())["decoder.up.1.upsample.conv.weight"], state["decoder.up_blocks.0.upsamplers.0.conv.weight"])
    enc = dfot_amd.ImageVAEEncoder(**CFG)
    enc.load_diffusers_state_dict(state)
    assert torch.equal(dict(enc.named_parameters())["encoder.mid.attn_1.k.weight"][:, :, 0, 0], state["encoder.mid_block.attentions.0.to_k.weight"])
    for bad in ("decoder.up_blocks.0.attentions.0.to_q.weight", "decoder.up_blocks.2.resnets.0.conv1.weight", "model_ema.decay",
                "decoder.mid_block.resnets.2.conv1.weight", "encoder.up_blocks.0.resnets.0.conv1.weight"):
        with pytest.raises(ValueError, match=bad.replace(".", r"\.")):
            dec.load_diffusers_state_dict({**state, bad: torch.zeros(1)})
    missing = "decoder.up_blocks.0.upsamplers.0.conv.weight"
    with pytest.raises(ValueError, match=r"decoder\.up\.1\.upsample\.conv\.weight"):
        dec.load_diffusers_state_dict({k: v for k, v in state.items() if k != missing})
    with pytest.raises(ValueError, match=r"size mismatch for decoder\.mid\.attn_1\.q\.weight"):
        dec.load_diffusers_state_dict({**state, "decoder.mid_block.attentions.0.to_q.weight": torch.zeros(256, 128)})
    with pytest.raises(ValueError, match="map to"):                                      # both attention spellings at once
        dec.load_diffusers_state_dict({**state, "decoder.mid_block.attentions.0.query.weight": torch.zeros(256, 256)})


def test_config_of_sd_vae_ft_ema_is_the_recipes_ddconfig():
    import dfot_amd
    dd = dfot_amd.ddconfig_from_diffusers(SD_VAE_FT_EMA)
    # configurations/algorithm/vae/image_vae.yaml's ddconfig, at the resolution of the Taichi recipes
    assert dd == dict(ch=128, ch_mult=[1, 2, 4, 4], num_res_blocks=2, z_channels=4, embed_dim=4, in_channels=3, out_ch=3, resolution=256)
    dec, enc = dfot_amd.ImageVAEDecoder(**dd), dfot_amd.ImageVAEEncoder(**dd)
    assert {**dict(dec.named_parameters()), **dict(enc.named_parameters())}.keys() == c1k.param_shapes(c1k.RECIPE).keys()
    for field, value in (("norm_num_groups", 16), ("act_fn", "gelu"), ("down_block_types", ["DownEncoderBlock2D"] * 3 + ["AttnDownEncoderBlock2D"]),
                         ("up_block_types", ["AttnUpDecoderBlock2D"] + ["UpDecoderBlock2D"] * 3), ("use_quant_conv", False),
                         ("use_post_quant_conv", False), ("mid_block_add_attention", False)):
        with pytest.raises(NotImplementedError, match=field):
            dfot_amd.ddconfig_from_diffusers({**SD_VAE_FT_EMA, field: value})
    ok = {**SD_VAE_FT_EMA, "use_quant_conv": True, "use_post_quant_conv": True, "mid_block_add_attention": True, "scaling_factor": 0.18215}
    assert dfot_amd.ddconfig_from_diffusers(ok) == dd


def test_safetensors_round_trip(tmp_path):
    st = pytest.importorskip("safetensors.torch")
    import dfot_amd
    state = diffusers_state()
    config = {**SD_VAE_FT_EMA, "block_out_channels": [128, 256], "down_block_types": ["DownEncoderBlock2D"] * 2,
              "up_block_types": ["UpDecoderBlock2D"] * 2, "layers_per_block": 1, "sample_size": 64}
    folder = tmp_path / "vae"
    os.makedirs(folder)
    st.save_file(state, str(folder / "diffusion_pytorch_model.safetensors"))
    with open(folder / "config.json", "w") as fh:
        json.dump(config, fh)
    want = dfot_amd.diffusers_to_reference_keys(state, LEVELS)
    for args in ((str(folder),), (str(folder / "diffusion_pytorch_model.safetensors"), config)):
        dd, sd = dfot_amd.load_diffusers_checkpoint(*args)
        assert dd == {k: (list(v) if k == "ch_mult" else v) for k, v in CFG.items() if k != "attn_resolutions"} | {"in_channels": 3}
        assert sd.keys() == want.keys() and all(torch.equal(sd[n], want[n]) for n in want)
        dfot_amd.ImageVAEDecoder(**dd).load_reference_state_dict(sd)
    with pytest.raises(ValueError, match="config"):
        dfot_amd.load_diffusers_checkpoint(str(folder / "diffusion_pytorch_model.safetensors"))


def test_mid_attention_row_rule():
    import dfot_amd
    dec = dfot_amd.ImageVAEDecoder(**CFG)
    dec._check_rows(1, 32, 32, "latents")          # 1024 positions: a 256 x 256 frame
    dec._check_rows(1, 16, 32, "latents")          # 512: rectangular maps fall under the same rule
    dec._check_rows(1, 64, 64, "latents")          # 4096: a 512 x 512 frame
    dec._check_rows(2, 8, 8, "latents")
    with pytest.raises(ValueError, match="supported"):
        dec._check_rows(1, 24, 24, "latents")      # 576: no multiple of 256
    with pytest.raises(ValueError, match="supported"):
        dec._check_rows(2, 4, 4, "latents")
    with pytest.raises(ValueError, match="supported"):
        dec._check_rows(1, 128, 64, "latents")     # 8192: past the kernel's range
