"""CPU: the torch restatement of the TiTok-KL decoder (tests/titok_common.py) against the fixture captured from the reference's own
TiTok_KL source (tests/golden/titok*.npz, tools/make_golden_titok.py), the product module's state-dict inventory, strict loading,
refusals, the safetensors round trip, and a guard that the fixture depends on the latent at all.

Bar of the restatement: rel-L2 <= 1e-5 on the logits, the pixel decoder's input and the frames (fp32 against fp32 on the CPU).  Measured:
below 6e-6 on every stage of every case (the restatement spells nn.MultiheadAttention out, so the summation order differs)."""
import pytest
import torch

import titok_common as tc

G = tc.load()
CASES = ["a", "b", "c"]
_REST = {}


def restated(case):
    """(params, cfg, logits, pixel input, frames) of the restatement on the fixture's z, computed once per case"""
    if case not in _REST:
        p, cfg = tc.seeded_params(G, case), tc.config(case)
        with torch.no_grad():
            lg = tc.logits(p, cfg, tc.T(G[f"z_{case}"]))
            lat = tc.pixel_input(p, lg)
            _REST[case] = (p, cfg, lg, lat, tc.pixel_decode(p, lat))
    return _REST[case]


@pytest.mark.parametrize("case", CASES)
def test_restatement_vs_reference_fixture(case):
    p, cfg, lg, lat, frames = restated(case)
    c = tc.CASES[case]
    grid = c["image_size"] // 16
    assert lg.shape == (c["frames"], 1024, grid, grid) and frames.shape == (c["frames"], 3, c["image_size"], c["image_size"])
    stages = [(lat, "pixel_input"), (frames, "frames")] + ([(lg, "logits")] if case in tc.LOGIT_CASES else [])
    for got, key in stages:
        ref = tc.T(G[f"{key}_{case}"])
        r = tc.rel(got, ref)
        print(f"case {case} {key}: rel-L2 {r:.3e}, max abs diff {(got - ref).abs().max().item():.3e}")
        assert got.shape == ref.shape and r <= 1e-5
    assert f"logits_{case}" in G or case not in tc.LOGIT_CASES


@pytest.mark.parametrize("case", CASES)
def test_fixture_depends_on_the_latent(case):
    """Sensitivity guard: with plain seeded weights the 1024-way softmax is nearly uniform and the frames of two independent z differ by
    1.6e-2 -- less than any bf16 tolerance, so a broken transformer would pass every frame test.  With the recorded gain on
    decoder.ffn.2.weight they differ by 0.70 / 0.49 / 0.42 (a / b / c, measured on the CPU); the bar is 0.3."""
    p, cfg, _, _, frames = restated(case)
    assert float(G["ffn2_gain"]) == 8.0
    with torch.no_grad():
        other = tc.decode(p, cfg, tc.T(G[f"z2_{case}"]))
    r = tc.rel(other, frames)
    print(f"case {case}: frames of two independent z differ by rel-L2 {r:.2f}")
    assert r > 0.3


@pytest.mark.parametrize("case", CASES)
def test_product_module_registers_the_reference_keys(case):
    import dfot_amd
    shapes = tc.key_shapes(G, case)
    dec = dfot_amd.TiTokDecoder(**tc.config(case), vit_enc_model_size="small", vit_enc_patch_size=16, use_checkpoint=True)  # no GPU touched
    own = {n: tuple(t.shape) for n, t in dec.named_parameters()}
    assert own == shapes
    assert list(own) == list(shapes)                       # registration order of the reference
    assert all(not t.is_cuda for t in dec.parameters())
    ignored = [str(n) for n in G[f"ignored_{case}"]]
    assert ignored and all(n.startswith("encoder.") or n == "latent_tokens" for n in ignored) and not set(ignored) & set(own)
    # bias-free ResnetBlock convolutions; nin_shortcut only where the channel count changes, and square
    assert not any(n.endswith(("conv1.bias", "conv2.bias", "nin_shortcut.bias")) for n in own)
    assert own["pixel_decoder.up.3.block.0.nin_shortcut.weight"] == (256, 256, 1, 1)
    assert "pixel_decoder.up.2.block.0.nin_shortcut.weight" not in own and "pixel_decoder.up.0.upsample_conv.weight" not in own


def test_strict_loading_and_ignored_encoder_keys():
    import ast
    import dfot_amd
    p = tc.seeded_params(G, "a")
    enc = {str(n): torch.zeros(ast.literal_eval(str(s))) for n, s in zip(G["ignored_a"], G["ignored_shapes_a"])}
    dec = dfot_amd.TiTokDecoder(**tc.config("a"))
    assert dec.load_reference_state_dict({**enc, **p}) == list(enc)
    assert all(torch.equal(t, p[n]) for n, t in dec.named_parameters())
    assert dec.load_reference_state_dict({"vae." + n: t for n, t in p.items()}) == []
    missing = {n: t for n, t in p.items() if n != "decoder.transformer.3.attn.in_proj_weight"}
    with pytest.raises(ValueError, match="decoder.transformer.3.attn.in_proj_weight"):
        dec.load_reference_state_dict(missing)
    with pytest.raises(ValueError, match="size mismatch for pixel_quantize_conv.weight"):
        dec.load_reference_state_dict({**p, "pixel_quantize_conv.weight": torch.zeros(256, 512, 1, 1)})
    with pytest.raises(ValueError, match="unexpected key.*quantize.embedding"):
        dec.load_reference_state_dict({**p, "quantize.embedding.weight": torch.zeros(2, 2)})


def test_refusals_name_the_field():
    import dfot_amd
    from dfot_amd import titok
    with pytest.raises(ValueError, match="vit_dec_model_size='huge'"):
        dfot_amd.TiTokDecoder(vit_dec_model_size="huge")
    with pytest.raises(NotImplementedError, match="vit_dec_patch_size=8"):
        dfot_amd.TiTokDecoder(vit_dec_patch_size=8)
    with pytest.raises(ValueError, match="image_size=250"):
        dfot_amd.TiTokDecoder(image_size=250)
    lmax = titok.max_sequence_length()
    assert lmax >= 1057                                    # a 512^2 frame
    too_big = 16 * (int((lmax - 33) ** 0.5) + 1)
    with pytest.raises(ValueError, match=f"image_size={too_big}.*{lmax}"):
        dfot_amd.TiTokDecoder(image_size=too_big, vit_dec_model_size="small")
    dec = dfot_amd.TiTokDecoder(**tc.config("a"))
    with pytest.raises(ValueError, match="GPU only"):
        dec.decode(torch.zeros(2, 4, 1, 32))
    with pytest.raises(ValueError, match="GPU only"):
        dec.decode_logits(torch.zeros(2, 4, 1, 32))
    with pytest.raises(ValueError, match="GPU only"):
        dec.decode_pixels(torch.zeros(2, 256, 4, 4))
    with pytest.raises(ValueError, match=r"\(F, 4, 1, 32\)"):
        dec.decode(torch.zeros(2, 4, 32))
    with pytest.raises(ValueError, match="b t c h w"):
        dfot_amd.decode_titok_latents(dec, torch.zeros(1, 2, 4, 1, 32), shape="b c t h w")


def test_checkpoint_round_trip(tmp_path):
    import dfot_amd
    from safetensors.torch import save_file
    p = tc.seeded_params(G, "a")
    full = {**p, "latent_tokens": torch.ones(32, 512), "encoder.ln_pre.weight": torch.ones(512)}
    path = str(tmp_path / "model.safetensors")
    save_file({n: t.contiguous() for n, t in full.items()}, path)
    sd = dfot_amd.load_titok_checkpoint(path)
    assert set(sd) == set(full) and all(torch.equal(sd[n], full[n]) for n in full)
    dec = dfot_amd.TiTokDecoder(**tc.config("a"))
    assert sorted(dec.load_reference_state_dict(sd)) == ["encoder.ln_pre.weight", "latent_tokens"]
    assert all(torch.equal(t, p[n]) for n, t in dec.named_parameters())
