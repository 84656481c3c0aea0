"""CPU: the torch restatement of the TiTok-KL encoder (tests/titok_enc_common.py) against the fixture captured from the reference's own
TiTok_KL source (tests/golden/titok_enc.npz, tools/make_golden_titok_enc.py), the product module's state-dict inventory, strict loading,
refusals, the C ABI's three new symbols, and guards that the fixture depends on the image and on how `reshape` is read.

Bars:
  * restatement against the fixture: rel-L2 <= 1e-4, the bar SURVEY section 8c sets for whole-model CPU restatements (measured: below 2e-6);
  * `bar(case)` = 2 x rel_autocast_moments_<case> is what tests/test_gpu_titok_enc.py holds the engine to; the fixture's two guards
    (another image, the transposing reading of the reshape) must each move the moments by at least 5 x that."""
import ctypes
import os
import re

import pytest
import torch

import titok_common as tc
import titok_enc_common as te

G = te.load()
CASES = ["a", "b", "c"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dfot_op_titok_patch_rows", "dfot_op_titok_enc_tokens", "dfot_op_titok_moments")
_REST = {}


def bar(case):
    return 2.0 * float(G[f"rel_autocast_moments_{case}"])


def restated(case):
    """(params, cfg, moments of the restatement on the fixture's frames), computed once per case"""
    if case not in _REST:
        p, cfg = te.seeded_params(G, case), te.config(case)
        with torch.no_grad():
            _REST[case] = (p, cfg, te.moments(p, cfg, te.inputs(G, case)))
    return _REST[case]


@pytest.mark.parametrize("case", CASES)
def test_restatement_vs_reference_fixture(case):
    _, _, mom = restated(case)
    ref = te.T(G[f"moments_{case}"])
    r = te.rel(mom, ref)
    print(f"case {case} moments: rel-L2 {r:.3e}, max abs diff {(mom - ref).abs().max().item():.3e}")
    assert mom.shape == ref.shape == (te.CASES[case]["frames"], 8, 1, 32)
    assert r <= 1e-4
    mean, logvar, _ = te.posterior(mom)
    assert torch.equal(mean, mom[:, :4]) and torch.equal(logvar, mom[:, 4:].clamp(-30.0, 20.0))


@pytest.mark.parametrize("case", CASES)
def test_the_reshape_is_not_a_transpose(case):
    """step 5 read as `permute(0, 2, 1)` in front of the reshape gives other moments: the fixture pins the reinterpreting reading"""
    p, cfg, _ = restated(case)
    with torch.no_grad():
        wrong = te.moments(p, cfg, te.inputs(G, case), reading="transpose")
    r = te.rel(wrong, te.T(G[f"moments_{case}"]))
    print(f"case {case}: the transposing reading differs from the fixture by rel-L2 {r:.3f} ({r / bar(case):.1f} x bar)")
    assert r > 5 * bar(case)


@pytest.mark.parametrize("case", CASES)
def test_fixture_depends_on_the_image(case):
    """Sensitivity guard: the moments of the second, independent input differ from the first's by at least 5 x the GPU test's bar (and the
    restatement reproduces the second ones too).  The gains that make it so are the recorded ones."""
    p, cfg, _ = restated(case)
    assert float(G["qk_gain"]) == 2.0 and float(G["patch_gain"]) == 8.0
    ref, ref2 = te.T(G[f"moments_{case}"]), te.T(G[f"moments2_{case}"])
    r = te.rel(ref2, ref)
    print(f"case {case}: moments of two independent inputs differ by rel-L2 {r:.3f} ({r / bar(case):.1f} x bar)")
    assert r >= 5 * bar(case)
    with torch.no_grad():
        assert te.rel(te.moments(p, cfg, te.inputs(G, case, "x2")), ref2) <= 1e-4


@pytest.mark.parametrize("case", CASES)
def test_product_module_registers_the_reference_keys(case):
    import dfot_amd
    shapes = te.key_shapes(G, case)
    enc = dfot_amd.TiTokEncoder(**te.config(case), use_l2_norm=True, vit_dec_model_size="small", vit_dec_patch_size=16, use_checkpoint=True)
    own = {n: tuple(t.shape) for n, t in enc.named_parameters()}
    assert own == shapes
    assert list(own) == list(shapes)                       # registration order of the reference: latent_tokens first
    assert all(not t.is_cuda for t in enc.parameters())   # no GPU touched
    assert list(own)[0] == "latent_tokens" and own["encoder.patch_embed.weight"] == (enc.width, 3, 16, 16)
    assert own["encoder.conv_out.weight"] == (8, enc.width, 1, 1)


def test_strict_loading_and_ignored_decoder_keys():
    import dfot_amd
    p = te.seeded_params(G, "a")
    dec = {n: torch.zeros(s) for n, s in tc.key_shapes(tc.load(), "a").items()}
    enc = dfot_amd.TiTokEncoder(**te.config("a"))
    assert enc.load_reference_state_dict({**p, **dec}) == list(dec)
    assert all(torch.equal(t, p[n]) for n, t in enc.named_parameters())
    assert enc.load_reference_state_dict({"vae." + n: t for n, t in p.items()}) == []
    for gone in ("latent_tokens", "encoder.transformer.3.attn.in_proj_weight"):
        with pytest.raises(ValueError, match=gone):
            enc.load_reference_state_dict({n: t for n, t in p.items() if n != gone})
    with pytest.raises(ValueError, match="size mismatch for encoder.conv_out.weight"):
        enc.load_reference_state_dict({**p, "encoder.conv_out.weight": torch.zeros(24, 512, 1, 1)})
    with pytest.raises(ValueError, match="unexpected key.*quantize.embedding"):
        enc.load_reference_state_dict({**p, "quantize.embedding.weight": torch.zeros(2, 2)})


def test_the_decoder_still_ignores_and_returns_the_encoder_keys():
    import dfot_amd
    gd = tc.load()
    p_enc, p_dec = te.seeded_params(G, "a"), tc.seeded_params(gd, "a")
    dec = dfot_amd.TiTokDecoder(**tc.config("a"))
    assert dec.load_reference_state_dict({**p_enc, **p_dec}) == list(p_enc)
    assert list(p_enc) == [str(n) for n in gd["ignored_a"]]          # the two fixtures name the same keys, in the same order
    assert all(torch.equal(t, p_dec[n]) for n, t in dec.named_parameters())


def test_refusals_name_the_field():
    import dfot_amd
    from dfot_amd import titok
    with pytest.raises(ValueError, match="vit_enc_model_size='huge'"):
        dfot_amd.TiTokEncoder(vit_enc_model_size="huge")
    with pytest.raises(NotImplementedError, match="vit_enc_patch_size=8"):
        dfot_amd.TiTokEncoder(vit_enc_patch_size=8)
    with pytest.raises(ValueError, match="image_size=250"):
        dfot_amd.TiTokEncoder(image_size=250)
    with pytest.raises(ValueError, match="token_size=65.*128"):
        dfot_amd.TiTokEncoder(token_size=65)
    with pytest.raises(ValueError, match="num_latent_tokens=0"):
        dfot_amd.TiTokEncoder(num_latent_tokens=0)
    lmax = titok.max_sequence_length()
    too_big = 16 * (int((lmax - 33) ** 0.5) + 1)
    with pytest.raises(ValueError, match=f"image_size={too_big}.*{lmax}"):
        dfot_amd.TiTokEncoder(image_size=too_big, vit_enc_model_size="small")
    dfot_amd.TiTokEncoder(vit_enc_model_size="small", vit_dec_model_size="huge", vit_dec_patch_size=8)   # decoder-only keywords: ignored
    enc = dfot_amd.TiTokEncoder(**te.config("a"))
    with pytest.raises(ValueError, match="GPU only"):
        enc.encode(torch.zeros(2, 3, 64, 64))
    with pytest.raises(ValueError, match="GPU only"):
        enc.encode_moments(torch.zeros(2, 3, 64, 64))
    with pytest.raises(ValueError, match=r"\(F, 3, 64, 64\)"):
        enc.encode(torch.zeros(2, 3, 32, 64))
    with pytest.raises(ValueError, match="b t c h w"):
        dfot_amd.encode_titok_frames(enc, torch.zeros(1, 2, 3, 64, 64), shape="b c t h w")
    with pytest.raises(ValueError, match=r"\(B, T, 3, S, S\)"):
        dfot_amd.encode_titok_frames(enc, torch.zeros(2, 3, 64, 64))


def test_the_new_ops_are_declared_bound_documented_and_exported():
    from dfot_amd import capi
    header = open(os.path.join(ROOT, "include", "dfot_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    exported = ctypes.CDLL(capi.LIB_PATH)
    for sym in SYMBOLS:
        assert re.search(rf"\bint {sym}\(", header), f"{sym} is not declared in include/dfot_hip.h"
        assert sym in capi.SIGNATURES and callable(getattr(capi.lib, sym))
        assert f"`{sym}`" in integration, f"{sym} is not in INTEGRATION.md's ABI table"
        assert getattr(exported, sym) is not None
    # the argument counts of the bindings are the header's
    for sym in SYMBOLS:
        decl = re.search(rf"\bint {sym}\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == len(capi.SIGNATURES[sym][1])


def test_checkpoint_round_trip_feeds_both_halves(tmp_path):
    import dfot_amd
    from safetensors.torch import save_file
    p_enc, p_dec = te.seeded_params(G, "a"), tc.seeded_params(tc.load(), "a")
    path = str(tmp_path / "model.safetensors")
    save_file({n: t.contiguous() for n, t in {**p_enc, **p_dec}.items()}, path)
    sd = dfot_amd.load_titok_checkpoint(path)
    enc, dec = dfot_amd.TiTokEncoder(**te.config("a")), dfot_amd.TiTokDecoder(**tc.config("a"))
    assert sorted(enc.load_reference_state_dict(sd)) == sorted(p_dec) and sorted(dec.load_reference_state_dict(sd)) == sorted(p_enc)
    assert all(torch.equal(t, p_enc[n]) for n, t in enc.named_parameters())
