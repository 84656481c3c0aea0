"""GPU: the TiTok-KL decoder (dfot_amd.titok) on the three configurations of tests/golden/titok*.npz, against the fixture captured from the
reference's own TiTok_KL source in fp32 (never against the engine itself), plus frame independence, row padding, repacking and the
helper-level decode.

Bars:
  * logits (cases a, b; the module method that stops after the transformer and the ffn): rel-L2 < 2 x rel_autocast_logits_<case>, the error
    the reference itself has under torch.autocast("cpu", bfloat16) against its fp32 run (7.6e-3 / 7.8e-3, stored in the fixture); the
    factor of two covers a different rounding order and bf16 probabilities, not a wrong term.
  * frames (a, b, c), also of the pixel decoder alone fed the fixture's fp32 input: rel-L2 < max(2e-2, rel_autocast_frames_<case>); 2e-2 is
    the bar every other decoder here is held to (tests/test_gpu_vae.py:94), the reference's own bf16 autocast loses 3.8e-2 / 4.3e-2 /
    4.5e-2 on these cases.
Achieved values are printed by every test."""
import pytest
import torch

import titok_common as tc

pytestmark = pytest.mark.gpu

G = tc.load()
CASES = ["a", "b", "c"]
_CACHE = {}


def setup(case):
    """(params, cfg, decoder on the GPU), built once per case"""
    if case not in _CACHE:
        import dfot_amd
        p, cfg = tc.seeded_params(G, case), tc.config(case)
        dec = dfot_amd.TiTokDecoder(**cfg).cuda()
        assert dec.load_reference_state_dict(p) == []
        _CACHE[case] = (p, cfg, dec)
    return _CACHE[case]


def frames_bar(case):
    return max(2e-2, float(G[f"rel_autocast_frames_{case}"]))


@pytest.mark.parametrize("case", tc.LOGIT_CASES)
def test_logits_vs_reference_fixture(case):
    _, _, dec = setup(case)
    out = dec.decode_logits(tc.T(G[f"z_{case}"]).cuda()).cpu()
    ref = tc.T(G[f"logits_{case}"])
    r, bar = tc.rel(out, ref), 2.0 * float(G[f"rel_autocast_logits_{case}"])
    print(f"TiTok logits {case}: rel-L2 vs the reference fixture {r:.3e} (bar {bar:.3e})")
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert r < bar


@pytest.mark.parametrize("case", CASES)
def test_frames_vs_reference_fixture(case):
    _, _, dec = setup(case)
    z = tc.T(G[f"z_{case}"]).cuda()
    out = dec.decode(z).cpu()
    ref = tc.T(G[f"frames_{case}"])
    lat = dec.decode_pixel_input(z).cpu()
    r, r_lat = tc.rel(out, ref), tc.rel(lat, tc.T(G[f"pixel_input_{case}"]))
    print(f"TiTok decode {case}: frames rel-L2 vs the reference fixture {r:.3e} (bar {frames_bar(case):.3e}), pixel-decoder input {r_lat:.3e}, "
          f"max_abs {(out - ref).abs().max().item():.3e}")
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert r < frames_bar(case)


@pytest.mark.parametrize("case", CASES)
def test_pixel_decoder_alone_vs_reference_fixture(case):
    _, _, dec = setup(case)
    out = dec.decode_pixels(tc.T(G[f"pixel_input_{case}"]).cuda()).cpu()
    ref = tc.T(G[f"frames_{case}"])
    r = tc.rel(out, ref)
    print(f"TiTok pixel decoder {case}: rel-L2 vs the reference fixture {r:.3e} (bar {frames_bar(case):.3e})")
    assert out.shape == ref.shape and r < frames_bar(case)


def test_frames_are_independent_bit_for_bit_and_any_count_runs():
    """49-token sequences: 1, 2 and 3 frames are 49, 98 and 147 token rows (padded to 128 / 128 / 256) and 16, 32, 48 rows of the 4 x 4
    map (padded to 8 frames).  A frame decodes to the same bits alone, in a batch of 3, and under vae_batch_size 1 against 2."""
    import dfot_amd
    _, _, dec = setup("a")
    z = tc.T(G["z_a"]).cuda()
    whole = dec.decode(z)
    assert whole.shape == (3, 3, 64, 64) and torch.isfinite(whole).all()
    for f in range(3):
        assert torch.equal(dec.decode(z[f:f + 1]), whole[f:f + 1])
    assert torch.equal(dec.decode(z[:2]), whole[:2])
    assert torch.equal(dec.decode_logits(z[1:2]), dec.decode_logits(z)[1:2])
    lat = torch.stack([z, z.flip(0)], 0)[:, :2]                      # 2 videos x 2 frames
    one, two = (dfot_amd.decode_titok_latents(dec, lat, vae_batch_size=n) for n in (1, 2))
    assert torch.equal(one, two) and torch.equal(one[0], whole[:2])


def test_frames_are_independent_at_the_production_sequence():
    """289-token sequences (case c's module): 2 frames are 578 token rows, so the second sequence starts in the middle of a tile"""
    _, _, dec = setup("c")
    z = torch.cat([tc.T(G["z_c"]), tc.T(G["z2_c"])], 0).cuda()
    both = dec.decode(z)
    assert torch.equal(both[:1], dec.decode(z[:1])) and torch.equal(both[1:], dec.decode(z[1:]))
    assert tc.rel(both[:1].cpu(), tc.T(G["frames_c"])) < frames_bar("c")


def test_weights_changed_in_place_are_repacked():
    import dfot_amd
    p, cfg, _ = setup("a")
    dec = dfot_amd.TiTokDecoder(**cfg).cuda()
    dec.load_reference_state_dict(p)
    z = tc.T(G["z_a"])
    before = dec.decode(z.cuda()).cpu()
    p2 = {n: t.clone() for n, t in p.items()}
    gen = torch.Generator().manual_seed(11)
    for n in ("decoder.transformer.2.attn.in_proj_weight", "decoder.transformer.5.mlp.c_proj.weight", "pixel_decoder.up.3.block.0.nin_shortcut.weight",
              "decoder.decoder_embed.weight"):
        p2[n] = p2[n] + 0.5 * p2[n].std() * torch.randn(p2[n].shape, generator=gen)
        with torch.no_grad():
            dec.get_parameter(n).copy_(p2[n])
    with torch.no_grad():
        ref = tc.decode(p2, cfg, z)
    after = dec.decode(z.cuda()).cpu()
    r, moved = tc.rel(after, ref), tc.rel(ref, tc.T(G["frames_a"]))
    print(f"TiTok decode a after an in-place weight change: rel-L2 vs the restatement {r:.3e}; the change moved the frames by {moved:.3e}")
    assert moved > 5 * frames_bar("a") and not torch.equal(before, after)
    assert r < frames_bar("a")


def test_decode_titok_latents_matches_the_restatement():
    import dfot_amd
    p, cfg, dec = setup("a")
    gen = torch.Generator().manual_seed(12)
    lat = torch.randn(2, 3, 4, 1, 32, generator=gen)
    out = dfot_amd.decode_titok_latents(dec, lat.cuda()).cpu()
    with torch.no_grad():
        ref = tc.decode_latents(p, cfg, lat)
    r = tc.rel(out, ref)
    print(f"decode_titok_latents (2, 3, 4, 1, 32): rel-L2 vs the restatement {r:.3e}")
    assert out.shape == ref.shape == (2, 3, 3, 64, 64)
    assert r < frames_bar("a")
