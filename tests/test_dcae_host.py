"""CPU: the torch restatement of the DC-AE (tests/dcae_common.py) against the fixture captured from the reference's own Encoder / Decoder
source (tests/golden/dcae.npz, tools/make_golden_dcae.py), the sensitivities the fixture records, the product modules' state-dict
inventory, every refusal (raised before anything touches the device), the C ABI declarations of the new ops and the BatchNorm fold.

The fixture's diffusers layers are stand-ins written from knowledge of diffusers 0.32.2, unverified against the library
(tools/ref_loader.py): what is pinned here is pinned to them.

Bar of the restatement: both sides are fp32 torch, so 4x the deviation the tool measured when the fixture was made (7.8e-7 for f8, 1.0e-6
for f16), as tests/test_dit_fac_train_host.py does; floor 2e-6 for another BLAS / thread count (a few fp32 roundings, 6e-8 each, through
about 30 layers)."""
import os
import re

import pytest
import torch

import dcae_common as dc
from conftest import ROOT

G = dc.load()
FLOOR = 2e-6


@pytest.fixture(scope="module", params=list(dc.CASES))
def case(request):
    c = dc.CASES[request.param]
    p = dc.seeded_params(dc.key_shapes(G, request.param))
    x = 2.0 * (dc.T(G[f"y_{request.param}"]).float() / 255.0) - 1.0
    return request.param, dc.config(c), p, x, dc.T(G[f"latents_{request.param}"]), dc.T(G[f"recon_{request.param}"])


def test_fixture_is_data_only_and_small():
    import numpy
    assert all(isinstance(G[k], numpy.ndarray) for k in G.files)
    assert os.path.getsize(os.path.join(dc.GOLDEN, "dcae.npz")) < 1 << 20
    for tag, c in dc.CASES.items():
        r = 2 ** (len(c["channels"]) - 1)
        assert G[f"y_{tag}"].shape == (3, 3, c["size"], c["size"]) and G[f"latents_{tag}"].shape == (3, 32, c["size"] // r, c["size"] // r)
        assert G[f"recon_{tag}"].shape == G[f"y_{tag}"].shape
        assert any(n.endswith("running_var") for n in dc.key_shapes(G, tag)) and any(".norm.weight" in n for n in dc.key_shapes(G, tag))


def test_seeded_weights_are_the_fixture_s(case):
    tag, _, p, *_ = case
    assert dc.digest(p) == int(G[f"digest_{tag}"])


def test_restatement_vs_reference_fixture(case):
    tag, cfg, p, x, lat, rec = case
    with torch.no_grad():
        d_lat, d_rec = dc.rel(dc.encode(p, cfg, x), lat), dc.rel(dc.decode(p, cfg, lat), rec)
    stored = float(G[f"host_rel_{tag}"])
    print(f"{tag}: restatement vs fixture: latents {d_lat:.2e}, reconstruction {d_rec:.2e} (when the fixture was made: {stored:.2e})")
    assert stored < 1e-5
    assert max(d_lat, d_rec) <= max(4 * stored, FLOOR)


@pytest.mark.parametrize("mistake", dc.MISTAKES)
def test_sensitivities_clear_twice_the_parity_bar(case, mistake):
    """each deliberate mistake moves the result by at least 2x the GPU parity bar, in the fixture's record and re-measured here"""
    tag, cfg, p, x, lat, rec = case
    with torch.no_grad():
        s_lat, s_rec = dc.rel(dc.encode(p, cfg, x, mistake=mistake), lat), dc.rel(dc.decode(p, cfg, lat, mistake=mistake), rec)
    print(f"{tag} {mistake}: latents move by {s_lat:.3f} (stored {float(G[f'sens_{mistake}_lat_{tag}']):.3f}), reconstruction by {s_rec:.3f} "
          f"(stored {float(G[f'sens_{mistake}_rec_{tag}']):.3f})")
    for got, key in ((s_lat, "lat"), (s_rec, "rec")):
        stored = float(G[f"sens_{mistake}_{key}_{tag}"])
        assert abs(got - stored) <= 1e-3 * max(stored, 1.0)
        if not (mistake == "batch_stats" and key == "lat"):   # the encoder has no BatchNorm: its ResBlocks are hard-wired to rms_norm
            assert stored >= 2 * dc.BAR
    if mistake == "batch_stats":   # no BatchNorm on that path: only the restatement's own deviation from the fixture is left
        assert s_lat <= max(4 * float(G[f"host_rel_{tag}"]), FLOOR)


def test_product_modules_register_the_reference_keys_in_order(case):
    import dfot_amd
    tag, cfg, *_ = case
    shapes = dc.key_shapes(G, tag)
    enc, dec = dfot_amd.DCAEEncoder(**cfg), dfot_amd.DCAEDecoder(**cfg)      # constructing a module does not touch the GPU
    own_e = {n: tuple(t.shape) for n, t in enc.state_dict().items()}
    own_d = {n: tuple(t.shape) for n, t in dec.state_dict().items()}
    assert list(own_e) == [n for n in shapes if n.startswith("encoder.")]
    assert list(own_d) == [n for n in shapes if n.startswith("decoder.")]
    assert own_e == {n: s for n, s in shapes.items() if n.startswith("encoder.")}
    assert own_d == {n: s for n, s in shapes.items() if n.startswith("decoder.")}
    assert len(own_e) + len(own_d) == len(shapes)
    assert any(n.endswith("norm.num_batches_tracked") for n in own_d) and not any("running" in n for n in own_e)
    assert dec.state_dict()[next(n for n in own_d if n.endswith("num_batches_tracked"))].dtype == torch.long


def test_strict_loading_on_the_host(case):
    import dfot_amd
    tag, cfg, p, *_ = case
    enc, dec = dfot_amd.DCAEEncoder(**cfg), dfot_amd.DCAEDecoder(**cfg)
    assert sorted(enc.load_reference_state_dict(p)) == sorted(n for n in p if n.startswith("decoder."))
    assert sorted(dec.load_reference_state_dict({"vae." + n: t for n, t in p.items()})) == sorted("vae." + n for n in p if n.startswith("encoder."))
    name = next(n for n in p if n.endswith("running_var"))
    assert torch.equal(dec.state_dict()[name], p[name])
    with pytest.raises(ValueError, match="keys not found"):
        dec.load_reference_state_dict({n: t for n, t in p.items() if n != name})
    with pytest.raises(ValueError, match="size mismatch"):
        dec.load_reference_state_dict({**p, name: torch.zeros(3)})


def test_stock_configurations_build():
    import dfot_amd
    for kind, stages, r in (("8x", 4, 8), ("16x", 5, 16)):
        cfg = dfot_amd.dcae_config(kind)
        enc, dec = dfot_amd.DCAEEncoder(**cfg), dfot_amd.DCAEDecoder(**cfg)
        assert len(enc.ch) == stages and enc.s_factor == dec.s_factor == r and enc.scaling_factor == 0.2889
    with pytest.raises(ValueError, match="unknown DC-AE configuration"):
        dfot_amd.dcae_config("32x")
    # the non-model keys of the reference's yaml files are accepted
    dfot_amd.DCAEDecoder(**dfot_amd.dcae_config("8x"), name="dc_ae_preprocessor", pretrained_path=None, pretrained_kwargs={}, batch_size=4)


@pytest.mark.parametrize("cls,side", [("DCAEEncoder", "encoder"), ("DCAEDecoder", "decoder")])
def test_constructor_refusals(cls, side):
    import dfot_amd
    make = getattr(dfot_amd, cls)
    base = dc.config(dc.CASES["f8"])

    def bad(exc, match, **kw):
        with pytest.raises(exc, match=match):
            make(**{**base, **kw})
    bad(NotImplementedError, f"{side}_qkv_multiscales", **{f"{side}_qkv_multiscales": [[], [], [], [5]]})
    bad(NotImplementedError, "downsample_block_type", downsample_block_type="Conv")
    bad(NotImplementedError, "upsample_block_type", upsample_block_type="interpolate")
    bad(NotImplementedError, "attention_head_dim", attention_head_dim=16)
    bad(NotImplementedError, f"{side}_block_types", **{f"{side}_block_types": ["ResBlock", "ResBlock", "AttnBlock", "EfficientViTBlock"]})
    bad(NotImplementedError, "use_fp16", use_fp16=True)
    bad(NotImplementedError, "in_channels", in_channels=1)
    bad(NotImplementedError, "latent_channels", latent_channels=16)
    bad(NotImplementedError, f"{side}_layers_per_block", **{f"{side}_layers_per_block": [1, 1, 1, 1]})
    bad(ValueError, f"{side}_block_out_channels", **{f"{side}_block_out_channels": [64, 96, 128, 128]})
    bad(ValueError, f"{side}_block_out_channels", **{f"{side}_block_out_channels": [64, 64, 128, 2048]})
    bad(TypeError, "unknown configuration keys", attn_resolutions=[])
    if cls == "DCAEDecoder":
        bad(NotImplementedError, "decoder_act_fns", decoder_act_fns=["relu", "relu6", "relu", "silu"])
        bad(NotImplementedError, "decoder_norm_types", decoder_norm_types=["batch_norm", "group_norm", "batch_norm", "rms_norm"])
        bad(NotImplementedError, "decoder_norm_types", decoder_norm_types="batch_norm")
    make(**{**base, f"{side}_block_types": "ResBlock"})          # one string for all stages, as the reference accepts


def test_call_time_refusals_before_any_launch():
    import dfot_amd
    cfg = dc.config(dc.CASES["f8"])
    enc, dec = dfot_amd.DCAEEncoder(**cfg), dfot_amd.DCAEDecoder(**cfg)
    with pytest.raises(ValueError, match="GPU only"):
        dec.decode(torch.zeros(3, 32, 8, 8))
    with pytest.raises(ValueError, match="GPU only"):
        enc.encode(torch.zeros(3, 3, 64, 64))
    with pytest.raises(ValueError, match=r"\(F, 32, h, w\)"):
        dec.decode(torch.zeros(3, 4, 8, 8))
    with pytest.raises(ValueError, match="spatial factor 8"):
        enc.encode(torch.zeros(1, 3, 60, 60))
    # a 4x4 map at the EfficientViT stage is 16 <= 32 positions: the reference's quadratic branch
    with pytest.raises(NotImplementedError, match="quadratic"):
        dec.decode(torch.zeros(1, 32, 4, 4))
    with pytest.raises(NotImplementedError, match="quadratic"):
        enc.encode(torch.zeros(1, 3, 32, 32))
    # 12 x 12 = 144 positions: more than 32, not a multiple of 64
    with pytest.raises(ValueError, match="144 positions"):
        dec.decode(torch.zeros(1, 32, 12, 12))
    with pytest.raises(ValueError, match="positions"):
        dec.decode(torch.zeros(1, 32, 128, 128))
    with pytest.raises(NotImplementedError, match="autograd"):
        dec.decode(torch.zeros(1, 32, 8, 8, requires_grad=True))
    with pytest.raises(NotImplementedError, match="autograd"):
        enc.encode(torch.zeros(1, 3, 64, 64, requires_grad=True))
    with pytest.raises(ValueError, match="b t c h w"):
        dfot_amd.decode_dcae_latents(dec, torch.zeros(1, 2, 32, 8, 8), shape="b c t h w")
    with pytest.raises(ValueError, match=r"\(B, T, 3, H, W\)"):
        dfot_amd.encode_dcae_frames(enc, torch.zeros(2, 3, 64, 64))


def test_header_declares_and_capi_binds_the_new_ops():
    from dfot_amd import capi
    header = open(os.path.join(ROOT, "include", "dfot_hip.h")).read()
    nargs = {"dfot_op_dcae_linear_attention": 8, "dfot_op_dcae_dw_glu": 9, "dfot_op_dcae_down_shortcut": 11, "dfot_op_dcae_up_shortcut": 12,
             "dfot_op_dcae_rmsnorm": 11, "dfot_op_dcae_act_bf16": 5}
    for name, n in nargs.items():
        m = re.search(rf"\bint {name}\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == n, name
        assert name in capi.SIGNATURES and hasattr(capi.lib, name) and len(capi.SIGNATURES[name][1]) == n


def test_batch_norm_fold_equals_eval_mode_batchnorm_in_fp64():
    import dfot_amd
    g = torch.Generator().manual_seed(5)
    co, ci = 12, 8
    bn = torch.nn.BatchNorm2d(co, eps=1e-5).double().eval()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * torch.randn(co, generator=g, dtype=torch.float64))
        bn.bias.copy_(0.2 * torch.randn(co, generator=g, dtype=torch.float64))
        bn.running_mean.copy_(0.5 * torch.randn(co, generator=g, dtype=torch.float64))
        bn.running_var.copy_(0.3 + torch.rand(co, generator=g, dtype=torch.float64))
        w = torch.randn(co, ci, 3, 3, generator=g, dtype=torch.float64)
        x = torch.randn(2, ci, 6, 5, generator=g, dtype=torch.float64)
        ref = bn(torch.nn.functional.conv2d(x, w, None, padding=1))
        for fold in (dfot_amd.DCAEDecoder.fold_batch_norm, dc.bn_fold):
            w2, b2 = fold(w, bn.weight, bn.bias, bn.running_mean, bn.running_var)
            got = torch.nn.functional.conv2d(x, w2, b2, padding=1)
            err = float((got - ref).abs().max() / ref.abs().max())
            print(f"{fold.__qualname__}: max deviation from eval-mode BatchNorm2d {err:.2e}")
            assert err <= 1e-12
