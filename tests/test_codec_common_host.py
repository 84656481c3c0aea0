"""Host: what the four latent codecs share (dfot_amd.codec_common) -- the split-K rule, the ``b t c h w`` chunk loop, the strict loader
and the class hierarchy.  Pure CPU: no kernel is launched."""
import inspect
import math

import pytest
import torch

import dfot_amd
from dfot_amd import codec_common as cc, dcae, image_vae, titok, vae


# ------------------------------------------------------------------ the split-K rule
def rule(rows1, n, k):
    """the rule as the codecs' bit-equality tests rely on it: K >= 2048 and ceil(rows1 / 128) * ceil(N / 128) <= 256"""
    return k >= 2048 and math.ceil(rows1 / 128) * math.ceil(n / 128) <= 256


def test_splits_k_at_its_boundaries():
    assert list(inspect.signature(cc.splits_k).parameters) == ["rows1", "n", "k"]           # one frame's rows: no batch size
    assert not cc.splits_k(64, 512, 2047) and cc.splits_k(64, 512, 2048)
    # tile products 256 and 257: 16 x 16, 1 x 256, 256 x 1 against 257 x 1, 1 x 257
    assert cc.splits_k(16 * 128, 16 * 128, 2048) and cc.splits_k(128, 256 * 128, 4096) and cc.splits_k(256 * 128, 128, 2048)
    assert not cc.splits_k(256 * 128 + 1, 128, 2048) and not cc.splits_k(128, 256 * 128 + 1, 2048)
    assert cc.splits_k(256 * 128 - 127, 1, 2048)                                                 # partial tiles count as whole ones
    for rows1 in (1, 64, 127, 128, 129, 289, 1024, 4096, 32768, 32769):
        for n in (1, 32, 128, 129, 512, 1024, 4096, 32768):
            for k in (64, 768, 2047, 2048, 4096):
                assert cc.splits_k(rows1, n, k) == rule(rows1, n, k), (rows1, n, k)


# ------------------------------------------------------------------ the chunk loop
@pytest.mark.parametrize("vae_batch_size, want", [(1, [(1, 0), (1, 1), (1, 2)]), (2, [(2, 0), (1, 2)]), (8, [(3, 0)])])
def test_map_frame_chunks_sizes_order_and_round_trip(vae_batch_size, want):
    x = torch.arange(3 * 4 * 2 * 5).reshape(3, 4, 2, 5, 1).float()
    seen = []

    def body(ch, row):
        seen.append((ch.shape[0], row))
        assert torch.equal(ch, x[row:row + ch.shape[0]])
        flat = cc.flat_frames(ch)
        assert flat.shape == (ch.shape[0] * 4, 2, 5, 1) and all(torch.equal(flat[i], ch[i // 4, i % 4]) for i in range(flat.shape[0]))
        return flat + 1.0
    out = cc.map_frame_chunks(body, x, vae_batch_size, "b t c h w", "latents", "(B, T, C, h, w)")
    assert seen == want
    assert out.shape == x.shape and torch.equal(out, x + 1.0)
    assert [c.shape[0] for c in cc.chunks(x, vae_batch_size)] == [b for b, _ in want]


def test_map_frame_chunks_refusals_come_before_the_body():
    def body(ch, row):
        raise AssertionError("the per-chunk function ran")
    x = torch.zeros(3, 4, 2, 5, 1)
    with pytest.raises(ValueError, match="^only the 'b t c h w' layout of the sampling path is supported$"):
        cc.map_frame_chunks(body, x, 2, "b c t h w", "latents", "(B, T, C, h, w)")
    with pytest.raises(ValueError, match="^only the 'b t c h w' layout of the training / sampling path is supported$"):
        cc.map_frame_chunks(body, x, 2, "b c t h w", "videos", "(B, T, 3, H, W)", "training / sampling")
    with pytest.raises(ValueError, match=r"^videos have shape \(12, 2, 5, 1\), expected \(B, T, 3, H, W\)$"):
        cc.map_frame_chunks(body, x.reshape(12, 2, 5, 1), 2, "b t c h w", "videos", "(B, T, 3, H, W)")
    for fn, arg in ((dfot_amd.decode_image_latents, "latents"), (dfot_amd.encode_image_frames, "videos"), (dfot_amd.decode_titok_latents, "latents"),
                    (dfot_amd.encode_titok_frames, "videos"), (dfot_amd.decode_dcae_latents, "latents"), (dfot_amd.encode_dcae_frames, "videos")):
        with pytest.raises(ValueError, match="only the 'b t c h w' layout"):
            fn(None, x, shape="b c t h w")
        with pytest.raises(ValueError, match=f"{arg} have shape"):
            fn(None, x[0])


# ------------------------------------------------------------------ the strict loader
class Half(cc.CodecModule):
    def __init__(self):
        super().__init__()
        self._specs = [("top", (2, 3)), ("enc.conv.weight", (4, 3, 3, 3)), ("enc.conv.bias", (4,)), ("enc.norm.weight", (4,)),
                       ("enc.norm.running_mean", (4,)), ("enc.norm.running_var", (4,)), ("enc.norm.num_batches_tracked", ())]
        self._register()


def state():
    g = torch.Generator().manual_seed(3)
    m = Half()
    return {n: (torch.tensor(7) if t.dtype == torch.long else torch.randn(t.shape, generator=g)) for n, t in m._tensors().items()}


def test_registration_follows_the_specs():
    m = Half()
    assert list(m.state_dict()) == m._names == [n for n, _ in m._specs]
    assert [n for n, _ in m.named_buffers()] == ["enc.norm.running_mean", "enc.norm.running_var", "enc.norm.num_batches_tracked"]
    assert torch.equal(m.enc.norm.running_var, torch.ones(4)) and m.enc.norm.num_batches_tracked.dtype == torch.long
    assert not any(p.requires_grad for p in m.parameters())


def test_strict_loader():
    sd = state()
    m = Half()
    assert m.load_reference_state_dict(sd) == []
    for n, t in m.state_dict().items():                     # parameters and buffers alike
        assert torch.equal(t, sd[n]), n
    m = Half()
    ignored = m.load_reference_state_dict({**{"vae." + n: v for n, v in sd.items()}, "vae.dec.conv.weight": torch.zeros(1), "loss.w": torch.zeros(1)})
    assert ignored == ["vae.dec.conv.weight", "loss.w"]    # a vae. prefix is stripped; foreign keys are returned, under their own names
    assert all(torch.equal(t, sd[n]) for n, t in m.state_dict().items())
    with pytest.raises(ValueError, match=r"keys not found in the checkpoint: \['enc.norm.running_var'\]"):
        Half().load_reference_state_dict({n: v for n, v in sd.items() if n != "enc.norm.running_var"})
    with pytest.raises(ValueError, match=r"size mismatch for enc.conv.bias: \(5,\) vs \(4,\)"):
        Half().load_reference_state_dict({**sd, "enc.conv.bias": torch.zeros(5)})


def test_strict_loader_with_the_other_half_named():
    sd = state()

    def other(n):
        return n.startswith("dec.")
    m = Half()
    assert m.load_reference_state_dict({**sd, "vae.dec.conv.weight": torch.zeros(1)}, other) == ["vae.dec.conv.weight"]
    m = Half()
    with pytest.raises(ValueError, match="unexpected key in a reference state dict: loss.w"):
        m.load_reference_state_dict({**sd, "loss.w": torch.zeros(1)}, other)
    assert all(not t.any() for n, t in m.state_dict().items() if not n.endswith("running_var"))      # refused before anything was copied
    enc, dec = dfot_amd.TiTokEncoder(image_size=32, vit_enc_model_size="small"), dfot_amd.TiTokDecoder(image_size=32, vit_dec_model_size="small")
    both = {**{n: torch.zeros_like(t) for n, t in enc.state_dict().items()}, **{n: torch.zeros_like(t) for n, t in dec.state_dict().items()}}
    assert enc.load_reference_state_dict(both) == list(dec.state_dict()) and dec.load_reference_state_dict(both) == list(enc.state_dict())
    for half in (enc, dec):
        with pytest.raises(ValueError, match="unexpected key in a TiTok_KL state dict: vae.loss.w"):
            half.load_reference_state_dict({**both, "vae.loss.w": torch.zeros(1)})


def test_host_resident_weights_are_refused_before_any_packing():
    m = Half()
    with pytest.raises(RuntimeError, match=r"^parameter top is on cpu; move the module to the GPU first \(there is no CPU path\)$"):
        m._sync()
    with pytest.raises(RuntimeError, match=r"^encoder.conv_in.conv.weight is on cpu; move the module to the GPU first"):
        dfot_amd.DCAEEncoder(**dfot_amd.dcae_config("8x"))._sync()


# ------------------------------------------------------------------ the hierarchy
def test_every_codec_derives_from_the_shared_base_alone():
    bases = (vae._VideoVAEModule, image_vae._ImageVAEModule, titok._TiTokModule, dcae._DCAEModule)
    for b in bases:
        assert b.__bases__ == (cc.CodecModule,), b
    for cls in (dfot_amd.TiTokDecoder, dfot_amd.TiTokEncoder, dfot_amd.DCAEDecoder, dfot_amd.DCAEEncoder):
        assert not issubclass(cls, (vae._VideoVAEModule, image_vae._ImageVAEModule)), cls
        assert not hasattr(cls, "_attn") and not hasattr(cls, "load_diffusers_state_dict"), cls
    for cls in (dfot_amd.ImageVAEDecoder, dfot_amd.ImageVAEEncoder):
        assert callable(cls.load_diffusers_state_dict) and not issubclass(cls, vae._VideoVAEModule)
    assert not hasattr(dfot_amd.VideoVAEDecoder, "load_diffusers_state_dict")
    assert vae._VideoVAEModule._res is image_vae._ImageVAEModule._res is cc.gn_res_block      # the GroupNorm ResnetBlock, once
    assert dfot_amd.TiTokDecoder._res is not cc.gn_res_block                                  # its shortcut differs
