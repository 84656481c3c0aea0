"""TiTok-KL on the MI355X engine: the 1-D token autoencoder whose latent space the taichi recipes run in
(``algorithm/vae=titok_kl_preprocessor``: 32 tokens of 4 channels per frame, latents ``[4, 1, 32]``).  Forward only; the decoder
(``TiTokDecoder``) and the encoder (``TiTokEncoder``) are two modules over the one checkpoint.

Mirrors:
  * ``TiTok_KL.encode``                         algorithms/vae/tiktok_kl/titok_kl.py:78-98  (encoder, ``DiagonalGaussianDistribution``;
    ``sample=True`` returns the mode)
  * ``TiTokEncoder``                            algorithms/vae/tiktok_kl/blocks_kl.py:95-166  (the same ViT over
    ``[cls | grid^2 patches | 32 latent tokens]``, ``ln_post`` of the latent rows, ``conv_out`` behind a ``reshape`` that reinterprets each
    frame's ``32 x C`` block as ``C x 32`` without permuting: dfot_op_titok_moments computes exactly that)
  * ``BaseVideoAlgo._encode``                   algorithms/common/base_pytorch_video_algo.py:553-596  (TiTok branch :592-593)
  * ``TiTok_KL.decode``                         algorithms/vae/tiktok_kl/titok_kl.py:100-109  (F.normalize, decoder, channel softmax,
    ``pixel_quantize_conv``, ``pixel_decoder``)
  * ``TiTokDecoder`` / ``ResidualAttentionBlock``   algorithms/vae/tiktok_kl/blocks_kl.py:39-88, 169-245  (a ViT over
    ``[cls | grid^2 mask tokens | 32 latent tokens]``: 289 tokens for a 256x256 frame)
  * ``Decoder`` / ``ResnetBlock`` / ``UpsamplingBlock``   algorithms/vae/tiktok_kl/maskgit_vqgan.py:53-90, 122-154, 197-245
  * ``BaseVideoAlgo._run_vae`` / ``_decode``    algorithms/common/base_pytorch_video_algo.py:553-629  (TiTok branch :611-617: chunks of
    ``vae.batch_size`` videos, ``decode(y)`` returned as it is)
The module registers the reference's state-dict names (``decoder.*``, ``pixel_quantize_conv.*``, ``pixel_decoder.*``); the encoder's keys
(``encoder.*``, ``latent_tokens``) are ignored on load and returned.

Every value is computed by a HIP kernel behind the C ABI; host code only sequences the calls.  No CPU fallback.  The token assembly,
LayerNorm, the ragged multi-head attention and bias + GELU / tanh are the kernels of csrc/titok.hip (the attention applies the
``log2(e) / 8`` scale itself; the packed ``in_proj`` rows are left as the checkpoint has them); every Linear and 1x1 convolution is an MFMA
GEMM on bf16 operands with fp32 accumulation, the residual stream stays fp32.  The pixel decoder runs channels-last on the ops of the
ImageVAE (dfot_op_conv3t_f32 with one temporal tap, dfot_op_upconv3x3_f32, dfot_op_groupnorm).  Two quirks of its ``ResnetBlock`` are kept:
its convolutions and ``nin_shortcut`` have no bias (a null bias pointer), and with a channel change the block returns
``h + nin_shortcut(h)`` with h the conv2 output -- the block's input is dropped (a GEMM whose residual is its own operand's fp32 source).

GEMM rows: ANY frame count >= 1 runs.  ``frames * 289`` token rows are no multiple of the 128-row GEMM tile, so the token buffers are
padded to whole tiles inside (and the pixel decoder's frame count to whole tiles of its coarsest map).  This differs from the ImageVAE,
which refuses such inputs.  Pad rows are zero-initialised, each GEMM row depends on its own operand row only, and the attention and the
gathering ``ln_post`` never load a row their sequence does not own: a pad row cannot reach a real row's result.  Nothing mixes frames and
every summation order is decided from one frame's shape, so a frame decodes to the same bits whatever batch it is part of.
"""
from __future__ import annotations

import math
from typing import Dict, List, Mapping, Optional, Tuple

import torch

from . import capi
from .codec_common import BF, _P, _S, CodecModule, conv3x3, flat_frames, gemm, map_frame_chunks, pack_1x1, pack_conv3x3, pad_to, upconv3x3
from .image_vae import ImageVAEPosterior

PRESETS = {"small": (512, 8, 8), "base": (768, 12, 12), "large": (1024, 24, 16)}     # width, layers, heads (head dim 64)
_PIXEL_UP = ((4, 512, 512), (3, 512, 256), (2, 256, 256), (1, 256, 128), (0, 128, 128))  # (block index, in, out) in run order
_ACT_GELU, _ACT_TANH = 0, 1             # dfot_op_bias_act_bf16


def max_sequence_length() -> int:
    """L_max of dfot_op_mha_packed"""
    return int(capi.lib.dfot_op_mha_packed_max_len())


class _TiTokModule(CodecModule):
    """What the two ViT halves of ``TiTok_KL`` share on top of the codec base: the LayerNorm / bias + activation calls and the loop over
    the ``ResidualAttentionBlock``s.  Subclasses set ``width``, ``layers``, ``heads`` and ``seq`` and pack their matrices in
    ``_pack_weights``.  Every GEMM's K split is decided from ONE frame's padded rows (``codec_common.splits_k``)."""

    _reference_model = "TiTok_KL"

    def _ln(self, x: torch.Tensor, name: str, rows: int, gather: Tuple[int, int, int] = (0, 0, 0), out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """LayerNorm(eps 1e-5) of the first `rows` rows -> bf16 GEMM operand (rows past `rows` of `out` stay as they are: zero)"""
        if out is None:
            out = torch.zeros(x.shape, dtype=BF, device=x.device)
        capi.check(capi.lib.dfot_op_layernorm(_P(x), _P(self._par(name + ".weight")), _P(self._par(name + ".bias")), 1e-5, _P(out), None, rows,
                                              self.width, *gather, _S()))
        return out

    def _bias_act(self, x: torch.Tensor, bias: torch.Tensor, act: int) -> torch.Tensor:
        out = torch.empty(x.shape, dtype=BF, device=x.device)
        capi.check(capi.lib.dfot_op_bias_act_bf16(_P(x), x.shape[1], _P(bias), _P(out), x.shape[0], x.shape[1], act, _S()))
        return out

    def _blocks(self, prefix: str, x: torch.Tensor, f: int) -> torch.Tensor:
        """``layers`` x ResidualAttentionBlock ``{prefix}.{i}`` on the fp32 residual stream x [pad128(f * seq)][width] (pad rows zero) of f
        sequences of ``seq`` rows back to back"""
        w, L = self.width, self.seq
        rows, rows1, mp, dev = f * L, L, x.shape[0], x.device
        p, pk = self._par, self._packed
        h = torch.zeros(mp, w, dtype=BF, device=dev)          # LayerNorm output: pad rows stay zero
        o = torch.zeros(mp, w, dtype=BF, device=dev)          # attention output: rows >= F * L are never written
        qkv = torch.empty(mp, 3 * w, dtype=BF, device=dev)
        for i in range(self.layers):
            r = f"{prefix}.{i}"
            self._ln(x, r + ".ln_1", rows, out=h)
            capi.check(capi.lib.dfot_op_gemm_bf16(_P(h), w, _P(pk[r + ".attn.in_proj_weight"]), _P(p(r + ".attn.in_proj_bias")), _P(qkv), 3 * w,
                                                  mp, 3 * w, w, _S()))
            capi.check(capi.lib.dfot_op_mha_packed(_P(qkv), 3 * w, _P(o), f, L, self.heads, _S()))
            x = gemm(o, pk[r + ".attn.out_proj.weight"], rows1, p(r + ".attn.out_proj.bias"), x)
            self._ln(x, r + ".ln_2", rows, out=h)
            u = gemm(h, pk[r + ".mlp.c_fc.weight"], rows1)
            x = gemm(self._bias_act(u, p(r + ".mlp.c_fc.bias"), _ACT_GELU), pk[r + ".mlp.c_proj.weight"], rows1, p(r + ".mlp.c_proj.bias"), x)
        return x


class TiTokDecoder(_TiTokModule):
    """The decoder half of the reference ``TiTok_KL`` with its constructor keywords; encoder-only keywords (``vit_enc_model_size``,
    ``vit_enc_patch_size``, ``use_checkpoint``, ...) are accepted and ignored.  Any frame count >= 1 decodes (see the module docstring)."""

    def __init__(self, image_size: int = 256, token_size: int = 4, use_l2_norm: bool = True, vit_dec_model_size: str = "large",
                 vit_dec_patch_size: int = 16, num_latent_tokens: int = 32, **encoder_only_keywords_ignored):
        super().__init__()
        if vit_dec_model_size not in PRESETS:
            raise ValueError(f"vit_dec_model_size='{vit_dec_model_size}' is not one of {sorted(PRESETS)}")
        if int(vit_dec_patch_size) != 16:
            raise NotImplementedError(f"vit_dec_patch_size={vit_dec_patch_size} is not supported: the pixel decoder upsamples by 16 (the reference "
                                      "hard-wires it)")
        if int(image_size) < 16 or int(image_size) % 16:
            raise ValueError(f"image_size={image_size} must be a positive multiple of 16")
        if not 1 <= int(token_size) <= 64:
            raise ValueError(f"token_size={token_size} must be in [1, 64]")
        if int(num_latent_tokens) < 1:
            raise ValueError(f"num_latent_tokens={num_latent_tokens} must be positive")
        self.image_size, self.token_size, self.l2norm = int(image_size), int(token_size), bool(use_l2_norm)
        self.size, self.nlat = vit_dec_model_size, int(num_latent_tokens)
        self.width, self.layers, self.heads = PRESETS[vit_dec_model_size]
        self.grid = self.image_size // 16
        self.seq = 1 + self.grid ** 2 + self.nlat
        if self.seq > max_sequence_length():
            raise ValueError(f"image_size={image_size} gives sequences of {self.seq} tokens; the attention kernel takes up to {max_sequence_length()}")
        w = self.width
        sp: List[Tuple[str, Tuple[int, ...]]] = [
            ("decoder.class_embedding", (1, w)), ("decoder.positional_embedding", (self.grid ** 2 + 1, w)), ("decoder.mask_token", (1, 1, w)),
            ("decoder.latent_token_positional_embedding", (self.nlat, w)),
            ("decoder.decoder_embed.weight", (w, self.token_size)), ("decoder.decoder_embed.bias", (w,)),
            ("decoder.ln_pre.weight", (w,)), ("decoder.ln_pre.bias", (w,))]
        for i in range(self.layers):
            r = f"decoder.transformer.{i}"
            sp += [(f"{r}.ln_1.weight", (w,)), (f"{r}.ln_1.bias", (w,)), (f"{r}.attn.in_proj_weight", (3 * w, w)), (f"{r}.attn.in_proj_bias", (3 * w,)),
                   (f"{r}.attn.out_proj.weight", (w, w)), (f"{r}.attn.out_proj.bias", (w,)), (f"{r}.ln_2.weight", (w,)), (f"{r}.ln_2.bias", (w,)),
                   (f"{r}.mlp.c_fc.weight", (4 * w, w)), (f"{r}.mlp.c_fc.bias", (4 * w,)), (f"{r}.mlp.c_proj.weight", (w, 4 * w)),
                   (f"{r}.mlp.c_proj.bias", (w,))]
        sp += [("decoder.ln_post.weight", (w,)), ("decoder.ln_post.bias", (w,)), ("decoder.ffn.0.weight", (2 * w, w, 1, 1)),
               ("decoder.ffn.0.bias", (2 * w,)), ("decoder.ffn.2.weight", (1024, 2 * w, 1, 1)), ("decoder.ffn.2.bias", (1024,)),
               ("pixel_quantize_conv.weight", (256, 1024, 1, 1)), ("pixel_quantize_conv.bias", (256,)),
               ("pixel_decoder.conv_in.weight", (512, 256, 3, 3)), ("pixel_decoder.conv_in.bias", (512,))]

        def res(name, ci, co):
            out = [(f"{name}.norm1.weight", (ci,)), (f"{name}.norm1.bias", (ci,)), (f"{name}.conv1.weight", (co, ci, 3, 3)),
                   (f"{name}.norm2.weight", (co,)), (f"{name}.norm2.bias", (co,)), (f"{name}.conv2.weight", (co, co, 3, 3))]
            return out + ([(f"{name}.nin_shortcut.weight", (co, co, 1, 1))] if ci != co else [])
        for i in range(2):
            sp += res(f"pixel_decoder.mid.{i}", 512, 512)
        for idx, ci, co in sorted(_PIXEL_UP):          # the reference registers up.0 first
            sp += res(f"pixel_decoder.up.{idx}.block.0", ci, co) + res(f"pixel_decoder.up.{idx}.block.1", co, co)
            if idx != 0:
                sp += [(f"pixel_decoder.up.{idx}.upsample_conv.weight", (co, co, 3, 3)), (f"pixel_decoder.up.{idx}.upsample_conv.bias", (co,))]
        sp += [("pixel_decoder.norm_out.weight", (128,)), ("pixel_decoder.norm_out.bias", (128,)),
               ("pixel_decoder.conv_out.weight", (3, 128, 3, 3)), ("pixel_decoder.conv_out.bias", (3,))]
        self._specs = sp
        self._register()

    # ------------------------------------------------------------------ weights -> bf16 GEMM operands
    def _pack_weights(self, f: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """every matrix weight (Linear [out][in], in_proj_weight, 1x1 and 3x3 convolutions) packed to its bf16 GEMM operand; biases, norm
        weights and the embeddings are read in fp32 as they stand"""
        pk: Dict[str, torch.Tensor] = {}
        for name, w in f.items():
            if name.endswith("weight") and w.ndim == 2 and name != "decoder.decoder_embed.weight":
                pk[name] = w.to(BF).contiguous()
            elif w.ndim == 4 and w.shape[2:] == (1, 1):
                pk[name] = pack_1x1(w, *w.shape[:2])
            elif w.ndim == 4:       # 3x3: output channels padded to 64, input channels as they are
                co, ci = w.shape[:2]
                pk[name] = pack_conv3x3(w, pad_to(co, 64), ci)
                if name[:-6] + "bias" in f:
                    b = torch.zeros(pad_to(co, 64), device=w.device)
                    b[:co] = f[name[:-6] + "bias"]
                    pk[name[:-6] + "bias"] = b
        return pk

    # ------------------------------------------------------------------ building blocks
    def _check(self, z: torch.Tensor) -> torch.device:
        if z.ndim != 4 or tuple(z.shape[1:]) != (self.token_size, 1, self.nlat):
            raise ValueError(f"z has shape {tuple(z.shape)}, expected (F, {self.token_size}, 1, {self.nlat})")
        if z.shape[0] < 1:
            raise ValueError("z holds no frame")
        if not z.is_cuda:
            raise ValueError(f"latents are on {z.device}: the decoder runs on the GPU only (there is no CPU path)")
        dev = next(self.parameters()).device
        capi.require_device(dev, z=z)
        return dev

    def _frames_padded(self, f: int) -> int:
        """frames the grid-shaped part runs on: whole 128-row tiles of the coarsest map"""
        return pad_to(f, 128 // math.gcd(128, self.grid ** 2))

    def _transformer(self, z: torch.Tensor) -> torch.Tensor:
        """steps 1-3 and the ffn: z (F, token_size, 1, nlat) -> logits fp32 [Fp * grid^2][1024], rows of frames >= F are padding"""
        dev = self._check(z)
        self._sync()
        f, w, L, g2 = z.shape[0], self.width, self.seq, self.grid ** 2
        mp = pad_to(f * L, 128)
        p = self._par
        x = torch.zeros(mp, w, device=dev)
        zf = z.detach().float().contiguous()                  # (a local: the op takes a raw pointer)
        capi.check(capi.lib.dfot_op_titok_tokens(
            _P(zf), _P(p("decoder.decoder_embed.weight")), _P(p("decoder.decoder_embed.bias")),
            _P(p("decoder.latent_token_positional_embedding")), _P(p("decoder.class_embedding")), _P(p("decoder.mask_token")),
            _P(p("decoder.positional_embedding")), _P(p("decoder.ln_pre.weight")), _P(p("decoder.ln_pre.bias")), 1e-5, _P(x), f, g2, self.nlat,
            self.token_size, w, int(self.l2norm), _S()))
        x = self._blocks("decoder.transformer", x, f)
        fp = self._frames_padded(f)
        y = torch.zeros(fp * g2, w, dtype=BF, device=dev)     # ln_post of rows 1 .. grid^2 of every sequence, compact
        self._ln(x, "decoder.ln_post", f * g2, gather=(L, 1, g2), out=y)
        u = gemm(y, self._packed["decoder.ffn.0.weight"], g2)
        return gemm(self._bias_act(u, p("decoder.ffn.0.bias"), _ACT_TANH), self._packed["decoder.ffn.2.weight"], g2, p("decoder.ffn.2.bias"))

    def _pixel_input(self, lg: torch.Tensor) -> torch.Tensor:
        """softmax over the 1024 channels + pixel_quantize_conv: fp32 [rows][1024] -> fp32 [rows][256]"""
        probs = torch.empty(lg.shape, dtype=BF, device=lg.device)
        capi.check(capi.lib.dfot_op_softmax_rows(_P(lg), _P(probs), lg.shape[0], 1024, 1.0, _S()))
        return gemm(probs, self._packed["pixel_quantize_conv.weight"], self.grid ** 2, self._par("pixel_quantize_conv.bias"))

    def _conv(self, x: torch.Tensor, name: str, resid: Optional[torch.Tensor] = None, up: bool = False) -> torch.Tensor:
        """Conv2dSame(k 3) = Conv2d(k 3, s 1, p 1) on a bf16 [F][H][W][Ci] operand -> fp32 [F][H'][W'][Co]; up: nearest 2x fused in front"""
        wp, bias = self._packed[name + ".weight"], self._packed.get(name + ".bias")
        return upconv3x3(x, wp, bias) if up else conv3x3(x, wp, bias, resid)

    def _res(self, x: torch.Tensor, name: str, ci: int, co: int, b: int) -> torch.Tensor:
        h = self._conv(self._gn(x, name + ".norm1", True, b), name + ".conv1")
        if ci == co:
            return self._conv(self._gn(h, name + ".norm2", True, b), name + ".conv2", resid=x)
        h = self._conv(self._gn(h, name + ".norm2", True, b), name + ".conv2")
        f, hh, ww, _ = h.shape                                # h + nin_shortcut(h): the block's input is dropped
        return gemm(self._bf(h).reshape(f * hh * ww, co), self._packed[name + ".nin_shortcut.weight"], hh * ww,
                    resid=h.reshape(f * hh * ww, co)).reshape(f, hh, ww, co)

    def _pixel_decoder(self, lat: torch.Tensor) -> torch.Tensor:
        """maskgit_vqgan.Decoder on fp32 channels-last [Fp][g][g][256] -> fp32 [Fp][16 g][16 g][64] (channels >= 3 are 0)"""
        f = lat.shape[0]
        h = self._conv(self._bf(lat), "pixel_decoder.conv_in")
        for i in range(2):
            h = self._res(h, f"pixel_decoder.mid.{i}", 512, 512, f)
        for idx, ci, co in _PIXEL_UP:
            h = self._res(h, f"pixel_decoder.up.{idx}.block.0", ci, co, f)
            h = self._res(h, f"pixel_decoder.up.{idx}.block.1", co, co, f)
            if idx != 0:
                h = self._conv(self._bf(h), f"pixel_decoder.up.{idx}.upsample_conv", up=True)
        return self._conv(self._gn(h, "pixel_decoder.norm_out", True, f), "pixel_decoder.conv_out")

    def _to_nchw(self, rows: torch.Tensor, f: int, c: int) -> torch.Tensor:
        g = self.grid
        return rows[: f * g * g, :c].reshape(f, g, g, c).permute(0, 3, 1, 2).contiguous()

    # ------------------------------------------------------------------ public entry points
    @torch.no_grad()
    def decode_logits(self, z: torch.Tensor) -> torch.Tensor:
        """``TiTokDecoder.forward``: z (F, token_size, 1, num_latent_tokens) -> logits (F, 1024, grid, grid)"""
        return self._to_nchw(self._transformer(z), z.shape[0], 1024)

    @torch.no_grad()
    def decode_pixel_input(self, z: torch.Tensor) -> torch.Tensor:
        """``pixel_quantize_conv(decoder(z).softmax(1))``: the pixel decoder's input (F, 256, grid, grid)"""
        return self._to_nchw(self._pixel_input(self._transformer(z)), z.shape[0], 256)

    @torch.no_grad()
    def decode_pixels(self, lat: torch.Tensor) -> torch.Tensor:
        """the pixel decoder alone: (F, 256, grid, grid) fp32 -> frames (F, 3, 16 grid, 16 grid)"""
        g = self.grid
        if lat.ndim != 4 or tuple(lat.shape[1:]) != (256, g, g):
            raise ValueError(f"the pixel decoder's input has shape {tuple(lat.shape)}, expected (F, 256, {g}, {g})")
        if not lat.is_cuda:
            raise ValueError(f"the pixel decoder's input is on {lat.device}: the decoder runs on the GPU only (there is no CPU path)")
        capi.require_device(next(self.parameters()).device, lat=lat)
        self._sync()
        f = lat.shape[0]
        cl = torch.zeros(self._frames_padded(f), g, g, 256, device=lat.device)
        cl[:f] = lat.detach().float().permute(0, 2, 3, 1)
        return self._pixel_decoder(cl)[:f, :, :, :3].permute(0, 3, 1, 2).contiguous()

    @torch.no_grad()
    def decode(self, z: torch.Tensor) -> torch.Tensor:
        """``TiTok_KL.decode``: z (F, token_size, 1, num_latent_tokens) -> frames (F, 3, image_size, image_size)"""
        f, g = z.shape[0], self.grid
        lat = self._pixel_input(self._transformer(z))
        return self._pixel_decoder(lat.reshape(-1, g, g, 256))[:f, :, :, :3].permute(0, 3, 1, 2).contiguous()

    def load_reference_state_dict(self, state_dict: Mapping[str, torch.Tensor]) -> List[str]:
        """keys of a reference ``TiTok_KL`` (optionally ``vae.``-prefixed): the decoder's own keys are loaded strictly (every one present,
        with its shape); the encoder's (``encoder.*``, ``latent_tokens``) are ignored and returned.  Any other key raises ``ValueError``."""
        return super().load_reference_state_dict(state_dict, lambda n: n.startswith("encoder.") or n == "latent_tokens")


class TiTokEncoder(_TiTokModule):
    """The encoder half of the reference ``TiTok_KL`` (``encoder.*`` and ``latent_tokens``) with its constructor keywords; decoder-only
    keywords (``use_l2_norm``, ``vit_dec_model_size``, ``vit_dec_patch_size``, ``use_checkpoint``, ...) are accepted and ignored.  Any frame
    count >= 1 encodes, and a frame encodes to the same bits whatever batch it is part of (see the module docstring)."""

    def __init__(self, image_size: int = 256, token_size: int = 4, vit_enc_model_size: str = "large", vit_enc_patch_size: int = 16,
                 num_latent_tokens: int = 32, **decoder_only_keywords_ignored):
        super().__init__()
        if vit_enc_model_size not in PRESETS:
            raise ValueError(f"vit_enc_model_size='{vit_enc_model_size}' is not one of {sorted(PRESETS)}")
        if int(vit_enc_patch_size) != 16:
            raise NotImplementedError(f"vit_enc_patch_size={vit_enc_patch_size} is not supported: the patch gather is written for 16 x 16 patches "
                                      "(the recipes' size)")
        if int(image_size) < 16 or int(image_size) % 16:
            raise ValueError(f"image_size={image_size} must be a positive multiple of 16")
        if not 1 <= int(token_size) <= 64:
            raise ValueError(f"token_size={token_size} must be in [1, 64]: the moments hold 2 * token_size <= 128 channels")
        if not 1 <= int(num_latent_tokens) <= 128:
            raise ValueError(f"num_latent_tokens={num_latent_tokens} must be in [1, 128]")
        self.image_size, self.token_size = int(image_size), int(token_size)
        self.size, self.nlat = vit_enc_model_size, int(num_latent_tokens)
        self.width, self.layers, self.heads = PRESETS[vit_enc_model_size]
        self.grid = self.image_size // 16
        self.seq = 1 + self.grid ** 2 + self.nlat
        if self.seq > max_sequence_length():
            raise ValueError(f"image_size={image_size} gives sequences of {self.seq} tokens; the attention kernel takes up to {max_sequence_length()}")
        w = self.width
        sp: List[Tuple[str, Tuple[int, ...]]] = [
            ("latent_tokens", (self.nlat, w)),                 # a parameter of TiTok_KL itself: first in its state dict
            ("encoder.class_embedding", (1, w)), ("encoder.positional_embedding", (self.grid ** 2 + 1, w)),
            ("encoder.latent_token_positional_embedding", (self.nlat, w)),
            ("encoder.patch_embed.weight", (w, 3, 16, 16)), ("encoder.patch_embed.bias", (w,)),
            ("encoder.ln_pre.weight", (w,)), ("encoder.ln_pre.bias", (w,))]
        for i in range(self.layers):
            r = f"encoder.transformer.{i}"
            sp += [(f"{r}.ln_1.weight", (w,)), (f"{r}.ln_1.bias", (w,)), (f"{r}.attn.in_proj_weight", (3 * w, w)), (f"{r}.attn.in_proj_bias", (3 * w,)),
                   (f"{r}.attn.out_proj.weight", (w, w)), (f"{r}.attn.out_proj.bias", (w,)), (f"{r}.ln_2.weight", (w,)), (f"{r}.ln_2.bias", (w,)),
                   (f"{r}.mlp.c_fc.weight", (4 * w, w)), (f"{r}.mlp.c_fc.bias", (4 * w,)), (f"{r}.mlp.c_proj.weight", (w, 4 * w)),
                   (f"{r}.mlp.c_proj.bias", (w,))]
        sp += [("encoder.ln_post.weight", (w,)), ("encoder.ln_post.bias", (w,)),
               ("encoder.conv_out.weight", (2 * self.token_size, w, 1, 1)), ("encoder.conv_out.bias", (2 * self.token_size,))]
        self._specs = sp
        self._register()

    def _pack_weights(self, f: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """the Linear weights and ``patch_embed.weight`` (flattened (C, 3 * 16 * 16): the column order dfot_op_titok_patch_rows writes) packed
        to bf16 GEMM operands; ``conv_out.weight``, biases, norm weights and the embeddings are read in fp32"""
        return {name: w.reshape(w.shape[0], -1).to(BF).contiguous() for name, w in f.items()
                if name == "encoder.patch_embed.weight" or (name.endswith("weight") and w.ndim == 2)}

    def _check(self, x: torch.Tensor) -> torch.device:
        s = self.image_size
        if x.ndim != 4 or tuple(x.shape[1:]) != (3, s, s):
            raise ValueError(f"x has shape {tuple(x.shape)}, expected (F, 3, {s}, {s})")
        if x.shape[0] < 1:
            raise ValueError("x holds no frame")
        if not x.is_cuda:
            raise ValueError(f"frames are on {x.device}: the encoder runs on the GPU only (there is no CPU path)")
        dev = next(self.parameters()).device
        capi.require_device(dev, x=x)
        return dev

    def _moments(self, x: torch.Tensor) -> torch.Tensor:
        """``TiTokEncoder.forward`` (blocks_kl.py:140-166): frames (F, 3, S, S) -> moments fp32 [F][num_latent][2 * token_size]"""
        dev = self._check(x)
        self._sync()
        f, w, L, g2, oc = x.shape[0], self.width, self.seq, self.grid ** 2, 2 * self.token_size
        p = self._par
        xf = x.detach().float().contiguous()                  # (a local: the op takes a raw pointer)
        a = torch.zeros(pad_to(f * g2, 128), 768, dtype=BF, device=dev)     # pad rows stay zero
        capi.check(capi.lib.dfot_op_titok_patch_rows(_P(xf), _P(a), f, self.image_size, _S()))
        patches = gemm(a, self._packed["encoder.patch_embed.weight"], g2, p("encoder.patch_embed.bias"))   # K = 768: never split
        tok = torch.zeros(pad_to(f * L, 128), w, device=dev)
        capi.check(capi.lib.dfot_op_titok_enc_tokens(
            _P(patches), w, _P(p("encoder.class_embedding")), _P(p("encoder.positional_embedding")), _P(p("latent_tokens")),
            _P(p("encoder.latent_token_positional_embedding")), _P(p("encoder.ln_pre.weight")), _P(p("encoder.ln_pre.bias")), 1e-5, _P(tok), f, g2,
            self.nlat, w, _S()))
        tok = self._blocks("encoder.transformer", tok, f)
        t = torch.empty(f * self.nlat, w, device=dev)         # ln_post of the last num_latent rows of every sequence, compact, fp32
        capi.check(capi.lib.dfot_op_layernorm(_P(tok), _P(p("encoder.ln_post.weight")), _P(p("encoder.ln_post.bias")), 1e-5, None, _P(t), f * self.nlat, w,
                                              L, 1 + g2, self.nlat, _S()))
        mom = torch.empty(f, self.nlat, oc, device=dev)
        capi.check(capi.lib.dfot_op_titok_moments(_P(t), _P(p("encoder.conv_out.weight")), _P(p("encoder.conv_out.bias")), _P(mom), oc, f, self.nlat, w,
                                                  oc, _S()))
        return mom

    # ------------------------------------------------------------------ public entry points
    @torch.no_grad()
    def encode_moments(self, x: torch.Tensor) -> torch.Tensor:
        """``TiTokEncoder.forward``: frames (F, 3, S, S) -> moments (F, 2 * token_size, 1, num_latent_tokens), mean | logvar (not clamped)"""
        return self._moments(x).permute(0, 2, 1).unsqueeze(2).contiguous()

    @torch.no_grad()
    def encode(self, x: torch.Tensor, sample: bool = False, sample_posterior: bool = False, noise: Optional[torch.Tensor] = None,
               generator: Optional[torch.Generator] = None):
        """``TiTok_KL.encode`` (titok_kl.py:78-98): the posterior of the frames (F, 3, S, S) (``mean`` / ``logvar`` / ``std`` of shape
        (F, token_size, 1, num_latent_tokens), ``parameters``, ``mode()``, ``sample(noise, generator)``); with ``sample`` its mode, or with
        ``sample_posterior`` too ``mean + std * noise`` (noise given, or drawn from ``generator``).  No L2 normalisation: ``decode`` does it."""
        post = ImageVAEPosterior(self._moments(x).unsqueeze(1), self.token_size)       # [F][1][num_latent][2 ts]: h = 1, w = num_latent
        if not sample:
            return post
        return post.sample(noise, generator) if sample_posterior else post.mode()

    def load_reference_state_dict(self, state_dict: Mapping[str, torch.Tensor]) -> List[str]:
        """keys of a reference ``TiTok_KL`` (optionally ``vae.``-prefixed): the encoder's own keys (``encoder.*``, ``latent_tokens``) are
        loaded strictly (every one present, with its shape); the decoder's (``decoder.*``, ``pixel_quantize_conv.*``, ``pixel_decoder.*``)
        are ignored and returned.  Any other key raises ``ValueError``."""
        return super().load_reference_state_dict(state_dict, lambda n: n.startswith(("decoder.", "pixel_quantize_conv.", "pixel_decoder.")))


def load_titok_checkpoint(path: str) -> Dict[str, torch.Tensor]:
    """The recipe's ``model.safetensors`` (a ``TiTok_KL`` state dict) from disk, for either half:

        vae = TiTokDecoder(image_size=256, token_size=4).cuda(); vae.load_reference_state_dict(load_titok_checkpoint("model.safetensors"))"""
    from safetensors.torch import load_file
    return load_file(path)


@torch.no_grad()
def decode_titok_latents(vae: TiTokDecoder, latents: torch.Tensor, vae_batch_size: int = 2, shape: str = "b t c h w") -> torch.Tensor:
    """``BaseVideoAlgo._decode`` for a TiTok_KL (base_pytorch_video_algo.py:553-629): latents in the sampler's ``b t c h w`` layout
    (``(B, T, 4, 1, 32)``), chunks of ``vae.batch_size`` videos whose frames go to the batch, ``decode(y)`` as it is (no rescaling, unlike the
    ImageVAE branch), result ``(B, T, 3, H, W)``.  Frames are independent, so the chunking does not change a bit of the result."""
    return map_frame_chunks(lambda ch, row: vae.decode(flat_frames(ch)), latents, vae_batch_size, shape, "latents", "(B, T, C, 1, tokens)")


@torch.no_grad()
def encode_titok_frames(vae: TiTokEncoder, videos: torch.Tensor, vae_batch_size: int = 2, shape: str = "b t c h w") -> torch.Tensor:
    """``BaseVideoAlgo._encode`` for a TiTok_KL (base_pytorch_video_algo.py:553-596, TiTok branch :592-593, and
    ``Titok_KLPreprocessor._encode_videos``, tiktok_kl/preprocessor.py:124-132): videos ``(B, T, 3, S, S)``, chunks of ``vae.batch_size``
    videos whose frames go to the batch, ``encode(y, sample=True)`` -- the posterior's mode -- as it is (no rescaling), result
    ``(B, T, token_size, 1, num_latent_tokens)``.  Frames are independent, so the chunking does not change a bit of the result."""
    return map_frame_chunks(lambda ch, row: vae.encode(flat_frames(ch), sample=True), videos, vae_batch_size, shape, "videos", "(B, T, 3, S, S)")
