"""ImageVAE decoder and encoder on the MI355X engine: the per-frame Stable-Diffusion-style autoencoder whose latent space the DMLab /
Minecraft recipes run in (``BaseVideoAlgo`` picks ``VideoVAE if is_latent_video_vae else ImageVAE``).

Mirrors, for this model family:
  * ``ImageVAE.encode`` / ``decode``           algorithms/vae/image_vae/trainer.py:281-345  (Encoder + 1x1 quant_conv -> posterior;
    1x1 post_quant_conv + Decoder)
  * ``Encoder`` / ``Decoder``                  algorithms/vae/image_vae/model.py:18-245
  * ``ResnetBlock2D``, ``AttnBlock``, ``Upsample``, ``Downsample``   algorithms/vae/common/modules/{resnet,attention,updownsample}.py
  * ``BaseVideoAlgo._run_vae`` / ``_encode`` / ``_decode``   algorithms/common/base_pytorch_video_algo.py:553-629  (ImageVAE branch:
    ``b c t h w -> (b t) c h w``, chunks of ``vae.batch_size`` videos, ``encode(2 y - 1).sample()``, ``decode(z) * 0.5 + 0.5``)
The modules register the reference's state-dict names (``decoder.*`` / ``post_quant_conv.*``, ``encoder.*`` / ``quant_conv.*``).
The KL-f8 autoencoder of the taichikl recipes (``stabilityai/sd-vae-ft-ema``, a diffusers ``AutoencoderKL``, which ``_encode`` /
``_decode`` call the same way, :590-591,605-609) is this architecture under other key names: ``load_diffusers_state_dict`` /
``load_diffusers_checkpoint`` / ``diffusers_to_reference_keys`` / ``ddconfig_from_diffusers`` below.  The mid attention takes 64, 256 or a
multiple of 256 positions from 512 to 4096 per frame (8x8 ... 64x64 maps: 64x64 ... 512x512 frames at f8).

Every value is computed by a HIP kernel behind the C ABI; host code only sequences the calls.  No CPU fallback.  Activations are
channels-last [frames][H][W][C].  Stride-1 3x3 convolutions run on the strided implicit-GEMM entry with one temporal tap
(dfot_op_conv3t_f32, whose summation order depends on one frame's shape only), 1x1 projections on the MFMA GEMM, GroupNorm(32) (+ SiLU)
per frame on dfot_op_groupnorm; the mid attention, Downsample and Upsample are the kernels of csrc/image_vae.hip
(dfot_op_ivae_attention, dfot_op_conv3x3_s2_f32, dfot_op_upconv3x3_f32).  Nothing mixes frames, so a frame decodes / encodes to the same
bits whatever batch it is part of.

GEMM rows: every launch takes whole 128-row tiles, so ``frames * H * W`` at the coarsest level must be a multiple of 128.  Inputs that
do not fill the tiles are REFUSED at call time (no internal padding): the ``ValueError`` states the next frame count that works.
"""
from __future__ import annotations

import math
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import torch

from . import capi
from .codec_common import (BF, _P, _S, CodecModule, channel_vector, conv3x3, flat_frames, gn_res_block, map_frame_chunks, pack_1x1, pack_conv3x3,
                           pack_conv_layers, pad_to, refuse_layout, upconv3x3)

_WIDTHS = (128, 256, 512, 1024)


def _attn_rows_ok(n: int) -> bool:
    """dfot_op_ivae_attention's rule on the positions per frame: the register-resident kernels at 64 and 256, the streaming one at a
    multiple of 256 in [512, 4096] (1024 = a 256x256 frame at f8, 4096 = a 512x512 one)"""
    return n in (64, 256) or (512 <= n <= 4096 and n % 256 == 0)


def _refuse(kind: str, attn_resolutions, use_linear_attn, attn_type, resamp_with_conv, tanh_out=False, give_pre_end=False) -> None:
    if tuple(attn_resolutions):
        raise NotImplementedError(f"{kind}: attn_resolutions={list(attn_resolutions)} (attention inside the up / down levels) is not "
                                  "supported; the mid attention is")
    if use_linear_attn:
        raise NotImplementedError(f"{kind}: use_linear_attn is not supported")
    if attn_type != "vanilla":
        raise NotImplementedError(f"{kind}: attn_type='{attn_type}' is not supported (only 'vanilla')")
    if tanh_out:
        raise NotImplementedError(f"{kind}: tanh_out is not supported")
    if give_pre_end:
        raise NotImplementedError(f"{kind}: give_pre_end is not supported")
    if not resamp_with_conv:
        raise NotImplementedError(f"{kind}: resamp_with_conv=False is not supported")


class _ImageVAEModule(CodecModule):
    """What the ImageVAE encoder and decoder share on top of the codec base: 2-D weight packing, the convolution dispatch, the GroupNorm
    ResnetBlock, the fused mid attention and the diffusers key map."""

    _res = gn_res_block

    def _pack_weights(self, f: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        return pack_conv_layers(f, self._pack)

    def _spec_conv(self, name: str, ci: int, co: int, k: int, kind: str = "s1") -> None:
        self._kind[name] = kind if k == 3 else "1x1"
        self._specs += [(f"{name}.weight", (co, ci, k, k)), (f"{name}.bias", (co,))]

    def _spec_norm(self, name: str, c: int) -> None:
        self._specs += [(f"{name}.weight", (c,)), (f"{name}.bias", (c,))]

    def _spec_res(self, name: str, ci: int, co: int) -> None:
        self._spec_norm(f"{name}.norm1", ci)
        self._spec_conv(f"{name}.conv1", ci, co, 3)
        self._spec_norm(f"{name}.norm2", co)
        self._spec_conv(f"{name}.conv2", co, co, 3)
        if ci != co:
            self._spec_conv(f"{name}.nin_shortcut", ci, co, 1)

    def _spec_mid(self, root: str, top: int) -> None:
        self._spec_res(f"{root}.mid.block_1", top, top)
        self._spec_norm(f"{root}.mid.attn_1.norm", top)
        for n in ("q", "k", "v", "proj_out"):
            self._spec_conv(f"{root}.mid.attn_1.{n}", top, top, 1)
        self._spec_res(f"{root}.mid.block_2", top, top)

    def _pack(self, name: str, w: torch.Tensor) -> Tuple[torch.Tensor, int]:
        """[co][ci][k][k] fp32 -> bf16 [cop][9 * cip] (tap-major, dfot_op_pack_conv3) or [cop][cip] for 1x1; both channel counts padded
        to 64, so that a narrow output (the latent) is the next layer's K operand as it stands"""
        co, ci, kh, kw = w.shape
        cip, cop = pad_to(ci, 64), pad_to(co, 64)
        return (pack_1x1 if (kh, kw) == (1, 1) else pack_conv3x3)(w, cop, cip), cop

    def _conv(self, x: torch.Tensor, name: str, resid: Optional[torch.Tensor] = None) -> torch.Tensor:
        """one convolution on a bf16 [F][H][W][Ci] operand -> fp32 [F][H'][W'][Co] (+ resid where the layer has one)"""
        wp, bias = self._packed[name + ".weight"], self._packed[name + ".bias"]
        f, h, w, ci = x.shape
        co, kind = wp.shape[0], self._kind[name]
        if kind == "1x1":
            out = torch.empty(f, h, w, co, device=x.device)
            capi.check(capi.lib.dfot_op_gemm_f32(_P(x), ci, _P(wp), _P(bias), _P(resid), _P(out), co, f * h * w, co, ci, _S()))
        elif kind == "s1":      # Conv2d(k 3, s 1, p 1) per frame: the strided entry with one temporal tap and stride 1
            out = conv3x3(x, wp, bias, resid)
        elif kind == "down":    # Downsample: pad (0, 1, 0, 1) + Conv2d(k 3, s 2)
            out = torch.empty(f, h // 2, w // 2, co, device=x.device)
            capi.check(capi.lib.dfot_op_conv3x3_s2_f32(_P(x), _P(wp), _P(bias), _P(out), f, h, w, ci, co, _S()))
        else:                   # Upsample: nearest 2x fused into the gather of Conv2d(k 3, s 1, p 1)
            out = upconv3x3(x, wp, bias)
        return out

    def _attn(self, x: torch.Tensor, name: str, b: int) -> torch.Tensor:
        """AttnBlock: per frame, one head over the H*W positions with all C channels; one fused launch for all frames"""
        f, h, w, c = x.shape
        n = h * w
        hn = self._gn(x, name + ".norm", False, f)
        q, k, v, o = (torch.empty(f * n, c, dtype=BF, device=x.device) for _ in range(4))
        for dst, nm in ((q, "q"), (k, "k"), (v, "v")):
            capi.check(capi.lib.dfot_op_gemm_bf16(_P(hn), c, _P(self._packed[f"{name}.{nm}.weight"]), _P(self._packed[f"{name}.{nm}.bias"]), _P(dst), c,
                                                  f * n, c, c, _S()))
        capi.check(capi.lib.dfot_op_ivae_attention(_P(q), _P(k), _P(v), _P(o), f, n, c, _S()))
        out = torch.empty_like(x)
        capi.check(capi.lib.dfot_op_gemm_f32(_P(o), c, _P(self._packed[f"{name}.proj_out.weight"]), _P(self._packed[f"{name}.proj_out.bias"]), _P(x),
                                             _P(out), c, f * n, c, c, _S()))
        return out

    def load_diffusers_state_dict(self, state_dict: Mapping[str, torch.Tensor]) -> List[str]:
        """a diffusers ``AutoencoderKL`` state dict (see ``diffusers_to_reference_keys``): renamed, then loaded as strictly as
        ``load_reference_state_dict`` loads; returns the ignored keys under their reference names (the other half of the autoencoder)"""
        return self.load_reference_state_dict(diffusers_to_reference_keys(state_dict, self.levels))

    def _check_rows(self, frames: int, h: int, w: int, what: str) -> None:
        """(h, w): the coarsest map (the mid blocks').  Every finer level has 4x the rows, so this one decides."""
        if not _attn_rows_ok(h * w):
            raise ValueError(f"{what}: the mid attention runs over {h}x{w} = {h * w} positions per frame; supported: 64, 256 and the "
                             "multiples of 256 from 512 to 4096")
        need = 128 // math.gcd(128, h * w)
        if frames % need:
            raise ValueError(f"{what}: {frames} frames of {h}x{w} at the coarsest level are {frames * h * w} GEMM rows, not whole 128-row tiles; "
                             f"{pad_to(frames, need)} frames would work (a multiple of {need})")


class ImageVAEDecoder(_ImageVAEModule):
    """``post_quant_conv`` + ``Decoder`` of the reference ImageVAE with its ``ddconfig`` keywords (model.py:128-245, trainer.py:340-343).
    Frames that do not fill whole 128-row GEMM tiles are refused at call time (see the module docstring)."""

    def __init__(self, ch: int = 128, out_ch: int = 3, ch_mult: Sequence[int] = (1, 2, 4, 4), num_res_blocks: int = 2, z_channels: int = 4,
                 embed_dim: int = 4, resolution: int = 256, attn_resolutions: Sequence[int] = (), dropout: float = 0.0,
                 resamp_with_conv: bool = True, in_channels: int = 3, double_z: bool = True, give_pre_end: bool = False, tanh_out: bool = False,
                 use_linear_attn: bool = False, attn_type: str = "vanilla"):
        super().__init__()
        _refuse("ImageVAEDecoder", attn_resolutions, use_linear_attn, attn_type, resamp_with_conv, tanh_out, give_pre_end)
        self.ch, self.out_ch, self.mult, self.nres = int(ch), int(out_ch), tuple(ch_mult), int(num_res_blocks)
        self.z, self.embed, self.resolution = int(z_channels), int(embed_dim), int(resolution)
        self.levels = len(self.mult)
        chans = [self.ch * m for m in self.mult]
        for c in chans:
            if c not in _WIDTHS:
                raise ValueError(f"decoder width {c} not in {set(_WIDTHS)} (GroupNorm / GEMM tiling of the engine)")
        if self.out_ch > 64 or self.z > 64 or self.embed > 64:
            raise ValueError("out_ch, z_channels and embed_dim up to 64 are supported (one K tile)")
        self._specs: List[Tuple[str, Tuple[int, ...]]] = []
        self._kind: Dict[str, str] = {}
        top = chans[-1]
        self._spec_conv("decoder.conv_in", self.z, top, 3)
        self._spec_mid("decoder", top)
        self.plan: List[Tuple[int, List[Tuple[str, int, int]]]] = []
        cin = top
        for lvl in reversed(range(self.levels)):
            blocks = []
            for i in range(self.nres + 1):
                blocks.append((f"decoder.up.{lvl}.block.{i}", cin, chans[lvl]))
                cin = chans[lvl]
            self.plan.append((lvl, blocks))
        for lvl, blocks in sorted(self.plan, key=lambda e: e[0]):   # the reference inserts up modules at the front: up.0 registers first
            for name, ci, co in blocks:
                self._spec_res(name, ci, co)
            if lvl != 0:
                self._spec_conv(f"decoder.up.{lvl}.upsample.conv", blocks[-1][2], blocks[-1][2], 3, "up")
        self._spec_norm("decoder.norm_out", chans[0])
        self._spec_conv("decoder.conv_out", chans[0], self.out_ch, 3)
        self._spec_conv("post_quant_conv", self.embed, self.z, 1)
        self._register()

    @torch.no_grad()
    def decode(self, z: torch.Tensor) -> torch.Tensor:
        """ImageVAE.decode: z (F, embed_dim, h, w) -> (F, out_ch, h * 2^(levels-1), w * 2^(levels-1))"""
        if z.ndim != 4 or z.shape[1] != self.embed:
            raise ValueError(f"z has shape {tuple(z.shape)}, expected (F, {self.embed}, h, w)")
        if not z.is_cuda:
            raise ValueError(f"latents are on {z.device}: the decoder runs on the GPU only (there is no CPU path)")
        dev = next(self.parameters()).device
        capi.require_device(dev, z=z)
        f, cz, h, w = z.shape
        self._check_rows(f, h, w, f"latents {tuple(z.shape)}")
        self._sync()
        cl = torch.zeros(f, h, w, 64, device=dev)
        cl[..., :cz] = z.detach().float().permute(0, 2, 3, 1)
        y = self._conv(self._bf(cl), "post_quant_conv")            # [.., 64] fp32, channels >= z_channels are 0
        hcur = self._conv(self._bf(y), "decoder.conv_in")
        top = self.ch * self.mult[-1]
        hcur = self._res(hcur, "decoder.mid.block_1", top, top, f)
        hcur = self._attn(hcur, "decoder.mid.attn_1", f)
        hcur = self._res(hcur, "decoder.mid.block_2", top, top, f)
        for lvl, blocks in self.plan:
            for name, ci, co in blocks:
                hcur = self._res(hcur, name, ci, co, f)
            if lvl != 0:
                hcur = self._conv(self._bf(hcur), f"decoder.up.{lvl}.upsample.conv")
        y = self._conv(self._gn(hcur, "decoder.norm_out", True, f), "decoder.conv_out")[..., : self.out_ch]
        return y.permute(0, 3, 1, 2).contiguous()


class ImageVAEPosterior:
    """``DiagonalGaussianDistribution`` of the encoder's moments (algorithms/vae/common/distribution.py) for frames: mean / logvar
    (clamped to [-30, 20]) / std in the reference's (F, C, h, w) layout, ``parameters`` the raw moments."""

    def __init__(self, moments_cl: torch.Tensor, zc: int):
        self._mom = moments_cl                                   # fp32 [F][h][w][ld], mean | logvar in channels [0, 2 zc)
        f, h, w, ld = moments_cl.shape
        self._geo = (f, h, w, ld, zc)
        self.mean, self.logvar, self.std = (torch.empty(f, zc, h, w, device=moments_cl.device) for _ in range(3))
        capi.check(capi.lib.dfot_op_vae_posterior(_P(moments_cl), ld, None, None, None, _P(self.mean), _P(self.logvar), _P(self.std), None, f, 1,
                                                  h * w, zc, _S()))

    @property
    def parameters(self) -> torch.Tensor:
        return self._mom[..., : 2 * self._geo[-1]].permute(0, 3, 1, 2).contiguous()

    def mode(self) -> torch.Tensor:
        return self.mean

    def latents(self, eps: Optional[torch.Tensor] = None, data_mean: Optional[torch.Tensor] = None,
                data_std: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mean (+ std * eps), optionally normalised, as (F, C, h, w): one posterior kernel"""
        f, h, w, ld, zc = self._geo
        z = torch.empty(f, zc, h, w, device=self._mom.device)
        capi.check(capi.lib.dfot_op_vae_posterior(_P(self._mom), ld, _P(eps), _P(data_mean), _P(data_std), None, None, None, _P(z), f, 1, h * w, zc,
                                                  _S()))
        return z

    def sample(self, noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """mean + std * noise; noise (F, C, h, w) as the reference draws it (``torch.randn(mean.shape)``), from ``generator`` when not given"""
        if noise is None:
            noise = torch.randn(tuple(self.mean.shape), generator=generator, device=generator.device if generator is not None else self._mom.device)
        if tuple(noise.shape) != tuple(self.mean.shape):
            raise ValueError(f"noise has shape {tuple(noise.shape)}, expected {tuple(self.mean.shape)}")
        return self.latents(noise.to(device=self._mom.device, dtype=torch.float32).contiguous())


class ImageVAEEncoder(_ImageVAEModule):
    """``Encoder`` + ``quant_conv`` of the reference ImageVAE with its ``ddconfig`` keywords (model.py:18-125, trainer.py:334-338).
    Frames that do not fill whole 128-row GEMM tiles are refused at call time (see the module docstring)."""

    def __init__(self, ch: int = 128, out_ch: int = 3, ch_mult: Sequence[int] = (1, 2, 4, 4), num_res_blocks: int = 2, z_channels: int = 4,
                 embed_dim: int = 4, resolution: int = 256, attn_resolutions: Sequence[int] = (), dropout: float = 0.0,
                 resamp_with_conv: bool = True, in_channels: int = 3, double_z: bool = True, give_pre_end: bool = False, tanh_out: bool = False,
                 use_linear_attn: bool = False, attn_type: str = "vanilla"):
        super().__init__()
        _refuse("ImageVAEEncoder", attn_resolutions, use_linear_attn, attn_type, resamp_with_conv)
        if in_channels != 3:
            raise NotImplementedError(f"ImageVAEEncoder: in_channels={in_channels} is not supported (RGB frames only)")
        if not double_z:
            raise NotImplementedError("ImageVAEEncoder: double_z=False is not supported (the posterior needs mean and logvar)")
        self.ch, self.mult, self.nres = int(ch), tuple(ch_mult), int(num_res_blocks)
        self.z, self.embed, self.resolution = int(z_channels), int(embed_dim), int(resolution)
        self.levels = len(self.mult)
        self.s_factor = 2 ** (self.levels - 1)
        chans = [self.ch * m for m in self.mult]
        for c in chans:
            if c not in _WIDTHS:
                raise ValueError(f"encoder width {c} not in {set(_WIDTHS)} (GroupNorm / GEMM tiling of the engine)")
        if 2 * self.z > 64 or 2 * self.embed > 64:
            raise ValueError("z_channels and embed_dim up to 32 are supported (the moments fit one K tile)")
        self._specs: List[Tuple[str, Tuple[int, ...]]] = []
        self._kind: Dict[str, str] = {}
        self._spec_conv("encoder.conv_in", 3, self.ch, 3)
        self.plan: List[Tuple[int, List[Tuple[str, int, int]]]] = []
        cin = self.ch
        for lvl in range(self.levels):
            blocks = []
            for i in range(self.nres):
                blocks.append((f"encoder.down.{lvl}.block.{i}", cin, chans[lvl]))
                self._spec_res(f"encoder.down.{lvl}.block.{i}", cin, chans[lvl])
                cin = chans[lvl]
            if lvl != self.levels - 1:
                self._spec_conv(f"encoder.down.{lvl}.downsample.conv", cin, cin, 3, "down")
            self.plan.append((lvl, blocks))
        self._spec_mid("encoder", chans[-1])
        self._spec_norm("encoder.norm_out", chans[-1])
        self._spec_conv("encoder.conv_out", chans[-1], 2 * self.z, 3)
        self._spec_conv("quant_conv", 2 * self.z, 2 * self.embed, 1)
        self._register()

    def _check(self, x: torch.Tensor) -> None:
        if x.dtype != torch.float32:
            raise ValueError(f"frames must be float32, got {x.dtype}")
        if not x.is_cuda:
            raise ValueError(f"frames are on {x.device}: the encoder runs on the GPU only (there is no CPU path)")
        capi.require_device(next(self.parameters()).device, frames=x)
        h, w = x.shape[-2:]
        if x.shape[-3] != 3:
            raise ValueError(f"frames have {x.shape[-3]} channels, expected 3")
        if h % self.s_factor or w % self.s_factor:
            raise ValueError(f"frames of {h}x{w} are not divisible by the encoder's spatial factor {self.s_factor}")
        self._check_rows(x.numel() // (3 * h * w), h // self.s_factor, w // self.s_factor, f"frames {tuple(x.shape)}")

    def _moments(self, x: torch.Tensor, b: int, t: int, strides: Tuple[int, ...], scale: float, shift: float) -> torch.Tensor:
        """frames (b x t of them, element strides (b, c, t, h, w)), scale * x + shift -> moments fp32 [b * t][h'][w'][64]"""
        self._sync()
        h, w = x.shape[-2:]
        sb, sc, st, sh, sw = strides
        xp = torch.empty(b * t, h, w, 64, dtype=BF, device=x.device)
        capi.check(capi.lib.dfot_op_vae_pixels(capi.C.c_void_p(x.data_ptr()), sb, sc, st, sh, sw, scale, shift,
                                               _P(xp), b, t, h, w, _S()))
        f = b * t
        hcur = self._conv(xp, "encoder.conv_in")
        for lvl, blocks in self.plan:
            for name, ci, co in blocks:
                hcur = self._res(hcur, name, ci, co, f)
            if lvl != self.levels - 1:
                hcur = self._conv(self._bf(hcur), f"encoder.down.{lvl}.downsample.conv")
        top = self.ch * self.mult[-1]
        hcur = self._res(hcur, "encoder.mid.block_1", top, top, f)
        hcur = self._attn(hcur, "encoder.mid.attn_1", f)
        hcur = self._res(hcur, "encoder.mid.block_2", top, top, f)
        hcur = self._conv(self._gn(hcur, "encoder.norm_out", True, f), "encoder.conv_out")    # [.., 64]: channels >= 2 z are 0
        return self._conv(self._bf(hcur), "quant_conv")

    @torch.no_grad()
    def encode(self, x: torch.Tensor) -> ImageVAEPosterior:
        """ImageVAE.encode: x (F, 3, H, W) in [-1, 1] -> the posterior of the latents (F, embed_dim, H / 2^(levels-1), W / 2^(levels-1))"""
        if x.ndim != 4:
            raise ValueError(f"frames have shape {tuple(x.shape)}, expected (F, 3, H, W)")
        self._check(x)
        sf, sc, sh, sw = x.stride()
        return ImageVAEPosterior(self._moments(x, x.shape[0], 1, (sf, sc, 0, sh, sw), 1.0, 0.0), self.embed)


# ---------------------------------------------------------------------------------------------------------------------------------
# diffusers-layout checkpoints (``AutoencoderKL``: stabilityai/sd-vae-ft-ema and the VAEs fine-tuned from it).  The map is stated from
# the format's public key layout; the library itself is not a dependency.
_DIFFUSERS_ATTN = {"to_q": "q", "to_k": "k", "to_v": "v", "to_out.0": "proj_out",          # current spelling (Linear projections)
                   "query": "q", "key": "k", "value": "v", "proj_attn": "proj_out",        # legacy hub checkpoints
                   "group_norm": "norm"}
_DIFFUSERS_RES = {"norm1": "norm1", "conv1": "conv1", "norm2": "norm2", "conv2": "conv2", "conv_shortcut": "nin_shortcut"}


def _diffusers_key(key: str, levels: int) -> Optional[str]:
    """one diffusers ``AutoencoderKL`` key -> the reference's (ldm) name, None when the key is not one of the format's"""
    stem, dot, leaf = key.rpartition(".")
    if not dot or leaf not in ("weight", "bias"):
        return None
    if stem in ("quant_conv", "post_quant_conv"):
        return key
    side, _, rest = stem.partition(".")
    if side not in ("encoder", "decoder"):
        return None
    if rest in ("conv_in", "conv_out"):
        return key
    if rest == "conv_norm_out":
        return f"{side}.norm_out.{leaf}"
    parts = rest.split(".")
    if parts[0] == "mid_block" and len(parts) >= 4:
        if parts[1] == "resnets" and parts[2] in ("0", "1") and len(parts) == 4 and parts[3] in _DIFFUSERS_RES and parts[3] != "conv_shortcut":
            return f"{side}.mid.block_{int(parts[2]) + 1}.{_DIFFUSERS_RES[parts[3]]}.{leaf}"
        if parts[1] == "attentions" and parts[2] == "0" and ".".join(parts[3:]) in _DIFFUSERS_ATTN:
            return f"{side}.mid.attn_1.{_DIFFUSERS_ATTN['.'.join(parts[3:])]}.{leaf}"
        return None
    blocks, ref = ("down_blocks", "down") if side == "encoder" else ("up_blocks", "up")
    if parts[0] != blocks or len(parts) != 5 or not parts[1].isdigit() or int(parts[1]) >= levels:
        return None
    lvl = int(parts[1]) if side == "encoder" else levels - 1 - int(parts[1])
    if parts[2] == "resnets" and parts[3].isdigit() and parts[4] in _DIFFUSERS_RES:
        return f"{side}.{ref}.{lvl}.block.{int(parts[3])}.{_DIFFUSERS_RES[parts[4]]}.{leaf}"
    if parts[2:] == (["downsamplers", "0", "conv"] if side == "encoder" else ["upsamplers", "0", "conv"]):
        return f"{side}.{ref}.{lvl}.{'downsample' if side == 'encoder' else 'upsample'}.conv.{leaf}"
    return None


def diffusers_to_reference_keys(state: Mapping[str, torch.Tensor], levels: int) -> Dict[str, torch.Tensor]:
    """A diffusers ``AutoencoderKL`` state dict under the reference's names (``levels = len(block_out_channels)``):
    ``down_blocks.{i}.resnets.{j}`` -> ``down.{i}.block.{j}``, ``up_blocks.{i}`` -> ``up.{levels - 1 - i}`` (diffusers counts the up
    blocks from the coarsest), ``mid_block.resnets.{0,1}`` -> ``mid.block_{1,2}``, ``mid_block.attentions.0`` -> ``mid.attn_1`` with
    ``to_q / to_k / to_v / to_out.0`` (or the legacy ``query / key / value / proj_attn``) -> ``q / k / v / proj_out``, ``conv_shortcut`` ->
    ``nin_shortcut``, ``conv_norm_out`` -> ``norm_out``, ``downsamplers.0`` / ``upsamplers.0`` -> ``downsample`` / ``upsample``.  The
    attention projections are Linear layers there: their [C, C] weights become the reference's 1x1 convolutions [C, C, 1, 1].
    A key that is not one of the format's raises ``ValueError`` naming it, as do two keys that map to one name."""
    out: Dict[str, torch.Tensor] = {}
    for key, t in state.items():
        name = _diffusers_key(key, int(levels))
        if name is None:
            raise ValueError(f"unknown key in a diffusers AutoencoderKL state dict with {levels} levels: {key}")
        if name in out:
            raise ValueError(f"two keys of the diffusers state dict map to {name}: {key} is the second")
        if ".mid.attn_1." in name and name.endswith(".weight") and not name.endswith(".norm.weight") and t.ndim == 2:
            t = t.reshape(*t.shape, 1, 1)
        out[name] = t
    return out


def ddconfig_from_diffusers(config: Mapping) -> Dict[str, object]:
    """The constructor keywords of ``ImageVAEDecoder`` / ``ImageVAEEncoder`` from a diffusers ``AutoencoderKL`` config (the mapping of its
    config.json).  Whatever the engine does not run is refused by the field's name."""
    def bad(field: str, why: str):
        return NotImplementedError(f"diffusers AutoencoderKL config: {field}={config.get(field)!r} is not supported ({why})")
    if "block_out_channels" not in config:
        raise ValueError("diffusers AutoencoderKL config: block_out_channels is missing")
    if config.get("norm_num_groups", 32) != 32:
        raise bad("norm_num_groups", "GroupNorm(32) only")
    if config.get("act_fn", "silu") != "silu":
        raise bad("act_fn", "SiLU only")
    boc = [int(c) for c in config["block_out_channels"]]
    if any(t != "DownEncoderBlock2D" for t in config.get("down_block_types", ["DownEncoderBlock2D"] * len(boc))):
        raise bad("down_block_types", "DownEncoderBlock2D only")
    if any(t != "UpDecoderBlock2D" for t in config.get("up_block_types", ["UpDecoderBlock2D"] * len(boc))):
        raise bad("up_block_types", "UpDecoderBlock2D only")
    for field in ("down_block_types", "up_block_types"):
        if field in config and len(config[field]) != len(boc):
            raise bad(field, f"one block type per entry of block_out_channels={boc}")
    for field in ("use_quant_conv", "use_post_quant_conv"):
        if not config.get(field, True):
            raise bad(field, "the 1x1 quant_conv / post_quant_conv are part of the engine's path")
    if not config.get("mid_block_add_attention", True):
        raise bad("mid_block_add_attention", "the mid block runs with its attention")
    ch = boc[0]
    if any(c % ch for c in boc):
        raise bad("block_out_channels", "every width must be a multiple of the first")
    zc = int(config.get("latent_channels", 4))
    return dict(ch=ch, ch_mult=[c // ch for c in boc], num_res_blocks=int(config.get("layers_per_block", 1)), z_channels=zc, embed_dim=zc,
                in_channels=int(config.get("in_channels", 3)), out_ch=int(config.get("out_channels", 3)),
                resolution=int(config.get("sample_size", 32)))


def load_diffusers_checkpoint(path: str, config: Optional[Mapping] = None) -> Tuple[Dict[str, object], Dict[str, torch.Tensor]]:
    """A diffusers-layout VAE from disk -> (constructor keywords, state dict under the reference's names).  ``path`` is a directory with
    ``config.json`` and one ``*.safetensors`` file (``diffusion_pytorch_model.safetensors`` if several), or one ``.safetensors`` file, whose
    ``config`` (the mapping of config.json) must then be given.

        dd, sd = load_diffusers_checkpoint("sd-vae-ft-ema")
        dec = ImageVAEDecoder(**dd).cuda(); dec.load_reference_state_dict(sd)"""
    import glob
    import json
    import os
    from safetensors.torch import load_file
    if os.path.isdir(path):
        if config is None:
            with open(os.path.join(path, "config.json")) as fh:
                config = json.load(fh)
        files = sorted(glob.glob(os.path.join(path, "*.safetensors")))
        if not files:
            raise FileNotFoundError(f"no *.safetensors file in {path}")
        if len(files) > 1:
            named = [f for f in files if os.path.basename(f) == "diffusion_pytorch_model.safetensors"]
            if len(named) != 1:
                raise ValueError(f"{path} holds {len(files)} *.safetensors files and no diffusion_pytorch_model.safetensors; name the file")
            files = named
        path = files[0]
    elif config is None:
        raise ValueError(f"{path} is a single file: its AutoencoderKL config (the mapping of config.json) must be given")
    dd = ddconfig_from_diffusers(config)
    return dd, diffusers_to_reference_keys(load_file(path), len(dd["ch_mult"]))


@torch.no_grad()
def decode_image_latents(vae: ImageVAEDecoder, latents: torch.Tensor, vae_batch_size: int = 2, shape: str = "b t c h w") -> torch.Tensor:
    """``BaseVideoAlgo._decode`` for an ImageVAE (base_pytorch_video_algo.py:553-629): latents in the sampler's ``b t c h w`` layout, chunks of
    ``vae.batch_size`` videos whose frames go to the batch (``(b t) c h w``), ``decode(y) * 0.5 + 0.5``, result back in ``b t c h w`` (frames
    in [0, 1]).  Frames are independent, so the chunking does not change a bit of the result."""
    return map_frame_chunks(lambda ch, row: vae.decode(flat_frames(ch)) * 0.5 + 0.5, latents, vae_batch_size, shape, "latents", "(B, T, C, h, w)")


@torch.no_grad()
def encode_image_frames(vae: ImageVAEEncoder, videos: torch.Tensor, vae_batch_size: int = 2, shape: str = "b t c h w", sample: bool = True,
                        noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None, data_mean=None,
                        data_std=None) -> torch.Tensor:
    """``BaseVideoAlgo._encode`` for an ImageVAE (base_pytorch_video_algo.py:553-596): frames in [0, 1] in the ``b t c h w`` layout, chunks of
    ``vae.batch_size`` videos whose frames go to the batch, ``encode(2 y - 1).sample()`` (``.mode()`` with sample=False), latents back in
    ``b t c h w``; with data_mean / data_std also ``_normalize_x`` (:491-496), fused into the posterior kernel.  ``noise`` (b t c h w, like
    the output) replaces the draws; otherwise each chunk draws ``randn`` of its ((b t), c, h, w) latent shape from ``generator``, as the
    reference does per chunk."""
    layout = (shape, "videos", "(B, T, 3, H, W)", "training / sampling")
    refuse_layout(videos, *layout)          # the layout refusals come before those of the other arguments
    dev, zc = videos.device, vae.embed
    dm, ds = channel_vector(data_mean, zc, dev, "data_mean"), channel_vector(data_std, zc, dev, "data_std")
    if (dm is None) != (ds is None):
        raise ValueError("data_mean and data_std go together")
    if noise is not None and noise.shape[0] != videos.shape[0]:
        raise ValueError(f"noise has {noise.shape[0]} videos, the input {videos.shape[0]}")

    def encode_chunk(ch: torch.Tensor, row: int) -> torch.Tensor:
        vae._check(ch)
        b, t = ch.shape[:2]
        sb, st, sc, sh, sw = ch.stride()
        post = ImageVAEPosterior(vae._moments(ch, b, t, (sb, sc, st, sh, sw), 2.0, -1.0), zc)
        lshape = (b, t, zc, *post.mean.shape[2:])
        eps = None
        if sample:
            if noise is not None:
                eps = noise[row:row + b].to(device=dev, dtype=torch.float32).contiguous()
                if tuple(eps.shape) != lshape:
                    raise ValueError(f"noise has shape {tuple(noise.shape)}, expected (B, {t}, {zc}, {lshape[3]}, {lshape[4]})")
            else:
                eps = torch.randn(tuple(post.mean.shape), generator=generator, device=generator.device if generator is not None else dev).to(dev)
        return post.latents(eps, dm, ds)
    return map_frame_chunks(encode_chunk, videos, vae_batch_size, *layout)
