"""VideoVAE decoder and encoder on the MI355X engine: latents -> frames for the latent datasets (Kinetics-600), and frames -> latents
for the online latent path (``VideoVAEEncoder`` / ``encode_videos`` at the end of this file: ``BaseVideoAlgo._encode``).

Mirrors the reference's decode path for this model family:
  * ``BaseVideoAlgo._decode`` / ``_run_vae``   algorithms/common/base_pytorch_video_algo.py:553-629   (chunking by
    ``vae.batch_size``, ``decode(y, n_frames) * 0.5 + 0.5``, the ``b t c h w`` layout contract)
  * ``VideoVAE.decode`` / ``_decode``          algorithms/vae/video_vae/model.py:445-476  (post_quant_conv, Decoder, last
    ``desired_length`` frames)
  * ``Decoder.forward``                        algorithms/vae/video_vae/model.py:255-281
  * ``ResnetBlock3D``, ``AttnBlock3D``, ``PaddedConv3D``, ``SpatialUpsample2x``, ``Spatial2xTime2x3DUpsample``
                                               algorithms/vae/common/modules/{resnet,attention,conv,updownsample}.py
with the default (causal) module choice of ``VideoVAE.__init__`` -- what ``VideoVAE_K600.ckpt`` is built from (bash/k600/*.sh:17).
The module registers the reference's decoder state-dict names (``decoder.*``, ``post_quant_conv.conv.*``), so the ``vae.``-prefixed
keys of a reference checkpoint load with ``load_state_dict``.  Every value is computed by a HIP kernel behind the C ABI: the 3x3x3
causal convolutions are three implicit-GEMM 3x3 convolutions (frames t-2, t-1, t) accumulated in fp32, the 1x1x1 projections and the
per-frame attention products are MFMA GEMMs, GroupNorm / upsampling / softmax are the HBM-bound kernels of csrc/vae.hip.
Host code only sequences the calls (the decode runs once per generated video, after the 50-step sampler).  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import capi
from .codec_common import BF, _P, _S, CodecModule, channel_vector, chunks, gn_res_block, pack_1x1, pack_conv3x3, pack_conv_layers, pad_to, refuse_layout


class _VideoVAEModule(CodecModule):
    """What the VideoVAE encoder and decoder share on top of the codec base: the GroupNorm ResnetBlock and AttnBlock3D on channels-last
    [B][T][H][W][C] activations.  Subclasses list their parameters in ``_specs`` and provide ``_pack`` and ``_conv``."""

    _res = gn_res_block

    def _pack_weights(self, f: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        return pack_conv_layers(f, self._pack)

    def _attn(self, x: torch.Tensor, name: str, b: int) -> torch.Tensor:
        """AttnBlock3D: per frame, one head over the H*W positions with all C channels"""
        bb, t, h, w, c = x.shape
        n = h * w
        hn = self._gn(x, name + ".norm", False, b)
        q, k, v = (torch.empty(bb * t * n, c, dtype=BF, device=x.device) for _ in range(3))
        for dst, nm in ((q, "q"), (k, "k"), (v, "v")):
            capi.check(capi.lib.dfot_op_gemm_bf16(_P(hn), c, _P(self._packed[f"{name}.{nm}.conv.weight"]), _P(self._packed[f"{name}.{nm}.conv.bias"]),
                                                  _P(dst), c, bb * t * n, c, c, _S()))
        o = torch.empty(bb * t * n, c, dtype=BF, device=x.device)
        scores = torch.empty(n, n, device=x.device)
        probs = torch.empty(n, n, dtype=BF, device=x.device)
        vt = torch.empty(c, n, dtype=BF, device=x.device)
        for f in range(bb * t):
            qf, kf, vf, of = (a[f * n:(f + 1) * n] for a in (q, k, v, o))
            capi.check(capi.lib.dfot_op_gemm_f32(_P(qf), c, _P(kf), None, None, _P(scores), n, n, n, c, _S()))          # S = Q K^T
            capi.check(capi.lib.dfot_op_softmax_rows(_P(scores), _P(probs), n, n, float(c) ** -0.5, _S()))
            capi.check(capi.lib.dfot_op_transpose_bf16(_P(vf), _P(vt), n, c, _S()))                                       # V^T [C][N]
            capi.check(capi.lib.dfot_op_gemm_bf16(_P(probs), n, _P(vt), None, _P(of), c, n, c, n, _S()))                  # O = P V
        out = torch.empty_like(x)
        capi.check(capi.lib.dfot_op_gemm_f32(_P(o), c, _P(self._packed[f"{name}.proj_out.conv.weight"]), _P(self._packed[f"{name}.proj_out.conv.bias"]),
                                             _P(x), _P(out), c, bb * t * n, c, c, _S()))
        return out


class VideoVAEDecoder(_VideoVAEModule):
    def __init__(self, z_channels: int = 16, hidden_size: int = 128, hidden_size_mult: Sequence[int] = (1, 2, 4, 4), num_res_blocks: int = 2,
                 embed_dim: Optional[int] = None, use_quant_layer: bool = True,
                 spatial_upsample: Sequence[str] = ("", "SpatialUpsample2x", "Spatial2xTime2x3DUpsample", "Spatial2xTime2x3DUpsample"),
                 attn_resolutions: Sequence[int] = (), is_causal: bool = True):
        super().__init__()
        if not is_causal:
            raise NotImplementedError("only the causal VideoVAE (VideoVAE's default, the K600 checkpoint) is supported")
        if tuple(attn_resolutions):
            raise NotImplementedError("decoder attention inside the up levels (attn_resolutions) is not supported; the mid attention is")
        for u in spatial_upsample:
            if u not in ("", "SpatialUpsample2x", "Spatial2xTime2x3DUpsample"):
                raise NotImplementedError(f"unsupported decoder upsample '{u}'")
        self.z, self.hidden, self.mult, self.nres = int(z_channels), int(hidden_size), tuple(hidden_size_mult), int(num_res_blocks)
        self.embed = int(embed_dim if embed_dim is not None else z_channels)
        self.use_quant, self.up_kind = bool(use_quant_layer), tuple(spatial_upsample)
        self.levels = len(self.mult)
        chans = [self.hidden * m for m in self.mult]
        for c in chans:
            if c not in (128, 256, 512, 1024):
                raise ValueError(f"decoder width {c} not in {{128, 256, 512, 1024}} (GroupNorm / GEMM tiling of the engine)")
        self._specs: List[Tuple[str, Tuple[int, ...]]] = []

        def conv3(name, ci, co, k=(3, 3, 3)):
            self._specs += [(f"{name}.conv.weight", (co, ci, *k)), (f"{name}.conv.bias", (co,))]

        def norm(name, c):
            self._specs += [(f"{name}.weight", (c,)), (f"{name}.bias", (c,))]

        def res(name, ci, co):
            norm(f"{name}.norm1", ci)
            conv3(f"{name}.conv1", ci, co)
            norm(f"{name}.norm2", co)
            conv3(f"{name}.conv2", co, co)
            if ci != co:
                conv3(f"{name}.nin_shortcut", ci, co, (1, 1, 1))
        if self.use_quant:
            conv3("post_quant_conv", self.embed, self.z, (1, 1, 1))
        top = chans[-1]
        conv3("decoder.conv_in", self.z, top)
        res("decoder.mid.block_1", top, top)
        norm("decoder.mid.attn_1.norm", top)
        for n in ("q", "k", "v", "proj_out"):
            conv3(f"decoder.mid.attn_1.{n}", top, top, (1, 1, 1))
        res("decoder.mid.block_2", top, top)
        self.plan: List[Tuple[int, List[Tuple[str, int, int]], str]] = []
        cin = top
        for lvl in reversed(range(self.levels)):
            blocks = []
            for i in range(self.nres + 1):
                blocks.append((f"decoder.up.{lvl}.block.{i}", cin, chans[lvl]))
                cin = chans[lvl]
            self.plan.append((lvl, blocks, self.up_kind[lvl]))
        # registration order of the reference: up modules are inserted at the front, so up.0 comes first in the state dict
        for lvl, blocks, kind in sorted(self.plan, key=lambda e: e[0]):
            for name, ci, co in blocks:
                res(name, ci, co)
            # both upsample modules hold a PaddedConv3D named `conv`, whose nn.Conv3d is `conv` again: ...upsample.conv.conv.weight
            if kind == "SpatialUpsample2x":
                conv3(f"decoder.up.{lvl}.upsample.conv", blocks[-1][2], blocks[-1][2], (1, 3, 3))
            elif kind == "Spatial2xTime2x3DUpsample":
                conv3(f"decoder.up.{lvl}.upsample.conv", blocks[-1][2], blocks[-1][2])
        norm("decoder.norm_out", chans[0])
        conv3("decoder.conv_out", chans[0], 3)
        self._register()

    # ------------------------------------------------------------------ weights -> bf16 GEMM operands
    def _pack(self, name: str, w: torch.Tensor) -> Tuple[torch.Tensor, int]:
        co, ci, kt, kh, kw = w.shape
        cip, cop = pad_to(ci, 64), pad_to(co, 8)
        if (kh, kw) == (1, 1):  # 1x1x1: a Linear [co][ci]
            return pack_1x1(w, cop, cip), cop
        # one packed [co][tap][ci] operand per temporal tap
        return torch.stack([pack_conv3x3(w[:, :, dt], cop, cip) for dt in range(kt)]), cop

    # ------------------------------------------------------------------ building blocks (channels-last [B][T][H][W][C])
    def _conv(self, x: torch.Tensor, name: str, resid: Optional[torch.Tensor] = None) -> torch.Tensor:
        """PaddedConv3D (causal, first-frame replication) on a bf16 [B][T][H][W][Ci] operand -> fp32 [B][T][H][W][Co] (+ resid)"""
        wp, bias = self._packed[name + ".conv.weight"], self._packed[name + ".conv.bias"]
        b, t, h, w, ci = x.shape
        if wp.ndim == 2:  # 1x1x1
            co = wp.shape[0]
            out = torch.empty(b, t, h, w, co, device=x.device)
            m = b * t * h * w
            capi.check(capi.lib.dfot_op_gemm_f32(_P(x), ci, _P(wp), _P(bias), _P(resid), _P(out), co, m, co, ci, _S()))
            return out
        kt, co = wp.shape[0], wp.shape[1]
        out = torch.empty(b, t, h, w, co, device=x.device)
        for dt in range(kt):
            shift = kt - 1 - dt
            xs = x
            if shift:
                xs = torch.empty_like(x)
                capi.check(capi.lib.dfot_op_frame_shift(_P(x), _P(xs), b, t, h * w * ci, shift, _S()))
            acc = resid if dt == 0 else out
            capi.check(capi.lib.dfot_op_conv3x3_f32(_P(xs), _P(wp[dt]), _P(bias) if dt == 0 else None, _P(acc), _P(out), b * t, h, w, ci, co, _S()))
        return out

    # ------------------------------------------------------------------ decode
    @torch.no_grad()
    def decode(self, z: torch.Tensor, desired_length: Optional[int] = None) -> torch.Tensor:
        """VideoVAE.decode: z (B, z_channels, T, H, W) -> (B, 3, T', 8H, 8W) with T' = 1 + 4 (T - 1) for the default module choice; the
        LAST ``desired_length`` frames are returned when given."""
        if z.ndim != 5 or z.shape[1] != (self.embed if self.use_quant else self.z):
            raise ValueError(f"z has shape {tuple(z.shape)}, expected (B, {self.embed if self.use_quant else self.z}, T, H, W)")
        self._sync()
        dev = next(self.parameters()).device
        capi.require_device(dev, z=z)
        b, cz, t, h, w = z.shape
        if (t * h * w) % 128:
            raise ValueError(f"T*H*W = {t * h * w} must be a multiple of 128 (GEMM row tiles)")
        cl = torch.zeros(b, t, h, w, pad_to(cz, 64), device=dev)
        cl[..., :cz] = z.detach().float().permute(0, 2, 3, 4, 1)
        x = self._bf(cl)
        if self.use_quant:
            y = self._conv(x, "post_quant_conv")                      # [.., pad8(z)] fp32
            cl = torch.zeros(b, t, h, w, pad_to(self.z, 64), device=dev)
            cl[..., : self.z] = y[..., : self.z]
            x = self._bf(cl)
        hcur = self._conv(x, "decoder.conv_in")
        top = self.hidden * self.mult[-1]
        hcur = self._res(hcur, "decoder.mid.block_1", top, top, b)
        hcur = self._attn(hcur, "decoder.mid.attn_1", b)
        hcur = self._res(hcur, "decoder.mid.block_2", top, top, b)
        for lvl, blocks, kind in self.plan:
            for name, ci, co in blocks:
                hcur = self._res(hcur, name, ci, co, b)
            if kind:
                bb, tt, hh, ww, cc = hcur.shape
                mode = 1 if kind == "Spatial2xTime2x3DUpsample" else 0
                t2 = 1 + 2 * (tt - 1) if mode == 1 else tt
                up = torch.empty(bb, t2, 2 * hh, 2 * ww, cc, device=dev)
                capi.check(capi.lib.dfot_op_upsample3d(_P(hcur), _P(up), bb, tt, hh, ww, cc, mode, _S()))
                hcur = self._conv(self._bf(up), f"decoder.up.{lvl}.upsample.conv")
        y = self._conv(self._gn(hcur, "decoder.norm_out", True, b), "decoder.conv_out")[..., :3]
        out = y.permute(0, 4, 1, 2, 3).contiguous()
        if desired_length is not None:
            out = out[:, :, -desired_length:]
            assert out.shape[2] == desired_length, f"Desired length {desired_length} does not match decoded length {out.shape[2]}"
        return out


@torch.no_grad()
def decode_latents(vae: VideoVAEDecoder, latents: torch.Tensor, n_frames: int, vae_batch_size: int = 2, shape: str = "b t c h w") -> torch.Tensor:
    """``BaseVideoAlgo._decode`` for a VideoVAE (base_pytorch_video_algo.py:553-629): latents in the sampler's ``b t c h w`` layout, chunks of
    ``vae.batch_size`` videos, ``decode(y, n_frames) * 0.5 + 0.5``, result back in ``b t c h w`` (frames in [0, 1])."""
    if shape != "b t c h w":
        raise ValueError("only the 'b t c h w' layout of the sampling path is supported")
    x = latents.permute(0, 2, 1, 3, 4)
    outs = [vae.decode(ch, n_frames) * 0.5 + 0.5 for ch in chunks(x, vae_batch_size)]
    return torch.cat(outs, 0).permute(0, 2, 1, 3, 4).contiguous()


_ENC_RESNETS = ("ResnetBlock2D", "ResnetBlock2D", "ResnetBlock3D", "ResnetBlock3D")
_ENC_DOWN = ("Downsample", "Spatial2xTime2x3DDownsample", "Spatial2xTime2x3DDownsample", "")


class VideoVAEPosterior:
    """``DiagonalGaussianDistribution`` of the encoder's moments (algorithms/vae/common/distribution.py): mean / logvar (clamped to
    [-30, 20]) / std in the reference's (B, C, T, H, W) layout (views of b t c h w tensors), ``parameters`` the raw moments."""

    def __init__(self, moments_cl: torch.Tensor, zc: int):
        self._mom = moments_cl                                   # fp32 [B][T][h][w][ld], mean | logvar in channels [0, 2 zc)
        b, t, h, w, ld = moments_cl.shape
        self._geo = (b, t, h, w, ld, zc)
        mean, logvar, std = (torch.empty(b, t, zc, h, w, device=moments_cl.device) for _ in range(3))
        capi.check(capi.lib.dfot_op_vae_posterior(_P(moments_cl), ld, None, None, None, _P(mean), _P(logvar), _P(std), None, b, t, h * w, zc, _S()))
        self.mean, self.logvar, self.std = (a.permute(0, 2, 1, 3, 4) for a in (mean, logvar, std))

    @property
    def parameters(self) -> torch.Tensor:
        zc = self._geo[-1]
        return self._mom[..., : 2 * zc].permute(0, 4, 1, 2, 3).contiguous()

    def mode(self) -> torch.Tensor:
        return self.mean

    def latents(self, eps_btchw: Optional[torch.Tensor] = None, data_mean: Optional[torch.Tensor] = None,
                data_std: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mean (+ std * eps), optionally normalised, as b t c h w: one posterior kernel"""
        b, t, h, w, ld, zc = self._geo
        z = torch.empty(b, t, zc, h, w, device=self._mom.device)
        capi.check(capi.lib.dfot_op_vae_posterior(_P(self._mom), ld, _P(eps_btchw), _P(data_mean), _P(data_std), None, None, None, _P(z), b, t, h * w,
                                                  zc, _S()))
        return z

    def sample(self, noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """mean + std * noise; noise (B, C, T, H, W) as the reference draws it (``torch.randn(mean.shape)``), from ``generator`` when not
        given (on the generator's device, then moved)"""
        if noise is None:
            noise = torch.randn(tuple(self.mean.shape), generator=generator, device=generator.device if generator is not None else self._mom.device)
        if tuple(noise.shape) != tuple(self.mean.shape):
            raise ValueError(f"noise has shape {tuple(noise.shape)}, expected {tuple(self.mean.shape)}")
        eps = noise.to(device=self._mom.device, dtype=torch.float32).permute(0, 2, 1, 3, 4).contiguous()
        return self.latents(eps).permute(0, 2, 1, 3, 4)


class VideoVAEEncoder(_VideoVAEModule):
    """VideoVAE encoder + quant_conv on the MI355X engine: frames -> latent posterior (``VideoVAE.encode``, video_vae/model.py:38-150,
    402-443), the first step of every K600 batch when latents are computed online (``BaseVideoAlgo._encode``).

    Registers the reference's ``encoder.*`` and ``quant_conv.*`` state-dict names.  conv_in runs on the stride-1 implicit-GEMM conv over a
    64-channel pixel operand (dfot_op_vae_pixels); every other convolution -- ResnetBlock2D (per frame), Downsample (2-D, stride 2),
    ResnetBlock3D / conv_out (3x3x3 causal) and Spatial2xTime2x3DDownsample (3x3x3, stride 2 in T, H, W) -- is ONE launch of the strided
    causal implicit-GEMM mode (dfot_op_conv3t_f32), temporal taps accumulated in registers, whose summation order depends on one video's
    shape only: a video encodes to the same latents whatever batch it is part of.  GroupNorm statistics follow the reference's
    scopes: per frame inside ResnetBlock2D (``@video_to_image``), per video over (T, H, W) everywhere else."""

    def __init__(self, hidden_size: int = 128, z_channels: int = 16, hidden_size_mult: Sequence[int] = (1, 2, 4, 4),
                 attn_resolutions: Sequence[int] = (), dropout: float = 0.0, resolution: int = 256, temporal_length: int = 17,
                 double_z: bool = True, embed_dim: Optional[int] = None, num_res_blocks: int = 2, q_conv: str = "PaddedConv3D",
                 encoder_conv_in: str = "Conv2d", encoder_conv_out: str = "PaddedConv3D", encoder_attention: str = "AttnBlock3D",
                 encoder_resnet_blocks: Sequence[str] = _ENC_RESNETS, encoder_spatial_downsample: Sequence[str] = _ENC_DOWN,
                 encoder_temporal_downsample: Sequence[str] = ("", "", "", ""), encoder_mid_resnet: str = "ResnetBlock3D",
                 use_quant_layer: bool = True, is_causal: bool = True):
        super().__init__()
        if not is_causal:
            raise NotImplementedError("only the causal VideoVAE (VideoVAE's default, the K600 checkpoint) is supported")
        if tuple(attn_resolutions):
            raise NotImplementedError("encoder attention inside the down levels (attn_resolutions) is not supported; the mid attention is")
        mult = tuple(hidden_size_mult)
        if len(encoder_resnet_blocks) != len(mult) or len(encoder_spatial_downsample) != len(mult):
            raise ValueError("encoder_resnet_blocks / encoder_spatial_downsample need one entry per level")
        choice = dict(q_conv=(q_conv, "PaddedConv3D"), encoder_conv_in=(encoder_conv_in, "Conv2d"), encoder_conv_out=(encoder_conv_out, "PaddedConv3D"),
                      encoder_attention=(encoder_attention, "AttnBlock3D"), encoder_mid_resnet=(encoder_mid_resnet, "ResnetBlock3D"))
        for arg, (got, want) in choice.items():
            if got != want:
                raise NotImplementedError(f"{arg}='{got}' is not supported (only '{want}', the VideoVAE default)")
        for r in encoder_resnet_blocks:
            if r not in ("ResnetBlock2D", "ResnetBlock3D"):
                raise NotImplementedError(f"unsupported encoder res block '{r}'")
        for d in encoder_spatial_downsample:
            if d not in ("", "Downsample", "Spatial2xTime2x3DDownsample"):
                raise NotImplementedError(f"unsupported encoder downsample '{d}'")
        if any(encoder_temporal_downsample):
            raise NotImplementedError("encoder_temporal_downsample modules are not supported")
        if encoder_spatial_downsample[-1]:
            # Encoder.forward feeds `h` (the last res block's output) to mid.block_1, not hs[-1]: equal only without a last-level downsample
            raise NotImplementedError("a downsample at the last encoder level is not supported (the reference then feeds mid.block_1 the "
                                      "pre-downsample activation)")
        self.hidden, self.mult, self.nres, self.z = int(hidden_size), mult, int(num_res_blocks), int(z_channels)
        self.embed = int(embed_dim if embed_dim is not None else z_channels)
        self.double_z, self.use_quant = bool(double_z), bool(use_quant_layer)
        self.res_kind, self.down_kind = tuple(encoder_resnet_blocks), tuple(encoder_spatial_downsample)
        self.t_factor = 2 ** sum("Time" in d for d in self.down_kind)
        self.s_factor = 2 ** sum(bool(d) for d in self.down_kind)
        self.temporal_length = int(temporal_length)
        if self.temporal_length % self.t_factor != 1 % self.t_factor:
            raise ValueError(f"temporal_length {temporal_length} must be {self.t_factor} * k + 1 (causal VideoVAE)")
        chans = [self.hidden * m for m in mult]
        for c in chans:
            if c not in (128, 256, 512, 1024):
                raise ValueError(f"encoder width {c} not in {{128, 256, 512, 1024}} (GroupNorm / GEMM tiling of the engine)")
        self.out_ch = 2 * self.z if self.double_z else self.z
        self.moment_ch = 2 * self.embed if self.use_quant else self.out_ch
        if self.moment_ch % 2:
            raise ValueError("the moments split into mean and logvar: an even channel count is needed")
        self._specs: List[Tuple[str, Tuple[int, ...]]] = []
        self._kind: Dict[str, Tuple[int, int, int]] = {}     # conv module -> (kt, spatial stride, time stride)

        def conv(name, ci, co, k, stride=1, three_d=True):
            kt = k[0] if three_d else 1
            self._kind[name] = (kt, stride, stride if three_d else 1)
            wname = f"{name}.conv.weight" if three_d else f"{name}.weight"
            self._specs.extend([(wname, (co, ci, *k)), (wname[:-6] + "bias", (co,))])

        def norm(name, c):
            self._specs.extend([(f"{name}.weight", (c,)), (f"{name}.bias", (c,))])

        def res(name, ci, co, three_d):
            norm(f"{name}.norm1", ci)
            conv(f"{name}.conv1", ci, co, (3, 3, 3) if three_d else (3, 3), three_d=three_d)
            norm(f"{name}.norm2", co)
            conv(f"{name}.conv2", co, co, (3, 3, 3) if three_d else (3, 3), three_d=three_d)
            if ci != co:
                conv(f"{name}.nin_shortcut", ci, co, (1, 1, 1) if three_d else (1, 1), three_d=three_d)

        conv("encoder.conv_in", 3, self.hidden, (3, 3), three_d=False)
        self.plan: List[Tuple[int, List[Tuple[str, int, int, bool]], str]] = []
        cin = self.hidden
        for lvl in range(len(mult)):
            three_d = self.res_kind[lvl] == "ResnetBlock3D"
            blocks = []
            for i in range(self.nres):
                blocks.append((f"encoder.down.{lvl}.block.{i}", cin, chans[lvl], three_d))
                res(f"encoder.down.{lvl}.block.{i}", cin, chans[lvl], three_d)
                cin = chans[lvl]
            kind = self.down_kind[lvl]
            if kind == "Downsample":        # nn.Conv2d named `conv`: ...downsample.conv.weight (4-D)
                conv(f"encoder.down.{lvl}.downsample.conv", cin, cin, (3, 3), stride=2, three_d=False)
            elif kind:                      # PaddedConv3D named `conv` holding an nn.Conv3d `conv`: ...downsample.conv.conv.weight (5-D)
                conv(f"encoder.down.{lvl}.downsample.conv", cin, cin, (3, 3, 3), stride=2)
            self.plan.append((lvl, blocks, kind))
        top = chans[-1]
        res("encoder.mid.block_1", top, top, True)
        norm("encoder.mid.attn_1.norm", top)
        for n in ("q", "k", "v", "proj_out"):
            conv(f"encoder.mid.attn_1.{n}", top, top, (1, 1, 1))
        res("encoder.mid.block_2", top, top, True)
        norm("encoder.norm_out", top)
        conv("encoder.conv_out", top, self.out_ch, (3, 3, 3))
        if self.use_quant:
            conv("quant_conv", self.out_ch, 2 * self.embed, (1, 1, 1))
        self._register()

    # ------------------------------------------------------------------ weights -> bf16 GEMM operands
    def _pack(self, name: str, w: torch.Tensor) -> Tuple[torch.Tensor, int]:
        """[co][ci](kt)(kh)(kw) fp32 -> bf16 [cop][kt * 9 * cip] (tap-major, temporal taps outermost: the K order of dfot_op_conv3t_f32) or
        [cop][cip] for 1x1(x1).  Output channels are padded to 64 too, so that the 32-channel conv_out result is quant_conv's K operand."""
        if w.ndim == 4:
            w = w.unsqueeze(2)
        co, ci, kt, kh, kw = w.shape
        cip, cop = pad_to(ci, 64), pad_to(co, 64)
        if (kh, kw) == (1, 1):
            return pack_1x1(w, cop, cip), cop
        return torch.cat([pack_conv3x3(w[:, :, dt], cop, cip) for dt in range(kt)], 1).contiguous(), cop

    def _conv(self, x: torch.Tensor, name: str, resid: Optional[torch.Tensor] = None) -> torch.Tensor:
        """one convolution of the encoder on a bf16 [B][T][H][W][Ci] operand -> fp32 [B][T'][H'][W'][Co] (+ resid)"""
        kt, s, st = self._kind[name]
        wkey = f"{name}.conv.weight" if f"{name}.conv.weight" in self._packed else f"{name}.weight"
        wp, bias = self._packed[wkey], self._packed[wkey[:-6] + "bias"]
        b, t, h, w, ci = x.shape
        co = wp.shape[0]
        if wp.shape[1] == ci:  # 1x1(x1)
            out = torch.empty(b, t, h, w, co, device=x.device)
            capi.check(capi.lib.dfot_op_gemm_f32(_P(x), ci, _P(wp), _P(bias), _P(resid), _P(out), co, b * t * h * w, co, ci, _S()))
            return out
        if name == "encoder.conv_in":  # 3x3 per frame over the 64-channel pixel operand: the engine's conv3x3 over B*T images
            out = torch.empty(b, t, h, w, co, device=x.device)
            capi.check(capi.lib.dfot_op_conv3x3_f32(_P(x), _P(wp), _P(bias), _P(resid), _P(out), b * t, h, w, ci, co, _S()))
            return out
        out = torch.empty(b, (t - 1) // st + 1, h // s, w // s, co, device=x.device)
        capi.check(capi.lib.dfot_op_conv3t_f32(_P(x), _P(wp), _P(bias), _P(resid), _P(out), b, t, h, w, ci, co, kt, s, st, _S()))
        return out

    # ------------------------------------------------------------------ encode
    def gemm_rows(self, b: int, t: int, h: int, w: int) -> List[Tuple[str, int]]:
        """(what, M) of every GEMM / implicit-GEMM launch for a (b, 3, t, h, w) input: each M must fill whole 128-row tiles"""
        rows = [("conv_in", b * t * h * w)]
        for lvl, _, kind in self.plan:
            rows.append((f"level {lvl} res blocks at {t}x{h}x{w}", b * t * h * w))
            if kind:
                if "Time" in kind:
                    t = (t - 1) // 2 + 1
                h, w = h // 2, w // 2
                rows.append((f"level {lvl} downsample to {t}x{h}x{w}", b * t * h * w))
        rows.append((f"mid / conv_out at {t}x{h}x{w}", b * t * h * w))
        rows.append((f"mid attention over one {h}x{w} frame", h * w))
        return rows

    def check_input_shape(self, b: int, t: int, h: int, w: int) -> None:
        """ValueError unless b videos of t frames of h x w can be encoded: t = 4k + 1 <= temporal_length, h and w divisible by the
        spatial factor, and every GEMM of the plan (gemm_rows) made of whole 128-row tiles"""
        shape = (b, 3, t, h, w)
        if t > self.temporal_length or t % self.t_factor != 1 % self.t_factor:
            raise ValueError(f"input {shape}: {t} frames, the causal VideoVAE takes {self.t_factor} * k + 1 <= {self.temporal_length} frames")
        if h % self.s_factor or w % self.s_factor:
            raise ValueError(f"input {shape}: frames of {h}x{w} are not divisible by the encoder's spatial factor {self.s_factor}")
        for what, m in self.gemm_rows(b, t, h, w):
            if m % 128:
                raise ValueError(f"input {shape}: {what} has M = {m} GEMM rows, not a multiple of the 128-row tile")

    def _check(self, x: torch.Tensor, t_axis: int) -> None:
        if not x.is_cuda:
            raise ValueError(f"videos are on {x.device}: the encoder runs on the GPU only (there is no CPU path)")
        capi.require_device(next(self.parameters()).device, videos=x)
        self.check_input_shape(x.shape[0], x.shape[t_axis], x.shape[-2], x.shape[-1])

    def _moments(self, x: torch.Tensor, geo, scale: float, shift: float) -> torch.Tensor:
        """frames (geo = ((b, t, h, w), element strides of b, c, t, h, w), scale * x + shift) -> moments fp32 [B][T'][h'][w'][64]"""
        self._sync()
        (b, t, h, w), (sb, sc, st, sh, sw) = geo
        xp = torch.empty(b, t, h, w, 64, dtype=BF, device=x.device)
        capi.check(capi.lib.dfot_op_vae_pixels(C.c_void_p(x.data_ptr()), sb, sc, st, sh, sw, scale, shift, _P(xp), b, t, h, w, _S()))
        hcur = self._conv(xp, "encoder.conv_in")
        for lvl, blocks, kind in self.plan:
            for name, ci, co, three_d in blocks:
                hcur = self._res(hcur, name, ci, co, b if three_d else b * hcur.shape[1])
            if kind:
                hcur = self._conv(self._bf(hcur), f"encoder.down.{lvl}.downsample.conv")
        top = self.hidden * self.mult[-1]
        hcur = self._res(hcur, "encoder.mid.block_1", top, top, b)
        hcur = self._attn(hcur, "encoder.mid.attn_1", b)
        hcur = self._res(hcur, "encoder.mid.block_2", top, top, b)
        hcur = self._conv(self._gn(hcur, "encoder.norm_out", True, b), "encoder.conv_out")     # [.., 64]: channels >= out_ch are 0
        if self.use_quant:
            hcur = self._conv(self._bf(hcur), "quant_conv")
        return hcur

    def _frames(self, x: torch.Tensor, layout: str) -> Tuple[Tuple[int, int, int, int], Tuple[int, ...]]:
        """(b, t, h, w) and the element strides (b, c, t, h, w) of a float32 video tensor in `layout`"""
        if x.dtype != torch.float32:
            raise ValueError(f"videos must be float32, got {x.dtype}")
        if layout == "b c t h w":
            (b, c, t, h, w), (sb, sc, st, sh, sw) = x.shape, x.stride()
        else:
            (b, t, c, h, w), (sb, st, sc, sh, sw) = x.shape, x.stride()
        if c != 3:
            raise ValueError(f"videos have {c} channels, expected 3")
        return (b, t, h, w), (sb, sc, st, sh, sw)

    @torch.no_grad()
    def _encode(self, x: torch.Tensor) -> torch.Tensor:
        """VideoVAE._encode: x (B, 3, T, H, W) in [-1, 1] -> moments (B, 2 * embed_dim, 1 + (T - 1) / 4, H / 8, W / 8)"""
        return self.encode(x).parameters

    @torch.no_grad()
    def encode(self, x: torch.Tensor) -> VideoVAEPosterior:
        """VideoVAE.encode: x (B, 3, T, H, W) in [-1, 1], T = 4k + 1 <= temporal_length -> the posterior of the latents"""
        if x.ndim != 5:
            raise ValueError(f"videos have shape {tuple(x.shape)}, expected (B, 3, T, H, W)")
        self._check(x, 2)
        return VideoVAEPosterior(self._moments(x, self._frames(x, "b c t h w"), 1.0, 0.0), self.moment_ch // 2)


@torch.no_grad()
def encode_videos(vae: VideoVAEEncoder, videos: torch.Tensor, vae_batch_size: int = 2, shape: str = "b t c h w", sample: bool = True,
                  noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None, data_mean=None, data_std=None) -> torch.Tensor:
    """``BaseVideoAlgo._encode`` for a VideoVAE (base_pytorch_video_algo.py:553-596): frames in [0, 1] in the ``b t c h w`` layout, chunks of
    ``vae.batch_size`` videos, ``encode(2 y - 1).sample()`` (``.mode()`` with sample=False), latents back in ``b t c h w``; with data_mean /
    data_std also ``_normalize_x`` (:491-496), fused into the posterior kernel.  ``noise`` (b t c h w, like the output) replaces the draws;
    otherwise each chunk draws ``randn`` of its (b, c, t, h, w) latent shape from ``generator``, as the reference does per chunk."""
    refuse_layout(videos, shape, "videos", "(B, T, 3, H, W)", "training / sampling")
    vae._check(videos, 1)
    dev = videos.device
    zc = vae.moment_ch // 2
    dm, ds = channel_vector(data_mean, zc, dev, "data_mean"), channel_vector(data_std, zc, dev, "data_std")
    if (dm is None) != (ds is None):
        raise ValueError("data_mean and data_std go together")
    if noise is not None and noise.shape[0] != videos.shape[0]:
        raise ValueError(f"noise has {noise.shape[0]} videos, the input {videos.shape[0]}")
    outs, row = [], 0
    for ch in chunks(videos, vae_batch_size):
        post = VideoVAEPosterior(vae._moments(ch, vae._frames(ch, "b t c h w"), 2.0, -1.0), zc)
        eps = None
        if sample:
            if noise is not None:
                eps = noise[row:row + ch.shape[0]].to(device=dev, dtype=torch.float32).contiguous()
                if tuple(eps.shape[1:]) != (post.mean.shape[2], zc, *post.mean.shape[3:]):
                    raise ValueError(f"noise has shape {tuple(noise.shape)}, expected (B, {post.mean.shape[2]}, {zc}, {post.mean.shape[3]}, "
                                     f"{post.mean.shape[4]})")
            else:
                draw = torch.randn(tuple(post.mean.shape), generator=generator, device=generator.device if generator is not None else dev)
                eps = draw.to(dev).permute(0, 2, 1, 3, 4).contiguous()
        outs.append(post.latents(eps, dm, ds))
        row += ch.shape[0]
    return torch.cat(outs, 0)
