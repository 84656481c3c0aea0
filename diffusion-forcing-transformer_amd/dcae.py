"""DC-AE encoder and decoder on the MI355X engine: the deep-compression autoencoder whose 32-channel 8x8 latents the dmlab / Minecraft
``@DiT/B`` recipes run in (``dc_ae_preprocessor``: 64^2 frames, x8; ``dc_ae_16x_preprocessor``: 128^2 frames, x16).

Mirrors, for this model family:
  * ``Encoder`` / ``Decoder`` / ``MyAutoencoderDC``   algorithms/vae/dc_ae/autoencoder_dc_model.py:286-466, 469-737
  * ``ResBlock``, ``EfficientViTBlock``, ``DCDownBlock2d``, ``DCUpBlock2d``, ``SanaMultiscaleLinearAttention``   :45-283
  * ``GLUMBConv``, ``RMSNorm``, ``SanaMultiscaleAttnProcessor2_0``   diffusers 0.32.2 (restated from knowledge of that release; the
    library is not a dependency and the restatement is not checked against it)
  * ``BaseVideoAlgo._load_vae`` / ``_encode`` / ``_decode``   algorithms/common/base_pytorch_video_algo.py:511-520, 588-604
    (the ``MyAutoencoderDC`` branch: ``encode(2 y - 1)``, ``decode(z) * 0.5 + 0.5``, no posterior, ``scaling_factor`` not applied)
The modules register the reference's state-dict names in its order (``encoder.*`` / ``decoder.*``, the BatchNorm buffers included).

Every value is computed by a HIP kernel behind the C ABI; host code only sequences the calls.  No CPU fallback, forward only.
Activations are channels-last [frames][H][W][C].  3x3 convolutions run on dfot_op_conv3t_f32 (one temporal tap), 1x1 convolutions and the
attention projections on the MFMA GEMM (to_q / to_k / to_v as ONE GEMM with the three weights stacked: its output is the reference's
[q | k | v] concatenation, whose 96-column groups are the heads), the rest on the kernels of csrc/dcae.hip: ReLU linear attention,
depthwise 3x3 + SiLU gate, pixel (un)shuffle with the channel-mean / channel-repeat shortcuts, channel RMSNorm.  The model runs in eval
mode (``_from_pretrained_custom``), so a ResBlock's BatchNorm is an affine map of its running statistics: it is folded into ``conv2``'s
weights and bias in fp32 before the bf16 rounding.  Nothing mixes frames: a frame has the same bits whatever batch it is part of.

GEMM rows: every launch takes whole 128-row tiles.  ``encode`` / ``decode`` take any frame count >= 1: the batch is padded inside with
zero frames up to whole tiles at the coarsest map, and the padding is dropped from the result.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import torch

from . import capi
from .codec_common import BF, _P, _S, CodecModule, conv3x3, flat_frames, gemm, map_frame_chunks, pack_conv3x3, pad_to

_ACTS = {"relu": 1, "silu": 2}       # dfot_op_dcae_act_bf16
_OTHER_KEYS = ("name", "defaults", "pretrained_path", "pretrained_kwargs", "precision", "latent_type", "max_encode_length", "logging",
               "batch_size")   # keys of the reference's yaml files that do not describe the model
MAX_POSITIONS = 4096     # dfot_op_dcae_linear_attention: N a multiple of 64 up to this

DCAE_CONFIGS = {
    # configurations/algorithm/dc_ae_preprocessor.yaml (dmlab) and dc_ae_16x_preprocessor.yaml (Minecraft)
    "8x": dict(channels=(128, 256, 512, 512), enc_layers=(0, 4, 8, 2), dec_layers=(0, 5, 10, 2)),
    "16x": dict(channels=(128, 256, 512, 512, 1024), enc_layers=(0, 4, 8, 2, 2), dec_layers=(0, 5, 10, 2, 2)),
}


def dcae_config(kind: str = "8x") -> Dict[str, object]:
    """The constructor keywords of the two stock autoencoders: "8x" (dmlab, 64^2 frames) and "16x" (Minecraft, 128^2 frames)"""
    if kind not in DCAE_CONFIGS:
        raise ValueError(f"unknown DC-AE configuration '{kind}' (known: {sorted(DCAE_CONFIGS)})")
    c = DCAE_CONFIGS[kind]
    n = len(c["channels"])
    types = ["ResBlock"] * 3 + ["EfficientViTBlock"] * (n - 3)
    return dict(in_channels=3, latent_channels=32, attention_head_dim=32, encoder_block_types=list(types), decoder_block_types=list(types),
                encoder_block_out_channels=list(c["channels"]), decoder_block_out_channels=list(c["channels"]),
                encoder_layers_per_block=list(c["enc_layers"]), decoder_layers_per_block=list(c["dec_layers"]),
                encoder_qkv_multiscales=[[] for _ in range(n)], decoder_qkv_multiscales=[[] for _ in range(n)],
                decoder_norm_types=["batch_norm"] * 3 + ["rms_norm"] * (n - 3), decoder_act_fns=["relu"] * 3 + ["silu"] * (n - 3),
                downsample_block_type="pixel_unshuffle", upsample_block_type="pixel_shuffle", scaling_factor=0.2889)


def _per_stage(v, n: int, what: str) -> Tuple:
    v = (v,) * n if isinstance(v, str) else tuple(v)
    if len(v) != n:
        raise ValueError(f"{what} has {len(v)} entries for {n} stages")
    return v


def _plan(kind: str, side: str, types, channels, layers, multiscales, norms, acts, head_dim: int, latent: int, in_channels: int):
    """validates one half's configuration (every refusal names its field, nothing touches the device) -> (channels, layers, types, norms, acts)"""
    ch = tuple(int(c) for c in channels)
    n = len(ch)
    if n < 2:
        raise ValueError(f"{kind}: {side}_block_out_channels needs at least 2 stages, got {list(ch)}")
    layers = tuple(int(v) for v in _per_stage(layers, n, f"{side}_layers_per_block"))
    types = _per_stage(types, n, f"{side}_block_types")
    norms, acts = _per_stage(norms, n, "decoder_norm_types"), _per_stage(acts, n, "decoder_act_fns")
    ms = tuple(multiscales)
    if len(ms) != n:
        raise ValueError(f"{side}_qkv_multiscales has {len(ms)} entries for {n} stages")
    if any(len(tuple(m)) for m in ms):
        raise NotImplementedError(f"{kind}: {side}_qkv_multiscales={[list(m) for m in ms]} is not supported (multiscale QKV projections; "
                                  "both stock configurations leave them empty)")
    if head_dim != 32:
        raise NotImplementedError(f"{kind}: attention_head_dim={head_dim} is not supported (the linear-attention kernel has head dimension 32)")
    if in_channels != 3:
        raise NotImplementedError(f"{kind}: in_channels={in_channels} is not supported (RGB frames only)")
    if latent != 32:
        raise NotImplementedError(f"{kind}: latent_channels={latent} is not supported (32, as in both stock configurations)")
    for i, t in enumerate(types):
        if t not in ("ResBlock", "EfficientViTBlock"):
            raise NotImplementedError(f"{kind}: {side}_block_types[{i}]='{t}' is not supported (ResBlock and EfficientViTBlock are)")
    for i, a in enumerate(acts):
        if a not in _ACTS:
            raise NotImplementedError(f"{kind}: decoder_act_fns[{i}]='{a}' is not supported (relu and silu are)")
    for i, nt in enumerate(norms):
        if nt not in ("rms_norm", "batch_norm"):
            raise NotImplementedError(f"{kind}: decoder_norm_types[{i}]='{nt}' is not supported (rms_norm and batch_norm are)")
        if nt == "batch_norm" and types[i] == "EfficientViTBlock" and layers[i] > 0:
            raise NotImplementedError(f"{kind}: decoder_norm_types[{i}]='batch_norm' on an EfficientViTBlock stage is not supported "
                                      "(rms_norm there, as in both stock configurations)")
    if layers[0] != 0:
        raise NotImplementedError(f"{kind}: {side}_layers_per_block[0]={layers[0]} is not supported (stage 0 is empty in both stock "
                                  "configurations: conv_in / conv_out are the resampling blocks)")
    if any(v <= 0 for v in layers[1:]):
        raise NotImplementedError(f"{kind}: {side}_layers_per_block={list(layers)}: every stage after the first needs at least one layer "
                                  "(a stage without layers has no resampling block either)")
    for i, c in enumerate(ch[1:], 1):
        if c % 64 or c > 1024:
            raise ValueError(f"{kind}: {side}_block_out_channels[{i}]={c} is not supported (a multiple of 64 up to 1024: GEMM K tiles, "
                             "the depthwise kernel's 256-channel slabs)")
    for i in range(1, n - 1):
        if (4 * ch[i]) % ch[i + 1]:
            raise ValueError(f"{kind}: {side}_block_out_channels {ch[i]} -> {ch[i + 1]}: the shortcut needs 4 * {ch[i]} to be a multiple of "
                             f"{ch[i + 1]} (the channel-group size / repeat count)")
    if ch[-1] % latent:
        raise ValueError(f"{kind}: {side}_block_out_channels[-1]={ch[-1]} is not a multiple of latent_channels={latent}")
    return ch, layers, types, norms, acts


class _DCAEModule(CodecModule):
    """What the DC-AE encoder and decoder share on top of the codec base (registration under the reference's names, BatchNorm buffers
    included; strict loading): the weight forms of this model and its blocks."""

    _tensor_noun = ""

    def _common(self, kind: str, cfg: Mapping) -> Mapping:
        cfg = dict(cfg)
        for k in _OTHER_KEYS:
            cfg.pop(k, None)
        if cfg.pop("use_fp16", False):
            raise NotImplementedError(f"{kind}: use_fp16 is not supported (fp32 weights, bf16 GEMM operands)")
        known = set(dcae_config("8x"))
        extra = sorted(set(cfg) - known)
        if extra:
            raise TypeError(f"{kind}: unknown configuration keys {extra}")
        full = dcae_config("8x")
        full.update(cfg)
        if full["downsample_block_type"] != "pixel_unshuffle":
            raise NotImplementedError(f"{kind}: downsample_block_type='{full['downsample_block_type']}' is not supported (only 'pixel_unshuffle')")
        if full["upsample_block_type"] != "pixel_shuffle":
            raise NotImplementedError(f"{kind}: upsample_block_type='{full['upsample_block_type']}' is not supported (only 'pixel_shuffle')")
        self.scaling_factor = float(full["scaling_factor"])
        self.latent = int(full["latent_channels"])
        self._specs: List[Tuple[str, Tuple[int, ...]]] = []
        self._bn: List[str] = []        # ResBlocks whose norm is a BatchNorm2d
        return full

    # ------------------------------------------------------------------ registration
    def _spec_conv(self, name: str, ci: int, co: int) -> None:
        self._specs += [(f"{name}.weight", (co, ci, 3, 3)), (f"{name}.bias", (co,))]

    def _spec_block(self, name: str, kind: str, c: int, norm: str) -> None:
        if kind == "ResBlock":
            self._spec_conv(f"{name}.conv1", c, c)
            self._specs += [(f"{name}.conv2.weight", (c, c, 3, 3)), (f"{name}.norm.weight", (c,)), (f"{name}.norm.bias", (c,))]
            if norm == "batch_norm":
                self._specs += [(f"{name}.norm.running_mean", (c,)), (f"{name}.norm.running_var", (c,)), (f"{name}.norm.num_batches_tracked", ())]
                self._bn.append(name)
            return
        self._specs += [(f"{name}.attn.to_{n}.weight", (c, c)) for n in ("q", "k", "v", "out")]
        self._specs += [(f"{name}.attn.norm_out.weight", (c,)), (f"{name}.attn.norm_out.bias", (c,))]
        self._specs += [(f"{name}.conv_out.conv_inverted.weight", (8 * c, c, 1, 1)), (f"{name}.conv_out.conv_inverted.bias", (8 * c,)),
                        (f"{name}.conv_out.conv_depth.weight", (8 * c, 1, 3, 3)), (f"{name}.conv_out.conv_depth.bias", (8 * c,)),
                        (f"{name}.conv_out.conv_point.weight", (c, 4 * c, 1, 1)),
                        (f"{name}.conv_out.norm.weight", (c,)), (f"{name}.conv_out.norm.bias", (c,))]

    # ------------------------------------------------------------------ weights -> GEMM / kernel operands
    @staticmethod
    def fold_batch_norm(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, mean: torch.Tensor, var: torch.Tensor,
                        eps: float = 1e-5) -> Tuple[torch.Tensor, torch.Tensor]:
        """eval-mode BatchNorm2d after a bias-free convolution w [co][ci][k][k]: (w', b') with bn(conv(x, w)) = conv(x, w') + b'"""
        s = gamma / torch.sqrt(var + eps)
        return w * s.reshape(-1, 1, 1, 1), beta - mean * s

    def _pack_weights(self, f: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        dev = next(iter(f.values())).device
        pk: Dict[str, torch.Tensor] = {}

        def conv(name: str, w: torch.Tensor, b: Optional[torch.Tensor]) -> None:
            cop = pad_to(w.shape[0], 64)            # both channel counts padded to 64: a narrow output is the next layer's K operand
            pk[name + ".weight"] = pack_conv3x3(w, cop, pad_to(w.shape[1], 64))
            bias = torch.zeros(cop, device=dev)
            if b is not None:
                bias[: b.shape[0]] = b
            pk[name + ".bias"] = bias

        for name in self._names:
            if not name.endswith(".weight") or f[name].ndim < 2:
                continue
            stem, w = name[:-7], f[name]
            if stem.endswith(".attn.to_q"):
                root = stem[:-5]
                pk[root + ".qkv"] = torch.cat([f[f"{root}.to_{n}.weight"] for n in "qkv"], 0).to(BF).contiguous()
            elif stem.endswith((".attn.to_k", ".attn.to_v")):
                continue
            elif stem.endswith(".attn.to_out"):
                pk[name] = w.to(BF).contiguous()
            elif stem.endswith(".conv_depth"):
                pk[name] = w.reshape(w.shape[0], 9).t().contiguous()          # fp32 [9][2 hc], tap-major
                pk[stem + ".bias"] = f[stem + ".bias"].contiguous()
            elif stem.endswith((".conv_inverted", ".conv_point")):
                pk[name] = w.reshape(w.shape[0], w.shape[1]).to(BF).contiguous()
                if stem + ".bias" in f:
                    pk[stem + ".bias"] = f[stem + ".bias"].contiguous()
            elif stem.endswith(".conv2"):
                blk = stem[:-6]
                if blk in self._bn:
                    conv(stem, *self.fold_batch_norm(w, f[blk + ".norm.weight"], f[blk + ".norm.bias"], f[blk + ".norm.running_mean"],
                                                      f[blk + ".norm.running_var"]))
                else:
                    conv(stem, w, None)
            else:
                conv(stem, w, f[stem + ".bias"])
        return pk

    # ------------------------------------------------------------------ building blocks (channels-last [F][H][W][C])
    def _conv3(self, xb: torch.Tensor, name: str, resid: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Conv2d(k 3, s 1, p 1) on a bf16 [F][H][W][Ci] operand -> fp32 [F][H][W][pad64(Co)] (+ resid)"""
        return conv3x3(xb, self._packed[name + ".weight"], self._packed[name + ".bias"], resid)

    def _rms(self, x: torch.Tensor, name: str, resid: Optional[torch.Tensor] = None, f32: bool = True, bf16: bool = False, relu: bool = False):
        """channel RMSNorm (weight, bias, eps 1e-5) (+ resid) (ReLU) -> (fp32 or None, bf16 or None)"""
        c = x.shape[-1]
        o32 = torch.empty_like(x) if f32 else None
        o16 = torch.empty(x.shape, dtype=BF, device=x.device) if bf16 else None
        capi.check(capi.lib.dfot_op_dcae_rmsnorm(_P(x), _P(self._par(name + ".weight")), _P(self._par(name + ".bias")), 1e-5, _P(resid), _P(o32),
                                                 _P(o16), int(relu), x.numel() // c, c, _S()))
        return o32, o16

    def _res_block(self, h: torch.Tensor, name: str, norm: str, act: str) -> torch.Tensor:
        """ResBlock (:126-138): x + norm(conv2(act(conv1(x)))); a BatchNorm is part of conv2's packed weights"""
        t = self._conv3(self._bf(h), name + ".conv1")
        tb = torch.empty(t.shape, dtype=BF, device=t.device)
        capi.check(capi.lib.dfot_op_dcae_act_bf16(_P(t), _P(tb), t.numel(), _ACTS[act], _S()))
        if norm == "batch_norm":
            return self._conv3(tb, name + ".conv2", resid=h)
        return self._rms(self._conv3(tb, name + ".conv2"), name + ".norm", resid=h)[0]

    def _vit_block(self, h: torch.Tensor, name: str) -> torch.Tensor:
        """EfficientViTBlock (:141-172): ReLU linear attention (+ residual), then GLUMBConv (+ residual)"""
        f, hh, ww, c = h.shape
        n, m = hh * ww, f * hh * ww
        hb, qkv = self._bf(h), torch.empty(m, 3 * c, dtype=BF, device=h.device)
        capi.check(capi.lib.dfot_op_gemm_bf16(_P(hb), c, _P(self._packed[name + ".attn.qkv"]), None, _P(qkv), 3 * c, m, 3 * c, c, _S()))
        o = torch.empty(m, c, dtype=BF, device=h.device)
        capi.check(capi.lib.dfot_op_dcae_linear_attention(_P(qkv), 3 * c, _P(o), c, f, n, c // 32, _S()))
        u = gemm(o, self._packed[name + ".attn.to_out.weight"], n)
        h1, h1b = self._rms(u.view(f, hh, ww, c), name + ".attn.norm_out", resid=h, bf16=True)
        mb = name + ".conv_out"
        t = gemm(h1b.view(m, c), self._packed[mb + ".conv_inverted.weight"], n, self._packed[mb + ".conv_inverted.bias"], silu_bf16=True)
        gl = torch.empty(m, 4 * c, dtype=BF, device=h.device)
        capi.check(capi.lib.dfot_op_dcae_dw_glu(_P(t), _P(self._packed[mb + ".conv_depth.weight"]), _P(self._packed[mb + ".conv_depth.bias"]), _P(gl),
                                                f, hh, ww, 4 * c, _S()))
        u = gemm(gl, self._packed[mb + ".conv_point.weight"], n)
        return self._rms(u.view(f, hh, ww, c), mb + ".norm", resid=h1)[0]

    def _block(self, h: torch.Tensor, name: str, kind: str, norm: str, act: str) -> torch.Tensor:
        return self._res_block(h, name, norm, act) if kind == "ResBlock" else self._vit_block(h, name)

    def _down(self, conv: torch.Tensor, src: Optional[torch.Tensor], cout: int, factor: int) -> torch.Tensor:
        f, h, w, ldc = conv.shape
        out = torch.empty(f, h // factor, w // factor, cout, device=conv.device)
        capi.check(capi.lib.dfot_op_dcae_down_shortcut(_P(conv), ldc, _P(src), _P(out), f, h, w, src.shape[-1] if src is not None else 0, cout, factor,
                                                       _S()))
        return out

    def _up(self, conv: torch.Tensor, src: Optional[torch.Tensor], cin: int, cout: int, factor: int) -> torch.Tensor:
        f, h, w, ldc = conv.shape
        out = torch.empty(f, factor * h, factor * w, cout, device=conv.device)
        capi.check(capi.lib.dfot_op_dcae_up_shortcut(_P(conv), ldc, _P(src), src.shape[-1] if src is not None else 0, _P(out), f, h, w, cin, cout,
                                                     factor, _S()))
        return out

    # ------------------------------------------------------------------ call-time checks (before any device work)
    def _check_maps(self, what: str, s_top: Tuple[int, int], types: Sequence[str], layers: Sequence[int]) -> int:
        """s_top: the coarsest map (the last stage's).  Stage i runs at s_top * 2^(n - 1 - i).  Returns the frame multiple that fills the
        GEMM tiles at the coarsest map."""
        n = len(types)
        for i in range(1, n):
            if types[i] != "EfficientViTBlock" or layers[i] == 0:
                continue
            hh, ww = (s << (n - 1 - i) for s in s_top)
            if hh * ww <= 32:
                raise NotImplementedError(f"{what}: stage {i} (EfficientViTBlock) would run over a {hh}x{ww} map: H*W <= 32 takes the "
                                          "reference's quadratic attention branch, which is not supported")
            if (hh * ww) % 64 or hh * ww > MAX_POSITIONS:
                raise ValueError(f"{what}: stage {i} (EfficientViTBlock) would run over {hh}x{ww} = {hh * ww} positions per frame; supported: "
                                 f"a multiple of 64 up to {MAX_POSITIONS}")
        return 128 // math.gcd(128, s_top[0] * s_top[1])

    @staticmethod
    def _refuse_autograd(what: str, t: torch.Tensor) -> None:
        if torch.is_grad_enabled() and t.requires_grad:
            raise NotImplementedError(f"{what} under autograd is not supported: the module is forward only (call it under torch.no_grad() or "
                                      "detach the input)")


class DCAEEncoder(_DCAEModule):
    """``Encoder`` of the reference ``MyAutoencoderDC`` with its config keys (autoencoder_dc_model.py:286-372, 522-531); the decoder's
    keys are accepted and ignored.  ``encode`` is deterministic: the model has no posterior."""

    def __init__(self, **cfg):
        super().__init__()
        c = self._common("DCAEEncoder", cfg)
        n = len(tuple(c["encoder_block_out_channels"]))
        self.ch, self.layers, self.types, _, _ = _plan("DCAEEncoder", "encoder", c["encoder_block_types"], c["encoder_block_out_channels"],
                                                       c["encoder_layers_per_block"], c["encoder_qkv_multiscales"], ("rms_norm",) * n, ("silu",) * n,
                                                       int(c["attention_head_dim"]), self.latent, int(c["in_channels"]))
        self.s_factor = 2 ** (n - 1)
        self._spec_conv("encoder.conv_in.conv", 3, self.ch[1] // 4)
        for i in range(n):
            for j in range(self.layers[i]):
                self._spec_block(f"encoder.down_blocks.{i}.{j}", self.types[i], self.ch[i], "rms_norm")
            if i < n - 1 and self.layers[i] > 0:
                self._spec_conv(f"encoder.down_blocks.{i}.{self.layers[i]}.conv", self.ch[i], self.ch[i + 1] // 4)
        self._spec_conv("encoder.conv_out", self.ch[-1], self.latent)
        self._register()

    def _check(self, x: torch.Tensor) -> int:
        if x.dtype != torch.float32:
            raise ValueError(f"frames must be float32, got {x.dtype}")
        self._refuse_autograd("DCAEEncoder.encode", x)
        h, w = x.shape[-2:]
        if x.shape[-3] != 3:
            raise ValueError(f"frames have {x.shape[-3]} channels, expected 3")
        if h % self.s_factor or w % self.s_factor:
            raise ValueError(f"frames of {h}x{w} are not divisible by the encoder's spatial factor {self.s_factor}")
        need = self._check_maps(f"frames {tuple(x.shape)}", (h // self.s_factor, w // self.s_factor), self.types, self.layers)
        if not x.is_cuda:
            raise ValueError(f"frames are on {x.device}: the encoder runs on the GPU only (there is no CPU path)")
        capi.require_device(next(self.parameters()).device, frames=x)
        return need

    def _latents(self, x: torch.Tensor, b: int, t: int, strides: Tuple[int, ...], scale: float, shift: float, need: int) -> torch.Tensor:
        """frames (b x t of them, element strides (b, c, t, h, w)), scale * x + shift -> latents fp32 (b * t, latent, h', w')"""
        self._sync()
        h, w = x.shape[-2:]
        sb, sc, st, sh, sw = strides
        f, fp = b * t, pad_to(b * t, need)
        xp = torch.zeros(fp, h, w, 64, dtype=BF, device=x.device)    # frames past f: the zero padding up to whole GEMM tiles
        capi.check(capi.lib.dfot_op_vae_pixels(C.c_void_p(x.data_ptr()), sb, sc, st, sh, sw, scale, shift, _P(xp), b, t, h, w, _S()))
        n = len(self.ch)
        hcur = self._down(self._conv3(xp, "encoder.conv_in.conv"), None, self.ch[1], 2)
        for i in range(n):
            for j in range(self.layers[i]):
                hcur = self._block(hcur, f"encoder.down_blocks.{i}.{j}", self.types[i], "rms_norm", "silu")
            if i < n - 1 and self.layers[i] > 0:
                hcur = self._down(self._conv3(self._bf(hcur), f"encoder.down_blocks.{i}.{self.layers[i]}.conv"), hcur, self.ch[i + 1], 2)
        z = self._down(self._conv3(self._bf(hcur), "encoder.conv_out"), hcur, self.latent, 1)
        return z[:f].permute(0, 3, 1, 2).contiguous()

    def encode(self, x: torch.Tensor) -> torch.Tensor:
        """MyAutoencoderDC.encode: x (F, 3, S, S) in [-1, 1] -> latents (F, 32, S / r, S / r), any F >= 1"""
        if x.ndim != 4 or x.shape[0] < 1:
            raise ValueError(f"frames have shape {tuple(x.shape)}, expected (F, 3, H, W) with F >= 1")
        need = self._check(x)
        with torch.no_grad():
            sf, sc, sh, sw = x.stride()
            return self._latents(x.detach(), x.shape[0], 1, (sf, sc, 0, sh, sw), 1.0, 0.0, need)


class DCAEDecoder(_DCAEModule):
    """``Decoder`` of the reference ``MyAutoencoderDC`` with its config keys (autoencoder_dc_model.py:375-465, 533-544); the encoder's
    keys are accepted and ignored."""

    def __init__(self, **cfg):
        super().__init__()
        c = self._common("DCAEDecoder", cfg)
        n = len(tuple(c["decoder_block_out_channels"]))
        self.ch, self.layers, self.types, self.norms, self.acts = _plan(
            "DCAEDecoder", "decoder", c["decoder_block_types"], c["decoder_block_out_channels"], c["decoder_layers_per_block"],
            c["decoder_qkv_multiscales"], c["decoder_norm_types"], c["decoder_act_fns"], int(c["attention_head_dim"]), self.latent,
            int(c["in_channels"]))
        self.s_factor = 2 ** (n - 1)
        self._spec_conv("decoder.conv_in", self.latent, self.ch[-1])
        for i in range(n):          # the reference inserts the stages at the front of a list: up_blocks.0 registers first
            j0 = 0
            if i < n - 1 and self.layers[i] > 0:
                self._spec_conv(f"decoder.up_blocks.{i}.0.conv", self.ch[i + 1], 4 * self.ch[i])
                j0 = 1
            for j in range(self.layers[i]):
                self._spec_block(f"decoder.up_blocks.{i}.{j0 + j}", self.types[i], self.ch[i], self.norms[i])
        self._specs += [("decoder.norm_out.weight", (self.ch[1],)), ("decoder.norm_out.bias", (self.ch[1],))]
        self._spec_conv("decoder.conv_out.conv", self.ch[1], 12)
        self._register()

    def decode(self, z: torch.Tensor) -> torch.Tensor:
        """MyAutoencoderDC.decode: z (F, 32, h, w) -> frames (F, 3, h r, w r), any F >= 1"""
        if z.ndim != 4 or z.shape[1] != self.latent or z.shape[0] < 1:
            raise ValueError(f"z has shape {tuple(z.shape)}, expected (F, {self.latent}, h, w) with F >= 1")
        self._refuse_autograd("DCAEDecoder.decode", z)
        f, cz, h, w = z.shape
        need = self._check_maps(f"latents {tuple(z.shape)}", (h, w), self.types, self.layers)
        if not z.is_cuda:
            raise ValueError(f"latents are on {z.device}: the decoder runs on the GPU only (there is no CPU path)")
        dev = next(self.parameters()).device
        capi.require_device(dev, z=z)
        with torch.no_grad():
            self._sync()
            n = len(self.ch)
            zc = torch.zeros(pad_to(f, need), h, w, 64, device=dev)     # frames past f: the zero padding up to whole GEMM tiles
            zc[:f, ..., :cz] = z.detach().float().permute(0, 2, 3, 1)
            hcur = self._up(self._conv3(self._bf(zc), "decoder.conv_in"), zc, cz, self.ch[-1], 1)
            for i in reversed(range(n)):
                j0 = 0
                if i < n - 1 and self.layers[i] > 0:
                    hcur = self._up(self._conv3(self._bf(hcur), f"decoder.up_blocks.{i}.0.conv"), hcur, self.ch[i + 1], self.ch[i], 2)
                    j0 = 1
                for j in range(self.layers[i]):
                    hcur = self._block(hcur, f"decoder.up_blocks.{i}.{j0 + j}", self.types[i], self.norms[i], self.acts[i])
            hb = self._rms(hcur, "decoder.norm_out", f32=False, bf16=True, relu=True)[1]
            y = self._up(self._conv3(hb, "decoder.conv_out.conv"), None, 0, 3, 2)
            return y[:f].permute(0, 3, 1, 2).contiguous()


def load_dcae_checkpoint(path: str) -> Dict[str, torch.Tensor]:
    """The flat state dict ``MyAutoencoderDC._from_pretrained_custom`` reads (:706-724): a ``.safetensors`` file, or a ``.pth`` /
    ``.pt`` file holding the mapping itself.

        sd = load_dcae_checkpoint("dcae_dmlab.pth")
        dec = DCAEDecoder(**dcae_config("8x")).cuda(); dec.load_reference_state_dict(sd)"""
    if str(path).endswith(".safetensors"):
        from safetensors.torch import load_file
        return dict(load_file(path))
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, Mapping) or not all(torch.is_tensor(v) for v in sd.values()):
        raise ValueError(f"{path} does not hold a flat state dict (a mapping of names to tensors)")
    return dict(sd)


def decode_dcae_latents(vae: DCAEDecoder, latents: torch.Tensor, vae_batch_size: int = 2, shape: str = "b t c h w") -> torch.Tensor:
    """``BaseVideoAlgo._decode`` for a ``MyAutoencoderDC`` (base_pytorch_video_algo.py:597-604): latents in the sampler's ``b t c h w``
    layout, chunks of ``vae.batch_size`` videos whose frames go to the batch, ``decode(y) * 0.5 + 0.5``, result back in ``b t c h w``.
    Like the reference, ``scaling_factor`` is not applied.  Frames are independent, so the chunking does not change a bit."""
    return map_frame_chunks(lambda ch, row: vae.decode(flat_frames(ch)) * 0.5 + 0.5, latents, vae_batch_size, shape, "latents", "(B, T, C, h, w)")


def encode_dcae_frames(vae: DCAEEncoder, videos: torch.Tensor, vae_batch_size: int = 2, shape: str = "b t c h w") -> torch.Tensor:
    """``BaseVideoAlgo._encode`` for a ``MyAutoencoderDC`` (base_pytorch_video_algo.py:588-596): frames in [0, 1] in the ``b t c h w``
    layout, chunks of ``vae.batch_size`` videos whose frames go to the batch, ``encode(2 y - 1)`` (fused into the pixel pack), latents
    back in ``b t c h w``.  Deterministic; ``scaling_factor`` is not applied."""
    def encode_chunk(ch: torch.Tensor, row: int) -> torch.Tensor:
        need = vae._check(ch)
        b, t = ch.shape[:2]
        sb, st, sc, sh, sw = ch.stride()
        with torch.no_grad():
            return vae._latents(ch.detach(), b, t, (sb, sc, st, sh, sw), 2.0, -1.0, need)
    return map_frame_chunks(encode_chunk, videos, vae_batch_size, shape, "videos", "(B, T, 3, H, W)", "training / sampling")
