"""What the latent codecs (VideoVAE, ImageVAE, TiTok-KL, DC-AE) share on the host: the module base (registration under the reference's
state-dict names, packing on weight change, strict loading, GroupNorm / cast calls), the weight packers, the GEMM call with its split-K
rule, the one-tap and fused-upsample convolution calls, and the ``b t c h w`` chunk loop.  Every value is still computed by a HIP kernel
behind the C ABI; nothing here is specific to one codec, and the codec modules import their shared private names from here only.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Mapping, Optional, Tuple

import torch
from torch import nn

from . import capi

BF = torch.bfloat16
_P = capi.ptr
_S = capi.stream_ptr
_GEMM_KS2 = 8             # GemmVariant GEMM_DMA_128_KS2 (csrc/gemm.h): 128x128 tile with K split inside the workgroup
_E_BF16, _ACT_SILU = 1, 2  # dfot_op_gemm_ex: the bf16 epilogue and its SiLU
_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def pad_to(n: int, m: int) -> int:
    return -(-n // m) * m


def channel_vector(v, n: int, dev, what: str) -> Optional[torch.Tensor]:
    if v is None:
        return None
    t = torch.as_tensor(v, dtype=torch.float32).reshape(-1).to(dev).contiguous()
    if t.numel() != n:
        raise ValueError(f"{what} has {t.numel()} values, expected one per latent channel ({n})")
    return t


# ---------------------------------------------------------------------------------------------------------------------------------
# weights -> bf16 GEMM operands
def pack_conv3x3(w: torch.Tensor, cop: int, cip: int) -> torch.Tensor:
    """[co][ci][3][3] fp32 -> bf16 [cop][9 * cip] (tap-major: dfot_op_pack_conv3), channels zero-padded to cop / cip"""
    co, ci = w.shape[:2]
    w2 = torch.zeros(cop, cip, 3, 3, device=w.device)
    w2[:co, :ci] = w
    out = torch.empty(cop, 9 * cip, dtype=BF, device=w.device)
    capi.check(capi.lib.dfot_op_pack_conv3(_P(w2.contiguous()), _P(out), cop, cip, 0, _S()))
    return out


def pack_1x1(w: torch.Tensor, cop: int, cip: int) -> torch.Tensor:
    """[co][ci](1)(1)(1) fp32 -> bf16 [cop][cip]: a Linear, channels zero-padded to cop / cip"""
    co, ci = w.shape[:2]
    m = w.reshape(co, ci)
    if (cop, cip) != (co, ci):
        m = torch.zeros(cop, cip, device=w.device)
        m[:co, :ci] = w.reshape(co, ci)
    return m.to(BF).contiguous()


def pack_conv_layers(f: Mapping[str, torch.Tensor], pack: Callable[[str, torch.Tensor], Tuple[torch.Tensor, int]]) -> Dict[str, torch.Tensor]:
    """every convolution weight of f (ndim >= 4; norm weights and biases are 1-D) through ``pack(name, w) -> (operand, cop)``, its bias
    zero-padded to cop"""
    pk: Dict[str, torch.Tensor] = {}
    for name, w in f.items():
        if w.ndim < 4:
            continue
        pk[name], cop = pack(name, w)
        b = torch.zeros(cop, device=w.device)
        b[: w.shape[0]] = f[name[:-6] + "bias"]
        pk[name[:-6] + "bias"] = b
    return pk


# ---------------------------------------------------------------------------------------------------------------------------------
# kernel calls
def splits_k(rows1: int, n: int, k: int) -> bool:
    """Whether a GEMM of ONE frame's ``rows1`` rows by n columns over k splits K inside the workgroup (the one tile form with another
    summation order, picked for few tiles and a long K).  The batch is not an argument: a frame's bits do not depend on it."""
    return k >= 2048 and (pad_to(rows1, 128) // 128) * (-(-n // 128)) <= 256


def gemm(a: torch.Tensor, w: torch.Tensor, rows1: int, bias: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
         silu_bf16: bool = False) -> torch.Tensor:
    """a bf16 [M][K] w^T (+ bias) (+ resid) -> fp32 [M][N], or SiLU(.) as bf16 (the GEMM's bf16 epilogue with act = 2).  ``rows1``: one
    frame's rows (see ``splits_k``)."""
    m, (n, k) = a.shape[0], w.shape
    out = torch.empty(m, n, dtype=BF if silu_bf16 else torch.float32, device=a.device)
    ks2 = splits_k(rows1, n, k)
    if not silu_bf16 and not ks2:   # here the shape-picked form never splits K: a frame's tile count only grows with the batch
        capi.check(capi.lib.dfot_op_gemm_f32(_P(a), k, _P(w), _P(bias), _P(resid), _P(out), n, m, n, k, _S()))
        return out
    d = capi.GemmDesc()
    d.qscale, d.eps, d.ksplit, d.variant = 1.0, 1e-6, 1, (_GEMM_KS2 if ks2 else -1)
    d.A, d.lda, d.W, d.M, d.N, d.K = a.data_ptr(), k, w.data_ptr(), m, n, k
    d.bias, d.resid, d.ldo = (bias.data_ptr() if bias is not None else None), (resid.data_ptr() if resid is not None else None), n
    if silu_bf16:
        d.epi, d.act, d.out_bf16 = _E_BF16, _ACT_SILU, out.data_ptr()
    else:
        d.out_f32 = out.data_ptr()
    capi.check(capi.lib.dfot_op_gemm_ex(C.byref(d), _S()))
    return out


def conv3x3(x: torch.Tensor, wp: torch.Tensor, bias: Optional[torch.Tensor], resid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Conv2d(k 3, s 1, p 1) per frame on a bf16 [F][H][W][Ci] operand -> fp32 [F][H][W][Co] (+ resid): the strided implicit-GEMM entry
    with one temporal tap and stride 1, whose summation order depends on one frame's shape only"""
    f, h, w, ci = x.shape
    co = wp.shape[0]
    out = torch.empty(f, h, w, co, device=x.device)
    capi.check(capi.lib.dfot_op_conv3t_f32(_P(x), _P(wp), _P(bias), _P(resid), _P(out), f, 1, h, w, ci, co, 1, 1, 1, _S()))
    return out


def upconv3x3(x: torch.Tensor, wp: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """nearest 2x fused into the gather of Conv2d(k 3, s 1, p 1): bf16 [F][H][W][Ci] -> fp32 [F][2 H][2 W][Co]"""
    f, h, w, ci = x.shape
    co = wp.shape[0]
    out = torch.empty(f, 2 * h, 2 * w, co, device=x.device)
    capi.check(capi.lib.dfot_op_upconv3x3_f32(_P(x), _P(wp), _P(bias), _P(out), f, h, w, ci, co, _S()))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the module base
class CodecModule(nn.Module):
    """Parameters (and BatchNorm-style buffers) registered under the reference's state-dict names from ``_specs``; per weight change, one
    name -> detached tensor map (``_par``) and the packed operands a subclass builds in ``_pack_weights``; strict loading."""

    _reference_model = "reference"     # the model a foreign key is reported against
    _tensor_noun = "parameter "        # how a host-resident tensor is reported ("" where buffers are registered too)

    def _register(self) -> None:
        self._names = [n for n, _ in self._specs]
        for name, shape in self._specs:
            *path, leaf = name.split(".")
            node: nn.Module = self
            for part in path:
                if part not in node._modules:
                    node.add_module(part, nn.Module())
                node = node._modules[part]
            if leaf == "num_batches_tracked":
                node.register_buffer(leaf, torch.tensor(0, dtype=torch.long))
            elif leaf in _BUFFERS:
                node.register_buffer(leaf, torch.ones(shape) if leaf == "running_var" else torch.zeros(shape))
            else:
                node.register_parameter(leaf, nn.Parameter(torch.zeros(shape), requires_grad=False))
        self._packed: Dict[str, torch.Tensor] = {}
        self._live: Dict[str, torch.Tensor] = {}
        self._sig = None

    def _tensors(self) -> Dict[str, torch.Tensor]:
        sd = dict(self.named_parameters())
        sd.update(dict(self.named_buffers()))
        return {n: sd[n] for n in self._names}

    def init_random(self, seed: int = 0) -> None:
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for n, p in self.named_parameters():
                if n.endswith("bias"):
                    v = 0.02 * torch.randn(p.shape, generator=g)
                elif p.ndim == 1:
                    v = 1.0 + 0.1 * torch.randn(p.shape, generator=g)
                else:
                    v = torch.randn(p.shape, generator=g) / (p[0].numel() ** 0.5)
                p.copy_(v.to(p.device))
            g = torch.Generator().manual_seed(seed + 1)
            for n, b in self.named_buffers():
                if n.endswith("running_var"):
                    b.copy_((0.5 + torch.rand(b.shape, generator=g)).to(b.device))
                elif n.endswith("running_mean"):
                    b.copy_((0.1 * torch.randn(b.shape, generator=g)).to(b.device))

    # ------------------------------------------------------------------ weights -> kernel operands, once per weight change
    def _sync(self) -> None:
        """(data_ptr, _version) of every tensor is the signature: a ``.cuda()`` / ``.to()`` move or an in-place edit changes it, and
        then ``_par``'s map and the packed operands (``_pack_weights`` of the subclass) are rebuilt"""
        ts = self._tensors()
        sig = tuple((t.data_ptr(), t._version) for t in ts.values())
        if sig == self._sig:
            return
        for name, t in ts.items():
            if not t.is_cuda:
                raise RuntimeError(f"{self._tensor_noun}{name} is on {t.device}; move the module to the GPU first (there is no CPU path)")
        self._live = {n: t.detach() for n, t in ts.items()}
        self._packed = self._pack_weights({n: (t.float() if t.is_floating_point() else t) for n, t in self._live.items()})
        self._sig = sig

    def _pack_weights(self, f: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """f: every tensor of ``_names`` on the GPU, detached, floating ones as fp32 -> the packed operands of this codec"""
        raise NotImplementedError

    def _par(self, name: str) -> torch.Tensor:
        return self._live[name]

    # ------------------------------------------------------------------ building blocks
    def _gn(self, x: torch.Tensor, name: str, silu: bool, b: int) -> torch.Tensor:
        """GroupNorm(32) with statistics over each of ``b`` equal slices of x: b = videos (over T, H, W) or videos * frames (per frame)"""
        c = x.shape[-1]
        pixels = x.numel() // (b * c)
        out = torch.empty(x.shape, dtype=BF, device=x.device)
        scratch = torch.empty(int(capi.lib.dfot_op_groupnorm_scratch_floats(b, pixels)), device=x.device)
        capi.check(capi.lib.dfot_op_groupnorm(_P(x), _P(self._par(name + ".weight")), _P(self._par(name + ".bias")), 1e-6, _P(out), _P(scratch), b,
                                              pixels, c, int(silu), _S()))
        return out

    def _bf(self, x: torch.Tensor) -> torch.Tensor:
        out = torch.empty(x.shape, dtype=BF, device=x.device)
        capi.check(capi.lib.dfot_op_f32_to_bf16(_P(x), _P(out), x.numel(), _S()))
        return out

    # ------------------------------------------------------------------ loading
    def load_reference_state_dict(self, state_dict: Mapping[str, torch.Tensor],
                                  other_half: Optional[Callable[[str], bool]] = None) -> List[str]:
        """keys of the reference model (optionally ``vae.``-prefixed as in the Lightning checkpoint): this module's own keys -- buffers
        among them -- are loaded, strictly (every one must be present with its shape); every other key is ignored and returned.  With
        ``other_half`` (a predicate on the unprefixed name: the keys of the model's other half), any key that is neither this module's
        nor the other half's raises ``ValueError`` before anything is copied."""
        own = self._tensors()
        names = {k: (k[4:] if k.startswith("vae.") else k) for k in state_dict}
        if other_half is not None:
            for k, n in names.items():
                if n not in own and not other_half(n):
                    raise ValueError(f"unexpected key in a {self._reference_model} state dict: {k}")
        ignored, seen = [], set()
        with torch.no_grad():
            for k, v in state_dict.items():
                n = names[k]
                if n in own:
                    if tuple(v.shape) != tuple(own[n].shape):
                        raise ValueError(f"size mismatch for {n}: {tuple(v.shape)} vs {tuple(own[n].shape)}")
                    own[n].copy_(v)
                    seen.add(n)
                else:
                    ignored.append(k)
        missing = [n for n in own if n not in seen]
        if missing:
            raise ValueError(f"keys not found in the checkpoint: {missing[:5]}{'...' if len(missing) > 5 else ''}")
        return ignored


def gn_res_block(m: CodecModule, x: torch.Tensor, name: str, ci: int, co: int, b: int) -> torch.Tensor:
    """The GroupNorm ``ResnetBlock`` of the VideoVAE and the ImageVAE on module m's ``_conv``: conv2(silu(norm2(conv1(silu(norm1(x))))))
    + x, or + nin_shortcut(x) with a channel change.  Bound as their ``_res``."""
    h = m._conv(m._gn(x, name + ".norm1", True, b), name + ".conv1")
    sc = x if ci == co else m._conv(m._bf(x), name + ".nin_shortcut")
    return m._conv(m._gn(h, name + ".norm2", True, b), name + ".conv2", resid=sc)


# ---------------------------------------------------------------------------------------------------------------------------------
# ``BaseVideoAlgo._encode`` / ``_decode``: chunks of ``vae.batch_size`` videos
def chunks(x: torch.Tensor, vae_batch_size: int):
    return torch.chunk(x, (x.shape[0] + vae_batch_size - 1) // vae_batch_size, 0)


def flat_frames(ch: torch.Tensor) -> torch.Tensor:
    """``b t c h w -> (b t) c h w``"""
    b, t = ch.shape[:2]
    return ch.reshape(b * t, *ch.shape[2:])


def refuse_layout(x: torch.Tensor, shape: str, what: str, expected: str, path: str = "sampling") -> None:
    if shape != "b t c h w":
        raise ValueError(f"only the 'b t c h w' layout of the {path} path is supported")
    if x.ndim != 5:
        raise ValueError(f"{what} have shape {tuple(x.shape)}, expected {expected}")


def map_frame_chunks(body: Callable[[torch.Tensor, int], torch.Tensor], x: torch.Tensor, vae_batch_size: int, shape: str, what: str,
                     expected: str, path: str = "sampling") -> torch.Tensor:
    """The per-frame codecs' loop: x (B, T, ...) in chunks of ``vae_batch_size`` videos; ``body(chunk, first video's index)`` returns the
    chunk's frames ``((b t), ...)``, which go back to ``(b, t, ...)`` and are concatenated.  Refuses another layout and ndim != 5 first."""
    refuse_layout(x, shape, what, expected, path)
    outs, row = [], 0
    for ch in chunks(x, vae_batch_size):
        b, t = ch.shape[:2]
        y = body(ch, row)
        outs.append(y.reshape(b, t, *y.shape[1:]))
        row += b
    return torch.cat(outs, 0)
