"""Drop-in UViT3D backbone (the reference's pose-free U-ViT, algorithms/dfot/backbones/u_vit/u_vit3d.py:22-335) backed by libdfot_hip.so.

UViT3DPose's parent class in the reference: the same U-Net, conditioned by a per-frame vector only,

    emb = noise_level_pos_embedding(k) [+ external_cond_embedding(external_cond, external_cond_mask)]          (u_vit3d.py:306-310)

so it serves every dataset without camera poses: unconditioned video (``external_cond=None``) and action-conditioned video
(``(B, T, external_cond_dim)`` actions: dmlab, Minecraft).  Constructor keywords, ``forward`` signature and state-dict key names / order are
the reference's (up_blocks are listed before mid_blocks, as its ``state_dict()`` lists them), so reference checkpoints load with
``load_state_dict`` / ``checkpoint.load_reference_checkpoint``.  The engine is ``dfot_uvit3d_*`` (include/dfot_hip.h): one embedding kernel
per forward, the pose-free norm kernels, and every GEMM / convolution / attention kernel of the pose engine unchanged; there is no
conditioning cache and no per-window state.  Forward only: under autograd it raises NotImplementedError.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import capi, ops
from .backbone import UViTModule, _get

_BLOCKS = ["ResBlock", "ResBlock", "TransformerBlock", "TransformerBlock"]


class UViT3D(UViTModule):
    """The handle type is UViT3DPose's (backbone.UViTModule: its read-outs, taps and initialisers); construction and forward are its own."""
    _create = "dfot_uvit3d_create"

    def __init__(self, cfg, x_shape: Sequence[int], max_tokens: int, external_cond_dim: int = 0, use_causal_mask: bool = True,
                 external_cond_type: str = "action", external_cond_num_classes: Optional[int] = None):
        super().__init__()
        block_types = list(_get(cfg, "block_types", _BLOCKS))
        if "AxialTransformerBlock" in block_types:
            raise ValueError("block type 'AxialTransformerBlock' is not built: only [ResBlock, ResBlock, TransformerBlock, TransformerBlock]")
        if block_types != _BLOCKS:
            raise ValueError(f"unsupported block_types {block_types}: only {_BLOCKS}")
        pos = _get(cfg, "pos_emb_type", "rope")
        if pos != "rope":
            raise ValueError(f"pos_emb_type {pos!r} is not built: only 'rope'")
        if not _get(cfg, "use_fourier_noise_embedding", False):
            raise ValueError("only the Fourier noise-level embedding (use_fourier_noise_embedding: true, continuous diffusion) is built")
        if int(_get(cfg, "patch_size", 2)) != 2:
            raise ValueError("only patch_size=2 is supported")
        if external_cond_dim and external_cond_type != "action":
            raise ValueError(f"external_cond_type {external_cond_type!r} is not built for UViT3D: only 'action'")
        channels, heads = list(_get(cfg, "channels")), int(_get(cfg, "num_heads"))
        for lvl in (2, 3):
            d, rem = divmod(int(channels[lvl]), heads)
            if rem or d not in (64, 128):
                raise ValueError(f"head dim {channels[lvl]}/{heads} = {channels[lvl] / heads:g} at level {lvl} is outside the engine's limit: "
                                 "the attention kernels are built for head dim 64 or 128")
        self.cfg = cfg
        self.x_shape = tuple(x_shape)
        self.max_tokens = self.temporal_length = int(max_tokens)
        self.external_cond_dim = int(external_cond_dim or 0)
        self.external_cond_type = external_cond_type
        self.external_cond_num_classes = external_cond_num_classes
        self.external_cond_dropout = float(_get(cfg, "external_cond_dropout", 0.0) or 0.0) if self.external_cond_dim else 0.0
        self.use_causal_mask = use_causal_mask
        c = capi.UViT3DConfig()
        c.channels[:] = channels
        c.emb_channels = int(_get(cfg, "emb_channels"))
        c.num_updown_blocks[:] = list(_get(cfg, "num_updown_blocks"))
        c.num_mid_blocks = int(_get(cfg, "num_mid_blocks"))
        c.num_heads = heads
        c.in_channels = int(self.x_shape[0])
        c.resolution = int(self.x_shape[-1])
        c.max_tokens = self.max_tokens
        c.cond_dim = self.external_cond_dim
        c.noise_dim = 256  # UViT3D.noise_level_dim (u_vit3d.py:187-189)
        c.rope_theta = 10000.0
        c.eps = 1e-6
        c.cond_dropout = int(self.external_cond_dropout > 0)
        self._ccfg = c
        self._build_tree()
        self.live_frames = None      # set by the sampler around its backbone calls (uint8 (B, T), 0 = output discarded), None otherwise
        self._dropout_generator: Optional[torch.Generator] = None  # generator of the per-video condition dropout draw in train()

    # ------------------------------------------------------------------ forward
    def _condition_mask(self, external_cond_mask: Optional[torch.Tensor], batch: int, dev) -> Optional[torch.Tensor]:
        """which videos run without their condition, as RandomDropoutCondEmbedding decides it (embeddings.py:345-387): built with dropout 0
        the module IS a TimestepEmbedding and never sees the mask; with dropout > 0 a (B,) mask zeroes the embedding in eval() (it is
        refused in train(), as the reference asserts), and train() draws one Bernoulli(dropout) per video from _dropout_generator."""
        if self.external_cond_dropout <= 0:
            return None
        if external_cond_mask is not None:
            assert not self.training, "embedding mask is only allowed during inference"
            assert external_cond_mask.ndim == 1, "embedding mask should be of shape (B,)"
            if external_cond_mask.shape[0] != batch:
                raise ValueError(f"external_cond_mask has shape {tuple(external_cond_mask.shape)}, expected {(batch,)}")
            return external_cond_mask.detach().to(device=dev, dtype=torch.uint8).contiguous()
        if self.training:
            return (torch.rand(batch, device=dev, generator=self._dropout_generator) < self.external_cond_dropout).to(torch.uint8)
        return None

    def forward(self, x: torch.Tensor, noise_levels: torch.Tensor, external_cond: Optional[torch.Tensor] = None,
                external_cond_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """BaseBackbone.forward; dispatched as the torch operator ``dfot::uvit3d_forward`` (ops.py)."""
        assert x.shape[1] == self.temporal_length, (
            f"Temporal length of U-ViT is set to {self.temporal_length}, but input has temporal length {x.shape[1]}.")
        if external_cond is not None and not self.external_cond_dim:
            raise ValueError("this UViT3D was built with external_cond_dim 0: it has no external condition embedding")
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("UViT3D is forward only: training and reconstruction guidance (the gradient w.r.t. x) are not built; "
                                      "call it under torch.no_grad() or with parameters that do not require grad")
        if self._op_key is None:
            self._op_key = ops.register_model(self)
        mask = None if external_cond is None else self._condition_mask(external_cond_mask, x.shape[0], x.device)
        return torch.ops.dfot.uvit3d_forward(x, noise_levels, external_cond, mask, self._op_key)

    def _forward_impl(self, x: torch.Tensor, noise_levels: torch.Tensor, external_cond: Optional[torch.Tensor] = None,
                      external_cond_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        b = x.shape[0]
        if x.ndim != 5 or tuple(x.shape[1:]) != (self.temporal_length, *self.x_shape):
            raise ValueError(f"x has shape {tuple(x.shape)}, expected (B, {self.temporal_length}, {', '.join(map(str, self.x_shape))})")
        if tuple(noise_levels.shape) != (b, self.temporal_length):
            raise ValueError(f"noise_levels has shape {tuple(noise_levels.shape)}, expected {(b, self.temporal_length)}")
        if not noise_levels.is_floating_point():
            raise TypeError("UViT3D takes floating noise levels (ContinuousDiffusion passes precond_scale * logsnr)")
        if external_cond is not None and tuple(external_cond.shape) != (b, self.temporal_length, self.external_cond_dim):
            raise ValueError(f"external_cond has shape {tuple(external_cond.shape)}, expected {(b, self.temporal_length, self.external_cond_dim)}")
        if external_cond_mask is not None and tuple(external_cond_mask.shape) != (b,):
            raise ValueError(f"external_cond_mask has shape {tuple(external_cond_mask.shape)}, expected {(b,)}")
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError(f"the backbone's parameters are on {dev}; move the module to the GPU first (there is no CPU path)")
        # the kernels dereference raw pointers: a host tensor must be refused before anything is launched
        capi.require_device(dev, x=x, noise_levels=noise_levels, external_cond=external_cond, external_cond_mask=external_cond_mask)
        self.sync_weights()
        self.reserve(b)
        xf = x.detach().to(torch.float32).contiguous()
        kf = noise_levels.detach().to(torch.float32).contiguous()
        cf = None if external_cond is None else external_cond.detach().to(torch.float32).contiguous()
        mf = None if external_cond_mask is None else external_cond_mask.to(torch.uint8).contiguous()
        live = self.live_frames
        if live is not None:
            if tuple(live.shape) != (b, self.temporal_length) or live.dtype != torch.uint8 or not live.is_contiguous():
                raise ValueError(f"live_frames must be a contiguous uint8 tensor of shape {(b, self.temporal_length)}")
            capi.require_device(dev, live_frames=live)
        out = torch.empty_like(xf)
        capi.check(capi.lib.dfot_uvit3d_forward_live(self._handle, capi.ptr(xf, torch.float32, "x"), capi.ptr(kf, torch.float32, "noise_levels"),
                                                     capi.ptr(cf, torch.float32, "external_cond"), capi.ptr(mf, torch.uint8, "external_cond_mask"),
                                                     capi.ptr(out), b, capi.ptr(live, torch.uint8, "live_frames"), capi.stream_ptr()))
        return out.to(x.dtype)

    def read_nemb(self, batch: int) -> torch.Tensor:
        """tap "nemb": the per-frame embedding of the last forward, (batch * T, emb_channels)"""
        out = torch.empty(batch * self.temporal_length, int(self._ccfg.emb_channels), device="cuda", dtype=torch.float32)
        capi.check(capi.lib.dfot_uvit_read_tap(self._handle, b"nemb", capi.ptr(out), out.numel(), capi.stream_ptr()))
        return out
