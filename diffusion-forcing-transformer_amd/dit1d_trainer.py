"""Training of the DiT1D backbone (``dit1d_backbone.DiT1D``: the reference's frame-causal transformer over 1-D token latents,
algorithms/dfot/backbones/dit1d/dit_model.py, dit1d.yaml) on the MI355X engine: forward with saved activations and the hand-written
backward of ``csrc/dit1d_train.inl`` (share_norm blocks: ``csrc/dit1d_train.hip``; frame-causal attention backward:
``csrc/attention_frame_causal.hip`` / ``csrc/attention_bwd.hip``), the flat AdamW state and the denoising loss every trainer shares.

``DiT1DTrainer`` has the constructor keywords and the method set of ``trainer.DiT3DTrainer``, which it extends with ``_family = "dit1d"``:
the engine binding (layout, flat AdamW state, weight sync, reserve, backward, input gradient), the loss, the optimizer step, the state
dicts, accumulation and EMA are that class's; its own are the configuration checks, the forward and the refusals.  ``pos_embed`` is a frozen
parameter of the reference (``requires_grad=False``): it is kept OUT of the flat parameter / gradient / moment buffers (``self.buffers``,
as the Fourier buffers of a continuous DiT3D), so it has no gradient, no optimizer state, no weight decay and no entry in ``grad_dict()``;
``state_dict()`` lists it first, where the reference's does, and loads strictly into ``DiT1D``.

Built: what ``DiT1D`` builds (``dit1d_backbone.check_config``) with hidden_size and the MLP width multiples of 128, discrete diffusion,
no condition, ``T == max_tokens``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import capi
from .backbone import _get
from .diffusion import DiffusionConfig
from .dit1d_backbone import check_config, sincos_pos_embed_1d
from .trainer import DiT3DTrainer


class DiT1DTrainer(DiT3DTrainer):
    _family = "dit1d"

    def __init__(self, cfg, x_shape: Sequence[int], max_tokens: int, timesteps: int = 1000, diffusion: Optional[DiffusionConfig] = None,
                 lr: float = 5e-5, weight_decay: float = 0.01, betas: Tuple[float, float] = (0.9, 0.99), eps: float = 1e-8,
                 max_grad_norm: Optional[float] = 1.0, loss_weighting: Optional[Dict] = None, external_cond_dim: int = 0):
        if _get(cfg, "use_fourier_noise_embedding", False):
            raise ValueError("use_fourier_noise_embedding=True is not built: DiT1D embeds integer noise levels (discrete diffusion only)")
        if diffusion is not None and diffusion.is_continuous:
            raise ValueError("DiffusionConfig(is_continuous=True) is not built: DiT1DTrainer trains under discrete diffusion only")
        self.x_shape, self.causal_attn_mode, c = check_config(cfg, x_shape, max_tokens, external_cond_dim, timesteps)
        if c.hidden % 128 or c.mlp_hidden % 128:
            raise ValueError(f"hidden_size={c.hidden} / MLP width {c.mlp_hidden}: training needs multiples of 128 (the weight-gradient GEMMs "
                             "tile a feature axis by 128)")
        self.is_continuous = False
        self.external_cond_dropout = 0.0
        self._ccfg = c
        self.max_tokens = int(c.max_tokens)
        self._handle = C.c_void_p()
        capi.check(capi.lib.dfot_dit1d_train_create(C.byref(c), C.byref(self._handle)))
        self._bind_engine()
        # the frozen pos_embed (the reference's sin-cos table until a state dict brings another): a tensor of its own
        self.buffers: Dict[str, torch.Tensor] = {"pos_embed": sincos_pos_embed_1d(int(c.hidden), self.max_tokens * int(c.tokens_per_frame)).cuda()}
        self._load_buffers()
        self._init_training_state(timesteps, diffusion, lr, weight_decay, betas, eps, max_grad_norm, loss_weighting)
        self._keep: Optional[Tuple[torch.Tensor, torch.Tensor]] = None

    def forward(self, x: torch.Tensor, noise_levels: torch.Tensor, cond: Optional[torch.Tensor] = None,
                cond_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        if cond is not None or cond_mask is not None:
            raise ValueError("this DiT1DTrainer is unconditioned (external_cond_dim 0): it takes no condition")
        if x.ndim != 5 or tuple(x.shape[2:]) != self.x_shape:
            raise ValueError(f"x has shape {tuple(x.shape)}, expected (B, {self.max_tokens}, {', '.join(map(str, self.x_shape))})")
        b, t = x.shape[:2]
        if t != self.max_tokens:
            raise ValueError(f"T = {t} tokens, but DiT1D trains at T == max_tokens = {self.max_tokens} only: its pos_embed add fixes the "
                             "sequence length, as in the reference")
        if tuple(noise_levels.shape) != (b, t):
            raise ValueError(f"noise_levels has shape {tuple(noise_levels.shape)}, expected {(b, t)}")
        if noise_levels.is_floating_point():
            raise TypeError("DiT1DTrainer takes integer noise levels (DiscreteDiffusion passes the level index); continuous diffusion "
                            "(floating noise levels) is not built")
        self._prepare(b)
        xd = x.to(device="cuda", dtype=torch.float32).contiguous()
        lv = noise_levels.to(device="cuda", dtype=torch.int32).contiguous()
        out = torch.empty_like(xd)
        capi.check(capi.lib.dfot_dit1d_train_forward(self._handle, capi.ptr(xd), capi.ptr(lv), capi.ptr(out), b, t, capi.stream_ptr()))
        self._keep = (xd, lv)  # the engine reads x again in backward (token-embedding gradient)
        return out

    def _require_forward(self, what: str) -> None:
        if self._keep is None:
            raise RuntimeError(f"{what}: no forward to differentiate; call forward (or loss_and_grads) first")

    def backward(self, d_out: torch.Tensor) -> None:
        self._require_forward("backward")
        if tuple(d_out.shape) != tuple(self._keep[0].shape):
            raise ValueError(f"d_out has shape {tuple(d_out.shape)}, the last forward's output {tuple(self._keep[0].shape)}")
        super().backward(d_out)

    def input_grad(self) -> torch.Tensor:
        """d(sum(out * d_out)) / d x of the last forward / backward pair, in x's layout"""
        self._require_forward("input_grad")
        return super().input_grad()

    def _condition(self, conditions, b: int, t: int, generator):
        if conditions is not None:
            raise ValueError("this DiT1DTrainer is unconditioned (external_cond_dim 0): it takes no conditions")
        return None, None

    def difference_loss_and_grads(self, *args, **kwargs):
        raise ValueError("difference_loss_and_grads needs the difference model (DiT3DTrainer, variant factorized_matrix_attention)")
