"""Training of the DiT3D backbone on the MI355X engine: hand-written forward-with-saved-activations and backward
(``csrc/dit_train.inl``), fused AdamW with gradient-norm clipping on flat fp32 buffers (``flat_optim.FlatAdamW``), data parallelism by ONE all-reduce of
the flat gradient buffer per step (RCCL through ``torch.distributed``; the buffer is a torch tensor).

Mirrors, for the DiT3D "full" / rope_3d model (README ``@DiT/XL``, attention-only blocks in this fork):
  * ``DFoTVideo.training_step``                     algorithms/dfot/dfot_video.py:41-75
  * ``DiscreteDiffusion.forward`` (pred_v)          algorithms/dfot/diffusion/discrete_diffusion.py:345-377
  * ``BasePytorchAlgo.configure_optimizers``        AdamW(lr, weight_decay, betas) + Lightning's gradient_clip_val
  * DDP gradient averaging                          experiments (Lightning ``ddp`` strategy)
No autograd and no torch kernels on the path: torch provides device memory, the stream and the collective.

Continuous diffusion (``@diffusion/continuous``): built with ``diffusion=DiffusionConfig(is_continuous=True, ...)`` and a cfg with
``use_fourier_noise_embedding: true`` the same trainer runs ``ContinuousDiffusion.forward`` (continuous_diffusion.py:140-167): levels are
t in [0, 1], the backbone receives ``precond_scale * logsnr(t)`` as floats, the loss is the sigmoid-weighted one of ``dfot_vpred_loss``.
FourierEmbedding's ``freqs`` / ``phases`` are buffers: they are kept OUT of the flat parameter / gradient / moment buffers (``self.buffers``),
so they have no gradient, no optimizer state, no weight decay and no entry in ``grad_dict()``; ``state_dict()`` lists them first, where
the reference's does.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import capi
from .backbone import _get
from .diffusion import DiffusionConfig, Schedule, denoising_loss, masked_mean
from .flat_optim import FlatAdamW, FlatAdamWOwner, alias


class DiT3DTrainer(FlatAdamWOwner):
    params, grads = alias("params"), alias("grads")

    def __init__(self, cfg, x_shape: Sequence[int], max_tokens: int, timesteps: int = 1000,
                 diffusion: Optional[DiffusionConfig] = None, lr: float = 5e-5, weight_decay: float = 0.01,
                 betas: Tuple[float, float] = (0.9, 0.99), eps: float = 1e-8, max_grad_norm: Optional[float] = 1.0,
                 loss_weighting: Optional[Dict] = None, external_cond_type: str = "action",
                 external_cond_num_classes: Optional[int] = None, external_cond_dim: int = 0):
        from .dit_backbone import FOURIER_BUFFERS, configure_condition
        self.x_shape = tuple(int(v) for v in x_shape)
        c = capi.DiTConfigF()
        configure_condition(c, cfg, external_cond_type, external_cond_num_classes, external_cond_dim)
        self.external_cond_dropout = float(_get(cfg, "external_cond_dropout", 0.0) or 0.0) if external_cond_dim else 0.0
        c.depth = int(_get(cfg, "depth"))
        c.num_heads = int(_get(cfg, "num_heads"))
        c.patch_size = int(_get(cfg, "patch_size", 2))
        c.in_channels, c.height, c.width = self.x_shape
        c.noise_dim, c.timesteps, c.rope_theta, c.eps = 256, int(timesteps), 10000.0, 1e-6
        self._configure(c, cfg, int(max_tokens))
        fourier = bool(_get(cfg, "use_fourier_noise_embedding", False))
        continuous = bool(diffusion is not None and diffusion.is_continuous)
        if fourier != continuous:
            raise ValueError(f"use_fourier_noise_embedding={fourier} with DiffusionConfig(is_continuous={continuous}): continuous diffusion "
                             "needs the Fourier noise-level embedding (float levels) and discrete diffusion the indexed one")
        self.is_continuous = continuous
        c.fourier_noise = int(fourier)
        self._ccfg = c
        self.max_tokens = int(c.max_tokens)
        self._handle = C.c_void_p()
        self._create(c)
        self._bind_engine()
        # FourierEmbedding's buffers (reference draw: 2 pi N(0,1), 2 pi U[0,1)); tensors of their own, never part of the flat buffers
        self.buffers: Dict[str, torch.Tensor] = {}
        if fourier:
            self.buffers = {FOURIER_BUFFERS[0]: (2 * np.pi * torch.randn(int(c.noise_dim))).cuda(),
                            FOURIER_BUFFERS[1]: (2 * np.pi * torch.rand(int(c.noise_dim))).cuda()}
            self._load_buffers()
        self._init_training_state(timesteps, diffusion, lr, weight_decay, betas, eps, max_grad_norm, loss_weighting)

    _family = "dit"  # the engine's C family: every call below is dfot_<family>_train_<name> (DiT1DTrainer: "dit1d")

    def _engine(self, name: str):
        return getattr(capi.lib, f"dfot_{self._family}_train_{name}")

    def _bind_engine(self) -> None:
        """the created handle's parameter layout, the flat AdamW state over it (torch owns the buffers: the gradient buffer is what
        torch.distributed all-reduces), attached to the engine"""
        h = self._handle
        self.numel = int(self._engine("total_numel")(h))
        shape, ndim = (C.c_int64 * 4)(), C.c_int()
        self.layout: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        for i in range(self._engine("num_params")(h)):
            capi.check(self._engine("param_shape")(h, i, shape, C.byref(ndim)))
            self.layout[self._engine("param_name")(h, i).decode()] = (
                int(self._engine("param_offset")(h, i)), tuple(int(shape[k]) for k in range(ndim.value)))
        self.opt = FlatAdamW(self.layout, self.numel)
        capi.check(self._engine("attach")(h, capi.ptr(self.params), capi.ptr(self.grads)))

    def _init_training_state(self, timesteps, diffusion, lr, weight_decay, betas, eps, max_grad_norm, loss_weighting) -> None:
        self.lr, self.weight_decay, self.betas, self.eps, self.max_grad_norm = lr, weight_decay, tuple(betas), eps, max_grad_norm
        self.schedule = Schedule(diffusion or DiffusionConfig(beta_schedule="cosine", is_continuous=False, timesteps=timesteps))
        self.loss_weighting = dict(loss_weighting or {})
        self._reserved = 0
        self._dirty = True
        self._last: Optional[dict] = None

    def _configure(self, c: "capi.DiTConfigF", cfg, max_tokens: int) -> None:
        """backbone keys -> the engine config's model fields (variant, widths, heads, max_tokens); the subclass hook of the constructor"""
        ratio = _get(cfg, "spatial_mlp_ratio", None)
        variant = _get(cfg, "variant", "full")
        if variant == "full":  # DiT3D (dit3d.yaml)
            if _get(cfg, "pos_emb_type", "rope_3d") != "rope_3d":
                raise ValueError("DiT3DTrainer builds the 'full' DiT3D with pos_emb_type='rope_3d'")
            c.variant, c.hidden_size, c.max_tokens = 0, int(_get(cfg, "hidden_size")), max_tokens
        elif variant == "factorized_matrix_attention" and _get(cfg, "use_temporal_rope", False):
            # dit3d_factorized_matrix.yaml (FacMatDiT) shares variant and pos_emb_type with the difference model; building that one
            # instead would double the tokens and drop the RoPE
            raise ValueError("no training path for DiT variant 'factorized_matrix_attention' with use_temporal_rope (FacMatDiT): it is inference only")
        elif variant == "factorized_matrix_attention":  # DifferenceDiT3D (bash/k600): as dit_backbone.DifferenceDiT3D._configure
            if _get(cfg, "pos_emb_type") != "sinusoidal_2d" or _get(cfg, "merge_type", "interleaved") != "interleaved":
                raise ValueError("the difference model trains with pos_emb_type='sinusoidal_2d' and merge_type='interleaved'")
            if _get(cfg, "matrix_block", "matrix") != "matrix" or _get(cfg, "matrix_multi_token", False) or _get(cfg, "fixed_u", None):
                raise ValueError("only matrix_block='matrix' with learned factors and multi_token=False is supported")
            if ratio is None:
                raise AssertionError("spatial_mlp_ratio must be specified for matrix attention")
            tratio = _get(cfg, "mlp_ratio", None)
            c.variant, c.hidden_size, c.max_tokens = 1, int(_get(cfg, "embed_row_dim")), 2 * max_tokens
            c.embed_col_dim = int(_get(cfg, "embed_col_dim"))
            c.num_col_heads, c.num_row_heads = int(_get(cfg, "num_col_heads")), int(_get(cfg, "num_row_heads"))
            c.temporal_mlp_hidden = int(c.hidden_size * tratio) if tratio else 0
            c.use_bias = int(bool(_get(cfg, "use_bias")))
        else:
            raise ValueError(f"no training path for DiT variant {variant!r}")
        c.mlp_hidden = int(c.hidden_size * ratio) if ratio else 0

    def _create(self, c: "capi.DiTConfigF") -> None:
        """the engine handle of the configured model; the other subclass hook"""
        capi.check(capi.lib.dfot_dit_train_create_f(C.byref(c), C.byref(self._handle)))

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h:
            self._engine("destroy")(h)
            self._handle = None

    # ------------------------------------------------------------------ parameters (reference state_dict names)
    def _load_buffers(self) -> None:
        for k, t in self.buffers.items():
            capi.check(self._engine("load_buffer")(self._handle, k.encode(), capi.ptr(t, torch.float32, k), t.numel(), capi.stream_ptr()))

    def load_state_dict(self, state: Dict[str, torch.Tensor], strict: bool = True) -> None:
        missing = [k for k in (*self.buffers, *self.layout) if k not in state]
        extra = [k for k in state if k not in self.layout and k not in self.buffers]
        if strict and (missing or extra):
            raise KeyError(f"state_dict mismatch: missing {missing[:4]}, unexpected {extra[:4]}")
        for k in self.buffers:
            if k in state:
                if tuple(state[k].shape) != tuple(self.buffers[k].shape):
                    raise ValueError(f"{k}: shape {tuple(state[k].shape)} != {tuple(self.buffers[k].shape)}")
                self.buffers[k].copy_(state[k].to(device="cuda", dtype=torch.float32))
        self._load_buffers()
        for k in self.layout:
            if k in state:
                t = state[k]
                if tuple(t.shape) != self.layout[k][1]:
                    raise ValueError(f"{k}: shape {tuple(t.shape)} != {self.layout[k][1]}")
                self.view(k).copy_(t.to(device="cuda", dtype=torch.float32))
        self._dirty = True

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {**{k: t.detach().clone() for k, t in self.buffers.items()}, **{k: self.view(k).detach().clone() for k in self.layout}}

    def grad_dict(self) -> Dict[str, torch.Tensor]:
        return {k: self.view(k, self.grads).detach().clone() for k in self.layout}

    def _sync(self) -> None:
        if self._dirty:
            capi.check(self._engine("sync_weights")(self._handle, capi.stream_ptr()))
            self._dirty = False

    # ------------------------------------------------------------------ forward / backward (the autograd pair)
    def forward(self, x: torch.Tensor, noise_levels: torch.Tensor, cond: Optional[torch.Tensor] = None,
                cond_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """cond: fp32 actions (B, T, cond_dim) or int32 labels (B, T) per (video, token) (dit_backbone.condition_tensors); cond_mask:
        uint8 (B,), the videos whose condition embedding is dropped"""
        b, t = x.shape[:2]
        if tuple(x.shape[2:]) != self.x_shape:
            raise ValueError(f"x has frame shape {tuple(x.shape[2:])}, expected {self.x_shape}")
        self._prepare(b)
        xd = x.to(device="cuda", dtype=torch.float32).contiguous()
        if self.is_continuous != bool(noise_levels.is_floating_point()):
            raise TypeError("a continuous-diffusion trainer takes floating noise levels (precond_scale * logsnr)" if self.is_continuous
                            else "DiT3DTrainer takes integer noise levels (DiscreteDiffusion passes the level index)")
        lv = noise_levels.to(device="cuda", dtype=torch.float32 if self.is_continuous else torch.int32).contiguous()
        out = torch.empty_like(xd)
        pc = pl = pm = None
        if cond is not None:
            action = self._ccfg.cond_type == capi.COND_ACTION
            if self._ccfg.cond_type == capi.COND_NONE:
                raise ValueError("this trainer was built without an external condition embedding")
            want = (b, t, int(self._ccfg.cond_dim)) if action else (b, t)
            if tuple(cond.shape) != want or (cond_mask is not None and tuple(cond_mask.shape) != (b,)):
                raise ValueError(f"condition has shape {tuple(cond.shape)}, expected {want} (mask {(b,)})")
            cd = cond.to(device="cuda", dtype=torch.float32 if action else torch.int32).contiguous()
            md = None if cond_mask is None else cond_mask.to(device="cuda", dtype=torch.uint8).contiguous()
            pc, pl, pm = (capi.ptr(cd) if action else None), (None if action else capi.ptr(cd)), capi.ptr(md)
        lib, h, s = capi.lib, self._handle, capi.stream_ptr()
        if self.is_continuous:
            capi.check(lib.dfot_dit_train_forward_f(h, capi.ptr(xd), capi.ptr(lv), pc, pl, pm, capi.ptr(out), b, t, s))
        elif cond is None:
            capi.check(lib.dfot_dit_train_forward(h, capi.ptr(xd), capi.ptr(lv), capi.ptr(out), b, t, s))
        else:
            capi.check(lib.dfot_dit_train_forward_cond(h, capi.ptr(xd), capi.ptr(lv), pc, pl, pm, capi.ptr(out), b, t, s))
        self._keep = (xd, lv)  # the engine reads x again in backward (patch-embedding gradient)
        return out

    def capture_attention(self, *args, **kwargs) -> None:
        """attention maps are a read-out of the inference engine (DiT3D.capture_attention); the training handles do not form them"""
        raise NotImplementedError(f"capture_attention: {type(self).__name__} is a training engine; attention maps are captured on the "
                                  "inference model (DiT3D.capture_attention) with the same weights")

    def _prepare(self, b: int) -> None:
        """workspace for a batch of b and current compute weights"""
        if b > self._reserved:
            capi.check(self._engine("reserve")(self._handle, b))
            self._reserved = b
        self._sync()

    def backward(self, d_out: torch.Tensor) -> None:
        g = d_out.to(device="cuda", dtype=torch.float32).contiguous()
        capi.check(self._engine("backward")(self._handle, capi.ptr(g), capi.stream_ptr()))

    def input_grad(self) -> torch.Tensor:
        """d(sum(out * d_out)) / d x of the last forward / backward pair, in x's layout (reconstruction guidance, discrete_diffusion.py:485-513)"""
        dx = torch.empty_like(self._keep[0])
        capi.check(self._engine("input_grad")(self._handle, capi.ptr(dx), capi.stream_ptr()))
        return dx

    # ------------------------------------------------------------------ one training step
    def _condition(self, conditions: Optional[torch.Tensor], b: int, t: int, generator: Optional[torch.Generator]):
        """conditions as the reference's training_step passes them to the model -> (cond, per-video dropout mask) of forward().  Dropout
        (cfg.external_cond_dropout > 0) is drawn per video from `generator` (a CUDA generator; None: the default one): action embeddings of
        dropped videos are zeroed (RandomEmbeddingDropout), labels of dropped videos index the null-class row (LabelEmbedding.token_drop)."""
        if conditions is None:
            return None, None
        from .dit_backbone import condition_tensors
        cond, labels = condition_tensors(self._ccfg, conditions.to("cuda"), b, t, self._ccfg.variant == 1)
        drop = None
        if self.external_cond_dropout > 0:
            drop = torch.rand(b, device="cuda", generator=generator) < self.external_cond_dropout
        if labels is not None:
            if drop is not None:
                labels = torch.where(drop[:, None], torch.full_like(labels, int(self._ccfg.num_classes)), labels)
            return labels, None
        return cond, None if drop is None else drop.to(torch.uint8)

    def loss_and_grads(self, xs: torch.Tensor, k: torch.Tensor, noise: torch.Tensor, masks: Optional[torch.Tensor] = None,
                       conditions: Optional[torch.Tensor] = None, dropout_generator: Optional[torch.Generator] = None):
        """DiscreteDiffusion.forward (pred_v; k: integer levels) or, in a continuous-diffusion trainer, ContinuousDiffusion.forward (k in
        [0, 1]) + _reweight_loss + backward (diffusion.denoising_loss): noise every token to its level, one forward, the weighted error
        averaged over (B, T) with the loss masks, gradients of every parameter.  Returns the loss (device scalar).
        conditions: the external condition of the batch (actions (B, T, dim) / labels (B, 1)), embedded as in DiT3D.forward."""
        b, t = xs.shape[:2]
        cond, cdrop = self._condition(conditions, b, t, dropout_generator)
        self.last_cond_dropout = cdrop
        _, per_token, _, dv = denoising_loss(self.schedule.cfg if self.is_continuous else self.schedule, lambda x_k, lv: self.forward(x_k, lv, cond, cdrop),
                                             xs, k, noise, masks, self.loss_weighting, want_grad=True)
        self.backward(dv)
        return masked_mean(per_token, masks)[0]

    def difference_loss_and_grads(self, frames: torch.Tensor, k: torch.Tensor, noise: torch.Tensor, masks: Optional[torch.Tensor] = None,
                                  conditions: Optional[torch.Tensor] = None, dropout_generator: Optional[torch.Generator] = None):
        """DifferenceDFoTVideo.training_step (difference_dfot_video.py:80-105): frame differences (first frame against itself) are
        interleaved with the frames (difference first), noise levels and loss masks are doubled the same way, then the ordinary
        denoising loss on the 2T merged tokens.  frames (B,T,C,H,W), k / masks (B,T), noise (B,2T,C,H,W)."""
        if self._ccfg.variant != 1:
            raise ValueError("difference_loss_and_grads needs the difference model (variant factorized_matrix_attention)")
        fr = frames.to(device="cuda", dtype=torch.float32)
        diff = torch.diff(fr, dim=1, prepend=fr[:, :1])
        merge = lambda a, b: torch.stack([a, b], dim=2).flatten(1, 2)
        kk = k.to("cuda")
        mk = None if masks is None else merge(masks.to("cuda"), masks.to("cuda"))
        cc = None if conditions is None else merge(conditions.to("cuda"), conditions.to("cuda"))  # merge_tensors(conditions, conditions)
        return self.loss_and_grads(merge(diff, fr), merge(kk, kk), noise, mk, cc, dropout_generator)

    @property
    def _hyper(self) -> Dict:
        return dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay)

    @_hyper.setter
    def _hyper(self, h: Dict) -> None:
        self.lr, self.betas, self.eps, self.weight_decay = h["lr"], h["betas"], h["eps"], h["weight_decay"]

    def optimizer_step(self, world_size: int = 1) -> None:
        """[all-reduce + average the flat gradient buffer] -> global-norm clip -> AdamW -> refresh the bf16 compute weights"""
        self.opt.step(self.lr, self.betas, self.eps, self.weight_decay, self.max_grad_norm, world_size)
        self._dirty = True

    def training_step(self, xs: torch.Tensor, k: torch.Tensor, noise: torch.Tensor, masks: Optional[torch.Tensor] = None,
                      world_size: int = 1, conditions: Optional[torch.Tensor] = None,
                      dropout_generator: Optional[torch.Generator] = None) -> torch.Tensor:
        loss = self.loss_and_grads(xs, k, noise, masks, conditions, dropout_generator)
        self.optimizer_step(world_size)
        return loss


class FacMatDiTTrainer(DiT3DTrainer):
    """Trainer of the FacMatDiT backbone: ``name: dit3d`` with ``variant: factorized_matrix_attention``, ``pos_emb_type: sinusoidal_2d``, with
    or without ``use_temporal_rope`` (dit3d_factorized_matrix.yaml + the @FacMatDiT shortcuts; the reference's bash/taichikl recipes).  Same
    constructor keywords and methods as DiT3DTrainer; max_tokens is the algorithm's (not doubled: there are no difference tokens), any
    1 <= T <= max_tokens <= 32 trains.  The matrix attention and its backward run with the RoPE-1D over the frame axis
    (csrc/attention_matrix.hip, csrc/attention_matrix_bwd.hip).  Discrete diffusion only; embed_col_dim 64 or 128.  Exactly 64 patches per
    frame (latents 4x16x16 at patch 2, the taichi res-128 facmat-s-*-bias recipes) train when the constructor gets ``allow_p64=True``;
    without the keyword the shape is refused in the words it always was.  max_tokens and T must then be even, so that a window is a whole
    number of 128-row tiles; the spatial blocks run the 64-token attention and its packed backward (csrc/attention_seq64.hip,
    csrc/attention_seq64_bwd.hip) and the gradients of the left factors qkv_u / proj_u are computed on the operands as they lie
    (csrc/facmat_factor_wgrad.hip)."""

    allow_p64 = False  # the constructor keyword; a class default, so that _configure also runs on an instance __init__ has not seen

    def __init__(self, *args, allow_p64: bool = False, **kwargs):
        self.allow_p64 = bool(allow_p64)
        super().__init__(*args, **kwargs)

    def _configure(self, c: "capi.DiTConfigF", cfg, max_tokens: int) -> None:
        from .dit_backbone import configure_facmat
        variant, pos = _get(cfg, "variant", "full"), _get(cfg, "pos_emb_type", "rope_3d")
        if variant != "factorized_matrix_attention" or pos != "sinusoidal_2d":
            raise ValueError(f"FacMatDiTTrainer builds variant='factorized_matrix_attention' with pos_emb_type='sinusoidal_2d', not "
                             f"{variant!r} / {pos!r} (DiT3DTrainer trains the 'full' DiT3D and the difference model)")
        if _get(cfg, "use_fourier_noise_embedding", False):
            raise ValueError("use_fourier_noise_embedding=True is not supported by FacMatDiTTrainer: it trains under discrete diffusion only")
        try:  # refuses matrix_multi_token, flatten_matrix_rope, fixed_u, matrix_block, patches, max_tokens by name
            configure_facmat(c, cfg, max_tokens, allow_p64=self.allow_p64)
        except ValueError as err:
            if self.allow_p64 or max_tokens % 2 or (c.height // c.patch_size) * (c.width // c.patch_size) != 64 or "patches per frame" not in str(err):
                raise
            # the refusal in the words it always had, then the way on: this shape is the one the keyword switches on
            raise ValueError(f"{err} by default: FacMatDiTTrainer(..., allow_p64=True) trains them (even max_tokens, even T)") from None

    def _create(self, c: "capi.DiTConfigF") -> None:
        # the p64 entry builds what the older one builds at a multiple of 128 patches; the older one is held to its refusal of 64
        create = capi.lib.dfot_facmat_train_create_p64 if self.allow_p64 else capi.lib.dfot_facmat_train_create
        capi.check(create(C.byref(c), C.byref(self._handle)))

    def _check_tokens(self, t: int) -> None:
        c = self._ccfg
        if (c.height // c.patch_size) * (c.width // c.patch_size) == 64 and t % 2:
            raise ValueError(f"FacMatDiTTrainer at 64 patches per frame takes an even number of tokens: {t} tokens × 64 patches = {t * 64} rows; "
                             "the row tiles need a multiple of 128")

    def forward(self, x, noise_levels, cond=None, cond_mask=None):
        self._check_tokens(int(x.shape[1]))
        return super().forward(x, noise_levels, cond, cond_mask)

    def loss_and_grads(self, xs, k, noise, masks=None, conditions=None, dropout_generator=None):
        self._check_tokens(int(xs.shape[1]))  # before the noising kernels, not only before the forward
        return super().loss_and_grads(xs, k, noise, masks, conditions, dropout_generator)


class FacDiTTrainer(DiT3DTrainer):
    """Trainer of the FacDiT backbone: ``name: dit3d`` with ``variant: factorized_attention``, ``pos_emb_type: sinusoidal_factorized``
    (dit3d_factorized_attention.yaml + the @FacDiT shortcuts; the reference's bash/taichikl train_dfot_facdit-* recipes).  Same constructor
    keywords and methods as DiT3DTrainer; ``spatial_mlp_ratio`` is the spatial blocks' MLP (0 / None: none), ``mlp_ratio`` the temporal
    blocks'; ``use_gradient_checkpointing`` is ignored (the engine keeps every activation its backward needs).  At a multiple of 128 patches
    per frame any 1 <= T <= max_tokens <= 32 trains, with the first T rows of the temporal table.  Exactly 64 patches per frame (latents
    4x16x16 at patch 2, the taichi res-128 recipes) train when the constructor gets ``allow_p64=True``; without the keyword the shape is
    refused in the words it always was, so nothing that relied on the refusal changes.  max_tokens and T must then be even, so that a
    window is a whole number of 128-row tiles; the spatial blocks run the 64-token attention and its backward (csrc/attention_seq64.hip, csrc/attention_seq64_bwd.hip, which stores
    dq | dk | dv straight into the packed gradient rows).  The temporal attention and its backward run over the frames of every patch
    position (csrc/attention_temporal.hip, csrc/attention_temporal_bwd.hip).  Discrete diffusion only."""

    allow_p64 = False  # the constructor keyword; a class default, so that _configure also runs on an instance __init__ has not seen

    def __init__(self, *args, allow_p64: bool = False, **kwargs):
        self.allow_p64 = bool(allow_p64)
        super().__init__(*args, **kwargs)

    def _configure(self, c: "capi.DiTConfigF", cfg, max_tokens: int) -> None:
        from .dit_backbone import configure_fac
        variant, pos = _get(cfg, "variant", "full"), _get(cfg, "pos_emb_type", "rope_3d")
        if variant != "factorized_attention" or pos != "sinusoidal_factorized":
            raise ValueError(f"FacDiTTrainer builds variant='factorized_attention' with pos_emb_type='sinusoidal_factorized', not "
                             f"{variant!r} / {pos!r} (DiT3DTrainer trains the 'full' DiT3D and the difference model, FacMatDiTTrainer the "
                             "factorized-matrix DiT3D)")
        if _get(cfg, "use_fourier_noise_embedding", False):
            raise ValueError("use_fourier_noise_embedding=True is not supported by FacDiTTrainer: it trains under discrete diffusion only")
        try:
            configure_fac(c, cfg, max_tokens, allow_p64=self.allow_p64)  # refuses the patch count and max_tokens by name, as DiT3D does
        except ValueError as err:
            if self.allow_p64 or max_tokens % 2 or (c.height // c.patch_size) * (c.width // c.patch_size) != 64:
                raise
            # the refusal in the words it always had, then the way on: this shape is the one the keyword switches on
            raise ValueError(f"{err} by default: FacDiTTrainer(..., allow_p64=True) trains them (even max_tokens, even T)") from None

    def _create(self, c: "capi.DiTConfigF") -> None:
        capi.check(capi.lib.dfot_facdit_train_create(C.byref(c), C.byref(self._handle)))

    def _check_tokens(self, t: int) -> None:
        c = self._ccfg
        if (c.height // c.patch_size) * (c.width // c.patch_size) == 64 and t % 2:
            raise ValueError(f"FacDiTTrainer at 64 patches per frame takes an even number of tokens: {t} tokens × 64 patches = {t * 64} rows; "
                             "the row tiles need a multiple of 128")

    def forward(self, x, noise_levels, cond=None, cond_mask=None):
        self._check_tokens(int(x.shape[1]))
        return super().forward(x, noise_levels, cond, cond_mask)

    def loss_and_grads(self, xs, k, noise, masks=None, conditions=None, dropout_generator=None):
        self._check_tokens(int(xs.shape[1]))  # before the noising kernels, not only before the forward
        return super().loss_and_grads(xs, k, noise, masks, conditions, dropout_generator)
