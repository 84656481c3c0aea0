"""Drop-in DiT3D backbone (the reference's Kinetics-600 model) backed by libdfot_hip.so.

Mirrors the reference's plugin contract for this path:
  * constructor keywords of DiscreteDiffusion._build_model (algorithms/dfot/diffusion/discrete_diffusion.py:64-92)
    and DiT3D.__init__ (algorithms/dfot/backbones/dit/dit3d.py:13-83): variant "full" with pos_emb_type "rope_3d", and variant
    "factorized_attention" with pos_emb_type "sinusoidal_factorized" (spatial + temporal blocks; trained by trainer.FacDiTTrainer), and variant
    "factorized_matrix_attention" with pos_emb_type "sinusoidal_2d" (FacMatDiT: spatial + matrix blocks, RoPE-1D over the frames; inference only),
    external condition "action" / "label" (base_backbone.py:42-62), causal masking rejected exactly as the reference does;
  * ``forward(x, noise_levels, external_cond=None, external_cond_mask=None)`` (dit3d.py:146-192) with integer
    ``noise_levels`` -- the level index DiscreteDiffusion.model_predictions passes (discrete_diffusion.py:173-174);
  * state-dict key names / shapes / order of the reference module, so its checkpoints load with ``load_state_dict``.
Parameters live here as fp32 ``nn.Parameter``s; the C library keeps packed bf16 copies and a per-level modulation table
that are rebuilt whenever a parameter changes.

With ``use_fourier_noise_embedding: true`` (``@diffusion/continuous``, base_backbone.py:35-39) the model runs under ContinuousDiffusion:
``noise_levels`` are floating ``precond_scale * logsnr`` values, ``noise_level_pos_embedding.timesteps.{freqs,phases}`` are persistent
buffers (FourierEmbedding, embeddings.py:94-109) and no per-level table exists: the embedding is evaluated per frame in every forward.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict
from typing import Optional, Sequence, Tuple, Union

import torch

from . import capi, ops
from .engine_module import EngineModule, _get


# FourierEmbedding's persistent buffers, in the reference's state_dict order (before noise_level_pos_embedding.embedding.*)
FOURIER_BUFFERS = ("noise_level_pos_embedding.timesteps.freqs", "noise_level_pos_embedding.timesteps.phases")


def configure_condition(c: "capi.DiTConfig", cfg, external_cond_type, external_cond_num_classes, external_cond_dim) -> None:
    """BaseBackbone._build_external_cond_embedding (base_backbone.py:42-62) -> the engine's condition fields."""
    c.cond_type, c.cond_dim, c.num_classes, c.cond_dropout = capi.COND_NONE, 0, 0, 0
    if not external_cond_dim:
        return
    c.cond_dropout = int(float(_get(cfg, "external_cond_dropout", 0.0) or 0.0) > 0)
    if external_cond_type == "label":
        if not external_cond_num_classes or int(external_cond_num_classes) <= 0:
            raise ValueError("external_cond_type='label' needs external_cond_num_classes")
        c.cond_type, c.num_classes = capi.COND_LABEL, int(external_cond_num_classes)
    elif external_cond_type == "action":
        c.cond_type, c.cond_dim = capi.COND_ACTION, int(external_cond_dim)
    else:
        raise ValueError(f"Unknown external condition type: {external_cond_type}. Supported types are 'label' and 'action'.")


def condition_tensors(c: "capi.DiTConfig", external_cond: torch.Tensor, batch: int, tokens: int, difference: bool):
    """external_cond as the reference's forward consumes it -> what the engine takes: (cond fp32 [B,T,cond_dim] | None, labels int32 [B,T] | None).
    label, DiT3D: (B, 1) or (B, T) class ids, broadcast over the tokens as ``emb + cond_emb`` does (dit3d.py:171-173);
    label, DifferenceDiT3D: (B, 2), each repeated over T/2 tokens (``repeat(cond_emb, "b two d -> b (two p) d")``, difference_dit3d.py:203-206)."""
    if c.cond_type == capi.COND_ACTION:
        if tuple(external_cond.shape) != (batch, tokens, c.cond_dim):
            raise ValueError(f"external_cond has shape {tuple(external_cond.shape)}, expected {(batch, tokens, int(c.cond_dim))}")
        return external_cond.detach().to(torch.float32).contiguous(), None
    lab = external_cond.detach().long()
    if difference:
        if tuple(lab.shape) != (batch, 2):
            raise ValueError(f"external_cond (labels) has shape {tuple(lab.shape)}, expected {(batch, 2)}")
        lab = lab.repeat_interleave(tokens // 2, dim=1)
    else:
        if lab.ndim != 2 or lab.shape[0] != batch or lab.shape[1] not in (1, tokens):
            raise ValueError(f"external_cond (labels) has shape {tuple(lab.shape)}, expected {(batch, 1)} or {(batch, tokens)}")
        lab = lab.expand(batch, tokens)
    return None, lab.to(torch.int32).contiguous()


def _check_patches(variant: str, c: "capi.DiTConfig", max_tokens: int, allow_p64: bool, what: str) -> None:
    """the patch-count rule of the two factorized variants: a multiple of 128 per frame, or (inference only: allow_p64) exactly 64 with an
    even max_tokens, so that a full window is a whole number of 128-row tiles (csrc/attention_seq64.hip runs the 64-token frames).  The
    trainers (allow_p64 False) refuse 64 patches in the words they always had; at an odd max_tokens the inference class refuses in the
    same words plus the rule it broke, and so do the trainers: one message for one configuration."""
    patches = (c.height // c.patch_size) * (c.width // c.patch_size)
    if patches == 64 and allow_p64 and max_tokens % 2 == 0:
        return
    if patches % 128 != 0:
        msg = (f"variant '{variant}': x_shape {(c.in_channels, c.height, c.width)} with patch_size {c.patch_size} gives {patches} patches per "
               f"frame; the {what} need a multiple of 128 ")
        if patches == 64 and max_tokens % 2:
            msg += (f"(the 64-patch recipes are not supported) in training; inference takes 64 patches with an even max_tokens only: max_tokens "
                    f"{max_tokens} × 64 patches per frame = {max_tokens * 64} rows per window; the row tiles need a multiple of 128")
        elif allow_p64:
            msg += "(or exactly 64 with an even max_tokens)"
        else:
            msg += "(the 64-patch recipes are not supported)"
        raise ValueError(msg)


def configure_facmat(c: "capi.DiTConfig", cfg, max_tokens: int, allow_p64: bool = False) -> None:
    """dit3d_factorized_matrix.yaml (+ the @FacMatDiT shortcuts) -> engine variant 3: per depth a per-frame spatial DiTBlock (num_heads,
    spatial_mlp_ratio) and a MatrixDiTBlock (embed_col_dim x embed_row_dim, num_col_heads x num_row_heads, mlp_ratio, use_bias) whose
    attention rotates q and k with a RoPE-1D over the frame axis when use_temporal_rope is set (dit_base.py:197-226, 297-306;
    dit_blocks.py:289-342).  c.patch_size / height / width are already set.  Every unsupported key is refused by name."""
    if _get(cfg, "matrix_block", "matrix") not in (None, "matrix"):
        raise ValueError(f"matrix_block={_get(cfg, 'matrix_block')!r} is not supported: only matrix_block='matrix'")
    if _get(cfg, "matrix_multi_token", False):
        raise ValueError("matrix_multi_token=True is not supported: every frame is one token of the matrix attention")
    rope = bool(_get(cfg, "use_temporal_rope", False))
    if rope and _get(cfg, "flatten_matrix_rope", False):
        raise ValueError("flatten_matrix_rope=True is not supported: the temporal RoPE rotates every row of the head matrix on its own")
    if _get(cfg, "fixed_u", None):
        raise ValueError(f"fixed_u={_get(cfg, 'fixed_u')!r} is not supported: the left factors qkv_u / proj_u are learned parameters")
    ratio, tratio = _get(cfg, "spatial_mlp_ratio", None), _get(cfg, "mlp_ratio", None)
    if ratio is None:
        raise AssertionError("spatial_mlp_ratio must be specified for matrix attention")
    if _get(cfg, "use_bias", None) is None:
        raise AssertionError("use_bias must be specified for matrix attention")
    _check_patches("factorized_matrix_attention", c, max_tokens, allow_p64, "per-frame kernels")
    if max_tokens > 32:
        raise ValueError(f"variant 'factorized_matrix_attention': max_tokens {max_tokens} exceeds the matrix attention kernel's 32 frames")
    c.hidden_size = int(_get(cfg, "embed_row_dim"))
    c.max_tokens = max_tokens
    c.mlp_hidden = int(c.hidden_size * ratio) if ratio else 0
    c.variant = 3
    c.embed_col_dim = int(_get(cfg, "embed_col_dim"))
    c.num_col_heads = int(_get(cfg, "num_col_heads"))
    c.num_row_heads = int(_get(cfg, "num_row_heads"))
    c.temporal_mlp_hidden = int(c.hidden_size * tratio) if tratio else 0
    c.use_bias = int(bool(_get(cfg, "use_bias")))
    c.use_temporal_rope = int(rope)


def configure_fac(c: "capi.DiTConfig", cfg, max_tokens: int, allow_p64: bool = False) -> None:
    """dit3d_factorized_attention.yaml (+ the @FacDiT shortcuts) -> engine variant 2: per depth a per-frame spatial DiTBlock
    (spatial_mlp_ratio) and a temporal DiTBlock (mlp_ratio) over the frames of every patch position (dit_base.py:197-226, 364-417).
    c.patch_size / height / width are already set.  Shared by DiT3D and trainer.FacDiTTrainer."""
    ratio, tratio = _get(cfg, "spatial_mlp_ratio", None), _get(cfg, "mlp_ratio", 4.0)
    c.hidden_size = int(_get(cfg, "hidden_size"))
    c.max_tokens = max_tokens
    c.mlp_hidden = int(c.hidden_size * ratio) if ratio else 0
    c.variant = 2
    c.temporal_mlp_hidden = int(c.hidden_size * tratio) if tratio else 0
    _check_patches("factorized_attention", c, max_tokens, allow_p64, "per-frame attention kernels")
    if max_tokens > 32:
        raise ValueError(f"variant 'factorized_attention': max_tokens {max_tokens} exceeds the temporal attention kernel's 32 frames")


def _init_random_matrix(tensors, seed: int) -> None:
    """init_random of the models with matrix blocks: as DiT3D.init_random; the matrix factors are (in, out) matrices (fan-in = rows), their
    biases ~ N(0, 0.05^2)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in tensors.items():
            leaf = name.rsplit(".", 1)[-1]
            if leaf in ("bias", "qkv_bias", "proj_bias"):
                v = 0.05 * torch.randn(t.shape, generator=g)
            elif leaf in ("qkv_u", "proj_u", "qkv_v", "proj_v"):
                v = torch.randn(t.shape, generator=g) / math.sqrt(t.shape[0])
            elif name.startswith("diff_embedder"):
                v = 0.3 * torch.randn(t.shape, generator=g)
            else:
                gain = 0.5 if ".modulation." in name else 1.0
                v = gain * torch.randn(t.shape, generator=g) / math.sqrt(math.prod(t.shape[1:]))
            t.copy_(v.to(t.device))


class DiT3D(EngineModule):
    _family, _create = "dit", "dfot_dit_create_f"

    def __init__(self, cfg, x_shape: Sequence[int], max_tokens: int, external_cond_type: str = "action",
                 external_cond_num_classes: Optional[int] = None, external_cond_dim: int = 0,
                 use_causal_mask: bool = False, timesteps: int = 1000, **kwargs):
        if use_causal_mask:
            raise NotImplementedError("Causal masking is not yet implemented for DiT3D backbone")
        super().__init__()
        self.cfg = cfg
        self.x_shape = tuple(int(v) for v in x_shape)
        self.external_cond_type = external_cond_type
        self.external_cond_num_classes = external_cond_num_classes
        self.external_cond_dim = int(external_cond_dim or 0)
        self.external_cond_dropout = float(_get(cfg, "external_cond_dropout", 0.0) or 0.0) if self.external_cond_dim else 0.0
        self.use_causal_mask = False
        self.patch_size = int(_get(cfg, "patch_size", 2))
        c = capi.DiTConfigF()
        c.depth = int(_get(cfg, "depth"))
        c.num_heads = int(_get(cfg, "num_heads"))
        c.patch_size = self.patch_size
        c.in_channels, c.height, c.width = self.x_shape
        c.noise_dim = 256
        c.timesteps = int(timesteps)
        c.rope_theta = 10000.0
        c.eps = 1e-6
        configure_condition(c, cfg, external_cond_type, external_cond_num_classes, self.external_cond_dim)
        self.use_fourier_noise_embedding = bool(_get(cfg, "use_fourier_noise_embedding", False))
        c.fourier_noise = int(self.use_fourier_noise_embedding)
        self._configure(c, cfg, int(max_tokens))
        self.hidden_size = int(c.hidden_size)
        self.max_tokens = int(c.max_tokens)
        self._ccfg = c
        self.num_patches = (c.height // c.patch_size) * (c.width // c.patch_size)
        self._build_tree()
        # training form (autograd): the saved-activation engine of trainer.DiT3DTrainer, built at the first forward under grad
        self._ctor = dict(max_tokens=int(max_tokens), timesteps=int(timesteps), external_cond_type=external_cond_type,
                          external_cond_num_classes=external_cond_num_classes, external_cond_dim=self.external_cond_dim)
        # training-time dropout of the condition embedding, per video (RandomEmbeddingDropout: torch.rand(emb.shape[:1]) < p): drawn from
        # this generator (None: the default CUDA generator) so that a run is reproducible
        self._dropout_generator: Optional[torch.Generator] = None
        self._trainer = None
        self._trainer_sig = None
        self._train_stamp = 0  # counts training forwards (see backbone.UViT3DPose._train_backward_impl)
        self._train_names = [n for n, _ in self.named_parameters()]
        self._capture_names: Tuple[str, ...] = ()  # attention-map capture: the selected module names, in block order; () = off

    def _configure(self, c: "capi.DiTConfig", cfg, max_tokens: int) -> None:
        """dit3d.yaml / dit3d_factorized_attention.yaml / dit3d_factorized_matrix.yaml keys -> engine config (variant 0 / 2 / 3)."""
        variant = _get(cfg, "variant", "full")
        pos = _get(cfg, "pos_emb_type", "rope_3d")
        supported = "DiT3D builds variant='full' with pos_emb_type='rope_3d', variant='factorized_attention' with " \
                    "pos_emb_type='sinusoidal_factorized' (see DifferenceDiT3D for 'factorized_matrix_attention' over difference tokens), " \
                    "and variant='factorized_matrix_attention' with pos_emb_type='sinusoidal_2d'"
        want_pos = {"full": "rope_3d", "factorized_attention": "sinusoidal_factorized", "factorized_matrix_attention": "sinusoidal_2d"}
        if variant not in want_pos:
            raise ValueError(f"unsupported DiT variant {variant!r}: {supported}")
        if pos != want_pos[variant]:
            raise ValueError(f"unsupported pos_emb_type {pos!r} for variant {variant!r}: {supported}")
        ratio = _get(cfg, "spatial_mlp_ratio", None)
        if variant == "factorized_matrix_attention":
            configure_facmat(c, cfg, max_tokens, allow_p64=True)
            return
        if variant == "factorized_attention":
            configure_fac(c, cfg, max_tokens, allow_p64=True)
            return
        c.hidden_size = int(_get(cfg, "hidden_size"))
        c.max_tokens = max_tokens
        c.mlp_hidden = int(c.hidden_size * ratio) if ratio else 0
        c.variant = 0

    @property
    def in_channels(self) -> int:
        return self.x_shape[0]

    @property
    def noise_level_dim(self) -> int:
        return 256

    def _new_tensor(self, name: str, shape: Tuple[int, ...]) -> torch.Tensor:
        if name == FOURIER_BUFFERS[0]:  # drawn as FourierEmbedding.__init__ draws them (bandwidth 1), from torch's default generator
            return 2 * math.pi * torch.randn(shape)
        if name == FOURIER_BUFFERS[1]:
            return 2 * math.pi * torch.rand(shape)
        return super()._new_tensor(name, shape)

    def reset_parameters(self, seed: int = 0) -> None:
        """The reference's init (dit3d.py:92-109, dit_blocks.py:392-395,422-425,476-486,528-531): xavier-uniform Linear
        weights, N(0, 0.02) embedding MLP, zero biases, zero modulations and zero final projection."""
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, t in self._tensors().items():
                if name.endswith(("bias", "qkv_bias", "proj_bias")) or ".modulation." in name or name.startswith("dit_base.final_layer.linear"):
                    t.zero_()
                elif name.startswith(("noise_level_pos_embedding", "diff_embedder", "external_cond_embedding")):  # _mlp_init (dit3d.py:98-107)
                    t.copy_(0.02 * torch.randn(t.shape, generator=g))
                else:
                    fan_out, fan_in = t.shape[0], math.prod(t.shape[1:])
                    bound = math.sqrt(6.0 / (fan_in + fan_out))
                    t.copy_((torch.rand(t.shape, generator=g) * 2 - 1) * bound)

    def init_random(self, seed: int = 0) -> None:
        """Non-degenerate random weights for benchmarks (the reference zero-inits every modulation and the final
        projection, which makes the output identically zero): weights ~ N(0, 1/fan_in) (modulations at half gain),
        biases ~ N(0, 0.05^2) -- the distribution of oracle.dit.seeded_params."""
        if self._ccfg.variant == 3:
            return _init_random_matrix(self._tensors(), seed)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, t in self._tensors().items():
                if name.endswith(".bias"):
                    v = 0.05 * torch.randn(t.shape, generator=g)
                else:
                    gain = 0.5 if ".modulation." in name else 1.0
                    v = gain * torch.randn(t.shape, generator=g) / math.sqrt(math.prod(t.shape[1:]))
                t.copy_(v.to(t.device))

    def attn_timing(self):
        tot, n = C.c_double(), C.c_int64()
        capi.check(capi.lib.dfot_dit_attn_timing(self._handle, C.byref(tot), C.byref(n)))
        return tot.value, n.value

    def reserve(self, batch: int) -> None:
        try:
            super().reserve(batch)
        except capi.DfotError as e:
            if self._capture_names and e.code == capi.ERR_SHAPE:  # the captured maps at this batch exceed max_bytes
                raise ValueError(str(e)) from None
            raise

    def _condition_mask(self, external_cond_mask: Optional[torch.Tensor], batch: int, dev) -> Optional[torch.Tensor]:
        """which videos run without their condition, as the reference's modules decide it: an action model built with
        external_cond_dropout == 0 IS a TimestepEmbedding and never sees the mask (embeddings.py:377-378,385-386); with dropout > 0 the
        mask zeroes the embedding in eval() and a fresh per-video draw does in train() (a mask is refused there, as the reference asserts);
        label models never receive the mask (dit3d.py:171-173)."""
        if self._ccfg.cond_type != capi.COND_ACTION or self.external_cond_dropout <= 0:
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

    def _labels_with_dropout(self, labels: torch.Tensor) -> torch.Tensor:
        """LabelEmbedding.token_drop in train(): the labels of dropped videos index the extra (null class) row"""
        if self.training and self.external_cond_dropout > 0:
            drop = torch.rand(labels.shape[0], device=labels.device, generator=self._dropout_generator) < self.external_cond_dropout
            labels = torch.where(drop[:, None], torch.full_like(labels, int(self._ccfg.num_classes)), labels)
        return labels

    def forward(self, x: torch.Tensor, noise_levels: torch.Tensor, external_cond: Optional[torch.Tensor] = None,
                external_cond_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """BaseBackbone.forward; dispatched as the torch operators ``dfot::dit3d_forward`` / ``dfot::dit3d_forward_cond`` (ops.py)."""
        if external_cond is not None and self._ccfg.cond_type == capi.COND_NONE:
            raise ValueError("this DiT3D was built without an external condition embedding")
        if self._op_key is None:
            self._op_key = ops.register_model(self)
        params = [p for _, p in self.named_parameters()]
        train = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        if train and self._ccfg.variant in (2, 3):
            name = "factorized_attention" if self._ccfg.variant == 2 else "factorized_matrix_attention"
            raise NotImplementedError(f"variant {name!r} is inference only: there is no training path and no input gradient "
                                      "(reconstruction guidance); call it under torch.no_grad() / with parameters that do not require grad")
        c = mask = None
        if external_cond is not None:
            b, t = x.shape[:2]
            cond, labels = condition_tensors(self._ccfg, external_cond, b, t, self._ccfg.variant == 1)
            mask = self._condition_mask(external_cond_mask, b, x.device)
            if labels is not None:
                labels = self._labels_with_dropout(labels)
            c = cond if cond is not None else labels
        if self.use_fourier_noise_embedding:  # float levels (ContinuousDiffusion): one operator pair, the condition optional
            if train:
                return torch.ops.dfot.dit3d_forward_f_train(x, noise_levels, c, mask, params, self._op_key)
            return torch.ops.dfot.dit3d_forward_f(x, noise_levels, c, mask, self._op_key)
        if external_cond is not None:
            if train:
                return torch.ops.dfot.dit3d_forward_cond_train(x, noise_levels, c, mask, params, self._op_key)
            return torch.ops.dfot.dit3d_forward_cond(x, noise_levels, c, mask, self._op_key)
        if train:
            # the reference's training_step differentiates through `self.model(...)` (discrete_diffusion.py model_predictions ->
            # accelerator.backward): saved-activation forward + the hand-written backward, registered with autograd (ops.py)
            return torch.ops.dfot.dit3d_forward_train(x, noise_levels, params, self._op_key)
        return torch.ops.dfot.dit3d_forward(x, noise_levels, self._op_key)

    # ------------------------------------------------------------------ training form (autograd)
    def _train_engine(self, params):
        """trainer.DiT3DTrainer on the module's CURRENT weights: built once; its flat parameter buffer is refreshed (and the bf16
        compute copies re-packed) whenever a parameter changed since the last training forward."""
        from . import trainer as _trainer
        from .diffusion import DiffusionConfig
        buffers = dict(self.named_buffers())
        sig = tuple((t.data_ptr(), t._version) for t in (*params, *buffers.values()))
        if self._trainer is None:
            self._trainer = _trainer.DiT3DTrainer(self.cfg, self.x_shape, self._ctor["max_tokens"], timesteps=self._ctor["timesteps"],
                                                  external_cond_type=self._ctor["external_cond_type"],
                                                  external_cond_num_classes=self._ctor["external_cond_num_classes"],
                                                  external_cond_dim=self._ctor["external_cond_dim"],
                                                  diffusion=DiffusionConfig(is_continuous=True) if self.use_fourier_noise_embedding else None)
            missing = [n for n in self._trainer.layout if n not in self._train_names]
            if missing:
                raise RuntimeError(f"the training engine expects parameters the module does not have: {missing[:4]}")
        if sig != self._trainer_sig:
            with torch.no_grad():
                self._trainer.load_state_dict({**{n: t for n, t in zip(self._train_names, params) if n in self._trainer.layout}, **buffers})
            self._trainer_sig = sig
        return self._trainer

    def _check_level_dtype(self, noise_levels: torch.Tensor) -> None:
        if self.use_fourier_noise_embedding:
            if not noise_levels.is_floating_point():
                raise TypeError("this DiT3D was built with use_fourier_noise_embedding: it takes floating noise levels "
                                "(ContinuousDiffusion passes precond_scale * logsnr)")
        elif noise_levels.is_floating_point():
            raise TypeError("DiT3D takes integer noise levels (DiscreteDiffusion passes the level index)")

    def _train_forward_impl(self, x, noise_levels, params, cond=None, cond_mask=None):
        if x.ndim != 5 or tuple(x.shape[2:]) != self.x_shape:
            raise ValueError(f"x has shape {tuple(x.shape)}, expected (B, T, {', '.join(map(str, self.x_shape))})")
        if x.shape[1] > self.max_tokens:
            raise ValueError(f"{x.shape[1]} tokens exceed max_tokens={self.max_tokens}")
        if tuple(noise_levels.shape) != tuple(x.shape[:2]):
            raise ValueError(f"noise_levels has shape {tuple(noise_levels.shape)}, expected {tuple(x.shape[:2])}")
        self._check_level_dtype(noise_levels)
        dev = params[0].device
        if dev.type != "cuda":
            raise RuntimeError(f"the backbone's parameters are on {dev}; move the module to the GPU first (there is no CPU path)")
        capi.require_device(dev, x=x, noise_levels=noise_levels, external_cond=cond, external_cond_mask=cond_mask)
        self._train_stamp += 1
        with torch.no_grad():
            return self._train_engine(params).forward(x, noise_levels, cond, cond_mask).to(x.dtype)

    def _train_backward_impl(self, grad_out, params, stamp=None, want_dx=False):
        eng = self._trainer
        if eng is None:
            raise RuntimeError("backward without a training forward")
        if stamp is not None and stamp != self._train_stamp:
            raise RuntimeError(
                f"DiT3D: backward of training forward #{stamp}, but forward #{self._train_stamp} has run since and overwritten the saved "
                "activations (one engine per module). Run backward after each forward (accumulate gradients as forward/backward pairs).")
        with torch.no_grad():
            eng.backward(grad_out)
            grads = [eng.view(n, eng.grads).to(p.dtype).clone() if n in eng.layout else torch.zeros_like(p)
                     for n, p in zip(self._train_names, params)]
            if want_dx:  # reconstruction guidance differentiates the prediction w.r.t. x_t (discrete_diffusion.py:485-513)
                grads.append(eng.input_grad().to(grad_out.dtype))
            return grads

    def _forward_impl(self, x: torch.Tensor, noise_levels: torch.Tensor, cond: Optional[torch.Tensor] = None,
                      cond_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """cond: what condition_tensors returned (fp32 actions or int32 labels per (video, token)); cond_mask: uint8 (B,) or None"""
        if x.ndim != 5 or tuple(x.shape[2:]) != self.x_shape:
            raise ValueError(f"x has shape {tuple(x.shape)}, expected (B, T, {', '.join(map(str, self.x_shape))})")
        b, t = x.shape[:2]
        if t > self.max_tokens:
            raise ValueError(f"{t} tokens exceed max_tokens={self.max_tokens}")
        if tuple(noise_levels.shape) != (b, t):
            raise ValueError(f"noise_levels has shape {tuple(noise_levels.shape)}, expected {(b, t)}")
        self._check_level_dtype(noise_levels)
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError(f"the backbone's parameters are on {dev}; move the module to the GPU first (there is no CPU path)")
        capi.require_device(dev, x=x, noise_levels=noise_levels, external_cond=cond, external_cond_mask=cond_mask)
        self.sync_weights()
        self.reserve(b)
        xf = x.detach().to(torch.float32).contiguous()
        out = torch.empty_like(xf)
        if self.use_fourier_noise_embedding:
            kf = noise_levels.detach().to(torch.float32).contiguous()
            pc = pl = None
            if cond is not None:
                action = self._ccfg.cond_type == capi.COND_ACTION
                want = (b, t, int(self._ccfg.cond_dim)) if action else (b, t)
                if tuple(cond.shape) != want or (cond_mask is not None and tuple(cond_mask.shape) != (b,)):
                    raise ValueError(f"condition has shape {tuple(cond.shape)}, expected {want} (mask {(b,)})")
                pc = capi.ptr(cond, torch.float32, "external_cond") if action else None
                pl = None if action else capi.ptr(cond, torch.int32, "external_cond")
            capi.check(capi.lib.dfot_dit_forward_f(self._handle, capi.ptr(xf, torch.float32, "x"), capi.ptr(kf, torch.float32, "noise_levels"),
                                                   pc, pl, capi.ptr(cond_mask if cond is not None else None, torch.uint8, "external_cond_mask"),
                                                   capi.ptr(out), b, t, capi.stream_ptr()))
            return out.to(x.dtype)
        kf = noise_levels.detach().to(torch.int32).contiguous()
        if cond is None:
            capi.check(capi.lib.dfot_dit_forward(self._handle, capi.ptr(xf, torch.float32, "x"), capi.ptr(kf, torch.int32, "noise_levels"),
                                                 capi.ptr(out), b, t, capi.stream_ptr()))
            return out.to(x.dtype)
        action = self._ccfg.cond_type == capi.COND_ACTION
        want = (b, t, int(self._ccfg.cond_dim)) if action else (b, t)
        if tuple(cond.shape) != want or (cond_mask is not None and tuple(cond_mask.shape) != (b,)):
            raise ValueError(f"condition has shape {tuple(cond.shape)}, expected {want} (mask {(b,)})")
        pc = capi.ptr(cond, torch.float32, "external_cond") if action else None
        pl = None if action else capi.ptr(cond, torch.int32, "external_cond")
        capi.check(capi.lib.dfot_dit_forward_cond(self._handle, capi.ptr(xf, torch.float32, "x"), capi.ptr(kf, torch.int32, "noise_levels"),
                                                  pc, pl, capi.ptr(cond_mask, torch.uint8, "external_cond_mask"), capi.ptr(out), b, t,
                                                  capi.stream_ptr()))
        return out.to(x.dtype)

    def read_tap(self, name: str, rows: int) -> torch.Tensor:
        """"emb" (rows = timesteps; not on a Fourier model), "stream" (rows = B*T*P), "cond_emb" (rows = B*T of the last per-frame forward),
        "noise_feat" (rows = B*T of the last float-level forward, noise_level_dim columns)"""
        out = torch.empty(rows, self.noise_level_dim if name == "noise_feat" else self.hidden_size, device="cuda", dtype=torch.float32)
        capi.check(capi.lib.dfot_dit_read_tap(self._handle, name.encode(), capi.ptr(out), out.numel(), capi.stream_ptr()))
        return out

    # ------------------------------------------------------------------ attention maps (the reference's attn_hook)
    def attention_block_names(self) -> Tuple[str, ...]:
        """the reference's module names of the blocks whose attention mixes frames -- the keys of the hook's ``attn_maps[timestep]``:
        ``dit_base.blocks.{i}.attn`` (variant "full"), ``dit_base.temporal_blocks.{i}.attn`` (the two factorized variants)"""
        stem = "dit_base.blocks" if self._ccfg.variant == 0 else "dit_base.temporal_blocks"
        return tuple(f"{stem}.{i}.attn" for i in range(int(self._ccfg.depth)))

    def capture_attention(self, blocks: Union[None, bool, Sequence[str]] = None, form: str = "frame", max_bytes: int = 1 << 30) -> None:
        """Record, in every later forward, the attention map of the named blocks (None: every frame-mixing block); ``capture_attention(False)``
        turns it off and releases the buffers.  form "frame": per head, query frame x key frame (rows sum to 1); "full": the N x N softmax
        matrix of variant "full" (refused above ``max_bytes``); on "factorized_matrix_attention" every frame is one token and both forms are
        the (B, col heads, row heads, T, T) map.  One map launch per selected block is added to the forward; its outputs do not change.
        Not to be called while a graph is being captured: it synchronises the device and (re)allocates."""
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("capture_attention: capture settings cannot change while a graph is being captured")
        if blocks is False:
            capi.check(capi.lib.dfot_dit_capture_attention(self._handle, None, 0, capi.ATTN_MAP_OFF, 0))
            self._capture_names = ()
            self._bump_generation()  # captured graphs hold the map launches
            return
        if self._ccfg.variant == 1:
            raise NotImplementedError("capture_attention: DifferenceDiT3D (the difference model) is not supported")
        if form not in ("frame", "full"):
            raise ValueError(f"capture_attention: form {form!r} is not one of 'frame', 'full'")
        if form == "full" and self._ccfg.variant == 2:
            raise ValueError("capture_attention: form='full' is not available on variant 'factorized_attention': a temporal block has one "
                             "T x T map per patch position and only their mean, the frame map, is formed")
        names = self.attention_block_names()
        if blocks is None or blocks is True:
            chosen = list(range(len(names)))
        else:
            if isinstance(blocks, str):
                blocks = [blocks]
            chosen = []
            for b in blocks:
                if b not in names:
                    stem, _, leaf = str(b).rpartition(".")
                    if self._ccfg.variant != 0 and leaf == "attn" and stem.startswith("dit_base.blocks.") and stem[16:].isdigit() \
                            and int(stem[16:]) < len(names):
                        raise ValueError(f"capture_attention: {b!r} is a spatial block: its attention runs inside one frame and has no frame "
                                         f"axis; the frame-mixing blocks are {names[0]!r} .. {names[-1]!r}")
                    raise ValueError(f"capture_attention: unknown block {b!r}; the frame-mixing blocks are {names[0]!r} .. {names[-1]!r}")
                chosen.append(names.index(b))
            chosen = sorted(set(chosen))
        arr = (C.c_int32 * len(chosen))(*chosen)
        code = capi.ATTN_MAP_FULL if form == "full" else capi.ATTN_MAP_FRAME
        try:
            capi.check(capi.lib.dfot_dit_capture_attention(self._handle, arr, len(chosen), code, int(max_bytes)))
        except capi.DfotError as e:
            if e.code == capi.ERR_SHAPE:
                raise ValueError(str(e)) from None
            raise
        self._capture_names = tuple(names[i] for i in chosen)
        self._capture_max_bytes = int(max_bytes)
        self._bump_generation()

    @property
    def capturing_attention(self) -> bool:
        return bool(self._capture_names)

    def attention_maps(self) -> "OrderedDict[str, torch.Tensor]":
        """name -> fp32 device tensor of the last forward, in block order.  Rows follow the model batch: under History Guidance one row per
        (video, branch), in ``HistoryGuidance.prepare``'s order."""
        if not self._capture_names:
            raise RuntimeError("attention_maps: attention capture is off (call capture_attention first)")
        out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
        shape = (C.c_int64 * 5)()
        ndim = C.c_int()
        for slot, name in enumerate(self._capture_names):
            try:
                capi.check(capi.lib.dfot_dit_attention_map_shape(self._handle, slot, shape, C.byref(ndim)))
            except capi.DfotError as e:
                if e.code == capi.ERR_STATE:
                    raise RuntimeError("attention_maps: no forward has run since capture_attention was called") from None
                raise
            t = torch.empty(tuple(shape[k] for k in range(ndim.value)), device="cuda", dtype=torch.float32)
            capi.check(capi.lib.dfot_dit_read_attention_map(self._handle, slot, capi.ptr(t), t.numel(), capi.stream_ptr()))
            out[name] = t
        return out


class DifferenceDiT3D(DiT3D):
    """The bash/k600 backbone: ``difference_dit3d`` with variant ``factorized_matrix_attention`` (per-frame spatial DiT blocks
    alternating with frame-token MatrixDiT blocks), ``pos_emb_type: sinusoidal_2d``, ``merge_type: interleaved``
    (algorithms/dfot/backbones/dit/difference_dit3d.py:12-226; dit_base.py:155-226; dit_blocks.py:211-350,549-652).
    Like the reference class it doubles ``max_tokens``: ``forward`` takes the 2T interleaved (difference, frame) tokens."""

    def _configure(self, c: "capi.DiTConfig", cfg, max_tokens: int) -> None:
        if _get(cfg, "variant") != "factorized_matrix_attention":
            raise ValueError(f"unsupported DifferenceDiT3D variant {_get(cfg, 'variant')!r}: only 'factorized_matrix_attention'")
        if _get(cfg, "pos_emb_type") != "sinusoidal_2d":
            raise ValueError("only pos_emb_type='sinusoidal_2d' is supported")
        if _get(cfg, "merge_type", "interleaved") != "interleaved":
            raise ValueError("only merge_type='interleaved' is supported")
        if _get(cfg, "matrix_block", "matrix") != "matrix" or _get(cfg, "matrix_multi_token", False) or _get(cfg, "fixed_u", None):
            raise ValueError("only matrix_block='matrix' with learned factors and multi_token=False is supported")
        ratio, tratio = _get(cfg, "spatial_mlp_ratio", None), _get(cfg, "mlp_ratio", None)
        if ratio is None:
            raise AssertionError("spatial_mlp_ratio must be specified for matrix attention")
        c.hidden_size = int(_get(cfg, "embed_row_dim"))
        c.max_tokens = 2 * max_tokens  # doubling max_tokens for difference encoding
        c.mlp_hidden = int(c.hidden_size * ratio) if ratio else 0
        c.variant = 1
        c.embed_col_dim = int(_get(cfg, "embed_col_dim"))
        c.num_col_heads = int(_get(cfg, "num_col_heads"))
        c.num_row_heads = int(_get(cfg, "num_row_heads"))
        c.temporal_mlp_hidden = int(c.hidden_size * tratio) if tratio else 0
        c.use_bias = int(bool(_get(cfg, "use_bias")))

    def init_random(self, seed: int = 0) -> None:
        """As DiT3D.init_random; the matrix factors are (in, out) matrices (fan-in = rows), their biases ~ N(0, 0.05^2)."""
        _init_random_matrix(self._tensors(), seed)
