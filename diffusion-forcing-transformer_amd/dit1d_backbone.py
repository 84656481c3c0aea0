"""Drop-in DiT1D backbone (the reference's frame-causal transformer over 1-D token latents,
algorithms/dfot/backbones/dit1d/dit_model.py:358-530, configurations/algorithm/backbone/dit1d.yaml) backed by libdfot_hip.so.

Its input is ``(B, T, C, 1, L)``: per frame L one-dimensional tokens of C channels -- the ``[4, 1, 32]`` TiTok-KL latent of the taichi
recipe (``titok.TiTokEncoder`` / ``TiTokDecoder``).  It is the one backbone of the reference that sees its frames causally: a token attends
to every token of its own and of earlier frames and to none of later frames (``causal_attn_mode: temporal_causal`` /
``video_temporal_causal``, which build the same mask without context tokens; ``null`` runs without a mask).

Built: the stock configuration -- ``merge_mode: share_norm`` (whose blocks overwrite the residual stream with its LayerNorm),
``use_rotary_emb: false`` (the frozen ``pos_embed`` parameter is part of the state dict and is loaded, not recomputed), ``qk_norm: false``,
``learn_sigma: false``, no external condition (a non-zero ``external_cond_dim`` makes the reference's own constructor raise), discrete
noise levels.  Constructor keywords, ``forward`` signature and the state-dict key names / order are the reference's.  The ``pos_embed``
add fixes the sequence length: like the reference, the model runs at exactly ``max_tokens`` frames.  Forward only: under autograd it raises
NotImplementedError; training is ``dit1d_trainer.DiT1DTrainer``, whose state dict loads into this module.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch
from torch import nn

from . import capi, ops
from .engine_module import EngineModule, _get

CAUSAL_MODES = (None, "temporal_causal", "video_temporal_causal")
FRAME_LENGTHS = (16, 32, 64, 128)


def sincos_pos_embed_1d(hidden: int, tokens: int) -> torch.Tensor:
    """get_1d_sincos_pos_embed (dit_model.py:556-615): [sin | cos] halves, omega_i = 10000^(-i / (hidden/2)), positions 0 .. tokens-1 over the
    whole video; float64 like the reference's numpy, returned as float32 (1, tokens, hidden)"""
    omega = 1.0 / 10000 ** (torch.arange(hidden // 2, dtype=torch.float64) / (hidden / 2.0))
    out = torch.arange(tokens, dtype=torch.float64)[:, None] * omega[None]
    return torch.cat([out.sin(), out.cos()], dim=1).float().unsqueeze(0)


def state_dict_layout(hidden: int, depth: int, mlp_hidden: int, channels: int, tokens: int):
    """[(key, shape)] in the order DIT1D registers its parameters (dit_model.py:429-456; a module's own parameters come before its
    children's, so pos_embed is first) -- the order the engine enumerates too (checked when the engine handle is created)"""
    out = [("pos_embed", (1, tokens, hidden))]

    def linear(name, o, i):
        out.extend([(f"{name}.weight", (o, i)), (f"{name}.bias", (o,))])
    linear("x_embedder", hidden, channels)
    linear("t_embedder.mlp.0", hidden, 256)
    linear("t_embedder.mlp.2", hidden, hidden)
    for i in range(depth):
        linear(f"blocks.{i}.attn.qkv", 3 * hidden, hidden)
        linear(f"blocks.{i}.attn.proj", hidden, hidden)
        linear(f"blocks.{i}.mlp.fc1", mlp_hidden, hidden)
        linear(f"blocks.{i}.mlp.fc2", hidden, mlp_hidden)
        linear(f"blocks.{i}.adaLN_modulation.1", 6 * hidden, hidden)
    linear("final_layer.1", channels, hidden)
    return out


def check_config(cfg, x_shape: Sequence[int], max_tokens: int, external_cond_dim: int = 0, timesteps: int = 1000):
    """What DiT1D and DiT1DTrainer build, refused by name otherwise.  -> (x_shape, causal_attn_mode, engine config)"""
    merge = _get(cfg, "merge_mode", "share_norm")
    if merge != "share_norm":
        raise ValueError(f"merge_mode={merge!r} is not built: only merge_mode='share_norm' (the stock dit1d.yaml)")
    if _get(cfg, "use_rotary_emb", False):
        raise ValueError("use_rotary_emb=True is not built: the model adds the frozen pos_embed table (use_rotary_emb: false)")
    if _get(cfg, "qk_norm", False):
        raise ValueError("qk_norm=True is not built: the attention takes q and k as the projection gives them (qk_norm: false)")
    if _get(cfg, "learn_sigma", False):
        raise ValueError("learn_sigma=True is not built: the output has the input's channels (learn_sigma: false)")
    mode = _get(cfg, "causal_attn_mode", "video_temporal_causal")
    if mode not in CAUSAL_MODES:
        raise ValueError(f"causal_attn_mode={mode!r} is unknown: one of None, 'temporal_causal', 'video_temporal_causal'")
    if external_cond_dim:
        raise ValueError(f"external_cond_dim={external_cond_dim} is not built: the reference's own DiT1D constructor fails on a non-zero "
                         "external_cond_dim (external_cond_emb_dim reads self.external_cond_dim, which is never assigned); the model is "
                         "unconditioned")
    x_shape = tuple(int(v) for v in x_shape)
    if len(x_shape) != 3 or x_shape[1] != 1:
        raise ValueError(f"x_shape[1] must be 1: DiT1D takes 1-D token latents (C, 1, L), got x_shape {x_shape}")
    channels, _, length = x_shape
    if length not in FRAME_LENGTHS:
        raise ValueError(f"L = x_shape[2] = {length} tokens per frame is outside the frame-causal attention kernel's {set(FRAME_LENGTHS)}")
    max_tokens = int(max_tokens)
    if max_tokens <= 0 or (max_tokens * length) % 128 != 0:
        raise ValueError(f"max_tokens * L = {max_tokens} x {length} = {max_tokens * length} tokens per window; the attention row tiles need a "
                         "multiple of 128")
    hidden, heads = int(_get(cfg, "hidden_size")), int(_get(cfg, "num_heads"))
    if hidden <= 0 or hidden % 64 or hidden > 2048:
        raise ValueError(f"hidden_size={hidden} is outside the engine's limit: a multiple of 64, at most 2048")
    depth = int(_get(cfg, "depth"))
    if depth <= 0:
        raise ValueError(f"depth={depth} must be positive")
    mlp_hidden = int(hidden * float(_get(cfg, "mlp_ratio", 4.0)))
    if mlp_hidden <= 0 or mlp_hidden % 64:
        raise ValueError(f"mlp_ratio={_get(cfg, 'mlp_ratio', 4.0)} gives an MLP width of {mlp_hidden}; the GEMMs need a positive multiple of 64")
    if not 1 <= channels <= 64:
        raise ValueError(f"x_shape[0] = {channels} channels is outside the token embedding's 1 .. 64")
    if int(timesteps) <= 0:
        raise ValueError(f"timesteps={timesteps} must be positive")
    if heads <= 0 or hidden % heads or (hidden // heads) % 8 or hidden // heads > 128:
        raise ValueError(f"head dim hidden_size / num_heads = {hidden} / {heads} = {hidden / max(heads, 1):g} must be a multiple of 8, at most 128")
    c = capi.DiT1DConfig()
    c.hidden, c.depth, c.heads = hidden, depth, heads
    c.mlp_hidden = mlp_hidden
    c.in_channels, c.tokens_per_frame, c.max_tokens = channels, length, max_tokens
    c.timesteps = int(timesteps)
    c.causal = int(mode is not None)
    c.eps = 1e-6
    return x_shape, mode, c


class DiT1D(EngineModule):
    _family, _create = "dit1d", "dfot_dit1d_create"

    def __init__(self, cfg, x_shape: Sequence[int], max_tokens: int, external_cond_type: Optional[str] = None,
                 external_cond_num_classes: Optional[int] = None, external_cond_dim: int = 0, use_causal_mask: bool = True,
                 timesteps: int = 1000):
        super().__init__()
        self.x_shape, mode, c = check_config(cfg, x_shape, max_tokens, external_cond_dim, timesteps)
        channels, _, length = self.x_shape
        max_tokens, hidden, depth, mlp_hidden = int(c.max_tokens), int(c.hidden), int(c.depth), int(c.mlp_hidden)
        self.cfg = cfg
        self.causal_attn_mode = mode
        self.external_cond_type = external_cond_type
        self.external_cond_num_classes = external_cond_num_classes
        self.external_cond_dim = 0
        self.use_causal_mask = use_causal_mask  # ignored, as the reference ignores it: causal_attn_mode decides
        self.max_tokens = self.num_frames = max_tokens
        self.num_patches = self.n_token_per_frame = length
        self.hidden_size = hidden
        self._ccfg = c
        # The module (parameters, the sin-cos pos_embed) is built on the host; the engine handle, whose creation allocates device memory, is
        # created at the first weight sync or reserve, which also checks that the engine enumerates exactly these keys and shapes.
        self._build_tree(state_dict_layout(hidden, depth, mlp_hidden, channels, max_tokens * length))
        with torch.no_grad():
            self.pos_embed.copy_(sincos_pos_embed_1d(hidden, max_tokens * length))

    @property
    def in_channels(self) -> int:
        return self.x_shape[0]

    @property
    def noise_level_dim(self) -> int:
        return 256

    def _new_tensor(self, name: str, shape: Tuple[int, ...]) -> torch.Tensor:
        # pos_embed is a frozen parameter in the reference (requires_grad=False); the others are what its optimizer trains
        return nn.Parameter(torch.zeros(shape, dtype=torch.float32), requires_grad=name != "pos_embed")

    def reset_parameters(self, seed: int = 0) -> None:
        """The reference's init (dit_model.py:458-486): xavier-uniform Linear weights, N(0, 0.02) timestep MLP, zero biases, zero
        modulations and a zero output layer; pos_embed is the sin-cos table."""
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, t in self._tensors().items():
                if name == "pos_embed":
                    t.copy_(sincos_pos_embed_1d(self.hidden_size, self.max_tokens * self.num_patches))
                elif name.endswith(".bias") or ".adaLN_modulation." in name or name.startswith("final_layer"):
                    t.zero_()
                elif name.startswith("t_embedder"):
                    t.copy_(0.02 * torch.randn(t.shape, generator=g))
                else:
                    bound = math.sqrt(6.0 / (t.shape[0] + t.shape[1]))
                    t.copy_((torch.rand(t.shape, generator=g) * 2 - 1) * bound)

    def init_random(self, seed: int = 0) -> None:
        """Non-degenerate random weights for benchmarks and examples (the reference zero-inits every modulation and the output layer, which
        makes the output identically zero): weights ~ N(0, 1/fan_in) (modulations at half gain), biases ~ N(0, 0.05^2); pos_embed stays."""
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, t in self._tensors().items():
                if name == "pos_embed":
                    continue
                if name.endswith(".bias"):
                    v = 0.05 * torch.randn(t.shape, generator=g)
                else:
                    gain = 0.5 if ".adaLN_modulation." in name else 1.0
                    v = gain * torch.randn(t.shape, generator=g) / math.sqrt(t.shape[1])
                t.copy_(v.to(t.device))

    def forward(self, x: torch.Tensor, noise_levels: torch.Tensor, external_cond: Optional[torch.Tensor] = None,
                external_cond_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """BaseBackbone.forward; dispatched as the torch operator ``dfot::dit1d_forward`` (ops.py)."""
        if external_cond is not None:
            raise ValueError("this DiT1D is unconditioned (external_cond_dim 0): it takes no external_cond")
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("DiT1D is forward only: training and reconstruction guidance (the gradient w.r.t. x) need the backward of "
                                      "the frame-causal attention, which is not built; call it under torch.no_grad() or with parameters that "
                                      "do not require grad")
        if self._op_key is None:
            self._op_key = ops.register_model(self)
        return torch.ops.dfot.dit1d_forward(x, noise_levels, self._op_key)

    def _forward_impl(self, x: torch.Tensor, noise_levels: torch.Tensor) -> torch.Tensor:
        if x.ndim != 5 or tuple(x.shape[2:]) != self.x_shape:
            raise ValueError(f"x has shape {tuple(x.shape)}, expected (B, {self.max_tokens}, {', '.join(map(str, self.x_shape))})")
        b, t = x.shape[:2]
        if t != self.max_tokens:
            raise ValueError(f"T = {t} tokens, but this DiT1D runs at T == max_tokens = {self.max_tokens} only: its pos_embed add fixes the "
                             "sequence length, as in the reference")
        if tuple(noise_levels.shape) != (b, t):
            raise ValueError(f"noise_levels has shape {tuple(noise_levels.shape)}, expected {(b, t)}")
        if noise_levels.is_floating_point():
            raise TypeError("DiT1D takes integer noise levels (DiscreteDiffusion passes the level index); continuous diffusion "
                            "(floating noise levels) is not built")
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError(f"the backbone's parameters are on {dev}; move the module to the GPU first (there is no CPU path)")
        capi.require_device(dev, x=x, noise_levels=noise_levels)
        self.sync_weights()
        self.reserve(b)
        xf = x.detach().to(torch.float32).contiguous()
        kf = noise_levels.detach().to(torch.int32).contiguous()
        out = torch.empty_like(xf)
        capi.check(capi.lib.dfot_dit1d_forward(self._handle, capi.ptr(xf, torch.float32, "x"), capi.ptr(kf, torch.int32, "noise_levels"),
                                               capi.ptr(out), b, t, capi.stream_ptr()))
        return out.to(x.dtype)
