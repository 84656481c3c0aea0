"""Loader that executes the reference's OWN source files on CPU (build container only).

Used only by tools/make_golden.py to capture golden vectors; never shipped to or run on the
GPU box (``/root/reference`` does not exist there) and never imported by the product or tests.

The reference imports third-party packages this image lacks.  They are replaced by minimal
stand-ins that restate the pinned upstream semantics (versions from the reference's
requirements.txt).  Each stand-in is a few lines; none of the reference's own code is
replaced or copied:

  timm==1.0.17     PatchEmbed  -> Conv2d(k=s=patch) [+ flatten(2).transpose(1,2) if flatten]
                   Mlp         -> fc1 -> act -> fc2
  diffusers==0.32.2 TimestepEmbedding -> linear_1 -> SiLU -> linear_2 ; LabelEmbedding -> nn.Embedding
                   for install_dcae() (the DC-AE file imports its layers from diffusers); written from knowledge of that release and
                   NOT checked against the library, which is not available here:
                   RMSNorm(dim, eps, elementwise_affine, bias) -> x * rsqrt(mean(x^2, -1) in fp32 + eps) * weight + bias
                   get_normalization -> rms_norm: RMSNorm(C, 1e-5, True, True); batch_norm: nn.BatchNorm2d(C)
                   get_activation    -> silu / swish, relu, relu6, gelu, mish
                   GLUMBConv         -> conv_inverted 1x1 C -> 8C, SiLU, depthwise 3x3 on 8C, chunk(2): x * silu(gate),
                                        conv_point 1x1 4C -> C (no bias), RMSNorm on channels, + residual
                   SanaMultiscaleAttnProcessor2_0 -> cat[to_q | to_k | to_v] (+ multiscale branches), reshape (B, -1, 3 * head_dim, H W),
                                        chunk(3, dim 2), ReLU on q and k, linear attention iff H W > head_dim (fp32), to_out, norm_out,
                                        + residual
                   ConfigMixin / ModelMixin / register_to_config / apply_forward_hook / EncoderOutput / DecoderOutput -> trivial
  rotary_embedding_torch==0.8.6 rotate_half -> interleaved pairs (x1,x2) -> (-x2,x1)
  omegaconf==2.3.0 DictConfig  -> attribute dict with .get ; OmegaConf.to_container -> plain dict
  lightning==2.5.1 LightningModule -> nn.Module with .device/.log/.trainer
  wandb, roma, colorama, torchmetrics...: names only (never called on this path)

The reference's heavy package __init__ files (they import VAE / metric / dataset stacks) are
bypassed by registering namespace packages for ``algorithms``, ``algorithms.dfot`` ... so
that only the files on the hot path are executed.
"""
from __future__ import annotations

import importlib
import importlib.machinery
import sys
import types

import torch
from torch import nn

REF = "/root/reference"


def _mod(name: str, **attrs):
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _ns(name: str, path: str):
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)
    m.__path__ = [path]
    sys.modules[name] = m
    return m


class AttrDict(dict):
    """Stand-in for omegaconf.DictConfig: recursive attribute access + .get."""

    def __init__(self, d=None, **kw):
        super().__init__()
        for k, v in {**(d or {}), **kw}.items():
            self[k] = self._wrap(v)

    @classmethod
    def _wrap(cls, v):
        if isinstance(v, dict) and not isinstance(v, AttrDict):
            return cls(v)
        return v

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = self._wrap(v)


def _to_container(cfg, resolve=True):
    if isinstance(cfg, dict):
        return {k: _to_container(v) for k, v in cfg.items()}
    if isinstance(cfg, (list, tuple)):
        return [_to_container(v) for v in cfg]
    return cfg


class _PatchEmbed(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, norm_layer=None,
                 flatten=True, bias=True, **_):
        super().__init__()
        ps = (patch_size, patch_size) if isinstance(patch_size, int) else tuple(patch_size)
        self.patch_size = ps
        if img_size is not None:
            im = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)
            self.grid_size = (im[0] // ps[0], im[1] // ps[1])
            self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.flatten = flatten
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=ps, stride=ps, bias=bias)
        self.norm = nn.Identity()

    def forward(self, x):
        x = self.proj(x)
        if self.flatten:
            x = x.flatten(2).transpose(1, 2)
        return self.norm(x)


class _Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU,
                 bias=True, drop=0.0, **_):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features, bias=bias)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features, bias=bias)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class _TimestepEmbedding(nn.Module):
    def __init__(self, in_channels, time_embed_dim, **_):
        super().__init__()
        self.linear_1 = nn.Linear(in_channels, time_embed_dim)
        self.act = nn.SiLU()
        self.linear_2 = nn.Linear(time_embed_dim, time_embed_dim)

    def forward(self, sample):
        return self.linear_2(self.act(self.linear_1(sample)))


class _LabelEmbedding(nn.Module):
    def __init__(self, num_classes, hidden_size, dropout_prob):
        super().__init__()
        self.embedding_table = nn.Embedding(num_classes + int(dropout_prob > 0), hidden_size)

    def forward(self, labels, force_drop_ids=None):
        return self.embedding_table(labels)


def _rotate_half(x):
    x = x.reshape(*x.shape[:-1], -1, 2)
    x1, x2 = x.unbind(dim=-1)
    return torch.stack((-x2, x1), dim=-1).flatten(-2)


class _LightningModule(nn.Module):
    trainer = None
    logger = None

    @property
    def device(self):
        for p in self.parameters():
            return p.device
        return torch.device("cpu")

    def log(self, *a, **k):
        pass

    def log_dict(self, *a, **k):
        pass

    def save_hyperparameters(self, *a, **k):
        pass


def install():
    """Registers stand-ins + namespace packages, imports the hot-path reference modules and
    returns a dict of the reference classes needed."""
    if REF not in sys.path:
        sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    import accelerate  # noqa: F401  (real, must precede the wandb stub)
    import transformers  # noqa: F401

    oc = _mod("omegaconf", DictConfig=AttrDict,
              OmegaConf=types.SimpleNamespace(to_container=_to_container, create=AttrDict))
    _mod("omegaconf.omegaconf", open_dict=lambda cfg: __import__("contextlib").nullcontext())
    oc.omegaconf = sys.modules["omegaconf.omegaconf"]
    _mod("timm")
    _mod("timm.models")
    _mod("timm.models.vision_transformer", PatchEmbed=_PatchEmbed, Mlp=_Mlp, Attention=nn.Module)
    _mod("timm.layers", PatchEmbed=_PatchEmbed, Mlp=_Mlp)
    _mod("diffusers")
    _mod("diffusers.models")
    _mod("diffusers.models.embeddings", TimestepEmbedding=_TimestepEmbedding, LabelEmbedding=_LabelEmbedding)
    _mod("rotary_embedding_torch")
    _mod("rotary_embedding_torch.rotary_embedding_torch", rotate_half=_rotate_half)
    _mod("roma")
    _mod("wandb", Video=object)
    _mod("colorama", Fore=types.SimpleNamespace(CYAN="", RESET="", RED="", GREEN="", YELLOW=""))
    lt = _mod("lightning")
    pl = _mod("lightning.pytorch", LightningModule=_LightningModule)
    lt.pytorch = pl
    _mod("lightning.pytorch.utilities", grad_norm=lambda *a, **k: {})
    _mod("lightning.pytorch.utilities.types", STEP_OUTPUT=object)
    _mod("lightning.pytorch.loggers")
    _mod("lightning.pytorch.loggers.logger", Logger=object)
    _mod("lightning_utilities")
    _mod("lightning_utilities.core")
    _mod("lightning_utilities.core.apply_func", apply_to_collection=lambda d, *a, **k: d)

    for name, rel in [
        ("algorithms", "algorithms"), ("algorithms.common", "algorithms/common"),
        ("algorithms.dfot", "algorithms/dfot"), ("algorithms.dfot.backbones", "algorithms/dfot/backbones"),
        ("algorithms.dfot.backbones.modules", "algorithms/dfot/backbones/modules"),
        ("algorithms.dfot.backbones.u_vit", "algorithms/dfot/backbones/u_vit"),
        ("algorithms.dfot.backbones.dit", "algorithms/dfot/backbones/dit"),
        ("algorithms.dfot.diffusion", "algorithms/dfot/diffusion"), ("utils", "utils"),
    ]:
        _ns(name, f"{REF}/{rel}")
    _mod("utils.distributed_utils", is_rank_zero=True, rank_zero_print=print)
    _mod("utils.logging_utils", log_video=lambda *a, **k: None)
    dummy = type("Dummy", (), {})
    _mod("algorithms.vae", ImageVAE=dummy, VideoVAE=dummy, MyAutoencoderDC=dummy, AutoencoderKL=dummy,
         TiTok_KL=dummy)
    _mod("algorithms.common.metrics")
    _mod("algorithms.common.metrics.video", VideoMetric=dummy, SharedVideoMetricModelRegistry=dummy)
    _mod("algorithms.common.attn_hook", register_hooks=None, clear_hooks=None, save_attention_maps=None,
         attn_maps={})

    imp = importlib.import_module
    imp("algorithms.dfot.backbones.modules.embeddings")
    imp("algorithms.dfot.backbones.base_backbone")
    blocks = imp("algorithms.dfot.backbones.u_vit.u_vit_blocks")
    uvit = imp("algorithms.dfot.backbones.u_vit.u_vit3d")
    uvit_pose = imp("algorithms.dfot.backbones.u_vit.u_vit3d_pose")
    bb = sys.modules["algorithms.dfot.backbones"]
    for n in ("Unet3D", "DiT3D", "DiT3DPose", "FARDiT", "DIT1D", "DifferenceDiT3D"):
        setattr(bb, n, None)
    bb.UViT3D, bb.UViT3DPose = uvit.UViT3D, uvit_pose.UViT3DPose
    dit3d = imp("algorithms.dfot.backbones.dit.dit3d")  # K600 backbone (only the "full" variant is exercised)
    bb.DiT3D = dit3d.DiT3D
    diffdit = imp("algorithms.dfot.backbones.dit.difference_dit3d")  # bash/k600 backbone (factorized matrix attention)
    bb.DifferenceDiT3D = diffdit.DifferenceDiT3D
    dd = imp("algorithms.dfot.diffusion.discrete_diffusion")
    cd = imp("algorithms.dfot.diffusion.continuous_diffusion")
    dpk = sys.modules["algorithms.dfot.diffusion"]
    dpk.DiscreteDiffusion, dpk.ContinuousDiffusion = dd.DiscreteDiffusion, cd.ContinuousDiffusion
    hgm = imp("algorithms.dfot.history_guidance")
    pose_algo = imp("algorithms.dfot.dfot_video_pose")
    video_algo = sys.modules["algorithms.dfot.dfot_video"]
    diff_algo = imp("algorithms.dfot.difference_dfot_video")
    geo = imp("utils.geometry_utils")
    return {
        "UViT3D": uvit.UViT3D, "UViT3DPose": uvit_pose.UViT3DPose, "blocks": blocks, "DiscreteDiffusion": dd.DiscreteDiffusion,
        "ContinuousDiffusion": cd.ContinuousDiffusion, "HistoryGuidance": hgm.HistoryGuidance,
        "DFoTVideoPose": pose_algo.DFoTVideoPose, "DFoTVideo": video_algo.DFoTVideo, "DiT3D": dit3d.DiT3D,
        "DifferenceDiT3D": diffdit.DifferenceDiT3D, "DifferenceDFoTVideo": diff_algo.DifferenceDFoTVideo,
        "geometry": geo, "AttrDict": AttrDict,
    }


def install_vae():
    """The reference's VideoVAE (algorithms/vae/video_vae/model.py and algorithms/vae/common/modules/*) importable on its own: namespace
    packages skip algorithms/vae/__init__.py and video_vae/__init__.py (they pull trainers / lightning / lpips), utils.ckpt_utils (wandb /
    huggingface download helpers, only used by from_pretrained) is a four-name stand-in.  Returns the VideoVAE class."""
    if REF not in sys.path:
        sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    for name, rel in [("algorithms", "algorithms"), ("algorithms.vae", "algorithms/vae"), ("algorithms.vae.video_vae", "algorithms/vae/video_vae"),
                      ("utils", "utils")]:
        _ns(name, f"{REF}/{rel}")
    _mod("utils.ckpt_utils", is_wandb_run_path=lambda p: False, is_hf_path=lambda p: False, wandb_to_local_path=lambda p: p,
         download_pretrained=lambda p: p)
    model = importlib.import_module("algorithms.vae.video_vae.model")   # imports algorithms.vae.common(.modules) for real
    return model.VideoVAE


def install_image_vae():
    """The reference's ImageVAE building blocks (algorithms/vae/image_vae/model.py and algorithms/vae/common/modules/*) importable on their
    own: image_vae/__init__.py and trainer.py pull Lightning / lpips, so the namespace packages skip them.  Returns (Encoder, Decoder); the
    ImageVAE wrapper around them (trainer.py:281-345) is two nn.Conv2d(.., 1) that tools/make_golden_image_vae.py states itself."""
    if REF not in sys.path:
        sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    for name, rel in [("algorithms", "algorithms"), ("algorithms.vae", "algorithms/vae"), ("algorithms.vae.image_vae", "algorithms/vae/image_vae"),
                      ("utils", "utils")]:
        if name not in sys.modules:
            _ns(name, f"{REF}/{rel}")
    model = importlib.import_module("algorithms.vae.image_vae.model")   # imports algorithms.vae.common.modules for real
    return model.Encoder, model.Decoder


def install_titok():
    """The reference's TiTok_KL (algorithms/vae/tiktok_kl/{titok_kl,blocks_kl,maskgit_vqgan}.py) importable on its own: namespace packages
    skip algorithms/vae/__init__.py and tiktok_kl/__init__.py (they pull the trainers), ``OmegaConf.create`` is the AttrDict stand-in above
    (the pixel decoder only reads attributes of its config).  Returns the TiTok_KL class."""
    if REF not in sys.path:
        sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    for name, rel in [("algorithms", "algorithms"), ("algorithms.vae", "algorithms/vae"), ("algorithms.vae.tiktok_kl", "algorithms/vae/tiktok_kl"),
                      ("utils", "utils")]:
        if name not in sys.modules:
            _ns(name, f"{REF}/{rel}")
    if "omegaconf" not in sys.modules:
        _mod("omegaconf", DictConfig=AttrDict, OmegaConf=types.SimpleNamespace(to_container=_to_container, create=AttrDict))
    model = importlib.import_module("algorithms.vae.tiktok_kl.titok_kl")   # imports algorithms.vae.common.distribution for real
    return model.TiTok_KL


# ---------------------------------------------------------------------------------------------------------------------------------
# diffusers 0.32.2 stand-ins for the DC-AE file (see the header: stated from knowledge of the release, unverified against the library)
class _RMSNorm(nn.Module):
    def __init__(self, dim, eps, elementwise_affine=True, bias=False):
        super().__init__()
        self.eps, self.weight, self.bias = eps, None, None
        if elementwise_affine:
            self.weight = nn.Parameter(torch.ones(dim))
            if bias:
                self.bias = nn.Parameter(torch.zeros(dim))

    def forward(self, x):
        dtype = x.dtype
        var = x.to(torch.float32).pow(2).mean(-1, keepdim=True)
        x = x * torch.rsqrt(var + self.eps)
        if self.weight is not None:
            x = x.to(self.weight.dtype) * self.weight
            if self.bias is not None:
                x = x + self.bias
            return x
        return x.to(dtype)


def _get_normalization(norm_type="batch_norm", num_features=None, eps=1e-5, elementwise_affine=True, bias=True):
    if norm_type == "rms_norm":
        return _RMSNorm(num_features, eps=eps, elementwise_affine=elementwise_affine, bias=bias)
    if norm_type == "batch_norm":
        return nn.BatchNorm2d(num_features, eps=eps, affine=elementwise_affine)
    raise ValueError(f"norm_type={norm_type} is not supported")


def _get_activation(act_fn):
    acts = {"silu": nn.SiLU, "swish": nn.SiLU, "relu": nn.ReLU, "relu6": nn.ReLU6, "gelu": nn.GELU, "mish": nn.Mish}
    return acts[act_fn.lower()]()


class _GLUMBConv(nn.Module):
    def __init__(self, in_channels, out_channels, expand_ratio=4, norm_type=None, residual_connection=True):
        super().__init__()
        hidden = int(expand_ratio * in_channels)
        self.norm_type, self.residual_connection = norm_type, residual_connection
        self.nonlinearity = nn.SiLU()
        self.conv_inverted = nn.Conv2d(in_channels, hidden * 2, 1, 1, 0)
        self.conv_depth = nn.Conv2d(hidden * 2, hidden * 2, 3, 1, 1, groups=hidden * 2)
        self.conv_point = nn.Conv2d(hidden, out_channels, 1, 1, 0, bias=False)
        self.norm = _RMSNorm(out_channels, eps=1e-5, elementwise_affine=True, bias=True) if norm_type == "rms_norm" else None

    def forward(self, x):
        residual = x
        x = self.conv_depth(self.nonlinearity(self.conv_inverted(x)))
        x, gate = torch.chunk(x, 2, dim=1)
        x = self.conv_point(x * self.nonlinearity(gate))
        if self.norm_type == "rms_norm":
            x = self.norm(x.movedim(1, -1)).movedim(-1, 1)
        return x + residual if self.residual_connection else x


class _SanaMultiscaleAttentionProjection(nn.Module):
    def __init__(self, in_channels, num_attention_heads, kernel_size):
        super().__init__()
        ch = 3 * in_channels
        self.proj_in = nn.Conv2d(ch, ch, kernel_size, padding=kernel_size // 2, groups=ch, bias=False)
        self.proj_out = nn.Conv2d(ch, ch, 1, 1, 0, groups=3 * num_attention_heads, bias=False)

    def forward(self, x):
        return self.proj_out(self.proj_in(x))


class _SanaMultiscaleAttnProcessor2_0:
    def __call__(self, attn, hidden_states):
        height, width = hidden_states.shape[-2:]
        use_linear = height * width > attn.attention_head_dim
        residual, dtype = hidden_states, hidden_states.dtype
        hidden_states = hidden_states.movedim(1, -1)
        hidden_states = torch.cat([attn.to_q(hidden_states), attn.to_k(hidden_states), attn.to_v(hidden_states)], dim=3).movedim(-1, 1)
        multi = [hidden_states] + [block(hidden_states) for block in attn.to_qkv_multiscale]
        hidden_states = torch.cat(multi, dim=1)
        if use_linear:
            hidden_states = hidden_states.to(torch.float32)
        hidden_states = hidden_states.reshape(hidden_states.shape[0], -1, 3 * attn.attention_head_dim, height * width)
        query, key, value = hidden_states.chunk(3, dim=2)
        query, key = attn.nonlinearity(query), attn.nonlinearity(key)
        _SanaMultiscaleAttnProcessor2_0.branches.append("linear" if use_linear else "quadratic")
        if use_linear:
            hidden_states = attn.apply_linear_attention(query, key, value).to(dtype)
        else:
            hidden_states = attn.apply_quadratic_attention(query, key, value)
        hidden_states = torch.reshape(hidden_states, (hidden_states.shape[0], -1, height, width))
        hidden_states = attn.to_out(hidden_states.movedim(1, -1)).movedim(-1, 1)
        if attn.norm_type == "rms_norm":
            hidden_states = attn.norm_out(hidden_states.movedim(1, -1)).movedim(-1, 1)
        else:
            hidden_states = attn.norm_out(hidden_states)
        return hidden_states + residual if attn.residual_connection else hidden_states


_SanaMultiscaleAttnProcessor2_0.branches = []   # which branch each call took (tools/make_golden_dcae.py asserts: linear only)


def install_dcae():
    """The reference's DC-AE (algorithms/vae/dc_ae/autoencoder_dc_model.py) importable on its own: namespace packages skip the package
    __init__ files, the diffusers layers it imports are the stand-ins above (unverified against the library), the Lightning / omegaconf /
    utils imports are names only.  Returns (MyAutoencoderDC, the module): the module also holds Encoder, Decoder and the blocks."""
    if REF not in sys.path:
        sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    for name, rel in [("algorithms", "algorithms"), ("algorithms.vae", "algorithms/vae"), ("algorithms.vae.dc_ae", "algorithms/vae/dc_ae"),
                      ("algorithms.common", "algorithms/common"), ("utils", "utils")]:
        if name not in sys.modules:
            _ns(name, f"{REF}/{rel}")
    if "omegaconf" not in sys.modules:
        _mod("omegaconf", DictConfig=AttrDict, OmegaConf=types.SimpleNamespace(to_container=_to_container, create=AttrDict))
    _mod("algorithms.common.base_pytorch_algo", BasePytorchAlgo=_LightningModule)
    if "lightning" not in sys.modules:
        lt = _mod("lightning")
        lt.pytorch = _mod("lightning.pytorch", LightningModule=_LightningModule)
        _mod("lightning.pytorch.utilities")
        _mod("lightning.pytorch.utilities.types", STEP_OUTPUT=object)
    _mod("utils.storage_utils", safe_torch_save=None)
    _mod("utils.logging_utils", log_video=lambda *a, **k: None)
    _mod("utils.ckpt_utils", is_wandb_run_path=lambda p: False, is_hf_path=lambda p: False, wandb_to_local_path=lambda p: p,
         download_pretrained=lambda p: p)
    for name in ("diffusers", "diffusers.models", "diffusers.models.autoencoders", "diffusers.models.transformers", "diffusers.utils"):
        if name not in sys.modules:
            _mod(name)
    out_cls = lambda n: type(n, (dict,), {})  # noqa: E731
    _mod("diffusers.configuration_utils", ConfigMixin=type("ConfigMixin", (), {}), register_to_config=lambda f: f)
    _mod("diffusers.models.activations", get_activation=_get_activation)
    _mod("diffusers.models.attention_processor", SanaMultiscaleAttentionProjection=_SanaMultiscaleAttentionProjection,
         SanaMultiscaleAttnProcessor2_0=_SanaMultiscaleAttnProcessor2_0)
    _mod("diffusers.models.autoencoders.vae", DecoderOutput=out_cls("DecoderOutput"), EncoderOutput=out_cls("EncoderOutput"))
    _mod("diffusers.models.modeling_utils", ModelMixin=type("ModelMixin", (nn.Module,), {}))
    _mod("diffusers.models.normalization", RMSNorm=_RMSNorm, get_normalization=_get_normalization)
    _mod("diffusers.models.transformers.sana_transformer", GLUMBConv=_GLUMBConv)
    _mod("diffusers.utils.accelerate_utils", apply_forward_hook=lambda f: f)
    model = importlib.import_module("algorithms.vae.dc_ae.autoencoder_dc_model")
    return model.MyAutoencoderDC, model


def install_dit1d():
    """The reference's DIT1D (algorithms/dfot/backbones/dit1d/dit_model.py) importable on its own: namespace packages skip the package
    __init__ files; timm's Mlp is the stand-in above, ``timm.layers.use_fused_attn`` answers False (the module then runs its own
    ``softmax(q k^T * scale + mask) v``, dit_model.py:78-85, the arithmetic F.scaled_dot_product_attention restates), and
    ``rotary_embedding_torch.RotaryEmbedding`` is a name that is never constructed (use_rotary_emb: false).  The constructor's eight
    ``print`` calls are silenced.  Returns (DIT1D constructor, the module): the module also holds get_1d_sincos_pos_embed."""
    import contextlib
    import functools
    import io
    if REF not in sys.path:
        sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    for name, rel in [("algorithms", "algorithms"), ("algorithms.dfot", "algorithms/dfot"), ("algorithms.dfot.backbones", "algorithms/dfot/backbones"),
                      ("algorithms.dfot.backbones.dit1d", "algorithms/dfot/backbones/dit1d")]:
        if name not in sys.modules:
            _ns(name, f"{REF}/{rel}")
    for name in ("timm", "timm.models"):
        if name not in sys.modules:
            _mod(name)
    if "timm.models.vision_transformer" not in sys.modules:
        _mod("timm.models.vision_transformer", PatchEmbed=_PatchEmbed, Mlp=_Mlp, Attention=nn.Module)
    if "timm.layers" not in sys.modules:
        _mod("timm.layers", PatchEmbed=_PatchEmbed, Mlp=_Mlp)
    sys.modules["timm.layers"].use_fused_attn = lambda: False
    if "rotary_embedding_torch" not in sys.modules:
        _mod("rotary_embedding_torch")

    class _NeverBuilt:
        def __init__(self, *a, **k):
            raise AssertionError("RotaryEmbedding is a name only: use_rotary_emb is false on this path")
    sys.modules["rotary_embedding_torch"].RotaryEmbedding = _NeverBuilt
    model = importlib.import_module("algorithms.dfot.backbones.dit1d.dit_model")

    @functools.wraps(model.DIT1D)
    def quiet(*a, **k):
        with contextlib.redirect_stdout(io.StringIO()):
            return model.DIT1D(*a, **k)
    return quiet, model
