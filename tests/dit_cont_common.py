"""Shared helpers of tests/test_dit_cont_host.py, tests/test_gpu_dit_cont.py and tools/make_golden_dit_cont.py (not a test module): the
DiT family under continuous diffusion (``use_fourier_noise_embedding: true``, float noise levels).

  * fourier_features / fourier_embedding   torch restatement of FourierEmbedding (embeddings.py:94-109) + TimestepEmbedding: the argument
                                           level * freqs + phases is formed in fp32 exactly as the reference forms it (one multiply, one
                                           add), everything after it in the requested dtype
  * forward_dit / forward_diff / forward_fac / forward_facmat   the continuous forwards, COMPOSED with the existing restatements
                                           (oracle.dit, dit_fac_common, dit_facmat_common): only the noise-level embedding is swapped
  * key_shapes / seeded_params             the reference's state-dict keys with the two buffers in front, seeded per key
"""
import contextlib
import hashlib
import math

import numpy as np
import torch
import torch.nn.functional as F

import dit_fac_common as fac
import dit_facmat_common as facmat
from dit_cond_common import DIFF_TINY, SMALL, T, diff_cfg, dit_cfg, load, rel  # noqa: F401

NOISE_DIM = 256
FREQS, PHASES = "noise_level_pos_embedding.timesteps.freqs", "noise_level_pos_embedding.timesteps.phases"
EMB = "noise_level_pos_embedding.embedding"
PRECOND = 0.125


def fourier_buffers(seed=0):
    """FourierEmbedding.__init__'s draw (2 pi N(0,1), 2 pi U[0,1)) from a seeded generator"""
    g = torch.Generator().manual_seed(1000 + seed)
    return {FREQS: 2 * np.pi * torch.randn(NOISE_DIM, generator=g), PHASES: 2 * np.pi * torch.rand(NOISE_DIM, generator=g)}


def fourier_argument(levels, freqs, phases):
    """the fp32 argument of the cosine as the reference forms it: y[..., None] * freqs, then + phases (two rounded fp32 operations)"""
    y = levels.to(torch.float32)[..., None] * freqs.to(torch.float32)
    return y + phases.to(torch.float32)


def fourier_features(levels, freqs, phases, dtype=torch.float32):
    if dtype == torch.float32:
        return fourier_argument(levels, freqs, phases).cos() * np.sqrt(2)
    return fourier_argument(levels, freqs, phases).to(dtype).cos() * math.sqrt(2)


def fourier_embedding(p, levels, dtype=torch.float32):
    """StochasticTimeEmbedding(use_fourier=True): TimestepEmbedding(FourierEmbedding(levels)) -> [..., hidden]"""
    f = fourier_features(levels, p[FREQS], p[PHASES], dtype)
    w = lambda n: p[f"{EMB}.{n}"].to(dtype)
    return F.linear(F.silu(F.linear(f, w("linear_1.weight"), w("linear_1.bias"))), w("linear_2.weight"), w("linear_2.bias"))


def with_buffers(params, seed=0):
    """reference order: the two buffers precede noise_level_pos_embedding.embedding.*"""
    return {**fourier_buffers(seed), **params}


def key_shapes(keys):
    return [(FREQS, (NOISE_DIM,)), (PHASES, (NOISE_DIM,))] + list(keys)


def seeded_params(keys, seed=0):
    """keys: [(name, shape)] of a discrete model (dit_fac_common / dit_facmat_common key_shapes) -> its seeded weights + the two buffers"""
    mod = facmat if any(n.endswith("qkv_u") for n, _ in keys) else fac
    return with_buffers(mod.seeded_params(list(keys)), seed)


def digest(params):
    h = hashlib.sha256()
    for k in params:
        h.update(k.encode())
        h.update(params[k].contiguous().numpy().tobytes())
    return h.hexdigest()


@contextlib.contextmanager
def _fourier_oracle(dtype):
    """oracle.dit's forwards call its module-level noise_level_embedding(p, cfg, k): swap it for the Fourier one"""
    from oracle import dit as odit
    keep = odit.noise_level_embedding
    odit.noise_level_embedding = lambda p, cfg, k: fourier_embedding(p, k, dtype)
    try:
        yield odit
    finally:
        odit.noise_level_embedding = keep


def forward_dit(params, cfg, x, levels, dtype=torch.float32):
    """DiT3D "full" / rope_3d (oracle.dit.forward) at float levels; params include the buffers"""
    with _fourier_oracle(dtype) as odit:
        p = {k: (v if k in (FREQS, PHASES) else v.to(dtype)) for k, v in params.items()}
        return odit.forward(p, cfg, x.to(dtype), levels)


def forward_diff(params, cfg, x, levels, dtype=torch.float32):
    """DifferenceDiT3D (oracle.dit.diff_forward) at float levels"""
    with _fourier_oracle(dtype) as odit:
        p = {k: (v if k in (FREQS, PHASES) else v.to(dtype)) for k, v in params.items()}
        return odit.diff_forward(p, cfg, x.to(dtype), levels)


def _through_condition_path(params, levels, dtype):
    """The fac / facmat restatements form emb = MLP(sinusoidal(k)) + MLP_cond(cond) inline.  With the noise MLP's last Linear zeroed the
    first term vanishes, and the Fourier features handed in as the `cond` of a condition MLP that carries the noise MLP's weights make the
    second term exactly linear_2(SiLU(linear_1(feat))): the restated forward then runs at emb = the Fourier embedding."""
    p = {k: v for k, v in params.items() if k not in (FREQS, PHASES)}
    for n in ("linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias"):
        p[f"external_cond_embedding.{n}"] = params[f"{EMB}.{n}"]
    p[f"{EMB}.linear_2.weight"] = torch.zeros_like(params[f"{EMB}.linear_2.weight"])
    p[f"{EMB}.linear_2.bias"] = torch.zeros_like(params[f"{EMB}.linear_2.bias"])
    return p, fourier_features(levels, params[FREQS], params[PHASES], dtype)


def forward_fac(params, x, levels, dtype=torch.float64, **over):
    p, feat = _through_condition_path(params, levels, dtype)
    return fac.forward_host(p, x, torch.zeros(levels.shape, dtype=torch.long), cond=feat, dtype=dtype, **over)


def forward_facmat(params, x, levels, cc, rr, rope, dtype=torch.float64, **over):
    p, feat = _through_condition_path(params, levels, dtype)
    return facmat.forward_host(p, x, torch.zeros(levels.shape, dtype=torch.long), cc, rr, rope, cond=feat, dtype=dtype, **over)


def cont(cfg):
    """a backbone cfg with the @diffusion/continuous flag"""
    return dict(cfg, use_fourier_noise_embedding=True)


def logsnr_extremes():
    """precond_scale * logsnr[0] and precond_scale * logsnr[999] of cosine_simple_diffusion shifted 0.125: what the sampler really sends"""
    from dfot_amd.diffusion import DiffusionConfig, Schedule
    s = Schedule(DiffusionConfig(is_continuous=True))
    return float(np.float32(PRECOND) * s.logsnr[0]), float(np.float32(PRECOND) * s.logsnr[-1])
