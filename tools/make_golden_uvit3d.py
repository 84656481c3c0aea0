#!/usr/bin/env python3
"""Generate tests/golden/uvit3d.npz by executing the reference's own UViT3D (algorithms/dfot/backbones/u_vit/u_vit3d.py) on CPU in fp32,
eval().

Run ONLY in the build container (needs the reference checkout):   python tools/make_golden_uvit3d.py
Built on tools/ref_loader.py like tools/make_golden_dit_fac.py.  Configuration: tests/uvit3d_common.TINY (channels 128/128/128/256, emb 128,
one block per level, 2 heads: head dims 64 and 128, patch 2, frames 3x64x64, max_tokens 8, batch 2: 128 tokens at the coarsest level).
Weights: uvit3d_common.seeded_params, one generator per key seeded from the key's name and shape; the file stores the reference module's
ordered key list, the shapes and a digest of the tensors, not the tensors.

  names_<m>, shapes_<m>, digest_<m>   m in {a (no condition embedding), b (action dim 4, dropout 0), c (action dim 4, dropout 0.1)}
  inputs_digest, mask                  digest of uvit3d_common.inputs() (x [2,8,3,64,64], float levels [2,8], actions [2,8,4]: drawn from a fixed seed, not
                                       stored -- one frame tensor is 786 KB) and the per-video mask [True, False]
  out_a, out_b, out_c, out_c_masked    forwards (a: external_cond None; b, c: with cond; c_masked: with cond and mask), on the lattice
                                       uvit3d_common.sample() (every 13th element)
  run_*                                DFoTVideo._predict_videos around model b (assigned to diffusion_model.model, see main) under ContinuousDiffusion: 3 DDIM steps, vanilla history guidance
                                       1.5, 2 context tokens; every normal draw is recorded and checked to be the seeded generator's sequence
                                       (run_draw_shapes, run_draws_digest), run_inputs_digest, run_pred on the lattice, run_pred_min / _max
  host_rel                             the largest fp32 rel-L2 between tests/uvit3d_common.forward_host and the outputs above, as measured here
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_loader  # noqa: E402
from make_golden import RandnRecorder, save  # noqa: E402
from make_golden_dit import video_cfg  # noqa: E402
from make_golden_dit_cont import CONT  # noqa: E402
from oracle import dit as odit  # noqa: E402
import uvit3d_common as uc  # noqa: E402

torch.set_num_threads(8)


class SeededRandn:
    """While active, every torch.randn / torch.randn_like of the reference is served, in call order, by ONE CPU generator seeded here
    (whatever generator or global state the call names): the draws are then a function of the seed and of the shapes asked for, so the
    fixture stores the shapes and a digest and the tests re-draw them (uvit3d_common.trace_draws) -- 786 KB each, they cannot be stored."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self._randn, self._randn_like = torch.randn, torch.randn_like

    def __enter__(self):
        me = self

        def randn(*size, generator=None, device=None, dtype=None, **k):
            if len(size) == 1 and not isinstance(size[0], int):
                size = tuple(size[0])
            return me._randn(tuple(size), generator=me.g).to(device=device, dtype=dtype)

        def randn_like(x, **k):
            return me._randn(tuple(x.shape), generator=me.g).to(device=x.device, dtype=x.dtype)
        torch.randn, torch.randn_like = randn, randn_like
        return self

    def __exit__(self, *a):
        torch.randn, torch.randn_like = self._randn, self._randn_like


def make(R, tag):
    dim, drop = uc.CASES[tag]
    model = R["UViT3D"](R["AttrDict"](uc.backbone_cfg(drop)), x_shape=list(uc.X_SHAPE), max_tokens=uc.MAX_TOKENS, external_cond_dim=dim,
                        use_causal_mask=False).eval()
    keys = [(n, tuple(t.shape)) for n, t in model.state_dict().items()]
    assert keys == uc.key_shapes(dim, drop), "key_shapes disagrees with the reference"
    params = uc.seeded_params(keys)
    model.load_state_dict(params, strict=True)
    return model, params, keys


def meta(out, tag, params, keys):
    out[f"names_{tag}"] = np.array([n for n, _ in keys])
    out[f"shapes_{tag}"] = np.array([" ".join(map(str, s)) for _, s in keys])
    out[f"digest_{tag}"] = np.array(uc.digest(params))


@torch.no_grad()
def main():
    R = ref_loader.install()
    x, levels, cond, mask = uc.inputs()
    out = dict(inputs_digest=np.array(uc.tensor_digest(x, levels, cond)), mask=mask)
    host = []
    for tag in "abc":
        print("uvit3d", tag)
        model, params, keys = make(R, tag)
        meta(out, tag, params, keys)
        c = None if tag == "a" else cond
        o = model(x, levels, c)
        out[f"out_{tag}"] = uc.sample(o)
        host.append(uc.rel(uc.forward_host(params, x, levels, c, dtype=torch.float32), o))
        if tag == "b":  # dropout 0: the module is a plain TimestepEmbedding and takes no mask
            assert not hasattr(model.external_cond_embedding, "dropout")
        if tag == "c":
            o = model(x, levels, cond, mask)
            out["out_c_masked"] = uc.sample(o)
            host.append(uc.rel(uc.forward_host(params, x, levels, cond, mask, dtype=torch.float32), o))

    print("uvit3d sampler trace")
    small = odit.DiTConfig(hidden_size=128, depth=1, num_heads=2, patch_size=2, in_channels=uc.X_SHAPE[0], resolution=uc.X_SHAPE[1:],
                           max_tokens=uc.MAX_TOKENS)
    cfg = video_cfg(R["AttrDict"], small, sampling_steps=3, hg=dict(name="vanilla", guidance_scale=1.5))
    cfg["diffusion"] = R["AttrDict"](dict(CONT, sampling_timesteps=3))
    cfg["backbone"]["use_fourier_noise_embedding"] = True
    cfg["external_cond_dim"] = uc.COND_DIM
    # DiscreteDiffusion._build_model (discrete_diffusion.py:84-92) passes external_cond_type / external_cond_num_classes to every backbone
    # class, and UViT3D.__init__ (u_vit3d.py:30-37) does not take them: the algorithm cannot construct a "u_vit3d" backbone from its
    # config.  The algorithm is therefore built around a stand-in backbone of the same x_shape / max_tokens / external_cond_dim, and the
    # reference's own UViT3D module, constructed directly as above, takes its place before anything runs.
    algo = R["DFoTVideo"](cfg).eval()
    model, _, _ = make(R, "b")
    algo.diffusion_model.model = model
    vid, rcond = uc.trace_inputs()
    algo.generator = torch.Generator().manual_seed(uc.DRAW_SEED)
    with SeededRandn(uc.DRAW_SEED), RandnRecorder() as rec:
        pred = algo._predict_videos(vid.clone(), n_context_tokens=2, conditions=rcond.clone())
    shapes = [tuple(d.shape) for d in rec.draws]
    again = uc.trace_draws(shapes)
    assert len(shapes) > 0 and all(torch.equal(d, r) for d, r in zip(rec.draws, again)), "the recorded draws are not the seeded sequence"
    assert torch.equal(pred[:, :2], vid[:, :2])
    out.update(run_inputs_digest=np.array(uc.tensor_digest(vid, rcond)), run_pred=uc.sample(pred), run_pred_min=pred.min(), run_pred_max=pred.max(),
               run_draw_shapes=np.array([" ".join(map(str, sh)) for sh in shapes]), run_draws_digest=np.array(uc.tensor_digest(*rec.draws)))
    out["host_rel"] = np.array(max(host))
    print("host restatement (fp32) vs the reference (fp32): rel-L2", host)
    save("uvit3d.npz", **out)


if __name__ == "__main__":
    main()
