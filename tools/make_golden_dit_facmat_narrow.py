#!/usr/bin/env python3
"""Generate tests/golden/dit_facmat_narrow.npz by executing the reference's own DiT3D on CPU in fp32, eval(), with variant
"factorized_matrix_attention" at narrow column widths: embed_col_dim 1, 8, 16, 32 and 3 (tests/dit_facmat_narrow_common.CASES), the rungs
S-1-1 .. S-32-4 of the @FacMatDiT ladder.

Run ONLY in the build container (needs the reference checkout):   python tools/make_golden_dit_facmat_narrow.py
Built on tools/ref_loader.py like tools/make_golden_dit_p64.py.  Geometry: dit_facmat_common.TINY (embed_row_dim 128, depth 2, 4 spatial
heads, 4 row heads), at 128 patches per frame (latents 4x16x8, patch 1, max_tokens 5) and, for e8 and e32, at 64 (4x16x16, patch 2,
max_tokens 4).  Weights: the seeded_params of dit_facmat_common with a gain on the q | k columns of the matrix blocks' right factor -- per
case the smallest gain of GAINS at which every host frame map of the case clears CONTRAST_BAR against uniform and against its transpose.
The file stores the reference module's ordered key list, the shapes, the gain and a digest of the tensors, not the tensors.

  x, k, x64, k64                        inputs [2,5,4,16,8] / [2,4,4,16,16] and integer levels
  gain_<tag>                            the gain of the case
  names_<tag>, shapes_<tag>, digest_<tag>, out_<tag>_t5, out_<tag>_t3          every case at 128 patches: T = 5 and the first 3 tokens
  names64_<tag>, shapes64_<tag>, digest64_<tag>, out64_<tag>_t4, out64_<tag>_t2  e8, e32 at 64 patches: T = 4 and the first 2 tokens
  names_act, digest_act, act_cond, act_mask, out_act, out_act_masked          e8 with an action condition (dim 3, dropout 0.1)
  run_vid, run_pred, run_n_noise, run_noise<i>                                a 3-step sampler run of e8 (2 context frames), draws recorded
  host_rel                              the largest fp32 rel-L2 between the host restatement and the outputs above, as measured here
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
from oracle import dit as odit  # noqa: E402
import dit_facmat_common as fm  # noqa: E402
import dit_facmat_narrow_common as nc  # noqa: E402

torch.set_num_threads(8)


def make(R, tag, gain, patches=128, cond=False):
    geo = nc.GEOM[patches]
    kw = dict(external_cond_type="action", external_cond_num_classes=None, external_cond_dim=nc.COND_DIM if cond else 0)
    model = R["DiT3D"](R["AttrDict"](nc.cfg(tag, patches, cond)), x_shape=list(geo["x_shape"]), max_tokens=geo["max_tokens"],
                       use_causal_mask=False, **kw).eval()
    keys = [(n, tuple(t.shape)) for n, t in model.state_dict().items()]
    assert keys == nc.keys(tag, patches, cond), "key_shapes disagrees with the reference"
    params = nc.seeded(tag, gain, patches, cond)
    model.load_state_dict(params, strict=True)
    assert (model.dit_base.temporal_rope is not None) == bool(nc.CASES[tag][3])
    return model, params, keys


def meta(out, tag, params, keys, pre=""):
    out[f"names{pre}_{tag}"] = np.array([n for n, _ in keys])
    out[f"shapes{pre}_{tag}"] = np.array([" ".join(map(str, s)) for _, s in keys])
    out[f"digest{pre}_{tag}"] = np.array(nc.digest(params))


def pick_gain(tag, xs):
    """the smallest gain at which every host map of the case (at every geometry it runs at) is CONTRAST_BAR from uniform and its transpose"""
    for gain in nc.GAINS:
        worst = []
        for patches, (x, k) in xs.items():
            if patches == 64 and tag not in nc.P64_TAGS:
                continue
            maps = nc.host_frame_maps(tag, nc.seeded(tag, gain, patches), x, k, patches)
            worst += [min(nc.contrast(w)) for w in maps.values()]
        print(f"  {tag} gain {gain}: smallest contrast of a host frame map {min(worst):.3e}")
        if min(worst) >= nc.CONTRAST_BAR:
            return gain
    raise AssertionError(f"{tag}: no gain up to {nc.GAINS[-1]} separates the maps from uniform / their transpose")


@torch.no_grad()
def main():
    R = ref_loader.install()
    g = torch.Generator().manual_seed(83)
    x = torch.randn(2, 5, 4, 16, 8, generator=g)
    k = torch.randint(0, 1000, (2, 5), generator=g)
    x64 = torch.randn(2, 4, *nc.GEOM[64]["x_shape"], generator=g)
    k64 = torch.randint(0, 1000, (2, 4), generator=g)
    out = dict(x=x, k=k, x64=x64, k64=k64)
    host = []
    gains = {}
    for tag in nc.CASES:
        print("dit facmat narrow", tag, nc.CASES[tag])
        gain = gains[tag] = pick_gain(tag, {128: (x, k), 64: (x64, k64)})
        out[f"gain_{tag}"] = np.array(gain)
        model, params, keys = make(R, tag, gain)
        meta(out, tag, params, keys)
        o5, o3 = model(x, k), model(x[:, :3].contiguous(), k[:, :3].contiguous())
        out[f"out_{tag}_t5"], out[f"out_{tag}_t3"] = o5, o3
        host += [nc.rel(nc.host(tag, params, x, k, dtype=torch.float32), o5),
                 nc.rel(nc.host(tag, params, x[:, :3], k[:, :3], dtype=torch.float32), o3)]
        if tag in nc.P64_TAGS:
            model, params, keys = make(R, tag, gain, 64)
            meta(out, tag, params, keys, "64")
            o4, o2 = model(x64, k64), model(x64[:, :2].contiguous(), k64[:, :2].contiguous())
            out[f"out64_{tag}_t4"], out[f"out64_{tag}_t2"] = o4, o2
            host += [nc.rel(nc.host(tag, params, x64, k64, patches=64, dtype=torch.float32), o4),
                     nc.rel(nc.host(tag, params, x64[:, :2], k64[:, :2], patches=64, dtype=torch.float32), o2)]

    print("dit facmat narrow act")
    tag = nc.COND_TAG
    model, params, keys = make(R, tag, gains[tag], cond=True)
    meta(out, "act", params, keys)
    cond = torch.randn(2, 5, nc.COND_DIM, generator=g)
    mask = torch.tensor([True, False])
    oa, om = model(x, k, cond), model(x, k, cond, mask)
    out.update(act_cond=cond, act_mask=mask, out_act=oa, out_act_masked=om)
    host += [nc.rel(nc.host(tag, params, x, k, cond, dtype=torch.float32), oa),
             nc.rel(nc.host(tag, params, x, k, cond, mask, dtype=torch.float32), om)]

    print("dit facmat narrow sampler trace")
    tag = nc.TRACE_TAG
    small = odit.DiTConfig(**{n: v for n, v in fm.TINY.items() if n not in ("mlp_ratio", "embed_col_dim")})
    cfg = video_cfg(R["AttrDict"], small, sampling_steps=3, hg=dict(name="vanilla", guidance_scale=1.5))
    cfg["backbone"] = R["AttrDict"](nc.cfg(tag))
    algo = R["DFoTVideo"](cfg).eval()
    _, params, keys = make(R, tag, gains[tag])
    algo.diffusion_model.model.load_state_dict(params, strict=True)
    vid = torch.randn(2, 5, 4, 16, 8, generator=g)
    algo.generator = torch.Generator().manual_seed(0)
    with RandnRecorder() as rec:
        pred = algo._predict_videos(vid.clone(), n_context_tokens=2, conditions=None)
    out.update(run_vid=vid, run_pred=pred, run_n_noise=np.array(len(rec.draws)))
    out.update({f"run_noise{i}": d for i, d in enumerate(rec.draws)})
    out["host_rel"] = np.array(max(host))
    print("host restatement (fp32) vs the reference (fp32): rel-L2", host)
    save(nc.FIXTURE, **out)


if __name__ == "__main__":
    main()
