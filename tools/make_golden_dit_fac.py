#!/usr/bin/env python3
"""Generate tests/golden/dit_fac.npz by executing the reference's own DiT3D (variant "factorized_attention", pos_emb_type
"sinusoidal_factorized") on CPU in fp32, eval().

Run ONLY in the build container (needs the reference checkout):   python tools/make_golden_dit_fac.py
Built on tools/ref_loader.py like tools/make_golden_dit_cond.py.  Configuration: tests/dit_fac_common.TINY (hidden 128, depth 2, 4 heads,
patch 1, latents 4x16x8, max_tokens 5).  Weights: dit_fac_common.seeded_params, one generator per key seeded from the key's name and
shape; the file stores the reference module's ordered key list, the shapes and a digest of the tensors, not the tensors.

  names_<m>, shapes_<m>, digest_<m>   m in {mlp0 (spatial_mlp_ratio 0.0), mlp4 (4.0), act (mlp0 + action dim 3, dropout 0.1)}
  x, k                                 input [2,5,4,16,8] and integer levels [2,5]
  out_<m>_t5, out_<m>_t3               m in {mlp0, mlp4}: forward at T = 5 and on the first 3 tokens
  out_mlp0_frame4, sens_frame4         forward with frame 4 alone perturbed, and the relative change of the OTHER frames' output
  tpos_t5                              the module's temporal table (first 5 rows)
  act_cond, act_mask, out_act, out_act_masked
  run_*                                DFoTVideo._predict_videos: 3 DDIM steps, vanilla history guidance 1.5, 2 context tokens, every normal
                                       draw recorded (run_noise<i>), run_vid, run_pred
  host_rel                             the largest fp32 rel-L2 between tests/dit_fac_common.forward_host and the outputs above, as measured
                                       here (the host test asserts a small margin over it)
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
import dit_fac_common as fc  # noqa: E402

torch.set_num_threads(8)


def make(R, ratio, cond=False):
    A = R["AttrDict"]
    kw = dict(external_cond_type="action", external_cond_num_classes=None, external_cond_dim=fc.COND_DIM if cond else 0)
    model = R["DiT3D"](A(fc.backbone_cfg(ratio, fc.COND_DROPOUT if cond else 0.0)), x_shape=[4, 16, 8], max_tokens=5, use_causal_mask=False,
                       **kw).eval()
    sd = model.state_dict()
    keys = [(n, tuple(t.shape)) for n, t in sd.items()]
    assert keys == fc.key_shapes(ratio, fc.COND_DIM if cond else 0, fc.COND_DROPOUT if cond else 0.0), "key_shapes disagrees with the reference"
    params = fc.seeded_params(keys)
    model.load_state_dict(params, strict=True)
    return model, params, keys


def meta(out, tag, params, keys):
    out[f"names_{tag}"] = np.array([n for n, _ in keys])
    out[f"shapes_{tag}"] = np.array([" ".join(map(str, s)) for _, s in keys])
    out[f"digest_{tag}"] = np.array(fc.digest(params))


@torch.no_grad()
def main():
    R = ref_loader.install()
    g = torch.Generator().manual_seed(71)
    x = torch.randn(2, 5, 4, 16, 8, generator=g)
    k = torch.randint(0, 1000, (2, 5), generator=g)
    out = dict(x=x, k=k)
    host = []
    for tag, ratio in (("mlp0", 0.0), ("mlp4", 4.0)):
        print("dit fac", tag)
        model, params, keys = make(R, ratio)
        meta(out, tag, params, keys)
        o5, o3 = model(x, k), model(x[:, :3].contiguous(), k[:, :3].contiguous())
        out[f"out_{tag}_t5"], out[f"out_{tag}_t3"] = o5, o3
        host += [fc.rel(fc.forward_host(params, x, k, dtype=torch.float32), o5),
                 fc.rel(fc.forward_host(params, x[:, :3], k[:, :3], dtype=torch.float32), o3)]
        if tag == "mlp0":
            out["tpos_t5"] = model.dit_base.temporal_pos_emb.pos_emb[0, :5].clone()
            x4 = x.clone()
            x4[:, 4] = 4.0 * torch.randn(2, 4, 16, 8, generator=g)  # a different, louder frame
            o4 = model(x4, k)
            out["x_frame4"], out["out_mlp0_frame4"] = x4, o4
            out["sens_frame4"] = np.array(fc.rel(o4[:, :4], o5[:, :4]))  # the temporal path is live: frames 0-3 move
            print("  frames 0-3 move by", float(out["sens_frame4"]), "when frame 4 alone is perturbed")
            host.append(fc.rel(fc.forward_host(params, x4, k, dtype=torch.float32), o4))
    print("dit fac act")
    model, params, keys = make(R, 0.0, cond=True)
    meta(out, "act", params, keys)
    cond = torch.randn(2, 5, fc.COND_DIM, generator=g)
    mask = torch.tensor([True, False])
    oa, om = model(x, k, cond), model(x, k, cond, mask)
    out.update(act_cond=cond, act_mask=mask, out_act=oa, out_act_masked=om)
    host += [fc.rel(fc.forward_host(params, x, k, cond, dtype=torch.float32), oa),
             fc.rel(fc.forward_host(params, x, k, cond, mask, dtype=torch.float32), om)]

    print("dit fac sampler trace")
    small = odit.DiTConfig(**{n: v for n, v in fc.TINY.items() if n != "mlp_ratio"})
    cfg = video_cfg(R["AttrDict"], small, sampling_steps=3, hg=dict(name="vanilla", guidance_scale=1.5))
    cfg["backbone"] = R["AttrDict"](fc.backbone_cfg(0.0))
    algo = R["DFoTVideo"](cfg).eval()
    _, params, keys = make(R, 0.0)
    algo.diffusion_model.model.load_state_dict(params, strict=True)
    vid = torch.randn(2, 5, 4, 16, 8, generator=g)
    algo.generator = torch.Generator().manual_seed(0)
    with RandnRecorder() as rec:
        pred = algo._predict_videos(vid.clone(), n_context_tokens=2, conditions=None)
    out.update(run_vid=vid, run_pred=pred, run_n_noise=np.array(len(rec.draws)))
    out.update({f"run_noise{i}": d for i, d in enumerate(rec.draws)})
    out["host_rel"] = np.array(max(host))
    print("host restatement (fp32) vs the reference (fp32): rel-L2", host)
    save("dit_fac.npz", **out)


if __name__ == "__main__":
    main()
