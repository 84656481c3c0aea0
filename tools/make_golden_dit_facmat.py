#!/usr/bin/env python3
"""Generate tests/golden/dit_facmat.npz by executing the reference's own DiT3D (variant "factorized_matrix_attention", pos_emb_type
"sinusoidal_2d", use_temporal_rope: the FacMatDiT backbone of configurations/algorithm/backbone/dit3d_factorized_matrix.yaml) on CPU in
fp32, eval().

Run ONLY in the build container (needs the reference checkout):   python tools/make_golden_dit_facmat.py
Built on tools/ref_loader.py like tools/make_golden_dit_fac.py.  Configuration: tests/dit_facmat_common.TINY (embed_row_dim 128,
embed_col_dim 64, depth 2, 4 spatial heads, patch 1, latents 4x16x8, max_tokens 5) and the four models of dit_facmat_common.CASES
(col x row heads, use_bias, spatial_mlp_ratio, use_temporal_rope).  Weights: dit_facmat_common.seeded_params, one generator per key seeded
from the key's name and shape; the file stores the reference module's ordered key list, the shapes and a digest of the tensors, not the
tensors.

  names_<m>, shapes_<m>, digest_<m>   m in {a, b, c, d, act (model a + action dim 3, dropout 0.1)}
  x, k                                 input [2,5,4,16,8] and integer levels [2,5]
  out_<m>_t5, out_<m>_t3               m in {a, b, c, d}: forward at T = 5 and on the first 3 tokens (the first rows of the RoPE table)
  rope_effect                          rel-L2 between model a's output and the same weights run with use_temporal_rope False
  x_frame4, out_a_frame4, sens_frame4  forward with frame 4 alone perturbed, and the relative change of the OTHER frames' output
  act_cond, act_mask, out_act, out_act_masked
  run_*                                DFoTVideo._predict_videos: 3 DDIM steps, vanilla history guidance 1.5, 2 context tokens, every normal
                                       draw recorded (run_noise<i>), run_vid, run_pred
  host_rel                             the largest fp32 rel-L2 between tests/dit_facmat_common.forward_host and the outputs above, as
                                       measured here (the host test asserts a small margin over it)
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

torch.set_num_threads(8)


def make(R, tag, cond=False, rope=None):
    cc, rr, bias, ratio, case_rope = fm.CASES[tag]
    rope = case_rope if rope is None else rope
    kw = dict(external_cond_type="action", external_cond_num_classes=None, external_cond_dim=fm.COND_DIM if cond else 0)
    model = R["DiT3D"](R["AttrDict"](fm.backbone_cfg(cc, rr, bias, ratio, rope, fm.COND_DROPOUT if cond else 0.0)), x_shape=[4, 16, 8],
                       max_tokens=5, use_causal_mask=False, **kw).eval()
    keys = [(n, tuple(t.shape)) for n, t in model.state_dict().items()]
    assert keys == fm.key_shapes(bias, ratio, fm.COND_DIM if cond else 0, fm.COND_DROPOUT if cond else 0.0), "key_shapes disagrees with the reference"
    params = fm.seeded_params(keys)
    model.load_state_dict(params, strict=True)
    assert (model.dit_base.temporal_rope is not None) == bool(rope)
    return model, params, keys


def meta(out, tag, params, keys):
    out[f"names_{tag}"] = np.array([n for n, _ in keys])
    out[f"shapes_{tag}"] = np.array([" ".join(map(str, s)) for _, s in keys])
    out[f"digest_{tag}"] = np.array(fm.digest(params))


@torch.no_grad()
def main():
    R = ref_loader.install()
    g = torch.Generator().manual_seed(73)
    x = torch.randn(2, 5, 4, 16, 8, generator=g)
    k = torch.randint(0, 1000, (2, 5), generator=g)
    out = dict(x=x, k=k)
    host = []
    for tag, (cc, rr, bias, ratio, rope) in fm.CASES.items():
        print("dit facmat", tag)
        model, params, keys = make(R, tag)
        meta(out, tag, params, keys)
        o5, o3 = model(x, k), model(x[:, :3].contiguous(), k[:, :3].contiguous())
        out[f"out_{tag}_t5"], out[f"out_{tag}_t3"] = o5, o3
        host += [fm.rel(fm.forward_host(params, x, k, cc, rr, rope, dtype=torch.float32), o5),
                 fm.rel(fm.forward_host(params, x[:, :3], k[:, :3], cc, rr, rope, dtype=torch.float32), o3)]
        if tag == "a":
            plain, _, _ = make(R, tag, rope=False)
            out["rope_effect"] = np.array(fm.rel(plain(x, k), o5))
            print("  the rotation moves the output by", float(out["rope_effect"]))
            x4 = x.clone()
            x4[:, 4] = 4.0 * torch.randn(2, 4, 16, 8, generator=g)  # a different, louder frame
            o4 = model(x4, k)
            out["x_frame4"], out["out_a_frame4"] = x4, o4
            out["sens_frame4"] = np.array(fm.rel(o4[:, :4], o5[:, :4]))  # the matrix attention is live: frames 0-3 move
            print("  frames 0-3 move by", float(out["sens_frame4"]), "when frame 4 alone is perturbed")
            host.append(fm.rel(fm.forward_host(params, x4, k, cc, rr, rope, dtype=torch.float32), o4))
    print("dit facmat act")
    cc, rr, bias, ratio, rope = fm.CASES["a"]
    model, params, keys = make(R, "a", cond=True)
    meta(out, "act", params, keys)
    cond = torch.randn(2, 5, fm.COND_DIM, generator=g)
    mask = torch.tensor([True, False])
    oa, om = model(x, k, cond), model(x, k, cond, mask)
    out.update(act_cond=cond, act_mask=mask, out_act=oa, out_act_masked=om)
    host += [fm.rel(fm.forward_host(params, x, k, cc, rr, rope, cond, dtype=torch.float32), oa),
             fm.rel(fm.forward_host(params, x, k, cc, rr, rope, cond, mask, dtype=torch.float32), om)]

    print("dit facmat sampler trace")
    small = odit.DiTConfig(**{n: v for n, v in fm.TINY.items() if n not in ("mlp_ratio", "embed_col_dim")})
    cfg = video_cfg(R["AttrDict"], small, sampling_steps=3, hg=dict(name="vanilla", guidance_scale=1.5))
    cfg["backbone"] = R["AttrDict"](fm.backbone_cfg(cc, rr, bias, ratio, rope))
    algo = R["DFoTVideo"](cfg).eval()
    _, params, keys = make(R, "a")
    algo.diffusion_model.model.load_state_dict(params, strict=True)
    vid = torch.randn(2, 5, 4, 16, 8, generator=g)
    algo.generator = torch.Generator().manual_seed(0)
    with RandnRecorder() as rec:
        pred = algo._predict_videos(vid.clone(), n_context_tokens=2, conditions=None)
    out.update(run_vid=vid, run_pred=pred, run_n_noise=np.array(len(rec.draws)))
    out.update({f"run_noise{i}": d for i, d in enumerate(rec.draws)})
    out["host_rel"] = np.array(max(host))
    print("host restatement (fp32) vs the reference (fp32): rel-L2", host)
    save("dit_facmat.npz", **out)


if __name__ == "__main__":
    main()
