#!/usr/bin/env python3
"""Generate tests/golden/dit1d.npz by executing the reference's own DIT1D (algorithms/dfot/backbones/dit1d/dit_model.py) on CPU in fp32,
eval().

Run ONLY in the build container (needs the reference checkout):   python tools/make_golden_dit1d.py
Built on tools/ref_loader.py (install_dit1d) like tools/make_golden_uvit3d.py.  Configuration: tests/dit1d_common.TINY (hidden 128, depth 2,
C 4, L 32, max_tokens 8, batch 2: N = 256 tokens, two 128-row query tiles) with 4 heads (head dim 32, tag h4) and 2 heads (head dim 64, h2).
Weights: dit1d_common.seeded_params, one generator per key; the q and k rows of qkv.weight carry a gain, started at dit1d_common.QK_GAIN and
raised here until every sensitivity below reaches dit1d_common.SENS_FLOOR (5 x the parity bar), so that an engine with no mask, a wrong mask
or the un-normalised residual base stays at least four bars away from a pass.  The file holds data only:

  qk_gain                               the gain the loop ended at (the tests build their weights with it)
  names_<tag>, shapes_<tag>, digest_<tag>   the reference module's ordered key list, the shapes, a digest of the seeded tensors
  inputs_digest                         digest of dit1d_common.inputs() (x [2,8,4,1,32], integer levels [2,8]: drawn from a fixed seed)
  out_causal_<tag>, out_nomask_<tag>    the reference's outputs under causal_attn_mode video_temporal_causal and null
  same_modes                            1: temporal_causal gave the bits of video_temporal_causal (no context tokens: the same mask)
  sens_nomask / sens_tokencausal / sens_transposed / sens_residual
                                        rel-L2 between the reference's causal output and dit1d_common.forward_host (fp64) run with no mask, a
                                        per-token causal mask, the transposed mask, the un-normalised residual base: the smaller of the two tags
  host_rel                              the largest fp32 rel-L2 between dit1d_common.forward_host and the reference outputs
  sincos_hidden, sincos_tokens, sincos  get_1d_sincos_pos_embed of the reference at a small size (what a fresh model's pos_embed holds)
  run_*                                 DFoTVideo._predict_videos around the reference's DIT1D (h4; assigned to diffusion_model.model) under
                                        DiscreteDiffusion: 3 DDIM steps, vanilla history guidance 1.5, 2 context tokens; every normal draw is
                                        served by one seeded generator and recorded by shape and digest (run_draw_shapes, run_draws_digest);
                                        run_inputs_digest, run_pred, run_qk_gain (the gain of the trace's weights)
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
from make_golden_uvit3d import SeededRandn  # noqa: E402
from oracle import dit as odit  # noqa: E402
import dit1d_common as dc  # noqa: E402

torch.set_num_threads(8)
RUN_QK_GAIN = 1.0  # the sampler trace runs the un-gained weights: three guided steps on a sharp softmax amplify bf16 rounding, not mistakes


def make(DIT1D, A, tag, gain, mode="video_temporal_causal"):
    heads = dc.CASES[tag]
    model = DIT1D(A(dc.backbone_cfg(heads, causal_attn_mode=mode)), x_shape=list(dc.X_SHAPE), max_tokens=dc.MAX_TOKENS, external_cond_type=None,
                  external_cond_num_classes=None, external_cond_dim=0, use_causal_mask=True).eval()
    keys = [(n, tuple(t.shape)) for n, t in model.state_dict().items()]
    assert keys == dc.key_shapes(heads), "key_shapes disagrees with the reference"
    params = dc.seeded_params(keys, gain)
    assert all(bool((t != 0).any()) for t in params.values())
    model.load_state_dict(params, strict=True)
    return model, params, keys


@torch.no_grad()
def main():
    R = ref_loader.install()
    DIT1D, module = ref_loader.install_dit1d()
    A = R["AttrDict"]
    x, k = dc.inputs()
    gain = dc.QK_GAIN
    while True:
        out = dict(inputs_digest=np.array(dc.tensor_digest(x, k)), qk_gain=np.array(gain))
        host, sens = [], {name: [] for name in dc.SENSITIVITIES}
        same = True
        for tag, heads in dc.CASES.items():
            model, params, keys = make(DIT1D, A, tag, gain)
            out[f"names_{tag}"] = np.array([n for n, _ in keys])
            out[f"shapes_{tag}"] = np.array([" ".join(map(str, s)) for _, s in keys])
            out[f"digest_{tag}"] = np.array(dc.digest(params))
            oc = model(x, k)
            on = make(DIT1D, A, tag, gain, None)[0](x, k)
            same = same and torch.equal(make(DIT1D, A, tag, gain, "temporal_causal")[0](x, k), oc)
            assert tuple(oc.shape) == tuple(x.shape)
            out[f"out_causal_{tag}"], out[f"out_nomask_{tag}"] = oc, on
            host += [dc.rel(dc.forward_host(params, x, k, heads, dtype=torch.float32), oc),
                     dc.rel(dc.forward_host(params, x, k, heads, mask="none", dtype=torch.float32), on)]
            for name, kw in dc.SENSITIVITIES.items():
                sens[name].append(dc.rel(dc.forward_host(params, x, k, heads, **kw), oc))
        print(f"gain {gain}: sensitivities {sens}; host restatement (fp32) vs the reference rel-L2 {host}")
        if all(min(v) >= dc.SENS_FLOOR for v in sens.values()):
            break
        gain += 2.0
        assert gain <= 16.0, "the sensitivities do not reach the floor"
    out.update({name: np.array(min(v)) for name, v in sens.items()})
    out.update(host_rel=np.array(max(host)), same_modes=np.array(int(same)))
    out.update(sincos_hidden=np.array(16), sincos_tokens=np.array(40), sincos=module.get_1d_sincos_pos_embed(16, 40))

    print("dit1d sampler trace")
    # the algorithm is built around a stand-in backbone of the same x_shape / max_tokens (as tools/make_golden_uvit3d.py does); the
    # reference's own DIT1D module, constructed directly as above, takes its place before anything runs
    small = odit.DiTConfig(hidden_size=128, depth=1, num_heads=2, patch_size=1, in_channels=dc.X_SHAPE[0], resolution=dc.X_SHAPE[1:],
                           max_tokens=dc.MAX_TOKENS)
    algo = R["DFoTVideo"](video_cfg(A, small, sampling_steps=3, hg=dict(name="vanilla", guidance_scale=1.5))).eval()
    model, params, _ = make(DIT1D, A, "h4", RUN_QK_GAIN)
    algo.diffusion_model.model = model
    vid = dc.trace_inputs()
    algo.generator = torch.Generator().manual_seed(dc.DRAW_SEED)
    with SeededRandn(dc.DRAW_SEED), RandnRecorder() as rec:
        pred = algo._predict_videos(vid.clone(), n_context_tokens=2, conditions=None)
    shapes = [tuple(d.shape) for d in rec.draws]
    again = dc.trace_draws(shapes)
    assert len(shapes) > 0 and all(torch.equal(d, r) for d, r in zip(rec.draws, again)), "the recorded draws are not the seeded sequence"
    assert torch.equal(pred[:, :2], vid[:, :2])
    out.update(run_inputs_digest=np.array(dc.tensor_digest(vid)), run_pred=pred, run_qk_gain=np.array(RUN_QK_GAIN),
               run_digest=np.array(dc.digest(params)),
               run_draw_shapes=np.array([" ".join(map(str, sh)) for sh in shapes]), run_draws_digest=np.array(dc.tensor_digest(*rec.draws)))
    save(dc.FIXTURE, **out)


if __name__ == "__main__":
    main()
