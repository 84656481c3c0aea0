#!/usr/bin/env python3
"""Generate tests/golden/dit_cont.npz: the DiT family under continuous diffusion, by executing the reference's own source on CPU.

Run ONLY in the build container (needs the reference checkout):   python tools/make_golden_dit_cont.py
Built on tools/ref_loader.py like tools/make_golden_dit_cond.py.  Every model is the reference's OWN DiT3D / DifferenceDiT3D with
`use_fourier_noise_embedding: true`, and ContinuousDiffusion (is_continuous, precond_scale 0.125, cosine_simple_diffusion shifted 0.125,
training_schedule cosine / shift 0.125, sigmoid loss weighting) around them, in fp32 at the tiny configuration of the other DiT fixtures
(hidden 128, depth 2, 4 heads, latents 4x16x8, patch 1, max_tokens 5, B = 2; DIFF_TINY for the difference model).  Weights are the seeded
ones of the existing fixtures plus seeded FourierEmbedding buffers (tests/dit_cont_common.py): the file stores inputs, outputs and digests.

  names / diff_names      the reference's state_dict keys in order (the two buffers first)
  levels, x, out          DiT3D unconditioned; the levels include 0.125 * logsnr[0] and 0.125 * logsnr[999]
  feat                    FourierEmbedding's own output for `levels` (the reference module, fp32)
  act_*                   DiT3D action-conditioned (dim 3, dropout 0.1): condition tensors, out with the per-video mask [True, False]
  xd, levels_d, diff_out  the difference model (10 merged tokens)
  trace_*                 DFoTVideo._predict_videos, 3 DDIM steps, vanilla History Guidance 1.5, every normal draw recorded
  train_dit_* / train_diff_*   one ContinuousDiffusion.forward + _reweight_loss + backward: t in [0,1], noise, loss, gradient norm of every
                          parameter, the small gradient tensors (as training_grads.npz)
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
from make_golden_dit import DIFF_TINY, video_cfg  # noqa: E402
from make_golden_dit_cond import SMALL, cond_params  # noqa: E402
from oracle import dit as odit  # noqa: E402
import dit_cont_common as cc  # noqa: E402

torch.set_num_threads(8)

CONT = dict(is_continuous=True, precond_scale=0.125, timesteps=1000, beta_schedule="cosine_simple_diffusion",
            schedule_fn_kwargs=dict(shifted=0.125, interpolated=False), use_causal_mask=False, clip_noise=20.0, objective="pred_v",
            loss_weighting=dict(strategy="sigmoid", sigmoid_bias=-1.0), training_schedule=dict(name="cosine", shift=0.125),
            ddim_sampling_eta=0.0, reconstruction_guidance=0.0)


def cont_video_cfg(A, small, steps, hg, backbone=None):
    cfg = video_cfg(A, small, sampling_steps=steps, hg=hg)
    cfg["diffusion"] = A(dict(CONT, sampling_timesteps=steps))
    if backbone is not None:
        cfg["backbone"] = A(backbone)
    cfg["backbone"]["use_fourier_noise_embedding"] = True
    return cfg


def diff_backbone(oc):
    return dict(name="difference_dit3d", variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", merge_type="interleaved",
                patch_size=1, hidden_size=None, embed_col_dim=oc.embed_col_dim, embed_row_dim=oc.hidden_size, num_heads=oc.num_heads,
                num_col_heads=1, num_row_heads=oc.num_row_heads, depth=oc.depth, mlp_ratio=4.0, spatial_mlp_ratio=4.0, use_bias=True,
                matrix_block="matrix", flatten_matrix_rope=False, matrix_multi_token=False, use_gradient_checkpointing=False)


def load_into(model, params):
    names = list(model.state_dict().keys())
    assert names == list(params.keys()), [n for n in names if n not in params][:4]
    model.load_state_dict(params, strict=True)
    return names


def main():
    R = ref_loader.install()
    A = R["AttrDict"]
    small = odit.DiTConfig(**SMALL)
    oc = odit.DiffDiTConfig(**DIFF_TINY)
    ps = cc.with_buffers(odit.seeded_params(small, 2), 0)
    dps = cc.with_buffers(odit.diff_seeded_params(oc, 3), 1)
    lo, hi = cc.logsnr_extremes()
    out = dict(digest=np.array(cc.digest(ps)), digest_diff=np.array(cc.digest(dps)))
    g = torch.Generator().manual_seed(51)

    with torch.no_grad():
        print("dit3d, float levels")
        algo = R["DFoTVideo"](cont_video_cfg(A, small, 3, dict(name="vanilla", guidance_scale=1.5))).eval()
        dm = algo.diffusion_model
        assert abs(float(dm.precond_scale * dm.logsnr[0]) - lo) < 1e-6 and abs(float(dm.precond_scale * dm.logsnr[999]) - hi) < 1e-6
        model = dm.model
        out["names"] = np.array(load_into(model, ps))
        x = torch.randn(2, 5, 4, 16, 8, generator=g)
        levels = 2.5 * torch.randn(2, 5, generator=g)
        levels[0, 0], levels[1, 4], levels[0, 2] = lo, hi, 0.0
        out.update(x=x, levels=levels, out=model(x, levels), feat=model.noise_level_pos_embedding.timesteps(levels))

        print("sampler trace")
        vid = torch.randn(2, 5, 4, 16, 8, generator=g)
        algo.generator = torch.Generator().manual_seed(0)
        with RandnRecorder() as rec:
            pred = algo._predict_videos(vid.clone(), n_context_tokens=2, conditions=None)
        out.update(trace_vid=vid, trace_pred=pred, trace_n_noise=np.array(len(rec.draws)))
        out.update({f"trace_noise{i}": d for i, d in enumerate(rec.draws)})

        print("dit3d, action condition")
        bc = dict(name="dit3d", variant="full", pos_emb_type="rope_3d", patch_size=1, hidden_size=128, depth=2, num_heads=4, mlp_ratio=4.0,
                  use_gradient_checkpointing=False, external_cond_dropout=0.1, use_fourier_noise_embedding=True)
        am = R["DiT3D"](A(bc), x_shape=[4, 16, 8], max_tokens=5, external_cond_type="action", external_cond_num_classes=None,
                        external_cond_dim=3, use_causal_mask=False).eval()
        cp = cond_params(am, 12)
        names = list(am.state_dict().keys())
        am.load_state_dict({**ps, **cp}, strict=True)
        cond = torch.randn(2, 5, 3, generator=g)
        mask = torch.tensor([True, False])
        out.update(act_names=np.array(names), act_cond=cond, act_mask=mask, act_out=am(x, levels, cond, mask), act_out_nomask=am(x, levels, cond))
        out.update({f"act_cond/{n}": t for n, t in cp.items()})

        print("difference dit, float levels")
        dalgo = R["DifferenceDFoTVideo"](cont_video_cfg(A, small, 3, dict(name="conditional"), diff_backbone(oc))).eval()
        dmodel = dalgo.diffusion_model.model
        out["diff_names"] = np.array(load_into(dmodel, dps))
        xd = torch.randn(2, 10, 4, 16, 8, generator=g)
        ld = 2.5 * torch.randn(2, 10, generator=g)
        ld[0, 0], ld[0, 1], ld[1, 8], ld[1, 9] = lo, lo, hi, hi
        out.update(xd=xd, levels_d=ld, diff_out=dmodel(xd, ld))

    print("training steps")
    xs = torch.randn(2, 5, 4, 16, 8, generator=g)
    t = torch.rand(2, 5, generator=g)
    t[0, 0], t[1, 4] = 0.0, 1.0
    masks = torch.ones(2, 5)
    masks[1, 3] = 0
    algo.train()
    dalgo.train()
    for tag, al in (("dit", algo), ("diff", dalgo)):
        model = al.diffusion_model.model
        for p_ in model.parameters():
            p_.grad = None
        if tag == "diff":
            x_in = al.merge_tensors(torch.diff(xs, dim=1, prepend=xs[:, :1]), xs)
            k_in, m_in = al.merge_tensors(t, t), al.merge_tensors(masks, masks)
        else:
            x_in, k_in, m_in = xs, t, masks
        with torch.enable_grad(), RandnRecorder() as rec:
            _, loss = al.diffusion_model(x_in, None, k=k_in)
            loss = al._reweight_loss(loss, m_in)
            loss.backward()
        grads = {n: p_.grad.detach().clone() for n, p_ in model.named_parameters()}
        assert cc.FREQS not in grads and cc.PHASES not in grads
        out.update({f"train_{tag}_loss": loss.detach(), f"train_{tag}_noise": rec.draws[0], f"train_{tag}_names": np.array(list(grads)),
                    f"train_{tag}_norms": np.array([float(v.norm()) for v in grads.values()], np.float64)})
        for n, v in grads.items():
            if v.numel() <= 4096 or n.endswith(("attn.qkv_u", "attn.proj_u")):
                out[f"train_{tag}_grad/{n}"] = v
    out.update(train_xs=xs, train_t=t, train_masks=masks)
    save("dit_cont.npz", **out)


if __name__ == "__main__":
    main()
