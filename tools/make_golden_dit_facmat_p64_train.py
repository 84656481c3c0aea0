#!/usr/bin/env python3
"""Generate tests/golden/dit_facmat_p64_train.npz by executing the reference's own DFoTVideo training loss with the reference's DiT3D
(variant "factorized_matrix_attention", pos_emb_type "sinusoidal_2d": the FacMatDiT backbone) at 64 patches per frame on CPU in fp32,
differentiated by the reference's autograd.  tools/make_golden_dit_facmat_train.py restated at the geometry of tests/dit_p64_common.py:
latents 4x16x16 at patch_size 2, the shape of the taichi res-128 recipes
(bash/taichikl/resolution_128/train_dfot_facmat-s-{64-1,64-4,64-16,128-1}-bias_*.sh).

Run ONLY in the build container (needs the reference checkout):   python tools/make_golden_dit_facmat_p64_train.py
Built on tools/ref_loader.py.  Discrete diffusion, cosine schedule, pred_v, fused_min_snr with cum_snr_decay 0.96, _reweight_loss with one
masked token; backbone embed_row_dim 128, depth 2, 4 spatial heads, max_tokens 4; the two cases of
dit_facmat_p64_train_common.TRAIN_CASES (b: embed_col_dim 64, 2 column heads, 2 row heads, biases, spatial MLP 4, temporal RoPE; e128:
embed_col_dim 128, 1 column head, 4 row heads, none of the three), weights from seeded_params; input B = 2, T = 4.

  xs, k, masks                  the batch [2,4,4,16,16], integer levels [2,4], loss masks [2,4] (one zero)
  <m>_noise, <m>_loss           m in {b, e128}: the recorded normal draw of DiscreteDiffusion.forward and the reweighted loss
  <m>_names, <m>_norms          ordered parameter names and the norm of every gradient (float64)
  <m>_digest                    digest of the weights
  <m>_grad/<name>               gradient tensors with <= 4096 elements (attn.qkv_u / attn.proj_u of case b among them: 64 x 64)
  host_rel, host_loss_rel       the largest gradient rel-L2 / loss deviation of the host restatement (fp32 autograd through
                                dit_facmat_common.forward_host at this geometry + oracle.sampler.discrete_training_loss,
                                tests/dit_facmat_p64_train_common.host_loss_and_grads) against the above, as measured here
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
import dit_p64_common as pc  # noqa: E402
import dit_facmat_p64_train_common as ft  # noqa: E402

torch.set_num_threads(8)


@torch.enable_grad()
def main():
    R = ref_loader.install()
    torch.manual_seed(17)  # the reference draws the training noise from the default generator (the draw is recorded all the same)
    A = R["AttrDict"]
    g = torch.Generator().manual_seed(94)
    xs = torch.randn(pc.BATCH, pc.MAX_TOKENS, *pc.X_SHAPE, generator=g)
    k = torch.randint(0, 1000, (pc.BATCH, pc.MAX_TOKENS), generator=g)
    masks = torch.ones(pc.BATCH, pc.MAX_TOKENS)
    masks[1, 2] = 0
    out = {}
    host, host_loss = [], []
    small = odit.DiTConfig(**{n: v for n, v in {**fm.TINY, **pc.OVER}.items() if n not in ("mlp_ratio", "embed_col_dim")})
    for tag in ft.TRAIN_CASES:
        print("dit facmat p64 train", tag)
        (cc, rr, bias, ratio, rope), over = ft.MODELS[tag]
        cfg = video_cfg(A, small, sampling_steps=3, hg=dict(name="conditional"))
        cfg["backbone"] = A(ft.cfg(tag))
        algo = R["DFoTVideo"](cfg).train()
        model = algo.diffusion_model.model
        keys = [(n, tuple(t.shape)) for n, t in model.state_dict().items()]
        # b is a case of dit_facmat_common.CASES; e128 has the keys of case a (no bias, no spatial MLP) at embed_col_dim 128
        assert keys == pc.mat_keys("b" if tag == "b" else "a", **over), "key_shapes disagrees with the reference"
        assert keys == ft.keys(tag)
        params = fm.seeded_params(keys)
        model.load_state_dict(params, strict=True)
        assert (model.dit_base.temporal_rope is not None) == bool(rope)
        for p_ in model.parameters():
            p_.grad = None
        with RandnRecorder() as rec:
            _, loss = algo.diffusion_model(xs, None, k=k)
        loss = algo._reweight_loss(loss, masks)
        loss.backward()
        grads = {n: p_.grad.detach().clone() for n, p_ in model.named_parameters()}
        assert list(grads) == [n for n, _ in keys]
        out[f"{tag}_loss"] = loss.detach()
        out[f"{tag}_noise"] = rec.draws[0]
        out[f"{tag}_names"] = np.array(list(grads))
        out[f"{tag}_norms"] = np.array([float(v.norm()) for v in grads.values()], np.float64)
        assert min(out[f"{tag}_norms"]) > 0
        for n, v in grads.items():
            if v.numel() <= 4096:
                out[f"{tag}_grad/{n}"] = v
        out[f"{tag}_digest"] = np.array(fm.digest(params))
        hl, hg = ft.host_loss_and_grads(tag, xs, k, torch.as_tensor(rec.draws[0]), masks)
        ref_loss = float(out[f"{tag}_loss"])
        host_loss.append(abs(float(hl) - ref_loss) / abs(ref_loss))
        host.append(max(fm.rel(hg[n], grads[n]) for n in grads))
        print(f"  loss {ref_loss:.6f}; restatement: loss deviation {host_loss[-1]:.2e}, worst gradient rel-L2 {host[-1]:.2e}")
    out["host_rel"] = np.array(max(host))
    out["host_loss_rel"] = np.array(max(host_loss))
    save(ft.FIXTURE, xs=xs, k=k, masks=masks, **out)


if __name__ == "__main__":
    main()
