#!/usr/bin/env python3
"""Generate tests/golden/uvit3d_train.npz by executing the reference's own continuous-diffusion training loss with the reference's UViT3D
(algorithms/dfot/backbones/u_vit/u_vit3d.py) on CPU in fp32, train(), differentiated by the reference's autograd.

Run ONLY in the build container (needs the reference checkout):   python tools/make_golden_uvit3d_train.py
Built on tools/ref_loader.py like tools/make_golden_dit_fac_train.py.  ContinuousDiffusion (tools/make_golden_dit_cont.CONT: cosine training
schedule with shift 0.125, pred_v, sigmoid weighting, precond_scale 0.125), _reweight_loss with one masked token; backbone at
tests/uvit3d_common.TINY, constructed directly and assigned to diffusion_model.model as tools/make_golden_uvit3d.py does (the algorithm cannot
build a "u_vit3d" backbone from its config); cases a (no condition) and c (actions, dropout 0.1) of uvit3d_common.CASES.  In train() the
reference draws the per-video condition dropout itself (RandomEmbeddingDropout, embeddings.py:356-357: torch.rand(B) < p); the one draw is
served here so that the first video is dropped (uvit3d_train_common.DROP), and counted.

  inputs_digest, masks          digest of uvit3d_train_common.train_inputs() (xs [2,8,3,64,64], t [2,8], actions [2,8,4]: drawn from a seed, not
                                stored -- one frame tensor is 786 KB) and the loss masks [2,8] (one zero)
  noise_seed, noise_shape, noise_digest   the normal draw of ContinuousDiffusion.forward, served from uvit3d_train_common.train_noise()'s generator
                                and recorded: its seed, shape and digest (the tensor is as large as xs)
  <m>_loss                      m in {a, c}: the reweighted loss
  <m>_names, <m>_norms          ordered parameter names and the norm of every gradient (float64)
  <m>_digest                    digest of the weights
  <m>_grad/<name>               gradient tensors with <= 4096 elements
  c_drop                        the condition-dropout mask the reference used in case c
  host_rel, host_loss_rel       the largest gradient rel-L2 / loss deviation of the host restatement (fp32 autograd through
                                uvit3d_common.forward_host + oracle.sampler.training_loss, uvit3d_train_common.host_loss_and_grads) against the
                                above, as measured here
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
from make_golden_dit_cont import cont_video_cfg  # noqa: E402
from make_golden_uvit3d import SeededRandn, make  # noqa: E402
from oracle import dit as odit  # noqa: E402
import uvit3d_common as uc  # noqa: E402
import uvit3d_train_common as ut  # noqa: E402

torch.set_num_threads(8)


class ServedRand:
    """While active, torch.rand of shape (B,) -- the per-video condition dropout draw -- returns 0 where `drop` is set and 1 elsewhere"""

    def __init__(self, drop):
        self.drop, self.calls, self._rand = drop, 0, torch.rand

    def __enter__(self):
        me = self

        def rand(*size, **k):
            shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
            if shape == tuple(me.drop.shape):
                me.calls += 1
                return (~me.drop).to(torch.float32).to(device=k.get("device"))
            return me._rand(*size, **k)
        torch.rand = rand
        return self

    def __exit__(self, *a):
        torch.rand = self._rand


@torch.enable_grad()
def main():
    R = ref_loader.install()
    A = R["AttrDict"]
    xs, t, masks, cond = ut.train_inputs()
    out = dict(inputs_digest=np.array(uc.tensor_digest(xs, t, cond)), masks=masks, noise_seed=np.array(ut.NOISE_SEED))
    small = odit.DiTConfig(hidden_size=128, depth=1, num_heads=2, patch_size=2, in_channels=uc.X_SHAPE[0], resolution=uc.X_SHAPE[1:],
                           max_tokens=uc.MAX_TOKENS)
    host, host_loss = [], []
    for tag in ut.TRAIN_CASES:
        print("uvit3d train", tag)
        dim, drop = uc.CASES[tag]
        cfg = cont_video_cfg(A, small, 3, dict(name="vanilla", guidance_scale=1.5))
        cfg["external_cond_dim"] = dim
        algo = R["DFoTVideo"](cfg).train()
        model, params, keys = make(R, tag)
        algo.diffusion_model.model = model.train()
        for p_ in model.parameters():
            p_.grad = None
        c_in, c_drop = ut.case_cond(tag)
        with SeededRandn(ut.NOISE_SEED), RandnRecorder() as rec, ServedRand(ut.DROP) as served:
            _, loss = algo.diffusion_model(xs, c_in, k=t)
        loss = algo._reweight_loss(loss, masks)
        loss.backward()
        assert len(rec.draws) == 1 and torch.equal(torch.as_tensor(rec.draws[0]), ut.train_noise()), "the recorded draw is not the seeded one"
        assert served.calls == (1 if c_drop is not None else 0), served.calls
        grads = {n: p_.grad.detach().clone() for n, p_ in model.named_parameters()}
        assert list(grads) == ut.trainable(params)
        out[f"{tag}_loss"] = loss.detach()
        out[f"{tag}_names"] = np.array(list(grads))
        out[f"{tag}_norms"] = np.array([float(v.norm()) for v in grads.values()], np.float64)
        assert min(out[f"{tag}_norms"]) > 0
        for n, v in grads.items():
            if v.numel() <= 4096:
                out[f"{tag}_grad/{n}"] = v
        out[f"{tag}_digest"] = np.array(uc.digest(params))
        if c_drop is not None:
            out[f"{tag}_drop"] = c_drop
        hl, hg = ut.host_loss_and_grads(tag)
        ref_loss = float(out[f"{tag}_loss"])
        host_loss.append(abs(float(hl) - ref_loss) / abs(ref_loss))
        host.append(max(uc.rel(hg[n], grads[n]) for n in grads))
        print(f"  loss {ref_loss:.6f}; restatement: loss deviation {host_loss[-1]:.2e}, worst gradient rel-L2 {host[-1]:.2e}")
    noise = ut.train_noise()
    out.update(noise_shape=np.array(noise.shape), noise_digest=np.array(uc.tensor_digest(noise)))
    out["host_rel"] = np.array(max(host))
    out["host_loss_rel"] = np.array(max(host_loss))
    save("uvit3d_train.npz", **out)


if __name__ == "__main__":
    main()
