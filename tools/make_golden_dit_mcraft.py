#!/usr/bin/env python3
"""Generate tests/golden/dit_mcraft.npz: the Minecraft / dmlab DiT recipe's geometry, by executing the reference's own source on CPU.

Run ONLY in the build container (needs the reference checkout):   python tools/make_golden_dit_mcraft.py
Built on tools/ref_loader.py like tools/make_golden_dit_cont.py.  The model is the reference's OWN DiT3D ("full", rope_3d,
`use_fourier_noise_embedding: true`) at x_shape (32, 8, 8), patch 2, max_tokens 16 -- a 128-wide patch vector, 16 patches per frame -- with
hidden 384, depth 2, 6 heads (tests/dit_mcraft_common.FIX), and ContinuousDiffusion around it as in make_golden_dit_cont.CONT.  Weights are
seeded (dit_mcraft_common.seeded_params) and NOT stored: the file holds their sha256, inputs and results.

  names / act_names       the reference's state_dict keys in order, unconditioned / action-conditioned (dim 4, dropout 0.1)
  digest / act_digest     sha256 over (key, bytes) in that order
  x, levels, out          eval forward, unconditioned, B = 2, T = 8
  cond, mask, act_out     the same inputs with actions and the per-video mask [True, False]
  train_*                 one ContinuousDiffusion.forward + _reweight_loss + backward of the action-conditioned model on xs = x (mask_first
                          actions, the per-video condition dropout fixed to train_dropmask): t, noise, loss, every parameter's gradient norm,
                          the full gradients of the final linear and of the patch embedding
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
from make_golden_dit_cond import cond_params  # noqa: E402
from make_golden_dit_cont import CONT  # noqa: E402
import dit_cont_common as cc  # noqa: E402
import dit_mcraft_common as mc  # noqa: E402

torch.set_num_threads(8)

STORED_GRADS = ("dit_base.final_layer.linear.weight", "dit_base.final_layer.linear.bias", "patch_embedder.proj.weight", "patch_embedder.proj.bias")
B, T = 2, 8


def weights(module, cfg, action):
    """the seeded tensors in the module's own key order; the condition draws are checked against the reference-keyed ones"""
    names = list(module.state_dict().keys())
    p = mc.seeded_params(cfg, action, names)
    if action:
        for n, t in cond_params(module, 12).items():
            assert torch.equal(p[n], t), n
    module.load_state_dict(p, strict=True)
    return names, p


def main():
    R = ref_loader.install()
    A = R["AttrDict"]
    cfg = mc.ocfg()
    g = torch.Generator().manual_seed(61)
    lo, hi = cc.logsnr_extremes()
    x = torch.randn(B, T, *mc.X_SHAPE, generator=g)
    levels = 2.5 * torch.randn(B, T, generator=g)
    levels[0, 0], levels[1, T - 1], levels[0, 2] = lo, hi, 0.0
    cond = torch.randn(B, T, mc.COND_DIM, generator=g)
    mask = torch.tensor([True, False])
    out = dict(x=x, levels=levels, cond=cond, mask=mask)

    def build(action):
        bc = dict(mc.backbone_cfg(cfg, mc.DROPOUT if action else 0.0), use_gradient_checkpointing=False)
        return R["DiT3D"](A(bc), x_shape=list(mc.X_SHAPE), max_tokens=mc.MAX_TOKENS, external_cond_type="action", external_cond_num_classes=None,
                          external_cond_dim=mc.COND_DIM if action else 0, use_causal_mask=False).eval()

    with torch.no_grad():
        print("unconditioned forward")
        m = build(False)
        names, p = weights(m, cfg, False)
        out.update(names=np.array(names), digest=np.array(cc.digest(p)), out=m(x, levels))
        print("action-conditioned forward")
        am = build(True)
        names, p = weights(am, cfg, True)
        out.update(act_names=np.array(names), act_digest=np.array(cc.digest(p)), act_out=am(x, levels, cond, mask))

    print("training step")
    vc = video_cfg(A, cfg, sampling_steps=3, hg=dict(name="conditional"))
    vc["diffusion"] = A(dict(CONT, sampling_timesteps=3))
    vc["backbone"]["use_fourier_noise_embedding"] = True
    vc["backbone"]["external_cond_dropout"] = mc.DROPOUT
    vc["external_cond_type"], vc["external_cond_dim"], vc["external_cond_processing"] = "action", mc.COND_DIM, "mask_first"
    algo = R["DFoTVideo"](vc).train()
    model = algo.diffusion_model.model
    weights(model, cfg, True)
    t = torch.rand(B, T, generator=g)
    t[0, 0], t[1, T - 1] = 0.0, 1.0
    masks = torch.ones(B, T)
    masks[1, 3] = 0
    drop = torch.tensor([False, True])
    real_rand = torch.rand

    def fixed_rand(*a, **kw):  # RandomEmbeddingDropout: torch.rand(emb.shape[:1]) < p  -> the stored per-video mask
        shape = a[0] if len(a) == 1 and not isinstance(a[0], int) else a
        if tuple(shape) == (B,):
            return torch.where(drop, torch.zeros(B), torch.ones(B))
        return real_rand(*a, **kw)
    torch.rand = fixed_rand
    try:
        with RandnRecorder() as rec:
            _, loss = algo.diffusion_model(x, algo._process_conditions(cond.clone()), k=t)
    finally:
        torch.rand = real_rand
    loss = algo._reweight_loss(loss, masks)
    loss.backward()
    grads = {n: p_.grad.detach().clone() for n, p_ in model.named_parameters()}
    assert cc.FREQS not in grads and cc.PHASES not in grads
    out.update(train_t=t, train_masks=masks, train_dropmask=drop, train_noise=rec.draws[0], train_loss=loss.detach(),
               train_names=np.array(list(grads)), train_norms=np.array([float(v.norm()) for v in grads.values()], np.float64))
    for n in STORED_GRADS:
        out[f"train_grad/{n}"] = grads[n]
    save("dit_mcraft.npz", **out)


if __name__ == "__main__":
    main()
