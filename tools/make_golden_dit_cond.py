#!/usr/bin/env python3
"""Generate the fixtures of the action / label conditioned DiT family under tests/golden/ by executing the reference's own source on CPU.

Run ONLY in the build container (needs the reference checkout):   python tools/make_golden_dit_cond.py
Built on tools/ref_loader.py like tools/make_golden_dit.py.  Every model is the reference's OWN DiT3D / DifferenceDiT3D in fp32 at the
tiny configuration of the existing DiT fixtures (hidden 128, depth 2, 4 heads, 16x8 latents, 5 tokens; DIFF_TINY for the difference
model).  Weights: oracle.dit.seeded_params / diff_seeded_params for the tensors every model has (non-zero modulations -- the reference's
zero init would make the condition invisible) plus seeded tensors for the reference module's `external_cond_embedding.*` keys, stored in
the file; the key list of the reference's state_dict is stored in order.

  dit_cond.npz     per mode m in {act_d0 (action dim 3, dropout 0), act_d1 (dropout 0.1), label (101 classes), diff_act (difference model,
                   action dim 3, dropout 0.1)}:  <m>_names, <m>_cond/<key> (condition-embedding tensors), <m>_cond (the condition),
                   <m>_out (forward with it), <m>_mask_ignored (whether external_cond_mask = [True, False] left the output unchanged: an
                   action module built with dropout 0 is a plain TimestepEmbedding and a label module is never handed the mask), and
                   where the mask acts (act_d1, diff_act) <m>_out_masked, for act_d1 also <m>_out_none (external_cond = None);
                   shared x, k (and xd, kd for the difference model), digests of the shared weights
  dit_cond_run.npz  one sampler trace (DFoTVideo._predict_videos: action dim 3, dropout 0.1, mask_first, vanilla History Guidance 1.5,
                   3 DDIM steps, every normal draw recorded) and one training step (DFoTVideo.training_step's loss path with the dropout
                   draw of RandomEmbeddingDropout replaced by the stored mask): loss, gradient norms of every parameter, the gradients
                   of the condition embedding
The label-embedding class of the reference is third party (diffusers.LabelEmbedding) and not importable here: ref_loader's stand-in
(an nn.Embedding with the extra null-class row when dropout > 0) restates it, as for the existing fixtures.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ref_loader  # noqa: E402
from make_golden import RandnRecorder, save, weights_digest  # noqa: E402
from make_golden_dit import DIFF_TINY, video_cfg  # noqa: E402
from oracle import dit as odit  # noqa: E402

torch.set_num_threads(8)

SMALL = dict(hidden_size=128, depth=2, num_heads=4, patch_size=1, in_channels=4, resolution=(16, 8), max_tokens=5)
MODES = {  # name -> (external_cond_type, external_cond_dim, num_classes, external_cond_dropout, seed of the condition tensors)
    "act_d0": ("action", 3, None, 0.0, 11),
    "act_d1": ("action", 3, None, 0.1, 12),
    "label": ("label", 1, 101, 0.0, 13),
}


def cond_params(module, seed: int):
    """seeded tensors for the reference module's own external_cond_embedding keys (names and shapes are read from the module)"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, t in module.state_dict().items():
        if not name.startswith("external_cond_embedding"):
            continue
        if name.endswith(".bias"):
            out[name] = 0.05 * torch.randn(t.shape, generator=g)
        elif "embedding_table" in name:
            out[name] = 0.5 * torch.randn(t.shape, generator=g)
        else:
            out[name] = torch.randn(t.shape, generator=g) / math.sqrt(t.shape[1])
    return out


def backbone_cfg(A, ocfg, dropout):
    return A(dict(name="dit3d", variant="full", pos_emb_type="rope_3d", patch_size=ocfg.patch_size, hidden_size=ocfg.hidden_size,
                  depth=ocfg.depth, num_heads=ocfg.num_heads, mlp_ratio=4.0, use_gradient_checkpointing=False,
                  external_cond_dropout=dropout))


def diff_backbone_cfg(A, oc, dropout):
    return A(dict(name="difference_dit3d", variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", merge_type="interleaved",
                  patch_size=oc.patch_size, hidden_size=None, embed_col_dim=oc.embed_col_dim, embed_row_dim=oc.hidden_size,
                  num_heads=oc.num_heads, num_col_heads=oc.num_col_heads, num_row_heads=oc.num_row_heads, depth=oc.depth,
                  mlp_ratio=oc.mlp_ratio or None, spatial_mlp_ratio=oc.spatial_mlp_ratio, use_bias=oc.use_bias, matrix_block="matrix",
                  flatten_matrix_rope=False, matrix_multi_token=False, use_gradient_checkpointing=False, external_cond_dropout=dropout))


def load_all(module, base, cseed):
    cp = cond_params(module, cseed)
    names = list(module.state_dict().keys())
    assert set(names) == set(base) | set(cp), sorted(set(names) ^ (set(base) | set(cp)))
    module.load_state_dict({**base, **cp}, strict=True)
    return names, cp


@torch.no_grad()
def forward_fixture(R):
    A = R["AttrDict"]
    small = odit.DiTConfig(**SMALL)
    base = odit.seeded_params(small, 2)
    g = torch.Generator().manual_seed(31)
    x = torch.randn(2, 5, 4, 16, 8, generator=g)
    k = torch.randint(0, 1000, (2, 5), generator=g)
    mask = torch.tensor([True, False])
    out = dict(x=x, k=k, mask=mask, digest=np.array(weights_digest(base)))
    for m, (ctype, cdim, ncls, drop, cseed) in MODES.items():
        print("dit cond", m)
        model = R["DiT3D"](backbone_cfg(A, small, drop), x_shape=[4, 16, 8], max_tokens=5, external_cond_type=ctype,
                           external_cond_num_classes=ncls, external_cond_dim=cdim, use_causal_mask=False).eval()
        names, cp = load_all(model, base, cseed)
        cond = torch.randint(0, ncls, (2, 1), generator=g) if ctype == "label" else torch.randn(2, 5, cdim, generator=g)
        out[f"{m}_names"] = np.array(names)
        out.update({f"{m}_cond/{n}": t for n, t in cp.items()})
        o, om = model(x, k, cond), model(x, k, cond, mask)
        out.update({f"{m}_cond": cond, f"{m}_out": o, f"{m}_mask_ignored": np.array(bool(torch.equal(o, om)))})
        if m == "act_d1":  # the only mode whose module looks at the mask (see the docstring)
            out.update({f"{m}_out_masked": om, f"{m}_out_none": model(x, k)})
    print("difference dit cond")
    oc = odit.DiffDiTConfig(**DIFF_TINY)
    dbase = odit.diff_seeded_params(oc, 3)
    import importlib
    dd = importlib.import_module("algorithms.dfot.backbones.dit.difference_dit3d")
    model = dd.DifferenceDiT3D(diff_backbone_cfg(A, oc, 0.1), x_shape=[oc.in_channels, *oc.resolution], max_tokens=oc.max_tokens,
                               external_cond_type="action", external_cond_num_classes=None, external_cond_dim=3, use_causal_mask=False).eval()
    names, cp = load_all(model, dbase, 14)
    xd = torch.randn(2, 10, 4, 16, 8, generator=g)
    kd = torch.randint(0, 1000, (2, 10), generator=g)
    cond = torch.randn(2, 10, 3, generator=g)
    out.update(xd=xd, kd=kd, digest_diff=np.array(weights_digest(dbase)), diff_act_names=np.array(names), diff_act_cond=cond,
               diff_act_out=model(xd, kd, cond), diff_act_out_masked=model(xd, kd, cond, mask))
    out.update({f"diff_act_cond/{n}": t for n, t in cp.items()})
    save("dit_cond.npz", **out)


def run_fixture(R):
    A = R["AttrDict"]
    small = odit.DiTConfig(**SMALL)
    base = odit.seeded_params(small, 2)

    def algo_for(steps, hg):
        cfg = video_cfg(A, small, sampling_steps=steps, hg=hg)
        cfg["external_cond_type"], cfg["external_cond_dim"], cfg["external_cond_processing"] = "action", 3, "mask_first"
        cfg["backbone"]["external_cond_dropout"] = 0.1
        return R["DFoTVideo"](cfg)

    print("conditioned sampler trace")
    algo = algo_for(3, dict(name="vanilla", guidance_scale=1.5)).eval()
    names, cp = load_all(algo.diffusion_model.model, base, 12)
    g = torch.Generator().manual_seed(41)
    vid = torch.randn(2, 5, 4, 16, 8, generator=g)
    actions = torch.randn(2, 5, 3, generator=g)
    algo.generator = torch.Generator().manual_seed(0)
    with torch.no_grad(), RandnRecorder() as rec:
        pred = algo._predict_videos(vid.clone(), n_context_tokens=2, conditions=actions.clone())
    out = dict(vid=vid, actions=actions, pred=pred, n_noise=np.array(len(rec.draws)), digest=np.array(weights_digest(base)),
               names=np.array(names), processed=algo._process_conditions(actions.clone()))
    out.update({f"noise{i}": d for i, d in enumerate(rec.draws)})
    out.update({f"cond/{n}": t for n, t in cp.items()})

    print("conditioned training step")
    algo = algo_for(4, dict(name="conditional")).train()
    load_all(algo.diffusion_model.model, base, 12)
    xs = torch.randn(2, 5, 4, 16, 8, generator=g)
    k = torch.randint(0, 1000, (2, 5), generator=g)
    masks = torch.ones(2, 5)
    masks[1, 3] = 0
    for tag, drop in (("keep", torch.tensor([False, False])), ("drop", torch.tensor([False, True]))):
        model = algo.diffusion_model.model
        for p_ in model.parameters():
            p_.grad = None
        real_rand = torch.rand

        def fixed_rand(*a, **kw):  # RandomEmbeddingDropout: torch.rand(emb.shape[:1]) < p  -> the stored per-video mask
            shape = a[0] if len(a) == 1 and not isinstance(a[0], int) else a
            if tuple(shape) == (2,):
                return torch.where(drop, torch.zeros(2), torch.ones(2))
            return real_rand(*a, **kw)
        torch.rand = fixed_rand
        try:
            with RandnRecorder() as rec:
                _, loss = algo.diffusion_model(xs, algo._process_conditions(actions.clone()), k=k)
        finally:
            torch.rand = real_rand
        loss = algo._reweight_loss(loss, masks)
        loss.backward()
        grads = {n: p_.grad.detach().clone() for n, p_ in model.named_parameters()}
        out.update({f"train_{tag}_loss": loss.detach(), f"train_{tag}_noise": rec.draws[0], f"train_{tag}_dropmask": drop,
                    f"train_{tag}_grad_names": np.array(list(grads)),
                    f"train_{tag}_norms": np.array([float(v.norm()) for v in grads.values()], np.float64)})
        out.update({f"train_{tag}_grad/{n}": v for n, v in grads.items() if n.startswith("external_cond_embedding")})
    out.update(train_xs=xs, train_k=k, train_masks=masks)
    save("dit_cond_run.npz", **out)


def main():
    R = ref_loader.install()
    forward_fixture(R)
    run_fixture(R)


if __name__ == "__main__":
    main()
