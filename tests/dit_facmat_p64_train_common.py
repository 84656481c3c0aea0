"""Shared helpers of tests/test_dit_facmat_p64_train_host.py, tests/test_gpu_dit_facmat_p64_train.py and
tools/make_golden_dit_facmat_p64_train.py (not a test module): the training loss of the FacMatDiT backbone at 64 patches per frame (latents
4x16x16 at patch 2, the taichi res-128 facmat-s-*-bias recipes), restated on the host.  tests/dit_facmat_train_common.py at the geometry of
tests/dit_p64_common.py: embed_row_dim 128, depth 2, 4 spatial heads, X_SHAPE (4, 16, 16), patch 2, MAX_TOKENS 4.

  * LOSS_WEIGHTING        the loss weighting of the fixture (fused_min_snr, cum_snr_decay 0.96), as tests/golden/dit_facmat_train.npz uses
  * MODELS                tag -> ((num_col_heads, num_row_heads, use_bias, spatial_mlp_ratio, use_temporal_rope), geometry overrides):
                          "a", "b", "d" are dit_facmat_common.CASES at embed_col_dim 64; "e128" is embed_col_dim 128 with one column head,
                          4 row heads, no bias, no spatial MLP and no RoPE
  * TRAIN_CASES           the cases of tests/golden/dit_facmat_p64_train.npz: "b" and "e128"
  * keys / cfg / case_params / host   key order, backbone configuration, seeded weights and the host forward of a model
                          (dit_p64_common.mat_keys / mat_host for the tags of dit_facmat_common.CASES; the same functions of
                          dit_facmat_common with the same geometry for "e128")
  * host_loss_and_grads   fp32 (or fp64) autograd through the host forward + oracle.sampler.discrete_training_loss with the loss masks of
                          DFoTVideo._reweight_loss: (loss, {name: gradient})
  * trainer               dfot_amd.FacMatDiTTrainer(..., allow_p64=True) at a model with the seeded weights
"""
import torch

import dit_facmat_common as fm
import dit_p64_common as pc
from dit_facmat_train_common import LOSS_WEIGHTING  # noqa: F401
from dit_p64_common import MAX_TOKENS, X_SHAPE  # noqa: F401

E128 = dict(embed_col_dim=128)
MODELS = {
    "a": (fm.CASES["a"], {}),
    "b": (fm.CASES["b"], {}),
    "d": (fm.CASES["d"], {}),
    "e128": ((1, 4, False, 0.0, False), E128),
}
TRAIN_CASES = ("b", "e128")
FIXTURE = "dit_facmat_p64_train.npz"


def keys(tag, cond=False):
    (cc, rr, bias, ratio, rope), over = MODELS[tag]
    if tag in fm.CASES and not cond:
        return pc.mat_keys(tag)
    return fm.key_shapes(bias, ratio, pc.COND_DIM if cond else 0, pc.COND_DROPOUT if cond else 0.0, **{**pc.OVER, **over})


def cfg(tag, cond=False):
    (cc, rr, bias, ratio, rope), over = MODELS[tag]
    return fm.backbone_cfg(cc, rr, bias, ratio, rope, pc.COND_DROPOUT if cond else 0.0, **{**pc.OVER, **over})


def case_params(tag, cond=False):
    return fm.seeded_params(keys(tag, cond))


def host(tag, params, x, k, cond=None, mask=None, dtype=torch.float64):
    (cc, rr, bias, ratio, rope), over = MODELS[tag]
    if tag in fm.CASES and cond is None:
        return pc.mat_host(tag, params, x, k, dtype=dtype)
    return fm.forward_host(params, x, k, cc, rr, rope, cond, mask, dtype=dtype, **{**pc.OVER, **over})


def host_loss_and_grads(tag, xs, k, noise, masks, dtype=torch.float32, weighting=LOSS_WEIGHTING):
    from oracle import sampler as osm, schedule as sch
    ps = {n: t.clone().to(dtype).requires_grad_() for n, t in case_params(tag).items()}
    model = lambda x, lv, c, m: host(tag, ps, x, lv, dtype=dtype)
    _, per_el = osm.discrete_training_loss(model, sch.build_tables(beta_schedule="cosine"), xs.to(dtype), k, noise.to(dtype).clamp(-20, 20), **weighting)
    loss = (per_el * masks.to(dtype)[..., None, None, None]).mean()
    loss.backward()
    return loss.detach(), {n: t.grad.detach() for n, t in ps.items()}


def trainer(tag, cond=False, **kw):
    import dfot_amd
    if cond:
        kw.update(external_cond_type="action", external_cond_dim=pc.COND_DIM)
    params = case_params(tag, cond)
    tr = dfot_amd.FacMatDiTTrainer(cfg(tag, cond), x_shape=X_SHAPE, max_tokens=MAX_TOKENS, allow_p64=True, **kw)
    tr.load_state_dict(params, strict=True)
    return tr, params
