"""Shared helpers of tests/test_dit_facmat_train_host.py, tests/test_gpu_dit_facmat_train.py and tools/make_golden_dit_facmat_train.py
(not a test module): the training loss of the FacMatDiT backbone restated on the host.

  * LOSS_WEIGHTING     the loss weighting of the fixture (fused_min_snr, cum_snr_decay 0.96), as tests/golden/training_grads.npz uses
  * host_loss_and_grads   fp32 (or fp64) autograd through dit_facmat_common.forward_host + oracle.sampler.discrete_training_loss with the
                          loss masks of DFoTVideo._reweight_loss: (loss, {name: gradient})
  * trainer            dfot_amd.FacMatDiTTrainer at a fixture case with the seeded weights
"""
import torch

import dit_facmat_common as fm

LOSS_WEIGHTING = dict(strategy="fused_min_snr", cum_snr_decay=0.96)
TRAIN_CASES = ("a", "b")  # the cases of tests/golden/dit_facmat_train.npz


def host_loss_and_grads(tag, xs, k, noise, masks, dtype=torch.float32, weighting=LOSS_WEIGHTING):
    from oracle import sampler as osm, schedule as sch
    cc, rr, bias, ratio, rope = fm.CASES[tag]
    ps = {n: t.clone().to(dtype).requires_grad_() for n, t in fm.case_params(tag).items()}
    model = lambda x, lv, c, m: fm.forward_host(ps, x, lv, cc, rr, rope, dtype=dtype)
    _, per_el = osm.discrete_training_loss(model, sch.build_tables(beta_schedule="cosine"), xs.to(dtype), k, noise.to(dtype).clamp(-20, 20), **weighting)
    loss = (per_el * masks.to(dtype)[..., None, None, None]).mean()
    loss.backward()
    return loss.detach(), {n: t.grad.detach() for n, t in ps.items()}


def trainer(tag, cond=False, **kw):
    import dfot_amd
    cc, rr, bias, ratio, rope = fm.CASES[tag]
    if cond:
        kw.update(external_cond_type="action", external_cond_dim=fm.COND_DIM)
    params = fm.case_params(tag, cond)
    tr = dfot_amd.FacMatDiTTrainer(fm.backbone_cfg(cc, rr, bias, ratio, rope, fm.COND_DROPOUT if cond else 0.0), x_shape=(4, 16, 8), max_tokens=5, **kw)
    tr.load_state_dict(params, strict=True)
    return tr, params
