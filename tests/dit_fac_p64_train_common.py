"""Shared helpers of tests/test_dit_fac_p64_train_host.py, tests/test_gpu_dit_fac_p64_train.py and tools/make_golden_dit_fac_p64_train.py
(not a test module): the training loss of the FacDiT backbone at 64 patches per frame (latents 4x16x16 at patch 2, the taichi res-128
recipes), restated on the host.  tests/dit_fac_train_common.py at the geometry of tests/dit_p64_common.py: hidden 128, depth 2, 4 heads,
X_SHAPE (4, 16, 16), patch 2, MAX_TOKENS 4.

  * LOSS_WEIGHTING        the loss weighting of the fixture (fused_min_snr, cum_snr_decay 0.96), as tests/golden/dit_fac_train.npz uses
  * TRAIN_CASES           the cases of tests/golden/dit_fac_p64_train.npz: tag -> spatial_mlp_ratio
  * case_params           the seeded weights of a case (dit_fac_common.seeded_params of dit_p64_common.fac_keys)
  * host_loss_and_grads   fp32 (or fp64) autograd through dit_p64_common.fac_host + oracle.sampler.discrete_training_loss with the loss
                          masks of DFoTVideo._reweight_loss: (loss, {name: gradient})
  * trainer               dfot_amd.FacDiTTrainer(..., allow_p64=True) at a fixture case with the seeded weights
  * skipped_temporal_backward / skipped_spatial_backward   contexts in which the host forward differentiates as an engine would that left
                          out the backward of the temporal / the spatial (64-token) attention (dq = dk = dv = 0 in those blocks): the
                          figures the GPU tests quote for such bugs
"""
import contextlib
import math

import torch
import torch.nn.functional as F

import dit_fac_common as fc
import dit_p64_common as pc
from dit_fac_train_common import LOSS_WEIGHTING  # noqa: F401
from dit_p64_common import MAX_TOKENS, X_SHAPE  # noqa: F401

TRAIN_CASES = dict(pc.FAC_CASES)  # mlp0: spatial_mlp_ratio 0.0, mlp4: 4.0
FIXTURE = "dit_fac_p64_train.npz"


def case_params(tag, cond=False):
    return fc.seeded_params(pc.fac_keys(TRAIN_CASES[tag], cond))


def host_loss_and_grads(tag, xs, k, noise, masks, dtype=torch.float32, weighting=LOSS_WEIGHTING):
    from oracle import sampler as osm, schedule as sch
    ps = {n: t.clone().to(dtype).requires_grad_() for n, t in case_params(tag).items()}
    model = lambda x, lv, c, m: pc.fac_host(ps, x, lv, dtype=dtype)
    _, per_el = osm.discrete_training_loss(model, sch.build_tables(beta_schedule="cosine"), xs.to(dtype), k, noise.to(dtype).clamp(-20, 20), **weighting)
    loss = (per_el * masks.to(dtype)[..., None, None, None]).mean()
    loss.backward()
    return loss.detach(), {n: t.grad.detach() for n, t in ps.items()}


def trainer(tag, cond=False, **kw):
    import dfot_amd
    if cond:
        kw.update(external_cond_type="action", external_cond_dim=pc.COND_DIM)
    params = case_params(tag, cond)
    tr = dfot_amd.FacDiTTrainer(pc.fac_cfg(TRAIN_CASES[tag], cond), x_shape=X_SHAPE, max_tokens=MAX_TOKENS, allow_p64=True, **kw)
    tr.load_state_dict(params, strict=True)
    return tr, params


@contextlib.contextmanager
def _skipped_backward(which):
    """dit_fac_common._dit_block with the attention output of the blocks whose name contains `which` detached: the forward is unchanged,
    and no gradient flows back through that attention to q, k, v (so none reaches attn.qkv through it)"""
    plain = fc._dit_block

    def block(p, pre, x, c, heads, has_mlp):
        if which not in pre:
            return plain(p, pre, x, c, heads, has_mlp)
        m, gate = fc._ada_ln(p, f"{pre}.norm1", x, c, 3)
        s, n, ch = m.shape
        d = ch // heads
        qkv = F.linear(m, p[f"{pre}.attn.qkv.weight"], p[f"{pre}.attn.qkv.bias"]).reshape(s, n, 3, heads, d).permute(2, 0, 3, 1, 4)
        w = torch.softmax(qkv[0] @ qkv[1].transpose(-2, -1) / math.sqrt(d), dim=-1)
        o = (w @ qkv[2]).transpose(1, 2).reshape(s, n, ch).detach() + 0.0 * qkv.sum()  # zero, not missing, gradients
        x = m + gate * F.linear(o, p[f"{pre}.attn.proj.weight"], p[f"{pre}.attn.proj.bias"])
        if has_mlp:
            m, gate = fc._ada_ln(p, f"{pre}.norm2", x, c, 3)
            hid = F.gelu(F.linear(m, p[f"{pre}.mlp.fc1.weight"], p[f"{pre}.mlp.fc1.bias"]), approximate="tanh")
            x = m + gate * F.linear(hid, p[f"{pre}.mlp.fc2.weight"], p[f"{pre}.mlp.fc2.bias"])
        return x
    fc._dit_block = block
    try:
        yield
    finally:
        fc._dit_block = plain


def skipped_temporal_backward():
    return _skipped_backward("dit_base.temporal_blocks.")


def skipped_spatial_backward():
    return _skipped_backward("dit_base.blocks.")
