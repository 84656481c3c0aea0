"""Shared helpers of tests/test_uvit3d_train_host.py, tests/test_gpu_uvit3d_train.py and tools/make_golden_uvit3d_train.py (not a test module):
the training step of the pose-free U-ViT (the reference's UViT3D under ContinuousDiffusion.forward and _reweight_loss) at
uvit3d_common.TINY.

  * TRAIN_CASES          fixture cases of uvit3d_common.CASES: a (no condition) and c (actions, dropout 0.1, the first video dropped)
  * train_inputs         batch, levels t in [0, 1] (both ends included), loss masks with one masked token, actions -- drawn from a seed
  * train_noise          the normal draw of ContinuousDiffusion.forward: the fixture stores its seed, shape and digest, not the 786 KB tensor
  * host_loss_and_grads  fp32 torch autograd through uvit3d_common.forward_host + oracle.sampler.training_loss, reweighted by the masks
"""
import torch

import uvit3d_common as uc
from oracle import sampler as osm

TRAIN_CASES = ("a", "c")
TRAIN_SEED, NOISE_SEED = 85, 86
DROP = torch.tensor([True, False])  # case c: RandomEmbeddingDropout drops the first video


def train_inputs():
    g = torch.Generator().manual_seed(TRAIN_SEED)
    xs = torch.randn(uc.BATCH, uc.MAX_TOKENS, *uc.X_SHAPE, generator=g)
    t = torch.rand(uc.BATCH, uc.MAX_TOKENS, generator=g)
    t[0, 0], t[1, 7] = 0.0, 1.0
    cond = torch.randn(uc.BATCH, uc.MAX_TOKENS, uc.COND_DIM, generator=g)
    masks = torch.ones(uc.BATCH, uc.MAX_TOKENS)
    masks[1, 3] = 0
    return xs, t, masks, cond


def train_noise():
    return torch.randn(uc.BATCH, uc.MAX_TOKENS, *uc.X_SHAPE, generator=torch.Generator().manual_seed(NOISE_SEED))


def case_cond(tag):
    """(actions or None, dropped videos or None) of a fixture case"""
    dim, drop = uc.CASES[tag]
    return (train_inputs()[3] if dim else None), (DROP if drop > 0 else None)


def trainable(params):
    return [n for n in params if n not in (uc.FREQS, uc.PHASES)]


def host_loss_and_grads(tag, dtype=torch.float32):
    xs, t, masks, _ = train_inputs()
    cond, drop = case_cond(tag)
    ps = {n: v.clone().requires_grad_(n not in (uc.FREQS, uc.PHASES)) for n, v in uc.case_params(tag).items()}
    _, per_el = osm.training_loss(lambda x, lv, c, m: uc.forward_host(ps, x, lv, c, drop, dtype=dtype), xs, cond, t, train_noise())
    loss = (per_el * masks[:, :, None, None, None]).mean()
    loss.backward()
    return loss.detach(), {n: ps[n].grad for n in trainable(ps)}
