#!/usr/bin/env python3
"""Generate tests/golden/dit1d_train.npz by executing the reference's own DFoTVideo training loss around the reference's DIT1D
(algorithms/dfot/backbones/dit1d/dit_model.py, stock dit1d.yaml) on CPU in fp32, differentiated by the reference's autograd.

Run ONLY in the build container (needs the reference checkout):   python tools/make_golden_dit1d_train.py
Built on tools/ref_loader.py like tools/make_golden_dit_fac_train.py; the reference's DIT1D from ref_loader.install_dit1d() is assigned to
diffusion_model.model, as tools/make_golden_dit1d.py does for sampling.  Discrete diffusion, cosine schedule, pred_v, fused_min_snr with
cum_snr_decay 0.96, _reweight_loss with one masked token; backbone at tests/dit1d_common.TINY, inputs dit1d_common.inputs() (B 2, T 8,
[4, 1, 32]), the cases of dit1d_train_common.TRAIN_CASES (h4 and h2: both q/k/v row strides; h4_nomask: causal_attn_mode null), weights
from dit1d_common.seeded_params at the gain below.

The gain of the q and k rows of every qkv.weight is dit1d_train_common.TRAIN_GAIN = 2.75, not the 4.0 that tests/golden/dit1d.npz records
for sampling.  At 4.0 the engine's gradients miss the 5e-2 bar against fp32 autograd (x_embedder.weight 7.0e-2, the input gradient 6.9e-2,
case h4, one MI355X) -- and so does dit1d_train_common.forward_emulated, plain fp32 autograd with the GEMM operands rounded to bf16 where
the engine rounds them (7.1e-2 / 7.2e-2 at the same two places; 9.3e-2 in case h2): the deviation is the operands' precision under so
sharp a softmax, not the backward.  That emulation cannot hold half the bar (2.5e-2) at 4.0, nor at 3.0 (3.0e-2); 2.75 is the largest
multiple of 0.25 at which it does in all three cases for the random upstream gradient of test_backward_matches_autograd (2.2e-2; the
engine measures 2.2e-2 too; under this fixture's loss the emulation is at 1.3e-2), and there an attention backward without the frame mask
still misses every attn.qkv.weight gradient of the reference by 0.27 .. 0.43, more than 5 x the bar.  The attn.qkv.bias gradients miss by
0.23 .. 0.41; their smallest figure (block 1) does not move with the gain (0.23 in case h2 at 4.0 as well), so it is recorded and not part
of the condition.  tests/test_dit1d_train_host.py asserts each of these statements; this tool asserts the weight condition on the
reference's own gradients before it writes the file.

  inputs_digest, masks, qk_gain     digest of (x, k) of dit1d_common.inputs(), the loss masks [2, 8] (one zero), the gain
  <m>_noise, <m>_loss               m in {h4, h2, h4_nomask}: the recorded normal draw of DiscreteDiffusion.forward and the reweighted loss
  <m>_names, <m>_norms              ordered names of the trainable parameters (pos_embed is frozen: no gradient) and the norm of every
                                    gradient (float64)
  <m>_digest                        digest of the weights (pos_embed included)
  <m>_grad/<name>                   gradient tensors with <= 4096 elements
  host_rel, host_loss_rel           the largest gradient rel-L2 / loss deviation of the host restatement (fp32 autograd through
                                    dit1d_common.forward_host + oracle.sampler.discrete_training_loss,
                                    tests/dit1d_train_common.host_loss_and_grads) against the above, as measured here
  nomask_qkv_weight, nomask_qkv_bias  the smallest rel-L2 by which dit1d_train_common.wrong_backward("nomask") misses an attn.qkv.weight /
                                    attn.qkv.bias gradient of the reference (cases h4, h2)
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
import dit1d_common as dc  # noqa: E402
import dit1d_train_common as tc  # noqa: E402

torch.set_num_threads(8)
FIXTURE = "dit1d_train.npz"


@torch.enable_grad()
def main():
    R = ref_loader.install()
    DIT1D, _ = ref_loader.install_dit1d()
    torch.manual_seed(17)  # the reference draws the training noise from the default generator (the draw is recorded all the same)
    A = R["AttrDict"]
    xs, k = dc.inputs()
    masks = torch.ones(dc.BATCH, dc.MAX_TOKENS)
    masks[1, 3] = 0
    out = dict(inputs_digest=np.array(dc.tensor_digest(xs, k)), qk_gain=np.array(tc.TRAIN_GAIN))
    host, host_loss, nomask, nomask_b = [], [], [], []
    # the algorithm is built around a stand-in backbone of the same x_shape / max_tokens; the reference's own DIT1D takes its place
    small = odit.DiTConfig(hidden_size=128, depth=1, num_heads=2, patch_size=1, in_channels=dc.X_SHAPE[0], resolution=dc.X_SHAPE[1:],
                           max_tokens=dc.MAX_TOKENS)
    for tag, (heads, mode) in tc.TRAIN_CASES.items():
        print("dit1d train", tag)
        algo = R["DFoTVideo"](video_cfg(A, small, sampling_steps=3, hg=dict(name="conditional"))).train()
        model = DIT1D(A(dc.backbone_cfg(heads, causal_attn_mode=mode)), x_shape=list(dc.X_SHAPE), max_tokens=dc.MAX_TOKENS, external_cond_type=None,
                      external_cond_num_classes=None, external_cond_dim=0, use_causal_mask=True).train()
        keys = [(n, tuple(t.shape)) for n, t in model.state_dict().items()]
        assert keys == dc.key_shapes(heads), "key_shapes disagrees with the reference"
        params = tc.case_params(tag)
        model.load_state_dict(params, strict=True)
        assert not model.pos_embed.requires_grad
        algo.diffusion_model.model = model
        for p_ in model.parameters():
            p_.grad = None
        with RandnRecorder() as rec:
            _, loss = algo.diffusion_model(xs, None, k=k)
        loss = algo._reweight_loss(loss, masks)
        loss.backward()
        assert model.pos_embed.grad is None
        grads = {n: p_.grad.detach().clone() for n, p_ in model.named_parameters() if p_.requires_grad}
        assert list(grads) == [n for n, _ in keys if n != "pos_embed"]
        out[f"{tag}_loss"] = loss.detach()
        out[f"{tag}_noise"] = rec.draws[0]
        out[f"{tag}_names"] = np.array(list(grads))
        out[f"{tag}_norms"] = np.array([float(v.norm()) for v in grads.values()], np.float64)
        assert min(out[f"{tag}_norms"]) > 0
        for n, v in grads.items():
            if v.numel() <= 4096:
                out[f"{tag}_grad/{n}"] = v
        out[f"{tag}_digest"] = np.array(dc.digest(params))
        noise = torch.as_tensor(rec.draws[0])
        hl, hg = tc.host_loss_and_grads(tag, xs, k, noise, masks)
        ref_loss = float(out[f"{tag}_loss"])
        host_loss.append(abs(float(hl) - ref_loss) / abs(ref_loss))
        host.append(max(dc.rel(hg[n], grads[n]) for n in grads))
        print(f"  loss {ref_loss:.6f}; restatement: loss deviation {host_loss[-1]:.2e}, worst gradient rel-L2 {host[-1]:.2e}")
        if mode is not None:
            with tc.wrong_backward("nomask"):
                _, wrong = tc.host_loss_and_grads(tag, xs, k, noise, masks, torch.float64)
            nomask += [dc.rel(wrong[n], grads[n]) for n in grads if n.endswith(".attn.qkv.weight")]
            nomask_b += [dc.rel(wrong[n], grads[n]) for n in grads if n.endswith(".attn.qkv.bias")]
            print(f"  a backward without the frame mask against the reference's attn.qkv gradients: weight {[round(v, 3) for v in nomask[-2:]]}, "
                  f"bias {[round(v, 3) for v in nomask_b[-2:]]}")
    assert min(nomask) >= 5 * 5e-2, "the no-mask backward no longer misses attn.qkv.weight by 5 x the bar: the gain is too low"
    out.update(host_rel=np.array(max(host)), host_loss_rel=np.array(max(host_loss)), nomask_qkv_weight=np.array(min(nomask)),
               nomask_qkv_bias=np.array(min(nomask_b)))
    save(FIXTURE, masks=masks, **out)


if __name__ == "__main__":
    main()
