#!/usr/bin/env python3
"""Generate tests/golden/image_vae_1024.npz by executing the reference's own ImageVAE encoder / decoder on CPU (build container only:
needs the reference source, loaded through tools/ref_loader.install_image_vae()).

    python tools/make_golden_image_vae_1024.py

One configuration, laid out as the cases of tests/golden/image_vae.npz (tools/make_golden_image_vae.py), whose mid attention runs over
1024 positions per frame, the count of a 256 x 256 frame of the KL-f8 recipes:
  C   ch 128, ch_mult [1, 2], num_res_blocks 1, resolution 64, 2 frames   mid attention at 32 x 32 (N = 1024, C = 256)
Frames y in [0, 1] and `moments = quant_conv(encoder(2 y - 1))`; latents z and `frames = decoder(post_quant_conv(z))`.  Weights are the
seeded ones of oracle.vae.seeded_tensor (the tests re-create them; they are not stored).

The fixture must see the attention: with the softmax replaced by a uniform average over the keys (module `AttnBlock.forward` with
constant weights 1 / N), frames and moments have to move by at least 4e-2 rel-L2, twice the 2e-2 parity bar of the GPU tests.  Both
figures are asserted before the file is written and stored in it (`uniform_attention_frames`, `uniform_attention_moments`).
Data only -- no reference source.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_loader  # noqa: E402
from oracle import vae as ovae  # noqa: E402

SEED = 41
CASE = "c"
CFG = dict(ch_mult=(1, 2), resolution=64, frames=2)
SEES_ATTENTION = 4e-2


def ddconfig():
    return dict(double_z=True, z_channels=4, resolution=CFG["resolution"], in_channels=3, out_ch=3, ch=128, ch_mult=list(CFG["ch_mult"]),
                num_res_blocks=1, attn_resolutions=[], dropout=0.0)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@torch.no_grad()
def main():
    import image_vae_common as ivc
    Encoder, Decoder = ref_loader.install_image_vae()
    g = torch.Generator().manual_seed(SEED)
    dd, embed = ddconfig(), 4
    vae = nn.Module()
    vae.encoder, vae.decoder = Encoder(**dd), Decoder(**dd)
    vae.quant_conv = nn.Conv2d(2 * dd["z_channels"], 2 * embed, 1)       # ImageVAE.__init__, trainer.py:295-296
    vae.post_quant_conv = nn.Conv2d(embed, dd["z_channels"], 1)
    vae.eval()
    sd = {n: ovae.seeded_tensor(n, t.shape) for n, t in vae.state_dict().items()}
    vae.load_state_dict(sd, strict=True)
    r, f = CFG["resolution"], CFG["frames"]
    lr = r // 2 ** (len(CFG["ch_mult"]) - 1)
    y = torch.rand(f, 3, r, r, generator=g)
    z = torch.randn(f, embed, lr, lr, generator=g)
    moments = vae.quant_conv(vae.encoder(2.0 * y - 1.0))                  # ImageVAE.encode, trainer.py:334-338
    frames = vae.decoder(vae.post_quant_conv(z))                          # ImageVAE.decode, trainer.py:340-343
    assert moments.shape == (f, 2 * embed, lr, lr) and frames.shape == (f, 3, r, r)
    assert lr * lr == 1024

    # does the fixture see the attention?  the restatement with uniform attention weights against the reference's output
    cfg = dict(ch_mult=CFG["ch_mult"], num_res_blocks=1)
    real_softmax = torch.softmax
    try:
        torch.softmax = lambda s, dim: torch.full_like(s, 1.0 / s.shape[dim])
        uni_frames = rel(ivc.decode(sd, cfg, z), frames)
        uni_moments = rel(ivc.encode(sd, cfg, 2.0 * y - 1.0), moments)
    finally:
        torch.softmax = real_softmax
    print(f"restatement vs reference: frames {rel(ivc.decode(sd, cfg, z), frames):.3e}, moments "
          f"{rel(ivc.encode(sd, cfg, 2.0 * y - 1.0), moments):.3e}")
    print(f"uniform attention moves the frames by {uni_frames:.3e} and the moments by {uni_moments:.3e} rel-L2")
    assert uni_frames >= SEES_ATTENTION and uni_moments >= SEES_ATTENTION, (uni_frames, uni_moments)

    names = list(sd)
    out = {f"y_{CASE}": y, f"z_{CASE}": z, f"moments_{CASE}": moments, f"frames_{CASE}": frames}
    out[f"names_{CASE}"] = np.array(names)
    out[f"shapes_{CASE}"] = np.array([str(tuple(sd[n].shape)) for n in names])
    out[f"tag_{CASE}"] = np.array(f"ch 128 ch_mult {list(CFG['ch_mult'])} num_res_blocks 1 resolution {r} frames {f} z 4 embed 4")
    path = os.path.join(ROOT, "tests", "golden", "image_vae_1024.npz")
    np.savez(path, **{k: (v.numpy().astype(np.float32) if torch.is_tensor(v) else v) for k, v in out.items()}, seed=np.array(SEED),
             weight_seed=np.array(71), uniform_attention_frames=np.array(uni_frames), uniform_attention_moments=np.array(uni_moments))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
