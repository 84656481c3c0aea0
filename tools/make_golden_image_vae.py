#!/usr/bin/env python3
"""Generate tests/golden/image_vae.npz by executing the reference's own ImageVAE encoder / decoder on CPU (build container only: needs
the reference source, loaded through tools/ref_loader.install_image_vae()).

    python tools/make_golden_image_vae.py

The reference's `Encoder` / `Decoder` (algorithms/vae/image_vae/model.py:18-245) are run as the `ImageVAE` wrapper runs them
(image_vae/trainer.py:281-345): `quant_conv(encoder(x))` are the posterior's moments, `decoder(post_quant_conv(z))` the frames.  The
wrapper itself imports Lightning, so its two `nn.Conv2d(.., 1)` are stated here.  Weights are the seeded ones of oracle.vae.seeded_tensor
(the tests re-create them bit-identically; they are not stored).  Two configurations (z_channels = embed_dim = 4, in_channels = out_ch = 3):
  A   ch 128, ch_mult [1, 2],    num_res_blocks 1, resolution 16, 4 frames   mid attention at 8 x 8   (N = 64,  C = 256)
  B   ch 128, ch_mult [1, 2, 2], num_res_blocks 1, resolution 64, 2 frames   mid attention at 16 x 16 (N = 256, C = 256); a level without
                                                                             a channel change (no nin_shortcut), two up and two down stages
Per case: frames y in [0, 1] and `moments = quant_conv(encoder(2 y - 1))`; latents z and `frames = decoder(post_quant_conv(z))`.
Stored with the state-dict names and shapes.  Data only -- no reference source.
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

import ref_loader  # noqa: E402
from oracle import vae as ovae  # noqa: E402

SEED = 37
CASES = {"a": dict(ch_mult=(1, 2), resolution=16, frames=4), "b": dict(ch_mult=(1, 2, 2), resolution=64, frames=2)}


def ddconfig(case):
    c = CASES[case]
    return dict(double_z=True, z_channels=4, resolution=c["resolution"], in_channels=3, out_ch=3, ch=128, ch_mult=list(c["ch_mult"]),
                num_res_blocks=1, attn_resolutions=[], dropout=0.0)


@torch.no_grad()
def main():
    Encoder, Decoder = ref_loader.install_image_vae()
    g = torch.Generator().manual_seed(SEED)
    out = {}
    for case, c in CASES.items():
        dd, embed = ddconfig(case), 4
        vae = nn.Module()
        vae.encoder, vae.decoder = Encoder(**dd), Decoder(**dd)
        vae.quant_conv = nn.Conv2d(2 * dd["z_channels"], 2 * embed, 1)       # ImageVAE.__init__, trainer.py:295-296
        vae.post_quant_conv = nn.Conv2d(embed, dd["z_channels"], 1)
        vae.eval()
        sd = {n: ovae.seeded_tensor(n, t.shape) for n, t in vae.state_dict().items()}
        vae.load_state_dict(sd, strict=True)
        r, f = c["resolution"], c["frames"]
        lr = r // 2 ** (len(c["ch_mult"]) - 1)
        y = torch.rand(f, 3, r, r, generator=g)
        z = torch.randn(f, embed, lr, lr, generator=g)
        moments = vae.quant_conv(vae.encoder(2.0 * y - 1.0))                  # ImageVAE.encode, trainer.py:334-338
        frames = vae.decoder(vae.post_quant_conv(z))                          # ImageVAE.decode, trainer.py:340-343
        assert moments.shape == (f, 2 * embed, lr, lr) and frames.shape == (f, 3, r, r)
        names = list(sd)
        out.update({f"y_{case}": y, f"z_{case}": z, f"moments_{case}": moments, f"frames_{case}": frames})
        out[f"names_{case}"] = np.array(names)
        out[f"shapes_{case}"] = np.array([str(tuple(sd[n].shape)) for n in names])
        out[f"tag_{case}"] = np.array(f"ch 128 ch_mult {list(c['ch_mult'])} num_res_blocks 1 resolution {r} frames {f} z 4 embed 4")
    path = os.path.join(ROOT, "tests", "golden", "image_vae.npz")
    np.savez(path, **{k: (v.numpy().astype(np.float32) if torch.is_tensor(v) else v) for k, v in out.items()}, seed=np.array(SEED),
             weight_seed=np.array(71))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
