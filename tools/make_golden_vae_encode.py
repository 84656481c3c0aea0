#!/usr/bin/env python3
"""Generate tests/golden/vae_encode.npz by executing the reference's own VideoVAE encoder on CPU (build container only: needs the
reference source, loaded through tools/ref_loader.install_vae()).

    python tools/make_golden_vae_encode.py

The reference VideoVAE (default causal module choice, hidden 128, z 16, embed 16, temporal_length 17) gets the seeded weights of
oracle.vae.seeded_tensor (the tests re-create them bit-identically) and encodes frames y in [0, 1] drawn from a seeded torch.Generator
(the tests redraw them; they are not stored):
  case a   2 videos x 17 frames x 128 x 64 (non-square: catches H / W swaps)   `_encode(2 y - 1)` moments, one `encode(...).sample()` with
                                                                                the eps it drew
  case b   1 video  x  1 frame  x 128 x 128                                      `_encode(2 y - 1)` moments
Stored with the encoder's state-dict names and shapes.  Data only -- no reference source.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ref_loader  # noqa: E402
from oracle import vae as ovae  # noqa: E402

SEED = 29          # frames
SAMPLE_SEED = 31   # the global RNG state the reference's sample() draws from
SHAPES = {"a": (2, 3, 17, 128, 64), "b": (1, 3, 1, 128, 128)}


def frames():
    """the fixture's input frames in [0, 1], (B, 3, T, H, W) per case (tests/test_gpu_vae_encode.py draws them the same way)"""
    g = torch.Generator().manual_seed(SEED)
    return {k: torch.rand(s, generator=g) for k, s in SHAPES.items()}


@torch.no_grad()
def main():
    VideoVAE = ref_loader.install_vae()
    torch.manual_seed(0)
    vae = VideoVAE(hidden_size=128, z_channels=16, embed_dim=16, resolution=128, temporal_length=17).eval()
    sd = {n: ovae.seeded_tensor(n, t.shape) for n, t in vae.state_dict().items() if n.startswith(("encoder.", "quant_conv."))}
    missing, unexpected = vae.load_state_dict(sd, strict=False)
    assert not unexpected and all(m.startswith(("decoder.", "post_quant_conv.")) for m in missing)
    ys = frames()
    out = {}
    for k, y in ys.items():
        out[f"moments_{k}"] = vae._encode(2.0 * y - 1.0)
    post = vae.encode(2.0 * ys["a"] - 1.0)
    torch.manual_seed(SAMPLE_SEED)
    eps = torch.randn(post.mean.shape)
    torch.manual_seed(SAMPLE_SEED)
    sample = post.sample()
    torch.testing.assert_close(sample, post.mean + post.std * eps, rtol=0, atol=0)
    assert out["moments_a"].shape == (2, 32, 5, 16, 8) and out["moments_b"].shape == (1, 32, 1, 16, 16)
    names = list(sd)  # registration order of the reference
    path = os.path.join(ROOT, "tests", "golden", "vae_encode.npz")
    np.savez(path, **{k: v.numpy().astype(np.float32) for k, v in out.items()}, sample_a=sample.numpy(), eps_a=eps.numpy(),
             seed=np.array(SEED), weight_seed=np.array(71), names=np.array(names), shapes=np.array([str(tuple(sd[n].shape)) for n in names]))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
