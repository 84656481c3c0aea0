#!/usr/bin/env python3
"""Generate tests/golden/titok_enc.npz by executing the reference's own TiTok_KL encoder on CPU in fp32 (build container only: needs the
reference source, loaded through tools/ref_loader.install_titok()).

    python tools/make_golden_titok_enc.py

The reference's `TiTok_KL` (algorithms/vae/tiktok_kl/titok_kl.py) is built with its own constructor and run as `encode` runs it (:78-98):
`encoder(pixel_values=x, latent_tokens=self.latent_tokens)` gives the moments (F, 2 * token_size, 1, 32), `encode(x, sample=True)` their
first token_size channels (the mode; asserted bit-equal here).  Weights are the seeded ones of oracle.vae.seeded_tensor (the tests
re-create them bit-identically; they are not stored) with TWO changes, both recorded in the file:
  * the q and k rows (the first 2 C rows) of every `encoder.transformer.*.attn.in_proj_weight` are multiplied by QK_GAIN = 2,
  * `encoder.patch_embed.weight` is multiplied by PATCH_GAIN = 8.
With plain seeded weights the softmax is near uniform, a latent token receives the mean over all patches and the moments barely depend on
the image (rel-L2 between the moments of two independent inputs: 0.12 / 0.12 / 0.04 on a / b / c, against 8e-3 ... 1.1e-2 that the
reference's own bf16 autocast loses): at 256^2 a broken patch path could hide inside a bf16 tolerance.  With the gains that figure is
about 0.5 / 0.5 / 0.25 against autocast losses of 3e-2 / 4e-2 / 2e-2.  Sharper gains are of no use: at q/k x 2.5 the reference's own
autocast run already loses 0.09 - 0.17.
The tool REFUSES a seed or gain for which, on any case, sensitivity < 5 x bar with bar = 2 x rel_autocast_moments_<case> (the bar of
tests/test_gpu_titok_enc.py).
Three configurations (token_size 4, 32 latent tokens, patch 16), those of tools/make_golden_titok.py:
  a   small (512 / 8 layers / 8 heads),   64^2  frames (L = 1 + 16 + 32  = 49),  3 frames
  b   base  (768 / 12 / 12),              128^2 frames (L = 1 + 64 + 32  = 97),  2 frames
  c   small,                              256^2 frames (L = 1 + 256 + 32 = 289, the production sequence), 1 frame
Inputs are `torch.rand(F, 3, S, S, generator=torch.Generator().manual_seed(seed))` on the CPU; the file stores the seeds plus the sum and
eight sampled values of every input (the tests re-draw the inputs and check them against these: two 256^2 images would not fit a fixture
file).  Per case: the moments, the moments of a second independent input (the sensitivity guard, and for c the second frame of the
frame-independence test), the encoder keys' names and shapes, and rel_autocast_moments: the rel-L2 the reference itself loses under
torch.autocast("cpu", bfloat16) against its fp32 run.  Data only -- no reference source.
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

SEED = 57
QK_GAIN = 2.0
PATCH_GAIN = 8.0
CASES = {"a": dict(size="small", image_size=64, frames=3), "b": dict(size="base", image_size=128, frames=2),
         "c": dict(size="small", image_size=256, frames=1)}


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def draw(seed, frames, size):
    return torch.rand(frames, 3, size, size, generator=torch.Generator().manual_seed(seed))


def probe(x):
    """what the tests check a re-drawn input against: its sum (fp64) and eight values at evenly spaced flat positions"""
    flat = x.reshape(-1)
    idx = torch.linspace(0, flat.numel() - 1, 8).long()
    return np.array(float(flat.double().sum())), flat[idx].numpy().astype(np.float32)


def with_gains(name, t):
    if name.startswith("encoder.transformer.") and name.endswith(".attn.in_proj_weight"):
        t = t.clone()
        t[: 2 * t.shape[1]] *= QK_GAIN
    elif name == "encoder.patch_embed.weight":
        t = t * PATCH_GAIN
    return t


@torch.no_grad()
def main():
    TiTok_KL = ref_loader.install_titok()
    out = {}
    for i, (case, c) in enumerate(CASES.items()):
        vae = TiTok_KL(image_size=c["image_size"], token_size=4, use_l2_norm=True, vit_enc_model_size=c["size"], vit_dec_model_size="small",
                       vit_enc_patch_size=16, vit_dec_patch_size=16, num_latent_tokens=32, use_checkpoint=False).eval()
        sd = {n: with_gains(n, ovae.seeded_tensor(n, t.shape)) for n, t in vae.state_dict().items()}
        vae.load_state_dict(sd, strict=True)
        seeds = (SEED + 10 * i, SEED + 10 * i + 1)
        x, x2 = (draw(s, c["frames"], c["image_size"]) for s in seeds)
        moments = vae.encoder(pixel_values=x, latent_tokens=vae.latent_tokens)
        assert moments.shape == (c["frames"], 8, 1, 32)
        assert torch.equal(vae.encode(x, sample=True), moments[:, :4])
        with torch.autocast("cpu", dtype=torch.bfloat16):
            moments_bf = vae.encoder(pixel_values=x, latent_tokens=vae.latent_tokens)
        moments2 = vae.encoder(pixel_values=x2, latent_tokens=vae.latent_tokens)
        loss, sens = rel(moments_bf.float(), moments), rel(moments2, moments)
        names = [n for n in sd if n.startswith("encoder.") or n == "latent_tokens"]
        print(f"case {case}: {len(sd)} keys, {len(names)} the encoder's; moments std {moments.std():.3f}; moments of two independent inputs differ by "
              f"rel-L2 {sens:.3f}; bf16 autocast loses {loss:.2e}; sensitivity / bar = {sens / (2 * loss):.1f}")
        assert sens >= 5 * 2 * loss, "the fixture must depend on the image by 5 x the GPU test's bar: pick another SEED or gain"
        out.update({f"moments_{case}": moments, f"moments2_{case}": moments2})
        for tag, s, t in (("x", seeds[0], x), ("x2", seeds[1], x2)):
            out[f"{tag}_seed_{case}"] = np.array(s)
            out[f"{tag}_sum_{case}"], out[f"{tag}_probe_{case}"] = probe(t)
        out[f"rel_autocast_moments_{case}"] = np.array(loss)
        out[f"names_{case}"] = np.array(names)
        out[f"shapes_{case}"] = np.array([str(tuple(sd[n].shape)) for n in names])
        out[f"tag_{case}"] = np.array(f"vit_enc_model_size {c['size']} image_size {c['image_size']} frames {c['frames']} token_size 4 latent tokens 32")
    out.update(seed=np.array(SEED), weight_seed=np.array(71), qk_gain=np.array(QK_GAIN), patch_gain=np.array(PATCH_GAIN))
    path = os.path.join(ROOT, "tests", "golden", "titok_enc.npz")
    np.savez_compressed(path, **{k: (v.numpy().astype(np.float32) if torch.is_tensor(v) else v) for k, v in out.items()})
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 2 ** 20


if __name__ == "__main__":
    main()
