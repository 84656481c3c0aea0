#!/usr/bin/env python3
"""Generate tests/golden/titok.npz by executing the reference's own TiTok_KL.decode on CPU in fp32 (build container only: needs the
reference source, loaded through tools/ref_loader.install_titok()).

    python tools/make_golden_titok.py

The reference's `TiTok_KL` (algorithms/vae/tiktok_kl/titok_kl.py) is built with its own constructor and run as `decode` runs it (:100-109):
`F.normalize(z, dim=1)`, `decoder(z)` (the logits), `pixel_quantize_conv(logits.softmax(1))` (the pixel decoder's input),
`pixel_decoder(..)` (the frames).  Weights are the seeded ones of oracle.vae.seeded_tensor (the tests re-create them bit-identically; they
are not stored) with ONE change: `decoder.ffn.2.weight` is multiplied by FFN2_GAIN = 8, recorded in the file.  With plain seeded weights
the 1024-way softmax is almost uniform (largest probability 0.01) and the decoded frames barely depend on the latent (rel-L2 between the
frames of two independent z: 1.6e-2 at 256^2), less than any bf16 tolerance, so a broken transformer would pass; with the gain the logits
have a standard deviation near 5 and that figure is 0.70 / 0.49 / 0.42 on the cases below.  Three configurations (token_size 4, 32 latent tokens, patch 16):
  a   small (512 / 8 layers / 8 heads),   64^2  frames (L = 1 + 16 + 32  = 49),  3 frames
  b   base  (768 / 12 / 12),              128^2 frames (L = 1 + 64 + 32  = 97),  2 frames
  c   small,                              256^2 frames (L = 1 + 256 + 32 = 289, the production sequence), 1 frame
(At 256^2 single draws of that figure spread from 0.26 to 0.49 with these weights; the tool refuses a SEED that gives less than 0.4
on any case.)  Per case: z, a second independent latent z2 (what the sensitivity guard of tests/test_titok_host.py decodes), the pixel
decoder's input, the frames, the decoder keys' names and shapes, the names of the ignored keys (encoder.*,
latent_tokens), and rel_autocast_logits / rel_autocast_frames: the rel-L2 the reference itself loses under
torch.autocast("cpu", bfloat16) against its fp32 run.  The logits are stored for a and b only (size).  Written as titok.npz plus
titok_b.npz, titok_b_logits.npz and titok_c.npz (the large arrays of b and c), each under 1 MiB.  Data only -- no reference source.
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
FFN2_GAIN = 8.0
CASES = {"a": dict(size="small", image_size=64, frames=3), "b": dict(size="base", image_size=128, frames=2),
         "c": dict(size="small", image_size=256, frames=1)}
LOGIT_CASES = ("a", "b")


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def stages(vae, z):
    """TiTok_KL.decode, titok_kl.py:100-109, with its intermediates"""
    zn = torch.nn.functional.normalize(z, dim=1) if vae.use_l2_norm else z
    logits = vae.decoder(zn)
    lat = vae.pixel_quantize_conv(logits.softmax(1))
    return logits, lat, vae.pixel_decoder(lat)


@torch.no_grad()
def main():
    TiTok_KL = ref_loader.install_titok()
    g = torch.Generator().manual_seed(SEED)
    out = {}
    for case, c in CASES.items():
        vae = TiTok_KL(image_size=c["image_size"], token_size=4, use_l2_norm=True, vit_enc_model_size="small", vit_dec_model_size=c["size"],
                       vit_enc_patch_size=16, vit_dec_patch_size=16, num_latent_tokens=32, use_checkpoint=False).eval()
        sd = {n: ovae.seeded_tensor(n, t.shape) for n, t in vae.state_dict().items()}
        sd["decoder.ffn.2.weight"] = sd["decoder.ffn.2.weight"] * FFN2_GAIN
        vae.load_state_dict(sd, strict=True)
        z = torch.randn(c["frames"], 4, 1, 32, generator=g)
        logits, lat, frames = stages(vae, z)
        assert torch.equal(frames, vae.decode(z))
        with torch.autocast("cpu", dtype=torch.bfloat16):
            logits_bf, _, frames_bf = stages(vae, z)
        z2 = torch.randn(c["frames"], 4, 1, 32, generator=g)
        _, _, other = stages(vae, z2)
        assert rel(other, frames) > 0.4, "the fixture must depend on the latent: pick another SEED"
        names = [n for n in sd if not (n.startswith("encoder.") or n == "latent_tokens")]
        print(f"case {case}: {len(sd)} keys, {len(names)} the decoder's; logits std {logits.std():.2f}, largest probability "
              f"{logits.softmax(1).max():.3f}; frames of two independent z differ by rel-L2 {rel(other, frames):.2f}; bf16 autocast loses "
              f"{rel(logits_bf.float(), logits):.2e} (logits) {rel(frames_bf.float(), frames):.2e} (frames)")
        out.update({f"z_{case}": z, f"z2_{case}": z2, f"pixel_input_{case}": lat, f"frames_{case}": frames})
        if case in LOGIT_CASES:
            out[f"logits_{case}"] = logits
        out[f"rel_autocast_logits_{case}"] = np.array(rel(logits_bf.float(), logits))
        out[f"rel_autocast_frames_{case}"] = np.array(rel(frames_bf.float(), frames))
        out[f"names_{case}"] = np.array(names)
        out[f"shapes_{case}"] = np.array([str(tuple(sd[n].shape)) for n in names])
        out[f"ignored_{case}"] = np.array([n for n in sd if n not in names])
        out[f"ignored_shapes_{case}"] = np.array([str(tuple(sd[n].shape)) for n in sd if n not in names])
        out[f"tag_{case}"] = np.array(f"vit_dec_model_size {c['size']} image_size {c['image_size']} frames {c['frames']} token_size 4 latent tokens 32")
    out.update(seed=np.array(SEED), weight_seed=np.array(71), ffn2_gain=np.array(FFN2_GAIN))
    # several files, each under 1 MiB: the large arrays of b and c on their own, everything else in titok.npz (tests/titok_common.load
    # reads them back as one mapping)
    parts = {"titok_b.npz": ("pixel_input_b", "frames_b"), "titok_b_logits.npz": ("logits_b",), "titok_c.npz": ("frames_c",)}
    parts["titok.npz"] = tuple(k for k in out if not any(k in v for v in parts.values()))
    for fn, keys in parts.items():
        path = os.path.join(ROOT, "tests", "golden", fn)
        np.savez_compressed(path, **{k: (out[k].numpy().astype(np.float32) if torch.is_tensor(out[k]) else out[k]) for k in keys})
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 2 ** 20


if __name__ == "__main__":
    main()
