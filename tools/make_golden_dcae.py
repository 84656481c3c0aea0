#!/usr/bin/env python3
"""Generate tests/golden/dcae.npz by executing the reference's own DC-AE (algorithms/vae/dc_ae/autoencoder_dc_model.py: Encoder, Decoder,
MyAutoencoderDC) on CPU (build container only: needs the reference source, loaded through tools/ref_loader.install_dcae()).

    python tools/make_golden_dcae.py

The reference file imports its layers from diffusers, which is not available here: ref_loader supplies stand-ins (RMSNorm, GLUMBConv, the
Sana attention processor, ...) written from knowledge of diffusers 0.32.2 and NOT checked against the library.  Everything this fixture
pins about those layers is therefore pinned to the stand-ins.

Two configurations with the block pattern of the stock ones (ResBlock stages, EfficientViT from stage 3 on; stage 0 empty) but narrow
(tests/dcae_common.CASES), 3 frames each (an odd count: the engine pads the rows to GEMM tiles inside):
  f8    channels [64, 64, 128, 128],       64^2 frames  -> 8 x 8 latents, attention over 64 positions (4 heads)
  f16   channels [64, 64, 128, 128, 256],  128^2 frames -> 8 x 8 latents, attention over 256 (4 heads) and 64 positions (8 heads)
Encoder ResBlocks are rms_norm + SiLU (hard-wired in the reference), decoder ResBlocks batch_norm + ReLU (f16: stage 2 rms_norm + SiLU);
the model is in eval mode as `_from_pretrained_custom` leaves it.  Weights: dcae_common.seeded_tensor, one generator per key, with
non-trivial BatchNorm running statistics and norm weights / biases (the tests re-create them; a digest is stored).

Per case: frames `y` (uint8; the model sees 2 y / 255 - 1), `latents = encode(.)`, `recon = decode(latents)`, the state-dict names and
shapes in the reference's order, `host_rel_*` = the deviation of the restatement tests/dcae_common.py from the reference as measured here,
and `sens_<mistake>_{lat,rec}` = the relative change under each deliberate mistake of dcae_common.MISTAKES (asserted here to be at least
twice the parity bar 2e-2).  Data only -- no reference source.
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
import dcae_common as dc  # noqa: E402

SEED = 41


@torch.no_grad()
def main():
    torch.set_num_threads(1)
    AutoencoderDC, _ = ref_loader.install_dcae()
    branches = ref_loader._SanaMultiscaleAttnProcessor2_0.branches
    g = torch.Generator().manual_seed(SEED)
    out = {}
    for case, c in dc.CASES.items():
        cfg = dc.config(c)
        model = AutoencoderDC(ref_loader.AttrDict(cfg))
        model.eval()
        sd = {n: dc.seeded_tensor(n, t.shape) for n, t in model.state_dict().items()}
        model.load_state_dict(sd, strict=True)
        y8 = torch.randint(0, 256, (dc.FRAMES, 3, c["size"], c["size"]), generator=g, dtype=torch.uint8)
        x = 2.0 * (y8.float() / 255.0) - 1.0
        lat = model.encode(x)
        rec = model.decode(lat)
        r = 2 ** (len(c["channels"]) - 1)
        assert lat.shape == (dc.FRAMES, 32, c["size"] // r, c["size"] // r) and rec.shape == x.shape
        assert torch.isfinite(lat).all() and torch.isfinite(rec).all()
        h_lat, h_rec = dc.encode(sd, cfg, x), dc.decode(sd, cfg, lat)
        host = max(dc.rel(h_lat, lat), dc.rel(h_rec, rec))
        print(f"{case}: latents rms {lat.pow(2).mean().sqrt():.3f}, recon rms {rec.pow(2).mean().sqrt():.3f}, restatement deviation {host:.2e}")
        assert host < 1e-5, host
        for m in dc.MISTAKES:
            s_lat, s_rec = dc.rel(dc.encode(sd, cfg, x, mistake=m), lat), dc.rel(dc.decode(sd, cfg, lat, mistake=m), rec)
            print(f"  mistake {m:12s}: latents move by {s_lat:.3f}, reconstruction by {s_rec:.3f}")
            # the encoder has no BatchNorm (its ResBlocks are rms_norm): that mistake can only show in the decoder
            assert s_rec >= 2 * dc.BAR and (m == "batch_stats" or s_lat >= 2 * dc.BAR), (case, m, s_lat, s_rec)
            out[f"sens_{m}_lat_{case}"], out[f"sens_{m}_rec_{case}"] = np.array(s_lat), np.array(s_rec)
        names = list(sd)
        out.update({f"y_{case}": y8.numpy(), f"latents_{case}": lat.numpy(), f"recon_{case}": rec.numpy(), f"host_rel_{case}": np.array(host),
                    f"names_{case}": np.array(names), f"shapes_{case}": np.array([str(tuple(sd[n].shape)) for n in names]),
                    f"digest_{case}": np.array(dc.digest(sd), dtype=np.int64)})
    assert branches and set(branches) == {"linear"}, set(branches)
    path = os.path.join(ROOT, "tests", "golden", "dcae.npz")
    np.savez_compressed(path, **out, seed=np.array(SEED), weight_seed=np.array(83))
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
