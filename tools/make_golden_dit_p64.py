#!/usr/bin/env python3
"""Generate tests/golden/dit_p64.npz by executing the reference's own DiT3D on CPU in fp32, eval(), at 64 patches per frame: variants
"factorized_attention" (FacDiT) and "factorized_matrix_attention" (FacMatDiT) on latents 4x16x16 with patch_size 2, the shape of the
taichi res-128 recipes (bash/taichikl/resolution_128).

Run ONLY in the build container (needs the reference checkout):   python tools/make_golden_dit_p64.py
Built on tools/ref_loader.py like tools/make_golden_dit_fac.py / make_golden_dit_facmat.py.  Geometry: tests/dit_p64_common (hidden 128,
depth 2, 4 heads = head dim 32, max_tokens 4, batch 2).  Weights: the seeded_params of dit_fac_common / dit_facmat_common, one generator
per key seeded from the key's name and shape; the file stores the reference module's ordered key list, the shapes and a digest of the
tensors, not the tensors.

  names_<m>, shapes_<m>, digest_<m>   m in {fac_mlp0, fac_mlp4 (spatial_mlp_ratio 0 / 4), mat_b, mat_d (dit_facmat_common.CASES b: use_bias
                                       + temporal RoPE, d: neither), fac_act (fac_mlp0 + action dim 3, dropout 0.1)}
  x, k                                 input [2,4,4,16,16] and integer levels [2,4]
  out_<m>_t4, out_<m>_t2               m in {fac_mlp0, fac_mlp4, mat_b, mat_d}: forward at T = 4 and on the first 2 tokens
  x_frame3                             x with frame 3 alone replaced by a louder one
  out_fac_mlp0_frame3, sens_frame3     its FacDiT output and the relative change of the OTHER frames' (0-2) output: the temporal attention
  out_mat_b_frame3, sens_frame3_mat    the same of FacMatDiT b: the matrix attention
  act_cond, act_mask, out_act, out_act_masked
  host_rel                             the largest fp32 rel-L2 between the host restatements (dit_p64_common.fac_host / mat_host) and the
                                       outputs above, as measured here (the host test asserts a small margin over it)
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
from make_golden import save  # noqa: E402
import dit_fac_common as fc  # noqa: E402
import dit_facmat_common as fm  # noqa: E402
import dit_p64_common as pc  # noqa: E402

torch.set_num_threads(8)
LIVE_BAR = 2 * pc.FIXTURE_BAR  # the liveness tests need the reference's own movement above twice the parity bar


def make(R, cfg, keys_want, seeded, cond=False):
    kw = dict(external_cond_type="action", external_cond_num_classes=None, external_cond_dim=pc.COND_DIM if cond else 0)
    model = R["DiT3D"](R["AttrDict"](cfg), x_shape=list(pc.X_SHAPE), max_tokens=pc.MAX_TOKENS, use_causal_mask=False, **kw).eval()
    keys = [(n, tuple(t.shape)) for n, t in model.state_dict().items()]
    assert keys == keys_want, "key_shapes disagrees with the reference"
    params = seeded(keys)
    model.load_state_dict(params, strict=True)
    return model, params, keys


def meta(out, tag, params, keys):
    out[f"names_{tag}"] = np.array([n for n, _ in keys])
    out[f"shapes_{tag}"] = np.array([" ".join(map(str, s)) for _, s in keys])
    out[f"digest_{tag}"] = np.array(pc.digest(params))


@torch.no_grad()
def main():
    R = ref_loader.install()
    g = torch.Generator().manual_seed(79)
    x = torch.randn(pc.BATCH, pc.MAX_TOKENS, *pc.X_SHAPE, generator=g)
    k = torch.randint(0, 1000, (pc.BATCH, pc.MAX_TOKENS), generator=g)
    x3 = x.clone()
    x3[:, 3] = 4.0 * torch.randn(pc.BATCH, *pc.X_SHAPE, generator=g)  # a different, louder frame
    x2, k2 = x[:, :2].contiguous(), k[:, :2].contiguous()
    out = dict(x=x, k=k, x_frame3=x3)
    host = []

    def frame3(model, o4, tag, sens_key, host_fn):
        o3 = model(x3, k)
        sens = pc.rel(o3[:, :3], o4[:, :3])
        print(f"  frames 0-2 move by {sens} when frame 3 alone is perturbed")
        assert sens > LIVE_BAR, f"{tag}: the perturbation moves frames 0-2 by {sens}, not above {LIVE_BAR}: choose a louder one"
        out[f"out_{tag}_frame3"], out[sens_key] = o3, np.array(sens)
        host.append(pc.rel(host_fn(x3, k), o3))

    for tag, ratio in pc.FAC_CASES.items():
        print("dit p64 fac", tag)
        model, params, keys = make(R, pc.fac_cfg(ratio), pc.fac_keys(ratio), fc.seeded_params)
        meta(out, f"fac_{tag}", params, keys)
        o4, o2 = model(x, k), model(x2, k2)
        out[f"out_fac_{tag}_t4"], out[f"out_fac_{tag}_t2"] = o4, o2
        host_fn = lambda xx, kk, params=params: pc.fac_host(params, xx, kk, dtype=torch.float32)  # noqa: E731
        host += [pc.rel(host_fn(x, k), o4), pc.rel(host_fn(x2, k2), o2)]
        if tag == "mlp0":
            frame3(model, o4, "fac_mlp0", "sens_frame3", host_fn)
    for tag in pc.MAT_CASES:
        print("dit p64 facmat", tag)
        model, params, keys = make(R, pc.mat_cfg(tag), pc.mat_keys(tag), fm.seeded_params)
        assert (model.dit_base.temporal_rope is not None) == bool(fm.CASES[tag][4])
        meta(out, f"mat_{tag}", params, keys)
        o4, o2 = model(x, k), model(x2, k2)
        out[f"out_mat_{tag}_t4"], out[f"out_mat_{tag}_t2"] = o4, o2
        host_fn = lambda xx, kk, params=params, tag=tag: pc.mat_host(tag, params, xx, kk, dtype=torch.float32)  # noqa: E731
        host += [pc.rel(host_fn(x, k), o4), pc.rel(host_fn(x2, k2), o2)]
        if tag == "b":
            frame3(model, o4, "mat_b", "sens_frame3_mat", host_fn)

    print("dit p64 fac act")
    model, params, keys = make(R, pc.fac_cfg(0.0, cond=True), pc.fac_keys(0.0, cond=True), fc.seeded_params, cond=True)
    meta(out, "fac_act", params, keys)
    cond = torch.randn(pc.BATCH, pc.MAX_TOKENS, pc.COND_DIM, generator=g)
    mask = torch.tensor([True, False])
    oa, om = model(x, k, cond), model(x, k, cond, mask)
    out.update(act_cond=cond, act_mask=mask, out_act=oa, out_act_masked=om)
    host += [pc.rel(pc.fac_host(params, x, k, cond, dtype=torch.float32), oa),
             pc.rel(pc.fac_host(params, x, k, cond, mask, dtype=torch.float32), om)]
    out["host_rel"] = np.array(max(host))
    print("host restatements (fp32) vs the reference (fp32): rel-L2", host)
    save(pc.FIXTURE, **out)


if __name__ == "__main__":
    main()
