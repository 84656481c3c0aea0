#!/usr/bin/env python3
"""Generate tests/golden/dit_attnmap.npz: the frame-to-frame attention maps of the three tiny DiT3D models of tests/dit_attnmap_common.py,
from the reference's own modules on CPU in fp32, eval().

Run ONLY in the build container (needs the reference checkout):   python tools/make_golden_dit_attnmap.py
Built on tools/ref_loader.py like tools/make_golden_dit_fac.py.

Where the maps come from
  full    the reference's own ``store_attn_map`` path (Attention.forward keeps the softmax matrix, dit_blocks.py:100-118): the frame maps
          are reduced from it, and one head of one video of a T = 2 forward is stored whole, in the layout the reference stored.
  fac     the hook cannot reshape a temporal block's T-token sequence and
  facmat  MatrixAttention.forward raises with ``store_attn_map`` set, so for the temporal and matrix blocks the softmax is recomputed
          here from the module's own layers (qkv / qkv_u, qkv_v, q_norm, k_norm, rope, scale, proj) on the input a forward pre-hook
          captured; the attention output rebuilt from the recomputed map is asserted equal to the module's own output, so the
          restatement is checked against the reference, not trusted.  (The same check runs on the full variant, against attn_map too.)

Asserted here, on the CPU, for every stored frame map F: rel-L2(F, uniform 1/T) >= 4e-2 and rel-L2(F, F^T) >= 4e-2 (twice the parity bar
of the GPU test); the gain on the seeded q / k weights is raised until both hold.  A second pass restates the forward with the engine's
bf16 roundings (bf16 Linear weights and inputs, bf16 matrix factors, q and k rounded where the kernels read them); its rel-L2 against the fp32
maps is printed, stored (restate_<variant>) and asserted <= 1e-2 (half the bar).

  x, k                         input [2,5,4,16,8], integer levels [2,5]
  gain_<v>, digest_<v>         v in {full, fac, facmat}: the q / k gain and the digest of the weights
  frame_<v>_<i>                frame map of frame-mixing block i at T = 5: [2,4,5,5] (full, fac), [2,1,4,5,5] (facmat)
  full_hook                    block 1, video 1, head 2 of the full variant at T = 2 as the reference stored it: (t, h, w, N) = (2,16,8,256)
  full_hook_frame              its frame map [2,2], reduced here along the hook's axes
  restate_<v>                  rel-L2 of the bf16 restatement's frame maps against the fp32 ones (the largest over the blocks)
  restate_full_map             the same figure for the stored full map
"""
from __future__ import annotations

import math
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
import dit_attnmap_common as am  # noqa: E402
import dit_facmat_common as fm  # noqa: E402

torch.set_num_threads(8)
GAINS = (1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0)


def bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def reference_model(R, variant, params):
    cfg = dict(am.engine_cfg(variant))
    if variant == "full":
        cfg.update(name="dit3d", mlp_ratio=4.0, use_gradient_checkpointing=False)
    model = R["DiT3D"](R["AttrDict"](cfg), x_shape=[4, am.HEIGHT, am.WIDTH], max_tokens=am.TOKENS, external_cond_type="action",
                       external_cond_num_classes=None, external_cond_dim=0, use_causal_mask=False).eval()
    model.load_state_dict(params, strict=True)
    return model


def attention_probs(attn, x, rounded):
    """Attention.forward (dit_blocks.py:88-123) from the module's own layers; rounded: q (scaled into the exp2 domain) and k go to bf16
    where the engine's QKV epilogue stores them, the softmax is exact.  Returns (probabilities [B, heads, N, N] fp64, output)"""
    b, n, c = x.shape
    if rounded:
        x = bf(x)  # the AdaLN output is a bf16 GEMM operand
    qkv = attn.qkv(x).reshape(b, n, 3, attn.num_heads, attn.head_dim).permute(2, 0, 3, 1, 4)
    q, k, v = qkv.unbind(0)
    q, k = attn.q_norm(q), attn.k_norm(k)
    if attn.rope is not None:
        q, k = attn.rope(q), attn.rope(k)
    if rounded:
        s = bf(q * (attn.scale * math.log2(math.e))).double() @ bf(k).double().transpose(-2, -1) * math.log(2.0)
    else:
        s = (q * attn.scale).double() @ k.double().transpose(-2, -1)
    w = s.softmax(-1)
    o = attn.proj((w.to(v.dtype) @ v).transpose(1, 2).reshape(b, n, c))
    return w, o


def matrix_probs(attn, x, rounded):
    """MatrixAttention.forward (dit_blocks.py:303-346, multi_token False, flatten_rope False) from the module's own parameters; rounded:
    (q|k|v) go to bf16 as the engine's Z buffer holds them and q, k once more after the rotation, as the kernel's MFMA operands"""
    b, l, n, d = x.shape
    if rounded:
        x = bf(x)  # the AdaLN output is a bf16 GEMM operand
    qkv = torch.einsum("nm,blnd,dk->blmk", attn.qkv_u, x, attn.qkv_v)
    if attn.use_bias:
        qkv = qkv + attn.qkv_bias[None, None]
    if rounded:
        qkv = bf(qkv)
    cc, rr, hn, hd = attn.num_col_heads, attn.num_row_heads, attn.head_col_dim, attn.head_row_dim
    q, k, v = qkv.reshape(b, l, cc, hn, 3, rr, hd).permute(4, 0, 2, 5, 1, 3, 6).unbind(0)  # b c r l n d
    q, k = attn.q_norm(q), attn.k_norm(k)
    if attn.rope is not None:
        q = attn.rope(q.transpose(3, 4)).transpose(3, 4)
        k = attn.rope(k.transpose(3, 4)).transpose(3, 4)
    if rounded:
        q, k = bf(q), bf(k)
    w = (torch.einsum("bcrlnd,bcrknd->bcrlk", q.double(), k.double()) * attn.scale).softmax(-1)
    o = torch.einsum("bcrlk,bcrknd->bcrlnd", w.to(v.dtype), v).permute(0, 3, 1, 4, 2, 5).reshape(b, l, cc * hn, rr * hd)
    o = torch.einsum("nm,blnd,dk->blmk", attn.proj_u, o, attn.proj_v)
    if attn.use_bias:
        o = o + attn.proj_bias[None, None]
    return w, o


def frame_from_hook(hook):
    """(..., t, h, w, N) -> (..., t, t): mean over the query's h, w, sum over the patches of a key frame"""
    t = hook.shape[-4]
    return hook.mean(dim=(-3, -2)).reshape(*hook.shape[:-4], t, t, -1).sum(-1)


PROBS = {}


def maps_of(R, variant, params, x, k, rounded, store=False):
    """frame maps of every frame-mixing block of one forward: {block index: [B, heads.., T, T] fp64}.  rounded: the bf16 restatement (bf16
    Linear weights / matrix factors, every Linear input rounded to bf16, q and k rounded as the kernels read them).  store (full variant,
    fp32 pass): also return the reference's own attn_map of every block"""
    if rounded:
        params = {n: (bf(t) if t.ndim >= 2 and not n.startswith("patch_embedder") else t) for n, t in params.items()}
    model = reference_model(R, variant, params)
    handles = []
    if rounded:
        for mod in model.modules():
            if isinstance(mod, torch.nn.Linear):
                handles.append(mod.register_forward_pre_hook(lambda m, a: (bf(a[0]),) + tuple(a[1:])))
    blocks = model.dit_base.blocks if variant == "full" else model.dit_base.temporal_blocks
    seen = {}
    for i, blk in enumerate(blocks):
        handles.append(blk.attn.register_forward_hook(lambda m, a, o, i=i: seen.__setitem__(i, (a[0].detach().clone(), o.detach().clone()))))
        if store:
            blk.attn.store_attn_map = True
    b, t = x.shape[:2]
    stored = {}
    if store:  # the reference deletes nothing itself: the hook of attn_hook/hook.py reads module.attn_map after the forward
        for i, blk in enumerate(blocks):
            handles.append(blk.attn.register_forward_hook(lambda m, a, o, i=i: stored.__setitem__(i, m.attn_map.detach().clone())))
    model(x, k)
    for h in handles:
        h.remove()
    out = {}
    for i, blk in enumerate(blocks):
        xin, own = seen[i]
        w, o = (matrix_probs if variant == "facmat" else attention_probs)(blk.attn, xin, rounded)
        PROBS[i] = w  # of the last call (the restatement figure of the stored full map)
        if not rounded:
            err = fm.rel(o, own)
            assert err < 1e-5, f"{variant} block {i}: the output rebuilt from the recomputed map differs from the module's own by {err:.2e}"
        if variant == "full":
            if store:
                err = fm.rel(w.reshape(stored[i].shape), stored[i])
                assert err < 1e-5, f"full block {i}: recomputed map vs the reference's attn_map {err:.2e}"
                out[i] = frame_from_hook(stored[i].double())
            else:
                out[i] = frame_from_hook(w.reshape(b, -1, t, am.HEIGHT, am.WIDTH, w.shape[-1]))
        elif variant == "fac":  # sequences (b p): one T x T map per patch position; the frame map is their mean
            out[i] = w.reshape(b, -1, *w.shape[1:]).mean(1)
        else:
            out[i] = w
    return (out, stored) if store else out


@torch.no_grad()
def main():
    R = ref_loader.install()
    g = torch.Generator().manual_seed(91)
    x = torch.randn(2, am.TOKENS, 4, am.HEIGHT, am.WIDTH, generator=g)
    k = torch.randint(0, 1000, (2, am.TOKENS), generator=g)
    out = dict(x=x, k=k)
    for variant in am.VARIANTS:
        for gain in GAINS:
            params = am.seeded(variant, gain)
            maps = maps_of(R, variant, params, x, k, rounded=False, store=variant == "full")
            stored = None
            if variant == "full":
                maps, stored = maps
            checked = list(maps.values())
            if variant == "full":  # one head of one video, whole, at T = 2 (N = 256), in the layout the reference stored
                t2 = am.FULL_TOKENS
                _, stored2 = maps_of(R, variant, params, x[:, :t2].contiguous(), k[:, :t2].contiguous(), rounded=False, store=True)
                hook = stored2[am.FULL_BLOCK][am.FULL_BATCH_ROW, am.FULL_HEAD]
                assert tuple(hook.shape) == (t2, am.HEIGHT, am.WIDTH, t2 * am.PATCHES)
                checked.append(frame_from_hook(hook.double()))
            worst = [min(c) for c in zip(*(am.contrast(f) for f in checked))]
            print(f"{variant} gain {gain}: smallest rel-L2 against uniform {worst[0]:.3e}, against the transpose {worst[1]:.3e}")
            if min(worst) >= am.CONTRAST_BAR:
                break
        else:
            raise AssertionError(f"{variant}: no gain up to {GAINS[-1]} separates the maps from uniform / their transpose")
        for i, f in maps.items():
            assert tuple(f.shape) == am.map_shape(variant, 2), (variant, f.shape)
            assert float((f.sum(-1) - 1).abs().max()) < 1e-5
            out[f"frame_{variant}_{i}"] = f.float()
        out[f"gain_{variant}"] = np.array(gain)
        out[f"digest_{variant}"] = np.array(fm.digest(params))
        rmaps = maps_of(R, variant, params, x, k, rounded=True)
        restate = max(fm.rel(rmaps[i], maps[i]) for i in maps)
        print(f"{variant}: bf16 host restatement vs the fp32 maps rel-L2 {restate:.3e}")
        assert restate <= am.RESTATE_BAR, f"{variant}: the bf16 restatement is {restate:.3e} away from fp32 (> {am.RESTATE_BAR}): change the inputs"
        out[f"restate_{variant}"] = np.array(restate)
        if variant == "full":
            out["full_hook"] = hook
            out["full_hook_frame"] = checked[-1].float()
            maps_of(R, variant, params, x[:, :t2].contiguous(), k[:, :t2].contiguous(), rounded=True)
            rfull = fm.rel(PROBS[am.FULL_BLOCK][am.FULL_BATCH_ROW, am.FULL_HEAD].reshape(hook.shape), hook)
            print(f"full: bf16 host restatement of the stored full map rel-L2 {rfull:.3e}")
            assert rfull <= am.RESTATE_BAR
            out["restate_full_map"] = np.array(rfull)
    save("dit_attnmap.npz", **out)


if __name__ == "__main__":
    main()
