#!/usr/bin/env python3
"""Micro-benchmarks of the C-ABI primitives at the RE10K model shapes (model batch 2), HIP-event timed.
Usage (GPU box): python tools/bench_ops.py [gemm] [conv] [attn] [tattn] [mattn] [tattn_bwd] [facdit_train] [mattn_bwd] [facmat_train] [vae_encode] [equal] [dit_front] [ivae] [uvit3d] [gnfilm_frame] [uvit3d_train] [attnmap] [titok] [titok_enc] [mcraft] [sattn64] [facmat_narrow] [dcae] [attn_fc] [attn_fc_bwd] [dit1d] [seq64_bwd] [seq64_bwd_packed] [facdit_s128_train] [facmat_factor_wgrad] [facmat_s128_train]"""
import ctypes as C
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dfot_amd  # noqa: E402
from dfot_amd import capi  # noqa: E402

S = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
P = lambda t: C.c_void_p(t.data_ptr())


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def gemm(m, n, k, variant):
    a = torch.randn(m, k, device="cuda").bfloat16()
    w = (torch.randn(n, k, device="cuda") / math.sqrt(k)).bfloat16()
    out = torch.empty(m, n, device="cuda")
    ms = timeit(lambda: capi.check(capi.lib.dfot_op_gemm(P(a), k, P(w), None, P(out), m, n, k, variant, S())))
    return ms, 2.0 * m * n * k / ms / 1e9


def conv(bt, h, w, cin, cout, variant):
    a = torch.randn(bt, h, w, cin, device="cuda").bfloat16()
    wt = (torch.randn(cout, 9 * cin, device="cuda") / math.sqrt(9 * cin)).bfloat16()
    out = torch.empty(bt, h, w, cout, device="cuda")
    ms = timeit(lambda: capi.check(capi.lib.dfot_op_conv3x3(P(a), P(wt), None, P(out), bt, h, w, cin, cout, variant, S())))
    return ms, 2.0 * bt * h * w * cout * 9 * cin / ms / 1e9


def attn(b, heads, n, d, variant):
    q = torch.randn(b, heads, n, d, device="cuda").bfloat16() * 0.2
    k = torch.randn(b, heads, n, d, device="cuda").bfloat16()
    v = torch.randn(b, heads, n, d, device="cuda").bfloat16()
    o = torch.empty(b, n, heads * d, device="cuda", dtype=torch.bfloat16)
    ms = timeit(lambda: capi.check(capi.lib.dfot_op_attention(P(q), P(k), P(v), P(o), heads * d, b, heads, n, d, variant, S())))
    return ms, 4.0 * b * heads * n * n * d / ms / 1e9


def dit_front(name, bb, cls, x_shape, max_tokens, batch, tokens):
    """front end (everything up to and including the modulation GEMM) and whole forward of one DiT shape on three paths: float levels
    (Fourier model), the conditioned int-level path (dfot_dit_forward_cond, the yardstick: the same downstream work) and the unconditioned
    per-level table.  HIP events, 5 warm-up + 50 timed launches each."""
    kw = dict(external_cond_type="action", external_cond_dim=4)
    models = {"float": cls(dict(bb, use_fourier_noise_embedding=True), x_shape=x_shape, max_tokens=max_tokens, **kw),
              "int cond": cls(bb, x_shape=x_shape, max_tokens=max_tokens, **kw)}
    x = torch.randn(batch, tokens, *x_shape, device="cuda")
    cond = torch.randn(batch, tokens, 4, device="cuda")
    levels = {"float": 2.5 * torch.randn(batch, tokens, device="cuda"), "int cond": torch.randint(0, 1000, (batch, tokens), device="cuda")}
    rows = []
    with torch.no_grad():
        for tag, m in models.items():
            m.cuda().eval()
            m.init_random(0)
            calls = {tag: lambda m=m, tag=tag: m(x, levels[tag], cond)}
            if tag == "int cond":
                calls["int table"] = lambda m=m: m(x, levels["int cond"])
            for path, fn in calls.items():
                fn()
                m.set_option("front_only", 1)
                front = timeit(fn, iters=50, warm=5)
                m.set_option("front_only", 0)
                whole = timeit(fn, iters=50, warm=5)
                rows.append((path, front, whole))
    for path, front, whole in rows:
        print(f"dit_front {name:10s} B={batch} T={tokens} {path:9s}: front end {front*1e3:8.1f} us  forward {whole:8.3f} ms", flush=True)
    f, c = rows[0], rows[1]
    print(f"dit_front {name:10s} float - int cond: front end {(f[1]-c[1])*1e3:+.1f} us, forward {(f[2]-c[2])*1e3:+.1f} us", flush=True)


def final_layer(hidden, oc_c, patch, hw, frames, form):
    """dfot_op_dit_final_layer alone: frames x (hw / patch)^2 rows -> (ms, rows, outputs per row)"""
    per_frame = (hw // patch) ** 2
    rows, oc = frames * per_frame, patch * patch * oc_c
    x = torch.randn(rows, hidden, device="cuda")
    table = 0.5 * torch.randn(frames, 2 * hidden, device="cuda")
    levels = torch.arange(frames, device="cuda", dtype=torch.int32)
    w = torch.randn(oc, hidden, device="cuda") / math.sqrt(hidden)
    b = torch.zeros(oc, device="cuda")
    out = torch.empty(frames, oc_c, hw, hw, device="cuda")
    ms = timeit(lambda: capi.check(capi.lib.dfot_op_dit_final_layer(P(x), P(table), P(levels), 2 * hidden, 0, P(w), P(b), P(out), hidden, per_frame, rows,
                                                                    1e-6, frames - 1, oc_c, hw, hw, patch, form, S())), iters=50, warm=5)
    return ms, rows, oc


def mcraft():
    """The Minecraft / dmlab recipe (`dataset=minecraft algorithm=dfot_video @diffusion/continuous @DiT/B`): latents 32x8x8, patch 2 (128-wide
    patch vector, 16 patches per frame), 16 frames, actions of dim 4.  The chunked final-layer launch alone next to the LDS-resident one at
    the K600 shape, one forward at batch 16, one training step at batch 8."""
    ms, rows, oc = final_layer(768, 32, 2, 8, 16 * 16, 2)
    print(f"mcraft final layer chunked  rows={rows} hidden=768 oc={oc}: {ms*1e3:8.1f} us  {ms * 1e6 / (rows * oc):6.3f} ns per (row x output), "
          f"weight {oc * 768 * 4 / 1024:.0f} KB per 16-row workgroup in 3 chunks", flush=True)
    ms, rows, oc = final_layer(1152, 16, 1, 16, 8 * 5, 1)
    print(f"mcraft final layer resident rows={rows} hidden=1152 oc={oc} (K600): {ms*1e3:8.1f} us  {ms * 1e6 / (rows * oc):6.3f} ns per (row x output), "
          f"weight {oc * 1152 * 4 / 1024:.0f} KB per 16-row workgroup", flush=True)
    ms, rows, oc = final_layer(1152, 16, 1, 16, 8 * 5, 2)
    print(f"mcraft final layer chunked  rows={rows} hidden=1152 oc={oc} (K600, one chunk): {ms*1e3:8.1f} us  {ms * 1e6 / (rows * oc):6.3f} ns per (row x output)",
          flush=True)
    bb = dict(name="dit3d", variant="full", pos_emb_type="rope_3d", patch_size=2, hidden_size=768, depth=12, num_heads=12, mlp_ratio=4.0,
              external_cond_dropout=0.1, use_fourier_noise_embedding=True)
    kw = dict(external_cond_type="action", external_cond_dim=4)
    model = dfot_amd.DiT3D(bb, x_shape=(32, 8, 8), max_tokens=16, **kw).cuda().eval()
    model.init_random(0)
    x = torch.randn(16, 16, 32, 8, 8, device="cuda")
    lv = 2.5 * torch.randn(16, 16, device="cuda")
    cond = torch.randn(16, 16, 4, device="cuda")
    with torch.no_grad():
        ms = timeit(lambda: model(x, lv, cond), iters=50, warm=5)
    print(f"mcraft forward @DiT/B B=16 T=16 (4096 rows): {ms:8.3f} ms", flush=True)
    tr = dfot_amd.DiT3DTrainer(bb, x_shape=(32, 8, 8), max_tokens=16, diffusion=dfot_amd.DiffusionConfig(is_continuous=True), **kw)
    tr.load_state_dict({k: v.detach() for k, v in model.state_dict().items()})
    g = torch.Generator(device="cuda").manual_seed(0)
    xs, noise = torch.randn(8, 16, 32, 8, 8, device="cuda", generator=g), torch.randn(8, 16, 32, 8, 8, device="cuda", generator=g)
    t = torch.rand(8, 16, device="cuda", generator=g)
    acts = torch.randn(8, 16, 4, device="cuda", generator=g)
    ms = timeit(lambda: tr.training_step(xs, t, noise, None, conditions=acts, dropout_generator=g), iters=20, warm=3)
    print(f"mcraft training step @DiT/B B=8 T=16, actions, continuous: {ms:8.2f} ms", flush=True)


HBM_TBS = 8.0  # the HBM3E rate the repository's rooflines use


def tattn(b, heads, tokens, patches, d):
    """temporal attention of the factorized-attention DiT: us and GB/s against the kernel's algorithmic bytes, (3 dstride + d) * 2 per
    (row, head): q, k, v rows as the QKV epilogue stores them (pad columns included) read once, the compact output written once"""
    ds = 64 if d <= 64 else 128
    q, k, v = (torch.zeros(b * tokens, heads, patches, ds, device="cuda", dtype=torch.bfloat16) for _ in range(3))
    for t, mul in ((q, 0.2), (k, 1.0), (v, 1.0)):
        t[..., :d] = (torch.randn(b * tokens, heads, patches, d, device="cuda") * mul).bfloat16()
    o = torch.empty(b * tokens * patches, heads * d, device="cuda", dtype=torch.bfloat16)
    ms = timeit(lambda: capi.check(capi.lib.dfot_op_attention_temporal(P(q), P(k), P(v), P(o), heads * d, b, tokens, patches, heads, d, S())),
                iters=50, warm=5)
    nbytes = b * tokens * patches * heads * (3 * ds + d) * 2.0
    return ms, nbytes / ms / 1e6, 4.0 * b * heads * patches * tokens * tokens * d / ms / 1e9


def attnmap():
    """the attention-map launches next to the forward attention launch whose q, k they re-read, at the K600 shape (DiT/XL full attention: 16
    heads, d 72, 5 frames x 256 patches) and the taichikl shapes (FacDiT temporal blocks: 16 frames x 256 patches; FacMatDiT XL-64-1 matrix
    blocks: 16 frames, E 64, h 1152, 1 x 16 heads); model batch 2.  us per launch (the frame forms include their finalize)."""
    b, heads, d, ds = 2, 16, 72, 128

    def padded(shape):
        t = torch.zeros(*shape, ds, device="cuda", dtype=torch.bfloat16)
        t[..., :d] = torch.randn(*shape, d, device="cuda").bfloat16()
        return t
    tokens, patches = 5, 256
    n = tokens * patches
    q, k, v = padded((b, heads, n)) * 0.2, padded((b, heads, n)), padded((b, heads, n))
    o = torch.empty(b * n, heads * d, device="cuda", dtype=torch.bfloat16)
    ws = torch.empty(capi.lib.dfot_op_attention_map_workspace_bytes(0, b, heads, tokens, patches) // 4, device="cuda")
    frame, full = torch.empty(b, heads, tokens, tokens, device="cuda"), torch.empty(b, heads, n, n, device="cuda")
    fwd = timeit(lambda: capi.check(capi.lib.dfot_op_attention_padded(P(q), P(k), P(v), P(o), heads * d, b, heads, n, d, S())), iters=50, warm=5)
    t_frame = timeit(lambda: capi.check(capi.lib.dfot_op_attention_map(P(q), P(k), P(frame), P(ws), ws.numel() * 4, capi.ATTN_MAP_FRAME, b, heads, n,
                                                                     tokens, d, S())), iters=50, warm=5)
    t_full = timeit(lambda: capi.check(capi.lib.dfot_op_attention_map(P(q), P(k), P(full), None, 0, capi.ATTN_MAP_FULL, b, heads, n, tokens, d, S())),
                    iters=50, warm=5)
    print(f"attnmap K600 full attention B={b} N={n} d={d}: forward {fwd*1e3:8.1f} us  frame map {t_frame*1e3:8.1f} us  full map {t_full*1e3:8.1f} us "
          f"({full.numel() * 4 / 1e6:.0f} MB written)", flush=True)
    tokens = 16
    q, k, v = padded((b * tokens, heads, patches)) * 0.2, padded((b * tokens, heads, patches)), padded((b * tokens, heads, patches))
    o = torch.empty(b * tokens * patches, heads * d, device="cuda", dtype=torch.bfloat16)
    ws = torch.empty(capi.lib.dfot_op_attention_map_workspace_bytes(1, b, heads, tokens, patches) // 4, device="cuda")
    frame = torch.empty(b, heads, tokens, tokens, device="cuda")
    fwd = timeit(lambda: capi.check(capi.lib.dfot_op_attention_temporal(P(q), P(k), P(v), P(o), heads * d, b, tokens, patches, heads, d, S())),
                 iters=50, warm=5)
    t_frame = timeit(lambda: capi.check(capi.lib.dfot_op_attention_temporal_map(P(q), P(k), P(frame), P(ws), ws.numel() * 4, b, tokens, patches, heads,
                                                                              d, S())), iters=50, warm=5)
    print(f"attnmap taichikl temporal B={b} T={tokens} P={patches} d={d}: forward {fwd*1e3:8.1f} us  frame map {t_frame*1e3:8.1f} us", flush=True)
    e, h, cc, rr = 64, 1152, 1, 16
    z = torch.randn(b * tokens * e, 3 * h, device="cuda").bfloat16()
    o = torch.empty(b * tokens * e, h, device="cuda", dtype=torch.bfloat16)
    ang = torch.arange(tokens, dtype=torch.float64)[:, None] / (10000.0 ** (torch.arange(0, h // rr, 2, dtype=torch.float64) / (h // rr)))
    table = torch.stack([ang.cos(), ang.sin()], -1).float().contiguous().cuda()
    m = torch.empty(b, cc, rr, tokens, tokens, device="cuda")
    scale = 1.0 / math.sqrt((e // cc) * (h // rr))
    fwd = timeit(lambda: capi.check(capi.lib.dfot_op_matrix_attention_rope(P(z), P(o), P(table), b, tokens, e, h, cc, rr, scale, S())), iters=50, warm=5)
    t_map = timeit(lambda: capi.check(capi.lib.dfot_op_matrix_attention_map(P(z), P(table), P(m), b, tokens, e, h, cc, rr, scale, S())), iters=50, warm=5)
    print(f"attnmap taichikl matrix B={b} L={tokens} E={e} h={h}: forward {fwd*1e3:8.1f} us  map {t_map*1e3:8.1f} us", flush=True)


def sattn64(b, heads, tokens, d):
    """per-frame spatial attention at 64 patches per frame (the taichi res-128 recipes): us of dfot_op_attention_seq64 over b * tokens
    sequences of 64, GB/s against its algorithmic bytes ((3 dstride + d) * 2 per (row, head), as tattn counts them), and next to it us of
    dfot_op_attention_padded at the same number of rows with n = 128: half as many sequences, twice as long -- the same bytes, twice the score
    FLOPs; the only yardstick there is, since that launcher cannot run n = 64"""
    ds, nseq = 64 if d <= 64 else 128, b * tokens
    q, k, v = (torch.zeros(nseq, heads, 64, ds, device="cuda", dtype=torch.bfloat16) for _ in range(3))
    for t, mul in ((q, 0.2), (k, 1.0), (v, 1.0)):
        t[..., :d] = (torch.randn(nseq, heads, 64, d, device="cuda") * mul).bfloat16()
    o = torch.empty(nseq * 64, heads * d, device="cuda", dtype=torch.bfloat16)
    ms = timeit(lambda: capi.check(capi.lib.dfot_op_attention_seq64(P(q), P(k), P(v), P(o), heads * d, nseq, heads, d, S())), iters=50, warm=5)
    # the same buffers read as nseq / 2 sequences of 128 (per head the rows of two neighbouring frames are not adjacent: another problem on the
    # same bytes, which is all a timing needs)
    ms128 = timeit(lambda: capi.check(capi.lib.dfot_op_attention_padded(P(q), P(k), P(v), P(o), heads * d, nseq // 2, heads, 128, d, S())),
                   iters=50, warm=5)
    return ms, nseq * 64 * heads * (3 * ds + d) * 2.0 / ms / 1e6, ms128


def attn_fc(b, heads, n, frame_len, d, rounds=7):
    """the frame-causal launch (dfot_op_attention_frame_causal) next to dfot_op_attention_padded on the same unit-normal operands, alternated
    over `rounds` rounds in one process: ([ms frame-causal], [ms padded]) per round; the non-causal launcher is the only yardstick there is
    (it computes another result: every (query tile, 128-key block) pair instead of the pairs on and below the block diagonal)"""
    ds = 64 if d <= 64 else 128
    q, k, v = (torch.zeros(b, heads, n, ds, device="cuda", dtype=torch.bfloat16) for _ in range(3))
    for t, mul in ((q, math.log2(math.e) / math.sqrt(d)), (k, 1.0), (v, 1.0)):
        t[..., :d] = (torch.randn(b, heads, n, d, device="cuda") * mul).bfloat16()
    o = torch.empty(b * n, heads * d, device="cuda", dtype=torch.bfloat16)
    fc, pad = [], []
    for _ in range(rounds):
        fc.append(timeit(lambda: capi.check(capi.lib.dfot_op_attention_frame_causal(P(q), P(k), P(v), P(o), heads * d, b, heads, n, frame_len, d, S())),
                         iters=100, warm=10))
        pad.append(timeit(lambda: capi.check(capi.lib.dfot_op_attention_padded(P(q), P(k), P(v), P(o), heads * d, b, heads, n, d, S())),
                          iters=100, warm=10))
    return fc, pad


def attn_fc_bwd(b, heads, n, frame_len, d, rounds=7):
    """the frame-causal backward (dfot_op_attention_frame_causal_bwd: delta + dQ + dK/dV kernels) next to the non-causal
    dfot_op_attention_bwd_lse on the same q, k, v, d_o, each with the o and lse of its own forward, alternated over `rounds` rounds in
    one process: ([ms frame-causal], [ms non-causal]) per round.  The frame-causal kernels stream a subset of the non-causal tile products"""
    ds = 64 if d <= 64 else 128
    q, k, v = (torch.zeros(b, heads, n, ds, device="cuda", dtype=torch.bfloat16) for _ in range(3))
    for t, mul in ((q, math.log2(math.e) / math.sqrt(d)), (k, 1.0), (v, 1.0)):
        t[..., :d] = (torch.randn(b, heads, n, d, device="cuda") * mul).bfloat16()
    d_o = torch.randn(b * n, heads * d, device="cuda").bfloat16()
    o_fc, o_nc = (torch.empty(b * n, heads * d, device="cuda", dtype=torch.bfloat16) for _ in range(2))
    lse_fc, lse_nc, delta = (torch.empty(b, heads, n, device="cuda", dtype=torch.float32) for _ in range(3))
    dq, dk, dv = (torch.empty_like(q) for _ in range(3))
    capi.check(capi.lib.dfot_op_attention_frame_causal_lse(P(q), P(k), P(v), P(o_fc), heads * d, P(lse_fc), b, heads, n, frame_len, d, S()))
    capi.check(capi.lib.dfot_op_attention_fwd_lse(P(q), P(k), P(v), P(o_nc), heads * d, P(lse_nc), b, heads, n, d, S()))
    fc, nc = [], []
    for _ in range(rounds):
        fc.append(timeit(lambda: capi.check(capi.lib.dfot_op_attention_frame_causal_bwd(P(q), P(k), P(v), P(o_fc), P(d_o), heads * d, P(lse_fc), P(delta),
                                                                                        P(dq), P(dk), P(dv), b, heads, n, frame_len, d, S())),
                         iters=50, warm=5))
        nc.append(timeit(lambda: capi.check(capi.lib.dfot_op_attention_bwd_lse(P(q), P(k), P(v), P(o_nc), P(d_o), heads * d, P(lse_nc), P(delta), P(dq),
                                                                               P(dk), P(dv), b, heads, n, d, S())),
                         iters=50, warm=5))
    return fc, nc


def seq64_bwd(nseq, heads, d, rounds=7):
    """the 64-token attention backward (dfot_op_attention_seq64_bwd, one launch) next to its forward (dfot_op_attention_seq64) on the same
    unit-normal operands and next to a device copy that moves the bytes the backward moves (4 reads + 3 writes of 64 x dstride bf16 per
    (sequence, head): a copy of 3.5 such tiles reads and writes as much), alternated over `rounds` rounds in one process:
    ([ms backward], [ms forward], [ms copy], bytes moved)"""
    ds = 64 if d <= 64 else 128
    q, k, v = (torch.zeros(nseq, heads, 64, ds, device="cuda", dtype=torch.bfloat16) for _ in range(3))
    for t, mul in ((q, math.log2(math.e) / math.sqrt(d)), (k, 1.0), (v, 1.0)):
        t[..., :d] = (torch.randn(nseq, heads, 64, d, device="cuda") * mul).bfloat16()
    d_o = torch.randn(nseq * 64, heads * d, device="cuda").bfloat16()
    o = torch.empty_like(d_o)
    dq, dk, dv = (torch.empty_like(q) for _ in range(3))
    nbytes = 7 * nseq * heads * 64 * ds * 2
    src = torch.randn(nbytes // 4, device="cuda").bfloat16()  # nbytes / 2 bytes read + nbytes / 2 written
    dst = torch.empty_like(src)
    bwd, fwd, cp = [], [], []
    for _ in range(rounds):
        bwd.append(timeit(lambda: capi.check(capi.lib.dfot_op_attention_seq64_bwd(P(q), P(k), P(v), P(d_o), heads * d, P(dq), P(dk), P(dv), nseq, heads,
                                                                                  d, S())), iters=100, warm=10))
        fwd.append(timeit(lambda: capi.check(capi.lib.dfot_op_attention_seq64(P(q), P(k), P(v), P(o), heads * d, nseq, heads, d, S())), iters=100, warm=10))
        cp.append(timeit(lambda: dst.copy_(src), iters=100, warm=10))
    return bwd, fwd, cp, nbytes


def seq64_bwd_packed(nseq, heads, d, rounds=7):
    """the packed form of the 64-token attention backward (dfot_op_attention_seq64_bwd_packed: one launch that stores dq | dk | dv into the
    rows of dqkv [nseq*64][3*heads*d]) next to the pair it replaces in a spatial block's backward (dfot_op_attention_seq64_bwd, then
    dfot_op_dit_qkv_grad_pack without a rope table) on the same unit-normal operands, and next to a device copy that moves the bytes the
    packed form moves (q, k, v tiles of 64 x dstride, d_o and dqkv rows of heads*d and 3*heads*d columns), alternated over `rounds` rounds
    in one process: ([ms packed], [ms pair], [ms copy], bytes moved)"""
    ds = 64 if d <= 64 else 128
    q, k, v = (torch.zeros(nseq, heads, 64, ds, device="cuda", dtype=torch.bfloat16) for _ in range(3))
    for t, mul in ((q, math.log2(math.e) / math.sqrt(d)), (k, 1.0), (v, 1.0)):
        t[..., :d] = (torch.randn(nseq, heads, 64, d, device="cuda") * mul).bfloat16()
    d_o = torch.randn(nseq * 64, heads * d, device="cuda").bfloat16()
    dq, dk, dv = (torch.empty_like(q) for _ in range(3))
    ldg = 3 * heads * d
    packed_out, pair_out = (torch.empty(nseq * 64, ldg, device="cuda", dtype=torch.bfloat16) for _ in range(2))
    nbytes = (3 * nseq * heads * 64 * ds + 4 * nseq * 64 * heads * d) * 2
    src = torch.randn(nbytes // 4, device="cuda").bfloat16()  # nbytes / 2 bytes read + nbytes / 2 written
    dst = torch.empty_like(src)

    def packed():
        capi.check(capi.lib.dfot_op_attention_seq64_bwd_packed(P(q), P(k), P(v), P(d_o), heads * d, P(packed_out), ldg, nseq, heads, d, S()))

    def pair():
        capi.check(capi.lib.dfot_op_attention_seq64_bwd(P(q), P(k), P(v), P(d_o), heads * d, P(dq), P(dk), P(dv), nseq, heads, d, S()))
        capi.check(capi.lib.dfot_op_dit_qkv_grad_pack(P(dq), P(dk), P(dv), None, P(pair_out), nseq * 64, 64, heads, d, ds, S()))
    packed(), pair()
    torch.cuda.synchronize()
    assert torch.equal(packed_out.view(torch.int16), pair_out.view(torch.int16)), "the two forms disagree"
    pk, pr, cp = [], [], []
    for _ in range(rounds):
        pk.append(timeit(packed, iters=100, warm=10))
        pr.append(timeit(pair, iters=100, warm=10))
        cp.append(timeit(lambda: dst.copy_(src), iters=100, warm=10))
    return pk, pr, cp, nbytes


def facdit_s128_train(b, mlp, rounds=7):
    """one training step (loss, backward, clip, AdamW) of FacDiT-S (hidden 384, depth 6, 6 heads; spatial_mlp_ratio 4 with `mlp`, else 0) at
    the taichi res-128 shape (4x16x16 latents, patch 2 = 64 patches per frame, 16 frames), with the spatial blocks' attention backward in
    its packed form and as the pair (three buffers + pack kernel), alternated on ONE trainer over `rounds` rounds: ([ms packed], [ms pair])"""
    bb = dict(name="dit3d", variant="factorized_attention", pos_emb_type="sinusoidal_factorized", patch_size=2, hidden_size=384, depth=6,
              num_heads=6, mlp_ratio=4.0, spatial_mlp_ratio=4.0 if mlp else 0.0)
    tr = dfot_amd.FacDiTTrainer(bb, x_shape=(4, 16, 16), max_tokens=16, allow_p64=True,
                                loss_weighting=dict(strategy="fused_min_snr", cum_snr_decay=0.96))
    model = dfot_amd.DiT3D(bb, x_shape=(4, 16, 16), max_tokens=16)  # for its init_random only
    model.init_random(0)
    tr.load_state_dict({n: t.detach() for n, t in model.state_dict().items()})
    del model
    xs, noise = torch.randn(b, 16, 4, 16, 16, device="cuda"), torch.randn(b, 16, 4, 16, 16, device="cuda")
    k = torch.randint(0, 1000, (b, 16))
    out = {1: [], 0: []}
    for _ in range(rounds):
        for form in (1, 0):
            capi.check(capi.lib.dfot_facdit_train_set_seq64_packed(tr._handle, form))
            out[form].append(timeit(lambda: tr.training_step(xs, k, noise), iters=10, warm=2))
    capi.check(capi.lib.dfot_facdit_train_set_seq64_packed(tr._handle, 1))
    return out[1], out[0]


def facmat_factor_wgrad(frames, ra, rb, hd, rounds=7):
    """a left-factor gradient of the FacMatDiT matrix block at 64 patches per frame (dfot_op_facmat_factor_wgrad: the partial-tile launch
    and the slice sum) on unit-normal operands a [frames][ra][hd], b [frames][rb][hd], next to a device copy of the bytes it reads (both
    operands once; the ra x rb fp32 result is noise next to them), alternated over `rounds` rounds in one process:
    ([ms op], [ms copy], bytes read)"""
    a = torch.randn(frames, ra, hd, device="cuda").bfloat16()
    b = torch.randn(frames, rb, hd, device="cuda").bfloat16()
    out = torch.empty(ra, rb, device="cuda")
    nbytes = (a.numel() + b.numel()) * 2
    src = torch.randn(nbytes // 2, device="cuda").bfloat16()  # a copy that READS nbytes (and writes as many)
    dst = torch.empty_like(src)
    op, cp = [], []
    for _ in range(rounds):
        op.append(timeit(lambda: capi.check(capi.lib.dfot_op_facmat_factor_wgrad(P(a), P(b), P(out), frames, ra, rb, hd, S())), iters=100, warm=10))
        cp.append(timeit(lambda: dst.copy_(src), iters=100, warm=10))
    return op, cp, nbytes


def facmat_s128_train(b, e, rounds=7):
    """one training step (loss, backward, clip, AdamW) of FacMatDiT-S-`e`-1 with use_bias (embed_row_dim 384, depth 6, 12 spatial heads, 6 row
    heads) at the taichi res-128 shape (4x16x16 latents, patch 2 = 64 patches per frame, 16 frames): [ms] over `rounds` rounds"""
    bb = dict(name="dit3d", variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", use_temporal_rope=True, patch_size=2,
              embed_col_dim=e, embed_row_dim=384, num_heads=12, num_col_heads=1, num_row_heads=6, depth=6, mlp_ratio=4.0, spatial_mlp_ratio=4.0,
              use_bias=True, matrix_block="matrix")
    tr = dfot_amd.FacMatDiTTrainer(bb, x_shape=(4, 16, 16), max_tokens=16, allow_p64=True,
                                   loss_weighting=dict(strategy="fused_min_snr", cum_snr_decay=0.96))
    model = dfot_amd.DiT3D(bb, x_shape=(4, 16, 16), max_tokens=16)  # for its init_random only
    model.init_random(0)
    tr.load_state_dict({n: t.detach() for n, t in model.state_dict().items()})
    del model
    xs, noise = torch.randn(b, 16, 4, 16, 16, device="cuda"), torch.randn(b, 16, 4, 16, 16, device="cuda")
    k = torch.randint(0, 1000, (b, 16))
    return [timeit(lambda: tr.training_step(xs, k, noise), iters=10, warm=2) for _ in range(rounds)]


def dit1d_forward(b, rounds=5):
    """whole forward of DiT1D at the stock dit1d.yaml widths (hidden 1152, depth 28, 16 heads) on the taichi token latents [4, 1, 32] x 16 frames,
    frame-causal and unmasked, next to DiT3D @DiT/XL patch 1 (full attention, RoPE-3D) on the same latents, alternated in one process:
    {name: [ms per round]}.  Not the same amount of work: a DiT1D block carries a 4x MLP (12 H^2 weights), a `full` DiT3D block at @DiT/XL
    (spatial_mlp_ratio unset) none (4 H^2)"""
    bb1 = dict(name="dit1d", hidden_size=1152, depth=28, num_heads=16, mlp_ratio=4, learn_sigma=False, merge_mode="share_norm",
               causal_attn_mode="video_temporal_causal", use_rotary_emb=False, qk_norm=False)
    bb3 = dict(name="dit3d", variant="full", pos_emb_type="rope_3d", patch_size=1, hidden_size=1152, depth=28, num_heads=16)
    models = {"DiT1D frame-causal": dfot_amd.DiT1D(bb1, x_shape=(4, 1, 32), max_tokens=16),
              "DiT1D no mask": dfot_amd.DiT1D(dict(bb1, causal_attn_mode=None), x_shape=(4, 1, 32), max_tokens=16),
              "DiT3D XL patch 1": dfot_amd.DiT3D(bb3, x_shape=(4, 1, 32), max_tokens=16)}
    for m in models.values():
        m.cuda().eval()
        m.init_random(0)
    x = torch.randn(b, 16, 4, 1, 32, device="cuda")
    k = torch.randint(0, 1000, (b, 16), device="cuda")
    out = {name: [] for name in models}
    with torch.no_grad():
        for _ in range(rounds):
            for name, model in models.items():
                out[name].append(timeit(lambda: model(x, k), iters=10, warm=3))
    return out


def dit1d_train_ops(rows=4096, hidden=1152, per=32, rounds=7):
    """the share_norm LayerNorm kernels of DiT1D training alone at rows x hidden (one table row per frame of `per` rows), next to the DiT3D
    pair that does the same job with one fp32 input stream fewer (dfot_op_dit_ln_bwd: ln_bwd_rows + ln_bwd_frames + the plane sum),
    alternated in one process: {name: ([ms per round], algorithmic bytes)}"""
    frames, ldt = rows // per, 6 * hidden
    x, dres, dm = (torch.randn(rows, hidden, device="cuda") for _ in range(3))
    table = torch.randn(frames, ldt, device="cuda")
    n, rstd, m = torch.empty_like(x), torch.empty(rows, device="cuda"), torch.empty(rows, hidden, dtype=torch.bfloat16, device="cuda")
    dx, stats = torch.empty_like(x), torch.empty(rows, 2, device="cuda")
    part, dmod = torch.zeros(4, frames, ldt, device="cuda"), torch.zeros(frames, ldt, device="cuda")
    lib = capi.lib
    fb = rows * hidden * 4  # one fp32 stream
    runs = {
        "ln_share_train": (lambda: capi.check(lib.dfot_op_dit1d_ln_share_train(P(x), P(n), P(rstd), P(m), P(table), ldt, 0, hidden, per, rows, 1e-6, S())),
                           2 * fb + fb // 2),
        "ln_share_bwd": (lambda: capi.check(lib.dfot_op_dit1d_ln_share_bwd(P(dres), P(dm), P(n), P(rstd), P(table), ldt, 0, P(dx), P(part), hidden, per,
                                                                           frames, S())), 4 * fb),
        "dit ln_bwd (rows + frames + plane sum)": (lambda: capi.check(lib.dfot_op_dit_ln_bwd(P(dm), P(x), P(table), ldt, 0, P(dx), P(stats), P(part), P(dmod),
                                                                                            hidden, per, frames, 1e-6, S())), 3 * fb + 2 * fb),
    }
    out = {name: ([], nbytes) for name, (_, nbytes) in runs.items()}
    for _ in range(rounds):
        for name, (fn, _) in runs.items():
            out[name][0].append(timeit(fn))
    return out


def dit1d_train(b, depth=28):
    """one training step (loss, backward, AdamW) of DiT1D at the stock dit1d.yaml widths on 16 frames of [4, 1, 32], ms"""
    bb = dict(name="dit1d", hidden_size=1152, depth=depth, num_heads=16, mlp_ratio=4, learn_sigma=False, merge_mode="share_norm",
              causal_attn_mode="video_temporal_causal", use_rotary_emb=False, qk_norm=False)
    tr = dfot_amd.DiT1DTrainer(bb, x_shape=(4, 1, 32), max_tokens=16, loss_weighting=dict(strategy="fused_min_snr", cum_snr_decay=0.96))
    model = dfot_amd.DiT1D(bb, x_shape=(4, 1, 32), max_tokens=16)  # for its init_random only
    model.init_random(0)
    tr.load_state_dict({n: t.detach() for n, t in model.state_dict().items()})
    del model
    xs, noise = torch.randn(b, 16, 4, 1, 32, device="cuda"), torch.randn(b, 16, 4, 1, 32, device="cuda")
    k = torch.randint(0, 1000, (b, 16))
    return timeit(lambda: tr.training_step(xs, k, noise), iters=5, warm=2)


def facmat_narrow_ops(frames, p, h, e):
    """the two left-factor kernels of csrc/facmat_narrow.hip at one shape: (us, algorithmic bytes) of contract and expand, and us of a device
    copy of each launch's byte count timed in the same run (a copy of n bytes reads n / 2 and writes n / 2)"""
    m = torch.randn(frames, p, h, device="cuda").bfloat16()
    o = torch.randn(frames, e, h, device="cuda").bfloat16()
    uc = (torch.randn(e, p, device="cuda") / math.sqrt(p)).bfloat16()
    ue = (torch.randn(p, e, device="cuda") / math.sqrt(e)).bfloat16()
    w, s = torch.empty_like(o), torch.empty_like(m)
    nbytes = 2.0 * (frames * p * h + frames * e * h + e * p)  # either direction: the big tile once, the small one once, u once
    src = torch.empty(int(nbytes) // 2, device="cuda", dtype=torch.uint8)
    dst = torch.empty_like(src)
    out = []
    for _ in range(5):  # alternate the three launches; the median of each
        out.append((timeit(lambda: capi.check(capi.lib.dfot_op_facmat_contract(P(m), P(uc), P(w), frames, p, h, e, S())), iters=50, warm=5),
                    timeit(lambda: capi.check(capi.lib.dfot_op_facmat_expand(P(o), P(ue), P(s), frames, p, h, e, S())), iters=50, warm=5),
                    timeit(lambda: dst.copy_(src), iters=50, warm=5)))
    med = lambda i: sorted(t[i] for t in out)[len(out) // 2]  # noqa: E731
    return med(0), med(1), med(2), nbytes


def facmat_narrow_forward(widths, b, rounds=5):
    """whole forwards of @FacMatDiT/S-<E>-<cc> (depth 6, use_bias, temporal RoPE) at the res-128 shape -- 4x16x16 latents, patch 2 (64 patches),
    16 frames -- for every (E, cc) of `widths`, alternated over `rounds` rounds in one process: {(E, cc): [ms per round]}"""
    models = {}
    for e, cc in widths:
        bb = dict(name="dit3d", variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", use_temporal_rope=True, patch_size=2,
                  embed_col_dim=e, embed_row_dim=384, num_heads=12, num_col_heads=cc, num_row_heads=6, depth=6, mlp_ratio=4.0,
                  spatial_mlp_ratio=4.0, use_bias=True, matrix_block="matrix")
        models[(e, cc)] = dfot_amd.DiT3D(bb, x_shape=(4, 16, 16), max_tokens=16).cuda().eval()
        models[(e, cc)].init_random(0)
    x = torch.randn(b, 16, 4, 16, 16, device="cuda")
    k = torch.randint(0, 1000, (b, 16), device="cuda")
    out = {w: [] for w in widths}
    with torch.no_grad():
        for _ in range(rounds):
            for w, model in models.items():
                out[w].append(timeit(lambda: model(x, k), iters=50, warm=5))
    return out


def p64_forward(kind, b):
    """whole forward of FacDiT-S / FacMatDiT-S-64-1 (depth 6) at the res-128 shape: 4x16x16 latents, patch 2 (64 patches), 16 frames; ms"""
    if kind == "facdit":
        bb = dict(name="dit3d", variant="factorized_attention", pos_emb_type="sinusoidal_factorized", patch_size=2, hidden_size=384, depth=6,
                  num_heads=6, mlp_ratio=4.0, spatial_mlp_ratio=0.0)
    else:
        bb = dict(name="dit3d", variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", use_temporal_rope=True, patch_size=2,
                  embed_col_dim=64, embed_row_dim=384, num_heads=12, num_col_heads=1, num_row_heads=6, depth=6, mlp_ratio=4.0,
                  spatial_mlp_ratio=4.0, use_bias=True, matrix_block="matrix")
    model = dfot_amd.DiT3D(bb, x_shape=(4, 16, 16), max_tokens=16).cuda().eval()
    model.init_random(0)
    x = torch.randn(b, 16, 4, 16, 16, device="cuda")
    k = torch.randint(0, 1000, (b, 16), device="cuda")
    with torch.no_grad():
        return timeit(lambda: model(x, k), iters=20, warm=5)


def facdit_forward(b):
    """whole forward of FacDiT-XL at the taichikl shape (4x32x32 latents, patch 2, 16 frames), ms; attention launches timed on their own"""
    bb = dict(name="dit3d", variant="factorized_attention", pos_emb_type="sinusoidal_factorized", patch_size=2, hidden_size=1152, depth=28,
              num_heads=16, mlp_ratio=4.0, spatial_mlp_ratio=0.0)
    model = dfot_amd.DiT3D(bb, x_shape=(4, 32, 32), max_tokens=16).cuda().eval()
    model.init_random(0)
    x = torch.randn(b, 16, 4, 32, 32, device="cuda")
    k = torch.randint(0, 1000, (b, 16), device="cuda")
    with torch.no_grad():
        return timeit(lambda: model(x, k), iters=10, warm=3)


def tattn_bwd(b, heads, tokens, patches, d):
    """backward of the temporal attention on unit-normal operands: ms of dfot_op_attention_temporal_bwd, ms of the forward on the same q, k,
    v in the same process, and the backward's algorithmic bytes, (6 dstride + d) * 2 per (row, head): q, k, v rows read once (pad columns
    included) and dq, dk, dv rows counted whole, the compact d_o read once"""
    ds = 64 if d <= 64 else 128
    q, k, v = (torch.zeros(b * tokens, heads, patches, ds, device="cuda", dtype=torch.bfloat16) for _ in range(3))
    for t, mul in ((q, 0.2), (k, 1.0), (v, 1.0)):
        t[..., :d] = (torch.randn(b * tokens, heads, patches, d, device="cuda") * mul).bfloat16()
    d_o = torch.randn(b * tokens * patches, heads * d, device="cuda").bfloat16()
    o = torch.empty_like(d_o)
    dq, dk, dv = (torch.zeros_like(q) for _ in range(3))
    ms_bwd = timeit(lambda: capi.check(capi.lib.dfot_op_attention_temporal_bwd(P(q), P(k), P(v), P(d_o), heads * d, P(dq), P(dk), P(dv), b, tokens,
                                                                              patches, heads, d, S())), iters=50, warm=5)
    ms_fwd = timeit(lambda: capi.check(capi.lib.dfot_op_attention_temporal(P(q), P(k), P(v), P(o), heads * d, b, tokens, patches, heads, d, S())),
                    iters=50, warm=5)
    return ms_bwd, ms_fwd, b * tokens * patches * heads * (6 * ds + d) * 2.0


def facdit_train(b, depth=28):
    """one training step (loss, backward, AdamW) of FacDiT-XL (@DiT/XL widths, both MLP ratios 4) at the taichikl shape (4x32x32 latents,
    patch 2, 16 frames), ms"""
    bb = dict(name="dit3d", variant="factorized_attention", pos_emb_type="sinusoidal_factorized", patch_size=2, hidden_size=1152, depth=depth,
              num_heads=16, mlp_ratio=4.0, spatial_mlp_ratio=4.0)
    tr = dfot_amd.FacDiTTrainer(bb, x_shape=(4, 32, 32), max_tokens=16, loss_weighting=dict(strategy="fused_min_snr", cum_snr_decay=0.96))
    model = dfot_amd.DiT3D(bb, x_shape=(4, 32, 32), max_tokens=16)  # for its init_random only
    model.init_random(0)
    tr.load_state_dict({n: t.detach() for n, t in model.state_dict().items()})
    del model
    xs, noise = torch.randn(b, 16, 4, 32, 32, device="cuda"), torch.randn(b, 16, 4, 32, 32, device="cuda")
    k = torch.randint(0, 1000, (b, 16))
    return timeit(lambda: tr.training_step(xs, k, noise), iters=5, warm=2)


def uvit3d_forward(b=2):
    """whole forward of the pose-free UViT3D next to UViT3DPose.forward_cached (the pose caches built once, outside the timed region) at the
    RE10K widths, 256x256 frames, 8 tokens, model batch b, same process: (ms pose-free, ms pose)"""
    from bench import RE10K
    x = torch.randn(b, 8, 3, 256, 256, device="cuda")
    k = torch.randn(b, 8, device="cuda")
    out = []
    with torch.no_grad():
        free = dfot_amd.UViT3D({n: v for n, v in RE10K.items() if n != "conditioning"}, x_shape=(3, 256, 256), max_tokens=8, external_cond_dim=0).cuda().eval()
        free.init_random(0)
        out.append(timeit(lambda: free(x, k), iters=10, warm=3))
        del free
        torch.cuda.empty_cache()
        pose = dfot_amd.UViT3DPose(RE10K, x_shape=(3, 256, 256), max_tokens=8).cuda().eval()
        pose.init_random(0)
        cond = torch.randn(b, 8, 180, 256, 256, device="cuda")
        out.append(timeit(lambda: pose(x, k, cond), iters=10, warm=3))  # the same cond tensor every call: the cache hits by identity
    return tuple(out)


def uvit3d_train(b):
    """one training step (loss, backward, clipped AdamW) of UViT3DTrainer at the `examples/train.py uvit3d --full` shape (u_vit3d.yaml widths,
    8 heads, 8 frames of 3 x 256 x 256), MLP dropout on: (ms per step, peak device memory in GiB).  The FiLM path is the process's
    DFOT_UVIT3D_TRAIN_ROW_FILM (1 = the per-row yardstick), so the two paths are timed in alternating processes"""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from train import uvit3d_cfg
    cfg, res = uvit3d_cfg(True)
    init = dfot_amd.UViT3D(cfg, x_shape=(3, res, res), max_tokens=8, external_cond_dim=0)
    init.init_random(seed=0)
    tr = dfot_amd.UViT3DTrainer({k: v.detach() for k, v in init.state_dict().items()}, dict(cfg, resolution=res, max_tokens=8, in_channels=3, cond_dim=0))
    del init
    tr.dropout_generator = torch.Generator(device="cuda").manual_seed(0)
    g = torch.Generator().manual_seed(1)
    xs, noise = torch.randn(b, 8, 3, res, res, generator=g), torch.randn(b, 8, 3, res, res, generator=g)
    t = torch.rand(b, 8, generator=g)

    def step():
        tr.loss_and_grads(xs, None, t, noise)
        tr.optimizer_step(lr=5e-5)
    torch.cuda.reset_peak_memory_stats()
    ms = timeit(step, iters=5, warm=2)
    return ms, torch.cuda.max_memory_allocated() / 2 ** 30, tr.row_film


def gnfilm_frame(bt=64):
    """the four per-frame FiLM norm ops next to their per-row counterparts at levels 0-3 of the `uvit3d --full` shape with B 8, T 8
    (64 frames; GroupNorm at 128 / 256 channels, RMS at 512 / 1024): [(level, op, us frame, us row)].  The per-row backward is timed with the
    frame_sums pass it needs for the same result"""
    L = capi.lib
    BF = torch.bfloat16
    out = []
    for lvl, (c, r) in enumerate(((128, 128), (256, 64), (512, 32), (1024, 16))):
        P_, rows = r * r, bt * r * r
        x = torch.randn(rows, c, device="cuda")
        tab = torch.randn(bt, 2 * c, device="cuda") * 0.3
        film = tab.to(BF).repeat_interleave(P_, 0).contiguous()
        o = torch.empty(rows, c, dtype=BF, device="cuda")
        dx, dxb = torch.empty(rows, c, device="cuda"), torch.empty(rows, c, dtype=BF, device="cuda")
        dfilm, dtab, sums = torch.empty(rows, 2 * c, dtype=BF, device="cuda"), torch.empty(bt, 2 * c, device="cuda"), torch.empty(bt, 2 * c, device="cuda")
        v1, v2, v3 = (torch.randn(c, device="cuda") for _ in range(3))
        fs = lambda: capi.check(L.dfot_op_frame_sums_bf16(P(dfilm), 2 * c, P(sums), bt, P_, 2 * c, S()))
        if lvl < 2:
            stats = torch.empty(bt, 32, 2, device="cuda")
            dy = torch.randn(rows, c, device="cuda").to(BF)
            pairs = {
                "gn_silu_fwd": (lambda: capi.check(L.dfot_op_gn_silu_fwd_frame(P(x), P(v1), P(v2), P(tab), 2 * c, 1e-6, P(o), P(stats), bt, P_, c, S())),
                                lambda: capi.check(L.dfot_op_gn_silu_fwd2(P(x), P(v1), P(v2), P(film), 2 * c, 1e-6, P(o), P(stats), bt, P_, c, S()))),
                "gn_silu_bwd": (lambda: capi.check(L.dfot_op_gn_silu_bwd_frame(P(x), P(dy), P(stats), P(v1), P(v2), P(tab), 2 * c, None, None, P(dxb), P(dtab),
                                                                              2 * c, P(v3), P(v3), bt, P_, c, S())),
                                lambda: (capi.check(L.dfot_op_gn_silu_bwd6(P(x), P(dy), P(stats), P(v1), P(v2), P(film), 2 * c, None, None, P(dxb), P(dfilm),
                                                                          2 * c, P(v3), P(v3), bt, P_, c, S())), fs())),
            }
        else:
            dxn, dres = torch.randn(rows, c, device="cuda"), torch.randn(rows, c, device="cuda")
            pairs = {
                "rms_film_fwd": (lambda: capi.check(L.dfot_op_rms_film_fwd_frame(P(x), P(v1), P(tab), 2 * c, 1e-6, P(o), rows, P_, c, S())),
                                 lambda: capi.check(L.dfot_op_rms_film_fwd(P(x), P(v1), P(film), 1e-6, P(o), rows, c, S()))),
                "rms_film_bwd": (lambda: capi.check(L.dfot_op_rms_film_bwd_frame(P(x), P(dxn), P(v1), P(tab), 2 * c, 1e-6, P(dres), P(dx), P(dxb), P(dtab), 2 * c,
                                                                                P(v3), rows, P_, c, S())),
                                 lambda: (capi.check(L.dfot_op_rms_film_bwd_res(P(x), P(dxn), P(v1), P(film), 1e-6, P(dres), P(dx), P(dxb), P(dfilm), P(v3),
                                                                               rows, c, S())), fs())),
            }
        for name, (frame, row) in pairs.items():
            for _ in range(3):  # alternate the two forms
                out.append((lvl, name, c, rows, timeit(frame, iters=20, warm=3) * 1e3, timeit(row, iters=20, warm=3) * 1e3))
    return out


def mattn(b, tokens, e, h, cc, rr, rope):
    """matrix attention of the FacMatDiT backbone on one (q|k|v) matrix: us of dfot_op_matrix_attention_rope (with and without the table) and of
    the DifferenceDiT3D launcher (dfot_op_matrix_attention: no rotation; one pair of tokens per wave pass at the lengths it has no register form
    for), GB/s against the algorithmic bytes -- q, k, v read once, o written once"""
    hd = h // rr
    z = torch.randn(b * tokens * e, 3 * h, device="cuda").bfloat16()
    o = torch.empty(b * tokens * e, h, device="cuda", dtype=torch.bfloat16)
    ang = torch.arange(tokens, dtype=torch.float64)[:, None] * 10000.0 ** (-torch.arange(0, hd, 2, dtype=torch.float64) / hd)[None]
    table = torch.stack([ang.cos(), ang.sin()], -1).float().cuda().contiguous()
    scale = 1.0 / math.sqrt((e // cc) * hd)
    new = lambda t: timeit(lambda: capi.check(capi.lib.dfot_op_matrix_attention_rope(P(z), P(o), P(t) if rope and t is not None else None, b, tokens, e,
                                                                                      h, cc, rr, scale, S())), iters=50, warm=5)
    ms_rope, ms_plain = new(table), new(None)
    ms_old = timeit(lambda: capi.check(capi.lib.dfot_op_matrix_attention(P(z), P(o), b, tokens, e, h, cc, rr, scale, S())), iters=50, warm=5)
    return ms_rope, ms_plain, ms_old, b * tokens * e * 4.0 * h * 2.0


def facmat_forward(b, row=1152, heads=16, depth=28):
    """whole forward of FacMatDiT (XL-64-1 by default) at the taichikl shape (4x32x32 latents, patch 2, 16 frames), ms"""
    bb = dict(name="dit3d", variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", use_temporal_rope=True, patch_size=2,
              embed_col_dim=64, embed_row_dim=row, num_heads=heads, num_col_heads=1, num_row_heads=heads, depth=depth, mlp_ratio=4.0,
              spatial_mlp_ratio=4.0, use_bias=False, matrix_block="matrix")
    model = dfot_amd.DiT3D(bb, x_shape=(4, 32, 32), max_tokens=16).cuda().eval()
    model.init_random(0)
    x = torch.randn(b, 16, 4, 32, 32, device="cuda")
    k = torch.randint(0, 1000, (b, 16), device="cuda")
    with torch.no_grad():
        return timeit(lambda: model(x, k), iters=10, warm=3)


def mattn_bwd(b, tokens, e, h, cc, rr):
    """backward of the FacMatDiT matrix attention on one (q|k|v) matrix and a unit-normal d_o: us of dfot_op_matrix_attention_rope_bwd with and
    without the table, us of the forward on the same input, and the algorithmic bytes -- q, k, v, d_o read once, dq, dk, dv written once"""
    hd = h // rr
    z = torch.randn(b * tokens * e, 3 * h, device="cuda").bfloat16()
    d_o = torch.randn(b * tokens * e, h, device="cuda").bfloat16()
    dz, o = torch.empty_like(z), torch.empty_like(d_o)
    ang = torch.arange(tokens, dtype=torch.float64)[:, None] * 10000.0 ** (-torch.arange(0, hd, 2, dtype=torch.float64) / hd)[None]
    table = torch.stack([ang.cos(), ang.sin()], -1).float().cuda().contiguous()
    scale = 1.0 / math.sqrt((e // cc) * hd)
    bwd = lambda t: timeit(lambda: capi.check(capi.lib.dfot_op_matrix_attention_rope_bwd(P(z), P(d_o), None if t is None else P(t), P(dz), b, tokens, e,
                                                                                          h, cc, rr, scale, S())), iters=50, warm=5)
    ms_rope, ms_plain = bwd(table), bwd(None)
    ms_fwd = timeit(lambda: capi.check(capi.lib.dfot_op_matrix_attention_rope(P(z), P(o), P(table), b, tokens, e, h, cc, rr, scale, S())), iters=50, warm=5)
    return ms_rope, ms_plain, ms_fwd, b * tokens * e * 7.0 * h * 2.0


def facmat_train(b, row=1152, heads=16, depth=28):
    """one training step (loss, backward, AdamW) of FacMatDiT (XL-64-1 by default: use_bias, both MLP ratios 4) at the taichikl shape
    (4x32x32 latents, patch 2, 16 frames), ms"""
    bb = dict(name="dit3d", variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", use_temporal_rope=True, patch_size=2,
              embed_col_dim=64, embed_row_dim=row, num_heads=heads, num_col_heads=1, num_row_heads=heads, depth=depth, mlp_ratio=4.0,
              spatial_mlp_ratio=4.0, use_bias=True, matrix_block="matrix")
    tr = dfot_amd.FacMatDiTTrainer(bb, x_shape=(4, 32, 32), max_tokens=16, loss_weighting=dict(strategy="fused_min_snr", cum_snr_decay=0.96))
    model = dfot_amd.DiT3D(bb, x_shape=(4, 32, 32), max_tokens=16)  # for its init_random only
    model.init_random(0)
    tr.load_state_dict({n: t.detach() for n, t in model.state_dict().items()})
    del model
    xs, noise = torch.randn(b, 16, 4, 32, 32, device="cuda"), torch.randn(b, 16, 4, 32, 32, device="cuda")
    k = torch.randint(0, 1000, (b, 16))
    return timeit(lambda: tr.training_step(xs, k, noise), iters=5, warm=2)


def vae_encode(b=2, t=17, res=128):
    """VideoVAE encoder (K600: hidden 128, z 16) on b videos of t x res x res frames: the whole encode_videos after warm-up, then every
    convolution shape of the plan on its own, grouped by class.  FLOPs are the reference's (true channel counts), from the shapes here."""
    enc = dfot_amd.VideoVAEEncoder(z_channels=16, embed_dim=16, resolution=res, temporal_length=17).cuda()
    enc.init_random(seed=0)
    videos = torch.rand(b, t, 3, res, res, device="cuda")
    noise = torch.randn(b, (t - 1) // 4 + 1, 16, res // 8, res // 8, device="cuda")
    ms = timeit(lambda: dfot_amd.encode_videos(enc, videos, vae_batch_size=b, noise=noise), iters=10, warm=3)
    # (class, count, B, T_in, H_in, W_in, true Cin, Cin as run, Cout, kt, s, st)
    c = [128, 256, 512, 512]
    t1, t2 = (t - 1) // 2 + 1, (t - 1) // 4 + 1
    r1, r2, r3 = res // 2, res // 4, res // 8
    convs = [("2-D stride 1", 1, b, t, res, res, 3, 64, c[0], 1, 1, 1),                      # conv_in
             ("2-D stride 1", 4, b, t, res, res, c[0], c[0], c[0], 1, 1, 1),              # level 0 res blocks
             ("2-D stride 2", 1, b, t, res, res, c[0], c[0], c[0], 1, 2, 1),              # level 0 Downsample
             ("2-D stride 1", 1, b, t, r1, r1, c[0], c[0], c[1], 1, 1, 1),
             ("2-D stride 1", 3, b, t, r1, r1, c[1], c[1], c[1], 1, 1, 1),                # level 1 res blocks
             ("3x3x3 stride 2", 1, b, t, r1, r1, c[1], c[1], c[1], 3, 2, 2),              # level 1 downsample
             ("3x3x3 stride 1", 1, b, t1, r2, r2, c[1], c[1], c[2], 3, 1, 1),
             ("3x3x3 stride 1", 3, b, t1, r2, r2, c[2], c[2], c[2], 3, 1, 1),             # level 2 res blocks
             ("3x3x3 stride 2", 1, b, t1, r2, r2, c[2], c[2], c[2], 3, 2, 2),             # level 2 downsample
             ("3x3x3 stride 1", 8, b, t2, r3, r3, c[3], c[3], c[3], 3, 1, 1),             # level 3 + mid res blocks
             ("3x3x3 stride 1", 1, b, t2, r3, r3, c[3], c[3], 32, 3, 1, 1)]               # conv_out (run with 64 output columns)
    total_flop = 0.0
    by_class = {}
    for cls, n, bb, tt, hh, ww, ci_true, ci, co, kt, s, st in convs:
        to, ho, wo = (tt - 1) // st + 1, hh // s, ww // s
        flop = 2.0 * bb * to * ho * wo * co * kt * 9 * ci_true
        co_run = -(-co // 64) * 64
        a = torch.randn(bb, tt, hh, ww, ci, device="cuda").bfloat16()
        wt = (torch.randn(co_run, kt * 9 * ci, device="cuda") / math.sqrt(kt * 9 * ci)).bfloat16()
        out = torch.empty(bb, to, ho, wo, co_run, device="cuda")
        if kt == 1 and s == 1:
            fn = lambda: capi.check(capi.lib.dfot_op_conv3x3_f32(P(a), P(wt), None, None, P(out), bb * tt, hh, ww, ci, co_run, S()))
        else:
            fn = lambda: capi.check(capi.lib.dfot_op_conv3t_f32(P(a), P(wt), None, None, P(out), bb, tt, hh, ww, ci, co_run, kt, s, st, S()))
        cms = timeit(fn)
        print(f"vae_encode conv {cls:14s} x{n} {bb}x{tt}x{hh}x{ww} {ci_true}->{co} kt={kt} s={s} st={st}: {cms*1e3:8.1f} us  "
              f"{flop / cms / 1e9:7.1f} TF/s", flush=True)
        e = by_class.setdefault(cls, [0.0, 0.0])
        e[0] += n * cms
        e[1] += n * flop
        total_flop += n * flop
    # the rest of the plan: 1x1 shortcuts, attention projections and products, quant_conv
    other = 2.0 * b * t * r1 * r1 * c[0] * c[1] + 2.0 * b * t1 * r2 * r2 * c[1] * c[2]
    other += b * t2 * (4 * 2.0 * r3 * r3 * c[3] * c[3] + 2 * 2.0 * (r3 * r3) ** 2 * c[3]) + 2.0 * b * t2 * r3 * r3 * 32 * 32
    total_flop += other
    for cls, (cms, flop) in by_class.items():
        print(f"vae_encode class {cls:14s}: {cms:7.3f} ms per {b} videos  {flop / 1e12:6.3f} TFLOP  {flop / cms / 1e9:7.1f} TF/s  "
              f"({flop / cms / 1e9 / 2500:.2f} of the 2.5 PF bf16 peak)", flush=True)
    print(f"vae_encode {b} x {t} x {res}^2: {ms:.3f} ms = {ms / b:.3f} ms per video, {total_flop / b / 1e12:.3f} TFLOP per video, "
          f"{total_flop / ms / 1e9:.1f} TF/s", flush=True)


def equal(nbytes):
    """dfot_op_equal_bits on two equal buffers (the worst case: nothing ends early, every byte of both is read): us and GB/s of the
    2 x nbytes it reads"""
    a = torch.randn(nbytes // 4, device="cuda")
    b = a.clone()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ms = timeit(lambda: capi.check(capi.lib.dfot_op_equal_bits(P(a), P(b), nbytes, P(flag), S())), iters=50, warm=5)
    assert int(flag.item()) == 0
    return ms, 2.0 * nbytes / ms / 1e6


def ivae():
    """the three ImageVAE ops (csrc/image_vae.hip) at the image_vae.yaml recipe's shapes, the per-frame loop of existing ops that the
    fused attention replaces (vae.py:_attn), and a whole decode / encode of 16 frames at 128 x 128 and at 256 x 256.  The attention runs
    at N = 256 (a 128 x 128 frame: the register-resident kernel) and at N = 1024 (a 256 x 256 frame: the streaming kernel).  Each figure:
    the median of 7 repeats of (3 warm-up + 20 timed launches between two HIP events)."""
    import statistics
    med = lambda fn: statistics.median(timeit(fn) for _ in range(7))
    c = 512
    for n, frames in ((256, 16), (256, 128), (1024, 16), (1024, 128)):
        q, k, v = (torch.randn(frames * n, c, device="cuda").bfloat16() for _ in range(3))
        o = torch.empty_like(q)
        ms = med(lambda: capi.check(capi.lib.dfot_op_ivae_attention(P(q), P(k), P(v), P(o), frames, n, c, S())))
        scores, probs = torch.empty(n, n, device="cuda"), torch.empty(n, n, dtype=torch.bfloat16, device="cuda")
        vt, o2 = torch.empty(c, n, dtype=torch.bfloat16, device="cuda"), torch.empty_like(q)

        def loop():
            for f in range(frames):
                qf, kf, vf, of = (a[f * n:(f + 1) * n] for a in (q, k, v, o2))
                capi.check(capi.lib.dfot_op_gemm_f32(P(qf), c, P(kf), None, None, P(scores), n, n, n, c, S()))
                capi.check(capi.lib.dfot_op_softmax_rows(P(scores), P(probs), n, n, float(c) ** -0.5, S()))
                capi.check(capi.lib.dfot_op_transpose_bf16(P(vf), P(vt), n, c, S()))
                capi.check(capi.lib.dfot_op_gemm_bf16(P(probs), n, P(vt), None, P(of), c, n, c, n, S()))
        ms_loop = med(loop)
        diff = ((o.float() - o2.float()).norm() / o2.float().norm()).item()
        flop = 4.0 * frames * n * n * c
        print(f"ivae attention {frames:3d} frames N={n} C={c}: fused {ms*1e3:8.1f} us ({flop / ms / 1e9:6.1f} TF/s)  per-frame loop of 4 launches "
              f"{ms_loop*1e3:9.1f} us  ({ms_loop / ms:.1f}x; rel-L2 between them {diff:.1e})", flush=True)
    for name, entry, (frames, h, w, ci, co), up in (("upsample-conv 512->512 16^2 -> 32^2", capi.lib.dfot_op_upconv3x3_f32, (16, 16, 16, 512, 512), True),
                                                    ("downsample 128->128 128^2 -> 64^2", capi.lib.dfot_op_conv3x3_s2_f32, (16, 128, 128, 128, 128), False)):
        x = torch.randn(frames, h, w, ci, device="cuda").bfloat16()
        wt = (torch.randn(co, 9 * ci, device="cuda") / math.sqrt(9 * ci)).bfloat16()
        ho, wo = (2 * h, 2 * w) if up else (h // 2, w // 2)
        out = torch.empty(frames, ho, wo, co, device="cuda")
        ms = med(lambda: capi.check(entry(P(x), P(wt), None, P(out), frames, h, w, ci, co, S())))
        print(f"ivae {name}, {frames} frames: {ms*1e3:8.1f} us  {2.0 * frames * ho * wo * co * 9 * ci / ms / 1e9:6.1f} TF/s", flush=True)
    cfg = dict(ch=128, out_ch=3, ch_mult=(1, 2, 4, 4), num_res_blocks=2, z_channels=4, embed_dim=4, resolution=128)
    dec, enc = dfot_amd.ImageVAEDecoder(**cfg).cuda(), dfot_amd.ImageVAEEncoder(**cfg).cuda()
    dec.init_random(0)
    enc.init_random(1)
    for r in (128, 256):    # the frame size is the caller's: the same modules run both
        z, y = torch.randn(16, 4, r // 8, r // 8, device="cuda"), torch.rand(16, 3, r, r, device="cuda") * 2 - 1
        print(f"ivae decode 16 frames 4x{r // 8}x{r // 8} -> 3x{r}x{r} (image_vae.yaml): {med(lambda: dec.decode(z)):.3f} ms", flush=True)
        print(f"ivae encode 16 frames 3x{r}x{r} -> moments (image_vae.yaml): {med(lambda: enc.encode(y)):.3f} ms", flush=True)


def dcae():
    """the DC-AE of the dmlab / Minecraft latents (csrc/dcae.hip): each new launch alone at the stock shapes of 16 frames, next to a
    device-to-device copy of the same number of bytes (the yardstick of the streaming kernels: what moving that traffic costs at all), and a
    whole encode / decode of 16 frames at both stock configurations.  No speed threshold: nothing of this had been measured before.  Each
    figure: the median of 7 repeats of (3 warm-up + 20 timed launches between two HIP events)."""
    import statistics
    med = lambda fn, **kw: statistics.median(timeit(fn, **kw) for _ in range(7))

    def copy_us(nbytes):
        a = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        b = torch.empty_like(a)
        return med(lambda: b.copy_(a)) * 1e3

    def line(name, us, nbytes):
        print(f"dcae {name}: {us:8.1f} us  ({nbytes / 1e6:7.2f} MB moved, {nbytes / us / 1e6:5.2f} TB/s; a device copy of as many bytes: "
              f"{copy_us(nbytes):6.1f} us)", flush=True)
    f = 16
    for n, c in ((64, 512), (256, 512), (64, 1024)):      # dmlab stage 3; Minecraft stage 3 and stage 4
        side, heads, m = int(n ** 0.5), c // 32, f * n
        qkv = torch.randn(m, 3 * c, device="cuda").bfloat16()
        o = torch.empty(m, c, dtype=torch.bfloat16, device="cuda")
        us = med(lambda: capi.check(capi.lib.dfot_op_dcae_linear_attention(P(qkv), 3 * c, P(o), c, f, n, heads, S()))) * 1e3
        line(f"linear_attention {f} frames N={n} C={c} ({f * heads} workgroups)", us, qkv.numel() * 2 + o.numel() * 2)
        t = torch.randn(f, side, side, 8 * c, device="cuda").bfloat16()
        wt, bias = torch.randn(9, 8 * c, device="cuda") / 3, torch.zeros(8 * c, device="cuda")
        gl = torch.empty(f, side, side, 4 * c, dtype=torch.bfloat16, device="cuda")
        us = med(lambda: capi.check(capi.lib.dfot_op_dcae_dw_glu(P(t), P(wt), P(bias), P(gl), f, side, side, 4 * c, S()))) * 1e3
        line(f"dw_glu {f} frames {side}x{side} 2h={8 * c}", us, t.numel() * 2 + gl.numel() * 2)
        x, r = torch.randn(m, c, device="cuda"), torch.randn(m, c, device="cuda")
        w1, b1 = torch.ones(c, device="cuda"), torch.zeros(c, device="cuda")
        o32, o16 = torch.empty_like(x), torch.empty(m, c, dtype=torch.bfloat16, device="cuda")
        us = med(lambda: capi.check(capi.lib.dfot_op_dcae_rmsnorm(P(x), P(w1), P(b1), 1e-5, P(r), P(o32), P(o16), 0, m, c, S()))) * 1e3
        line(f"rmsnorm + residual, fp32 and bf16 out, {m} rows of {c}", us, x.numel() * 14)
    for name, (h, cin, cout) in {"down 256 -> 512 at 32x32": (32, 256, 512), "down 512 -> 512 at 16x16": (16, 512, 512)}.items():
        conv, src = torch.randn(f, h, h, cout // 4, device="cuda"), torch.randn(f, h, h, cin, device="cuda")
        out = torch.empty(f, h // 2, h // 2, cout, device="cuda")
        us = med(lambda: capi.check(capi.lib.dfot_op_dcae_down_shortcut(P(conv), cout // 4, P(src), P(out), f, h, h, cin, cout, 2, S()))) * 1e3
        line(f"{name} (unshuffle + group mean {4 * cin // cout})", us, (conv.numel() + src.numel() + out.numel()) * 4)
    for name, (h, cin, cout) in {"up 512 -> 256 at 16x16": (16, 512, 256), "up 256 -> 128 at 32x32": (32, 256, 128)}.items():
        conv, src = torch.randn(f, h, h, 4 * cout, device="cuda"), torch.randn(f, h, h, cin, device="cuda")
        out = torch.empty(f, 2 * h, 2 * h, cout, device="cuda")
        us = med(lambda: capi.check(capi.lib.dfot_op_dcae_up_shortcut(P(conv), 4 * cout, P(src), cin, P(out), f, h, h, cin, cout, 2, S()))) * 1e3
        line(f"{name} (shuffle + repeat {4 * cout // cin})", us, (conv.numel() + src.numel() + out.numel()) * 4)
    t32 = torch.randn(f * 32 * 32, 256, device="cuda")
    tb = torch.empty(t32.shape, dtype=torch.bfloat16, device="cuda")
    us = med(lambda: capi.check(capi.lib.dfot_op_dcae_act_bf16(P(t32), P(tb), t32.numel(), 2, S()))) * 1e3
    line(f"act_bf16 (SiLU) {t32.shape[0]} rows of 256", us, t32.numel() * 6)
    for kind, size in (("8x", 64), ("16x", 128)):
        cfg = dfot_amd.dcae_config(kind)
        enc, dec = dfot_amd.DCAEEncoder(**cfg).cuda(), dfot_amd.DCAEDecoder(**cfg).cuda()
        enc.init_random(1)
        dec.init_random(0)
        y, z = torch.rand(f, 3, size, size, device="cuda") * 2 - 1, torch.randn(f, 32, 8, 8, device="cuda")
        ms_e, ms_d = med(lambda: enc.encode(y), iters=5, warm=1), med(lambda: dec.decode(z), iters=5, warm=1)
        print(f"dcae {kind} encode {f} frames 3x{size}x{size} -> 32x8x8: {ms_e:.3f} ms; decode 32x8x8 -> 3x{size}x{size}: {ms_d:.3f} ms", flush=True)


def titok():
    """the TiTok-KL decoder of the taichi recipes: the ragged attention launch alone at the production shape (16 frames of 289 tokens, the
    `large` preset's 16 heads) and a whole decode of 16 frames at 256 x 256 through the `large` decoder (and the `small` one).  Each figure:
    the median of 7 repeats of (3 warm-up + 20 timed launches between two HIP events)."""
    import statistics
    med = lambda fn, **kw: statistics.median(timeit(fn, **kw) for _ in range(7))
    for seqs, length, heads in ((16, 289, 16), (1, 289, 16), (16, 1057, 16)):
        rows = -(-seqs * length // 128) * 128
        qkv = torch.randn(rows, 3 * heads * 64, device="cuda").bfloat16()
        o = torch.zeros(rows, heads * 64, dtype=torch.bfloat16, device="cuda")
        ms = med(lambda: capi.check(capi.lib.dfot_op_mha_packed(P(qkv), 3 * heads * 64, P(o), seqs, length, heads, S())))
        flop = 4.0 * seqs * heads * length * length * 64
        print(f"titok mha_packed seqs {seqs:2d} len {length:4d} heads {heads}: {ms*1e3:8.1f} us ({flop / ms / 1e9:6.1f} TF/s)", flush=True)
    for size in ("large", "small"):
        dec = dfot_amd.TiTokDecoder(image_size=256, token_size=4, vit_dec_model_size=size).cuda()
        dec.init_random(0)
        z = torch.randn(16, 4, 1, 32, device="cuda")
        ms_t = med(lambda: dec.decode_pixel_input(z), iters=5, warm=1)
        ms = med(lambda: dec.decode(z), iters=5, warm=1)
        print(f"titok decode 16 frames 4x1x32 -> 3x256x256 ({size}): {ms:.3f} ms, of which the transformer up to the pixel decoder's input "
              f"{ms_t:.3f} ms", flush=True)


def titok_enc():
    """the TiTok-KL encoder of the taichi recipes: 16 frames at 256 x 256 through the `large` encoder (and the `small` one) -- the yardstick
    is the transformer share `titok` prints for the decoder, the same 24 blocks over the same 16 x 289 tokens -- and its three own launches
    alone at that shape.  Each figure: the median of 7 repeats of (warm-up + timed launches between two HIP events)."""
    import statistics
    med = lambda fn, **kw: statistics.median(timeit(fn, **kw) for _ in range(7))
    f, s, c, nlat, oc = 16, 256, 1024, 32, 8
    g2 = (s // 16) ** 2
    x = torch.rand(f, 3, s, s, device="cuda")
    rows = torch.zeros(f * g2, 768, dtype=torch.bfloat16, device="cuda")
    us = med(lambda: capi.check(capi.lib.dfot_op_titok_patch_rows(P(x), P(rows), f, s, S()))) * 1e3
    print(f"titok_enc patch_rows {f} frames {s}x{s} -> [{f * g2}][768] bf16: {us:8.1f} us ({(x.numel() * 4 + rows.numel() * 2) / us / 1e6:6.2f} TB/s)",
          flush=True)
    patches = torch.randn(f * g2, c, device="cuda")
    cls, pos, lat, lpos = (torch.randn(n, c, device="cuda") for n in (1, g2 + 1, nlat, nlat))
    gamma, beta = torch.ones(c, device="cuda"), torch.zeros(c, device="cuda")
    tok = torch.zeros(-(-f * (1 + g2 + nlat) // 128) * 128, c, device="cuda")
    us = med(lambda: capi.check(capi.lib.dfot_op_titok_enc_tokens(P(patches), c, P(cls), P(pos), P(lat), P(lpos), P(gamma), P(beta), 1e-5, P(tok), f, g2,
                                                                   nlat, c, S()))) * 1e3
    print(f"titok_enc enc_tokens {f} x {1 + g2 + nlat} rows of {c}: {us:8.1f} us ({(patches.numel() + f * (1 + g2 + nlat) * c) * 4 / us / 1e6:6.2f} TB/s)",
          flush=True)
    t, w, bias = torch.randn(f, nlat, c, device="cuda"), torch.randn(oc, c, device="cuda") / 32, torch.zeros(oc, device="cuda")
    mom = torch.empty(f, nlat, oc, device="cuda")
    us = med(lambda: capi.check(capi.lib.dfot_op_titok_moments(P(t), P(w), P(bias), P(mom), oc, f, nlat, c, oc, S()))) * 1e3
    print(f"titok_enc moments {f} frames [{nlat}][{c}] -> [{nlat}][{oc}]: {us:8.1f} us", flush=True)
    for size in ("large", "small"):
        enc = dfot_amd.TiTokEncoder(image_size=s, token_size=4, vit_enc_model_size=size).cuda()
        enc.init_random(0)
        ms = med(lambda: enc.encode_moments(x), iters=5, warm=1)
        ms_z = med(lambda: enc.encode(x, sample=True), iters=5, warm=1)
        print(f"titok_enc encode {f} frames 3x{s}x{s} -> moments 8x1x32 ({size}): {ms:.3f} ms; encode(x, sample=True) -> 4x1x32: {ms_z:.3f} ms", flush=True)


def main():
    what = sys.argv[1:] or ["gemm", "conv", "attn"]
    if "titok" in what:
        titok()
    if "titok_enc" in what:
        titok_enc()
    if "attnmap" in what:
        attnmap()
    if "mcraft" in what:
        mcraft()
    if "ivae" in what:
        ivae()
    if "dcae" in what:
        dcae()
    if "vae_encode" in what:
        vae_encode()
    variants = [int(x) for x in os.environ.get("VARIANTS", "1").split(",")]
    if "gemm" in what:
        for name, (m, n, k) in {"L2 qkv+mlp": (16384, 4032, 576), "L2 out": (16384, 576, 2880), "L3 qkv+mlp": (4096, 8064, 1152),
                                "L3 out": (4096, 1152, 5760), "film L0": (131072, 256, 1024), "pose": (131072, 1024, 768),
                                "square 4096": (4096, 4096, 4096), "DiT qkv B8": (10240, 3456, 1152), "DiT proj B8": (10240, 1152, 1152),
                                "DiT qkv B2": (2560, 3456, 1152), "DiT proj B2": (2560, 1152, 1152),
                                "MLP fc1 B8": (20480, 4608, 1152), "MLP fc2 B8": (20480, 1152, 4608)}.items():
            if os.environ.get("ONLY") and os.environ["ONLY"] not in name:
                continue
            for v in variants:
                ms, tf = gemm(m, n, k, v)
                print(f"gemm {name:12s} M={m:6d} N={n:5d} K={k:5d} variant={v}: {ms*1e3:8.1f} us  {tf:7.1f} TF/s", flush=True)
            if os.environ.get("HIPBLASLT"):  # vendor library on the same shape, for orientation only (never on the product path)
                a = torch.randn(m, k, device="cuda").bfloat16()
                w = torch.randn(n, k, device="cuda").bfloat16()
                ms = timeit(lambda: torch.nn.functional.linear(a, w))
                print(f"gemm {name:12s} M={m:6d} N={n:5d} K={k:5d} torch/hipBLASLt: {ms*1e3:8.1f} us  {2.0*m*n*k/ms/1e9:7.1f} TF/s", flush=True)
    if "uvit3d" in what:
        free, pose = uvit3d_forward(2)
        print(f"uvit3d forward 256x256 Bm=2 T=8: UViT3D {free:.2f} ms, UViT3DPose.forward_cached {pose:.2f} ms, ratio {free / pose:.3f}")
    if "gnfilm_frame" in what:
        for lvl, name, c, rows, us_frame, us_row in gnfilm_frame():
            print(f"gnfilm_frame L{lvl} {name:13s} C={c:4d} rows={rows:7d} (64 frames): per-frame {us_frame:8.1f} us  per-row {us_row:8.1f} us  "
                  f"ratio {us_frame / us_row:.3f}", flush=True)
    if "uvit3d_train" in what:
        for b in (8, 4, 2, 1):  # the largest of these batches that fits
            try:
                ms, gib, row = uvit3d_train(b)
            except (torch.cuda.OutOfMemoryError, capi.DfotError) as err:
                print(f"uvit3d_train B={b}: does not fit ({type(err).__name__})", flush=True)
                torch.cuda.empty_cache()
                continue
            print(f"uvit3d_train full widths B={b} T=8 256x256, {'per-row' if row else 'per-frame'} FiLM: {ms:.2f} ms per training step, peak memory "
                  f"{gib:.2f} GiB", flush=True)
            break
    if "dit_front" in what:
        xl = dict(name="dit3d", variant="full", pos_emb_type="rope_3d", patch_size=1, hidden_size=1152, depth=28, num_heads=16)
        dit_front("XL K600", xl, dfot_amd.DiT3D, (16, 16, 16), 5, 8, 5)  # @DiT/XL at the K600 latents: B = 8, T = 5, P = 256
        b = dict(name="dit3d", variant="full", pos_emb_type="rope_3d", patch_size=2, hidden_size=768, depth=12, num_heads=12)
        # @DiT/B width, 16 tokens x 16 patches, B = 16.  8 latent channels (a final weight that stays in LDS; `mcraft` measures the recipe's own
        # 32 channels, whose 393 KB weight takes the chunked final layer); the front end does not depend on the channel count
        dit_front("DiT/B", b, dfot_amd.DiT3D, (8, 8, 8), 16, 16, 16)
    if "conv" in what:
        for name, (bt, h, w, ci, co) in {"L0 res": (16, 128, 128, 128, 128), "L1 res": (16, 64, 64, 256, 256),
                                         "down0": (16, 64, 64, 128, 256), "down1": (16, 32, 32, 256, 576),
                                         "down2": (16, 16, 16, 576, 1152), "up2": (16, 16, 16, 1152, 576),
                                         "up1": (16, 32, 32, 576, 256), "up0": (16, 64, 64, 256, 128)}.items():
            for v in variants:
                ms, tf = conv(bt, h, w, ci, co, v)
                print(f"conv {name:8s} {bt}x{h}x{w} {ci}->{co} variant={v}: {ms*1e3:8.1f} us  {tf:7.1f} TF/s", flush=True)
    if "tattn" in what:
        for name, (b, hd, t, pn, d) in {"XL B2": (2, 16, 16, 256, 72), "XL B16": (16, 16, 16, 256, 72), "S B2": (2, 6, 16, 256, 64),
                                        "S B16": (16, 6, 16, 256, 64)}.items():
            ms, gbs, tf = tattn(b, hd, t, pn, d)
            print(f"tattn {name:6s} B={b} H={hd} T={t} P={pn} d={d}: {ms*1e3:8.1f} us  {gbs:7.1f} GB/s ({gbs / 1e3 / HBM_TBS:.2f} of {HBM_TBS:.0f} TB/s HBM)  "
                  f"{tf:6.2f} TF/s", flush=True)
        for b in (2, 16):
            print(f"facdit XL forward B={b} x 16 frames x 256 patches: {facdit_forward(b):.3f} ms", flush=True)
    if "sattn64" in what:
        # @FacMatDiT/S spatial blocks (384 / 12 heads = d 32) and @FacDiT/S (6 heads, d 64); 2 and 16 videos x 16 frames x 64 patches
        for name, (hd, d) in {"FacMat-S": (12, 32), "FacDiT-S": (6, 64)}.items():
            for b in (2, 16):
                ms, gbs, ms128 = sattn64(b, hd, 16, d)
                print(f"sattn64 {name:8s} B={b:2d} x 16 frames H={hd} d={d}: seq64 {ms*1e3:8.1f} us  {gbs:7.1f} GB/s ({gbs / 1e3 / HBM_TBS:.2f} of "
                      f"{HBM_TBS:.0f} TB/s HBM)  padded n=128 at equal rows {ms128*1e3:8.1f} us  seq64 / padded {ms / ms128:.2f}", flush=True)
        for kind, label in (("facdit", "FacDiT-S"), ("facmat", "FacMatDiT-S-64-1")):
            print(f"{label} forward (depth 6) B=2 x 16 frames x 64 patches: {p64_forward(kind, 2):.3f} ms", flush=True)
    if "attn_fc" in what:
        med = lambda r: sorted(r)[len(r) // 2]  # noqa: E731
        # the stock DiT1D attention (1152 / 16 heads = d 72, L = 32) at 16 and 32 frames, model batch 16
        for n in (512, 1024):
            fc, pad = attn_fc(16, 16, n, 32, 72)
            tiles = n // 128
            print(f"attn_fc B=16 H=16 N={n} L=32 d=72: frame-causal median {med(fc)*1e3:8.1f} us (min {min(fc)*1e3:.1f}, max {max(fc)*1e3:.1f})  "
                  f"padded {med(pad)*1e3:8.1f} us (min {min(pad)*1e3:.1f}, max {max(pad)*1e3:.1f})  frame-causal / padded {med(fc) / med(pad):.2f}  "
                  f"({tiles * (tiles + 1) // 2} of {tiles * tiles} (query tile, 128-key block) pairs visited; {len(fc)} alternated rounds)", flush=True)
    if "attn_fc_bwd" in what:
        med = lambda r: sorted(r)[len(r) // 2]  # noqa: E731
        # the backward at the attn_fc shapes; the condition of DESIGN.md section 4e: the frame-causal median is not above the non-causal
        # median by more than the non-causal min-to-max spread of the same run
        for n in (512, 1024):
            fc, nc = attn_fc_bwd(16, 16, n, 32, 72)
            tiles = n // 64
            print(f"attn_fc_bwd B=16 H=16 N={n} L=32 d=72: frame-causal median {med(fc)*1e3:8.1f} us (min {min(fc)*1e3:.1f}, max {max(fc)*1e3:.1f})  "
                  f"non-causal {med(nc)*1e3:8.1f} us (min {min(nc)*1e3:.1f}, max {max(nc)*1e3:.1f})  frame-causal / non-causal "
                  f"{med(fc) / med(nc):.2f}  ({tiles * (tiles + 2) // 4} of {tiles * tiles // 2} (128-row block, 64-row tile) pairs streamed per "
                  f"kernel; {len(fc)} alternated rounds)", flush=True)
    if "seq64_bwd" in what:
        med = lambda r: sorted(r)[len(r) // 2]  # noqa: E731
        # @FacDiT/S at res-128 (6 heads, d 64), 16 videos x 16 frames = 256 sequences of 64 patches; d 72 and d 128 at the same sequence count
        for d in (64, 72, 128):
            bwd, fwd, cp, nbytes = seq64_bwd(256, 6, d)
            print(f"seq64_bwd 256 sequences H=6 d={d}: backward median {med(bwd)*1e3:7.1f} us (min {min(bwd)*1e3:.1f})  forward {med(fwd)*1e3:7.1f} us "
                  f"(min {min(fwd)*1e3:.1f})  copy of {nbytes / 1e6:.1f} MB moved {med(cp)*1e3:7.1f} us (min {min(cp)*1e3:.1f})  backward / forward "
                  f"{med(bwd) / med(fwd):.2f}  backward / copy {med(bwd) / med(cp):.2f}  ({len(bwd)} alternated rounds)", flush=True)
    if "seq64_bwd_packed" in what:
        med = lambda r: sorted(r)[len(r) // 2]  # noqa: E731
        # the shapes of seq64_bwd: @FacDiT/S at res-128 (16 videos x 16 frames, 6 heads, d 64), then d 72 and d 128
        for d in (64, 72, 128):
            pk, pr, cp, nbytes = seq64_bwd_packed(256, 6, d)
            print(f"seq64_bwd_packed 256 sequences H=6 d={d}: packed median {med(pk)*1e3:7.1f} us (min {min(pk)*1e3:.1f}, max {max(pk)*1e3:.1f})  "
                  f"pair (backward + qkv_grad_pack) {med(pr)*1e3:7.1f} us (min {min(pr)*1e3:.1f}, max {max(pr)*1e3:.1f})  copy of {nbytes / 1e6:.1f} MB "
                  f"moved {med(cp)*1e3:7.1f} us (min {min(cp)*1e3:.1f}, max {max(cp)*1e3:.1f})  packed / pair {med(pk) / med(pr):.2f}  packed / copy "
                  f"{med(pk) / med(cp):.2f}  ({len(pk)} alternated rounds, equal bits)", flush=True)
    if "facdit_s128_train" in what:
        med = lambda r: sorted(r)[len(r) // 2]  # noqa: E731
        for mlp in (False, True):
            pk, pr = facdit_s128_train(16, mlp)
            print(f"facdit_s128_train FacDiT-S{'-mlp' if mlp else ''} B=16 x 16 frames x 64 patches (hidden 384, depth 6): step with the packed "
                  f"spatial backward median {med(pk):.3f} ms (min {min(pk):.3f}, max {max(pk):.3f})  with the pair {med(pr):.3f} ms (min {min(pr):.3f}, "
                  f"max {max(pr):.3f})  packed / pair {med(pk) / med(pr):.3f}  ({len(pk)} alternated rounds)", flush=True)
    factor_us = {}  # E -> us of the two left-factor gradients of one matrix block at the S shape (filled by facmat_factor_wgrad)
    if "facmat_factor_wgrad" in what:
        med = lambda r: sorted(r)[len(r) // 2]  # noqa: E731
        # @FacMatDiT/group_S at res-128: 16 videos x 16 frames = 256 frames, embed_row_dim 384, 64 patches; dU' is (E, P), dU is (P, E)
        for e in (64, 128):
            for name, (ra, rb) in (("dU' (E, P)", (e, 64)), ("dU  (P, E)", (64, e))):
                op, cp, nbytes = facmat_factor_wgrad(256, ra, rb, 384)
                factor_us[e] = factor_us.get(e, 0.0) + med(op) * 1e3
                print(f"facmat_factor_wgrad 256 frames hd=384 E={e} {name} {ra} x {rb}: launch + slice sum median {med(op)*1e3:7.1f} us (min "
                      f"{min(op)*1e3:.1f}, max {max(op)*1e3:.1f})  copy reading the same {nbytes / 1e6:.1f} MB {med(cp)*1e3:7.1f} us (min "
                      f"{min(cp)*1e3:.1f}, max {max(cp)*1e3:.1f})  op / copy {med(op) / med(cp):.2f}  {nbytes / med(op) / 1e9:.2f} TB/s read  "
                      f"({len(op)} alternated rounds)", flush=True)
    if "facmat_s128_train" in what:
        med = lambda r: sorted(r)[len(r) // 2]  # noqa: E731
        for e in (64, 128):
            ms = facmat_s128_train(16, e)
            share = f"  the two left-factor gradients x 6 blocks = {6 * factor_us[e] / 1e3:.3f} ms = {6 * factor_us[e] / 1e3 / med(ms):.1%} of the step" \
                if e in factor_us else "  (run facmat_factor_wgrad in the same call for the factor gradients' share)"
            print(f"facmat_s128_train FacMatDiT-S-{e}-1-bias B=16 x 16 frames x 64 patches (embed_row_dim 384, depth 6): step median {med(ms):.3f} ms "
                  f"(min {min(ms):.3f}, max {max(ms):.3f}; {len(ms)} rounds){share}", flush=True)
    if "dit1d" in what:
        ms = dit1d_forward(16)
        for name, r in ms.items():
            r = sorted(r)
            print(f"{name} forward B=16 x 16 frames x 32 tokens (hidden 1152, depth 28): median {r[len(r) // 2]:.3f} ms  (min {r[0]:.3f}, max {r[-1]:.3f} "
                  f"over {len(r)} alternated rounds)", flush=True)
    if "dit1d_train" in what:
        for name, (r, nbytes) in dit1d_train_ops().items():
            r = sorted(r)
            med = r[len(r) // 2]
            print(f"dit1d_train {name} rows 4096 x hidden 1152: median {med*1e3:7.1f} us (min {r[0]*1e3:.1f}, max {r[-1]*1e3:.1f} over {len(r)} alternated "
                  f"rounds)  {nbytes / 1e6:.1f} MB  {nbytes / med / 1e6:7.1f} GB/s ({nbytes / med / 1e9 / HBM_TBS:.2f} of {HBM_TBS:.0f} TB/s HBM)", flush=True)
        for b in (8, 4, 2):  # the largest of these batches that fits
            try:
                ms = dit1d_train(b)
            except (torch.cuda.OutOfMemoryError, capi.DfotError) as err:
                print(f"dit1d_train XL B={b}: does not fit ({type(err).__name__})", flush=True)
                torch.cuda.empty_cache()
                continue
            print(f"dit1d_train stock widths B={b} x 16 frames x 32 tokens: {ms:.2f} ms per training step", flush=True)
            break
    if "facmat_narrow" in what:
        # the S shape (embed_row_dim 384, 64 patches, 16 videos x 16 frames) and an XL-like one (1152, 256 patches, 128 frames)
        for name, (frames, p, h) in {"S": (256, 64, 384), "XL": (128, 256, 1152)}.items():
            for e in (1, 8, 32):
                tc, tx, tcopy, nbytes = facmat_narrow_ops(frames, p, h, e)
                gb = lambda t: nbytes / t / 1e6  # noqa: E731
                print(f"facmat_narrow {name:2s} frames={frames} P={p} h={h} E={e:2d}: {nbytes / 1e6:7.2f} MB  contract {tc*1e3:7.1f} us {gb(tc):7.1f} GB/s  "
                      f"expand {tx*1e3:7.1f} us {gb(tx):7.1f} GB/s  device copy of the same bytes {tcopy*1e3:7.1f} us {gb(tcopy):7.1f} GB/s  "
                      f"(contract {tcopy / tc:.2f}, expand {tcopy / tx:.2f} of the copy's rate)", flush=True)
        widths = [(64, 1), (1, 1), (8, 1), (32, 4)]
        ms = facmat_narrow_forward(widths, 16)
        for e, cc in widths:
            r = sorted(ms[(e, cc)])
            print(f"FacMatDiT-S-{e}-{cc} forward (depth 6) B=16 x 16 frames x 64 patches: median {r[len(r) // 2]:.3f} ms  (min {r[0]:.3f}, max {r[-1]:.3f} over "
                  f"{len(r)} alternated rounds)", flush=True)
    if "tattn_bwd" in what:
        for name, (b, hd, t, pn, d) in {"XL B2": (2, 16, 16, 256, 72), "XL B16": (16, 16, 16, 256, 72), "S B2": (2, 6, 16, 256, 64),
                                        "S B16": (16, 6, 16, 256, 64)}.items():
            ms_bwd, ms_fwd, nbytes = tattn_bwd(b, hd, t, pn, d)
            gbs = nbytes / ms_bwd / 1e6
            print(f"tattn_bwd {name:6s} B={b} H={hd} T={t} P={pn} d={d}: backward {ms_bwd*1e3:8.1f} us  {gbs:7.1f} GB/s ({gbs / 1e3 / HBM_TBS:.2f} of "
                  f"{HBM_TBS:.0f} TB/s HBM)  forward {ms_fwd*1e3:8.1f} us  backward / forward {ms_bwd / ms_fwd:.2f}", flush=True)
    if "facdit_train" in what:
        depth = 28
        for b in (2, 8):
            try:
                ms = facdit_train(b, depth=depth)
            except (torch.cuda.OutOfMemoryError, capi.DfotError) as err:
                print(f"facdit_train XL B={b}: does not fit ({type(err).__name__})", flush=True)
                torch.cuda.empty_cache()
                continue
            ms_attn = tattn_bwd(b, 16, 16, 256, 72)[0]
            print(f"facdit_train XL B={b} x 16 frames x 256 patches: {ms:.2f} ms per training step; temporal attention backward {depth} x "
                  f"{ms_attn*1e3:.1f} us = {depth * ms_attn / ms * 100:.1f} % of it", flush=True)
            torch.cuda.empty_cache()
    if "mattn" in what:
        # @FacMatDiT/S-64-1 (embed_row_dim 384, 6 row heads) and XL-64-1 (1152, 16); embed_col_dim 64, one col head
        for name, (h, rr) in {"S": (384, 6), "XL": (1152, 16)}.items():
            for b in (2, 16):
                for tokens in (16, 17, 32):
                    ms_rope, ms_plain, ms_old, nbytes = mattn(b, tokens, 64, h, 1, rr, True)
                    print(f"mattn {name:2s} B={b:2d} L={tokens} E=64 h={h} rr={rr}: rope {ms_rope*1e3:8.1f} us ({nbytes / ms_rope / 1e6:6.1f} GB/s)  "
                          f"no table {ms_plain*1e3:8.1f} us  variant-1 launcher {ms_old*1e3:8.1f} us  ({ms_old / ms_plain:.1f}x)", flush=True)
        depth = 28
        ms = facmat_forward(2, depth=depth)
        ms_attn = mattn(2, 16, 64, 1152, 1, 16, True)[0]
        print(f"facmat XL forward B=2 x 16 frames x 256 patches: {ms:.3f} ms; matrix attention {depth} x {ms_attn*1e3:.1f} us = "
              f"{depth * ms_attn / ms * 100:.1f} % of it", flush=True)
    if "mattn_bwd" in what:
        for name, (h, rr) in {"S": (384, 6), "XL": (1152, 16)}.items():
            for b in (2, 8, 16):
                for tokens in (16, 17, 32):
                    ms_rope, ms_plain, ms_fwd, nbytes = mattn_bwd(b, tokens, 64, h, 1, rr)
                    gbs = nbytes / ms_rope / 1e6
                    print(f"mattn_bwd {name:2s} B={b:2d} L={tokens} E=64 h={h} rr={rr} ({b * rr:3d} workgroups): rope {ms_rope*1e3:8.1f} us ({gbs:6.1f} GB/s, "
                          f"{gbs / 1e3 / HBM_TBS:.3f} of {HBM_TBS:.0f} TB/s HBM)  no table {ms_plain*1e3:8.1f} us  forward {ms_fwd*1e3:8.1f} us", flush=True)
    if "facmat_train" in what:
        depth = 28
        for b in (8, 4, 2, 1):  # the largest of these batches that fits
            try:
                ms = facmat_train(b, depth=depth)
            except (torch.cuda.OutOfMemoryError, capi.DfotError) as err:
                print(f"facmat_train XL B={b}: does not fit ({type(err).__name__})", flush=True)
                torch.cuda.empty_cache()
                continue
            ms_attn = mattn_bwd(b, 16, 64, 1152, 1, 16)[0]
            print(f"facmat_train XL-64-1 B={b} x 16 frames x 256 patches: {ms:.2f} ms per training step; matrix attention backward {depth} x "
                  f"{ms_attn*1e3:.1f} us = {depth * ms_attn / ms * 100:.1f} % of it", flush=True)
            break
    if "equal" in what:
        # the conditioning of one window at model batch 2 and 8 (B, 8, 180, 256, 256 fp32), and a size that stays in the 256 MiB Infinity Cache
        for name, nbytes in {"cond Bm2": 2 * 8 * 180 * 256 * 256 * 4, "cond Bm8": 8 * 8 * 180 * 256 * 256 * 4, "64 MiB": 64 << 20}.items():
            ms, gbs = equal(nbytes)
            print(f"equal {name:8s} {nbytes / 1e6:8.1f} MB x 2: {ms*1e3:8.1f} us  {gbs:7.1f} GB/s ({gbs / 1e3 / HBM_TBS:.2f} of {HBM_TBS:.0f} TB/s HBM)", flush=True)
    if "attn" in what:
        shapes = {"L2": (2, 9, 8192, 64), "L3": (2, 9, 2048, 128), "L2 Bm8": (8, 9, 8192, 64)}
        if os.environ.get("ATTN_SHAPE"):  # e.g. ATTN_SHAPE=2,8,2048,128: one extra shape (workgroup-count experiments)
            shapes = {"custom": tuple(int(x) for x in os.environ["ATTN_SHAPE"].split(","))}
        for name, (b, hd, n, d) in shapes.items():
            if os.environ.get("ONLY") and os.environ["ONLY"] != name:
                continue
            if os.environ.get("ONLY") and os.environ["ONLY"] != name:
                continue
            for v in [int(x) for x in os.environ.get("ATTN_VARIANTS", "0").split(",")]:
                ms, tf = attn(b, hd, n, d, v)
                print(f"attn {name:7s} B={b} H={hd} N={n} d={d} variant={v}: {ms*1e3:8.1f} us  {tf:7.1f} TF/s", flush=True)


if __name__ == "__main__":
    main()
