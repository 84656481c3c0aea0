"""GPU parity of the training path (backward kernels, trainer) against torch autograd through the fp32 oracle restatement.
Tolerances: bf16 operands / fp32 accumulation, relative L2 of each gradient tensor."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


@pytest.mark.parametrize("d,heads,n,batch", [(72, 4, 640, 2), (32, 4, 256, 1), (64, 2, 384, 2), (128, 1, 256, 1), (96, 2, 256, 1), (120, 1, 128, 2), (48, 3, 128, 1)])
def test_attention_backward(d, heads, n, batch):
    """dq / dk / dv of softmax(q k^T / sqrt d) v for an upstream gradient d_o, vs autograd in fp32 on the bf16-rounded operands"""
    from dfot_amd import capi
    g = torch.Generator().manual_seed(d + n)
    q, k, v = (torch.randn(batch, heads, n, d, generator=g) for _ in range(3))
    do = torch.randn(batch, n, heads * d, generator=g)
    ds = 64 if d <= 64 else 128
    scale = math.log2(math.e) / math.sqrt(d)
    bf = lambda t: t.to(torch.bfloat16)

    def pad(t):
        out = torch.zeros(batch, heads, n, ds, dtype=torch.bfloat16, device="cuda")
        out[..., :d] = t.cuda()
        return out
    qs = bf(q * scale)  # what the forward consumes; the oracle uses exactly this q (unscaled back in fp32)
    qd, kd, vd = pad(qs), pad(bf(k)), pad(bf(v))
    dod = bf(do).cuda().contiguous()
    o = torch.empty(batch, n, heads * d, dtype=torch.bfloat16, device="cuda")
    dq, dk, dv = (torch.full((batch, heads, n, ds), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(3))
    capi.check(capi.lib.dfot_op_attention_bwd(capi.ptr(qd), capi.ptr(kd), capi.ptr(vd), capi.ptr(dod), capi.ptr(o), heads * d,
                                              capi.ptr(dq), capi.ptr(dk), capi.ptr(dv), batch, heads, n, d, capi.stream_ptr()))
    torch.cuda.synchronize()
    qr = (qs.float() / scale).requires_grad_()
    kr, vr = bf(k).float().requires_grad_(), bf(v).float().requires_grad_()
    ref = torch.softmax(qr @ kr.transpose(-1, -2) / math.sqrt(d), -1) @ vr
    ref = ref.transpose(1, 2).reshape(batch, n, heads * d)
    ref.backward(bf(do).float())
    assert rel(o.float().cpu(), ref.detach()) < 1.5e-2
    for name, got, want in (("dq", dq, qr.grad), ("dk", dk, kr.grad), ("dv", dv, vr.grad)):
        got = got.float().cpu()
        assert torch.isfinite(got).all(), name
        assert (got[..., d:] == 0).all(), name  # pad columns stay zero
        r = rel(got[..., :d], want)
        print(f"attention_bwd d={d} {name}: rel {r:.2e}")
        assert r < 2e-2, (name, r)


@pytest.mark.parametrize("mode", [0, 2])
def test_attention_backward_both_staging_forms(mode):
    """the backward kernels exist register-staged and LDS-DMA-staged for every head-dim instance; the default mixes them (DMA for the
    128-element rows).  DFOT_ATTN_BWD_DMA = 0 / 2 forces one form everywhere: the whole test_attention_backward matrix in a child"""
    import subprocess, sys
    if os.environ.get("DFOT_ATTN_BWD_DMA") is not None:
        pytest.skip("already inside the forced-mode child")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", "test_attention_backward and not both_staging"],
                       env=dict(os.environ, DFOT_ATTN_BWD_DMA=str(mode)), capture_output=True, text=True, timeout=600)
    print(r.stdout[-600:], r.stderr[-1500:] if r.returncode else "")
    assert r.returncode == 0


def _tiny_trainer(depth=2, hidden=128, heads=4, seed=3, res=(16, 8), chans=4, tokens=5, patch=1, mlp_ratio=None):
    import dfot_amd
    from oracle import dit as odit
    ocfg = odit.DiTConfig(hidden_size=hidden, depth=depth, num_heads=heads, patch_size=patch, in_channels=chans, resolution=res, max_tokens=tokens,
                          spatial_mlp_ratio=mlp_ratio)
    params = odit.seeded_params(ocfg, seed)
    tr = dfot_amd.DiT3DTrainer(dict(variant="full", pos_emb_type="rope_3d", patch_size=patch, hidden_size=hidden, depth=depth, num_heads=heads,
                                    spatial_mlp_ratio=mlp_ratio), x_shape=(chans, *res), max_tokens=tokens)
    tr.load_state_dict(params, strict=True)
    return ocfg, params, tr


@pytest.mark.parametrize("hidden,heads,depth,mlp,patch,res", [(128, 4, 2, None, 1, (16, 8)), (256, 4, 1, None, 1, (16, 8)),
                                                              (256, 4, 2, 4.0, 2, (32, 16)), (128, 2, 1, 2.0, 1, (16, 8))])
def test_dit_backward_matches_autograd(hidden, heads, depth, mlp, patch, res):
    """every parameter gradient of sum(out * d_out) vs torch autograd through the fp32 oracle restatement of DiT3D.forward
    (attention-only blocks as README @DiT/XL, and blocks with the MLP branch of spatial_mlp_ratio, patch 2)"""
    from oracle import dit as odit
    ocfg, params, tr = _tiny_trainer(depth=depth, hidden=hidden, heads=heads, mlp_ratio=mlp, patch=patch, res=res)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 5, 4, *res, generator=g)
    k = torch.randint(0, 1000, (2, 5), generator=g)
    d_out = torch.randn(2, 5, 4, *res, generator=g)
    out = tr.forward(x, k).cpu()
    tr.backward(d_out)
    grads = {n: t.cpu() for n, t in tr.grad_dict().items()}
    ps = {n: t.clone().requires_grad_() for n, t in params.items()}
    ref = odit.forward(ps, ocfg, x, k)
    assert rel(out, ref.detach()) < 2e-2
    (ref * d_out).sum().backward()
    worst = 0.0
    for n, t in ps.items():
        r = rel(grads[n], t.grad)
        worst = max(worst, r)
        assert torch.isfinite(grads[n]).all(), n
        assert r < 5e-2, (n, r)
    print(f"DiT3D backward hidden={hidden}: worst gradient rel-L2 {worst:.2e}")


def test_dit_drop_in_backbone_is_trainable_through_autograd():
    """VERDICT r1 #6 for the Kinetics-600 backbone: `dfot_amd.DiT3D(...)` called with gradients enabled dispatches
    `dfot::dit3d_forward_train`; `loss.backward()` fills `param.grad` with the hand-written backward's result (equal to
    DiT3DTrainer.backward on the same weights, within tolerance of autograd through the oracle), a second backward gives the same
    gradients (nothing accumulates inside the engine), and under no_grad the module still runs the fused inference engine."""
    import dfot_amd
    from oracle import dit as odit
    ocfg, params, tr = _tiny_trainer(depth=2, hidden=128, heads=4)
    model = dfot_amd.DiT3D(dict(variant="full", pos_emb_type="rope_3d", patch_size=1, hidden_size=128, depth=2, num_heads=4, spatial_mlp_ratio=None),
                           x_shape=(4, 16, 8), max_tokens=5).cuda()
    model.load_state_dict(params, strict=True)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 5, 4, 16, 8, generator=g).cuda()
    k = torch.randint(0, 1000, (2, 5), generator=g).cuda()
    w = torch.randn(2, 5, 4, 16, 8, generator=g).cuda()
    v = model(x, k)
    assert v.requires_grad
    (v * w).sum().backward()
    named = dict(model.named_parameters())
    first = {n: p.grad.clone() for n, p in named.items()}
    out = tr.forward(x, k)
    assert torch.equal(out, v.detach())
    tr.backward(w)
    tg = tr.grad_dict()
    assert sorted(tg) == sorted(named)
    for n, p in named.items():
        assert rel(p.grad, tg[n]) < 2e-2, (n, rel(p.grad, tg[n]))
    ps = {n: t.clone().requires_grad_() for n, t in params.items()}
    ref = odit.forward(ps, ocfg, x.cpu(), k.cpu())
    (ref * w.cpu()).sum().backward()
    rs = {n: rel(p.grad.cpu(), ps[n].grad) for n, p in named.items()}
    worst = max(rs, key=rs.get)
    print(f"DiT3D drop-in autograd: forward rel-L2 {rel(v.detach().cpu(), ref.detach()):.2e}; worst gradient rel-L2 {rs[worst]:.2e} at {worst}")
    assert rs[worst] < 5e-2
    model.zero_grad()
    (model(x, k) * w).sum().backward()
    for n, p in named.items():
        assert rel(p.grad, first[n]) < 2e-2, n
    with torch.no_grad():
        before = model(x, k)
    assert not before.requires_grad and rel(before.cpu(), ref.detach()) < 2e-2
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    opt.step()
    with torch.no_grad():
        after = model(x, k)
    assert rel(after, before) > 1e-4   # the inference engine picked the updated weights up
    v2 = model(x, k)                  # ... and so does the training engine
    assert rel(v2.detach(), after) < 2e-2


def test_dit_training_step_matches_torch_adamw():
    """loss, clipped AdamW update of every parameter after one step vs torch (autograd + clip_grad_norm_ + torch.optim.AdamW)"""
    from oracle import dit as odit, sampler as osm, schedule as sch
    ocfg, params, tr = _tiny_trainer(depth=2)
    tr.lr, tr.weight_decay, tr.max_grad_norm = 1e-3, 0.01, 1.0
    tr.loss_weighting = dict(strategy="fused_min_snr", cum_snr_decay=0.9)
    g = torch.Generator().manual_seed(4)
    xs = torch.randn(2, 5, 4, 16, 8, generator=g)
    k = torch.randint(0, 1000, (2, 5), generator=g)
    noise = torch.randn(2, 5, 4, 16, 8, generator=g)
    masks = torch.ones(2, 5)
    masks[1, 0] = 0
    loss = float(tr.training_step(xs, k, noise, masks).item())
    new = {n: t.cpu() for n, t in tr.state_dict().items()}
    # torch reference
    ps = {n: t.clone().requires_grad_() for n, t in params.items()}
    tables = sch.build_tables(beta_schedule="cosine")
    model = lambda x, lv, c, m: odit.forward(ps, ocfg, x, lv)
    _, per_tok = osm.discrete_training_loss(model, tables, xs, k, noise, strategy="fused_min_snr", cum_snr_decay=0.9)
    ref_loss = (per_tok * masks[..., None, None, None]).mean()
    ref_loss.backward()
    plist = list(ps.values())
    torch.nn.utils.clip_grad_norm_(plist, 1.0)
    opt = torch.optim.AdamW(plist, lr=1e-3, weight_decay=0.01, betas=(0.9, 0.99), eps=1e-8)
    opt.step()
    assert abs(loss - ref_loss.item()) < 2e-2 * abs(ref_loss.item()), (loss, ref_loss.item())
    checked = 0
    for n, t in ps.items():
        # the first Adam step moves a weight by ~ lr * g / (|g| + eps): compare the UPDATE where the (clipped) gradient is not
        # negligible -- where it is ~0 (e.g. the key bias, whose exact gradient vanishes) the step is the sign of rounding noise
        upd, ref_upd = new[n] - params[n], t.detach() - params[n]
        big = t.grad.abs() > 1e-2 * t.grad.abs().max()
        if big.any():
            r = rel(upd[big], ref_upd[big])
            assert r < 5e-2, (n, r)
            checked += int(big.sum())
    assert checked > 1000


def _ddp_worker(rank, world, port, q):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)  # one GPU on the test box: gloo carries the CUDA gradient buffer
    try:
        ocfg, params, tr = _tiny_trainer(depth=2)
        tr.lr, tr.max_grad_norm = 1e-3, 1.0
        g = torch.Generator().manual_seed(4)
        xs = torch.randn(4, 5, 4, 16, 8, generator=g)
        k = torch.randint(0, 1000, (4, 5), generator=g)
        noise = torch.randn(4, 5, 4, 16, 8, generator=g)
        sl = slice(2 * rank, 2 * rank + 2)
        loss = tr.training_step(xs[sl], k[sl], noise[sl], None, world_size=world)
        q.put((rank, float(loss.item()), tr.grads.cpu().numpy(), tr.params.cpu().numpy()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_data_parallel_step_equals_single_process_step():
    """two ranks with half the batch each (flat-gradient all-reduce, mean) take the same optimizer step as one process with the
    whole batch: averaged gradients and updated parameters agree"""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=480) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(60)
    ocfg, params, tr = _tiny_trainer(depth=2)
    tr.lr, tr.max_grad_norm = 1e-3, 1.0
    g = torch.Generator().manual_seed(4)
    xs = torch.randn(4, 5, 4, 16, 8, generator=g)
    k = torch.randint(0, 1000, (4, 5), generator=g)
    noise = torch.randn(4, 5, 4, 16, 8, generator=g)
    loss = float(tr.training_step(xs, k, noise, None).item())
    grads, new = tr.grads.cpu().numpy(), tr.params.cpu().numpy()
    assert np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])  # replicas stay identical
    assert abs(0.5 * (res[0][1] + res[1][1]) - loss) < 1e-3 * abs(loss)
    gr = np.linalg.norm(res[0][2] - grads) / np.linalg.norm(grads)
    print(f"data-parallel vs single-process gradient rel-L2 {gr:.2e}")
    assert gr < 2e-2  # bf16 GEMMs over different row groupings
    big = np.abs(grads) > 1e-2 * np.abs(grads).max()
    upd, ref = res[0][3] - tr_initial(params, tr), new - tr_initial(params, tr)
    assert np.linalg.norm(upd[big] - ref[big]) / np.linalg.norm(ref[big]) < 5e-2


def tr_initial(params, tr):
    flat = np.zeros(tr.numel, np.float32)
    for name, (off, shape) in tr.layout.items():
        flat[off: off + int(np.prod(shape))] = params[name].numpy().ravel()
    return flat


@pytest.mark.parametrize("name", ["tiny", "tiny2"])
def test_difference_dit_backward_matches_autograd(name):
    """DifferenceDiT3D (factorized matrix attention): every parameter gradient vs autograd through the fp32 oracle restatement --
    per-frame spatial blocks + MatrixDiTBlock (left / right factors, 2-D biases, attention over the frames), diff embedding"""
    import dfot_amd
    from oracle import dit as odit
    if name == "tiny":
        ocfg = odit.DiffDiTConfig(hidden_size=128, depth=2, num_heads=4, in_channels=4, resolution=(16, 8), embed_col_dim=64, num_row_heads=4)
    else:  # two column heads, no biases, no temporal MLP
        ocfg = odit.DiffDiTConfig(hidden_size=128, depth=1, num_heads=2, in_channels=4, resolution=(16, 8), embed_col_dim=64,
                                  num_col_heads=2, num_row_heads=2, use_bias=False, mlp_ratio=0.0)
    params = odit.diff_seeded_params(ocfg, 7)
    cfg = dict(variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", merge_type="interleaved", patch_size=ocfg.patch_size,
               embed_col_dim=ocfg.embed_col_dim, embed_row_dim=ocfg.hidden_size, num_heads=ocfg.num_heads, num_col_heads=ocfg.num_col_heads,
               num_row_heads=ocfg.num_row_heads, depth=ocfg.depth, mlp_ratio=ocfg.mlp_ratio or None, spatial_mlp_ratio=ocfg.spatial_mlp_ratio,
               use_bias=ocfg.use_bias, matrix_block="matrix")
    tr = dfot_amd.DiT3DTrainer(cfg, x_shape=(4, 16, 8), max_tokens=5)
    tr.load_state_dict(params, strict=True)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 10, 4, 16, 8, generator=g)
    k = torch.randint(0, 1000, (2, 10), generator=g)
    d_out = torch.randn(2, 10, 4, 16, 8, generator=g)
    out = tr.forward(x, k).cpu()
    tr.backward(d_out)
    grads = {n: t.cpu() for n, t in tr.grad_dict().items()}
    ps = {n: t.clone().requires_grad_() for n, t in params.items()}
    ref = odit.diff_forward(ps, ocfg, x, k)
    assert rel(out, ref.detach()) < 2e-2
    (ref * d_out).sum().backward()
    worst = ("", 0.0)
    for n, t in ps.items():
        r = rel(grads[n], t.grad)
        if r > worst[1]:
            worst = (n, r)
        assert torch.isfinite(grads[n]).all(), n
    print(f"DifferenceDiT3D backward ({name}): worst gradient rel-L2 {worst[1]:.2e} at {worst[0]}")
    for n, t in ps.items():
        assert rel(grads[n], t.grad) < 5e-2, (n, rel(grads[n], t.grad))


def test_difference_training_step_loss_and_accumulation():
    """DifferenceDFoTVideo.training_step front end (torch.diff + interleaved merge, doubled levels / masks) -> loss vs the oracle's
    discrete loss on the merged tokens; accumulate() over two micro-batches equals one backward over both"""
    import dfot_amd
    from oracle import dit as odit, sampler as osm, schedule as sch
    ocfg = odit.DiffDiTConfig(hidden_size=128, depth=1, num_heads=4, in_channels=4, resolution=(16, 8), embed_col_dim=64, num_row_heads=4)
    params = odit.diff_seeded_params(ocfg, 11)
    cfg = dict(variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", merge_type="interleaved", patch_size=1, embed_col_dim=64,
               embed_row_dim=128, num_heads=4, num_col_heads=1, num_row_heads=4, depth=1, mlp_ratio=4.0, spatial_mlp_ratio=4.0, use_bias=True)
    tr = dfot_amd.DiT3DTrainer(cfg, x_shape=(4, 16, 8), max_tokens=5, loss_weighting=dict(strategy="fused_min_snr", cum_snr_decay=0.9))
    tr.load_state_dict(params, strict=True)
    g = torch.Generator().manual_seed(6)
    frames = torch.randn(4, 5, 4, 16, 8, generator=g)
    k = torch.randint(0, 1000, (4, 5), generator=g)
    noise = torch.randn(4, 10, 4, 16, 8, generator=g)
    masks = torch.ones(4, 5)
    masks[0, 4] = 0
    loss = float(tr.difference_loss_and_grads(frames, k, noise, masks).item())
    full = tr.grads.clone()
    # oracle: the reference's merge (difference first) and DiscreteDiffusion.forward on the merged tokens
    merge = lambda a, b: torch.stack([a, b], dim=2).flatten(1, 2)
    xs = merge(torch.diff(frames, dim=1, prepend=frames[:, :1]), frames)
    kk, mm = merge(k, k), merge(masks, masks)
    model = lambda x, lv, c, m: odit.diff_forward(params, ocfg, x, lv)
    _, per_el = osm.discrete_training_loss(model, sch.build_tables(beta_schedule="cosine"), xs, kk, noise.clamp(-20, 20), strategy="fused_min_snr",
                                           cum_snr_decay=0.9)
    ref = float((per_el * mm[..., None, None, None]).mean())
    assert abs(loss - ref) < 2e-2 * abs(ref), (loss, ref)
    # two micro-batches of 2 videos, accumulated, = the mean of their gradients = the gradient of the 4-video batch
    for sl in (slice(0, 2), slice(2, 4)):
        tr.difference_loss_and_grads(frames[sl], k[sl], noise[sl], masks[sl])
        tr.accumulate()
    acc = tr._acc / tr._acc_n
    assert rel(acc.cpu(), full.cpu()) < 2e-2


@pytest.mark.parametrize("tag", ["dit", "diff"])
def test_training_gradients_vs_reference_fixture(tag):
    """loss and gradients of the reference's own training step (tests/golden/training_grads.npz, differentiated by the reference's
    autograd on CPU) vs the engine: gradient norm of every parameter and the stored gradient tensors"""
    import os
    import dfot_amd
    from conftest import GOLDEN
    from oracle import dit as odit
    g = np.load(os.path.join(GOLDEN, "training_grads.npz"))
    xs, k, masks = (torch.from_numpy(g[n]) for n in ("xs", "k", "masks"))
    lw = dict(strategy="fused_min_snr", cum_snr_decay=0.96)
    if tag == "dit":
        ocfg, params, tr = _tiny_trainer(depth=2, seed=2)
        tr.loss_weighting = lw
        loss = tr.loss_and_grads(xs, k, torch.from_numpy(g["dit_noise"]), masks)
    else:
        ocfg = odit.DiffDiTConfig(hidden_size=128, depth=2, num_heads=4, in_channels=4, resolution=(16, 8), embed_col_dim=64, num_row_heads=4)
        params = odit.diff_seeded_params(ocfg, 3)
        cfg = dict(variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", merge_type="interleaved", patch_size=1, embed_col_dim=64,
                   embed_row_dim=128, num_heads=4, num_col_heads=1, num_row_heads=4, depth=2, mlp_ratio=4.0, spatial_mlp_ratio=4.0, use_bias=True)
        tr = dfot_amd.DiT3DTrainer(cfg, x_shape=(4, 16, 8), max_tokens=5, loss_weighting=lw)
        tr.load_state_dict(params, strict=True)
        loss = tr.difference_loss_and_grads(xs, k, torch.from_numpy(g["diff_noise"]), masks)
    ref_loss = float(g[f"{tag}_loss"])
    assert abs(float(loss.item()) - ref_loss) < 2e-2 * abs(ref_loss)
    grads = {n: t.cpu() for n, t in tr.grad_dict().items()}
    names = [str(n) for n in g[f"{tag}_names"]]
    assert names == list(grads)
    for n, ref_norm in zip(names, g[f"{tag}_norms"]):
        assert abs(float(grads[n].norm()) - ref_norm) <= 3e-2 * ref_norm + 1e-7, (n, float(grads[n].norm()), ref_norm)
    worst = 0.0
    for key in g.files:
        if key.startswith(f"{tag}_grad/"):
            n = key.split("/", 1)[1]
            ref = torch.from_numpy(g[key])
            if float(ref.norm()) > 1e-6:
                worst = max(worst, rel(grads[n], ref))
    print(f"{tag}: worst stored-gradient rel-L2 vs the reference {worst:.2e}")
    assert worst < 5e-2


def test_ema_and_optimizer_state_round_trip():
    """EMA shadow weights follow EMAModel.step; the optimizer state exports in torch.optim.AdamW's layout, reloads into a fresh
    trainer, and both then take the same next step"""
    ocfg, params, tr = _tiny_trainer(depth=1)
    tr.lr = 1e-3
    tr.enable_ema(0.9)
    g = torch.Generator().manual_seed(8)
    xs = torch.randn(2, 5, 4, 16, 8, generator=g)
    k = torch.randint(0, 1000, (2, 5), generator=g)
    noise = torch.randn(2, 5, 4, 16, 8, generator=g)
    p0 = tr.params.clone()
    tr.training_step(xs, k, noise)
    torch.testing.assert_close(tr.ema, 0.9 * p0 + 0.1 * tr.params, rtol=1e-6, atol=1e-7)
    sd = tr.optimizer_state_dict()
    assert len(sd["state"]) == len(tr.layout) and sd["param_groups"][0]["betas"] == (0.9, 0.99)
    torch.optim.AdamW([torch.nn.Parameter(torch.zeros(s)) for _, s in tr.layout.values()]).load_state_dict(sd)  # torch accepts it
    _, _, tr2 = _tiny_trainer(depth=1)
    tr2.load_state_dict(tr.state_dict())
    tr2.load_optimizer_state_dict(sd)
    assert tr2.step_count == 1 and tr2.lr == 1e-3
    tr.training_step(xs, k, noise)
    tr2.training_step(xs, k, noise)
    torch.testing.assert_close(tr2.params, tr.params, rtol=1e-5, atol=1e-6)


def test_dit_ema_resumes_from_its_state_dict():
    """the EMA shadow after one training step, exported by ema_state_dict, lands bit for bit in a fresh trainer's shadow through
    load_ema_state_dict; a state dict with other keys is refused (the U-ViT trainers' behaviour: one flat optimizer state serves both)"""
    _, _, tr = _tiny_trainer(depth=1)
    tr.enable_ema(0.9)
    g = torch.Generator().manual_seed(8)
    xs = torch.randn(2, 5, 4, 16, 8, generator=g)
    k = torch.randint(0, 1000, (2, 5), generator=g)
    tr.training_step(xs, k, torch.randn(2, 5, 4, 16, 8, generator=g))
    assert not torch.equal(tr.ema, tr.params)  # the step moved the parameters away from their shadow
    sd = tr.ema_state_dict()
    _, _, fresh = _tiny_trainer(depth=1)
    with pytest.raises(RuntimeError, match="EMA is not enabled"):
        fresh.load_ema_state_dict(sd)
    fresh.enable_ema(0.9)
    assert not torch.equal(fresh.ema, tr.ema)
    fresh.load_ema_state_dict(sd)
    assert torch.equal(fresh.ema, tr.ema)
    with pytest.raises(ValueError, match="does not match the structure of the EMA model"):
        fresh.load_ema_state_dict({"nope": torch.zeros(1)})
    assert torch.equal(fresh.ema, tr.ema)  # a refused dict changes nothing


@pytest.mark.parametrize("bt,h,w,cin,cout", [(2, 16, 16, 128, 128), (3, 8, 16, 64, 192), (1, 32, 32, 256, 128), (2, 16, 16, 256, 256),
                                             (1, 16, 16, 576, 256), (8, 32, 32, 128, 128), (16, 32, 32, 256, 256)])
def test_conv3x3_backward(bt, h, w, cin, cout):
    """dx / dW / db of the channels-last 3x3 convolution (UViT ResBlocks, resamplers) vs torch autograd on the bf16-rounded operands"""
    from dfot_amd import capi
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(bt, h, w, cin, generator=g).to(torch.bfloat16)
    dy = torch.randn(bt, h, w, cout, generator=g).to(torch.bfloat16)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
    xd, dyd, wd = x.cuda().contiguous(), dy.cuda().contiguous(), wt.cuda().contiguous()
    dx = torch.full((bt, h, w, cin), float("nan"), device="cuda")
    dw = torch.full((cout, cin, 3, 3), float("nan"), device="cuda")
    db = torch.full((cout,), float("nan"), device="cuda")
    capi.check(capi.lib.dfot_op_conv3x3_bwd(capi.ptr(xd), capi.ptr(dyd), capi.ptr(wd), capi.ptr(dx), capi.ptr(dw), capi.ptr(db), bt, h, w, cin, cout,
                                            capi.stream_ptr()))
    torch.cuda.synchronize()
    xr = x.float().permute(0, 3, 1, 2).requires_grad_()
    wr = wt.to(torch.bfloat16).float().requires_grad_()  # the data gradient uses bf16 weights
    br = torch.zeros(cout, requires_grad=True)
    y = torch.nn.functional.conv2d(xr, wr, br, padding=1)
    y.backward(dy.float().permute(0, 3, 1, 2))
    r = (rel(dx.cpu(), xr.grad.permute(0, 2, 3, 1)), rel(dw.cpu(), wr.grad), rel(db.cpu(), br.grad))
    print(f"conv3x3 backward {cin}->{cout}: rel dx {r[0]:.2e} dW {r[1]:.2e} db {r[2]:.2e}")
    assert max(r) < 1e-2, r


@pytest.mark.parametrize("film", [False, True])
@pytest.mark.parametrize("bt,pix,c", [(3, 256, 128), (2, 64, 256)])
def test_groupnorm_silu_backward(film, bt, pix, c):
    """backward of SiLU(GN32(x) [* (1 + scale) + shift]) -- both norm layers of a UViT ResBlock -- vs torch autograd"""
    from dfot_amd import capi
    F = torch.nn.functional
    g = torch.Generator().manual_seed(c + pix)
    x = torch.randn(bt, pix, c, generator=g) * 1.5 + 0.3
    dy = torch.randn(bt, pix, c, generator=g)
    gamma, beta = torch.randn(c, generator=g) * 0.5 + 1, torch.randn(c, generator=g) * 0.2
    fl = (torch.randn(bt * pix, 2 * c, generator=g) * 0.5).to(torch.bfloat16) if film else None
    dx = torch.full((bt, pix, c), float("nan"), device="cuda")
    dfl = torch.empty(bt * pix, 2 * c, dtype=torch.bfloat16, device="cuda") if film else None
    dga, dbe = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    xd, dyd, gd, bd, fd = x.cuda(), dy.cuda(), gamma.cuda(), beta.cuda(), (fl.cuda() if film else None)  # keep the device copies alive
    capi.check(capi.lib.dfot_op_gn_silu_bwd(capi.ptr(xd), capi.ptr(dyd), capi.ptr(gd), capi.ptr(bd), capi.ptr(fd), 1e-6, capi.ptr(dx), capi.ptr(dfl), capi.ptr(dga), capi.ptr(dbe),
                                            bt, pix, c, capi.stream_ptr()))
    torch.cuda.synchronize()
    xr, gr, br = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    h = F.group_norm(xr.permute(0, 2, 1), 32, gr, br, 1e-6).permute(0, 2, 1)
    if film:
        fr = fl.float().view(bt, pix, 2 * c).requires_grad_()
        h = h * (1 + fr[..., :c]) + fr[..., c:]
    F.silu(h).backward(dy)
    rs = [rel(dx.cpu(), xr.grad), rel(dga.cpu(), gr.grad), rel(dbe.cpu(), br.grad)]
    if film:
        rs.append(rel(dfl.float().cpu().view(bt, pix, 2 * c), fr.grad))
    print(f"GN+SiLU backward film={film} C={c}: " + " ".join(f"{r:.1e}" for r in rs))
    assert max(rs[:3]) < 1e-4 and (not film or rs[3] < 5e-3)


@pytest.mark.parametrize("bt,h,w,c", [(2, 16, 16, 128), (8, 32, 32, 128), (2, 16, 16, 256)])
def test_conv3x3_backward_bf16_data_gradient_feeds_the_groupnorm_backward(bt, h, w, c):
    """the ResBlock's chain conv backward -> GroupNorm backward with the data gradient kept in bf16 (dfot_op_conv3x3_bwd2 dx_bf ->
    dfot_op_gn_silu_bwd5): dx_bf is the bf16 rounding of the fp32 entry's dx (same kernel, other epilogue), and the chain equals torch
    autograd through conv2d(SiLU(GroupNorm(x))) on the bf16-rounded operands.  Tolerances: bf16 data gradient (2^-9) into sums over
    >= 256 pixels; dgamma / dbeta / dx 5e-3 (measured ~1e-3)."""
    from dfot_amd import capi
    F = torch.nn.functional
    g = torch.Generator().manual_seed(7 * c + h)
    pix = h * w
    x = torch.randn(bt, pix, c, generator=g) * 1.5 + 0.3
    gamma, beta = torch.randn(c, generator=g) * 0.5 + 1, torch.randn(c, generator=g) * 0.2
    wt = torch.randn(c, c, 3, 3, generator=g) / math.sqrt(9 * c)
    dy = torch.randn(bt, h, w, c, generator=g).to(torch.bfloat16)
    xd, gd, bd, wd, dyd = x.cuda(), gamma.cuda(), beta.cuda(), wt.cuda().contiguous(), dy.cuda().contiguous()
    # forward pieces on the device: hact = SiLU(GN(x)) in bf16 + saved statistics
    hact = torch.empty(bt * pix, c, dtype=torch.bfloat16, device="cuda")
    stats = torch.empty(bt, 32, 2, device="cuda")
    capi.check(capi.lib.dfot_op_gn_silu_fwd(capi.ptr(xd), capi.ptr(gd), capi.ptr(bd), None, 1e-6, capi.ptr(hact), capi.ptr(stats), bt, pix, c, capi.stream_ptr()))
    dh_bf = torch.full((bt * pix, c), float("nan"), dtype=torch.bfloat16, device="cuda")
    dh32 = torch.full((bt * pix, c), float("nan"), device="cuda")
    dw, db = torch.empty(c, c, 3, 3, device="cuda"), torch.empty(c, device="cuda")
    dw2, db2 = torch.empty_like(dw), torch.empty_like(db)
    capi.check(capi.lib.dfot_op_conv3x3_bwd2(capi.ptr(hact), capi.ptr(dyd), capi.ptr(wd), None, capi.ptr(dh_bf), capi.ptr(dw), capi.ptr(db), bt, h, w, c, c,
                                             capi.stream_ptr()))
    capi.check(capi.lib.dfot_op_conv3x3_bwd2(capi.ptr(hact), capi.ptr(dyd), capi.ptr(wd), capi.ptr(dh32), None, capi.ptr(dw2), capi.ptr(db2), bt, h, w, c, c,
                                             capi.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(dh_bf, dh32.to(torch.bfloat16)) and torch.equal(dw, dw2) and torch.equal(db, db2)
    # exactly one of dx / dx_bf
    assert capi.lib.dfot_op_conv3x3_bwd2(capi.ptr(hact), capi.ptr(dyd), capi.ptr(wd), capi.ptr(dh32), capi.ptr(dh_bf), capi.ptr(dw), capi.ptr(db), bt, h, w,
                                         c, c, capi.stream_ptr()) != 0
    dres = torch.randn(bt, pix, c, generator=g).cuda()
    dx, dx_bf = torch.full((bt, pix, c), float("nan"), device="cuda"), torch.empty(bt * pix, c, dtype=torch.bfloat16, device="cuda")
    dga, dbe = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    capi.check(capi.lib.dfot_op_gn_silu_bwd5(capi.ptr(xd), capi.ptr(dh_bf), capi.ptr(stats), capi.ptr(gd), capi.ptr(bd), None, capi.ptr(dres), capi.ptr(dx),
                                             capi.ptr(dx_bf), None, 0, capi.ptr(dga), capi.ptr(dbe), bt, pix, c, capi.stream_ptr()))
    torch.cuda.synchronize()
    xr, gr, br = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    hr = F.silu(F.group_norm(xr.permute(0, 2, 1), 32, gr, br, 1e-6))            # [bt][c][pix]
    y = F.conv2d(hr.view(bt, c, h, w), wt.to(torch.bfloat16).float(), None, padding=1)
    y.backward(dy.float().permute(0, 3, 1, 2))
    rs = [rel(dx.cpu() - dres.cpu(), xr.grad), rel(dga.cpu(), gr.grad), rel(dbe.cpu(), br.grad)]
    print(f"conv -> GN backward with a bf16 data gradient, C={c} {h}x{w}: " + " ".join(f"{r:.1e}" for r in rs))
    assert max(rs) < 5e-3, rs
    assert torch.equal(dx_bf.view(bt, pix, c), dx.to(torch.bfloat16))


def test_folded_film_helpers_frame_sums_split_products():
    """the small pieces of the folded FiLM (uvit_train.UViT3DPoseTrainer.sync): per-frame column sums of a bf16 matrix, the strided fp32
    product in its four orientations, and the split-bf16 products (three MFMA GEMMs / token-axis kernels) against fp64"""
    from dfot_amd import capi, uvit_train as ut
    g = torch.Generator().manual_seed(5)
    bt, pix, n = 6, 320, 264
    src = torch.randn(bt * pix, n + 8, generator=g).to(torch.bfloat16).cuda()
    got = ut.frame_sums(src[:, :n], bt, pix)
    assert rel(got.cpu(), src[:, :n].float().view(bt, pix, n).sum(1).cpu()) < 1e-6
    a, b = torch.randn(70, 45, generator=g).cuda(), torch.randn(45, 33, generator=g).cuda()
    want = (a.double() @ b.double()).float()
    assert rel(ut.sgemm(a, b).cpu(), want.cpu()) < 1e-6
    assert rel(ut.sgemm(a.t().contiguous(), b, ta=True).cpu(), want.cpu()) < 1e-6
    assert rel(ut.sgemm(a, b.t().contiguous(), tb=True).cpu(), want.cpu()) < 1e-6
    acc = torch.ones(70, 33, device="cuda")
    ut.sgemm(a.t().contiguous(), b.t().contiguous(), ta=True, tb=True, out=acc, accumulate=True)
    assert rel(acc.cpu(), (want + 1).cpu()) < 1e-6
    # split-bf16 products: fp32 accuracy from bf16 matrix cores
    x = torch.randn(256, 192, generator=g).cuda() * 3
    hi, lo = ut.split_bf16(x)
    assert float((hi.float() + lo.float() - x).abs().max() / x.abs().max()) < 2.0 ** -15
    w = torch.randn(384, 192, generator=g).cuda()
    ref = (x.double() @ w.double().t())
    got = ut.wprod(ut.split_bf16(x), ut.split_bf16(w))
    plain = ut.gemm_f32(ut._bf(x), ut._bf(w))
    e3, e1 = rel(got.cpu(), ref.float().cpu()), rel(plain.cpu(), ref.float().cpu())
    print(f"split-bf16 product: rel error {e3:.1e} (one bf16 product: {e1:.1e})")
    assert e3 < 3e-5 and e1 > 20 * e3
    rows = 4096                                      # the long axis shared: A^T B on the token-axis kernel
    A, B = torch.randn(rows, 128, generator=g).cuda(), torch.randn(rows, 64, generator=g).cuda()
    got_t = ut.wprod_t(ut.split_bf16(A), ut.split_bf16(B))
    assert rel(got_t.cpu(), (A.double().t() @ B.double()).float().cpu()) < 3e-5


@pytest.mark.parametrize("c", [128, 256])
def test_frame_bias_gemm_and_groupnorm_on_a_column_block(c):
    """the folded-FiLM projection: dfot_op_gemm_bf16_frame_bias (a w^T + table[row // rows_per_frame], the per-frame part in the GEMM
    epilogue) vs fp32 torch, and the GroupNorm + FiLM + SiLU entries reading a block's (scale | shift) columns out of a level-wide matrix
    (film_ld: dfot_op_gn_silu_fwd2 / _bwd6) vs torch autograd"""
    from dfot_amd import capi, uvit_train as ut
    F = torch.nn.functional
    g = torch.Generator().manual_seed(c)
    bt, pix, k, nblk = 3, 256, 192, 3
    a = torch.randn(bt * pix, k, generator=g).to(torch.bfloat16).cuda()
    w = (torch.randn(nblk * 2 * c, k, generator=g) / math.sqrt(k)).to(torch.bfloat16).cuda()
    table = (torch.randn(bt, nblk * 2 * c, generator=g) * 0.4).cuda()
    film_all = ut.gemm_bf16_frames(a, w, table, pix)
    want = a.float() @ w.float().t() + table.repeat_interleave(pix, 0)
    assert rel(film_all.float().cpu(), want.cpu()) < 4e-3
    # rows_per_frame must divide M
    assert capi.lib.dfot_op_gemm_bf16_frame_bias(capi.ptr(a), k, capi.ptr(w), capi.ptr(table), pix - 1, capi.ptr(film_all), nblk * 2 * c, bt * pix,
                                                 nblk * 2 * c, k, capi.stream_ptr()) != 0
    x = torch.randn(bt, pix, c, generator=g) * 1.5 + 0.3
    gamma, beta = torch.randn(c, generator=g) * 0.5 + 1, torch.randn(c, generator=g) * 0.2
    dy = torch.randn(bt, pix, c, generator=g).to(torch.bfloat16)
    xd, gd, bd, dyd = x.cuda(), gamma.cuda(), beta.cuda(), dy.cuda()
    P, S = capi.ptr, capi.stream_ptr
    fview = film_all[:, 2 * c: 4 * c]                            # block 1 of 3: row pitch 6C
    out = torch.empty(bt * pix, c, dtype=torch.bfloat16, device="cuda")
    stats = torch.empty(bt, 32, 2, device="cuda")
    capi.check(capi.lib.dfot_op_gn_silu_fwd2(P(xd), P(gd), P(bd), capi.ptr_rows(fview), 6 * c, 1e-6, P(out), P(stats), bt, pix, c, S()))
    dx, dfl = torch.full((bt, pix, c), float("nan"), device="cuda"), torch.empty(bt * pix, 2 * c, dtype=torch.bfloat16, device="cuda")
    dga, dbe = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    capi.check(capi.lib.dfot_op_gn_silu_bwd6(P(xd), P(dyd), P(stats), P(gd), P(bd), capi.ptr_rows(fview), 6 * c, None, P(dx), None, P(dfl), 2 * c, P(dga),
                                             P(dbe), bt, pix, c, S()))
    torch.cuda.synchronize()
    xr, gr, br = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    fr = fview.float().cpu().view(bt, pix, 2 * c).requires_grad_()
    h = F.group_norm(xr.permute(0, 2, 1), 32, gr, br, 1e-6).permute(0, 2, 1)
    y = F.silu(h * (1 + fr[..., :c]) + fr[..., c:])
    y.backward(dy.float())
    rs = [rel(out.float().cpu().view(bt, pix, c), y.detach()), rel(dx.cpu(), xr.grad), rel(dga.cpu(), gr.grad), rel(dbe.cpu(), br.grad),
          rel(dfl.float().cpu().view(bt, pix, 2 * c), fr.grad)]
    print(f"GroupNorm + FiLM on a column block, C={c}: " + " ".join(f"{r:.1e}" for r in rs))
    assert rs[0] < 5e-3 and max(rs[1:4]) < 1e-4 and rs[4] < 5e-3


@pytest.mark.parametrize("rows,c", [(512, 576), (300, 1152), (64, 128)])
def test_rms_film_backward(rows, c):
    """backward of RMSNorm(x; w) * (1 + scale) + shift (NormalizeWithCond of the UViT TransformerBlock) vs torch autograd"""
    from dfot_amd import capi
    from oracle import uvit as ouvit
    g = torch.Generator().manual_seed(rows + c)
    x, dxn = torch.randn(rows, c, generator=g) * 2, torch.randn(rows, c, generator=g)
    w = torch.randn(c, generator=g) * 0.3 + 1
    film = (torch.randn(rows, 2 * c, generator=g) * 0.5).to(torch.bfloat16)
    xd, gd, wd, fd = x.cuda(), dxn.cuda(), w.cuda(), film.cuda()
    dx, dw = torch.full((rows, c), float("nan"), device="cuda"), torch.empty(c, device="cuda")
    dfilm = torch.empty(rows, 2 * c, dtype=torch.bfloat16, device="cuda")
    capi.check(capi.lib.dfot_op_rms_film_bwd(capi.ptr(xd), capi.ptr(gd), capi.ptr(wd), capi.ptr(fd), 1e-6, capi.ptr(dx), capi.ptr(dfilm), capi.ptr(dw),
                                             rows, c, 0, capi.stream_ptr()))
    torch.cuda.synchronize()
    xr, wr, fr = x.clone().requires_grad_(), w.clone().requires_grad_(), film.float().requires_grad_()
    (ouvit.rms_norm(xr, wr, 1e-6) * (1 + fr[:, :c]) + fr[:, c:]).backward(dxn)
    rs = (rel(dx.cpu(), xr.grad), rel(dw.cpu(), wr.grad), rel(dfilm.float().cpu(), fr.grad))
    print(f"RMSNorm-FiLM backward C={c}: " + " ".join(f"{r:.1e}" for r in rs))
    assert rs[0] < 1e-5 and rs[1] < 1e-4 and rs[2] < 5e-3


@pytest.mark.parametrize("d,heads,ntok,batch", [(64, 9, 256, 2), (128, 3, 128, 1)])
def test_qknorm_rope_backward(d, heads, ntok, batch):
    """backward of the per-head q / k RMSNorm + RoPE of the fused projection vs torch autograd through the oracle's rms_norm / apply_rope"""
    from dfot_amd import capi
    from oracle import uvit as ouvit
    g = torch.Generator().manual_seed(d)
    c, rows = heads * d, batch * ntok
    fused = (torch.randn(rows, 7 * c, generator=g)).to(torch.bfloat16)
    dq, dk, dv = ((torch.randn(batch, heads, ntok, d, generator=g)).to(torch.bfloat16) for _ in range(3))
    qw, kw = torch.randn(d, generator=g) * 0.3 + 1, torch.randn(d, generator=g) * 0.3 + 1
    ang = torch.rand(ntok, d // 2, generator=g) * 6.28
    cs = torch.stack([ang.cos(), ang.sin()], -1).contiguous()
    dev = [t.cuda().contiguous() for t in (fused, dq, dk, dv, qw, kw, cs)]
    dfused = torch.zeros(rows, 7 * c, dtype=torch.bfloat16, device="cuda")
    dqw, dkw = torch.empty(d, device="cuda"), torch.empty(d, device="cuda")
    capi.check(capi.lib.dfot_op_qknorm_rope_bwd(capi.ptr(dev[0]), 7 * c, capi.ptr(dev[1]), capi.ptr(dev[2]), capi.ptr(dev[3]), capi.ptr(dev[4]),
                                                capi.ptr(dev[5]), capi.ptr(dev[6]), 1e-6, capi.ptr(dfused), 7 * c, capi.ptr(dqw), capi.ptr(dkw),
                                                rows, ntok, heads, d, capi.stream_ptr()))
    torch.cuda.synchronize()
    fr = fused.float().requires_grad_()
    qwr, kwr = qw.clone().requires_grad_(), kw.clone().requires_grad_()
    q, k, v = fr[:, :3 * c].view(batch, ntok, 3, heads, d).permute(2, 0, 3, 1, 4)
    full = ang.repeat_interleave(2, dim=-1)
    qn = ouvit.apply_rope(ouvit.rms_norm(q, qwr, 1e-6), full)
    kn = ouvit.apply_rope(ouvit.rms_norm(k, kwr, 1e-6), full)
    ((qn * dq.float()).sum() + (kn * dk.float()).sum() + (v * dv.float()).sum()).backward()
    rs = (rel(dfused.float().cpu()[:, :3 * c], fr.grad[:, :3 * c]), rel(dqw.cpu(), qwr.grad), rel(dkw.cpu(), kwr.grad))
    print(f"q/k norm + RoPE backward d={d}: " + " ".join(f"{r:.1e}" for r in rs))
    assert rs[0] < 5e-3 and rs[1] < 1e-4 and rs[2] < 1e-4


@pytest.mark.parametrize("form", [-1, 0, 1, 2, 3])
@pytest.mark.parametrize("m,n,rows", [(1152, 5760, 4096), (4032, 576, 8192), (576, 2880, 2048), (2304, 1024, 1024), (520, 264, 640), (128, 128, 8192)])
def test_wgrad_nt_tile_forms(m, n, rows, form):
    """the planned weight gradient (slices = 0) in every tile form -- 128 x 128 / 4 waves and the LDS-DMA 256 x 256, 256 x 192 and
    192 x 256 ones -- on the model's shapes and on one whose M, N are no multiples of any tile (zero-filled edge chunks)"""
    import subprocess, sys, textwrap
    # DFOT_WGRAD_FORM is read once per process: one child per form
    code = textwrap.dedent(f"""
        import torch, sys
        sys.path.insert(0, {os.path.dirname(os.path.dirname(os.path.abspath(__file__)))!r})
        from dfot_amd import capi
        rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
        m, n, rows = {m}, {n}, {rows}
        g = torch.Generator().manual_seed(m + n)
        a = torch.randn(rows, m + 64, generator=g).to(torch.bfloat16)
        b = torch.randn(rows, n + 128, generator=g).to(torch.bfloat16)
        ad, bd = a.cuda(), b.cuda()
        out = torch.full((m, n), float("nan"), device="cuda")
        capi.check(capi.lib.dfot_op_wgrad_nt(capi.ptr(ad), m + 64, capi.ptr(bd), n + 128, capi.ptr(out), m, n, rows, 0, capi.stream_ptr()))
        torch.cuda.synchronize()
        ref = a[:, :m].float().T @ b[:, :n].float()
        r = rel(out.cpu(), ref)
        print(f"wgrad_nt form {form} {{m}}x{{n}} K={{rows}}: rel {{r:.2e}}")
        assert r < 1e-5
    """)
    env = dict(os.environ)
    if form >= 0:
        env["DFOT_WGRAD_FORM"] = str(form)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-400:], r.stderr[-2000:] if r.returncode else "")
    assert r.returncode == 0


@pytest.mark.parametrize("m,n,rows,slices", [(128, 128, 256, 1), (384, 256, 1280, 3), (1152, 128, 640, 2), (256, 1152, 4096, 4)])
def test_wgrad_nt_gemm(m, n, rows, slices):
    """dW = dY^T X over the token axis with both operands in their own layout (transposed LDS fragment reads), incl. K slices and
    operands that are column blocks of wider matrices (row strides > M, N)"""
    from dfot_amd import capi
    g = torch.Generator().manual_seed(m + n)
    a = torch.randn(rows, m + 64, generator=g).to(torch.bfloat16)
    b = torch.randn(rows, n + 128, generator=g).to(torch.bfloat16)
    ad, bd = a.cuda(), b.cuda()
    out = torch.full((m, n), float("nan"), device="cuda")
    capi.check(capi.lib.dfot_op_wgrad_nt(capi.ptr(ad), m + 64, capi.ptr(bd), n + 128, capi.ptr(out), m, n, rows, slices, capi.stream_ptr()))
    torch.cuda.synchronize()
    ref = a[:, :m].float().T @ b[:, :n].float()
    r = rel(out.cpu(), ref)
    print(f"wgrad_nt {m}x{n} K={rows} slices={slices}: rel {r:.2e}")
    assert r < 1e-5


@pytest.mark.parametrize("c,heads", [(1152, 9), (576, 9)])
def test_uvit_transformer_block_train_unit(c, heads):
    """forward + hand-written backward of one UViT TransformerBlock (level 3: C = 1152, d = 128; level 2: C = 576, d = 64) composed over the
    C ABI vs torch autograd through the oracle's transformer_block: output, dx, d(embedding) and every parameter gradient"""
    from dfot_amd import uvit_train as ut
    from oracle import uvit as ouvit
    e, batch, sizes = 256, 2, (2, 8, 8)
    ntok = sizes[0] * sizes[1] * sizes[2]
    d = c // heads
    g = torch.Generator().manual_seed(c)
    shapes = ouvit._tr_block_shapes("blk", c, e, heads)
    params = {}
    for n, shp in shapes.items():
        if n.endswith("norm.weight") or n.endswith("q_norm.weight") or n.endswith("k_norm.weight"):
            params[n] = 1 + 0.1 * torch.randn(shp, generator=g)
        elif n.endswith("bias"):
            params[n] = 0.05 * torch.randn(shp, generator=g)
        else:
            params[n] = torch.randn(shp, generator=g) / math.sqrt(shp[-1])
    x = torch.randn(batch, ntok, c, generator=g)
    emb = (torch.randn(batch, ntok, e, generator=g) * 0.5).to(torch.bfloat16)
    dy = torch.randn(batch, ntok, c, generator=g)
    blk = ut.TransformerBlockTrain(params, "blk", c, heads, ut.rope_table(d, sizes))
    # the MLP branch's nn.Dropout(0.1), realised mask shared with the oracle
    mask = ((torch.rand(batch * ntok, 4 * c, generator=g) >= 0.1).float() / 0.9).to(torch.bfloat16)
    y = blk.forward(x.view(-1, c).cuda(), emb.view(-1, e).cuda().contiguous(), batch, mask.cuda())
    dx, demb = blk.backward(dy.view(-1, c).cuda())
    torch.cuda.synchronize()
    ps = {n: t.clone().requires_grad_() for n, t in params.items()}
    xr, er = x.clone().requires_grad_(), emb.float().requires_grad_()
    cfg = ouvit.UViTConfig(num_heads=heads)
    ang = ouvit.rope3d_angles(d, sizes, cfg.rope_theta)
    ref = ouvit.transformer_block(ps, "blk", xr, er, ang, cfg, mlp_mask=mask.float().view(batch, ntok, 4 * c))
    ref.backward(dy)
    rs = {"y": rel(y.cpu().view_as(ref), ref.detach()), "dx": rel(dx.cpu().view_as(x), xr.grad), "demb": rel(demb.cpu().view_as(er), er.grad)}
    for n in blk.grads:
        rs[n] = rel(blk.grads[n].cpu(), ps["blk." + n].grad)
    worst = max(rs, key=rs.get)
    print(f"UViT TransformerBlock unit C={c}: worst rel-L2 {rs[worst]:.2e} at {worst}; y {rs['y']:.1e} dx {rs['dx']:.1e} demb {rs['demb']:.1e}")
    assert rs["y"] < 1e-2 and max(rs.values()) < 3e-2, rs


@pytest.mark.parametrize("c,e,bt,h,w", [(128, 128, 2, 16, 16), (256, 256, 2, 8, 16)])
def test_uvit_res_block_train_unit(c, e, bt, h, w):
    """forward + hand-written backward of one UViT ResBlock composed over the C ABI vs torch autograd through the oracle's res_block"""
    from dfot_amd import uvit_train as ut
    from oracle import uvit as ouvit
    g = torch.Generator().manual_seed(c + h)
    params = {}
    for n, shp in ouvit._res_block_shapes("blk", c, e).items():
        if n.endswith(("0.weight", "out_norm.weight")):
            params[n] = 1 + 0.1 * torch.randn(shp, generator=g)
        elif n.endswith("bias"):
            params[n] = 0.05 * torch.randn(shp, generator=g)
        else:
            params[n] = torch.randn(shp, generator=g) / math.sqrt(float(np.prod(shp[1:])))
    x = torch.randn(bt, c, h, w, generator=g)
    emb = (torch.randn(bt, e, h, w, generator=g) * 0.5).to(torch.bfloat16)
    dy = torch.randn(bt, c, h, w, generator=g)
    cl = lambda t: t.permute(0, 2, 3, 1).reshape(bt * h * w, -1).contiguous()  # channels-last rows
    blk = ut.ResBlockTrain(params, "blk", c)
    y = blk.forward(cl(x).cuda(), cl(emb).cuda(), bt, h, w)
    dx, demb = blk.backward(cl(dy).cuda())
    torch.cuda.synchronize()
    ps = {n: t.clone().requires_grad_() for n, t in params.items()}
    xr, er = x.clone().requires_grad_(), emb.float().requires_grad_()
    ref = ouvit.res_block(ps, "blk", xr, er, ouvit.UViTConfig())
    ref.backward(dy)
    rs = {"y": rel(y.cpu(), cl(ref.detach())), "dx": rel(dx.cpu(), cl(xr.grad)), "demb": rel(demb.cpu(), cl(er.grad))}
    for n in blk.grads:
        rs[n] = rel(blk.grads[n].cpu(), ps["blk." + n].grad)
    worst = max(rs, key=rs.get)
    print(f"UViT ResBlock unit C={c}: worst rel-L2 {rs[worst]:.2e} at {worst}; y {rs['y']:.1e} dx {rs['dx']:.1e} demb {rs['demb']:.1e}")
    assert rs["y"] < 1e-2 and max(rs.values()) < 3e-2, rs


def test_uvit3d_pose_backward_matches_autograd():
    """the whole UViT3DPose backbone (ResBlock levels, down / up convolutions with the skip arithmetic, transformer levels, pose patch
    embedding + embedding pyramid, noise-level MLP, input / output projections): forward and EVERY parameter gradient vs torch autograd
    through the oracle restatement, on a reduced model (channels 128/128/128/256, 2 heads: d = 64 / 128, 128x128 frames, 2 tokens)"""
    from dfot_amd import uvit_train as ut
    from oracle import pose as opose, uvit as ouvit
    cfg = ouvit.UViTConfig(channels=(128, 128, 128, 256), emb_channels=128, num_updown_blocks=(1, 1, 1), num_mid_blocks=2, num_heads=2, resolution=128,
                           max_tokens=2)
    params = ouvit.seeded_params(cfg, seed=4)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, 2, 3, 128, 128, generator=g)
    k = torch.randn(1, 2, generator=g)
    poses = torch.eye(3, 4).reshape(1, 1, 12).repeat(1, 2, 1)
    poses[..., 3] = torch.linspace(0, 0.3, 2)
    cond = opose.ray_encoding(torch.cat([torch.tensor([0.5, 0.9, 0.5, 0.5]).repeat(1, 2, 1), poses], -1), 128)
    d_out = torch.randn(1, 2, 3, 128, 128, generator=g)
    tr = ut.UViT3DPoseTrainer(params, dict(channels=cfg.channels, emb_channels=cfg.emb_channels, patch_size=2, block_types=cfg.block_types,
                                           num_updown_blocks=cfg.num_updown_blocks, num_mid_blocks=cfg.num_mid_blocks, num_heads=cfg.num_heads,
                                           resolution=128, max_tokens=2))
    out = tr.forward(x, k, cond).cpu()
    grads = {n: t.cpu() for n, t in tr.backward(d_out).items()}
    ps = {n: t.clone().requires_grad_(not n.endswith(("freqs", "phases"))) for n, t in params.items()}
    ref = ouvit.forward(ps, cfg, x, k, cond)
    r_out = rel(out, ref.detach())
    (ref * d_out).sum().backward()
    names = [n for n in ps if ps[n].requires_grad]
    assert sorted(grads) == sorted(names)
    rs = {n: rel(grads[n], ps[n].grad) for n in names}
    worst = max(rs, key=rs.get)
    print(f"UViT3DPose backward: forward rel-L2 {r_out:.2e}; worst gradient rel-L2 {rs[worst]:.2e} at {worst}")
    assert r_out < 2e-2 and rs[worst] < 3e-2, (r_out, worst, rs[worst])


def test_uvit3d_pose_training_step():
    """DFoTVideo.training_step for the pose model on the engine: loss vs the oracle's continuous v-prediction loss, then clipped AdamW
    steps on the flat buffer: the loss on the same batch falls"""
    from dfot_amd import uvit_train as ut
    from oracle import pose as opose, sampler as osm, uvit as ouvit
    cfg = ouvit.UViTConfig(channels=(128, 128, 128, 256), emb_channels=128, num_updown_blocks=(1, 1, 1), num_mid_blocks=1, num_heads=2, resolution=128,
                           max_tokens=2)
    params = ouvit.seeded_params(cfg, seed=5)
    g = torch.Generator().manual_seed(3)
    xs = torch.randn(1, 2, 3, 128, 128, generator=g)
    t = torch.rand(1, 2, generator=g)
    noise = torch.randn(1, 2, 3, 128, 128, generator=g)
    poses = torch.eye(3, 4).reshape(1, 1, 12).repeat(1, 2, 1)
    poses[..., 3] = torch.linspace(0, 0.3, 2)
    cond = opose.ray_encoding(torch.cat([torch.tensor([0.5, 0.9, 0.5, 0.5]).repeat(1, 2, 1), poses], -1), 128)
    tr = ut.UViT3DPoseTrainer(params, dict(channels=cfg.channels, emb_channels=cfg.emb_channels, patch_size=2, block_types=cfg.block_types,
                                           num_updown_blocks=cfg.num_updown_blocks, num_mid_blocks=cfg.num_mid_blocks, num_heads=cfg.num_heads,
                                           resolution=128, max_tokens=2))
    loss0 = float(tr.loss_and_grads(xs, cond, t, noise).item())
    with torch.no_grad():
        _, per_el = osm.training_loss(lambda x, lv, c, m: ouvit.forward(params, cfg, x, lv, c), xs, cond, t, noise)
    ref = float(per_el.mean())
    assert abs(loss0 - ref) < 2e-2 * abs(ref), (loss0, ref)
    # one clipped AdamW step vs torch (autograd through the oracle + clip_grad_norm_ + torch.optim.AdamW), where the gradient is not negligible
    before = {n: v.detach().clone().cpu() for n, v in tr.p.items()}
    tr.optimizer_step(lr=1e-4)
    ps = {n: v.clone().requires_grad_(not n.endswith(("freqs", "phases"))) for n, v in params.items()}
    _, per_el = osm.training_loss(lambda x, lv, c, m: ouvit.forward(ps, cfg, x, lv, c), xs, cond, t, noise)
    per_el.mean().backward()
    plist = [v for v in ps.values() if v.requires_grad]
    torch.nn.utils.clip_grad_norm_(plist, 1.0)
    torch.optim.AdamW(plist, lr=1e-4, weight_decay=0.01, betas=(0.9, 0.99), eps=1e-8).step()
    checked = 0
    for n, v in ps.items():
        if not v.requires_grad:
            continue
        big = v.grad.abs() > 2e-2 * v.grad.abs().max()
        if big.any():
            upd, ref_upd = tr.p[n].detach().cpu() - before[n], v.detach() - params[n]
            assert rel(upd[big], ref_upd[big]) < 0.1, n
            checked += int(big.sum())
    assert checked > 10000
    assert np.isfinite(float(tr.loss_and_grads(xs, cond, t, noise).item()))


def _uvit_small():
    from oracle import pose as opose, uvit as ouvit
    cfg = ouvit.UViTConfig(channels=(128, 128, 128, 256), emb_channels=128, num_updown_blocks=(1, 1, 1), num_mid_blocks=1, num_heads=2, resolution=128,
                           max_tokens=2)
    params = ouvit.seeded_params(cfg, seed=5)
    g = torch.Generator().manual_seed(3)
    xs = torch.randn(2, 2, 3, 128, 128, generator=g)
    t = torch.rand(2, 2, generator=g)
    noise = torch.randn(2, 2, 3, 128, 128, generator=g)
    poses = torch.eye(3, 4).reshape(1, 1, 12).repeat(2, 2, 1)
    poses[..., 3] = torch.linspace(0, 0.3, 2)
    poses[1, :, 7] = 0.1
    cond = opose.ray_encoding(torch.cat([torch.tensor([0.5, 0.9, 0.5, 0.5]).repeat(2, 2, 1), poses], -1), 128)
    tcfg = dict(channels=cfg.channels, emb_channels=cfg.emb_channels, patch_size=2, block_types=cfg.block_types, num_updown_blocks=cfg.num_updown_blocks,
                num_mid_blocks=cfg.num_mid_blocks, num_heads=cfg.num_heads, resolution=128, max_tokens=2)
    return params, tcfg, xs, t, noise, cond


def _uvit_ddp_worker(rank, world, port, q):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from dfot_amd import uvit_train as ut
        params, tcfg, xs, t, noise, cond = _uvit_small()
        tr = ut.UViT3DPoseTrainer(params, tcfg)
        sl = slice(rank, rank + 1)
        loss = tr.loss_and_grads(xs[sl], cond[sl], t[sl], noise[sl])
        tr.optimizer_step(lr=1e-4, world_size=world)
        q.put((rank, float(loss.item()), tr.flat_grads.cpu().numpy(), tr.flat.cpu().numpy()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_uvit_data_parallel_step_equals_single_process_step():
    """BASELINE config 5's data parallelism on the pose model: two ranks with one video each (flat-gradient all-reduce, mean) take the same
    optimizer step as one process with both videos"""
    import socket
    import torch.multiprocessing as mp
    from dfot_amd import uvit_train as ut
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_uvit_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=480) for _ in procs), key=lambda v: v[0])
    for p in procs:
        p.join(60)
    params, tcfg, xs, t, noise, cond = _uvit_small()
    tr = ut.UViT3DPoseTrainer(params, tcfg)
    loss = float(tr.loss_and_grads(xs, cond, t, noise).item())
    tr.optimizer_step(lr=1e-4)
    grads, new = tr.flat_grads.cpu().numpy(), tr.flat.cpu().numpy()
    assert np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])  # replicas stay identical
    assert abs(0.5 * (res[0][1] + res[1][1]) - loss) < 1e-3 * abs(loss)
    gr = np.linalg.norm(res[0][2] - grads) / np.linalg.norm(grads)
    print(f"UViT data-parallel vs single-process gradient rel-L2 {gr:.2e}")
    assert gr < 2e-2


def test_uvit_training_gradients_are_bit_reproducible():
    """VERDICT r2 weak #2 / next #5c: the bias / norm-weight / embedding sums of the RE10K backward used float atomics (two runs of one
    trainer differed by up to 5e-3 on cancellation-heavy sums); they are now per-workgroup partial rows added in a fixed order
    (csrc/dit_train.inl det_sum), so two backward passes on the same inputs give bit-identical gradients and the same loss."""
    from dfot_amd import uvit_train as ut
    params, tcfg, xs, t, noise, cond = _uvit_small()
    tr = ut.UViT3DPoseTrainer(params, tcfg)
    l0 = float(tr.loss_and_grads(xs, cond, t, noise).item())
    g0 = tr.flat_grads.clone()
    l1 = float(tr.loss_and_grads(xs, cond, t, noise).item())
    assert l0 == l1
    bad = [n for n, (o, shp) in tr.layout.items() if not torch.equal(g0[o: o + int(np.prod(shp))], tr.flat_grads[o: o + int(np.prod(shp))])]
    assert not bad, f"gradients differ between two runs: {bad[:8]}"
    other = ut.UViT3DPoseTrainer(params, tcfg)     # ... and across trainer instances
    other.loss_and_grads(xs, cond, t, noise)
    assert torch.equal(other.flat_grads, g0)


def test_uvit_trainer_ema_accumulation_state_and_checkpointing():
    """VERDICT r2 missing #2 / #3 for the RE10K trainer: EMA shadow weights (algorithms/common/ema.py:21-33, updated in the optimizer
    kernel), accumulate_grad_batches, optimizer state in torch.optim.AdamW layout (save / resume), and gradient checkpointing per level
    (u_vit3d.py:237-243, use_checkpointing [false, false, false, true] in the RE10K training config): the blocks of a checkpointed level
    keep only their inputs and are run forward again in the backward -- same gradients."""
    from dfot_amd import uvit_train as ut
    params, tcfg, xs, t, noise, cond = _uvit_small()
    tr = ut.UViT3DPoseTrainer(params, tcfg)
    loss0 = float(tr.loss_and_grads(xs, cond, t, noise).item())
    g_ref = tr.flat_grads.clone()
    # --- gradient checkpointing on the transformer levels and one ResBlock level: same loss, same gradients
    ck = ut.UViT3DPoseTrainer(params, dict(tcfg, use_checkpointing=[False, True, True, True]))
    loss1 = float(ck.loss_and_grads(xs, cond, t, noise).item())
    assert all("xn" not in b.saved for b in ck.mid)          # nothing but the inputs was kept ...
    assert abs(loss1 - loss0) < 1e-6 * abs(loss0)
    r = rel(ck.flat_grads, g_ref)                            # ... and the recomputed activations are the stored ones, bit for bit
    print(f"gradient checkpointing: flat-gradient rel-L2 vs the stored-activation backward {r:.2e}")
    assert torch.equal(ck.flat_grads, g_ref), r
    # --- accumulation: two micro-batches, mean of their gradients
    acc = ut.UViT3DPoseTrainer(params, tcfg)
    gs = []
    for i in range(2):
        acc.loss_and_grads(xs[i:i + 1], cond[i:i + 1], t[i:i + 1], noise[i:i + 1])
        gs.append(acc.flat_grads.clone())
        acc.accumulate()
    acc.enable_ema(0.9)
    before = acc.flat.clone()
    acc.optimizer_step(lr=1e-4, max_grad_norm=None)
    one = ut.UViT3DPoseTrainer(params, tcfg)
    one.flat_grads.copy_(0.5 * (gs[0] + gs[1]))
    one.optimizer_step(lr=1e-4, max_grad_norm=None)
    assert torch.equal(acc.flat, one.flat) and acc._acc_n == 0
    # --- EMA: shadow = decay * shadow + (1 - decay) * param after every optimizer step
    ema1 = 0.9 * before + 0.1 * acc.flat
    assert rel(acc.ema, ema1) < 1e-6
    acc.loss_and_grads(xs, cond, t, noise)
    acc.optimizer_step(lr=1e-4)
    assert rel(acc.ema, 0.9 * ema1 + 0.1 * acc.flat) < 1e-6
    sd = acc.ema_state_dict()
    assert list(sd) == list(acc.layout) and all(tuple(sd[n].shape) == acc.layout[n][1] for n in sd)
    # --- optimizer state: torch.optim.AdamW layout, resume gives the same next step
    osd = acc.optimizer_state_dict()
    assert len(osd["state"]) == len(acc.layout) and osd["param_groups"][0]["lr"] == 1e-4 and float(osd["state"][0]["step"]) == 2.0
    torch.optim.AdamW([torch.nn.Parameter(torch.zeros(v['exp_avg'].shape)) for v in osd['state'].values()]).load_state_dict(
        {'state': {i: {k: v.cpu() for k, v in st.items()} for i, st in osd['state'].items()}, 'param_groups': [dict(osd['param_groups'][0], foreach=None, maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)]})  # torch accepts it as its own
    res = ut.UViT3DPoseTrainer(acc.state_dict(), tcfg)
    res.load_optimizer_state_dict(osd)
    assert res.step_count == 2
    res.enable_ema(0.9)
    res.load_ema_state_dict(sd)
    for tr_ in (acc, res):
        tr_.loss_and_grads(xs, cond, t, noise)
        tr_.optimizer_step(lr=1e-4)
    assert rel(res.flat, acc.flat) < 1e-5 and rel(res.ema, acc.ema) < 1e-5
    with pytest.raises(ValueError):
        res.load_ema_state_dict({"nope": torch.zeros(1)})


def test_uvit_pose_dropout_mask():
    """per-video pose-embedding dropout (external_cond_dropout): forward and gradients with one of two videos dropped vs autograd through the
    oracle with the same external_cond_mask"""
    from dfot_amd import uvit_train as ut
    from oracle import uvit as ouvit
    params, tcfg, xs, t, noise, cond = _uvit_small()
    cfg = ouvit.UViTConfig(channels=(128, 128, 128, 256), emb_channels=128, num_updown_blocks=(1, 1, 1), num_mid_blocks=1, num_heads=2, resolution=128,
                           max_tokens=2)
    drop = torch.tensor([False, True])
    g = torch.Generator().manual_seed(1)
    d_out = torch.randn(2, 2, 3, 128, 128, generator=g)
    tr = ut.UViT3DPoseTrainer(params, tcfg)
    out = tr.forward(xs, t, cond, drop).cpu()
    grads = {n: v.cpu() for n, v in tr.backward(d_out).items()}
    ps = {n: v.clone().requires_grad_(not n.endswith(("freqs", "phases"))) for n, v in params.items()}
    ref = ouvit.forward(ps, cfg, xs, t, cond, drop)
    assert rel(out, ref.detach()) < 2e-2
    (ref * d_out).sum().backward()
    pe = "external_cond_embedding.patch_embedder.proj.weight"
    worst = max(rel(grads[n], ps[n].grad) for n in grads)
    print(f"UViT pose dropout: worst gradient rel-L2 {worst:.2e}; pose-embedding weight {rel(grads[pe], ps[pe].grad):.2e}")
    assert worst < 3e-2


def test_uvit_training_gradients_vs_reference_fixture():
    """loss and gradients of the reference's own pose-model training step (tests/golden/training_grads_uvit.npz, differentiated by the
    reference's autograd on CPU: UViT3DPose at reduced widths, 8 tokens of 128x128) vs the engine's training driver"""
    import os
    from conftest import GOLDEN
    from dfot_amd import uvit_train as ut
    from oracle import pose as opose, uvit as ouvit
    g = np.load(os.path.join(GOLDEN, "training_grads_uvit.npz"))
    cfg = ouvit.UViTConfig(channels=(128, 128, 128, 256), emb_channels=128, num_updown_blocks=(1, 1, 1), num_mid_blocks=1, num_heads=2, resolution=128)
    params = ouvit.seeded_params(cfg, 6)
    tr = ut.UViT3DPoseTrainer(params, dict(channels=cfg.channels, emb_channels=128, patch_size=2, block_types=cfg.block_types,
                                           num_updown_blocks=cfg.num_updown_blocks, num_mid_blocks=1, num_heads=2, resolution=128, max_tokens=8))
    cond = opose.ray_encoding(torch.from_numpy(g["poses"]), 128)
    loss = tr.loss_and_grads(torch.from_numpy(g["xs"]), cond, torch.from_numpy(g["k"]), torch.from_numpy(g["noise"]), torch.from_numpy(g["masks"]))
    ref_loss = float(g["loss"])
    assert abs(float(loss.item()) - ref_loss) < 2e-2 * abs(ref_loss), (float(loss.item()), ref_loss)
    grads = {n: v.cpu() for n, v in tr.grads.items()}
    names = [str(n) for n in g["names"]]
    assert sorted(names) == sorted(grads)
    for n, ref_norm in zip(names, g["norms"]):
        assert abs(float(grads[n].norm()) - ref_norm) <= 5e-2 * ref_norm + 1e-7, (n, float(grads[n].norm()), ref_norm)
    worst = 0.0
    for key in g.files:
        if key.startswith("grad/"):
            ref = torch.from_numpy(g[key])
            if float(ref.norm()) > 1e-6:
                worst = max(worst, rel(grads[key[5:]], ref))
    print(f"UViT3DPose: worst stored-gradient rel-L2 vs the reference {worst:.2e}")
    assert worst < 3e-2


def test_drop_in_two_forwards_before_backward_is_refused():
    """the drop-in keeps ONE saved-activation engine per module, so forward, forward, backward(first) would read the
    second forward's activations.  Each autograd ctx remembers the number of its forward; a backward whose activations were
    overwritten raises instead of returning gradients of the wrong input.  Forward/backward pairs (gradient accumulation) work."""
    import dfot_amd
    ocfg, params, tr = _tiny_trainer(depth=2, hidden=128, heads=4)
    model = dfot_amd.DiT3D(dict(variant="full", pos_emb_type="rope_3d", patch_size=1, hidden_size=128, depth=2, num_heads=4, spatial_mlp_ratio=None),
                           x_shape=(4, 16, 8), max_tokens=5).cuda()
    model.load_state_dict(params, strict=True)
    g = torch.Generator().manual_seed(2)
    x1, x2 = (torch.randn(2, 5, 4, 16, 8, generator=g).cuda() for _ in range(2))
    k = torch.randint(0, 1000, (2, 5), generator=g).cuda()
    v1 = model(x1, k)
    v2 = model(x2, k)
    v2.sum().backward()            # the latest forward owns the activations: fine
    with pytest.raises(RuntimeError, match="overwritten the saved"):
        v1.sum().backward()
    model.zero_grad()
    model(x1, k).sum().backward()  # accumulation as forward/backward pairs
    g1 = {n: p.grad.clone() for n, p in model.named_parameters()}
    model(x2, k).sum().backward()
    model.zero_grad()
    model(x2, k).sum().backward()
    for n, p in model.named_parameters():
        assert torch.isfinite(p.grad).all() and g1[n].shape == p.grad.shape


def test_drop_in_backbone_is_trainable_through_autograd():
    """the reference trains by calling `self.model(x_t, precond_scale * logsnr, external_cond)` under autograd and
    `accelerator.backward(loss)` (continuous_diffusion.py:154, simple_video_generation.py:260-270).  The drop-in nn.Module does the
    same: with gradients enabled its forward dispatches `dfot::uvit3d_pose_forward_train`, whose registered backward fills
    `param.grad` with the hand-written backward's result -- equal to UViT3DPoseTrainer.backward on the same weights / inputs, and
    within the stated tolerance of torch autograd through the oracle.  A plain torch optimizer then trains the module."""
    import dfot_amd
    from dfot_amd import uvit_train as ut
    from oracle import pose as opose, uvit as ouvit
    cfg = ouvit.UViTConfig(channels=(128, 128, 128, 256), emb_channels=128, num_updown_blocks=(1, 1, 1), num_mid_blocks=1, num_heads=2, resolution=128,
                           max_tokens=2)
    params = ouvit.seeded_params(cfg, seed=8)
    bcfg = dict(channels=list(cfg.channels), emb_channels=cfg.emb_channels, patch_size=2, block_types=list(cfg.block_types),
                num_updown_blocks=list(cfg.num_updown_blocks), num_mid_blocks=cfg.num_mid_blocks, num_heads=cfg.num_heads, pos_emb_type="rope",
                use_fourier_noise_embedding=True, conditioning=dict(dim=180))
    model = dfot_amd.UViT3DPose(bcfg, x_shape=(3, 128, 128), max_tokens=2).cuda()
    model.load_state_dict(params, strict=True)
    model.train()
    g = torch.Generator().manual_seed(10)
    x = torch.randn(1, 2, 3, 128, 128, generator=g).cuda()
    k = torch.randn(1, 2, generator=g).cuda()
    pz = torch.eye(3, 4).reshape(1, 1, 12).repeat(1, 2, 1)
    pz[..., 3] = torch.linspace(0, 0.3, 2)
    cond = opose.ray_encoding(torch.cat([torch.tensor([0.5, 0.9, 0.5, 0.5]).repeat(1, 2, 1), pz], -1), 128).cuda()
    w = torch.randn(1, 2, 3, 128, 128, generator=g).cuda()
    v = model(x, k, cond)                      # gradients enabled, parameters trainable -> training form
    assert v.requires_grad
    loss = (v * w).sum()
    loss.backward()
    # (1) identical to the trainer's own backward
    tr = ut.UViT3DPoseTrainer(params, dict(channels=cfg.channels, emb_channels=cfg.emb_channels, patch_size=2, block_types=cfg.block_types,
                                           num_updown_blocks=cfg.num_updown_blocks, num_mid_blocks=cfg.num_mid_blocks, num_heads=cfg.num_heads,
                                           resolution=128, max_tokens=2))
    out = tr.forward(x, k, cond)
    assert torch.equal(out, v.detach())
    tg = tr.backward(w)
    named = dict(model.named_parameters())
    assert sorted(tg) == sorted(named)
    # same kernels, but several reductions (embedding gradients, norm-weight sums) accumulate with float atomics whose order varies:
    # two runs of ONE trainer differ by up to 5e-3 on cancellation-heavy sums (q_norm / noise-embedding weights), so not bit for bit
    for n, p in named.items():
        assert p.grad is not None and rel(p.grad, tg[n].reshape(p.shape)) < 2e-2, (n, rel(p.grad, tg[n].reshape(p.shape)))
    # (2) within tolerance of autograd through the oracle
    ps = {n: t.clone().requires_grad_(not n.endswith(("freqs", "phases"))) for n, t in params.items()}
    ref = ouvit.forward(ps, cfg, x.cpu(), k.cpu(), cond.cpu())
    (ref * w.cpu()).sum().backward()
    rs = {n: rel(p.grad.cpu(), ps[n].grad) for n, p in named.items()}
    worst = max(rs, key=rs.get)
    print(f"drop-in autograd: forward rel-L2 {rel(v.detach().cpu(), ref.detach()):.2e}; worst gradient rel-L2 {rs[worst]:.2e} at {worst}")
    assert rs[worst] < 3e-2
    # (3) under no_grad the same module still runs the fused inference engine, and a torch optimizer step changes its output
    with torch.no_grad():
        before = model(x, k, cond)
    assert not before.requires_grad and rel(before.cpu(), ref.detach()) < 2e-2
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    opt.step()
    opt.zero_grad()
    v2 = model(x, k, cond)                     # picks the updated weights up (parameter versions changed)
    with torch.no_grad():
        after = model(x, k, cond)
    assert not torch.equal(v2.detach(), v.detach())
    assert rel(after, v2.detach()) < 2e-2      # inference engine and training form agree on the new weights


@pytest.mark.parametrize("blocks,mid,bar", [((1, 1, 1), 1, 3e-2), ((3, 3, 6), 20, 6e-2)])
def test_uvit3d_pose_backward_at_re10k_widths(blocks, mid, bar):
    """VERDICT r1 weak #4 / r2 next #5d: whole-model backward at the REAL RE10K widths -- channels 128/256/576/1152, 9 heads (d = 64 at
    level 2, d = 128 at level 3), emb 1024 -- at 64x64 frames, 8 tokens: forward and every parameter gradient vs torch autograd through the
    fp32 oracle; once at reduced depth (1+1+1 blocks, 1 mid: every gradient within 3e-2) and once at the FULL depth of the RE10K model
    (3+3+6 blocks, 20 mid: 38 residual blocks of bf16 activations between the loss and the first layers, stated bar 6e-2, median printed)."""
    from dfot_amd import uvit_train as ut
    from oracle import pose as opose, uvit as ouvit
    torch.set_num_threads(16)
    cfg = ouvit.UViTConfig(num_updown_blocks=blocks, num_mid_blocks=mid, resolution=64)   # default widths = RE10K
    assert tuple(cfg.channels) == (128, 256, 576, 1152) and cfg.num_heads == 9 and cfg.emb_channels == 1024
    params = ouvit.seeded_params(cfg, seed=12)
    g = torch.Generator().manual_seed(13)
    x = torch.randn(1, 8, 3, 64, 64, generator=g)
    k = torch.randn(1, 8, generator=g)
    pz = torch.eye(3, 4).reshape(1, 1, 12).repeat(1, 8, 1)
    pz[..., 3] = torch.linspace(0, 0.4, 8)
    cond = opose.ray_encoding(torch.cat([torch.tensor([0.5, 0.9, 0.5, 0.5]).repeat(1, 8, 1), pz], -1), 64)
    d_out = torch.randn(1, 8, 3, 64, 64, generator=g)
    tr = ut.UViT3DPoseTrainer(params, dict(channels=cfg.channels, emb_channels=cfg.emb_channels, patch_size=2, block_types=cfg.block_types,
                                           num_updown_blocks=cfg.num_updown_blocks, num_mid_blocks=cfg.num_mid_blocks, num_heads=cfg.num_heads,
                                           resolution=64, max_tokens=8))
    out = tr.forward(x, k, cond).cpu()
    grads = {n: t.cpu() for n, t in tr.backward(d_out).items()}
    ps = {n: t.clone().requires_grad_(not n.endswith(("freqs", "phases"))) for n, t in params.items()}
    ref = ouvit.forward(ps, cfg, x, k, cond)
    r_out = rel(out, ref.detach())
    (ref * d_out).sum().backward()
    names = [n for n in ps if ps[n].requires_grad]
    assert sorted(grads) == sorted(names)
    rs = {n: rel(grads[n], ps[n].grad) for n in names}
    worst = max(rs, key=rs.get)
    over = {n: round(v, 4) for n, v in rs.items() if v >= 3e-2}
    print(f"UViT3DPose backward at RE10K widths, depth {blocks}/{mid}: forward rel-L2 {r_out:.2e}; worst gradient rel-L2 {rs[worst]:.2e} at {worst}; "
          f"median {sorted(rs.values())[len(rs) // 2]:.2e}; above 3e-2: {over}")
    assert r_out < 2e-2 and rs[worst] < bar and sorted(rs.values())[len(rs) // 2] < 2e-2, (r_out, over)


def test_uvit3d_pose_input_gradient_matches_fp32_autograd():
    """d loss / d x of the autograd drop-in (ops.py: produced only when x requires it; reconstruction guidance differentiates the
    prediction w.r.t. x_t) vs torch autograd through oracle.uvit in fp32: the last step is dfot_op_embed_input_dgrad"""
    import dfot_amd
    from oracle import pose as opose, uvit as ouvit
    res = 64
    ocfg = ouvit.UViTConfig(resolution=res, num_updown_blocks=(1, 1, 1), num_mid_blocks=1)
    params = ouvit.seeded_params(ocfg, 4)
    cfg = dict(channels=list(ocfg.channels), emb_channels=ocfg.emb_channels, patch_size=2, block_types=list(ocfg.block_types),
               num_updown_blocks=list(ocfg.num_updown_blocks), num_mid_blocks=ocfg.num_mid_blocks, num_heads=ocfg.num_heads,
               pos_emb_type="rope", use_fourier_noise_embedding=True, conditioning=dict(dim=180))
    model = dfot_amd.UViT3DPose(cfg, x_shape=(3, res, res), max_tokens=8).cuda().eval()
    model.load_state_dict(params, strict=True)
    for p_ in model.parameters():
        p_.requires_grad_(False)  # sampling-time use: only x requires a gradient
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 8, 3, res, res, generator=g)
    k = torch.randn(1, 8, generator=g)
    pz = torch.eye(3, 4).reshape(1, 1, 12).repeat(1, 8, 1)
    pz[..., 3] = torch.linspace(0, 0.5, 8)
    cond = opose.ray_encoding(torch.cat([torch.tensor([0.5, 0.9, 0.5, 0.5]).repeat(1, 8, 1), pz], -1), res)
    tgt = torch.randn(1, 8, 3, res, res, generator=g)
    xr = x.clone().requires_grad_(True)
    gp = {n: t.cuda() for n, t in params.items()}
    ((ouvit.forward(gp, ocfg, xr.cuda(), k.cuda(), cond.cuda(), None).cpu() - tgt) ** 2).sum().backward()
    xe = x.clone().cuda().requires_grad_(True)
    ((model(xe, k.cuda(), cond.cuda(), None) - tgt.cuda()) ** 2).sum().backward()
    rel = ((xe.grad.cpu() - xr.grad).norm() / xr.grad.norm()).item()
    print(f"d loss / d x: rel-L2 {rel:.3e}")
    assert torch.isfinite(xe.grad).all() and rel < 3e-2


# ---------------------------------------------------------------------------------------------------------------------------------------
# round 4: the trainer's choice of the no-running-max attention kernel is safe by construction

def _attn_fwd_lse_bounded(q, k, v, bound, own_scratch=True):
    """q pre-scaled [B][H][N][64] bf16 -> (o [B][N][H*64] bf16, lse [B][H][N] fp32 log2-domain) through dfot_op_attention_fwd_lse_bounded"""
    from dfot_amd import capi
    b, h, n, d = q.shape
    o = torch.empty(b, n, h * d, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(b, h, n, dtype=torch.float32, device="cuda")
    need = int(capi.lib.dfot_op_attention_scratch_bytes(b, h, n, d)) if own_scratch else 0
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda") if need else None
    capi.check(capi.lib.dfot_op_attention_fwd_lse_bounded(capi.ptr(q), capi.ptr(k), capi.ptr(v), capi.ptr(o), h * d, capi.ptr(lse), b, h, n, d,
                                                          float(bound), capi.ptr(scratch), need, capi.stream_ptr()))
    torch.cuda.synchronize()
    return o, lse


@pytest.mark.parametrize("bound", [80.0, float("inf"), float("nan")])
def test_bounded_attention_forward_beyond_the_bound_is_exact_and_feeds_the_backward(bound):
    """scores far beyond the no-running-max range (|s| up to ~100 in the log2 domain: exp2 without a maximum overflows fp32 row sums):
    a caller that says so (bound >= 64, inf, or NaN) gets the running-max kernel -- output and log-sum-exp equal the fp64 softmax, and
    dfot_op_attention_bwd_lse on that lse gives autograd's dq / dk / dv."""
    from dfot_amd import capi
    b, h, n, d = 2, 3, 512, 64
    g = torch.Generator().manual_seed(7)
    scale = math.log2(math.e) / math.sqrt(d)
    q = (4.0 * torch.randn(b, h, n, d, generator=g))
    k = (4.0 * torch.randn(b, h, n, d, generator=g))
    v = torch.randn(b, h, n, d, generator=g)
    do = torch.randn(b, n, h * d, generator=g)
    bf = lambda t: t.to(torch.bfloat16)
    qs, kb, vb = bf(q * scale).cuda(), bf(k).cuda(), bf(v).cuda()
    s2 = qs.double() @ kb.double().transpose(-1, -2)           # log2-domain scores
    assert float(s2.abs().max()) > 70.0                         # beyond what exp2 without a running max can sum
    o, lse = _attn_fwd_lse_bounded(qs, kb, vb, bound)
    ref_lse = torch.logsumexp(s2 * math.log(2.0), -1) / math.log(2.0)
    ref_o = (torch.softmax(s2 * math.log(2.0), -1) @ vb.double()).transpose(1, 2).reshape(b, n, h * d)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    assert rel(o.float(), ref_o) < 1.5e-2 and float((lse.double() - ref_lse).abs().max()) < 2e-2
    # backward from that lse
    dod = bf(do).cuda().contiguous()
    delta = torch.empty(b, h, n, dtype=torch.float32, device="cuda")
    dq, dk, dv = (torch.full((b, h, n, d), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(3))
    capi.check(capi.lib.dfot_op_attention_bwd_lse(capi.ptr(qs), capi.ptr(kb), capi.ptr(vb), capi.ptr(o), capi.ptr(dod), h * d, capi.ptr(lse),
                                                  capi.ptr(delta), capi.ptr(dq), capi.ptr(dk), capi.ptr(dv), b, h, n, d, capi.stream_ptr()))
    torch.cuda.synchronize()
    qr = (qs.float() / scale).requires_grad_()
    kr, vr = kb.float().requires_grad_(), vb.float().requires_grad_()
    ref = (torch.softmax(qr @ kr.transpose(-1, -2) / math.sqrt(d), -1) @ vr).transpose(1, 2).reshape(b, n, h * d)
    ref.backward(dod.float())
    for name, got, want in (("dq", dq, qr.grad), ("dk", dk, kr.grad), ("dv", dv, vr.grad)):
        r = rel(got.float(), want)
        print(f"bounded attention (bound {bound}) {name}: rel {r:.2e}")
        assert torch.isfinite(got.float()).all() and r < 2.5e-2, (name, r)


def test_bounded_attention_below_the_bound_takes_the_fast_kernel_with_caller_scratch():
    """ordinary QK-normed scores (|s| < 64): the pipelined no-running-max kernel, its key-split partial rows in the CALLER's buffer
    (nothing allocated on the launch path, nothing shared between trainers); same result with the library's own block"""
    b, h, n, d = 2, 9, 1024, 64   # 72 query tiles of 256 rows on 512 slots: the tail is split over the keys -> partial rows are used
    g = torch.Generator().manual_seed(9)
    scale = math.log2(math.e) / math.sqrt(d)
    nrm = lambda t: t / t.pow(2).mean(-1, keepdim=True).sqrt()
    q, k = nrm(torch.randn(b, h, n, d, generator=g)), nrm(torch.randn(b, h, n, d, generator=g))
    v = torch.randn(b, h, n, d, generator=g)
    qs, kb, vb = (q * scale).to(torch.bfloat16).cuda(), k.to(torch.bfloat16).cuda(), v.to(torch.bfloat16).cuda()
    s2 = qs.double() @ kb.double().transpose(-1, -2)
    o, lse = _attn_fwd_lse_bounded(qs, kb, vb, 13.0, own_scratch=True)
    o2, lse2 = _attn_fwd_lse_bounded(qs, kb, vb, 13.0, own_scratch=False)
    ref_o = (torch.softmax(s2 * math.log(2.0), -1) @ vb.double()).transpose(1, 2).reshape(b, n, h * d)
    ref_lse = torch.logsumexp(s2 * math.log(2.0), -1) / math.log(2.0)
    assert rel(o.float(), ref_o) < 1.5e-2 and float((lse.double() - ref_lse).abs().max()) < 2e-2
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


def _re10k_width_trainer(seed=21):
    from dfot_amd import uvit_train as ut
    from oracle import pose as opose, uvit as ouvit
    cfg = ouvit.UViTConfig(num_updown_blocks=(1, 1, 1), num_mid_blocks=1, resolution=64)   # RE10K widths: level 2 has d = 64
    params = ouvit.seeded_params(cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(1, 8, 3, 64, 64, generator=g)
    k = torch.randn(1, 8, generator=g)
    pz = torch.eye(3, 4).reshape(1, 1, 12).repeat(1, 8, 1)
    pz[..., 3] = torch.linspace(0, 0.4, 8)
    cond = opose.ray_encoding(torch.cat([torch.tensor([0.5, 0.9, 0.5, 0.5]).repeat(1, 8, 1), pz], -1), 64)
    tcfg = dict(channels=cfg.channels, emb_channels=cfg.emb_channels, patch_size=2, block_types=cfg.block_types, num_updown_blocks=cfg.num_updown_blocks,
                num_mid_blocks=cfg.num_mid_blocks, num_heads=cfg.num_heads, resolution=64, max_tokens=8)
    return ut, ouvit, cfg, params, tcfg, x, k, cond


def _true_bound(blk):
    d = blk.d
    wq, wk = (blk.p[n].abs().view(d // 2, 2).amax(-1) for n in ("q_norm.weight", "k_norm.weight"))
    return float((wq * wk).max()) * math.sqrt(d) * math.log2(math.e)


def test_trainer_score_bound_follows_an_external_weight_change_at_once():
    """q_norm / k_norm weights scaled up in a LIVE trainer (what a checkpoint load or the autograd drop-in
    after load_state_dict does: copy into trainer.p, then sync()).  The bound the blocks hold must be the NEW weights' bound before the
    next forward is issued (>= 64 here: running-max kernel), and that forward must match the oracle on the new weights."""
    ut, ouvit, cfg, params, tcfg, x, k, cond = _re10k_width_trainer()
    tr = ut.UViT3DPoseTrainer(params, tcfg)
    d64 = [b for b in tr._blocks() if isinstance(b, ut.TransformerBlockTrain) and b.d == 64]
    assert d64 and all(b.score_bound < 64 and b.score_bound >= _true_bound(b) for b in d64)
    out0 = tr.forward(x, k, cond).cpu()
    assert rel(out0, ouvit.forward(params, cfg, x, k, cond)) < 2e-2
    # x2.4 on both norms = x5.76 on the scores: bound ~ 75 >= 64.  (x4 each = x16 makes the softmax so peaked that bf16 q / k rounding
    # alone costs 2.6e-2 against the fp32 oracle -- finite and on the running-max kernel, but no longer a 2e-2 comparison)
    new = {n: (t * 2.4 if n.endswith(("q_norm.weight", "k_norm.weight")) else t.clone()) for n, t in params.items()}
    with torch.no_grad():
        for n, t in new.items():
            tr.p[n].copy_(t)
    tr.sync()                                   # external change: exact bound, read back synchronously
    assert all(b.score_bound >= 64 and b.score_bound >= _true_bound(b) for b in d64), [b.score_bound for b in d64]
    out1 = tr.forward(x, k, cond).cpu()
    ref1 = ouvit.forward(new, cfg, x, k, cond)
    r = rel(out1, ref1)
    print(f"trainer forward right after a x2.4 q/k-norm change: rel-L2 {r:.2e} (bound {d64[0].score_bound:.1f})")
    assert torch.isfinite(out1).all() and r < 2e-2
    # ... and the backward that follows consumes the running-max kernel's lse
    grads = tr.backward(torch.randn(1, 8, 3, 64, 64, generator=torch.Generator().manual_seed(3)))
    assert all(torch.isfinite(gr).all() for gr in grads.values())


def test_trainer_score_bound_is_an_upper_bound_through_its_own_optimizer_steps():
    """the trainer's own AdamW steps never read the device: the host adds the largest move an Adam step can make to every |w|.  After a few
    deliberately LARGE steps (lr 2e-2) the bound each block holds is still >= the true bound of its current weights, with no exact read
    in between; the periodic exact read resets the drift."""
    ut, ouvit, cfg, params, tcfg, x, k, cond = _re10k_width_trainer(seed=31)
    tr = ut.UViT3DPoseTrainer(params, tcfg)
    d64 = [b for b in tr._blocks() if isinstance(b, ut.TransformerBlockTrain) and b.d == 64]
    reads0 = tr.bound_exact_reads
    g = torch.Generator().manual_seed(5)
    for step in range(4):
        tr.forward(x, k, cond)
        tr.backward(torch.randn(1, 8, 3, 64, 64, generator=g))
        tr.optimizer_step(lr=2e-2, betas=(0.9, 0.99), weight_decay=0.01, max_grad_norm=1.0)
        for b in d64:
            true = _true_bound(b)
            assert b.score_bound >= true, (step, b.score_bound, true)
    assert tr.bound_exact_reads == reads0 and tr._bound_drift > 0     # no device read on the trainer's own steps
    tr.sync()                                                           # an external sync re-reads exactly
    assert tr.bound_exact_reads == reads0 + 1 and tr._bound_drift == 0.0
    assert all(0 <= b.score_bound - _true_bound(b) < 1e-3 * b.score_bound for b in d64)


def test_drop_in_forward_after_load_state_dict_uses_the_new_weights_bound():
    """one training forward on the initial weights, then load_state_dict with q/k-norm weights x2.4 (bound >= 64), then
    the next training forward: it must run the running-max kernel (finite, oracle-matching), not the stale fast choice."""
    import dfot_amd
    ut, ouvit, cfg, params, tcfg, x, k, cond = _re10k_width_trainer(seed=41)
    bcfg = dict(channels=list(cfg.channels), emb_channels=cfg.emb_channels, patch_size=2, block_types=list(cfg.block_types),
                num_updown_blocks=list(cfg.num_updown_blocks), num_mid_blocks=cfg.num_mid_blocks, num_heads=cfg.num_heads, pos_emb_type="rope",
                use_fourier_noise_embedding=True, conditioning=dict(dim=180))
    model = dfot_amd.UViT3DPose(bcfg, x_shape=(3, 64, 64), max_tokens=8).cuda()
    model.load_state_dict(params, strict=True)
    model.train()
    xd, kd, cd = x.cuda(), k.cuda(), cond.cuda()
    v0 = model(xd, kd, cd)
    v0.sum().backward()
    new = {n: (t * 2.4 if n.endswith(("q_norm.weight", "k_norm.weight")) else t.clone()) for n, t in params.items()}
    model.load_state_dict(new, strict=True)
    v1 = model(xd, kd, cd)
    d64 = [b for b in model._trainer._blocks() if isinstance(b, ut.TransformerBlockTrain) and b.d == 64]
    assert all(b.score_bound >= 64 for b in d64)
    r = rel(v1.detach().cpu(), ouvit.forward(new, cfg, x, k, cond))
    print(f"drop-in forward after load_state_dict (q/k-norm x2.4): rel-L2 {r:.2e}")
    assert torch.isfinite(v1).all() and r < 2e-2
    v1.sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())


# ---------------------------------------------------------------------------------------------------------------------------------------
# round 4: BASELINE config 5 pinned at (nearly) its real size

@pytest.mark.timeout(900)
def test_attention_backward_at_the_level2_launch_shape_of_config5():
    """dfot_op_attention_fwd_lse_bounded + dfot_op_attention_bwd_lse at (B * H, N, d) = (72, 8192, 64): the launch shape of the level-2
    blocks in the 8 videos x 8 frames x 256 x 256 training step (attn_bwd_dkv_kernel<64,64,64> / attn_bwd_dq_kernel over 128-key tiles x 72
    head-batches, the forward's key-split tail).  Reference: fp32 softmax attention under autograd on the GPU, one (video, head) at a
    time (a 8192 x 8192 fp32 score matrix each) on the same bf16-rounded operands."""
    from dfot_amd import capi
    b, h, n, d = 8, 9, 8192, 64
    g = torch.Generator(device="cuda").manual_seed(17)
    scale = math.log2(math.e) / math.sqrt(d)
    nrm = lambda t: t / t.pow(2).mean(-1, keepdim=True).sqrt()
    q = nrm(torch.randn(b, h, n, d, device="cuda", generator=g)) * (1 + 0.1 * torch.randn(d, device="cuda", generator=g))
    k = nrm(torch.randn(b, h, n, d, device="cuda", generator=g)) * (1 + 0.1 * torch.randn(d, device="cuda", generator=g))
    v = torch.randn(b, h, n, d, device="cuda", generator=g)
    do = torch.randn(b, n, h * d, device="cuda", generator=g).to(torch.bfloat16)
    qs, kb, vb = (q * scale).to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16)
    o, lse = _attn_fwd_lse_bounded(qs, kb, vb, 20.0)
    delta = torch.empty(b, h, n, dtype=torch.float32, device="cuda")
    dq, dk, dv = (torch.full((b, h, n, d), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(3))
    capi.check(capi.lib.dfot_op_attention_bwd_lse(capi.ptr(qs), capi.ptr(kb), capi.ptr(vb), capi.ptr(o), capi.ptr(do), h * d, capi.ptr(lse),
                                                  capi.ptr(delta), capi.ptr(dq), capi.ptr(dk), capi.ptr(dv), b, h, n, d, capi.stream_ptr()))
    torch.cuda.synchronize()
    num = {x: 0.0 for x in ("o", "dq", "dk", "dv", "lse")}
    den = dict(num)
    dov = do.float().view(b, n, h, d)
    for bi in range(b):
        for hi in range(h):
            qr = (qs[bi, hi].float() / scale).requires_grad_()
            kr, vr = kb[bi, hi].float().requires_grad_(), vb[bi, hi].float().requires_grad_()
            s = qr @ kr.t() / math.sqrt(d)
            ref = torch.softmax(s, -1) @ vr
            ref.backward(dov[bi, :, hi])
            ref_lse = torch.logsumexp(s.detach().double(), -1) / math.log(2.0)
            for name, got, want in (("o", o.view(b, n, h, d)[bi, :, hi], ref.detach()), ("dq", dq[bi, hi], qr.grad), ("dk", dk[bi, hi], kr.grad),
                                    ("dv", dv[bi, hi], vr.grad), ("lse", lse[bi, hi], ref_lse)):
                num[name] += float((got.double() - want.double()).pow(2).sum())
                den[name] += float(want.double().pow(2).sum())
            del s, ref, qr, kr, vr
    rs = {x: math.sqrt(num[x] / den[x]) for x in num}
    print("attention fwd/bwd at (72, 8192, 64): rel-L2 " + ", ".join(f"{x} {r:.2e}" for x, r in rs.items()))
    assert all(torch.isfinite(t.float()).all() for t in (o, dq, dk, dv))
    assert rs["o"] < 1.5e-2 and rs["lse"] < 1e-3 and max(rs["dq"], rs["dk"], rs["dv"]) < 2e-2, rs


@pytest.mark.timeout(1800)
def test_uvit3d_pose_training_step_at_config5_frame_size_full_depth():
    """BASELINE config 5 nearer its real size (continuous_diffusion.py:140-167, realestate10k_video_generation.yaml:44,49-51): the RE10K
    model at FULL depth (3+3+6 / 20 blocks), 256 x 256 frames, 8 frames, batch 2 -- every kernel of the training step at its production
    launch geometry per video (level-0 GroupNorm over 16384-pixel images, 113-slice convolution weight gradients, N = 8192 attention
    backward) -- with level-3 checkpointing as in the recipe.  Engine loss and every parameter gradient vs torch autograd through
    oracle.uvit in fp32 ON THE GPU (fused SDPA, every block under torch.utils.checkpoint so that it fits).  Bars: loss 1e-2 relative;
    gradients worst <= 3e-2, median <= 1.5e-2 relative L2 (bf16 activations through 38 residual blocks; measured 1.7e-2 / 7.9e-3, printed)."""
    from dfot_amd import uvit_train as ut
    from oracle import pose as opose, sampler as osm, uvit as ouvit
    res, batch = 256, 2
    cfg = ouvit.UViTConfig(resolution=res)   # defaults = the RE10K model
    assert tuple(cfg.channels) == (128, 256, 576, 1152) and tuple(cfg.num_updown_blocks) == (3, 3, 6) and cfg.num_mid_blocks == 20
    params = ouvit.seeded_params(cfg, seed=14)
    g = torch.Generator().manual_seed(15)
    xs = torch.randn(batch, 8, 3, res, res, generator=g)
    noise = torch.randn(batch, 8, 3, res, res, generator=g)
    t = torch.rand(batch, 8, generator=g)
    pz = torch.eye(3, 4).reshape(1, 1, 12).repeat(batch, 8, 1)
    pz[..., 3] = torch.linspace(0, 0.4, 8)
    pz[1, :, 7] = 0.1
    cond = opose.ray_encoding(torch.cat([torch.tensor([0.5, 0.9, 0.5, 0.5]).repeat(batch, 8, 1), pz], -1), res)
    tr = ut.UViT3DPoseTrainer(params, dict(channels=cfg.channels, emb_channels=cfg.emb_channels, patch_size=2, block_types=cfg.block_types,
                                           num_updown_blocks=cfg.num_updown_blocks, num_mid_blocks=cfg.num_mid_blocks, num_heads=cfg.num_heads,
                                           resolution=res, max_tokens=8, use_checkpointing=[False, False, False, True]))
    loss = float(tr.loss_and_grads(xs, cond.cuda(), t, noise).item())
    grads = {n: tr._view(n, tr.flat_grads).detach().clone() for n in tr.layout}
    torch.cuda.synchronize()
    # fp32 autograd through the oracle on the GPU
    old = (ouvit.USE_SDPA, ouvit.CHECKPOINT_BLOCKS, torch.backends.cuda.matmul.allow_tf32)
    ouvit.USE_SDPA, ouvit.CHECKPOINT_BLOCKS, torch.backends.cuda.matmul.allow_tf32 = True, True, False
    try:
        ps = {n: v.cuda().requires_grad_(not n.endswith(("freqs", "phases"))) for n, v in params.items()}
        _, per_el = osm.training_loss(lambda x, lv, c, m: ouvit.forward(ps, cfg, x, lv, c), xs.cuda(), cond.cuda(), t.cuda(), noise.cuda())
        ref_loss = per_el.mean()
        ref_loss.backward()
        ref_loss = ref_loss.detach()
    finally:
        ouvit.USE_SDPA, ouvit.CHECKPOINT_BLOCKS, torch.backends.cuda.matmul.allow_tf32 = old
    names = [n for n in ps if ps[n].requires_grad]
    assert sorted(grads) == sorted(names)
    rs = {n: rel(grads[n].reshape(ps[n].shape), ps[n].grad) for n in names}
    worst = max(rs, key=rs.get)
    med = sorted(rs.values())[len(rs) // 2]
    over = {n: round(v, 4) for n, v in rs.items() if v >= 3e-2}
    print(f"config 5 at {res}x{res}, batch {batch}, full depth: loss {loss:.6f} vs oracle {float(ref_loss):.6f}; gradient rel-L2 worst {rs[worst]:.2e} at "
          f"{worst}, median {med:.2e}; above 3e-2: {over}")
    assert abs(loss - float(ref_loss)) < 1e-2 * abs(float(ref_loss))
    assert rs[worst] < 3e-2 and med < 1.5e-2, (worst, rs[worst], med)
