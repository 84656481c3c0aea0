"""GPU tests of FacDiT training (DiT3D, variant "factorized_attention", pos_emb_type "sinusoidal_factorized"): the backward of the temporal
attention at the op level, the trainer's forward and every parameter gradient against fp32 autograd through the host restatement, the
reference's own training step (tests/golden/dit_fac_train.npz, tools/make_golden_dit_fac_train.py), and the trainer's mechanics.

Bars (the ones tests/test_gpu_dit_facmat_train.py:6-12 cites for the same quantities): the op against fp64 autograd rel-L2 < 2e-2 for each
of dq, dk, dv (tests/test_gpu_train.py:52, the flash-attention backward); the forward rel-L2 < 2e-2 and every parameter gradient rel-L2 <
5e-2 against autograd (test_difference_dit_backward_matches_autograd); against the reference's fixture loss within 2e-2, every gradient norm
within 3e-2, stored tensors rel-L2 < 5e-2 (test_training_gradients_vs_reference_fixture); accumulation rel < 2e-2
(test_difference_training_step_loss_and_accumulation).  The optimizer step is compared with torch.optim.AdamW on the ENGINE's gradients, so
both sides do the same fp32 arithmetic on the same numbers: the update (new - old, ~1e-3 of weights ~1e-1) carries the weights' fp32
rounding, ~1e-7 * 1e-1 / 1e-3 = 1e-5 relative; the bar is 1e-3.

What a trainer measures whose temporal attention backward were skipped (dq = dk = dv = 0 in the temporal blocks), computed on the host with
dit_fac_train_common.skipped_temporal_backward at the input of test_backward_matches_autograd: the gradients of every temporal attn.qkv
weight and bias are zero (rel-L2 1.0), 34 of the 46 parameter gradients of case mlp0 and 46 of the 58 of case mlp4 miss the 5e-2 bar, and
the input gradient of test_gradient_crosses_frames_only_through_the_temporal_attention is exactly zero on frames 0-3 where autograd gives a
norm of 2.44 (of 17.6 for the whole input).

Every test here fails on the parent commit: its library exports neither symbol and its package has no FacDiTTrainer."""
import math

import pytest
import torch

import dit_fac_common as fc
import dit_fac_train_common as ft
from dit_fac_common import T, rel

pytestmark = pytest.mark.gpu

OP_BAR = 2e-2
FWD_BAR = 2e-2
GRAD_BAR = 5e-2
PATCHES, HEADS = 128, 2


# ---------------------------------------------------------------------------------------------------------------- the kernel
def _case(tokens, d, batch, seed=3):
    """bf16-rounded unit-normal q, k, v [(b t)][heads][P][d] and d_o [(b t p)][heads*d] on the host"""
    g = torch.Generator().manual_seed(seed + 1000 * tokens + d)
    q, k, v = (torch.randn(batch * tokens, HEADS, PATCHES, d, generator=g).to(torch.bfloat16).float() for _ in range(3))
    d_o = torch.randn(batch * tokens * PATCHES, HEADS * d, generator=g).to(torch.bfloat16).float()
    return q, k, v, d_o


def _device(q, k, v, d):
    """operands as the per-frame QKV epilogue leaves them: rows of dstride elements, q scaled into the exp2 domain, pads zero"""
    ds = 64 if d <= 64 else 128

    def pad(t, mul=1.0):
        out = torch.zeros(*t.shape[:-1], ds, dtype=torch.bfloat16, device="cuda")
        out[..., :d] = (t * mul).to(torch.bfloat16).cuda()
        return out
    return pad(q, math.log2(math.e) / math.sqrt(d)), pad(k), pad(v)


def _run_bwd(host, tokens, d, batch, tail=0):
    """(dq, dk, dv) [(b t) + tail][heads][P][dstride] of the op, started as NaN; the `tail` extra frames after the end hold 7.0"""
    from dfot_amd import capi
    q, k, v, d_o = host
    dev = _device(q, k, v, d)
    gd = d_o.to(torch.bfloat16).cuda()
    outs = []
    for _ in range(3):
        t = torch.full((batch * tokens + tail, HEADS, PATCHES, dev[0].shape[-1]), float("nan"), dtype=torch.bfloat16, device="cuda")
        t[batch * tokens:] = 7.0
        outs.append(t)
    capi.check(capi.lib.dfot_op_attention_temporal_bwd(capi.ptr(dev[0]), capi.ptr(dev[1]), capi.ptr(dev[2]), capi.ptr(gd), HEADS * d, capi.ptr(outs[0]),
                                                       capi.ptr(outs[1]), capi.ptr(outs[2]), batch, tokens, PATCHES, HEADS, d, capi.stream_ptr()))
    torch.cuda.synchronize()
    return outs


def _ref_bwd(host, tokens, d, batch):
    """fp64 autograd through softmax(q k^T / sqrt(d)) v over the frames of every (video, head, patch): (dq, dk, dv) in the layout of q"""
    q, k, v, d_o = host
    leaves = [t.double().reshape(batch, tokens, HEADS, PATCHES, d).requires_grad_() for t in (q, k, v)]
    qq, kk, vv = (t.permute(0, 2, 3, 1, 4) for t in leaves)  # b h p t d
    o = torch.softmax(qq @ kk.transpose(-1, -2) / math.sqrt(d), -1) @ vv
    go = d_o.double().reshape(batch, tokens, PATCHES, HEADS, d).permute(0, 3, 2, 1, 4)
    (o * go).sum().backward()
    return [t.grad.reshape(batch * tokens, HEADS, PATCHES, d) for t in leaves]


@pytest.mark.parametrize("d", [32, 64, 72])
@pytest.mark.parametrize("tokens", [1, 2, 3, 5, 16, 17, 32])
def test_attention_temporal_backward_vs_fp64(tokens, d):
    """dstride 64 and 128, a T below, at and above each bound the kernel is compiled for (4, 8, 16, 32), a d that does not fill its dstride;
    batch 2, 2 heads, 128 patches (several workgroups per (video, head)).  One frame is the degenerate case: the softmax is the constant 1,
    so dq = dk = 0 and dv = d_o exactly."""
    batch = 2
    host = _case(tokens, d, batch)
    got = [t.float().cpu() for t in _run_bwd(host, tokens, d, batch)]
    for t in got:
        assert torch.isfinite(t[..., :d]).all()          # the outputs started as NaN: every live element was written ...
        assert torch.isnan(t[..., d:]).all()              # ... and no pad column was
    got = [t[..., :d] for t in got]
    if tokens == 1:
        assert bool((got[0] == 0).all()) and bool((got[1] == 0).all())
        d_o = host[3].reshape(batch, PATCHES, HEADS, d).permute(0, 2, 1, 3)
        assert torch.equal(got[2], d_o)
        return
    ref = _ref_bwd(host, tokens, d, batch)
    r = [rel(a, b) for a, b in zip(got, ref)]
    print(f"temporal attention backward T={tokens} d={d}: rel-L2 dq {r[0]:.2e} dk {r[1]:.2e} dv {r[2]:.2e}")
    assert max(r) < OP_BAR, r


@pytest.mark.parametrize("tokens,d", [(5, 72), (17, 64)])
def test_attention_temporal_backward_bits_do_not_depend_on_the_batch_or_the_run(tokens, d):
    """the second video alone gives the bits it gives in a batch of two; two runs are bit-identical (fixed summation order, no atomics)"""
    host = _case(tokens, d, 2)
    both, again = _run_bwd(host, tokens, d, 2), _run_bwd(host, tokens, d, 2)
    alone = _run_bwd((host[0][tokens:], host[1][tokens:], host[2][tokens:], host[3][tokens * PATCHES:]), tokens, d, 1)
    for a, b, c in zip(both, again, alone):
        assert torch.equal(a[..., :d].view(torch.int16), b[..., :d].view(torch.int16))
        assert torch.equal(a[tokens:, ..., :d].view(torch.int16), c[..., :d].view(torch.int16))


def test_attention_temporal_backward_invalid_shapes_launch_nothing():
    from dfot_amd import capi
    n = 2 * 33 * 2 * 128 * 128
    z = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    outs = [torch.full((n,), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(3)]

    def call(ldo, batch, tokens, patches, heads, d, ptrs=None):
        q, k, v, g, dq, dk, dv = ptrs or [capi.ptr(z)] * 4 + [capi.ptr(t) for t in outs]
        return capi.lib.dfot_op_attention_temporal_bwd(q, k, v, g, ldo, dq, dk, dv, batch, tokens, patches, heads, d, capi.stream_ptr())
    #            ldo  batch T  patches heads d
    for args in ((128, 2, 0, 128, 2, 64), (128, 2, 33, 128, 2, 64), (72, 2, 4, 128, 2, 36), (272, 2, 4, 128, 2, 136), (128, 2, 4, 64, 2, 64),
                 (120, 2, 4, 128, 2, 64), (132, 2, 4, 128, 2, 64), (128, 0, 4, 128, 2, 64), (128, 2, 4, 128, 0, 64), (128, 65536, 4, 128, 2, 64),
                 (128, 2, -1, 128, 2, 64), (128, 2, 4, 192, 2, 64)):
        assert call(*args) == capi.ERR_SHAPE, args
        assert capi.lib.dfot_last_error()
    good = [capi.ptr(z)] * 4 + [capi.ptr(t) for t in outs]
    for i in range(7):  # a null pointer in every position
        assert call(128, 2, 4, 128, 2, 64, good[:i] + [None] + good[i + 1:]) == capi.ERR_ARG, i
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs) and bool((z == 0).all())  # nothing was launched
    assert call(128, 2, 4, 128, 2, 64) == capi.OK
    torch.cuda.synchronize()
    live = 2 * 4 * 2 * 128 * 64
    for t in outs:  # q = k = v = d_o = 0 -> zero gradients, and nothing past the end
        assert bool((t[:live] == 0).all()) and bool(torch.isnan(t[live:]).all())


@pytest.mark.parametrize("tokens,d", [(17, 72), (32, 64), (3, 32)])
def test_attention_temporal_backward_writes_nothing_past_the_end(tokens, d):
    """two sentinel frames (2 heads x 128 patches x dstride each) after the end of dq, dk and dv stay as they were"""
    host = _case(tokens, d, 2)
    for t in _run_bwd(host, tokens, d, 2, tail=2):
        assert bool((t[2 * tokens:] == 7.0).all()) and torch.isfinite(t[: 2 * tokens, ..., :d].float()).all()


# ---------------------------------------------------------------------------------------------------------------- the whole model
def _autograd(tag, x, k, d_out, cond=None, mask=None, want_dx=False):
    ps = {n: t.clone().requires_grad_() for n, t in ft.case_params(tag, cond is not None).items()}
    xx = x.clone().requires_grad_(want_dx)
    out = fc.forward_host(ps, xx, k, cond, mask, dtype=torch.float32)
    (out * d_out).sum().backward()
    grads = {n: t.grad for n, t in ps.items()}
    return (out.detach(), grads, xx.grad) if want_dx else (out.detach(), grads)


def _check(label, tr, out, ref_out, ref_grads):
    r = rel(out.cpu(), ref_out)
    grads = {n: t.cpu() for n, t in tr.grad_dict().items()}
    assert list(grads) == list(ref_grads)
    worst = ("", 0.0)
    for n, gref in ref_grads.items():
        assert torch.isfinite(grads[n]).all(), n
        assert float(gref.norm()) > 0, n
        rg = rel(grads[n], gref)
        if rg > worst[1]:
            worst = (n, rg)
    print(f"FacDiT training {label}: forward rel-L2 {r:.2e}, worst gradient rel-L2 {worst[1]:.2e} at {worst[0]}")
    assert r < FWD_BAR
    for n, gref in ref_grads.items():
        assert rel(grads[n], gref) < GRAD_BAR, (n, rel(grads[n], gref))


@pytest.mark.parametrize("tag", list(ft.TRAIN_CASES))
def test_backward_matches_autograd(tag):
    """with and without the spatial MLP; (B, T) = (2, 5), (1, 5), (2, 3): a single video, and a short input on the first rows of the longer
    temporal table.  A skipped temporal backward misses the bar on 34 of 46 (mlp0) / 46 of 58 (mlp4) gradients (module docstring)."""
    tr, _ = ft.trainer(tag)
    g = torch.Generator().manual_seed(31)
    for b, t in ((2, 5), (1, 5), (2, 3)):
        x = torch.randn(b, t, 4, 16, 8, generator=g)
        k = torch.randint(0, 1000, (b, t), generator=g)
        d_out = torch.randn(b, t, 4, 16, 8, generator=g)
        out = tr.forward(x, k)
        tr.backward(d_out)
        _check(f"{tag} B={b} T={t}", tr, out, *_autograd(tag, x, k, d_out))


def test_action_conditioned_backward_matches_autograd():
    """case mlp0 with actions and the per-video mask (video 0 runs without its condition): the condition embedding's gradients included"""
    tr, _ = ft.trainer("mlp0", cond=True)
    g = torch.Generator().manual_seed(32)
    x = torch.randn(2, 5, 4, 16, 8, generator=g)
    k = torch.randint(0, 1000, (2, 5), generator=g)
    d_out = torch.randn(2, 5, 4, 16, 8, generator=g)
    cond = torch.randn(2, 5, fc.COND_DIM, generator=g)
    mask = torch.tensor([True, False])
    out = tr.forward(x, k, cond, mask.to(torch.uint8))
    tr.backward(d_out)
    ref_out, ref_grads = _autograd("mlp0", x, k, d_out, cond, mask)
    assert any(n.startswith("external_cond_embedding") for n in ref_grads)
    _check("mlp0, action-conditioned with the per-video mask", tr, out, ref_out, ref_grads)


def test_gradient_crosses_frames_only_through_the_temporal_attention():
    """The upstream gradient lives on frame 4 alone.  The spatial blocks, the MLPs and the conditioning are per frame, so what reaches the
    INPUT of frames 0-3 came through the temporal attention's backward and nothing else: autograd gives those frames a gradient of norm 2.44
    (17.6 for the whole input), a trainer that skipped the temporal backward gives exactly zero.  The other way round: with frame 4 of the
    input changed, the gradient reaching frames 0-3 changes."""
    tr, _ = ft.trainer("mlp0")
    g = torch.Generator().manual_seed(31)
    x = torch.randn(2, 5, 4, 16, 8, generator=g)
    k = torch.randint(0, 1000, (2, 5), generator=g)
    d_out = torch.randn(2, 5, 4, 16, 8, generator=g)
    d_out[:, :4] = 0
    tr.forward(x, k)
    tr.backward(d_out)
    dx = tr.input_grad().cpu()
    _, _, ref_dx = _autograd("mlp0", x, k, d_out, want_dx=True)
    with ft.skipped_temporal_backward():
        _, _, skipped_dx = _autograd("mlp0", x, k, d_out, want_dx=True)
    assert float(skipped_dx[:, :4].norm()) == 0.0 and float(ref_dx[:, :4].norm()) > 1.0
    r03, r4 = rel(dx[:, :4], ref_dx[:, :4]), rel(dx[:, 4], ref_dx[:, 4])
    print(f"input gradient for an upstream gradient on frame 4 alone: frames 0-3 norm {float(dx[:, :4].norm()):.3f} (autograd "
          f"{float(ref_dx[:, :4].norm()):.3f}), rel-L2 {r03:.2e}; frame 4 rel-L2 {r4:.2e}")
    assert r03 < GRAD_BAR and r4 < GRAD_BAR
    x2 = x.clone()
    x2[:, 4] = 2.0 * torch.randn(2, 4, 16, 8, generator=g)
    tr.forward(x2, k)
    tr.backward(d_out)
    dx2 = tr.input_grad().cpu()
    _, _, ref_dx2 = _autograd("mlp0", x2, k, d_out, want_dx=True)
    assert rel(dx2[:, :4], dx[:, :4]) > 2 * GRAD_BAR  # frames 0-3 did not change, their gradient did
    assert rel(dx2[:, :4], ref_dx2[:, :4]) < GRAD_BAR


@pytest.mark.parametrize("tag", list(ft.TRAIN_CASES))
def test_training_gradients_vs_reference_fixture(tag):
    """loss and gradients of the reference's own training step (differentiated by the reference's autograd on CPU) vs the engine"""
    g = fc.load("dit_fac_train.npz")
    tr, params = ft.trainer(tag, loss_weighting=ft.LOSS_WEIGHTING)
    assert fc.digest(params) == str(g[f"{tag}_digest"])
    loss = tr.loss_and_grads(T(g["xs"]), T(g["k"]), T(g[f"{tag}_noise"]), T(g["masks"]))
    ref_loss = float(g[f"{tag}_loss"])
    print(f"{tag}: loss {float(loss.item()):.6f}, reference {ref_loss:.6f}")
    assert abs(float(loss.item()) - ref_loss) < 2e-2 * abs(ref_loss)
    grads = {n: t.cpu() for n, t in tr.grad_dict().items()}
    names = [str(n) for n in g[f"{tag}_names"]]
    assert names == list(grads)
    worst_norm = 0.0
    for n, ref_norm in zip(names, g[f"{tag}_norms"]):
        worst_norm = max(worst_norm, abs(float(grads[n].norm()) - ref_norm) / ref_norm)
    print(f"{tag}: worst gradient-norm deviation vs the reference {worst_norm:.2e}")
    for n, ref_norm in zip(names, g[f"{tag}_norms"]):
        assert abs(float(grads[n].norm()) - ref_norm) <= 3e-2 * ref_norm + 1e-7, (n, float(grads[n].norm()), ref_norm)
    worst = 0.0
    for key in g.files:
        if key.startswith(f"{tag}_grad/"):
            worst = max(worst, rel(grads[key.split("/", 1)[1]], T(g[key])))
    print(f"{tag}: worst stored-gradient rel-L2 vs the reference {worst:.2e}")
    assert worst < 5e-2


# ---------------------------------------------------------------------------------------------------------------- trainer mechanics
def _batch(b, seed):
    g = torch.Generator().manual_seed(seed)
    masks = torch.ones(b, 5)
    masks[0, 4] = 0
    return (torch.randn(b, 5, 4, 16, 8, generator=g), torch.randint(0, 1000, (b, 5), generator=g), torch.randn(b, 5, 4, 16, 8, generator=g), masks)


def test_accumulation_equals_one_batch_and_gradients_are_bit_reproducible():
    tr, _ = ft.trainer("mlp4", loss_weighting=ft.LOSS_WEIGHTING)
    xs, k, noise, masks = _batch(4, 41)
    tr.loss_and_grads(xs, k, noise, masks)
    full = tr.grads.clone()
    tr.loss_and_grads(xs, k, noise, masks)
    assert torch.equal(tr.grads.view(torch.int32), full.view(torch.int32))  # two runs, the same bits
    for sl in (slice(0, 2), slice(2, 4)):  # two micro-batches of 2 videos = the mean of their gradients = the gradient of the 4-video batch
        tr.loss_and_grads(xs[sl], k[sl], noise[sl], masks[sl])
        tr.accumulate()
    acc = tr._acc / tr._acc_n
    r = rel(acc.cpu(), full.cpu())
    print(f"two accumulated micro-batches vs the 4-video batch: rel-L2 {r:.2e}")
    assert r < 2e-2


def test_training_step_equals_torch_adamw_on_the_engines_gradients():
    tr, params = ft.trainer("mlp0", loss_weighting=ft.LOSS_WEIGHTING)
    tr.lr, tr.weight_decay, tr.max_grad_norm = 1e-3, 0.01, 1.0
    tr.enable_ema(0.9)
    xs, k, noise, masks = _batch(2, 42)
    loss = tr.training_step(xs, k, noise, masks)
    assert math.isfinite(float(loss.item())) and tr.step_count == 1
    new = {n: t.cpu() for n, t in tr.state_dict().items()}
    ps = {n: t.clone().requires_grad_() for n, t in params.items()}
    for n, gr in tr.grad_dict().items():  # the gradient buffer is left as the step used it (unclipped)
        ps[n].grad = gr.cpu()
    plist = list(ps.values())
    torch.nn.utils.clip_grad_norm_(plist, 1.0)
    torch.optim.AdamW(plist, lr=1e-3, weight_decay=0.01, betas=(0.9, 0.99), eps=1e-8).step()
    worst = max(rel(new[n] - params[n], t.detach() - params[n]) for n, t in ps.items())
    print(f"one step vs torch.optim.AdamW on the engine's gradients: worst update rel-L2 {worst:.2e}")
    assert worst < 1e-3
    torch.testing.assert_close(tr.ema.cpu(), 0.9 * tr_flat(params, tr) + 0.1 * tr.params.cpu(), rtol=1e-6, atol=1e-7)
    # the optimizer state exports in torch's layout and reloads into a fresh trainer, which then takes the same next step
    sd = tr.optimizer_state_dict()
    tr2, _ = ft.trainer("mlp0", loss_weighting=ft.LOSS_WEIGHTING)
    tr2.load_state_dict(tr.state_dict())
    tr2.load_optimizer_state_dict(sd)
    tr2.max_grad_norm = 1.0
    assert tr2.step_count == 1 and tr2.lr == 1e-3
    tr.ema = None
    tr.training_step(xs, k, noise, masks)
    tr2.training_step(xs, k, noise, masks)
    torch.testing.assert_close(tr2.params, tr.params, rtol=1e-5, atol=1e-6)


def tr_flat(params, tr):
    flat = torch.zeros(tr.numel)
    for name, (off, shape) in tr.layout.items():
        flat[off: off + params[name].numel()] = params[name].reshape(-1)
    return flat


def test_facdit_train_create_builds_variant_2_only():
    from dfot_amd import capi
    tr, _ = ft.trainer("mlp0")

    def config(**over):
        c = capi.DiTConfigF()
        for f, _ in capi.DiTConfig._fields_:
            setattr(c, f, getattr(tr._ccfg, f))
        for f, v in over.items():
            setattr(c, f, v)
        return c
    for variant in (0, 1, 3):
        handle = capi.C.c_void_p()
        assert capi.lib.dfot_facdit_train_create(capi.C.byref(config(variant=variant)), capi.C.byref(handle)) == capi.ERR_ARG
        assert b"variant 2" in capi.lib.dfot_last_error() and not handle.value
    handle = capi.C.c_void_p()
    assert capi.lib.dfot_facdit_train_create(capi.C.byref(config(fourier_noise=1)), capi.C.byref(handle)) == capi.ERR_ARG  # a follow-up
    assert b"fourier_noise" in capi.lib.dfot_last_error() and not handle.value
    assert capi.lib.dfot_dit_train_create_f(capi.C.byref(config()), capi.C.byref(handle)) == capi.ERR_ARG  # the refusal names the new entry
    assert b"dfot_facdit_train_create" in capi.lib.dfot_last_error() and not handle.value
