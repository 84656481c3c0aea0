"""GPU tests of FacMatDiT training (DiT3D, variant "factorized_matrix_attention", pos_emb_type "sinusoidal_2d", with and without
use_temporal_rope): the backward of the matrix attention with the temporal RoPE at the op level, the trainer's forward and every parameter
gradient against fp32 autograd through the host restatement, the reference's own training step (tests/golden/dit_facmat_train.npz,
tools/make_golden_dit_facmat_train.py), and the trainer's mechanics.

Bars (all taken from the existing training tests): the op against fp64 autograd rel-L2 < 2e-2 for each of dq, dk, dv (tests/test_gpu_train.py:52,
the flash-attention backward); the forward rel-L2 < 2e-2 and every parameter gradient rel-L2 < 5e-2 against autograd
(test_difference_dit_backward_matches_autograd); against the reference's fixture loss within 2e-2, every gradient norm within 3e-2, stored
tensors rel-L2 < 5e-2 (test_training_gradients_vs_reference_fixture); accumulation rel < 2e-2 (test_difference_training_step_loss_and_accumulation).
The optimizer step is compared with torch.optim.AdamW on the ENGINE's gradients, so both sides do the same fp32 arithmetic on the same
numbers: the update (new - old, ~1e-3 of weights ~1e-1) carries the weights' fp32 rounding, ~1e-7 * 1e-1 / 1e-3 = 1e-5 relative; the bar is
1e-3.  Every test here fails on the parent commit: its library exports neither symbol and its package has no FacMatDiTTrainer."""
import math

import pytest
import torch

import dit_facmat_common as fm
import dit_facmat_train_common as ft
from dit_facmat_common import T, rel

pytestmark = pytest.mark.gpu

OP_BAR = 2e-2
FWD_BAR = 2e-2
GRAD_BAR = 5e-2


# ---------------------------------------------------------------------------------------------------------------- the kernel
def make_do(batch, tokens, h, seed=5):
    g = torch.Generator().manual_seed(seed + 100 * tokens + h)
    return torch.randn(batch * tokens * fm.OP_E, h, generator=g).to(torch.bfloat16).float()


def _run_bwd(z, d_o, batch, tokens, h, cc, rr, table, e=fm.OP_E, tail=0):
    """dz [batch*tokens*e][3h] of the op, started as NaN; `tail` extra sentinel rows (7.0) after the end"""
    from dfot_amd import capi
    zd, gd = z.to(torch.bfloat16).cuda(), d_o.to(torch.bfloat16).cuda()
    rows = batch * tokens * e
    dz = torch.full((rows + tail, 3 * h), float("nan"), dtype=torch.bfloat16, device="cuda")
    dz[rows:] = 7.0
    scale = 1.0 / math.sqrt((e // cc) * (h // rr))
    capi.check(capi.lib.dfot_op_matrix_attention_rope_bwd(capi.ptr(zd), capi.ptr(gd), capi.ptr(table), capi.ptr(dz), batch, tokens, e, h, cc, rr,
                                                          scale, capi.stream_ptr()))
    torch.cuda.synchronize()
    return dz


def _ref_bwd(z, d_o, batch, tokens, h, cc, rr, rope, e=fm.OP_E):
    """fp64 autograd through dit_facmat_common.matrix_attention_core (fp64 angles): dz [batch*tokens*e][3h]"""
    zq = z.double().reshape(batch, tokens, e, 3 * h).requires_grad_()
    o, _ = fm.matrix_attention_core(zq, cc, rr, rope, torch.float64)
    (o * d_o.double().reshape(batch, tokens, e, h)).sum().backward()
    return zq.grad.reshape(batch * tokens * e, 3 * h)


@pytest.mark.parametrize("tokens", fm.OP_TOKENS)
def test_matrix_attention_rope_backward_vs_fp64(tokens):
    """with and without the table, at every head shape (hd in {32, 64, 72}, hn in {64, 32}); batch 2.  One frame is the degenerate case:
    the softmax is the constant 1, so dq = dk = 0 and dv = d_o exactly."""
    batch = 2
    for cc, rr, h in fm.OP_HEADS:
        z, d_o = fm.make_z(batch, tokens, cc, rr, h), make_do(batch, tokens, h)
        for rope in (True, False):
            table = fm.rope_table(tokens, h // rr).cuda() if rope else None
            got = _run_bwd(z, d_o, batch, tokens, h, cc, rr, table)
            assert torch.isfinite(got.float()).all()  # dz started as NaN: every element was written
            got = got.float().cpu()
            if tokens == 1:
                assert bool((got[:, : 2 * h] == 0).all())
                assert torch.equal(got[:, 2 * h:].to(torch.bfloat16), d_o.to(torch.bfloat16))
                continue
            ref = _ref_bwd(z, d_o, batch, tokens, h, cc, rr, rope)
            r = [rel(got[:, i * h: (i + 1) * h], ref[:, i * h: (i + 1) * h]) for i in range(3)]
            print(f"matrix attention backward L={tokens} (cc, rr, h)={(cc, rr, h)} rope={rope}: rel-L2 dq {r[0]:.2e} dk {r[1]:.2e} dv {r[2]:.2e}")
            assert max(r) < OP_BAR, r


def test_matrix_attention_backward_bits_do_not_depend_on_the_batch_or_the_run():
    """the second video alone gives the bits it gives in a batch of two; two runs are bit-identical (fixed summation order, no atomics)"""
    cc, rr, h = fm.OP_HEADS[1]
    for tokens in (5, 17):
        z, d_o = fm.make_z(2, tokens, cc, rr, h), make_do(2, tokens, h)
        table = fm.rope_table(tokens, h // rr).cuda()
        both = _run_bwd(z, d_o, 2, tokens, h, cc, rr, table)
        again = _run_bwd(z, d_o, 2, tokens, h, cc, rr, table)
        alone = _run_bwd(z[tokens * fm.OP_E:], d_o[tokens * fm.OP_E:], 1, tokens, h, cc, rr, table)
        assert torch.equal(both.view(torch.int16), again.view(torch.int16))
        assert torch.equal(both[tokens * fm.OP_E:].view(torch.int16), alone.view(torch.int16))


def test_matrix_attention_backward_uses_the_first_rows_of_a_longer_table():
    cc, rr, h = fm.OP_HEADS[2]
    z, d_o = fm.make_z(2, 5, cc, rr, h), make_do(2, 5, h)
    long = _run_bwd(z, d_o, 2, 5, h, cc, rr, fm.rope_table(32, h // rr).cuda())
    exact = _run_bwd(z, d_o, 2, 5, h, cc, rr, fm.rope_table(5, h // rr).cuda())
    assert torch.equal(long.view(torch.int16), exact.view(torch.int16))


def test_matrix_attention_backward_invalid_shapes_launch_nothing():
    from dfot_amd import capi
    z = torch.zeros(2 * 33 * 64 * 3 * 128, dtype=torch.bfloat16, device="cuda")
    d_o = torch.zeros(2 * 33 * 64 * 128, dtype=torch.bfloat16, device="cuda")
    dz = torch.full((2 * 33 * 64 * 3 * 128,), 7.0, dtype=torch.bfloat16, device="cuda")
    table = fm.rope_table(32, 32).cuda()

    def call(batch, tokens, e, h, cc, rr, zz=z, gg=d_o, out=dz):
        return capi.lib.dfot_op_matrix_attention_rope_bwd(capi.ptr(zz), capi.ptr(gg), capi.ptr(table), capi.ptr(out), batch, tokens, e, h, cc, rr, 0.01,
                                                          capi.stream_ptr())
    #            batch L  E   h    cc rr      (the argument table of tests/test_gpu_dit_facmat.py)
    for args in ((2, 0, 64, 128, 1, 4), (2, 33, 64, 128, 1, 4), (2, -1, 64, 128, 1, 4), (2, 4, 64, 128, 3, 4), (2, 4, 64, 128, 1, 3),
                 (2, 4, 64, 120, 1, 20), (0, 4, 64, 128, 1, 4), (2, 4, 0, 128, 1, 4), (2, 4, 64, 128, 0, 4), (2, 4, 64, 128, 1, 0)):
        assert call(*args) == capi.ERR_SHAPE, args
        assert capi.lib.dfot_last_error()
    for kw in (dict(zz=None), dict(gg=None), dict(out=None), dict(out=z), dict(out=d_o)):  # null pointers; dz aliasing z or d_o
        assert call(2, 4, 64, 128, 1, 4, **kw) == capi.ERR_ARG, list(kw)
    torch.cuda.synchronize()
    assert bool((dz == 7.0).all()) and bool((z == 0).all()) and bool((d_o == 0).all())  # nothing was launched
    assert call(2, 4, 64, 128, 1, 4) == capi.OK
    torch.cuda.synchronize()
    n = 2 * 4 * 64 * 3 * 128
    assert bool((dz[:n] == 0).all()) and bool((dz[n:] == 7.0).all())  # z = d_o = 0 -> dz = 0, and nothing past the end


def test_matrix_attention_backward_writes_nothing_past_the_end():
    """L = 17 (two token tiles, 15 padding rows) and hd = 72 (8-byte accesses, a partial last reduction step): 64 sentinel rows stay"""
    cc, rr, h = fm.OP_HEADS[2]
    z, d_o = fm.make_z(2, 17, cc, rr, h), make_do(2, 17, h)
    dz = _run_bwd(z, d_o, 2, 17, h, cc, rr, fm.rope_table(17, h // rr).cuda(), tail=64)
    assert bool((dz[2 * 17 * fm.OP_E:] == 7.0).all()) and torch.isfinite(dz[: 2 * 17 * fm.OP_E].float()).all()


# ---------------------------------------------------------------------------------------------------------------- the whole model
def _autograd(tag, x, k, d_out, cond=None, mask=None):
    cc, rr, bias, ratio, rope = fm.CASES[tag]
    ps = {n: t.clone().requires_grad_() for n, t in fm.case_params(tag, cond is not None).items()}
    out = fm.forward_host(ps, x, k, cc, rr, rope, cond, mask, dtype=torch.float32)
    (out * d_out).sum().backward()
    return out.detach(), {n: t.grad for n, t in ps.items()}


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
    print(f"FacMatDiT training {label}: forward rel-L2 {r:.2e}, worst gradient rel-L2 {worst[1]:.2e} at {worst[0]}")
    assert r < FWD_BAR
    for n, gref in ref_grads.items():
        assert rel(grads[n], gref) < GRAD_BAR, (n, rel(grads[n], gref))


@pytest.mark.parametrize("tag", list(fm.CASES))
def test_backward_matches_autograd(tag):
    """both head splits, with and without bias / spatial MLP / rotation (cases a-d); (B, T) = (2, 5), (1, 5), (2, 3): odd frame totals
    (the 64-row (frame, e) blocks of the factor GEMMs do not fill a 128-row tile) and a short input on a longer RoPE table"""
    tr, _ = ft.trainer(tag)
    g = torch.Generator().manual_seed(31)
    for b, t in ((2, 5), (1, 5), (2, 3)):
        x = torch.randn(b, t, 4, 16, 8, generator=g)
        k = torch.randint(0, 1000, (b, t), generator=g)
        d_out = torch.randn(b, t, 4, 16, 8, generator=g)
        out = tr.forward(x, k)
        tr.backward(d_out)
        _check(f"{tag} {fm.CASES[tag]} B={b} T={t}", tr, out, *_autograd(tag, x, k, d_out))


def test_action_conditioned_backward_matches_autograd():
    """case a with actions and the per-video mask (video 0 runs without its condition): the condition embedding's gradients included"""
    tr, _ = ft.trainer("a", cond=True)
    g = torch.Generator().manual_seed(32)
    x = torch.randn(2, 5, 4, 16, 8, generator=g)
    k = torch.randint(0, 1000, (2, 5), generator=g)
    d_out = torch.randn(2, 5, 4, 16, 8, generator=g)
    cond = torch.randn(2, 5, fm.COND_DIM, generator=g)
    mask = torch.tensor([True, False])
    out = tr.forward(x, k, cond, mask.to(torch.uint8))
    tr.backward(d_out)
    ref_out, ref_grads = _autograd("a", x, k, d_out, cond, mask)
    assert any(n.startswith("external_cond_embedding") for n in ref_grads)
    _check("a, action-conditioned with the per-video mask", tr, out, ref_out, ref_grads)


@pytest.mark.parametrize("tag", ft.TRAIN_CASES)
def test_training_gradients_vs_reference_fixture(tag):
    """loss and gradients of the reference's own training step (differentiated by the reference's autograd on CPU) vs the engine"""
    g = fm.load("dit_facmat_train.npz")
    tr, params = ft.trainer(tag, loss_weighting=ft.LOSS_WEIGHTING)
    assert fm.digest(params) == str(g[f"{tag}_digest"])
    loss = tr.loss_and_grads(T(g["xs"]), T(g["k"]), T(g[f"{tag}_noise"]), T(g["masks"]))
    ref_loss = float(g[f"{tag}_loss"])
    print(f"{tag}: loss {float(loss.item()):.6f}, reference {ref_loss:.6f}")
    assert abs(float(loss.item()) - ref_loss) < 2e-2 * abs(ref_loss)
    grads = {n: t.cpu() for n, t in tr.grad_dict().items()}
    names = [str(n) for n in g[f"{tag}_names"]]
    assert names == list(grads)
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
    tr, _ = ft.trainer("b", loss_weighting=ft.LOSS_WEIGHTING)
    xs, k, noise, masks = _batch(4, 41)
    tr.loss_and_grads(xs, k, noise, masks)
    full = tr.grads.clone()
    tr.loss_and_grads(xs, k, noise, masks)
    assert torch.equal(tr.grads.view(torch.int32), full.view(torch.int32))  # two runs, the same bits
    for sl in (slice(0, 2), slice(2, 4)):  # two micro-batches of 2 videos = the mean of their gradients = the gradient of the 4-video batch
        tr.loss_and_grads(xs[sl], k[sl], noise[sl], masks[sl])
        tr.accumulate()
    acc = tr._acc / tr._acc_n
    assert rel(acc.cpu(), full.cpu()) < 2e-2


def test_training_step_equals_torch_adamw_on_the_engines_gradients():
    tr, params = ft.trainer("a", loss_weighting=ft.LOSS_WEIGHTING)
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
    tr2, _ = ft.trainer("a", loss_weighting=ft.LOSS_WEIGHTING)
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


def test_facmat_train_create_builds_variant_3_only():
    from dfot_amd import capi
    tr, _ = ft.trainer("a")
    for variant in (0, 1):
        c = capi.DiTConfigF()
        for f, _ in capi.DiTConfig._fields_:
            setattr(c, f, getattr(tr._ccfg, f))
        c.variant = variant
        handle = capi.C.c_void_p()
        assert capi.lib.dfot_facmat_train_create(capi.C.byref(c), capi.C.byref(handle)) == capi.ERR_ARG
        assert b"variant 3" in capi.lib.dfot_last_error() and not handle.value
    c = capi.DiTConfigF()
    for f, _ in capi.DiTConfig._fields_:
        setattr(c, f, getattr(tr._ccfg, f))
    c.fourier_noise = 1
    handle = capi.C.c_void_p()
    assert capi.lib.dfot_facmat_train_create(capi.C.byref(c), capi.C.byref(handle)) == capi.ERR_ARG  # continuous training: a follow-up
    assert capi.lib.dfot_dit_train_create_f(capi.C.byref(c), capi.C.byref(handle)) == capi.ERR_ARG    # the refusal names the new entry
    assert b"dfot_facmat_train_create" in capi.lib.dfot_last_error()
