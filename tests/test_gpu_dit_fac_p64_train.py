"""GPU tests of FacDiT training at 64 patches per frame (latents 4x16x16 at patch 2, the taichi res-128 recipes): the temporal attention's
backward at 64 patches and the packed form of the 64-token attention backward at the op level, the trainer's forward and every parameter
gradient against fp32 autograd through the host restatement, the reference's own training step (tests/golden/dit_fac_p64_train.npz,
tools/make_golden_dit_fac_p64_train.py), and the trainer's mechanics and refusals.  Geometry: tests/dit_p64_common.py (hidden 128, depth 2,
4 heads, max_tokens 4).

Bars, those of tests/test_gpu_dit_fac_train.py for the same quantities: the temporal op against fp64 autograd rel-L2 < 2e-2 for each of dq,
dk, dv; the forward rel-L2 < 2e-2 and every parameter gradient rel-L2 < 5e-2 against autograd; against the reference's fixture loss within
2e-2, every gradient norm within 3e-2, stored tensors rel-L2 < 5e-2; accumulation rel < 2e-2.  The packed backward is held to EQUAL BITS
with dfot_op_dit_qkv_grad_pack (no rope table) applied to the outputs of dfot_op_attention_seq64_bwd on the same operands; its accuracy
against fp64 then is that op's (tests/test_gpu_attention_seq64_bwd_ops.py).

Checked on the CPU at exactly the inputs of test_backward_matches_autograd (generator seed 31; (B, T) = (2, 4), (1, 4), (2, 2)): no
parameter has a zero reference gradient; fp32 autograd is within 7e-7 of fp64 autograd on every gradient; a trainer that skipped the spatial
(64-token) attention backward (dit_fac_p64_train_common.skipped_spatial_backward: dq = dk = dv = 0 in the spatial blocks) would miss the
5e-2 bar on 28 of the 46 parameter gradients of case mlp0 and on 32-33 of the 58 of case mlp4, one that skipped the temporal backward on
34 of 46 and 46 of 58.

Every test here fails on the parent commit: its library exports neither dfot_op_attention_temporal_bwd_p64 nor
dfot_op_attention_seq64_bwd_packed, and its FacDiTTrainer and dfot_facdit_train_create refuse 64 patches per frame."""
import math

import pytest
import torch

import attention_seq64_bwd_common as sc
import dit_fac_common as fc
import dit_fac_p64_train_common as ft
import dit_p64_common as pc
from dit_fac_common import T, rel

pytestmark = pytest.mark.gpu

OP_BAR = 2e-2
FWD_BAR = 2e-2
GRAD_BAR = 5e-2
PATCHES, HEADS = 64, 2
MT = pc.MAX_TOKENS


# ---------------------------------------------------------------------------------------------------------------- temporal backward, P = 64
def _case(tokens, d, batch, seed=5):
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


def _run_temporal(host, tokens, d, batch, tail=2):
    """(dq, dk, dv) [(b t) + tail][heads][64][dstride] of the op, started as NaN; the `tail` extra frames after the end hold 7.0"""
    from dfot_amd import capi
    q, k, v, d_o = host
    dev = _device(q, k, v, d)
    gd = d_o.to(torch.bfloat16).cuda()
    outs = []
    for _ in range(3):
        t = torch.full((batch * tokens + tail, HEADS, PATCHES, dev[0].shape[-1]), float("nan"), dtype=torch.bfloat16, device="cuda")
        t[batch * tokens:] = 7.0
        outs.append(t)
    capi.check(capi.lib.dfot_op_attention_temporal_bwd_p64(capi.ptr(dev[0]), capi.ptr(dev[1]), capi.ptr(dev[2]), capi.ptr(gd), HEADS * d,
                                                           capi.ptr(outs[0]), capi.ptr(outs[1]), capi.ptr(outs[2]), batch, tokens, HEADS, d,
                                                           capi.stream_ptr()))
    torch.cuda.synchronize()
    return outs


def _ref_temporal(host, tokens, d, batch):
    """fp64 autograd through softmax(q k^T / sqrt(d)) v over the frames of every (video, head, patch): (dq, dk, dv) in the layout of q"""
    q, k, v, d_o = host
    leaves = [t.double().reshape(batch, tokens, HEADS, PATCHES, d).requires_grad_() for t in (q, k, v)]
    qq, kk, vv = (t.permute(0, 2, 3, 1, 4) for t in leaves)  # b h p t d
    o = torch.softmax(qq @ kk.transpose(-1, -2) / math.sqrt(d), -1) @ vv
    go = d_o.double().reshape(batch, tokens, PATCHES, HEADS, d).permute(0, 3, 2, 1, 4)
    (o * go).sum().backward()
    return [t.grad.reshape(batch * tokens, HEADS, PATCHES, d) for t in leaves]


@pytest.mark.parametrize("d", [32, 64, 72])
@pytest.mark.parametrize("tokens", [1, 2, 5, 16, 32])
def test_attention_temporal_backward_at_64_patches_vs_fp64(tokens, d):
    """dstride 64 and 128, a d that does not fill its dstride, a T in each of the kernel's compile-time bounds (4, 8, 16, 32) and an odd one;
    batch 2, 2 heads.  The launcher's PB runs from 32 (T = 1, 2: two workgroups per (video, head)) down to 1 (T = 32, d = 72).  The
    outputs start as NaN and carry two sentinel frames; the second video alone gives the bits it gives in the batch."""
    batch = 2
    host = _case(tokens, d, batch)
    outs = _run_temporal(host, tokens, d, batch)
    for t in outs:
        assert bool((t[batch * tokens:] == 7.0).all())        # nothing past the end
        live = t[: batch * tokens].float()
        assert torch.isfinite(live[..., :d]).all()            # every live element was written ...
        assert torch.isnan(live[..., d:]).all()               # ... and no pad column was
    alone = _run_temporal((host[0][tokens:], host[1][tokens:], host[2][tokens:], host[3][tokens * PATCHES:]), tokens, d, 1)
    for a, c in zip(outs, alone):
        assert torch.equal(a[tokens: 2 * tokens, ..., :d].view(torch.int16), c[:tokens, ..., :d].view(torch.int16))
    got = [t[: batch * tokens, ..., :d].float().cpu() for t in outs]
    if tokens == 1:  # the softmax is the constant 1: dq = dk = 0 and dv = d_o exactly
        assert bool((got[0] == 0).all()) and bool((got[1] == 0).all())
        d_o = host[3].reshape(batch, PATCHES, HEADS, d).permute(0, 2, 1, 3)
        assert torch.equal(got[2], d_o)
        return
    ref = _ref_temporal(host, tokens, d, batch)
    r = [rel(a, b) for a, b in zip(got, ref)]
    print(f"temporal attention backward at 64 patches T={tokens} d={d}: rel-L2 dq {r[0]:.2e} dk {r[1]:.2e} dv {r[2]:.2e}")
    assert max(r) < OP_BAR, r


# ---------------------------------------------------------------------------------------------------------------- packed backward
SLACK, TAIL_ROWS = 8, 5


def _run_packed(c, dev):
    from dfot_amd import capi
    d, nseq, heads = c["d"], c["nseq"], c["heads"]
    ldg = 3 * heads * d + SLACK
    out = torch.full((nseq * 64 + TAIL_ROWS, ldg), float("nan"), dtype=torch.bfloat16, device="cuda")
    out[nseq * 64:] = 7.0
    capi.check(capi.lib.dfot_op_attention_seq64_bwd_packed(*(capi.ptr(t) for t in dev), heads * d, capi.ptr(out), ldg, nseq, heads, d, capi.stream_ptr()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("d", [32, 64, 72, 128])
def test_packed_backward_equals_the_three_buffer_form_packed(d):
    """one instantiation per row stride and a d that does not fill it; 3 sequences x 2 heads.  The live region holds the bits
    dfot_op_dit_qkv_grad_pack makes of dfot_op_attention_seq64_bwd's outputs; the 8 slack columns of every row keep their NaN and the
    5 rows after the last one their 7.0; two runs give the same bits"""
    from dfot_amd import capi
    c = sc.make_case(d, 1.0)
    nseq, heads, ds = c["nseq"], c["heads"], sc.dstride(d)
    dev = sc.pack(c, "cuda")
    out, again = _run_packed(c, dev), _run_packed(c, dev)
    three = [torch.full((nseq, heads, 64, ds), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    capi.check(capi.lib.dfot_op_attention_seq64_bwd(*(capi.ptr(t) for t in dev), heads * d, *(capi.ptr(t) for t in three), nseq, heads, d,
                                                    capi.stream_ptr()))
    want = torch.full((nseq * 64, 3 * heads * d), float("nan"), dtype=torch.bfloat16, device="cuda")
    capi.check(capi.lib.dfot_op_dit_qkv_grad_pack(*(capi.ptr(t) for t in three), None, capi.ptr(want), nseq * 64, 64, heads, d, ds, capi.stream_ptr()))
    torch.cuda.synchronize()
    live = 3 * heads * d
    assert torch.isfinite(want.float()).all()
    assert torch.equal(out[: nseq * 64, :live].view(torch.int16), want.view(torch.int16))
    assert torch.isnan(out[: nseq * 64, live:].float()).all()
    assert bool((out[nseq * 64:] == 7.0).all())
    assert torch.equal(out[: nseq * 64, :live].view(torch.int16), again[: nseq * 64, :live].view(torch.int16))
    # the layout, stated without the pack op: dq | dk | dv, head-major, token rows
    for i, t in enumerate(three):
        assert torch.equal(out[: nseq * 64, i * heads * d: (i + 1) * heads * d].view(torch.int16),
                           t[..., :d].transpose(1, 2).reshape(nseq * 64, heads * d).contiguous().view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------- the whole model
def _autograd(tag, x, k, d_out, cond=None, mask=None, want_dx=False):
    ps = {n: t.clone().requires_grad_() for n, t in ft.case_params(tag, cond is not None).items()}
    xx = x.clone().requires_grad_(want_dx)
    out = pc.fac_host(ps, xx, k, cond, mask, dtype=torch.float32)
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
    print(f"FacDiT training at 64 patches {label}: forward rel-L2 {r:.2e}, worst gradient rel-L2 {worst[1]:.2e} at {worst[0]}")
    assert r < FWD_BAR
    for n, gref in ref_grads.items():
        assert rel(grads[n], gref) < GRAD_BAR, (n, rel(grads[n], gref))


@pytest.mark.parametrize("tag", list(ft.TRAIN_CASES))
def test_backward_matches_autograd(tag):
    """with and without the spatial MLP; (B, T) = (2, 4), (1, 4), (2, 2): a single video, and a short input on the first rows of the longer
    temporal table.  A skipped spatial backward misses the bar on 28 of 46 (mlp0) / 32-33 of 58 (mlp4) gradients, a skipped temporal one on
    34 of 46 / 46 of 58 (module docstring)."""
    tr, _ = ft.trainer(tag)
    g = torch.Generator().manual_seed(31)
    for b, t in ((2, 4), (1, 4), (2, 2)):
        x = torch.randn(b, t, *pc.X_SHAPE, generator=g)
        k = torch.randint(0, 1000, (b, t), generator=g)
        d_out = torch.randn(b, t, *pc.X_SHAPE, generator=g)
        out = tr.forward(x, k)
        tr.backward(d_out)
        _check(f"{tag} B={b} T={t}", tr, out, *_autograd(tag, x, k, d_out))


def test_both_forms_of_the_spatial_backward_give_the_same_gradient_bits():
    """the trainer's default is the packed form; the three-buffer form + pack kernel, selected on the same handle, leaves the same bits"""
    from dfot_amd import capi
    tr, _ = ft.trainer("mlp4")
    g = torch.Generator().manual_seed(33)
    x = torch.randn(2, MT, *pc.X_SHAPE, generator=g)
    k = torch.randint(0, 1000, (2, MT), generator=g)
    d_out = torch.randn(2, MT, *pc.X_SHAPE, generator=g)
    tr.forward(x, k)
    tr.backward(d_out)
    packed = tr.grads.clone()
    capi.check(capi.lib.dfot_facdit_train_set_seq64_packed(tr._handle, 0))
    tr.forward(x, k)
    tr.backward(d_out)
    assert float(packed.norm()) > 0 and torch.equal(tr.grads.view(torch.int32), packed.view(torch.int32))


def test_action_conditioned_backward_matches_autograd():
    """case mlp0 with actions and the per-video mask (video 0 runs without its condition): the condition embedding's gradients included"""
    tr, _ = ft.trainer("mlp0", cond=True)
    g = torch.Generator().manual_seed(32)
    x = torch.randn(2, MT, *pc.X_SHAPE, generator=g)
    k = torch.randint(0, 1000, (2, MT), generator=g)
    d_out = torch.randn(2, MT, *pc.X_SHAPE, generator=g)
    cond = torch.randn(2, MT, pc.COND_DIM, generator=g)
    mask = torch.tensor([True, False])
    out = tr.forward(x, k, cond, mask.to(torch.uint8))
    tr.backward(d_out)
    ref_out, ref_grads = _autograd("mlp0", x, k, d_out, cond, mask)
    assert any(n.startswith("external_cond_embedding") for n in ref_grads)
    _check("mlp0, action-conditioned with the per-video mask", tr, out, ref_out, ref_grads)


def test_gradient_crosses_frames_only_through_the_temporal_attention():
    """The upstream gradient lives on the last frame alone.  The spatial blocks, the MLPs and the conditioning are per frame, so what
    reaches the INPUT of the earlier frames came through the temporal attention's backward and nothing else: autograd gives those frames a
    gradient of norm 3.37 (38.1 for the whole input), a host that skips the temporal backward gives exactly zero."""
    tr, _ = ft.trainer("mlp0")
    g = torch.Generator().manual_seed(31)
    x = torch.randn(2, MT, *pc.X_SHAPE, generator=g)
    k = torch.randint(0, 1000, (2, MT), generator=g)
    d_out = torch.randn(2, MT, *pc.X_SHAPE, generator=g)
    d_out[:, : MT - 1] = 0
    tr.forward(x, k)
    tr.backward(d_out)
    dx = tr.input_grad().cpu()
    _, _, ref_dx = _autograd("mlp0", x, k, d_out, want_dx=True)
    with ft.skipped_temporal_backward():
        _, _, skipped_dx = _autograd("mlp0", x, k, d_out, want_dx=True)
    early, last = slice(0, MT - 1), MT - 1
    assert float(skipped_dx[:, early].norm()) == 0.0 and float(ref_dx[:, early].norm()) > 1.0
    r_early, r_last = rel(dx[:, early], ref_dx[:, early]), rel(dx[:, last], ref_dx[:, last])
    print(f"input gradient for an upstream gradient on frame {last} alone: frames 0-{last - 1} norm {float(dx[:, early].norm()):.3f} (autograd "
          f"{float(ref_dx[:, early].norm()):.3f} of {float(ref_dx.norm()):.3f}), rel-L2 {r_early:.2e}; frame {last} rel-L2 {r_last:.2e}")
    assert r_early < GRAD_BAR and r_last < GRAD_BAR


@pytest.mark.parametrize("tag", list(ft.TRAIN_CASES))
def test_training_gradients_vs_reference_fixture(tag):
    """loss and gradients of the reference's own training step (differentiated by the reference's autograd on CPU) vs the engine"""
    g = fc.load(ft.FIXTURE)
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
def _batch(b, seed, t=MT):
    g = torch.Generator().manual_seed(seed)
    masks = torch.ones(b, t)
    masks[0, t - 1] = 0
    return (torch.randn(b, t, *pc.X_SHAPE, generator=g), torch.randint(0, 1000, (b, t), generator=g),
            torch.randn(b, t, *pc.X_SHAPE, generator=g), masks)


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
    print(f"two accumulated micro-batches vs the 4-video batch at 64 patches: rel-L2 {r:.2e}")
    assert r < 2e-2


def test_an_odd_token_count_is_refused_by_name_and_leaves_the_gradients():
    from dfot_amd import capi
    tr, _ = ft.trainer("mlp0", loss_weighting=ft.LOSS_WEIGHTING)
    xs, k, noise, masks = _batch(2, 43)
    tr.loss_and_grads(xs, k, noise, masks)
    before = tr.grads.clone()
    assert float(before.norm()) > 0
    x3, k3, n3, m3 = _batch(2, 44, t=3)
    for call in (lambda: tr.forward(x3, k3), lambda: tr.loss_and_grads(x3, k3, n3, m3), lambda: tr.training_step(x3, k3, n3, m3)):
        with pytest.raises(ValueError, match=r"even number of tokens: 3 tokens × 64 patches = 192 rows"):
            call()
    # the engine's own check, below the Python one: DFOT_ERR_SHAPE before anything is launched
    xd, kd = x3.cuda().contiguous(), k3.to(torch.int32).cuda().contiguous()
    out = torch.full_like(xd, float("nan"))
    assert capi.lib.dfot_dit_train_forward(tr._handle, capi.ptr(xd), capi.ptr(kd), capi.ptr(out), 2, 3, capi.stream_ptr()) == capi.ERR_SHAPE
    assert b"multiple of 128" in capi.lib.dfot_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert torch.equal(tr.grads.view(torch.int32), before.view(torch.int32)) and tr.step_count == 0


def test_the_full_dit3d_still_trains_at_64_patches_per_frame():
    """The sibling res-128 recipe (train_dfot_dit-s_taichikl_16_res128_ru.sh: variant "full", rope_3d) has the same 64 patches per frame but
    whole-video attention sequences (T x 64 tokens, a multiple of 128 at an even T): it keeps launch_attention_padded with its log-sum-exp
    and launch_attention_bwd, and must not take the 64-token path that variant 2 takes at this patch count.  DiT3DTrainer's forward and
    every parameter gradient against fp32 autograd through oracle.dit, the bars of the tests above; T = max_tokens and a shorter window.
    (The parent commit passes this test; an engine that chose the kernels or sized the workspace by the patch count alone does not.)"""
    import dfot_amd
    from oracle import dit as odit
    dcfg = odit.DiTConfig(hidden_size=256, depth=2, num_heads=4, in_channels=4, resolution=(16, 16), patch_size=2, max_tokens=MT)
    params = odit.seeded_params(dcfg, seed=6)
    tr = dfot_amd.DiT3DTrainer(dict(variant="full", pos_emb_type="rope_3d", patch_size=2, hidden_size=256, depth=2, num_heads=4),
                               x_shape=pc.X_SHAPE, max_tokens=MT)
    tr.load_state_dict(params, strict=True)
    g = torch.Generator().manual_seed(35)
    for b, t in ((2, MT), (1, 2)):
        x = torch.randn(b, t, *pc.X_SHAPE, generator=g)
        k = torch.randint(0, 1000, (b, t), generator=g)
        d_out = torch.randn(b, t, *pc.X_SHAPE, generator=g)
        out = tr.forward(x, k)
        tr.backward(d_out)
        ps = {n: v.clone().requires_grad_() for n, v in params.items()}
        ref = odit.forward(ps, dcfg, x, k)
        (ref * d_out).sum().backward()
        _check(f"full DiT3D B={b} T={t}", tr, out, ref.detach(), {n: v.grad for n, v in ps.items()})


def _config(src, **over):
    from dfot_amd import capi
    c = capi.DiTConfigF()
    for f, _ in capi.DiTConfig._fields_:
        setattr(c, f, getattr(src, f))
    for f, v in over.items():
        setattr(c, f, v)
    return c


def test_create_refuses_an_odd_max_tokens_and_the_matrix_trainer_64_patches():
    from dfot_amd import capi, dit_backbone
    tr, _ = ft.trainer("mlp0")
    handle = capi.C.c_void_p()
    assert capi.lib.dfot_facdit_train_create(capi.C.byref(_config(tr._ccfg, max_tokens=5)), capi.C.byref(handle)) == capi.ERR_SHAPE
    assert b"even max_tokens" in capi.lib.dfot_last_error() and not handle.value
    assert capi.lib.dfot_facdit_train_create(capi.C.byref(_config(tr._ccfg, height=8)), capi.C.byref(handle)) == capi.ERR_ARG  # 32 patches
    assert b"32 patches per frame must be a multiple of 128" in capi.lib.dfot_last_error() and not handle.value
    # FacMatDiT at the same geometry: the inference configuration (which takes 64 patches) handed to the training entry
    c = _config(tr._ccfg)
    dit_backbone.configure_facmat(c, pc.mat_cfg("b"), MT, allow_p64=True)
    assert c.variant == 3
    assert capi.lib.dfot_facmat_train_create(capi.C.byref(c), capi.C.byref(handle)) == capi.ERR_ARG
    assert b"64 patches per frame must be a multiple of 128" in capi.lib.dfot_last_error() and not handle.value
