"""GPU tests of FacMatDiT training at 64 patches per frame (latents 4x16x16 at patch 2, the taichi res-128 facmat-s-*-bias recipes): the
left-factor gradient kernel (csrc/facmat_factor_wgrad.hip) at the op level, the trainer's forward and every parameter gradient against fp32
autograd through the host restatement, the reference's own training step (tests/golden/dit_facmat_p64_train.npz,
tools/make_golden_dit_facmat_p64_train.py), and the trainer's mechanics and refusals.  Geometry: tests/dit_p64_common.py (embed_row_dim
128, depth 2, 4 spatial heads, max_tokens 4); models: tests/dit_facmat_p64_train_common.MODELS.

Bars.  The op: dit_block_common.assert_sum_bound, |got - ref64| <= (N + 4) 2^-24 sum |terms| elementwise with N = frames * hd additions;
the operands are bf16, so every product is exact in fp32 and the bound holds for any summation order (MFMA accumulation, the frame slices,
the slice sum).  The whole model, those of tests/test_gpu_dit_facmat_train.py for the same quantities: forward rel-L2 < 2e-2 and every
parameter gradient rel-L2 < 5e-2 against autograd (:25-26); against the reference's fixture loss within 2e-2, every gradient norm within
3e-2, stored tensors rel-L2 < 5e-2 (:199-210); accumulation rel < 2e-2 (:232); a reloaded optimizer state continues within rtol 1e-5,
atol 1e-6 (:263).

Every test here fails on the parent commit: its library exports neither dfot_op_facmat_factor_wgrad nor dfot_facmat_train_create_p64, and
its FacMatDiTTrainer has no allow_p64 keyword."""
import math

import pytest
import torch

import dit_block_common as bc
import dit_facmat_common as fm
import dit_facmat_p64_train_common as ft
import dit_facmat_train_common as ft128
import dit_p64_common as pc
from dit_facmat_common import T, rel

pytestmark = pytest.mark.gpu

FWD_BAR = 2e-2   # tests/test_gpu_dit_facmat_train.py:25
GRAD_BAR = 5e-2  # tests/test_gpu_dit_facmat_train.py:26
MT = pc.MAX_TOKENS
GUARD = 4096     # floats after the output that must keep their NaN


# ---------------------------------------------------------------------------------------------------------------- the kernel
def _operands(frames, ra, rb, hd, seed=7):
    g = torch.Generator().manual_seed(seed + 1000 * frames + ra + 2 * rb + hd)
    a = torch.randn(frames, ra, hd, generator=g).to(torch.bfloat16)
    b = torch.randn(frames, rb, hd, generator=g).to(torch.bfloat16)
    return a, b


def _run(a, b, frames, ra, rb, hd):
    """out [ra * rb + GUARD] of the op, started as NaN"""
    from dfot_amd import capi
    ad, bd = a.cuda().contiguous(), b.cuda().contiguous()
    out = torch.full((ra * rb + GUARD,), float("nan"), device="cuda")
    capi.check(capi.lib.dfot_op_facmat_factor_wgrad(capi.ptr(ad), capi.ptr(bd), capi.ptr(out), frames, ra, rb, hd, capi.stream_ptr()))
    torch.cuda.synchronize()
    return out


# (frames, Ra, Rb, hd): both orientations at E 64 and 128; one frame (a single slice, stored straight into the output), a few frames
# (one frame per slice), and frame counts beyond one slice per frame on a 256-CU device at one tile (34 frames still fit; 300 frames over
# 256 or, at two tiles, 128 slices leave an uneven split: the first 44 slices take one frame more)
OP_SHAPES = [(1, 64, 64, 128), (2, 64, 128, 128), (7, 128, 64, 256), (34, 64, 64, 384), (34, 128, 64, 384), (300, 64, 64, 128),
             (300, 128, 64, 128), (3, 128, 128, 128)]


@pytest.mark.parametrize("frames,ra,rb,hd", OP_SHAPES)
def test_factor_wgrad_vs_fp64(frames, ra, rb, hd):
    a, b = _operands(frames, ra, rb, hd)
    out = _run(a, b, frames, ra, rb, hd)
    assert bool(torch.isnan(out[ra * rb:]).all())  # nothing past the end
    got = out[: ra * rb].reshape(ra, rb).cpu()
    ref = torch.einsum("fad,fbd->ab", a.double(), b.double())
    abs_terms = torch.einsum("fad,fbd->ab", a.double().abs(), b.double().abs())
    k = bc.assert_sum_bound(f"facmat_factor_wgrad frames {frames} {ra} x {rb} hd {hd}", got, ref, abs_terms, frames * hd)
    print(f"facmat_factor_wgrad frames {frames} {ra} x {rb} hd {hd}: rel-L2 {k[1]:.3e}")
    # the orientation: an asymmetric pair, exact in fp32 -- row i of a is e_i-like, so out[i][j] picks b's entries, not its transpose
    if frames == 1:
        a1 = torch.zeros(1, ra, hd)
        a1[0, torch.arange(ra), torch.arange(ra)] = 1.0  # a[i][d] = [d == i]  (ra <= hd)
        b1 = (torch.arange(rb)[:, None] * 3 + torch.arange(hd)[None, :] * 5).float().remainder(251.0).reshape(1, rb, hd)
        o1 = _run(a1.to(torch.bfloat16), b1.to(torch.bfloat16), 1, ra, rb, hd)[: ra * rb].reshape(ra, rb).cpu()
        assert torch.equal(o1, b1[0, :, :ra].t().contiguous())  # out[i][j] = b[j][i]


def test_factor_wgrad_bits_do_not_depend_on_the_run_or_on_what_ran_before():
    frames, ra, rb, hd = 34, 128, 64, 384
    a, b = _operands(frames, ra, rb, hd)
    first = _run(a, b, frames, ra, rb, hd)
    again = _run(a, b, frames, ra, rb, hd)
    assert torch.equal(bc.bits(first), bc.bits(again))
    # other shapes in between reuse (and regrow) the op's workspace and leave other partial tiles in it
    for other in ((300, 64, 64, 128), (2, 64, 128, 128), (1, 64, 64, 128)):
        _run(*_operands(*other), *other)
    after = _run(a, b, frames, ra, rb, hd)
    assert torch.equal(bc.bits(first), bc.bits(after))
    assert torch.isfinite(first[: ra * rb]).all() and float(first[: ra * rb].abs().max()) > 0


def test_factor_wgrad_invalid_shapes_launch_nothing():
    from dfot_amd import capi
    a, b = _operands(2, 128, 128, 256)
    ad, bd = a.cuda(), b.cuda()
    out = torch.full((128 * 128 + GUARD,), float("nan"), device="cuda")

    def call(frames, ra, rb, hd, aa=ad, bb=bd, oo=out):
        return capi.lib.dfot_op_facmat_factor_wgrad(capi.ptr(aa), capi.ptr(bb), capi.ptr(oo), frames, ra, rb, hd, capi.stream_ptr())
    for args in ((2, 32, 64, 128), (2, 64, 96, 128), (2, 256, 64, 128), (2, 64, 0, 128), (2, 64, 64, 64), (2, 64, 64, 192), (2, 64, 64, 0),
                 (0, 64, 64, 128), (-3, 64, 64, 128)):
        assert call(*args) == capi.ERR_SHAPE, args
        assert capi.lib.dfot_last_error().startswith(b"op_facmat_factor_wgrad:")
    for kw in (dict(aa=None), dict(bb=None), dict(oo=None)):
        assert call(2, 64, 64, 128, **kw) == capi.ERR_ARG, list(kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())  # nothing was launched
    assert call(2, 128, 128, 256) == capi.OK
    torch.cuda.synchronize()
    assert torch.isfinite(out[: 128 * 128]).all() and bool(torch.isnan(out[128 * 128:]).all())


# ---------------------------------------------------------------------------------------------------------------- the whole model
def _autograd(tag, x, k, d_out, cond=None, mask=None):
    ps = {n: t.clone().requires_grad_() for n, t in ft.case_params(tag, cond is not None).items()}
    out = ft.host(tag, ps, x, k, cond, mask, dtype=torch.float32)  # pc.mat_host for the tags of dit_facmat_common.CASES
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
    factors = max(rel(grads[n], gref) for n, gref in ref_grads.items() if n.endswith(("attn.qkv_u", "attn.proj_u")))
    print(f"FacMatDiT training at 64 patches {label}: forward rel-L2 {r:.2e}, worst gradient rel-L2 {worst[1]:.2e} at {worst[0]}; "
          f"worst left-factor gradient {factors:.2e}")
    assert r < FWD_BAR
    for n, gref in ref_grads.items():
        assert rel(grads[n], gref) < GRAD_BAR, (n, rel(grads[n], gref))


@pytest.mark.parametrize("tag", ["b", "e128", "a", "d"])
def test_backward_matches_autograd(tag):
    """both fixture cases (E 64 with biases, spatial MLP and RoPE; E 128 with none of them) and cases a and d at E 64 (the other head
    split without / with the MLP, with / without the rotation); (B, T) = (2, 4) and (1, 2): a full window and a short single video"""
    tr, _ = ft.trainer(tag)
    g = torch.Generator().manual_seed(31)
    for b, t in ((2, 4), (1, 2)):
        x = torch.randn(b, t, *pc.X_SHAPE, generator=g)
        k = torch.randint(0, 1000, (b, t), generator=g)
        d_out = torch.randn(b, t, *pc.X_SHAPE, generator=g)
        out = tr.forward(x, k)
        tr.backward(d_out)
        _check(f"{tag} {ft.MODELS[tag]} B={b} T={t}", tr, out, *_autograd(tag, x, k, d_out))


def test_action_conditioned_backward_matches_autograd():
    """case a with actions and the per-video mask (video 0 runs without its condition): the condition embedding's gradients included"""
    tr, _ = ft.trainer("a", cond=True)
    g = torch.Generator().manual_seed(32)
    x = torch.randn(2, MT, *pc.X_SHAPE, generator=g)
    k = torch.randint(0, 1000, (2, MT), generator=g)
    d_out = torch.randn(2, MT, *pc.X_SHAPE, generator=g)
    cond = torch.randn(2, MT, pc.COND_DIM, generator=g)
    mask = torch.tensor([True, False])
    out = tr.forward(x, k, cond, mask.to(torch.uint8))
    tr.backward(d_out)
    ref_out, ref_grads = _autograd("a", x, k, d_out, cond, mask)
    assert any(n.startswith("external_cond_embedding") for n in ref_grads)
    _check("a, action-conditioned with the per-video mask", tr, out, ref_out, ref_grads)


@pytest.mark.parametrize("tag", ft.TRAIN_CASES)
def test_training_gradients_vs_reference_fixture(tag):
    """loss and gradients of the reference's own training step (differentiated by the reference's autograd on CPU) vs the engine; the bars
    of test_training_gradients_vs_reference_fixture in tests/test_gpu_dit_facmat_train.py:199-210"""
    g = fm.load(ft.FIXTURE)
    tr, params = ft.trainer(tag, loss_weighting=ft.LOSS_WEIGHTING)
    assert fm.digest(params) == str(g[f"{tag}_digest"])
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
    tr, _ = ft.trainer("b", loss_weighting=ft.LOSS_WEIGHTING)
    xs, k, noise, masks = _batch(4, 41)
    tr.loss_and_grads(xs, k, noise, masks)
    full = tr.grads.clone()
    tr.loss_and_grads(xs, k, noise, masks)
    assert float(full.norm()) > 0 and torch.equal(tr.grads.view(torch.int32), full.view(torch.int32))  # two runs, the same bits
    for sl in (slice(0, 2), slice(2, 4)):  # two micro-batches of 2 videos = the mean of their gradients = the gradient of the 4-video batch
        tr.loss_and_grads(xs[sl], k[sl], noise[sl], masks[sl])
        tr.accumulate()
    acc = tr._acc / tr._acc_n
    r = rel(acc.cpu(), full.cpu())
    print(f"two accumulated micro-batches vs the 4-video batch at 64 patches: rel-L2 {r:.2e}")
    assert r < 2e-2


def test_training_step_changes_the_weights_and_a_reloaded_optimizer_state_continues():
    tr, params = ft.trainer("e128", loss_weighting=ft.LOSS_WEIGHTING)
    tr.lr, tr.weight_decay, tr.max_grad_norm = 1e-3, 0.01, 1.0
    xs, k, noise, masks = _batch(2, 42)
    loss = tr.training_step(xs, k, noise, masks)
    assert math.isfinite(float(loss.item())) and tr.step_count == 1
    new = {n: t.cpu() for n, t in tr.state_dict().items()}
    for n in ("dit_base.temporal_blocks.0.attn.qkv_u", "dit_base.temporal_blocks.1.attn.proj_u", "dit_base.blocks.0.attn.qkv.weight"):
        assert not torch.equal(new[n], params[n]), n
    sd = tr.optimizer_state_dict()
    tr2, _ = ft.trainer("e128", loss_weighting=ft.LOSS_WEIGHTING)
    tr2.load_state_dict(tr.state_dict())
    tr2.load_optimizer_state_dict(sd)
    tr2.max_grad_norm = 1.0
    assert tr2.step_count == 1 and tr2.lr == 1e-3
    tr.training_step(xs, k, noise, masks)
    tr2.training_step(xs, k, noise, masks)
    torch.testing.assert_close(tr2.params, tr.params, rtol=1e-5, atol=1e-6)  # tests/test_gpu_dit_facmat_train.py:263


def test_an_odd_token_count_is_refused_by_name_and_leaves_the_gradients():
    from dfot_amd import capi
    tr, _ = ft.trainer("e128", loss_weighting=ft.LOSS_WEIGHTING)
    xs, k, noise, masks = _batch(2, 43)
    tr.loss_and_grads(xs, k, noise, masks)
    before = tr.grads.clone()
    assert float(before.norm()) > 0
    x3, k3, n3, m3 = _batch(2, 44, t=3)
    for call in (lambda: tr.forward(x3, k3), lambda: tr.loss_and_grads(x3, k3, n3, m3)):
        with pytest.raises(ValueError, match=r"even number of tokens: 3 tokens × 64 patches = 192 rows"):
            call()
    # the engine's own check, below the Python one: DFOT_ERR_SHAPE before anything is launched
    xd, kd = x3.cuda().contiguous(), k3.to(torch.int32).cuda().contiguous()
    out = torch.full_like(xd, float("nan"))
    assert capi.lib.dfot_dit_train_forward(tr._handle, capi.ptr(xd), capi.ptr(kd), capi.ptr(out), 2, 3, capi.stream_ptr()) == capi.ERR_SHAPE
    assert b"even number of tokens" in capi.lib.dfot_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert torch.equal(tr.grads.view(torch.int32), before.view(torch.int32)) and tr.step_count == 0


def _config(src, **over):
    from dfot_amd import capi
    c = capi.DiTConfigF()
    for f, _ in capi.DiTConfig._fields_:
        setattr(c, f, getattr(src, f))
    for f, v in over.items():
        setattr(c, f, v)
    return c


def test_the_new_entry_refuses_an_odd_max_tokens_other_variants_and_fourier_noise():
    from dfot_amd import capi
    tr, _ = ft.trainer("b")
    create = capi.lib.dfot_facmat_train_create_p64
    handle = capi.C.c_void_p()
    assert create(capi.C.byref(_config(tr._ccfg, max_tokens=5)), capi.C.byref(handle)) == capi.ERR_SHAPE
    assert b"even max_tokens" in capi.lib.dfot_last_error() and not handle.value
    assert create(capi.C.byref(_config(tr._ccfg, height=8)), capi.C.byref(handle)) == capi.ERR_ARG  # 32 patches
    assert b"32 patches per frame must be a multiple of 128" in capi.lib.dfot_last_error() and not handle.value
    for variant in (0, 1, 2):  # variant 1, the DifferenceDiT3D, keeps refusing 64 patches: nothing builds it here
        assert create(capi.C.byref(_config(tr._ccfg, variant=variant)), capi.C.byref(handle)) == capi.ERR_ARG
        assert b"variant 3" in capi.lib.dfot_last_error() and not handle.value
    assert capi.lib.dfot_dit_train_create_f(capi.C.byref(_config(tr._ccfg, variant=1, max_tokens=2 * MT)), capi.C.byref(handle)) == capi.ERR_ARG
    assert b"64 patches per frame must be a multiple of 128" in capi.lib.dfot_last_error() and not handle.value
    c = _config(tr._ccfg)
    c.fourier_noise = 1
    assert create(capi.C.byref(c), capi.C.byref(handle)) == capi.ERR_ARG
    assert b"fourier_noise" in capi.lib.dfot_last_error() and not handle.value
    # the older entry keeps its refusal of the very configuration the new one builds
    assert capi.lib.dfot_facmat_train_create(capi.C.byref(_config(tr._ccfg)), capi.C.byref(handle)) == capi.ERR_ARG
    assert b"64 patches per frame must be a multiple of 128" in capi.lib.dfot_last_error() and not handle.value


def test_at_128_patches_the_new_entry_gives_the_old_entrys_gradient_bits():
    """case b of tests/golden/dit_facmat_train.npz (latents 4x16x8 at patch 1, T = 5): the trainer built with allow_p64=True goes through
    dfot_facmat_train_create_p64 and must take the code path of dfot_facmat_train_create there"""
    import dfot_amd
    g = fm.load("dit_facmat_train.npz")
    old, params = ft128.trainer("b", loss_weighting=ft128.LOSS_WEIGHTING)
    cc, rr, bias, ratio, rope = fm.CASES["b"]
    new = dfot_amd.FacMatDiTTrainer(fm.backbone_cfg(cc, rr, bias, ratio, rope), x_shape=(4, 16, 8), max_tokens=5, allow_p64=True,
                                    loss_weighting=ft128.LOSS_WEIGHTING)
    new.load_state_dict(params, strict=True)
    losses = [tr.loss_and_grads(T(g["xs"]), T(g["k"]), T(g["b_noise"]), T(g["masks"])) for tr in (old, new)]
    assert float(old.grads.norm()) > 0
    assert torch.equal(old.grads.view(torch.int32), new.grads.view(torch.int32))
    assert float(losses[0].item()) == float(losses[1].item())
