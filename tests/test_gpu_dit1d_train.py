"""GPU tests of DiT1D training (dfot_amd.DiT1DTrainer, csrc/dit1d_train.inl, csrc/dit1d_train.hip): the trainer's forward against the fp64
host restatement and against dfot_amd.DiT1D, every parameter gradient and the input gradient against fp32 autograd through the host
restatement (tests/dit1d_train_common.py) and against the reference's own training step under its own autograd (tests/golden/dit1d_train.npz,
tools/make_golden_dit1d_train.py), at the geometry of tests/dit1d_common.py (B 2, T 8, [4, 1, 32], hidden 128, depth 2) and the
attention gain dit1d_train_common.TRAIN_GAIN = 2.75, in the three cases h4, h2 (both q/k/v row strides) and h4 without the mask; causality
of the backward, exactly; and the trainer's mechanics.

The gain: at the 4.0 recorded in tests/golden/dit1d.npz the engine misses the gradient bar (x_embedder.weight 7.0e-2, input gradient
6.9e-2, case h4) -- and so does plain fp32 autograd whose GEMM operands are rounded to bf16 where the engine rounds them
(dit1d_train_common.forward_emulated: 7.1e-2 / 7.2e-2 at the same places), so that is the operands' precision under so sharp a softmax
and no fault of the backward.  2.75 is the largest multiple of 0.25 at which that emulation holds half the bar (2.2e-2; the engine measures
2.2e-2 too), and the no-mask backward still misses every attn.qkv gradient by >= 5 x the bar there (tests/test_dit1d_train_host.py).

Bars (the ones tests/test_gpu_dit_fac_train.py:5-11 cites for the same quantities): forward rel-L2 < 2e-2, every parameter gradient and the
input gradient rel-L2 < 5e-2 against autograd, the training loss within 2e-2, against the reference's fixture the loss within 2e-2, every
gradient norm within 3e-2 and the stored tensors rel-L2 < 5e-2, accumulation rel < 2e-2, the optimizer step < 1e-3 on the
update against torch.optim.AdamW on the ENGINE's gradients.  fp32 autograd is within 1.5e-6 of fp64 on every gradient here, so fp32 is
an adequate yardstick.

Measured on one MI355X: forward 3.1e-3 .. 3.3e-3 against the fp64 host restatement and 1.6e-3 against dfot_amd.DiT1D; worst parameter
gradient 2.1e-2 .. 2.2e-2 and input gradient 1.7e-2 for a random d_out; under the training loss 1.4e-2 .. 1.8e-2 with the loss within
2.3e-4; against the reference's fixture the loss within 2.4e-4, gradient norms within 1.3e-3 .. 2.5e-3, stored tensors 1.1e-2 .. 1.3e-2;
accumulation 7.4e-8; the AdamW update 2.3e-5.

What a wrong backward measures, computed on the host in fp64 with dit1d_train_common.wrong_backward under the training loss at
dit1d_common.inputs() (tests/test_dit1d_train_host.py; the forward, hence the loss, unchanged): an attention backward that recomputes the
probabilities WITHOUT the frame mask misses the 5e-2 bar on 20 of the 28 parameter gradients (the 8 it leaves exact are the last block's
proj / MLP and the final layer, which no attention backward reaches), attn.qkv.weight by 0.47 / 0.37 (h4, blocks 0 / 1) and 0.40 / 0.30
(h2); one under a per-token causal mask on the same 20, attn.qkv.weight by 0.28 / 0.20 and 0.26 / 0.17.  The DiT3D LayerNorm backward (the
residual gradient through (1 + scale) and into dshift / dscale; wrong_backward("dit3d_ln"), all three cases) misses the bar on 22 of 28 (all
but the last block's MLP and the final layer), the adaLN_modulation weights by 1.6 .. 1.9; a LayerNorm backward with the neighbouring row's
statistics ("neighbour") on 16 .. 19 of 28, the worst by 0.22 .. 0.31.  In scratch builds of the library with either mutation in
d1_ln_share_bwd_kernel, test_backward_matches_autograd, test_training_loss_and_gradients_match_the_host (all three cases of each) and
test_gradient_reaches_earlier_frames_only fail here, and every case of test_ln_share_bwd in tests/test_gpu_dit1d_train_ops.py (with the
neighbouring row also test_ln_share_bwd_without_modulation).

Every test here fails on the parent commit: its package has no DiT1DTrainer, its library no dfot_dit1d_train_* symbol, and there is no
tests/golden/dit1d_train.npz."""
import math

import pytest
import torch

import dit1d_common as dc
import dit1d_train_common as tc
from dit1d_common import rel

pytestmark = pytest.mark.gpu

FWD_BAR = 2e-2
GRAD_BAR = 5e-2
B, T = dc.BATCH, dc.MAX_TOKENS


def _d_out(seed=33):
    return torch.randn(B, T, *dc.X_SHAPE, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("tag", list(tc.TRAIN_CASES))
def test_backward_matches_autograd(tag):
    tr, params = tc.trainer(tag)
    x, k = dc.inputs()
    d_out = _d_out()
    out = tr.forward(x, k)
    tr.backward(d_out)
    dx = tr.input_grad().cpu()
    ref_out, ref_grads, ref_dx = tc.host_forward_backward(tag, x, k, d_out)
    out64 = dc.forward_host(params, x, k, tc.TRAIN_CASES[tag][0], mask=tc._mask(tag))
    grads = {n: t.cpu() for n, t in tr.grad_dict().items()}
    assert list(grads) == list(ref_grads) == [n for n, _ in dc.key_shapes(tc.TRAIN_CASES[tag][0]) if n != "pos_embed"]
    rels = {n: rel(grads[n], g) for n, g in ref_grads.items()}
    worst = max(rels, key=rels.get)
    print(f"DiT1D training {tag}: forward rel-L2 {rel(out.cpu(), out64):.2e} (fp64 host), worst gradient rel-L2 {rels[worst]:.2e} at {worst}, "
          f"input gradient {rel(dx, ref_dx):.2e}")
    assert rel(out.cpu(), out64) < FWD_BAR and rel(out.cpu(), ref_out) < FWD_BAR
    for n, g in ref_grads.items():
        assert torch.isfinite(grads[n]).all() and float(g.norm()) > 0, n
        assert rels[n] < GRAD_BAR, (n, rels[n])
    assert rel(dx, ref_dx) < GRAD_BAR


@pytest.mark.parametrize("tag", ["h4", "h4_nomask"])
def test_forward_is_the_inference_models(tag):
    """the same weights in dfot_amd.DiT1D (fused gated epilogue, per-level table) and in the trainer (plain GEMM + gate, per-frame
    modulations): state_dict() loads strictly, pos_embed first, and the two forwards agree"""
    import dfot_amd
    tr, params = tc.trainer(tag)
    sd = tr.state_dict()
    assert list(sd) == [n for n, _ in dc.key_shapes(tc.TRAIN_CASES[tag][0])] and list(sd)[0] == "pos_embed"
    heads, mode = tc.TRAIN_CASES[tag]
    model = dfot_amd.DiT1D(dc.backbone_cfg(heads, causal_attn_mode=mode), x_shape=dc.X_SHAPE, max_tokens=T).cuda().eval()
    model.load_state_dict(sd, strict=True)
    x, k = dc.inputs()
    with torch.no_grad():
        ref = model(x.cuda(), k.cuda()).cpu()
    out = tr.forward(x, k).cpu()
    print(f"{tag}: trainer forward vs DiT1D rel-L2 {rel(out, ref):.2e}")
    assert rel(out, ref) < FWD_BAR


def test_gradient_reaches_earlier_frames_only():
    """d_out lives on frame 2 alone.  Under the frame mask a token of frame 2 saw frames 0-2, so the input gradient is non-zero there and
    bit-zero on frames 3-7 (every per-row kernel keeps a zero row zero, the attention backward skips masked blocks); without the mask it is
    non-zero on all eight."""
    x, k = dc.inputs()
    d_out = _d_out()
    d_out[:, :2] = 0
    d_out[:, 3:] = 0
    for tag, live in (("h4", 3), ("h4_nomask", T)):
        tr, _ = tc.trainer(tag)
        tr.forward(x, k)
        tr.backward(d_out)
        dx = tr.input_grad().cpu()
        _, _, ref_dx = tc.host_forward_backward(tag, x, k, d_out)
        norms = [float(dx[:, f].norm()) for f in range(T)]
        print(f"{tag}: input-gradient norm per frame {[round(v, 3) for v in norms]} (autograd {[round(float(ref_dx[:, f].norm()), 3) for f in range(T)]})")
        assert all(v > 1e-3 for v in norms[:live])
        assert bool((dx[:, live:] == 0).all())
        assert rel(dx[:, :live], ref_dx[:, :live]) < GRAD_BAR


def _batch(b, seed):
    g = torch.Generator().manual_seed(seed)
    masks = torch.ones(b, T)
    masks[0, T - 1] = 0
    return (torch.randn(b, T, *dc.X_SHAPE, generator=g), torch.randint(0, 1000, (b, T), generator=g), torch.randn(b, T, *dc.X_SHAPE, generator=g), masks)


@pytest.mark.parametrize("tag", list(tc.TRAIN_CASES))
def test_training_loss_and_gradients_match_the_host(tag):
    """the shared denoising loss (cosine schedule, pred_v, fused_min_snr, one masked token) through the trainer against the host restatement"""
    tr, _ = tc.trainer(tag, loss_weighting=tc.LOSS_WEIGHTING)
    xs, k, noise, masks = _batch(B, 5)
    loss = float(tr.loss_and_grads(xs, k, noise, masks).item())
    ref_loss, ref_grads = tc.host_loss_and_grads(tag, xs, k, noise, masks)
    grads = {n: t.cpu() for n, t in tr.grad_dict().items()}
    rels = {n: rel(grads[n], g) for n, g in ref_grads.items()}
    worst = max(rels, key=rels.get)
    print(f"{tag}: loss {loss:.6f} (host {float(ref_loss):.6f}), worst gradient rel-L2 {rels[worst]:.2e} at {worst}")
    assert abs(loss - float(ref_loss)) < 2e-2 * abs(float(ref_loss))
    for n in ref_grads:
        assert rels[n] < GRAD_BAR, (n, rels[n])


@pytest.mark.parametrize("tag", list(tc.TRAIN_CASES))
def test_training_gradients_vs_reference_fixture(tag):
    """loss and gradients of the reference's own training step (its DFoTVideo loss around its DIT1D, differentiated by its autograd on CPU)
    against the engine"""
    g = dc.load("dit1d_train.npz")
    tr, params = tc.trainer(tag, loss_weighting=tc.LOSS_WEIGHTING)
    assert dc.digest(params) == str(g[f"{tag}_digest"]) and float(g["qk_gain"]) == tc.TRAIN_GAIN
    xs, k = dc.inputs()
    assert dc.tensor_digest(xs, k) == str(g["inputs_digest"])
    loss = float(tr.loss_and_grads(xs, k, dc.T(g[f"{tag}_noise"]), dc.T(g["masks"])).item())
    ref_loss = float(g[f"{tag}_loss"])
    grads = {n: t.cpu() for n, t in tr.grad_dict().items()}
    names = [str(n) for n in g[f"{tag}_names"]]
    assert names == list(grads) and "pos_embed" not in names
    worst_norm = max(abs(float(grads[n].norm()) - ref_norm) / ref_norm for n, ref_norm in zip(names, g[f"{tag}_norms"]))
    worst = max(rel(grads[key.split("/", 1)[1]], dc.T(g[key])) for key in g.files if key.startswith(f"{tag}_grad/"))
    print(f"{tag}: loss {loss:.6f}, reference {ref_loss:.6f}; worst gradient-norm deviation {worst_norm:.2e}, worst stored-gradient rel-L2 {worst:.2e}")
    assert abs(loss - ref_loss) < 2e-2 * abs(ref_loss)
    for n, ref_norm in zip(names, g[f"{tag}_norms"]):
        assert abs(float(grads[n].norm()) - ref_norm) <= 3e-2 * ref_norm + 1e-7, (n, float(grads[n].norm()), ref_norm)
    assert worst < 5e-2


def test_accumulation_equals_one_batch_and_gradients_are_bit_reproducible():
    tr, _ = tc.trainer("h4", loss_weighting=tc.LOSS_WEIGHTING)
    xs, k, noise, masks = _batch(4, 41)
    tr.loss_and_grads(xs, k, noise, masks)
    full = tr.grads.clone()
    tr.loss_and_grads(xs, k, noise, masks)
    assert torch.equal(tr.grads.view(torch.int32), full.view(torch.int32))  # two runs, the same bits
    for sl in (slice(0, 2), slice(2, 4)):
        tr.loss_and_grads(xs[sl], k[sl], noise[sl], masks[sl])
        tr.accumulate()
    r = rel((tr._acc / tr._acc_n).cpu(), full.cpu())
    print(f"two accumulated micro-batches vs the 4-video batch: rel-L2 {r:.2e}")
    assert r < 2e-2


def _flat(params, tr):
    flat = torch.zeros(tr.numel)
    for name, (off, shape) in tr.layout.items():
        flat[off: off + params[name].numel()] = params[name].reshape(-1)
    return flat


def test_training_step_equals_torch_adamw_and_pos_embed_stays_frozen():
    tr, params = tc.trainer("h4", loss_weighting=tc.LOSS_WEIGHTING)
    tr.lr, tr.weight_decay, tr.max_grad_norm = 1e-3, 0.01, 1.0
    tr.enable_ema(0.9)
    xs, k, noise, masks = _batch(B, 42)
    loss = tr.training_step(xs, k, noise, masks)
    assert math.isfinite(float(loss.item())) and tr.step_count == 1
    new = {n: t.cpu() for n, t in tr.state_dict().items()}
    assert "pos_embed" not in tr.grad_dict() and "pos_embed" not in tr.layout and "pos_embed" not in tr.ema_state_dict()
    assert len(tr.optimizer_state_dict()["state"]) == len(tr.layout) == len(params) - 1
    ps = {n: t.clone().requires_grad_() for n, t in params.items() if n != "pos_embed"}
    for n, gr in tr.grad_dict().items():
        ps[n].grad = gr.cpu()
    plist = list(ps.values())
    torch.nn.utils.clip_grad_norm_(plist, 1.0)
    torch.optim.AdamW(plist, lr=1e-3, weight_decay=0.01, betas=(0.9, 0.99), eps=1e-8).step()
    worst = max(rel(new[n] - params[n], t.detach() - params[n]) for n, t in ps.items())
    print(f"one step vs torch.optim.AdamW on the engine's gradients: worst update rel-L2 {worst:.2e}")
    assert worst < 1e-3
    torch.testing.assert_close(tr.ema.cpu(), 0.9 * _flat(params, tr) + 0.1 * tr.params.cpu(), rtol=1e-6, atol=1e-7)
    # the optimizer state and the EMA shadow export and reload into a fresh trainer, which then takes the same next step
    sd, ema = tr.optimizer_state_dict(), tr.ema_state_dict()
    tr2, _ = tc.trainer("h4", loss_weighting=tc.LOSS_WEIGHTING)
    tr2.load_state_dict(tr.state_dict())
    tr2.load_optimizer_state_dict(sd)
    tr2.enable_ema(0.9)
    tr2.load_ema_state_dict(ema)
    tr2.max_grad_norm = 1.0
    assert tr2.step_count == 1 and tr2.lr == 1e-3
    for _ in range(2):  # three steps in all, weight_decay > 0
        tr.training_step(xs, k, noise, masks)
        tr2.training_step(xs, k, noise, masks)
    torch.testing.assert_close(tr2.params, tr.params, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(tr2.ema, tr.ema, rtol=1e-5, atol=1e-6)
    assert tr.step_count == 3
    assert torch.equal(tr.state_dict()["pos_embed"].cpu().view(torch.int32), params["pos_embed"].view(torch.int32))  # bit-identical


def test_refusals_by_name():
    import dfot_amd
    from dfot_amd import DiffusionConfig
    tr, _ = tc.trainer("h4")
    x, k = dc.inputs()
    with pytest.raises(ValueError, match="T == max_tokens = 8 only"):
        tr.forward(x[:, :4], k[:, :4])
    with pytest.raises(TypeError, match="integer noise levels"):
        tr.forward(x, k.float())
    with pytest.raises(ValueError, match="takes no condition"):
        tr.forward(x, k, torch.zeros(B, T, 2))
    fresh, _ = tc.trainer("h4")
    with pytest.raises(RuntimeError, match="backward: no forward to differentiate"):
        fresh.backward(torch.zeros_like(x))
    with pytest.raises(RuntimeError, match="input_grad: no forward to differentiate"):
        fresh.input_grad()
    with pytest.raises(ValueError, match="d_out has shape"):
        tr.forward(x, k), tr.backward(torch.zeros(B, T, 4, 1, 16))
    with pytest.raises(ValueError, match="takes no conditions"):
        tr.loss_and_grads(x, k, torch.zeros_like(x), None, conditions=torch.zeros(B, T, 2))
    cfg = dc.backbone_cfg(4)
    with pytest.raises(ValueError, match="use_fourier_noise_embedding"):
        dfot_amd.DiT1DTrainer({**cfg, "use_fourier_noise_embedding": True}, x_shape=dc.X_SHAPE, max_tokens=T)
    with pytest.raises(ValueError, match="is_continuous"):
        dfot_amd.DiT1DTrainer(cfg, x_shape=dc.X_SHAPE, max_tokens=T, diffusion=DiffusionConfig(is_continuous=True))
    with pytest.raises(ValueError, match="external_cond_dim=3"):
        dfot_amd.DiT1DTrainer(cfg, x_shape=dc.X_SHAPE, max_tokens=T, external_cond_dim=3)
    with pytest.raises(ValueError, match="merge_mode"):
        dfot_amd.DiT1DTrainer({**cfg, "merge_mode": "concat"}, x_shape=dc.X_SHAPE, max_tokens=T)
    with pytest.raises(ValueError, match="multiples of 128"):
        dfot_amd.DiT1DTrainer({**cfg, "hidden_size": 192, "num_heads": 3}, x_shape=dc.X_SHAPE, max_tokens=T)
    # the engine's own refusals name the field
    from dfot_amd import capi
    c = capi.DiT1DConfig()
    for f, _ in capi.DiT1DConfig._fields_:
        setattr(c, f, getattr(tr._ccfg, f))
    c.hidden = 192
    handle = capi.C.c_void_p()
    assert capi.lib.dfot_dit1d_train_create(capi.C.byref(c), capi.C.byref(handle)) == capi.ERR_SHAPE
    assert b"hidden 192" in capi.lib.dfot_last_error() and not handle.value
    tr.forward(x, k)  # reserved and synchronised: what is left to refuse is the shape
    xd, kd, out = x.cuda(), k.int().cuda(), torch.empty_like(x).cuda()
    assert capi.lib.dfot_dit1d_train_forward(tr._handle, capi.ptr(xd), capi.ptr(kd), capi.ptr(out), B, 4, capi.stream_ptr()) == capi.ERR_SHAPE
    assert b"max_tokens = 8 only" in capi.lib.dfot_last_error()
