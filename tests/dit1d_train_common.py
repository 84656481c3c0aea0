"""Shared helpers of tests/test_dit1d_train_host.py and tests/test_gpu_dit1d_train.py (not a test module): the training loss of the DiT1D
backbone restated on the host, on top of tests/dit1d_common.py.

  * LOSS_WEIGHTING        fused_min_snr with cum_snr_decay 0.96, as the other trainers' tests use
  * TRAIN_CASES           tag -> (heads, causal_attn_mode): h4 and h2 (both q/k/v row strides) and h4 without the mask
  * TRAIN_GAIN            the gain of the q and k rows of every qkv.weight in the training cases: 2.75, not the 4.0 recorded in
                          tests/golden/dit1d.npz for sampling.  At 4.0 the engine's gradients miss the 5e-2 bar against fp32 autograd
                          (x_embedder.weight 7.0e-2, the input gradient 6.9e-2 in case h4, one MI355X) and so does forward_emulated
                          below, which is plain autograd with the GEMM operands rounded to bf16 where the engine rounds them
                          (7.1e-2 / 7.2e-2 at the same two places): the deviation is the operands' precision under a softmax that
                          sharp, not the backward.  The gain is therefore lowered, to the largest multiple of 0.25 at which the
                          emulation holds HALF the bar in all three cases (2.2e-2 at 2.75; 3.0e-2 at 3.0), and only because the
                          no-mask backward still misses every attn.qkv.weight gradient by more than 5 x the bar there (0.27 .. 0.47;
                          the attn.qkv.bias gradients by 0.23 .. 0.41, whose smallest figure does not move with the gain).
                          tests/test_dit1d_train_host.py asserts each of these statements; tools/make_golden_dit1d_train.py has the
                          whole reasoning.
  * case_params           the seeded weights of a case at TRAIN_GAIN
  * host_forward_backward fp32 / fp64 autograd of <out, d_out> through dit1d_common.forward_host: (out, {name: gradient}, dx); pos_embed
                          is frozen and gets no gradient
  * host_loss_and_grads   autograd through forward_host + oracle.sampler.discrete_training_loss with the loss masks of
                          DFoTVideo._reweight_loss: (loss, {name: gradient})
  * trainer               dfot_amd.DiT1DTrainer at a case with the seeded weights
  * forward_emulated      forward_host in fp32 with every bf16 tensor of the engine rounded to bf16: GEMM operands (modulated rows, weights,
                          q / k / v, the probabilities, o, a, u, GELU(u), y) in the forward, and the gradients the engine stores in bf16
                          (da, dh, du, dO, dq, dk, dv, dqkv) in the backward; sums, LayerNorm, gates and the residual stream stay fp32
  * wrong_backward        context in which forward_host differentiates as an engine with a wrong backward would, the forward unchanged:
                          "nomask" (the attention backward recomputes the probabilities without the frame mask), "token" (under a
                          per-token causal mask), "dit3d_ln" (the DiT3D LayerNorm backward: the residual gradient through (1 + scale)
                          and into dshift / dscale), "neighbour" (the LayerNorm backward with the neighbouring row's statistics)
"""
import contextlib

import torch
import torch.nn.functional as F

import dit1d_common as dc

LOSS_WEIGHTING = dict(strategy="fused_min_snr", cum_snr_decay=0.96)
TRAIN_CASES = {"h4": (4, "video_temporal_causal"), "h2": (2, "video_temporal_causal"), "h4_nomask": (4, None)}


TRAIN_GAIN = 2.75


def case_params(tag, gain=None):
    return dc.seeded_params(dc.key_shapes(TRAIN_CASES[tag][0]), TRAIN_GAIN if gain is None else gain)


def _mask(tag):
    return "frame" if TRAIN_CASES[tag][1] is not None else "none"


def _leaves(tag, dtype, gain=None):
    return {n: (t.clone().to(dtype).requires_grad_() if n != "pos_embed" else t.clone().to(dtype)) for n, t in case_params(tag, gain).items()}


def host_forward_backward(tag, x, k, d_out, dtype=torch.float32, gain=None, emulated=False):
    ps = _leaves(tag, dtype, gain)
    xx = x.clone().to(dtype).requires_grad_()
    fwd = forward_emulated if emulated else dc.forward_host
    out = fwd(ps, xx, k, TRAIN_CASES[tag][0], mask=_mask(tag), dtype=dtype)
    (out * d_out.to(dtype)).sum().backward()
    return out.detach(), {n: t.grad.detach() for n, t in ps.items() if n != "pos_embed"}, xx.grad.detach()


def host_loss_and_grads(tag, xs, k, noise, masks, dtype=torch.float32, weighting=LOSS_WEIGHTING, gain=None, emulated=False):
    from oracle import sampler as osm, schedule as sch
    ps = _leaves(tag, dtype, gain)
    fwd = forward_emulated if emulated else dc.forward_host
    model = lambda x, lv, c, m: fwd(ps, x, lv, TRAIN_CASES[tag][0], mask=_mask(tag), dtype=dtype)
    _, per_el = osm.discrete_training_loss(model, sch.build_tables(beta_schedule="cosine"), xs.to(dtype), k, noise.to(dtype).clamp(-20, 20), **weighting)
    loss = (per_el * masks.to(dtype)[..., None, None, None]).mean()
    loss.backward()
    return loss.detach(), {n: t.grad.detach() for n, t in ps.items() if n != "pos_embed"}


def trainer(tag, **kw):
    import dfot_amd
    heads, mode = TRAIN_CASES[tag]
    params = case_params(tag)
    tr = dfot_amd.DiT1DTrainer(dc.backbone_cfg(heads, causal_attn_mode=mode), x_shape=dc.X_SHAPE, max_tokens=dc.MAX_TOKENS, **kw)
    tr.load_state_dict(params, strict=True)
    return tr, params


class _Round(torch.autograd.Function):
    """bf16 rounding in the forward, straight through in the backward"""

    @staticmethod
    def forward(ctx, x):
        return x.bfloat16().to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundGrad(torch.autograd.Function):
    """identity in the forward, the gradient rounded to bf16"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().to(g.dtype)


class _NeighbourLayerNorm(torch.autograd.Function):
    """LayerNorm whose backward normalises with the statistics of the neighbouring row (the previous token of the sequence)"""

    @staticmethod
    def forward(ctx, x, eps):
        ctx.save_for_backward(x)
        ctx.eps = eps
        return F.layer_norm(x, x.shape[-1:], eps=eps)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        xs = x.roll(1, dims=-2)
        rstd = 1 / torch.sqrt(xs.var(-1, unbiased=False, keepdim=True) + ctx.eps)
        n = (xs - xs.mean(-1, keepdim=True)) * rstd
        return rstd * (g - g.mean(-1, keepdim=True) - n * (g * n).mean(-1, keepdim=True)), None


def forward_emulated(params, x, levels, heads, mask="frame", dtype=torch.float32):
    return _forward(params, x, levels, heads, mask, dtype, bf16=True)


def _forward(params, x, levels, heads, mask="frame", dtype=torch.float64, bf16=False, ln="true"):
    """dit1d_common.forward_host (residual "norm") written once more with two switches; with both off it is forward_host, value and
    gradients (tests/test_dit1d_train_host.py).  bf16: the engine's bf16 tensors (r = a bf16 operand, rr = one whose gradient is bf16
    too).  ln: how the blocks' LayerNorms differentiate, the forward value unchanged -- "true"; "dit3d": the residual base carries the
    gradient paths of the MODULATED row, i.e. the residual gradient goes through (1 + scale) and into dshift / dscale, what the DiT3D
    kernels compute; "neighbour": the LayerNorm backward uses the neighbouring row's statistics."""
    ident = lambda t: t  # noqa: E731
    r = _Round.apply if bf16 else ident

    def rr(t):
        return _RoundGrad.apply(_Round.apply(t)) if bf16 else t
    rg = _RoundGrad.apply if bf16 else ident

    def norm(t):
        return _NeighbourLayerNorm.apply(t, 1e-6) if ln == "neighbour" else F.layer_norm(t, t.shape[-1:], eps=1e-6)

    def base_of(n, m):
        return n.detach() + (m - m.detach()) if ln == "dit3d" else n
    p = {n: t.to(dtype) for n, t in params.items()}
    b, t, c, _, length = x.shape
    h = p["x_embedder.weight"].shape[0]
    d = h // heads
    tok = x.to(dtype)[..., 0, :].permute(0, 1, 3, 2).reshape(b, t * length, c)
    s = F.linear(tok, p["x_embedder.weight"], p["x_embedder.bias"]) + p["pos_embed"]
    te = dc.timestep_embedding(levels, dtype)
    te = F.linear(F.silu(F.linear(te, p["t_embedder.mlp.0.weight"], p["t_embedder.mlp.0.bias"])), p["t_embedder.mlp.2.weight"],
                  p["t_embedder.mlp.2.bias"])
    am = dc.attention_mask(t, length, mask, dtype)

    def per_token(v):
        return v[:, :, None, :].expand(b, t, length, h).reshape(b, t * length, h)
    depth = sum(1 for n in p if n.endswith("attn.qkv.weight"))
    for i in range(depth):
        pre = f"blocks.{i}"
        mod = F.linear(r(F.silu(te)), r(p[f"{pre}.adaLN_modulation.1.weight"]), p[f"{pre}.adaLN_modulation.1.bias"])
        sh1, sc1, g1, sh2, sc2, g2 = (per_token(m) for m in mod.chunk(6, dim=2))
        n1 = norm(s)
        m1 = n1 * (1 + sc1) + sh1
        qkv = rg(F.linear(r(m1), r(p[f"{pre}.attn.qkv.weight"]), p[f"{pre}.attn.qkv.bias"]))
        q, k, v = qkv.view(b, t * length, 3, heads, d).permute(2, 0, 3, 1, 4)
        q, k, v = rr(q * d ** -0.5), rr(k), rr(v)
        a = q @ k.transpose(-2, -1)
        if am is not None:
            a = a + am
        o = rr((r(torch.softmax(a, -1)) @ v).transpose(1, 2).reshape(b, t * length, h))
        s = base_of(n1, m1) + g1 * rr(F.linear(o, r(p[f"{pre}.attn.proj.weight"]), p[f"{pre}.attn.proj.bias"]))
        n2 = norm(s)
        m2 = n2 * (1 + sc2) + sh2
        u = rr(F.linear(r(m2), r(p[f"{pre}.mlp.fc1.weight"]), p[f"{pre}.mlp.fc1.bias"]))
        y = rr(F.linear(rr(F.gelu(u, approximate="tanh")), r(p[f"{pre}.mlp.fc2.weight"]), p[f"{pre}.mlp.fc2.bias"]))
        s = base_of(n2, m2) + g2 * y
    out = F.linear(F.layer_norm(s, (h,), eps=1e-6), p["final_layer.1.weight"], p["final_layer.1.bias"])
    return out.view(b, t, length, c).permute(0, 1, 3, 2).unsqueeze(-2)


class _MaskedBackward(torch.autograd.Function):
    """softmax(a + forward mask) in the forward; the backward differentiates softmax(a + backward mask): what a flash backward computes
    that recomputes the probabilities under another mask"""

    @staticmethod
    def forward(ctx, a, fwd_mask, bwd_mask):
        ctx.save_for_backward(a, bwd_mask)
        return torch.softmax(a + fwd_mask, -1)

    @staticmethod
    def backward(ctx, gp):
        a, bwd_mask = ctx.saved_tensors
        p = torch.softmax(a + bwd_mask, -1)
        return p * (gp - (gp * p).sum(-1, keepdim=True)), None, None


@contextlib.contextmanager
def wrong_backward(kind, tokens=dc.MAX_TOKENS, length=dc.X_SHAPE[2]):
    """"nomask" / "token": forward_host forms `(a + attention_mask(...)).softmax(dim=-1)`: inside the context the mask it adds is zero, so
    the softmax call receives the plain scores; it applies the frame mask itself in the forward and differentiates under the other mask.
    "dit3d_ln" / "neighbour": dit1d_common.forward_host is _forward above with that LayerNorm backward."""
    plain, plain_mask, plain_fwd = torch.Tensor.softmax, dc.attention_mask, dc.forward_host
    if kind in ("dit3d_ln", "neighbour"):
        dc.forward_host = lambda params, x, levels, heads, mask="frame", residual="norm", dtype=torch.float64: _forward(
            params, x, levels, heads, mask, dtype, ln="dit3d" if kind == "dit3d_ln" else "neighbour")
    else:
        fwd = plain_mask(tokens, length, "frame", torch.float64)
        bwd = {"nomask": torch.zeros_like(fwd), "token": plain_mask(tokens, length, "token", torch.float64)}[kind]
        torch.Tensor.softmax = lambda self, dim=-1, **kw: _MaskedBackward.apply(self, fwd.to(self.dtype), bwd.to(self.dtype))
        dc.attention_mask = lambda t, l, mode, dtype: torch.zeros(t * l, t * l, dtype=dtype)
    try:
        yield
    finally:
        torch.Tensor.softmax, dc.attention_mask, dc.forward_host = plain, plain_mask, plain_fwd
