"""torch.library registration of the engine's entry points (namespace ``dfot``).

The reference is a PyTorch program; its natural plug-in surface is a set of torch operators.  Each operator below is a thin
shim over one C-ABI call of libdfot_hip.so (``capi``) with a fake ("meta") implementation for shape inference, so that
FakeTensor tracing, ``torch.compile`` graphs and stream capture treat the HIP kernels as opaque ops:

    dfot::uvit3d_pose_forward(x, noise_levels, external_cond, external_cond_mask?, model) -> v      [dfot_uvit_forward]
    dfot::uvit3d_pose_forward_train(x, noise_levels, external_cond, mask?, params[], model) -> v    [autograd: dfot_op_* forward/backward]
    dfot::uvit3d_forward(x, noise_levels (float), external_cond?, external_cond_mask?, model) -> v  [dfot_uvit3d_forward_live]
    dfot::dit3d_forward(x, noise_levels, model) -> v                                                [dfot_dit_forward]
    dfot::dit3d_forward_cond(x, noise_levels, external_cond, external_cond_mask?, model) -> v       [dfot_dit_forward_cond]
    dfot::dit3d_forward_f(x, noise_levels (float), external_cond?, external_cond_mask?, model) -> v [dfot_dit_forward_f]
    dfot::dit3d_forward_f_train(x, noise_levels (float), external_cond?, mask?, params[], model) -> v  [autograd: dfot_dit_train_forward_f]
    dfot::dit1d_forward(x, noise_levels, model) -> v                                                [dfot_dit1d_forward]
    dfot::frame_causal_attention(q, k, v, frame_len) -> o                    [autograd: dfot_op_attention_frame_causal_lse / _bwd]
    dfot::attention_seq64(q, k, v) -> o                                      [autograd: dfot_op_attention_seq64 / _seq64_bwd]
    dfot::ray_encoding(raw_poses, resolution) -> cond                                               [dfot_ray_encode]
    dfot::hg_prepare(x, noise?, qa, qb, nfe) -> x_in                                                [dfot_hg_prepare]
    dfot::ddim_hg_step(x, x_in, v, sa, s1, an, cn, keep, weight, gen, nfe) -> x_next                [dfot_ddim_compose / _tokw]
    dfot::dit_final_layer(x, table, levels, off, weight, bias, eps, c, h, w, patch, form) -> out    [dfot_op_dit_final_layer]

``model`` is an integer key of a live backbone module (``register_model``): operators take tensors and scalars only.
The nn.Module mirrors (`UViT3DPose`, `UViT3D`, `DiT3D`, `DifferenceDiT3D`, `DiT1D`) dispatch their ``forward`` through these operators and the
sampler's ``_process_conditions`` through ``dfot::ray_encoding``; the sampler's step loop calls the same C entry points
directly (it re-uses its output buffers across steps), ``dfot::hg_prepare`` / ``dfot::ddim_hg_step`` are the functional forms
for a host that drives the step itself.
"""
from __future__ import annotations

import weakref
from typing import List, Optional

import torch
from torch import Tensor
from torch.library import custom_op

from . import capi

_MODELS: "weakref.WeakValueDictionary[int, torch.nn.Module]" = weakref.WeakValueDictionary()


def register_model(module: torch.nn.Module) -> int:
    key = id(module)
    _MODELS[key] = module
    return key


def _model(key: int):
    try:
        return _MODELS[key]
    except KeyError:
        raise RuntimeError(f"dfot: backbone {key} is not registered (or was garbage-collected)") from None


@custom_op("dfot::uvit3d_pose_forward", mutates_args=())
def uvit3d_pose_forward(x: Tensor, noise_levels: Tensor, external_cond: Tensor, external_cond_mask: Optional[Tensor],
                        model: int) -> Tensor:
    return _model(model)._forward_impl(x, noise_levels, external_cond, external_cond_mask)


@uvit3d_pose_forward.register_fake
def _(x, noise_levels, external_cond, external_cond_mask, model):
    return torch.empty_like(x)


# the pose-free U-ViT (uvit3d_backbone.UViT3D): float levels, optional actions (B, T, dim) and the optional per-video uint8 mask (B,)
@custom_op("dfot::uvit3d_forward", mutates_args=())
def uvit3d_forward(x: Tensor, noise_levels: Tensor, external_cond: Optional[Tensor], external_cond_mask: Optional[Tensor], model: int) -> Tensor:
    return _model(model)._forward_impl(x, noise_levels, external_cond, external_cond_mask)


@uvit3d_forward.register_fake
def _(x, noise_levels, external_cond, external_cond_mask, model):
    return torch.empty_like(x)


# ---- training form: the same backbone under autograd -------------------------------------------------------------------
# `params` are the module's trainable tensors in `model._train_names` order; they are operator inputs so that autograd hands
# their gradients back (torch.library.register_autograd).  Forward = the saved-activation forward of uvit_train.UViT3DPoseTrainer
# on the module's current weights, backward = its hand-written backward: what `accelerator.backward(loss)` walks into when the
# reference's training_step calls `self.model(x_t, precond_scale * logsnr, external_cond)` (continuous_diffusion.py:154,
# experiments/simple_video_generation.py:260-270).  The gradient w.r.t. x is produced only when x requires it: training never
# differentiates w.r.t. x_t, reconstruction guidance does (discrete_diffusion.py:485-513: torch.autograd.grad(guidance_loss, x)).
@custom_op("dfot::uvit3d_pose_forward_train", mutates_args=())
def uvit3d_pose_forward_train(x: Tensor, noise_levels: Tensor, external_cond: Tensor, external_cond_mask: Optional[Tensor],
                              params: List[Tensor], model: int) -> Tensor:
    return _model(model)._train_forward_impl(x, noise_levels, external_cond, external_cond_mask, params)


@uvit3d_pose_forward_train.register_fake
def _(x, noise_levels, external_cond, external_cond_mask, params, model):
    return torch.empty_like(x)


# `stamp` = the module's training-forward counter at the time of the forward this backward belongs to: the saved activations live
# in the module's ONE engine, so a second training forward before this backward has overwritten them -- the backward then raises
# instead of returning the gradients of another input (forward, forward, backward, backward is refused; run backward after each
# forward, e.g. gradient accumulation as forward/backward pairs).
@custom_op("dfot::uvit3d_pose_backward", mutates_args=())
def uvit3d_pose_backward(grad_out: Tensor, params: List[Tensor], model: int, stamp: int, want_dx: bool = False) -> List[Tensor]:
    return _model(model)._train_backward_impl(grad_out, params, stamp, want_dx)


@uvit3d_pose_backward.register_fake
def _(grad_out, params, model, stamp, want_dx=False):
    return [torch.empty_like(p) for p in params] + ([torch.empty_like(grad_out)] if want_dx else [])


def _train_setup_context(ctx, inputs, output):
    ctx.params = inputs[4]
    ctx.model = inputs[5]
    ctx.stamp = _model(inputs[5])._train_stamp  # setup_context runs right after the forward it describes


def _train_backward(ctx, grad_out):
    want_dx = bool(ctx.needs_input_grad[0])
    grads = torch.ops.dfot.uvit3d_pose_backward(grad_out.contiguous(), ctx.params, ctx.model, ctx.stamp, want_dx)
    dx = None
    if want_dx:
        dx = grads[-1].view_as(grad_out)
        grads = grads[:-1]
    return dx, None, None, None, grads, None


uvit3d_pose_forward_train.register_autograd(_train_backward, setup_context=_train_setup_context)


@custom_op("dfot::dit3d_forward", mutates_args=())
def dit3d_forward(x: Tensor, noise_levels: Tensor, model: int) -> Tensor:
    return _model(model)._forward_impl(x, noise_levels)


@dit3d_forward.register_fake
def _(x, noise_levels, model):
    return torch.empty_like(x)


# the same forward with an external condition per (video, token): fp32 actions (B, T, cond_dim) or int32 labels (B, T), and the
# optional per-video uint8 mask (B,) of the videos that run without it
@custom_op("dfot::dit3d_forward_cond", mutates_args=())
def dit3d_forward_cond(x: Tensor, noise_levels: Tensor, external_cond: Tensor, external_cond_mask: Optional[Tensor], model: int) -> Tensor:
    return _model(model)._forward_impl(x, noise_levels, external_cond, external_cond_mask)


@dit3d_forward_cond.register_fake
def _(x, noise_levels, external_cond, external_cond_mask, model):
    return torch.empty_like(x)


# DiT3D / DifferenceDiT3D under autograd: as uvit3d_pose_forward_train, backed by trainer.DiT3DTrainer (dfot_dit_train_*)
@custom_op("dfot::dit3d_forward_train", mutates_args=())
def dit3d_forward_train(x: Tensor, noise_levels: Tensor, params: List[Tensor], model: int) -> Tensor:
    return _model(model)._train_forward_impl(x, noise_levels, params)


@dit3d_forward_train.register_fake
def _(x, noise_levels, params, model):
    return torch.empty_like(x)


@custom_op("dfot::dit3d_backward", mutates_args=())
def dit3d_backward(grad_out: Tensor, params: List[Tensor], model: int, stamp: int, want_dx: bool = False) -> List[Tensor]:
    return _model(model)._train_backward_impl(grad_out, params, stamp, want_dx)


@dit3d_backward.register_fake
def _(grad_out, params, model, stamp, want_dx=False):
    return [torch.empty_like(p) for p in params] + ([torch.empty_like(grad_out)] if want_dx else [])


def _dit_train_setup_context(ctx, inputs, output):
    ctx.params = inputs[2]
    ctx.model = inputs[3]
    ctx.stamp = _model(inputs[3])._train_stamp


def _dit_train_backward(ctx, grad_out):
    want_dx = bool(ctx.needs_input_grad[0])
    grads = torch.ops.dfot.dit3d_backward(grad_out.contiguous(), ctx.params, ctx.model, ctx.stamp, want_dx)
    dx = None
    if want_dx:
        dx, grads = grads[-1], grads[:-1]
    return dx, None, grads, None


dit3d_forward_train.register_autograd(_dit_train_backward, setup_context=_dit_train_setup_context)


@custom_op("dfot::dit3d_forward_cond_train", mutates_args=())
def dit3d_forward_cond_train(x: Tensor, noise_levels: Tensor, external_cond: Tensor, external_cond_mask: Optional[Tensor],
                             params: List[Tensor], model: int) -> Tensor:
    return _model(model)._train_forward_impl(x, noise_levels, params, external_cond, external_cond_mask)


@dit3d_forward_cond_train.register_fake
def _(x, noise_levels, external_cond, external_cond_mask, params, model):
    return torch.empty_like(x)


def _dit_cond_train_setup_context(ctx, inputs, output):
    ctx.params = inputs[4]
    ctx.model = inputs[5]
    ctx.stamp = _model(inputs[5])._train_stamp


def _dit_cond_train_backward(ctx, grad_out):
    dx, _, grads, _ = _dit_train_backward(ctx, grad_out)
    return dx, None, None, None, grads, None


dit3d_forward_cond_train.register_autograd(_dit_cond_train_backward, setup_context=_dit_cond_train_setup_context)


# ---- float noise levels (a DiT3D / DifferenceDiT3D built with use_fourier_noise_embedding, under ContinuousDiffusion): one operator
# for the unconditioned and the conditioned call (external_cond None / given), and its training form with the backward of the int ops
@custom_op("dfot::dit3d_forward_f", mutates_args=())
def dit3d_forward_f(x: Tensor, noise_levels: Tensor, external_cond: Optional[Tensor], external_cond_mask: Optional[Tensor], model: int) -> Tensor:
    return _model(model)._forward_impl(x, noise_levels, external_cond, external_cond_mask)


@dit3d_forward_f.register_fake
def _(x, noise_levels, external_cond, external_cond_mask, model):
    return torch.empty_like(x)


@custom_op("dfot::dit3d_forward_f_train", mutates_args=())
def dit3d_forward_f_train(x: Tensor, noise_levels: Tensor, external_cond: Optional[Tensor], external_cond_mask: Optional[Tensor],
                          params: List[Tensor], model: int) -> Tensor:
    return _model(model)._train_forward_impl(x, noise_levels, params, external_cond, external_cond_mask)


@dit3d_forward_f_train.register_fake
def _(x, noise_levels, external_cond, external_cond_mask, params, model):
    return torch.empty_like(x)


dit3d_forward_f_train.register_autograd(_dit_cond_train_backward, setup_context=_dit_cond_train_setup_context)


# the DiT1D backbone (dit1d_backbone.DiT1D): integer levels, no condition; forward only
@custom_op("dfot::dit1d_forward", mutates_args=())
def dit1d_forward(x: Tensor, noise_levels: Tensor, model: int) -> Tensor:
    return _model(model)._forward_impl(x, noise_levels)


@dit1d_forward.register_fake
def _(x, noise_levels, model):
    return torch.empty_like(x)


# ---- frame-causal attention as a differentiable operator: the drop-in for the reference DiT1D's
# F.scaled_dot_product_attention(q, k, v, attn_mask=<block lower triangular>) (dit1d/dit_model.py:57-88) ---------------------------------
# q, k, v (B, heads, N, d) of one floating dtype on the GPU; o = softmax(q k^T / sqrt(d) + mask) v with mask[i, j] = -inf iff
# j // frame_len > i // frame_len, in q's shape and dtype.  The result is a transposed view of the kernel's compact (B, N, heads, d)
# buffer, so the reference's `x.transpose(1, 2).reshape(B, N, C)` is a view.  Host plumbing in torch: q, k, v are packed into the kernels'
# [B][heads][N][dstride] bf16 layout (pad columns zero, q times log2(e)/sqrt(d) BEFORE the bf16 rounding, as the engines' QKV epilogue
# does); the gradients come back in the inputs' dtype, first d columns.
_FC_FRAME_LENS = (16, 32, 64, 128)
_LOG2E = 1.4426950408889634


def _fc_check(q: Tensor, k: Tensor, v: Tensor, frame_len: int, need_gpu: bool = True):
    if q.dim() != 4 or k.shape != q.shape or v.shape != q.shape:
        raise ValueError(f"frame_causal_attention: q, k, v must share one (B, heads, N, d) shape, got {tuple(q.shape)}, {tuple(k.shape)}, "
                         f"{tuple(v.shape)}")
    if not q.is_floating_point() or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError(f"frame_causal_attention: q, k, v must share one floating dtype, got {q.dtype}, {k.dtype}, {v.dtype}")
    b, heads, n, d = q.shape
    if frame_len not in _FC_FRAME_LENS:
        raise ValueError(f"frame_causal_attention: frame_len {frame_len} not in {_FC_FRAME_LENS}")
    if n <= 0 or n % 128 != 0:
        raise ValueError(f"frame_causal_attention: N={n} must be a positive multiple of 128")
    if d <= 0 or d % 8 != 0 or d > 128:
        raise ValueError(f"frame_causal_attention: head dim {d} must be a multiple of 8, <= 128")
    if b <= 0 or heads <= 0:
        raise ValueError(f"frame_causal_attention: batch {b} and heads {heads} must be positive")
    if need_gpu and not (q.is_cuda and k.is_cuda and v.is_cuda):
        raise ValueError(f"frame_causal_attention: q, k, v are on {q.device}, {k.device}, {v.device}: GPU tensors only (there is no CPU path)")
    return b, heads, n, d


def _fc_pack(t: Tensor, d: int, mul: float = 1.0) -> Tensor:
    """(B, heads, N, d) of any strides -> contiguous [B][heads][N][dstride] bf16, pad columns zero; the product with `mul` is taken in fp32.
    The pack of both attention operators (frame_causal_attention above, attention_seq64 below)"""
    ds = 64 if d <= 64 else 128
    src = t.detach().float() * mul if mul != 1.0 else t.detach()
    if ds == d:
        return src.to(torch.bfloat16).contiguous()
    out = torch.zeros(*t.shape[:3], ds, dtype=torch.bfloat16, device=t.device)
    out[..., :d] = src
    return out


# what the last forward left for its backward: (packed q, k, v, compact o, lse).  register_autograd's setup_context sees the operator's
# inputs and output only; it runs right after the forward it describes (same thread), takes the entry and clears it
_FC_SAVED = None


@custom_op("dfot::frame_causal_attention", mutates_args=())
def frame_causal_attention(q: Tensor, k: Tensor, v: Tensor, frame_len: int) -> Tensor:
    global _FC_SAVED
    b, heads, n, d = _fc_check(q, k, v, frame_len)
    qp, kp, vp = _fc_pack(q, d, _LOG2E / d ** 0.5), _fc_pack(k, d), _fc_pack(v, d)
    o = torch.empty(b * n, heads * d, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(b, heads, n, dtype=torch.float32, device=q.device)
    capi.check(capi.lib.dfot_op_attention_frame_causal_lse(capi.ptr(qp), capi.ptr(kp), capi.ptr(vp), capi.ptr(o), heads * d, capi.ptr(lse),
                                                           b, heads, n, frame_len, d, capi.stream_ptr()))
    out = o.view(b, n, heads, d).transpose(1, 2)
    out = out if q.dtype == torch.bfloat16 else out.to(q.dtype)  # .to keeps the strides: still compact as (B, N, heads, d)
    _FC_SAVED = (out.data_ptr(), qp, kp, vp, o, lse)
    return out


@frame_causal_attention.register_fake
def _(q, k, v, frame_len):
    b, heads, n, d = _fc_check(q, k, v, frame_len, need_gpu=False)
    return q.new_empty((b, n, heads, d)).transpose(1, 2)


@custom_op("dfot::frame_causal_attention_backward", mutates_args=())
def frame_causal_attention_backward(grad_out: Tensor, qp: Tensor, kp: Tensor, vp: Tensor, o: Tensor, lse: Tensor, frame_len: int,
                                    d: int) -> List[Tensor]:
    b, heads, n, _ = qp.shape
    d_o = grad_out.detach().transpose(1, 2).to(torch.bfloat16).contiguous().view(b * n, heads * d)
    delta = torch.empty_like(lse)
    dq, dk, dv = (torch.empty_like(qp) for _ in range(3))
    capi.check(capi.lib.dfot_op_attention_frame_causal_bwd(capi.ptr(qp), capi.ptr(kp), capi.ptr(vp), capi.ptr(o), capi.ptr(d_o), heads * d,
                                                           capi.ptr(lse), capi.ptr(delta), capi.ptr(dq), capi.ptr(dk), capi.ptr(dv), b, heads, n,
                                                           frame_len, d, capi.stream_ptr()))
    return [t[..., :d].to(grad_out.dtype) for t in (dq, dk, dv)]


@frame_causal_attention_backward.register_fake
def _(grad_out, qp, kp, vp, o, lse, frame_len, d):
    return [grad_out.new_empty((*qp.shape[:3], d)) for _ in range(3)]


def _fc_setup_context(ctx, inputs, output):
    global _FC_SAVED
    saved, _FC_SAVED = _FC_SAVED, None
    if saved is None or saved[0] != output.data_ptr():
        raise RuntimeError("dfot::frame_causal_attention: the forward left no saved operands for this output (the operator is not "
                           "differentiable under FakeTensor tracing)")
    ctx.save_for_backward(*saved[1:])
    ctx.frame_len, ctx.d = inputs[3], inputs[0].shape[3]


def _fc_backward(ctx, grad_out):
    dq, dk, dv = torch.ops.dfot.frame_causal_attention_backward(grad_out, *ctx.saved_tensors, ctx.frame_len, ctx.d)
    return dq, dk, dv, None


frame_causal_attention.register_autograd(_fc_backward, setup_context=_fc_setup_context)


# ---- attention over 64-token sequences as a differentiable operator: the drop-in for the F.scaled_dot_product_attention(q, k, v) that the
# reference's spatial DiTBlock issues per frame at 64 patches per frame (the taichi res-128 recipes) ------------------------------------
# q, k, v (F, heads, 64, d) of one floating dtype on the GPU, F = the number of sequences (frames); o = softmax(q k^T / sqrt(d)) v in q's
# shape and dtype, a transposed view of the kernel's compact (F, 64, heads, d) buffer.  Host plumbing as frame_causal_attention above (_fc_pack
# serves both).  The backward kernel recomputes the 64 x 64 softmax, so the forward saves the packed q, k, v and nothing else.
def _s64_check(q: Tensor, k: Tensor, v: Tensor, need_gpu: bool = True):
    if q.dim() != 4 or k.shape != q.shape or v.shape != q.shape:
        raise ValueError(f"attention_seq64: q, k, v must share one (F, heads, 64, d) shape, got {tuple(q.shape)}, {tuple(k.shape)}, "
                         f"{tuple(v.shape)}")
    if not q.is_floating_point() or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError(f"attention_seq64: q, k, v must share one floating dtype, got {q.dtype}, {k.dtype}, {v.dtype}")
    f, heads, n, d = q.shape
    if n != 64:
        raise ValueError(f"attention_seq64: N={n} must be 64")
    if d <= 0 or d % 8 != 0 or d > 128:
        raise ValueError(f"attention_seq64: head dim {d} must be a multiple of 8, <= 128")
    if f <= 0 or heads <= 0:
        raise ValueError(f"attention_seq64: sequences {f} and heads {heads} must be positive")
    if need_gpu and not (q.is_cuda and k.is_cuda and v.is_cuda):
        raise ValueError(f"attention_seq64: q, k, v are on {q.device}, {k.device}, {v.device}: GPU tensors only (there is no CPU path)")
    return f, heads, d


# what the last forward left for its backward: (packed q, k, v), handed over as _FC_SAVED is
_S64_SAVED = None


@custom_op("dfot::attention_seq64", mutates_args=())
def attention_seq64(q: Tensor, k: Tensor, v: Tensor) -> Tensor:
    global _S64_SAVED
    f, heads, d = _s64_check(q, k, v)
    qp, kp, vp = _fc_pack(q, d, _LOG2E / d ** 0.5), _fc_pack(k, d), _fc_pack(v, d)
    o = torch.empty(f * 64, heads * d, dtype=torch.bfloat16, device=q.device)
    capi.check(capi.lib.dfot_op_attention_seq64(capi.ptr(qp), capi.ptr(kp), capi.ptr(vp), capi.ptr(o), heads * d, f, heads, d, capi.stream_ptr()))
    out = o.view(f, 64, heads, d).transpose(1, 2)
    out = out if q.dtype == torch.bfloat16 else out.to(q.dtype)  # .to keeps the strides: still compact as (F, 64, heads, d)
    _S64_SAVED = (out.data_ptr(), qp, kp, vp)
    return out


@attention_seq64.register_fake
def _(q, k, v):
    f, heads, d = _s64_check(q, k, v, need_gpu=False)
    return q.new_empty((f, 64, heads, d)).transpose(1, 2)


@custom_op("dfot::attention_seq64_backward", mutates_args=())
def attention_seq64_backward(grad_out: Tensor, qp: Tensor, kp: Tensor, vp: Tensor, d: int) -> List[Tensor]:
    f, heads = qp.shape[:2]
    d_o = grad_out.detach().transpose(1, 2).to(torch.bfloat16).contiguous().view(f * 64, heads * d)
    dq, dk, dv = (torch.empty_like(qp) for _ in range(3))
    capi.check(capi.lib.dfot_op_attention_seq64_bwd(capi.ptr(qp), capi.ptr(kp), capi.ptr(vp), capi.ptr(d_o), heads * d, capi.ptr(dq), capi.ptr(dk),
                                                    capi.ptr(dv), f, heads, d, capi.stream_ptr()))
    return [t[..., :d].to(grad_out.dtype) for t in (dq, dk, dv)]


@attention_seq64_backward.register_fake
def _(grad_out, qp, kp, vp, d):
    return [grad_out.new_empty((*qp.shape[:3], d)) for _ in range(3)]


def _s64_setup_context(ctx, inputs, output):
    global _S64_SAVED
    saved, _S64_SAVED = _S64_SAVED, None
    if saved is None or saved[0] != output.data_ptr():
        raise RuntimeError("dfot::attention_seq64: the forward left no saved operands for this output (the operator is not differentiable "
                           "under FakeTensor tracing)")
    ctx.save_for_backward(*saved[1:])
    ctx.d = inputs[0].shape[3]


def _s64_backward(ctx, grad_out):
    dq, dk, dv = torch.ops.dfot.attention_seq64_backward(grad_out, *ctx.saved_tensors, ctx.d)
    return dq, dk, dv


attention_seq64.register_autograd(_s64_backward, setup_context=_s64_setup_context)


@custom_op("dfot::ray_encoding", mutates_args=())
def ray_encoding(raw_poses: Tensor, resolution: int, normalized: bool = False) -> Tensor:
    """normalized = False: poses are raw and become relative to frame 0 (the reference's default, normalize_by "first");
    True: the caller already expressed them in its world frame (pose.normalize_poses)"""
    b, t = raw_poses.shape[:2]
    raw = raw_poses.detach().to(device="cuda", dtype=torch.float32).contiguous()
    out = torch.empty(b, t, 180, resolution, resolution, device="cuda", dtype=torch.float32)
    fn = capi.lib.dfot_ray_encode_normalized if normalized else capi.lib.dfot_ray_encode
    capi.check(fn(capi.ptr(raw), capi.ptr(out), b, t, resolution, capi.stream_ptr()))
    return out


@ray_encoding.register_fake
def _(raw_poses, resolution, normalized=False):
    b, t = raw_poses.shape[:2]
    return raw_poses.new_empty((b, t, 180, resolution, resolution), dtype=torch.float32)


@custom_op("dfot::hg_prepare", mutates_args=())
def hg_prepare(x: Tensor, noise: Optional[Tensor], qa: Tensor, qb: Tensor, nfe: int) -> Tensor:
    b, t = x.shape[:2]
    f = x[0, 0].numel()
    F32 = torch.float32
    for name, tab in (("qa", qa), ("qb", qb)):
        if tuple(tab.shape) != (b * nfe, t):
            raise ValueError(f"{name} has shape {tuple(tab.shape)}, expected {(b * nfe, t)}")
    if noise is not None and tuple(noise.shape) != (b * nfe, *x.shape[1:]):
        raise ValueError(f"noise has shape {tuple(noise.shape)}, expected {(b * nfe, *x.shape[1:])}")
    px, pn, pa, pb = capi.ptr(x, F32, "x"), capi.ptr(noise, F32, "noise"), capi.ptr(qa, F32, "qa"), capi.ptr(qb, F32, "qb")
    x_in = torch.empty(b * nfe, *x.shape[1:], device=x.device, dtype=torch.float32)
    capi.check(capi.lib.dfot_hg_prepare(px, pn, pa, pb, capi.ptr(x_in), b, nfe, t, f, capi.stream_ptr()))
    return x_in


@hg_prepare.register_fake
def _(x, noise, qa, qb, nfe):
    return x.new_empty((x.shape[0] * nfe, *x.shape[1:]))


@custom_op("dfot::ddim_hg_step", mutates_args=())
def ddim_hg_step(x: Tensor, x_in: Tensor, v: Tensor, sa: Tensor, s1: Tensor, an: Tensor, cn: Tensor, keep: Tensor,
                 weight: Tensor, gen: Tensor, nfe: int) -> Tensor:
    b, t = x.shape[:2]
    f = x[0, 0].numel()
    F32 = torch.float32
    for name, big in (("x_in", x_in), ("v", v)):
        if tuple(big.shape) != (b * nfe, *x.shape[1:]):
            raise ValueError(f"{name} has shape {tuple(big.shape)}, expected {(b * nfe, *x.shape[1:])}")
    tabs = dict(sa=sa, s1=s1, an=an, cn=cn, keep=keep)
    for name, tab in tabs.items():
        if tuple(tab.shape) != (b * nfe, t):
            raise ValueError(f"{name} has shape {tuple(tab.shape)}, expected {(b * nfe, t)}")
    if tuple(gen.shape) != (b, t):
        raise ValueError(f"gen has shape {tuple(gen.shape)}, expected {(b, t)}")
    tokw = weight.ndim == 2
    if (tokw and tuple(weight.shape) != (nfe, t)) or (not tokw and tuple(weight.shape) != (nfe,)):
        raise ValueError(f"weight has shape {tuple(weight.shape)}, expected {(nfe,)} or {(nfe, t)}")
    ptrs = [capi.ptr(x, F32, "x"), capi.ptr(x_in, F32, "x_in"), capi.ptr(v, F32, "v")]
    ptrs += [capi.ptr(tab, F32, name) for name, tab in tabs.items()]
    ptrs += [capi.ptr(weight, F32, "weight"), capi.ptr(gen, torch.uint8, "gen")]
    x_next = torch.empty_like(x)
    fn = capi.lib.dfot_ddim_compose_tokw if tokw else capi.lib.dfot_ddim_compose
    capi.check(fn(*ptrs, capi.ptr(x_next), b, nfe, t, f, capi.stream_ptr()))
    return x_next


@ddim_hg_step.register_fake
def _(x, x_in, v, sa, s1, an, cn, keep, weight, gen, nfe):
    return torch.empty_like(x)


# the DiT final layer alone (AdaLN -> Linear -> unpatchify): x [rows][hidden], table [levels][ldt] with (shift | scale) at column `off`,
# levels int32 [frames], weight [patch * patch * channels][hidden] -> [frames][channels][height][width].  form 0 = the engine's choice,
# 1 = the LDS-resident kernel (an error when the weight does not fit), 2 = the chunked kernel
@custom_op("dfot::dit_final_layer", mutates_args=())
def dit_final_layer(x: Tensor, table: Tensor, levels: Tensor, off: int, weight: Tensor, bias: Tensor, eps: float, channels: int, height: int,
                    width: int, patch: int, form: int) -> Tensor:
    F32 = torch.float32
    if x.ndim != 2 or weight.ndim != 2 or table.ndim != 2 or weight.shape[1] != x.shape[1]:
        raise ValueError(f"x {tuple(x.shape)}, table {tuple(table.shape)}, weight {tuple(weight.shape)}: expected (rows, hidden), (levels, ldt), (oc, hidden)")
    oc = patch * patch * channels
    if tuple(weight.shape) != (oc, x.shape[1]) or tuple(bias.shape) != (oc,):
        raise ValueError(f"weight {tuple(weight.shape)} / bias {tuple(bias.shape)}, expected {(oc, x.shape[1])} / {(oc,)}")
    per_frame = (height // patch) * (width // patch)
    if per_frame <= 0 or x.shape[0] % per_frame != 0 or tuple(levels.shape) != (x.shape[0] // per_frame,):
        raise ValueError(f"{x.shape[0]} rows of {per_frame} per frame need levels of shape {(x.shape[0] // max(per_frame, 1),)}, got {tuple(levels.shape)}")
    frames = x.shape[0] // per_frame
    out = torch.empty(frames, channels, height, width, device=x.device, dtype=F32)
    capi.check(capi.lib.dfot_op_dit_final_layer(capi.ptr(x, F32, "x"), capi.ptr(table, F32, "table"), capi.ptr(levels, torch.int32, "levels"),
                                                table.shape[1], off, capi.ptr(weight, F32, "weight"), capi.ptr(bias, F32, "bias"), capi.ptr(out),
                                                x.shape[1], per_frame, x.shape[0], eps, table.shape[0] - 1, channels, height, width, patch, form,
                                                capi.stream_ptr()))
    return out


@dit_final_layer.register_fake
def _(x, table, levels, off, weight, bias, eps, channels, height, width, patch, form):
    return x.new_empty((levels.shape[0], channels, height, width))
