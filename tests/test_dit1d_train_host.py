"""Host-side checks of DiT1D training (no GPU): the dfot_dit1d_train_* family is declared, bound with the same arity and exported; the
constructor refuses by name what it does not build, before any device call; the host restatement's gradients have the parameter names of
the reference without the frozen pos_embed, and fp32 autograd is an adequate yardstick for them; and what a wrong attention backward
measures against that yardstick (the figures tests/test_gpu_dit1d_train.py quotes).

Fails on the parent commit: no DiT1DTrainer, no dfot_dit1d_train_* symbols."""
import ctypes as C
import os
import re

import pytest
import torch

import dit1d_common as dc
import dit1d_train_common as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = {"create": 2, "destroy": 1, "num_params": 1, "param_name": 2, "param_shape": 4, "param_offset": 2, "total_numel": 1, "load_buffer": 5,
          "attach": 3, "sync_weights": 2, "reserve": 2, "forward": 7, "backward": 3, "input_grad": 3}


@pytest.mark.parametrize("name", sorted(FAMILY))
def test_family_is_declared_bound_and_exported(name):
    from dfot_amd import capi
    sym = f"dfot_dit1d_train_{name}"
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dfot_hip.h")).read(), flags=re.S)
    m = re.search(r"\b" + sym + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, f"{sym} is not declared in include/dfot_hip.h"
    assert len(m.group(1).split(",")) == FAMILY[name] == len(capi.SIGNATURES[sym][1])
    assert getattr(capi.lib, sym) is not None
    assert sym in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_constructor_refusals_by_name():
    import dfot_amd
    cfg = dc.backbone_cfg(4)
    kw = dict(x_shape=dc.X_SHAPE, max_tokens=dc.MAX_TOKENS)
    for over, text in (({"use_fourier_noise_embedding": True}, "use_fourier_noise_embedding=True is not built"),
                       ({"merge_mode": "concat"}, "merge_mode='concat' is not built"), ({"use_rotary_emb": True}, "use_rotary_emb=True is not built"),
                       ({"qk_norm": True}, "qk_norm=True is not built"), ({"learn_sigma": True}, "learn_sigma=True is not built"),
                       ({"causal_attn_mode": "causal"}, "causal_attn_mode='causal' is unknown"),
                       ({"hidden_size": 192, "num_heads": 3}, "training needs multiples of 128"),
                       ({"hidden_size": 100}, "hidden_size=100 is outside the engine's limit")):
        with pytest.raises(ValueError, match=re.escape(text)):
            dfot_amd.DiT1DTrainer({**cfg, **over}, **kw)
    with pytest.raises(ValueError, match="is_continuous=True"):
        dfot_amd.DiT1DTrainer(cfg, diffusion=dfot_amd.DiffusionConfig(is_continuous=True), **kw)
    with pytest.raises(ValueError, match="external_cond_dim=3 is not built"):
        dfot_amd.DiT1DTrainer(cfg, external_cond_dim=3, **kw)
    with pytest.raises(ValueError, match=re.escape("x_shape[1] must be 1")):
        dfot_amd.DiT1DTrainer(cfg, x_shape=(4, 2, 32), max_tokens=8)
    with pytest.raises(ValueError, match="multiple of 128"):
        dfot_amd.DiT1DTrainer(cfg, x_shape=dc.X_SHAPE, max_tokens=3)
    assert issubclass(dfot_amd.DiT1DTrainer, dfot_amd.flat_optim.FlatAdamWOwner)


def _batch():
    x, k = dc.inputs()
    g = torch.Generator().manual_seed(5)
    masks = torch.ones(dc.BATCH, dc.MAX_TOKENS)
    masks[0, dc.MAX_TOKENS - 1] = 0
    return x, k, torch.randn(x.shape, generator=g), masks


def test_host_gradients_names_and_fp32_yardstick():
    xs, k, noise, masks = _batch()
    for tag in ("h4", "h2"):
        _, g64 = tc.host_loss_and_grads(tag, xs, k, noise, masks, torch.float64)
        _, g32 = tc.host_loss_and_grads(tag, xs, k, noise, masks, torch.float32)
        assert list(g64) == [n for n, _ in dc.key_shapes(tc.TRAIN_CASES[tag][0]) if n != "pos_embed"] and len(g64) == 28
        worst = max(dc.rel(g32[n], g64[n]) for n in g64)
        print(f"{tag}: fp32 autograd against fp64, worst gradient rel-L2 {worst:.2e}")
        assert worst < 5e-2 / 1000  # three orders of magnitude under the gradient bar


def test_training_gain_is_the_largest_at_which_bf16_operands_hold_half_the_bar():
    """dit1d_train_common.TRAIN_GAIN: plain autograd with the engine's bf16 roundings (forward_emulated) against fp32 autograd.  At the
    sampling fixture's gain it misses the 5e-2 gradient bar by itself; at TRAIN_GAIN it holds half of it in every case; one step of 0.25
    above it does not."""
    x, k = dc.inputs()
    d_out = torch.randn(x.shape, generator=torch.Generator().manual_seed(33))

    def worst(tag, gain):
        _, ref, ref_dx = tc.host_forward_backward(tag, x, k, d_out, gain=gain)
        _, em, em_dx = tc.host_forward_backward(tag, x, k, d_out, gain=gain, emulated=True)
        return max(max(dc.rel(em[n], ref[n]) for n in ref), dc.rel(em_dx, ref_dx))
    sampling = float(dc.load()["qk_gain"])
    assert tc.TRAIN_GAIN < sampling == 4.0
    at = {tag: worst(tag, tc.TRAIN_GAIN) for tag in tc.TRAIN_CASES}
    above = {tag: worst(tag, tc.TRAIN_GAIN + 0.25) for tag in tc.TRAIN_CASES}
    top = {tag: worst(tag, sampling) for tag in tc.TRAIN_CASES}
    print(f"bf16-operand emulation against fp32 autograd, worst of the gradients: gain {tc.TRAIN_GAIN} {at}; +0.25 {above}; {sampling} {top}")
    assert max(at.values()) < 5e-2 / 2 < max(above.values()) and min(top.values()) > 5e-2


@pytest.mark.parametrize("kind", ["nomask", "token"])
def test_a_wrong_attention_backward_misses_the_gradient_bar(kind):
    """the forward (hence the loss) unchanged, the attention backward recomputing its probabilities under another mask: everything an
    attention backward reaches misses 5e-2; without the mask the qkv weights miss by at least 5 x the bar (the condition under which
    TRAIN_GAIN was lowered), under the per-token mask by more than twice the bar"""
    xs, k, noise, masks = _batch()
    before = (torch.Tensor.softmax, dc.attention_mask, dc.forward_host)
    for tag in ("h4", "h2"):
        loss, ref = tc.host_loss_and_grads(tag, xs, k, noise, masks, torch.float64)
        with tc.wrong_backward(kind):
            wloss, wrong = tc.host_loss_and_grads(tag, xs, k, noise, masks, torch.float64)
        assert float(wloss) == float(loss)  # the loss proves nothing about the backward's mask
        rels = {n: dc.rel(wrong[n], ref[n]) for n in ref}
        missed = [n for n, r in rels.items() if r > 5e-2]
        qkv = [rels[f"blocks.{i}.attn.qkv.weight"] for i in range(2)]
        print(f"{tag} {kind}: {len(missed)} of {len(rels)} gradients miss 5e-2; attn.qkv.weight {qkv[0]:.2f} / {qkv[1]:.2f}")
        assert len(missed) == 20 and (kind != "nomask" or min(qkv) >= 5 * 5e-2) and min(qkv) > 2 * 5e-2
        exact = [n for n, r in rels.items() if r == 0.0]
        assert all(n.startswith(("blocks.1.attn.proj", "blocks.1.mlp", "final_layer")) for n in exact) and len(exact) == 8
    # the context restores what it patched
    assert (torch.Tensor.softmax, dc.attention_mask, dc.forward_host) == before and all(a is b for a, b in zip(
        (torch.Tensor.softmax, dc.attention_mask, dc.forward_host), before))


def _fixture():
    return dc.load("dit1d_train.npz")


def test_fixture_integrity():
    g = _fixture()
    xs, k = dc.inputs()
    assert str(g["inputs_digest"]) == dc.tensor_digest(xs, k)
    assert float(g["qk_gain"]) == tc.TRAIN_GAIN
    masks = dc.T(g["masks"])
    assert tuple(masks.shape) == (dc.BATCH, dc.MAX_TOKENS) and int((masks == 0).sum()) == 1 and int((masks == 1).sum()) == masks.numel() - 1
    for tag, (heads, _) in tc.TRAIN_CASES.items():
        names = [str(n) for n in g[f"{tag}_names"]]
        assert names == [n for n, _ in dc.key_shapes(heads) if n != "pos_embed"] and "pos_embed" not in names
        assert str(g[f"{tag}_digest"]) == dc.digest(tc.case_params(tag))
        assert len(g[f"{tag}_norms"]) == len(names) == 28 and min(g[f"{tag}_norms"]) > 0 and g[f"{tag}_norms"].dtype.name == "float64"
        assert tuple(g[f"{tag}_noise"].shape) == tuple(xs.shape) and float(g[f"{tag}_loss"]) > 0
        shapes = dict(dc.key_shapes(heads))
        stored = [key.split("/", 1)[1] for key in g.files if key.startswith(f"{tag}_grad/")]
        assert sorted(stored) == sorted(n for n in names if torch.Size(shapes[n]).numel() <= 4096) and len(stored) >= 14
        for n in stored:
            assert tuple(g[f"{tag}_grad/{n}"].shape) == tuple(shapes[n])
            assert abs(float(dc.T(g[f"{tag}_grad/{n}"]).double().norm()) - g[f"{tag}_norms"][names.index(n)]) < 1e-5 * g[f"{tag}_norms"][names.index(n)]
    assert float(g["nomask_qkv_weight"]) >= 5 * 5e-2


@pytest.mark.parametrize("tag", list(tc.TRAIN_CASES))
def test_host_restatement_matches_the_reference_fixture(tag):
    """the reference's own DFoTVideo training loss under its own autograd (tests/golden/dit1d_train.npz) against fp32 autograd through
    forward_host + oracle.sampler.discrete_training_loss: the loss and every gradient (norms for all 28, the stored tensors elementwise).
    The tool measured 0 for both (host_rel, host_loss_rel: the restatement is the reference's arithmetic op for op); the bar here, 1e-4, is
    what fp32 reassociation on another CPU or torch build may cost, 500 x under the gradient bar it stands in for."""
    g = _fixture()
    assert float(g["host_rel"]) < 1e-4 and float(g["host_loss_rel"]) < 1e-4
    xs, k = dc.inputs()
    loss, grads = tc.host_loss_and_grads(tag, xs, k, dc.T(g[f"{tag}_noise"]), dc.T(g["masks"]))
    ref_loss = float(g[f"{tag}_loss"])
    assert abs(float(loss) - ref_loss) < 1e-4 * abs(ref_loss)
    names = [str(n) for n in g[f"{tag}_names"]]
    assert names == list(grads)
    for n, ref_norm in zip(names, g[f"{tag}_norms"]):
        assert abs(float(grads[n].double().norm()) - ref_norm) < 1e-4 * ref_norm, n
    worst = max(dc.rel(grads[key.split("/", 1)[1]], dc.T(g[key])) for key in g.files if key.startswith(f"{tag}_grad/"))
    print(f"{tag}: host restatement against the reference fixture: loss {float(loss):.6f} / {ref_loss:.6f}, worst stored gradient rel-L2 {worst:.2e}")
    assert worst < 1e-4


def test_the_mutable_copy_of_forward_host_is_forward_host():
    """dit1d_train_common._forward with both switches off: forward_host's value and gradients, bit for bit"""
    g = _fixture()
    xs, k = dc.inputs()
    for tag in tc.TRAIN_CASES:
        noise, masks = dc.T(g[f"{tag}_noise"]), dc.T(g["masks"])
        loss, ref = tc.host_loss_and_grads(tag, xs, k, noise, masks, torch.float64)
        plain = dc.forward_host
        dc.forward_host = lambda p, x, lv, h, mask="frame", residual="norm", dtype=torch.float64: tc._forward(p, x, lv, h, mask, dtype)
        try:
            loss2, copy = tc.host_loss_and_grads(tag, xs, k, noise, masks, torch.float64)
        finally:
            dc.forward_host = plain
        assert torch.equal(loss2, loss) and all(torch.equal(copy[n], ref[n]) for n in ref)


@pytest.mark.parametrize("kind", ["dit3d_ln", "neighbour"])
def test_a_wrong_layer_norm_backward_misses_the_gradient_bar(kind):
    """the forward (hence the loss) unchanged, under the fixture's training loss, all three cases.  dit3d_ln -- the DiT3D LayerNorm
    backward, the residual gradient pushed through (1 + scale) and into dshift / dscale: 22 of the 28 gradients miss 5e-2 (all but the
    last block's MLP and the final layer, which lie behind every share_norm LayerNorm), the adaLN_modulation weights by 1.6 .. 1.9.
    neighbour -- the backward normalising with the neighbouring row's statistics: 16 .. 19 of 28 miss, the worst by 0.22 .. 0.31."""
    g = _fixture()
    xs, k = dc.inputs()
    before = dc.forward_host
    for tag in tc.TRAIN_CASES:
        noise, masks = dc.T(g[f"{tag}_noise"]), dc.T(g["masks"])
        loss, ref = tc.host_loss_and_grads(tag, xs, k, noise, masks, torch.float64)
        with tc.wrong_backward(kind):
            wloss, wrong = tc.host_loss_and_grads(tag, xs, k, noise, masks, torch.float64)
        assert float(wloss) == float(loss)
        rels = {n: dc.rel(wrong[n], ref[n]) for n in ref}
        missed = [n for n, r in rels.items() if r > 5e-2]
        mods = [rels[f"blocks.{i}.adaLN_modulation.1.weight"] for i in range(2)]
        print(f"{tag} {kind}: {len(missed)} of {len(rels)} gradients miss 5e-2, worst {max(rels.values()):.2f}; adaLN_modulation.1.weight "
              f"{mods[0]:.2f} / {mods[1]:.2f}")
        untouched = [n for n, r in rels.items() if r == 0.0]
        assert sorted(untouched) == sorted(n for n in ref if n.startswith(("blocks.1.mlp", "final_layer"))) and len(untouched) == 6
        if kind == "dit3d_ln":
            assert len(missed) == 22 and min(mods) > 1.0
        else:
            assert len(missed) >= 14 and max(rels.values()) >= 4 * 5e-2
    assert dc.forward_host is before
