"""Host-side checks of the Minecraft / dmlab DiT recipe (no GPU): the C entry points of the final layer, the fixture's weight digest, and
the restatement used as the GPU yardstick against the reference's own forward at 32 channels."""
import os
import re

import pytest
import torch

import dit_cont_common as cc
import dit_mcraft_common as mc
from conftest import GOLDEN
from dit_mcraft_common import T, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_args(name):
    text = open(os.path.join(ROOT, "include", "dfot_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, f"{name} is not declared in include/dfot_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,count,last_int", [("dfot_op_dit_final_layer", 19, "form"), ("dfot_op_dit_final_layer_chunked", 19, "chunk")])
def test_final_layer_entry_points_are_declared_bound_and_exported(name, count, last_int):
    """x, table, levels, ldt, off, w, b, out, hidden, rows_per_frame, rows, eps, max_level, c, h, w, patch, form | chunk, stream"""
    from dfot_amd import capi
    args = _declared_args(name)
    assert len(args) == count and args[-2] == f"int {last_int}" and args[-1] == "void* stream"
    res, bound = capi.SIGNATURES[name]
    assert len(bound) == count
    assert getattr(capi.lib, name) is not None  # exported by the built library
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_fixture_digests_are_those_of_the_seeded_weights():
    g = load("dit_mcraft.npz")
    cfg = mc.ocfg()
    assert os.path.getsize(os.path.join(GOLDEN, "dit_mcraft.npz")) < 1_000_000
    assert cc.digest(mc.seeded_params(cfg, False, [str(n) for n in g["names"]])) == str(g["digest"])
    assert cc.digest(mc.seeded_params(cfg, True, [str(n) for n in g["act_names"]])) == str(g["act_digest"])
    # the generator script names the same model
    src = open(os.path.join(ROOT, "tools", "make_golden_dit_mcraft.py")).read()
    assert "mc.ocfg()" in src and "mc.seeded_params(cfg, action, names)" in src
    assert (cfg.hidden_size, cfg.depth, cfg.num_heads, cfg.in_channels, cfg.patch_size, cfg.max_tokens) == (384, 2, 6, 32, 2, 16)


def test_restatement_agrees_with_the_reference_forward_at_32_channels():
    """fp32 on the CPU, as tests/test_oracle_dit.py holds oracle.dit to its fixture: the evidence that the yardstick of the GPU tests is
    right at this geometry, with and without the action embedding and its per-video mask"""
    g = load("dit_mcraft.npz")
    cfg = mc.ocfg()
    x, lv = T(g["x"]), T(g["levels"])
    with torch.no_grad():
        out = mc.forward(mc.seeded_params(cfg, False), cfg, x, lv)
        act = mc.forward(mc.seeded_params(cfg, True), cfg, x, lv, T(g["cond"]), T(g["mask"]))
    torch.testing.assert_close(out, T(g["out"]), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(act, T(g["act_out"]), rtol=1e-4, atol=1e-4)
    assert torch.equal(act[0], out[0]) and not torch.equal(act[1], out[1])  # the masked video is the unconditioned one


def test_final_layer_restatement_is_the_oracle_forwards_tail():
    """final_layer_fp64 (the op tests' yardstick) on the oracle's own last-block output reproduces the oracle's output"""
    import torch.nn.functional as F
    from oracle import dit as odit
    cfg = mc.ocfg(depth=1)
    p = odit.seeded_params(cfg, 4)
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(1, 8, *mc.X_SHAPE, generator=gen)
    k = torch.randint(0, 1000, (1, 8), generator=gen)
    taps = {}
    with torch.no_grad():
        want = odit.forward(p, cfg, x, k, taps)
        pre = "dit_base.final_layer.norm_final.modulation.1"
        mod = F.linear(F.silu(taps["emb"].reshape(8, -1).double()), p[f"{pre}.weight"].double(), p[f"{pre}.bias"].double())
        got = mc.final_layer_fp64(taps["block0"].reshape(8 * 16, -1), mod, p["dit_base.final_layer.linear.weight"], p["dit_base.final_layer.linear.bias"],
                                  32, 8, 8, 2, cfg.eps)
    torch.testing.assert_close(got.reshape(want.shape).float(), want, rtol=1e-5, atol=1e-5)  # the oracle ran in fp32
