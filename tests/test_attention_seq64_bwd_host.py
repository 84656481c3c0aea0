"""Host checks (no GPU) around the 64-token attention backward: the C symbol dfot_op_attention_seq64_bwd is declared in the header, in
kernels.h (its launcher) and in capi.SIGNATURES with 12 arguments; it refuses null pointers and shapes outside the kernel's rules with the
right error code before any device work (host addresses that are never dereferenced, as in test_attention_frame_causal_bwd_host); the
operator dfot::attention_seq64 exists with a fake implementation of q's shape and dtype; its Python refusals name their rule.

The last two tests are about the GPU test's bar (tests/test_gpu_attention_seq64_bwd_ops.py, rel-L2 < 2e-2 against fp64) on exactly that
test's inputs, through attention_seq64_bwd_common.emulate(), a host restatement of the kernel's roundings:
  * the emulation stays within HALF the bar on every input, so the bar leaves room for the kernel's own summation order.  Measured (seeds
    3 + d, nseq 3, heads 2; worst of dq, dk, dv over d in {32, 64, 72, 96, 128}): gain 1: 3.3e-3, gain 2: 5.3e-3 (6.8e-3 if delta were
    taken from a bf16 o).  Scores reach |S'| = 7.0 at gain 1 and 28.0 at gain 2 (exp2 domain); the mean row maximum of P is 0.10 and 0.6.
  * what broken kernels would measure, each many times the bar:
      delta omitted:                                   dq / dk 0.21 - 0.29 at gain 1, 1.5 - 2.1 at gain 2
      delta of row i ^ 32 (the two halves swapped):    dq / dk 0.29 - 0.39 at gain 1, 2.0 - 2.9 at gain 2
      dk without ln 2:                                 dk 0.44 (= 1 / ln 2 - 1) at either gain
Every test fails on the parent commit, where neither the symbol nor the operator exists."""
import ctypes as C
import functools
import os
import re

import pytest
import torch

from attention_seq64_bwd_common import BAR, GAINS, HEAD_DIMS, emulate, make_case, reference, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dfot_op_attention_seq64_bwd"


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    from dfot_amd import capi
    return capi


def test_header_kernels_h_and_capi_declare_the_symbol(capi):
    hdr = open(os.path.join(ROOT, "include", "dfot_hip.h")).read()
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", hdr)
    assert m and len(m.group(1).split(",")) == 12
    kh = open(os.path.join(ROOT, "diffusion-forcing-transformer_amd", "csrc", "kernels.h")).read()
    m = re.search(r"\bint\s+launch_attention_seq64_bwd\s*\(([^)]*)\)", kh)
    assert m and len(m.group(1).split(",")) == 12
    assert NAME in capi.SIGNATURES and hasattr(capi.lib, NAME)
    assert len(capi.SIGNATURES[NAME][1]) == 12


def test_refuses_bad_arguments_before_any_device_work(capi):
    op = getattr(capi.lib, NAME)
    buf = C.create_string_buffer(64)
    p = C.c_void_p(C.addressof(buf))
    assert op(None, None, None, None, 64, None, None, None, 1, 2, 32, None) == capi.ERR_ARG
    for hole in range(7):  # q, k, v, d_o | dq, dk, dv
        ptrs = [p] * 7
        ptrs[hole] = None
        assert op(*ptrs[:4], 64, *ptrs[4:], 1, 2, 32, None) == capi.ERR_ARG, hole
        assert capi.lib.dfot_last_error().startswith(b"attention_seq64_bwd:")
    # (ldo, nseq, heads, d)
    for args in ((72, 1, 2, 36), (64, 1, 2, 0), (272, 1, 2, 136), (64, 0, 2, 32), (64, 1, 0, 32), (64, 65536, 32768, 32), (56, 1, 2, 32),
                 (68, 1, 2, 32)):
        assert op(p, p, p, p, args[0], p, p, p, *args[1:], None) == capi.ERR_SHAPE, args
        assert capi.lib.dfot_last_error().startswith(b"attention_seq64_bwd:"), capi.lib.dfot_last_error()


def test_operator_is_exported_with_a_fake_of_q_shape_and_dtype(capi):
    from torch._subclasses.fake_tensor import FakeTensorMode
    import dfot_amd
    assert hasattr(torch.ops.dfot, "attention_seq64") and hasattr(torch.ops.dfot, "attention_seq64_backward")
    assert dfot_amd.attention_seq64 is dfot_amd.ops.attention_seq64
    with FakeTensorMode():
        for dtype in (torch.bfloat16, torch.float32):
            q = torch.empty(5, 3, 64, 72, dtype=dtype)
            o = torch.ops.dfot.attention_seq64(q, q, q)
            assert o.shape == q.shape and o.dtype == dtype
            assert o.stride() == (64 * 3 * 72, 72, 3 * 72, 1)  # the transposed view of a compact (F, 64, heads, d) buffer
            qp = torch.empty(5, 3, 64, 128, dtype=torch.bfloat16)
            grads = torch.ops.dfot.attention_seq64_backward(o, qp, qp, qp, 72)
            assert [tuple(g.shape) for g in grads] == [(5, 3, 64, 72)] * 3 and all(g.dtype == dtype for g in grads)


def test_python_refusals_name_the_operator_and_their_rule(capi):
    import dfot_amd
    f = dfot_amd.attention_seq64
    q = torch.zeros(2, 2, 64, 32, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="attention_seq64: .*GPU tensors only"):
        f(q, q, q)  # host tensors
    with pytest.raises(ValueError, match="attention_seq64: .*share one .* shape"):
        f(q, q[:, :1], q)
    with pytest.raises(ValueError, match="attention_seq64: .*share one .* shape"):
        f(q[0], q[0], q[0])
    with pytest.raises(ValueError, match="attention_seq64: .*share one floating dtype"):
        f(q, q.float(), q)
    with pytest.raises(ValueError, match="attention_seq64: .*share one floating dtype"):
        f(q.int(), q.int(), q.int())
    n128 = torch.zeros(2, 2, 128, 32, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="attention_seq64: N=128 must be 64"):
        f(n128, n128, n128)
    d12, d136 = q[..., :12], torch.zeros(2, 2, 64, 136, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="attention_seq64: head dim 12 must be a multiple of 8, <= 128"):
        f(d12, d12, d12)
    with pytest.raises(ValueError, match="attention_seq64: head dim 136 must be a multiple of 8, <= 128"):
        f(d136, d136, d136)


@functools.lru_cache(maxsize=None)
def measured(d, gain, fault=None):
    c = make_case(d, gain)
    return [rel(a, b) for a, b in zip(emulate(c, fault), reference(c))]


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_emulation_stays_within_half_the_gpu_bar(d, gain):
    e = measured(d, gain)
    print(f"attention_seq64_bwd emulation d={d} gain={gain}: dq {e[0]:.2e} dk {e[1]:.2e} dv {e[2]:.2e}")
    assert max(e) < BAR / 2


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_the_gpu_bar_separates_broken_kernels(d, gain):
    """each fault moves the tensors it touches far past the bar and leaves the others where the sound emulation has them"""
    sound = measured(d, gain)
    for fault, hit in (("no_delta", (0, 1)), ("delta_halves_swapped", (0, 1)), ("dk_without_ln2", (1,))):
        e = measured(d, gain, fault)
        print(f"attention_seq64_bwd {fault} d={d} gain={gain}: dq {e[0]:.2e} dk {e[1]:.2e} dv {e[2]:.2e}")
        for i in range(3):
            if i in hit:
                assert e[i] > 10 * BAR, (fault, i)
            else:
                assert e[i] == sound[i], (fault, i)
