"""Host checks (no GPU) around the frame-causal attention backward: the two C symbols dfot_op_attention_frame_causal_lse / _bwd are declared
in the header and in capi.SIGNATURES with 12 and 17 arguments, each refuses null pointers and shapes outside the kernel's rules with the
right error code before any device work (host addresses that are never dereferenced, as in test_dit1d_host), the operator
dfot::frame_causal_attention exists with a fake implementation of q's shape and dtype, and its Python refusals name their rule.
Every test fails on the parent commit, where neither the symbols nor the operator exist."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    from dfot_amd import capi
    return capi


def test_header_and_capi_declare_both_symbols(capi):
    hdr = open(os.path.join(ROOT, "include", "dfot_hip.h")).read()
    for name, nargs in (("dfot_op_attention_frame_causal_lse", 12), ("dfot_op_attention_frame_causal_bwd", 17)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert name in capi.SIGNATURES and hasattr(capi.lib, name), name
        assert len(capi.SIGNATURES[name][1]) == nargs, name


# (ldo, n, frame_len, d, word of the message): the cases of the issue
BAD_SHAPES = [(64, 256, 24, 32, b"frame_len"), (64, 192, 32, 32, b"N=192"), (64, 256, 32, 12, b"head dim"), (68, 256, 32, 32, b"row stride")]


def test_lse_forward_refuses_bad_arguments_before_any_device_work(capi):
    op = capi.lib.dfot_op_attention_frame_causal_lse
    buf = C.create_string_buffer(64)
    p = C.c_void_p(C.addressof(buf))
    assert op(None, None, None, None, 64, None, 1, 2, 256, 32, 32, None) == capi.ERR_ARG
    for hole in range(4):  # q, k, v, o
        ptrs = [p] * 4
        ptrs[hole] = None
        assert op(*ptrs, 64, p, 1, 2, 256, 32, 32, None) == capi.ERR_ARG, hole
    assert op(p, p, p, p, 64, None, 1, 2, 256, 32, 32, None) == capi.ERR_ARG  # the lse pointer is what this entry is for
    assert b"attention_frame_causal" in capi.lib.dfot_last_error()
    for ldo, n, frame_len, d, word in BAD_SHAPES:
        assert op(p, p, p, p, ldo, p, 1, 2, n, frame_len, d, None) == capi.ERR_SHAPE, (ldo, n, frame_len, d)
        assert word in capi.lib.dfot_last_error(), capi.lib.dfot_last_error()


def test_backward_refuses_bad_arguments_before_any_device_work(capi):
    op = capi.lib.dfot_op_attention_frame_causal_bwd
    buf = C.create_string_buffer(64)
    p = C.c_void_p(C.addressof(buf))
    assert op(*([None] * 5), 64, *([None] * 5), 1, 2, 256, 32, 32, None) == capi.ERR_ARG
    for hole in range(10):  # q, k, v, o, d_o | lse, delta, dq, dk, dv
        ptrs = [p] * 10
        ptrs[hole] = None
        assert op(*ptrs[:5], 64, *ptrs[5:], 1, 2, 256, 32, 32, None) == capi.ERR_ARG, hole
        assert b"attention_frame_causal_bwd" in capi.lib.dfot_last_error()
    for ldo, n, frame_len, d, word in BAD_SHAPES:
        assert op(*([p] * 5), ldo, *([p] * 5), 1, 2, n, frame_len, d, None) == capi.ERR_SHAPE, (ldo, n, frame_len, d)
        assert b"attention_frame_causal_bwd" in capi.lib.dfot_last_error() and word in capi.lib.dfot_last_error(), capi.lib.dfot_last_error()


def test_operator_is_registered_with_a_fake_of_q_shape_and_dtype(capi):
    from torch._subclasses.fake_tensor import FakeTensorMode
    import dfot_amd
    assert hasattr(torch.ops.dfot, "frame_causal_attention")
    assert dfot_amd.frame_causal_attention is dfot_amd.ops.frame_causal_attention
    with FakeTensorMode():
        for dtype in (torch.bfloat16, torch.float32):
            q = torch.empty(2, 3, 256, 72, dtype=dtype)
            o = torch.ops.dfot.frame_causal_attention(q, q, q, 32)
            assert o.shape == q.shape and o.dtype == dtype
            assert o.transpose(1, 2).is_contiguous()  # (B, N, heads, d) compact: the reference's transpose + reshape is a view


def test_python_refusals_name_their_rule(capi):
    import dfot_amd
    f = dfot_amd.frame_causal_attention
    q = torch.zeros(1, 2, 256, 32, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="GPU tensors only"):
        f(q, q, q, 32)  # host tensors
    with pytest.raises(ValueError, match="share one .* shape"):
        f(q, q[:, :1], q, 32)
    with pytest.raises(ValueError, match="share one .* shape"):
        f(q[0], q[0], q[0], 32)
    with pytest.raises(ValueError, match="share one floating dtype"):
        f(q, q.float(), q, 32)
    with pytest.raises(ValueError, match="share one floating dtype"):
        f(q.int(), q.int(), q.int(), 32)
    with pytest.raises(ValueError, match=r"frame_len 24 not in \(16, 32, 64, 128\)"):
        f(q, q, q, 24)
    n192 = q[:, :, :192]
    with pytest.raises(ValueError, match="N=192 must be a positive multiple of 128"):
        f(n192, n192, n192, 32)
    d12, d136 = q[..., :12], torch.zeros(1, 2, 256, 136, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="head dim 12 must be a multiple of 8, <= 128"):
        f(d12, d12, d12, 32)
    with pytest.raises(ValueError, match="head dim 136 must be a multiple of 8, <= 128"):
        f(d136, d136, d136, 32)
