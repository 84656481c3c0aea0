"""Op-level GPU tests of dfot_op_facmat_contract / dfot_op_facmat_expand (csrc/facmat_narrow.hip), the left factors of the MatrixDiTBlock at
1 <= embed_col_dim <= 32, against fp64 on the same bf16-rounded operands.

Grid: frames in {1, 3, 10} x P in {64, 128, 384} x h in {128, 384, 1152} x E in {1, 3, 8, 16, 32}.
Bar: the bf16-output bar of tests/test_gpu_gemm_epilogue.py (lines 5-8, applied by its check(), lines 94-110, with nulp = 1 as its plain
bf16 case does at line 192): |got - bf16(ref)| <= 1 ulp(bf16(ref)) + 1e-6 * mag + 1e-6 * |ref|, mag = the product on absolute values.
Every output lies between two guard blocks that must stay untouched, and a frame gives the same bits alone and as frame 7 of 10.
The ops do not exist on the parent commit: every test here fails there."""
import pytest
import torch

import dit_facmat_narrow_common as nc

pytestmark = pytest.mark.gpu
GUARD = 1024  # bf16 elements before and after every output


def ulp_bf16(x):
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)  # tests/test_gpu_gemm_epilogue.py:90


def within_bar(got, ref, mag):
    """worst |got - bf16(ref)| / (1 ulp + 1e-6 mag + 1e-6 |ref|)"""
    ref16 = ref.float().bfloat16().double()
    tol = 1e-6 * mag + 1e-6 * ref.abs() + ulp_bf16(ref16)
    return ((got.double() - ref16).abs() / tol).max().item()


def run(op, a, u, out_shape, frames, p, h, e):
    """the op on device copies; the output sits between two guards of 7.0; returns (output, guards intact)"""
    from dfot_amd import capi
    n = 1
    for s in out_shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), 7.0, dtype=torch.bfloat16, device="cuda")
    out = buf[GUARD: GUARD + n]
    ad, ud = a.cuda().contiguous(), u.cuda().contiguous()
    capi.check(getattr(capi.lib, op)(capi.ptr(ad), capi.ptr(ud), capi.ptr(out), frames, p, h, e, capi.stream_ptr()))
    torch.cuda.synchronize()
    intact = bool((buf[:GUARD] == 7.0).all()) and bool((buf[GUARD + n:] == 7.0).all())
    return out.reshape(out_shape).cpu(), intact


@pytest.mark.parametrize("h", nc.OP_H)
@pytest.mark.parametrize("p", nc.OP_P)
def test_contract_and_expand_vs_fp64(p, h):
    worst = {"contract": 0.0, "expand": 0.0}
    for frames in nc.OP_FRAMES:
        for e in nc.OP_E:
            m, uc, o, ue = nc.op_operands(frames, p, h, e)
            w, ok = run("dfot_op_facmat_contract", m, uc, (frames, e, h), frames, p, h, e)
            assert ok, f"contract frames={frames} P={p} h={h} E={e}: a guard element was written"
            assert torch.isfinite(w.float()).all()
            rc = within_bar(w, nc.contract_ref(m, uc), nc.contract_ref(m.abs(), uc.abs()))
            s, ok = run("dfot_op_facmat_expand", o, ue, (frames, p, h), frames, p, h, e)
            assert ok, f"expand frames={frames} P={p} h={h} E={e}: a guard element was written"
            assert torch.isfinite(s.float()).all()
            rx = within_bar(s, nc.expand_ref(o, ue), nc.expand_ref(o.abs(), ue.abs()))
            print(f"frames={frames} P={p} h={h} E={e}: worst error / bar contract {rc:.3f}, expand {rx:.3f}")
            assert rc <= 1.0 and rx <= 1.0, (frames, p, h, e, rc, rx)
            worst["contract"], worst["expand"] = max(worst["contract"], rc), max(worst["expand"], rx)
    print(f"P={p} h={h}: worst error / bar {worst}")


@pytest.mark.parametrize("e", nc.OP_E)
def test_a_frame_gives_the_same_bits_alone_and_as_frame_7_of_10(e):
    p, h = 128, 384
    m, uc, o, ue = nc.op_operands(10, p, h, e, seed=5)
    w10, _ = run("dfot_op_facmat_contract", m, uc, (10, e, h), 10, p, h, e)
    w1, _ = run("dfot_op_facmat_contract", m[7:8], uc, (1, e, h), 1, p, h, e)
    assert torch.equal(w10[7:8], w1)
    s10, _ = run("dfot_op_facmat_expand", o, ue, (10, p, h), 10, p, h, e)
    s1, _ = run("dfot_op_facmat_expand", o[7:8], ue, (1, p, h), 1, p, h, e)
    assert torch.equal(s10[7:8], s1)


def test_refused_calls_launch_nothing():
    from dfot_amd import capi
    m, uc, o, ue = nc.op_operands(2, 64, 128, 8)
    md, ud = m.cuda(), uc.cuda()
    out = torch.full((2 * 64 * 128,), 7.0, dtype=torch.bfloat16, device="cuda")
    for name in ("dfot_op_facmat_contract", "dfot_op_facmat_expand"):
        fn = getattr(capi.lib, name)
        for e in (0, 33, 48):
            assert fn(capi.ptr(md), capi.ptr(ud), capi.ptr(out), 2, 64, 128, e, capi.stream_ptr()) == capi.ERR_SHAPE
        assert fn(capi.ptr(md), capi.ptr(ud), capi.ptr(out), 2, 96, 128, 8, capi.stream_ptr()) == capi.ERR_SHAPE
        assert fn(capi.ptr(md), None, capi.ptr(out), 2, 64, 128, 8, capi.stream_ptr()) == capi.ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
