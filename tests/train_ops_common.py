"""Helpers shared by the op-level training tests (test_gpu_train_ops.py, test_gpu_train_bwd_ops.py): NaN-prefilled buffers with sentinel
tails, the run-twice harness, the element-wise comparison against a bar and the worst-ratio table.  The method is stated in the header
of test_gpu_train_ops.py."""
import ctypes as C

import pytest
import torch

NAN = float("nan")
U = 2.0 ** -24
WORST = {}


@pytest.fixture(scope="module")
def capi():
    import dfot_amd  # noqa: F401
    from dfot_amd import capi as c
    assert torch.cuda.is_available()
    return c


@pytest.fixture(scope="module", autouse=True)
def worst_ratio_table():
    WORST.clear()  # one table per module that imports this fixture
    yield
    print("\nworst elementwise error / bar per op family:")
    for fam, (r, name) in sorted(WORST.items()):
        print(f"  {fam:18s} {r:.3f}  ({name})")


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    """device pointer of a tensor or view (offsets included); None -> NULL"""
    return C.c_void_p(0 if t is None else t.data_ptr())


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def nan_buf(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def bf(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).bfloat16()


def run(capi, fn, outs):
    """fn() calls an entry point and returns its status; it runs twice, each time from the initial contents of `outs`, and the two results
    must agree bit for bit.  Returns host copies of the outputs."""
    init = [o.clone() for o in outs]
    res = []
    for _ in range(2):
        for o, i in zip(outs, init):
            o.copy_(i)
        capi.check(fn())
        res.append([o.cpu() for o in outs])
    for x, y in zip(*res):
        assert torch.equal(bits(x), bits(y)), "second run on the same stream differs"
    return res[0]


def record(fam, name, ratio):
    if ratio > WORST.get(fam, (-1.0, ""))[0]:
        WORST[fam] = (ratio, name)


def ulp_bf16(x):
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


def check(fam, name, got, exp, bar, nulp=0):
    """got: host output buffer; exp: fp64 reference of the same shape, NaN where nothing may be written; bar: the fp32 bar (bf16 outputs:
    nulp > 0 and the reference is rounded to bf16 first)"""
    got = got.double()
    w = ~torch.isnan(exp)
    assert torch.isnan(got[~w]).all(), f"{name}: {int((~torch.isnan(got[~w])).sum())} stores outside the output"
    assert torch.isfinite(got[w]).all(), f"{name}: {int((~torch.isfinite(got[w])).sum())} outputs missing or not finite"
    ref = exp[w]
    tol = bar[w].clamp_min(1e-300)
    if nulp:
        ref = ref.float().bfloat16().double()
        tol = tol + nulp * ulp_bf16(ref)
    ratio = ((got[w] - ref).abs() / tol).max().item() if ref.numel() else 0.0
    print(f"{name}: worst error / bar = {ratio:.3f}")
    record(fam, name, ratio)
    assert ratio <= 1.0, name


def exact(fam, name, got, exp):
    """bitwise equality of whole buffers (exp carries the NaN sentinel where nothing may be written)"""
    assert got.dtype == exp.dtype and got.shape == exp.shape
    bad = bits(got) != bits(exp)
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        pytest.fail(f"{name}: {int(bad.sum())} elements differ, first at flat index {i}: got {got.flatten()[i].item()!r} "
                    f"(bits {bits(got).flatten()[i].item():#x}), want {exp.flatten()[i].item()!r} (bits {bits(exp).flatten()[i].item():#x})")
    print(f"{name}: bit-exact")
    record(fam, name, 0.0)


def tail(t, n, fill=NAN):
    """host tensor t flattened, followed by n sentinel elements (what a buffer with n extra elements behind the output must hold)"""
    return torch.cat([t.flatten(), torch.full((n,), fill, dtype=t.dtype)])


def seq_bar(c, mag, ref):
    return c * U * mag + U * ref.abs()
