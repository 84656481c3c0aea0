"""dfot_op_equal_bits: the device-side exact comparison behind the content key of the UViT3DPose pose / FiLM cache.

Every bar is exact: the flag is 0 for buffers with equal bits and 1 as soon as one bit differs, wherever it sits -- first byte, last byte,
either side of the seam between the 16-byte body and the tail -- on the 16-byte path and on the scalar paths a misaligned base takes.
Sizes: the small ones sit around one 16-byte load, 4092 / 4100 around one workgroup of them, (1 << 22) + 20 spans many workgroups, and
40 MiB + 36 is the smallest size class at which a thread of the capped grid (2048 x 256) runs the four-loads-in-flight loop AND the
remainder loop on 16-byte elements."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [0, 4, 12, 16, 4092, 4096 + 4, (1 << 22) + 20]
BIG = 40 * (1 << 20) + 36
SENTINEL = 0x5A5A5A5A

P = lambda t: C.c_void_p(t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def capi():
    from dfot_amd import capi as c
    return c


def pair(nbytes, off_a=0, off_b=0, seed=0):
    """two uint8 views of `nbytes` equal random bytes whose bases sit off_a / off_b bytes past a 16-byte boundary"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    src = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g)
    out = []
    for off in (off_a, off_b):
        buf = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        view = buf[off:off + nbytes]
        view.copy_(src)
        out.append(view)
    return out


def differs(capi, a, b, nbytes):
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    capi.check(capi.lib.dfot_op_equal_bits(P(a), P(b), nbytes, P(flag), S()))
    return int(flag.item())


def places(nbytes):
    """byte 0, the last byte, the last byte of the 16-byte-aligned body and the first byte of the tail (those that exist)"""
    body = nbytes // 16 * 16
    pl = {0: "byte 0", nbytes - 1: "last byte"}
    if body:
        pl[body - 1] = "last byte of the body"
    if body < nbytes:
        pl[body] = "first byte of the tail"
    return pl


def check_size(capi, nbytes, off_a, off_b, extra=()):
    a, b = pair(nbytes, off_a, off_b, seed=nbytes % 1000 + off_a)
    if nbytes:
        assert a.data_ptr() % 16 == off_a and b.data_ptr() % 16 == off_b
    assert differs(capi, a, b, nbytes) == 0
    if nbytes == 0:
        return
    pl = places(nbytes)
    pl.update({int(i): "interior" for i in extra})
    for i, (pos, what) in enumerate(sorted(pl.items())):
        bit = 1 << (i % 8)
        b[pos] ^= bit
        assert differs(capi, a, b, nbytes) == 1, f"{nbytes} bytes: flipped bit {bit:#x} of byte {pos} ({what}) not seen"
        assert differs(capi, b, a, nbytes) == 1
        b[pos] ^= bit
    assert differs(capi, a, b, nbytes) == 0


@pytest.mark.parametrize("nbytes", SIZES)
def test_equal_and_single_flipped_bits_aligned(capi, nbytes):
    check_size(capi, nbytes, 0, 0)


@pytest.mark.parametrize("nbytes", SIZES)
@pytest.mark.parametrize("off_a,off_b", [(4, 4), (4, 0), (1, 0)])
def test_base_off_16_byte_alignment_takes_the_scalar_path(capi, nbytes, off_a, off_b):
    """4 bytes off a 16-byte boundary (both bases, or one of them): 4-byte loads; 1 byte off: byte loads"""
    check_size(capi, nbytes, off_a, off_b)


def test_grid_stride_loop_beyond_the_capped_grid(capi):
    """more 16-byte elements than 4 x (2048 x 256): flips in the unrolled part, in the remainder part and at the seams"""
    per_pass = 2048 * 256 * 16
    check_size(capi, BIG, 0, 0, extra=(per_pass + 5, 3 * per_pass + 17, 4 * per_pass + 33, BIG - 36 - 16 * 7))


def test_bitwise_not_float_compare(capi):
    nan_a = torch.from_numpy(np.array([0x7FC00001, 0xFFC12345, 0x7F800001], dtype=np.uint32).view(np.int32)).cuda()
    nan_b = nan_a.clone()
    assert torch.isnan(nan_a.view(torch.float32)).all()
    assert differs(capi, nan_a, nan_b, 12) == 0                     # equal NaN payloads: equal
    nan_b[1] ^= 1                                                  # another payload of the same NaN class: different bits
    assert differs(capi, nan_a, nan_b, 12) == 1
    pz = torch.zeros(8, device="cuda")
    nz = torch.zeros(8, device="cuda")
    nz[5] = -0.0
    assert torch.equal(pz, nz)                                     # equal as floats ...
    assert differs(capi, pz, nz, 32) == 1                          # ... but the cache is a function of the bits


def test_several_compares_share_one_flag(capi):
    a, b = pair(4096)
    c, d = pair(64, seed=1)
    d[63] ^= 0x80
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    capi.check(capi.lib.dfot_op_equal_bits(P(c), P(d), 64, P(flag), S()))      # differs: sets the flag
    capi.check(capi.lib.dfot_op_equal_bits(P(a), P(b), 4096, P(flag), S()))    # equal: must leave it alone
    assert int(flag.item()) == 1


def test_bad_arguments_are_refused_before_any_launch(capi):
    a, b = pair(4096)
    b[0] ^= 1                                                      # a launch would write 1
    flag = torch.full((2,), SENTINEL, dtype=torch.int32, device="cuda")
    lib = capi.lib
    assert lib.dfot_op_equal_bits(P(a), P(b), 4096, None, S()) == capi.ERR_ARG                                 # null flag
    assert lib.dfot_op_equal_bits(P(a), P(b), 4096, C.c_void_p(flag.data_ptr() + 2), S()) == capi.ERR_ARG      # misaligned flag
    assert lib.dfot_op_equal_bits(None, P(b), 4096, P(flag), S()) == capi.ERR_ARG
    assert lib.dfot_op_equal_bits(P(a), None, 4096, P(flag), S()) == capi.ERR_ARG
    assert lib.dfot_op_equal_bits(P(a), P(b), -16, P(flag), S()) == capi.ERR_ARG
    assert lib.dfot_op_equal_bits(None, None, 0, P(flag), S()) == capi.OK                                      # empty: equal, no launch
    assert lib.dfot_op_equal_bits(None, None, 0, None, S()) == capi.ERR_ARG
    torch.cuda.synchronize()
    assert flag.tolist() == [SENTINEL, SENTINEL]
