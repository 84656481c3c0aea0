"""GPU: dfot_op_ivae_attention beyond 256 positions per frame (the streaming kernel of csrc/image_vae.hip: N a multiple of 256 in
[512, 4096], e.g. the 32 x 32 = 1024 positions of a 256 x 256 frame), against an fp64 softmax of the same bf16-rounded operands, as
run_attention of tests/test_gpu_image_vae_ops.py does.

Bar: rel-L2 < 1.5e-2, that file's bar for the fused attention (from tests/test_gpu_dit.py:88: bf16 rounding of P and O).  The output
buffer is NaN before the call and must be finite after it; the GUARD rows behind the last frame must keep their sentinel."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BAR = 1.5e-2
GUARD = 64          # rows behind the output that the op must not touch
SENTINEL = -7.0


@pytest.fixture(scope="module")
def capi():
    import dfot_amd  # noqa: F401
    from dfot_amd import capi as c
    assert torch.cuda.is_available()
    return c


def bf(t):
    return t.to(torch.bfloat16).float()


def report(name, got, ref):
    rel = ((got.double() - ref).norm() / ref.norm().clamp_min(1e-12)).item()
    print(f"{name}: max_abs={(got.double() - ref).abs().max().item():.3e} rel_l2={rel:.3e}")
    return rel


def launch(capi, q, k, v):
    """q, k, v fp32 [frames][n][c] (bf16-representable) -> the op's output, bf16 [frames][n][c] on the GPU (guard checked)"""
    frames, n, c = q.shape
    qd, kd, vd = (t.to(torch.bfloat16).reshape(frames * n, c).contiguous().cuda() for t in (q, k, v))
    buf = torch.full((frames * n + GUARD, c), float("nan"), dtype=torch.bfloat16, device="cuda")
    buf[frames * n:] = SENTINEL
    capi.check(capi.lib.dfot_op_ivae_attention(capi.ptr(qd), capi.ptr(kd), capi.ptr(vd), capi.ptr(buf), frames, n, c, capi.stream_ptr()))
    torch.cuda.synchronize()
    assert (buf[frames * n:] == SENTINEL).all(), "the op wrote behind its last row"
    return buf[: frames * n].reshape(frames, n, c)


def reference(q, k, v):
    q64, k64, v64 = (t.double() for t in (q, k, v))
    return torch.softmax(q64 @ k64.transpose(1, 2) / math.sqrt(q.shape[-1]), -1) @ v64


def run_attention(capi, q, k, v):
    return launch(capi, q, k, v).float().cpu(), reference(q, k, v)


@pytest.mark.parametrize("frames,n,c", [(3, 512, 128), (2, 1024, 512), (1, 1024, 1024), (1, 4096, 128), (2, 768, 256), (1, 1280, 384)])
def test_streaming_attention(capi, frames, n, c):
    """the smallest and largest N and C, an odd count of 256-row steps (768, 1280 = 5 x 256), an odd C / 128, more than one frame"""
    g = torch.Generator().manual_seed(n + c)
    q, k, v = (bf(torch.randn(frames, n, c, generator=g)) for _ in range(3))
    got, ref = run_attention(capi, q, k, v)
    rel = report(f"ivae attention frames {frames} N {n} C {c}", got, ref)
    assert torch.isfinite(got).all() and rel < BAR


def test_key_order_one_hot_on_a_key_of_another_block(capi):
    """q_i = 4 k_pi(i), pi(i) = (389 i + 77) mod N: row i's score with key pi(i) is 4 |k|^2 / sqrt(C) ~ 45, every other one ~ N(0, 16),
    so the softmax is one-hot on key pi(i), which lies in another 128-key block than i for almost every row, and the output is v[pi(i)].
    A key block or a P slice taken in the wrong order returns another row of v: far outside any tolerance."""
    n, c = 1024, 128
    g = torch.Generator().manual_seed(21)
    k, v = (bf(torch.randn(1, n, c, generator=g)) for _ in range(2))
    pi = (389 * torch.arange(n) + 77) % n
    assert len(set(pi.tolist())) == n and ((pi // 128) != (torch.arange(n) // 128)).float().mean() > 0.8
    q = 4.0 * k[:, pi]
    got, ref = run_attention(capi, q, k, v)
    rel, rel_v = report("key order vs fp64", got, ref), report("key order vs v[pi]", got, v[:, pi].double())
    assert torch.isfinite(got).all() and rel < BAR and rel_v < BAR


@pytest.mark.parametrize("rising", [True, False])
def test_running_max_moves_in_every_block(capi, rising):
    """k_j = noise + t_j with t rising (or falling) along the keys and q = noise + 1: score / sqrt(C) = noise of std ~ 1.4 + 11.3 t_j,
    t over [0, 3], so a row's block maximum climbs by about 4 per 128-key block (every block rescales the accumulator), or falls by
    as much (the first block's maximum stays and later blocks add small terms)."""
    n, c = 1024, 128
    g = torch.Generator().manual_seed(31 + rising)
    ramp = 3.0 * torch.arange(n) / n
    t = ramp if rising else 3.0 - ramp
    q = bf(torch.randn(2, n, c, generator=g) + 1.0)
    k = bf(torch.randn(2, n, c, generator=g) + t[None, :, None])
    v = bf(torch.randn(2, n, c, generator=g))
    bmax = (q.double() @ k.double().transpose(1, 2)).reshape(2, n, n // 128, 128).amax(-1)
    step = bmax[..., 1:] - bmax[..., :-1]
    moved = ((step > 0) if rising else (step < 0)).float().mean().item()
    print(f"block maximum {'rises' if rising else 'falls'} in {moved:.3f} of the (row, block) steps")
    assert moved > 0.95
    got, ref = run_attention(capi, q, k, v)
    rel = report(f"running max, scores {'rising' if rising else 'falling'}", got, ref)
    assert torch.isfinite(got).all() and rel < BAR


@pytest.mark.parametrize("mult,floor", [(8.0, 30.0), (32.0, 89.0)])
def test_large_scores_need_the_max_subtraction(capi, mult, floor):
    """the operands of test_fused_attention_large_scores_need_the_max_subtraction (tests/test_gpu_image_vae_ops.py) at N = 1024, C = 512"""
    g = torch.Generator().manual_seed(5)
    n, c = 1024, 512
    q, k, v = (bf(torch.randn(2, n, c, generator=g)) for _ in range(3))
    q = bf(q * mult)
    top = ((q @ k.transpose(1, 2)) / math.sqrt(c)).max().item()
    print(f"largest score / sqrt(C) at q x {mult:g}: {top:.1f}")
    assert top > floor
    got, ref = run_attention(capi, q, k, v)
    rel = report(f"ivae attention N 1024, q x {mult:g}", got, ref)
    assert torch.isfinite(got).all() and rel < BAR


@pytest.mark.parametrize("n", [512, 1024])
def test_frames_do_not_mix(capi, n):
    """frame 1's k / v are far from its neighbours' (another scale and offset): a read across a frame boundary shows at once"""
    g = torch.Generator().manual_seed(9 + n)
    c = 128
    q, k, v = (bf(torch.randn(3, n, c, generator=g)) for _ in range(3))
    k[1] = bf(3.0 * k[1] + 2.0)
    v[1] = bf(50.0 * v[1] - 100.0)
    got, ref = run_attention(capi, q, k, v)
    for f in range(3):
        assert report(f"ivae attention N {n}, frame {f}", got[f], ref[f]) < BAR


@pytest.mark.parametrize("n,c", [(1024, 512), (512, 384)])
def test_same_bits_on_every_call_and_in_every_launch(capi, n, c):
    g = torch.Generator().manual_seed(n)
    q, k, v = (bf(torch.randn(3, n, c, generator=g)) for _ in range(3))
    whole = launch(capi, q, k, v)
    assert torch.isfinite(whole.float()).all()
    assert torch.equal(whole, launch(capi, q, k, v))
    for f in (1, 2):
        assert torch.equal(whole[f:f + 1], launch(capi, q[f:f + 1], k[f:f + 1], v[f:f + 1])), f"frame {f} alone differs"


def test_refuses_other_shapes(capi):
    """below the range, inside it but no multiple of 256 (640 and 1152 are multiples of the kernel's 128-key block, so only the
    entry point's rule stops them), above it; and the rule on C at a streaming N.  (1280 = 5 x 256 is inside the rule and runs.)"""
    t = torch.zeros(128 * 128, dtype=torch.bfloat16, device="cuda")
    for n, c in ((384, 128), (640, 128), (1152, 128), (8192, 128), (1024, 192)):
        rc = capi.lib.dfot_op_ivae_attention(capi.ptr(t), capi.ptr(t), capi.ptr(t), capi.ptr(torch.empty_like(t)), 1, n, c, capi.stream_ptr())
        assert rc == capi.ERR_SHAPE
        msg = capi.lib.dfot_last_error().decode()
        assert f"N={n}" in msg and f"C={c}" in msg
