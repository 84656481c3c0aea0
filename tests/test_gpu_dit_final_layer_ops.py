"""The DiT final layer (AdaLN -> Linear -> unpatchify) at op level: dfot_op_dit_final_layer in its LDS-resident form (1), its chunked form
(2: the weight streams through LDS, for weights past 160 KiB) and the engine's own choice (0).

Where both forms run they must give the same bits (same summation order per output); where only the chunked form runs it is held against a
float64 restatement (tests/dit_mcraft_common.final_layer_fp64)."""
import functools

import pytest
import torch

from dit_mcraft_common import final_layer_fp64

pytestmark = pytest.mark.gpu

LEVELS, OFF = 5, 64  # rows of the modulation table; column of (shift | scale) inside a row
ROWS = [(40, 8), (256, 16)]  # (rows, rows per frame): 40 is no multiple of the 16-row workgroup and leaves a ragged last one

# Error of the LDS-resident kernel on the commit before the chunked form existed, through the model path (one forward of a depth-1
# continuous DiT3D, taps "stream" and "cond_emb", the final layer restated in float64 from them):
#   4 channels, patch 2, hidden 256 (B 2, T 4):          max-abs 1.996e-03, rel-L2 5.479e-04 (max |ref| 3.37, rms 0.97)
#   K600 geometry, 16 channels, patch 1, hidden 1152:    max-abs 1.837e-03, rel-L2 5.443e-04 (max |ref| 3.74, rms 1.01)
# (that path's modulation comes from the engine's bf16 GEMM, which is most of these figures; the kernel's own fp32 error is what the tests
# below print for the resident form, ~1e-6).  The chunked form gets twice the smaller pair as its bar: the same arithmetic in the same order,
# the factor for the longer output loop.  The cases below draw outputs of the same scale (rms ~1.2).
PARENT_MAXABS, PARENT_REL = 1.837e-03, 5.443e-04
BAR_MAXABS, BAR_REL = 2 * PARENT_MAXABS, 2 * PARENT_REL


def geometry(oc, per_frame):
    """(channels, patch, height, width) with patch^2 * channels = oc and (height / patch) * (width / patch) = per_frame"""
    patch = 1 if oc < 64 else 2
    gh, gw = (2, 4) if per_frame == 8 else (4, 4)
    assert gh * gw == per_frame
    return oc // (patch * patch), patch, gh * patch, gw * patch


@functools.lru_cache(maxsize=None)
def case(hidden, oc, rows, per_frame):
    g = torch.Generator().manual_seed(hidden * 7 + oc + rows)
    frames = rows // per_frame
    x = 1.5 * torch.randn(rows, hidden, generator=g) + 0.3
    table = 0.5 * torch.randn(LEVELS, OFF + 2 * hidden + 32, generator=g)
    levels = torch.randint(-1, LEVELS + 1, (frames,), generator=g, dtype=torch.int32)  # -1 and LEVELS are clamped
    w = torch.randn(oc, hidden, generator=g) / hidden ** 0.5
    b = 0.1 * torch.randn(oc, generator=g)
    dev = tuple(t.cuda() for t in (x, table, levels, w, b))
    return dev, (x, table, levels, w, b)


@functools.lru_cache(maxsize=None)
def reference(hidden, oc, rows, per_frame):
    _, (x, table, levels, w, b) = case(hidden, oc, rows, per_frame)
    c, patch, hh, ww = geometry(oc, per_frame)
    mod = table[levels.long().clamp(0, LEVELS - 1), OFF:OFF + 2 * hidden]
    return final_layer_fp64(x, mod, w, b, c, hh, ww, patch)


def run(hidden, oc, rows, per_frame, form, chunk=None):
    from dfot_amd import capi
    (x, table, levels, w, b), _ = case(hidden, oc, rows, per_frame)
    c, patch, hh, ww = geometry(oc, per_frame)
    out = torch.full((rows // per_frame, c, hh, ww), float("nan"), device="cuda")
    head = (capi.ptr(x), capi.ptr(table), capi.ptr(levels), table.shape[1], OFF, capi.ptr(w), capi.ptr(b), capi.ptr(out), hidden, per_frame, rows,
            1e-6, LEVELS - 1, c, hh, ww, patch)
    if chunk is None:
        rc = capi.lib.dfot_op_dit_final_layer(*head, form, capi.stream_ptr())
    else:
        rc = capi.lib.dfot_op_dit_final_layer_chunked(*head, chunk, capi.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("rows,per_frame", ROWS)
@pytest.mark.parametrize("hidden,oc,chunk", [(128, 128, 53), (320, 128, None), (1152, 16, None)])
def test_chunked_form_equals_resident_form_bit_for_bit(hidden, oc, chunk, rows, per_frame):
    """hidden 128 with a test-only chunk of 53 output rows (128 = 53 + 53 + 22, the split of the recipe's 768-wide weight); hidden 320: the
    largest weight the resident form takes (exactly 160 KiB), VEC 1; hidden 1152 / 16 outputs: the K600 shape"""
    from dfot_amd import capi
    rc1, resident = run(hidden, oc, rows, per_frame, 1)
    rc2, chunked = run(hidden, oc, rows, per_frame, 2, chunk)
    rc0, auto = run(hidden, oc, rows, per_frame, 0)
    assert (rc0, rc1, rc2) == (capi.OK,) * 3, capi.lib.dfot_last_error()
    assert not bool(torch.isnan(resident).any()) and not bool(torch.isnan(chunked).any())  # every element written
    assert torch.equal(resident, chunked)
    assert torch.equal(auto, resident)  # the engine's own choice: what every model that ran before still launches
    ref = reference(hidden, oc, rows, per_frame)
    d = resident.cpu().double() - ref
    print(f"hidden {hidden} oc {oc} rows {rows}: resident form max-abs {float(d.abs().max()):.3e} rel-L2 {float(d.norm() / ref.norm()):.3e}")


# every width the LayerNorm dispatch instantiates (hidden = 128 k for k = 1..10, 12, 16 and 64 k for k = 1, 3, 5, 7, 9)
WIDTHS = [128 * k for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16)] + [64 * k for k in (1, 3, 5, 7, 9)]


@pytest.mark.parametrize("hidden", WIDTHS)
def test_every_kernel_width_gives_the_same_bits_in_both_forms(hidden):
    """16 outputs fit in LDS at every width (128 KB at 2048), so each instantiation of the chunked kernel meets its resident twin: chunks of
    7, 7 and 2 output rows, 40 rows (a ragged last workgroup)"""
    from dfot_amd import capi
    rc1, resident = run(hidden, 16, 40, 8, 1)
    rc2, chunked = run(hidden, 16, 40, 8, 2, 7)
    assert (rc1, rc2) == (capi.OK, capi.OK), capi.lib.dfot_last_error()
    assert not bool(torch.isnan(chunked).any()) and torch.equal(resident, chunked)


@pytest.mark.parametrize("rows,per_frame", ROWS)
@pytest.mark.parametrize("hidden,oc", [(384, 128), (448, 128), (768, 128), (1152, 256)])
def test_chunked_form_vs_float64(hidden, oc, rows, per_frame):
    """only the chunked form runs: 384 = the smallest width past the resident form, 448 = VEC 1 / CNT 7, 768 = the recipe's own (chunks of
    53, 53, 22 output rows), 1152 x 256 = the largest patch vector.

    Bar: twice the resident kernel's error on the parent commit through the model path (PARENT_* above): measured max-abs 1.996e-03 /
    rel-L2 5.479e-04 (4 channels, patch 2, hidden 256) and 1.837e-03 / 5.443e-04 (K600 geometry), the smaller pair doubled = 3.674e-03 /
    1.089e-03.  The chunked form measures max-abs 6.1e-07 .. 1.1e-06 and rel-L2 1.0e-07 .. 1.2e-07 on these cases."""
    from dfot_amd import capi
    rc, out = run(hidden, oc, rows, per_frame, 2)
    assert rc == capi.OK, capi.lib.dfot_last_error()
    assert not bool(torch.isnan(out).any())  # every element written
    rc0, auto = run(hidden, oc, rows, per_frame, 0)
    assert rc0 == capi.OK and torch.equal(auto, out)
    ref = reference(hidden, oc, rows, per_frame)
    d = out.cpu().double() - ref
    maxabs, rel = float(d.abs().max()), float(d.norm() / ref.norm())
    print(f"hidden {hidden} oc {oc} rows {rows}: chunked form max-abs {maxabs:.3e} rel-L2 {rel:.3e} (max |ref| {float(ref.abs().max()):.2f})")
    assert maxabs <= BAR_MAXABS and rel <= BAR_REL


def test_resident_form_refuses_a_weight_that_does_not_fit_and_bad_chunks():
    from dfot_amd import capi
    rc, _ = run(384, 128, 40, 8, 1)
    assert rc == capi.ERR_SHAPE and b"final layer: weight (196608 B) does not fit in LDS" in capi.lib.dfot_last_error()
    rc, _ = run(384, 128, 40, 8, 3)
    assert rc == capi.ERR_ARG and b"form 3" in capi.lib.dfot_last_error()
    rc, _ = run(384, 128, 40, 8, 2, 0)
    assert rc == capi.ERR_ARG
    rc, _ = run(384, 128, 40, 8, 2, 107)  # 107 rows of 384 floats are past 160 KiB
    assert rc == capi.ERR_ARG and b"at most 106 fit" in capi.lib.dfot_last_error()


def test_torch_operator():
    import dfot_amd  # noqa: F401  (registers the operators)
    (x, table, levels, w, b), _ = case(768, 128, 256, 16)
    out = torch.ops.dfot.dit_final_layer(x, table, levels, OFF, w, b, 1e-6, 32, 8, 8, 2, 0)
    _, direct = run(768, 128, 256, 16, 2)
    assert torch.equal(out, direct)
