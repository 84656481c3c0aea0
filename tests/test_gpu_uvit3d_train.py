"""Training the pose-free UViT3D on the GPU: the per-frame FiLM norm ops (dfot_op_gn_silu_fwd_frame / _bwd_frame, dfot_op_rms_film_fwd_frame /
_bwd_frame) against float64 torch autograd on the same inputs, and dfot_amd.UViT3DTrainer against torch autograd through
tests/uvit3d_common.forward_host, the continuous-diffusion training loss of oracle.sampler, torch.optim.AdamW and the reference fixture
tests/golden/uvit3d_train.npz.

Bars.  Op level: those of test_groupnorm_silu_backward, test_frame_bias_gemm_and_groupnorm_on_a_column_block and test_rms_film_backward
(tests/test_gpu_train.py) for the per-row ops -- bf16 outputs 5e-3, fp32 outputs 1e-4 (1e-5 for the RMS dx); the per-frame FiLM gradient is an
fp32 fixed-order sum like dgamma, so it takes dgamma's 1e-4 and no longer the bf16 tensor's 5e-3.  Whole model: those of
test_uvit3d_pose_backward_matches_autograd / test_uvit3d_pose_training_step / test_uvit_data_parallel_step_equals_single_process_step /
test_training_gradients_vs_reference_fixture, which run the same block code at the same widths.
"""
import numpy as np
import pytest
import torch

import uvit3d_common as uc

pytestmark = pytest.mark.gpu
F = torch.nn.functional
BF = torch.bfloat16


def rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm())


@pytest.fixture(scope="module")
def capi():
    from dfot_amd import capi as c
    return c


def P(t):
    from dfot_amd import capi as c
    return c.ptr(t)


def PV(t):
    from dfot_amd import capi as c
    return c.ptr_rows(t)


def S():
    from dfot_amd import capi as c
    return c.stream_ptr()


# ---------------------------------------------------------------------------------------------------------------- GroupNorm pair
def _gn_case(bt, pix, c, wide, res):
    g = torch.Generator().manual_seed(1000 * bt + pix + c)
    x = torch.randn(bt, pix, c, generator=g) * 1.5 + 0.3
    dy = torch.randn(bt, pix, c, generator=g).to(BF)
    gamma, beta = torch.randn(c, generator=g) * 0.5 + 1, torch.randn(c, generator=g) * 0.2
    ld, c0 = (6 * c, 2 * c) if wide else (2 * c, 0)
    table = torch.randn(bt, ld, generator=g) * 0.5
    dres = torch.randn(bt, pix, c, generator=g) if res else None
    return x, dy, gamma, beta, table, ld, c0, dres


def _gn_run(capi, dev, bt, pix, c, ld, c0, res):
    """one forward + backward on device buffers `dev`; returns fresh outputs"""
    xd, dyd, gd, bd, td, rd = dev
    fview = td[:, c0: c0 + 2 * c]
    out = torch.full((bt * pix, c), float("nan"), dtype=BF, device="cuda")
    stats = torch.empty(bt, 32, 2, device="cuda")
    capi.check(capi.lib.dfot_op_gn_silu_fwd_frame(P(xd), P(gd), P(bd), PV(fview), ld, 1e-6, P(out), P(stats), bt, pix, c, S()))
    dx = torch.full((bt, pix, c), float("nan"), device="cuda")
    dxb = torch.full((bt, pix, c), float("nan"), dtype=BF, device="cuda") if res else None
    dtab = torch.full((bt, ld), 7.0, device="cuda")  # the neighbouring columns must keep this fill
    dga, dbe = torch.full((c,), float("nan"), device="cuda"), torch.full((c,), float("nan"), device="cuda")
    capi.check(capi.lib.dfot_op_gn_silu_bwd_frame(P(xd), P(dyd), P(stats), P(gd), P(bd), PV(fview), ld, P(rd), P(dx), P(dxb), PV(dtab[:, c0: c0 + 2 * c]), ld,
                                                  P(dga), P(dbe), bt, pix, c, S()))
    torch.cuda.synchronize()
    return out, dx, dxb, dtab, dga, dbe


@pytest.mark.parametrize("bt,pix,c,wide,res", [(3, 64, 128, False, False), (2, 1024, 256, True, False), (2, 4096, 128, False, True),
                                               (1, 256, 1024, False, False)])
def test_groupnorm_frame_pair(capi, bt, pix, c, wide, res):
    """SiLU(GN32(x) (1 + scale[f]) + shift[f]) and its backward with the per-frame FiLM gradient summed in the kernel, vs float64 autograd.
    (3, 64, 128): one chunk per frame, odd frame count; (2, 4096, 128): the 512-pixel chunk branch, run with dres and both dx and dx_bf;
    (1, 256, 1024): the widest row; (2, 1024, 256): film_ld = dfilm_ld = 6C at column offset 2C, neighbours checked untouched.
    Two consecutive calls must give byte-identical outputs."""
    x, dy, gamma, beta, table, ld, c0, dres = _gn_case(bt, pix, c, wide, res)
    dev = tuple(None if t is None else t.cuda() for t in (x, dy, gamma, beta, table, dres))
    table0 = dev[4].clone()
    out, dx, dxb, dtab, dga, dbe = _gn_run(capi, dev, bt, pix, c, ld, c0, res)
    again = _gn_run(capi, dev, bt, pix, c, ld, c0, res)
    for a, b in zip((out, dx, dxb, dtab, dga, dbe), again):
        assert a is None or torch.equal(a.view(torch.uint8 if a.dtype != BF else torch.int16), b.view(torch.uint8 if b.dtype != BF else torch.int16))
    assert torch.equal(dev[4], table0)
    xr, gr, br = (t.double().requires_grad_() for t in (x, gamma, beta))
    fr = table[:, c0: c0 + 2 * c].double().requires_grad_()
    h = F.group_norm(xr.permute(0, 2, 1), 32, gr, br, 1e-6).permute(0, 2, 1)
    y = F.silu(h * (1 + fr[:, None, :c]) + fr[:, None, c:])
    y.backward(dy.double())
    want_dx = xr.grad + (dres.double() if res else 0)
    rs = dict(out=rel(out.view(bt, pix, c), y.detach()), dx=rel(dx, want_dx), dgamma=rel(dga, gr.grad), dbeta=rel(dbe, br.grad),
              dfilm=rel(dtab[:, c0: c0 + 2 * c], fr.grad))
    if res:
        rs["dx_bf"] = rel(dxb, want_dx)
    print(f"GroupNorm frame pair {(bt, pix, c)} ld={ld}: " + " ".join(f"{k} {v:.1e}" for k, v in rs.items()))
    assert rs["out"] < 5e-3 and rs.get("dx_bf", 0.0) < 5e-3
    assert max(rs["dx"], rs["dgamma"], rs["dbeta"]) < 1e-4 and rs["dfilm"] < 1e-4
    if wide:  # columns outside the block's 2C keep their fill
        assert bool((dtab[:, :c0] == 7.0).all()) and bool((dtab[:, c0 + 2 * c:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- RMS pair
def _rms_run(capi, dev, frames, rpf, c):
    xd, gd, wd, td, rd = dev
    rows = frames * rpf
    out = torch.full((rows, c), float("nan"), dtype=BF, device="cuda")
    capi.check(capi.lib.dfot_op_rms_film_fwd_frame(P(xd), P(wd), P(td), 2 * c, 1e-6, P(out), rows, rpf, c, S()))
    dx = torch.full((rows, c), float("nan"), device="cuda")
    dxb = torch.full((rows, c), float("nan"), dtype=BF, device="cuda")
    dtab = torch.full((frames, 2 * c), float("nan"), device="cuda")
    dw = torch.full((c,), float("nan"), device="cuda")
    capi.check(capi.lib.dfot_op_rms_film_bwd_frame(P(xd), P(gd), P(wd), P(td), 2 * c, 1e-6, P(rd), P(dx), P(dxb), P(dtab), 2 * c, P(dw), rows, rpf, c, S()))
    torch.cuda.synchronize()
    return out, dx, dxb, dtab, dw


@pytest.mark.parametrize("frames,rpf,c", [(8, 16, 256), (5, 64, 128), (3, 1024, 512), (4, 64, 576)])
def test_rms_frame_pair(capi, frames, rpf, c):
    """RMSNorm(x; w) (1 + scale[f]) + shift[f] and its backward vs float64 autograd.  (8, 16, 256): fewer rows per frame than a workgroup has
    waves per chunk; (5, 64, 128): a frame count that divides nothing; (4, 64, 576): an RE10K width (one float per lane access)."""
    from oracle import uvit as ouvit
    g = torch.Generator().manual_seed(frames * 7 + rpf + c)
    rows = frames * rpf
    x, dxn = torch.randn(rows, c, generator=g) * 2, torch.randn(rows, c, generator=g)
    w = torch.randn(c, generator=g) * 0.3 + 1
    table = torch.randn(frames, 2 * c, generator=g) * 0.5
    dres = torch.randn(rows, c, generator=g)
    dev = tuple(t.cuda() for t in (x, dxn, w, table, dres))
    got = _rms_run(capi, dev, frames, rpf, c)
    again = _rms_run(capi, dev, frames, rpf, c)
    for a, b in zip(got, again):
        assert torch.equal(a.view(torch.int16 if a.dtype == BF else torch.int32), b.view(torch.int16 if b.dtype == BF else torch.int32))
    out, dx, dxb, dtab, dw = got
    xr, wr, fr = x.double().requires_grad_(), w.double().requires_grad_(), table.double().requires_grad_()
    fe = fr.repeat_interleave(rpf, 0)
    y = ouvit.rms_norm(xr, wr, 1e-6) * (1 + fe[:, :c]) + fe[:, c:]
    y.backward(dxn.double())
    want_dx = xr.grad + dres.double()
    rs = dict(out=rel(out, y.detach()), dx=rel(dx, want_dx), dx_bf=rel(dxb, want_dx), dw=rel(dw, wr.grad), dfilm=rel(dtab, fr.grad))
    print(f"RMS frame pair {(frames, rpf, c)}: " + " ".join(f"{k} {v:.1e}" for k, v in rs.items()))
    assert rs["out"] < 5e-3 and rs["dx_bf"] < 5e-3
    assert rs["dx"] < 1e-5 and rs["dw"] < 1e-4 and rs["dfilm"] < 1e-4


# ---------------------------------------------------------------------------------------------------------------- misuse
def _misuse_cases(capi):
    L, A, SH, N = capi.lib, capi.ERR_ARG, capi.ERR_SHAPE, None
    return {
        "gn_fwd C=192": (SH, lambda b: L.dfot_op_gn_silu_fwd_frame(P(b["f"]), P(b["f"]), P(b["f"]), P(b["f"]), 384, 1e-6, P(b["h"]), P(b["f2"]), 2, 64, 192, S())),
        "gn_bwd C=192": (SH, lambda b: L.dfot_op_gn_silu_bwd_frame(P(b["f"]), P(b["h"]), P(b["f"]), P(b["f"]), P(b["f"]), P(b["f"]), 384, N, P(b["f2"]), N,
                                                                   P(b["f3"]), 384, P(b["f3"]), P(b["f3"]), 2, 64, 192, S())),
        "gn_fwd film_ld < 2C": (A, lambda b: L.dfot_op_gn_silu_fwd_frame(P(b["f"]), P(b["f"]), P(b["f"]), P(b["f"]), 128, 1e-6, P(b["h"]), P(b["f2"]), 2, 64, 128, S())),
        "gn_bwd film_ld < 2C": (A, lambda b: L.dfot_op_gn_silu_bwd_frame(P(b["f"]), P(b["h"]), P(b["f"]), P(b["f"]), P(b["f"]), P(b["f"]), 128, N, P(b["f2"]), N,
                                                                          P(b["f3"]), 256, P(b["f3"]), P(b["f3"]), 2, 64, 128, S())),
        "gn_bwd dfilm_ld < 2C": (A, lambda b: L.dfot_op_gn_silu_bwd_frame(P(b["f"]), P(b["h"]), P(b["f"]), P(b["f"]), P(b["f"]), P(b["f"]), 256, N, P(b["f2"]), N,
                                                                           P(b["f3"]), 128, P(b["f3"]), P(b["f3"]), 2, 64, 128, S())),
        "gn_fwd null out": (A, lambda b: L.dfot_op_gn_silu_fwd_frame(P(b["f"]), P(b["f"]), P(b["f"]), P(b["f"]), 256, 1e-6, N, P(b["f2"]), 2, 64, 128, S())),
        "gn_bwd null dx and dx_bf": (A, lambda b: L.dfot_op_gn_silu_bwd_frame(P(b["f"]), P(b["h"]), P(b["f"]), P(b["f"]), P(b["f"]), P(b["f"]), 256, N, N, N,
                                                                               P(b["f3"]), 256, P(b["f3"]), P(b["f3"]), 2, 64, 128, S())),
        "gn_bwd null dfilm_vec": (A, lambda b: L.dfot_op_gn_silu_bwd_frame(P(b["f"]), P(b["h"]), P(b["f"]), P(b["f"]), P(b["f"]), P(b["f"]), 256, N, P(b["f2"]), N,
                                                                            N, 256, P(b["f3"]), P(b["f3"]), 2, 64, 128, S())),
        "rms_fwd width 100": (SH, lambda b: L.dfot_op_rms_film_fwd_frame(P(b["f"]), P(b["f"]), P(b["f"]), 200, 1e-6, P(b["h"]), 8, 4, 100, S())),
        "rms_fwd film_ld < 2C": (A, lambda b: L.dfot_op_rms_film_fwd_frame(P(b["f"]), P(b["f"]), P(b["f"]), 128, 1e-6, P(b["h"]), 8, 4, 128, S())),
        "rms_fwd rows % rows_per_frame": (A, lambda b: L.dfot_op_rms_film_fwd_frame(P(b["f"]), P(b["f"]), P(b["f"]), 256, 1e-6, P(b["h"]), 10, 4, 128, S())),
        "rms_fwd null out": (A, lambda b: L.dfot_op_rms_film_fwd_frame(P(b["f"]), P(b["f"]), P(b["f"]), 256, 1e-6, N, 8, 4, 128, S())),
        "rms_bwd rows % rows_per_frame": (A, lambda b: L.dfot_op_rms_film_bwd_frame(P(b["f"]), P(b["f"]), P(b["f"]), P(b["f"]), 256, 1e-6, P(b["f"]), P(b["f2"]),
                                                                                    N, P(b["f3"]), 256, P(b["f3"]), 10, 4, 128, S())),
        "rms_bwd film_ld < 2C": (A, lambda b: L.dfot_op_rms_film_bwd_frame(P(b["f"]), P(b["f"]), P(b["f"]), P(b["f"]), 128, 1e-6, P(b["f"]), P(b["f2"]),
                                                                           N, P(b["f3"]), 256, P(b["f3"]), 8, 4, 128, S())),
        "rms_bwd width 100": (SH, lambda b: L.dfot_op_rms_film_bwd_frame(P(b["f"]), P(b["f"]), P(b["f"]), P(b["f"]), 200, 1e-6, P(b["f"]), P(b["f2"]),
                                                                         N, P(b["f3"]), 200, P(b["f3"]), 8, 4, 100, S())),
        "rms_bwd null dw": (A, lambda b: L.dfot_op_rms_film_bwd_frame(P(b["f"]), P(b["f"]), P(b["f"]), P(b["f"]), 256, 1e-6, P(b["f"]), P(b["f2"]),
                                                                      N, P(b["f3"]), 256, N, 8, 4, 128, S())),
    }


MISUSE = ["gn_fwd C=192", "gn_bwd C=192", "gn_fwd film_ld < 2C", "gn_bwd film_ld < 2C", "gn_bwd dfilm_ld < 2C", "gn_fwd null out",
          "gn_bwd null dx and dx_bf", "gn_bwd null dfilm_vec", "rms_fwd width 100", "rms_fwd film_ld < 2C", "rms_fwd rows % rows_per_frame",
          "rms_fwd null out", "rms_bwd rows % rows_per_frame", "rms_bwd film_ld < 2C", "rms_bwd width 100", "rms_bwd null dw"]


def test_frame_ops_refuse_misuse(capi):
    """the documented status comes back and nothing is launched: every buffer keeps its NaN fill"""
    cases = _misuse_cases(capi)
    assert set(cases) == set(MISUSE)
    bufs = {k: torch.full((1 << 16,), float("nan"), device="cuda") for k in ("f", "f2", "f3")}
    bufs["h"] = torch.full((1 << 16,), float("nan"), dtype=BF, device="cuda")
    for name in MISUSE:
        code, call = cases[name]
        got = call(bufs)
        torch.cuda.synchronize()
        assert got == code, f"{name}: status {got}, expected {code} ({capi.lib.dfot_last_error().decode()})"
        for k, t in bufs.items():
            assert torch.isnan(t.float()).all(), f"{name}: buffer {k} was written"


# ---------------------------------------------------------------------------------------------------------------- whole model
# uvit3d_common.TINY: channels 128/128/128/256, 2 heads (d = 64 and 128), 64 x 64 frames, T 8, B 2 -- the smallest model the engine accepts;
# its levels give 1024, 256, 64 and 16 rows per frame
import functools  # noqa: E402

DROP = torch.tensor([True, False])


def tcfg(tag, **over):
    dim, drop = uc.CASES[tag]
    return dict(uc.TINY, resolution=uc.X_SHAPE[-1], max_tokens=uc.MAX_TOKENS, in_channels=uc.X_SHAPE[0], cond_dim=dim, external_cond_dropout=drop, **over)


def trainer(tag, **kw):
    import dfot_amd
    over = kw.pop("cfg", {})
    return dfot_amd.UViT3DTrainer(uc.case_params(tag), tcfg(tag, **over), **kw)


def trainable(params):
    return [n for n in params if n not in (uc.FREQS, uc.PHASES)]


def case_inputs(tag):
    x, levels, cond, _ = uc.inputs()
    dim, drop = uc.CASES[tag]
    return x, levels, (cond if dim else None), (DROP if drop > 0 else None)


@functools.lru_cache(maxsize=None)
def autograd_reference(tag):
    """forward and every parameter gradient through uvit3d_common.forward_host (fp32 on the CPU) for a fixed random d_out; computed once per case"""
    x, levels, cond, drop = case_inputs(tag)
    d_out = torch.randn(x.shape, generator=torch.Generator().manual_seed(17))
    ps = {n: t.clone().requires_grad_(n not in (uc.FREQS, uc.PHASES)) for n, t in uc.case_params(tag).items()}
    ref = uc.forward_host(ps, x, levels, cond, drop, dtype=torch.float32)
    (ref * d_out).sum().backward()
    return d_out, ref.detach(), {n: ps[n].grad for n in trainable(ps)}


@functools.lru_cache(maxsize=None)
def step_inputs():
    g = torch.Generator().manual_seed(3)
    xs = torch.randn(uc.BATCH, uc.MAX_TOKENS, *uc.X_SHAPE, generator=g)
    t = torch.rand(uc.BATCH, uc.MAX_TOKENS, generator=g)
    noise = torch.randn(uc.BATCH, uc.MAX_TOKENS, *uc.X_SHAPE, generator=g)
    return xs, t, noise, uc.inputs()[2]


def flat_view(tr, name, flat):
    o, shp = tr.layout[name]
    return flat[o: o + int(np.prod(shp))].view(shp)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_uvit3d_trainer_backward_matches_autograd(tag):
    """forward and EVERY parameter gradient (no tensor exempted) vs torch autograd through the host restatement, random d_out;
    case c with cond_drop = [True, False]"""
    x, levels, cond, drop = case_inputs(tag)
    d_out, ref, ref_grads = autograd_reference(tag)
    tr = trainer(tag)
    out = tr.forward(x, levels, cond, drop).cpu()
    grads = {n: t.cpu() for n, t in tr.backward(d_out).items()}
    assert sorted(grads) == sorted(ref_grads)
    r_out = rel(out, ref)
    rs = {n: rel(grads[n], ref_grads[n]) for n in ref_grads}
    worst = max(rs, key=rs.get)
    print(f"UViT3DTrainer case {tag}: forward rel-L2 {r_out:.2e}; worst gradient rel-L2 {rs[worst]:.2e} at {worst}")
    assert r_out < 2e-2 and rs[worst] < 3e-2, (r_out, worst, rs[worst])


def test_row_film_and_frame_film_paths_agree():
    """the A/B switch as a constructor keyword: the per-row yardstick (film broadcast to [rows][2C] bf16, per-row ops, frame_sums) and the
    per-frame kernels give the same training step within the bar for regrouped bf16 work"""
    xs, t, noise, cond = step_inputs()
    row, frm = trainer("c", row_film=True), trainer("c", row_film=False)
    assert row.row_film and not frm.row_film
    l_row = float(row.loss_and_grads(xs, cond, t, noise, cond_drop=DROP).item())
    l_frm = float(frm.loss_and_grads(xs, cond, t, noise, cond_drop=DROP).item())
    rs = {n: rel(flat_view(frm, n, frm.flat_grads), flat_view(row, n, row.flat_grads)) for n in frm.layout}
    worst = max(rs, key=rs.get)
    print(f"row vs frame FiLM: loss {l_row:.6f} / {l_frm:.6f}; worst gradient rel-L2 {rs[worst]:.2e} at {worst}")
    assert abs(l_row - l_frm) < 1e-3 * abs(l_row)
    assert rs[worst] < 2e-2, (worst, rs[worst])


def test_uvit3d_training_gradients_are_bit_reproducible():
    xs, t, noise, cond = step_inputs()
    tr = trainer("c")
    l0 = float(tr.loss_and_grads(xs, cond, t, noise, cond_drop=DROP).item())
    g0 = tr.flat_grads.clone()
    l1 = float(tr.loss_and_grads(xs, cond, t, noise, cond_drop=DROP).item())
    assert l0 == l1
    bad = [n for n in tr.layout if not torch.equal(flat_view(tr, n, g0), flat_view(tr, n, tr.flat_grads))]
    assert not bad, f"gradients differ between two runs: {bad[:8]}"
    other = trainer("c")
    other.loss_and_grads(xs, cond, t, noise, cond_drop=DROP)
    assert torch.equal(other.flat_grads, g0)


def test_uvit3d_training_step():
    """loss vs oracle.sampler.training_loss through forward_host, one clipped AdamW step vs torch where the gradient is not negligible (the
    0.1 bar of test_uvit3d_pose_training_step on elements above 2 % of the tensor's largest gradient; its floor of 10000 checked elements scaled
    by this model's share of that model's parameter count), and a finite loss on the next step"""
    from oracle import sampler as osm, uvit as ouvit
    xs, t, noise, cond = step_inputs()
    params = uc.case_params("c")
    tr = trainer("c")
    loss0 = float(tr.loss_and_grads(xs, cond, t, noise, cond_drop=DROP).item())
    before = {n: v.detach().clone().cpu() for n, v in tr.p.items()}
    tr.optimizer_step(lr=1e-4)
    ps = {n: v.clone().requires_grad_(n not in (uc.FREQS, uc.PHASES)) for n, v in params.items()}
    _, per_el = osm.training_loss(lambda x, lv, c, m: uc.forward_host(ps, x, lv, c, DROP, dtype=torch.float32), xs, cond, t, noise)
    ref = per_el.mean()
    ref_loss = float(ref.detach())
    print(f"UViT3DTrainer loss {loss0:.6f} vs oracle {ref_loss:.6f}")
    assert abs(loss0 - ref_loss) < 2e-2 * abs(ref_loss), (loss0, ref_loss)
    ref.backward()
    plist = [v for v in ps.values() if v.requires_grad]
    torch.nn.utils.clip_grad_norm_(plist, 1.0)
    torch.optim.AdamW(plist, lr=1e-4, weight_decay=0.01, betas=(0.9, 0.99), eps=1e-8).step()
    pose = ouvit.UViTConfig(channels=(128, 128, 128, 256), emb_channels=128, num_updown_blocks=(1, 1, 1), num_mid_blocks=1, num_heads=2, resolution=128,
                            max_tokens=2)
    n_pose = sum(int(np.prod(s)) for n, s in ouvit.param_shapes(pose).items() if not n.endswith(("freqs", "phases")))
    floor = int(10000 * sum(v.numel() for v in plist) / n_pose)
    checked = 0
    for n, v in ps.items():
        if not v.requires_grad:
            continue
        big = v.grad.abs() > 2e-2 * v.grad.abs().max()
        if big.any():
            upd, ref_upd = tr.p[n].detach().cpu() - before[n], v.detach() - params[n]
            assert rel(upd[big], ref_upd[big]) < 0.1, n
            checked += int(big.sum())
    print(f"checked {checked} elements (floor {floor})")
    assert checked > floor
    assert np.isfinite(float(tr.loss_and_grads(xs, cond, t, noise, cond_drop=DROP).item()))


def test_uvit3d_trainer_ema_accumulation_state_and_checkpointing():
    """the assertions of test_uvit_trainer_ema_accumulation_state_and_checkpointing on this trainer: the shared code serves both"""
    xs, t, noise, cond = step_inputs()
    run = lambda tr_, sl=slice(None): tr_.loss_and_grads(xs[sl], cond[sl], t[sl], noise[sl], cond_drop=DROP[sl])
    tr = trainer("c")
    loss0 = float(run(tr).item())
    g_ref = tr.flat_grads.clone()
    ck = trainer("c", cfg=dict(use_checkpointing=[False, True, True, True]))
    loss1 = float(run(ck).item())
    assert all("xn" not in b.saved for b in ck.mid) and all("h1" not in b.saved for b in ck.down[1])
    assert abs(loss1 - loss0) < 1e-6 * abs(loss0)
    assert torch.equal(ck.flat_grads, g_ref), rel(ck.flat_grads, g_ref)
    acc = trainer("c")
    gs = []
    for i in range(2):
        run(acc, slice(i, i + 1))
        gs.append(acc.flat_grads.clone())
        acc.accumulate()
    acc.enable_ema(0.9)
    before = acc.flat.clone()
    acc.optimizer_step(lr=1e-4, max_grad_norm=None)
    one = trainer("c")
    one.flat_grads.copy_(0.5 * (gs[0] + gs[1]))
    one.optimizer_step(lr=1e-4, max_grad_norm=None)
    assert torch.equal(acc.flat, one.flat) and acc._acc_n == 0
    ema1 = 0.9 * before + 0.1 * acc.flat
    assert rel(acc.ema, ema1) < 1e-6
    run(acc)
    acc.optimizer_step(lr=1e-4)
    assert rel(acc.ema, 0.9 * ema1 + 0.1 * acc.flat) < 1e-6
    sd = acc.ema_state_dict()
    assert list(sd) == list(acc.layout) == trainable(uc.case_params("c")) and all(tuple(sd[n].shape) == acc.layout[n][1] for n in sd)
    osd = acc.optimizer_state_dict()
    assert len(osd["state"]) == len(acc.layout) and osd["param_groups"][0]["lr"] == 1e-4 and float(osd["state"][0]["step"]) == 2.0
    import dfot_amd
    res = dfot_amd.UViT3DTrainer(acc.state_dict(), tcfg("c"))
    res.load_optimizer_state_dict(osd)
    assert res.step_count == 2
    res.enable_ema(0.9)
    res.load_ema_state_dict(sd)
    for tr_ in (acc, res):
        run(tr_)
        tr_.optimizer_step(lr=1e-4)
    assert rel(res.flat, acc.flat) < 1e-5 and rel(res.ema, acc.ema) < 1e-5
    with pytest.raises(ValueError):
        res.load_ema_state_dict({"nope": torch.zeros(1)})


def test_uvit3d_forward_under_autograd_still_raises():
    """the boundary next to the trainer: the drop-in module stays forward only"""
    model, _ = uc.build("a")
    x, levels, _, _ = uc.inputs()
    with pytest.raises(NotImplementedError):
        model(x.cuda().requires_grad_(), levels.cuda())


@pytest.mark.parametrize("tag", ["a", "c"])
def test_uvit3d_training_gradients_vs_reference_fixture(tag):
    """loss and gradients of the reference's own UViT3D training step (tests/golden/uvit3d_train.npz: ContinuousDiffusion.forward +
    _reweight_loss with one masked token, differentiated by the reference's autograd on CPU) vs the engine: the loss, the norm of EVERY
    gradient and every stored gradient tensor, at the bars of test_training_gradients_vs_reference_fixture"""
    import uvit3d_train_common as utc
    g = uc.load("uvit3d_train.npz")
    xs, t, masks, _ = utc.train_inputs()
    cond, drop = utc.case_cond(tag)
    tr = trainer(tag)
    loss = float(tr.loss_and_grads(xs, cond, t, utc.train_noise(), masks, cond_drop=drop).item())
    ref_loss = float(g[f"{tag}_loss"])
    grads = {n: v.cpu() for n, v in tr.grads.items()}
    names = [str(n) for n in g[f"{tag}_names"]]
    assert names == list(tr.layout) and sorted(names) == sorted(grads)
    norm_dev = {n: abs(float(grads[n].norm()) - ref_norm) / ref_norm for n, ref_norm in zip(names, g[f"{tag}_norms"])}
    worst_norm = max(norm_dev, key=norm_dev.get)
    rs = {key.split("/", 1)[1]: rel(grads[key.split("/", 1)[1]], uc.T(g[key])) for key in g.files if key.startswith(f"{tag}_grad/")}
    worst = max(rs, key=rs.get)
    print(f"case {tag}: loss {loss:.6f} vs the reference {ref_loss:.6f} ({abs(loss - ref_loss) / abs(ref_loss):.2e}); worst gradient-norm deviation "
          f"{norm_dev[worst_norm]:.2e} at {worst_norm}; worst stored-gradient rel-L2 {rs[worst]:.2e} at {worst}")
    assert abs(loss - ref_loss) < 2e-2 * abs(ref_loss), (loss, ref_loss)
    assert norm_dev[worst_norm] <= 5e-2, (worst_norm, norm_dev[worst_norm])
    assert rs[worst] < 5e-2, (worst, rs[worst])
