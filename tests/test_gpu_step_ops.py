"""Op-level tests of the sampler-step, loss and optimizer kernels behind the plain dfot_* names (csrc/kernels.hip): dfot_hg_prepare,
dfot_ddim_compose(_tokw), dfot_ddim_noise, dfot_vpred_loss / dfot_vspace_loss / dfot_vloss_grad, dfot_sumsq, dfot_adamw_step.

Every reference is the documented formula (include/dfot_hip.h) evaluated by torch in float64 on the same fp32 inputs.  Every output and
scratch buffer is NaN-prefilled, every operand the contract says is not read is NaN there, and the groups of four elements at each edge
a kernel has (start / end of a row, the 1024-element workgroup / stride edge, the 4096-element chunk edge) are amplified x8 so that a
dropped or doubled group moves the result far past the bar.

Bars: elementwise fp32 outputs rtol = atol = 1e-5 (the bar test_sampler_step_kernels holds ddim_compose to); sums of non-negative terms
(per-token loss, sumsq) 1e-5 relative; copied-through values bit-identical; AdamW against the fp32 error of torch.optim.AdamW itself."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
F64 = torch.float64


@pytest.fixture(scope="module")
def capi():
    import dfot_amd  # noqa: F401
    from dfot_amd import capi as c
    assert torch.cuda.is_available()
    return c


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def nan_buf(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device="cuda", dtype=dtype)


def edge_mask(f):
    """the groups of four at every edge: start of row, end of row, 1020-1027, 4092-4099"""
    m = torch.zeros(f, dtype=torch.bool)
    for lo, hi in ((0, 4), (f - 4, f), (1020, 1028), (4092, 4100)):
        m[max(lo, 0):max(min(hi, f), 0)] = True
    return m


def spiked(g, *shape):
    t = torch.randn(*shape, generator=g)
    t[..., edge_mask(shape[-1])] *= 8.0
    return t


def close(got, ref64, what):
    got = got.detach().cpu()
    assert torch.isfinite(got).all(), f"{what}: output not finite (a NaN operand was read, or an element was not written)"
    np.testing.assert_allclose(got.double().numpy(), ref64.numpy(), rtol=1e-5, atol=1e-5, err_msg=what)


def e_(t):
    return t[..., None]


# ---------------------------------------------------------------------------------------------------------------------
# 1. sampler step
# ---------------------------------------------------------------------------------------------------------------------
# one thread; several rows in one partial workgroup; f/4 = 257 and 1025 (no power of two: the % and / index split) over several workgroups
SAMPLER_SHAPES = [(1, 1, 1, 4), (2, 3, 5, 12), (3, 2, 7, 1028), (2, 2, 8, 4100)]


@functools.lru_cache(maxsize=None)
def sampler_case(b, nfe, t, f):
    """host fp32 inputs of one sampler step, already poisoned where the contract says an operand is not read"""
    g = torch.Generator().manual_seed(1000 * b + 100 * nfe + 10 * t + f)
    rows = b * nfe
    d = {}
    d["x"] = spiked(g, b, t, f)
    # hg_prepare: qb == 0 (and qa == 1: kept history) on every third (row, token), noise NaN there
    th = torch.rand(rows, t, generator=g) * 1.4 + 0.1
    kept = (torch.arange(rows * t).view(rows, t) % 3) == 1
    d["qa"] = torch.where(kept, torch.ones(()), th.cos())
    d["qb"] = torch.where(kept, torch.zeros(()), th.sin())
    d["noise"] = spiked(g, rows, t, f)
    d["noise"][kept] = NAN
    # ddim_compose
    d["gen"] = ((torch.arange(b)[:, None] + torch.arange(t)[None]) % 3 != 1).to(torch.uint8)
    d["keep"] = ((torch.arange(rows)[:, None] + torch.arange(t)[None]) % 3 == 1).float()
    gen_rows = d["gen"].bool().repeat_interleave(nfe, 0)           # (rows, t): the token of this branch row is generated
    computed = gen_rows & (d["keep"] == 0)
    k, n_ = torch.rand(rows, t, generator=g) * 1.4 + 0.1, torch.rand(rows, t, generator=g) * 1.4 + 0.1
    d["sa"], d["s1"], d["an"], d["cn"] = k.cos(), k.sin(), n_.cos(), n_.sin()
    d["x_in"] = spiked(g, rows, t, f)
    d["x_in"][~gen_rows] = NAN
    d["v"] = spiked(g, rows, t, f)
    d["v"][~computed] = NAN
    d["w"] = torch.tensor([1.5, -0.75, 0.25])[:nfe].contiguous()
    d["w_tok"] = (d["w"][:, None] * (1.0 + 0.25 * torch.arange(t)[None])).contiguous()   # differs along t
    # ddim_noise: sigma == 0 on kept rows and on every fourth row besides; noise NaN wherever its coefficient is 0 or gen is 0
    sg = torch.rand(rows, t, generator=g) * 0.5 + 0.1
    sg[(d["keep"] != 0) | ((torch.arange(rows * t).view(rows, t) % 4) == 2)] = 0.0
    d["sigma"] = sg
    d["w_tok0"] = d["w_tok"].clone()
    if nfe * t > 1:
        d["w_tok0"][-1, -1] = 0.0                                   # sigma * w == 0 through the weight
    d["x_next0"] = spiked(g, b, t, f)
    d["eps"] = spiked(g, rows, t, f)
    if t > 1:
        assert all(0 < int(d["gen"][i].sum()) < t for i in range(b)), "gen must hold both values within one video"
        assert 0 < int(d["keep"][0].sum()) < t, "keep must hold both values within one branch"
    return d


def compose_ref(d, b, nfe, t, f, w):
    """float64 x_next of dfot_ddim_compose / _tokw (w: [nfe] or [nfe, t])"""
    x_in, v = d["x_in"].double().nan_to_num(0.0), d["v"].double().nan_to_num(0.0)
    sa, s1, an, cn = (e_(d[k].double()) for k in ("sa", "s1", "an", "cn"))
    x0 = sa * x_in - s1 * v
    ep = sa * v + s1 * x_in
    xp = torch.where(e_(d["keep"]) != 0, x_in, x0 * an + ep * cn).view(b, nfe, t, f)
    wv = w.double().view(1, nfe, -1, 1)
    return torch.where(e_(d["gen"].bool()), (xp * wv).sum(1), d["x"].double())


def run_compose(capi, d, b, nfe, t, f, w, tokw):
    dev = {k: d[k].cuda() for k in ("x", "x_in", "v", "sa", "s1", "an", "cn", "keep", "gen")}
    wd = w.cuda()
    out = nan_buf(b, t, f)
    fn = capi.lib.dfot_ddim_compose_tokw if tokw else capi.lib.dfot_ddim_compose
    capi.check(fn(P(dev["x"]), P(dev["x_in"]), P(dev["v"]), P(dev["sa"]), P(dev["s1"]), P(dev["an"]), P(dev["cn"]), P(dev["keep"]), P(wd),
                  P(dev["gen"]), P(out), b, nfe, t, f, S()))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("b,nfe,t,f", SAMPLER_SHAPES)
def test_hg_prepare(capi, b, nfe, t, f):
    """x_in = qa * x + qb * noise per (branch row, token); noise is not read where qb == 0, and may be NULL when every qb is 0"""
    d = sampler_case(b, nfe, t, f)
    xr = d["x"].repeat_interleave(nfe, 0)
    x, noise, qa, qb = d["x"].cuda(), d["noise"].cuda(), d["qa"].cuda(), d["qb"].cuda()
    x_in = nan_buf(b * nfe, t, f)
    capi.check(capi.lib.dfot_hg_prepare(P(x), P(noise), P(qa), P(qb), P(x_in), b, nfe, t, f, S()))
    ref = e_(d["qa"].double()) * xr.double() + e_(d["qb"].double()) * d["noise"].double().nan_to_num(0.0)
    close(x_in, ref, "hg_prepare")
    kept = d["qb"] == 0
    assert torch.equal(x_in.cpu()[kept], xr[kept]), "rows with qa = 1, qb = 0 must be copied bit for bit"
    # every qb == 0: the sampler passes noise = NULL
    x_in2 = nan_buf(b * nfe, t, f)
    zero = torch.zeros_like(qb)
    capi.check(capi.lib.dfot_hg_prepare(P(x), None, P(qa), P(zero), P(x_in2), b, nfe, t, f, S()))
    close(x_in2, e_(d["qa"].double()) * xr.double(), "hg_prepare without noise")
    assert torch.equal(x_in2.cpu()[kept], xr[kept])


@pytest.mark.parametrize("b,nfe,t,f", SAMPLER_SHAPES)
def test_ddim_compose(capi, b, nfe, t, f):
    """both weight forms against float64; v is NaN on kept rows, v and x_in are NaN on non-generated tokens (not read by contract);
    non-generated tokens come back as x bit for bit; a weight[nfe][t] table constant along t is the weight[nfe] form bit for bit"""
    d = sampler_case(b, nfe, t, f)
    gen = d["gen"].bool()
    plain = run_compose(capi, d, b, nfe, t, f, d["w"], False)
    close(plain, compose_ref(d, b, nfe, t, f, d["w"]), "ddim_compose")
    assert torch.equal(plain[~gen], d["x"][~gen])
    tok = run_compose(capi, d, b, nfe, t, f, d["w_tok"], True)
    close(tok, compose_ref(d, b, nfe, t, f, d["w_tok"]), "ddim_compose_tokw")    # reading weight[h] instead of weight[h*t + tk] fails here
    assert torch.equal(tok[~gen], d["x"][~gen])
    const = run_compose(capi, d, b, nfe, t, f, d["w"][:, None].repeat(1, t).contiguous(), True)
    assert torch.equal(const, plain)


@pytest.mark.parametrize("tokw", [0, 1])
@pytest.mark.parametrize("b,nfe,t,f", SAMPLER_SHAPES)
def test_ddim_noise(capi, b, nfe, t, f, tokw):
    """x_next += sum_h w * sigma * noise on generated tokens, untouched elsewhere; noise is NaN wherever sigma * w == 0 or gen == 0"""
    d = sampler_case(b, nfe, t, f)
    gen = d["gen"].bool()
    w = d["w_tok0"] if tokw else d["w"]
    coef = d["sigma"].double().view(b, nfe, t) * w.double().view(1, nfe, -1)             # (b, nfe, t)
    noise = d["eps"].clone()
    noise[(coef.reshape(b * nfe, t) == 0) | ~gen.repeat_interleave(nfe, 0)] = NAN
    x_next = d["x_next0"].cuda()
    nd, sd, wd, gd = noise.cuda(), d["sigma"].cuda(), w.cuda(), d["gen"].cuda()
    capi.check(capi.lib.dfot_ddim_noise(P(nd), P(sd), P(wd), P(gd), P(x_next), b, nfe, t, f, tokw, S()))
    add = (e_(coef) * noise.double().nan_to_num(0.0).view(b, nfe, t, f)).sum(1)
    ref = torch.where(e_(gen), d["x_next0"].double() + add, d["x_next0"].double())
    close(x_next, ref, "ddim_noise")
    assert torch.equal(x_next.cpu()[~gen], d["x_next0"][~gen])
    if nfe * t > 1:
        assert (add.abs().amax(-1)[gen] > 0).any(), "the case must add noise somewhere"


def test_sampler_torch_ops_equal_the_direct_calls(capi):
    """dfot::hg_prepare and dfot::ddim_hg_step (both weight ranks) return the bits of the C entry points they wrap"""
    b, nfe, t, f = SAMPLER_SHAPES[1]
    d = sampler_case(b, nfe, t, f)
    dev = {k: v.cuda() for k, v in d.items()}
    x_in = nan_buf(b * nfe, t, f)
    capi.check(capi.lib.dfot_hg_prepare(P(dev["x"]), P(dev["noise"]), P(dev["qa"]), P(dev["qb"]), P(x_in), b, nfe, t, f, S()))
    got = torch.ops.dfot.hg_prepare(dev["x"], dev["noise"], dev["qa"], dev["qb"], nfe)
    assert torch.isfinite(got).all() and torch.equal(got, x_in)
    for w, tokw in ((d["w"], False), (d["w_tok"], True)):
        direct = run_compose(capi, d, b, nfe, t, f, w, tokw)
        got = torch.ops.dfot.ddim_hg_step(dev["x"], dev["x_in"], dev["v"], dev["sa"], dev["s1"], dev["an"], dev["cn"], dev["keep"], w.cuda(),
                                          dev["gen"], nfe)
        assert torch.isfinite(got).all() and torch.equal(got.cpu(), direct)


# ---------------------------------------------------------------------------------------------------------------------
# 2. loss and its gradient
# ---------------------------------------------------------------------------------------------------------------------
# below one 1024 stride; around one stride; around one 4096 chunk; two whole chunks; three chunks and a 4-element fourth
LOSS_F = [4, 8, 1020, 1024, 1028, 4092, 4096, 4100, 8192, 12292]
LOSS_BT = [(1, 1), (7, 1), (1, 7), (2, 3)]


@functools.lru_cache(maxsize=None)
def loss_case(bt, f, seed):
    g = torch.Generator().manual_seed(7919 * seed + 31 * bt + f)
    d = {k: spiked(g, bt, f) for k in ("x", "noise", "v")}
    th = torch.rand(bt, generator=g) * 0.9 + 0.4        # cos^2 in [0.07, 0.85]: eps-space loss = alpha^2 * v-space loss, > 10 % apart
    d["alpha"], d["sigma"] = th.cos(), th.sin()
    d["w"] = torch.rand(bt, generator=g) + 0.5
    if bt > 1:
        d["w"][1] = 0.0
    d["coef"] = torch.randn(bt, generator=g)
    return d


def loss_ref(d, vspace):
    """float64 (per-token loss, x_pred, unweighted error d)"""
    x, n, v = d["x"].double(), d["noise"].double(), d["v"].double()
    a, s = e_(d["alpha"].double()), e_(d["sigma"].double())
    xt = a * x + s * n
    err = v - (a * n - s * x) if vspace else (a * v + s * xt) - n
    return (err * err * e_(d["w"].double())).mean(-1), a * xt - s * v, err


def run_loss(capi, d, b, t, f, vspace, scratch, want_x_pred):
    dev = {k: d[k].cuda() for k in ("x", "noise", "v", "alpha", "sigma", "w")}
    loss = nan_buf(b * t)
    x_pred = nan_buf(b * t, f) if want_x_pred else None
    fn = capi.lib.dfot_vspace_loss if vspace else capi.lib.dfot_vpred_loss
    capi.check(fn(P(dev["x"]), P(dev["noise"]), P(dev["v"]), P(dev["alpha"]), P(dev["sigma"]), P(dev["w"]), P(x_pred), P(scratch), P(loss),
                  b, t, f, S()))
    torch.cuda.synchronize()
    return loss.cpu(), (x_pred.cpu() if want_x_pred else None)


@pytest.mark.parametrize("vspace", [0, 1])
@pytest.mark.parametrize("b,t", LOSS_BT)
@pytest.mark.parametrize("f", LOSS_F)
def test_vloss(capi, f, b, t, vspace):
    """per-token loss within 1e-5 relative of float64 mean_f(d^2 w) (non-negative terms); exactly 0.0 on the w == 0 row; x_pred at the
    elementwise bar; scratch sized exactly by dfot_vpred_loss_scratch_floats and reusable with stale partials in it"""
    bt = b * t
    n_scratch = int(capi.lib.dfot_vpred_loss_scratch_floats(b, t, f))
    assert n_scratch == bt * ((f + 4095) // 4096)
    first, d = loss_case(bt, f, 1), loss_case(bt, f, 2)
    scratch = nan_buf(n_scratch)
    run_loss(capi, first, b, t, f, vspace, scratch, True)
    assert torch.isfinite(scratch).all(), "every partial of the scratch buffer must be written"
    loss, x_pred = run_loss(capi, d, b, t, f, vspace, scratch, True)        # the scratch now holds the partials of other inputs
    fresh, _ = run_loss(capi, d, b, t, f, vspace, nan_buf(n_scratch), True)
    assert torch.equal(loss, fresh), "the result depends on what the scratch buffer held"
    none, _ = run_loss(capi, d, b, t, f, vspace, nan_buf(n_scratch), False)
    assert torch.equal(loss, none), "x_pred = NULL changes the loss"
    ref, ref_pred, _ = loss_ref(d, vspace)
    other, _, _ = loss_ref(d, not vspace)
    pos = d["w"] > 0
    assert ((ref - other).abs()[pos] > 0.1 * torch.maximum(ref, other)[pos]).all(), "the case does not tell the two spaces apart"
    assert torch.isfinite(loss).all()
    rel = ((loss.double() - ref).abs()[pos] / ref[pos]).max().item()
    print(f"vloss vspace={vspace} bt={b}x{t} f={f}: worst per-token rel err {rel:.3e} (bar 1e-5)")
    assert rel <= 1e-5
    assert (loss[~pos] == 0.0).all(), "a token of weight 0 has loss exactly 0"
    close(x_pred, ref_pred, "x_pred")


@pytest.mark.parametrize("vspace", [0, 1])
@pytest.mark.parametrize("b,t,f", [(1, 1, 4), (7, 1, 1028), (2, 3, 4100), (1, 7, 12292)])
def test_vloss_grad(capi, b, t, f, vspace):
    """dv against the closed form coef * d * dd/dv, and against autograd of the loss it claims to differentiate.  The kernel comment
    says dv = coef[bt] * d(loss term)/dv with the factor 2 / f and the weight left out (the trainers fold them into coef): with
    loss_term = mean_f(d^2), d(loss_term)/dv = (2 / f) d dd/dv, so dv is the gradient of  L = sum_bt coef[bt] * (f / 2) * loss_term[bt]."""
    bt = b * t
    d = loss_case(bt, f, 3)
    dev = {k: d[k].cuda() for k in ("x", "noise", "v", "alpha", "sigma", "coef")}
    dv = nan_buf(bt, f)
    capi.check(capi.lib.dfot_vloss_grad(P(dev["x"]), P(dev["noise"]), P(dev["v"]), P(dev["alpha"]), P(dev["sigma"]), P(dev["coef"]), P(dv),
                                        b, t, f, vspace, S()))
    _, _, err = loss_ref(d, vspace)
    cf = e_(d["coef"].double())
    closed = cf * err * (1.0 if vspace else e_(d["alpha"].double()))
    close(dv, closed, "vloss_grad vs closed form")
    v = d["v"].double().requires_grad_()
    ones = dict(d, v=v, w=torch.ones(bt))
    term, _, _ = loss_ref(ones, vspace)
    grad, = torch.autograd.grad((d["coef"].double() * (f / 2) * term).sum(), v)
    close(dv, grad, "vloss_grad vs autograd")


# ---------------------------------------------------------------------------------------------------------------------
# 3. sumsq
# ---------------------------------------------------------------------------------------------------------------------
def run_sumsq(capi, x, prefill=NAN):
    out = torch.full((1,), prefill, device="cuda")
    capi.check(capi.lib.dfot_sumsq(P(x), x.numel(), P(out), S()))
    torch.cuda.synchronize()
    return out.cpu()


# scalar tail of 1-3 elements with and without a float4 body; one workgroup edge; the fixed grid stride of 1024 * 1024 elements and past it
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1025, 2 ** 20, 2 ** 20 + 1, 2 ** 20 + 5, 2 ** 21 + 7])
def test_sumsq(capi, n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    x[-3:] *= 1e3                                                    # a dropped tail element dominates
    other = torch.randn(n, generator=g).cuda()
    xd = x.cuda()
    ref = x.double().pow(2).sum().item()
    got = run_sumsq(capi, xd)
    assert torch.isfinite(got).all()
    rel = abs(got.item() - ref) / ref
    print(f"sumsq n={n}: rel err {rel:.3e} (bar 1e-5; torch fp32 sum {abs(x.pow(2).sum().item() - ref) / ref:.3e})")
    assert rel <= 1e-5
    assert torch.equal(run_sumsq(capi, xd), got), "two calls on the same input differ"
    run_sumsq(capi, other)                                           # the per-workgroup partials are one static buffer of the process
    assert torch.equal(run_sumsq(capi, xd), got), "a call on another input in between changed the result"
    assert torch.equal(run_sumsq(capi, xd, prefill=3e30), got), "out must be overwritten, not accumulated into"


def test_sumsq_refuses_a_misaligned_buffer(capi):
    buf = torch.ones(64, device="cuda")
    out = nan_buf(1)
    with pytest.raises(capi.DfotError) as e:
        capi.check(capi.lib.dfot_sumsq(P(buf[1:]), 60, P(out), S()))
    torch.cuda.synchronize()
    assert e.value.code == capi.ERR_ARG
    assert torch.isnan(out).all(), "a refused call wrote to out"
    assert run_sumsq(capi, buf).item() == 64.0


# ---------------------------------------------------------------------------------------------------------------------
# 4. AdamW (+ clip + EMA), single steps from an injected state
# ---------------------------------------------------------------------------------------------------------------------
ADAM_N = 100003
ADAM_EPS = 1e-8
EMA_DECAY = 0.999
# each beta pair, weight decay and learning rate appears with each step
ADAM_HYPER = {"a": dict(betas=(0.9, 0.99), wd=0.0, lr=1e-3), "b": dict(betas=(0.9, 0.999), wd=0.01, lr=1e-1)}
ADAM_STEPS = [1, 2, 3, 10, 1000]
QUANTITIES = ("delta", "m", "v", "ema-p")


def f32(x):
    """the value the C ABI receives for a float argument"""
    return float(np.float32(x))


@functools.lru_cache(maxsize=None)
def adam_state(family):
    """p, g, m, v, ema of ADAM_N elements; |m| and |g| span four decades; 'same': sign(m) == sign(g), so nothing cancels in the new m and
    per-element relative error means something; 'indep': independent signs"""
    g_ = torch.Generator().manual_seed({"same": 11, "indep": 12}[family])
    n = ADAM_N
    sign = lambda: torch.where(torch.rand(n, generator=g_) < 0.5, -1.0, 1.0)
    mag = lambda: 10.0 ** (-4.0 * torch.rand(n, generator=g_)) * (0.5 + torch.rand(n, generator=g_))
    sg = sign()
    grad = mag() * sg
    m = mag() * (sg if family == "same" else sign())
    v = grad.square() * (0.25 + 1.5 * torch.rand(n, generator=g_))
    p = torch.randn(n, generator=g_)
    ema = p + 0.01 * torch.randn(n, generator=g_)
    return dict(p=p, g=grad, m=m, v=v, ema=ema)


def adam_ref64(st, n, step, betas, wd, lr, sumsq=None, max_norm=0.0):
    """torch.optim.AdamW semantics in float64 on the float32-rounded hyper-parameters: decoupled decay, step_size = lr / c1,
    denom = sqrt(v) / sqrt(c2) + eps, c = 1 - beta^step in double; clip_grad_norm_; EMA.  Returns the four judged quantities."""
    b1, b2, lr, wd, eps, dec = f32(betas[0]), f32(betas[1]), f32(lr), f32(wd), f32(ADAM_EPS), f32(EMA_DECAY)
    p, g, m, v, ema = (st[k][:n].double() for k in ("p", "g", "m", "v", "ema"))
    if sumsq is not None:
        g = g * min(1.0, f32(max_norm) / (math.sqrt(sumsq) + 1e-6))
    m2 = b1 * m + (1 - b1) * g
    v2 = b2 * v + (1 - b2) * g * g
    c1, c2 = 1 - b1 ** step, 1 - b2 ** step
    p2 = p * (1 - lr * wd) - (lr / c1) * m2 / (v2.sqrt() / math.sqrt(c2) + eps)
    ema2 = dec * ema + (1 - dec) * p2
    return {"delta": p2 - p, "m": m2, "v": v2, "ema-p": ema2 - p2}


def judged(st, n, p2, m2, v2, ema2):
    return {"delta": p2.double() - st["p"][:n].double(), "m": m2.double(), "v": v2.double(), "ema-p": ema2.double() - p2.double()}


def adam_torch32(st, n, step, betas, wd, lr, clip_to=None):
    """the yardstick: torch.optim.AdamW(foreach=False) in fp32 on the CPU with the state injected, then the plain fp32 EMA line"""
    p = st["p"][:n].clone().requires_grad_()
    p.grad = st["g"][:n].clone()
    if clip_to is not None:
        torch.nn.utils.clip_grad_norm_([p], f32(clip_to), foreach=False)
    opt = torch.optim.AdamW([p], lr=f32(lr), betas=(f32(betas[0]), f32(betas[1])), eps=f32(ADAM_EPS), weight_decay=f32(wd), foreach=False)
    opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": st["m"][:n].clone(), "exp_avg_sq": st["v"][:n].clone()}
    opt.step()
    s = opt.state[p]
    assert int(s["step"].item()) == step
    pn = p.detach()
    ema = f32(EMA_DECAY) * st["ema"][:n] + (1.0 - f32(EMA_DECAY)) * pn
    return judged(st, n, pn, s["exp_avg"], s["exp_avg_sq"], ema)


def adam_kernel(capi, st, n, step, betas, wd, lr, sumsq=None, max_norm=0.0, ema=True, pad=300):
    """one dfot_adamw_step on device copies of the first n elements, in buffers `pad` elements too long (NaN behind n)"""
    bufs = {}
    for k in ("p", "g", "m", "v", "ema"):
        bufs[k] = nan_buf(n + pad)
        bufs[k][:n] = st[k][:n].cuda()
    capi.check(capi.lib.dfot_adamw_step(P(bufs["p"]), P(bufs["g"]), P(bufs["m"]), P(bufs["v"]), n, lr, betas[0], betas[1], ADAM_EPS, wd, step,
                                        P(sumsq), max_norm, P(bufs["ema"]) if ema else None, EMA_DECAY, S()))
    torch.cuda.synchronize()
    out = {k: t.cpu() for k, t in bufs.items()}
    for k, t in out.items():
        assert torch.isnan(t[n:]).all(), f"adamw wrote {k} at an index >= n"
        assert torch.isfinite(t[:n]).all()
    return {k: t[:n] for k, t in out.items()}


def rel_l2(got, ref):
    return ((got - ref).norm() / ref.norm()).item()


def worst_rel(got, ref):
    return ((got - ref).abs() / ref.abs()).max().item()


@functools.lru_cache(maxsize=None)
def adam_yardstick(family, step, hyper, clip_to=None, sumsq=None):
    """fp32 error of torch.optim.AdamW against float64 over the whole ADAM_N-element state: (rel-L2, worst element) per quantity.  It is
    measured on the whole population also for the short runs: over 1 or 255 elements it is a noisy figure that can be exactly 0."""
    st, h = adam_state(family), ADAM_HYPER[hyper]
    ref = adam_ref64(st, ADAM_N, step, h["betas"], h["wd"], h["lr"], sumsq, clip_to or 0.0)
    y = adam_torch32(st, ADAM_N, step, h["betas"], h["wd"], h["lr"], clip_to)
    return {q: (rel_l2(y[q], ref[q]), worst_rel(y[q], ref[q])) for q in QUANTITIES}


def judge_adam(tag, family, n, out, st, ref, yard):
    """rel-L2 of each quantity <= 4 x the yardstick's; on the same-sign family also every element <= 4 x the yardstick's worst element.
    The factor 4 is for fused-multiply-add contraction and the other association of lr / c1 * m / denom.  A single element (n = 1) has no
    population to average over, so it is held to the worst-element figure alone."""
    got = judged(st, n, out["p"], out["m"], out["v"], out["ema"])
    for q in QUANTITIES:
        l2, worst = rel_l2(got[q], ref[q]), worst_rel(got[q], ref[q])
        print(f"adamw {tag} {family} n={n} {q:6s}: rel_l2 {l2:.3e} (torch fp32 {yard[q][0]:.3e})  worst element {worst:.3e} (torch fp32 {yard[q][1]:.3e})")
        if n > 1:
            assert l2 <= 4 * yard[q][0], f"{q}: rel-L2 {l2:.3e} above 4 x {yard[q][0]:.3e}"
        if family == "same":
            assert worst <= 4 * yard[q][1], f"{q}: worst element {worst:.3e} above 4 x {yard[q][1]:.3e}"


@pytest.mark.parametrize("family", ["same", "indep"])
@pytest.mark.parametrize("hyper", sorted(ADAM_HYPER))
@pytest.mark.parametrize("step", ADAM_STEPS)
def test_adamw_step_vs_float64(capi, step, hyper, family):
    st, h = adam_state(family), ADAM_HYPER[hyper]
    yard = adam_yardstick(family, step, hyper)
    for n in (1, 255, 257, ADAM_N):
        if n == 1 and family != "same":
            continue
        out = adam_kernel(capi, st, n, step, h["betas"], h["wd"], h["lr"])
        ref = adam_ref64(st, n, step, h["betas"], h["wd"], h["lr"])
        judge_adam(f"step={step} {hyper}", family, n, out, st, ref, yard)


@pytest.mark.parametrize("family", ["same", "indep"])
@pytest.mark.parametrize("step,hyper", [(1, "b"), (2, "a"), (10, "b")])
def test_adamw_clips_with_the_norm_of_dfot_sumsq(capi, step, hyper, family):
    """clipping engaged as the trainers use the pair: dfot_sumsq on g feeds dfot_adamw_step; max_norm is a tenth of the gradient norm, so
    sumsq = 100 * max_norm^2 and the coefficient is about 0.1"""
    st, h = adam_state(family), ADAM_HYPER[hyper]
    n = ADAM_N
    sumsq64 = st["g"].double().pow(2).sum().item()
    max_norm = f32(math.sqrt(sumsq64) / 10)
    gd = st["g"].cuda()
    ss = nan_buf(1)
    capi.check(capi.lib.dfot_sumsq(P(gd), n, P(ss), S()))
    out = adam_kernel(capi, st, n, step, h["betas"], h["wd"], h["lr"], sumsq=ss, max_norm=max_norm)
    ref = adam_ref64(st, n, step, h["betas"], h["wd"], h["lr"], sumsq64, max_norm)
    free = adam_ref64(st, n, step, h["betas"], h["wd"], h["lr"])
    assert rel_l2(ref["m"], free["m"]) > 1e-2, "the case must engage the clip"
    judge_adam(f"clipped step={step} {hyper}", family, n, out, st, ref, adam_yardstick(family, step, hyper, max_norm, sumsq64))


@pytest.mark.parametrize("n", [1, 257, 100003])
def test_adamw_identities(capi, n):
    """bit-exact: no grad_sumsq == a grad_sumsq below max_norm^2; ema = NULL leaves p, m, v as with EMA; wd = 0 and lr = 0 leave p alone
    while m and v update (indices >= n of the oversized buffers stay NaN in every run: adam_kernel)"""
    st, h = adam_state("indep"), ADAM_HYPER["b"]
    args = (st, n, 3, h["betas"], h["wd"], h["lr"])
    base = adam_kernel(capi, *args)
    below = torch.tensor([0.25 * 2.0 ** 2], device="cuda")           # norm 1 under max_norm 2: coefficient min(1, 2 / (1 + 1e-6)) = 1
    clipped = adam_kernel(capi, *args, sumsq=below, max_norm=2.0)
    no_ema = adam_kernel(capi, *args, ema=False)
    for k in ("p", "m", "v"):
        assert torch.equal(clipped[k], base[k]), f"{k}: an inactive clip changed the step"
        assert torch.equal(no_ema[k], base[k]), f"{k}: ema = NULL changed the step"
    assert torch.equal(clipped["ema"], base["ema"])
    assert torch.equal(no_ema["ema"], st["ema"][:n]) and not torch.equal(base["ema"], st["ema"][:n])
    still = adam_kernel(capi, st, n, 3, h["betas"], 0.0, 0.0)
    assert torch.equal(still["p"], st["p"][:n]), "lr = 0, wd = 0 moved the parameters"
    assert torch.equal(still["m"], base["m"]) and torch.equal(still["v"], base["v"])
    assert not torch.equal(still["m"], st["m"][:n]) and not torch.equal(still["v"], st["v"][:n])


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals: argument checks that return before any launch
# ---------------------------------------------------------------------------------------------------------------------
def refusal_cases(capi):
    L, N = capi.lib, None
    A, SH = capi.ERR_ARG, capi.ERR_SHAPE

    def hg(b, nfe, t, f, **nul):
        p = lambda k, u: N if nul.get(k) else P(u[k])
        return lambda u: L.dfot_hg_prepare(p("in0", u), p("in1", u), p("tab0", u), p("tab1", u), p("out0", u), b, nfe, t, f, S())

    def comp(fn, b, nfe, t, f, **nul):
        p = lambda k, u: N if nul.get(k) else P(u[k])
        return lambda u: fn(p("in0", u), p("in1", u), p("in2", u), p("tab0", u), p("tab1", u), p("tab2", u), p("tab3", u), p("tab4", u),
                            p("tab5", u), p("gen", u), p("out0", u), b, nfe, t, f, S())

    def noi(b, nfe, t, f, **nul):
        p = lambda k, u: N if nul.get(k) else P(u[k])
        return lambda u: L.dfot_ddim_noise(p("in0", u), p("tab0", u), p("tab1", u), p("gen", u), p("out0", u), b, nfe, t, f, 0, S())

    def loss(fn, b, t, f, **nul):
        p = lambda k, u: N if nul.get(k) else P(u[k])
        return lambda u: fn(p("in0", u), p("in1", u), p("in2", u), p("tab0", u), p("tab1", u), p("tab2", u), p("out0", u), p("out1", u),
                            p("out2", u), b, t, f, S())

    def grad(b, t, f, **nul):
        p = lambda k, u: N if nul.get(k) else P(u[k])
        return lambda u: L.dfot_vloss_grad(p("in0", u), p("in1", u), p("in2", u), p("tab0", u), p("tab1", u), p("tab2", u), p("out0", u),
                                           b, t, f, 0, S())

    def adam(n, step):
        return lambda u: L.dfot_adamw_step(P(u["out0"]), P(u["in0"]), P(u["out1"]), P(u["out2"]), n, 1e-3, 0.9, 0.99, 1e-8, 0.0, step, N, 0.0,
                                           N, 0.0, S())

    cases = {
        "hg_prepare f % 4": (SH, hg(2, 2, 2, 6)), "hg_prepare null": (A, hg(2, 2, 2, 8, tab1=1)),
        "ddim_compose f % 4": (SH, comp(L.dfot_ddim_compose, 2, 2, 2, 6)), "ddim_compose null": (A, comp(L.dfot_ddim_compose, 2, 2, 2, 8, gen=1)),
        "ddim_compose_tokw f % 4": (SH, comp(L.dfot_ddim_compose_tokw, 2, 2, 2, 6)),
        "ddim_compose_tokw null": (A, comp(L.dfot_ddim_compose_tokw, 2, 2, 2, 8, tab5=1)),
        "ddim_noise f % 4": (SH, noi(2, 2, 2, 6)), "ddim_noise null": (A, noi(2, 2, 2, 8, in0=1)),
        "vpred_loss f % 4": (SH, loss(L.dfot_vpred_loss, 2, 2, 6)), "vpred_loss null": (A, loss(L.dfot_vpred_loss, 2, 2, 8, out1=1)),
        "vspace_loss f % 4": (SH, loss(L.dfot_vspace_loss, 2, 2, 6)), "vspace_loss null": (A, loss(L.dfot_vspace_loss, 2, 2, 8, out2=1)),
        "vloss_grad f % 4": (SH, grad(2, 2, 6)), "vloss_grad null": (A, grad(2, 2, 8, tab2=1)),
        "sumsq n = 0": (A, lambda u: L.dfot_sumsq(P(u["in0"]), 0, P(u["out0"]), S())),
        "sumsq n < 0": (A, lambda u: L.dfot_sumsq(P(u["in0"]), -4, P(u["out0"]), S())),
        "sumsq null": (A, lambda u: L.dfot_sumsq(N, 8, P(u["out0"]), S())),
        "sumsq misaligned": (A, lambda u: L.dfot_sumsq(P(u["in0"][1:]), 8, P(u["out0"]), S())),
        "adamw step = 0": (A, adam(8, 0)), "adamw n = 0": (A, adam(0, 1)), "adamw n < 0": (A, adam(-8, 1)),
        "adamw null": (A, lambda u: L.dfot_adamw_step(P(u["out0"]), N, P(u["out1"]), P(u["out2"]), 8, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1, N, 0.0, N,
                                                      0.0, S())),
        # one workgroup row per (video, token) in gridDim.y: 65535 at most
        "vpred_loss bt > 65535": (SH, loss(L.dfot_vpred_loss, 256, 256, 4)), "vspace_loss bt > 65535": (SH, loss(L.dfot_vspace_loss, 65536, 1, 4)),
    }
    for bad in (0, -1):
        for pos, name in enumerate(("batch", "nfe", "tokens", "f")):
            dims = [2, 2, 2, 8]
            dims[pos] = bad
            cases[f"hg_prepare {name} = {bad}"] = (SH, hg(*dims))
            cases[f"ddim_compose {name} = {bad}"] = (SH, comp(L.dfot_ddim_compose, *dims))
            cases[f"ddim_compose_tokw {name} = {bad}"] = (SH, comp(L.dfot_ddim_compose_tokw, *dims))
            cases[f"ddim_noise {name} = {bad}"] = (SH, noi(*dims))
        for pos, name in enumerate(("batch", "tokens", "f")):
            dims = [2, 2, 8]
            dims[pos] = bad
            cases[f"vpred_loss {name} = {bad}"] = (SH, loss(L.dfot_vpred_loss, *dims))
            cases[f"vspace_loss {name} = {bad}"] = (SH, loss(L.dfot_vspace_loss, *dims))
            cases[f"vloss_grad {name} = {bad}"] = (SH, grad(*dims))
    return cases


REFUSALS = (
    ["hg_prepare f % 4", "hg_prepare null", "ddim_compose f % 4", "ddim_compose null", "ddim_compose_tokw f % 4", "ddim_compose_tokw null",
     "ddim_noise f % 4", "ddim_noise null", "vpred_loss f % 4", "vpred_loss null", "vspace_loss f % 4", "vspace_loss null", "vloss_grad f % 4",
     "vloss_grad null", "sumsq n = 0", "sumsq n < 0", "sumsq null", "sumsq misaligned", "adamw step = 0", "adamw n = 0", "adamw n < 0",
     "adamw null", "vpred_loss bt > 65535", "vspace_loss bt > 65535"]
    + [f"{fn} {dim} = {bad}" for bad in (0, -1) for fn in ("hg_prepare", "ddim_compose", "ddim_compose_tokw", "ddim_noise")
       for dim in ("batch", "nfe", "tokens", "f")]
    + [f"{fn} {dim} = {bad}" for bad in (0, -1) for fn in ("vpred_loss", "vspace_loss", "vloss_grad") for dim in ("batch", "tokens", "f")])


@pytest.mark.parametrize("case", REFUSALS)
def test_refusal(capi, case):
    """the entry point returns the documented status through capi.check and writes nothing (every float buffer keeps its NaN fill, also
    after a synchronize: nothing was launched); a valid call afterwards succeeds.  The buffers are large enough for every shape asked."""
    cases = refusal_cases(capi)
    assert set(cases) == set(REFUSALS)
    code, call = cases[case]
    bufs = {k: nan_buf(1 << 19) for k in ("in0", "in1", "in2", "tab0", "tab1", "tab2", "tab3", "tab4", "tab5", "out0", "out1", "out2")}
    bufs["gen"] = torch.ones(1 << 19, device="cuda", dtype=torch.uint8)
    with pytest.raises(capi.DfotError) as e:
        capi.check(call(bufs))
    torch.cuda.synchronize()
    assert e.value.code == code, f"{case}: {e.value}"
    for k, t in bufs.items():
        if k != "gen":
            assert torch.isnan(t).all(), f"{case}: buffer {k} was written"
    x = torch.arange(16, device="cuda", dtype=torch.float32).view(1, 2, 8)
    one, zero, x_in = torch.ones(2, 2, device="cuda"), torch.zeros(2, 2, device="cuda"), nan_buf(2, 2, 8)
    capi.check(capi.lib.dfot_hg_prepare(P(x), None, P(one), P(zero), P(x_in), 1, 2, 2, 8, S()))
    assert torch.equal(x_in, x.repeat_interleave(2, 0))
