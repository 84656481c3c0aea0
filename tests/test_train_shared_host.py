"""Host checks (no GPU) of what every trainer shares: the flat optimizer state (flat_optim.FlatAdamW on the CPU: layout, views, the
accumulated mean, the state-dict round trips and refusals), the host tables of the denoising loss (diffusion.denoising_tables, both
diffusions, against the formulas written out here) and that the two trainer families end in the same FlatAdamW functions."""
import numpy as np
import pytest
import torch

B, T, F = 2, 3, 8
LAYOUT = {"a.weight": (0, (3, 5)), "a.bias": (16, (5,)), "scale": (24, ())}  # offsets padded to four floats, a scalar last
NUMEL = 28
HYPER = dict(lr=3e-4, betas=(0.8, 0.95), eps=1e-7, weight_decay=0.05)


def _opt():
    from dfot_amd.flat_optim import FlatAdamW
    return FlatAdamW(LAYOUT, NUMEL, device="cpu")


def test_views_have_the_layouts_shapes_and_alias_the_buffers():
    opt = _opt()
    for buf in (opt.params, opt.grads, opt.exp_avg, opt.exp_avg_sq):
        assert buf.shape == (NUMEL,) and buf.dtype == torch.float32 and buf.device.type == "cpu"
    for i, (name, (off, shape)) in enumerate(LAYOUT.items()):
        assert opt.view(name).shape == shape and opt.view(name, opt.grads).shape == shape
        opt.view(name).fill_(i + 1.0)
        opt.view(name, opt.grads).fill_(-(i + 1.0))
        n = int(np.prod(shape))
        assert (opt.params[off: off + n] == i + 1.0).all() and (opt.grads[off: off + n] == -(i + 1.0)).all()
    assert float(opt.params.sum()) == 15 * 1 + 5 * 2 + 3 and float(opt.exp_avg.abs().sum()) == 0  # the padding stays untouched


def test_two_accumulated_gradients_give_their_average():
    opt = _opt()
    g = torch.Generator().manual_seed(0)
    g1, g2 = torch.randn(NUMEL, generator=g), torch.randn(NUMEL, generator=g)
    assert not opt.take_accumulated()
    opt.grads.copy_(g1)
    opt.accumulate(True)
    opt.grads.copy_(g2)
    opt.accumulate(False)
    assert opt._acc_n == 2 and not opt._acc_reduced  # one micro-batch was not reduced: the mean still needs its exchange
    assert opt.take_accumulated()
    assert torch.equal(opt.grads, (g1 + g2) * 0.5) and opt._acc_n == 0 and float(opt._acc.abs().sum()) == 0
    opt.accumulate(True)
    assert opt._acc_reduced  # a new round starts from its own micro-batches


def _stepped():
    opt = _opt()
    g = torch.Generator().manual_seed(1)
    opt.exp_avg.copy_(torch.randn(NUMEL, generator=g))
    opt.exp_avg_sq.copy_(torch.rand(NUMEL, generator=g))
    opt.step_count = 7
    return opt


def test_optimizer_state_dict_is_torch_adamws_and_round_trips():
    opt = _stepped()
    sd = opt.optimizer_state_dict(HYPER)
    assert len(sd["state"]) == len(LAYOUT) and sd["param_groups"][0]["betas"] == (0.8, 0.95)
    torch.optim.AdamW([torch.nn.Parameter(torch.zeros(s)) for _, s in LAYOUT.values()]).load_state_dict(sd)  # torch accepts it
    other = _opt()
    assert other.optimizer_state_dict(HYPER)["state"] == {}  # before any step, as a fresh torch optimizer
    assert other.load_optimizer_state_dict(sd) == HYPER and other.step_count == 7
    for name in LAYOUT:
        assert torch.equal(other.view(name, other.exp_avg), opt.view(name, opt.exp_avg))
        assert torch.equal(other.view(name, other.exp_avg_sq), opt.view(name, opt.exp_avg_sq))
    assert other.load_optimizer_state_dict({"state": {}}) is None and other.step_count == 0


def test_differing_per_parameter_steps_are_refused():
    sd = _stepped().optimizer_state_dict(HYPER)
    sd["state"][1]["step"] = torch.tensor(8.0)
    with pytest.raises(ValueError, match="per-parameter step counts differ: the flat optimizer keeps one"):
        _opt().load_optimizer_state_dict(sd)


def test_ema_state_dict_round_trip_and_refusals():
    opt = _opt()
    with pytest.raises(RuntimeError, match="EMA is not enabled"):
        opt.ema_state_dict()
    with pytest.raises(RuntimeError, match="EMA is not enabled"):
        opt.load_ema_state_dict({})
    opt.params.copy_(torch.arange(NUMEL, dtype=torch.float32))
    opt.enable_ema(0.9)
    assert opt.ema_decay == 0.9 and torch.equal(opt.ema, opt.params) and opt.ema.data_ptr() != opt.params.data_ptr()
    sd = opt.ema_state_dict()
    assert list(sd) == list(LAYOUT) and all(sd[n].shape == LAYOUT[n][1] for n in LAYOUT)
    other = _opt()
    other.enable_ema(0.9)
    other.load_ema_state_dict({n: t.double() for n, t in sd.items()})
    assert all(torch.equal(other.view(n, other.ema), sd[n]) for n in LAYOUT) and other.ema.dtype == torch.float32
    for bad in ({n: sd[n] for n in list(LAYOUT)[:-1]}, {**sd, "extra": torch.zeros(1)}):
        with pytest.raises(ValueError, match="does not match the structure of the EMA model"):
            other.load_ema_state_dict(bad)


# ---------------------------------------------------------------------------------------------------------------- the loss tables
def _masks():
    m = torch.ones(B, T)
    m[1, 2] = 0
    return m


def test_discrete_tables_are_the_schedules():
    from dfot_amd.diffusion import ALPHA, COEF, LEVEL, SIGMA, WEIGHT, DiffusionConfig, Schedule, denoising_tables
    sch = Schedule(DiffusionConfig(beta_schedule="cosine", is_continuous=False, timesteps=1000))
    k = torch.tensor([[0, 417, 999], [3, 3, 250]])
    lw = dict(strategy="fused_min_snr", cum_snr_decay=0.96)
    tab = denoising_tables(sch, k, F, _masks(), True, lw)
    assert tab.shape == (5, B, T) and tab.dtype == torch.float32 and tab.device.type == "cpu"
    kk = k.numpy()
    w = sch.loss_weights(kk, **lw)
    assert np.array_equal(tab[ALPHA].numpy(), sch.sqrt_alphas_cumprod[kk]) and np.array_equal(tab[SIGMA].numpy(), sch.sqrt_one_minus_alphas_cumprod[kk])
    assert np.array_equal(tab[WEIGHT].numpy(), w) and np.array_equal(tab[LEVEL].numpy(), kk.astype(np.float32))
    assert np.array_equal(tab[COEF].numpy(), (2.0 * w * _masks().numpy() / (F * B * T)).astype(np.float32))
    assert float(tab[COEF][1, 2]) == 0 and int((tab[COEF] != 0).sum()) == B * T - 1
    plain = denoising_tables(sch, k, F)  # no gradient wanted: no coefficient row; the default weighting
    assert plain.shape == (4, B, T) and np.array_equal(plain[WEIGHT].numpy(), sch.loss_weights(kk)) and torch.equal(plain[:WEIGHT], tab[:WEIGHT])
    ones = denoising_tables(sch, k, F, None, True, lw)  # no masks: every token counts
    assert np.array_equal(ones[COEF].numpy(), (2.0 * w / (F * B * T)).astype(np.float32))


def test_continuous_tables_are_training_logsnr_tables():
    from dfot_amd.diffusion import ALPHA, COEF, LEVEL, SIGMA, WEIGHT, DiffusionConfig, denoising_tables
    dcfg = DiffusionConfig(precond_scale=0.25, training_schedule_shift=0.5, loss_sigmoid_bias=-2.0)
    t = torch.tensor([[0.0, 0.31, 1.0], [0.5, 0.5, 0.07]])
    tab = denoising_tables(dcfg, t, F, _masks(), True)
    assert tab.shape == (5, B, T) and tab.dtype == torch.float32 and tab.device.type == "cpu"
    logsnr, alpha, sigma, weight = dcfg.training_logsnr_tables(t)
    assert torch.equal(tab[ALPHA], alpha) and torch.equal(tab[SIGMA], sigma) and torch.equal(tab[WEIGHT], weight)
    assert torch.equal(tab[LEVEL], 0.25 * logsnr)
    assert torch.equal(tab[COEF], 2.0 * weight * _masks() / (F * B * T))
    assert float(tab[COEF][1, 2]) == 0 and int((tab[COEF] != 0).sum()) == B * T - 1
    assert torch.equal(denoising_tables(dcfg, t, F), tab[:COEF])


# ---------------------------------------------------------------------------------------------------------------- one implementation
SHARED = {"view": "view", "accumulate": "accumulate", "enable_ema": "enable_ema", "ema_state_dict": "ema_state_dict",
          "load_ema_state_dict": "load_ema_state_dict", "optimizer_state_dict": "optimizer_state_dict",
          "load_optimizer_state_dict": "load_optimizer_state_dict", "grad_norm": "grad_norm", "optimizer_step": "step"}


def test_both_trainer_families_end_in_the_same_flat_adamw_functions():
    """every shared optimizer method of a DiT trainer and of a U-ViT trainer calls the FlatAdamW function of the table above on the trainer's
    `opt` and nothing else of it; all but optimizer_step (whose signature is the family's) are one function object for both families"""
    from dfot_amd import trainer, uvit_train
    from dfot_amd.flat_optim import FlatAdamW
    families = (trainer.DiT3DTrainer, uvit_train._UViTTrainerBase)
    for sub in (trainer.FacDiTTrainer, trainer.FacMatDiTTrainer, uvit_train.UViT3DTrainer, uvit_train.UViT3DPoseTrainer):
        assert all(getattr(sub, m) is getattr(fam, m) for fam in families if issubclass(sub, fam) for m in SHARED)
    called = []

    class Spy:
        def __getattr__(self, name):
            assert callable(FlatAdamW.__dict__[name]), name  # a function FlatAdamW itself defines

            def record(*a, **k):
                called.append(FlatAdamW.__dict__[name])
                return None
            return record
    args = {"view": ("n",), "enable_ema": (0.9,), "load_ema_state_dict": ({},), "load_optimizer_state_dict": ({},)}
    for method, target in SHARED.items():
        if method != "optimizer_step":
            assert getattr(families[0], method) is getattr(families[1], method), method
        for fam in families:
            tr = object.__new__(fam)
            tr.__dict__.update(opt=Spy(), lr=1e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.0, max_grad_norm=1.0, _hyper=HYPER, sync=lambda own_step: None)
            del called[:]
            getattr(tr, method)(*args.get(method, ()))
            assert called == [FlatAdamW.__dict__[target]], (fam.__name__, method)
