"""The DiT family under continuous diffusion, the parts that need no GPU: the restatement against the reference fixture
(tools/make_golden_dit_cont.py), the Fourier features, configuration errors, state-dict order, operator registration."""
import re

import numpy as np
import pytest
import torch

import dit_cont_common as cc
from dit_cont_common import T, load, rel


def _small():
    from oracle import dit as odit
    return odit, odit.DiTConfig(**cc.SMALL), odit.DiffDiTConfig(**cc.DIFF_TINY)


def test_fourier_features_equal_the_reference_modules():
    """fp32, same two rounded operations for the argument: bit-equal to FourierEmbedding.forward on the same CPU"""
    g = load("dit_cont.npz")
    b = cc.fourier_buffers(0)
    feat = cc.fourier_features(T(g["levels"]), b[cc.FREQS], b[cc.PHASES])
    ref = T(g["feat"])
    assert feat.dtype == torch.float32 and tuple(feat.shape) == (2, 5, 256)
    assert float((feat - ref).abs().max()) <= 2.5e-7  # one fp32 ulp of sqrt(2): libm builds may differ in the cosine's last bit
    # the float64 cosine of the SAME fp32 argument agrees to the fp32 cosine's own error; an argument formed in one rounding would not
    f64 = cc.fourier_features(T(g["levels"]), b[cc.FREQS], b[cc.PHASES], torch.float64)
    assert float((f64 - ref.double()).abs().max()) < 5e-7
    lo, hi = cc.logsnr_extremes()
    lv = g["levels"]
    assert np.float32(lo) in lv and np.float32(hi) in lv and lo > 1.0 and hi < -2.0


def test_restatement_matches_the_reference_fixture_to_fp32_accuracy():
    g = load("dit_cont.npz")
    odit, small, oc = _small()
    ps = cc.with_buffers(odit.seeded_params(small, 2), 0)
    dps = cc.with_buffers(odit.diff_seeded_params(oc, 3), 1)
    assert cc.digest(ps) == str(g["digest"]) and cc.digest(dps) == str(g["digest_diff"])
    with torch.no_grad():
        out = cc.forward_dit(ps, small, T(g["x"]), T(g["levels"]))
        dout = cc.forward_diff(dps, oc, T(g["xd"]), T(g["levels_d"]))
    assert rel(out, T(g["out"])) < 1e-5
    assert rel(dout, T(g["diff_out"])) < 1e-5
    # the swap of the oracle's embedding is undone afterwards
    assert odit.noise_level_embedding.__module__ == "oracle.dit"


def test_condition_path_composition_equals_the_direct_restatement():
    """forward_fac / forward_facmat hand the Fourier features through the restatements' condition MLP; on the embedding alone that is
    exactly fourier_embedding"""
    import dit_fac_common as fac
    keys = fac.key_shapes(4.0)
    params = cc.seeded_params(keys, 3)
    assert list(params)[:2] == [cc.FREQS, cc.PHASES] and list(params)[2:] == [n for n, _ in keys]
    lv = torch.tensor([[0.3, -1.7, 2.9]])
    p, feat = cc._through_condition_path(params, lv, torch.float64)
    from dit_cond_common import action_embedding_fp64
    e = action_embedding_fp64(p, feat)
    assert rel(e, cc.fourier_embedding(params, lv, torch.float64)) < 1e-12
    assert float(p[f"{cc.EMB}.linear_2.weight"].abs().max()) == 0.0


def test_state_dict_order_of_the_reference_lists_the_buffers_first():
    g = load("dit_cont.npz")
    odit, small, oc = _small()
    for key, plain in (("names", list(odit.param_shapes(small))), ("diff_names", list(odit.diff_param_shapes(oc)))):
        names = [str(n) for n in g[key]]
        assert names[:2] == [cc.FREQS, cc.PHASES] and names[2:] == plain
    act = [str(n) for n in g["act_names"]]
    assert act[:2] == [cc.FREQS, cc.PHASES] and act[2].startswith(cc.EMB) and act[6].startswith("external_cond_embedding.embedding.linear_1")
    # buffers have no gradient in the reference's training step
    for tag in ("dit", "diff"):
        gn = [str(n) for n in g[f"train_{tag}_names"]]
        assert cc.FREQS not in gn and cc.PHASES not in gn and len(gn) == len(g[f"train_{tag}_norms"])


def test_checkpoint_with_the_fourier_buffers_loads_strictly():
    from dfot_amd.checkpoint import load_reference_checkpoint, reference_parameter_order
    g = load("dit_cont.npz")
    names = [str(n) for n in g["names"]]
    module = torch.nn.Module()
    gen = torch.Generator().manual_seed(0)
    state = {}
    for i, n in enumerate(names):
        t = torch.randn(256 if n in (cc.FREQS, cc.PHASES) else 3, generator=gen)
        state[n] = t
        if n in (cc.FREQS, cc.PHASES):
            module.register_buffer(f"p{i}", torch.zeros_like(t))
        else:
            module.register_parameter(f"p{i}", torch.nn.Parameter(torch.zeros_like(t)))
    module.state_dict = lambda: {n: getattr(module, f"p{i}").detach() for i, n in enumerate(names)}

    def load_sd(sd, strict=True):
        assert list(sd) == names
        for i, n in enumerate(names):
            getattr(module, f"p{i}").data.copy_(sd[n])
    module.load_state_dict = load_sd
    load_reference_checkpoint(module, {"state_dict": {"diffusion_model.model." + n: t for n, t in state.items()}})
    for n, t in module.state_dict().items():
        assert torch.equal(t, state[n]), n
    without = {"diffusion_model.model." + n: t for n, t in state.items() if n != cc.PHASES}
    with pytest.raises(ValueError, match="The following keys are not found in the checkpoint: .*timesteps.phases"):
        load_reference_checkpoint(module, {"state_dict": without})
    assert len(reference_parameter_order(module)) == len(names) - 2  # EMA lists follow named_parameters(): no buffers


def test_config_field_and_mirror():
    """dfot_dit_config keeps its size and last field; dfot_dit_config_f = that struct + a trailing int32_t fourier_noise, mirrored by a
    ctypes subclass whose base fields alias the base's"""
    import ctypes
    from dfot_amd import capi
    assert capi.DiTConfig._fields_[-1][0] == "use_temporal_rope"
    assert capi.DiTConfigF._fields_ == [("fourier_noise", ctypes.c_int32)] and issubclass(capi.DiTConfigF, capi.DiTConfig)
    assert capi.DiTConfigF.fourier_noise.offset == ctypes.sizeof(capi.DiTConfig) == ctypes.sizeof(capi.DiTConfigF) - 4
    c = capi.DiTConfigF()
    c.hidden_size, c.use_temporal_rope, c.fourier_noise = 128, 1, 1
    raw = (ctypes.c_int32 * (ctypes.sizeof(c) // 4)).from_buffer_copy(c)
    assert raw[0] == 128 and raw[-2] == 1 and raw[-1] == 1 and capi.DiTConfigF().fourier_noise == 0
    hdr = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "dfot_hip.h")).read()
    assert re.search(r"typedef struct \{\s*dfot_dit_config base;\s*int32_t fourier_noise;\s*\} dfot_dit_config_f;", hdr)
    assert "fourier_noise" not in hdr[hdr.index("int32_t use_temporal_rope;"):hdr.index("} dfot_dit_config;")]
    for name in ("dfot_dit_create_f", "dfot_dit_train_create_f", "dfot_dit_forward_f", "dfot_dit_train_forward_f", "dfot_dit_train_load_buffer"):
        assert name in capi.SIGNATURES and re.search(r"\b" + name + r"\(", hdr)
    assert capi.SIGNATURES["dfot_dit_forward_f"] == capi.SIGNATURES["dfot_dit_forward_cond"]


def test_trainer_refuses_mismatched_diffusion_and_embedding():
    import dfot_amd
    from dfot_amd import DiffusionConfig
    with pytest.raises(ValueError, match="use_fourier_noise_embedding=False with DiffusionConfig\\(is_continuous=True\\)"):
        dfot_amd.DiT3DTrainer(cc.dit_cfg(), x_shape=(4, 16, 8), max_tokens=5, diffusion=DiffusionConfig(is_continuous=True))
    with pytest.raises(ValueError, match="use_fourier_noise_embedding=True with DiffusionConfig\\(is_continuous=False\\)"):
        dfot_amd.DiT3DTrainer(cc.cont(cc.dit_cfg()), x_shape=(4, 16, 8), max_tokens=5)
    with pytest.raises(ValueError, match="use_fourier_noise_embedding=True with DiffusionConfig\\(is_continuous=False\\)"):
        dfot_amd.DiT3DTrainer(cc.cont(cc.diff_cfg()), x_shape=(4, 16, 8), max_tokens=5,
                              diffusion=DiffusionConfig(beta_schedule="cosine", is_continuous=False))


def test_level_dtype_rules():
    """float levels on a discrete model and integer levels on a Fourier model are TypeErrors (checked before anything touches the GPU)"""
    from dfot_amd.dit_backbone import DiT3D
    m = DiT3D.__new__(DiT3D)
    m.use_fourier_noise_embedding = True
    m._check_level_dtype(torch.zeros(2, 5))
    with pytest.raises(TypeError, match="use_fourier_noise_embedding: it takes floating noise levels"):
        m._check_level_dtype(torch.zeros(2, 5, dtype=torch.int32))
    m.use_fourier_noise_embedding = False
    m._check_level_dtype(torch.zeros(2, 5, dtype=torch.long))
    with pytest.raises(TypeError, match="DiT3D takes integer noise levels"):
        m._check_level_dtype(torch.zeros(2, 5))


def test_float_level_operators_are_registered_with_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import dfot_amd  # noqa: F401
    for name in ("dit3d_forward_f", "dit3d_forward_f_train"):
        assert hasattr(torch.ops.dfot, name), name
    with FakeTensorMode():
        z, k = torch.empty(3, 5, 16, 16, 16), torch.empty(3, 5)
        assert torch.ops.dfot.dit3d_forward_f(z, k, None, None, 0).shape == z.shape
        assert torch.ops.dfot.dit3d_forward_f(z, k, torch.empty(3, 5, 3), torch.empty(3, dtype=torch.uint8), 0).shape == z.shape
        assert torch.ops.dfot.dit3d_forward_f_train(z, k, None, None, [torch.empty(4)], 0).shape == z.shape
        assert torch.ops.dfot.dit3d_forward(z, torch.empty(3, 5, dtype=torch.long), 0).shape == z.shape
