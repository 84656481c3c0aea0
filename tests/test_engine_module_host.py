"""Host: the base of the four backbone modules (dfot_amd.engine_module.EngineModule) against a stub engine -- an object with the entry
points of an engine family over a Python list, no library call.  Pure CPU: the device check of sync_weights is answered "yes" for the
host tensors (torch.Tensor.is_cuda patched), the stream is NULL and nothing dereferences a pointer."""
import ctypes as C
import gc

import pytest
import torch
from torch import nn

import dfot_amd
from dfot_amd import backbone, capi, engine_module as em

# in the order a module tree lists its state dict: a module's own tensors, then its children in the order they first appear
LAYOUT = [("top", (1, 4, 2)), ("enc.proj.weight", (4, 3)), ("enc.proj.bias", (4,)), ("enc.norm.weight", (4,)), ("freqs.table", (6,)),
          ("out.0.weight", (2, 4, 1, 1))]


class StubEngine:
    """create / destroy / num_params / param_name / param_shape / load_weight / finalize / reserve / set_option over a list"""

    def __init__(self, layout=LAYOUT):
        self.layout, self.log, self.live, self.created, self.max_batch = list(layout), [], set(), 0, 0

    def create(self, cfg, out):
        self.created += 1
        self.live.add(self.created)
        out._obj.value = self.created
        self.log.append("create")
        return capi.OK

    def destroy(self, h):
        assert h.value in self.live, "destroy of a handle that is not live"
        self.live.remove(h.value)
        self.log.append("destroy")
        return capi.OK

    def num_params(self, h):
        return len(self.layout)

    def param_name(self, h, i):
        return self.layout[i][0].encode()

    def param_shape(self, h, i, shape, ndim):
        ndim._obj.value = len(self.layout[i][1])
        for k, v in enumerate(self.layout[i][1]):
            shape[k] = v
        return capi.OK

    def load_weight(self, h, name, data, shape, ndim, stream):
        assert h.value in self.live
        self.log.append(("load", name.decode(), tuple(shape[k] for k in range(ndim))))
        return capi.OK

    def finalize(self, h, stream):
        self.log.append("finalize")
        return capi.OK

    def reserve(self, h, batch):
        assert h.value in self.live
        self.log.append(("reserve", batch))
        self.max_batch = max(self.max_batch, batch)
        return capi.OK

    def set_option(self, h, key, value):
        self.log.append(("option", key.decode(), value))
        return capi.OK


class Stubbed(em.EngineModule):
    _engine = None  # the instance's stub, instead of the library binding

    def __init__(self, engine, layout=None):
        super().__init__()
        self._engine = engine
        self._ccfg = C.c_int(0)
        self.reserves_seen = []
        self._build_tree(layout)

    def _new_tensor(self, name, shape):
        if name == "freqs.table":
            return torch.full(shape, 2.0)                                            # a persistent buffer
        if name == "top":
            return nn.Parameter(torch.ones(shape), requires_grad=False)              # a frozen parameter
        return super()._new_tensor(name, shape)

    def _after_reserve(self):
        self.reserves_seen.append(self._reserved)


@pytest.fixture
def on_device(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)
    monkeypatch.setattr(capi, "stream_ptr", lambda: C.c_void_p(0))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)


def loads(engine):
    return [e[1] for e in engine.log if isinstance(e, tuple) and e[0] == "load"]


def test_tree_state_dict_order_and_register_hook():
    eng = StubEngine()
    m = Stubbed(eng)
    assert eng.log == ["create"] and m._handle.value == 1                           # eager: the handle exists after construction
    assert m._names == [n for n, _ in LAYOUT] == list(m.state_dict())               # engine order == state_dict order, buffer included
    assert [tuple(t.shape) for t in m.state_dict().values()] == [s for _, s in LAYOUT]
    assert type(m.enc) is type(m.enc.proj) is type(m.out) is em._Node and isinstance(m.enc.proj.weight, nn.Parameter)
    assert m.out._modules["0"].weight.shape == (2, 4, 1, 1)
    assert [n for n, _ in m.named_buffers()] == ["freqs.table"] and torch.equal(m.freqs.table, torch.full((6,), 2.0))
    assert not m.top.requires_grad and torch.equal(m.top, torch.ones(1, 4, 2))
    assert all(p.requires_grad and not p.any() for n, p in m.named_parameters() if n != "top")
    assert list(m._tensors()) == [n for n, _ in LAYOUT if n != "freqs.table"]        # parameters alone ...
    assert set(m._engine_tensors()) == set(m._names)                                # ... the engine loads the buffer too
    assert backbone._Node is em._Node and backbone._get is em._get                  # still importable from backbone
    assert em._get({"a": 1}, "a") == 1 and em._get(object(), "a", 5) == 5


def test_the_four_backbones_derive_from_the_base():
    for cls in (dfot_amd.UViT3DPose, dfot_amd.UViT3D):
        assert cls.__bases__ == (backbone.UViTModule,) and cls._family == "uvit"
    assert backbone.UViTModule.__bases__ == dfot_amd.DiT3D.__bases__ == dfot_amd.DiT1D.__bases__ == (em.EngineModule,)
    assert not issubclass(dfot_amd.UViT3D, dfot_amd.UViT3DPose)
    creates = {c: c._create for c in (dfot_amd.UViT3DPose, dfot_amd.UViT3D, dfot_amd.DiT3D, dfot_amd.DifferenceDiT3D, dfot_amd.DiT1D)}
    assert list(creates.values()) == ["dfot_uvit_create", "dfot_uvit3d_create", "dfot_dit_create_f", "dfot_dit_create_f", "dfot_dit1d_create"]
    for cls in creates:                                                             # the plumbing exists once
        for name in ("_ensure_handle", "_build_tree", "_signature", "sync_weights", "_bump_generation", "__del__"):
            assert getattr(cls, name) is getattr(em.EngineModule, name), (cls, name)
        assert cls is dfot_amd.DiT3D or cls is dfot_amd.DifferenceDiT3D or cls.reserve is em.EngineModule.reserve
    b = em.engine_binding("dit1d", "dfot_dit1d_create")
    assert b is em.engine_binding("dit1d", "dfot_dit1d_create") and b.set_option is None
    assert b.create is not None and b.load_weight is not None
    assert em.engine_binding("uvit", "dfot_uvit3d_create").set_option is not None


def test_deferred_handle(on_device):
    eng = StubEngine()
    m = Stubbed(eng, LAYOUT)
    assert eng.log == [] and not m._handle.value and list(m.state_dict()) == [n for n, _ in LAYOUT]
    m.sync_weights()
    assert eng.log[0] == "create" and m._handle.value == 1 and loads(eng) == m._names and eng.log[-1] == "finalize"
    m.reserve(2)
    assert eng.log.count("create") == 1
    r = Stubbed(StubEngine(), LAYOUT)                                               # a reserve before any sync creates it too
    r.reserve(1)
    assert r._engine.log == ["create", ("reserve", 1)]


def test_deferred_handle_refuses_another_layout(on_device):
    for other in (LAYOUT[:-1], LAYOUT[1:] + LAYOUT[:1], [(n, s[::-1]) for n, s in LAYOUT]):
        eng = StubEngine(other)
        m = Stubbed(eng, LAYOUT)
        with pytest.raises(RuntimeError, match="^the engine's parameter list differs from the module's state-dict layout$"):
            m.sync_weights()
        assert eng.log == ["create", "destroy"] and not eng.live and not m._handle.value and m._synced is None


def test_host_resident_weights_are_refused_before_the_handle_exists():
    eng = StubEngine()
    m = Stubbed(eng, LAYOUT)
    with pytest.raises(RuntimeError, match=r"^parameter top is on cpu; move the module to the GPU first$"):
        m.sync_weights()
    assert eng.log == [] and m.reserve_generation == 0
    eager = Stubbed(StubEngine())
    with pytest.raises(RuntimeError, match=r"^parameter top is on cpu; move the module to the GPU first$"):
        eager.sync_weights()
    assert loads(eager._engine) == []                                               # nothing was loaded


def test_sync_skips_reruns_and_counts(on_device):
    eng = StubEngine()
    m = Stubbed(eng)
    assert m.reserve_generation == 0 and m._synced is None
    m.sync_weights()
    assert loads(eng) == m._names and m.reserve_generation == 1 and m._synced == m._signature()
    assert [e for e in eng.log if isinstance(e, tuple)][1] == ("load", "enc.proj.weight", (4, 3))
    n = len(eng.log)
    m.sync_weights()                                                                # unchanged signature: nothing happens
    assert len(eng.log) == n and m.reserve_generation == 1
    with torch.no_grad():
        m.enc.proj.bias.add_(1.0)                                                   # an in-place edit bumps _version
    m.sync_weights()
    assert loads(eng) == m._names * 2 and eng.log.count("finalize") == 2 and m.reserve_generation == 2
    with torch.no_grad():
        m.freqs.table.mul_(2.0)                                                     # a buffer counts too
    m.sync_weights()
    assert eng.log.count("finalize") == 3 and m.reserve_generation == 3
    m.sync_weights(force=True)
    assert loads(eng) == m._names * 4 and eng.log.count("finalize") == 4 and m.reserve_generation == 4
    m.load_state_dict({k: torch.zeros_like(v) for k, v in m.state_dict().items()})  # copy_ into every tensor
    m.sync_weights()
    assert eng.log.count("finalize") == 5 and m.reserve_generation == 5


def test_reserve_and_set_option_count_generations(on_device):
    eng = StubEngine()
    m = Stubbed(eng)
    m.reserve(2)
    assert eng.log[-1] == ("reserve", 2) and m._reserved == 2 and m.reserve_generation == 1 and m.reserves_seen == [2]
    n = len(eng.log)
    m.reserve(2)
    m.reserve(1)                                                                    # no growth: no call, no generation, no hook
    assert len(eng.log) == n and m._reserved == 2 and m.reserve_generation == 1 and m.reserves_seen == [2]
    m.reserve(5)
    assert eng.log[-1] == ("reserve", 5) and m.reserve_generation == 2 and m.reserves_seen == [2, 5]
    m.set_option("gemm_variant", 3)
    assert eng.log[-1] == ("option", "gemm_variant", 3) and m.reserve_generation == 3 and m.reserves_seen == [2, 5]


def test_a_failed_reserve_changes_nothing(on_device):
    eng = StubEngine()
    m = Stubbed(eng)
    eng.reserve = lambda h, batch: capi.ERR_SHAPE
    with pytest.raises(capi.DfotError) as e:
        m.reserve(3)
    assert e.value.code == capi.ERR_SHAPE and m._reserved == 0 and m.reserve_generation == 0 and m.reserves_seen == []


def test_del_destroys_once_and_tolerates_no_handle():
    eng = StubEngine()
    m = Stubbed(eng)
    m.__del__()
    assert eng.log == ["create", "destroy"] and not m._handle.value
    m.__del__()                                                                     # the handle is gone: nothing to destroy
    del m
    gc.collect()
    assert eng.log == ["create", "destroy"]
    lazy = StubEngine()
    Stubbed(lazy, LAYOUT).__del__()                                                 # never created
    assert lazy.log == []
    em.EngineModule.__del__(object.__new__(Stubbed))                                # a constructor that raised before the base ran
