"""GPU: the registry contract of the dit and dit1d engines through the real C ABI (tests/test_gpu_uvit3d.py::test_abi_errors does it for
uvit): an unexpected key, a wrong shape and a null argument are refused in the engine's own wording; finalize on a fresh handle names the
first key of the state dict; a load_weight after a finalize takes the handle out of the finalized state until finalize runs again; a
reserve that does not grow leaves workspace_bytes alone.  All of these are error returns; nothing here faults.

DiT: the SMALL configuration of tests/dit_cond_common.py.  DiT1D: hidden 64, one block, L = 16, max_tokens = 8, 4 channels, 8 timesteps."""
import ctypes

import pytest
import torch

import dit_cond_common as dc

pytestmark = pytest.mark.gpu


def _dit():
    import dfot_amd
    make = lambda: dfot_amd.DiT3D(dc.dit_cfg(), x_shape=(4, 16, 8), max_tokens=5).cuda()  # noqa: E731
    return "dit", "", make, (2, 5, 4, 16, 8), 1000


def _dit1d():
    import dfot_amd
    cfg = dict(hidden_size=64, depth=1, num_heads=2, mlp_ratio=4.0)
    make = lambda: dfot_amd.DiT1D(cfg, x_shape=(4, 1, 16), max_tokens=8, timesteps=8).cuda()  # noqa: E731
    return "dit1d", "dit1d ", make, (2, 8, 4, 1, 16), 8


@pytest.mark.parametrize("engine", [_dit, _dit1d], ids=["dit", "dit1d"])
def test_registry_contract(engine):
    from dfot_amd import capi
    family, prefix, make, x_shape, timesteps = engine()
    L, P, S = capi.lib, capi.ptr, capi.stream_ptr
    load, finalize, reserve, forward, ws_bytes = (getattr(L, f"dfot_{family}_{op}") for op in
                                                  ("load_weight", "finalize", "reserve", "forward", "workspace_bytes"))

    def err():
        return L.dfot_last_error().decode()

    def dims(*shape):
        return (ctypes.c_int64 * len(shape))(*shape)
    model = make()
    model.init_random(1)
    tensors = model._engine_tensors()
    names = model._names
    assert names == list(model.state_dict())
    first = tensors[names[0]].detach().contiguous()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(x_shape, generator=g).cuda()
    k = torch.randint(0, timesteps, x_shape[:2], generator=g).to(torch.int32).cuda()

    def run(handle, batch=1):
        out = torch.zeros_like(x[:batch])
        return forward(handle, P(x[:batch].contiguous()), P(k[:batch].contiguous()), P(out), batch, x_shape[1], S()), out

    # a fresh handle: finalize names the first key in state-dict order, then the one key left out
    fresh = make()
    fresh._ensure_handle()
    assert fresh._names == names
    assert finalize(fresh._handle, S()) == capi.ERR_STATE and err() == f"{prefix}finalize: missing key '{names[0]}'"
    hole = names[len(names) // 2]
    for name in names:
        if name != hole:
            t = tensors[name].detach().contiguous()
            capi.check(load(fresh._handle, name.encode(), P(t), dims(*t.shape), t.ndim, S()))
    assert finalize(fresh._handle, S()) == capi.ERR_STATE and err() == f"{prefix}finalize: missing key '{hole}'"
    rc, _ = run(fresh._handle)
    assert rc == capi.ERR_STATE and "not finalized" in err()

    # refusals of load_weight, in the engine's wording; none of them touches the synced handle
    model.sync_weights()
    model.reserve(1)
    h = model._handle
    rc, want = run(h)
    assert rc == capi.OK
    assert load(h, b"blocks.0.nope.weight", P(first), dims(*first.shape), first.ndim, S()) == capi.ERR_NAME
    assert err() == f"{prefix}load_weight: unexpected key 'blocks.0.nope.weight'"
    extent = list(first.shape)
    extent[-1] += 1
    for wrong in (extent, list(first.shape) + [1], list(first.shape)[:-1]):
        assert load(h, names[0].encode(), P(first), dims(*wrong), len(wrong), S()) == capi.ERR_SHAPE
        assert err() == f"{prefix}load_weight: size mismatch for '{names[0]}'"
    assert load(h, names[0].encode(), None, dims(*first.shape), first.ndim, S()) == capi.ERR_ARG
    assert err() == f"{prefix}load_weight: null argument"
    assert load(h, None, P(first), dims(*first.shape), first.ndim, S()) == capi.ERR_ARG
    rc, out = run(h)
    assert rc == capi.OK and torch.equal(out, want)            # still finalized

    # a load after a finalize: not finalized until finalize runs again, then the same bits (the same weights were loaded)
    capi.check(load(h, names[0].encode(), P(first), dims(*first.shape), first.ndim, S()))
    rc, _ = run(h)
    assert rc == capi.ERR_STATE and err() == f"{prefix}forward: weights not finalized"
    capi.check(finalize(h, S()))
    rc, out = run(h)
    assert rc == capi.OK and torch.equal(out, want) and bool(out.isfinite().all()) and bool(out.any())

    # a reserve that does not grow leaves the workspace alone
    at1 = ws_bytes(h)
    assert at1 > 0
    capi.check(reserve(h, 1))
    assert ws_bytes(h) == at1
    model.reserve(2)
    at2 = ws_bytes(h)
    assert at2 > at1
    capi.check(reserve(h, 1))
    capi.check(reserve(h, 2))
    assert ws_bytes(h) == at2
    rc, out = run(h, 2)
    assert rc == capi.OK and bool(out.isfinite().all())
    torch.cuda.synchronize()
