"""The pose / FiLM cache of UViT3DPose.forward is keyed by identity first and by content second (dfot_op_equal_bits).

Model: the reduced-depth 64 x 64 RE10K-width backbone of tests/test_gpu_backbone.py (one block per level), batch 2; noise levels, poses and
the per-video mask are those of tests/golden/backbone_tiny.npz (whose 16 x 16 frames this engine does not take: x is seeded here and the
poses are ray-encoded at 64 x 64).  Every bar is exact: integer counters (the engine's own ``cond_builds`` next to the module's
``cond_cache_stats``) and ``torch.equal`` between outputs."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    import dfot_amd
    from oracle import uvit as ouvit
    ocfg = ouvit.UViTConfig(resolution=64, num_updown_blocks=(1, 1, 1), num_mid_blocks=1)
    params = ouvit.seeded_params(ocfg, 3)
    cfg = dict(channels=list(ocfg.channels), emb_channels=ocfg.emb_channels, patch_size=2, block_types=list(ocfg.block_types),
               num_updown_blocks=[1, 1, 1], num_mid_blocks=1, num_heads=ocfg.num_heads, pos_emb_type="rope",
               use_fourier_noise_embedding=True, conditioning=dict(dim=180))

    def make(state=params):
        model = dfot_amd.UViT3DPose(cfg, x_shape=(3, 64, 64), max_tokens=8).cuda()
        model.load_state_dict(state, strict=True)
        return model

    g = np.load(os.path.join(GOLDEN, "backbone_tiny.npz"))
    k, poses, mask = (torch.from_numpy(g[n]).cuda() for n in ("k", "poses", "mask"))
    assert tuple(k.shape) == (2, 8) and mask.tolist() == [True, False]
    x = torch.randn(2, 8, 3, 64, 64, generator=torch.Generator().manual_seed(0)).cuda()
    with torch.no_grad():
        cond = torch.ops.dfot.ray_encoding(poses, 64)
        base = make()(x, k, cond, mask)       # computed once, shared, never written
    return dict(make=make, params=params, x=x, k=k, cond=cond, mask=mask, base=base)


def counters(model):
    s = model.cond_cache_stats
    return int(model.query("cond_builds")), s["builds"], s["identity_hits"], s["content_hits"]


def test_equal_content_in_fresh_tensors_hits_the_cache(tiny):
    """what the reference's sampler does: a new tensor with the same values on every step"""
    model = tiny["make"]()
    x, k, cond, mask = (tiny[n] for n in ("x", "k", "cond", "mask"))
    with torch.no_grad():
        outs = [model(x, k, cond.clone(), mask.clone()) for _ in range(3)]
    assert int(model.query("cond_builds")) == 1
    assert model.cond_cache_stats == {"builds": 1, "identity_hits": 0, "content_hits": 2}
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(outs[0], tiny["base"])             # one call on the original tensors
    # the hit re-keyed to the tensors of the last call and dropped the older ones
    assert model._cond_refs[0].data_ptr() != cond.data_ptr() and model._cond_key[0] == model._cond_refs[0].data_ptr()


def change(name):
    def first(c, m):
        c.view(-1)[0] += 1.0
    def last(c, m):
        c.view(-1)[-1] += 1.0
    def frame(c, m):
        c[1, 1] += 0.5
    def mask(c, m):
        m[1] = True
    return dict(first=first, last=last, frame=frame, mask=mask)[name]


@pytest.mark.parametrize("what", ["first", "last", "frame", "mask"])
def test_any_changed_bit_is_a_miss(tiny, what):
    """one element at the very first / very last position, frame 1 of video 1 only, or the mask alone: the cache is rebuilt and the output is
    that of a model that never saw the old conditioning"""
    model = tiny["make"]()
    x, k, cond, mask = (tiny[n] for n in ("x", "k", "cond", "mask"))
    with torch.no_grad():
        assert torch.equal(model(x, k, cond, mask), tiny["base"])
        assert counters(model) == (1, 1, 0, 0)
        c2, m2 = cond.clone(), mask.clone()
        change(what)(c2, m2)
        got = model(x, k, c2, m2)
        assert counters(model) == (2, 2, 0, 0)
        assert torch.equal(got, tiny["make"]()(x, k, c2, m2))
        if what in ("frame", "mask"):                     # video 1 is unmasked: its conditioning reaches the output
            assert not torch.equal(got, tiny["base"])
        # ... and the new pair is the key now: equal content hits, the old content misses
        assert torch.equal(model(x, k, c2.clone(), m2.clone()), got)
        assert counters(model) == (2, 2, 0, 1)
        assert torch.equal(model(x, k, cond.clone(), mask.clone()), tiny["base"])
        assert counters(model) == (3, 3, 0, 1)


def test_in_place_write_to_the_kept_tensor_makes_it_stale(tiny):
    model = tiny["make"]()
    x, k, mask = (tiny[n] for n in ("x", "k", "mask"))
    c = tiny["cond"].clone()
    with torch.no_grad():
        model(x, k, c, mask)
        assert counters(model) == (1, 1, 0, 0)
        c.add_(1)                                         # same object, new version: identity misses, and the kept bits are gone
        got = model(x, k, c, mask)
        assert counters(model) == (2, 2, 0, 0)
        assert torch.equal(got, tiny["make"]()(x, k, c, mask))
        # the kept tensor is written again, WITHOUT a forward in between: a clone of its old values now meets a stale kept tensor
        old = c.clone()
        c.add_(1)
        got = model(x, k, old, mask)
        assert counters(model) == (3, 3, 0, 0)
        assert torch.equal(got, tiny["make"]()(x, k, old, mask))
        # the same through the mask: a new mask object with equal bits is a content hit (the kept cond is compared with itself) ...
        m = mask.clone()
        assert torch.equal(model(x, k, old, m), got)
        assert counters(model) == (3, 3, 0, 1)
        m.logical_not_()
        m.logical_not_()                                  # ... and a kept mask with its old bits but a new version is stale
        assert torch.equal(model(x, k, old.clone(), m.clone()), got)
        assert counters(model) == (4, 4, 0, 1)


def test_identity_path_is_unchanged(tiny):
    model = tiny["make"]()
    x, k, cond, mask = (tiny[n] for n in ("x", "k", "cond", "mask"))
    with torch.no_grad():
        outs = [model(x, k, cond, mask) for _ in range(3)]
    assert counters(model) == (1, 1, 2, 0)
    assert all(torch.equal(o, tiny["base"]) for o in outs)
    assert model._cond_flag is None                       # no compare ever ran


def test_invalidation_still_forces_a_build(tiny):
    model = tiny["make"]()
    x, k, cond, mask = (tiny[n] for n in ("x", "k", "cond", "mask"))
    with torch.no_grad():
        model(x, k, cond, mask)
        model._cond_key = None                            # explicit invalidation (tests/test_gpu_backbone.py relies on it)
        assert torch.equal(model(x, k, cond.clone(), mask), tiny["base"])
        assert counters(model) == (2, 2, 0, 0)
        model._cond_key = None
        assert torch.equal(model(x, k, cond, mask), tiny["base"])
        assert counters(model) == (3, 3, 0, 0)
        # new weights: the FiLM projections are stale even for identical conditioning, by identity and by content
        g = torch.Generator().manual_seed(5)
        moved = {n: t + 0.01 * torch.randn(t.shape, generator=g) for n, t in tiny["params"].items()}
        model.load_state_dict(moved, strict=True)
        got = model(x, k, cond, mask)
        assert counters(model) == (4, 4, 0, 0)
        assert torch.equal(got, tiny["make"](moved)(x, k, cond, mask)) and not torch.equal(got, tiny["base"])
        model.load_state_dict(tiny["params"], strict=True)
        assert torch.equal(model(x, k, cond.clone(), mask), tiny["base"])
        assert counters(model) == (5, 5, 0, 0)
        # a larger reservation re-allocates the workspace the caches live in
        model(x, k, cond.clone(), mask)
        assert counters(model) == (5, 5, 0, 1)
        model.reserve(3)
        assert torch.equal(model(x, k, cond.clone(), mask), tiny["base"])
        assert counters(model) == (6, 6, 0, 1)


@pytest.mark.parametrize("form", ["fp64", "strided"])
def test_conditioning_that_is_not_plain_fp32_memory_is_a_miss(tiny, form):
    """equal values, but not comparable as raw memory: rebuilt (from the converted copy, as before), same result"""
    model = tiny["make"]()
    x, k, cond, mask = (tiny[n] for n in ("x", "k", "cond", "mask"))
    odd = cond.double() if form == "fp64" else cond.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert torch.equal(odd.float(), cond) and (odd.dtype != torch.float32 or not odd.is_contiguous())
    with torch.no_grad():
        model(x, k, cond, mask)
        assert torch.equal(model(x, k, odd, mask), tiny["base"])
        assert counters(model) == (2, 2, 0, 0)
        assert torch.equal(model(x, k, cond.clone(), mask), tiny["base"])   # the kept tensor is the odd one: not comparable either
        assert counters(model) == (3, 3, 0, 0)
        assert torch.equal(model(x, k, odd, mask), tiny["base"])
        assert counters(model) == (4, 4, 0, 0)
        assert torch.equal(model(x, k, odd, mask), tiny["base"])            # identity still works for it
        assert counters(model) == (4, 4, 1, 0)


def test_under_graph_capture_only_identity_counts(tiny):
    """a host read of the flag is illegal while the stream captures: a cloned cond is a miss there, the build is captured with the forward
    (one stream, no parallel branches), and the replay reproduces the eager output"""
    model = tiny["make"]()
    x, k, cond, mask = (tiny[n] for n in ("x", "k", "cond", "mask"))
    with torch.no_grad():
        eager = model(x, k, cond, mask)                   # also syncs the weights and reserves the workspace outside the capture
        assert counters(model) == (1, 1, 0, 0)
        c2 = cond.clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            out = model(x, k, c2, mask)
        assert counters(model) == (2, 2, 0, 0)            # no compare was launched: a miss, recorded as a build
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(eager, tiny["base"])
        # after the capture the content path is back
        assert torch.equal(model(x, k, cond.clone(), mask), eager)
        assert counters(model) == (2, 2, 0, 1)
