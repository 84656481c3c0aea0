"""Shared helpers of tests/test_dit1d_host.py, tests/test_gpu_dit1d.py and tools/make_golden_dit1d.py (not a test module): the DiT1D
backbone (the reference's algorithms/dfot/backbones/dit1d/dit_model.py:358-530 at the stock dit1d.yaml).

  * key_shapes        the reference module's state-dict keys and shapes, in its registration order (pos_embed first)
  * seeded_params     weights drawn per key from a seed derived from the key's name and shape (the fixture stores a digest, not tensors);
                      the q and k rows of every qkv.weight carry a gain so that the attention is sharp enough for the mask to matter
  * forward_host      a torch restatement of DIT1D.forward in any float dtype, with the three wrong masks and the wrong residual base the
                      fixture's sensitivities are measured with
"""
import hashlib
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = "dit1d.npz"

# hidden 128, depth 2, C 4, L 32, max_tokens 8: N = 256 tokens = two 128-row query tiles, hence one key block never loaded, one loaded
# whole and two that straddle the block diagonal.  Cases: tag -> heads (head dim 32 and 64: both row strides of the q/k/v layout)
TINY = dict(hidden_size=128, depth=2, mlp_ratio=4, learn_sigma=False, merge_mode="share_norm", causal_attn_mode="video_temporal_causal",
            use_rotary_emb=False, qk_norm=False)
CASES = {"h4": 4, "h2": 2}
X_SHAPE, MAX_TOKENS, BATCH = (4, 1, 32), 8, 2
TIMESTEPS, FREQ_DIM = 1000, 256
FIXTURE_BAR = 2e-2   # forward vs a reference fixture, rel-L2 (tests/test_gpu_dit_fac.py FIXTURE_BAR)
SENS_FLOOR = 0.1     # 5 x the bar: what every recorded sensitivity must reach
QK_GAIN = 4.0        # the recipe's starting gain; tools/make_golden_dit1d.py raises it until the sensitivities reach SENS_FLOOR and records it
INPUT_SEED, TRACE_SEED, DRAW_SEED = 91, 92, 0
SENSITIVITIES = {"sens_nomask": dict(mask="none"), "sens_tokencausal": dict(mask="token"), "sens_transposed": dict(mask="transposed"),
                 "sens_residual": dict(residual="raw")}


def load(name=FIXTURE):
    return np.load(os.path.join(GOLDEN, name))


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def tensor_digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().numpy().tobytes())
    return h.hexdigest()


def digest(params):
    h = hashlib.sha256()
    for k in params:
        h.update(k.encode())
        h.update(params[k].contiguous().numpy().tobytes())
    return h.hexdigest()


def backbone_cfg(heads, **over):
    return {**TINY, "name": "dit1d", "num_heads": heads, **over}


def inputs():
    """x [2, 8, 4, 1, 32] and integer levels [2, 8] (both ends of the range included)"""
    g = torch.Generator().manual_seed(INPUT_SEED)
    x = torch.randn(BATCH, MAX_TOKENS, *X_SHAPE, generator=g)
    k = torch.randint(0, TIMESTEPS, (BATCH, MAX_TOKENS), generator=g)
    k[0, 0], k[1, 7] = 0, TIMESTEPS - 1
    return x, k


def trace_inputs():
    g = torch.Generator().manual_seed(TRACE_SEED)
    return torch.randn(BATCH, MAX_TOKENS, *X_SHAPE, generator=g)


def trace_draws(shapes):
    """the normal draws of the sampler trace: the reference draws them one after another from torch.Generator().manual_seed(DRAW_SEED)"""
    g = torch.Generator().manual_seed(DRAW_SEED)
    return [torch.randn(tuple(int(v) for v in s), generator=g) for s in shapes]


def key_shapes(heads=4, hidden=None, depth=None, channels=X_SHAPE[0], length=X_SHAPE[2], max_tokens=MAX_TOKENS, mlp_ratio=None):
    """[(state-dict key, shape)] in the order DIT1D.__init__ registers them (dit_model.py:429-456): pos_embed is assigned after x_embedder and
    t_embedder, but nn.Module lists a module's own parameters before its children's"""
    h = hidden or TINY["hidden_size"]
    depth = depth or TINY["depth"]
    mh = int(h * (mlp_ratio or TINY["mlp_ratio"]))
    out = [("pos_embed", (1, max_tokens * length, h))]

    def linear(name, o, i):
        out.extend([(f"{name}.weight", (o, i)), (f"{name}.bias", (o,))])
    linear("x_embedder", h, channels)
    linear("t_embedder.mlp.0", h, FREQ_DIM)
    linear("t_embedder.mlp.2", h, h)
    for i in range(depth):
        linear(f"blocks.{i}.attn.qkv", 3 * h, h)
        linear(f"blocks.{i}.attn.proj", h, h)
        linear(f"blocks.{i}.mlp.fc1", mh, h)
        linear(f"blocks.{i}.mlp.fc2", h, mh)
        linear(f"blocks.{i}.adaLN_modulation.1", 6 * h, h)
    linear("final_layer.1", channels, h)
    return out


def seeded_params(keys, qk_gain=QK_GAIN):
    """every tensor from its own generator, seeded by sha256(name, shape): matrices N(0, 1/fan_in) with the q and k rows of qkv.weight
    raised by qk_gain, biases N(0, 0.05^2), pos_embed N(0, 0.5^2) (NOT the sin-cos table: an engine that recomputed the table instead of
    loading the tensor would miss the fixture).  Nothing is zero: the reference's zero-init of the modulations and of the output layer
    would hide everything."""
    out = {}
    for name, shape in keys:
        seed = int.from_bytes(hashlib.sha256(f"{name}{tuple(shape)}".encode()).digest()[:7], "little")
        g = torch.Generator().manual_seed(seed)
        if name == "pos_embed":
            t = 0.5 * torch.randn(shape, generator=g)
        elif name.endswith(".bias"):
            t = 0.05 * torch.randn(shape, generator=g)
        else:
            t = torch.randn(shape, generator=g) / math.sqrt(shape[1])
            if name.endswith("attn.qkv.weight"):
                t[: 2 * shape[0] // 3] *= qk_gain
        out[name] = t.to(torch.float32)
    return out


def sincos_formula(hidden, tokens):
    """get_1d_sincos_pos_embed (dit_model.py:556-615) restated: [sin | cos], omega_i = 10000^(-i / (hidden / 2)), positions 0 .. tokens - 1"""
    omega = 1.0 / 10000 ** (np.arange(hidden // 2, dtype=np.float64) / (hidden / 2.0))
    out = np.einsum("m,d->md", np.arange(tokens, dtype=np.float64), omega)
    return np.concatenate([np.sin(out), np.cos(out)], axis=1)


def attention_mask(tokens, length, mode, dtype):
    """additive (N, N) mask, rows = queries: "frame" frame(key) > frame(query) is masked (the reference's, dit_model.py:407-427), "none",
    "token" key > query (a per-token causal mask), "transposed" frame(key) < frame(query) (the reference's mask transposed)"""
    if mode == "none":
        return None
    i = torch.arange(tokens * length)
    fq, fk = (i // length)[:, None], (i // length)[None, :]
    banned = {"frame": fk > fq, "token": i[None, :] > i[:, None], "transposed": fk < fq}[mode]
    return torch.zeros(tokens * length, tokens * length, dtype=dtype).masked_fill(banned, float("-inf"))


def timestep_embedding(levels, dtype):
    """TimestepEmbedder.timestep_embedding (dit_model.py:133-150): [cos | sin], the argument formed in fp32 as the reference forms it"""
    half = FREQ_DIM // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float32) / half).to(levels.device)
    args = levels[:, :, None].float() * freqs[None, None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1).to(dtype)


def forward_host(params, x, levels, heads, mask="frame", residual="norm", dtype=torch.float64):
    """DIT1D.forward (dit_model.py:494-530) with the share_norm block (:248-271).  mask: see attention_mask; residual "norm" is the
    reference's (the LayerNorm output is the residual base), "raw" keeps the stream that entered the block (what every other DiT does)."""
    p = {n: t.to(dtype) for n, t in params.items()}
    b, t, c, _, length = x.shape
    h = p["x_embedder.weight"].shape[0]
    d = h // heads
    tok = x.to(dtype)[..., 0, :].permute(0, 1, 3, 2).reshape(b, t * length, c)
    s = F.linear(tok, p["x_embedder.weight"], p["x_embedder.bias"]) + p["pos_embed"]
    te = timestep_embedding(levels, dtype)
    te = F.linear(F.silu(F.linear(te, p["t_embedder.mlp.0.weight"], p["t_embedder.mlp.0.bias"])), p["t_embedder.mlp.2.weight"],
                  p["t_embedder.mlp.2.bias"])
    am = attention_mask(t, length, mask, dtype)
    if am is not None:
        am = am.to(x.device)

    def per_token(v):  # (B, T, H) -> (B, T*L, H)
        return v[:, :, None, :].expand(b, t, length, h).reshape(b, t * length, h)
    depth = sum(1 for n in p if n.endswith("attn.qkv.weight"))
    for i in range(depth):
        pre = f"blocks.{i}"
        mod = F.linear(F.silu(te), p[f"{pre}.adaLN_modulation.1.weight"], p[f"{pre}.adaLN_modulation.1.bias"])
        sh1, sc1, g1, sh2, sc2, g2 = (per_token(m) for m in mod.chunk(6, dim=2))
        n1 = F.layer_norm(s, (h,), eps=1e-6)
        base = n1 if residual == "norm" else s
        qkv = F.linear(n1 * (1 + sc1) + sh1, p[f"{pre}.attn.qkv.weight"], p[f"{pre}.attn.qkv.bias"])
        q, k, v = qkv.view(b, t * length, 3, heads, d).permute(2, 0, 3, 1, 4)
        a = (q * d ** -0.5) @ k.transpose(-2, -1)
        if am is not None:
            a = a + am
        o = (a.softmax(dim=-1) @ v).transpose(1, 2).reshape(b, t * length, h)
        s = base + g1 * F.linear(o, p[f"{pre}.attn.proj.weight"], p[f"{pre}.attn.proj.bias"])
        n2 = F.layer_norm(s, (h,), eps=1e-6)
        base = n2 if residual == "norm" else s
        m = F.linear(F.gelu(F.linear(n2 * (1 + sc2) + sh2, p[f"{pre}.mlp.fc1.weight"], p[f"{pre}.mlp.fc1.bias"]), approximate="tanh"),
                     p[f"{pre}.mlp.fc2.weight"], p[f"{pre}.mlp.fc2.bias"])
        s = base + g2 * m
    out = F.linear(F.layer_norm(s, (h,), eps=1e-6), p["final_layer.1.weight"], p["final_layer.1.bias"])
    return out.view(b, t, length, c).permute(0, 1, 3, 2).unsqueeze(-2)


def build(tag, qk_gain, causal_attn_mode="video_temporal_causal"):
    """the engine's DiT1D at the fixture's configuration with the seeded weights"""
    import dfot_amd
    heads = CASES[tag]
    params = seeded_params(key_shapes(heads), qk_gain)
    model = dfot_amd.DiT1D(backbone_cfg(heads, causal_attn_mode=causal_attn_mode), x_shape=X_SHAPE, max_tokens=MAX_TOKENS).cuda().eval()
    model.load_state_dict(params, strict=True)
    return model, params
