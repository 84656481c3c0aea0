"""Shared helpers of tests/test_uvit3d_host.py, tests/test_gpu_uvit3d.py and tools/make_golden_uvit3d.py (not a test module): the
pose-free U-ViT (the reference's UViT3D, algorithms/dfot/backbones/u_vit/u_vit3d.py:22-335).

  * key_shapes        the reference module's state-dict keys and shapes, in its registration order (up_blocks before mid_blocks)
  * seeded_params     weights drawn per key from a seed derived from the key's name and shape (so the fixture stores a digest, not tensors)
  * forward_host      a torch restatement of UViT3D.forward in any float dtype, built on oracle.uvit's block functions
  * embedding         the per-frame embedding (noise MLP + action MLP) alone, the fp64 reference of the engine's "nemb" tap
"""
import hashlib
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import uvit as ouvit

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the smallest configuration the engine accepts: head dims 64 (level 2) and 128 (level 3), 8 x 4 x 4 = 128 tokens at the coarsest level
TINY = dict(channels=[128, 128, 128, 256], emb_channels=128, patch_size=2,
            block_types=["ResBlock", "ResBlock", "TransformerBlock", "TransformerBlock"], block_dropouts=[0.0, 0.0, 0.0, 0.0],
            num_updown_blocks=[1, 1, 1], num_mid_blocks=1, num_heads=2, pos_emb_type="rope", use_checkpointing=[False] * 4,
            use_fourier_noise_embedding=True)
X_SHAPE, MAX_TOKENS, BATCH = (3, 64, 64), 8, 2
COND_DIM, COND_DROPOUT = 4, 0.1
NOISE_DIM = 256
# fixture cases: tag -> (external_cond_dim, external_cond_dropout)
CASES = {"a": (0, 0.0), "b": (COND_DIM, 0.0), "c": (COND_DIM, COND_DROPOUT)}
FREQS, PHASES = "noise_level_pos_embedding.timesteps.freqs", "noise_level_pos_embedding.timesteps.phases"
ZERO_INIT = (".attn_out.", ".mlp_out.2.", ".out_rest.1.", "project_output")  # what the reference zero-initialises


def load(name="uvit3d.npz"):
    return np.load(os.path.join(GOLDEN, name))


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# A frame tensor of the fixture's shape is 786 KB, so the fixture (committed files stay under 1 MiB) holds no such tensor whole: the inputs are
# drawn here from fixed seeds (the fixture stores their digest), and every reference output is stored on the lattice sample() below
INPUT_SEED, TRACE_SEED, DRAW_SEED = 83, 84, 0
SAMPLE_START, SAMPLE_STRIDE = 5, 13  # 13 is coprime to every extent of the tensors: the lattice visits every video, frame, channel, row, column


def sample(t):
    return t.reshape(-1)[SAMPLE_START::SAMPLE_STRIDE]


def tensor_digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().numpy().tobytes())
    return h.hexdigest()


def inputs():
    """x [2,8,3,64,64], float levels [2,8] in the range of precond_scale * logsnr (both ends and 0 included), actions [2,8,4], mask"""
    g = torch.Generator().manual_seed(INPUT_SEED)
    x = torch.randn(BATCH, MAX_TOKENS, *X_SHAPE, generator=g)
    levels = 1.25 * torch.randn(BATCH, MAX_TOKENS, generator=g)
    levels[0, 0], levels[1, 7], levels[0, 3] = -2.5, 2.5, 0.0
    cond = torch.randn(BATCH, MAX_TOKENS, COND_DIM, generator=g)
    return x, levels, cond, torch.tensor([True, False])


def trace_inputs():
    g = torch.Generator().manual_seed(TRACE_SEED)
    return torch.randn(BATCH, MAX_TOKENS, *X_SHAPE, generator=g), torch.randn(BATCH, MAX_TOKENS, COND_DIM, generator=g)


def trace_draws(shapes):
    """the normal draws of the sampler trace: the reference draws them one after another from torch.Generator().manual_seed(DRAW_SEED)"""
    g = torch.Generator().manual_seed(DRAW_SEED)
    return [torch.randn(tuple(int(v) for v in s), generator=g) for s in shapes]


def backbone_cfg(dropout=0.0, **over):
    cfg = dict(TINY, name="u_vit3d", **over)
    if dropout:
        cfg["external_cond_dropout"] = dropout
    return cfg


def ocfg(**over):
    c = {**TINY, **over}
    return ouvit.UViTConfig(channels=tuple(c["channels"]), emb_channels=c["emb_channels"], num_updown_blocks=tuple(c["num_updown_blocks"]),
                            num_mid_blocks=c["num_mid_blocks"], num_heads=c["num_heads"], in_channels=X_SHAPE[0], resolution=X_SHAPE[-1],
                            max_tokens=MAX_TOKENS, cond_dim=0, noise_dim=NOISE_DIM)


def key_shapes(cond_dim=0, cond_dropout=0.0, **over):
    """[(state-dict key, shape)] in the order the reference registers them: base_backbone.py:35-40 (the two embeddings), then
    u_vit3d.py:67-185: embed_input, project_output, down_blocks, up_blocks (both lists are created before mid_blocks is assigned), mid_blocks.
    The RoPE tables (pos_embs) are non-persistent buffers and do not appear."""
    oc = ocfg(**over)
    e, ch = oc.emb_channels, list(oc.channels)
    out = [(FREQS, (NOISE_DIM,)), (PHASES, (NOISE_DIM,))]

    def linear(name, o, i):
        out.extend([(f"{name}.weight", (o, i)), (f"{name}.bias", (o,))])
    linear("noise_level_pos_embedding.embedding.linear_1", e, NOISE_DIM)
    linear("noise_level_pos_embedding.embedding.linear_2", e, e)
    if cond_dim:
        pre = "external_cond_embedding" + (".embedding" if cond_dropout > 0 else "")
        linear(f"{pre}.linear_1", e, cond_dim)
        linear(f"{pre}.linear_2", e, e)
    out += [("embed_input.proj.weight", (ch[0], oc.in_channels, 2, 2)), ("embed_input.proj.bias", (ch[0],)),
            ("project_output.proj.weight", (ch[0], oc.in_channels, 2, 2)), ("project_output.proj.bias", (oc.in_channels,))]

    def block(prefix, lvl):
        shapes = ouvit._res_block_shapes(prefix, ch[lvl], e) if lvl < 2 else ouvit._tr_block_shapes(prefix, ch[lvl], e, oc.num_heads)
        out.extend(shapes.items())
    for lvl, n in enumerate(oc.num_updown_blocks):
        for i in range(n):
            block(f"down_blocks.{lvl}.{i}", lvl)
        out += [(f"down_blocks.{lvl}.{n}.conv.weight", (ch[lvl + 1], ch[lvl], 3, 3)), (f"down_blocks.{lvl}.{n}.conv.bias", (ch[lvl + 1],))]
    for j, lvl in enumerate(reversed(range(3))):
        out += [(f"up_blocks.{j}.0.conv.weight", (ch[lvl], ch[lvl + 1], 3, 3)), (f"up_blocks.{j}.0.conv.bias", (ch[lvl],))]
        for i in range(oc.num_updown_blocks[lvl]):
            block(f"up_blocks.{j}.{i + 1}", lvl)
    for i in range(oc.num_mid_blocks):
        block(f"mid_blocks.{i}", 3)
    return out


def seeded_params(keys):
    """every tensor from its own generator, seeded by sha256(name, shape): Fourier freqs 2 pi N(0,1), phases 2 pi U(0,1), norm gains
    1 + N(0, 0.1^2), biases N(0, 0.05^2), weights N(0, 1/fan_in), at 0.3 gain for the layers the reference zero-initialises (they are NOT zero
    here: zeros would hide every block)."""
    out = {}
    for name, shape in keys:
        seed = int.from_bytes(hashlib.sha256(f"{name}{tuple(shape)}".encode()).digest()[:7], "little")
        g = torch.Generator().manual_seed(seed)
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "freqs":
            t = 2 * math.pi * torch.randn(shape, generator=g)
        elif leaf == "phases":
            t = 2 * math.pi * torch.rand(shape, generator=g)
        elif leaf == "bias":
            t = 0.05 * torch.randn(shape, generator=g)
        elif len(shape) == 1:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            fan_in = shape[0] if name.startswith("project_output") else math.prod(shape[1:])
            t = torch.randn(shape, generator=g) / math.sqrt(fan_in)
            if any(s in name for s in ZERO_INIT):
                t = 0.3 * t
        out[name] = t.to(torch.float32)
    return out


def digest(params):
    h = hashlib.sha256()
    for k in params:
        h.update(k.encode())
        h.update(params[k].contiguous().numpy().tobytes())
    return h.hexdigest()


def case_params(tag):
    return seeded_params(key_shapes(*CASES[tag]))


def embedding(params, levels, cond=None, mask=None, dtype=torch.float64):
    """emb = noise_level_pos_embedding(k) [+ external_cond_embedding(cond, mask)], (B, T, E) (u_vit3d.py:306-310).  The Fourier argument is
    formed in fp32 as the reference forms it (embeddings.py:104-109); everything after it in `dtype`."""
    p = {n: t.to(dtype) for n, t in params.items()}
    arg = levels.to(torch.float32)[..., None] * params[FREQS].float() + params[PHASES].float()
    feat = arg.to(dtype).cos() * math.sqrt(2.0)
    pre = "noise_level_pos_embedding.embedding"
    emb = F.linear(F.silu(F.linear(feat, p[f"{pre}.linear_1.weight"], p[f"{pre}.linear_1.bias"])), p[f"{pre}.linear_2.weight"], p[f"{pre}.linear_2.bias"])
    if cond is not None:
        pre = next(n for n in p if n.startswith("external_cond_embedding")).rsplit(".linear_1", 1)[0]
        ce = F.linear(F.silu(F.linear(cond.to(dtype), p[f"{pre}.linear_1.weight"], p[f"{pre}.linear_1.bias"])),
                      p[f"{pre}.linear_2.weight"], p[f"{pre}.linear_2.bias"])
        if mask is not None and pre.endswith(".embedding"):  # dropout 0: a plain TimestepEmbedding, the mask is never seen (embeddings.py:385-386)
            ce = torch.where(mask.view(-1, 1, 1), torch.zeros_like(ce), ce)
        emb = emb + ce
    return emb


def forward_host(params, x, levels, cond=None, mask=None, dtype=torch.float64, **over):
    """UViT3D.forward (u_vit3d.py:284-335): the per-frame embedding reaches the ResBlocks as emb[:, :, None, None] (u_vit_blocks.py:89) and the
    transformer levels repeated over h w (u_vit3d.py:218); the blocks are oracle.uvit's."""
    oc = ocfg(**over)
    p = {n: t.to(dtype) for n, t in params.items()}
    b, t = x.shape[:2]
    assert t == oc.max_tokens
    emb = embedding(params, levels, cond, mask, dtype).flatten(0, 1)  # (B*T, E)
    h = F.conv2d(x.to(dtype).flatten(0, 1), p["embed_input.proj.weight"], p["embed_input.proj.bias"], stride=2)
    angles = {lvl: ouvit.rope3d_angles(oc.channels[lvl] // oc.num_heads, (t, oc.level_res(lvl), oc.level_res(lvl)), oc.rope_theta).to(dtype)
              for lvl in (2, 3)}

    def run_level(h, lvl, prefixes):
        if lvl < 2:
            for pre in prefixes:
                h = ouvit.res_block(p, pre, h, emb[:, :, None, None], oc)
            return h
        hh, ww = h.shape[-2:]
        tok = h.view(b, t, -1, hh, ww).permute(0, 1, 3, 4, 2).reshape(b, t * hh * ww, -1)
        etok = emb.view(b, t, 1, -1).expand(b, t, hh * ww, emb.shape[-1]).reshape(b, t * hh * ww, -1)
        for pre in prefixes:
            tok = ouvit.transformer_block(p, pre, tok, etok, angles[lvl], oc)
        return tok.view(b, t, hh, ww, -1).permute(0, 1, 4, 2, 3).reshape(b * t, -1, hh, ww)

    before, after = [], []
    for lvl, n in enumerate(oc.num_updown_blocks):
        h = run_level(h, lvl, [f"down_blocks.{lvl}.{i}" for i in range(n)])
        before.append(h)
        h = F.conv2d(F.avg_pool2d(h, 2, 2), p[f"down_blocks.{lvl}.{n}.conv.weight"], p[f"down_blocks.{lvl}.{n}.conv.bias"], padding=1)
        after.append(h)
    h = run_level(h, 3, [f"mid_blocks.{i}" for i in range(oc.num_mid_blocks)])
    for j, lvl in enumerate(reversed(range(3))):
        h = h - after.pop()
        h = F.conv2d(h, p[f"up_blocks.{j}.0.conv.weight"], p[f"up_blocks.{j}.0.conv.bias"], padding=1)
        h = F.interpolate(h, scale_factor=2, mode="nearest") + before.pop()
        h = run_level(h, lvl, [f"up_blocks.{j}.{i + 1}" for i in range(oc.num_updown_blocks[lvl])])
    out = F.conv_transpose2d(h, p["project_output.proj.weight"], p["project_output.proj.bias"], stride=2)
    return out.view(b, t, *out.shape[1:])


def build(tag, cond_dim=None, **over):
    """the engine's UViT3D at the fixture's configuration with the seeded weights, eval() as the reference's module was"""
    import dfot_amd
    dim, drop = CASES[tag]
    dim = dim if cond_dim is None else cond_dim
    params = seeded_params(key_shapes(dim, drop, **over))
    model = dfot_amd.UViT3D(backbone_cfg(drop, **over), x_shape=X_SHAPE, max_tokens=MAX_TOKENS, external_cond_dim=dim).cuda().eval()
    model.load_state_dict(params, strict=True)
    return model, params
