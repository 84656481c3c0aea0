"""Pure-torch helpers for the attention maps ``DiT3D.attention_maps()`` returns (the read-out of the reference's
algorithms/common/attn_hook/hook.py).  They run on any device and touch no kernel.

A *full* map is the softmax matrix ``A[b, head, i, j]`` over the N = tokens * P tokens of a video (frame-major: token i belongs to
frame ``i // P``).  The *frame* map keeps what the hook's heat map shows, per head:

    F[b, head, tq, tk] = (1/P) * sum_{i in frame tq} sum_{j in frame tk} A[b, head, i, j]

Its rows sum to 1; the hook's picture is ``F.sum(1)`` (hook.py:82-85, 132).
"""
from __future__ import annotations

import torch


def frame_map(full: torch.Tensor, tokens: int) -> torch.Tensor:
    """full [..., N, N] with N = tokens * P  ->  [..., tokens, tokens]: the mean over the query rows of a frame of the probability
    mass on the key columns of a frame."""
    n = full.shape[-1]
    if full.shape[-2] != n or tokens <= 0 or n % tokens:
        raise ValueError(f"frame_map: a [..., N, N] map with N divisible by tokens={tokens} is expected, got {tuple(full.shape)}")
    p = n // tokens
    lead = full.shape[:-2]
    return full.reshape(*lead, tokens, p, tokens, p).sum(dim=(-3, -1)) / p


def to_hook_layout(full: torch.Tensor, tokens: int, height: int, width: int) -> torch.Tensor:
    """full [B, heads, N, N] -> the layout Attention.forward stores for the hook (dit_blocks.py:118):
    ``rearrange(attn_map, 'b heads (t h w) d -> b heads t h w d', h=height, w=width)``, i.e. (B, heads, t, h, w, N)."""
    if full.ndim != 4 or full.shape[-2] != tokens * height * width or full.shape[-1] != full.shape[-2]:
        raise ValueError(f"to_hook_layout: expected [B, heads, N, N] with N = {tokens}*{height}*{width}, got {tuple(full.shape)}")
    b, heads, n, _ = full.shape
    return full.reshape(b, heads, tokens, height, width, n)
