#!/usr/bin/env python3
"""What the 3-line backbone registration delivers on its own: the reference's sampling loop around a plain
``model(x, k, cond, mask)``, at the headline shape (RE10K model, model batch 2 = one video x 2 History-Guidance branches, 8 frames, 256 x 256).

The reference's sampler builds a NEW conditioning tensor on every DDIM step (dfot_video.py:728-746 -> dfot_video_pose.py:64-110), so the
backbone's identity-keyed pose / FiLM cache never hits there; the content key (dfot_op_equal_bits) does.  Legs, each a fresh child process
under its own time limit (a leg that fails or runs out of time ends the run; nothing is started after it):

  dropin   per step: dfot::ray_encoding of the same poses (a fresh 755 MB tensor) -> dfot::hg_prepare -> model(x_in, k, cond_fresh, None)
           -> dfot::ddim_hg_step; no live / fresh hints.  ms per step over --samples samples of --steps steps after one warm-up sample.
  same     the same loop with ONE conditioning tensor per sample (identity hit on every step but the first = forward_cached): what this
           project's own sampler pays for the backbone, without its frame hints and graph
  ops      HIP events, alone on the device: dfot_op_equal_bits on two 755 MB buffers (5 warm-up + 50 timed launches), one
           dfot_uvit_set_conditions and one dfot::ray_encoding at the same shape

Only the public Python surface is used, so the script also runs on a commit without the content key (``cond_cache_stats`` and the compare are
then reported as null).  Prints ONE JSON line.  Usage (GPU box): python tools/bench_dropin.py [--steps 50] [--samples 3] [--legs dropin,same,ops]"""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RE10K = dict(channels=[128, 256, 576, 1152], emb_channels=1024, patch_size=2,
             block_types=["ResBlock", "ResBlock", "TransformerBlock", "TransformerBlock"],
             num_updown_blocks=[3, 3, 6], num_mid_blocks=20, num_heads=9, pos_emb_type="rope",
             use_fourier_noise_embedding=True, conditioning=dict(dim=180))
RES, T, NFE, BM = 256, 8, 2, 2
HBM_TBS = 8.0  # the HBM3E rate the repository's rooflines use
LEG_TIMEOUT = {"dropin": 420, "same": 300, "ops": 240}  # seconds, model set-up and the first import of torch included


def poses(seed=100):
    import torch
    g = torch.Generator().manual_seed(seed)
    k = torch.tensor([0.5, 0.9, 0.5, 0.5]).repeat(1, T, 1)
    ang = 0.1 * torch.randn(1, T, generator=g).cumsum(1)
    c, s, o, z = ang.cos(), ang.sin(), torch.ones_like(ang), torch.zeros_like(ang)
    rot = torch.stack([c, z, s, z, o, z, -s, z, c], -1).view(1, T, 3, 3)
    trans = torch.stack([torch.linspace(0, 0.5, T).repeat(1, 1), torch.zeros(1, T), torch.linspace(0, -0.3, T).repeat(1, 1)], -1)
    raw = torch.cat([k, torch.cat([rot, trans[..., None]], -1).reshape(1, T, 12)], -1)
    return raw.repeat(BM, 1, 1).cuda()  # both History-Guidance branches see the video's poses


def step_tables(steps):
    """per-step coefficient tables of a DDIM sample with vanilla History Guidance 4.0 (frame 0 = context: kept by the conditional branch,
    fully noised for the unconditional one), cosine schedule; [steps][...] on the device, built before the timed region"""
    import torch
    abar = lambda u: math.cos(0.5 * math.pi * min(max(u, 0.0), 1.0) * 0.999) ** 2
    tabs = {n: torch.zeros(steps, BM, T) for n in ("qa", "qb", "sa", "s1", "an", "cn", "keep", "k")}
    for i in range(steps):
        a_k, a_n = abar(1.0 - i / steps), abar(1.0 - (i + 1) / steps)
        tabs["qa"][i], tabs["sa"][i], tabs["s1"][i], tabs["an"][i], tabs["cn"][i] = 1.0, math.sqrt(a_k), math.sqrt(1 - a_k), math.sqrt(a_n), math.sqrt(1 - a_n)
        tabs["k"][i] = 0.125 * math.log(a_k / (1 - a_k))
        tabs["keep"][i, :, 0] = 1.0
        tabs["qa"][i, 1, 0], tabs["qb"][i, 1, 0] = 0.0, 1.0                         # unconditional branch: the context frame is noise
        tabs["k"][i, 0, 0], tabs["k"][i, 1, 0] = 0.125 * 20.0, 0.125 * -20.0        # clean / fully noised context level
    gen = torch.ones(1, T, dtype=torch.uint8)
    gen[0, 0] = 0
    return {n: t.cuda() for n, t in tabs.items()}, torch.tensor([5.0, -4.0]).cuda(), gen.cuda()


def leg_loop(args, fresh_cond: bool):
    import torch
    import dfot_amd
    model = dfot_amd.UViT3DPose(RE10K, x_shape=(3, RES, RES), max_tokens=T).cuda()
    model.init_random(seed=0)
    raw = poses()
    tabs, weight, gen = step_tables(args.steps)
    x0 = torch.randn(1, T, 3, RES, RES, generator=torch.Generator().manual_seed(0)).cuda()
    noise = torch.randn(BM, T, 3, RES, RES, generator=torch.Generator().manual_seed(1)).cuda()
    ops = torch.ops.dfot

    def sample():
        x = x0
        cond = None
        for i in range(args.steps):
            if fresh_cond or cond is None:
                cond = ops.ray_encoding(raw, RES)                                     # a NEW (Bm, 8, 180, 256, 256) tensor
            x_in = ops.hg_prepare(x, noise, tabs["qa"][i], tabs["qb"][i], NFE)
            v = model(x_in, tabs["k"][i], cond, None)
            x = ops.ddim_hg_step(x, x_in, v, tabs["sa"][i], tabs["s1"][i], tabs["an"][i], tabs["cn"][i], tabs["keep"][i], weight, gen, NFE)
        return x

    with torch.no_grad():
        sample()
        torch.cuda.synchronize()
        stats0 = dict(getattr(model, "cond_cache_stats", None) or {})
        t0 = time.perf_counter()
        for _ in range(args.samples):
            out = sample()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    assert torch.isfinite(out).all()
    stats = getattr(model, "cond_cache_stats", None)
    return {"ms_per_step": dt / (args.samples * args.steps) * 1e3, "steps_timed": args.samples * args.steps,
            "cond_cache_stats": None if stats is None else {n: stats[n] - stats0.get(n, 0) for n in stats},
            "checksum": float(out.double().abs().mean().item())}


def events(fn, warm, iters):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def leg_ops(args):
    import torch
    import dfot_amd
    from dfot_amd import capi
    P = lambda t: C.c_void_p(t.data_ptr())
    S = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    raw = poses()
    out = {}
    with torch.no_grad():
        cond = torch.ops.dfot.ray_encoding(raw, RES)
        nbytes = cond.numel() * cond.element_size()
        out["cond_bytes"] = nbytes
        out["ray_encoding_us"] = events(lambda: torch.ops.dfot.ray_encoding(raw, RES), 2, 10) * 1e3
        if hasattr(capi.lib, "dfot_op_equal_bits"):
            other = cond.clone()
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")
            ms = events(lambda: capi.check(capi.lib.dfot_op_equal_bits(P(cond), P(other), nbytes, P(flag), S())), 5, 50)
            assert int(flag.item()) == 0
            gbs = 2.0 * nbytes / ms / 1e6
            out["equal_bits"] = {"us": ms * 1e3, "GB_per_s": gbs, "bytes_read": 2 * nbytes, "frac_of_hbm_peak": gbs / 1e3 / HBM_TBS,
                                 "hbm_peak_TB_per_s": HBM_TBS, "warmup": 5, "launches": 50}
            del other
        else:
            out["equal_bits"] = None
        model = dfot_amd.UViT3DPose(RE10K, x_shape=(3, RES, RES), max_tokens=T).cuda()
        model.init_random(seed=0)
        model.sync_weights()
        model.reserve(BM)
        build = lambda: capi.check(capi.lib.dfot_uvit_set_conditions(model._handle, P(cond), None, BM, S()))
        out["set_conditions_us"] = events(build, 2, 10) * 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50, help="DDIM steps per sample")
    ap.add_argument("--samples", type=int, default=3, help="timed samples (one more runs first as warm-up)")
    ap.add_argument("--legs", default="dropin,same,ops")
    ap.add_argument("--leg", default=None, help="internal: this process IS one leg")
    args = ap.parse_args()
    if args.leg:
        res = leg_ops(args) if args.leg == "ops" else leg_loop(args, fresh_cond=args.leg == "dropin")
        print("LEG " + json.dumps(res), flush=True)
        return 0
    line = {"metric": "drop-in UViT3DPose.forward in the reference's sampling loop, RE10K 8f, model batch 2, 256x256", "unit": "ms/step",
            "steps": args.steps, "samples": args.samples}
    rc = 0
    for leg in args.legs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--steps", str(args.steps), "--samples", str(args.samples)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT[leg])
        except subprocess.TimeoutExpired:
            line[leg] = {"error": f"no result within {LEG_TIMEOUT[leg]} s"}
            rc = 1
            break
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
        if r.returncode != 0 or not got:
            line[leg] = {"error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
            rc = 1
            break  # after a failed GPU step nothing more is started on the device
        line[leg] = json.loads(got[-1][4:])
    if "dropin" in line and "same" in line and "ms_per_step" in line["dropin"] and "ms_per_step" in line.get("same", {}):
        line["value"] = line["dropin"]["ms_per_step"]
        line["dropin_over_same_tensor_ms"] = line["dropin"]["ms_per_step"] - line["same"]["ms_per_step"]
    print(json.dumps(line), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
