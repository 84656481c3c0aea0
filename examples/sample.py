#!/usr/bin/env python3
"""End-to-end sampling with the MI355X engine, the way the reference's validation loop calls its algorithm.

  python examples/sample.py re10k    [--ckpt DFoT_RE10K.ckpt] [--frames 8] [--steps 50] [--out out.npz]
  python examples/sample.py k600     [--ckpt K600.ckpt] [--batch 8]
  python examples/sample.py k600diff [--ckpt ...]
  python examples/sample.py facdit   [--ckpt ...]   (FacDiT-XL, the taichikl recipe: 4x32x32 latents, patch 2, 16 frames)
  python examples/sample.py facmat   [--ckpt ...]   (FacMatDiT XL-64-1, the same recipe: matrix attention with RoPE over the 16 frames)
  python examples/sample.py facdit-s128 [--ckpt ...]   (FacDiT-S, the taichi res-128 recipes: 4x16x16 latents, patch 2 = 64 patches per frame,
                                                        16 frames; --decode-image-vae gives the 128x128 frames)
  python examples/sample.py facmat-s128 [--ckpt ...]   (FacMatDiT S-64-1 of the same ladder: 12 spatial heads, 1 x 6 matrix heads, use_bias)
  python examples/sample.py facmat-s128-1 / facmat-s128-8   (FacMatDiT S-1-1 / S-8-1 with use_bias, the narrow rungs of that ladder: the left
                                                        factors of the matrix blocks are the streaming kernels of csrc/facmat_narrow.hip)
  python examples/sample.py facmat-s128 --embed-col-dim 32 --col-heads 4   (any other rung: a width of 1 .. 32 or a multiple of 64)
  python examples/sample.py <k600|facdit|facmat> --attention-maps maps.npz [--attention-steps 0 25 49]   (which frame attends to which)
  python examples/sample.py uvit3d   [--cond action:4]   (the pose-free U-ViT at the RE10K widths, 256x256 frames, continuous diffusion)
  python examples/sample.py k600 --continuous --decode-image-vae   (latents -> frames through a random-weight per-frame ImageVAE)
  python examples/sample.py facdit --decode-image-vae [--image-vae-ckpt sd-vae-ft-ema/]   (the taichikl recipe's KL-f8 autoencoder:
                                                     4x32x32 latents -> 256x256 frames; the checkpoint in the diffusers layout)
  python examples/sample.py mcraft   [--ckpt ...]   (the Minecraft / dmlab DiT recipe: @DiT/B on 32x8x8 latents, patch 2, 16 frames, actions of
                                                     dim 4 with mask_first, continuous diffusion; --decode-image-vae decodes the 8x8 latents)
  python examples/sample.py mcraft --decode-dc-ae [--dc-ae 8x|16x] [--dc-ae-ckpt dcae.pth] [--encode-dc-ae]   (the recipe's own autoencoder:
                                                     DC-AE, 32x8x8 latents -> 64x64 frames (8x, dmlab) or 128x128 frames (16x, Minecraft);
                                                     --encode-dc-ae encodes synthetic context frames into the run's context latents)
  python examples/sample.py taichi --decode-titok [--titok-ckpt model.safetensors]   (DiT-XL on the 1-D token latents 4x1x32 of the taichi
                                                     recipe, patch 1, 16 frames; TiTok-KL decoder: 32 tokens -> a 256x256 frame)
  python examples/sample.py taichi --encode-titok [--decode-titok] [--titok-ckpt model.safetensors]   (the context latents of the run are
                                                     256x256 context frames encoded by the TiTok-KL encoder: frames -> latents -> latents -> frames)
  python examples/sample.py taichi1d [--decode-titok] [--encode-titok]   (DiT1D, the frame-causal backbone at the stock dit1d.yaml widths, on
                                                     the same 4x1x32 token latents, 16 frames: every frame attends to itself and earlier frames)

Without --ckpt the backbone gets seeded random weights (there is no network here to fetch the released checkpoints);
with it, the reference's .ckpt / ema.safetensors is read by dfot_amd.load_reference_checkpoint (keys
`diffusion_model.model.*`, optional `_orig_mod.` prefix, EMA weights).  Inputs are synthetic unless --inputs points at an
.npz with `xs` (B,T,C,H,W, already normalised) and, for re10k, `conditions` (B,T,16 raw camera poses).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dfot_amd  # noqa: E402
from bench import RE10K, synth_poses  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model", choices=["re10k", "uvit3d", "k600", "k600diff", "facdit", "facmat", "facdit-s128", "facmat-s128", "facmat-s128-1",
                                      "facmat-s128-8", "taichi", "taichi1d", "mcraft"])
    ap.add_argument("--ckpt")
    ap.add_argument("--inputs")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="sample_out.npz")
    ap.add_argument("--embed-col-dim", type=int, help="facmat*: column width of the matrix token (1 .. 32 or a multiple of 64; default: the recipe's)")
    ap.add_argument("--col-heads", type=int, help="facmat*: num_col_heads (must divide the column width; default 1)")
    ap.add_argument("--cond", help="k600 / k600diff: synthetic external condition, 'action:DIM' (e.g. action:3, as dmlab) or 'label:CLASSES' (label:101)")
    ap.add_argument("--continuous", action="store_true",
                    help="k600 / k600diff / facdit / facmat: continuous diffusion as @diffusion/continuous (Fourier noise-level embedding, float levels, "
                         "cosine_simple_diffusion shifted 0.125), the way the dmlab / Minecraft DiT recipes run")
    ap.add_argument("--decode-image-vae", action="store_true",
                    help="decode the sampled latents with an ImageVAE (image_vae.yaml widths, z_channels = the latent channels; random weights "
                         "unless --image-vae-ckpt is given), the per-frame autoencoder of the dmlab / Minecraft / taichikl recipes; latents of "
                         "8x8, 16x16 (k600; facdit-s128 / facmat-s128: 128x128 frames) or 32x32 (facdit / facmat: 256x256 frames), the mid "
                         "attention's sizes")
    ap.add_argument("--image-vae-ckpt", metavar="PATH",
                    help="with --decode-image-vae: a VAE in the diffusers layout (a folder with config.json and a .safetensors file, e.g. "
                         "stabilityai/sd-vae-ft-ema or the fine-tuned Taichi VAE), read by dfot_amd.load_diffusers_checkpoint")
    ap.add_argument("--decode-titok", action="store_true",
                    help="taichi: decode the sampled 4x1x32 token latents with the TiTok-KL decoder (the `large` preset at 256x256, as "
                         "titok_kl_preprocessor; random weights unless --titok-ckpt is given)")
    ap.add_argument("--encode-titok", action="store_true",
                    help="taichi: encode synthetic 256x256 context frames with the TiTok-KL encoder (the `large` preset, as titok_kl_preprocessor; "
                         "random weights unless --titok-ckpt is given) into the context latents of the run")
    ap.add_argument("--titok-ckpt", metavar="model.safetensors",
                    help="with --decode-titok / --encode-titok: the recipe's TiTok_KL checkpoint, read by dfot_amd.load_titok_checkpoint (one file "
                         "feeds both halves)")
    ap.add_argument("--decode-dc-ae", action="store_true",
                    help="mcraft: decode the sampled 32x8x8 latents with the DC-AE decoder (dc_ae_preprocessor / dc_ae_16x_preprocessor widths; "
                         "random weights unless --dc-ae-ckpt is given)")
    ap.add_argument("--encode-dc-ae", action="store_true",
                    help="mcraft: encode synthetic context frames (64x64 at 8x, 128x128 at 16x) with the DC-AE encoder into the context latents "
                         "of the run")
    ap.add_argument("--dc-ae", choices=["8x", "16x"], default="8x", help="the DC-AE configuration: 8x (dmlab, 64x64 frames) or 16x (Minecraft, 128x128)")
    ap.add_argument("--dc-ae-ckpt", metavar="PATH",
                    help="with --decode-dc-ae / --encode-dc-ae: the flat .pth / .safetensors state dict of the reference's MyAutoencoderDC, read "
                         "by dfot_amd.load_dcae_checkpoint (one file feeds both halves)")
    ap.add_argument("--attention-maps", metavar="OUT.npz",
                    help="k600 / facdit / facmat: write the frame-to-frame attention maps of every frame-mixing block (per head, query frame x key "
                         "frame; rows follow the model batch) at the steps of --attention-steps, as '<step>/<block name>' and '<step>/noise_levels'")
    ap.add_argument("--attention-steps", type=int, nargs="*", default=None, help="step indices of the window (default: first, middle, last)")
    a = ap.parse_args()
    if a.attention_maps and not (a.model in ("k600", "facdit", "facdit-s128") or a.model.startswith("facmat")):
        raise SystemExit("--attention-maps: the DiT3D models k600, facdit, facdit-s128 and facmat* only")
    if (a.embed_col_dim or a.col_heads) and not a.model.startswith("facmat"):
        raise SystemExit("--embed-col-dim / --col-heads: the facmat* models only")
    if (a.decode_titok or a.encode_titok) and a.model not in ("taichi", "taichi1d"):
        raise SystemExit("--decode-titok / --encode-titok: the taichi / taichi1d models only (latents of 4x1x32 tokens)")
    if (a.decode_dc_ae or a.encode_dc_ae) and a.model != "mcraft":
        raise SystemExit("--decode-dc-ae / --encode-dc-ae: the mcraft model only (latents of 32x8x8)")
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    noise = dfot_amd.device_noise_fn(gen)
    conds = None
    if a.model == "re10k":
        model = dfot_amd.UViT3DPose(RE10K, x_shape=(3, 256, 256), max_tokens=8).cuda()
        long_video = a.frames > 8
        cfg = dfot_amd.SamplerConfig(
            x_shape=(3, 256, 256), max_tokens=8, diffusion=dfot_amd.DiffusionConfig(sampling_timesteps=a.steps),
            prediction_guidance=(dict(name="stabilized_vanilla", guidance_scale=4.0, stabilization_level=0.02) if long_video
                                 else dict(name="vanilla", guidance_scale=4.0)),
            interpolation_guidance=dict(name="vanilla", guidance_scale=1.5), keyframe_density=(0.0625 if a.frames >= 128 else 0.5) if long_video else None,  # >= max_tokens key frames
            interpolation_max_batch_size=4)
        sampler = dfot_amd.DFoTVideoPoseSampler(cfg, model, noise)
        xs = torch.randn(a.batch, a.frames, 3, 256, 256, generator=torch.Generator().manual_seed(a.seed))
        conds = synth_poses(a.batch, a.frames, 100 + a.seed)
        n_ctx = 1
    elif a.model == "uvit3d":  # UViT3DPose's parent class: no poses; unconditioned, or actions (B, T, DIM) as dmlab / Minecraft pass them
        dim = 0
        if a.cond:
            ctype, num = a.cond.split(":")
            if ctype != "action":
                raise SystemExit("uvit3d takes --cond action:DIM only")
            dim = int(num)
            conds = torch.randn(a.batch, 8, dim, generator=torch.Generator().manual_seed(200 + a.seed))
        ucfg = {k: v for k, v in RE10K.items() if k != "conditioning"}
        model = dfot_amd.UViT3D(ucfg, x_shape=(3, 256, 256), max_tokens=8, external_cond_dim=dim, use_causal_mask=False).cuda()
        cfg = dfot_amd.SamplerConfig(x_shape=(3, 256, 256), max_tokens=8, diffusion=dfot_amd.DiffusionConfig(sampling_timesteps=a.steps, is_continuous=True),
                                     prediction_guidance=dict(name="vanilla", guidance_scale=1.5) if dim else {"name": "conditional"},
                                     external_cond_type="action", external_cond_dim=dim, external_cond_processing="mask_first" if dim else None)
        sampler = dfot_amd.DFoTVideoSampler(cfg, model, noise)
        xs = torch.randn(a.batch, 8, 3, 256, 256, generator=torch.Generator().manual_seed(a.seed))
        n_ctx = 2
    elif a.model == "mcraft":  # `dataset=minecraft algorithm=dfot_video @diffusion/continuous @DiT/B`: a 128-wide patch vector, 256 tokens per video
        x_shape, tokens, dim = (32, 8, 8), 16, 4
        bb = dict(name="dit3d", variant="full", pos_emb_type="rope_3d", patch_size=2, hidden_size=768, depth=12, num_heads=12, mlp_ratio=4.0,
                  external_cond_dropout=0.1, use_fourier_noise_embedding=True)
        model = dfot_amd.DiT3D(bb, x_shape=x_shape, max_tokens=tokens, external_cond_type="action", external_cond_dim=dim).cuda()
        cfg = dfot_amd.SamplerConfig(x_shape=x_shape, max_tokens=tokens, diffusion=dfot_amd.DiffusionConfig(sampling_timesteps=a.steps, is_continuous=True),
                                     prediction_guidance=dict(name="vanilla", guidance_scale=1.5), external_cond_type="action", external_cond_dim=dim,
                                     external_cond_processing="mask_first")
        sampler = dfot_amd.DFoTVideoSampler(cfg, model, noise)
        xs = torch.randn(a.batch, tokens, *x_shape, generator=torch.Generator().manual_seed(a.seed))
        conds = torch.randn(a.batch, tokens, dim, generator=torch.Generator().manual_seed(200 + a.seed))
        n_ctx = 4
    elif a.model == "taichi1d":  # `backbone=dit1d` at the stock dit1d.yaml widths: the frame-causal transformer over the 4x1x32 token latents
        x_shape, tokens = (4, 1, 32), 16
        bb = dict(name="dit1d", hidden_size=1152, depth=28, num_heads=16, mlp_ratio=4, learn_sigma=False, merge_mode="share_norm",
                  causal_attn_mode="video_temporal_causal", use_rotary_emb=False, qk_norm=False)
        model = dfot_amd.DiT1D(bb, x_shape=x_shape, max_tokens=tokens).cuda()
        cfg = dfot_amd.SamplerConfig(x_shape=x_shape, max_tokens=tokens,
                                     diffusion=dfot_amd.DiffusionConfig(sampling_timesteps=a.steps, beta_schedule="cosine", is_continuous=False),
                                     prediction_guidance={"name": "conditional"})
        sampler = dfot_amd.DFoTVideoSampler(cfg, model, noise)
        xs = torch.randn(a.batch, tokens, *x_shape, generator=torch.Generator().manual_seed(a.seed))
        n_ctx = 2
    else:
        s128 = "-s128" in a.model  # the res-128 ladder: S widths, depth 6, 16x16 latents (64 patches per frame)
        diff, fac, facmat = a.model == "k600diff", a.model.startswith("facdit"), a.model.startswith("facmat")
        x_shape, tokens = ((4, 16, 16), 16) if s128 else ((4, 32, 32), 16) if fac or facmat else ((4, 1, 32), 16) if a.model == "taichi" else ((16, 16, 16), 5)
        ckw, skw = {}, {}
        if a.cond:
            ctype, num = a.cond.split(":")
            ckw = dict(external_cond_type=ctype, external_cond_dim=int(num) if ctype == "action" else 1,
                       external_cond_num_classes=int(num) if ctype == "label" else None)
            skw = dict(external_cond_type=ctype, external_cond_dim=ckw["external_cond_dim"], external_cond_processing="mask_first" if ctype == "action" else None)
            g = torch.Generator().manual_seed(200 + a.seed)
            conds = torch.randn(a.batch, tokens, int(num), generator=g) if ctype == "action" else torch.randint(0, int(num), (a.batch, 1), generator=g)
        if diff:
            bb = dict(name="difference_dit3d", variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", merge_type="interleaved",
                      patch_size=1, embed_col_dim=64, embed_row_dim=1152, num_heads=12, num_col_heads=1, num_row_heads=16, depth=28,
                      mlp_ratio=4.0, spatial_mlp_ratio=4.0, use_bias=True, matrix_block="matrix")
            model = dfot_amd.DifferenceDiT3D(dict(bb, use_fourier_noise_embedding=a.continuous), x_shape=(16, 16, 16), max_tokens=5, **ckw).cuda()
        elif fac:  # per depth a per-frame spatial block and a temporal block over the 16 frames of every patch position (inference only)
            bb = dict(name="dit3d", variant="factorized_attention", pos_emb_type="sinusoidal_factorized", patch_size=2, hidden_size=1152,
                      depth=28, num_heads=16, mlp_ratio=4.0, spatial_mlp_ratio=0.0)
            if s128:  # @FacDiT/S
                bb.update(hidden_size=384, depth=6, num_heads=6)
            model = dfot_amd.DiT3D(dict(bb, use_fourier_noise_embedding=a.continuous), x_shape=x_shape, max_tokens=tokens, **ckw).cuda()
        elif facmat:  # per depth a per-frame spatial block and a matrix block whose attention takes every frame as one token (inference only)
            bb = dict(name="dit3d", variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", use_temporal_rope=True, patch_size=2,
                      embed_col_dim=64, embed_row_dim=1152, num_heads=16, num_col_heads=1, num_row_heads=16, depth=28, mlp_ratio=4.0,
                      spatial_mlp_ratio=4.0, use_bias=False, matrix_block="matrix", flatten_matrix_rope=False, matrix_multi_token=False)
            if s128:  # @FacMatDiT/S-64-1; facmat-s128-1 / facmat-s128-8: S-1-1 / S-8-1 (train_dfot_facmat-s-{1,8}-1-bias)
                bb.update(embed_row_dim=384, depth=6, num_heads=12, num_row_heads=6, use_bias=True)
                if a.model != "facmat-s128":
                    bb.update(embed_col_dim=int(a.model.rsplit("-", 1)[1]))
            if a.embed_col_dim:
                bb.update(embed_col_dim=a.embed_col_dim)
            if a.col_heads:
                bb.update(num_col_heads=a.col_heads)
            model = dfot_amd.DiT3D(dict(bb, use_fourier_noise_embedding=a.continuous), x_shape=x_shape, max_tokens=tokens, **ckw).cuda()
        else:
            bb = dict(name="dit3d", variant="full", pos_emb_type="rope_3d", patch_size=1, hidden_size=1152, depth=28, num_heads=16)
            model = dfot_amd.DiT3D(dict(bb, use_fourier_noise_embedding=a.continuous), x_shape=x_shape, max_tokens=tokens, **ckw).cuda()
        cfg = dfot_amd.SamplerConfig(x_shape=x_shape, max_tokens=10 if diff else tokens,
                                     diffusion=(dfot_amd.DiffusionConfig(sampling_timesteps=a.steps, is_continuous=True) if a.continuous else
                                                dfot_amd.DiffusionConfig(sampling_timesteps=a.steps, beta_schedule="cosine", is_continuous=False)),
                                     prediction_guidance=dict(name="vanilla", guidance_scale=1.5) if a.cond else {"name": "conditional"}, **skw)
        sampler = (dfot_amd.DifferenceDFoTVideoSampler if diff else dfot_amd.DFoTVideoSampler)(cfg, model, noise)
        xs = torch.randn(a.batch, tokens, *x_shape, generator=torch.Generator().manual_seed(a.seed))
        n_ctx = 2
    if a.ckpt:
        ignored = dfot_amd.load_reference_checkpoint(model, a.ckpt)
        print(f"loaded {a.ckpt} ({len(ignored)} non-backbone keys ignored)")
    else:
        model.init_random(seed=a.seed)
    if a.inputs:
        data = np.load(a.inputs)
        xs = torch.from_numpy(data["xs"]).float()
        if "conditions" in data.files:
            conds = torch.from_numpy(data["conditions"])
            conds = conds.float() if conds.is_floating_point() else conds.long()
    xs = xs.cuda()
    conds = None if conds is None else conds.cuda()
    titok_sd = dfot_amd.load_titok_checkpoint(a.titok_ckpt) if a.titok_ckpt else None
    if a.encode_titok:  # `_encode` of the reference: context frames (B, n_ctx, 3, 256, 256) in [0, 1] -> the posterior's mode, not rescaled
        enc = dfot_amd.TiTokEncoder(image_size=256, token_size=xs.shape[2], vit_enc_model_size="large", num_latent_tokens=xs.shape[4]).cuda()
        if titok_sd is not None:
            ignored = enc.load_reference_state_dict(titok_sd)
            print(f"loaded {a.titok_ckpt} ({len(ignored)} decoder keys ignored)")
        else:
            enc.init_random(seed=a.seed + 1)
        ctx = torch.rand(xs.shape[0], n_ctx, 3, 256, 256, generator=torch.Generator().manual_seed(300 + a.seed)).cuda()
        dfot_amd.encode_titok_frames(enc, ctx[:1, :1], vae_batch_size=1)   # packs the weights, loads the kernels
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        xs[:, :n_ctx] = dfot_amd.encode_titok_frames(enc, ctx, vae_batch_size=2)
        torch.cuda.synchronize()
        print(f"TiTok encode ({a.titok_ckpt or 'random weights'}): {tuple(ctx.shape)} -> {tuple(xs[:, :n_ctx].shape)} in "
              f"{(time.perf_counter() - t0) * 1e3:.1f} ms")
    dcae_sd = dfot_amd.load_dcae_checkpoint(a.dc_ae_ckpt) if a.dc_ae_ckpt else None
    if a.encode_dc_ae:  # `_encode` of the reference for MyAutoencoderDC: context frames in [0, 1] -> latents, scaling_factor not applied
        enc = dfot_amd.DCAEEncoder(**dfot_amd.dcae_config(a.dc_ae)).cuda()
        if dcae_sd is not None:
            ignored = enc.load_reference_state_dict(dcae_sd)
            print(f"loaded {a.dc_ae_ckpt} ({len(ignored)} decoder keys ignored)")
        else:
            enc.init_random(seed=a.seed + 1)
        size = xs.shape[-1] * enc.s_factor
        ctx = torch.rand(xs.shape[0], n_ctx, 3, size, size, generator=torch.Generator().manual_seed(300 + a.seed)).cuda()
        dfot_amd.encode_dcae_frames(enc, ctx[:1, :1], vae_batch_size=1)   # packs the weights, loads the kernels
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        xs[:, :n_ctx] = dfot_amd.encode_dcae_frames(enc, ctx, vae_batch_size=2)
        torch.cuda.synchronize()
        print(f"DC-AE {a.dc_ae} encode ({a.dc_ae_ckpt or 'random weights'}): {tuple(ctx.shape)} -> {tuple(xs[:, :n_ctx].shape)} in "
              f"{(time.perf_counter() - t0) * 1e3:.1f} ms")
    model.eval()  # (train() would draw the per-video dropout of a condition embedding)
    if a.attention_maps:
        steps = a.attention_steps if a.attention_steps else sorted({0, a.steps // 2, a.steps - 1})
        sampler.cfg.attention_map_steps = tuple(steps)  # the window that collects runs the eager step loop
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if a.model == "k600diff":
        out = sampler._sample_all_videos(xs, n_context_tokens=n_ctx, conditions=conds)["prediction"]
    else:
        out = sampler._predict_videos(xs, n_context_tokens=n_ctx, conditions=conds)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    gen_frames = (out.shape[1] - n_ctx) * out.shape[0]
    print(f"{a.model}: {tuple(out.shape)} in {dt:.2f} s  ({gen_frames / dt:.2f} generated frames/s, "
          f"{sampler.window_forwards} backbone forwards of one window)")
    if a.decode_image_vae:
        zc, lh, _ = out.shape[2:]
        if a.image_vae_ckpt:
            dd, sd = dfot_amd.load_diffusers_checkpoint(a.image_vae_ckpt)
            if dd["embed_dim"] != zc:
                raise SystemExit(f"--image-vae-ckpt: the VAE has {dd['embed_dim']} latent channels, the sampled latents {zc}")
            vae = dfot_amd.ImageVAEDecoder(**dd).cuda()
            vae.load_reference_state_dict(sd)
        else:
            vae = dfot_amd.ImageVAEDecoder(ch=128, out_ch=3, ch_mult=(1, 2, 4, 4), num_res_blocks=2, z_channels=zc, embed_dim=zc,
                                           resolution=8 * lh).cuda()
            vae.init_random(seed=a.seed)
        dfot_amd.decode_image_latents(vae, out[:1], vae_batch_size=1)   # packs the weights, loads the kernels
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames = dfot_amd.decode_image_latents(vae, out, vae_batch_size=2)
        torch.cuda.synchronize()
        print(f"ImageVAE decode ({a.image_vae_ckpt or 'random weights'}): {tuple(out.shape)} -> {tuple(frames.shape)} in {(time.perf_counter() - t0) * 1e3:.1f} ms"
              f"{'' if bool(torch.isfinite(frames).all()) else '  (NON-FINITE frames)'}")
    if a.decode_dc_ae:
        vae = dfot_amd.DCAEDecoder(**dfot_amd.dcae_config(a.dc_ae)).cuda()
        if dcae_sd is not None:
            ignored = vae.load_reference_state_dict(dcae_sd)
            print(f"loaded {a.dc_ae_ckpt} ({len(ignored)} encoder keys ignored)")
        else:
            vae.init_random(seed=a.seed)
        dfot_amd.decode_dcae_latents(vae, out[:1, :1], vae_batch_size=1)   # packs the weights, loads the kernels
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames = dfot_amd.decode_dcae_latents(vae, out, vae_batch_size=2)
        torch.cuda.synchronize()
        print(f"DC-AE {a.dc_ae} decode ({a.dc_ae_ckpt or 'random weights'}): {tuple(out.shape)} -> {tuple(frames.shape)} in "
              f"{(time.perf_counter() - t0) * 1e3:.1f} ms{'' if bool(torch.isfinite(frames).all()) else '  (NON-FINITE frames)'}")
    if a.decode_titok:
        vae = dfot_amd.TiTokDecoder(image_size=256, token_size=out.shape[2], vit_dec_model_size="large", num_latent_tokens=out.shape[4]).cuda()
        if titok_sd is not None:
            ignored = vae.load_reference_state_dict(titok_sd)
            print(f"loaded {a.titok_ckpt} ({len(ignored)} encoder keys ignored)")
        else:
            vae.init_random(seed=a.seed)
        dfot_amd.decode_titok_latents(vae, out[:1, :1], vae_batch_size=1)   # packs the weights, loads the kernels
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames = dfot_amd.decode_titok_latents(vae, out, vae_batch_size=2)
        torch.cuda.synchronize()
        print(f"TiTok decode ({a.titok_ckpt or 'random weights'}): {tuple(out.shape)} -> {tuple(frames.shape)} in {(time.perf_counter() - t0) * 1e3:.1f} ms")
    np.savez_compressed(a.out, out=out.cpu().numpy())
    if a.attention_maps:  # plotting is the caller's: the hook's picture of a block is its map summed over the heads
        maps = {f"{step}/{name}": t.cpu().numpy() for step, rec in sampler.attention_maps.items() for name, t in rec.items()}
        np.savez_compressed(a.attention_maps, **maps)
        print(f"attention maps of steps {sorted(sampler.attention_maps)} ({len(maps)} arrays) -> {a.attention_maps}")


if __name__ == "__main__":
    main()
