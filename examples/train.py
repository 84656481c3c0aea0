#!/usr/bin/env python3
"""Training loop with the MI355X engine, the way the reference's Lightning trainer drives `training_step`.

  python examples/train.py k600     [--ckpt K600.ckpt] [--steps 100] [--batch 8] [--save out.ckpt]
  python examples/train.py k600 --pixels [--vae-ckpt VideoVAE_K600.ckpt]                # online latents: frames -> VideoVAE encoder -> step
  python examples/train.py k600diff [--accumulate 2]                                  # the model bash/k600/*.sh train
  python examples/train.py facmat   [--xl] [--batch 8]                                # FacMatDiT (dit3d_factorized_matrix.yaml); --xl: XL-64-1, taichikl shape
  python examples/train.py facdit   [--xl] [--batch 8]                                # FacDiT (dit3d_factorized_attention.yaml); --xl: @DiT/XL widths, taichikl shape
  python examples/train.py facdit-s128 [--mlp] [--batch 16]                           # FacDiT-S at 64 patches per frame, the taichi res-128 recipes (4x16x16
                                                                                      # latents, patch 2, 16 frames); --mlp: spatial_mlp_ratio 4 (facdit-s-mlp)
  python examples/train.py facmat-s128 [--embed-col-dim 64|128] [--col-heads N] [--batch 16]   # FacMatDiT-S with use_bias at the same shape, the taichi res-128
                                                                                      # facmat-s-{64-1,64-4,64-16,128-1}-bias recipes (default S-64-1)
  python examples/train.py taichi1d [--xl] [--batch 8]                                # DiT1D (dit1d.yaml), frame-causal, 4x1x32 token latents; --xl: its stock widths, 16 frames
  python examples/train.py mcraft   [--b] [--batch 8]                                 # the Minecraft / dmlab DiT recipe (32x8x8 latents, patch 2, 16 frames,
                                                                                      # actions of dim 4, continuous); --b: @DiT/B, else width 384, depth 2
  python examples/train.py re10k    [--batch 8]                                       # RE10K UViT3DPose (BASELINE config 5), synthetic frames + poses
  python examples/train.py uvit3d   [--cond action:4] [--full] [--batch 2]            # pose-free UViT3D (u_vit3d.yaml); --full: its widths, 8 heads, 256 x 256
  python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 examples/train.py k600   # data parallel, one rank per GPU

Data are synthetic latents (no dataset offline), or with --pixels synthetic 17 x 128 x 128 frames encoded online the way the K600
configuration does it (latent.type: online: `_encode` + `_normalize_x` on every batch, data_mean / data_std of
configurations/dataset/kinetics_600.yaml); everything else is the reference's recipe: per-token noise levels from
`_get_training_noise_levels` (random_independent for @DiT/XL, random_uniform + variable context for bash/k600), fused-min-SNR
v-loss, AdamW lr 5e-5 / wd 0.01 / betas (0.9, 0.99), gradient clipping 1.0, gradients averaged over the ranks.
The saved file uses the reference's key names (`diffusion_model.model.*`) and loads into the reference or into the samplers here.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dfot_amd  # noqa: E402


# configurations/dataset/kinetics_600.yaml: per-channel statistics of the VideoVAE latents
K600_DATA_MEAN = [-0.284, 0.016, -0.728, -0.138, 0.941, -2.504, 0.147, -0.062, 0.833, 0.151, -0.627, 0.269, 0.268, -0.732, -1.598, 0.199]
K600_DATA_STD = [5.591, 5.257, 7.033, 6.401, 6.091, 11.233, 5.608, 7.5, 5.277, 5.46, 5.179, 6.8, 5.474, 5.111, 7.078, 5.024]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model", choices=["k600", "k600diff", "facmat", "facdit", "facdit-s128", "facmat-s128", "taichi1d", "re10k", "uvit3d", "mcraft"])
    ap.add_argument("--ckpt")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--accumulate", type=int, default=1)
    ap.add_argument("--lr", type=float, default=5e-5)
    ap.add_argument("--warmup-steps", type=int, default=10000, help="re10k: linear lr warm-up (constant_with_warmup, realestate10k_video_generation.yaml)")
    ap.add_argument("--save")
    ap.add_argument("--cond", help="k600 / k600diff: train with a synthetic external condition, 'action:DIM' (action:3) or 'label:CLASSES' (label:101)")
    ap.add_argument("--continuous", action="store_true",
                    help="k600 / k600diff: continuous diffusion as @diffusion/continuous (Fourier noise-level embedding, levels in [0, 1], cosine "
                         "training schedule shifted 0.125, sigmoid loss weighting)")
    ap.add_argument("--xl", action="store_true", help="facmat / facdit: @FacMatDiT/XL-64-1 / @DiT/XL widths at the taichikl shape (4x32x32 latents, "
                                                      "patch 2, 16 frames) instead of the tiny default (width 128, depth 2, 4x16x8 latents, 5 frames); "
                                                      "taichi1d: the dit1d.yaml widths (1152, depth 28, 16 heads) at 16 frames of 4x1x32 instead of "
                                                      "width 128, depth 2, 8 frames")
    ap.add_argument("--mlp", action="store_true", help="facdit-s128: spatial_mlp_ratio 4 (train_dfot_facdit-s-mlp_taichikl_16_res128_ru.sh) instead of "
                                                       "attention-only spatial blocks (train_dfot_facdit-s_taichikl_16_res128_ru.sh)")
    ap.add_argument("--embed-col-dim", type=int, default=64, choices=[64, 128],
                    help="facmat-s128: column width of the matrix token, @FacMatDiT/group_S/S-64-* or S-128-1 (narrower widths do not train)")
    ap.add_argument("--col-heads", type=int, default=1, help="facmat-s128: num_col_heads (1, 4 or 16 in the recipes; must divide the column width)")
    ap.add_argument("--b", action="store_true", help="mcraft: @DiT/B (hidden 768, depth 12, 12 heads) instead of the tiny default (hidden 384, depth 2, 6 heads)")
    ap.add_argument("--full", action="store_true", help="uvit3d: the widths, depths and dropouts of u_vit3d.yaml with num_heads 8 (its 4 heads give head "
                                                        "dim 256, which the attention kernels do not take) on 8 frames of 3 x 256 x 256, instead of the "
                                                        "tiny default (channels 128/128/128/256, 2 heads, one block per level, 8 frames of 3 x 64 x 64)")
    ap.add_argument("--pixels", action="store_true", help="k600 / k600diff: encode synthetic frames online with the VideoVAE encoder")
    ap.add_argument("--vae-ckpt", help="--pixels: reference VideoVAE checkpoint (vae.* keys); random encoder weights otherwise")
    a = ap.parse_args()
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", torch.cuda.current_device()))
    if a.model == "re10k":
        return train_re10k(a, rank, world)
    if a.model == "uvit3d":
        return train_uvit3d(a, rank, world)
    if a.model in ("facmat", "facdit", "facdit-s128", "facmat-s128", "taichi1d"):
        return train_factorized(a, rank, world)
    diff, mcraft = a.model == "k600diff", a.model == "mcraft"
    x_shape, tokens = ((32, 8, 8), 16) if mcraft else ((16, 16, 16), 5)
    if mcraft:  # dataset=minecraft / dmlab: actions of dim 4 with mask_first; @diffusion/continuous
        a.cond, a.continuous = a.cond or "action:4", True
    ctype, cnum, ckw = None, 0, {}
    if a.cond:
        ctype, cnum = a.cond.split(":")[0], int(a.cond.split(":")[1])
        ckw = dict(external_cond_type=ctype, external_cond_dim=cnum if ctype == "action" else 1,
                   external_cond_num_classes=cnum if ctype == "label" else None)
    gdrop = torch.Generator(device="cuda").manual_seed(3000 + rank)  # per-video dropout of the condition embedding
    if diff:
        cfg = dict(name="difference_dit3d", variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", merge_type="interleaved",
                   patch_size=1, embed_col_dim=64, embed_row_dim=1152, num_heads=12, num_col_heads=1, num_row_heads=16, depth=28,
                   mlp_ratio=4.0, spatial_mlp_ratio=4.0, use_bias=True, matrix_block="matrix")
        cfg["use_fourier_noise_embedding"] = a.continuous
        if a.cond:
            cfg["external_cond_dropout"] = 0.1
        init = dfot_amd.DifferenceDiT3D(cfg, x_shape=(16, 16, 16), max_tokens=5, **ckw)
        sampling = dfot_amd.TrainingNoise(noise_level="random_uniform", is_continuous=a.continuous, n_context_tokens=2,
                                          variable_context=dfot_amd.ContextTraining(enabled=True, prob=0.25, dropout=0.3))
    else:
        cfg = dict(name="dit3d", variant="full", pos_emb_type="rope_3d", patch_size=1, hidden_size=1152, depth=28, num_heads=16)
        if mcraft:  # patch 2 on 8x8 latents of 32 channels: a 128-wide patch vector, 16 patches per frame
            cfg.update(patch_size=2, **(dict(hidden_size=768, depth=12, num_heads=12) if a.b else dict(hidden_size=384, depth=2, num_heads=6)))
        cfg["use_fourier_noise_embedding"] = a.continuous
        if a.cond:
            cfg["external_cond_dropout"] = 0.1
        init = dfot_amd.DiT3D(cfg, x_shape=x_shape, max_tokens=tokens, **ckw)
        sampling = dfot_amd.TrainingNoise(noise_level="random_independent", is_continuous=a.continuous, n_context_tokens=2)
    trainer = dfot_amd.DiT3DTrainer(cfg, x_shape=x_shape, max_tokens=tokens, lr=a.lr,
                                    diffusion=dfot_amd.DiffusionConfig(is_continuous=True) if a.continuous else None, **ckw)
    if a.ckpt:
        dfot_amd.load_reference_checkpoint(trainer, a.ckpt)
    else:
        init.init_random(seed=0)  # the same on every rank
        trainer.load_state_dict({k: v.detach() for k, v in init.state_dict().items()})
    del init
    g = torch.Generator().manual_seed(1000 + rank)
    encoder = None
    if a.pixels:
        encoder = dfot_amd.VideoVAEEncoder(z_channels=16, embed_dim=16, resolution=128, temporal_length=17).cuda()
        if a.vae_ckpt:
            sd = torch.load(a.vae_ckpt, map_location="cpu", weights_only=False)
            encoder.load_reference_state_dict(sd.get("state_dict", sd))
        else:
            encoder.init_random(seed=0)
        gv = torch.Generator(device="cuda").manual_seed(2000 + rank)
    masks = torch.ones(a.batch, tokens, dtype=torch.bool)
    t0 = time.perf_counter()
    for step in range(a.steps):
        for _ in range(a.accumulate):
            if encoder is not None:   # on_after_batch_transfer with latent.type online: _encode (vae.batch_size 2) then _normalize_x
                videos = torch.rand(a.batch, 17, 3, 128, 128, device="cuda", generator=gv)
                frames = dfot_amd.encode_videos(encoder, videos, vae_batch_size=2, generator=gv, data_mean=K600_DATA_MEAN, data_std=K600_DATA_STD)
            else:
                frames = torch.randn(a.batch, tokens, *x_shape, generator=g)
            noise = torch.randn(a.batch, 2 * tokens if diff else tokens, *x_shape, generator=g)
            levels, loss_masks = sampling.sample(a.batch, tokens, masks, g, training=True)
            conds = None
            if ctype == "action":
                conds = torch.randn(a.batch, tokens, cnum, generator=g)
                conds[:, :1] = 0  # external_cond_processing: mask_first
            elif ctype == "label":
                conds = torch.randint(0, cnum, (a.batch, 1), generator=g)
            loss = (trainer.difference_loss_and_grads if diff else trainer.loss_and_grads)(frames, levels, noise, loss_masks, conditions=conds,
                                                                                           dropout_generator=gdrop)
            if a.accumulate > 1:
                trainer.accumulate()
        trainer.optimizer_step(world)
        if rank == 0 and (step % 5 == 0 or step == a.steps - 1):
            print(f"step {step:4d}  loss {float(loss.item()):.4f}  {(time.perf_counter() - t0) / (step + 1) * 1e3:.1f} ms/step", flush=True)
    if a.save and rank == 0:
        torch.save({"state_dict": {"diffusion_model.model." + k: v.cpu() for k, v in trainer.state_dict().items()}}, a.save)
        print("saved", a.save)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def train_factorized(a, rank, world):
    """DFoTVideo training of the two factorized DiT3D backbones, discrete diffusion, random_independent levels, fused-min-SNR v-loss:
    facmat (bash/taichikl/train_dfot_facmat-*): factorized matrix attention with the temporal RoPE, FacMatDiTTrainer;
    facdit (bash/taichikl/train_dfot_facdit-*): factorized attention, sinusoidal_factorized, FacDiTTrainer -- the baseline of the former;
    facdit-s128 (bash/taichikl/resolution_128/train_dfot_facdit-s[-mlp]_taichikl_16_res128_ru.sh): the same model at the @FacDiT/S widths
        (hidden 384, depth 6, 6 heads) on 4x16x16 latents with patch 2 -- 64 patches per frame, 16 frames -- with (--mlp) or without the spatial MLP;
    facmat-s128 (bash/taichikl/resolution_128/train_dfot_facmat-s-{64-1,64-4,64-16,128-1}-bias_taichikl_16_res128_ru.sh): FacMatDiT at the
        @FacMatDiT/group_S widths (embed_row_dim 384, 6 row heads, depth 6, 12 spatial heads) with use_bias at that shape; --embed-col-dim 64 | 128
        and --col-heads choose the rung;
    taichi1d (`backbone=dit1d`): the frame-causal DiT1D over the 4x1x32 TiTok-KL token latents, DiT1DTrainer (unconditioned)"""
    if a.continuous or a.pixels:
        raise SystemExit(f"{a.model} trains on synthetic latents under discrete diffusion")
    x_shape, tokens = ((4, 32, 32), 16) if a.xl else ((4, 16, 8), 5)
    backbone_cls = dfot_amd.DiT3D
    if a.model == "taichi1d":
        x_shape, tokens = (4, 1, 32), 16 if a.xl else 8
        cfg = dict(hidden_size=1152, depth=28, num_heads=16) if a.xl else dict(hidden_size=128, depth=2, num_heads=4)
        cfg.update(name="dit1d", mlp_ratio=4, learn_sigma=False, merge_mode="share_norm", causal_attn_mode="video_temporal_causal",
                   use_rotary_emb=False, qk_norm=False)
        trainer_cls, backbone_cls = dfot_amd.DiT1DTrainer, dfot_amd.DiT1D
        if a.cond:
            raise SystemExit("taichi1d: the DiT1D backbone is unconditioned")
    elif a.model == "facdit-s128":
        x_shape, tokens = (4, 16, 16), 16
        cfg = dict(name="dit3d", variant="factorized_attention", pos_emb_type="sinusoidal_factorized", patch_size=2, hidden_size=384, depth=6,
                   num_heads=6, mlp_ratio=4.0, spatial_mlp_ratio=4.0 if a.mlp else 0.0)
        trainer_cls = dfot_amd.FacDiTTrainer
    elif a.model == "facmat-s128":
        x_shape, tokens = (4, 16, 16), 16
        if a.embed_col_dim % a.col_heads:
            raise SystemExit(f"facmat-s128: --col-heads {a.col_heads} does not divide --embed-col-dim {a.embed_col_dim}")
        cfg = dict(name="dit3d", variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", use_temporal_rope=True, patch_size=2,
                   embed_col_dim=a.embed_col_dim, embed_row_dim=384, num_heads=12, num_col_heads=a.col_heads, num_row_heads=6, depth=6,
                   mlp_ratio=4.0, spatial_mlp_ratio=4.0, use_bias=True, matrix_block="matrix")
        trainer_cls = dfot_amd.FacMatDiTTrainer
    elif a.model == "facdit":
        cfg = dict(patch_size=2, hidden_size=1152, num_heads=16, depth=28) if a.xl else dict(patch_size=1, hidden_size=128, num_heads=4, depth=2)
        cfg.update(name="dit3d", variant="factorized_attention", pos_emb_type="sinusoidal_factorized", mlp_ratio=4.0, spatial_mlp_ratio=4.0)
        trainer_cls = dfot_amd.FacDiTTrainer
    else:
        if a.xl:
            cfg = dict(patch_size=2, embed_col_dim=64, embed_row_dim=1152, num_heads=16, num_col_heads=1, num_row_heads=16, depth=28)
        else:
            cfg = dict(patch_size=1, embed_col_dim=64, embed_row_dim=128, num_heads=4, num_col_heads=1, num_row_heads=4, depth=2)
        cfg.update(name="dit3d", variant="factorized_matrix_attention", pos_emb_type="sinusoidal_2d", use_temporal_rope=True, mlp_ratio=4.0,
                   spatial_mlp_ratio=4.0, use_bias=True, matrix_block="matrix")
        trainer_cls = dfot_amd.FacMatDiTTrainer
    ckw = {}
    if a.cond:
        ctype, cnum = a.cond.split(":")[0], int(a.cond.split(":")[1])
        if ctype != "action":
            raise SystemExit(f"{a.model}: --cond action:DIM")
        ckw = dict(external_cond_type="action", external_cond_dim=cnum)
        cfg["external_cond_dropout"] = 0.1
    # 64 patches per frame train on request: without the keyword the trainer refuses them as it always did
    tkw = dict(ckw, allow_p64=True) if a.model in ("facdit-s128", "facmat-s128") else ckw
    trainer = trainer_cls(cfg, x_shape=x_shape, max_tokens=tokens, lr=a.lr, loss_weighting=dict(strategy="fused_min_snr", cum_snr_decay=0.96), **tkw)
    if a.ckpt:
        dfot_amd.load_reference_checkpoint(trainer, a.ckpt)
    else:
        init = backbone_cls(cfg, x_shape=x_shape, max_tokens=tokens, **ckw)
        init.init_random(seed=0)  # the same on every rank
        trainer.load_state_dict({k: v.detach() for k, v in init.state_dict().items()})
        del init
    sampling = dfot_amd.TrainingNoise(noise_level="random_independent", is_continuous=False, n_context_tokens=2)
    g = torch.Generator().manual_seed(1000 + rank)
    gdrop = torch.Generator(device="cuda").manual_seed(3000 + rank)
    masks = torch.ones(a.batch, tokens, dtype=torch.bool)
    t0 = time.perf_counter()
    for step in range(a.steps):
        for _ in range(a.accumulate):
            frames = torch.randn(a.batch, tokens, *x_shape, generator=g)
            noise = torch.randn(a.batch, tokens, *x_shape, generator=g)
            levels, loss_masks = sampling.sample(a.batch, tokens, masks, g, training=True)
            conds = None
            if a.cond:
                conds = torch.randn(a.batch, tokens, cnum, generator=g)
                conds[:, :1] = 0  # external_cond_processing: mask_first
            loss = trainer.loss_and_grads(frames, levels, noise, loss_masks, conditions=conds, dropout_generator=gdrop)
            if a.accumulate > 1:
                trainer.accumulate()
        trainer.optimizer_step(world)
        if rank == 0 and (step % 5 == 0 or step == a.steps - 1):
            print(f"step {step:4d}  loss {float(loss.item()):.4f}  {(time.perf_counter() - t0) / (step + 1) * 1e3:.1f} ms/step", flush=True)
    if a.save and rank == 0:
        torch.save({"state_dict": {"diffusion_model.model." + k: v.cpu() for k, v in trainer.state_dict().items()}}, a.save)
        print("saved", a.save)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def train_re10k(a, rank, world):
    """DFoTVideoPose training on the op-by-op UViT3DPose driver: per-token independent continuous levels, sigmoid-weighted v-loss"""
    from bench import RE10K, synth_poses
    from dfot_amd import parallel
    from dfot_amd.training import lr_at_step
    from dfot_amd.uvit_train import UViT3DPoseTrainer
    dcfg = dfot_amd.DiffusionConfig()  # training schedule (cosine, shift 0.125), sigmoid loss weighting (bias -1), precond_scale 0.125
    init = dfot_amd.UViT3DPose(RE10K, x_shape=(3, 256, 256), max_tokens=8)
    if a.ckpt:
        dfot_amd.load_reference_checkpoint(init, a.ckpt)
    else:
        init.init_random(seed=0)
    trainer = UViT3DPoseTrainer({k: v.detach() for k, v in init.state_dict().items()}, dict(RE10K, resolution=256, max_tokens=8))
    del init
    sampling = dfot_amd.TrainingNoise(noise_level="random_independent", is_continuous=True, n_context_tokens=1)
    g = torch.Generator().manual_seed(1000 + rank)
    masks = torch.ones(a.batch, 8, dtype=torch.bool)
    t0 = time.perf_counter()
    for step in range(a.steps):
        frames = torch.randn(a.batch, 8, 3, 256, 256, generator=g)
        noise = torch.randn(a.batch, 8, 3, 256, 256, generator=g)
        cond = torch.ops.dfot.ray_encoding(synth_poses(a.batch, 8, 7 * step + rank), 256)
        levels, loss_masks = sampling.sample(a.batch, 8, masks, g, training=True)
        reducer = parallel.OverlappedGradReducer() if world > 1 else None   # gradient all-reduce overlapped with the backward
        loss = trainer.loss_and_grads(frames, cond, levels, noise, loss_masks, diffusion=dcfg, reducer=reducer)
        lr = lr_at_step(step, a.lr, "constant_with_warmup", a.warmup_steps)  # realestate10k_video_generation.yaml:19-22
        trainer.optimizer_step(lr=lr, world_size=world)
        if rank == 0 and (step % 5 == 0 or step == a.steps - 1):
            print(f"step {step:4d}  loss {float(loss.item()):.4f}  {(time.perf_counter() - t0) / (step + 1) * 1e3:.1f} ms/step", flush=True)
    if a.save and rank == 0:
        torch.save({"state_dict": {"diffusion_model.model." + k: v.cpu() for k, v in trainer.state_dict().items()}}, a.save)
        print("saved", a.save)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


UVIT3D_TINY = dict(channels=[128, 128, 128, 256], emb_channels=128, block_dropouts=[0.0, 0.0, 0.0, 0.0], num_updown_blocks=[1, 1, 1], num_mid_blocks=1,
                   num_heads=2)
UVIT3D_FULL = dict(channels=[128, 256, 512, 1024], emb_channels=1024, block_dropouts=[0.0, 0.0, 0.1, 0.1], num_updown_blocks=[3, 3, 3], num_mid_blocks=16,
                   num_heads=8)


def uvit3d_cfg(full: bool, cond_dim: int = 0):
    """(backbone configuration, frame resolution) of the uvit3d entry; shared with tools/bench_ops.py"""
    cfg = dict(UVIT3D_FULL if full else UVIT3D_TINY, name="u_vit3d", patch_size=2, pos_emb_type="rope", use_checkpointing=[False] * 4,
               block_types=["ResBlock", "ResBlock", "TransformerBlock", "TransformerBlock"], use_fourier_noise_embedding=True)
    if cond_dim:
        cfg["external_cond_dropout"] = 0.1
    return cfg, (256 if full else 64)


def train_uvit3d(a, rank, world):
    """DFoTVideo training of the pose-free U-ViT under continuous diffusion on the op-by-op UViT3DTrainer: unconditioned, or with a synthetic
    action sequence (--cond action:DIM, per-video dropout 0.1 of the action embedding)"""
    from dfot_amd import parallel
    cdim = 0
    if a.cond:
        ctype, cdim = a.cond.split(":")[0], int(a.cond.split(":")[1])
        if ctype != "action":
            raise SystemExit("uvit3d: --cond action:DIM")
    cfg, res = uvit3d_cfg(a.full, cdim)
    tokens = 8
    dcfg = dfot_amd.DiffusionConfig()  # training schedule (cosine, shift 0.125), sigmoid loss weighting (bias -1), precond_scale 0.125
    init = dfot_amd.UViT3D(cfg, x_shape=(3, res, res), max_tokens=tokens, external_cond_dim=cdim)
    if a.ckpt:
        dfot_amd.load_reference_checkpoint(init, a.ckpt)
    else:
        init.init_random(seed=0)  # the same on every rank
    trainer = dfot_amd.UViT3DTrainer({k: v.detach() for k, v in init.state_dict().items()},
                                     dict(cfg, resolution=res, max_tokens=tokens, in_channels=3, cond_dim=cdim))
    del init
    trainer.dropout_generator = torch.Generator(device="cuda").manual_seed(4000 + rank)  # block_dropouts of the MLP branches
    sampling = dfot_amd.TrainingNoise(noise_level="random_independent", is_continuous=True, n_context_tokens=1)
    g = torch.Generator().manual_seed(1000 + rank)
    masks = torch.ones(a.batch, tokens, dtype=torch.bool)
    t0 = time.perf_counter()
    for step in range(a.steps):
        for _ in range(a.accumulate):
            frames = torch.randn(a.batch, tokens, 3, res, res, generator=g)
            noise = torch.randn(a.batch, tokens, 3, res, res, generator=g)
            levels, loss_masks = sampling.sample(a.batch, tokens, masks, g, training=True)
            conds = drop = None
            if cdim:
                conds = torch.randn(a.batch, tokens, cdim, generator=g)
                conds[:, :1] = 0  # external_cond_processing: mask_first
                drop = torch.rand(a.batch, generator=g) < 0.1
            reducer = parallel.OverlappedGradReducer() if world > 1 and a.accumulate == 1 else None
            loss = trainer.loss_and_grads(frames, conds, levels, noise, loss_masks, diffusion=dcfg, cond_drop=drop, reducer=reducer)
            if a.accumulate > 1:
                trainer.accumulate()
        trainer.optimizer_step(lr=a.lr, world_size=world)
        if rank == 0 and (step % 5 == 0 or step == a.steps - 1):
            print(f"step {step:4d}  loss {float(loss.item()):.4f}  {(time.perf_counter() - t0) / (step + 1) * 1e3:.1f} ms/step", flush=True)
    if a.save and rank == 0:
        torch.save({"state_dict": {"diffusion_model.model." + k: v.cpu() for k, v in trainer.state_dict().items()}}, a.save)
        print("saved", a.save)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
