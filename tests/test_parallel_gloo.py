"""world_size-2 gloo test (CPU) of the window sharding used for the 200-frame plan: round-robin shards + one
all-gather per stage reproduce the serial result exactly, including the ragged case (odd window counts) and the
case of more ranks than windows."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _window_result(ids):
    # stand-in for one sampled window: deterministic function of the window id only
    if not ids:
        return torch.zeros(0, 8, 3, 4, 4)
    return torch.stack([torch.full((8, 3, 4, 4), float(i)) + torch.arange(8).view(8, 1, 1, 1) * 0.01 for i in ids])


def _worker(rank, world, port, counts, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dfot_amd import parallel
    ok = True
    for n in counts:
        out = parallel.run_sharded(n, _window_result, max_batch=4)
        ref = _window_result(list(range(n)))
        ok = ok and torch.equal(out, ref)
    q.put((rank, ok))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sharded_windows_equal_serial_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, [11, 35, 1, 2], q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60)
    assert all(ok for _, ok in res), res


def test_shard_assignment_covers_every_window_once():
    from dfot_amd import parallel
    for n in (1, 2, 11, 35, 48):
        for world in (1, 2, 4, 8):
            ids = sorted(i for r in range(world) for i in parallel.shard_windows(n, world, r))
            assert ids == list(range(n))
            assert max(len(parallel.shard_windows(n, world, r)) for r in range(world)) == -(-n // world)


def _interp_worker(rank, world, port, q):
    """Runs the sampler's REAL _interpolate_videos control flow (planner, batching, sharding, gather, write-back) with
    the device step replaced by a deterministic stub, sharded over 2 gloo ranks, and compares with the serial run."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import dfot_amd
    from dfot_amd import sampler as smp

    class Stub(smp.DFoTVideoPoseSampler):
        def __init__(self, cfg):
            self.cfg, self.max_tokens, self.x_shape, self.timesteps = cfg, cfg.max_tokens, tuple(cfg.x_shape), 1000
            self.noise_fn, self.shard_windows, self.calls = None, False, 0
            self.device = "cpu"  # the stub never touches the GPU

        def _sample_sequence(self, batch_size, length=None, context=None, context_mask=None, conditions=None,
                             history_guidance=None, **_):
            self.calls += batch_size
            known = (context_mask >= 1).view(batch_size, -1, 1, 1, 1).float()
            fill = conditions[..., 0].view(batch_size, -1, 1, 1, 1).expand_as(context)  # depends on the window only
            return context * known + (1 - known) * fill, None

    cfg = dfot_amd.SamplerConfig(x_shape=(3, 4, 4), interpolation_guidance=dict(name="vanilla", guidance_scale=1.5),
                                 interpolation_max_batch_size=4)
    n = 200
    xs = torch.arange(n, dtype=torch.float32).view(1, n, 1, 1, 1).expand(1, n, 3, 4, 4).contiguous()
    known = torch.zeros(1, n, dtype=torch.bool)
    keys = torch.linspace(0, n - 1, 12).round().long()
    known[:, keys] = True
    conds = torch.arange(n, dtype=torch.float32).view(1, n, 1).expand(1, n, 16).contiguous() + 0.5
    serial = Stub(cfg)
    ref = serial._interpolate_videos(xs, known, conds)
    sharded = Stub(cfg)
    sharded.shard_windows = True
    out = sharded._interpolate_videos(xs, known, conds)
    q.put((rank, bool(torch.equal(out, ref)), serial.calls, sharded.calls))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sharded_interpolation_control_flow_equals_serial_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_interp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60)
    assert all(ok for _, ok, _, _ in res), res
    # 11 + 35 windows in total; each rank samples about half of them when sharded
    assert all(serial == 46 for _, _, serial, _ in res), res
    assert sorted(sh for _, _, _, sh in res) == [22, 24], res  # 11 -> 6+5 and 35 -> 18+17 windows


def _grad_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dfot_amd import parallel
    n = 1000 + 37
    g = torch.Generator().manual_seed(5)
    base = torch.randn(world, n, generator=g)       # every rank builds all shards, keeps its own
    flat = base[rank].clone()
    parallel.allreduce_mean_(flat, bucket_numel=256)  # several ragged buckets
    q.put((rank, bool(torch.allclose(flat, base.mean(0), atol=1e-6))))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_flat_gradient_allreduce_mean_world2():
    """the data-parallel training exchange: one flat gradient buffer, bucketed async all-reduce, mean over ranks"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_grad_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60)
    assert all(ok for _, ok in res), res


def _overlap_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dfot_amd import parallel
    g = torch.Generator().manual_seed(11)
    sizes = [37, 1000, 4, 512, 129, 64]
    all_grads = [[torch.randn(n, generator=g) for n in sizes] for _ in range(world)]  # every rank builds all, keeps its own
    flat = torch.zeros(sum(sizes))
    red = parallel.OverlappedGradReducer(bucket_numel=600)   # several ragged buckets, flushed while "the backward" goes on
    off = 0
    for gr in all_grads[rank]:
        red.add(flat[off: off + gr.numel()], gr)
        off += gr.numel()
    red.finish()
    ref = torch.cat([torch.stack([all_grads[r][i] for r in range(world)]).mean(0) for i in range(len(sizes))])
    whole = torch.cat(all_grads[rank]).clone()
    parallel.allreduce_mean_(whole, bucket_numel=256)
    # branch exchange: rank r evaluated branch r of 3 samples
    v_local = torch.full((3, 8, 2), float(rank)) + torch.arange(3).view(3, 1, 1) * 10
    v = parallel.exchange_branches(v_local, nfe=2)
    ok_v = v.shape == (6, 8, 2) and all(float(v[b * 2 + h, 0, 0]) == h + 10 * b for b in range(3) for h in range(2))
    q.put((rank, bool(torch.allclose(flat, ref, atol=1e-6)), bool(torch.equal(flat, whole)), ok_v))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_overlapped_gradient_reducer_and_branch_exchange_world2():
    """gradients handed over piecewise during the backward and all-reduced per bucket == the one-shot flat all-reduce (bit for bit);
    the History-Guidance branch exchange returns rows in the sampler's (sample, branch) order"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_overlap_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60)
    assert all(a and b and c for _, a, b, c in res), res


def _branch_group_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dfot_amd import parallel
    nfe = 2
    divides = world % nfe == 0
    ok = True
    if divides:
        parallel.branch_group(nfe)  # every rank of the world enters dist.new_group
        # rank r evaluated branch r % 2 of 3 samples; the value also carries the pair id to show nothing crosses pairs
        v_local = torch.full((3, 8, 2), float(rank % 2) + 100.0 * (rank // 2)) + torch.arange(3).view(3, 1, 1) * 10
        v = parallel.exchange_branches(v_local, nfe=2)
        ok = v.shape == (6, 8, 2) and all(float(v[b * 2 + h, 0, 0]) == h + 10 * b + 100.0 * (rank // 2) for b in range(3) for h in range(2))
    else:
        try:  # three ranks do not divide into pairs: refused on every rank (the sampler then runs the step unsplit everywhere)
            parallel.branch_group(nfe)
            ok = False
        except ValueError:
            pass
    # in-place range reducer: out-of-order hand-over, ranges merge, result == the one-shot flat all-reduce
    g = torch.Generator().manual_seed(3)
    sizes = [40, 300, 8, 700, 129]
    all_grads = [[torch.randn(n, generator=g) for n in sizes] for _ in range(world)]
    offs = [sum(sizes[:i]) for i in range(len(sizes))]
    flat = torch.zeros(sum(sizes))
    red = parallel.OverlappedGradReducer(bucket_numel=600, flat=flat)
    for i in (4, 3, 0, 2, 1):   # the backward hands the deepest parameters over first
        red.add(flat[offs[i]: offs[i] + sizes[i]], all_grads[rank][i])
    red.finish()
    whole = torch.cat(all_grads[rank]).clone()
    parallel.allreduce_mean_(whole, bucket_numel=1 << 20)
    # (three ranks: a ring's per-element summation order depends on how the buffer is cut, so close, not bit-equal; two ranks: bit-equal above)
    q.put((rank, divides, ok, bool(torch.allclose(flat, whole, atol=1e-6)), red.calls))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [3, 4])
def test_branch_groups_are_pairs_and_ranges_reduce_in_place(world):
    """two History-Guidance branches: four ranks form two pairs that exchange only inside the pair; three ranks do not divide into
    pairs and the grouping is refused on every rank (no leftover rank with another model batch, dist.new_group entered by all
    ranks or by none); the gradient reducer all-reduces merged ranges of the flat buffer in place"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_branch_group_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(60)
    assert [m for _, m, _, _, _ in res] == [world % 2 == 0] * world, res
    assert all(ok and same for _, _, ok, same, _ in res), res
    assert all(1 <= calls <= 3 for *_, calls in res), res


def _sampler_branch_worker(rank, world, port, q):
    """the SAMPLER's own branch-parallel path (dry run: host plumbing, gloo): replicated key-frame windows of a short rollout"""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import dfot_amd
    from dfot_amd import parallel
    cfg = dfot_amd.SamplerConfig(x_shape=(3, 16, 16), diffusion=dfot_amd.DiffusionConfig(sampling_timesteps=3),
                                 prediction_guidance=dict(name="vanilla", guidance_scale=2.0), keyframe_density=0.25,
                                 interpolation_guidance=dict(name="vanilla", guidance_scale=1.5), interpolation_max_batch_size=2)
    samp = dfot_amd.DFoTVideoPoseSampler(cfg, backbone=None, noise_fn=parallel.WindowKeyedNoise(5, device="cpu"))
    samp.device, samp.dry_run, samp.branch_parallel, samp.shard_windows = "cpu", True, True, True
    out = samp._predict_videos(torch.zeros(1, 40, 3, 16, 16), n_context_tokens=1, conditions=None)
    ref = out.clone()
    dist.broadcast(ref, 0)
    q.put((rank, getattr(samp, "branch_exchanges", 0), bool(torch.equal(ref, out)), samp.window_forwards))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])
def test_sampler_branch_parallel_every_rank_same_path(world):
    """through the sampler itself.  world 2 / nfe 2: every key-frame step exchanges branches inside the pair.
    world 3 / nfe 2: NO rank splits (all three evaluate both branches, the same model batch everywhere) and nobody is left outside a
    collective -- the run finishes, windows are still sharded and all-gathered, all ranks end with the same rollout."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sampler_branch_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=200) for _ in procs)
    for p in procs:
        p.join(60)
    ex = [e for _, e, _, _ in res]
    assert all(same for _, _, same, _ in res), res
    assert len(set(ex)) == 1 and (ex[0] > 0) == (world % 2 == 0), res


def test_branch_parallel_needs_rank_independent_noise(monkeypatch):
    """with the default per-rank torch.randn noise the gathered v would mix branches of different states -- refused"""
    import dfot_amd
    from dfot_amd import parallel
    cfg = dfot_amd.SamplerConfig(x_shape=(3, 32, 32), diffusion=dfot_amd.DiffusionConfig(sampling_timesteps=2))
    samp = dfot_amd.DFoTVideoPoseSampler(cfg, backbone=None, noise_fn=lambda tag, shape: torch.zeros(shape))
    samp.device, samp.dry_run, samp.branch_parallel = "cpu", True, True
    monkeypatch.setattr(parallel, "world_info", lambda group=None: (2, 0))
    with pytest.raises(ValueError, match="rank-independent noise"):
        samp._predict_videos(torch.zeros(1, 8, 3, 32, 32), n_context_tokens=1, conditions=None)


@pytest.mark.timeout(600)
def test_bench_gpus_flag_starts_the_ranks():
    """VERDICT r2 missing #1: `python bench.py --gpus 2` without a launcher starts two ranks itself (fresh child processes with RANK /
    WORLD_SIZE / MASTER_* set) and prints rank 0's line with "n_gpus": 2.  Run under the `--dry-run` switch (gloo, CPU, nothing
    launched): the 200-frame plan is sharded over the two ranks, the key-frame windows take the History-Guidance branch-split path,
    the finished windows are all-gathered per plan stage and both ranks end with the same rollout."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "200f", "--res", "64", "--sampling-steps", "2",
                        "--dry-run", "--steps", "1", "--warmup", "0"], capture_output=True, text=True, timeout=500, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 1
    line = rows[0]
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["ranks_bit_identical"] is True
    assert line["config"]["frames_per_step"] == 199 and line["sampler_mode"].startswith("dry-run")
    assert line["rccl_ranks"] == 2 and line["collective_backend"] == "gloo" and "keyframe_phase" in line
    # a rank that fails takes the job down with a non-zero exit code instead of hanging the others
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "k600", "--dry-run"], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode != 0


@pytest.mark.timeout(900)
def test_bench_driver_command_measures_the_sharded_workloads():
    """`bench.py --gpus N --full` with the DEFAULT workload.  Its line must carry, next to the weak-scaling 8f
    headline, the workloads whose N-rank form is not N replicas: `extra.200f` (sharded windows, branch split, ranks bit-identical)
    with n_gpus = N, and `extra.train_re10k` (here: marked skipped, the dry run has no device).  Rank processes are coordinators
    that never touch the GPU; headline and extras are fresh worker processes with their own rendezvous."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--res", "64", "--sampling-steps", "2", "--dry-run",
                        "--full", "--steps", "1", "--warmup", "0"], capture_output=True, text=True, timeout=800, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 1
    line = rows[0]
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["rccl_ranks"] == 2
    assert line["config"]["frames_per_step"] == 7 and abs(line["value"] * line["ms_per_step"] / 1e3 - 14) < 1e-6  # two videos
    ex = line["extra"]
    assert set(ex) == {"200f", "train_re10k"}
    assert ex["200f"]["n_gpus"] == 2 and ex["200f"]["rccl_ranks"] == 2 and ex["200f"]["ranks_bit_identical"] is True
    assert ex["200f"]["scaling"] == "strong" and "keyframe_phase" in ex["200f"]
    assert "skipped" in ex["train_re10k"]


@pytest.mark.timeout(600)
def test_bench_plain_run_is_the_headline_alone():
    """Without `--full` the default command does only what its headline needs: the rank processes ARE the 8f workers (no
    coordinator, no extras) and the line carries the headline fields but no `extra` and no `cpu_baseline`."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--res", "64", "--sampling-steps", "2", "--dry-run",
                        "--steps", "1", "--warmup", "0"], capture_output=True, text=True, timeout=500, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 1
    line = rows[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["rccl_ranks"] == 2 and line["steps"] == 1 and line["warmup"] == 0
    assert line["config"]["frames_per_step"] == 7 and abs(line["value"] * line["ms_per_step"] / 1e3 - 14) < 1e-6  # two videos
    assert "extra" not in line and "cpu_baseline" not in line
