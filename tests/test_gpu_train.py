"""The training driver runs on the path bench.py measures (missing #3 / #5): `python -m video_vae_amd.train` replays one captured
hipGraph per (batch, frames) shape of the reference's curriculum (train/rl_nonadversarial.py:276-277,287-295,332), writes the periodic
sample clips (:337-343) and runs the per-epoch eval_step loop (:200-208,362-391)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), PYTHONUNBUFFERED="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, "-m", "video_vae_amd.train"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("flavour", ["rl", "model"])
def test_train_driver_replays_one_graph_per_curriculum_shape(dev, tmp_path, flavour):
    """Two epochs of the batch <-> frames curriculum (2 x 8 frames, then 1 x 16): each shape runs eagerly once, is captured, and every later
    step is a replay; sample clips of the reconstruction and the original land every 5 steps; two eval batches per epoch."""
    out = _run(["--small", "--size", "32", "--per_device_batch_size", "2", "--max_frames", "8", "--epochs", "2", "--steps", "12", "--flavour", flavour,
                "--log_every", "3", "--sample_every", "5", "--sample_dir", str(tmp_path), "--sample_ext", "npz", "--eval_steps", "2"])
    lines = out.splitlines()
    caps = [l for l in lines if l.startswith("captured the train step")]
    assert len(caps) == 2 and "(2, 8, 32, 32, 3)" in caps[0] and "(1, 16, 32, 32, 3)" in caps[1], out[-3000:]
    for epoch, (b, t) in enumerate([(2, 8), (1, 16)]):
        logged = [l for l in lines if l.startswith(f"Epoch {epoch}, Step")]
        assert logged and "mode = eager" in logged[0] and all("mode = hipgraph" in l for l in logged[1:]), logged
        assert all(f"effective_batch_size = {b}, effective_max_frames = {t}" in l for l in logged)
        assert sum(l.startswith(f"VALIDATION Epoch {epoch}, Step") for l in lines) == 2
        for i in (4, 9):
            for kind in ("latent", "original"):
                f = tmp_path / "train" / f"epoch{epoch}" / f"video_{i}_{kind}.npz"
                assert f.exists(), (f, os.listdir(tmp_path))
                frames = np.load(f)["frames"]
                assert frames.dtype == np.uint8 and frames.shape[1:] == (32, 32, 3) and 1 <= frames.shape[0] <= t
    # the loss is finite and logged with the reference's keys in every line
    keys = ("MSE", "kl_loss", "selection_loss") + (("rl_loss", "per_sample_MAE") if flavour == "rl" else ())
    for l in lines:
        if l.startswith("Epoch "):
            assert all(k + " = " in l for k in keys) and "nan" not in l.lower(), l
    summ = [l for l in lines if l.startswith("train summary:") and "hipgraph" in l]
    assert summ, out[-2000:]


def test_train_driver_eager_flag_never_captures(dev):
    out = _run(["--small", "--size", "32", "--per_device_batch_size", "2", "--max_frames", "8", "--steps", "6", "--eager", "--log_every", "2"])
    assert "captured the train step" not in out and "mode = hipgraph" not in out and "train summary:" in out


def test_capture_on_another_stream_than_the_eager_steps_raises(dev):
    """The one-stream rule as an exception (round 3's segfault in `python -m video_vae_amd.train`): an eager step on the
    default stream whose loss is still held pins every AccumulateGrad node to that stream; GraphedTrainStep -- which would capture on a
    fresh stream -- refuses instead of letting the autograd engine crash.  Dropping the pass, or handing the stream over, is accepted."""
    import gc
    import torch
    import video_vae_amd as V
    from video_vae_amd import loss as L, optim
    from video_vae_amd._lib import VvaeError
    from video_vae_amd.graph import GraphedTrainStep
    from test_gpu_model import TINY
    m = V.VideoVAE(rngs=V.Rngs(2), dtype=torch.bfloat16, **TINY).to(dev)
    opt = optim.Optimizer(m, 1e-4)
    video = torch.rand((2, 8, 32, 32, 3), device=dev).to(torch.bfloat16)
    mask = torch.ones((2, 8), device=dev)
    hw = 16
    loss, aux = L.loss_fn_plain(m, video, L.expand_mask(mask, hw), mask, V.Rngs(3), L.HPARAMS)
    opt.zero_grad()
    loss.backward()                                      # eager, on the default stream; `loss` keeps the pass's graph alive
    opt.update()
    with pytest.raises(VvaeError, match="One stream for the whole run"):
        GraphedTrainStep(m, opt, video, mask, L.HPARAMS, hw, V.Rngs(3), warmup=1)
    del loss, aux
    gc.collect()
    step = GraphedTrainStep(m, opt, video, mask, L.HPARAMS, hw, V.Rngs(3), warmup=1)       # nothing of the eager pass is left: fine
    l2, _ = step()
    assert torch.isfinite(l2)


@pytest.mark.parametrize("grad_dtype", ["f32", "bf16"])
def test_bench_under_torchrun_runs_the_rccl_staged_graph_path(dev, grad_dtype):
    """bench.py as the DRIVER launches it for N > 1 -- `python -m torch.distributed.run --nproc-per-node ... bench.py --gpus ...` -- with the one
    rank a one-GPU box allows: process group on RCCL ("nccl"), GradReducer attached, the step captured as 1 + 3 graphs with each stage's
    buckets all-reduced under the next (graph.py), finite loss.  Puts the data-parallel path's execution into the driver-side record
    (VERDICT r03 next #6); no scaling figure can come from one rank."""
    import json
    import socket
    import torch
    torch.cuda.empty_cache()                             # the child needs ~40 GB of the card this process has been caching on
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "1", "--force-ddp", "--steps", "3", "--warmup", "1", "--settle-seconds", "0", "--no-cpu-baseline",
           "--no-kernel-timing", "--grad-dtype", grad_dtype]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    line = [l for l in r.stdout.splitlines() if l.lstrip().startswith("{") and '"metric"' in l]
    assert len(line) == 1, r.stdout[-2000:]
    out = json.loads(line[0])
    assert out["rccl_ranks"] == 1 and out["n_gpus"] == 1 and out["grad_allreduce_dtype"] == grad_dtype
    assert out["value"] > 0 and out["ms_per_step"] > 0
    nodes = out["config"]["graph_nodes"]
    assert isinstance(nodes, list) and len(nodes) == 4 and all(set(c) == {"kernel"} for c in nodes), nodes          # 1 + 3 graphs, kernels only
    assert "4 hipgraphs" in out["config"]["launch_mode"]


def _bench_line(args, timeout=900):
    import json
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    line = [l for l in r.stdout.splitlines() if l.lstrip().startswith("{") and '"metric"' in l]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0])


def test_bench_plain_run_is_headline_only_and_full_adds_the_rest(dev, tmp_path):
    """A plain bench.py run prints the headline (and writes --dump-outputs) without the legs that take runs of their own; --full adds
    the per-launch HIP-event leg (roofline, kernels, conv_stack) and the `also` block (the CPU leg is a host test)."""
    import torch
    torch.cuda.empty_cache()                             # each child needs ~40 GB of the card this process has been caching on
    short = ["--steps", "2", "--warmup", "1", "--settle-seconds", "0"]
    moved = ("roofline", "roofline_step_dominant", "kernels", "conv_stack", "also", "cpu_baseline")
    plain = _bench_line(short + ["--dump-outputs", str(tmp_path)])
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["unit"] == "frames/s" and plain["higher_is_better"] is True
    assert plain["dtype"] == "bf16" and "hipgraph" in plain["config"]["launch_mode"]
    assert not any(k in plain for k in moved), sorted(plain)
    assert {"loss", "params", "grads"} <= {f[:-4] for f in os.listdir(tmp_path)}
    full = _bench_line(short + ["--full", "--no-cpu-baseline", "--also-steps", "1"])
    assert full["value"] > 0 and "cpu_baseline" not in full
    assert full["roofline"]["kernel"].startswith("conv3d") and full["roofline"]["avg_ms"] > 0 and full["kernels"] and full["conv_stack"]["ms_per_step"] > 0
    for name in ("rl_flavour", "c5_shape"):
        assert "error" not in full["also"][name] and full["also"][name]["finite"], full["also"]
