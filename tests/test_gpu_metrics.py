"""GPU: the reconstruction-metrics kernel (vvae_recon_metrics_fwd through metrics.frame_metrics) against the float64 restatement of the
definition for every dtype pair, its determinism (run to run and eager vs graph replay), masked frames that are never read, the replayed
"evaluate" inference graph of both flavours against eager reconstruct + frame_metrics, and ``infer eval`` end to end."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_metrics_host import ref_metrics

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 64
SHAPES = [(1, 1, 11, 11, 3), (2, 5, 64, 64, 3), (3, 7, 37, 53, 3), (2, 3, 24, 40, 1), (4, 16, 256, 256, 3)]
DTYPES = [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)]


def _pair(shape, seed, dev):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g)
    y = x + 0.1 * torch.randn(shape, generator=g)
    b, t = shape[:2]
    mask = (torch.rand((b, t), generator=g) > 0.3).float()
    mask[0, 0] = 1
    if b > 1:
        mask[-1] = 0                                   # one clip without a valid frame
    return x.to(dev), y.to(dev), mask.to(dev)


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_kernel_vs_float64_definition(dev, shape):
    from video_vae_amd.metrics import frame_metrics
    x32, y32, mask = _pair(shape, sum(shape), dev)
    for dx, dy in DTYPES:
        x, y = x32.to(dx), y32.to(dy)
        fm = frame_metrics(x, y, mask)
        torch.cuda.synchronize()
        mse, psnr, ssim = ref_metrics(x.cpu(), y.cpu(), mask.cpu())
        valid = mask.cpu().numpy() != 0
        for got in fm:
            assert got.dtype == torch.float32 and got.shape == shape[:2] and got.is_cuda
            assert torch.all(got[mask == 0] == 0)
        assert np.abs(fm.ssim.cpu().double().numpy() - ssim)[valid].max() <= 1e-4, (dx, dy)
        assert np.abs(fm.psnr.cpu().double().numpy() - psnr)[valid].max() <= 1e-3, (dx, dy)
        np.testing.assert_allclose(fm.mse.cpu().double().numpy(), mse, rtol=1e-4, atol=1e-9)


def test_deterministic_and_graph_replay_bitwise(dev):
    from video_vae_amd.metrics import frame_metrics
    x, y, mask = _pair((4, 16, 256, 256, 3), 11, dev)
    y = y.to(torch.bfloat16)
    a = frame_metrics(x, y, mask)
    b = frame_metrics(x, y, mask)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        frame_metrics(x, y, mask)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = frame_metrics(x, y, mask)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        for u, v in zip(out, a):
            assert torch.equal(u, v)


def test_masked_frames_are_never_read(dev):
    from video_vae_amd.metrics import frame_metrics
    x, y, mask = _pair((3, 7, 37, 53, 3), 12, dev)
    a = frame_metrics(x, y, mask)
    dead = mask == 0
    x2, y2 = x.clone(), y.clone()
    x2[dead] = float("nan")
    y2[dead] = 1e30
    b = frame_metrics(x2, y2, mask)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
        assert torch.all(torch.isfinite(v))


def test_unsupported_gpu_shape_raises(dev):
    from video_vae_amd._lib import VvaeError
    from video_vae_amd.metrics import frame_metrics
    x = torch.rand((1, 1, 16, 1024, 3), device=dev)
    with pytest.raises(VvaeError):
        frame_metrics(x, x, torch.ones(1, 1, device=dev))


def test_every_output_bit_equals_the_recorded_parent(dev):
    """frame_metrics (every dtype pair, the one-strip limits, an operand off its 16-byte boundary), frame_metrics_wide, ms_ssim with its
    terms, plane_metrics and temporal_mse against tests/golden/metrics_parent_bits.npz, recorded on the GPU before the SSIM moment pass had
    one plan and one launch path (make_metrics_parent_bits.py): every member, bit for bit."""
    spec = importlib.util.spec_from_file_location("make_metrics_parent_bits", os.path.join(ROOT, "tests", "golden", "make_metrics_parent_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    got = mod.record(dev)
    with np.load(os.path.join(ROOT, "tests", "golden", "metrics_parent_bits.npz")) as want:
        assert sorted(got) == sorted(want.files) and len(got) > 200
        bad = [k for k in want.files
               if got[k].dtype != torch.from_numpy(want[k]).dtype or not torch.equal(got[k], torch.from_numpy(want[k]))]
    assert not bad, bad
    assert got["pm_sse"].dtype == torch.int64 and all(v.dtype == torch.float32 for k, v in got.items() if k != "pm_sse")
    for shape in mod.FW_SHAPES[:2]:                      # a shape frame_metrics takes: frame_metrics_wide gives its results
        for k in (k for k in got if k.startswith(f"fw_{mod.tag(shape)}_")):
            assert torch.equal(got[k], got["fm" + k[2:]]), k
    live = [k for k in got if k.endswith("_ssim") and "_masked" not in k]
    assert all(float(got[k].max()) > 0.1 for k in live) and all(not got[k].any() for k in got if "_masked" in k)


def _small(flavour, seed):
    import video_vae_amd as V
    from video_vae_amd import rl_model
    from video_vae_amd.infer import model_config
    cls = rl_model.VideoVAE if flavour == "rl" else V.VideoVAE
    return cls(rngs=V.Rngs(seed), **model_config(SMALL, True))


@pytest.mark.parametrize("flavour", ["model", "rl"])
def test_graphed_evaluate_equals_eager(dev, flavour):
    """"evaluate" replays (recon, FrameMetrics, selection) bitwise equal to eager reconstruct followed by frame_metrics; no memset node;
    clip_metrics' kept_fraction from the replayed selection.  rl: the threshold gate and explicit Bernoulli uniforms."""
    import video_vae_amd as V
    from video_vae_amd.infer import GraphedInference, InferenceWeights
    from video_vae_amd.metrics import frame_metrics, summarize
    b, t = 2, 8
    m = _small(flavour, 3).to(dev)
    w = InferenceWeights(m)
    g = torch.Generator().manual_seed(4)
    xs = [torch.rand((b, t, SMALL, SMALL, 3), generator=g).to(dev) for _ in range(2)]
    mk = [torch.ones(b, t, device=dev), torch.ones(b, t, device=dev)]
    mk[1][1, 5:] = 0
    runs = [(None, None)]
    if flavour == "rl":
        runs.append((V.Rngs(5), [torch.rand((b, t, 1, 1), generator=g).to(dev) for _ in range(2)]))
    for rngs, us in runs:
        gi = GraphedInference(m, w, b, t, "evaluate", rngs=rngs)
        assert gi.census is not None and gi.census.get("memset", 0) == 0, gi.census
        for i in range(2):
            noise = {"bernoulli_u": us[i]} if us is not None else None
            recon, fm, sel = gi(xs[i], mk[i], noise=noise)
            rg = None
            if us is not None:
                rg = V.Rngs(0)
                rg.inject("bernoulli_u", us[i])
            want_sel = m.encode(xs[i], mk[i], rg, want_log_variance=False).selection
            if us is not None:
                rg = V.Rngs(0)
                rg.inject("bernoulli_u", us[i])
            want = m.reconstruct(xs[i], mk[i], rg)
            want_fm = frame_metrics(xs[i], want, mk[i])
            assert torch.equal(recon, want) and torch.equal(sel, want_sel)
            for u, v in zip(fm, want_fm):
                assert torch.equal(u, v)
            assert torch.all(fm.ssim[mk[i] == 0] == 0) and torch.all(fm.psnr[mk[i] != 0] > 0)
            cm = summarize(fm, mk[i], sel)
            kept = (sel * mk[i]).sum(1) / mk[i].sum(1)
            assert torch.allclose(cm.kept_fraction, kept) and cm.frames.tolist() == mk[i].sum(1).long().tolist()
        del gi


def test_cli_eval_end_to_end(dev, tmp_path):
    """infer eval on a saved --small checkpoint and two clips (12 frames: two windows of 8; 5 frames: one short window): the JSON's per-clip
    and per-frame numbers equal those of an in-process replayed "evaluate" graph over the same windows and batches."""
    from video_vae_amd import model_loader
    from video_vae_amd.infer import GraphedInference, InferenceWeights, _batches, clip_windows
    rng = np.random.default_rng(3)
    data = tmp_path / "data"
    data.mkdir()
    np.save(data / "long.npy", rng.integers(0, 256, size=(12, 40, 48, 3), dtype=np.uint8))
    np.save(data / "short.npy", rng.integers(0, 256, size=(5, 40, 48, 3), dtype=np.uint8))
    model = _small("rl", 9)
    model_loader.save_checkpoint(model, None, str(tmp_path / "ckpt"))
    out = tmp_path / "m.json"
    cmd = ["timeout", "-k", "10", "180", sys.executable, "-m", "video_vae_amd.infer", "eval", "--model_path", str(tmp_path / "ckpt"),
           "--data", str(data), "--size", str(SMALL), "--frames", "8", "--batch", "2", "--small", "--threshold", "--per-frame",
           "--out", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1].startswith("eval: 2 clips, 17 frames")
    res = json.loads(out.read_text())
    assert res["config"]["flavour"] == "rl" and res["config"]["frames"] == 8 and res["dataset"]["frames"] == 17
    clips = {c["name"]: c for c in res["clips"]}
    assert {k: clips[k]["frames"] for k in clips} == {"long": 12, "short": 5}
    m = model.to(dev)
    gi = GraphedInference(m, InferenceWeights(m), 2, 8, "evaluate")
    for name in ("long", "short"):
        per = {"psnr": [], "ssim": [], "mse": [], "selection": []}
        for grp, real in _batches(clip_windows(str(data / f"{name}.npy"), SMALL, 8), 2):
            grp = grp + [grp[-1]] * (2 - real)
            video = torch.from_numpy(np.stack([g[0] for g in grp])).to(dev).float() / 255.0
            mask = torch.from_numpy(np.stack([g[1] for g in grp])).to(dev)
            _, fm, sel = gi(video, mask)
            for i in range(real):
                c = grp[i][2]
                for k, v in (("psnr", fm.psnr), ("ssim", fm.ssim), ("mse", fm.mse), ("selection", sel)):
                    per[k] += v[i, :c].double().cpu().tolist()
        e = clips[name]
        for k in ("psnr", "ssim", "mse"):
            assert e["per_frame"][k] == per[k], (name, k)
            assert abs(e[k] - float(np.mean(per[k]))) <= 1e-9 * max(1.0, abs(e[k])), (name, k)
        assert abs(e["kept_fraction"] - float(np.mean(per["selection"]))) <= 1e-12
    n = sum(c["frames"] for c in res["clips"])
    assert abs(res["dataset"]["psnr"] - sum(c["psnr"] * c["frames"] for c in res["clips"]) / n) < 1e-9
