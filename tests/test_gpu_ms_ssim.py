"""GPU: multi-scale SSIM (vvae_ms_ssim_fwd through metrics.ms_ssim) against the float64 restatement of the definition for every dtype
pair and noise level, closed forms, an element-aligned operand, determinism (run to run and eager vs graph replay), masked frames that
are never read, frame_metrics beside it, and ``infer eval --ms-ssim`` in its three modes.

Shapes (B, T, H, W, C) with their scale counts (test_ms_ssim_host.CASES) and what each is there for:
  (1, 2, 44, 47, 3) m3     an odd width dropped twice (47 -> 23 -> 11), the last level exactly one valid position per channel, several
                           bands; levels 1 and 2 have row lengths that are no multiple of 4 (element accesses)
  (2, 3, 45, 44, 1) m3     odd height, one channel
  (1, 1, 22, 23, 4) m2     the smallest two-level frame, four channels
  (2, 2, 48, 48, 3) m3     every level 16-byte aligned: the vector pool
  (1, 1, 176, 176, 3) m5,  the default weights on the smallest frame they take, and on odd extents
  (1, 2, 181, 203, 4) m5
  (1, 1, 24, 700, 3) m2    level 0 in column strips (2100 values a row), level 1 not
  (1, 2, 24, 1400, 3) m2   both levels in strips
  (4, 16, 256, 256, 3) m5  the production shape (fp32 / bf16 only)

Bars: |ms_ssim - ref| <= 1e-4 and |terms - ref| <= 1e-4 against float64, the project's bar for SSIM (tests/test_gpu_metrics.py); every
test first asserts that every reference term is >= 0.02, so the powers are well-conditioned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_ms_ssim_host import C1, CASES, CASE_IDS, W5, assert_conditioned, case_reference, make_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 64
DTYPES = [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)]
NOISE = [0.02, 0.1, 0.3]


@pytest.mark.parametrize("a", NOISE)
@pytest.mark.parametrize("shape,scales", CASES, ids=CASE_IDS)
def test_kernels_vs_float64_definition(dev, shape, scales, a):
    from video_vae_amd.metrics import ms_ssim
    pairs = DTYPES[1:2] if shape[:2] == (4, 16) else DTYPES
    for dx, dy in pairs:
        x, y, mask, ref, ref_terms = case_reference(shape, scales, a, dx, dy)
        assert_conditioned(ref_terms, mask)
        ms, terms = ms_ssim(x.to(dev), y.to(dev), mask.to(dev), weights=W5[:scales], return_terms=True)
        torch.cuda.synchronize()
        assert ms.dtype == torch.float32 and ms.shape == shape[:2] and ms.is_cuda
        assert terms.dtype == torch.float32 and terms.shape == shape[:2] + (scales, shape[4])
        dead = (mask == 0).to(dev)
        assert torch.all(ms[dead] == 0) and torch.all(terms[dead] == 0)
        et = np.abs(terms.cpu().double().numpy() - ref_terms)
        em = np.abs(ms.cpu().double().numpy() - ref)
        print(f"{shape} m{scales} a={a} {dx}/{dy}: |ms - ref| {em.max():.2e}, |terms - ref| per level "
              f"{[float(f'{v:.2e}') for v in et.max(axis=(0, 1, 3))]}, least term {ref_terms[mask.numpy() != 0].min():.3f}")
        assert et.max() <= 1e-4, (dx, dy, et.max(axis=(0, 1, 3)))         # per level: which one is wrong
        assert em.max() <= 1e-4, (dx, dy)
        assert torch.equal(ms_ssim(x.to(dev), y.to(dev), mask.to(dev), weights=W5[:scales]), ms)


def test_constants_and_identical_operands(dev):
    from video_vae_amd.metrics import ms_ssim
    one = torch.ones(1, 1, device=dev)
    x, y = torch.full((1, 1, 44, 44, 3), 0.5, device=dev), torch.full((1, 1, 44, 44, 3), 0.25, device=dev)
    want = ((2 * 0.5 * 0.25 + C1) / (0.25 + 0.0625 + C1)) ** 0.3001
    ms, terms = ms_ssim(x, y, one, weights=W5[:3], return_terms=True)
    assert abs(float(ms) - want) <= 1e-5
    assert float((terms[0, 0, :2] - 1).abs().max()) <= 1e-5
    z, _, _ = make_pair((1, 1, 181, 203, 4), 0.1, seed=1)
    for dt in (torch.float32, torch.bfloat16):
        zz = z.to(dev).to(dt)
        ms, terms = ms_ssim(zz, zz.clone(), one, return_terms=True)
        assert abs(float(ms) - 1.0) <= 1e-5 and float((terms - 1).abs().max()) <= 1e-5


@pytest.mark.parametrize("shape,scales", [((2, 2, 48, 48, 3), 3), ((1, 2, 44, 47, 3), 3)])
def test_element_aligned_bf16_operand(dev, shape, scales):
    """A bf16 operand that starts one element into its storage (2-byte aligned): the same bits as its contiguous copy."""
    from video_vae_amd.metrics import ms_ssim
    x, y, mask = make_pair(shape, 0.1, seed=2)
    x, mask = x.to(dev), mask.to(dev)
    yb = y.to(dev).to(torch.bfloat16)
    store = torch.zeros(yb.numel() + 1, dtype=torch.bfloat16, device=dev)
    view = store[1:].view(shape)
    view.copy_(yb)
    assert view.is_contiguous() and view.data_ptr() % 4 == 2
    a = ms_ssim(x, yb, mask, weights=W5[:scales], return_terms=True)
    b = ms_ssim(x, view, mask, weights=W5[:scales], return_terms=True)
    c = ms_ssim(view, x, mask, weights=W5[:scales], return_terms=True)
    d = ms_ssim(yb, x, mask, weights=W5[:scales], return_terms=True)
    for u, v in list(zip(a, b)) + list(zip(c, d)):
        assert torch.equal(u, v)


def test_deterministic_and_graph_replay_bitwise(dev):
    from video_vae_amd.metrics import ms_ssim
    shape = (4, 16, 256, 256, 3)
    x, y, mask = (v.to(dev) for v in make_pair(shape, 0.1, seed=3))
    y = y.to(torch.bfloat16)
    x2, y2, _ = (v.to(dev) for v in make_pair(shape, 0.3, seed=4))
    y2 = y2.to(torch.bfloat16)
    a = ms_ssim(x, y, mask, return_terms=True)
    b = ms_ssim(x, y, mask, return_terms=True)
    a2 = ms_ssim(x2, y2, mask, return_terms=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert not torch.equal(a[0], a2[0])
    sx, sy = x.clone(), y.clone()                      # the graph's static operands, rewritten between replays
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ms_ssim(sx, sy, mask, return_terms=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = ms_ssim(sx, sy, mask, return_terms=True)
    for (nx, ny), want in (((x, y), a), ((x2, y2), a2), ((x, y), a)):
        sx.copy_(nx)
        sy.copy_(ny)
        g.replay()
        torch.cuda.synchronize()
        for u, v in zip(out, want):
            assert torch.equal(u, v)


@pytest.mark.parametrize("shape,scales", [((2, 3, 45, 44, 1), 3), ((1, 2, 24, 1400, 3), 2), ((2, 2, 48, 48, 3), 3)])
def test_masked_frames_are_never_read(dev, shape, scales):
    from video_vae_amd.metrics import ms_ssim
    x, y, mask = (v.to(dev) for v in make_pair(shape, 0.1, seed=5))
    assert int((mask == 0).sum()) >= 1
    a = ms_ssim(x, y, mask, weights=W5[:scales], return_terms=True)
    dead = mask == 0
    x2, y2 = x.clone(), y.clone()
    x2[dead] = float("nan")
    y2[dead] = 1e30
    b = ms_ssim(x2, y2, mask, weights=W5[:scales], return_terms=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v) and torch.all(torch.isfinite(v))
        assert torch.all(v[dead] == 0) and torch.all(v[~dead] > 0)


def test_frame_metrics_beside_ms_ssim(dev):
    from video_vae_amd.metrics import frame_metrics, ms_ssim
    x, y, mask = (v.to(dev) for v in make_pair((2, 3, 176, 180, 3), 0.1, seed=6))
    y = y.to(torch.bfloat16)
    alone = frame_metrics(x, y, mask)
    ms_ssim(x, y, mask)
    beside = frame_metrics(x, y, mask)
    ms_ssim(x, y, mask)
    torch.cuda.synchronize()
    for u, v in zip(alone, beside):
        assert torch.equal(u, v)


def test_unsupported_gpu_shape_raises(dev):
    from video_vae_amd import ops
    from video_vae_amd._lib import VvaeError
    x = torch.rand((1, 1, 175, 176, 3), device=dev)
    one = torch.ones(1, 1, device=dev)
    with pytest.raises(VvaeError):
        ops.ms_ssim(x, x, one)
    with pytest.raises(VvaeError):
        ops.ms_ssim(x[:, :, :43, :44], x[:, :, :43, :44], one, weights=W5[:3])
    with pytest.raises(VvaeError):
        ops.ms_ssim(x, x, one, weights=W5 + (0.1,))
    assert ops.ms_ssim(x[:, :, :44, :44], x[:, :, :44, :44], one, weights=W5[:3])[1] is None


# ------------------------------------------------------------------------------------------------ infer eval --ms-ssim
def _small(seed):
    import video_vae_amd as V
    from video_vae_amd import rl_model
    from video_vae_amd.infer import model_config
    return rl_model.VideoVAE(rngs=V.Rngs(seed), **model_config(SMALL, True))


def _ramp_clip(rng, n, h, w):
    """A moving ramp with a little noise, uint8 (n, h, w, 3): structured content.  (On white-noise clips an untrained model's
    reconstruction has a negative mean CS at some level of some frames, which max(., 0) turns into an MS-SSIM of exactly 0.)"""
    yy, xx = np.mgrid[0:h, 0:w]
    v = 40 + 2 * xx[None, :, :, None] + yy[None, :, :, None] + 5 * np.arange(n)[:, None, None, None] + rng.integers(-3, 4, size=(n, h, w, 3))
    return np.clip(v, 0, 255).astype(np.uint8)


def _eval(tmp_path, data, out, extra):
    cmd = ["timeout", "-k", "10", "180", sys.executable, "-m", "video_vae_amd.infer", "eval", "--model_path", str(tmp_path / "ckpt"),
           "--data", str(data), "--size", str(SMALL), "--frames", "8", "--batch", "2", "--small", "--threshold", "--per-frame",
           "--out", str(out)] + extra
    return subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)


def _has_key(node, key):
    if isinstance(node, dict):
        return key in node or any(_has_key(v, key) for v in node.values())
    if isinstance(node, list):
        return any(_has_key(v, key) for v in node)
    return False


def test_cli_eval_ms_ssim(dev, tmp_path):
    """infer eval --ms-ssim --ms-ssim-scales 3 on two clips (12 and 5 frames): per_frame["ms_ssim"] equals metrics.ms_ssim of an in-process
    replayed "evaluate" graph's (video, recon, mask) over the same batches, value for value; the clip and dataset means are
    frame-weighted; the same command without the flags writes no ms_ssim key; five scales at --size 64 exit with status 2."""
    from video_vae_amd import model_loader
    from video_vae_amd.infer import GraphedInference, InferenceWeights, _batches, clip_windows
    from video_vae_amd.metrics import ms_ssim
    rng = np.random.default_rng(3)
    data = tmp_path / "data"
    data.mkdir()
    np.save(data / "long.npy", _ramp_clip(rng, 12, 40, 48))
    np.save(data / "short.npy", _ramp_clip(rng, 5, 40, 48))
    model = _small(9)
    model_loader.save_checkpoint(model, None, str(tmp_path / "ckpt"))
    r = _eval(tmp_path, data, tmp_path / "five.json", ["--ms-ssim"])
    assert r.returncode == 2 and "176x176" in r.stderr and not (tmp_path / "five.json").exists(), r.stderr[-3000:]
    r = _eval(tmp_path, data, tmp_path / "plain.json", [])
    assert r.returncode == 0, r.stderr[-3000:]
    assert not _has_key(json.loads((tmp_path / "plain.json").read_text()), "ms_ssim")
    assert not _has_key(json.loads((tmp_path / "plain.json").read_text()), "ms_ssim_scales")
    r = _eval(tmp_path, data, tmp_path / "m.json", ["--ms-ssim", "--ms-ssim-scales", "3"])
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads((tmp_path / "m.json").read_text())
    plain = json.loads((tmp_path / "plain.json").read_text())
    assert res["config"]["ms_ssim"] is True and res["config"]["ms_ssim_scales"] == 3 and res["dataset"]["frames"] == 17
    clips = {c["name"]: c for c in res["clips"]}
    for c in plain["clips"]:                               # everything that was there stays what it was
        for k in c:
            assert clips[c["name"]][k] == c[k] or k == "per_frame"
        for k in c["per_frame"]:
            assert clips[c["name"]]["per_frame"][k] == c["per_frame"][k]
    m = model.to(dev)
    gi = GraphedInference(m, InferenceWeights(m), 2, 8, "evaluate")
    for name in ("long", "short"):
        per = []
        for grp, real in _batches(clip_windows(str(data / f"{name}.npy"), SMALL, 8), 2):
            grp = grp + [grp[-1]] * (2 - real)
            video = torch.from_numpy(np.stack([g[0] for g in grp])).to(dev).float() / 255.0
            mask = torch.from_numpy(np.stack([g[1] for g in grp])).to(dev)
            recon, _, _ = gi(video, mask)
            ms = ms_ssim(video, recon, mask, weights=W5[:3])
            for i in range(real):
                per += ms[i, :grp[i][2]].double().cpu().tolist()
        e = clips[name]
        assert len(per) == e["frames"] and e["per_frame"]["ms_ssim"] == per, name
        assert all(0.0 <= v <= 1.0 for v in per) and 0.0 < e["ms_ssim"] <= 1.0
        assert abs(e["ms_ssim"] - float(np.mean(per))) <= 1e-9
    n = sum(c["frames"] for c in res["clips"])
    assert abs(res["dataset"]["ms_ssim"] - sum(c["ms_ssim"] * c["frames"] for c in res["clips"]) / n) <= 1e-9


def test_cli_eval_ms_ssim_tiled_and_windowed(dev, tmp_path):
    """--tile --overlap 8 on a 40 x 80 clip (two scales: 40 >> 2 is below the window, and three scales exit with status 2 there) and
    --temporal-overlap 2 at three scales: a finite ms_ssim in (0, 1] per clip, the mean of its frames' values."""
    from video_vae_amd import model_loader
    rng = np.random.default_rng(4)
    data = tmp_path / "data"
    data.mkdir()
    np.save(data / "wide.npy", _ramp_clip(rng, 10, 40, 80))
    model_loader.save_checkpoint(_small(9), None, str(tmp_path / "ckpt"))
    runs = {"tile": ["--tile", "--overlap", "8", "--ms-ssim", "--ms-ssim-scales", "2"],
            "windows": ["--temporal-overlap", "2", "--ms-ssim", "--ms-ssim-scales", "3"]}
    for name, extra in runs.items():
        out = tmp_path / f"{name}.json"
        r = _eval(tmp_path, data, out, extra)
        assert r.returncode == 0, (name, r.stderr[-3000:])
        res = json.loads(out.read_text())
        assert res["config"]["ms_ssim"] is True and res["config"]["ms_ssim_scales"] == int(extra[-1])
        for c in res["clips"]:
            assert c["frames"] == 10 and len(c["per_frame"]["ms_ssim"]) == 10
            assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in c["per_frame"]["ms_ssim"])
            assert np.isfinite(c["ms_ssim"]) and 0.0 < c["ms_ssim"] <= 1.0
            assert abs(c["ms_ssim"] - float(np.mean(c["per_frame"]["ms_ssim"]))) <= 1e-9
        assert abs(res["dataset"]["ms_ssim"] - res["clips"][0]["ms_ssim"]) <= 1e-9
    r = _eval(tmp_path, data, tmp_path / "small.json", ["--tile", "--overlap", "8", "--ms-ssim", "--ms-ssim-scales", "3"])
    assert r.returncode == 2 and "44x44" in r.stderr and not (tmp_path / "small.json").exists(), r.stderr[-3000:]
