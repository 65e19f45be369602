"""CPU: the reconstruction metrics (video_vae_amd.metrics) -- the ABI entries of the kernel, the composed framework-op path against a float64
numpy restatement of the definition, the properties every PSNR / SSIM has, masking and clip means, and the infer eval command line.  No HIP
compute runs here."""
import ctypes
import importlib.util
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------ the definition, restated in float64 numpy
def _taps():
    k = np.arange(11, dtype=np.float64) - 5
    g = np.exp(-k * k / (2 * 1.5 ** 2))
    return g / g.sum()


def ref_frame(x, y, clamp=True):
    """One frame pair (H, W, C) -> (mse, psnr, ssim), float64: Wang et al. 2004 with the 11-tap Gaussian (sigma 1.5) at valid positions,
    C1 = 0.01^2, C2 = 0.03^2, averaged over positions and channels (skimage's structural_similarity with gaussian_weights=True,
    use_sample_covariance=False, data_range=1)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if clamp:
        x, y = np.clip(x, 0, 1), np.clip(y, 0, 1)
    g = _taps()
    h, w = x.shape[:2]

    def filt(a):
        r = sum(g[k] * a[k:h - 10 + k] for k in range(11))
        return sum(g[k] * r[:, k:w - 10 + k] for k in range(11))
    ux, uy = filt(x), filt(y)
    vx, vy, vxy = filt(x * x) - ux * ux, filt(y * y) - uy * uy, filt(x * y) - ux * uy
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    s = (2 * ux * uy + c1) * (2 * vxy + c2) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    mse = float(np.mean((x - y) ** 2))
    return mse, 10 * math.log10(1 / max(mse, 1e-10)), float(s.mean())


def ref_metrics(video, recon, mask, clamp=True):
    """(B, T, H, W, C) pairs and a (B, T) mask -> float64 (mse, psnr, ssim) arrays (B, T), 0 on masked frames."""
    video = torch.as_tensor(video).float().numpy()
    recon = torch.as_tensor(recon).float().numpy()
    mask = np.asarray(torch.as_tensor(mask).float())
    out = np.zeros((3,) + mask.shape)
    for b in range(mask.shape[0]):
        for t in range(mask.shape[1]):
            if mask[b, t] != 0:
                out[:, b, t] = ref_frame(video[b, t], recon[b, t], clamp)
    return out


def pair(b, t, h, w, c, seed, noise=0.1):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((b, t, h, w, c), generator=g)
    y = x + noise * torch.randn((b, t, h, w, c), generator=g)         # some values leave [0, 1]: clamping matters
    return x, y


# ------------------------------------------------------------------------------ tests
def test_metrics_entries_declared_and_exported():
    from video_vae_amd._lib import parse_header, LIB_PATH
    protos = parse_header()
    want = {"vvae_recon_metrics_supported": (ctypes.c_int, 5), "vvae_recon_metrics_part_floats": (ctypes.c_size_t, 5),
            "vvae_recon_metrics_fwd": (ctypes.c_int, 16)}
    so = ctypes.CDLL(LIB_PATH)
    for name, (ret, nargs) in want.items():
        assert name in protos, name
        assert protos[name][0] is ret and len(protos[name][1]) == nargs, (name, protos[name])
        assert hasattr(so, name), name


def test_supported_shapes_and_scratch_size():
    from video_vae_amd._lib import lib
    l = lib()
    assert l.vvae_recon_metrics_supported(256, 256, 3, 0, 1) and l.vvae_recon_metrics_supported(11, 11, 1, 1, 1)
    assert l.vvae_recon_metrics_supported(37, 53, 4, 1, 0)
    assert not l.vvae_recon_metrics_supported(10, 64, 3, 0, 0) and not l.vvae_recon_metrics_supported(64, 10, 3, 0, 0)
    assert not l.vvae_recon_metrics_supported(64, 64, 5, 0, 0) and not l.vvae_recon_metrics_supported(64, 64, 3, 2, 0)
    assert not l.vvae_recon_metrics_supported(64, 1024, 3, 0, 0)
    n = l.vvae_recon_metrics_part_floats(4, 16, 256, 256, 3)
    assert n > 0 and n % (2 * 64) == 0
    assert l.vvae_recon_metrics_part_floats(4, 16, 8, 256, 3) == 0
    assert l.vvae_recon_metrics_fwd(None, 0, None, 0, None, None, None, None, None, 1, 1, 16, 16, 3, 1, None) == 1001


def test_plans_equal_the_recorded_ones_row_by_row():
    """Shapes taken and scratch sizes of the SSIM moment pass (both entries), MS-SSIM at 1 to 5 scales, the plane metrics and the
    temporal error, against tests/golden/metrics_plans.json (recorded before the moment pass had one planner; make_metrics_plans.py)."""
    spec = importlib.util.spec_from_file_location("make_metrics_plans", os.path.join(ROOT, "tests", "golden", "make_metrics_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(ROOT, "tests", "golden", "metrics_plans.json")) as fh:
        want = json.load(fh)
    assert want["columns"] == ["C", "H", "W", "B", "T"] + mod.COLUMNS
    got = mod.record()
    assert len(got) == len(want["rows"]) >= 200
    for g, w in zip(got, want["rows"]):
        assert g == w, dict(zip(want["columns"], zip(g, w)))
    taken = [r for r in want["rows"] if r[5]]
    assert any(r[:3] == [3, 37, 680] for r in taken) and not any(r[0] == 3 and r[2] >= 681 for r in taken)    # the thread bound at C = 3
    assert any(r[:3] == [1, 37, 2048] for r in taken) and not any(r[2] == 2049 for r in taken)


@pytest.mark.parametrize("shape", [(2, 3, 32, 32, 3), (1, 2, 24, 40, 1), (1, 1, 11, 11, 3), (2, 2, 40, 24, 3), (1, 2, 13, 17, 4)])
def test_composed_matches_numpy_definition(shape):
    from video_vae_amd.metrics import frame_metrics
    x, y = pair(*shape, seed=sum(shape))
    mask = torch.ones(shape[:2])
    if shape[1] > 1:
        mask[0, -1] = 0
    fm = frame_metrics(x, y, mask)
    ref = ref_metrics(x, y, mask)
    for got, want in zip(fm, ref):
        assert got.dtype == torch.float32 and got.shape == shape[:2]
        np.testing.assert_allclose(got.double().numpy(), want, rtol=1e-6, atol=1e-7)
    assert float(fm.ssim[mask != 0].min()) < 0.99 and float(fm.psnr[mask != 0].max()) < 40


def test_bf16_operands_are_converted():
    from video_vae_amd.metrics import frame_metrics
    x, y = pair(1, 2, 20, 20, 3, seed=5)
    yb = y.to(torch.bfloat16)
    fm = frame_metrics(x, yb, torch.ones(1, 2))
    for got, want in zip(fm, ref_metrics(x, yb.float(), torch.ones(1, 2))):
        np.testing.assert_allclose(got.double().numpy(), want, rtol=1e-6, atol=1e-7)


def test_identical_frames_and_constant_offset():
    from video_vae_amd.metrics import frame_metrics
    x, _ = pair(2, 2, 16, 16, 3, seed=1)
    fm = frame_metrics(x, x.clone(), torch.ones(2, 2))
    assert torch.all(fm.mse == 0) and torch.allclose(fm.ssim, torch.ones(2, 2), atol=1e-7)
    assert torch.allclose(fm.psnr, torch.full((2, 2), 100.0), atol=1e-5)
    base = 0.2 + 0.5 * x                                             # in [0.2, 0.7]: the offset never clamps
    for d in (0.1, 0.02):
        fm = frame_metrics(base, base + d, torch.ones(2, 2))
        np.testing.assert_allclose(fm.psnr.double().numpy(), -20 * math.log10(d), atol=1e-4)


def test_clamping():
    from video_vae_amd.metrics import frame_metrics
    x, y = pair(1, 2, 16, 16, 3, seed=3, noise=0.5)
    mask = torch.ones(1, 2)
    a = frame_metrics(x, y, mask)
    b = frame_metrics(x.clamp(0, 1), y.clamp(0, 1), mask)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    c = frame_metrics(x, y, mask, clamp=False)
    assert not torch.allclose(c.mse, a.mse)
    for got, want in zip(c, ref_metrics(x, y, mask, clamp=False)):
        np.testing.assert_allclose(got.double().numpy(), want, rtol=1e-6, atol=1e-7)


def test_masked_frames_are_zero_and_never_nan():
    from video_vae_amd.metrics import frame_metrics
    x, y = pair(2, 3, 16, 16, 3, seed=4)
    mask = torch.tensor([[1.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
    x[0, 1] = float("nan")
    fm = frame_metrics(x, y, mask)
    for v in fm:
        assert torch.all(v[mask == 0] == 0) and torch.all(torch.isfinite(v))
        assert torch.all(v[mask != 0] != 0)


def test_clip_means_weighted_by_valid_frames():
    from video_vae_amd.metrics import clip_metrics, frame_metrics
    x, y = pair(3, 4, 16, 16, 3, seed=6)
    mask = torch.tensor([[1.0, 1.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]])
    sel = torch.tensor([[1.0, 0.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0], [0.0, 1.0, 1.0, 1.0]])
    fm = frame_metrics(x, y, mask)
    cm = clip_metrics(x, y, mask, sel)
    assert cm.frames.tolist() == [3, 0, 1]
    for got, per in zip((cm.mse, cm.psnr, cm.ssim), fm):
        assert got.shape == (3,)
        assert abs(float(got[0]) - float(per[0, :3].mean())) < 1e-6
        assert float(got[1]) == 0.0
        assert abs(float(got[2]) - float(per[2, 0])) < 1e-6
    np.testing.assert_allclose(cm.kept_fraction.numpy(), [2 / 3, 0.0, 0.0], atol=1e-7)
    assert clip_metrics(x, y, mask).kept_fraction is None


def test_shape_validation():
    from video_vae_amd.metrics import frame_metrics
    x, y = pair(1, 2, 16, 16, 3, seed=7)
    with pytest.raises(ValueError):
        frame_metrics(x[:, :, :10], y[:, :, :10], torch.ones(1, 2))
    with pytest.raises(ValueError):
        frame_metrics(x[:, :, :, :10], y[:, :, :, :10], torch.ones(1, 2))
    with pytest.raises(ValueError):
        frame_metrics(x[0], y[0], torch.ones(1, 2))
    with pytest.raises(ValueError):
        frame_metrics(x, y[:, :1], torch.ones(1, 2))
    with pytest.raises(ValueError):
        frame_metrics(x, y, torch.ones(2, 1))


def test_kernel_op_has_no_cpu_fallback():
    from video_vae_amd import ops
    from video_vae_amd._lib import VvaeError
    x, y = pair(1, 1, 16, 16, 3, seed=8)
    with pytest.raises(VvaeError):
        ops.recon_metrics(x, y, torch.ones(1, 1))


def test_evaluate_mode_and_eval_command_exist():
    from video_vae_amd.infer import MODES
    assert "evaluate" in MODES and MODES[:3] == ("encode", "decode", "reconstruct")
    r = subprocess.run([sys.executable, "-m", "video_vae_amd.infer", "eval", "--help"], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--model_path", "--data", "--flavour", "--size", "--frames", "--batch", "--small", "--threshold", "--seed", "--out",
                 "--per-frame"):
        assert flag in r.stdout, flag
