"""GPU: the scene-cut kernels (csrc/scenes.hip) against the composed definition of scenes.py, bitwise counts and determinism; scene_cuts
on a synthetic clip; ClipInference with cuts against per-scene runs, against no cuts, and the isolation of one scene from another;
``infer scenes`` and ``infer encode|decode|eval --scene-cuts`` end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 64
# (L, H, W): W = 1; odd W and H W not a multiple of 4 (byte loads); one chunk; several chunks (720p); W = 8192, several chunks
SHAPES = [(3, 5, 1), (3, 7, 13), (2, 33, 64), (3, 720, 1280), (2, 40, 8192)]
SIZES = [("hsv", 1), ("hsv", 26), ("hsv", 64), ("gray", 16), ("gray", 256)]


def _clip(shape, seed):
    """A random uint8 clip whose last frame is one solid colour (the contention case: every pixel in one bin)."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(0, 256, tuple(shape) + (3,), generator=g, dtype=torch.uint8)
    c[-1] = torch.tensor([30, 170, 90], dtype=torch.uint8)
    return c


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("space,n", SIZES)
def test_kernel_counts_and_corr_equal_definition(dev, shape, space, n):
    from video_vae_amd import ops
    from video_vae_amd.scenes import frame_histograms, histogram_correlation
    clip = _clip(shape, shape[1] * 7 + n)
    want = frame_histograms(clip, n, space)
    counts, corr = ops.scene_hist(clip.to(dev), n, space)
    counts2, corr2 = ops.scene_hist(clip.to(dev), n, space)
    torch.cuda.synchronize()
    assert counts.dtype == torch.int32 and counts.shape == want.shape
    assert torch.equal(counts.cpu(), want), (shape, space, n)
    assert (counts.sum(dim=1) == shape[1] * shape[2]).all()
    assert int((counts[-1] != 0).sum()) == 1                                   # the solid frame
    np.testing.assert_allclose(corr.cpu().numpy(), histogram_correlation(want).numpy(), rtol=1e-12, atol=1e-12)
    assert torch.equal(counts, counts2) and torch.equal(corr, corr2)
    assert torch.equal(ops.scene_corr(counts), corr)


def test_solid_clip_and_degenerate_corr(dev):
    from video_vae_amd import ops
    clip = torch.zeros((3, 1080, 1920, 3), dtype=torch.uint8)
    clip[1, ..., 0] = 255                                                     # pure red: H 0, S 255 -> bin 63; black: bin 0
    counts, corr = ops.scene_hist(clip.to(dev), 64, "hsv")
    assert counts[:, 0].tolist() == [1080 * 1920, 0, 1080 * 1920] and int(counts[1, 63].item()) == 1080 * 1920
    assert (counts.sum(dim=1) == 1080 * 1920).all() and corr.cpu().numpy().max() < 0
    ramp = torch.arange(256, dtype=torch.uint8).reshape(1, 1, 256, 1).expand(2, 1, 256, 3).contiguous()   # every gray bin once
    c, r = ops.scene_hist(ramp.to(dev), 256, "gray")
    assert (c == 1).all() and r.tolist() == [1.0]
    with pytest.raises(ops.VvaeError):
        ops.scene_hist(clip[:, :, :1].contiguous().to(dev), 65, "hsv")


def _palette_clip(lengths, hw, seed):
    """Scenes of distinct palettes, every frame of a scene the same palette proportions in new places; -> uint8 (L, H, W, 3)."""
    rng = np.random.default_rng(seed)
    pals = [rng.integers(0, 70, size=(4, 3)), rng.integers(180, 256, size=(4, 3)), np.array([[0, 0, 255], [0, 40, 200], [10, 10, 230],
                                                                                             [0, 90, 255]])]
    frames = []
    for i, n in enumerate(lengths):
        p = pals[i % 3]
        for _ in range(n):
            frames.append(p[rng.permutation(np.arange(hw[0] * hw[1]) % 4).reshape(hw)].astype(np.uint8))
    return np.stack(frames)


def test_scene_cuts_three_scenes(dev):
    from video_vae_amd.scenes import scene_cuts
    clip = torch.from_numpy(_palette_clip((5, 4, 6), (72, 128), 1))
    for space, n in (("hsv", 64), ("hsv", 16), ("gray", 64)):
        assert scene_cuts(clip.to(dev), n, 0.85, space) == [5, 9], space
        assert scene_cuts(clip, n, 0.85, space) == [5, 9], space


def _small(flavour, seed):
    import video_vae_amd as V
    from video_vae_amd import rl_model
    from video_vae_amd.infer import model_config
    cls = rl_model.VideoVAE if flavour == "rl" else V.VideoVAE
    return cls(rngs=V.Rngs(seed), **model_config(SMALL, True))


def _u8(shape, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(dev)


@pytest.mark.parametrize("tiled", [True, False])
def test_clip_with_cuts_equals_scenes_alone(dev, tiled):
    """Windows of 4 overlapping by 2, scenes of 5, 4 and 2 frames (the last one padded), batch 4 so that batches mix scenes.  Every
    window sees exactly the frames (and zero padding) it sees when its scene runs alone, and the kernels of the model are batch-position
    independent, so the frames match bitwise."""
    from video_vae_amd.infer import InferenceWeights
    from video_vae_amd.tiling import ClipInference, ScenePlan, TileGrid
    m = _small("model", 4).to(dev)
    w = InferenceWeights(m)
    hw = (100, 150) if tiled else (SMALL, SMALL)
    g = TileGrid(hw[0], hw[1], SMALL, 16 if tiled else 0)
    clip = _u8((11,) + hw + (3,), 7, dev)
    cuts = [5, 9]
    for mode in ("reconstruct", "encode"):
        ci = ClipInference(m, w, g, 4, 4, 2, mode)
        out = ci(clip, cuts=cuts)
        plan = ScenePlan(11, 4, 2, cuts)
        assert out.plan == plan and out.selection.shape == (plan.windows, g.tiles, 4)
        for i, (a, e) in enumerate(plan.scenes):
            alone = ci(clip[a:e])
            ws = slice(plan.first[i], plan.first[i] + plan.plans[i].windows)
            assert alone.plan.starts == plan.plans[i].starts
            assert torch.equal(out.selection[ws], alone.selection), (mode, i)
            if mode == "reconstruct":
                assert torch.equal(out.frames[a:e], alone.frames), (mode, i)
            else:
                assert torch.equal(out.mean[ws], alone.mean), (mode, i)
        none = ci(clip)
        empty = ci(clip, cuts=[])
        assert empty.plan.starts == none.plan.starts
        for u, v in zip((empty.frames, empty.selection, empty.mean), (none.frames, none.selection, none.mean)):
            assert (u is None and v is None) or torch.equal(u, v)


def test_isolation_across_a_cut(dev):
    """--temporal-overlap 4 (windows of 8): perturbing every pixel of scene A leaves scene B's frames bitwise unchanged with the cut;
    without it a window straddles the boundary and they change."""
    from video_vae_amd.infer import InferenceWeights
    from video_vae_amd.tiling import ClipInference, TileGrid
    m = _small("rl", 3).to(dev)
    w = InferenceWeights(m)
    ci = ClipInference(m, w, TileGrid(SMALL, SMALL, SMALL, 0), 4, 8, 4, "reconstruct")
    clip = _u8((20, SMALL, SMALL, 3), 9, dev)
    other = clip.clone()
    other[:9] = 255 - other[:9]
    a, b = ci(clip, cuts=[9]), ci(other, cuts=[9])
    assert torch.equal(a.frames[9:], b.frames[9:])
    assert not torch.equal(a.frames[:9], b.frames[:9])
    assert not torch.equal(ci(clip).frames[9:], ci(other).frames[9:])


def _run(args):
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "video_vae_amd.infer"] + args
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def _common(tmp_path, data, frames):
    return ["--model_path", str(tmp_path / "ckpt"), "--data", str(data), "--size", str(SMALL), "--frames", str(frames), "--batch", "4",
            "--small", "--threshold"]


def _data(tmp_path):
    data = tmp_path / "data"
    data.mkdir()
    np.save(data / "wide.npy", _palette_clip((9, 5), (100, 150), 2))           # a cut at 9
    np.save(data / "small.npy", _palette_clip((6,), (40, 48), 3))              # no cut
    return data


def test_cli_scenes(dev, tmp_path):
    data = _data(tmp_path)
    out = tmp_path / "scenes.json"
    _run(["scenes", "--data", str(data), "--out", str(out)])
    res = json.loads(out.read_text())
    assert res["config"]["hist_size"] == 64 and res["config"]["similarity"] == 0.85 and res["config"]["space"] == "hsv"
    by = {c["name"]: c for c in res["clips"]}
    assert by["wide"]["cuts"] == [9] and by["wide"]["scenes"] == [[0, 9], [9, 14]] and by["small"]["cuts"] == []
    assert (by["wide"]["frames"], by["wide"]["height"], by["wide"]["width"]) == (14, 100, 150)
    _run(["scenes", "--data", str(data), "--out", str(out), "--scene-gray", "--scene-hist", "32"])
    res = json.loads(out.read_text())
    assert res["config"]["space"] == "gray" and {c["name"]: c["cuts"] for c in res["clips"]} == {"wide": [9], "small": []}


def test_cli_encode_decode_eval_scene_cuts(dev, tmp_path):
    from video_vae_amd import model_loader
    from video_vae_amd.infer import InferenceWeights, centre_square
    from video_vae_amd.metrics import temporal_mse, temporal_summary_scenes
    from video_vae_amd.tiling import ClipInference, TileGrid
    data = _data(tmp_path)
    model = _small("rl", 9)
    model_loader.save_checkpoint(model, None, str(tmp_path / "ckpt"))
    m = model.to(dev)
    w = InferenceWeights(m)
    for tiled in (True, False):
        tile = ["--tile", "--overlap", "16"] if tiled else []
        lat, rec = tmp_path / f"lat{int(tiled)}", tmp_path / f"rec{int(tiled)}"
        _run(["encode"] + _common(tmp_path, data, 8) + tile + ["--scene-cuts", "--temporal-overlap", "4", "--out", str(lat)])
        _run(["decode", "--model_path", str(tmp_path / "ckpt"), "--batch", "4", "--latents", str(lat), "--out", str(rec)])
        out = tmp_path / f"ev{int(tiled)}.json"
        _run(["eval"] + _common(tmp_path, data, 8) + tile + ["--scene-cuts", "--temporal-overlap", "4", "--temporal-metrics",
                                                             "--per-frame", "--out", str(out)])
        res = json.loads(out.read_text())
        assert res["config"]["scene_cuts"] == {"hist_size": 64, "similarity": 0.85, "space": "hsv"}
        assert res["dataset"]["scene_pairs"] == 1 and res["dataset"]["pairs"] == 13 + 5
        clips = {c["name"]: c for c in res["clips"]}
        rc = ev = None
        for name, n, cuts in (("wide", 14, [9]), ("small", 6, [])):
            raw = np.load(data / f"{name}.npy")
            clip = raw if tiled else centre_square(raw, SMALL)
            g = TileGrid(clip.shape[1], clip.shape[2], SMALL, 16) if tiled else TileGrid(SMALL, SMALL, SMALL, 0)
            u8 = torch.from_numpy(clip).to(dev)
            with np.load(lat / f"{name}.npz") as z:
                assert z["scene_cuts"].dtype == np.int64 and z["scene_cuts"].tolist() == cuts and int(z["n_frames"]) == n
            rc = ClipInference(m, w, g, 4, 8, 4, "reconstruct") if rc is None else rc.with_grid(g)
            want = (np.clip(rc(u8, cuts=cuts).frames.cpu().numpy(), 0, 1) * 255).astype(np.uint8)
            with np.load(rec / f"{name}.npz") as z:
                got = z["frames"]
            assert got.shape == (n, g.height, g.width, 3) and got.dtype == np.uint8
            np.testing.assert_array_equal(got, want)
            e = clips[name]
            assert e["scene_cuts"] == cuts and len(e["scenes"]) == len(cuts) + 1 and e["scene_pairs"] == len(cuts)
            ev = ClipInference(m, w, g, 4, 8, 4, "evaluate") if ev is None else ev.with_grid(g)
            o = ev(u8, cuts=cuts)
            assert e["per_frame"]["psnr"] == o.metrics.psnr[0].double().cpu().tolist()
            tm = temporal_mse(u8.float()[None] / 255.0, o.frames[None])[0].double().cpu().numpy()
            summ = temporal_summary_scenes(tm, 8, cuts)
            assert all(e[k] == summ[k] for k in summ)


def test_cli_without_scene_flags_unchanged(dev, tmp_path):
    """No --scene-* flag: no new key in the JSON or the latent files.  A clip without cuts gives the same per-frame values with
    --scene-cuts as without (its ScenePlan is the WindowPlan)."""
    from video_vae_amd import model_loader
    data = _data(tmp_path)
    model_loader.save_checkpoint(_small("rl", 9), None, str(tmp_path / "ckpt"))
    base = ["eval"] + _common(tmp_path, data, 4) + ["--temporal-overlap", "2", "--temporal-metrics", "--per-frame"]
    _run(base + ["--out", str(tmp_path / "a.json")])
    _run(base + ["--scene-cuts", "--out", str(tmp_path / "b.json")])
    a, b = json.loads((tmp_path / "a.json").read_text()), json.loads((tmp_path / "b.json").read_text())
    assert "scene_cuts" not in a["config"] and "scene_pairs" not in a["dataset"]
    for c in a["clips"]:
        assert not {"scene_cuts", "scenes", "tmse_scene", "scene_pairs"} & set(c)
    sa, sb = [next(c for c in r["clips"] if c["name"] == "small") for r in (a, b)]
    assert sb["scene_cuts"] == [] and sa["per_frame"] == sb["per_frame"]
    for k in ("psnr", "ssim", "mse", "kept_fraction", "tmse", "tmse_seam", "tmse_inner", "pairs", "seam_pairs"):
        assert sa[k] == sb[k], k
    _run(["encode"] + _common(tmp_path, data, 4) + ["--temporal-overlap", "2", "--out", str(tmp_path / "lat")])
    with np.load(tmp_path / "lat" / "wide.npz") as z:
        assert "scene_cuts" not in z.files
