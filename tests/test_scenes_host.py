"""CPU: scene-cut detection (scenes.py: OpenCV's 8-bit HSV / gray conversions, the histogram bin tables, the composed histograms, the
correlation, the reference's change-point rule), the scene-aware window plan (tiling.ScenePlan), the composed blend over scenes and the
latent files with ``scene_cuts``."""
import math
import sys

import numpy as np
import pytest
import torch

from test_temporal_host import ref_blend_windows


@pytest.mark.parametrize("rgb,hsv", [((255, 0, 0), (0, 255, 255)), ((0, 255, 0), (60, 255, 255)), ((0, 0, 255), (120, 255, 255)),
                                     ((255, 255, 0), (30, 255, 255)), ((0, 255, 255), (90, 255, 255)), ((255, 0, 255), (150, 255, 255)),
                                     ((128, 128, 128), (0, 0, 128)), ((200, 100, 50), (10, 191, 200)), ((0, 0, 0), (0, 0, 0))])
def test_hsv_pins(rgb, hsv):
    from video_vae_amd.scenes import rgb_to_hsv
    h, s, v = rgb_to_hsv(np.array([rgb], dtype=np.uint8))
    assert (int(h[0]), int(s[0]), int(v[0])) == hsv


def test_hue_stays_in_range_and_gray_pins():
    from video_vae_amd.scenes import rgb_to_gray, rgb_to_hsv
    g = np.arange(0, 256, 3, dtype=np.uint8)
    rgb = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    h, s, v = rgb_to_hsv(rgb)
    assert h.min() == 0 and h.max() <= 179 and s.max() <= 255 and (v == rgb.max(axis=1)).all()
    assert rgb_to_gray(np.array([[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]], dtype=np.uint8)).tolist() == \
        [255, 0, 76, 150, 29]


def test_divisor_and_bin_tables():
    from video_vae_amd.scenes import bin_table, hsv_divisors, tables
    sdiv, hdiv = hsv_divisors()
    assert sdiv[0] == 0 and hdiv[0] == 0 and sdiv[1] == 255 << 12 and hdiv[1] == (180 << 12) // 6 and sdiv[255] == 4096
    for i in range(1, 256):                              # no .5 tie: the rounding mode does not matter
        assert abs((255 << 12) / i - sdiv[i]) < 0.5 and abs((180 << 12) / (6 * i) - hdiv[i]) < 0.5
    for n in (1, 8, 26, 30, 50, 64):
        hb, sb = bin_table(n, 180), bin_table(n, 256)
        for j in range(256):
            assert hb[j] == min(math.floor(j * (n / 180.0)), n - 1)        # cv2.calcHist: the scale n / 180 first, in float64
            assert sb[j] == min(math.floor(j * (n / 256.0)), n - 1) == min((j * n) >> 8, n - 1)
        assert hb[:180].max() <= n - 1 and sb.max() == n - 1
    # OpenCV's order differs from j n / 180 where j n / 180 is an integer the scaled product misses (26 bins: hue 90 -> bin 12, not 13)
    assert bin_table(26, 180)[90] == 12 and math.floor(90 * 26 / 180.0) == 13
    t = tables(64, "hsv")
    assert t.dtype == np.int32 and t.shape == (1024,) and (t[:256] == sdiv).all() and (t[768:] == bin_table(64, 256)).all()
    assert tables(16, "gray").shape == (256,)
    for bad in ((0, "hsv"), (65, "hsv"), (257, "gray"), (8, "rgb")):
        with pytest.raises(ValueError):
            tables(*bad)


def _loop_hist(clip, n, space):
    """The per-pixel Python loop: one scalar OpenCV conversion per pixel."""
    from video_vae_amd.scenes import bin_table, hsv_divisors
    sdiv, hdiv = hsv_divisors()
    hb, sb = bin_table(n, 180), bin_table(n, 256)
    out = np.zeros((clip.shape[0], n * n if space == "hsv" else n), dtype=np.int64)
    for f in range(clip.shape[0]):
        for r, g, b in clip[f].reshape(-1, 3).tolist():
            if space == "gray":
                out[f, sb[(4899 * r + 9617 * g + 1868 * b + 8192) >> 14]] += 1
                continue
            v = max(r, g, b)
            d = v - min(r, g, b)
            s = (d * int(sdiv[v]) + 2048) >> 12
            h = g - b if v == r else (b - r + 2 * d if v == g else r - g + 4 * d)
            h = (h * int(hdiv[d]) + 2048) >> 12
            if h < 0:
                h += 180
            out[f, hb[h] * n + sb[s]] += 1
    return out


@pytest.mark.parametrize("space,n", [("hsv", 8), ("hsv", 26), ("gray", 16), ("gray", 256)])
def test_composed_histograms_equal_pixel_loop(space, n):
    from video_vae_amd.scenes import frame_histograms
    rng = np.random.default_rng(n)
    clip = rng.integers(0, 256, size=(3, 5, 7, 3), dtype=np.uint8)
    clip[2] = (40, 200, 90)                                                   # a solid frame: one bin
    got = frame_histograms(torch.from_numpy(clip), n, space)
    assert got.dtype == torch.int32 and got.shape == (3, n * n if space == "hsv" else n)
    np.testing.assert_array_equal(got.numpy(), _loop_hist(clip, n, space))
    assert (got.sum(dim=1) == 35).all() and int((got[2] != 0).sum()) == 1


def _ref_correl(a, b):
    a, b = [float(x) for x in a], [float(x) for x in b]
    n = len(a)
    s1, s2 = sum(a), sum(b)
    s11, s22, s12 = sum(x * x for x in a), sum(y * y for y in b), sum(x * y for x, y in zip(a, b))
    num = s12 - s1 * s2 / n
    den = (s11 - s1 * s1 / n) * (s22 - s2 * s2 / n)
    return num / math.sqrt(den) if abs(den) > sys.float_info.epsilon else 1.0


def test_correlation_definition_and_degenerate_case():
    from video_vae_amd.scenes import histogram_correlation
    rng = np.random.default_rng(3)
    c = torch.from_numpy(rng.integers(0, 1000, size=(5, 64)).astype(np.int32))
    got = histogram_correlation(c)
    assert got.dtype == torch.float64 and got.shape == (4,)
    for i in range(4):
        assert abs(float(got[i]) - _ref_correl(c[i].tolist(), c[i + 1].tolist())) <= 1e-13
    np.testing.assert_allclose(got.numpy(), [np.corrcoef(c[i].double(), c[i + 1].double())[0, 1] for i in range(4)], rtol=1e-12)
    flat = torch.full((2, 16), 7, dtype=torch.int32)                          # zero variance: 1.0
    assert histogram_correlation(flat).tolist() == [1.0]
    same = torch.tensor([[5, 0, 0, 1], [5, 0, 0, 1]], dtype=torch.int32)
    assert abs(float(histogram_correlation(same)[0]) - 1.0) <= 1e-15
    assert histogram_correlation(c[:1]).shape == (0,)


def test_change_indices_accumulates_and_resets():
    from video_vae_amd.scenes import change_indices
    assert change_indices([0.99, 0.2, 0.99]) == [2]                      # one clear cut
    assert change_indices([0.95, 0.95, 0.95, 0.95]) == [3]               # drift: 0.05 + 0.05 + 0.05 > 0.15 at frame 3
    assert change_indices([0.95, 0.95, 0.95, 0.95, 0.95, 0.95]) == [3, 6]   # the accumulator restarts after a cut
    assert change_indices([0.1, 0.1, 0.1]) == [1, 2, 3]                  # back-to-back cuts
    assert change_indices([0.5, 1.0], similarity=0.4) == []               # 0.5 is not > 0.6
    assert change_indices([]) == []


def test_scene_cuts_on_three_palettes():
    from video_vae_amd.scenes import scene_cuts, scene_ranges
    rng = np.random.default_rng(5)
    pal = [rng.integers(0, 80, size=(4, 3)), rng.integers(170, 256, size=(4, 3)), np.array([[0, 0, 255], [0, 40, 200], [10, 10, 230],
                                                                                             [0, 90, 255]])]
    frames = []
    for p, n in zip(pal, (4, 3, 5)):
        for _ in range(n):                                  # the same palette proportions in new places: one histogram per scene
            frames.append(p[rng.permutation(np.arange(48) % 4).reshape(6, 8)].astype(np.uint8))
    clip = torch.from_numpy(np.stack(frames))
    for space, hs in (("hsv", 16), ("gray", 32)):
        assert scene_cuts(clip, hs, 0.85, space) == [4, 7], space
    assert scene_ranges([4, 7], 12) == [[0, 4], [4, 7], [7, 12]] and scene_ranges([], 3) == [[0, 3]]


# ------------------------------------------------------------------------------------------------ ScenePlan
@pytest.mark.parametrize("length,frames,o,cuts", [(20, 4, 2, [7, 9, 16]), (13, 4, 0, [3]), (10, 4, 1, [1, 2, 9]), (30, 8, 4, [12])])
def test_scene_plan_never_crosses_a_cut(length, frames, o, cuts):
    from video_vae_amd.tiling import ScenePlan, WindowPlan
    p = ScenePlan(length, frames, o, cuts)
    assert p.cuts == cuts and p.scenes[0][0] == 0 and p.scenes[-1][1] == length
    assert p.windows == len(p.starts) == len(p.counts) == p.weights.shape[0] == p.mask().shape[0]
    for w, (st, c) in enumerate(zip(p.starts, p.counts)):
        si, lw = p.scene(w)
        a, e = p.scenes[si]
        assert a <= st and st + c <= e                                      # a window's real frames lie in its scene
        assert p.mask()[w].sum() == c and (p.mask()[w, :c] == 1).all()
        if e - a < frames:                                                  # a short scene: one padded window
            assert p.plans[si].windows == 1 and c == e - a
        else:
            assert c == frames
        assert st - a == p.plans[si].starts[lw]
    for f in range(length):
        cov = p.covering(f)
        assert cov and all(p.starts[w] <= f < p.starts[w] + p.counts[w] for w in cov)
        assert len({p.scene(w)[0] for w in cov}) == 1
        assert p.scene(cov[0])[0] == sum(1 for c in cuts if c <= f)
    assert p.ring() == max(q.ring() for q in p.plans)
    assert p.stored_ratio() == sum(p.counts) / length and p.starts_array().dtype == np.int64
    np.testing.assert_array_equal(np.concatenate([q.weights for q in p.plans]), p.weights)
    assert p == ScenePlan(length, frames, o, list(cuts)) and p != WindowPlan(length, frames, o)


@pytest.mark.parametrize("length,frames,o", [(9, 4, 2), (3, 8, 2), (16, 4, 0), (13, 4, 1)])
def test_scene_plan_without_cuts_is_the_window_plan(length, frames, o):
    from video_vae_amd.tiling import ScenePlan, WindowPlan
    p, q = ScenePlan(length, frames, o, []), WindowPlan(length, frames, o)
    assert p.starts == q.starts and p.counts == q.counts and p.windows == q.windows and p.ring() == q.ring()
    np.testing.assert_array_equal(p.weights, q.weights)
    np.testing.assert_array_equal(p.mask(), q.mask())
    assert all(p.covering(f) == q.covering(f) for f in range(length))


@pytest.mark.parametrize("cuts", [[5, 3], [3, 3], [0], [10], [12], [2.5]])
def test_scene_plan_rejects_bad_cuts(cuts):
    from video_vae_amd.tiling import ScenePlan
    with pytest.raises(ValueError):
        ScenePlan(10, 4, 1, cuts)


def test_composed_blend_on_scene_plan_is_the_scene_blends():
    from video_vae_amd.tiling import ScenePlan, TileGrid, blend_windows
    plan, grid = ScenePlan(17, 4, 2, [3, 11]), TileGrid(20, 30, 16, 4)
    g = torch.Generator().manual_seed(1)
    tiles = torch.rand((plan.windows, grid.tiles, 4, 16, 16, 3), generator=g)
    got = blend_windows(tiles, plan, grid)
    assert got.shape == (17, 20, 30, 3) and got.dtype == torch.float64
    want = np.concatenate([ref_blend_windows(tiles[plan.first[i]:plan.first[i] + p.windows].numpy(), p, grid)
                           for i, p in enumerate(plan.plans)])
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=1e-12)
    for i, ((a, e), p) in enumerate(zip(plan.scenes, plan.plans)):
        assert torch.equal(got[a:e], blend_windows(tiles[plan.first[i]:plan.first[i] + p.windows], p, grid))


# ------------------------------------------------------------------------------------------------ latent files
def _packed(plan, grid, seed):
    from video_vae_amd.infer import pack_latents_windows
    rng = np.random.default_rng(seed)
    fw = min(plan.frames, plan.length)
    mean = rng.standard_normal((plan.windows, grid.tiles, fw, 4, 6)).astype(np.float32)
    sel = rng.integers(0, 2, size=(plan.windows, grid.tiles, fw)).astype(np.float32)
    return pack_latents_windows(torch.from_numpy(mean), torch.from_numpy(sel), grid, plan), mean, sel


def test_latent_windows_round_trip_with_scene_cuts():
    from video_vae_amd.infer import unpack_latents_windows
    from video_vae_amd.tiling import ScenePlan, TileGrid
    plan, grid = ScenePlan(14, 4, 2, [2, 9]), TileGrid(40, 50, 32, 8)
    arrays, mean, sel = _packed(plan, grid, 0)
    assert arrays["scene_cuts"].dtype == np.int64 and arrays["scene_cuts"].tolist() == [2, 9]
    assert arrays["window_starts"].tolist() == plan.starts
    assert not arrays["selection"][0, :, 2:].any()                       # the padding of the 2-frame scene is not kept
    fill = torch.arange(6, dtype=torch.float32)
    comp, s, g2, p2 = unpack_latents_windows(arrays, fill)
    assert p2 == plan and g2 == grid
    keep = sel != 0
    for w, c in enumerate(plan.counts):
        keep[w, :, c:] = False
    np.testing.assert_array_equal(s, keep.astype(np.uint8))
    np.testing.assert_array_equal(comp[keep], mean[keep])
    assert (comp[~keep] == fill.numpy()).all()
    bad = dict(arrays, scene_cuts=np.array([3, 9], dtype=np.int64))      # starts that do not fit the cuts
    with pytest.raises(ValueError):
        unpack_latents_windows(bad, fill)


def test_latent_windows_without_cuts_unchanged():
    from video_vae_amd.infer import unpack_latents_windows
    from video_vae_amd.tiling import TileGrid, WindowPlan
    plan, grid = WindowPlan(9, 4, 2), TileGrid(32, 32, 32, 0)
    arrays, mean, sel = _packed(plan, grid, 1)
    assert "scene_cuts" not in arrays and sorted(arrays) == ["mean", "n_frames", "selection", "temporal_overlap", "tile_grid", "window",
                                                            "window_starts"]
    np.testing.assert_array_equal(arrays["selection"], (sel != 0).astype(np.uint8))
    np.testing.assert_array_equal(arrays["mean"], mean[sel != 0])
    _, _, _, p2 = unpack_latents_windows(arrays, torch.zeros(6))
    assert p2 == plan and isinstance(p2, WindowPlan)


def test_temporal_summary_scenes_splits_off_the_cut_pairs():
    from video_vae_amd.metrics import temporal_summary, temporal_summary_scenes
    v = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0]                     # pairs t = 1 .. 9
    s = temporal_summary_scenes(v, 4, [3, 8])
    assert s["scene_pairs"] == 2 and s["tmse_scene"] == (3.0 + 8.0) / 2
    assert s["seam_pairs"] == 1 and s["tmse_seam"] == 4.0                 # t = 4 (t = 8 is a cut)
    assert s["tmse_inner"] == (1 + 2 + 5 + 6 + 7 + 9) / 6 and s["pairs"] == 9 and s["tmse"] == 5.0
    base = temporal_summary(v, 4)
    assert {k: temporal_summary_scenes(v, 4, [])[k] for k in base} == base
