"""CPU: the temporal window plan (the issue's examples, a coverage sweep, the bridge to hard cuts), the composed window blend against the
clip it was cut from and against a direct numpy restatement, the temporal-difference metric against numpy, and the windowed latent
files' round trip."""
import numpy as np
import pytest
import torch

from video_vae_amd.infer import pack_latents_windows, unpack_latents_windows, windows
from video_vae_amd.metrics import temporal_mse, temporal_summary
from video_vae_amd.tiling import TileGrid, WindowPlan, axis_starts, axis_weights, blend_windows


def test_plan_examples():
    p = WindowPlan(9, 4, 2)
    assert p.starts == [0, 1, 3, 5] and p.windows == 4 and p.counts == [4, 4, 4, 4]
    assert p.covering(3) == [0, 1, 2] and p.covering(8) == [3]
    assert p.final(0) == 1 and p.final(3) == 9
    assert p.stored_ratio() == 16 / 9 and p.ring() == 3
    np.testing.assert_array_equal(p.weights, axis_weights(9, 4, 2))
    short = WindowPlan(5, 8, 4)                       # shorter than a window: one window at 0, padded and masked
    assert short.starts == [0] and short.counts == [5] and short.stored_ratio() == 1.0
    np.testing.assert_array_equal(short.mask(), np.array([[1, 1, 1, 1, 1, 0, 0, 0]], dtype=np.float32))
    assert WindowPlan(64, 16, 4).starts == [0, 12, 24, 36, 48]
    assert WindowPlan(64, 16, 8).starts == [0, 8, 16, 24, 32, 40, 48]
    for bad in (-1, 3, 5):
        with pytest.raises(ValueError):
            WindowPlan(9, 4, bad)
    with pytest.raises(ValueError):
        WindowPlan(0, 4, 0)


@pytest.mark.parametrize("frames", [1, 2, 4, 5, 16])
def test_plan_sweep(frames):
    for o in range(frames // 2 + 1):
        for length in range(1, 6 * frames + 9):
            p = WindowPlan(length, frames, o)
            assert p.starts == axis_starts(length, frames, o)
            cover = np.zeros(length, dtype=int)
            for st, c in zip(p.starts, p.counts):
                assert c == min(frames, length)           # every window full unless the clip is shorter than one
                cover[st:st + c] += 1
            assert cover.min() >= 1 and p.starts[-1] + p.counts[-1] == length
            for a, b in zip(p.starts, p.starts[1:]):
                assert a < b and a + frames - b >= o, (length, frames, o, p.starts)
            assert p.ring() <= p.windows and p.ring() <= 4
            if length % frames == 0 and o == 0:           # hard cuts
                assert [(st, c) for st, c in zip(p.starts, p.counts)] == windows(length, frames)


def ref_blend_windows(tiles, plan, grid):
    """Direct float64 restatement: per output value, the covering (window, ty, tx) in ascending order."""
    tiles = np.asarray(tiles, dtype=np.float64)
    s, c = grid.tile, tiles.shape[-1]
    wt = axis_weights(plan.length, plan.frames, plan.overlap)
    out = np.zeros((plan.length, grid.height, grid.width, c))
    for f in range(plan.length):
        for y in range(grid.height):
            for x in range(grid.width):
                num, den = np.zeros(c), 0.0
                for w in plan.covering(f):
                    q = f - plan.starts[w]
                    for ty, y0 in enumerate(grid.ys):
                        if not y0 <= y < y0 + s:
                            continue
                        for tx, x0 in enumerate(grid.xs):
                            if not x0 <= x < x0 + s:
                                continue
                            wk = wt[w, q] * grid.weights_y[ty][y - y0] * grid.weights_x[tx][x - x0]
                            num += wk * tiles[w, ty * grid.nx + tx, q, y - y0, x - x0]
                            den += wk
                out[f, y, x] = num / den
    return out


def window_crops(clip, plan, grid):
    """Tiles (windows, ny nx, F, S, S, C) of a float64 clip (L, H, W, C): zero-padded past L, edge-replicated past the frame."""
    fr = plan.frames
    padded = np.concatenate([clip, np.zeros((max(0, fr - clip.shape[0]),) + clip.shape[1:])]) if clip.shape[0] < fr else clip
    out = np.zeros((plan.windows, grid.tiles, fr, grid.tile, grid.tile, clip.shape[-1]))
    for w, st in enumerate(plan.starts):
        for k in range(grid.tiles):
            y0, x0 = grid.origin(k)
            yi = np.minimum(np.arange(y0, y0 + grid.tile), grid.height - 1)
            xi = np.minimum(np.arange(x0, x0 + grid.tile), grid.width - 1)
            out[w, k] = padded[st:st + fr][:, yi][:, :, xi]
    return out


@pytest.mark.parametrize("length,frames,o,hw,s,so", [(9, 4, 2, (40, 48), 64, 16), (9, 4, 2, (70, 100), 32, 8), (5, 4, 2, (33, 90), 16, 0),
                                                     (3, 4, 2, (20, 20), 16, 4), (13, 4, 1, (49, 40), 32, 16), (8, 4, 0, (30, 30), 32, 0)])
def test_composed_blend_of_window_crops_is_the_clip(length, frames, o, hw, s, so):
    plan, grid = WindowPlan(length, frames, o), TileGrid(hw[0], hw[1], s, so)
    rng = np.random.default_rng(length * 7 + sum(hw))
    clip = rng.random((length,) + hw + (3,))
    got = blend_windows(torch.from_numpy(window_crops(clip, plan, grid)), plan, grid)
    assert got.dtype == torch.float64 and got.shape == clip.shape
    assert np.abs(got.numpy() - clip).max() <= 1e-12
    if length == 9 and frames == 4:                   # a frame in three windows
        assert max(len(plan.covering(f)) for f in range(length)) == 3


def test_composed_blend_matches_restatement():
    plan, grid = WindowPlan(9, 4, 2), TileGrid(30, 40, 16, 4)
    rng = np.random.default_rng(2)
    tiles = rng.random((plan.windows, grid.tiles, 4, 16, 16, 2))
    got = blend_windows(torch.from_numpy(tiles), plan, grid).numpy()
    np.testing.assert_allclose(got, ref_blend_windows(tiles, plan, grid), rtol=1e-12, atol=1e-12)


def ref_tmse(x, y):
    x = np.clip(np.asarray(x, dtype=np.float64), 0, 1)
    y = np.clip(np.asarray(y, dtype=np.float64), 0, 1)
    d = (y[:, 1:] - y[:, :-1]) - (x[:, 1:] - x[:, :-1])
    return (d ** 2).mean(axis=(2, 3, 4))


@pytest.mark.parametrize("shape", [(2, 5, 12, 13, 3), (1, 1, 8, 8, 3), (1, 3, 5, 7, 1), (1, 2, 4, 4, 4)])
def test_tmse_cpu_matches_numpy(shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.rand(shape, generator=g) * 1.2 - 0.1
    y = x + 0.2 * torch.randn(shape, generator=g)
    got = temporal_mse(x, y)
    assert got.dtype == torch.float32 and got.shape == (shape[0], shape[1] - 1)
    np.testing.assert_allclose(got.double().numpy(), ref_tmse(x.numpy(), y.numpy()), rtol=1e-6, atol=1e-12)
    assert torch.equal(temporal_mse(x, x), torch.zeros_like(got))


def test_temporal_summary():
    v = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]      # pairs (t - 1, t) for t = 1 .. 8; seams at t = 4, 8
    s = temporal_summary(np.array(v), 4)
    assert s == {"tmse": 4.5, "tmse_seam": 6.0, "tmse_inner": 4.0, "pairs": 8, "seam_pairs": 2}
    assert temporal_summary(np.zeros(0), 4) == {"tmse": 0.0, "tmse_seam": 0.0, "tmse_inner": 0.0, "pairs": 0, "seam_pairs": 0}


@pytest.mark.parametrize("length,frames,o,grid", [(9, 4, 2, TileGrid(100, 150, 64, 16)), (5, 8, 2, TileGrid(64, 64, 64, 0))])
def test_pack_unpack_latents_windows_round_trip(length, frames, o, grid):
    plan = WindowPlan(length, frames, o)
    fw = min(frames, length)
    n, k, hw, ld = plan.windows, grid.tiles, 4, 6
    rng = np.random.default_rng(length)
    mean = torch.from_numpy(rng.standard_normal((n, k, fw, hw, ld)).astype(np.float32)).to(torch.bfloat16)
    lv = torch.from_numpy(rng.standard_normal((n, k, fw, hw, ld)).astype(np.float32))
    sel = torch.from_numpy((rng.random((n, k, fw)) > 0.4).astype(np.float32))
    sel[0, 0] = 1
    sel[-1, -1, 0] = 0
    fill = torch.randn(ld)
    arrays = pack_latents_windows(mean, sel, grid, plan, lv)
    assert arrays["window_starts"].dtype == np.int64 and arrays["window_starts"].tolist() == plan.starts
    assert int(arrays["temporal_overlap"]) == o and int(arrays["window"]) == frames and int(arrays["n_frames"]) == length
    assert list(arrays["tile_grid"]) == list(grid.as_array())
    assert arrays["selection"].dtype == np.uint8 and arrays["selection"].shape == (n, k, fw)
    keep = sel.numpy() != 0
    np.testing.assert_array_equal(arrays["mean"], mean.float().numpy()[keep])            # window, tile, frame order
    np.testing.assert_array_equal(arrays["log_variance"], lv.numpy()[keep])
    comp, s2, g2, p2 = unpack_latents_windows(arrays, fill)
    assert g2 == grid and p2 == plan and comp.shape == (n, k, fw, hw, ld)
    np.testing.assert_array_equal(s2, keep.astype(np.uint8))
    np.testing.assert_array_equal(comp[keep], mean.float().numpy()[keep])
    np.testing.assert_array_equal(comp[~keep], np.broadcast_to(fill.numpy(), comp[~keep].shape))
    for key, bad in (("mean", arrays["mean"][1:]), ("window_starts", arrays["window_starts"] + 1),
                     ("selection", arrays["selection"][:, :, :-1]), ("temporal_overlap", np.int64(frames)),
                     ("n_frames", np.int64(length + 1))):
        broken = dict(arrays, **{key: bad})
        with pytest.raises(ValueError):
            unpack_latents_windows(broken, fill)
    with pytest.raises(ValueError):
        pack_latents_windows(mean, sel[:, :, :-1], grid, plan)
