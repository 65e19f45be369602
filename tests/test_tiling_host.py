"""CPU: the tile grid (the issue's examples, a coverage / minimality sweep), the composed gather and blend against a direct numpy
restatement of the definition in tiling.py, and the tiled latent files' round trip."""
import math

import numpy as np
import pytest
import torch

from video_vae_amd.tiling import TileGrid, axis_starts, axis_tiles, blend_tiles, gather_tiles


def test_grid_examples():
    assert axis_starts(720, 256, 32) == [0, 154, 309, 464]
    assert axis_starts(1280, 256, 32) == [0, 204, 409, 614, 819, 1024]
    assert axis_starts(490, 256, 32) == [0, 117, 234]
    assert sum(s <= 240 < s + 256 for s in axis_starts(490, 256, 32)) == 3
    assert axis_starts(200, 256, 32) == [0] and axis_starts(256, 256, 32) == [0]
    g = TileGrid(720, 1280, 256, 32)
    assert (g.ny, g.nx, g.tiles) == (4, 6, 24)
    assert g.origin(7) == (154, 204)
    with pytest.raises(ValueError):
        TileGrid(720, 1280, 256, 129)


@pytest.mark.parametrize("o", [0, 16, 32, 128])
def test_grid_sweep(o):
    s = 256
    for length in range(11, 2001):
        st = axis_starts(length, s, o)
        n = len(st)
        assert st[0] == 0 and min(st[-1] + s, length) == length and (n == 1 or st[-1] + s == length)
        cover = np.zeros(length, dtype=int)
        for a in st:
            cover[a:a + s] += 1
        assert cover.min() >= 1, length
        for a, b in zip(st, st[1:]):
            assert a + s - b >= o, (length, o, st)
        if n > 1:                                     # n - 1 tiles cannot cover L with neighbours overlapping by o
            assert (n - 1) * s - (n - 2) * o < length, (length, o)
        assert n == axis_tiles(length, s, o)


def ref_blend(tiles, grid):
    """Direct float64 restatement of the blend: per output pixel, the covering tiles in ascending k."""
    tiles = np.asarray(tiles, dtype=np.float64)
    n = tiles.shape[0] // grid.tiles
    t, s, c = tiles.shape[1], grid.tile, tiles.shape[4]
    h, w = grid.height, grid.width

    def wt(i, p, length, st):
        v = 1.0
        if i > 0 and st[i - 1] + s - st[i] > 0:
            v *= min(1.0, (p + 0.5) / (st[i - 1] + s - st[i]))
        if i < len(st) - 1 and st[i] + s - st[i + 1] > 0:
            v *= min(1.0, (s - p - 0.5) / (st[i] + s - st[i + 1]))
        return v

    out = np.zeros((n, t, h, w, c))
    den_min = np.inf
    for y in range(h):
        for x in range(w):
            num, den = np.zeros((n, t, c)), 0.0
            for ty, y0 in enumerate(grid.ys):
                if not y0 <= y < y0 + s:
                    continue
                for tx, x0 in enumerate(grid.xs):
                    if not x0 <= x < x0 + s:
                        continue
                    wk = wt(ty, y - y0, h, grid.ys) * wt(tx, x - x0, w, grid.xs)
                    num += wk * tiles[ty * grid.nx + tx::grid.tiles, :, y - y0, x - x0, :]
                    den += wk
            den_min = min(den_min, den)
            out[:, :, y, x] = num / den
    return out, den_min


def _crops(frame, grid):
    """Tiles of a float64 (N, T, H, W, C) frame, edge-replicated, flat (window, k) order."""
    n = frame.shape[0]
    out = []
    for q in range(n * grid.tiles):
        wdx, k = divmod(q, grid.tiles)
        y0, x0 = grid.origin(k)
        yi = np.minimum(np.arange(y0, y0 + grid.tile), grid.height - 1)
        xi = np.minimum(np.arange(x0, x0 + grid.tile), grid.width - 1)
        out.append(frame[wdx][:, yi][:, :, xi])
    return np.stack(out)


@pytest.mark.parametrize("hw,s,o", [((40, 48), 64, 16), ((70, 100), 32, 8), ((49, 40), 32, 16), ((33, 90), 16, 0)])
def test_composed_blend_of_crops_is_the_frame(hw, s, o):
    g = TileGrid(hw[0], hw[1], s, o)
    rng = np.random.default_rng(sum(hw))
    frame = rng.random((2, 3) + hw + (3,))
    got = blend_tiles(torch.from_numpy(_crops(frame, g)), g)
    assert got.dtype == torch.float64
    assert np.abs(got.numpy() - frame).max() <= 1e-12


def test_composed_blend_matches_restatement():
    g = TileGrid(70, 100, 32, 12)                    # several tiles per axis, overlaps of unequal size
    rng = np.random.default_rng(3)
    tiles = rng.random((2 * g.tiles, 2, 32, 32, 2))
    want, den_min = ref_blend(tiles, g)
    got = blend_tiles(torch.from_numpy(tiles), g).numpy()
    assert den_min > 0
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


def test_three_tile_overlap_weights():
    """L = 490, S = 256, o = 32: column 240 lies in three tiles; every pixel's total weight is positive, and where exactly two tiles
    overlap the weights sum to 1."""
    st = axis_starts(490, 256, 32)
    g = TileGrid(64, 490, 256, 32)
    tot = np.zeros(490)
    cnt = np.zeros(490, dtype=int)
    for i, a in enumerate(st):
        tot[a:a + 256] += g.weights_x[i]
        cnt[a:a + 256] += 1
    assert cnt[240] == 3 and tot.min() > 0
    np.testing.assert_allclose(tot[cnt == 2], 1.0, atol=1e-12)


def test_composed_gather_replicates_edges():
    g = TileGrid(40, 48, 64, 16)
    rng = np.random.default_rng(0)
    u8 = torch.from_numpy(rng.integers(0, 256, (2, 3, 40, 48, 3), dtype=np.uint8))
    tiles = gather_tiles(u8, g)
    assert tiles.shape == (2, 3, 64, 64, 3) and tiles.dtype == torch.float32
    assert torch.equal(tiles[:, :, :40, :48], u8.float() / 255)
    assert torch.equal(tiles[:, :, 50, 60], u8[:, :, 39, 47].float() / 255)


def test_pack_unpack_latents_tiled_round_trip():
    from video_vae_amd.infer import pack_latents_tiled, unpack_latents_tiled
    g = TileGrid(100, 150, 64, 16)
    k, n, hw, ld = g.tiles, 7, 4, 6
    rng = np.random.default_rng(1)
    mean = torch.from_numpy(rng.standard_normal((k, n, hw, ld)).astype(np.float32)).to(torch.bfloat16)
    lv = torch.from_numpy(rng.standard_normal((k, n, hw, ld)).astype(np.float32))
    sel = torch.from_numpy((rng.random((k, n)) > 0.4).astype(np.float32))
    sel[0] = 1
    sel[1] = 0
    sel[2, 3] = 0                                     # tiles keep different frames
    fill = torch.randn(ld)
    arrays = pack_latents_tiled(mean, sel, g, lv)
    assert arrays["tile_grid"].dtype == np.int64 and list(arrays["tile_grid"]) == [100, 150, 64, 16, g.ny, g.nx]
    assert arrays["selection"].dtype == np.uint8 and arrays["selection"].shape == (k, n)
    assert arrays["mean"].dtype == np.float32 and arrays["mean"].shape == (int(sel.sum()), hw, ld)
    keep = sel.numpy() != 0
    np.testing.assert_array_equal(arrays["mean"], mean.float().numpy()[keep])     # tile-major, then frame order
    np.testing.assert_array_equal(arrays["log_variance"], lv.numpy()[keep])
    comp, s2, g2 = unpack_latents_tiled(arrays, fill)
    assert g2 == g and comp.shape == (k, n, hw, ld)
    np.testing.assert_array_equal(s2, keep.astype(np.uint8))
    np.testing.assert_array_equal(comp[keep], mean.float().numpy()[keep])
    np.testing.assert_array_equal(comp[~keep], np.broadcast_to(fill.numpy(), comp[~keep].shape))
    arrays["mean"] = arrays["mean"][1:]
    with pytest.raises(ValueError):
        unpack_latents_tiled(arrays, fill)


def test_pixel_ratio():
    g = TileGrid(720, 1280, 256, 32)
    assert math.isclose(g.pixel_ratio(), 24 * 256 * 256 / (720 * 1280))
