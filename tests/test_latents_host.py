"""CPU: the three latent-file formats (video_vae_amd/latents.py) against tests/golden/latent_formats.json, recorded from the functions as
they were before they shared one core (tests/golden/make_latent_formats.py): the same keys in the same order, the same dtypes, shapes
and bytes, the same dense arrays back; and the malformed files that were refused are still refused."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _maker():
    spec = importlib.util.spec_from_file_location("make_latent_formats", os.path.join(GOLDEN, "make_latent_formats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_formats_equal_the_recorded_ones():
    with open(os.path.join(GOLDEN, "latent_formats.json")) as fh:
        want = json.load(fh)
    got = _maker().record()
    assert sorted(got) == sorted(want) and len(want) == 27
    for name in want:
        assert got[name]["keys"] == want[name]["keys"], name
        for part in ("arrays", "comp", "sel"):
            assert got[name][part] == want[name][part], (name, part)


def test_infer_exports_the_formats():
    """Tests and tools import the formats from video_vae_amd.infer: the very functions of latents.py, not copies."""
    from video_vae_amd import infer, latents
    for name in ("pack_latents", "unpack_latents", "pack_latents_tiled", "unpack_latents_tiled", "pack_latents_windows",
                 "unpack_latents_windows", "save_latents"):
        assert getattr(infer, name) is getattr(latents, name), name


def test_malformed_files_are_refused():
    from video_vae_amd.latents import (pack_latents, pack_latents_tiled, pack_latents_windows, unpack_latents, unpack_latents_tiled,
                                       unpack_latents_windows)
    from video_vae_amd.quant import quantise_reference
    from video_vae_amd.tiling import ScenePlan, TileGrid, WindowPlan
    m = _maker()
    hw, ld, fill, grid = m.HW, m.LD, m.fill_token(), TileGrid(6, 7, 4, 1)
    rng = np.random.default_rng(5)

    def inputs(shape, bits=None):
        x = rng.standard_normal(shape + (hw, ld)).astype(np.float32)
        sel = np.ones(shape, dtype=np.float32)
        sel.reshape(-1)[1] = 0
        if bits is None:
            return torch.from_numpy(x), torch.from_numpy(sel), None
        q, step = quantise_reference(x.reshape(-1, hw, ld), bits)
        return torch.from_numpy(x), torch.from_numpy(sel), (torch.from_numpy(q.reshape(x.shape)), torch.from_numpy(step.reshape(shape + (ld,))), bits)

    def refused(unpack, arrays, **changed):
        with pytest.raises(ValueError):
            unpack(dict(arrays, **changed), fill)

    # a wrong kept count, in every format, float and quantised
    x, sel, _ = inputs((5,))
    a = pack_latents(x, sel)
    refused(unpack_latents, a, mean=a["mean"][1:])
    refused(unpack_latents, a, n_frames=np.int64(6))
    x, sel, quant = inputs((5,), 4)
    a = pack_latents(x, sel, quant=quant)
    refused(unpack_latents, a, mean_q=a["mean_q"][:2], mean_step=a["mean_step"][:2])
    refused(unpack_latents, a, mean_step=a["mean_step"][:2])
    # codes beyond qmax: 4 bits hold -7 .. 7
    assert int(np.abs(a["mean_q"]).max()) == 7
    refused(unpack_latents, a, mean_q=np.where(a["mean_q"] == 7, np.int8(8), a["mean_q"]))
    refused(unpack_latents, a, quant_bits=np.int64(3))
    refused(unpack_latents, a, quant_bits=np.int64(9))
    x, sel, _ = inputs((4, 5))
    a = pack_latents_tiled(x, sel, grid)
    refused(unpack_latents_tiled, a, mean=a["mean"][1:])
    refused(unpack_latents_tiled, a, selection=a["selection"][:, :-1])
    refused(unpack_latents_tiled, a, tile_grid=np.array([6, 7, 4, 1, 2, 3], dtype=np.int64))
    with pytest.raises(ValueError):
        pack_latents_tiled(x[:3], sel[:3], grid)
    x, sel, quant = inputs((4, 5), 4)
    a = pack_latents_tiled(x, sel, grid, quant=quant)
    refused(unpack_latents_tiled, a, mean_q=a["mean_q"][1:], mean_step=a["mean_step"][1:])
    plan = WindowPlan(11, 4, 1)
    x, sel, _ = inputs((plan.windows, 4, 4))
    a = pack_latents_windows(x, sel, grid, plan)
    refused(unpack_latents_windows, a, mean=a["mean"][1:])
    refused(unpack_latents_windows, a, selection=a["selection"][:, :, :-1])
    # starts that do not fit the plan
    refused(unpack_latents_windows, a, window_starts=a["window_starts"] + 1)
    refused(unpack_latents_windows, a, temporal_overlap=np.int64(4))
    refused(unpack_latents_windows, a, n_frames=np.int64(12))
    with pytest.raises(ValueError):
        pack_latents_windows(x, sel[:, :, :-1], grid, plan)
    x, sel, quant = inputs((plan.windows, 4, 4), 4)
    a = pack_latents_windows(x, sel, grid, plan, quant=quant)
    refused(unpack_latents_windows, a, mean_q=a["mean_q"][:-1], mean_step=a["mean_step"][:-1])
    scenes = ScenePlan(11, 4, 1, [3, 7])
    x, sel, _ = inputs((scenes.windows, 4, 4))
    a = pack_latents_windows(x, sel, grid, scenes)
    refused(unpack_latents_windows, a, scene_cuts=np.array([3, 9], dtype=np.int64))
    refused(unpack_latents_windows, a, scene_cuts=np.array([7, 3], dtype=np.int64))
