"""The latent quantiser on the host: the numpy reference (video_vae_amd/quant.py), the rate summary, the quantised latent files of the three
formats and the parser.  No GPU."""
import numpy as np
import pytest
import torch

from video_vae_amd import infer as I
from video_vae_amd.quant import dequantise_reference, quantise_reference, rate_dataset, rate_summary, qmax_of
from video_vae_amd.tiling import ScenePlan, TileGrid, WindowPlan

BITS = (2, 4, 8)
HW, LD = 16, 24


def _bf16(a):
    """float32 values that bf16 represents exactly (what the encoder's means are)."""
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def _latent(frames, seed, hw=HW, ld=LD):
    rng = np.random.default_rng(seed)
    x = _bf16(rng.standard_normal((frames, hw, ld)) * rng.uniform(0.01, 3.0, size=(frames, 1, ld)))
    x[:, :, 1] = 0.0                                       # a dead channel
    x[:, 3, 2] = 1000.0                                    # a channel with one huge outlier
    x[:, :, 4] = -np.abs(x[:, :, 4])                       # a channel whose maximum is negative
    return x


@pytest.mark.parametrize("bits", BITS)
def test_reference_properties(bits):
    qmax = qmax_of(bits)
    assert qmax == 2 ** (bits - 1) - 1
    x = _latent(3, bits)
    q, step = quantise_reference(x, bits)
    assert q.dtype == np.int8 and q.shape == x.shape and step.dtype == np.float32 and step.shape == (3, LD)
    assert int(q.min()) >= -qmax and int(q.max()) <= qmax
    xq = dequantise_reference(q, step)
    assert xq.dtype == np.float32
    # |xq - x| <= 0.5 step (1 + 2^-10): half a step, plus the roundings of inv, step and the two products (a relative 2^-23 times at
    # most qmax = 127, far below 2^-10); evaluated in float64 so that the check itself adds nothing
    bound = 0.5 * step.astype(np.float64)[:, None, :] * (1 + 2.0 ** -10)
    assert np.all(np.abs(xq.astype(np.float64) - x.astype(np.float64)) <= bound)
    # the zero channel: step 0, codes 0
    assert np.all(step[:, 1] == 0) and np.all(q[:, :, 1] == 0) and np.all(xq[:, :, 1] == 0)
    # amax itself maps to +-qmax
    amax = np.abs(x).max(axis=1)
    for f in range(3):
        for c in range(LD):
            if c == 1:
                continue
            i = int(np.argmax(np.abs(x[f, :, c])))
            assert q[f, i, c] == (qmax if x[f, i, c] > 0 else -qmax), (f, c)
            assert step[f, c] == np.float32(amax[f, c]) / np.float32(qmax)
    assert np.all(q[:, 3, 2] == qmax) and np.all(q[:, :, 4] <= 0) and np.all(q[:, :, 4].min(axis=1) == -qmax)
    # a single frame (hw, ld) gives that frame's row
    q1, s1 = quantise_reference(x[1], bits)
    assert np.array_equal(q1, q[1]) and np.array_equal(s1[0], step[1])


@pytest.mark.parametrize("bits", BITS)
def test_reference_ties_round_to_even(bits):
    """A channel with amax == qmax has inv == 1, so entries k + 0.5 (exact in bf16 for k < 128) are ties: they go to the even neighbour."""
    qmax = qmax_of(bits)
    k = np.arange(0, qmax, dtype=np.float32)
    ties = np.concatenate([k + 0.5, -(k + 0.5), [qmax]]).astype(np.float32)
    assert np.array_equal(_bf16(ties), ties)
    x = np.zeros((1, ties.size, 8), dtype=np.float32)
    x[0, :, 0] = ties
    q, step = quantise_reference(x, bits)
    assert step[0, 0] == 1.0
    want = np.concatenate([2 * np.round((k + 0.5) / 2), -2 * np.round((k + 0.5) / 2), [qmax]])      # the even neighbour of k + 0.5
    want = np.clip(want, -qmax, qmax)
    assert np.array_equal(q[0, :, 0].astype(np.float64), want)
    for kk in range(qmax):
        assert q[0, kk, 0] == (kk if kk % 2 == 0 else min(kk + 1, qmax))


def test_reference_dead_channels_and_refusals():
    x = np.ones((2, 4, 8), dtype=np.float32)
    x[0, 1, 0] = np.inf
    x[0, 2, 1] = np.nan
    x[1, :, 2] = 1e-31
    q, step = quantise_reference(x, 8)
    assert step[0, 0] == 0 and step[0, 1] == 0 and step[1, 2] == 0 and np.all(q[0, :, :2] == 0) and np.all(q[1, :, 2] == 0)
    assert step[1, 0] == np.float32(1) / np.float32(127) and np.all(q[1, :, 0] == 127)
    assert np.all(dequantise_reference(q, step)[0, :, :2] == 0)
    for bad in (1, 9):
        with pytest.raises(ValueError):
            quantise_reference(x, bad)
    with pytest.raises(ValueError):
        dequantise_reference(q, step[:1])


def test_rate_summary_on_hand_made_counts():
    counts = np.zeros(256, dtype=np.int64)
    counts[[100, 128, 129, 200]] = 6                       # four equally likely symbols: exactly 2 bits per code
    sel = np.array([1, 0, 1, 0, 0])
    r = rate_summary(counts, sel, n_frames=5, height=4, width=6, ld=3, bits=8)
    assert r["codes"] == 24 and r["kept"] == 2 and r["pixels"] == 120
    assert r["bits_raw"] == 24 * 8 and r["bits_entropy"] == 48.0 and r["bits_side"] == 2 * 3 * 32 + 5
    assert r["bpp_raw"] == (192 + 197) / 120 and r["bpp_entropy"] == (48 + 197) / 120
    one = np.zeros((2, 256), dtype=np.int64)               # a single symbol costs nothing; per-frame rows are pooled
    one[0, 128], one[1, 128] = 10, 20
    s = rate_summary(one, np.ones(2), n_frames=2, height=8, width=8, ld=3, bits=4)
    assert s["codes"] == 30 and s["bits_entropy"] == 0.0 and s["bits_raw"] == 120 and s["bpp_entropy"] == s["bits_side"] / 128
    none = rate_summary(np.zeros(256), np.zeros(3), n_frames=3, height=2, width=2, ld=3, bits=4)
    assert none["bits_raw"] == 0 and none["bits_entropy"] == 0.0 and none["bits_side"] == 3
    d = rate_dataset([r, s])                               # ratios of sums, not means of ratios
    assert d["pixels"] == 248 and d["bits_side"] == r["bits_side"] + s["bits_side"]
    assert d["bpp_raw"] == (r["bits_raw"] + s["bits_raw"] + d["bits_side"]) / 248
    assert d["bpp_entropy"] == (48.0 + 0.0 + d["bits_side"]) / 248
    assert abs(d["bpp_raw"] - (r["bpp_raw"] + s["bpp_raw"]) / 2) > 1e-3         # the mean of ratios is another number
    skew = np.zeros(256, dtype=np.int64)
    skew[128], skew[129] = 3, 1
    h = rate_summary(skew, np.ones(1), 1, 2, 2, 4, 2)["bits_entropy"] / 4
    assert abs(h - (0.75 * np.log2(4 / 3) + 0.25 * 2)) < 1e-12


# ------------------------------------------------------------------------------------------------ latent files
FILL = torch.linspace(-0.5, 0.5, LD)


def _check_dense(comp, sel, x, kept, bits):
    """comp (..., hw, ld) equals the dequantised reference on the kept frames (``kept`` bool, shaped like sel) and the fill token elsewhere."""
    assert np.array_equal(sel != 0, kept)
    flat, xs, kp = comp.reshape((-1,) + comp.shape[-2:]), x.reshape((-1,) + x.shape[-2:]), kept.reshape(-1)
    q, step = quantise_reference(xs, bits)
    want = dequantise_reference(q, step)
    assert comp.dtype == np.float32
    for f in range(flat.shape[0]):
        if kp[f]:
            assert np.array_equal(flat[f], want[f]), f
        else:
            assert np.array_equal(flat[f], np.broadcast_to(FILL.numpy(), flat[f].shape)), f


def _quant(x, bits):
    """Dense (codes, step, bits) shaped like x, as the kernel hands them over."""
    q, step = quantise_reference(x.reshape((-1,) + x.shape[-2:]), bits)
    return torch.from_numpy(q.reshape(x.shape)), torch.from_numpy(step.reshape(x.shape[:-2] + x.shape[-1:])), bits


@pytest.mark.parametrize("bits", (4, 8))
def test_pack_unpack_plain(bits, tmp_path):
    x = _latent(5, 10)
    sel = np.array([1, 0, 1, 1, 0], dtype=np.float32)
    arrays = I.pack_latents(torch.from_numpy(x), torch.from_numpy(sel), quant=_quant(x, bits))
    assert "mean" not in arrays and arrays["mean_q"].dtype == np.int8 and arrays["mean_q"].shape == (3, HW, LD)
    assert arrays["mean_step"].dtype == np.float32 and arrays["mean_step"].shape == (3, LD) and int(arrays["quant_bits"]) == bits
    q, step = quantise_reference(x[sel != 0], bits)
    assert np.array_equal(arrays["mean_q"], q) and np.array_equal(arrays["mean_step"], step)
    nbytes = I.save_latents(str(tmp_path / "a.npz"), arrays)           # deflated, and read back through the file
    assert 0 < nbytes < arrays["mean_q"].nbytes + arrays["mean_step"].nbytes + 2048
    with np.load(tmp_path / "a.npz") as z:
        back = {k: z[k] for k in z.files}
    comp, s = I.unpack_latents(back, FILL)
    _check_dense(comp, s, x, sel != 0, bits)
    bad = dict(arrays, mean_q=arrays["mean_q"][:2], mean_step=arrays["mean_step"][:2])
    with pytest.raises(ValueError):
        I.unpack_latents(bad, FILL)
    with pytest.raises(ValueError):
        I.unpack_latents(dict(arrays, mean_step=arrays["mean_step"][:2]), FILL)


def test_pack_unpack_tiled_and_windows():
    bits = 6
    grid = TileGrid(40, 56, 32, 8)
    assert grid.tiles == 4
    x = _latent(4 * 5, 11).reshape(4, 5, HW, LD)
    sel = (np.random.default_rng(0).random((4, 5)) < 0.6)
    arrays = I.pack_latents_tiled(torch.from_numpy(x), torch.from_numpy(sel.astype(np.float32)), grid, quant=_quant(x, bits))
    assert "mean" not in arrays and arrays["mean_q"].shape == (int(sel.sum()), HW, LD)
    q, step = quantise_reference(x[sel], bits)                         # tile-major then frame order, as today's mean rows
    assert np.array_equal(arrays["mean_q"], q) and np.array_equal(arrays["mean_step"], step)
    comp, s, g = I.unpack_latents_tiled(arrays, FILL)
    assert g == grid
    _check_dense(comp, s, x, sel, bits)
    with pytest.raises(ValueError):
        I.unpack_latents_tiled(dict(arrays, mean_q=arrays["mean_q"][1:], mean_step=arrays["mean_step"][1:]), FILL)
    # windows, plain plan
    one = TileGrid(32, 32, 32, 0)
    plan = WindowPlan(10, 4, 1)
    xw = _latent(plan.windows * 4, 12).reshape(plan.windows, 1, 4, HW, LD)
    selw = np.random.default_rng(1).random((plan.windows, 1, 4)) < 0.7
    arrays = I.pack_latents_windows(torch.from_numpy(xw), torch.from_numpy(selw.astype(np.float32)), one, plan, quant=_quant(xw, bits))
    q, step = quantise_reference(xw[selw], bits)
    assert np.array_equal(arrays["mean_q"], q) and np.array_equal(arrays["mean_step"], step) and "scene_cuts" not in arrays
    comp, s, g, p = I.unpack_latents_windows(arrays, FILL)
    assert p == plan and g == one
    _check_dense(comp, s, xw, selw, bits)
    with pytest.raises(ValueError):
        I.unpack_latents_windows(dict(arrays, mean_q=arrays["mean_q"][:-1], mean_step=arrays["mean_step"][:-1]), FILL)
    # scenes: the padded frames of a short scene's window are stored as not kept
    sp = ScenePlan(10, 4, 0, [3])
    assert sp.counts[0] == 3
    xs = _latent(sp.windows * 4, 13).reshape(sp.windows, 1, 4, HW, LD)
    sels = np.ones((sp.windows, 1, 4), dtype=bool)
    arrays = I.pack_latents_windows(torch.from_numpy(xs), torch.from_numpy(sels.astype(np.float32)), one, sp, quant=_quant(xs, bits))
    kept = sels.copy()
    for w, c in enumerate(sp.counts):
        kept[w, :, c:] = False
    assert not kept.all() and arrays["mean_q"].shape[0] == int(kept.sum()) and arrays["scene_cuts"].tolist() == [3]
    comp, s, g, p = I.unpack_latents_windows(arrays, FILL)
    assert isinstance(p, ScenePlan) and p == sp
    _check_dense(comp, s, xs, kept, bits)


def test_unquantised_files_are_what_they_were():
    """Without ``quant`` the three packers give the arrays they always gave (names, order, dtypes, values) and unpack as before."""
    x = _latent(5, 14)
    sel = np.array([1, 1, 0, 1, 0], dtype=np.float32)
    a = I.pack_latents(torch.from_numpy(x), torch.from_numpy(sel), torch.from_numpy(x * 2))
    assert list(a) == ["mean", "selection", "n_frames", "log_variance"]
    assert a["mean"].dtype == np.float32 and np.array_equal(a["mean"], x[sel != 0]) and np.array_equal(a["log_variance"], 2 * x[sel != 0])
    comp, s = I.unpack_latents(a, FILL)
    assert np.array_equal(comp[sel != 0], x[sel != 0]) and np.array_equal(comp[1 + 1], np.broadcast_to(FILL.numpy(), (HW, LD)))
    assert s.tolist() == [1, 1, 0, 1, 0]
    grid = TileGrid(40, 56, 32, 8)
    xt = _latent(20, 15).reshape(4, 5, HW, LD)
    selt = np.random.default_rng(2).random((4, 5)) < 0.5
    a = I.pack_latents_tiled(torch.from_numpy(xt), torch.from_numpy(selt.astype(np.float32)), grid)
    assert list(a) == ["tile_grid", "mean", "selection", "n_frames"] and np.array_equal(a["mean"], xt[selt])
    comp, s, _ = I.unpack_latents_tiled(a, FILL)
    assert np.array_equal(comp[selt], xt[selt]) and np.array_equal(s != 0, selt)
    plan = WindowPlan(10, 4, 1)
    xw = _latent(plan.windows * 4, 16).reshape(plan.windows, 1, 4, HW, LD)
    selw = np.random.default_rng(3).random((plan.windows, 1, 4)) < 0.5
    a = I.pack_latents_windows(torch.from_numpy(xw), torch.from_numpy(selw.astype(np.float32)), TileGrid(32, 32, 32, 0), plan)
    assert list(a) == ["tile_grid", "window_starts", "temporal_overlap", "window", "n_frames", "mean", "selection"]
    comp, s, _, _ = I.unpack_latents_windows(a, FILL)
    assert np.array_equal(comp[selw], xw[selw]) and np.array_equal(s != 0, selw)


# ------------------------------------------------------------------------------------------------ parser
def test_parser_quantise_bits(capsys):
    enc = ["encode", "--model_path", "ck", "--data", "d", "--out", "o"]
    ev = ["eval", "--model_path", "ck", "--data", "d"]
    for cmd in (enc, ev):
        assert I.parse_args(cmd).quantise_bits is None
        for n in range(2, 9):
            assert I.parse_args(cmd + ["--quantise-bits", str(n)]).quantise_bits == n
        for bad in ("1", "9", "0", "-3", "x"):
            with pytest.raises(SystemExit) as e:
                I.parse_args(cmd + ["--quantise-bits", bad])
            assert e.value.code == 2
    for extra in (["--tile"], ["--temporal-overlap", "2"], ["--scene-cuts"], ["--tile", "--temporal-overlap", "0", "--scene-cuts"]):
        assert I.parse_args(enc + ["--quantise-bits", "6"] + extra).quantise_bits == 6
        with pytest.raises(SystemExit) as e:                # eval: plain mode only, and the message says why
            I.parse_args(ev + ["--quantise-bits", "6"] + extra)
        assert e.value.code == 2
    assert "plain mode only" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        I.parse_args(enc + ["--quantise-bits", "6", "--with-logvar"])
    assert e.value.code == 2
    assert "--with-logvar" in capsys.readouterr().err
    with pytest.raises(SystemExit):                        # decode needs no flag: the file says what it is
        I.parse_args(["decode", "--model_path", "ck", "--latents", "l", "--out", "o", "--quantise-bits", "6"])


def test_graphed_inference_refuses_quant_bits_elsewhere():
    with pytest.raises(ValueError):
        I.GraphedInference(None, None, 1, 1, "decode", quant_bits=8)
    with pytest.raises(ValueError):
        I.GraphedInference(None, None, 1, 1, "reconstruct", quant_bits=8)


def test_latent_quantise_fails_loudly_without_gpu():
    from video_vae_amd import ops
    from video_vae_amd._lib import VvaeError
    with pytest.raises(VvaeError):
        ops.latent_quantise(torch.zeros(2, 4, 8), torch.ones(2), 8)
