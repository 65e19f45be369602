"""CPU: multi-scale SSIM (video_vae_amd.metrics.ms_ssim) -- the composed framework-op path against a float64 numpy restatement of the
definition (the fp32 2 x 2 pool with its dropped odd row and column included), closed forms, masks and refusals, the infer eval flags and
the ABI entries of the kernels.  No HIP compute runs here."""
import ctypes
import functools

import numpy as np
import pytest
import torch

W5 = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 0.01 ** 2, 0.03 ** 2

# (B, T, H, W, C), scales: what each is there for is said in tests/test_gpu_ms_ssim.py, which runs the same list on the GPU
CASES = [((1, 2, 44, 47, 3), 3), ((2, 3, 45, 44, 1), 3), ((1, 1, 22, 23, 4), 2), ((2, 2, 48, 48, 3), 3), ((1, 1, 176, 176, 3), 5),
         ((1, 2, 181, 203, 4), 5), ((1, 1, 24, 700, 3), 2), ((1, 2, 24, 1400, 3), 2), ((4, 16, 256, 256, 3), 5)]
CASE_IDS = ["x".join(map(str, s)) + f"-m{m}" for s, m in CASES]


# ------------------------------------------------------------------------------ the definition, restated in numpy
def _taps():
    k = np.arange(11, dtype=np.float64) - 5
    g = np.exp(-k * k / (2 * 1.5 ** 2))
    return g / g.sum()


def ref_pool(v):
    """fp32 (H, W, C) -> (H // 2, W // 2, C): ((v00 + v01) + (v10 + v11)) * 0.25 in fp32, an odd trailing row or column dropped."""
    assert v.dtype == np.float32
    h2, w2 = v.shape[0] // 2 * 2, v.shape[1] // 2 * 2
    v = v[:h2, :w2]
    return ((v[0::2, 0::2] + v[0::2, 1::2]) + (v[1::2, 0::2] + v[1::2, 1::2])) * np.float32(0.25)


def ref_level(x, y):
    """One level, fp32 (H, W, C) each -> float64 (cs[c], ssim[c]): the means over the valid positions of CS and S per channel."""
    x, y = x.astype(np.float64), y.astype(np.float64)
    g = _taps()
    h, w = x.shape[:2]

    def filt(a):
        r = sum(g[k] * a[k:h - 10 + k] for k in range(11))
        return sum(g[k] * r[:, k:w - 10 + k] for k in range(11))
    ux, uy = filt(x), filt(y)
    vx, vy, vxy = filt(x * x) - ux * ux, filt(y * y) - uy * uy, filt(x * y) - ux * uy
    cs = (2 * vxy + C2) / (vx + vy + C2)
    s = (2 * ux * uy + C1) / (ux * ux + uy * uy + C1) * cs
    return cs.mean(axis=(0, 1)), s.mean(axis=(0, 1))


def ref_frame(x, y, weights, clamp=True):
    """One frame pair (H, W, C) -> (ms_ssim, terms (M, C)), float64."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    if clamp:
        x, y = np.clip(x, 0, 1), np.clip(y, 0, 1)
    m = len(weights)
    terms = np.zeros((m, x.shape[2]))
    for j in range(m):
        cs, s = ref_level(x, y)
        terms[j] = s if j == m - 1 else cs
        if j < m - 1:
            x, y = ref_pool(x), ref_pool(y)
    per_channel = np.prod(np.maximum(terms, 0.0) ** np.asarray(weights, np.float64)[:, None], axis=0)
    return float(per_channel.mean()), terms


def ref_ms_ssim(video, recon, mask, weights, clamp=True):
    """(B, T, H, W, C) pairs and a (B, T) mask -> float64 ms_ssim (B, T) and terms (B, T, M, C), 0 on masked frames (never read)."""
    video = torch.as_tensor(video).float().numpy()
    recon = torch.as_tensor(recon).float().numpy()
    mask = np.asarray(torch.as_tensor(mask).float())
    ms = np.zeros(mask.shape)
    terms = np.zeros(mask.shape + (len(weights), video.shape[4]))
    for b in range(mask.shape[0]):
        for t in range(mask.shape[1]):
            if mask[b, t] != 0:
                ms[b, t], terms[b, t] = ref_frame(video[b, t], recon[b, t], weights, clamp)
    return ms, terms


# ------------------------------------------------------------------------------ inputs shared with the GPU tests
def make_pair(shape, a, seed=0):
    """x: uniform noise smoothed by a 5 x 5 box with replicate padding; y = clamp(x + a N(0, 1)); a mask with at least one dropped
    frame wherever B T > 1 -> fp32 tensors."""
    rng = np.random.default_rng(seed)
    b, t, h, w, c = shape
    u = rng.random((b, t, h, w, c))
    p = np.pad(u, ((0, 0), (0, 0), (2, 2), (2, 2), (0, 0)), mode="edge")
    x = sum(p[:, :, i:i + h, j:j + w] for i in range(5) for j in range(5)) / 25.0
    y = np.clip(x + a * rng.standard_normal(shape), 0.0, 1.0)
    mask = np.ones((b, t), np.float32)
    if b * t > 1:
        mask.reshape(-1)[(b * t) // 2] = 0
        if b * t >= 16:
            mask.reshape(-1)[3::4] = 0
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(y.astype(np.float32)), torch.from_numpy(mask)


@functools.lru_cache(maxsize=None)
def case_reference(shape, scales, a, dx, dy, seed=0):
    """The inputs of a case in the dtypes (dx, dy) and their float64 reference, computed once -> (x, y, mask, ms, terms)."""
    x, y, mask = make_pair(shape, a, seed)
    x, y = x.to(dx), y.to(dy)
    ms, terms = ref_ms_ssim(x, y, mask, W5[:scales])
    return x, y, mask, ms, terms


def assert_conditioned(terms, mask):
    """Every per-level, per-channel term of the reference is >= 0.02: the powers are well-conditioned, max(., 0) never acts."""
    valid = np.asarray(mask) != 0
    assert terms[valid].min() >= 0.02, terms[valid].min()


# ------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("shape,scales", CASES, ids=CASE_IDS)
def test_composed_matches_numpy_restatement(shape, scales):
    from video_vae_amd.metrics import ms_ssim
    x, y, mask, ref, ref_terms = case_reference(shape, scales, 0.1, torch.float32, torch.bfloat16)
    assert_conditioned(ref_terms, mask)
    ms, terms = ms_ssim(x, y, mask, weights=W5[:scales], return_terms=True)
    assert ms.dtype == torch.float32 and ms.shape == shape[:2]
    assert terms.dtype == torch.float32 and terms.shape == shape[:2] + (scales, shape[4])
    # the outputs are fp32: the float64 values agree far below an fp32 ulp, so they round to the reference's own fp32 values
    r32 = lambda v: v.astype(np.float32).astype(np.float64)
    assert np.abs(ms.double().numpy() - r32(ref)).max() <= 1e-10
    assert np.abs(terms.double().numpy() - r32(ref_terms)).max() <= 1e-10
    assert torch.all(ms[mask == 0] == 0) and torch.all(terms[mask == 0] == 0)


def test_identical_operands_give_one():
    from video_vae_amd.metrics import ms_ssim
    x, _, _ = make_pair((1, 2, 48, 50, 3), 0.1, seed=1)
    ms, terms = ms_ssim(x, x.clone(), torch.ones(1, 2), weights=W5[:3], return_terms=True)
    assert np.abs(ms.double().numpy() - 1.0).max() <= 1e-12
    assert np.abs(terms.double().numpy() - 1.0).max() <= 1e-12


def test_constant_frames_closed_form():
    """x = 0.5, y = 0.25: every CS is 1 and the last level's S is the luminance term, so ms_ssim = l^w2."""
    from video_vae_amd.metrics import ms_ssim
    x, y = torch.full((1, 1, 44, 44, 3), 0.5), torch.full((1, 1, 44, 44, 3), 0.25)
    lum = (2 * 0.5 * 0.25 + C1) / (0.25 + 0.0625 + C1)
    want = lum ** 0.3001
    assert abs(want - 0.93525) < 1e-5
    ms, terms = ms_ssim(x, y, torch.ones(1, 1), weights=W5[:3], return_terms=True)
    # fp32 output: the float64 value rounds to the closed form's fp32 value
    assert abs(float(ms) - float(np.float32(want))) <= 1e-9
    assert np.abs(terms[0, 0, :2].double().numpy() - 1.0).max() <= 1e-9
    assert np.abs(terms[0, 0, 2].double().numpy() - float(np.float32(lum))).max() <= 1e-9


def test_one_scale_is_ssim():
    from video_vae_amd.metrics import frame_metrics, ms_ssim
    x, y, mask = make_pair((2, 2, 24, 31, 3), 0.1, seed=2)
    ms = ms_ssim(x, y, mask, weights=(1.0,))
    assert np.abs(ms.double().numpy() - frame_metrics(x, y, mask).ssim.double().numpy()).max() <= 1e-6


def test_pool_of_a_hand_written_level():
    from video_vae_amd.metrics import pool2x2
    v = torch.tensor([[1.0, 3.0, 2.0, 2.0, 9.0],
                      [5.0, 7.0, 0.0, 4.0, 9.0],
                      [0.5, 0.5, 8.0, 6.0, 9.0],
                      [1.5, 1.5, 2.0, 0.0, 9.0],
                      [9.0, 9.0, 9.0, 9.0, 9.0]]).view(5, 5, 1)
    got = pool2x2(v)
    assert got.shape == (2, 2, 1) and got.dtype == torch.float32
    assert got.view(2, 2).tolist() == [[4.0, 2.0], [1.0, 4.0]]
    assert np.array_equal(ref_pool(v.numpy()), got.numpy())
    two = torch.stack([v, 2 * v]).view(1, 2, 5, 5, 1)                 # leading dimensions and channels pass through
    assert pool2x2(two)[0, 1].view(2, 2).tolist() == [[8.0, 4.0], [2.0, 8.0]]


def test_weights_are_used_as_given():
    from video_vae_amd.metrics import ms_ssim
    x, y, mask = make_pair((1, 1, 44, 44, 3), 0.1, seed=3)
    _, terms = ms_ssim(x, y, mask, weights=W5[:3], return_terms=True)
    t = terms[0, 0].double().numpy()
    for w in ((2.0, 0.0, 0.5), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)):
        want = np.prod(t ** np.asarray(w)[:, None], axis=0).mean()
        assert abs(float(ms_ssim(x, y, mask, weights=w)) - want) <= 1e-6


def test_masked_frames_are_zero_even_when_nan():
    from video_vae_amd.metrics import ms_ssim
    x, y, _ = make_pair((2, 3, 22, 22, 3), 0.1, seed=4)
    mask = torch.tensor([[1.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
    x[0, 1] = float("nan")
    y[1] = float("nan")
    ms, terms = ms_ssim(x, y, mask, weights=W5[:2], return_terms=True)
    assert terms.shape == (2, 3, 2, 3)
    for v in (ms, terms):
        assert torch.all(torch.isfinite(v)) and torch.all(v[mask == 0] == 0) and torch.all(v[mask != 0] > 0)


def test_refusals_name_the_smallest_frame():
    from video_vae_amd.metrics import ms_ssim
    one = torch.ones(1, 1)
    x = torch.rand(1, 1, 175, 176, 3)
    with pytest.raises(ValueError, match="176x176"):
        ms_ssim(x, x, one)
    ms_ssim(x[:, :, :44, :44], x[:, :, :44, :44], one, weights=W5[:3])
    with pytest.raises(ValueError, match="44x44"):
        ms_ssim(x[:, :, :43, :44], x[:, :, :43, :44], one, weights=W5[:3])
    small = x[:, :, :44, :44]
    for bad in (W5 + (0.1,), (), (0.5, -0.1)):
        with pytest.raises(ValueError):
            ms_ssim(small, small, one, weights=bad)
    five = torch.rand(1, 1, 44, 44, 5)
    with pytest.raises(ValueError, match="44x44"):
        ms_ssim(five, five, one, weights=W5[:3])
    with pytest.raises(ValueError):
        ms_ssim(small, small, torch.ones(1, 2), weights=W5[:3])


def test_kernel_op_has_no_cpu_fallback():
    from video_vae_amd import ops
    from video_vae_amd._lib import VvaeError
    x = torch.rand(1, 1, 44, 44, 3)
    with pytest.raises(VvaeError):
        ops.ms_ssim(x, x, torch.ones(1, 1), weights=W5[:3])


def test_parser_knows_the_flags(capsys):
    from video_vae_amd import infer as I
    from video_vae_amd.metrics import MS_SSIM_WEIGHTS
    assert MS_SSIM_WEIGHTS == W5
    ev = ["eval", "--model_path", "ck", "--data", "d"]
    a = I.parse_args(ev)
    assert a.ms_ssim is False and a.ms_ssim_scales == 5
    a = I.parse_args(ev + ["--ms-ssim"])
    assert a.ms_ssim is True and a.ms_ssim_scales == 5
    a = I.parse_args(ev + ["--size", "64", "--ms-ssim", "--ms-ssim-scales", "3"])
    assert a.ms_ssim is True and a.ms_ssim_scales == 3
    assert I.parse_args(ev + ["--size", "64", "--ms-ssim-scales", "5"]).ms_ssim is False      # nothing is asked for: nothing is refused
    for bad in (["--size", "64", "--ms-ssim"], ["--ms-ssim", "--ms-ssim-scales", "6"], ["--ms-ssim", "--ms-ssim-scales", "0"]):
        with pytest.raises(SystemExit) as e:
            I.parse_args(ev + bad)
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert "ms-ssim" in err
    with pytest.raises(SystemExit):
        I.parse_args(ev + ["--size", "64", "--ms-ssim"])
    assert "176x176" in capsys.readouterr().err
    assert I.parse_args(ev + ["--size", "64", "--tile", "--ms-ssim"]).ms_ssim is True           # tiled: the clip decides, not --size
    with pytest.raises(SystemExit):                                                              # encode has no metrics
        I.parse_args(["encode", "--model_path", "ck", "--data", "d", "--out", "o", "--ms-ssim"])


def test_entries_declared_and_exported():
    from video_vae_amd._lib import LIB_PATH, parse_header
    protos = parse_header()
    want = {"vvae_ms_ssim_supported": (ctypes.c_int, 6), "vvae_ms_ssim_ws_floats": (ctypes.c_size_t, 6),
            "vvae_ms_ssim_fwd": (ctypes.c_int, 21)}
    so = ctypes.CDLL(LIB_PATH)
    for name, (ret, nargs) in want.items():
        assert name in protos, name
        assert protos[name][0] is ret and len(protos[name][1]) == nargs, (name, protos[name])
        assert hasattr(so, name), name
    assert protos["vvae_ms_ssim_fwd"][1][14:19] == [ctypes.c_double] * 5


def test_supported_shapes_and_workspace_size():
    from video_vae_amd._lib import lib
    l = lib()
    assert l.vvae_ms_ssim_supported(176, 176, 3, 5, 0, 1) and l.vvae_ms_ssim_supported(11, 11, 1, 1, 1, 1)
    assert l.vvae_ms_ssim_supported(720, 1280, 3, 5, 0, 0) and l.vvae_ms_ssim_supported(176, 8192, 4, 5, 0, 0)
    assert not l.vvae_ms_ssim_supported(175, 176, 3, 5, 0, 0) and not l.vvae_ms_ssim_supported(176, 175, 3, 5, 0, 0)
    assert not l.vvae_ms_ssim_supported(176, 176, 5, 5, 0, 0) and not l.vvae_ms_ssim_supported(176, 176, 3, 6, 0, 0)
    assert not l.vvae_ms_ssim_supported(176, 176, 3, 0, 0, 0) and not l.vvae_ms_ssim_supported(176, 8193, 3, 5, 0, 0)
    assert not l.vvae_ms_ssim_supported(176, 176, 3, 5, 2, 0)
    # the pyramid of both operands (levels 1 .. M - 1) and at least one (S, CS) pair per frame, level and channel
    b, t, h, w, c, m = 4, 16, 256, 256, 3, 5
    pyramid = 2 * sum(b * t * (h >> j) * (w >> j) * c for j in range(1, m))
    n = l.vvae_ms_ssim_ws_floats(b, t, h, w, c, m)
    assert pyramid + 2 * b * t * m * c <= n <= pyramid + 2 * b * t * 16 * m * c + 64       # at most 16 bands a level at 64 frames
    assert 6 <= l.vvae_ms_ssim_ws_floats(1, 1, 44, 44, 3, 1) <= 2 * 3 * 44 + 4          # no pyramid; at most a band per row
    assert l.vvae_ms_ssim_ws_floats(1, 1, 43, 44, 3, 3) == 0 and l.vvae_ms_ssim_ws_floats(256, 256, 44, 44, 3, 3) == 0
    assert l.vvae_ms_ssim_fwd(None, 0, None, 0, None, None, None, None, 1, 1, 44, 44, 3, 3, *W5, 1, None) == 1001
