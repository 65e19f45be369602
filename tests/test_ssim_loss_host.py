"""The SSIM distortion term without a GPU: metrics.ssim_grad_reference (the specification) against an independent scalar-loop fixture and
against float64 autograd of the composed path, the CPU route of ops.ssim_frames, loss.add_ssim_term, the train flag and the ABI entries."""
import os

import numpy as np
import pytest
import torch

from video_vae_amd import metrics as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim_grad_small.npz")
BAR = 1e-12          # of the gradient's scale (max |reference|): float64 sums of 121 products, far below


def _fixture():
    z = np.load(GOLDEN)
    return [{k: z[f"{k}{i}"] for k in ("x", "y", "mask", "gout", "clamp", "video_div", "ssim", "drecon")} for i in range(int(z["cases"]))]


def _family(kind, shape, seed):
    """(x, y) float64 of ``shape`` (B, T, H, W, C): random, near (y = x + small noise), flat (x constant 0.5) and ramp (y = 0.9 x + 0.03)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g, dtype=torch.float64)
    noise = torch.randn(shape, generator=g, dtype=torch.float64)
    if kind == "random":
        return x, torch.rand(shape, generator=g, dtype=torch.float64)
    if kind == "near":
        return x, x + 0.02 * noise
    if kind == "flat":
        x = torch.full(shape, 0.5, dtype=torch.float64)
        return x, x + 0.01 * noise
    w = shape[3]
    x = (torch.arange(w, dtype=torch.float64) / (w - 1)).view(1, 1, 1, w, 1).expand(shape).contiguous()
    return x, 0.9 * x + 0.03


def test_fixture_holds_the_cases_the_kernel_can_get_wrong():
    cases = _fixture()
    assert len(cases) == 3
    assert cases[0]["x"].shape[2:] == (11, 11, 1)                                  # a single valid position
    assert cases[1]["y"].shape == (2, 2, 13, 27, 3) and int(cases[1]["video_div"]) == 2 and (cases[1]["mask"] == 0).sum() == 1
    y = cases[2]["y"]
    assert int(cases[2]["clamp"]) == 1 and (y < 0).any() and (y > 1).any() and (y == 0).any() and (y == 1).any()
    assert os.path.getsize(GOLDEN) < 200_000


def test_reference_equals_the_fixture():
    for i, c in enumerate(_fixture()):
        ssim, d = M.ssim_grad_reference(c["x"], c["y"], c["mask"], c["gout"], clamp=bool(c["clamp"]), video_div=int(c["video_div"]))
        assert ssim.dtype == torch.float64 and d.dtype == torch.float64 and tuple(d.shape) == c["y"].shape
        scale = np.abs(c["drecon"]).max()
        err = np.abs(d.numpy() - c["drecon"]).max() / scale
        print(f"case {i}: gradient scale {scale:.3e}, error {err:.2e} of it; ssim error {np.abs(ssim.numpy() - c['ssim']).max():.2e}")
        assert err <= BAR
        assert np.abs(ssim.numpy() - c["ssim"]).max() <= BAR
        masked = c["mask"] == 0
        assert not d.numpy()[masked].any() and not ssim.numpy()[masked].any()
        if c["clamp"]:
            y = c["y"]
            out = (y < 0) | (y > 1)
            assert not d.numpy()[out].any()
            edge = (y == 0) | (y == 1)
            assert np.count_nonzero(d.numpy()[edge]) == edge.sum()              # the gradient passes at exactly 0 and 1


def test_reference_never_reads_masked_frames():
    c = _fixture()[1]
    x, y = c["x"].astype(np.float64), c["y"].astype(np.float64).copy()
    y[c["mask"] == 0] = np.nan
    ssim, d = M.ssim_grad_reference(x, y, c["mask"], c["gout"], clamp=False, video_div=2)
    assert np.isfinite(ssim.numpy()).all() and np.isfinite(d.numpy()).all()
    assert np.abs(d.numpy() - c["drecon"]).max() <= BAR * np.abs(c["drecon"]).max()


@pytest.mark.parametrize("kind", ["random", "near", "flat", "ramp"])
@pytest.mark.parametrize("shape", [(11, 11, 3), (13, 27, 3), (40, 52, 3), (33, 70, 1)])
@pytest.mark.parametrize("clamp", [False, True])
def test_reference_equals_float64_autograd_of_the_composed_path(shape, kind, clamp):
    h, w, c = shape
    x, y = _family(kind, (2, 2, h, w, c), seed=h * w + c)
    if clamp:
        y = y * 1.3 - 0.1
    mask = torch.tensor([[1.0, 1.0], [0.0, 2.0]])
    gout = torch.tensor([[1.0, -0.5], [3.0, 0.25]], dtype=torch.float64)
    leaf = y.clone().requires_grad_(True)
    # _frame_metrics_composed's arithmetic, kept in float64 up to the gradient
    xs, ys = (x.clamp(0, 1), leaf.clamp(0, 1)) if clamp else (x, leaf)
    ux, uy, uxx, uyy, uxy = M._ssim_moments(xs, ys)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    s = (2 * ux * uy + M.C1) * (2 * vxy + M.C2) / ((ux * ux + uy * uy + M.C1) * (vx + vy + M.C2))
    frames = s.reshape(2, 2, -1).mean(dim=2)
    (frames * gout * (mask != 0)).sum().backward()
    ssim, d = M.ssim_grad_reference(x, y, mask, gout, clamp=clamp)
    scale = float(leaf.grad.abs().max())
    err = float((d - leaf.grad).abs().max()) / scale
    print(f"{h}x{w}x{c} {kind} clamp={clamp}: scale {scale:.3e}, error {err:.2e}")
    assert scale > 0 and err <= BAR
    assert float((ssim - frames.detach() * (mask != 0)).abs().max()) <= BAR
    # and the composed operator's forward is that value in fp32
    got = M.ssim_frames_composed(x, y, mask, clamp)
    assert got.dtype == torch.float32 and torch.equal(got, ssim.to(torch.float32))
    fm = M.frame_metrics(x.float(), y.float(), mask, clamp).ssim               # the metric of the evaluation side, on fp32 operands
    assert float((M.ssim_frames_composed(x.float(), y.float(), mask, clamp) - fm).abs().max()) <= 2.0 ** -23


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("video_div", [1, 2])
def test_cpu_route_of_the_operator(dtype, video_div):
    from video_vae_amd import ops
    b, t, h, w, c = 2, 3, 13, 27, 3
    x, y = _family("near", (b, t, h, w, c), seed=3)
    x = x[:b // video_div].to(dtype)
    y = y.to(dtype)
    mask = torch.tensor([[1.0, 0.0, 1.0], [1.0, 1.0, 1.0]])
    gout = torch.tensor([[1.0, 5.0, -2.0], [0.0, 0.5, 1.0]])
    leaf = y.clone().requires_grad_(True)
    vid = x.clone().requires_grad_(True)
    out = ops.ssim_frames(vid, leaf, mask, video_div=video_div, clamp=True)
    assert out.dtype == torch.float32 and tuple(out.shape) == (b, t) and out.requires_grad
    out.backward(gout)
    ssim, d = M.ssim_grad_reference(x, y, mask, gout, clamp=True, video_div=video_div)
    assert torch.equal(out.detach(), ssim.to(torch.float32))
    assert leaf.grad.dtype == dtype
    scale = float(d.abs().max())
    tol = 1e-6 * scale + (2.0 ** -8) * d.abs() if dtype == torch.bfloat16 else torch.full_like(d, 1e-6 * scale)
    assert bool(((leaf.grad.double() - d).abs() <= tol).all())
    assert not leaf.grad[0, 1].any() and not leaf.grad[1, 0].any()              # a masked frame; an upstream gradient of 0
    from video_vae_amd._lib import VvaeError
    for bad in (lambda: ops.ssim_frames(x, y[:, :2], mask), lambda: ops.ssim_frames(x, y, mask[:, :2], video_div=video_div),
                lambda: ops.ssim_frames(x, y, mask, video_div=3), lambda: ops.ssim_frames(x.to("meta"), y, mask, video_div=video_div)):
        with pytest.raises(VvaeError):
            bad()


def test_add_ssim_term_off_leaves_the_objects_untouched(monkeypatch):
    from video_vae_amd import loss as L, ops
    monkeypatch.setattr(ops, "ssim_frames", lambda *a, **k: (_ for _ in ()).throw(AssertionError("launched with the term off")))
    loss, aux = torch.tensor(1.5), {"MSE": torch.tensor(0.25)}
    video = recon = torch.zeros(1, 1, 11, 11, 1)
    for hp in ({}, {"ssim_weight": None}, {"ssim_weight": 0}, {"ssim_weight": 0.0}):
        got_loss, got_aux = L.add_ssim_term(loss, aux, video, recon, torch.ones(1, 1), dict(L.HPARAMS, **hp))
        assert got_loss is loss and got_aux is aux and list(aux) == ["MSE"]
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            L.add_ssim_term(loss, aux, video, recon, torch.ones(1, 1), dict(L.HPARAMS, ssim_weight=bad))


@pytest.mark.parametrize("video_div", [1, 2])
def test_add_ssim_term_on_is_the_stated_formula(video_div):
    from video_vae_amd import loss as L
    b, t = 4, 3
    x, y = _family("near", (b, t, 12, 13, 2), seed=9)
    x = x[:b // video_div].float()
    y = y.float().requires_grad_(True)
    mask = torch.tensor([[1.0, 1.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.0, 1.0, 0.0]])     # sample 1 is all masked
    loss0, aux = torch.tensor(0.75), {"MSE": torch.tensor(0.25)}
    loss, aux2 = L.add_ssim_term(loss0, aux, x, y, mask, dict(L.HPARAMS, ssim_weight=0.5), video_div=video_div)
    assert aux2 is aux and list(aux) == ["MSE", "ssim"]
    frames = M.ssim_grad_reference(x, y.detach(), mask, torch.ones(b, t), clamp=False, video_div=video_div)[0].numpy()
    m = mask.numpy().astype(np.float64)
    want = float(((frames * m).sum(1) / np.maximum(m.sum(1), 1.0)).mean())
    assert abs(float(aux["ssim"].detach()) - want) <= 1e-6
    assert torch.equal(loss, loss0 + 0.5 * (1.0 - aux["ssim"]))
    loss.backward()
    gout = torch.from_numpy(-0.5 * m / np.maximum(m.sum(1, keepdims=True), 1.0) / b)
    d = M.ssim_grad_reference(x, y.detach(), mask, gout, clamp=False, video_div=video_div)[1]
    assert float((y.grad.double() - d).abs().max()) <= 1e-5 * float(d.abs().max())
    assert not y.grad[1].any()


def test_train_flag():
    from video_vae_amd import train
    assert train.parse_args([]).ssim_weight is None
    assert train.parse_args(["--ssim-weight", "0.5"]).ssim_weight == 0.5
    assert train.parse_args(["--ssim-weight", "0"]).ssim_weight == 0.0
    assert train.parse_args(["--small", "--size", "32", "--ssim-weight", "0.25"]).ssim_weight == 0.25
    for bad in (["--ssim-weight", "-1"], ["--ssim-weight", "nan"], ["--ssim-weight", "x"], ["--size", "1024", "--ssim-weight", "0.5"]):
        with pytest.raises(SystemExit):
            train.parse_args(bad)
    assert train.parse_args(["--size", "1024", "--ssim-weight", "0"]).ssim_weight == 0.0      # off: any frame size


def test_parser_names_the_limits(capsys):
    from video_vae_amd import train
    with pytest.raises(SystemExit):
        train.parse_args(["--size", "1024", "--ssim-weight", "0.5"])
    assert "W C <= 2048" in capsys.readouterr().err


def test_header_declares_and_library_exports_the_entries():
    from video_vae_amd._lib import lib, parse_header
    protos = parse_header()
    want = {"vvae_ssim_loss_supported": 5, "vvae_ssim_loss_ws_floats": 5, "vvae_ssim_loss_band_rows": 5, "vvae_ssim_loss_fwd": 15,
            "vvae_ssim_loss_bwd": 16}
    for name, nargs in want.items():
        assert name in protos and len(protos[name][1]) == nargs, name
        assert getattr(lib(), name) is not None
    assert len(protos["vvae_recon_metrics_fwd"][1]) == 16                           # the existing entry keeps its signature


def test_supported_shapes_and_workspace_size():
    """Host-side entries only: the one-strip shapes, and 3 maps of (H - 10) rows of W rounded up to 4 floats per frame and channel plus the
    forward's partial sums."""
    from video_vae_amd._lib import lib
    l = lib()
    for h, w, c, ok in ((11, 11, 1, 1), (11, 512, 4, 1), (40, 256, 3, 1), (256, 256, 3, 1), (11, 513, 4, 0), (10, 20, 3, 0), (20, 10, 3, 0),
                        (16, 16, 5, 0), (16, 16, 0, 0), (11, 2048, 1, 1), (11, 2049, 1, 0)):
        assert l.vvae_ssim_loss_supported(h, w, c, 1, 1) == ok, (h, w, c)
        assert (l.vvae_ssim_loss_ws_floats(1, 1, h, w, c) > 0) == bool(ok)
        assert bool(l.vvae_recon_metrics_supported(h, w, c, 1, 1)) == bool(ok)      # the same shapes as the metrics entry
    assert l.vvae_ssim_loss_supported(16, 16, 3, 2, 0) == 0
    assert l.vvae_ssim_loss_ws_floats(65535, 1, 11, 11, 1) > 0 and l.vvae_ssim_loss_ws_floats(65536, 1, 11, 11, 1) == 0
    assert l.vvae_ssim_loss_ws_floats(256, 256, 11, 11, 1) == 0
    n = l.vvae_ssim_loss_ws_floats(2, 3, 13, 27, 3)
    maps = 6 * 3 * 3 * 3 * 28
    assert maps <= n <= maps + 6 * 2 * 13 + 4
    r = l.vvae_ssim_loss_band_rows(2, 3, 35, 20, 3)
    assert 0 < r < 35
