"""The latent quantiser on the GPU: ops.latent_quantise (csrc/quant.hip) against quant.quantise_reference on every bit, inside captured
graphs, inside GraphedInference, and through infer encode / decode / eval --quantise-bits."""
import json
import math
import os

import numpy as np
import pytest
import torch

from video_vae_amd.quant import code_counts, dequantise_reference, quantise_reference, qmax_of, rate_dataset, rate_summary

pytestmark = pytest.mark.gpu

SMALL = 64          # the --small model at 64 x 64 frames: hw = 16, ld = 96 (tests/test_gpu_infer.py)
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
# (frames, hw, ld): one token; a few tokens; the production frame (12 groups per thread, all in registers); the looping path with a token
# count that does not divide the stride; another ld that is no power of two
SHAPES = [(1, 1, 96), (3, 4, 96), (5, 256, 96), (2, 260, 96), (3, 16, 24)]


def _small(flavour="model", seed=2):
    from video_vae_amd.infer import model_config
    import video_vae_amd as V
    from video_vae_amd import rl_model
    cls = rl_model.VideoVAE if flavour == "rl" else V.VideoVAE
    return cls(rngs=V.Rngs(seed), **model_config(SMALL, True))


def _data(frames, hw, ld, bits, seed):
    """float32 (frames, hw, ld) of bf16-representable values with: channel 1 all zero; channel 2 one huge outlier; channel 3 amax == qmax
    (inv == 1) and ties k + 0.5 of both signs; channel 4 a negative maximum; channel 5 tiny values (amax below 1e-30: dead)."""
    qmax = qmax_of(bits)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((frames, hw, ld)) * rng.uniform(0.01, 4.0, size=(frames, 1, ld))
    x = torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).float().numpy()
    x[:, :, 1] = 0.0
    x[:, :, 2] *= 1e-2
    x[:, hw // 2, 2] = -3.0e4
    k = (np.arange(hw) % qmax).astype(np.float32)
    x[:, :, 3] = (k + 0.5) * np.where(np.arange(hw) % 2, -1.0, 1.0).astype(np.float32)
    x[:, 0, 3] = qmax
    x[:, :, 4] = -np.abs(x[:, :, 4]) - 0.125
    x[:, :, 5] = 1e-32
    return torch.from_numpy(x).to(torch.bfloat16).float().numpy()


def _reference(x, keep, bits):
    """codes, step, counts, dequantised of the kept frames; zeros / the input on the others."""
    q, step = quantise_reference(x, bits)
    k = keep != 0
    q[~k], step[~k] = 0, 0
    counts = np.stack([np.bincount(q[f].astype(np.int64).reshape(-1) + 128, minlength=256) if k[f] else np.zeros(256, dtype=np.int64)
                       for f in range(x.shape[0])])
    xq = np.where(k[:, None, None], dequantise_reference(q, step), x)
    return q, step, counts, xq


def _garbage(shape, ld, dev):
    from video_vae_amd.quant import QuantisedLatents
    lead = tuple(shape[:-2])
    return QuantisedLatents(torch.full(tuple(shape), 0x55, dtype=torch.int8, device=dev),
                            torch.full(lead + (ld,), float("nan"), dtype=torch.float32, device=dev),
                            torch.full(lead + (256,), -7, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("frames,hw,ld", SHAPES)
def test_kernel_equals_the_reference_on_every_bit(dev, frames, hw, ld, dtype, bits):
    from video_vae_amd import ops
    dt = DTYPES[dtype]
    assert ops.latent_quantise_supported(hw, ld, dt)
    x = _data(frames, hw, ld, bits, seed=frames * 1000 + hw + bits)
    if dtype == "fp32":                                    # values bf16 cannot hold: the fp32 products round for real
        x[:, :, 6:] = (x[:, :, 6:] * np.float32(1.0009765625) + np.float32(3e-5)).astype(np.float32)
    keeps = [np.ones(frames, dtype=np.float32), np.zeros(frames, dtype=np.float32)]      # all kept; every frame dropped
    if frames >= 3:
        mid = np.ones(frames, dtype=np.float32)
        mid[frames // 2] = 0.0                             # a dropped frame in the middle
        mid[0] = 2.5                                       # any nonzero flag keeps
        keeps.insert(0, mid)
    for keep in keeps:
        q, step, counts, xq = _reference(x, keep, bits)
        kd = torch.from_numpy(keep).to(dev)
        for in_place in (False, True):
            lat = torch.from_numpy(x).to(dev).to(dt)
            before = lat.clone()
            out = ops.latent_quantise(lat, kd, bits, dequantise_in_place=in_place, out=_garbage(lat.shape, ld, dev))
            assert np.array_equal(out.codes.cpu().numpy(), q), (keep.tolist(), in_place)
            assert np.array_equal(out.step.cpu().numpy().view(np.uint32), step.view(np.uint32)), (keep.tolist(), in_place)
            assert np.array_equal(out.counts.cpu().numpy().astype(np.int64), counts), (keep.tolist(), in_place)
            want = torch.from_numpy(xq).to(dt) if in_place else before.cpu()
            assert torch.equal(lat.cpu().view(torch.int16 if dt == torch.bfloat16 else torch.int32),
                               want.view(torch.int16 if dt == torch.bfloat16 else torch.int32)), (keep.tolist(), in_place)
            dropped = torch.from_numpy(keep == 0)
            assert torch.equal(lat.cpu()[dropped], before.cpu()[dropped])
    # counts of a kept frame sum to its elements; leading dimensions pass through
    lat = torch.from_numpy(x).to(dev).to(dt).reshape(1, frames, hw, ld)
    out = ops.latent_quantise(lat, torch.ones(1, frames, device=dev), bits)
    assert out.codes.shape == (1, frames, hw, ld) and out.step.shape == (1, frames, ld) and out.counts.shape == (1, frames, 256)
    assert out.counts.sum(dim=-1).tolist() == [[hw * ld] * frames]


def test_refusals(dev):
    from video_vae_amd import ops
    from video_vae_amd._lib import VvaeError
    assert not ops.latent_quantise_supported(16, 12, torch.bfloat16) and not ops.latent_quantise_supported(16, 96, torch.float16)
    x = torch.zeros(2, 4, 96, device=dev)
    for bad in (lambda: ops.latent_quantise(x, torch.ones(2, device=dev), 9), lambda: ops.latent_quantise(x, torch.ones(3, device=dev), 8),
                lambda: ops.latent_quantise(torch.zeros(2, 4, 12, device=dev), torch.ones(2, device=dev), 8),
                lambda: ops.latent_quantise(x.transpose(0, 1), torch.ones(4, device=dev), 8),
                lambda: ops.latent_quantise(x.cpu(), torch.ones(2), 8)):
        with pytest.raises(VvaeError):
            bad()


def test_captured_and_replayed_equals_eager(dev):
    """The op inside a captured graph, replayed twice with other data copied into the static input between the replays: bitwise the eager
    results; the graph holds no memset node."""
    from video_vae_amd import ops
    from video_vae_amd.graph import graph_node_census
    frames, hw, ld, bits = 5, 16, 96, 6
    datas = [torch.from_numpy(_data(frames, hw, ld, bits, seed=s)).to(dev).to(torch.bfloat16) for s in (1, 2)]
    keeps = [torch.tensor([1, 1, 0, 1, 1.0], device=dev), torch.tensor([0, 1, 1, 1, 0.0], device=dev)]
    static, keep = datas[0].clone(), keeps[0].clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.latent_quantise(static.clone(), keep, bits, dequantise_in_place=True)
    torch.cuda.synchronize()
    try:
        g = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        out = ops.latent_quantise(static, keep, bits, dequantise_in_place=True)
    census = graph_node_census(g)
    assert census is not None and census.get("memset", 0) == 0 and census.get("kernel", 0) >= 1, census
    for i in (0, 1, 0):
        static.copy_(datas[i])
        keep.copy_(keeps[i])
        g.replay()
        eager_lat = datas[i].clone()
        want = ops.latent_quantise(eager_lat, keeps[i], bits, dequantise_in_place=True)
        for a, e in zip(out, want):
            assert torch.equal(a, e), i
        assert torch.equal(static, eager_lat), i


def test_graphed_evaluate_through_the_quantiser(dev):
    """GraphedInference("evaluate", quant_bits=8) on the small model: its reconstruction is bitwise the decode of the reference-quantised
    means of an "encode" runner (same batch, same mask, the last window partly masked); metrics and counts follow."""
    from video_vae_amd.infer import GraphedInference, InferenceWeights
    from video_vae_amd.metrics import frame_metrics
    b, t, bits = 2, 8, 8
    m = _small("model").to(dev)
    w = InferenceWeights(m)
    x = torch.rand((b, t, SMALL, SMALL, 3), generator=torch.Generator().manual_seed(1)).to(dev)
    mk = torch.ones(b, t, device=dev)
    mk[1, 5:] = 0
    enc = GraphedInference(m, w, b, t, "encode", want_log_variance=False)
    lat = enc(x, mk)
    mean, sel = lat.mean.float().cpu().numpy(), (lat.selection * mk).cpu().numpy()
    hw, ld = mean.shape[2:]
    assert sel.sum() > 0 and (sel[1, 5:] == 0).all()
    q, step, counts, _ = _reference(mean.reshape(b * t, hw, ld), sel.reshape(-1), bits)
    fill = m.fill_token.detach().float().cpu().numpy().reshape(1, 1, ld)
    comp = np.where(sel.reshape(-1, 1, 1) != 0, dequantise_reference(q, step), fill).astype(np.float32).reshape(b, t, hw, ld)
    dec = GraphedInference(m, w, b, t, "decode")
    want = dec(torch.from_numpy(comp).to(dev).to(m.decoder.dtype), mk).clone()
    ev = GraphedInference(m, w, b, t, "evaluate", quant_bits=bits)
    assert ev.census is not None and ev.census.get("memset", 0) == 0, ev.census
    out = ev(x, mk)
    assert len(out) == 4
    recon, fm, s, cnt = out
    assert torch.equal(recon, want)
    assert torch.equal(s, lat.selection)
    for a, e in zip(fm, frame_metrics(x, want, mk)):
        assert torch.equal(a, e)
    assert np.array_equal(cnt.cpu().numpy().astype(np.int64).reshape(b * t, 256), counts)
    # the "encode" runner with quant_bits hands the kernel's codes over beside the Latents
    encq = GraphedInference(m, w, b, t, "encode", want_log_variance=False, quant_bits=bits)
    lat2, ql = encq(x, mk)
    assert torch.equal(lat2.mean, lat.mean) and torch.equal(lat2.compressed_representation, lat.compressed_representation)
    assert np.array_equal(ql.codes.cpu().numpy().reshape(b * t, hw, ld), q)
    assert np.array_equal(ql.step.cpu().numpy().reshape(b * t, ld).view(np.uint32), step.view(np.uint32))
    assert np.array_equal(ql.counts.cpu().numpy().astype(np.int64).reshape(b * t, 256), counts)
    # off: the tuple and the reconstruction of a runner built without the argument
    off = GraphedInference(m, w, b, t, "evaluate", quant_bits=None)(x, mk)
    assert len(off) == 3
    plain = GraphedInference(m, w, b, t, "evaluate")(x, mk)
    assert len(plain) == 3 and torch.equal(off[0], plain[0])
    assert not torch.equal(off[0], recon)


@pytest.mark.parametrize("mode", ["plain", "temporal"])
def test_cli_quantised_encode_decode_eval(dev, tmp_path, mode):
    """infer encode / decode / eval --quantise-bits 6 (run in this process: infer.main) on two short synthetic clips."""
    import video_vae_amd as V
    from video_vae_amd import data as D
    from video_vae_amd import infer as I
    bits = 6
    data = str(tmp_path / "data")
    D.write_synthetic_clips(data, 2, 10, 40, 48, seed=1)                          # clip 0: 8 frames, clip 1: 10 frames
    V.save_checkpoint(_small("model", seed=9), None, str(tmp_path / "ckpt"))
    ck = ["--model_path", str(tmp_path / "ckpt")]
    common = ck + ["--data", data, "--size", str(SMALL), "--frames", "4", "--batch", "2", "--small", "--flavour", "model"]
    extra = ["--temporal-overlap", "1"] if mode == "temporal" else []
    I.main(["encode"] + common + extra + ["--out", str(tmp_path / "lat")])
    I.main(["encode"] + common + extra + ["--out", str(tmp_path / "latq"), "--quantise-bits", str(bits)])
    os.makedirs(tmp_path / "latd")
    names = ("clip0000", "clip0001")
    files = {}
    for name in names:
        with np.load(tmp_path / "lat" / f"{name}.npz") as z:
            plain = {k: z[k] for k in z.files}
        with np.load(tmp_path / "latq" / f"{name}.npz") as z:
            quant = {k: z[k] for k in z.files}
        assert "mean" not in quant and int(quant["quant_bits"]) == bits and plain["mean"].shape[0] > 0
        q, step = quantise_reference(plain["mean"], bits)
        assert quant["mean_q"].dtype == np.int8 and np.array_equal(quant["mean_q"], q)
        assert np.array_equal(quant["mean_step"].view(np.uint32), step.view(np.uint32))
        for k in plain:
            if k != "mean":
                assert np.array_equal(plain[k], quant[k]), k
        assert os.path.getsize(tmp_path / "latq" / f"{name}.npz") < os.path.getsize(tmp_path / "lat" / f"{name}.npz") / 2
        np.savez(tmp_path / "latd" / f"{name}.npz", **dict(plain, mean=dequantise_reference(q, step)))
        files[name] = quant
    I.main(["decode"] + ck + ["--latents", str(tmp_path / "latq"), "--out", str(tmp_path / "recq"), "--batch", "2"])
    I.main(["decode"] + ck + ["--latents", str(tmp_path / "latd"), "--out", str(tmp_path / "recd"), "--batch", "2"])
    frames = {}
    for name in names:
        with np.load(tmp_path / "recq" / f"{name}.npz") as a, np.load(tmp_path / "recd" / f"{name}.npz") as e:
            assert a["frames"].dtype == np.uint8 and np.array_equal(a["frames"], e["frames"]), name
            frames[name] = a["frames"]
    if mode != "plain":
        with pytest.raises(SystemExit):                    # eval through the quantiser is plain mode only
            I.main(["eval"] + common + extra + ["--quantise-bits", str(bits), "--out", str(tmp_path / "m.json")])
        return
    I.main(["eval"] + common + ["--quantise-bits", str(bits), "--per-frame", "--out", str(tmp_path / "m.json")])
    res = json.loads((tmp_path / "m.json").read_text())
    assert res["config"]["quantise_bits"] == bits
    clips = {c["name"]: c for c in res["clips"]}
    rates = []
    for name in names:
        f, e = files[name], clips[name]
        r = rate_summary(code_counts(f["mean_q"]), f["selection"], int(f["n_frames"]), SMALL, SMALL, f["mean_q"].shape[2], bits)
        rates.append(r)
        assert e["bits_side"] == r["bits_side"] and e["rate"]["codes"] == r["codes"] == f["mean_q"].size
        assert abs(e["bpp_raw"] - r["bpp_raw"]) <= 1e-12 * r["bpp_raw"] and abs(e["bpp_entropy"] - r["bpp_entropy"]) <= 1e-12 * r["bpp_raw"]
        assert e["bpp_entropy"] <= e["bpp_raw"]
        # PSNR of the decoded files against eval's.  A decoded file holds uint8 frames: each value y of eval's clamped reconstruction
        # moved by d, |d| < 1 / 255.  By the triangle inequality in L2, rmse' lies within 1 / 255 of rmse, so per frame
        # |psnr' - psnr| <= 20 log10(rmse / (rmse - 1 / 255)); 1e-4 dB on top for the fp32 sums of the metrics kernel.
        x = I.centre_square(np.load(os.path.join(data, "videos0", f"{name}.npy")), SMALL).astype(np.float64) / 255.0
        y = frames[name].astype(np.float64) / 255.0
        mse_dec = ((x - y) ** 2).reshape(x.shape[0], -1).mean(axis=1)
        for i in range(x.shape[0]):
            rmse = math.sqrt(e["per_frame"]["mse"][i])
            assert rmse > 2 / 255
            tol = 20 * math.log10(rmse / (rmse - 1 / 255)) + 1e-4
            got, want = 10 * math.log10(1 / mse_dec[i]), e["per_frame"]["psnr"][i]
            print(f"{name} frame {i}: psnr decoded file {got:.4f} dB, eval {want:.4f} dB, bound {tol:.4f} dB")
            assert abs(got - want) <= tol, (name, i, got, want, tol)
    d = rate_dataset(rates)
    assert res["dataset"]["bits_side"] == d["bits_side"]
    assert abs(res["dataset"]["bpp_raw"] - d["bpp_raw"]) <= 1e-12 * d["bpp_raw"]
    assert abs(res["dataset"]["bpp_entropy"] - d["bpp_entropy"]) <= 1e-12 * d["bpp_raw"]
    assert res["dataset"]["bpp_entropy"] <= res["dataset"]["bpp_raw"]
