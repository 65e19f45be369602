"""The entropy coder on the GPU: ops.rans_encode / ops.rans_decode (csrc/rans.hip) against entropy.encode_reference / decode_reference on
every word, count and state, inside a captured graph, and through infer encode / decode / eval --entropy-code."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from video_vae_amd.entropy import (L, CodedFrames, M, capacity, coded_bits, decode_reference, encode_reference, gather_streams,
                                   normalise_counts, table_size)
from video_vae_amd.quant import code_counts, qmax_of, rate_dataset

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_entropy_stream import laplacian_codes  # noqa: E402
from util import capacity_offsets, coded_garbage  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = 64          # the --small model at 64 x 64 frames: hw = 16, ld = 96 (tests/test_gpu_infer.py)
# (frames, hw, ld): fewer symbols than lanes; a partial last step; a few steps; another ld; the production frame (384 steps); a frame
# whose last step is partial after many full ones; n = 24 415, no multiple of 64, whose stream crosses several ring refills and the wrap
SHAPES = [(2, 1, 8), (1, 1, 96), (3, 4, 96), (3, 16, 24), (5, 256, 96), (2, 260, 96), (2, 257, 95)]


def _codes(shape, bits, seed):
    return laplacian_codes(shape, bits, qmax_of(bits) / 6.0 + 0.4, seed)


def _host(coded):
    """words (frames, capacity), n_words (frames,), state (frames, 64) on the host, leading dimensions flattened."""
    n_words = coded.n_words.cpu().numpy().astype(np.int64).reshape(-1)
    return coded.words.cpu().numpy().reshape(n_words.shape[0], -1), n_words, coded.state.cpu().numpy().reshape(n_words.shape[0], 64)


def _check_encode(out, codes, keep, freq, bits):
    """The capacity-layout output of ops.rans_encode against the definition: the kept frames' words, counts and states; zero words and
    states L on the others."""
    k = keep != 0
    want = encode_reference(codes[k], freq, bits)
    got = gather_streams(out.words, out.n_words, out.state, keep=keep)
    assert got.words.dtype == np.uint16 and got.state.dtype == np.uint32
    assert np.array_equal(got.n_words, want.n_words), (got.n_words, want.n_words)
    assert np.array_equal(got.state, want.state)
    assert np.array_equal(got.words, want.words)
    _, n_words, state = _host(out)
    assert (n_words[~k] == 0).all() and (state[~k] == L).all()
    return want


@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("frames,hw,ld", SHAPES)
def test_kernels_equal_the_definition(dev, frames, hw, ld, bits):
    from video_vae_amd import ops
    assert ops.rans_supported(hw, ld, bits)
    codes = _codes((frames, hw, ld), bits, 1000 * frames + hw + ld + bits)
    freq = normalise_counts(code_counts(codes), bits)
    cap = capacity(hw * ld)
    cd = torch.from_numpy(codes).to(dev)
    keeps = [np.ones(frames, dtype=np.float32), np.zeros(frames, dtype=np.float32)]          # all kept; every frame dropped
    if frames >= 3:
        mid = np.ones(frames, dtype=np.float32)
        mid[frames // 2] = 0.0                             # a dropped frame in the middle
        mid[0] = 2.5                                       # any nonzero flag keeps
        keeps.insert(0, mid)
    for keep in keeps:
        out = ops.rans_encode(cd, torch.from_numpy(keep).to(dev), freq, bits, out=coded_garbage(frames, cap, dev))
        assert out.words.shape == (frames, cap) and out.n_words.shape == (frames,) and out.state.shape == (frames, 64)
        want = _check_encode(out, codes, keep, freq, bits)
        k = keep != 0
        # decode straight from the capacity layout ...
        got, ok = ops.rans_decode(out.words, capacity_offsets(out.n_words, cap, dev), out.n_words, out.state, freq, bits, hw, ld)
        assert got.dtype == torch.int8 and got.shape == (frames, hw, ld) and ok.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy()[k], codes[k]) and (ok.cpu().numpy()[k] == 1).all(), keep.tolist()
        # ... and from the streams concatenated as a latent file holds them
        if k.any():
            offs = np.concatenate([[0], np.cumsum(want.n_words)[:-1]]).astype(np.int64)
            words = torch.from_numpy(want.words if want.words.size else np.zeros(1, dtype=np.uint16)).to(dev)
            got, ok = ops.rans_decode(words, torch.from_numpy(offs).to(dev), torch.from_numpy(want.n_words).to(dev),
                                      torch.from_numpy(want.state).to(dev), freq, bits, hw, ld)
            assert np.array_equal(got.cpu().numpy(), codes[k]) and (ok.cpu().numpy() == 1).all(), keep.tolist()
    # leading dimensions pass through
    out = ops.rans_encode(cd.reshape(1, frames, hw, ld), torch.ones(1, frames, device=dev), freq, bits)
    assert out.words.shape == (1, frames, cap) and out.n_words.shape == (1, frames) and out.state.shape == (1, frames, 64)
    _check_encode(out, codes, np.ones(frames, dtype=np.float32), freq, bits)


def test_special_tables(dev):
    from video_vae_amd import ops
    # an all-zero frame under a one-symbol table (freq << 20 is 2^32) beside nothing else: no word, every state L, and it decodes
    for hw, ld in ((4, 24), (256, 96)):
        z = np.zeros((2, hw, ld), dtype=np.int8)
        freq = normalise_counts(code_counts(z), 6)
        assert freq[31] == M
        out = ops.rans_encode(torch.from_numpy(z).to(dev), torch.ones(2, device=dev), freq, 6, out=coded_garbage(2, capacity(hw * ld), dev))
        _check_encode(out, z, np.ones(2, dtype=np.float32), freq, 6)
        assert (out.n_words.cpu().numpy() == 0).all() and (out.state.cpu().numpy() == L).all()
        got, ok = ops.rans_decode(out.words, capacity_offsets(out.n_words, capacity(hw * ld), dev), out.n_words, out.state, freq, 6, hw, ld)
        assert np.array_equal(got.cpu().numpy(), z) and ok.cpu().numpy().tolist() == [1, 1]
    # one all-zero frame among others, under the clip's pooled table
    codes = _codes((3, 16, 96), 6, 3)
    codes[1] = 0
    freq = normalise_counts(code_counts(codes), 6)
    out = ops.rans_encode(torch.from_numpy(codes).to(dev), torch.ones(3, device=dev), freq, 6)
    _check_encode(out, codes, np.ones(3, dtype=np.float32), freq, 6)
    # symbols of frequency 1: every code of 8 bits present, most of them once among 24 576
    rare = _codes((2, 256, 96), 8, 9)
    rare[0].reshape(-1)[:255] = np.arange(-127, 128, dtype=np.int8)
    rare[1].reshape(-1)[-255:] = np.arange(-127, 128, dtype=np.int8)[::-1]
    freq = normalise_counts(code_counts(rare), 8)
    assert (freq >= 1).all() and int((freq == 1).sum()) > 50
    out = ops.rans_encode(torch.from_numpy(rare).to(dev), torch.ones(2, device=dev), freq, 8)
    _check_encode(out, rare, np.ones(2, dtype=np.float32), freq, 8)
    got, ok = ops.rans_decode(out.words, capacity_offsets(out.n_words, capacity(256 * 96), dev), out.n_words, out.state, freq, 8, 256, 96)
    assert np.array_equal(got.cpu().numpy(), rare) and ok.cpu().numpy().tolist() == [1, 1]


def test_a_changed_word_fails_its_frame_only(dev):
    """A valid stream with one word's value changed: ok == 0 for that frame, the other frames exact.  The words tensor carries a whole
    frame's capacity of spare words behind the last stream, so no reader, bounded or not, could leave the allocation."""
    from video_vae_amd import ops
    bits, frames, hw, ld = 6, 3, 16, 96
    codes = _codes((frames, hw, ld), bits, 5)
    freq = normalise_counts(code_counts(codes), bits)
    coded = encode_reference(codes, freq, bits)
    cap = capacity(hw * ld)
    words = np.concatenate([coded.words, np.zeros(cap, dtype=np.uint16)])
    words[int(coded.n_words[0]) + 17] ^= 0x0100            # in the middle frame
    with pytest.raises(ValueError, match="frame 1"):       # the definition refuses it too
        decode_reference(CodedFrames(words[:coded.words.size], coded.n_words, coded.state), freq, bits, hw, ld)
    offs = np.concatenate([[0], np.cumsum(coded.n_words)[:-1]]).astype(np.int64)
    args = (torch.from_numpy(offs).to(dev), torch.from_numpy(coded.n_words).to(dev), torch.from_numpy(coded.state).to(dev), freq, bits, hw, ld)
    got, ok = ops.rans_decode(torch.from_numpy(words).to(dev), *args)
    assert ok.cpu().numpy().tolist() == [1, 0, 1]
    assert np.array_equal(got.cpu().numpy()[[0, 2]], codes[[0, 2]])
    # counts and offsets that point outside the words: ok == 0, nothing read out there
    wild = torch.tensor([0, 1 << 40, -5], dtype=torch.int64, device=dev)
    got, ok = ops.rans_decode(torch.from_numpy(words).to(dev), wild, *args[1:])
    assert ok.cpu().numpy().tolist() == [1, 0, 0] and np.array_equal(got.cpu().numpy()[0], codes[0])


def test_refusals(dev):
    from video_vae_amd import ops
    from video_vae_amd._lib import VvaeError
    assert not ops.rans_supported(16, 96, 9) and not ops.rans_supported(0, 96, 6)
    c = torch.zeros(2, 4, 24, dtype=torch.int8, device=dev)
    k = torch.ones(2, device=dev)
    freq = normalise_counts(code_counts(np.zeros((1, 4, 24), dtype=np.int8)), 4)
    for bad in (lambda: ops.rans_encode(c, k, freq, 9), lambda: ops.rans_encode(c, torch.ones(3, device=dev), freq, 4),
                lambda: ops.rans_encode(c.float(), k, freq, 4), lambda: ops.rans_encode(c.transpose(1, 2), k, freq, 4),
                lambda: ops.rans_encode(c, k, freq[:-1], 4), lambda: ops.rans_encode(c, k, np.ones(15, dtype=np.uint16), 4),
                lambda: ops.rans_encode(c.cpu(), k.cpu(), freq, 4), lambda: ops.rans_encode(c, k, freq, 6),
                lambda: ops.rans_decode(torch.zeros(8, device=dev), torch.zeros(2, dtype=torch.int64, device=dev),      # float words
                                        torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(2, 64, dtype=torch.int32, device=dev),
                                        freq, 4, 4, 24),
                lambda: ops.rans_decode(torch.from_numpy(np.zeros(8, dtype=np.uint16)).to(dev), torch.zeros(3, dtype=torch.int64, device=dev),
                                        torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(2, 64, dtype=torch.int32, device=dev),
                                        freq, 4, 4, 24),
                lambda: ops.rans_decode(torch.from_numpy(np.zeros(8, dtype=np.uint16)).to(dev), torch.zeros(2, dtype=torch.int64, device=dev),
                                        torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(2, 32, dtype=torch.int32, device=dev),
                                        freq, 4, 4, 24)):
        with pytest.raises(VvaeError):
            bad()


def test_captured_and_replayed_equals_eager(dev):
    """Encode and decode inside one captured graph, replayed on other codes, flags and another table copied into the static inputs
    between the replays: the eager results on every bit; the graph holds no memset node."""
    from video_vae_amd import ops
    from video_vae_amd.graph import graph_node_census
    frames, hw, ld, bits = 5, 16, 96, 6
    cap = capacity(hw * ld)
    datas = [_codes((frames, hw, ld), bits, s) // d for s, d in ((1, 1), (2, 3))]            # two spreads: two tables
    tables = [torch.from_numpy(normalise_counts(code_counts(c), bits)).to(dev) for c in datas]
    assert not torch.equal(tables[0].cpu(), tables[1].cpu())
    datas = [torch.from_numpy(c).to(dev) for c in datas]
    keeps = [torch.tensor([1, 1, 0, 1, 1.0], device=dev), torch.tensor([0, 1, 1, 1, 0.0], device=dev)]
    codes, keep, table = datas[0].clone(), keeps[0].clone(), tables[0].clone()
    base = torch.arange(frames, device=dev, dtype=torch.int64) * cap + cap

    def run(c, k, t):
        out = ops.rans_encode(c, k, t, bits)
        return out, ops.rans_decode(out.words, base - out.n_words, out.n_words, out.state, t, bits, hw, ld)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run(codes, keep, table)
    torch.cuda.synchronize()
    try:
        g = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        out, (back, ok) = run(codes, keep, table)
    census = graph_node_census(g)
    assert census is not None and census.get("memset", 0) == 0 and census.get("kernel", 0) >= 2, census
    for i in (0, 1, 0):
        codes.copy_(datas[i])
        keep.copy_(keeps[i])
        table.copy_(tables[i])
        g.replay()
        torch.cuda.synchronize()
        want, (wback, wok) = run(datas[i], keeps[i], tables[i])
        k = keeps[i].cpu().numpy() != 0
        for a, e in zip(gather_streams(*out, keep=keeps[i]), gather_streams(*want, keep=keeps[i])):
            assert np.array_equal(a, e), i
        assert np.array_equal(out.n_words.cpu().numpy(), want.n_words.cpu().numpy()), i
        assert np.array_equal(out.state.cpu().numpy(), want.state.cpu().numpy()), i
        assert np.array_equal(back.cpu().numpy()[k], datas[i].cpu().numpy()[k]) and np.array_equal(ok.cpu().numpy(), wok.cpu().numpy()), i
        assert (ok.cpu().numpy()[k] == 1).all(), i
        _check_encode(out, datas[i].cpu().numpy(), keeps[i].cpu().numpy(), tables[i].cpu().numpy(), bits)


# ------------------------------------------------------------------------------------------------ the command line
def _small(seed=9):
    from video_vae_amd.infer import model_config
    import video_vae_amd as V
    return V.VideoVAE(rngs=V.Rngs(seed), **model_config(SMALL, True))


@pytest.mark.parametrize("mode", ["plain", "temporal"])
def test_cli_entropy_coded_encode_decode_eval(dev, tmp_path, mode):
    """infer encode --quantise-bits 6 --entropy-code, decode and eval (run in this process: infer.main) on two short synthetic clips:
    the coded file holds the definition's stream of the quantised file's codes, decodes to the same frames, and eval's bits_coded is
    the size of that stream."""
    import video_vae_amd as V
    from video_vae_amd import data as D
    from video_vae_amd import infer as I
    bits = 6
    data = str(tmp_path / "data")
    D.write_synthetic_clips(data, 2, 10, 40, 48, seed=1)                          # clip 0: 8 frames, clip 1: 10 frames
    V.save_checkpoint(_small(), None, str(tmp_path / "ckpt"))
    ck = ["--model_path", str(tmp_path / "ckpt")]
    common = ck + ["--data", data, "--size", str(SMALL), "--frames", "4", "--batch", "2", "--small", "--flavour", "model"]
    extra = ["--temporal-overlap", "1"] if mode == "temporal" else []
    quant = ["--quantise-bits", str(bits)]
    I.main(["encode"] + common + extra + quant + ["--out", str(tmp_path / "latq")])
    I.main(["encode"] + common + extra + quant + ["--entropy-code", "--out", str(tmp_path / "lata")])
    names = ("clip0000", "clip0001")
    sizes, cross = {}, {}
    for name in names:
        with np.load(tmp_path / "latq" / f"{name}.npz") as z:
            q = {k: z[k] for k in z.files}
        with np.load(tmp_path / "lata" / f"{name}.npz") as z:
            a = {k: z[k] for k in z.files}
        assert "mean_q" not in a and "mean" not in a and q["mean_q"].shape[0] > 0
        freq = normalise_counts(code_counts(q["mean_q"]), bits)                   # one table per file, pooled over its kept frames
        want = encode_reference(q["mean_q"], freq, bits)
        assert np.array_equal(a["ans_freq"], freq) and a["ans_shape"].tolist() == list(q["mean_q"].shape[1:])
        assert a["mean_ans"].dtype == np.uint16 and np.array_equal(a["mean_ans"], want.words)
        assert a["ans_words"].dtype == np.uint32 and np.array_equal(a["ans_words"], want.n_words)
        assert a["ans_state"].dtype == np.uint32 and np.array_equal(a["ans_state"], want.state)
        for k in q:
            if k != "mean_q":
                assert np.array_equal(q[k], a[k]), k
        sizes[name] = coded_bits(want, freq)
        cross[name] = float(-np.log2(freq.astype(np.float64)[q["mean_q"].astype(np.int64).reshape(-1) + qmax_of(bits)] / M).sum())
    I.main(["decode"] + ck + ["--latents", str(tmp_path / "latq"), "--out", str(tmp_path / "recq"), "--batch", "2"])
    I.main(["decode"] + ck + ["--latents", str(tmp_path / "lata"), "--out", str(tmp_path / "reca"), "--batch", "2"])
    for name in names:
        with np.load(tmp_path / "reca" / f"{name}.npz") as x, np.load(tmp_path / "recq" / f"{name}.npz") as e:
            assert x["frames"].dtype == np.uint8 and np.array_equal(x["frames"], e["frames"]), name
    if mode != "plain":
        return
    I.main(["eval"] + common + quant + ["--per-frame", "--out", str(tmp_path / "mq.json")])
    I.main(["eval"] + common + quant + ["--entropy-code", "--per-frame", "--out", str(tmp_path / "ma.json")])
    rq, ra = json.loads((tmp_path / "mq.json").read_text()), json.loads((tmp_path / "ma.json").read_text())
    assert ra["config"]["entropy_code"] is True and "entropy_code" not in rq["config"]
    cq, ca = {c["name"]: c for c in rq["clips"]}, {c["name"]: c for c in ra["clips"]}
    for name in names:
        e, p = ca[name], cq[name]
        assert e["bits_coded"] == sizes[name] + e["bits_side"] == e["rate"]["bits_coded"]
        assert e["bpp_coded"] == e["bits_coded"] / e["rate"]["pixels"]
        assert "bits_coded" not in p and "bits_coded" not in p["rate"]
        for k in ("psnr", "ssim", "mse", "kept_fraction", "bpp_raw", "bpp_entropy", "bits_side"):
            assert e[k] == p[k], (name, k)
        assert e["per_frame"] == p["per_frame"]
        # no stream beats the entropy of its codes (the cross-entropy under any table is at least that), and this one stays within the
        # size bound of tests/test_entropy_host.py: per kept frame the cross-entropy + 2048 + n / 16, the 32-bit count, and the table
        kept, n = e["rate"]["kept"], e["rate"]["codes"]
        assert e["rate"]["bits_entropy"] <= cross[name] * (1 + 1e-12)
        assert cross[name] <= e["bits_coded"] - e["bits_side"] <= cross[name] + n / 16 + (2048 + 32) * kept + 16 * table_size(bits)
    d = rate_dataset(ca[name]["rate"] for name in names)
    assert ra["dataset"]["bits_coded"] == d["bits_coded"] == sum(ca[name]["bits_coded"] for name in names)
    assert ra["dataset"]["bpp_coded"] == d["bpp_coded"]
    for k in ("psnr", "ssim", "mse", "bpp_raw", "bpp_entropy"):
        assert ra["dataset"][k] == rq["dataset"][k], k
    assert "bits_coded" not in rq["dataset"]
