"""The temporal coder on the GPU: ops.rans_temporal_counts / ops.rans_encode_temporal / ops.rans_decode_temporal (csrc/rans.hip) against
entropy.temporal_counts / encode_temporal_reference / decode_temporal_reference on every count, word, state and code, eager and inside a
captured graph, against the committed stream, and through infer encode / decode / eval --entropy-temporal.  Every comparison is exact."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from video_vae_amd.entropy import (L, M, TEMPORAL_TABLES, CodedFrames, capacity, chain_flags, chain_prev, chain_starts, coded_bits,
                                   decode_temporal_reference, encode_temporal_reference, gather_streams, normalise_counts,
                                   normalise_temporal_counts, table_size, temporal_counts)
from video_vae_amd.quant import code_counts, qmax_of, rate_dataset

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_entropy_temporal_stream as G  # noqa: E402
from util import capacity_offsets, coded_garbage  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = 64          # the --small model at 64 x 64 frames: hw = 16, ld = 96 (tests/test_gpu_infer.py)
# (hw, ld, bits), each in chains of 1, 2 and 5 frames: 35 symbols (one step with idle lanes; the counts read by bytes); 60 (by dwords); 384
# and 6144 (by 16 bytes; a partial block of steps and whole ones); 2 and 8 bits; 12 350 symbols (a partial last step, a stream that crosses
# ring refills); the production frame
CASES = [(5, 7, 6), (5, 12, 4), (16, 24, 2), (16, 24, 4), (16, 24, 8), (64, 96, 6), (130, 95, 6), (256, 96, 6)]


def _offsets(n_words):
    return np.concatenate([[0], np.cumsum(n_words)[:-1]]).astype(np.int64)


def _decode(dev, coded, freq9, bits, hw, ld, chain, thr, spare=0):
    """ops.rans_decode_temporal on host CodedFrames (the streams concatenated, ``spare`` zero words behind them) -> (codes, ok) on the host."""
    from video_vae_amd import ops
    words = np.concatenate([coded.words, np.zeros(max(spare, 1), dtype=np.uint16)])
    back, ok = ops.rans_decode_temporal(torch.from_numpy(words).to(dev), torch.from_numpy(_offsets(coded.n_words)).to(dev),
                                        torch.from_numpy(np.asarray(coded.n_words).astype(np.int32)).to(dev),
                                        torch.from_numpy(coded.state).to(dev), freq9, bits, hw, ld, chain_starts(chain), thr)
    assert back.dtype == torch.int8 and back.shape == (len(chain), hw, ld) and ok.dtype == torch.int32 and ok.shape == (len(chain),)
    return back.cpu().numpy(), ok.cpu().numpy()


def _check(dev, codes, keep, bits, period=16):
    """Counts, encode and decode of the dense ``codes`` (frames, hw, ld) under ``keep`` (any shape of that many flags, time last) against
    the definition on the kept frames; the dropped frames: zero counts, no words, states L."""
    from video_vae_amd import ops
    frames, hw, ld = codes.shape
    assert ops.rans_temporal_supported(hw, ld, bits)
    k = keep.reshape(-1) != 0
    chain = chain_flags(keep, period)
    prev = chain_prev(keep, chain)
    sub = codes[k]
    thr, freq9 = G.model_of(sub, chain, bits)
    cd, kd = torch.from_numpy(codes).to(dev), torch.from_numpy(keep.reshape(-1).astype(np.float32)).to(dev)
    counts = ops.rans_temporal_counts(cd, kd, prev, bits, thr)
    assert counts.dtype == torch.int32 and counts.shape == (frames, TEMPORAL_TABLES, 256)
    counts = counts.cpu().numpy()
    assert np.array_equal(counts[k], temporal_counts(sub, chain, thr)) and (counts[~k] == 0).all()
    assert np.array_equal(normalise_temporal_counts(counts, bits), freq9)
    cap = capacity(hw * ld)
    out = ops.rans_encode_temporal(cd, kd, prev, freq9, bits, thr, out=coded_garbage(frames, cap, dev))
    assert out.words.shape == (frames, cap) and out.n_words.shape == (frames,) and out.state.shape == (frames, 64)
    want = encode_temporal_reference(sub, freq9, bits, chain, thr)
    got = gather_streams(out.words, out.n_words, out.state, keep=k)
    assert np.array_equal(got.n_words, want.n_words), (got.n_words, want.n_words)
    assert np.array_equal(got.state, want.state) and np.array_equal(got.words, want.words)
    n_words, state = out.n_words.cpu().numpy(), out.state.cpu().numpy()
    assert (n_words[~k] == 0).all() and (state[~k] == L).all()
    back, ok = _decode(dev, got, freq9, bits, hw, ld, chain, thr)                  # the streams concatenated, as a latent file holds them
    assert np.array_equal(back, sub) and (ok == 1).all()
    if k.all():                                                                    # and straight from the encoder's capacity layout
        back, ok = ops.rans_decode_temporal(out.words, capacity_offsets(out.n_words, cap, dev), out.n_words, out.state, freq9, bits, hw, ld,
                                            chain_starts(chain), thr)
        assert np.array_equal(back.cpu().numpy(), codes) and (ok.cpu().numpy() == 1).all()
    return want, freq9, thr, chain


@pytest.mark.parametrize("hw,ld,bits", CASES)
def test_kernels_equal_the_definition(dev, hw, ld, bits):
    codes, chain = G.ar1_codes(G.CHAINS, hw, ld, bits, 1000 + hw + ld + bits)
    # chains of 1, 2 and 5 as three sequences, padded with dropped frames (never read) to a common length
    dense = np.zeros((3, 5) + codes.shape[1:], dtype=np.int8)
    keep = np.zeros((3, 5), dtype=np.float32)
    at = 0
    for s, n in enumerate(G.CHAINS):
        dense[s, :n], keep[s, :n] = codes[at:at + n], 1
        at += n
    want, freq9, thr, got_chain = _check(dev, dense.reshape((15,) + codes.shape[1:]), keep, bits)
    assert got_chain.tolist() == chain.tolist()
    assert np.array_equal(decode_temporal_reference(want, freq9, bits, hw, ld, chain, thr), codes)
    if hw * ld >= 384 and bits > 2:
        assert int((freq9 != freq9[0]).any(axis=1).sum()) >= 4                     # the classes are in use


def test_committed_stream(dev):
    """tests/golden/entropy_temporal_stream.npz, written by the reference coder: the kernels make its words, counts and states of its
    codes, and its codes of its stream."""
    from video_vae_amd import ops
    with np.load(os.path.join(GOLDEN, "entropy_temporal_stream.npz")) as z:
        stored = {k: z[k] for k in z.files}
    for tag in ("a", "z"):
        g = {k[2:]: v for k, v in stored.items() if k.startswith(tag + "_")}
        bits, (frames, hw, ld) = int(g["bits"]), g["codes"].shape
        keep = np.ones(frames, dtype=np.float32)
        prev = chain_prev(keep, g["chain"])
        cd, kd = torch.from_numpy(g["codes"]).to(dev), torch.from_numpy(keep).to(dev)
        counts = ops.rans_temporal_counts(cd, kd, prev, bits, g["thr"]).cpu().numpy()
        assert np.array_equal(normalise_temporal_counts(counts, bits), g["freq"])
        out = ops.rans_encode_temporal(cd, kd, prev, g["freq"], bits, g["thr"])
        got = gather_streams(out.words, out.n_words, out.state)
        assert np.array_equal(got.words, g["words"]) and np.array_equal(got.n_words, g["n_words"]) and np.array_equal(got.state, g["state"])
        back, ok = _decode(dev, CodedFrames(g["words"], g["n_words"], g["state"]), g["freq"], bits, hw, ld, g["chain"], g["thr"])
        assert np.array_equal(back, g["codes"]) and (ok == 1).all()


def test_static_coder_is_the_temporal_coder_with_equal_rows(dev):
    """Nine copies of a static table: ops.rans_encode_temporal writes ops.rans_encode's words, counts and states whatever the chains, and
    ops.rans_decode_temporal returns the codes of ops.rans_decode with ok all 1."""
    from video_vae_amd import ops
    bits, hw, ld = 6, 64, 24
    codes, _ = G.ar1_codes((6,), hw, ld, bits, 31)
    freq = normalise_counts(code_counts(codes), bits)
    freq9 = np.stack([freq] * TEMPORAL_TABLES)
    thr = np.array([-4, -2, -1, 0, 1, 2, 4], dtype=np.int64)
    cap = capacity(hw * ld)
    cd, keep = torch.from_numpy(codes).to(dev), torch.ones(6, device=dev)
    static = ops.rans_encode(cd, keep, freq, bits, out=coded_garbage(6, cap, dev))
    assert int(static.n_words.min()) > 64
    offsets = capacity_offsets(static.n_words, cap, dev)
    want, ok = ops.rans_decode(static.words, offsets, static.n_words, static.state, freq, bits, hw, ld)
    assert np.array_equal(want.cpu().numpy(), codes) and (ok.cpu().numpy() == 1).all()
    for lengths in ((6,), (1, 2, 3), (1,) * 6):
        chain = G.chain_of(lengths)
        temporal = ops.rans_encode_temporal(cd, keep, chain_prev(np.ones(6), chain), freq9, bits, thr, out=coded_garbage(6, cap, dev))
        for a, e in zip(gather_streams(*temporal), gather_streams(*static)):
            assert a.dtype == e.dtype and np.array_equal(a, e)
        assert torch.equal(temporal.n_words, static.n_words) and torch.equal(temporal.state, static.state)
        back, ok = ops.rans_decode_temporal(temporal.words, offsets, temporal.n_words, temporal.state, freq9, bits, hw, ld, chain_starts(chain),
                                            thr)
        assert torch.equal(back, want) and (ok.cpu().numpy() == 1).all(), lengths


def test_dropped_frames_and_a_chain_of_one(dev):
    codes, _ = G.ar1_codes((10,), 16, 24, 6, 17)
    _check(dev, codes, np.array([[2.5, 0, 1, 0, 1], [0, 0, 1, 0, 0]], dtype=np.float32), 6)      # dropped frames inside a chain; a chain of one
    _check(dev, codes, np.array([[0, 1, 1, 1, 1], [1, 1, 1, 1, 1]], dtype=np.float32), 6, period=2)
    _check(dev, codes, np.array([[1, 1, 1, 1, 1], [1, 1, 1, 1, 1]], dtype=np.float32), 6, period=1)   # every frame on its own
    _check(dev, codes[:1], np.ones((1, 1), dtype=np.float32), 6)                                 # one frame


def test_all_zero_frames(dev):
    # a zero frame alone in row 0: a one-symbol table (freq << 20 is 2^32), no word, every state L, and the chain behind it decodes
    for hw, ld in ((5, 7), (16, 24)):
        codes, chain = G.zero_start_codes(hw, ld, 6, 5)
        want, freq9, thr, _ = _check(dev, codes, np.ones((1, 3), dtype=np.float32), 6)
        assert int(freq9[0, qmax_of(6)]) == M and want.n_words[0] == 0 and (want.state[0] == L).all()
    want, freq9, thr, _ = _check(dev, np.zeros((2, 16, 24), dtype=np.int8), np.ones((1, 2), dtype=np.float32), 6)
    assert thr.tolist() == [0] * 7 and (freq9[:, qmax_of(6)] == M).all() and want.words.size == 0 and (want.state == L).all()


def test_decode_ok(dev):
    """ok is one flag per frame.  A tampered frame: ok 0 there; up to and including the first bad frame of each chain ok equals the
    definition's verdict, and the codes before it are exact -- behind it the chain is decoded from what the bad frame produced.  Counts
    and offsets that point outside the words: ok 0 and nothing read out there (a frame's capacity of spare words lies behind the last
    stream)."""
    from video_vae_amd import ops
    bits, hw, ld = 6, 16, 96
    codes, chain = G.ar1_codes((2, 4, 1), hw, ld, bits, 23)
    thr, freq9 = G.model_of(codes, chain, bits)
    coded = encode_temporal_reference(codes, freq9, bits, chain, thr)
    n, spare = coded.n_words, capacity(hw * ld)
    starts = chain_starts(chain).tolist()

    def expect(tampered, first_bad):
        back, ok = _decode(dev, tampered, freq9, bits, hw, ld, chain, thr, spare)
        with pytest.raises(ValueError, match=f"frame {min(first_bad)}"):           # the definition names the first in file order
            decode_temporal_reference(tampered, freq9, bits, hw, ld, chain, thr)
        for a, b in zip(starts[:-1], starts[1:]):
            bad = [f for f in first_bad if a <= f < b]
            stop = bad[0] if bad else b
            assert (ok[a:stop] == 1).all() and np.array_equal(back[a:stop], codes[a:stop]), (a, b)
            if bad:
                assert ok[stop] == 0

    back, ok = _decode(dev, coded, freq9, bits, hw, ld, chain, thr, spare)
    assert ok.tolist() == [1] * 7 and np.array_equal(back, codes)
    offs = _offsets(n)
    words = coded.words.copy()                             # a flipped word in frame 3, the second of its chain
    words[offs[3] + 17] ^= 0x0800
    expect(CodedFrames(words, n, coded.state), [3])
    state = coded.state.copy()                             # a wrong state at a chain start and one in another chain
    state[2, 5] ^= 0x00010000
    state[1, 0] += 1
    expect(CodedFrames(coded.words, n, state), [1, 2])
    at = int(offs[4]) + 9                                  # frame 4's stream without its 10th word
    expect(CodedFrames(np.concatenate([coded.words[:at], coded.words[at + 1:]]), n - np.eye(7, dtype=np.int64)[4], coded.state), [4])
    for d in (1, -1):                                      # a count that lies, the others' streams where they were
        back, ok = ops.rans_decode_temporal(torch.from_numpy(np.concatenate([coded.words, np.zeros(spare, dtype=np.uint16)])).to(dev),
                                            torch.from_numpy(offs).to(dev), torch.from_numpy((n + d * np.eye(7, dtype=np.int64)[6]).astype(np.int32)).to(dev),
                                            torch.from_numpy(coded.state).to(dev), freq9, bits, hw, ld, chain_starts(chain), thr)
        assert ok.cpu().numpy().tolist() == [1] * 6 + [0] and np.array_equal(back.cpu().numpy()[:6], codes[:6]), d
    far = offs.copy()                                      # offsets outside the words
    far[1], far[6] = 1 << 40, -5
    back, ok = ops.rans_decode_temporal(torch.from_numpy(np.concatenate([coded.words, np.zeros(spare, dtype=np.uint16)])).to(dev),
                                        torch.from_numpy(far).to(dev), torch.from_numpy(n.astype(np.int32)).to(dev),
                                        torch.from_numpy(coded.state).to(dev), freq9, bits, hw, ld, chain_starts(chain), thr)
    ok = ok.cpu().numpy().tolist()
    assert ok[0] == 1 and ok[1] == 0 and ok[2:6] == [1] * 4 and ok[6] == 0 and np.array_equal(back.cpu().numpy()[[0, 2, 3, 4, 5]], codes[[0, 2, 3, 4, 5]])


def test_refusals(dev):
    from video_vae_amd import ops
    from video_vae_amd._lib import VvaeError
    assert ops.rans_temporal_supported(256, 96, 6) and ops.rans_temporal_supported(5, 7, 2) and not ops.rans_temporal_supported(5, 7, 9)
    c, k = torch.zeros(2, 16, 24, dtype=torch.int8, device=dev), torch.ones(2, device=dev)
    prev, thr = np.array([-1, 0], dtype=np.int32), np.zeros(7, dtype=np.int64)
    freq9 = np.zeros((TEMPORAL_TABLES, table_size(4)), dtype=np.uint16)
    freq9[:, 7] = M
    dec = (torch.from_numpy(np.zeros(8, dtype=np.uint16)).to(dev), torch.zeros(2, dtype=torch.int64, device=dev),
           torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(2, 64, dtype=torch.int32, device=dev))
    start = np.array([0, 2], dtype=np.int32)
    for bad in (lambda: ops.rans_temporal_counts(c, k, prev, 9, thr), lambda: ops.rans_temporal_counts(c, k, prev[:1], 4, thr),
                lambda: ops.rans_temporal_counts(c, k, prev, 4, thr[:6]), lambda: ops.rans_temporal_counts(c, k, prev, 4, [3, 2, 1, 0, 0, 0, 0]),
                lambda: ops.rans_temporal_counts(c, k, torch.zeros(2, dtype=torch.int64, device=dev), 4, thr),
                lambda: ops.rans_temporal_counts(c.cpu(), k.cpu(), prev, 4, thr), lambda: ops.rans_encode_temporal(c, k, prev, freq9[:4], 4, thr),
                lambda: ops.rans_encode_temporal(c, k, prev, freq9[0], 4, thr), lambda: ops.rans_encode_temporal(c, k, prev, freq9[:, :-1], 4, thr),
                lambda: ops.rans_encode_temporal(c, torch.ones(3, device=dev), prev, freq9, 4, thr),
                lambda: ops.rans_decode_temporal(*dec, freq9[:4], 4, 16, 24, start, thr),
                lambda: ops.rans_decode_temporal(*dec, freq9, 4, 16, 24, np.array([0, 1, 2, 2], dtype=np.int32), thr),
                lambda: ops.rans_decode_temporal(*dec, freq9, 4, 16, 24, np.array([0], dtype=np.int32), thr),
                lambda: ops.rans_decode_temporal(*dec, freq9, 4, 16, 24, start, thr[:3])):
        with pytest.raises(VvaeError):
            bad()


def test_captured_and_replayed_equals_eager(dev):
    """Counts, encode and decode on one stream inside one captured graph, replayed on other codes, flags, chains and tables copied into the
    static inputs between the replays (the thresholds and the number of chains are fixed in the capture): the definition on every bit,
    twice; the graph holds no memset node."""
    from video_vae_amd import ops
    from video_vae_amd.graph import graph_node_census
    frames, hw, ld, bits = 6, 16, 24, 6
    cap = capacity(hw * ld)
    thr = np.array([-6, -3, -1, 0, 1, 3, 6], dtype=np.int64)
    hosts = [G.ar1_codes((frames,), hw, ld, bits, s)[0] // d for s, d in ((1, 1), (2, 3))]
    keeps = [np.ones(frames, dtype=np.float32), np.ones(frames, dtype=np.float32)]            # decode reads every frame: all kept
    chains = [G.chain_of((2, 3, 1)), G.chain_of((1, 1, 4))]                                     # three chains each
    prevs = [torch.from_numpy(chain_prev(k, c)).to(dev) for k, c in zip(keeps, chains)]
    starts = [torch.from_numpy(chain_starts(c)).to(dev) for c in chains]
    tables = [torch.from_numpy(normalise_temporal_counts(temporal_counts(h, c, thr), bits)).to(dev) for h, c in zip(hosts, chains)]
    assert not torch.equal(tables[0].cpu(), tables[1].cpu())
    datas = [torch.from_numpy(h).to(dev) for h in hosts]
    codes, keep, prev, start, table = datas[0].clone(), torch.ones(frames, device=dev), prevs[0].clone(), starts[0].clone(), tables[0].clone()
    base = torch.arange(frames, device=dev, dtype=torch.int64) * cap + cap

    def run():
        counts = ops.rans_temporal_counts(codes, keep, prev, bits, thr)
        out = ops.rans_encode_temporal(codes, keep, prev, table, bits, thr)
        return counts, out, ops.rans_decode_temporal(out.words, base - out.n_words, out.n_words, out.state, table, bits, hw, ld, start, thr)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run()
    torch.cuda.synchronize()
    try:
        g = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        counts, out, (back, ok) = run()
    census = graph_node_census(g)
    assert census is not None and census.get("memset", 0) == 0 and census.get("kernel", 0) >= 3, census
    for i in (0, 1, 1, 0):
        codes.copy_(datas[i])
        prev.copy_(prevs[i])
        start.copy_(starts[i])
        table.copy_(tables[i])
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy(), temporal_counts(hosts[i], chains[i], thr)), i
        want = encode_temporal_reference(hosts[i], tables[i].cpu().numpy(), bits, chains[i], thr)
        for a, e in zip(gather_streams(*out), want):
            assert np.array_equal(a, e), i
        assert np.array_equal(back.cpu().numpy(), hosts[i]) and (ok.cpu().numpy() == 1).all(), i


# ------------------------------------------------------------------------------------------------ the command line
def _small(seed=9):
    from video_vae_amd.infer import model_config
    import video_vae_amd as V
    return V.VideoVAE(rngs=V.Rngs(seed), **model_config(SMALL, True))


def _palette_clip(lengths, hw, seed):
    """Scenes of distinct palettes, every frame of a scene the same palette proportions in new places (no cut inside a scene) -> uint8
    (L, H, W, 3)."""
    rng = np.random.default_rng(seed)
    pals = [rng.integers(0, 70, size=(4, 3)), rng.integers(180, 256, size=(4, 3))]
    frames = []
    for i, n in enumerate(lengths):
        for _ in range(n):
            frames.append(pals[i % 2][rng.permutation(np.arange(hw[0] * hw[1]) % 4).reshape(hw)].astype(np.uint8))
    return np.stack(frames)


MODES = {"plain": [], "tile": ["--tile", "--overlap", "16"], "overlap": ["--temporal-overlap", "1"],
         "scenes": ["--scene-cuts", "--temporal-overlap", "1"]}


@pytest.mark.parametrize("mode", list(MODES))
def test_cli_entropy_temporal_encode_decode(dev, tmp_path, mode):
    """infer encode --small --quantise-bits 6 --entropy-code --entropy-temporal --entropy-period 3 and decode (run in this process:
    infer.main) on two short synthetic clips: the file holds the definition's temporal stream of the quantised file's codes, with the
    chains of its selection, and decodes to the frames of the run without --entropy-code byte for byte."""
    import video_vae_amd as V
    from video_vae_amd import data as D
    from video_vae_amd import infer as I
    bits, period = 6, 3
    data = str(tmp_path / "data")
    if mode == "scenes":                                                          # scenes of 5 and 4 frames; one scene of 7
        os.makedirs(data)
        np.save(os.path.join(data, "clip0000.npy"), _palette_clip((5, 4), (40, 48), 2))
        np.save(os.path.join(data, "clip0001.npy"), _palette_clip((7,), (40, 48), 3))
    else:
        height, width = (72, 100) if mode == "tile" else (40, 48)                 # 2 x 2 tiles: four sequences per clip
        D.write_synthetic_clips(data, 2, 10, height, width, seed=1)               # clip 0: 8 frames, clip 1: 10 frames
    V.save_checkpoint(_small(), None, str(tmp_path / "ckpt"))
    ck = ["--model_path", str(tmp_path / "ckpt")]
    common = ck + ["--data", data, "--size", str(SMALL), "--frames", "4", "--batch", "2", "--small", "--flavour", "model"] + MODES[mode]
    quant = ["--quantise-bits", str(bits)]
    I.main(["encode"] + common + quant + ["--out", str(tmp_path / "latq")])
    I.main(["encode"] + common + quant + ["--entropy-code", "--entropy-temporal", "--entropy-period", str(period), "--out", str(tmp_path / "latt")])
    names = ("clip0000", "clip0001")
    chained = 0
    for name in names:
        with np.load(tmp_path / "latq" / f"{name}.npz") as z:
            q = {k: z[k] for k in z.files}
        with np.load(tmp_path / "latt" / f"{name}.npz") as z:
            t = {k: z[k] for k in z.files}
        assert "mean_q" not in t and "ans_ctx" not in t and q["mean_q"].shape[0] > 0 and list(q["mean_q"].shape[1:]) == [16, 96]
        chain = chain_flags(q["selection"], period)                               # the file's selection carries the (..., T) layout
        thr, freq9 = G.model_of(q["mean_q"], chain, bits)
        want = encode_temporal_reference(q["mean_q"], freq9, bits, chain, thr)
        assert t["ans_chain"].dtype == np.uint8 and np.array_equal(t["ans_chain"], chain)
        assert t["ans_tthr"].dtype == np.int64 and np.array_equal(t["ans_tthr"], thr)
        assert t["ans_freq"].dtype == np.uint16 and np.array_equal(t["ans_freq"], freq9) and t["ans_shape"].tolist() == [16, 96]
        assert t["mean_ans"].dtype == np.uint16 and np.array_equal(t["mean_ans"], want.words)
        assert np.array_equal(t["ans_words"], want.n_words) and np.array_equal(t["ans_state"], want.state)
        for k in q:
            if k != "mean_q":
                assert np.array_equal(q[k], t[k]), k
        chained += int(chain.sum())
    assert chained > 0
    I.main(["decode"] + ck + ["--latents", str(tmp_path / "latq"), "--out", str(tmp_path / "recq"), "--batch", "2"])
    I.main(["decode"] + ck + ["--latents", str(tmp_path / "latt"), "--out", str(tmp_path / "rect"), "--batch", "2"])
    for name in names:
        with np.load(tmp_path / "rect" / f"{name}.npz") as x, np.load(tmp_path / "recq" / f"{name}.npz") as e:
            assert x["frames"].dtype == np.uint8 and np.array_equal(x["frames"], e["frames"]), name


def test_cli_eval_prints_the_temporal_size_only_with_the_flag(dev, tmp_path):
    import video_vae_amd as V
    from video_vae_amd import data as D
    from video_vae_amd import infer as I
    bits = 6
    data = str(tmp_path / "data")
    D.write_synthetic_clips(data, 2, 10, 40, 48, seed=1)
    V.save_checkpoint(_small(), None, str(tmp_path / "ckpt"))
    common = ["--model_path", str(tmp_path / "ckpt"), "--data", data, "--size", str(SMALL), "--frames", "4", "--batch", "2", "--small",
              "--flavour", "model", "--quantise-bits", str(bits), "--entropy-code"]
    I.main(["encode"] + common + ["--entropy-temporal", "--out", str(tmp_path / "latt")])
    I.main(["eval"] + common + ["--per-frame", "--out", str(tmp_path / "ma.json")])
    I.main(["eval"] + common + ["--entropy-temporal", "--per-frame", "--out", str(tmp_path / "mt.json")])
    ra, rt = json.loads((tmp_path / "ma.json").read_text()), json.loads((tmp_path / "mt.json").read_text())
    assert rt["config"]["entropy_temporal"] is True and rt["config"]["entropy_period"] == 16
    assert "entropy_temporal" not in ra["config"] and "entropy_period" not in ra["config"]
    ca, ct = {c["name"]: c for c in ra["clips"]}, {c["name"]: c for c in rt["clips"]}
    names = ("clip0000", "clip0001")
    for name in names:
        with np.load(tmp_path / "latt" / f"{name}.npz") as z:                      # the size of the stream a file of this clip holds
            f = {k: z[k] for k in z.files}
        size = coded_bits(CodedFrames(f["mean_ans"], f["ans_words"].astype(np.int64), f["ans_state"]), f["ans_freq"])
        e, p = ct[name], ca[name]
        assert e["bits_coded_temporal"] == size + e["bits_side"] == e["rate"]["bits_coded_temporal"]
        assert e["bpp_coded_temporal"] == e["bits_coded_temporal"] / e["rate"]["pixels"]
        assert "bits_coded_temporal" not in p and "bits_coded_temporal" not in p["rate"] and "bits_coded_context" not in e
        for k in ("psnr", "ssim", "mse", "kept_fraction", "bpp_raw", "bpp_entropy", "bits_side", "bits_coded", "bpp_coded"):
            assert e[k] == p[k], (name, k)
        assert e["per_frame"] == p["per_frame"]
    d = rate_dataset(ct[name]["rate"] for name in names)
    assert rt["dataset"]["bits_coded_temporal"] == d["bits_coded_temporal"] == sum(ct[name]["bits_coded_temporal"] for name in names)
    assert rt["dataset"]["bpp_coded_temporal"] == d["bpp_coded_temporal"]
    for k in ("psnr", "ssim", "mse", "bpp_raw", "bpp_entropy", "bits_coded", "bpp_coded"):
        assert rt["dataset"][k] == ra["dataset"][k], k
    assert "bits_coded_temporal" not in ra["dataset"]
