"""CPU: the temporal coder's definition (video_vae_amd/entropy.py: chains, thresholds, nine tables, encode_temporal_reference /
decode_temporal_reference), its latent-file members, its flags, and the committed stream tests/golden/entropy_temporal_stream.npz."""
import os
import sys

import numpy as np
import pytest
import torch

from video_vae_amd import infer as I
from video_vae_amd.entropy import (L, M, STATE_BITS, TEMPORAL_CLASSES, TEMPORAL_TABLES, CodedFrames, TemporalModel, chain_flags, chain_prev,
                                   chain_starts, coded_bits, decode_temporal_reference, encode_reference,
                                   encode_temporal_reference, normalise_counts, normalise_temporal_counts, table_size, temporal_contexts,
                                   temporal_counts, temporal_thresholds, temporal_thresholds_of_counts)
from video_vae_amd.quant import code_counts, qmax_of, quantise_reference, rate_dataset, rate_summary
from video_vae_amd.tiling import ScenePlan, TileGrid, WindowPlan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_entropy_temporal_stream as G  # noqa: E402

SIZES = [(5, 7), (16, 24), (64, 96)]                       # 35 symbols: one step with idle lanes; one frame of the --small model at 32 x 32


def _frame_counts(codes):
    return np.stack([code_counts(c) for c in codes])


def _round_trip(codes, chain, bits):
    thr, freq9 = G.model_of(codes, chain, bits)
    coded = encode_temporal_reference(codes, freq9, bits, chain, thr)
    back = decode_temporal_reference(coded, freq9, bits, codes.shape[1], codes.shape[2], chain, thr)
    assert back.dtype == np.int8 and np.array_equal(back, codes)
    return coded, freq9, thr


# ------------------------------------------------------------------------------------------------ chains
def test_chain_flags():
    flags = lambda keep, period: chain_flags(np.array(keep), period).tolist()
    assert flags([0, 1, 1, 0, 1, 1], 16) == [0, 1, 1, 1]                  # the first frame dropped; a dropped frame does not break a chain
    assert flags([1, 1, 1, 1, 1], 1) == [0, 0, 0, 0, 0]                  # period 1: every frame starts a chain
    assert flags([1, 1, 0, 1, 1, 1], 2) == [0, 1, 0, 1, 0]
    assert flags([1, 1, 1], 7) == [0, 1, 1]                              # longer than the sequence
    assert flags([[1, 1, 1, 1], [0, 0, 1, 1], [0, 0, 0, 0], [1, 0, 0, 1]], 3) == [0, 1, 1, 0, 0, 1, 0, 1]     # every row a sequence
    assert flags([[[1, 1], [1, 1]], [[0, 1], [1, 0]]], 16) == [0, 1, 0, 1, 0, 0]
    none = chain_flags(np.zeros((2, 5)), 4)
    assert none.dtype == np.uint8 and none.shape == (0,)
    assert chain_flags(torch.tensor([0.0, 2.5, 1.0]), 16).tolist() == [0, 1]       # a tensor; any nonzero flag keeps
    for period in (0, -1):
        with pytest.raises(ValueError):
            chain_flags(np.ones(3), period)
    assert chain_starts(np.array([0, 1, 0, 0, 1, 1], dtype=np.uint8)).tolist() == [0, 2, 3, 6]
    assert chain_starts(np.zeros(0, dtype=np.uint8)).tolist() == [0]
    keep = np.array([[0, 1, 1, 0, 1], [1, 0, 0, 1, 0]])
    assert chain_prev(keep, chain_flags(keep, 2)).tolist() == [-1, -1, 1, -1, -1, -1, -1, -1, 5, -1]
    for bad in (np.array([1, 0], dtype=np.uint8), np.array([0, 2], dtype=np.uint8), np.zeros(2)):
        with pytest.raises(ValueError):
            chain_starts(bad)
    with pytest.raises(ValueError):                        # one flag per coded frame
        temporal_thresholds(np.zeros((2, 4, 4), dtype=np.int8), np.zeros(3, dtype=np.uint8))


@pytest.mark.parametrize("bits", [2, 4, 8])
def test_thresholds_from_histograms_equal_the_sorted_pool(bits):
    for seed, lengths in enumerate(((1, 2, 5), (3,), (1, 1), (2, 2, 2))):
        codes, chain = G.ar1_codes(lengths, 16, 24, bits, 40 + seed)
        thr = temporal_thresholds(codes, chain)
        assert thr.dtype == np.int64 and thr.shape == (TEMPORAL_CLASSES - 1,) and (np.diff(thr) >= 0).all()
        pool = np.sort(np.concatenate([codes[f - 1].reshape(-1) for f in range(len(chain)) if chain[f]] or [np.zeros(0, dtype=np.int8)]))
        want = [int(pool[(k + 1) * pool.size // 8]) for k in range(7)] if pool.size else [0] * 7
        assert thr.tolist() == want
        assert np.array_equal(temporal_thresholds_of_counts(_frame_counts(codes), chain), thr)
    skew = np.zeros((2, 3, 8), dtype=np.int8)                             # a pool of 24 with 21 equal codes: thresholds repeat
    skew[0, 0, :3] = [-1, 1, 1]
    chain = np.array([0, 1], dtype=np.uint8)
    assert temporal_thresholds(skew, chain).tolist() == [0, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(temporal_thresholds_of_counts(_frame_counts(skew), chain), temporal_thresholds(skew, chain))


def test_contexts_and_counts():
    codes, chain = G.ar1_codes((2, 3), 5, 7, 4, 3)
    thr = temporal_thresholds(codes, chain)
    ctx = temporal_contexts(codes, chain, thr)
    assert ctx.shape == (5, 35) and (ctx[[0, 2]] == 0).all() and ctx[[1, 3, 4]].min() >= 1 and ctx.max() <= TEMPORAL_CLASSES
    f, i = 3, 17
    assert ctx[f, i] == 1 + sum(int(codes[f - 1].reshape(-1)[i]) > int(t) for t in thr)
    counts = temporal_counts(codes, chain, thr)
    assert counts.shape == (5, TEMPORAL_TABLES, 256) and counts.dtype == np.int64
    assert np.array_equal(counts.sum(axis=1), _frame_counts(codes)) and counts[[0, 2], 1:].sum() == 0 and counts[[1, 3, 4], 0].sum() == 0
    freq9 = normalise_temporal_counts(counts, 4)
    assert freq9.shape == (TEMPORAL_TABLES, table_size(4)) and freq9.dtype == np.uint16 and (freq9.astype(np.int64).sum(axis=1) == M).all()
    empty = counts.copy()
    empty[:, 4] = 0                                                       # a row without a symbol gets the pooled table
    assert np.array_equal(normalise_temporal_counts(empty, 4)[4], normalise_counts(empty.sum(axis=(0, 1)), 4))


# ------------------------------------------------------------------------------------------------ round trips
@pytest.mark.parametrize("hw,ld", SIZES)
@pytest.mark.parametrize("bits", [2, 4, 6, 8])
def test_round_trip(hw, ld, bits):
    codes, chain = G.ar1_codes(G.CHAINS, hw, ld, bits, 100 * bits + hw)
    assert chain.tolist() == [0, 0, 1, 0, 1, 1, 1, 1]
    coded, freq9, thr = _round_trip(codes, chain, bits)
    assert coded.n_words.shape == (8,) and coded.state.shape == (8, 64) and int(coded.n_words.sum()) == coded.words.shape[0]
    if hw * ld < 64:
        assert (coded.state[:, hw * ld:] == L).all()                      # the idle lanes never moved


@pytest.mark.parametrize("hw,ld", SIZES)
def test_round_trip_zero_frame_with_a_one_symbol_row(hw, ld):
    """The chain's first frame is all zeros and the only user of row 0: that table is one symbol wide (freq << 20 is 2^32, never reached),
    the frame emits no word and leaves every state at L; the frame behind it sees one class."""
    bits = 6
    codes, chain = G.zero_start_codes(hw, ld, bits, 5)
    coded, freq9, thr = _round_trip(codes, chain, bits)
    assert int(freq9[0, qmax_of(bits)]) == M and coded.n_words[0] == 0 and (coded.state[0] == L).all()
    assert np.unique(temporal_contexts(codes, chain, thr)[1]).size == 1
    zeros = np.zeros((2, hw, ld), dtype=np.int8)                          # nothing but zeros: every table, no word at all
    coded, freq9, thr = _round_trip(zeros, np.array([0, 1], dtype=np.uint8), bits)
    assert thr.tolist() == [0] * 7 and (freq9[:, qmax_of(bits)] == M).all() and coded.words.size == 0 and (coded.state == L).all()


def test_nine_equal_rows_give_the_static_stream():
    bits = 6
    codes, _ = G.ar1_codes((8,), 16, 24, bits, 7)
    freq = normalise_counts(code_counts(codes), bits)
    static = encode_reference(codes, freq, bits)
    thr = np.array([-3, -1, 0, 0, 1, 2, 4], dtype=np.int64)
    for chain in (G.chain_of((8,)), G.chain_of((1, 2, 5)), G.chain_of((1,) * 8)):
        got = encode_temporal_reference(codes, np.stack([freq] * TEMPORAL_TABLES), bits, chain, thr)
        for a, e in zip(got, static):
            assert a.dtype == e.dtype and np.array_equal(a, e)
        assert np.array_equal(decode_temporal_reference(static, np.stack([freq] * TEMPORAL_TABLES), bits, 16, 24, chain, thr), codes)


def test_tampered_streams():
    bits, hw, ld = 6, 16, 24
    codes, chain = G.ar1_codes((2, 4), hw, ld, bits, 11)
    coded, freq9, thr = _round_trip(codes, chain, bits)
    dec = lambda c, t=thr, ch=chain: decode_temporal_reference(c, freq9, bits, hw, ld, ch, t)
    offs = np.concatenate([[0], np.cumsum(coded.n_words)])
    words = coded.words.copy()                             # a flipped word in frame 3 (the second frame of the second chain)
    words[offs[3] + 5] ^= 0x0400
    with pytest.raises(ValueError, match="frame 3"):
        dec(CodedFrames(words, coded.n_words, coded.state))
    state = coded.state.copy()                             # a wrong state in frame 2: frames 3 .. 5 decode from what it produced, frame 2 is named
    state[2, 9] ^= 0x00010000
    with pytest.raises(ValueError, match="frame 2"):
        dec(CodedFrames(coded.words, coded.n_words, state))
    state = coded.state.copy()                             # two bad frames: the first in file order is named
    state[4, 0] += 1
    state[1, 0] += 1
    with pytest.raises(ValueError, match="frame 1"):
        dec(CodedFrames(coded.words, coded.n_words, state))
    for d in (1, -1):                                      # a count that lies moves the next frame's stream too
        n = coded.n_words.copy()
        n[2] += d
        n[3] -= d
        with pytest.raises(ValueError, match="frame 2"):
            dec(CodedFrames(coded.words, n, coded.state))
    wrong = thr.copy()                                     # wrong thresholds: refused, or other codes
    wrong[3:] += 2
    try:
        assert not np.array_equal(dec(coded, wrong), codes)
    except ValueError as e:
        assert "frame" in str(e)
    try:                                                   # wrong chain flags likewise
        assert not np.array_equal(dec(coded, thr, G.chain_of((6,))), codes)
    except ValueError as e:
        assert "frame" in str(e)
    assert thr[0] < thr[6]
    for bad in (thr[:6], thr[::-1].copy(), thr.astype(np.float64)):
        with pytest.raises(ValueError):
            dec(coded, bad)
    for bad in (chain[:-1], np.array([1, 0, 1, 1, 1, 1], dtype=np.uint8)):
        with pytest.raises(ValueError):
            dec(coded, thr, bad)
    with pytest.raises(ValueError):                        # four tables are not nine
        decode_temporal_reference(coded, freq9[:4], bits, hw, ld, chain, thr)
    with pytest.raises(ValueError):                        # a code its row does not hold
        one_symbol = np.zeros_like(freq9)
        one_symbol[:, qmax_of(bits)] = M
        encode_temporal_reference(codes, one_symbol, bits, chain, thr)


def test_coded_bits_formula():
    bits = 6
    codes, chain = G.ar1_codes(G.CHAINS, 16, 24, bits, 13)
    coded, freq9, _ = _round_trip(codes, chain, bits)
    assert coded_bits(coded, freq9) == 16 * coded.words.shape[0] + 8 * (64 * 32 + 32 + 1) + 16 * 9 * (2 * qmax_of(bits) + 1) + 7 * 32
    freq = normalise_counts(code_counts(codes), bits)      # one-row and four-row tables give what they gave
    static = encode_reference(codes, freq, bits)
    assert coded_bits(static, freq) == 16 * static.words.shape[0] + 8 * STATE_BITS + 16 * table_size(bits)
    assert coded_bits(static, np.stack([freq] * 4)) == 16 * static.words.shape[0] + 8 * STATE_BITS + 16 * 4 * table_size(bits) + 3 * 32


def _sizes(codes, chain, bits):
    coded, freq9, _ = _round_trip(codes, chain, bits)
    freq = normalise_counts(code_counts(codes), bits)
    return coded_bits(coded, freq9), coded_bits(encode_reference(codes, freq, bits), freq)


@pytest.mark.parametrize("bits", [4, 6])
def test_size_below_the_static_coder_on_a_correlated_source(bits):
    """Eight frames of 64 x 24 of the seeded AR(1) scale mixture (rho 0.9), one chain, everything a file stores counted on both sides.
    Measured: 0.842 at 4 bits, 0.957 at 6 bits; only the order is asserted."""
    codes, chain = G.ar1_codes((8,), 64, 24, bits, 3)
    temporal, static = _sizes(codes, chain, bits)
    print(f"temporal / static coded_bits at {bits} bits: {temporal / static:.4f}")
    assert temporal < static


def test_size_not_below_the_static_coder_on_independent_frames():
    """The same frames without correlation (rho 0): a model that leaked the answer would still shrink them.  Measured: 1.032."""
    codes, chain = G.ar1_codes((8,), 64, 24, 4, 3, rho=0.0)
    temporal, static = _sizes(codes, chain, 4)
    print(f"temporal / static coded_bits on independent frames: {temporal / static:.4f}")
    assert temporal >= 0.95 * static


def test_rate_summary_with_temporal_bits():
    counts = np.zeros(256, dtype=np.int64)
    counts[[100, 128, 129, 200]] = 6
    sel = np.array([1, 0, 1, 0, 0])
    base = rate_summary(counts, sel, n_frames=5, height=4, width=6, ld=3, bits=8, coded=5000, coded_context=4000)
    r = rate_summary(counts, sel, 5, 4, 6, 3, 8, 5000, 4000, 3000)        # the last keyword
    assert {k: r[k] for k in base} == base
    assert r["bits_coded_temporal"] == 3000 + base["bits_side"] and r["bpp_coded_temporal"] == r["bits_coded_temporal"] / 120
    d = rate_dataset([r, dict(r, bits_coded_temporal=7000, pixels=80)])
    assert d["bits_coded_temporal"] == r["bits_coded_temporal"] + 7000 and d["bpp_coded_temporal"] == d["bits_coded_temporal"] / 200
    assert "bits_coded_temporal" not in rate_dataset([r, base]) and "bits_coded_temporal" not in rate_dataset([base])


# ------------------------------------------------------------------------------------------------ the committed stream
def test_temporal_stream_fixture_reproduces():
    rec = G.record()
    with np.load(os.path.join(GOLDEN, "entropy_temporal_stream.npz")) as z:
        stored = {k: z[k] for k in z.files}
    assert sorted(stored) == sorted(rec)
    for k in rec:
        assert stored[k].dtype == np.asarray(rec[k]).dtype and np.array_equal(stored[k], rec[k]), k
    for tag, shape, chain in (("a", (8, 16, 24), [0, 0, 1, 0, 1, 1, 1, 1]), ("z", (3, 5, 7), [0, 1, 1])):
        g = {k[2:]: v for k, v in stored.items() if k.startswith(tag + "_")}
        bits = int(g["bits"])
        assert g["codes"].shape == shape and g["chain"].tolist() == chain and g["thr"].dtype == np.int64 and g["thr"].shape == (7,)
        assert g["freq"].shape == (TEMPORAL_TABLES, table_size(bits)) and int(g["n_words"].sum()) == g["words"].shape[0]
        assert (g["words"].shape[0] > 0) == (tag == "a")                  # 35 symbols: at most one per lane, and no lane renormalises
        back = decode_temporal_reference(CodedFrames(g["words"], g["n_words"], g["state"]), g["freq"], bits, shape[1], shape[2], g["chain"],
                                         g["thr"])
        assert np.array_equal(back, g["codes"])
    assert np.unique(temporal_contexts(stored["a_codes"], stored["a_chain"], stored["a_thr"])).size >= 6
    assert not stored["z_codes"][0].any() and int(stored["z_freq"][0, qmax_of(6)]) == M and stored["z_n_words"][0] == 0


# ------------------------------------------------------------------------------------------------ latent files
HW, LD = 16, 24
FILL = torch.linspace(-0.5, 0.5, LD)
TMP_KEYS = ["mean_ans", "ans_words", "ans_state", "ans_freq", "ans_shape", "ans_tthr", "ans_chain", "mean_step", "quant_bits"]


def _latent(shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape + (HW, LD)) * rng.uniform(0.01, 3.0, size=shape + (HW, 1))
    return torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).float().numpy()


def _quant_and_entropy(x, kept, bits, period):
    """(quant, temporal entropy) of dense means x with ``kept`` bool (x's leading shape, time last)."""
    q, step = quantise_reference(x.reshape((-1, HW, LD)), bits)
    quant = (torch.from_numpy(q.reshape(x.shape)), torch.from_numpy(step.reshape(x.shape[:-2] + (LD,))), bits)
    sub = q[kept.reshape(-1)]
    chain = chain_flags(kept, period)
    thr, freq9 = G.model_of(sub, chain, bits)
    return quant, (encode_temporal_reference(sub, freq9, bits, chain, thr), freq9, TemporalModel(thr, chain))


def _same_dense(a, b):
    assert len(a) == len(b)
    assert a[0].dtype == np.float32 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for x, y in zip(a[2:], b[2:]):
        assert x == y


def test_pack_unpack_plain_temporal(tmp_path):
    bits = 6
    x = _latent((7,), 21)
    sel = np.array([1, 0, 1, 1, 0, 1, 1], dtype=np.float32)
    quant, temporal = _quant_and_entropy(x, sel != 0, bits, 3)
    assert temporal[2].chain.tolist() == [0, 1, 1, 0, 1]
    args = (torch.from_numpy(x), torch.from_numpy(sel))
    plain = I.pack_latents(*args, quant=quant)
    arrays = I.pack_latents(*args, quant=quant, entropy=temporal)
    assert list(arrays) == TMP_KEYS + ["selection", "n_frames"]
    assert arrays["ans_freq"].dtype == np.uint16 and arrays["ans_freq"].shape == (TEMPORAL_TABLES, table_size(bits))
    assert arrays["ans_tthr"].dtype == np.int64 and arrays["ans_tthr"].shape == (7,) and np.array_equal(arrays["ans_tthr"], temporal[2].thr)
    assert arrays["ans_chain"].dtype == np.uint8 and arrays["ans_chain"].tolist() == [0, 1, 1, 0, 1]
    assert np.array_equal(arrays["mean_ans"], temporal[0].words) and arrays["ans_shape"].tolist() == [HW, LD]
    _same_dense(I.unpack_latents(arrays, FILL), I.unpack_latents(plain, FILL))
    I.save_latents(str(tmp_path / "t.npz"), arrays)
    with np.load(tmp_path / "t.npz") as z:
        back = {k: z[k] for k in z.files}
    assert list(back) == list(arrays)
    _same_dense(I.unpack_latents(back, FILL), I.unpack_latents(plain, FILL))
    state = arrays["ans_state"].copy()                     # a stream that fails the end check names the chain's first bad frame
    state[1, 0] ^= 0x00010000
    with pytest.raises(ValueError, match="frame 1"):
        I.unpack_latents(dict(arrays, ans_state=state), FILL)
    for bad in (dict(arrays, ans_chain=arrays["ans_chain"][:-1]), dict(arrays, ans_chain=np.append(arrays["ans_chain"], np.uint8(1))),
                dict(arrays, ans_chain=np.array([1, 1, 1, 0, 1], dtype=np.uint8)), dict(arrays, ans_tthr=arrays["ans_tthr"][:6]),
                dict(arrays, ans_freq=arrays["ans_freq"][0]), dict(arrays, ans_freq=arrays["ans_freq"][:4])):
        with pytest.raises(ValueError):
            I.unpack_latents(bad, FILL)
    with pytest.raises(ValueError):                        # nine tables need the model
        I.pack_latents(*args, quant=quant, entropy=temporal[:2])
    with pytest.raises(ValueError):                        # chain flags of another clip
        I.pack_latents(*args, quant=quant, entropy=(temporal[0], temporal[1], TemporalModel(temporal[2].thr, temporal[2].chain[:-1])))


def test_pack_unpack_tiled_windows_and_scenes_temporal():
    bits = 4
    grid = TileGrid(40, 56, 32, 8)
    x = _latent((4, 5), 22)
    sel = np.random.default_rng(0).random((4, 5)) < 0.6
    quant, temporal = _quant_and_entropy(x, sel, bits, 2)
    args = (torch.from_numpy(x), torch.from_numpy(sel.astype(np.float32)), grid)
    arrays = I.pack_latents_tiled(*args, quant=quant, entropy=temporal)
    assert list(arrays) == ["tile_grid"] + TMP_KEYS + ["selection", "n_frames"]
    _same_dense(I.unpack_latents_tiled(arrays, FILL), I.unpack_latents_tiled(I.pack_latents_tiled(*args, quant=quant), FILL))
    with pytest.raises(ValueError):
        I.unpack_latents_tiled(dict(arrays, ans_chain=arrays["ans_chain"][1:]), FILL)
    one = TileGrid(32, 32, 32, 0)
    for plan, tail in ((WindowPlan(10, 4, 1), []), (ScenePlan(10, 4, 1, [3]), ["scene_cuts"])):
        xw = _latent((plan.windows, 1, 4), 23)
        selw = np.random.default_rng(1).random((plan.windows, 1, 4)) < 0.7
        if isinstance(plan, ScenePlan):                    # the padding of a short scene's window is not kept
            for w, c in enumerate(plan.counts):
                selw[w, :, c:] = False
        quant, temporal = _quant_and_entropy(xw, selw, bits, 16)
        args = (torch.from_numpy(xw), torch.from_numpy(selw.astype(np.float32)), one, plan)
        arrays = I.pack_latents_windows(*args, quant=quant, entropy=temporal)
        assert list(arrays) == ["tile_grid", "window_starts", "temporal_overlap", "window", "n_frames"] + TMP_KEYS + ["selection"] + tail
        _same_dense(I.unpack_latents_windows(arrays, FILL), I.unpack_latents_windows(I.pack_latents_windows(*args, quant=quant), FILL))
        with pytest.raises(ValueError):
            I.unpack_latents_windows(dict(arrays, ans_chain=arrays["ans_chain"] ^ 1), FILL)


# ------------------------------------------------------------------------------------------------ parser, library
def test_parser_entropy_temporal(capsys):
    enc = ["encode", "--model_path", "ck", "--data", "d", "--out", "o"]
    ev = ["eval", "--model_path", "ck", "--data", "d"]
    coded = ["--quantise-bits", "6", "--entropy-code"]
    for cmd in (enc, ev):
        a = I.parse_args(cmd + coded)
        assert a.entropy_temporal is False and a.entropy_period == 16                            # off by default
        a = I.parse_args(cmd + coded + ["--entropy-temporal"])
        assert a.entropy_temporal is True and a.entropy_period == 16
        assert I.parse_args(cmd + coded + ["--entropy-temporal", "--entropy-period", "4"]).entropy_period == 4
        for rest in (["--entropy-temporal"], ["--quantise-bits", "6", "--entropy-temporal"]):
            with pytest.raises(SystemExit) as e:
                I.parse_args(cmd + rest)
            assert e.value.code == 2
            assert "--entropy-code" in capsys.readouterr().err
        with pytest.raises(SystemExit) as e:
            I.parse_args(cmd + coded + ["--entropy-temporal", "--entropy-period", "0"])
        assert e.value.code == 2
    for extra in (["--tile"], ["--temporal-overlap", "2"], ["--scene-cuts"]):
        assert I.parse_args(enc + coded + ["--entropy-temporal"] + extra).entropy_temporal is True
    with pytest.raises(SystemExit) as e:                   # a file has one form
        I.parse_args(enc + coded + ["--entropy-temporal", "--entropy-context"])
    assert e.value.code == 2 and "one form" in capsys.readouterr().err
    a = I.parse_args(ev + coded + ["--entropy-temporal", "--entropy-context"])                  # eval prints both
    assert a.entropy_temporal is True and a.entropy_context is True
    with pytest.raises(SystemExit):                        # decode takes no flag: the file says what it is
        I.parse_args(["decode", "--model_path", "ck", "--latents", "l", "--out", "o", "--entropy-temporal"])


def test_library_exports_the_temporal_coder():
    from video_vae_amd._lib import lib, parse_header
    protos = parse_header()
    for name in ("vvae_rans_temporal_supported", "vvae_rans_temporal_counts", "vvae_rans_encode_temporal", "vvae_rans_decode_temporal"):
        assert name in protos and getattr(lib(), name) is not None
    s = lib().vvae_rans_temporal_supported
    assert s(256, 96, 6) == 1 and s(5, 7, 2) == 1 and s(1, 1, 8) == 1 and s(5, 7, 9) == 0 and s(0, 7, 4) == 0
    assert s(8, 96, 6) == 1                                # no condition on the token grid


def test_ops_fail_loudly_without_gpu():
    from video_vae_amd import ops
    from video_vae_amd._lib import VvaeError
    freq9 = np.zeros((TEMPORAL_TABLES, table_size(4)), dtype=np.uint16)
    freq9[:, 7] = M
    c, k, prev, thr = torch.zeros(2, 16, 24, dtype=torch.int8), torch.ones(2), np.array([-1, 0], dtype=np.int32), np.zeros(7, dtype=np.int64)
    with pytest.raises(VvaeError):
        ops.rans_temporal_counts(c, k, prev, 4, thr)
    with pytest.raises(VvaeError):
        ops.rans_encode_temporal(c, k, prev, freq9, 4, thr)
    with pytest.raises(VvaeError):
        ops.rans_decode_temporal(torch.zeros(8, dtype=torch.uint16), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32),
                                 torch.zeros(2, 64, dtype=torch.uint32), freq9, 4, 16, 24, np.array([0, 2], dtype=np.int32), thr)
