"""The entropy coder on the host: the numpy definition (video_vae_amd/entropy.py), the range-coded latent files of the three formats, the
committed stream fixture and the parser.  No GPU."""
import os
import sys
import zipfile

import numpy as np
import pytest
import torch

from video_vae_amd import infer as I
from video_vae_amd.entropy import (L, LANES, M, CodedFrames, capacity, coded_bits, decode_context_reference, decode_reference,
                                   encode_reference, gather_streams, normalise_counts, table_size)
from video_vae_amd.quant import code_counts, dequantise_reference, quantise_reference, qmax_of, rate_dataset, rate_summary
from video_vae_amd.tiling import ScenePlan, TileGrid, WindowPlan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_entropy_parent_streams as P  # noqa: E402
import make_entropy_stream as G  # noqa: E402

BITS = (2, 4, 6, 8)
# (hw, ld): n = 1, 8 (fewer symbols than lanes), 96 (a partial last step), 384, 1 536 (the --small model's frame), 24 576 (the production
# frame), 24 960
FRAMES = [(1, 1), (1, 8), (1, 96), (4, 96), (16, 96), (256, 96), (260, 96)]


def _codes(shape, bits, seed):
    """Seeded Laplacian codes whose spread grows with the range of ``bits``."""
    return G.laplacian_codes(shape, bits, qmax_of(bits) / 6.0 + 0.4, seed)


def _table_of(codes, bits):
    return normalise_counts(code_counts(codes), bits)


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("bits", BITS)
def test_normalise_counts_properties(bits):
    qmax = qmax_of(bits)
    codes = _codes((3, 16, 24), bits, bits)
    counts = code_counts(codes)
    freq = normalise_counts(counts, bits)
    assert freq.dtype == np.uint16 and freq.shape == (2 * qmax + 1,) == (table_size(bits),)
    assert int(freq.astype(np.int64).sum()) == M
    assert np.array_equal(freq > 0, counts[128 - qmax:128 + qmax + 1] > 0)                 # the support is preserved
    assert np.array_equal(freq, normalise_counts(counts.copy(), bits))                     # deterministic
    per_frame = np.stack([code_counts(codes[f]) for f in range(3)])                        # per-frame rows are pooled
    assert np.array_equal(freq, normalise_counts(per_frame, bits))


def test_normalise_counts_cases():
    one = np.zeros(256, dtype=np.int64)
    one[128 - 3] = 777                                     # a single symbol owns the table
    freq = normalise_counts(one, 4)
    assert freq[7 - 3] == M and int(freq.astype(np.int64).sum()) == M and np.count_nonzero(freq) == 1
    dom = np.ones(256, dtype=np.int64)                     # 255 present symbols, one dominant
    dom[0] = 0
    dom[128] = 10 ** 6
    freq = normalise_counts(dom, 8)
    assert freq.shape == (255,) and (freq >= 1).all() and int(freq.astype(np.int64).sum()) == M
    assert freq[127] == M - 254 and (np.delete(freq, 127) == 1).all()
    flat = np.zeros(256, dtype=np.int64)                   # ties: the lowest index takes the difference
    flat[128 - 1:128 + 2] = 5
    assert normalise_counts(flat, 2).tolist() == [1366, 1365, 1365]
    over = np.zeros(256, dtype=np.int64)                   # the floors of max(1, .) sum to more than M: taken from the largest
    over[1:] = 1
    over[128] = 3
    freq = normalise_counts(over, 8)
    assert int(freq.astype(np.int64).sum()) == M and (freq >= 1).all()
    with pytest.raises(ValueError):
        normalise_counts(np.zeros(256, dtype=np.int64), 6)
    with pytest.raises(ValueError):                        # a code beyond +-qmax of the bits
        normalise_counts(dom, 4)
    with pytest.raises(ValueError):
        normalise_counts(one, 9)


# ------------------------------------------------------------------------------------------------ round trips
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("hw,ld", FRAMES)
def test_round_trip(hw, ld, bits):
    codes = _codes((3, hw, ld), bits, 100 * bits + hw + ld)
    freq = _table_of(codes, bits)
    coded = encode_reference(codes, freq, bits)
    n = hw * ld
    assert coded.words.dtype == np.uint16 and coded.words.shape == (int(coded.n_words.sum()),)
    assert coded.n_words.dtype == np.int64 and coded.n_words.shape == (3,) and (coded.n_words <= capacity(n)).all()
    assert coded.state.dtype == np.uint32 and coded.state.shape == (3, LANES) and (coded.state >= L).all()
    if n < LANES:
        assert (coded.state[:, n:] == L).all()             # the lanes that never had a symbol
    back = decode_reference(coded, freq, bits, hw, ld)
    assert back.dtype == np.int8 and np.array_equal(back, codes)
    assert coded_bits(coded, freq) == 16 * coded.words.shape[0] + 3 * (64 * 32 + 32) + 16 * freq.shape[0]
    one = encode_reference(codes[1], freq, bits)           # a single frame (hw, ld) gives that frame's stream
    a = int(coded.n_words[0])
    assert np.array_equal(one.words, coded.words[a:a + int(coded.n_words[1])]) and np.array_equal(one.state[0], coded.state[1])


def test_round_trip_special_tables():
    # an all-zero frame under a one-symbol table: freq << 20 is 2^32, nothing is ever emitted and every state stays L
    for hw, ld in ((4, 24), (256, 96)):
        z = np.zeros((2, hw, ld), dtype=np.int8)
        freq = _table_of(z, 6)
        assert freq[31] == M
        coded = encode_reference(z, freq, 6)
        assert coded.words.size == 0 and (coded.n_words == 0).all() and (coded.state == L).all()
        assert np.array_equal(decode_reference(coded, freq, 6, hw, ld), z)
    # a table pooled from more frames than are coded
    codes = _codes((5, 16, 24), 4, 7)
    freq = _table_of(codes, 4)
    coded = encode_reference(codes[1:3], freq, 4)
    assert np.array_equal(decode_reference(coded, freq, 4, 16, 24), codes[1:3])
    # symbols of frequency 1: every code of 8 bits present, most of them once among 24 576
    rare = _codes((1, 256, 96), 8, 9)
    rare.reshape(-1)[:255] = np.arange(-127, 128, dtype=np.int8)
    freq = _table_of(rare, 8)
    assert (freq >= 1).all() and int((freq == 1).sum()) > 50
    assert np.array_equal(decode_reference(encode_reference(rare, freq, 8), freq, 8, 256, 96), rare)
    # no frames at all
    none = encode_reference(np.zeros((0, 4, 24), dtype=np.int8), freq, 8)
    assert none.words.size == 0 and none.n_words.shape == (0,) and decode_reference(none, freq, 8, 4, 24).shape == (0, 4, 24)
    with pytest.raises(ValueError):                        # a code outside the table's support
        encode_reference(np.full((1, 4, 24), 5, dtype=np.int8), _table_of(np.zeros((1, 4, 24), dtype=np.int8), 4), 4)
    with pytest.raises(ValueError):                        # a table that does not sum to M
        encode_reference(np.zeros((1, 4, 24), dtype=np.int8), np.ones(15, dtype=np.uint16), 4)


@pytest.mark.parametrize("bits", BITS)
def test_coded_size_is_near_the_cross_entropy(bits):
    """Per frame, 16 n_words + 2048 (the words and the 64 states) is at most the frame's cross-entropy under the stored table plus
    2048 + n / 16 bits: a lane ends below 2^32 having started at 2^16, so the states cost at most 16 + 16 bits per lane beyond the
    information they hold, and n / 16 is slack well under rANS's worst-case loss per symbol at a 12-bit scale.  Measured here (seeded
    Laplacian codes, states included), the largest excess over the cross-entropy per (bits, n): n = 96 (hardly a word emitted yet):
    1 915.2 / 1 777.9 / 1 588.4 / 1 462.1 bits at 2 / 4 / 6 / 8 bits; n = 1 536: 1 541.8 / 1 586.9 / 1 592.7 / 1 517.5; n = 24 576:
    1 585.9 / 1 511.5 / 1 561.3 / 1 515.0; n = 24 960: 1 564.2 / 1 563.5 / 1 559.8 / 1 576.7."""
    qmax = qmax_of(bits)
    for hw, ld in ((1, 96), (16, 96), (256, 96), (260, 96)):
        n = hw * ld
        codes = _codes((3, hw, ld), bits, 100 * bits + hw + ld)
        freq = _table_of(codes, bits)
        coded = encode_reference(codes, freq, bits)
        p = freq.astype(np.float64) / M
        for f in range(3):
            cross = float(-np.log2(p[codes[f].astype(np.int64).reshape(-1) + qmax]).sum())
            size = 16 * int(coded.n_words[f]) + 2048
            print(f"bits {bits} n {n} frame {f}: {size} bits, cross-entropy {cross:.1f}, excess {size - cross:.1f}")
            assert size <= cross + 2048 + n / 16, (bits, n, f, size, cross)


def test_corrupted_streams_raise():
    bits, hw, ld = 6, 16, 96
    codes = _codes((3, hw, ld), bits, 5)
    freq = _table_of(codes, bits)
    coded = encode_reference(codes, freq, bits)
    assert (coded.n_words > 64).all()
    words = coded.words.copy()                             # a changed word in the middle frame
    words[int(coded.n_words[0]) + 17] ^= 0x0100
    with pytest.raises(ValueError, match="frame 1"):
        decode_reference(CodedFrames(words, coded.n_words, coded.state), freq, bits, hw, ld)
    short = coded.n_words.copy()                           # the last word dropped: the read past the end yields 0, the count is off
    short[2] -= 1
    with pytest.raises(ValueError, match="frame 2"):
        decode_reference(CodedFrames(coded.words[:-1], short, coded.state), freq, bits, hw, ld)
    state = coded.state.copy()                             # a changed state
    state[0, 5] ^= 0x00010000
    with pytest.raises(ValueError, match="frame 0"):
        decode_reference(CodedFrames(coded.words, coded.n_words, state), freq, bits, hw, ld)
    wild = np.full_like(coded.state, 0xffffffff)           # states that make every lane read at every step: still no index error
    with pytest.raises(ValueError):
        decode_reference(CodedFrames(coded.words, coded.n_words, wild), freq, bits, hw, ld)
    for bad in (CodedFrames(coded.words[:-1], coded.n_words, coded.state),                 # counts that do not sum to the words
                CodedFrames(coded.words, coded.n_words, coded.state[:, :32]),
                CodedFrames(coded.words.astype(np.int32), coded.n_words, coded.state)):
        with pytest.raises(ValueError):
            decode_reference(bad, freq, bits, hw, ld)
    with pytest.raises(ValueError):                        # more words than a frame of n symbols can hold
        decode_reference(coded, freq, bits, 1, 8)


def test_gather_streams():
    """The capacity layout of ops.rans_encode -> the host layout: a frame's stream is the last n_words entries of its row."""
    codes = _codes((3, 4, 24), 4, 11)
    freq = _table_of(codes, 4)
    coded = encode_reference(codes, freq, 4)
    cap = capacity(4 * 24)
    rows = np.full((3, cap), 0xabcd, dtype=np.uint16)
    a = 0
    for f in range(3):
        k = int(coded.n_words[f])
        rows[f, cap - k:] = coded.words[a:a + k]
        a += k
    got = gather_streams(torch.from_numpy(rows), torch.from_numpy(coded.n_words.astype(np.int32)), torch.from_numpy(coded.state))
    for x, y in zip(got, coded):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    keep = np.array([1.0, 0.0, 2.0], dtype=np.float32)
    got = gather_streams(rows, coded.n_words, coded.state, keep=keep)
    want = encode_reference(codes[[0, 2]], freq, 4)
    for x, y in zip(got, want):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------ the committed stream
def test_stream_fixture_reproduces():
    """tests/golden/entropy_stream.npz (two frames of 4 x 24 at 4 bits) is what the definition makes today, member for member, and
    decodes to its codes."""
    rec = G.record()
    with np.load(os.path.join(GOLDEN, "entropy_stream.npz")) as z:
        stored = {k: z[k] for k in z.files}
    assert sorted(stored) == sorted(rec)
    for k in rec:
        assert stored[k].dtype == np.asarray(rec[k]).dtype and np.array_equal(stored[k], rec[k]), k
    assert stored["codes"].shape == (2, 4, 24) and int(stored["bits"]) == 4 and int(stored["n_words"].sum()) == stored["words"].shape[0] > 0
    back = decode_reference(CodedFrames(stored["words"], stored["n_words"], stored["state"]), stored["freq"], 4, 4, 24)
    assert np.array_equal(back, stored["codes"])


def test_parent_streams_reproduce():
    """tests/golden/entropy_parent_streams.npz holds what the static and the context coder's definitions made of nine small cases when
    each had a loop of its own (recorded from that tree).  The one loop per direction makes every array of it, exactly, and decodes every
    stream to its codes."""
    rec = P.record()
    with np.load(os.path.join(GOLDEN, "entropy_parent_streams.npz")) as z:
        stored = {k: z[k] for k in z.files}
    assert sorted(stored) == sorted(rec)
    for k in rec:
        assert stored[k].dtype == np.asarray(rec[k]).dtype and np.array_equal(stored[k], rec[k]), k
    cases = sorted({k.split("_")[0] for k in stored})
    assert cases == [f"c{i}" for i in range(len(P.CONTEXT) + 1)] + [f"s{i}" for i in range(len(P.STATIC) + 1)]
    for case in cases:
        m = {k[len(case) + 1:]: v for k, v in stored.items() if k.startswith(case + "_")}
        coded = CodedFrames(m["words"], m["n_words"], m["state"])
        hw, ld = m["codes"].shape[1:]
        if case[0] == "s":
            back = decode_reference(coded, m["freq"], int(m["bits"]), hw, ld)
        else:
            back = decode_context_reference(coded, m["freq"], int(m["bits"]), hw, ld, int(m["grid_w"]), m["thr"])
        assert back.dtype == np.int8 and np.array_equal(back, m["codes"]), case
    assert stored["s2_words"].size > 64 and stored["c3_words"].size > 1024 and stored["s3_words"].size == 0


# ------------------------------------------------------------------------------------------------ latent files
HW, LD = 16, 24
FILL = torch.linspace(-0.5, 0.5, LD)
ANS_KEYS = ["mean_ans", "ans_words", "ans_state", "ans_freq", "ans_shape", "mean_step", "quant_bits"]


def _latent(shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape + (HW, LD)) * rng.uniform(0.01, 3.0, size=shape + (1, LD))
    x = torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).float().numpy()
    x[..., 1] = 0.0                                        # a dead channel
    return x


def _quant_and_entropy(x, kept, bits):
    """(quant, entropy) of dense means x with ``kept`` bool (x's leading shape): the dense codes and steps as the quantiser hands them
    over, and the coded kept frames (row-major over kept) with the table of their pooled counts."""
    q, step = quantise_reference(x.reshape((-1, HW, LD)), bits)
    quant = (torch.from_numpy(q.reshape(x.shape)), torch.from_numpy(step.reshape(x.shape[:-2] + (LD,))), bits)
    sub = q[kept.reshape(-1)]
    freq = _table_of(sub, bits)
    return quant, (encode_reference(sub, freq, bits), freq)


def _same_dense(a, b):
    assert len(a) == len(b)
    assert a[0].dtype == np.float32 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for x, y in zip(a[2:], b[2:]):
        assert x == y


def test_pack_unpack_plain_entropy(tmp_path):
    bits = 6
    x = _latent((5,), 21)
    sel = np.array([1, 0, 1, 1, 0], dtype=np.float32)
    quant, entropy = _quant_and_entropy(x, sel != 0, bits)
    plain = I.pack_latents(torch.from_numpy(x), torch.from_numpy(sel), quant=quant)
    assert list(plain) == ["mean_q", "mean_step", "quant_bits", "selection", "n_frames"]     # without entropy: as it was
    arrays = I.pack_latents(torch.from_numpy(x), torch.from_numpy(sel), quant=quant, entropy=entropy)
    assert list(arrays) == ANS_KEYS + ["selection", "n_frames"]
    assert arrays["mean_ans"].dtype == np.uint16 and arrays["ans_words"].dtype == np.uint32 and arrays["ans_words"].shape == (3,)
    assert arrays["ans_state"].dtype == np.uint32 and arrays["ans_state"].shape == (3, 64) and arrays["ans_freq"].dtype == np.uint16
    assert arrays["ans_shape"].dtype == np.int64 and arrays["ans_shape"].tolist() == [HW, LD] and int(arrays["quant_bits"]) == bits
    assert np.array_equal(arrays["mean_ans"], entropy[0].words) and np.array_equal(arrays["mean_step"], plain["mean_step"])
    for k in ("selection", "n_frames"):
        assert np.array_equal(arrays[k], plain[k])
    _same_dense(I.unpack_latents(arrays, FILL), I.unpack_latents(plain, FILL))
    comp, _ = I.unpack_latents(arrays, FILL)
    q, step = quantise_reference(x[sel != 0], bits)
    assert np.array_equal(comp[sel != 0], dequantise_reference(q, step))
    # the file is stored, not deflated, and reads back to the same dense result
    nbytes = I.save_latents(str(tmp_path / "a.npz"), arrays)
    assert nbytes == os.path.getsize(tmp_path / "a.npz")
    with zipfile.ZipFile(tmp_path / "a.npz") as zf:
        assert all(i.compress_type == zipfile.ZIP_STORED for i in zf.infolist())
    I.save_latents(str(tmp_path / "q.npz"), plain)
    with zipfile.ZipFile(tmp_path / "q.npz") as zf:
        assert all(i.compress_type == zipfile.ZIP_DEFLATED for i in zf.infolist())
    with np.load(tmp_path / "a.npz") as z:
        back = {k: z[k] for k in z.files}
    assert list(back) == list(arrays)
    _same_dense(I.unpack_latents(back, FILL), I.unpack_latents(plain, FILL))
    # a stream that fails the end check names the file's frame; members that do not fit raise too
    state = arrays["ans_state"].copy()
    state[1, 0] ^= 0x00010000
    with pytest.raises(ValueError, match="frame 1"):
        I.unpack_latents(dict(arrays, ans_state=state), FILL)
    with pytest.raises(ValueError):
        I.unpack_latents(dict(arrays, mean_ans=arrays["mean_ans"][:-1]), FILL)
    with pytest.raises(ValueError):
        I.unpack_latents(dict(arrays, ans_freq=arrays["ans_freq"][:-1]), FILL)
    with pytest.raises(ValueError):                        # the coded frames must be the kept ones
        I.pack_latents(torch.from_numpy(x), torch.from_numpy(np.ones(5, dtype=np.float32)), quant=quant, entropy=entropy)
    with pytest.raises(ValueError):                        # entropy codes the quantiser's codes
        I.pack_latents(torch.from_numpy(x), torch.from_numpy(sel), entropy=entropy)


def test_pack_unpack_tiled_and_windows_entropy():
    bits = 4
    grid = TileGrid(40, 56, 32, 8)
    x = _latent((4, 5), 22)
    sel = np.random.default_rng(0).random((4, 5)) < 0.6
    quant, entropy = _quant_and_entropy(x, sel, bits)
    args = (torch.from_numpy(x), torch.from_numpy(sel.astype(np.float32)), grid)
    arrays = I.pack_latents_tiled(*args, quant=quant, entropy=entropy)
    assert list(arrays) == ["tile_grid"] + ANS_KEYS + ["selection", "n_frames"]
    assert list(I.pack_latents_tiled(*args, quant=quant)) == ["tile_grid", "mean_q", "mean_step", "quant_bits", "selection", "n_frames"]
    _same_dense(I.unpack_latents_tiled(arrays, FILL), I.unpack_latents_tiled(I.pack_latents_tiled(*args, quant=quant), FILL))
    one = TileGrid(32, 32, 32, 0)
    plan = WindowPlan(10, 4, 1)
    xw = _latent((plan.windows, 1, 4), 23)
    selw = np.random.default_rng(1).random((plan.windows, 1, 4)) < 0.7
    quant, entropy = _quant_and_entropy(xw, selw, bits)
    args = (torch.from_numpy(xw), torch.from_numpy(selw.astype(np.float32)), one, plan)
    arrays = I.pack_latents_windows(*args, quant=quant, entropy=entropy)
    assert list(arrays) == ["tile_grid", "window_starts", "temporal_overlap", "window", "n_frames"] + ANS_KEYS + ["selection"]
    _same_dense(I.unpack_latents_windows(arrays, FILL), I.unpack_latents_windows(I.pack_latents_windows(*args, quant=quant), FILL))
    # scenes: the padded frames of a short scene's window are not kept, so they are not coded either
    sp = ScenePlan(10, 4, 0, [3])
    xs = _latent((sp.windows, 1, 4), 24)
    kept = np.ones((sp.windows, 1, 4), dtype=bool)
    for w, c in enumerate(sp.counts):
        kept[w, :, c:] = False
    assert not kept.all()
    quant, entropy = _quant_and_entropy(xs, kept, bits)
    args = (torch.from_numpy(xs), torch.ones(sp.windows, 1, 4), one, sp)
    arrays = I.pack_latents_windows(*args, quant=quant, entropy=entropy)
    assert list(arrays)[-2:] == ["selection", "scene_cuts"] and arrays["ans_words"].shape == (int(kept.sum()),)
    _same_dense(I.unpack_latents_windows(arrays, FILL), I.unpack_latents_windows(I.pack_latents_windows(*args, quant=quant), FILL))


def test_rate_summary_with_coded_bits():
    counts = np.zeros(256, dtype=np.int64)
    counts[[100, 128, 129, 200]] = 6
    sel = np.array([1, 0, 1, 0, 0])
    base = rate_summary(counts, sel, n_frames=5, height=4, width=6, ld=3, bits=8)
    assert "bits_coded" not in base and "bits_coded" not in rate_dataset([base])
    r = rate_summary(counts, sel, n_frames=5, height=4, width=6, ld=3, bits=8, coded=5000)
    assert {k: r[k] for k in base} == base
    assert r["bits_coded"] == 5000 + base["bits_side"] and r["bpp_coded"] == r["bits_coded"] / 120
    d = rate_dataset([r, dict(r, bits_coded=7000, pixels=80)])
    assert d["bits_coded"] == r["bits_coded"] + 7000 and d["bpp_coded"] == d["bits_coded"] / 200
    assert "bits_coded" not in rate_dataset([r, base])


# ------------------------------------------------------------------------------------------------ parser, library
def test_parser_entropy_code(capsys):
    enc = ["encode", "--model_path", "ck", "--data", "d", "--out", "o"]
    ev = ["eval", "--model_path", "ck", "--data", "d"]
    for cmd in (enc, ev):
        assert I.parse_args(cmd).entropy_code is False and I.parse_args(cmd + ["--quantise-bits", "6"]).entropy_code is False
        assert I.parse_args(cmd + ["--quantise-bits", "6", "--entropy-code"]).entropy_code is True
        with pytest.raises(SystemExit) as e:
            I.parse_args(cmd + ["--entropy-code"])
        assert e.value.code == 2
        assert "--quantise-bits" in capsys.readouterr().err
    for extra in (["--tile"], ["--temporal-overlap", "2"], ["--scene-cuts"]):
        assert I.parse_args(enc + ["--quantise-bits", "6", "--entropy-code"] + extra).entropy_code is True
        with pytest.raises(SystemExit):                    # eval through the quantiser is plain mode only
            I.parse_args(ev + ["--quantise-bits", "6", "--entropy-code"] + extra)
    with pytest.raises(SystemExit):                        # decode takes no flag: the file says what it is
        I.parse_args(["decode", "--model_path", "ck", "--latents", "l", "--out", "o", "--entropy-code"])


def test_library_exports_the_coder():
    from video_vae_amd._lib import lib, parse_header
    protos = parse_header()
    for name in ("vvae_rans_supported", "vvae_rans_encode", "vvae_rans_decode"):
        assert name in protos and getattr(lib(), name) is not None
    l = lib()
    assert l.vvae_rans_supported(256, 96, 6) == 1 and l.vvae_rans_supported(1, 1, 2) == 1
    assert l.vvae_rans_supported(256, 96, 9) == 0 and l.vvae_rans_supported(0, 96, 6) == 0 and l.vvae_rans_supported(1 << 20, 1 << 11, 6) == 0


def test_ops_fail_loudly_without_gpu():
    from video_vae_amd import ops
    from video_vae_amd._lib import VvaeError
    freq = _table_of(np.zeros((1, 4, 24), dtype=np.int8), 4)
    with pytest.raises(VvaeError):
        ops.rans_encode(torch.zeros(2, 4, 24, dtype=torch.int8), torch.ones(2), freq, 4)
    with pytest.raises(VvaeError):
        ops.rans_decode(torch.zeros(8, dtype=torch.uint16), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32),
                        torch.zeros(2, 64, dtype=torch.uint32), freq, 4, 4, 24)
