"""The context coder on the host: the numpy definition (video_vae_amd/entropy.py: token energies, thresholds, contexts, the four tables,
encode_context_reference / decode_context_reference), its sizes against the static coder's through the real coder, the latent files with
``ans_ctx``, the committed stream fixture and the parser.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

from video_vae_amd import infer as I
from video_vae_amd.entropy import (CONTEXTS, L, M, CodedFrames, coded_bits, context_counts, context_supported, context_thresholds,
                                   decode_context_reference, decode_reference, encode_context_reference, encode_reference,
                                   normalise_context_counts, normalise_counts, table_size, token_contexts, token_energy)
from video_vae_amd.quant import code_counts, quantise_reference, qmax_of, rate_dataset, rate_summary
from video_vae_amd.tiling import TileGrid, WindowPlan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_entropy_context_stream as G  # noqa: E402


def _model(codes, grid_w, bits):
    """(thr int64 (2,), freq4) of the coded frames, as infer builds them."""
    thr = np.array(context_thresholds(token_energy(codes), grid_w), dtype=np.int64)
    return thr, normalise_context_counts(context_counts(codes, grid_w, thr), bits)


def _round_trip(codes, grid_w, bits, thr=None, freq4=None):
    hw, ld = codes.shape[-2:]
    if thr is None:
        thr, freq4 = _model(codes, grid_w, bits)
    coded = encode_context_reference(codes, freq4, bits, grid_w, thr)
    assert coded.words.dtype == np.uint16 and coded.state.dtype == np.uint32 and int(coded.n_words.sum()) == coded.words.shape[0]
    back = decode_context_reference(coded, freq4, bits, hw, ld, grid_w, thr)
    assert back.dtype == np.int8 and np.array_equal(back, codes.reshape(back.shape))
    return coded, freq4, thr


# ------------------------------------------------------------------------------------------------ energies, thresholds, contexts
@pytest.mark.parametrize("hw,grid_w,ld", [(64, 8, 24), (15, 5, 24), (8, 8, 96)])
def test_context_rule_against_a_plain_loop(hw, grid_w, ld):
    """token_energy / token_contexts / context_counts against a per-symbol Python loop: a full grid, a partial last row, and a frame
    whose tokens all sit in row 0."""
    bits = 6
    codes = G.mixture_codes(2, hw, grid_w, ld, bits, hw + ld)
    energy = token_energy(codes)
    assert energy.dtype == np.int64 and energy.shape == (2, hw)
    thr = context_thresholds(energy, grid_w)
    pool = sorted(int(energy[f, j]) for f in range(2) for j in range(hw - grid_w))
    assert thr == ((pool[len(pool) // 3], pool[2 * len(pool) // 3]) if pool else (0, 0))
    ctx = token_contexts(energy, grid_w, thr)
    counts = np.zeros((2, CONTEXTS, 256), dtype=np.int64)
    for f in range(2):
        for i in range(hw * ld):
            j = i // ld
            e = sum(abs(int(v)) for v in codes[f, j])
            assert e == energy[f, j]
            if j < grid_w:
                want = 0
            else:
                above = sum(abs(int(v)) for v in codes[f, j - grid_w])
                want = 1 + (above > thr[0]) + (above > thr[1])
            assert ctx[f, j] == want, (f, j)
            counts[f, want, int(codes[f, j, i % ld]) + 128] += 1
    assert np.array_equal(context_counts(codes, grid_w, thr), counts)
    assert np.array_equal(counts.sum(axis=(0, 1)), code_counts(codes))
    if hw <= grid_w:
        assert thr == (0, 0) and (ctx == 0).all()
    else:
        assert set(np.unique(ctx)) == {0, 1, 2, 3}


def test_tables():
    bits = 6
    codes = G.mixture_codes(2, 64, 8, 24, bits, 3)
    thr, freq4 = _model(codes, 8, bits)
    counts = context_counts(codes, 8, thr)
    assert freq4.dtype == np.uint16 and freq4.shape == (CONTEXTS, table_size(bits)) and (freq4.astype(np.int64).sum(axis=1) == M).all()
    for k in range(CONTEXTS):
        assert np.array_equal(freq4[k], normalise_counts(counts[:, k], bits))
    assert np.array_equal(freq4, normalise_context_counts(counts.sum(axis=0), bits))           # per-frame rows are pooled
    # a context without a symbol gets the pooled table
    counts[:, 2] = 0
    holed = normalise_context_counts(counts, bits)
    assert np.array_equal(holed[2], normalise_counts(counts.sum(axis=1), bits)) and np.array_equal(holed[[0, 1, 3]], freq4[[0, 1, 3]])
    with pytest.raises(ValueError):
        normalise_context_counts(np.zeros((CONTEXTS, 256), dtype=np.int64), bits)


def test_support_condition():
    # production (16 wide, 96 channels), --small (8, 24), 512-pixel tiles (32, 96); the bound itself
    assert context_supported(256, 96, 6, 16) and context_supported(64, 24, 6, 8) and context_supported(1024, 96, 6, 32)
    assert context_supported(30, 7, 4, 10) and not context_supported(30, 7, 4, 9)
    assert not context_supported(64, 24, 6, 0) and not context_supported(64, 24, 6, 1) and not context_supported(64, 24, 9, 8)
    codes = np.zeros((1, 30, 7), dtype=np.int8)
    freq4 = np.zeros((CONTEXTS, table_size(4)), dtype=np.uint16)
    freq4[:, qmax_of(4)] = M
    with pytest.raises(ValueError, match="grid_w"):
        encode_context_reference(codes, freq4, 4, 9, np.zeros(2, dtype=np.int64))
    # the bound is what the decoder needs: at grid_w = 10 every symbol of the token above sits in an earlier step
    for j in range(10, 30):
        assert ((j - 10 + 1) * 7 - 1) // 64 < (j * 7) // 64


# ------------------------------------------------------------------------------------------------ round trips
@pytest.mark.parametrize("bits", [2, 6, 8])
@pytest.mark.parametrize("frames,hw,grid_w,ld", [(3, 64, 8, 24), (2, 15, 5, 24), (2, 30, 10, 7), (1, 8, 8, 96)])
def test_round_trip(frames, hw, grid_w, ld, bits):
    """Bit for bit, with n a multiple of 64 (1 536, 768), not one (360, 210), and at the bound of the support condition (10 x 7)."""
    codes = G.mixture_codes(frames, hw, grid_w, ld, bits, 100 * bits + hw)
    coded, freq4, thr = _round_trip(codes, grid_w, bits)
    one = encode_context_reference(codes[0], freq4, bits, grid_w, thr)                        # one frame (hw, ld)
    assert np.array_equal(one.words, coded.words[:int(coded.n_words[0])]) and np.array_equal(one.state[0], coded.state[0])


def test_round_trip_special_cases():
    bits = 6
    # an all-zero frame alone: one-symbol tables (freq << 20 is 2^32), no word, every state L
    z = np.zeros((2, 64, 24), dtype=np.int8)
    coded, freq4, thr = _round_trip(z, 8, bits)
    assert thr.tolist() == [0, 0] and (freq4[:, qmax_of(bits)] == M).all()
    assert coded.words.shape == (0,) and (coded.state == L).all()
    # an all-zero frame among others
    codes = G.mixture_codes(3, 64, 8, 24, bits, 5)
    codes[1] = 0
    _round_trip(codes, 8, bits)
    # thr0 == thr1: context 2 is empty and gets the pooled table
    thr = np.array([40, 40], dtype=np.int64)
    counts = context_counts(codes, 8, thr)
    assert counts[:, 2].sum() == 0 and counts[:, 1].sum() > 0 and counts[:, 3].sum() > 0
    freq4 = normalise_context_counts(counts, bits)
    assert np.array_equal(freq4[2], normalise_counts(code_counts(codes), bits))
    _round_trip(codes, 8, bits, thr, freq4)
    # thresholds above every energy: contexts 2 and 3 are empty
    thr = np.array([10 ** 6, 10 ** 6], dtype=np.int64)
    counts = context_counts(codes, 8, thr)
    assert counts[:, 2:].sum() == 0
    _round_trip(codes, 8, bits, thr, normalise_context_counts(counts, bits))
    # a code outside its context's table is refused
    freq4 = normalise_context_counts(counts, bits).copy()
    s = int(np.nonzero(freq4[1])[0][0])
    freq4[1, s + 1] += freq4[1, s]
    freq4[1, s] = 0
    with pytest.raises(ValueError, match="support"):
        encode_context_reference(codes, freq4, bits, 8, thr)


@pytest.mark.parametrize("hw,grid_w,ld", [(64, 8, 24), (15, 5, 24)])
def test_equal_rows_give_the_static_stream(hw, grid_w, ld):
    """With all four rows equal to the static table the stream is encode_reference's word for word, whatever the thresholds."""
    bits = 6
    codes = G.mixture_codes(2, hw, grid_w, ld, bits, 7)
    freq = normalise_counts(code_counts(codes), bits)
    want = encode_reference(codes, freq, bits)
    for thr in ((0, 0), context_thresholds(token_energy(codes), grid_w)):
        got = encode_context_reference(codes, np.stack([freq] * CONTEXTS), bits, grid_w, np.array(thr, dtype=np.int64))
        for a, e in zip(got, want):
            assert a.dtype == e.dtype and np.array_equal(a, e)
        assert np.array_equal(decode_context_reference(want, np.stack([freq] * CONTEXTS), bits, hw, ld, grid_w, np.array(thr)), codes)
        assert np.array_equal(decode_reference(got, freq, bits, hw, ld), codes)


def test_static_coder_is_the_context_coder_with_one_table():
    """Four copies of a static table under any valid layout and thresholds: encode_reference's words, counts and states, and
    decode_context_reference inverts the static stream."""
    bits, hw, ld = 6, 64, 24
    codes = G.mixture_codes(2, hw, 8, ld, bits, 29)
    freq = normalise_counts(code_counts(codes), bits)
    freq4 = np.stack([freq] * CONTEXTS)
    want = encode_reference(codes, freq, bits)
    assert want.words.size > 64
    for grid_w in (4, 8, 13, 64, 100):                     # (grid_w - 1) ld >= 63 from 4 on; no row below the first from 64 on
        for thr in ((0, 0), context_thresholds(token_energy(codes), grid_w), (7, 1000), (10 ** 6, 3)):
            thr = np.array(thr, dtype=np.int64)
            got = encode_context_reference(codes, freq4, bits, grid_w, thr)
            for a, e in zip(got, want):
                assert a.dtype == e.dtype and np.array_equal(a, e), (grid_w, thr)
            assert np.array_equal(decode_context_reference(want, freq4, bits, hw, ld, grid_w, thr), codes), (grid_w, thr)


def test_corrupt_streams():
    """A truncated stream, a flipped word and wrong thresholds each raise ValueError naming the frame or decode to other codes; none
    indexes outside the stream (numpy would raise IndexError)."""
    bits, hw, grid_w, ld = 6, 64, 8, 24
    codes = G.mixture_codes(3, hw, grid_w, ld, bits, 11)
    coded, freq4, thr = _round_trip(codes, grid_w, bits)
    n0 = int(coded.n_words[0])

    def refused_or_different(c, t, frame):
        try:
            back = decode_context_reference(c, freq4, bits, hw, ld, grid_w, t)
        except ValueError as e:
            assert f"frame {frame}" in str(e)
            return
        assert not np.array_equal(back, codes)

    # the last frame's last word missing: it reads zeros past its end
    cut = CodedFrames(coded.words[:-1], np.concatenate([coded.n_words[:-1], coded.n_words[-1:] - 1]), coded.state)
    with pytest.raises(ValueError, match="frame 2"):
        decode_context_reference(cut, freq4, bits, hw, ld, grid_w, thr)
    # a word of the middle frame flipped: its symbols change, so do its energies and every later context
    words = coded.words.copy()
    words[n0 + 5] ^= 0x0100
    refused_or_different(CodedFrames(words, coded.n_words, coded.state), thr, 1)
    # thresholds that are not the encoder's
    refused_or_different(coded, np.array([thr[0] + 25, thr[1] + 60], dtype=np.int64), 0)
    # a count that lies
    with pytest.raises(ValueError):
        decode_context_reference(CodedFrames(coded.words, coded.n_words + 1, coded.state), freq4, bits, hw, ld, grid_w, thr)
    # tables and thresholds of the wrong kind
    with pytest.raises(ValueError):
        decode_context_reference(coded, freq4[0], bits, hw, ld, grid_w, thr)
    with pytest.raises(ValueError):
        decode_context_reference(coded, freq4, bits, hw, ld, grid_w, np.array([1.0, 2.0]))
    with pytest.raises(ValueError):
        decode_context_reference(coded, freq4, bits, hw, ld, 1, thr)


# ------------------------------------------------------------------------------------------------ sizes, through the real coder
def _source(mixture):
    """Two frames of 16 x 16 tokens x 96 channels: standard normals (default_rng(0)), times sigma[r, c] = exp(sin(2 pi r / 16) +
    cos(2 pi c / 16)) for the scale mixture."""
    rng = np.random.default_rng(0)
    r, c = np.arange(16)[:, None], np.arange(16)[None]
    sigma = np.exp(np.sin(2 * np.pi * r / 16) + np.cos(2 * np.pi * c / 16))
    x = rng.standard_normal((2, 16, 16, 96))
    if mixture:
        x = x * sigma[None, :, :, None]
    return x.reshape(2, 256, 96).astype(np.float32)


@pytest.mark.parametrize("mixture,bits,cap", [(True, 6, 0.95), (True, 4, 0.88), (False, 6, 1.03)])
def test_sizes_against_the_static_coder(mixture, bits, cap):
    """coded_bits of the context stream against the static stream's, tables and thresholds included, both through the reference coder.
    Measured: 0.9247 (mixture, 6 bits), 0.8534 (mixture, 4 bits), 1.0109 (i.i.d. normals, 6 bits)."""
    codes, _ = quantise_reference(_source(mixture), bits)
    freq = normalise_counts(code_counts(codes), bits)
    static = encode_reference(codes, freq, bits)
    coded, freq4, thr = _round_trip(codes, 16, bits)
    ratio = coded_bits(coded, freq4) / coded_bits(static, freq)
    print(f"context / static coded_bits: {ratio:.4f} (cap {cap})")
    assert ratio <= cap


def test_coded_bits_formula():
    bits = 6
    codes = G.mixture_codes(3, 64, 8, 24, bits, 13)
    coded, freq4, _ = _round_trip(codes, 8, bits)
    assert coded_bits(coded, freq4) == 16 * coded.words.shape[0] + 3 * (64 * 32 + 32) + 16 * 4 * (2 * qmax_of(bits) + 1) + 3 * 32
    freq = normalise_counts(code_counts(codes), bits)                                          # the static size is what it was
    static = encode_reference(codes, freq, bits)
    assert coded_bits(static, freq) == 16 * static.words.shape[0] + 3 * (64 * 32 + 32) + 16 * (2 * qmax_of(bits) + 1)


def test_rate_summary_with_context_bits():
    counts = np.zeros(256, dtype=np.int64)
    counts[[100, 128, 129, 200]] = 6
    sel = np.array([1, 0, 1, 0, 0])
    base = rate_summary(counts, sel, n_frames=5, height=4, width=6, ld=3, bits=8, coded=5000)
    r = rate_summary(counts, sel, n_frames=5, height=4, width=6, ld=3, bits=8, coded=5000, coded_context=4000)
    assert {k: r[k] for k in base} == base                                                     # the static figures do not move
    assert r["bits_coded_context"] == 4000 + base["bits_side"] and r["bpp_coded_context"] == r["bits_coded_context"] / 120
    d = rate_dataset([r, dict(r, bits_coded_context=7000, pixels=80)])
    assert d["bits_coded_context"] == r["bits_coded_context"] + 7000 and d["bpp_coded_context"] == d["bits_coded_context"] / 200
    assert "bits_coded_context" not in rate_dataset([r, base]) and "bits_coded_context" not in rate_dataset([base])


# ------------------------------------------------------------------------------------------------ the committed stream
def test_context_stream_fixture_reproduces():
    """tests/golden/entropy_context_stream.npz (two frames of 33 x 24 at 4 bits, 5 tokens wide) is what the definition makes today,
    member for member, and decodes to its codes."""
    rec = G.record()
    with np.load(os.path.join(GOLDEN, "entropy_context_stream.npz")) as z:
        stored = {k: z[k] for k in z.files}
    assert sorted(stored) == sorted(rec)
    for k in rec:
        assert stored[k].dtype == np.asarray(rec[k]).dtype and np.array_equal(stored[k], rec[k]), k
    assert stored["codes"].shape == (G.FRAMES, G.HW, G.LD) and int(stored["bits"]) == G.BITS and int(stored["grid_w"]) == G.GRID_W
    assert stored["freq"].shape == (CONTEXTS, table_size(G.BITS)) and int(stored["n_words"].sum()) == stored["words"].shape[0] > 0
    assert stored["thr"][0] < stored["thr"][1]
    assert set(np.unique(token_contexts(token_energy(stored["codes"]), G.GRID_W, stored["thr"]))) == {0, 1, 2, 3}
    back = decode_context_reference(CodedFrames(stored["words"], stored["n_words"], stored["state"]), stored["freq"], G.BITS, G.HW, G.LD,
                                    G.GRID_W, stored["thr"])
    assert np.array_equal(back, stored["codes"])


# ------------------------------------------------------------------------------------------------ latent files
HW, GRID_W, LD = 16, 4, 24
FILL = torch.linspace(-0.5, 0.5, LD)
CTX_KEYS = ["mean_ans", "ans_words", "ans_state", "ans_freq", "ans_shape", "ans_ctx", "mean_step", "quant_bits"]
ANS_KEYS = [k for k in CTX_KEYS if k != "ans_ctx"]


def _latent(shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape + (HW, LD)) * rng.uniform(0.01, 3.0, size=shape + (HW, 1))
    return torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).float().numpy()


def _quant_and_entropy(x, kept, bits):
    """(quant, static entropy, context entropy) of dense means x with ``kept`` bool (x's leading shape)."""
    q, step = quantise_reference(x.reshape((-1, HW, LD)), bits)
    quant = (torch.from_numpy(q.reshape(x.shape)), torch.from_numpy(step.reshape(x.shape[:-2] + (LD,))), bits)
    sub = q[kept.reshape(-1)]
    freq = normalise_counts(code_counts(sub), bits)
    thr, freq4 = _model(sub, GRID_W, bits)
    return quant, (encode_reference(sub, freq, bits), freq), \
        (encode_context_reference(sub, freq4, bits, GRID_W, thr), freq4, (GRID_W, int(thr[0]), int(thr[1])))


def _same_dense(a, b):
    assert len(a) == len(b)
    assert a[0].dtype == np.float32 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for x, y in zip(a[2:], b[2:]):
        assert x == y


def test_pack_unpack_plain_context(tmp_path):
    bits = 6
    x = _latent((5,), 21)
    sel = np.array([1, 0, 1, 1, 0], dtype=np.float32)
    quant, static, context = _quant_and_entropy(x, sel != 0, bits)
    args = (torch.from_numpy(x), torch.from_numpy(sel))
    plain = I.pack_latents(*args, quant=quant)
    old = I.pack_latents(*args, quant=quant, entropy=static)
    assert list(old) == ANS_KEYS + ["selection", "n_frames"] and old["ans_freq"].shape == (table_size(bits),)     # without the flag: as it was
    arrays = I.pack_latents(*args, quant=quant, entropy=context)
    assert list(arrays) == CTX_KEYS + ["selection", "n_frames"]
    assert arrays["ans_freq"].dtype == np.uint16 and arrays["ans_freq"].shape == (CONTEXTS, table_size(bits))
    assert arrays["ans_ctx"].dtype == np.int64 and arrays["ans_ctx"].tolist() == list(context[2])
    assert np.array_equal(arrays["mean_ans"], context[0].words) and arrays["ans_shape"].tolist() == [HW, LD]
    for k in ("mean_step", "quant_bits", "selection", "n_frames", "ans_shape"):
        assert np.array_equal(arrays[k], old[k]), k
    _same_dense(I.unpack_latents(arrays, FILL), I.unpack_latents(plain, FILL))
    I.save_latents(str(tmp_path / "c.npz"), arrays)
    with np.load(tmp_path / "c.npz") as z:
        back = {k: z[k] for k in z.files}
    assert list(back) == list(arrays)
    _same_dense(I.unpack_latents(back, FILL), I.unpack_latents(plain, FILL))
    # a stream that fails the end check names the file's frame; members that do not fit raise
    state = arrays["ans_state"].copy()
    state[1, 0] ^= 0x00010000
    with pytest.raises(ValueError, match="frame 1"):
        I.unpack_latents(dict(arrays, ans_state=state), FILL)
    for bad in (dict(arrays, ans_ctx=arrays["ans_ctx"][:2]), dict(arrays, ans_ctx=np.array([1, 0, 0], dtype=np.int64)),
                dict(arrays, ans_freq=arrays["ans_freq"][0]), dict(old, ans_freq=arrays["ans_freq"])):
        with pytest.raises(ValueError):
            I.unpack_latents(bad, FILL)
    with pytest.raises(ValueError):                        # four tables need the layout and the thresholds
        I.pack_latents(*args, quant=quant, entropy=context[:2])
    with pytest.raises(ValueError):                        # a layout outside the support condition
        I.pack_latents(*args, quant=quant, entropy=(context[0], context[1], (1, 0, 0)))


def test_pack_unpack_tiled_and_windows_context():
    bits = 4
    grid = TileGrid(40, 56, 32, 8)
    x = _latent((4, 5), 22)
    sel = np.random.default_rng(0).random((4, 5)) < 0.6
    quant, static, context = _quant_and_entropy(x, sel, bits)
    args = (torch.from_numpy(x), torch.from_numpy(sel.astype(np.float32)), grid)
    arrays = I.pack_latents_tiled(*args, quant=quant, entropy=context)
    assert list(arrays) == ["tile_grid"] + CTX_KEYS + ["selection", "n_frames"]
    assert list(I.pack_latents_tiled(*args, quant=quant, entropy=static)) == ["tile_grid"] + ANS_KEYS + ["selection", "n_frames"]
    _same_dense(I.unpack_latents_tiled(arrays, FILL), I.unpack_latents_tiled(I.pack_latents_tiled(*args, quant=quant), FILL))
    one = TileGrid(32, 32, 32, 0)
    plan = WindowPlan(10, 4, 1)
    xw = _latent((plan.windows, 1, 4), 23)
    selw = np.random.default_rng(1).random((plan.windows, 1, 4)) < 0.7
    quant, static, context = _quant_and_entropy(xw, selw, bits)
    args = (torch.from_numpy(xw), torch.from_numpy(selw.astype(np.float32)), one, plan)
    arrays = I.pack_latents_windows(*args, quant=quant, entropy=context)
    assert list(arrays) == ["tile_grid", "window_starts", "temporal_overlap", "window", "n_frames"] + CTX_KEYS + ["selection"]
    _same_dense(I.unpack_latents_windows(arrays, FILL), I.unpack_latents_windows(I.pack_latents_windows(*args, quant=quant), FILL))


# ------------------------------------------------------------------------------------------------ parser, library
def test_parser_entropy_context(capsys):
    enc = ["encode", "--model_path", "ck", "--data", "d", "--out", "o"]
    ev = ["eval", "--model_path", "ck", "--data", "d"]
    for cmd in (enc, ev):
        a = I.parse_args(cmd + ["--quantise-bits", "6", "--entropy-code"])
        assert a.entropy_code is True and a.entropy_context is False                            # off by default
        assert I.parse_args(cmd + ["--quantise-bits", "6", "--entropy-code", "--entropy-context"]).entropy_context is True
        for rest in (["--entropy-context"], ["--quantise-bits", "6", "--entropy-context"]):
            with pytest.raises(SystemExit) as e:
                I.parse_args(cmd + rest)
            assert e.value.code == 2
            assert "--entropy-code" in capsys.readouterr().err
    for extra in (["--tile"], ["--temporal-overlap", "2"], ["--scene-cuts"]):
        assert I.parse_args(enc + ["--quantise-bits", "6", "--entropy-code", "--entropy-context"] + extra).entropy_context is True
    with pytest.raises(SystemExit):                        # decode takes no flag: the file says what it is
        I.parse_args(["decode", "--model_path", "ck", "--latents", "l", "--out", "o", "--entropy-context"])


def test_library_exports_the_context_coder():
    from video_vae_amd._lib import lib, parse_header
    protos = parse_header()
    for name in ("vvae_rans_context_supported", "vvae_rans_context_counts", "vvae_rans_encode_ctx", "vvae_rans_decode_ctx"):
        assert name in protos and getattr(lib(), name) is not None
    s = lib().vvae_rans_context_supported
    assert s(256, 96, 6, 16) == 1 and s(64, 24, 6, 8) == 1 and s(1024, 96, 6, 32) == 1 and s(8, 96, 6, 8) == 1
    assert s(30, 7, 4, 10) == 1 and s(30, 7, 4, 9) == 0 and s(64, 24, 6, 1) == 0 and s(64, 24, 6, 0) == 0 and s(64, 24, 9, 8) == 0
    assert s(4096, 96, 6, 64) == 1 and s(4097, 96, 6, 64) == 0                                   # the energies must fit in LDS
    for hw, ld, bits, grid_w in ((256, 96, 6, 16), (30, 7, 4, 10), (30, 7, 4, 9), (64, 24, 9, 8)):
        assert bool(s(hw, ld, bits, grid_w)) == context_supported(hw, ld, bits, grid_w)


def test_ops_fail_loudly_without_gpu():
    from video_vae_amd import ops
    from video_vae_amd._lib import VvaeError
    freq4 = np.zeros((CONTEXTS, table_size(4)), dtype=np.uint16)
    freq4[:, 7] = M
    c, k = torch.zeros(2, 16, 24, dtype=torch.int8), torch.ones(2)
    with pytest.raises(VvaeError):
        ops.rans_context_counts(c, k, 4, 4, (0, 0))
    with pytest.raises(VvaeError):
        ops.rans_encode_context(c, k, freq4, 4, 4, (0, 0))
    with pytest.raises(VvaeError):
        ops.rans_decode_context(torch.zeros(8, dtype=torch.uint16), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32),
                                torch.zeros(2, 64, dtype=torch.uint32), freq4, 4, 16, 24, 4, (0, 0))
