"""The context coder on the GPU: ops.rans_context_counts / ops.rans_encode_context / ops.rans_decode_context (csrc/rans.hip) against
entropy.context_counts / encode_context_reference / decode_context_reference on every count, word, state and code, inside a captured
graph, and through infer encode / decode / eval --entropy-context.  Every comparison is exact."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from video_vae_amd.entropy import (CONTEXTS, L, M, CodedFrames, capacity, coded_bits, context_counts, context_thresholds,
                                   decode_context_reference, encode_context_reference, gather_streams, normalise_context_counts,
                                   table_size, token_energy)
from video_vae_amd.quant import qmax_of, rate_dataset

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_entropy_context_stream import mixture_codes  # noqa: E402
from util import capacity_offsets, coded_garbage  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = 64          # the --small model at 64 x 64 frames: hw = 16 (4 tokens wide), ld = 96 (tests/test_gpu_infer.py)
FORMS = (None, "compact", "full")          # the library's pick (by frames against CUs) and both slot-table forms
# (frames, hw, grid_w, ld, bits): the --small model's frame; a partial last row and a partial last step (n = 360); the production frame;
# 2 and 8 bits; the bound of the support condition, (grid_w - 1) ld = 63, with an ld that is no multiple of 4 (energies read by bytes);
# energies read by bytes again, with a partial last step (n = 12 350) and a stream that crosses ring refills
CASES = [(3, 64, 8, 24, 6), (2, 15, 5, 24, 6), (2, 256, 16, 96, 6), (2, 64, 8, 24, 2), (2, 64, 8, 24, 8), (2, 30, 10, 7, 4),
         (2, 130, 13, 95, 6)]


def _model(codes, grid_w, bits):
    thr = context_thresholds(token_energy(codes), grid_w)
    return thr, normalise_context_counts(context_counts(codes, grid_w, thr), bits)


def _check(dev, codes, keep, grid_w, bits):
    """Counts, encode and decode (both slot forms, from the capacity layout and from concatenated streams) of ``codes`` under ``keep``
    against the definition of the kept frames; the dropped frames: zero counts, no words, states L."""
    from video_vae_amd import ops
    frames, hw, ld = codes.shape
    assert ops.rans_context_supported(hw, ld, bits, grid_w)
    k = keep != 0
    thr, freq4 = _model(codes[k], grid_w, bits)
    cd, kd = torch.from_numpy(codes).to(dev), torch.from_numpy(keep).to(dev)
    counts = ops.rans_context_counts(cd, kd, bits, grid_w, thr)
    assert counts.dtype == torch.int32 and counts.shape == (frames, CONTEXTS, 256)
    counts = counts.cpu().numpy()
    assert np.array_equal(counts[k], context_counts(codes[k], grid_w, thr)) and (counts[~k] == 0).all()
    assert np.array_equal(normalise_context_counts(counts, bits), freq4)
    cap = capacity(hw * ld)
    out = ops.rans_encode_context(cd, kd, freq4, bits, grid_w, thr, out=coded_garbage(frames, cap, dev))
    assert out.words.shape == (frames, cap) and out.n_words.shape == (frames,) and out.state.shape == (frames, 64)
    want = encode_context_reference(codes[k], freq4, bits, grid_w, np.array(thr))
    got = gather_streams(out.words, out.n_words, out.state, keep=keep)
    assert np.array_equal(got.n_words, want.n_words), (got.n_words, want.n_words)
    assert np.array_equal(got.state, want.state) and np.array_equal(got.words, want.words)
    n_words, state = out.n_words.cpu().numpy(), out.state.cpu().numpy()
    assert (n_words[~k] == 0).all() and (state[~k] == L).all()
    offs = np.concatenate([[0], np.cumsum(want.n_words)[:-1]]).astype(np.int64)
    words = torch.from_numpy(want.words if want.words.size else np.zeros(1, dtype=np.uint16)).to(dev)
    for form in FORMS:
        back, ok = ops.rans_decode_context(out.words, capacity_offsets(out.n_words, cap, dev), out.n_words, out.state, freq4, bits, hw, ld,
                                           grid_w, thr, slot_form=form)
        assert back.dtype == torch.int8 and back.shape == (frames, hw, ld) and ok.dtype == torch.int32
        assert np.array_equal(back.cpu().numpy()[k], codes[k]) and (ok.cpu().numpy()[k] == 1).all(), form
        back, ok = ops.rans_decode_context(words, torch.from_numpy(offs).to(dev), torch.from_numpy(want.n_words).to(dev),
                                           torch.from_numpy(want.state).to(dev), freq4, bits, hw, ld, grid_w, thr, slot_form=form)
        assert np.array_equal(back.cpu().numpy(), codes[k]) and (ok.cpu().numpy() == 1).all(), form
    return want, freq4, thr


@pytest.mark.parametrize("frames,hw,grid_w,ld,bits", CASES)
def test_kernels_equal_the_definition(dev, frames, hw, grid_w, ld, bits):
    codes = mixture_codes(frames, hw, grid_w, ld, bits, 1000 * frames + hw + ld + bits)
    want, freq4, thr = _check(dev, codes, np.ones(frames, dtype=np.float32), grid_w, bits)
    assert np.array_equal(decode_context_reference(want, freq4, bits, hw, ld, grid_w, np.array(thr)), codes)
    if hw > 2 * grid_w:
        assert thr[0] < thr[1] and int((freq4 != freq4[0]).any(axis=1).sum()) >= 2              # the contexts are in use


def test_static_coder_is_the_context_coder_with_one_table(dev):
    """Four copies of a static table: ops.rans_encode_context writes ops.rans_encode's words, counts and states, and both slot forms of
    ops.rans_decode_context return the codes of ops.rans_decode with ok all 1."""
    from video_vae_amd import ops
    from video_vae_amd.entropy import normalise_counts
    from video_vae_amd.quant import code_counts
    frames, hw, grid_w, ld, bits = 2, 64, 8, 24, 6
    codes = mixture_codes(frames, hw, grid_w, ld, bits, 31)
    freq = normalise_counts(code_counts(codes), bits)
    freq4 = np.stack([freq] * CONTEXTS)
    thr = context_thresholds(token_energy(codes), grid_w)
    cap = capacity(hw * ld)
    cd, keep = torch.from_numpy(codes).to(dev), torch.ones(frames, device=dev)
    static = ops.rans_encode(cd, keep, freq, bits, out=coded_garbage(frames, cap, dev))
    context = ops.rans_encode_context(cd, keep, freq4, bits, grid_w, thr, out=coded_garbage(frames, cap, dev))
    assert int(static.n_words.min()) > 64
    for a, e in zip(gather_streams(*context), gather_streams(*static)):
        assert a.dtype == e.dtype and np.array_equal(a, e)
    assert torch.equal(context.n_words, static.n_words) and torch.equal(context.state, static.state)
    offsets = capacity_offsets(static.n_words, cap, dev)
    want, ok = ops.rans_decode(static.words, offsets, static.n_words, static.state, freq, bits, hw, ld)
    assert np.array_equal(want.cpu().numpy(), codes) and (ok.cpu().numpy() == 1).all()
    for form in ("compact", "full"):
        back, ok = ops.rans_decode_context(context.words, offsets, context.n_words, context.state, freq4, bits, hw, ld, grid_w, thr,
                                           slot_form=form)
        assert torch.equal(back, want) and (ok.cpu().numpy() == 1).all(), form


def test_dropped_frames(dev):
    codes = mixture_codes(4, 64, 8, 24, 6, 17)
    _check(dev, codes, np.array([2.5, 1, 0, 1], dtype=np.float32), 8, 6)                        # any nonzero flag keeps
    _check(dev, codes, np.array([0, 0, 1, 0], dtype=np.float32), 8, 6)


def test_all_zero_frames(dev):
    from video_vae_amd import ops
    # alone: one-symbol tables (freq << 20 is 2^32), no word, every state L, and it decodes
    z = np.zeros((2, 64, 24), dtype=np.int8)
    want, freq4, thr = _check(dev, z, np.ones(2, dtype=np.float32), 8, 6)
    assert thr == (0, 0) and (freq4[:, qmax_of(6)] == M).all() and want.words.size == 0 and (want.state == L).all()
    # among others, under the clip's tables
    codes = mixture_codes(3, 64, 8, 24, 6, 19)
    codes[1] = 0
    _check(dev, codes, np.ones(3, dtype=np.float32), 8, 6)
    # equal thresholds: an empty context with the pooled table
    thr = (40, 40)
    counts = ops.rans_context_counts(torch.from_numpy(codes).to(dev), torch.ones(3, device=dev), 6, 8, thr).cpu().numpy()
    assert np.array_equal(counts, context_counts(codes, 8, thr)) and counts[:, 2].sum() == 0
    freq4 = normalise_context_counts(counts, 6)
    out = ops.rans_encode_context(torch.from_numpy(codes).to(dev), torch.ones(3, device=dev), freq4, 6, 8, thr)
    want = encode_context_reference(codes, freq4, 6, 8, np.array(thr))
    for a, e in zip(gather_streams(*out), want):
        assert np.array_equal(a, e)


def test_decode_ok(dev):
    """A valid stream: ok 1.  One word removed from the middle frame's stream, and a count that lies: ok 0 for that frame only, the
    neighbours' codes exact.  The words tensor carries a whole frame's capacity of spare words behind the last stream."""
    from video_vae_amd import ops
    bits, frames, hw, grid_w, ld = 6, 3, 64, 8, 24
    codes = mixture_codes(frames, hw, grid_w, ld, bits, 23)
    thr, freq4 = _model(codes, grid_w, bits)
    coded = encode_context_reference(codes, freq4, bits, grid_w, np.array(thr))
    spare = np.zeros(capacity(hw * ld), dtype=np.uint16)
    n = coded.n_words
    offs = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    state = torch.from_numpy(coded.state).to(dev)

    def run(words, offsets, n_words, form):
        back, ok = ops.rans_decode_context(torch.from_numpy(np.concatenate([words, spare])).to(dev), torch.from_numpy(offsets).to(dev),
                                           torch.from_numpy(n_words).to(dev), state, freq4, bits, hw, ld, grid_w, thr, slot_form=form)
        return back.cpu().numpy(), ok.cpu().numpy().tolist()

    for form in FORMS:
        back, ok = run(coded.words, offs, n, form)
        assert ok == [1, 1, 1] and np.array_equal(back, codes)
        # the middle frame's stream without its 18th word
        at = int(n[0]) + 17
        cut = np.concatenate([coded.words[:at], coded.words[at + 1:]])
        n_cut = n - np.array([0, 1, 0])
        back, ok = run(cut, np.concatenate([[0], np.cumsum(n_cut)[:-1]]).astype(np.int64), n_cut, form)
        assert ok == [1, 0, 1] and np.array_equal(back[[0, 2]], codes[[0, 2]])
        with pytest.raises(ValueError, match="frame 1"):   # the definition refuses it too
            decode_context_reference(CodedFrames(cut, n_cut, coded.state), freq4, bits, hw, ld, grid_w, np.array(thr))
        # a count that claims one word more, and one that claims one fewer
        for d in (1, -1):
            back, ok = run(coded.words, offs, n + np.array([0, d, 0]), form)
            assert ok == [1, 0, 1] and np.array_equal(back[[0, 2]], codes[[0, 2]]), d
        # counts and offsets that point outside the words: ok 0, nothing read out there
        back, ok = run(coded.words, np.array([0, 1 << 40, -5], dtype=np.int64), n, form)
        assert ok == [1, 0, 0] and np.array_equal(back[0], codes[0])


def test_refusals(dev):
    from video_vae_amd import ops
    from video_vae_amd._lib import VvaeError
    assert ops.rans_context_supported(256, 96, 6, 16) and ops.rans_context_supported(30, 7, 4, 10)
    assert not ops.rans_context_supported(30, 7, 4, 9) and not ops.rans_context_supported(4097, 96, 6, 64)
    c, k = torch.zeros(2, 16, 24, dtype=torch.int8, device=dev), torch.ones(2, device=dev)
    freq4 = np.zeros((CONTEXTS, table_size(4)), dtype=np.uint16)
    freq4[:, 7] = M
    dec = (torch.from_numpy(np.zeros(8, dtype=np.uint16)).to(dev), torch.zeros(2, dtype=torch.int64, device=dev),
           torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(2, 64, dtype=torch.int32, device=dev))
    for bad in (lambda: ops.rans_context_counts(c, k, 4, 1, (0, 0)), lambda: ops.rans_context_counts(c, k, 4, 4, (-1, 0)),
                lambda: ops.rans_context_counts(c.cpu(), k.cpu(), 4, 4, (0, 0)), lambda: ops.rans_encode_context(c, k, freq4, 4, 3, (0, 0)),
                lambda: ops.rans_encode_context(c, k, freq4[0], 4, 4, (0, 0)), lambda: ops.rans_encode_context(c, k, freq4[:, :-1], 4, 4, (0, 0)),
                lambda: ops.rans_encode_context(c, torch.ones(3, device=dev), freq4, 4, 4, (0, 0)),
                lambda: ops.rans_decode_context(*dec, freq4, 4, 16, 24, 1, (0, 0)),
                lambda: ops.rans_decode_context(*dec, freq4, 4, 16, 24, 4, (0, 0), slot_form="other"),
                lambda: ops.rans_decode_context(*dec, freq4[0], 4, 16, 24, 4, (0, 0))):
        with pytest.raises(VvaeError):
            bad()


def test_captured_and_replayed_equals_eager(dev):
    """Counts, encode and decode (both slot forms) on one stream inside one captured graph, replayed on other codes, flags and tables
    copied into the static inputs between the replays: the eager results on every bit, twice; the graph holds no memset node."""
    from video_vae_amd import ops
    from video_vae_amd.graph import graph_node_census
    frames, hw, grid_w, ld, bits = 4, 64, 8, 24, 6
    cap = capacity(hw * ld)
    datas = [mixture_codes(frames, hw, grid_w, ld, bits, s) // d for s, d in ((1, 1), (2, 3))]
    thr = (30, 90)                                         # fixed in the capture: kernel arguments
    tables = [torch.from_numpy(normalise_context_counts(context_counts(c, grid_w, thr), bits)).to(dev) for c in datas]
    assert not torch.equal(tables[0].cpu(), tables[1].cpu())
    datas = [torch.from_numpy(c).to(dev) for c in datas]
    keeps = [torch.tensor([1, 0, 1, 1.0], device=dev), torch.tensor([0, 1, 1, 0.0], device=dev)]
    codes, keep, table = datas[0].clone(), keeps[0].clone(), tables[0].clone()
    base = torch.arange(frames, device=dev, dtype=torch.int64) * cap + cap

    def run(c, k, t):
        counts = ops.rans_context_counts(c, k, bits, grid_w, thr)
        out = ops.rans_encode_context(c, k, t, bits, grid_w, thr)
        return counts, out, [ops.rans_decode_context(out.words, base - out.n_words, out.n_words, out.state, t, bits, hw, ld, grid_w, thr,
                                                     slot_form=form) for form in FORMS]

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
        counts, out, backs = run(codes, keep, table)
    census = graph_node_census(g)
    assert census is not None and census.get("memset", 0) == 0 and census.get("kernel", 0) >= 4, census
    for i in (0, 1, 1, 0):
        codes.copy_(datas[i])
        keep.copy_(keeps[i])
        table.copy_(tables[i])
        g.replay()
        torch.cuda.synchronize()
        k = keeps[i].cpu().numpy() != 0
        host = datas[i].cpu().numpy()
        assert np.array_equal(counts.cpu().numpy()[k], context_counts(host[k], grid_w, thr)) and (counts.cpu().numpy()[~k] == 0).all(), i
        want = encode_context_reference(host[k], tables[i].cpu().numpy(), bits, grid_w, np.array(thr))
        for a, e in zip(gather_streams(*out, keep=keeps[i]), want):
            assert np.array_equal(a, e), i
        assert (out.n_words.cpu().numpy()[~k] == 0).all() and (out.state.cpu().numpy()[~k] == L).all(), i
        for back, ok in backs:
            assert np.array_equal(back.cpu().numpy()[k], host[k]) and (ok.cpu().numpy()[k] == 1).all(), i


# ------------------------------------------------------------------------------------------------ the command line
def _small(seed=9):
    from video_vae_amd.infer import model_config
    import video_vae_amd as V
    return V.VideoVAE(rngs=V.Rngs(seed), **model_config(SMALL, True))


def test_cli_entropy_context_encode_decode_eval(dev, tmp_path):
    """infer encode --small --quantise-bits 6 --entropy-code --entropy-context, decode and eval (run in this process: infer.main) on two
    short synthetic clips: the file holds the definition's context stream of the quantised file's codes, decodes to the frames of the run
    without --entropy-context byte for byte, and eval prints both sizes with bpp_coded unmoved."""
    import video_vae_amd as V
    from video_vae_amd import data as D
    from video_vae_amd import infer as I
    bits, grid_w = 6, 4
    data = str(tmp_path / "data")
    D.write_synthetic_clips(data, 2, 10, 40, 48, seed=1)                          # clip 0: 8 frames, clip 1: 10 frames
    V.save_checkpoint(_small(), None, str(tmp_path / "ckpt"))
    ck = ["--model_path", str(tmp_path / "ckpt")]
    common = ck + ["--data", data, "--size", str(SMALL), "--frames", "4", "--batch", "2", "--small", "--flavour", "model"]
    quant = ["--quantise-bits", str(bits)]
    I.main(["encode"] + common + quant + ["--out", str(tmp_path / "latq")])
    I.main(["encode"] + common + quant + ["--entropy-code", "--out", str(tmp_path / "lata")])
    I.main(["encode"] + common + quant + ["--entropy-code", "--entropy-context", "--out", str(tmp_path / "latc")])
    names = ("clip0000", "clip0001")
    sizes = {}
    for name in names:
        with np.load(tmp_path / "latq" / f"{name}.npz") as z:
            q = {k: z[k] for k in z.files}
        with np.load(tmp_path / "lata" / f"{name}.npz") as z:
            a = {k: z[k] for k in z.files}
        with np.load(tmp_path / "latc" / f"{name}.npz") as z:
            c = {k: z[k] for k in z.files}
        assert "ans_ctx" not in a and a["ans_freq"].shape == (table_size(bits),)                  # without the flag: the static file
        assert "mean_q" not in c and q["mean_q"].shape[0] > 0 and list(q["mean_q"].shape[1:]) == [16, 96]
        thr, freq4 = _model(q["mean_q"], grid_w, bits)
        want = encode_context_reference(q["mean_q"], freq4, bits, grid_w, np.array(thr))
        assert c["ans_ctx"].dtype == np.int64 and c["ans_ctx"].tolist() == [grid_w, thr[0], thr[1]]
        assert c["ans_freq"].dtype == np.uint16 and np.array_equal(c["ans_freq"], freq4)
        assert c["ans_shape"].tolist() == [16, 96]
        assert c["mean_ans"].dtype == np.uint16 and np.array_equal(c["mean_ans"], want.words)
        assert np.array_equal(c["ans_words"], want.n_words) and np.array_equal(c["ans_state"], want.state)
        for k in q:
            if k != "mean_q":
                assert np.array_equal(q[k], c[k]), k
        sizes[name] = coded_bits(want, freq4)
    I.main(["decode"] + ck + ["--latents", str(tmp_path / "lata"), "--out", str(tmp_path / "reca"), "--batch", "2"])
    I.main(["decode"] + ck + ["--latents", str(tmp_path / "latc"), "--out", str(tmp_path / "recc"), "--batch", "2"])
    for name in names:
        with np.load(tmp_path / "recc" / f"{name}.npz") as x, np.load(tmp_path / "reca" / f"{name}.npz") as e:
            assert x["frames"].dtype == np.uint8 and np.array_equal(x["frames"], e["frames"]), name
    I.main(["eval"] + common + quant + ["--entropy-code", "--per-frame", "--out", str(tmp_path / "ma.json")])
    I.main(["eval"] + common + quant + ["--entropy-code", "--entropy-context", "--per-frame", "--out", str(tmp_path / "mc.json")])
    ra, rc = json.loads((tmp_path / "ma.json").read_text()), json.loads((tmp_path / "mc.json").read_text())
    assert rc["config"]["entropy_context"] is True and "entropy_context" not in ra["config"]
    ca, cc = {c["name"]: c for c in ra["clips"]}, {c["name"]: c for c in rc["clips"]}
    for name in names:
        e, p = cc[name], ca[name]
        assert e["bits_coded_context"] == sizes[name] + e["bits_side"] == e["rate"]["bits_coded_context"]
        assert e["bpp_coded_context"] == e["bits_coded_context"] / e["rate"]["pixels"]
        assert "bits_coded_context" not in p and "bits_coded_context" not in p["rate"]
        for k in ("psnr", "ssim", "mse", "kept_fraction", "bpp_raw", "bpp_entropy", "bits_side", "bits_coded", "bpp_coded"):
            assert e[k] == p[k], (name, k)
        assert e["per_frame"] == p["per_frame"]
    d = rate_dataset(cc[name]["rate"] for name in names)
    assert rc["dataset"]["bits_coded_context"] == d["bits_coded_context"] == sum(cc[name]["bits_coded_context"] for name in names)
    assert rc["dataset"]["bpp_coded_context"] == d["bpp_coded_context"]
    for k in ("psnr", "ssim", "mse", "bpp_raw", "bpp_entropy", "bits_coded", "bpp_coded"):
        assert rc["dataset"][k] == ra["dataset"][k], k
    assert "bits_coded_context" not in ra["dataset"]
