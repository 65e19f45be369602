"""What the range coder costs and what it saves.

  * the kernels alone: ops.rans_encode and ops.rans_decode on seeded Laplacian codes at the production frame (256 x 96 symbols, 6 bits,
    every frame kept, one table), for 16 and 64 frames; HIP events around --burst back-to-back launches, median of --repeats bursts, per
    launch.  One wavefront per frame: the time is that of 384 dependent steps, whatever the frame count below the CU count.
  * the files: synthetic clips (data.write_synthetic_clips) through the "encode" graph with the quantiser at --bits (the full C3 model
    with seeded random weights, or --model_path; --size 256, --frames 16, --batch 4, the deterministic gate); per clip the deflated int8
    file of ``--quantise-bits`` and the range-coded file of ``--entropy-code`` (infer.pack_latents + save_latents) -> bpp_file of each;
    bpp_coded (entropy.coded_bits + the side bits) against bpp_entropy (quant.rate_summary), ratios of sums over the clips.

  * --context: beside each of the above the context coder (four tables, a symbol's table chosen by the activity of the token above):
    ops.rans_context_counts, ops.rans_encode_context and ops.rans_decode_context in both slot-table forms, timed in the same run as the
    static kernels; the files and bpp_coded_context of ``--entropy-context``.

  * --temporal: the temporal coder (nine tables, a symbol's table chosen by the previous frame's code at the same place) on seeded
    AR(1) codes (rho 0.9) in chains of 16 frames: ops.rans_temporal_counts and ops.rans_encode_temporal at 16 and 1024 frames,
    ops.rans_decode_temporal (one wavefront per chain) at 1, 16 and 256 chains, each beside the static and the context kernels on the same
    codes in the same run; and the files and bpp_coded_temporal of ``--entropy-temporal``.

Random weights have no meaningful rate: the numbers are recorded, not judged.

    python tools/entropy_bench.py [--clips 4] [--clip-frames 48] [--bits 6] [--repeats 20] [--context] [--temporal] [--out profiles/r15_entropy_bench.txt]
"""
import argparse
import os
import sys
import tempfile

sys.path.insert(0, ".")
import numpy as np
import torch

SIZE, T, B = 256, 16, 4
HW, LD, GRID_W = 256, 96, 16


def _median(v):
    return sorted(v)[len(v) // 2]


def _time(fn, args):
    for _ in range(args.burst):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.burst):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / args.burst)
    return _median(us), min(us)


def kernel_stage(args, log, dev):
    from video_vae_amd import ops
    from video_vae_amd.entropy import capacity, encode_reference, gather_streams, normalise_counts
    from video_vae_amd.quant import code_counts, entropy_bits, qmax_of
    qmax = qmax_of(args.bits)
    cap = capacity(HW * LD)
    for frames in (16, 64) + ((1024,) if args.context else ()):    # 1024: four frames per CU, where the LDS a wave holds decides how many run
        rng = np.random.default_rng(frames)
        codes = np.clip(np.rint(rng.laplace(size=(frames, HW, LD)) * qmax / 6.0), -qmax, qmax).astype(np.int8)
        counts = code_counts(codes)
        freq = torch.from_numpy(normalise_counts(counts, args.bits)).to(dev)
        cd, keep = torch.from_numpy(codes).to(dev), torch.ones(frames, device=dev)
        out = ops.rans_encode(cd, keep, freq, args.bits)
        want = encode_reference(codes[:2], freq.cpu().numpy(), args.bits)
        got = gather_streams(out.words[:2], out.n_words[:2], out.state[:2])
        assert all(np.array_equal(a, e) for a, e in zip(got, want)), "the kernel's stream is not the definition's"
        offsets = torch.arange(frames, device=dev, dtype=torch.int64) * cap + cap - out.n_words.to(torch.int64)
        back, ok = ops.rans_decode(out.words, offsets, out.n_words, out.state, freq, args.bits, HW, LD)
        assert torch.equal(back, cd) and bool((ok == 1).all()), "the decoded codes are not the coded ones"
        enc = _time(lambda: ops.rans_encode(cd, keep, freq, args.bits, out=out), args)
        dec = _time(lambda: ops.rans_decode(out.words, offsets, out.n_words, out.state, freq, args.bits, HW, LD), args)
        words = int(out.n_words.sum())
        log(f"  {frames:3d} frames of {HW}x{LD} at {args.bits} bits ({entropy_bits(counts):.3f} bits per code, {words / frames:.0f} words per frame): "
            f"rans_encode median {enc[0]:7.2f} us best {enc[1]:7.2f} us, rans_decode median {dec[0]:7.2f} us best {dec[1]:7.2f} us per launch "
            f"({args.burst} per burst, {args.repeats} bursts; decode includes its two output allocations)")
        if args.context:
            context_kernels(args, log, dev, codes, cd, keep, enc[0], dec[0])


def context_kernels(args, log, dev, codes, cd, keep, static_enc, static_dec):
    """The context coder's kernels on the codes of ``kernel_stage``, checked against the definition on two frames, against the static
    kernels' medians of the same run."""
    from video_vae_amd import ops
    from video_vae_amd.entropy import (capacity, context_counts, context_thresholds, encode_context_reference, gather_streams,
                                       normalise_context_counts, token_energy)
    frames, cap = codes.shape[0], capacity(HW * LD)
    thr = context_thresholds(token_energy(codes), GRID_W)
    counts = ops.rans_context_counts(cd, keep, args.bits, GRID_W, thr)
    assert np.array_equal(counts[:2].cpu().numpy(), context_counts(codes[:2], GRID_W, thr)), "the kernel's counts are not the definition's"
    freq4 = normalise_context_counts(counts.sum(dim=0).cpu().numpy(), args.bits)
    tables = torch.from_numpy(freq4).to(dev)
    out = ops.rans_encode_context(cd, keep, tables, args.bits, GRID_W, thr)
    want = encode_context_reference(codes[:2], freq4, args.bits, GRID_W, np.array(thr))
    got = gather_streams(out.words[:2], out.n_words[:2], out.state[:2])
    assert all(np.array_equal(a, e) for a, e in zip(got, want)), "the kernel's stream is not the definition's"
    offsets = torch.arange(frames, device=dev, dtype=torch.int64) * cap + cap - out.n_words.to(torch.int64)
    decode = lambda form: ops.rans_decode_context(out.words, offsets, out.n_words, out.state, tables, args.bits, HW, LD, GRID_W, thr,
                                                  slot_form=form)
    for form in ("compact", "full", None):
        back, ok = decode(form)
        assert torch.equal(back, cd) and bool((ok == 1).all()), "the decoded codes are not the coded ones"
    cnt = _time(lambda: ops.rans_context_counts(cd, keep, args.bits, GRID_W, thr), args)
    enc = _time(lambda: ops.rans_encode_context(cd, keep, tables, args.bits, GRID_W, thr, out=out), args)
    dec = {form: _time(lambda: decode(form), args) for form in ("compact", "full", None)}
    log(f"      context coder, {GRID_W} tokens wide, thresholds {thr}, {int(out.n_words.sum()) / frames:.0f} words per frame: "
        f"rans_context_counts median {cnt[0]:7.2f} us best {cnt[1]:7.2f} us (includes its output allocation), "
        f"rans_encode_ctx median {enc[0]:7.2f} us best {enc[1]:7.2f} us ({enc[0] / static_enc:.3f} x rans_encode), "
        f"rans_decode_ctx compact median {dec['compact'][0]:7.2f} us best {dec['compact'][1]:7.2f} us ({dec['compact'][0] / static_dec:.3f} x "
        f"rans_decode), full median {dec['full'][0]:7.2f} us best {dec['full'][1]:7.2f} us ({dec['full'][0] / static_dec:.3f} x rans_decode), "
        f"the library's pick median {dec[None][0]:7.2f} us")


def temporal_stage(args, log, dev):
    """The temporal coder's kernels against the static and the context kernels on the same codes, every result checked first."""
    from video_vae_amd import ops
    from video_vae_amd.entropy import (capacity, chain_flags, chain_prev, chain_starts, context_thresholds, encode_temporal_reference,
                                       gather_streams, normalise_context_counts, normalise_counts, normalise_temporal_counts,
                                       temporal_thresholds_of_counts)
    from video_vae_amd.quant import qmax_of
    qmax, cap, period, rho = qmax_of(args.bits), capacity(HW * LD), 16, 0.9
    for chains in (1, 16, 64, 256):
        frames = chains * period
        g = torch.Generator(device=dev).manual_seed(chains)
        x = torch.empty((chains, period, HW, LD), device=dev)
        for t in range(period):                            # AR(1) in time, Laplacian innovations: the codes' spread is rans_encode's
            u = torch.rand((chains, HW, LD), device=dev, generator=g) - 0.5
            noise = -torch.sign(u) * torch.log1p(-2.0 * u.abs())
            x[:, t] = noise if t == 0 else rho * x[:, t - 1] + (1.0 - rho * rho) ** 0.5 * noise
        cd = torch.clamp(torch.round(x * qmax / 6.0), -qmax, qmax).to(torch.int8).reshape(frames, HW, LD).contiguous()
        keep = torch.ones(frames, device=dev)
        chain = chain_flags(np.ones((chains, period)), period)
        prev = torch.from_numpy(chain_prev(np.ones(frames), chain)).to(dev)
        start = torch.from_numpy(chain_starts(chain)).to(dev)
        hist = torch.stack([torch.bincount(c.reshape(-1).to(torch.int64) + 128, minlength=256) for c in cd]).cpu().numpy()
        thr = temporal_thresholds_of_counts(hist, chain)
        freq = torch.from_numpy(normalise_counts(hist, args.bits)).to(dev)
        counts = ops.rans_temporal_counts(cd, keep, prev, args.bits, thr)
        freq9 = normalise_temporal_counts(counts.sum(dim=0).cpu().numpy(), args.bits)
        tables = torch.from_numpy(freq9).to(dev)
        out = ops.rans_encode_temporal(cd, keep, prev, tables, args.bits, thr)
        want = encode_temporal_reference(cd[:3].cpu().numpy(), freq9, args.bits, chain[:3], thr)
        got = gather_streams(out.words[:3], out.n_words[:3], out.state[:3])
        assert all(np.array_equal(a, e) for a, e in zip(got, want)), "the kernel's stream is not the definition's"
        offsets = torch.arange(frames, device=dev, dtype=torch.int64) * cap + cap - out.n_words.to(torch.int64)
        decode = lambda: ops.rans_decode_temporal(out.words, offsets, out.n_words, out.state, tables, args.bits, HW, LD, start, thr)
        back, ok = decode()
        assert torch.equal(back, cd) and bool((ok == 1).all()), "the decoded codes are not the coded ones"
        static = ops.rans_encode(cd, keep, freq, args.bits)
        soffs = torch.arange(frames, device=dev, dtype=torch.int64) * cap + cap - static.n_words.to(torch.int64)
        cthr = context_thresholds(cd.abs().sum(-1).cpu().numpy(), GRID_W)
        tables4 = torch.from_numpy(normalise_context_counts(ops.rans_context_counts(cd, keep, args.bits, GRID_W, cthr).sum(dim=0).cpu().numpy(),
                                                            args.bits)).to(dev)
        ctx = ops.rans_encode_context(cd, keep, tables4, args.bits, GRID_W, cthr)
        coffs = torch.arange(frames, device=dev, dtype=torch.int64) * cap + cap - ctx.n_words.to(torch.int64)
        t = {"counts": _time(lambda: ops.rans_temporal_counts(cd, keep, prev, args.bits, thr), args),
             "counts_ctx": _time(lambda: ops.rans_context_counts(cd, keep, args.bits, GRID_W, cthr), args),
             "enc": _time(lambda: ops.rans_encode_temporal(cd, keep, prev, tables, args.bits, thr, out=out), args),
             "enc_static": _time(lambda: ops.rans_encode(cd, keep, freq, args.bits, out=static), args),
             "enc_ctx": _time(lambda: ops.rans_encode_context(cd, keep, tables4, args.bits, GRID_W, cthr, out=ctx), args),
             "dec": _time(decode, args),
             "dec_static": _time(lambda: ops.rans_decode(static.words, soffs, static.n_words, static.state, freq, args.bits, HW, LD), args),
             "dec_ctx": _time(lambda: ops.rans_decode_context(ctx.words, coffs, ctx.n_words, ctx.state, tables4, args.bits, HW, LD, GRID_W, cthr),
                              args)}
        m = {k: v[0] for k, v in t.items()}
        log(f"  temporal coder, {chains:3d} chains of {period} frames ({frames} frames of {HW}x{LD} at {args.bits} bits, rho {rho}), thresholds "
            f"{thr.tolist()}, words per frame {int(out.n_words.sum()) / frames:.0f} against static {int(static.n_words.sum()) / frames:.0f} and "
            f"context {int(ctx.n_words.sum()) / frames:.0f}: rans_temporal_counts median {m['counts']:7.2f} us (rans_context_counts "
            f"{m['counts_ctx']:7.2f} us), rans_encode_temporal median {m['enc']:7.2f} us ({m['enc'] / m['enc_static']:.3f} x rans_encode "
            f"{m['enc_static']:7.2f} us, {m['enc'] / m['enc_ctx']:.3f} x rans_encode_ctx {m['enc_ctx']:7.2f} us), rans_decode_temporal median "
            f"{m['dec']:8.2f} us = {m['dec'] / period:7.2f} us per frame of a chain ({m['dec'] / period / m['dec_static']:.3f} x rans_decode "
            f"{m['dec_static']:7.2f} us, rans_decode_ctx {m['dec_ctx']:7.2f} us) per launch ({args.burst} per burst, {args.repeats} bursts)")


def file_stage(args, log, dev):
    from video_vae_amd import data as D
    from video_vae_amd import infer as I
    from video_vae_amd.entropy import coded_bits
    from video_vae_amd.quant import rate_dataset, rate_summary
    model = I.build_model("model", SIZE, args.small, args.model_path, dev)
    weights = I.InferenceWeights(model)
    ld = model.encoder.selection_layer1.kernel.shape[0]
    log(f"  files: {args.clips} clips of up to {args.clip_frames} frames at {SIZE}x{SIZE}, {'small' if args.small else 'full C3'} model "
        f"({'seeded random weights' if not args.model_path else args.model_path}), --frames {T} --batch {B}, {args.bits} bits")
    with tempfile.TemporaryDirectory() as tmp:
        D.write_synthetic_clips(os.path.join(tmp, "clips"), args.clips, args.clip_frames, 360, 480, seed=1)
        runner = I.GraphedInference(model, weights, B, T, "encode", want_log_variance=False, quant_bits=args.bits)
        rates, deflated, coded_file, context_file, temporal_file = [], 0, 0, 0, 0
        grid_w = SIZE // model.encoder.patch_embedding.patch_size
        for ci, path in enumerate(I._clip_paths(os.path.join(tmp, "clips"))):
            items = I.clip_windows(path, SIZE, T)
            means, sels, codes, steps, counts = [], [], [], [], []
            for grp, real in I._full_batches(items, B):
                lat, q = runner(I._window_batch(grp, dev), I._mask_batch(grp, dev))
                for i in range(real):
                    c = grp[i][2]
                    means.append(lat.mean[i, :c].float().cpu())
                    sels.append(lat.selection[i, :c].cpu())
                    codes.append(q.codes[i, :c].clone())
                    steps.append(q.step[i, :c].cpu())
                    counts.append(q.counts[i, :c].clone())
            sel, dcodes, dcounts = torch.cat(sels), torch.cat(codes), torch.cat(counts)
            quant = (dcodes.cpu(), torch.cat(steps), args.bits)
            entropy = I._entropy_code(dcodes, sel.to(dev), dcounts, args.bits)
            deflated += I.save_latents(os.path.join(tmp, f"q{ci}.npz"), I.pack_latents(torch.cat(means), sel, quant=quant))
            coded_file += I.save_latents(os.path.join(tmp, f"a{ci}.npz"), I.pack_latents(torch.cat(means), sel, quant=quant, entropy=entropy))
            context = None
            if args.context:
                context = I._entropy_code(dcodes, sel.to(dev), dcounts, args.bits, grid_w)
                context_file += I.save_latents(os.path.join(tmp, f"c{ci}.npz"), I.pack_latents(torch.cat(means), sel, quant=quant, entropy=context))
            temporal = None
            if args.temporal:
                temporal = I._entropy_code(dcodes, sel.to(dev), dcounts, args.bits, period=16)
                temporal_file += I.save_latents(os.path.join(tmp, f"t{ci}.npz"), I.pack_latents(torch.cat(means), sel, quant=quant, entropy=temporal))
            rates.append(rate_summary(dcounts.cpu().numpy(), sel.numpy(), sel.shape[0], SIZE, SIZE, ld, args.bits, coded=coded_bits(*entropy),
                                      coded_context=None if context is None else coded_bits(*context[:2]),
                                      coded_temporal=None if temporal is None else coded_bits(*temporal[:2])))
        d = rate_dataset(rates)
        log(f"  kept {d['kept']} frames, {d['codes']} codes: bpp_file deflate {8.0 * deflated / d['pixels']:.4f}, bpp_file range-coded "
            f"{8.0 * coded_file / d['pixels']:.4f}; bpp_coded {d['bpp_coded']:.4f} against bpp_entropy {d['bpp_entropy']:.4f} "
            f"(bits_coded - bits_side = {(d['bits_coded'] - d['bits_side']) / max(d['bits_entropy'], 1e-9):.4f} x bits_entropy), bpp_raw {d['bpp_raw']:.4f}")
        if args.context:
            log(f"      context coder, {grid_w} tokens wide: bpp_file {8.0 * context_file / d['pixels']:.4f}; bpp_coded_context "
                f"{d['bpp_coded_context']:.4f} = {d['bits_coded_context'] / d['bits_coded']:.4f} x bpp_coded (random weights: the rate on a "
                "trained model is not measured)")
        if args.temporal:
            log(f"      temporal coder, chains of up to 16 frames: bpp_file {8.0 * temporal_file / d['pixels']:.4f}; bpp_coded_temporal "
                f"{d['bpp_coded_temporal']:.4f} = {d['bits_coded_temporal'] / d['bits_coded']:.4f} x bpp_coded (synthetic clips through random "
                "weights: the rate on a trained model is not measured)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--clip-frames", dest="clip_frames", type=int, default=48)
    ap.add_argument("--bits", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--model_path", default=None)
    ap.add_argument("--small", action="store_true", help="the depth-1 model (a quick check of the tool)")
    ap.add_argument("--context", action="store_true", help="also the context coder: its kernels beside the static ones, its files and sizes")
    ap.add_argument("--temporal", action="store_true", help="also the temporal coder: its kernels beside the others, its files and sizes")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("entropy_bench needs a GPU")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    log(f"entropy_bench: interleaved rANS, one wavefront per frame (csrc/rans.hip), {torch.cuda.get_device_name(0)}")
    kernel_stage(args, log, dev)
    if args.temporal:
        temporal_stage(args, log, dev)
    file_stage(args, log, dev)
    if args.out:
        if os.path.dirname(args.out):
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
