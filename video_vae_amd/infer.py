"""Inference: encode clips to latents and decode latents back to frames, as replayed hipGraphs, without an optimizer.

  * ``InferenceWeights(model)``: the bf16 weight shadows the forward reads (``p.bf16`` for every fp32 parameter, ``p.bf16_t`` for the Linear
    kernels marked ``want_t``), so that a model loaded without an ``optim.Optimizer`` runs the same kernels and product routes as the
    train step's forward.  ``refresh()`` re-derives them in place after the parameters were written: a graph captured earlier replays
    the new weights.
  * ``GraphedInference(model, weights, batch, frames, mode)``: one forward-only hipGraph per (mode, batch, frames); ``mode`` is "encode",
    "decode" or "reconstruct" (VideoVAE.encode / decode / reconstruct), or "evaluate" (reconstruct and metrics.frame_metrics in one graph).
    Captured on a private stream, replayed on the caller's current stream; the inputs are copied into static buffers, and the OUTPUTS ARE
    STATIC TENSORS that the next replay overwrites (clone what you keep).
  * ``python -m video_vae_amd.infer encode|decode|eval|scenes|compare ...``: a folder of clips to one latent ``.npz`` per clip (latents.py) and
    back to frames; PSNR / SSIM / MSE of the reconstructions and the kept-frame fraction as one JSON file; the scene cuts of every clip
    as one JSON file; ``compare`` scores one folder of clips against another with the plane-wise Y'CbCr metrics (plane_metrics.py), no
    model.  Each command's ``--help`` says what its flags do.  A clip runs in one of three modes: plain (the centre square at
    ``--size``, hard windows of ``--frames`` through one ``GraphedInference``), ``--tile`` (its own resolution, tiling.TiledInference)
    and ``--temporal-overlap`` / ``--scene-cuts`` (overlapping windows per scene, tiled or not, tiling.ClipInference); each mode has
    its own latent-file format, which ``decode`` recognises.
"""
import argparse
import gc
import json
import math
import os
import sys

import numpy as np
import torch

from . import data as D
from . import ops
from .graph import graph_node_census
from .metrics import MS_SSIM_WEIGHTS, frame_metrics, ms_ssim, ms_ssim_check, temporal_mse, temporal_summary, temporal_summary_scenes
from .entropy import CONTEXTS, M as RANS_SCALE, TEMPORAL_TABLES, TemporalModel, chain_flags, chain_prev, chain_starts, coded_bits, \
    context_thresholds, gather_streams, normalise_context_counts, normalise_counts, normalise_temporal_counts, table_size, \
    temporal_thresholds_of_counts
from .latents import (coded_members, pack_latents, pack_latents_tiled, pack_latents_windows, save_latents, unpack_latents,
                      unpack_latents_tiled, unpack_latents_windows)
from .quant import qmax_of, rate_dataset, rate_summary
from .scenes import scene_ranges
from . import plane_metrics as PM
from .rngs import Rngs

MODES = ("encode", "decode", "reconstruct", "evaluate")


class InferenceWeights:
    """The bf16 shadows of a model's fp32 parameters for a forward without an optimizer (no Adam state, no flat fp32 buffer).

    Every shadow slot is padded to 8 bf16 elements, so each ``p.bf16`` is 16-byte aligned (what the own GEMMs take).  When the parameters
    already carry an optimizer's shadows those are used and nothing is allocated."""

    def __init__(self, model):
        self.params = [p for p in model.parameters() if p.dtype == torch.float32]
        if not self.params or not all(p.is_cuda for p in self.params):
            raise ValueError("InferenceWeights needs a model whose fp32 parameters live on a GPU")
        dev = self.params[0].device
        self.shared = all(getattr(p, "bf16", None) is not None for p in self.params)
        self.shadow = self.tbuf = None
        if not self.shared:
            offsets, off = [], 0
            for p in self.params:
                offsets.append(off)
                off += (p.numel() + 7) // 8 * 8
            self.shadow = torch.empty(off, dtype=torch.bfloat16, device=dev)
            for p, o in zip(self.params, offsets):
                p.bf16 = self.shadow[o:o + p.numel()].view(p.shape)
            self.tbuf, _ = ops.transposed_shadows(self.params, dev)
        self.tpairs = [(p.bf16, p.bf16_t) for p in self.params if getattr(p, "bf16_t", None) is not None]
        self.refresh()

    @torch.no_grad()
    def refresh(self):
        """Re-derive every shadow from its fp32 parameter, in place (the addresses a captured graph reads stay the same)."""
        torch._foreach_copy_([p.bf16 for p in self.params], [p.detach() for p in self.params])
        ops.transpose_grouped(self.tpairs)


class GraphedInference:
    """One replayed forward-only hipGraph of ``model.encode`` / ``decode`` / ``reconstruct`` (or "evaluate") at a fixed (batch, frames).

    ``__call__(inputs, mask, noise=None)``: ``inputs`` = video (batch, frames, H, W, C) for "encode" / "reconstruct" / "evaluate", the
    compressed representation (batch, frames, hw, ld) for "decode"; ``mask`` (batch, frames).  Returns the static output of the capture
    (``Latents`` for "encode", ``(reconstruction, metrics.FrameMetrics, selection)`` for "evaluate", the reconstruction otherwise): the
    next replay overwrites it.  "evaluate" runs exactly reconstruct's launches, then the metrics of the reconstruction against the input video.
    rl flavour with ``rngs``: the Bernoulli uniforms are static buffers refilled before each replay from a device generator seeded from
    ``rngs.seed`` (``noise={"bernoulli_u": u}`` hands explicit ones over); without ``rngs`` the gate is the deterministic threshold.
    ``with_selection``: "reconstruct" returns ``(reconstruction, selection)`` from exactly reconstruct's launches (tiling.TiledInference).
    ``quant_bits`` (2 .. 8; "evaluate" and "encode" only): the latent quantiser (ops.latent_quantise) runs inside the captured graph on
    the frames selection * mask keeps.  "evaluate": in place on the compressed representation between encode and decode, and the call
    returns ``(reconstruction, FrameMetrics, selection, counts)`` (``self.quantised`` keeps the QuantisedLatents, static like the outputs);
    "encode": on the means, and the call returns ``(Latents, quant.QuantisedLatents)``.  With ``None`` the captured graph and what is returned are exactly those described above."""

    def __init__(self, model, weights, batch, frames, mode, rngs=None, want_log_variance=True, warmup=2, frame_shape=None,
                 with_selection=False, quant_bits=None):
        if mode not in MODES:
            raise ValueError(f"mode {mode!r}: one of {MODES}")
        if quant_bits is not None:
            if mode not in ("encode", "evaluate"):
                raise ValueError(f"quant_bits with mode {mode!r}: the quantiser runs in \"encode\" and \"evaluate\" graphs only")
            qmax_of(quant_bits)
        self.quant_bits = None if quant_bits is None else int(quant_bits)
        self.model, self.weights, self.mode = model, weights, mode
        self.want_log_variance = bool(want_log_variance)
        self.with_selection = bool(with_selection)
        enc = model.encoder
        dev = model.fill_token.device
        p = enc.patch_embedding.patch_size
        hw, ld = enc.selection_layer2.kernel.shape[0], enc.selection_layer1.kernel.shape[0]
        if frame_shape is None:
            side = math.isqrt(hw) * p
            frame_shape = (side, side, enc.last_dim // (p * p))
        self.mask = torch.ones((batch, frames), dtype=torch.float32, device=dev)
        if mode == "decode":
            self.input = torch.zeros((batch, frames, hw, ld), dtype=model.decoder.dtype, device=dev)
        else:
            self.input = torch.zeros((batch, frames) + tuple(frame_shape), dtype=torch.float32, device=dev)
        # the draws go through a private Rngs: the caller's keeps its own stream and no injected buffers
        self.rngs = Rngs(rngs.seed) if (rngs is not None and mode != "decode" and enc.flavour == "rl") else None
        self.noise = {}
        self._capture(warmup, rngs.seed if rngs is not None else 0)

    def _run(self):
        m = self.model
        if self.mode == "encode":
            lat = m.encode(self.input, self.mask, self.rngs, self.want_log_variance)
            if self.quant_bits is None:
                return lat
            return lat, ops.latent_quantise(lat.mean.contiguous(), lat.selection * self.mask, self.quant_bits)
        if self.mode == "decode":
            return m.decode(self.input, self.mask)
        if self.mode == "evaluate":
            lat = m.encode(self.input, self.mask, self.rngs, want_log_variance=False)
            if self.quant_bits is None:
                recon = m.decode(lat.compressed_representation, self.mask)
                return recon, frame_metrics(self.input, recon, self.mask), lat.selection
            comp = lat.compressed_representation
            if not comp.is_contiguous():
                raise RuntimeError("the compressed representation is not contiguous: the quantiser cannot write it in place")
            q = ops.latent_quantise(comp, lat.selection * self.mask, self.quant_bits, dequantise_in_place=True)
            self.quantised = q                        # static like the outputs: eval --entropy-code codes q.codes
            recon = m.decode(comp, self.mask)
            return recon, frame_metrics(self.input, recon, self.mask), lat.selection, q.counts
        if self.with_selection:                       # VideoVAE.reconstruct, keeping the selection
            lat = m.encode(self.input, self.mask, self.rngs, want_log_variance=False)
            return m.decode(lat.compressed_representation, self.mask), lat.selection
        return m.reconstruct(self.input, self.mask, self.rngs)

    def _refill(self):
        for kind, buf in self.noise.values():
            buf.normal_(generator=self.gen) if kind == "normal" else buf.uniform_(generator=self.gen)

    def _capture(self, warmup, seed):
        self.stream = torch.cuda.Stream()
        self.stream.wait_stream(torch.cuda.current_stream())
        self.gen = torch.Generator(device=self.input.device)
        self.gen.manual_seed((0x9E3779B97F4A7C15 * (seed + 1)) & 0x7FFFFFFFFFFFFFFF)
        with torch.cuda.stream(self.stream):
            if self.rngs is not None:                 # discover the draws and pin them to static buffers
                self.rngs.recording = {}
                self._run()
                for name, (kind, shape, dtype) in self.rngs.recording.items():
                    buf = torch.empty(shape, dtype=dtype, device=self.input.device)
                    self.noise[name] = (kind, buf)
                    self.rngs.inject(name, buf)
                self.rngs.recording = None
            for _ in range(warmup):                   # allocator, library heuristics, one-time kernel attributes
                self._refill()
                self._run()
            self._refill()
        torch.cuda.synchronize()
        gc.collect()
        try:
            g = torch.cuda.CUDAGraph(keep_graph=True)        # keeps the hipGraph_t: its nodes are counted below
        except TypeError:
            g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=self.stream):
            self.out = self._run()
        self.census = graph_node_census(g)
        if self.census and self.census.get("memset", 0):
            raise RuntimeError(f"the captured {self.mode} graph holds {self.census['memset']} hipGraph memset node(s) ({self.census}): on ROCm 7.2 "
                               "a replayed memset node writes garbage (DESIGN.md section 3).  Replace the op that issued hipMemsetAsync.")
        self.graph = g

    def __call__(self, inputs=None, mask=None, noise=None):
        if inputs is not None:
            self.input.copy_(inputs)
        if mask is not None:
            self.mask.copy_(mask.reshape(self.mask.shape))
        if noise is None:
            self._refill()
        else:
            if set(noise) != set(self.noise):
                raise KeyError(f"noise for {sorted(noise)} given, the captured graph draws {sorted(self.noise)}")
            for name, t in noise.items():
                self.noise[name][1].copy_(t.reshape(self.noise[name][1].shape))
        self.graph.replay()
        return self.out


# ------------------------------------------------------------------------------------------------ command line
def model_config(size, small):
    """The driver's model (train.py): patch 16, depth 9 / 12; ``small`` = depth 1 (smoke runs)."""
    cfg = dict(height=size, width=size, channels=3, patch_size=16, encoder_depth=9, decoder_depth=12, mlp_dim=1536, num_heads=8,
               qkv_features=512, max_temporal_len=64, spatial_compression_rate=8, unembedding_upsample_rate=4)
    if small:
        cfg.update(encoder_depth=1, decoder_depth=1, mlp_dim=256, qkv_features=128, num_heads=4)
    return cfg


def build_model(flavour, size, small, model_path, dev, ema=False):
    """``ema``: after the normal load, overwrite the parameters with the checkpoint's weight average (model_loader.load_ema_weights) --
    before any InferenceWeights is derived from them."""
    import video_vae_amd as V
    from . import rl_model
    from .model_loader import load_checkpoint, load_ema_weights
    cls = rl_model.VideoVAE if flavour == "rl" else V.VideoVAE
    model = cls(rngs=V.Rngs(2), **model_config(size, small)).to(dev)
    if model_path:
        load_checkpoint(model, None, model_path)
    if ema:
        if not model_path:
            raise ValueError("--ema needs a checkpoint: the weight average is part of its optimizer state")
        load_ema_weights(model, model_path)
    return model


def _setup(args, flavour=None):
    """(device, model, InferenceWeights, rngs) of a command: the model of ``args`` (of ``flavour`` when given) with the checkpoint's
    weights, and the Rngs of the Bernoulli gate, None where the gate is the threshold (--threshold, the "model" flavour)."""
    dev = torch.device("cuda", 0)
    flavour = flavour or args.flavour
    model = build_model(flavour, args.size, args.small, args.model_path, dev, ema=args.ema)
    rngs = None if flavour == "model" or args.threshold else Rngs(args.seed)
    return dev, model, InferenceWeights(model), rngs


def centre_square(frames, size):
    """uint8 (T, H, W, 3) -> (T, size, size, 3): the centred square crop of side min(H, W), resized (bilinear, half-pixel centres)."""
    h, w = frames.shape[1:3]
    s = min(h, w)
    top, left = (h - s) // 2, (w - s) // 2
    return D._resize_u8(np.ascontiguousarray(frames[:, top:top + s, left:left + s]), size, size)


def windows(n_frames, frames):
    """[(start, count)] of the consecutive windows of ``frames`` frames covering a clip; the last one may be short (zero-padded, masked)."""
    return [(s, min(frames, n_frames - s)) for s in range(0, max(n_frames, 1), frames)]


def _batches(items, batch):
    """(group, number of items) for groups of ``batch`` items; the last group may be short (``_full_batches`` fills it up)."""
    for i in range(0, len(items), batch):
        grp = items[i:i + batch]
        yield grp, len(grp)


def _full_batches(items, batch):
    """``_batches`` with a short last group filled up with copies of its last item (a replay has a fixed batch): (group of ``batch``
    items, number of real ones); the caller drops the outputs of the copies."""
    for grp, real in _batches(items, batch):
        yield grp + [grp[-1]] * (batch - real), real


def _stem(path):
    return os.path.splitext(os.path.basename(path))[0]


def _y4m_read(args):
    """The command's --y4m-matrix / --y4m-range as data.open_y4m takes them: how a .y4m clip's planes become RGB."""
    return {"matrix": getattr(args, "y4m_matrix", "bt601"), "range": getattr(args, "y4m_range", "header")}


def _read_raw(path, y4m=None):
    """A clip on disk as it is: uint8 (T, H, W, 3), every frame, at its own resolution (a .y4m clip converted on the host)."""
    clip, _ = D._read_frames(path, 0, 1 << 30, y4m)
    return np.asarray(clip)


def _open_raw(path, y4m=None):
    """``_read_raw`` for a clip that goes to the device as it is: a .y4m clip stays a y4m.Y4MClip (nothing read or converted yet), which
    data.upload_rgb / data.upload_centre_square upload as planes and convert there -- the bytes of ``_read_raw``."""
    return D.open_y4m(path, y4m) if path.endswith(D.Y4M_EXT) else _read_raw(path)


def _pad_window(x, frames, fill=0, axis=0):
    """``x`` (a numpy array, or a tensor on any device) with c <= ``frames`` frames along ``axis`` -> (x padded along that axis to
    ``frames`` with ``fill`` (a scalar, or an array that broadcasts), of x's kind; mask fp32 numpy (frames,): 1 on the c real frames)."""
    c = x.shape[axis]
    shape = tuple(x.shape[:axis]) + (frames,) + tuple(x.shape[axis + 1:])
    out = x.new_empty(shape) if torch.is_tensor(x) else np.empty(shape, dtype=x.dtype)
    out[...] = fill
    out[(slice(None),) * axis + (slice(0, c),)] = x
    return out, (np.arange(frames) < c).astype(np.float32)


def clip_windows(path, size, frames, device=None, y4m=None):
    """A clip on disk -> [(uint8 (frames, size, size, 3), mask fp32 (frames,), real frame count)]: its centre-square frames cut into
    ``windows``, the last one zero-padded and masked.  ``device`` (--device-resize): the clip is cropped and resized there
    (data.upload_centre_square; a .y4m clip is converted to RGB there too) and the windows are uint8 tensors on it, never copied back.
    ``y4m``: a .y4m clip's matrix and range (``_y4m_read``)."""
    if device is None:
        clip = centre_square(_read_raw(path, y4m), size)
    else:
        clip = D.upload_centre_square(_open_raw(path, y4m), size, device)
    return [_pad_window(clip[s:s + c], frames) + (c,) for s, c in windows(clip.shape[0], frames)]


def clip_windows_native(path, frames, y4m=None):
    """A clip on disk at its own resolution, no crop, no resize -> (uint8 (n_windows, frames, H, W, 3), mask fp32 (n_windows, frames),
    [real frame count per window]): its ``windows``, the last one zero-padded and masked."""
    clip = _read_raw(path, y4m)
    wins = windows(clip.shape[0], frames)
    video, mask = _pad_window(clip, len(wins) * frames)               # the windows are consecutive: only the last one is padded
    return video.reshape((len(wins), frames) + clip.shape[1:]), mask.reshape(len(wins), frames), [c for _, c in wins]


def _clip_paths(data):
    paths = D.list_video_files(data)
    if not paths:
        raise SystemExit(f"no clips (.npy / .npz / .y4m) under {data}")
    return paths


def _tiled_runner(runner, model, weights, args, grid, mode, rngs, want_log_variance=False):
    """The TiledInference of the command (captured on first use), on ``grid``."""
    from .tiling import TiledInference
    if runner is None:
        return TiledInference(model, weights, grid, args.batch, args.frames, mode, rngs=rngs, want_log_variance=want_log_variance)
    return runner.with_grid(grid)


def _quantise_means(mean, selection, mask, bits):
    """quant.QuantisedLatents of a tiled or windowed runner's means (N, ny nx, T, hw, ld) on the GPU (ops.latent_quantise: the quantiser
    is per frame, so running it on the collected means equals running it window by window); a frame is kept where selection (N, ny nx, T)
    and mask (N, T) both are nonzero."""
    return ops.latent_quantise(mean.contiguous(), (selection * mask.reshape(mask.shape[0], 1, -1)).contiguous(), bits)


def _context_grid(args, model):
    """--entropy-context: the token columns of a frame (or tile) as the encoder lays its tokens out; None without the flag."""
    return args.size // model.encoder.patch_embedding.patch_size if getattr(args, "entropy_context", False) else None


def _entropy_period(args):
    """--entropy-temporal: the most frames of a chain (--entropy-period); None without the flag."""
    return args.entropy_period if getattr(args, "entropy_temporal", False) else None


def _entropy_code(codes, keep, counts, bits, grid_w=None, period=None):
    """Range-code a clip's quantised frames (entropy.py, ops.rans_encode): ``codes`` int8 (..., hw, ld) on the GPU, dense, in the order
    the latent file stores its frames; ``keep`` (...) nonzero on the frames the file keeps; ``counts`` (..., 256) the quantiser's histograms
    of those frames (zeros on the others).  One table for the clip, normalised on the host from the summed counts (a clip without a kept
    frame: the one-symbol table of code 0) -> (entropy.CodedFrames of the kept frames on the host, freq).
    ``grid_w`` (--entropy-context): the context coder instead.  The kept frames' token energies (torch) give the clip's thresholds on the
    host, ops.rans_context_counts the histograms per context, the host their four tables, ops.rans_encode_context the stream
    -> (CodedFrames, freq4, (grid_w, thr0, thr1)), what the packers take.
    ``period`` (--entropy-temporal): the temporal coder instead.  The last axis of ``keep`` is time and every index of its leading axes a
    sequence of its own (entropy.chain_flags); the quantiser's counts of the kept frames give the clip's thresholds on the host,
    ops.rans_temporal_counts the histograms per table row, the host their nine tables, ops.rans_encode_temporal the stream
    -> (CodedFrames, freq9, entropy.TemporalModel(thr, chain))."""
    hw, ld = codes.shape[-2:]
    flags = (keep.reshape(-1) != 0).float()
    codes = codes.reshape(-1, hw, ld).contiguous()
    one_symbol = np.zeros(table_size(bits), dtype=np.uint16)
    one_symbol[qmax_of(bits)] = RANS_SCALE
    if period is not None:
        if not ops.rans_temporal_supported(hw, ld, bits):
            raise SystemExit(f"--entropy-temporal: frames of {hw} tokens x {ld} channels are outside what the coder takes")
        chain = chain_flags(keep, period)
        prev = chain_prev(keep, chain)
        thr = temporal_thresholds_of_counts(counts.reshape(-1, 256)[flags != 0].cpu().numpy(), chain)
        by_row = ops.rans_temporal_counts(codes, flags, prev, bits, thr).sum(dim=0).cpu().numpy().astype(np.int64)
        freq9 = normalise_temporal_counts(by_row, bits) if by_row.sum() else np.stack([one_symbol] * TEMPORAL_TABLES)
        coded = ops.rans_encode_temporal(codes, flags, prev, freq9, bits, thr)
        return gather_streams(coded.words, coded.n_words, coded.state, keep=flags), freq9, TemporalModel(thr, chain)
    if grid_w is not None:
        if not ops.rans_context_supported(hw, ld, bits, grid_w):
            raise SystemExit(f"--entropy-context: frames of {hw} tokens x {ld} channels, {grid_w} tokens wide, are outside what the context "
                             "coder takes (at most 4096 tokens, (grid_w - 1) ld >= 63); run without it")
        thr = context_thresholds(codes.abs().sum(-1)[flags != 0].cpu().numpy(), grid_w)
        by_context = ops.rans_context_counts(codes, flags, bits, grid_w, thr).sum(dim=0).cpu().numpy().astype(np.int64)
        freq4 = normalise_context_counts(by_context, bits) if by_context.sum() else np.stack([one_symbol] * CONTEXTS)
        coded = ops.rans_encode_context(codes, flags, freq4, bits, grid_w, thr)
        return gather_streams(coded.words, coded.n_words, coded.state, keep=flags), freq4, (grid_w,) + thr
    pooled = counts.reshape(-1, 256).sum(dim=0).cpu().numpy().astype(np.int64)
    freq = normalise_counts(pooled, bits) if pooled.sum() else one_symbol
    coded = ops.rans_encode(codes, flags, freq, bits)
    return gather_streams(coded.words, coded.n_words, coded.state, keep=flags), freq


def _entropy_decode(arrays, dev, name):
    """A latent file's arrays with ``mean_ans`` -> the arrays with ``mean_q`` in its place, decoded on the GPU (ops.rans_decode, for a
    file with ``ans_ctx`` ops.rans_decode_context, for one with ``ans_chain`` ops.rans_decode_temporal); a frame whose stream fails the
    end check raises ValueError naming the file and the frame (counted among its kept frames; in a chain, the first)."""
    coded, freq, bits, hw, ld, *context = coded_members(arrays)
    frames = coded.n_words.shape[0]
    codes = np.zeros((0, hw, ld), dtype=np.int8)
    if frames:
        offsets = np.concatenate([[0], np.cumsum(coded.n_words)[:-1]]).astype(np.int64)
        decode = ops.rans_decode_context if context else ops.rans_decode
        if context and isinstance(context[0], TemporalModel):
            decode, context = ops.rans_decode_temporal, (chain_starts(context[0].chain), context[0].thr)
        got, ok = decode(torch.from_numpy(coded.words).to(dev), torch.from_numpy(offsets).to(dev),
                         torch.from_numpy(coded.n_words.astype(np.int32)).to(dev), torch.from_numpy(coded.state).to(dev), freq, bits, hw, ld, *context)
        bad = np.nonzero(ok.cpu().numpy() == 0)[0]
        if bad.size:
            raise ValueError(f"{name}: the rANS stream of kept frame {int(bad[0])} is not valid (words left over or a lane not back at its start)")
        codes = got.cpu().numpy()
    out = {k: v for k, v in arrays.items() if k != "mean_ans" and not k.startswith("ans_")}
    out["mean_q"] = codes
    return out


def _rate_keys(args):
    """The keys of a rate summary that eval lifts beside the metrics."""
    return ("bpp_raw", "bpp_entropy", "bits_side") + (("bits_coded", "bpp_coded") if args.entropy_code else ()) + \
        (("bits_coded_context", "bpp_coded_context") if getattr(args, "entropy_context", False) else ()) + \
        (("bits_coded_temporal", "bpp_coded_temporal") if getattr(args, "entropy_temporal", False) else ())


def _rate_note(nbytes, n_frames, height, width):
    """', <bytes> bytes, bpp_file <8 bytes / pixels>' of a quantised latent file."""
    return f", {nbytes} bytes, bpp_file {8.0 * nbytes / (n_frames * height * width):.4f}"


def _write_latents(args, path, arrays, n_frames, height, width):
    """Write the latent file of the clip at ``path`` under --out: ``arrays`` and the model's ``size`` / ``small`` -> the rate note of
    the printed line ('' for a file that is not quantised)."""
    arrays.update(size=np.int64(args.size), small=np.int64(bool(args.small)))
    nbytes = save_latents(os.path.join(args.out, _stem(path) + ".npz"), arrays)
    return _rate_note(nbytes, n_frames, height, width) if "mean_q" in arrays or "mean_ans" in arrays else ""


def cmd_encode_tiled(args):
    """encode --tile: every clip at its own resolution, tiled (tiling.py); one .npz per clip (pack_latents_tiled)."""
    from .tiling import TileGrid
    dev, model, weights, rngs = _setup(args)
    runner = None
    os.makedirs(args.out, exist_ok=True)
    for path in _clip_paths(args.data):
        video, mask, counts = clip_windows_native(path, args.frames, _y4m_read(args))
        grid = TileGrid(video.shape[2], video.shape[3], args.size, args.overlap)
        runner = _tiled_runner(runner, model, weights, args, grid, "encode", rngs, args.with_logvar)
        out = runner(torch.from_numpy(video).to(dev), torch.from_numpy(mask).to(dev))
        dense = lambda x: torch.cat([x[:, i, :c] for i, c in enumerate(counts)], dim=1)                    # (ny nx, n_frames, ...)
        raw = lambda x: dense(x).cpu()
        keep = lambda x: raw(x.float())
        quant = entropy = None
        if args.quantise_bits is not None:
            q = _quantise_means(out.mean, out.selection, torch.from_numpy(mask).to(dev), args.quantise_bits)
            quant = (raw(q.codes.transpose(0, 1)), raw(q.step.transpose(0, 1)), args.quantise_bits)
            if args.entropy_code:
                entropy = _entropy_code(dense(q.codes.transpose(0, 1)), dense(out.selection.transpose(0, 1)), dense(q.counts.transpose(0, 1)),
                                        args.quantise_bits, _context_grid(args, model), _entropy_period(args))
        arrays = pack_latents_tiled(keep(out.mean.transpose(0, 1)), keep(out.selection.transpose(0, 1)), grid,
                                    keep(out.log_variance.transpose(0, 1)) if args.with_logvar else None, quant=quant, entropy=entropy)
        arrays["window"] = np.int64(args.frames)
        note = _write_latents(args, path, arrays, int(arrays["n_frames"]), grid.height, grid.width)
        print(f"{path}: {int(arrays['n_frames'])} frames of {grid.height}x{grid.width}, {grid.ny}x{grid.nx} tiles, "
              f"{int(arrays['selection'].sum())} tile frames kept{note}", flush=True)


def read_clip(path, size, tile, device=None, y4m=None):
    """A clip on disk -> uint8 (n, H, W, 3): at its own resolution (``tile``) or its centre square resized to size x size; with
    ``device`` (--device-resize, untiled) the square is cut and resized there and returned as a tensor on it (a .y4m clip is uploaded as
    planes and converted there).  ``y4m``: a .y4m clip's matrix and range (``_y4m_read``)."""
    if device is not None and not tile:
        return D.upload_centre_square(_open_raw(path, y4m), size, device)
    clip = _read_raw(path, y4m)
    return np.ascontiguousarray(clip) if tile else centre_square(clip, size)


def _window_batch(grp, dev):
    """The windows of a group (clip_windows items) as one fp32 (batch, frames, size, size, 3) video in [0, 1] on ``dev``."""
    if torch.is_tensor(grp[0][0]):
        return torch.stack([g[0] for g in grp]).float() / 255.0
    return torch.from_numpy(np.stack([g[0] for g in grp])).to(dev).float() / 255.0


def _mask_batch(grp, dev):
    """The masks of a group (the second entry of its items) as one fp32 (batch, frames) tensor on ``dev``."""
    return torch.from_numpy(np.stack([g[1] for g in grp])).to(dev)


def detect_cuts(u8, args):
    """The scene cuts of a uint8 RGB clip (L, H, W, 3) on the GPU with the command's --scene-* settings (scenes.scene_cuts)."""
    from .scenes import scene_cuts
    return scene_cuts(u8, args.scene_hist, args.scene_similarity, "gray" if args.scene_gray else "hsv")


def scene_config(args):
    return {"hist_size": args.scene_hist, "similarity": args.scene_similarity, "space": "gray" if args.scene_gray else "hsv"}


def read_clip_cuts(path, args, dev):
    """(read_clip of the command, that clip on the GPU, its scene cuts or None): with --scene-cuts the cuts are found on the clip as read
    from disk, at its own resolution, before any crop or resize (with --tile that upload is the clip the model runs).  --device-resize:
    the centre square is cut and resized on the GPU and the first entry is that device tensor too (its callers read its shape only);
    with --scene-cuts the one upload of the raw clip serves the histograms and the resize.  A .y4m clip's --scene-cuts upload is its
    planes, converted to RGB on the GPU (data.upload_rgb); the first entry is then the y4m.Y4MClip where only its shape is read."""
    device_resize = getattr(args, "device_resize", False)
    y4m = _y4m_read(args)
    if not args.scene_cuts:
        if device_resize:
            u8 = read_clip(path, args.size, args.tile, dev, y4m)
            return u8, u8, None
        clip = read_clip(path, args.size, args.tile, y4m=y4m)
        return clip, torch.from_numpy(clip).to(dev), None
    raw = _open_raw(path, y4m)
    u8 = D.upload_rgb(raw, dev)
    cuts = detect_cuts(u8, args)
    if args.tile:
        return raw, u8, cuts
    if device_resize:
        sq = D.device_centre_square(u8, args.size)
        return sq, sq, cuts
    clip = centre_square(raw[:], args.size)                   # a Y4MClip: converted on the host, the bytes of the upload
    return clip, torch.from_numpy(clip).to(dev), cuts


def _clip_grid(clip, args):
    """The TileGrid of a clip: its own tiles (--tile), else the 1 x 1 grid of the centre square."""
    from .tiling import TileGrid
    if args.tile:
        return TileGrid(clip.shape[1], clip.shape[2], args.size, args.overlap)
    return TileGrid(args.size, args.size, args.size, 0)


def _clip_runner(runner, model, weights, args, grid, mode, rngs, want_log_variance=False):
    """The ClipInference of the command (captured on first use), on ``grid``."""
    from .tiling import ClipInference
    if runner is None:
        return ClipInference(model, weights, grid, args.batch, args.frames, args.temporal_overlap, mode, rngs=rngs,
                             want_log_variance=want_log_variance)
    return runner.with_grid(grid)


def cmd_encode_windows(args):
    """encode --temporal-overlap: every clip in overlapping windows (tiled or the centre square); one .npz per clip (pack_latents_windows)."""
    dev, model, weights, rngs = _setup(args)
    runner = None
    os.makedirs(args.out, exist_ok=True)
    for path in _clip_paths(args.data):
        clip, u8, cuts = read_clip_cuts(path, args, dev)
        grid = _clip_grid(clip, args)
        runner = _clip_runner(runner, model, weights, args, grid, "encode", rngs, args.with_logvar)
        out = runner(u8, cuts=cuts)
        fw = min(args.frames, clip.shape[0])
        quant = entropy = None
        if args.quantise_bits is not None:
            real = torch.from_numpy(out.plan.mask()).to(dev)                                             # 0 on a short window's padding
            q = _quantise_means(out.mean, out.selection, real, args.quantise_bits)
            quant = (q.codes[:, :, :fw], q.step[:, :, :fw], args.quantise_bits)
            if args.entropy_code:                         # the frames the packer keeps: selected and not padding
                kept = (out.selection * real.reshape(real.shape[0], 1, -1))[:, :, :fw]
                entropy = _entropy_code(q.codes[:, :, :fw], kept, q.counts[:, :, :fw], args.quantise_bits, _context_grid(args, model),
                                        _entropy_period(args))
        arrays = pack_latents_windows(out.mean[:, :, :fw], out.selection[:, :, :fw], grid, out.plan,
                                      out.log_variance[:, :, :fw] if args.with_logvar else None, quant=quant, entropy=entropy)
        note = _write_latents(args, path, arrays, clip.shape[0], grid.height, grid.width)
        cut_note = "" if cuts is None else f"scene cuts {cuts}, "
        print(f"{path}: {clip.shape[0]} frames of {grid.height}x{grid.width}, {grid.ny}x{grid.nx} tiles, {cut_note}"
              f"windows at {out.plan.starts}, {int(arrays['selection'].sum())} tile frames kept{note}", flush=True)


def _write_json(path, out):
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)


def cmd_scenes(args):
    """The scene cuts of every clip under --data (scenes.scene_cuts on the GPU, the clip as read) -> one JSON file."""
    dev = torch.device("cuda", 0)
    clips = []
    for path in _clip_paths(args.data):
        raw = _open_raw(path, _y4m_read(args))                # a .y4m clip: uploaded as planes, converted on the GPU
        cuts = detect_cuts(D.upload_rgb(raw, dev), args)
        clips.append({"name": _stem(path), "path": path, "frames": int(raw.shape[0]), "height": int(raw.shape[1]),
                      "width": int(raw.shape[2]), "cuts": cuts, "scenes": scene_ranges(cuts, raw.shape[0])})
        print(f"{path}: {raw.shape[0]} frames, {len(cuts) + 1} scenes, cuts at {cuts}", flush=True)
    _write_json(args.out, {"config": dict(data=args.data, **scene_config(args)), "clips": clips})
    print(f"scenes: {len(clips)} clips, {sum(len(c['cuts']) for c in clips)} cuts -> {args.out}", flush=True)


def cmd_encode(args):
    if args.temporal_overlap is not None:
        return cmd_encode_windows(args)
    if args.tile:
        return cmd_encode_tiled(args)
    dev, model, weights, rngs = _setup(args)
    bits = args.quantise_bits
    runner = GraphedInference(model, weights, args.batch, args.frames, "encode", rngs=rngs, want_log_variance=args.with_logvar,
                              quant_bits=bits)
    os.makedirs(args.out, exist_ok=True)
    for path in _clip_paths(args.data):
        items = clip_windows(path, args.size, args.frames, dev if args.device_resize else None, _y4m_read(args))
        means, lvs, sels, codes, steps, dcodes, dcounts = [], [], [], [], [], [], []
        for grp, real in _full_batches(items, args.batch):
            lat = runner(_window_batch(grp, dev), _mask_batch(grp, dev))
            if bits is not None:                          # the codes of the kernel that ran inside the graph
                lat, q = lat
            for i in range(real):
                c = grp[i][2]
                means.append(lat.mean[i, :c].float().cpu())
                sels.append(lat.selection[i, :c].cpu())
                if args.with_logvar:
                    lvs.append(lat.log_variance[i, :c].float().cpu())
                if bits is not None:
                    codes.append(q.codes[i, :c].cpu())
                    steps.append(q.step[i, :c].cpu())
                    if args.entropy_code:                 # the runner's outputs are static: cloned
                        dcodes.append(q.codes[i, :c].clone())
                        dcounts.append(q.counts[i, :c].clone())
        entropy = _entropy_code(torch.cat(dcodes), torch.cat(sels).to(dev), torch.cat(dcounts), bits, _context_grid(args, model),
                                _entropy_period(args)) if args.entropy_code else None
        arrays = pack_latents(torch.cat(means), torch.cat(sels), torch.cat(lvs) if args.with_logvar else None,
                              quant=None if bits is None else (torch.cat(codes), torch.cat(steps), bits), entropy=entropy)
        arrays["window"] = np.int64(args.frames)
        note = _write_latents(args, path, arrays, int(arrays["n_frames"]), args.size, args.size)
        print(f"{path}: {int(arrays['n_frames'])} frames, {int(arrays['selection'].sum())} kept{note}", flush=True)


def _write_video(args, name, video, note=""):
    """Write the frames (n, H, W, 3) of the latent file ``name`` under --out as --ext and print the file's line (``note``: its grid)."""
    n = video.shape[0]
    out_path = os.path.join(args.out, os.path.splitext(name)[0] + "." + args.ext)
    if args.ext == "y4m":
        # on the GPU: uint8 by batch_to_video's rule (clip to [0, 1], x 255 in fp32, truncate), then the planes (ops.rgb_to_yuv); only they
        # come back.  The file is byte for byte what batch_to_video(..., ".y4m") writes from the same frames on the host.
        from . import y4m
        u8 = (video.to(torch.device("cuda", 0)).float().clamp(0, 1) * 255).to(torch.uint8)
        full = args.y4m_range == "full"
        planes = ops.rgb_to_yuv(u8, args.y4m_chroma, args.y4m_matrix, full)
        y4m.write(out_path, tuple(p.cpu().numpy() for p in planes), fps=args.fps, chroma=args.y4m_chroma, full=full)
        print(f"Saved video to {out_path} ({n} frames, {video.shape[2]}x{video.shape[1]}, {args.fps} fps)", file=sys.stderr)
    else:
        D.batch_to_video({"video": video[None], "mask": torch.ones(1, n)}, out_path)
    print(f"{name}: {n} frames{note} -> {out_path}", flush=True)


def _frames_out(args, frames):
    """The frames a decode path hands to ``_write_video``: on the host, except for --ext y4m, whose conversion runs on the GPU."""
    return frames if args.ext == "y4m" else frames.cpu()


def _decode_tiled(args, model, weights, window, fill, arrays, name, runner):
    """One tiled latent file -> its (n_frames, H, W, 3) frames: every tile's windows decoded, blended (tiling.TiledInference "decode")."""
    from .tiling import TiledInference
    dev = torch.device("cuda", 0)
    comp, _, grid = unpack_latents_tiled(arrays, fill)
    wins = windows(comp.shape[1], window)
    cr, mask = (np.stack(x) for x in zip(*[_pad_window(comp[:, s:s + c], window, fill, axis=1) for s, c in wins]))
    if runner is None:
        runner = TiledInference(model, weights, grid, args.batch, window, "decode")
    runner = runner.with_grid(grid)
    out = runner(torch.from_numpy(cr).to(dev).to(model.decoder.dtype), torch.from_numpy(mask).to(dev))
    _write_video(args, name, _frames_out(args, torch.cat([out.frames[i, :c] for i, (_, c) in enumerate(wins)])),
                 f" of {grid.height}x{grid.width} ({grid.ny}x{grid.nx} tiles)")
    return runner


def _decode_windows(args, model, weights, fill, arrays, name, runner):
    """One windowed latent file -> its (n_frames, H, W, 3) frames (tiling.ClipInference "decode")."""
    dev = torch.device("cuda", 0)
    comp, _, grid, plan = unpack_latents_windows(arrays, fill)
    cr, _ = _pad_window(comp, plan.frames, fill, axis=2)               # a clip shorter than a window: the fill token past it
    if runner is None:
        from .tiling import ClipInference
        runner = ClipInference(model, weights, grid, args.batch, plan.frames, plan.overlap, "decode")
    runner = runner.with_grid(grid, plan.overlap)
    out = runner(torch.from_numpy(cr).to(dev).to(model.decoder.dtype), plan.length, cuts=getattr(plan, "cuts", None))
    _write_video(args, name, _frames_out(args, out.frames), f" of {grid.height}x{grid.width} ({grid.ny}x{grid.nx} tiles, windows at {plan.starts})")
    return runner


def cmd_decode(args):
    files = sorted(f for f in os.listdir(args.latents) if f.endswith(".npz"))
    if not files:
        raise SystemExit(f"no latent files (.npz) under {args.latents}")
    with np.load(os.path.join(args.latents, files[0])) as z:
        window, size, small = int(z["window"]), int(z["size"]), bool(int(z["small"]))
    # the model the files name; the Decoder is the same in both flavours
    dev, model, weights, _ = _setup(argparse.Namespace(**vars(args), size=size, small=small), "model")
    runner = GraphedInference(model, weights, args.batch, window, "decode")
    fill = model.fill_token.detach().float().cpu().numpy().reshape(-1)
    tiled = windowed = None
    os.makedirs(args.out, exist_ok=True)
    for name in files:
        with np.load(os.path.join(args.latents, name)) as z:
            arrays = {k: z[k] for k in z.files}
        if "mean_ans" in arrays:                          # range-coded: decoded on the GPU, then a quantised file like any other
            arrays = _entropy_decode(arrays, dev, name)
        if "window_starts" in arrays:
            windowed = _decode_windows(args, model, weights, fill, arrays, name, windowed)
            continue
        if "tile_grid" in arrays:
            tiled = _decode_tiled(args, model, weights, window, fill, arrays, name, tiled)
            continue
        comp, _ = unpack_latents(arrays, fill)
        items = [_pad_window(comp[s:s + c], window, fill) + (c,) for s, c in windows(comp.shape[0], window)]
        recon = []
        for grp, real in _full_batches(items, args.batch):
            cr = torch.from_numpy(np.stack([g[0] for g in grp])).to(dev).to(model.decoder.dtype)
            out = runner(cr, _mask_batch(grp, dev))
            recon += [_frames_out(args, out[i, :grp[i][2]].float().clone()) for i in range(real)]         # the output is static
        _write_video(args, name, torch.cat(recon))


def _metric_arrays(fm):
    """metrics.FrameMetrics -> {"psnr", "ssim", "mse"}: its per-frame values as numpy arrays."""
    return {"psnr": fm.psnr.cpu().numpy(), "ssim": fm.ssim.cpu().numpy(), "mse": fm.mse.cpu().numpy()}


def _clip_entry(args, path, per, shape=(), kept_fraction=None, extra=()):
    """A clip's entry of eval's JSON from ``per`` = {"psnr", "ssim", "mse", "selection"}, float64 per frame: name, path, frames,
    ``shape`` (the tiled modes' height / width / tiles), the means, ``kept_fraction`` (the mean selection unless given), ``extra`` (what
    the mode adds) and, with --per-frame, ``per`` itself."""
    entry = {"name": _stem(path), "path": path, "frames": int(per["psnr"].shape[0]), **dict(shape)}
    entry.update({k: float(per[k].mean()) for k in ("psnr", "ssim", "mse")})
    entry["kept_fraction"] = float(per["selection"].mean()) if kept_fraction is None else kept_fraction
    entry.update(extra)
    if args.per_frame:
        entry["per_frame"] = {k: per[k].tolist() for k in per}
    return entry


def _eval_tiled(args, model, weights, rngs):
    """eval --tile: every clip at its own resolution through tiling.TiledInference("evaluate") (all its windows in one call) -> the clip
    entries; metrics of the stitched frames, kept_fraction = the mean selection over tiles and valid frames."""
    from .tiling import TileGrid
    dev = torch.device("cuda", 0)
    runner, clips = None, []
    for path in _clip_paths(args.data):
        video, mask, counts = clip_windows_native(path, args.frames, _y4m_read(args))
        grid = TileGrid(video.shape[2], video.shape[3], args.size, args.overlap)
        runner = _tiled_runner(runner, model, weights, args, grid, "evaluate", rngs)
        out = runner(torch.from_numpy(video).to(dev), torch.from_numpy(mask).to(dev))
        got = {**_metric_arrays(out.metrics), "selection": out.selection.mean(dim=1).cpu().numpy()}
        per = {k: np.concatenate([got[k][i, :c] for i, c in enumerate(counts)]).astype(np.float64) for k in got}
        entry = _clip_entry(args, path, per, dict(height=grid.height, width=grid.width, tiles=[grid.ny, grid.nx]))
        if args.ms_ssim:
            ms = _ms_ssim_or_exit(args, torch.from_numpy(video).to(dev).float() / 255.0, out.frames, torch.from_numpy(mask).to(dev))
            _add_ms_ssim(entry, torch.cat([ms[i, :c] for i, c in enumerate(counts)]), args)
        if args.temporal_metrics:
            x = torch.cat([torch.from_numpy(video[i, :c]) for i, c in enumerate(counts)]).to(dev).float() / 255.0
            y = torch.cat([out.frames[i, :c] for i, c in enumerate(counts)])
            _add_temporal(entry, temporal_mse(x[None], y[None])[0], args)
        clips.append(entry)
    return clips


def _ms_ssim_or_exit(args, video, recon, mask):
    """metrics.ms_ssim at --ms-ssim-scales scales (the first N standard weights) -> fp32 (B, T); frames the scales do not take end the
    command with the ValueError's message and exit status 2."""
    try:
        return ms_ssim(video, recon, mask, weights=MS_SSIM_WEIGHTS[:args.ms_ssim_scales])
    except ValueError as e:
        print(f"eval --ms-ssim: {e}", file=sys.stderr, flush=True)
        raise SystemExit(2)


def _add_ms_ssim(entry, values, args):
    """entry += ms_ssim, the mean over one clip's real frames of their per-frame ``values`` (and the list with --per-frame)."""
    v = values.double().cpu().numpy()
    entry["ms_ssim"] = float(v.mean())
    if args.per_frame:
        entry["per_frame"]["ms_ssim"] = v.tolist()


def _add_temporal(entry, tmse, args, cuts=None):
    """entry += tmse / tmse_seam / tmse_inner / pairs / seam_pairs of one clip's pair values (and the per-pair list with --per-frame);
    with scene ``cuts`` also tmse_scene / scene_pairs, the pairs across cuts, which then leave the seam and inner means."""
    v = tmse.double().cpu().numpy()
    entry.update(temporal_summary(v, args.frames) if cuts is None else temporal_summary_scenes(v, args.frames, cuts))
    if args.per_frame:
        entry["per_frame"]["tmse"] = v.tolist()


def _eval_windows(args, model, weights, rngs):
    """eval --temporal-overlap: every clip through tiling.ClipInference("evaluate") on overlapping windows (tiled or the 1 x 1 grid of the
    centre square) -> the clip entries; metrics of the stitched clip; kept_fraction = the mean selection over windows, tiles and real
    window frames; a frame's selection = the mean over its windows of their mean over tiles."""
    dev = torch.device("cuda", 0)
    runner, clips = None, []
    for path in _clip_paths(args.data):
        clip, u8, cuts = read_clip_cuts(path, args, dev)
        grid = _clip_grid(clip, args)
        runner = _clip_runner(runner, model, weights, args, grid, "evaluate", rngs)
        out = runner(u8, cuts=cuts)
        plan = out.plan
        selw = out.selection.mean(dim=1).cpu().numpy().astype(np.float64)                # (windows, F)
        per = {k: v[0].astype(np.float64) for k, v in _metric_arrays(out.metrics).items()}
        per["selection"] = np.array([np.mean([selw[w, f - plan.starts[w]] for w in plan.covering(f)]) for f in range(plan.length)])
        extra = dict(windows=plan.windows, stored_ratio=plan.stored_ratio())
        if cuts is not None:
            extra.update(scene_cuts=list(cuts), scenes=scene_ranges(cuts, plan.length))
        entry = _clip_entry(args, path, per, dict(height=grid.height, width=grid.width, tiles=[grid.ny, grid.nx]) if args.tile else (),
                            float(np.concatenate([selw[w, :c] for w, c in enumerate(plan.counts)]).mean()), extra)
        if args.ms_ssim:
            ones = torch.ones((1, plan.length), dtype=torch.float32, device=dev)
            _add_ms_ssim(entry, _ms_ssim_or_exit(args, u8.float()[None] / 255.0, out.frames[None], ones)[0], args)
        if args.temporal_metrics:
            _add_temporal(entry, temporal_mse(u8.float()[None] / 255.0, out.frames[None])[0], args, cuts)
        clips.append(entry)
    return clips


def _eval_untiled(args, model, weights, rngs):
    """The clip entries of eval: centre-square windows through one replayed "evaluate" graph."""
    dev = torch.device("cuda", 0)
    bits = args.quantise_bits
    runner = GraphedInference(model, weights, args.batch, args.frames, "evaluate", rngs=rngs, quant_bits=bits)
    ld = model.encoder.selection_layer1.kernel.shape[0]
    clips = []
    for path in _clip_paths(args.data):
        items = clip_windows(path, args.size, args.frames, dev if args.device_resize else None, _y4m_read(args))
        per = {"psnr": [], "ssim": [], "mse": [], "selection": []}
        xs, ys, mss, pms = [], [], [], []
        pooled = np.zeros((256,), dtype=np.int64)         # --quantise-bits: the clip's code histogram, its real frames only
        dcodes, dkeep, dcounts = [], [], []               # --entropy-code: the clip's codes stay on the GPU until the clip ends
        for grp, real in _full_batches(items, args.batch):
            video = _window_batch(grp, dev)
            mask = _mask_batch(grp, dev)
            if bits is None:
                recon, fm, sel = runner(video, mask)
            else:
                recon, fm, sel, counts = runner(video, mask)
                counts = counts.cpu().numpy().astype(np.int64)
                for i in range(real):
                    pooled += counts[i, :grp[i][2]].sum(axis=0)
                    if args.entropy_code:                 # static tensors of the graph: cloned
                        dcodes.append(runner.quantised.codes[i, :grp[i][2]].clone())
                        dcounts.append(runner.quantised.counts[i, :grp[i][2]].clone())
                        dkeep.append((sel * mask)[i, :grp[i][2]].clone())
            if args.ms_ssim:                              # eagerly, beside the replayed graph, from its inputs and static output
                ms = _ms_ssim_or_exit(args, video, recon, mask)
                mss += [ms[i, :grp[i][2]] for i in range(real)]
            if args.yuv_metrics:                          # likewise: the uint8 windows against the uint8 reconstruction, as planes
                pms += _yuv_window_metrics(args, grp, real, recon, dev)
            got = {**_metric_arrays(fm), "selection": sel.cpu().numpy()}
            for i in range(real):
                for k in per:
                    per[k].append(got[k][i, :grp[i][2]])
                if args.temporal_metrics:                 # the windows' real frames, concatenated (the outputs are static: cloned)
                    xs.append(video[i, :grp[i][2]].clone())
                    ys.append(recon[i, :grp[i][2]].clone())
        per = {k: np.concatenate(v).astype(np.float64) for k, v in per.items()}
        extra = {}
        if bits is not None:
            coded = coded_context = coded_temporal = None
            if args.entropy_code:                         # the size of the stream a file of this clip would hold
                coded = coded_bits(*_entropy_code(torch.cat(dcodes), torch.cat(dkeep), torch.cat(dcounts), bits))
            if getattr(args, "entropy_context", False):   # and of the context coder's, side by side
                coded_context = coded_bits(*_entropy_code(torch.cat(dcodes), torch.cat(dkeep), torch.cat(dcounts), bits,
                                                          _context_grid(args, model))[:2])
            if getattr(args, "entropy_temporal", False):  # and of the temporal coder's
                coded_temporal = coded_bits(*_entropy_code(torch.cat(dcodes), torch.cat(dkeep), torch.cat(dcounts), bits,
                                                           period=args.entropy_period)[:2])
            extra["rate"] = rate_summary(pooled, per["selection"], int(per["psnr"].shape[0]), args.size, args.size, ld, bits, coded=coded,
                                         coded_context=coded_context, coded_temporal=coded_temporal)
            extra.update({k: extra["rate"][k] for k in _rate_keys(args)})
        entry = _clip_entry(args, path, per, extra=extra)
        if args.ms_ssim:
            _add_ms_ssim(entry, torch.cat(mss), args)
        if args.yuv_metrics:
            _add_planes(entry, PM.concat_planes(pms), args)
        if args.temporal_metrics:
            _add_temporal(entry, temporal_mse(torch.cat(xs)[None], torch.cat(ys)[None])[0], args)
        clips.append(entry)
    return clips


def _yuv_window_metrics(args, grp, real, recon, dev):
    """eval --yuv-metrics: the PlaneMetrics of the real windows of a group: their uint8 frames (clip_windows items) against the
    reconstruction taken to uint8 by batch_to_video's rule (clip to [0, 1], x 255 in fp32, truncate: what decode --ext y4m runs), both
    through ops.rgb_to_yuv with --y4m-matrix, limited range unless --y4m-range full; the real frames only."""
    full = args.y4m_range == "full"
    rec8 = (recon.float().clamp(0, 1) * 255).to(torch.uint8)
    out = []
    for i in range(real):
        c = grp[i][2]
        src = grp[i][0] if torch.is_tensor(grp[i][0]) else torch.from_numpy(grp[i][0]).to(dev)
        a = ops.rgb_to_yuv(src[:c].contiguous(), args.yuv_chroma, args.y4m_matrix, full)
        b = ops.rgb_to_yuv(rec8[i, :c].contiguous(), args.yuv_chroma, args.y4m_matrix, full)
        out.append(PM.plane_metrics(a, b, args.yuv_chroma))
    return out


def _add_planes(entry, pm, args):
    """entry += psnr_y / psnr_u / psnr_v / psnr_yuv / ssim_y / mse_y, the means over one clip's frames of its PlaneMetrics (and the
    per-frame lists and integer sse rows with --per-frame)."""
    entry.update({k: v for k, v in PM.summarize_planes(pm).items() if k != "frames"})
    if args.per_frame:
        entry.setdefault("per_frame", {}).update(PM.per_frame_planes(pm))


def _clip_shape(path, y4m=None):
    """(T, H, W, 3) of a clip on disk without converting it."""
    if path.endswith(D.Y4M_EXT):
        return tuple(D.open_y4m(path, y4m).shape)
    if path.endswith(".npy"):
        return tuple(np.load(path, mmap_mode="r").shape)
    return tuple(_read_raw(path, y4m).shape)


def pair_clips(ref_dir, test_dir, y4m=None):
    """The clips of two folders paired by file stem (data.list_video_files on both sides) -> [(stem, ref path, test path, (T, H, W))].
    A stem missing on either side, a pair with different frame sizes or different frame counts: SystemExit naming it and both values.
    Host only."""
    sides = []
    for d in (ref_dir, test_dir):
        paths = _clip_paths(d)
        by_stem = {}
        for p in paths:
            if _stem(p) in by_stem:
                raise SystemExit(f"compare: {d} holds two clips named {_stem(p)!r}: {by_stem[_stem(p)]} and {p}")
            by_stem[_stem(p)] = p
        sides.append(by_stem)
    ref, test = sides
    for stem in sorted(set(ref) ^ set(test)):
        have, miss = (ref_dir, test_dir) if stem in ref else (test_dir, ref_dir)
        raise SystemExit(f"compare: clip {stem!r} is under {have} and missing under {miss}")
    pairs = []
    for stem in sorted(ref):
        a, b = _clip_shape(ref[stem], y4m), _clip_shape(test[stem], y4m)
        if a[1:3] != b[1:3]:
            raise SystemExit(f"compare: clip {stem!r}: frames of {a[1]}x{a[2]} in {ref[stem]} and of {b[1]}x{b[2]} in {test[stem]}")
        if a[0] != b[0]:
            raise SystemExit(f"compare: clip {stem!r}: {a[0]} frames in {ref[stem]} and {b[0]} in {test[stem]}")
        if a[0] < 1:
            raise SystemExit(f"compare: clip {stem!r} has no frames")
        pairs.append((stem, ref[stem], test[stem], a[:3]))
    return pairs


def run_pieces(a, b, run_bytes=D.UPLOAD_RUN_BYTES):
    """[(s, e)] covering the frames of two y4m.Y4MClip of one length: their ``runs`` intersected, so each piece is one run of either file."""
    n = a.shape[0]
    cuts = sorted({0, n} | {e for s, e in a.runs(0, n, run_bytes)} | {e for s, e in b.runs(0, n, run_bytes)})
    return list(zip(cuts[:-1], cuts[1:]))


def _compare_planes(a, b, dev):
    """Two .y4m clips of one chroma form, piece by piece: on the GPU the frame records of both go up as they lie in the file and their
    planes are views of the two uploads; without one the planes are views of the memory-mapped files.  No colour conversion."""
    parts = []
    for s, e in run_pieces(a, b):
        if dev is None:
            parts.append(PM.plane_metrics(a.planes(s, e), b.planes(s, e), a.chroma))
            continue
        planes = []
        for clip in (a, b):
            rec, line, stride = clip.records(s, e)
            buf = torch.from_numpy(np.array(rec)).to(dev)                  # copy: the memory map is read-only
            h, w = clip.shape[1:3]
            ch, cw = clip.header.chroma_shape
            view = lambda off, r, c: buf.as_strided((e - s, r, c), (stride, c, 1), off)
            planes.append((view(line, h, w),) + ((None, None) if clip.chroma == "mono" else
                                                 (view(line + h * w, ch, cw), view(line + h * w + ch * cw, ch, cw))))
        parts.append(PM.plane_metrics(planes[0], planes[1], a.chroma))
    return PM.concat_planes(parts)


def _compare_rgb(a, b, args, full, dev):
    """Any other pair: both sides become RGB (on the GPU by data.upload_rgb), then planes by ops.rgb_to_yuv with --y4m-matrix and the
    pair's range in the --yuv-chroma form; without a GPU the same through y4m.rgb_to_yuv_reference, 64 frames at a time."""
    from . import y4m
    if dev is not None:
        up = lambda c: D.upload_rgb(c if isinstance(c, y4m.Y4MClip) else np.array(c), dev)     # a copy: an .npy is mapped read-only
        pa = ops.rgb_to_yuv(up(a), args.yuv_chroma, args.y4m_matrix, full)
        pb = ops.rgb_to_yuv(up(b), args.yuv_chroma, args.y4m_matrix, full)
        return PM.concat_planes([PM.plane_metrics(pa, pb, args.yuv_chroma)])
    parts = []
    for s in range(0, a.shape[0], 64):
        pa = y4m.rgb_to_yuv_reference(np.asarray(a[s:s + 64]), args.yuv_chroma, args.y4m_matrix, full)
        pb = y4m.rgb_to_yuv_reference(np.asarray(b[s:s + 64]), args.yuv_chroma, args.y4m_matrix, full)
        parts.append(PM.plane_metrics(pa, pb, args.yuv_chroma))
    return PM.concat_planes(parts)


def cmd_compare(args):
    """Score the clips under --test against those under --ref with the plane-wise metrics (plane_metrics.py) -> one JSON file of eval's
    shape.  No model.  Two .y4m clips of one chroma form and siting are compared as they lie in their files (route "planes"); any other
    pair through RGB (route "rgb").  Without a GPU the host reference runs."""
    from .y4m import Y4MClip
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else None
    y4m = _y4m_read(args)
    clips = []
    for stem, ref_path, test_path, (n, h, w) in pair_clips(args.ref, args.test, y4m):
        a, b = _open_raw(ref_path, y4m), _open_raw(test_path, y4m)
        both = isinstance(a, Y4MClip) and isinstance(b, Y4MClip)
        try:
            if both and (a.chroma, a.siting) == (b.chroma, b.siting):
                route, chroma = "planes", a.chroma
                pm = _compare_planes(a, b, dev)
            else:
                route, chroma = "rgb", args.yuv_chroma
                own = [c.full for c in (a, b) if isinstance(c, Y4MClip)]
                full = (own[0] if own else False) if args.y4m_range == "header" else args.y4m_range == "full"
                pm = _compare_rgb(a, b, args, full, dev)
        except ValueError as e:
            raise SystemExit(f"compare: clip {stem!r}: {e}")
        entry = {"name": stem, "ref": ref_path, "test": test_path, "frames": n, "height": h, "width": w, "chroma": chroma, "route": route}
        _add_planes(entry, pm, args)
        clips.append(entry)
        print(f"{stem}: {n} frames of {h}x{w}, {chroma} by {route}: psnr_y {entry['psnr_y']:.3f} dB, psnr_yuv {entry['psnr_yuv']:.3f} dB, "
              f"ssim_y {entry['ssim_y']:.4f}", flush=True)
    total = sum(c["frames"] for c in clips)
    dataset = {"clips": len(clips), "frames": total}
    dataset.update({k: sum(c[k] * c["frames"] for c in clips) / total for k in PM.KEYS})
    config = dict(ref=args.ref, test=args.test, y4m_matrix=args.y4m_matrix, y4m_range=args.y4m_range, yuv_chroma=args.yuv_chroma,
                  device="gpu" if dev is not None else "host")
    _write_json(args.out, {"config": config, "dataset": dataset, "clips": clips})
    print(f"compare: {len(clips)} clips, {total} frames: psnr_y {dataset['psnr_y']:.3f} dB, psnr_u {dataset['psnr_u']:.3f} dB, "
          f"psnr_v {dataset['psnr_v']:.3f} dB, psnr_yuv {dataset['psnr_yuv']:.3f} dB, ssim_y {dataset['ssim_y']:.4f} -> {args.out}", flush=True)


def cmd_eval(args):
    """Reconstruct every clip through one replayed "evaluate" graph (tiled: tiling.TiledInference) and write its per-frame metrics,
    reduced per clip and over the dataset (frame-weighted), as JSON.  The padding of a short last window and the copies filling a short
    last batch never count."""
    dev, model, weights, rngs = _setup(args)
    if args.temporal_overlap is not None:
        clips = _eval_windows(args, model, weights, rngs)
    elif args.tile:
        clips = _eval_tiled(args, model, weights, rngs)
    else:
        clips = _eval_untiled(args, model, weights, rngs)
    n = sum(c["frames"] for c in clips)
    dataset = {"clips": len(clips), "frames": n}
    dataset.update({k: sum(c[k] * c["frames"] for c in clips) / n for k in ("psnr", "ssim", "mse", "kept_fraction")})
    if args.ms_ssim:
        dataset.update(ms_ssim=sum(c["ms_ssim"] * c["frames"] for c in clips) / n)
    if args.yuv_metrics:
        dataset.update({k: sum(c[k] * c["frames"] for c in clips) / n for k in PM.KEYS})
    if args.temporal_metrics:                         # pair-weighted
        pairs = sum(c["pairs"] for c in clips)
        seams = sum(c["seam_pairs"] for c in clips)
        wmean = lambda k, w, tot: sum(c[k] * w(c) for c in clips) / tot if tot else 0.0
        dataset.update(tmse=wmean("tmse", lambda c: c["pairs"], pairs), tmse_seam=wmean("tmse_seam", lambda c: c["seam_pairs"], seams),
                       tmse_inner=wmean("tmse_inner", lambda c: c["pairs"] - c["seam_pairs"] - c.get("scene_pairs", 0),
                                        pairs - seams - sum(c.get("scene_pairs", 0) for c in clips)), pairs=pairs, seam_pairs=seams)
        if args.scene_cuts:
            scene = sum(c["scene_pairs"] for c in clips)
            dataset.update(tmse_scene=wmean("tmse_scene", lambda c: c["scene_pairs"], scene), scene_pairs=scene)
    if args.scene_cuts:
        dataset.update(scene_cuts=sum(len(c["scene_cuts"]) for c in clips), scenes=sum(len(c["scenes"]) for c in clips))
    if args.quantise_bits is not None:                # ratios of sums over the clips, not means of their ratios
        dataset["rate"] = rate_dataset(c["rate"] for c in clips)
        dataset.update({k: dataset["rate"][k] for k in _rate_keys(args)})
    config = {k: getattr(args, k) for k in ("model_path", "data", "flavour", "size", "frames", "batch", "small", "threshold", "seed")}
    config.update(clamp=True, gate="threshold" if rngs is None else "bernoulli", weights="ema" if args.ema else "raw",
                  resize="device" if args.device_resize else "host")
    if args.tile:
        config.update(tile=True, overlap=args.overlap)
    if args.temporal_overlap is not None:
        config.update(temporal_overlap=args.temporal_overlap)
    if args.temporal_metrics:
        config.update(temporal_metrics=True)
    if args.ms_ssim:
        config.update(ms_ssim=True, ms_ssim_scales=args.ms_ssim_scales)
    if args.yuv_metrics:
        config.update(yuv_metrics=True, yuv_chroma=args.yuv_chroma, yuv_matrix=args.y4m_matrix,
                      yuv_range="full" if args.y4m_range == "full" else "limited")
    if args.scene_cuts:
        config.update(scene_cuts=scene_config(args))
    if args.quantise_bits is not None:
        config.update(quantise_bits=args.quantise_bits)
    if args.entropy_code:
        config.update(entropy_code=True)
    if getattr(args, "entropy_context", False):
        config.update(entropy_context=True)
    if getattr(args, "entropy_temporal", False):
        config.update(entropy_temporal=True, entropy_period=args.entropy_period)
    _write_json(args.out, {"config": config, "dataset": dataset, "clips": clips})
    rate = "" if args.quantise_bits is None else f", bpp raw {dataset['bpp_raw']:.4f} / entropy {dataset['bpp_entropy']:.4f}"
    if args.entropy_code:
        rate += f" / coded {dataset['bpp_coded']:.4f}"
    if getattr(args, "entropy_context", False):
        rate += f" / coded with contexts {dataset['bpp_coded_context']:.4f}"
    if getattr(args, "entropy_temporal", False):
        rate += f" / coded against the previous frame {dataset['bpp_coded_temporal']:.4f}"
    if args.ms_ssim:
        rate += f", ms-ssim ({args.ms_ssim_scales} scales) {dataset['ms_ssim']:.4f}"
    if args.yuv_metrics:
        rate += f", psnr-y {dataset['psnr_y']:.3f} dB, psnr-yuv {dataset['psnr_yuv']:.3f} dB, ssim-y {dataset['ssim_y']:.4f}"
    print(f"eval: {len(clips)} clips, {n} frames: psnr {dataset['psnr']:.3f} dB, ssim {dataset['ssim']:.4f}, mse {dataset['mse']:.3e}, "
          f"kept {dataset['kept_fraction']:.3f}{rate} -> {args.out}", flush=True)


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m video_vae_amd.infer", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    e = sub.add_parser("encode", help="clips -> one latent .npz per clip (kept frames' means, per-frame selection)")
    v = sub.add_parser("eval", help="clips -> PSNR / SSIM / MSE of their reconstructions and the kept-frame fraction, per clip and "
                                    "over the dataset, as JSON")
    for a in (e, v):
        a.add_argument("--model_path", required=True, help="checkpoint directory (model_loader.save_checkpoint)")
        a.add_argument("--data", required=True, help="directory of clips (.npy / .npz uint8 (T, H, W, 3), .y4m YUV4MPEG2; videos{i}/ "
                                                     "sub-directories or flat)")
        a.add_argument("--flavour", default="rl", choices=["rl", "model"])
        a.add_argument("--size", type=int, default=256, help="frames are centre-cropped to a square and resized to size x size "
                                                             "(with --tile: the model's frame side, the tile side)")
        a.add_argument("--frames", type=int, default=16, help="window length; the last window of a clip is zero-padded and masked")
        a.add_argument("--batch", type=int, default=4, help="windows per replay")
        a.add_argument("--small", action="store_true", help="the depth-1 model of train.py --small")
        a.add_argument("--threshold", action="store_true", help="rl flavour: gate by round(probability) instead of a Bernoulli draw")
        a.add_argument("--seed", type=int, default=0, help="rl flavour: seed of the Bernoulli draws")
    for a in (e, v):
        a.add_argument("--tile", action="store_true", help="read clips at their own resolution (no crop, no resize) and run size x size "
                                                           "tiles blended back (tiling.py)")
        a.add_argument("--overlap", type=int, default=32, help="--tile: least overlap of neighbouring tiles, 0 .. size // 2")
        a.add_argument("--temporal-overlap", dest="temporal_overlap", type=int, default=None,
                       help="windows of --frames frames whose neighbours overlap by at least this many frames (0 .. frames // 2), "
                            "blended back in time (tiling.ClipInference); without it a clip is cut into hard windows")
    sc = sub.add_parser("scenes", help="clips -> their scene cuts (per-frame colour histograms on the GPU), as JSON; no model")
    sc.add_argument("--data", required=True, help="directory of clips (.npy / .npz uint8 (T, H, W, 3), .y4m YUV4MPEG2; videos{i}/ "
                                                  "sub-directories or flat)")
    sc.add_argument("--out", default="scenes.json", help="the JSON file written")
    c = sub.add_parser("compare", help="two folders of clips, paired by file stem -> PSNR-Y / -U / -V, the sample-pooled PSNR-YUV and SSIM-Y of "
                                       "--test against --ref on their 8-bit Y'CbCr planes (plane_metrics.py), as JSON; no model")
    c.add_argument("--ref", required=True, help="directory of the reference clips (.npy / .npz uint8 (T, H, W, 3), .y4m YUV4MPEG2)")
    c.add_argument("--test", required=True, help="directory of the clips scored against them; the same stems, frame sizes and frame counts")
    c.add_argument("--out", default="metrics.json", help="the JSON file written")
    c.add_argument("--per-frame", dest="per_frame", action="store_true", help="also store every frame's values and its integer squared errors")
    c.add_argument("--y4m-matrix", dest="y4m_matrix", default="bt601", choices=["bt601", "bt709"],
                   help="pairs that go through RGB: the matrix .y4m planes become RGB with and RGB becomes planes with (y4m.py)")
    c.add_argument("--y4m-range", dest="y4m_range", default="header", choices=["header", "limited", "full"],
                   help="pairs that go through RGB: the range of both conversions; header = a .y4m side's own (limited unless it says "
                        "XCOLORRANGE=FULL; the reference's where both are .y4m), limited for a pair without one")
    for a in (v, c):
        a.add_argument("--yuv-chroma", dest="yuv_chroma", default="420", choices=["420", "444"],
                       help="the chroma form RGB frames are taken to planes in (eval --yuv-metrics; compare: pairs that are not two "
                            ".y4m clips of one form, which are compared as they lie in their files)")
    for a in (e, v, sc):
        a.add_argument("--y4m-matrix", dest="y4m_matrix", default="bt601", choices=["bt601", "bt709"],
                       help=".y4m clips: the matrix their planes become RGB with (y4m.py); the container carries no matrix tag")
        a.add_argument("--y4m-range", dest="y4m_range", default="header", choices=["header", "limited", "full"],
                       help=".y4m clips: their range; header = limited unless the file says XCOLORRANGE=FULL")
        a.add_argument("--scene-hist", dest="scene_hist", type=int, default=64,
                       help="scene cuts: bins per histogram axis (HSV: n x n over hue and saturation, up to 64; gray: n, up to 256)")
        a.add_argument("--scene-similarity", dest="scene_similarity", type=float, default=0.85,
                       help="scene cuts: a cut when the accumulated 1 - correlation of consecutive histograms exceeds 1 - this")
        a.add_argument("--scene-gray", dest="scene_gray", action="store_true", help="scene cuts: gray histograms instead of HSV")
    for a in (e, v):
        a.add_argument("--scene-cuts", dest="scene_cuts", action="store_true",
                       help="find each clip's scene cuts and window / blend every scene on its own (tiling.ScenePlan); without "
                            "--temporal-overlap the windows do not overlap")
        a.add_argument("--device-resize", dest="device_resize", action="store_true",
                       help="crop the centre square and resize it to --size on the GPU (csrc/resize.hip: the host path's bytes) instead "
                            "of on the host; not with --tile, which does not resize")
    for a in (e, v):
        a.add_argument("--quantise-bits", dest="quantise_bits", type=int, default=None, choices=range(2, 9), metavar="N",
                       help="quantise the kept means to N bits (2 .. 8) with one step per kept frame and channel (quant.py, "
                            "csrc/quant.hip); encode stores int8 codes and the steps, eval measures through the quantiser and adds "
                            "bits per pixel; off by default")
        a.add_argument("--entropy-code", dest="entropy_code", action="store_true",
                       help="with --quantise-bits: range-code the codes (interleaved rANS, one table per clip; entropy.py, csrc/rans.hip); "
                            "encode stores the stream in place of the int8 codes (decode needs no flag), eval (plain mode) adds the coded "
                            "size as bits_coded / bpp_coded; off by default")
        a.add_argument("--entropy-context", dest="entropy_context", action="store_true",
                       help="with --entropy-code: four tables per clip, a symbol's table chosen by the activity (sum of |code|) of the token "
                            "above its own (entropy.py); encode stores that stream (decode needs no flag), eval (plain mode) adds its size "
                            "as bits_coded_context / bpp_coded_context beside bits_coded / bpp_coded; off by default")
        a.add_argument("--entropy-temporal", dest="entropy_temporal", action="store_true",
                       help="with --entropy-code: nine tables per clip, a symbol's table chosen by the previous kept frame's code at the "
                            "same place (entropy.py: chains of frames); encode stores that stream (decode needs no flag; not with "
                            "--entropy-context: a file has one form), eval (plain mode) adds its size as bits_coded_temporal / "
                            "bpp_coded_temporal; off by default")
        a.add_argument("--entropy-period", dest="entropy_period", type=int, default=16, metavar="P",
                       help="--entropy-temporal: a chain holds at most P kept frames, then a frame is coded on its own again (P >= 1)")
    e.add_argument("--out", required=True)
    e.add_argument("--with-logvar", dest="with_logvar", action="store_true", help="also store the kept frames' log-variance")
    v.add_argument("--out", default="metrics.json", help="the JSON file written")
    v.add_argument("--per-frame", dest="per_frame", action="store_true", help="also store every frame's psnr / ssim / mse / selection")
    v.add_argument("--temporal-metrics", dest="temporal_metrics", action="store_true",
                   help="also the temporal-difference error of consecutive frames (tmse), over all pairs, the pairs across the hard-cut "
                        "seams (later frame a multiple of --frames) and the others")
    v.add_argument("--ms-ssim", dest="ms_ssim", action="store_true",
                   help="also the multi-scale SSIM of every frame (metrics.ms_ssim: Wang, Simoncelli, Bovik 2003), per clip and over the "
                        "dataset; off by default")
    v.add_argument("--ms-ssim-scales", dest="ms_ssim_scales", type=int, default=5, metavar="N",
                   help="--ms-ssim: the number of scales, 1 .. 5, with the first N standard weights; N scales need frames of at least "
                        "11 * 2^(N - 1) on a side (176 at 5)")
    v.add_argument("--yuv-metrics", dest="yuv_metrics", action="store_true",
                   help="also the plane-wise metrics of the 8-bit Y'CbCr planes (plane_metrics.py): PSNR-Y / -U / -V, the sample-pooled "
                        "PSNR-YUV and SSIM-Y of the uint8 reconstruction against the uint8 frames, both taken to planes with --y4m-matrix "
                        "in the --yuv-chroma form, limited range unless --y4m-range full; plain mode only; off by default")
    d = sub.add_parser("decode", help="latent .npz files -> frames (data.batch_to_video)")
    d.add_argument("--model_path", required=True)
    d.add_argument("--latents", required=True)
    d.add_argument("--out", required=True)
    d.add_argument("--batch", type=int, default=4)
    d.add_argument("--ext", default="npz", choices=["npz", "npy", "mp4", "y4m"],
                   help="mp4 needs ffmpeg on PATH; y4m: YUV4MPEG2, converted from RGB on the GPU (csrc/yuv.hip), no library needed")
    d.add_argument("--y4m-matrix", dest="y4m_matrix", default="bt601", choices=["bt601", "bt709"], help="--ext y4m: the matrix (y4m.py)")
    d.add_argument("--y4m-range", dest="y4m_range", default="limited", choices=["limited", "full"],
                   help="--ext y4m: the range, written as XCOLORRANGE")
    d.add_argument("--y4m-chroma", dest="y4m_chroma", default="420", choices=["420", "444"],
                   help="--ext y4m: 4:2:0 (C420jpeg, chroma at the centre of its 2 x 2 block) or 4:4:4")
    d.add_argument("--fps", default="30:1", metavar="N:D", help="--ext y4m: the frame rate written into the header")
    for a in (e, v, d):
        a.add_argument("--ema", action="store_true", help="run the checkpoint's averaged weights (train.py --ema) instead of its last iterate")
    return ap


def parse_args(argv=None):
    """The command's arguments; combinations that make no sense are refused here (argparse's error: exit status 2)."""
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.cmd == "decode":
        n, _, d = args.fps.partition(":")
        if not (n.isdigit() and d.isdigit() and int(n) > 0 and int(d) > 0):
            ap.error(f"--fps {args.fps}: N:D with positive integers")
    if getattr(args, "device_resize", False) and args.tile:
        ap.error("--device-resize cannot be combined with --tile: tiled runs read clips at their own resolution and do not resize")
    if getattr(args, "entropy_code", False) and args.quantise_bits is None:
        ap.error("--entropy-code needs --quantise-bits: the coder codes the quantiser's codes")
    if getattr(args, "entropy_context", False) and not args.entropy_code:
        ap.error("--entropy-context needs --entropy-code: it chooses the range coder's tables")
    if getattr(args, "entropy_temporal", False):
        if not args.entropy_code:
            ap.error("--entropy-temporal needs --entropy-code: it chooses the range coder's tables")
        if args.cmd == "encode" and args.entropy_context:
            ap.error("--entropy-temporal cannot be combined with --entropy-context in encode: a latent file has one form")
        if args.entropy_period < 1:
            ap.error("--entropy-period must be at least 1")
    if getattr(args, "ms_ssim", False):
        if not 1 <= args.ms_ssim_scales <= len(MS_SSIM_WEIGHTS):
            ap.error(f"--ms-ssim-scales must be 1 .. {len(MS_SSIM_WEIGHTS)}")
        if not args.tile:                             # --size decides the frames: refused before the model is built
            try:
                ms_ssim_check(args.size, args.size, 3, args.ms_ssim_scales)
            except ValueError as e:
                ap.error(f"--ms-ssim at --size {args.size}: {e}")
    if getattr(args, "yuv_metrics", False) and (args.tile or args.temporal_overlap is not None or args.scene_cuts):
        ap.error("eval --yuv-metrics runs in plain mode only: the tiled and windowed runners (--tile, --temporal-overlap, --scene-cuts) "
                 "stitch their frames in their own loops, which do not hand the uint8 windows over; run it without them")
    if getattr(args, "quantise_bits", None) is not None:
        if getattr(args, "with_logvar", False):
            ap.error("--quantise-bits cannot be combined with --with-logvar: the log-variance is not quantised")
        if args.cmd == "eval" and (args.tile or args.temporal_overlap is not None or args.scene_cuts):
            ap.error("eval --quantise-bits runs in plain mode only: the tiled and windowed runners (tiling.TiledInference / ClipInference) "
                     "replay a \"reconstruct\" graph and unpack its two outputs, so handing quant_bits through them is not all it takes; "
                     "encode --quantise-bits takes --tile, --temporal-overlap and --scene-cuts")
    return args


def main(argv=None):
    args = parse_args(argv)
    if getattr(args, "scene_cuts", False) and args.temporal_overlap is None:
        args.temporal_overlap = 0                     # scenes run through the windowed path
    {"encode": cmd_encode, "decode": cmd_decode, "eval": cmd_eval, "scenes": cmd_scenes, "compare": cmd_compare}[args.cmd](args)


if __name__ == "__main__":
    main()
