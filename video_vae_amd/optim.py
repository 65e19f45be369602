"""optax.chain(clip_by_global_norm(1.0), adam(warmup_cosine_decay_schedule)) on flat fp32 buffers.

Reference: train/rl_nonadversarial.py:241-253.  All parameters live in ONE flat fp32 buffer (params are views into
it), and so do the gradients and Adam moments: the whole update is two HIP launches (squared-norm reduction, fused
clip+Adam, which also refreshes a bf16 shadow copy of the weights for the next forward) regardless of the parameter
count.  The buffer is laid out in REVERSE registration order and cut into buckets, so the gradients that become ready
first in backward (the UNet at the decoder tail) fill the first bucket.

Gradients land in the flat buffer bucket by bucket: a post-accumulate hook per parameter counts arrivals; when a
bucket is complete its gradients are copied (and widened to fp32) into their slots with one fused multi-tensor copy
and the autograd-owned tensors are released -- no zero-fill of the buffer, no per-parameter accumulate kernels --
and, under data parallelism, the bucket's slice is all-reduced right away (ddp.GradReducer).
"""
import contextlib
import ctypes
import math

import torch

from . import ops
from ._lib import lib, check


def warmup_cosine_decay_schedule(init_value, peak_value, warmup_steps, decay_steps, end_value):
    """optax.warmup_cosine_decay_schedule: returns schedule(count), count 0-based."""
    def schedule(count):
        if count < warmup_steps:
            return init_value + (peak_value - init_value) * (count / warmup_steps)
        span = decay_steps - warmup_steps
        c = min(count - warmup_steps, span)
        cosine = 0.5 * (1.0 + math.cos(math.pi * c / span))
        alpha = end_value / peak_value
        return peak_value * ((1 - alpha) * cosine + alpha)
    return schedule


def reference_schedule(batch_size=2, learning_rate=2e-5, decay_steps=1_000_000):
    """The reference's schedule constants (rl_nonadversarial.py:44-52,241-247)."""
    return warmup_cosine_decay_schedule(0.0, learning_rate, 20000 // math.sqrt(batch_size), decay_steps, learning_rate / 10)


def ema_decay_at(decay, n, warmup):
    """Decay of the weight average for the update after ``n`` earlier ones: ``decay``, or with ``warmup`` min(decay, (1 + n) / (10 + n)),
    which lets a young average follow the weights instead of remembering their initialisation.  A function of the update count alone
    (``Optimizer.count`` before its increment), so a resumed run continues the ramp where it stopped."""
    return min(decay, (1 + n) / (10 + n)) if warmup else decay


def _copy_all(dsts, srcs):
    """Gradients -> their slots of the flat buffer: one grouped HIP launch per 64 tensors (a memcpy node each costs ~4 us of
    GPU time inside the replayed graph), the framework's foreach copy for anything that is not a plain fp32 GPU range."""
    fast = [(d, s) for d, s in zip(dsts, srcs) if ops.copy_grouped_ok(d, s)]
    rest = [(d, s) for d, s in zip(dsts, srcs) if not ops.copy_grouped_ok(d, s)]
    if fast:
        ops.copy_grouped([d for d, _ in fast], [s for _, s in fast])
    if rest:
        torch._foreach_copy_([d for d, _ in rest], [s for _, s in rest])


def _vp(t):
    """The device pointer of a tensor as a C-ABI argument (None -> NULL)."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


STREAM_TAG = "vvae_accumulate_stream"


def accumulate_grad_node(param):
    """The live AccumulateGrad node of a leaf parameter (made on the current stream if none is alive), or None."""
    with torch.enable_grad():
        fn = param.expand_as(param).grad_fn
    nxt = fn.next_functions if fn is not None else ()
    return nxt[0][0] if nxt and nxt[0][0] is not None else None


class Optimizer:
    """Counterpart of ``nnx.Optimizer(model, optax.chain(clip_by_global_norm(max_norm), adam(schedule)))``.

    ``zero_grad()`` then backward then ``update()``.  After ``update()`` the gradients of the step are in ``self.g``.

    ``ema_decay`` (default None: off) keeps an exponential moving average of the weights in ``self.ema`` (flat fp32, the offsets of
    ``self.p``; ``p.ema`` views per parameter), advanced inside the fused update by ema_decay_at(ema_decay, count, ema_warmup);
    ``swapped_ema()`` puts it in the parameters' place for an evaluation.

    ``accum_steps`` = K > 1 (optax.MultiSteps): ``update()`` is still called once per micro-step; the first K - 1 calls of a cycle only sum
    the gradients into ``self.acc`` (flat fp32 like ``self.g``, in arrival order) and return None, the K-th applies ONE clip + Adam (+ average)
    update with the mean gradient.  ``count``, the schedule, the bias corrections and the decay of the average advance once per applied update.
    """

    def __init__(self, model, schedule, max_norm=1.0, b1=0.9, b2=0.999, eps=1e-8, bf16_shadow=True,
                 bucket_bytes=64 << 20, ema_decay=None, ema_warmup=False, accum_steps=1):
        if isinstance(accum_steps, bool) or not isinstance(accum_steps, int) or accum_steps < 1:
            raise ValueError(f"accum_steps {accum_steps!r} is not an integer >= 1")
        self.accum_steps = accum_steps
        self.micro = 0                 # micro-steps already folded into self.acc in the current cycle
        self.acc = None                # the fp32 sum of those micro-steps' gradients (accum_steps > 1 only)
        self.last_update = False       # whether the last update() call applied an update
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay {ema_decay} is outside [0, 1)")
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.ema = None
        self.ema_swapped = False       # True inside swapped_ema(): self.p holds the average, self.ema the raw weights
        self.model = model
        self.schedule = schedule if callable(schedule) else (lambda count, lr=schedule: lr)
        self.max_norm, self.b1, self.b2, self.eps = max_norm, b1, b2, eps
        self.count = 0
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        self.names = [n for n, _ in named][::-1]
        self.params = [p for _, p in named][::-1]
        dev = self.params[0].device
        for p in self.params:
            if p.dtype != torch.float32:
                raise ValueError("Optimizer expects fp32 parameters (param_dtype=float32)")
        self.offsets, off = [], 0
        for p in self.params:
            self.offsets.append(off)
            off += (p.numel() + 3) // 4 * 4          # 16-byte aligned slots
        self.numel = off
        self.p = torch.zeros(off, dtype=torch.float32, device=dev)
        self.g = torch.zeros(off, dtype=torch.float32, device=dev)
        self.m = torch.zeros(off, dtype=torch.float32, device=dev)
        self.v = torch.zeros(off, dtype=torch.float32, device=dev)
        if self.accum_steps > 1:
            self.acc = torch.zeros(off, dtype=torch.float32, device=dev)
        self.gnorm_sq = torch.zeros(1, dtype=torch.float64, device=dev)
        self.gnorm_part = torch.zeros(max(1, lib().vvae_sqnorm_blocks(off)) if dev.type == "cuda" else 1, dtype=torch.float64, device=dev)
        self.shadow = torch.zeros(off, dtype=torch.bfloat16, device=dev) if bf16_shadow else None
        self.gviews = []
        for p, o in zip(self.params, self.offsets):
            n = p.numel()
            self.p[o:o + n].copy_(p.data.reshape(-1))
            p.data = self.p[o:o + n].view(p.shape)
            p.grad = None
            self.gviews.append(self.g[o:o + n].view(p.shape))
            p.gview = self.gviews[-1]                             # written directly by ops.deferred_wgrad
            if self.shadow is not None:
                p.bf16 = self.shadow[o:o + n].view(p.shape)       # read by layers.Linear: no per-call weight casts
        if self.shadow is not None:
            self.shadow.copy_(self.p)
        if self.ema_decay is not None:
            self.ema = self.p.clone()
            for p, o in zip(self.params, self.offsets):
                p.ema = self.ema[o:o + p.numel()].view(p.shape)
        # transposed bf16 shadows (out, in) of the Linear kernels whose forward runs on the own NT GEMM (layers mark them ``want_t``:
        # the MLP's fc1, whose product also emits SiLU); refreshed after every update from the bf16 shadow, one grouped launch per 64
        self.tpairs = []
        if self.shadow is not None and dev.type == "cuda":
            _, self.tpairs = ops.transposed_shadows(self.params, dev)
            ops.transpose_grouped(self.tpairs)
        # ---- buckets: contiguous [start, end) element ranges aligned to parameter slots ----
        cap = max(1, bucket_bytes // 4)
        ends = [o + (p.numel() + 3) // 4 * 4 for o, p in zip(self.offsets, self.params)]
        self.buckets, self.param_bucket, self.bucket_params = [], [], []
        start, members = 0, []
        for i, e in enumerate(ends):
            self.param_bucket.append(len(self.buckets))
            members.append(i)
            if e - start >= cap or i == len(ends) - 1:
                self.buckets.append((start, e))
                self.bucket_params.append(members)
                start, members = e, []
        self.arrived = [0] * len(self.buckets)
        self.landed = [False] * len(self.buckets)
        self.index = {id(p): i for i, p in enumerate(self.params)}
        self.external = set()          # parameter indices whose flat-buffer slot was written directly this step
        self.clean = set(range(len(self.params)))     # slots known to hold zeros (self.g starts zeroed)
        self.hooks_active = True       # False while gradients arrive through land_all (graph capture) instead of the hooks
        self.reducer = None            # set by ddp.GradReducer
        self.defer_reduce = False      # graph mode: do not launch collectives from the landing hooks (see graph.py)
        self.prelaunched = set()       # graph mode: buckets already handed to the reducer between the two replays of a step
        for i, p in enumerate(self.params):
            p.register_post_accumulate_grad_hook(self._make_hook(i))

    # ---- gradient landing -------------------------------------------------------------------------------
    def _make_hook(self, i):
        tagged = [False]

        def hook(param):
            if not tagged[0] and param.is_cuda:
                # Remember, ON the parameter's AccumulateGrad node, which stream it is pinned to (the engine runs the node -- and this
                # hook -- on the stream that was current when the node was made).  graph.GraphedTrainStep reads the tag back: a capture
                # on another stream while such a node is alive crashes the autograd engine (the r03b incident).
                tagged[0] = True
                node = accumulate_grad_node(param)
                if node is not None:
                    node.metadata.setdefault(STREAM_TAG, torch.cuda.current_stream(param.device).cuda_stream)
            if param.grad is None:               # the engine also runs the hook for an undefined gradient (a backward that returned
                return                           # None: parked weight gradients) -- those arrive through mark_external instead
            self._arrive(i)
        return hook

    def _arrive(self, i):
        """One more gradient of parameter i's bucket is there: a complete bucket lands."""
        b = self.param_bucket[i]
        self.arrived[b] += 1
        if self.arrived[b] == len(self.bucket_params[b]) and not self.landed[b]:
            self._land(b)

    def _install(self, indices, grads):
        """Gradients -> the flat-buffer slots ``indices`` (None = zeros): the one landing loop, which also keeps ``self.clean``."""
        dsts, srcs = [], []
        for i, gr in zip(indices, grads):
            if i in self.external:
                self.clean.discard(i)                             # already in place (ops.deferred_wgrad)
            elif gr is None:
                if i not in self.clean:                           # a slot nobody has written since it was last zeroed stays zero
                    self.gviews[i].zero_()
                    self.clean.add(i)
            else:
                self.clean.discard(i)
                if gr.data_ptr() != self.gviews[i].data_ptr():    # (a gradient that already is its slot needs no copy)
                    dsts.append(self.gviews[i])
                    srcs.append(gr)
        if dsts:
            _copy_all(dsts, srcs)

    @torch.no_grad()
    def _land(self, b):
        """Move bucket b's gradients into the flat buffer (missing ones = zeros) and hand the slice to the reducer."""
        members = self.bucket_params[b]
        self._install(members, [self.params[i].grad for i in members])
        for i in members:
            self.params[i].grad = None
        self.landed[b] = True
        if not self.defer_reduce:
            self.reduce_bucket(b)

    @torch.no_grad()
    def land_all(self, grads):
        """Install gradients given in ``self.params`` order (None = zero), e.g. from torch.autograd.grad (graph capture)."""
        self._install(range(len(self.params)), grads)
        self.landed = [True] * len(self.buckets)
        if not self.defer_reduce:                                   # same contract as _land: a landed bucket goes to the reducer
            for b in range(len(self.buckets)):
                self.reduce_bucket(b)

    @torch.no_grad()
    def land_subset(self, indices, grads):
        """land_all for a subset of ``self.params`` (indices, gradients in the same order); buckets are not marked landed."""
        self._install(indices, grads)

    def _fold(self, dst, src, overwrite=False):
        """dst = (overwrite ? 0 : dst) + src on flat fp32 ranges: one HIP pass on the GPU, torch.add on CPU tensors (host tests, gloo)."""
        if dst.is_cuda:
            check(lib().vvae_grad_fold_f32(_vp(dst), _vp(src), dst.numel(), int(overwrite), _stream()), "vvae_grad_fold_f32")
        elif overwrite:
            torch.add(src, 0.0, out=dst)
        else:
            torch.add(dst, src, out=dst)

    @torch.no_grad()
    def reduce_bucket(self, b):
        """The one place a landed bucket is handed to the reducer (the landing hooks, land_all, graph.py's prelaunch and update()'s deferred
        branch all come through here).  Before the last micro-step of an accumulation cycle nothing is communicated; on the last one the
        bucket's slice of the accumulator is folded into the gradients first, so the all-reduce carries this rank's sum over the cycle and
        still overlaps the rest of that micro-step's backward.  -> whether the bucket was launched."""
        if self.reducer is None or self.micro < self.accum_steps - 1:
            return False
        if self.acc is not None:
            s, e = self.buckets[b]
            self._fold(self.g[s:e], self.acc[s:e])
            self.clean.difference_update(self.bucket_params[b])       # a slot without a gradient this micro-step may now hold an earlier one's
        self.reducer.launch(b)
        return True

    def reset_accumulation(self):
        """Drop a partial accumulation cycle (an epoch's end, a stop signal): the next micro-step starts a new sum."""
        self.micro = 0

    def mark_external(self, param):
        """The gradient of ``param`` has been written straight into its flat-buffer slot for this step (ops.deferred_wgrad):
        it counts as arrived, so a completed bucket goes to the reducer while backward is still running."""
        i = self.index[id(param)]
        self.external.add(i)
        if self.hooks_active:
            self._arrive(i)

    def zero_grad(self):
        self.external = set()
        for p in self.params:
            p.grad = None
        self.arrived = [0] * len(self.buckets)
        self.landed = [False] * len(self.buckets)
        if self.reducer is not None:
            self.reducer.reset()

    def set_grads(self, grads):
        """Test helper: install explicit gradients {name: tensor} as if backward had produced them."""
        self.zero_grad()
        by_name = dict(zip(self.names, range(len(self.names))))
        for n, gr in grads.items():
            i = by_name[n]
            self.params[i].grad = gr.to(self.g.device)
        for b in range(len(self.buckets)):
            self._land(b)

    @torch.no_grad()
    def update(self):
        """optimizer.update(grads): clip by global norm, then Adam with lr = schedule(count).  With accum_steps = K > 1 the first K - 1 calls
        of a cycle fold the gradients into the accumulator and return None; the K-th updates with the mean and returns lr."""
        if self.ema_swapped:
            raise RuntimeError("Optimizer.update inside swapped_ema(): the parameters hold the weight average, not the Adam iterate")
        for b in range(len(self.buckets)):
            if not self.landed[b]:
                self._land(b)                    # parameters that received no gradient this step contribute zeros
        if self.micro < self.accum_steps - 1:    # not the cycle's last micro-step: acc (+)= g, no collective, no update
            self._fold(self.acc, self.g, overwrite=self.micro == 0)
            self.micro += 1
            self.last_update = False
            return None
        fused_acc = self.acc is not None and self.reducer is None      # the update itself reads g + acc: no fold pass on the last micro-step
        gscale = 1.0 / self.accum_steps
        if self.reducer is not None:
            if self.defer_reduce:
                if not self.prelaunched:
                    self.reducer.reset()
                for b in range(len(self.buckets)):
                    if b not in self.prelaunched:
                        self.reduce_bucket(b)
                self.prelaunched = set()
            self.reducer.finish()
            gscale = 1.0 / (self.reducer.world_size * self.accum_steps)
        if not self.p.is_cuda:
            raise RuntimeError("Optimizer.update runs the fused HIP clip+Adam kernel and needs GPU parameters")
        s = _stream()
        lr = float(self.schedule(self.count))
        d = ema_decay_at(self.ema_decay, self.count, self.ema_warmup) if self.ema is not None else None
        self.count += 1
        # global norm without atomics: per-workgroup partial sums of squares, folded in one fixed order inside the Adam kernel.  Both passes
        # read g + acc when acc is given; the same Adam pass advances the weight average when there is one (one more read and write per parameter)
        acc = _vp(self.acc if fused_acc else None)
        check(lib().vvae_sqnorm_partials(_vp(self.g), acc, self.numel, _vp(self.gnorm_part), s), "vvae_sqnorm_partials")
        check(lib().vvae_adam_clip_step(_vp(self.p), _vp(self.g), acc, _vp(self.m), _vp(self.v), _vp(self.shadow), self.numel,
                                        _vp(self.gnorm_part), self.gnorm_part.numel(), _vp(self.gnorm_sq), gscale, self.max_norm, lr,
                                        self.b1, self.b2, self.eps, self.count, _vp(self.ema), d if d is not None else 0.0, s),
              "vvae_adam_clip_step")
        if self.ema is not None:
            self.last_ema_decay = d
        ops.transpose_grouped(self.tpairs)
        self.micro = 0
        self.last_lr = lr
        self.last_update = True
        return lr

    def refresh_shadow(self):
        """Re-derive the bf16 shadows after parameters were written from outside (checkpoint load, broadcast)."""
        if self.shadow is not None:
            self.shadow.copy_(self.p)
            ops.transpose_grouped(self.tpairs)

    # ---- weight average ----
    def _swap_ema(self):
        if not self.p.is_cuda:
            raise RuntimeError("swapped_ema() runs the HIP swap kernel and needs GPU parameters")
        check(lib().vvae_swap_refresh_f32(_vp(self.p), _vp(self.ema), _vp(self.shadow), self.numel, _stream()), "vvae_swap_refresh_f32")
        ops.transpose_grouped(self.tpairs)

    @contextlib.contextmanager
    def swapped_ema(self):
        """Evaluate with the averaged weights: inside the block the parameters (and their bf16 shadows) hold the average and ``self.ema``
        the raw weights, exchanged in place by one HIP pass -- no tensor moves, so a captured graph replays the swapped-in values -- and
        exchanged back on exit.  Not re-entrant; ``update()`` inside it raises."""
        if self.ema is None:
            raise RuntimeError("swapped_ema() needs an Optimizer built with ema_decay")
        if self.ema_swapped:
            raise RuntimeError("swapped_ema() is already active: it does not nest")
        self._swap_ema()
        self.ema_swapped = True
        try:
            yield self
        finally:
            self._swap_ema()
            self.ema_swapped = False

    def grad_norm(self):
        """||g|| of the last update (host sync); with accum_steps > 1 the norm of the cycle's mean gradient."""
        scale = 1.0 / ((self.reducer.world_size if self.reducer is not None else 1) * self.accum_steps)
        return float(self.gnorm_sq.item()) ** 0.5 * scale

    # ---- checkpoint state (model_loader.save_checkpoint / load_checkpoint) ----
    def _no_partial_cycle(self, what):
        if self.micro != 0:
            raise RuntimeError(f"Optimizer.{what} with {self.micro} of {self.accum_steps} micro-steps accumulated: finish the cycle or "
                               "reset_accumulation() first (the accumulator is not part of a checkpoint)")

    def state_dict(self):
        self._no_partial_cycle("state_dict")
        out = {"count": self.count}
        for n, p, o in zip(self.names, self.params, self.offsets):
            k = p.numel()
            out[f"mu.{n}"] = self.m[o:o + k].view(p.shape).detach().cpu().clone()
            out[f"nu.{n}"] = self.v[o:o + k].view(p.shape).detach().cpu().clone()
        if self.ema is not None:
            if self.ema_swapped:
                raise RuntimeError("Optimizer.state_dict inside swapped_ema(): parameters and average are exchanged")
            out["ema_decay"] = self.ema_decay
            for n, p, o in zip(self.names, self.params, self.offsets):
                out[f"ema.{n}"] = self.ema[o:o + p.numel()].view(p.shape).detach().cpu().clone()
        return out

    def load_state_dict(self, state):
        self._no_partial_cycle("load_state_dict")
        self.count = int(state["count"])
        for n, p, o in zip(self.names, self.params, self.offsets):
            k = p.numel()
            self.m[o:o + k].copy_(state[f"mu.{n}"].reshape(-1))
            self.v[o:o + k].copy_(state[f"nu.{n}"].reshape(-1))
        if self.ema is not None:                 # (with the average off, a state's ema.* entries are not looked at)
            if self.ema_swapped:
                raise RuntimeError("Optimizer.load_state_dict inside swapped_ema(): parameters and average are exchanged")
            if all(f"ema.{n}" in state for n in self.names):
                for n, p, o in zip(self.names, self.params, self.offsets):
                    self.ema[o:o + p.numel()].copy_(state[f"ema.{n}"].reshape(-1))
            else:
                ops.note_fallback("ema-from-parameters", "the optimizer state holds no weight average (ema.*): the average starts from "
                                                         "the loaded parameters")
                self.ema.copy_(self.p)
        self.refresh_shadow()
