"""Weight average (EMA) beside the fused clip + Adam update, over a flat buffer of the production model's size.   python tools/ema_bench.py

In one process, alternating the variants round by round (every window is WINDOW eager calls between two HIP events; the kernels are three
orders of magnitude longer than a launch, so the queue never runs dry):
  (a) the update as it was (sqnorm + clip + Adam + bf16 shadow)             vvae_adam_clip_step, ema = NULL
  (b) the update that also advances the average in the same pass           vvae_adam_clip_step with ema given
  (c) (a) followed by the framework's ema.lerp_(p, 1 - d)                   what the average costs outside the kernel
  (d) one swapped_ema() entry plus exit (two vvae_swap_refresh_f32 passes)
Prints the median and the spread of the per-call time over the rounds, and the HBM rate over the bytes each variant has to move."""
import statistics
import sys
sys.path.insert(0, ".")
import torch
from video_vae_amd import optim

N = 170_631_304
WINDOW, ROUNDS, D = 100, 7, 0.999


def flat_model():
    m = torch.nn.Linear(1, 1)
    m.weight = torch.nn.Parameter(torch.randn(N // 4, 4))
    m.bias = None
    return m.cuda()


def window(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(WINDOW):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / WINDOW * 1e3          # us per call


def main():
    plain = optim.Optimizer(flat_model(), 1e-4)
    fused = optim.Optimizer(flat_model(), 1e-4, ema_decay=D)
    plain.g.normal_()
    fused.g.copy_(plain.g)
    side = plain.p.clone()                             # (c)'s average: a framework tensor beside the plain optimizer

    def outside():
        plain.update()
        side.lerp_(plain.p, 1 - D)

    def swap():
        with fused.swapped_ema():
            pass

    adam = N * (4 * 4 + 3 * 4 + 2) + N * 4              # g p m v in, p m v + bf16 out; + the squared-norm pass over g
    variants = [("a", "update (sqnorm + clip + Adam + shadow)", plain.update, adam),
                ("b", "update with the average fused in", fused.update, adam + N * 8),
                ("c", "update, then ema.lerp_(p, 1 - d)", outside, adam + N * 12),
                ("d", "swapped_ema() entry + exit", swap, 2 * N * (8 + 8 + 2))]
    times = {k: [] for k, *_ in variants}
    for _, _, f, _ in variants:                        # warm-up: code objects, allocator, clocks
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for k, _, f, _ in variants:
            times[k].append(window(f))
    print(f"{N / 1e6:.1f} M parameters, d = {D}; {ROUNDS} rounds of {WINDOW} calls per variant, alternating; per call: median [min .. max]", flush=True)
    med = {}
    for k, what, _, nbytes in variants:
        t = times[k]
        med[k] = statistics.median(t)
        print(f"({k}) {what}: {med[k]:.1f} us [{min(t):.1f} .. {max(t):.1f}] = {nbytes / med[k] / 1e6:.2f} TB/s over {nbytes / 1e9:.2f} GB", flush=True)
    print(f"the average costs {med['b'] - med['a']:+.1f} us fused (b - a) and {med['c'] - med['a']:+.1f} us outside (c - a); "
          f"b / c = {med['b'] / med['c']:.3f} (bytes: {(adam + N * 8) / (adam + N * 12):.3f})", flush=True)


if __name__ == "__main__":
    main()
