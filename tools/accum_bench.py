"""Gradient accumulation beside the fused clip + Adam update, over a flat buffer of the production model's size.   python tools/accum_bench.py

In one process and from one binary, alternating the variants round by round (every window is WINDOW eager calls between two HIP events; the
kernels are three orders of magnitude longer than a launch, so the queue never runs dry):
  (a) today's update (sqnorm + clip + Adam + bf16 shadow)                    vvae_sqnorm_partials + vvae_adam_clip_step, acc = NULL
  (b) the fold of a cycle's first micro-step, acc = 0 + g                     vvae_grad_fold_f32, overwrite
  (c) the fold of a later micro-step, acc += g                                vvae_grad_fold_f32
  (d) the final fused update on g + acc                                       the same two entries with acc given
  (e) (c) followed by (a): what the last micro-step would cost with a fold pass of its own
Prints the median and the spread of the per-call time over the rounds, and the HBM rate over the bytes each variant has to move."""
import statistics
import sys
sys.path.insert(0, ".")
import torch
from video_vae_amd import optim

N = 170_631_304
WINDOW, ROUNDS = 100, 7


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
    accum = optim.Optimizer(flat_model(), 1e-4, accum_steps=2)
    plain.g.normal_()
    accum.g.copy_(plain.g)
    accum.acc.copy_(plain.g)

    def final():
        accum.micro = 1                                # the last micro-step of a cycle: update() reads g + acc and resets the counter
        accum.update()

    def unfused():
        accum._fold(accum.g, accum.acc)
        plain.update()

    adam = N * (4 * 4 + 3 * 4 + 2) + N * 4              # g p m v in, p m v + bf16 out; + the squared-norm pass over g
    variants = [("a", "update (sqnorm + clip + Adam + shadow)", plain.update, adam),
                ("b", "fold, first micro-step (acc = 0 + g)", lambda: accum._fold(accum.acc, accum.g, overwrite=True), N * 8),
                ("c", "fold, later micro-step (acc += g)", lambda: accum._fold(accum.acc, accum.g), N * 12),
                ("d", "final update fused on g + acc", final, adam + N * 8),
                ("e", "fold pass, then update (a)", unfused, adam + N * 12)]
    times = {k: [] for k, *_ in variants}
    for _, _, f, _ in variants:                        # warm-up: code objects, allocator, clocks
        for _ in range(20):
            f()
        accum.acc.copy_(plain.g)                       # keep the sums finite over thousands of folds
        accum.g.copy_(plain.g)
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for k, _, f, _ in variants:
            times[k].append(window(f))
            accum.acc.copy_(plain.g)
            accum.g.copy_(plain.g)
    print(f"{N / 1e6:.1f} M parameters; {ROUNDS} rounds of {WINDOW} calls per variant, alternating; per call: median [min .. max]", flush=True)
    med = {}
    for k, what, _, nbytes in variants:
        t = times[k]
        med[k] = statistics.median(t)
        print(f"({k}) {what}: {med[k]:.1f} us [{min(t):.1f} .. {max(t):.1f}] = {nbytes / med[k] / 1e6:.2f} TB/s over {nbytes / 1e9:.2f} GB", flush=True)
    print(f"the fused final update costs {med['d'] - med['a']:+.1f} us over today's (d - a); a fold pass of its own would cost "
          f"{med['e'] - med['a']:+.1f} us (e - a); d / e = {med['d'] / med['e']:.3f} (bytes: {(adam + N * 8) / (adam + N * 12):.3f})", flush=True)


if __name__ == "__main__":
    main()
