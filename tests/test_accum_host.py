"""Host side of gradient accumulation (optim.Optimizer(accum_steps=K), train.py --grad-accum K): argument validation, the schedule's batch
factor, the bookkeeping of a cycle on CPU tensors (the folds run as torch.add there; only the Adam launch needs the GPU), the checkpoint
guards, and a gloo world-2 rehearsal of which micro-step communicates and what it sends."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _toy():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.Tanh(), torch.nn.Linear(16, 16), torch.nn.Tanh(), torch.nn.Linear(16, 3))


def _grads(model, seed):
    g = torch.Generator().manual_seed(seed)
    return {n: torch.randn(p.shape, generator=g) for n, p in model.named_parameters()}


@pytest.mark.parametrize("bad", [0, -1, 1.5, 2.0, "2", None, True])
def test_constructor_refuses_anything_but_an_integer_of_at_least_one(bad):
    from video_vae_amd import optim
    with pytest.raises(ValueError):
        optim.Optimizer(_toy(), 1e-3, accum_steps=bad)


def test_one_micro_step_per_update_allocates_no_accumulator():
    from video_vae_amd import optim
    opt = optim.Optimizer(_toy(), 1e-3)
    assert opt.accum_steps == 1 and opt.acc is None and opt.micro == 0 and opt.last_update is False
    opt = optim.Optimizer(_toy(), 1e-3, accum_steps=3)
    assert opt.acc.shape == opt.g.shape and opt.acc.dtype == torch.float32 and opt.acc.data_ptr() != opt.g.data_ptr()


def test_parser_and_driver_validation():
    from video_vae_amd import train
    ap = train.build_parser()
    assert ap.parse_args([]).grad_accum == 1 and ap.parse_args(["--grad-accum", "4"]).grad_accum == 4
    for bad in (["--grad-accum", "1.5"], ["--grad-accum", "two"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    for bad in ("0", "-2"):                                   # refused before the driver touches a GPU
        with pytest.raises(SystemExit):
            train.main(["--grad-accum", bad])


def test_schedule_is_sized_for_batch_times_world_times_accumulation():
    """The reference warms up over 20000 / sqrt(global batch) updates: 16 hosts x 4 clips = 64 -> 2500.  B = 2 on 4 ranks with K = 8 is the
    same 64; K = 1 leaves the schedule what it was."""
    from video_vae_amd import optim, train
    s = train.build_schedule(2, 4, 8)
    ref = optim.reference_schedule(batch_size=64)
    for c in (0, 1, 1250, 2499, 2500, 2501, 500_000, 2_000_000):
        assert s(c) == ref(c)
    assert s(2500) == 2e-5 and s(1250) == 1e-5 and s(2499) < 2e-5 and s(2501) < 2e-5
    one, was = train.build_schedule(2, 1), optim.reference_schedule(batch_size=2)
    assert all(one(c) == was(c) for c in (0, 7071, 14142, 20_000))
    assert train.build_schedule(2, 1, 4)(5000) != one(5000)


def test_cycle_bookkeeping_guards_and_reset_on_cpu_tensors():
    from video_vae_amd import optim
    m = _toy()
    opt = optim.Optimizer(m, 1e-3, bucket_bytes=256, accum_steps=3, ema_decay=0.9)
    state0 = opt.state_dict()                                                # micro == 0: allowed
    p0, m0, v0, e0, sh0 = opt.p.clone(), opt.m.clone(), opt.v.clone(), opt.ema.clone(), opt.shadow.clone()
    g1, g2, g3 = _grads(m, 1), _grads(m, 2), _grads(m, 3)
    opt.set_grads(g1)
    assert opt.update() is None and opt.micro == 1 and opt.last_update is False
    assert torch.equal(opt.acc, opt.g)                                       # the first micro-step overwrites: acc was never zero-filled
    f1 = opt.g.clone()
    opt.set_grads(g2)
    assert opt.update() is None and opt.micro == 2
    assert torch.equal(opt.acc, f1 + opt.g)
    for t, t0 in ((opt.p, p0), (opt.m, m0), (opt.v, v0), (opt.ema, e0), (opt.shadow, sh0)):
        assert torch.equal(t, t0)
    assert opt.count == 0 and not hasattr(opt, "last_lr")
    with pytest.raises(RuntimeError, match="micro-steps accumulated"):
        opt.state_dict()
    with pytest.raises(RuntimeError, match="micro-steps accumulated"):
        opt.load_state_dict(state0)
    opt.reset_accumulation()
    assert opt.micro == 0
    opt.load_state_dict(state0)
    assert set(opt.state_dict()) == set(state0) and not any("acc" in k for k in state0)      # the accumulator is never written out
    opt.set_grads(g3)                                                        # a new cycle after the drop starts a new sum
    assert opt.update() is None and opt.micro == 1 and torch.equal(opt.acc, opt.g)
    opt.set_grads(g1)
    opt.update()
    opt.set_grads(g2)
    with pytest.raises(RuntimeError, match="needs GPU parameters"):          # the K-th micro-step is the fused HIP update
        opt.update()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _accum_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sys.path.insert(0, ROOT)
        from video_vae_amd import optim, ddp
        torch.set_num_threads(1)
        m, twin = _toy(), _toy()
        opt = optim.Optimizer(m, 1e-2, bucket_bytes=256, bf16_shadow=False, accum_steps=2)
        plain = optim.Optimizer(twin, 1e-2, bucket_bytes=256, bf16_shadow=False)        # no reducer: this rank's own gradients
        red = ddp.GradReducer(opt)
        calls = []
        launch = red.launch
        red.launch = lambda b: (calls.append(b), launch(b))[1]
        g = torch.Generator().manual_seed(100 + rank)
        xs = [torch.randn((5, 6), generator=g) for _ in range(2)]
        own = []
        for x in xs:
            plain.zero_grad()
            twin(x).square().mean().backward()
            for b in range(len(plain.buckets)):
                if not plain.landed[b]:
                    plain._land(b)
            own.append(plain.g.clone())
        res = {"nbuckets": len(opt.buckets), "own": own[1] + own[0]}                     # what the last micro-step sends: g + acc
        opt.zero_grad()
        m(xs[0]).square().mean().backward()
        assert opt.update() is None and opt.micro == 1
        res["calls1"] = list(calls)
        res["acc1"] = opt.acc.clone()
        res["own1"] = own[0]
        opt.zero_grad()
        m(xs[1]).square().mean().backward()                # the landing hooks fold and launch bucket by bucket
        for b in range(len(opt.buckets)):
            if not opt.landed[b]:
                opt._land(b)
        res["calls2"] = list(calls)
        red.finish()
        res["reduced"] = opt.g.clone()
        torch.save(res, os.path.join(out, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_gloo_world2_only_the_last_micro_step_communicates(tmp_path):
    """Two ranks, K = 2: a counting wrapper around reducer.launch sees no call on micro-step 1 and one per bucket on micro-step 2; every
    reduced slice is the sum over the ranks of g + acc (two addends per element: one commutative fp32 add, so equality is bitwise)."""
    mp.spawn(_accum_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    for r in (r0, r1):
        assert r["nbuckets"] > 1
        assert r["calls1"] == [] and sorted(r["calls2"]) == list(range(r["nbuckets"]))
        assert torch.equal(r["acc1"], r["own1"])
    assert not torch.equal(r0["own"], r1["own"])
    assert torch.equal(r0["reduced"], r1["reduced"])
    assert torch.equal(r0["reduced"], r0["own"] + r1["own"])
