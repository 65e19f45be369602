"""CPU: host logic of the weight average (EMA) -- the decay ramp, the optimizer's state keys, the checkpoint round trip,
load_ema_weights, the swapped_ema() guards, the drivers' flags and the world_size=2 gloo broadcast.  No HIP compute is called here."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _toy(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.Tanh(), torch.nn.Linear(16, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))


def _opt(model, **kw):
    from video_vae_amd import optim
    return optim.Optimizer(model, 1e-2, bucket_bytes=256, bf16_shadow=False, **kw)


def test_ema_decay_at_values():
    from video_vae_amd.optim import ema_decay_at
    assert ema_decay_at(0.999, 0, True) == 1 / 10
    assert ema_decay_at(0.999, 1, True) == 2 / 11
    assert ema_decay_at(0.999, 90, True) == 91 / 100
    assert ema_decay_at(0.9, 90, True) == 0.9                       # the cap: (1 + 90) / (10 + 90) = 0.91 > 0.9
    assert ema_decay_at(0.9, 80, True) == 0.9 and ema_decay_at(0.9, 79, True) == 80 / 89
    assert ema_decay_at(0.999, 10 ** 9, True) == 0.999
    for n in (0, 1, 90, 10 ** 6):
        assert ema_decay_at(0.999, n, False) == 0.999
    ramp = [ema_decay_at(0.999, n, True) for n in range(200)]
    assert all(a < b for a, b in zip(ramp, ramp[1:]))               # strictly rising until the cap


def test_state_keys_with_and_without_ema():
    m = _toy()
    opt = _opt(m, ema_decay=0.99)
    assert opt.ema is not None and opt.ema.dtype == torch.float32 and opt.ema.shape == opt.p.shape
    assert torch.equal(opt.ema, opt.p) and opt.ema.data_ptr() != opt.p.data_ptr()
    for p, o in zip(opt.params, opt.offsets):
        assert p.ema.shape == p.shape and p.ema.data_ptr() == opt.ema[o:].data_ptr()       # same offsets as the parameter views
        assert torch.equal(p.ema, p.data)
    sd = opt.state_dict()
    names = [n for n, _ in m.named_parameters()]
    assert set(sd) == {"count", "ema_decay"} | {f"{k}.{n}" for k in ("mu", "nu", "ema") for n in names}
    assert sd["ema_decay"] == 0.99
    plain = _opt(_toy())
    assert plain.ema is None and not hasattr(plain.params[0], "ema")
    assert set(plain.state_dict()) == {"count"} | {f"{k}.{n}" for k in ("mu", "nu") for n in names}      # exactly today's keys
    with pytest.raises(ValueError):
        _opt(_toy(), ema_decay=1.0)
    with pytest.raises(ValueError):
        _opt(_toy(), ema_decay=-0.1)


def _perturb(opt, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        opt.p.add_(torch.randn(opt.p.shape, generator=g) * 0.1)
        opt.m.copy_(torch.randn(opt.m.shape, generator=g))
        opt.v.copy_(torch.rand(opt.v.shape, generator=g))
        if opt.ema is not None:
            opt.ema.copy_(torch.randn(opt.ema.shape, generator=g))
    opt.count = 7


def _live(opt, t):
    """The entries of a flat buffer that belong to parameters (slots are padded to 4 floats)."""
    return torch.cat([t[o:o + p.numel()] for p, o in zip(opt.params, opt.offsets)])


def test_checkpoint_round_trip(tmp_path, capfd):
    import video_vae_amd as V
    m0 = _toy()
    o0 = _opt(m0, ema_decay=0.99)
    _perturb(o0, 1)
    V.save_checkpoint(m0, o0, str(tmp_path / "ema"))
    # -> a fresh EMA optimizer: the average comes back bitwise, next to parameters, moments and count
    m1 = _toy(5)
    o1 = _opt(m1, ema_decay=0.99)
    V.load_checkpoint(m1, o1, str(tmp_path / "ema"))
    assert o1.count == 7
    for a, b in ((o0.ema, o1.ema), (o0.p, o1.p), (o0.m, o1.m), (o0.v, o1.v)):
        assert torch.equal(_live(o0, a), _live(o1, b))
    assert not torch.equal(o1.ema, o1.p)
    # -> a plain optimizer: works, the ema.* entries are not looked at
    m2 = _toy(6)
    o2 = _opt(m2)
    V.load_checkpoint(m2, o2, str(tmp_path / "ema"))
    assert o2.ema is None and o2.count == 7 and torch.equal(_live(o2, o2.p), _live(o0, o0.p))
    # an EMA-less checkpoint -> an EMA optimizer: the average starts at the loaded parameters, and that is said
    m3 = _toy(7)
    o3 = _opt(m3)
    _perturb(o3, 2)
    V.save_checkpoint(m3, o3, str(tmp_path / "plain"))
    state = torch.load(tmp_path / "plain" / "checkpoint.pt", weights_only=True)
    assert not any(k.startswith("ema") for k in state["optimizer"])
    m4 = _toy(8)
    o4 = _opt(m4, ema_decay=0.5)
    with torch.no_grad():
        o4.ema.fill_(123.0)
    capfd.readouterr()
    V.load_checkpoint(m4, o4, str(tmp_path / "plain"))
    assert torch.equal(_live(o4, o4.p), _live(o3, o3.p)) and torch.equal(o4.ema, o4.p)
    assert "average starts from the loaded parameters" in capfd.readouterr().err
    V.load_checkpoint(m4, o4, str(tmp_path / "plain"))
    assert "average starts" not in capfd.readouterr().err           # once per process


def test_load_ema_weights_in_place(tmp_path):
    import video_vae_amd as V
    from video_vae_amd.model_loader import load_ema_weights
    assert V.load_ema_weights is load_ema_weights
    m0 = _toy()
    o0 = _opt(m0, ema_decay=0.99)
    _perturb(o0, 3)
    V.save_checkpoint(m0, o0, str(tmp_path / "ema"))
    m1 = _toy(9)
    V.load_checkpoint(m1, None, str(tmp_path / "ema"))
    ptrs = [p.data_ptr() for p in m1.parameters()]
    raw = {n: p.detach().clone() for n, p in m1.named_parameters()}
    V.load_ema_weights(m1, str(tmp_path / "ema"))
    assert [p.data_ptr() for p in m1.parameters()] == ptrs          # copied in place
    for (n, p), (n0, p0) in zip(m1.named_parameters(), m0.named_parameters()):
        assert n == n0 and torch.equal(p.data, p0.ema) and not torch.equal(p.data, raw[n])
    m2 = _toy()
    o2 = _opt(m2)
    V.save_checkpoint(m2, o2, str(tmp_path / "plain"))
    with pytest.raises(KeyError, match="no weight average"):
        V.load_ema_weights(m1, str(tmp_path / "plain"))
    V.save_checkpoint(m2, None, str(tmp_path / "bare"))             # a model-only checkpoint has no optimizer entry at all
    with pytest.raises(KeyError, match="no weight average"):
        V.load_ema_weights(m1, str(tmp_path / "bare"))


def test_swapped_ema_guards():
    """Nesting and update() inside the block are refused before any kernel is called; so is swapped_ema() without an average."""
    opt = _opt(_toy(), ema_decay=0.9)
    calls = []
    opt._swap_ema = lambda: calls.append(1)                          # the HIP swap itself needs a GPU (tests/test_gpu_ema.py)
    with opt.swapped_ema():
        assert opt.ema_swapped and len(calls) == 1
        with pytest.raises(RuntimeError, match="nest"):
            with opt.swapped_ema():
                pass
        assert opt.ema_swapped and len(calls) == 1                   # the refused entry did not swap anything back
        count = opt.count
        with pytest.raises(RuntimeError, match="swapped_ema"):
            opt.update()
        assert opt.count == count
        with pytest.raises(RuntimeError, match="swapped_ema"):
            opt.state_dict()
    assert not opt.ema_swapped and len(calls) == 2
    with pytest.raises(ZeroDivisionError):                           # an exception inside the block still swaps back
        with opt.swapped_ema():
            1 / 0
    assert not opt.ema_swapped and len(calls) == 4
    with pytest.raises(RuntimeError, match="ema_decay"):
        with _opt(_toy()).swapped_ema():
            pass
    with pytest.raises(RuntimeError, match="GPU"):                   # no CPU stand-in for the swap
        with _opt(_toy(), ema_decay=0.9).swapped_ema():
            pass


def test_driver_flags():
    from video_vae_amd import infer, train
    a = train.build_parser().parse_args([])
    assert a.ema is None and a.ema_warmup is False and a.eval_ema is False          # off by default
    a = train.build_parser().parse_args(["--ema", "0.999", "--ema-warmup", "--eval-ema", "--eval_steps", "2"])
    assert a.ema == 0.999 and a.ema_warmup and a.eval_ema
    ap = infer.build_parser()
    for cmd in (["encode", "--model_path", "ck", "--data", "d", "--out", "o"], ["eval", "--model_path", "ck", "--data", "d"],
                ["decode", "--model_path", "ck", "--latents", "l", "--out", "o"]):
        assert ap.parse_args(cmd).ema is False
        assert ap.parse_args(cmd + ["--ema"]).ema is True


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _broadcast_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sys.path.insert(0, ROOT)
        from video_vae_amd import ddp
        torch.set_num_threads(1)
        opt = _opt(_toy(100 + rank), ema_decay=0.99)                  # replicas start different, averages included
        _perturb(opt, 10 + rank)
        opt.count = 3 + rank
        red = ddp.GradReducer(opt)
        before = opt.ema.clone()
        red.broadcast_state(0)
        torch.save({"ema": opt.ema.clone(), "p": opt.p.clone(), "count": opt.count, "before": before}, os.path.join(out, f"r{rank}.pt"))
        plain = _opt(_toy(rank))                                      # without an average the broadcast is what it was
        ddp.GradReducer(plain).broadcast_state(0)
        assert plain.ema is None
    finally:
        dist.destroy_process_group()


def test_broadcast_state_carries_the_average(tmp_path):
    mp.spawn(_broadcast_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    assert not torch.equal(r0["before"], r1["before"])
    assert torch.equal(r0["ema"], r0["before"])                       # rank 0's average is the source
    assert torch.equal(r1["ema"], r0["ema"]) and torch.equal(r1["p"], r0["p"]) and r1["count"] == r0["count"] == 3
    assert not torch.equal(r0["ema"], r0["p"])
