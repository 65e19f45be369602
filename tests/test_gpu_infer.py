"""GPU: the inference path -- the fused eval heads (vvae_encoder_head_eval_fwd) against the oracle, encode / decode / reconstruct of the tiny fp32
VAE against oracle.model (train=False), replayed hipGraphs against eager, InferenceWeights, the reference's batch-isolation and masking
properties (train/human_tests.py:62-93), the production shape, and the command line end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.utils._python_dispatch

from oracle import model as OM
from oracle import loss as OLoss
from oracle.unet import sub
from test_gpu_parity_r2 import BF16_FACTOR, BF16_FLOOR, rel_l2
from util import assert_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(height=32, width=32, channels=3, patch_size=8, encoder_depth=1, decoder_depth=1, mlp_dim=64, num_heads=4,
            qkv_features=32, max_temporal_len=8, spatial_compression_rate=4, unembedding_upsample_rate=4)
SMALL = 64          # the --small model of the driver at 64 x 64 frames: hw = 16, ld = 96 (the bf16 path with the fused heads)


def _small(flavour="model", seed=2):
    from video_vae_amd.infer import model_config
    import video_vae_amd as V
    from video_vae_amd import rl_model
    cls = rl_model.VideoVAE if flavour == "rl" else V.VideoVAE
    return cls(rngs=V.Rngs(seed), **model_config(SMALL, True))


def _video(b, t, seed, size=SMALL, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((b, t, size, size, 3), generator=g).to(dev)


# --------------------------------------------------------------------------------------------- 1. the eval heads vs the oracle
CASES = [("model", False), ("rl", True), ("rl", False)]


@pytest.mark.parametrize("b,t,hw,ld", [(2, 3, 16, 96), (1, 4, 256, 96), (2, 16, 256, 192)])
def test_eval_head_vs_oracle(dev, b, t, hw, ld):
    """ops.encoder_head_eval (bf16) vs oracle.model.encoder_heads(train=False) + latent_gate with z = mean, fp32 (``ref``) and bf16-emulated
    (``emu``), through selector kernels as in test_gpu_fused_vs_oracle.test_encoder_head_vs_oracle.  Every oracle logit is >= 0.05 from 0;
    identical selections; log_variance / comp within 3 x the emulation's error + 2e-3.  One frame is masked (padding: dropped)."""
    from video_vae_amd import ops
    bf = torch.bfloat16
    eye = torch.eye(ld)
    for seed in range(200):                      # inputs whose logits all sit away from the threshold, with kept and dropped frames
        g = torch.Generator().manual_seed(1000 * hw + 10 * b + seed)
        mean_in = (torch.randn(b, t, hw, ld, generator=g) * 0.5).to(bf).float()
        v_in = (torch.randn(b, t, hw, ld, generator=g) * 1.5).to(bf).float()
        p = {"spatial_compression.kernel": torch.cat([eye, torch.zeros(ld, ld)]), "spatial_compression.bias": torch.zeros(ld),
             "variance_estimator.kernel": torch.cat([torch.zeros(ld, ld), eye]), "variance_estimator.bias": torch.zeros(ld),
             "selection_layer1.kernel": torch.randn(ld, 1, generator=g) * 2 * ld ** -0.5, "selection_layer1.bias": torch.randn(1, generator=g) * 0.1,
             "selection_layer2.kernel": torch.randn(hw, 1, generator=g) * 2 * hw ** -0.5, "selection_layer2.bias": torch.randn(1, generator=g) - 1}
        si = mean_in @ p["selection_layer1.kernel"] + p["selection_layer1.bias"]
        logits = (si[..., 0] @ p["selection_layer2.kernel"])[..., 0] + p["selection_layer2.bias"] + 1
        if float(logits.abs().min()) >= 0.05 and bool((logits > 0).any()) and bool((logits < 0).any()):
            break
    else:
        pytest.fail("no input with every logit 0.05 away from 0")
    assert float(logits.abs().min()) >= 0.05
    fill = torch.randn(1, 1, 1, ld, generator=g) * 0.02
    mask = torch.ones(b, t)
    mask[-1, -1] = 0.0
    x = torch.cat([mean_in, v_in], dim=-1)
    D = {k: v.to(dev) for k, v in p.items()}
    md, vd = mean_in.to(dev, bf), v_in.to(dev, bf)
    assert ops.encoder_head_eval_ok(md, D["selection_layer1.kernel"], D["selection_layer1.bias"], D["selection_layer2.kernel"],
                                    D["selection_layer2.bias"], fill.to(dev))
    for flavour, with_u in CASES:
        u = None
        out = {}
        for dt in (torch.float32, bf):
            mean, lv, sel = OM.encoder_heads(p, x, None, False, flavour, dt)
            if flavour == "rl":
                prob = sel.reshape(b, t)
                if u is None and with_u:
                    u = torch.rand(b, t, generator=g)
                    u = torch.where((u - prob).abs() < 0.02, torch.where(prob > 0.5, prob - 0.05, prob + 0.05), u)
                s = (u < prob).float() if with_u else torch.round(prob)
            else:
                s = sel.reshape(b, t)
            s = s * mask
            out[dt] = (lv, OM.latent_gate(fill, s.reshape(b, t, 1, 1), mean), s)
        (lv_r, comp_r, s_r), (lv_e, comp_e, s_e) = out[torch.float32], out[bf]
        assert torch.equal(s_r, s_e)
        assert 0 < float(s_r.sum()) < b * t, (flavour, s_r)
        lv_g, comp_g, s_g, prob_g = ops.encoder_head_eval(md, vd, D["selection_layer1.kernel"], D["selection_layer1.bias"], D["selection_layer2.kernel"],
                                                          D["selection_layer2.bias"], fill.to(dev), None if u is None else u.to(dev), mask.to(dev),
                                                          flavour == "rl")
        what = f"{flavour}{' u' if with_u else ''}"
        assert torch.equal(s_g.cpu(), s_r), (what, s_g.cpu(), s_r)
        assert (prob_g is None) == (flavour == "model")
        assert comp_g.dtype == bf and lv_g.dtype == bf
        for name, got, emu, ref in (("log_variance", lv_g, lv_e, lv_r), ("comp", comp_g, comp_e, comp_r)):
            e_got, e_emu = rel_l2(got, ref), rel_l2(emu, ref)
            assert e_got <= BF16_FACTOR * e_emu + BF16_FLOOR, f"{what} {name}: gpu {e_got:.3e}, emulated oracle {e_emu:.3e}"
        lv_none, comp_none, s_none, _ = ops.encoder_head_eval(md, None, D["selection_layer1.kernel"], D["selection_layer1.bias"],
                                                              D["selection_layer2.kernel"], D["selection_layer2.bias"], fill.to(dev),
                                                              None if u is None else u.to(dev), mask.to(dev), flavour == "rl")
        assert lv_none is None and torch.equal(comp_none, comp_g) and torch.equal(s_none, s_g)


# --------------------------------------------------------------------------------------------- 2. tiny fp32 VAE vs oracle.model
def _load(module, params, dev):
    sd = module.state_dict()
    with torch.no_grad():
        for k, v in params.items():
            sd[k].copy_(v)
    return module.to(dev)


@pytest.mark.parametrize("flavour", ["model", "rl"])
def test_tiny_encode_decode_reconstruct_fp32_vs_oracle(dev, flavour):
    """encode / decode / reconstruct of the tiny fp32 VAE vs the oracle composed with train=False and z = mean; rl: un-doubled, the injected
    uniforms as the Bernoulli draws (kept 0.02 away from the probabilities).  Masked frames are dropped on both sides."""
    import video_vae_amd as V
    from video_vae_amd import rl_model
    cfg = OM.VAEConfig(**TINY)
    p = OM.init_video_vae(cfg, seed=3, zero_final=False)
    b, t = 2, 8
    video = torch.rand((b, t, 32, 32, 3), generator=torch.Generator().manual_seed(0))
    mask = torch.ones(b, t)
    mask[1, 6:] = 0
    emask = OLoss.expand_mask(mask.bool(), cfg.hw)
    with torch.no_grad():
        mean, lv, sel = OM.encoder(sub(p, "encoder"), cfg, video, emask, None, False, flavour)
        prob = None
        if flavour == "rl":
            prob = sel.reshape(b, t)
            u = torch.rand(b, t, generator=torch.Generator().manual_seed(9))
            u = torch.where((u - prob).abs() < 0.02, torch.where(prob > 0.5, prob - 0.05, prob + 0.05), u)
            u[0, :2] = torch.tensor([0.0, 0.9999])
            s = (u < prob).float()
        else:
            s = sel.reshape(b, t)
        s = s * mask
        comp = OM.latent_gate(p["fill_token"], s.reshape(b, t, 1, 1), mean)
        recon = OM.decoder(sub(p, "decoder"), cfg, comp, emask)
    cls = rl_model.VideoVAE if flavour == "rl" else V.VideoVAE
    m = _load(cls(rngs=V.Rngs(2), dtype=torch.float32, **TINY), p, dev)
    rngs = None
    if flavour == "rl":
        rngs = V.Rngs(3)
        rngs.inject("bernoulli_u", u.reshape(b, t, 1, 1))
    vg, mg = video.to(dev), mask.to(dev)
    lat = m.encode(vg, mg, rngs)
    assert torch.equal(lat.selection.cpu(), s)
    if flavour == "rl":
        assert_close(lat.probability, prob, what="probability")
    else:
        assert lat.probability is None
    assert_close(lat.mean, mean, what="mean")
    assert_close(lat.log_variance, lv, what="log_variance")
    assert_close(lat.compressed_representation, comp, what="compressed_representation")
    assert_close(m.decode(comp.to(dev), mg), recon, what="decode")
    assert_close(m.reconstruct(vg, mg, rngs), recon, what="reconstruct")
    assert m.encode(vg, emask.to(dev), rngs).selection.equal(lat.selection)       # the (b*hw, 1, 1, t) mask form forward takes


# --------------------------------------------------------------------------------------------- 3. graph replay vs eager
class _OpLog(torch.utils._python_dispatch.TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.ops.append(func.overloadpacket.__name__)
        return func(*args, **(kwargs or {}))


NO_KERNEL = {"empty", "empty_strided", "empty_like", "view", "reshape", "_reshape_alias", "_unsafe_view", "detach", "alias", "select", "slice",
             "as_strided", "t", "transpose", "unsqueeze", "squeeze", "expand", "permute", "lift_fresh"}


def test_graph_replay_bitwise_equals_eager(dev):
    """GraphedInference encode / decode / reconstruct (model flavour) and rl encode with explicit noise: two different batches replayed in
    turn, each bitwise equal to the eager call; no memset node in any graph; the eval heads are ONE launch and no framework kernel runs
    between the encoder's last product and the decoder's first."""
    import video_vae_amd as V
    from video_vae_amd import ops
    from video_vae_amd.infer import GraphedInference, InferenceWeights
    b, t = 2, 8
    torch.manual_seed(0)
    m = _small("model").to(dev)
    w = InferenceWeights(m)
    x = [_video(b, t, s) for s in (1, 2)]
    mk = [torch.ones(b, t, device=dev), torch.ones(b, t, device=dev)]
    mk[1][1, 5:] = 0
    comp = [m.encode(xi, mi).compressed_representation.clone() for xi, mi in zip(x, mk)]
    for mode in ("encode", "decode", "reconstruct"):
        gi = GraphedInference(m, w, b, t, mode)
        assert gi.census is not None and gi.census.get("memset", 0) == 0, gi.census
        got = []
        for i in range(2):
            out = gi(comp[i] if mode == "decode" else x[i], mk[i])
            got.append([o.clone() for o in out if o is not None] if mode == "encode" else [out.clone()])
        for i in range(2):
            if mode == "encode":
                want = [o for o in m.encode(x[i], mk[i]) if o is not None]
            elif mode == "decode":
                want = [m.decode(comp[i], mk[i])]
            else:
                want = [m.reconstruct(x[i], mk[i])]
            for a, e in zip(got[i], want):
                assert torch.equal(a, e), (mode, i)
        del gi
    # rl flavour with rngs: the noise override of the replay vs the same uniforms injected into the eager call
    r = _small("rl", seed=4).to(dev)
    wr = InferenceWeights(r)
    gi = GraphedInference(r, wr, b, t, "encode", rngs=V.Rngs(5))
    assert set(gi.noise) == {"bernoulli_u"}
    for i in range(2):
        u = torch.rand((b, t, 1, 1), generator=torch.Generator().manual_seed(20 + i)).to(dev)
        lat = gi(x[i], mk[i], noise={"bernoulli_u": u})
        rg = V.Rngs(0)
        rg.inject("bernoulli_u", u)
        want = r.encode(x[i], mk[i], rg)
        assert torch.equal(lat.selection, want.selection) and torch.equal(lat.probability, want.probability)
        assert torch.equal(lat.compressed_representation, want.compressed_representation)
        assert torch.equal(lat.selection, ((u.reshape(b, t) < want.probability).float() * mk[i]))
    # one fused launch between the two products (eager: the same sequence the graph holds)
    calls = []
    real = ops.encoder_head_eval

    def spy(*a, **k):
        calls.append(1)
        log.ops.append("<encoder_head_eval>")
        return real(*a, **k)
    ops.encoder_head_eval = spy
    try:
        with _OpLog() as log:
            m.reconstruct(x[0], mk[0])
    finally:
        ops.encoder_head_eval = real
    assert len(calls) == 1
    i = log.ops.index("<encoder_head_eval>")
    before = max(j for j in range(i) if log.ops[j] in ("addmm", "mm"))
    after = min(j for j in range(i + 1, len(log.ops)) if log.ops[j] in ("addmm", "mm"))
    between = [o for o in log.ops[before + 1:after] if o != "<encoder_head_eval>"]
    assert all(o in NO_KERNEL for o in between), between


# --------------------------------------------------------------------------------------------- 4. InferenceWeights
def test_inference_weights_routes_and_refresh(dev, tmp_path):
    """With the shadows (own product routes) vs without (per-call casts, library products): equal selections, the rest within the bf16 bar.
    After load_checkpoint(model, None, path) + refresh(), a graph captured before replays the new weights' eager outputs bitwise."""
    import video_vae_amd as V
    from video_vae_amd.infer import GraphedInference, InferenceWeights
    b, t = 2, 8
    plain = _small("model", seed=7).to(dev)
    shad = _small("model", seed=7).to(dev)
    w = InferenceWeights(shad)
    assert not w.shared and w.shadow.data_ptr() % 16 == 0 and all(p.bf16.data_ptr() % 16 == 0 for p in w.params)
    assert any(getattr(p, "bf16_t", None) is not None for p in w.params)
    assert all(getattr(p, "bf16", None) is None for p in plain.parameters())
    x, mk = _video(b, t, 3), torch.ones(b, t, device=dev)
    from video_vae_amd import ops
    real, calls = ops.gemm_nt, []

    def spy(*args, **kw):
        calls.append(1)
        return real(*args, **kw)
    ops.gemm_nt = spy
    try:
        a = plain.encode(x, mk)
        n_plain = len(calls)
        e = shad.encode(x, mk)
    finally:
        ops.gemm_nt = real
    assert n_plain == 0 and len(calls) > 0, (n_plain, len(calls))      # the shadows put products on the own GEMM
    assert torch.equal(a.selection, e.selection)
    for name in ("mean", "log_variance", "compressed_representation"):
        err = rel_l2(getattr(e, name), getattr(a, name))
        print(f"encode {name} with vs without the shadows: rel l2 {err:.3e}")
        assert err <= 2e-2, (name, err)
    err = rel_l2(shad.reconstruct(x, mk), plain.reconstruct(x, mk))
    print(f"reconstruct with vs without the shadows: rel l2 {err:.3e}")
    assert err <= 3e-2
    gi = GraphedInference(shad, w, b, t, "reconstruct")
    first = gi(x, mk).clone()
    other = _small("model", seed=11)
    V.save_checkpoint(other, None, str(tmp_path))
    V.load_checkpoint(shad, None, str(tmp_path))
    w.refresh()
    again = gi(x, mk).clone()
    assert not torch.equal(again, first)
    assert torch.equal(again, shad.reconstruct(x, mk))


# --------------------------------------------------------------------------------------------- 5. reference properties
def test_batch_isolation_and_masked_equals_truncated(dev):
    """train/human_tests.py:62-93 at the small config, atol 1e-1 as there: encoding clip 0 alone matches row 0 of the batch; an 11-frame clip
    with frame 10 masked reconstructs frames 0-9 as the 10-frame clip does."""
    from video_vae_amd.infer import InferenceWeights
    m = _small("model", seed=8).to(dev)
    InferenceWeights(m)
    x = _video(3, 8, 4)
    mk = torch.ones(3, 8, device=dev)
    full = m.encode(x, mk)
    one = m.encode(x[:1], mk[:1])
    d = float((full.mean[:1].float() - one.mean.float()).abs().max())
    print(f"batch isolation: max |diff| of the mean {d:.3e}")
    assert d <= 1e-1 and torch.equal(full.selection[:1], one.selection)
    x11 = _video(1, 11, 5)
    m11 = torch.ones(1, 11, device=dev)
    m11[0, 10] = 0
    r11 = m.reconstruct(x11, m11)
    r10 = m.reconstruct(x11[:, :10].contiguous(), torch.ones(1, 10, device=dev))
    d = float((r11[:, :10].float() - r10.float()).abs().max())
    print(f"masked vs truncated: max |diff| of frames 0-9 {d:.3e}")
    assert d <= 1e-1


# --------------------------------------------------------------------------------------------- 6. production shape
def test_c3_replayed_reconstruct(dev):
    """B=4, T=16, 256 x 256, full depth, model flavour: the replayed reconstruct is finite, bitwise the eager one, holds no memset node, and
    the peak allocation stays under 8 GB."""
    from video_vae_amd.infer import GraphedInference, InferenceWeights, model_config
    import video_vae_amd as V
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    m = V.VideoVAE(rngs=V.Rngs(2), **model_config(256, False)).to(dev)
    w = InferenceWeights(m)
    x = _video(4, 16, 6, size=256)
    mk = torch.ones(4, 16, device=dev)
    mk[3, 12:] = 0
    gi = GraphedInference(m, w, 4, 16, "reconstruct")
    assert gi.census.get("memset", 0) == 0, gi.census
    got = gi(x, mk).clone()
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, m.reconstruct(x, mk))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"C3 replayed reconstruct: peak allocated {peak / 2 ** 30:.2f} GiB, graph nodes {gi.census}")
    assert peak < 8e9


# --------------------------------------------------------------------------------------------- 7. command line
def test_cli_encode_decode_end_to_end(dev, tmp_path):
    """infer encode / decode on synthetic clips (--small, rl flavour, --threshold): latent files and decoded frames of the right shapes; the
    decoded frames are bitwise what an in-process replayed reconstruct of the same windows gives."""
    import video_vae_amd as V
    from video_vae_amd import data as D
    from video_vae_amd.infer import GraphedInference, InferenceWeights, centre_square, windows
    D.write_synthetic_clips(str(tmp_path / "data"), 2, 10, 40, 48, seed=1)          # clip 0: 8 frames, clip 1: 10 frames
    model = _small("rl", seed=9)
    V.save_checkpoint(model, None, str(tmp_path / "ckpt"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--model_path", str(tmp_path / "ckpt"), "--batch", "2"]
    enc = ["timeout", "-k", "10", "120", sys.executable, "-m", "video_vae_amd.infer", "encode", "--data", str(tmp_path / "data"), "--out",
           str(tmp_path / "lat"), "--size", str(SMALL), "--frames", "4", "--small", "--threshold"] + common
    r = subprocess.run(enc, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    dec = ["timeout", "-k", "10", "120", sys.executable, "-m", "video_vae_amd.infer", "decode", "--latents", str(tmp_path / "lat"), "--out",
           str(tmp_path / "rec")] + common
    r = subprocess.run(dec, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    m = model.to(dev)
    w = InferenceWeights(m)
    gi = GraphedInference(m, w, 2, 4, "reconstruct")
    for name, n in (("clip0000", 8), ("clip0001", 10)):
        with np.load(tmp_path / "lat" / f"{name}.npz") as z:
            assert int(z["n_frames"]) == n and z["selection"].shape == (n,) and z["selection"].dtype == np.uint8
            assert z["mean"].shape == (int(z["selection"].sum()), 16, 96) and z["mean"].dtype == np.float32
        with np.load(tmp_path / "rec" / f"{name}.npz") as z:
            frames = z["frames"]
        assert frames.shape == (n, SMALL, SMALL, 3) and frames.dtype == np.uint8
        clip = centre_square(np.load(tmp_path / "data" / "videos0" / f"{name}.npy"), SMALL)
        wins = []
        for s, c in windows(n, 4):
            v = np.zeros((4, SMALL, SMALL, 3), dtype=np.uint8)
            v[:c] = clip[s:s + c]
            mk = np.zeros(4, dtype=np.float32)
            mk[:c] = 1
            wins.append((v, mk, c))
        recon = []
        for i in range(0, len(wins), 2):
            grp = wins[i:i + 2]
            real = len(grp)
            grp = grp + [grp[-1]] * (2 - real)
            out = gi(torch.from_numpy(np.stack([g[0] for g in grp])).to(dev).float() / 255.0, torch.from_numpy(np.stack([g[1] for g in grp])).to(dev))
            recon += [out[j, :grp[j][2]].float().cpu() for j in range(real)]
        want = (np.clip(torch.cat(recon).numpy(), 0, 1) * 255).astype(np.uint8)
        assert np.array_equal(frames, want), name
