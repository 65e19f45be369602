"""CPU: the inference surface (ABI entry of the eval heads, encode / decode / reconstruct on both flavours, model-only checkpoint
loading, the latent file format and the command line).  No HIP compute runs here."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(height=32, width=32, channels=3, patch_size=8, encoder_depth=1, decoder_depth=1, mlp_dim=64, num_heads=4,
            qkv_features=32, max_temporal_len=8, spatial_compression_rate=4, unembedding_upsample_rate=4)


def test_eval_head_entry_declared_and_exported():
    from video_vae_amd._lib import parse_header, LIB_PATH
    protos = parse_header()
    assert "vvae_encoder_head_eval_fwd" in protos
    ret, args = protos["vvae_encoder_head_eval_fwd"]
    assert ret is ctypes.c_int and len(args) == 20
    assert hasattr(ctypes.CDLL(LIB_PATH), "vvae_encoder_head_eval_fwd")


def test_both_flavours_have_the_inference_methods():
    import video_vae_amd as V
    from video_vae_amd import rl_model
    for cls in (V.VideoVAE, rl_model.VideoVAE):
        for name in ("encode", "decode", "reconstruct"):
            assert callable(getattr(cls, name, None)), (cls, name)


def test_load_checkpoint_without_optimizer(tmp_path):
    import video_vae_amd as V
    from video_vae_amd import optim
    src = V.VideoVAE(rngs=V.Rngs(5), dtype=torch.float32, **TINY)
    opt = optim.Optimizer(src, 1e-3, bf16_shadow=False)
    with torch.no_grad():
        for p in src.parameters():
            p.add_(0.25)
    V.save_checkpoint(src, opt, str(tmp_path))
    dst = V.VideoVAE(rngs=V.Rngs(6), dtype=torch.float32, **TINY)
    assert any(not torch.equal(a, b) for a, b in zip(src.state_dict().values(), dst.state_dict().values()))
    V.load_checkpoint(dst, None, str(tmp_path))
    ref = src.state_dict()
    for k, v in dst.state_dict().items():
        assert torch.equal(v, ref[k]), k


def test_latent_pack_unpack_round_trip():
    from video_vae_amd.infer import pack_latents, unpack_latents
    g = torch.Generator().manual_seed(0)
    n, hw, ld = 7, 4, 8
    fill = torch.randn(1, 1, 1, ld, generator=g)
    mean = torch.randn(n, hw, ld, generator=g).to(torch.bfloat16)
    lv = torch.randn(n, hw, ld, generator=g).to(torch.bfloat16)
    sel = torch.tensor([1, 0, 0, 1, 1, 0, 1], dtype=torch.float32)
    arrays = pack_latents(mean, sel, lv)
    assert arrays["mean"].dtype == np.float32 and arrays["mean"].shape == (4, hw, ld)
    assert arrays["selection"].dtype == np.uint8 and arrays["selection"].tolist() == [1, 0, 0, 1, 1, 0, 1]
    assert int(arrays["n_frames"]) == n and arrays["log_variance"].shape == (4, hw, ld)
    comp, s = unpack_latents(arrays, fill)
    dense = fill * (1 - sel.view(n, 1, 1)) + mean.float() * sel.view(n, 1, 1)      # the latent gate with z = mean
    assert torch.equal(torch.from_numpy(comp), dense.reshape(n, hw, ld))
    assert torch.equal(torch.from_numpy(comp).to(torch.bfloat16)[sel != 0], mean[sel != 0])       # lossless from bf16
    none = pack_latents(mean, torch.zeros(n))
    comp0, _ = unpack_latents(none, fill)
    assert comp0.shape == (n, hw, ld) and np.all(comp0 == fill.numpy().reshape(1, 1, ld))


def test_windows_cover_a_clip():
    from video_vae_amd.infer import windows
    assert windows(16, 16) == [(0, 16)]
    assert windows(37, 16) == [(0, 16), (16, 16), (32, 5)]
    assert windows(3, 16) == [(0, 3)]


def test_infer_cli_help():
    env = dict(os.environ, PYTHONPATH=ROOT)
    for sub in ([], ["encode"], ["decode"]):
        out = subprocess.run([sys.executable, "-m", "video_vae_amd.infer"] + sub + ["--help"], cwd=ROOT, env=env, capture_output=True,
                             text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert "usage" in out.stdout
