"""Encoder / Decoder / VideoVAE with the surface of the reference's train/model.py (5-tuple, Gumbel-STE gate)."""
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F
from einops import rearrange
from torch import nn

from . import ops
from .layers import PatchEmbedding, FactoredAttention, GumbelSigmoidSTE, PatchUnEmbedding, Linear, linear_pair
from .rngs import Rngs
from .unet import UNet


class Latents(NamedTuple):
    """What ``VideoVAE.encode`` returns (one row per clip: never pair-doubled)."""
    compressed_representation: torch.Tensor      # (b, t, hw, ld) in the decoder's compute dtype: fill token on dropped frames, mean on kept ones
    selection: torch.Tensor                      # (b, t) fp32 in {0, 1}: the frame gate that was applied
    probability: Optional[torch.Tensor]          # (b, t) fp32 sigmoid(logits) (rl flavour), None for the model flavour
    mean: torch.Tensor                           # (b, t, hw, ld)
    log_variance: Optional[torch.Tensor]         # (b, t, hw, ld), None when not asked for


def eval_mask(mask, b, t):
    """The temporal mask as the blocks take it: a (b, t) mask becomes its (b, 1, 1, t) view (loss.compact_mask); any form forward accepts
    passes through unchanged."""
    return mask.reshape(b, 1, 1, t) if mask.dim() == 2 else mask


def frame_mask(mask, b, t):
    """(b, t) float view of the temporal mask the drivers pass: (b*hw,1,1,t) as train_step expands it (rl_nonadversarial.py:190-192)
    or (b,1,1,t) (claude_distributed/layers.py:213-214); every patch of a sample carries the same row."""
    return mask.reshape(b, -1, t)[:, 0].to(torch.float32)


class Encoder(nn.Module):
    """Reference train/model.py:14-60 -> (mean, log_variance, selection (b,t,1,1) in {0,1})."""

    flavour = "model"

    def __init__(self, height, width, channels, patch_size, depth, mlp_dim, num_heads, qkv_features, max_temporal_len,
                 spatial_compression_rate, rngs, dtype=torch.bfloat16, param_dtype=torch.float32):
        super().__init__()
        max_spatial_len = height // patch_size * width // patch_size
        self.last_dim = channels * patch_size * patch_size
        self.dtype = dtype
        self.patch_embedding = PatchEmbedding(height, width, channels, patch_size, rngs, dtype, param_dtype)
        ld = self.last_dim // spatial_compression_rate
        self.spatial_compression = Linear(self.last_dim, ld, rngs, dtype, param_dtype)
        self.variance_estimator = Linear(self.last_dim, ld, rngs, dtype, param_dtype)
        self.selection_layer1 = Linear(ld, 1, rngs, dtype, param_dtype)
        self.selection_layer2 = Linear(max_spatial_len, 1, rngs, dtype, param_dtype)
        self.gumbel_sigmoid = GumbelSigmoidSTE(temperature=1.0)
        self.layers = nn.ModuleList([
            FactoredAttention(mlp_dim, self.last_dim, num_heads, qkv_features, max_temporal_len, max_spatial_len, rngs,
                              dtype, param_dtype) for _ in range(depth)])

    def _features(self, x, mask):
        x = self.patch_embedding(x)
        # each layer hands its last residual add to the next layer's first LayerNorm kernel (layers.FactoredAttention)
        pend, n = None, len(self.layers)
        for i, layer in enumerate(self.layers):
            r = layer(x, mask, pending=pend, defer=i + 1 < n)
            if i + 1 < n:
                pend = r
            else:
                x = r
        return x

    def _trunk(self, x, mask):
        x = self._features(x, mask)
        mean, v = linear_pair(x, self.spatial_compression, self.variance_estimator)      # GPU: one node, the input gradients meet inside a product
        variance = F.softplus(v)
        log_variance = torch.log(variance)
        si = rearrange(self.selection_layer1(mean), "b t hw 1 -> b t hw")
        return mean, log_variance, self.selection_layer2(si) + 1

    def forward(self, x, mask, rngs, train=True):
        mean, log_variance, logits = self._trunk(x, mask)
        selection = self.gumbel_sigmoid(logits.float(), rngs, train=train)
        return mean, log_variance, rearrange(selection, "b t 1 -> b t 1 1")

    def gated_ok(self, x, fill_token):
        """May forward_gated run?  (bf16 GPU model, temperature 1, fp32 parameters, shapes the fused kernel covers.)"""
        sl1, sl2 = self.selection_layer1, self.selection_layer2
        return (self.dtype == torch.bfloat16 and x.is_cuda and self.gumbel_sigmoid.temperature == 1.0
                and ops.encoder_head_shape_ok(x.shape[0], x.shape[1], sl2.kernel.shape[0], sl1.kernel.shape[0], sl1.kernel, sl1.bias, sl2.kernel,
                                              sl2.bias, fill_token))

    def forward_gated(self, x, mask, rngs, fill_token):
        """Train mode on the GPU -> (mean, log_variance, selection, compressed_representation, kl (b, t)): everything behind the two
        768 -> ld products -- softplus / log, both selection layers, the Gumbel-sigmoid STE, the reparameterisation, the KL term and the
        latent gate fill * (1 - s) + z * s of VideoVAE.__call__ (model.py:121-133) -- in one launch each way (ops.encoder_head) instead of
        ~45 framework launches per step.  The noise draws keep the reference's order: Gumbel, then reparameterisation."""
        sl1, sl2 = self.selection_layer1, self.selection_layer2
        h = self._features(x, mask)
        mean, v = linear_pair(h, self.spatial_compression, self.variance_estimator)      # one node: the two input gradients meet inside a product
        b, t = mean.shape[0], mean.shape[1]
        u = rngs.draw("gumbel_u", "uniform", (b, t, 1), mean.device)
        eps = rngs.draw("reparam_eps", "normal", mean.shape, mean.device)
        log_variance, comp, selection, kl = ops.encoder_head(mean, v, sl1.kernel, sl1.bias, sl2.kernel, sl2.bias, fill_token, u, eps,
                                                             frame_mask(mask, b, t))
        return mean, log_variance, selection, comp, kl

    @torch.no_grad()
    def heads_eval(self, x, mask, fill_token, u=None, want_log_variance=True):
        """Encoder forward in eval mode plus the latent gate with z = mean (reference train/model.py:121-133 with train=False) ->
        (mean, log_variance or None, selection (b, t), probability (b, t) or None, compressed_representation).  model flavour: selection =
        round(sigmoid(logits)) (layers.py:250-252); rl flavour: probability = sigmoid(logits), selection = u < probability when ``u`` (b, t)
        uniforms are given, else round(probability).  Frames ``mask`` marks 0 are dropped.  On the bf16 GPU path (gated_ok) the heads and
        the gate are one launch (ops.encoder_head_eval); elsewhere the same math from framework ops."""
        rl = self.flavour == "rl"
        b, t = x.shape[0], x.shape[1]
        mbt = frame_mask(mask, b, t)                  # a view of a float mask: nothing runs between the encoder's last product and the decoder
        h = self._features(x, mask)
        if want_log_variance:
            mean, v = linear_pair(h, self.spatial_compression, self.variance_estimator)
        else:
            mean, v = self.spatial_compression(h.to(self.dtype)), None       # reconstruct: the variance head is not run at all
        if self.gated_ok(x, fill_token):
            log_variance, comp, selection, probability = ops.encoder_head_eval(
                mean, v, self.selection_layer1.kernel, self.selection_layer1.bias, self.selection_layer2.kernel, self.selection_layer2.bias,
                fill_token, u, mbt, rl)
            return mean, log_variance, selection, probability, comp
        log_variance = torch.log(F.softplus(v)) if v is not None else None
        logits = self.selection_layer2(rearrange(self.selection_layer1(mean), "b t hw 1 -> b t hw")) + 1
        if rl:
            prob = torch.sigmoid(logits)
            sel = (u.reshape(prob.shape) < prob) if u is not None else torch.round(prob)
            probability = prob.float().reshape(b, t)
        else:
            sel, probability = self.gumbel_sigmoid(logits.float(), None, train=False), None
        selection = sel.float().reshape(b, t) * (mbt != 0)
        s4 = selection.reshape(b, t, 1, 1)
        comp = (fill_token * (1 - s4) + mean * s4).to(mean.dtype)
        return mean, log_variance, selection, probability, comp


class Decoder(nn.Module):
    """Reference train/model.py:62-97: Linear -> depth x FactoredAttention -> un-patchify -> coarse + UNet(features)."""

    def __init__(self, height, width, channels, patch_size, depth, mlp_dim, num_heads, qkv_features, max_temporal_len,
                 spatial_compression_rate, unembedding_upsample_rate, rngs, dtype=torch.bfloat16, param_dtype=torch.float32):
        super().__init__()
        self.last_dim = channels * patch_size * patch_size
        self.dtype = dtype
        self.patch_unembedding = PatchUnEmbedding(height, width, channels, patch_size, unembedding_upsample_rate, rngs,
                                                  dtype, param_dtype)
        self.spatial_decompression = Linear(self.last_dim // spatial_compression_rate, self.last_dim, rngs, dtype, param_dtype)
        max_spatial_len = height // patch_size * width // patch_size
        self.layers = nn.ModuleList([
            FactoredAttention(mlp_dim, self.last_dim, num_heads, qkv_features, max_temporal_len, max_spatial_len, rngs,
                              dtype, param_dtype) for _ in range(depth)])
        self.unet = UNet(channels=channels * unembedding_upsample_rate, base_features=16, num_levels=3,
                         out_features=channels, rngs=rngs, dtype=dtype, param_dtype=param_dtype)

    def forward(self, x, mask, rngs, train=True):
        x = self.spatial_decompression(x)
        # each layer hands its last residual add to the next layer's first LayerNorm kernel (layers.FactoredAttention)
        pend, n = None, len(self.layers)
        for i, layer in enumerate(self.layers):
            r = layer(x, mask, pending=pend, defer=i + 1 < n)
            if i + 1 < n:
                pend = r
            else:
                x = r
        plan = self.unet.pad_plan(x.is_cuda)                        # the UNet's 12-channel weights ride in the un-embedding's pad launch
        out = self.patch_unembedding.forward_padded(x, plan)       # bf16 GPU path: un-patchify + channel pad in one copy
        if out is not None and plan is not None:
            feat, x, padded = out
            return self.unet(feat, residual=x, padded=padded)
        feat, x = out if out is not None else self.patch_unembedding(x)
        return self.unet(feat, residual=x)                          # x + self.unet(feat): the add rides in the UNet's final product


class InferenceMixin:
    """encode / decode / reconstruct of both VideoVAE flavours: forward-only, under torch.no_grad(), one row per clip.

    ``mask`` is (b, t) (1 = real frame) or any form ``forward`` accepts.  Frames the mask marks 0 are dropped (selection 0, fill token):
    the decoder's input is then fixed by the kept frames' means and the selection alone.  The rl flavour is NOT pair-doubled here: its gate
    is one Bernoulli draw per clip and frame from the ``"bernoulli_u"`` stream of ``rngs``, or, with ``rngs=None``, the deterministic
    threshold round(probability).  ``forward(..., train=False)`` keeps the reference's semantics (pair doubling in the rl flavour)."""

    @torch.no_grad()
    def encode(self, x, mask, rngs=None, want_log_variance=True):
        b, t = x.shape[0], x.shape[1]
        u = None
        if self.encoder.flavour == "rl" and rngs is not None:
            u = rngs.draw("bernoulli_u", "uniform", (b, t, 1, 1), x.device)
        mean, log_variance, selection, probability, comp = self.encoder.heads_eval(x, eval_mask(mask, b, t), self.fill_token, u,
                                                                                   want_log_variance)
        return Latents(comp, selection, probability, mean, log_variance)

    @torch.no_grad()
    def decode(self, compressed_representation, mask):
        b, t = compressed_representation.shape[0], compressed_representation.shape[1]
        return self.decoder(compressed_representation, eval_mask(mask, b, t), None, train=False)

    @torch.no_grad()
    def reconstruct(self, x, mask, rngs=None):
        """decode(encode(x, mask, rngs).compressed_representation, mask), without the log-variance."""
        return self.decode(self.encode(x, mask, rngs, want_log_variance=False).compressed_representation, mask)


def fake_quantise_latent(model, compressed_representation, keep):
    """Quantisation-aware training (``model.latent_quant_bits`` in 2 .. 8): the gated latent through the latent quantiser on the frames the
    hard selection ``keep`` kept (ops.latent_fake_quant: one launch on the GPU, straight-through gradient), which is what
    GraphedInference "evaluate" feeds the decoder under --quantise-bits.  The per-frame code histogram stays on the model as
    ``_quant_counts`` for the loss to pick up (loss.code_entropy), like ``_kl``.  With ``model.latent_rate_on`` (loss.set_quantiser:
    hparams["rate_weight"] > 0) the UNQUANTISED gated latent also goes through ops.latent_rate, with the same ``keep`` and the cost table of
    the counts just produced (loss.rate_cost_table); the (b, t) rates stay on the model as ``_quant_rate`` (loss.add_rate_term)."""
    comp = compressed_representation.contiguous()
    counts = torch.empty(tuple(comp.shape[:-2]) + (256,), dtype=torch.int32, device=comp.device)
    out = ops.latent_fake_quant(comp, keep, model.latent_quant_bits, counts)
    model._quant_counts = counts
    if getattr(model, "latent_rate_on", False):
        from .loss import rate_cost_table
        model._quant_rate = ops.latent_rate(comp, keep, model.latent_quant_bits, rate_cost_table(counts, model.latent_quant_bits))
    return out


class VideoVAE(InferenceMixin, nn.Module):
    """Reference train/model.py:101-136 -> (reconstruction, compressed_representation, selection, log_variance, mean).

    ``latent_quant_bits`` (None, or 2 .. 8): quantisation-aware training.  When set, ``forward`` (train or not, either branch) quantises
    the gated compressed representation of the frames the selection kept before the decoder sees it (fake_quantise_latent) and returns
    that tensor; encode / decode / reconstruct are not affected (infer has its own flag)."""

    latent_quant_bits = None
    latent_rate_on = False

    def __init__(self, height, width, channels, patch_size, encoder_depth, decoder_depth, mlp_dim, num_heads, qkv_features,
                 max_temporal_len, spatial_compression_rate, unembedding_upsample_rate, rngs, dtype=torch.bfloat16,
                 param_dtype=torch.float32):
        super().__init__()
        key = rngs.sampling()
        self.encoder = Encoder(height, width, channels, patch_size, encoder_depth, mlp_dim, num_heads, qkv_features,
                               max_temporal_len, spatial_compression_rate, rngs, dtype, param_dtype)
        self.decoder = Decoder(height, width, channels, patch_size, decoder_depth, mlp_dim, num_heads, qkv_features,
                               max_temporal_len, spatial_compression_rate, unembedding_upsample_rate, rngs, dtype, param_dtype)
        ld = channels * patch_size * patch_size // spatial_compression_rate
        self.fill_token = nn.Parameter(torch.randn((1, 1, 1, ld), generator=key.generator("cpu")) * 0.02)

    def forward(self, x, mask, rngs, train=True):
        self._kl = self._quant_counts = self._quant_rate = None
        if train and type(self.encoder) is Encoder and self.encoder.gated_ok(x, self.fill_token):
            # GPU train step: heads, noise, KL and gate come out of one kernel; compressed_representation holds the decoder's compute dtype
            # (the reference's fp32 sum rounded once, which is what its decoder's first Linear does to it: the same numbers downstream)
            mean, log_variance, selection, compressed_representation, kl = self.encoder.forward_gated(x, mask, rngs, self.fill_token)
            self._kl = (mean, log_variance, kl)
            if self.latent_quant_bits is not None:
                compressed_representation = fake_quantise_latent(self, compressed_representation, selection)
            reconstruction = self.decoder(compressed_representation, mask, rngs, train=train)
            return reconstruction, compressed_representation, selection, log_variance, mean
        mean, log_variance, selection = self.encoder(x, mask, rngs, train=train)
        if train:
            noise = rngs.draw("reparam_eps", "normal", log_variance.shape, log_variance.device)
            # z and the per-sample KL term in ONE pass over (mean, log_variance): the loss picks the KL up from here
            # (loss.kl_from_model) instead of streaming the two tensors a second time
            sampled_latent, kl = ops.reparameterise_kl(mean, log_variance, noise, frame_mask(mask, mean.shape[0], mean.shape[1]))
            self._kl = (mean, log_variance, kl)
        else:
            sampled_latent = mean
        # fill * (1 - s) + z * s as the reference writes it (model.py:133).  torch.lerp(fill, z, s) would be one launch instead of four,
        # but its backward adds a multi-block framework reduction (the gradient of the broadcast fill_token) to the captured step, and
        # those are kept out of a replayed hipGraph (the reduction's semaphore memset is a graph memset node).
        compressed_representation = self.fill_token * (1 - selection) + sampled_latent * selection
        if self.latent_quant_bits is not None:
            compressed_representation = fake_quantise_latent(self, compressed_representation, selection)
        reconstruction = self.decoder(compressed_representation, mask, rngs, train=train)
        return reconstruction, compressed_representation, selection, log_variance, mean
