"""Checkpoint save / load with the reference's call surface.

``load_checkpoint(model, optimizer, path) -> None`` mutates in place (reference train/model_loader.py:35-42);
``save_checkpoint(model, optimizer, path) -> None`` (reference train/rl_nonadversarial.py:62-67).
``optimizer=None`` loads (saves) the model alone: inference needs no Adam state (infer.InferenceWeights re-derives the bf16 shadows).
The reference stores ``{"model": nnx.state(model), "optimizer": nnx.state(optimizer)}`` with orbax in a directory
``path``; here the same two-entry tree (parameter names = Flax attribute paths) is one ``checkpoint.pt`` inside it.
A weight average kept by the optimizer (``Optimizer(..., ema_decay=...)``) travels inside the ``"optimizer"`` entry as ``ema.{name}``;
``load_ema_weights(model, path)`` writes it into a model's parameters for inference.
"""
import os

import torch


def save_checkpoint(model, optimizer, path):
    os.makedirs(path, exist_ok=True)
    state = {
        "model": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
    }
    if optimizer is not None:
        state["optimizer"] = optimizer.state_dict()
    tmp = os.path.join(path, "checkpoint.pt.tmp")
    torch.save(state, tmp)
    os.replace(tmp, os.path.join(path, "checkpoint.pt"))


def load_checkpoint(model, optimizer, path):
    state = torch.load(os.path.join(path, "checkpoint.pt"), map_location="cpu", weights_only=True)
    own = model.state_dict()
    missing = set(own) - set(state["model"])
    extra = set(state["model"]) - set(own)
    if missing or extra:
        raise KeyError(f"checkpoint/model mismatch: missing {sorted(missing)[:5]}, unexpected {sorted(extra)[:5]}")
    with torch.no_grad():
        for k, v in state["model"].items():
            own[k].copy_(v)          # in place: keeps parameters aliased to the optimizer's flat buffer (and a captured graph's pointers)
    if optimizer is not None:
        optimizer.load_state_dict(state["optimizer"])


def load_ema_weights(model, path):
    """Overwrite ``model``'s parameters, in place, with the weight average stored in the checkpoint's optimizer state (``ema.{name}``).
    Buffers and any parameter the average does not cover keep what ``load_checkpoint`` gave them, so call that first."""
    state = torch.load(os.path.join(path, "checkpoint.pt"), map_location="cpu", weights_only=True)
    ema = {k[len("ema."):]: v for k, v in state.get("optimizer", {}).items() if k.startswith("ema.")}
    if not ema:
        raise KeyError(f"{path}: the checkpoint holds no weight average (no ema.* entries in its optimizer state); it was trained without --ema")
    own = dict(model.named_parameters())
    extra = set(ema) - set(own)
    if extra:
        raise KeyError(f"checkpoint/model mismatch: averaged weights for unknown parameters {sorted(extra)[:5]}")
    with torch.no_grad():
        for k, v in ema.items():
            own[k].copy_(v)
