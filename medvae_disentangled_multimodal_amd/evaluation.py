"""Evaluation driver: the metric loop of the reference's evaluate.py:55-135 (without its data loading and plots).

Per test batch the reference calls compute_reconstruction_metrics(x, rec) and compute_latent_metrics(z), keeps the
floats, and aggregates every key to mean / std / min / max over the batches into `metrics.json`. Here the seven
per-batch values stay on the device (`metrics.*_device`) in one preallocated [num_batches, 7] tensor: the loop issues
no host synchronisation, the aggregation runs on the device, and one device-to-host copy brings the result back.
"""
from __future__ import annotations

import contextlib
import json
import os
from typing import Any, Dict, Iterable, Optional, Tuple

import torch

from . import ops
from .metrics import compute_latent_metrics_device, compute_reconstruction_metrics_device

RECONSTRUCTION_KEYS = ("mse", "mae", "psnr", "ssim")
LATENT_KEYS = ("latent_mean_avg", "latent_std_avg", "latent_sparsity")


def evaluate_model(module, batches: Iterable, num_batches: Optional[int] = None, output_dir: Optional[str] = None,
                   keep_latents: int = 1000, use_ema: bool = False) -> Tuple[Dict[str, Any], Dict[str, Optional[torch.Tensor]]]:
    """Run `module` (a VAELightningModule) over `batches` of device tensors -- (x, labels), (x, labels, modality) or
    (x, labels, modality, modality_indices), dispatched like validation_step -- in eval mode, without autograd and in
    the module's precision. At most `num_batches` batches are read (default: len(batches)).

    Returns (metrics, collected):
      metrics   = {"reconstruction": {"mse": {"mean", "std", "min", "max"}, "mae", "psnr", "ssim"},
                   "latent": {"latent_mean_avg": {...}, "latent_std_avg", "latent_sparsity"}} over the batches (std is
                  the population std, numpy's default, as the reference uses), also written to
                  `output_dir`/metrics.json when `output_dir` is given;
      collected = {"latents", "labels", "modalities"}: the first `keep_latents` samples' z, labels and modality
                  vectors as host tensors (what the reference hands to its latent-space plot); "modalities" is None
                  for batches without one.
    use_ema: evaluate the exponential moving average of the weights (optimizer_config["ema_decay"]): the loop runs
    inside module.ema_scope(), which puts the live weights back on every exit path.
    The model's train / eval state and the math mode are restored on every exit path."""
    if num_batches is None:
        if not hasattr(batches, "__len__"):
            batches = list(batches)
        num_batches = len(batches)
    num_batches = int(num_batches)
    if num_batches <= 0:
        raise ValueError("evaluate_model: no batches to evaluate")
    keys = RECONSTRUCTION_KEYS + LATENT_KEYS
    rows = None
    latents, labels, modalities = [], [], []
    kept = done = 0
    was_training = module.model.training
    module.model.eval()
    prev = ops.set_precision(module.precision)
    try:
        with torch.no_grad(), (module.ema_scope() if use_ema else contextlib.nullcontext()):
            for i, batch in enumerate(batches):
                if i >= num_batches:
                    break
                if not torch.is_tensor(batch[0]) or batch[0].dim() != 4:
                    raise ValueError(f"evaluate_model: batch {i} does not start with a [B, C, H, W] image tensor")
                x, outputs = module._forward_batch(batch)
                z = outputs["z"]
                if rows is None:
                    rows = torch.empty((num_batches, len(keys)), device=x.device, dtype=torch.float32)
                vals = compute_reconstruction_metrics_device(x, outputs["reconstruction"])
                vals.update(compute_latent_metrics_device(z))
                rows[i].copy_(torch.stack([vals[k] for k in keys]))
                take = min(z.shape[0], keep_latents - kept)  # (host integers: shapes, no device value is read)
                if take > 0:
                    latents.append(z[:take])
                    if len(batch) > 1 and torch.is_tensor(batch[1]):
                        labels.append(batch[1][:take])
                    if len(batch) > 2 and torch.is_tensor(batch[2]):
                        modalities.append(batch[2][:take])
                    kept += take
                done = i + 1
            if done == 0:
                raise ValueError("evaluate_model: no batches to evaluate")
            # (in double: the batches' values lie close together, and fp32 would round their spread away)
            r = rows[:done].double()
            stats = torch.stack([r.mean(0), r.std(0, unbiased=False), r.min(0).values, r.max(0).values]).cpu()
            collected = {name: torch.cat(parts, 0).cpu() if parts else None
                         for name, parts in (("latents", latents), ("labels", labels), ("modalities", modalities))}
    finally:
        ops.restore_math_mode(prev)
        module.model.train(was_training)
    metrics: Dict[str, Any] = {"reconstruction": {}, "latent": {}}
    for j, k in enumerate(keys):
        metrics["reconstruction" if k in RECONSTRUCTION_KEYS else "latent"][k] = {
            name: float(stats[s, j]) for s, name in enumerate(("mean", "std", "min", "max"))}
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
        with open(os.path.join(output_dir, "metrics.json"), "w") as f:
            json.dump(metrics, f, indent=2)
    return metrics, collected
