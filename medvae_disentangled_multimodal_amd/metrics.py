"""Validation and evaluation metrics on the device (src/utils/metrics.py:14-101, used by
VAELightningModule.validation_step, src/lightning_module.py:220-300, and by evaluate.py:85-96).

`compute_reconstruction_metrics` / `compute_kl_metrics` / `compute_latent_metrics` keep the reference's
names, arguments and returned keys (floats, like the reference's `.item()` values); the `*_device`
variants return 0-d device tensors so a validation loop can log without a host sync per batch. MSE / MAE
reuse the fused loss reductions, PSNR follows torchmetrics' `peak_signal_noise_ratio(data_range=1.0)`,
SSIM, the KL statistics and the latent statistics run on `csrc/metrics.hip`.
"""
from __future__ import annotations

import math
from typing import Dict

import torch

from . import _lib, ops


def ssim_per_image(preds: torch.Tensor, target: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    ops._check(preds, "ssim input")
    p = ops.nhwc(preds.float())
    t = ops.nhwc(target.to(device=p.device, dtype=torch.float32))
    n, c, h, w = p.shape
    out = torch.empty(n, device=p.device, dtype=torch.float32)
    _lib.call("mvae_ssim", p.data_ptr(), t.data_ptr(), n, h, w, c, float(data_range), out.data_ptr(),
              ops._stream(p))
    return out


def compute_reconstruction_metrics_device(original: torch.Tensor, reconstructed: torch.Tensor) -> Dict[str, torch.Tensor]:
    with torch.no_grad():
        mse = ops.mse_mean(reconstructed, original)
        mae = ops.l1_mean(reconstructed, original)
        psnr = -10.0 * torch.log10(mse)  # torchmetrics PSNR, data_range = 1.0, over the whole batch
        ssim = ssim_per_image(reconstructed, original, 1.0).mean()
    return {"mse": mse, "mae": mae, "psnr": psnr, "ssim": ssim}


def compute_kl_metrics_device(mean: torch.Tensor, logvar: torch.Tensor) -> Dict[str, torch.Tensor]:
    ld_m = ops._pixel_ld(mean) if mean.dim() == 4 else None
    ld_l = ops._pixel_ld(logvar) if logvar.dim() == 4 else None
    if ld_m is not None and ld_m == ld_l:
        mu, lv, ld = mean, logvar, ld_m  # channel slices of the encoder output, read in place
        npix, zc = mean.shape[0] * mean.shape[2] * mean.shape[3], mean.shape[1]
    else:  # [B, D] latents (or any layout): per-sample sums over dim 1
        mu = mean.detach().float().reshape(mean.shape[0], mean.shape[1], -1).transpose(1, 2).contiguous()
        lv = logvar.detach().float().reshape(logvar.shape[0], logvar.shape[1], -1).transpose(1, 2).contiguous()
        npix, zc = mu.shape[0] * mu.shape[1], mu.shape[2]
        ld = zc
    out = torch.empty(4, device=mean.device, dtype=torch.float32)
    ws = ops.ARENA.get("klstats", _lib.query("mvae_kl_stats_workspace_bytes", npix), mean.device)
    _lib.call("mvae_kl_stats", mu.data_ptr(), lv.data_ptr(), ld, npix, zc, out.data_ptr(), ws.data_ptr(),
              ws.numel(), ops._stream(mean))
    return {"kl_total": out[0], "kl_mean": out[1], "kl_std": out[2], "kl_per_dim_mean": out[3]}


def compute_latent_metrics_device(latents: torch.Tensor) -> Dict[str, torch.Tensor]:
    """compute_latent_metrics (src/utils/metrics.py:76-101) as 0-d device tensors, without a host sync. The three
    values do not depend on the order of the features, so a channels_last latent (or a channel slice of one, such as
    the mean half of the encoder output) is read in place as [B][H*W][C], and an NCHW-contiguous or 2-D latent as
    [B][1][D]; any other layout is made contiguous first."""
    t = latents.detach().float()
    ops._check(t, "latent metrics input")
    if t.dim() < 2 or t.numel() == 0:
        raise ValueError(f"latent metrics need non-empty [B, D] or [B, C, H, W] latents, got {tuple(t.shape)}")
    if t.dim() == 4 and not t.is_contiguous():
        t, ld = ops._pix(t)  # channels_last or a channel slice of it in place, anything else through a copy
        batch, pixels, channels = t.shape[0], t.shape[2] * t.shape[3], t.shape[1]
        stride = pixels * ld
    else:
        t = t.flatten(1)  # a view of the NCHW-contiguous tensor (other ranks and layouts: a contiguous copy)
        if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
            t = t.contiguous()
        batch, pixels, channels = t.shape[0], 1, t.shape[1]
        ld, stride = channels, (t.stride(0) if batch > 1 else channels)
    out = torch.empty(3, device=t.device, dtype=torch.float32)
    ws = ops.ARENA.get("latstats", _lib.query("mvae_latent_stats_workspace_bytes", batch, pixels, channels), t.device)
    _lib.call("mvae_latent_stats", t.data_ptr(), ld, stride, batch, pixels, channels, out.data_ptr(), ws.data_ptr(),
              ws.numel(), ops._stream(t))
    return {"latent_mean_avg": out[0], "latent_std_avg": out[1], "latent_sparsity": out[2]}


def compute_reconstruction_metrics(original: torch.Tensor, reconstructed: torch.Tensor) -> Dict[str, float]:
    return {k: float(v) for k, v in compute_reconstruction_metrics_device(original, reconstructed).items()}


def compute_kl_metrics(mean: torch.Tensor, logvar: torch.Tensor) -> Dict[str, float]:
    return {k: float(v) for k, v in compute_kl_metrics_device(mean, logvar).items()}


def compute_latent_metrics(latents: torch.Tensor) -> Dict[str, float]:
    return {k: float(v) for k, v in compute_latent_metrics_device(latents).items()}
