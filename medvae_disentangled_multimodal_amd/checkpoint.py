"""Lightning-checkpoint interchange (main.py:51-61,110-116: ModelCheckpoint / trainer.save_checkpoint;
quick_generate.py:37-42: loading `model.`-prefixed weights).

A checkpoint written here has the layout Lightning 2.5 writes for the reference's VAELightningModule
-- `state_dict` with `model.`-prefixed parameter names (logical OIHW conv weights),
`optimizer_states` in torch.optim.Adam/AdamW's own `state_dict()` format over `model.parameters()`
order, `epoch`, `global_step`, `lr_schedulers` -- so the reference can resume from it, and a
reference checkpoint loads here (weights and Adam moments land in the flat buffers).
Loading uses `torch.load(weights_only=True)`: nothing in the file is executed; a checkpoint that
needs arbitrary unpickling is refused.

A module that keeps an exponential moving average of its weights (optimizer_config["ema_decay"]) adds ONE top-level
key, `ema_state = {"decay": float, "weights": {name: logical-OIHW cpu tensor}}` (parameter names as in
`model.named_parameters()`); every other key is what it is without the average, so the reference still loads the file
strictly. `weights="ema"` writes the averaged weights as `state_dict["model.*"]` instead, without optimizer states: a
file the reference's generate.py / quick_generate.py load as the model to sample from.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Any, Dict

import torch

from .optim import FlatParameters

LIGHTNING_VERSION = "2.5.2"  # the reference's pin (uv.lock)


def _torch_optimizer_state(opt, flat) -> Dict[str, Any]:
    state = {}
    steps = opt.steps.cpu()
    for i, (p, off) in enumerate(zip(flat.params, flat.offsets)):
        if int(steps[i]) == 0:
            continue
        state[i] = {"step": torch.tensor(float(steps[i])),
                    "exp_avg": FlatParameters._view(opt.exp_avg, off, p).detach().contiguous().cpu(),
                    "exp_avg_sq": FlatParameters._view(opt.exp_avg_sq, off, p).detach().contiguous().cpu()}
    g = opt.param_groups[0]
    group = {"lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"], "weight_decay": g["weight_decay"],
             "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
             "fused": None, "params": list(range(len(flat.params)))}
    if opt.decoupled:
        group["decoupled_weight_decay"] = True
    return {"state": state, "param_groups": [group]}


def _ema_weights(module) -> "OrderedDict[str, torch.Tensor]":
    """{parameter name: averaged weight}, logical shapes (conv weights OIHW, contiguous), on the CPU."""
    opt, flat = module.optimizer, module.flat
    if opt is None or getattr(opt, "ema", None) is None:
        raise RuntimeError('checkpoint: the module keeps no EMA (optimizer_config["ema_decay"] is not set, or no '
                           "optimizer is configured yet)")
    if getattr(module, "_in_ema_scope", False):
        raise RuntimeError("checkpoint: called inside ema_scope() (the weights and their average are exchanged)")
    return OrderedDict((n, FlatParameters._view(opt.ema, off, p).detach().contiguous().cpu())
                       for n, p, off in zip(flat.names, flat.params, flat.offsets))


def lightning_checkpoint(module, epoch: int = 0, weights: str = "live") -> Dict[str, Any]:
    """The dict `trainer.save_checkpoint` would write for this module: the LightningModule's own state dict
    (`model.*` and the criterion's `criterion.*` -- LPIPS network, discriminator weights and BatchNorm
    buffers), one optimizer state per optimizer (the discriminator's Adam second, lightning_module.py:
    427-433). Lightning checkpoints at optimisation-step boundaries only: a module inside a gradient-accumulation
    window (micro-batches in the flat gradient, no step yet) is refused, since the file could not hold that state.
    weights="ema": the averaged weights in place of the live ones in `state_dict`, and no optimizer states (a model to
    evaluate or sample from, not to resume)."""
    if weights not in ("live", "ema"):
        raise ValueError(f'checkpoint: weights must be "live" or "ema", got {weights!r}')
    if getattr(module, "accumulating", False):
        raise RuntimeError("checkpoint: a gradient-accumulation window is open (accumulate_grad_batches = "
                           f"{module.accumulate_grad_batches}); save at a step boundary, after the window's last "
                           "fit_step")
    sd = OrderedDict((f"model.{k}", v.detach().contiguous().cpu()) for k, v in module.model.state_dict().items())
    crit = getattr(module, "criterion", None)
    if isinstance(crit, torch.nn.Module):
        sd.update((f"criterion.{k}", v.detach().contiguous().cpu()) for k, v in crit.state_dict().items())
    ck = {"epoch": int(epoch), "global_step": int(getattr(module, "global_step_count", 0)),
          "pytorch-lightning_version": LIGHTNING_VERSION, "state_dict": sd, "loops": {}, "callbacks": {},
          "lr_schedulers": [], "optimizer_states": []}
    if weights == "ema":
        for n, v in _ema_weights(module).items():
            sd[f"model.{n}"] = v
        return ck
    if getattr(module, "_in_ema_scope", False):
        raise RuntimeError("checkpoint: called inside ema_scope() (the weights and their average are exchanged)")
    if module.optimizer is not None and getattr(module.optimizer, "ema", None) is not None:
        ck["ema_state"] = {"decay": float(module.optimizer.ema_decay), "weights": dict(_ema_weights(module))}
    if module.optimizer is not None:
        ck["optimizer_states"] = [_torch_optimizer_state(module.optimizer, module.flat)]
        if getattr(module, "optimizer_d", None) is not None:
            ck["optimizer_states"].append(_torch_optimizer_state(module.optimizer_d, module.flat_d))
        if module.scheduler is not None and hasattr(module.scheduler, "state_dict"):
            ck["lr_schedulers"] = [module.scheduler.state_dict()]
    return ck


def save_checkpoint(module, path: str, epoch: int = 0, weights: str = "live"):
    torch.save(lightning_checkpoint(module, epoch, weights), path)


def load_checkpoint(module, ckpt, strict: bool = True, load_optimizer: bool = True):
    """Load a Lightning checkpoint (path or dict) of the reference's VAELightningModule (or of this
    one) into `module`: model weights (into the flat parameter buffer) and, when present and an
    optimizer is configured, the Adam/AdamW moments and step counts. A module that keeps an EMA of its weights takes
    the checkpoint's `ema_state` weights into its flat EMA buffer, or, from a checkpoint without one, restarts the
    average from the loaded weights; a module without EMA ignores the key."""
    if getattr(module, "_in_ema_scope", False):
        raise RuntimeError("load_checkpoint: called inside ema_scope()")
    if isinstance(ckpt, str):
        ckpt = torch.load(ckpt, map_location="cpu", weights_only=True)
    module._graph = None  # a captured step froze the old hyper-parameters (betas / eps / lr) as launch values
    if hasattr(module, "_reset_window"):
        module._reset_window()  # (an open accumulation window belongs to the replaced weights: the next fit_step opens one)
    sd = {k[len("model."):]: v for k, v in ckpt["state_dict"].items() if k.startswith("model.")}
    module.model.load_state_dict(sd, strict=strict)
    crit = getattr(module, "criterion", None)
    csd = {k[len("criterion."):]: v for k, v in ckpt["state_dict"].items() if k.startswith("criterion.")}
    if isinstance(crit, torch.nn.Module) and (csd or (strict and len(crit.state_dict()) > 0)):
        crit.load_state_dict(csd, strict=strict)
    states = ckpt.get("optimizer_states") or []
    if load_optimizer and states:
        if module.optimizer is None:
            module.configure_optimizers()
        _load_optimizer_state(module.optimizer, module.flat, states[0])
        if len(states) > 1 and getattr(module, "optimizer_d", None) is not None:
            _load_optimizer_state(module.optimizer_d, module.flat_d, states[1])
    if module.optimizer is None and ckpt.get("ema_state") and \
            getattr(module, "optimizer_config", {}).get("ema_decay") is not None:
        module.configure_optimizers()  # (the average lives in the optimizer's flat EMA buffer)
    opt = module.optimizer
    if opt is not None and getattr(opt, "ema", None) is not None:
        _load_ema(opt, module.flat, (ckpt.get("ema_state") or {}).get("weights"), strict)
    module.global_step_count = int(ckpt.get("global_step", 0))
    return ckpt


def _load_ema(opt, flat, weights, strict: bool):
    with torch.no_grad():
        if weights is None:
            opt.ema.copy_(flat.data)
            return
        missing = [n for n in flat.names if n not in weights]
        if strict and (missing or len(weights) != len(flat.names)):
            raise RuntimeError(f"checkpoint: ema_state does not match the model's parameters (missing {missing[:4]}, "
                               f"unexpected {[n for n in weights if n not in flat.names][:4]})")
        for n, p, off in zip(flat.names, flat.params, flat.offsets):
            # (a parameter the file has no average for starts from its loaded weight)
            FlatParameters._view(opt.ema, off, p).copy_(weights[n] if n in weights else p.detach())


def _load_optimizer_state(opt, flat, st):
    steps = torch.zeros(len(flat.params), dtype=torch.int32)
    with torch.no_grad():
        for i, (p, off) in enumerate(zip(flat.params, flat.offsets)):
            s = st["state"].get(i, st["state"].get(str(i)))
            if s is None:
                FlatParameters._view(opt.exp_avg, off, p).zero_()
                FlatParameters._view(opt.exp_avg_sq, off, p).zero_()
                continue
            FlatParameters._view(opt.exp_avg, off, p).copy_(s["exp_avg"])
            FlatParameters._view(opt.exp_avg_sq, off, p).copy_(s["exp_avg_sq"])
            steps[i] = int(float(s["step"]))
    opt.steps.copy_(steps)
    g = st["param_groups"][0]
    for k in ("lr", "betas", "eps", "weight_decay"):
        if k in g:
            opt.param_groups[0][k] = tuple(g[k]) if k == "betas" else g[k]
