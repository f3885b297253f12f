"""Gradient accumulation (VAELightningModule(accumulate_grad_batches=N)) as host logic, no kernels run: argument
validation, the window counter that decides which fit_step call zeroes / prepares and which one exchanges / steps,
the number of collectives per window, and the checkpoint guard."""
import inspect

import pytest
import torch

import medvae_disentangled_multimodal_amd as M
from medvae_disentangled_multimodal_amd import checkpoint, ops

KW = dict(input_channels=3, latent_dim=4, hidden_channels=32, ch_mult=(1, 2), num_res_blocks=1,
          attn_resolutions=[8], resolution=16)
DKW = dict(num_modalities=5, shared_latent_dim=2, modality_latent_dim=2, hidden_channels=32, ch_mult=(1, 2),
           num_res_blocks=1, attn_resolutions=[], dropout=0.0, resolution=16)


def _module(n=None, loss=None, model=None, **kw):
    torch.manual_seed(0)
    model = M.BaseVAE(**KW) if model is None else model
    if n is not None:
        kw["accumulate_grad_batches"] = n
    return M.VAELightningModule(model, {"type": "adamw", "lr": 2e-4}, {"type": "none"}, loss or {"type": "vae"},
                                gradient_clip_val=1.0, **kw)


@pytest.mark.parametrize("bad", [0, -1, 2.5])
def test_invalid_accumulate_grad_batches_raises(bad):
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        _module(bad)


def test_manual_optimisation_refuses_accumulation():
    with pytest.raises(ValueError, match="lpips_discriminator"):
        _module(2, loss={"type": "lpips_discriminator", "allow_synthetic_lpips": True})


def test_default_and_signature():
    mod = _module()
    assert mod.accumulate_grad_batches == 1 and mod.accumulating is False
    assert _module(4).accumulate_grad_batches == 4
    ps = list(inspect.signature(M.VAELightningModule.fit_step).parameters.values())
    assert [p.name for p in ps] == ["self", "batch", "batch_idx", "eps", "last_batch"]
    assert ps[2].default == 0 and ps[3].default is None and ps[4].default is False
    assert all(p.kind == p.POSITIONAL_OR_KEYWORD for p in ps[:4]) and ps[4].kind == ps[4].KEYWORD_ONLY
    with pytest.raises(AttributeError):
        mod.accumulating = True  # read-only


class _Trace:
    """fit_step with the device work stubbed: records what each call asked of the two phases."""

    def __init__(self, mod, monkeypatch):
        self.calls, self.steps, self.stale, self.closed = [], 0, 0, []
        monkeypatch.setattr(ops, "set_precision", lambda p: 0)
        monkeypatch.setattr(ops, "restore_math_mode", lambda m: None)
        orig_stale = ops.flat_weights_stale

        def stale():
            self.stale += 1
            orig_stale()
        monkeypatch.setattr(ops, "flat_weights_stale", stale)

        def fb(batch, batch_idx, eps, exchange=True, first=True):
            self.calls.append((first, exchange))
            mod._last_outputs = None
            return torch.tensor(float(len(self.calls)), requires_grad=True)

        def opt(used=None, exchange=True):
            self.steps += 1
            ops.flat_weights_stale()
        monkeypatch.setattr(mod, "_forward_backward", fb)
        monkeypatch.setattr(mod, "_optimizer_phase", opt)
        # (the window's boundary -- exchange, then the division by N -- ahead of the optimizer phase)
        monkeypatch.setattr(mod, "_close_window", lambda exchange=True: self.closed.append((len(self.calls), self.steps)))
        mod.optimizer = object()  # (configured: fit_step builds no flat buffers here)


def test_window_counter_n3(monkeypatch):
    mod = _module(3)
    t = _Trace(mod, monkeypatch)
    seen = []
    for i in range(3):
        loss = mod.fit_step(None, 7)  # (a constant batch_idx, as bench.py passes: the position is the module's own count)
        assert not loss.requires_grad and float(loss) == i + 1  # undivided, detached
        seen.append((mod.global_step_count, mod.accumulating, t.steps))
    assert t.calls == [(True, False), (False, False), (False, True)]  # zero / prep on 1 only; exchange on 3 only
    assert seen == [(0, True, 0), (0, True, 0), (1, False, 1)]
    assert t.stale == 1  # the prepared weight formats live until the optimizer step, not per micro-batch
    assert t.closed == [(3, 0)]  # the window's sum is divided once, after call 3's backward and before its step
    mod.fit_step(None, 7)
    assert t.calls[-1] == (True, False) and mod.accumulating


def test_last_batch_closes_the_window_early(monkeypatch):
    mod = _module(3)
    t = _Trace(mod, monkeypatch)
    mod.fit_step(None, 0)
    mod.fit_step(None, 1, last_batch=True)
    assert t.calls == [(True, False), (False, True)] and t.steps == 1
    assert mod.global_step_count == 1 and not mod.accumulating
    mod.fit_step(None, 0)  # the next epoch's first micro-batch opens a new window
    assert t.calls[-1] == (True, False) and mod.accumulating and mod.global_step_count == 1
    mod.fit_step(None, 1)
    mod.fit_step(None, 2)
    assert t.calls[-1] == (False, True) and mod.global_step_count == 2 and not mod.accumulating


def test_n1_steps_every_call(monkeypatch):
    mod = _module(1)
    t = _Trace(mod, monkeypatch)
    for i in range(3):
        mod.fit_step(None, 0, last_batch=(i == 1))
        assert mod.global_step_count == i + 1 and not mod.accumulating
    assert t.calls == [(True, True)] * 3 and t.steps == 3 and t.stale == 3
    assert t.closed == []  # no division at N = 1: the launches it always issued


def test_an_error_inside_a_window_resets_it(monkeypatch):
    mod = _module(3)
    t = _Trace(mod, monkeypatch)
    mod.fit_step(None, 0)

    def boom(*a, **k):
        raise RuntimeError("step failed")
    good = mod._forward_backward
    monkeypatch.setattr(mod, "_forward_backward", boom)
    with pytest.raises(RuntimeError, match="step failed"):
        mod.fit_step(None, 1)
    assert not mod.accumulating and t.stale == 1  # (error path: the prepared formats are dropped)
    monkeypatch.setattr(mod, "_forward_backward", good)
    mod.fit_step(None, 0)
    assert t.calls[-1] == (True, False)


class _CountingGroup:
    """Stands in for ddp.DataParallel: counts what a window asks of the process group."""
    world = 2

    def __init__(self):
        self.begin = self.allreduce = self.any = 0

    def begin_backward(self):
        self.begin += 1

    def allreduce_gradients(self, flat):
        self.allreduce += 1

    def any_across_ranks(self, flags):
        self.any += 1
        return flags


def test_one_exchange_per_window(monkeypatch):
    """The real _forward_backward / _optimizer_phase on a CPU disentangled module with the model, loss and optimizer
    stubbed: N = 3 asks the process group for one begin_backward, one allreduce_gradients and one any_across_ranks
    per window, the optimizer gets the sum of the window's gradients divided by 3, and the usage mask handed to it is
    the union of the window's modalities."""
    model = M.DisentangledConditionalVAE(**DKW)
    mod = _module(3, loss={"type": "disentangled_vae"}, model=model)
    mod.configure_optimizers()
    monkeypatch.setattr(ops, "set_precision", lambda p: 0)
    monkeypatch.setattr(ops, "restore_math_mode", lambda m: None)
    preps = []
    monkeypatch.setattr(ops, "prep_flat_weights", lambda d: preps.append(1))
    zeros = []
    monkeypatch.setattr(mod.optimizer, "zero_grad", lambda *a, **k: (zeros.append(1), mod.flat.grad.zero_()))
    masks, handed = [], []
    monkeypatch.setattr(mod.optimizer, "step",
                        lambda used=None, **k: (masks.append(used.clone()), handed.append(mod.flat.grad.clone())))
    backprop = []

    def training_step(batch, batch_idx, eps=None):
        mod._usage = batch
        mod._last_outputs = None
        w = torch.ones((), requires_grad=True)

        def hook(g):  # (stands in for the gradient producers: every one adds into its flat slot)
            backprop.append(float(g))
            mod.flat.grad.add_(float(g) * (1 + len(backprop) % 3))
        w.register_hook(hook)
        return w * 6.0
    monkeypatch.setattr(mod, "training_step", training_step)
    pg = mod.process_group = _CountingGroup()
    windows = [[torch.tensor([0, 0]), torch.tensor([3, 3]), torch.tensor([0, 3])],
               [torch.tensor([1, 1]), torch.tensor([1, 1]), torch.tensor([2, 1])]]
    for w, idxs in enumerate(windows):
        for idx in idxs:
            loss = mod.fit_step(idx, 0)
            assert float(loss) == 6.0
        assert (pg.begin, pg.allreduce, pg.any) == (w + 1, w + 1, w + 1)
        assert (len(preps), len(zeros), len(masks)) == (w + 1, w + 1, w + 1)
    assert backprop == [6.0] * 6  # every micro-batch backpropagates its own, undivided loss ...
    for g in handed:  # ... and the optimizer sees the window's sum / 3: 6 * (1 + 2 + 3) / 3
        assert torch.equal(g, torch.full_like(g, 12.0))
    pm = torch.tensor([model.parameter_modality(n) for n in mod.flat.names])
    for mask, mods in zip(masks, ({0, 3}, {1, 2})):
        for m in range(5):
            assert bool(mask[pm == m].bool().all()) == (m in mods) and bool(mask[pm == m].bool().any()) == (m in mods)
        assert bool(mask[pm == -1].bool().all()) and not bool(mask[pm == -2].bool().any())


def test_checkpoint_refused_inside_a_window_and_load_resets(monkeypatch, tmp_path):
    mod = _module(2)
    mod.configure_optimizers()
    path = str(tmp_path / "a.ckpt")
    checkpoint.save_checkpoint(mod, path)
    mod._accum_pos = 1
    assert mod.accumulating
    with pytest.raises(RuntimeError, match="accumulation window is open"):
        checkpoint.save_checkpoint(mod, path)
    with pytest.raises(RuntimeError, match="accumulation window is open"):
        checkpoint.lightning_checkpoint(mod)
    checkpoint.load_checkpoint(mod, path)
    assert not mod.accumulating
    checkpoint.save_checkpoint(mod, path)
