"""Exponential moving average of the weights (optimizer_config["ema_decay"]) as host logic, no kernels run: argument
validation, the flat EMA buffer FusedAdam creates, and the checkpoint's `ema_state` key / weights="ema" form through
the KRSC views of the flat buffers."""
import io

import pytest
import torch

import medvae_disentangled_multimodal_amd as M
from medvae_disentangled_multimodal_amd import checkpoint
from medvae_disentangled_multimodal_amd.optim import FlatParameters

KW = dict(input_channels=3, latent_dim=4, hidden_channels=32, ch_mult=(1, 2), num_res_blocks=1,
          attn_resolutions=[8], resolution=16)


def _module(ema=None, seed=0, configure=True, **oc):
    torch.manual_seed(seed)
    cfg = {"type": "adamw", "lr": 2e-4, **oc}
    if ema is not None:
        cfg["ema_decay"] = ema
    mod = M.VAELightningModule(M.BaseVAE(**KW), cfg, {"type": "none"}, {"type": "vae"}, gradient_clip_val=1.0)
    if configure:
        mod.configure_optimizers()
    return mod


def _known_ema(mod):
    """Overwrite the flat EMA buffer with distinct values (element i of the live region holds i + 0.25; the padding
    stays zero) and return {name: logical tensor} read through the KRSC view."""
    opt, flat = mod.optimizer, mod.flat
    opt.ema.zero_()
    for p, off in zip(flat.params, flat.offsets):
        opt.ema[off:off + p.numel()] = torch.arange(off, off + p.numel(), dtype=torch.float32) + 0.25
    return {n: FlatParameters._view(opt.ema, off, p).clone() for n, p, off in zip(flat.names, flat.params, flat.offsets)}


def _roundtrip(ck):
    """Through torch.save / torch.load(weights_only=True), as a file would go."""
    buf = io.BytesIO()
    torch.save(ck, buf)
    buf.seek(0)
    return torch.load(buf, map_location="cpu", weights_only=True)


@pytest.mark.parametrize("bad", [1.0, -0.1, "x"])
def test_invalid_ema_decay_is_rejected(bad):
    with pytest.raises(ValueError, match="ema_decay"):
        _module(bad, configure=False)
    flat = FlatParameters(torch.nn.Linear(3, 2))
    from medvae_disentangled_multimodal_amd.optim import Adam, AdamW, FusedAdam
    for make in (FusedAdam, Adam, AdamW):
        with pytest.raises(ValueError, match="ema_decay"):
            make(flat, ema_decay=bad)


def test_ema_buffer_starts_as_the_weights():
    mod = _module(0.99)
    opt, flat = mod.optimizer, mod.flat
    assert opt.ema_decay == 0.99
    assert opt.ema.dtype == torch.float32 and opt.ema.shape == (flat.numel,)
    assert opt.ema.data_ptr() != flat.data.data_ptr()
    assert torch.equal(opt.ema, flat.data)  # padding included
    used = torch.zeros(flat.numel, dtype=torch.bool)
    for p, off in zip(flat.params, flat.offsets):
        used[off:off + p.numel()] = True
    assert bool((~used).any()) and not bool(opt.ema[~used].any())
    assert float(opt.ema.abs().max()) > 0
    assert set(opt.state_dict()) == {"exp_avg", "exp_avg_sq", "steps", "param_groups", "ema"}
    # the optimizer's own state round trip carries the average
    other = _module(0.99, seed=1)
    assert not torch.equal(other.optimizer.ema, opt.ema)
    other.optimizer.load_state_dict(opt.state_dict())
    assert torch.equal(other.optimizer.ema, opt.ema)
    # ema_decay = 0 is allowed (the average is the weights after every step)
    assert _module(0).optimizer.ema_decay == 0.0


def test_no_ema_without_the_key():
    for mod in (_module(), _module(configure=False, ema_decay=None)):
        if mod.optimizer is None:
            mod.configure_optimizers()
        assert mod.optimizer.ema is None and mod.optimizer.ema_decay is None
        assert set(mod.optimizer.state_dict()) == {"exp_avg", "exp_avg_sq", "steps", "param_groups"}
        assert {k for k in mod.state_dict() if k.startswith("model.")} == {f"model.{k}" for k in mod.model.state_dict()}
        assert not any("ema" in k for k in mod.state_dict())
        with pytest.raises(RuntimeError, match="EMA is not enabled"):
            with mod.ema_scope():
                pass
        with pytest.raises(RuntimeError, match="no EMA"):
            mod.optimizer.swap_ema()
        ck = checkpoint.lightning_checkpoint(mod)
        assert "ema_state" not in ck
        with pytest.raises(RuntimeError, match="no EMA"):
            checkpoint.lightning_checkpoint(mod, weights="ema")
    # the module's own keys are the same with the average on: it lives in the optimizer
    assert set(_module(0.9).state_dict()) == set(_module().state_dict())


def test_ema_scope_refuses_an_open_window():
    mod = _module(0.9)
    mod._accum_pos = 1
    with pytest.raises(RuntimeError, match="accumulation window"):
        with mod.ema_scope():
            pass


def test_checkpoint_carries_ema_state():
    mod = _module(0.75)
    want = _known_ema(mod)
    # a 4-D weight whose Cin differs from kh * kw: a wrong permutation of the KRSC view cannot pass unseen
    name = next(n for n, p in zip(mod.flat.names, mod.flat.params) if p.dim() == 4 and p.shape[2] == 3 and
                p.shape[1] != 9 and p.shape[0] != p.shape[1])
    ck = checkpoint.lightning_checkpoint(mod, epoch=2)
    live = checkpoint.lightning_checkpoint(_module())
    assert set(ck) == set(live) | {"ema_state"}
    assert list(ck["state_dict"]) == list(live["state_dict"])
    for k, v in ck["state_dict"].items():  # the live weights, untouched by the average
        assert torch.equal(v, mod.model.state_dict()[k[len("model."):]])
    es = _roundtrip(ck)["ema_state"]
    assert es["decay"] == 0.75 and isinstance(es["decay"], float)
    assert list(es["weights"]) == mod.flat.names
    for n, p in zip(mod.flat.names, mod.flat.params):
        w = es["weights"][n]
        assert w.shape == p.shape and w.is_contiguous() and w.device.type == "cpu"
        assert torch.equal(w, want[n]), n
    # the logical tensor, element by element: [o, i, r, s] sits at ((o * kh + r) * kw + s) * cin + i of the flat slot
    p = mod.flat.params[mod.flat.index_of(name)]
    off = mod.flat.offsets[mod.flat.index_of(name)]
    co, ci, kh, kw = p.shape
    for o, i, r, s in [(0, 0, 0, 0), (1, 2, 0, 1), (co - 1, ci - 1, kh - 1, kw - 1), (3, 1, 2, 0)]:
        assert float(es["weights"][name][o, i, r, s]) == off + ((o * kh + r) * kw + s) * ci + i + 0.25

    # table row 1: the checkpoint has ema_state, EMA is enabled -> into the flat EMA buffer, bitwise, padding zero
    fresh = _module(0.75, seed=5)
    assert not torch.equal(fresh.optimizer.ema, mod.optimizer.ema)
    checkpoint.load_checkpoint(fresh, _roundtrip(ck))
    assert torch.equal(fresh.optimizer.ema, mod.optimizer.ema)
    assert torch.equal(fresh.flat.data, mod.flat.data)
    assert not torch.equal(fresh.optimizer.ema, fresh.flat.data)
    # ... also for a module whose optimizer is not configured yet
    lazy = _module(0.75, seed=6, configure=False)
    checkpoint.load_checkpoint(lazy, _roundtrip(ck))
    assert lazy.optimizer is not None and torch.equal(lazy.optimizer.ema, mod.optimizer.ema)

    # table row 2: no ema_state, EMA enabled -> the average restarts from the loaded weights
    fresh = _module(0.75, seed=5)
    _known_ema(fresh)
    checkpoint.load_checkpoint(fresh, _roundtrip(live))
    assert torch.equal(fresh.optimizer.ema, fresh.flat.data)
    assert torch.equal(fresh.flat.data, _module().flat.data)

    # table row 3: ema_state in the file, EMA not enabled -> ignored
    plain = _module(seed=5)
    checkpoint.load_checkpoint(plain, _roundtrip(ck))
    assert plain.optimizer.ema is None
    assert torch.equal(plain.flat.data, mod.flat.data)


def test_checkpoint_of_the_averaged_weights():
    mod = _module(0.75)
    want = _known_ema(mod)
    buffers = {k: v for k, v in mod.model.state_dict().items() if k not in want}
    ck = _roundtrip(checkpoint.lightning_checkpoint(mod, epoch=1, weights="ema"))
    assert ck["optimizer_states"] == [] and "ema_state" not in ck
    assert list(ck["state_dict"]) == list(checkpoint.lightning_checkpoint(mod)["state_dict"])
    for n in mod.flat.names:
        assert torch.equal(ck["state_dict"][f"model.{n}"], want[n]), n
    for k, v in buffers.items():
        assert torch.equal(ck["state_dict"][f"model.{k}"], v)
    # it loads as a model: strictly, into a module with or without an average of its own
    for ema in (None, 0.5):
        other = _module(ema, seed=3)
        checkpoint.load_checkpoint(other, ck)
        assert torch.equal(other.flat.data, mod.optimizer.ema)
        if ema is not None:
            assert torch.equal(other.optimizer.ema, other.flat.data)
    with pytest.raises(ValueError, match="weights"):
        checkpoint.lightning_checkpoint(mod, weights="both")
