"""Exponential moving average of the weights inside the fused Adam step (mvae_multi_tensor_adam_ema, csrc/optim.hip),
the in-place buffer exchange (mvae_swap_buffers) and their use by the training module (optimizer_config["ema_decay"],
ema_scope, evaluate(use_ema=True), the weights="ema" checkpoint).

Kernel-level tests run on a bare module whose parameters have 3, 5, 64 and 65536 + 7 elements plus one conv weight
(8, 4, 3, 3): the empty 16-B body, the scalar tail, a tensor of two chunks and the KRSC view. No model forward runs.
Module-level tests use the tiny BaseVAE of the known-answer anchor (hidden 32, ch_mult (1, 2, 4), 28x28, batch 4).

Bound of the float64 comparisons. One update forms d = (float)decay and omd = (float)(1.0 - decay) (2^-24 relative
each), the products ema * d and omd * p (2^-24 each; one of them is folded into an FMA where the compiler contracts)
and their sum (2^-24): under 4 * 2^-24 = 2^-22 of the larger of |ema| and |p| per step. The error an earlier step left
in ema is multiplied by d < 1, so after K steps |ema - ema64| <= K * 2^-22 * max(|p|, |ema|), the maximum taken element
by element over the trajectory (the initial average, every post-step parameter, every float64 average)."""
import pytest
import torch

import exact_inputs as E

pytestmark = pytest.mark.gpu

SIZES = [3, 5, 64, 65536 + 7]
CONV = (8, 4, 3, 3)
MASKED, INF = 2, 1  # the tensor `used` masks out, the tensor that gets a non-finite gradient
KAT = dict(input_channels=3, latent_dim=16, hidden_channels=32, ch_mult=(1, 2, 4), num_res_blocks=1,
           attn_resolutions=[], dropout=0.0, resolution=28)
DIS = dict(num_modalities=5, shared_latent_dim=8, modality_latent_dim=8, hidden_channels=32, ch_mult=(1, 2, 4),
           num_res_blocks=1, attn_resolutions=[], dropout=0.0, resolution=28, modality_separation_weight=0.1,
           contrastive_weight=0.05)
DIS_LOSS = dict(type="disentangled_vae", recon_loss_type="mse", kl_weight=1.0, recon_weight=1.0,
                separation_weight=0.1, contrastive_weight=0.05)
B = 4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def _bare(dev, init=None, seed=17, **kw):
    """(flat, optimizer) over the bare module; init(shape) -> initial parameter values."""
    from medvae_disentangled_multimodal_amd.optim import FlatParameters, FusedAdam
    torch.manual_seed(seed)
    mod = torch.nn.Module()
    for i, s in enumerate([(n,) for n in SIZES] + [CONV]):
        mod.register_parameter(f"p{i}", torch.nn.Parameter(torch.randn(s) if init is None else init(s)))
    flat = FlatParameters(mod, dev)
    return flat, FusedAdam(flat, **kw)


def _owned(flat):
    m = torch.zeros(flat.numel, dtype=torch.bool)
    for p, off in zip(flat.params, flat.offsets):
        m[off:off + p.numel()] = True
    return m


def _set_grads(flat, it, inf=True):
    """The same seeded gradients for every optimizer of a test (step `it`), one tensor with an inf."""
    g = torch.Generator().manual_seed(100 + it)
    for j, p in enumerate(flat.params):
        v = torch.randn(p.shape, generator=g) * (3.0 if it == 0 else 0.3)
        if inf and j == INF and it == 1:
            v.view(-1)[2] = float("inf")
        p.grad.copy_(v.to(p.device))


def _used(flat, dev):
    u = torch.ones(len(flat.params), dtype=torch.int32, device=dev)
    u[MASKED] = 0
    return u


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _recurrence(e0, traj, decay):
    """(float64 average after the trajectory, element-wise magnitude max(|p|, |ema|) over it)."""
    e = e0.detach().double().cpu()
    mag = e.abs()
    for p in traj:
        p = p.detach().double().cpu()
        e = decay * e + (1.0 - decay) * p
        mag = torch.maximum(mag, torch.maximum(p.abs(), e.abs()))
    return e, mag


def _check_recurrence(ema, e0, traj, decay, what):
    ref, mag = _recurrence(e0, traj, decay)
    bound = len(traj) * 2.0 ** -22 * mag
    err = (ema.detach().double().cpu() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max |ema - ema64| {float(err.max()):.3e}, worst error / bound {worst:.3f}")
    E.assert_within(ema, ref, bound, ["flat"], what)


def _module(dev, ema=None, n=1, seed=3, lr=1e-3, cls="BaseVAE", kw=KAT, loss=None):
    import medvae_disentangled_multimodal_amd as M
    torch.manual_seed(seed)
    model = getattr(M, cls)(**kw).to(dev)
    oc = {"type": "adamw", "lr": lr}
    if ema is not None:
        oc["ema_decay"] = ema
    mod = M.VAELightningModule(model, oc, {"type": "none"}, loss or {"type": "vae"}, gradient_clip_val=1.0,
                               accumulate_grad_batches=n)
    mod.configure_optimizers()
    return mod


def _micro(dev, i, zc=16):
    g = torch.Generator().manual_seed(40 + i)
    x = (torch.randint(0, 256, (B, 3, 28, 28), generator=g).float() / 255 * 2 - 1).to(dev)
    eps = torch.randn(B, zc, 7, 7, generator=g).to(dev)
    return (x, torch.zeros(B, 1, dtype=torch.long, device=dev)), eps


# ---------------------------------------------------------------------------------------------------------------------
# 1 .. 4: the kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam_l2"])
def test_adam_is_unchanged_by_the_ema_form(dev, decoupled):
    kw = dict(lr=1e-2, betas=(0.9, 0.999), weight_decay=1e-2, decoupled=decoupled, max_grad_norm=1.0)
    fa, a = _bare(dev, **kw)
    fb, b = _bare(dev, ema_decay=0.999, **kw)
    assert a.ema is None and torch.equal(b.ema, fb.data) and torch.equal(fa.data, fb.data)
    for it in range(3):
        for f, o in ((fa, a), (fb, b)):
            _set_grads(f, it)
            o.step(used=_used(f, dev))
        torch.cuda.synchronize()
        for name, x, y in (("params", fa.data, fb.data), ("grads", fa.grad, fb.grad), ("exp_avg", a.exp_avg, b.exp_avg),
                           ("exp_avg_sq", a.exp_avg_sq, b.exp_avg_sq), ("steps", a.steps, b.steps),
                           ("scalars", a.scalars, b.scalars)):
            assert torch.equal(_bits(x), _bits(y)), (it, name)
    assert [int(s) for s in a.steps.cpu()] == [3, 3, 0, 3, 3]
    assert not torch.equal(b.ema, fb.data)


def test_ema_update_is_exact(dev):
    gen = torch.Generator().manual_seed(5)

    def ints(shape):  # integer multiples of 8 below 2^12
        return (torch.randint(-511, 512, tuple(shape), generator=gen) * 8).float()
    flat, opt = _bare(dev, init=ints, lr=0.0, weight_decay=0.0, ema_decay=0.5)
    owned = _owned(flat)
    e0 = torch.zeros(flat.numel)
    e0[owned] = ints((int(owned.sum()),))
    opt.ema.copy_(e0.to(dev))
    p0 = flat.data.clone()
    assert float(p0.abs().max()) < 2 ** 12 and float(e0.abs().max()) < 2 ** 12
    for it in range(3):
        _set_grads(flat, it)
        opt.step(used=_used(flat, dev))
    torch.cuda.synchronize()
    assert torch.equal(_bits(flat.data), _bits(p0))  # lr = 0: p + (-0) * (m / denom)
    exp = e0.clone()
    for _ in range(3):  # exact in fp32: multiples of 4, 2, 1 below 2^12
        exp = 0.5 * exp + 0.5 * p0.cpu()
    exp64, _ = _recurrence(e0, [p0] * 3, 0.5)
    assert torch.equal(exp.double(), exp64)
    E.assert_exact(opt.ema, exp, ["flat"], "ema after three steps of decay 0.5")
    off, n = flat.offsets[MASKED], flat.params[MASKED].numel()
    assert int(opt.steps[MASKED]) == 0
    assert not torch.equal(opt.ema[off:off + n].cpu(), e0[off:off + n])  # the tensor without a gradient averaged too
    assert not bool(opt.ema.cpu()[~owned].any())  # the padding is still zero
    assert not torch.equal(opt.ema.cpu()[owned], p0.cpu()[owned])


def test_ema_against_float64(dev):
    K, decay = 5, 0.999
    flat, opt = _bare(dev, lr=1e-3, weight_decay=1e-2, decoupled=True, ema_decay=decay)
    opt.ema.mul_(0.75)  # (exact; an average that starts away from the weights)
    e0, traj = opt.ema.clone(), []
    for it in range(K):
        _set_grads(flat, it, inf=False)
        opt.step()
        traj.append(flat.data.clone())
    torch.cuda.synchronize()
    assert not torch.equal(traj[0], traj[-1])
    _check_recurrence(opt.ema, e0, traj, decay, f"bare module, {K} steps of decay {decay}")


@pytest.mark.parametrize("n,shift", [(1, 0), (3, 0), (4, 0), (65536 + 7, 0), (65536 + 7, 1), (2 * 2048 * 1024 + 5, 0)],
                         ids=["1", "3", "4", "65543", "65543-unaligned", "grid-stride"])
def test_swap_buffers(dev, n, shift):
    """Lengths below, at and above one 16-B group, past one chunk, from a start that is not 16-B aligned (the scalar
    form), and more groups than the launch has threads (the grid-stride loop)."""
    from medvae_disentangled_multimodal_amd import _lib
    g = torch.Generator().manual_seed(n)
    a0, b0 = torch.randn(n + shift + 3, generator=g).to(dev), torch.randn(n + shift + 3, generator=g).to(dev)
    a, b = a0.clone(), b0.clone()
    st = torch.cuda.current_stream(dev).cuda_stream

    def swap():
        _lib.call("mvae_swap_buffers", a.data_ptr() + 4 * shift, b.data_ptr() + 4 * shift, n, st)
    swap()
    torch.cuda.synchronize()
    sl = slice(shift, shift + n)
    assert torch.equal(_bits(a[sl]), _bits(b0[sl])) and torch.equal(_bits(b[sl]), _bits(a0[sl]))
    for t, t0 in ((a, a0), (b, b0)):  # nothing outside the n elements is touched
        assert torch.equal(_bits(t[:shift]), _bits(t0[:shift])) and torch.equal(_bits(t[shift + n:]), _bits(t0[shift + n:]))
    swap()
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(a0)) and torch.equal(_bits(b), _bits(b0))


def test_swap_buffers_rejects_null_and_empty(dev):
    from medvae_disentangled_multimodal_amd import _lib
    lib = _lib.load()
    a, b = torch.ones(8, device=dev), torch.zeros(8, device=dev)
    for args in ((None, b.data_ptr(), 8), (a.data_ptr(), None, 8), (a.data_ptr(), b.data_ptr(), 0)):
        assert lib.mvae_swap_buffers(*args, None) == -1
        assert b"swap_buffers" in lib.mvae_last_error()
        with pytest.raises(RuntimeError, match="swap_buffers"):
            _lib.call("mvae_swap_buffers", *args, None)
    torch.cuda.synchronize()
    assert bool((a == 1).all()) and bool((b == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 5 .. 9: the training module
# ---------------------------------------------------------------------------------------------------------------------
def test_fit_steps_average_the_weights(dev):
    decay = 0.999
    mod = _module(dev, ema=decay)
    e0, traj = mod.optimizer.ema.clone(), []
    assert torch.equal(e0, mod.flat.data)
    for i in range(3):
        batch, eps = _micro(dev, i)
        mod.fit_step(batch, 0, eps=eps)
        traj.append(mod.flat.data.clone())
    torch.cuda.synchronize()
    owned = _owned(mod.flat)
    assert not torch.equal(mod.optimizer.ema, mod.flat.data)
    assert float((mod.optimizer.ema != mod.flat.data).cpu()[owned].float().mean()) > 0.9
    _check_recurrence(mod.optimizer.ema, e0, traj, decay, "three fit_steps")
    assert not bool(mod.optimizer.ema.cpu()[~owned].any())


def test_graphed_steps_average_like_eager_steps(dev):
    micro = [_micro(dev, i) for i in range(4)]

    def run(graphed):
        mod = _module(dev, ema=0.9)
        mod.fit_step(micro[0][0], 0, eps=micro[0][1])
        for batch, eps in micro[1:]:
            (mod.fit_step_graphed if graphed else mod.fit_step)(batch, 0, eps=eps)
        torch.cuda.synchronize()
        return mod
    a, b = run(False), run(True)
    assert b._graph is not None and a.global_step_count == b.global_step_count == 4
    assert torch.equal(_bits(a.flat.data), _bits(b.flat.data))
    assert torch.equal(_bits(a.optimizer.ema), _bits(b.optimizer.ema))
    assert not torch.equal(b.optimizer.ema, b.flat.data)
    b.teardown()


def test_one_update_per_accumulation_window(dev, monkeypatch):
    from medvae_disentangled_multimodal_amd import _lib
    decay = 0.9
    mod = _module(dev, ema=decay, n=2)
    seen, orig = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (seen.append(name), orig(name, *a))[1])
    e0, traj, calls = mod.optimizer.ema.clone(), [], []
    for i in range(4):
        before = mod.optimizer.ema.clone()
        seen.clear()
        batch, eps = _micro(dev, i)
        mod.fit_step(batch, 0, eps=eps)
        calls.append((seen.count("mvae_multi_tensor_adam_ema"), seen.count("mvae_multi_tensor_adam")))
        if i % 2 == 0:  # a micro-batch that leaves the window open: no update
            assert torch.equal(_bits(mod.optimizer.ema), _bits(before))
        else:
            traj.append(mod.flat.data.clone())
    torch.cuda.synchronize()
    assert calls == [(0, 0), (1, 0), (0, 0), (1, 0)]
    assert mod.global_step_count == 2 and len(traj) == 2
    _check_recurrence(mod.optimizer.ema, e0, traj, decay, "two windows of two micro-batches")
    # one update more or fewer is far outside the bound
    one, mag = _recurrence(e0, traj[:1], decay)
    two, _ = _recurrence(e0, traj, decay)
    assert float(((one - two).abs() / (2 * 2.0 ** -22 * mag).clamp_min(1e-300)).max()) > 100


def test_evaluate_with_the_averaged_weights(dev):
    import medvae_disentangled_multimodal_amd as M
    from medvae_disentangled_multimodal_amd import checkpoint
    from medvae_disentangled_multimodal_amd.evaluation import evaluate_model

    def trained():
        mod = _module(dev, ema=0.9, lr=1e-2)
        for i in range(3):
            batch, eps = _micro(dev, i)
            mod.fit_step(batch, 0, eps=eps)
        return mod

    def evaluate(mod, **kw):
        torch.manual_seed(123)  # (validation draws its reparameterisation noise)
        return {k: v.clone() for k, v in mod.evaluate(batch, "val", **kw).items()}

    mod, twin = trained(), trained()
    batch, _ = _micro(dev, 7)
    p0, e0 = mod.flat.data.clone(), mod.optimizer.ema.clone()
    assert not torch.equal(p0, e0)
    with_ema = evaluate(mod, use_ema=True)
    assert torch.equal(_bits(mod.flat.data), _bits(p0)) and torch.equal(_bits(mod.optimizer.ema), _bits(e0))
    live = evaluate(mod)
    assert float(with_ema["val/loss"]) != float(live["val/loss"])
    assert float(with_ema["val/mse"]) != float(live["val/mse"])

    # a second module holding the averaged weights as its own, through the weights="ema" checkpoint
    other = _module(dev, seed=9)
    checkpoint.load_checkpoint(other, checkpoint.lightning_checkpoint(mod, weights="ema"))
    assert torch.equal(_bits(other.flat.data), _bits(e0))
    ref = evaluate(other)
    assert set(ref) == set(with_ema) and "val/loss" in ref
    for k in ref:
        assert torch.equal(_bits(ref[k]), _bits(with_ema[k])), k
    torch.manual_seed(123)
    m_ema, _ = evaluate_model(mod, [batch], use_ema=True)
    torch.manual_seed(123)
    m_ref, _ = evaluate_model(other, [batch])
    assert m_ema == m_ref
    assert torch.equal(_bits(mod.flat.data), _bits(p0)) and torch.equal(_bits(mod.optimizer.ema), _bits(e0))

    # inside the scope the model holds the average; no optimisation step may run; the weights come back when the body raises
    with pytest.raises(ZeroDivisionError):
        with mod.ema_scope():
            assert torch.equal(_bits(mod.flat.data), _bits(e0)) and torch.equal(_bits(mod.optimizer.ema), _bits(p0))
            for step in (mod.fit_step, mod.fit_step_graphed):
                with pytest.raises(RuntimeError, match="ema_scope"):
                    step(batch, 0)
            1 / 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(mod.flat.data), _bits(p0)) and torch.equal(_bits(mod.optimizer.ema), _bits(e0))

    # a following step is the one of a run that never entered the scope
    nb, neps = _micro(dev, 3)
    la, lb = mod.fit_step(nb, 0, eps=neps), twin.fit_step(nb, 0, eps=neps)
    torch.cuda.synchronize()
    assert float(la) == float(lb)
    assert torch.equal(_bits(mod.flat.data), _bits(twin.flat.data))
    assert torch.equal(_bits(mod.optimizer.ema), _bits(twin.optimizer.ema))
    assert not torch.equal(mod.flat.data, p0)

    plain = _module(dev)
    with pytest.raises(RuntimeError, match="EMA is not enabled"):
        plain.evaluate(batch, use_ema=True)


def test_absent_modality_head_is_averaged_without_a_step(dev):
    decay = 0.9
    mod = _module(dev, ema=decay, cls="DisentangledConditionalVAE", kw=DIS, loss=DIS_LOSS)
    mod.optimizer.ema.mul_(0.5)  # (exact; away from the weights, so an average that did not move shows)
    e0, p0 = mod.optimizer.ema.clone(), mod.flat.data.clone()
    (x, labels), eps = _micro(dev, 0)
    idx = torch.tensor([0, 1, 2, 3], device=dev)  # no sample of modality 4
    mod.fit_step((x, labels, torch.nn.functional.one_hot(idx, 12).float(), idx), 0, eps=eps)
    torch.cuda.synchronize()
    steps, absent = mod.optimizer.steps.cpu(), 0
    for j, (name, p, off) in enumerate(zip(mod.flat.names, mod.flat.params, mod.flat.offsets)):
        sl = slice(off, off + p.numel())
        if mod.model.parameter_modality(name) == 4:
            absent += 1
            assert int(steps[j]) == 0 and torch.equal(_bits(mod.flat.data[sl]), _bits(p0[sl])), name
            assert not torch.equal(mod.optimizer.ema[sl], e0[sl]), name
        elif mod.model.parameter_modality(name) in (-1, 0, 1, 2, 3):
            assert int(steps[j]) == 1, name
    assert absent >= 2
    _check_recurrence(mod.optimizer.ema, e0, [mod.flat.data], decay, "one step without modality 4")
