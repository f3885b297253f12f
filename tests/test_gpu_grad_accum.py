"""Gradient accumulation on the GPU (VAELightningModule(accumulate_grad_batches=N)).

A window of N fit_step calls must leave, before the optimizer phase, the flat gradient sum_i g_i / N of its micro-batches
(every producer adds into its slot; one that overwrites misses by order 1), step the optimizer once, prepare the weight
formats once, step every modality head any micro-batch used, and give the same parameters eagerly, replayed from graphs
and data-parallel.

Tiny model throughout: hidden 32, ch_mult (1, 2), one res block, attention at 8, resolution 16, latent 4, micro-batch 4.

Bars: the accumulated gradient is held per parameter tensor to ||acc - sum g_i / N|| / ||sum |g_i| / N|| <= 3e-5 (float64
sums), the project's 3xBF16-vs-float64 bar (tests/test_gpu_kernels.py); the Winograd weight gradient to
the 2e-4 conv bar of tests/test_gpu_winograd.py; the whole step against the CPU oracle to the post-step bar of
tests/test_gpu_parity.py; the data-parallel step to the bar of tests/test_gpu_ddp.py."""
import os
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import exact_inputs as E

pytestmark = pytest.mark.gpu
CL = torch.channels_last
GRAD_TOL = 3e-5   # DESIGN section 3 / tests/test_gpu_kernels.py
WINO_TOL = 2e-4   # tests/test_gpu_winograd.py CONV_TOL
B = 4

TINY = dict(hidden_channels=32, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[8], resolution=16)
MODELS = {
    "attn": ("BaseVAE", dict(TINY, input_channels=3, latent_dim=4), {"type": "vae"}),
    "linattn": ("BaseVAE", dict(TINY, input_channels=3, latent_dim=4, use_linear_attn=True), {"type": "vae"}),
    "cvae": ("ConditionalVAE", dict(TINY, input_channels=3, latent_dim=4, condition_method="concat"), {"type": "vae"}),
    "dis": ("DisentangledConditionalVAE", dict(TINY, num_modalities=5, shared_latent_dim=2, modality_latent_dim=2,
                                                 modality_separation_weight=0.1, contrastive_weight=0.05),
            {"type": "disentangled_vae"}),
}
# every head of the disentangled model sees a sample within the first two micro-batches
DIS_IDX = [[0, 1, 2, 0], [3, 4, 3, 1], [2, 4, 0, 1]]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _module(kind, dev, n=1, precision="32", dropout=0.0, opt=None):
    import medvae_disentangled_multimodal_amd as M
    cls, kw, loss = MODELS[kind]
    torch.manual_seed(3)
    model = getattr(M, cls)(**dict(kw, dropout=dropout)).to(dev)
    mod = M.VAELightningModule(model, opt or {"type": "adamw", "lr": 1e-3}, {"type": "none"}, loss,
                               gradient_clip_val=1.0, precision=precision, accumulate_grad_batches=n)
    mod.configure_optimizers()
    return mod


def _micro(kind, dev, i, idx=None, b=B):
    """(batch, eps) of micro-batch i: the same for every module of a test."""
    g = torch.Generator().manual_seed(40 + i)
    x = (torch.rand(b, 3, 16, 16, generator=g) * 2 - 1).to(dev)
    eps = torch.randn(b, 4, 8, 8, generator=g).to(dev)
    labels = torch.zeros(b, 1, dtype=torch.long, device=dev)
    if kind == "dis":
        ix = torch.tensor(DIS_IDX[i] if idx is None else idx, device=dev)
        return (x, labels, torch.nn.functional.one_hot(ix, 12).float(), ix), eps
    if kind == "cvae":
        ix = (torch.arange(b, device=dev) + 3 * i) % 12
        return (x, labels, torch.nn.functional.one_hot(ix, 12).float()), eps
    return (x, labels), eps


def _grad_alone(kind, dev, precision, i):
    """The flat gradient of micro-batch i alone: an N = 1 module with the same weights, _forward_backward only."""
    from medvae_disentangled_multimodal_amd import ops
    mod = _module(kind, dev, 1, precision)
    batch, eps = _micro(kind, dev, i)
    prev = ops.set_precision(precision)
    try:
        mod._forward_backward(batch, 0, eps)
    finally:
        ops.flat_weights_stale()
        ops.restore_math_mode(prev)
    torch.cuda.synchronize()
    return mod.flat.grad.detach().double().cpu()


def _window_grad(kind, dev, precision, n, calls, last_batch_at=None):
    """The flat gradient a window of `calls` micro-batches hands to the optimizer phase, the module after it."""
    mod = _module(kind, dev, n, precision)
    seen = []
    phase = mod._optimizer_phase

    def spy(*a, **k):
        seen.append(mod.flat.grad.detach().double().cpu())
        return phase(*a, **k)
    mod._optimizer_phase = spy
    for i in range(calls):
        batch, eps = _micro(kind, dev, i)
        mod.fit_step(batch, 0, eps=eps, last_batch=(i == last_batch_at))
        assert len(seen) == (1 if i == calls - 1 else 0)
    torch.cuda.synchronize()
    return seen[0], mod


_ALONE = {}


def _alone(kind, dev, precision):
    key = (kind, precision)
    if key not in _ALONE:
        _ALONE[key] = [_grad_alone(kind, dev, precision, i) for i in range(3)]
    return _ALONE[key]


def _check_accumulated(mod, acc, gs, n, what):
    """Per parameter tensor: ||acc - sum g_i / n|| / ||sum |g_i| / n|| <= GRAD_TOL, no live tensor's expectation zero."""
    exp = sum(gs) / n
    mag = sum(g.abs() for g in gs) / n
    dead = getattr(mod.model, "parameter_modality", lambda name: -1)
    bad = []
    for name, p, off in zip(mod.flat.names, mod.flat.params, mod.flat.offsets):
        sl = slice(off, off + p.numel())
        if dead(name) == -2:  # (a parameter no forward reads -- the disentangled model's modality_embedding: no gradient)
            assert not bool(exp[sl].any()) and not bool(acc[sl].any()), name
            continue
        assert bool(exp[sl].any()), f"{what}: the expected gradient of {name} is all zero"
        err = float((acc[sl] - exp[sl]).norm() / mag[sl].norm())
        print(f"{what} {name}: {err:.3e}")  # (every figure, before the assertion)
        if not err <= GRAD_TOL:
            bad.append((name, err))
    assert not bad, (what, f"{len(bad)} tensors beyond {GRAD_TOL}", bad[:6])


# 1 ------------------------------------------------------------------------------------------------------------------
def test_window_of_two_steps_once(dev):
    mod = _module("attn", dev, 2)
    p0 = mod.flat.data.clone()
    b0, e0 = _micro("attn", dev, 0)
    b1, e1 = _micro("attn", dev, 1)
    l0 = mod.fit_step(b0, 0, eps=e0)
    torch.cuda.synchronize()
    assert mod.global_step_count == 0 and mod.accumulating
    assert torch.equal(mod.flat.data, p0)  # no step yet
    assert int(mod.optimizer.steps.max()) == 0
    l1 = mod.fit_step(b1, 0, eps=e1)
    torch.cuda.synchronize()
    assert mod.global_step_count == 1 and not mod.accumulating
    assert bool((mod.optimizer.steps == 1).all())
    for name, p, off in zip(mod.flat.names, mod.flat.params, mod.flat.offsets):
        assert not torch.equal(mod.flat.data[off:off + p.numel()], p0[off:off + p.numel()]), f"{name} did not move"
    assert not l0.requires_grad and not l1.requires_grad and float(l0) != float(l1)
    # the returned and logged losses are the undivided ones
    one = _module("attn", dev, 1)
    assert float(one.fit_step(b0, 0, eps=e0)) == float(l0)


# 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
@pytest.mark.parametrize("kind", sorted(MODELS))
def test_accumulated_gradient_is_the_sum(dev, kind, precision, n):
    """Every micro-batch backpropagates its own undivided loss -- bitwise the backward it runs alone -- and the window's
    sum is divided by N once at the boundary, so only the fp32 adds into the slots and one division differ from the
    float64 sum, at N = 3 as at N = 2 (a 1 / 3 loss scale in every backward would re-round each bf16 / 3xBF16 operand:
    measured 1e-5 .. 3e-5 in "32", up to 1.7e-2 in "bf16-mixed", and order 1 on the biases whose exact gradient is 0
    and whose stored values are rounding noise)."""
    gs = _alone(kind, dev, precision)
    acc, mod = _window_grad(kind, dev, precision, n, n)
    assert mod.global_step_count == 1
    _check_accumulated(mod, acc, gs[:n], n, f"{kind}/{precision}/N={n}")


# 3 ------------------------------------------------------------------------------------------------------------------
def _exact_problem(n, ci, co, h, k, seed):
    g = torch.Generator().manual_seed(seed)
    return [(E.family_i((n, ci, h, h), g), E.family_i((n, co, h, h), g)) for _ in range(2)], E.family_i((co, ci, k, k), g)


@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
@pytest.mark.parametrize("k,n,ci,co,h", [(3, 2, 32, 64, 9), (1, 2, 32, 16, 8)], ids=["3x3", "1x1"])
def test_two_backward_passes_accumulate_exactly(dev, precision, k, n, ci, co, h):
    """Integer inputs (tests/exact_inputs.py family I): two backward passes of one conv into the same flat slot, weight
    and bias, give the integer sum bitwise -- in bf16-mixed through the packed-dy path."""
    from medvae_disentangled_multimodal_amd import ops
    pairs, wt = _exact_problem(n, ci, co, h, k, 7 * k)
    pad = (k // 2,) * 4
    _, _, wgrad = E.conv_ops(pairs[0][0].shape, wt.shape, 1, pad, False)
    E.check_exact(sum(wgrad(dy.abs(), x.abs()) for x, dy in pairs), 1.0, "wgrad sum")
    E.check_exact(sum(dy.abs().sum((0, 2, 3)) for _, dy in pairs), 1.0, "bias grad sum")
    exp_w = sum(wgrad(dy.double(), x.double()) for x, dy in pairs)
    exp_b = sum(dy.double().sum((0, 2, 3)) for _, dy in pairs)
    geom = ops.ConvGeom(k, k, 1, pad[0], pad[1], pad[2], pad[3], False)
    wd = wt.to(dev).contiguous(memory_format=CL).requires_grad_()
    bd = torch.zeros(co, device=dev).requires_grad_()
    wd._mvae_main_grad = torch.zeros_like(wd, memory_format=CL)
    bd._mvae_main_grad = torch.zeros_like(bd)
    prev = ops.set_precision(precision)
    try:
        for x, dy in pairs:
            xd = x.to(dev).contiguous(memory_format=CL).requires_grad_()
            ops.conv2d(xd, wd, bd, geom).backward(dy.to(dev).contiguous(memory_format=CL))
    finally:
        ops.restore_math_mode(prev)
    torch.cuda.synchronize()
    assert wd.grad is None and bd.grad is None
    E.assert_exact(wd._mvae_main_grad, exp_w, "kcrs", f"{k}x{k} {precision} dw over two passes")
    E.assert_exact(bd._mvae_main_grad, exp_b, "k", f"{k}x{k} {precision} db over two passes")


# 4 ------------------------------------------------------------------------------------------------------------------
def test_winograd_weight_gradient_accumulates(dev, monkeypatch):
    from medvae_disentangled_multimodal_amd import _lib, ops
    c, h = 512, 8
    geom = ops.ConvGeom(3, 3, 1, 1, 1, 1, 1, False)
    prev = ops.set_precision("32")
    try:
        n = next(i for i in range(1, 513) if ops._wino_ok(geom, i, h, h, c, c))  # (the size rule decides, not the test)
        g = torch.Generator().manual_seed(12)
        wt = torch.randn(c, c, 3, 3, generator=g) / (3 * c ** 0.5)
        xs = [torch.randn(n, c, h, h, generator=g) for _ in range(2)]
        dys = [torch.randn(n, c, h, h, generator=g) for _ in range(2)]
        seen, orig = [], _lib.call
        monkeypatch.setattr(_lib, "call", lambda name, *a: (seen.append(name), orig(name, *a))[1])
        wd = wt.to(dev).contiguous(memory_format=CL).requires_grad_()
        bd = torch.zeros(c, device=dev).requires_grad_()
        wd._mvae_main_grad = torch.zeros_like(wd, memory_format=CL)
        bd._mvae_main_grad = torch.zeros_like(bd)
        single = []
        for x, dy in zip(xs, dys):
            xd = x.to(dev).contiguous(memory_format=CL).requires_grad_()
            before = wd._mvae_main_grad.clone()
            ops.conv2d(xd, wd, bd, geom).backward(dy.to(dev).contiguous(memory_format=CL))
            single.append(wd._mvae_main_grad - before)
        torch.cuda.synchronize()
    finally:
        ops.restore_math_mode(prev)
    assert seen.count("mvae_winograd_wgrad_output") == 2
    assert all(float(t.abs().max()) > 0 for t in single)  # the second pass added, all over the tensor
    # float64 weight gradient of both passes at once (it is linear in the batch), for every 64th output channel (8 of
    # them, from both 256-wide GEMM tiles: the whole tensor in float64 on the CPU would take a minute)
    sel = torch.arange(0, c, 64)
    w0 = wt[sel].double().requires_grad_()
    torch.nn.functional.conv2d(torch.cat(xs).double(), w0, None, padding=1).backward(torch.cat(dys)[:, sel].double())
    got = wd._mvae_main_grad.double().cpu()[sel]
    err = float((got - w0.grad).norm() / w0.grad.norm())
    print(f"winograd dw over two passes (n = {n}): {err:.3e}")
    assert err <= WINO_TOL, err
    eb = float((bd._mvae_main_grad.double().cpu() - torch.cat(dys).double().sum((0, 2, 3))).norm() /
               torch.cat(dys).double().sum((0, 2, 3)).norm())
    assert eb <= 1e-5, eb


# 5 ------------------------------------------------------------------------------------------------------------------
def test_window_matches_the_oracle_step(dev):
    """base_c1_full (a case tests/test_gpu_parity.py steps), its batch of 2 as two micro-batches of 1, N = 2, against
    oracle/torch_ref.py run the torch way: (loss / 2).backward() twice, clip, AdamW. Bar: the parity file's post-step
    bar (|dp| <= 2 lr everywhere, < 0.01 lr for >= 98 % of the elements of the selected tensors)."""
    import medvae_disentangled_multimodal_amd as M
    from cases import CASES, FULL_GRADS
    from golden_io import golden_state, load_case
    from oracle import torch_ref as R
    name = "base_c1_full"
    meta, data = load_case(name)
    case = CASES[name]
    x, eps = torch.from_numpy(data["in.x"]), torch.from_numpy(data["in.eps"])
    assert x.shape[0] == 2
    P = golden_state(meta)
    arch = R.make_arch(case["cls"], case["kwargs"])
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    lc = case["loss"]
    ref_losses = []
    for i in range(2):
        out = R.forward(leaves, arch, x[i:i + 1], None, eps[i:i + 1])
        loss = R.vae_loss(out, x[i:i + 1], lc.get("recon_weight", 1.0), lc.get("kl_weight", 1.0),
                          lc.get("recon_loss_type", "mse"))["loss"]
        ref_losses.append(float(loss))
        (loss / 2).backward()
    grads = {k: t.grad.clone() for k, t in leaves.items() if t.grad is not None}
    R.clip_grads(grads, case["clip"])
    oc = case["optimizer"]
    newP = {k: v.detach().clone() for k, v in P.items()}
    for k, g in grads.items():
        R.adam_step(newP[k], g, torch.zeros_like(g), torch.zeros_like(g), 1, oc["lr"], tuple(oc["betas"]), 1e-8,
                    oc["weight_decay"], oc["type"] == "adamw")

    model = getattr(M, case["cls"])(**case["kwargs"])
    model.load_state_dict(golden_state(meta))
    mod = M.VAELightningModule(model.to(dev), oc, {"type": "none"}, lc, gradient_clip_val=case["clip"],
                               accumulate_grad_batches=2)
    mod.configure_optimizers()
    for i in range(2):
        xb = x[i:i + 1].to(dev)
        loss = mod.fit_step((xb, torch.zeros(1, 1, dtype=torch.long, device=dev)), 0, eps=eps[i:i + 1].to(dev))
        assert abs(float(loss) - ref_losses[i]) <= 1e-3 * abs(ref_losses[i])
    torch.cuda.synchronize()
    assert mod.global_step_count == 1
    lr = oc["lr"]
    names = mod.flat.names
    for k in names:
        d = (mod.flat.params[names.index(k)].detach().cpu() - newP[k]).abs()
        assert float(d.max()) <= 2.0 * lr * 1.001 + 1e-7, k
    for k in FULL_GRADS[name]:
        d = (mod.flat.params[names.index(k)].detach().cpu() - newP[k]).abs()
        frac = float((d > 0.01 * lr).float().mean())
        print(f"{k}: max |dp| {float(d.max()):.3e}, fraction beyond 0.01 lr {frac:.4f}")
        assert frac < 0.02, k


# 6 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_weight_formats_prepared_once_per_window(dev, precision, monkeypatch):
    from medvae_disentangled_multimodal_amd import _lib, ops
    mod = _module("attn", dev, 3, precision)
    micro = [_micro("attn", dev, i) for i in range(3)]
    for _ in range(2):  # two windows: the re-layout table is learned in the first and built for the second
        for batch, eps in micro:
            mod.fit_step(batch, 0, eps=eps)
    count = {"prep": 0, "tables": 0}
    prep, tables = ops.prep_flat_weights, ops._prep_transposed
    monkeypatch.setattr(ops, "prep_flat_weights", lambda *a: (count.__setitem__("prep", count["prep"] + 1), prep(*a))[1])
    monkeypatch.setattr(ops, "_prep_transposed",
                        lambda *a: (count.__setitem__("tables", count["tables"] + 1), tables(*a))[1])
    seen, orig = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (seen.append(name), orig(name, *a))[1])
    per_micro = []
    for batch, eps in micro:
        seen.clear()
        mod.fit_step(batch, 0, eps=eps)
        per_micro.append(list(seen))
    torch.cuda.synchronize()
    assert count == {"prep": 1, "tables": 1}
    assert mod.global_step_count == 3 and not ops._FLATW.fresh and not ops._WT.fresh  # stale after the optimizer step
    conv = ("mvae_split_bf16", "mvae_pack_bf16", "mvae_conv_weight_transpose", "mvae_conv_weight_transpose_batched")
    launches = [{k: s.count(k) for k in conv} for s in per_micro]
    print(precision, launches)
    assert launches[0]["mvae_conv_weight_transpose_batched"] == 1
    for later in launches[1:]:
        # the later micro-batches read the first one's prepared copies: no batched re-layout, and no more per-conv
        # weight conversions than the micro-batch that ran the prep
        assert later["mvae_conv_weight_transpose_batched"] == 0
        assert later["mvae_conv_weight_transpose"] <= launches[0]["mvae_conv_weight_transpose"]
    assert launches[1] == launches[2]
    assert per_micro[0].count("mvae_multi_tensor_adam") == 0 and per_micro[2].count("mvae_multi_tensor_adam") == 1


# 7 ------------------------------------------------------------------------------------------------------------------
def test_usage_mask_is_the_union_of_the_window(dev):
    mod = _module("dis", dev, 2)
    p0 = mod.flat.data.clone()
    for i, m in enumerate((0, 3)):
        batch, eps = _micro("dis", dev, i, idx=[m] * B)
        mod.fit_step(batch, 0, eps=eps)
    torch.cuda.synchronize()
    steps = mod.optimizer.steps.cpu()
    heads = 0
    for j, (name, p, off) in enumerate(zip(mod.flat.names, mod.flat.params, mod.flat.offsets)):
        m = mod.model.parameter_modality(name)
        same = torch.equal(mod.flat.data[off:off + p.numel()], p0[off:off + p.numel()])
        if m in (0, 3) or m == -1:
            assert int(steps[j]) == 1 and not same, name
            heads += m >= 0
        else:
            assert int(steps[j]) == 0 and same, name
    assert heads >= 4  # both modalities' heads were there to be checked


# 8 ------------------------------------------------------------------------------------------------------------------
def test_early_close_divides_by_n(dev):
    gs = _alone("attn", dev, "32")
    acc, mod = _window_grad("attn", dev, "32", 4, 3, last_batch_at=2)
    assert mod.global_step_count == 1 and not mod.accumulating
    assert bool((mod.optimizer.steps == 1).all())
    _check_accumulated(mod, acc, gs, 4, "early close N=4")


# 9 ------------------------------------------------------------------------------------------------------------------
def test_replayed_windows_match_eager_windows_bitwise(dev):
    """N = 2, dropout 0.1: one eager window, then two windows replayed from the three captured pieces, against three
    eager windows. The captured pieces freeze the host dropout seeds drawn while recording and advance the device salt
    once per micro-batch; the eager run is given the same seeds and salt."""
    from medvae_disentangled_multimodal_amd import encoder_decoder as ED
    from medvae_disentangled_multimodal_amd import ops
    salt = ops.dropout_salt(dev)
    s0 = salt.clone()
    micro = [_micro("attn", dev, i) for i in range(2)]

    def run(graphed):
        salt.copy_(s0)
        mod = _module("attn", dev, 2, dropout=0.1)
        ED.set_dropout_seed(5)
        for batch, eps in micro:
            mod.fit_step(batch, 0, eps=eps)
        losses = []
        for _ in range(2):
            ED.set_dropout_seed(77)  # (replays: drawn once, by the recording of the first and the later piece, in order)
            for batch, eps in micro:
                if graphed:
                    losses.append(float(mod.fit_step_graphed(batch, 0, eps=eps)))
                else:
                    salt.add_(1)
                    losses.append(float(mod.fit_step(batch, 0, eps=eps)))
        torch.cuda.synchronize()
        return mod, losses

    a, la = run(False)
    b, lb = run(True)
    assert b._graph is not None and {"graph", "graph_next", "graph_opt"} <= set(b._graph)
    assert a.global_step_count == b.global_step_count == 3
    assert la == lb
    assert torch.equal(a.flat.data, b.flat.data)
    assert torch.equal(a.optimizer.exp_avg, b.optimizer.exp_avg)
    assert torch.equal(a.optimizer.steps, b.optimizer.steps)
    b.teardown()


# 10 -----------------------------------------------------------------------------------------------------------------
def _dp_micro(i):
    g = torch.Generator().manual_seed(90 + i)
    return torch.rand(B, 3, 16, 16, generator=g) * 2 - 1, torch.randn(B, 4, 8, 8, generator=g)


def _dp_worker(rank, world, init_file, out_file):
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    from medvae_disentangled_multimodal_amd import ddp
    dev = torch.device("cuda:0")
    mod = _module("attn", dev, 2)
    dp = ddp.DataParallel(mod, bucket_bytes=64 << 10)
    calls = []
    orig = dist.all_reduce

    def counting(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    dist.all_reduce = counting
    per_micro = []
    h = B // world
    for i in range(2):
        x, eps = _dp_micro(i)
        sl = slice(h * rank, h * rank + h)
        mod.fit_step((x[sl].to(dev), torch.zeros(h, 1, dtype=torch.long, device=dev)), 0, eps=eps[sl].to(dev))
        per_micro.append(len(calls))
    torch.cuda.synchronize()
    dist.all_reduce = orig
    torch.save({"params": mod.flat.data.cpu(), "per_micro": per_micro, "nb": len(dp.buckets),
                "early": sum(dp.launched), "steps": mod.optimizer.steps.cpu()}, f"{out_file}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_window(dev):
    with tempfile.TemporaryDirectory() as d:
        init_file, out = os.path.join(d, "init"), os.path.join(d, "out")
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=_dp_worker, args=(r, 2, init_file, out)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=300)
        assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
        r0, r1 = (torch.load(f"{out}.{r}", weights_only=True) for r in range(2))
    for r in (r0, r1):
        # one exchange per window: nothing on the first micro-batch, every bucket once on the second (as many
        # all-reduces as a step of N = 1), some of them launched from inside its backward
        assert r["per_micro"] == [0, r["nb"]] and r["nb"] > 4 and r["early"] > 0
        assert bool((r["steps"] == 1).all())
    assert torch.equal(r0["params"], r1["params"])
    # a single process running N = 2 over the rank-concatenated micro-batches, the bar of tests/test_gpu_ddp.py
    mod = _module("attn", dev, 2)
    p0 = mod.flat.data.detach().cpu().double()
    seen = []
    phase = mod._optimizer_phase
    mod._optimizer_phase = lambda *a, **k: (seen.append(mod.flat.grad.detach().double().cpu()), phase(*a, **k))[1]
    for i in range(2):
        x, eps = _dp_micro(i)
        mod.fit_step((x.to(dev), torch.zeros(B, 1, dtype=torch.long, device=dev)), 0, eps=eps.to(dev))
    torch.cuda.synchronize()
    single, ref = mod.flat.data.detach().cpu().double(), seen[0]
    dp_p = r0["params"].double()
    lr = mod.optimizer.param_groups[0]["lr"]
    signal = torch.zeros_like(ref, dtype=torch.bool)
    for prm, off in zip(mod.flat.params, mod.flat.offsets):
        g = ref[off:off + prm.numel()]
        signal[off:off + prm.numel()] = g.abs() > 1e-3 * g.abs().max()
    assert float(signal.double().mean()) > 0.9
    assert float((dp_p[signal] - single[signal]).norm() / single[signal].norm()) < 1e-5
    assert float((dp_p - single).abs().max()) <= 2 * lr * 1.001
    assert not torch.equal(p0, single)
