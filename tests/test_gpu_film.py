"""FiLM conditioning on the device: the csrc/film.hip kernels through ops.film and through the C entry points, the
GroupNorm-statistics boundary in the encoder, and training steps of ConditionalVAE(condition_method="film",
apply_film=True).

Bounds (derived, not measured): the forward is one multiply-add per element, fused or not -- at most two roundings of
2^-24 relative each on magnitudes up to |x scale| + |shift|, well inside 2^-22 (|x scale| + |shift|); a pixel sum of P
fp32 terms in ANY order is within P 2^-24 sum |term| of the exact sum (first-order worst case, the rounding of each
product included)."""
import pytest
import torch

import exact_inputs as E
from golden_io import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(3, 64, 5, 5), (2, 6, 3, 3), (1, 4, 1, 1), (2, 128, 32, 32)]
IDS = ["odd-pixels", "scalar-tail", "one", "multi-chunk"]
NAMES = ["b", "c", "h", "w"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _cl(t, dev):
    return t.to(dev).contiguous(memory_format=torch.channels_last)


def _ref64(x, scale, shift, dy):
    """(y, dx, dscale, dshift) in float64 on the CPU."""
    x, scale, shift, dy = (t.detach().cpu().double() for t in (x, scale, shift, dy))
    return (x * scale[..., None, None] + shift[..., None, None], dy * scale[..., None, None], (dy * x).sum((2, 3)),
            dy.sum((2, 3)))


def _run(x, scale, shift, dy, dev, x_grad=True):
    from medvae_disentangled_multimodal_amd import ops
    xd = x.to(dev) if x.is_cuda else _cl(x, dev)
    xd = xd.detach().requires_grad_(x_grad)
    sc, sh = scale.to(dev).requires_grad_(), shift.to(dev).requires_grad_()
    y = ops.film(xd, sc, sh)
    y.backward(dy.to(dev))
    torch.cuda.synchronize()
    return y.detach(), xd.grad, sc.grad, sh.grad


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_film_exact_on_integers(dev, shape):
    """Integers in {-3..3}: every product (<= 9) and every pixel sum (<= 9 P < 2^24) is an fp32 number, so y, dx, dscale
    and dshift equal the float64 result in every element -- a pixel dropped or counted twice at a workgroup boundary
    shows."""
    g = torch.Generator().manual_seed(sum(shape))
    b, c, h, w = shape
    x, dy = E.family_i(shape, g), E.family_i(shape, g)
    scale, shift = E.family_i((b, c), g), E.family_i((b, c), g)
    E.check_exact((dy.abs() * x.abs()).sum((2, 3)) + 9, E.grid_of("I"), "film pixel sums")
    got = _run(x, scale, shift, dy, dev)
    for t, r, what, names in zip(got, _ref64(x, scale, shift, dy), ("y", "dx", "dscale", "dshift"),
                                 (NAMES, NAMES, NAMES[:2], NAMES[:2])):
        E.assert_exact(t, r, names, f"film {what} {shape}")
    assert got[0].is_contiguous(memory_format=torch.channels_last) and got[0].dtype == torch.float32


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_film_random_against_float64(dev, shape):
    g = torch.Generator().manual_seed(7 + sum(shape))
    b, c, h, w = shape
    x, dy = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    scale, shift = torch.randn(b, c, generator=g) + 3.0, torch.randn(b, c, generator=g) - 2.0
    y, dx, dsc, dsh = _run(x, scale, shift, dy, dev)
    y64, dx64, dsc64, dsh64 = _ref64(x, scale, shift, dy)
    x64, dy64 = x.double(), dy.double()
    p = h * w
    E.assert_within(y, y64, 2.0 ** -22 * ((x64 * scale.double()[..., None, None]).abs() +
                                          shift.double()[..., None, None].abs()), NAMES, f"film y {shape}")
    E.assert_within(dx, dx64, 2.0 ** -24 * dx64.abs(), NAMES, f"film dx {shape}")  # one rounded product
    E.assert_within(dsc, dsc64, p * 2.0 ** -24 * (dy64 * x64).abs().sum((2, 3)), NAMES[:2], f"film dscale {shape}")
    E.assert_within(dsh, dsh64, p * 2.0 ** -24 * dy64.abs().sum((2, 3)), NAMES[:2], f"film dshift {shape}")


@pytest.mark.parametrize("lo,hi", [(8, 24), (3, 9), (2, 6)], ids=["aligned", "odd-offset", "unaligned-quad"])
def test_film_on_a_channel_slice(dev, lo, hi):
    """A channel slice of a wider NHWC tensor (a chunk of a conv output): 16-byte aligned it is read in place, otherwise
    through the 4-byte path or a copy -- the values are the same either way, and exact on integers."""
    g = torch.Generator().manual_seed(lo)
    wide = _cl(E.family_i((2, 32, 5, 3), g), dev)
    x = wide[:, lo:hi]
    c = hi - lo
    dy, scale, shift = E.family_i((2, c, 5, 3), g), E.family_i((2, c), g), E.family_i((2, c), g)
    before = wide.clone()
    got = _run(x, scale, shift, dy, dev)
    for t, r, what in zip(got, _ref64(x, scale, shift, dy), ("y", "dx", "dscale", "dshift")):
        E.assert_exact(t, r, None, f"film slice [{lo}:{hi}] {what}")
    assert torch.equal(wide, before)
    # ... and a sliced output gradient
    from medvae_disentangled_multimodal_amd import ops
    xs = x.detach().requires_grad_()
    sc = scale.to(dev).requires_grad_()
    gy = _cl(E.family_i((2, 32, 5, 3), g), dev)
    y = ops.film(xs, sc, shift.to(dev))
    y.backward(gy[:, lo:hi])
    _, dx64, dsc64, _ = _ref64(x, scale, shift, gy[:, lo:hi])
    E.assert_exact(xs.grad, dx64, None, "dx from a sliced dy")
    E.assert_exact(sc.grad, dsc64, None, "dscale from a sliced dy")


def test_film_backward_is_deterministic(dev):
    shape = (2, 128, 32, 32)
    g = torch.Generator().manual_seed(21)
    x, dy = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    scale, shift = torch.randn(2, 128, generator=g), torch.randn(2, 128, generator=g)
    a = _run(x, scale, shift, dy, dev)
    junk = torch.randn(1 << 20, device=dev)  # (other work in between)
    b = _run(x, scale, shift, dy, dev)
    del junk
    for s, t, what in zip(a, b, ("y", "dx", "dscale", "dshift")):
        assert torch.equal(s.view(torch.int32), t.view(torch.int32)), what


def test_film_skips_dx_for_an_input_without_gradient(dev):
    from medvae_disentangled_multimodal_amd import _lib
    shape = (2, 128, 32, 32)
    b, c, h, w = shape
    g = torch.Generator().manual_seed(22)
    x, dy = E.family_i(shape, g), E.family_i(shape, g)
    scale, shift = E.family_i((b, c), g), E.family_i((b, c), g)
    _, dx, dsc, dsh = _run(x, scale, shift, dy, dev, x_grad=False)
    _, _, dsc64, dsh64 = _ref64(x, scale, shift, dy)
    assert dx is None
    E.assert_exact(dsc, dsc64, NAMES[:2], "dscale, no dx")
    E.assert_exact(dsh, dsh64, NAMES[:2], "dshift, no dx")
    # through the C entry point: the flag, not a null pointer, decides -- a poisoned dx buffer stays as it is
    xd, dyd, scd = _cl(x, dev), _cl(dy, dev), scale.to(dev)
    poison = torch.full(shape, float("nan"), device=dev).contiguous(memory_format=torch.channels_last)
    dsc2, dsh2 = torch.empty(b, c, device=dev), torch.empty(b, c, device=dev)
    ws = torch.empty(_lib.query("mvae_film_workspace_bytes", b, h * w, c), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.call("mvae_film_bwd", xd.data_ptr(), c, dyd.data_ptr(), c, scd.data_ptr(), poison.data_ptr(), dsc2.data_ptr(),
              dsh2.data_ptr(), b, h * w, c, 0, ws.data_ptr(), ws.numel(), st)
    torch.cuda.synchronize()
    assert bool(torch.isnan(poison).all())
    E.assert_exact(dsc2, dsc64, NAMES[:2], "dscale, C entry point")
    E.assert_exact(dsh2, dsh64, NAMES[:2], "dshift, C entry point")
    _lib.call("mvae_film_bwd", xd.data_ptr(), c, dyd.data_ptr(), c, scd.data_ptr(), poison.data_ptr(), dsc2.data_ptr(),
              dsh2.data_ptr(), b, h * w, c, 1, ws.data_ptr(), ws.numel(), st)
    torch.cuda.synchronize()
    E.assert_exact(poison, _ref64(x, scale, shift, dy)[1], NAMES, "dx, C entry point")


def test_film_bad_arguments_launch_nothing(dev):
    from medvae_disentangled_multimodal_amd import _lib
    lib = _lib.load()
    b, c, p = 2, 8, 16
    x = torch.ones(b, p, c, device=dev)
    sc = torch.ones(b, c, device=dev)
    out = torch.full((b, p, c), 7.0, device=dev)
    dsc, dsh = torch.full((b, c), 7.0, device=dev), torch.full((b, c), 7.0, device=dev)
    need = _lib.query("mvae_film_workspace_bytes", b, p, c)
    ws = torch.full((need,), 7, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    ptr = lambda t: t.data_ptr()
    assert lib.mvae_film_bwd(ptr(x), c, ptr(x), c, ptr(sc), ptr(out), ptr(dsc), ptr(dsh), b, p, c, 1, ptr(ws), need - 1,
                             st) == -2
    assert b"workspace" in lib.mvae_last_error()
    assert lib.mvae_film_bwd(ptr(x), 0, ptr(x), 0, ptr(sc), ptr(out), ptr(dsc), ptr(dsh), b, p, 0, 1, ptr(ws), need,
                             st) == -1
    assert lib.mvae_film_fwd(ptr(x), 0, ptr(sc), ptr(sc), ptr(out), b, p, 0, st) == -1
    assert b"film_fwd" in lib.mvae_last_error()
    with pytest.raises(RuntimeError, match="film_bwd"):
        _lib.call("mvae_film_bwd", ptr(x), c, ptr(x), c, ptr(sc), ptr(out), ptr(dsc), ptr(dsh), b, p, c, 1, ptr(ws), 0,
                  st)
    torch.cuda.synchronize()
    for t in (out, dsc, dsh):
        assert bool((t == 7.0).all())
    assert bool((ws == 7).all())


def test_film_output_carries_nothing_of_its_input(dev):
    """The conv epilogue's GroupNorm statistics (and the DyPack request, a backward link) ride on the conv output as
    attributes; the modulated map has none, and a GroupNorm of it equals the GroupNorm of a bare copy bitwise."""
    from medvae_disentangled_multimodal_amd import ops
    from medvae_disentangled_multimodal_amd.encoder_decoder import Conv2d, Normalize
    torch.manual_seed(3)
    conv, norm = Conv2d(32, 64, 3, 1, 1).to(dev), Normalize(64).to(dev)  # (two channels per group)
    x = _cl(torch.randn(4, 32, 16, 16), dev).requires_grad_()
    h = conv(x, gn_stats=True)
    assert hasattr(h, ops.GN_PART_ATTR), "the test needs a conv that emits GroupNorm statistics"
    scale = torch.tensor([1.0, 5.0], device=dev).repeat(4, 32)  # about 3 and -2, uneven inside every group
    shift = torch.tensor([-4.0, 0.0], device=dev).repeat(4, 32)
    y = ops.film(h, scale, shift)
    assert type(y) is torch.Tensor
    for attr in (ops.GN_PART_ATTR, ops.DYPACK_ATTR, ops.GN_BWD_ATTR, ops.GN_LAZY_ATTR, ops.XSPLIT_ATTR, ops.BF16_ATTR):
        assert not hasattr(y, attr), attr
    with torch.no_grad():
        a = norm(y, silu=True)
        b = norm(y.detach().clone(memory_format=torch.channels_last), silu=True)
        stale = norm(h, silu=True)  # what reusing h's statistics for y's consumer would normalize
    assert torch.equal(a, b) and not torch.allclose(a, stale, atol=1e-2)
    ref = torch.nn.functional.silu(torch.nn.functional.group_norm(y.detach().double().cpu(), 32,
                                                                  norm.weight.detach().double().cpu(),
                                                                  norm.bias.detach().double().cpu(), 1e-6))
    assert rel_err(a.cpu(), ref) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# the encoder: both hand-offs (level 0 -> downsample, last level -> mid.block_1) against a float64 restatement
# ---------------------------------------------------------------------------------------------------------------------
KW = dict(input_channels=1, latent_dim=4, hidden_channels=32, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[],
          dropout=0.0, resolution=16, condition_dim=3, condition_method="film")
B = 4


def _model(dev, apply_film=True, seed=11):
    import medvae_disentangled_multimodal_amd as M
    torch.manual_seed(seed)
    model = M.ConditionalVAE(**KW, apply_film=apply_film)
    with torch.no_grad():  # far from the identity: scale about 3, shift about -2 per channel
        for layer in model.film_layers:
            layer.scale_transform.bias.add_(3.0)
            layer.shift_transform.bias.add_(-2.0)
    return model.to(dev)


def _inputs(seed=12):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, 16, 16, generator=g)
    cond = torch.nn.functional.one_hot(torch.tensor([0, 2, 1, 2]), 3).float()
    gy = torch.randn(B, 8, 8, 8, generator=g)
    return x, cond, gy


def _encoder64(P, x, cond):
    """oracle/torch_ref.py's encoder for ch_mult=(1, 2), one block per level, no level attention, with the FiLM line
    (conditional_vae.py FiLMLayer.forward) after each level's block."""
    from oracle import torch_ref as R
    lin = lambda name: cond @ P[f"{name}.weight"].t() + P[f"{name}.bias"]
    h = R.conv(P, "encoder.conv_in", x)
    for i in range(2):
        h = R.resblock(P, f"encoder.down.{i}.block.0", h)
        scale, shift = lin(f"film_layers.{i}.scale_transform"), lin(f"film_layers.{i}.shift_transform")
        h = h * scale[..., None, None] + shift[..., None, None]
        if i == 0:
            h = R.downsample(P, "encoder.down.0.downsample", h)
    h = R.resblock(P, "encoder.mid.block_1", h)
    h = R.attnblock(P, "encoder.mid.attn_1", h)
    h = R.resblock(P, "encoder.mid.block_2", h)
    return R.conv(P, "encoder.conv_out", R.silu(R.gn(P, "encoder.norm_out", h)))


@pytest.fixture(scope="module")
def encoder_reference():
    """(state, expected encoder output, float64 gradients) -- computed once on the CPU, shared, never changed."""
    import medvae_disentangled_multimodal_amd as M
    torch.manual_seed(11)
    model = M.ConditionalVAE(**KW, apply_film=True)
    with torch.no_grad():
        for layer in model.film_layers:
            layer.scale_transform.bias.add_(3.0)
            layer.shift_transform.bias.add_(-2.0)
    x, cond, gy = _inputs()
    P = {k: v.detach().double().requires_grad_() for k, v in model.state_dict().items()
         if k.startswith(("encoder.", "film_layers."))}
    x64 = x.double().requires_grad_()
    h = _encoder64(P, x64, cond.double())
    (h * gy.double()).sum().backward()
    grads = {k: v.grad.detach() for k, v in P.items()}
    return h.detach(), x64.grad.detach(), grads


def test_encoder_statistics_stop_at_film(dev, encoder_reference):
    """"32-exact" forward of the modulated encoder against float64 under the whole-model tolerance of
    tests/test_gpu_parity.py for that precision (1e-4, norm-wise). A Normalize that took the statistics the level's last
    conv emitted -- they describe the map before the modulation by 3 x - 2 -- is off by orders of magnitude."""
    from medvae_disentangled_multimodal_amd import ops
    h64, _, _ = encoder_reference
    model = _model(dev)
    x, cond, _ = _inputs()
    seen = []
    orig = ops.film
    prev = ops.set_precision("32-exact")
    try:
        ops.film = lambda *a: (seen.append(tuple(a[0].shape)), orig(*a))[1]
        with torch.no_grad():
            mean, logvar = model.encode(x.to(dev), cond.to(dev))
        torch.cuda.synchronize()
    finally:
        ops.film = orig
        ops.restore_math_mode(prev)
    assert seen == [(B, 32, 16, 16), (B, 64, 8, 8)]  # before the downsample, before mid.block_1
    got = torch.cat([mean, logvar], 1).cpu()
    err = rel_err(got, h64)
    print(f"film encoder forward, 32-exact: rel err {err:.3e}")
    assert err < 1e-4, err
    # the condition matters: another modality, another posterior
    with torch.no_grad():
        other, _ = model.encode(x.to(dev), cond.flip(0).to(dev))
    assert rel_err(other.cpu(), mean.cpu()) > 1e-2


def test_encoder_backward_through_film(dev, encoder_reference):
    """The same model's backward against float64 autograd of the restatement: the input gradient and every conv, norm
    and FiLM Linear gradient. Tolerance as tests/test_gpu_parity.py's "32-exact" step: the global norm within 1e-4, a
    full gradient within 10 x 1e-4 norm-wise. Some gradients are zero in exact arithmetic (a conv bias in front of a
    one-channel-per-group GroupNorm), so each tensor's error is allowed, on top of 1e-3 of its own norm, 1e-6 of the
    global norm -- a hundredth of what the global criterion allows for the whole gradient."""
    from medvae_disentangled_multimodal_amd import ops
    _, dx64, g64 = encoder_reference
    model = _model(dev)
    x, cond, gy = _inputs()
    xd = x.to(dev).requires_grad_()
    prev = ops.set_precision("32-exact")
    try:
        mean, logvar = model.encode(xd, cond.to(dev))
        (torch.cat([mean, logvar], 1) * gy.to(dev)).sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.restore_math_mode(prev)
    params = dict(model.named_parameters())
    total = float(torch.sqrt(sum((g ** 2).sum() for g in g64.values())))
    got_total = float(torch.sqrt(sum((params[k].grad.double() ** 2).sum() for k in g64)))
    print(f"film encoder backward, 32-exact: global norm {got_total:.6e} vs {total:.6e}")
    assert abs(got_total - total) <= 1e-4 * total
    err = rel_err(xd.grad.cpu(), dx64)
    print(f"  dx rel err {err:.3e}")
    assert err < 1e-3
    assert any(k.startswith("film_layers.1.shift_transform") for k in g64) and len(g64) > 40
    for k, ref in g64.items():
        g = params[k].grad
        assert g is not None, k
        d = float((g.detach().double().cpu() - ref).norm())
        print(f"  {k}: |err| {d:.3e} |ref| {float(ref.norm()):.3e}")
        assert d <= 1e-3 * float(ref.norm()) + 1e-6 * total, k
    assert float(g64["film_layers.0.scale_transform.weight"].norm()) > 1e-3 * total  # (not a vacuous comparison)


def test_apply_film_off_is_bitwise_the_unconditioned_encode(dev):
    import medvae_disentangled_multimodal_amd as M
    model = _model(dev, apply_film=False)
    x, cond, _ = _inputs()
    with torch.no_grad():
        mean, logvar = model.encode(x.to(dev), cond.to(dev))
        m0, l0 = M.BaseVAE.encode(model, x.to(dev))
    assert torch.equal(mean, m0) and torch.equal(logvar, l0)


# ---------------------------------------------------------------------------------------------------------------------
# training steps
# ---------------------------------------------------------------------------------------------------------------------
LOSS = dict(type="vae", recon_loss_type="mse", kl_weight=1.0, recon_weight=1.0)


def _module(dev, apply_film=True):
    import medvae_disentangled_multimodal_amd as M
    mod = M.VAELightningModule(_model(dev, apply_film), dict(type="adam", lr=5e-4, weight_decay=0.0, betas=[0.9, 0.999]),
                               {"type": "none"}, LOSS, gradient_clip_val=0.5)
    mod.configure_optimizers()
    return mod


def _steps(dev, n):
    g = torch.Generator().manual_seed(31)
    out = []
    for i in range(n):
        x = (torch.randint(0, 256, (B, 1, 16, 16), generator=g).float() / 255 * 2 - 1).to(dev)
        cond = torch.nn.functional.one_hot(torch.tensor([(i + j) % 3 for j in range(B)]), 3).float().to(dev)
        eps = torch.randn(B, 4, 8, 8, generator=g).to(dev)
        out.append(((x, torch.zeros(B, 1, dtype=torch.long, device=dev), cond), eps))
    return out


def _film_slices(mod):
    return [(n, slice(off, off + p.numel())) for n, p, off in zip(mod.flat.names, mod.flat.params, mod.flat.offsets)
            if n.startswith("film_layers.")]


@pytest.mark.parametrize("apply_film", [True, False], ids=["applied", "unused"])
def test_fit_steps_move_the_film_parameters_only_when_applied(dev, apply_film):
    mod = _module(dev, apply_film)
    p0 = mod.flat.data.clone()
    for i, (batch, eps) in enumerate(_steps(dev, 3)):
        loss = mod.fit_step(batch, i, eps=eps)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and not torch.equal(mod.flat.data, p0)
    slices = _film_slices(mod)
    assert len(slices) == 8
    for name, sl in slices:
        moved = not torch.equal(mod.flat.data[sl], p0[sl])
        assert moved == apply_film, name  # (the optimizer reads the flat gradient only: the Linears' arrived there)


def test_graphed_film_steps_match_eager_steps_bitwise(dev):
    steps = _steps(dev, 4)

    def run(graphed):
        mod = _module(dev)
        mod.fit_step(steps[0][0], 0, eps=steps[0][1])  # (state a capture needs is built eagerly)
        for i, (batch, eps) in enumerate(steps[1:], 1):
            (mod.fit_step_graphed if graphed else mod.fit_step)(batch, i, eps=eps)
        torch.cuda.synchronize()
        return mod
    a, b = run(False), run(True)
    assert b._graph is not None and a.global_step_count == b.global_step_count == 4
    assert torch.equal(a.flat.data.view(torch.int32), b.flat.data.view(torch.int32))
    assert torch.equal(a.optimizer.exp_avg.view(torch.int32), b.optimizer.exp_avg.view(torch.int32))
    b.teardown()


def test_evaluate_model_runs_on_a_film_module(dev):
    import math
    from medvae_disentangled_multimodal_amd.evaluation import evaluate_model
    mod = _module(dev)
    metrics, collected = evaluate_model(mod, [s[0] for s in _steps(dev, 2)])
    assert collected["latents"].shape[0] == 2 * B

    def leaves(d):
        for v in d.values():
            yield from leaves(v) if isinstance(v, dict) else [v]
    vals = list(leaves(metrics))
    assert vals and all(math.isfinite(float(v)) for v in vals), metrics
