"""The GroupNorm backward applied on load in the Winograd dy transform (ops.WINOGRAD_GNBWD_LOAD,
mvae_group_norm_bwd_dy_transforms): kernel level against the plain transform of a float64 dx, the ResnetBlock edge
conv1 -> GroupNorm+SiLU -> conv2 with the fusion on and off and against float64, the fallbacks, determinism."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CONV_TOL = 2e-4   # the Winograd tests' bar against float64 (tests/test_gpu_winograd.py)
# Fusion on against off, norm-wise. The two runs feed conv1's backward dy values that differ in their last fp32 bits (the
# fused transform evaluates dx with the hardware exp / reciprocal, gn_dx_kernel with its own sequence), and the transform
# then cuts every V / D' word into bf16 hi + bf16 lo, 16 significant bits: a last-bit change of a word can move its lo
# half by one unit, 2^-17 of the word, in either run. Two independent re-roundings at that resolution bound the relative
# distance of the GEMM operands, and so of the (linear) gradients, by 2 * 2^-17 = 2^-16. (The 5e-6 that
# tests/test_gpu_winograd.py holds two paths to does not apply: there the split operands are bitwise equal and only a
# sum order differs; a first version of this test borrowed it and measured 8.7e-6 on conv1's input gradient.)
PATH_TOL = 2.0 ** -16
U = 2.0 ** -24    # fp32 unit roundoff
# F(4x4, 3x3): largest absolute row sum of B^T (V = B^T P B) and of A = (A^T)^T (D' = A D A^T)
BT_ROW, A_ROW = 10.0, 15.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture()
def fp32x3():
    from medvae_disentangled_multimodal_amd import ops
    prev = ops.set_precision("32")
    yield
    ops.restore_math_mode(prev)


def cl(t, dev):
    return t.to(dev).contiguous(memory_format=torch.channels_last)


def rel(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _words(buf, pos, tiles, k):
    """hi + lo of a split4_bf16 operand [pos][tiles][k / 4] x (hi01, hi23, lo01, lo23), in float64: [pos][tiles][k]."""
    w = buf.view(torch.int32).view(pos, tiles, k // 4, 4)
    lo16 = lambda t: (t << 16).view(torch.float32).double()
    hi16 = lambda t: (t & -65536).view(torch.float32).double()
    e = [lo16(w[..., 0]) + lo16(w[..., 2]), hi16(w[..., 0]) + hi16(w[..., 2]),
         lo16(w[..., 1]) + lo16(w[..., 3]), hi16(w[..., 1]) + hi16(w[..., 3])]
    return torch.stack(e, dim=-1).reshape(pos, tiles, k)


def _coef(n, c, groups, g):
    """Random coefficient rows [5][n * c]: rstd-like positive scale and p per (n, c), q and r per (n, group)."""
    cpg = c // groups
    sc, sh = torch.rand(n, c, generator=g) + 0.5, torch.randn(n, c, generator=g) * 0.3
    p = torch.rand(n, c, generator=g) + 0.5
    q = (torch.randn(n, groups, generator=g) * 0.2).repeat_interleave(cpg, 1)
    r = (torch.randn(n, groups, generator=g) * 0.2).repeat_interleave(cpg, 1)
    return torch.stack([sc, sh, p, q, r]).float().contiguous()


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("c,groups,hw", [(32, 32, 8), (32, 8, 32), (64, 32, 32), (64, 8, 8)])
def test_fused_transform_matches_plain_transform_of_float64_dx(dev, fp32x3, c, groups, hw, silu):
    """V and D' of the fused entry point against mvae_winograd_dy_transforms on dx = fp32(float64 formula).

    Bound, per transformed element (hi + lo reassembled, both sides). The fused kernel evaluates, per element, a = sc x +
    sh (1 fma), s = rcp(1 + exp(-a)) (exp and rcp to ~2 and 1 ulp, one add), g = s (1 + a (1 - s)) (a subtract, an fma,
    a multiply), da = dy g, dx = fma(p, da, fma(q, x, r)): at most 10 roundings, each of relative size u = 2^-24 on a
    partial result no larger than m = |p da| (1 + |a|) + |q x| + |r|; the reference dx carries its own rounding, u |dx|
    <= u m. So |dx_fused - dx_ref| <= 11 u max(m) = e: "one ulp of dx" with the operation count of the formula, taken at
    the largest term since dx cancels. Through V = B^T P B every element moves by at most e (max abs row sum of B^T)^2 =
    100 e, through D' = A D A^T by at most 225 e. The transforms' own fp32 roundings act on inputs that differ by e:
    identical code on both sides, at most 12 adds per output on values <= 100 max|dx| (225), each u: 24 u rowsum^2
    max|dx| covers both sides. Each side then splits its fp32 word into bf16 hi + bf16 lo, exact to 2^-16 of the word
    (truncation or RNE), so the reassembled words may differ by a further 2 * 2^-16 |word|."""
    from medvae_disentangled_multimodal_amd import _lib, ops
    n, mt, pos = 2, 4, 36
    g = torch.Generator().manual_seed(c * 1000 + groups * 10 + hw + int(silu))
    x = cl(torch.randn(n, c, hw, hw, generator=g), dev)
    dy = cl(torch.randn(n, c, hw, hw, generator=g), dev)
    coef = _coef(n, c, groups, g).to(dev)
    sc, sh, p, q, r = (coef[i].double().view(n, c, 1, 1) for i in range(5))
    xd, dd = x.double(), dy.double()
    a = sc * xd + sh
    s = torch.sigmoid(a)
    da = dd * s * (1 + a * (1 - s)) if silu else dd
    dx64 = p * da + q * xd + r
    dx = dx64.float().contiguous(memory_format=torch.channels_last)
    m = ((p * da).abs() * (1 + a.abs()) + (q * xd).abs() + r.abs()).max().item()
    e = 11 * U * m
    tiles = n * (-(-hw // mt)) ** 2
    nbytes = 4 * pos * tiles * c
    v0, d0, v1, d1 = (torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(4))
    st = ops._stream(x)
    _lib.call("mvae_winograd_dy_transforms", dx.data_ptr(), v0.data_ptr(), d0.data_ptr(), n, hw, hw, c, 0, mt, st)
    rows = _lib.query("mvae_group_norm_bwd_dy_rows", n, hw, hw, c, mt)
    assert rows == -(-tiles * (c // 4) // 256)
    cs = torch.full((rows, c), float("nan"), device=dev)
    _lib.call("mvae_group_norm_bwd_dy_transforms", x.data_ptr(), dy.data_ptr(), coef.data_ptr(), n * c, 0, int(silu),
              v1.data_ptr(), d1.data_ptr(), cs.data_ptr(), n, hw, hw, c, mt, st)
    torch.cuda.synchronize()
    dmax = dx64.abs().max().item()
    for name, got, ref, row in (("V", v1, v0, BT_ROW), ("D'", d1, d0, A_ROW)):
        gw, rw = _words(got, pos, tiles, c), _words(ref, pos, tiles, c)
        tol = row * row * (e + 24 * U * dmax) + 2 * 2.0 ** -16 * rw.abs()
        ratio = ((gw - rw).abs() / tol).max().item()
        print(f"{name} c={c} G={groups} hw={hw} silu={silu}: worst |err| / tol = {ratio:.3f}")
        assert torch.isfinite(gw).all() and ratio <= 1.0, (name, ratio)
    # the conv bias gradient from the workgroups' column sums: fp32 sums of at most 64 values per row (the tile's 16
    # pixels, then 256 / (c / 4) <= 32 tiles in LDS), fp64 after: 64 u sum|dx| on top of e per element
    ws = torch.empty(_lib.query("mvae_group_norm_bwd_dy_bias_workspace_bytes", c), dtype=torch.uint8, device=dev)
    db = torch.full((c,), float("nan"), device=dev)
    _lib.call("mvae_group_norm_bwd_dy_bias", cs.data_ptr(), rows, c, db.data_ptr(), 0.0, ws.data_ptr(), ws.numel(), st)
    ref = dx64.sum((0, 2, 3)).cpu()
    tol = (64 * U * dx64.abs().sum((0, 2, 3)) + n * hw * hw * e).cpu() + 2 * U * ref.abs()
    ratio = ((db.double().cpu() - ref).abs() / tol).max().item()
    print(f"bias c={c} G={groups} hw={hw} silu={silu}: worst |err| / tol = {ratio:.3f}")
    assert ratio <= 1.0
    # an image chunk: the second image alone, its coefficient rows found through the offset -- the same bytes
    t1 = tiles // n
    v2, d2 = (torch.empty(nbytes // n, dtype=torch.uint8, device=dev) for _ in range(2))
    cs2 = torch.empty(_lib.query("mvae_group_norm_bwd_dy_rows", 1, hw, hw, c, mt), c, device=dev)
    _lib.call("mvae_group_norm_bwd_dy_transforms", x[1:].data_ptr(), dy[1:].data_ptr(), coef.data_ptr(), n * c, 1,
              int(silu), v2.data_ptr(), d2.data_ptr(), cs2.data_ptr(), 1, hw, hw, c, mt, st)
    torch.cuda.synchronize()
    for full, part in ((v1, v2), (d1, d2)):
        assert torch.equal(full.view(pos, tiles, c * 4)[:, t1:], part.view(pos, t1, c * 4))


def test_entry_point_rejects_what_it_does_not_cover(dev, fp32x3):
    """No F(2x2) form, no channel count whose 4-groups do not divide a workgroup, coefficient rows that end early."""
    from medvae_disentangled_multimodal_amd import _lib
    assert _lib.query("mvae_group_norm_bwd_dy_rows", 2, 8, 8, 32, 2) == 0
    assert _lib.query("mvae_group_norm_bwd_dy_rows", 2, 8, 8, 96, 4) == 0
    t = torch.zeros(1 << 16, device=dev)
    with pytest.raises(RuntimeError):
        _lib.call("mvae_group_norm_bwd_dy_transforms", t.data_ptr(), t.data_ptr(), t.data_ptr(), 32, 1, 1, t.data_ptr(),
                  t.data_ptr(), t.data_ptr(), 1, 8, 8, 32, 4, None)


# ---- block level: conv1 -> GroupNorm(8)+SiLU -> conv2 at B = 2, C = 32, 32 x 32 -------------------------------------
N, C, HW, G = 2, 32, 32, 8


def _inputs():
    g = torch.Generator().manual_seed(77)
    return dict(x=torch.randn(N, C, HW, HW, generator=g), wa=torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5),
                ba=torch.randn(C, generator=g) * 0.1, gam=torch.rand(C, generator=g) + 0.5,
                bet=torch.randn(C, generator=g) * 0.1, wb=torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5),
                dy=torch.randn(N, C, HW, HW, generator=g))


@pytest.fixture(scope="module")
def oracle():
    """float64 gradients of conv1's input, weight and bias (computed once)."""
    t = {k: v.double().requires_grad_(k != "dy") for k, v in _inputs().items()}
    h = F.conv2d(t["x"], t["wa"], t["ba"], padding=1)
    y = F.conv2d(F.silu(F.group_norm(h, G, t["gam"], t["bet"], eps=1e-6)), t["wb"], None, padding=1)
    y.backward(t["dy"])
    return [t[k].grad.detach() for k in ("x", "wa", "ba")]


def _block(dev, monkeypatch, fused, mode="plain", chunks=False):
    """The chain on the HIP path (streaming GroupNorm, every 3x3 conv on F(4x4)); returns conv1's (dx, dw, db), the
    entry points called, and mode's extra result."""
    from medvae_disentangled_multimodal_amd import _lib, ops
    for k, v in (("WINOGRAD", True), ("WINOGRAD_MIN_C", 1), ("WINOGRAD_MIN_C_WIDE", 1), ("WINOGRAD_TILE", 4),
                 ("WINOGRAD_MAX_W", 64), ("WINOGRAD_MIN_MACS", 0.0), ("WINOGRAD_GN", True), ("WINOGRAD_GN_LINK", True),
                 ("DYSPLIT_MIN_MACS", 0.0), ("DIRECT_WGRAD", False), ("BWD_OVERLAP", False),
                 ("WINOGRAD_GNBWD_LOAD", fused)):
        monkeypatch.setattr(ops, k, v)
    if chunks:  # (one image per 4 GiB descriptor: the existing chunk rule then cuts B = 2 into two chunks)
        monkeypatch.setattr(ops, "_MAX_DESC_BYTES", 36 * (HW // 4) ** 2 * C * 4)
    t = _inputs()
    x = cl(t["x"], dev).requires_grad_(True)
    wa, wb = (cl(t[k], dev).requires_grad_(True) for k in ("wa", "wb"))
    ba, gam, bet = (t[k].to(dev).requires_grad_(True) for k in ("ba", "gam", "bet"))
    dy = cl(t["dy"], dev)
    geom = ops.ConvGeom(3, 3, 1, 1, 1, 1, 1, False)
    seen, orig, extra = [], _lib.call, None

    def spy(name, *args):
        seen.append(name)
        return orig(name, *args)
    _lib.call("mvae_set_group_norm_path", 1)  # (the streaming GroupNorm chain at this size)
    prev = ops.set_precision("32")
    monkeypatch.setattr(_lib, "call", spy)
    try:
        h = ops.conv2d(x, wa, ba, geom, gn_stats=True)
        if mode == "retain":
            h.retain_grad()
        hg = ops.group_norm(h, gam, bet, G, 1e-6, silu=True, for_conv=C, conv_dy_only=mode != "consumer2")
        y = ops.conv2d(hg, wb, None, geom)
        if mode == "read":  # the gradient of conv1's output itself: the pass ends there, with the placeholder
            (extra,) = torch.autograd.grad(y, [h], dy)
        elif mode == "twice":
            y.backward(dy, retain_graph=True)
            for p in (x, wa, ba, gam, bet, wb):
                p.grad = None
            del seen[:]
            y.backward(dy)
        elif mode == "consumer2":
            (y * dy).sum().add((h * h).sum() * 0.5).backward()
        else:
            y.backward(dy)
        if mode == "retain":
            extra = h.grad
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(_lib, "call", orig)
        _lib.call("mvae_set_group_norm_path", 0)
        ops.restore_math_mode(prev)
    return [None if p.grad is None else p.grad.detach().clone() for p in (x, wa, ba)], seen, extra


FUSED = "mvae_group_norm_bwd_dy_transforms"


@pytest.mark.parametrize("chunks", [False, True], ids=["one", "two_chunks"])
def test_block_gradients_fused_off_and_float64(dev, monkeypatch, oracle, chunks):
    """conv1's input, weight and bias gradients: the fusion on takes the fused transform (once per image chunk) and
    never gn_dx's entry point; on, off and float64 agree -- each against float64 within the conv bar (2e-4), as
    tests/test_gpu_winograd.py's conv -> GroupNorm -> conv test, and on against off within PATH_TOL (derived above)."""
    on, seen, _ = _block(dev, monkeypatch, True, chunks=chunks)
    off, seen_off, _ = _block(dev, monkeypatch, False, chunks=chunks)
    assert seen.count(FUSED) == (2 if chunks else 1) and "mvae_group_norm_bwd_part_coef_nhwc" in seen
    assert "mvae_group_norm_bwd_part_split_nhwc" not in seen and "mvae_bias_grad" not in seen
    assert FUSED not in seen_off and "mvae_group_norm_bwd_part_split_nhwc" in seen_off
    for name, a, b, r in zip(("dx", "dw", "db"), on, off, oracle):
        print(f"{name}: on/off {rel(a, b):.2e}  on/f64 {rel(a, r):.2e}  off/f64 {rel(b, r):.2e}")
        assert rel(a, b) < PATH_TOL and rel(a, r) < CONV_TOL and rel(b, r) < CONV_TOL


@pytest.mark.parametrize("mode", ["retain", "twice", "consumer2"])
def test_fallbacks_write_dx_as_before(dev, monkeypatch, mode):
    """retain_grad on conv1's output, a second backward over a retained graph, a second consumer of conv1's output: the
    GroupNorm backward writes dx itself, bitwise the switch-off run, and no deferred value exists to be read."""
    on, seen, extra = _block(dev, monkeypatch, True, mode)
    off, _, extra_off = _block(dev, monkeypatch, False, mode)
    assert FUSED not in seen and "mvae_group_norm_bwd_part_coef_nhwc" not in seen
    for a, b in zip(on, off):
        assert torch.equal(a, b)
    if mode == "retain":
        assert torch.isfinite(extra).all() and torch.equal(extra, extra_off)


def test_forced_read_of_a_deferred_gradient_raises(dev, monkeypatch):
    from medvae_disentangled_multimodal_amd import ops
    _, seen, g = _block(dev, monkeypatch, True, "read")
    assert isinstance(g, ops.DeferredGnGrad) and tuple(g.shape) == (N, C, HW, HW)
    for read in (lambda: g.sum(), lambda: g.cpu(), lambda: g + 1, lambda: g.clone()):
        with pytest.raises(RuntimeError, match="deferred"):
            read()


def test_fused_backward_is_bitwise_reproducible(dev, monkeypatch):
    a, seen, _ = _block(dev, monkeypatch, True)
    b, _, _ = _block(dev, monkeypatch, True)
    assert FUSED in seen
    for u, v in zip(a, b):
        assert torch.equal(u, v)
