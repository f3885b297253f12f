"""Exact tests of the conv / GEMM family: on the input families of tests/exact_inputs.py the 3xBF16, packed bf16 and
exact-fp32 MFMA paths and their fp32 accumulators are exact, so every output element must equal the float64 emulation
bitwise, whatever the summation order. A dropped tap, a wrong index, a tile-tail error, a missed split-K partial or a
dropped cross term shows as a mismatch at a named coordinate.

Each conv case checks the forward with integer bias and residual, the input gradient, the weight and bias gradients
into .grad and accumulated into a pre-filled `_mvae_main_grad` (integer fill). Shapes are the smallest that reach the
path named in each case's comment; the reference of a case is computed once and shared by the modes that run it.

Family L and tap-summed weights: the sub-pixel Upsample forms split the weights after summing taps in fp32
(mvae_conv_weight_upsample_fwd / _dgrad); a sum of family-L weights such as 2 - 2 + 2^-8 is a bf16 number itself, so its
split is not the sum of the taps' splits. Upsample cases therefore draw the activations from L and the weights from I
(tap sums are integers <= 12: hi exact, lo = 0) -- the lo(x) * hi(w) cross term is still needed for every element.

Winograd F(2x2, 3x3) (transforms use +-1 and 1/2 only) is exact on family I. On family L it is not, for an arithmetic
reason: the transforms add four inputs first and split the sum afterwards (csrc/winograd.hip input / weight transforms
write V and U in the split4 layout), so hi(V) can carry multiples of 2^-9 and hi(U) multiples of 2^-11 whose products
lie on a 2^-20 grid next to sums of 2^14: not fp32 numbers. Family L (and F(4x4), whose filter transform has 1/6 and
1/24) is checked element-wise with the bound of `exact_inputs.tau` instead."""
import pytest
import torch

import exact_inputs as E

pytestmark = pytest.mark.gpu
CL = torch.channels_last
P1, P0, DS = (1, 1, 1, 1), (0, 0, 0, 0), (0, 0, 1, 1)
W_FILL, B_FILL = 5.0, -3.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def cl(t, dev):
    return t.to(dev).contiguous(memory_format=CL)


# name: (n, cin, cout, h, w, k, stride, pads (t, l, b, r), upsample, families)
CASES = {
    # K tails (cin * 9 % 32 != 0, reference K order); cin 3 / 6 take the scalar gather
    "cin3": (2, 3, 32, 9, 9, 3, 1, P1, False, "IL"),
    "cin6": (2, 6, 16, 8, 8, 3, 1, P1, False, "IL"),
    "cin48_cout40": (2, 48, 40, 9, 9, 3, 1, P1, False, "IL"),   # ... and an N tail (cout 40)
    "cin96_cout48": (2, 96, 48, 9, 9, 3, 1, P1, False, "IL"),   # permuted K order (3 chunks per tap), N tail 48
    "cout1": (2, 32, 1, 12, 12, 3, 1, P1, False, "IL"),         # N tail 1; small-cout weight gradient
    "cout3": (2, 64, 3, 10, 10, 3, 1, P1, False, "IL"),         # N tail 3; small-cout weight gradient
    "m_tail": (3, 64, 64, 7, 5, 3, 1, P1, False, "IL"),         # M = 105 pixels: no multiple of any tile height
    "down_odd": (3, 32, 32, 15, 15, 3, 2, DS, False, "IL"),     # stride 2, pad (0,1,0,1), odd size (gather dgrad)
    "down_even": (2, 64, 64, 14, 14, 3, 2, DS, False, "IL"),    # ... even size: input gradient by parity class
    "s2_sym": (2, 32, 64, 10, 12, 3, 2, P1, False, "IL"),       # symmetric-pad stride 2, non-square
    "k4s2": (2, 16, 32, 16, 16, 4, 2, P1, False, "IL"),         # 4x4 stride 2 (PatchGAN)
    "pw": (4, 128, 64, 8, 8, 1, 1, P0, False, "IL"),            # 1x1: batched-GEMM entry
    "pw_s2": (2, 32, 16, 8, 8, 1, 2, P0, False, "IL"),          # 1x1 stride 2 (empty parity classes)
    "ups": (2, 32, 32, 7, 7, 3, 1, P1, True, "IL"),             # Upsample: sub-pixel fwd, 4x4 stride-2 dgrad
    "ups_cin3": (2, 3, 8, 5, 6, 3, 1, P1, True, "IL"),          # ... scalar gather, non-square
    "ups_48_40": (2, 48, 40, 6, 9, 3, 1, P1, True, "IL"),       # ... K and N tails, non-square
    "skinny_fwd": (64, 64, 3, 32, 32, 3, 1, P1, False, "IL"),   # 128x16 tiles (>= 512 of them): conv_out forward
    "skinny_dgrad": (64, 6, 64, 32, 32, 3, 1, P1, False, "IL"),  # 128x16 tiles: conv_in input gradient
    "direct32_28": (4, 32, 32, 28, 28, 3, 1, P1, False, "IL"),  # mvae_conv2d_direct32_nhwc fwd + dgrad, direct wgrad
    "direct32_7x11": (3, 32, 32, 7, 11, 3, 1, P1, False, "IL"),
    "direct32_31x5": (2, 32, 32, 31, 5, 3, 1, P1, False, "IL"),
    "direct32_60": (1, 32, 32, 60, 60, 3, 1, P1, False, "IL"),  # one large image (family L: 3600 pixels just fit 2^24)
    "wdirect_64_32": (3, 64, 32, 28, 28, 3, 1, P1, False, "IL"),   # direct weight gradient, cin 64 -> cout 32
    "wdirect_9x11": (2, 64, 32, 9, 11, 3, 1, P1, False, "IL"),     # ... odd, non-square
    "wdirect_bands": (520, 32, 32, 7, 5, 3, 1, P1, False, "IL"),   # ... 520 one-band images > the 512-workgroup cap
    "splitk_7x7": (4, 128, 128, 7, 7, 3, 1, P1, False, "IL"),      # smallest fwd + dgrad the planner splits over K
    "splitk_4x4": (1, 256, 256, 4, 4, 3, 1, P1, False, "IL"),
    "tile_256x256": (130, 32, 256, 15, 17, 3, 1, P1, False, "IL"),  # M = 33150, N = 256: the 256x256 forward tile
    "tile_256x128": (66, 32, 256, 15, 17, 3, 1, P1, False, "IL"),   # M = 16830, N = 256: the 256x128 forward tile
    # (the p2 path is chosen inside the library by the image size; the project has no way to observe it)
    "p2_16": (4, 64, 128, 16, 16, 3, 1, P1, False, "IL"),          # power-of-two gather weight gradient
    "p2_8x32": (2, 256, 64, 8, 32, 3, 1, P1, False, "IL"),
    "p2_64x8": (3, 64, 64, 64, 8, 3, 1, P1, False, "IL"),
    "p2_cout256": (16, 128, 256, 8, 8, 3, 1, P1, False, "IL"),     # ... cout 256: more than two N tiles
}
# Family L on these shapes covers y and dx only: their weight gradient sums 18 200 .. 66 560 pixels, and
# pixels * 3.002^2 * 2^9 >= 2^24 breaks the precondition, while shrinking the pixel count would leave the tile config /
# persistent loop the case is there for. The weight and bias gradients of these shapes are checked on family I.
L_YDX_ONLY = {"skinny_fwd", "skinny_dgrad", "wdirect_bands", "tile_256x256", "tile_256x128"}
# kernels a case must launch on the default path (forward + backward through ops.conv2d)
MUST_CALL = {
    "cout1": {"mvae_conv2d_wgrad_small_cout_nhwc"}, "cout3": {"mvae_conv2d_wgrad_small_cout_nhwc"},
    "down_even": {"mvae_conv2d_dgrad_stride2_nhwc"}, "s2_sym": {"mvae_conv2d_dgrad_stride2_nhwc"},
    "k4s2": {"mvae_conv2d_dgrad_stride2_nhwc"}, "pw_s2": {"mvae_conv2d_dgrad_stride2_nhwc"},
    "pw": {"mvae_gemm_strided_batched"},
    "ups": {"mvae_conv2d_upsample_nhwc", "mvae_conv_weight_upsample_dgrad", "mvae_conv2d_wgrad_upsample_nhwc"},
    "ups_cin3": {"mvae_conv2d_upsample_nhwc"}, "ups_48_40": {"mvae_conv2d_upsample_nhwc"},
    "direct32_28": {"mvae_conv2d_direct32_nhwc", "mvae_conv2d_wgrad_direct_nhwc"},
    "direct32_7x11": {"mvae_conv2d_direct32_nhwc"}, "direct32_31x5": {"mvae_conv2d_direct32_nhwc"},
    "direct32_60": {"mvae_conv2d_direct32_nhwc"},
    "wdirect_64_32": {"mvae_conv2d_wgrad_direct_nhwc"}, "wdirect_9x11": {"mvae_conv2d_wgrad_direct_nhwc"},
    "wdirect_bands": {"mvae_conv2d_wgrad_direct_nhwc"},
    "splitk_7x7": {"mvae_conv2d_ws_nhwc"}, "splitk_4x4": {"mvae_conv2d_ws_nhwc"},
}
_REF = {}


def _problem(name, fam):
    """Inputs and expected outputs of one case and family (computed once): x, w, b, res, dy and y, dx, dw, db."""
    key = (name, fam)
    if key in _REF:
        return _REF[key]
    n, ci, co, h, w_, k, s, pads, ups, _ = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) * 2 + (fam == "L"))
    fw = "I" if (ups and fam == "L") else fam  # (tap-summed weights: see the module docstring)
    x, wt = E.family(fam, (n, ci, h, w_), g), E.family(fw, (co, ci, k, k), g)
    fwd, dgrad, wgrad = E.conv_ops(x.shape, wt.shape, s, pads, ups)
    ho, wo = fwd(torch.zeros(1, ci, h, w_), torch.zeros(1, ci, k, k)).shape[2:]
    b, res = E.family_i((co,), g), E.family_i((n, co, ho, wo), g)
    dy = E.family(fam, (n, co, ho, wo), g)
    grid = E.grid_of(fam)
    # the exactness precondition, per output (a condition on the inputs; fp32 is enough for a bound)
    E.check_exact(fwd(x.abs(), wt.abs()) + b.abs().view(1, -1, 1, 1) + res.abs(), grid, f"{name} fwd")
    E.check_exact(dgrad(dy.abs(), wt.abs()), grid, f"{name} dgrad")
    with_w = not (fam == "L" and name in L_YDX_ONLY)
    if with_w:
        E.check_exact(wgrad(dy.abs(), x.abs()) + W_FILL, grid, f"{name} wgrad")
        E.check_exact(dy.abs().sum((0, 2, 3)) + abs(B_FILL), grid, f"{name} bias grad")
    # float64, or fp32 for the large shapes: under the precondition every fp32 partial sum is exact as well
    # (tests/test_exact_inputs.py shows the two agree bitwise)
    big = float(n) * ho * wo * co * ci * k * k > 3e8
    cast = (lambda t: t.float()) if big else (lambda t: t)
    em = lambda op, a, b_: E.emulate(lambda p, q: op(cast(p), cast(q)).double(), a, b_)  # noqa: E731
    exp = dict(y=em(fwd, x, wt) + b.double().view(1, -1, 1, 1) + res.double(), dx=em(dgrad, dy, wt),
               dw=em(wgrad, dy, x) if with_w else None, db=dy.double().sum((0, 2, 3)) if with_w else None)
    _REF[key] = (dict(x=x, w=wt, b=b, res=res, dy=dy), exp, (fwd, dgrad, wgrad))
    return _REF[key]


def _spy(monkeypatch):
    from medvae_disentangled_multimodal_amd import _lib
    seen, orig = [], _lib.call

    def spy(name, *args):
        seen.append(name)
        return orig(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    return seen


def _geom(name):
    from medvae_disentangled_multimodal_amd import ops
    n, ci, co, h, w_, k, s, pads, ups, _ = CASES[name]
    return ops.ConvGeom(k, k, s, pads[0], pads[1], pads[2], pads[3], ups)


def _fwd_bwd(dev, name, t, main_grad, with_w=True):
    """with_w=False: forward and input gradient only (the weights and the bias take no gradient)."""
    from medvae_disentangled_multimodal_amd import ops
    xd, wd, bd = cl(t["x"], dev).requires_grad_(), cl(t["w"], dev), t["b"].to(dev)
    if not with_w:
        y = ops.conv2d(xd, wd, bd, _geom(name), residual=cl(t["res"], dev))
        y.backward(cl(t["dy"], dev))
        torch.cuda.synchronize()
        return y.detach(), xd.grad, None, None
    wd.requires_grad_()
    bd.requires_grad_()
    if main_grad:
        wd._mvae_main_grad = torch.full_like(wd, W_FILL, memory_format=CL)
        bd._mvae_main_grad = torch.full_like(bd, B_FILL)
    y = ops.conv2d(xd, wd, bd, _geom(name), residual=cl(t["res"], dev))
    y.backward(cl(t["dy"], dev))
    torch.cuda.synchronize()
    if main_grad:
        assert wd.grad is None and bd.grad is None
        return y.detach(), xd.grad, wd._mvae_main_grad - W_FILL, bd._mvae_main_grad - B_FILL
    return y.detach(), xd.grad, wd.grad, bd.grad


def _check(got, exp, what, dw_bounded=None):
    """dw_bounded = (float64 reference, element-wise bound): the weight gradient of a path that is not exact."""
    y, dx, dw, db = got
    E.assert_exact(y, exp["y"], "nchw", f"{what} y")
    E.assert_exact(dx, exp["dx"], "nchw", f"{what} dx")
    if exp["dw"] is None:  # (L_YDX_ONLY)
        assert dw is None and db is None
        return
    if dw_bounded is None:
        E.assert_exact(dw, exp["dw"], "kcrs", f"{what} dw", {"k": 64, "c": 32})
    else:
        E.assert_within(dw, dw_bounded[0], dw_bounded[1], "kcrs", f"{what} dw (bounded)")
    E.assert_exact(db, exp["db"], "k", f"{what} db")


def _small_cout_bound(name, fam):
    """The small-cout weight gradient (cout <= 4, mvae_conv2d_wgrad_small_cout_nhwc) multiplies in plain fp32,
    `acc[r * 3 + s][o][e] += dv[o] * xv.x` (csrc/conv_small.hip:96-99), not in 3xBF16: on family L the lo*lo products
    (2^-18) are computed and each fp32 fused multiply-add rounds, so it is not on the 2^-9 grid. Family I stays exact;
    family L is held to the element-wise bound tau(K) * op(|dy|, |x|) against the float64 product (K = pixels)."""
    if fam != "L" or CASES[name][2] > 4:
        return None
    t, _, (_, _, wgrad) = _problem(name, fam)
    n, ci, co, h, w_ = CASES[name][:5]
    d = lambda v: v.double()  # noqa: E731
    return wgrad(d(t["dy"]), d(t["x"])), E.tau(n * h * w_) * wgrad(d(t["dy"]).abs(), d(t["x"]).abs())


def _cases(fams="IL", only=None):
    return [pytest.param(nm, f, id=f"{nm}-{f}") for nm, c in CASES.items() for f in c[9]
            if f in fams and (only is None or only(nm, c))]


@pytest.mark.parametrize("name,fam", _cases())
def test_conv_default_path_exact(dev, name, fam, monkeypatch):
    """The default 3xBF16 path (register-staged loop, weights pre-split by the weight prep, direct / small-cout /
    parity-class / split-K kernels where the planners choose them): every element of y, dx, dw, db."""
    from medvae_disentangled_multimodal_amd import _lib
    t, exp, _ = _problem(name, fam)
    n, ci, co, h, w_, k, s, pads, ups, _ = CASES[name]
    if name.startswith("splitk"):  # both the forward and the input gradient split (as test_conv_splitk_matches_unsplit)
        assert _lib.query("mvae_conv2d_split_workspace_bytes", n, ci, co, 3, 3, h, w_) > 0
        assert _lib.query("mvae_conv2d_split_workspace_bytes", n, co, ci, 3, 3, h, w_) > 0
    if name.startswith("tile_"):
        assert _choose_tile(n * h * w_, co) == {"tile_256x256": 0, "tile_256x128": 1}[name]
    seen = _spy(monkeypatch)
    with_w = exp["dw"] is not None
    _check(_fwd_bwd(dev, name, t, False, with_w), exp, f"{name}/{fam} .grad", _small_cout_bound(name, fam))
    missing = MUST_CALL.get(name, set()) - set(seen) - (set() if with_w else {"mvae_conv2d_wgrad_direct_nhwc"})
    assert not missing, (name, "path not taken", missing)
    if name.startswith("splitk"):
        assert seen.count("mvae_conv2d_ws_nhwc") == 2
    if name.startswith("direct32"):
        assert seen.count("mvae_conv2d_direct32_nhwc") == 2
    if with_w:
        _check(_fwd_bwd(dev, name, t, True), exp, f"{name}/{fam} main_grad", _small_cout_bound(name, fam))


def _choose_tile(m, n):
    """The forward / input-gradient tile cost model of csrc/gemm_core.h choose_tile (0 = 256x256, 1 = 256x128),
    restated: the library exports no query for the tile it launches, so this asserts the model, not the launch. It
    has to follow gemm_core.h:1979-1990 by hand if that model changes, and it does not hold under the experiment
    knob MVAE_GEMM_TILE. Should a query be exported, use that instead."""
    tm, tn = (256, 256, 128, 128, 64), (256, 128, 256, 128, 64)
    eff, res, area = (1.0, 0.82, 0.82, 0.70, 0.50), (1, 1, 1, 2, 4), (65536, 32768, 32768, 16384, 4096)
    best, bt = 4, 1e300
    for c in range(5):
        tiles = -(-m // tm[c]) * -(-n // tn[c])
        cost = -(-tiles // (256 * res[c])) * res[c] * area[c] / eff[c]
        if cost < bt * 0.999:
            bt, best = cost, c
    return best


_SMALL = lambda nm, c: c[0] * c[3] * c[4] <= 4096  # noqa: E731  (the modes below re-run the small shapes only)


@pytest.mark.parametrize("name,fam", _cases(only=lambda nm, c: _SMALL(nm, c) and c[2] % 4 == 0 and c[5] != 1 and not c[8]))
def test_conv_presplit_dy_exact(dev, name, fam, monkeypatch):
    """dy split once (mvae_split_bf16) and handed pre-split to both backward GEMMs (`dys=`: MVAE_CONV_XSPLIT dgrad
    operand, MVAE_CONV_DYSPLIT wgrad operand), as test_conv_backward_with_presplit_dy forces it."""
    from medvae_disentangled_multimodal_amd import ops
    monkeypatch.setattr(ops, "DY_SPLIT_MIN", 0)
    monkeypatch.setattr(ops, "DY_SPLIT", True)
    t, exp, _ = _problem(name, fam)
    seen = _spy(monkeypatch)
    _check(_fwd_bwd(dev, name, t, False), exp, f"{name}/{fam} dys .grad")
    assert "mvae_split_bf16" in seen
    _check(_fwd_bwd(dev, name, t, True), exp, f"{name}/{fam} dys main_grad")


@pytest.mark.parametrize("name,fam", _cases(only=lambda nm, c: _SMALL(nm, c) and c[1] % 4 == 0 and c[5] != 1 and not c[8]))
def test_conv_presplit_x_exact(dev, name, fam):
    """The conv input pre-split in HBM (`x_split=`: what a GroupNorm writes for its conv): forward and weight
    gradient read the split4_bf16 groups."""
    from medvae_disentangled_multimodal_amd import _lib, ops
    t, exp, _ = _problem(name, fam)
    n, ci, co, h, w_, k, s, pads, ups, _ = CASES[name]
    geom = _geom(name)
    xd = cl(t["x"], dev)
    xs = torch.empty_like(xd)
    _lib.call("mvae_split_bf16", xd.data_ptr(), xs.data_ptr(), xd.numel(), ops._stream(xd))
    y = ops.conv2d_forward_raw(xs, cl(t["w"], dev), t["b"].to(dev), cl(t["res"], dev), geom, x_split=True)
    E.assert_exact(y, exp["y"], "nchw", f"{name}/{fam} x_split y")
    dw = torch.full((co, ci, k, k), W_FILL, device=dev).contiguous(memory_format=CL)
    db = torch.full((co,), B_FILL, device=dev)
    dyd = cl(t["dy"], dev)
    fused = ops.conv2d_wgrad_raw(dyd, xs, dw, 1.0, geom, db=db, x_split=True)
    torch.cuda.synchronize()
    sb = _small_cout_bound(name, fam)
    if sb is None:
        E.assert_exact(dw - W_FILL, exp["dw"], "kcrs", f"{name}/{fam} x_split dw")
    else:
        E.assert_within(dw - W_FILL, sb[0], sb[1], "kcrs", f"{name}/{fam} x_split dw (bounded)")
    if fused:
        E.assert_exact(db - B_FILL, exp["db"], "k", f"{name}/{fam} x_split db")
    else:  # (no fused bias sum on this route -- the caller sums dy itself, ops.bias_grad_raw: db must be untouched)
        E.assert_exact(db, torch.full((co,), B_FILL), "k", f"{name}/{fam} x_split db left alone")
        ops.bias_grad_raw(dyd.data_ptr(), n * y.shape[2] * y.shape[3], co, db, 1.0, dev, ops._stream(xd))
        torch.cuda.synchronize()
        E.assert_exact(db - B_FILL, exp["db"], "k", f"{name}/{fam} x_split db (bias_grad_raw)")


def _dma_ok(nm, c):
    return _SMALL(nm, c) and c[1] % 8 == 0 and c[2] % 8 == 0 and c[5] != 1


@pytest.mark.parametrize("name,fam", _cases(only=_dma_ok))
def test_conv_planar_dma_exact(dev, name, fam, monkeypatch):
    """3xBF16 on planar hi / lo bf16 operands staged by LDS-DMA (MVAE_CONV_PLANAR), forced as in
    tests/test_gpu_bf16_dma.py."""
    from medvae_disentangled_multimodal_amd import ops
    monkeypatch.setattr(ops, "BF16_DMA", True)
    monkeypatch.setattr(ops, "PLANAR_DMA", True)
    monkeypatch.setattr(ops, "PLANAR_MIN_MACS", 0)
    t, exp, _ = _problem(name, fam)
    seen = _spy(monkeypatch)
    prev = ops.set_precision("32")
    try:
        assert ops._dma_fmt() == 3
        got = _fwd_bwd(dev, name, t, False)
        got_m = _fwd_bwd(dev, name, t, True)
    finally:
        ops.restore_math_mode(prev)
    assert "mvae_split_planar" in seen or "mvae_split_planar_colsum" in seen
    _check(got, exp, f"{name}/{fam} planar .grad")
    _check(got_m, exp, f"{name}/{fam} planar main_grad")


@pytest.mark.parametrize("name,fam", _cases("I", only=lambda nm, c: _SMALL(nm, c)))
def test_conv_packed_bf16_exact(dev, name, fam, monkeypatch):
    """bf16-mixed (PREC 4: packed bf16 operands through the LDS-DMA loop, the c5 path; channel counts that are no
    multiple of 8 and 1x1 convs stay on the register-staged bf16 loop): integers are bf16 numbers, so it is exact."""
    from medvae_disentangled_multimodal_amd import ops
    monkeypatch.setattr(ops, "BF16_DMA", True)
    t, exp, _ = _problem(name, fam)
    seen = _spy(monkeypatch)
    prev = ops.set_precision("bf16-mixed")
    try:
        assert ops._MATH[0] == 1
        got = _fwd_bwd(dev, name, t, False)
        got_m = _fwd_bwd(dev, name, t, True)
    finally:
        ops.restore_math_mode(prev)
    if _dma_ok(name, CASES[name]):
        assert "mvae_pack_bf16" in seen
    _check(got, exp, f"{name}/{fam} bf16 .grad")
    _check(got_m, exp, f"{name}/{fam} bf16 main_grad")


@pytest.mark.parametrize("name,fam", _cases("I", only=lambda nm, c: _SMALL(nm, c)))
def test_conv_exact_fp32_mode_exact(dev, name, fam, monkeypatch):
    """ops.math_scope(2): every GEMM on the f32-input MFMA, no pre-split operand formed."""
    from medvae_disentangled_multimodal_amd import ops
    t, exp, _ = _problem(name, fam)
    seen = _spy(monkeypatch)
    with ops.math_scope(2):
        assert ops._MATH[0] == 2
        got = _fwd_bwd(dev, name, t, False)
        got_m = _fwd_bwd(dev, name, t, True)
    assert ops._MATH[0] == 0 and "mvae_split_bf16" not in seen
    _check(got, exp, f"{name}/{fam} fp32 .grad")
    _check(got_m, exp, f"{name}/{fam} fp32 main_grad")


@pytest.mark.parametrize("fam", ["I", "L"])
def test_upsample_gather_form_exact(dev, fam):
    """The gather form of Upsample's conv (mvae_conv2d_nhwc mode 1: 9 taps on the upsampled grid, no tap sums, so
    family-L weights stay exact), cin 3 and non-square included."""
    from medvae_disentangled_multimodal_amd import _lib
    for n, ci, co, h, w_ in ((3, 64, 32, 7, 9), (2, 3, 8, 5, 6)):
        g = torch.Generator().manual_seed(ci + (fam == "L"))
        x, wt = E.family(fam, (n, ci, h, w_), g), E.family(fam, (co, ci, 3, 3), g)
        b = E.family_i((co,), g)
        fwd, _, _ = E.conv_ops(x.shape, wt.shape, 1, P1, True)
        E.check_exact(fwd(x.abs(), wt.abs()) + 3, E.grid_of(fam), "ups gather")
        exp = E.emulate(fwd, x, wt) + b.double().view(1, -1, 1, 1)
        xd, wd, bd = cl(x, dev), cl(wt, dev), b.to(dev)
        y = torch.empty((n, co, 2 * h, 2 * w_), device=dev).contiguous(memory_format=CL)
        _lib.call("mvae_conv2d_nhwc", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), None, y.data_ptr(), n, h, w_, ci, co,
                  3, 3, 1, 1, 1, 2 * h, 2 * w_, 1, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        E.assert_exact(y, exp, "nchw", f"ups gather {ci}/{fam}")


@pytest.mark.parametrize("fam", ["I", "L"])
@pytest.mark.parametrize("ci,co,h,w,beta", [(32, 32, 28, 28, 0.0), (64, 32, 14, 14, 1.0), (32, 64, 14, 14, 0.5),
                                              (64, 64, 9, 11, 0.0)])
def test_wgrad_direct_capi_exact(dev, ci, co, h, w, beta, fam):
    """mvae_conv2d_wgrad_direct_nhwc for every (cin, cout) pair it takes (ops routes only cout 32 to it), dw and dbias
    accumulated with beta in {0, 1, 0.5} onto integers (0.5 * integer stays on the grid)."""
    from medvae_disentangled_multimodal_amd import _lib
    n = 3
    g = torch.Generator().manual_seed(ci * 3 + co + h + (fam == "L"))
    x, dy = E.family(fam, (n, ci, h, w), g), E.family(fam, (n, co, h, w), g)
    dw0, db0 = E.family_i((co, ci, 3, 3), g), E.family_i((co,), g)
    _, _, wgrad = E.conv_ops(x.shape, dw0.shape, 1, P1, False)
    grid = E.grid_of(fam) * 2
    E.check_exact(wgrad(dy.abs(), x.abs()) + 3, grid, "wgrad direct")
    E.check_exact(dy.abs().sum((0, 2, 3)) + 3, grid, "wgrad direct bias")
    exp_dw = beta * dw0.double() + E.emulate(wgrad, dy, x)
    exp_db = beta * db0.double() + dy.double().sum((0, 2, 3))
    xd, dyd = x.permute(0, 2, 3, 1).contiguous().to(dev), dy.permute(0, 2, 3, 1).contiguous().to(dev)
    dwd, dbd = dw0.permute(0, 2, 3, 1).contiguous().to(dev), db0.to(dev)
    ws = torch.empty(_lib.query("mvae_conv2d_wgrad_direct_workspace_bytes", n, h, w, ci, co), dtype=torch.uint8,
                     device=dev)
    _lib.call("mvae_conv2d_wgrad_direct_nhwc", dyd.data_ptr(), xd.data_ptr(), dwd.data_ptr(), dbd.data_ptr(),
              float(beta), n, h, w, ci, co, 0, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    E.assert_exact(dwd.permute(0, 3, 1, 2), exp_dw, "kcrs", f"wgrad direct {ci}->{co} dw")
    E.assert_exact(dbd, exp_db, "k", f"wgrad direct {ci}->{co} db")


@pytest.mark.parametrize("fam", ["I", "L"])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("m,n,k,batch", [(49, 100, 37, 2), (3, 200, 512, 1), (300, 260, 96, 2)])
def test_gemm_strided_batched_exact(dev, ta, tb, m, n, k, batch, fam):
    """C = 0.5 op(A) op(B) + bias + residual + 0.25 C0 (powers of two keep the grid: 2^-10 for family L, 1/4 for I);
    ragged M / N / K, a K of 16 K-tiles, and a multi-tile shape (300 x 260: tails in both directions)."""
    from medvae_disentangled_multimodal_amd import _lib
    g = torch.Generator().manual_seed(m * 7 + n + k + (fam == "L"))
    A = E.family(fam, (batch, k, m) if ta else (batch, m, k), g)
    B = E.family(fam, (batch, n, k) if tb else (batch, k, n), g)
    C0, bias, res = E.family_i((batch, m, n), g), E.family_i((n,), g), E.family_i((batch, m, n), g)
    op = lambda a, b: (a.transpose(1, 2) if ta else a) @ (b.transpose(1, 2) if tb else b)  # noqa: E731
    E.check_exact(op(A.abs(), B.abs()) + 9, E.grid_of(fam) * 4, "gemm")
    exp = 0.5 * E.emulate(op, A, B) + bias.double() + res.double() + 0.25 * C0.double()
    Ad, Bd, Cd, bd, rd = A.to(dev), B.to(dev), C0.to(dev).clone(), bias.to(dev), res.to(dev)
    ws = torch.empty(_lib.query("mvae_gemm_workspace_bytes", m, n, k, batch) + 16, dtype=torch.uint8, device=dev)
    _lib.call("mvae_gemm_strided_batched", ta, tb, m, n, k, 0.5, Ad.data_ptr(), m if ta else k, m * k, Bd.data_ptr(),
              k if tb else n, n * k, 0.25, Cd.data_ptr(), n, m * n, batch, bd.data_ptr(), rd.data_ptr(), n, m * n,
              ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    E.assert_exact(Cd, exp, ("batch", "m", "n"), f"gemm ta{ta} tb{tb} {m}x{n}x{k}/{fam}", {"m": 64, "n": 64})


# ------------------------------------------------------------------------------------------
# Winograd
# ------------------------------------------------------------------------------------------
# n, cin, cout, h, w: the ragged / edge-cut shapes of tests/test_gpu_winograd.py CASES and one wide-channel shape
WINO = [(3, 64, 64, 7, 7), (2, 32, 48, 14, 10), (2, 32, 96, 12, 8), (1, 256, 128, 4, 16), (2, 64, 32, 8, 32),
        (1, 32, 64, 12, 64), (2, 512, 512, 8, 8)]


def _wino_on(monkeypatch, tile):
    from medvae_disentangled_multimodal_amd import ops
    for k_, v in (("WINOGRAD", True), ("WINOGRAD_MIN_C", 1), ("WINOGRAD_MIN_C_WIDE", 1), ("WINOGRAD_TILE", tile),
                  ("WINOGRAD_MAX_W", 64), ("WINOGRAD_MIN_MACS", 0.0)):
        monkeypatch.setattr(ops, k_, v)
    return ops


def _wino_wgrad_kernel(ci, co):
    """ops routes the weight gradient of a (32 | 64) -> 32 channel conv to the direct kernel ahead of Winograd."""
    return "mvae_conv2d_wgrad_direct_nhwc" if ci in (32, 64) and co == 32 else "mvae_winograd_wgrad_gemm"


_wino_problem = E.wino_problem


def _wino_run(dev, ops, t, geom, with_res=True):
    xd, wd, bd = cl(t["x"], dev).requires_grad_(), cl(t["w"], dev).requires_grad_(), t["b"].to(dev).requires_grad_()
    y = ops.conv2d(xd, wd, bd, geom, residual=cl(t["res"], dev) if with_res else None)
    y.backward(cl(t["dy"], dev))
    torch.cuda.synchronize()
    return y.detach(), xd.grad, wd.grad, bd.grad


@pytest.mark.parametrize("n,ci,co,h,w", WINO)
def test_winograd_f2_exact_family_i(dev, n, ci, co, h, w, monkeypatch):
    """F(2x2, 3x3) forward (bias, residual), input gradient and weight gradient on integers. Precondition on the
    transformed operands: |V| <= 4 * 3 (B^T d B adds four inputs), |U| <= 9 * 3 / 4 on a 1/4 grid, so a position sum
    over cin stays below cin * 12 * 6.75 on a 1/4 grid and the output transform adds nine of them; the weight
    gradient sums |D'| |V| <= 144 over the tiles and its output transform (1/2 per side) adds nine on a 1/4 grid."""
    ops = _wino_on(monkeypatch, 2)
    geom = ops.ConvGeom(3, 3, 1, 1, 1, 1, 1, False)
    assert ops._wino_ok(geom, n, h, w, ci, co) and ops._wino_ok(geom, n, h, w, co, ci)
    t, (fwd, dgrad, wgrad) = _wino_problem(n, ci, co, h, w, "I", n * ci + h * w)
    tiles = n * -(-h // 2) * -(-w // 2)
    E.check_exact(torch.tensor(9.0 * max(ci, co) * 12 * 6.75 + 6), 4.0, "winograd position sums")
    E.check_exact(torch.tensor(9.0 * tiles * 144), 4.0, "winograd weight-gradient sums")
    f64 = lambda op: (lambda a, b: op(a.float(), b.float()).double())  # noqa: E731  (exact: integers, see _problem)
    exp = dict(y=E.emulate(f64(fwd), t["x"], t["w"]) + t["b"].double().view(1, -1, 1, 1) + t["res"].double(),
               dx=E.emulate(f64(dgrad), t["dy"], t["w"]), dw=E.emulate(f64(wgrad), t["dy"], t["x"]),
               db=t["dy"].double().sum((0, 2, 3)))
    seen = _spy(monkeypatch)
    got = _wino_run(dev, ops, t, geom)
    assert {"mvae_winograd_gemm", "mvae_winograd_output_transform", _wino_wgrad_kernel(ci, co)} <= set(seen)
    assert "mvae_conv2d_nhwc" not in seen and "mvae_conv2d_wgrad_nhwc" not in seen
    _check(got, exp, f"winograd F2 {n}x{ci}x{co}x{h}x{w}")


@pytest.mark.parametrize("n,ci,co,h,w", [(2, 32, 32, 8, 8), (1, 64, 16, 4, 12)])
def test_winograd_f2_upsample_exact_family_i(dev, n, ci, co, h, w, monkeypatch):
    """The Upsample conv as four Winograd class convs (class kernels are tap sums: integers up to 12)."""
    ops = _wino_on(monkeypatch, 2)
    geom = ops.ConvGeom(3, 3, 1, 1, 1, 1, 1, True)
    assert ops._wino_ups_ok(geom, n, h, w, ci, co)
    t, (fwd, dgrad, wgrad) = _wino_problem(n, ci, co, h, w, "I", 5 + ci, ups=True)
    E.check_exact(torch.tensor(9.0 * max(ci, 4 * co) * 12 * 27 + 6), 4.0, "winograd upsample position sums")
    E.check_exact(torch.tensor(9.0 * n * h * w * 144), 4.0, "winograd upsample weight-gradient sums")
    exp = dict(y=E.emulate(fwd, t["x"], t["w"]) + t["b"].double().view(1, -1, 1, 1),
               dx=E.emulate(dgrad, t["dy"], t["w"]), dw=E.emulate(wgrad, t["dy"], t["x"]),
               db=t["dy"].double().sum((0, 2, 3)))
    seen = _spy(monkeypatch)
    got = _wino_run(dev, ops, t, geom, with_res=False)
    assert "mvae_winograd_output_transform_upsample" in seen and "mvae_winograd_upsample_fold" in seen
    _check(got, exp, f"winograd F2 upsample {n}x{ci}x{co}x{h}x{w}")


@pytest.mark.parametrize("tile,fam", [(2, "L"), (4, "N"), (4, "L")])
@pytest.mark.parametrize("shape,ups", E.WINO_BOUNDED_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_winograd_bounded(dev, shape, ups, tile, fam, monkeypatch):
    """Where Winograd cannot be exact (F(2x2) on family L: split after the transform's additions, see the module
    docstring; F(4x4): 1/6 and 1/24 in the filter transform, on random normal inputs "N" and on family L), the plain
    conv and the Upsample class convs (output transform, class weight gradient and fold included), every element
    against float64: |got - ref| <= f * tau(K) * op(|a|, |b|), tau = 3 * 2^-18 + K * 2^-24 (exact_inputs.tau), K the
    direct conv's reduction length, f per shape and output from exact_inputs.wino_factor: 4 x the CPU statistic of the
    float64 emulation for F(4x4) (table WINO_MEASURED, regenerated by tests/test_exact_inputs.py), the derived 9 for
    F(2x2) on family L, where that statistic is 0."""
    n, ci, co, h, w = shape
    ops = _wino_on(monkeypatch, tile)
    geom = ops.ConvGeom(3, 3, 1, 1, 1, 1, 1, ups)
    assert ops._wino_ups_ok(geom, n, h, w, ci, co) if ups else ops._wino_ok(geom, n, h, w, ci, co)
    t, (fwd, dgrad, wgrad) = _wino_problem(n, ci, co, h, w, fam, E.wino_bounded_seed(n, ci, h), ups)
    d = lambda v: v.double()  # noqa: E731
    fy, fx, fw = E.wino_factor(tile, fam, shape, ups)
    seen = _spy(monkeypatch)
    y, dx, dw, db = _wino_run(dev, ops, t, geom, with_res=not ups)
    if ups:
        assert {"mvae_winograd_output_transform_upsample", "mvae_winograd_dy_transforms_upsample",
                "mvae_winograd_upsample_fold"} <= set(seen)
    else:
        assert "mvae_winograd_gemm" in seen and _wino_wgrad_kernel(ci, co) in seen
    x, wt, dy = t["x"], t["w"], t["dy"]
    res = 0 if ups else d(t["res"])
    ref_y = fwd(d(x), d(wt)) + d(t["b"]).view(1, -1, 1, 1) + res
    by = fy * E.tau(9 * ci) * (fwd(d(x).abs(), d(wt).abs()) + d(t["b"]).abs().view(1, -1, 1, 1) + abs(res))
    pix = dy.shape[0] * dy.shape[2] * dy.shape[3]
    for nm, got, ref, bound in (("y", y, ref_y, by),
                                ("dx", dx, dgrad(d(dy), d(wt)), fx * E.tau(9 * co) * dgrad(d(dy).abs(), d(wt).abs())),
                                ("dw", dw, wgrad(d(dy), d(x)), fw * E.tau(pix) * wgrad(d(dy).abs(), d(x).abs()))):
        err = ((got.detach().cpu().double() - ref).abs() / bound.clamp_min(1e-300)).max().item()
        print(f"winograd F{tile} {fam} ups={ups} {nm}: max |err| / bound = {err:.3f}")
        E.assert_within(got, ref, bound, "nchw" if nm != "dw" else "kcrs", f"winograd F{tile}/{fam} ups={ups} {nm}")
