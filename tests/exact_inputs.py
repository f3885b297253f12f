"""Inputs on which the 3xBF16 / bf16 / fp32 MFMA paths of the conv / GEMM kernels are exact, and element-wise reporters.

3xBF16 (csrc/gemm_core.h:10-13): an fp32 operand x is split into hi = bf16(x), lo = bf16(x - hi) and a product is
hi*hi + hi*lo + lo*hi in an fp32 accumulator (lo*lo is dropped by design).

Family I: integers in {-3..3}. Every value is a bf16 number (hi = x, lo = 0); products and fp32 sums are exact while
the sum of absolute terms stays below 2^24, in any summation order.

Family L: x = s*a + t*2^-9, a in {2, 3}, s, t in {-1, +1}. bf16 has 8 significant bits, so in [2, 4) its spacing is
2^-6 and x lies 1/8 of a spacing from s*a: hi = s*a with no round-to-even tie (0 and +-1 are left out: 2^-9 next to them
is representable or a tie), lo = t*2^-9 exactly and hi + lo == x. The kernel's value is then
op(hi_a, hi_b) + op(hi_a, lo_b) + op(lo_a, hi_b) -- not op(a, b) -- on a 2^-9 grid (hi*lo) of which the products
hi*hi are multiples, so fp32 sums are exact while (sum of absolute terms) * 2^9 < 2^24.

Test infrastructure only (no kernel is called here)."""
import math

import torch
import torch.nn.functional as F

GRID = {"I": 1.0, "L": 512.0}
LIMIT = float(2 ** 24)


def family_i(shape, gen):
    return torch.randint(-3, 4, tuple(shape), generator=gen).float()


def family_l(shape, gen):
    a = torch.randint(2, 4, tuple(shape), generator=gen).float()
    s = torch.randint(0, 2, tuple(shape), generator=gen).float() * 2 - 1
    t = torch.randint(0, 2, tuple(shape), generator=gen).float() * 2 - 1
    return s * a + t * 2.0 ** -9


def family(name, shape, gen):
    return family_l(shape, gen) if name == "L" else family_i(shape, gen)


def split(x):
    """(hi, lo) of the 3xBF16 split as float64 tensors: hi = RNE_bf16(x), lo = RNE_bf16(x - hi)."""
    x = x.float()
    hi = x.bfloat16().float()
    lo = (x - hi).bfloat16().float()
    return hi.double(), lo.double()


def emulate(op, a, b):
    """The 3xBF16 value of the bilinear `op` (a float64 conv / GEMM) on fp32 operands a, b: three calls of op."""
    ha, la = split(a)
    hb, lb = split(b)
    return op(ha, hb) + op(ha, lb) + op(la, hb)


def emulate_hi_only(op, a, b):
    """What a kernel that dropped the cross terms would give (used to show that the exact tests see that)."""
    return op(split(a)[0], split(b)[0])


def grid_of(*fams):
    return max(GRID[f] for f in fams)


def check_exact(abs_bound, grid, what=""):
    """The exactness precondition (a condition on the inputs): abs_bound = op(|a|, |b|) + |bias| + |residual| element
    by element; every partial sum of the kernel is a multiple of 1/grid below 2^24/grid, i.e. an fp32 number."""
    m = float(abs_bound.max())
    if not m * grid < LIMIT:
        raise AssertionError(f"{what}: not exact in fp32: max |terms| {m:.0f} x grid {grid:.0f} >= 2^24 -- shrink the shape")


# ------------------------------------------------------------------------------------------
# float64 references of the conv (as bilinear ops)
# ------------------------------------------------------------------------------------------
def conv_fwd(x, w, k, stride, pads, ups):
    """y of the project's conv geometry: nearest x2 (ups), pad (t, l, b, r), k x k conv at `stride`."""
    if ups:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    t, l, b, r = pads
    return F.conv2d(F.pad(x, (l, r, t, b)), w, None, stride=stride)


def conv_ops(x_shape, w_shape, stride, pads, ups):
    """(fwd(x, w), dgrad(dy, w), wgrad(dy, x)) of one geometry, each bilinear in its two arguments, in the arguments'
    dtype (float64, or float32 where the caller has checked the precondition: exact either way)."""
    k = w_shape[2]

    def fwd(x, w):
        return conv_fwd(x, w, k, stride, pads, ups)

    def dgrad(dy, w):
        x0 = torch.zeros(x_shape, dtype=dy.dtype, requires_grad=True)
        return torch.autograd.grad(conv_fwd(x0, w, k, stride, pads, ups), x0, dy)[0]

    def wgrad(dy, x):
        w0 = torch.zeros(w_shape, dtype=dy.dtype, requires_grad=True)
        return torch.autograd.grad(conv_fwd(x, w0, k, stride, pads, ups), w0, dy)[0]

    return fwd, dgrad, wgrad


# ------------------------------------------------------------------------------------------
# element-wise reporters
# ------------------------------------------------------------------------------------------
def _where(idx, shape, names, tile):
    parts = []
    for d, (i, n) in enumerate(zip(idx, shape)):
        nm = names[d] if names and d < len(names) else f"d{d}"
        tag = " first" if i == 0 and n > 1 else (" last" if i == n - 1 and n > 1 else "")
        if tile and tile.get(nm):
            t = tile[nm]
            tag += f" tile {i // t}+{i % t}" + ("(tail tile)" if (i // t) == (n - 1) // t and n % t else "")
        parts.append(f"{nm}={i}/{n}{tag}")
    return ", ".join(parts)


def _report(kind, bad, got, exp, names, tile, extra=None, limit=8):
    idx = bad.nonzero()
    lines = [f"{kind}: {idx.shape[0]} of {bad.numel()} elements wrong"]
    for row in idx[:limit].tolist():
        r = tuple(row)
        s = f"  [{_where(r, got.shape, names, tile)}] got {got[r].item()!r} expected {exp[r].item()!r}"
        if extra is not None:
            s += f" (allowed {extra[r].item():.3e})"
        lines.append(s)
    for d in range(got.dim()):  # which index values along each axis hold errors: a whole edge / tile shows at once
        vals = idx[:, d].unique().tolist()
        nm = names[d] if names and d < len(names) else f"d{d}"
        lines.append(f"  {nm}: {len(vals)} of {got.shape[d]} indices, " + (str(vals) if len(vals) <= 12 else
                                                                           f"{vals[:6]} .. {vals[-6:]}"))
    return "\n".join(lines)


def assert_exact(got, expected, names=None, what="", tile=None):
    """got == expected in every element (bitwise up to the sign of zero), both taken to float64 on the CPU."""
    g = got.detach().cpu().double()
    e = expected.detach().cpu().double()
    assert g.shape == e.shape, (what, tuple(g.shape), tuple(e.shape))
    bad = ~(g == e)  # (NaN counts as wrong)
    if bool(bad.any()):
        raise AssertionError(_report(f"{what}: not exact", bad, g, e, names, tile))


def assert_within(got, ref, bound, names=None, what="", tile=None):
    """|got - ref| <= bound in every element (bound: a tensor of got's shape, or a scalar)."""
    g = got.detach().cpu().double()
    r = ref.detach().cpu().double()
    b = torch.as_tensor(bound, dtype=torch.float64).expand_as(r)
    assert g.shape == r.shape, (what, tuple(g.shape), tuple(r.shape))
    bad = ~((g - r).abs() <= b)
    if bool(bad.any()):
        raise AssertionError(_report(f"{what}: outside the bound", bad, g, r, names, tile, extra=b))


def tau(k):
    """Element-wise relative bound of a 3xBF16 product sum of k terms against sum |a||b|: each operand's split leaves
    |x - hi - lo| <= 2^-18 |x| (two of them), the dropped lo*lo <= 2^-18 |a||b|, plus worst-case fp32 accumulation."""
    return 3 * 2.0 ** -18 + k * 2.0 ** -24


def ulp32(t):
    """fp32 unit in the last place of |t| (float64 tensor of t's shape; the smallest normal's for tiny values)."""
    a = t.detach().double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


# ------------------------------------------------------------------------------------------
# Winograd: problems and the CPU statistic behind the element-wise bound of the paths that cannot be exact
# ------------------------------------------------------------------------------------------
def wino_problem(n, ci, co, h, w_, fam, seed, ups=False):
    """x, w, bias, residual, dy of a 3x3 / pad-1 conv (Upsample's when ups) from family I / L, or random normal ("N":
    weights scaled by 1 / sqrt(9 cin)); bias and residual are integers. Returns (tensors, (fwd, dgrad, wgrad))."""
    g = torch.Generator().manual_seed(seed)
    draw = (lambda s: family(fam, s, g)) if fam in "IL" else (lambda s: torch.randn(s, generator=g))
    x, wt = draw((n, ci, h, w_)), draw((co, ci, 3, 3))
    if fam not in "IL":
        wt = wt / math.sqrt(9 * ci)
    ops = conv_ops(x.shape, wt.shape, 1, (1, 1, 1, 1), ups)
    ho, wo = (2 * h, 2 * w_) if ups else (h, w_)
    b, res, dy = family_i((co,), g), family_i((n, co, ho, wo), g), draw((n, co, ho, wo))
    return dict(x=x, w=wt, b=b, res=res, dy=dy), ops


def round_split(t):
    """hi + lo of the 3xBF16 split of a float64 tensor: what the Winograd GEMMs see of V, U and D'."""
    hi, lo = split(t)
    return hi + lo


def wino_bounded_seed(n, ci, h):
    return 3 * n + ci + h


def wino_statistic(tile, fam, shape, ups):
    """max |emulation - conv64| / (tau(K) op(|a|, |b|)) for y, dx, dw: the float64 Winograd emulation of tests/wino_ref.py
    with V, U, D' rounded to hi + lo, against the plain float64 conv, on the problem the GPU test of the same
    (tile, family, shape) uses. K: the direct conv's reduction length."""
    import wino_ref as WR
    n, ci, co, h, w_ = shape
    t, (fwd, dgrad, wgrad) = wino_problem(n, ci, co, h, w_, fam, wino_bounded_seed(n, ci, h), ups)
    x, wt, dy = t["x"].double(), t["w"].double(), t["dy"].double()
    if ups:
        ey, ex, ew = WR.ups_conv(x, wt, tile, round_split), WR.ups_dgrad(dy, wt, tile, round_split), \
            WR.ups_wgrad(x, dy, tile, round_split)
    else:
        ey, ex, ew = WR.conv(x, wt, tile, round_split), WR.conv(dy, WR.dgrad_weights(wt), tile, round_split), \
            WR.wgrad(x, dy, tile, round_split)
    pix = dy.shape[0] * dy.shape[2] * dy.shape[3]

    def stat(e, ref, k, ab):
        return float(((e - ref).abs() / (tau(k) * ab)).max())
    return (stat(ey, fwd(x, wt), 9 * ci, fwd(x.abs(), wt.abs())),
            stat(ex, dgrad(dy, wt), 9 * co, dgrad(dy.abs(), wt.abs())),
            stat(ew, wgrad(dy, x), pix, wgrad(dy.abs(), x.abs())))


WINO_BOUNDED_SHAPES = [((3, 64, 64, 7, 7), False), ((2, 32, 48, 14, 10), False), ((1, 256, 128, 4, 16), False),
                       ((2, 64, 32, 8, 32), False), ((2, 32, 32, 8, 8), True), ((1, 64, 16, 4, 12), True)]

# wino_statistic (y, dx, dw) of F(4x4) on the shapes above, random normal ("N") and family L, measured on the CPU
# (tests/test_exact_inputs.py regenerates it and compares). F(2x2) on family L gives 0 everywhere: its V and U are
# hi + lo exactly, so nothing can be taken from the emulation and the factor is derived instead (wino_factor).
WINO_MEASURED = {
    (4, "N", (3, 64, 64, 7, 7), False): (0.4113, 0.5304, 3.34),
    (4, "N", (2, 32, 48, 14, 10), False): (1.2, 0.8079, 1.055),
    (4, "N", (1, 256, 128, 4, 16), False): (0.1223, 0.4493, 14.73),
    (4, "N", (2, 64, 32, 8, 32), False): (1.247, 2.619, 0.823),
    (4, "N", (2, 32, 32, 8, 8), True): (2.168, 0.5388, 0.3311),
    (4, "N", (1, 64, 16, 4, 12), True): (1.041, 1.127, 1.215),
    (4, "L", (3, 64, 64, 7, 7), False): (0.1712, 0.1775, 0.4937),
    (4, "L", (2, 32, 48, 14, 10), False): (0.4158, 0.271, 0.2582),
    (4, "L", (1, 256, 128, 4, 16), False): (0.06556, 0.1867, 1.965),
    (4, "L", (2, 64, 32, 8, 32), False): (0.4796, 0.8446, 0.1561),
    (4, "L", (2, 32, 32, 8, 8), True): (0.6374, 0.1881, 0.1339),
    (4, "L", (1, 64, 16, 4, 12), True): (0.2978, 0.4213, 0.3154),
}


def wino_factor(tile, fam, shape, ups):
    """Factors (y, dx, dw) of the bound f * tau(K) * op(|a|, |b|) for a Winograd conv that cannot be exact.
    F(4x4): the measured statistic of this shape times 4, for the fp32 (not float64) transform rounding that the
    emulation does not model. F(2x2) on family L: the errors left (the dropped lo*lo, fp32 accumulation) are relative to
    |V||U| summed over the positions, not to the direct taps; per side the transforms' largest absolute row sums are
    |A^T| 3, |B^T| 2, |G| 1.5, so that sum is at most (3 * 2 * 1.5)^2 = 81 times a 3x3 window's |x||w| where the direct
    sum has 9 taps: f = 9 (wider than the plain tau of a direct conv, by this derivation)."""
    if tile == 2:
        return (9.0, 9.0, 9.0)
    return tuple(4.0 * v for v in WINO_MEASURED[(tile, fam, tuple(shape), bool(ups))])
