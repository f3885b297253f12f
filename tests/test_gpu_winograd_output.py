"""The Winograd output transforms (csrc/winograd.hip: wino_out_kernel, wino_out_any_kernel, wino_out_ups_kernel) driven
directly through their C entry points on a synthetic M -- no GEMM in front of them.

Exact-integer cases: M, bias and residual are small integers (|M| <= 64). A^T has integer entries (largest row sum of
|A^T| is 19 for m = 4), so every intermediate of y = A^T M A + bias + residual is an integer below 19^2 * 64 + 128 <
2^24 -- exact in fp32 whatever the operation order -- and the 32-pixel block sums {sum y, sum y^2} (< 128 * 2^30 <
2^53) are exact in fp64 for any summation order: everything is compared with torch.equal against float64.

GroupNorm-backward partials (random M and x): dx must equal the plain variant's bit for bit; the partials are held to
the bound test_gpu_winograd.py applies against float64 (1e-5 norm-wise relative).

Every y is prefilled with NaN (a hole in the thread mapping cannot hide), and every statistics / partials case runs
twice and must repeat bit for bit (no atomics)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

AT = {2: torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64),
      4: torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]],
                      dtype=torch.float64)}

# (n, H, W, N): the smallest shapes reaching every WSEG / TR branch of the block kernel (W = 8, 16, 32, 64 = two
# segments per row, H != W), N = 40 and 36: channel-group counts no workgroup divides (a tail of idle lanes)
BLOCK_GEOS = [(2, 8, 8, 64), (2, 16, 16, 40), (1, 32, 32, 64), (1, 64, 64, 32), (2, 8, 32, 40)]
ANY_GEOS = [(3, 7, 7, 64), (1, 12, 20, 36)]  # wino_out_any: edge tiles cut
BLOCK_CASES = [(g, 4) for g in BLOCK_GEOS] + [(g, 2) for g in BLOCK_GEOS[:2]]  # tile 2 at W = 8: TR = 2


def _id(case):
    (n, h, w, c), tile = case
    return f"n{n}_{h}x{w}x{c}_F{tile}"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _int_m(tile, n, h, w, cols, seed):
    g = torch.Generator().manual_seed(seed)
    th, tw = -(-h // tile), -(-w // tile)
    return torch.randint(-64, 65, ((tile + 2) ** 2, n * th * tw, cols), generator=g).float()


def _transform64(m, tile, n, h, w):
    """A^T M A of M [a^2][T][cols] in float64 -> [n][h][w][cols] (edge tiles cut)."""
    al, th, tw = tile + 2, -(-h // tile), -(-w // tile)
    mt = m.double().reshape(al, al, n, th, tw, -1)
    y = torch.einsum("ai,ijbhwc,ej->bhawec", AT[tile], mt, AT[tile])
    return y.reshape(n, th * tile, tw * tile, -1)[:, :h, :w].contiguous()


def _stats64(y):
    """{sum, sum of squares} per 32-pixel block and 4-channel group of an NHWC float64 tensor."""
    n, h, w, c = y.shape
    t = y.reshape(n * h * w // 32, 32, c // 4, 4)
    return torch.stack([t.sum((1, 3)), (t * t).sum((1, 3))], -1).flatten()


def _out(dev, m, bias, res, n, h, w, c, tile, stats):
    """mvae_winograd_output_transform on a NaN-prefilled y -> (y, statistics or None), on the CPU."""
    from medvae_disentangled_multimodal_amd import _lib
    md = m.to(dev)
    bd = bias.to(dev) if bias is not None else None
    rd = res.to(dev) if res is not None else None
    y = torch.full((n, h, w, c), float("nan"), device=dev)
    part = torch.full((n * h * w // 32 * (c // 4) * 2,), float("nan"), device=dev, dtype=torch.float64) if stats else None
    _lib.call("mvae_winograd_output_transform", md.data_ptr(), bd.data_ptr() if bd is not None else None,
              rd.data_ptr() if rd is not None else None, y.data_ptr(), part.data_ptr() if stats else None, n, h, w, c,
              tile, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return y.cpu(), part.cpu() if stats else None


def _int_operands(n, h, w, c, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-64, 65, (c,), generator=g).float(), torch.randint(-64, 65, (n, h, w, c), generator=g).float())


@pytest.mark.parametrize("case", BLOCK_CASES, ids=_id)
def test_plain_exact(dev, case):
    (n, h, w, c), tile = case
    m = _int_m(tile, n, h, w, c, 1)
    bias, res = _int_operands(n, h, w, c, 2)
    y, _ = _out(dev, m, bias, res, n, h, w, c, tile, False)
    assert not torch.isnan(y).any()
    assert torch.equal(y.double(), _transform64(m, tile, n, h, w) + bias.double() + res.double())
    y0, _ = _out(dev, m, None, None, n, h, w, c, tile, False)  # (no bias, no residual: the input gradient's call)
    assert torch.equal(y0.double(), _transform64(m, tile, n, h, w))


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("case", BLOCK_CASES, ids=_id)
def test_statistics_exact(dev, case, with_res):
    (n, h, w, c), tile = case
    m = _int_m(tile, n, h, w, c, 3)
    bias, res = _int_operands(n, h, w, c, 4)
    if not with_res:
        res = None
    y, part = _out(dev, m, bias, res, n, h, w, c, tile, True)
    assert not torch.isnan(y).any() and not torch.isnan(part).any()
    want = _transform64(m, tile, n, h, w) + bias.double() + (res.double() if with_res else 0.0)
    assert torch.equal(y.double(), want)
    assert torch.equal(part, _stats64(want))
    y2, part2 = _out(dev, m, bias, res, n, h, w, c, tile, True)
    assert torch.equal(y, y2) and torch.equal(part, part2)


@pytest.mark.parametrize("case", [(g, 4) for g in ANY_GEOS] + [(ANY_GEOS[0], 2)], ids=_id)
def test_any_geometry_exact(dev, case):
    (n, h, w, c), tile = case
    m = _int_m(tile, n, h, w, c, 5)
    bias, res = _int_operands(n, h, w, c, 6)
    y, _ = _out(dev, m, bias, res, n, h, w, c, tile, False)
    assert not torch.isnan(y).any()
    assert torch.equal(y.double(), _transform64(m, tile, n, h, w) + bias.double() + res.double())


@pytest.mark.parametrize("case", [((2, 8, 8, 64), 4), ((2, 16, 16, 40), 4), ((1, 12, 20, 36), 4), ((2, 8, 8, 64), 2),
                                  ((2, 16, 16, 40), 2)], ids=_id)
def test_upsample_exact(dev, case):
    """M [a^2][T][4 cout], columns class-major (pq cout + c): y[2i + p][2j + q] = (A^T M_pq A)[i][j] + bias."""
    from medvae_disentangled_multimodal_amd import _lib
    (n, h, w, c), tile = case
    m = _int_m(tile, n, h, w, 4 * c, 7)
    bias, _ = _int_operands(1, 1, 1, c, 8)
    md, bd = m.to(dev), bias.to(dev)
    y = torch.full((n, 2 * h, 2 * w, c), float("nan"), device=dev)
    _lib.call("mvae_winograd_output_transform_upsample", md.data_ptr(), bd.data_ptr(), y.data_ptr(), n, h, w, c, tile,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    y = y.cpu()
    assert not torch.isnan(y).any()
    lo = _transform64(m, tile, n, h, w).reshape(n, h, w, 2, 2, c)  # [b][i][j][p][q][c]
    want = lo.permute(0, 1, 3, 2, 4, 5).reshape(n, 2 * h, 2 * w, c) + bias.double()
    assert torch.equal(y.double(), want)


GNB_CASES = [((n, h, w, 40), t) for ((n, h, w, _), t) in BLOCK_CASES]


@pytest.mark.parametrize("silu", [0, 1], ids=["nosilu", "silu"])
@pytest.mark.parametrize("case", GNB_CASES, ids=_id)
def test_gn_backward_partials(dev, case, silu):
    """N = 40 in 10 groups: 4 channels per GroupNorm group, the tightest case in which no 4-channel group straddles."""
    from medvae_disentangled_multimodal_amd import _lib
    (n, h, w, c), tile = case
    groups = 10
    g = torch.Generator().manual_seed(9 + silu)
    al, th, tw = tile + 2, h // tile, w // tile
    m = torch.randn(al * al, n * th * tw, c, generator=g)
    x = torch.randn(n, h, w, c, generator=g) * 1.5 + 0.3
    gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    xs = x.double().reshape(n, h * w, groups, c // groups)
    mean = xs.mean((1, 3)).float()
    rstd = (xs.var((1, 3), unbiased=False) + 1e-6).rsqrt().float()
    md, xd, gd, bd = m.to(dev), x.to(dev), gamma.to(dev), beta.to(dev)
    mu, rs = mean.flatten().to(dev), rstd.flatten().to(dev)

    def run():
        dx = torch.full((n, h, w, c), float("nan"), device=dev)
        part = torch.full((n * h * w // 32 * c * 2,), float("nan"), device=dev, dtype=torch.float64)
        _lib.call("mvae_winograd_output_gnbwd", md.data_ptr(), dx.data_ptr(), xd.data_ptr(), mu.data_ptr(),
                  rs.data_ptr(), gd.data_ptr(), bd.data_ptr(), groups, silu, part.data_ptr(), n, h, w, c, tile,
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return dx.cpu(), part.cpu()

    dx, part = run()
    assert not torch.isnan(dx).any() and not torch.isnan(part).any()
    plain, _ = _out(dev, m, None, None, n, h, w, c, tile, False)
    assert torch.equal(dx, plain)
    xh = ((xs - mean.double()[:, None, :, None]) * rstd.double()[:, None, :, None]).reshape(n, h, w, c)
    d = dx.double()
    if silu:
        yn = xh * gamma.double() + beta.double()
        sg = torch.sigmoid(yn)
        d = d * sg * (1 + yn * (1 - sg))
    blk = lambda t: t.reshape(n * h * w // 32, 32, c).sum(1)  # noqa: E731
    want = torch.stack([blk(d), blk(d * xh)], -1).flatten()
    err = float((part - want).norm() / want.norm())
    print(f"gnb partials {case} silu={silu}: rel {err:.3e}")
    assert err < 1e-5
    dx2, part2 = run()
    assert torch.equal(dx, dx2) and torch.equal(part, part2)
