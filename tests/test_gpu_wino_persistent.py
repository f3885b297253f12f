"""The persistent form of the Winograd position GEMM (csrc/gemm_core.h gemm3x_persist_kernel) against the per-tile
kernel it replaces (MVAE_NO_PERSISTENT_GEMM keeps every launch on gemm3x_kernel): M must be bitwise the same -- the
K-tile order, MFMA sequence and accumulation order are unchanged -- and a conv through it must meet the float64
Winograd emulation at the suite's tolerance for the arithmetic.

The persistent form serves the forward / input-gradient GEMMs (pre-split ROW x ROW operands) of at least two rounds of
256x256 or 256x128 tiles; the weight-gradient GEMM stays on gemm3x_kernel (its cases below compare that kernel with
itself under both settings: the dispatch must not change what it computes)."""
import pytest
import torch

import wino_ref

pytestmark = pytest.mark.gpu

CONV_TOL = 2e-4   # tests/test_gpu_winograd.py: 3xBF16 convs against float64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _operand(numel, dev, seed):
    """A pre-split GEMM operand (split4_bf16 groups of fp32 normals; finite under the exact mode's bit split too)."""
    from medvae_disentangled_multimodal_amd import _lib
    g = torch.Generator(device=dev).manual_seed(seed)
    t = torch.randn(numel, device=dev, generator=g)
    s = torch.empty_like(t)
    _lib.call("mvae_split_bf16", t.data_ptr(), s.data_ptr(), t.numel(), torch.cuda.current_stream().cuda_stream)
    return s


def _both(monkeypatch, fn, out_numel, dev):
    """fn(out) under the default dispatch and under MVAE_NO_PERSISTENT_GEMM, each into a NaN-filled buffer."""
    outs = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("MVAE_NO_PERSISTENT_GEMM", "1")
        else:
            monkeypatch.delenv("MVAE_NO_PERSISTENT_GEMM", raising=False)
        out = torch.full((out_numel,), float("nan"), device=dev)
        fn(out)
        outs.append(out)
    torch.cuda.synchronize()
    monkeypatch.delenv("MVAE_NO_PERSISTENT_GEMM", raising=False)
    return outs


# (tiles, k_in, n_out). A 256x256 launch has 256 workgroups, a round is 256 tiles.
GEMM_CASES = [
    (512 * 256 + 256, 64, 256),  # 513 row tiles per position: many rounds and a ragged last one, 2 K-tiles
    (300, 96, 260),              # M and N tails inside a tile, 3 K-tiles (under one round: the per-tile kernel)
    (256 * 600, 32, 256),        # a single K-tile: prologue and epilogue back to back
    (5000, 96, 260),             # 256x128 tiles with M and N tails, workgroups with 8 and 9 tiles (tile 4)
    (256 * 40 + 8, 64, 128),     # 256x128 tiles, one column of tiles
    (256 * 3, 160, 512),         # 256x256: tile 4 gives 216 tiles (one round), tile 2 96
    (256 * 6 + 4, 160, 512),     # 256x256: 14 tiles per position, 504 / 224 tiles: workgroups with 1 and 2 tiles
    (256 * 9, 128, 512),         # 256x256: 648 tiles (tile 4): workgroups with 2 and 3 tiles
]


@pytest.mark.parametrize("prec", ["32", "32-exact"])
@pytest.mark.parametrize("tile", [2, 4])
@pytest.mark.parametrize("tiles,k_in,n_out", GEMM_CASES)
def test_persistent_position_gemm_is_bitwise_the_per_tile_kernel(dev, monkeypatch, tiles, k_in, n_out, tile, prec):
    from medvae_disentangled_multimodal_amd import _lib, ops
    pos = (tile + 2) ** 2
    v = _operand(pos * tiles * k_in, dev, 1)
    u = _operand(pos * n_out * k_in, dev, 2)
    st = torch.cuda.current_stream().cuda_stream
    prev = ops.set_precision(prec)
    try:
        new, old = _both(monkeypatch, lambda m: _lib.call("mvae_winograd_gemm", v.data_ptr(), u.data_ptr(),
                                                          m.data_ptr(), tiles, k_in, n_out, tile, st),
                         pos * tiles * n_out, dev)
    finally:
        ops.restore_math_mode(prev)
    assert not bool(torch.isnan(old).any())
    assert torch.equal(new.view(torch.int32), old.view(torch.int32))


@pytest.mark.parametrize("prec", ["32", "32-exact"])
@pytest.mark.parametrize("tile", [2, 4])
@pytest.mark.parametrize("tiles,cout,cin", [(1024, 512, 768), (37 * 32, 260, 256)])
def test_weight_gradient_gemm_is_unchanged(dev, monkeypatch, tiles, cout, cin, tile, prec):
    from medvae_disentangled_multimodal_amd import _lib, ops
    pos = (tile + 2) ** 2
    d = _operand(pos * tiles * cout, dev, 3)
    v = _operand(pos * tiles * cin, dev, 4)
    ws = torch.empty(_lib.query("mvae_gemm_workspace_bytes", cout, cin, tiles, pos), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    prev = ops.set_precision(prec)
    try:
        new, old = _both(monkeypatch, lambda m: _lib.call("mvae_winograd_wgrad_gemm", d.data_ptr(), v.data_ptr(),
                                                          m.data_ptr(), tiles, cout, cin, tile, ws.data_ptr(),
                                                          ws.numel(), st),
                         pos * cout * cin, dev)
    finally:
        ops.restore_math_mode(prev)
    assert not bool(torch.isnan(old).any())
    assert torch.equal(new.view(torch.int32), old.view(torch.int32))


def _wino_flags(monkeypatch, tile):
    from medvae_disentangled_multimodal_amd import ops
    monkeypatch.setattr(ops, "WINOGRAD", True)
    monkeypatch.setattr(ops, "WINOGRAD_MIN_C", 1)
    monkeypatch.setattr(ops, "WINOGRAD_MIN_C_WIDE", 1)
    monkeypatch.setattr(ops, "WINOGRAD_TILE", tile)
    monkeypatch.setattr(ops, "WINOGRAD_MAX_W", 64)
    monkeypatch.setattr(ops, "WINOGRAD_MIN_MACS", 0.0)


def test_forward_through_the_persistent_gemm_matches_float64(dev, monkeypatch):
    """16 images of 64x64 at 64 -> 256 channels, F(4x4): 4096 GEMM rows, 16 tiles of 256x256 per position, 576 in all
    -- two full rounds on the persistent kernel and a finer-tiled remainder launch. Sampled output pixels against the
    float64 emulation (unrounded operands: the 3xBF16 arithmetic is an fp32 emulation)."""
    from medvae_disentangled_multimodal_amd import _lib, ops
    _wino_flags(monkeypatch, 4)
    n, ci, co, h, w = 16, 64, 256, 64, 64
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, ci, h, w, generator=g)
    wt = torch.randn(co, ci, 3, 3, generator=g) / (3 * ci ** 0.5)
    b = torch.randn(co, generator=g)
    geom = ops.ConvGeom(3, 3, 1, 1, 1, 1, 1, False)
    assert ops._wino_ok(geom, n, h, w, ci, co)
    seen = []
    orig = _lib.call

    def spy(name, *args):
        seen.append(name)
        return orig(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)
    y = ops.conv2d_forward_raw(cl(x), cl(wt), b.to(dev), None, geom)
    monkeypatch.setattr(_lib, "call", orig)
    torch.cuda.synchronize()
    assert "mvae_winograd_gemm" in seen
    s = 512
    ns = torch.randint(0, n, (s,), generator=g)
    oh = torch.randint(0, h, (s,), generator=g)
    ow = torch.randint(0, w, (s,), generator=g)
    ref = wino_ref.rows(x, wt, b, ns, oh, ow, 4, wino_ref.ident)
    got = y.cpu().double()[ns, :, oh, ow]
    err = float((got - ref).norm() / ref.norm())
    assert err < CONV_TOL, err


def test_weight_gradient_matches_float64(dev, monkeypatch):
    from medvae_disentangled_multimodal_amd import ops
    _wino_flags(monkeypatch, 4)
    n, ci, co, h, w = 2, 64, 64, 16, 16
    g = torch.Generator().manual_seed(12)
    x = torch.randn(n, ci, h, w, generator=g)
    dy = torch.randn(n, co, h, w, generator=g)
    geom = ops.ConvGeom(3, 3, 1, 1, 1, 1, 1, False)
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)
    xd, dyd = cl(x), cl(dy)
    dw = cl(torch.zeros(co, ci, 3, 3))
    assert ops._wino_wgrad_ok(geom, xd, dyd, dw, None)
    ops.conv2d_wgrad_raw(dyd, xd, dw, 0.0, geom)
    torch.cuda.synchronize()
    ref = wino_ref.wgrad(x, dy, 4, wino_ref.ident)
    err = float((dw.cpu().double() - ref).norm() / ref.norm())
    assert err < CONV_TOL, err
