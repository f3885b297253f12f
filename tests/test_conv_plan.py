"""ops.plan_conv on the host: the flagship shapes' families, and the facts that tie GroupNorm, conv2d and the conv
backward together -- they read one plan, so they cannot disagree. No GPU needed."""
import itertools
import subprocess
import sys

import pytest
import torch

from medvae_disentangled_multimodal_amd import ops

G3 = ops.G3
UP = ops.ConvGeom(3, 3, 1, 1, 1, 1, 1, True)
DOWN = ops.ConvGeom(3, 3, 2, 0, 0, 1, 1)
P1 = ops.ConvGeom(1, 1)
SWITCHES = dict(WINOGRAD=True, WINOGRAD_TILE=4, WINOGRAD_TILE_BF16=2, WINOGRAD_MAX_W=64, WINOGRAD_BF16_MAX_W=16,
                WINOGRAD_MIN_C=512, WINOGRAD_MIN_C_WIDE=256, WINOGRAD_MIN_MACS=1e10, WINOGRAD_EXACT=True,
                WINOGRAD_BF16=True, WINOGRAD_UPSAMPLE=True, WINOGRAD_UPSAMPLE_BF16=False, WINOGRAD_WGRAD=True,
                WINOGRAD_GN=True, WINOGRAD_DY_FP32=True, SUBPIXEL_UPSAMPLE=True, STRIDE2_CLASSES=True, DIRECT32=True,
                DIRECT_WGRAD=True, SMALL_COUT_WGRAD=True, BF16_DMA=True, PLANAR_DMA=False, DYPACK=True, DYSPLIT=True,
                DYBIAS=True, GN_BWD_FUSED=False, DYSPLIT_MIN_MACS=1e11)


@pytest.fixture
def rules(monkeypatch):
    for k, v in SWITCHES.items():
        monkeypatch.setattr(ops, k, v)
    monkeypatch.setattr(ops, "_MATH", [0])  # (a private list: the process-wide mode is untouched)
    return monkeypatch


def test_c4_levels(rules):
    """c4 at B = 256 in the 3xBF16 arithmetic: all three passes of every wide 3x3 level on Winograd F(4x4)."""
    for h, c in ((8, 2048), (16, 1024), (32, 512), (64, 256)):
        p = ops.plan_conv(G3, 256, c, h, h, c, 0)
        assert (p.fwd[0], p.dgrad[0], p.wgrad[0]) == ("wino", "wino", "wino")
        assert (p.tile, p.elsize, p.chunks) == (4, 4, ((0, 256),))
        assert p.alg("wino") == pytest.approx(p.ref / 4) and p.ref == 2.0 * 256 * h * h * c * c * 9
        assert p.gn_on_load and p.dy_format == "bias"  # dy read in fp32: the GroupNorm sums the bias gradient only
    p = ops.plan_conv(G3, 256, 512, 64, 64, 256, 0)
    assert p.fwd[0] == "wino" and len(p.chunks) == 2 and p.chunks[0][0] == 0 and p.chunks[-1][1] == 256
    p = ops.plan_conv(G3, 256, 128, 64, 64, 128, 0)   # 128 channels: the implicit GEMM, dy pre-split by the GroupNorm
    assert (p.fwd, p.dgrad, p.wgrad) == (("gemm",), ("gemm",), ("gemm",))
    assert p.chunks == () and not p.gn_on_load and p.dy_format == "split" and p.dy_copy_ok
    assert p.alg("gemm") == p.ref
    p = ops.plan_conv(UP, 256, 512, 32, 32, 256, 0)   # Upsample: four class convs on the low-resolution input
    assert (p.fwd, p.dgrad, p.wgrad) == (("wino_ups", "subpixel"), ("wino_ups", "upsample"),
                                          ("wino_ups", "subpixel", "gemm"))
    assert p.alg("subpixel") == pytest.approx(p.ref * 4 / 9) and p.dy_format == "bias" and not p.gn_on_load
    p = ops.plan_conv(DOWN, 256, 256, 64, 64, 256, 0)
    assert (p.fwd, p.dgrad, p.wgrad) == (("gemm",), ("stride2", "gemm"), ("gemm",))
    p = ops.plan_conv(P1, 256, 1024, 16, 16, 1024, 0)
    assert (p.fwd, p.dgrad, p.wgrad) == (("pointwise",), ("pointwise",), ("pointwise", "gemm"))
    p = ops.plan_conv(G3, 256, 256, 64, 64, 3, 0)     # Decoder.conv_out
    assert p.wgrad[0] == "small_cout" and p.fwd == ("gemm",)


def test_small_levels_and_math_modes(rules):
    p = ops.plan_conv(G3, 512, 32, 28, 28, 32, 0)     # c3's 28x28 level
    assert (p.fwd[0], p.dgrad[0], p.wgrad[0]) == ("direct32", "direct32", "direct")
    assert ops.plan_conv(G3, 32, 512, 7, 7, 512, 0).fwd == ("gemm",)  # c1 at B = 32: below WINOGRAD_MIN_MACS
    # bf16-mixed (c5): F(2x2) on packed bf16 up to width 16, the LDS-DMA GEMM on packed operands elsewhere
    for h, c in ((8, 2048), (16, 1024)):
        p = ops.plan_conv(G3, 256, c, h, h, c, 1)
        assert p.fwd[0] == "wino" and (p.tile, p.elsize) == (2, 2) and p.alg("wino") == pytest.approx(p.ref * 4 / 9)
        assert p.dy_format == "bias" and not p.dy_pack
    p = ops.plan_conv(G3, 256, 512, 32, 32, 512, 1)
    assert (p.fwd[0], p.dgrad[0], p.wgrad[0]) == ("dma", "dma", "dma")
    assert p.dy_format == "packed" and p.dy_pack and p.dy_copy_ok and not p.gn_on_load
    p = ops.plan_conv(UP, 256, 512, 32, 32, 256, 1)   # upsample-Winograd off in bf16-mixed
    assert p.wino is None and p.fwd == ("dma", "subpixel") and p.alg("subpixel") == pytest.approx(p.ref * 4 / 9)
    # exact fp32 (c4x): F(4x4) at every c4 level, no value-split operand anywhere
    p = ops.plan_conv(G3, 256, 512, 64, 64, 256, 2)
    assert p.fwd[0] == "wino" and p.tile == 4 and len(p.chunks) == 2 and p.dy_format == "bias"
    p = ops.plan_conv(G3, 256, 128, 64, 64, 128, 2)
    assert p.fwd == ("gemm",) and p.dy_format is None
    assert ops._MATH[0] == 0                          # (planning in another mode leaves the current one alone)


def test_switches_are_read_at_call_time(rules):
    assert ops.plan_conv(G3, 256, 1024, 16, 16, 1024, 0).fwd[0] == "wino"
    rules.setattr(ops, "WINOGRAD", False)
    assert ops.plan_conv(G3, 256, 1024, 16, 16, 1024, 0).fwd == ("gemm",)
    rules.setattr(ops, "WINOGRAD", True)
    rules.setattr(ops, "WINOGRAD_MIN_C", 2048)
    assert ops.plan_conv(G3, 256, 1024, 16, 16, 1024, 0).fwd == ("gemm",)
    rules.setattr(ops, "WINOGRAD_MIN_C", 512)
    rules.setattr(ops, "WINOGRAD_WGRAD", False)
    p = ops.plan_conv(G3, 256, 1024, 16, 16, 1024, 0)
    assert p.fwd[0] == "wino" and p.wgrad == ("gemm",) and not p.gn_on_load


SWEEP = [(g, m, c, co, s) for g in (G3, UP, DOWN, P1) for m in (0, 1, 2)
         for c, co in itertools.product((3, 8, 32, 64, 256, 512), repeat=2) for s in (7, 8, 14, 16, 32, 64)]


@pytest.mark.parametrize("low", [False, True], ids=["default", "lowered"])
def test_dy_format_and_deferred_input_agree_across_the_sweep(rules, low):
    """For every geometry: the dy format a GroupNorm would write (DyPack.fmt, read by GroupNormFn.backward), the one
    conv2d requests and the one the planned backward families read are one value of one plan, and that value fits
    the families; a plan that normalizes a GroupNorm on load has a weight gradient that never reads x."""
    if low:
        for k, v in dict(WINOGRAD_MIN_C=1, WINOGRAD_MIN_C_WIDE=1, WINOGRAD_MIN_MACS=0.0, DYSPLIT_MIN_MACS=0.0).items():
            rules.setattr(ops, k, v)
    seen = set()
    for g, m, c, co, s in SWEEP:
        p = ops.plan_conv(g, 64, c, s, s, co, m)
        req = ops.DyPack(None, p.dy_format, p.dy_copy_ok)  # what conv2d(gn_stats=True) attaches for the GroupNorm
        assert req.fmt == p.dy_format and p.dy_format in ("packed", "split", "bias", None)
        seen.add(p.dy_format)
        if p.dy_format == "packed":    # the backward reads the packed copy on the LDS-DMA GEMMs; it never packs a second
            assert "dma" in p.dgrad and m == 1 and p.wino != "wino"
            assert p.dy_pack or p.wino == "wino_ups"
        elif p.dy_format == "split":   # both backward GEMMs (or the Winograd dy transform) take the split operand
            assert m != 2 and co % 4 == 0 and p.dgrad[0] in ("wino", "direct32", "stride2", "gemm") and "dma" not in p.dgrad
        elif p.dy_format == "bias":    # dy read in fp32 by a Winograd transform
            assert p.dgrad[0] in ("wino", "wino_ups") and p.dy_bias and not p.dy_copy_ok
        if p.dy_copy_ok:
            assert p.dy_format in ("packed", "split") and "gnbwd" not in p.dgrad
        if p.dy_pack:
            assert p.wino is None and p.dgrad[0] == "dma"
        if p.gn_on_load:
            assert p.fwd[0] == "wino" and "wino" in p.wgrad
            # with a deferred input every family ahead of the Winograd one is ruled out (_wgrad_family): none reads x
            x = torch.empty(1).expand(1, c, s, s).as_subclass(ops.DeferredGnOutput)
            lazy = ops.LazyGn(torch.zeros(1, c, s, s).contiguous(memory_format=torch.channels_last), True)
            dy = torch.zeros(1, co, s, s).contiguous(memory_format=torch.channels_last)
            dw = torch.zeros(co, c, 3, 3).contiguous(memory_format=torch.channels_last)
            if all(t.data_ptr() % 16 == 0 for t in (lazy.x, dy, dw)):
                assert ops._wgrad_family(p, x, dy, dw, None, False, None, None, lazy) == "wino"
        assert (p.chunks != ()) == (p.wino is not None)
    assert seen == {"packed", "split", "bias", None}


def test_plan_conv_needs_no_device():
    """In a process without a GPU in sight: no tensor, no device, no library call."""
    code = ("import os; os.environ['HIP_VISIBLE_DEVICES'] = ''; os.environ['CUDA_VISIBLE_DEVICES'] = ''\n"
            "import torch\n"
            "assert not torch.cuda.is_available()\n"
            "from medvae_disentangled_multimodal_amd import ops, _lib\n"
            "def no(*a, **k): raise AssertionError('library call')\n"
            "_lib.call = _lib.query = _lib.load = no\n"
            "torch.empty = torch.zeros = no\n"
            "for m in (0, 1, 2):\n"
            "    p = ops.plan_conv(ops.G3, 256, 512, 64, 64, 256, m)\n"
            "    assert p.math == m and p.fwd and p.dgrad and p.wgrad\n"
            "print('ok')\n")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
