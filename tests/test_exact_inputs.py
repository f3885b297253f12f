"""CPU self-test of tests/exact_inputs.py: the hi / lo identities of the two input families, that the float64 emulation
of the 3xBF16 value is reproduced bitwise by fp32 arithmetic in another summation order, that the precondition check
rejects a shape that is too large, and that the reporters name the wrong elements."""
import pytest
import torch
import torch.nn.functional as F

import exact_inputs as E


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_family_i_is_bf16():
    x = E.family_i((4096,), _gen(0))
    hi, lo = E.split(x)
    assert set(x.unique().tolist()) == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0}
    assert torch.equal(hi, x.double()) and not lo.any()


def test_family_l_split_identities():
    x = E.family_l((4096,), _gen(1))
    hi, lo = E.split(x)
    assert set(hi.unique().tolist()) == {-3.0, -2.0, 2.0, 3.0}
    assert set(lo.unique().tolist()) == {-2.0 ** -9, 2.0 ** -9}
    assert torch.equal((hi + lo).float(), x) and torch.equal(hi + lo, x.double())
    # signs of hi and lo are independent: all four combinations occur
    assert len(set(zip(hi.sign().tolist(), lo.sign().tolist()))) == 4


@pytest.mark.parametrize("fam", ["I", "L"])
def test_emulation_is_reproduced_by_fp32_in_another_order(fam):
    """x 4x64x16x16, w 32x64x3x3, pad 1 (and the weight gradient, K = 1024 pixels): the three 3xBF16 terms summed in
    fp32, with the channels permuted (another summation order), equal the float64 emulation bitwise."""
    g = _gen(2)
    x, w = E.family(fam, (4, 64, 16, 16), g), E.family(fam, (32, 64, 3, 3), g)
    dy = E.family(fam, (4, 32, 16, 16), g)
    fwd, dgrad, wgrad = E.conv_ops(x.shape, w.shape, 1, (1, 1, 1, 1), False)
    grid = E.grid_of(fam)
    E.check_exact(fwd(x.abs().double(), w.abs().double()), grid, "fwd")
    E.check_exact(wgrad(dy.abs().double(), x.abs().double()), grid, "wgrad")
    exp = E.emulate(fwd, x, w)
    perm = torch.randperm(64, generator=g)
    (hx, lx), (hw, lw) = E.split(x), E.split(w)
    f32 = lambda t: t.float()  # noqa: E731
    for p in (torch.arange(64), perm):
        got = sum(fwd(f32(a)[:, p], f32(b)[:, p]) for a, b in ((hx, hw), (hx, lw), (lx, hw)))
        assert got.dtype == torch.float32
        E.assert_exact(got, exp, "nchw", f"fp32 order {p[:3].tolist()}")
    expw = E.emulate(wgrad, dy, x)
    pn = torch.randperm(4, generator=g)
    (hd, ld), (hx, lx) = E.split(dy), E.split(x)
    gotw = sum(wgrad(f32(a)[pn], f32(b)[pn]) for a, b in ((hd, hx), (hd, lx), (ld, hx)))
    E.assert_exact(gotw, expw, "kcrs", "wgrad fp32")
    if fam == "L":
        full = fwd(x.double(), w.double())
        d_full = float((exp - full).abs().max())
        d_hi = float((exp - E.emulate_hi_only(fwd, x, w)).abs().max())
        assert 0 < d_full < 1e-3 < 0.1 < d_hi  # lo*lo computed too / cross terms dropped: both distinguishable
        assert torch.equal(exp * 512, (exp * 512).round())  # on the 2^-9 grid
    else:
        assert torch.equal(exp, fwd(x.double(), w.double()))


def test_precondition_rejects_large_shape():
    x = torch.full((1, 4096, 3, 3), 3.0)
    w = torch.full((1, 4096, 3, 3), 3.0)
    s = F.conv2d(x.double(), w.double())  # 9 * 4096 * 9 = 331776
    E.check_exact(s, 1.0, "I")
    with pytest.raises(AssertionError, match="shrink"):
        E.check_exact(s, 512.0, "L")
    with pytest.raises(AssertionError, match="shrink"):
        E.check_exact(s * 64, 1.0, "I")


def test_reporters_name_the_elements():
    a = torch.zeros(2, 3, 5, 5)
    b = a.clone().double()
    E.assert_exact(a, b, "nchw")
    E.assert_exact(-a, b, "nchw")  # the sign of zero does not count
    a[1, 2, 4, 0] = 1.0
    with pytest.raises(AssertionError) as ei:
        E.assert_exact(a, b, "nchw", "y", tile={"w": 4})
    msg = str(ei.value)
    assert "1 of 150" in msg and "n=1/2 last" in msg and "h=4/5 last" in msg and "w=0/5 first" in msg
    assert "got 1.0 expected 0.0" in msg
    E.assert_within(a, b, 1.0, "nchw")
    with pytest.raises(AssertionError, match="outside the bound"):
        E.assert_within(a, b, torch.full_like(b, 0.5), "nchw")
    a[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match="2 of 150"):
        E.assert_exact(a, b, "nchw")
    with pytest.raises(AssertionError, match="outside the bound"):
        E.assert_within(a, b, 10.0, "nchw")


def test_tau_and_ulp():
    assert E.tau(2304) == 3 * 2.0 ** -18 + 2304 * 2.0 ** -24
    t = torch.tensor([1.0, 1.5, 2.0, 0.75, -3.0, 0.0])
    assert E.ulp32(t).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24, 2.0 ** -22, 2.0 ** -149]


@pytest.mark.parametrize("tile,fam", [(4, "N"), (4, "L"), (2, "L")])
def test_winograd_statistic_table_is_current(tile, fam):
    """The recorded statistics behind the Winograd bounds are what wino_statistic gives today on the same shapes and
    seeds (float64 on the CPU; 1 % for the digits kept in the table); F(2x2) on family L is 0: V and U are hi + lo."""
    for shape, ups in E.WINO_BOUNDED_SHAPES:
        got = E.wino_statistic(tile, fam, shape, ups)
        if tile == 2:
            assert got == (0.0, 0.0, 0.0), (shape, ups, got)
            assert E.wino_factor(tile, fam, shape, ups) == (9.0, 9.0, 9.0)
            continue
        rec = E.WINO_MEASURED[(tile, fam, shape, ups)]
        for g, r in zip(got, rec):
            assert abs(g - r) <= 0.01 * r, (shape, ups, got, rec)
        assert E.wino_factor(tile, fam, shape, ups) == tuple(4.0 * r for r in rec)
