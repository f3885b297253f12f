"""CPU self-test of tests/gn_ref.py (no kernel is called): the float64 reference against torch's group_norm and
autograd, the dropout hash mirror, the family B preconditions, the dispatch mirror against the table of named shapes,
the fp32 emulation of the formula inside the element-wise tolerance at every element, perturbed references that the
element-wise comparison must reject, and the SiLU statistic."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_inputs as E
import gn_ref as R

G = R.GROUPS
SHAPES = R.shapes()
IDS = ["x".join(map(str, s[0])) for s in SHAPES]
NAMES = ("n", "hw", "c")


def _flat(shape):
    nb, h, w, C = shape
    return nb, h * w, C


@pytest.mark.parametrize("shape,silu,add", [((3, 7, 7, 32), False, False), ((2, 5, 3, 96), True, True),
                                            ((2, 4, 4, 160), True, False), ((4, 1, 1, 64), False, True)])
def test_reference_matches_torch_group_norm_and_autograd(shape, silu, add):
    nb, hw, C = _flat(shape)
    t = R.problem(shape, "N")
    x = t["x"].double().view(nb, shape[1], shape[2], C).permute(0, 3, 1, 2).requires_grad_()
    gm, bt = t["gamma"].double().requires_grad_(), t["beta"].double().requires_grad_()
    y = F.group_norm(x, G, gm, bt, eps=R.EPS)
    if silu:
        y = y * torch.sigmoid(y)
    dy = t["dy"].double().view(nb, shape[1], shape[2], C).permute(0, 3, 1, 2)
    (y * dy).sum().backward()
    ref = R.forward(t["x"], t["gamma"], t["beta"], G, silu=silu)
    rb = R.backward(t["x"], t["dy"], t["gamma"], t["beta"], G, ref["mean"], ref["rstd"], silu=silu,
                    add=t["add"] if add else None)
    nhwc = lambda v: v.permute(0, 2, 3, 1).reshape(nb, hw, C)  # noqa: E731
    E.assert_within(ref["y"], nhwc(y), 1e-13 * (1 + nhwc(y).abs()), NAMES, "y")
    exp = nhwc(x.grad) + (t["add"].double() if add else 0.0)
    E.assert_within(rb["dx"], exp, 1e-11 * (1 + exp.abs()), NAMES, "dx")
    E.assert_within(rb["dgamma"], gm.grad, 1e-11 * (1 + gm.grad.abs()), "c", "dgamma")
    E.assert_within(rb["dbeta"], bt.grad, 1e-11 * (1 + bt.grad.abs()), "c", "dbeta")
    E.assert_within(rb["colsum"], exp.sum((0, 1)), 1e-10 * (1 + exp.abs().sum((0, 1))), "c", "colsum")


def test_hash_mirror_is_deterministic_keeps_one_minus_p_and_depends_on_salt():
    seed, salt, p, n = 77, 0x1234567890ABCDEF, 0.1, 2 ** 20
    a = R.keep_mask(seed, salt, p, 1, n // 64, 64)
    assert torch.equal(a, R.keep_mask(seed, salt, p, 1, n // 64, 64))
    pf = float(np.float32(p))
    sigma = (pf * (1 - pf) / n) ** 0.5
    assert abs(float(a.double().mean()) - (1 - pf)) < 4 * sigma
    b = R.keep_mask(seed, salt + 1, p, 1, n // 64, 64)
    assert 0.1 < float((a != b).double().mean()) < 0.3  # two independent masks differ in 2 p (1 - p) = 0.18
    assert not torch.equal(a, R.keep_mask(seed + 1, salt, p, 1, n // 64, 64))
    assert torch.equal(R.keep_mask(seed, None, p, 1, 64, 64), R.keep_mask(seed, 0, p, 1, 64, 64))  # salt 0 = no salt
    # the global element offset: sample 1 continues sample 0's counter
    two = R.keep_mask(seed, salt, p, 2, 32, 64)
    assert torch.equal(two.view(1, 64, 64), R.keep_mask(seed, salt, p, 1, 64, 64))
    # one value by hand (splitmix64 finalizer of seed + golden * (idx + 1))
    z = (5 + 0x9E3779B97F4A7C15 * 4) % 2 ** 64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    z ^= z >> 31
    assert float(R.hash_uniform(5, np.array([3], dtype=np.uint64))[0]) == (z >> 40) / 2.0 ** 24


@pytest.mark.parametrize("shape", [s[0] for s in SHAPES], ids=IDS)
def test_family_b_preconditions(shape):
    nb, hw, C = _flat(shape)
    x = R.problem(shape, "B")["x"]
    R.check_family_b(x, G)
    ks = torch.log2(x.abs().view(nb, hw, G, C // G).amax((1, 3)))
    if nb * G >= 64:
        assert set(ks.flatten().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    with pytest.raises(AssertionError):
        bad = x.clone()
        bad[0, 0, 0] = -bad[0, 0, 0] if float(bad[0, 0, 0]) != 0 else 1.0
        R.check_family_b(bad, G)


def test_mirror_gives_the_table():
    for shape, fwd, bwd in SHAPES:
        nb, hw, C = _flat(shape)
        assert R.fwd_slab(hw, C, G) == fwd, shape
        assert R.bwd_slab(nb, hw, C, G) == bwd, shape
    assert R.bwd_slab(600, 900, 32, 32) == (0, 0) and R.bwd_slab(500, 900, 32, 32) == (16, 8)  # the 64 MB rule
    assert R.resident_slab(64, 1056, 32, 16) == (0, 0)  # 66 channels are no whole number of quads
    nb = R.unit_walk_nb(256)
    assert nb == 3073 and nb * 49 * 32 <= 4.82e6


def _emulation_cases(shape, fwd, bwd):
    yield "streaming", (0, 0), (0, 0)
    if fwd[0]:
        yield "resident", fwd, bwd


@pytest.mark.parametrize("fam", ["B", "S", "N"])
@pytest.mark.parametrize("shape,fwd,bwd", SHAPES, ids=IDS)
def test_fp32_emulation_is_inside_the_tolerance_at_every_element(shape, fwd, bwd, fam):
    """(this emulation is not the kernel; no element is excluded)"""
    nb, hw, C = _flat(shape)
    cpg = C // G
    t = R.problem(shape, fam)
    x, gm, bt, dy, add = (t[k] for k in ("x", "gamma", "beta", "dy", "add"))
    ref = R.forward(x, gm, bt, G)
    for what, fs, bs in _emulation_cases(shape, fwd, bwd):
        emu = R.emulate_forward(x, gm, bt, G, fs)
        tol = R.fwd_tol(x, gm, bt, G, ref, R.resident_depth(*fs, cpg))
        for k in ("mean", "rstd"):
            E.assert_within(emu[k], ref[k], tol[k], ("n", "g"), f"{what} {k}")
        E.assert_within(emu["y"], ref["y"], tol["y"], NAMES, f"{what} y", tile={"c": cpg})
        rb = R.backward(x, dy, gm, bt, G, emu["mean"], emu["rstd"], add=add)
        eb = R.emulate_backward(x, dy, gm, bt, G, emu["mean"], emu["rstd"], bs, add=add)
        tb = R.bwd_tol(x, gm, G, rb, R.resident_depth(*bs, cpg))
        E.assert_within(eb["dx"], rb["dx"], tb["dx"], NAMES, f"{what} dx", tile={"c": cpg})
        E.assert_within(eb["dgamma"], rb["dgamma"] + 0.5, tb["dgamma"], "c", f"{what} dgamma")
        E.assert_within(eb["dbeta"], rb["dbeta"] - 0.25, tb["dbeta"], "c", f"{what} dbeta")
    if fam == "B":  # exact: the emulation's mean is 0 and y is fl(x sc + beta) whatever the summation order
        assert not emu["mean"].any()


def _rejected(got, ref, tol, what):
    """the element-wise comparison fails; returns the number of differing elements it reports"""
    with pytest.raises(AssertionError) as e:
        E.assert_within(got, ref, tol, NAMES, what)
    return int(re.search(r"(\d+) of \d+ elements wrong", str(e.value)).group(1))


# measured (elements outside the bound / elements), family N: see test_perturbed_references_are_rejected
@pytest.mark.parametrize("shape,fwd,bwd", SHAPES[:-1], ids=IDS[:-1])
def test_perturbed_references_are_rejected(shape, fwd, bwd):
    """Each perturbation of the float64 reference must fail the element-wise comparison against the unperturbed one,
    under the widest tolerance the shape is ever given (the resident depth where the shape has one)."""
    nb, hw, C = _flat(shape)
    cpg = C // G
    t = R.problem(shape, "N")
    x, gm, bt = t["x"], t["gamma"], t["beta"]
    ref = R.forward(x, gm, bt, G)
    tol = R.fwd_tol(x, gm, bt, G, ref, R.resident_depth(*fwd, cpg))["y"]
    counts = {}
    # gamma read one channel late in the last slab
    sc = fwd[0] or min(C, 1024)
    g2 = gm.clone()
    g2[C - sc:C - 1] = gm[C - sc + 1:]
    counts["gamma"] = _rejected(R.forward(x, g2, bt, G)["y"], ref["y"], tol, "gamma one channel late")
    # the last group's mean taken from the group before it
    xg = x.double().view(nb, hw, G, cpg)
    mu = ref["mean"].clone()
    mu[:, -1] = mu[:, -2]
    y2 = (((xg - mu.view(nb, 1, G, 1)) * ref["rstd"].view(nb, 1, G, 1)).reshape(nb, hw, C) * gm.double() + bt.double())
    counts["mean"] = _rejected(y2, ref["y"], tol, "last group's mean from the group before")
    # the last hw mod rpar rows left un-normalised
    rpar = R.NT // (fwd[0] // 4) if fwd[0] else R.streaming_rpar(C)
    tail = hw % rpar
    if tail:
        y3 = ref["y"].clone()
        y3[:, hw - tail:] = x[:, hw - tail:].double()
        counts["tail"] = _rejected(y3, ref["y"], tol, "tail rows un-normalised")
        assert counts["tail"] > 0.9 * nb * tail * C
    # the mask computed with the per-sample offset instead of the global offset
    good, bad = R.keep_mask(77, 5, 0.5, nb, hw, C), R.keep_mask(77, 5, 0.5, nb, hw, C, per_sample=True)
    yd = R.forward(x, gm, bt, G, mask=good, p=0.5)["y"]
    counts["mask"] = _rejected(R.forward(x, gm, bt, G, mask=bad, p=0.5)["y"], yd, 2 * tol, "per-sample mask offset")
    assert torch.equal(good[0], bad[0]) and counts["mask"] > 0.4 * (nb - 1) * hw * C
    assert counts["gamma"] > 0.9 * nb * hw * (sc - 1) and counts["mean"] > 0.9 * nb * hw * cpg
    print("perturbed", shape, counts)


@pytest.mark.parametrize("fam", ["S", "N"])
@pytest.mark.parametrize("shape", [s[0] for s in SHAPES], ids=IDS)
def test_silu_statistic_is_the_recorded_one(shape, fam):
    key = R.silu_key(fam, shape)
    sf, sb = R.silu_statistic(fam, shape)
    print("silu statistic", key, f"({sf / R.U:.4g}, {sb / R.U:.4g}),")
    rf, rb = R.SILU_MEASURED.get(key, (0.0, 0.0))
    assert abs(sf / R.U - rf) <= 1e-3 * rf and abs(sb / R.U - rb) <= 1e-3 * rb
