"""Element-wise GroupNorm tests through the C ABI on every dispatch path (tests/gn_ref.py: dispatch mirror, float64
reference, hash mirror, input families, tolerance and its derivation). Every shape of gn_ref.TABLE runs on path 0 (auto:
the resident kernels where the mirror says so) and path 1 (streaming); the path a shape takes is asserted against
mvae_group_norm_bwd_streaming before anything is compared. No element is excluded from a comparison.

The backward is compared with the float64 closed form evaluated at the mean / rstd the kernel's forward returned (its
saved inputs); those are themselves compared with the float64 statistics.

SiLU cases: the bound is four times the CPU statistic of the shape (gn_ref.SILU_MEASURED, in units of 2^-24, (forward,
backward); family S with the residual add, family N without):
  3x7x7x32 S (1.451, 0.4384) N (1.734, 2.287)      2x20x20x32 S (1.54, 0.2355) N (1.931, 3.027)
  2x28x28x32 S (1.526, 0.1378) N (1.877, 3.063)    2x30x30x32 S (1.793, 0.1346) N (1.939, 3.203)
  2x7x7x256 S (1.741, 0.8569) N (1.921, 2.718)     2x7x7x512 S (1.8, 0.8816) N (1.83, 3.279)
  2x7x7x1024 S (1.732, 0.8388) N (2.007, 3.11)     2x4x4x2048 S (1.742, 2.049) N (1.866, 3.38)
  4x1x1x64 S (1.177, 5.725) N (1.073, 3.441)       5x9x9x96 S (1.68, 0.2673) N (1.908, 2.935)
  2x8x8x160 S (1.494, 0.7649) N (1.713, 2.914)     2x8x8x1056 S (1.855, 0.8158) N (1.98, 3.897)
  3073x7x7x32 S (1.867, 0.7597) N (2.279, 3.748)"""
import contextlib
import functools

import pytest
import torch

import exact_inputs as E
import gn_ref as R

pytestmark = pytest.mark.gpu

G = R.GROUPS
NAMES = ("n", "hw", "c")
ROWS = list(range(len(R.TABLE)))
ROW_IDS = ["x".join("walk" if v is None else str(v) for v in s) for s, _, _ in R.TABLE]
PATHS = [0, 1]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def table(dev):
    return R.shapes(torch.cuda.get_device_properties(dev).multi_processor_count)


@contextlib.contextmanager
def gn_path(path):
    from medvae_disentangled_multimodal_amd import _lib
    _lib.call("mvae_set_group_norm_path", path)
    try:
        yield
    finally:
        _lib.call("mvae_set_group_norm_path", 0)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws(nb, hw, C, dev):
    from medvae_disentangled_multimodal_amd import _lib
    return torch.empty(_lib.query("mvae_group_norm_workspace_bytes", nb, hw, C), dtype=torch.uint8, device=dev)


@functools.lru_cache(maxsize=2)
def _problem(shape, fam):
    return R.problem(shape, fam)


@functools.lru_cache(maxsize=2)
def _fwd_ref(shape, fam, silu):
    t = _problem(shape, fam)
    return R.forward(t["x"], t["gamma"], t["beta"], G, silu=silu)


def _to(t, dev, keys=("x", "gamma", "beta", "dy", "add")):
    return {k: t[k].to(dev) for k in keys}


def _fwd(d, shape, silu=False, drop=0.0, seed=0, y_split=0):
    """forward on the current path: (y as a byte buffer of the format's size, mean, rstd), on the device"""
    from medvae_disentangled_multimodal_amd import _lib
    nb, hw, C = shape[0], shape[1] * shape[2], shape[3]
    dev = d["x"].device
    ws = _ws(nb, hw, C, dev)
    y = torch.empty(nb * hw * C * (2 if y_split == 2 else 4), dtype=torch.uint8, device=dev)
    mean = torch.empty(nb * G, device=dev)
    rstd = torch.empty_like(mean)
    _lib.call("mvae_group_norm_fwd_nhwc", d["x"].data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr(),
              y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), nb, hw, C, G, 1e-6, int(silu), float(drop), seed,
              y_split, ws.data_ptr(), ws.numel(), _stream())
    torch.cuda.synchronize()
    return y, mean, rstd


def _bwd(d, shape, mean, rstd, silu=False, drop=0.0, seed=0, add=False, init_dg=0.5, init_db=-0.25):
    from medvae_disentangled_multimodal_amd import _lib
    nb, hw, C = shape[0], shape[1] * shape[2], shape[3]
    dev = d["x"].device
    ws = _ws(nb, hw, C, dev)
    dx = torch.empty_like(d["x"])
    dg = torch.full((C,), init_dg, device=dev)  # accumulated into (+=)
    db = torch.full((C,), init_db, device=dev)
    _lib.call("mvae_group_norm_bwd_nhwc", d["x"].data_ptr(), d["dy"].data_ptr(), d["gamma"].data_ptr(),
              d["beta"].data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), _ptr(d["add"] if add else None),
              dg.data_ptr(), db.data_ptr(), nb, hw, C, G, int(silu), float(drop), seed, ws.data_ptr(), ws.numel(),
              _stream())
    torch.cuda.synchronize()
    return dx, dg, db


def _f32(buf, shape):
    return buf.view(torch.float32).view(shape[0], shape[1] * shape[2], shape[3]).cpu()


def _assert_path(shape, bwd):
    """(path 0 is selected) the library's backward takes the path the mirror says"""
    from medvae_disentangled_multimodal_amd import _lib
    nb, hw, C = shape[0], shape[1] * shape[2], shape[3]
    assert R.bwd_slab(nb, hw, C, G) == bwd
    assert _lib.query("mvae_group_norm_bwd_streaming", nb, hw, C, G, 0) == int(bwd[0] == 0), (shape, bwd)


def _depths(shape, fwd, bwd, path):
    cpg = shape[3] // G
    return (0, 0) if path == 1 else (R.resident_depth(*fwd, cpg), R.resident_depth(*bwd, cpg))


def _ratio(got, ref, tol):
    return float(((got.detach().cpu().double() - ref.double()).abs() / tol).max())


def test_mirror_matches_the_library_over_a_sweep(dev, table):
    """The table's paths, and ~260 further geometries, against mvae_group_norm_bwd_streaming (no kernel launch): the
    backward's answer validates the slab rule the forward shares."""
    from medvae_disentangled_multimodal_amd import _lib
    _lib.call("mvae_set_group_norm_path", 0)
    for shape, fwd, bwd in table:
        nb, hw, C = shape[0], shape[1] * shape[2], shape[3]
        assert R.fwd_slab(hw, C, G) == fwd, shape
        _assert_path(shape, bwd)
    n = 0
    for hw in (1, 16, 49, 64, 81, 196, 400, 784, 900, 1024, 4096):
        for C in (16, 32, 64, 96, 128, 160, 256, 512, 1024, 1056, 2048, 4096):
            for g in (min(32, C), 8):
                for nb in (2, 600):
                    exp = int(R.bwd_slab(nb, hw, C, g)[0] == 0)
                    assert _lib.query("mvae_group_norm_bwd_streaming", nb, hw, C, g, 0) == exp, (nb, hw, C, g)
                    n += 1
    assert n >= 200
    with gn_path(1):
        assert _lib.query("mvae_group_norm_bwd_streaming", 3, 49, 32, 32, 0) == 1


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("path", PATHS)
def test_family_b_is_exact(dev, table, row, path):
    """Balanced +-2^k inputs: mean bitwise 0, rstd within 1 ulp of the float64 value (printed: whether bitwise), y in all
    four output formats bitwise fl(x * fl(rstd_out * gamma) + beta), and dbeta of integer dy the exact integer sum."""
    shape, fwd, bwd = table[row]
    nb, hw, C = shape[0], shape[1] * shape[2], shape[3]
    _assert_path(shape, bwd)
    t = _problem(shape, "B")
    R.check_family_b(t["x"], G)
    d = _to(t, dev)
    with gn_path(path):
        y, mean, rstd = _fwd(d, shape)
        assert not bool(mean.view(torch.int32).any()), "mean is not bitwise 0"
        var = (t["x"].double() ** 2).view(nb, hw, G, C // G).mean((1, 3))
        exp_rs = (1.0 / torch.sqrt(var + R.EPS)).float().reshape(-1)
        ulps = ((rstd.cpu().double() - exp_rs.double()).abs() / R.ulp32(exp_rs)).max()
        print(f"rstd {shape} path {path}: bitwise {torch.equal(rstd.cpu(), exp_rs)}, worst {float(ulps):.0f} ulp")
        assert float(ulps) <= 1
        sc = (rstd.cpu().double().view(nb, 1, G, 1) * t["gamma"].double().view(1, 1, G, C // G)).float()
        exp = (t["x"].double() * sc.double().reshape(nb, 1, C) + t["beta"].double()).float()
        E.assert_exact(_f32(y, shape), exp, NAMES, "y", tile={"c": fwd[0] or C})
        hi = exp.bfloat16().float()
        lo = (exp - hi).bfloat16().float()
        bf = lambda b: b.view(torch.bfloat16).float().cpu()  # noqa: E731
        y1 = bf(_fwd(d, shape, y_split=1)[0]).view(-1, 8)  # split4_bf16 groups: 4 hi then 4 lo per 4 elements
        E.assert_exact(y1[:, :4].reshape(nb, hw, C), hi, NAMES, "y_split 1 hi")
        E.assert_exact(y1[:, 4:].reshape(nb, hw, C), lo, NAMES, "y_split 1 lo")
        E.assert_exact(bf(_fwd(d, shape, y_split=2)[0]).view(nb, hw, C), hi, NAMES, "y_split 2")
        y3 = bf(_fwd(d, shape, y_split=3)[0]).view(2, nb, hw, C)  # hi plane, then lo plane
        E.assert_exact(y3[0], hi, NAMES, "y_split 3 hi")
        E.assert_exact(y3[1], lo, NAMES, "y_split 3 lo")
        E.check_exact(t["dy"].abs().double().sum((0, 1)) + 3, 1.0, "dbeta")
        _, _, db = _bwd(d, shape, mean, rstd, init_db=3.0)
        E.assert_exact(db, 3.0 + t["dy"].double().sum((0, 1)), "c", "dbeta")


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("path", PATHS)
def test_dropout_mask_is_the_hash_of_seed_salt_and_global_offset(dev, table, row, p, path):
    """Family B: the zero pattern is the mirror's mask, kept elements are within 1 ulp of fl(y0 / fl(1 - p)). Family N:
    the backward's recomputed mask against the float64 closed form with the mirror's mask (K + 2: fl(1 - p) and the
    division)."""
    import numpy as np
    from medvae_disentangled_multimodal_amd import ops
    shape, fwd, bwd = table[row]
    nb, hw, C = shape[0], shape[1] * shape[2], shape[3]
    salt = int(ops.dropout_salt(dev).item())  # (the process-wide tensor: never one the test owns)
    seed = 1234 + row
    keep = R.keep_mask(seed, salt, p, nb, hw, C)
    t = _problem(shape, "B")
    d = _to(t, dev)
    with gn_path(path):
        y0 = _f32(_fwd(d, shape)[0], shape)
        y = _f32(_fwd(d, shape, drop=p, seed=seed)[0], shape)
    assert bool((y0 != 0).all())
    E.assert_exact((y != 0).double(), keep.double(), NAMES, "kept pattern")
    exp = torch.where(keep, (y0.double() / float(np.float32(1) - np.float32(p))).float(), torch.zeros_like(y0))
    E.assert_within(y, exp, R.ulp32(exp), NAMES, "kept values")
    # backward, family N, no SiLU
    t = _problem(shape, "N")
    d = _to(t, dev)
    _, db_depth = _depths(shape, fwd, bwd, path)
    with gn_path(path):
        _, mean, rstd = _fwd(d, shape, drop=p, seed=seed)
        dx, dg, db = _bwd(d, shape, mean, rstd, drop=p, seed=seed, add=True)
    rb = R.backward(t["x"], t["dy"], t["gamma"], t["beta"], G, mean.cpu().view(nb, G), rstd.cpu().view(nb, G),
                    add=t["add"], mask=keep, p=p)
    tb = R.bwd_tol(t["x"], t["gamma"], G, rb, db_depth, ku=(R.K_BWD + 2) * R.U)
    tb["dgamma"], tb["dbeta"] = tb["dgamma"] + 2 * R.U * tb["basis_dgamma"], tb["dbeta"] + 2 * R.U * tb["basis_dbeta"]
    E.assert_within(dx.cpu().view(nb, hw, C), rb["dx"], tb["dx"], NAMES, "dx", tile={"c": bwd[0] or C})
    E.assert_within(dg.cpu(), rb["dgamma"] + 0.5, tb["dgamma"], "c", "dgamma")
    E.assert_within(db.cpu(), rb["dbeta"] - 0.25, tb["dbeta"], "c", "dbeta")


def test_advancing_the_salt_draws_the_mirrors_new_mask(dev, table):
    from medvae_disentangled_multimodal_amd import ops
    shape = table[4][0]
    nb, hw, C = shape[0], shape[1] * shape[2], shape[3]
    d = _to(_problem(shape, "B"), dev)
    salt_t = ops.dropout_salt(dev)
    salt = int(salt_t.item())
    try:
        a = _f32(_fwd(d, shape, drop=0.5, seed=9)[0], shape) != 0
        salt_t += 1
        torch.cuda.synchronize()
        b = _f32(_fwd(d, shape, drop=0.5, seed=9)[0], shape) != 0
    finally:
        salt_t.fill_(salt)
        torch.cuda.synchronize()
    assert torch.equal(a, R.keep_mask(9, salt, 0.5, nb, hw, C))
    assert torch.equal(b, R.keep_mask(9, salt + 1, 0.5, nb, hw, C)) and not torch.equal(a, b)


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("fam,silu,add", [("S", False, False), ("S", True, True), ("N", False, True),
                                          ("N", True, False)])
@pytest.mark.parametrize("path", PATHS)
def test_every_output_is_within_the_elementwise_bound(dev, table, row, fam, silu, add, path):
    """mean, rstd, y, dx, dgamma, dbeta against float64, each element within tol_i: streaming at depth 0, resident with
    its summation term (gn_ref's docstring); the worst |err| / tol_i of each output is printed."""
    shape, fwd, bwd = table[row]
    nb, hw, C = shape[0], shape[1] * shape[2], shape[3]
    _assert_path(shape, bwd)
    t = _problem(shape, fam)
    d = _to(t, dev)
    ref = _fwd_ref(shape, fam, silu)
    with gn_path(path):
        y, mean, rstd = _fwd(d, shape, silu=silu)
        dx, dg, db = _bwd(d, shape, mean, rstd, silu=silu, add=add)
    df, dbk = _depths(shape, fwd, bwd, path)
    kf, kb = R.silu_ku(fam, shape) if silu else (R.K_FWD * R.U, R.K_BWD * R.U)
    tol = R.fwd_tol(t["x"], t["gamma"], t["beta"], G, ref, df, kf, silu=silu)
    mean, rstd = mean.cpu().view(nb, G), rstd.cpu().view(nb, G)
    rb = R.backward(t["x"], t["dy"], t["gamma"], t["beta"], G, mean, rstd, silu=silu, add=t["add"] if add else None)
    tb = R.bwd_tol(t["x"], t["gamma"], G, rb, dbk, kb, silu=silu)
    got = dict(mean=(mean, ref["mean"], tol["mean"]), rstd=(rstd, ref["rstd"], tol["rstd"]),
               y=(_f32(y, shape), ref["y"], tol["y"]), dx=(dx.cpu().view(nb, hw, C), rb["dx"], tb["dx"]),
               dgamma=(dg.cpu(), rb["dgamma"] + 0.5, tb["dgamma"]), dbeta=(db.cpu(), rb["dbeta"] - 0.25, tb["dbeta"]))
    print(f"ratio {shape} {fam} silu {int(silu)} add {int(add)} path {path} fwd {fwd} bwd {bwd}: " +
          " ".join(f"{k} {_ratio(*v):.3f}" for k, v in got.items()))
    for k, (g, r, b) in got.items():
        names = NAMES if g.dim() == 3 else (("n", "g") if g.dim() == 2 else "c")
        E.assert_within(g, r, b, names, k, tile={"c": (bwd[0] if k == "dx" else fwd[0]) or C} if g.dim() == 3 else None)


@pytest.mark.parametrize("row", [4, len(R.TABLE) - 1], ids=[ROW_IDS[4], ROW_IDS[-1]])
@pytest.mark.parametrize("path", PATHS)
def test_pack_split_and_colsum_forms(dev, table, row, path):
    """dx / dgamma / dbeta of the pack, split and colsum forms bitwise the plain backward's, the second copy bitwise
    mvae_pack_bf16 / mvae_split_bf16 of dx, and every bias column sum against the float64 reference's."""
    from medvae_disentangled_multimodal_amd._lib import call, query
    shape, fwd, bwd = table[row]
    nb, hw, C = shape[0], shape[1] * shape[2], shape[3]
    t = _problem(shape, "N")
    d = _to(t, dev)
    gen = torch.Generator().manual_seed(row)
    bias0 = torch.randn(C, generator=gen)
    st = _stream()
    with gn_path(path):
        _, mean, rstd = _fwd(d, shape)
        dx0, dg0, db0 = _bwd(d, shape, mean, rstd, add=True)
        rb = R.backward(t["x"], t["dy"], t["gamma"], t["beta"], G, mean.cpu().view(nb, G), rstd.cpu().view(nb, G),
                        add=t["add"])
        tb = R.bwd_tol(t["x"], t["gamma"], G, rb, _depths(shape, fwd, bwd, path)[1])
        ws = _ws(nb, hw, C, dev)
        cs = torch.empty(query("mvae_group_norm_colsum_workspace_bytes", nb, hw, C), dtype=torch.uint8, device=dev)
        for fmt in ("pack", "split", "colsum"):
            dx1 = torch.empty_like(dx0)
            dg1, db1 = torch.full((C,), 0.5, device=dev), torch.full((C,), -0.25, device=dev)
            bias = bias0.to(dev)
            head = (d["x"].data_ptr(), d["dy"].data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr(),
                    mean.data_ptr(), rstd.data_ptr(), dx1.data_ptr(), d["add"].data_ptr(), dg1.data_ptr(),
                    db1.data_ptr(), nb, hw, C, G, 0, 0.0, 0, ws.data_ptr(), ws.numel())
            if fmt == "colsum":
                call("mvae_group_norm_bwd_colsum_nhwc", *head, bias.data_ptr(), 1.0, cs.data_ptr(), cs.numel(), st)
            else:
                cp = torch.empty(dx0.numel() * (4 if fmt == "split" else 2), dtype=torch.uint8, device=dev)
                call(f"mvae_group_norm_bwd_{fmt}_nhwc", *head, cp.data_ptr(), bias.data_ptr(), 1.0, cs.data_ptr(),
                     cs.numel(), st)
                exp = torch.empty_like(cp)
                call("mvae_split_bf16" if fmt == "split" else "mvae_pack_bf16", dx0.data_ptr(), exp.data_ptr(),
                     dx0.numel(), st)
            torch.cuda.synchronize()
            assert torch.equal(dx1, dx0) and torch.equal(dg1, dg0) and torch.equal(db1, db0), fmt
            if fmt != "colsum":
                assert torch.equal(cp, exp), fmt
            E.assert_within(bias.cpu(), bias0.double() + rb["colsum"], tb["colsum"](bias0), "c", f"{fmt} bias sums")


@pytest.mark.parametrize("shape", R.PART_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_part_forms_from_host_built_partials(dev, shape):
    """The forms fed by a conv epilogue, with `part` built on the host from the float64 reference in the documented
    layouts (no conv): every output within tol_i at depth 0; mvae_group_norm_stats_nhwc without part within 1 ulp of
    the with-part result."""
    from medvae_disentangled_multimodal_amd._lib import call, query
    nb, hw, C = shape[0], shape[1] * shape[2], shape[3]
    cpg = C // G
    t = R.problem(shape, "N")
    d = _to(t, dev)
    st = _stream()
    ref = R.forward(t["x"], t["gamma"], t["beta"], G)
    tol = R.fwd_tol(t["x"], t["gamma"], t["beta"], G, ref, 0)
    part = R.fwd_part(t["x"]).to(dev)
    ws = _ws(nb, hw, C, dev)
    new = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
    y, mean, rstd = new(nb, hw, C), new(nb * G), new(nb * G)
    call("mvae_group_norm_fwd_part_nhwc", d["x"].data_ptr(), part.data_ptr(), d["gamma"].data_ptr(),
         d["beta"].data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), nb, hw, C, G, 1e-6, 0, 0.0, 0, 0,
         ws.data_ptr(), ws.numel(), st)
    out = {}
    for with_part in (True, False):
        m2, r2, scale, shift = new(nb * G), new(nb * G), new(nb, C), new(nb, C)
        call("mvae_group_norm_stats_nhwc", d["x"].data_ptr(), part.data_ptr() if with_part else None,
             d["gamma"].data_ptr(), d["beta"].data_ptr(), m2.data_ptr(), r2.data_ptr(), scale.data_ptr(),
             shift.data_ptr(), nb, hw, C, G, 1e-6, ws.data_ptr(), ws.numel(), st)
        torch.cuda.synchronize()
        out[with_part] = [v.cpu() for v in (m2, r2, scale, shift)]
    y2 = new(nb, hw, C)
    call("mvae_group_norm_apply_nhwc", d["x"].data_ptr(), scale.data_ptr(), shift.data_ptr(), y2.data_ptr(), nb, hw, C,
         0, 0, st)
    torch.cuda.synchronize()
    sc_ref = (ref["rstd"].view(nb, G, 1) * t["gamma"].double().view(1, G, cpg)).reshape(nb, C)
    sh_ref = t["beta"].double() - (ref["mean"].view(nb, G, 1) * sc_ref.view(nb, G, cpg)).reshape(nb, C)
    m2, r2, scale_c, shift_c = out[True]
    for name, got, r, b, names in (
            ("mean", mean.cpu().view(nb, G), ref["mean"], tol["mean"], ("n", "g")),
            ("rstd", rstd.cpu().view(nb, G), ref["rstd"], tol["rstd"], ("n", "g")),
            ("y", y.cpu(), ref["y"], tol["y"], NAMES),
            ("stats mean", m2.view(nb, G), ref["mean"], tol["mean"], ("n", "g")),
            ("stats rstd", r2.view(nb, G), ref["rstd"], tol["rstd"], ("n", "g")),
            ("scale", scale_c, sc_ref, tol["scale"], ("n", "c")), ("shift", shift_c, sh_ref, tol["shift"], ("n", "c")),
            ("apply y", y2.cpu(), ref["y"], tol["y"], NAMES)):
        print(f"part ratio {shape} {name} {_ratio(got, r, b):.3f}")
        E.assert_within(got, r, b, names, name, tile={"c": cpg})
    for name, a, b in zip(("mean", "rstd", "scale", "shift"), out[False], out[True]):
        E.assert_within(a, b, R.ulp32(b), None, f"stats without part: {name}")
    # backward from host-built {sum dyn, sum dyn xhat} partials, at the saved statistics of the forward above
    rb = R.backward(t["x"], t["dy"], t["gamma"], t["beta"], G, mean.cpu().view(nb, G), rstd.cpu().view(nb, G),
                    add=t["add"])
    tb = R.bwd_tol(t["x"], t["gamma"], G, rb, 0)
    bpart = R.bwd_part(rb["dyn"], rb["xh"]).to(dev)
    gen = torch.Generator().manual_seed(C)
    bias0 = torch.randn(C, generator=gen)
    cs = torch.empty(query("mvae_group_norm_colsum_workspace_bytes", nb, hw, C), dtype=torch.uint8, device=dev)
    for split in (False, True):
        dx = new(nb, hw, C)
        dg, db = torch.full((C,), 0.5, device=dev), torch.full((C,), -0.25, device=dev)
        head = (d["x"].data_ptr(), d["dy"].data_ptr(), bpart.data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr(),
                mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), d["add"].data_ptr(), dg.data_ptr(), db.data_ptr(), nb,
                hw, C, G, 0, ws.data_ptr(), ws.numel())
        if split:
            bias = bias0.to(dev)
            cp = torch.empty(dx.numel() * 4, dtype=torch.uint8, device=dev)
            call("mvae_group_norm_bwd_part_split_nhwc", *head, cp.data_ptr(), bias.data_ptr(), 1.0, cs.data_ptr(),
                 cs.numel(), st)
        else:
            call("mvae_group_norm_bwd_part_nhwc", *head, st)
        torch.cuda.synchronize()
        for name, got, r, b, names in (("dx", dx.cpu(), rb["dx"], tb["dx"], NAMES),
                                       ("dgamma", dg.cpu(), rb["dgamma"] + 0.5, tb["dgamma"], "c"),
                                       ("dbeta", db.cpu(), rb["dbeta"] - 0.25, tb["dbeta"], "c")):
            print(f"part ratio {shape} split {int(split)} {name} {_ratio(got, r, b):.3f}")
            E.assert_within(got, r, b, names, f"bwd_part split {int(split)} {name}", tile={"c": cpg})
        if split:
            E.assert_within(bias.cpu(), bias0.double() + rb["colsum"], tb["colsum"](bias0), "c", "dbias")
            q = cp.view(torch.bfloat16).float().cpu().view(-1, 8)
            hi = dx.cpu().bfloat16().float()
            E.assert_exact(q[:, :4].reshape(nb, hw, C), hi, NAMES, "dx_split hi")
            E.assert_exact(q[:, 4:].reshape(nb, hw, C), (dx.cpu() - hi).bfloat16().float(), NAMES, "dx_split lo")


SENTINEL = -7.5


def test_rejected_calls_raise_and_write_nothing(dev):
    from medvae_disentangled_multimodal_amd._lib import call, query
    st = _stream()
    full = lambda *s: torch.full(s, SENTINEL, device=dev)  # noqa: E731

    def case(nb, hw, C, g, part_forms, short_ws=False):
        n = nb * hw * C
        x, dy, gm, bt = (torch.randn(k, device=dev) for k in (n, n, C, C))
        part = torch.zeros(2 * n + 64, dtype=torch.float64, device=dev)
        ws = torch.empty(query("mvae_group_norm_workspace_bytes", nb, hw, C) + 64, dtype=torch.uint8, device=dev)
        wsn = query("mvae_group_norm_workspace_bytes", nb, hw, C) - 1 if short_ws else ws.numel()
        cs = torch.empty(query("mvae_group_norm_colsum_workspace_bytes", nb, hw, C) + 64, dtype=torch.uint8, device=dev)
        ng = nb * max(g, 1)
        outs = dict(y=full(n), mean=full(ng), rstd=full(ng), scale=full(nb * C), shift=full(nb * C), dx=full(n),
                    dg=full(C), db=full(C), cp=full(n), bias=full(C))
        o = {k: v.data_ptr() for k, v in outs.items()}
        xs, ds, gs, bs, ps = x.data_ptr(), dy.data_ptr(), gm.data_ptr(), bt.data_ptr(), part.data_ptr()
        calls = [("mvae_group_norm_fwd_part_nhwc", (xs, ps, gs, bs, o["y"], o["mean"], o["rstd"], nb, hw, C, g, 1e-6, 1,
                                                    0.0, 0, 0, ws.data_ptr(), wsn, st)),
                 ("mvae_group_norm_bwd_part_nhwc", (xs, ds, ps, gs, bs, o["mean"], o["rstd"], o["dx"], None, o["dg"],
                                                    o["db"], nb, hw, C, g, 1, ws.data_ptr(), wsn, st)),
                 ("mvae_group_norm_bwd_part_split_nhwc", (xs, ds, ps, gs, bs, o["mean"], o["rstd"], o["dx"], None,
                                                          o["dg"], o["db"], nb, hw, C, g, 1, ws.data_ptr(), wsn,
                                                          o["cp"], o["bias"], 1.0, cs.data_ptr(), cs.numel(), st))]
        if not short_ws:  # (with part, the statistics form needs no workspace)
            calls.append(("mvae_group_norm_stats_nhwc", (xs, ps, gs, bs, o["mean"], o["rstd"], o["scale"], o["shift"], nb,
                                                         hw, C, g, 1e-6, ws.data_ptr(), wsn, st)))
        if not part_forms:
            calls += [("mvae_group_norm_fwd_nhwc", (xs, gs, bs, o["y"], o["mean"], o["rstd"], nb, hw, C, g, 1e-6, 1, 0.0,
                                                    0, 0, ws.data_ptr(), wsn, st)),
                      ("mvae_group_norm_bwd_nhwc", (xs, ds, gs, bs, o["mean"], o["rstd"], o["dx"], None, o["dg"],
                                                    o["db"], nb, hw, C, g, 1, 0.0, 0, ws.data_ptr(), wsn, st)),
                      ("mvae_group_norm_stats_nhwc", (xs, None, gs, bs, o["mean"], o["rstd"], o["scale"], o["shift"], nb,
                                                      hw, C, g, 1e-6, ws.data_ptr(), wsn, st))]
        for name, args in calls:
            with pytest.raises(RuntimeError):
                call(name, *args)
            torch.cuda.synchronize()
            for k, v in outs.items():
                assert bool((v == SENTINEL).all()), (name, k, (nb, hw, C, g))

    case(2, 40, 128, 32, part_forms=True)    # hw % 32 != 0: the part forms only
    case(2, 32, 6, 2, part_forms=False)      # C % 4 != 0
    case(2, 32, 40, 32, part_forms=False)    # C % groups != 0
    case(2, 64, 128, 32, part_forms=False, short_ws=True)  # a workspace one byte short
