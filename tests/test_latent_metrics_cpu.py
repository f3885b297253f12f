"""Latent metrics without a GPU: the new C ABI entry points report argument errors without touching a device, the
workspace query plans on the host, and the reference fixture (tests/golden/ref_latent_metrics.npz) is what its
generator writes -- byte for byte where the reference is present -- and agrees with the float64 restatement of
src/utils/metrics.py:76-101."""
import importlib.util
import os
import shutil
import warnings

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("latent_mean_avg", "latent_std_avg", "latent_sparsity")


def restate(z):
    """The three formulas in float64 on [B, ...] -> [B, D]; returns (mean, std, sparse count, elements)."""
    z = np.asarray(z, dtype=np.float64).reshape(z.shape[0], -1)
    with np.errstate(invalid="ignore", divide="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mean = z.mean(axis=0).mean()
        std = z.std(axis=0, ddof=1).mean() if z.shape[0] > 1 else np.nan
    return mean, std, int((np.abs(z) < 0.1).sum()), z.size


def test_latent_stats_entry_points_report_argument_errors_without_gpu():
    from medvae_disentangled_multimodal_amd import _lib
    lib = _lib.load()
    one = 16  # a non-null, 16-byte aligned address that is never dereferenced: every call below fails its checks first
    calls = [
        (None, 0, 0, 0, 0, 0, None, None, 0, None),
        (None, 8, 32, 2, 4, 8, one, one, 1 << 20, None),   # no input
        (one, 8, 32, 2, 4, 8, None, one, 1 << 20, None),   # no output
        (one, 8, 32, 0, 4, 8, one, one, 1 << 20, None),    # batch = 0
        (one, 8, 32, 2, 0, 8, one, one, 1 << 20, None),    # pixels = 0
        (one, 8, 32, 2, 4, 0, one, one, 1 << 20, None),    # channels = 0
        (one, 4, 32, 2, 4, 8, one, one, 1 << 20, None),    # ld < channels
        (one, 8, -32, 2, 4, 8, one, one, 1 << 20, None),   # negative image stride
    ]
    for args in calls:
        assert lib.mvae_latent_stats(*args) == -1, args
        assert b"latent_stats" in lib.mvae_last_error(), (args, lib.mvae_last_error())
    with pytest.raises(RuntimeError, match="latent_stats"):
        _lib.call("mvae_latent_stats", None, 0, 0, 0, 0, 0, None, None, 0, None)
    # a missing, misaligned or short workspace is reported too (status -2, like the other workspace-taking entries)
    need = _lib.query("mvae_latent_stats_workspace_bytes", 2, 4, 8)
    for ws, nbytes in ((None, 0), (one, need - 1), (one + 4, 1 << 20)):
        assert lib.mvae_latent_stats(one, 8, 32, 2, 4, 8, one, ws, nbytes, None) == -2, (ws, nbytes)
        assert b"latent_stats" in lib.mvae_last_error()


def test_latent_stats_workspace_planning_without_gpu():
    from medvae_disentangled_multimodal_amd import _lib
    q = lambda *a: _lib.query("mvae_latent_stats_workspace_bytes", *a)
    assert q(0, 0, 0) == 0 and q(0, 4, 8) == 0 and q(2, 0, 8) == 0 and q(2, 4, 0) == 0
    # one split: a (sum of means, sum of stds) pair per 256 features, one count per workgroup, mean + M2 per feature
    assert q(2, 1, 4) == 16 + 16 + 2 * 4 * 8
    # the flagship latent [256][8 * 8][256]: D = 16 384 features in 64 groups of 64 quads, the batch in 8 splits of 32
    # (512 workgroups, two per CU): the partial means and M2s are [8][D] doubles each
    d = 64 * 256
    assert q(256, 64, 256) == (d // 256) * 16 + 64 * 8 * 8 + 2 * 8 * d * 8
    # D tiny and the batch large: the batch is split although a single workgroup would hold every feature
    assert q(300, 1, 4) > q(2, 1, 4) + 2 * 4 * 8


@pytest.mark.parametrize("tag", ["flat", "spatial", "offset", "single"])
def test_reference_fixture_agrees_with_the_float64_restatement(tag):
    """The reference's own fp32 results against the formulas in float64: the bounds of the GPU test (1e-5 relative
    on latent_std_avg, 1e-5 mean|z| absolute on latent_mean_avg, the sparse count exact), and the recorded distance
    of its latent_std_avg from float64 is of the order of 1e-6 or below."""
    ref = np.load(os.path.join(GOLDEN, "ref_latent_metrics.npz"), allow_pickle=False)
    z = ref[f"{tag}.z"]
    mean, std, count, n = restate(z)
    assert abs(float(ref[f"{tag}.latent_mean_avg"]) - mean) <= 1e-5 * np.abs(z).mean()
    assert round(float(ref[f"{tag}.latent_sparsity"]) * n) == count
    if z.shape[0] == 1:
        assert np.isnan(ref[f"{tag}.latent_std_avg"]) and np.isnan(std)
    else:
        assert float(ref[f"{tag}.latent_std_avg"]) == pytest.approx(std, rel=1e-5)
        assert float(ref[f"{tag}.std_err_vs_f64"]) < 2e-6
        assert abs(float(ref[f"{tag}.latent_std_avg"]) - std) / std == pytest.approx(
            float(ref[f"{tag}.std_err_vs_f64"]), abs=1e-12)
    shapes = {t: ref[f"{t}.z"].shape for t in ("flat", "spatial")}
    assert len(shapes["flat"]) == 2 and len(shapes["spatial"]) == 4 and min(s[0] for s in shapes.values()) >= 2


def test_fixture_generator_reproduces_the_committed_file(tmp_path):
    """The generator, run in a scratch copy next to a copy of make_ref_fixtures.py, writes the committed archive byte
    for byte (needs the reference checkout the generators read: MEDVAE_REFERENCE)."""
    for name in ("make_ref_fixtures.py", "make_ref_latent_fixtures.py"):
        shutil.copy(os.path.join(GOLDEN, name), tmp_path / name)
    spec = importlib.util.spec_from_file_location("scratch_make_ref_latent_fixtures",
                                                  tmp_path / "make_ref_latent_fixtures.py")
    gen = importlib.util.module_from_spec(spec)
    import sys
    path, mods = list(sys.path), {k: sys.modules.get(k) for k in ("make_ref_fixtures",)}
    sys.modules.pop("make_ref_fixtures", None)
    try:
        spec.loader.exec_module(gen)
        assert os.path.dirname(os.path.abspath(gen.base.__file__)) == str(tmp_path)
        if not os.path.isfile(os.path.join(gen.base.REF, "src", "utils", "metrics.py")):
            pytest.skip("the reference checkout is not on this machine")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (torch warns about the B = 1 case's std, as in the reference)
            gen.main(str(tmp_path))
    finally:
        sys.path[:] = path
        sys.modules.pop("make_ref_fixtures", None)
        for k, v in mods.items():
            if v is not None:
                sys.modules[k] = v
    got = (tmp_path / "ref_latent_metrics.npz").read_bytes()
    want = open(os.path.join(GOLDEN, "ref_latent_metrics.npz"), "rb").read()
    assert got == want
    assert len(want) < 300 * 1024
