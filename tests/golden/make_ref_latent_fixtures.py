#!/usr/bin/env python3
"""Golden vectors for the evaluation loop's latent metrics (row f3) from the REFERENCE's own compute_latent_metrics
(src/utils/metrics.py:76-101; build container only).

    python3 -B tests/golden/make_ref_latent_fixtures.py [output directory]

The function is pure torch but its module imports sklearn and torchmetrics (not installed), so it is extracted by
`ast` with the helpers of make_ref_fixtures.py and run on seeded inputs. Only data is written
(ref_latent_metrics.npz: per case the input `<tag>.z` and the three outputs, plus `<tag>.std_err_vs_f64`, the
relative distance of the reference's fp32 latent_std_avg from the same formula in float64); no reference source is
stored. The archive is written with fixed member timestamps, so a rerun reproduces it byte for byte.
"""
from __future__ import annotations

import io
import os
import sys
import zipfile
from typing import Dict, Optional, Tuple

sys.dont_write_bytecode = True
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import make_ref_fixtures as base  # noqa: E402

KEYS = ("latent_mean_avg", "latent_std_avg", "latent_sparsity")
# tag -> shape, offset, scale: a 2-D and a 4-D latent, one with |mean| >> std, and the B = 1 case (std is NaN)
CASES = (("flat", (6, 40), 0.0, 1.0), ("spatial", (4, 16, 7, 7), 0.0, 0.5), ("offset", (64, 8, 2, 2), 1000.0, 0.01),
         ("single", (1, 8, 2, 2), 0.0, 1.0))


def reference_latent_metrics():
    path = os.path.join(base.REF, "src", "utils", "metrics.py")
    ns = {"torch": torch, "F": F, "np": np, "Dict": Dict, "Tuple": Tuple, "Optional": Optional}
    base._compile(base._defs(path, ["compute_latent_metrics"]), ns, path)
    return ns["compute_latent_metrics"]


def latent_fixture(rng: np.random.Generator):
    fn = reference_latent_metrics()
    rec = {}
    for tag, shape, offset, scale in CASES:
        z = (offset + scale * rng.standard_normal(shape)).astype(np.float32)
        m = fn(torch.from_numpy(z))
        rec[f"{tag}.z"] = z
        for k in KEYS:
            rec[f"{tag}.{k}"] = np.array(m[k], dtype=np.float64)
        z64 = z.astype(np.float64).reshape(shape[0], -1)
        with np.errstate(invalid="ignore", divide="ignore"):
            std64 = z64.std(axis=0, ddof=1).mean() if shape[0] > 1 else np.nan
        rec[f"{tag}.std_err_vs_f64"] = np.array(abs(m["latent_std_avg"] - std64) / std64, dtype=np.float64)
    return rec


def save_npz(path: str, arrays: Dict[str, np.ndarray]):
    """np.savez with the members' timestamps pinned (np.savez stamps the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main(outdir: str = HERE) -> Dict[str, np.ndarray]:
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # (one summation order whatever the machine)
    try:
        rec = latent_fixture(np.random.Generator(np.random.PCG64(76)))
    finally:
        torch.set_num_threads(threads)
    save_npz(os.path.join(outdir, "ref_latent_metrics.npz"), rec)
    for tag, shape, _, _ in CASES:
        print(tag, shape, {k: float(rec[f"{tag}.{k}"]) for k in KEYS},
              "fp32 latent_std_avg vs float64: %.2e relative" % float(rec[f"{tag}.std_err_vs_f64"]))
    return rec


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
