#!/usr/bin/env python3
"""mvae_latent_stats (csrc/metrics.hip) device time on the flagship latent [256, 256, 8, 8] (16 MiB), a quarter batch and
the same features as an NCHW-flattened [B, D] latent: HIP events around 20 back-to-back entry-point calls (the three
launches of one call each), median and min..max over 7 rounds. 24 distinct inputs (384 MiB, more than the 256 MiB
Infinity Cache) visited in turn ("rotating") and one input repeated ("resident"); algorithmic bytes (one pass over z)
per second against the 5.31 TB/s copy ceiling; a torch copy of the same tensor (2 x the bytes) and the same three values
through torch ops in the same run for scale.
tools/latent_stats_bench.py"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from medvae_disentangled_multimodal_amd import _lib, metrics, ops  # noqa: E402

COPY_CEILING = 5.31e12  # B/s, the project's measured copy ceiling (profiles/r02_ceilings.txt)

dev = torch.device("cuda:0")
res = {}
for name, shape in (("c4_256x256x8x8", (256, 256, 8, 8)), ("b64_256x8x8", (64, 256, 8, 8)), ("c4_2d_nchw", (256, 16384))):
    nt = 24
    zs = [torch.randn(shape, device=dev) for _ in range(nt)]
    if len(shape) == 4:
        zs = [z.contiguous(memory_format=torch.channels_last) for z in zs]
        b, p, c = shape[0], shape[2] * shape[3], shape[1]
    else:
        b, p, c = shape[0], 1, shape[1]
    out = torch.empty(3, device=dev)
    ws = ops.ARENA.get("latstats", _lib.query("mvae_latent_stats_workspace_bytes", b, p, c), dev)
    st = ops._stream(zs[0])
    def run(i, reps, rotate):
        for k in range(reps):
            z = zs[(i * reps + k) % nt] if rotate else zs[0]
            _lib.call("mvae_latent_stats", z.data_ptr(), c, p * c, b, p, c, out.data_ptr(), ws.data_ptr(), ws.numel(), st)
    dst = torch.empty_like(zs[0])
    def copy(i, reps, rotate):
        for k in range(reps):
            dst.copy_(zs[(i * reps + k) % nt] if rotate else zs[0])
    nbytes = zs[0].numel() * 4
    for what, fn in (("stats", run), ("copy", copy)):
        for rotate in (True, False):
            fn(0, 20, rotate)
            torch.cuda.synchronize()
            ts = []
            for r in range(7):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(r, 20, rotate); e1.record(); torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3 / 20)
            med = statistics.median(ts)
            per_byte = nbytes * (2 if what == "copy" else 1)
            res[f"{name} {what} {'rotating' if rotate else 'resident'}"] = {
                "med_us": round(med, 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2),
                "TB/s": round(per_byte / med / 1e6, 3),
                "of_copy_ceiling": round(per_byte / med * 1e6 / COPY_CEILING, 2)}
    # torch eager for comparison (the reference's formulation on the device)
    z = zs[0]
    f = lambda: (z.flatten(1).mean(0).mean(), z.flatten(1).std(0).mean(), (z.abs() < 0.1).float().mean())
    f(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20): f()
    e1.record(); torch.cuda.synchronize()
    res[f"{name} torch_eager"] = {"us": round(e0.elapsed_time(e1) * 1e3 / 20, 2)}
    print(name, metrics.compute_latent_metrics(zs[0]))
for k, v in res.items():
    print(k, json.dumps(v))
