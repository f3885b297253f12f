#!/usr/bin/env python3
"""mvae_film_fwd / mvae_film_bwd (csrc/film.hip) device time at the flagship c4 encoder's first and last level shapes,
[256, 128, 64, 64] (512 MiB per tensor) and [256, 1024, 8, 8] (64 MiB per tensor): HIP events around 10 back-to-back
entry-point calls, median and min..max over 7 rounds, after a warm-up of every shape. The inputs rotate over enough
distinct tensors to exceed the 256 MiB Infinity Cache. Algorithmic bytes -- forward 2 B P C 4, backward 3 B P C 4, or 2
with dx skipped -- per second, next to the 6.29 TB/s float4 copy the MI355X reaches (79 % of the 8 TB/s HBM3E
specification), the project's own measured copy ceiling (profiles/r02_ceilings.txt) and a torch copy of the same tensor in
the same run (2 x the bytes).
tools/film_bench.py"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from medvae_disentangled_multimodal_amd import _lib, ops  # noqa: E402

COPY_PEAK = 6.29e12     # B/s, float4 copy on the MI355X
COPY_CEILING = 5.31e12  # B/s, the project's measured copy ceiling (profiles/r02_ceilings.txt)
REPS, ROUNDS = 10, 7

dev = torch.device("cuda:0")
res = {}
for name, shape, nt in (("c4_level0_256x128x64x64", (256, 128, 64, 64), 2), ("c4_level3_256x1024x8x8", (256, 1024, 8, 8), 8)):
    b, c, h, w = shape
    p = h * w
    xs = [torch.randn(shape, device=dev).contiguous(memory_format=torch.channels_last) for _ in range(nt)]
    dys = [torch.randn(shape, device=dev).contiguous(memory_format=torch.channels_last) for _ in range(nt)]
    out = torch.empty_like(xs[0])
    scale, shift = torch.randn(b, c, device=dev), torch.randn(b, c, device=dev)
    dsc, dsh = torch.empty(b, c, device=dev), torch.empty(b, c, device=dev)
    ws = ops.ARENA.get("film", _lib.query("mvae_film_workspace_bytes", b, p, c), dev)
    st = ops._stream(xs[0])

    def fwd(i):
        _lib.call("mvae_film_fwd", xs[i % nt].data_ptr(), c, scale.data_ptr(), shift.data_ptr(), out.data_ptr(), b, p, c, st)

    def bwd(i, dx=1):
        _lib.call("mvae_film_bwd", xs[i % nt].data_ptr(), c, dys[i % nt].data_ptr(), c, scale.data_ptr(), out.data_ptr(),
                  dsc.data_ptr(), dsh.data_ptr(), b, p, c, dx, ws.data_ptr(), ws.numel(), st)

    nbytes = xs[0].numel() * 4
    for what, fn, passes in (("fwd", fwd, 2), ("bwd", bwd, 3), ("bwd_no_dx", lambda i: bwd(i, 0), 2),
                             ("torch_copy", lambda i: out.copy_(xs[i % nt]), 2)):
        for i in range(REPS):
            fn(i)
        torch.cuda.synchronize()
        ts = []
        for r in range(ROUNDS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(REPS):
                fn(r * REPS + k)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / REPS)
        med = statistics.median(ts)
        rate = passes * nbytes / med * 1e6
        res[f"{name} {what}"] = {"med_us": round(med, 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2),
                                 "algorithmic_MiB": passes * nbytes >> 20, "TB/s": round(rate / 1e12, 3),
                                 "of_6.29_TB/s_copy": round(rate / COPY_PEAK, 2),
                                 "of_project_copy_ceiling": round(rate / COPY_CEILING, 2)}
    del xs, dys, out
for k, v in res.items():
    print(k, json.dumps(v))
