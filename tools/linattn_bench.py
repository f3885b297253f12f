#!/usr/bin/env python3
"""Linear attention core timing (csrc/linattn.hip + the batched GEMMs of ops.LinAttnCoreFn) next to the vanilla
attention core at the geometries a 224x224 model puts attention on: the stock mid block (b 32, 28x28, C 1024) and a
56x56 level at C 512, where the vanilla path would need 1.3 GB of scores per block and is skipped. Forward and backward
of each core in interleaved rounds (median and min..max over the rounds, HIP events on the launch stream), then the
stages of the linear core one by one: the streaming kernels' algorithmic bytes/s against the 5.31 TB/s copy ceiling and
the four GEMM shapes' TF/s next to the same (m, n, k, batch) on compact operands.
tools/linattn_bench.py [precision] [rounds]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from medvae_disentangled_multimodal_amd import _lib, ops  # noqa: E402

SHAPES = [("mid224_28x28x1024", 32, 1024, 28, True), ("lvl56_56x56x512", 32, 512, 56, False)]
COPY_CEILING = 5.31e12  # B/s, the project's measured copy ceiling (profiles/r02_ceilings.txt)


def timed(fn, reps=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3  # seconds


def spread(ts):
    return {"med_us": round(statistics.median(ts) * 1e6, 1), "min_us": round(min(ts) * 1e6, 1),
            "max_us": round(max(ts) * 1e6, 1)}


def cores(b, c, h, vanilla, rounds, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    cl = torch.channels_last
    qkv = torch.randn(b, 3 * c, h, h, device=dev, generator=g).contiguous(memory_format=cl).requires_grad_()
    go = torch.randn(b, c, h, h, device=dev, generator=g).contiguous(memory_format=cl)
    fns = {"linear_fwd": lambda: ops.linear_attention_core(qkv)}
    o = ops.linear_attention_core(qkv)
    fns["linear_bwd"] = lambda: torch.autograd.grad(o, qkv, go, retain_graph=True)
    if vanilla:
        tq, tk, tv = (torch.randn(b, c, h, h, device=dev, generator=g).contiguous(memory_format=cl).requires_grad_()
                      for _ in range(3))
        fns["vanilla_fwd"] = lambda: ops.attention_core(tq, tk, tv)
        ov = ops.attention_core(tq, tk, tv)
        fns["vanilla_bwd"] = lambda: torch.autograd.grad(ov, (tq, tk, tv), go, retain_graph=True)
    for fn in fns.values():  # warm-up: code objects, arena buffers
        fn()
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(rounds):  # interleaved: every variant once per round
        for k, fn in fns.items():
            ts[k].append(timed(fn))
    n = h * h
    row = {}
    for k, t in ts.items():
        fl = (4.0 if k.endswith("fwd") else 8.0) * (n * c * c * b if k.startswith("linear") else n * n * c * b)
        row[k] = dict(spread(t), **{"TF/s": round(fl / statistics.median(t) / 1e12, 1)})
    return row


def stages(b, c, h, rounds, dev):
    n = h * h
    st = torch.cuda.current_stream(dev).cuda_stream
    qkv = torch.randn(b, n, 3 * c, device=dev)
    dqkv = torch.randn(b, n, 3 * c, device=dev)
    do = torch.randn(b, n, c, device=dev)
    ksm = torch.empty(b, n, c, device=dev)
    stats = torch.empty(b, 2, c, device=dev)
    cx, dcx = torch.randn(b, c, c, device=dev), torch.randn(b, c, c, device=dev)
    ws = torch.empty(_lib.query("mvae_linattn_workspace_bytes", b, n, c), dtype=torch.uint8, device=dev)
    qp, gp, l3, s3 = qkv.data_ptr(), dqkv.data_ptr(), 3 * c, 3 * c * n
    kp = qp + 4 * c
    nb = 4.0 * b * n * c  # bytes of one [b, n, C] fp32 pass
    hbm = {
        "kstats": (nb, lambda: _lib.call("mvae_linattn_kstats", kp, l3, s3, stats.data_ptr(), b, n, c, ws.data_ptr(),
                                         ws.numel(), st)),
        "ksoftmax": (2 * nb, lambda: _lib.call("mvae_linattn_ksoftmax", kp, l3, s3, stats.data_ptr(), ksm.data_ptr(), b,
                                               n, c, st)),
        "dk": (5 * nb, lambda: _lib.call("mvae_linattn_dk", kp, l3, s3, stats.data_ptr(), gp + 4 * c, l3, s3, b, n, c,
                                         ws.data_ptr(), ws.numel(), st)),
    }
    # (ta, tb, m, n, k, A, lda, sA, B, ldb, sB, C, ldc, sC, split_k) as LinAttnCoreFn launches them, then compact
    a3 = torch.randn(b, n, c, device=dev)
    o3 = torch.empty(b, n, c, device=dev)
    gemms = {
        "ctx=ksm^T.V": ((1, 0, c, c, n, ksm.data_ptr(), c, n * c, qp + 8 * c, l3, s3, cx.data_ptr(), c, c * c, True),
                        (1, 0, c, c, n, ksm.data_ptr(), c, n * c, a3.data_ptr(), c, n * c, cx.data_ptr(), c, c * c, True)),
        "O=Q.ctx": ((0, 0, n, c, c, qp, l3, s3, cx.data_ptr(), c, c * c, o3.data_ptr(), c, n * c, False),
                    (0, 0, n, c, c, a3.data_ptr(), c, n * c, cx.data_ptr(), c, c * c, o3.data_ptr(), c, n * c, False)),
        "dQ=dO.ctx^T": ((0, 1, n, c, c, do.data_ptr(), c, n * c, cx.data_ptr(), c, c * c, gp, l3, s3, False),
                        (0, 1, n, c, c, do.data_ptr(), c, n * c, cx.data_ptr(), c, c * c, o3.data_ptr(), c, n * c, False)),
        "dksm=V.dctx^T": ((0, 1, n, c, c, qp + 8 * c, l3, s3, dcx.data_ptr(), c, c * c, gp + 4 * c, l3, s3, False),
                          (0, 1, n, c, c, a3.data_ptr(), c, n * c, dcx.data_ptr(), c, c * c, o3.data_ptr(), c, n * c, False)),
    }
    hbm["kstats"][1]()
    fns = {k: f for k, (_, f) in hbm.items()}
    for name, (sliced, compact) in gemms.items():
        for tag, a in (("sliced", sliced), ("compact", compact)):
            fns[f"{name} {tag}"] = (lambda a=a: ops._la_gemm(*a[:14], b, st, dev, split_k=a[14]))
    for fn in fns.values():
        fn()
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(timed(fn))
    row = {}
    for k, (nbytes, _) in hbm.items():
        bw = nbytes / statistics.median(ts[k])
        row[k] = dict(spread(ts[k]), **{"TB/s": round(bw / 1e12, 2), "of_copy_ceiling": round(bw / COPY_CEILING, 2)})
    for name, (sliced, _) in gemms.items():
        fl = 2.0 * sliced[2] * sliced[3] * sliced[4] * b
        for tag in ("sliced", "compact"):
            k = f"{name} {tag}"
            row[k] = dict(spread(ts[k]), **{"TF/s": round(fl / statistics.median(ts[k]) / 1e12, 1)})
    return row


def main():
    prec = sys.argv[1] if len(sys.argv) > 1 else "32"
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    ops.set_precision(prec)
    dev = torch.device("cuda:0")
    for lab, b, c, h, vanilla in SHAPES:
        row = cores(b, c, h, vanilla, rounds, dev)
        if not vanilla:
            row["vanilla"] = f"skipped: {4.0 * b * (h * h) ** 2 / 1e9:.1f} GB of scores per block at this batch"
        print(prec, lab, "cores", json.dumps(row), flush=True)
        print(prec, lab, "stages", json.dumps(stages(b, c, h, rounds, dev)), flush=True)


if __name__ == "__main__":
    main()
