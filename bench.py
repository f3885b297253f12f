#!/usr/bin/env python3
"""Training-throughput benchmark of the MI355X conv-VAE hot path.

Workload (BASELINE.json metric, config 4): multimodal ConditionalVAE at 64x64x3, batch 256 per GPU
(configs/experiment/multi_modal_cvae.yaml + model.resolution=64, training.loss.type=vae;
AdamW lr 1e-4 betas (0.5, 0.999) wd 1e-5, gradient clip 1.0 -- configs/training/advanced.yaml),
927 M parameters, fp32 semantics. One step = one Lightning automatic-optimisation step:
forward + VAE loss + backward + [gradient all-reduce] + non-finite zeroing + clip + AdamW.
Synthetic MedMNIST-shaped data resident in HBM (x = randint(0,256)/255*2-1, random one-hot of 12).

    python bench.py [--gpus N --steps K --warmup W --config c4|c5|c2|c3] [--dump-outputs DIR] [--full]
        N > 1 without a launcher: bench.py spawns N rank processes itself (before anything touches
        the GPU), one per GPU, RCCL ("nccl") process group over 127.0.0.1
    torchrun --nproc-per-node N bench.py --gpus N ...   (the same, launched externally)

A plain run sets up, warms up, times the K steps, writes the last timed step's outputs (--dump-outputs DIR:
DIR/<name>.npy, float32, the same inputs and so the same arrays from run to run) and prints the line; its
`roofline`, `cpu_baseline`, `configs` and `parity` are measured under --full only.

Rank 0 prints ONE JSON line (value = images/s over all ranks, max-over-ranks timing), with --full also
  roofline:     the implicit-GEMM MFMA kernel family, live HIP-event timing of every launch in one
                instrumented step after the timed region (algorithmic FLOPs = the reference's conv /
                bmm FLOPs), peak = the 3xBF16 ceiling (bf16 dense MFMA 2.5 PF / 3 products)
  cpu_baseline: the CPU oracle (reference algorithm restated, tests-pinned) timed on this host on a
                bounded sample (rank 0, N=1 only)
  configs:      the other BASELINE configs (c1 / c2 / c3 / c5 / c4x) on the same GPU (N=1, no --config / --batch)
  parity:       one step of the cvae_c4_full golden case against the reference's recorded outputs (same condition).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MODALITIES = ["chestmnist", "pathmnist", "octmnist", "pneumoniamnist", "dermamnist", "bloodmnist", "tissuemnist",
              "retinamnist", "breastmnist", "organamnist", "organcmnist", "organsmnist"]

CONFIGS = {
    # BASELINE config 4 (the metric's config): multi_modal_cvae @ 64x64, bs 256 per GPU
    "c4": dict(cls="ConditionalVAE", res=64, batch=256,
               kwargs=dict(input_channels=3, latent_dim=256, hidden_channels=256, ch_mult=(1, 2, 4, 8),
                           num_res_blocks=2, attn_resolutions=[16], dropout=0.0, resolution=64,
                           modalities=MODALITIES, condition_method="concat"),
               opt=dict(type="adamw", lr=1e-4, weight_decay=1e-5, betas=[0.5, 0.999]), clip=1.0,
               loss=dict(type="vae", recon_loss_type="mse", kl_weight=1.0, recon_weight=1.0)),
    # BASELINE config 5: config 4 + bf16-mixed + LPIPS(VGG) generator objective (LPIPS + 1e-5 * KL.sum()/B)
    "c5": dict(cls="ConditionalVAE", res=64, batch=256, precision="bf16-mixed",
               kwargs=dict(input_channels=3, latent_dim=256, hidden_channels=256, ch_mult=(1, 2, 4, 8),
                           num_res_blocks=2, attn_resolutions=[16], dropout=0.0, resolution=64,
                           modalities=MODALITIES, condition_method="concat"),
               opt=dict(type="adamw", lr=1e-4, weight_decay=1e-5, betas=[0.5, 0.999]), clip=1.0,
               loss=dict(type="lpips_discriminator", perceptual_factor=1.0, kl_factor=1e-5,
                         discriminator_iter_start=10000, allow_synthetic_lpips=True, lpips_net="vgg")),
    # BASELINE config 1: chest_base_vae at 28x28x1 with the 3-level ch_mult (SURVEY top note 3), bs 32, AdamW 2e-4
    # wd 1e-4, clip 1.0 (the reference runs it on the CPU; here it is the same step on the GPU path)
    "c1": dict(cls="BaseVAE", res=28, batch=32, cpu_batch=32, graph=True,
               kwargs=dict(input_channels=1, latent_dim=256, hidden_channels=128, ch_mult=(1, 2, 4),
                           num_res_blocks=2, attn_resolutions=[16], dropout=0.0, resolution=28),
               opt=dict(type="adamw", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.999]), clip=1.0,
               loss=dict(type="vae", recon_loss_type="mse", kl_weight=1.0, recon_weight=1.0)),
    # BASELINE config 2: path_beta_vae at 28x28x3 with the 3-level ch_mult, bs 256
    "c2": dict(cls="BetaVAE", res=28, batch=256, cpu_batch=16, graph=True,
               kwargs=dict(input_channels=3, latent_dim=128, hidden_channels=128, ch_mult=(1, 2, 4),
                           num_res_blocks=2, attn_resolutions=[16], dropout=0.0, resolution=28, beta=6.0),
               opt=dict(type="adamw", lr=1e-4, weight_decay=1e-4, betas=[0.9, 0.999]), clip=1.0,
               loss=dict(type="vae", recon_loss_type="mse", kl_weight=6.0, recon_weight=1.0)),
    # BASELINE config 3: disentangled_multi_modal_cvae_quick (configs/model/disentangled_conditional_vae_quick.yaml,
    # configs/experiment/disentangled_multi_modal_cvae_quick.yaml: Adam lr 5e-4, clip 0.5, dropout 0.1), bs 512,
    # a mixed batch of the 5 modalities (1-channel images zero-padded to 3 by the collate)
    "c3": dict(cls="DisentangledConditionalVAE", res=28, batch=512, cpu_batch=512, graph=True,
               kwargs=dict(num_modalities=5, shared_latent_dim=8, modality_latent_dim=8, hidden_channels=32,
                           ch_mult=(1, 2, 4), num_res_blocks=1, attn_resolutions=[], dropout=0.1, resolution=28,
                           modality_separation_weight=0.1, contrastive_weight=0.05),
               opt=dict(type="adam", lr=5e-4, weight_decay=0.0, betas=[0.9, 0.999]), clip=0.5,
               loss=dict(type="disentangled_vae", recon_loss_type="mse", kl_weight=1.0, recon_weight=1.0,
                         separation_weight=0.1, contrastive_weight=0.05)),
}
# config 4 in EXACT fp32 (the reference's arithmetic: every conv / bmm on the f32-input MFMA, v_mfma_f32_*_f32, no
# operand rounding) -- timed next to the default 3xBF16 line against the 157.3 TF/s fp32 MFMA peak
CONFIGS["c4x"] = dict(CONFIGS["c4"], precision="32-exact")
METRIC_C4 = "training images/sec (whole node) + ELBO parity, multimodal CVAE 64\u00d764 bs=256"

BF16_DENSE_PEAK_TF = 2500.0
PEAK_3XBF16_TF = BF16_DENSE_PEAK_TF / 3.0
FP32_MFMA_PEAK_TF = 157.3  # dense f32-input MFMA (v_mfma_f32_32x32x2_f32 / 16x16x4_f32)
HBM_PEAK_GBS = 8000.0
# measured on MI355X (profiles/r02_ceilings.txt): the GEMM main-loop structure without global traffic, per MFMA
# shape (fp32-equivalent TF/s), and plain HBM streams (read-only / copy)
STRUCT_CEIL_TF = {"conv_fwd": 598.0, "conv_dgrad": 598.0, "conv_wgrad": 559.0, "attn_gemm": 559.0}
HBM_MEASURED_GBS = {"read_only": 6262.0, "copy": 5314.0}


def _pmc_traffic(config, family="gemm"):
    """HBM bytes per launch of a kernel family (gemm: gemm3x_kernel; gn: the gn_* GroupNorm chains) from the
    committed PMC passes (tools/gpu_evidence.sh traffic: FETCH_SIZE x2 + WRITE_SIZE, rocprofv3 --pmc, separate passes) --
    counters cannot be read inside this timed run, so the profile of the same command is attached (newest round
    first)."""
    for tag in ("r06", "r05", "r04", "r03", "r02", "r01"):
        path = os.path.join(ROOT, "profiles", f"{tag}_{config}_{family}_traffic.json")
        if os.path.exists(path):
            break
    else:
        return None
    with open(path) as f:
        t = json.load(f)
    return {"bytes_per_launch": round(t["traffic_bytes_per_launch"]), "unit": "B",
            "fetch_bytes_per_launch": round(t["fetch_bytes_per_launch"]),
            "write_bytes_per_launch": round(t["write_bytes_per_launch"]), "launches": t["launches"],
            "total_bytes_per_step": round(t.get("traffic_bytes_total", 0.0) / t.get("steps", 1)),
            "source": os.path.relpath(path, ROOT)}


def gemm_algorithmic_bytes(tag, shape):
    """Operand + output bytes of one GEMM-family launch if every operand were read once and the output written
    once (fp32): conv passes from the layer shape (n, cin, h, w, cout, k, stride, upsample), attention products
    from (m, n, k, batch)."""
    if tag == "attn_gemm":
        m, n, k, b = shape
        return 4.0 * b * (m * k + k * n + m * n)
    n, c, h, w, co, k, stride, ups = shape
    ho, wo = (2 * h, 2 * w) if ups else (h // stride, w // stride) if stride > 1 else (h, w)
    return 4.0 * (n * h * w * c + co * k * k * c + n * ho * wo * co)


def make_batch(cfg, device, gen):
    B, r = cfg["batch"], cfg["res"]
    C = cfg["kwargs"].get("input_channels", 3)
    x = torch.randint(0, 256, (B, C, r, r), generator=gen, device=device).float() / 255 * 2 - 1
    labels = torch.zeros(B, 1, dtype=torch.long, device=device)
    if cfg["cls"] == "DisentangledConditionalVAE":
        # modality ids 0..4 (medmnist_data.py:138-152); gray modalities 0 / 3 zero-padded to 3 channels (:16-72)
        idx = torch.randint(0, 5, (B,), generator=gen, device=device)
        gray = (idx == 0) | (idx == 3)
        x[:, 1:] = torch.where(gray.view(B, 1, 1, 1), torch.zeros_like(x[:, 1:]), x[:, 1:])
        oh = torch.nn.functional.one_hot(idx, 12).float()
        return (x, labels, oh, idx)
    if cfg["cls"] == "ConditionalVAE":
        idx = torch.randint(0, 12, (B,), generator=gen, device=device)
        oh = torch.nn.functional.one_hot(idx, 12).float()
        return (x, labels, oh)
    return (x, labels)


def cpu_baseline(cfg, seconds_budget=20.0):
    """Time the CPU oracle (oracle/torch_ref.py: the reference algorithm, pinned by the golden tests)
    on a bounded sample: training steps (fwd+loss+bwd+clip+Adam/AdamW) at the config's `cpu_batch`
    (default 2) on the host's torch threads."""
    from oracle import torch_ref as R
    threads = torch.get_num_threads()
    a = R.make_arch(cfg["cls"], dict(cfg["kwargs"]))
    g = torch.Generator().manual_seed(0)
    P = {k: torch.randn(s, generator=g) * 0.02 for k, s in R.param_shapes(a)}
    bs = cfg.get("cpu_batch", 2)
    x = torch.randint(0, 256, (bs, a.input_channels, a.resolution, a.resolution), generator=g).float() / 255 * 2 - 1
    cond = None
    if a.cls == "ConditionalVAE":
        cond = torch.nn.functional.one_hot(torch.randint(0, 12, (bs,), generator=g), 12).float()
    elif a.cls == "DisentangledConditionalVAE":
        cond = torch.randint(0, 5, (bs,), generator=g)
        x[:, 1:] = torch.where(((cond == 0) | (cond == 3)).view(bs, 1, 1, 1), torch.zeros_like(x[:, 1:]), x[:, 1:])
    eps = torch.randn(bs, a.latent_dim, a.enc_res, a.enc_res, generator=g)
    t0 = time.perf_counter()
    steps = 0
    while True:
        R.train_step(P, a, x, cond, eps, cfg["loss"], cfg["opt"], cfg["clip"])
        steps += 1
        if time.perf_counter() - t0 > seconds_budget / 2 or steps >= 3:
            break
    dt = (time.perf_counter() - t0) / steps
    try:
        affinity = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        affinity = None
    return {"value": round(bs / dt, 4), "unit": "images/s", "cores": threads, "host_nproc": os.cpu_count(),
            "cores_note": (f"torch intra-op threads = {threads} (OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS')}, "
                           f"the GPU box's CPU share for one GPU); process CPU affinity {affinity} of "
                           f"{os.cpu_count()} host CPUs"),
            "kind": "port",
            "sample": f"{steps} oracle training step(s) at batch {bs} of the same model (fp32, CPU), "
                      f"{dt:.2f} s/step"}


def _free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n: int, cmd=None) -> int:
    """`bench.py --gpus N` without an external launcher: start N rank processes of this script (fresh
    interpreters -- this parent never touches the GPU), one per GPU, with torchrun's environment
    (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT). Rank 0 prints the JSON line.
    Returns the first non-zero child exit code (the other ranks are then stopped)."""
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), GROUP_RANK="0",
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen(cmd or [sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    pending = list(procs)
    while pending:
        for p in list(pending):
            c = p.poll()
            if c is None:
                continue
            pending.remove(p)
            if c != 0 and rc == 0:
                rc = c
                for q in pending:
                    q.terminate()
        time.sleep(0.2)
    return rc


def cpu_baseline_for(cfg, seconds_budget=20.0):
    """cpu_baseline() for any config; c5's objective (bf16 + LPIPS-VGG generator loss) is timed as the oracle's fp32
    LPIPS-VGG objective over the same model (the reference's CPU path has no bf16 autocast for these convs)."""
    if cfg["loss"]["type"] in ("vae", "disentangled_vae"):
        return cpu_baseline(cfg, seconds_budget)
    from oracle import torch_ref as R
    from medvae_disentangled_multimodal_amd.lpips import LPIPS
    lp = LPIPS(net=cfg["loss"].get("lpips_net", "alex"), allow_synthetic=True)
    c = dict(cfg)
    c["loss"] = dict(cfg["loss"], lpips_weights={k: v.detach() for k, v in lp.internal_weights().items()})
    out = cpu_baseline(c, seconds_budget)
    out["sample"] += "; objective: LPIPS-VGG (oracle lpips_vgg, synthetic weights) + 1e-5 * KL.sum()/B"
    return out


def _roofline(rec_all, bf16, config, step_ms, detail, rank, exact=False):
    """GEMM-family (MFMA) and GroupNorm-family (HBM) rooflines from the HIP-event records of one step."""
    rec = [r for r in rec_all if r[0] not in ops_hbm_tags()]
    hbm_rec = [r for r in rec_all if r[0] in ops_hbm_tags()]
    tot_ms = sum(r[2].elapsed_time(r[3]) for r in rec)
    tot_fl = sum(r[1] for r in rec)
    tot_ref = sum(r[5] for r in rec)
    if detail and rank == 0:
        agg = {}
        for tag, f, s_, e, shp, _ in rec:
            d = agg.setdefault((tag, shp), [0, 0.0, 0.0])
            d[0] += 1
            d[1] += f
            d[2] += s_.elapsed_time(e)
        for (tag, shp), (cnt, f, ms) in sorted(agg.items(), key=lambda kv: -kv[1][2]):
            print(f"[detail {config}] {tag:10s} {str(shp):42s} x{cnt:3d} {ms:8.2f} ms {f / (ms * 1e-3) / 1e12:7.1f} TF/s",
                  file=sys.stderr)
    by = {}
    for tag, f, s_, e, _, _ in rec:
        d = by.setdefault(tag, [0, 0.0, 0.0])
        d[0] += 1
        d[1] += f
        d[2] += s_.elapsed_time(e)
    ach = tot_fl / (tot_ms * 1e-3) / 1e12
    alg_bytes = sum(gemm_algorithmic_bytes(r[0], r[4]) for r in rec) / max(len(rec), 1)
    peak = BF16_DENSE_PEAK_TF if bf16 else FP32_MFMA_PEAK_TF if exact else PEAK_3XBF16_TF
    # HBM traffic of every kernel the timed passes launch (implicit GEMM, reducers, Winograd transforms, attention):
    # the PMC bytes of one step over the passes of one step, so `traffic` and `algorithmic_bytes_per_launch` are per
    # timed pass alike (older rounds: gemm3x_kernel launches only)
    pmc = _pmc_traffic(config, "mfma")
    if pmc is not None and rec:
        pmc["bytes_per_launch"] = round(pmc["total_bytes_per_step"] / len(rec))
        pmc["unit_note"] = "HBM bytes per timed pass (PMC family bytes per step / passes per step)"
    else:
        pmc = _pmc_traffic(config)
    roofline = {"bound": "mfma", "kernel": ("gemm3x_kernel (implicit-GEMM conv, Winograd position GEMMs with their "
                                            "transforms, attention bmm; all launches)"),
                "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
                "frac": round(ach / peak, 4), "traffic": (pmc or {}).get("bytes_per_launch"),
                "traffic_unit": (pmc or {}).get("unit_note", "HBM bytes per gemm3x launch (PMC)"), "traffic_detail": pmc,
                "algorithmic_bytes_per_launch": round(alg_bytes),
                "peak_note": ("bf16 dense MFMA peak 2.5 PF/s (bf16 operands, fp32 accumulate)" if bf16 else
                              "exact fp32: dense f32-input MFMA peak 157.3 TF/s" if exact else
                              "3xBF16 fp32-emulation ceiling = bf16 dense MFMA 2.5 PF/s / 3; "
                              "native fp32 MFMA peak is 157.3 TF/s"),
                "achieved_note": ("algorithmic FLOPs of the algorithms run (Upsample convs in sub-pixel form "
                                  "count 4/9 of the reference conv's FLOPs, Winograd F(4x4,3x3) convs 1/4) over the "
                                  "time of all their launches, transforms included"),
                "reference_equivalent_TFLOP/s": round(tot_ref / (tot_ms * 1e-3) / 1e12, 2),
                "launches_per_step": len(rec), "avg_launch_us": round(tot_ms * 1e3 / max(len(rec), 1), 2),
                "gemm_ms_per_step": round(tot_ms, 2), "instrumented_step_ms": round(step_ms, 2),
                "gemm_share_of_step": round(tot_ms / step_ms, 3),
                "by_pass": {k: {"launches": v[0], "ms": round(v[2], 2),
                                "TFLOP/s": round(v[1] / (v[2] * 1e-3) / 1e12, 1)} for k, v in by.items()}}
    if not bf16 and not exact:  # measured ceiling of the main-loop structure (no global traffic): r02_ceilings.txt
        for k, v in roofline["by_pass"].items():
            c = STRUCT_CEIL_TF.get(k)
            if c is None:
                continue
            v["structure_ceiling_TFLOP/s"] = c
            v["frac_of_structure_ceiling"] = round(v["TFLOP/s"] / c, 3)
        roofline["structure_ceiling_note"] = (
            "measured on the box: the kernel's per-wave 3xBF16 LDS-fragment + MFMA loop with one barrier per "
            "K-tile and no global loads, random operands (tools/micro/mfma_shape.hip): 16x16x32 (fwd / dgrad) "
            "598 TF/s, 32x32x16 (wgrad / attention) 559 TF/s fp32-equivalent")
    loss_rec = [r for r in hbm_rec if r[0].startswith("loss_")]
    hbm_rec = [r for r in hbm_rec if r[0].startswith("gn_")]
    if loss_rec:  # the loss side (reparameterization, KL, reconstruction; SURVEY 8(d) bytes) against the HBM roofline
        lb = {}
        for tag, nbytes, s_, e, shp, _ in loss_rec:
            d = lb.setdefault(f"{shp[0]}_{tag[5:]}", [0, 0.0, 0.0])
            d[0] += 1
            d[1] += nbytes
            d[2] += s_.elapsed_time(e)
        lms = sum(v[2] for v in lb.values())
        lby = sum(v[1] for v in lb.values())
        roofline["hbm_loss_kernels"] = {
            "bound": "hbm", "kernel": "reparam_fwd / reparam_bwd, KL reduce / kl_bwd, MSE reduce / recon_bwd (csrc/loss.hip)",
            "achieved": round(lby / (lms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(lby / (lms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "ms_per_step": round(lms, 3),
            "algorithmic_bytes_per_step": round(lby),
            "bytes_note": "algorithmic bytes (SURVEY 8(d)): reparam fwd 16 B/latent (read mu, logvar, eps; write z), "
                          "reparam bwd 16 B/latent (read dz, eps, logvar; write dlogvar), KL fwd 8 B/latent, KL bwd "
                          "16 B/latent (write dmu, dlogvar), MSE fwd 8 B/pixel, MSE bwd 12 B/pixel; the reduce launches "
                          "include their fixed-order final stage",
            "by_pass": {k: {"launches": v[0], "ms": round(v[2], 4), "bytes": round(v[1]),
                            "GB/s": round(v[1] / (v[2] * 1e-3) / 1e9, 1)} for k, v in lb.items()}}
        lpmc = _pmc_traffic(config, "loss")
        if lpmc:
            moved = lpmc["total_bytes_per_step"]
            roofline["hbm_loss_kernels"].update({"traffic_bytes_per_step": moved,
                                                 "traffic_over_algorithmic": round(moved / max(lby, 1.0), 3),
                                                 "traffic_detail": lpmc})
    if hbm_rec:  # the memory-bound GroupNorm(+SiLU) family against the HBM roofline
        hb = {}
        for tag, nbytes, s_, e, _, _ in hbm_rec:
            d = hb.setdefault(tag, [0, 0.0, 0.0])
            d[0] += 1
            d[1] += nbytes
            d[2] += s_.elapsed_time(e)
        hms = sum(v[2] for v in hb.values())
        hby = sum(v[1] for v in hb.values())
        roofline["hbm_kernels"] = {
            "bound": "hbm", "kernel": "GroupNorm(+SiLU) fwd / bwd (gn_* kernel chains, all launches)",
            "achieved": round(hby / (hms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(hby / (hms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "ms_per_step": round(hms, 2),
            "measured_stream_GB/s": HBM_MEASURED_GBS,
            "bytes_note": "algorithmic bytes: fwd 8 B/elem (read x, write y), bwd 12 B/elem (read x, dy; write dx) "
                          "+ 4 B/elem where the residual branch's gradient is summed in (ResnetBlock / AttnBlock "
                          "norm1); chains include the statistics finalize and parameter-gradient kernels",
            "by_pass": {k: {"launches": v[0], "ms": round(v[2], 2),
                            "GB/s": round(v[1] / (v[2] * 1e-3) / 1e9, 1)} for k, v in hb.items()}}
        gpmc = _pmc_traffic(config, "gn")
        if gpmc:  # moved vs algorithmic bytes of the whole family over one step
            moved = gpmc["total_bytes_per_step"]
            roofline["hbm_kernels"].update({
                "traffic_bytes_per_step": moved, "algorithmic_bytes_per_step": round(hby),
                "traffic_over_algorithmic": round(moved / max(hby, 1.0), 3), "traffic_detail": gpmc})
    return roofline


def ops_hbm_tags():
    from medvae_disentangled_multimodal_amd import ops
    return ops.HBM_TAGS


DUMP_SAMPLE = 1 << 20        # elements kept of an output larger than this (a fixed, seeded sample of its flat view)
DUMP_PARAM_SAMPLE = 1 << 12  # elements kept of each updated parameter tensor


def _flat_sample(t, limit, gen):
    """`t` flattened, in float32 on the host; of a tensor with more than `limit` elements a sample at `limit` flat
    positions drawn from `gen` (seeded by the caller, so the positions are the same from run to run)."""
    t = t.detach().reshape(-1)
    if t.numel() > limit:
        idx = torch.randint(0, t.numel(), (limit,), generator=gen)
        t = t[idx.to(t.device)]
    return t.float().cpu().numpy()


def dump_outputs(path, mod, loss):
    """--dump-outputs: what the last timed step handed its caller -- the loss, the model outputs of that step
    (reconstruction, mean, logvar, z, ...: VAELightningModule._last_outputs) and the parameters it updated -- as
    `path`/<name>.npy in float32. Outputs over DUMP_SAMPLE elements and every parameter tensor over DUMP_PARAM_SAMPLE
    are stored as seeded samples of their flat views (about 25 MB in all for c4)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    gen = torch.Generator().manual_seed(20240)
    np.save(os.path.join(path, "loss.npy"), loss.detach().float().reshape(1).cpu().numpy())
    outs = mod._last_outputs if isinstance(mod._last_outputs, dict) else {}
    for k in sorted(outs):
        v = outs[k]
        if torch.is_tensor(v) and v.is_floating_point():
            np.save(os.path.join(path, f"{k}.npy"), _flat_sample(v, DUMP_SAMPLE, gen))
    params = [_flat_sample(p, DUMP_PARAM_SAMPLE, gen) for _, p in sorted(mod.model.named_parameters())]
    np.save(os.path.join(path, "params_after_step.npy"), np.concatenate(params))


def run_config(name, args, rank, world, dev, want_cpu=True, steps=None, warmup=None, dump=None):
    """Build the config's model, warm up, time `args.steps` steps (barrier + synchronize on both sides, max over
    ranks), write the last timed step's outputs to `dump` (if given), then under --full one instrumented step for
    the rooflines and the CPU baseline. Returns the measured fields of the JSON line."""
    import medvae_disentangled_multimodal_amd as M
    from medvae_disentangled_multimodal_amd import ddp, ops
    cfg = dict(CONFIGS[name])
    if args.batch:
        cfg["batch"] = args.batch
    n_steps = args.steps if steps is None else steps
    n_warm = args.warmup if warmup is None else warmup
    torch.manual_seed(42)
    model = getattr(M, cfg["cls"])(**cfg["kwargs"]).to(dev)
    mod = M.VAELightningModule(model, cfg["opt"], {"type": "none"}, cfg["loss"], gradient_clip_val=cfg["clip"],
                               precision=cfg.get("precision", "32"))
    mod.configure_optimizers()
    if world > 1:
        ddp.DataParallel(mod)
    nparams = sum(p.numel() for p in model.parameters())
    gen = torch.Generator(device=dev).manual_seed(1234 + rank)
    batches = [make_batch(cfg, dev, gen) for _ in range(2)]

    # the small configs (c1-c3: ~800 launches of a few microseconds per step) replay the whole step as one captured
    # HIP graph -- same kernels and arithmetic, the host issues one launch per step (N > 1: the graph holds the
    # bucketed RCCL all-reduces too, or two graphs around an eager exchange on other backends); eager for c4 / c5
    graphed = cfg.get("graph", False) and not args.eager
    launch = ("hip graph (captured step" + ("" if world == 1 else f", dp capture {mod._dp_capture_mode()}") + ")"
              if graphed else "eager")
    step = mod.fit_step_graphed if graphed else mod.fit_step
    for i in range(n_warm):
        mod.fit_step(batches[i % 2], i)
    if graphed:  # graph set-up, untimed: one eager step (if no warm-up ran), the capture (records, executes
        if n_warm == 0:  # nothing), one replay
            mod.fit_step(batches[0], 0)
        step(batches[n_warm % 2], n_warm)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n_steps):
        loss = step(batches[i % 2], i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    loss_v = float(loss.detach())
    peak_gb = torch.cuda.max_memory_allocated(dev) / 1e9  # HBM held by the step (caching allocator peak)
    if dump and rank == 0:
        dump_outputs(dump, mod, loss)

    roofline = None
    bf16 = cfg.get("precision", "32") == "bf16-mixed"
    exact = cfg.get("precision", "32") == "32-exact"
    if args.full and not args.no_kernel_timing:
        ops.PROFILE = []
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        mod.fit_step(batches[0], 0)
        torch.cuda.synchronize()
        step_ms = (time.perf_counter() - t1) * 1e3
        rec_all = ops.PROFILE
        ops.PROFILE = None
        roofline = _roofline(rec_all, bf16, name, step_ms, args.detail, rank, exact)
    del mod, model, batches, step
    torch.cuda.synchronize()
    torch.cuda.empty_cache()

    cpu = None
    if args.full and rank == 0 and world == 1 and want_cpu and not args.no_cpu_baseline:
        cpu = cpu_baseline_for(cfg)
    imgs = cfg["batch"] * world * n_steps
    return {"value": round(imgs / dt, 3), "unit": "images/s", "steps": n_steps, "warmup": n_warm,
            "ms_per_step": round(dt / n_steps * 1e3, 3),
            "dtype": ("bf16 (bf16-mixed: bf16 MFMA operands, fp32 accumulate/activations)" if bf16
                      else "fp32 (exact: f32-input MFMA, no operand rounding)" if exact
                      else "fp32 (3xBF16 MFMA, fp32 accumulate)"),
            "config": {"workload": f"{cfg['cls']} {cfg['res']}x{cfg['res']}x{cfg['kwargs'].get('input_channels', 3)} "
                                   f"train step (fwd+loss+bwd+clip+{cfg['opt']['type']})"
                                   + (" + LPIPS-VGG generator objective" if bf16 else "")
                                   + (", exact fp32 arithmetic" if exact else ""),
                       "model": cfg["cls"], "params": nparams, "global_batch": cfg["batch"] * world,
                       "per_gpu_batch": cfg["batch"], "resolution": cfg["res"], "parallelism": f"dp{world}",
                       "rccl_world_size": world, "backend": dist.get_backend() if world > 1 else None,
                       "step_launch": launch, "peak_hbm_GB": round(peak_gb, 1)},
            "loss": round(loss_v, 6), "roofline": roofline, "cpu_baseline": cpu}


def parity_block(dev):
    """ELBO parity of the metric's model at its exact architecture: one training step of the cvae_c4_full golden
    case (the reference's own src.models ConditionalVAE, 927 M parameters, B=2; tests/golden/make_golden.py) on the
    HIP path, compared with the reference's outputs, loss terms and global gradient norm (north_star: 1e-3
    relative), plus the one-hot condition map bitwise. Runs after the timed region."""
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    import medvae_disentangled_multimodal_amd as M
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from cases import CASES
    from weights import synth_param
    name = "cvae_c4_full"
    case = CASES[name]
    with open(os.path.join(ROOT, "tests", "golden", f"{name}.json")) as f:
        meta = json.load(f)
    data = dict(np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"), allow_pickle=False))
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:  # the golden weights, regenerated from their names (weights.py)
        arrs = list(ex.map(lambda ks: synth_param(ks[0], ks[1]), [(k, tuple(s)) for k, s in meta["params"]]))
    state = {k: torch.from_numpy(a) for (k, _), a in zip(meta["params"], arrs)}
    model = getattr(M, case["cls"])(**case["kwargs"])
    model.load_state_dict(state)
    model = model.to(dev)
    mod = M.VAELightningModule(model, case["optimizer"], {"type": "none"}, case["loss"], gradient_clip_val=case["clip"])
    mod.configure_optimizers()
    x = torch.from_numpy(data["in.x"]).to(dev)
    batch = (x, torch.zeros(x.shape[0], 1, dtype=torch.long, device=dev), torch.from_numpy(data["in.cond"]).to(dev))
    eps = torch.from_numpy(data["in.eps"]).to(dev)
    lin = model.condition_proj[0]
    with torch.no_grad():  # the one-hot condition map, before the step updates condition_proj
        from medvae_disentangled_multimodal_amd import ops
        xc, _ = ops.condition_concat(x, batch[2], lin.weight, lin.bias)
    cm = xc[:, x.shape[1]:].detach().cpu().numpy()
    bitwise = bool(np.array_equal(cm.view(np.int32), data["out.cond_map"].view(np.int32)))
    # the Winograd convs the timed run uses at B = 256 forced on at B = 2 (the size rule would keep the implicit GEMM)
    prev_min = ops.WINOGRAD_MIN_MACS
    ops.WINOGRAD_MIN_MACS = 0.0
    try:
        mod.fit_step(batch, 0, eps=eps)
        torch.cuda.synchronize()
    finally:
        ops.WINOGRAD_MIN_MACS = prev_min
    out = mod._last_outputs

    def rel(a, b):
        a = a.detach().double().cpu().flatten()
        b = torch.from_numpy(b).double().flatten()
        return float((a - b).norm() / b.norm())

    errs = {f"out.{k}": rel(out[k], data[f"out.{k}"]) for k in ("reconstruction", "mean", "logvar", "z")}
    for k in ("loss", "recon_loss", "kl_loss"):
        ref = float(data[f"loss.{k}"])
        errs[f"loss.{k}"] = abs(float(mod.logged[f"train/{k}"]) - ref) / abs(ref)
    has = [k for k, v in meta["param_has_grad"].items() if v]
    exact = math.sqrt(sum(float(data[f"gradsum.{k}"][1]) for k in has))
    errs["grad_global_norm_vs_exact"] = abs(float(mod.optimizer.last_total_norm) - exact) / exact
    del mod, model
    torch.cuda.empty_cache()
    worst = max(errs.values())
    return {"case": f"{name} (reference src.models ConditionalVAE, c4 architecture, B=2, injected eps, Winograd convs "
                    f"forced as at B=256)",
            "tolerance": 1e-3, "pass": bool(worst < 1e-3 and bitwise), "max_rel_err": worst,
            "rel_err": {k: float(f"{v:.3e}") for k, v in errs.items()}, "condition_map_bitwise": bitwise,
            "seconds": round(time.perf_counter() - t0, 1)}


STDOUT_LINE_LIMIT = 8192  # bytes: the driver keeps only the tail of stdout (round 4's 25.8 KB line was not parsed)
_DTYPE_SHORT = {"bf16": "bf16", "fp32 (exact": "fp32-exact", "fp32 (3xBF16": "fp32-3xbf16"}


def _short_dtype(d):
    for k, v in _DTYPE_SHORT.items():
        if d and d.startswith(k):
            return v
    return d


def _compact_roofline(r):
    """the roofline of one config without notes, PMC detail or per-launch tables: the figures the driver checks"""
    if not r:
        return None
    out = {k: r[k] for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch",
                             "launches_per_step", "avg_launch_us", "gemm_ms_per_step", "instrumented_step_ms",
                             "reference_equivalent_TFLOP/s")
           if k in r}
    out["kernel"] = "gemm3x_kernel + wino_* (MFMA-roofline family)"
    if r.get("by_pass"):  # per pass: [launches, ms per step, TFLOP/s]
        out["by_pass"] = {k: [v["launches"], v["ms"], v["TFLOP/s"]] for k, v in r["by_pass"].items()}
    for fam in ("hbm_kernels", "hbm_loss_kernels"):
        h = r.get(fam)
        if h:
            out[fam] = {k: h[k] for k in ("achieved", "peak", "unit", "frac", "ms_per_step", "traffic_over_algorithmic")
                        if k in h}
    return out


def compact_line(full):
    """The ONE stdout JSON line (rank 0), at most STDOUT_LINE_LIMIT bytes: the headline fields, the headline config's
    roofline (no notes / PMC detail), its cpu_baseline, one short entry per extra config and the parity summary. The
    full record (`full`: notes, PMC traffic detail, per-family tables) goes to the detail file and stderr."""
    out = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                                "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "loss")
           if k in full}
    out["roofline"] = _compact_roofline(full.get("roofline"))
    cb = full.get("cpu_baseline")
    out["cpu_baseline"] = None if not cb else {k: cb[k] for k in ("value", "unit", "cores", "kind", "sample") if k in cb}
    if full.get("configs"):
        cfgs = {}
        for name, c in full["configs"].items():
            r = c.get("roofline") or {}
            e = {"value": c["value"], "ms_per_step": c["ms_per_step"], "steps": c.get("steps"),
                 "dtype": _short_dtype(c.get("dtype")), "frac": r.get("frac"), "peak": r.get("peak")}
            if r.get("by_pass"):
                e["TFLOP/s_by_pass"] = {k: v["TFLOP/s"] for k, v in r["by_pass"].items()}
            h = r.get("hbm_kernels")
            if h:
                e["gn_hbm_frac"] = h.get("frac")
            cpu = c.get("cpu_baseline")
            e["cpu_baseline"] = None if not cpu else cpu.get("value")
            cfgs[name] = e
        out["configs"] = cfgs
    p = full.get("parity")
    if p:
        out["parity"] = {k: p[k] for k in ("tolerance", "pass", "max_rel_err", "condition_map_bitwise") if k in p}
        out["parity"]["case"] = "cvae_c4_full"
    if full.get("detail_file"):
        out["detail_file"] = full["detail_file"]
    s = json.dumps(out, separators=(",", ":"))
    if len(s) > STDOUT_LINE_LIMIT:  # never lose the headline: drop the per-config block first
        out.pop("configs", None)
        s = json.dumps(out, separators=(",", ":"))
    return s


def write_detail(full, path):
    """the full record (every roofline table, note and PMC detail) to `path`; returns the path written (None when it
    could not be). stderr gets one readable line per config and pass."""
    for name, c in [(full.get("config", {}).get("model", "head"), full)] + list((full.get("configs") or {}).items()):
        r = c.get("roofline") or {}
        bp = " ".join(f"{k}={v['TFLOP/s']}" for k, v in (r.get("by_pass") or {}).items())
        print(f"[bench detail] {name}: {c.get('value')} img/s, {c.get('ms_per_step')} ms/step, frac {r.get('frac')} of "
              f"{r.get('peak')} {r.get('unit')}; TF/s by pass: {bp}", file=sys.stderr, flush=True)
    try:
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(path, "w") as f:
            json.dump(full, f, indent=1)
        return path
    except OSError:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default=None, choices=sorted(CONFIGS),
                    help="one config alone (default: c4; with --full at N=1 also the c1 / c2 / c3 / c5 / c4x block and "
                         "the parity block; c4x = c4 in exact fp32)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: the instrumented step's rooflines, the CPU baseline, "
                         "the other configs and the parity block, and the detail file (off: set up, warm up, time the "
                         "steps, print the line)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the last timed step's outputs (loss, model outputs, a sample of the updated "
                         "parameters) as DIR/<name>.npy, float32")
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch override (default: config)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-kernel-timing", action="store_true", help="with --full: skip the instrumented step")
    ap.add_argument("--no-parity", action="store_true", help="with --full: skip the parity block")
    ap.add_argument("--detail", action="store_true", help="per-shape GEMM launch timings on stderr")
    ap.add_argument("--eager", action="store_true", help="launch every kernel from Python (no HIP-graph replay)")
    ap.add_argument("--detail-out", default=os.path.join("bench_out", "bench_detail.json"),
                    help="with --full: where the full record (all roofline tables and notes) is written; stdout carries "
                         "the compact line")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus))
    if env_world is not None and int(env_world) != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={env_world} ranks")

    from medvae_disentangled_multimodal_amd import ddp

    # MVAE_BENCH_BACKEND / MVAE_BENCH_ONE_DEVICE: rehearse the multi-rank bench on a 1-GPU box (gloo transport,
    # every rank on cuda:0); the production path is RCCL with one rank per GPU
    rank, world, local = ddp.init_from_env(os.environ.get("MVAE_BENCH_BACKEND"))
    if os.environ.get("MVAE_BENCH_ONE_DEVICE"):
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    head = args.config or "c4"
    full = args.full and args.config is None and world == 1 and args.batch is None
    line = run_config(head, args, rank, world, dev, dump=args.dump_outputs)
    extra, parity = None, None
    if full:  # the other BASELINE configs on the same box, same clock (their own images/s; not summed)
        extra = {}
        for c in ("c1", "c2", "c3", "c5", "c4x"):
            # c4x (exact fp32, ~4x the 3xBF16 step time): a short timed region, and the c4 line's CPU baseline (same
            # model and step on the CPU)
            short = c == "c4x"
            # the graph-replayed 28x28 configs step in 8-30 ms: at least 50 timed steps, so one host hiccup in a
            # ~0.1 s timed region cannot move their line (measured once: c1 2,695 vs 3,580 img/s on a rerun)
            fast = c in ("c1", "c2", "c3")
            r = run_config(c, args, rank, world, dev, want_cpu=not short,
                           steps=min(args.steps, 4) if short else max(args.steps, 50) if fast else None,
                           warmup=min(args.warmup, 1) if short else None)
            if short:
                r["cpu_baseline"] = dict(line["cpu_baseline"] or {}, note="the c4 line's baseline (same model / step)") \
                    if line["cpu_baseline"] else None
            extra[c] = {k: r[k] for k in ("value", "unit", "ms_per_step", "steps", "warmup", "dtype", "config",
                                          "loss", "roofline", "cpu_baseline")}
            print(f"[bench] {c}: {r['value']} images/s ({r['ms_per_step']} ms/step)", file=sys.stderr, flush=True)
        if not args.no_parity:
            parity = parity_block(dev)

    if rank == 0:
        out = {"metric": METRIC_C4 if head == "c4" else f"training images/sec (whole node), config {head}",
               "value": line["value"], "unit": "images/s", "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "ms_per_step": line["ms_per_step"], "higher_is_better": True,
               "scaling": "weak", "vs_baseline": None, "dtype": line["dtype"],
               "data": "synthetic (MedMNIST-shaped, resident in HBM; random-init weights)",
               "config": line["config"], "loss": line["loss"], "roofline": line["roofline"],
               "cpu_baseline": line["cpu_baseline"]}
        if extra is not None:
            out["configs"] = extra
        if parity is not None:
            out["parity"] = parity
        if args.full:
            out["detail_file"] = write_detail(out, args.detail_out)
        print(compact_line(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
