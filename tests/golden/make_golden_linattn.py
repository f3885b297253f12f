#!/usr/bin/env python3
"""Golden vectors of the linear-attention path (`use_linear_attn` / `attn_type="linear"`) from the REFERENCE
implementation (run where the reference checkout is available, like make_golden.py; needs einops).

    python3 -B tests/golden/make_golden_linattn.py

Writes
  linattn_block.npz  for each shape in BLOCK_SHAPES the reference's own LinAttnBlock (src.models.encoder_decoder)
                     with the synthetic weights of weights.py: input, to_qkv / to_out weights, output, and the
                     gradients w.r.t. the input and the three parameters for a fixed upstream gradient. (The
                     n = 784, C = 128 geometry of the kernel tests is left to their float64 restatement: its
                     tensors alone would exceed the size limit of a committed file.)
  linattn_base.npz + .json  one full training step (forward with an injected eps, VAELoss, backward, clip, Adam) of
                     a small BaseVAE with use_linear_attn=True, in the fields make_golden.run_case records for
                     every case: the state-dict names and shapes in order (`params`), the per-tensor (sum, sum of
                     squares) of the reference's initial weights under torch.manual_seed(0)
                     (`seeded_init_torch_seed0`), outputs, loss terms, gradient / post-step checksums and the
                     full gradients listed in the case's `full_grads`.
Only data leaves this script.
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as G  # noqa: E402  (puts the reference on sys.path; nothing runs on import)
from weights import synth_param  # noqa: E402

from src.models.encoder_decoder import LinAttnBlock  # noqa: E402  (the reference)

BLOCK_SHAPES = [(2, 32, 1, 1), (3, 32, 7, 7), (1, 36, 1, 17), (2, 64, 14, 14)]

BASE_CASE = dict(
    cls="BaseVAE",
    kwargs=dict(input_channels=1, latent_dim=4, hidden_channels=32, ch_mult=[1, 2], num_res_blocks=1,
                attn_resolutions=[14], dropout=0.0, resolution=28, use_linear_attn=True),
    batch=4, cond="none",
    loss=dict(type="vae", recon_loss_type="mse", kl_weight=1.0, recon_weight=1.0),
    optimizer=dict(type="adamw", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.999]),
    clip=1.0,
    full_grads=["encoder.conv_in.weight", "encoder.down.1.attn.0.to_qkv.weight", "encoder.mid.attn_1.to_out.weight",
                "decoder.mid.attn_1.to_out.bias", "decoder.up.1.attn.1.to_qkv.weight", "decoder.conv_out.weight"],
)


def tag(shape):
    return "x".join(map(str, shape))


def block_fixtures():
    rec = {}
    for shape in BLOCK_SHAPES:
        b, c, h, w = shape
        t = tag(shape)
        blk = LinAttnBlock(c)
        names = [(k, tuple(v.shape)) for k, v in blk.state_dict().items()]
        assert [k for k, _ in names] == ["to_qkv.weight", "to_out.weight", "to_out.bias"], names
        state = {k: synth_param(f"linattn_block.{t}.{k}", s) for k, s in names}
        blk.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
        rng = np.random.Generator(np.random.PCG64(4242 + c + h * w))
        x = torch.from_numpy(rng.standard_normal(size=shape).astype(np.float32)).requires_grad_()
        go = torch.from_numpy(rng.standard_normal(size=shape).astype(np.float32))
        y = blk(x)
        y.backward(go)
        rec[f"{t}.x"] = x.detach().numpy().copy()
        rec[f"{t}.go"] = go.numpy().copy()
        rec[f"{t}.y"] = y.detach().numpy().copy()
        rec[f"{t}.dx"] = x.grad.numpy().copy()
        for k, p in blk.named_parameters():
            rec[f"{t}.{k}"] = state[k]
            rec[f"{t}.grad.{k}"] = p.grad.numpy().copy()
        print(f"linattn_block {t}: |y|={float(y.detach().norm()):.6f} |dx|={float(x.grad.norm()):.6f}")
    np.savez(os.path.join(HERE, "linattn_block.npz"), **rec)


if __name__ == "__main__":
    torch.set_num_threads(8)
    block_fixtures()
    G.FULL_GRADS["linattn_base"] = BASE_CASE["full_grads"]  # (in this process only: cases.py stays as it is)
    G.run_case("linattn_base", BASE_CASE)
