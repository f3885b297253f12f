"""Launch-trace equivalence of the conv dispatch (tests/golden/conv_launch_trace.py): every case of the matrix makes
exactly the library calls recorded in tests/golden/conv_launch_trace.json -- written by the same script on the commit
before ops.plan_conv -- with the same arguments in the same order, and the matrix reaches every conv-family entry
point."""
import json

import pytest
import torch

import conv_launch_trace as T

pytestmark = pytest.mark.gpu

# entry points of the traced families the matrix does not reach, each with its reason (at most five)
NOT_REACHED = {
    "mvae_split_planar": "the planar LDS-DMA operand format is opt-in (MVAE_PLANAR_DMA) and off in every configuration",
    "mvae_split_planar_colsum": "the planar LDS-DMA operand format is opt-in (MVAE_PLANAR_DMA), as above",
    "mvae_conv_weight_transpose_batched": "launched by the trainer's per-step weight prep (prep_flat_weights), not by a conv",
}
FAMILIES = ("mvae_conv", "mvae_winograd", "mvae_split_", "mvae_pack_", "mvae_group_norm_bwd_pack",
            "mvae_group_norm_bwd_split", "mvae_group_norm_bwd_colsum")


@pytest.fixture(scope="module")
def traces():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return T.run_matrix(torch.device("cuda:0"))


@pytest.fixture(scope="module")
def golden():
    with open(T.TRACE_JSON) as f:
        return T.decode(json.load(f))


def test_matrix_is_the_recorded_one(golden):
    assert [k["id"] for k in T.matrix()] == list(golden)


def test_every_trace_is_identical(traces, golden):
    bad = []
    for cid, want in golden.items():
        got = traces[cid]
        if got != want:
            i = next((j for j, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            bad.append(f"{cid}: call {i}: got {got[i] if i < len(got) else None!r}, "
                       f"recorded {want[i] if i < len(want) else None!r}")
    assert not bad, f"{len(bad)} of {len(golden)} cases differ:\n" + "\n".join(bad[:40])


def test_matrix_reaches_every_conv_family_entry_point(traces):
    from medvae_disentangled_multimodal_amd import _lib
    assert len(NOT_REACHED) <= 5
    seen = {"mvae_" + s.split("|")[0] for tr in traces.values() for s in tr}
    family = {n for n in _lib.SIGNATURES if n.startswith(FAMILIES)}
    assert set(NOT_REACHED) <= family
    assert family - seen == set(NOT_REACHED)
