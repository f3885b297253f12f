"""bench.py --dump-outputs: the arrays of the last timed step are written as float32 .npy files, outputs past the
sample limits as samples at the same seeded positions on every run (CPU-only: the writer runs on a stand-in module)."""
import types

import numpy as np
import torch

import bench


def _module(scale=1.0):
    g = torch.Generator().manual_seed(3)
    model = torch.nn.ModuleDict({"b": torch.nn.Linear(5, 3), "a": torch.nn.Conv2d(3, 70, 9)})  # a.weight: 17,010 > 2^12
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * scale)
    outs = {"reconstruction": torch.randn(bench.DUMP_SAMPLE + 77, generator=g).double() * scale,
            "mean": torch.randn(2, 4, 3, 3, generator=g) * scale, "posterior": object(),
            "indices": torch.arange(4)}
    return types.SimpleNamespace(model=model, _last_outputs=outs)


def test_dump_outputs_writes_float32_arrays_and_fixed_samples(tmp_path):
    mod = _module()
    loss = torch.tensor(1.25, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "a"), mod, loss)
    bench.dump_outputs(str(tmp_path / "b"), mod, loss)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["loss.npy", "mean.npy", "params_after_step.npy", "reconstruction.npy"]
    a = {n: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert a[n].dtype == np.float32 and a[n].ndim == 1
        assert np.array_equal(a[n], np.load(tmp_path / "b" / n)), n  # same positions, same values
    assert a["loss.npy"].tolist() == [1.25]
    assert np.array_equal(a["mean.npy"], mod._last_outputs["mean"].reshape(-1).numpy())  # small: stored whole
    assert a["reconstruction.npy"].size == bench.DUMP_SAMPLE
    # parameters in name order: a.bias (70, whole), a.weight (sampled), b.bias (3), b.weight (15)
    sd = dict(mod.model.named_parameters())
    assert a["params_after_step.npy"].size == 70 + bench.DUMP_PARAM_SAMPLE + 3 + 15
    assert np.array_equal(a["params_after_step.npy"][:70], sd["a.bias"].detach().numpy())
    assert np.array_equal(a["params_after_step.npy"][-15:], sd["b.weight"].detach().reshape(-1).numpy())
    # a sample is values of the tensor at fixed positions: scaling the tensor scales the stored sample
    bench.dump_outputs(str(tmp_path / "c"), _module(2.0), loss)
    for n in ("reconstruction.npy", "params_after_step.npy"):
        assert np.array_equal(np.load(tmp_path / "c" / n), 2.0 * a[n]), n
