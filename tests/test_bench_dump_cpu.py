"""bench.py --dump-outputs: the files it writes for a step's outputs (CPU, a stand-in model)."""
import os
import types

import numpy as np
import torch

import bench


def _step():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.BatchNorm2d(8), torch.nn.ReLU(), torch.nn.Conv2d(8, 4, 1))
    loss = m(torch.randn(2, 3, 6, 6)).square().mean()
    loss.backward()
    return m, {"loss": loss.detach(), "log_vars": {"depth/scale 0": 0.25, "layout": 0.5, "loss": 0.75}}


def test_dump_outputs_files(tmp_path):
    m, out = _step()
    bench.dump_outputs(str(tmp_path), types.SimpleNamespace(model=m), out, lambda s: None)
    got = {f: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["buffers.npy", "grads.npy", "log_vars.depth_scale_0.npy", "log_vars.layout.npy", "loss.npy",
                           "params.npy"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["loss.npy"][0] == float(out["loss"]) and got["log_vars.layout.npy"][0] == 0.5
    params = [p for p in m.parameters()]
    assert np.array_equal(got["params.npy"], torch.cat([p.detach().reshape(-1) for p in params]).numpy())
    assert np.array_equal(got["grads.npy"], torch.cat([p.grad.reshape(-1) for p in params]).numpy())
    assert np.array_equal(got["buffers.npy"], torch.cat([m[1].running_mean, m[1].running_var]).numpy())


def test_dump_outputs_samples_long_vectors(tmp_path, monkeypatch):
    m, out = _step()
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), types.SimpleNamespace(model=m), out, lambda s: None)
    a, b = np.load(tmp_path / "a" / "params.npy"), np.load(tmp_path / "b" / "params.npy")
    full = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).numpy()
    idx = np.unique(np.random.default_rng(0).integers(0, full.size, 100))
    assert full.size > 100 and np.array_equal(a, b) and np.array_equal(a, full[idx])
