"""bench.py's host-side surface: the --full / --dump-outputs options and the dump's layout
(float32 .npy files, a fixed seeded sample of every large parameter tensor)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "3", "--warmup", "1")
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 3, 1)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d", "--no-cpu-baseline")
    assert a.full and a.dump_outputs == "d" and a.no_cpu_baseline and not a.no_roofline


def _model():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(400, 200), torch.nn.Linear(200, 7))   # 80000 > sample
    x = torch.randn(4, 400)
    logits = m(x)
    loss = logits.square().sum()
    loss.backward()
    m[1].bias.grad = None          # a parameter the step left without a gradient
    return m, loss, logits


def test_dump_outputs_layout(tmp_path):
    m, loss, logits = _model()
    d = str(tmp_path / "a" / "b")     # created on demand
    bench.dump_outputs(d, loss, logits, m)
    assert sorted(os.listdir(d)) == ["grads.npy", "logits.npy", "loss.npy", "params.npy"]
    arr = {n[:-4]: np.load(os.path.join(d, n)) for n in os.listdir(d)}
    assert all(v.dtype == np.float32 for v in arr.values())
    assert arr["loss"].shape == (1,) and arr["loss"][0] == np.float32(loss.item())
    assert np.array_equal(arr["logits"], logits.detach().numpy())
    n = bench.DUMP_SAMPLE + 200 + 200 * 7 + 7
    assert arr["grads"].shape == arr["params"].shape == (n,)
    # small tensors are whole and in named_parameters() order; the missing gradient is zeros
    s = bench.DUMP_SAMPLE
    assert np.array_equal(arr["params"][s:s + 200], m[0].bias.detach().numpy())
    assert np.array_equal(arr["grads"][s + 200:s + 1600], m[1].weight.grad.reshape(-1).numpy())
    assert not arr["grads"][-7:].any()
    # the large tensor: the same sorted, seeded indices for params and grads
    idx = np.sort(np.random.default_rng(0).choice(80000, s, replace=False))
    assert np.array_equal(arr["params"][:s], m[0].weight.detach().reshape(-1).numpy()[idx])
    assert np.array_equal(arr["grads"][:s], m[0].weight.grad.reshape(-1).numpy()[idx])


def test_dump_outputs_repeats(tmp_path):
    for name in ("x", "y"):
        m, loss, logits = _model()
        bench.dump_outputs(str(tmp_path / name), loss, logits, m)
    for f in ("grads", "params", "logits", "loss"):
        assert np.array_equal(np.load(tmp_path / "x" / (f + ".npy")),
                              np.load(tmp_path / "y" / (f + ".npy")))
