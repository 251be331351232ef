"""bench.py --dump-outputs: what dump_outputs writes -- float arrays, within the byte limit, the same from run to run
(CPU only: a small module's gradients stand in for the benchmark model's)."""
import os

import numpy as np
import torch

import bench


def _module_with_gradients():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(300, 200), torch.nn.Linear(200, 1))
    loss = m(torch.randn(4, 300)).square().mean()
    loss.backward()
    return m, loss


def test_dump_outputs_stays_under_the_limit_and_samples_the_same_entries_every_run(tmp_path, monkeypatch):
    m, loss = _module_with_gradients()
    limit = 100_000                          # the 240 000-byte weight gradient must be sampled, the rest fits whole
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", limit)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), loss, m)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(["loss.npy"] + [f"grad.{n}.npy" for n, _ in m.named_parameters()])
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64), (n, a.dtype)
        np.testing.assert_array_equal(a, b, err_msg=n)
        total += a.nbytes
    assert total <= limit
    np.testing.assert_allclose(np.load(tmp_path / "a" / "loss.npy"), [loss.item()], rtol=1e-7)
    for n, p in m.named_parameters():
        got = np.load(tmp_path / "a" / f"grad.{n}.npy")
        want = p.grad.numpy()
        if want.nbytes <= limit // 4:
            np.testing.assert_array_equal(got, want, err_msg=n)
        else:
            assert got.ndim == 1 and 0 < got.size < want.size and np.isin(got, want.reshape(-1)).all(), n
