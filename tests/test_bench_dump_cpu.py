"""bench.py --dump-outputs: what the last timed step computed, as DIR/<name>.npy in float32 / float64 -- the step's losses and
each network's state after the update (a fixed seeded sample when a network is larger than its share of the budget).
CPU: a stand-in trainer with the surface dump_outputs() reads (losses, flush_losses, model.networks)."""
import os
import subprocess
import sys
from collections import defaultdict
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

import bench

REPO = Path(__file__).resolve().parents[1]


def _trainer():
    torch.manual_seed(0)
    nets = {"G": torch.nn.Sequential(torch.nn.Linear(40, 30), torch.nn.BatchNorm1d(30)), "D": torch.nn.Linear(30, 2)}
    losses = {"gan": defaultdict(list), "aux": defaultdict(list)}
    losses["gan"]["D"] += [0.5, 0.25]
    tr = SimpleNamespace(losses=losses, model=SimpleNamespace(networks=nets))
    tr.flush_losses = lambda: losses["aux"]["rec"].append(1.5)         # a deferred loss of the last step
    return tr, nets


def _flat(net):
    return torch.cat([v.flatten().float() for v in net.state_dict().values()]).numpy()


def test_dump_writes_the_last_steps_losses_and_network_state(tmp_path):
    tr, nets = _trainer()
    bench.dump_outputs(tr, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["D_state.npy", "G_state.npy", "loss_aux_rec.npy", "loss_gan_D.npy"]
    assert np.load(tmp_path / "loss_gan_D.npy").dtype == np.float64 and float(np.load(tmp_path / "loss_gan_D.npy")) == 0.25
    assert float(np.load(tmp_path / "loss_aux_rec.npy")) == 1.5
    for name, net in nets.items():
        got = np.load(tmp_path / f"{name}_state.npy")
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, _flat(net))


def test_dump_samples_a_large_network_at_fixed_indices(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_ELEMS", 200)
    tr, nets = _trainer()
    for run in ("a", "b"):
        bench.dump_outputs(tr, str(tmp_path / run))
    full = _flat(nets["G"])
    a, b = np.load(tmp_path / "a" / "G_state.npy"), np.load(tmp_path / "b" / "G_state.npy")
    assert a.shape == (100,) and a.dtype == np.float32
    np.testing.assert_array_equal(a, b)
    assert np.isin(a, full).all()
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total < 200 * 4 + 4 * 1024


def test_the_full_dump_budget_stays_under_64_mb():
    assert bench.DUMP_ELEMS * 4 + 64 * 1024 < 64 * 10 ** 6


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--steps", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=120)
    assert r.returncode == 2 and b"--steps" in r.stderr
