"""bench.py --dump-outputs: the files are float64, stay within the budget, and a sampled dump is the same rows every time."""
import numpy as np

import bench
from conftest import GOLDEN
from vasp_amd.mesh import FsiMesh

HIST = [(1.0, 1.0, True, 12, 1e-3), (1e-4, 1e-4, False, 9, 2e-3)]


def _state(mesh):
    return np.arange(6 * mesh.num_nodes + mesh.num_vertices, dtype=np.float64)


def test_a_small_state_is_written_whole(tmp_path):
    mesh = FsiMesh.read(GOLDEN / "cylinder" / "cylinder.h5")
    x = _state(mesh)
    info = bench.dump_outputs(tmp_path, x, mesh, HIST)
    assert not info["sampled"]
    d, v, p = mesh.split(x)
    for name, ref in (("displacement", d), ("velocity", v), ("pressure", p), ("newton_history", np.array(HIST, dtype=float))):
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, ref)


def test_a_large_state_is_a_fixed_sample_within_the_budget(tmp_path, monkeypatch):
    mesh = FsiMesh.read(GOLDEN / "cylinder" / "cylinder.h5")
    x = _state(mesh)
    budget = x.nbytes // 3
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", budget)
    info = [bench.dump_outputs(tmp_path / str(i), x, mesh, HIST) for i in range(2)]
    assert info[0]["sampled"] and info[0]["arrays"] == info[1]["arrays"]
    assert sum(f.stat().st_size for f in (tmp_path / "0").iterdir()) <= budget
    d = np.load(tmp_path / "0" / "displacement.npy")
    v = np.load(tmp_path / "0" / "velocity.npy")
    nodes = d[:, 0] / 3                                  # x[i] = i: the rows name the nodes they came from
    assert np.all(np.diff(nodes) > 0) and np.array_equal(v[:, 0] - 3 * mesh.num_nodes, d[:, 0])
    for f in (tmp_path / "0").iterdir():
        assert np.array_equal(np.load(f), np.load(tmp_path / "1" / f.name))
