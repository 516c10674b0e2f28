"""``--hi-pass-tensor`` without a GPU (vasp_amd/hi_pass_tensor.py): the options, the refusals, the six-to-nine expansion, the
files of the writer, the host restatement of the principal-amplitude rule, and the run class on a host stand-in."""
import contextlib
import io
import json
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN
from vasp_amd import hi_pass as hp
from vasp_amd import hi_pass_tensor as hpt

CYL = GOLDEN / "cylinder" / "cylinder.h5"


def test_options_from_the_command_line_a_config_file_and_new_arguments(tmp_path):
    from vasp_amd.monolithic import SESSIONS, parse
    a = parse(["--hi-pass-tensor", "strain", "stress", "--hi-pass-tensor-window", "8", "--hi-pass-bands", "0", "200", "--hi-pass-amplitude"])
    assert a["hi_pass_tensor"] == ["strain", "stress"] and a["hi_pass_tensor_window"] == 8 and a["hi_pass_amplitude"] is True
    assert "hi_pass" not in a and hp.bands(a) == [(0.0, 200.0)]
    assert hpt.quantities({"hi_pass_tensor": ["stress", "strain"]}) == ["strain", "stress"] and hpt.quantities({"hi_pass_tensor": "stress"}) == ["stress"]
    assert hpt.window({}) == 50 and hpt.window(a) == 8 and hp.bands({}) == [(25.0, 1000.0)]
    assert not any(k.startswith("hi_pass_tensor") for k in parse([]))
    cfg = tmp_path / "run.cfg"
    cfg.write_text('hi_pass_tensor = ["strain"]\nhi-pass-tensor-window = 16\n')
    c = parse(["-c", str(cfg)])
    assert c["hi_pass_tensor"] == ["strain"] and c["hi_pass_tensor_window"] == 16
    n = parse(["--new-arguments", "hi_pass_tensor=['stress']", "hi_pass_tensor_window=12"])
    assert n["hi_pass_tensor"] == ["stress"] and n["hi_pass_tensor_window"] == 12
    for bad in (["d"], ["strain", "p"], ["Stress"]):
        with pytest.raises(SystemExit, match="strain and / or stress"):
            hpt.quantities({"hi_pass_tensor": bad})
    # --hi-pass itself is as it was
    with pytest.raises(SystemExit, match="d, v and / or p"):
        hp.quantities({"hi_pass": ["strain"]})
    assert set(hp.VIZ_TYPE) == {"d", "v", "p"}
    rows = [r for r in SESSIONS if r[0] == "hi_pass_tensor"]
    assert rows == [("hi_pass_tensor", "hi_pass_tensor", "hi_pass_tensor_refusal", "HiPassTensorRun", "hi_pass_begin_cells")]
    assert [r[0] for r in SESSIONS].index("hi_pass_tensor") == [r[0] for r in SESSIONS].index("hi_pass") + 1


def _refusal(extra, world=1, cls=None, tensor=("strain",)):
    from vasp_amd.monolithic import parameters
    with contextlib.redirect_stdout(io.StringIO()):
        _, _, v = parameters(["-p", "cylinder", "--hi-pass-tensor", *tensor, "--verbose", "False", *extra])
    return hpt.hi_pass_tensor_refusal(v, world, cls)


class _NoCells:
    """A backend class without the device call."""

    def __init__(self, desc):
        raise AssertionError("refused before a backend is built")


def test_each_refusal_has_its_message(tmp_path, monkeypatch):
    ok = ["-dt", "0.001", "-T", "0.039", "--save-step", "1"]           # 40 frames: the loop steps while t <= T
    assert _refusal(ok) == "" and _refusal(ok, tensor=("strain", "stress")) == ""
    assert "cannot be used with --restart-folder" in _refusal(ok + ["--restart-folder", str(tmp_path)])
    assert "one rank only (WORLD_SIZE > 1)" in _refusal(ok, world=2)
    assert "needs --save-step" in _refusal(["-dt", "0.001", "-T", "0.04", "--save-step", "0"])
    msg = _refusal(["-dt", "0.001", "-T", "0.032", "--save-step", "1"])
    assert msg.startswith("--hi-pass-tensor: the run saves 33 frames") and "padlen + 1 = 34" in msg
    assert _refusal(["-dt", "0.001", "-T", "0.032", "--save-step", "1", "--hi-pass-bands", "0", "200"]) == ""       # low-pass: 19
    assert "saves 40 frames, fewer than the window of 50 (--hi-pass-tensor-window)" in _refusal(ok + ["--hi-pass-amplitude"])
    assert _refusal(ok + ["--hi-pass-amplitude", "--hi-pass-tensor-window", "40"]) == ""
    assert _refusal(ok + ["--hi-pass-amplitude", "--hi-pass-window", "40"]) != ""          # the window of d, v, p is another option
    assert "must be at least 1" in _refusal(ok + ["--hi-pass-tensor-window", "0"])
    assert "hi_pass_begin_cells (_NoCells has none)" in _refusal(ok, cls=_NoCells)
    with pytest.raises(SystemExit, match="strain and / or stress"):
        _refusal(ok, tensor=("v",))
    # the options that the reference applies to d, v, p only: refused on their own, accepted beside --hi-pass
    two = ["--hi-pass-bands", "25", "200", "210", "400"]
    for extra, name in ((["--hi-pass-multiband"] + two, "--hi-pass-multiband"), (["--hi-pass-stride", "2"], "--hi-pass-stride"),
                        (["--hi-pass-start-time", "0.002"], "--hi-pass-start-time"), (["--hi-pass-end-time", "0.03"], "--hi-pass-end-time"),
                        (["--hi-pass-point-ids", "3"], "--hi-pass-point-ids")):
        msg = _refusal(ok + extra)
        assert msg.startswith(name) and "act on d, v and p" in msg, extra
    assert _refusal(ok + ["--hi-pass", "v", "--hi-pass-point-ids", "3", "--hi-pass-end-time", "0.038"]) == ""
    # through the driver: refused before anything is built (no results folder appears), on every rank
    from vasp_amd import monolithic
    argv = ["-p", "cylinder", "-dt", "0.001", "-T", "0.01", "--save-step", "1", "--verbose", "False", "--folder", str(tmp_path / "r"),
            "--hi-pass-tensor", "stress", "--new-arguments", f"mesh_path={CYL}"]
    with pytest.raises(SystemExit, match="hi_pass_begin_cells"):
        monolithic.run(argv, backend_factory=_NoCells)
    assert not (tmp_path / "r").exists()
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    with pytest.raises(SystemExit, match="one rank only"):
        monolithic.run(argv, backend_factory=_NoCells)


def test_six_rows_expand_to_the_nine_entries():
    # [REF create_hi_pass_viz.py:254-263]: columns 0..8 <- components 0, 1, 5, 1, 2, 3, 5, 3, 4 of (11, 12, 22, 23, 33, 31)
    assert hpt.EXPAND == (0, 1, 5, 1, 2, 3, 5, 3, 4)
    rows = np.array([[11.0, 12.0, 22.0, 23.0, 33.0, 31.0], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]])
    nine = hpt.expand(rows)
    assert nine.shape == (2, 9)
    assert nine[0].tolist() == [11.0, 12.0, 31.0, 12.0, 22.0, 23.0, 31.0, 23.0, 33.0]
    assert nine[1].tolist() == [1.0, 2.0, 6.0, 2.0, 3.0, 4.0, 6.0, 4.0, 5.0]
    T = nine.reshape(2, 3, 3)
    assert np.array_equal(T, np.swapaxes(T, 1, 2))
    assert np.array_equal(hpt.expand(rows.reshape(-1)), nine)            # a flat frame of the session
    # the rows are entries 0, 1, 4, 5, 8, 6 of a symmetric tensor: expansion gives it back
    full = np.arange(9.0).reshape(3, 3)
    full = full + full.T
    assert np.array_equal(hpt.expand(full.reshape(9)[[0, 1, 4, 5, 8, 6]]).reshape(3, 3), full)


def _datasets(g, prefix=""):
    from vasp_amd.h5lite import Dataset
    out = {}
    for k in g.keys():
        if isinstance(g[k], Dataset):
            out[prefix + k] = np.asarray(g[k].data)
        else:
            out.update(_datasets(g[k], prefix + k + "/"))
    return out


def test_writer_files(tmp_path):
    from vasp_amd.h5lite import read_h5
    from vasp_amd.mesh import FsiMesh
    from vasp_amd.stress_strain import StressStrainWriter, solid_cells, solid_submesh
    mesh = FsiMesh.read(CYL)
    cells = solid_cells(mesh, 2)[:7]
    geometry, topology = solid_submesh(mesh, cells)
    n, nv = len(cells), len(geometry)
    rng = np.random.default_rng(3)
    frames = 1e-4 * rng.standard_normal((3, 4 * n, 6))
    w = hpt.TensorWriter(tmp_path / "Visualization_hi_pass", geometry, topology)
    viz = "GreenLagrangeStrain_25_to_1000"
    w.write_series(viz, (hpt.expand(f) for f in frames), 3, 9, 0.002, 0.0)
    mag = np.abs(rng.standard_normal((3, 4 * n)))
    w.write_series(viz + "_max_principal_amplitude", iter(mag), 3, 1, 0.002, 0.0)
    with pytest.raises(ValueError, match="expected 4"):
        w.write_series("x", iter(mag), 4, 1, 0.002, 0.0)
    # the dof-info of the StressStrain files of the same sub-mesh
    ss = StressStrainWriter(tmp_path / "StressStrain", geometry, topology)
    ss.write_frame(dict(TrueStress=np.zeros((n, 4, 3, 3)), GreenLagrangeStrain=np.zeros((n, 4, 3, 3)), MaxPrincipalStress=np.zeros((n, 4)),
                        MaxPrincipalStrain=np.zeros((n, 4))), 0.001)
    ss.close()
    info = ("cell_dofs", "cells", "mesh/geometry", "mesh/topology", "x_cell_dofs")
    for name, src, ncomp, data in ((viz, "GreenLagrangeStrain", 9, np.stack([hpt.expand(f) for f in frames])),
                                   (viz + "_max_principal_amplitude", "MaxPrincipalStrain", 1, mag)):
        d = _datasets(read_h5(tmp_path / "Visualization_hi_pass" / f"{name}.h5"))
        want = _datasets(read_h5(tmp_path / "StressStrain" / f"{src}.h5"))
        assert sorted(d) == sorted([f"{name}/{name}_{k}/vector" for k in range(3)] + [f"{name}/{name}_0/{i}" for i in info])
        for k in range(3):
            v = d[f"{name}/{name}_{k}/vector"]
            assert v.dtype == np.float32 and v.shape == (n * 4 * ncomp, 1)
            assert np.array_equal(v[:, 0], data[k].reshape(-1).astype(np.float32))
        for i in info:
            a, b = d[f"{name}/{name}_0/{i}"], want[f"{src}/{src}_0/{i}"]
            assert a.dtype == b.dtype and np.array_equal(a, b), (name, i)
        text = (tmp_path / "Visualization_hi_pass" / f"{name}.xdmf").read_text()
        att = "Tensor" if ncomp == 9 else "Scalar"
        assert text.startswith(f'<?xml version="1.0"?>\n<Xdmf Version="3.0">\n  <Domain>\n    <Grid GridType="Collection" CollectionType="Temporal" Name="{name}">\n')
        assert text.endswith("      </Grid>\n    </Grid>\n  </Domain>\n</Xdmf>\n") and text.count("<Grid Name=") == 3
        assert f'<Topology NumberOfElements="{n}" TopologyType="Tetrahedron" NodesPerElement="4">' in text
        assert f'<DataItem Dimensions="{n} 4" NumberType="UInt" Format="HDF">{name}.h5:{name}/{name}_0/mesh/topology</DataItem>' in text
        assert f'<DataItem Dimensions="{nv} 3" Format="HDF">{name}.h5:{name}/{name}_0/mesh/geometry</DataItem>' in text
        assert [float(x) for x in __import__("re").findall(r'<Time Value="(.+?)" />', text)] == [0.0, 0.002, 0.004]
        assert f'ElementFamily="DG" ElementDegree="1" ElementCell="tetrahedron" Name="{name}" Center="Other" AttributeType="{att}">' in text
        assert f'<DataItem Dimensions="{4 * n * ncomp} 1" NumberType="Float" Format="HDF">{name}.h5:{name}/{name}_2/vector</DataItem>' in text
        assert f'<DataItem Dimensions="{4 * n * ncomp} 1" NumberType="UInt" Format="HDF">{name}.h5:{name}/{name}_0/cell_dofs</DataItem>' in text
        assert f'<DataItem Dimensions="{n + 1} 1" NumberType="UInt" Format="HDF">{name}.h5:{name}/{name}_0/x_cell_dofs</DataItem>' in text
    # the table: the header and the 13 columns of --hi-pass
    table = np.stack([hp.amplitude_row(k * 0.002, mag[k], mag[k].max(), int(np.argmax(mag[k]))) for k in range(3)])
    w.write_table(viz, table)
    lines = (tmp_path / "Visualization_hi_pass" / f"{viz}.csv").read_text().splitlines()
    assert lines[0] == "# " + hp.CSV_HEADER and len(lines) == 4
    got = np.loadtxt(tmp_path / "Visualization_hi_pass" / f"{viz}.csv", delimiter=",")
    assert got.shape == (3, 13) and np.array_equal(got, table) and np.array_equal(got[:, 12], mag.argmax(axis=1))
    assert not list((tmp_path / "Visualization_hi_pass").glob("*.png"))


def test_principal_amplitude_rule_on_the_host():
    """The shortcut, then the closed form.  Distance to LAPACK: tests/test_post_oracle.py holds kopp_max_eigenvalue to 1e-10
    of the tensor's largest entry on well-scaled symmetric tensors; entries of 1e-3 are far above get_eig's perturbation
    thresholds (p ~ 1e-6 against 1e-16, q ~ 1e-9 against 1e-24), so the same distance holds here."""
    from oracle.post_oracle import kopp_max_eigenvalue
    rng = np.random.default_rng(17)
    amp = 1e-3 * rng.standard_normal((400, 6))
    amp[::5] *= 1e-6                                    # every entry near 1e-9: the shortcut
    amp[3::5] = 0.0
    amp[4, :] = [9.9e-9, -9.9e-9, 0.0, 5e-9, 9.99e-9, 1e-10]
    amp[9, :] = [9.9e-9, -9.9e-9, 0.0, 5e-9, 1e-8, 1e-10]       # one entry at the threshold: strictly below is required
    got = hpt.principal_amplitude(amp, kopp_max_eigenvalue)
    T = hpt.expand(amp).reshape(-1, 3, 3)
    small = (np.abs(T) < 1e-8).all(axis=(1, 2))
    assert small[::5].all() and small[3::5].all() and small[4] and not small[9] and 150 < small.sum() < 170
    assert got.shape == (400,) and not got[small].any() and np.array_equal(np.signbit(got[small]), np.zeros(small.sum(), bool))
    assert np.array_equal(got[~small], kopp_max_eigenvalue(T[~small])) and got[9] != 0.0
    ref = np.linalg.eigvalsh(T)[:, -1]
    big = ~small & (np.abs(T).max(axis=(1, 2)) > 1e-6)
    rel = np.abs(got[big] - ref[big]) / np.abs(T[big]).max(axis=(1, 2))
    print(f"closed form vs eigvalsh on {big.sum()} tensors of scale 1e-3: largest distance {rel.max():.3e} of the largest entry")
    assert big.sum() > 200 and rel.max() < 1e-10
    assert hpt.principal_amplitude(amp.reshape(100, 4, 6), kopp_max_eigenvalue).shape == (400,)


class _HostCells:
    """``HipBackend.hi_pass_*`` of the tensor quantities on the host: frames of noise instead of the cell arithmetic, the
    filter and the RMS of ``HostBandSession``, the principal amplitude by ``principal_amplitude``."""

    def __init__(self):
        self.sessions = {}

    def hi_pass_begin_cells(self, q, cells, capacity):
        self.sessions[q], self.dofs = hp.HostBandSession(6, capacity), 4 * len(cells)

    def hi_pass_sample(self, q):
        rng = np.random.default_rng(len(self.sessions[q].raw) + (100 if q == "stress" else 0))
        self.sessions[q].sample(1e-4 * rng.standard_normal((self.dofs, 6)))

    def hi_pass_filter(self, q, *args):
        self.sessions[q].filter(*args)

    def hi_pass_amplitude(self, q, window):
        self.sessions[q].amplitude(window)

    def hi_pass_fetch(self, q, what, k, with_max=False):
        from oracle.post_oracle import kopp_max_eigenvalue
        s = self.sessions[q]
        if what in ("raw", "filtered"):
            return s.fetch(what, k)
        mag = hpt.principal_amplitude(s.amp[k], kopp_max_eigenvalue)
        out = mag if what == "magnitude" else s.amp[k]
        return (out, float(mag.max()), int(np.argmax(mag))) if with_max else out

    def hi_pass_export(self, q, first, count):
        return self.sessions[q].export(first, count)

    def hi_pass_import(self, q, frames):
        self.sessions[q].import_(np.asarray(frames).reshape(len(frames), -1, 6))

    def hi_pass_end(self, q):
        self.sessions.pop(q)


def test_the_run_class_writes_every_band_and_goes_through_a_checkpoint(tmp_path):
    """``HiPassTensorRun`` on a host stand-in for the device calls: what it writes per band, its log lines, and that a run
    which saves after 11 frames and is continued from the saved state writes the bytes of one that was not split."""
    from conftest import prepare_case
    from vasp_amd.h5lite import read_h5
    extra = ["save_step=1", "hi_pass_tensor=['strain','stress']", "hi_pass_bands=[0,200,25,400]", "hi_pass_amplitude=True",
             "hi_pass_tensor_window=8"]

    def run(folder, split):
        ns = prepare_case("cylinder", CYL, folder, T="0.0235", extra=extra)[0]
        session = hpt.HiPassTensorRun(_HostCells(), ns["mesh"], ns)
        lines = []
        for k in range(24):
            session.sample((k + 1) * 1e-3, None)
            if split and k == 10:
                results = Path(ns["results_folder"])
                hp.save_sessions([session], results, 0.011, 10)
                (results / "Checkpoint" / "default_variables.json").write_text(json.dumps(dict(t=0.011, counter=10)))
                entry = json.loads((hp.sessions_folder(results) / hp.MANIFEST).read_text())["sessions"]["hi_pass_tensor"]
                assert entry["frames"] == 11 and sorted(entry["quantities"]) == ["strain", "stress"]
                assert entry["quantities"]["stress"]["rows"] == 24 * len(session.cells)
                assert (hp.sessions_folder(results) / "hi_pass_tensor_strain.f64").stat().st_size == 8 * 24 * len(session.cells) * 11
                for s in session.sessions.values():
                    s.end()
                session = hpt.HiPassTensorRun(_HostCells(), ns["mesh"], dict(ns, restart_folder=str(results)))
                assert session.frames == session.saved == 11 and len(session.times) == 11
        session.finish(lines.append)
        return Path(ns["results_folder"]) / "Visualization_hi_pass", lines, len(session.cells)

    whole, lines, n = run(tmp_path / "whole", False)
    split, lines_split, _ = run(tmp_path / "split", True)
    assert [line.replace(str(tmp_path / "split"), "") for line in lines_split] == [line.replace(str(tmp_path / "whole"), "") for line in lines]
    assert lines[-1].startswith("Hi-pass tensors of 24 frames (strain, stress) written to ")
    assert sum("25_to_400: 24 frames recorded, the filter needs more than 33: nothing written" in line for line in lines) == 2
    names = sorted(p.name for p in whole.iterdir())
    assert names == sorted(f"{v}_0_to_200{s}" for v in hpt.VIZ_TYPE.values()
                           for s in (".csv", ".h5", ".xdmf", "_amplitude.h5", "_amplitude.xdmf", "_max_principal_amplitude.h5",
                                     "_max_principal_amplitude.xdmf"))
    for name in names:
        if name.endswith(".h5"):
            a, b = _datasets(read_h5(whole / name)), _datasets(read_h5(split / name))
            assert sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a), name
            viz = name[:-3]
            assert a[f"{viz}/{viz}_23/vector"].shape == (4 * n * (1 if "principal" in viz else 9), 1)
        else:
            assert (whole / name).read_bytes() == (split / name).read_bytes(), name
    # low-pass: the amplitude is the filtered tensor itself [REF create_hi_pass_viz.py:229-230]
    f = _datasets(read_h5(whole / "TrueStress_0_to_200.h5"))["TrueStress_0_to_200/TrueStress_0_to_200_5/vector"]
    a = _datasets(read_h5(whole / "TrueStress_0_to_200_amplitude.h5"))["TrueStress_0_to_200_amplitude/TrueStress_0_to_200_amplitude_5/vector"]
    assert np.array_equal(f, a)
    # a state recorded on other cells is refused
    ns = prepare_case("cylinder", CYL, tmp_path / "other", T="0.0235", extra=extra)[0]
    other = dict(ns, restart_folder=str(split.parent), dx_s_id=[2, 1])
    with pytest.raises(SystemExit, match="recorded otherwise than this run would record, it differs in rows .*cells"):
        hpt.HiPassTensorRun(_HostCells(), ns["mesh"], other)
