"""Host side of ``--spectrogram wss``, ``--spectrogram-region domain`` and the sound file of ``PointList``
(vasp_amd/spectrogram.py): the rows of the wall shear stress on the boundary mesh of the fluid, their region and sampling
rules, names, defaults and refusals; domain sampling against a restatement of the reference's
``get_domain_ids_specified_region``; the sound file of the host session against scipy's own filter."""
import contextlib
import copy
import io

import numpy as np
import pytest

from test_spectrogram import CYL, REGION, _Stub, _stub_run
from vasp_amd import spectrogram as sp
from vasp_amd.hemodynamics import FACET_VERTS, fluid_boundary_facets


# ---- the rows of the wall shear stress --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wall(cylinder_case):
    """The cylinder's boundary mesh of the fluid: facets, the coordinate of every DG1 dof, and a sphere that holds a part
    of them."""
    ns = cylinder_case[0]
    mesh = ns["mesh"]
    _, cells, local = fluid_boundary_facets(mesh, ns["dx_f_id"])
    xyz = mesh.coords[mesh.tets[cells[:, None], FACET_VERTS[local]]].reshape(-1, 3)       # dof 3 f + k: vertex k of facet f
    centre = xyz[7]
    r = float(np.sort(np.linalg.norm(xyz - centre, axis=1))[len(xyz) // 5])              # about a fifth of the dofs
    return ns, mesh, cells, local, xyz, [*map(float, centre), r]


def _opts(ns, **kw):
    v = dict(ns, spectrogram=["wss"], **{"spectrogram_" + k: x for k, x in kw.items()})
    return v, sp.options(v)


def test_region_dofs_of_a_sphere_and_a_box(wall):
    ns, mesh, cells, local, xyz, sphere = wall
    v, o = _opts(ns, sampling="All", fsi_region=sphere)
    sel = sp.select_nodes(mesh, 1, "wss", v, o)
    expect = np.nonzero(np.linalg.norm(xyz - np.array(sphere[:3]), axis=1) < sphere[3])[0]
    assert 0 < len(expect) < len(xyz) and np.array_equal(sel["ids"], expect)              # All: every region dof once, in order
    assert np.array_equal(sel["facet_cells"], cells) and np.array_equal(sel["facet_local"], local)      # the WHOLE facet list
    assert sel["mu"] == 3.5e-3 and sel["name"] == "wss_all" and sel["case_suffix"] == ""
    # interface_only is ignored: the boundary mesh is sampled by the sphere alone
    vi, oi = _opts(ns, sampling="All", fsi_region=sphere, interface_only=True)
    assert np.array_equal(sp.select_nodes(mesh, 1, "wss", vi, oi)["ids"], expect)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    mid = 0.5 * (lo + hi)
    box = [float(lo[0]) - 1, float(mid[0]), float(lo[1]) - 1, float(hi[1]) + 1, float(mid[2]), float(hi[2]) + 1]
    vb, ob = _opts(ns, sampling="All", region="box", fsi_region=box)
    inside = (xyz[:, 0] > box[0]) & (xyz[:, 0] < box[1]) & (xyz[:, 1] > box[2]) & (xyz[:, 1] < box[3]) & (xyz[:, 2] > box[4]) & (xyz[:, 2] < box[5])
    assert 0 < inside.sum() < len(xyz) and np.array_equal(sp.select_nodes(mesh, 1, "wss", vb, ob)["ids"], np.nonzero(inside)[0])
    # strictly inside: a dof on the sphere itself is out
    d = np.linalg.norm(xyz - np.array(sphere[:3]), axis=1)
    on = [*sphere[:3], float(np.sort(d)[len(xyz) // 5])]
    assert not (d[sp.select_nodes(mesh, 1, "wss", *_opts(ns, sampling="All", fsi_region=on))["ids"]] >= on[3]).any()
    with pytest.raises(SystemExit, match="--spectrogram wss: no nodes found in the specified fsi region"):
        sp.select_nodes(mesh, 1, "wss", *_opts(ns, sampling="All", fsi_region=[10.0, 10.0, 10.0, 1e-3]))


def test_sampling_rules_rows_and_names(wall):
    ns, mesh, cells, local, xyz, sphere = wall
    region = np.nonzero(np.linalg.norm(xyz - np.array(sphere[:3]), axis=1) < sphere[3])[0]
    n = 2 * len(region) + 5                                                   # more draws than the region has: duplicates
    v, o = _opts(ns, fsi_region=sphere, n_samples=n, seed=7)
    sel = sp.select_nodes(mesh, 1, "wss", v, o)
    assert np.array_equal(sel["ids"], np.random.default_rng(7).choice(region, n))
    assert len(np.unique(sel["ids"])) < n and sel["name"] == f"wss_all_n_samples_{n}"
    assert not np.array_equal(sel["ids"], sp.select_nodes(mesh, 1, "wss", *_opts(ns, fsi_region=sphere, n_samples=n, seed=8))["ids"])
    # component all: the three components stacked component-major; x: one; mag: code 3
    assert np.array_equal(sel["dofs"], np.tile(sel["ids"], 3)) and np.array_equal(sel["comps"], np.repeat([0, 1, 2], n))
    for comp, code in (("x", 0), ("y", 1), ("z", 2), ("mag", 3)):
        s = sp.select_nodes(mesh, 1, "wss", *_opts(ns, fsi_region=sphere, n_samples=n, seed=7, component=comp))
        assert np.array_equal(s["dofs"], sel["ids"]) and (s["comps"] == code).all() and s["name"] == f"wss_{comp}_n_samples_{n}"
        assert s["dofs"].dtype == np.int32 and s["comps"].dtype == np.int32
    # PointList: dof ids, refused outside 0 .. 3 nf - 1
    nd = 3 * len(cells)
    pl = sp.select_nodes(mesh, 1, "wss", *_opts(ns, fsi_region=sphere, sampling="PointList", point_ids=[nd - 1, 0, 4], component="mag"))
    assert pl["ids"].tolist() == [nd - 1, 0, 4] and pl["name"] == "wss_mag" and pl["case_suffix"] == f"_PointList_[{nd - 1}, 0, 4]"
    for bad in ([nd], [-1], [0, nd + 7]):
        with pytest.raises(SystemExit, match=rf"ids must be in 0 \.\. {nd - 1}"):
            sp.select_nodes(mesh, 1, "wss", *_opts(ns, fsi_region=sphere, sampling="PointList", point_ids=bad))
    names = sp.file_names(pl["name"], "case" + pl["case_suffix"], np.float64(3.0), -18)
    assert names["spectrogram"] == f"wss_mag_case_PointList_[{nd - 1}, 0, 4]_3.0_windows_thresh-18_spectrogram.csv"
    assert names["psd"] == f"wss_mag_psd_no_filter_case_PointList_[{nd - 1}, 0, 4].csv"


def test_run_side_rows_fingerprint_defaults_and_refusals(wall, tmp_path):
    ns, mesh, cells, local, xyz, sphere = wall
    assert sp.quantities({"spectrogram": ["wss", "p", "d"], "mu_f": 3.5e-3}) == ["d", "p", "wss"]
    assert sp.quantities({"spectrogram": "wss", "mu_f": [3.5e-3, 4e-3]}) == ["wss"]
    with pytest.raises(SystemExit, match="wss where the parameters hold the viscosity mu_f"):      # no viscosity, no wall shear stress
        sp.quantities({"spectrogram": ["v", "wss"]})
    with pytest.raises(SystemExit, match=r"got \['tawss'\]"):
        sp.quantities({"spectrogram": ["tawss", "wss"], "mu_f": 3.5e-3})
    assert sp.MIN_COLOR["wss"] == -18 and sp.fields({"spectrogram": ["wss", "p"], "mu_f": 3.5e-3}) == ["p", "v"]
    base = dict(ns, results_folder=tmp_path, spectrogram=["v", "wss"], spectrogram_sampling="All", spectrogram_fsi_region=sphere, save_deg=2)
    run = sp.SpectrogramRun(None, mesh, base, open_sessions=False)
    n = len(run.sel["wss"]["ids"])
    assert run.quantities == ["v", "wss"] and run.rows("wss") == 3 * n and run.min_color("wss") == -18 and run.min_color("v") == -20
    for comp in ("x", "mag"):
        r = sp.SpectrogramRun(None, mesh, dict(base, spectrogram_component=comp), open_sessions=False)
        assert r.rows("wss") == n and len(r.sel["wss"]["dofs"]) == n
    assert sp.SpectrogramRun(None, mesh, dict(base, spectrogram_min_color=-9), open_sessions=False).min_color("wss") == -9
    fp = run.fingerprint("wss")
    assert fp["mu"] == 3.5e-3 and fp["rows"] == 3 * n and {"facets", "dofs", "comps", "dt_sample", "component"} <= set(fp)
    other = sp.SpectrogramRun(None, mesh, dict(base, mu_f=4e-3, spectrogram_seed=1, spectrogram_sampling="RandomPoint", spectrogram_n_samples=n), open_sessions=False).fingerprint("wss")
    assert other["mu"] == 4e-3 and other["dofs"] != fp["dofs"] and other["facets"] == fp["facets"] and other["rows"] == fp["rows"]
    args = run.begin_args("wss", 128, 300)
    assert np.array_equal(args[0], cells) and args[2] == 3.5e-3 and np.array_equal(args[3], run.sel["wss"]["dofs"][128:300])
    # domain is refused for the wall shear stress, with the reason
    with pytest.raises(SystemExit, match="carries no cell markers"):
        sp.options(dict(base, spectrogram_region="domain", spectrogram_fluid_sampling_domain_id=1))
    # a backend without spec_begin_wss: refused before anything is built, by the refusal function and by the driver
    v = dict(base, save_step=1, T=0.099, dt=0.001)
    assert "needs a backend with spec_begin_wss (_Stub has none)" in sp.spectrogram_refusal(v, 1, _Stub)
    assert sp.spectrogram_refusal(dict(v, spectrogram=["v"]), 1, _Stub) == ""
    with pytest.raises(SystemExit, match="spec_begin_wss"):
        sp.SpectrogramRun(_Stub(cylinder_desc(ns)), mesh, base)
    from vasp_amd import monolithic
    with pytest.raises(SystemExit, match="--spectrogram wss needs a backend with spec_begin_wss"):
        monolithic.run(["-p", "cylinder", "-dt", "0.001", "-T", "0.099", "--save-step", "1", "--verbose", "False", "--folder", str(tmp_path / "r"),
                        "--spectrogram", "wss", *REGION, "--new-arguments", f"mesh_path={CYL}"], backend_factory=_Stub)
    assert not (tmp_path / "r").exists()


def cylinder_desc(ns):
    mesh = ns["mesh"]
    return dict(num_nodes=mesh.num_nodes, coords=mesh.coords)


# ---- --spectrogram-region domain --------------------------------------------------------------------------------------

def test_domain_sampling_takes_the_nodes_of_the_marked_cells(cylinder_case):
    """Part of the fluid and part of the solid get labels of their own (7, 8); the ids are those of a restatement of
    get_domain_ids_specified_region on the output's cells - no sphere, no box."""
    ns = cylinder_case[0]
    mesh = copy.copy(ns["mesh"])
    x = mesh.coords[mesh.tets].mean(axis=1)[:, 0]
    markers = mesh.cell_markers.copy()
    half = x > np.median(x)
    markers[(markers == ns["dx_f_id"]) & half] = 7
    markers[(markers == ns["dx_s_id"]) & half] = 8
    mesh.cell_markers = markers
    assert (markers == 7).any() and (markers == 8).any() and (markers == ns["dx_f_id"]).any() and (markers == ns["dx_s_id"]).any()
    v = dict(ns, spectrogram=["d", "v", "p"], spectrogram_sampling="All", spectrogram_region="domain", fsi_region=None,
             spectrogram_fluid_sampling_domain_id=7, spectrogram_solid_sampling_domain_id=8)
    o = sp.options(v)
    assert o["region"] == "domain" and o["fsi_region"] is None                                # fsi_region is not required
    for q, deg in (("d", 2), ("v", 2), ("p", 1)):
        cells = mesh.tet_nodes if deg == 2 else mesh.tets
        fluid, solid = np.unique(cells[np.nonzero(markers == 7)]), np.unique(cells[np.nonzero(markers == 8)])
        ids = sp.select_nodes(mesh, 2, q, v, o)["ids"]
        assert np.array_equal(ids, solid if q == "d" else fluid), q
        both = sp.select_nodes(mesh, 2, q, v, sp.options(dict(v, spectrogram_interface_only=True)))["ids"]
        assert len(both) > 0 and np.array_equal(both, np.intersect1d(fluid, solid)), q
    # the defaults are the reference's 1 and 2 (on this mesh the other halves), but at least one id is the user's to give
    d = sp.options(dict(ns, spectrogram=["v"], spectrogram_region="domain", spectrogram_fluid_sampling_domain_id=7))
    assert (d["fluid_sampling_domain_id"], d["solid_sampling_domain_id"]) == (7, 2)
    d = sp.options(dict(ns, spectrogram=["d"], spectrogram_region="domain", spectrogram_solid_sampling_domain_id=8))
    assert (d["fluid_sampling_domain_id"], d["solid_sampling_domain_id"]) == (1, 8)
    for region in ("domain", "cylinder"):
        with pytest.raises(SystemExit, match="domain together with --spectrogram-fluid-sampling-domain-id and / or"):
            sp.options(dict(ns, spectrogram=["v"], spectrogram_region=region))
    assert np.array_equal(sp.select_nodes(mesh, 2, "v", v, dict(o, fluid_sampling_domain_id=1))["ids"], np.unique(mesh.tet_nodes[markers == 1]))
    with pytest.raises(SystemExit, match="no nodes found"):
        sp.select_nodes(mesh, 2, "v", v, dict(o, fluid_sampling_domain_id=99))
    from vasp_amd.monolithic import parse
    a = parse(["--spectrogram", "v", "--spectrogram-region", "domain", "--spectrogram-fluid-sampling-domain-id", "7",
               "--spectrogram-solid-sampling-domain-id", "8"])
    assert a["spectrogram_fluid_sampling_domain_id"] == 7 and a["spectrogram_solid_sampling_domain_id"] == 8


# ---- the sound file of PointList --------------------------------------------------------------------------------------

def test_point_list_writes_the_sound_file_of_the_high_passed_rows(tmp_path):
    from scipy.io import wavfile
    from scipy.signal import butter, filtfilt
    ids = [3, 11, 40]
    ns, lines = _stub_run(tmp_path / "mycase", ["--spectrogram", "v", "--spectrogram-sampling", "PointList", "--spectrogram-point-ids",
                                                *map(str, ids), *REGION])
    mesh, states = ns["mesh"], np.stack(ns["backend"].states)
    n, N2 = len(states), mesh.num_nodes
    out = tmp_path / "mycase" / "1" / "Spectrograms"
    path = out / "v_all_sound_mycase_PointList_[3, 11, 40].wav"
    assert path.exists() and len(list(out.iterdir())) == 5
    fs = n / (n * 1e-3)
    rate, y = wavfile.read(path)
    assert rate == int(fs) and y.dtype == np.float64 and y.shape == (n,)
    rows = np.concatenate([states[:, 3 * N2:6 * N2].reshape(n, N2, 3)[:, ids, c] for c in range(3)], axis=1)       # component-major
    b, a = butter(6, 25.0 / (0.5 * fs), btype="highpass")
    filtered = np.stack([filtfilt(b, a, rows[:, r]) for r in range(rows.shape[1])])
    m = filtered.max()
    y2 = np.zeros(n)
    for row in filtered:
        y2 += row / m
    y2 = y2 / len(filtered)
    assert m > 0 and np.array_equal(y, y2)
    # All and RandomPoint write none
    _stub_run(tmp_path / "other", ["--spectrogram", "p", "--spectrogram-n-samples", "4", *REGION])
    assert not [p for p in (tmp_path / "other" / "1" / "Spectrograms").iterdir() if p.suffix == ".wav"]


class _Still(_Stub):
    """A state that never moves: every history is zero."""

    def newton_solve(self, **kw):
        self.steps += 1
        self.U = np.zeros(self.n)
        self.states.append(self.U.copy())
        return [(1e-8, 1e-9, False, 2, 1e-9)]


def test_an_all_zero_history_writes_no_sound_file_and_says_so(tmp_path):
    from vasp_amd import monolithic
    lines = []
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        monolithic.run(["-p", "cylinder", "-dt", "0.001", "-T", "0.099", "--theta", "0.51", "--folder", str(tmp_path / "still"), "--sub-folder", "1",
                        "--save-step", "1", "--save-deg", "2", "--verbose", "False", "--new-arguments", f"mesh_path={CYL}", "--spectrogram", "v",
                        "--spectrogram-sampling", "PointList", "--spectrogram-point-ids", "3", "11", "40", *REGION], backend_factory=_Still,
                       out=lines.append)
    out = tmp_path / "still" / "1" / "Spectrograms"
    assert len(list(out.iterdir())) == 4 and not list(out.glob("*.wav"))
    said = [line for line in lines if "no sound file written" in line]
    assert len(said) == 1 and "\n" not in said[0] and "v_all" in said[0]
    assert sp.sound_of(np.zeros((30, 3))) is None and sp.sound_of(np.full((30, 3), -1.0)) is None and sp.sound_of(np.full((4, 2), np.nan)) is None
