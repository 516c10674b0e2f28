"""Host side of --spectrogram (vasp_amd/spectrogram.py): the NumPy twin of the device session against scipy itself, the
chroma filter bank, chromagram and SBI against recorded results of the reference's own filter bank, the region and sampling
rules, the refusals, the CSV files, and the C-ABI's new entry points.

The bound on a power (``power_bound``)
--------------------------------------
One row, one segment of K frames, one bin: X = sum_j t_j y_j with t_j the table entry (|t_j| <= 1) and y_j = w_j (x_j - m).
Against the exact value, the computed X is off by at most

* one rounding each (2^-53, relative) for the table entry, for the product t_j y_j, for the difference x_j - m and for the
  product with w_j: 4 roundings, counted as 8 to have room for the constants of a (1 + u)^k expansion;
* K roundings of the accumulation, whatever its order (a dot product of K terms, BLAS or the matrix pipe);
* the error of the mean: m is a sum of K terms of size <= max|x|, off by at most K 2^-53 max|x|, and enters every y_j
  with weight w_j.

So |dX| <= (K + 8) 2^-53 (sum_j |w_j (x_j - m)| + sum_j w_j max|x|); the factor 2 in front covers scipy's own FFT, whose
error is below that of the dot product it replaces.  The power P = f s |X|^2 (s the scale, f = 2 for a doubled bin) then
moves by at most f s (2 |X| dX + dX^2), with |X| taken from scipy's P.  The average over the rows is bounded by the average
of the rows' bounds.  Nothing in it is tuned to what the code gives: on the rows of this file the host session uses between
3e-5 and 4 % of it (most with a single row and short segments; the tests print the share, NOTEBOOK.md section 13 lists them).
"""
import contextlib
import importlib.util
import io
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from vasp_amd import spectrogram as sp

_spec = importlib.util.spec_from_file_location("make_spectrogram", GOLDEN / "make_spectrogram.py")
make_spectrogram = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_spectrogram)
CYL = GOLDEN / "cylinder" / "cylinder.h5"
U = 2.0 ** -53


# ---- helpers shared with tests/test_gpu_spectrogram.py ----------------------------------------------------------------

def synthetic_rows(n, rows, fs=1000.0, seed=3):
    """(n, rows): per row a mean of 1e4 .. 2e4 (a pressure), a slow 7 Hz carrier of 50, a chirp of amplitude 1 from 50 Hz
    upwards and noise whose level depends on the row (0.01 .. 1)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None] / fs
    return (1e4 * (1 + rng.random(rows)))[None, :] + 50 * np.sin(2 * np.pi * 7 * t + rng.uniform(0, 6, rows)[None, :]) \
        + np.sin(2 * np.pi * (50 + 100 * t) * t) + rng.standard_normal((n, rows)) * rng.uniform(0.01, 1, rows)[None, :]


def scipy_spectrogram_rows(x, fs, K, nov, nfft, window, scaling):
    """scipy.signal.spectrogram row by row, as get_spectrogram calls it: (rows, bins, segments)."""
    from scipy.signal import spectrogram
    return np.stack([spectrogram(x[:, r], fs=fs, nperseg=K, noverlap=nov, nfft=nfft, window=window, scaling=scaling)[2]
                     for r in range(x.shape[1])])


def scipy_periodogram_rows(x, fs, scaling):
    """scipy.signal.periodogram row by row, as get_psd calls it: (rows, bins, 1)."""
    from scipy.signal import periodogram
    return np.stack([periodogram(x[:, r], fs=fs, window="blackmanharris", scaling=scaling)[1] for r in range(x.shape[1])])[:, :, None]


def power_bound(x, P_rows, w, K, step, nfft, scaling, fs, accumulation_only=False):
    """(bins, segments): the module docstring's bound on the row-averaged power.  ``accumulation_only``: the part of it that
    two evaluations with the same mean and the same y_j can differ by - the K roundings of the accumulation on either side
    and 8 for a table entry rounded differently, no factor for scipy's FFT, no error of the mean:
    (2 K + 8) 2^-53 sum_j |w_j (x_j - m)|."""
    w = np.asarray(w, dtype=np.float64)
    scale = 1.0 / (fs * np.sum(w * w)) if scaling == "density" else 1.0 / np.sum(w) ** 2
    nbins = nfft // 2 + 1
    f = np.full(nbins, 2.0)
    f[0] = 1.0
    if nfft % 2 == 0:
        f[-1] = 1.0
    out = np.empty((nbins, P_rows.shape[2]))
    for seg in range(P_rows.shape[2]):
        xs = x[seg * step:seg * step + K]
        a = np.sum(np.abs(w[:, None] * (xs - xs.mean(axis=0))), axis=0)
        if accumulation_only:
            dX = (2 * K + 8) * U * a
        else:
            dX = 2 * (K + 8) * U * (a + np.sum(np.abs(w)) * np.abs(xs).max(axis=0))
        X = np.sqrt(P_rows[:, :, seg] / (scale * f[None, :]))
        out[:, seg] = ((2 * X * dX[:, None] + dX[:, None] ** 2) * scale * f[None, :]).mean(axis=0)
    return out


def host_session(x):
    s = sp.HostSpecSession(x.shape[1], len(x))
    for frame in x:
        s.sample(frame)
    return s


# ---- the host session against scipy -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n,rows,K,nov,window,seed", [(1501, 96, 256, 192, "blackmanharris", 3), (1500, 130, 128, 96, "hann", 4),
                                                     (700, 1, 64, 48, "blackmanharris", 5), (333, 7, 100, 75, "hann", 6)])
def test_host_spectrogram_equals_scipy_within_the_derived_bound(n, rows, K, nov, window, seed):
    fs = 1000.0
    x = synthetic_rows(n, rows, fs, seed)
    s = host_session(x)
    w = sp.window_values(window, K)
    for scaling in ("spectrum", "density"):
        got = s.spectrogram(K, nov, 2 * K, w, scaling, fs)
        ref_rows = scipy_spectrogram_rows(x, fs, K, nov, 2 * K, window, scaling)
        ref = ref_rows.mean(axis=0)
        bound = power_bound(x, ref_rows, w, K, K - nov, 2 * K, scaling, fs)
        share = (np.abs(got - ref) / bound).max()
        print(f"n {n} rows {rows} K {K} {window} {scaling}: share of the bound {share:.3e}, max relative error "
              f"{(np.abs(got - ref) / ref).max():.3e}")
        assert got.shape == ref.shape == (K + 1, (n - nov) // (K - nov))
        assert (np.abs(got - ref) <= bound).all()


@pytest.mark.parametrize("n,rows", [(1501, 96), (1500, 40), (257, 1)])
def test_host_periodogram_equals_scipy_within_the_derived_bound(n, rows):
    fs = 987.5
    x = synthetic_rows(n, rows, fs, 8)
    s = host_session(x)
    w = sp.window_values("blackmanharris", n)
    for scaling in ("spectrum", "density"):
        got = s.periodogram(w, scaling, fs)
        ref_rows = scipy_periodogram_rows(x, fs, scaling)
        bound = power_bound(x, ref_rows, w, n, n, n, scaling, fs)[:, 0]
        err = np.abs(got - ref_rows.mean(axis=0)[:, 0])
        print(f"n {n} rows {rows} {scaling}: share of the bound {(err / bound).max():.3e}")
        assert got.shape == (n // 2 + 1,)
        assert (err <= bound).all()


def test_filtered_source_and_magnitude_rows():
    """The filtered series is scipy's filtfilt bit for bit (vasp_amd.hi_pass), so its spectrogram is held to the same bound
    on the filtered rows; component 'mag' is the root of the sum of squares in numpy.linalg.norm's order."""
    from scipy.signal import filtfilt
    fs, n, K, nov = 1000.0, 600, 128, 96
    rng = np.random.default_rng(12)
    vec = synthetic_rows(n, 3 * 20, fs, 9).reshape(n, 20, 3) - 1.5e4 + rng.standard_normal((n, 20, 3))
    x = np.stack([sp.component_rows(v, "mag") for v in vec])
    assert np.abs(x - np.linalg.norm(vec, axis=2)).max() <= 2 * np.finfo(float).eps * x.max()
    assert np.array_equal(sp.component_rows(vec[0], "all"), np.concatenate([vec[0][:, 0], vec[0][:, 1], vec[0][:, 2]]))
    assert np.array_equal(sp.component_rows(vec[0], "y"), vec[0][:, 1])
    s = host_session(x)
    hp = sp.highpass_design(fs, 25.0)
    assert len(hp["b"]) == 7 and hp["padlen"] == sp.HP_PADLEN == 21
    s.filter(hp["b"], hp["a"], hp["zi"], hp["padlen"])
    y = np.stack([filtfilt(hp["b"], hp["a"], x[:, r]) for r in range(x.shape[1])], axis=1)
    assert np.array_equal(np.stack([s.fetch(k, True) for k in range(n)]), y)
    w = sp.window_values("blackmanharris", K)
    got = s.spectrogram(K, nov, 2 * K, w, "spectrum", fs)
    ref_rows = scipy_spectrogram_rows(y, fs, K, nov, 2 * K, "blackmanharris", "spectrum")
    assert (np.abs(got - ref_rows.mean(axis=0)) <= power_bound(y, ref_rows, w, K, K - nov, 2 * K, "spectrum", fs)).all()
    s.filter()                                               # back to the raw rows
    ref_rows = scipy_spectrogram_rows(x, fs, K, nov, 2 * K, "blackmanharris", "spectrum")
    got = s.spectrogram(K, nov, 2 * K, w, "spectrum", fs)
    assert (np.abs(got - ref_rows.mean(axis=0)) <= power_bound(x, ref_rows, w, K, K - nov, 2 * K, "spectrum", fs)).all()


def reference_pipeline(x, T, o, min_color):
    """create_spectrogram_composite / create_spectrum with scipy, row by row as the reference runs them: the clamped log
    spectrogram of the high-passed rows, the raw rows' power, the periodogram, and the bounds on the two powers."""
    from scipy.signal import butter, filtfilt
    n, rows = x.shape
    fs = n / T
    num_windows = np.round(o["num_windows_per_sec"] * T) + 3
    K = sp.shift_bit_length(int(n / num_windows))
    nov = int(o["overlap_frac"] * K)
    b, a = butter(6, o["lowcut"] / (0.5 * fs), btype="highpass")
    y = np.stack([filtfilt(b, a, x[:, r]) for r in range(rows)], axis=1)
    w = sp.window_values(o["window"], K)
    Pf_rows = scipy_spectrogram_rows(y, fs, K, nov, 2 * K, o["window"], "spectrum")
    Pr_rows = scipy_spectrogram_rows(x, fs, K, nov, 2 * K, o["window"], "spectrum")
    scaling = "spectrum" if rows > 1 else "density"
    Pp_rows = scipy_periodogram_rows(x, fs, scaling)
    return dict(K=K, nov=nov, fs=fs, num_windows=num_windows, Pf=Pf_rows.mean(axis=0), Pr=Pr_rows.mean(axis=0), Pp=Pp_rows.mean(axis=0)[:, 0],
                bf=power_bound(y, Pf_rows, w, K, K - nov, 2 * K, "spectrum", fs), br=power_bound(x, Pr_rows, w, K, K - nov, 2 * K, "spectrum", fs),
                bp=power_bound(x, Pp_rows, sp.window_values("blackmanharris", n), n, n, n, scaling, fs)[:, 0])


def assert_log_close(got, P_ref, bound, min_color=None):
    """A written log power against the reference's power and its bound, in the power domain: an entry above the clamp is
    the log of a power within the bound (16 ulps for log and exp); a clamped entry needs a power that the bound lets fall to
    the clamp; and where the reference itself is clamped as well, the two are equal - both are min_color."""
    eps = 16 * np.finfo(float).eps
    clamped = np.zeros(got.shape, dtype=bool) if min_color is None else got == min_color
    if min_color is not None:
        assert (got >= min_color).all()
        assert (P_ref[clamped] - bound[clamped] <= np.exp(min_color) * (1 + eps)).all()
        with np.errstate(divide="ignore"):
            both = clamped & (np.maximum(np.log(P_ref), min_color) == min_color)
        assert np.array_equal(got[both], np.full(both.sum(), float(min_color)))
    free = ~clamped
    assert (np.abs(np.exp(got[free]) - P_ref[free]) <= bound[free] + eps * P_ref[free]).all()


OPTS = dict(num_windows_per_sec=4, overlap_frac=0.75, window="blackmanharris", lowcut=25.0)


@pytest.mark.parametrize("rows", [24, 1])
def test_pipeline_equals_the_reference_pipeline_on_scipy(rows):
    """The whole of create_spectrogram_composite and create_spectrum: the log spectrogram clamped at min_color, and the
    no-filter spectrum - with one row in scipy's "density" scaling, the reference's silent fall-back (get_psd)."""
    n, T, min_color = 1201, 1.201, -5
    x = synthetic_rows(n, rows, n / T, 21)
    ref = reference_pipeline(x, T, OPTS, min_color)
    res = sp.pipeline(host_session(x), rows, n, T, 0.25, OPTS, min_color)
    assert (res["plan"]["nperseg"], res["plan"]["noverlap"], res["plan"]["nfft"]) == (ref["K"], ref["nov"], 2 * ref["K"]) == (256, 192, 512)
    assert res["psd_scaling"] == ("spectrum" if rows > 1 else "density")
    assert (np.abs(res["power_filtered"] - ref["Pf"]) <= ref["bf"]).all() and (np.abs(res["power_raw"] - ref["Pr"]) <= ref["br"]).all()
    assert (np.abs(res["power_psd"] - ref["Pp"]) <= ref["bp"]).all()
    assert_log_close(res["spectrogram"], ref["Pf"], ref["bf"], min_color)
    assert (res["spectrogram"] == min_color).any() and (res["spectrogram"] > min_color).any()
    assert_log_close(res["psd"], ref["Pp"], ref["bp"])
    from scipy.signal import spectrogram
    f, t, _ = spectrogram(x[:, 0], fs=ref["fs"], nperseg=ref["K"], noverlap=ref["nov"], nfft=2 * ref["K"])
    assert np.allclose(res["freqs"], f, rtol=1e-14) and np.allclose(res["bins"], t + 0.25, rtol=1e-14)       # bins shifted by the start time
    # chromagram and SBI of scipy's raw power: the session's power is within its bound of it, a relative change of at most e;
    # through the filter bank (weights >= 0, columns scaled to sum 1) that moves a chroma entry by at most 2 e of itself (e
    # in the numerator, e in the normalising sum), and c log c by (|log c| + 1) times as much
    chroma = sp.chromagram(np.exp(np.maximum(np.log(ref["Pr"]), min_color)), ref["fs"], 2 * ref["K"])
    assert res["chroma"].shape == (24, len(t)) and np.allclose(res["chroma"].sum(axis=0), 1.0, rtol=1e-14)
    assert (ref["Pr"] > 2 * ref["br"]).all()
    e = (ref["br"] / (ref["Pr"] - ref["br"])).max() + 16 * np.finfo(float).eps
    print(f"rows {rows}: relative bound on the raw power {e:.3e}, chroma off by {(np.abs(res['chroma'] - chroma) / chroma).max():.3e} of itself")
    assert (np.abs(res["chroma"] - chroma) <= 2 * e * chroma).all()
    dsbi = (2 * e * chroma * (np.abs(np.log(chroma)) + 1)).sum(axis=0) / np.log(24)
    assert (np.abs(res["sbi"] - sp.sbi(chroma)) <= dsbi + 16 * np.finfo(float).eps).all()
    assert ((res["sbi"] > 0) & (res["sbi"] < 1)).all()


# ---- chroma, SBI, sizes -----------------------------------------------------------------------------------------------

def test_chroma_filterbank_chromagram_and_sbi_equal_the_recorded_reference():
    """The filter bank is float32 and must equal the reference's to the bit or to one float32 ulp (numpy's exp / log2 may move
    by an ulp between builds); chromagram and SBI are one dot product per entry over a column of the spectrogram: 8 ulps of the
    column's sum of |filter x power| over the normalising sum.  The run that made the fixture showed 0 for all three."""
    g = np.load(GOLDEN / "spectrogram" / "chroma.npz")
    for i, (fs, n_fft, nseg) in enumerate(make_spectrogram.PAIRS):
        fb = sp.chroma_filterbank(fs, n_fft)
        P = g[f"P{i}"]
        assert np.array_equal(P, make_spectrogram.spectrum(fs, n_fft, nseg, 40 + i))
        assert fb.dtype == np.float32 and fb.shape == (24, n_fft // 2 + 1)
        assert (np.abs(fb - g[f"fb{i}"]) <= np.spacing(np.abs(g[f"fb{i}"]))).all()
        c = sp.chromagram(P, fs, n_fft)
        tol = 8 * np.finfo(float).eps * (np.abs(g[f"fb{i}"]).astype(float) @ P).sum(axis=0) / (g[f"fb{i}"].astype(float) @ P).sum(axis=0)
        print(f"pair {i}: filter bank {np.abs(fb - g[f'fb{i}']).max():.1e}, chroma {np.abs(c - g[f'chroma{i}']).max():.1e}, "
              f"SBI {np.abs(sp.sbi(c) - g[f'sbi{i}']).max():.1e}")
        if np.array_equal(fb, g[f"fb{i}"]):
            assert (np.abs(c - g[f"chroma{i}"]) <= tol[None, :]).all()
            assert np.abs(sp.sbi(c) - g[f"sbi{i}"]).max() <= 24 * 40 * tol.max()     # d(c log c) <= (|log c| + 1) dc, |log c| < 39 here
        assert np.allclose(c, g[f"chroma{i}"], rtol=1e-6, atol=1e-12) and np.allclose(sp.sbi(c), g[f"sbi{i}"], rtol=1e-6)


def test_window_arithmetic_equals_the_recorded_values():
    plans = np.load(GOLDEN / "spectrogram" / "chroma.npz")["plans"]
    assert len(plans) == len(make_spectrogram.PLANS) >= 5
    for n, T, per_sec, frac, num_windows, nperseg, noverlap, nfft in plans:
        p = sp.window_plan(int(n), T, int(per_sec), frac)
        assert (p["num_windows"], p["nperseg"], p["noverlap"], p["nfft"]) == (num_windows, nperseg, noverlap, nfft)
        assert p["nseg"] == (int(n) - int(noverlap)) // (int(nperseg) - int(noverlap))
    assert [sp.shift_bit_length(k) for k in (1, 2, 3, 64, 65, 166)] == [1, 2, 4, 64, 128, 256]


# ---- region and sampling rules ----------------------------------------------------------------------------------------

def test_region_and_sampling_rules_on_the_stenosis_mesh(stenosis_case):
    ns = stenosis_case[0]
    mesh = ns["mesh"]
    v = dict(ns, spectrogram=["d", "v", "p"], spectrogram_sampling="All")
    o = sp.options(v)
    assert o["fsi_region"] == [float(c) for c in ns["fsi_region"]] and o["n_samples"] == 1000 and o["lowcut"] == 25 and o["seed"] == 0
    fluid_cells = np.isin(mesh.cell_markers, ns["dx_f_id"])
    solid_cells = mesh.cell_markers == ns["dx_s_id"]
    centre, r = np.array(o["fsi_region"][:3]), o["fsi_region"][3]
    for q, deg in (("d", 2), ("v", 2), ("p", 1)):
        sel = sp.select_nodes(mesh, 2, q, v, o)
        ids = sel["ids"]
        assert sel["degree"] == deg and len(ids) > 0 and len(np.unique(ids)) == len(ids)           # All: no duplicates
        cells = mesh.tet_nodes if deg == 2 else mesh.tets
        coords = mesh.node_coords if deg == 2 else mesh.coords
        own = np.unique(cells[solid_cells if q == "d" else fluid_cells])
        assert np.isin(ids, own).all()                                                               # d: solid nodes only
        assert (np.linalg.norm(coords[ids] - centre, axis=1) < r).all()
        expect = own[np.linalg.norm(coords[own] - centre, axis=1) < r]
        assert np.array_equal(np.sort(ids), expect)
        assert np.array_equal(sel["nodes"], ids) and sel["nodes_b"] is None and sel["name"] == f"{q}_all"
    # interface-only: the intersection
    oi = sp.options(dict(v, spectrogram_interface_only=True))
    both = np.intersect1d(np.unique(mesh.tet_nodes[fluid_cells]), np.unique(mesh.tet_nodes[solid_cells]))
    ids = sp.select_nodes(mesh, 2, "v", v, oi)["ids"]
    assert len(ids) > 0 and np.isin(ids, both).all() and np.array_equal(ids, sp.select_nodes(mesh, 2, "d", v, oi)["ids"])
    # a seeded draw repeats, another seed draws other nodes; the reference's names
    orp = sp.options(dict(v, spectrogram_sampling="RandomPoint", spectrogram_n_samples=50, spectrogram_seed=7))
    a, b = sp.select_nodes(mesh, 2, "v", v, orp), sp.select_nodes(mesh, 2, "v", v, orp)
    c = sp.select_nodes(mesh, 2, "v", v, sp.options(dict(v, spectrogram_sampling="RandomPoint", spectrogram_n_samples=50, spectrogram_seed=8)))
    assert np.array_equal(a["ids"], b["ids"]) and len(a["ids"]) == 50 and not np.array_equal(a["ids"], c["ids"])
    assert np.isin(a["ids"], sp.region_ids(mesh, 2, "v", v, orp)).all() and a["name"] == "v_all_n_samples_50"
    pl = sp.select_nodes(mesh, 2, "d", v, sp.options(dict(v, spectrogram_sampling="PointList", spectrogram_point_ids=[3, 11], spectrogram_component="mag")))
    assert pl["ids"].tolist() == [3, 11] and pl["name"] == "d_mag" and pl["case_suffix"] == "_PointList_[3, 11]"
    # an open box around the same centre
    box = [centre[0] - r, centre[0] + r, centre[1] - r, centre[1] + r, centre[2] - r, centre[2] + r]
    ob = sp.options(dict(v, spectrogram_region="box", spectrogram_fsi_region=box))
    ids_box = sp.select_nodes(mesh, 2, "v", v, ob)["ids"]
    assert set(sp.select_nodes(mesh, 2, "v", v, o)["ids"]) <= set(ids_box)
    # an empty sphere is refused
    with pytest.raises(SystemExit, match="no nodes found in the specified fsi region"):
        sp.select_nodes(mesh, 2, "v", v, sp.options(dict(v, spectrogram_fsi_region=[10.0, 10.0, 10.0, 1e-3])))
    with pytest.raises(SystemExit, match="sphere or box"):
        sp.options(dict(v, spectrogram_region="domain"))
    with pytest.raises(SystemExit, match="get_window"):
        sp.options(dict(v, spectrogram_window="kaiser"))
    with pytest.raises(SystemExit, match="d, v and / or p"):
        sp.quantities({"spectrogram": ["wss"]})


def test_options_from_the_command_line_a_config_file_and_new_arguments(tmp_path):
    from vasp_amd.monolithic import parse
    a = parse(["--spectrogram", "v", "p", "--spectrogram-sampling", "All", "--spectrogram-fsi-region", "0.008", "0", "0", "0.004",
               "--spectrogram-min-color", "-12", "--spectrogram-interface-only", "--spectrogram-seed", "3"])
    assert a["spectrogram"] == ["v", "p"] and a["spectrogram_sampling"] == "All" and a["spectrogram_fsi_region"] == [0.008, 0, 0, 0.004]
    assert a["spectrogram_min_color"] == -12 and a["spectrogram_interface_only"] is True and a["spectrogram_seed"] == 3
    assert not any(k.startswith("spectrogram") for k in parse([]))
    cfg = tmp_path / "run.cfg"
    cfg.write_text('spectrogram = ["d"]\nspectrogram_fsi_region = [0, 0, 0, 1]\nspectrogram-n-samples = 20\nspectrogram_window = hann\n')
    c = parse(["-c", str(cfg)])
    assert c["spectrogram"] == ["d"] and c["spectrogram_fsi_region"] == [0, 0, 0, 1] and c["spectrogram_n_samples"] == 20
    assert c["spectrogram_window"] == "hann"
    n = parse(["--new-arguments", "spectrogram=['p']", "spectrogram_component=mag", "spectrogram_point_ids=[4, 5]"])
    assert n["spectrogram"] == ["p"] and n["spectrogram_component"] == "mag" and n["spectrogram_point_ids"] == [4, 5]
    o = sp.options(dict(c, fsi_region=[9, 9, 9, 9]))
    assert o["fsi_region"] == [0.0, 0.0, 0.0, 1.0] and o["window"] == "hann" and o["n_samples"] == 20 and o["sampling"] == "RandomPoint"


# ---- refusals ---------------------------------------------------------------------------------------------------------

REGION = ["--spectrogram-fsi-region", "0", "0", "0", "100"]


def _refusal(extra, world=1):
    from vasp_amd.monolithic import parameters
    with contextlib.redirect_stdout(io.StringIO()):
        _, _, v = parameters(["-p", "cylinder", "--spectrogram", "v", "--verbose", "False", *REGION, *extra])
    return sp.spectrogram_refusal(v, world, None)


class _Stub:
    """Host stand-in for HipBackend in the time loop, without a device session: every dof has a mean, a slow carrier and a
    tone of its own, so SpectrogramRun records and transforms on the host."""

    def __init__(self, desc):
        self.n = 6 * int(desc["num_nodes"]) + len(desc["coords"])
        rng = np.random.default_rng(5)
        self.f, self.ph, self.mean = rng.uniform(40.0, 400.0, self.n), rng.uniform(0, 6.28, self.n), rng.uniform(-1, 1, self.n)
        self.U = np.zeros(self.n)
        self.steps = 0
        self.states = []

    def set_dirichlet_values(self, v): pass
    def set_interface_pressure(self, P): pass
    def shift(self): pass
    def set_state(self, which, x): self.U[:] = x

    def newton_solve(self, **kw):
        self.steps += 1
        t = 1e-3 * self.steps
        self.U = self.mean + 1e-1 * np.sin(2 * np.pi * 3.0 * t + self.ph) + 1e-3 * np.sin(2 * np.pi * self.f * t + self.ph)
        self.states.append(self.U.copy())
        return [(1e-8, 1e-9, False, 2, 1e-9)]

    def get_state(self, which, out=None):
        out[:] = self.U
        return out


def test_each_refusal_has_its_message(tmp_path, monkeypatch):
    ok = ["-dt", "0.001", "-T", "0.099", "--save-step", "1"]            # 100 frames
    assert _refusal(ok) == ""
    assert "cannot be used with --restart-folder" in _refusal(ok + ["--restart-folder", str(tmp_path)])
    assert "one rank only (WORLD_SIZE > 1)" in _refusal(ok, world=2)
    assert "needs --save-step" in _refusal(["-dt", "0.001", "-T", "0.099", "--save-step", "0"])
    msg = _refusal(["-dt", "0.001", "-T", "0.020", "--save-step", "1"])
    assert "saves 21 frames" in msg and "padlen + 1 = 22" in msg
    msg = _refusal(ok + ["--spectrogram-num-windows-per-sec", "0"])            # 3 windows of 33 -> segments of 64, 75 % overlap: 3 of them
    assert msg == ""
    msg = _refusal(ok + ["--spectrogram-overlap-frac", "0"])                   # segments of 64 without overlap: one
    assert "segments of 64 frames and 1 of them" in msg and "at least two" in msg
    from vasp_amd import monolithic
    argv = ["-p", "cylinder", "-dt", "0.001", "-T", "0.01", "--save-step", "1", "--verbose", "False", "--folder", str(tmp_path / "r"),
            "--spectrogram", "d", *REGION, "--new-arguments", f"mesh_path={CYL}"]
    with pytest.raises(SystemExit, match="padlen"):                            # through the driver: before anything is built
        monolithic.run(argv, backend_factory=_Stub)
    assert not (tmp_path / "r").exists()
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    with pytest.raises(SystemExit, match="one rank only"):
        monolithic.run(argv[:5] + ["0.099"] + argv[6:], backend_factory=_Stub)


# ---- the files --------------------------------------------------------------------------------------------------------

def _stub_run(folder, extra, T="0.099"):
    from vasp_amd import monolithic
    lines = []
    with contextlib.redirect_stdout(io.StringIO()):
        ns = monolithic.run(["-p", "cylinder", "-dt", "0.001", "-T", T, "--theta", "0.51", "--folder", str(folder), "--sub-folder", "1",
                             "--save-step", "1", "--save-deg", "2", "--verbose", "False", "--new-arguments", f"mesh_path={CYL}",
                             *extra], backend_factory=_Stub, out=lines.append)
    return ns, lines


def read_csv(path):
    """(header line without its '# ', the table)."""
    with open(path) as fh:
        header = fh.readline()
    assert header.startswith("# ")
    return header[2:].strip(), np.loadtxt(path, delimiter=",", ndmin=2)


def test_driver_writes_the_four_files_of_the_host_pipeline(tmp_path):
    ns, lines = _stub_run(tmp_path / "mycase", ["--spectrogram", "v", "p", "--spectrogram-sampling", "All", *REGION])
    mesh, states = ns["mesh"], np.stack(ns["backend"].states)
    n = len(states)
    assert n == 100 and any("Spectrograms of 100 frames (v, p; All" in line for line in lines)
    out = tmp_path / "mycase" / "1" / "Spectrograms"
    assert sorted(p.name for p in out.iterdir()) == sorted(
        f for q, c in (("v", -20), ("p", -5)) for f in sp.file_names(f"{q}_all", "mycase", np.float64(3.0), c).values())
    assert (out / "v_all_mycase_3.0_windows_thresh-20_spectrogram.csv").exists() and (out / "p_all_psd_no_filter_mycase.csv").exists()
    N2 = mesh.num_nodes
    v = dict(ns, spectrogram_sampling="All", spectrogram_fsi_region=[0, 0, 0, 100])
    o = sp.options(v)
    for q, min_color in (("v", -20), ("p", -5)):
        sel = sp.select_nodes(mesh, 2, q, v, o)
        if q == "p":
            x = states[:, 6 * N2:][:, sel["ids"]]
        else:
            x = np.concatenate([states[:, 3 * N2:6 * N2].reshape(n, N2, 3)[:, sel["ids"], c] for c in range(3)], axis=1)
        res = sp.pipeline(host_session(x), x.shape[1], n, n * 1e-3, 0.0, o, min_color)
        names = sp.file_names(sel["name"], "mycase", res["plan"]["num_windows"], min_color)
        head, tab = read_csv(out / names["spectrogram"])
        nseg = res["plan"]["nseg"]
        assert (res["plan"]["nperseg"], nseg) == (64, 3) and tab.shape == (65, 1 + nseg)
        assert [float(t) for t in head.split(",")] == [round(b, 2) for b in res["bins"]]                     # precision = 2
        assert np.array_equal(tab[:, 0], res["freqs"]) and np.array_equal(tab[:, 1:], res["spectrogram"])
        assert tab[1, 0] == pytest.approx(1000.0 / 128) and (tab[:, 1:] >= min_color).all()
        head_c, tab_c = read_csv(out / names["chromagram"])
        assert head_c == head and tab_c.shape == (24, 1 + nseg) and np.array_equal(tab_c[:, 0], np.linspace(0, 1, 24))
        assert np.array_equal(tab_c[:, 1:], res["chroma"]) and np.allclose(tab_c[:, 1:].sum(axis=0), 1.0, rtol=1e-14)
        head_s, tab_s = read_csv(out / names["sbi"])
        assert head_s == "t (s), SBI" and np.array_equal(tab_s, np.array([res["bins"], res["sbi"]]).T)
        head_p, tab_p = read_csv(out / names["psd"])
        assert head_p == "Freqs(Hz),spectrum" and tab_p.shape == (n // 2 + 1, 2)
        assert np.array_equal(tab_p[:, 0], res["psd_freqs"]) and np.array_equal(tab_p[:, 1], res["psd"])
        # and the numbers are the reference's pipeline on scipy
        ref = reference_pipeline(x, n * 1e-3, o, min_color)
        assert_log_close(tab[:, 1:], ref["Pf"], ref["bf"], min_color)
        assert_log_close(tab_p[:, 1], ref["Pp"], ref["bp"])
    plain, _ = _stub_run(tmp_path / "plain", [], T="0.004")
    assert not (tmp_path / "plain" / "1" / "Spectrograms").exists()


def test_a_stopped_run_writes_nothing_and_says_so(tmp_path):
    (tmp_path / "1").mkdir(parents=True)
    (tmp_path / "1" / "killturtle").write_text("")
    ns, lines = _stub_run(tmp_path, ["--spectrogram", "v", "--spectrogram-n-samples", "10", *REGION])
    assert ns["backend"].steps == 1
    assert any("1 frames recorded, too few" in line for line in lines)
    assert not (tmp_path / "1" / "Spectrograms").exists()


# ---- the C-ABI --------------------------------------------------------------------------------------------------------

SPEC_CALLS = ("fsi_spec_begin", "fsi_spec_sample", "fsi_spec_filter", "fsi_spec_fetch", "fsi_spec_spectrogram", "fsi_spec_periodogram",
              "fsi_spec_end")


def test_header_and_binding_agree_on_the_spec_entry_points():
    from vasp_amd import capi
    header = (ROOT / "include" / "vaspfsi.h").read_text()
    lib = capi.load_library()
    for name in SPEC_CALLS:
        m = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.M | re.S)
        assert m, name
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(m.group(1).split(",")), name
        doc = header[:m.start()].rsplit("/*", 1)[1]
        assert "REF" in doc or name == "fsi_spec_end", name               # every call names the reference lines it replaces
    for name, k in capi.HipBackend.SPEC_MODE.items():
        assert re.search(r"#define FSI_SPEC_%s %d\b" % (name.upper(), k), header)
    for name, k in capi.HipBackend.SPEC_SCALING.items():
        assert re.search(r"#define FSI_SPEC_%s %d\b" % (name.upper(), k), header)
    for meth in ("spec_begin", "spec_sample", "spec_filter", "spec_fetch", "spec_spectrogram", "spec_periodogram", "spec_end"):
        assert hasattr(capi.HipBackend, meth)
    src = (ROOT / "vasp_amd" / "csrc" / "fsi_spec.hip").read_text()
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in src and "atomicAdd" not in src
    sessions = (ROOT / "vasp_amd" / "csrc" / "fsi_sessions.hip").read_text()      # the band-pass session's sampling kernel, through the shared history
    assert "history_sample(" in sessions.split("int fsi_spec_sample")[1].split("int fsi_spec_fetch")[0]
    assert "launch_band_sample" in sessions.split("int history_sample")[1].split("int history_filter")[0]
    hpp = (ROOT / "vasp_amd" / "csrc" / "fsi_spec.hpp").read_text()
    assert int(re.search(r"SPEC_ROWS = (\d+)", hpp).group(1)) == sp.ROWS
