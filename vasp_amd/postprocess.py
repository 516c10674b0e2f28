"""The post-processing sessions of ``vasp_amd.monolithic`` on a results folder that already exists:
``python -m vasp_amd.postprocess --folder <results> --hi-pass v --hi-pass-bands 100 150 ...``.

Counterpart of the way the reference's tools are used - ``vasp-compute-hemo``, ``vasp-compute-stress``,
``vasp-create-hi-pass-viz``, ``vasp-create-spectrograms-chromagrams`` and ``vasp-create-spectrum`` take the folder of a
finished run, many times over with other bands, windows, regions and strides
[REF src/vasp/postprocessing/postprocessing_common.py:14-60,63-121] - where ``--hemodynamics`` ... ``--spectrogram`` of a run
sample the state while it steps.  Nothing is solved here and no problem file is read:

* the mesh is ``<results>/Mesh/mesh.h5`` (``prepare`` writes it with the problem's final markers), the parameters are
  ``<results>/Checkpoint/default_variables.json`` (what the reference's ``read_parameters_from_file`` reads) under the -c file
  under the command line under ``--new-arguments``;
* the frames are those of ``<results>/Visualization`` (``frames.FrameSource``) with ``k % stride == 0`` and
  ``start <= t_k <= end``; each goes into the state of a context without boundary data and with the smallest Krylov store
  (``HipBackend.set_frame``; the context is otherwise a run's: ``HipBackend`` still builds the matrix structure and runs
  ``fsi_solver_setup`` once, so starting the tool costs what starting a run costs) and every open session samples it - the same ``*Run`` classes, constructed from ``SESSIONS`` and
  told the frame times (``ns["frame_times"]``, ``ns["frame_stride"]``, ``ns["frame_start"]``), write the files a run writes
  into ``--output-folder`` (default: the results folder);
* a backend without the device methods records on the host where a run does, and is refused where a run refuses it.

At ``save_deg 2`` the files hold the whole state in FP64 and the outputs are those of the run, bit for bit.  At ``save_deg 1``
they hold the vertex values: a mid-edge node takes the mean of its edge's vertices, the P1 field the reference's tools see.

Band-pass histories larger than the device (``--hi-pass``, ``--hi-pass-tensor``): where the histories of all asked quantities
do not fit into ``--history-memory`` bytes (default: what ``fsi_band_room`` reports as available), each quantity goes through
its session in strips of rows, one quantity at a time (``hi_pass_strips``): the frames are read once per strip - with
``--hi-pass-amplitude`` once per strip and series -, the files are those of the unsplit path byte for byte, and the amplitude
table is formed on the device from a board of the magnitudes.  Where they fit, nothing differs from a call without the option.

Spectrogram histories larger than the device (``--spectrogram``): the same limit bounds them.  Where the sessions of all
asked spectrogram quantities do not fit beside the band-pass sessions of the first frame loop, every spectrogram quantity
goes through its session in strips of rows after that loop, one at a time (``spectrogram_strips``): the three mean powers
are sums over blocks of rows in a fixed order, carried from strip to strip, so the four CSV files are those of the unsplit
path byte for byte; the frames are read once per strip.

``--spectrogram wss`` reads the velocity; at ``save_deg 1`` its rows differ from a run's as those of ``--hemodynamics`` do.  With
``--spectrogram-region domain`` the markers are those of the mesh that is read: ``--mesh-path`` supplies a mesh labelled for
the purpose, as the reference intends.  The sound file of ``--spectrogram-sampling PointList`` is written by the unsplit path
only - a list of points never needs strips.

Not done: more than one rank, strips during a run, reading ``Checkpoint/sessions/*.f64`` instead of the frames, overlapping the reads with the device
work, PNG figures.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys
import time as _time
from pathlib import Path
from typing import Callable, Dict, List, Optional

import numpy as np

from . import hi_pass, vortex
from .fem import FormTerms
from .frames import FrameSource, selected_indices
from .mesh import FsiMesh
from .monolithic import (POD_NEEDS_HI_PASS, SESSIONS, SPI_NEEDS_HI_PASS, _session_part, add_session_arguments, build_description, build_properties,
                         resolve_arguments)

# what build_description and the sessions read of the run's parameters: without the JSON all of it must be given
NEEDED = ("dt", "save_step", "save_deg", "dx_f_id", "dx_s_id", "rho_f", "mu_f", "rho_s", "mu_s", "lambda_s", "material_model")
RUN_WINDOW = ("hi_pass_stride", "hi_pass_start_time", "hi_pass_end_time")
KRYLOV_CAPACITY_MIN = 8                         # csrc/fsi_setup.hip: the smallest FsiTuning.krylov_capacity a context takes


def parse(argv: Optional[List[str]] = None) -> Dict[str, object]:
    ap = argparse.ArgumentParser(prog="python -m vasp_amd.postprocess",
                                 description="hemodynamic indices, stress and strain, band-pass filtered fields and spectrograms "
                                             "of a finished results folder, on the MI355X")
    ap.add_argument("--folder", dest="results", default=None, help="the results folder of a run (<folder>/<sub-folder> of the run)")
    ap.add_argument("--mesh-path", dest="mesh_path", default=None, help="default: <results>/Mesh/mesh.h5")
    ap.add_argument("--output-folder", dest="output_folder", default=None, help="default: the results folder")
    ap.add_argument("--start-time", dest="start_time", type=float, default=None,
                    help="first time of the frames that are read, and the time the written files start at (default: 0)")
    ap.add_argument("--end-time", dest="end_time", type=float, default=None, help="last time of the frames that are read")
    ap.add_argument("--stride", dest="stride", type=int, default=None, help="read every S-th saved frame (default: 1)")
    ap.add_argument("--new-arguments", dest="new_arguments", nargs="*", default=[])
    add_session_arguments(ap)
    ap.add_argument("--history-memory", dest="history_memory", type=int, default=None, metavar="BYTES",
                    help="device memory the histories of --hi-pass / --hi-pass-tensor / --spectrogram may take (default: what the "
                         "device has free beside the context); quantities that do not fit go through their session in strips of rows")
    ap.add_argument("-c", "--config", dest="config", default=None, help="config file with `key = value` lines, as vasp_amd.monolithic's")
    return resolve_arguments(ap, argv)


def parameters(args: Dict[str, object]) -> Dict[str, object]:
    """The run's parameters under the given ones.  What names the run's own folders and its position in time is dropped: the
    sessions must neither continue a checkpoint nor count the frames from ``T``."""
    results = Path(str(args["results"]))
    path = results / "Checkpoint" / "default_variables.json"
    v: Dict[str, object] = {}
    if path.exists():
        v = json.loads(path.read_text())
    ap = argparse.ArgumentParser(add_help=False)
    add_session_arguments(ap)
    for key in ["restart_folder", "folder", "sub_folder", "t", "counter", *vars(ap.parse_args([]))]:      # the run's own options are not this call's
        v.pop(key, None)
    v.update(args)
    missing = [k for k in NEEDED if v.get(k) is None]
    if missing:
        raise SystemExit(f"{path} not found and no value given for {', '.join(missing)}" if not path.exists() else
                         f"{path} holds no {', '.join(missing)}: give them with --new-arguments")
    v.setdefault("theta", 0.5)
    return v


def frame_window(v: dict):
    """(stride, start, end or None) of --stride, --start-time, --end-time; their use beside the run's own window is refused."""
    given = [k for k in ("stride", "start_time", "end_time") if v.get(k) is not None]
    run_given = [k for k in RUN_WINDOW if v.get(k) is not None]
    if given and run_given:
        dashes = lambda keys: ", ".join("--" + k.replace("_", "-") for k in keys)
        raise SystemExit(f"{dashes(given)} together with {dashes(run_given)}: --stride / --start-time / --end-time select the frames "
                         "of a finished folder that are read, --hi-pass-stride / --hi-pass-start-time / --hi-pass-end-time the "
                         "recorded frames of a run that --hi-pass writes; on a finished folder use --stride / --start-time / "
                         "--end-time, which apply to every option")
    stride = 1 if v.get("stride") is None else v["stride"]
    if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or stride < 1:
        raise SystemExit(f"--stride must be an integer >= 1, got {stride!r}")
    t0 = 0.0 if v.get("start_time") is None else float(v["start_time"])
    t1 = None if v.get("end_time") is None else float(v["end_time"])
    if t0 < 0.0 or (t1 is not None and t1 < t0):
        raise SystemExit(f"--start-time / --end-time: need 0 <= start <= end, got {t0:g} and {t1}")
    return int(stride), t0, t1


def fields_read(v: dict) -> List[str]:
    """The union, in the order d, v, p, of the fields the asked options read (the ``reads`` of their ``*Run`` classes)."""
    need = set()
    for key, module, _, run_cls, _ in SESSIONS:
        if not v.get(key):
            continue
        reads = _session_part(module, run_cls).reads
        need.update(_session_part(module, "quantities")(v) if reads is None else reads(v) if callable(reads) else reads)
    return [q for q in ("d", "v", "p") if q in need]


def default_backend(desc):
    """One context on one GPU, with the smallest Krylov store it takes: nothing is solved in it."""
    from .capi import HipBackend          # raises loudly if libvaspfsi.so or the GPU is missing
    return HipBackend(desc, tuning={"krylov_capacity": KRYLOV_CAPACITY_MIN})


def prepare(argv: Optional[List[str]] = None, backend_factory: Callable = default_backend, out=print):
    """Everything before a context exists: the parameters, the frames that are read, the mesh, every refusal.  Returns
    (ns, mesh, source, indices, fields)."""
    args = parse(argv)
    if not args.get("results"):
        raise SystemExit("--folder: the results folder of a finished run is needed")
    results = Path(str(args["results"]))
    if not results.is_dir():
        raise SystemExit(f"results folder {results} not found")
    world = int(os.environ.get("WORLD_SIZE", 1))
    if world > 1:
        raise SystemExit(f"vasp_amd.postprocess runs on one rank only (WORLD_SIZE = {world})")
    if args.get("hi_pass_spi") and not args.get("hi_pass"):
        raise SystemExit(SPI_NEEDS_HI_PASS)
    if args.get("hi_pass_pod") and not args.get("hi_pass"):
        raise SystemExit(POD_NEEDS_HI_PASS)
    if not args.get("hi_pass") and vortex.refusal(args, []):
        raise SystemExit(vortex.refusal(args, []))
    if not any(args.get(key) for key, *_ in SESSIONS):
        raise SystemExit("nothing to do: give one of " + ", ".join("--" + key.replace("_", "-") for key, *_ in SESSIONS))
    v = parameters(args)
    stride, t0, t1 = frame_window(v)
    source = FrameSource(results)
    fields = fields_read(v)
    source.check_files(fields)
    mesh_path = Path(str(args.get("mesh_path") or results / "Mesh" / "mesh.h5"))      # never the problem's own input mesh
    if not mesh_path.exists():
        raise SystemExit(f"{mesh_path} not found: the mesh of the run (--mesh-path)")
    mesh = FsiMesh.read(mesh_path)
    indices = selected_indices(source.times, float(v["dt"]), stride, t0, t1)
    if fields and len(source):
        n = source.node_count(fields)
        if n not in (mesh.num_vertices, mesh.num_nodes):
            raise SystemExit(f"{source.folder}: a frame has {n} nodes, the mesh {mesh_path} has {mesh.num_vertices} vertices (save_deg 1) "
                             f"and {mesh.num_nodes} P2 nodes (save_deg 2)")
        deg = 2 if n == mesh.num_nodes else 1
        if min(int(v["save_deg"]), 2) != deg:
            out(f"save_deg = {v['save_deg']} in the parameters, the frames of {source.folder} have {n} nodes: read as save_deg {deg}")
        v["save_deg"] = source.save_deg = deg
    # the start time of the written files is --start-time where it was given; without it the options keep their own (--hi-pass-start-time)
    v.update(frame_times=[source.times[k] for k in indices], frame_stride=stride, restart_folder=None,
             frame_start=t0 if v.get("start_time") is not None else None)
    if backend_factory is default_backend:
        from .capi import HipBackend
        cls = HipBackend
    else:
        cls = backend_factory if isinstance(backend_factory, type) else None
    for key, module, refusal, _, _ in SESSIONS:
        why = _session_part(module, refusal)(v, world, cls) if v.get(key) else ""
        if why:
            raise SystemExit(why)
    if v.get("history_memory") is not None and (isinstance(v["history_memory"], bool) or not isinstance(v["history_memory"], (int, np.integer))
                                                or v["history_memory"] < 1):
        raise SystemExit(f"--history-memory must be a number of bytes >= 1, got {v['history_memory']!r}")
    if not indices:
        span = f"its {len(source)} frames run from t = {source.times[0]!r} to {source.times[-1]!r}" if len(source) else "it lists no frame"
        raise SystemExit(f"no saved frame of {source.folder} lies in the window and stride asked for (--stride {stride}, --start-time {t0:g}, "
                         f"--end-time {t1}): {span}")
    if v.get("history_memory") is not None:      # a limit no strip fits into: refused here, in the bytes of hi_pass.host_room, fsi_band_room's twin
        from . import hi_pass_strips as strips
        need = lambda rows, capacity: hi_pass.host_room(rows, capacity)[0]
        band_jobs, amplitude, limit = strips.jobs(mesh, v), bool(v.get("hi_pass_amplitude")), int(v["history_memory"])
        if not strips.everything_fits(band_jobs, len(indices) + 1, amplitude, limit, need):
            if v.get("hi_pass") and v.get("hi_pass_phase_average"):
                raise SystemExit(hi_pass.PHASE_STRIPS)
            if v.get("hi_pass") and v.get("hi_pass_flow_metrics"):
                raise SystemExit(hi_pass.METRICS_STRIPS)
            if v.get("hi_pass") and v.get("hi_pass_vortex"):
                raise SystemExit(vortex.VORTEX_STRIPS)
            if v.get("hi_pass") and v.get("hi_pass_spi"):
                raise SystemExit(hi_pass.SPI_STRIPS)
            if v.get("hi_pass") and v.get("hi_pass_pod"):
                raise SystemExit(hi_pass.POD_STRIPS)
            for j in band_jobs:
                if j.units:
                    strips.plan_strips(j.units, j.rows_per_unit, len(indices) + 1, j.board_bytes(amplitude), limit, need,
                                       "node" if j.kind == "field" else "cell")
        if v.get("spectrogram"):                  # the same for a spectrogram strip, in the bytes of spectrogram.host_room, fsi_spec_room's twin
            from . import spectrogram as sg, spectrogram_strips as spec_strips
            plan = sg.SpectrogramRun(None, mesh, {**v, "results_folder": results}, open_sessions=False)
            for q in plan.quantities:
                magnitude = spec_strips.is_magnitude(plan, q)
                spec_strips.plan_row_strips(plan.rows(q), spec_strips.granule_of(cls), len(indices) + 1, limit,
                                            lambda rows, capacity: sg.host_room(rows, capacity, magnitude)[0])
    build_properties(v)
    ns: Dict[str, object] = dict(v)
    output = Path(str(v.get("output_folder") or results))
    ns.update(default_variables=v, mesh=mesh, results_folder=output, case=results.absolute().parent.name)
    return ns, mesh, source, indices, fields


def run(argv: Optional[List[str]] = None, backend_factory: Callable = default_backend, out=print):
    """Evaluate the asked options over the selected frames; returns the namespace (for tests), with the wall time of the three
    parts of a frame in ``ns["frame_seconds"]``: ``read`` - finding the frame's blocks in the mapped files (opening a file,
    walking its tables; no data is touched), ``set_frame`` - the page faults of the mapping, the host-to-device copy and the
    state kernel, up to the stream synchronise the call ends in -, ``sample``."""
    ns, mesh, source, indices, fields = prepare(argv, backend_factory, out)
    save_deg = int(ns["save_deg"])
    if save_deg < 2:
        out("save_deg 1: the frames hold vertex values, a mid-edge node takes the mean of its edge's two vertices; the cell-based "
            "options (--hemodynamics, --stress-strain, --hi-pass-tensor) differ from an evaluation during the run by that interpolation")
    desc, _, _ = build_description(mesh, ns["default_variables"], [], FormTerms())
    backend = backend_factory(desc)
    ns["backend"] = backend
    Path(ns["results_folder"]).mkdir(parents=True, exist_ok=True)
    # band-pass histories that do not fit the device (or --history-memory) go through their sessions in strips, after the others
    from . import hi_pass_strips as strips
    need = (lambda rows, capacity: backend.hi_pass_room(rows, capacity)[0]) if hasattr(backend, "hi_pass_room") else \
        (lambda rows, capacity: hi_pass.host_room(rows, capacity)[0])
    band_jobs = strips.jobs(mesh, ns) if indices else []
    in_strips, limit = set(), None
    if band_jobs:
        limit = ns.get("history_memory")
        if limit is None:
            limit = (backend.hi_pass_room if hasattr(backend, "hi_pass_room") else hi_pass.host_room)(1, 1)[1]
        if not strips.everything_fits(band_jobs, len(indices) + 1, bool(ns.get("hi_pass_amplitude")), int(limit), need):
            in_strips = {"hi_pass", "hi_pass_tensor"}
            if ns.get("hi_pass") and ns.get("hi_pass_phase_average"):
                raise SystemExit(hi_pass.PHASE_STRIPS)
            if ns.get("hi_pass") and ns.get("hi_pass_flow_metrics"):
                raise SystemExit(hi_pass.METRICS_STRIPS)
            if ns.get("hi_pass") and ns.get("hi_pass_vortex"):
                raise SystemExit(vortex.VORTEX_STRIPS)
            if ns.get("hi_pass") and ns.get("hi_pass_spi"):
                raise SystemExit(hi_pass.SPI_STRIPS)
            if ns.get("hi_pass") and ns.get("hi_pass_pod"):
                raise SystemExit(hi_pass.POD_STRIPS)
    # the same for the spectrogram histories: where they do not fit beside the band-pass sessions of the first frame loop
    spec_run = None
    if ns.get("spectrogram") and indices:
        from . import spectrogram as sg, spectrogram_strips as spec_strips
        if limit is None:
            limit = ns.get("history_memory")
        if limit is None:
            limit = (backend.spec_room if hasattr(backend, "spec_room") else sg.host_room)(1, 1)[1]
        plan = sg.SpectrogramRun(backend, mesh, ns, open_sessions=False)
        beside = 0 if in_strips or not band_jobs else \
            sum(need(j.units * j.rows_per_unit, len(indices) + 1) + j.board_bytes(bool(ns.get("hi_pass_amplitude"))) for j in band_jobs if j.units)
        if spec_strips.total_need(plan, len(indices) + 1) + beside > int(limit):
            spec_run = plan
            in_strips = in_strips | {"spectrogram"}
    band_strips = bool(in_strips & {"hi_pass", "hi_pass_tensor"})
    sessions = []
    for key, module, _, run_cls, needs in SESSIONS:
        if not ns.get(key):
            continue
        if needs and not hasattr(backend, needs):
            raise SystemExit(f"--{key.replace('_', '-')} needs a backend with {needs} ({type(backend).__name__} has none)")
        if key not in in_strips:
            sessions.append(_session_part(module, run_cls)(backend, mesh, ns))
    device = hasattr(backend, "set_frame")
    host_state = {}

    def state():                                  # the host copy of the frame's state, for a session that records on the host
        if "x" not in host_state:
            host_state["x"] = source.state(mesh, host_state["views"])
        return host_state["x"]

    seconds = dict(read=0.0, set_frame=0.0, sample=0.0)
    tick = _time.perf_counter

    def sample_frames(read, samplers):
        """The selected frames, the fields ``read`` of each put into the state and handed to every one of ``samplers``."""
        nonlocal host_state
        t_read = tick()
        for t, views in source.frames(indices, read):
            t_set = tick()
            host_state = dict(views=views)
            if device:
                backend.set_frame("n", **views)
            elif hasattr(backend, "set_state"):
                backend.set_state("n", state())
            t_sample = tick()
            for session in samplers:
                session.sample(t, state)
            t_next = tick()
            seconds["read"] += t_set - t_read
            seconds["set_frame"] += t_sample - t_set
            seconds["sample"] += t_next - t_sample
            t_read = t_next
        host_state = {}

    passes = 0
    try:
        if sessions or not in_strips:
            sample_frames(fields if not in_strips else fields_read({**ns, **{k: None for k in in_strips}}), sessions)
            passes += 1
        for session in sessions:
            session.finish(out)
        for job in (band_jobs if band_strips else []):
            passes += strips.run_quantity(job, backend, mesh, ns, int(limit), need, sample_frames, out)["passes"]
        for q in (spec_run.quantities if spec_run is not None else []):
            passes += spec_strips.run_quantity(q, spec_run, int(limit), sample_frames, out)["passes"]
    finally:
        source.close()
    ns["strips"] = bool(in_strips)
    if indices:
        n = len(indices) * max(passes, 1)
        out("Read %d of %d frames; per frame %.2f ms finding it in the mapped files, %.2f ms reading it into the state (page faults, "
            "host-to-device copy, state kernel), %.2f ms sampling"
            % (len(indices), len(source), *(1e3 * seconds[k] / n for k in ("read", "set_frame", "sample"))))
    ns["frame_seconds"], ns["frames_read"] = seconds, len(indices)
    return ns


def main(argv: Optional[List[str]] = None) -> int:
    ns = run(argv)
    with contextlib.suppress(Exception):
        ns["backend"].close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
