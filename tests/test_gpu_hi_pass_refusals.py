"""The first refusal of every ``HipBackend.hi_pass_*`` method that takes a quantity, word for word (csrc/fsi_sessions.hip: the
fsi_band_* entry points).  The order in which an entry point looks at its context, its quantity and its session differs from one
to the next and is part of the interface, so each text is written out here and not put together: a quantity out of range, no
open session, a session of p handed to a call of a vector on P2 nodes, a strain session handed to a call of a vector or a scalar,
and the calls that come before the call they need.  No kernel result is compared."""
import numpy as np
import pytest

from test_hi_pass_ladder import A, B, FRAMES, ZI

pytestmark = pytest.mark.gpu

NODES = 66
RANGE5 = "quantity must be 0 (d), 1 (v), 2 (p), 3 (strain) or 4 (stress)"
NO_SESSION = "no band-pass session for this quantity (fsi_band_begin first)"
VECTOR = "quantity must be 0 (d) or 1 (v)"
# method -> (entry point, the call, the text behind "<entry point>: " of: a quantity out of range, no open session, a session
# of p where a vector is needed, a strain session where a vector or a scalar is needed); None: the method has no such refusal
CALLS = {
    "begin": ("fsi_band_begin", lambda hb, q: hb.hi_pass_begin(q, [0], None, 1), "quantity must be 0 (d), 1 (v) or 2 (p)", None, None, None),
    "begin_cells": ("fsi_band_begin_cells", lambda hb, q: hb.hi_pass_begin_cells(q, hb.two_solid_cells, 1),
                    "quantity must be 3 (strain) or 4 (stress)", None, None, None),
    "sample": ("fsi_band_sample", lambda hb, q: hb.hi_pass_sample(q), RANGE5, NO_SESSION, None, None),
    "filter": ("fsi_band_filter", lambda hb, q: hb.hi_pass_filter(q, B, A, ZI, 0), RANGE5, NO_SESSION, None, None),
    "select": ("fsi_band_select", lambda hb, q: hb.hi_pass_select(q), RANGE5, NO_SESSION, None, None),
    "filter_next": ("fsi_band_filter_next", lambda hb, q: hb.hi_pass_filter_next(q, B, A, ZI, 0), RANGE5, NO_SESSION, None, None),
    "trace": ("fsi_band_trace", lambda hb, q: hb.hi_pass_trace(q, "raw", [0]), RANGE5, NO_SESSION, None,
              "a strain / stress session has no point traces"),
    "amplitude": ("fsi_band_amplitude", lambda hb, q: hb.hi_pass_amplitude(q, 0), RANGE5, NO_SESSION, None, None),
    "phase": ("fsi_band_phase", lambda hb, q: hb.hi_pass_phase(q, 1), RANGE5, NO_SESSION, None, None),
    "phase_fetch": ("fsi_band_phase_fetch", lambda hb, q: hb.hi_pass_phase_fetch(q, "energy", 0), RANGE5, NO_SESSION, None,
                    "a strain / stress session has no energy: 0.5 |u'|^2 is that of a vector or a scalar"),
    "spi": ("fsi_band_spi", lambda hb, q: hb.hi_pass_spi(q, None, 0, 1), RANGE5, NO_SESSION, None,
            "a strain / stress session has no spectral power index: it is that of a vector or a scalar (d, v, p)"),
    "spi_fetch": ("fsi_band_spi_fetch", lambda hb, q: hb.hi_pass_spi_fetch(q), RANGE5, NO_SESSION, None, None),
    "pod_gram": ("fsi_band_pod_gram", lambda hb, q: hb.hi_pass_pod_gram(q), RANGE5, NO_SESSION, None,
                 "a strain / stress session has no proper orthogonal decomposition: it is that of a vector or a scalar (d, v, p)"),
    "pod_modes": ("fsi_band_pod_modes", lambda hb, q: hb.hi_pass_pod_modes(q, np.ones((hb.selected(q), 1))), RANGE5, NO_SESSION, None, None),
    "pod_fetch": ("fsi_band_pod_fetch", lambda hb, q: hb.hi_pass_pod_fetch(q, "gram"), RANGE5, NO_SESSION, None, None),
    "cells": ("fsi_band_cells", lambda hb, q: hb.hi_pass_cells(q, [3, 11]),
              VECTOR + ": the strain rate is that of a vector on P2 nodes", NO_SESSION, VECTOR + ": the strain rate is that of a vector on P2 nodes", None),
    "cell_rate": ("fsi_band_cell_rate", lambda hb, q: hb.hi_pass_cell_rate(q, "raw"), VECTOR, NO_SESSION, VECTOR, None),
    "cell_rate_current": ("fsi_band_cell_rate_current", lambda hb, q: hb.hi_pass_cell_rate_current(q, "raw"), VECTOR, NO_SESSION, VECTOR, None),
    "cell_weights": ("fsi_band_cell_weights", lambda hb, q: hb.hi_pass_cell_weights(q, [1.0, 1.0]), VECTOR, NO_SESSION, VECTOR, None),
    "cell_vortex": ("fsi_band_cell_vortex", lambda hb, q: hb.hi_pass_cell_vortex(q, "raw"), VECTOR, NO_SESSION, VECTOR, None),
    "cell_vortex_current": ("fsi_band_cell_vortex_current", lambda hb, q: hb.hi_pass_cell_vortex_current(q, "raw"), VECTOR, NO_SESSION, VECTOR, None),
    "fetch": ("fsi_band_fetch", lambda hb, q: hb.hi_pass_fetch(q, "raw", 0), RANGE5, NO_SESSION, None, None),
    "export": ("fsi_band_export", lambda hb, q: hb.hi_pass_export(q, 0, 1), RANGE5, NO_SESSION, None, None),
    "import": ("fsi_band_import", lambda hb, q: hb.hi_pass_import(q, np.zeros((1, 1, 3))), RANGE5, NO_SESSION, None, None),
    "end": ("fsi_band_end", lambda hb, q: hb.hi_pass_end(q), RANGE5, None, None, None),      # the end of no session is no error
    "board_attach": ("fsi_band_board_attach", lambda hb, q: hb.hi_pass_board_attach(q, -1), RANGE5, NO_SESSION, None, None),
}
SITUATIONS = ("out-of-range", "no-session", "session-of-p", "strain-session")
ROWS = [(name, k) for name, row in CALLS.items() for k in range(4) if row[2 + k] is not None]


@pytest.fixture(scope="module")
def hb(cylinder_case):
    from vasp_amd.capi import HipBackend
    backend = HipBackend(cylinder_case[1])
    backend.BAND_QUANTITY = dict(HipBackend.BAND_QUANTITY, beyond=7)      # this instance's: a name for a quantity out of range
    backend.two_solid_cells = np.nonzero(np.asarray(cylinder_case[1]["cell_kind"]) == 1)[0][:2]
    backend.selected = lambda q: backend._band.get(q, backend.NO_BAND)["selected"] or 1
    yield backend
    backend.close()


def refusal(call) -> str:
    from vasp_amd.capi import FsiError
    with pytest.raises(FsiError) as e:
        call()
    assert e.value.code == 1
    return str(e.value).split(": ", 1)[1]


def test_every_method_that_takes_a_quantity_is_in_the_table():
    from vasp_amd.capi import HipBackend
    import inspect
    takes = {n[len("hi_pass_"):] for n, f in inspect.getmembers(HipBackend, inspect.isfunction)
             if n.startswith("hi_pass_") and "quantity" in inspect.signature(f).parameters}
    assert takes == set(CALLS)


@pytest.mark.parametrize("name,k", ROWS, ids=[f"{n}-{SITUATIONS[k]}" for n, k in ROWS])
def test_the_first_refusal_of_a_method(hb, name, k):
    fn, call, *texts = CALLS[name]
    rng = np.random.default_rng(22)
    try:
        if k == 2:
            hb.hi_pass_begin("p", np.arange(NODES, dtype=np.int32), None, FRAMES)
            hb.hi_pass_import("p", rng.standard_normal((FRAMES, NODES, 1)))
        if k == 3:                                    # two whole cycles of one frame, so that a phase average stands
            hb.hi_pass_begin_cells("strain", hb.two_solid_cells, 2)
            hb.hi_pass_import("strain", rng.standard_normal((2, 8, 6)))
            hb.hi_pass_phase("strain", 1)
        assert refusal(lambda: call(hb, ("beyond", "v", "p", "strain")[k])) == f"{fn}: {texts[k]}"
    finally:
        hb.hi_pass_end("p")
        hb.hi_pass_end("strain")


def test_the_calls_that_come_too_early(hb, cylinder_case):
    """On a session of v with 12 imported frames: on 66 nodes, then on every P2 node with two cells attached."""
    mesh = cylinder_case[0]["mesh"]
    rng = np.random.default_rng(23)
    try:
        hb.hi_pass_begin("v", np.arange(NODES, dtype=np.int32), None, FRAMES)
        hb.hi_pass_import("v", rng.standard_normal((FRAMES, NODES, 3)))
        assert refusal(lambda: hb.hi_pass_filter_next("v", B, A, ZI, 0)) == "fsi_band_filter_next: no filtered series (fsi_band_filter first)"
        hb.hi_pass_filter("v", B, A, ZI, 0)
        assert refusal(lambda: hb.hi_pass_fetch("v", "amplitude", 0)) == "fsi_band_fetch: no amplitude (fsi_band_amplitude first)"
        assert refusal(lambda: hb.hi_pass_spi("v", None, 1, 1)) == \
            "fsi_band_spi: a slab out of order: bin0 = 1, no slab stands before it (bin0 = 0 first)"
        assert refusal(lambda: hb.hi_pass_pod_modes("v", np.ones((FRAMES, 1)))) == "fsi_band_pod_modes: no Gram matrix (fsi_band_pod_gram first)"
        assert refusal(lambda: hb.hi_pass_cell_rate("v", "raw")) == "fsi_band_cell_rate: no cell list (fsi_band_cells first)"
        hb.hi_pass_begin("v", np.arange(mesh.num_nodes, dtype=np.int32), None, FRAMES)
        hb.hi_pass_import("v", rng.standard_normal((FRAMES, mesh.num_nodes, 3)))
        hb.hi_pass_cells("v", [3, 11])
        assert refusal(lambda: hb.hi_pass_cell_vortex("v", "raw", cells=False, sums=True)) == \
            "fsi_band_cell_vortex: sums_out without weights (fsi_band_cell_weights first)"
        assert refusal(lambda: hb.hi_pass_cell_rate_current("v", "raw")) == \
            "fsi_band_cell_rate_current: no session of quantity 0 (d): the current configuration is x = X + d (fsi_band_begin of d first)"
    finally:
        hb.hi_pass_end("v")


PARTITIONED = ("phase", "phase_fetch", "spi", "spi_fetch", "pod_gram", "pod_modes", "pod_fetch", "cells", "cell_rate", "cell_rate_current",
               "cell_weights", "cell_vortex", "cell_vortex_current", "export", "import", "board_attach")


def test_a_partitioned_context_is_refused_before_the_quantity_is_looked_at(cylinder_case):
    """A context told that it is one part of a partition (every cell owned, nothing shared: no call of this test reaches a
    collective), as tests/test_gpu_hi_pass_pod.py sets one up: the entry points that refuse it do so first, also where the
    quantity is out of range."""
    import ctypes as C
    from vasp_amd.capi import HipBackend
    red = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int32)(lambda user, v, n: 0)
    halo = C.CFUNCTYPE(C.c_int, C.c_void_p)(lambda user: 0)

    class FsiComm(C.Structure):
        _fields_ = [("user", C.c_void_p), ("allreduce_sum", type(red)), ("halo_exchange", type(halo))]

    comm = FsiComm(None, red, halo)
    backend = HipBackend(cylinder_case[1])
    backend.BAND_QUANTITY = dict(HipBackend.BAND_QUANTITY, beyond=7)
    backend.two_solid_cells = None
    backend.selected = lambda q: 1
    try:
        backend._check(backend.lib.fsi_set_partition(backend.ctx, len(backend.cell_u2i), 0, None, 0, None, 0, None, None, None, C.byref(comm)))
        for name in PARTITIONED:
            assert refusal(lambda: CALLS[name][1](backend, "beyond")) == f"{CALLS[name][0]}: partitioned contexts are not supported", name
        for name in set(CALLS) - set(PARTITIONED) - {"begin", "begin_cells"}:      # these never ask, and look for the quantity
            assert refusal(lambda: CALLS[name][1](backend, "beyond")) == f"{CALLS[name][0]}: {CALLS[name][2]}", name
    finally:
        backend.close()
