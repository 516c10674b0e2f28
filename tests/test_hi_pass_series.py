"""Where a series of a band-pass session lies, on the NumPy twin (vasp_amd/hi_pass.py: HostBandSession.series, the twin of
series_view in csrc/fsi_sessions.hip): the selected raw frames, the filtered series, the period's mean frames - and that a
series which does not stand is refused by the callers that own the refusal, in their words."""
import numpy as np
import pytest

from test_hi_pass_ladder import A, B, CONN, FRAMES, GRAD, NODES, X, ZI, same_bits
from vasp_amd import hi_pass as hp


def session():
    s = hp.HostBandSession(3, FRAMES)
    s.import_(X)
    return s


def test_raw_is_the_strided_selection():
    s = session()
    assert s.select(1, 5, 2) == 5
    assert same_bits(s.series("raw"), X[1:10:2])


def test_series_is_the_array_a_filtered_trace_reads():
    s = session()
    s.select(1, 5, 2)
    s.filter(B, A, ZI, 0)
    assert s.series("series").shape == (5, NODES, 3)
    assert same_bits(s.series("series"), hp.filtfilt_rows(B, A, X[1:10:2], ZI, 0))
    assert same_bits(s.series("series").transpose(1, 0, 2), s.trace("filtered", range(NODES))[:, :, 1:])
    assert same_bits(s.series("raw"), X[1:10:2])          # the selection stands under its filtered series


def test_phase_mean_is_what_phase_fetch_returns():
    s = session()
    s.select(2, 8, 1)
    s.phase(4)
    assert s.series("phase_mean").shape == (4, NODES, 3)
    for j in range(4):
        assert same_bits(s.series("phase_mean")[j], s.phase_fetch("mean", j))
    assert same_bits(s.series("series"), X[2:10] - np.tile(s.series("phase_mean"), (2, 1, 1)))      # the fluctuation is the series


def test_a_series_that_does_not_stand_is_refused_by_its_callers():
    s = session()
    s.cells(CONN[0], GRAD[0])
    assert s.series("series") is None and s.series("phase_mean") is None
    for text, call in (("hi-pass trace: no filtered series (filter first)", lambda: s.trace("filtered", [0])),
                       ("hi-pass filter_next: no filtered series (filter first)", lambda: s.filter_next(B, A, ZI, 0)),
                       ("hi-pass pod_gram: no filtered series (filter or phase first)", lambda: s.pod_gram("series")),
                       ("hi-pass cell_rate: no filtered series (filter or phase first)", lambda: s.cell_rate("series")),
                       ("hi-pass cell_rate: no phase average (phase first)", lambda: s.cell_rate("phase_mean")),
                       ("hi-pass phase_fetch: no phase average (phase first)", lambda: s.phase_fetch("mean", 0))):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == text
