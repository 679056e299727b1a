"""The cases of tests/test_gpu_window_stop.py (early termination of the windowed schedule,
td_set_window_stop) are not vacuous: on the CPU oracle alone (pyoracle.turbo_decode_window's rows
through the numpy rules), each case's stop counts are the spread it was built for -- several distinct
counts in a batch, a ragged second wave of 64 that finishes while the first goes on, frames that never
pass their CRC.  The spreads are conditions on the inputs, not tolerances."""
import numpy as np
import pytest

import window_stop_cases as W
from window_stop_cases import CRC24B, ITERS, crc24, spread, stops


@pytest.mark.parametrize("algo,precision,want", [
    ("logmap", "f64", {2: 10, 3: 27, 4: 12, 5: 9, 6: 2, 7: 2, 8: 8}),
    ("logmap", "f32", {2: 10, 3: 27, 4: 12, 5: 8, 6: 2, 7: 3, 8: 8}),
    ("maxlog", "f64", {2: 10, 3: 10, 4: 5, 5: 4, 6: 3, 8: 38}),
])
def test_case_a(algo, precision, want):
    rows = W.synth_case("A", 0.0, 70, algo, precision)[1]
    used = stops(rows, "hda")
    assert spread(used) == want
    if algo == "logmap":   # the wave-exit case: the ragged second wave all stops at 3, wave 0 runs to 8
        assert np.all(used[64:] == 3) and used[:64].max() == ITERS


def test_case_a_min_iters():
    rows = W.synth_case("A", 0.0, 70)[1]
    assert spread(stops(rows, "hda", 4)) == {4: 46, 5: 10, 6: 3, 7: 2, 8: 9}
    assert np.all(stops(rows, "hda", ITERS) == ITERS)


@pytest.mark.parametrize("sched,ebn0,B,want", [
    ("B", 0.0, 70, {2: 4, 3: 14, 4: 19, 5: 12, 6: 8, 7: 6, 8: 7}),
    ("C", 0.5, 70, {3: 8, 4: 17, 5: 8, 6: 6, 7: 6, 8: 25}),
    ("D", 1.0, 19, {3: 3, 4: 10, 5: 6}),
    ("D", 0.5, 19, {4: 4, 5: 5, 6: 3, 7: 2, 8: 5}),
    ("E", 1.0, 9, {4: 5, 5: 4}),
])
def test_hda_cases(sched, ebn0, B, want):
    assert spread(stops(W.synth_case(sched, ebn0, B)[1], "hda")) == want


def test_case_e_maxlog():
    assert spread(stops(W.synth_case("E", 1.0, 9, "maxlog")[1], "hda")) == {4: 2, 5: 5, 6: 2}


def test_crc_cases():
    rows = W.crc_case("A", CRC24B, 1.2, 70)[1]
    assert spread(stops(rows, "crc")) == {1: 13, 2: 18, 3: 5, 4: 4, 6: 1, 8: 29}
    assert sum(crc24(r[-1], CRC24B) != 0 for r in rows) == 29   # frames that never pass
    rows = W.crc_case("D", CRC24B, 1.1, 19)[1]
    assert spread(stops(rows, "crc")) == {2: 4, 3: 13, 4: 2}


def test_abi_declares_and_exports_the_switch():
    """td_set_window_stop is declared in the header, exported by the library, and rejects a null handle
    (the checks that need a handle run on the GPU: test_gpu_window_stop.py::test_interface)."""
    import ctypes as C
    import os

    from conftest import REPO
    from turbo_decoder_cuda_amd import _native as N
    header = open(os.path.join(REPO, "include", "turbo_mi355x.h")).read()
    assert "int td_set_window_stop(td_handle* h, const td_stop_params* s);" in header
    assert "td_set_window_stop" in N.EXPORTS and hasattr(N.lib(), "td_set_window_stop")
    s = N.TdStopParams(N.TD_STOP_HDA, 1, 0)
    assert N.lib().td_set_window_stop(None, C.byref(s)) == N.TD_EINVAL
    assert b"td_set_window_stop" in N.lib().td_last_error()


@pytest.mark.parametrize("sched,B,want", [("D", 6, [4, 3, 4, 4, 5, 3]), ("Dn", 6, [7, 5, 7, 7, 8, 5]), ("E", 2, [4, 5])])
def test_single_frames(sched, B, want):
    """The frames the B = 1 tests decode one at a time (a codeword's oracle rows do not depend on its batch)."""
    full = 19 if sched in ("D", "Dn") else 9
    rows = W.synth_case(sched, 1.0, full)[1][:B]
    assert stops(rows, "hda").tolist() == want
