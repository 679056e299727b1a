"""The fixed-point decoder's lane code (csrc/td_fixed_core.h, what a lane of the gfx950 kernels runs) as a
stand-alone host program under ASan + UBSan: the one build and the one run that the test_fixed_*_host.py
files share.  tests/fixed_core_host.cpp is the program, a child process with its own main; nothing is
loaded into this interpreter."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

SAN = ["-fsanitize=address", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"]
SENTINEL = 0x5a5a            # the program's Le where nothing was written
RULES = {None: 0, "hda": 1, "crc": 2}


_EXE = []


def build(tmp_path_factory):
    """Compile tests/fixed_core_host.cpp once a test session, under pytest's own temporary directory; the
    executable's path."""
    if not _EXE:
        exe = str(tmp_path_factory.mktemp("fixed_core") / "fixed_core_host")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *SAN, f"-I{REPO}/turbo_decoder_cuda_amd/csrc",
                               os.path.join(REPO, "tests", "fixed_core_host.cpp"), "-o", exe])
        _EXE.append(exe)
    return _EXE[0]


@pytest.fixture(scope="module")
def core_host(tmp_path_factory):
    return build(tmp_path_factory)


def run_core(exe, tmp_path, q, pi, iters, all_iters, setting, win=None, rule=None, min_iters=1, poly=0, tab=None,
             nii=False, timeout=300):
    """One decode of the batch q [B][3K+12] by the program: the exact schedule (win None) or the sub-block one
    (win = (window, overlap)), a stop rule or none, Max-Log-MAP (tab None) or tab = (shift, corr[8]), NII on or
    off.  Returns the rows [B][rows][K], Le [B][iters][2][K+3] and the iterations used [B] (without a rule:
    iters)."""
    B, K = q.shape[0], len(pi)
    L, rows = K + 3, iters if all_iters else 1
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    shift, corr = tab if tab is not None else (0, (0,) * 8)
    with open(fin, "wb") as f:
        f.write(np.array([K, iters, int(all_iters), *setting, B, *(win or (0, 0)), RULES[rule], min_iters, poly,
                          int(tab is not None), shift, *corr, int(nii)], dtype=np.int32).tobytes())
        f.write(np.asarray(pi).astype(np.int32).tobytes())
        f.write(np.ascontiguousarray(q).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        (r.returncode, r.stderr[-3000:])
    raw = np.fromfile(fout, dtype=np.uint8)
    nb, nl = B * rows * K, B * iters * 2 * L * 2
    return (raw[:nb].reshape(B, rows, K), raw[nb:nb + nl].view(np.int16).reshape(B, iters, 2, L),
            raw[nb + nl:].view(np.int32))
