"""The host statements of GMRES's three basis kernels (spmv_cpu_krylov_project,
spmv_cpu_krylov_combine, spmv_cpu_krylov_normalize; host/krylov.c) compiled with
ASan + UBSan into a stand-alone program (its own main, nothing preloaded) and
driven with exactly-sized buffers, ld == width and ld > width, w_out == w,
w_out a column of the basis' allocation, s = 0, n = 0 and the refused inputs
(tests/san/krylov_harness.c; `make test-san-krylov` runs the same)."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from conftest import REPO


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc with libasan")
def test_krylov_harness_under_asan_ubsan():
    subprocess.run(["make", "-C", str(REPO), "build/san/krylov_harness"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=99", OMP_NUM_THREADS="4")
    r = subprocess.run([str(REPO / "build" / "san" / "krylov_harness")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "krylov harness:" in r.stdout and "calls clean" in r.stdout
