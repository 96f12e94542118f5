"""The host statements of BiCGSTAB's two fused vector updates
(spmv_cpu_bicgstab_update_multi, spmv_cpu_bicgstab_dir_multi, host/bicgstab.c)
compiled with ASan + UBSan into a stand-alone program (its own main, nothing
preloaded) and driven with exactly-sized buffers, ld == k and ld > k, Sh == R,
zero denominators and n = 0 (tests/san/bicgstab_harness.c;
`make test-san-bicgstab` runs the same)."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from conftest import REPO


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc with libasan")
def test_bicgstab_harness_under_asan_ubsan():
    subprocess.run(["make", "-C", str(REPO), "build/san/bicgstab_harness"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=99", OMP_NUM_THREADS="4")
    r = subprocess.run([str(REPO / "build" / "san" / "bicgstab_harness")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "bicgstab harness:" in r.stdout and "calls clean" in r.stdout
