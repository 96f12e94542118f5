"""The host side of block CSR (spmv_bsr_plan, spmv_bsr_fill, spmv_cpu_bsr,
host/bsr.c) compiled with ASan + UBSan into a stand-alone program (its own
main, nothing preloaded) and driven over the fixtures for every block size
with exactly-sized buffers, sizes that are no multiple of the block size and
the refused inputs (tests/san/bsr_harness.c; `make test-san-bsr` runs the
same)."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, REPO


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc with libasan")
def test_bsr_harness_under_asan_ubsan():
    subprocess.run(["make", "-C", str(REPO), "build/san/bsr_harness"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=99", OMP_NUM_THREADS="4")
    files = sorted(str(p) for p in GOLDEN.glob("*.mtx"))
    assert len(files) > 10
    r = subprocess.run([str(REPO / "build" / "san" / "bsr_harness"), *files], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert f"bsr harness: {len(files)} files" in r.stdout and "calls clean" in r.stdout
