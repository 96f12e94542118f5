"""The balanced multi-vector CSR run (spmv_plan_prepare_multi), the parts that
need no GPU: the C-ABI symbols and their NULL-plan answers, the host planner
spmv_csr_multi_plan against a numpy restatement of its definition
(include/spmv_host.h), its refusals, the binding's own checks and the
sanitizer harness tests/san/multi_plan_harness.c.
"""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import exact
import spmv_amd as sa
from conftest import GOLDEN, golden_cases

REPO = Path(__file__).resolve().parents[1]
CASES = [c["name"] for c in golden_cases()]
SMALL_OPTS = [(4, 8), (0, 3), (0, 1)]

HIP_NEW = ("spmv_multi_opts_init", "spmv_plan_prepare_multi", "spmv_plan_get_multi_info")
HOST_NEW = ("spmv_csr_multi_plan",)


def test_symbols_exported_and_bound():
    hip = ctypes.CDLL(str(sa.LIB_DIR / "libspmv_hip.so"))
    host = ctypes.CDLL(str(sa.LIB_DIR / "libspmv_host.so"))
    for name in HIP_NEW:
        assert name in sa.HIP_SYMBOLS and hasattr(hip, name)  # found by its C name
        assert getattr(sa.hip_lib(), name).argtypes == sa.HIP_SYMBOLS[name][1]
    for name in HOST_NEW:
        assert name in sa.HOST_SYMBOLS and hasattr(host, name)
        assert getattr(sa.host_lib(), name).argtypes == sa.HOST_SYMBOLS[name][1]
    header = (REPO / "include" / "spmv.h").read_text()
    for name in HIP_NEW + ("SPMV_M_NONE = 0", "SPMV_M_BALANCED = 1", "spmv_multi_opts", "spmv_multi_info"):
        assert name in header, name
    assert "spmv_csr_multi_plan" in (REPO / "include" / "spmv_host.h").read_text()
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    P = ctypes.POINTER
    assert sa.HIP_SYMBOLS["spmv_multi_opts_init"] == (None, [P(sa.MultiOpts)])
    assert sa.HIP_SYMBOLS["spmv_plan_prepare_multi"] == (ctypes.c_int, [vp, ctypes.c_int, P(sa.MultiOpts)])
    assert sa.HIP_SYMBOLS["spmv_plan_get_multi_info"] == (ctypes.c_int, [vp, P(sa.MultiInfo)])
    assert sa.HOST_SYMBOLS["spmv_csr_multi_plan"] == \
        (ctypes.c_int, [i64, vp, i32, i32, P(i64), P(i64), P(i64), vp, vp, vp, vp, vp])
    assert ctypes.sizeof(sa.MultiOpts) == 8
    assert ctypes.sizeof(sa.MultiInfo) == 144 == 4 * 4 + 8 * 8 + 64
    assert sa.MULTI_MODES == {None: 0, "balanced": 1}


def test_null_plan_answers():
    lib = sa.hip_lib()
    info, o = sa.MultiInfo(), sa.MultiOpts(7, 7)
    lib.spmv_multi_opts_init(ctypes.byref(o))
    assert (o.long_len, o.seg_len) == (-1, -1)
    lib.spmv_multi_opts_init(None)  # tolerated, as spmv_plan_opts_init
    for mode in (0, 1, 99):
        assert lib.spmv_plan_prepare_multi(None, mode, ctypes.byref(o)) == sa.OTHER_ERROR
        assert b"NULL" in lib.spmv_last_error()
    assert lib.spmv_plan_prepare_multi(None, 1, None) == sa.OTHER_ERROR
    assert lib.spmv_plan_get_multi_info(None, ctypes.byref(info)) == sa.OTHER_ERROR
    assert b"NULL" in lib.spmv_last_error()


# ------------------------------------------------------------- the planner
def restate(ptr, long_len, seg_len):
    """The definition, row by row: -> the tables as lists."""
    seg_beg, seg_cnt, seg_dest, long_row, long_first = [], [], [], [], []
    slot = 0
    for r in range(ptr.size - 1):
        b, e = int(ptr[r]), int(ptr[r + 1])
        if e - b <= long_len:
            continue
        long_row.append(r)
        long_first.append(slot)
        starts = list(range(b, e, seg_len))
        for s in starts:
            seg_beg.append(s)
            seg_cnt.append(min(seg_len, e - s))
            if len(starts) == 1:
                seg_dest.append(r)
            else:
                seg_dest.append(~slot)
                slot += 1
    return seg_beg, seg_cnt, seg_dest, long_row + [-1], long_first + [slot]


def check_plan(n_rows, ptr, long_len, seg_len, what):
    ptr = np.ascontiguousarray(ptr, np.int64)
    counts = sa.csr_multi_plan(n_rows, ptr, long_len, seg_len, counts_only=True)
    p = sa.csr_multi_plan(n_rows, ptr, long_len, seg_len)
    assert {k: p[k] for k in counts} == counts, f"{what}: the NULL call counts differently"
    want = restate(ptr, long_len, seg_len)
    for k, w in zip(("seg_beg", "seg_cnt", "seg_dest", "long_row", "long_first"), want):
        assert p[k].tolist() == w, f"{what}: {k}"
    assert p["seg_beg"].dtype == np.int64 and all(p[k].dtype == np.int32 for k in ("seg_cnt", "seg_dest", "long_row"))
    lens = np.diff(ptr)
    assert p["n_long"] == int((lens > long_len).sum()) == p["long_row"].size - 1
    assert p["n_seg"] == p["seg_beg"].size and p["n_slots"] == int((p["seg_dest"] < 0).sum())
    # the invariants once more, from the tables alone: every entry of every long
    # row in exactly one segment, segments in order, all but a row's last full
    cover = np.zeros(int(ptr[-1]) + 1, np.int64)
    np.add.at(cover, p["seg_beg"], 1)
    np.add.at(cover, p["seg_beg"] + p["seg_cnt"], -1)
    in_long = np.zeros(int(ptr[-1]) + 1, np.int64)
    np.add.at(in_long, ptr[:-1][lens > long_len], 1)
    np.add.at(in_long, ptr[1:][lens > long_len], -1)
    assert np.array_equal(np.cumsum(cover), np.cumsum(in_long)), f"{what}: coverage"
    assert (np.diff(p["seg_beg"]) > 0).all() and (p["seg_cnt"] >= 1).all() and (p["seg_cnt"] <= seg_len).all()
    ends_row = np.isin(p["seg_beg"] + p["seg_cnt"], ptr[1:][lens > long_len])
    assert (p["seg_cnt"][~ends_row] == seg_len).all(), f"{what}: a short segment inside a row"
    slots = ~p["seg_dest"][p["seg_dest"] < 0]
    assert np.array_equal(slots, np.arange(p["n_slots"])), f"{what}: slots not consecutive"
    return p


@pytest.mark.parametrize("opts", SMALL_OPTS, ids=lambda o: f"{o[0]}-{o[1]}")
@pytest.mark.parametrize("name", CASES)
def test_planner_golden(name, opts):
    m = sa.read_mtx(GOLDEN / f"{name}.mtx")
    ptr, _, _ = sa.csr_from_coo(m)
    p = check_plan(m.n_rows, ptr, *opts, what=f"{name} {opts}")
    if name == "all_empty":
        assert (p["n_long"], p["n_seg"], p["n_slots"]) == (0, 0, 0) and p["long_first"].tolist() == [0]


def test_planner_long_inputs():
    m = sa.read_mtx(GOLDEN / "long_rows.mtx")
    ptr, _, _ = sa.csr_from_coo(m)
    lens = np.diff(ptr)
    assert sorted(lens[lens > 128].tolist()) == [1500, 5000]
    p = check_plan(m.n_rows, ptr, 128, 1024, "long_rows")
    assert (p["n_long"], p["n_seg"], p["n_slots"]) == (2, 7, 7)
    for key in ("one_row", "rmat"):
        g = exact.generated(key)
        ptr, _, _ = sa.csr_from_coo(g)
        p = check_plan(g.n_rows, ptr, 128, 1024, key)
        if key == "one_row":
            assert (p["n_long"], p["n_seg"], p["n_slots"]) == (1, 20, 20) and p["seg_cnt"][-1] == 20_001 - 19 * 1024
        else:
            assert p["n_long"] > 0 and p["n_slots"] > 0 and (p["seg_dest"] >= 0).any()


def test_planner_hand_made_edges():
    """Rows of exactly long_len, long_len + 1, seg_len, seg_len + 1, 2 seg_len
    and 2 seg_len + 1 entries, empty rows between them, a long last row."""
    for long_len, seg_len in ((4, 8), (8, 8), (0, 3), (3, 1), (100, 8)):
        lens = [long_len, 0, long_len + 1, 0, 0, seg_len, seg_len + 1, 0, 2 * seg_len, 2 * seg_len + 1, 0, 1,
                5 * seg_len + long_len + 2]
        ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        p = check_plan(len(lens), ptr, long_len, seg_len, f"edges ({long_len}, {seg_len})")
        assert p["long_row"][-2] == len(lens) - 1
        by_row = {r: int(f1 - f0) for r, f0, f1 in zip(p["long_row"][:-1], p["long_first"][:-1], p["long_first"][1:])}
        for r, n in enumerate(lens):
            if n > long_len:
                segs = -(-n // seg_len)
                assert by_row[r] == (segs if segs > 1 else 0), (long_len, seg_len, r)
            else:
                assert r not in by_row


def test_planner_refusals_write_nothing():
    lens = [3, 0, 9, 20, 1]
    ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    bad = ptr.copy()
    bad[2] = ptr[-1] + 1
    f = sa.host_lib().spmv_csr_multi_plan
    cnt = np.full(3, 0x5A5A5A5A, np.int64)
    sb = np.full(64, 0x5A5A5A5A, np.int64)
    i32 = np.full((4, 65), 0x5A5A5A5A, np.int32)
    before = [a.copy() for a in (cnt, sb, i32)]
    c = [cnt[i:].ctypes.data for i in range(3)]
    P64 = ctypes.POINTER(ctypes.c_int64)

    def call(n_rows=5, p=ptr, long_len=0, seg_len=3, c0=c[0], arrays=None):
        arrays = [sb.ctypes.data] + [i32[i].ctypes.data for i in range(4)] if arrays is None else arrays
        cs = [ctypes.cast(v, P64) if v else None for v in (c0, c[1], c[2])]
        return f(n_rows, p.ctypes.data if p is not None else None, long_len, seg_len, *cs, *arrays)

    some = [sb.ctypes.data, None, i32[1].ctypes.data, i32[2].ctypes.data, i32[3].ctypes.data]
    for what, rc in {
        "n_rows < 0": call(n_rows=-1), "NULL row_ptr": call(p=None), "decreasing row_ptr": call(p=bad),
        "long_len < 0": call(long_len=-1), "seg_len = 0": call(seg_len=0), "seg_len < 0": call(seg_len=-3),
        "NULL count": call(c0=None), "some arrays NULL": call(arrays=some),
    }.items():
        assert rc == sa.OTHER_ERROR, what
        for a, b in zip((cnt, sb, i32), before):
            assert np.array_equal(a, b), f"{what}: a refused call wrote an output"
    assert call() == sa.SUCCESS and cnt.tolist() == [4, 1 + 3 + 7 + 1, 3 + 7]
    # the wrapper's own check and the error path through it
    with pytest.raises(sa.SpmvError) as e:
        sa.csr_multi_plan(4, ptr, 0, 3)
    assert e.value.rc == sa.OTHER_ERROR
    for kw in ({"long_len": -1, "seg_len": 3}, {"long_len": 0, "seg_len": 0}):
        with pytest.raises(sa.SpmvError) as e:
            sa.csr_multi_plan(5, ptr, **kw)
        assert e.value.rc == sa.OTHER_ERROR
    with pytest.raises(sa.SpmvError):
        sa.csr_multi_plan(5, bad, 0, 3)


def test_too_many_segments_refused():
    """2^31 segments of one entry: refused from the offsets alone, nothing written."""
    ptr = np.array([0, 1 << 31], np.int64)
    with pytest.raises(sa.SpmvError) as e:
        sa.csr_multi_plan(1, ptr, 0, 1, counts_only=True)
    assert e.value.rc == sa.OTHER_ERROR
    assert sa.csr_multi_plan(1, ptr, 0, 2, counts_only=True) == {"n_long": 1, "n_seg": 1 << 30, "n_slots": 1 << 30}
    assert sa.csr_multi_plan(1, np.array([0, (1 << 31) - 1], np.int64), 0, 1, counts_only=True)["n_seg"] == (1 << 31) - 1


# ------------------------------------------------------------ the binding
def test_prepare_multi_checks_arguments_before_the_c_call():
    """A plan-less format and a bad mode are SpmvError(OTHER_ERROR) raised in
    Python; the transposed calls answer the same way."""
    bare = sa.DeviceMatrix("csr16", 4, 6, 4, "cpu", plan=None)
    with pytest.raises(sa.SpmvError) as e:
        bare.prepare_multi()
    assert e.value.rc == sa.OTHER_ERROR and "no plan" in str(e.value)
    with pytest.raises(sa.SpmvError) as e:
        bare.multi_info
    assert e.value.rc == sa.OTHER_ERROR
    for mode in ("Balanced", "copy", 1, 0, True, ("balanced",)):
        with pytest.raises(sa.SpmvError) as e:
            bare.prepare_multi(mode)
        assert e.value.rc == sa.OTHER_ERROR and "mode" in str(e.value), mode
    with pytest.raises(sa.SpmvError) as e:
        bare.prepare_transpose("copy")
    assert e.value.rc == sa.OTHER_ERROR
    with pytest.raises(sa.SpmvError) as e:
        bare.prepare_transpose("balanced")
    assert e.value.rc == sa.OTHER_ERROR


# -------------------------------------------------------------- sanitizers
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc with libasan")
def test_multi_plan_harness_under_asan_ubsan():
    """spmv_csr_multi_plan compiled with ASan + UBSan into a stand-alone
    program and driven over the fixtures, the hand-made offsets, the long
    rows and the refusals with exactly-sized outputs."""
    subprocess.run(["make", "-C", str(REPO), "build/san/multi_plan_harness"], check=True, capture_output=True)
    fixtures = sorted(str(p) for p in (REPO / "tests" / "golden").glob("*.mtx"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=99", OMP_NUM_THREADS="4")
    r = subprocess.run([str(REPO / "build" / "san" / "multi_plan_harness"), *fixtures], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert f"multi plan harness: {len(fixtures)} files clean" in r.stdout
