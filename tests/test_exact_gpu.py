"""Every kernel path against an order-independent reference (tests/exact.py):
bit-exact on integer data, within the fp64 forward-error bound on real data
with a wide dynamic range.

The 1e-6 parity rule of the other GPU tests cannot see a value that passed
through fp32 or a dropped entry that is small against its row, and the
bitwise tests compare kernels that share their staging code.  Here every
y must EQUAL an int64 reference on integerize()'d data (any summation order
is exact there), and meet (n_i + 2) 2^-53 sum|a_ij x_j| on real data.

Every output buffer starts as NaN.  A format that refuses a matrix (ELL
padding, CSR16 escapes, SELL16 windows, a single-pass COO that does not fit)
is skipped only where to_device raises SpmvError; every parameter set must
run on at least one matrix.  The integer / real copies of a matrix and their
references are computed once and shared.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import exact
import spmv_amd as sa
import test_spmm_gpu
import test_transpose_gpu
from conftest import GOLDEN, golden_cases
from test_gpu_parity import ARM_PARAMS, ARM_ROW_LENGTHS, FMT_PARAMS

pytestmark = pytest.mark.gpu

CASES = [c["name"] for c in golden_cases()]
ARMS = [f"arm{n}" for n in ARM_ROW_LENGTHS]
SMALL = CASES + ARMS
KEYS = SMALL + list(exact.GENERATED)
SENTINEL = 12345.0


def _ids(params):
    return [f"{f}-{'-'.join(f'{k}{v}' for k, v in kw.items()) or 'default'}" for f, kw in params]


def _unique(params):
    out = []
    for p in params:
        if p not in out:
            out.append(p)
    return out


SMALL_PARAMS = _unique(FMT_PARAMS + ARM_PARAMS)

# The union of the option lists of test_gpu_parity's test_rmat_skewed,
# test_ragged_long_rows, test_csr_tiled_edge_tiles and
# test_coo_cmrs_hot_bit_identical (hot in {0, 1, 4096} and COO's reference
# table of 2), then bigplan off, the COO / HYB carry pass, the extra formats.
_HOT = [("coo", {}), ("cmrs", {"cmrs_variant": 1}), ("cmrs", {"cmrs_variant": 1, "h": 32}), ("sell", {"xwin": False}),
        ("sell", {"sigma": 1 << 24, "ki": 2, "xwin": False}), ("sell", {"split": 0, "xwin": False}), ("hyb", {}),
        ("hyb", {"ki": 1})]
GEN_PARAMS = _unique([
    ("coo", {}), ("csr", {}), ("csr", {"variant": 2}), ("csr", {"variant": 4}), ("csr", {"variant": 1}), ("sell", {}),
    ("cmrs", {}), ("hyb", {}), ("sell", {"split": 0}), ("sell", {"split": 256, "ki": 2}),
    ("sell", {"split": 64, "ki": 1, "xwin": False}), ("sell", {"sigma": 65536, "ki": 2}),
    ("csr", {"variant": 4, "hot": 4096}), ("csr", {"variant": 4, "hot": 0}), ("cmrs", {"cmrs_variant": 0}),
    ("cmrs", {"cmrs_variant": 1, "h": 1}), ("cmrs", {"cmrs_variant": 1, "h": 64}),
    ("cmrs", {"h": 8}), ("cmrs", {"h": 32}), ("csr", {"lanes": 64}), ("csr", {"lanes": 2, "variant": 2}),
    ("csr", {"lanes": 2, "variant": 1}),
] + [(f, {**kw, "hot": H}) for f, kw in _HOT for H in (1, 4096, 0)] + [
    ("coo", {"hot": 2}), ("csr", {"variant": 4, "hot": 1}),
    ("csr", {"variant": 4, "hot": 0, "bigplan": False}), ("csr", {"variant": 4, "hot": 4096, "bigplan": False}),
    ("coo", {"coo_tail": False}), ("coo", {"coo_tail": True}), ("coo", {"xwin": True}),
    ("hyb", {"coo_tail": False, "hyb_k": 2}), ("hyb", {"hyb_k": 52}), ("cmrs", {"h": 8, "xwin": False}),
    ("csr", {"variant": 3}), ("csr", {"xwin": True}), ("ell", {}), ("ell", {"ki": 1, "xwin": True}),
    ("csr16", {}), ("csr16", {"csr16_max_escape": None}), ("sell16", {}), ("sell16", {"ki": 1}),
    ("csrf32", {}), ("csrf32", {"lanes": 2}), ("csrf32", {"hot": 4096}), ("csrf32", {"variant": 4, "hot": 0}),
    ("csrg", {}), ("csrg", {"groups": 1}), ("csrg", {"groups": 5}), ("csrg", {"groups": 32}),
])

_ran = {}    # (fmt, repr(kw)) -> matrices the forward checks ran on
_worst = {}  # format -> largest error / bound seen


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    yield torch, torch.device("cuda:0")
    if _worst:  # the measured figures (pytest -s)
        print("\nlargest |y - ref| / bound per format: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(_worst.items())))


def matrix(key):
    if key in exact.GENERATED:
        return exact.generated(key)
    if key in ARMS:
        i = ARMS.index(key)
        return sa.gen_random(300, 300, ARM_ROW_LENGTHS[i], ARM_ROW_LENGTHS[i], 11 + i)
    return sa.read_mtx(GOLDEN / f"{key}.mtx")


@functools.lru_cache(maxsize=None)
def integer_case(key, k=1):
    return exact.integerize(matrix(key), seed=KEYS.index(key) + 1000 * k, k=k)


@functools.lru_cache(maxsize=None)
def real_case(key, f32=False):
    """(matrix, x, xt, (ref, bound), (ref_t, bound_t)); f32: the matrix csrf32 stores."""
    if f32:
        mr, x, xt, _, _ = real_case(key)
        mr = exact.rounded_f32(mr)
    else:
        mr, x, xt = exact.realize(matrix(key), seed=500 + KEYS.index(key))
    fwd = (exact.exact_reference(mr, x), exact.fp64_bound(mr, x))
    tr = None if f32 else (exact.exact_reference(mr, xt, transpose=True), exact.fp64_bound(mr, xt, transpose=True))
    return mr, x, xt, fwd, tr


def to_dev(torch, dev, a):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # a copy: the shared inputs stay read-only


def build(dev, m, fmt, kw, small):
    kw = dict(kw)
    if fmt == "ell" and small:
        kw.setdefault("ell_max_padding", None)  # tiny fixtures pad to 64 rows
    return sa.to_device(m, fmt, dev, **kw)


def run(torch, dev, dm, m, x):
    y = torch.full((max(m.n_rows, 1),), float("nan"), dtype=torch.float64, device=dev)
    dm.run(to_dev(torch, dev, x), y)
    torch.cuda.synchronize()
    return y.cpu().numpy()[: m.n_rows]


def note(fmt, worst):
    _worst[fmt] = max(_worst.get(fmt, 0.0), worst)


def forward_checks(torch, dev, key, fmt, kw):
    """Exact and bounded forward runs of one parameter set on one matrix;
    False where to_device refuses the matrix."""
    small = key in SMALL
    e = integer_case(key)
    what = f"{fmt} {kw} on {key}"
    try:
        dm = build(dev, e.m, fmt, kw, small)
    except sa.SpmvError:
        return False
    exact.assert_exact(run(torch, dev, dm, e.m, e.x), e.ref, what)
    del dm
    mr, x, _, (ref, bound), _ = real_case(key, f32=(fmt == "csrf32"))  # csrf32: its contract is the rounded values
    dm = build(dev, mr, fmt, kw, small)  # the same structure: accepted like the integer copy
    note(fmt, exact.assert_fp64(run(torch, dev, dm, mr, x), mr, x, ref=ref, bound=bound, what=what))
    _ran.setdefault((fmt, repr(kw)), []).append(key)
    return True


# ----------------------------------------------------------- 1. forward
@pytest.mark.parametrize("fmt,kw", SMALL_PARAMS, ids=_ids(SMALL_PARAMS))
def test_forward_small(torch_dev, fmt, kw):
    """Every parameter set of the parity tests on every golden fixture and on
    the four launch-rule matrices (300 x 300, rows of 4 / 20 / 64 / 128)."""
    torch, dev = torch_dev
    ran = [key for key in SMALL if forward_checks(torch, dev, key, fmt, kw)]
    assert set(ARMS) <= set(ran) and len(ran) >= len(SMALL) // 2, ran


@pytest.mark.parametrize("fmt,kw", GEN_PARAMS, ids=_ids(GEN_PARAMS))
@pytest.mark.parametrize("key", exact.GENERATED)
def test_forward_generated(torch_dev, key, fmt, kw):
    torch, dev = torch_dev
    forward_checks(torch, dev, key, fmt, kw)


def test_every_parameter_set_ran_on_a_generated_matrix(torch_dev):
    """Refusals are legitimate per matrix, never per format: every parameter
    set, hence every format of ALL_FORMATS, passed the forward checks on at
    least one generated matrix (run alone, this test runs them itself)."""
    torch, dev = torch_dev
    for fmt, kw in GEN_PARAMS:
        done = [k for k in _ran.get((fmt, repr(kw)), []) if k in exact.GENERATED]
        if not done:
            done = [k for k in ("cantlike", "rmat") if forward_checks(torch, dev, k, fmt, kw)]
        assert done, f"{fmt} {kw} ran on no generated matrix"
    assert {f for f, _ in GEN_PARAMS} == set(sa.ALL_FORMATS)


# ------------------------------------------------------ 2. multi-vector
MULTI_KS = (1, 3, 8, 9)
MULTI_IDS = _ids(test_spmm_gpu.FMT_PARAMS)


def run_multi(torch, dev, dm, m, X, k, layout):
    """One run_multi of the first k columns of X; "offset" starts X and Y one
    element into their buffers (8-byte aligned only)."""
    nc, nr = max(m.n_cols, 1), max(m.n_rows, 1)
    Xk = to_dev(torch, dev, X[:, :k])
    if layout == "offset":
        Xbuf = torch.full((nc * k + 1,), float("nan"), dtype=torch.float64, device=dev)
        Xv = Xbuf[1:].view(nc, k)
        Xv.copy_(Xk)
        Ybuf = torch.full((nr * k + 2,), SENTINEL, dtype=torch.float64, device=dev)
        Yv = Ybuf[1:1 + nr * k].view(nr, k)
        assert Xv.data_ptr() % 16 == 8 and Yv.data_ptr() % 16 == 8
    else:
        Xv = Xk
        Ybuf = torch.full((nr * k,), SENTINEL, dtype=torch.float64, device=dev)
        Yv = Ybuf.view(nr, k)
    Yv.fill_(float("nan"))
    dm.run_multi(Xv, Yv)
    torch.cuda.synchronize()
    if layout == "offset":
        flanks = Ybuf.cpu().numpy()[[0, -1]]
        assert np.array_equal(flanks.view(np.int64), np.full(2, SENTINEL).view(np.int64)), "Y's flanks written"
    return Yv.cpu().numpy()[: m.n_rows]


@pytest.mark.parametrize("fmt,kw", test_spmm_gpu.FMT_PARAMS, ids=MULTI_IDS)
@pytest.mark.parametrize("key", ["n67", "long_rows", "ragged_shuffled"])
def test_multi_exact_and_bounded(torch_dev, key, fmt, kw):
    """Every column equals the int64 reference for every k and layout (so
    column j's bits cannot depend on k or the layout), and meets the fp64
    bound on real data."""
    torch, dev = torch_dev
    e = integer_case(key, k=max(MULTI_KS))
    dm = build(dev, e.m, fmt, kw, True)
    assert dm.multi_supported
    for k in MULTI_KS:
        for layout in ("plain", "offset"):
            Y = run_multi(torch, dev, dm, e.m, e.x, k, layout)
            exact.assert_exact(Y, e.ref[:, :k], f"{fmt} {kw} on {key} k={k} {layout}")
    mr, x, _, (ref, bound), _ = real_case(key)
    scales = (1.0, -1.0, 2.0, 0.5, -4.0, 8.0, 0.25, -2.0, 16.0)  # exact scalings: the references scale with them
    X = np.stack([s * x for s in scales], axis=1)
    dm = build(dev, mr, fmt, kw, True)
    for k in (3, 9):
        Y = run_multi(torch, dev, dm, mr, X, k, "offset")
        for j in range(k):
            note(fmt + " (multi)", exact.assert_fp64(Y[:, j], mr, x, ref=scales[j] * ref, bound=abs(scales[j]) * bound,
                                                   what=f"{fmt} {kw} on {key} k={k} column {j}"))


@pytest.mark.parametrize("fmt,kw", [("csr", {}), ("csr", {"variant": 3}), ("csr", {"variant": 4, "hot": 4096}),
                                    ("sell", {}), ("ell", {})],
                         ids=["csr-default", "csr-variant3", "csr-variant4-hot4096", "sell", "ell"])
@pytest.mark.parametrize("key", ["rmat", "cantlike"])
def test_multi_generated(torch_dev, key, fmt, kw):
    torch, dev = torch_dev
    e = integer_case(key, k=3)
    try:
        dm = build(dev, e.m, fmt, kw, False)
    except sa.SpmvError:
        assert fmt == "ell" and key == "rmat"  # padding
        return
    for layout in ("plain", "offset"):
        exact.assert_exact(run_multi(torch, dev, dm, e.m, e.x, 3, layout), e.ref, f"{fmt} {kw} on {key} {layout}")
    mr, x, _, (ref, bound), _ = real_case(key)
    dm = build(dev, mr, fmt, kw, False)
    Y = run_multi(torch, dev, dm, mr, np.stack([x, -2.0 * x, 0.5 * x], axis=1), 3, "plain")
    for j, s in enumerate((1.0, -2.0, 0.5)):
        note(fmt + " (multi)", exact.assert_fp64(Y[:, j], mr, x, ref=s * ref, bound=abs(s) * bound,
                                               what=f"{fmt} {kw} on {key} column {j}"))


# -------------------------------------------------------- 3. transposed
TAIL = 3


def run_t(torch, dev, dm, m, xt):
    y = torch.full((m.n_cols + TAIL,), SENTINEL, dtype=torch.float64, device=dev)
    y[: m.n_cols] = float("nan")
    dm.run_t(to_dev(torch, dev, xt), y)
    torch.cuda.synchronize()
    yh = y.cpu().numpy()
    assert np.array_equal(yh[m.n_cols:].view(np.int64), np.full(TAIL, SENTINEL).view(np.int64)), "tail of y written"
    return yh[: m.n_cols]


def transposed_checks(torch, dev, key, kw):
    e = integer_case(key)
    mr, _, xt, _, (ref_t, bound_t) = real_case(key)
    what = f"csr {kw} on {key}"
    dm = sa.to_device(e.m, "csr", dev, **kw)
    dr = sa.to_device(mr, "csr", dev, **kw)
    ys = {}
    for mode in test_transpose_gpu.MODES:
        dm.prepare_transpose(mode)
        ys[mode] = [run_t(torch, dev, dm, e.m, e.xt) for _ in range(2)]
        for y in ys[mode]:
            exact.assert_exact(y, e.ref_t, f"{what} {mode}")
        # integer sums are exact in any order: even the atomics give the same bits on every run
        assert np.array_equal(ys[mode][0].view(np.int64), ys[mode][1].view(np.int64)), f"{what} {mode}: runs differ"
        dr.prepare_transpose(mode)
        note(f"csr (transposed, {mode})", exact.assert_fp64(run_t(torch, dev, dr, mr, xt), mr, xt, transpose=True,
                                                            ref=ref_t, bound=bound_t, what=f"{what} {mode}"))
    assert np.array_equal(ys["scatter"][0].view(np.int64), ys["copy"][0].view(np.int64)), f"{what}: modes differ"


@pytest.mark.parametrize("kw", test_transpose_gpu.CSR_PLANS, ids=test_transpose_gpu.PLAN_IDS)
def test_transposed_fixtures(torch_dev, kw):
    torch, dev = torch_dev
    for key in CASES:
        transposed_checks(torch, dev, key, kw)


@pytest.mark.parametrize("kw", test_transpose_gpu.CSR_PLANS + [{"variant": 4, "hot": 4096}],
                         ids=test_transpose_gpu.PLAN_IDS + ["variant4-hot4096"])
@pytest.mark.parametrize("key", ["cantlike", "rmat", "ragged"])
def test_transposed_generated(torch_dev, key, kw):
    """LDS windows everywhere (cant-like), global atomics for wide row blocks
    (R-MAT, ragged), columns with thousands of entries."""
    torch, dev = torch_dev
    transposed_checks(torch, dev, key, kw)


# -------------------------------------------- 4. forward memory contract
@pytest.mark.parametrize("fmt,kw", FMT_PARAMS, ids=_ids(FMT_PARAMS))
@pytest.mark.parametrize("key", ["n67", "long_rows", "ragged_shuffled", "cantlike"])
def test_forward_memory_contract(torch_dev, key, fmt, kw):
    """spmv_plan_run's contract (include/spmv.h): x and y need 8-byte
    alignment only, nothing outside y[0..n_rows) is written, no value outside
    x[0..n_cols) enters a result.  x and y start one element into larger
    buffers; x's flanks are NaN, y's flanks 12345.0.  Everything stays inside
    the buffers, so an over-read shows as a wrong number."""
    torch, dev = torch_dev
    e = integer_case(key)
    m = e.m
    try:
        dm = build(dev, m, fmt, kw, key != "cantlike")
    except sa.SpmvError:
        assert fmt in ("ell", "csr16", "sell16"), (fmt, key)  # the formats with a documented refusal
        return
    pad = 9
    xbuf = torch.full((1 + m.n_cols + pad,), float("nan"), dtype=torch.float64, device=dev)
    x = xbuf[1:1 + m.n_cols]
    x.copy_(to_dev(torch, dev, e.x))
    ybuf = torch.full((1 + m.n_rows + pad,), SENTINEL, dtype=torch.float64, device=dev)
    y = ybuf[1:1 + m.n_rows]
    y.fill_(float("nan"))
    assert x.is_contiguous() and y.is_contiguous()
    assert x.data_ptr() % 16 == 8 and y.data_ptr() % 16 == 8
    dm.run(x, y)
    torch.cuda.synchronize()
    yh = ybuf.cpu().numpy()
    exact.assert_exact(yh[1:1 + m.n_rows], e.ref, f"{fmt} {kw} on {key}, unaligned")
    flanks = np.concatenate((yh[:1], yh[1 + m.n_rows:]))
    assert np.array_equal(flanks.view(np.int64), np.full(1 + pad, SENTINEL).view(np.int64)), "y's flanks written"
    xh = xbuf.cpu().numpy()
    assert np.isnan(xh[0]) and np.isnan(xh[1 + m.n_cols:]).all() and np.array_equal(xh[1:1 + m.n_cols], e.x)
