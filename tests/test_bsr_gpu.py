"""Block CSR on the GPU (spmv_plan_bsr, spmv_bsr_run; csrc/bsr.hip): parity on
every fixture, the exact-integer and fp64-bound checks of tests/exact.py on
the cant-like matrix, the kernel's own edges (a block row of exactly one LDS
chunk, one block more, several chunks, empty workgroups, hub block rows), the
memory contract of spmv_plan_run with x and y one element into larger
buffers, bit-identical runs under every switch, the refusals and a
block-Jacobi preconditioned CG solve.  Every y starts as NaN."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import exact
import iterate as it
import spmv_amd as sa
from conftest import GOLDEN, golden_cases
from oracle import oracle
from precond_cases import block_congruence, scipy_csr

pytestmark = pytest.mark.gpu

CASES = [c["name"] for c in golden_cases()]
BLOCKS = (2, 3, 4)
SENTINEL = 12345.0
INF = float("inf")

# csrc/bsr.hip's constants, mirrored (as tests/thresholds.py mirrors the others'):
BSR_CHUNK = 256          # kBsrChunk: blocks per LDS chunk
BSR_CHUNK_ALIGN = 32     # kBsrChunkAlign: a workgroup's first chunk starts on a multiple of it
BSR_BLOCKS_PER_LANE = 2  # kBsrBlocksPerLane: the lane rule of spmv_bsr_auto_lanes
BSR_MIN_LANES = 8        # kBsrMinLanes: the rule's floor
WG = 256                 # kBlock: a workgroup owns WG / lanes block rows


def auto_lanes(n_brows, n_blocks):
    """spmv_bsr_auto_lanes, restated."""
    mean = n_blocks / n_brows if n_brows > 0 else 0.0
    L = BSR_MIN_LANES
    while L < 64 and 2 * L * BSR_BLOCKS_PER_LANE <= mean * 1.5:
        L *= 2
    return L


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch, torch.device("cuda:0")


def run(torch, dev, dm, x):
    xd = torch.from_numpy(np.array(x, dtype=np.float64)).to(dev)  # a copy: the shared inputs are read-only
    y = torch.full((max(dm.n_rows, 1),), float("nan"), dtype=torch.float64, device=dev)
    dm.run(xd, y)
    torch.cuda.synchronize()
    return y.cpu().numpy()[: dm.n_rows]


def bsr(dev, m, b, lanes=0):
    return sa.to_device(m, "bsr", dev, block=b, lanes=lanes, bsr_max_fill=INF)


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("lanes", [0, 2, 64], ids=["rule", "lanes2", "lanes64"])
@pytest.mark.parametrize("b", BLOCKS)
@pytest.mark.parametrize("name", CASES)
def test_golden_fixtures(torch_dev, name, b, lanes):
    torch, dev = torch_dev
    m = sa.read_mtx(GOLDEN / f"{name}.mtx")
    dm = bsr(dev, m, b, lanes)
    p = dm.params
    assert p["format"] == 5 and p["kernel"] == "bsr_kernel" and p["owned_bytes"] == 0 and p["b"] == b
    assert p["lanes"] == (lanes or auto_lanes(p["n_brows"], p["n_blocks"]))
    assert p["lanes"] == (lanes or sa.hip_lib().spmv_bsr_auto_lanes(p["n_brows"], p["n_blocks"]))
    assert f"{b}x{b}" in p["plan"] and f"{p['lanes']} lanes" in p["plan"] and f"{p['n_blocks']} blocks" in p["plan"]
    assert dm.nnz == m.nnz and dm.stored_bytes == 8 * p["n_blocks"] * b * b + 4 * p["n_blocks"] + 8 * (p["n_brows"] + 1)
    x = sa.ramp_x(m.n_cols)
    y = run(torch, dev, dm, x)
    for y_ref in (oracle.file_order_spmv(m.n_rows, m.row, m.col, m.val, x), np.load(GOLDEN / f"{name}.y.npy")):
        bad = oracle.parity(y, y_ref, m.row, m.col, m.val, x, m.n_rows, rel=1e-6)
        assert bad.size == 0, f"{bad.size} bad rows, first {bad[:5]}: got {y[bad[:5]]} want {y_ref[bad[:5]]}"


# --------------------------------------------------------------- cant-like
@functools.lru_cache(maxsize=None)
def cant_case(order):
    m = sa.gen_cantlike(order)
    e = exact.integerize(m, seed=40 + order)
    mr, x, _ = exact.realize(m, seed=50 + order)
    return m, e, mr, x, exact.exact_reference(mr, x), exact.fp64_bound(mr, x)


@pytest.mark.parametrize("b", BLOCKS)
@pytest.mark.parametrize("order", [0, 1])
def test_cantlike(torch_dev, order, b):
    """b = 3 under the default fill rule, b = 2 and 4 with the rule off."""
    torch, dev = torch_dev
    m, e, mr, x, ref, bound = cant_case(order)
    kw = {} if b == 3 else {"bsr_max_fill": INF}
    dm = sa.to_device(m, "bsr", dev, block=b, **kw)
    assert dm.params["lanes"] == auto_lanes(dm.params["n_brows"], dm.params["n_blocks"])
    xr = sa.ramp_x(m.n_cols)
    y = run(torch, dev, dm, xr)
    bad = oracle.parity(y, oracle.file_order_spmv(m.n_rows, m.row, m.col, m.val, xr), m.row, m.col, m.val, xr, m.n_rows)
    assert bad.size == 0, (bad.size, bad[:5])
    del dm
    exact.assert_exact(run(torch, dev, sa.to_device(e.m, "bsr", dev, block=b, **kw), e.x), e.ref, f"cant-like b={b}")
    worst = exact.assert_fp64(run(torch, dev, sa.to_device(mr, "bsr", dev, block=b, **kw), x), mr, x, ref=ref,
                              bound=bound, what=f"cant-like b={b}")
    print(f"cant-like order {order} b={b}: largest error / bound {worst:.3f}")


def test_cantlike_b4_is_refused_by_the_rule(torch_dev):
    _, dev = torch_dev
    with pytest.raises(sa.SpmvError, match="not fewer than CSR"):
        sa.to_device(cant_case(0)[0], "bsr", dev, block=4)


# ------------------------------------------- edges by the kernel's constants
@functools.lru_cache(maxsize=None)
def chunk_edge_case(b):
    """Block rows of exactly one chunk, one block more and one fewer, several
    chunks plus a rest, the alignment step and its neighbours, empty ones in
    between, with 1..b*b entries per block; the sizes are no multiples of b
    (a partial last block row and block column, both with entries)."""
    C, A = BSR_CHUNK, BSR_CHUNK_ALIGN
    lens = [5, C, 0, C + 1, 1, C - 1, 3 * C + 17, 0, 0, A - 1, A, A + 1, 2 * C, 7, 0, C, C, 4 * C - 3, 2, C + A, 9]
    n_brows, n_bcols = len(lens), 5 * C
    n_rows, n_cols = n_brows * b - 1, n_bcols * b - 1
    rng = np.random.default_rng(100 + b)
    rows, cols = [], []
    for I, n in enumerate(lens):
        bc = rng.choice(n_bcols, n, replace=False)
        if I == n_brows - 1 and n_bcols - 1 not in bc:
            bc[0] = n_bcols - 1  # the partial last block column in the partial last block row
        for J in bc:
            k = rng.integers(1, b * b + 1)
            slots = rng.choice(b * b, k, replace=False)
            rows.append(I * b + slots // b)
            cols.append(J * b + slots % b)
    r, c = np.concatenate(rows), np.concatenate(cols)
    keep = (r < n_rows) & (c < n_cols)
    r, c = r[keep].astype(np.int32), c[keep].astype(np.int32)
    o = np.lexsort((c, r))
    m = sa.Coo(n_rows, n_cols, r[o], c[o], rng.uniform(-1, 1, r.size), False, f"chunk edges b={b}")
    ptr, col, val = sa.csr_from_coo(m)
    s = sa.bsr_build(n_rows, n_cols, ptr, col, val, b)
    got = np.diff(s["brow_ptr"]).tolist()
    # a block can lose all its entries only where the matrix cuts it
    assert got[:-1] == lens[:-1] and 0 < got[-1] <= lens[-1], (got, lens)
    assert C in got and C + 1 in got and C - 1 in got and max(got) > 3 * C
    return exact.integerize(m, seed=200 + b)


@pytest.mark.parametrize("lanes", [0, 2, 8, 64], ids=["rule", "lanes2", "lanes8", "lanes64"])
@pytest.mark.parametrize("b", BLOCKS)
def test_chunk_edges(torch_dev, b, lanes):
    """lanes 64: 4 block rows per workgroup, so a workgroup's range starts at
    any offset from the alignment step and a long block row carries its
    accumulators over several chunks; lanes 2: all 21 block rows in one
    workgroup, 9 chunks."""
    torch, dev = torch_dev
    e = chunk_edge_case(b)
    exact.assert_exact(run(torch, dev, bsr(dev, e.m, b, lanes), e.x), e.ref, f"chunk edges b={b} lanes={lanes}")


@pytest.mark.parametrize("lanes", [0, 2, 64], ids=["rule", "lanes2", "lanes64"])
def test_one_block_row_over_many_chunks(torch_dev, lanes):
    torch, dev = torch_dev
    e = exact.integerize(exact.generated("one_row"), seed=31)
    dm = bsr(dev, e.m, 3, lanes)
    assert dm.params["n_brows"] == 1 and dm.params["n_blocks"] > 6 * BSR_CHUNK
    exact.assert_exact(run(torch, dev, dm, e.x), e.ref, f"one_row lanes={lanes}")


@pytest.mark.parametrize("key", ["empty_runs", "rmat"])
def test_empty_workgroups_and_hub_block_rows(torch_dev, key):
    """empty_runs: workgroups whose block rows are all empty write zeros;
    rmat at b = 3 (fill about 9): hub block rows of many chunks beside empty
    ones."""
    torch, dev = torch_dev
    e = exact.integerize(exact.generated(key), seed=32)
    dm = bsr(dev, e.m, 3)
    ptr = dm.arrays["brow_ptr"].cpu().numpy()
    per_wg = WG // dm.params["lanes"]
    first = ptr[::per_wg]
    if key == "empty_runs":
        assert (np.diff(first) == 0).any(), "no workgroup with empty block rows only"
    assert (np.diff(ptr) == 0).any() and np.diff(ptr).max() > 2 * BSR_CHUNK
    exact.assert_exact(run(torch, dev, dm, e.x), e.ref, key)


# --------------------------------------------------------- memory contract
@functools.lru_cache(maxsize=None)
def contract_case(key):
    m = {"random301": lambda: sa.gen_random(301, 500, 0, 60), "random503": lambda: sa.gen_random(301, 503, 0, 60, seed=2),
         "cantlike": lambda: exact.generated("cantlike")}[key]()
    return exact.integerize(m, seed=60)


@pytest.mark.parametrize("b", BLOCKS)
@pytest.mark.parametrize("key", ["random301", "random503", "cantlike"])
def test_memory_contract(torch_dev, key, b):
    """The construction of test_forward_memory_contract (tests/test_exact_gpu.py):
    x and y start one element into larger buffers (8-byte alignment only), x's
    flanks are NaN (an x read past n_cols through a partial last block column
    turns a row into NaN: 500 = 2 mod 3, 503 and 62,451 are odd), y's flanks a
    sentinel compared bit for bit."""
    torch, dev = torch_dev
    e = contract_case(key)
    m = e.m
    dm = bsr(dev, m, b)
    pad = 9
    xbuf = torch.full((1 + m.n_cols + pad,), float("nan"), dtype=torch.float64, device=dev)
    x = xbuf[1:1 + m.n_cols]
    x.copy_(torch.from_numpy(e.x.copy()).to(dev))
    ybuf = torch.full((1 + m.n_rows + pad,), SENTINEL, dtype=torch.float64, device=dev)
    y = ybuf[1:1 + m.n_rows]
    y.fill_(float("nan"))
    assert x.is_contiguous() and y.is_contiguous()
    assert x.data_ptr() % 16 == 8 and y.data_ptr() % 16 == 8
    dm.run(x, y)
    torch.cuda.synchronize()
    yh = ybuf.cpu().numpy()
    exact.assert_exact(yh[1:1 + m.n_rows], e.ref, f"bsr b={b} on {key}, unaligned")
    flanks = np.concatenate((yh[:1], yh[1 + m.n_rows:]))
    assert np.array_equal(flanks.view(np.int64), np.full(1 + pad, SENTINEL).view(np.int64)), "y's flanks written"
    xh = xbuf.cpu().numpy()
    assert np.isnan(xh[0]) and np.isnan(xh[1 + m.n_cols:]).all() and np.array_equal(xh[1:1 + m.n_cols], e.x)


# -------------------------------------------------------------------- bits
@pytest.mark.parametrize("b", BLOCKS)
def test_same_bits(torch_dev, b):
    """Two runs of one plan, spmv_bsr_run with the plan's lanes, and every
    spmv_set_option switch at 0 and 1: the same bits."""
    torch, dev = torch_dev
    m = cant_case(0)[2]  # wide-range real values: a changed summation order shows
    x = torch.from_numpy(cant_case(0)[3].copy()).to(dev)
    dm = bsr(dev, m, b)

    def once(fn=None):
        y = torch.full((m.n_rows,), float("nan"), dtype=torch.float64, device=dev)
        (fn or dm.run)(x, y)
        torch.cuda.synchronize()
        return y

    def one_call(xx, yy):
        d = dm.dims()
        d.nnz = dm.params["n_blocks"] * b * b
        a = dm.arrays
        sa._check(sa.hip_lib().spmv_bsr_run(d, b, dm.params["n_brows"], sa._ptr(a["brow_ptr"]), sa._ptr(a["bcol"]),
                                            sa._ptr(a["bval"]), sa._ptr(xx), sa._ptr(yy), dm.params["lanes"]),
                  "spmv_bsr_run")

    y0 = once()
    assert not torch.isnan(y0).any()
    assert torch.equal(y0.view(torch.int64), once().view(torch.int64)), "two runs differ"
    assert torch.equal(y0.view(torch.int64), once(one_call).view(torch.int64)), "spmv_bsr_run differs"
    old = {name: sa.get_option(name) for name in sa.OPTIONS}
    try:
        for name in sa.OPTIONS:
            for v in (0, 1):
                sa.set_option(name, v)
                assert torch.equal(y0.view(torch.int64), once().view(torch.int64)), (name, v)
                assert torch.equal(y0.view(torch.int64), once(one_call).view(torch.int64)), (name, v, "one call")
            sa.set_option(name, None if old[name] < 0 else old[name])
    finally:
        for name, v in old.items():
            sa.set_option(name, None if v < 0 else v)
    # other lanes: another (equally valid) summation order
    other = bsr(dev, m, b, 2 if dm.params["lanes"] != 2 else 4)
    y2 = torch.full((m.n_rows,), float("nan"), dtype=torch.float64, device=dev)
    other.run(x, y2)
    torch.cuda.synchronize()
    exact.assert_fp64(y2.cpu().numpy(), m, cant_case(0)[3], ref=cant_case(0)[4], bound=cant_case(0)[5], what="lanes")


def test_graph_capture(torch_dev):
    """The run allocates and synchronises nothing: it can be captured."""
    torch, dev = torch_dev
    e = chunk_edge_case(3)
    dm = bsr(dev, e.m, 3)
    x = torch.from_numpy(e.x.copy()).to(dev)
    y = torch.full((e.m.n_rows,), float("nan"), dtype=torch.float64, device=dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        dm.run(x, y)  # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    y.fill_(float("nan"))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dm.run(x, y)
    g.replay()
    torch.cuda.synchronize()
    exact.assert_exact(y.cpu().numpy(), e.ref, "captured run")


# --------------------------------------------------------------- refusals
def test_refusals(torch_dev):
    torch, dev = torch_dev
    m = sa.read_mtx(GOLDEN / "n67.mtx")
    dm = bsr(dev, m, 3)
    assert not dm.multi_supported and not dm.transpose_supported and not dm.symmetric_supported
    X = torch.zeros((m.n_cols, 2), dtype=torch.float64, device=dev)
    Y = torch.zeros((m.n_rows, 2), dtype=torch.float64, device=dev)
    with pytest.raises(sa.SpmvError, match="BSR plans have no multi-vector kernel"):
        dm.run_multi(X, Y)
    for prepare in (dm.prepare_transpose, dm.prepare_symmetric, dm.prepare_multi):
        with pytest.raises(sa.SpmvError):
            prepare()
    with pytest.raises(sa.SpmvError, match="block must be 2, 3 or 4"):
        sa.to_device(m, "bsr", dev, block=5, bsr_max_fill=INF)
    with pytest.raises(sa.SpmvError, match="lanes"):
        sa.to_device(m, "bsr", dev, block=3, lanes=3, bsr_max_fill=INF)

    lib, P, a, p = sa.hip_lib(), sa._ptr, dm.arrays, dm.params
    stored = p["n_blocks"] * 9

    def create(b=3, n_brows=p["n_brows"], nnz=stored, arrays=(P(a["brow_ptr"]), P(a["bcol"]), P(a["bval"]))):
        d = dm.dims()
        d.nnz = nnz
        plan = ctypes.c_void_p()
        rc = lib.spmv_plan_bsr(d, b, n_brows, *arrays, ctypes.byref(sa.plan_opts()), ctypes.byref(plan))
        if rc == sa.SUCCESS:
            lib.spmv_plan_destroy(plan)
        else:
            assert not plan.value
        return rc, lib.spmv_last_error().decode()

    assert create()[0] == sa.SUCCESS
    for kw, why in ((dict(n_brows=p["n_brows"] + 1), "n_brows"), (dict(nnz=stored + 1), "multiple of b"),
                    (dict(b=5), "2, 3 or 4"), (dict(b=1), "2, 3 or 4"), (dict(arrays=(None, P(a["bcol"]), P(a["bval"]))), "NULL"),
                    (dict(arrays=(P(a["brow_ptr"]), None, P(a["bval"]))), "NULL"),
                    (dict(arrays=(P(a["brow_ptr"]), P(a["bcol"]), None)), "NULL")):
        rc, msg = create(**kw)
        assert rc == sa.OTHER_ERROR and why in msg, (kw, rc, msg)


# ------------------------------------------------------------------ solver
def test_cg_with_block_jacobi(torch_dev):
    """The same recurrence over the BSR and the CSR operator (only the
    product's summation order differs): the true residual reaches 1e-10 and
    the iteration counts agree within 2.  The recurrence stops at 1e-11, a
    factor 10 below the asserted true residual, for the drift between the
    two; checked every iteration so the counts are not rounded to a step."""
    torch, dev = torch_dev
    m = block_congruence(16, 3)
    A = scipy_csr(m)
    b = np.random.default_rng(9).uniform(-1, 1, m.n_rows)
    bd = torch.from_numpy(b).to(dev)
    its = {}
    for fmt, kw in (("csr", {}), ("bsr", {"block": 3})):
        op = it.build_operator(m, fmt=fmt, device=dev, bjacobi=3, **kw)
        x, n, rel = it.cg(op, bd, tol=1e-11, maxit=2000, check_every=1)
        res = np.linalg.norm(b - A @ x.cpu().numpy()) / np.linalg.norm(b)
        print(f"{fmt}: {n} iterations, recurrence {rel:.3g}, true residual {res:.3g}")
        assert rel <= 1e-11 and res <= 1e-10, (fmt, n, rel, res)
        its[fmt] = n
    assert op.kernels.dm.params["fill"] == 1.0 and op.kernels.dm.kernel == "bsr_kernel"
    assert abs(its["bsr"] - its["csr"]) <= 2, its
    B = torch.from_numpy(np.ones((m.n_rows, 2))).to(dev)
    for solver in (it.cg_multi, it.bicgstab_multi):
        with pytest.raises(sa.SpmvError, match="'bsr' matrix has no multi-vector run"):
            solver(op, B)
    h, x1 = it.power_iteration(op, 3)
    assert np.isfinite(h).all()
    x, n, rel = it.bicgstab(op, bd, tol=1e-10, maxit=2000, check_every=1)
    assert rel <= 1e-10 and np.isfinite(x.cpu().numpy()).all()
