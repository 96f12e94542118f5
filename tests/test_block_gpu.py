"""The two block kernels of LOBPCG on the MI355X (csrc/block.hip), at their
own edges.

spmv_gram_multi against spmv_dot_multi with k = 1 per pair, == on the bits: the
row counts are the steps of G(n) = min(ceil(n / 512), 1024) (a single
workgroup, the second step of a thread's loop, the cap), the data is spread
over 2^+-30 (tests/exact.py's generator) so that another summation order
changes bits.  spmv_block_combine_multi against the host statement
(spmv_cpu_block_combine_multi), == on the bits, at the row counts where its own
grid and unroll constants change; they are restated below and held against the
source by test_constants_match_the_source.

One flat buffer of random doubles lives on the device for the whole module.
Every operand is a window (first element, leading dimension) into it: both
kernels only read their operands, which may overlap, so the same data serves
every width, leading dimension and alignment.
"""
from __future__ import annotations

import re

import numpy as np
import pytest

import spmv_amd as sa
from conftest import PKG
from exact import wide_range

pytestmark = pytest.mark.gpu

GUARD = -7.25e300
# csrc/vec_multi.h, csrc/block.hip
K_BLOCK = 256
DOT_MULTI_BLOCKS = 1024
GRAM_TILE = 4
GRAM_MAX = 24
COMBINE_MAX = 8
COMBINE_ROWS = 2
COMBINE_GRID_CAP = 4096

GRAM_NS = (0, 1, 255, 256, 257, 511, 512, 513, 1025, 524288, 524289, 524801)
GRAM_WIDTHS = ((1, 1), (3, 5), (8, 8), (7, 8), (9, 2), (24, 24))
# one workgroup / two; a thread's unrolled step (rows i and i + stride) and its
# tail; the grid cap: one more row than 4096 workgroups cover in one step
COMBINE_CAP_ROWS = COMBINE_GRID_CAP * K_BLOCK * COMBINE_ROWS
COMBINE_NS = (0, 1, 255, 256, 257, 511, 512, 513, 1024, 1025)
COMBINE_BIG_NS = (COMBINE_CAP_ROWS, COMBINE_CAP_ROWS + 1, COMBINE_CAP_ROWS + K_BLOCK + 1)
COMBINE_WIDTHS = ((1,), (3,), (8,), (1, 3), (8, 8), (3, 8, 1), (8, 8, 8))
COMBINE_KC = (1, 5, 8)
FLAT = max((max(GRAM_NS) + 1) * (GRAM_MAX + 4), (max(COMBINE_BIG_NS) + 1) * 6) + 64


def test_constants_match_the_source():
    vec = (PKG / "csrc" / "vec_multi.h").read_text()
    blk = (PKG / "csrc" / "block.hip").read_text()
    common = (PKG / "csrc" / "common.h").read_text()

    def const(text, name):
        return int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))

    assert const(common, "kBlock") == K_BLOCK
    assert const(vec, "kDotMultiBlocks") == DOT_MULTI_BLOCKS
    assert const(blk, "kGramTile") == GRAM_TILE and const(blk, "kGramMax") == GRAM_MAX
    assert const(blk, "kCombineMax") == COMBINE_MAX and const(blk, "kCombineRows") == COMBINE_ROWS
    assert const(blk, "kCombineGridCap") == COMBINE_GRID_CAP
    assert "const int64_t per = (int64_t)kBlock * 2;" in vec  # G(n): 512 rows per workgroup
    assert "const int64_t per = (int64_t)kBlock * kCombineRows;" in blk


@pytest.fixture(scope="module")
def flat():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    host = wide_range(np.random.default_rng(2024), FLAT)
    host[host == 0.0] = 0.5
    t = torch.from_numpy(host).to(dev)
    host.setflags(write=False)
    assert t.data_ptr() % 16 == 0
    return torch, dev, host, t


def _stream(torch, dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _guarded(torch, dev, count):
    """count doubles of NaN between two GUARD pairs -> (tensor, pointer of the first)."""
    t = torch.full((count + 4,), float("nan"), dtype=torch.float64, device=dev)
    t[:2] = GUARD
    t[-2:] = GUARD
    return t, t.data_ptr() + 16


def _live(t):
    h = t.cpu().numpy()
    assert (h[:2] == GUARD).all() and (h[-2:] == GUARD).all(), "a guard was overwritten"
    return h[2:-2].copy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _odd(w):
    return w + 1 if w % 2 == 0 else w + 2


def _even(w):
    return w + 2 + w % 2


# ------------------------------------------------------------------- the Gram
def _gram(flat, n, ka, offa, lda, kb, offb, ldb):
    """spmv_gram_multi on two windows of the flat buffer, with guards behind
    out and a workspace of exactly spmv_gram_multi_ws_bytes (guards behind it
    too) -> (ka, kb) host."""
    torch, dev, _, t = flat
    lib = sa.hip_lib()
    assert offa + max(n - 1, 0) * lda + ka <= FLAT and offb + max(n - 1, 0) * ldb + kb <= FLAT
    nbytes = lib.spmv_gram_multi_ws_bytes(n, ka, kb)
    g = min(max((n + 2 * K_BLOCK - 1) // (2 * K_BLOCK), 1), DOT_MULTI_BLOCKS)
    assert nbytes == g * ka * kb * 8
    ws, ws_ptr = _guarded(torch, dev, nbytes // 8)
    out, out_ptr = _guarded(torch, dev, ka * kb)
    rc = lib.spmv_gram_multi(n, ka, t.data_ptr() + 8 * offa, lda, kb, t.data_ptr() + 8 * offb, ldb, out_ptr, ws_ptr,
                             nbytes, 0, _stream(torch, dev))
    assert rc == 0, lib.spmv_last_error().decode()
    _live(ws)
    return _live(out).reshape(ka, kb)


_dot_cache = {}


def _dots(flat, n, ka, offa, lda, kb, offb, ldb):
    """The reference: spmv_dot_multi with k = 1 per pair (memoised per pair of
    columns within one n: many layouts name the same two columns)."""
    torch, dev, _, t = flat
    lib = sa.hip_lib()
    ws = torch.empty(lib.spmv_dot_multi_ws_bytes(n, 1), dtype=torch.uint8, device=dev)
    todo = [(a, b) for a in range(ka) for b in range(kb) if (n, offa + a, lda, offb + b, ldb) not in _dot_cache]
    if todo:
        out = torch.full((len(todo),), float("nan"), dtype=torch.float64, device=dev)
        for i, (a, b) in enumerate(todo):
            rc = lib.spmv_dot_multi(n, 1, t.data_ptr() + 8 * (offa + a), lda, t.data_ptr() + 8 * (offb + b), ldb,
                                    out.data_ptr() + 8 * i, sa._ptr(ws), ws.numel(), 0, _stream(torch, dev))
            assert rc == 0, lib.spmv_last_error().decode()
        for (a, b), v in zip(todo, out.cpu().numpy()):
            _dot_cache[(n, offa + a, lda, offb + b, ldb)] = v
    return np.array([[_dot_cache[(n, offa + a, lda, offb + b, ldb)] for b in range(kb)] for a in range(ka)])


@pytest.mark.parametrize("n", GRAM_NS)
def test_gram_has_the_bits_of_dot_multi(flat, n):
    _dot_cache.clear()
    for ka, kb in GRAM_WIDTHS:
        w = max(ka, kb)
        layouts = {
            # ld = the width; B one element off a 16-byte address
            "tight": (0, ka, 1 + ka, kb),
            # odd leading dimensions: the 8-byte path
            "odd": (0, _odd(ka), 3, _odd(kb)),
            # even and wider, both first elements on 16-byte addresses: the vector path
            "even": (0, _even(ka), 2 * _even(w), _even(kb)),
            # overlapping column slices of ONE tensor (ld even, B one column to the right)
            "overlap": (4, _even(w + 1), 5, _even(w + 1)),
        }
        for name, (offa, lda, offb, ldb) in layouts.items():
            got = _gram(flat, n, ka, offa, lda, kb, offb, ldb)
            want = _dots(flat, n, ka, offa, lda, kb, offb, ldb)
            assert same_bits(got, want), (n, ka, kb, name, np.argwhere(got != want)[:5].tolist())
            if n == 0:
                assert same_bits(got, np.zeros((ka, kb)))
        # A is B: the same bits as the pairs, and a symmetric matrix
        if ka == kb:
            for ld, off in ((ka, 0), (_odd(ka), 1), (_even(ka), 2)):
                got = _gram(flat, n, ka, off, ld, ka, off, ld)
                assert same_bits(got, _dots(flat, n, ka, off, ld, ka, off, ld)), (n, ka, ld)
                assert same_bits(got, got.T), (n, ka, ld)
    _dot_cache.clear()


def test_gram_against_longdouble(flat):
    """The values themselves, not only their agreement with spmv_dot_multi:
    (n + 2) 2^-53 sum |a b| against np.longdouble (tests/exact.py's bound)."""
    _, _, host, _ = flat
    n, ka, kb, lda, ldb, offb = 1025, 7, 8, 9, 10, 20
    got = _gram(flat, n, ka, 0, lda, kb, offb, ldb)
    A = np.lib.stride_tricks.as_strided(host, (n, ka), (8 * lda, 8)).astype(np.longdouble)
    B = np.lib.stride_tricks.as_strided(host[offb:], (n, kb), (8 * ldb, 8)).astype(np.longdouble)
    err = np.abs(got.astype(np.longdouble) - A.T @ B).astype(np.float64)
    assert (err <= (n + 2) * 2.0 ** -53 * (np.abs(A).T @ np.abs(B)).astype(np.float64)).all()


def test_gram_refusals(flat):
    torch, dev, _, t = flat
    lib = sa.hip_lib()
    n, ka, kb = 300, 3, 5
    nbytes = lib.spmv_gram_multi_ws_bytes(n, ka, kb)
    ws, ws_ptr = _guarded(torch, dev, nbytes // 8)
    out, out_ptr = _guarded(torch, dev, ka * kb)
    p = t.data_ptr()
    st = _stream(torch, dev)

    def call(n=n, ka=ka, A=p, lda=ka, kb=kb, B=p + 8, ldb=kb, out=out_ptr, ws=ws_ptr, ws_bytes=nbytes):
        return lib.spmv_gram_multi(n, ka, A, lda, kb, B, ldb, out, ws, ws_bytes, 0, st)

    for kw in (dict(n=-1), dict(ka=0), dict(kb=0), dict(ka=25, lda=25), dict(kb=25, ldb=25), dict(lda=2), dict(ldb=4),
               dict(A=None), dict(B=None), dict(out=None)):
        assert call(**kw) == sa.OTHER_ERROR, kw
        assert "spmv_gram_multi: bad arguments" in lib.spmv_last_error().decode(), kw
    for kw in (dict(ws=None), dict(ws_bytes=nbytes - 1), dict(ws_bytes=0)):
        assert call(**kw) == sa.OTHER_ERROR, kw
        assert "spmv_gram_multi: workspace too small" in lib.spmv_last_error().decode(), kw
    torch.cuda.synchronize()
    assert np.isnan(_live(out)).all() and np.isnan(_live(ws)).all()  # nothing was written
    assert call() == 0
    assert call(n=0, A=None, B=None) == 0  # n == 0 reads no block and writes zeros
    assert same_bits(_live(out), np.zeros(ka * kb))


# ---------------------------------------------------------------- the combine
class YBuffer:
    """(n + 2) rows of ldy doubles behind `off` elements, GUARD at both ends,
    random elsewhere: the device tensor and its host image."""

    def __init__(self, torch, dev, n, kc, ldy, off, seed):
        self.n, self.kc, self.ldy, self.off = n, kc, ldy, off
        self.host = np.random.default_rng(seed).uniform(-1.0, 1.0, off + (n + 2) * ldy + 2)
        self.host[:off] = GUARD
        self.host[-2:] = GUARD
        self.t = torch.from_numpy(self.host).to(dev)
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + 8 * off

    def rows(self, h):
        return np.lib.stride_tricks.as_strided(h[self.off:], (self.n, self.kc), (8 * self.ldy, 8))


def _combine_case(flat, n, widths, kc, layout, seed, C=None):
    """One launch against the host statement: every element of Y's buffer,
    live or not, must have the host's bits."""
    torch, dev, host, t = flat
    lib = sa.hip_lib()
    if layout == "odd":  # odd leading dimensions, first elements on 8-byte addresses
        lds = [_odd(w) for w in widths]
        offs = [1 + 2 * q for q in range(len(widths))]
        ldy, offy = _odd(kc), 1
    elif layout == "even":  # even ones on 16-byte addresses: the pair loads and stores
        lds = [_even(w) for w in widths]
        offs = [2 * q * 10 for q in range(len(widths))]
        ldy, offy = _even(kc), 0
    else:  # the widths themselves
        lds = list(widths)
        offs = [q * 7 for q in range(len(widths))]
        ldy, offy = kc, 0
    for w, ld, off in zip(widths, lds, offs):
        assert off + max(n - 1, 0) * ld + w <= FLAT
    rng = np.random.default_rng(seed)
    if C is None:
        C = wide_range(rng, (sum(widths), kc))
    y = YBuffer(torch, dev, n, kc, ldy, offy, seed + 1)
    args = []
    for q in range(3):
        args += [widths[q], t.data_ptr() + 8 * offs[q], lds[q]] if q < len(widths) else [0, None, 0]
    rc = lib.spmv_block_combine_multi(n, kc, sa._ptr(C), *args, y.ptr, ldy, 0, _stream(torch, dev))
    assert rc == 0, lib.spmv_last_error().decode()
    want = y.host.copy()
    blocks = [np.lib.stride_tricks.as_strided(host[off:], (n, w), (8 * ld, 8)) for w, ld, off in zip(widths, lds, offs)]
    sa.cpu_block_combine_multi(n, C, blocks, y.rows(want))
    got = y.t.cpu().numpy()
    assert same_bits(got, want), (n, widths, kc, layout, np.argwhere(got != want)[:5].tolist())


@pytest.mark.parametrize("n", COMBINE_NS)
def test_combine_has_the_bits_of_the_host_statement(flat, n):
    seed = 100 * n
    for widths in COMBINE_WIDTHS:
        for kc in COMBINE_KC:
            for layout in ("tight", "odd", "even"):
                seed += 1
                _combine_case(flat, n, widths, kc, layout, seed)


@pytest.mark.parametrize("n", COMBINE_BIG_NS)
def test_combine_past_the_grid_cap(flat, n):
    """More rows than 4096 workgroups cover in one unrolled step: the second
    trip of a thread's loop and its tail (narrow blocks keep it quick)."""
    _combine_case(flat, n, (1,), 1, "tight", 7)
    _combine_case(flat, n, (1, 2), 2, "even", 8)
    _combine_case(flat, n, (3,), 1, "odd", 9)


def test_combine_special_values(flat):
    """+-0.0, Inf and NaN in an operand reach exactly the elements the host
    statement says (a zero in C does not skip a term)."""
    import torch

    _, dev, _, _ = flat
    lib = sa.hip_lib()
    n, widths, kc = 300, (3, 2), 4
    rng = np.random.default_rng(11)
    blocks = [rng.uniform(-1.0, 1.0, (n, w)) for w in widths]
    blocks[0][5, 1] = np.inf
    blocks[0][6, 0] = -np.inf
    blocks[1][7, 1] = np.nan
    blocks[0][8] = -0.0
    blocks[1][8] = -0.0
    blocks[1][299, 0] = np.inf
    C = rng.uniform(-1.0, 1.0, (5, kc))
    C[1, 2] = 0.0  # Inf * 0 = NaN in column 2 of row 5
    C[:, 3] = 0.0
    C[0, 0] = -0.0
    want = np.full((n, kc), GUARD)
    sa.cpu_block_combine_multi(n, C, blocks, want)
    assert np.isnan(want[5, 2]) and np.isnan(want[7]).all() and np.isfinite(want[9]).all()
    assert same_bits(want[8], np.zeros(kc))  # a chain from +0.0 over signed zeros stays +0.0
    dv = [torch.from_numpy(b).to(dev) for b in blocks]
    Y = torch.full((n, kc), GUARD, dtype=torch.float64, device=dev)
    rc = lib.spmv_block_combine_multi(n, kc, sa._ptr(C), 3, dv[0].data_ptr(), 3, 2, dv[1].data_ptr(), 2, 0, None, 0,
                                      Y.data_ptr(), kc, 0, _stream(torch, dev))
    assert rc == 0, lib.spmv_last_error().decode()
    got = Y.cpu().numpy()
    # a NaN where and only where the host statement has one (which NaN an
    # invalid operation returns is the processor's choice); every other
    # element, signed zeros and infinities included, bit for bit
    nan = np.isnan(want)
    assert nan.sum() >= 9 and np.array_equal(np.isnan(got), nan)
    assert same_bits(np.where(nan, 0.0, got), np.where(nan, 0.0, want))
    assert np.isinf(want).any()


def test_combine_refusals(flat):
    torch, dev, _, t = flat
    lib = sa.hip_lib()
    n, kc = 300, 2
    C = np.ones((6, kc))
    y = YBuffer(torch, dev, n, kc, kc, 0, 3)
    p = t.data_ptr()
    st = _stream(torch, dev)

    def call(n=n, kc=kc, C=sa._ptr(C), ka0=2, A0=p, ld0=2, ka1=0, A1=None, ld1=0, ka2=0, A2=None, ld2=0, Y=y.ptr,
             ldy=kc):
        return lib.spmv_block_combine_multi(n, kc, C, ka0, A0, ld0, ka1, A1, ld1, ka2, A2, ld2, Y, ldy, 0, st)

    for kw in (dict(n=-1), dict(kc=0), dict(kc=9, ldy=9), dict(C=None), dict(ka0=-1), dict(ka0=9, ld0=9), dict(ka0=0),
               dict(A0=None), dict(ld0=1), dict(ka1=2, A1=None, ld1=2), dict(ka1=2, A1=p, ld1=1),
               dict(ka2=9, A2=p, ld2=9), dict(ka2=-3, A2=p, ld2=9), dict(Y=None), dict(ldy=1)):
        assert call(**kw) == sa.OTHER_ERROR, kw
        assert "spmv_block_combine_multi: bad arguments" in lib.spmv_last_error().decode(), kw
    torch.cuda.synchronize()
    assert same_bits(y.t.cpu().numpy(), y.host)  # nothing was written
    assert call(n=0, A0=None, Y=None) == 0  # n == 0: no block is needed, nothing is touched
    assert call() == 0 and call(ka1=2, A1=p + 8, ld1=3, ka2=2, A2=p, ld2=2) == 0  # operands may overlap
