"""iterate.py — iterated SpMV over row shards: power iteration, CG,
multi-right-hand-side CG, BiCGSTAB, restarted GMRES and the LOBPCG eigensolver.

SURVEY.md §8f row 3: "Iterated SpMV (power iteration / CG) reusing the y
all-gather as the next x".  The reference stops after one SpMV (reference
csr.c:198-236: launch, read y back, check), so this module has no reference
counterpart; it is the natural consumer of the row-sharded design of §8e.

Layout.  Rank r owns rows [bounds[r], bounds[r+1]) (spmv_partition_rows,
nnz-balanced).  The vector that multiplies A is kept in the GATHERED layout:
`world` blocks of `pad` entries, block r = rank r's rows followed by zeros.
The shard's column indices are renumbered into that layout once, at build
time, so `all_gather_into_tensor` of each rank's padded block IS the next
x — no reorder pass, and the y all-gather becomes the input
of the next SpMV directly.

Overlap (build_operator(..., overlap=True), world > 1).  The shard is
split by column into a LOCAL part (columns in this rank's own block, which
it already holds) and a REMOTE part (every other column).  One step of
A·x then starts the all-gather of the own block (RCCL runs it on its own
stream), runs the local SpMV on the compute stream while the exchange is in
flight, waits, runs the remote SpMV into a scratch y and adds it
(spmv_axpy_ratio with ratio 1: an exact add).  overlap=False with split=True
runs the same launches with the wait first, so the two produce the same
bits; the split itself regroups each row's sum (local entries, then
remote) and so differs from the unsplit SpMV within the parity rule.

Per iteration everything stays on the device: SpMV (libspmv_hip), the
deterministic dot product, and the vector updates read their scalars
(norms, CG's alpha = rr/pAp and beta = rr'/rr) from device memory; the
scalars are all-reduced in place over RCCL (`torch.distributed`, backend
nccl) and never visit the host except for CG's convergence test every
`check_every` iterations.  With one rank the loop can be captured into a
HIP graph (`graph=True`).

Several right-hand sides (cg_multi): k independent CG recurrences, one per
column of a row-major (rows, k) block, share ONE multi-vector product
(DeviceMatrix.run_multi / run_sym_multi) per iteration and the block vector
kernels of csrc/vec_multi.hip; the k alphas and betas are k-vectors in device
memory.  build_operator(symmetric="fused" | "expand") builds the operator on
the stored half of a symmetric matrix (prepare_symmetric), for cg, cg_multi
and power_iteration alike.

Preconditioning (build_operator(bjacobi=bs), cg / cg_multi(precond=...)): a
block-Jacobi preconditioner (sa.BlockJacobi, csrc/precond.hip) built from the
very shard the operator uploads.  It is fully parallel (no level schedules,
nothing that waits on another workgroup), keeps every scalar in device memory,
and its fused kernel also returns the two dot products a preconditioned
iteration needs, so PCG launches as many kernels per iteration as CG.
build_operator(chebyshev=deg) puts a Chebyshev polynomial of that degree in
M^-1 A over it (Chebyshev): the stronger preconditioner that keeps to the same
rule.  Its coefficients are host floats computed before the solve, so an inner
step is one product and one fused kernel, with no reduction.

Non-symmetric matrices (bicgstab, bicgstab_multi): right-preconditioned
BiCGSTAB on the same layout, products and device-resident scalars, one
recurrence per column, with three fused block kernels of its own
(spmv_dot2_multi, spmv_bicgstab_update_dot_multi, spmv_bicgstab_dir_multi) so
that an iteration is 10 launches; block Jacobi is its preconditioner.
BiCGSTAB can break down and has no restart; gmres is the method that cannot:
right-preconditioned restarted GMRES(m <= 31), one right-hand side, its basis
one row-major block and three kernels of its own (spmv_krylov_project_dot,
spmv_krylov_combine, spmv_krylov_normalize; csrc/krylov.hip).  The Hessenberg
matrix and its Givens rotations live on the host, which reads three small
results once per Arnoldi step.

Eigenpairs (lobpcg): the k <= 8 smallest or largest eigenpairs of a symmetric
operator by LOBPCG in its orthonormal-basis form, on the multi-vector products,
the block-Jacobi apply and two block kernels of its own (spmv_gram_multi,
spmv_block_combine_multi; csrc/block.hip).  Its small Gram matrices visit the
host every iteration (Cholesky, a 3k x 3k eigenproblem); everything of the
matrix's length stays on the device.

The device work goes through a `kernels` object (HipKernels by default).
Tests substitute a numpy double to exercise the multi-rank orchestration on
CPU ranks (gloo); the product path only ever builds HipKernels.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass

import numpy as np

import spmv_amd as sa


# ------------------------------------------------------------------ layout
@dataclass
class ShardLayout:
    """Row ownership and the gathered vector layout for `world` ranks."""

    bounds: np.ndarray  # int64[world + 1]
    pad: int  # entries per rank in the gathered vector

    @property
    def world(self) -> int:
        return len(self.bounds) - 1

    def positions(self, idx: np.ndarray) -> np.ndarray:
        """Gathered-layout position of global row/column indices."""
        idx = np.asarray(idx, np.int64)
        owner = np.searchsorted(self.bounds, idx, side="right") - 1
        return (owner * self.pad + (idx - self.bounds[owner])).astype(np.int64)

    def to_gathered(self, v: np.ndarray) -> np.ndarray:
        out = np.zeros(self.world * self.pad, dtype=v.dtype)
        out[self.positions(np.arange(len(v)))] = v
        return out

    def from_gathered(self, g: np.ndarray, n: int) -> np.ndarray:
        return np.asarray(g)[self.positions(np.arange(n))]


def layout_for(n_rows: int, row_counts: np.ndarray, world: int, align: int = 1024) -> ShardLayout:
    """nnz-balanced row ranges (spmv_partition_rows) and a pad rounded up to
    64 entries (one wave of x per block)."""
    ptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(row_counts, out=ptr[1:])
    bounds = sa.partition_rows(n_rows, ptr, world, align)
    pad = int(np.max(np.diff(bounds))) if world > 0 else 0
    pad = max(64, (pad + 63) // 64 * 64)
    return ShardLayout(bounds, pad)


def local_shard(m: sa.Coo, layout: ShardLayout, rank: int) -> sa.Coo:
    """Rank `rank`'s rows with columns renumbered into the gathered layout
    (square matrices: x and y share the row partition)."""
    if m.n_rows != m.n_cols:
        raise sa.SpmvError(sa.OTHER_ERROR, "local_shard", "iterated SpMV needs a square matrix")
    lo, hi = int(layout.bounds[rank]), int(layout.bounds[rank + 1])
    loc = sa.shard(m, lo, hi)
    col = layout.positions(loc.col)
    if col.size and col.max() > np.iinfo(np.int32).max:
        raise sa.SpmvError(sa.OTHER_ERROR, "local_shard", "gathered layout exceeds int32 columns")
    return sa.Coo(hi - lo, layout.world * layout.pad, loc.row, col.astype(np.int32), loc.val, m.symmetric,
                  f"{m.label} rank {rank}/{layout.world}")


def split_local_remote(loc: sa.Coo, layout: ShardLayout, rank: int):
    """(local, remote) parts of a gathered-layout shard: `local` keeps the
    entries whose column lies in this rank's own block, renumbered to
    [0, pad) so it multiplies the rank's send block directly; `remote` keeps
    the rest with gathered-layout columns.  Both keep all the shard's rows
    and their entries in the shard's order."""
    base = rank * layout.pad
    own = (loc.col >= base) & (loc.col < base + layout.pad)
    local = sa.Coo(loc.n_rows, layout.pad, loc.row[own], (loc.col[own] - base).astype(np.int32), loc.val[own],
                   False, f"{loc.label} local")
    remote = sa.Coo(loc.n_rows, loc.n_cols, loc.row[~own], loc.col[~own], loc.val[~own], False,
                    f"{loc.label} remote")
    return local, remote


# ------------------------------------------------------------- collectives
class Comm:
    """In-place collectives over torch.distributed (nccl = RCCL on ROCm);
    with one rank they are no-ops and the gathered vector aliases the local
    block."""

    def __init__(self, dist=None):
        self.dist = dist if dist is not None and dist.is_available() and dist.is_initialized() else None
        self.rank = self.dist.get_rank() if self.dist else 0
        self.world = self.dist.get_world_size() if self.dist else 1

    def allreduce(self, t) -> None:
        if self.dist is not None and self.world > 1:
            self.dist.all_reduce(t)

    def allgather(self, out, inp) -> None:
        if self.dist is not None and self.world > 1:
            self.dist.all_gather_into_tensor(out, inp)
        elif out.data_ptr() != inp.data_ptr():
            out[: inp.numel()].copy_(inp)

    def allgather_start(self, out, inp):
        """Start the all-gather; returns a handle for wait() (None when
        alone: the copy is done at once)."""
        if self.dist is not None and self.world > 1:
            return self.dist.all_gather_into_tensor(out, inp, async_op=True)
        if out.data_ptr() != inp.data_ptr():
            out[: inp.numel()].copy_(inp)
        return None

    @staticmethod
    def wait(work, stream=None) -> None:
        """Make the compute stream wait for a started collective (NCCL: a
        stream dependency, the host does not block).  work.wait() orders
        torch's CURRENT stream only; when the kernels run on another
        `stream`, that stream waits on an event recorded on the current one
        behind the collective."""
        if work is None:
            return
        work.wait()
        if stream is not None:
            torch = sa._torch()
            cur = torch.cuda.current_stream(stream.device)
            if cur.cuda_stream != stream.cuda_stream:
                ev = torch.cuda.Event()
                ev.record(cur)
                stream.wait_event(ev)

    def allgatherv(self, full, bounds) -> str:
        """In-place all-gather of row shards of their REAL sizes: `full`
        holds this rank's rows [bounds[rank], bounds[rank+1]) and receives
        every other rank's, no padding to the largest shard.  Over RCCL one
        torch all_gather of unequal parts (ProcessGroupNCCL issues it as
        grouped broadcasts, one per shard); over gloo one broadcast per
        non-empty shard.  Returns how it was done."""
        if self.dist is None or self.world == 1:
            return "none (one rank)"
        parts = [full[int(bounds[r]):int(bounds[r + 1])] for r in range(self.world)]
        if self.dist.get_backend() == "nccl":
            self.dist.all_gather(parts, parts[self.rank])
            return "rccl all_gather of unequal parts (grouped broadcasts)"
        for r in range(self.world):
            if parts[r].numel():
                self.dist.broadcast(parts[r], src=r)
        return "gloo broadcast per shard"


# ---------------------------------------------------------------- kernels
class HipKernels:
    """The device kernels of one iteration, all on one stream."""

    def __init__(self, dm: sa.DeviceMatrix, stream=None, symmetric: bool = False):
        """symmetric: dm holds the stored half of a symmetric matrix and was
        prepared (prepare_symmetric): spmv is run_sym, spmm run_sym_multi."""
        torch = sa._torch()
        self.dm = dm
        self.symmetric = symmetric
        self.dev = torch.device(dm.device)
        self.lib = sa.hip_lib()
        self.stream = stream

    def _s(self):
        torch = sa._torch()
        st = self.stream if self.stream is not None else torch.cuda.current_stream(self.dev)
        return st.cuda_stream

    def spmv(self, x_full, y) -> None:
        if self.symmetric:
            self.dm.run_sym(x_full, y, self.stream)
        else:
            self.dm.run(x_full, y, self.stream)

    @property
    def multi_supported(self) -> bool:
        """spmm can run this matrix (a CSR, ELL or SELL plan)."""
        return self.dm.multi_supported

    def spmm(self, X_full, Y) -> None:
        """Y = A X_full for row-major (rows, k) blocks."""
        if self.symmetric:
            self.dm.run_sym_multi(X_full, Y, self.stream)
        else:
            self.dm.run_multi(X_full, Y, self.stream)

    def dot(self, n, a, b, out, ws) -> None:
        sa._check(self.lib.spmv_dot(n, sa._ptr(a), sa._ptr(b), sa._ptr(out), sa._ptr(ws), ws.numel(),
                                    self.dev.index or 0, self._s()), "spmv_dot")

    def axpy_ratio(self, n, num, den, sign, x, y) -> None:
        sa._check(self.lib.spmv_axpy_ratio(n, sa._ptr(num), sa._ptr(den), float(sign), sa._ptr(x), sa._ptr(y),
                                           self.dev.index or 0, self._s()), "spmv_axpy_ratio")

    def xpay_ratio(self, n, num, den, x, y) -> None:
        sa._check(self.lib.spmv_xpay_ratio(n, sa._ptr(num), sa._ptr(den), sa._ptr(x), sa._ptr(y),
                                           self.dev.index or 0, self._s()), "spmv_xpay_ratio")

    def scale_rsqrt(self, n, s, x, y) -> None:
        sa._check(self.lib.spmv_scale_rsqrt(n, sa._ptr(s), sa._ptr(x), sa._ptr(y), self.dev.index or 0,
                                            self._s()), "spmv_scale_rsqrt")

    def dot_ws(self, n):
        torch = sa._torch()
        nbytes = self.lib.spmv_dot_ws_bytes(n)
        return torch.empty(nbytes, dtype=torch.uint8, device=self.dev)

    # the block kernels (csrc/vec_multi.hip): A, B, X, Y are row-major
    # (>= n, k) blocks with inner stride 1, out / num / den hold k scalars
    @staticmethod
    def _ld(t) -> int:
        return sa._ld(t, t.shape[1])

    def dot_multi(self, n, A, B, out, ws) -> None:
        sa._check(self.lib.spmv_dot_multi(n, A.shape[1], sa._ptr(A), self._ld(A), sa._ptr(B), self._ld(B),
                                          sa._ptr(out), sa._ptr(ws), ws.numel(), self.dev.index or 0, self._s()),
                  "spmv_dot_multi")

    def axpy_ratio_multi(self, n, num, den, sign, X, Y) -> None:
        sa._check(self.lib.spmv_axpy_ratio_multi(n, X.shape[1], sa._ptr(num), sa._ptr(den), float(sign), sa._ptr(X),
                                                 self._ld(X), sa._ptr(Y), self._ld(Y), self.dev.index or 0,
                                                 self._s()), "spmv_axpy_ratio_multi")

    def xpay_ratio_multi(self, n, num, den, X, Y) -> None:
        sa._check(self.lib.spmv_xpay_ratio_multi(n, X.shape[1], sa._ptr(num), sa._ptr(den), sa._ptr(X), self._ld(X),
                                                 sa._ptr(Y), self._ld(Y), self.dev.index or 0, self._s()),
                  "spmv_xpay_ratio_multi")

    def dot_multi_ws(self, n, k):
        torch = sa._torch()
        nbytes = self.lib.spmv_dot_multi_ws_bytes(n, k)
        return torch.empty(nbytes, dtype=torch.uint8, device=self.dev)

    # the fused block kernels of BiCGSTAB (_bicgstab): out holds 2k scalars,
    # ws dot_multi_ws(n, 2k)
    def dot2_multi(self, n, A, B, C, out, ws) -> None:
        """out[:k] = column sums of A B, out[k:2k] of A C (C may be A)."""
        sa._check(self.lib.spmv_dot2_multi(n, A.shape[1], sa._ptr(A), self._ld(A), sa._ptr(B), self._ld(B),
                                           sa._ptr(C), self._ld(C), sa._ptr(out), sa._ptr(ws), ws.numel(),
                                           self.dev.index or 0, self._s()), "spmv_dot2_multi")

    def bicgstab_update_dot(self, n, a_num, a_den, w_num, w_den, Ph, Sh, T, R0, X, R, out, ws) -> None:
        """X += alpha Ph + omega Sh, R -= omega T (alpha = a_num / a_den,
        omega = w_num / w_den, 0 for a zero denominator; Sh may be R), and
        out[:k] = column sums of R0 R, out[k:2k] of R R over the new R."""
        sa._check(self.lib.spmv_bicgstab_update_dot_multi(
            n, X.shape[1], sa._ptr(a_num), sa._ptr(a_den), sa._ptr(w_num), sa._ptr(w_den), sa._ptr(Ph), self._ld(Ph),
            sa._ptr(Sh), self._ld(Sh), sa._ptr(T), self._ld(T), sa._ptr(R0), self._ld(R0), sa._ptr(X), self._ld(X),
            sa._ptr(R), self._ld(R), sa._ptr(out), sa._ptr(ws), ws.numel(), self.dev.index or 0, self._s()),
            "spmv_bicgstab_update_dot_multi")

    def bicgstab_dir(self, n, rho_new, rv, tt, ts, V, R, P) -> None:
        """P = R + beta (P - omega V), beta = (rho_new / rv) (tt / ts), omega =
        ts / tt (each ratio 0 for a zero denominator)."""
        sa._check(self.lib.spmv_bicgstab_dir_multi(n, P.shape[1], sa._ptr(rho_new), sa._ptr(rv), sa._ptr(tt),
                                                   sa._ptr(ts), sa._ptr(V), self._ld(V), sa._ptr(R), self._ld(R),
                                                   sa._ptr(P), self._ld(P), self.dev.index or 0, self._s()),
                  "spmv_bicgstab_dir_multi")

    # the block kernels of LOBPCG (csrc/block.hip)
    def gram(self, n, A, B, out, ws) -> None:
        """out[a * kb + b] = sum over the first n rows of A[:, a] B[:, b], for
        blocks of ka and kb <= 24 columns (A may be B); ws: gram_ws(n, ka, kb)."""
        sa._check(self.lib.spmv_gram_multi(n, A.shape[1], sa._ptr(A), self._ld(A), B.shape[1], sa._ptr(B),
                                           self._ld(B), sa._ptr(out), sa._ptr(ws), ws.numel(), self.dev.index or 0,
                                           self._s()), "spmv_gram_multi")

    def gram_ws(self, n, ka, kb):
        torch = sa._torch()
        nbytes = self.lib.spmv_gram_multi_ws_bytes(n, ka, kb)
        return torch.empty(nbytes, dtype=torch.uint8, device=self.dev)

    def block_combine(self, n, C, blocks, Y) -> None:
        """Y[:n, :kc] = [blocks[0] blocks[1] blocks[2]] C: 1 to 3 blocks of up to
        8 columns, C a HOST (sum of their widths, kc <= 8) matrix that travels in
        the kernel arguments.  Y must not overlap a block."""
        C, kc = sa.combine_matrix(C, blocks, "block_combine")
        args = []
        for q in range(3):
            t = blocks[q] if q < len(blocks) else None
            args += [0, None, 0] if t is None else [t.shape[1], sa._ptr(t), self._ld(t)]
        ldy = sa._ld(Y, kc)
        sa._check(self.lib.spmv_block_combine_multi(n, kc, sa._ptr(C), *args, sa._ptr(Y), ldy, self.dev.index or 0,
                                                    self._s()), "spmv_block_combine_multi")

    # the basis kernels of GMRES (csrc/krylov.hip): V is the (>= n, c <= 32)
    # view of the basis' first c columns; w, w_out, t, v are (>= n, 1) views,
    # each possibly a column of a block
    def krylov_project_dot(self, n, V, h, w, w_out, out, ws) -> None:
        """w_out = w - V h (h: c device scalars, or None for zeros; w_out may
        then be None, and may be w or another column of V's block otherwise),
        out[:c] = V^T w_out, out[c] = w_out . w_out; ws: krylov_project_ws(n)."""
        sa._check(self.lib.spmv_krylov_project_dot(n, V.shape[1], sa._ptr(V), self._ld(V), sa._ptr(h), sa._ptr(w),
                                                   self._ld(w), sa._ptr(w_out),
                                                   0 if w_out is None else self._ld(w_out), sa._ptr(out),
                                                   sa._ptr(ws), ws.numel(), self.dev.index or 0, self._s()),
                  "spmv_krylov_project_dot")

    def krylov_project_ws(self, n):
        """The workspace of krylov_project_dot for any basis width."""
        torch = sa._torch()
        nbytes = self.lib.spmv_dot_multi_ws_bytes(n, sa.KRYLOV_MAX_COLS + 1)
        return torch.empty(nbytes, dtype=torch.uint8, device=self.dev)

    def krylov_combine(self, n, V, y, t) -> None:
        """t = V y, y a HOST float64 array of c scalars that travels in the
        kernel arguments."""
        y = np.ascontiguousarray(y, np.float64)
        if y.ndim != 1 or y.shape[0] != V.shape[1]:
            raise sa.SpmvError(sa.OTHER_ERROR, "krylov_combine", f"y must hold {V.shape[1]} scalars, not {y.shape}")
        sa._check(self.lib.spmv_krylov_combine(n, V.shape[1], sa._ptr(V), self._ld(V), sa._ptr(y), sa._ptr(t),
                                               self._ld(t), self.dev.index or 0, self._s()), "spmv_krylov_combine")

    def krylov_normalize(self, n, s, w, v, copy=None) -> None:
        """v = w / sqrt(s[0]) (0 for s[0] <= 0; v may be w), and the same values
        into the contiguous vector `copy` when one is given."""
        sa._check(self.lib.spmv_krylov_normalize(n, sa._ptr(s), sa._ptr(w), self._ld(w), sa._ptr(v), self._ld(v),
                                                 sa._ptr(copy), self.dev.index or 0, self._s()),
                  "spmv_krylov_normalize")

    # the preconditioner M (sa.BlockJacobi over this rank's n rows):
    # Z = M^-1 R, out[:k] = column sums of R Z, out[k:2k] of R R
    def precond_apply_dot(self, M, n, R, Z, out, ws) -> None:
        sa._check(self.lib.spmv_bjacobi_apply_dot_multi(M.handle, R.shape[1], sa._ptr(R), self._ld(R), sa._ptr(Z),
                                                        self._ld(Z), sa._ptr(out), sa._ptr(ws), ws.numel(), self._s()),
                  "spmv_bjacobi_apply_dot_multi")

    def precond_apply(self, M, n, R, Z) -> None:
        """Z = M^-1 R alone (BiCGSTAB needs no sums of it)."""
        sa._check(self.lib.spmv_bjacobi_apply_multi(M.handle, R.shape[1], sa._ptr(R), self._ld(R), sa._ptr(Z),
                                                    self._ld(Z), self._s()), "spmv_bjacobi_apply_multi")

    def precond_ws(self, M, n, k):
        return M.ws(n, k)

    # one step of the Chebyshev recurrence over M^-1 (Chebyshev below): AZ =
    # None is step 0, D = Zout = b M^-1 R; otherwise D = a D + b M^-1 (R - AZ),
    # Zout = Zin + D (Zout may be Zin).  a and b are host floats.
    def _cheb_args(self, M, a, b, R, AZ, D, Zin, Zout):
        if AZ is None:
            Zin = None
        ld = [0 if t is None else self._ld(t) for t in (R, AZ, D, Zin, Zout)]
        return (M.handle, R.shape[1], float(a), float(b), sa._ptr(R), ld[0], sa._ptr(AZ), ld[1], sa._ptr(D), ld[2],
                sa._ptr(Zin), ld[3], sa._ptr(Zout), ld[4])

    def cheb_step(self, M, n, a, b, R, AZ, D, Zin, Zout) -> None:
        sa._check(self.lib.spmv_bjacobi_cheb_step_multi(*self._cheb_args(M, a, b, R, AZ, D, Zin, Zout), self._s()),
                  "spmv_bjacobi_cheb_step_multi")

    def cheb_step_dot(self, M, n, a, b, R, AZ, D, Zin, Zout, out, ws) -> None:
        """cheb_step, and out[:k] = column sums of R Zout, out[k:2k] of R R."""
        sa._check(self.lib.spmv_bjacobi_cheb_step_dot_multi(*self._cheb_args(M, a, b, R, AZ, D, Zin, Zout),
                                                            sa._ptr(out), sa._ptr(ws), ws.numel(), self._s()),
                  "spmv_bjacobi_cheb_step_dot_multi")


# --------------------------------------------------------------- operator
@dataclass
class DistOperator:
    """One rank's share of a square matrix in the gathered layout."""

    layout: ShardLayout
    rank: int
    n: int  # global rows
    kernels: object  # HipKernels (or a test double); the LOCAL part when split
    device: object = None
    remote: object = None  # kernels of the remote-column part (split shards only)
    overlap: bool = False  # split shards: run the local part while the all-gather is in flight
    # sa.BlockJacobi over this rank's rows (build_operator(bjacobi=bs)), a Chebyshev over one (chebyshev=deg), or None
    precond: object = None

    @property
    def world(self) -> int:
        return self.layout.world

    @property
    def lo(self) -> int:
        return int(self.layout.bounds[self.rank])

    @property
    def rows(self) -> int:
        return int(self.layout.bounds[self.rank + 1] - self.layout.bounds[self.rank])

    @property
    def pad(self) -> int:
        return self.layout.pad


def build_operator(m: sa.Coo, rank: int = 0, world: int = 1, fmt: str = "csr", device="cuda:0", align: int = 1024,
                   split: bool = False, overlap: bool = False, expand_symmetric: bool = False,
                   symmetric: str | None = None, bjacobi: int | None = None, chebyshev: int | None = None,
                   cheb_ratio: float = 30.0, cheb_boost: float = 1.1, cheb_bounds=None, **fmt_kw) -> DistOperator:
    """Partition, renumber and upload this rank's shard (HIP kernels).
    split (implied by overlap): local / remote column parts
    (split_local_remote), each its own device matrix.
    expand_symmetric: m holds one half of a symmetric matrix (a Matrix Market
    `symmetric` file); sa.expand_symmetric turns it into the matrix it
    describes before sharding, which is what CG needs.  Default: the entries
    as listed.
    symmetric ("fused" or "expand"): m holds one half of a symmetric matrix
    and STAYS that half: the CSR device matrix is built over it and prepared
    with prepare_symmetric(symmetric), so the operator's products are
    run_sym / run_sym_multi ("expand" is bitwise reproducible, "fused" is
    not).  One rank, CSR, unsplit only; anything else is refused before
    anything is uploaded.
    bjacobi (a block size, 1..16): also builds a block-Jacobi preconditioner
    (sa.BlockJacobi) from the very shard that is uploaded, whatever fmt, and
    stores it in the operator's `precond`, which cg and cg_multi then use.
    Its blocks are cut from this rank's rows, so they never span two ranks; a
    split shard builds it from its local part.
    chebyshev (a degree, 1..16): the preconditioner becomes a Chebyshev
    polynomial of that degree in M^-1 A over the block-Jacobi M (Chebyshev;
    bjacobi=None then means bs = 1, point Jacobi): `precond` is the Chebyshev
    object and `precond.M` the sa.BlockJacobi.  Unsplit operators only.
    cheb_bounds=(lmin, lmax), 0 < lmin < lmax, is taken as given.  Otherwise
    lmax = cheb_boost * estimate_lmax(op, M) (10 steps of the power method;
    with world > 1 every rank must be building its operator, since the
    estimate all-reduces over torch.distributed) and lmin = lmax / cheb_ratio.
    10 steps, 1.1 and 30 are the conventions of Ifpack2's and hypre's
    Chebyshev smoothers, not measurements of this project's.  The power method
    approaches the largest eigenvalue from below and AN UNDERESTIMATED lmax
    MAKES THE PRECONDITIONER INDEFINITE (CG may then break down or stall):
    that is what cheb_boost guards against; raise it, or pass cheb_bounds,
    for a matrix on which ten steps are too few.
    fmt="bsr" (block=2, 3 or 4 and the other sa.to_device keywords through
    fmt_kw): block CSR, for power_iteration, cg and bicgstab (no multi-vector
    run: cg_multi and bicgstab_multi refuse).  On more than one rank align must
    be a multiple of the block size."""
    def refuse_cheb(why):
        return sa.SpmvError(sa.OTHER_ERROR, "build_operator", f"chebyshev={chebyshev!r}: {why}")

    if fmt in sa.BLOCK_FORMATS and world > 1:
        # each rank blocks its own shard from its first row: bounds that cut a
        # block row of the whole matrix would break its blocks apart
        block = fmt_kw.get("block", 3)
        if isinstance(block, (int, np.integer)) and not isinstance(block, bool) and block > 0 and align % block:
            raise sa.SpmvError(sa.OTHER_ERROR, "build_operator",
                               f'fmt="{fmt}" with block={block} on {world} ranks: align={align} must be a multiple of '
                               "the block size (a shard bound would cut a block row)")

    if chebyshev is None:
        if cheb_bounds is not None:
            raise sa.SpmvError(sa.OTHER_ERROR, "build_operator", "cheb_bounds without chebyshev=degree")
    else:
        if not isinstance(chebyshev, (int, np.integer)) or isinstance(chebyshev, bool) or not 1 <= chebyshev <= 16:
            raise refuse_cheb("must be a degree in 1..16")
        if split or overlap:
            raise refuse_cheb("no split / overlap operators")
        if cheb_bounds is not None:
            try:
                lmin, lmax = (float(v) for v in cheb_bounds)
            except (TypeError, ValueError):
                raise refuse_cheb(f"cheb_bounds must be (lmin, lmax), not {cheb_bounds!r}") from None
            if not (np.isfinite(lmax) and 0.0 < lmin < lmax):
                raise refuse_cheb(f"cheb_bounds must satisfy 0 < lmin < lmax, not {cheb_bounds!r}")
        elif not (np.isfinite(cheb_ratio) and cheb_ratio > 1.0 and np.isfinite(cheb_boost) and cheb_boost > 0.0):
            raise refuse_cheb("cheb_ratio must be > 1 and cheb_boost > 0")
        if bjacobi is None:
            bjacobi = 1
        op = build_operator(m, rank, world, fmt, device, align, False, False, expand_symmetric, symmetric, bjacobi,
                            **fmt_kw)
        M = op.precond
        if cheb_bounds is None:
            comm = Comm(sa._torch().distributed) if world > 1 else Comm()
            lmax = float(cheb_boost) * estimate_lmax(op, M, comm)
            lmin = lmax / float(cheb_ratio)
        op.precond = Chebyshev(M, int(chebyshev), lmin, lmax)
        return op
    if bjacobi is not None and (not isinstance(bjacobi, (int, np.integer)) or isinstance(bjacobi, bool)
                                or not 1 <= bjacobi <= 16):
        raise sa.SpmvError(sa.OTHER_ERROR, "build_operator", f"bjacobi must be a block size in 1..16, not {bjacobi!r}")

    def precond(shard, col_base=0, half=False):
        return None if bjacobi is None else sa.BlockJacobi.from_coo(shard, int(bjacobi), device, col_base, half)

    if symmetric is not None:
        def refuse(why):
            return sa.SpmvError(sa.OTHER_ERROR, "build_operator", f"symmetric={symmetric!r}: {why}")

        if symmetric not in ("fused", "expand"):
            raise refuse('must be None, "fused" or "expand"')
        if world != 1:
            raise refuse("one rank only (the stored half is not row-sharded)")
        if fmt != "csr":
            raise refuse(f'format "csr" only, not {fmt!r}')
        if split or overlap:
            raise refuse("no split / overlap operators")
        if expand_symmetric:
            raise refuse("expand_symmetric=True expands on the host: choose one of the two")
        if m.n_rows != m.n_cols:
            raise refuse("the matrix is not square")
        counts = np.bincount(m.row, minlength=m.n_rows).astype(np.int64)
        layout = layout_for(m.n_rows, counts, 1, align)  # one block: positions are the identity
        dm = sa.to_device(m, "csr", device, **fmt_kw)  # the half itself, n x n
        dm.prepare_symmetric(symmetric)
        return DistOperator(layout, rank, m.n_rows, HipKernels(dm, symmetric=True), device,
                            precond=precond(m, 0, True))
    if expand_symmetric:
        m = sa.expand_symmetric(m)
    counts = np.bincount(m.row, minlength=m.n_rows).astype(np.int64)
    layout = layout_for(m.n_rows, counts, world, align)
    loc = local_shard(m, layout, rank)
    if not (split or overlap):
        return DistOperator(layout, rank, m.n_rows, HipKernels(sa.to_device(loc, fmt, device, **fmt_kw)), device,
                            precond=precond(loc, rank * layout.pad))
    local, remote = split_local_remote(loc, layout, rank)
    return DistOperator(layout, rank, m.n_rows, HipKernels(sa.to_device(local, fmt, device, **fmt_kw)), device,
                        HipKernels(sa.to_device(remote, fmt, device, **fmt_kw)), overlap, precond(local))


def _fmt_of(kernels) -> str:
    """The format name of an operator's device matrix, for messages."""
    return repr(getattr(getattr(kernels, "dm", None), "fmt", "?"))


def _zeros(op, n):
    torch = sa._torch()
    return torch.zeros(n, dtype=torch.float64, device=op.device)


class _Apply:
    """y = A·x for the vector whose own block is `send` (gathered into
    `full` by this call).  Unsplit: all-gather, then one SpMV on `full`.
    Split: start the all-gather, local SpMV on `send` (before or after the
    wait: overlap), wait, remote SpMV on `full` into a scratch vector, exact
    add."""

    def __init__(self, op, comm, full, send, multi=False):
        """multi: full and send are (.., k) blocks and the product is spmm
        (unsplit operators only)."""
        self.op, self.comm, self.full, self.send, self.multi = op, comm, full, send, multi
        if op.remote is not None:
            self.y2 = _zeros(op, max(op.rows, 1))
            self.one = _zeros(op, 1) + 1.0

    def __call__(self, y) -> None:
        op, comm = self.op, self.comm
        st = getattr(op.kernels, "stream", None)
        cur = sa._torch().cuda.current_stream(st.device) if st is not None else None
        # the collective (or the one-rank copy) runs on torch's current
        # stream and reads `send`, which the kernels' stream produced: order
        # it behind them (both directions)
        _order(st, cur)
        if op.remote is None:
            comm.allgather(self.full, self.send)
            _order(cur, st)
            (op.kernels.spmm if self.multi else op.kernels.spmv)(self.full, y)
            return
        work = comm.allgather_start(self.full, self.send)
        if work is None:
            _order(cur, st)  # one rank: the copy was queued on the current stream
        if not op.overlap:
            comm.wait(work, st)
        op.kernels.spmv(self.send, y)  # own block only: runs while the exchange is in flight
        comm.wait(work, st)
        op.remote.spmv(self.full, self.y2)
        op.kernels.axpy_ratio(op.rows, self.one, self.one, 1.0, self.y2, y)  # y += y_remote, exact


def _order(src, dst) -> None:
    """dst waits for the work queued on src so far (no-op for one stream)."""
    if src is None or dst is None or src.cuda_stream == dst.cuda_stream:
        return
    ev = sa._torch().cuda.Event()
    ev.record(src)
    dst.wait_event(ev)


def _gathered_pair(op, comm):
    """(full gathered vector, this rank's send block); one tensor when alone."""
    if comm.world > 1:
        return _zeros(op, op.world * op.pad), _zeros(op, op.pad)
    full = _zeros(op, op.pad)
    return full, full


# -------------------------------------------------------- power iteration
def _kernel_stream(op):
    """Context that makes the operator's kernel stream torch's current one
    for a whole solve, so torch copies, host reads and the collectives are
    ordered with the HIP kernels; no-op on the default stream."""
    st = getattr(op.kernels, "stream", None)
    return sa._torch().cuda.stream(st) if st is not None else contextlib.nullcontext()


def power_iteration(op: DistOperator, iters: int, comm: Comm | None = None, x0=None, graph: bool = False,
                    block: int = 16):
    """x <- A x / ||A x||, `iters` times, on the operator's kernel stream
    (_power_iteration has the details)."""
    with _kernel_stream(op):
        return _power_iteration(op, iters, comm, x0, graph, block)


def _power_iteration(op: DistOperator, iters: int, comm: Comm | None = None, x0=None, graph: bool = False,
                     block: int = 16):
    """x <- A x / ||A x||, `iters` times.  Returns (hist, x_local): hist is a
    host array [iters, 2] of (x·Ax, ||Ax||²) per iteration — x·Ax converges
    to the dominant eigenvalue of a symmetric A — and x_local is this
    rank's block of the final normalised x (device).  graph=True (one rank)
    replays `block` iterations per HIP graph launch; same kernels, same
    bits."""
    torch = sa._torch()
    comm = comm or Comm()
    k = op.kernels
    rows = op.rows
    full, send = _gathered_pair(op, comm)
    x_loc = send[:rows]
    if x0 is None:  # deterministic start, no zero entries, not orthogonal to much
        gidx = np.arange(op.lo, op.lo + rows)
        x_loc.copy_(torch.from_numpy(1.0 + (gidx % 7) / 7.0))
    else:
        x_loc.copy_(x0)
    ws = k.dot_ws(rows)
    s0 = _zeros(op, 1)
    k.dot(rows, x_loc, x_loc, s0, ws)
    comm.allreduce(s0)
    k.scale_rsqrt(rows, s0, x_loc, x_loc)
    y = _zeros(op, max(rows, 1))
    hist = _zeros(op, 2 * max(iters, 1)).view(-1, 2)
    apply = _Apply(op, comm, full, send)

    def step(h):
        apply(y)  # gathers x (overlapped with the local part when split)
        k.dot(rows, x_loc, y, h[0:1], ws)
        k.dot(rows, y, y, h[1:2], ws)
        comm.allreduce(h)  # both scalars in one collective
        k.scale_rsqrt(rows, h[1:2], y, x_loc)

    done = 0
    if graph and comm.world == 1 and iters > block:
        # one eager step (first-call setup), then `block` steps per graph
        # replay: 7 launches per step become one graph launch per block
        step(hist[0])
        done = 1
        blk = _zeros(op, 2 * block).view(-1, 2)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for j in range(block):
                step(blk[j])
        while done + block <= iters:
            g.replay()
            hist[done:done + block].copy_(blk)
            done += block
    for it in range(done, iters):
        step(hist[it])
    return hist[:iters].cpu().numpy(), x_loc


# ---------------------------------------------------------------------- CG
def _precond_of(op, precond):
    """precond=None: the operator's own preconditioner, if it has one;
    False: none; anything else: that preconditioner."""
    if precond is False:
        return None
    return getattr(op, "precond", None) if precond is None else precond


def cg(op: DistOperator, b_loc, comm: Comm | None = None, tol: float = 1e-10, maxit: int = 1000,
       check_every: int = 10, precond=None):
    """Conjugate gradients on the operator's kernel stream (_cg); with a
    preconditioner (precond, or the operator's: _precond_of) preconditioned
    CG through the block kernels with k = 1, ld = 1 (_pcg)."""
    with _kernel_stream(op):
        M = _precond_of(op, precond)
        if M is None:
            return _cg(op, b_loc, comm, tol, maxit, check_every)
        if isinstance(M, Chebyshev):
            M.check(op)
        comm = comm or Comm()
        full, send = _gathered_pair(op, comm)
        X, its, rel = _pcg(op, comm, M, b_loc.unsqueeze(1), full, send, False, tol, maxit, check_every)
        return X[:, 0], its, float(rel[0])


def _cg(op: DistOperator, b_loc, comm: Comm | None = None, tol: float = 1e-10, maxit: int = 1000,
        check_every: int = 10):
    """Conjugate gradients for a symmetric positive definite A, x0 = 0.
    Returns (x_local, iterations, relative residual ||r||/||b||)."""
    comm = comm or Comm()
    k = op.kernels
    rows = op.rows
    full, send = _gathered_pair(op, comm)
    p = send[:rows]
    x = _zeros(op, rows)
    r = b_loc.clone()
    p.copy_(b_loc)
    apply = _Apply(op, comm, full, send)
    Ap = _zeros(op, max(rows, 1))
    ws = k.dot_ws(rows)
    rr, rr_new, pAp = _zeros(op, 1), _zeros(op, 1), _zeros(op, 1)
    k.dot(rows, r, r, rr, ws)
    comm.allreduce(rr)
    bb = float(rr.item())
    if bb == 0.0:
        return x, 0, 0.0
    it = 0
    while it < maxit:
        apply(Ap)  # gathers p (overlapped with the local part when split)
        k.dot(rows, p, Ap, pAp, ws)
        comm.allreduce(pAp)
        k.axpy_ratio(rows, rr, pAp, 1.0, p, x)  # x += alpha p
        k.axpy_ratio(rows, rr, pAp, -1.0, Ap, r)  # r -= alpha Ap
        k.dot(rows, r, r, rr_new, ws)
        comm.allreduce(rr_new)
        k.xpay_ratio(rows, rr_new, rr, r, p)  # p = r + beta p
        rr, rr_new = rr_new, rr
        it += 1
        if it % check_every == 0 or it == maxit:
            if float(rr.item()) <= tol * tol * bb:
                break
    return x, it, float(np.sqrt(max(float(rr.item()), 0.0) / bb))


# ------------------------------------------------ CG, several right-hand sides
def cg_multi(op: DistOperator, B_loc, comm: Comm | None = None, tol: float = 1e-10, maxit: int = 1000,
             check_every: int = 10, precond=None):
    """Conjugate gradients for k right-hand sides at once, on the operator's
    kernel stream (_cg_multi); preconditioned when the operator has a
    preconditioner or `precond` names one (_precond_of; False: none)."""
    with _kernel_stream(op):
        return _cg_multi(op, B_loc, comm, tol, maxit, check_every, _precond_of(op, precond))


def _check_block(op, B_loc, who: str = "cg_multi") -> int:
    """B_loc must be a contiguous float64 (rows, k >= 1) tensor on the
    operator's device; returns k."""
    torch = sa._torch()

    def refuse(why):
        return sa.SpmvError(sa.OTHER_ERROR, who, why)

    if not isinstance(B_loc, torch.Tensor) or B_loc.dtype != torch.float64:
        raise refuse("B_loc must be a float64 tensor")
    if B_loc.dim() != 2:
        raise refuse("B_loc must be 2-D (rows, k): one column per right-hand side")
    if B_loc.shape[0] != op.rows or B_loc.shape[1] < 1:
        raise refuse(f"B_loc must be ({op.rows}, k >= 1), not {tuple(B_loc.shape)}")
    if not B_loc.is_contiguous():
        raise refuse("B_loc must be contiguous (row-major, ld = k)")
    here = torch.device(op.device if op.device is not None else "cpu")
    if B_loc.device.type != here.type or (B_loc.device.index or 0) != (here.index or 0):
        raise refuse(f"B_loc must be on {here}")
    return int(B_loc.shape[1])


def _rel(rr_host, bb):
    """|r_j| / |b_j| per column from the squared norms rr_host and bb (0.0
    for a zero column b_j)."""
    out = np.zeros(bb.shape[0])
    live = bb > 0.0
    out[live] = np.sqrt(np.maximum(rr_host[live], 0.0) / bb[live])
    return out


def _cg_multi(op: DistOperator, B_loc, comm: Comm | None = None, tol: float = 1e-10, maxit: int = 1000,
              check_every: int = 10, M=None):
    """k independent CG recurrences (x0 = 0, A symmetric positive definite),
    one per column of B_loc (rows, k), sharing one multi-vector product per
    iteration; NOT block CG (no k x k Gram systems).  Returns (X_local
    (rows, k), iterations, rel: numpy (k,) of ||r_j|| / ||b_j||).

    Per iteration: one spmm, dot_multi(P, AP), two axpy_ratio_multi,
    dot_multi(R, R), one xpay_ratio_multi.  The k alphas and betas stay in
    device memory; the host reads rr every `check_every` iterations and
    stops when EVERY column has rr_j <= tol^2 bb_j, or at maxit.

    No freeze mask: a column that has converged keeps iterating with the
    others (its updates shrink with its residual).  What keeps such a column
    finite is the block kernels' rule that a zero denominator gives the
    ratio 0: once rr_j (or p_j·Ap_j) is exactly 0, alpha_j and beta_j are 0
    and the column stands still instead of turning into 0/0.  A column with
    b_j = 0 hits the rule at once: x_j = 0 exactly, rel_j = 0.0.

    Column j's bits do not depend on k or on the other columns when the
    operator's spmm is reproducible (forward plans, symmetric="expand").

    With more than one rank the gathered layout carries over: `full` is
    (world * pad, k), `send` (pad, k), one all_gather_into_tensor per
    iteration and one all-reduce per k-vector of scalars.  Unsplit operators
    only.

    M (a preconditioner): the same checks and layout, then _pcg."""
    comm = comm or Comm()
    k = op.kernels
    if op.remote is not None:
        raise sa.SpmvError(sa.OTHER_ERROR, "cg_multi", "split / overlap operators are not supported")
    if not getattr(k, "multi_supported", False):
        raise sa.SpmvError(sa.OTHER_ERROR, "cg_multi",
                           f"the operator's {_fmt_of(k)} matrix has no multi-vector run (CSR, ELL and SELL plans "
                           "have one)")
    nv = _check_block(op, B_loc)
    torch = sa._torch()
    rows = op.rows

    def zeros(*shape):
        return torch.zeros(shape, dtype=torch.float64, device=op.device)

    send = zeros(op.pad, nv)
    full = zeros(op.world * op.pad, nv) if comm.world > 1 else send
    if M is not None:
        return _pcg(op, comm, M, B_loc, full, send, True, tol, maxit, check_every)
    P = send[:rows]
    X = zeros(rows, nv)
    R = B_loc.clone()
    P.copy_(B_loc)
    apply = _Apply(op, comm, full, send, multi=True)
    AP = zeros(max(rows, 1), nv)
    ws = k.dot_multi_ws(rows, nv)
    rr, rr_new, pAp = zeros(nv), zeros(nv), zeros(nv)
    k.dot_multi(rows, R, R, rr, ws)
    comm.allreduce(rr)
    bb = rr.cpu().numpy().copy()

    if not (bb > 0.0).any():
        return X, 0, np.zeros(nv)
    it = 0
    while it < maxit:
        apply(AP)  # gathers P
        k.dot_multi(rows, P, AP, pAp, ws)
        comm.allreduce(pAp)
        k.axpy_ratio_multi(rows, rr, pAp, 1.0, P, X)  # x_j += alpha_j p_j
        k.axpy_ratio_multi(rows, rr, pAp, -1.0, AP, R)  # r_j -= alpha_j Ap_j
        k.dot_multi(rows, R, R, rr_new, ws)
        comm.allreduce(rr_new)
        k.xpay_ratio_multi(rows, rr_new, rr, R, P)  # p_j = r_j + beta_j p_j
        rr, rr_new = rr_new, rr
        it += 1
        if it % check_every == 0 or it == maxit:
            if (rr.cpu().numpy() <= tol * tol * bb).all():
                break
    return X, it, _rel(rr.cpu().numpy(), bb)


# ------------------------------------------- Chebyshev over block Jacobi
def chebyshev_coefficients(degree: int, lmin: float, lmax: float):
    """The `degree` pairs (a_i, b_i) of the Chebyshev recurrence for A z = r
    over B = M^-1 A with spectrum bounds (lmin, lmax), as host floats:
    theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta,
    rho_0 = 1 / sigma;  step 0: (0, 1 / theta);  step i >= 1:
    rho_i = 1 / (2 sigma - rho_(i-1)), a_i = rho_i rho_(i-1), b_i = 2 rho_i / delta."""
    theta, delta = (lmax + lmin) / 2.0, (lmax - lmin) / 2.0
    sigma = theta / delta
    rho = 1.0 / sigma
    coef = [(0.0, 1.0 / theta)]
    for _ in range(1, degree):
        rho_new = 1.0 / (2.0 * sigma - rho)
        coef.append((rho_new * rho, 2.0 * rho_new / delta))
        rho = rho_new
    return coef


class Chebyshev:
    """z = p(M^-1 A) M^-1 r: `degree` steps of the Chebyshev recurrence for
    A z = r over B = M^-1 A, M a block-Jacobi preconditioner (sa.BlockJacobi,
    or a test double of it), with the bounds (lmin, lmax) of B's spectrum:
        step 0:      d = (1/theta) M^-1 r,  z = d
        step i >= 1: d = a_i d + b_i M^-1 (r - A z),  z = z + d
    (chebyshev_coefficients).  degree applications of M^-1 and degree - 1
    products; a step is one fused kernel (kernels.cheb_step), so an inner step
    costs a product and a vector kernel and no reduction: the coefficients are
    host floats, known before the solve.  The polynomial is fixed, hence a
    legitimate (linear, symmetric) preconditioner for CG; it is positive
    definite when lmax bounds B's spectrum from above.  AN UNDERESTIMATED lmax
    MAKES IT INDEFINITE and CG may then break down: estimate_lmax's value is
    raised by a safety factor for that reason (build_operator's cheb_boost).
    lmin is NOT an estimate of B's smallest eigenvalue: the smoother
    convention lmax / ratio (ratio about 30) gives fewer CG iterations than
    the exact value.

    The products run through the operator's own path (_Apply: the all-gather,
    then spmm, or spmv under cg), so the iterate Z lives in a send / full
    buffer pair of this object's own, allocated on the first apply for a given
    operator and width and reused; the last step reads it and writes the
    caller's Z, together with the two dot products of a PCG iteration
    (kernels.cheb_step_dot).  Unsplit operators only."""

    def __init__(self, M, degree: int, lmin: float, lmax: float):
        if not isinstance(degree, (int, np.integer)) or isinstance(degree, bool) or not 1 <= degree <= 16:
            raise sa.SpmvError(sa.OTHER_ERROR, "Chebyshev", f"degree must be an integer in 1..16, not {degree!r}")
        lmin, lmax = float(lmin), float(lmax)
        if not (np.isfinite(lmax) and 0.0 < lmin < lmax):
            raise sa.SpmvError(sa.OTHER_ERROR, "Chebyshev", f"bounds must satisfy 0 < lmin < lmax, not ({lmin}, {lmax})")
        self.M, self.degree, self.lmin, self.lmax = M, int(degree), lmin, lmax
        self.coef = chebyshev_coefficients(self.degree, lmin, lmax)
        self._state = None  # (operator and ranks, {(width, multi): buffers}, operator)

    @staticmethod
    def check(op) -> None:
        """Refuses a split / overlap operator, before any device work."""
        if op.remote is not None:
            raise sa.SpmvError(sa.OTHER_ERROR, "Chebyshev", "split / overlap operators are not supported")

    def ws(self, kernels, n, k):
        return kernels.precond_ws(self.M, n, k)

    def _buffers(self, op, comm, nv, multi):
        """(send, az, D, product) for blocks of nv columns: made on the first
        apply of that width on this operator, then reused."""
        owner = (id(op), id(comm.dist), comm.world)
        if self._state is None or self._state[0] != owner:
            self._state = (owner, {}, op)  # the operator is kept so that its id stays its own
        made = self._state[1]
        if (nv, multi) not in made:
            torch = sa._torch()

            def zeros(r):
                return torch.zeros((r, nv) if multi else (r,), dtype=torch.float64, device=op.device)

            send = zeros(op.pad)
            full = zeros(op.world * op.pad) if comm.world > 1 else send
            D = torch.zeros((max(op.rows, 1), nv), dtype=torch.float64, device=op.device)
            made[nv, multi] = (send, zeros(max(op.rows, 1)), D, _Apply(op, comm, full, send, multi=multi))
        return made[nv, multi]

    def apply_dot(self, op, comm, R, Z, out, ws, multi: bool) -> None:
        """Z = p(M^-1 A) M^-1 R for the (rows, nv) block R, out[:nv] = column
        sums of R Z, out[nv:] of R R: 2 degree - 1 launches of the matrix and
        step kernels for nv <= 8, plus the final launch of the sums."""
        k, M, rows = op.kernels, self.M, op.rows
        send, az, D, product = self._buffers(op, comm, int(R.shape[1]), multi)
        if self.degree == 1:
            a, b = self.coef[0]
            k.cheb_step_dot(M, rows, a, b, R, None, D, None, Z, out, ws)
            return
        Zs, AZ = (t if multi else t.unsqueeze(1) for t in (send[:rows], az))
        a, b = self.coef[0]
        k.cheb_step(M, rows, a, b, R, None, D, None, Zs)
        for a, b in self.coef[1:-1]:
            product(az)  # gathers Zs
            k.cheb_step(M, rows, a, b, R, AZ, D, Zs, Zs)
        a, b = self.coef[-1]
        product(az)
        k.cheb_step_dot(M, rows, a, b, R, AZ, D, Zs, Z, out, ws)


def estimate_lmax(op: DistOperator, M, comm: Comm | None = None, iters: int = 10) -> float:
    """An estimate of the largest eigenvalue of M^-1 A (M a block-Jacobi
    preconditioner of the operator's rows) by `iters` steps of the power
    method from power_iteration's deterministic start vector: x <- M^-1 A x /
    ||M^-1 A x||.  Returns the last growth factor ||M^-1 A x|| / ||x||, which
    approaches the eigenvalue from below on the test matrices: multiply it by
    a safety factor before it bounds a Chebyshev polynomial (Chebyshev).  Built
    from the solver's kernels; one host read, at the end."""
    Chebyshev.check(op)
    if iters < 1:
        raise sa.SpmvError(sa.OTHER_ERROR, "estimate_lmax", "iters must be >= 1")
    with _kernel_stream(op):
        torch = sa._torch()
        comm = comm or Comm()
        k, rows = op.kernels, op.rows
        full, send = _gathered_pair(op, comm)
        x = send[:rows]
        gidx = np.arange(op.lo, op.lo + rows)
        x.copy_(torch.from_numpy(1.0 + (gidx % 7) / 7.0))
        ws = k.dot_ws(rows)
        pws = k.precond_ws(M, rows, 1)
        s, unused = _zeros(op, 1), _zeros(op, 2)
        k.dot(rows, x, x, s, ws)
        comm.allreduce(s)
        k.scale_rsqrt(rows, s, x, x)  # ||x|| = 1 from here on
        y, z = _zeros(op, max(rows, 1)), _zeros(op, max(rows, 1))
        product = _Apply(op, comm, full, send)
        for _ in range(iters):
            product(y)  # gathers x
            k.precond_apply_dot(M, rows, y.unsqueeze(1), z.unsqueeze(1), unused, pws)
            k.dot(rows, z, z, s, ws)
            comm.allreduce(s)
            k.scale_rsqrt(rows, s, z, x)
        return float(np.sqrt(float(s.item())))


# ------------------------------------------------------- preconditioned CG
def _pcg(op: DistOperator, comm: Comm, M, B, full, send, multi: bool, tol: float, maxit: int, check_every: int):
    """Preconditioned CG (x0 = 0) for the nv columns of B (rows, nv) with the
    preconditioner M, one recurrence per column as in _cg_multi.  `full` and
    `send` are the gathered buffers of the product: (.., nv) blocks and spmm
    when `multi`, vectors and spmv otherwise (nv = 1: cg, any operator _cg
    runs).  Returns (X (rows, nv), iterations, rel: numpy (nv,)).

    Per iteration:
        the product AP = A P                             1 launch
        pAp = dot_multi(P, AP)                           2
        x_j += alpha_j p_j, r_j -= alpha_j Ap_j          2   alpha_j = rz_j / pAp_j
        z = M^-1 r, rz' = r.z, rr = r.r  (one kernel)    2   precond_apply_dot
        p_j = z_j + beta_j p_j                           1   beta_j = rz'_j / rz_j
    which is _cg_multi's count (8 for nv <= 8): the fused kernel stands where
    dot_multi(R, R) stood.  rz' and rr are 2 nv scalars in one tensor and
    travel in ONE all-reduce.  The stop test and the returned rel use rr
    against bb, as without a preconditioner.  The zero-denominator rule of
    the ratio kernels carries over: a column with b_j = 0 has z_j = 0 and
    rz_j = 0, so alpha_j = beta_j = 0 and x_j stays exactly 0."""
    torch = sa._torch()
    k = op.kernels
    rows = op.rows
    nv = int(B.shape[1])
    if isinstance(M, Chebyshev):
        M.check(op)

    def zeros(*shape):
        return torch.zeros(shape, dtype=torch.float64, device=op.device)

    def block(t):  # a product vector as a (.., 1) block with ld = 1
        return t if multi else t.unsqueeze(1)

    P = block(send[:rows])
    X = zeros(rows, nv)
    R = B.clone()
    Z = zeros(max(rows, 1), nv)
    ap = zeros(max(rows, 1), nv) if multi else zeros(max(rows, 1))
    AP = block(ap)
    apply = _Apply(op, comm, full, send, multi=multi)
    ws = k.dot_multi_ws(rows, nv)
    if isinstance(M, Chebyshev):
        pws = M.ws(k, rows, nv)

        def precond_apply_dot(R, Z, out):
            M.apply_dot(op, comm, R, Z, out, pws, multi)
    else:
        pws = k.precond_ws(M, rows, nv)

        def precond_apply_dot(R, Z, out):
            k.precond_apply_dot(M, rows, R, Z, out, pws)
    pAp = zeros(nv)
    # (rz, rr) of the last and of the coming residual: two tensors of 2 nv
    # scalars, each with views of its halves (no slicing inside the loop)
    (s, rz, rr), (s_new, rz_new, rr_new) = ((t, t[:nv], t[nv:]) for t in (zeros(2 * nv), zeros(2 * nv)))
    precond_apply_dot(R, Z, s)
    comm.allreduce(s)
    bb = rr.cpu().numpy().copy()

    if not (bb > 0.0).any():
        return X, 0, np.zeros(nv)
    P.copy_(Z[:rows])
    it = 0
    while it < maxit:
        apply(ap)  # gathers P
        k.dot_multi(rows, P, AP, pAp, ws)
        comm.allreduce(pAp)
        k.axpy_ratio_multi(rows, rz, pAp, 1.0, P, X)  # x_j += alpha_j p_j
        k.axpy_ratio_multi(rows, rz, pAp, -1.0, AP, R)  # r_j -= alpha_j Ap_j
        precond_apply_dot(R, Z, s_new)  # z = M^-1 r, (rz', rr)
        comm.allreduce(s_new)
        k.xpay_ratio_multi(rows, rz_new, rz, Z, P)  # p_j = z_j + beta_j p_j
        (s, rz, rr), (s_new, rz_new, rr_new) = (s_new, rz_new, rr_new), (s, rz, rr)
        it += 1
        if it % check_every == 0 or it == maxit:
            if (rr.cpu().numpy() <= tol * tol * bb).all():
                break
    return X, it, _rel(rr.cpu().numpy(), bb)


# ----------------------------------------------------------------- BiCGSTAB
def bicgstab(op: DistOperator, b_loc, comm: Comm | None = None, tol: float = 1e-10, maxit: int = 1000,
             check_every: int = 10, precond=None):
    """BiCGSTAB for a general (non-symmetric) square matrix, x0 = 0, on the
    operator's kernel stream: _bicgstab through the block kernels with k = 1,
    ld = 1 and the operator's single-vector product, so split and overlap
    operators work.  precond as for cg (_precond_of): a block-Jacobi
    preconditioner, applied from the right; a Chebyshev one is refused.
    Returns (x_local, iterations, rel) with rel the TRUE relative residual
    ||b - A x|| / ||b||: after a breakdown (_bicgstab) it is what shows that
    the column has not converged."""
    with _kernel_stream(op):
        M = _bicgstab_precond(op, precond)
        X, its, rel = _bicgstab(op, comm or Comm(), M, b_loc.unsqueeze(1), False, tol, maxit, check_every)
        return X[:, 0], its, float(rel[0])


def bicgstab_multi(op: DistOperator, B_loc, comm: Comm | None = None, tol: float = 1e-10, maxit: int = 1000,
                   check_every: int = 10, precond=None):
    """BiCGSTAB for k right-hand sides at once: k independent recurrences, one
    per column of the row-major (rows, k) block B_loc, sharing two multi-vector
    products per iteration (_bicgstab); NOT a block method.  Unsplit operators
    whose matrix has a multi-vector run, as cg_multi.  Returns (X_local
    (rows, k), iterations, rel: numpy (k,) of the true ||b_j - A x_j|| / ||b_j||)."""
    with _kernel_stream(op):
        M = _bicgstab_precond(op, precond)
        if op.remote is not None:
            raise sa.SpmvError(sa.OTHER_ERROR, "bicgstab_multi", "split / overlap operators are not supported")
        if not getattr(op.kernels, "multi_supported", False):
            raise sa.SpmvError(sa.OTHER_ERROR, "bicgstab_multi",
                               f"the operator's {_fmt_of(op.kernels)} matrix has no multi-vector run (CSR, ELL "
                               "and SELL plans have one)")
        _check_block(op, B_loc, "bicgstab_multi")
        return _bicgstab(op, comm or Comm(), M, B_loc, True, tol, maxit, check_every)


def _bicgstab_precond(op, precond, who: str = "bicgstab"):
    """_precond_of, refusing a Chebyshev polynomial before any device work: its
    bounds assume a real positive spectrum, which a non-symmetric matrix does
    not have."""
    M = _precond_of(op, precond)
    if isinstance(M, Chebyshev):
        raise sa.SpmvError(sa.OTHER_ERROR, who,
                           "a Chebyshev preconditioner needs a real positive spectrum: use block Jacobi or none")
    return M


def _bicgstab(op: DistOperator, comm: Comm, M, B, multi: bool, tol: float, maxit: int, check_every: int):
    """Right-preconditioned BiCGSTAB (x0 = 0, shadow residual r^ = b) for the nv
    columns of B (rows, nv), one recurrence per column.  `multi`: the products
    are spmm on (.., nv) blocks, otherwise spmv on vectors (nv = 1, any
    operator).  M: a block-Jacobi preconditioner or None.  Returns (X (rows, nv),
    iterations, rel: numpy (nv,)).

    Per iteration, with ratio(a, b) = a / b and 0 WHEN b == 0 (the rule of the
    block ratio kernels):
        p^ = M^-1 p;  v = A p^;  rv = r^.v                 product, dot_multi (2)
        r -= alpha v              alpha = ratio(rho, rv)   axpy_ratio_multi (1)
        s^ = M^-1 r;  t = A s^;  ts = t.r, tt = t.t        product, dot2_multi (2)
        x += alpha p^ + omega s^, r -= omega t,            bicgstab_update_dot (2)
          rho' = r^.r, rr = r.r   omega = ratio(ts, tt)
        p = r + beta (p - omega v)                         bicgstab_dir (1)
          beta = ratio(rho', rv) ratio(tt, ts)   (= (rho'/rho)(alpha/omega))
    10 launches for nv <= 8 without a preconditioner, 12 with one.  Every
    scalar is a k-vector in device memory; (ts, tt) and (rho', rr) travel in one
    all-reduce each, so there are three per iteration.  The host reads rr every
    `check_every` iterations and stops when EVERY column has rr_j <= tol^2 bb_j,
    or at maxit.

    Without M, p^ is p and s^ is r: P and R are then the own blocks of the two
    gathered buffer pairs themselves, and the update kernel is called with
    Sh = R.  With M, p^ and s^ live in the pairs and P, R apart.

    Breakdown.  rv = 0, ts = 0 (hence omega = 0) or rho' = 0 on a column that
    has not converged is BiCGSTAB's breakdown.  The guarded ratios then make
    that column stand still or stagnate; nothing becomes NaN, the other columns
    go on, and THERE IS NO RESTART.  The stop test runs on the recurrence's
    rr, which can also drift from the true residual, so the returned rel is
    computed afresh, ||b_j - A x_j|| / ||b_j|| from one extra product and one
    dot_multi after the loop (0.0 for a zero column): read it to see whether a
    column converged.  A column with b_j = 0 keeps x_j = 0 exactly."""
    torch = sa._torch()
    k = op.kernels
    rows = op.rows
    nv = int(B.shape[1])

    def zeros(*shape):
        return torch.zeros(shape, dtype=torch.float64, device=op.device)

    def block(t):  # a product vector as a (.., 1) block with ld = 1
        return t if multi else t.unsqueeze(1)

    def pair():  # (product over the pair, its own block's rows as a block)
        send = zeros(op.pad, nv) if multi else zeros(op.pad)
        if comm.world > 1:
            full = zeros(op.world * op.pad, nv) if multi else zeros(op.world * op.pad)
        else:
            full = send
        return _Apply(op, comm, full, send, multi=multi), block(send[:rows])

    def product_vector():
        v = zeros(max(rows, 1), nv) if multi else zeros(max(rows, 1))
        return v, block(v)

    apply_p, Ph = pair()
    apply_s, Sh = pair()
    P, R = (Ph, Sh) if M is None else (zeros(max(rows, 1), nv), zeros(max(rows, 1), nv))
    v, V = product_vector()
    t, T = product_vector()
    X = zeros(rows, nv)
    R0 = B.clone()
    R[:rows].copy_(B)
    P[:rows].copy_(B)
    ws = k.dot_multi_ws(rows, 2 * nv)
    rv, tst = zeros(nv), zeros(2 * nv)
    ts, tt = tst[:nv], tst[nv:]
    # (rho, rr) of the last and of the coming residual, as in _pcg
    (s, rho, rr), (s_new, rho_new, rr_new) = ((u, u[:nv], u[nv:]) for u in (zeros(2 * nv), zeros(2 * nv)))
    k.dot2_multi(rows, R0, R0, R0, s, ws)  # rho = rr = b.b
    comm.allreduce(s)
    bb = rr.cpu().numpy().copy()
    if not (bb > 0.0).any():
        return X, 0, np.zeros(nv)
    it = 0
    while it < maxit:
        if M is not None:
            k.precond_apply(M, rows, P, Ph)
        apply_p(v)  # gathers p^
        k.dot_multi(rows, R0, V, rv, ws)
        comm.allreduce(rv)
        k.axpy_ratio_multi(rows, rho, rv, -1.0, V, R)  # r_j -= alpha_j v_j: r holds s
        if M is not None:
            k.precond_apply(M, rows, R, Sh)
        apply_s(t)  # gathers s^
        k.dot2_multi(rows, T, R, T, tst, ws)
        comm.allreduce(tst)
        k.bicgstab_update_dot(rows, rho, rv, ts, tt, Ph, Sh, T, R0, X, R, s_new, ws)
        comm.allreduce(s_new)
        k.bicgstab_dir(rows, rho_new, rv, tt, ts, V, R, P)
        (s, rho, rr), (s_new, rho_new, rr_new) = (s_new, rho_new, rr_new), (s, rho, rr)
        it += 1
        if it % check_every == 0 or it == maxit:
            if (rr.cpu().numpy() <= tol * tol * bb).all():
                break
    # the true residual b - A x: x through the first pair, fma(-1, A x, b) is exact
    Ph[:rows].copy_(X)
    apply_p(v)
    T[:rows].copy_(B)
    one = zeros(nv) + 1.0
    k.axpy_ratio_multi(rows, one, one, -1.0, V, T)
    k.dot_multi(rows, T, T, rv, ws)
    comm.allreduce(rv)
    return X, it, _rel(rv.cpu().numpy(), bb)


# -------------------------------------------------------------------- GMRES
def gmres(op: DistOperator, b_loc, comm: Comm | None = None, tol: float = 1e-10, maxit: int = 1000,
          restart: int = 20, precond=None):
    """Restarted GMRES(restart) for a general (non-symmetric) square matrix,
    x0 = 0, preconditioned from the right, on the operator's kernel stream
    (_gmres has the method and its launch and all-reduce counts).  Every
    operator bicgstab accepts: any format including BSR, split / overlap,
    several ranks.  precond as for bicgstab (_precond_of): a block-Jacobi
    preconditioner or none; a Chebyshev one is refused.  restart is an integer
    in 1..31 (the basis has restart + 1 <= 32 columns).  Returns (x_local,
    iterations, rel): iterations counts Arnoldi steps (one product each, plus
    one per cycle for the residual), rel is the TRUE relative residual
    ||b - A x|| / ||b||.  The solver returns only when that residual is
    <= tol, or at maxit steps.  Refusals (restart, the shape, dtype or device of
    b_loc, the preconditioner) are an SpmvError before any device work."""
    if not isinstance(restart, (int, np.integer)) or isinstance(restart, bool) or \
            not 1 <= restart <= sa.KRYLOV_MAX_COLS - 1:
        raise sa.SpmvError(sa.OTHER_ERROR, "gmres",
                           f"restart must be an integer in 1..{sa.KRYLOV_MAX_COLS - 1}, not {restart!r}")
    torch = sa._torch()
    if not isinstance(b_loc, torch.Tensor) or b_loc.dim() != 1:
        raise sa.SpmvError(sa.OTHER_ERROR, "gmres", f"b_loc must be a 1-D float64 tensor of {op.rows} entries")
    _check_block(op, b_loc.unsqueeze(1), "gmres")
    M = _bicgstab_precond(op, precond, "gmres")
    with _kernel_stream(op):
        return _gmres(op, comm or Comm(), M, b_loc, float(tol), int(maxit), int(restart))


def _givens_column(H, cs, sn, g, j) -> None:
    """Applies the j rotations so far to column j of the Hessenberg matrix H,
    makes rotation j (it zeroes H[j + 1, j]) and applies it to H and to the
    right-hand side g.  A zero column gets the identity rotation."""
    for i in range(j):
        a, b = H[i, j], H[i + 1, j]
        H[i, j], H[i + 1, j] = cs[i] * a + sn[i] * b, cs[i] * b - sn[i] * a
    a, b = H[j, j], H[j + 1, j]
    d = float(np.hypot(a, b))
    cs[j], sn[j] = (1.0, 0.0) if d == 0.0 else (a / d, b / d)
    H[j, j], H[j + 1, j] = d, 0.0
    g[j + 1] = -sn[j] * g[j]
    g[j] = cs[j] * g[j]


def _back_substitute(H, g, kk):
    """y with H[:kk, :kk] y = g[:kk] for the upper triangle the rotations left;
    a zero pivot (a singular matrix) gives y_i = 0, not a division by zero."""
    y = np.zeros(kk)
    for i in range(kk - 1, -1, -1):
        s = g[i] - float(H[i, i + 1:kk] @ y[i + 1:])
        y[i] = 0.0 if H[i, i] == 0.0 else s / H[i, i]
    return y


def _gmres(op: DistOperator, comm: Comm, M, b_loc, tol: float, maxit: int, m: int):
    """Right-preconditioned GMRES(m), x0 = 0: A M^-1 u = b, x = M^-1 u.  The
    basis V is one row-major (rows, m + 1) block; the Hessenberg matrix, the
    Givens rotations and the small triangular solve live on the host.

    Step j of a cycle (c = j + 1 basis columns so far), classical Gram-Schmidt
    applied twice (CGS2), the sums of each pass fused into the pass before it:
        send = M^-1 v_j                      precond_apply (1), or nothing: the
                                             normalisation already wrote v_j there
        w = A send                           the product (1; 3 on a split operator)
        h1 = V^T w                           krylov_project_dot, h = None (2)
        w' = w - V h1,  h2 = V^T w'          krylov_project_dot (2)
        w'' = w' - V h2 into column c,       krylov_project_dot (2)
          V^T w'' and ||w''||^2
        v_c = w'' / ||w''||                  krylov_normalize (1)
    8 launches without a preconditioner, 9 with one, whatever c; THREE
    all-reduces of c + 1 scalars (each pass needs the sums of the one before),
    and ONE host visit, which reads the three results together.  Then on the
    host H[:c, j] = h1 + h2, H[c, j] = ||w''||, the rotations so far are applied
    to the column and a new one is made (_givens_column); |g[c]| is the residual
    norm of the least-squares problem.

    A cycle ends after m steps, when |g[c]| <= tol ||b||, when H[c, j] = 0 (the
    Krylov space is invariant: the solution lies in it) or at maxit steps.
    Then y solves the triangular system, t = V y (krylov_combine, 1 launch),
    x += M^-1 t, and the TRUE residual r = b - A x comes from one extra
    product, as at the end of _bicgstab: the solver returns only when
    ||r|| <= tol ||b||, or at maxit; otherwise r / ||r|| is the next cycle's v_0.
    The estimate |g| can drift below the true residual in a long cycle; the
    return value never rests on it.

    Zero norms: b = 0 returns x = 0, 0 iterations, rel = 0.0.  ||w''|| = 0
    makes v_c = 0 (krylov_normalize's rule) and ends the cycle; a zero pivot in
    the triangle gives a zero coefficient.  Nothing becomes NaN."""
    torch = sa._torch()
    k = op.kernels
    rows = op.rows

    def zeros(*shape):
        return torch.zeros(shape, dtype=torch.float64, device=op.device)

    full, send = _gathered_pair(op, comm)
    apply = _Apply(op, comm, full, send)
    copy = send[:rows] if M is None else None  # where krylov_normalize leaves the product's input
    Z = send[:rows].unsqueeze(1)
    V = zeros(max(rows, 1), m + 1)
    w, t = zeros(max(rows, 1)), zeros(max(rows, 1))
    W, T = w.unsqueeze(1), t.unsqueeze(1)
    B = b_loc.unsqueeze(1)
    x = zeros(rows)
    X = x.unsqueeze(1)
    ws = k.krylov_project_ws(rows)
    dws = k.dot_multi_ws(rows, 1)
    d = zeros(3, m + 2)  # the sums of a step's three passes
    rr, one = zeros(1), zeros(1) + 1.0
    k.dot_multi(rows, B, B, rr, dws)
    comm.allreduce(rr)
    bb = float(rr.item())
    if bb == 0.0:
        return x, 0, 0.0
    bnorm = float(np.sqrt(bb))
    k.krylov_normalize(rows, rr, B, V[:, 0:1], copy)
    res = bnorm
    its = 0
    while True:
        H = np.zeros((m + 1, m))
        cs, sn, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        g[0] = res
        kk = 0
        while kk < m and its < maxit:
            j, c = kk, kk + 1
            Vc, v_new = V[:, :c], V[:, c:c + 1]
            if M is not None:
                k.precond_apply(M, rows, V[:, j:j + 1], Z)
            apply(w)  # gathers send
            for p, (h, dst) in enumerate(((None, None), (d[0, :c], W), (d[1, :c], v_new))):
                k.krylov_project_dot(rows, Vc, h, W, dst, d[p, :c + 1], ws)
                comm.allreduce(d[p, :c + 1])
            k.krylov_normalize(rows, d[2, c:c + 1], v_new, v_new, copy)
            hd = d.cpu().numpy()  # the step's one host visit
            H[:c, j] = hd[0, :c] + hd[1, :c]
            H[c, j] = hnext = float(np.sqrt(max(hd[2, c], 0.0)))
            _givens_column(H, cs, sn, g, j)
            kk += 1
            its += 1
            if abs(g[kk]) <= tol * bnorm or hnext == 0.0:
                break
        if kk > 0:
            k.krylov_combine(rows, V[:, :kk], _back_substitute(H, g, kk), T)
            if M is not None:
                k.precond_apply(M, rows, T, W)
            k.axpy_ratio_multi(rows, one, one, 1.0, T if M is None else W, X)  # x += M^-1 V y
        # the true residual b - A x: fma(-1, A x, b) is exact
        send[:rows].copy_(x)
        apply(w)
        T[:rows].copy_(B)
        k.axpy_ratio_multi(rows, one, one, -1.0, W, T)
        k.dot_multi(rows, T, T, rr, dws)
        comm.allreduce(rr)
        res = float(np.sqrt(max(float(rr.item()), 0.0)))
        if res <= tol * bnorm or its >= maxit or kk == 0:
            return x, its, res / bnorm
        k.krylov_normalize(rows, rr, T, V[:, 0:1], copy)


# ------------------------------------------------------------------- LOBPCG
def lobpcg(op: DistOperator, k: int | None = None, X0=None, largest: bool = False, tol: float = 1e-8,
           atol: float = 0.0, maxit: int = 500, precond=None, comm: Comm | None = None, seed: int = 0):
    """The k <= 8 smallest (largest=True: largest) eigenpairs of the symmetric
    operator `op` by LOBPCG, on the operator's kernel stream (_lobpcg has the
    method).  k defaults to X0's width, or to 1 without an X0.  Returns
    (lam, X, iterations, res): lam a numpy (k,) array, ascending (descending for
    `largest`); X this rank's (rows, k) block with X^T X = I; res[j] the TRUE
    residual ||A x_j - lam_j x_j||_2, computed afresh from one extra product
    after the loop (the rule of bicgstab's rel), lam_j the Rayleigh quotient of
    x_j from that same product.  Column j has converged when
    res_j <= tol |lam_j| + atol; the loop ends when every column has, or at
    maxit.

    Every operator cg_multi runs on: unsplit operators whose matrix has a
    multi-vector run, symmetric="fused" | "expand", several ranks.  precond as
    for cg (_precond_of): the operator's block-Jacobi preconditioner by default,
    False for none; a Chebyshev one is refused.  X0: a float64 (rows, k) tensor
    on the operator's device with independent columns; default
    numpy.random.default_rng(seed).standard_normal((n, k)) indexed by GLOBAL
    row, so the start does not depend on the number of ranks.  Refused before
    any device work: k outside 1..8, 3k > n, a non-square operator, a format
    without a multi-vector run, an X0 of the wrong shape or dtype."""
    with _kernel_stream(op):
        M = _precond_of(op, precond)
        if isinstance(M, Chebyshev):
            raise sa.SpmvError(sa.OTHER_ERROR, "lobpcg",
                               "a Chebyshev preconditioner is not supported: use block Jacobi or none")
        k = _lobpcg_check(op, k, X0)
        return _lobpcg(op, k, X0, bool(largest), float(tol), float(atol), int(maxit), M, comm or Comm(), seed)


def _lobpcg_check(op, k, X0) -> int:
    """The refusals of lobpcg, all before any device work; returns k."""
    torch = sa._torch()

    def refuse(why):
        return sa.SpmvError(sa.OTHER_ERROR, "lobpcg", why)

    kn = op.kernels
    if op.remote is not None:
        raise refuse("split / overlap operators are not supported")
    if not getattr(kn, "multi_supported", False):
        raise refuse(f"the operator's {_fmt_of(kn)} matrix has no multi-vector run (CSR, ELL and SELL plans have one)")
    # a shard of a square matrix: this rank's rows, and columns either in the
    # gathered layout or (the stored half of symmetric=...) the matrix's own
    mat = getattr(kn, "dm", None)
    shape = (mat.n_rows, mat.n_cols) if mat is not None else getattr(getattr(kn, "A", None), "shape", None)
    if shape is not None and (shape[0] != op.rows or shape[1] not in (op.n, op.world * op.pad)):
        raise refuse(f"the operator is not square ({op.n} rows, a {shape[0]} x {shape[1]} shard on {op.world} ranks)")
    if X0 is not None:
        if not isinstance(X0, torch.Tensor) or X0.dtype != torch.float64:
            raise refuse("X0 must be a float64 tensor")
        if X0.dim() != 2 or X0.shape[0] != op.rows or (k is not None and X0.shape[1] != k):
            raise refuse(f"X0 must be ({op.rows}, k), not {tuple(X0.shape)}")
        here = torch.device(op.device if op.device is not None else "cpu")
        if X0.device.type != here.type or (X0.device.index or 0) != (here.index or 0):
            raise refuse(f"X0 must be on {here}")
        k = int(X0.shape[1])
    k = 1 if k is None else k
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 1 <= k <= 8:
        raise refuse(f"k must be in 1..8, not {k!r}")
    if 3 * k > op.n:
        raise refuse(f"k = {k} needs a basis of 3k = {3 * k} vectors, the matrix has {op.n} rows")
    return int(k)


def _chol_inverse(G: np.ndarray):
    """R^-1 for the Gram matrix G = R^T R of a block V (V R^-1 is orthonormal),
    or None when G is not numerically positive definite.  G is scaled to a unit
    diagonal first, so a column of V that is tiny against the others (a
    converged residual) does not by itself make the factorisation fail."""
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.sqrt(np.diag(G))
        if not (np.isfinite(d).all() and (d > 0.0).all()):
            return None
        Gs = G / np.outer(d, d)
    Gs = 0.5 * (Gs + Gs.T)
    if not np.isfinite(Gs).all():
        return None
    try:
        L = np.linalg.cholesky(Gs)
    except np.linalg.LinAlgError:
        return None
    Rinv = np.linalg.inv(L).T / d[:, None]
    return Rinv if np.isfinite(Rinv).all() else None


def _ortho_matrix(B: np.ndarray, G: np.ndarray):
    """The matrix C of one projection + Cholesky-QR pass of a block V against
    an orthonormal basis Q: with B = Q^T V (q x k, q may be 0) and G = V^T V,
    (V - Q B) has the Gram matrix G - B^T B = R^T R, and [Q V] C with
    C = [-B R^-1; R^-1] is orthonormal and orthogonal to Q.  None when the
    factorisation fails."""
    Rinv = _chol_inverse(G - B.T @ B)
    return None if Rinv is None else np.vstack([-B @ Rinv, Rinv])


def _lobpcg(op: DistOperator, k: int, X0, largest: bool, tol: float, atol: float, maxit: int, M, comm: Comm, seed):
    """LOBPCG (locally optimal block preconditioned CG) in the orthonormal-basis
    form of Hetmaniuk and Lehoucq, standard problem, no locking.  The basis
    S = [X W P] is ONE row-major (rows, 3k) block and AS = [AX AW AP] another,
    so that a Gram matrix over any part of the basis is one kernel.

    Per iteration:
        R = AX - X diag(lam)                       block_combine of [AX X]
        W = M^-1 R (precond_apply), or R itself
        W: projected against X and orthonormalised, twice:
           gram ([X W]^T W), host Cholesky of W^T W - B^T B, block_combine
        AW = A W                                   the ONE spmm
        P: projected against X and W and orthonormalised in the same way,
           AP following by the same combinations of [AX AW AP]
        T = S^T A S                                one gram, 3k x 3k
        numpy.linalg.eigh(T) on the host: C
        X+ = S C, AX+ = AS C, P+ = [W P] C_WP, AP+ likewise: block_combine
           into the spare pair of blocks, which is then swapped in
    The first iteration, and one whose P fails its Cholesky factorisation (a
    restart), run on [X W].  A factorisation of W's Gram matrix that fails ends
    the loop: the residual has then reached rounding.  A rank-deficient X0
    raises SpmvError.

    THE SMALL MATRICES GO TO THE HOST: every group of Gram matrices computed
    together is all-reduced once (Comm) and read by the host, which
    synchronises with the stream, five times per iteration.  That is inherent
    in the method (the Cholesky factors and the 3k x 3k eigenproblem are host
    work); everything of length `rows` stays on the device, and C travels back
    in kernel arguments.

    The stop test runs on the recurrence's residual (AX is carried along, not
    recomputed).  When it passes, lam and the true residual are computed from one
    extra product (lam_j = x_j^T A x_j / x_j^T x_j: the carried Ritz values and
    AX gather about one rounding of ||A|| per iteration); if those do not pass,
    the fresh A X and lam replace the carried ones and the loop goes on.  The
    returned lam and res are always the fresh ones.

    With a forward or symmetric="expand" operator every kernel is deterministic
    (fixed reduction trees, fma chains in a fixed order) and so is the host
    step: two calls with the same arguments return the same bits.
    symmetric="fused" is not reproducible (its product is not)."""
    torch = sa._torch()
    kn = op.kernels
    rows, n = op.rows, op.n

    def zeros(*shape):
        return torch.zeros(shape, dtype=torch.float64, device=op.device)

    def cols(T, j):  # block j of a basis block: X, W, P = 0, 1, 2
        return T[:, j * k:(j + 1) * k]

    # two (S, AS) pairs: the combinations of an iteration's end write the spare
    # one.  S has `pad` rows: alone, its W columns are the product's input.
    pairs = [(zeros(op.pad, 3 * k), zeros(max(rows, 1), 3 * k)) for _ in range(2)]
    t1, t2, t3 = (zeros(max(rows, 1), k) for _ in range(3))
    if comm.world > 1:
        send, full = zeros(op.pad, k), zeros(op.world * op.pad, k)
        apply_shared = _Apply(op, comm, full, send, multi=True)
    else:
        applies = {id(S): _Apply(op, comm, cols(S, 1), cols(S, 1), multi=True) for S, _ in pairs}

    def product(S, AS):  # AW = A W
        if comm.world > 1:
            send[:rows].copy_(cols(S, 1)[:rows])
            apply_shared(cols(AS, 1))
        else:
            applies[id(S)](cols(AS, 1))

    gout = zeros(9 * k * k + k)
    ws = kn.gram_ws(rows, 3 * k, 3 * k)
    ws_dot, ws_dot2 = kn.dot_multi_ws(rows, k), kn.dot_multi_ws(rows, 2 * k)

    def grams(*blocks, norms=None):
        """One group: the Gram matrices of the (A, B) pairs, and the column
        sums of squares of `norms`, in one all-reduce and one host read."""
        off = 0
        shapes = []
        for A, B in blocks:
            ka, kb = A.shape[1], B.shape[1]
            kn.gram(rows, A, B, gout[off:off + ka * kb], ws)
            shapes.append((ka, kb))
            off += ka * kb
        if norms is not None:
            kn.dot_multi(rows, norms, norms, gout[off:off + k], ws_dot)
            off += k
        comm.allreduce(gout[:off])
        host = gout[:off].cpu().numpy()
        out, off = [], 0
        for ka, kb in shapes:
            out.append(host[off:off + ka * kb].reshape(ka, kb).copy())
            off += ka * kb
        if norms is not None:
            out.append(host[off:off + k].copy())
        return out

    def residual_matrix(lam):  # R = [AX X] [I; -diag(lam)]
        return np.vstack([np.eye(k), -np.diag(lam)])

    (S, AS), (S2, AS2) = pairs
    X, W = cols(S, 0), cols(S, 1)
    # start: X0 -> t1, orthonormalised twice into W's place (the product's
    # input), AW = A W, then Rayleigh-Ritz on that block alone into X, AX
    if X0 is None:
        start = np.random.default_rng(seed).standard_normal((n, k))[op.lo:op.lo + rows]
        t1[:rows].copy_(torch.from_numpy(np.ascontiguousarray(start)))
    else:
        t1[:rows].copy_(X0)
    none = np.zeros((0, k))
    for src, dst in ((t1, t2), (t2, W)):
        (G,) = grams((src, src))
        C = _ortho_matrix(none, G)
        if C is None:
            raise sa.SpmvError(sa.OTHER_ERROR, "lobpcg", "X0 is rank-deficient (its Gram matrix has no Cholesky "
                                                         "factorisation)")
        kn.block_combine(rows, C, [src], dst)
    product(S, AS)
    (T,) = grams((W, cols(AS, 1)))
    lam, V = np.linalg.eigh(0.5 * (T + T.T))
    order = np.argsort(-lam if largest else lam, kind="stable")
    lam, V = lam[order], np.ascontiguousarray(V[:, order])
    kn.block_combine(rows, V, [W], X)
    kn.block_combine(rows, V, [cols(AS, 1)], cols(AS, 0))

    def converged(res, lam):
        return bool((res <= tol * np.abs(lam) + atol).all())

    def true_residual(S, AS):
        """(lam, res) afresh from one more product: X goes through W's place,
        whose old content no later step reads; lam_j is the Rayleigh quotient
        x_j^T (A x_j) / x_j^T x_j of the fresh product (the carried Ritz value
        has the drift of the carried AX in it) and res_j = ||A x_j - lam_j x_j||."""
        X, W, AW = cols(S, 0), cols(S, 1), cols(AS, 1)
        W[:rows].copy_(X[:rows])
        product(S, AS)
        kn.dot2_multi(rows, X, AW, X, gout[:2 * k], ws_dot2)
        comm.allreduce(gout[:2 * k])
        q = gout[:2 * k].cpu().numpy()
        fresh = q[:k] / q[k:]
        kn.block_combine(rows, residual_matrix(fresh), [AW, X], t1)
        kn.dot_multi(rows, t1, t1, gout[:k], ws_dot)
        comm.allreduce(gout[:k])
        return fresh, np.sqrt(np.maximum(gout[:k].cpu().numpy(), 0.0))

    has_p = False
    it = 0
    refreshed = -1
    res_true = None
    while True:
        X, W, P = (cols(S, j) for j in range(3))
        AX, AW, AP = (cols(AS, j) for j in range(3))
        XW = S[:, :2 * k]
        # the residual, into W's place (or, under a preconditioner, beside it)
        if M is None:
            kn.block_combine(rows, residual_matrix(lam), [AX, X], W)
            G1, = grams((XW, W))
            rr = np.diag(G1[k:]).copy()
        else:
            kn.block_combine(rows, residual_matrix(lam), [AX, X], t1)
            kn.precond_apply(M, rows, t1, W)
            G1, rr = grams((XW, W), norms=t1)
        res = np.sqrt(np.maximum(rr, 0.0))
        if converged(res, lam) or it >= maxit:
            # the recurrence's word is checked against the true residual; where
            # the carried AX has drifted too far, the fresh A X (now in AW's
            # place) replaces it and the loop goes on, once per iteration
            lam_true, res_true = true_residual(S, AS)
            if converged(res_true, lam_true) or it >= maxit or refreshed == it:
                break
            AX[:rows].copy_(AW[:rows])
            lam, refreshed = lam_true, it
            continue
        res_true = None
        # W: two passes of projection against X + Cholesky QR (W -> t2 -> W)
        C = _ortho_matrix(G1[:k], G1[k:])
        if C is None:
            break
        kn.block_combine(rows, C, [X, W], t2)
        Gx, Gw = grams((X, t2), (t2, t2))
        C = _ortho_matrix(Gx, Gw)
        if C is None:
            break
        kn.block_combine(rows, C, [X, t2], W)
        product(S, AS)
        # P (and AP by the same matrix): against X and W (P -> t2 -> P)
        m = 2 * k
        if has_p:
            G3, = grams((S, P))
            C = _ortho_matrix(G3[:2 * k], G3[2 * k:])
            if C is not None:
                kn.block_combine(rows, C, [X, W, P], t2)
                kn.block_combine(rows, C, [AX, AW, AP], t3)
                Gq, Gp = grams((XW, t2), (t2, t2))
                C = _ortho_matrix(Gq, Gp)
                if C is not None:
                    kn.block_combine(rows, C, [X, W, t2], P)
                    kn.block_combine(rows, C, [AX, AW, t3], AP)
                    m = 3 * k
        # Rayleigh-Ritz on the orthonormal basis
        T, = grams((S[:, :m], AS[:, :m]))
        w, V = np.linalg.eigh(0.5 * (T + T.T))
        pick = np.arange(m - 1, m - 1 - k, -1) if largest else np.arange(k)
        lam = w[pick]
        C = np.ascontiguousarray(V[:, pick])
        basis = [X, W, P][:m // k]
        images = [AX, AW, AP][:m // k]
        kn.block_combine(rows, C, basis, cols(S2, 0))
        kn.block_combine(rows, C, images, cols(AS2, 0))
        kn.block_combine(rows, C[k:], basis[1:], cols(S2, 2))
        kn.block_combine(rows, C[k:], images[1:], cols(AS2, 2))
        (S, AS), (S2, AS2) = (S2, AS2), (S, AS)
        has_p = True
        it += 1
    if res_true is None:  # W's factorisation failed
        lam_true, res_true = true_residual(S, AS)
    X = cols(S, 0)
    order = np.argsort(-lam_true if largest else lam_true, kind="stable")
    if not np.array_equal(order, np.arange(k)):
        # two Rayleigh quotients a rounding apart changed places: the columns
        # follow (a chain over one 1.0 and zeros copies exactly)
        kn.block_combine(rows, np.eye(k)[:, order], [X], cols(S2, 0))
        X, lam_true, res_true = cols(S2, 0), lam_true[order], res_true[order]
    return lam_true.copy(), X[:rows].clone(), it, res_true
