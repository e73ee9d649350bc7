"""Cases, restated rules and references for the factor-and-solve chain (pchol.hip and the first
part of linalg.hip): the code between x4_q and W_q.  No GPU here; test_factor_cases.py checks this
file on the CPU and test_gpu_factor_chain.py runs the device against it.

Three layers:
  * the dispatch rules restated (pchol path and panels, the merged substitution's partition, its
    split-K and sub-batches, the selection panel variant), compared with fisdf_factor_plan;
  * references in np.clongdouble / np.longdouble (64-bit mantissa): greedy pivoted Cholesky, the
    factor along a given pivot order, forward and adjoint substitution;
  * the same algorithms in plain float64, blocked where the device is blocked.  They are used only
    to measure what float64 arithmetic alone costs against the long-double reference: a device
    result may be 16 times that far from the reference (another summation order, the
    3-multiplication complex product), never less than n eps.  The bound so comes from the
    reference side, not from the code under test.
"""
import functools
from collections import namedtuple

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
EPS = float(np.finfo(np.float64).eps)
BOUND_FACTOR = 16.0

# ------------------------------------------------------------------ restated rules
BLOCKED, STEP = 0, 1
PCHOL_ROWS = 1024      # rows one pchol_panel workgroup holds (one per thread)
PCHOL_NB = 32          # pivots per panel
SEL_THREADS = 512      # threads of the real selection panel kernel


def pchol_path(n):
    return BLOCKED if n <= PCHOL_ROWS else STEP


def pchol_panels(rmax):
    """(j0, width) of every panel launch of the blocked path."""
    return [(j0, min(PCHOL_NB, rmax - j0)) for j0 in range(0, rmax, PCHOL_NB)]


def merged_partition(r):
    """s0 and the (b0, m, b1) of every block row: the partial block first, then full 64s."""
    nblk = (r + 63) // 64
    s0 = r - 64 * (nblk - 1)
    rows, b0 = [], 0
    for b in range(nblk):
        m = s0 if b == 0 else 64
        rows.append((b0, m, b0 + m))
        b0 += m
    return s0, rows


def trsm_split_k(nc, b1):
    if b1 < 256:
        return 1
    tiles = (nc + 63) // 64
    return max(1, min(256 // max(tiles, 1), b1 // 128, 16))


def merged_rows(r, ncol, batch, lower_rhs, work_elems):
    """(b0, m, b1, nc, ks, sub) per block row; work_elems None = no workspace (no split-K);
    sub = 0: the workspace cannot hold one matrix's partials (the call fails)."""
    out = []
    for b0, m, b1 in merged_partition(r)[1]:
        nc = min(ncol, b1) if lower_rhs else ncol
        ks = trsm_split_k(nc, b1) if work_elems is not None else 1
        sub = batch
        if ks > 1:
            per = ks * m * nc
            sub = 0 if per > work_elems else max(1, min(batch, work_elems // per))
        out.append((b0, m, b1, nc, ks, sub))
    return out


def merged_partials(r, ncol, lower_rhs):
    """Largest split-K partial of one matrix over the block rows (0: no row splits)."""
    return max([ks * m * nc for _, m, _, nc, ks, _ in merged_rows(r, ncol, 1, lower_rhs, 1 << 62)
                if ks > 1] or [0])


def split_work_elems(r, batch):
    return batch * max(merged_partials(r, r, False), merged_partials(r, r, True))


def sel_variant(n):
    """(rows per thread, pivots per panel) of pchol_real_panel for an n x n Gram."""
    per = (n + SEL_THREADS - 1) // SEL_THREADS
    if n < 1 or per > 8:
        return (0, 0)
    return (2, 16) if per <= 2 else (4, 16) if per <= 4 else (7, 12) if per <= 7 else (8, 8)


def sel_panels(n, rmax):
    nb = sel_variant(n)[1]
    return [(j0, min(nb, rmax - j0)) for j0 in range(0, rmax, nb)]


# ------------------------------------------------------------------ references
Fact = namedtuple("Fact", "piv rank L thr dmax min_gap last_pivot resid_after")


def relerr(x, ref):
    """max |x - ref| / max |ref| (long double)."""
    ref = np.asarray(ref)
    if ref.size == 0:
        return 0.0
    wide = CLD if np.iscomplexobj(ref) or np.iscomplexobj(x) else LD
    den = np.abs(ref).max()
    return float(np.abs(np.asarray(x, wide) - ref.astype(wide)).max() / (den if den > 0 else 1))


def bound(err64, n):
    return max(BOUND_FACTOR * err64, n * EPS)


def _threshold(dmax, n, tol_rel, tol_abs):
    thr = tol_rel * dmax if tol_rel > 0 else n * EPS * dmax
    return type(thr)(tol_abs) if tol_abs > thr else thr


def _gap(dm, p, dmax):
    if dm.size < 2:
        return np.inf
    second = np.partition(dm, -2)[-2]
    return np.inf if second == -np.inf else float((dm[p] - second) / dmax)


def greedy_ld(col, diag, rmax, tol_rel, tol_abs=0.0, real=False):
    """Greedy pivoted Cholesky in long double.  col(p): column p of the matrix, diag: its
    diagonal.  arg-max of the residual diagonal with the first index on ties, stop when
    not d_max > thr, thr = max(tol_rel > 0 ? tol_rel m : n eps m, tol_abs), at most rmax pivots.
    L (n x rank): rows in the matrix's own order."""
    ct = LD if real else CLD
    d = np.asarray(diag, LD).copy()
    n = d.size
    dmax = d.max()
    thr = _threshold(dmax, n, LD(tol_rel), LD(tol_abs))
    L = np.zeros((n, rmax), ct)
    chosen = np.zeros(n, bool)
    piv, gaps, last = [], [], np.inf
    for j in range(rmax):
        dm = np.where(chosen, -np.inf, d)
        p = int(np.argmax(dm))
        if not dm[p] > thr:
            break
        gaps.append(_gap(dm, p, dmax))
        last = float(dm[p])
        sq = np.sqrt(dm[p])
        c = (np.asarray(col(p), ct) - L[:, :j] @ np.conj(L[p, :j])) / sq
        c[chosen] = 0
        c[p] = sq
        L[:, j] = c
        chosen[p] = True
        d = d - (c.real ** 2 + c.imag ** 2 if not real else c * c)
        piv.append(p)
    rest = d[~chosen]
    resid = float(rest.max()) if rest.size else 0.0
    return Fact(np.array(piv, np.int32), len(piv), L[:, :len(piv)], float(thr), float(dmax),
                min(gaps) if gaps else np.inf, last, resid)


def pchol_ld(A, rmax, tol_rel, tol_abs=0.0):
    A = np.asarray(A)
    return greedy_ld(lambda p: A[:, p], A.diagonal().real, rmax, tol_rel, tol_abs)


def factor_along_ld(A, order):
    """The factor of A along a given pivot order (long double), rows in A's own order."""
    A = np.asarray(A).astype(CLD)
    n = A.shape[0]
    L = np.zeros((n, len(order)), CLD)
    done = np.zeros(n, bool)
    for j, p in enumerate(order):
        c = A[:, p] - L[:, :j] @ np.conj(L[p, :j])
        sq = np.sqrt(c[p].real)
        c = c / sq
        c[done] = 0
        c[p] = sq
        L[:, j] = c
        done[p] = True
    return L


def solve_lower_ld(L, B):
    """X = L^{-1} B by forward substitution (long double)."""
    L, B = np.asarray(L).astype(CLD), np.asarray(B).astype(CLD)
    X = np.zeros_like(B)
    for i in range(L.shape[0]):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def solve_adjoint_ld(L, B):
    """X = L^{-H} B by backward substitution with L^H (long double)."""
    L, B = np.asarray(L).astype(CLD), np.asarray(B).astype(CLD)
    X = np.zeros_like(B)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (B[i] - np.conj(L[i + 1:, i]) @ X[i + 1:]) / np.conj(L[i, i])
    return X


# ------------------------------------------------------------------ float64 restatements
def greedy_f64(A, rmax, tol_rel, tol_abs=0.0, nb=None, skip_updates=False):
    """The device's pivoted Cholesky in float64 numpy.  nb None: left-looking, one pivot per step
    from the untouched matrix (pchol_step / pchol_pick).  nb: right-looking panels of nb pivots on
    a trailing copy W (only its lower triangle is read), W -= L_panel L_panel^H after each panel
    (pchol_panel<32>; pchol_real_panel for a real A).  skip_updates leaves the trailing updates out:
    a wrong algorithm, run to show that an input's pivots depend on them."""
    A = np.asarray(A)
    n = A.shape[0]
    d = A.diagonal().real.astype(np.float64).copy()
    dmax = d.max()
    thr = _threshold(dmax, n, float(tol_rel), float(tol_abs))
    L = np.zeros((n, rmax), A.dtype)
    W = A.copy() if nb else A
    chosen = np.zeros(n, bool)
    piv, gaps, last = [], [], np.inf
    j0 = 0
    for j in range(rmax):
        if nb and j > 0 and j % nb == 0:
            P = L[:, j0:j]
            W = W if skip_updates else W - P @ P.conj().T
            j0 = j
        dm = np.where(chosen, -np.inf, d)
        p = int(np.argmax(dm))
        if not dm[p] > thr:
            break
        gaps.append(_gap(dm, p, dmax))
        last = float(dm[p])
        sq = np.sqrt(dm[p])
        if nb:  # column p of the Hermitian trailing matrix from its lower triangle
            w = np.concatenate([W[p, :p].conj(), W[p:, p]])
        else:
            w = A[:, p]
        c = (w - L[:, j0:j] @ L[p, j0:j].conj()) / sq
        c[chosen] = 0
        c[p] = sq
        L[:, j] = c
        chosen[p] = True
        d = d - (c.real ** 2 + c.imag ** 2)
        piv.append(p)
    rest = d[~chosen]
    return Fact(np.array(piv, np.int32), len(piv), L[:, :len(piv)], float(thr), float(dmax),
                min(gaps) if gaps else np.inf, last, float(rest.max()) if rest.size else 0.0)


def chol_f64(A):
    """Right-looking unpivoted Cholesky (float64): the factor and every pivot as it is met, up to
    and including the first one that is not positive (NaN after it)."""
    W = np.array(A, np.complex128)
    n = W.shape[0]
    pivots = np.full(n, np.nan)
    for k in range(n):
        pivots[k] = W[k, k].real
        if not pivots[k] > 0:
            break
        lk = np.sqrt(pivots[k])
        W[k, k] = lk
        W[k + 1:, k] /= lk
        W[k + 1:, k + 1:] -= np.outer(W[k + 1:, k], W[k + 1:, k].conj())
    return np.tril(W), pivots


def _trinv_f64(T):
    m = T.shape[0]
    X = np.zeros_like(T)
    for i in range(m):
        e = np.zeros(m, T.dtype)
        e[i] = 1
        X[i] = (e - T[i, :i] @ X[:i]) / T[i, i]
    return X


def trsm_blocked_f64(L, B, lower, nb=64):
    """trsm_blocked in float64: per 64-row block one update with the solved blocks and one product
    with the diagonal block's inverse (forward with L, or backward with L^H)."""
    L = np.asarray(L)
    r = L.shape[0]
    B = np.array(B, np.complex128)
    X = np.zeros_like(B)
    blocks = [(b0, min(r, b0 + nb)) for b0 in range(0, r, nb)]
    for b0, b1 in (blocks if lower else blocks[::-1]):
        Ti = _trinv_f64(L[b0:b1, b0:b1])
        if lower:
            rhs = B[b0:b1] - L[b0:b1, :b0] @ X[:b0]
            X[b0:b1] = Ti @ rhs
        else:
            rhs = B[b0:b1] - L[b1:, b0:b1].conj().T @ X[b1:]
            X[b0:b1] = Ti.conj().T @ rhs
    return X


def trsm_merged_f64(L, X):
    """build_trsm_q + trsm_merged_batched in float64: Q[b, b] = L_bb^{-1}, Q[b, :b0] =
    -L_bb^{-1} L[b, :b0], then X[b] = Q[b, :b1] X[:b1] in place, block row by block row."""
    L = np.asarray(L)
    r = L.shape[0]
    X = np.array(X, np.complex128)
    for b0, m, b1 in merged_partition(r)[1]:
        Ti = _trinv_f64(L[b0:b1, b0:b1])
        Q = np.concatenate([-Ti @ L[b0:b1, :b0], Ti], axis=1)
        X[b0:b1] = Q @ X[:b1]
    return X


# ------------------------------------------------------------------ input generators
def _gauss(rng, n, k, real):
    g = rng.standard_normal((n, k))
    return g.astype(np.complex128) if real else g + 1j * rng.standard_normal((n, k))


def _herm(A):
    A = 0.5 * (A + A.conj().T)
    A[np.diag_indices(A.shape[0])] = A.diagonal().real
    return A


def low_rank(n, k, decay, seed, real=False):
    """Gaussian factor with a geometric column decay: exactly Hermitian, rank k up to rounding."""
    B = _gauss(np.random.default_rng(seed), n, k, real) * decay ** np.arange(k)
    return _herm(B @ B.conj().T)


def full_rank(n, seed, real=False):
    B = _gauss(np.random.default_rng(seed), n, n + 8, real)
    return _herm(B @ B.conj().T / n + np.eye(n))


def make_matrix(spec, n):
    kind = spec[0]
    if kind == "zero":
        return np.zeros((n, n), np.complex128)
    if kind == "low":
        _, k, decay, seed, real = spec
        return low_rank(n, k, decay, seed, real)
    if kind == "full":
        _, seed, real = spec
        return full_rank(n, seed, real)
    raise ValueError(spec)


def tri_lower(n, seed, real=False):
    """A well-conditioned lower-triangular matrix (diagonal in [1, 2))."""
    rng = np.random.default_rng(seed)
    T = np.tril(_gauss(rng, n, n, real)) * 0.3 / np.sqrt(n)
    T[np.diag_indices(n)] = 1.0 + rng.random(n)
    return T


# ------------------------------------------------------------------ a. pchol
# mats: ("zero",), ("low", k, decay, seed, real), ("full", seed, real).  tol_abs_rel: tol_abs as
# a multiple of the batch's largest diagonal entry (0: none).
PcholCase = namedtuple("PcholCase", "name n rmax tol_rel tol_abs_rel mats solo")
PCHOL_CASES = [
    PcholCase("n1", 1, 1, 1e-12, 0.0, (("full", 1, False),), ()),
    PcholCase("n33_full_toln", 33, 33, -1.0, 0.0, (("full", 2, False), ("full", 3, True)), (1,)),
    PcholCase("n33_rmax31", 33, 31, 1e-11, 0.0,
              (("full", 4, False), ("low", 20, 0.7, 5, True)), ()),
    PcholCase("n33_rmax32", 33, 32, 0.0, 0.0, (("full", 6, True), ("full", 7, False)), ()),
    PcholCase("n97_full_toln", 97, 97, -1.0, 0.0, (("full", 8, False),), ()),
    PcholCase("n97_rmax33", 97, 33, 1e-11, 0.0,
              (("full", 9, False), ("low", 33, 0.8, 10, False), ("low", 32, 0.8, 11, False),
               ("low", 31, 0.8, 12, True)), (2,)),
    PcholCase("n130_mixed_rmax33", 130, 33, 1e-11, 0.0,
              (("zero",), ("low", 1, 1.0, 13, False), ("low", 20, 0.7, 14, False),
               ("full", 15, False)), (2, 3)),
    PcholCase("n130_mixed_rmaxn", 130, 130, 1e-11, 0.0,
              (("zero",), ("low", 1, 1.0, 16, True), ("low", 70, 0.9, 17, False),
               ("full", 18, True)), (2, 3)),
    PcholCase("n130_tol_abs", 130, 130, 1e-13, 1e-9,
              (("low", 40, 0.85, 19, False), ("low", 25, 0.8, 20, True)), ()),
    PcholCase("n1024_rmax64", 1024, 64, 1e-11, 0.0,
              (("low", 33, 0.8, 21, False), ("low", 40, 0.8, 22, True)), (0,)),
    PcholCase("n1025_step_rmax48", 1025, 48, 1e-11, 0.0,
              (("low", 40, 0.8, 23, False), ("low", 40, 0.8, 24, True)), (1,)),
    PcholCase("n1025_step_rmax31", 1025, 31, 1e-11, 0.0,
              (("low", 40, 0.8, 23, False), ("zero",), ("low", 1, 1.0, 25, True)), ()),
]
PCHOL_BY_NAME = {c.name: c for c in PCHOL_CASES}


def pchol_lda(c):
    return c.n + 3


def pchol_stride(c):
    return c.n * pchol_lda(c) + 5


PcholData = namedtuple("PcholData", "A tol_abs ref f64 L_bound")


@functools.lru_cache(maxsize=None)
def pchol_data(name):
    """Inputs (batch, n, n), tol_abs, the long-double factorisations, the float64 restatement's
    and the bound on the device's factor error per matrix."""
    c = PCHOL_BY_NAME[name]
    A = np.stack([make_matrix(s, c.n) for s in c.mats])
    tol_abs = c.tol_abs_rel * float(max(a.diagonal().real.max() for a in A))
    nb = PCHOL_NB if pchol_path(c.n) == BLOCKED else None
    ref = [pchol_ld(a, c.rmax, c.tol_rel, tol_abs) for a in A]
    f64 = [greedy_f64(a, c.rmax, c.tol_rel, tol_abs, nb) for a in A]
    bnd = [bound(relerr(g.L, r.L) if g.rank == r.rank else np.inf, c.n) for g, r in zip(f64, ref)]
    return PcholData(A, tol_abs, ref, f64, bnd)


# ------------------------------------------------------------------ b. chol_unpivoted failure
CHOL_FAIL_N, CHOL_FAIL_TOL, CHOL_FAIL_AT = 100, 1e-10, 70


@functools.lru_cache(maxsize=None)
def chol_fail_batch():
    """Three Hermitian matrices of size 100; the middle one has row/column 70 equal to row/column
    69, so it is exactly singular and its pivot 70 (in the second 64-block) is rounding only."""
    A = np.stack([full_rank(CHOL_FAIL_N, 30 + b) for b in range(3)])
    k = CHOL_FAIL_AT
    A[1][k, :] = A[1][k - 1, :]
    A[1][:, k] = A[1][:, k - 1]
    A[1][k, k] = A[1][k - 1, k - 1]
    return A


# ------------------------------------------------------------------ c. gather / scatter
GATHER_N = 130
GATHER_RANKS = (0, 1, 40, 130)


# ------------------------------------------------------------------ d. merged operator
MERGED_N = (1, 63, 64, 65, 100, 129, 191, 256, 257, 292, 320)   # 100, 292: s0 = 36
MERGED_RHS = ("identity", 1, 70, 520)     # lower_rhs with the identity, or a general ncol
MERGED_BATCH = 3
MergedData = namedtuple("MergedData", "L X ref bound lower_rhs ncol")


@functools.lru_cache(maxsize=None)
def merged_data(n, rhs):
    Ls = np.stack([tri_lower(n, 1000 + 10 * n + b) for b in range(MERGED_BATCH)])
    if rhs == "identity":
        ncol, lower = n, True
        X = np.stack([np.eye(n, dtype=np.complex128)] * MERGED_BATCH)
    else:
        ncol, lower = int(rhs), False
        X = np.stack([_gauss(np.random.default_rng(2000 + 10 * n + b), n, ncol, False)
                      for b in range(MERGED_BATCH)])
    ref = [solve_lower_ld(l, x) for l, x in zip(Ls, X)]
    bnd = [bound(relerr(trsm_merged_f64(l, x), r), n) for l, x, r in zip(Ls, X, ref)]
    return MergedData(Ls, X, ref, bnd, lower, ncol)


# ------------------------------------------------------------------ e. trsm_blocked
TRSM_NIP = 200
TRSM_R = (1, 40, 64, 65, 130, 200)
TRSM_NCOL_FIT = (1, 45, 600)
TrsmData = namedtuple("TrsmData", "Lfac piv L B ref bound")


@functools.lru_cache(maxsize=None)
def trsm_data(r, lower, a_real, form):
    """form "fit": one matrix, a right-hand side per ncol of TRSM_NCOL_FIT; "wpp": three matrices,
    ncol = TRSM_NIP.  Lfac: the factor as pchol leaves it (rows in a shuffled order piv), L its
    leading r x r in pivot order."""
    batch = 1 if form == "fit" else 3
    ncols = TRSM_NCOL_FIT if form == "fit" else (TRSM_NIP,)
    seed = 3000 + 16 * r + 4 * lower + 2 * a_real + (form == "wpp")
    rng = np.random.default_rng(seed)
    Lfac = np.zeros((batch, TRSM_NIP, TRSM_NIP), np.complex128)
    piv = np.stack([rng.permutation(TRSM_NIP) for _ in range(batch)]).astype(np.int32)
    L = np.stack([tri_lower(r, seed + 100 + b, bool(a_real)) for b in range(batch)])
    for b in range(batch):
        Lfac[b][piv[b][:r], :r] = L[b]
    B = {nc: np.stack([_gauss(rng, r, nc, False) for _ in range(batch)]) for nc in ncols}
    solve = solve_lower_ld if lower else solve_adjoint_ld
    ref = {nc: [solve(L[b], B[nc][b]) for b in range(batch)] for nc in ncols}
    bnd = {nc: [bound(relerr(trsm_blocked_f64(L[b], B[nc][b], lower), ref[nc][b]), r)
                for b in range(batch)] for nc in ncols}
    return TrsmData(Lfac, piv, L, B, ref, bnd)


# ------------------------------------------------------------------ f. chain
CHAIN_N, CHAIN_NCOL, CHAIN_TOL = 130, 90, 1e-6
CHAIN_MATS = (("full", 40, False), ("low", 70, 0.943, 41, False), ("low", 40, 0.902, 42, False))
ChainData = namedtuple("ChainData", "A Y ref W bound")


def _chain_w(L, Y, solve_lo, solve_ad, wide):
    U = solve_lo(L, Y)
    G = U @ U.conj().T
    T = solve_ad(L, G).conj().T
    return solve_ad(L, T).conj().T.astype(wide)


@functools.lru_cache(maxsize=None)
def chain_data():
    """W = P (A_rr)^{-1} Y_r Y_r^H (A_rr)^{-1} P^T per matrix, r = the pivoted Cholesky's rank, in
    long double; the bound from the same chain in float64 along the same pivots."""
    n = CHAIN_N
    A = np.stack([make_matrix(s, n) for s in CHAIN_MATS])
    Y = np.stack([_gauss(np.random.default_rng(50 + b), n, CHAIN_NCOL, False) for b in range(3)])
    ref = [pchol_ld(a, n, CHAIN_TOL) for a in A]
    W, bnd = [], []
    for b in range(3):
        p, r = ref[b].piv, ref[b].rank
        Lr = ref[b].L[p]                                   # r x r, pivot order
        S = _chain_w(Lr, Y[b][p], solve_lower_ld, solve_adjoint_ld, CLD)
        w = np.zeros((n, n), CLD)
        w[np.ix_(p, p)] = S
        g = greedy_f64(A[b], n, CHAIN_TOL, 0.0, PCHOL_NB)
        assert np.array_equal(g.piv, p)
        S64 = _chain_w(g.L[p], Y[b][p], lambda l, x: trsm_blocked_f64(l, x, 1),
                       lambda l, x: trsm_blocked_f64(l, x, 0), np.complex128)
        W.append(w)
        bnd.append(bound(relerr(S64, S), n))
    return ChainData(A, Y, ref, W, bnd)


# ------------------------------------------------------------------ g. min-norm past 1024
MIN_NORM_N, MIN_NORM_RANK, MIN_NORM_TOL = 1025, 40, 1e-12


# ------------------------------------------------------------------ h. selection panel variants
# B has 10 columns, so x4 = (B B^T)^2 has rank 55: the trailing updates move the residual diagonal
# by a large part of itself and a panel that missed one picks other pivots (with 64 columns the
# Gram is so close to diagonal that the first 20 pivots survive a dropped update)
SelCase = namedtuple("SelCase", "name n k nip_max tol seed")
SEL_NK = 2
SEL_CASES = [
    SelCase("sel600", 600, 10, 40, -1.0, 60),
    SelCase("sel1030", 1030, 10, 40, -1.0, 61),
    SelCase("sel2049", 2049, 10, 30, -1.0, 62),
    SelCase("sel3585", 3585, 10, 20, -1.0, 63),
    SelCase("sel600_rank10", 600, 4, 40, 1e-10, 64),
]
SEL_BY_NAME = {c.name: c for c in SEL_CASES}


def sel_input(name):
    """x2 = Re(B B^T) + i garbage (the selection must ignore the imaginary part); the real part
    exactly symmetric."""
    c = SEL_BY_NAME[name]
    rng = np.random.default_rng(c.seed)
    B = rng.standard_normal((c.n, c.k))
    g = np.tril(B @ B.T)
    g = g + np.tril(g, -1).T
    return g + 1j * rng.standard_normal((c.n, c.n))


def sel_reference(name, x2=None):
    """The long-double greedy sequence of x4 = Re(x2)^2 / nk, columns formed on demand."""
    c = SEL_BY_NAME[name]
    re = (sel_input(name) if x2 is None else x2).real
    sc = LD(1) / LD(SEL_NK)
    col = lambda p: re[:, p].astype(LD) ** 2 * sc
    return greedy_ld(col, re.diagonal().astype(LD) ** 2 * sc, c.nip_max, c.tol, 0.0, real=True)


def sel_f64(name, x2=None, skip_updates=False):
    c = SEL_BY_NAME[name]
    re = (sel_input(name) if x2 is None else x2).real
    x4 = re * re * (1.0 / SEL_NK)
    return greedy_f64(x4, c.nip_max, c.tol, 0.0, sel_variant(c.n)[1], skip_updates)
