"""The factor-and-solve chain between x4_q and W_q on the GPU against the long-double references of
tests/factor_cases.py: pivoted Cholesky on both paths, the unpivoted Cholesky's failure flag, the
pivot-order gather / scatter, the merged and the blocked triangular operators, the whole chain, the
minimum-norm operator past 1024 rows and the four real selection panel kernels.

Inputs live in padded buffers with NaN in the padding, outputs inside sentinel-filled buffers whose
padding and guard regions are checked afterwards.  Every forward-error bound is the float64 host
restatement's own error against long double times 16, floored at n eps (factor_cases.bound); each
comparison prints the device's error next to it."""
import ctypes as C

import numpy as np
import pytest

import factor_cases as F

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = complex(-7.25e77, 3.5e66)
ISENT = -777


@pytest.fixture(scope="module")
def env():
    import torch
    from fisdf import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ctx = _lib.Context(0, torch.cuda.current_stream().cuda_stream)
    return torch, _lib, ctx


class Buf:
    """A device buffer of `count` elements between two guard regions, all filled with `fill`."""

    def __init__(self, torch, count, fill, dtype=None):
        self.dtype = dtype or torch.complex128
        self.fill, self.count = fill, count
        self.flat = torch.full((count + 2 * GUARD,), fill, dtype=self.dtype, device="cuda")
        self.ptr = C.c_void_p(self.flat.data_ptr() + GUARD * self.flat.element_size())

    def put(self, host):
        import torch
        host = np.ascontiguousarray(host).reshape(-1)
        assert host.size == self.count
        self.flat[GUARD:GUARD + self.count] = torch.from_numpy(host).cuda()
        return self

    def get(self):
        return self.flat[GUARD:GUARD + self.count].cpu().numpy()

    def guards_intact(self):
        g = np.concatenate([self.flat[:GUARD].cpu().numpy(), self.flat[GUARD + self.count:].cpu().numpy()])
        return bool((np.isnan(g) if self.fill != self.fill else g == self.fill).all())


def pack(mats, ld, stride, fill=np.nan):
    """(batch, rows, cols) -> flat (batch * stride) with row stride ld and `fill` in the padding."""
    mats = np.asarray(mats)
    batch, rows, cols = mats.shape
    assert ld >= cols and stride >= rows * ld
    flat = np.full(batch * stride, fill, mats.dtype)
    for b in range(batch):
        flat[b * stride:b * stride + rows * ld].reshape(rows, ld)[:, :cols] = mats[b]
    return flat


def unpack(flat, batch, rows, cols, ld, stride, fill):
    """The (batch, rows, cols) views of a packed buffer and whether its padding still holds fill."""
    out = np.empty((batch, rows, cols), flat.dtype)
    mask = np.ones(flat.size, bool)
    for b in range(batch):
        v = flat[b * stride:b * stride + rows * ld].reshape(rows, ld)
        out[b] = v[:, :cols]
        mask[b * stride:b * stride + rows * ld].reshape(rows, ld)[:, :cols] = False
    pad = flat[mask]
    ok = np.isnan(pad).all() if isinstance(fill, float) and np.isnan(fill) else (pad == fill).all()
    return out, bool(ok)


# ------------------------------------------------------------------ a. pchol
def run_pchol(env, A, c, tol_abs):
    torch, L, ctx = env
    batch, n = A.shape[0], c.n
    lda, sA = F.pchol_lda(c), F.pchol_stride(c)
    dA = Buf(torch, batch * sA, complex(np.nan, np.nan)).put(pack(A, lda, sA, complex(np.nan, np.nan)))
    dL = Buf(torch, batch * n * c.rmax, SENT)
    dP = Buf(torch, batch * c.rmax, ISENT, torch.int32)
    dR = Buf(torch, batch, ISENT, torch.int32)
    path = C.c_int(-9)
    ctx.call("fisdf_pivoted_cholesky_ex", dA.ptr, lda, sA, n, batch, c.rmax, c.tol_rel, tol_abs,
             dL.ptr, dP.ptr, dR.ptr, C.byref(path))
    assert dL.guards_intact() and dP.guards_intact() and dR.guards_intact() and dA.guards_intact()
    back, pad_ok = unpack(dA.get(), batch, n, n, lda, sA, np.nan)
    assert pad_ok and np.array_equal(back, A)            # the input is left alone
    return (dP.get().reshape(batch, c.rmax), dR.get(), dL.get().reshape(batch, n, c.rmax),
            path.value)


@pytest.mark.parametrize("name", [c.name for c in F.PCHOL_CASES])
def test_pchol_both_paths(env, name):
    c, d = F.PCHOL_BY_NAME[name], F.pchol_data(name)
    piv, rank, Lf, path = run_pchol(env, d.A, c, d.tol_abs)
    assert path == F.pchol_path(c.n)
    for b, ref in enumerate(d.ref):
        r = int(rank[b])
        assert r == ref.rank, (b, r, ref.rank)
        assert np.array_equal(piv[b, :r], ref.piv), (b, piv[b, :r], ref.piv)
        assert (piv[b, r:] == ISENT).all()               # complete_perm_kernel relies on this
        Lb = Lf[b][:, :r]
        Lp = Lb[piv[b, :r]]
        assert (np.triu(Lp, 1) == 0).all()               # exactly lower trapezoidal in pivot order
        assert (Lp.diagonal().imag == 0).all() and (Lp.diagonal().real > 0).all()
        err = F.relerr(Lb, ref.L)
        res = abs(d.A[b] - Lb @ Lb.conj().T).max()
        res_bound = ref.resid_after + 1e-13 * ref.dmax
        print(f"{name}[{b}] path {path} rank {r}: |L - L_ld| / |L| {err:.2e} (bound "
              f"{d.L_bound[b]:.2e}), max |A - L L^H| {res:.2e} (bound {res_bound:.2e})")
        assert err <= d.L_bound[b]
        assert res <= res_bound
        if c.mats[b][-1] is True:                         # real input: Im L exactly zero
            assert abs(d.A[b].imag).max() == 0 and (Lb.imag == 0).all()
    for s in c.solo:                                      # alone == inside the batch, bit for bit
        p1, r1, L1, _ = run_pchol(env, d.A[s:s + 1], c, d.tol_abs)
        r = int(rank[s])
        assert int(r1[0]) == r and np.array_equal(p1[0], piv[s])
        assert np.array_equal(L1[0][:, :r], Lf[s][:, :r])


# ------------------------------------------------------------------ b. chol_unpivoted failure
def test_cholesky_flags_the_singular_matrix_only(env):
    torch, L, ctx = env
    A = F.chol_fail_batch()
    n = F.CHOL_FAIL_N

    def run(mats):
        dA = Buf(torch, mats.size, SENT).put(mats)
        fail = np.full(len(mats), ISENT, np.int32)
        ctx.call("fisdf_cholesky", dA.ptr, n, len(mats), F.CHOL_FAIL_TOL, fail.ctypes.data_as(L._ip))
        assert dA.guards_intact()
        return fail, dA.get().reshape(len(mats), n, n)

    fail, out = run(A)
    assert fail.tolist() == [0, 1, 0]
    for b in (0, 2):
        f1, o1 = run(A[b:b + 1])
        assert f1.tolist() == [0] and np.array_equal(np.tril(o1[0]), np.tril(out[b]))
        Lb = np.tril(out[b])
        res = abs(Lb @ Lb.conj().T - A[b]).max() / abs(A[b]).max()
        print(f"cholesky beside a failing matrix, b={b}: rel |L L^H - A| {res:.1e} (bound 1e-13)")
        assert res < 1e-13


# ------------------------------------------------------------------ c. gather / scatter / adjoint
def test_gather_scatter_conj_transpose_are_exact(env):
    torch, L, ctx = env
    n, ranks = F.GATHER_N, F.GATHER_RANKS
    batch = len(ranks)
    rng = np.random.default_rng(70)
    Lf = rng.standard_normal((batch, n, n)) + 1j * rng.standard_normal((batch, n, n))
    piv = np.stack([rng.permutation(n) for _ in range(batch)]).astype(np.int32)
    for b, r in enumerate(ranks):
        Lf[b][:, r:] = np.nan                             # columns >= rank are unspecified
        piv[b, r:] = 1 << 30                              # and so are the pivots beyond it
    dL, dP = Buf(torch, Lf.size, SENT).put(Lf), Buf(torch, piv.size, ISENT, torch.int32).put(piv)
    dR = Buf(torch, batch, ISENT, torch.int32).put(np.array(ranks, np.int32))
    dLp = Buf(torch, batch * n * n, SENT)
    ctx.call("fisdf_gather_lp", dL.ptr, n, n, dP.ptr, dR.ptr, n, dLp.ptr, batch)
    want = np.zeros((batch, n, n), complex)
    for b, r in enumerate(ranks):
        want[b] = np.eye(n)
        want[b][:r, :r] = np.tril(Lf[b][piv[b, :r], :r])
    assert dLp.guards_intact() and np.array_equal(dLp.get().reshape(batch, n, n), want)
    # scatter_w: Wpp rows at ldw, batch stride sW, NaN outside the rank block
    ldw, sW = n + 3, n * (n + 3) + 5
    Wpp = rng.standard_normal((batch, n, n)) + 1j * rng.standard_normal((batch, n, n))
    for b, r in enumerate(ranks):
        Wpp[b][r:, :] = np.nan
        Wpp[b][:, r:] = np.nan
    dWpp = Buf(torch, batch * sW, SENT).put(pack(Wpp, ldw, sW, complex(np.nan, np.nan)))
    dW = Buf(torch, batch * n * n, SENT)
    ctx.call("fisdf_scatter_w", dWpp.ptr, ldw, sW, n, dP.ptr, dR.ptr, dW.ptr, n, batch)
    want = np.zeros((batch, n, n), complex)
    for b, r in enumerate(ranks):
        p = piv[b, :r]
        want[b][np.ix_(p, p)] = Wpp[b][:r, :r]
    assert dW.guards_intact() and np.array_equal(dW.get().reshape(batch, n, n), want)
    # conj_transpose with a padded batch stride
    m, sA = 37, 37 * 37 + 11
    Am = rng.standard_normal((3, m, m)) + 1j * rng.standard_normal((3, m, m))
    dA = Buf(torch, 3 * sA, SENT).put(pack(Am, m, sA, complex(np.nan, np.nan)))
    dB = Buf(torch, 3 * sA, SENT)
    ctx.call("fisdf_conj_transpose", dA.ptr, m, sA, dB.ptr, 3)
    got, pad_ok = unpack(dB.get(), 3, m, m, m, sA, SENT)
    assert dB.guards_intact() and pad_ok and np.array_equal(got, Am.conj().transpose(0, 2, 1))


# ------------------------------------------------------------------ d. merged operator
def run_merged(env, d, n, batch, use_work, work_elems):
    """Returns (rc, X (batch, n, ncol), rows) and checks guards and padding."""
    torch, L, ctx = env
    ld, sL = d.ncol + 3, n * n + 5
    sX = n * ld + 7
    nan = complex(np.nan, np.nan)
    dLp = Buf(torch, batch * sL, nan).put(pack(d.L[:batch], n, sL, nan))
    x0 = pack(d.X[:batch], ld, sX, nan)
    dX = Buf(torch, batch * sX, SENT).put(x0)
    nblk = (n + 63) // 64
    rows = np.full((nblk, 6), ISENT, np.int32)
    rc = ctx.lib.fisdf_trsm_merged_ex(ctx.h, dLp.ptr, sL, n, dX.ptr, ld, sX, d.ncol, batch,
                                      int(d.lower_rhs), int(use_work), work_elems,
                                      rows.ctypes.data_as(L._ip), nblk)
    assert dX.guards_intact() and dLp.guards_intact()
    flat = dX.get()
    X, pad_ok = unpack(flat, batch, n, d.ncol, ld, sX, np.nan)
    assert pad_ok
    if rc != 0:
        assert np.array_equal(flat.view(np.int64), x0.view(np.int64))   # X untouched, bit for bit
    return rc, X, [tuple(int(v) for v in r) for r in rows]


@pytest.mark.parametrize("rhs", F.MERGED_RHS)
@pytest.mark.parametrize("n", F.MERGED_N)
def test_merged_operator(env, n, rhs):
    d = F.merged_data(n, rhs)
    B = F.MERGED_BATCH
    per = F.merged_partials(n, d.ncol, d.lower_rhs)
    rc, X_none, rows = run_merged(env, d, n, B, False, 0)
    assert rc == 0 and rows == F.merged_rows(n, d.ncol, B, d.lower_rhs, None)
    rc, X_full, rows = run_merged(env, d, n, B, True, max(1, B * per))
    assert rc == 0 and rows == F.merged_rows(n, d.ncol, B, d.lower_rhs, max(1, B * per))
    for what, X in (("no workspace", X_none), ("workspace", X_full)):
        for b in range(B):
            err = F.relerr(X[b], d.ref[b])
            print(f"merged n={n} rhs={rhs} {what} b={b}: err {err:.2e} (bound {d.bound[b]:.2e})")
            assert err <= d.bound[b]
    for b in range(B):                      # split-K changes the summation order only
        assert F.relerr(X_full[b], X_none[b]) <= 2 * d.bound[b]
    if d.lower_rhs:                         # the identity stays lower triangular, exactly
        assert (np.triu(X_full, 1) == 0).all() and (np.triu(X_none, 1) == 0).all()
    # one matrix alone (batch 1) equals the same matrix inside the batch, bit for bit
    for use, Xb in ((False, X_none), (True, X_full)):
        rc, X1, rows = run_merged(env, d, n, 1, use, max(1, per))
        assert rc == 0 and np.array_equal(X1[0], Xb[0])
        assert rows == F.merged_rows(n, d.ncol, 1, d.lower_rhs, max(1, per) if use else None)
    if per:
        # a workspace of exactly one matrix's partials: sub-batches, the same bits
        rc, X_cap, rows = run_merged(env, d, n, B, True, per)
        want = F.merged_rows(n, d.ncol, B, d.lower_rhs, per)
        assert rc == 0 and rows == want and min(r[5] for r in want) == 1
        assert np.array_equal(X_cap, X_full)
        # one element less: an error before anything is launched on X
        rc, X_err, rows = run_merged(env, d, n, B, True, per - 1)
        assert rc != 0 and np.array_equal(X_err, d.X)
        assert min(r[5] for r in rows) == 0
        torch, L, ctx = env
        assert b"workspace too small" in ctx.lib.fisdf_last_error(ctx.h)


# ------------------------------------------------------------------ e. trsm_blocked
def gather_on_device(env, Lfac, piv, ranks, rpad):
    torch, L, ctx = env
    batch, n = Lfac.shape[:2]
    dL = Buf(torch, Lfac.size, SENT).put(Lfac)
    dP = Buf(torch, piv.size, ISENT, torch.int32).put(piv)
    dR = Buf(torch, batch, ISENT, torch.int32).put(np.asarray(ranks, np.int32))
    dLp = Buf(torch, batch * rpad * rpad, SENT)
    ctx.call("fisdf_gather_lp", dL.ptr, n, Lfac.shape[2], dP.ptr, dR.ptr, rpad, dLp.ptr, batch)
    assert dLp.guards_intact()
    return dLp


def run_trsm_blocked(env, dLp, ldl, sL, r, rows_x, Bm, lower, a_real):
    """B (batch, r, ncol) -> X: (batch, rows_x, ncol) view of the sentinel-filled output."""
    torch, L, ctx = env
    batch, _, ncol = Bm.shape
    ldb, ldx = ncol + 3, ncol + 5
    sB, sX = rows_x * ldb, rows_x * ldx + 9
    nan = complex(np.nan, np.nan)
    Bfull = np.full((batch, rows_x, ncol), nan)
    Bfull[:, :r] = Bm
    dB = Buf(torch, batch * sB, nan).put(pack(Bfull, ldb, sB, nan))
    dX = Buf(torch, batch * sX, SENT)
    ctx.call("fisdf_trsm_blocked_ex", lower, dLp.ptr, ldl, sL, r, dB.ptr, ldb, sB, dX.ptr, ldx, sX,
             ncol, batch, a_real)
    assert dX.guards_intact() and dB.guards_intact() and dLp.guards_intact()
    X, pad_ok = unpack(dX.get(), batch, rows_x, ncol, ldx, sX, SENT)
    assert pad_ok
    return X


@pytest.mark.parametrize("form", ["fit", "wpp"])
@pytest.mark.parametrize("a_real", [0, 1])
@pytest.mark.parametrize("lower", [1, 0])
@pytest.mark.parametrize("r", F.TRSM_R)
def test_trsm_blocked(env, r, lower, a_real, form):
    d = F.trsm_data(r, lower, a_real, form)
    nip = F.TRSM_NIP
    batch = d.L.shape[0]
    dLp = gather_on_device(env, d.Lfac, d.piv, [r] * batch, nip)
    Lp = dLp.get().reshape(batch, nip, nip)
    assert np.array_equal(Lp[:, :r, :r], d.L)            # the gather is exact (r < ldl)
    if a_real:
        assert (Lp.imag == 0).all()
    for ncol, Bm in d.B.items():
        X = run_trsm_blocked(env, dLp, nip, nip * nip, r, nip, Bm, lower, a_real)
        assert (X[:, r:] == SENT).all()                   # rows >= r are not written
        for b in range(batch):
            err = F.relerr(X[b, :r], d.ref[ncol][b])
            print(f"trsm_blocked r={r} lower={lower} a_real={a_real} {form} ncol={ncol} b={b}: "
                  f"err {err:.2e} (bound {d.bound[ncol][b]:.2e})")
            assert err <= d.bound[ncol][b]


# ------------------------------------------------------------------ f. chain
def test_chain_x4_to_w(env):
    torch, L, ctx = env
    d = F.chain_data()
    n, m = F.CHAIN_N, F.CHAIN_NCOL
    c = F.PcholCase("chain", n, n, F.CHAIN_TOL, 0.0, F.CHAIN_MATS, ())
    piv, rank, Lf, path = run_pchol(env, d.A, c, 0.0)
    for b in range(3):
        assert int(rank[b]) == d.ref[b].rank and np.array_equal(piv[b, :rank[b]], d.ref[b].piv)
    dLp = gather_on_device(env, Lf, piv, rank, n)
    Yp = np.zeros((3, n, m), complex)                     # Y in pivot order, zero beyond the rank
    for b in range(3):
        Yp[b, :rank[b]] = d.Y[b][piv[b, :rank[b]]]
    U = run_trsm_blocked(env, dLp, n, n * n, n, n, Yp, 1, 0)
    G = U @ U.conj().transpose(0, 2, 1)

    def adjoint(T):
        dA, dB = Buf(torch, T.size, SENT).put(T), Buf(torch, T.size, SENT)
        ctx.call("fisdf_conj_transpose", dA.ptr, n, n * n, dB.ptr, 3)
        return dB.get().reshape(3, n, n)

    T = adjoint(run_trsm_blocked(env, dLp, n, n * n, n, n, G, 0, 0))
    S = adjoint(run_trsm_blocked(env, dLp, n, n * n, n, n, T, 0, 0))
    dS = Buf(torch, S.size, SENT).put(S)
    dP = Buf(torch, piv.size, ISENT, torch.int32).put(piv)
    dR = Buf(torch, 3, ISENT, torch.int32).put(rank)
    dW = Buf(torch, 3 * n * n, SENT)
    ctx.call("fisdf_scatter_w", dS.ptr, n, n * n, n, dP.ptr, dR.ptr, dW.ptr, n, 3)
    assert dW.guards_intact()
    W = dW.get().reshape(3, n, n)
    for b in range(3):
        p = piv[b, :rank[b]]
        out = np.ones((n, n), bool)
        out[np.ix_(p, p)] = False
        assert (W[b][out] == 0).all()                     # zero outside the pivot block
        err = F.relerr(W[b], d.W[b])
        print(f"chain n={n} rank {rank[b]}: |W - W_ld| / |W| {err:.2e} (bound {d.bound[b]:.2e})")
        assert err <= d.bound[b]


# ------------------------------------------------------------------ g. min-norm past 1024
@pytest.mark.parametrize("real", [False, True])
def test_min_norm_operator_past_1024(env, real):
    """test_gpu_kernels.test_min_norm_operator's assertions at n = 1025, where the factor comes
    from the per-step pchol path."""
    torch, L, ctx = env
    rng = np.random.default_rng(81)
    n, rk = F.MIN_NORM_N, F.MIN_NORM_RANK
    B = rng.standard_normal((n, rk)) + (0 if real else 1j * rng.standard_normal((n, rk)))
    B = B.astype(np.complex128) * np.exp(-0.25 * np.arange(rk))
    A = B @ B.conj().T
    A = 0.5 * (A + A.conj().T)
    dA = torch.from_numpy(A).cuda()
    dM, dQ, dR = (torch.zeros(n, n, dtype=torch.complex128, device="cuda") for _ in range(3))
    piv = np.zeros(n, np.int32)
    rnk = np.zeros(1, np.int32)
    ctx.call("fisdf_min_norm_operator", L.ptr(dA), n, F.MIN_NORM_TOL, L.ptr(dM), L.ptr(dQ),
             L.ptr(dR), piv.ctypes.data_as(L._ip), rnk.ctypes.data_as(L._ip))
    r = int(rnk[0])
    assert r == F.pchol_ld(A, n, F.MIN_NORM_TOL).rank == rk
    assert 0 < r < n and sorted(piv) == list(range(n))
    M = dM.cpu().numpy()[:r]
    Q = dQ.cpu().numpy().reshape(-1)[:n * r].reshape(n, r)
    Ri = dR.cpu().numpy().reshape(-1)[:r * r].reshape(r, r)
    Ap = A[np.ix_(piv, piv)]
    L11 = np.linalg.cholesky(Ap[:r, :r])
    Af = np.concatenate([L11, np.linalg.solve(L11, Ap[:r, r:]).conj().T])
    X = Q @ np.linalg.inv(Ri)                          # the device's P L
    qerr = abs(Q.conj().T @ Q - np.eye(r)).max()
    aerr = abs(X - Af).max() / abs(Af).max()
    merr = abs(M - Ri @ Q.conj().T).max() / abs(M).max()
    v = rng.standard_normal(n) + (0 if real else 1j * rng.standard_normal(n))
    b = A @ v
    z = np.zeros(n, complex)
    z[piv] = M.conj().T @ (M @ b[piv])
    res = np.linalg.norm(A @ z - b) / np.linalg.norm(b)
    print(f"min-norm operator n={n} rank {r} real={real}: |Q^H Q - I| {qerr:.1e} (bound 1e-12), "
          f"rel |QR - PL| {aerr:.1e} (1e-6), |M - R^-1 Q^H| {merr:.1e} (1e-12), residual {res:.1e} "
          f"(1e-6), |z|/|v| {np.linalg.norm(z) / np.linalg.norm(v):.3f}")
    assert qerr < 1e-12 and aerr < 1e-6 and merr < 1e-12
    assert res < 1e-6 and np.linalg.norm(z) <= np.linalg.norm(v)
    if real:
        assert abs(M.imag).max() == 0.0


# ------------------------------------------------------------------ h. selection panel variants
@pytest.mark.parametrize("name", [c.name for c in F.SEL_CASES])
def test_selection_panel_variants(env, name, monkeypatch):
    torch, L, ctx = env
    monkeypatch.setenv("FISDF_SEL_MODE", "blocked")
    c = F.SEL_BY_NAME[name]
    x2 = F.sel_input(name)
    ref = F.sel_reference(name, x2)
    dx2 = torch.from_numpy(x2).cuda()
    perm = np.full(c.nip_max, ISENT, np.int32)
    npiv, full = C.c_int(-1), C.c_int(-1)
    ctx.call("fisdf_select_pivots", L.ptr(dx2), F.SEL_NK, c.n, c.nip_max, c.tol,
             perm.ctypes.data_as(L._ip), C.byref(npiv), C.byref(full))
    same = int((perm[:ref.rank] == ref.piv).sum())
    print(f"{name}: panel {F.sel_variant(c.n)} npiv {npiv.value} (reference {ref.rank}), identical "
          f"pivots {same}/{ref.rank}, min gap {ref.min_gap:.1e}")
    assert npiv.value == ref.rank
    assert np.array_equal(perm[:ref.rank], ref.piv)
    assert full.value == (1 if ref.rank < c.nip_max else 0)
