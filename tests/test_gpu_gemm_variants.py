"""Every dispatch path of zgemm() / herk() (csrc/zgemm.hip, csrc/zgemm_wide.hip) against an fp64
NumPy reference: the 16 op pairs in the 2-deep ring, the plain ring-3 loop and the pipelined
3-multiplication loop, split-K (with batch, beta and other op pairs than NN), the real and
triangular modes on the 64 x 64 kernel, the fused epilogues with their max |Im| monitors, the
HERK modes and the batched HERK, the wide kernel, and degenerate sizes.

Cases, references and conventions live in tests/gemm_cases.py (tests/test_gemm_cases.py checks on
the CPU that the tables reach every loop).  Every operand is a view: padded leading dimensions,
batch strides with a gap, NaN around A and B, the sentinel 7 + 7j around C, which must come back
bitwise unchanged; with beta = 0 the logical C starts as NaN and must come back finite.
Tolerance: the suite's own, max |out - ref| < 1e-12 max(K, 16) (test_gpu_kernels.py); the
squared / real / scaled epilogues max |out - ref| / max |ref| < 1e-12 (test_build_y_kmesh_paths).
"""
import ctypes as C

import numpy as np
import pytest

import gemm_cases as G

pytestmark = pytest.mark.gpu

NAN = complex(np.nan, np.nan)


@pytest.fixture(scope="module")
def env():
    import torch
    from fisdf import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ctx = _lib.Context(0, torch.cuda.current_stream().cuda_stream)
    ctx.max_imag()  # the product's monitors start from zero
    return torch, _lib, ctx


@pytest.fixture(scope="module")
def worst():
    """Largest error per group relative to its bound, printed when the module is done."""
    w = {}
    yield w
    for k in sorted(w):
        err, tol, name = w[k]
        print(f"\ngemm-variants {k}: largest error {err:.3e} (bound {tol:.3e}) at {name}")


def note(worst, group, err, tol, name):
    if group not in worst or err / tol > worst[group][0] / worst[group][1]:
        worst[group] = (err, tol, name)


def dev(torch, a):
    return torch.from_numpy(a).cuda()


def c2(z):
    z = complex(z)
    return (C.c_double * 2)(z.real, z.imag)


def launch(env, opA, opB, M, N, K, alpha, A, B, beta, C0, batch, ks=1, mode=0, epi=G.EPI_NONE,
           aux=None, entry="zgemm", repeat=1):
    """One GEMM on padded views.  A, B: logical (batch, rows, cols) as stored; C0: logical
    (batch, M, N) start of C (complex, or float64 for EPI_REAL).  Returns (rc, [flat C buffer per
    repeat], monitor, flat start of C)."""
    torch, L, ctx = env
    creal = epi == G.EPI_REAL
    abuf, av, sA = G.padded(batch, A.shape[1], A.shape[2], A.shape[2] + G.PAD_A, NAN)
    bbuf, bv, sB = G.padded(batch, B.shape[1], B.shape[2], B.shape[2] + G.PAD_B, NAN)
    av[...] = A
    bv[...] = B
    ldc = N + (3 if creal else G.PAD_C)
    cbuf, cv, sC = G.padded(batch, M, N, ldc, 7.0 if creal else G.SENTINEL,
                            dtype=np.float64 if creal else np.complex128)
    cv[...] = C0
    dA, dB = dev(torch, abuf), dev(torch, bbuf)
    dX, ldaux = None, 0
    if aux is not None:
        ldaux = N + 2
        xbuf, xv, _ = G.padded(1, M, N, ldaux, np.nan, dtype=np.float64)
        xv[...] = aux
        dX = dev(torch, xbuf)
    mon = C.c_double(-1.0)
    outs, rc = [], 0
    for _ in range(repeat):
        dC = dev(torch, cbuf)
        head = (ctx.h, opA, opB, M, N, K, c2(alpha), L.ptr(dA), A.shape[2] + G.PAD_A, sA,
                L.ptr(dB), B.shape[2] + G.PAD_B, sB, c2(beta), L.ptr(dC), ldc, sC, batch)
        if entry == "zgemm":
            assert mode == 0 and epi == G.EPI_NONE
            rc = ctx.lib.fisdf_zgemm(*head, ks)
        elif entry == "mode":
            assert ks == 1 and epi == G.EPI_NONE
            rc = ctx.lib.fisdf_zgemm_mode(*head, mode)
        else:
            rc = ctx.lib.fisdf_zgemm_ex(*head, ks, mode, epi, L.ptr(dX) if dX is not None else None,
                                        ldaux, C.byref(mon))
        ctx.call("fisdf_sync")
        outs.append(dC.cpu().numpy())
    return rc, outs, mon.value, cbuf


def start_c(c, rng):
    """(beta, logical C0) of a Gemm case: beta = 0 with a NaN C, or complex beta with a random C."""
    if c.beta:
        return G.BETA, G.rnd(rng, c.batch, c.M, c.N)
    return 0.0, np.full((c.batch, c.M, c.N), NAN)


def check_gemm(env, worst, group, c, entry, alpha=G.ALPHA, repeat=1):
    """Run a Gemm case and compare with the reference: logical part within the bound and finite,
    padding bitwise the sentinel, repeats bitwise equal."""
    rng = np.random.default_rng(abs(hash(tuple(c))) % (1 << 32))
    A, B, clean = G.make_operands(c, rng)
    beta, C0 = start_c(c, rng)
    rc, outs, _, _ = launch(env, c.opA, c.opB, c.M, c.N, c.K, alpha, A, B, beta, C0, c.batch, c.ks,
                            c.mode, entry=entry, repeat=repeat)
    torch, L, ctx = env
    assert rc == 0, ctx.lib.fisdf_last_error(ctx.h)
    ref = G.ref_gemm(clean, B, c.opA, c.opB, alpha, beta, C0, c.mode)
    ldc = c.N + G.PAD_C
    out = G.logical(outs[0], c.batch, c.M, c.N, ldc)
    assert np.isfinite(out.view(np.float64)).all(), "NaN / Inf in a stored result"
    err = abs(out - ref).max() if ref.size else 0.0
    print(f"{group} {G.gid(c)}: err {err:.3e} bound {G.tol_abs(c.K):.3e}")
    note(worst, group, err, G.tol_abs(c.K), G.gid(c))
    pad = G.padding_mask(c.batch, c.M, c.N, ldc)
    assert (outs[0][pad] == G.SENTINEL).all(), "the padding of C was written"
    assert err < G.tol_abs(c.K), err
    for o in outs[1:]:
        assert o.tobytes() == outs[0].tobytes(), "the same call twice differs bitwise"
    return out


# ---- 1. op matrix x loop variant ----------------------------------------------------------------
@pytest.mark.parametrize("c", G.GROUP_OPS, ids=G.gid)
def test_ops_by_loop(env, worst, c):
    """All 16 op pairs in the 2-deep ring (K = 20), the plain ring-3 loop (37) and the pipelined
    loop with 5, 6 and 7 K-steps (40, 48, 56): conjugation signs, the K-contiguous swizzle and the
    clamped-row addressing of each loop, batch 3, complex alpha and beta."""
    check_gemm(env, worst, "1-ops", c, "zgemm")


# ---- 2. split-K ---------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.GROUP_SPLITK, ids=G.gid)
def test_splitk(env, worst, c):
    """Split-K with batch 1 and 2, beta = 0 (NaN C) and complex, op pairs other than NN, splits of
    3, 2 and 1 K-steps in the pipelined loop; the reduction is deterministic: twice the same
    bits."""
    check_gemm(env, worst, "2-splitk", c, "ex", repeat=2)


# ---- 3. real and triangular modes on the 64 x 64 kernel ------------------------------------------
@pytest.mark.parametrize("c", G.GROUP_REAL, ids=G.gid)
def test_real_modes(env, worst, c):
    """A_REAL ignores an Im A of magnitude 1e3; RE_ONLY (real alpha, beta = 0) gives
    alpha Re(op(A) op(B)) with Im C exactly 0."""
    alpha = 0.6 if c.mode & G.RE_ONLY else G.ALPHA
    out = check_gemm(env, worst, "3-real", c, "mode", alpha=alpha)
    if c.mode & G.RE_ONLY:
        assert (out.imag == 0).all()


@pytest.mark.parametrize("c", G.GROUP_LOWER, ids=G.gid)
def test_lower_modes_small_n(env, worst, c):
    """A_LOWER (and with A_REAL) at N < 512, where the 64 x 64 kernel runs: garbage past each
    64-row tile's last row of A must never be read."""
    check_gemm(env, worst, "3-lower", c, "mode")


@pytest.mark.parametrize("c", G.GROUP_UPPER, ids=G.gid)
def test_upper_mode(env, worst, c):
    """A_UPPER for (C,N) and (C,C), with and without split-K: triu(A^H) op(B); garbage in the rows
    of A above each 64-column tile's first row must never be read."""
    check_gemm(env, worst, "3-upper", c, "ex", repeat=2 if c.ks > 1 else 1)


# ---- 4. dispatch acceptance -----------------------------------------------------------------------
@pytest.mark.parametrize("opA,opB,mode", G.GROUP_DISPATCH,
                         ids=["%s%s-m%d" % ("NTRC"[a], "NTRC"[b], m) for (a, b, m) in G.GROUP_DISPATCH])
def test_dispatch_accepts_or_fails(env, worst, opA, opB, mode):
    """Every (opA, opB, mode 0..9) either fails with a message and leaves C alone, or computes
    what the mode means: no call returns 0 without having launched a kernel."""
    torch, L, ctx = env
    c = G.Gemm(opA, opB, 16, 16, 16, 1, 1, mode, 0)
    rng = np.random.default_rng(1000 + mode * 16 + opA * 4 + opB)
    A, B, clean = G.make_operands(c, rng)
    alpha = 0.6 if mode & G.RE_ONLY else G.ALPHA
    C0 = np.full((1, 16, 16), NAN)
    rc, outs, _, before = launch(env, opA, opB, 16, 16, 16, alpha, A, B, 0.0, C0, 1, mode=mode,
                                 entry="mode")
    if rc != 0:
        assert len(ctx.lib.fisdf_last_error(ctx.h)) > 0
        assert outs[0].tobytes() == before.tobytes(), "a failed call wrote to C"
        assert not G.supported(opA, opB, mode), ctx.lib.fisdf_last_error(ctx.h)
        return
    assert G.supported(opA, opB, mode)
    out = G.logical(outs[0], 1, 16, 16, 16 + G.PAD_C)
    assert np.isfinite(out.view(np.float64)).all(), "returned 0 but left C unwritten"
    err = abs(out - G.ref_gemm(clean, B, opA, opB, alpha, mode=mode)).max()
    note(worst, "4-dispatch", err, G.tol_abs(16), "%d%d-m%d" % (opA, opB, mode))
    assert err < G.tol_abs(16), err
    assert (outs[0][G.padding_mask(1, 16, 16, 16 + G.PAD_C)] == G.SENTINEL).all()


# ---- 5. epilogues ---------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.GROUP_EPI, ids=G.eid)
def test_epilogues(env, worst, c):
    """EPI_STREAM, EPI_CSQUARE, EPI_REAL and EPI_WSRHO through fisdf_zgemm_ex: the output, the
    max |Im(alpha acc)| monitor, and the product's own monitors (fisdf_max_imag) untouched."""
    torch, L, ctx = env
    rng = np.random.default_rng(c.epi * 1000 + c.M + c.N + c.K + c.real)
    A, B, _ = G.make_operands(c, rng, real=c.real)
    alpha = 0.5 if c.real else G.ALPHA
    aux = rng.standard_normal((c.M, c.N)) if c.epi == G.EPI_WSRHO else None
    creal = c.epi == G.EPI_REAL
    C0 = np.full((c.batch, c.M, c.N), np.nan if creal else NAN)
    rc, outs, mon, _ = launch(env, c.opA, c.opB, c.M, c.N, c.K, alpha, A, B, 0.0, C0, c.batch,
                              epi=c.epi, aux=aux, entry="ex")
    assert rc == 0, ctx.lib.fisdf_last_error(ctx.h)
    ref, mon_ref = G.ref_epilogue(G.ref_acc(A, B, c.opA, c.opB), alpha, c.epi, aux)
    ldc = c.N + (3 if creal else G.PAD_C)
    out = G.logical(outs[0], c.batch, c.M, c.N, ldc)
    assert np.isfinite(out.view(np.float64)).all()
    pad = G.padding_mask(c.batch, c.M, c.N, ldc)
    assert (outs[0][pad] == (7.0 if creal else G.SENTINEL)).all(), "the padding of C was written"
    if c.epi == G.EPI_STREAM:
        err, tol = abs(out - ref).max(), G.tol_abs(c.K)
    else:
        err, tol = abs(out - ref).max() / abs(ref).max(), G.TOL_REL
    merr = abs(mon - mon_ref)
    print(f"5-epi {G.eid(c)}: err {err:.3e} bound {tol:.3e}; monitor {mon:.6e} ref {mon_ref:.6e}")
    note(worst, "5-epi", err, tol, G.eid(c))
    note(worst, "5-epi-monitor", merr, G.tol_abs(c.K), G.eid(c))
    assert err < tol, err
    assert merr < G.tol_abs(c.K), (mon, mon_ref)
    if c.epi == G.EPI_WSRHO:
        assert (out.imag == 0).all()
    if not c.real and c.epi != G.EPI_STREAM:
        assert mon > 0.1  # a monitor that saw the imaginary parts
    assert ctx.max_imag() == [0.0, 0.0, 0.0], "fisdf_zgemm_ex touched the product's monitors"


def test_zgemm_ex_rejects_what_it_cannot_do(env):
    """An epilogue with beta != 0, EPI_REAL with a batch, EPI_WSRHO without aux and an unknown
    epilogue fail with a message before anything is launched."""
    torch, L, ctx = env
    rng = np.random.default_rng(9)
    A, B = G.rnd(rng, 2, 16, 16), G.rnd(rng, 2, 16, 16)
    for epi, beta, batch in ((G.EPI_CSQUARE, G.BETA, 1), (G.EPI_REAL, 0.0, 2),
                             (G.EPI_WSRHO, 0.0, 1), (3, 0.0, 1)):
        creal = epi == G.EPI_REAL
        C0 = np.full((batch, 16, 16), np.nan if creal else NAN)
        rc, outs, _, before = launch(env, 0, 0, 16, 16, 16, G.ALPHA, A[:batch], B[:batch], beta, C0,
                                     batch, epi=epi, entry="ex")
        assert rc != 0 and len(ctx.lib.fisdf_last_error(ctx.h)) > 0, epi
        assert outs[0].tobytes() == before.tobytes()


# ---- 6. HERK --------------------------------------------------------------------------------------
def herk_ex(env, A, alpha, beta, C0, ks, mode):
    """fisdf_herk_ex on padded views (lda = K + 3, NaN; ldc = n + 5, sentinel; strides with the
    gap).  Returns (rc, flat C, flat start of C)."""
    torch, L, ctx = env
    batch, n, K = A.shape
    abuf, av, sA = G.padded(batch, n, K, K + 3, NAN)
    av[...] = A
    cbuf, cv, sC = G.padded(batch, n, n, n + 5, G.SENTINEL)
    cv[...] = C0
    dA, dC = dev(torch, abuf), dev(torch, cbuf)
    rc = ctx.lib.fisdf_herk_ex(ctx.h, n, K, alpha, L.ptr(dA), K + 3, sA, beta, L.ptr(dC), n + 5, sC,
                               batch, ks, mode)
    ctx.call("fisdf_sync")
    return rc, dC.cpu().numpy(), cbuf


def check_herk(worst, group, name, flat, ref, K, mode=0):
    batch, n = ref.shape[0], ref.shape[1]
    out = G.logical(flat, batch, n, n, n + 5)
    assert np.isfinite(out.view(np.float64)).all(), "NaN / Inf in a stored result"
    assert (flat[G.padding_mask(batch, n, n, n + 5)] == G.SENTINEL).all(), "padding of C written"
    err = abs(out - ref).max()  # both triangles
    print(f"{group} {name}: err {err:.3e} bound {G.tol_abs(K):.3e}")
    note(worst, group, err, G.tol_abs(K), name)
    assert err < G.tol_abs(K), err
    if mode & G.RE_ONLY:
        assert (out.imag == 0).all()
    # the mirror is a copy: elements in different 16-blocks are conjugates bit for bit
    blk = np.arange(n) // 16
    off = np.broadcast_to(blk[:, None] != blk[None, :], out.shape)
    assert out[off].tobytes() == out.conj().swapaxes(-1, -2)[off].tobytes()


@pytest.mark.parametrize("n,K,ks,mode", G.GROUP_HERK)
def test_herk_modes(env, worst, n, K, ks, mode):
    """alpha A A^H and alpha Re(A A^H) (alpha = -0.75, lda > K, ldc > n), with and without
    split-K."""
    torch, L, ctx = env
    rng = np.random.default_rng(n * 1000 + K * 10 + ks + mode)
    A = G.rnd(rng, 1, n, K)
    rc, flat, _ = herk_ex(env, A, G.HERK_ALPHA, 0.0, np.full((1, n, n), NAN), ks, mode)
    assert rc == 0, ctx.lib.fisdf_last_error(ctx.h)
    check_herk(worst, "6-herk", f"n{n}-K{K}-ks{ks}-m{mode}", flat,
               G.ref_herk(A, G.HERK_ALPHA, mode=mode), K, mode)


@pytest.mark.parametrize("n,K", G.GROUP_HERK_BATCHED)
def test_herk_batched(env, worst, n, K):
    """The Cholesky trailing update C[b] -= A[b] A[b]^H on a Hermitian C, batch 3, strides with
    gaps."""
    torch, L, ctx = env
    rng = np.random.default_rng(n * 1000 + K)
    A, C0 = G.rnd(rng, 3, n, K), G.rnd(rng, 3, n, n)
    C0 = C0 + C0.conj().swapaxes(-1, -2)
    rc, flat, _ = herk_ex(env, A, -1.0, 1.0, C0, 1, 0)
    assert rc == 0, ctx.lib.fisdf_last_error(ctx.h)
    check_herk(worst, "6-herk-batched", f"n{n}-K{K}", flat, G.ref_herk(A, -1.0, 1.0, C0), K)


def test_herk_ex_rejects_what_the_batched_herk_cannot_do(env):
    torch, L, ctx = env
    rng = np.random.default_rng(3)
    A, C0 = G.rnd(rng, 3, 24, 37), np.full((3, 24, 24), NAN)
    for ks, mode in ((2, 0), (1, G.RE_ONLY)):
        rc, flat, before = herk_ex(env, A, -1.0, 1.0, C0, ks, mode)
        assert rc != 0 and len(ctx.lib.fisdf_last_error(ctx.h)) > 0
        assert flat.tobytes() == before.tobytes()


# ---- 7. the wide kernel with views ------------------------------------------------------------------
@pytest.mark.parametrize("c", G.GROUP_WIDE, ids=G.gid)
def test_wide_views(env, worst, c):
    """The 64 x 128-tile kernel (FULL, A_REAL, A_LOWER and both) with padded lda / ldb / ldc,
    complex alpha, beta = 0 on a NaN C and complex beta."""
    check_gemm(env, worst, "7-wide", c, "mode")


# ---- 8. degenerate sizes ----------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.GROUP_K0, ids=G.gid)
def test_k_zero(env, worst, c):
    """K = 0 gives C = beta C on both kernels (beta = 0: zeros, C not read)."""
    out = check_gemm(env, worst, "8-k0", c, "zgemm")
    if not c.beta:
        assert (out == 0).all()


@pytest.mark.parametrize("c", G.GROUP_EMPTY, ids=G.gid)
def test_empty_sizes(env, c):
    """M = 0, N = 0 and batch = 0 return 0 and leave C untouched."""
    torch, L, ctx = env
    rng = np.random.default_rng(5)
    A, B, _ = G.make_operands(c, rng)
    cbuf = np.full(70 * (45 + G.PAD_C) + G.GAP, G.SENTINEL)
    abuf, av, sA = G.padded(c.batch, A.shape[1], A.shape[2], A.shape[2] + G.PAD_A, NAN)
    bbuf, bv, sB = G.padded(c.batch, B.shape[1], B.shape[2], B.shape[2] + G.PAD_B, NAN)
    av[...] = A
    bv[...] = B
    dA, dB, dC = dev(torch, abuf), dev(torch, bbuf), dev(torch, cbuf)
    for entry in ("fisdf_zgemm", "fisdf_zgemm_ex"):
        tail = (2,) if entry == "fisdf_zgemm" else (2, 0, 0, None, 0, None)
        rc = getattr(ctx.lib, entry)(ctx.h, c.opA, c.opB, c.M, c.N, c.K, c2(G.ALPHA), L.ptr(dA),
                                     A.shape[2] + G.PAD_A, sA, L.ptr(dB), B.shape[2] + G.PAD_B, sB,
                                     c2(G.BETA), L.ptr(dC), 45 + G.PAD_C, cbuf.size, c.batch, *tail)
        ctx.call("fisdf_sync")
        assert rc == 0, ctx.lib.fisdf_last_error(ctx.h)
        assert dC.cpu().numpy().tobytes() == cbuf.tobytes()
