"""The exact FFT-grid four-index integrals (ISDF.eri_method = "fft") on the device: the B builder
fisdf_pair34 and the whole fisdf_get_eri_fft through the C-ABI against the long-double
composition, then end to end against the oracle's exact_eri.

Cases, references, the restated plan rule, the bounds and the conventions live in
tests/eri_cases.py (tests/test_eri_cases.py checks them on the CPU).  Every input is a view into a
buffer of NaN, every output a view into the sentinel 7 + 7j, which must come back bitwise.  Each
family prints its largest error / bound ratio so far (RATIO).  End to end: |eri - exact_eri| <=
ERI_TOL max(1, max |ref|), ERI_TOL = 1e-10, the project's bar for ERI equalities; without the
feature get_eri gives the ISDF integrals, which need build() and whose fitting error is orders of
magnitude above that on toy331_fr and si_small.
"""
import functools

import numpy as np
import pytest

import eri_cases as E
import kfft_cases as K
from cases import inputs
from kfft_gpu import NAN, dev, edges_intact, env, nan_view, out_view  # noqa: F401 (env: a fixture)

pytestmark = pytest.mark.gpu

RATIO = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    """When the module's tests are done: the largest error / bound ratio of each family."""
    yield
    for fam, r in sorted(RATIO.items()):
        print(f"largest error/bound ratio, {fam}: {r:.3f}")


def note(family, err, tol):
    RATIO[family] = max(RATIO.get(family, 0.0), err / tol)
    print(f"  [{family}] err/bound {err / tol:.3f}, largest so far {RATIO[family]:.3f}")


def ptr_array(L, views):
    return (L._vp * len(views))(*[v.data_ptr() for v in views])


# ---- the B builder --------------------------------------------------------------------------------
def padded_view(torch, a, pad):
    """a (ngrid, n) at leading dimension n + pad inside NaN: (buffer, view of the first element
    on)."""
    ng, n = a.shape
    buf = np.full((ng, n + pad), NAN)
    buf[:, :n] = a
    return nan_view(torch, buf)


@pytest.mark.parametrize("c", E.PAIR34_CASES, ids=E.case_id)
def test_pair34(env, c):
    torch, L, ctx = env
    a1, a2, a3s, a4s = E.inputs(c)
    n1, n2, n3, n4 = c.sizes
    ngrid = E.ngrid_of(c)
    kd = E.case_kd(c)
    kd_c, kd_p = L.darr(kd if kd is not None else np.zeros(3))
    ma, mp = L.iarr(c.mesh)
    v3 = [padded_view(torch, a, E.LD_PAD) for a in a3s]
    v4 = [padded_view(torch, a, E.LD_PAD) for a in a4s]
    p3, p4 = ptr_array(L, [v for _, v in v3]), ptr_array(L, [v for _, v in v4])
    n = c.npair * n3 * n4 * ngrid
    for r0, r1 in E.row_ranges(c.npair, n3):
        ref = E.pair34_ref(a3s, a4s, c.mesh, kd, r0, r1)
        err64 = E.rel_err(E.pair34_ref(a3s, a4s, c.mesh, kd, r0, r1, wide=False), ref)
        ob, ov = out_view(torch, n)
        lo, hi = r0 * n4 * ngrid, r1 * n4 * ngrid
        ctx.call("fisdf_pair34", p3, p4, c.npair, n3, n4, n3 + E.LD_PAD, n4 + E.LD_PAD, mp,
                 kd_p if kd is not None else None, r0, r1, L.ptr(ov[lo:]))
        ctx.call("fisdf_sync")
        assert edges_intact(ob, n)
        out = ov.cpu().numpy()
        assert np.all(out[:lo] == E.SENTINEL) and np.all(out[hi:] == E.SENTINEL)
        got = out[lo:hi].reshape(ref.shape)
        err, tol = E.rel_err(got, ref), E.pair34_bound(err64)
        print(f"pair34 {E.case_id(c)} rows [{r0}, {r1}): err {err:.2e} float64 {err64:.2e} bound "
              f"{tol:.2e}")
        note("pair34", err, tol)
        assert err <= tol
    for r0, r1 in ((1, 1), (-1, 1), (0, c.npair * n3 + 1)):
        bad = ctx.lib.fisdf_pair34(ctx.h, p3, p4, c.npair, n3, n4, n3 + E.LD_PAD, n4 + E.LD_PAD, mp,
                                   None, r0, r1, L.ptr(ov))
        assert bad < 0 and ctx.lib.fisdf_last_error(ctx.h)
    bad = ctx.lib.fisdf_pair34(ctx.h, p3, p4, c.npair, n3, n4, n3 - 1, n4, mp, None, 0, 1, L.ptr(ov))
    assert bad < 0 and b"leading dimension" in ctx.lib.fisdf_last_error(ctx.h)


# ---- fisdf_get_eri_fft ----------------------------------------------------------------------------
def call_eri(env, c, a1, a2, a3s, a4s, work, mesh=None, sizes=None, npair=None, null=None):
    """One call on fresh NaN / sentinel buffers: (rc, output buffer, view, n)."""
    torch, L, ctx = env
    n1, n2, n3, n4 = c.sizes
    b1, v1 = nan_view(torch, a1)
    b2, v2 = nan_view(torch, a2)
    v3 = [nan_view(torch, a) for a in a3s]
    v4 = [nan_view(torch, a) for a in a4s]
    p3, p4 = ptr_array(L, [v for _, v in v3]), ptr_array(L, [v for _, v in v4])
    n = len(a3s) * n1 * n2 * n3 * n4
    ob, ov = out_view(torch, n)
    ma, mp = L.iarr(c.mesh if mesh is None else mesh)
    aa, ap = L.darr(E.LATTICE.ravel())
    qa, qp = L.darr(E.case_q(c))
    s = c.sizes if sizes is None else sizes
    args = [mp, ap, qp, float(c.omega), L.ptr(v1), s[0], L.ptr(v2), s[1], p3, p4,
            len(a3s) if npair is None else npair, s[2], s[3], int(work), L.ptr(ov)]
    if null is not None:
        args[null] = None
    rc = ctx.lib.fisdf_get_eri_fft(ctx.h, *args)
    ctx.call("fisdf_sync")
    return rc, ob, ov, n


@pytest.mark.parametrize("c", E.CASES, ids=E.case_id)
def test_get_eri_fft(env, c):
    torch, L, ctx = env
    a1, a2, a3s, a4s = E.inputs(c)
    ref, err64 = E.refs(c)
    ngrid = E.ngrid_of(c)
    ctx.call("fisdf_set_omega", 0.123)        # the context's own setting is not what is used
    runs = []
    for work in E.budgets(c) + [0]:           # every budget, and the default again: a repeat call
        rc, ob, ov, n = call_eri(env, c, a1, a2, a3s, a4s, work)
        assert rc == 0, ctx.lib.fisdf_last_error(ctx.h)
        assert edges_intact(ob, n)
        runs.append(ov.cpu().numpy().reshape(ref.shape))
    ctx.call("fisdf_set_omega", 0.0)
    for w, r in zip(E.budgets(c)[1:] + [0], runs[1:]):
        assert np.array_equal(r, runs[0]), f"budget {w}: max |d| {abs(r - runs[0]).max():.2e}"
    err, tol = E.rel_err(runs[0], ref), E.eri_bound(err64, ngrid)
    print(f"get_eri_fft {E.case_id(c)}: err {err:.2e} float64 {err64:.2e} bound {tol:.2e}")
    note("get_eri_fft", err, tol)
    assert err <= tol
    if c.npair > 1:                            # the pairs one call at a time: bitwise
        for p in range(c.npair):
            rc, ob, ov, n = call_eri(env, c, a1, a2, a3s[p:p + 1], a4s[p:p + 1], 0)
            assert rc == 0 and edges_intact(ob, n)
            assert np.array_equal(ov.cpu().numpy().reshape(ref.shape[1:]), runs[-1][p])


def test_get_eri_fft_refusals(env):
    """Every refusal comes before d_out is written: it stays as it was, bitwise."""
    torch, L, ctx = env
    c = next(c for c in E.CASES if c.sizes == E.MIXED and c.mesh == (8, 8, 8))
    a1, a2, a3s, a4s = E.inputs(c)
    n1, n2, n3, n4 = c.sizes
    row = 16 * max(n2, n4) * E.ngrid_of(c)
    calls = [
        (dict(work=0, null=4), b"null"),                               # d_a1
        (dict(work=0, null=8), b"null"),                               # h_d_a3
        (dict(work=0, null=0), b"null"),                               # mesh
        (dict(work=0, sizes=(0, n2, n3, n4)), b"sizes"),
        (dict(work=0, sizes=(n1, n2, n3, 0)), b"sizes"),
        (dict(work=0, npair=0), b"sizes"),
        (dict(work=row - 1), b"work_bytes"),
        (dict(work=16 * n2 * E.ngrid_of(c)), b"work_bytes"),           # a row i fits, a row of B not
        (dict(work=-1), b"bad arguments"),
    ]
    for kw, word in calls:
        rc, ob, ov, n = call_eri(env, c, a1, a2, a3s, a4s, **kw)
        msg = ctx.lib.fisdf_last_error(ctx.h)
        assert rc < 0 and word in msg, (kw, msg)
        assert np.all(ob.cpu().numpy() == E.SENTINEL)
    # a mesh fft3d refuses (17 has no radix): B is built into the arena, d_out is not reached
    mesh = E.REFUSED_MESH
    ng = int(np.prod(mesh))
    rng = np.random.default_rng(17)
    b1, b2 = K.F.rnd(rng, ng, n1), K.F.rnd(rng, ng, n2)
    b3 = [K.F.rnd(rng, ng, n3) for _ in range(c.npair)]
    b4 = [K.F.rnd(rng, ng, n4) for _ in range(c.npair)]
    rc, ob, ov, n = call_eri(env, c, b1, b2, b3, b4, 0, mesh=mesh)
    assert rc < 0 and b"fft" in ctx.lib.fisdf_last_error(ctx.h)
    assert np.all(ob.cpu().numpy() == E.SENTINEL)


# ---- end to end -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fresh(name):
    """The case's ISDF object without build(): the exact integrals need only the AOs on the grid
    (evaluated by the library, as a caller gets them)."""
    from fisdf import ISDF
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    df = ISDF(cell, cell.get_kpts(kmesh), m0=list(m0), c0=c0)
    df.eri_method = "fft"
    return df


@functools.lru_cache(maxsize=None)
def built(name):
    from fisdf import ISDF
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    df = ISDF(cell, cell.get_kpts(kmesh), m0=list(m0), c0=c0)
    df.build()
    return df


def _eri_ref(cell, kmesh, chi, coords):
    """The oracle's exact_eri as an eri_ref callable (test_coul.py's)."""
    from oracle import exact_ref as X
    kpts = cell.get_kpts(kmesh)

    def f(kq):
        idx = [int(np.argmin(abs(kpts - k).sum(1))) for k in kq]
        return X.exact_eri(chi, cell.lattice_vectors(), cell.mesh, kpts, coords, *idx)
    return f


def kidx_of(kmesh):
    from fisdf.cell import cartesian_prod
    ks = cartesian_prod([np.arange(n) for n in kmesh])

    def kidx(v):
        v = np.mod(v, kmesh)
        return int((v[0] * kmesh[1] + v[1]) * kmesh[2] + v[2])
    return ks, kidx


def quartets(kmesh):
    """(k1, k2, k3, k4): Gamma, and (where the mesh has them) two with q != 0."""
    nk = int(np.prod(kmesh))
    ks, kidx = kidx_of(kmesh)
    out = [(0, 0, 0)] + ([(0, 1, 2 % nk), (3 % nk, 5 % nk, 6 % nk)] if nk > 1 else [])
    return [(k1, k2, k3, kidx(ks[k1] - ks[k2] + ks[k3])) for k1, k2, k3 in out]


def within_bar(got, ref, what):
    err, tol = abs(got - ref).max(), E.ERI_TOL * max(1.0, abs(ref).max())
    print(f"{what}: |d eri| {err:.2e} (max |eri| {abs(ref).max():.3f})")
    note("end_to_end", err, tol)
    assert err <= tol


@pytest.mark.parametrize("name", E.E2E_CASES)
def test_exact_eri_end_to_end(name):
    from oracle.exact_ref import exact_eri
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    df = fresh(name)
    assert df._dev_state is None                       # no build()
    kpts = K.mesh_kpts(cell.a, kmesh)
    nao = cell.nao_nr()
    for q4 in quartets(kmesh):
        eri = df.get_eri(kpts[list(q4)])
        assert eri.shape == (nao * nao, nao * nao)
        ref = exact_eri(chi, cell.a, cell.mesh, kpts, coords, *q4).reshape(nao * nao, nao * nao)
        if abs(kpts[list(q4)]).max() < 1e-9:
            # the Gamma quartet comes back as its real part, as PySCF's does (on an even mesh the
            # lone Nyquist plane leaves a small imaginary part in the exact integrals themselves)
            assert np.isrealobj(eri)
            ref = ref.real
        within_bar(eri, ref, f"{name} {q4}")
    assert df._dev_state is None


NAME = "toy222"


def test_ao2mo_complex_coefficients():
    """MO coefficients of widths (3, 4, 2, 5), applied on the device, against the exact AO
    integrals transformed on the host."""
    from oracle.exact_ref import exact_eri
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(NAME)
    df = fresh(NAME)
    kpts = K.mesh_kpts(cell.a, kmesh)
    nao = cell.nao_nr()
    rng = np.random.default_rng(3)
    Cs = [K.F.rnd(rng, nao, n) for n in E.MIXED]
    q4 = quartets(kmesh)[2]
    ao = exact_eri(chi, cell.a, cell.mesh, kpts, coords, *q4)
    ref = np.einsum("mnkl,mi,nj,ka,lb->ijab", ao, Cs[0].conj(), Cs[1], Cs[2].conj(), Cs[3],
                    optimize=True).reshape(3 * 4, 2 * 5)
    mo = df.ao2mo(Cs, kpts[list(q4)])
    assert mo.shape == ref.shape
    within_bar(mo, ref, f"{NAME} ao2mo {q4}")
    with pytest.raises(ValueError):
        df.get_eri(kpts[[0, 1, 1, 3]])                 # violates k1 - k2 + k3 - k4 = G


def test_off_mesh_quartet():
    """Four k-points off the k-mesh that conserve momentum: the AOs are evaluated at them."""
    from oracle.exact_ref import exact_eri
    from fisdf import cell as C
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(NAME)
    df = fresh(NAME)
    rng = np.random.default_rng(4)
    kb = rng.uniform(-0.5, 0.5, (3, 3)) @ cell.reciprocal_vectors()
    kb = np.vstack([kb, kb[0] - kb[1] + kb[2]])
    xb = C.eval_ao_band(cell, coords, kb)
    nao = cell.nao_nr()
    ref = exact_eri(xb, cell.a, cell.mesh, kb, coords, 0, 1, 2, 3).reshape(nao * nao, -1)
    within_bar(df.get_eri(kb), ref, f"{NAME} off-mesh quartet")
    with pytest.raises(ValueError):
        df.get_eri(np.vstack([kb[:3], kb[3] + 0.01]))


def test_get_eri_omega():
    """coulG(q, omega) is an argument of the exact integrals: against the complex128 composition."""
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(NAME)
    df = fresh(NAME)
    kpts = K.mesh_kpts(cell.a, kmesh)
    k1, k2, k3, k4 = quartets(kmesh)[1]
    ref = E.eri64(chi[k1], chi[k2], [chi[k3]], [chi[k4]], cell.a, cell.mesh, kpts[k2] - kpts[k1],
                  0.4)[0]
    eri = df.get_eri(kpts[[k1, k2, k3, k4]], omega=0.4)
    within_bar(eri, ref, f"{NAME} omega 0.4")
    plain = df.get_eri(kpts[[k1, k2, k3, k4]])
    assert abs(plain - eri).max() > 1e-3               # the kernel did change


def test_get_eri_many_and_isdf_unchanged():
    """get_eri_many: one call for the pairs that share (k1, k2) equals the single calls bitwise;
    with eri_method = "isdf" it is a loop of the existing entry."""
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(NAME)
    df = fresh(NAME)
    kpts = K.mesh_kpts(cell.a, kmesh)
    ks, kidx = kidx_of(kmesh)
    k1, k2 = 3, 5
    k34 = np.stack([kpts[[k3, kidx(ks[k1] - ks[k2] + ks[k3])]] for k3 in (6, 0, 7)])
    many = df.get_eri_many(kpts[[k1, k2]], k34)
    assert many.shape == (3, cell.nao_nr() ** 2, cell.nao_nr() ** 2)
    for p in range(3):
        assert np.array_equal(many[p], df.get_eri(np.vstack([kpts[[k1, k2]], k34[p]])))
    dfi = built(NAME)
    assert dfi.eri_method == "isdf" and dfi.ERI_METHODS == ("isdf", "fft")
    many_i = dfi.get_eri_many(kpts[[k1, k2]], k34)
    for p in range(3):
        assert np.array_equal(many_i[p], dfi.get_eri(np.vstack([kpts[[k1, k2]], k34[p]])))
    assert abs(many_i - many).max() < 1e-6              # the fit's error on this case


def test_check_eri_with_the_exact_holder():
    """check_eri with FFTDF(cell, exact=True): the device's exact integrals in place of the
    oracle's, on the seven triples of test_coul.py's harness test."""
    from fisdf import coul
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(NAME)
    df = coul.FFTDF(cell, exact=True)
    c, x = coul.get_coul(df, kmesh=kmesh, m0=list(m0))
    triples = E.check_triples(int(np.prod(kmesh)))
    worst = coul.check_eri(df, kmesh, c, x, tol=1e-6, triples=triples)
    fed = coul.FFTDF(cell, eri_ref=_eri_ref(cell, kmesh, chi, coords))
    fed._isdf = df._isdf                                # the same fit, the oracle's exact ERIs
    worst_fed = coul.check_eri(fed, kmesh, c, x, tol=1e-6, triples=triples)
    print(f"check_eri worst: exact holder {worst:.3e}, oracle-fed {worst_fed:.3e}")
    assert abs(worst - worst_fed) <= 1e-9
    assert df._isdf.eri_method == "isdf"                # the fitted object is left as it was
    with pytest.raises(AssertionError):
        coul.check_eri(df, kmesh, c, x, tol=worst / 2, triples=triples)
    # before get_coul the holder's exact integrals come from a private object
    lone = coul.FFTDF(cell, cell.get_kpts(kmesh), exact=True)
    kpts = K.mesh_kpts(cell.a, kmesh)
    kq = kpts[list(quartets(kmesh)[1])]
    assert np.array_equal(lone.get_eri(kq), fresh(NAME).get_eri(kq))


def test_sharded_and_bad_method_raise():
    from fisdf import ISDF, kshard
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(NAME)
    kpts = cell.get_kpts(kmesh)
    df = ISDF(cell, kpts, m0=list(m0), c0=c0, comm=kshard.EmulatedGroup(0, 2))
    df.eri_method = "fft"
    with pytest.raises(NotImplementedError):
        df.get_eri(kpts[[0, 0, 0, 0]])
    df = fresh(NAME)
    df.eri_method = "exact"
    try:
        for call in (lambda: df.get_eri(kpts[[0, 0, 0, 0]]),
                     lambda: df.ao2mo(None, kpts[[0, 0, 0, 0]]),
                     lambda: df.get_eri_many(kpts[[0, 0]], kpts[None, [0, 0]])):
            with pytest.raises(ValueError):
                call()
    finally:
        df.eri_method = "fft"
