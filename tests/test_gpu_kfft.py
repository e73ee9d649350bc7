"""The exact FFT-grid K (ISDF.k_method = "fft") on the device: the pair-density builder and the
contraction through the C-ABI against long-double restatements, fisdf_get_k_fft against the
composed long-double reference, then end to end against the oracle's exact_k.

Cases, references, the restated plan rule, the bounds and the conventions live in
tests/kfft_cases.py (tests/test_kfft_cases.py checks them on the CPU).  Every input is a view into
a buffer of NaN (the k blocks of f are f_kstride > ngrid * nao apart), every output a view into the
sentinel 7 + 7j, which must come back bitwise.  Each family prints its largest error / bound ratio
so far (RATIO).  End to end: max |vk - exact_k| < JK_TOL = 1e-8 Ha, the project's bar; without the
feature vk is the ISDF K.
"""
import functools
import os

import numpy as np
import pytest

import kfft_cases as K
from cases import inputs
from kfft_gpu import edges_intact, env, f_view, nan_view, out_view  # noqa: F401 (env: a fixture)

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


# ---- the pair-density builder ---------------------------------------------------------------------
@pytest.mark.parametrize("c", K.PAIR_CASES, ids=K.pair_id)
def test_pair_density(env, c):
    torch, L, ctx = env
    f1, f2 = K.pair_inputs(c)
    b1, v1 = nan_view(torch, f1)
    b2, v2 = (b1, v1) if c.same else nan_view(torch, f2)
    n = c.nao * c.nao * c.ngrid
    for m0, m1 in K.row_ranges(c.nao):
        ref = K.pair_ref(f1, f2, m0, m1)
        ob, ov = out_view(torch, n)
        lo, hi = m0 * c.nao * c.ngrid, m1 * c.nao * c.ngrid
        ctx.call("fisdf_pair_density", L.ptr(v1), L.ptr(v2), c.ngrid, c.nao, m0, m1,
                 L.ptr(ov[lo:]))
        ctx.call("fisdf_sync")
        assert edges_intact(ob, n)
        out = ov.cpu().numpy()
        assert np.all(out[:lo] == K.SENTINEL) and np.all(out[hi:] == K.SENTINEL)
        got = out[lo:hi].reshape(ref.shape)
        # one complex product per element: 2 eps |ref| (kfft_cases' docstring)
        excess = float((abs(got.astype(K.CLD) - ref) / abs(ref)).max())
        print(f"pair {K.pair_id(c)} rows [{m0}, {m1}): worst element {excess / K.EPS:.2f} eps")
        note("pair", excess, 2 * K.EPS)
        assert excess <= 2 * K.EPS
    bad = ctx.lib.fisdf_pair_density(ctx.h, L.ptr(v1), L.ptr(v2), c.ngrid, c.nao, 1, 1, L.ptr(ov))
    assert bad < 0 and ctx.lib.fisdf_last_error(ctx.h)


# ---- the contraction ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def contract_refs(c, m0, m1, scale):
    Z, u, f1, vk0 = K.contract_inputs(c)
    Zr = Z[m0 * c.nao:m1 * c.nao]
    ref = K.contract_ref(Zr, u, f1, c.mesh, K.contract_kd(c), m0, m1, scale)
    return ref, K.rel_err(K.contract_ref(Zr, u, f1, c.mesh, K.contract_kd(c), m0, m1, scale,
                                         wide=False), ref)


@pytest.mark.parametrize("c", K.CONTRACT_CASES, ids=K.contract_id)
def test_exx_contract(env, c):
    torch, L, ctx = env
    Z, u, f1, vk0 = K.contract_inputs(c)
    ngrid = int(np.prod(c.mesh))
    kd = K.contract_kd(c)
    kd_c, kd_p = L.darr(kd if kd is not None else np.zeros(3))
    ma, mp = L.iarr(c.mesh)
    zb, zv = nan_view(torch, Z)
    ub, uv = nan_view(torch, u)
    fb, fv = nan_view(torch, f1)
    n = c.nset * c.nao * c.nao
    scale = 0.37

    def run(start, m0, m1, times=1):
        ob, ov = out_view(torch, n, start)
        for _ in range(times):
            ctx.call("fisdf_exx_contract", L.ptr(zv[m0 * c.nao * ngrid:]), L.ptr(uv), L.ptr(fv), mp,
                     kd_p if kd is not None else None, m0, m1, c.nao, c.nset, scale, L.ptr(ov))
        ctx.call("fisdf_sync")
        assert edges_intact(ob, n)
        return ov.cpu().numpy().reshape(c.nset, c.nao, c.nao)

    zero = np.zeros((c.nset, c.nao, c.nao), complex)
    for m0, m1 in K.row_ranges(c.nao):
        ref, err64 = contract_refs(c, m0, m1, scale)
        x = run(zero, m0, m1)
        assert np.array_equal(x, run(zero, m0, m1))               # ordered sums: repeatable
        outside = np.ones(c.nao, bool)
        outside[m0:m1] = False
        assert np.all(x[:, outside] == 0)
        err, tol = K.rel_err(x[:, m0:m1], ref), K.bound(err64, c.nao * ngrid)
        print(f"contract {K.contract_id(c)} rows [{m0}, {m1}): err {err:.2e} float64 {err64:.2e} "
              f"bound {tol:.2e}")
        note("contract", err, tol)
        assert err <= tol
        # onto a non-zero vk the call adds (one rounding of vk + x, fused or not: 2 eps of the
        # terms), twice in order, and leaves the other rows bitwise
        once, twice = run(vk0, m0, m1), run(vk0, m0, m1, times=2)
        assert np.array_equal(once[:, outside], vk0[:, outside])
        assert np.array_equal(twice[:, outside], vk0[:, outside])
        slack = 2 * K.EPS * (abs(vk0) + 2 * abs(x))
        assert np.all(abs(once - (vk0 + x)) <= slack)
        assert np.all(abs(twice - (once + x)) <= slack)
    # a row m travels alone as it does in the whole: bitwise
    whole = run(zero, 0, c.nao)
    m = min(1, c.nao - 1)
    assert np.array_equal(run(zero, m, m + 1)[:, m], whole[:, m])


def test_exx_contract_arguments_checked(env):
    torch, L, ctx = env
    c = next(c for c in K.CONTRACT_CASES if c.nao == 13 and c.nset == 2)
    Z, u, f1, vk0 = K.contract_inputs(c)
    zb, zv = nan_view(torch, Z)
    ub, uv = nan_view(torch, u)
    fb, fv = nan_view(torch, f1)
    n = c.nset * c.nao * c.nao
    ob, ov = out_view(torch, n)
    before = ob.cpu().numpy()
    ma, mp = L.iarr(c.mesh)
    for m0, m1, nao, nset in ((0, 0, c.nao, c.nset), (0, c.nao + 1, c.nao, c.nset),
                              (0, 1, 0, c.nset), (0, 1, c.nao, 0), (3, 2, c.nao, c.nset)):
        rc = ctx.lib.fisdf_exx_contract(ctx.h, L.ptr(zv), L.ptr(uv), L.ptr(fv), mp, None, m0, m1,
                                        nao, nset, 1.0, L.ptr(ov))
        assert rc < 0 and ctx.lib.fisdf_last_error(ctx.h)
    ctx.call("fisdf_sync")
    assert np.array_equal(ob.cpu().numpy(), before)


# ---- fisdf_get_k_fft ------------------------------------------------------------------------------
def call_get_k(env, c, f, D, kband, fband, work, fill=None, kstride_delta=0, mesh=None):
    """One call on fresh NaN / sentinel buffers: (rc, output buffer, view, n)."""
    torch, L, ctx = env
    nk, ngrid, nao = f.shape
    fb, fv, ks = f_view(torch, f)
    Db, Dv = nan_view(torch, D)
    no = nk if kband is None else len(kband)
    n = c.nset * no * nao * nao
    ob, ov = out_view(torch, n, fill)
    kma, kmp = L.iarr(c.kmesh)
    ma, mp = L.iarr(c.mesh if mesh is None else mesh)
    aa, ap = L.darr(K.LATTICE.ravel())
    if fband is not None:
        bb, bv = nan_view(torch, fband)
        kb_c, kb_p = L.darr(np.asarray(kband).ravel())
        band_args = (L.ptr(bv), kb_p, len(kband))
    else:
        band_args = (None, None, 0 if kband is None else len(kband))
    rc = ctx.lib.fisdf_get_k_fft(ctx.h, L.ptr(fv), ks + kstride_delta, kmp, mp, ap, nao, L.ptr(Dv),
                                 c.nset, float(c.omega), *band_args, int(work), L.ptr(ov))
    ctx.call("fisdf_sync")
    return rc, ob, ov, n


@pytest.mark.parametrize("c", K.GETK_CASES, ids=K.getk_id)
def test_get_k_fft(env, c):
    torch, L, ctx = env
    f, D, kpts, kband, fband = K.getk_inputs(c)
    ref, err64 = K.getk_refs(c)
    nk, ngrid, nao = f.shape
    ctx.call("fisdf_set_omega", 0.123)        # the context's own setting is not what is used
    runs = []
    for work in K.getk_budgets(c) + [0]:
        rc, ob, ov, n = call_get_k(env, c, f, D, kband, fband, work)
        assert rc == 0, ctx.lib.fisdf_last_error(ctx.h)
        assert edges_intact(ob, n)
        runs.append(ov.cpu().numpy().reshape(ref.shape))
    # ... and is left as it was: the context's coulG still carries omega = 0.123
    w = torch.empty(ngrid, dtype=torch.float64, device="cuda")
    ma, mp = L.iarr(c.mesh)
    aa, ap = L.darr(K.LATTICE.ravel())
    qa, qp = L.darr(kpts[-1] + 0.01)
    ctx.call("fisdf_coulg", mp, ap, qp, 1.0, 0, L.ptr(w))
    ctx.call("fisdf_set_omega", 0.0)
    ctx.call("fisdf_sync")
    wref = K.coulG(K.LATTICE, kpts[-1] + 0.01, c.mesh, 0.123)
    assert abs(w.cpu().numpy() - wref).max() <= 1e-12 * wref.max()
    for r in runs[1:]:                        # every budget and the repeat call: bitwise
        assert np.array_equal(r, runs[0])
    err, tol = K.rel_err(runs[0], ref), K.k_bound(err64, nk, nao, ngrid)
    print(f"get_k_fft {K.getk_id(c)}: err {err:.2e} float64 {err64:.2e} bound {tol:.2e}")
    note("get_k_fft", err, tol)
    assert err <= tol
    if c.band == "on":                        # mesh points given as band points: the mesh rows
        rc, ob, ov, n = call_get_k(env, c, f, D, None, None, 0)
        assert rc == 0
        rows = ov.cpu().numpy().reshape(c.nset, nk, nao, nao)[:, list(K.ON_MESH_BAND)]
        assert K.rel_err(runs[0], rows) <= tol


def test_get_k_fft_refusals(env):
    """Every refusal comes before the first launch: d_vk stays as it was, bitwise."""
    torch, L, ctx = env
    c = K.GETK_CASES[1]
    f, D, kpts, kband, fband = K.getk_inputs(c)
    nk, ngrid, nao = f.shape
    row = 16 * nao * ngrid
    offb = K.GETK_CASES[5]
    fo, Do, kpo, kbo, fbo = K.getk_inputs(offb)
    calls = [
        (c, f, D, None, None, dict(work=row - 1), b"work_bytes"),
        (c, f, D, None, None, dict(work=0, kstride_delta=-K.KPAD - 1), b"f_kstride"),
        (offb, fo, Do, kbo, None, dict(work=0), b"band"),
    ]
    for cc, ff, DD, kb, fb, kw, word in calls:
        rc, ob, ov, n = call_get_k(env, cc, ff, DD, kb, fb, **kw)
        assert rc < 0 and word in ctx.lib.fisdf_last_error(ctx.h), ctx.lib.fisdf_last_error(ctx.h)
        assert np.all(ob.cpu().numpy() == K.SENTINEL)
    # a mesh fft3d refuses (17 has no radix)
    mesh = K.REFUSED_MESH
    cr = c._replace(mesh=mesh, nao=3, nset=1)
    rng = np.random.default_rng(17)
    fr = K.F.rnd(rng, nk, int(np.prod(mesh)), 3)
    Dr = K.F.rnd(rng, 1, nk, 3, 3)
    rc, ob, ov, n = call_get_k(env, cr, fr, Dr, None, None, 0)
    assert rc < 0 and b"fft" in ctx.lib.fisdf_last_error(ctx.h)
    assert np.all(ob.cpu().numpy() == K.SENTINEL)


# ---- end to end -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def built(name):
    """A GPU build of the case (its own selection; the AOs evaluated by the library, as a caller
    gets them)."""
    from fisdf import ISDF
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    df = ISDF(cell, cell.get_kpts(kmesh), m0=list(m0), c0=c0)
    df.build()
    return df


@functools.lru_cache(maxsize=None)
def exact(name, omega=0.0):
    from oracle.exact_ref import exact_k
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    kpts = K.mesh_kpts(cell.a, kmesh)
    if omega:
        return K.exact_k64(chi, chi, kpts, kpts, dm, cell.a, cell.mesh, omega)
    if name == "toy222":
        gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toy222.npz")
        return np.load(gold)["vk_exact"]
    return exact_k(chi, dm, cell.a, cell.mesh, kpts, coords)


class method:
    """ISDF.j_method / k_method set for a block on the shared built object, then put back."""

    def __init__(self, df, k="fft", j="isdf"):
        self.df, self.k, self.j = df, k, j

    def __enter__(self):
        self.old = (self.df.k_method, self.df.j_method)
        self.df.k_method, self.df.j_method = self.k, self.j
        return self.df

    def __exit__(self, *exc):
        self.df.k_method, self.df.j_method = self.old


@pytest.mark.parametrize("name", K.E2E_CASES)
def test_exact_k_end_to_end(name):
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    df = built(name)
    with method(df, "fft"):
        vj, vk = df.get_jk(dm)
    vj_i, vk_i = df.get_jk(dm)
    ref = exact(name)
    assert vk.shape == dm.shape
    ek = abs(vk - ref).max()
    print(f"{name}: |K_fft - K_exact| {ek:.2e}, |K_isdf - K_exact| {abs(vk_i - ref).max():.2e} "
          f"(max|K| {abs(ref).max():.3f})")
    note("end_to_end", ek, K.JK_TOL)
    assert ek < K.JK_TOL
    assert np.array_equal(vj, vj_i)           # the J path is untouched
    # a Hermitian dm gives a Hermitian K, with no symmetrisation in the code
    assert abs(dm - dm.conj().swapaxes(-1, -2)).max() < 1e-12
    assert abs(vk - vk.conj().swapaxes(-1, -2)).max() <= 1e-12


def test_two_sets_and_general_dm():
    """nset = 2 with one non-Hermitian dm, hermi = 0."""
    from oracle.exact_ref import exact_k
    name = "toy331_fr"
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    df = built(name)
    rng = np.random.default_rng(11)
    dm2 = np.stack([dm[0], dm[0] + 0.1 * K.F.rnd(rng, *dm.shape[1:])])
    with method(df, "fft", "fft"):
        vj, vk = df.get_jk(dm2, hermi=0)
    assert vk.shape == dm2.shape == vj.shape
    ref = exact_k(chi, dm2, cell.a, cell.mesh, K.mesh_kpts(cell.a, kmesh), coords)
    err = abs(vk - ref).max()
    print(f"{name} nset 2 (one general dm): |dK| {err:.2e}")
    note("end_to_end", err, K.JK_TOL)
    assert err < K.JK_TOL
    assert abs(vk[1] - vk[1].conj().swapaxes(-1, -2)).max() > 1e-6


NAME = "toy222"


@pytest.mark.parametrize("omega", [0.4, -0.4])
def test_omega_without_refit(omega):
    """Range-separated K with the grid J: coulG(omega) is an argument, nothing is refitted."""
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(NAME)
    df = built(NAME)
    df.__dict__.get("_omega_dfs", {}).pop(omega, None)
    with method(df, "fft", "fft"):
        vj, vk = df.get_jk(dm, omega=omega)
        none, vk2 = df.get_jk(dm, omega=omega, with_j=False)
    with method(df, "fft", "isdf"):
        none2, vk3 = df.get_jk(dm, omega=omega, with_j=False)
    assert omega not in df.__dict__.get("_omega_dfs", {})
    assert none is None and none2 is None
    assert np.array_equal(vk, vk2) and np.array_equal(vk, vk3)
    err = abs(vk - exact(NAME, omega)).max()
    print(f"{NAME} omega {omega}: |dK| {err:.2e}")
    note("end_to_end", err, K.JK_TOL)
    assert err < K.JK_TOL
    with method(df, "fft"):                       # the context's Coulomb kernel was not changed
        assert abs(df.get_jk(dm, with_j=False)[1] - exact(NAME)).max() < K.JK_TOL


def test_omega_with_the_isdf_j():
    """j_method = "isdf" with J wanted: the omega sub-object is fitted for J, K is still exact."""
    omega = 0.4
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(NAME)
    df = built(NAME)
    df.__dict__.get("_omega_dfs", {}).pop(omega, None)
    try:
        with method(df, "fft", "isdf"):
            vj, vk = df.get_jk(dm, omega=omega)
        sub = df._omega_dfs[omega]
        assert sub.k_method == "fft" and sub.j_method == "isdf"
        with method(df, "isdf", "isdf"):
            vj_i, vk_i = df.get_jk(dm, omega=omega)
        assert df._omega_dfs[omega] is sub and sub.k_method == "isdf"
    finally:
        df.__dict__.get("_omega_dfs", {}).pop(omega, None)
    assert np.array_equal(vj, vj_i)
    err = abs(vk - exact(NAME, omega)).max()
    print(f"{NAME} omega {omega}, ISDF J: |K_fft - K_exact| {err:.2e}, |K_isdf - K_exact| "
          f"{abs(vk_i - exact(NAME, omega)).max():.2e}")
    assert err < K.JK_TOL


def test_exxdiv_ewald():
    """exxdiv='ewald' on the mesh: the exact K + madelung S D S."""
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(NAME)
    df = built(NAME)
    with method(df, "fft"):
        _, vk = df.get_jk(dm, with_j=False, exxdiv="ewald")
        with pytest.raises(NotImplementedError):
            df.get_jk(dm, omega=0.4, exxdiv="ewald")
    S = df.get_ovlp().cpu().numpy()
    ref = exact(NAME) + df.madelung() * np.einsum("kab,skbc,kcd->skad", S, dm, S)
    err = abs(vk - ref).max()
    print(f"{NAME} ewald: |dK| {err:.2e} (the term itself {abs(ref - exact(NAME)).max():.2e})")
    assert err < K.JK_TOL and abs(ref - exact(NAME)).max() > 1e-3


def test_kpts_band():
    """K at band k-points: off the mesh against exact_k_ref with host band AOs (a block of one
    band point at a time), a mixed list, a 1-D point, and what still raises."""
    from fisdf import cell as C
    import fisdf.isdf as M
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(NAME)
    df = built(NAME)
    rng = np.random.default_rng(4)
    kb = rng.uniform(-0.5, 0.5, (2, 3)) @ cell.reciprocal_vectors()
    xb = C.eval_ao_band(cell, coords, kb)
    kpts = K.mesh_kpts(cell.a, kmesh)
    ref = np.asarray(K.exact_k_ref(chi, xb, kpts, kb, dm, cell.a, cell.mesh), complex)
    ngrid = coords.shape[0]
    old = M.BAND_BLOCK_BYTES
    with method(df, "fft"):
        try:
            M.BAND_BLOCK_BYTES = 16 * ngrid * cell.nao_nr()          # blocks of one band point
            vj_b, vk_b = df.get_jk(dm, kpts_band=kb, with_j=False)
        finally:
            M.BAND_BLOCK_BYTES = old
        assert vj_b is None and vk_b.shape == (1, 2) + dm.shape[-2:]
        err = abs(vk_b - ref).max()
        print(f"{NAME} kpts_band off-mesh: |dK| {err:.2e}")
        note("end_to_end", err, K.JK_TOL)
        assert err < K.JK_TOL
        _, vk = df.get_jk(dm, with_j=False)
        mixed = np.stack([kb[1], df.kpts[5]])
        _, vk_m = df.get_jk(dm, kpts_band=mixed, with_j=False)
        assert abs(vk_m[:, 0] - ref[:, 1]).max() < K.JK_TOL
        assert abs(vk_m[:, 1] - vk[:, 5]).max() < K.JK_TOL
        _, vk1 = df.get_jk(dm, kpts_band=kb[1], with_j=False)
        assert vk1.shape == (1,) + dm.shape[-2:] and abs(vk1[0] - ref[0, 1]).max() < K.JK_TOL
        sel = [5, 0, 3]
        _, vk_s = df.get_jk(dm, kpts_band=df.kpts[sel], with_j=False)
        assert np.array_equal(vk_s, vk[:, sel])
        with pytest.raises(NotImplementedError):
            df.get_jk(dm, kpts_band=kb, with_j=False, exxdiv="ewald")
    with pytest.raises(NotImplementedError):          # the ISDF K has W_q on the mesh only
        df.get_jk(dm, kpts_band=kb, with_j=False)


def test_k_method_validated():
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(NAME)
    df = built(NAME)
    assert df.k_method == "isdf" and df.K_METHODS == ("isdf", "fft")
    with method(df, "exact"):
        with pytest.raises(ValueError):
            df.get_jk(dm)
