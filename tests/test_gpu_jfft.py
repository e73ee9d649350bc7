"""The exact FFT-grid J (ISDF.j_method = "fft") on the device: the two AO kernels and the potential
through the C-ABI against long-double restatements, then end to end against the oracle's exact_j.

Cases, references, the restated launch rules and the conventions live in tests/jfft_cases.py
(tests/test_jfft_cases.py checks on the CPU that the tables reach every branch).  Every input is a
view into a buffer of NaN (the k blocks of f are f_kstride > ngrid * nao apart), every output a
view into the sentinel 7 + 7j, which must come back bitwise.

Bound of the kernel tests (tests/factor_cases.py's rule): the device may be 16 times as far from
the long-double result as the float64 restatement of the same sums is, floored at n eps (n the
length of the longest sum: nk nao^2 for rho, ngrid for the Gram), in max-norm relative to
max |ref|; the potential is floored at 2 * fft_cases.TOL instead (two transforms).
End to end: max |vj - exact_j| < JK_TOL = 1e-8 Ha, the project's bar.  Without the feature vj is
the ISDF J, 8.9e-7 to 1.6e-1 Ha from exact_j on these cases.
"""
import functools

import numpy as np
import pytest

import fft_cases as F
import jfft_cases as J
from cases import inputs

pytestmark = pytest.mark.gpu

NAN = complex(np.nan, np.nan)


@pytest.fixture(scope="module")
def env():
    import torch
    from fisdf import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ctx = _lib.Context(0, torch.cuda.current_stream().cuda_stream)
    return torch, _lib, ctx


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan_view(torch, a):
    """a (flat) on the device inside NaN: (buffer, view of the logical part)."""
    a = np.asarray(a, complex).ravel()
    buf = np.full(a.size + 2 * J.EDGE, NAN)
    buf[J.EDGE:J.EDGE + a.size] = a
    d = dev(torch, buf)
    return d, d[J.EDGE:J.EDGE + a.size]


def f_view(torch, f):
    """f (nk, ngrid, nao) with its k blocks f_kstride apart in NaN: (buffer, view, f_kstride)."""
    nk, ngrid, nao = f.shape
    ks = ngrid * nao + J.KPAD
    buf = np.full(nk * ks + 2 * J.EDGE, NAN)
    for k in range(nk):
        buf[J.EDGE + k * ks: J.EDGE + k * ks + ngrid * nao] = f[k].ravel()
    d = dev(torch, buf)
    return d, d[J.EDGE:], ks


def out_view(torch, n):
    d = dev(torch, np.full(n + 2 * J.EDGE, J.SENTINEL))
    return d, d[J.EDGE:J.EDGE + n]


def edges_intact(d, n):
    h = d.cpu().numpy()
    return bool(np.all(h[:J.EDGE] == J.SENTINEL) and np.all(h[J.EDGE + n:] == J.SENTINEL))


@functools.lru_cache(maxsize=None)
def rho_refs(c):
    f, D, v = J.kernel_inputs(c)
    ref = J.rho_ref(f, D)
    return ref, J.rel_err(J.rho_ref(f, D, wide=False), ref)


@functools.lru_cache(maxsize=None)
def gram_refs(c, scale):
    f, D, v = J.kernel_inputs(c)
    ref = J.gram_ref(f, v, c.conj_v, scale)
    return ref, J.rel_err(J.gram_ref(f, v, c.conj_v, scale, wide=False), ref)


@pytest.mark.parametrize("c", J.KERNEL_CASES, ids=J.case_id)
def test_get_rho(env, c):
    torch, L, ctx = env
    f, D, v = J.kernel_inputs(c)
    ref, err64 = rho_refs(c)
    fb, fv, ks = f_view(torch, f)
    Db, Dv = nan_view(torch, D)
    n = c.nset * c.ngrid
    runs = []
    for _ in range(2):
        ob, ov = out_view(torch, n)
        ctx.call("fisdf_get_rho", L.ptr(fv), ks, c.nk, c.ngrid, c.nao, L.ptr(Dv), c.nset, L.ptr(ov))
        ctx.call("fisdf_sync")
        assert edges_intact(ob, n)
        runs.append(ov.cpu().numpy().reshape(c.nset, c.ngrid))
    assert np.array_equal(runs[0], runs[1])               # no atomics: bitwise repeatable
    err, tol = J.rel_err(runs[0], ref), J.bound(err64, J.rho_sum_length(c))
    print(f"rho {J.case_id(c)}: err {err:.2e} float64 {err64:.2e} bound {tol:.2e}")
    assert err <= tol
    if c.herm:                                            # Hermitian D: rho real to rounding
        assert abs(runs[0].imag).max() <= tol * float(abs(ref).max())


@pytest.mark.parametrize("c", J.KERNEL_CASES, ids=J.case_id)
def test_weighted_gram(env, c):
    torch, L, ctx = env
    f, D, v = J.kernel_inputs(c)
    scale = 0.37
    ref, err64 = gram_refs(c, scale)
    fb, fv, ks = f_view(torch, f)
    vb, vv = nan_view(torch, v)
    n = c.nset * c.nk * c.nao * c.nao
    runs = []
    for _ in range(2):
        ob, ov = out_view(torch, n)
        ctx.call("fisdf_weighted_gram", L.ptr(fv), ks, c.nk, c.ngrid, c.nao, L.ptr(vv), c.nset,
                 c.conj_v, scale, L.ptr(ov))
        ctx.call("fisdf_sync")
        assert edges_intact(ob, n)
        runs.append(ov.cpu().numpy().reshape(c.nset, c.nk, c.nao, c.nao))
    assert np.array_equal(runs[0], runs[1])               # ordered split reduction
    err, tol = J.rel_err(runs[0], ref), J.bound(err64, J.gram_sum_length(c))
    print(f"gram {J.case_id(c)}: err {err:.2e} float64 {err64:.2e} bound {tol:.2e}")
    assert err <= tol
    if c.herm:                                            # real v: each out[s][k] Hermitian
        dev_h = abs(runs[0] - runs[0].conj().swapaxes(-1, -2)).max()
        assert dev_h <= 2 * tol * float(abs(ref).max())


def test_kernel_arguments_checked(env):
    """Bad sizes are refused before anything is launched: the output stays the sentinel."""
    torch, L, ctx = env
    c = J.KERNEL_CASES[1]
    f, D, v = J.kernel_inputs(c)
    fb, fv, ks = f_view(torch, f)
    Db, Dv = nan_view(torch, D)
    ob, ov = out_view(torch, c.nset * c.ngrid)
    before = ob.cpu().numpy()
    for args in ((ks, 0, c.ngrid, c.nao, c.nset), (ks, c.nk, c.ngrid, 0, c.nset),
                 (ks, c.nk, c.ngrid, c.nao, 0), (c.ngrid * c.nao - 1, c.nk, c.ngrid, c.nao, c.nset)):
        kst, nk, ngrid, nao, nset = args
        rc = ctx.lib.fisdf_get_rho(ctx.h, L.ptr(fv), kst, nk, ngrid, nao, L.ptr(Dv), nset, L.ptr(ov))
        assert rc < 0 and ctx.lib.fisdf_last_error(ctx.h)
        rc = ctx.lib.fisdf_weighted_gram(ctx.h, L.ptr(fv), kst, nk, ngrid, nao, L.ptr(Dv), nset, 0,
                                         1.0, L.ptr(ov))
        assert rc < 0 and ctx.lib.fisdf_last_error(ctx.h)
    ctx.call("fisdf_sync")
    assert np.array_equal(ob.cpu().numpy(), before)


@functools.lru_cache(maxsize=None)
def potential_refs(c):
    rho = J.potential_inputs(c)
    ref = J.potential_ref(rho, J.LATTICE, c.mesh, c.omega)
    return ref, J.rel_err(J.potential_ref(rho, J.LATTICE, c.mesh, c.omega, wide=False), ref)


@pytest.mark.parametrize("c", J.POTENTIAL_CASES, ids=J.pot_id)
def test_coulomb_potential(env, c):
    torch, L, ctx = env
    rho = J.potential_inputs(c)
    ref, err64 = potential_refs(c)
    rb, rv = nan_view(torch, rho)
    ob, ov = out_view(torch, rho.size)
    ma, mp = L.iarr(c.mesh)
    aa, ap = L.darr(J.LATTICE.ravel())
    ctx.call("fisdf_set_omega", 0.123)        # the context's own setting is not what is used
    ctx.call("fisdf_coulomb_potential", L.ptr(rv), c.nset, mp, ap, float(c.omega), L.ptr(ov))
    ctx.call("fisdf_set_omega", 0.0)
    ctx.call("fisdf_sync")
    assert edges_intact(ob, rho.size)
    out = ov.cpu().numpy().reshape(rho.shape)
    err, tol = J.rel_err(out, ref), max(J.BOUND_FACTOR * err64, 2 * F.TOL)
    print(f"potential {J.pot_id(c)}: err {err:.2e} float64 {err64:.2e} bound {tol:.2e}")
    assert err <= tol


def test_coulomb_potential_refused_mesh(env):
    """A mesh fft3d refuses (17 has no radix): an error, and the output is untouched."""
    torch, L, ctx = env
    mesh = J.REFUSED_MESH
    n = int(np.prod(mesh))
    rng = np.random.default_rng(17)
    rb, rv = nan_view(torch, F.rnd(rng, 2, n))
    ob, ov = out_view(torch, 2 * n)
    before = ob.cpu().numpy()
    ma, mp = L.iarr(mesh)
    aa, ap = L.darr(J.LATTICE.ravel())
    rc = ctx.lib.fisdf_coulomb_potential(ctx.h, L.ptr(rv), 2, mp, ap, 0.0, L.ptr(ov))
    ctx.call("fisdf_sync")
    assert rc < 0 and b"fft" in ctx.lib.fisdf_last_error(ctx.h)
    assert np.array_equal(ob.cpu().numpy(), before)


# ---- end to end ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def built(name):
    """A GPU build of the case (its own selection; the AOs evaluated by the library, as a caller
    gets them) with the exact J switched on."""
    from fisdf import ISDF
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    df = ISDF(cell, cell.get_kpts(kmesh), m0=list(m0), c0=c0)
    df.build()
    df.j_method = "fft"
    return df


@functools.lru_cache(maxsize=None)
def exact(name, omega=0.0):
    from oracle.exact_ref import exact_j
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    if omega:
        return J.exact_j64(chi, dm, cell.a, cell.mesh, omega)
    return exact_j(chi, dm, cell.a, cell.mesh)


@pytest.mark.parametrize("name", J.E2E_CASES)
def test_exact_j_end_to_end(name):
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    df = built(name)
    vj, vk = df.get_jk(dm)
    ref = exact(name)
    if abs(df.kpts).max() < 1e-9:             # Gamma only: get_jk returns J.real
        assert not np.iscomplexobj(vj)
        ref = ref.real
    assert vj.shape == dm.shape == vk.shape
    ej = abs(vj - ref).max()
    try:
        df.j_method = "isdf"
        vj_i, vk_i = df.get_jk(dm)
    finally:
        df.j_method = "fft"
    print(f"{name}: |J_fft - J_exact| {ej:.2e}, |J_isdf - J_exact| {abs(vj_i - ref).max():.2e} "
          f"(max|J| {abs(ref).max():.3f})")
    assert ej < J.JK_TOL
    assert np.array_equal(vk, vk_i)           # the K path is untouched


NAME = "toy333_fr"


def test_two_sets_and_general_dm():
    """nset = 2, and a non-Hermitian dm (complex rho) with hermi = 0."""
    from fisdf import cell as C
    from oracle.exact_ref import exact_j
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(NAME)
    df = built(NAME)
    rng = np.random.default_rng(11)
    gen = dm[0] + 0.1 * F.rnd(rng, *dm.shape[1:])
    dm2 = np.stack([C.make_dm(cell.nao_nr(), kmesh, cell, seed=77), gen])
    vj, _ = df.get_jk(dm2, hermi=0, with_k=False)
    assert vj.shape == dm2.shape
    ref = exact_j(chi, dm2, cell.a, cell.mesh)
    err = abs(vj - ref).max()
    print(f"{NAME} nset 2 (one general dm): |dJ| {err:.2e}")
    assert err < J.JK_TOL
    rho = df.get_rho(dm2, hermi=0)
    assert np.iscomplexobj(rho) and abs(rho[1].imag).max() > 1e-6
    with pytest.raises(ValueError):
        df.get_rho(dm2, hermi=1)


def test_omega():
    """Range-separated kernels: the omega sub-object inherits j_method (with K: the refit), and
    J alone needs no refit; both against exact_j with coulG(omega)."""
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(NAME)
    df = built(NAME)
    vj, vk = df.get_jk(dm, omega=0.4)
    assert abs(vj - exact(NAME, 0.4)).max() < J.JK_TOL
    assert df._omega_dfs[0.4].j_method == "fft"
    vj2, none = df.get_jk(dm, omega=0.4, with_k=False)
    assert none is None and np.array_equal(vj, vj2)
    assert -0.4 not in df._omega_dfs
    vj3, _ = df.get_jk(dm, omega=-0.4, with_k=False)
    assert -0.4 not in df._omega_dfs              # no refit for J alone
    err = abs(vj3 - exact(NAME, -0.4)).max()
    print(f"{NAME} omega -0.4: |dJ| {err:.2e}")
    assert err < J.JK_TOL
    vj0, _ = df.get_jk(dm, with_k=False)          # the context's Coulomb kernel was put back
    assert abs(vj0 - exact(NAME)).max() < J.JK_TOL


def test_omega_j_method_switched_between_calls():
    """j_method changed on a live object after the omega sub-object exists: the cached sub-object
    (fitted once per omega) follows the parent's current setting in both directions."""
    W = -0.4    # short range: J is large and the ISDF J is far from exact, unlike at +0.4
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(NAME)
    df = built(NAME)
    ref = exact(NAME, W)
    df._omega_dfs.pop(W, None)                    # the sub-object is created under "isdf"
    try:
        df.j_method = "isdf"
        vj_i, vk_i = df.get_jk(dm, omega=W)
        df.j_method = "fft"
        vj_f, vk_f = df.get_jk(dm, omega=W)
        df.j_method = "isdf"
        vj_i2, _ = df.get_jk(dm, omega=W)
    finally:
        df.j_method = "fft"
        df._omega_dfs.pop(W, None)                # the shared object as the other tests expect it
    err = abs(vj_f - ref).max()
    print(f"{NAME} omega {W}: |J_fft - J_exact| {err:.2e}, |J_isdf - J_exact| "
          f"{abs(vj_i - ref).max():.2e}")
    assert err < J.JK_TOL
    assert not np.array_equal(vj_i, vj_f)
    assert np.array_equal(vj_i, vj_i2)
    assert np.array_equal(vk_i, vk_f)             # one fit serves both


def test_kpts_band_exact():
    """J at band k-points: off the mesh the exact v contracted with the band AOs on the FFT grid;
    on the mesh rows of the k-mesh J; a 1-D band point drops the band axis; K off the mesh still
    raises."""
    from fisdf import cell as C
    import fisdf.isdf as M
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(NAME)
    df = built(NAME)
    rng = np.random.default_rng(4)
    kb = rng.uniform(-0.5, 0.5, (3, 3)) @ cell.reciprocal_vectors()
    v = J.exact_v(chi, dm, cell.a, cell.mesh)
    xb = C.eval_ao_band(cell, coords, kb)
    ngrid = coords.shape[0]
    ref = np.einsum("kgm,sg,kgn->skmn", xb.conj(), v, xb) * (abs(np.linalg.det(cell.a)) / ngrid)
    old = M.BAND_BLOCK_BYTES
    try:
        M.BAND_BLOCK_BYTES = 2 * 16 * ngrid * cell.nao_nr()      # blocks of 2 + 1 band points
        vj_b, vk_b = df.get_jk(dm, kpts_band=kb, with_k=False)
    finally:
        M.BAND_BLOCK_BYTES = old
    assert vk_b is None and vj_b.shape == (1, 3) + dm.shape[-2:]
    err = abs(vj_b - ref).max()
    print(f"{NAME} kpts_band off-mesh: |dJ| {err:.2e}")
    assert err < J.JK_TOL
    vj1, _ = df.get_jk(dm, kpts_band=kb[1], with_k=False)
    assert vj1.shape == (1,) + dm.shape[-2:] and abs(vj1[0] - ref[0, 1]).max() < J.JK_TOL
    sel = [5, 0, 3]
    vj2, vk2 = df.get_jk(dm, kpts_band=df.kpts[sel])
    vj, vk = df.get_jk(dm)
    assert np.array_equal(vj2, vj[:, sel]) and np.array_equal(vk2, vk[:, sel])
    with pytest.raises(NotImplementedError):
        df.get_jk(dm, kpts_band=kb, with_j=False)


def test_get_rho_method():
    """rho integrates to the electron count of the grid quadrature, sum_g rho_g vol / ngrid =
    sum_k tr(D_k S_k) / nk with S = get_ovlp(), and equals the restatement."""
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(NAME)
    df = built(NAME)
    rho = df.get_rho(dm)
    ngrid = coords.shape[0]
    assert rho.shape == (1, ngrid) and not np.iscomplexobj(rho)
    assert df.get_rho(dm[0]).shape == (ngrid,)
    S = df.get_ovlp().cpu().numpy()
    nel = np.einsum("kmn,knm->", dm[0], S).real / len(S)
    got = rho[0].sum() * abs(np.linalg.det(cell.a)) / ngrid
    print(f"{NAME}: electrons {got:.12f} vs tr(DS) {nel:.12f}")
    assert abs(got - nel) <= 1e-12 * abs(nel)
    ref = J.rho_ref(chi, dm, wide=False)
    assert abs(rho - ref.real).max() <= 1e-12 * abs(ref).max()


def test_dump_load(tmp_path):
    """A fresh object restored from a dump evaluates the grid AOs on first use: the same J."""
    from fisdf import ISDF
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(NAME)
    df = built(NAME)
    vj, vk = df.get_jk(dm)
    path = tmp_path / "isdf.npz"
    df.dump(path)
    df2 = ISDF(cell, cell.get_kpts(kmesh), m0=list(m0), c0=c0).load(path)
    assert df2._ao_grid is None
    df2.j_method = "fft"
    vj2, vk2 = df2.get_jk(dm)
    assert np.array_equal(vj, vj2) and np.array_equal(vk, vk2)
