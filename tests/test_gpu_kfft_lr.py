"""The exact FFT-grid K in the occupied-orbital form (ISDF.k_form = "lowrank") on the device: the
pair builder against the orbitals on the grid and the segmented contraction through the C-ABI
against long-double restatements, fisdf_get_k_fft_lr against kfft_cases' long-double exact_k_ref on
D = A B^H, then through ISDF against the oracle's exact_k.

Cases, references, the restated plan rule and the bounds live in tests/kfft_lr_cases.py
(tests/test_kfft_lr_cases.py checks them on the CPU); the conventions are test_gpu_kfft.py's: every
input is a view into a buffer of NaN, every output a view into the sentinel 7 + 7j, which must come
back bitwise; each family prints its largest error / bound ratio so far (RATIO).
"""
import functools

import numpy as np
import pytest

import kfft_cases as K
import kfft_lr_cases as R
from cases import inputs
from kfft_gpu import NAN, edges_intact, env, f_view, nan_view, out_view  # noqa: F401 (env: a fixture)

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


# ---- the pair builder -----------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.PAIR_CASES, ids=R.pair_id)
def test_pair_density_lr(env, c):
    torch, L, ctx = env
    for ni in R.PAIR_NIS:
        f1, psi = R.pair_inputs(c, ni)
        ld = psi.shape[1]
        b1, v1 = nan_view(torch, f1)
        b2, v2 = nan_view(torch, psi)
        n = c.nao * ni * c.ngrid
        for m0, m1 in K.row_ranges(c.nao):
            ref = R.pair_ref(f1, psi[:, :ni], m0, m1)
            ob, ov = out_view(torch, n)
            lo, hi = m0 * ni * c.ngrid, m1 * ni * c.ngrid
            ctx.call("fisdf_pair_density_lr", L.ptr(v1), c.nao, L.ptr(v2), ni, ld, c.ngrid, m0, m1,
                     L.ptr(ov[lo:]))
            ctx.call("fisdf_sync")
            assert edges_intact(ob, n)
            out = ov.cpu().numpy()
            assert np.all(out[:lo] == K.SENTINEL) and np.all(out[hi:] == K.SENTINEL)
            got = out[lo:hi].reshape(ref.shape)
            # one complex product per element: 2 eps |ref| (kfft_cases' docstring)
            excess = float((abs(got.astype(K.CLD) - ref) / abs(ref)).max())
            print(f"pair_lr {R.pair_id(c)} I {ni} rows [{m0}, {m1}): worst element "
                  f"{excess / K.EPS:.2f} eps")
            note("pair_lr", excess, 2 * K.EPS)
            assert excess <= 2 * K.EPS
        # refused: an empty or reversed row range, rows beyond nao, ld below ni; nothing is written
        before = ob.cpu().numpy()
        for m0, m1, ldb in ((1, 1, ld), (0, c.nao + 1, ld), (1, 0, ld), (0, 1, ni - 1)):
            bad = ctx.lib.fisdf_pair_density_lr(ctx.h, L.ptr(v1), c.nao, L.ptr(v2), ni, ldb,
                                                c.ngrid, m0, m1, L.ptr(ov))
            assert bad < 0 and ctx.lib.fisdf_last_error(ctx.h)
        ctx.call("fisdf_sync")
        assert np.array_equal(ob.cpu().numpy(), before)


def test_pair_density_is_the_lr_builder_on_f2(env):
    """fisdf_pair_density(f1, f2) and fisdf_pair_density_lr(f1, nao, psi = f2, ni = nao, ld = nao)
    write the same bits: the dm form's builder is the general one at that point, which is what lets
    kfft.hip keep a single pair kernel."""
    torch, L, ctx = env
    for c in K.PAIR_CASES:
        f1, f2 = K.pair_inputs(c)
        b1, v1 = nan_view(torch, f1)
        b2, v2 = (b1, v1) if c.same else nan_view(torch, f2)
        n = c.nao * c.nao * c.ngrid
        for m0, m1 in K.row_ranges(c.nao):
            lo = m0 * c.nao * c.ngrid
            ob, ov = out_view(torch, n)
            ctx.call("fisdf_pair_density", L.ptr(v1), L.ptr(v2), c.ngrid, c.nao, m0, m1,
                     L.ptr(ov[lo:]))
            rb, rv = out_view(torch, n)
            ctx.call("fisdf_pair_density_lr", L.ptr(v1), c.nao, L.ptr(v2), c.nao, c.nao, c.ngrid,
                     m0, m1, L.ptr(rv[lo:]))
            ctx.call("fisdf_sync")
            assert edges_intact(ob, n) and edges_intact(rb, n)
            assert np.array_equal(ov.cpu().numpy(), rv.cpu().numpy()), (K.pair_id(c), m0, m1)


# ---- the segmented contraction --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def contract_refs(c, m0, m1, scale):
    Z, u, f1, vk0 = R.contract_inputs(c)
    ni = sum(c.lengths)
    args = (Z[m0 * ni:m1 * ni], u, f1, c.mesh, R.contract_kd(c), m0, m1, tuple(R.segments(c.lengths)),
            scale)
    ref = R.contract_ref(*args)
    return ref, K.rel_err(R.contract_ref(*args, wide=False), ref)


@pytest.mark.parametrize("c", R.CONTRACT_CASES, ids=R.contract_id)
def test_exx_contract_lr(env, c):
    """fisdf_exx_contract_lr always adds to vk (api.hip passes accumulate = 1), so this test covers
    adding onto zero and onto vk0.  The reduce's overwrite branch is reached only by
    fisdf_get_k_fft_lr, at the first k2 that has work: test_get_k_fft_lr runs it over a NaN-filled
    d_vk with sentinel edges, where a wrong overwrite shows as NaN or as an error above the bound."""
    torch, L, ctx = env
    Z, u, f1, vk0 = R.contract_inputs(c)
    ngrid, ni, nset = int(np.prod(c.mesh)), sum(c.lengths), len(c.lengths)
    kd = R.contract_kd(c)
    kd_c, kd_p = L.darr(kd if kd is not None else np.zeros(3))
    ma, mp = L.iarr(c.mesh)
    sa, sp = L.iarr(R.segments(c.lengths))
    zb, zv = nan_view(torch, Z)
    ub, uv = nan_view(torch, u)
    fb, fv = nan_view(torch, f1)
    n = nset * c.nao * c.nao
    scale = 0.37
    empty = [s for s, ln in enumerate(c.lengths) if ln == 0]
    longest = max(c.lengths)

    def run(start, m0, m1, times=1):
        ob, ov = out_view(torch, n, start)
        for _ in range(times):
            ctx.call("fisdf_exx_contract_lr", L.ptr(zv[m0 * ni * ngrid:]), L.ptr(uv), L.ptr(fv), mp,
                     kd_p if kd is not None else None, m0, m1, c.nao, ni, sp, nset, scale,
                     L.ptr(ov))
        ctx.call("fisdf_sync")
        assert edges_intact(ob, n)
        return ov.cpu().numpy().reshape(nset, c.nao, c.nao)

    zero = np.zeros((nset, c.nao, c.nao), complex)
    for m0, m1 in K.row_ranges(c.nao):
        ref, err64 = contract_refs(c, m0, m1, scale)
        x = run(zero, m0, m1)
        assert np.array_equal(x, run(zero, m0, m1))               # ordered sums: repeatable
        outside = np.ones(c.nao, bool)
        outside[m0:m1] = False
        assert np.all(x[:, outside] == 0)
        assert np.all(x[empty] == 0)                              # an empty segment: exact zeros
        err, tol = K.rel_err(x[:, m0:m1], ref), K.bound(err64, longest * ngrid)
        print(f"contract_lr {R.contract_id(c)} rows [{m0}, {m1}): err {err:.2e} float64 "
              f"{err64:.2e} bound {tol:.2e}")
        note("contract_lr", err, tol)
        assert err <= tol
        # onto a non-zero vk the call adds (one rounding of vk + x: 2 eps of the terms), twice in
        # order, and leaves the other rows and the empty sets bitwise
        once, twice = run(vk0, m0, m1), run(vk0, m0, m1, times=2)
        assert np.array_equal(once[:, outside], vk0[:, outside])
        assert np.array_equal(twice[:, outside], vk0[:, outside])
        assert np.array_equal(once[empty], vk0[empty]) and np.array_equal(twice[empty], vk0[empty])
        slack = 2 * K.EPS * (abs(vk0) + 2 * abs(x))
        assert np.all(abs(once - (vk0 + x)) <= slack)
        assert np.all(abs(twice - (once + x)) <= slack)
    # a row m travels alone as it does in the whole: bitwise
    whole = run(zero, 0, c.nao)
    m = min(1, c.nao - 1)
    assert np.array_equal(run(zero, m, m + 1)[:, m], whole[:, m])


def test_exx_contract_lr_arguments_checked(env):
    torch, L, ctx = env
    c = next(c for c in R.CONTRACT_CASES if c.nao == 13 and c.lengths == (2, 0, 1))
    Z, u, f1, vk0 = R.contract_inputs(c)
    ni, nset = sum(c.lengths), len(c.lengths)
    zb, zv = nan_view(torch, Z)
    ub, uv = nan_view(torch, u)
    fb, fv = nan_view(torch, f1)
    n = nset * c.nao * c.nao
    ob, ov = out_view(torch, n)
    before = ob.cpu().numpy()
    ma, mp = L.iarr(c.mesh)
    good = R.segments(c.lengths)
    for m0, m1, nao, nset_, seg in ((0, 0, c.nao, nset, good), (0, c.nao + 1, c.nao, nset, good),
                                    (0, 1, 0, nset, good), (0, 1, c.nao, 0, good),
                                    (3, 2, c.nao, nset, good), (0, 1, c.nao, nset, [1, 2, 2, 3]),
                                    (0, 1, c.nao, nset, [0, 2, 1, 3]),
                                    (0, 1, c.nao, nset, [0, 2, 2, 4]), (0, 1, c.nao, nset, None)):
        sa, sp = L.iarr(seg) if seg is not None else (None, None)
        rc = ctx.lib.fisdf_exx_contract_lr(ctx.h, L.ptr(zv), L.ptr(uv), L.ptr(fv), mp, None, m0, m1,
                                           nao, ni, sp, nset_, 1.0, L.ptr(ov))
        assert rc < 0 and ctx.lib.fisdf_last_error(ctx.h), (m0, m1, nao, nset_, seg)
    ctx.call("fisdf_sync")
    assert np.array_equal(ob.cpu().numpy(), before)


# ---- fisdf_get_k_fft_lr ---------------------------------------------------------------------------
def call_get_k(env, c, work, fill=None, ranks=None, rmax=None, mesh=None, f=None, null_a=False):
    """One call on fresh NaN / sentinel buffers: (rc, output buffer, view, n)."""
    torch, L, ctx = env
    b = c.base
    f0, A, B, rk, kpts, kband, fband = R.getk_inputs(c)
    f = f0 if f is None else f
    nk, ngrid, nao = f.shape
    fb, fv, ks = f_view(torch, f)
    Ab, Av = nan_view(torch, A)
    Bb, Bv = nan_view(torch, B)
    no = nk if kband is None else len(kband)
    n = b.nset * no * nao * nao
    ob, ov = out_view(torch, n, fill)
    kma, kmp = L.iarr(b.kmesh)
    ma, mp = L.iarr(b.mesh if mesh is None else mesh)
    aa, ap = L.darr(K.LATTICE.ravel())
    ra, rp = L.iarr(np.asarray(rk if ranks is None else ranks).ravel())
    if fband is not None:
        bb, bv = nan_view(torch, fband)
        kb_c, kb_p = L.darr(np.asarray(kband).ravel())
        band_args = (L.ptr(bv), kb_p, len(kband))
    else:
        band_args = (None, None, 0)
    rc = ctx.lib.fisdf_get_k_fft_lr(ctx.h, L.ptr(fv), ks, kmp, mp, ap, nao,
                                    None if null_a else L.ptr(Av), L.ptr(Bv), rp,
                                    A.shape[-1] if rmax is None else rmax, b.nset, float(b.omega),
                                    *band_args, int(work), L.ptr(ov))
    ctx.call("fisdf_sync")
    return rc, ob, ov, n


@pytest.mark.parametrize("c", R.GETK_CASES, ids=R.getk_id)
def test_get_k_fft_lr(env, c):
    torch, L, ctx = env
    b = c.base
    f, A, B, ranks, kpts, kband, fband = R.getk_inputs(c)
    ref, err64 = R.getk_refs(c)
    nk, ngrid, nao = f.shape
    ctx.call("fisdf_set_omega", 0.123)        # the context's own setting is not what is used
    runs = []
    for work in R.getk_budgets(c) + [0]:      # mc = 1, a partial last chunk, all, and a repeat
        rc, ob, ov, n = call_get_k(env, c, work)
        assert rc == 0, ctx.lib.fisdf_last_error(ctx.h)
        assert edges_intact(ob, n)
        runs.append(ov.cpu().numpy().reshape(ref.shape))
    ctx.call("fisdf_set_omega", 0.0)
    for r in runs[1:]:                        # every budget and the repeat call: bitwise
        assert np.array_equal(r, runs[0])
    err, tol = K.rel_err(runs[0], ref), K.k_bound(err64, nk, R.imax_of(c.ranks), ngrid)
    print(f"get_k_fft_lr {R.getk_id(c)}: err {err:.2e} float64 {err64:.2e} bound {tol:.2e}")
    note("get_k_fft_lr", err, tol)
    assert err <= tol
    # a set without orbitals is exactly zero
    for s in range(b.nset):
        if not ranks[s].any():
            assert np.all(runs[0][s] == 0)
    # all-zero ranks: exact zeros over a NaN-filled d_vk
    rc, ob, ov, n = call_get_k(env, c, 0, fill=np.full(ref.size, NAN), ranks=0 * ranks)
    assert rc == 0 and edges_intact(ob, n)
    z = ov.cpu().numpy()
    assert np.all(z == 0) and not np.isnan(z).any()


def test_get_k_fft_lr_refusals(env):
    """Every refusal leaves d_vk as it was, bitwise."""
    torch, L, ctx = env
    c = R.GETK_CASES[1]
    f, A, B, ranks, kpts, kband, fband = R.getk_inputs(c)
    nk, ngrid, nao = f.shape
    row = 16 * R.imax_of(c.ranks) * ngrid
    over, under = ranks.copy(), ranks.copy()
    over[1, 1], under[0, 0] = A.shape[-1] + 1, -1
    calls = [
        (dict(work=0, ranks=over), b"rank"),
        (dict(work=0, ranks=under), b"rank"),
        (dict(work=0, rmax=0), b"rmax"),
        (dict(work=0, null_a=True), b"null"),
        (dict(work=row - 1), b"work_bytes"),
    ]
    for kw, word in calls:
        rc, ob, ov, n = call_get_k(env, c, **kw)
        assert rc < 0 and word in ctx.lib.fisdf_last_error(ctx.h), ctx.lib.fisdf_last_error(ctx.h)
        assert np.all(ob.cpu().numpy() == K.SENTINEL)
    # a mesh fft3d refuses (17 has no radix): refused at the first transform, d_vk unwritten
    mesh = K.REFUSED_MESH
    rng = np.random.default_rng(17)
    fr = K.F.rnd(rng, nk, int(np.prod(mesh)), nao)
    rc, ob, ov, n = call_get_k(env, c, 0, mesh=mesh, f=fr)
    assert rc < 0 and b"fft" in ctx.lib.fisdf_last_error(ctx.h)
    assert np.all(ob.cpu().numpy() == K.SENTINEL)


# ---- through ISDF ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def built(name):
    """A GPU build of the case, once per file."""
    from fisdf import ISDF
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    df = ISDF(cell, cell.get_kpts(kmesh), m0=list(m0), c0=c0)
    df.build()
    return df


@functools.lru_cache(maxsize=None)
def exact(name, which="lowrank", omega=0.0):
    """The reference K of the rank-2 dm ("lowrank") or the case's own full-rank dm ("full")."""
    from oracle.exact_ref import exact_k
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    kpts = K.mesh_kpts(cell.a, kmesh)
    if which == "lowrank":
        dm = R.e2e_dm(name, chi.shape[0], chi.shape[2])
    if omega:
        return K.exact_k64(chi, chi, kpts, kpts, dm, cell.a, cell.mesh, omega)
    return exact_k(chi, dm, cell.a, cell.mesh, kpts, coords)


class form:
    """ISDF.k_method / k_form / j_method set for a block on the shared built object, then put
    back."""

    def __init__(self, df, k_form, k="fft", j="isdf"):
        self.df, self.new = df, (k, k_form, j)

    def __enter__(self):
        self.old = (self.df.k_method, self.df.k_form, self.df.j_method)
        self.df.k_method, self.df.k_form, self.df.j_method = self.new
        self.df.k_form_used = None
        return self.df

    def __exit__(self, *exc):
        self.df.k_method, self.df.k_form, self.df.j_method = self.old


@pytest.mark.parametrize("name", R.E2E_CASES)
def test_lowrank_end_to_end(name):
    from fisdf import tag_array
    cell, kmesh, m0, c0, x0, coords, chi, dm_full = inputs(name)
    df = built(name)
    nk, nao = chi.shape[0], chi.shape[2]
    Cm, occ = R.e2e_orbitals(name, nk, nao)
    dm = R.e2e_dm(name, nk, nao)
    ref = exact(name)
    with form(df, "lowrank"):
        _, vk = df.get_jk(dm, with_j=False)
        assert df.k_form_used == "lowrank"
        _, vk_t = df.get_jk(tag_array(dm, mo_coeff=Cm[None], mo_occ=occ[None]), with_j=False)
        assert df.k_form_used == "lowrank"
    with form(df, "auto"):
        _, vk_a = df.get_jk(dm, with_j=False)
        assert df.k_form_used == "lowrank"
    with form(df, "dm"):
        _, vk_d = df.get_jk(dm, with_j=False)
        assert df.k_form_used == "dm"
    assert vk.shape == dm.shape
    for what, v in (("svd", vk), ("tagged", vk_t), ("auto", vk_a), ("dm form", vk_d)):
        e = abs(v - ref).max()
        print(f"{name} rank {R.E2E_NOCC}, {what}: |K - K_exact| {e:.2e} (max|K| {abs(ref).max():.3f})")
        note("through_isdf", e, K.JK_TOL)
        assert e < K.JK_TOL
    assert np.array_equal(vk, vk_a)
    # a Hermitian dm gives a Hermitian K, with no symmetrisation in the code
    assert abs(dm - dm.conj().swapaxes(-1, -2)).max() < 1e-12
    assert abs(vk - vk.conj().swapaxes(-1, -2)).max() <= 1e-12
    assert abs(vk_t - vk_t.conj().swapaxes(-1, -2)).max() <= 1e-12


@pytest.mark.parametrize("name", R.E2E_CASES)
def test_full_rank_dm(name):
    """The case's own full-rank dm: "auto" is the dm form, bitwise; "lowrank" still exact."""
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    df = built(name)
    with form(df, "dm"):
        vj, vk_d = df.get_jk(dm)
    with form(df, "auto"):
        vj_a, vk_a = df.get_jk(dm)
        assert df.k_form_used == "dm"
    with form(df, "lowrank"):
        vj_l, vk_l = df.get_jk(dm)
        assert df.k_form_used == "lowrank"
    assert np.array_equal(vk_a, vk_d)
    assert np.array_equal(vj, vj_a) and np.array_equal(vj, vj_l)     # the J path is untouched
    e = abs(vk_l - exact(name, "full")).max()
    print(f"{name} full rank, lowrank: |K - K_exact| {e:.2e}")
    note("through_isdf", e, K.JK_TOL)
    assert e < K.JK_TOL


NAME = "toy222"


def test_two_sets_and_general_dm():
    """nset = 2 with one non-Hermitian dm, hermi = 0."""
    from oracle.exact_ref import exact_k
    name = "toy331_fr"
    cell, kmesh, m0, c0, x0, coords, chi, dm_full = inputs(name)
    df = built(name)
    nk, nao = chi.shape[0], chi.shape[2]
    dm = R.e2e_dm(name, nk, nao)
    rng = np.random.default_rng(11)
    X, Y = K.F.rnd(rng, nk, nao, 3), K.F.rnd(rng, nk, nao, 3)
    dm2 = np.stack([dm[0], 0.1 * np.einsum("kai,kbi->kab", X, Y.conj())])
    with form(df, "lowrank", j="fft"):
        vj, vk = df.get_jk(dm2, hermi=0)
        assert df.k_form_used == "lowrank"
    assert vk.shape == dm2.shape == vj.shape
    ref = exact_k(chi, dm2, cell.a, cell.mesh, K.mesh_kpts(cell.a, kmesh), coords)
    err = abs(vk - ref).max()
    print(f"{name} nset 2 (one general dm of rank 3): |dK| {err:.2e}")
    note("through_isdf", err, K.JK_TOL)
    assert err < K.JK_TOL
    assert abs(vk[1] - vk[1].conj().swapaxes(-1, -2)).max() > 1e-6


def test_omega_without_refit():
    """Range-separated K with the grid J: coulG(omega) is an argument, nothing is refitted."""
    omega = 0.4
    cell, kmesh, m0, c0, x0, coords, chi, dm_full = inputs(NAME)
    df = built(NAME)
    dm = R.e2e_dm(NAME, chi.shape[0], chi.shape[2])
    df.__dict__.get("_omega_dfs", {}).pop(omega, None)
    with form(df, "lowrank", j="fft"):
        vj, vk = df.get_jk(dm, omega=omega)
        assert df.k_form_used == "lowrank"
    assert omega not in df.__dict__.get("_omega_dfs", {})
    err = abs(vk - exact(NAME, "lowrank", omega)).max()
    print(f"{NAME} omega {omega}: |dK| {err:.2e}")
    note("through_isdf", err, K.JK_TOL)
    assert err < K.JK_TOL
    assert abs(vk - exact(NAME)).max() > 1e-4           # and it is not the full kernel's K


def test_kpts_band_and_ewald():
    """Off-mesh band k-points (a block of one band point at a time) against exact_k_ref; exxdiv =
    'ewald' is the bare K plus the madelung term, and is refused off the mesh."""
    from fisdf import cell as C
    import fisdf.isdf as M
    cell, kmesh, m0, c0, x0, coords, chi, dm_full = inputs(NAME)
    df = built(NAME)
    dm = R.e2e_dm(NAME, chi.shape[0], chi.shape[2])
    rng = np.random.default_rng(4)
    kb = rng.uniform(-0.5, 0.5, (2, 3)) @ cell.reciprocal_vectors()
    xb = C.eval_ao_band(cell, coords, kb)
    kpts = K.mesh_kpts(cell.a, kmesh)
    ref = np.asarray(K.exact_k_ref(chi, xb, kpts, kb, dm, cell.a, cell.mesh), complex)
    old = M.BAND_BLOCK_BYTES
    with form(df, "lowrank"):
        try:
            M.BAND_BLOCK_BYTES = 16 * coords.shape[0] * cell.nao_nr()    # blocks of one band point
            vj_b, vk_b = df.get_jk(dm, kpts_band=kb, with_j=False)
        finally:
            M.BAND_BLOCK_BYTES = old
        assert df.k_form_used == "lowrank"
        assert vj_b is None and vk_b.shape == (1, 2) + dm.shape[-2:]
        err = abs(vk_b - ref).max()
        print(f"{NAME} kpts_band off-mesh: |dK| {err:.2e}")
        note("through_isdf", err, K.JK_TOL)
        assert err < K.JK_TOL
        _, vk = df.get_jk(dm, with_j=False)
        sel = [5, 0, 3]
        _, vk_s = df.get_jk(dm, kpts_band=df.kpts[sel], with_j=False)
        assert np.array_equal(vk_s, vk[:, sel])
        _, vk_e = df.get_jk(dm, with_j=False, exxdiv="ewald")
        with pytest.raises(NotImplementedError):
            df.get_jk(dm, kpts_band=kb, with_j=False, exxdiv="ewald")
    S = df.get_ovlp().cpu().numpy()
    term = df.madelung() * np.einsum("kab,skbc,kcd->skad", S, dm, S)
    err = abs(vk_e - (vk + term)).max()
    print(f"{NAME} ewald: |K_ewald - (K + madelung S D S)| {err:.2e} (the term {abs(term).max():.2e})")
    assert err < K.JK_TOL and abs(term).max() > 1e-3


def test_k_form_validated_and_ignored_by_the_isdf_k():
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(NAME)
    df = built(NAME)
    assert df.k_form == "dm" and df.K_FORMS == ("dm", "lowrank", "auto")
    with form(df, "occupied"):
        with pytest.raises(ValueError):
            df.get_jk(dm)
    vj0, vk0 = df.get_jk(dm)
    for kf in ("lowrank", "auto", "occupied"):
        with form(df, kf, k="isdf"):
            vj, vk = df.get_jk(dm)
            assert df.k_form_used is None
        assert np.array_equal(vk, vk0) and np.array_equal(vj, vj0)
