"""CPU checks of tests/ao_cases.py and, through it, of the host restatement fisdf.cell: the
independent real solid harmonics are orthonormal on the sphere and follow the stated convention;
cell._real_sph (and with it pp_cases.solid_harmonics, the harmonics of the GTH projector
references) equals them for every (l, m); cell._radial_norm equals the long-double normalisation;
the host lattice sums (eval_ao_folded / eval_ao_kpts / eval_ao_band) equal the long-double sum on
the real-cell cases within factor_cases.bound; the case tables of test_gpu_ao_variants.py reach
every item they are meant to reach; no case has a (point, atom, T) triple near the cutoff."""
import itertools

import numpy as np
import pytest

import ao_cases as A
import kmesh_cases as K
from ao_cases import CLD, EPS, LD

LEPS = float(np.finfo(LD).eps)


def _points(n, seed=3, scale=2.0):
    return np.random.default_rng(seed).standard_normal((n, 3)) * scale


# ---- the independent harmonics -----------------------------------------------------------------
def test_pi_literal_and_gamma():
    assert abs(A.PI - 4 * np.arctan(LD(1))) <= 2 * LEPS * 4
    # Gamma(3/2) = sqrt(pi) / 2, and the recurrence Gamma(x + 1) = x Gamma(x)
    assert abs(A.gamma_half(0) - np.sqrt(A.PI) / 2) <= 2 * LEPS
    for l in range(3):
        assert abs(A.gamma_half(l + 1) / A.gamma_half(l) - (LD(2 * l + 3) / 2)) <= 4 * LEPS


def test_harmonics_are_orthonormal_on_the_sphere():
    """Gauss-Legendre in cos(theta) (8 nodes: exact to degree 15) times 16 uniform phi (exact for
    |m| < 16): exact for the degree-6 products of l, l' <= 3."""
    x, w = np.polynomial.legendre.leggauss(8)
    # the float64 nodes polished by Newton steps on P_8 in long double, weights 2/((1-x^2) P_8'^2)
    x = np.asarray(x, LD)
    for _ in range(3):
        p0, p1 = np.ones_like(x), x
        for n in range(1, 8):
            p0, p1 = p1, ((2 * n + 1) * x * p1 - n * p0) / (n + 1)
        dp = 8 * (x * p1 - p0) / (x * x - 1)
        x = x - p1 / dp
    w = 2 / ((1 - x * x) * dp * dp)
    nphi = 16
    phi = 2 * A.PI * np.arange(nphi).astype(LD) / nphi
    ct, ph = np.meshgrid(x, phi, indexing="ij")
    st = np.sqrt(1 - ct * ct)
    X, Y, Z = (st * np.cos(ph)).ravel(), (st * np.sin(ph)).ravel(), ct.ravel()
    W = (w[:, None] * np.full(nphi, 2 * A.PI / nphi)[None]).ravel()
    S = np.asarray([g for l in range(4) for g in A.sph(l, X, Y, Z)])
    assert S.shape == (16, 8 * nphi)
    gram = (S * W) @ S.T
    err = float(np.abs(gram - np.eye(16, dtype=LD)).max())
    print(f"orthonormality of the independent harmonics: {err:.2e}")
    assert err <= 64 * LEPS          # 128-term sums of terms below 1, in long double


def test_harmonics_follow_the_convention():
    """An explicit monomial form for one component of every l: sign, m order and (for l = 1) the
    (x, y, z) exception; the prefactors from closed forms."""
    p = _points(20).astype(LD)
    x, y, z = p.T
    r2 = x * x + y * y + z * z
    pi = A.PI
    want = {
        (0, 0): np.full_like(x, 1 / (2 * np.sqrt(pi))),
        (1, 0): np.sqrt(3 / (4 * pi)) * x, (1, 1): np.sqrt(3 / (4 * pi)) * y,
        (1, 2): np.sqrt(3 / (4 * pi)) * z,
        (2, 0): np.sqrt(LD(15) / (4 * pi)) * x * y,                      # m = -2
        (2, 2): np.sqrt(LD(5) / (16 * pi)) * (3 * z * z - r2),           # m = 0
        (2, 4): np.sqrt(LD(15) / (16 * pi)) * (x * x - y * y),           # m = +2
        (3, 0): np.sqrt(LD(35) / (32 * pi)) * (3 * x * x * y - y ** 3),  # m = -3
        (3, 3): np.sqrt(LD(7) / (16 * pi)) * z * (5 * z * z - 3 * r2),   # m = 0
        (3, 4): np.sqrt(LD(21) / (32 * pi)) * x * (5 * z * z - r2),      # m = +1
        (3, 6): np.sqrt(LD(35) / (32 * pi)) * (x ** 3 - 3 * x * y * y),  # m = +3, positive
    }
    for (l, j), ref in want.items():
        got = A.sph(l, x, y, z)[j]
        assert np.abs(got - ref).max() <= 32 * LEPS * np.abs(ref).max(), (l, j)
    assert [A.m_order(l) for l in range(4)] == [[0], [1, -1, 0], [-2, -1, 0, 1, 2],
                                                [-3, -2, -1, 0, 1, 2, 3]]


@pytest.mark.parametrize("l", range(4))
def test_host_harmonics_equal_the_independent_ones(l):
    """cell._real_sph and pp_cases.solid_harmonics, every m, at random points: a float64
    polynomial of at most 4 terms of degree l, so (4 + l) roundings and the constant's."""
    from fisdf.cell import _real_sph
    import pp_cases as P
    p = _points(200)
    ref = A.sph(l, p[:, 0], p[:, 1], p[:, 2])
    host = _real_sph(l, p[:, 0], p[:, 1], p[:, 2])
    pp = P.solid_harmonics(l, p)
    wide = P.solid_harmonics(l, p.astype(LD))        # float64 constants, long-double polynomial
    assert len(host) == len(pp) == len(ref) == 2 * l + 1
    tol = 4 * (5 + l) * EPS
    for j in range(2 * l + 1):
        s = float(np.abs(ref[j]).max())
        e1 = float(np.abs(np.asarray(host[j], LD) - ref[j]).max()) / s
        e2 = float(np.abs(np.asarray(pp[j], LD) - ref[j]).max()) / s
        e3 = float(np.abs(np.asarray(wide[j], LD) - ref[j]).max()) / s
        print(f"l {l} component {j}: cell {e1:.2e} pp {e2:.2e} pp in long double {e3:.2e}")
        assert max(e1, e2) <= tol and e3 <= 2 * EPS, (l, j)


def test_host_radial_norm_equals_the_long_double_one():
    from fisdf import cell as C
    n = 0
    for key, shells in C.BASIS.items():
        for (l, exps, coefs) in shells:
            ref = A.radial_norm(l, exps, coefs)
            got = C._radial_norm(l, exps, coefs)
            assert np.abs(np.asarray(got, LD) - ref).max() <= 8 * len(exps) * EPS * np.abs(ref).max()
            n += 1
    assert n >= 20
    # and the definition itself, by quadrature on a fine radial grid (l = 2, two primitives)
    l, e, c = 2, [1.3, 0.4], [0.7, -0.2]
    cn = A.radial_norm(l, e, c)
    r = np.linspace(0, 14, 140001).astype(LD)
    f = r ** 2 * (r ** l * (cn[0] * np.exp(-LD(e[0]) * r * r) + cn[1] * np.exp(-LD(e[1]) * r * r))) ** 2
    h = r[1] - r[0]
    simpson = h / 3 * (f[0] + f[-1] + 4 * f[1:-1:2].sum() + 2 * f[2:-1:2].sum())
    assert abs(simpson - 1) < 1e-12          # Simpson's h^4 error at h = 1e-4


# ---- the host lattice sums ---------------------------------------------------------------------
@pytest.mark.parametrize("c", A.REAL_CASES, ids=A.case_id)
def test_host_lattice_sums_equal_the_long_double_sum(c):
    from fisdf import cell as C
    d = A.real_data(c.name)
    cell = A.real_cell(c.cell, c.mesh)
    assert A.nao_of(d.tab) == cell.nao_nr()
    if c.kmesh is None:
        got = C.eval_ao_band(cell, d.coords, d.kband)
    else:
        got = C.eval_ao_kpts(cell, d.coords, c.kmesh)
        F = C.eval_ao_folded(cell, d.coords, c.kmesh)
        ef = A.col_err(F, d.F)
        assert np.all(ef <= [A.bound(e, d.nsum) for e in d.F_err64]), c.name
        # the mesh's k-points are those of the cell
        assert np.allclose(A.mesh_kpts(d.tab.a, c.kmesh), cell.get_kpts(c.kmesh), atol=1e-14)
    err = A.col_err(got, d.ref)
    tol = np.asarray([A.bound(e, d.nsum) for e in d.err64])
    worst = int(np.argmax(err / tol))
    print(f"{c.name}: host error {err[worst]:.2e} bound {tol[worst]:.2e} (column {worst}); "
          f"float64 restatement {d.err64.max():.2e}")
    assert np.all(err <= tol), c.name


def test_band_mode_on_the_mesh_equals_the_kmesh_sum():
    b, k = (A.raw_data(n) for n in A.BAND_MESH_PAIR)
    assert np.array_equal(b.tab.tn, k.tab.tn) and np.array_equal(b.coords, k.coords)
    # exp(i k . T) with float64 k and T against the integer-reduced phase: |k . T| eps
    assert np.all(A.col_err(b.ref, k.ref) <= 64 * EPS)


# ---- the tables --------------------------------------------------------------------------------
def test_tables_reach_every_item():
    raw, cases = A.RAW_BY_NAME, A.RAW_CASES
    labels = set()
    for c in cases:
        tab = A.raw_tables(c.shells, c.tn, c.rcut)
        if c.ng and len(tab.tn) and not A.expect_zero(c):
            labels |= {(l, m) for _, l, m in A.ao_labels(tab)}
        assert len(set(tab.exps)) == len(tab.exps)          # no two AOs coincide
    for c in A.REAL_CASES:
        cell = A.real_cell(c.cell, c.mesh)
        labels |= {(s[1], m) for s in cell.shells for m in A.m_order(s[1])}
    assert labels == {(l, m) for l in range(4) for m in range(-l, l + 1)}
    nps = {int(n) for c in cases for n in A.raw_tables(c.shells, c.tn, c.rcut).sh_np}
    assert nps == {1, 2, 3, 4, 5}
    mixed = A.raw_tables("mixed", "box", A.RCUT)
    assert list(mixed.sh_l) == [3, 0, 2, 1, 0] and len(set(mixed.sh_atom)) == 2
    assert (mixed.coefs < 0).any() and (mixed.coefs > 0).any()
    # the lattice is triclinic, the atoms generic
    ln = np.linalg.norm(A.LATTICE, axis=1)
    cs = [A.LATTICE[i] @ A.LATTICE[j] / ln[i] / ln[j] for i, j in ((0, 1), (0, 2), (1, 2))]
    assert min(abs(a - b) for a, b in itertools.combinations(list(ln), 2)) > 0.1
    assert min(abs(a - b) for a, b in itertools.combinations(cs + [0.0], 2)) > 0.01
    # both DFT routes and Gamma, by the restated rule; two meshes on each route
    routes = {}
    for c in cases + A.REAL_CASES:
        if c.kmesh is not None:
            routes.setdefault(K.route(c.kmesh)[0], set()).add(tuple(c.kmesh))
    assert (1, 1, 1) in routes[K.REG] and len(routes[K.REG] - {(1, 1, 1)}) >= 2
    assert len(routes[K.LDS]) >= 2 and set(routes) == {K.REG, K.LDS}
    # translations: shuffled is a permutation whose images are not contiguous; the negative box
    # goes below zero on every axis and is no multiple of a k-mesh axis used with it
    box, shuf, neg = (A.translations(k) for k in ("box", "shuffled", "neg"))
    assert sorted(map(tuple, box)) == sorted(map(tuple, shuf)) and not np.array_equal(box, shuf)
    for km in ((2, 2, 2), (1, 1, 3)):
        img = A.image_of(shuf, km)
        assert (np.diff(img) != 0).sum() > K.nk_of(km)
    assert (neg.min(axis=0) < 0).all() and (neg.min(axis=0) < -neg.max(axis=0)).any()
    for c in cases:
        if c.tn == "neg" and c.kmesh:
            ext = neg.max(axis=0) - neg.min(axis=0) + 1
            assert any(e % n for e, n in zip(ext, c.kmesh) if n > 1)
    # the masked, all-masked, nT = 0 and ng = 0 cases, in both modes
    for band in (False, True):
        sel = [c for c in cases if (c.kmesh is None) == band]
        assert any(c.rcut == A.RCUT_MASKED for c in sel) and any(c.rcut == A.RCUT_NONE for c in sel)
        assert any(c.tn == "none" for c in sel) and any(c.ng == 0 for c in sel)
        assert any(c.ng == 1 for c in sel)
        # both sides of the 256-thread boundary
        sizes = {c.ng * A.nao_of(A.raw_tables(c.shells, c.tn, c.rcut)) for c in sel}
        assert any(s % A.BLOCK == A.BLOCK - 1 for s in sizes) and any(s % A.BLOCK == 1 for s in sizes)
    for name in ("masked_222", "band_masked_off3"):
        d = A.raw_data(name)
        near, inside, total = A.near_cutoff(d.tab, d.coords)
        assert 0 < inside < 0.01 * total                      # most masked, some in range
        assert (np.abs(d.ref).max(axis=(0, 1)) > 0).all()     # and every AO column is reached
    for name in ("allmasked_312", "band_allmasked_off1"):
        d = A.raw_data(name)
        assert A.near_cutoff(d.tab, d.coords)[1] == 0 and not d.ref.any()
    # band mode: nkb 1 and 3, Gamma among the off-mesh points, nT 0 / 1 / many, nkb above and
    # below the number of images (one per translation)
    band = [c for c in cases if c.kmesh is None]
    nkb_nt = {(len(A.band_kpts(c.kband)), len(A.translations(c.tn))) for c in band}
    assert {n for n, _ in nkb_nt} == {1, 3} and {0, 1} <= {t for _, t in nkb_nt}
    assert any(n > t > 0 for n, t in nkb_nt) and any(t > 100 > n for n, t in nkb_nt)
    assert not A.band_kpts("off3")[0].any() and A.band_kpts("off3")[1:].all()
    assert raw[A.BAND_MESH_PAIR[0]].kband == "mesh" and raw[A.BAND_MESH_PAIR[1]].kmesh == A.ON_MESH
    # the real cells: s, p (toy), d (diamond), f (NiO), grid and random points, both entries
    assert {(c.cell, c.points) for c in A.REAL_CASES} == set(itertools.product(
        ("toy_cell", "diamond_cell", "nio_cell"), ("grid", "random")))
    assert {c.cell for c in A.REAL_CASES if c.kmesh is None} == {"toy_cell", "diamond_cell", "nio_cell"}
    # sizes stay small
    for c in A.REAL_CASES:
        d = A.real_data(c.name)
        assert len(d.coords) <= 200 and A.nao_of(d.tab) <= 80 and len(d.tab.tn) <= 2200


@pytest.mark.parametrize("c", A.RAW_CASES + A.REAL_CASES, ids=A.case_id)
def test_no_triple_is_near_the_cutoff(c):
    d = A.raw_data(c.name) if c in A.RAW_CASES else A.real_data(c.name)
    near, inside, total = A.near_cutoff(d.tab, d.coords)
    assert near == 0, (c.name, near)


@pytest.mark.parametrize("c", [c for c in A.RAW_CASES if c.ng and not A.expect_zero(c)],
                         ids=A.case_id)
def test_float64_restatement_is_a_sane_float64_sum(c):
    """within BOUND_FACTOR n eps of the long-double sum in every column whose largest value is
    not itself a cancellation (a column of one point may be)."""
    d = A.raw_data(c.name)
    big = np.abs(d.ref).max(axis=(0, 1)) > 0.01 * np.abs(d.ref).max()
    assert big.any() and np.all(d.err64[big] <= A.BOUND_FACTOR * d.nsum * EPS), c.name
