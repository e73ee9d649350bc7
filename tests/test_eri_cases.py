"""tests/eri_cases.py checked without a GPU: the restated plan rule against fisdf_eri_fft_plan (a
host function of the library), the reach of the case tables, and the convention of the composed
reference against the oracle's exact_eri."""
import ctypes as C

import numpy as np
import pytest

import eri_cases as E
import fft_cases as F

NGRIDS = (512, 260, 960)


@pytest.fixture(scope="module")
def lib():
    from fisdf import _lib
    return _lib.load()


def lib_plan(lib, n1, n2, n3, n4, npair, ngrid, work):
    v = [C.c_int() for _ in range(7)]
    b = C.c_long()
    rc = lib.fisdf_eri_fft_plan(n1, n2, n3, n4, npair, ngrid, work, *[C.byref(x) for x in v],
                                C.byref(b))
    assert rc == 0
    return E.Plan(*[x.value for x in v], b.value)


def test_plan_rule(lib):
    """The restated rule equals the library's over n in 1..40 (uniform and mixed), npair 1, 3, 8,
    the three ngrids and a budget ladder around every edge."""
    n = 0
    for ngrid in NGRIDS:
        for npair in (1, 3, 8):
            for k in range(1, 41):
                shapes = [(k, k, k, k)]
                if k % 7 == 0:
                    shapes += [(k, 41 - k, 3, k + 2), (2, k, k + 1, 5)]
                for s in shapes:
                    for w in E.budget_ladder(*s, npair, ngrid):
                        if w < 0:
                            continue
                        assert lib_plan(lib, *s, npair, ngrid, w) == E.plan(*s, npair, ngrid, w), \
                            (s, npair, ngrid, w)
                        n += 1
    assert n > 4000


def test_plan_refusals_and_limits(lib):
    row = 16 * 3 * 512
    p = lib_plan(lib, 2, 3, 4, 3, 2, 512, row - 1)
    assert (p.mc, p.nrow_chunks, p.bc, p.nb_chunks, p.b_once, p.bytes) == (0,) * 6
    assert p.tw == 8 and p.ksplit == E.ksplit(6, 12, 512)
    # the wider kind of row decides: n4 = 5 > n2 = 3
    assert lib_plan(lib, 2, 3, 4, 5, 2, 512, 16 * 5 * 512 - 1).mc == 0
    assert lib_plan(lib, 2, 3, 4, 5, 2, 512, 16 * 5 * 512).mc == 1
    z = [None] * 8
    for bad in ((0, 1, 1, 1, 1, 64, 0), (1, 1, 1, E.MAX_N + 1, 1, 64, 0), (1, 1, 1, 1, 0, 64, 0),
                (1, 1, 1, 1, E.MAX_PAIRS + 1, 64, 0), (1, 1, 1, 1, 1, 1 << 31, 0),
                (1, 1, 1, 1, 1, 64, -1)):
        assert lib.fisdf_eri_fft_plan(*bad, *z) < 0 and lib.fisdf_last_error(None)


def test_ksplit_does_not_see_budget_or_pairs():
    for c in E.CASES:
        ks = {E.plan(*c.sizes, npair, E.ngrid_of(c), w).ksplit
              for npair in (1, 3, 8) for w in E.budgets(c)}
        assert len(ks) == 1
    assert E.ksplit(1, 1, 260) == 1 and E.ksplit(1089, 1089, 960) == 2
    assert E.ksplit(26 * 26, 26 * 26, 36 ** 3) == 8       # the C3 shape


def test_tables_reach():
    plans = [(c, w, E.plan(*c.sizes, c.npair, E.ngrid_of(c), w)) for c in E.CASES
             for w in E.budgets(c)]
    assert all(p.mc >= 1 for _, _, p in plans)            # every budget of the tables is accepted
    assert {p.tw for _, _, p in plans} == set(E.TWS)
    assert {p.b_once for _, _, p in plans} == {0, 1}
    assert any(p.ksplit == 1 for _, _, p in plans) and any(p.ksplit >= 2 for _, _, p in plans)
    assert any(p.mc == 1 and c.sizes[0] > 1 for c, _, p in plans)
    assert any(c.sizes[0] % p.mc for c, _, p in plans)                      # partial row chunk
    assert any(not p.b_once and (c.npair * c.sizes[2]) % p.bc for c, _, p in plans)
    # a B chunk that crosses from one pair into the next, and one inside a pair
    assert any(not p.b_once and c.npair > 1 and c.sizes[2] % p.bc for c, _, p in plans)
    assert any(not p.b_once and p.bc < c.sizes[2] for c, _, p in plans)
    assert any(w == 0 for _, w, _ in plans)
    assert {c.mesh for c in E.CASES} == set(E.MESHES)
    assert {F.route(m) for m in E.MESHES} == set(E.ROUTES.values())
    assert all(F.route(m) == r for m, r in E.ROUTES.items())
    assert sorted({E.ngrid_of(c) for c in E.CASES}) == [260, 512, 960]
    for n in (1, 3, 13, 33):
        assert any(c.sizes == (n,) * 4 for c in E.CASES)
    assert any(len(set(c.sizes)) == 4 for c in E.CASES)
    assert {c.npair for c in E.CASES} == {1, 3}
    assert {c.q_kind for c in E.CASES} == set(E.KD_KINDS)
    assert {c.omega for c in E.CASES} == {0.0, 0.4}
    for mesh in E.MESHES:                                  # each mesh meets each kind of q
        assert {c.q_kind for c in E.CASES if c.mesh == mesh} == set(E.KD_KINDS)
    assert max(c.sizes[0] * c.sizes[1] * E.ngrid_of(c) for c in E.CASES) == 33 * 33 * 960
    assert not F.accepted(E.REFUSED_MESH)
    # the builder: more pairs than one launch holds, both widths, every kind of kd
    assert any(c.npair > E.PAIR34_CAP for c in E.PAIR34_CASES)
    assert {8 if c.sizes[3] <= 8 else 32 for c in E.PAIR34_CASES} == set(E.TWS)
    assert {c.q_kind for c in E.PAIR34_CASES} == set(E.KD_KINDS)
    for c in E.PAIR34_CASES:
        rr = E.row_ranges(c.npair, c.sizes[2])
        assert (0, c.npair * c.sizes[2]) in rr and all(0 <= a < b for a, b in rr)
    assert any(r0 // c.sizes[2] != (r1 - 1) // c.sizes[2] and r0 > 0
               for c in E.PAIR34_CASES for r0, r1 in E.row_ranges(c.npair, c.sizes[2]))


def test_case_kd_is_a_q():
    for c in E.CASES:
        kd = E.case_kd(c)
        if c.q_kind == "none":
            assert kd is None and not E.case_q(c).any()
        else:
            assert np.allclose(kd, E.LATTICE @ E.case_q(c), rtol=0, atol=1e-14)
            assert sum(abs(np.asarray(kd))) / 2 <= 4.19     # PAIR34_ROUNDINGS' premise
    c = next(c for c in E.CASES if c.q_kind == "irrational")
    assert np.allclose(E.case_kd(c), E.K.KD_IRRATIONAL, rtol=0, atol=1e-14)


def test_reference_matches_the_oracle():
    """The complex128 composition is oracle.exact_ref.exact_eri on a small random case: this ties
    the convention (which orbitals are conjugated, the sign of q, the index order) to the oracle's.
    The long-double composition agrees with both to what float64 costs."""
    from oracle.exact_ref import exact_eri
    from oracle.isdf_ref import get_kpts
    from fisdf.cell import cartesian_prod
    mesh, nao, kmesh = (6, 5, 4), 3, (2, 1, 2)
    ngrid = int(np.prod(mesh))
    rng = np.random.default_rng(5)
    chi = F.rnd(rng, 4, ngrid, nao)
    kpts = get_kpts(E.LATTICE, kmesh)
    # the grid of gen_uniform_grids: fftfreq fractions (wrapped around), as fft3d's phase has them
    coords = cartesian_prod([np.fft.fftfreq(n) for n in mesh]) @ E.LATTICE
    k1, k2, k3 = 1, 2, 3
    k4 = 0                                   # k1 - k2 + k3 - k4 = G on the (2, 1, 2) mesh
    ref = exact_eri(chi, E.LATTICE, mesh, kpts, coords, k1, k2, k3, k4).reshape(nao * nao, -1)
    args = (chi[k1], chi[k2], [chi[k3]], [chi[k4]], E.LATTICE, mesh, kpts[k2] - kpts[k1])
    got = E.eri64(*args)[0]
    assert abs(got - ref).max() <= 1e-12 * abs(ref).max()
    wide = E.eri_ref(*args)[0]
    assert E.rel_err(got, wide) <= 64 * ngrid * E.EPS
    # the builder's reference is the second factor of the same sum
    B = E.pair34_ref([chi[k3]], [chi[k4]], mesh, None, 0, nao, wide=False)
    p34 = (chi[k3].conj().T[:, None, :] * chi[k4].T[None, :, :]).reshape(-1, ngrid)
    assert np.array_equal(B, p34)


def test_eri_method_is_validated_before_the_device():
    from fisdf import ISDF, coul, toy_cell
    cell = toy_cell(mesh=(10, 10, 10))
    df = ISDF(cell, cell.get_kpts((2, 1, 1)))
    assert df.eri_method == "isdf" and df.ERI_METHODS == ("isdf", "fft")
    df.eri_method = "exact"
    for call in (lambda: df.get_eri(np.zeros((4, 3))), lambda: df.ao2mo(None, np.zeros((4, 3))),
                 lambda: df.get_eri_many(np.zeros((2, 3)), np.zeros((1, 2, 3)))):
        with pytest.raises(ValueError, match="eri_method"):
            call()
    # the holder without exact= and without eri_ref= still raises, and keeps its new argument
    with pytest.raises(NotImplementedError):
        coul.FFTDF(cell, exact=False).get_eri(kpts=np.zeros((4, 3)))
    assert coul.FFTDF(cell, exact=True)._exact and coul.FFTDF(cell)._isdf is None


def test_check_triples_are_the_harness_ones():
    t = E.check_triples(8)
    assert len(t) == 7 and t[-1] == (0, 0, 0) and all(0 <= k < 8 for x in t for k in x)
