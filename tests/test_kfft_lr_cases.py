"""The occupied-orbital form of the exact K on the CPU: fisdf.isdf.lowrank_factors and tag_array,
the restated plan rule of tests/kfft_lr_cases.py against fisdf_kfft_lr_plan, the reach of the case
tables through the variants that plan reports, and the references against each other.

test_lowrank_restatement_is_exact_k64 checks the references (the float64 low-rank restatement
against kfft_cases' exact_k64, the stage references against themselves) and passes without the
feature; every other test here calls the feature (lowrank_factors, tag_array, ISDF.k_form,
fisdf_kfft_lr_plan) and fails without it."""
import ctypes as C

import numpy as np
import pytest

import kfft_cases as K
import kfft_lr_cases as R

EPS = K.EPS


# ---- lowrank_factors -------------------------------------------------------------------------------
@pytest.mark.parametrize("nao", R.FACTOR_NAOS)
def test_lowrank_factors_find_the_rank(nao):
    from fisdf.isdf import lowrank_factors
    for r in R.factor_ranks(nao):
        dm, Cm, n = R.factor_dm(nao, r)
        A, B, ranks = lowrank_factors(dm)
        nk = dm.shape[0]
        assert ranks.shape == (1, nk) and ranks.dtype == np.int32
        assert np.all(ranks == r), (nao, r, ranks)
        assert A.shape == B.shape == (1, nk, nao, r)
        smax = max(np.linalg.svd(dm[k], compute_uv=False)[0] for k in range(nk))
        back = np.einsum("kai,kbi->kab", A[0], B[0].conj())
        err = abs(back - dm).max()
        print(f"nao {nao} rank {r}: |A B^H - D| {err:.2e}, nao eps sigma_max {nao * EPS * smax:.2e}")
        assert err <= nao * EPS * smax
        # the same dm as one of two sets: a set axis in, a set axis out
        A2, B2, r2 = lowrank_factors(np.stack([dm, 0.5 * dm]))
        assert r2.shape == (2, nk) and np.all(r2 == r)
        assert np.array_equal(A2[0], A[0]) and np.array_equal(B2[0], B[0])


def test_lowrank_factors_zero_general_and_tol():
    from fisdf.isdf import lowrank_factors
    A, B, ranks = lowrank_factors(np.zeros((3, 5, 5)))
    assert np.all(ranks == 0) and A.shape == (1, 3, 5, 1) and not A.any() and not B.any()
    # a non-Hermitian dm of rank 3 is reproduced; one zero k-point beside it has rank 0
    rng = np.random.default_rng(3)
    X, Y = K.F.rnd(rng, 13, 3), K.F.rnd(rng, 13, 3)
    dm = np.stack([X @ Y.conj().T, np.zeros((13, 13))])
    assert abs(dm[0] - dm[0].conj().T).max() > 1
    A, B, ranks = lowrank_factors(dm)
    assert ranks.tolist() == [[3, 0]]
    back = np.einsum("kai,kbi->kab", A[0], B[0].conj())
    assert abs(back - dm).max() <= 13 * EPS * np.linalg.svd(dm[0], compute_uv=False)[0]
    # the threshold is relative to the set's largest singular value: a looser tol drops columns
    s = np.linalg.svd(dm[0], compute_uv=False)
    loose = lowrank_factors(dm, tol=0.5 * (s[1] + s[2]) / s[0])[2]
    assert loose.tolist() == [[2, 0]]


def test_tagged_dm_gives_the_occupied_orbitals():
    from fisdf import tag_array
    from fisdf.isdf import lowrank_factors
    rng = np.random.default_rng(5)
    nk, nao, nmo = 2, 7, 7
    Cm = K.F.rnd(rng, nk, nao, nmo)
    occ = np.array([[2, 2, 0, 0, 0, 0, 0], [2, 0, 0, 1, 0, 0, 0]], float)
    dm = np.einsum("kai,ki,kbi->kab", Cm, occ, Cm.conj())
    t = tag_array(dm, mo_coeff=Cm, mo_occ=occ)
    assert isinstance(t, np.ndarray) and np.array_equal(t, dm) and t.mo_occ is occ
    assert type(np.asarray(t)) is np.ndarray
    A, B, ranks = lowrank_factors(t)
    assert ranks.tolist() == [[2, 2]]
    for k in range(nk):
        keep = occ[k] != 0
        assert np.array_equal(A[0, k], Cm[k][:, keep] * occ[k][keep])
        assert np.array_equal(B[0, k], Cm[k][:, keep])
    # with a set axis, and with a sequence per k-point as PySCF's KSCF keeps its orbitals
    t2 = tag_array(np.stack([dm, dm]), mo_coeff=[list(Cm), list(Cm)], mo_occ=[list(occ), occ[::-1]])
    A2, B2, r2 = lowrank_factors(t2)
    assert r2.tolist() == [[2, 2], [2, 2]] and np.array_equal(A2[0], A[0])
    assert np.array_equal(B2[1, 0], Cm[0][:, occ[1] != 0])
    # the tags are trusted: the array itself is not read
    A3, B3, r3 = lowrank_factors(tag_array(np.zeros_like(dm), mo_coeff=Cm, mo_occ=occ))
    assert np.array_equal(A3, A) and np.array_equal(r3, ranks)


def test_k_form_is_declared():
    from fisdf import ISDF
    assert ISDF.K_FORMS == ("dm", "lowrank", "auto") and ISDF.k_form == "dm"
    assert ISDF.k_rank_tol is None and ISDF.k_form_used is None


# ---- the plan ----------------------------------------------------------------------------------------
def lib_plan(lib, nao, ngrid, nset, imax, work):
    mc, nch, rl, nr, tw, sc, nn = (C.c_int() for _ in range(7))
    row, tot = C.c_long(), C.c_long()
    rc = lib.fisdf_kfft_lr_plan(nao, ngrid, nset, imax, work, C.byref(mc), C.byref(nch),
                                C.byref(rl), C.byref(nr), C.byref(tw), C.byref(sc), C.byref(nn),
                                C.byref(row), C.byref(tot))
    assert rc == 0
    return R.LrPlan(mc.value, nch.value, rl.value, nr.value, tw.value, sc.value, nn.value,
                    row.value, tot.value)


def test_plan_rule_matches_library():
    from fisdf import _lib
    lib = _lib.load()
    n = 0
    for nao in (1, 3, 13, 26, 33, 76, 130):
        for ngrid in (1, 63, 64, 65, 512, 1728, 46656):
            for nset in (1, 2, 3, 5):
                for imax in (1, 4, 8, 9, 26, 70):
                    for work in R.budget_ladder(nao, ngrid, imax):
                        got = lib_plan(lib, nao, ngrid, nset, imax, work)
                        want = R.plan(nao, ngrid, nset, imax, work)
                        assert got == want, (nao, ngrid, nset, imax, work, got, want)
                        n += 1
    assert n > 8000
    assert lib_plan(lib, K.MAX_NAO, 2 ** 31 - 1, K.MAX_SETS, K.MAX_NAO, 0) == R.plan(
        K.MAX_NAO, 2 ** 31 - 1, K.MAX_SETS, K.MAX_NAO, 0)
    for bad in ((0, 512, 1, 1, 0), (K.MAX_NAO + 1, 512, 1, 1, 0), (3, 512, K.MAX_SETS + 1, 1, 0),
                (3, 2 ** 31, 1, 1, 0), (3, 512, 1, 0, 0), (3, 512, 1, K.MAX_NAO + 1, 0),
                (3, 512, 0, 1, 0), (3, 512, 1, 1, -1)):
        assert lib.fisdf_kfft_lr_plan(*bad, *([None] * 9)) < 0


def test_plan_edges():
    """The edges of the rule by hand, asked of the library (and of the restated rule beside it)."""
    from fisdf import _lib
    lib = _lib.load()

    def plan(*a):
        got = lib_plan(lib, *a)
        assert got == R.plan(*a), (a, got)
        return got

    row = 16 * 4 * 512
    assert plan(13, 512, 1, 4, row - 1).mc == 0                 # one byte short of a row m
    assert plan(13, 512, 1, 4, row)[:2] == (1, 13)
    assert plan(13, 512, 1, 4, 2 * row + 5)[:2] == (2, 7)       # a partial last chunk
    assert plan(13, 512, 1, 4, 10 ** 12)[:2] == (13, 1)         # capped at nao
    # C3 at rank 4: 4 transform rows per m where the dm form has 26
    assert plan(26, 46656, 1, 4, 0).row_bytes * 26 == K.plan(26, 46656, 1).row_bytes * 4
    assert {plan(3, 64, s, 1, 0).exx_sc for s in (1, 2, 3)} == set(R.EXX_SCS)
    assert {plan(3, 64, 1, i, 0).pair_tw for i in (8, 9)} == set(R.PAIR_TWS)


def test_tables_reach_every_path():
    """The case tables against the variants that the library's plan reports for them."""
    from fisdf import _lib
    lib = _lib.load()
    assert {lib_plan(lib, 3, 64, 1, i, 0).pair_tw for i in R.PAIR_NIS} == set(R.PAIR_TWS)
    # the contraction: every (sets per launch, n-tiles) instantiation, both launch widths inside
    # one call, more than one column group, empty segments first and in the middle
    inst = set()
    for c in R.CONTRACT_CASES:
        nset = len(c.lengths)
        for s0 in range(0, nset, R.LR_SET_CHUNK):
            p = lib_plan(lib, c.nao, 64, min(R.LR_SET_CHUNK, nset - s0), sum(c.lengths), 0)
            inst.add((p.exx_sc, p.exx_nn))
    assert inst == {(sc, nn) for sc in R.EXX_SCS for nn in K.EXX_NNS}
    assert any(len(c.lengths) > 2 * R.LR_SET_CHUNK for c in R.CONTRACT_CASES)
    assert any(c.nao > 4 * K.EXX_NT for c in R.CONTRACT_CASES)
    assert any(c.lengths[0] == 0 for c in R.CONTRACT_CASES)
    assert any(0 in c.lengths[1:-1] for c in R.CONTRACT_CASES)
    assert any(sum(c.lengths) % 4 for c in R.CONTRACT_CASES) and any(33 in c.lengths
                                                                     for c in R.CONTRACT_CASES)
    assert any(c.nao % (R.LR_ROWS // sc) for c in R.CONTRACT_CASES for sc in R.EXX_SCS)
    splits = [K.grid_split(int(np.prod(c.mesh))) + (int(np.prod(c.mesh)),) for c in R.CONTRACT_CASES]
    assert any(g % rl for rl, nr, g in splits)                            # a partial last run
    assert any(rl > K.GT for rl, nr, g in splits)                         # more than one tile a run
    for m in K.CONTRACT_MESHES:
        assert {c.kd_kind for c in R.CONTRACT_CASES if c.mesh == m} == set(K.KD_KINDS)
        assert {c.lengths for c in R.CONTRACT_CASES if c.mesh == m} == set(R.SEG_TABLES)
    # get_k: the dm form's shapes; mc = 1, a partial last chunk, all; the rank tables' edges
    assert [c.base for c in R.GETK_CASES] == K.GETK_CASES
    for c in R.GETK_CASES:
        b, ranks = c.base, np.asarray(c.ranks)
        ngrid, nk = int(np.prod(b.mesh)), int(np.prod(b.kmesh))
        assert ranks.shape == (b.nset, nk) and ranks.max() <= b.nao
        mcs = [lib_plan(lib, b.nao, ngrid, b.nset, R.imax_of(c.ranks), w).mc
               for w in R.getk_budgets(c)]
        assert mcs == [1, 2, b.nao] and b.nao % 2
    tabs = [np.asarray(c.ranks) for c in R.GETK_CASES]
    assert any(t.shape[1] > 1 and not t[:, 0].any() for t in tabs)        # nothing at k2 = 0
    assert any(t.shape[0] > 1 and not t[1].any() and t[0].any() for t in tabs)   # an empty set
    assert any(not t[:, 1:-1].sum(axis=0).all() for t in tabs if t.shape[1] > 2)
    assert any(len(set(t.ravel())) > 2 for t in tabs)


# ---- the references ----------------------------------------------------------------------------------
def test_lowrank_restatement_is_exact_k64():
    """The float64 restatement of the three low-rank lines equals exact_k64 on D = A B^H, and the
    stage references agree with themselves.  This test compares references with references and
    touches nothing of the feature: it is the one test of this file that passes without it."""
    for c in R.GETK_CASES:
        b = c.base
        f, A, B, ranks, kpts, kband, fband = R.getk_inputs(c)
        fo, ko = (f if fband is None else fband), (kpts if kband is None else kband)
        D = R.dm_of(A, B, ranks, wide=False)
        a = K.exact_k64(f, fo, kpts, ko, D, K.LATTICE, b.mesh, b.omega)
        m = R.exact_k_lr64(f, fo, kpts, ko, A, B, ranks, K.LATTICE, b.mesh, b.omega)
        err = abs(a - m).max() / abs(a).max()
        print(f"{R.getk_id(c)}: low-rank restatement against exact_k64 {err:.2e}")
        assert err <= 1e-13
    c = R.GETK_CASES[3]
    ref, err64 = R.getk_refs(c)
    assert ref.dtype == K.CLD and 0 < err64 < 1e-13
    # the stage references: float64 against long double, one set against the sum of its segments
    c = next(c for c in R.CONTRACT_CASES if c.nao == 13 and c.lengths == (2, 0, 1))
    Z, u, f1, vk0 = R.contract_inputs(c)
    seg = R.segments(c.lengths)
    kd = R.contract_kd(c)
    a = R.contract_ref(Z, u, f1, c.mesh, kd, 0, c.nao, seg, 0.5)
    b = R.contract_ref(Z, u, f1, c.mesh, kd, 0, c.nao, seg, 0.5, wide=False)
    assert 0 < K.rel_err(b, a) < 1e-13 and not a[1].any()
    # one set over all of I is the dm form's contraction with nao = I rows per m
    ni = sum(c.lengths)
    one = R.contract_ref(Z, u, f1, c.mesh, kd, 0, c.nao, [0, ni], 0.5)
    assert K.rel_err(a.sum(axis=0), one[0]) < 1e-17
    # rows of a range are the rows of the whole
    part = R.contract_ref(Z[ni:2 * ni], u, f1, c.mesh, kd, 1, 2, seg, 0.5)
    assert np.array_equal(part[:, 0], a[:, 1])
    pc = R.PAIR_CASES[5]
    f1, psi = R.pair_inputs(pc, 3)
    P = R.pair_ref(f1, psi[:, :3], 0, pc.nao)
    assert P.shape == (pc.nao * 3, pc.ngrid)
    assert P[1 * 3 + 2, 7] == np.conj(K.CLD(f1[7, 1])) * K.CLD(psi[7, 2])
