"""CPU checks of tests/factor_cases.py: the restated dispatch rules equal the library's own host
functions (fisdf_factor_plan) over a sweep; the case tables of test_gpu_factor_chain.py reach every
path, panel boundary, partition shape, split and sub-batch the rules name; every generated input
has a unique pivot sequence (gap >= 1e-9 max diag at every step) and a clean stop (last pivot
>= 100 thr, residual <= thr / 100), on the long-double reference and on the float64 restatement;
the references agree with scipy / the oracle on well-conditioned examples."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.linalg

import factor_cases as F

GAP_MIN = 1e-9


def _plan_lib():
    from fisdf import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfisdf.so not built (run __graft_entry__.build())")
    return _lib.load()


def plan(lib, n, ncol=1, batch=1, work_elems=-1):
    path, nb, nblk, s0, rpt, snb = (C.c_int() for _ in range(6))
    we = C.c_long()
    cap = (n + 63) // 64
    rows = np.zeros((cap, 8), np.int32)
    rc = lib.fisdf_factor_plan(n, ncol, batch, work_elems, C.byref(path), C.byref(nb),
                               C.byref(nblk), C.byref(s0), rows.ctypes.data_as(C.POINTER(C.c_int)),
                               cap, C.byref(we), C.byref(rpt), C.byref(snb))
    assert rc == 0, lib.fisdf_last_error(None)
    assert nblk.value == cap
    return dict(path=path.value, nb=nb.value, s0=s0.value, rows=rows, work=we.value,
                sel=(rpt.value, snb.value))


def test_rules_equal_the_host_functions():
    """Every n in 1..1100 for the pchol path, the partition and the split of both right-hand-side
    kinds (ncol = n and a wide one); every n in 1..4096 (and beyond) for the selection panel."""
    lib = _plan_lib()
    big = 1 << 40
    for n in range(1, 1101):
        for ncol in (n, 520):
            p = plan(lib, n, ncol, 3, big)
            assert (p["path"], p["nb"]) == (F.pchol_path(n), F.PCHOL_NB), n
            s0, part = F.merged_partition(n)
            assert p["s0"] == s0 and [tuple(r[:3]) for r in p["rows"]] == part, n
            full = F.merged_rows(n, ncol, 3, False, big)
            low = F.merged_rows(n, ncol, 3, True, big)
            for r, f, l in zip(p["rows"], full, low):
                assert (r[3], r[4]) == (f[4], f[5]) and tuple(r[5:8]) == l[3:6], (n, ncol)
            assert p["work"] == F.split_work_elems(n, 3), n
    for n in list(range(1, 4097)) + [4097, 5000]:
        assert plan(lib, n)["sel"] == F.sel_variant(n), n
    assert plan(lib, 4097)["sel"] == (0, 0) and plan(lib, 1024)["path"] == F.BLOCKED
    assert plan(lib, 1025)["path"] == F.STEP


@pytest.mark.parametrize("n", [256, 257, 320, 600, 1030])
def test_sub_batch_rule_equals_the_host_function(n):
    """Without a workspace nothing splits; with one of exactly one matrix's largest partials every
    row runs, some in sub-batches; one element less and the plan reports a row that cannot run."""
    lib = _plan_lib()
    for ncol in (n, 70, 520):
        for we in (None, 0, F.merged_partials(n, ncol, False), F.merged_partials(n, ncol, False) - 1,
                   3 * F.merged_partials(n, ncol, False)):
            p = plan(lib, n, ncol, 3, -1 if we is None else we)
            for lower, cols in ((False, (3, 4)), (True, (6, 7))):
                want = F.merged_rows(n, ncol, 3, lower, we)
                got = [(int(r[cols[0]]), int(r[cols[1]])) for r in p["rows"]]
                assert got == [(w[4], w[5]) for w in want], (n, ncol, we, lower)
    per = F.merged_partials(n, n, False)
    assert per > 0
    assert min(r[5] for r in F.merged_rows(n, n, 3, False, per)) == 1
    assert min(r[5] for r in F.merged_rows(n, n, 3, False, per - 1)) == 0


def test_rule_examples():
    assert F.pchol_panels(33) == [(0, 32), (32, 1)] and F.pchol_panels(31) == [(0, 31)]
    assert F.merged_partition(257) == (1, [(0, 1, 1), (1, 64, 65), (65, 64, 129), (129, 64, 193),
                                           (193, 64, 257)])
    assert F.merged_partition(64) == (64, [(0, 64, 64)])
    assert F.trsm_split_k(320, 255) == 1 and F.trsm_split_k(320, 256) == 2
    assert F.trsm_split_k(64, 2048) == 16 and F.trsm_split_k(64 * 200, 2048) == 1
    assert [F.sel_variant(n) for n in (1, 1024, 1025, 2048, 2049, 3584, 3585, 4096, 4097)] == \
        [(2, 16), (2, 16), (4, 16), (4, 16), (7, 12), (7, 12), (8, 8), (8, 8), (0, 0)]


def test_tables_reach_every_path():
    cs = F.PCHOL_CASES
    assert {F.pchol_path(c.n) for c in cs} == {F.BLOCKED, F.STEP}
    assert {c.n for c in cs if F.pchol_path(c.n) == F.BLOCKED} == {1, 33, 97, 130, 1024}
    assert {c.n for c in cs if F.pchol_path(c.n) == F.STEP} == {1025}
    assert 1025 % 4 != 0                                # pchol_step: 4 rows per block
    blocked = [c for c in cs if F.pchol_path(c.n) == F.BLOCKED]
    assert {31, 32, 33} <= {c.rmax for c in blocked} and any(c.rmax == c.n > 33 for c in blocked)
    assert any(len(F.pchol_panels(c.rmax)) >= 3 for c in blocked)
    assert any(c.tol_rel > 0 for c in cs) and any(c.tol_rel < 0 for c in cs)
    assert any(c.tol_rel == 0 for c in cs) and any(c.tol_abs_rel > 0 for c in cs)
    for path in (F.BLOCKED, F.STEP):     # complex and real input, solo runs, on both paths
        ms = [m for c in cs if F.pchol_path(c.n) == path for m in c.mats if m[0] != "zero"]
        assert {m[-1] for m in ms} == {False, True}
        assert any(c.solo for c in cs if F.pchol_path(c.n) == path)
    # the mixed batch: zero, rank 1, rank-stopped, rmax-stopped
    for name in ("n130_mixed_rmax33", "n130_mixed_rmaxn"):
        c, d = F.PCHOL_BY_NAME[name], F.pchol_data(name)
        rk = [r.rank for r in d.ref]
        assert rk[0] == 0 and rk[1] == 1 and 1 < rk[2] < c.rmax and rk[3] == c.rmax, rk
    # a run that stops inside a panel, one at a panel boundary, one in the second panel
    rk = {r.rank for c in blocked for r in F.pchol_data(c.name).ref}
    assert {0, 1, 20, 31, 32, 33, 70, 97, 130} <= rk, sorted(rk)
    # selection: all four panel variants, three panels each, the last one partial
    assert {F.sel_variant(c.n) for c in F.SEL_CASES} == {(2, 16), (4, 16), (7, 12), (8, 8)}
    for c in F.SEL_CASES:
        pan = F.sel_panels(c.n, c.nip_max)
        assert len(pan) >= 3 and pan[-1][1] < pan[0][1], c
    assert {c.n for c in F.SEL_CASES} == {600, 1030, 2049, 3585}
    # merged operator: s0 in {1, middle, 63, 64}, rows with and without split, sub-batches 1 and > 1
    s0s = {F.merged_partition(n)[0] for n in F.MERGED_N}
    assert {1, 63, 64} <= s0s and any(1 < s < 63 for s in s0s)
    ks, subs = set(), set()
    for n in F.MERGED_N:
        for rhs in F.MERGED_RHS:
            lower, ncol = (True, n) if rhs == "identity" else (False, rhs)
            per = F.merged_partials(n, ncol, lower)
            for we in (3 * per, per):
                for row in F.merged_rows(n, ncol, F.MERGED_BATCH, lower, we):
                    ks.add(row[4])
                    if row[4] > 1:
                        subs.add(row[5])
    assert 1 in ks and max(ks) > 1 and 1 in subs and max(subs) > 1
    assert {r == "identity" for r in F.MERGED_RHS} == {False, True}
    # trsm_blocked: r < ldl, a partial last block, one block, several
    assert all(r <= F.TRSM_NIP for r in F.TRSM_R) and {1, 64, 65, 200} <= set(F.TRSM_R)
    assert any(r % 64 for r in F.TRSM_R if r > 64)


@pytest.mark.parametrize("name", [c.name for c in F.PCHOL_CASES])
def test_pchol_inputs_are_well_posed(name):
    c, d = F.PCHOL_BY_NAME[name], F.pchol_data(name)
    for b, (ref, g) in enumerate(zip(d.ref, d.f64)):
        for what, f in (("long double", ref), ("float64", g)):
            print(f"{name}[{b}] {what}: rank {f.rank} min gap {f.min_gap:.1e} last pivot / thr "
                  f"{f.last_pivot / f.thr if f.thr else np.inf:.1e} residual / thr "
                  f"{f.resid_after / f.thr if f.thr else 0:.1e}")
            assert f.min_gap >= GAP_MIN
            if f.rank < c.rmax:                      # stopped by the threshold
                assert f.resid_after <= f.thr / 100
                assert f.rank == 0 or f.last_pivot >= 100 * f.thr
        assert g.rank == ref.rank and np.array_equal(g.piv, ref.piv)
        assert np.isfinite(d.L_bound[b])
        if c.tol_abs_rel:
            assert d.tol_abs > 100 * c.tol_rel * ref.dmax and ref.thr == pytest.approx(d.tol_abs)
    if name == "n1":
        assert d.ref[0].rank == 1


@pytest.mark.parametrize("name", [c.name for c in F.SEL_CASES])
def test_selection_inputs_are_well_posed(name):
    c = F.SEL_BY_NAME[name]
    x2 = F.sel_input(name)
    assert np.array_equal(x2.real, x2.real.T) and not np.array_equal(x2.imag, x2.imag.T)
    ref, g = F.sel_reference(name, x2), F.sel_f64(name, x2)
    for what, f in (("long double", ref), ("float64", g)):
        print(f"{name} {what}: rank {f.rank} min gap {f.min_gap:.1e} last pivot / thr "
              f"{f.last_pivot / f.thr:.1e} residual / thr {f.resid_after / f.thr:.1e}")
        assert f.min_gap >= GAP_MIN
        if f.rank < c.nip_max:
            assert f.resid_after <= f.thr / 100 and f.last_pivot >= 100 * f.thr
    assert np.array_equal(ref.piv, g.piv)
    assert ref.rank == (10 if name == "sel600_rank10" else c.nip_max)
    if ref.rank > F.sel_variant(c.n)[1]:
        # the pivots past the first panel depend on the trailing update: without it they differ
        wrong = F.sel_f64(name, x2, skip_updates=True)
        first = int(np.argmin(np.append(wrong.piv[:ref.rank] == ref.piv[:wrong.rank], False)))
        print(f"{name}: without the trailing updates the pivots differ from step {first}")
        assert first < ref.rank


def test_chain_and_chol_fail_inputs_are_well_posed():
    d = F.chain_data()
    ranks = [r.rank for r in d.ref]
    print("chain ranks", ranks, "gaps", [f"{r.min_gap:.1e}" for r in d.ref], "bounds",
          [f"{b:.1e}" for b in d.bound])
    assert ranks == [130, 70, 40]
    for r in d.ref:
        assert r.min_gap >= GAP_MIN
        if r.rank < F.CHAIN_N:
            assert r.resid_after <= r.thr / 100 and r.last_pivot >= 100 * r.thr
    for b in range(3):
        p = d.ref[b].piv
        assert np.linalg.cond(d.A[b][np.ix_(p, p)]) < 1e6
    # the singular matrix of the unpivoted test: pivot 70 (second 64-block) is rounding only, far
    # below the threshold; every other matrix and every earlier pivot is far above it
    A = F.chol_fail_batch()
    assert F.CHOL_FAIL_AT >= 64 and np.linalg.matrix_rank(A[1]) == F.CHOL_FAIL_N - 1
    for b in range(3):
        assert np.array_equal(A[b], A[b].conj().T)
        _, piv = F.chol_f64(A[b])
        thr = F.CHOL_FAIL_TOL * A[b].diagonal().real.max()
        if b == 1:
            print(f"chol fail: pivot {piv[F.CHOL_FAIL_AT]:.1e} thr {thr:.1e}")
            assert abs(piv[F.CHOL_FAIL_AT]) <= thr / 100
            assert piv[:F.CHOL_FAIL_AT].min() >= 100 * thr
        else:
            assert piv.min() >= 100 * thr


def test_references_agree_with_scipy_and_the_oracle():
    from oracle import isdf_ref as R
    rng = np.random.default_rng(3)
    n = 60
    A = F.full_rank(n, 77)
    f = F.pchol_ld(A, n, -1.0)
    assert f.rank == n and sorted(f.piv) == list(range(n))
    Lp = f.L[f.piv]
    assert abs(np.triu(Lp, 1)).max() == 0
    ref = np.linalg.cholesky(A[np.ix_(f.piv, f.piv)])
    assert F.relerr(Lp.astype(complex), ref) < 1e-13
    assert F.relerr(F.factor_along_ld(A, f.piv), f.L) < 1e-17
    # the oracle's dpstrf on a real tie-free matrix: the same pivots
    Ar = F.low_rank(80, 30, 0.8, 78, real=True).real
    chol, perm, rank = R.pivoted_cholesky(Ar)
    fr = F.pchol_ld(Ar, 80, 1e-10)
    assert fr.rank == 30 and np.array_equal(fr.piv, perm[:30])
    g = F.greedy_f64(Ar.astype(complex), 80, 1e-10, 0.0, F.PCHOL_NB)
    gs = F.greedy_f64(Ar.astype(complex), 80, 1e-10, 0.0, None)
    assert np.array_equal(g.piv, fr.piv) and np.array_equal(gs.piv, fr.piv)
    assert F.relerr(g.L, fr.L) < 1e-9 and F.relerr(gs.L, fr.L) < 1e-9
    # substitutions vs scipy
    T = F.tri_lower(150, 79)
    B = rng.standard_normal((150, 7)) + 1j * rng.standard_normal((150, 7))
    lo = scipy.linalg.solve_triangular(T, B, lower=True)
    ad = scipy.linalg.solve_triangular(T, B, lower=True, trans="C")
    assert F.relerr(lo, F.solve_lower_ld(T, B)) < 1e-13
    assert F.relerr(ad, F.solve_adjoint_ld(T, B)) < 1e-13
    for lower, want in ((1, lo), (0, ad)):
        assert F.relerr(F.trsm_blocked_f64(T, B, lower), want) < 1e-13
    assert F.relerr(F.trsm_merged_f64(T, B), lo) < 1e-13
    L, piv = F.chol_f64(A)
    assert F.relerr(L, np.linalg.cholesky(A)) < 1e-13 and piv.min() > 0     # no NaN: all met


def test_bounds_are_small_for_the_well_conditioned_cases():
    """The per-case bounds come from float64 against long double: on the well-conditioned solves
    they stay within a few hundred eps (a bound near 1 would assert nothing)."""
    for n in (63, 257):
        for rhs in ("identity", 70):
            assert max(F.merged_data(n, rhs).bound) < 1e-11
    d = F.trsm_data(130, 0, 1, "wpp")
    assert max(d.bound[F.TRSM_NIP]) < 1e-11
    assert abs(d.L.imag).max() == 0
