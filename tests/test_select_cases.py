"""CPU checks of tests/select_cases.py: the restated selection rules equal the library's host
functions (fisdf_select_plan, fisdf_select_gram_plan) over a sweep; the case tables of
test_gpu_select_variants.py reach the paths they are named for; every pivot input has a unique
greedy sequence and a clean stop (DESIGN.md 3.3b's certificates) and depends on the updates; the
twin inputs' reference meets the twin rule; the Gram cases reach every split-K and launch count."""
import ctypes as C

import numpy as np
import pytest

import factor_cases as F
import select_cases as S

GAP_MIN = 1e-9
NCU = 256          # the case tables are held to their names on a 256-CU device


@pytest.fixture(scope="module")
def lib():
    from fisdf import _lib
    return _lib.load()


def plan(lib, n, rmax, ncu, lds_cols=0, wgs=0):
    mode, path = C.c_int(-9), C.c_int(-9)
    b, c, pn = (C.c_int * 4)(), (C.c_int * 7)(), (C.c_int * 2)()
    bl, cl = C.c_long(-9), C.c_long(-9)
    rc = lib.fisdf_select_plan(n, rmax, ncu, lds_cols, wgs, C.byref(mode), b, C.byref(bl), c,
                               C.byref(cl), pn, C.byref(path))
    assert rc == 0
    return (mode.value, S.BatchPlan(*b, bl.value), S.CoopPlan(*c, cl.value), tuple(pn), path.value)


def restated_plan(n, rmax, ncu, lds_cols=0, wgs=0):
    return (S.default_mode(rmax), S.batch_plan(n, rmax, ncu), S.coop_plan(n, rmax, ncu, lds_cols, wgs),
            F.sel_variant(n), F.pchol_path(n))


def test_plan_rules_equal_the_library(lib):
    ns = list(range(1, 4201)) + [8191, 8192, 8193, 8194]
    count = 0
    for n in ns:
        rmaxs = sorted({min(r, n) for r in (1, 16, 17, 44, 45, 63, 64, 600, 800, 1008, 1009, n)})
        for rmax in rmaxs:
            for ncu in (64, 128, 255, 256, 304):
                for lds_cols in (0, 16, 20):
                    got, want = plan(lib, n, rmax, ncu, lds_cols), restated_plan(n, rmax, ncu, lds_cols)
                    assert got == want, (n, rmax, ncu, lds_cols, got, want)
                    count += 1
    for n in (64, 150, 600, 2049, 8192):       # the grid cap
        for wgs in (1, 3, 127, 200):
            for ncu in (0, 2, 256):
                got, want = plan(lib, n, min(40, n), ncu, 0, wgs), restated_plan(n, min(40, n), ncu, 0, wgs)
                assert got == want, (n, ncu, wgs, got, want)
    print(f"{count} plans equal")
    assert lib.fisdf_select_plan(0, 1, 256, 0, 0, *([None] * 7)) != 0
    assert lib.fisdf_select_plan(8, 9, 256, 0, 0, *([None] * 7)) != 0


def test_refusal_boundaries():
    """The boundaries the cases are built around, each from the restated rules (equal to the
    library's by the sweep above)."""
    assert S.batch_plan(63, 1, NCU).why == S.B_N_SMALL and S.coop_plan(63, 1, NCU).why == S.C_N_SMALL
    assert S.batch_plan(4080, 40, NCU).ok and S.batch_plan(4081, 40, NCU).why == S.B_GRID
    assert S.batch_plan(4081, 40, 304).ok and S.batch_plan(4097, 40, 304).why == S.B_N_LARGE
    assert S.batch_plan(2000, 1008, NCU).ok and S.batch_plan(2000, 1009, NCU).why == S.B_LDS
    assert S.batch_plan(64, 44, NCU).ok and S.batch_plan(64, 45, NCU).why == S.B_SCRATCH
    assert S.coop_plan(64, 63, NCU).ok and S.coop_plan(64, 64, NCU).why == S.C_SCRATCH
    assert S.coop_plan(8192, 24, NCU).ok and S.coop_plan(8193, 24, NCU).why == S.C_ROWS
    assert S.coop_plan(600, 48, NCU, 15).why == S.C_K_SMALL
    assert S.default_mode(799) == 1 and S.default_mode(800) == 0


def test_pivot_cases_reach_their_names():
    table = []
    for c in S.PIV_CASES:
        k, G, RW, K, tpr = S.reached(c.n, c.rmax, NCU, c.mode, c.lds_cols, c.wgs)
        table.append(f"{c.name}: {S.KERNEL_NAMES[k]} G {G} RW {RW} K {K} tpr {tpr}")
        assert k == c.expect, (c.name, S.KERNEL_NAMES[k])
    print("\n".join(table))
    r = lambda name: S.reached(*[getattr(S.PIV_BY_NAME[name], f) for f in ("n", "rmax")], NCU,
                               *[getattr(S.PIV_BY_NAME[name], f) for f in ("mode", "lds_cols", "wgs")])
    assert r("c64_rw8")[1:3] == (8, 8) and r("c65_rw8_tail1")[1:3] == (9, 8) and 65 - 8 * 8 == 1
    assert r("c2048_rw16")[2::2] == (16, 32) and r("c2049_rw17")[2::2] == (17, 16)
    assert r("c4225_rw34_tpr8")[2::2] == (34, 8) and r("c8192_rw64")[1:] == (128, 64, 24, 8)
    assert r("c150_wgs3")[1:3] == (3, 50)
    for name in ("s600_k16", "s600_k20", "s2049_k16", "s2049_k20"):
        c = S.PIV_BY_NAME[name]
        assert r(name)[3] == c.lds_cols and c.rmax - c.lds_cols >= 28
    assert S.coop_plan(8192, 24, NCU).RW == S.SC_MAXRW
    # rmax = n: neither scratch fits, the panels run
    for name in ("n64_rmaxn", "n96_rmaxn"):
        c = S.PIV_BY_NAME[name]
        assert S.batch_plan(c.n, c.rmax, NCU).why == S.B_SCRATCH
        assert S.coop_plan(c.n, c.rmax, NCU).why == S.C_SCRATCH


def _certify(name, re, rmax, tol, ref=None):
    ref = ref or S.reference(re, rmax, tol)
    g = S.restated(re, rmax, tol)
    for what, f in (("long double", ref), ("float64", g)):
        print(f"{name} {what}: rank {f.rank} min gap {f.min_gap:.1e} last pivot / thr "
              f"{f.last_pivot / f.thr:.1e} residual / thr {f.resid_after / f.thr:.1e}")
        assert f.min_gap >= GAP_MIN
        if f.rank < rmax:
            assert f.resid_after <= f.thr / 100 and f.last_pivot >= 100 * f.thr
    assert g.rank == ref.rank and np.array_equal(g.piv, ref.piv)
    return ref


@pytest.mark.parametrize("name", [c.name for c in S.PIV_CASES])
def test_pivot_inputs_are_well_posed(name):
    c = S.PIV_BY_NAME[name]
    re = S.case_real(c)
    assert np.array_equal(re, re.T)
    if c.imag and 1 < c.n <= 600:
        im = S.case_imag(c)
        assert not np.array_equal(im, im.T) and not np.array_equal(im, S.case_imag(c, True))
    ref = _certify(name, re, c.rmax, c.tol)
    if c.family == "stop":
        assert ref.rank == c.k * (c.k + 1) // 2 < c.rmax and ref.rank in (10, 21)
    else:
        assert ref.rank == c.rmax
    if c.family in ("clustered", "strided"):
        rows = S.top_rows(c.family, c.n, c.seed)
        assert set(np.argsort(S.x4_of(re).diagonal())[-S.TOP:]) == set(rows)
        step = np.diff(rows) % c.n
        assert (step == (1 if c.family == "clustered" else 97)).all()
    if c.rmax <= 8:         # too few pivots for a forgotten update to show (the tiny Grams)
        return
    wrong = S.restated(re, c.rmax, c.tol, skip_updates=True)
    m = min(wrong.rank, ref.rank)
    assert wrong.rank != ref.rank or not np.array_equal(wrong.piv[:m], ref.piv[:m]), \
        "the pivots survive forgotten updates"


@pytest.mark.parametrize("name", [c.name for c in S.TWIN_CASES])
def test_twin_inputs(name):
    c = S.TWIN_BY_NAME[name]
    re = S.twin_real(c)
    assert np.array_equal(re, re.T)
    assert np.array_equal(re[c.a], re[c.b]) and np.array_equal(re[:, c.a], re[:, c.b])
    ref, expect = S.twin_reference(c)
    print(f"twin {name}: quotient min gap {ref.min_gap:.1e}, pair met at step "
          f"{int(np.argmax(expect == c.a)) if c.a in expect else None}")
    assert ref.rank == c.rmax and ref.min_gap >= GAP_MIN
    assert c.a in expect and c.b not in expect
    assert (expect[0] == c.a) == c.top
    # the reference alone, on the whole matrix (first index on ties), meets the rule
    full = S.reference(re, c.rmax, -1.0)
    assert S.twin_ok(c, full.piv, expect) and np.array_equal(full.piv, expect)
    swapped = np.where(expect == c.a, c.b, expect)
    assert S.twin_ok(c, swapped, expect) != c.top
    assert not S.twin_ok(c, np.append(expect[:-1], c.b), expect)


def gram_plan(lib, km, fold, nk, q0, q1, ng0, nao):
    info = (C.c_int * 3)()
    kmp = (C.c_int * 3)(*km) if km is not None else None
    assert lib.fisdf_select_gram_plan(kmp, fold, nk, q0, q1, ng0, nao, info) == 0
    return tuple(info)


def test_gram_cases_reach_every_split_and_launch_count(lib):
    seen = set()
    for g in S.GRAM_FOLD:
        nk = int(np.prod(g.km))
        reps, w = S.kmesh_reps(g.km)
        assert len(reps) == g.reps and sorted(set(w)) in ([1], [2], [1, 2])
        for fold, ks in ((1, g.ks_fold), (0, g.ks_all)):
            got = gram_plan(lib, g.km, fold, nk, 0, nk, g.ng0, g.nao)
            assert got == S.gram_plan(g.km, fold, nk, g.ng0, g.nao)
            assert got == ((g.reps, g.launches, ks) if fold else (nk, 1, ks)), (g, fold, got)
            seen.add(ks)
    assert seen == {1, 2, 4}
    assert max(g.launches for g in S.GRAM_FOLD) == 2
    for ng0 in S.GRAM_NG0:
        for nao in S.GRAM_NAO:
            for q0, q1 in S.GRAM_SHARDS + ((0, S.GRAM_PLAIN_NK),):
                got = gram_plan(lib, None, 0, S.GRAM_PLAIN_NK, q0, q1, ng0, nao)
                assert got == S.gram_plan(None, 0, q1 - q0, ng0, nao)
    # the fold needs the k-mesh and the whole of it; the k-mesh must have nk points
    info = (C.c_int * 3)()
    km = (C.c_int * 3)(2, 2, 2)
    assert lib.fisdf_select_gram_plan(None, 1, 8, 0, 8, 4, 1, info) != 0
    assert lib.fisdf_select_gram_plan(km, 1, 8, 0, 7, 4, 1, info) != 0
    assert lib.fisdf_select_gram_plan(km, 0, 9, 0, 9, 4, 1, info) != 0


def test_gram_symmetric_inputs_and_references():
    """On inputs with x0[-k] = conj(x0[k]) the weighted sum over the representatives is the plain
    sum over all k (in long double, to its own rounding)."""
    worst = 0.0
    for g in S.GRAM_FOLD:
        nk = int(np.prod(g.km))
        x0 = S.gram_x0(nk, g.ng0, g.nao, 300 + nk, g.km)
        for k in range(nk):
            assert np.array_equal(x0[S.kmesh_partner(k, g.km)], x0[k].conj())
        full, bound = S.gram_reference(x0)
        reps, w = S.kmesh_reps(g.km)
        folded, _ = S.gram_reference(x0, reps, w)
        d = F.relerr(folded, full)
        worst = max(worst, d / bound)
        assert d <= bound and np.isfinite(bound)
    print(f"folded against plain long-double reference: at most {worst:.2f} of the bound")


def test_bound_tie_input():
    re = S.tie_real()
    assert np.array_equal(re, re.T)
    x4 = S.x4_of(re)
    d = x4.diagonal()
    a, b = S.TIE_A, S.TIE_B
    assert d[a] == d[b] and a < b and a // 64 == 0 and b // 64 == 1
    assert set(np.argsort(d)[-4:]) == set(S.TIE_CROWD) and all(r // 64 == 0 for r in S.TIE_CROWD)
    assert np.sort(d)[-6] == d[a] and np.sort(d)[-7] < d[a]
    full = S.reference(re, S.TIE_RMAX, -1.0)
    assert set(full.piv[:4]) == set(S.TIE_CROWD) and tuple(full.piv[4:6]) == (a, b)
    # the two rows' updates are exact zeros: the tie is bit for bit whatever the path's arithmetic
    assert not full.L[a, :4].any() and not full.L[b, :5].any()
    keep = np.delete(np.arange(S.TIE_N), b)
    q = S.reference(re[np.ix_(keep, keep)], S.TIE_RMAX - 1, -1.0)
    print(f"bound tie: quotient min gap {q.min_gap:.1e}")
    assert q.min_gap >= GAP_MIN and np.array_equal(np.delete(full.piv, 5), keep[q.piv])
    g = S.restated(re, S.TIE_RMAX, -1.0)
    assert np.array_equal(g.piv, full.piv)


def test_composite_input_is_well_posed():
    x0, x4, ref = S.composite_input()
    g = F.greedy_f64(x4.astype(np.float64), S.COMP_NIP, -1.0)
    print(f"composite: rank {ref.rank} min gap {ref.min_gap:.1e} / {g.min_gap:.1e}")
    assert ref.rank == S.COMP_NIP and min(ref.min_gap, g.min_gap) >= GAP_MIN
    assert np.array_equal(g.piv, ref.piv)
    wrong = F.greedy_f64(x4.astype(np.float64), S.COMP_NIP, -1.0, 0.0, 4, True)
    assert not np.array_equal(wrong.piv, ref.piv)
