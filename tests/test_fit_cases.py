"""CPU checks of tests/fit_cases.py: the references check themselves (the long-double W_q against
the oracle's gelsy + FFT chain, the half-grid and the listed-G restatements against the full sum,
time reversal, W_s against the oracle), the case table meets the conditions that keep a case from
passing empty, and the restated host rules equal the library's own (fisdf_fit_plan,
fisdf_factor_plan is covered by test_factor_cases.py).

Only test_rules_equal_fit_plan needs the library entries this suite came with (fisdf_fit_plan);
every other test here reads no library at all and passes without fisdf_fit_report / fisdf_fit_plan.
"""
import ctypes as C
import os

import numpy as np
import pytest

import factor_cases as F
import fft_cases as FF
import fit_cases as T
from oracle import isdf_ref as R

SMALL = ["even222_wm04_n5", "mixed222_wm04_n5", "axes222_w0_n5", "k411_w0_n5", "toy222_w0_n5"]


def _plan_lib():
    from fisdf import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfisdf.so not built (run __graft_entry__.build())")
    return _lib.load()


def fit_plan(lib, kmesh, mesh, q, nq, nip):
    info = np.full(8, -9, np.int32)
    ip = C.POINTER(C.c_int)
    rc = lib.fisdf_fit_plan(np.asarray(kmesh, np.int32).ctypes.data_as(ip),
                            np.asarray(mesh, np.int32).ctypes.data_as(ip), q, nq, nip,
                            info.ctypes.data_as(ip))
    assert rc == 0, lib.fisdf_last_error(None)
    return [int(v) for v in info]


# ------------------------------------------------------------------ rules
def test_rules_equal_fit_plan(monkeypatch):
    """Self-conjugacy, m, the prefix planes and the fitted columns for every q of a sweep of
    k-meshes on meshes of both parities; the W_PP-in-the-lane threshold over nq; the W_PP split over
    nip with the environment's default, with FISDF_WPP_KSPLIT = 1, 2 and 40."""
    lib = _plan_lib()
    for var in ("FISDF_WPP_KSPLIT", "FISDF_LANE_WPP"):
        monkeypatch.delenv(var, raising=False)
    kmeshes = [(1, 1, 1), (2, 2, 2), (3, 1, 2), (4, 1, 1), (3, 2, 2), (2, 3, 4), (4, 4, 4), (1, 6, 1)]
    meshes = [(8, 12, 12), (13, 15, 15), (12, 13, 13), (6, 10, 10), (2, 64, 48), (1, 4, 4),
              (3, 5, 7)]
    for kmesh in kmeshes:
        for q in range(int(np.prod(kmesh))):
            for mesh in meshes:
                got = fit_plan(lib, kmesh, mesh, q, 1, 5)
                sc = T.self_conjugate(kmesh, q)
                m = T.self_m(kmesh, q) if sc else (0, 0, 0)
                planes = T.prefix_planes(mesh, m[0]) if sc else mesh[0]
                assert got[:6] == [int(sc), *m, planes, planes * mesh[1] * mesh[2]], (kmesh, q, mesh)
                if sc:
                    assert planes * mesh[1] * mesh[2] == T.fitted_columns(mesh, kmesh, q, True)
    for nq in range(1, 20):
        full = [5] * nq
        assert fit_plan(lib, (1, 1, 1), (8, 8, 8), 0, nq, 5)[6] == int(T.lane_wpp(nq, full, 5, T.LSTSQ))
    assert not T.lane_wpp(12, [5] * 11 + [4], 5, T.LSTSQ) and not T.lane_wpp(12, [5] * 12, 5, T.SVD)
    for env in (None, 1, 2, 40):
        if env is not None:
            monkeypatch.setenv("FISDF_WPP_KSPLIT", str(env))
        for nip in (1, 255, 256, 257, 1000):
            want = T.wpp_split(nip, T.WPP_KSPLIT_DEFAULT if env is None else env)
            assert fit_plan(lib, (1, 1, 1), (8, 8, 8), 0, 1, nip)[7] == want, (env, nip)


def test_lane_rule_examples():
    """The lane / ring rule at the points the GPU runs use (fisdf_fit_info is compared on the
    device): pipelined calls keep at most 3 lanes (2 when y arrives by marks), one q or one lane
    never pipelines, the ring is never deeper than the call."""
    assert T.fit_lanes(6, 0, -1, 0) == (2, 4) and T.fit_lanes(6, 4, 0, 0) == (4, 0)
    assert T.fit_lanes(6, 4, 1, 0) == (3, 5) and T.fit_lanes(6, 4, 1, 0, ready=True) == (2, 4)
    assert T.fit_lanes(6, 4, 0, 0, ready=True) == (3, 0) and T.fit_lanes(1, 0, -1, 0) == (1, 0)
    assert T.fit_lanes(6, 1, 1, 3) == (1, 0) and T.fit_lanes(3, 2, 1, 9) == (2, 3)


def test_pairing_is_an_involution_and_the_prefix_holds_one_member():
    """G -> -G - m is its own inverse; every pair has a member in the prefix planes and, outside a
    self-paired plane, exactly one."""
    for mesh in [c.mesh for c in T.CASES] + [(1, 4, 4), (3, 5, 7)]:
        for m in FF.HERM_M:
            pe, i0, p0 = T.partner_index(mesh, m)
            assert np.array_equal(pe[pe], np.arange(pe.size))
            nH = T.prefix_planes(mesh, m[0])
            inside, pin = i0 < nH, p0 < nH
            assert (inside | pin).all()
            assert ((inside & pin) == (i0 == p0)).all()


# ------------------------------------------------------------------ the table's conditions
def _self_q(c):
    return [(j, q) for j, q in enumerate(c.qs) if T.self_conjugate(c.kmesh, q)]


@pytest.mark.parametrize("name", [c.name for c in T.CASES + T.RANK_CASES])
def test_asymmetric_and_empty_tags(name):
    c = T.BY_NAME[name]
    assert list(c.qs) == sorted(set(c.qs)) and set(c.asym_q) | set(c.empty_q) <= set(c.qs)
    for j, q in _self_q(c):
        m = T.self_m(c.kmesh, q)
        cg = T.coulg(c.a, c.kmesh, c.mesh, q, c.omega)
        full = T.asym_full(cg, c.a, c.mesh, m)
        idx, f = T.asym_half(cg, c.a, c.mesh, m)
        assert (np.diff(full) > 0).all() and (np.diff(idx) > 0).all()
        assert np.isfinite(f).all() and (np.abs(f) <= 1).all()
        if q in c.asym_q:
            assert len(full) > 0 and len(idx) > 0, (name, q)
        if q in c.empty_q:
            assert len(full) == 0 and len(idx) == 0, (name, q)
        # the half list is the full list's prefix part, and the full list is closed under pairing
        pe, i0, _ = T.partner_index(c.mesh, m)
        assert set(full) == set(pe[full])
        assert set(idx) == {e for e in full if i0[e] < T.prefix_planes(c.mesh, m[0])}
    for q in set(c.asym_q) | set(c.empty_q):
        assert T.self_conjugate(c.kmesh, q)


def test_asymmetric_cases_carry_a_visible_imaginary_part():
    """On every q tagged asymmetric the reference's |Im W| / |W| exceeds 1000 times the bound the
    device is held to: a wrong factor, pairing or list there cannot pass.  Tagged empty: below the
    bound (the imaginary part is rounding)."""
    for c in T.CASES:
        for j, q in _self_q(c):
            ratio, bnd = T.imag_ratio(c.name, j), T.wq_bound(c.name, j)
            print(f"{c.name} q={q} m={T.self_m(c.kmesh, q)} omega={c.omega}: |Im W|/|W| "
                  f"{ratio:.2e}, bound {bnd:.2e}")
            if q in c.asym_q:
                assert ratio > 1000 * bnd, (c.name, q, ratio, bnd)
            if q in c.empty_q:
                assert ratio < bnd, (c.name, q, ratio, bnd)


def test_imaginary_part_per_omega():
    """What each omega leaves of the asymmetric part on mesh (8, 12, 12), k-mesh (2, 2, 2): 0, -0.4
    and +2.0 keep it at 1e-5 .. 1e-3, +0.4 damps it below the bound (that case tests the weights
    only, and is not tagged)."""
    for name, visible in (("even222_w0_n40", True), ("even222_wm04_n5", True),
                          ("even222_wp04_n5", False), ("even222_wp20_n5", True)):
        c = T.BY_NAME[name]
        r = [T.imag_ratio(name, j) for j in range(7)]
        print(f"omega {c.omega:+.1f}: |Im W|/|W| over q = 0..6 from {min(r):.1e} to {max(r):.1e}")
        assert (min(r) > 1e-5) if visible else (max(r) < T.wq_bound(name, 0))


def test_every_branch_is_reached():
    reached = set()
    for run in T.all_runs():
        reached |= T.run_branches(run)
    for run, env in T.split_runs():
        reached |= T.run_branches(run, T.WPP_KSPLIT_DEFAULT if env is None else env)
    assert reached == T.FIT_BRANCHES, (T.FIT_BRANCHES - reached, reached - T.FIT_BRANCHES)
    # the invariance runs reuse ring slots and cover 1, 2, 3 and 4 lanes
    inv = [T.run_lanes(r) for r in T.invariance_runs()]
    assert {nl for nl, _ in inv} == {1, 2, 3, 4}
    nq = len(T.BY_NAME[T.INVARIANCE_CASE].qs)
    assert nq == 6 and {d for _, d in inv} >= {0, 1, 2, nq}


@pytest.mark.parametrize("name", [c.name for c in T.RANK_CASES])
def test_rank_deficient_inputs_have_one_answer(name):
    """The long-double and the float64 greedy factorisations agree on rank and pivots, every
    pivot choice has a gap, the stop is clean (last pivot >= 100 thr, residual <= thr / 100)."""
    c = T.BY_NAME[name]
    x4 = T.inputs(name)[0]
    for j, r in enumerate(T.case_ranks(c)):
        if r == c.nip:
            assert np.linalg.cond(x4[j]) < 4.0 * (1 + 1e-9)
            continue
        if r == 0:
            assert not x4[j].any()
            continue
        ref = T.pchol_ref(name, j)
        f64 = F.greedy_f64(x4[j], c.nip, T.FIT_TOL, 0.0, F.PCHOL_NB)
        assert ref.rank == f64.rank == r and np.array_equal(ref.piv, f64.piv)
        assert ref.min_gap >= 1e-9 and ref.last_pivot >= 100 * ref.thr
        assert ref.resid_after <= ref.thr / 100
        assert T.NOISE * 1e3 <= T.FIT_TOL
        if T.self_conjugate(c.kmesh, c.qs[j]):
            assert not x4[j].imag.any()


# ------------------------------------------------------------------ the references
def _coords(a, mesh):
    """Grid points with the fftfreq fractions (gen_uniform_grids, wrap_around=True)."""
    f = np.stack(np.meshgrid(*[np.fft.fftfreq(n) for n in mesh], indexing="ij"), -1).reshape(-1, 3)
    return f @ a


@pytest.mark.parametrize("name", SMALL + ["gamma111_w0_n70", "k312_wm04_n40"])
def test_reference_equals_the_oracle(name):
    """The long-double W_q against oracle.isdf_ref.fit_and_coulomb (gelsy, forward and inverse FFT
    in float64): another formula for the same thing, so conventions (phase, weight, scale, which
    side is conjugated) are what this checks; cond(x4) = 4, so float64 leaves 1e-12 at the most."""
    c = T.BY_NAME[name]
    x4, y = T.inputs(name)
    coord = _coords(c.a, c.mesh)
    vol = abs(np.linalg.det(c.a))
    kpts = R.get_kpts(c.a, c.kmesh)
    for j, q in enumerate(c.qs):
        w, rank = R.fit_and_coulomb(x4[j], y[j].T, kpts[q], coord, c.a, c.mesh, vol,
                                    omega=c.omega)
        err = F.relerr(w, T.wq_ld(name, j))
        print(f"{name} q={q}: oracle against long double {err:.2e}")
        assert rank == c.nip and err < 1e-12


@pytest.mark.parametrize("name", SMALL + ["lds222_w0_n40"])
def test_half_grid_and_listed_restatements(name):
    """Re over the prefix planes with c + c' plus the signed listed term, and Re over every G plus
    the listed G's Im, both equal the plain sum over the grid: exactly up to the unlisted pairs,
    whose weights differ by less than the 1e-13 cut, so to well within ngrid eps."""
    c = T.BY_NAME[name]
    ngrid = int(np.prod(c.mesh))
    for j, q in _self_q(c):
        G = T.gram_ld(name, j)
        eh, ef = F.relerr(T.gram_half_ld(name, j), G), F.relerr(T.gram_full_listed_ld(name, j), G)
        print(f"{name} q={q}: half-grid restatement {eh:.1e}, listed restatement {ef:.1e}")
        assert eh <= ngrid * F.EPS and ef <= ngrid * F.EPS
        # and y real does give the Hermitian pairing the restatements rest on
        Z = T.zhat_ld(name, j)
        pe, _, _ = T.partner_index(c.mesh, T.self_m(c.kmesh, q))
        assert F.relerr(Z[:, pe], Z.conj()) <= ngrid * F.EPS * 1e-3


def test_time_reversal_conjugates_w():
    """W_{-q} of conjugated inputs is conj(W_q): what fitting one q of each pair relies on.  With
    k_{-q} = b - k_q the transform of conj(y) at G is the conjugate of y's at G' = -G - (k_q +
    k_{-q}), so the identity holds as far as get_coulG gives G and G' one weight: to rounding on
    an odd mesh (asserted), and only to the weight asymmetry of the Nyquist planes on an even one
    (1e-4 .. 1e-3 for Gaussian y, printed; the same asymmetry the self-conjugate q carry)."""
    rng = np.random.default_rng(11)
    for mesh, exact in (((13, 15, 15), True), ((8, 12, 12), False)):
        c = T._case("tr", mesh, (3, 1, 2), 5, -0.4)
        ngrid = int(np.prod(mesh))
        for q in (2, 3):
            p = T.partner_q(c.kmesh, q)
            assert p != q
            y = rng.standard_normal((5, ngrid)) + 1j * rng.standard_normal((5, ngrid))
            x4 = T.make_x4(5, 20 + q, False)
            Gq = T.gram_of_ld(c, q, FF.ref_fft3d(y, mesh, kd=T.kd_ld(c.kmesh, q)), c.omega)
            Gp = T.gram_of_ld(c, p, FF.ref_fft3d(y.conj(), mesh, kd=T.kd_ld(c.kmesh, p)), c.omega)
            Wq, Wp = T.apply_inverse_ld(x4, Gq), T.apply_inverse_ld(x4.conj(), Gp)
            err = F.relerr(Wp, Wq.conj())
            print(f"mesh {mesh} q={q} -q={p}: |W_-q - conj(W_q)| / |W| {err:.1e}")
            assert not exact or err <= ngrid * F.EPS


def test_min_norm_and_basic_operators():
    """(A A^H)^+ as A (A^H A)^-2 A^H against numpy's pinv of the truncated matrix, and the basic
    solution against a direct solve on the pivots."""
    name = "rank312_n40"
    j = 1
    fact = T.pchol_ref(name, j)
    A = fact.L.astype(complex)
    rng = np.random.default_rng(3)
    g = rng.standard_normal((40, 40)) + 1j * rng.standard_normal((40, 40))
    G = g @ g.conj().T
    P = np.linalg.pinv(A @ A.conj().T, rcond=1e-10)
    assert F.relerr(T.apply_pinv_ld(fact, G), P @ G @ P) < 1e-10
    p = fact.piv
    Ai = np.linalg.inv((A @ A.conj().T)[np.ix_(p, p)])
    want = np.zeros((40, 40), complex)
    want[np.ix_(p, p)] = Ai @ G[np.ix_(p, p)] @ Ai
    assert F.relerr(T.apply_basic_ld(fact, G, 40), want) < 1e-10


@pytest.mark.parametrize("kmesh,nip", T.WS_CASES)
def test_ws_reference_equals_the_oracle(kmesh, nip):
    """W_s over every q with weight 1 against get_k_kpts' own lines; over the time-reversal
    representatives with weight 2 for a paired q it is the same when W_{-q} = conj(W_q)."""
    a = T.LATTICE
    nk = int(np.prod(kmesh))
    Wq = T.ws_inputs(kmesh, nip)
    for q in range(nk):
        p = T.partner_q(kmesh, q)
        Wq[p] = Wq[q].conj() if p > q else Wq[p]
        if p == q:
            Wq[q] = Wq[q].real
    phase = R.get_phase(a, R.get_kpts(a, kmesh), kmesh)
    oracle = (phase @ Wq.reshape(nk, -1)).reshape(nk, nip, nip).real * np.sqrt(nk)
    ref = T.ws_ld(Wq, kmesh, range(nk), np.ones(nk))
    assert F.relerr(oracle, ref) < 1e-13
    reps, wt = T.tr_reps(kmesh)
    assert F.relerr(T.ws_ld(Wq[reps], kmesh, reps, wt), ref) < 1e-17 * 100
    ref2, bnd = T.ws_bound(Wq[reps], a, kmesh, reps, wt)
    assert bnd >= len(reps) * F.EPS and np.array_equal(ref2, T.ws_ld(Wq[reps], kmesh, reps, wt))
