"""tests/func_cases.py checked on the CPU: the long-double functional against the spot table, its
limits and scaling relations, every analytic derivative against central differences, the reach of
the case tables, the names of fisdf.xc, and the arena and block plans against the library's host
functions."""
import ctypes as C

import numpy as np
import pytest

import func_cases as Fc
import kmesh_cases as K
import xc_cases as X

LD = Fc.LD
EPS_LD = float(np.finfo(LD).eps)


# ================================================================ the reference functional
def test_spot_table():
    for rs, want in Fc.SPOT_EPS:
        assert abs(Fc.eps_unif(LD(rs))[0] / LD(want) - 1) < 1e-12
    for (n, sigma), ex, ec, el in Fc.SPOTS:
        for fn in (lambda f: Fc.naive_energy(f, n, sigma),
                   lambda f: Fc.parts(f, LD(n), LD(sigma))[:2]):
            x, c = fn(Fc.GGA)
            assert abs(x / LD(ex) - 1) < 1e-12 and abs(c / LD(ec) - 1) < 1e-12, (n, sigma)
            assert abs(sum(fn(Fc.LDA)) / LD(el) - 1) < 1e-12, (n, sigma)
    x, c = Fc.naive_energy(Fc.GGA, 2.5, 0.0)
    assert abs((x + c) / sum(Fc.naive_energy(Fc.LDA, 2.5, 0.0)) - 1) < 8 * EPS_LD


def _grid():
    n = np.array([1e-3, 0.1, 1.0, 2.5, 50.0], LD)
    s = np.array([1e-6, 0.02, 3.0, 100.0], LD)
    nn, ss = np.meshgrid(n, s, indexing="ij")
    return nn.ravel(), ss.ravel()


def test_stable_form_is_the_formula():
    """eps + H = gamma log1p(-q / D) is the issue's H + eps: compared where the literal formula
    has not yet lost anything to its cancellation."""
    n, s = _grid()
    x, c = Fc.naive_energy(Fc.GGA, n, s)
    P = Fc.parts(Fc.GGA, n, s)
    assert np.abs(P.ex / x - 1).max() < 64 * EPS_LD
    # the literal n (eps + H) cancels at large t^2: its error is a rounding of n eps, not of e_c
    neps = np.abs(Fc.parts(Fc.LDA, n, s).ec)
    assert (np.abs(P.ec - c) / neps).max() < 64 * EPS_LD
    mild = np.abs(c) > 0.1 * neps
    assert mild.sum() >= 10 and np.abs(P.ec / c - 1)[mild].max() < 1e3 * EPS_LD
    # float64 is the same code
    P64 = Fc.parts(Fc.GGA, n.astype(float), s.astype(float), np.float64)
    for a, b in zip(P64, P):
        assert a.dtype == np.float64 and np.abs(a / b - 1).max() < 1e-12


def test_pbe_at_sigma_zero_is_lda():
    n = 10.0 ** np.linspace(-14, 3, 69).astype(LD)
    g, l = Fc.parts(Fc.GGA, n, np.zeros_like(n)), Fc.parts(Fc.LDA, n, np.zeros_like(n))
    for a, b in ((g.ex, l.ex), (g.ec, l.ec), (g.vnx, l.vnx), (g.vnc, l.vnc)):
        assert np.abs(a / b - 1).max() < 16 * EPS_LD
    assert np.isfinite(g.vsx).all() and np.isfinite(g.vsc).all() and (g.vsc > 0).all()


def test_exchange_scaling_and_limits():
    n, s = _grid()
    P = Fc.parts(Fc.GGA, n, s)
    for lam in (LD(2), LD(1.7)):
        Q = Fc.parts(Fc.GGA, lam ** 3 * n, lam ** 8 * s)
        assert np.abs(Q.ex / (lam ** 4 * P.ex) - 1).max() < 64 * EPS_LD
    rho = np.concatenate([Fc.xc_table(1000, 3), Fc.xc_table(257, 3)], axis=2)
    nn = rho[:, 0]
    live = nn > Fc.RHO_CUT
    nl = np.where(live, nn, 1.0).astype(LD)
    sig = (rho[:, 1:].astype(LD) ** 2).sum(axis=1)
    T = Fc.parts(Fc.GGA, nl, sig)
    kap = LD(Fc.LD(Fc.KAPPA))
    assert (T.fx <= 1 + kap).all() and (T.fx >= 1).all()
    big = Fc.parts(Fc.GGA, LD(1e-3), LD(1e6))          # s^2 = 2.6e12, t^2 = 3.6e9
    assert 0 < 1 + kap - big.fx < 1e-11
    eps = Fc.eps_unif(Fc._c(LD)["rs0"] / np.cbrt(LD(1e-3)))[0]
    assert 0 > big.w > 1e-8 * eps                      # eps + H -> 0
    # eps + H rises from eps to 0 with t^2
    assert ((T.w <= 0) & (T.w >= Fc.parts(Fc.LDA, nl, sig).w * (1 + 8 * LD(EPS_LD)))).all()


@pytest.mark.parametrize("family", [Fc.LDA, Fc.GGA])
def test_derivatives_against_central_differences(family):
    """Each analytic derivative, exchange and correlation separately, against central differences
    of the long-double energy at steps h and h/2: the error falls by 4 +- 0.1."""
    n, s = _grid()
    P = Fc.parts(family, n, s)
    k = Fc._c(LD)
    worst = []
    for var, ana in (("n", (P.vnx, P.vnc)), ("sigma", (P.vsx, P.vsc))):
        if family == Fc.LDA and var == "sigma":
            assert not P.vsx.any() and not P.vsc.any()
            continue
        # the step in sigma is relative to sigma + the sigma at which s^2 or t^2 reaches 1,
        # whichever comes first: relative to sigma alone, a point with small s^2 and t^2 has e
        # linear in sigma to rounding and no truncation error to measure (sigma - step may then be
        # negative, which the formulas in s^2 and t^2 take)
        kf = k["kf0"] * np.cbrt(n)
        unit = np.minimum(4 * kf * kf * n * n, 16 * kf * n * n / k["pi"])
        errs = []
        for h in (LD(2) ** -8, LD(2) ** -9):
            dn, ds = (n * h, 0 * s) if var == "n" else (0 * n, (s + unit) * h)
            up, dw = Fc.parts(family, n + dn, s + ds), Fc.parts(family, n - dn, s - ds)
            step = 2 * (dn if var == "n" else ds)
            errs.append([(up.ex - dw.ex) / step - ana[0], (up.ec - dw.ec) / step - ana[1]])
        floor = [np.abs(f) / np.abs(step) * EPS_LD for f in (P.ex, P.ec)]    # step: that of h / 2
        for part in (0, 1):
            e1, e2 = np.abs(errs[0][part]), np.abs(errs[1][part])
            # the truncation error stands clear of the rounding of the difference quotient
            assert (e2 > 500 * floor[part]).all(), (var, part, e2 / floor[part])
            ratio = e1 / e2
            worst.append(float(np.abs(ratio - 4).max()))
            assert np.abs(ratio - 4).max() < 0.1, (var, part, ratio)
    print("largest |ratio - 4|:", max(worst))


def test_finite_on_the_tables():
    for c in Fc.XC_CASES:
        rho, ref, (e64, w64) = Fc.xc_data(c)
        f64 = Fc.func_ref(c.family, c.cx, c.cc, Fc.RHO_CUT, rho, np.float64)
        for a in (ref.e, ref.wv, ref.se, ref.sw, f64.e, f64.wv):
            assert np.isfinite(a).all(), Fc.xc_id(c)
        assert e64 < 64 * Fc.EPS and w64 < 64 * Fc.EPS, (Fc.xc_id(c), e64, w64)


# ================================================================ the reach of the tables
def test_tables_reach_their_branches():
    got = set()
    specials = {"at_cut", "ulp_above_cut", "ulp_below_cut", "n_zero", "n_negative", "sigma_zero",
                "s2_large"}
    for ng in Fc.NGS:
        for nset in (1, 3):
            b = Fc.table_branches(Fc.xc_table(ng, nset))
            got |= b
            if ng >= 255:
                assert specials <= b, (ng, nset)
    assert got == Fc.TABLE_BRANCHES
    assert "workgroup_partial" in Fc.table_branches(Fc.xc_table(257, 1))
    assert "workgroup_full" in Fc.table_branches(Fc.xc_table(256, 1))
    # the cut from both sides: zeros at and below it, values above it
    rho = Fc.xc_table(255, 1)
    ref = Fc.func_ref(Fc.GGA, 1.0, 1.0, Fc.RHO_CUT, rho)
    names = [s[0] for s in Fc.special_points(Fc.RHO_CUT)]
    for name in ("at_cut", "ulp_below_cut", "n_zero", "n_negative"):
        i = names.index(name)
        assert ref.e[0, i] == 0 and not ref.wv[0, :, i].any()
    i = names.index("ulp_above_cut")
    assert ref.e[0, i] < 0 and ref.wv[0, 0, i] < 0 and ref.wv[0, 1:, i].any()
    assert len({(c.family, c.cx, c.cc) for c in Fc.XC_CASES}) == 8


def test_fused_cases_reach_their_branches():
    rho_b, gram_b = set(), set()
    for c in Fc.BLOCK_CASES:
        rho_b |= X.rho_branches(c.nao, c.ng, c.nk, c.nset, 1)
        gram_b |= X.gram_branches(c.nao, c.ng, c.nk, c.nset, c.acc)
    assert {"d_tiled", "d_untiled", "hermi", "set_chunks", "sets_4", "sets_1", "sets_3",
            "one_block", "many_blocks", "point_tile_partial", "nao_tile_partial"} <= rho_b
    assert gram_b == X.GRAM_BRANCHES
    assert X.rho_set_chunks(33, 5, 1) == [4, 1]
    assert {Fc.XC_THREADS < c.ng for c in Fc.BLOCK_CASES} == {True, False}


def test_no_fused_point_is_at_or_below_the_cut():
    """so that the cut cannot hide a wrong value"""
    for c in Fc.BLOCK_CASES:
        w, d = Fc.block_ref(c)
        assert w.rho[:, 0].min() > 1e-3 and d.rho[:, 0].min() > 1e-3, Fc.block_id(c)


@pytest.mark.parametrize("name,least", [("toy_222", 0.116), ("toy_113", 0.028),
                                        ("diamond_112", 1.05e-3)])
def test_no_end_to_end_point_is_at_or_below_the_cut(name, least):
    c, d = X.E2E_BY_NAME[name], X.e2e_data(name)
    rho = X.rho_gga_ref(d.f4, Fc.e2e_dm(name), 1).real
    lo = float(rho[:, 0].min())
    print(f"{name}: smallest rho {lo:.4e}")
    assert lo > Fc.RHO_CUT and abs(lo / least - 1) < 0.01
    if name in Fc.E2E_TWO_SETS:
        assert X.rho_gga_ref(d.f4, Fc.e2e_dm(name, 2), 1).real[:, 0].min() > 0.02
    # the perturbed matrices of the energy tie
    if name in Fc.TIE_CASES:
        D, dl = Fc.tie_matrices(name)
        for m in (D + dl, D - dl):
            assert X.rho_gga_ref(d.f4, m[None], 1).real[:, 0].min() > 0.5 * least


def test_energy_tie_converges_to_the_trace():
    """(exc[D + d] - exc[D - d]) / 2 -> (1/nk) sum_k Re tr(V_k d_k) with error ratio 4 as d
    halves: the density, the functional's derivatives and the matrix fit together."""
    name = "toy_113"
    c, d = X.E2E_BY_NAME[name], X.e2e_data(name)
    nk, ngrid = K.nk_of(c.kmesh), len(d.coords)
    scale = LD(d.cell.vol) / ngrid
    D, dl = Fc.tie_matrices(name)

    def run(m):
        return Fc.block_pipeline(d.f4, m[None], Fc.GGA, 1.0, 1.0, Fc.RHO_CUT, scale)

    V = run(D).vxc[0]
    errs = []
    for h in (1, 2):
        dh = dl / h
        assert np.array_equal((D + dh) - (D - dh), 2 * dh)
        lhs = (run(D + dh).sums[0, 1] - run(D - dh).sums[0, 1]) / 2
        rhs = sum(np.trace(V[k] @ dh[k].astype(X.CLD)).real for k in range(nk)) / nk
        errs.append(abs(lhs - rhs) / abs(rhs))
    print("energy tie: relative errors", [float(e) for e in errs])
    assert errs[0] < 1e-2 and abs(errs[0] / errs[1] - 4) < 0.1


# ================================================================ fisdf.xc
def test_parse_xc():
    import fisdf
    from fisdf import xc
    assert set(xc.FUNCTIONALS) == {"lda", "pbe", "pbe0", "hf"}
    assert xc.parse_xc("PBE") is xc.FUNCTIONALS["pbe"] and xc.parse_xc("pbe,pbe") is xc.parse_xc("Pbe")
    assert xc.parse_xc("pbe0") == ("GGA", 0.75, 1.0, 0.25) and xc.parse_xc("LDA").code == xc.LDA
    assert xc.parse_xc("hf").family is None and not xc.parse_xc("hf").local
    assert [fisdf.hybrid_coeff(n) for n in ("lda", "pbe", "PBE0", "hf")] == [0, 0, 0.25, 1]
    assert fisdf.hybrid_coeff(lambda rho: None) == 0
    mix = xc.Functional("gga", 0.5, 1, 0.5)
    assert xc.parse_xc(mix) is mix and mix.code == xc.GGA and fisdf.hybrid_coeff(mix) == 0.5
    for bad in ("svwn", "b3lyp", "hse06", "scan", "tpss", "m06l", "", "pbe,", None, 3):
        with pytest.raises(ValueError, match="pbe0"):
            xc.parse_xc(bad)
    for bad in (("mgga", 1, 1, 0), ("GGA", np.nan, 1, 0), ("LDA", 1, np.inf, 0)):
        with pytest.raises(ValueError):
            xc.Functional(*bad)


# ================================================================ the plans
def test_arena_plan_matches_library():
    from fisdf import _lib, xc
    lib = _lib.load()
    for nao in (1, 8, 26, 33):
        for nset in range(1, 6):
            for ng in (1, 65, 997, 2049):
                for nk in (1, 2, 27):
                    pp, fx = C.c_long(), C.c_long()
                    assert lib.fisdf_nr_rks_plan(nk, ng, nao, nset, C.byref(pp), C.byref(fx)) == 0
                    want = Fc.arena_plan(nk, ng, nao, nset)
                    assert (pp.value, fx.value) == want == xc.nr_rks_arena(nk, ng, nao, nset)
    # the fixed part does not decrease with the block: the Python plan takes it at the whole grid
    fixed = [Fc.arena_plan(2, ng, 26, 4)[1] for ng in range(1, 5000, 37)]
    assert fixed == sorted(fixed)
    for bad in ((0, 5, 3, 1), (1, 0, 3, 1), (1, 5, 0, 1), (1, 5, 3, 0), (1 << 20, 5, 1 << 10, 1)):
        assert lib.fisdf_nr_rks_plan(*bad, None, None) != 0
    assert lib.fisdf_abi_version() == 4


def test_block_points():
    """deriv_block_points() is what it was; nr_rks's own plan holds the fused arena too."""
    from fisdf import ISDF
    d = X.e2e_data("toy_113")
    df = ISDF(d.cell, d.cell.get_kpts((1, 1, 3)))
    df._kmesh()
    nk, nao, ngrid = 3, d.cell.nao_nr(), len(d.coords)
    assert df.xc_rho_cut == 1e-15 and df.deriv_work_bytes == 512 << 20
    from fisdf.cell import lattice_translations
    ntn = len(lattice_translations(d.cell, df.grids_coords()))
    per_point, fixed = 96 * nk * nao, (1 << 20) + 4096 + 24 * ntn
    old = df.deriv_work_bytes
    try:
        for b in (1 << 21, 3 << 20, 1 << 24, 512 << 20):
            df.deriv_work_bytes = b
            assert df.deriv_block_points() == (b - fixed) // per_point
            for nset in (1, 4):
                ap, af = Fc.arena_plan(nk, ngrid, nao, nset)
                nb = df.nr_rks_block_points(nset)
                assert nb == (b - fixed - af) // (per_point + ap) <= df.deriv_block_points()
        df.deriv_work_bytes = 1000
        with pytest.raises(ValueError):
            df.nr_rks_block_points()
    finally:
        df.deriv_work_bytes = old
