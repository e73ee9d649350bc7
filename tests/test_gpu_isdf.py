"""GPU parity of the full ISDF path (build + get_jk) against the CPU oracle.

Bar (BASELINE.json north_star): J/K max-abs difference vs the oracle (the restated
reference CPU path, gelsy fit) < 1e-8 Ha.  Interpolation points: the oracle's pivots
are injected for the J/K parity; GPU selection is tested separately.
"""
import numpy as np
import pytest

from cases import inputs, oracle

pytestmark = pytest.mark.gpu

JK_TOL = 1e-8   # Ha, north_star (every case, rank-deficient x4_q included)


def make_df(name, inject=True, time_reversal=True, real_sc=True, pivoted=None, fit="lstsq"):
    from fisdf import ISDF
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    o = oracle(name)
    kpts = cell.get_kpts(kmesh)
    df = ISDF(cell, kpts, m0=list(m0), c0=c0)
    df.time_reversal = time_reversal
    df.real_self_conjugate = real_sc
    df.pivoted_fit = pivoted
    df.fit = fit
    d = df.device
    df._kmesh()
    df._ao_parent = d.to_dev(x0)
    df._ao_grid = d.to_dev(chi)
    if inject:
        df.set_interpolation_points(o["perm"])
    return df, o, dm


@pytest.mark.parametrize("name", ["toy222", "toy331", "toy331_fr", "toy333_fr",
                                  "diamond_szv_gamma", "nio_small", "si_small", "toy222_rank",
                                  "toy666"])
def test_jk_parity_vs_oracle(name):
    df, o, dm = make_df(name)
    df.build()
    vj, vk = df.get_jk(dm)
    assert vj.shape == dm.shape and vk.shape == dm.shape
    ej = abs(vj - o["vj"]).max()
    ek = abs(vk - o["vk"]).max()
    full_rank = min(df.ranks) == df.nip
    print(f"{name}: nip={df.nip} ranks {min(df.ranks)}-{max(df.ranks)}, {len(df.fit_qs)} q "
          f"fitted: |dJ|={ej:.2e} |dK|={ek:.2e}")
    assert df.min_norm_slots == sum(int(r < df.nip) for r in df.ranks)
    assert ej < JK_TOL
    assert ek < JK_TOL
    # reality invariants of fftisdf.py:43,81,216
    mi = df.device.ctx.max_imag()
    assert max(mi) < 1e-10, mi


@pytest.mark.parametrize("name", ["toy331", "toy331_fr", "toy222"])
def test_jk_parity_without_time_reversal(name):
    """Every q fitted independently (as the reference does) gives the same J/K, and the
    time-reversal build reproduces it: W_{-q} = conj(W_q) up to the null space of x4_q."""
    res = {}
    for tr in (False, True):
        df, o, dm = make_df(name, time_reversal=tr)
        df.build()
        vj, vk = df.get_jk(dm)
        nk = int(np.prod(df.kmesh))
        assert len(df.fit_qs) == (nk if not tr else len(set(map(tuple, np.sort(
            np.stack([np.arange(nk), df.q_partner], 1), 1)))))
        ej, ek = abs(vj - o["vj"]).max(), abs(vk - o["vk"]).max()
        print(f"{name} time_reversal={tr}: ranks {list(df.ranks)} |dJ|={ej:.2e} |dK|={ek:.2e}")
        assert ej < JK_TOL and ek < JK_TOL
        res[tr] = (vj, vk)
    d = max(abs(res[True][0] - res[False][0]).max(), abs(res[True][1] - res[False][1]).max())
    print(f"{name}: |JK(tr) - JK(all q)| = {d:.2e}")
    assert d < JK_TOL


@pytest.mark.parametrize("name", ["toy222", "toy331_fr", "diamond_szv_gamma", "si_small"])
def test_real_self_conjugate_path(name):
    """q with 2 k_q in the reciprocal lattice (all q of 2x2x2, Gamma) are fitted with a real
    factor (half-MFMA TRSM) and a real-part HERK; J/K agree with the all-complex fit."""
    res = {}
    for real_sc in (False, True):
        df, o, dm = make_df(name, real_sc=real_sc)
        df.build()
        vj, vk = df.get_jk(dm)
        ej, ek = abs(vj - o["vj"]).max(), abs(vk - o["vk"]).max()
        print(f"{name} real_sc={real_sc}: |dJ|={ej:.2e} |dK|={ek:.2e}")
        assert ej < JK_TOL and ek < JK_TOL
        res[real_sc] = (vj, vk, df._wq)
    dw = abs(res[True][2] - res[False][2]).max() / abs(res[False][2]).max()
    d = max(abs(res[True][0] - res[False][0]).max(), abs(res[True][1] - res[False][1]).max())
    print(f"{name}: |JK(real) - JK(complex)| = {d:.2e}, rel |dW| = {dw:.2e}")
    assert d < JK_TOL


@pytest.mark.parametrize("name", ["toy331_fr", "toy333_fr", "nio_small", "toy331"])
def test_unpivoted_fast_path(name):
    """The full-rank fast path (unpivoted blocked Cholesky) gives the J/K of the pivoted
    rank-revealing factorisation; rank-deficient x4_q fall back to the pivoted path."""
    res = {}
    for piv in (True, None):
        df, o, dm = make_df(name, pivoted=piv)
        df.build()
        vj, vk = df.get_jk(dm)
        full_rank = min(df.ranks) == df.nip
        print(f"{name} pivoted={piv}: used_pivoted={df.used_pivoted_fit} ranks "
              f"{min(df.ranks)}-{max(df.ranks)} |dK|={abs(vk - o['vk']).max():.2e}")
        if piv is None:
            assert df.used_pivoted_fit == (not full_rank)
        assert abs(vj - o["vj"]).max() < JK_TOL and abs(vk - o["vk"]).max() < JK_TOL
        res[piv] = (vj, vk)
    d = max(abs(res[True][0] - res[None][0]).max(), abs(res[True][1] - res[None][1]).max())
    print(f"{name}: |JK(unpivoted) - JK(pivoted)| = {d:.2e}")
    assert d < JK_TOL


@pytest.mark.parametrize("name", ["toy331", "toy222", "toy222_rank"])
def test_min_norm_fit(name):
    """Rank-deficient x4_q (nip above their numerical rank; toy222_rank is the reference demo's
    nip = parent-rank regime): the default fit applies the minimum-norm operator A^+ (gelsy's
    complete orthogonal step, fftisdf.py:108) on those q.  J/K vs the gelsy oracle < 1e-8 Ha;
    the round-1 basic solution (FISDF_FIT_BASIC) is printed beside it.  gelsy itself moves by
    1-4e-9 under a 2-4x change of its rcond here (tests/experiments/gelsy_sensitivity.py)."""
    errs = {}
    for fit in ("basic", "lstsq"):
        df, o, dm = make_df(name, fit=fit)
        df.build()
        vj, vk = df.get_jk(dm)
        ndef = sum(int(r < df.nip) for r in df.ranks)
        assert ndef > 0, "case is not rank-deficient"
        assert df.min_norm_slots == (ndef if fit == "lstsq" else 0)
        errs[fit] = (abs(vj - o["vj"]).max(), abs(vk - o["vk"]).max())
        print(f"{name} fit={fit}: ranks {min(df.ranks)}-{max(df.ranks)} of nip {df.nip}, "
              f"min-norm q {df.min_norm_slots}: |dJ|={errs[fit][0]:.2e} |dK|={errs[fit][1]:.2e} "
              f"(margin {JK_TOL / max(errs[fit]):.1f}x)")
    assert max(errs["lstsq"]) < JK_TOL


@pytest.mark.parametrize("name", ["nio_small", "toy331", "si_small", "toy222_rank"])
def test_svd_fit(name):
    """fit="svd" (the SVD-fit configuration C4, fftdf-with-k-svd.py:158-164 intent): the
    rank-revealing factor and the minimum-norm operator on every q.  J/K vs the SVD-pseudo-solve
    oracle and vs the gelsy oracle < 1e-8 Ha."""
    from cases import oracle_svd
    df, o, dm = make_df(name, fit="svd")
    df.build()
    vj, vk = df.get_jk(dm)
    s = oracle_svd(name)
    assert df.used_pivoted_fit and df.min_norm_slots == len(df.fit_qs)
    es = (abs(vj - s["vj"]).max(), abs(vk - s["vk"]).max())
    eg = (abs(vj - o["vj"]).max(), abs(vk - o["vk"]).max())
    print(f"{name} fit=svd: ranks {min(df.ranks)}-{max(df.ranks)} (svd oracle "
          f"{min(s['ranks'])}-{max(s['ranks'])}) of nip {df.nip}: vs svd oracle |dJ|={es[0]:.2e} "
          f"|dK|={es[1]:.2e}; vs gelsy |dJ|={eg[0]:.2e} |dK|={eg[1]:.2e}")
    assert max(es) < JK_TOL and max(eg) < JK_TOL


def test_kpts_band():
    """get_jk(kpts_band=...) (next-4; the reference asserts nband == nkpt, fftisdf.py:164,196):
    J at off-mesh band k-points vs the oracle's J from the same v with the band AOs at the
    interpolation points; J and K at band k-points on the k-mesh are the matching rows of the
    k-mesh result; K off the mesh raises NotImplementedError; a 1-D band k-point drops the band
    axis ([pyscf] _format_jks)."""
    from fisdf import cell as C
    from oracle import isdf_ref as R
    name = "toy333_fr"
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    df, o, dm = make_df(name)
    df.build()
    rng = np.random.default_rng(4)
    kb = rng.uniform(-0.5, 0.5, (3, 3)) @ cell.reciprocal_vectors()
    vj_b, vk_b = df.get_jk(dm, kpts_band=kb, with_k=False)
    assert vk_b is None and vj_b.shape == (1, 3) + dm.shape[-2:]
    xb = C.eval_ao_band(cell, cell.gen_uniform_grids(m0)[o["perm"]], kb)
    ref = R.get_j_kpts(o["xip"], o["w0"], dm, xband=xb)
    ej = abs(vj_b - ref).max()
    print(f"{name} kpts_band off-mesh: |dJ| {ej:.2e} (max|J| {abs(ref).max():.2f})")
    assert ej < JK_TOL
    sel = [5, 0, 3]
    vj2, vk2 = df.get_jk(dm, kpts_band=df.kpts[sel])
    vj, vk = df.get_jk(dm)
    assert abs(vj2 - vj[:, sel]).max() < 1e-12 and abs(vk2 - vk[:, sel]).max() < 1e-12
    with pytest.raises(NotImplementedError):
        df.get_jk(dm, kpts_band=kb, with_j=False)
    vj1, _ = df.get_jk(dm, kpts_band=kb[1], with_k=False)
    assert vj1.shape == (1,) + dm.shape[-2:] and abs(vj1[0] - ref[0, 1]).max() < JK_TOL


@pytest.mark.parametrize("name", ["toy222", "toy331_fr", "diamond_szv_gamma", "si_small"])
def test_half_grid_self_conjugate(name):
    """Self-conjugate q fitted on half the G grid (ISDF.half_grid; the Hermitian pairs
    G' = -G - 2 k_q of a real z_q, incl. odd meshes (toy331_fr: 15^3) and both parities of 2 k_q)
    give the full-grid W_q and the oracle's J/K."""
    res = {}
    for half in (0, 1):
        df, o, dm = make_df(name)
        df.half_grid = bool(half)
        df.build()
        vj, vk = df.get_jk(dm)
        ej, ek = abs(vj - o["vj"]).max(), abs(vk - o["vk"]).max()
        print(f"{name} half_grid={half}: |dJ|={ej:.2e} |dK|={ek:.2e}")
        assert ej < JK_TOL and ek < JK_TOL
        res[half] = (vj, vk, df._wq)
    dw = abs(res[1][2] - res[0][2]).max() / abs(res[0][2]).max()
    d = max(abs(res[1][0] - res[0][0]).max(), abs(res[1][1] - res[0][1]).max())
    print(f"{name}: |JK(half) - JK(full)| = {d:.2e}, rel |dW| = {dw:.2e}")
    assert d < 1e-9


def test_build_y_qlist():
    """fisdf_build_y_qs with a non-contiguous q-list writes y_q in list order."""
    from fisdf import _lib as L
    name = "toy331"
    df, o, dm = make_df(name)
    df.build()
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    d = df.device
    nk, ngrid, nip, nao = chi.shape[0], chi.shape[1], o["xip"].shape[1], chi.shape[2]
    qs = np.array([1, 4, 5, 8], np.int32)
    yT = d.empty((len(qs), nip, ngrid))
    km, kmp = L.iarr(kmesh)
    a, ap = L.darr(cell.a.ravel())
    d.ctx.call("fisdf_build_y_qs", L.ptr(df._ao_grid), ngrid * nao, 0, ngrid, ngrid,
               L.ptr(df._dev_state["X"]), nip, nao, kmp, ap, qs.ctypes.data_as(L._ip), len(qs),
               L.ptr(yT))
    y = yT.cpu().numpy().transpose(0, 2, 1)
    ref = o["y"][qs]
    assert abs(y - ref).max() / abs(ref).max() < 1e-12
    # y_{-q} = conj(y_q): the time-reversal identity the fit relies on
    part = df.q_partner
    for q in range(nk):
        assert abs(o["y"][part[q]] - o["y"][q].conj()).max() < 1e-12 * abs(o["y"]).max()


@pytest.mark.parametrize("name", ["toy222", "toy331", "toy333_fr"])
def test_x4_and_y_parity(name):
    df, o, dm = make_df(name)
    df.build()
    x4 = df._dev_state["x4"].cpu().numpy()
    rel = abs(x4 - o["x4"]).max() / abs(o["x4"]).max()
    assert rel < 1e-12
    # y for all q through the C-ABI build_y (transposed layout yT[q][I][g])
    from fisdf import _lib as L
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    d = df.device
    nk, ngrid, nip, nao = chi.shape[0], chi.shape[1], o["xip"].shape[1], chi.shape[2]
    km, kmp = L.iarr(kmesh)
    a, ap = L.darr(cell.a.ravel())
    # x4 through the C-ABI with every x2_k formed and with the representatives k <= -k only
    # (x2_{-k} = conj(x2_k)); both through the register k-mesh DFT pair and, FISDF_X4_DFT=0 in
    # another process, the dense Phi GEMMs (the build above)
    x4b = d.empty((nk, nip, nip))
    for tr in (0, 1):
        d.ctx.call("fisdf_set_time_reversal", tr)
        x4b.zero_()
        d.ctx.call("fisdf_build_x4", L.ptr(df._dev_state["X"]), nip, nao, kmp, ap, L.ptr(x4b))
        rel = abs(x4b.cpu().numpy() - o["x4"]).max() / abs(o["x4"]).max()
        print(f"{name} x4 time_reversal={tr}: max rel |x4 - x4_oracle| = {rel:.2e}")
        assert rel < 1e-12
    yT = d.empty((nk, nip, ngrid))
    # two blocks to exercise the g0 offset; every k computed, then fx_k for half the k-mesh
    # with fx_{-k} = conj(fx_k) (fisdf_set_time_reversal)
    h = ngrid // 2
    for tr in (0, 1):
        d.ctx.call("fisdf_set_time_reversal", tr)
        yT.zero_()
        for g0, g1 in ((0, h), (h, ngrid)):
            d.ctx.call("fisdf_build_y", L._vp(df._ao_grid.data_ptr() + g0 * nao * 16),
                       ngrid * nao, g0, g1 - g0, ngrid,
                       L.ptr(df._dev_state["X"]), nip, nao, kmp, ap, 0, nk, L.ptr(yT))
        y = yT.cpu().numpy().transpose(0, 2, 1)
        rel = abs(y - o["y"]).max() / abs(o["y"]).max()
        print(f"{name} time_reversal={tr}: max rel |y - y_oracle| = {rel:.2e}")
        assert rel < 1e-12


@pytest.mark.parametrize("name", ["toy222", "diamond_szv_gamma", "si_small"])
def test_selection_paths_agree(name, monkeypatch):
    """The batched-candidate selection (default), the cooperative left-looking one
    (FISDF_SEL_MODE=coop), its split form with only the first K columns of the owned L rows in
    LDS (forced here with FISDF_SEL_LDS_COLS; the default when the rows do not fit, as in C5) and
    the blocked right-looking one (FISDF_SEL_COOP=0) pick the same pivots as dpstrf on these
    cases."""
    import torch
    import select_cases as S
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    perms, ran = {}, {}
    for mode, env in (("batch", {"FISDF_SEL_COOP": "1", "FISDF_SEL_MODE": "batch"}),
                      ("coop", {"FISDF_SEL_COOP": "1", "FISDF_SEL_MODE": "coop"}),
                      ("split", {"FISDF_SEL_COOP": "1", "FISDF_SEL_MODE": "coop",
                                 "FISDF_SEL_LDS_COLS": "20"}),
                      ("blocked", {"FISDF_SEL_COOP": "0"})):
        monkeypatch.delenv("FISDF_SEL_LDS_COLS", raising=False)
        monkeypatch.delenv("FISDF_SEL_MODE", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        df, o, dm = make_df(name, inject=False)
        df.build()
        perms[mode] = df.perm.copy()
        # the kernel the mode names runs at this size (restated plan = the library's host
        # functions, test_select_cases.py): a refused one would repeat another mode's kernel
        n = df._ao_parent.shape[1]
        rmax = max(1, min(int(df.cell.nao_nr() * df.c0), n))
        ran[mode] = S.reached(n, rmax, ncu, {"batch": 0, "coop": 1, "split": 1, "blocked": 2}[mode],
                              20 if mode == "split" else 0)[0]
    print(f"{name}: " + ", ".join(f"{m} == dpstrf: {np.array_equal(p, o['perm'])}"
                                  for m, p in perms.items()))
    assert ran == {"batch": S.BATCH, "coop": S.COOP, "split": S.COOP_SPLIT, "blocked": S.PANEL}, ran
    for m, p in perms.items():
        assert np.array_equal(p, o["perm"]), m


@pytest.mark.parametrize("name", ["toy222", "diamond_szv_gamma"])
def test_gpu_selection(name):
    df, o, dm = make_df(name, inject=False)
    df.build()
    perm_gpu = df.perm
    assert len(perm_gpu) == o["nip"]
    overlap = len(set(perm_gpu.tolist()) & set(o["perm"].tolist())) / o["nip"]
    first = int(np.argmax(perm_gpu != o["perm"])) if (perm_gpu != o["perm"]).any() else len(perm_gpu)
    print(f"{name}: pivot-set overlap with dpstrf {overlap:.3f}, identical prefix {first}/{o['nip']}")
    # the GPU picks dpstrf's pivots here (test_gpu_selection.py certifies the general case),
    # so the J/K of the GPU-selected build meet the north_star bar against the oracle
    assert np.array_equal(perm_gpu, o["perm"])
    vj, vk = df.get_jk(dm)
    assert abs(vj - o["vj"]).max() < JK_TOL
    assert abs(vk - o["vk"]).max() < JK_TOL


def test_not_implemented_paths():
    df, o, dm = make_df("toy222")
    df.build()
    with pytest.raises(NotImplementedError):
        df.get_jk(dm, omega=0.3, exxdiv="ewald")   # range separation is supported alone
    with pytest.raises(NotImplementedError):
        df.get_jk(dm, exxdiv="vcut_sph")        # only 'ewald' is added (next-4)
    with pytest.raises(NotImplementedError):
        df.get_jk(dm[0, 0], kpts=np.zeros(3))


def test_get_eri_partner_q():
    """ERIs whose q = k2 - k1 is the time-reversal partner of a fitted q (W = conj(W_rep))."""
    from oracle import exact_ref as E, isdf_ref as R
    from fisdf.cell import cartesian_prod
    df, o, dm = make_df("toy331")
    df.build()
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs("toy331")
    kpts = R.get_kpts(cell.a, kmesh)
    ks = cartesian_prod([np.arange(n) for n in kmesh])
    nao = cell.nao_nr()
    fitted = set(int(q) for q in df.fit_qs)

    def kidx(v):
        v = np.mod(v, kmesh)
        return int((v[0] * kmesh[1] + v[1]) * kmesh[2] + v[2])

    seen = set()
    for (k1, k2, k3) in [(1, 0, 0), (0, 1, 4), (5, 2, 7), (8, 3, 2)]:
        q = kidx(ks[k2] - ks[k1])
        seen.add(q in fitted)
        k4 = kidx(ks[k1] - ks[k2] + ks[k3])
        eri = df.get_eri(kpts[[k1, k2, k3, k4]]).reshape(nao, nao, nao, nao)
        ex = E.exact_eri(chi, cell.a, cell.mesh, kpts, coords, k1, k2, k3, k4)
        print(k1, k2, k3, k4, "q", q, "fitted", q in fitted, "vs exact", abs(eri - ex).max())
        assert abs(eri - ex).max() < 1e-6
    assert seen == {True, False}
    wq = df._wq
    assert wq.shape == (9, df.nip, df.nip)
    for q in range(9):
        if df.q_partner[q] != q:
            assert abs(wq[df.q_partner[q]] - wq[q].conj()).max() == 0.0


@pytest.mark.parametrize("name", ["toy333_fr", "toy222_rank"])
def test_dump_load(name, tmp_path):
    """ISDF.dump / ISDF.load (checkpoint): a fresh object on the same cell restored from
    the .npz gives get_jk, get_eri and _x / _w0 / _wq bit for bit as after the build; a dump of
    another k-mesh is refused."""
    from fisdf import ISDF
    df, o, dm = make_df(name)
    df.build()
    vj, vk = df.get_jk(dm)
    path = tmp_path / "isdf.npz"
    df.dump(path)
    cell, kmesh, m0, c0, *_ = inputs(name)
    df2 = ISDF(cell, cell.get_kpts(kmesh), m0=list(m0), c0=c0).load(path)
    vj2, vk2 = df2.get_jk(dm)
    assert np.array_equal(vj, vj2) and np.array_equal(vk, vk2)
    for a in ("_x", "_w0", "_wq"):
        assert np.array_equal(getattr(df, a), getattr(df2, a)), a
    kpts = df.kpts
    nk = len(kpts)
    k4 = kpts[[0, min(1, nk - 1), min(2, nk - 1), 0]]
    try:
        e1 = df.get_eri(k4)
    except ValueError:                      # momentum conservation: use a diagonal quartet
        k4 = kpts[[0, 0, 0, 0]]
        e1 = df.get_eri(k4)
    assert np.array_equal(e1, df2.get_eri(k4))
    other = tuple(int(v) + 1 if i == 0 else int(v) for i, v in enumerate(kmesh))
    with pytest.raises(ValueError):
        ISDF(cell, cell.get_kpts(other), m0=list(m0), c0=c0).load(path)
    print(f"\n{name}: dump {path.stat().st_size / 1e6:.1f} MB, reloaded J/K, ERI, _wq bitwise")


def test_get_eri_and_ao2mo():
    """next-2: ISDF ERIs vs the exact FFT ERI (fftdf-with-k-lstsq.py:219-258 harness: fails
    above 1e-4) and vs the oracle's ISDF ERI; ao2mo with MO coefficients == transformed AO ERI."""
    from oracle import exact_ref as E, isdf_ref as R
    from fisdf.cell import cartesian_prod
    df, o, dm = make_df("toy222")
    df.build()
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs("toy222")
    kpts = R.get_kpts(cell.a, kmesh)
    ks = cartesian_prod([np.arange(n) for n in kmesh])
    nao = cell.nao_nr()

    def kidx(v):
        v = np.mod(v, kmesh)
        return int((v[0] * kmesh[1] + v[1]) * kmesh[2] + v[2])

    x = o["xip"]
    for (k1, k2, k3) in [(0, 0, 0), (0, 1, 2), (3, 5, 6), (7, 7, 1)]:
        q = kidx(ks[k2] - ks[k1])
        k4 = kidx(ks[k1] - ks[k2] + ks[k3])
        eri = df.get_eri(kpts[[k1, k2, k3, k4]]).reshape(nao, nao, nao, nao)
        ex = E.exact_eri(chi, cell.a, cell.mesh, kpts, coords, k1, k2, k3, k4)
        ref = np.einsum("IJ,Im,In,Jk,Jl->mnkl", o["wq"][q], x[k1].conj(), x[k2], x[k3].conj(),
                        x[k4], optimize=True)
        print(k1, k2, k3, k4, "vs exact", abs(eri - ex).max(), "vs oracle ISDF", abs(eri - ref).max())
        assert abs(eri - ex).max() < 1e-6
        assert abs(eri - ref).max() < 1e-7
    # ao2mo with random MO coefficients equals the AO ERI transformed on the host
    rng = np.random.default_rng(3)
    C = [rng.standard_normal((nao, n)) + 1j * rng.standard_normal((nao, n)) for n in (3, 4, 2, 5)]
    k4 = kidx(ks[3] - ks[5] + ks[6])
    kq = kpts[[3, 5, 6, k4]]
    ao = df.get_eri(kq).reshape(nao, nao, nao, nao)
    mo = df.ao2mo(C, kq).reshape(3, 4, 2, 5)
    ref = np.einsum("mnkl,mi,nj,ka,lb->ijab", ao, C[0].conj(), C[1], C[2].conj(), C[3],
                    optimize=True)
    assert abs(mo - ref).max() < 1e-10 * max(1.0, abs(ref).max())
    with pytest.raises(ValueError):
        df.get_eri(kpts[[0, 1, 1, 3]])   # violates k1 - k2 + k3 - k4 = G


def test_jk_row_blocks_sum_to_full():
    """fisdf_get_j_rows / fisdf_get_k_rows over a partition of the interpolation points sum
    to the full J / K (the sharded get_jk all-reduces exactly these partial sums)."""
    from fisdf import _lib as L
    name = "toy222"
    df, o, dm = make_df(name)
    df.build()
    vj_full, vk_full = df.get_jk(dm)
    d = df.device
    st = df._dev_state
    nip = st["X"].shape[1]
    nset, nk, nao = dm.shape[:3]
    ddm = d.to_dev(np.ascontiguousarray(dm, dtype=np.complex128))
    km, kmp = L.iarr(df.kmesh)
    a, ap = L.darr(np.asarray(df.cell.lattice_vectors(), float).ravel())
    cuts = [0, 37, 37, 200, nip]   # includes an empty block
    vj = np.zeros(dm.shape, complex)
    vk = np.zeros(dm.shape, complex)
    for i0, i1 in zip(cuts[:-1], cuts[1:]):
        pj = d.empty(dm.shape)
        pk = d.empty(dm.shape)
        d.ctx.call("fisdf_get_j_rows", L.ptr(st["X"]), L.ptr(st["W0"]), L.ptr(ddm), nset, nk, nip,
                   nao, i0, i1, L.ptr(pj))
        d.ctx.call("fisdf_get_k_rows", L.ptr(st["X"]), L.ptr(st["Ws"]), L.ptr(ddm), nset, nip, nao,
                   kmp, ap, i0, i1, L.ptr(pk))
        vj += pj.cpu().numpy()
        vk += pk.cpu().numpy()
    scale = max(abs(vk_full).max(), 1.0)
    assert abs(vj.real - vj_full).max() < 1e-12 * scale if np.isrealobj(vj_full) else \
        abs(vj - vj_full).max() < 1e-12 * scale
    assert abs(vk - vk_full).max() < 1e-12 * scale


def test_exxdiv_ewald():
    """next-4: exxdiv='ewald' = exxdiv=None K + madelung * S_k D_k S_k (PySCF
    _ewald_exxdiv_for_G0), S_k the FFT-grid overlap; J unchanged.  Checked against the oracle K
    plus the same correction formed on the host from the oracle's AO inputs."""
    from fisdf.cell import madelung
    df, o, dm = make_df("toy222")
    df.build()
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs("toy222")
    vj0, vk0 = df.get_jk(dm)
    vj1, vk1 = df.get_jk(dm, exxdiv="ewald")
    assert abs(vj1 - vj0).max() == 0.0
    S = np.einsum("kgm,kgn->kmn", chi.conj(), chi) * (cell.vol / chi.shape[1])
    assert abs(df.get_ovlp().cpu().numpy() - S).max() < 1e-12 * max(1.0, abs(S).max())
    mad = madelung(cell, kmesh)
    ref = o["vk"] + mad * np.einsum("kmp,xkpq,kqn->xkmn", S, dm, S)
    err = abs(vk1 - ref).max()
    print("ewald K vs oracle + correction", err, "madelung", mad)
    assert err < JK_TOL
    # the correction is Hermitian for a Hermitian dm, and repeated calls reuse the cached S
    d = vk1 - vk0
    assert abs(d - d.conj().swapaxes(-1, -2)).max() < 1e-12
    _, vk2 = df.get_jk(dm, exxdiv="ewald")
    assert abs(vk2 - vk1).max() == 0.0


@pytest.mark.parametrize("omega", [0.4, -0.4])
def test_range_separated_omega(omega):
    """next-4: get_jk(omega=w) = the ISDF J/K with PySCF get_coulG's range-separated kernel
    (w > 0 long range erf, w < 0 short range erfc) — the oracle rebuilt with coulG(omega) on the
    same points; the plain-Coulomb state is untouched and the omega state is cached."""
    from oracle import isdf_ref as R
    name = "toy331_fr"
    df, o, dm = make_df(name)
    df.build()
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    vj0, vk0 = df.get_jk(dm)
    vj, vk = df.get_jk(dm, omega=omega)
    out = R.build(o["xip"], chi, coords, cell.a, kmesh, cell.mesh, omega=omega)
    kpts = R.get_kpts(cell.a, kmesh)
    phase = R.get_phase(cell.a, kpts, kmesh)
    vj_ref = R.get_j_kpts(o["xip"], out["w0"], dm)
    vk_ref = R.get_k_kpts(o["xip"], out["wq"], dm, phase)
    ej, ek = abs(vj - vj_ref).max(), abs(vk - vk_ref).max()
    print(f"omega {omega}: |dJ| {ej:.2e} |dK| {ek:.2e}  (|K| {abs(vk_ref).max():.2e})")
    assert ej < JK_TOL and ek < JK_TOL
    assert abs(vk - vk0).max() > 1e-3            # a different kernel
    vj1, vk1 = df.get_jk(dm)
    assert abs(vj1 - vj0).max() == 0.0 and abs(vk1 - vk0).max() == 0.0
    assert len(df._omega_dfs) == 1


@pytest.mark.parametrize("name,piv", [("toy333_fr", None), ("toy222", None), ("toy331", True)])
def test_fit_schedule_invariance(name, piv):
    """W_q does not depend on the fit schedule: 1/2/3 MFMA lanes, the FFT in-lane or
    on the pipelined stream with ring depths 2..lanes+2 — same kernels, same per-q arithmetic,
    bitwise equal W_q.  Covers self-conjugate q (toy222: all q), complex q (toy333_fr) and the
    forced pivoted, rank-deficient factorisation (toy331)."""
    import ctypes as C
    base = None
    for lanes, mode, depth in [(1, 0, 0), (2, 0, 0), (3, 0, 0), (2, 1, 0), (3, 1, 0), (2, 1, 2),
                               (3, 1, 3)]:
        df, o, dm = make_df(name, pivoted=piv)
        d = df.device
        d.ctx.call("fisdf_set_fit_lanes", lanes)
        d.ctx.call("fisdf_set_fit_pipe", mode, depth)
        df.build()
        nl, nd = C.c_int(), C.c_int()
        d.ctx.call("fisdf_fit_info", C.byref(nl), C.byref(nd))
        nq = len(df.my_qs)
        assert nl.value == min(lanes, nq)
        assert nd.value == (0 if mode == 0 or nq < 2 or lanes < 2 else
                            min(nq, depth if depth else min(lanes, nq, 3) + 2))
        wq = df._wq
        if base is None:
            base = wq
        print(f"{name} lanes {lanes} pipe {mode} ring {nd.value}: max|W - W(1 lane)| "
              f"{abs(wq - base).max():.1e}")
        assert abs(wq - base).max() == 0.0


def test_arena_failed_growth_is_recoverable():
    """a failed arena growth leaves an empty arena (not a stale size over a null
    base); the next small request allocates a real buffer and the kernels using it are right."""
    import torch
    from fisdf._lib import FisdfError
    df, o, dm = make_df("toy222")
    d = df.device
    with pytest.raises(FisdfError):
        d.ctx.call("fisdf_reserve_workspace", 1 << 52)      # 4 PB
    from fisdf import _lib as L
    g = torch.Generator().manual_seed(5)
    A = torch.randn(96, 700, dtype=torch.complex128, generator=g)
    B = torch.randn(700, 80, dtype=torch.complex128, generator=g)
    dA, dB = A.to(d.dev), B.to(d.dev)
    dC = torch.zeros(96, 80, dtype=torch.complex128, device=d.dev)
    one, zero = np.array([1.0, 0.0]), np.zeros(2)
    d.ctx.call("fisdf_zgemm", 0, 0, 96, 80, 700, one.ctypes.data_as(L._dp), L.ptr(dA), 700, 0,
               L.ptr(dB), 80, 0, zero.ctypes.data_as(L._dp), L.ptr(dC), 80, 0, 1, 4)  # split-K: arena
    ref = A @ B
    assert (dC.cpu() - ref).abs().max() < 1e-12 * ref.abs().max()


def test_time_reversal_guard():
    """Bloch AO inputs without x_{-k} = conj(x_k) — here a k-dependent phase
    e^{i theta_k} with theta_{-k} != -theta_k — fail fisdf_build's device check, and the build fits
    every q (the reference's own path) instead of trusting W_{-q} = conj(W_q).  The oracle runs on
    the same inputs; the ISDF quantities are gauge invariant, so J/K also equal the untransformed
    case's."""
    from fisdf import ISDF
    from oracle import isdf_ref as R
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs("toy331_fr")
    o = oracle("toy331_fr")
    nk = int(np.prod(kmesh))
    ph = np.exp(1j * 0.37 * (1 + np.arange(nk)))
    x0g, chig = x0 * ph[:, None, None], chi * ph[:, None, None]
    perm = o["perm"]
    out = R.build(x0g[:, perm], chig, coords, cell.a, kmesh, cell.mesh)
    phase = R.get_phase(cell.a, R.get_kpts(cell.a, kmesh), kmesh)
    vj0 = R.get_j_kpts(x0g[:, perm], out["w0"], dm)
    vk0 = R.get_k_kpts(x0g[:, perm], out["wq"], dm, phase)
    df = ISDF(cell, cell.get_kpts(kmesh), m0=list(m0), c0=c0)
    d = df.device
    df._kmesh()
    df._ao_parent, df._ao_grid = d.to_dev(x0g), d.to_dev(chig)
    df.set_interpolation_points(perm)
    df.build()
    vj, vk = df.get_jk(dm)
    ej, ek = abs(vj - vj0).max(), abs(vk - vk0).max()
    print(f"toy331_fr gauge-twisted: time reversal used {df.time_reversal_used}, deviation "
          f"{df.tr_deviation:.2e}, fitted q {len(df.fit_qs)}/{nk}: |dJ|={ej:.2e} |dK|={ek:.2e}; "
          f"vs untwisted {abs(vj - o['vj']).max():.2e} / {abs(vk - o['vk']).max():.2e}")
    assert not df.time_reversal_used and df.tr_deviation > 1e-3
    assert len(df.fit_qs) == nk
    assert ej < JK_TOL and ek < JK_TOL
    assert abs(vj - o["vj"]).max() < JK_TOL and abs(vk - o["vk"]).max() < JK_TOL
    # the untwisted inputs pass the check and fold (the default path)
    df2, _, _ = make_df("toy331_fr")
    df2.build()
    assert df2.time_reversal_used and df2.tr_deviation < 1e-12, df2.tr_deviation
    assert len(df2.fit_qs) < nk


@pytest.mark.parametrize("name", ["toy222", "toy331_fr", "toy333_fr", "diamond_szv_gamma",
                                  "toy222_rank", "toy666"])
def test_streamed_y_matches(name):
    """The y build streamed behind the selection (fisdf_build: y formed in blocks of pivots on a
    second stream while the cooperative selection kernel publishes them) gives the build of the
    unstreamed path bit for bit: same points, W_q, W_s and J/K.  It engages when the selection
    returns the point cap under time reversal on a k-mesh the fused y kernel covers; otherwise
    (a rank-deficient parent Gram, toy222_rank; a 6x6x6 mesh) the streamed y is discarded or
    never started, and the result is again that of the unstreamed build."""
    import os
    res = {}
    for on in ("0", "1"):
        os.environ["FISDF_Y_STREAM"] = on
        try:
            df, o, dm = make_df(name, inject=False)
            df.build()
            vj, vk = df.get_jk(dm)
            st = df._dev_state
            res[on] = (df.perm.copy(), st["Wq"].cpu().numpy(), st["Ws"].cpu().numpy(), vj, vk,
                       df.y_streamed, df.nip)
        finally:
            os.environ.pop("FISDF_Y_STREAM", None)
    a, b = res["0"], res["1"]
    cell, kmesh, m0, c0, *_ = inputs(name)
    cap = min(int(cell.nao_nr() * c0), int(np.prod(m0)))
    print(f"\n{name}: nip {b[6]} (cap {cap}), streamed {b[5]} (unstreamed run {a[5]})")
    assert not a[5]
    assert np.array_equal(a[0], b[0])
    for i, what in ((1, "W_q"), (2, "W_s"), (3, "J"), (4, "K")):
        assert np.array_equal(a[i], b[i]), what
    fused = name != "toy666"          # k-meshes with a fused y kernel (linalg.hip yf_launch)
    # the cooperative selection (the kernel that publishes its pivots) runs below 800 pivots,
    # on a parent grid of at least 64 points, when its scratch fits (fewer pivots than points)
    ng0 = int(np.prod(m0))
    coop = cap < 800 and ng0 >= 64 and cap < ng0
    assert b[5] == (fused and coop and b[6] == cap)


@pytest.mark.parametrize("name", ["toy222", "toy331_fr"])
@pytest.mark.parametrize("rows,two", [("16", "1"), ("48", "0"), ("256", "1")])
def test_streamed_y_variants(name, rows, two):
    """The streamed y's schedule does not change its result: pivot blocks of 16 / 48 / 256 rows
    (FISDF_Y_STREAM_ROWS) on one stream or two (FISDF_Y_STREAM_2S) give the unstreamed build's
    W_q, W_s and J/K bit for bit."""
    import os
    env = {"FISDF_Y_STREAM_ROWS": rows, "FISDF_Y_STREAM_2S": two}
    res = {}
    for on in ("0", "1"):
        os.environ["FISDF_Y_STREAM"] = on
        os.environ.update(env)
        try:
            df, o, dm = make_df(name, inject=False)
            df.build()
            vj, vk = df.get_jk(dm)
            st = df._dev_state
            res[on] = (st["Wq"].cpu().numpy(), st["Ws"].cpu().numpy(), vj, vk, df.y_streamed,
                       df.nip)
        finally:
            for k in ["FISDF_Y_STREAM", *env]:
                os.environ.pop(k, None)
    a, b = res["0"], res["1"]
    print(f"\n{name} rows {rows} 2s {two}: nip {b[5]}, streamed {b[4]}")
    assert b[4] and not a[4]
    for i, what in ((0, "W_q"), (1, "W_s"), (2, "J"), (3, "K")):
        assert np.array_equal(a[i], b[i]), what


def _build_env(name, env, inject=False):
    import os
    os.environ.update(env)
    try:
        df, o, dm = make_df(name, inject=inject)
        df.build()
        vj, vk = df.get_jk(dm)
        st = df._dev_state
        return (st["Wq"].cpu().numpy(), st["Ws"].cpu().numpy(), vj, vk), o, df
    finally:
        for k in env:
            os.environ.pop(k, None)


@pytest.mark.parametrize("name", ["toy222", "toy331_fr", "nio_small"])
@pytest.mark.parametrize("env", [{"FISDF_FAC_EARLY": "0"}, {"FISDF_FAC_EARLY": "5"},
                                 {"FISDF_FACTOR_PRIO": "1"}, {"FISDF_X4_SIDE": "1"}],
                         ids=["early0", "early5", "prio1", "x4side"])
def test_schedule_switches_bitwise(name, env):
    """Round-6 scheduling switches move work between streams or reorder independent launches
    only: the first fitted slots' factor operators built before the rest (FISDF_FAC_EARLY, 0 =
    all at once), the factor chain's stream priority (FISDF_FACTOR_PRIO) and x4 on the side
    stream beside the streamed y (FISDF_X4_SIDE) leave W_q, W_s and J/K bit for bit."""
    ref, _, _ = _build_env(name, {})
    got, _, _ = _build_env(name, env)
    for i, what in enumerate(("W_q", "W_s", "J", "K")):
        assert np.array_equal(ref[i], got[i]), what


@pytest.mark.parametrize("name", ["nio_small", "si_small"])
def test_wpp_split_k(name):
    """W_PP = L^-H G L^-1's two upper-triangular GEMMs split 4-way over K (the default from
    256 points) against the unsplit products (FISDF_WPP_KSPLIT=1): W_q to rounding, J/K vs the
    oracle within the north-star bar both ways.  (Full-rank cases: a rank-deficient q takes the
    blocked back-substitutions instead, where the switch has no effect.)"""
    a, o, df = _build_env(name, {"FISDF_WPP_KSPLIT": "1"}, inject=True)
    b, _, _ = _build_env(name, {}, inject=True)
    assert df.nip >= 256 and min(df.ranks) == df.nip, "case does not split"
    dw = abs(a[0] - b[0]).max() / abs(a[0]).max()
    e = [max(abs(r[2] - o["vj"]).max(), abs(r[3] - o["vk"]).max()) for r in (a, b)]
    print(f"\n{name}: nip {df.nip}: rel |dW_q| split vs unsplit {dw:.1e}; |dJK| vs oracle "
          f"unsplit {e[0]:.2e} split {e[1]:.2e}")
    assert 0 < dw < 1e-12       # the split ran (another summation order), to rounding
    assert max(e) < JK_TOL


@pytest.mark.parametrize("name", ["toy222", "toy331_fr", "toy333_fr", "nio_small"])
def test_get_k_register_transform(name):
    """get_k's k-mesh transform pair (rho_s = Phi rho_k, V_s = W_s Re(rho_s), V_k = Phi^T V_s,
    fftisdf.py:211-222) in one register pass per column equals the two dense Phi GEMMs with the
    product in the first one's epilogue (FISDF_K_DFT=0) to rounding, and the oracle's K."""
    import os
    df, o, dm = make_df(name)
    df.build()
    res = {}
    for on in ("0", "1"):
        os.environ["FISDF_K_DFT"] = on
        try:
            res[on] = df.get_jk(dm)
        finally:
            os.environ.pop("FISDF_K_DFT", None)
    scale = max(1.0, abs(res["0"][1]).max())
    d = abs(res["1"][1] - res["0"][1]).max() / scale
    ek = abs(res["1"][1] - o["vk"]).max()
    print(f"\n{name}: |K(register) - K(GEMMs)| / max|K| = {d:.1e}; |dK| vs oracle {ek:.2e}")
    assert d < 1e-13
    assert ek < JK_TOL
    assert np.array_equal(res["1"][0], res["0"][0])     # J untouched
