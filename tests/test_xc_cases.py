"""CPU checks of tests/xc_cases.py: the reference gradient against central differences of
ao_cases' long-double value reference, the host restatement fisdf.cell.eval_ao_*(deriv=1) against
the reference, the consistency of the rho / V / T references, the input condition of the new
evaluator cases, and the coverage of the restated launch rules."""
import numpy as np
import pytest

import ao_cases as A
import kmesh_cases as K
import xc_cases as X

H = 1e-4        # bohr


def _fd(tab, coords, kmesh, kband, h):
    """central differences of the long-double value reference, (nk, 3, ng, nao)"""
    out = []
    for c in range(3):
        e = np.zeros(3, X.LD)
        e[c] = X.LD(h)
        co = np.asarray(coords, X.LD)
        if kband is None:
            p, m = A.kmesh_sum(tab, co + e, kmesh).chi, A.kmesh_sum(tab, co - e, kmesh).chi
        else:
            p, m = A.band_sum(tab, co + e, kband).chi, A.band_sum(tab, co - e, kband).chi
        out.append((p - m) / (2 * X.LD(h)))
    return np.stack(out, axis=1)


@pytest.mark.parametrize("kmesh,kband", [((2, 2, 2), None), (None, "off3")], ids=["kmesh", "band"])
def test_reference_gradient_against_central_differences(kmesh, kband):
    """The truncation term is O(h^2) and long-double rounding sits near 1e-15: the max-norm error
    at h is 4 times the one at h / 2, within 5 %."""
    tab = A.raw_tables("mixed", "box", A.RCUT)
    coords = A.raw_points(6, seed=11)
    kb = None if kband is None else A.band_kpts(kband)
    # no (point, atom, T) triple may cross the cutoff under the shifts
    inr = {A.near_cutoff(tab, coords + s * np.eye(3)[c] * H)[1] for s in (-1, 0, 1) for c in range(3)}
    assert len(inr) == 1
    ref = (X.kmesh_sum4(tab, coords, kmesh) if kb is None else X.band_sum4(tab, coords, kb)).chi
    assert np.array_equal(ref[:, 0], (A.kmesh_sum(tab, coords, kmesh) if kb is None
                                      else A.band_sum(tab, coords, kb)).chi)
    e1 = np.abs(_fd(tab, coords, kmesh, kb, H) - ref[:, 1:]).max()
    e2 = np.abs(_fd(tab, coords, kmesh, kb, H / 2) - ref[:, 1:]).max()
    print(f"central differences: error {float(e1):.3e} at h, {float(e2):.3e} at h/2, ratio {float(e1 / e2):.4f}")
    assert e1 > 0 and abs(float(e1 / e2) - 4) <= 0.05 * 4


def test_gradients_at_the_origin_are_finite():
    """On an atom: s has no gradient, p the constant one, d and f none (polynomials, no 1/r)."""
    z = np.zeros(1, X.LD)
    for l in range(4):
        g = np.array([[float(c[0]) for c in comp] for comp in X.sph_grad(l, z, z, z)])
        assert np.all(np.isfinite(g))
        if l == 1:
            want = float(np.sqrt(X.LD(3) / (4 * A.PI)))
            assert np.allclose(g, want * np.eye(3), rtol=1e-15, atol=0)
        else:
            assert not g.any()
    from fisdf import cell as C
    z64 = np.zeros(1)
    for l in range(4):
        got = np.array([[float(c[0]) for c in comp] for comp in C._real_sph_grad(l, z64, z64, z64)])
        ref = np.array([[float(c[0]) for c in comp] for comp in X.sph_grad(l, z, z, z)])
        assert np.allclose(got, ref, rtol=4e-16, atol=0)


@pytest.mark.parametrize("c", X.EV_CASES, ids=X.ev_id)
def test_evaluator_cases_keep_off_the_cutoff(c):
    tab, coords, kband = X.ev_inputs(c)
    assert A.near_cutoff(tab, coords)[0] == 0
    if c.atom:          # point 0 sits on atom 1 + ATOM_T to rounding
        d = coords[0] - (np.asarray(tab.atoms)[1] + np.asarray(X.ATOM_T) @ np.asarray(tab.a))
        assert np.abs(d).max() == 0
        assert list(X.ATOM_T) in np.asarray(tab.tn).tolist()


def test_evaluator_cases_cover_every_branch():
    hit = set()
    for c in X.EV_CASES:
        hit |= X.ev_branches(c)
    assert X.EV_BRANCHES <= hit, X.EV_BRANCHES - hit
    assert K.route((2, 2, 2))[0] == K.REG and K.route((1, 1, 3))[0] == K.LDS


@pytest.mark.parametrize("name", ["toy_grid_222", "diamond_rand_312", "nio_grid_band"])
def test_host_restatement_against_the_reference(name):
    """fisdf.cell.eval_ao_kpts / eval_ao_band (deriv=1) within the column bound, per component."""
    from fisdf import cell as C
    c = A.REAL_BY_NAME[name]
    cell = A.real_cell(c.cell, c.mesh)
    coords = A.real_points(c)
    tab = A.real_tables(cell, coords)
    assert A.near_cutoff(tab, coords)[0] == 0
    if c.kmesh is None:
        kb = A.band_kpts(c.kband, tab.a)
        wide, f64 = X.band_sum4(tab, coords, kb, True), X.band_sum4(tab, coords, kb, False)
        got = C.eval_ao_band(cell, coords, kb, deriv=1)
        assert np.array_equal(got[:, 0], C.eval_ao_band(cell, coords, kb))
        assert np.array_equal(got, cell.pbc_eval_gto("GTOval_sph_deriv1", coords, kpts=kb))
    else:
        wide, f64 = X.kmesh_sum4(tab, coords, c.kmesh, True), X.kmesh_sum4(tab, coords, c.kmesh, False)
        got = C.eval_ao_kpts(cell, coords, c.kmesh, deriv=1)
        assert np.array_equal(got[:, 0], C.eval_ao_kpts(cell, coords, c.kmesh))
        assert np.array_equal(got, C.bloch_ao(cell, coords, C.make_kpts(cell, c.kmesh), c.kmesh, deriv=1))
    assert got.shape == wide.chi.shape
    err, e64 = X.col_err4(got, wide.chi), X.col_err4(f64.chi, wide.chi)
    tol = np.vectorize(lambda e: X.bound(e, wide.nsum))(e64)
    print(f"{name}: largest error {err.max():.2e}, largest error / bound {(err / tol).max():.2f}")
    assert np.all(err <= tol), (err / tol).max()


def test_pbc_eval_gto_names():
    from fisdf import cell as C
    cell = C.toy_cell(mesh=(3, 3, 3))
    co = cell.gen_uniform_grids((3, 3, 3))[:5]
    assert cell.pbc_eval_gto("GTOval_deriv1", co).shape == (4, 5, 8)
    assert cell.pbc_eval_gto("GTOval_sph_deriv1", co, kpts=np.zeros((2, 3))).shape == (2, 4, 5, 8)
    assert cell.pbc_eval_gto("GTOval", co).shape == (5, 8)
    with pytest.raises(NotImplementedError):
        cell.pbc_eval_gto("GTOval_sph_deriv2", co)
    with pytest.raises(ValueError):
        C.eval_ao_kpts(cell, co, (1, 1, 2), deriv=2)


@pytest.mark.parametrize("c", [c for c in X.RHO_CASES if c.hermi and c.ng <= 65], ids=X.rho_id)
def test_rho_references_agree_for_hermitian_dms(c):
    f4, D = X.rho_inputs(c)
    h1, h0 = X.rho_gga_ref(f4, D, 1), X.rho_gga_ref(f4, D, 0)
    n = c.nk * c.nao * c.nao
    assert X.rel_err(h1, h0) <= 8 * n * float(np.finfo(X.LD).eps)
    assert not np.asarray(h1[:, 1:].imag, float).any()


@pytest.mark.parametrize("c", [c for c in X.GRAM_CASES if c.ng <= 65], ids=X.gram_id)
def test_v_reference_is_hermitian(c):
    f4, w, P = X.gram_inputs(c)
    v = X.gga_gram_ref(f4, w, 0.7)
    assert X.rel_err(v, v.conj().swapaxes(-1, -2)) <= 8 * 4 * c.ng * float(np.finfo(X.LD).eps)
    # and it is PySCF's aow form: aow = 1/2 w_0 f + sum_c w_c d_c f, V = f^H aow + h.c.
    f4l, wl = f4.astype(X.CLD), w.astype(X.LD)
    for s in range(c.nset):
        for k in range(c.nk):
            aow = 0.5 * wl[s, 0][:, None] * f4l[k, 0] + sum(wl[s, i][:, None] * f4l[k, i] for i in (1, 2, 3))
            m = f4l[k, 0].conj().T @ aow
            assert X.rel_err((m + m.conj().T) * X.LD(0.7), v[s, k]) <= 64 * c.ng * float(np.finfo(X.LD).eps)


def test_kernel_cases_cover_every_branch():
    hit = set()
    for c in X.RHO_CASES:
        hit |= X.rho_branches(*c)
    assert X.RHO_BRANCHES <= hit, X.RHO_BRANCHES - hit
    for hermi in (0, 1):        # every chunk size under both forms
        sizes = set()
        for c in X.RHO_CASES:
            if c.hermi == hermi:
                sizes |= set(X.rho_set_chunks(c.nao, c.nset, c.hermi))
        assert sizes == {1, 2, 3, 4}, (hermi, sizes)
    hit = set()
    for c in X.GRAM_CASES:
        hit |= X.gram_branches(*c)
    assert X.GRAM_BRANCHES <= hit, X.GRAM_BRANCHES - hit
    assert X.rho_set_chunks(76, 5, 0) == [2, 2, 1] and X.rho_set_chunks(76, 5, 1) == [4, 1]
    assert X.rho_set_chunks(26, 5, 0) == [4, 1]


def test_identity_is_exact_for_the_references():
    """e = a rho^2 + b sigma is quadratic in D: the central difference with step 1 equals
    (1/nk) sum_k Re tr(V_k delta_k) up to long-double rounding."""
    c = X.RhoCase(8, 65, 2, 1, 1)
    f4, D = X.rho_inputs(c)
    _, dl = X.rho_inputs(X.RhoCase(8, 65, 2, 2, 1))
    D, dl = X.quantize(D), X.quantize(dl[1:])
    vol = 3.1
    rho = lambda d: X.rho_gga_ref(f4, d, 1)[0].real
    ep, em = X.energy(rho(D + dl), vol), X.energy(rho(D - dl), vol)
    lhs = (ep - em) / 2
    V = X.gga_gram_ref(f4, X.identity_wv(rho(D))[None], X.LD(vol) / c.ng)[0]
    rhs = sum(np.trace(V[k] @ dl[0, k].astype(X.CLD)).real for k in range(c.nk)) / c.nk
    # the two energies cancel in lhs: rounding is relative to them
    assert abs(lhs - rhs) <= c.ng * float(np.finfo(X.LD).eps) * (abs(ep) + abs(em) + abs(rhs))
    assert abs(lhs) > 1e-3 * (abs(ep) + abs(em))
