"""tests/jk_cases.py on the CPU: the project's float64 oracle (oracle/isdf_ref.py get_j_kpts,
get_k_kpts) and the einsum of test_get_eri_and_ao2mo agree with the long-double references within
the bounds the device is held to; the bounds see each of nine subtle faults planted in the float64
restatements (error / bound above 100 on the case named beside it); the case tables reach every
branch they are there for.  No GPU."""
import numpy as np
import pytest

import jk_cases as J
from oracle import isdf_ref as R

ANCHOR_MESHES = [(1, 1, 1), (2, 2, 2), (3, 3, 1), (1, 1, 3)]


def ratio(got, ref, tol):
    return J.worst_ratio(J.block_err(got, ref), tol)


# ---- the oracle against the references -----------------------------------------------------------
@pytest.mark.parametrize("km", ANCHOR_MESHES, ids=str)
def test_oracle_j_matches_the_reference(km):
    nk, nip, nao, nset, nkb = J.nk_of(km), 37, 5, 3, 3
    rng = np.random.default_rng(11 + nk)
    X, W0 = J.make_x(rng, km, nip, nao, True), J.rnd(rng, nip, nip)
    D, Xb = J.make_dm(rng, km, nset, nao, True), J.rnd(rng, nkb, nip, nao)
    n = J.j_chain(nk, nao, nip, nip)
    for xb in (None, Xb):
        ref = J.j_rows(X, W0, D, 0, nip, Xb=xb)
        tol = J.block_bound(J.j_rows(X, W0, D, 0, nip, Xb=xb, wide=False), ref, n)
        r = ratio(R.get_j_kpts(X, W0, D, xband=xb), ref, tol)
        print(f"oracle J {km} band {xb is not None}: error / bound {r:.2f}")
        assert r <= 1


@pytest.mark.parametrize("km", ANCHOR_MESHES, ids=str)
def test_oracle_k_matches_the_reference(km):
    """W_s rebuilt from a W_q stack with W_{-q} = conj(W_q): sqrt(nk) Re(Phi W_q), the reference
    in long double, the oracle and the restatement in float64."""
    nk, nip, nao, nset = J.nk_of(km), 37, 5, 2
    rng = np.random.default_rng(23 + nk)
    X, D = J.make_x(rng, km, nip, nao, True), J.make_dm(rng, km, nset, nao, True)
    Wq = J.tr_symmetric(rng, km, nip, nip)
    ref, mon, scale = J.k_rows(X, J.ws_from_wq(Wq, km), D, km, 0, nip)
    assert mon < 1e-15 * scale                                 # symmetric inputs: rho_s is real
    phase = R.get_phase(J.LATTICE, R.get_kpts(J.LATTICE, km), km)
    ws64 = (phase @ Wq.reshape(nk, -1)).reshape(nk, nip, nip).real * np.sqrt(nk)
    r64, _ = J.k64(X, ws64, D, km, 0, nip, dense=nk > 1)
    tol = J.block_bound(r64, ref, J.k_chain(nk, nao, nip, nip))
    r = ratio(R.get_k_kpts(X, Wq, D, phase), ref, tol)
    print(f"oracle K {km}: error / bound {r:.2f}")
    assert r <= 1


def test_eri_einsum_matches_the_reference():
    c = J.ECase(37, 5, 0, "none")
    d = J.e_data(c)
    x = [d.X[k] for k in d.kidx]
    got = np.einsum("IJ,Im,In,Jk,Jl->mnkl", d.W, x[0].conj(), x[1], x[2].conj(), x[3],
                    optimize=True).reshape(c.nao ** 2, c.nao ** 2)
    r = ratio(got, d.ref, d.tol)
    print(f"ERI einsum: error / bound {r:.2f}")
    assert r <= 1


def test_phi_is_symmetric_on_a_k_mesh():
    """Phi[R, k] = exp(2 pi i sum_a r_a k_a / n_a) / sqrt(nk) = Phi[k, R]: putting Phi where Phi^T
    belongs is no fault on a k-mesh, so the planted fault of that family is conj(Phi) (the
    transform back run with the sign of the transform forth), the mistake next to it that is
    one."""
    for km in [(3, 2, 1), (1, 1, 3), (3, 3, 3)]:
        phi = J.mesh_dft(np.eye(J.nk_of(km)), km)
        assert np.array_equal(phi, phi.T)
        assert abs(phi - phi.conj()).max() > 0.5 / np.sqrt(J.nk_of(km))
        assert abs(J.device_phase64(km) - phi).max() < 1e-14


# ---- the bounds see subtle faults ------------------------------------------------------------------
J_FAULTS = {   # fault -> the case (and block) that must show it
    "rho_conj_dropped": (J.JCase((2, 2, 2), 13, 64, 3, 0, 0), (0, 64)),
    "rho_without_1_over_nk": (J.JCase((2, 2, 2), 8, 64, 1, 1, 0), (0, 64)),
    # nk nao = 65: a single term of the sum, t = 64, is lost
    "rho_lanes_from_64_skipped": (J.JCase((1, 1, 1), 65, 37, 1, 1, 0), (0, 37)),
    "row_offset_off_by_one": (J.JCase((3, 3, 3), 5, 130, 1, 0, 0), (37, 70)),
    "v_of_another_set": (J.JCase((1, 1, 1), 5, 37, 3, 0, 0), (0, 37)),
}
K_FAULTS = {
    "row_offset_off_by_one": (J.KCase((2, 2, 2), 37, 5, 2, 0, None), (0, 1)),
    "w_s_of_the_next_R": (J.KCase((1, 1, 2), 9, 3, 1, 0, None), (0, 9)),
    "rho_s_not_transposed": (J.KCase((2, 2, 2), 37, 5, 2, 0, None), (0, 37)),
    "phi_conj_for_phi_T": (J.KCase((3, 3, 1), 9, 3, 1, 0, None), (0, 9)),
}


@pytest.mark.parametrize("fault", sorted(J_FAULTS))
def test_j_bound_sees(fault):
    c, (i0, i1) = J_FAULTS[fault]
    assert c in J.J_CASES
    d = J.j_data(c)
    ref, tol = J.j_expect(c, i0, i1)
    clean = ratio(J.j_rows(d.X, d.W0, d.D, i0, i1, wide=False), ref, tol)
    bad = ratio(J.j_rows(d.X, d.W0, d.D, i0, i1, wide=False, fault=fault), ref, tol)
    print(f"J {fault} on {J.case_id(c)} [{i0},{i1}): error / bound {bad:.3g} (clean {clean:.3g})")
    assert clean <= 1 and bad > 100


@pytest.mark.parametrize("fault", sorted(K_FAULTS))
def test_k_bound_sees(fault):
    c, (i0, i1) = K_FAULTS[fault]
    assert c in J.K_CASES
    d, e = J.k_data(c), J.k_expect(c, i0, i1)
    dense = J.k_route(c) == "dense"
    clean = ratio(J.k64(d.X, d.Ws, d.D, c.kmesh, i0, i1, dense=dense)[0], e.ref, e.tol)
    bad = ratio(J.k64(d.X, d.Ws, d.D, c.kmesh, i0, i1, dense=dense, fault=fault)[0], e.ref, e.tol)
    print(f"K {fault} on {J.case_id(c)} [{i0},{i1}): error / bound {bad:.3g} (clean {clean:.3g})")
    assert clean <= 1 and bad > 100


def test_eri_bound_sees_conj_on_the_wrong_pair_factor():
    c = J.ECase(37, 5, 0, "1_and_3")
    assert c in J.E_CASES
    d = J.e_data(c)
    bad = ratio(J.eri(d.X, d.kidx, d.W, d.Cs, wide=False, fault="conj_on_the_wrong_pair_factor"),
                d.ref, d.tol)
    print(f"ERI conj on the wrong factor on {J.case_id(c)}: error / bound {bad:.3g}")
    assert bad > 100


def test_per_block_bounds_see_a_leak_between_sets():
    """the sets are scaled 1, 1e3, 1e-3: a part in 1e14 of set 1 added to set 2 is below n eps of
    the whole output's size and far above the bound of set 2's blocks."""
    c = J.JCase((2, 2, 2), 13, 64, 3, 0, 0)
    assert c in J.J_CASES
    ref, tol = J.j_expect(c, 0, c.nip)
    got = np.asarray(ref, complex)
    got[2] += 1e-14 * got[1]
    n = J.j_chain(J.nk_of(c.kmesh), c.nao, c.nip, c.nip)
    assert J.block_err(got, ref).max() < n * J.EPS * J.block_scale(ref).max()
    assert ratio(got, ref, tol) > 100


def test_monitor_reference_carries_information():
    sym = J.k_expect(J.KCase((2, 2, 2), 70, 13, 1, 1, None), 0, 70)
    gen = J.k_expect(J.KCase((2, 2, 2), 37, 5, 2, 0, None), 0, 37)
    assert sym.mon <= 1e-15 * sym.scale and gen.mon > 0.1 * gen.scale


# ---- the tables ------------------------------------------------------------------------------------
def test_j_table_reaches_every_branch():
    reached = set().union(*(J.j_reaches(c) for c in J.J_CASES + J.J_BAND_CASES))
    assert reached >= J.J_BRANCHES, J.J_BRANCHES - reached
    pairs = {(c.kmesh, c.nao, c.nip) for c in J.J_CASES}
    assert pairs == {(km, nao, nip) for km, nao in J.J_MESH_NAO for nip in J.J_NIP}
    assert sorted({J.nk_of(km) * nao for km, nao in J.J_MESH_NAO}) == [5, 63, 64, 65, 104, 135]
    assert {c.nset for c in J.J_CASES} == {1, 3}
    assert {(J.nk_of(c.kmesh), c.nkb) for c in J.J_BAND_CASES} == {(8, 1), (8, 3), (8, 11), (27, 3)}
    assert (37, 70) in J.row_blocks(70) and (37, 70) in J.row_blocks(130)
    for nip in J.J_NIP:
        p = J.partition(nip)
        assert len(p) == 4 and p[0][0] == 0 and p[-1][1] == nip
        assert all(a[1] == b[0] for a, b in zip(p[:-1], p[1:]))
        assert any(i0 == i1 for i0, i1 in J.row_blocks(nip))


def test_k_table_reaches_every_branch():
    reached = set().union(*(J.k_reaches(c) for c in J.K_CASES))
    assert reached >= J.K_BRANCHES, J.K_BRANCHES - reached
    for km in J.K_REG:                                   # each register mesh again under K_DFT = 0
        assert {c.kdft for c in J.K_CASES if c.kmesh == km and (c.nip, c.nao) == (9, 3)} \
            == {None, "0"}
    for km in J.K_NO_REG:
        assert km not in J.REG_MESHES
        assert all(J.k_route(c) == "dense" for c in J.K_CASES if c.kmesh == km)
    assert {(c.nip, c.nao) for c in J.K_CASES} >= set(J.K_SHAPES)
    assert {(c.nip, c.nao) for c in J.K_CASES if c.kmesh == (1, 1, 1)} >= set(J.K_SHAPES)
    assert {c.nset for c in J.K_CASES} == {1, 2}


def test_eri_table_reaches_every_branch():
    reached = set().union(*(J.e_reaches(c) for c in J.E_CASES))
    assert reached >= J.E_BRANCHES, J.E_BRANCHES - reached
    assert len(set(J.E_KIDX[0])) == 4 and len(set(J.E_KIDX[1])) == 1
    assert J.E_WIDTHS["all"] == (3, 4, 2, 5)
    for c in J.E_CASES:
        d = J.e_data(c)
        assert abs(d.W - d.W.conj().T).max() > 1             # not Hermitian
