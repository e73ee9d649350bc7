"""CPU checks of tests/pp_cases.py and fisdf/pp.py: the closed forms of the GTH pseudopotential
against quadrature (the authority over the table of q_{l,i}), the packing of ``_pseudo`` entries,
that the case tables reach every branch, and that the long-double references have the symmetries
of the definitions and can see the mistakes an implementation is likely to make."""
import math

import numpy as np
import pytest

import fft_cases as F
import pp_cases as P
from fisdf import _lib, cell as C, pp

RL = {0: 0.37, 1: 0.48, 2: 0.29, 3: 0.41}
KS = (0.3, 1.1, 2.7, 6.0)


@pytest.mark.parametrize("l", range(4))
@pytest.mark.parametrize("i", (1, 2, 3))
def test_projector_closed_form_against_quadrature(l, i):
    """4 pi int j_l(K r) p_i^l(r) r^2 dr = P_i^l(K) K^l for the projector normalised to 1, at four
    |K|: relative error < 1e-10, for fisdf.pp's float64 formulas and for the references' table."""
    from scipy.integrate import quad
    from scipy.special import spherical_jn
    rl = RL[l]
    norm = quad(lambda r: pp.proj_real_space(l, i, r, rl) ** 2 * r * r, 0, np.inf,
                epsabs=1e-15, epsrel=1e-13)[0]
    assert abs(norm - 1) < 1e-10
    for K in KS:
        val = 4 * math.pi * quad(lambda r: spherical_jn(l, K * r) * pp.proj_real_space(l, i, r, rl)
                                 * r * r, 0, 40 * rl, epsabs=1e-15, epsrel=1e-13, limit=400)[0]
        got = pp.proj_radial(l, i, K, rl) * K ** l
        assert abs(got - val) < 1e-10 * abs(val), (l, i, K, got, val)
        x2 = P.LD(K * rl) ** 2
        wide = (P.q_li(l, i, x2, P.LD) * P.PI ** P.LD(1.25) * P.LD(rl) ** (P.LD(l) + P.LD(1.5))
                * np.exp(-x2 / 2)) * P.LD(K) ** l
        assert abs(float(wide) - val) < 1e-10 * abs(val)


@pytest.mark.parametrize("j", range(4))
def test_local_polynomials_against_quadrature(j):
    """The four Gaussian terms of the local part: the 3-D Fourier transform of
    c_j (r/rloc)^{2j} e^{-r^2 / 2 rloc^2} is (2 pi)^{3/2} rloc^3 e^{-x^2/2} times the j-th
    polynomial; and the erf term's transform, -4 pi Z e^{-x^2/2} / G^2 with the G = 0 remainder
    2 pi Z rloc^2."""
    from scipy.integrate import quad
    from scipy.special import erf, spherical_jn
    rloc = 0.35
    cs = [0.0] * 4
    cs[j] = 1.0
    for G in KS:
        val = 4 * math.pi * quad(lambda r: spherical_jn(0, G * r) * (r / rloc) ** (2 * j)
                                 * math.exp(-0.5 * (r / rloc) ** 2) * r * r, 0, 40 * rloc,
                                 epsabs=1e-15, epsrel=1e-13, limit=400)[0]
        got = float(pp.vloc_radial(G * G, 0.0, rloc, cs))
        assert abs(got - val) < 1e-10 * abs(val)
        atom = P.Atom(np.zeros(3), 0.0, rloc, tuple(cs), (), False)
        assert abs(float(P.vloc_radial(P.LD(G * G), atom)) - val) < 1e-10 * abs(val)
    # G = 0: the Gaussian term's integral, and the remainder of -Z erf(r / sqrt(2) rloc) / r + Z / r
    val0 = 4 * math.pi * quad(lambda r: (r / rloc) ** (2 * j) * math.exp(-0.5 * (r / rloc) ** 2)
                              * r * r, 0, 40 * rloc, epsabs=1e-15, epsrel=1e-13)[0]
    assert abs(float(pp.vloc_radial(0.0, 0.0, rloc, cs)) - val0) < 1e-10 * val0
    rem = 4 * math.pi * quad(lambda r: (1 - erf(r / (math.sqrt(2) * rloc))) * r, 0, 40 * rloc,
                             epsabs=1e-15, epsrel=1e-13)[0]
    assert abs(float(pp.vloc_radial(0.0, 1.0, rloc, ())) - rem) < 1e-10 * rem
    assert abs(rem - 2 * math.pi * rloc ** 2) < 1e-10 * rem


def test_pack_pseudo():
    """Z from nelec, bare atoms, the layout of struct fisdf_pp_atom, the refusals."""
    cell = P.toy_cell((8, 9, 10))
    assert list(cell.atom_charges()) == [4, 18, 18, 6]
    assert [cell.atom_symbol(i) for i in range(cell.natm)] == list(P.SYMBOLS)
    tab = pp.pack_atoms(cell)
    mine = P.pack(P.atoms_of(), _lib)
    assert bytes(tab) == bytes(mine)
    assert [a.bare for a in tab] == [0, 0, 0, 1] and tab[3].z == 6.0
    assert tab[0].z == 4.0 and tab[0].nexp == 2 and tab[0].nl == 2 and list(tab[0].n) == [2, 1, 0, 0]
    assert tab[0].h[0][1] == tab[0].h[0][3] == -1.26
    assert tab[1].z == 18.0 and list(tab[1].n) == [3, 2, 1, 1]
    assert np.allclose([list(a.r) for a in tab], P.ATOM_XYZ, rtol=0, atol=0)
    bare = pp.pack_atoms(cell, bare=True)
    assert [a.bare for a in bare] == [1] * 4 and [a.z for a in bare] == [4.0, 18.0, 18.0, 6.0]
    # an empty _pseudo: the nuclear charges
    assert list(P.toy_cell((8, 9, 10), pseudo={}).atom_charges()) == [14, 28, 28, 6]
    with pytest.raises(KeyError):
        C.nuclear_charge("Uuo")
    ok = P.PSEUDO["Si"]
    for bad in (ok[:2] + [5, [1.0] * 5] + ok[4:],                         # nexp > 4
                ok[:4] + [5] + ok[5:] + [[0.3, 0, []]] * 3,                # l > 3
                ok[:5] + [[0.4, 4, np.eye(4).tolist()]] + ok[6:],          # n_l > 3
                ok[:5] + [[0.4, 2, [[1.0, 0.5], [0.4, 1.0]]]] + ok[6:],    # h not symmetric
                ok[:2] + [1] + ok[3:]):                                    # nexp != len(c)
        with pytest.raises(ValueError):
            pp.parse_entry(bad)


def test_tables_reach_every_branch():
    """Every (l, i), both FFT routes by fft_cases' restated rule, every branch of the overlap's
    restated launch rule, a refused mesh, one and several atom chunks."""
    atoms = P.atoms_of()
    assert {(l, i) for _, l, i, _ in P.row_labels(atoms)} == \
        {(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0), (3, 0)}
    assert P.atom_rows(atoms) == [5, 21, 21, 0] and len(P.row_labels(atoms)) == 47
    # every (l <= 3, i <= 3) of the closed form is covered by the quadrature test instead
    for mesh, route in P.ROUTES.items():
        assert F.route(mesh) == route
    assert not F.accepted(P.REFUSED_MESH)
    assert {n % 2 for n in P.MESHES[1]} == {0, 1}     # every fftfreq wrap: odd and even lengths
    reached = set()
    for c in P.OVERLAP_CASES:
        reached |= P.overlap_branches(c.np, c.nao, P.ngrid_of(c.mesh))
    assert reached == P.OVERLAP_BRANCHES
    assert {c.nao for c in P.OVERLAP_CASES} == {1, 5, 32, 33}
    assert {c.np for c in P.OVERLAP_CASES} >= {1, 47}
    assert P.overlap_split(1728) == (64, 27) and P.overlap_split(720) == (64, 12)
    assert P.overlap_split(17820) == (128, 140) and P.overlap_split(36 ** 3) == (192, 243)
    rows = P.atom_rows(atoms)
    ng = 720
    assert P.chunks(rows, ng) == [(0, 4)]
    assert P.chunks(rows, ng, 21 * 16 * ng) == [(0, 1), (1, 2), (2, 4)]
    assert P.chunks(rows, ng, 26 * 16 * ng) == [(0, 2), (2, 4)]
    assert P.chunks(rows, ng, 21 * 16 * ng - 1) is None
    assert P.chunks([0, 0], ng) == []


def _toy(mesh, ik):
    return P.toy_aos(mesh)[ik], P.KPTS[ik]


@pytest.mark.parametrize("mesh", P.MESHES, ids=str)
def test_references_have_the_symmetries(mesh):
    """Hermitian; unchanged when an atom moves by a lattice vector; Vnl unchanged under a
    permutation of m."""
    atoms = P.atoms_of()
    moved = P.ATOM_XYZ.copy()
    moved[1] += np.array([2, -1, 3]) @ P.LATTICE
    moved[3] += np.array([-1, 0, 1]) @ P.LATTICE
    atoms_moved = P.atoms_of(xyz=moved)
    for ik in (0, 2):
        f, k = _toy(mesh, ik)
        vl = P.vloc_ref(f, mesh, atoms)
        vn = P.vnl_ref(f, mesh, k, atoms)
        sl, sn = float(abs(vl).max()), float(abs(vn).max())
        assert abs(vl - vl.conj().T).max() < 1e-16 * sl
        assert abs(vn - vn.conj().T).max() < 1e-16 * sn
        # the moved position is rounded to float64, |dR| <= eps |R| ~ 2e-15 bohr, which turns
        # every phase by up to |K| |dR| ~ 4e-14 (|K| <= 20 on these meshes): 1e-13, relative
        assert abs(P.vloc_ref(f, mesh, atoms_moved) - vl).max() < 1e-13 * sl
        assert abs(P.vnl_ref(f, mesh, k, atoms_moved) - vn).max() < 1e-13 * sn
        perm = P.vnl_ref(f, mesh, k, atoms, m_perm=lambda l: list(range(2 * l + 1))[::-1])
        assert abs(perm - vn).max() < 1e-16 * sn
    # k = 0 with the real toy AOs: the matrices are real but for the G without a partner -G on an
    # even axis (3e-8 Ha on the 12^3 mesh, 3e-4 on the coarse one), the part get_pp drops at k = 0
    f, k = _toy(mesh, 0)
    full = P.vloc_ref(f, mesh, atoms) + P.vnl_ref(f, mesh, k, atoms)
    print(f"{mesh}: max |Im| at k = 0 before it is dropped {float(abs(full.imag).max()):.2e} Ha")
    dropped = P.pp_ref(f, mesh, k, atoms)
    assert not dropped.imag.any() and np.array_equal(dropped.real, full.real)


def test_inputs_can_see_the_likely_mistakes():
    """Each of: SI conjugated, the G = 0 term left out, h's off-diagonal left out, moves the toy
    cell's matrices by at least 1e-3 Ha."""
    mesh = P.MESHES[0]
    atoms = P.atoms_of()
    f, k = _toy(mesh, 2)
    vl = P.vloc_ref(f, mesh, atoms, wide=False)
    vn = P.vnl_ref(f, mesh, k, atoms, wide=False)
    d_si = abs(P.vloc_ref(f, mesh, atoms, wide=False, si_sign=+1) - vl).max()
    d_g0 = abs(P.vloc_ref(f, mesh, atoms, wide=False, drop_g0=True) - vl).max()
    d_h = abs(P.vnl_ref(f, mesh, k, atoms, wide=False, h_offdiag=False) - vn).max()
    print(f"SI conjugated {d_si:.2e}, G = 0 dropped {d_g0:.2e}, h diagonal only {d_h:.2e} Ha")
    assert d_si >= 1e-3 and d_g0 >= 1e-3 and d_h >= 1e-3


def test_float64_restatements_are_close():
    """The float64 restatements agree with the long-double references to rounding (what the GPU
    bounds are built on)."""
    for mesh in P.MESHES:
        ref, e64 = P.vloc_g_refs(mesh)
        assert e64 < 1e-13
        for ik in range(3):
            assert P.beta_refs(mesh, ik)[1] < 1e-13
    c = P.PP_CASES[1]
    assert P.pp_refs(c)[1] < 1e-12
    assert P.overlap_refs(P.OVERLAP_CASES[1])[1] < 1e-13
    assert _lib.ABI_VERSION == 4
