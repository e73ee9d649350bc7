"""CPU checks of tests/jfft_cases.py and of the exact-J option's host side: the restatements
compose to the oracle's exact_j, the case tables reach every branch of the two kernels' launch
rules, the potential meshes take the routes they are meant to, and the new names are declared."""
import os
import re

import numpy as np
import pytest

import fft_cases as F
import jfft_cases as J
from cases import inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["toy222", "toy331_fr"])
def test_restatement_is_exact_j(name):
    """The float64 restatement of the three stages, composed, is oracle.exact_ref.exact_j."""
    from oracle.exact_ref import exact_j
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs(name)
    ref = exact_j(chi, dm, cell.a, cell.mesh)
    out = J.exact_j64(chi, dm, cell.a, cell.mesh)
    err = abs(out - ref).max() / abs(ref).max()
    print(f"{name}: restatement vs exact_j {err:.2e}")
    assert err < 1e-13


def test_long_double_and_float64_restatements_agree():
    """The two layers state the same sums: float64 is within rounding of long double."""
    c = J.KERNEL_CASES[1]
    f, D, v = J.kernel_inputs(c)
    assert J.rel_err(J.rho_ref(f, D, wide=False), J.rho_ref(f, D)) < J.rho_sum_length(c) * J.EPS
    for cv in (0, 1):
        e = J.rel_err(J.gram_ref(f, v, cv, 0.37, wide=False), J.gram_ref(f, v, cv, 0.37))
        assert e < J.gram_sum_length(c) * J.EPS
    p = J.POTENTIAL_CASES[4]
    rho = J.potential_inputs(p)
    e = J.rel_err(J.potential_ref(rho, J.LATTICE, p.mesh, p.omega, wide=False),
                  J.potential_ref(rho, J.LATTICE, p.mesh, p.omega))
    assert e < 2 * F.TOL
    assert J.rho_ref(f, D).dtype == J.CLD and J.gram_ref(f, v).dtype == J.CLD


def test_omega_variant_of_exact_j():
    """coulG(omega): omega = 0 is exact_j; long range + short range = the full kernel except at
    G = 0, where the short-range limit pi / omega^2 is finite."""
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs("toy222")
    w0, wl, ws = (J.coulG(cell.a, cell.mesh, w) for w in (0.0, 0.4, -0.4))
    assert np.allclose((wl + ws)[1:], w0[1:], rtol=1e-13, atol=0)
    assert w0[0] == 0 and abs(ws[0] - np.pi / 0.16) < 1e-12
    assert abs(J.exact_j64(chi, dm, cell.a, cell.mesh, 0.4)
               - J.exact_j64(chi, dm, cell.a, cell.mesh)).max() > 1e-3


def test_j_method_default_and_check():
    """j_method defaults to the reference's J; a bogus value is refused by get_jk before any
    device access (no GPU needed)."""
    from fisdf import ISDF
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs("toy222")
    assert ISDF.j_method == "isdf"
    df = ISDF(cell, cell.get_kpts(kmesh), m0=list(m0), c0=c0)
    assert df.j_method == "isdf"
    df.j_method = "exact"
    with pytest.raises(ValueError, match="j_method"):
        df.get_jk(dm)
    assert df._d is None                      # no device was opened


def test_names_declared():
    from fisdf import _lib
    hdr = open(os.path.join(ROOT, "include", "fisdf.h")).read()
    for n in ("fisdf_get_rho", "fisdf_coulomb_potential", "fisdf_weighted_gram",
              "fisdf_get_j_fft"):
        assert re.search(r"\b%s\(" % n, hdr), n
        assert n in _lib._SIGS, n
    assert _lib.ABI_VERSION == 4


def test_kernel_cases_reach_every_branch():
    """The rule: every label of RHO_BRANCHES / GRAM_BRANCHES is taken by at least one case, every
    size list of the kernel tests appears, and f_kstride exceeds ngrid * nao in every case."""
    rho, gram = set(), set()
    for c in J.KERNEL_CASES:
        rho |= J.rho_branches(c.nao, c.ngrid, c.nk, c.nset)
        gram |= J.gram_branches(c.nao, c.ngrid, c.nk, c.nset)
    assert J.RHO_BRANCHES <= rho, J.RHO_BRANCHES - rho
    assert J.GRAM_BRANCHES <= gram, J.GRAM_BRANCHES - gram
    assert {c.nao for c in J.KERNEL_CASES} == {1, 8, 26, 33, 76, 130}
    assert {c.ngrid for c in J.KERNEL_CASES} == {64, 997, 1000, 1728}
    assert {c.nk for c in J.KERNEL_CASES} == {1, 2, 27}
    assert {c.nset for c in J.KERNEL_CASES} >= {1, 3, 5}
    assert {c.herm for c in J.KERNEL_CASES} == {True, False}
    assert {c.conj_v for c in J.KERNEL_CASES} == {0, 1}
    assert {(c.herm, c.conj_v) for c in J.KERNEL_CASES} == {(a, b) for a in (True, False)
                                                            for b in (0, 1)}
    assert J.KPAD > 0
    assert len({J.case_id(c) for c in J.KERNEL_CASES}) == len(J.KERNEL_CASES)


def test_gram_split_rule():
    for nk, ngrid, nao in [(1, 64, 1), (64, 46656, 26), (1, 997, 130), (27, 1728, 1), (2, 1000, 33)]:
        chunk, nsplit = J.gram_split(nk, ngrid, nao)
        assert chunk % J.GRAM_GT == 0 and (nsplit - 1) * chunk < ngrid <= nsplit * chunk
        assert nsplit == 1 or chunk >= 4 * J.GRAM_GT
    assert J.gram_split(64, 46656, 26) == (2944, 16)


def test_potential_cases_routes():
    """The potential's meshes take the register route, a plane-kernel route and three axis passes;
    the refused mesh is one fft3d refuses."""
    for c in J.POTENTIAL_CASES:
        assert F.base_route(c.mesh) == J.POTENTIAL_ROUTES[c.mesh], c
        assert F.accepted(c.mesh)
    assert {F.base_route(c.mesh) for c in J.POTENTIAL_CASES} == {F.REG, F.PLANE, F.AXES}
    assert J.AXES_MESH[0] != J.AXES_MESH[1] != J.AXES_MESH[2]
    assert {c.omega for c in J.POTENTIAL_CASES} == {0.0, 0.4, -0.4}
    assert {c.nset for c in J.POTENTIAL_CASES} == {1, 3}
    for mesh in J.POTENTIAL_ROUTES:
        assert {c.omega for c in J.POTENTIAL_CASES if c.mesh == mesh} == {0.0, 0.4, -0.4}
    assert not F.accepted(J.REFUSED_MESH)
