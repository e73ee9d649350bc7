"""GTH pseudopotentials: PySCF's ``cell._pseudo`` entries packed into the table of
``fisdf_get_pp`` (struct fisdf_pp_atom), and the closed forms of the local and non-local parts in
float64 (the formulas of include/fisdf.h and DESIGN §3.13, which csrc/pp.hip evaluates on the
device).  Only the protocol ``atom_coords()``, ``atom_charges()``, ``atom_symbol(ia)``,
``_pseudo`` and ``natm`` of the cell is used, so a ``pyscf.pbc.gto.Cell`` works as well as
``fisdf.cell.Cell``.

An entry is ``[nelec_per_l, rloc, nexp, [c1..c_nexp], nproj_types, [r_0, n_0, h_0], [r_1, n_1,
h_1], ...]`` with h_l a real symmetric n_l x n_l matrix; Z_ion = sum(nelec_per_l).  An atom whose
symbol has no entry is a bare nucleus of charge ``atom_charges()[ia]``.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib

LMAX, NPROJ_MAX, NEXP_MAX = 3, 3, 4


def q_li(l, i, x2):
    """q_{l,i}(x) of P_i^l(K) = q pi^{5/4} r_l^{l+3/2} e^{-x^2/2}, x = K r_l; i = 1, 2, 3."""
    x4 = x2 * x2
    s = math.sqrt
    table = {
        (0, 1): 4 * s(2.0),
        (0, 2): 8 * s(2.0 / 15) * (3 - x2),
        (0, 3): 16.0 / 3 * s(2.0 / 105) * (15 - 10 * x2 + x4),
        (1, 1): 8 / s(3.0),
        (1, 2): 16 / s(105.0) * (5 - x2),
        (1, 3): 32.0 / 3 / s(1155.0) * (35 - 14 * x2 + x4),
        (2, 1): 8 * s(2.0 / 15),
        (2, 2): 16.0 / 3 * s(2.0 / 105) * (7 - x2),
        (2, 3): 32.0 / 3 * s(2.0 / 15015) * (63 - 18 * x2 + x4),
        (3, 1): 16 / s(105.0),
        (3, 2): 32.0 / 3 / s(1155.0) * (9 - x2),
        (3, 3): 64.0 / 45 / s(1001.0) * (99 - 22 * x2 + x4),
    }
    return table[(l, i)]


def proj_radial(l, i, K, rl):
    """P_i^l(K): 4 pi int_0^inf j_l(K r) p_i^l(r) r^2 dr = P_i^l(K) K^l for the normalised HGH
    projector p_i^l(r) = sqrt(2) r^{l+2(i-1)} e^{-r^2/2 r_l^2} / (r_l^{l+(4i-1)/2}
    sqrt(Gamma(l+(4i-1)/2)))."""
    x2 = (K * rl) ** 2
    return q_li(l, i, x2) * math.pi ** 1.25 * rl ** (l + 1.5) * np.exp(-0.5 * x2)


def proj_real_space(l, i, r, rl):
    """The HGH projector p_i^l(r), normalised to int p^2 r^2 dr = 1."""
    e = l + (4 * i - 1) / 2.0
    return (math.sqrt(2.0) * r ** (l + 2 * (i - 1)) * np.exp(-0.5 * (r / rl) ** 2)
            / (rl ** e * math.sqrt(math.gamma(e))))


def vloc_poly(x2, cs):
    """c1 + c2 (3 - x^2) + c3 (15 - 10 x^2 + x^4) + c4 (105 - 105 x^2 + 21 x^4 - x^6)."""
    c = list(cs) + [0.0] * (4 - len(cs))
    x4 = x2 * x2
    return (c[0] + c[1] * (3 - x2) + c[2] * (15 - 10 * x2 + x4)
            + c[3] * (105 - 105 * x2 + 21 * x4 - x4 * x2))


def vloc_radial(G2, z, rloc, cs):
    """v_a(|G|) of the local part for G^2 (array), G = 0 included (the finite remainder of the erf
    term plus the Gaussian terms; the divergent -4 pi Z / G^2 dropped).  rloc = 0, cs = ():
    a bare nucleus."""
    G2 = np.asarray(G2, float)
    x2 = G2 * rloc * rloc
    gauss = (2 * math.pi) ** 1.5 * rloc ** 3
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.exp(-0.5 * x2) * (-z * 4 * math.pi / G2 + gauss * vloc_poly(x2, cs))
    v0 = 2 * math.pi * z * rloc * rloc + gauss * vloc_poly(0.0, cs)
    return np.where(G2 == 0, v0, v)


def parse_entry(entry):
    """One ``_pseudo`` entry -> (Z, rloc, [c...], [(r_l, n_l, h_l (n_l, n_l))...]); ValueError for
    what the library does not take (l > 3, n_l > 3, nexp > 4) or a malformed entry."""
    nelec, rloc, nexp, cs, ntypes = entry[0], float(entry[1]), int(entry[2]), entry[3], int(entry[4])
    cs = [float(c) for c in cs]
    if nexp > NEXP_MAX or nexp < 0:
        raise ValueError(f"pseudopotential: nexp = {nexp}, at most {NEXP_MAX} local coefficients")
    if len(cs) != nexp:
        raise ValueError(f"pseudopotential: {len(cs)} local coefficients for nexp = {nexp}")
    if not rloc > 0:
        raise ValueError("pseudopotential: rloc must be > 0")
    projs = entry[5:]
    if len(projs) != ntypes:
        raise ValueError(f"pseudopotential: {len(projs)} projector channels for nproj_types = "
                         f"{ntypes}")
    if ntypes > LMAX + 1:
        raise ValueError(f"pseudopotential: angular momentum {ntypes - 1} > {LMAX}")
    out = []
    for l, (rl, nl, hl) in enumerate(projs):
        nl = int(nl)
        if nl > NPROJ_MAX or nl < 0:
            raise ValueError(f"pseudopotential: {nl} projectors for l = {l}, at most {NPROJ_MAX}")
        h = np.asarray(hl, float).reshape(nl, nl) if nl else np.zeros((0, 0))
        if nl and abs(h - h.T).max() > 1e-12 * max(1.0, abs(h).max()):
            raise ValueError(f"pseudopotential: h of l = {l} is not symmetric")
        if nl and not float(rl) > 0:
            raise ValueError(f"pseudopotential: r_l of l = {l} must be > 0")
        out.append((float(rl), nl, h))
    return float(sum(nelec)), rloc, cs, out


def pack_atoms(cell, bare=False):
    """The cell's atoms as a ctypes array of ``_lib.PPAtom`` (struct fisdf_pp_atom).  bare: every
    atom a bare nucleus of charge ``atom_charges()[ia]`` (get_nuc)."""
    natm = int(cell.natm)
    coords = np.asarray(cell.atom_coords(), float).reshape(natm, 3)
    charges = np.asarray(cell.atom_charges())
    pseudo = {} if bare else (getattr(cell, "_pseudo", None) or {})
    tab = (_lib.PPAtom * natm)()
    for ia in range(natm):
        A = tab[ia]
        A.r[:] = coords[ia]
        sym = cell.atom_symbol(ia)
        if sym not in pseudo:
            A.bare, A.z = 1, float(charges[ia])
            continue
        z, rloc, cs, projs = parse_entry(pseudo[sym])
        A.bare, A.z, A.rloc, A.nexp, A.nl = 0, z, rloc, len(cs), len(projs)
        for j, c in enumerate(cs):
            A.c[j] = c
        for l, (rl, nl, h) in enumerate(projs):
            A.rl[l], A.n[l] = rl, nl
            for i in range(nl):
                for j in range(nl):
                    A.h[l][3 * i + j] = h[i, j]
    return tab
