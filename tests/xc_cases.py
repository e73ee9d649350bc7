"""Cases, restated launch rules and references for the AO first derivatives and what is built on
them: fisdf_eval_ao_deriv1 / fisdf_eval_ao_band_deriv1 (csrc/ao.hip, sph.h), fisdf_get_rho_gga and
fisdf_gga_gram (csrc/xc.hip), and ISDF.get_rho(xctype="GGA"), nr_vxc_mat and get_kin.  No tests and
no GPU here: tests/test_xc_cases.py checks this file (and the host restatement fisdf.cell) on the
CPU, tests/test_gpu_xc.py runs the device against it.

References, all in np.longdouble / np.clongdouble and none of them from sph.h or fisdf.cell:
  * the gradients of the real solid harmonics by differentiating ao_cases' exact-integer term
    lists term by term (S_lm = N P(r^2, z) Re / Im (x + i y)^m, product rule);
  * the lattice sums for the raw C-ABI tables as in ao_cases (same mask, same input condition
    near_cutoff(...) == 0), with  d_c [R(r^2) S(d)] = R' 2 d_c S + R d_c S;
  * rho, its gradient, V and T literally from their formulas:
        rho_0   = (1/nk) sum_k sum_mn f[g,m] D[m,n] conj f[g,n]
        d_c rho = (1/nk) sum_k sum_mn (d_c f[g,m] D[m,n] conj f[g,n] + f[g,m] D[m,n] conj d_c f[g,n])
        V_k[m,n] = scale sum_g {w_0 conj f[g,m] f[g,n]
                   + sum_c w_c (conj d_c f[g,m] f[g,n] + conj f[g,m] d_c f[g,n])}
        T_k[m,n] = 1/2 scale sum_g sum_c conj d_c f[g,m] d_c f[g,n].
Beside every long-double sum stands the same sum in float64 / complex128; it only measures what
float64 arithmetic alone costs, and a device result may be factor_cases.bound(err64, n) from the
reference: 16 times that, floored at n eps.
"""
import functools
from collections import namedtuple

import numpy as np

import ao_cases as A
import kmesh_cases as K
from factor_cases import BOUND_FACTOR, CLD, EPS, LD, bound  # noqa: F401
from factor_cases import relerr as rel_err
import fft_cases as F
from jfft_cases import EDGE, JK_TOL, KPAD, SENTINEL  # noqa: F401

CPAD = 7           # extra elements between the components of f4 (f_cstride = ng * nao + CPAD)
RPAD = 11          # extra elements between the rows of rho (rho_cstride = ng + RPAD)
WPAD = 5           # extra elements between the components of w


# ---- gradients of the real solid harmonics -----------------------------------------------------
def sph_grad(l, x, y, z, dt=LD):
    """(d/dx, d/dy, d/dz) of A.sph(l, ...)'s components in A.m_order(l): every factor of
    S_l,+-m = N P(r^2, z) {Re, Im}(x + i y)^m differentiated exactly."""
    x, y, z = (np.asarray(t, dt) for t in (x, y, z))
    r2 = x * x + y * y + z * z
    pi = dt(A.PI)
    zero = np.zeros_like(x)
    out = {}
    for m in range(l + 1):
        terms, (fn, fd) = A._pi_lm_terms(l, m)
        P, Pr, Pz = zero.copy(), zero.copy(), zero.copy()      # P, dP/d(r^2), dP/dz at fixed r^2
        for num, k, pz in terms:
            P = P + dt(num) * r2 ** k * z ** pz
            if k > 0:
                Pr = Pr + dt(num) * k * r2 ** (k - 1) * z ** pz
            if pz > 0:
                Pz = Pz + dt(num) * pz * r2 ** k * z ** (pz - 1)
        c = np.sqrt(dt(fn) / dt(fd)) / dt(2 ** l)
        P, Pr, Pz = P * c, Pr * c, Pz * c
        dP = (2 * x * Pr, 2 * y * Pr, 2 * z * Pr + Pz)
        re, im = np.ones_like(x), zero.copy()                  # (x + i y)^m and ^(m - 1)
        re1, im1 = zero.copy(), zero.copy()
        for _ in range(m):
            re1, im1 = re, im
            re, im = re * x - im * y, re * y + im * x
        dre = (m * re1, -m * im1, zero)                        # d (x + i y)^m = m (x + i y)^(m-1) (dx + i dy)
        dim = (m * im1, m * re1, zero)
        if m == 0:
            n = np.sqrt(dt(2 * l + 1) / (4 * pi))
            out[0] = tuple(n * dP[c_] for c_ in range(3))
        else:
            n = np.sqrt(dt(2 * l + 1) / (2 * pi))
            out[m] = tuple(n * (dP[c_] * re + P * dre[c_]) for c_ in range(3))
            out[-m] = tuple(n * (dP[c_] * im + P * dim[c_]) for c_ in range(3))
    return [out[m] for m in A.m_order(l)]


# ---- the lattice sums with first derivatives ---------------------------------------------------
def _blocks4(tab, coords, wide):
    """A._blocks with the four components: per translation the (4, ng, nao) block (None: nothing
    in range) and the (ng, natm) in-range mask."""
    dt = LD if wide else np.float64
    a = np.asarray(tab.a, dt)
    co, atoms = np.asarray(coords, dt).reshape(-1, 3), np.asarray(tab.atoms, dt)
    exps = np.asarray(tab.exps, dt)
    coefs = np.asarray(tab.coefs_ld if wide and tab.coefs_ld is not None else tab.coefs, dt)
    rc2 = dt(tab.rcut) * dt(tab.rcut)
    ng, nao = len(co), A.nao_of(tab)
    p0 = np.concatenate([[0], np.cumsum(tab.sh_np)])
    for n in np.asarray(tab.tn).reshape(-1, 3):
        T = (dt(int(n[0])) * a[0] + dt(int(n[1])) * a[1]) + dt(int(n[2])) * a[2]
        blk, inr = None, np.zeros((ng, len(atoms)), bool)
        for ia in range(len(atoms)):
            d = co - (atoms[ia] + T) if wide else (co - atoms[ia]) - T
            r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
            m = r2 < rc2
            inr[:, ia] = m
            if not m.any():
                continue
            if blk is None:
                blk = np.zeros((4, ng, nao), dt)
            dm = d[m]
            ao0 = 0
            for i, (sa, l, npr) in enumerate(zip(tab.sh_atom, tab.sh_l, tab.sh_np)):
                l = int(l)
                if sa == ia:
                    rad, drad = np.zeros(int(m.sum()), dt), np.zeros(int(m.sum()), dt)
                    for p in range(p0[i], p0[i] + int(npr)):
                        ex = np.exp(-exps[p] * r2[m])
                        rad = rad + ex * coefs[p]
                        drad = drad + ex * (dt(-2) * exps[p] * coefs[p])        # 2 R'
                    S = A.sph(l, dm[:, 0], dm[:, 1], dm[:, 2], dt)
                    G = sph_grad(l, dm[:, 0], dm[:, 1], dm[:, 2], dt)
                    for j in range(len(S)):
                        blk[0, m, ao0 + j] = rad * S[j]
                        for c in range(3):
                            blk[c + 1, m, ao0 + j] = drad * S[j] * dm[:, c] + rad * G[j][c]
                ao0 += A.NSPH[l]
        yield n, T, blk, inr


Sums4 = namedtuple("Sums4", "chi nsum")


def kmesh_sum4(tab, coords, kmesh, wide=True):
    """chi (nk, 4, ng, nao) of the k-mesh and the length of its longest sum (as A.kmesh_sum)."""
    nimg = K.nk_of(kmesh)
    ng, nao = len(np.reshape(coords, (-1, 3))), A.nao_of(tab)
    Fo = np.zeros((nimg, 4, ng, nao), LD if wide else np.float64)
    cnt = np.zeros((nimg, ng, len(tab.atoms)), np.int64)
    img = A.image_of(tab.tn, kmesh)
    for t, (n, T, blk, inr) in enumerate(_blocks4(tab, coords, wide)):
        cnt[img[t]] += inr
        if blk is not None:
            Fo[img[t]] += blk
    chi = np.zeros(Fo.shape, CLD if wide else np.complex128)
    if ng:
        chi = K.mesh_dft(Fo.reshape(nimg, -1), kmesh, wide=wide, scale=False).reshape(Fo.shape)
    return Sums4(chi, int(cnt.max(initial=0)) * int(max(tab.sh_np)) + nimg)


def band_sum4(tab, coords, kband, wide=True):
    """chi (nkb, 4, ng, nao) at band k-points (as A.band_sum)."""
    dt, cdt = (LD, CLD) if wide else (np.float64, np.complex128)
    kb = np.asarray(kband, dt).reshape(-1, 3)
    ng, nao = len(np.reshape(coords, (-1, 3))), A.nao_of(tab)
    chi = np.zeros((len(kb), 4, ng, nao), cdt)
    for n, T, blk, inr in _blocks4(tab, coords, wide):
        if blk is None:
            continue
        th = (kb[:, 0] * T[0] + kb[:, 1] * T[1]) + kb[:, 2] * T[2]
        ph = np.empty(len(kb), cdt)
        ph.real, ph.imag = np.cos(th), np.sin(th)
        chi += ph[:, None, None, None] * blk[None]
    return Sums4(chi, int(max(tab.sh_np)) + len(np.reshape(tab.tn, (-1, 3))))


def col_err4(x, ref):
    """A.col_err per component: (4, nao)."""
    return np.stack([A.col_err(np.asarray(x)[:, c], np.asarray(ref)[:, c]) for c in range(4)])


# ---- evaluator cases ---------------------------------------------------------------------------
# tables "mixed" (l = 0..3, 1..5 primitives, two atoms; nao 17) with shuffled translations, except
# where tn says otherwise.  kmesh (2, 2, 2): the register route of the k-mesh DFT; (1, 1, 3): the
# other one; kband: "off3" / "off1" of ao_cases.  atom: point 0 is moved onto atom 1 + a lattice
# translation
Ev = namedtuple("Ev", "name tn ng kmesh kband atom")
ATOM_T = (1, -1, 0)
EV_CASES = [
    Ev("reg_222", "shuffled", 29, (2, 2, 2), None, False),
    Ev("lds_113", "shuffled", 29, (1, 1, 3), None, False),
    Ev("band_off3", "shuffled", 29, None, "off3", False),
    Ev("ng1_222", "shuffled", 1, (2, 2, 2), None, False),
    Ev("ng1_band", "shuffled", 1, None, "off1", False),
    Ev("t255_113", "shuffled", 15, (1, 1, 3), None, False),        # 15 x 17 = 256 - 1
    Ev("t272_222", "shuffled", 16, (2, 2, 2), None, False),        # 16 x 17 straddles two blocks
    Ev("t289_band", "shuffled", 17, None, "off3", False),          # one point beyond
    Ev("ng0_222", "shuffled", 0, (2, 2, 2), None, False),
    Ev("ng0_band", "shuffled", 0, None, "off3", False),
    Ev("nT0_113", "none", 29, (1, 1, 3), None, False),
    Ev("nT0_band", "none", 29, None, "off1", False),
    Ev("atom_222", "shuffled", 16, (2, 2, 2), None, True),
    Ev("atom_band", "shuffled", 16, None, "off3", True),
]
EV_BY_NAME = {c.name: c for c in EV_CASES}


def ev_id(c):
    return c.name


def ev_branches(c):
    """The branches of the evaluator a case takes: the tail, the launch shape, the edge cases."""
    out = {"band" if c.kmesh is None else ("dft_reg" if K.route(c.kmesh)[0] == K.REG else "dft_generic")}
    n = c.ng * A.nao_of(A.raw_tables("mixed", "none", A.RCUT))
    if c.ng == 0:
        out.add("ng0")
    else:
        out.add("one_block" if n <= A.BLOCK else "many_blocks")
        out.add("block_partial" if n % A.BLOCK else "block_full")
    if c.tn == "none":
        out.add("nT0")
    if c.atom:
        out.add("on_atom")
    return out


EV_BRANCHES = {"band", "dft_reg", "dft_generic", "ng0", "one_block", "many_blocks", "block_partial",
               "nT0", "on_atom"}

EvData = namedtuple("EvData", "tab coords kband ref err64 nsum")


def ev_inputs(c):
    tab = A.raw_tables("mixed", c.tn, A.RCUT)
    coords = A.raw_points(c.ng, seed=5 + c.ng)
    if c.atom:
        coords = coords.copy()
        coords[0] = np.asarray(tab.atoms)[1] + np.asarray(ATOM_T, float) @ np.asarray(tab.a)
    kband = None if c.kband is None else A.band_kpts(c.kband)
    return tab, coords, kband


@functools.lru_cache(maxsize=None)
def ev_data(name):
    c = EV_BY_NAME[name]
    tab, coords, kband = ev_inputs(c)
    if kband is None:
        wide, f64 = kmesh_sum4(tab, coords, c.kmesh, True), kmesh_sum4(tab, coords, c.kmesh, False)
    else:
        wide, f64 = band_sum4(tab, coords, kband, True), band_sum4(tab, coords, kband, False)
    return EvData(tab, coords, kband, wide.chi, col_err4(f64.chi, wide.chi), wide.nsum)


# ---- the launch rules of xc.hip, restated --------------------------------------------------------
XC_NT = 32         # D whole in LDS up to this nao, tiled XC_NT x XC_NT beyond it
XC_PT = 32         # grid points per workgroup of rho_gga_kernel


def rho_set_chunks(nao, nset, hermi):
    """Sets per launch: 4, but 2 for general D beyond XC_NT (the second D tile)."""
    ch = 2 if nao > XC_NT and not hermi else 4
    return [min(ch, nset - s) for s in range(0, nset, ch)]


def rho_branches(nao, ng, nk, nset, hermi):
    out = {"d_tiled" if nao > XC_NT else "d_untiled", "hermi" if hermi else "general"}
    if nao > XC_NT and not hermi:
        out.add("second_tile")
    out.add("one_block" if ng <= XC_PT else "many_blocks")
    out.add("point_tile_partial" if ng % XC_PT else "point_tile_full")
    if nao > XC_NT and nao % XC_NT:
        out.add("nao_tile_partial")
    ch = rho_set_chunks(nao, nset, hermi)
    out |= {"sets_%d" % c for c in ch}
    if len(ch) > 1:
        out.add("set_chunks")
    return out


RHO_BRANCHES = {"d_tiled", "d_untiled", "hermi", "general", "second_tile", "one_block", "many_blocks",
                "point_tile_partial", "point_tile_full", "nao_tile_partial", "sets_1", "sets_2",
                "sets_3", "sets_4", "set_chunks"}


def gram_ksplit(ng):
    return max(1, min(64, ng // 1024))


def gram_branches(nao, ng, nk, nset, acc):
    return {"split_k" if gram_ksplit(ng) > 1 else "one_split", "accumulate" if acc else "overwrite",
            "one_set" if nset == 1 else "many_sets", "batched" if nk > 1 else "one_k"}


GRAM_BRANCHES = {"split_k", "one_split", "accumulate", "overwrite", "one_set", "many_sets", "batched",
                 "one_k"}

RhoCase = namedtuple("RhoCase", "nao ng nk nset hermi")
RHO_CASES = [
    RhoCase(1, 1, 1, 1, 1),
    RhoCase(1, 64, 27, 5, 0),
    RhoCase(8, 65, 2, 2, 1),
    RhoCase(8, 997, 2, 3, 0),
    RhoCase(26, 64, 27, 1, 1),        # the C3 AO count
    RhoCase(26, 997, 2, 4, 0),
    RhoCase(26, 65, 1, 5, 1),
    RhoCase(33, 65, 2, 1, 1),         # D tiled, one column over the tile
    RhoCase(33, 64, 1, 3, 0),         # general D tiled: chunks 2 + 1
    RhoCase(76, 65, 1, 5, 1),         # 3 x 3 tiles, the last partial, chunks 4 + 1
    RhoCase(76, 997, 1, 2, 0),
    RhoCase(8, 1, 2, 3, 1),
]

GramCase = namedtuple("GramCase", "nao ng nk nset acc")
GRAM_CASES = [
    GramCase(1, 1, 1, 1, 0),
    GramCase(8, 64, 2, 2, 1),
    GramCase(26, 65, 27, 1, 0),
    GramCase(26, 997, 2, 4, 0),
    GramCase(33, 997, 2, 3, 1),
    GramCase(76, 997, 1, 5, 0),
    GramCase(8, 2049, 1, 1, 1),       # the GEMM splits the grid
]


def rho_id(c):
    return "nao%d-g%d-k%d-s%d-%s" % (c.nao, c.ng, c.nk, c.nset, "h" if c.hermi else "g")


def gram_id(c):
    return "nao%d-g%d-k%d-s%d-acc%d" % c


@functools.lru_cache(maxsize=None)
def rho_inputs(c):
    """f4 (nk, 4, ng, nao) and D (nset, nk, nao, nao), Hermitian for hermi = 1."""
    rng = np.random.default_rng(1000 * c.nao + c.ng + 7 * c.nk + c.nset + 31 * c.hermi)
    f4 = F.rnd(rng, c.nk, 4, c.ng, c.nao)
    D = F.rnd(rng, c.nset, c.nk, c.nao, c.nao)
    if c.hermi:
        D = D + D.conj().swapaxes(-1, -2)
    return f4, D


@functools.lru_cache(maxsize=None)
def gram_inputs(c):
    """f4, w (nset, 4, ng) real, the Hermitian matrix accumulated onto (nset, nk, nao, nao)."""
    rng = np.random.default_rng(2000 * c.nao + c.ng + 7 * c.nk + c.nset)
    f4 = F.rnd(rng, c.nk, 4, c.ng, c.nao)
    w = rng.standard_normal((c.nset, 4, c.ng))
    P = F.rnd(rng, c.nset, c.nk, c.nao, c.nao)
    return f4, w, P + P.conj().swapaxes(-1, -2)


# ---- rho, V, T from their formulas: wide=True in clongdouble, else complex128 -------------------
def rho_gga_ref(f4, D, hermi, wide=True):
    """(nset, 4, ng): hermi = 0 both terms of the gradient, hermi = 1 (2/nk) Re sum t conj d_c f."""
    dt = CLD if wide else np.complex128
    f4, D = np.asarray(f4).astype(dt), np.asarray(D).astype(dt)
    nk = f4.shape[0]
    out = np.zeros((D.shape[0], 4, f4.shape[2]), dt)
    for s in range(D.shape[0]):
        for k in range(nk):
            f = f4[k, 0]
            t = f @ D[s, k]
            out[s, 0] += (t * f.conj()).sum(axis=1)
            for c in (1, 2, 3):
                second = (t * f4[k, c].conj()).sum(axis=1)
                if hermi:
                    out[s, c] += 2 * second.real
                else:
                    out[s, c] += ((f4[k, c] @ D[s, k]) * f.conj()).sum(axis=1) + second
    return out / nk


def gga_gram_ref(f4, w, scale=1.0, wide=True):
    """V (nset, nk, nao, nao) of w (nset, 4, ng)."""
    dt, rt = (CLD, LD) if wide else (np.complex128, np.float64)
    f4, w = np.asarray(f4).astype(dt), np.asarray(w).astype(rt)
    nk, _, ng, nao = f4.shape
    out = np.zeros((w.shape[0], nk, nao, nao), dt)
    for s in range(w.shape[0]):
        for k in range(nk):
            f = f4[k, 0]
            v = (f.conj().T * w[s, 0]) @ f
            for c in (1, 2, 3):
                v = v + (f4[k, c].conj().T * w[s, c]) @ f + (f.conj().T * w[s, c]) @ f4[k, c]
            out[s, k] = v
    return out * rt(scale)


def lda_gram_ref(f4, w, scale=1.0, wide=True):
    """(nset, nk, nao, nao) of w (nset, ng): scale f^H w f."""
    dt, rt = (CLD, LD) if wide else (np.complex128, np.float64)
    f, w = np.asarray(f4).astype(dt)[:, 0], np.asarray(w).astype(rt)
    return np.stack([np.stack([(fk.conj().T * ws) @ fk for fk in f]) for ws in w]) * rt(scale)


def kin_ref(f4, scale=1.0, wide=True):
    """T (nk, nao, nao) = 1/2 scale sum_c (d_c f)^H (d_c f)."""
    dt, rt = (CLD, LD) if wide else (np.complex128, np.float64)
    f4 = np.asarray(f4).astype(dt)
    return np.stack([sum(fk[c].conj().T @ fk[c] for c in (1, 2, 3)) for fk in f4]) * (rt(scale) / 2)


# ---- end to end ----------------------------------------------------------------------------------
# (cell builder of fisdf.cell, FFT mesh, k-mesh): the toy cell on 12^3 at two k-meshes (one on each
# route of the k-mesh DFT) and the diamond cell, whose basis has a d shell
E2e = namedtuple("E2e", "name cell mesh kmesh")
E2E_CASES = [E2e("toy_222", "toy_cell", (12, 12, 12), (2, 2, 2)),
             E2e("toy_113", "toy_cell", (12, 12, 12), (1, 1, 3)),
             E2e("diamond_112", "diamond_cell", (4, 4, 4), (1, 1, 2))]
E2E_BY_NAME = {c.name: c for c in E2E_CASES}
E2E_BAND_FRAC = np.array([[0.137, -0.291, 0.413], [-0.377, 0.219, 0.081]])     # off the mesh
IDENTITY_A, IDENTITY_B = 0.37, 0.23      # e(rho, sigma) = a rho^2 + b sigma

E2eData = namedtuple("E2eData", "cell coords tab f4 f4_64 nsum kband f4b f4b_64")


@functools.lru_cache(maxsize=None)
def e2e_data(name):
    """The cell, its FFT grid, and the long-double / float64 AO blocks on it: at the k-mesh
    (nk, 4, ngrid, nao) and at the off-mesh k-points."""
    c = E2E_BY_NAME[name]
    cell = A.real_cell(c.cell, c.mesh)
    coords = cell.gen_uniform_grids(cell.mesh)
    tab = A.real_tables(cell, coords)
    wide, f64 = kmesh_sum4(tab, coords, c.kmesh, True), kmesh_sum4(tab, coords, c.kmesh, False)
    kband = E2E_BAND_FRAC @ A.reciprocal(tab.a)
    wb, b64 = band_sum4(tab, coords, kband, True), band_sum4(tab, coords, kband, False)
    return E2eData(cell, coords, tab, wide.chi, f64.chi, wide.nsum, kband, wb.chi, b64.chi)


def e2e_dms(cell, kmesh, nset, seed=3):
    """Hermitian dms (nset, nk, nao, nao), entries of order one."""
    rng = np.random.default_rng(seed)
    nk, nao = K.nk_of(kmesh), cell.nao_nr()
    D = quantize(F.rnd(rng, nset, nk, nao, nao) * 0.3)
    return D + D.conj().swapaxes(-1, -2) + np.eye(nao)


def quantize(x):
    """x rounded to multiples of 2^-20: D + delta and D - delta are then exact in float64, so
    (D + delta) - (D - delta) = 2 delta holds for the matrices the device is given."""
    x = np.asarray(x)
    return np.round(x * 2.0 ** 20) / 2.0 ** 20


def energy(rho4, vol, a=IDENTITY_A, b=IDENTITY_B):
    """E = (vol/ngrid) sum_g (a rho^2 + b |grad rho|^2) of a real rho4 (4, ngrid), in rho4's
    arithmetic."""
    rho4 = np.asarray(rho4)
    dt = rho4.dtype.type
    e = dt(a) * rho4[0] * rho4[0] + dt(b) * (rho4[1] * rho4[1] + rho4[2] * rho4[2] + rho4[3] * rho4[3])
    return e.sum() * (dt(vol) / dt(rho4.shape[1]))


def identity_wv(rho4, a=IDENTITY_A, b=IDENTITY_B):
    """wv = [de/drho, 2 de/dsigma grad rho] = [2 a rho, 2 b grad rho]."""
    rho4 = np.asarray(rho4)
    dt = rho4.dtype.type
    return np.concatenate([dt(2 * a) * rho4[:1], dt(2 * b) * rho4[1:]])
