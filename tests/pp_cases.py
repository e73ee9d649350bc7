"""Cases, restated launch rules and references for the GTH pseudopotential matrices (csrc/pp.hip and
its entries in api.hip; ISDF.get_pp / get_nuc).  No tests and no GPU here: tests/test_pp_cases.py
checks this file on the CPU, tests/test_gpu_pp.py runs the device against it.

The references follow the definitions of include/fisdf.h literally, in
np.longdouble / np.clongdouble (wide=True):
  * V_G by the sum over the atoms;
  * v(r) = (1/Omega) sum_G V_G e^{iG.r} and a~_k(G, m) = (1/N) sum_g e^{-i(k+G).r_g} f_k[g, m] by the
    separable long-double DFT of fft_cases.py;
  * c[p, m] = sum_G conj(beta_p(G; k)) a~_k(G, m) from that a~ — not through the identity
    c = sum_g t_p e^{-ik.r} f that the library uses, so the identity itself is under test;
  * Vloc = (Omega/N) f^H diag(Re v) f and Vnl = sum conj(c) h c.
wide=False restates the same sums in float64 (numpy's fftn), which only measures what float64 costs:
a device result may be factor_cases.bound(err64, n) from the reference — 16 times as far as the
float64 restatement, never less than a floor n eps — in max-norm relative to max |ref|.  Floors:
  * fisdf_vloc_g, fisdf_gth_projectors: these are no long sums, but a phase whose float64 argument
    (k+G).R_a carries a rounding of eps |(k+G).R_a| / 2 per product and sum: n = natm +
    max |(k+G).R_a| (phase_floor);
  * fisdf_pp_overlap, fisdf_get_pp: n = ngrid, the length of an element's sum.

Conventions of every GPU case: random entries N(0,1) + i N(0,1); inputs are views inside NaN (the k
blocks of f are f_kstride > ngrid nao apart); outputs are views inside the sentinel 7 + 7j.
"""
import functools
from collections import namedtuple

import numpy as np

from factor_cases import BOUND_FACTOR, CLD, EPS, LD, bound  # noqa: F401
from factor_cases import relerr as rel_err  # noqa: F401
import fft_cases as F

SENTINEL = F.SENTINEL
EDGE, KPAD = 5, 3
JK_TOL = 1e-8              # the project's bar for J / K / one-electron matrices, Ha
PI = F.PI

# ---- the cell ------------------------------------------------------------------------------------
# fcc-primitive vectors times 6.5 bohr, one of them perturbed: nothing orthogonal, nothing symmetric
LATTICE = (np.ones((3, 3)) - np.eye(3)) * 3.25
LATTICE[2] += (0.31, -0.17, 0.23)
# four atoms of three symbols at generic off-grid positions (fractional), the last outside the cell
SYMBOLS = ("Si", "Ni", "Ni", "C")
FRAC = np.array([[0.113, 0.207, 0.051], [0.519, 0.631, 0.277], [0.263, 0.871, 0.733],
                 [-0.381, 0.442, 0.619]])
ATOM_XYZ = FRAC @ LATTICE
# symbol A: rloc 0.35, two c terms, s with n = 2 (non-diagonal h), p with n = 1
# symbol B: rloc 0.25, four c terms, s n = 3, p n = 2, d n = 1, f n = 1
# the third symbol, C, has no entry: a bare nucleus (charge 6)
PSEUDO = {
    "Si": [[2, 2], 0.35, 2, [-7.13, 1.27], 2,
           [0.42, 2, [[5.91, -1.26], [-1.26, 3.25]]],
           [0.48, 1, [[2.73]]]],
    "Ni": [[4, 6, 8], 0.25, 4, [3.61, -1.13, 0.42, -0.057], 4,
           [0.26, 3, [[9.2, -2.1, 0.7], [-2.1, 6.3, -1.4], [0.7, -1.4, 3.9]]],
           [0.29, 2, [[-4.4, 1.9], [1.9, -2.6]]],
           [0.22, 1, [[-11.3]]],
           [0.31, 1, [[-2.2]]]],
}
NUC = {"Si": 14, "Ni": 28, "C": 6}
MESHES = ((12, 12, 12), (8, 9, 10))           # the register FFT route; the Stockham (plane) route
ROUTES = {(12, 12, 12): F.REG, (8, 9, 10): F.PLANE}
REFUSED_MESH = (8, 17, 8)
KFRAC = ((0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.13, -0.21, 0.37))   # Gamma, on a 2x1x1 mesh, off any
KMESH = (2, 1, 1)
NSPH = {0: 1, 1: 3, 2: 5, 3: 7}


def recip(a, wide=True):
    """b = 2 pi inv(a)^T by cofactors (rows b_i, a_i . b_j = 2 pi delta_ij)."""
    dt = LD if wide else np.float64
    a = np.asarray(a).astype(dt)
    c = np.array([np.cross(a[1], a[2]), np.cross(a[2], a[0]), np.cross(a[0], a[1])]).astype(dt)
    det = a[0] @ c[0]
    return (2 * (PI if wide else np.pi)) * c / det


def volume(a, wide=True):
    a = np.asarray(a).astype(LD if wide else np.float64)
    return abs(a[0] @ np.cross(a[1], a[2]))


def kpoint(kfrac, wide=False):
    """Cartesian k of fractional coordinates (float64: what the caller hands the library)."""
    return np.asarray(kfrac, float) @ np.asarray(recip(LATTICE, wide=False), float)


KPTS = tuple(tuple(kpoint(k)) for k in KFRAC)


def gints(mesh):
    """The fftfreq integers of every G of the mesh, (ngrid, 3), C order."""
    ax = [np.where(np.arange(n) < (n + 1) // 2, np.arange(n), np.arange(n) - n) for n in mesh]
    g = np.meshgrid(*ax, indexing="ij")
    return np.stack([x.ravel() for x in g], axis=1)


def gvecs(mesh, wide=True):
    return gints(mesh).astype(LD if wide else np.float64) @ recip(LATTICE, wide)


def _expi(theta, wide):
    out = np.empty(np.shape(theta), dtype=CLD if wide else np.complex128)
    out.real, out.imag = np.cos(theta), np.sin(theta)
    return out


# ---- the table -----------------------------------------------------------------------------------
Atom = namedtuple("Atom", "xyz z rloc cs projs bare")     # projs: [(r_l, n_l, h_l)]


def atoms_of(pseudo=None, xyz=None, nuc=False):
    """The atoms as the definitions read them: Z = sum(nelec) with an entry, the nuclear charge of
    a bare atom; nuc: every atom bare with its atom_charges() (Z_ion where it has an entry)."""
    pseudo = PSEUDO if pseudo is None else pseudo
    xyz = ATOM_XYZ if xyz is None else xyz
    out = []
    for sym, r in zip(SYMBOLS, xyz):
        if sym in pseudo:
            e = pseudo[sym]
            z = float(sum(e[0]))
            if nuc:
                out.append(Atom(np.asarray(r, float), z, 0.0, (), (), True))
            else:
                projs = [(float(rl), int(n), np.asarray(h, float).reshape(int(n), int(n)))
                         for rl, n, h in e[5:]]
                out.append(Atom(np.asarray(r, float), z, float(e[1]), tuple(e[3]), projs, False))
        else:
            out.append(Atom(np.asarray(r, float), float(NUC[sym]), 0.0, (), (), True))
    return out


def atom_rows(atoms):
    """Projector rows of every atom."""
    return [sum(n * NSPH[l] for l, (_, n, _) in enumerate(a.projs)) for a in atoms]


def row_labels(atoms):
    """(atom, l, i, mm) of every projector row, table order: i slower than mm."""
    return [(ia, l, i, mm) for ia, a in enumerate(atoms) for l, (_, n, _) in enumerate(a.projs)
            for i in range(n) for mm in range(NSPH[l])]


def pack(atoms, lib):
    """ctypes array of lib.PPAtom from the Atom tuples (the test's own packing)."""
    tab = (lib.PPAtom * len(atoms))()
    for A, a in zip(tab, atoms):
        A.r[:] = a.xyz
        A.z, A.bare = a.z, int(a.bare)
        if a.bare:
            continue
        A.rloc, A.nexp, A.nl = a.rloc, len(a.cs), len(a.projs)
        A.c[:len(a.cs)] = a.cs
        for l, (rl, n, h) in enumerate(a.projs):
            A.rl[l], A.n[l] = rl, n
            for i in range(n):
                for j in range(n):
                    A.h[l][3 * i + j] = h[i, j]
    return tab


# ---- the definitions -------------------------------------------------------------------------------
def vloc_radial(G2, a, wide=True, drop_g0=False):
    """v_a(|G|) for every G^2 (the G = 0 branch where G2 == 0)."""
    dt = LD if wide else np.float64
    pi = PI if wide else np.pi
    z, rloc = dt(a.z), dt(a.rloc)
    cs = [dt(c) for c in a.cs] + [dt(0)] * (4 - len(a.cs))
    x2 = G2 * rloc * rloc
    x4 = x2 * x2
    poly = (cs[0] + cs[1] * (3 - x2) + cs[2] * (15 - 10 * x2 + x4)
            + cs[3] * (105 - 105 * x2 + 21 * x4 - x4 * x2))
    gauss = (2 * pi) ** dt(1.5) * rloc ** 3
    safe = np.where(G2 == 0, dt(1), G2)
    v = np.exp(-x2 / 2) * (-z * 4 * pi / safe + gauss * poly)
    v0 = 2 * pi * z * rloc * rloc + gauss * (cs[0] + 3 * cs[1] + 15 * cs[2] + 105 * cs[3])
    return np.where(G2 == 0, dt(0) if drop_g0 else v0, v)


def vloc_g_ref(mesh, atoms, wide=True, si_sign=-1, drop_g0=False):
    """V_G = sum_a SI_a(G) v_a(|G|), SI_a = exp(si_sign i G.R_a) (the definition: -1)."""
    dt = LD if wide else np.float64
    Gv = gvecs(mesh, wide)
    G2 = (Gv * Gv).sum(axis=1)
    out = np.zeros(len(Gv), dtype=CLD if wide else np.complex128)
    for a in atoms:
        out = out + _expi(si_sign * (Gv @ a.xyz.astype(dt)), wide) * vloc_radial(G2, a, wide, drop_g0)
    return out


def v_real_space(VG, mesh, wide=True):
    """v(r_g) = (1/Omega) sum_G V_G e^{iG.r_g}: the forward DFT between two conjugations."""
    if wide:
        return F.ref_fft3d(VG.conj()[None], mesh)[0].conj() / volume(LATTICE)
    return np.fft.ifftn(VG.reshape(mesh)).ravel() * (np.prod(mesh) / volume(LATTICE, False))


def vloc_ref(f, mesh, atoms, wide=True, **kw):
    """Vloc[m, n] = (Omega/N) sum_g conj(f[g, m]) Re v(r_g) f[g, n]; f (ngrid, nao)."""
    dt = CLD if wide else np.complex128
    v = v_real_space(vloc_g_ref(mesh, atoms, wide, **kw), mesh, wide).real
    f = np.asarray(f).astype(dt)
    sc = volume(LATTICE, wide) / (LD if wide else np.float64)(len(f))
    return (f.conj().T @ (v[:, None] * f)) * sc


def q_li(l, i, x2, dt):
    """q_{l,i}(x), i = 1, 2, 3: the table of the issue, restated."""
    s = lambda v: np.sqrt(dt(v))       # noqa: E731
    x4 = x2 * x2
    one = x2 * 0 + 1
    t = {(0, 1): 4 * s(2) * one,
         (0, 2): 8 * s(dt(2) / 15) * (3 - x2),
         (0, 3): dt(16) / 3 * s(dt(2) / 105) * (15 - 10 * x2 + x4),
         (1, 1): 8 / s(3) * one,
         (1, 2): 16 / s(105) * (5 - x2),
         (1, 3): dt(32) / 3 / s(1155) * (35 - 14 * x2 + x4),
         (2, 1): 8 * s(dt(2) / 15) * one,
         (2, 2): dt(16) / 3 * s(dt(2) / 105) * (7 - x2),
         (2, 3): dt(32) / 3 * s(dt(2) / 15015) * (63 - 18 * x2 + x4),
         (3, 1): 16 / s(105) * one,
         (3, 2): dt(32) / 3 / s(1155) * (9 - x2),
         (3, 3): dt(64) / 45 / s(1001) * (99 - 22 * x2 + x4)}
    return t[(l, i)]


def solid_harmonics(l, K):
    """S_lm(K) = |K|^l Y_lm, the normalisation and order of fisdf.cell._real_sph (the constants are
    the device's float64 ones; the polynomials are evaluated in K's precision)."""
    from fisdf.cell import _real_sph
    return _real_sph(l, K[:, 0], K[:, 1], K[:, 2])


def beta_ref(mesh, k, atoms, wide=True, m_perm=None):
    """beta_p(G; k) = e^{-iK.R_a} P_i^l(|K|) S_lm(K), K = k + G: (nproj, ngrid), rows in table
    order.  m_perm: a function l -> permutation of the 2 l + 1 mm (the order must not matter)."""
    dt = LD if wide else np.float64
    pi = PI if wide else np.pi
    K = gvecs(mesh, wide) + np.asarray(k).astype(dt)[None, :]
    K2 = (K * K).sum(axis=1)
    rows = []
    for a in atoms:
        si = _expi(-(K @ a.xyz.astype(dt)), wide)
        for l, (rl, n, _) in enumerate(a.projs):
            if n == 0:
                continue
            rl = dt(rl)
            x2 = K2 * rl * rl
            base = pi ** dt(1.25) * rl ** (dt(l) + dt(1.5)) * np.exp(-x2 / 2)
            S = solid_harmonics(l, K)
            order = list(range(NSPH[l])) if m_perm is None else list(m_perm(l))
            for i in range(1, n + 1):
                P = q_li(l, i, x2, dt) * base
                for mm in order:
                    rows.append(si * (P * S[mm]))
    if not rows:
        return np.zeros((0, len(K)), dtype=CLD if wide else np.complex128)
    return np.asarray(rows)


def atilde_ref(f, mesh, k, wide=True):
    """a~_k(G, m) = (1/N) sum_g e^{-i(k+G).r_g} f[g, m], as (nao, ngrid): the phase e^{-ik.r_g} =
    exp(-i frac(g).kd), kd = a k, then the forward DFT."""
    kd = LATTICE @ np.asarray(k, float)
    n = len(f)
    if wide:
        return F.ref_fft3d(np.asarray(f).T, mesh, kd=kd) / LD(n)
    ph = F.phase(mesh, kd).ravel().astype(np.complex128)
    x = (np.asarray(f).T * ph[None, :]).reshape(-1, *mesh)
    return np.fft.fftn(x, axes=(1, 2, 3)).reshape(-1, n) / n


def vnl_from_c(c, atoms, h_offdiag=True):
    """sum over (a, l, mm) and i, j of conj(c[(a,l,i,mm), m]) h_l[i, j] c[(a,l,j,mm), n]."""
    nao = c.shape[1]
    out = np.zeros((nao, nao), dtype=c.dtype)
    real = LD if c.dtype == CLD else np.float64
    row = 0
    for a in atoms:
        for l, (_, n, h) in enumerate(a.projs):
            nm = NSPH[l]
            blk = c[row:row + n * nm].reshape(n, nm, nao)
            hh = np.asarray(h).astype(real)
            if not h_offdiag:
                hh = np.diag(np.diag(hh))
            for mm in range(nm):
                out = out + blk[:, mm].conj().T @ (hh @ blk[:, mm])
            row += n * nm
    return out


def vnl_ref(f, mesh, k, atoms, wide=True, m_perm=None, h_offdiag=True):
    beta = beta_ref(mesh, k, atoms, wide, m_perm)
    c = beta.conj() @ atilde_ref(f, mesh, k, wide).T
    return vnl_from_c(c, atoms, h_offdiag)


def pp_ref(f, mesh, k, atoms, wide=True, with_nonlocal=True):
    """get_pp at one k-point: Vloc + Vnl; the imaginary part dropped at k = 0."""
    out = vloc_ref(f, mesh, atoms, wide)
    if with_nonlocal and sum(atom_rows(atoms)):
        out = out + vnl_ref(f, mesh, k, atoms, wide)
    if abs(np.asarray(k, float)).sum() < 1e-9:
        out = out.real.astype(out.dtype)
    return out


def overlap_ref(t, f, mesh, kd, scale, wide=True):
    """c[p, m] = scale sum_g t[p, g] exp(-i frac(g).kd) f[g, m]."""
    dt = CLD if wide else np.complex128
    t, f = np.asarray(t).astype(dt), np.asarray(f).astype(dt)
    if kd is not None:
        t = t * F.phase(mesh, kd).ravel().astype(dt)[None, :]
    return (t @ f) * (LD(scale) if wide else scale)


def phase_floor(mesh, k, atoms):
    """natm + max |(k + G).R_a|: the floor of the phase-bound stage entries, in eps."""
    K = gvecs(mesh, wide=False) + np.asarray(k, float)[None, :]
    return len(atoms) + max(float(abs(K @ a.xyz).max()) for a in atoms)


# ---- the launch rules, restated --------------------------------------------------------------------
GT, MT, PT, RUNS = 64, 32, 16, 256         # kPpGT, kPpMT, kPpPT, kPpRuns
WORK_BYTES = 1 << 29                       # the default budget of one k-point's projector rows


def overlap_split(ngrid):
    """(points per run, runs): whole steps of 64 points, at most 256 runs; from ngrid alone."""
    steps = -(-ngrid // GT)
    per = max(1, -(-steps // RUNS))
    return per * GT, max(1, -(-ngrid // (per * GT)))


def overlap_branches(np_, nao, ngrid):
    """The branches of pp_overlap_kernel and its launch that a case reaches."""
    run_len, nrun = overlap_split(ngrid)
    out = {"one-step-runs" if run_len == GT else "multi-step-runs"}
    out.add("partial-step" if ngrid % GT else "full-last-step")
    if ngrid % run_len and run_len > GT:
        out.add("short-last-run")
    out.add("one-run" if nrun == 1 else "many-runs")
    out.add("ao-tail" if nao % MT else "ao-full")
    if nao > MT:
        out.add("ao-tiles")
    last = np_ - (np_ - 1) // PT * PT          # rows of the last projector tile
    out.add("p-first-half-only" if last <= 8 else ("p-tail" if last < PT else "p-full"))
    if np_ > PT:
        out.add("p-tiles")
    return out


OVERLAP_BRANCHES = {"one-step-runs", "multi-step-runs", "partial-step", "full-last-step",
                    "short-last-run", "many-runs", "ao-tail", "ao-full", "ao-tiles",
                    "p-first-half-only", "p-tail", "p-full", "p-tiles"}


def chunks(rows, ngrid, work_bytes=0):
    """Atom chunks [a0, a1) of fisdf_get_pp under a byte budget for one k-point's projector rows:
    whole atoms while their rows fit; None when an atom's own rows do not (the call is refused)."""
    W = work_bytes or WORK_BYTES
    if sum(rows) == 0:
        return []
    cuts, cur = [0], 0
    for a, r in enumerate(rows):
        if r * 16 * ngrid > W:
            return None
        if cur > 0 and (cur + r) * 16 * ngrid > W:
            cuts.append(a)
            cur = 0
        cur += r
    cuts.append(len(rows))
    return list(zip(cuts[:-1], cuts[1:]))


# ---- the case tables -------------------------------------------------------------------------------
def ngrid_of(mesh):
    return int(np.prod(mesh))


# the overlap stage: (mesh, np, nao, kd kind).  The third mesh is beyond 256 steps of 64 points, so
# that runs of several steps, and a short last run, are reached (no transform runs in this stage)
BIG_MESH = (33, 30, 18)
OverlapCase = namedtuple("OverlapCase", "mesh np nao kd")
KD_OFF = tuple(LATTICE @ np.asarray(KPTS[2]))
KD_HALF = tuple(LATTICE @ np.asarray(KPTS[1]))
OVERLAP_CASES = [
    OverlapCase((12, 12, 12), 1, 1, None),
    OverlapCase((12, 12, 12), 5, 5, KD_OFF),
    OverlapCase((12, 12, 12), 47, 33, KD_HALF),
    OverlapCase((12, 12, 12), 16, 32, KD_OFF),
    OverlapCase((8, 9, 10), 1, 33, KD_OFF),
    OverlapCase((8, 9, 10), 26, 5, None),
    OverlapCase((8, 9, 10), 47, 1, KD_HALF),
    OverlapCase((8, 9, 10), 17, 33, KD_OFF),
    OverlapCase(BIG_MESH, 3, 5, KD_OFF),
]

# the whole entry on random f: (mesh, nao); every case runs the three k-points in one call
PpCase = namedtuple("PpCase", "mesh nao")
PP_CASES = [PpCase(m, n) for m in MESHES for n in (1, 5, 33)]


def case_id(c):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) and len(v) == 3
                    and all(isinstance(x, int) for x in v) else
                    ("kd" if isinstance(v, tuple) else str(v)) for v in c)


@functools.lru_cache(maxsize=None)
def overlap_inputs(c):
    ng = ngrid_of(c.mesh)
    rng = np.random.default_rng(7 + sum(c.mesh) + 10 * c.np + 1000 * c.nao)
    return F.rnd(rng, c.np, ng), F.rnd(rng, ng, c.nao)


@functools.lru_cache(maxsize=None)
def overlap_refs(c):
    t, f = overlap_inputs(c)
    sc = 1.0 / ngrid_of(c.mesh)
    ref = overlap_ref(t, f, c.mesh, c.kd, sc)
    return ref, rel_err(overlap_ref(t, f, c.mesh, c.kd, sc, wide=False), ref)


@functools.lru_cache(maxsize=None)
def pp_inputs(c):
    """f (3, ngrid, nao): random AOs at the three k-points."""
    rng = np.random.default_rng(11 + sum(c.mesh) + 100 * c.nao)
    return F.rnd(rng, len(KPTS), ngrid_of(c.mesh), c.nao)


@functools.lru_cache(maxsize=None)
def pp_refs(c, with_nonlocal=True, nuc=False):
    """(reference (3, nao, nao), the float64 restatement's relative distance)."""
    f = pp_inputs(c)
    atoms = atoms_of(nuc=nuc)
    ref = np.asarray([pp_ref(f[i], c.mesh, KPTS[i], atoms, True, with_nonlocal) for i in range(3)])
    r64 = np.asarray([pp_ref(f[i], c.mesh, KPTS[i], atoms, False, with_nonlocal) for i in range(3)])
    return ref, rel_err(r64, ref)


@functools.lru_cache(maxsize=None)
def vloc_g_refs(mesh, nuc=False):
    atoms = atoms_of(nuc=nuc)
    ref = vloc_g_ref(mesh, atoms)
    return ref, rel_err(vloc_g_ref(mesh, atoms, wide=False), ref)


@functools.lru_cache(maxsize=None)
def beta_refs(mesh, ik):
    atoms = atoms_of()
    ref = beta_ref(mesh, KPTS[ik], atoms).conj()
    return ref, rel_err(beta_ref(mesh, KPTS[ik], atoms, wide=False).conj(), ref)


# ---- end to end: the toy basis on the cell ---------------------------------------------------------
def toy_cell(mesh, pseudo=None):
    from fisdf import cell as C
    return C.Cell(a=LATTICE.copy(), atoms=[(s, r.copy()) for s, r in zip(SYMBOLS, ATOM_XYZ)],
                  basis="toy", mesh=mesh, pseudo=PSEUDO if pseudo is None else pseudo)


@functools.lru_cache(maxsize=None)
def toy_aos(mesh):
    """The toy basis' Bloch AOs at the three k-points on the FFT grid, host (3, ngrid, nao)."""
    from fisdf import cell as C
    cell = toy_cell(mesh)
    return C.eval_ao_band(cell, cell.gen_uniform_grids(mesh), np.asarray(KPTS))


@functools.lru_cache(maxsize=None)
def toy_refs(mesh, nuc=False):
    """get_pp (or get_nuc) of the toy cell at the three k-points, long double, (3, nao, nao)."""
    f = toy_aos(mesh)
    atoms = atoms_of(nuc=nuc)
    return np.asarray([pp_ref(f[i], mesh, KPTS[i], atoms, True, not nuc) for i in range(3)])
