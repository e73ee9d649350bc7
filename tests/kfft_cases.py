"""Cases, restated rules and references for the exact FFT-grid K (csrc/kfft.hip and its entries in
api.hip; ISDF.k_method = "fft"): the pair-density builder, the contraction back to nao x nao and
the whole fisdf_get_k_fft.  No tests and no GPU here: tests/test_kfft_cases.py checks this file on
the CPU, tests/test_gpu_kfft.py runs the device against it.

Three layers, as in tests/jfft_cases.py:
  * the launch rule restated (rows m per chunk from the byte budget, the grid runs, the
    instantiations by nao, the arena bytes): what fisdf_kfft_plan reports;
  * the stages in np.clongdouble on fft_cases' separable long-double DFT, the references;
  * the same sums in complex128 (numpy's fftn).  They only measure what float64 arithmetic costs
    against the long-double reference: a device result may be BOUND_FACTOR = 16 times that far
    from the reference, never less than n eps with n the length of the longest sum (nao ngrid for
    the contraction, nk nao ngrid for K, which also sums over k2), plus 2 fft_cases.TOL for the
    two transforms of K; max-norm relative to max |ref|.  The pair step is one complex product
    per element: its error is below sqrt(5) u |a b| (u = eps / 2; Brent, Percival, Zimmermann),
    so 2 eps |ref| per element is demanded.

Conventions of every GPU case: entries N(0,1) + i N(0,1); inputs are views inside NaN, the k blocks
of f f_kstride = ngrid nao + KPAD apart; outputs are views inside the sentinel 7 + 7j.
"""
import functools
from collections import namedtuple

import numpy as np

from factor_cases import BOUND_FACTOR, CLD, EPS, LD, bound  # noqa: F401
from factor_cases import relerr as rel_err  # noqa: F401
import fft_cases as F

SENTINEL = 7.0 + 7.0j
KPAD = 13          # extra elements between the k blocks of f
EDGE = 5           # NaN / sentinel elements before and after every buffer
JK_TOL = 1e-8      # the project's bar for J and K, Ha

# ---- the launch rule, restated -----------------------------------------------------------------
GT = 64                     # grid points per tile of both kernels (linalg.h kKfftGT)
EXX_MT, EXX_NT = 8, 32      # rows m per workgroup / columns per n-tile of the contraction
EXX_RUNS = 128              # grid runs the contraction aims at
SET_CHUNK = 4               # sets per pass over Z (kJfftSetChunk)
WORK_BYTES = 1 << 29        # the default budget of the transform rows (kKfftWorkBytes)
PAIR_TWS, EXX_NNS = (8, 32), (1, 2, 4)
MAX_NAO, MAX_SETS = 1 << 15, 1 << 10   # beyond them fisdf_kfft_plan is an error

Plan = namedtuple("Plan", "mc nchunk run_len nrun pair_tw exx_nn row_bytes bytes")


def _al(b):
    return -(-b // 256) * 256


def grid_split(ngrid):
    """(run_len, nrun): at most EXX_RUNS runs, each a whole number of GT-point tiles."""
    tiles = -(-ngrid // GT)
    per = -(-tiles // min(tiles, EXX_RUNS))
    return per * GT, -(-ngrid // (per * GT))


def plan(nao, ngrid, nset, work_bytes=0):
    """What fisdf_kfft_plan reports: mc = rows m per chunk = budget // (nao ngrid 16), at most
    nao; mc = nchunk = bytes = 0 when the budget is below one row m.  exx_nn: n-tiles per thread
    (beyond nao 128 the 4-tile instantiation runs once per group of 128 columns)."""
    row = 16 * nao * ngrid
    budget = work_bytes or WORK_BYTES
    run_len, nrun = grid_split(ngrid)
    tw = 8 if nao <= 8 else 32
    nt = -(-nao // EXX_NT)
    nn = 1 if nt <= 1 else 2 if nt <= 2 else 4
    mc = min(nao, budget // row)
    if mc < 1:
        return Plan(0, 0, run_len, nrun, tw, nn, row, 0)
    total = (_al(row * mc) + _al(16 * nset * nao * ngrid) + _al(8 * ngrid)
             + _al(16 * nrun * min(nset, SET_CHUNK) * mc * nao))
    return Plan(mc, -(-nao // mc), run_len, nrun, tw, nn, row, total)


def exx_instantiations(nao, nset):
    """The (sets, n-tiles) instantiations of exx_contract_kernel a call runs, and its column
    groups (more than one beyond nao 128)."""
    nn = plan(nao, 64, nset).exx_nn
    chunks = {min(SET_CHUNK, nset - s0) for s0 in range(0, nset, SET_CHUNK)}
    return {(sc, nn) for sc in chunks}, -(-nao // (nn * EXX_NT))


def budget_ladder(nao, ngrid):
    """Budgets around every edge of the rule: one byte short of a row, one row exactly, between
    rows, whole nao, beyond, and the default."""
    row = 16 * nao * ngrid
    return [row - 1, row, row + 1, 2 * row + 7, row * nao - 1, row * nao, row * nao + 1, 0]


# ---- references: wide=True in clongdouble, else complex128 ---------------------------------------
def pair_ref(f1, f2, m0, m1, wide=True):
    """P[(m - m0) nao + l][g] = conj(f1[g,m]) f2[g,l]."""
    dt = CLD if wide else np.complex128
    f1, f2 = np.asarray(f1).astype(dt), np.asarray(f2).astype(dt)
    out = f1[:, m0:m1].conj().T[:, None, :] * f2.T[None, :, :]
    return out.reshape(-1, f1.shape[0])


def conj_em(mesh, kd, wide=True):
    """conj(em)[g] = exp(+i frac(g).kd) flat on the mesh (ones for kd None)."""
    n = int(np.prod(mesh))
    if kd is None:
        return np.ones(n, CLD if wide else np.complex128)
    ph = F.phase(mesh, kd).conj().ravel()
    return ph if wide else ph.astype(np.complex128)


def contract_ref(Z, u, f1, mesh, kd, m0, m1, scale, wide=True):
    """K[s][m - m0][n] = scale sum_g t_s[m,g] f1[g,n], t_s[m,g] = conj(em[g]) sum_l
    conj(Z[(m - m0) nao + l][g]) u[s][l][g]."""
    dt = CLD if wide else np.complex128
    Z, u, f1 = (np.asarray(x).astype(dt) for x in (Z, u, f1))
    ngrid, nao = f1.shape
    Zc = Z.reshape(m1 - m0, nao, ngrid).conj()
    ce = conj_em(mesh, kd, wide)
    out = np.empty((u.shape[0], m1 - m0, nao), dt)
    for s in range(u.shape[0]):
        t = (Zc * u[s][None]).sum(axis=1) * ce
        out[s] = t @ f1
    return out * (LD(scale) if wide else scale)


def coulG(a, q, mesh, omega=0.0):
    """coulG(q, omega) of the oracle (float64: the device forms it in float64 too)."""
    from oracle.isdf_ref import get_coulG
    return get_coulG(np.asarray(a, float), np.asarray(q, float), mesh, omega=omega or None)


def mesh_kpts(a, kmesh):
    from oracle.isdf_ref import get_kpts
    return get_kpts(np.asarray(a, float), kmesh)


def exact_k_ref(f, f_band, kpts, kband, D, a, mesh, omega=0.0, wide=True):
    """K[s][k1][m,n] of the issue's four lines (PySCF fft_jk.get_k_kpts, the dm form) for the
    output points kband with AOs f_band (nb, ngrid, nao) and the k-mesh kpts with AOs f (nk, ngrid,
    nao); D (nset, nk, nao, nao) general.  wide: the transforms by fft_cases' long-double DFT (the
    phase em as the transform's kd = a q, the inverse as conj(fft(conj(x))) / N); else numpy."""
    dt = CLD if wide else np.complex128
    a = np.asarray(a, float)
    f, fb, D = (np.asarray(x).astype(dt) for x in (f, f_band, D))
    nk, ngrid, nao = f.shape
    nb = fb.shape[0]
    vol = abs(np.linalg.det(a))
    out = np.zeros((D.shape[0], nb, nao, nao), dt)
    for k2 in range(nk):
        u = D[:, k2] @ f[k2].conj().T                                   # (nset, l, g)
        for k1 in range(nb):
            q = np.asarray(kpts[k2], float) - np.asarray(kband[k1], float)
            w = coulG(a, q, mesh, omega)
            kd = a @ q
            pair = pair_ref(fb[k1], f[k2], 0, nao, wide)
            if wide:
                t = F.ref_fft3d(pair, mesh, kd=kd, weight=w) / LD(ngrid)
                v = F.ref_fft3d(t.conj(), mesh).conj()
                v = v * F.phase(mesh, kd).conj().ravel()
            else:
                em = F.phase(mesh, kd).ravel().astype(np.complex128)
                t = np.fft.fftn((pair * em).reshape(-1, *mesh), axes=(1, 2, 3)).reshape(-1, ngrid)
                v = np.fft.ifftn((t * w).reshape(-1, *mesh), axes=(1, 2, 3)).reshape(-1, ngrid)
                v = v * em.conj()
            v = v.reshape(nao, nao, ngrid)
            for s in range(D.shape[0]):
                tt = (v * u[s][None]).sum(axis=1)
                out[s, k1] += tt @ fb[k1]
    sc = vol / ngrid / nk
    return out * (LD(sc) if wide else sc)


def exact_k64(f, f_band, kpts, kband, D, a, mesh, omega=0.0):
    """The float64 restatement: what float64 arithmetic alone costs against exact_k_ref."""
    return exact_k_ref(f, f_band, kpts, kband, D, a, mesh, omega, wide=False)


def k_bound(err64, nk, nao, ngrid):
    return bound(err64, nk * nao * ngrid) + 2 * F.TOL


# ---- the pair cases --------------------------------------------------------------------------------
PAIR_NGRIDS = (1, 63, 65, 512)
PAIR_NAOS = (1, 3, 13, 33)
PairCase = namedtuple("PairCase", "ngrid nao same")
# f1 and f2 the same pointer where the sizes' sum is even, different pointers elsewhere
PAIR_CASES = [PairCase(g, n, (g + n) % 2 == 0) for g in PAIR_NGRIDS for n in PAIR_NAOS]


def row_ranges(nao):
    """(m0, m1): one row, all rows, a last partial range of a split in two-row chunks (the rows
    left over; for nao 1 the three coincide)."""
    last = (nao - 1) // 2 * 2
    return sorted({(min(1, nao - 1), min(1, nao - 1) + 1), (0, nao), (last, nao)})


def pair_id(c):
    return "g%d-nao%d-%s" % (c.ngrid, c.nao, "same" if c.same else "two")


@functools.lru_cache(maxsize=None)
def pair_inputs(c):
    rng = np.random.default_rng(100 * c.ngrid + c.nao)
    f1 = F.rnd(rng, c.ngrid, c.nao)
    return f1, (f1 if c.same else F.rnd(rng, c.ngrid, c.nao))


# ---- the contraction cases -------------------------------------------------------------------------
CONTRACT_MESHES = ((8, 8, 8), (8, 10, 12), (5, 4, 13))
CONTRACT_NAOS = (1, 3, 13, 33)
CONTRACT_NSETS = (1, 2, 3, 5)
LATTICE = np.array([[6.1, 0.2, -0.3], [0.4, 6.7, 0.1], [-0.2, 0.5, 7.3]])
KD_IRRATIONAL = (0.83, -1.91, 2.6)
KD_KINDS = ("none", "mesh", "irrational")
ContractCase = namedtuple("ContractCase", "mesh nao nset kd_kind")


WIDE_NAO = 76          # three n-tiles (the last partial: 12 columns), ten m-tiles (the last: 4)
GROUPS_NAO = 130       # beyond 128: two column groups
WIDE_MESH = (5, 4, 13)


def _contract_cases():
    """The full product mesh x nao x nset with the kinds of kd dealt round (each kind meets each
    mesh, nao and nset); nao 76 with every set count, so that every (sets, n-tiles) instantiation
    meets contract_ref; nao 130, two column groups; and one more mesh, (24, 24, 16) = 9216 points,
    whose runs hold two grid tiles each (the kernel's loop over tiles)."""
    out = []
    for i, mesh in enumerate(CONTRACT_MESHES):
        for j, nao in enumerate(CONTRACT_NAOS):
            for k, nset in enumerate(CONTRACT_NSETS):
                out.append(ContractCase(mesh, nao, nset, KD_KINDS[(i + j + k) % 3]))
    for k, nset in enumerate(CONTRACT_NSETS):
        out.append(ContractCase(WIDE_MESH, WIDE_NAO, nset, KD_KINDS[k % 3]))
    out.append(ContractCase(WIDE_MESH, GROUPS_NAO, 2, "mesh"))
    out.append(ContractCase((24, 24, 16), 3, 1, "irrational"))
    return out


CONTRACT_CASES = _contract_cases()


def contract_kd(c):
    """None, a·q for q = k2 - k1 of a (2, 3, 2) k-mesh of LATTICE, or an irrational vector."""
    if c.kd_kind == "none":
        return None
    if c.kd_kind == "irrational":
        return KD_IRRATIONAL
    kp = mesh_kpts(LATTICE, (2, 3, 2))
    return tuple(LATTICE @ (kp[7] - kp[2]))


def contract_id(c):
    return "%dx%dx%d-nao%d-s%d-%s" % (c.mesh + (c.nao, c.nset, c.kd_kind))


@functools.lru_cache(maxsize=None)
def contract_inputs(c):
    """(Z (nao nao, ngrid), u (nset, nao, ngrid), f1 (ngrid, nao), vk0 (nset, nao, nao))."""
    ngrid = int(np.prod(c.mesh))
    rng = np.random.default_rng(sum(c.mesh) + 1000 * c.nao + c.nset)
    return (F.rnd(rng, c.nao * c.nao, ngrid), F.rnd(rng, c.nset, c.nao, ngrid),
            F.rnd(rng, ngrid, c.nao), F.rnd(rng, c.nset, c.nao, c.nao))


# ---- the fisdf_get_k_fft cases ---------------------------------------------------------------------
# mc_of: the rows m per chunk the budget is made for (0: the default budget, mc = nao); band:
# None, "off" (two off-mesh points) or "on" (mesh points given as band points)
GetKCase = namedtuple("GetKCase", "kmesh mesh nao nset omega band")
GETK_CASES = [
    GetKCase((1, 1, 1), (8, 8, 8), 13, 1, 0.0, None),
    GetKCase((2, 1, 1), (8, 8, 8), 13, 2, 0.4, None),
    GetKCase((1, 2, 3), (8, 10, 12), 3, 2, -0.4, None),
    GetKCase((2, 1, 1), (8, 10, 12), 3, 1, 0.0, None),
    GetKCase((1, 2, 3), (8, 8, 8), 3, 1, 0.4, None),
    GetKCase((2, 1, 1), (8, 8, 8), 3, 2, 0.0, "off"),
    GetKCase((1, 2, 3), (8, 10, 12), 3, 1, -0.4, "off"),
    GetKCase((1, 2, 3), (8, 8, 8), 3, 2, 0.0, "on"),
]
GETK_ROUTES = {(8, 8, 8): F.REG, (8, 10, 12): F.PLANE}
REFUSED_MESH = (17, 8, 8)
ON_MESH_BAND = (4, 0, 3)        # k indices of the "on" case


def getk_budgets(c):
    """work_bytes giving mc = 1, 2 (nao 3: a partial last chunk) and nao."""
    row = 16 * c.nao * int(np.prod(c.mesh))
    return [row, 2 * row + 5, 0]


def getk_id(c):
    return "k%d%d%d-%dx%dx%d-nao%d-s%d-w%g-%s" % (c.kmesh + c.mesh + (c.nao, c.nset, c.omega,
                                                                     c.band or "mesh"))


@functools.lru_cache(maxsize=None)
def getk_inputs(c):
    """(f (nk, ngrid, nao), D (nset, nk, nao, nao) general, kpts, kband or None, f_band or None)."""
    nk, ngrid = int(np.prod(c.kmesh)), int(np.prod(c.mesh))
    rng = np.random.default_rng(sum(c.kmesh) + 10 * sum(c.mesh) + 1000 * c.nao + c.nset)
    f = F.rnd(rng, nk, ngrid, c.nao)
    D = F.rnd(rng, c.nset, nk, c.nao, c.nao)
    kpts = mesh_kpts(LATTICE, c.kmesh)
    if c.band is None:
        return f, D, kpts, None, None
    if c.band == "on":
        sel = list(ON_MESH_BAND)
        return f, D, kpts, kpts[sel].copy(), f[sel].copy()
    b = 2 * np.pi * np.linalg.inv(LATTICE).T
    kband = rng.uniform(-0.5, 0.5, (2, 3)) @ b
    return f, D, kpts, kband, F.rnd(rng, 2, ngrid, c.nao)


@functools.lru_cache(maxsize=None)
def getk_refs(c):
    """(long-double reference, float64 restatement's relative distance from it)."""
    f, D, kpts, kband, fb = getk_inputs(c)
    args = (f, f if fb is None else fb, kpts, kpts if kband is None else kband, D, LATTICE, c.mesh,
            c.omega)
    ref = exact_k_ref(*args)
    return ref, rel_err(exact_k64(*args), ref)


# ---- end to end ------------------------------------------------------------------------------------
E2E_CASES = ["toy222", "toy331_fr", "nio_small", "si_small"]
