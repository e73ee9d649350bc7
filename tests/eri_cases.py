"""Cases, the restated plan rule and references for the exact FFT-grid four-index integrals
(csrc/erifft.hip and its entries in api.hip; ISDF.eri_method = "fft"): the B builder fisdf_pair34 and
the whole fisdf_get_eri_fft.  No tests and no GPU here: tests/test_eri_cases.py checks this file on
the CPU, tests/test_gpu_eri_fft.py runs the device against it.

Three layers, as in tests/kfft_cases.py:
  * the plan rule restated (rows i per chunk and rows (p, k) per B chunk from the byte budget,
    whether B is built once, the builder's tile width, the split-K, the arena bytes): what
    fisdf_eri_fft_plan reports;
  * the composition in np.clongdouble — kfft_cases.pair_ref, fft_cases.ref_fft3d, the phase and
    the weight as kfft_cases.exact_k_ref forms them — the reference;
  * the same composition in complex128 (numpy's fftn), which only measures what float64 costs
    against the reference: a device result may be factor_cases.bound(err64, n) from the reference,
    16 times that far and never less than n eps, plus 2 fft_cases.TOL for the two transforms of
    the whole entry; max-norm relative to max |ref|.  n = ngrid for the whole entry (the length of
    an element's sum).  For the builder n = PAIR34_ROUNDINGS = 12, the roundings of its chain
    counted in eps: theta = sum_d frac_d kd_d has a division, a product and two sums, each below
    eps / 2 of sum_d |frac_d kd_d| <= (|kd_0| + |kd_1| + |kd_2|) / 2 <= 4.19 for the kd of these
    tables (the mesh-q one, 2 pi (1/2, -1/3, 1/2)), so |d theta| <= 8.4 eps; sincos adds 1 eps; the
    two complex products sqrt(5) eps / 2 each (Brent, Percival, Zimmermann); 11.7 eps in all.

Conventions of every GPU case are kfft_cases': entries N(0,1) + i N(0,1); inputs are views inside
NaN; outputs are views inside the sentinel 7 + 7j.
"""
import functools
from collections import namedtuple

import numpy as np

from factor_cases import BOUND_FACTOR, CLD, EPS, LD, bound  # noqa: F401
from factor_cases import relerr as rel_err  # noqa: F401
import fft_cases as F
import kfft_cases as K

SENTINEL = K.SENTINEL
LATTICE = K.LATTICE
ERI_TOL = 1e-10            # the project's bar for ERI equalities, times max(1, max |ref|)
PAIR34_ROUNDINGS = 12

# ---- the plan rule, restated -------------------------------------------------------------------
WORK_BYTES = 1 << 29       # the default budget (kKfftWorkBytes), for the transform rows and B each
PAIR34_CAP = 8             # pairs per launch of the builder (kPair34Cap)
TWS = (8, 32)              # the builder's tile widths, by n4
MAX_N, MAX_PAIRS = 1 << 15, 65535

Plan = namedtuple("Plan", "mc nrow_chunks bc nb_chunks b_once tw ksplit bytes")


def _al(b):
    return -(-b // 256) * 256


def ksplit(n12, n34, ngrid):
    """The selection Gram's rule on the tiles of the whole n1 n2 x n3 n4 product: doubled while
    tiles ks < 512 and every part keeps 256 grid points.  Neither the budget nor npair enters."""
    tiles = -(-n12 // 64) * -(-n34 // 64)
    ks = 1
    while tiles * ks < 512 and ngrid // (2 * ks) >= 256:
        ks *= 2
    return ks


def plan(n1, n2, n3, n4, npair, ngrid, work_bytes=0):
    """What fisdf_eri_fft_plan reports: mc = min(n1, W // (16 n2 ngrid)) rows i per chunk,
    bc = min(npair n3, W // (16 n4 ngrid)) rows (p, k) per B chunk; either below 1: all zero but
    tw and ksplit.  b_once: one B chunk."""
    W = work_bytes or WORK_BYTES
    row12, row34 = 16 * n2 * ngrid, 16 * n4 * ngrid
    tw = 8 if n4 <= 8 else 32
    ks = ksplit(n1 * n2, n3 * n4, ngrid)
    mc, bc = min(n1, W // row12), min(npair * n3, W // row34)
    if mc < 1 or bc < 1:
        return Plan(0, 0, 0, 0, 0, tw, ks, 0)
    nb = -(-npair * n3 // bc)
    work = ks * mc * n2 * min(bc, n3) * n4 if ks > 1 else 0
    total = _al(row12 * mc) + _al(row34 * bc) + _al(8 * ngrid) + _al(16 * work)
    return Plan(mc, -(-n1 // mc), bc, nb, int(nb == 1), tw, ks, total)


def budget_ladder(n1, n2, n3, n4, npair, ngrid):
    """Budgets around every edge of the rule: one byte short of a row of either kind, the rows
    exactly, between rows, everything, beyond, and the default."""
    out = {0}
    for row, n in ((16 * n2 * ngrid, n1), (16 * n4 * ngrid, npair * n3)):
        out |= {row - 1, row, row + 1, 2 * row + 7, row * n - 1, row * n, row * n + 1}
    return sorted(out)


# ---- references: wide=True in clongdouble, else complex128 ---------------------------------------
def pair34_ref(a3s, a4s, mesh, kd, r0, r1, wide=True):
    """B[(p n3 + k - r0) n4 + l][g] = conj(em[g]) conj(a3_p[g,k]) a4_p[g,l], rows (p, k) in
    [r0, r1)."""
    dt = CLD if wide else np.complex128
    n3 = np.shape(a3s[0])[1]
    ce = K.conj_em(mesh, kd, wide)
    rows = []
    for r in range(r0, r1):
        p, k = divmod(r, n3)
        a3, a4 = np.asarray(a3s[p]).astype(dt), np.asarray(a4s[p]).astype(dt)
        rows.append((ce * a3[:, k].conj())[None, :] * a4.T)
    return np.concatenate(rows, axis=0)


def eri_ref(a1, a2, a3s, a4s, a, mesh, q, omega=0.0, wide=True):
    """eri[p][i n2 + j][k n4 + l] of the issue's three lines (PySCF FFTDF.get_eri / ao2mo): the
    pair densities of (a1, a2), the transform pair as kfft_cases.exact_k_ref forms it (wide: the
    long-double DFT with the phase as the transform's kd = a q and the inverse as
    conj(fft(conj(x))) / N; else numpy), then the sum over the grid against every pair's
    conj(a3) a4."""
    dt = CLD if wide else np.complex128
    a = np.asarray(a, float)
    q = np.asarray(q, float)
    a1, a2 = np.asarray(a1).astype(dt), np.asarray(a2).astype(dt)
    ngrid, n1 = a1.shape
    n2 = a2.shape[1]
    vol = abs(np.linalg.det(a))
    w = K.coulG(a, q, mesh, omega)
    kd = a @ q
    pair = K.pair_ref(a1, a2, 0, n1, wide)                      # (n1 n2, ngrid)
    if wide:
        t = F.ref_fft3d(pair, mesh, kd=kd, weight=w) / LD(ngrid)
        v = F.ref_fft3d(t.conj(), mesh).conj()
        v = v * F.phase(mesh, kd).conj().ravel()
    else:
        em = F.phase(mesh, kd).ravel().astype(np.complex128)
        t = np.fft.fftn((pair * em).reshape(-1, *mesh), axes=(1, 2, 3)).reshape(-1, ngrid)
        v = np.fft.ifftn((t * w).reshape(-1, *mesh), axes=(1, 2, 3)).reshape(-1, ngrid)
        v = v * em.conj()
    sc = LD(vol) / LD(ngrid) if wide else vol / ngrid
    out = []
    for a3, a4 in zip(a3s, a4s):
        a3, a4 = np.asarray(a3).astype(dt), np.asarray(a4).astype(dt)
        p34 = (a3.conj().T[:, None, :] * a4.T[None, :, :]).reshape(-1, ngrid)
        out.append(v @ p34.T * sc)
    return np.asarray(out)


def eri64(a1, a2, a3s, a4s, a, mesh, q, omega=0.0):
    """The float64 restatement: what float64 arithmetic alone costs against eri_ref."""
    return eri_ref(a1, a2, a3s, a4s, a, mesh, q, omega, wide=False)


def eri_bound(err64, ngrid):
    return bound(err64, ngrid) + 2 * F.TOL


def pair34_bound(err64):
    return bound(err64, PAIR34_ROUNDINGS)


# ---- the case tables -----------------------------------------------------------------------------
MESHES = ((8, 8, 8), (8, 10, 12), (5, 4, 13))     # the register, plane and generic FFT routes
ROUTES = {(8, 8, 8): F.REG, (8, 10, 12): F.PLANE, (5, 4, 13): F.PLANE | F.BIG}
MIXED = (3, 4, 2, 5)
KD_KINDS = K.KD_KINDS                              # none, mesh-q, irrational
REFUSED_MESH = K.REFUSED_MESH

# sizes (n1, n2, n3, n4); q_kind as kfft_cases' kd kinds
EriCase = namedtuple("EriCase", "mesh sizes npair q_kind omega")
CASES = [
    EriCase((8, 8, 8), (1, 1, 1, 1), 1, "none", 0.0),
    EriCase((8, 8, 8), (3, 3, 3, 3), 3, "mesh", 0.4),
    EriCase((8, 8, 8), (13, 13, 13, 13), 1, "irrational", 0.0),
    EriCase((8, 8, 8), MIXED, 3, "mesh", 0.0),
    EriCase((8, 8, 8), (3, 3, 33, 33), 1, "irrational", 0.4),
    EriCase((8, 10, 12), (1, 1, 1, 1), 3, "irrational", 0.4),
    EriCase((8, 10, 12), (3, 3, 3, 3), 1, "none", 0.0),
    EriCase((8, 10, 12), (13, 13, 13, 13), 3, "mesh", 0.0),
    EriCase((8, 10, 12), (33, 33, 2, 5), 1, "irrational", 0.4),   # the largest: 33^2 rows of 960
    EriCase((5, 4, 13), (1, 1, 1, 1), 1, "mesh", 0.4),
    EriCase((5, 4, 13), (3, 3, 3, 3), 3, "irrational", 0.0),
    EriCase((5, 4, 13), (13, 13, 13, 13), 1, "none", 0.4),
    EriCase((5, 4, 13), (33, 33, 33, 33), 1, "mesh", 0.0),
    EriCase((5, 4, 13), MIXED, 3, "irrational", 0.4),
]


def case_id(c):
    return "%dx%dx%d-n%d.%d.%d.%d-p%d-%s-w%g" % (c.mesh + c.sizes + (c.npair, c.q_kind, c.omega))


def ngrid_of(c):
    return int(np.prod(c.mesh))


def case_q(c):
    """q = k2 - k1, Cartesian: zero, a difference of two points of a (2, 3, 2) k-mesh of LATTICE
    (kfft_cases.contract_kd's), or the q whose kd = a q is kfft_cases' irrational vector."""
    if c.q_kind == "none":
        return np.zeros(3)
    if c.q_kind == "irrational":
        return np.linalg.solve(LATTICE, np.asarray(K.KD_IRRATIONAL))
    kp = K.mesh_kpts(LATTICE, (2, 3, 2))
    return kp[7] - kp[2]


def case_kd(c):
    """What the builder is given: None at q = 0, else a q."""
    return None if c.q_kind == "none" else tuple(LATTICE @ case_q(c))


def budgets(c):
    """work_bytes of the case: the smallest the entry takes (one row of the wider kind: mc = 1 or
    bc = 1), two and five of them and a little (partial last chunks of both kinds, B rebuilt), and
    the default."""
    n1, n2, n3, n4 = c.sizes
    lo = 16 * max(n2, n4) * ngrid_of(c)
    return [lo, 2 * lo + 5, 5 * lo + 1, 0]


@functools.lru_cache(maxsize=None)
def inputs(c):
    """(a1 (ngrid, n1), a2 (ngrid, n2), a3s, a4s: npair arrays (ngrid, n3) / (ngrid, n4))."""
    n1, n2, n3, n4 = c.sizes
    ng = ngrid_of(c)
    rng = np.random.default_rng(sum(c.mesh) + 100 * sum(c.sizes) + c.npair)
    return (F.rnd(rng, ng, n1), F.rnd(rng, ng, n2),
            tuple(F.rnd(rng, ng, n3) for _ in range(c.npair)),
            tuple(F.rnd(rng, ng, n4) for _ in range(c.npair)))


@functools.lru_cache(maxsize=None)
def refs(c):
    """(long-double reference (npair, n1 n2, n3 n4), float64 restatement's relative distance)."""
    args = inputs(c) + (LATTICE, c.mesh, case_q(c), c.omega)
    ref = eri_ref(*args)
    return ref, rel_err(eri64(*args), ref)


def row_ranges(npair, n3):
    """(r0, r1) of the npair n3 rows (p, k): all, one row, the rows left over by a split in
    five-row chunks (crossing pairs where n3 is no multiple of five)."""
    n = npair * n3
    last = (n - 1) // 5 * 5
    return sorted({(0, n), (min(1, n - 1), min(1, n - 1) + 1), (last, n)})


# the builder's cases: (case of CASES whose a3 / a4 it takes, ld padding)
PAIR34_CASES = [c for c in CASES if c.sizes != (33, 33, 33, 33)] + [
    EriCase((5, 4, 13), (1, 1, 13, 3), 11, "mesh", 0.0),         # 11 pairs: two launches
]
LD_PAD = 3                  # ld3 = n3 + LD_PAD, ld4 = n4 + LD_PAD in the builder's cases

# ---- end to end ------------------------------------------------------------------------------------
E2E_CASES = ["toy222", "toy331_fr", "si_small"]


def check_triples(nk):
    """The seven triples of test_coul.py::test_get_coul_lstsq_and_eri_harness."""
    rng = np.random.default_rng(0)
    return [tuple(int(t) for t in rng.integers(0, nk, 3)) for _ in range(6)] + [(0, 0, 0)]
