"""Cases, restated rules and references for the exact FFT-grid K in the occupied-orbital (low-rank)
form (csrc/kfft.hip and its entries in api.hip; ISDF.k_form = "lowrank"): the pair builder
against the orbitals on the grid, the segmented contraction and the whole fisdf_get_k_fft_lr.  No
tests and no GPU here: tests/test_kfft_lr_cases.py checks this file on the CPU,
tests/test_gpu_kfft_lr.py runs the device against it.  Everything shared with the dm form — the
conventions of the buffers, the bound, the meshes, the lattice — is kfft_cases' (K).

D[s][k2] = A[:, :r] B[:, :r]^H with r = ranks[s][k2]; the transform rows of one k2 are the orbitals
of all sets stacked, I = sum_s r, set s owning the segment [seg[s], seg[s + 1]).

  * the launch rule restated: what fisdf_kfft_lr_plan reports;
  * the references: for the stages their long-double restatements, for the whole K kfft_cases'
    exact_k_ref (long double) on D formed in long double;
  * err64: the float64 NumPy restatement of the three low-rank lines against that reference.  A
    device result may be K.bound(err64, n) away, n the length of the longest sum: the longest
    segment x ngrid for the contraction, K.k_bound(err64, nk, imax, ngrid) for the whole call; the
    pair builder is one complex product per element, 2 eps |ref|.
"""
import functools
from collections import namedtuple

import numpy as np

import fft_cases as F
import kfft_cases as K
from kfft_cases import CLD, LD

# ---- the launch rule, restated -----------------------------------------------------------------
LR_ROWS = 32                 # rows (set, m) per workgroup of the contraction (linalg.h kLrRows)
LR_SET_CHUNK = 2             # sets per launch (kLrSetChunk)
PAIR_TWS, EXX_SCS = (8, 32), (1, 2)

LrPlan = namedtuple("LrPlan", "mc nchunk run_len nrun pair_tw exx_sc exx_nn row_bytes bytes")


def plan(nao, ngrid, nset, imax, work_bytes=0):
    """What fisdf_kfft_lr_plan reports: mc = rows m per chunk = budget // (imax ngrid 16), at most
    nao; mc = nchunk = bytes = 0 when the budget is below one row m.  The arena: the mc imax
    transform rows, psi and u (imax rows each), the Coulomb weight and the contraction's partial
    blocks (runs x sets per launch x mc x nao)."""
    row = 16 * imax * ngrid
    budget = work_bytes or K.WORK_BYTES
    run_len, nrun = K.grid_split(ngrid)
    tw = 8 if imax <= 8 else 32
    sc = min(nset, LR_SET_CHUNK)
    nn = K.plan(nao, ngrid, nset).exx_nn
    mc = min(nao, budget // row)
    if mc < 1:
        return LrPlan(0, 0, run_len, nrun, tw, sc, nn, row, 0)
    al = K._al
    total = al(row * mc) + 2 * al(row) + al(8 * ngrid) + al(16 * nrun * sc * mc * nao)
    return LrPlan(mc, -(-nao // mc), run_len, nrun, tw, sc, nn, row, total)


def budget_ladder(nao, ngrid, imax):
    """K.budget_ladder with a row m of imax transform rows."""
    row = 16 * imax * ngrid
    return [row - 1, row, row + 1, 2 * row + 7, row * nao - 1, row * nao, row * nao + 1, 0]


def segments(lengths):
    """nset + 1 offsets of the sets' segments."""
    return [0] + [int(x) for x in np.cumsum(lengths)]


# ---- references: wide=True in clongdouble, else complex128 ---------------------------------------
def pair_ref(f1, psi, m0, m1, wide=True):
    """P[(m - m0) I + i][g] = conj(f1[g,m]) psi[g,i]."""
    dt = CLD if wide else np.complex128
    f1, psi = np.asarray(f1).astype(dt), np.asarray(psi).astype(dt)
    out = f1[:, m0:m1].conj().T[:, None, :] * psi.T[None, :, :]
    return out.reshape(-1, f1.shape[0])


def contract_ref(Z, u, f1, mesh, kd, m0, m1, seg, scale, wide=True):
    """K[s][m - m0][n] = scale sum_g t_s[m,g] f1[g,n], t_s[m,g] = conj(em[g]) sum_{i in segment s}
    conj(Z[(m - m0) I + i][g]) u[i][g]; an empty segment gives zeros."""
    dt = CLD if wide else np.complex128
    Z, u, f1 = (np.asarray(x).astype(dt) for x in (Z, u, f1))
    ngrid, nao = f1.shape
    ni = u.shape[0]
    Zc = Z.reshape(m1 - m0, ni, ngrid).conj()
    ce = K.conj_em(mesh, kd, wide)
    out = np.zeros((len(seg) - 1, m1 - m0, nao), dt)
    for s in range(len(seg) - 1):
        a, b = seg[s], seg[s + 1]
        if b > a:
            out[s] = ((Zc[:, a:b] * u[None, a:b]).sum(axis=1) * ce) @ f1
    return out * (LD(scale) if wide else scale)


def dm_of(A, B, ranks, wide=True):
    """D[s][k] = A[s,k][:, :r] B[s,k][:, :r]^H, formed in long double (wide) or complex128; the
    columns beyond r (NaN in the GPU cases) are not read."""
    dt = CLD if wide else np.complex128
    nset, nk, nao = A.shape[:3]
    D = np.zeros((nset, nk, nao, nao), dt)
    for s in range(nset):
        for k in range(nk):
            r = int(ranks[s][k])
            D[s, k] = A[s, k, :, :r].astype(dt) @ B[s, k, :, :r].astype(dt).conj().T
    return D


def exact_k_lr64(f, f_band, kpts, kband, A, B, ranks, a, mesh, omega=0.0):
    """The three low-rank lines in float64 (numpy's fftn):
         pair[m,i,g] = conj(f1[g,m]) psiA_i(g) em[g]
         vR[m,i,g]   = ifft(coulG(q, omega) fft(pair[m,i,:]))[g] conj(em[g])
         K[s][k1][m,n] += scale sum_g (sum_{i<r} vR[m,i,g] conj(psiB_i(g))) f1[g,n]
    with psiA = f_k2 A, psiB = f_k2 B; a k2 / set without orbitals adds nothing."""
    a = np.asarray(a, float)
    f, fb = np.asarray(f, complex), np.asarray(f_band, complex)
    nk, ngrid, nao = f.shape
    nset, nb = A.shape[0], fb.shape[0]
    out = np.zeros((nset, nb, nao, nao), complex)
    for k2 in range(nk):
        for s in range(nset):
            r = int(ranks[s][k2])
            if r == 0:
                continue
            psiA = f[k2] @ np.asarray(A[s, k2, :, :r], complex)             # (g, i)
            psiB = f[k2] @ np.asarray(B[s, k2, :, :r], complex)
            for k1 in range(nb):
                q = np.asarray(kpts[k2], float) - np.asarray(kband[k1], float)
                w = K.coulG(a, q, mesh, omega)
                em = F.phase(mesh, a @ q).ravel().astype(np.complex128)
                pair = fb[k1].conj().T[:, None, :] * psiA.T[None, :, :] * em   # (m, i, g)
                t = np.fft.fftn(pair.reshape(-1, *mesh), axes=(1, 2, 3)).reshape(-1, ngrid)
                v = np.fft.ifftn((t * w).reshape(-1, *mesh), axes=(1, 2, 3)).reshape(-1, ngrid)
                v = (v * em.conj()).reshape(nao, r, ngrid)
                out[s, k1] += (v * psiB.conj().T[None]).sum(axis=1) @ fb[k1]
    return out * (abs(np.linalg.det(a)) / ngrid / nk)


# ---- lowrank_factors ---------------------------------------------------------------------------------
FACTOR_NAOS = (5, 26, 130)


def factor_ranks(nao):
    return (1, 4, nao // 2)


def factor_dm(nao, r, nk=2, seed=0):
    """(dm (nk, nao, nao) = (C n) C^H, C (nk, nao, r) complex normal, n (nk, r) in [0.5, 2])."""
    rng = np.random.default_rng(1000 * nao + 10 * r + seed)
    C = F.rnd(rng, nk, nao, r)
    n = rng.uniform(0.5, 2.0, (nk, r))
    return np.einsum("kai,ki,kbi->kab", C, n, C.conj()), C, n


# ---- the pair cases --------------------------------------------------------------------------------
PAIR_NIS = (1, 3, 13, 33, 70)
PSI_PAD = 3                  # psi's leading dimension is ni + PSI_PAD
PairCase = namedtuple("PairCase", "ngrid nao")
PAIR_CASES = [PairCase(g, n) for g in K.PAIR_NGRIDS for n in K.PAIR_NAOS]


def pair_id(c):
    return "g%d-nao%d" % c


@functools.lru_cache(maxsize=None)
def pair_inputs(c, ni):
    """(f1 (ngrid, nao), psi (ngrid, ni + PSI_PAD), NaN in the padding columns)."""
    rng = np.random.default_rng(100 * c.ngrid + 7 * c.nao + ni)
    psi = np.full((c.ngrid, ni + PSI_PAD), complex(np.nan, np.nan))
    psi[:, :ni] = F.rnd(rng, c.ngrid, ni)
    return F.rnd(rng, c.ngrid, c.nao), psi


# ---- the contraction cases -------------------------------------------------------------------------
# one set; an empty first set; an empty set between two; five sets (three launches, the last of one
# set); a segment of 33; two sets of I = 13
SEG_TABLES = ((4,), (0, 3), (2, 0, 1), (1, 1, 1, 1, 5), (33,), (7, 6))
CONTRACT_NAOS = (1, 3, 13, 33)
WIDE_NAOS = (K.WIDE_NAO, K.GROUPS_NAO)     # three n-tiles; two column groups
TWO_TILE_MESH = (24, 24, 16)               # 144 grid tiles: 72 runs of two tiles
ContractCase = namedtuple("ContractCase", "mesh nao lengths kd_kind")


def _contract_cases():
    """mesh x nao x segment table with the kinds of kd dealt round; nao 76 and 130 (the wide
    n-tile instantiations and the column groups) with every table on the 260-point mesh."""
    out = []
    for i, mesh in enumerate(K.CONTRACT_MESHES):
        for j, nao in enumerate(CONTRACT_NAOS):
            for k, lengths in enumerate(SEG_TABLES):
                out.append(ContractCase(mesh, nao, lengths, K.KD_KINDS[(i + j + k) % 3]))
    for j, nao in enumerate(WIDE_NAOS):
        for k, lengths in enumerate(SEG_TABLES):
            out.append(ContractCase(K.WIDE_MESH, nao, lengths, K.KD_KINDS[(j + k) % 3]))
    out.append(ContractCase(TWO_TILE_MESH, 3, (2, 1), "irrational"))
    return out


CONTRACT_CASES = _contract_cases()


def contract_id(c):
    return "%dx%dx%d-nao%d-seg%s-%s" % (c.mesh + (c.nao, "_".join(map(str, c.lengths)), c.kd_kind))


def contract_kd(c):
    return K.contract_kd(c)


@functools.lru_cache(maxsize=None)
def contract_inputs(c):
    """(Z (nao I, ngrid), u (I, ngrid), f1 (ngrid, nao), vk0 (nset, nao, nao))."""
    ngrid, ni, nset = int(np.prod(c.mesh)), sum(c.lengths), len(c.lengths)
    rng = np.random.default_rng(sum(c.mesh) + 1000 * c.nao + 31 * ni + nset)
    return (F.rnd(rng, c.nao * ni, ngrid), F.rnd(rng, ni, ngrid), F.rnd(rng, ngrid, c.nao),
            F.rnd(rng, nset, c.nao, c.nao))


# ---- the fisdf_get_k_fft_lr cases ------------------------------------------------------------------
# the shapes of K.GETK_CASES with a rank table each, ranks[s][k2]: no orbitals at k2 = 0 (the first
# k2 with work overwrites), none in a whole set, none at a k2 in the middle, unequal ranks
GETK_RANKS = (
    ((4,),),
    ((0, 3), (0, 5)),
    ((1, 0, 2, 3, 1, 2), (0, 0, 0, 0, 0, 0)),
    ((0, 2),),
    ((3, 1, 0, 2, 1, 3),),
    ((2, 1), (1, 3)),
    ((0, 1, 2, 3, 0, 1),),
    ((1, 2, 0, 1, 3, 2), (2, 0, 0, 3, 1, 1)),
)
RMAX_PAD = 2                 # rmax = the largest rank + RMAX_PAD: columns that are never read
LrGetKCase = namedtuple("LrGetKCase", "base ranks")
GETK_CASES = [LrGetKCase(c, r) for c, r in zip(K.GETK_CASES, GETK_RANKS)]


def getk_id(c):
    return K.getk_id(c.base)


def imax_of(ranks):
    return int(np.asarray(ranks).sum(axis=0).max())


def getk_budgets(c):
    """work_bytes giving mc = 1, 2 (nao odd: a partial last chunk) and nao."""
    row = 16 * imax_of(c.ranks) * int(np.prod(c.base.mesh))
    return [row, 2 * row + 5, 0]


@functools.lru_cache(maxsize=None)
def getk_inputs(c):
    """(f, A, B (nset, nk, nao, rmax) with NaN beyond the ranks, ranks (nset, nk) int32, kpts,
    kband or None, f_band or None); f, the k-points and the band AOs are K.getk_inputs'."""
    b = c.base
    f, _, kpts, kband, fband = K.getk_inputs(b)
    ranks = np.asarray(c.ranks, np.int32)
    nk = f.shape[0]
    assert ranks.shape == (b.nset, nk)
    rmax = int(ranks.max()) + RMAX_PAD
    rng = np.random.default_rng(77 + 1000 * b.nao + b.nset + sum(b.kmesh))
    A = np.full((b.nset, nk, b.nao, rmax), complex(np.nan, np.nan))
    B = A.copy()
    for s in range(b.nset):
        for k in range(nk):
            r = ranks[s, k]
            A[s, k, :, :r] = F.rnd(rng, b.nao, r)
            B[s, k, :, :r] = F.rnd(rng, b.nao, r)
    return f, A, B, ranks, kpts, kband, fband


@functools.lru_cache(maxsize=None)
def getk_refs(c):
    """(long-double reference: K.exact_k_ref on D = A B^H formed in long double; err64: the float64
    low-rank restatement's relative distance from it)."""
    b = c.base
    f, A, B, ranks, kpts, kband, fband = getk_inputs(c)
    fo, ko = (f if fband is None else fband), (kpts if kband is None else kband)
    ref = K.exact_k_ref(f, fo, kpts, ko, dm_of(A, B, ranks), K.LATTICE, b.mesh, b.omega)
    mine = exact_k_lr64(f, fo, kpts, ko, A, B, ranks, K.LATTICE, b.mesh, b.omega)
    return ref, K.rel_err(mine, ref)


# ---- end to end ------------------------------------------------------------------------------------
E2E_CASES = ["toy222", "toy331_fr"]
E2E_NOCC = 2


@functools.lru_cache(maxsize=None)
def e2e_orbitals(name, nk, nao):
    """(C (nk, nao, E2E_NOCC) with orthonormal columns, occ (nk, E2E_NOCC) = 2): two random
    orbitals per k-point; dm = (C occ) C^H is Hermitian of rank 2."""
    rng = np.random.default_rng(len(name) + nk + nao)
    C = np.stack([np.linalg.qr(F.rnd(rng, nao, E2E_NOCC))[0] for _ in range(nk)])
    return C, np.full((nk, E2E_NOCC), 2.0)


def e2e_dm(name, nk, nao):
    C, occ = e2e_orbitals(name, nk, nao)
    return np.einsum("kai,ki,kbi->kab", C, occ, C.conj())[None]
