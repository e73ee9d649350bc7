"""Cases, restated rules and references for the exact FFT-grid J (csrc/jfft.hip and its entries in
api.hip): the grid density, the Coulomb potential by two FFTs and the weighted AO Gram.  No tests
and no GPU here: tests/test_jfft_cases.py checks this file on the CPU, tests/test_gpu_jfft.py runs
the device against it.

Three layers, as in tests/factor_cases.py:
  * the launch rules restated (which kernel variant a shape takes, how the Gram splits the grid);
  * the three stages in np.clongdouble (64-bit mantissa), the references;
  * the same sums in plain complex128.  They only measure what float64 arithmetic alone costs
    against the long-double reference: a device result may be factor_cases.BOUND_FACTOR = 16 times
    that far from the reference (another summation order), never less than n eps with n the length
    of the longest sum.  The bound so comes from the reference side, not from the code under test.

Conventions of every kernel case: entries N(0,1) + i N(0,1); the Bloch-AO array in a buffer whose
k blocks are f_kstride = ngrid * nao + KPAD elements apart, with NaN in the gaps and around it;
NaN around the density matrices and around v; the sentinel 7 + 7j around every output.
"""
import functools
from collections import namedtuple

import numpy as np

from factor_cases import BOUND_FACTOR, CLD, EPS, LD, bound  # noqa: F401
from factor_cases import relerr as rel_err
import fft_cases as F

SENTINEL = 7.0 + 7.0j
KPAD = 13          # extra elements between the k blocks of f
EDGE = 5           # NaN / sentinel elements before and after every buffer

# ---- the launch rules, restated ----------------------------------------------------------------
SET_CHUNK = 4      # sets per pass over f (linalg.h kJfftSetChunk)
RHO_NT = 32        # D_sk whole in LDS up to this nao, tiled RHO_NT x RHO_NT beyond it
GRAM_NT = 32       # output tile of the Gram
GRAM_GT = 32       # grid points staged per step of the Gram
GRAM_WGS = 1024    # workgroups the Gram's grid split aims at


def set_chunks(nset):
    """Sets per launch: chunks of SET_CHUNK, the last one short."""
    return [min(SET_CHUNK, nset - s) for s in range(0, nset, SET_CHUNK)]


def rho_point_tile(nao, sets):
    """Grid points per workgroup of rho_grid: 2 per lane for one set with D untiled, else 1."""
    return 128 if nao <= RHO_NT and sets == 1 else 64


def rho_branches(nao, ngrid, nk, nset):
    """Every branch of rho_grid() this shape takes."""
    out = {"d_tiled" if nao > RHO_NT else "d_untiled"}
    for sets in set_chunks(nset):
        pt = rho_point_tile(nao, sets)
        out.add("points_%d" % pt)
        out.add("one_block" if ngrid <= pt else "many_blocks")
        out.add("point_tile_partial" if ngrid % pt else "point_tile_full")
    if nao > RHO_NT and nao % RHO_NT:
        out.add("nao_tile_partial")
    out |= {"sets_%d" % c for c in set_chunks(nset)}
    if nset > SET_CHUNK:
        out.add("set_chunks")
    return out


RHO_BRANCHES = {"d_tiled", "d_untiled", "points_64", "points_128", "one_block", "many_blocks",
                "point_tile_partial", "nao_tile_partial", "sets_1", "sets_2", "sets_3", "sets_4",
                "set_chunks"}


def gram_split(nk, ngrid, nao):
    """(chunk, nsplit) of weighted_gram_split: about GRAM_WGS workgroups, at least four grid
    steps per split, the chunk a whole number of steps."""
    ntile = -(-nao // GRAM_NT)
    wgs = nk * ntile * ntile
    want = max(1, -(-GRAM_WGS // wgs))
    want = min(want, max(1, -(-ngrid // (4 * GRAM_GT))))
    c = -(-ngrid // want)
    c = -(-c // GRAM_GT) * GRAM_GT
    return c, -(-ngrid // c)


def gram_branches(nao, ngrid, nk, nset):
    chunk, nsplit = gram_split(nk, ngrid, nao)
    out = {"one_tile" if nao <= GRAM_NT else "many_tiles"}
    if nao % GRAM_NT:
        out.add("nao_tile_partial")
    out.add("one_split" if nsplit == 1 else "many_splits")
    last = ngrid - (nsplit - 1) * chunk
    if last % GRAM_GT:
        out.add("grid_step_partial")
    out |= {"sets_%d" % c for c in set_chunks(nset)}
    if nset > SET_CHUNK:
        out.add("set_chunks")
    return out


GRAM_BRANCHES = {"one_tile", "many_tiles", "nao_tile_partial", "one_split", "many_splits",
                 "grid_step_partial", "sets_1", "sets_2", "sets_3", "sets_4", "set_chunks"}

# ---- the kernel cases --------------------------------------------------------------------------
# herm: Hermitian D (rho) / real v (Gram); conj_v: the Gram reads conj(v)
Case = namedtuple("Case", "nao ngrid nk nset herm conj_v")
KERNEL_CASES = [
    Case(1, 64, 1, 1, True, 0),          # the smallest corner: below one point tile
    Case(8, 997, 2, 3, False, 1),        # prime grid, 3 sets
    Case(26, 1000, 27, 1, True, 0),      # the C3 AO count, 27 k-points
    Case(26, 1728, 2, 5, False, 0),      # set chunks 4 + 1
    Case(8, 1000, 1, 2, True, 1),        # 2 sets
    Case(33, 1000, 2, 1, False, 1),      # D tiled, one column over the tile
    Case(76, 997, 1, 3, True, 1),        # D tiled 3 x 3
    Case(130, 997, 1, 1, False, 0),      # D tiled 5 x 5, partial last tile
    Case(130, 64, 2, 5, True, 0),        # tiled and chunked, one block
    Case(1, 1728, 27, 5, False, 1),      # nao 1 with every set chunk
]


def case_id(c):
    return "nao%d-g%d-k%d-s%d-%s-c%d" % (c.nao, c.ngrid, c.nk, c.nset, "h" if c.herm else "g",
                                         c.conj_v)


def rho_sum_length(c):
    return c.nk * c.nao * c.nao


def gram_sum_length(c):
    return c.ngrid


@functools.lru_cache(maxsize=None)
def kernel_inputs(c):
    """(f, D, v) of a case: f (nk, ngrid, nao), D (nset, nk, nao, nao) Hermitian on request,
    v (nset, ngrid) real on request (stored complex)."""
    rng = np.random.default_rng(1000 * c.nao + c.ngrid + 7 * c.nk + c.nset)
    f = F.rnd(rng, c.nk, c.ngrid, c.nao)
    D = F.rnd(rng, c.nset, c.nk, c.nao, c.nao)
    v = F.rnd(rng, c.nset, c.ngrid)
    if c.herm:
        D = D + D.conj().swapaxes(-1, -2)
        v = v.real + 0j
    return f, D, v


# ---- the three stages: wide=True in clongdouble, else complex128 -----------------------------
def rho_ref(f, D, wide=True):
    """rho[s][g] = (1/nk) sum_k sum_mn f_k[g,m] D[s,k][m,n] conj(f_k[g,n])."""
    dt = CLD if wide else np.complex128
    f, D = np.asarray(f).astype(dt), np.asarray(D).astype(dt)
    nk = f.shape[0]
    out = np.zeros((D.shape[0], f.shape[1]), dt)
    for s in range(D.shape[0]):
        for k in range(nk):
            out[s] += ((f[k] @ D[s, k]) * f[k].conj()).sum(axis=1)
    return out / nk


def gram_ref(f, v, conj_v=0, scale=1.0, wide=True):
    """out[s][k][m][n] = scale sum_g conj(f_k[g,m]) v_s[g] f_k[g,n] (conj_v: conj(v_s[g]))."""
    dt = CLD if wide else np.complex128
    f, v = np.asarray(f).astype(dt), np.asarray(v).astype(dt)
    if conj_v:
        v = v.conj()
    nk, ngrid, nao = f.shape
    out = np.zeros((v.shape[0], nk, nao, nao), dt)
    for s in range(v.shape[0]):
        for k in range(nk):
            out[s, k] = (f[k].conj().T * v[s]) @ f[k]
    return out * (LD(scale) if wide else scale)


def coulG(a, mesh, omega=0.0):
    """coulG(k = 0) of the oracle (float64: the device forms it in float64 too)."""
    from oracle.isdf_ref import get_coulG
    return get_coulG(np.asarray(a, float), np.zeros(3), mesh, omega=omega or None)


def potential_ref(rho, a, mesh, omega=0.0, wide=True):
    """v_s = ifft(coulG fft(rho_s)): long double by the separable DFT of fft_cases, the inverse as
    conj(fft(conj(x))) / N; float64 by scipy's fftn / ifftn (the oracle's fft / ifft)."""
    w = coulG(a, mesh, omega)
    if not wide:
        from oracle.isdf_ref import fft, ifft
        return ifft(fft(np.asarray(rho, complex), mesh) * w, mesh)
    n = LD(int(np.prod(mesh)))
    t = F.ref_fft3d(rho, mesh) * w.astype(LD)
    return F.ref_fft3d(t.conj(), mesh).conj() / n


def exact_j64(chi, dms, a, mesh, omega=0.0):
    """The float64 restatement composed end to end: oracle.exact_ref.exact_j, with coulG(omega)."""
    nk, ngrid, nao = chi.shape
    vol = abs(np.linalg.det(a))
    v = potential_ref(rho_ref(chi, dms, wide=False), a, mesh, omega, wide=False)
    return gram_ref(chi, v, 0, vol / ngrid, wide=False)


def exact_v(chi, dms, a, mesh, omega=0.0):
    """The exact potential on the grid (float64), for J at band k-points."""
    return potential_ref(rho_ref(chi, dms, wide=False), a, mesh, omega, wide=False)


# ---- the potential cases -----------------------------------------------------------------------
LATTICE = np.array([[6.1, 0.2, -0.3], [0.4, 6.7, 0.1], [-0.2, 0.5, 7.3]])
AXES_MESH = F.AXES_MESHES[1]           # (2, 64, 48): three axis passes
PotCase = namedtuple("PotCase", "mesh omega nset")
POTENTIAL_CASES = [
    PotCase((12, 12, 12), 0.0, 1), PotCase((12, 12, 12), 0.4, 3), PotCase((15, 15, 15), -0.4, 3),
    PotCase((12, 12, 12), -0.4, 1), PotCase((15, 15, 15), 0.4, 1),
    PotCase((15, 15, 15), 0.0, 1), PotCase((10, 10, 10), 0.4, 1), PotCase((10, 10, 10), -0.4, 3),
    PotCase((10, 10, 10), 0.0, 3), PotCase(AXES_MESH, 0.0, 3), PotCase(AXES_MESH, -0.4, 1),
    PotCase(AXES_MESH, 0.4, 1),
]
POTENTIAL_ROUTES = {(12, 12, 12): F.REG, (15, 15, 15): F.REG, (10, 10, 10): F.PLANE,
                    AXES_MESH: F.AXES}
REFUSED_MESH = (17, 8, 8)


def pot_id(c):
    return "%dx%dx%d-w%g-s%d" % (c.mesh + (c.omega, c.nset))


@functools.lru_cache(maxsize=None)
def potential_inputs(c):
    rng = np.random.default_rng(sum(c.mesh) + c.nset)
    return F.rnd(rng, c.nset, int(np.prod(c.mesh)))


# ---- end to end ----------------------------------------------------------------------------------
JK_TOL = 1e-8
E2E_CASES = ["toy333_fr", "toy331_fr", "toy666", "nio_small", "si_small"]
