"""Cases, restated rules and references for the separable k-mesh transforms: the y build
(kmesh_y_reg_kernel, kmesh_y_kernel, y_fused_kernel and its copies in linalg.hip), x4
(build_x4_on), get_k's pair (k_wsrho_reg_kernel, or two dense Phi GEMMs) and the Bloch AO's DFT
(ao.hip).  No tests and no GPU here: tests/test_kmesh_cases.py checks this file on the CPU,
tests/test_gpu_kmesh_variants.py runs the device against it.

Three layers, as in tests/factor_cases.py:
  * the launch rules restated (the compiled mesh list, the route of a transform, the LDS kernel's
    tile tiers, time reversal's partner / representative / slot / runs, the fused kernel's slot
    plan, workspace and tile walk), compared with fisdf_kmesh_plan;
  * every transform in np.clongdouble (64-bit mantissa) with twiddles exp(2 pi i t / n) whose
    index t = x j mod n is reduced as an integer (and exact at the quarter turns), the references;
  * the same sums in plain complex128.  They only measure what float64 arithmetic alone costs
    against the long-double reference: a device result may be factor_cases.BOUND_FACTOR = 16 times
    that far from the reference (another summation order, the butterflies, the 3-multiplication
    complex product), never less than n eps with n the length of the longest sum.  The bound so
    comes from the reference side, not from the code under test.

Conventions of every device case: entries N(0,1) + i N(0,1); NaN around every input and in every
row a kernel must not read; the sentinel 7 + 7j around every output and in every element of it
that must not be written.
"""
import functools
import itertools
from collections import namedtuple

import numpy as np

from factor_cases import BOUND_FACTOR, CLD, EPS, LD, bound  # noqa: F401
from factor_cases import relerr as rel_err  # noqa: F401
from fft_cases import PI, rnd  # noqa: F401
from jfft_cases import EDGE, SENTINEL  # noqa: F401

# ---- the launch rules, restated ----------------------------------------------------------------
REG, LDS, REFUSED = 0, 1, 2
# the k-meshes with compile-time instantiations (linalg.h FISDF_KM_REG_MESHES)
REG_MESHES = [(1, 1, 1), (1, 1, 2), (2, 2, 2), (3, 3, 1), (3, 3, 3), (4, 4, 4), (2, 2, 1),
              (1, 2, 2), (4, 4, 1), (2, 2, 4)]
UNRUN_BEFORE = [(2, 2, 1), (1, 2, 2), (4, 4, 1), (2, 2, 4)]   # launched by no test before these
KM_MAXN = 16
LDS_TILE_MAX = 64 * 1024       # the tile rule: nk x (CT + 1) complex + the twiddles
LDS_CAP = 160 * 1024
YF_KCHUNK = 28                 # nao per K chunk of the fused kernel (4 x YF_MAXKS)
YF_LDS_MAX = 80 * 1024
YF_NAO_MAX = 128
GPAIR = 4                      # g-tiles per group of the fused kernel's XCD walk


def nk_of(kmesh):
    return int(kmesh[0]) * int(kmesh[1]) * int(kmesh[2])


def route(kmesh, ncol=1):
    """(route, CT, lds bytes) of kmesh_route(): the register kernels for a listed mesh and
    ncol < 2^31; else tiles of CT columns, 64 halved down to 8 until the tile fits 64 KB, the
    launch asking for the tile, the twiddles and the nk-entry source table; refused above 16 per
    axis, above 160 KB, or from 2^31 tiles."""
    if min(kmesh) < 1 or max(kmesh) > KM_MAXN:
        return (REFUSED, 0, 0)
    nk = nk_of(kmesh)
    if tuple(kmesh) in REG_MESHES and ncol < 2 ** 31:
        return (REG, 0, 0)
    ct = 64
    while ct > 8 and 16 * (nk * (ct + 1) + 3 * KM_MAXN) > LDS_TILE_MAX:
        ct //= 2
    lds = 16 * (nk * (ct + 1) + 3 * KM_MAXN) + 4 * nk
    if lds > LDS_CAP or -(-ncol // ct) >= 2 ** 31:
        return (REFUSED, ct, lds)
    return (LDS, ct, lds)


def partner(kmesh):
    """index of -k for every k (k = (a n1 + b) n2 + c)."""
    n0, n1, n2 = kmesh
    a, b, c = np.unravel_index(np.arange(nk_of(kmesh)), kmesh)
    return (((n0 - a) % n0) * n1 + (n1 - b) % n1) * n2 + (n2 - c) % n2


def reps(kmesh):
    """the stored k under time reversal: k <= -k, ascending."""
    p = partner(kmesh)
    return np.flatnonzero(np.arange(p.size) <= p)


def rep_slot(kmesh):
    """slot[k]: the row of representative k (the number of representatives below it)."""
    p = partner(kmesh)
    isrep = np.arange(p.size) <= p
    return np.cumsum(isrep) - isrep


def rep_runs(kmesh):
    """the representatives as [begin, end) runs of consecutive k."""
    r, out = reps(kmesh), []
    for k in r:
        if out and out[-1][1] == k:
            out[-1][1] = k + 1
        else:
            out.append([int(k), int(k) + 1])
    return [tuple(x) for x in out]


def self_conjugate(kmesh):
    p = partner(kmesh)
    return np.flatnonzero(p == np.arange(p.size))


def inplane_partner(n1, n2):
    bc = np.arange(n1 * n2)
    return ((n1 - bc // n2) % n1) * n2 + (n2 - bc % n2) % n2


def inplane_rank(n1, n2):
    """rank[bc]: the in-plane representatives bc <= -bc below bc."""
    p = inplane_partner(n1, n2)
    isrep = np.arange(p.size) <= p
    return np.cumsum(isrep) - isrep


FusedPlan = namedtuple("FusedPlan", "applies nA nB kA kB lds nkc")
NO_FUSED = FusedPlan(False, 0, 0, (), (), 0, 0)


def fused_plan(kmesh, nao):
    """y_fused_plan(): chunk A = plane 1 whole (n0 >= 3), chunk B = the self-paired planes 0 (and
    n0 / 2) at their in-plane representatives; 4 KB of LDS per slot of the larger chunk."""
    n0, n1, n2 = kmesh
    P = n1 * n2
    if tuple(kmesh) not in REG_MESHES or not 1 <= nao <= YF_NAO_MAX or n0 > 4 or P > 16:
        return NO_FUSED
    kA = tuple(P + bc for bc in range(P)) if n0 >= 3 else ()
    p = inplane_partner(n1, n2)
    planes = (0, n0 // 2) if n0 % 2 == 0 and n0 > 1 else (0,)
    kB = tuple(a * P + bc for a in planes for bc in range(P) if bc <= p[bc])
    lds = 16 * 256 * max(len(kA), len(kB))
    if lds > YF_LDS_MAX:
        return NO_FUSED
    return FusedPlan(True, len(kA), len(kB), kA, kB, lds, -(-nao // YF_KCHUNK))


def fused_workspace(kmesh, nip, nao, m):
    """y_fused_workspace(): an upper bound of the slot count (from the shape alone, the mesh list
    is not consulted) times the mu-major copies of X and f."""
    n0, P = kmesh[0], kmesh[1] * kmesh[2]
    if n0 * P > 64 or n0 > 4 or P > 16 or m <= 0 or nip <= 0 or nao > YF_NAO_MAX:
        return 0
    nr = 2 if n0 % 2 == 0 and n0 > 1 else 1
    nslot = (P if n0 >= 3 else 0) + nr * P
    return 16 * nslot * nao * (nip + m)


def tile_walk(nIt, nGt, gpair=GPAIR):
    """(it, gt) of every workgroup id of y_fused_kernel (None: the workgroup returns at once):
    id & 7 is the XCD, an XCD walks its g-tiles in groups of gpair, the I-tiles slowest within a
    group."""
    grid = nIt * -(-nGt // (8 * gpair)) * gpair * 8
    out = []
    for b in range(grid):
        xcd, j = b & 7, b >> 3
        grp, rem = divmod(j, nIt * gpair)
        it, gt = rem // gpair, (grp * gpair + rem % gpair) * 8 + xcd
        out.append((it, gt) if gt < nGt else None)
    return out


# ---- twiddles and the transform ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def twiddles(n):
    """exp(2 pi i t / n), t < n, in long double; exact at the quarter turns."""
    t = np.arange(n)
    th = 2 * PI * t.astype(LD) / LD(n)
    w = np.empty(n, CLD)
    w.real, w.imag = np.cos(th), np.sin(th)
    for q, v in ((0, 1), (1, 1j), (2, -1), (3, -1j)):
        if (q * n) % 4 == 0:
            w[q * n // 4] = v
    return w


@functools.lru_cache(maxsize=None)
def dft_matrix(n, wide=True):
    """W[x, j] = exp(+2 pi i x j / n), the index x j reduced mod n as an integer."""
    x = np.arange(n)
    w = twiddles(n)[np.outer(x, x) % n]
    return w if wide else w.astype(np.complex128)


def mesh_dft(x, kmesh, wide=True, scale=True):
    """sum_R exp(+2 pi i sum_a r_a k_a / n_a) x[R] along the first axis of x (nk, ...), one
    product per mesh axis; scale: times 1 / sqrt(nk), which makes it Phi (= Phi^T)."""
    dt = CLD if wide else np.complex128
    a = np.asarray(x).astype(dt)
    shape = a.shape
    a = a.reshape(tuple(kmesh) + (-1,))
    for ax in range(3):
        if kmesh[ax] > 1:
            a = np.moveaxis(np.tensordot(dft_matrix(kmesh[ax], wide), a, axes=([1], [ax])), 0, ax)
    a = a.reshape(shape)
    if scale:
        nk = nk_of(kmesh)
        a = a / (np.sqrt(LD(nk)) if wide else np.sqrt(float(nk)))
    return a


def extend_half(fx_reps, kmesh):
    """all nk rows from the representatives' rows: row k = conj(row -k) for the others."""
    p, slot = partner(kmesh), rep_slot(kmesh)
    k = np.arange(p.size)
    rows = np.where(k <= p, slot, slot[p])
    out = np.asarray(fx_reps)[rows]
    mirror = k > p
    out[mirror] = out[mirror].conj()
    return out


# ---- the references: wide=True in clongdouble, else complex128 ---------------------------------
def y_ref(fx, kmesh, qs=None, conj_out=False, wide=True, with_scale=False):
    """(y[q] for q in qs, max |Im fx_s|): fx_s = Phi fx_k, y_s = Re(fx_s)^2, y_k = Phi^T y_s.
    with_scale: also max |fx_s|, the size of the field whose imaginary part is monitored."""
    fx_s = mesh_dft(fx, kmesh, wide)
    mon = float(np.abs(fx_s.imag).max()) if fx_s.size else 0.0
    y = mesh_dft(fx_s.real ** 2, kmesh, wide)
    if conj_out:
        y = y.conj()
    out = ((y if qs is None else y[np.asarray(qs, int)]), mon)
    return out + (float(np.abs(fx_s).max()),) if with_scale else out


def fx_ref(X, F, wide=True):
    """fx_k[I, g] = sum_mu X_k[I, mu] conj(F_k[g, mu])."""
    dt = CLD if wide else np.complex128
    return np.einsum("kim,kgm->kig", np.asarray(X).astype(dt), np.asarray(F).astype(dt).conj())


def x2_ref(X, wide=True):
    """x2_k[I, J] = sum_mu conj(X_k[I, mu]) X_k[J, mu]."""
    dt = CLD if wide else np.complex128
    X = np.asarray(X).astype(dt)
    return np.einsum("kim,kjm->kij", X.conj(), X)


def x4_ref(X, kmesh, wide=True):
    """(x4_k = Phi^H (Phi x2_k)^2, max |Im Phi x2_k|); the square is complex, as fftisdf.py:45."""
    x2_s = mesh_dft(x2_ref(X, wide), kmesh, wide)
    mon = float(np.abs(x2_s.imag).max())
    return mesh_dft((x2_s * x2_s).conj(), kmesh, wide).conj(), mon


def wsrho_ref(B, Ws, kmesh, wide=True, with_scale=False):
    """(V_k = Phi^T (W_s Re(Phi B)), max |Im Phi B|); with_scale: also max |Phi B|."""
    rho_s = mesh_dft(B, kmesh, wide)
    mon = float(np.abs(rho_s.imag).max())
    w = np.asarray(Ws).astype(LD if wide else np.float64)
    out = (mesh_dft(w * rho_s.real, kmesh, wide), mon)
    return out + (float(np.abs(rho_s).max()),) if with_scale else out


def lattice_phase64(kmesh, a):
    """Phi[R, q] = exp(i T_R . k_q) / sqrt(nk) as the dense path forms it in float64: T_R = r . a,
    k_q = (i / n) . b with b = 2 pi inv(a)^T."""
    a = np.asarray(a, float).reshape(3, 3)
    b = 2 * np.pi * np.linalg.inv(a).T
    r = np.array(list(itertools.product(*[range(n) for n in kmesh])), float)
    T, k = r @ a, (r / np.asarray(kmesh, float)) @ b
    return np.exp(1j * (T @ k.T)) / np.sqrt(float(nk_of(kmesh)))


def wsrho_dense64(B, Ws, kmesh, a):
    """the float64 restatement of the dense path: two products with the lattice's Phi."""
    phi = lattice_phase64(kmesh, a)
    rho_s = phi @ np.asarray(B, complex)
    return phi.T @ (np.asarray(Ws, float) * rho_s.real), float(np.abs(rho_s.imag).max())


def bloch_ref(F, kmesh, wide=True):
    """chi[k] = sum_R exp(2 pi i sum_a r_a k_a / n_a) F[R], F real, not normalised."""
    return mesh_dft(np.asarray(F, float), kmesh, wide, scale=False)


def band_ref(F, ph, wide=True):
    """chi[k][c] = sum_t ph[t][k] F[t][c]."""
    dt = CLD if wide else np.complex128
    F, ph = np.asarray(F, float), np.asarray(ph)
    if F.shape[0] == 0:
        return np.zeros((ph.shape[1], F.shape[1]), dt)
    return ph.astype(dt).T @ F.astype(dt)


# ---- inputs --------------------------------------------------------------------------------------
def tr_symmetric(rng, kmesh, *shape):
    """x[-k] = conj(x[k]) (real at the self-conjugate k), N(0,1) + i N(0,1) at the rest."""
    x = rnd(rng, nk_of(kmesh), *shape)
    p = partner(kmesh)
    for k in range(p.size):
        if p[k] == k:
            x[k] = x[k].real
        elif p[k] < k:
            x[k] = x[p[k]].conj()
    return x


def q_lists(kmesh):
    """all q; the first alone; the last alone; every other q with the last (not contiguous)."""
    nk = nk_of(kmesh)
    out = [list(range(nk))]
    if nk > 1:
        out += [[0], [nk - 1]]
    if nk > 3:
        out.append(sorted(set(range(1, nk, 2)) | {nk - 1}))
    return out


def mask_of(qs):
    return sum(1 << int(q) for q in qs)


# ---- the case tables -------------------------------------------------------------------------------
# register y transform: every mesh x half x conj_out; (ncol, m, goff, Is slack) shapes
RegY = namedtuple("RegY", "kmesh ncol m goff pad half conj_out qsel")
REG_SHAPES = [(1, 1, 0, 0), (63, 7, 0, 0), (64, 64, 3, 2), (65, 7, 0, 5), (200, 200, 5, 3)]


def _reg_cases():
    out = []
    for i, km in enumerate(REG_MESHES):
        for half, conj in itertools.product((0, 1), (0, 1)):
            nql = len(q_lists(km))
            for j, (ncol, m, goff, pad) in enumerate(REG_SHAPES):
                out.append(RegY(km, ncol, m, goff, pad, half, conj, (i + j + half + 2 * conj) % nql))
    return out


REG_Y_CASES = _reg_cases()
REG_Y_BIT63 = RegY((4, 4, 4), 65, 7, 2, 1, 1, 0, 2)          # q-list [63]: bit 63 of the mask
REG_Y_STRIDE = RegY((1, 1, 2), 64 * 32768 + 65, 4099, 0, 0, 0, 0, 0)   # beyond the 32768 workgroups
REG_GRID_CAP = 32768

# LDS y transform: mesh -> the tier it must take
LDS_MESHES = {(1, 1, 3): 64, (3, 1, 2): 64, (2, 3, 1): 64, (8, 8, 1): 32, (7, 9, 1): 32,
              (5, 5, 5): 16, (2, 9, 13): 16, (15, 16, 1): 8, (7, 8, 8): 8, (16, 16, 4): 8,
              (16, 1, 1): 64, (1, 16, 1): 64, (1, 1, 16): 64}
LDS_ABOVE_64K = (7, 8, 8)
LDS_NEAR_CAP = (16, 16, 4)
LDS_GRID_CAP = 4096
LdsY = namedtuple("LdsY", "kmesh ncol m goff pad half qsel")


def _lds_cases():
    out = []
    for i, (km, ct) in enumerate(LDS_MESHES.items()):
        for half in (0, 1):
            for j, ncol in enumerate((1, ct - 1, ct + 1, 3 * ct + 5)):
                m = ncol if j % 2 else max(1, min(ncol, 7))
                out.append(LdsY(km, ncol, m, j, j % 2, half, (i + j + half) % len(q_lists(km))))
    return out


LDS_Y_CASES = _lds_cases()
LDS_Y_STRIDE = LdsY((1, 1, 3), LDS_GRID_CAP * 64 + 65, 1031, 0, 0, 1, 0)
REFUSED_MESHES = [(17, 1, 1), (16, 16, 5)]

# fused y: (kmesh, nip, m, nao, goff, pad, qsel, rmask kind)
Fused = namedtuple("Fused", "kmesh nip m nao goff pad qsel real")
FUSED_NAO = (1, 2, 3, 4, 27, 28, 29, 31, 56, 57, 76, 128)
FUSED_NIP = (1, 15, 16, 200)
FUSED_M = (1, 15, 16, 512, 513, 530)


def _fused_cases():
    out = [Fused(km, 17, 17, 5, 0, 0, i % len(q_lists(km)), 0) for i, km in enumerate(REG_MESHES)]
    for km in ((2, 2, 2), (4, 4, 1)):
        out += [Fused(km, 17, 17, nao, 2, 3, i % len(q_lists(km)), 0)
                for i, nao in enumerate(FUSED_NAO)]
    for km in ((2, 2, 1), (3, 3, 1)):
        out += [Fused(km, nip, 17, 5, 0, 0, 0, 0) for nip in FUSED_NIP]
        out += [Fused(km, 17, m, 5, 1, 2, 0, 0) for m in FUSED_M]
        out.append(Fused(km, 33, 530, 6, 0, 0, 0, 0))     # a second XCD group, partial, 3 I-tiles
    # the real store: every self-conjugate q (real = 1), and q = 0 only of (3,3,3)
    out += [Fused(km, 17, 19, 5, 1, 2, 0, 1) for km in ((2, 2, 2), (4, 4, 4), (2, 2, 4), (3, 3, 3))]
    # a q-subset with real slots and a bit of rmask outside it (real = 2)
    out += [Fused(km, 17, 19, 5, 0, 0, 3, 2) for km in ((2, 2, 2), (4, 4, 4), (2, 2, 4))]
    return out


FUSED_CASES = _fused_cases()
FUSED_REFUSED_NAO = 129
Streamed = namedtuple("Streamed", "kmesh nip rows two m nao ng0")
STREAMED_CASES = [Streamed(km, 100, rows, two, 21, 5, 37)
                  for km in ((2, 2, 2), (4, 4, 4)) for rows in (16, 48) for two in (0, 1)]

# x4: (kmesh, nip, nao, time reversal, dense)
X4 = namedtuple("X4", "kmesh nip nao tr dense")
X4_SHAPES = [(1, 3), (17, 8), (65, 3)]
X4_DENSE_MESHES = [(2, 2, 1), (4, 4, 1), (1, 1, 3)]
X4_CASES = ([X4(km, *X4_SHAPES[(i + tr) % 3], tr, 0) for i, km in enumerate(REG_MESHES)
             for tr in (0, 1)]
            + [X4(km, nip, nao, 0, 0) for km in ((2, 2, 4),) for nip, nao in X4_SHAPES]
            + [X4(km, 17, 8, tr, 1) for km in X4_DENSE_MESHES for tr in (0, 1)])

# get_k's pair
WSRHO_NCOL = (1, 65, 300)
WSRHO_PAD = 11                 # ws_Rstride - ncol, NaN in the gap
WSRHO_OFF_LIST = (1, 1, 3)
WSRHO_PAIR_TOL = 1e-13         # register against dense, test_get_k_register_transform's
LATTICE = np.array([[6.1, 0.2, -0.3], [0.4, 6.7, 0.1], [-0.2, 0.5, 7.3]])

# Bloch AO
BLOCH_NCOL = (1, 65, 1000)
BLOCH_GENERIC = [(1, 1, 3), (3, 1, 2), (5, 5, 5)]
BLOCH_STRIDE = ((1, 1, 1), 64 * 65536 + 65)                  # beyond the 65536 workgroups
BLOCH_GRID_CAP = 65536
BAND_NT = (0, 1, 27)
BAND_NKB = (1, 3)


def case_id(c):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c)


# ---- what a case reaches -------------------------------------------------------------------------
def fused_branches(c):
    """the branches of y_fused_kernel / yf_mfma_chunk a fused case takes."""
    p = fused_plan(c.kmesh, c.nao)
    nIt, nGt = -(-c.nip // 16), -(-c.m // 16)
    out = {"mesh_%dx%dx%d" % c.kmesh, "nkc_%d" % p.nkc, "nao_mod4_%d" % (c.nao % 4)}
    if c.nao % YF_KCHUNK and (c.nao % YF_KCHUNK) <= YF_KCHUNK - 4:
        out.add("k_break_inside_chunk")
    if 0 < p.nA < 4 or 0 < p.nB < 4:
        out.add("idle_waves")
    if c.nip % 16:
        out.add("partial_I_tile")
    if c.m % 16:
        out.add("partial_g_tile")
    if nGt > 8 * GPAIR:
        out.add("second_group")
        if nGt % (8 * GPAIR):
            out.add("second_group_partial")
    if nIt > 1:
        out.add("many_I_tiles")
    return out


FUSED_BRANCHES = ({"mesh_%dx%dx%d" % km for km in REG_MESHES}
                  | {"nkc_1", "nkc_2", "nkc_3", "nkc_5", "nao_mod4_0", "nao_mod4_1", "nao_mod4_2",
                     "nao_mod4_3", "k_break_inside_chunk", "idle_waves", "partial_I_tile",
                     "partial_g_tile", "second_group", "second_group_partial", "many_I_tiles"})


# ---- inputs and references of the device cases (computed once, shared) -------------------------
# The monitor, max |Im| of the s-space field, is compared like every other output: its error is
# taken relative to the largest magnitude of that field (`scale`), not to the monitor itself.  The
# rounding of an imaginary part grows with the field, and under time reversal (or for the
# symmetric X of the x4 cases) the monitor is a rounding residue or zero, where an error relative
# to it means nothing.
YData = namedtuple("YData", "fx qs ref mon scale err64 mon64 nsum")


@functools.lru_cache(maxsize=None)
def y_data(kmesh, ncol, half, conj_out, qsel):
    """FX as the kernel is given it (the representatives' rows only under half), the q-list, the
    long-double y and monitor, and the float64 restatement's distance from both."""
    rng = np.random.default_rng(1000 * nk_of(kmesh) + 7 * ncol + 2 * half + conj_out + 31 * qsel)
    nrow = len(reps(kmesh)) if half else nk_of(kmesh)
    fx = rnd(rng, nrow, ncol)
    full = extend_half(fx, kmesh) if half else fx
    qs = q_lists(kmesh)[qsel]
    ref, mon, scale = y_ref(full, kmesh, qs, conj_out, with_scale=True)
    r64, m64 = y_ref(full, kmesh, qs, conj_out, wide=False)
    return YData(fx, qs, ref, mon, scale, rel_err(r64, ref), abs(m64 - mon) / scale, nk_of(kmesh))


FusedData = namedtuple("FusedData", "X F fullX fullF ref err64 nsum")


@functools.lru_cache(maxsize=None)
def fused_data(kmesh, nip, m, nao):
    """X (nk, nip, nao) and F (nk, m, nao): random at the plan's k, NaN at the others; the
    reference from the conjugate extension; y for every q."""
    rng = np.random.default_rng(100000 * nk_of(kmesh) + 1000 * nip + 10 * m + nao + kmesh[2])
    p, nk = partner(kmesh), nk_of(kmesh)
    plan = fused_plan(kmesh, min(nao, YF_NAO_MAX))
    ks = sorted(plan.kA + plan.kB)
    assert ks == list(reps(kmesh))
    X, F = rnd(rng, nk, nip, nao), rnd(rng, nk, m, nao)
    fullX, fullF = X.copy(), F.copy()
    for k in range(nk):
        if k not in ks:
            fullX[k], fullF[k] = X[p[k]].conj(), F[p[k]].conj()
            X[k], F[k] = np.nan, np.nan
    ref = y_ref(fx_ref(fullX, fullF).reshape(nk, nip * m), kmesh)[0]
    r64 = y_ref(fx_ref(fullX, fullF, wide=False).reshape(nk, nip * m), kmesh, wide=False)[0]
    return FusedData(X, F, fullX, fullF, ref.reshape(nk, nip, m), rel_err(r64, ref), max(nao, nk))


def x4_dense64(X, kmesh, a):
    """the float64 restatement of the dense x4 path: Phi^H (Phi x2_k)^2 with the lattice's Phi."""
    phi = lattice_phase64(kmesh, a)
    x2 = x2_ref(X, wide=False)
    x2_s = phi @ x2.reshape(x2.shape[0], -1)
    return (phi.conj().T @ (x2_s * x2_s)).reshape(x2.shape)


X4Data = namedtuple("X4Data", "X ref mon scale err64 err64_dense nsum")


@functools.lru_cache(maxsize=None)
def x4_data(kmesh, nip, nao):
    """X with X[-k] = conj(X[k]), so that the complex square of the dense path and the real one of
    the register path are the same numbers up to rounding; scale = max |x2_s|, what the monitor
    (max |Im x2_s|, zero in exact arithmetic) is measured against."""
    rng = np.random.default_rng(5000 * nk_of(kmesh) + 10 * nip + nao + kmesh[0])
    X = tr_symmetric(rng, kmesh, nip, nao)
    ref, mon = x4_ref(X, kmesh)
    r64, _ = x4_ref(X, kmesh, wide=False)
    scale = float(np.abs(mesh_dft(x2_ref(X), kmesh)).max())
    return X4Data(X, ref, mon, scale, rel_err(r64, ref),
                  rel_err(x4_dense64(X, kmesh, LATTICE), ref), max(nao, nk_of(kmesh)))


WsData = namedtuple("WsData", "B Ws ref mon scale err64 err64_dense mon64 nsum")


@functools.lru_cache(maxsize=None)
def wsrho_data(kmesh, ncol):
    rng = np.random.default_rng(77 * nk_of(kmesh) + ncol + kmesh[1])
    nk = nk_of(kmesh)
    B, Ws = rnd(rng, nk, ncol), rng.standard_normal((nk, ncol))
    ref, mon, scale = wsrho_ref(B, Ws, kmesh, with_scale=True)
    r64, m64 = wsrho_ref(B, Ws, kmesh, wide=False)
    d64, _ = wsrho_dense64(B, Ws, kmesh, LATTICE)
    return WsData(B, Ws, ref, mon, scale, rel_err(r64, ref), rel_err(d64, ref),
                  abs(m64 - mon) / scale, nk)


BlochData = namedtuple("BlochData", "F ref err64 nsum")


@functools.lru_cache(maxsize=None)
def bloch_data(kmesh, ncol):
    rng = np.random.default_rng(13 * nk_of(kmesh) + ncol + kmesh[2])
    F = rng.standard_normal((nk_of(kmesh), ncol))
    ref = bloch_ref(F, kmesh)
    return BlochData(F, ref, rel_err(bloch_ref(F, kmesh, wide=False), ref), nk_of(kmesh))


BandData = namedtuple("BandData", "F ph ref err64 nsum")


@functools.lru_cache(maxsize=None)
def band_data(nT, nkb, ncol):
    rng = np.random.default_rng(1000 * nT + 10 * nkb + ncol)
    F = rng.standard_normal((nT, ncol))
    th = rng.uniform(-20, 20, (max(nT, 1), nkb))
    ph = np.cos(th) + 1j * np.sin(th)
    ref = band_ref(F, ph[:nT])
    return BandData(F, ph, ref, rel_err(band_ref(F, ph[:nT], wide=False), ref), max(nT, 1))


StreamData = namedtuple("StreamData", "x0 piv F ref err64 nsum")


@functools.lru_cache(maxsize=None)
def streamed_data(kmesh, nip, m, nao, ng0):
    """x0 (nk, ng0, nao) and F (nk, m, nao), random at the plan's k and NaN elsewhere; pivots with
    repeats and both boundary rows; y of the gathered rows X = x0[:, piv]."""
    rng = np.random.default_rng(9000 * nk_of(kmesh) + nip + m + nao + ng0)
    p, nk = partner(kmesh), nk_of(kmesh)
    ks = set(reps(kmesh))
    x0, F = rnd(rng, nk, ng0, nao), rnd(rng, nk, m, nao)
    piv = rng.integers(0, ng0, nip).astype(np.int32)
    piv[[0, 1, nip // 2, nip - 1]] = [ng0 - 1, 0, 0, ng0 - 1]
    fullX, fullF = x0[:, piv], F.copy()
    for k in range(nk):
        if k not in ks:
            fullX[k], fullF[k] = x0[p[k]][piv].conj(), F[p[k]].conj()
            x0[k], F[k] = np.nan, np.nan
    ref = y_ref(fx_ref(fullX, fullF).reshape(nk, nip * m), kmesh)[0]
    r64 = y_ref(fx_ref(fullX, fullF, wide=False).reshape(nk, nip * m), kmesh, wide=False)[0]
    return StreamData(x0, piv, F, ref.reshape(nk, nip, m), rel_err(r64, ref), max(nao, nk))
