"""Cases and references for the layer that composes the factors into J, K and (ij|kl):
fisdf_get_j_rows / fisdf_get_j_band_rows, fisdf_get_k_rows / fisdf_get_k_rows_local, their
[0, nip) wrappers, fisdf_get_eri and the small kernels under them (rho_diag_kernel,
scale_rows_kernel, pair_product_kernel).  No tests and no GPU here: tests/test_jk_cases.py checks
this file on the CPU, tests/test_gpu_jk_variants.py runs the device against it.

Two layers, as in tests/kmesh_cases.py:
  * the contracts of include/fisdf.h and fftisdf.py:133-228 in np.clongdouble (64-bit mantissa),
    Phi from integers through kmesh_cases.mesh_dft: the references;
  * the same quantities in plain complex128 in the order the device takes (j64, k64, eri64).
    They only measure what float64 arithmetic costs against the reference, and they take a
    `fault` so that tests/test_jk_cases.py can show which subtle mistakes the bounds see.

Bound, per output block (set, k): a device block may be max(16 err64, n eps scale) from the
reference in max-norm, err64 the float64 restatement's own distance from the reference on that
block, scale the largest |ref| of the block, n the longest chain of sums that feeds an entry
(j_chain, k_chain, eri_chain).  An all-zero block (an empty row range) has the bound 0: exact
zeros.  The monitor max |Im rho_s| is compared relative to the largest |rho_s|.

Inputs: entries N(0,1) + i N(0,1).  symmetric: X[-k] = conj(X[k]), D[-k] = conj(D[k]), D[k]
Hermitian, so rho_s is real and the monitor a rounding residue; generic: nothing symmetric, D not
Hermitian, so the Re(.) of the contract and the monitor carry information.  Set x of a density
matrix is scaled by SET_SCALES[x]: a set leaking into another shows against the per-block bound.
"""
import functools
import math
from collections import namedtuple

import numpy as np

from factor_cases import BOUND_FACTOR, CLD, EPS, LD
from fft_cases import rnd
from kmesh_cases import (LATTICE, REG_MESHES, mesh_dft, nk_of, partner,  # noqa: F401
                         tr_symmetric)

SET_SCALES = (1.0, 1e3, 1e-3)


def _dt(wide):
    return CLD if wide else np.complex128


def _H(a):
    return a.conj().swapaxes(-1, -2)


# ---- inputs --------------------------------------------------------------------------------------
def make_x(rng, kmesh, nip, nao, sym):
    return tr_symmetric(rng, kmesh, nip, nao) if sym else rnd(rng, nk_of(kmesh), nip, nao)


def make_dm(rng, kmesh, nset, nao, sym):
    """(nset, nk, nao, nao), set x times SET_SCALES[x].  sym: D[k] Hermitian and D[-k] = conj(D[k])
    (real symmetric at a self-conjugate k)."""
    nk = nk_of(kmesh)
    D = rnd(rng, nset, nk, nao, nao)
    if sym:
        D = (D + _H(D)) / 2
        p = partner(kmesh)
        for k in range(nk):
            if p[k] == k:
                D[:, k] = D[:, k].real
            elif p[k] < k:
                D[:, k] = D[:, p[k]].conj()
    for x in range(nset):
        D[x] *= SET_SCALES[x]
    return D


# ---- row blocks ------------------------------------------------------------------------------------
def row_blocks(nip):
    """[0, nip), the first row, the last row, [37, 70) where it fits, an empty block inside."""
    out = [(0, nip), (0, 1), (nip - 1, nip)]
    if nip >= 70:
        out.append((37, 70))
    out.append((nip // 2, nip // 2))
    return list(dict.fromkeys(out))


def partition(nip):
    """four consecutive blocks that cover [0, nip) (some empty below nip = 4)."""
    cuts = [0, nip // 4, nip // 2, (3 * nip) // 4, nip]
    return list(zip(cuts[:-1], cuts[1:]))


# ---- bounds ----------------------------------------------------------------------------------------
def block_err(got, ref):
    """max |got - ref| over the last two axes, in long double."""
    d = np.abs(np.asarray(got).astype(CLD) - np.asarray(ref).astype(CLD))
    return d.reshape(d.shape[:-2] + (-1,)).max(axis=-1).astype(float) if d.size else \
        np.zeros(d.shape[:-2])


def block_scale(ref):
    a = np.abs(np.asarray(ref))
    return a.reshape(a.shape[:-2] + (-1,)).max(axis=-1).astype(float) if a.size else \
        np.zeros(a.shape[:-2])


def block_bound(r64, ref, n):
    """max(16 err64, n eps scale) per block of the last two axes."""
    return np.maximum(BOUND_FACTOR * block_err(r64, ref), n * EPS * block_scale(ref))


def worst_ratio(err, tol):
    """largest err / tol over the blocks; a block with tol = 0 must have err = 0 (inf if not)."""
    err, tol = np.atleast_1d(err), np.atleast_1d(tol)
    if err.size == 0:
        return 0.0
    r = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def j_chain(nk, nao, nip, nb):
    return nk * nao + nip + nb


def k_chain(nk, nao, nip, nb):
    return 2 * nao + 2 * nk + nip + nb


def eri_chain(nao, nip):
    return nao + 2 * nip


# ---- J ---------------------------------------------------------------------------------------------
def j_rho(X, D, wide=True, fault=None):
    """rho[x, I] = (1/nk) sum_{k,m,n} X_k[I,m] D[x,k,m,n] conj(X_k[I,n])."""
    X, D = np.asarray(X).astype(_dt(wide)), np.asarray(D).astype(_dt(wide))
    nk, nip, nao = X.shape
    T = X[None] @ D                                           # (nset, nk, nip, nao)
    prod = T * (X if fault == "rho_conj_dropped" else X.conj())[None]
    prod = prod.transpose(0, 2, 1, 3).reshape(D.shape[0], nip, nk * nao)   # t = k nao + n
    if fault == "rho_lanes_from_64_skipped":
        prod = prod[:, :, :64]
    rho = prod.sum(axis=-1)
    return rho if fault == "rho_without_1_over_nk" else rho / nk


def j_rows(X, W0, D, i0, i1, Xb=None, wide=True, fault=None):
    """J[x, k] = X_k[i0:i1]^H diag(v[x]) X_k[i0:i1], v = W0[i0:i1] rho; with Xb (nkb, nip, nao)
    the last step takes Xb in place of X (band k-points)."""
    dt = _dt(wide)
    rho = j_rho(X, D, wide, fault)
    v = rho @ np.asarray(W0).astype(dt)[i0:i1].T              # (nset, nb)
    if fault == "v_of_another_set":
        v = np.roll(v, 1, axis=0)
    Xo = np.asarray(X if Xb is None else Xb).astype(dt)
    Xo = Xo[:, i0 + 1:i1 + 1] if fault == "row_offset_off_by_one" else Xo[:, i0:i1]
    return _H(Xo)[None] @ (v[:, None, :, None] * Xo[None])


# ---- K ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_phase64(kmesh):
    """Phi[R, q] = exp(i T_R . k_q) / sqrt(nk) in float64 as the library's get_phase forms it on the
    host for the dense pair: b = 2 pi inv(a)^T from the cofactors over the determinant, k_q =
    (i / n) . b, T_R = r . a, the angle as a three-term dot product, LATTICE for a.  It is within 2
    eps of the exact Phi, which a block of K that the transform back cancels to a tenth of its
    terms feels (K_CASES' (3,2,1) nip = 1 case)."""
    A = [[float(v) for v in row] for row in LATTICE]
    cof = [[A[1][1] * A[2][2] - A[1][2] * A[2][1], A[0][2] * A[2][1] - A[0][1] * A[2][2],
            A[0][1] * A[1][2] - A[0][2] * A[1][1]],
           [A[1][2] * A[2][0] - A[1][0] * A[2][2], A[0][0] * A[2][2] - A[0][2] * A[2][0],
            A[0][2] * A[1][0] - A[0][0] * A[1][2]],
           [A[1][0] * A[2][1] - A[1][1] * A[2][0], A[0][1] * A[2][0] - A[0][0] * A[2][1],
            A[0][0] * A[1][1] - A[0][1] * A[1][0]]]
    det = A[0][0] * cof[0][0] - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) \
        + A[0][2] * cof[2][0]
    b = [[6.283185307179586 * (cof[j][i] / det) for j in range(3)] for i in range(3)]
    nk = nk_of(kmesh)
    idx = [divmod(q // kmesh[2], kmesh[1]) + (q % kmesh[2],) for q in range(nk)]
    s = math.sqrt(float(nk))
    phi = np.empty((nk, nk), complex)
    for R, r in enumerate(idx):
        T = [r[0] * A[0][c] + r[1] * A[1][c] + r[2] * A[2][c] for c in range(3)]
        for q, i in enumerate(idx):
            f = [i[0] / kmesh[0], i[1] / kmesh[1], i[2] / kmesh[2]]
            k = [f[0] * b[0][c] + f[1] * b[1][c] + f[2] * b[2][c] for c in range(3)]
            th = T[0] * k[0] + T[1] * k[1] + T[2] * k[2]
            phi[R, q] = complex(math.cos(th) / s, math.sin(th) / s)
    return phi


def _phi_apply(a, kmesh, wide, dense, transpose=False, fault=None):
    """Phi (or Phi^T) along the first axis: the separable mesh DFT, or (dense, float64 only) the
    product with device_phase64, the Phi of the dense device path.  On a k-mesh
    Phi[R, k] = Phi[k, R], so `transpose` changes nothing but the dense product's operand."""
    if fault == "phi_conj_for_phi_T":
        return _phi_apply(a.conj(), kmesh, wide, dense, transpose).conj()
    if not dense:
        return mesh_dft(a, kmesh, wide)
    phi = device_phase64(tuple(kmesh))
    return ((phi.T if transpose else phi) @ a.reshape(a.shape[0], -1)).reshape(a.shape)


def k_rows(X, Ws, D, kmesh, i0, i1, wide=True):
    """(K, max |Im rho_s|, max |rho_s|) of the row block [i0, i1), from the contract:
    rho_k = X_k D_k X_k^H / nk; rho_s = Phi rho_k; V_s[R,I,J] = W_s[R,I,J] Re(rho_s[R,J,I]) for I
    in the block; V_k = Phi^T V_s; K[x,k] = X_k[i0:i1]^H V_k X_k.  The two maxima run over the
    entries rho_s[R, J, I], I in the block, that enter V_s, all sets together."""
    dt = _dt(wide)
    X, D = np.asarray(X).astype(dt), np.asarray(D).astype(dt)
    nk = X.shape[0]
    Xb = X[:, i0:i1]
    rk = ((X[None] @ D) @ _H(Xb)[None]) / (LD(nk) if wide else float(nk))   # [x,k,J,I]
    rs = mesh_dft(rk.swapaxes(0, 1), kmesh, wide)                            # [R,x,J,I]
    mon = float(np.abs(rs.imag).max()) if rs.size else 0.0
    scale = float(np.abs(rs).max()) if rs.size else 0.0
    w = np.asarray(Ws).astype(LD if wide else np.float64)[:, None, i0:i1, :]
    vk = mesh_dft(w * rs.real.swapaxes(-1, -2), kmesh, wide)                 # [k,x,I,J]
    K = _H(Xb)[None] @ (vk.swapaxes(0, 1) @ X[None])
    return K, mon, scale


def k64(X, Ws, D, kmesh, i0, i1, dense=False, fault=None):
    """the same in complex128 in the device's order: T = conj(X_k[i0:i1]) D_k^T / nk, rho_k^T =
    T X_k^T, the pair, V_k X_k, then X_k[i0:i1]^H (.).  dense: Phi from the lattice."""
    X, D = np.asarray(X, complex), np.asarray(D, complex)
    nk = X.shape[0]
    Xb = X[:, i0 + 1:i1 + 1] if fault == "row_offset_off_by_one" else X[:, i0:i1]
    if fault == "rho_s_not_transposed":
        B1 = (((Xb[None] @ D) * (1.0 / nk)) @ _H(X)[None])                  # rho_k[I, J]
    else:
        B1 = ((Xb.conj()[None] @ D.swapaxes(-1, -2)) * (1.0 / nk)) @ X.swapaxes(-1, -2)[None]
    rs = _phi_apply(B1.swapaxes(0, 1), kmesh, False, dense)                  # [R,x,I,J]
    mon = float(np.abs(rs.imag).max()) if rs.size else 0.0
    w = np.asarray(Ws, float)
    if fault == "w_s_of_the_next_R":
        w = np.roll(w, -1, axis=0)
    vs = w[:, None, i0:i1, :] * rs.real
    vk = _phi_apply(vs.astype(complex), kmesh, False, dense, transpose=True,
                    fault=fault if fault == "phi_conj_for_phi_T" else None)
    return _H(X[:, i0:i1])[None] @ (vk.swapaxes(0, 1) @ X[None]), mon


def ws_from_wq(Wq, kmesh, wide=True):
    """W_s = sqrt(nk) Re(Phi W_q) (fftisdf.py:204-207)."""
    nk = nk_of(kmesh)
    ws = mesh_dft(np.asarray(Wq), kmesh, wide).real
    return ws * (np.sqrt(LD(nk)) if wide else np.sqrt(float(nk)))


# ---- ERI -------------------------------------------------------------------------------------------
def eri(X, kidx, Wq, Cs=None, wide=True, fault=None):
    """eri[i n2 + j][k n4 + l] = sum_IJ W_q[I,J] conj(A1[I,i]) A2[I,j] conj(A3[J,k]) A4[J,l],
    A_s = X[kidx[s]] C_s, C_s = 1 where Cs is None or Cs[s] is None."""
    dt = _dt(wide)
    X = np.asarray(X).astype(dt)
    A = [X[kidx[s]] if Cs is None or Cs[s] is None else X[kidx[s]] @ np.asarray(Cs[s]).astype(dt)
         for s in range(4)]
    nip = X.shape[1]
    if fault == "conj_on_the_wrong_pair_factor":
        P12 = (A[0][:, :, None] * A[1].conj()[:, None, :]).reshape(nip, -1)
    else:
        P12 = (A[0].conj()[:, :, None] * A[1][:, None, :]).reshape(nip, -1)
    P34 = (A[2].conj()[:, :, None] * A[3][:, None, :]).reshape(nip, -1)
    return P12.T @ (np.asarray(Wq).astype(dt) @ P34)


# ---- the case tables -------------------------------------------------------------------------------
JCase = namedtuple("JCase", "kmesh nao nip nset sym nkb")
J_MESH_NAO = [((1, 1, 1), 5), ((1, 1, 1), 63), ((1, 1, 1), 64), ((1, 1, 1), 65),
              ((2, 2, 2), 8), ((2, 2, 2), 13), ((3, 3, 3), 5)]
J_NIP = (1, 37, 64, 70, 130)
J_CASES = [JCase(km, nao, nip, (1, 3)[(i + j) % 2], (i + j // 2) % 2, 0)
           for i, (km, nao) in enumerate(J_MESH_NAO) for j, nip in enumerate(J_NIP)]
# the band form: nkb below and above nk = 8, and nk = 27; Xb is unrelated to X
J_BAND_CASES = [JCase((2, 2, 2), 8, 37, 3, 0, 1), JCase((2, 2, 2), 13, 70, 1, 1, 3),
                JCase((2, 2, 2), 8, 70, 3, 1, 11), JCase((3, 3, 3), 5, 37, 1, 0, 3)]

KCase = namedtuple("KCase", "kmesh nip nao nset sym kdft")     # kdft: FISDF_K_DFT, None = unset
K_SHAPES = [(1, 3), (37, 5), (70, 13), (130, 8)]
K_REG = [(1, 1, 2), (2, 2, 2), (3, 3, 1), (3, 3, 3), (4, 4, 4)]
K_NO_REG = [(3, 2, 1), (1, 1, 3)]
K_CASES = (
    # Gamma: EPI_WSRHO inside the X GEMM, every shape, both kinds
    [KCase((1, 1, 1), nip, nao, 1 + i % 2, (i + 1) % 2, None) for i, (nip, nao) in enumerate(K_SHAPES)]
    + [KCase((1, 1, 1), 37, 5, 2, 1, None), KCase((1, 1, 1), 9, 3, 1, 0, "0")]
    # the register kernels and, on the same inputs, the dense pair
    + [KCase(km, 9, 3, 1 + i % 2, i % 2, kd) for i, km in enumerate(K_REG) for kd in (None, "0")]
    + [KCase((2, 2, 2), 37, 5, 2, 0, kd) for kd in (None, "0")]
    + [KCase((2, 2, 2), 70, 13, 1, 1, kd) for kd in (None, "0")]
    + [KCase((3, 3, 1), 130, 8, 2, 1, None), KCase((1, 1, 2), 1, 3, 2, 0, None)]
    # no register kernel: the dense pair by default
    + [KCase(km, 9, 3, 2 - i % 2, i % 2, None) for i, km in enumerate(K_NO_REG)]
    + [KCase((3, 2, 1), 37, 5, 1, 0, None), KCase((1, 1, 3), 130, 8, 2, 1, None),
       KCase((1, 1, 3), 70, 13, 1, 0, None), KCase((3, 2, 1), 1, 3, 2, 1, None)])

ECase = namedtuple("ECase", "nip nao equal_k cs")
E_NK = 5
E_KIDX = {0: (3, 0, 4, 1), 1: (2, 2, 2, 2)}
E_WIDTHS = {"none": (None, None, None, None), "all": (3, 4, 2, 5), "1_and_3": (None, 4, None, 5),
            "nmo_1": (1, 1, 1, 1)}
E_CASES = [ECase(nip, nao, eq, cs) for nip in (37, 130) for nao in (5, 13) for eq in (0, 1)
           for cs in E_WIDTHS]


def case_id(c):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c)


def k_route(c):
    """what get_k_block does between its GEMMs: "gamma" (nk = 1, the epilogue of the X GEMM),
    "register" (a listed k-mesh, FISDF_K_DFT not 0) or "dense" (two Phi GEMMs)."""
    if nk_of(c.kmesh) == 1:
        return "gamma"
    return "register" if tuple(c.kmesh) in REG_MESHES and c.kdft != "0" else "dense"


# ---- what a case reaches ---------------------------------------------------------------------------
def j_reaches(c):
    nk, t = nk_of(c.kmesh), nk_of(c.kmesh) * c.nao
    out = {"rho_lanes_below_64" if t < 64 else "rho_lanes_exactly_64" if t == 64
           else "rho_lanes_partial_last_pass",
           "v_gemm_batch_%d" % c.nset, "sym" if c.sym else "generic", "empty_block"}
    if c.nip > 1:
        out.add("sub_block_operand_view")
    if c.nip == 1:
        out.add("nip_1")
    if c.nkb:
        out.add("band_nkb_below_nk" if c.nkb < nk else "band_nkb_above_nk")
    return out


J_BRANCHES = {"rho_lanes_below_64", "rho_lanes_exactly_64", "rho_lanes_partial_last_pass", "v_gemm_batch_1", "v_gemm_batch_3", "sym", "generic",
              "empty_block", "sub_block_operand_view", "nip_1", "band_nkb_below_nk",
              "band_nkb_above_nk"}


def k_reaches(c):
    out = {k_route(c), "sets_%d" % c.nset, "sym" if c.sym else "generic", "empty_block",
           "compact_w_s_rows", "w_s_rows_inside_nan"}
    if k_route(c) == "register":
        out.add("register_%dx%dx%d" % tuple(c.kmesh))
    if k_route(c) == "dense":
        out.add("dense_forced" if tuple(c.kmesh) in REG_MESHES else "dense_no_register_kernel")
    if c.nip > 1:
        out.add("sub_block_operand_view")
    for i0, i1 in row_blocks(c.nip) + partition(c.nip):
        n = (i1 - i0) * c.nip
        if 0 < n < 64:
            out.add("columns_below_64")
        if n > 64 and n % 64:
            out.add("columns_not_a_multiple_of_64")
    return out


K_BRANCHES = {"gamma", "register", "dense", "dense_forced", "dense_no_register_kernel", "sets_1",
              "sets_2", "sym", "generic", "empty_block", "compact_w_s_rows", "w_s_rows_inside_nan",
              "sub_block_operand_view", "columns_below_64", "columns_not_a_multiple_of_64"}
K_BRANCHES |= {"register_%dx%dx%d" % km for km in K_REG}


def e_reaches(c):
    return {"equal_k" if c.equal_k else "distinct_k",
            {"none": "ao", "all": "every_c", "1_and_3": "some_c", "nmo_1": "nmo_1"}[c.cs],
            "nip_%d" % c.nip, "nao_%d" % c.nao}


E_BRANCHES = {"equal_k", "distinct_k", "ao", "every_c", "some_c", "nmo_1", "nip_37", "nip_130",
              "nao_5", "nao_13"}


# ---- inputs and references of the device cases (computed once, shared) ---------------------------
JData = namedtuple("JData", "X W0 D Xb")


@functools.lru_cache(maxsize=None)
def j_data(c):
    rng = np.random.default_rng(100000 * nk_of(c.kmesh) + 1000 * c.nao + 7 * c.nip + c.nset
                                + 3 * c.nkb)
    X = make_x(rng, c.kmesh, c.nip, c.nao, c.sym)
    W0 = rnd(rng, c.nip, c.nip)
    D = make_dm(rng, c.kmesh, c.nset, c.nao, c.sym)
    Xb = rnd(rng, c.nkb, c.nip, c.nao) if c.nkb else None
    return JData(X, W0, D, Xb)


@functools.lru_cache(maxsize=None)
def _j_rho_cached(c, wide):
    d = j_data(c)
    return j_rho(d.X, d.D, wide)


def _j_from_rho(c, i0, i1, wide):
    d, dt = j_data(c), _dt(wide)
    v = _j_rho_cached(c, wide) @ d.W0.astype(dt)[i0:i1].T
    Xo = (d.X if d.Xb is None else d.Xb).astype(dt)[:, i0:i1]
    return _H(Xo)[None] @ (v[:, None, :, None] * Xo[None])


@functools.lru_cache(maxsize=None)
def j_expect(c, i0, i1):
    """(reference, bound per (set, k)) of the row block."""
    ref = _j_from_rho(c, i0, i1, True)
    r64 = _j_from_rho(c, i0, i1, False)
    return ref, block_bound(r64, ref, j_chain(nk_of(c.kmesh), c.nao, c.nip, i1 - i0))


KData = namedtuple("KData", "X Ws D")


@functools.lru_cache(maxsize=None)
def k_data(c):
    """the inputs do not depend on kdft: the register and the dense run see the same numbers."""
    rng = np.random.default_rng(300000 * nk_of(c.kmesh) + 1000 * c.nao + 7 * c.nip + c.nset
                                + 11 * c.kmesh[0])
    X = make_x(rng, c.kmesh, c.nip, c.nao, c.sym)
    Ws = rng.standard_normal((nk_of(c.kmesh), c.nip, c.nip))
    D = make_dm(rng, c.kmesh, c.nset, c.nao, c.sym)
    return KData(X, Ws, D)


KExpect = namedtuple("KExpect", "ref tol mon scale mon_tol")


@functools.lru_cache(maxsize=None)
def k_expect(c, i0, i1):
    """reference, bound per (set, k), the monitor, the size of rho_s and the monitor's bound
    (relative to that size).  The dense route is measured against the dense restatement."""
    d, nk = k_data(c), nk_of(c.kmesh)
    ref, mon, scale = k_rows(d.X, d.Ws, d.D, c.kmesh, i0, i1)
    r64, m64 = k64(d.X, d.Ws, d.D, c.kmesh, i0, i1, dense=k_route(c) == "dense")
    n = k_chain(nk, c.nao, c.nip, i1 - i0)
    mon_tol = max(BOUND_FACTOR * abs(m64 - mon) / scale, n * EPS) if scale > 0 else 0.0
    return KExpect(ref, block_bound(r64, ref, n), mon, scale, mon_tol)


EData = namedtuple("EData", "X W Cs kidx ref tol")


@functools.lru_cache(maxsize=None)
def e_data(c):
    rng = np.random.default_rng(7000 * c.nip + 100 * c.nao + 10 * c.equal_k + len(c.cs))
    X = rnd(rng, E_NK, c.nip, c.nao)
    W = rnd(rng, c.nip, c.nip)                       # generic, not Hermitian
    Cs = [None if n is None else rnd(rng, c.nao, n) for n in E_WIDTHS[c.cs]]
    kidx = E_KIDX[c.equal_k]
    ref = eri(X, kidx, W, Cs)
    r64 = eri(X, kidx, W, Cs, wide=False)
    return EData(X, W, Cs, kidx, ref, float(block_bound(r64, ref, eri_chain(c.nao, c.nip))))
