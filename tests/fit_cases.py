"""Cases, restated rules and references for the Coulomb fit: the calls that turn x4_q and y_q into
W_q (fisdf_factor_x4_qs + fisdf_fit_coulomb_qs) and W_q into W_s (fisdf_build_ws_qs / _rows /
_blocks).  No GPU here; test_fit_cases.py checks this file on the CPU and test_gpu_fit.py runs the
device against it.

Three layers, as in factor_cases.py:
  * the host-side rules of the fit restated (self-conjugacy of q and its m = 2 k_q, the half grid's
    prefix planes, the weight-asymmetric lists and their factors, lanes and ring depth, the
    W_PP-in-the-lane and W_PP split predicates), compared with fisdf_fit_plan on the CPU and with
    fisdf_fit_info / fisdf_fit_report on the device;
  * references in long double: W_q = S Zhat diag(c) Zhat^H S^H vol / N^2 with Zhat the long-double
    DFT of y_q times exp(-i k_q r), c the float64 get_coulG of oracle/isdf_ref.py (its box-edge
    rounding is the specification, so c enters as the float64 numbers it returns) and S the
    inverse, the pseudo-inverse or the basic solution operator of x4_q; W_s from long-double
    sin / cos;
  * the same chain in float64 (NumPy FFT, trsm_blocked_f64, float64 Gram), used only to measure
    what float64 alone costs against the long-double reference: a device result may be
    BOUND_FACTOR times that far away, never less than n eps with n the longest sum of the chain
    (ngrid for W_q, nq for W_s).  No bound is a number fixed in advance.

Inputs: x4_q = Q diag(lambda) Q^H with lambda in [1, 4] (real symmetric for a self-conjugate q),
or B B^H of rank r with the same spectrum plus Hermitian noise of 1e-13 (the rank cut is 1e-8);
y_q Gaussian, real for a self-conjugate q (z_q real is what makes Zhat(G') = conj(Zhat(G)),
G' = -G - 2 k_q, the premise of the real and half-grid paths).
"""
import functools
from collections import namedtuple

import numpy as np

import factor_cases as F
import fft_cases as FF
from jfft_cases import LATTICE
from oracle import isdf_ref as R

LD, CLD, EPS = F.LD, F.CLD, F.EPS
PI = FF.PI
TOY_LATTICE = (np.ones((3, 3)) - np.eye(3)) * 2.2          # fisdf.cell.toy_cell's fcc lattice
FIT_TOL = 1e-8                 # relative rank cut given to fisdf_factor_x4_qs
NOISE = 1e-13                  # Hermitian noise of a rank-deficient x4_q (1e5 below the cut)
IMAG_JUNK = 1e-3               # imaginary part added to a self-conjugate x4_q (stage_x4 drops it)
ASYM_CUT = 1e-13               # the library's relative cut between the weights of a pair
LSTSQ, SVD, BASIC = 0, 1, 2    # FISDF_FIT_*
LANE_WPP_MIN_Q = 12
WPP_SPLIT_NIP = 256
WPP_KSPLIT_DEFAULT = 4


# ------------------------------------------------------------------ restated rules
def q_index(kmesh, q):
    return (q // (kmesh[1] * kmesh[2]), (q // kmesh[2]) % kmesh[1], q % kmesh[2])


def self_conjugate(kmesh, q):
    """2 k_q is a reciprocal-lattice vector."""
    return all((2 * i) % n == 0 for i, n in zip(q_index(kmesh, q), kmesh))


def self_m(kmesh, q):
    """m with 2 k_q = m . b of a self-conjugate q."""
    assert self_conjugate(kmesh, q)
    return tuple(2 * i // n for i, n in zip(q_index(kmesh, q), kmesh))


def partner_q(kmesh, q):
    i = [(-j) % n for j, n in zip(q_index(kmesh, q), kmesh)]
    return (i[0] * kmesh[1] + i[1]) * kmesh[2] + i[2]


def prefix_planes(mesh, m0):
    return FF.half_prefix_planes(mesh[0], m0)


def fitted_columns(mesh, kmesh, q, half):
    if not half:
        return int(np.prod(mesh))
    return prefix_planes(mesh, self_m(kmesh, q)[0]) * mesh[1] * mesh[2]


def partner_index(mesh, m):
    """Flat index of G' = -G - m for every flat index of G, and the axis-0 index pair."""
    i = np.indices(mesh).reshape(3, -1)
    p = [(-i[d] - m[d]) % mesh[d] for d in range(3)]
    return (p[0] * mesh[1] + p[1]) * mesh[2] + p[2], i[0], p[0]


def wscale(a, mesh):
    return abs(np.linalg.det(a)) / float(np.prod(mesh)) ** 2


def coulg(a, kmesh, mesh, q, omega):
    return R.get_coulG(a, R.get_kpts(a, kmesh)[q], mesh, omega=omega)


def _differs(x, xp):
    return np.abs(x - xp) > ASYM_CUT * np.maximum(np.abs(x), np.abs(xp))


def asym_full(c, a, mesh, m):
    """asym_list_kernel: the G (ascending) whose sqrt weight differs from its partner's; the full
    grid's list is taken from the square-rooted weight the FFT applies."""
    w = np.sqrt(c * wscale(a, mesh))
    pe, _, _ = partner_index(mesh, m)
    return np.nonzero(_differs(w, w[pe]))[0]


def asym_half(c, a, mesh, m):
    """asym_half_kernel: the prefix G whose pair has unequal weights, and the factor of Im:
    (c - c') / (c + c') on a strict plane, 1 on a self-paired plane (both members listed)."""
    cs = c * wscale(a, mesh)
    pe, i0, p0 = partner_index(mesh, m)
    flag = _differs(cs, cs[pe]) & (i0 < prefix_planes(mesh, m[0]))
    idx = np.nonzero(flag)[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(p0[idx] != i0[idx], (cs[idx] - cs[pe][idx]) / (cs[idx] + cs[pe][idx]), 1.0)
    return idx, f


def half_weight(c, a, mesh, m):
    """half_weight_kernel without the square root: c + c' on a strict prefix plane, c on a
    self-paired plane, 0 beyond the prefix."""
    cs = c * wscale(a, mesh)
    pe, i0, p0 = partner_index(mesh, m)
    return np.where(i0 < prefix_planes(mesh, m[0]), np.where(p0 == i0, cs, cs + cs[pe]), 0.0)


def fit_lanes(nq, lanes, pipe_mode, depth, ready=False):
    """(lanes, ring depth) of a call: what fisdf_fit_info reports.  lanes / depth 0 and pipe_mode
    -1 are the defaults with an empty environment (2 lanes, pipe on, depth lanes + 2)."""
    nl = min(nq, lanes if lanes > 0 else 2)
    pipe = pipe_mode != 0 and nq > 1 and nl > 1
    if pipe:
        nl = min(nl, 2 if ready else 3)
    if ready:
        nl = min(nl, 3)
    return nl, (min(nq, depth if depth > 0 else nl + 2) if pipe else 0)


def min_norm_slot(rank, nip, mode):
    return rank > 0 and (mode == SVD or (mode == LSTSQ and rank < nip))


def lane_wpp(nq, ranks, nip, mode):
    return (nq >= LANE_WPP_MIN_Q and all(r == nip for r in ranks)
            and not any(min_norm_slot(r, nip, mode) for r in ranks))


def wpp_split(nip, env=WPP_KSPLIT_DEFAULT):
    return min(env, 16) if nip >= WPP_SPLIT_NIP and env > 1 else 1


# what fisdf_fit_report returns
Report = namedtuple("Report", "rank real half herm ncol nasym solve min_norm lane wpp split ysrc")
SOLVE_LINV, SOLVE_MIN_NORM, SOLVE_BLOCKED, SOLVE_NONE = 0, 1, 2, -1
WPP_TAIL_GEMM, WPP_LANE, WPP_TAIL_TRSM = 0, 1, 2
Y_CONTIG, Y_SLICES, Y_UNPACKED = 0, 1, 2


def predict_report(case, j, ranks, real_on, half_on, lanes, mode=LSTSQ, ysrc=Y_CONTIG,
                   ksplit_env=WPP_KSPLIT_DEFAULT, omega=None):
    """The report of the j-th q of a call over case.qs whose ranks are `ranks`, on `lanes` lanes
    (omega None: the case's)."""
    q, nip, mesh, kmesh = case.qs[j], case.nip, case.mesh, case.kmesh
    r = ranks[j]
    real = bool(real_on and self_conjugate(kmesh, q))
    half = real and bool(half_on)
    m = self_m(kmesh, q) if real else None
    herm = half and r > 0 and FF.route(mesh, m) == FF.REG_HERM
    nasym = 0
    if real and r > 0:
        c = coulg(case.a, kmesh, mesh, q, case.omega if omega is None else omega)
        nasym = len(asym_half(c, case.a, mesh, m)[0] if half else asym_full(c, case.a, mesh, m))
    cod = min_norm_slot(r, nip, mode)
    solve = SOLVE_NONE if r == 0 else SOLVE_MIN_NORM if cod else SOLVE_LINV if r == nip \
        else SOLVE_BLOCKED
    in_lane = lane_wpp(len(ranks), ranks, nip, mode)
    wpp = WPP_LANE if in_lane else WPP_TAIL_GEMM if all(x == nip for x in ranks) else WPP_TAIL_TRSM
    split = wpp_split(nip, ksplit_env) if wpp != WPP_TAIL_TRSM else 1
    return Report(r, int(real), int(half), int(herm), fitted_columns(mesh, kmesh, q, half), nasym,
                  solve, int(cod), j % lanes, wpp, split, ysrc)


# ------------------------------------------------------------------ inputs
def _gauss(rng, n, k, real):
    g = rng.standard_normal((n, k))
    return g.astype(np.complex128) if real else g + 1j * rng.standard_normal((n, k))


def make_x4(n, seed, real, rank=None):
    """Q diag(lambda) Q^H, lambda in [1, 4] with both ends present; rank given: only the first
    `rank` eigenpairs, plus Hermitian noise NOISE (real symmetric when `real`)."""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(_gauss(rng, n, n, real))[0]
    k = n if rank is None else rank
    lam = 1.0 + 3.0 * rng.random(k)
    lam[0], lam[-1] = 1.0, 4.0
    A = (Q[:, :k] * lam) @ Q[:, :k].conj().T
    if rank is not None:
        A = A + NOISE * _gauss(rng, n, n, real)
    A = F._herm(A)
    return A.real.astype(np.complex128) if real else A


def imag_junk(n, seed):
    """i K with K real antisymmetric: a Hermitian imaginary part that a self-conjugate x4_q
    cannot have, which the factor stage must drop."""
    k = np.random.default_rng(seed).standard_normal((n, n))
    return 1j * IMAG_JUNK * (k - k.T)


# ------------------------------------------------------------------ the case table
# qs: the fitted q-list (ascending); asym_q / empty_q: the self-conjugate q whose weight-asymmetric
# list must be non-empty / empty (on the full grid and on the half grid alike); ranks: None = every
# q full rank, else per q None (full), 0 (x4_q = 0) or r
FitCase = namedtuple("FitCase", "name a mesh kmesh qs nip omega asym_q empty_q ranks note")


def _case(name, mesh, kmesh, nip, omega, asym_q=(), empty_q=(), qs=None, a=LATTICE, ranks=None,
          note=""):
    nk = int(np.prod(kmesh))
    qs = tuple(range(nk)) if qs is None else tuple(qs)
    return FitCase(name, a, tuple(mesh), tuple(kmesh), qs, nip, omega, tuple(asym_q),
                   tuple(empty_q), ranks, note)


ALL8 = tuple(range(8))
CASES = [
    # register FFT, every axis even: the Nyquist planes pair -N/2 with itself, so seven of the
    # eight m have hundreds of asymmetric G and m = (1, 1, 1) has none
    _case("even222_w0_n40", (8, 12, 12), (2, 2, 2), 40, 0.0, asym_q=range(7), empty_q=(7,)),
    _case("even222_wm04_n5", (8, 12, 12), (2, 2, 2), 5, -0.4, asym_q=range(7), empty_q=(7,)),
    # omega > 0 multiplies the weights by exp(-|k+G|^2 / 4 omega^2): the lists are as long, but at
    # +0.4 the Nyquist planes' weights are so small that |Im W| / |W| <= 3e-14 (measured on the CPU,
    # test_fit_cases.test_imaginary_part_per_omega): that case tests the weights only.  At +2.0 the
    # ratio is 4e-5 .. 3e-4, so it carries the asymmetric path like 0 and -0.4
    _case("even222_wp04_n5", (8, 12, 12), (2, 2, 2), 5, 0.4, note="weights only"),
    _case("even222_wp20_n5", (8, 12, 12), (2, 2, 2), 5, 2.0, asym_q=range(7), empty_q=(7,)),
    # odd mesh: every pair has equal weights, the n == 0 branch
    _case("odd222_w0_n70", (13, 15, 15), (2, 2, 2), 70, 0.0, empty_q=ALL8),
    # n0 even, n1 = n2 odd: only m0 = 0 leaves the axis-0 Nyquist plane paired with itself
    _case("mixed222_wm04_n5", (12, 13, 13), (2, 2, 2), 5, -0.4, asym_q=(0, 1, 2, 3),
          empty_q=(4, 5, 6, 7)),
    # LDS plane route (no Hermitian FFT form: every plane is written, the prefix is fitted)
    _case("lds222_w0_n40", (6, 10, 10), (2, 2, 2), 40, 0.0, asym_q=range(7), empty_q=(7,)),
    # axis route, n0 = 2: prefix of 2 planes for m0 = 0, of 1 for m0 = 1
    _case("axes222_w0_n5", (2, 64, 48), (2, 2, 2), 5, 0.0, asym_q=range(7), empty_q=(7,)),
    _case("gamma111_w0_n70", (8, 12, 12), (1, 1, 1), 70, 0.0, asym_q=(0,)),
    # two self-conjugate and four complex q in one call
    _case("k312_wm04_n40", (8, 12, 12), (3, 1, 2), 40, -0.4, asym_q=(0, 1)),
    # q = 2 has m = (1, 0, 0)
    _case("k411_w0_n5", (8, 12, 12), (4, 1, 1), 5, 0.0, asym_q=(0, 2)),
    # 12 q without time reversal: W_PP in the lane
    _case("k322_w0_n40", (8, 12, 12), (3, 2, 2), 40, 0.0, asym_q=(0, 1, 2, 3)),
    # nip = 256: the W_PP split (a self-conjugate and a complex q)
    _case("split311_w0_n256", (8, 12, 12), (3, 1, 1), 256, 0.0, asym_q=(0,), qs=(0, 1)),
    _case("toy222_w0_n5", (8, 12, 12), (2, 2, 2), 5, 0.0, asym_q=range(7), empty_q=(7,),
          a=TOY_LATTICE),
]
# rank-deficient calls (run under every fit mode): a full-rank q, a rank-r q, x4_q = 0
RANK_CASES = [
    _case("rank312_n40", (8, 12, 12), (3, 1, 2), 40, 0.0, qs=(1, 2, 3), ranks=(None, 25, 0)),
    # a self-conjugate rank-deficient q (half grid when on), beside a complex full-rank one
    _case("rank312_self_n70", (8, 12, 12), (3, 1, 2), 70, -0.4, qs=(0, 1, 2), ranks=(0, 33, None)),
]
# six q for the lane / pipe / ring invariances (slots are reused with a ring of 1 and of 2)
INVARIANCE_CASE = "k312_wm04_n40"
BY_NAME = {c.name: c for c in CASES + RANK_CASES}
WS_CASES = [((2, 2, 2), 5), ((3, 1, 2), 7)]            # (kmesh, nip) of the W_s tests


def case_ranks(c):
    return tuple(c.nip if c.ranks is None or c.ranks[j] is None else c.ranks[j]
                 for j in range(len(c.qs)))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(x4 (nq, nip, nip) as the reference reads it, y (nq, nip, ngrid)) of a case; x4_q is exactly
    real for a self-conjugate q."""
    c = BY_NAME[name]
    ngrid = int(np.prod(c.mesh))
    x4, y = [], []
    for j, q in enumerate(c.qs):
        real = self_conjugate(c.kmesh, q)
        seed = 7000 + 131 * len(name) + 17 * q + c.nip
        r = None if c.ranks is None else c.ranks[j]
        x4.append(np.zeros((c.nip, c.nip), complex) if r == 0 else make_x4(c.nip, seed, real, r))
        y.append(_gauss(np.random.default_rng(seed + 1), c.nip, ngrid, real))
    return np.stack(x4), np.stack(y)


def device_x4(name, real_on):
    """x4 as handed to the device: with the real factor on, a self-conjugate q carries an imaginary
    part that the factor stage must drop."""
    c = BY_NAME[name]
    x4 = inputs(name)[0].copy()
    if real_on:
        for j, q in enumerate(c.qs):
            if self_conjugate(c.kmesh, q):
                x4[j] += imag_junk(c.nip, 9000 + q)
    return x4


# ------------------------------------------------------------------ references
def kd_ld(kmesh, q):
    """a . k_q = 2 pi i_d / n_d in long double."""
    return [2 * PI * LD(i) / LD(n) for i, n in zip(q_index(kmesh, q), kmesh)]


def weights_ld(c, a, mesh):
    return c.astype(LD) * LD(abs(np.linalg.det(a))) / LD(int(np.prod(mesh))) ** 2


@functools.lru_cache(maxsize=None)
def zhat_ld(name, j):
    c = BY_NAME[name]
    return FF.ref_fft3d(inputs(name)[1][j], c.mesh, kd=kd_ld(c.kmesh, c.qs[j]))


def gram_of_ld(c, q, Z, omega):
    """Zhat diag(c) Zhat^H vol / N^2 over the whole grid for q of the case's k-mesh."""
    return (Z * weights_ld(coulg(c.a, c.kmesh, c.mesh, q, omega), c.a, c.mesh)) @ Z.conj().T


@functools.lru_cache(maxsize=None)
def gram_ld(name, j, omega=None):
    """The Gram of the j-th q of a case (omega None: the case's)."""
    c = BY_NAME[name]
    return gram_of_ld(c, c.qs[j], zhat_ld(name, j), c.omega if omega is None else omega)


def gram_half_ld(name, j):
    """The same Gram as the half grid forms it: Re over the prefix planes with the pair's combined
    weight, Im from the listed G alone with the signed factor."""
    c = BY_NAME[name]
    q = c.qs[j]
    m = self_m(c.kmesh, q)
    cg = coulg(c.a, c.kmesh, c.mesh, q, c.omega)
    Z = zhat_ld(name, j)
    ncol = fitted_columns(c.mesh, c.kmesh, q, True)
    wh = half_weight(cg, c.a, c.mesh, m).astype(LD)
    re = ((Z[:, :ncol] * wh[:ncol]) @ Z[:, :ncol].conj().T).real
    idx, f = asym_half(cg, c.a, c.mesh, m)
    im = ((Z[:, idx] * (wh[idx] * f.astype(LD))) @ Z[:, idx].conj().T).imag
    out = np.zeros(re.shape, CLD)
    out.real, out.imag = re, im
    return out


def gram_full_listed_ld(name, j):
    """The same Gram as the full grid forms it for a real factor: Re over every G, Im from the
    listed G alone."""
    c = BY_NAME[name]
    q = c.qs[j]
    cg = coulg(c.a, c.kmesh, c.mesh, q, c.omega)
    Z = zhat_ld(name, j)
    idx = asym_full(cg, c.a, c.mesh, self_m(c.kmesh, q))
    w = weights_ld(cg, c.a, c.mesh)
    out = np.zeros((c.nip, c.nip), CLD)
    out.real = gram_ld(name, j).real
    out.imag = ((Z[:, idx] * w[idx]) @ Z[:, idx].conj().T).imag
    return out


def _two_sided(solve, L, G):
    """X^{-1} G X^{-H} for `solve`(L, .) = X^{-1} . and Hermitian G."""
    return solve(L, solve(L, G).conj().T).conj().T


def apply_inverse_ld(x4, G, order=None):
    """x4^{-1} G x4^{-1} through the long-double Cholesky factor."""
    L = F.factor_along_ld(x4, list(range(x4.shape[0])) if order is None else order)
    M = _two_sided(F.solve_lower_ld, L, G)                 # L^-1 G L^-H
    return _two_sided(F.solve_adjoint_ld, L, M)            # L^-H M L^-1


def apply_pinv_ld(fact, G):
    """(A A^H)^+ G (A A^H)^+ with A = P L of the long-double pivoted Cholesky:
    (A A^H)^+ = A (A^H A)^-2 A^H."""
    A = fact.L.astype(CLD)
    K = A.conj().T @ A
    core = apply_inverse_ld(K, apply_inverse_ld(K, A.conj().T @ G @ A))
    return A @ core @ A.conj().T


def apply_basic_ld(fact, G, n):
    """The basic solution on the r pivots: P [(L11 L11^H)^-1 G_PP (L11 L11^H)^-1] P^T."""
    p = fact.piv
    L11 = fact.L[p].astype(CLD)
    M = _two_sided(F.solve_lower_ld, L11, G[np.ix_(p, p)])
    out = np.zeros((n, n), CLD)
    out[np.ix_(p, p)] = _two_sided(F.solve_adjoint_ld, L11, M)
    return out


@functools.lru_cache(maxsize=None)
def pchol_ref(name, j):
    c = BY_NAME[name]
    return F.pchol_ld(inputs(name)[0][j], c.nip, FIT_TOL)


@functools.lru_cache(maxsize=None)
def wq_ld(name, j, mode=LSTSQ, omega=None):
    """The long-double W_q of the j-th q of a case under a fit mode."""
    c = BY_NAME[name]
    x4 = inputs(name)[0][j]
    G = gram_ld(name, j, omega)
    r = case_ranks(c)[j]
    if r == 0:
        return np.zeros((c.nip, c.nip), CLD)
    if r == c.nip:
        return apply_inverse_ld(x4, G)
    fact = pchol_ref(name, j)
    assert fact.rank == r, (name, j, fact.rank, r)
    return apply_basic_ld(fact, G, c.nip) if mode == BASIC else apply_pinv_ld(fact, G)


def phase_f64(mesh, kd):
    th = [-(np.fft.fftfreq(n) * k) for n, k in zip(mesh, kd)]
    return np.exp(1j * (th[0][:, None, None] + th[1][None, :, None] + th[2][None, None, :]))


@functools.lru_cache(maxsize=None)
def wq_f64(name, j, omega=None):
    """The chain in float64 as the device orders it, for a full-rank q: NumPy FFT of y times the
    phase, times sqrt(c vol / N^2); U = L^-1 Yhat by 64-row blocks; G = U U^H; L^-H G L^-1."""
    c = BY_NAME[name]
    x4, y = inputs(name)[0][j], inputs(name)[1][j]
    q = c.qs[j]
    kd = c.a @ R.get_kpts(c.a, c.kmesh)[q]
    cg = coulg(c.a, c.kmesh, c.mesh, q, c.omega if omega is None else omega)
    yh = np.fft.fftn(y.reshape(-1, *c.mesh) * phase_f64(c.mesh, kd), axes=(1, 2, 3))
    yh = yh.reshape(c.nip, -1) * np.sqrt(cg * wscale(c.a, c.mesh))
    L = F.chol_f64(x4)[0]
    return F._chain_w(L, yh, lambda l, x: F.trsm_blocked_f64(l, x, 1),
                      lambda l, x: F.trsm_blocked_f64(l, x, 0), np.complex128)


@functools.lru_cache(maxsize=None)
def wq_bound(name, j=None, omega=None):
    """The bound on max |W - W_ld| / max |W_ld| of a q: 16 times the float64 chain's own error,
    floored at ngrid eps.  A rank-deficient or zero q has no float64 restatement here; it takes the
    largest bound of the case's full-rank q (the same sums at most as long, the same spectrum)."""
    c = BY_NAME[name]
    ngrid = int(np.prod(c.mesh))
    ranks = case_ranks(c)
    if j is None or ranks[j] != c.nip:
        return max(wq_bound(name, i, omega) for i in range(len(c.qs)) if ranks[i] == c.nip)
    return F.bound(F.relerr(wq_f64(name, j, omega), wq_ld(name, j, LSTSQ, omega)), ngrid)


def imag_ratio(name, j):
    """max |Im W_q| / max |W_q| of the reference."""
    W = wq_ld(name, j)
    return float(np.abs(W.imag).max() / np.abs(W).max())


# ------------------------------------------------------------------ W_s
def ws_inputs(kmesh, nip, seed=400):
    nk = int(np.prod(kmesh))
    return _gauss(np.random.default_rng(seed + nk), nk, nip * nip, False).reshape(nk, nip, nip)


def ws_phase_ld(kmesh, qs):
    """exp(i T_R . k_q) (nk, nq) in long double: the angle is 2 pi sum_d r_d i_d / n_d."""
    nk = int(np.prod(kmesh))
    out = np.empty((nk, len(qs)), CLD)
    for Rr in range(nk):
        r = q_index(kmesh, Rr)
        for j, q in enumerate(qs):
            th = 2 * PI * sum(LD((rd * i) % n) / LD(n)
                              for rd, i, n in zip(r, q_index(kmesh, q), kmesh))
            out[Rr, j] = np.cos(th) + CLD(1j) * np.sin(th)
    return out


def ws_ld(Wq, kmesh, qs, wt):
    """W_s[R] = sqrt(nk) Re sum_i wt_i Phi[R, q_i] W_{q_i}, Phi = exp(i T_R . k_q) / sqrt(nk);
    Wq: the (len(qs), nip, nip) slots of the listed q."""
    ph = ws_phase_ld(kmesh, qs) * np.asarray(wt, LD)
    nip = Wq.shape[-1]
    return (ph @ Wq.reshape(len(qs), -1).astype(CLD)).real.reshape(-1, nip, nip)


def ws_f64(Wq, a, kmesh, qs, wt):
    """The library's own order in float64: Phi_sel = wt exp(i T . k) / sqrt(nk), one product,
    real part times sqrt(nk)."""
    nk = int(np.prod(kmesh))
    ph = R.get_phase(a, R.get_kpts(a, kmesh), kmesh)[:, list(qs)] * np.asarray(wt, float)
    nip = Wq.shape[-1]
    return ((ph @ Wq.reshape(len(qs), -1)).real * np.sqrt(nk)).reshape(-1, nip, nip)


def ws_bound(Wq, a, kmesh, qs, wt):
    ref = ws_ld(Wq, kmesh, qs, wt)
    return ref, F.bound(F.relerr(ws_f64(Wq, a, kmesh, qs, wt), ref), max(len(qs), 1))


def tr_reps(kmesh):
    """The time-reversal representatives q <= -q and their weights (2 for a paired one)."""
    nk = int(np.prod(kmesh))
    reps = [q for q in range(nk) if q <= partner_q(kmesh, q)]
    return reps, [1.0 if partner_q(kmesh, q) == q else 2.0 for q in reps]


# ------------------------------------------------------------------ runs and branches
# one device call: the case, real factor / half grid on, lanes, pipe mode and depth as set, the fit
# mode and how y is handed over ("contig", "slices", "ready")
Run = namedtuple("Run", "case real half lanes pipe depth mode y")


def wq_runs():
    """Every case with the real factor on / off and the half grid on / off (without the real
    factor the half-grid switch must change nothing), on the default lanes and pipe."""
    return [Run(c.name, real, half, 0, -1, 0, LSTSQ, "contig")
            for c in CASES for real in (0, 1) for half in (0, 1)]


def invariance_runs():
    n = INVARIANCE_CASE
    nq = len(BY_NAME[n].qs)
    lanes = [Run(n, 1, 1, l, 0, 0, LSTSQ, "contig") for l in (1, 2, 3, 4)]
    pipes = [Run(n, 1, 1, 2, 1, d, LSTSQ, "contig") for d in (1, 2, nq)]
    pipes.append(Run(n, 1, 1, 3, 1, 0, LSTSQ, "contig"))
    return lanes + pipes


def rank_runs():
    return [Run(c.name, 1, half, 0, -1, 0, mode, "contig")
            for c in RANK_CASES for mode in (LSTSQ, SVD, BASIC) for half in (0, 1)]


def y_runs():
    """The default lanes and pipe for every y source, then the forks only marks reach, on the
    eight q of even222_w0_n40: every lane on an aux stream (3 lanes, no pipe), the ready cap (4
    asked, 3 run), the ready-and-pipe cap (3 asked, 2 run beside the FFT stream, ring of 4), and
    pieces with the ring (fisdf_set_y_slices marks its q ready as well, so 3 asked, 2 run)."""
    n = "even222_w0_n40"
    return [Run(n, 1, 1, 0, -1, 0, LSTSQ, y) for y in ("slices", "ready")] + \
           [Run("axes222_w0_n5", 1, 1, 0, -1, 0, LSTSQ, "slices"),
            Run(n, 1, 1, 3, 0, 0, LSTSQ, "ready"), Run(n, 1, 1, 4, 0, 0, LSTSQ, "ready"),
            Run(n, 1, 1, 3, 1, 0, LSTSQ, "ready"), Run(n, 1, 1, 3, 1, 0, LSTSQ, "slices")]


def split_runs():
    return [(Run("split311_w0_n256", 1, 1, 0, -1, 0, LSTSQ, "contig"), env) for env in (None, 1)]


def all_runs():
    return wq_runs() + invariance_runs() + rank_runs() + y_runs() + [r for r, _ in split_runs()]


def run_ranks(run):
    """Ranks the device must return: FISDF_FIT_SVD factors every q with pivoting, which changes no
    rank here."""
    return case_ranks(BY_NAME[run.case])


def run_lanes(run):
    c = BY_NAME[run.case]
    return fit_lanes(len(c.qs), run.lanes, run.pipe, run.depth, run.y in ("slices", "ready"))


def run_ysrc(run):
    c = BY_NAME[run.case]
    if run.y != "slices":
        return Y_CONTIG
    return Y_SLICES if FF.reads_slices(c.mesh) else Y_UNPACKED


def run_reports(run, ksplit_env=WPP_KSPLIT_DEFAULT, omega=None):
    c = BY_NAME[run.case]
    nl, _ = run_lanes(run)
    ranks = run_ranks(run)
    return [predict_report(c, j, ranks, run.real, run.half, nl, run.mode, run_ysrc(run),
                           ksplit_env, omega) for j in range(len(c.qs))]


FIT_BRANCHES = {
    "real_factor", "complex_factor", "half_grid", "full_grid_real", "herm_fft", "half_plain_fft",
    "m0_0", "m0_1", "m1_0", "m1_1", "m2_0", "m2_1", "prefix_all_planes", "prefix_one_plane",
    "asym_full", "asym_half", "asym_full_empty", "asym_half_empty",
    "omega_zero", "omega_neg", "omega_pos",
    "fft_reg", "fft_plane", "fft_axes",
    "lanes_1", "lanes_2", "lanes_3", "lanes_4", "pipe_on", "pipe_off", "ring_reuse", "ring_whole",
    "wpp_lane", "wpp_tail_gemm", "wpp_tail_trsm", "wpp_split", "wpp_nosplit",
    "solve_linv", "solve_min_norm", "solve_blocked", "rank_zero", "min_norm_real_half",
    "y_contig", "y_slices", "y_unpacked", "y_ready",
}


def run_branches(run, ksplit_env=WPP_KSPLIT_DEFAULT):
    c = BY_NAME[run.case]
    nl, depth = run_lanes(run)
    out = {"lanes_%d" % nl, "pipe_on" if depth else "pipe_off",
           "omega_zero" if c.omega == 0 else "omega_neg" if c.omega < 0 else "omega_pos",
           {FF.REG: "fft_reg", FF.PLANE: "fft_plane", FF.AXES: "fft_axes"}[
               FF.base_route(c.mesh) & ~FF.BIG]}
    if depth:
        out.add("ring_reuse" if len(c.qs) > depth else "ring_whole")
    if run.y == "ready":
        out.add("y_ready")
    for j, rep in enumerate(run_reports(run, ksplit_env)):
        out.add("real_factor" if rep.real else "complex_factor")
        if rep.real:
            m = self_m(c.kmesh, c.qs[j])
            out.update("m%d_%d" % (d, m[d]) for d in range(3))
            out.add("half_grid" if rep.half else "full_grid_real")
            if rep.rank > 0:
                kind = "asym_half" if rep.half else "asym_full"
                out.add(kind if rep.nasym else kind + "_empty")
        if rep.half and rep.rank > 0:
            out.add("herm_fft" if rep.herm else "half_plain_fft")
            planes = rep.ncol // (c.mesh[1] * c.mesh[2])
            if planes == c.mesh[0]:
                out.add("prefix_all_planes")
            if planes == 1:
                out.add("prefix_one_plane")
        out.add({SOLVE_LINV: "solve_linv", SOLVE_MIN_NORM: "solve_min_norm",
                 SOLVE_BLOCKED: "solve_blocked", SOLVE_NONE: "rank_zero"}[rep.solve])
        if rep.min_norm and rep.half:
            out.add("min_norm_real_half")
        out.add({WPP_LANE: "wpp_lane", WPP_TAIL_GEMM: "wpp_tail_gemm",
                 WPP_TAIL_TRSM: "wpp_tail_trsm"}[rep.wpp])
        out.add("wpp_split" if rep.split > 1 else "wpp_nosplit")
        out.add({Y_CONTIG: "y_contig", Y_SLICES: "y_slices", Y_UNPACKED: "y_unpacked"}[rep.ysrc])
    return out
