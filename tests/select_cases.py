"""Cases, restated rules and references for the interpolation-point selection (pchol.hip from
pchol_select_coop on, select_gram and select_pivots_dev in api.hip).  No GPU here;
test_select_cases.py checks this file on the CPU and test_gpu_select_variants.py runs the device
against it.  The references, the float64 restatements and the error rule are factor_cases.py's.

  * the dispatch rules restated (default mode, the batched kernel's and the cooperative kernel's
    sizes and refusals, the Gram's representatives, launches and split-K), compared with
    fisdf_select_plan and fisdf_select_gram_plan;
  * pivot cases named for the path they are meant to reach, with inputs x2 = Re + i garbage whose
    greedy sequence is unique (certified in test_select_cases.py);
  * twin inputs (two bit-identical rows and columns) and the rule their pivots must meet;
  * Gram cases with their long-double references.
"""
from collections import namedtuple

import numpy as np

import factor_cases as F

LD = F.LD

# ------------------------------------------------------------------ restated rules
SEL_LDS = 150 * 1024        # dynamic LDS of a selection workgroup at most
SC_THREADS, SC_MAXRW = 512, 64
SB_M, SB_S, SB_ROWS = 32, 16, 16
SB_NMAX = 8 * 512
SB_NPUB = 1 + SB_M + SB_S + SB_M * SB_S
BATCH, COOP, COOP_SPLIT, PANEL, GENERIC_BLOCKED, GENERIC_STEP = range(6)
KERNEL_NAMES = ("batch", "coop", "coop-split", "panel", "generic blocked", "generic per-step")
# refusals, in the order the launchers check them
B_OK, B_N_SMALL, B_N_LARGE, B_RMAX, B_GRID, B_LDS, B_SCRATCH = range(7)
C_OK, C_N_SMALL, C_NO_GRID, C_K_SMALL, C_LDS, C_ROWS, C_SCRATCH = range(7)

BatchPlan = namedtuple("BatchPlan", "ok why grid RW lds")
CoopPlan = namedtuple("CoopPlan", "ok why split G RW K tpr lds")


def default_mode(rmax):
    return 0 if rmax >= 800 else 1


def batch_plan(n, rmax, ncu):
    if n < 2 * SB_M:
        return BatchPlan(0, B_N_SMALL, 0, 0, 0)
    if n > SB_NMAX:
        return BatchPlan(0, B_N_LARGE, 0, 0, 0)
    if rmax > 4096:
        return BatchPlan(0, B_RMAX, 0, 0, 0)
    grid = (n + SB_ROWS - 1) // SB_ROWS + 1
    if grid > ncu:
        return BatchPlan(0, B_GRID, grid, SB_ROWS, 0)
    owner = 8 * (8 * 256 + SB_M * SB_S + 2 * 16 * SB_S + SB_ROWS * rmax)
    leader = 8 * (3 * 8 * 256 + SB_M * SB_M + 64 + SB_M * SB_S + 16)
    lds = max(owner, leader)
    if lds > SEL_LDS:
        return BatchPlan(0, B_LDS, grid, SB_ROWS, lds)
    if 2 * n + 2 * SB_NPUB + n * rmax + 2 > n * n:
        return BatchPlan(0, B_SCRATCH, grid, SB_ROWS, lds)
    return BatchPlan(1, B_OK, grid, SB_ROWS, lds)


def coop_plan(n, rmax, ncu, lds_cols=0, wgs=0):
    if n < 64:
        return CoopPlan(0, C_N_SMALL, 0, 0, 0, 0, 0, 0)
    G = min(wgs if wgs > 0 else 128, ncu, (n + 7) // 8)
    if G < 1:
        return CoopPlan(0, C_NO_GRID, 0, 0, 0, 0, 0, 0)
    RW = (n + G - 1) // G
    G = (n + RW - 1) // RW
    K, split = rmax, 0
    lds = 8 * (RW * rmax + rmax + 2 * RW)
    if lds > SEL_LDS or lds_cols > 0:
        split = 1
        G = min(ncu, (n + 7) // 8)
        RW = (n + G - 1) // G
        G = (n + RW - 1) // RW
        num = SEL_LDS // 8 - rmax - 2 * RW
        K = -((-num) // RW) if num < 0 else num // RW      # C division truncates towards zero
        if lds_cols > 0:
            K = min(K, lds_cols)
        if K < 16:
            return CoopPlan(0, C_K_SMALL, 1, G, RW, K, 0, 0)
        K = min(K, rmax)
        lds = 8 * (RW * K + rmax + 2 * RW)
    if lds > SEL_LDS:
        return CoopPlan(0, C_LDS, split, G, RW, K, 0, lds)
    if RW > SC_MAXRW:
        return CoopPlan(0, C_ROWS, split, G, RW, K, 0, lds)
    tpr = 8
    while tpr < 32 and RW * tpr * 2 <= SC_THREADS:
        tpr *= 2
    if 4 * G + n * rmax + 2 > n * n:
        return CoopPlan(0, C_SCRATCH, split, G, RW, K, tpr, lds)
    return CoopPlan(1, C_OK, split, G, RW, K, tpr, lds)


def reached(n, rmax, ncu, mode=-1, lds_cols=0, wgs=0):
    """(kernel, G, RW, K, tpr) of what produces the pivots when nothing stalls: the mode's kernel,
    or the next one that takes the sizes (batch, coop, panel, generic)."""
    mode = default_mode(rmax) if mode < 0 else mode
    b = batch_plan(n, rmax, ncu)
    if mode == 0 and b.ok:
        return (BATCH, b.grid, b.RW, rmax, 0)
    c = coop_plan(n, rmax, ncu, lds_cols, wgs)
    if mode <= 1 and c.ok:
        return (COOP_SPLIT if c.split else COOP, c.G, c.RW, c.K, c.tpr)
    rpt, nb = F.sel_variant(n)
    if rpt:
        return (PANEL, 1, rpt, nb, 0)
    if F.pchol_path(n) == F.BLOCKED:
        return (GENERIC_BLOCKED, 0, 0, F.PCHOL_NB, 0)
    return (GENERIC_STEP, 0, 0, 0, 0)


def kmesh_partner(k, km):
    i2, i1, i0 = k % km[2], (k // km[2]) % km[1], k // (km[1] * km[2])
    return (((-i0) % km[0]) * km[1] + (-i1) % km[1]) * km[2] + (-i2) % km[2]


def kmesh_reps(km):
    """The k <= -k of the mesh and the weight of each in the folded sum (1 self-paired, 2 paired)."""
    nk = km[0] * km[1] * km[2]
    reps = [k for k in range(nk) if k <= kmesh_partner(k, km)]
    return reps, [1 if kmesh_partner(k, km) == k else 2 for k in reps]


def gram_ksplit(ng0, K):
    tiles = ((ng0 + 63) // 64) * ((ng0 + 63) // 64 + 1) // 2
    ks = 1
    while tiles * ks < 512 and K // (ks * 2) >= 256:
        ks *= 2
    return ks


def gram_plan(km, fold, nq, ng0, nao):
    """(k-points summed, permute launches, HERK split-K)."""
    launches = 1 if nq > 0 else 0
    if km is not None and fold:
        nq = len(kmesh_reps(km)[0])
        launches = (nq + 63) // 64
    return (nq, launches, gram_ksplit(ng0, nq * nao) if nq > 0 else 0)


# ------------------------------------------------------------------ pivot cases
NK = 2            # x4 = Re(x2)^2 / NK
TOP = 40          # rows with the largest diagonals in the clustered and strided families
# family: random | clustered | strided | graded | stop; k: columns of the factor B (x4 = (B B^T)^2
# has rank k (k + 1) / 2, so the updates move the residual diagonal by a large part of itself)
PivCase = namedtuple("PivCase", "name n rmax tol mode lds_cols wgs family k seed expect imag")


def _pc(name, n, rmax, mode, family, expect, tol=-1.0, lds_cols=0, wgs=0, k=10, seed=0, imag=True):
    return PivCase(name, n, rmax, tol, mode, lds_cols, wgs, family, k, seed, expect, imag)


PIV_CASES = [
    # the batched kernel
    _pc("b64_r44", 64, 44, 0, "random", BATCH, seed=101),
    _pc("b65", 65, 40, 0, "random", BATCH, seed=102),
    _pc("b600_random", 600, 40, 0, "random", BATCH, seed=103),
    _pc("b600_clustered", 600, 40, 0, "clustered", BATCH, seed=104),
    _pc("b600_strided", 600, 40, 0, "strided", BATCH, seed=105),
    _pc("b1030_clustered", 1030, 40, 0, "clustered", BATCH, seed=106),
    _pc("b4080_strided", 4080, 40, 0, "strided", BATCH, seed=107),
    _pc("b600_stop10_toln", 600, 40, 0, "stop", BATCH, k=4, seed=108),
    _pc("b600_stop10_tol", 600, 40, 0, "stop", BATCH, tol=1e-10, k=4, seed=109),
    _pc("b600_stop21_toln", 600, 40, 0, "stop", BATCH, k=6, seed=110),
    _pc("b600_stop21_tol", 600, 40, 0, "stop", BATCH, tol=1e-10, k=6, seed=111),
    # batch asked for and refused: the cooperative kernel runs
    _pc("b4081_to_coop", 4081, 40, 0, "strided", COOP, seed=112),
    _pc("b64_r45_to_coop", 64, 45, 0, "random", COOP, seed=113),
    # the cooperative kernel
    _pc("c64_rw8", 64, 40, 1, "random", COOP, seed=114),
    _pc("c64_r63", 64, 63, 1, "graded", COOP, seed=115),
    _pc("c65_rw8_tail1", 65, 40, 1, "random", COOP, seed=116),
    _pc("c150_wgs3", 150, 40, 1, "clustered", COOP, wgs=3, seed=117),
    _pc("c600_clustered", 600, 40, 1, "clustered", COOP, seed=104),
    _pc("c600_stop10_toln", 600, 40, 1, "stop", COOP, k=4, seed=108),
    _pc("c600_stop21_tol", 600, 40, 1, "stop", COOP, tol=1e-10, k=6, seed=111),
    _pc("c2048_rw16", 2048, 40, 1, "strided", COOP, seed=118),
    _pc("c2049_rw17", 2049, 40, 1, "clustered", COOP, seed=119),
    _pc("c4225_rw34_tpr8", 4225, 40, 1, "strided", COOP, seed=120),
    _pc("c8192_rw64", 8192, 24, 1, "strided", COOP, seed=121, imag=False),
    # its split form: rmax - K >= 28 columns read back from the global L
    _pc("s600_k16", 600, 48, 1, "random", COOP_SPLIT, lds_cols=16, seed=122),
    _pc("s600_k20", 600, 48, 1, "clustered", COOP_SPLIT, lds_cols=20, seed=123),
    _pc("s2049_k16", 2049, 48, 1, "clustered", COOP_SPLIT, lds_cols=16, seed=124),
    _pc("s2049_k20", 2049, 48, 1, "random", COOP_SPLIT, lds_cols=20, seed=125),
    _pc("s600_stop21_tol", 600, 40, 1, "stop", COOP_SPLIT, tol=1e-10, lds_cols=16, k=6, seed=111),
    # the register panels
    _pc("p600_clustered", 600, 40, 2, "clustered", PANEL, seed=104),
    _pc("p600_stop21_tol", 600, 40, 2, "stop", PANEL, tol=1e-10, k=6, seed=111),
    # tiny Grams (the panels' scratch, n*n + 17 n + 1 doubles, is larger than the n x n complex
    # work area below n = 18)
    _pc("t1", 1, 1, -1, "graded", PANEL, seed=131),
    _pc("t8_r1", 8, 1, -1, "graded", PANEL, seed=132),
    _pc("t8_rn", 8, 8, -1, "graded", PANEL, seed=133),
    _pc("t17_r1", 17, 1, -1, "graded", PANEL, seed=134),
    _pc("t17_r2", 17, 2, -1, "graded", PANEL, seed=135),
    _pc("t17_rn", 17, 17, -1, "graded", PANEL, seed=136),
    # refused by both co-resident kernels
    _pc("n63_to_panel", 63, 40, -1, "random", PANEL, seed=126),
    _pc("n8193_to_step", 8193, 24, -1, "strided", GENERIC_STEP, seed=127, imag=False),
    # rmax = n: neither scratch fits the n x n work area, the panels run
    _pc("n64_rmaxn", 64, 64, -1, "graded", PANEL, seed=128),
    _pc("n96_rmaxn", 96, 96, -1, "graded", PANEL, seed=129),
    # the default rule (mode -1) on either side of 800 pivots; the long-double reference of 800
    # pivots takes under two seconds, so the whole sequence is compared
    _pc("d1030_r799", 1030, 799, -1, "graded", COOP, seed=130),
    _pc("d1030_r800", 1030, 800, -1, "graded", BATCH, seed=130),
]
PIV_BY_NAME = {c.name: c for c in PIV_CASES}
# one stop case and one clustered case on all four kernels, identical results
CROSS = {"stop": ("b600_stop21_tol", "c600_stop21_tol", "s600_stop21_tol", "p600_stop21_tol"),
         "clustered": ("b600_clustered", "c600_clustered", "p600_clustered")}
CROSS_SPLIT_OF = {"clustered": ("c600_clustered", 20)}   # the same input with lds_cols = 20
# the imaginary garbage is exchanged for another on one case per kernel
IMAG_CASES = ("b600_random", "c65_rw8_tail1", "s600_k16", "p600_clustered")


def _mirror(g):
    g = np.tril(g)
    return g + np.tril(g, -1).T


def top_rows(family, n, seed):
    if family == "clustered":
        i0 = (seed * 37) % (n - TOP)
        return i0 + np.arange(TOP)
    return ((seed * 37) % n + 97 * np.arange(TOP)) % n       # strided: 97 rows apart


def case_real(c):
    """Re x2 of a case: B B^T (+ a graded diagonal), exactly symmetric."""
    rng = np.random.default_rng(c.seed)
    B = rng.standard_normal((c.n, c.k))
    if c.family in ("clustered", "strided"):
        # unit rows times a factor: 0.8..1 everywhere, 1.3..1.6 on the TOP rows, so that these hold
        # the TOP largest diagonals of x4 (the factor's fourth power)
        f = rng.uniform(0.8, 1.0, c.n)
        top = top_rows(c.family, c.n, c.seed)
        assert len(set(top.tolist())) == TOP
        f[top] = rng.uniform(1.3, 1.6, TOP)
        B *= (f / np.linalg.norm(B, axis=1))[:, None]
    g = _mirror(B @ B.T)
    if c.family == "graded":
        # full rank with a diagonal falling by 100 over the rows (shuffled)
        grade = g.diagonal().mean() * 10.0 ** (-2.0 * rng.permutation(c.n) / max(c.n - 1, 1))
        g[np.diag_indices(c.n)] += grade
    return g


def case_imag(c, other=False):
    if not c.imag:
        return None
    return np.random.default_rng(c.seed + (7777 if other else 5555)).standard_normal((c.n, c.n))


def case_x2(c, other_imag=False):
    re, im = case_real(c), case_imag(c, other_imag)
    return re + 1j * im if im is not None else re.astype(np.complex128)


def x4_of(re):
    return re * re * (1.0 / NK)


def reference(re, rmax, tol):
    """The long-double greedy sequence of x4 = re^2 / NK, columns formed on demand."""
    sc = LD(1) / LD(NK)
    col = lambda p: re[:, p].astype(LD) ** 2 * sc
    return F.greedy_ld(col, re.diagonal().astype(LD) ** 2 * sc, rmax, tol, 0.0, real=True)


def restated(re, rmax, tol, skip_updates=False):
    """float64: left-looking as the co-resident kernels are; with skip_updates the wrong algorithm
    that forgets the pivots of every finished group of four."""
    return F.greedy_f64(x4_of(re), rmax, tol, 0.0, 4 if skip_updates else None, skip_updates)


# ------------------------------------------------------------------ twin inputs
# rows and columns a < b of Re x2 bit-identical; top: the pair holds the largest diagonal, so it is
# met at step 0, where nothing has been updated and the smaller index must win
TwinCase = namedtuple("TwinCase", "name n rmax a b top seed")
TWIN_N, TWIN_RMAX = 600, 40
TWIN_CASES = [
    TwinCase("adjacent", TWIN_N, TWIN_RMAX, 300, 301, False, 201),
    TwinCase("apart16", TWIN_N, TWIN_RMAX, 300, 316, False, 202),
    TwinCase("half", TWIN_N, TWIN_RMAX, 100, 100 + TWIN_N // 2, False, 203),
    TwinCase("ends", TWIN_N, TWIN_RMAX, 0, TWIN_N - 1, False, 204),
    TwinCase("adjacent_top", TWIN_N, TWIN_RMAX, 15, 16, True, 205),
    TwinCase("half_top", TWIN_N, TWIN_RMAX, 100, 100 + TWIN_N // 2, True, 206),
]
TWIN_BY_NAME = {c.name: c for c in TWIN_CASES}
TWIN_MODES = (0, 1, 2)          # batch, coop, panels; coop also in its split form (lds_cols 16)


def twin_real(c):
    rng = np.random.default_rng(c.seed)
    B = rng.standard_normal((c.n, 10))
    nrm = np.linalg.norm(B, axis=1)
    B[c.a] *= (1.1 if c.top else 0.97) * nrm.max() / nrm[c.a]
    g = _mirror(B @ B.T)
    g[c.b, :] = g[c.a, :]
    g[:, c.b] = g[:, c.a]
    return g


def twin_x2(c):
    return twin_real(c) + 1j * np.random.default_rng(c.seed + 5555).standard_normal((c.n, c.n))


def twin_reference(c):
    """The reference of the matrix without row and column b, in the full matrix's indices."""
    re = twin_real(c)
    keep = np.delete(np.arange(c.n), c.b)
    ref = reference(re[np.ix_(keep, keep)], c.rmax, -1.0)
    return ref, keep[ref.piv]


def twin_ok(c, piv, expect):
    """expect: twin_reference's pivots.  The device's must be these, b allowed in a's place except
    at step 0, and the pair never twice."""
    piv = np.asarray(piv)
    if piv.shape != expect.shape or (c.a in piv and c.b in piv):
        return False
    if not np.array_equal(np.where(piv == c.b, c.a, piv), expect):
        return False
    return not (expect[0] == c.a and piv[0] != c.a)


# ------------------------------------------------------------------ Gram cases
# plain: x2 = Re sum_k x0_k x0_k^H over nk k-points without a k-mesh (fisdf_select_gram)
GRAM_NG0 = (1, 63, 64, 65, 130)
GRAM_NAO = (1, 3, 13)
GRAM_PLAIN_NK = 3
GRAM_SHARDS = ((0, 1), (1, 1), (1, 3))           # their sum is the whole; the middle one is empty
# fold: k-mesh, ng0, nao, representatives, permute launches, split-K folded and unfolded
GramFold = namedtuple("GramFold", "km ng0 nao reps launches ks_fold ks_all")
GRAM_FOLD = [
    GramFold((1, 1, 1), 65, 3, 1, 1, 1, 1),
    GramFold((2, 2, 2), 65, 13, 8, 1, 1, 1),
    GramFold((3, 3, 1), 64, 13, 5, 1, 1, 1),
    GramFold((4, 4, 4), 65, 13, 36, 1, 1, 2),
    GramFold((5, 5, 5), 63, 13, 63, 1, 2, 4),
    GramFold((1, 1, 127), 65, 3, 64, 1, 1, 1),
    GramFold((1, 1, 129), 65, 3, 65, 2, 1, 1),
    GramFold((6, 6, 6), 65, 3, 112, 2, 1, 2),
]


def gram_x0(nk, ng0, nao, seed, km=None):
    """x0 (nk, ng0, nao); with a k-mesh x0[-k] = conj(x0[k]) exactly (a self-paired k real)."""
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((nk, ng0, nao)) + 1j * rng.standard_normal((nk, ng0, nao))
    if km is not None:
        for k in range(nk):
            p = kmesh_partner(k, km)
            if p == k:
                x0[k] = x0[k].real
            elif k < p:
                x0[p] = x0[k].conj()
    return x0


def _gram(x0, ks, w, wide):
    """sum over the listed k of w_k Re(x0_k x0_k^H) in the real type `wide`."""
    ng0 = x0.shape[1]
    out = np.zeros((ng0, ng0), wide)
    for k, wk in zip(ks, w):
        re, im = x0[k].real.astype(wide), x0[k].imag.astype(wide)
        out += wide(wk) * (re @ re.T + im @ im.T)
    return out


def gram_reference(x0, ks=None, w=None):
    """(long-double reference, factor_cases.bound of the float64 restatement's own error, n = the
    Gram's size)."""
    ks = range(x0.shape[0]) if ks is None else ks
    w = [1] * len(ks) if w is None else w
    ref = _gram(x0, ks, w, LD)
    return ref, F.bound(F.relerr(_gram(x0, ks, w, np.float64), ref), x0.shape[1])


# ------------------------------------------------------------------ a tie with the batch's bound
# Rows TIE_A < TIE_B are orthogonal to every other row and have the same diagonal, bit for bit and
# at every step on every path (their updates are exact zeros).  Four larger rows share TIE_A's
# leader wave (rows 0..63 of the batched kernel's leader), so TIE_A is the best row left out of the
# first batch's candidates, its bound B, while TIE_B is a candidate of the next wave.  After the
# four, the candidates' best equals B and has the larger index: the batch must end there, and the
# next one take TIE_A, then TIE_B, as LAPACK's first-index rule has it.
TIE_N, TIE_RMAX, TIE_A, TIE_B, TIE_SEED = 600, 40, 10, 100, 301
TIE_CROWD = (1, 2, 3, 4)


def tie_real():
    rng = np.random.default_rng(TIE_SEED)
    B = rng.standard_normal((TIE_N, 10))
    f = rng.uniform(0.8, 1.0, TIE_N)
    f[list(TIE_CROWD)] = rng.uniform(1.5, 1.6, len(TIE_CROWD))
    B *= (f / np.linalg.norm(B, axis=1))[:, None]
    g = _mirror(B @ B.T)
    for r in (TIE_A, TIE_B):
        g[r, :] = 0.0
        g[:, r] = 0.0
        g[r, r] = 1.2
    return g


def tie_x2():
    im = np.random.default_rng(TIE_SEED + 5555).standard_normal((TIE_N, TIE_N))
    return tie_real() + 1j * im


# ------------------------------------------------------------------ composite entries
COMP_KM, COMP_NG0, COMP_NAO, COMP_NIP, COMP_SEED = (3, 3, 1), 130, 2, 40, 401


def composite_input():
    """x0 (9, 130, 2) with x0[-k] = conj(x0[k]), and the long-double sequence of its x4."""
    nk = COMP_KM[0] * COMP_KM[1] * COMP_KM[2]
    x0 = gram_x0(nk, COMP_NG0, COMP_NAO, COMP_SEED, COMP_KM)
    x2 = gram_reference(x0)[0]
    x4 = x2 * x2 / LD(nk)
    ref = F.greedy_ld(lambda p: x4[:, p], x4.diagonal(), COMP_NIP, -1.0, 0.0, real=True)
    return x0, x4, ref
