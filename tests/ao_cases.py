"""Cases and references for the Bloch AO evaluator: csrc/ao.hip (ao_folded_kernel, the table
building and translation grouping of eval_ao), csrc/sph.h, the C-ABI entries fisdf_eval_ao /
fisdf_eval_ao_band and the wrappers fisdf.ao.eval_ao_kpts_gpu / eval_ao_band_gpu.  No tests and no
GPU here: tests/test_ao_cases.py checks this file (and the host restatement fisdf.cell) on the
CPU, tests/test_gpu_ao_variants.py runs the device against it.

Nothing here takes a constant, an order or a normalisation from fisdf.cell or sph.h:
  * the real solid harmonics come from their definition (exact integer factorials, pi as a
    long-double literal), in np.longdouble;
  * the lattice sum is written for the raw tables the C-ABI takes,
        F_R(r)   = sum_{T = R mod kmesh} [|r - A - T|^2 < rcut^2]
                   sum_p c_p exp(-alpha_p |r - A - T|^2) S_lm(r - A - T)
        chi_k(r) = sum_R exp(2 pi i sum_a R_a k_a / n_a) F_R(r)          (k-mesh)
        chi_k(r) = sum_T exp(i k . T) F_T(r)                             (band k-points)
    in np.longdouble, the k-mesh phases from integer-reduced indices (kmesh_cases.mesh_dft);
  * the radial normalisation int r^2 (sum_i c_i r^l exp(-alpha_i r^2))^2 dr = 1 is restated with
    Gamma(l + 3/2) from its closed form, so the real-cell references do not take the coefficients
    stored in cell.shells.
Beside the long-double sums stand the same sums in float64, in the device's order ((r - A) - T,
the translations of an image in list order, then the DFT).  They only measure what float64
arithmetic alone costs: the device may be factor_cases.BOUND_FACTOR times that far from the
reference, never less than n eps (n the longest sum), per AO column.

The cutoff is a discontinuity, and the device forms (r - A) - T where the reference forms
r - (A + T): the inputs are chosen so that no (point, atom, T) triple has
|r^2 / rcut^2 - 1| < NEAR_CUT.  That is a condition on the inputs (near_cutoff counts the
triples, test_ao_cases.py holds the count at zero), not a tolerance.
"""
import functools
import math
from collections import namedtuple

import numpy as np

import kmesh_cases as K
from factor_cases import BOUND_FACTOR, CLD, EPS, LD, bound  # noqa: F401
from jfft_cases import EDGE, SENTINEL  # noqa: F401

PI = LD("3.14159265358979323846264338327950288")
NEAR_CUT = 1e-9
NSPH = {0: 1, 1: 3, 2: 5, 3: 7}
BLOCK = 256                    # threads of one ao_folded_kernel workgroup, one per (point, AO)


# ---- real solid harmonics from the definition --------------------------------------------------
def _pi_lm_terms(l, m):
    """Pi_l^m = sqrt((l-m)!/(l+m)!) 2^-l sum_k (-1)^k C(l,k) C(2l-2k,l) (l-2k)!/(l-2k-m)!
    r^2k z^(l-2k-m): the exact integers (numerator, k, power of z) and the integer ratio under the
    root."""
    terms = []
    for k in range((l - m) // 2 + 1):
        num = (-1) ** k * math.comb(l, k) * math.comb(2 * l - 2 * k, l) * math.factorial(l - 2 * k)
        assert num % math.factorial(l - 2 * k - m) == 0
        terms.append((num // math.factorial(l - 2 * k - m), k, l - 2 * k - m))
    return terms, (math.factorial(l - m), math.factorial(l + m))


def m_order(l):
    """m of every component: -l..l, except l = 1, which is (x, y, z) = (+1, -1, 0)."""
    return [1, -1, 0] if l == 1 else list(range(-l, l + 1))


def sph(l, x, y, z, dt=LD):
    """S_lm(x, y, z) = r^l Y_lm for the 2 l + 1 components in m_order(l), no Condon-Shortley sign:
    S_l0 = sqrt((2l+1)/4pi) Pi_l^0, S_l,+m = sqrt((2l+1)/2pi) Pi_l^m Re (x+iy)^m, S_l,-m the same
    with Im.  dt: the arithmetic (np.longdouble for the references)."""
    x, y, z = (np.asarray(t, dt) for t in (x, y, z))
    r2 = x * x + y * y + z * z
    pi = dt(PI)
    out = {}
    for m in range(l + 1):
        terms, (fn, fd) = _pi_lm_terms(l, m)
        P = np.zeros_like(x)
        for num, k, pz in terms:
            P = P + dt(num) * r2 ** k * z ** pz
        P = P * (np.sqrt(dt(fn) / dt(fd)) / dt(2 ** l))
        re, im = np.ones_like(x), np.zeros_like(x)          # (x + i y)^m
        for _ in range(m):
            re, im = re * x - im * y, re * y + im * x
        if m == 0:
            out[0] = np.sqrt(dt(2 * l + 1) / (4 * pi)) * P
        else:
            n = np.sqrt(dt(2 * l + 1) / (2 * pi))
            out[m], out[-m] = n * P * re, n * P * im
    return [out[m] for m in m_order(l)]


# ---- the radial normalisation ------------------------------------------------------------------
def gamma_half(l):
    """Gamma(l + 3/2) = (2l+1)!! sqrt(pi) / 2^(l+1)."""
    dfact = 1
    for j in range(1, 2 * l + 2, 2):
        dfact *= j
    return LD(dfact) * np.sqrt(PI) / LD(2 ** (l + 1))


def radial_norm(l, exps, coefs):
    """coefs scaled so that int_0^inf r^2 (sum_i c_i r^l exp(-alpha_i r^2))^2 dr = 1, with
    int r^(2l+2) exp(-s r^2) dr = Gamma(l + 3/2) / (2 s^(l + 3/2)); long double."""
    e, c = np.asarray(exps, LD), np.asarray(coefs, LD)
    s = e[:, None] + e[None, :]
    ov = gamma_half(l) / (2 * s ** (LD(2 * l + 3) / 2))
    return c / np.sqrt(c @ ov @ c)


# ---- the raw tables and the lattice sum --------------------------------------------------------
# the arguments of the C-ABI: atoms (natm, 3), shells (atom, l, nprim), exponents and coefficients
# shell after shell, integer translations tn (nT, 3), lattice a (rows), rcut.  coefs_ld: the
# coefficients in long double where they are known wider than float64 (the real cells)
Tables = namedtuple("Tables", "atoms sh_atom sh_l sh_np exps coefs tn a rcut coefs_ld")


def nao_of(tab):
    return int(sum(NSPH[int(l)] for l in tab.sh_l))


def ao_labels(tab):
    """(shell, l, m) of every AO column."""
    return [(i, int(l), m) for i, l in enumerate(tab.sh_l) for m in m_order(int(l))]


def image_of(tn, kmesh):
    """R = n mod kmesh of every translation, as the index (R0 n1 + R1) n2 + R2."""
    r = np.mod(np.asarray(tn, np.int64).reshape(-1, 3), np.asarray(kmesh, np.int64))
    return (r[:, 0] * kmesh[1] + r[:, 1]) * kmesh[2] + r[:, 2]


def _blocks(tab, coords, wide):
    """the (ng, nao) block of every translation (None: nothing in range), and per translation the
    (ng, natm) in-range mask.  wide: long double with r - (A + T); else float64 with (r - A) - T
    and T = n0 a0 + n1 a1 + n2 a2 added in that order, as the device forms them."""
    dt = LD if wide else np.float64
    a = np.asarray(tab.a, dt)
    co, atoms = np.asarray(coords, dt).reshape(-1, 3), np.asarray(tab.atoms, dt)
    exps = np.asarray(tab.exps, dt)
    coefs = np.asarray(tab.coefs_ld if wide and tab.coefs_ld is not None else tab.coefs, dt)
    rc2 = dt(tab.rcut) * dt(tab.rcut)
    ng, nao = len(co), nao_of(tab)
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
                blk = np.zeros((ng, nao), dt)
            ao0 = 0
            for i, (sa, l, npr) in enumerate(zip(tab.sh_atom, tab.sh_l, tab.sh_np)):
                l = int(l)
                if sa == ia:
                    rad = np.zeros(int(m.sum()), dt)
                    for p in range(p0[i], p0[i] + int(npr)):       # the device's order
                        rad = rad + np.exp(-exps[p] * r2[m]) * coefs[p]
                    for j, g in enumerate(sph(l, d[m, 0], d[m, 1], d[m, 2], dt)):
                        blk[m, ao0 + j] = rad * g
                ao0 += NSPH[l]
        yield n, T, blk, inr


def near_cutoff(tab, coords):
    """the (point, atom, T) triples with |r^2 / rcut^2 - 1| < NEAR_CUT, and those in range, of all."""
    a, co = np.asarray(tab.a, LD), np.asarray(coords, LD).reshape(-1, 3)
    tn = np.asarray(tab.tn, np.int64).reshape(-1, 3)
    if len(tn) == 0 or len(co) == 0:
        return 0, 0, 0
    sh = np.asarray(tab.atoms, LD)[None, :, :] + (tn.astype(LD) @ a)[:, None, :]      # A + T
    d = co[None, None] - sh[:, :, None, :]
    q = (d * d).sum(-1) / (LD(tab.rcut) * LD(tab.rcut))
    return int((np.abs(q - 1) < NEAR_CUT).sum()), int((q < 1).sum()), q.size


Sums = namedtuple("Sums", "chi nsum F")        # F: the folded images (k-mesh), else None


def kmesh_sum(tab, coords, kmesh, wide=True):
    """chi (nk, ng, nao) of the k-mesh and the length of its longest sum: the in-range
    translations of one image at one (point, atom), times the largest nprim, plus the images."""
    nimg = K.nk_of(kmesh)
    ng, nao = len(np.reshape(coords, (-1, 3))), nao_of(tab)
    F = np.zeros((nimg, ng, nao), LD if wide else np.float64)
    cnt = np.zeros((nimg, ng, len(tab.atoms)), np.int64)
    img = image_of(tab.tn, kmesh)
    for t, (n, T, blk, inr) in enumerate(_blocks(tab, coords, wide)):
        cnt[img[t]] += inr
        if blk is not None:
            F[img[t]] += blk
    chi = np.zeros((nimg, ng, nao), CLD if wide else np.complex128)
    if ng:
        chi = K.mesh_dft(F.reshape(nimg, -1), kmesh, wide=wide, scale=False).reshape(nimg, ng, nao)
    return Sums(chi, int(cnt.max(initial=0)) * int(max(tab.sh_np)) + nimg, F)


def band_sum(tab, coords, kband, wide=True):
    """chi (nkb, ng, nao) at the band k-points: one image per translation, phases exp(i k . T);
    float64: the phases from the float64 T, summed in list order, as the device does."""
    dt, cdt = (LD, CLD) if wide else (np.float64, np.complex128)
    kb = np.asarray(kband, dt).reshape(-1, 3)
    ng, nao = len(np.reshape(coords, (-1, 3))), nao_of(tab)
    chi = np.zeros((len(kb), ng, nao), cdt)
    for n, T, blk, inr in _blocks(tab, coords, wide):
        if blk is None:
            continue
        th = (kb[:, 0] * T[0] + kb[:, 1] * T[1]) + kb[:, 2] * T[2]
        ph = np.empty(len(kb), cdt)
        ph.real, ph.imag = np.cos(th), np.sin(th)
        chi += ph[:, None, None] * blk[None]
    return Sums(chi, int(max(tab.sh_np)) + len(np.reshape(tab.tn, (-1, 3))), None)


def col_err(x, ref):
    """per AO column: max over k and points of |x - ref| over max |ref| of that column (1 where the
    column of the reference is all zero), long double."""
    ref = np.asarray(ref, CLD)
    if ref.size == 0:
        return np.zeros(ref.shape[-1])
    den = np.abs(ref).max(axis=(0, 1))
    num = np.abs(np.asarray(x, CLD) - ref).max(axis=(0, 1))
    return np.asarray(num / np.where(den > 0, den, 1), np.float64)


def reciprocal(a):
    """b with a_i . b_j = 2 pi delta_ij (rows), float64 as a caller would hand it over."""
    return 2 * np.pi * np.linalg.inv(np.asarray(a, float)).T


def mesh_kpts(a, kmesh):
    """the k-points of a k-mesh, (k0 n1 + k1) n2 + k2 order: sum_a (k_a / n_a) b_a."""
    fr = np.stack(np.meshgrid(*[np.arange(n) / n for n in kmesh], indexing="ij"), -1).reshape(-1, 3)
    return fr @ reciprocal(a)


# ---- raw-table cases ---------------------------------------------------------------------------
# triclinic: no two lengths (4.11, 4.99, 5.69 bohr) or angles equal
LATTICE = np.array([[4.1, 0.3, -0.2], [0.7, 4.9, 0.5], [-0.4, 0.9, 5.6]])
ATOMS = np.array([[0.37, 0.81, 1.13], [2.29, 3.07, 2.61]])        # generic positions
RCUT, RCUT_MASKED, RCUT_NONE = 6.0, 2.3, 1e-3

# shells: (atom, l, exponents, coefficients); all exponents distinct, so no two AOs coincide
SHELLS = {
    # one shell of each l on one atom, nprim = 1 (nao 16)
    "each_l": [(0, 0, [0.83], [1.0]), (0, 1, [0.61], [1.3]), (0, 2, [0.47], [0.9]),
               (0, 3, [0.39], [1.1])],
    # two atoms, shells in mixed order (f, s, d, p, s), nprim 1..5, some coefficients negative
    # (nao 17)
    "mixed": [(1, 3, [0.52], [0.8]),
              (0, 0, [3.1, 1.7, 0.93, 0.44, 0.29], [0.15, -0.11, -0.47, 0.57, 0.2]),
              (1, 2, [1.25, 0.41], [0.6, -0.35]),
              (0, 1, [2.2, 0.77, 0.33], [-0.09, 0.28, 0.49]),
              (1, 0, [1.9, 0.85, 0.48, 0.31], [0.2, -0.3, 0.5, 0.45])],
    # s, p, d on the second atom (nao 9)
    "spd": [(1, 0, [0.71, 0.36], [0.4, 0.7]), (1, 1, [0.58], [1.0]), (1, 2, [0.43], [-1.2])],
}


def _box(lo, hi):
    return np.stack(np.meshgrid(*[np.arange(l, h + 1) for l, h in zip(lo, hi)], indexing="ij"),
                    -1).reshape(-1, 3)


def translations(kind):
    if kind == "box":                   # cartesian order, the images interleaved
        return _box((-2, -2, -2), (2, 2, 2))
    if kind == "shuffled":              # the translations of one image are not contiguous
        t = _box((-2, -2, -2), (2, 2, 2))
        return t[np.random.default_rng(77).permutation(len(t))]
    if kind == "neg":                   # 5 x 7 x 5, mostly negative: no multiple of a k-mesh axis
        return _box((-3, -2, -4), (1, 4, 0))
    if kind == "one":
        return np.array([[1, -1, 0]])
    assert kind == "none"
    return np.zeros((0, 3), int)


def raw_tables(shells, tn, rcut):
    sh = SHELLS[shells]
    return Tables(ATOMS, np.array([s[0] for s in sh], np.int32), np.array([s[1] for s in sh], np.int32),
                  np.array([len(s[2]) for s in sh], np.int32),
                  np.array([e for s in sh for e in s[2]], float),
                  np.array([c for s in sh for c in s[3]], float),
                  np.ascontiguousarray(translations(tn), np.int32), LATTICE, float(rcut), None)


def raw_points(ng, seed):
    """random points (no grid) in the cell and half a cell around it."""
    return np.random.default_rng(seed).uniform(-0.5, 1.5, (ng, 3)) @ LATTICE


# off-mesh band k-points (fractions of the reciprocal vectors), one of them Gamma
BAND_FRAC = np.array([[0.0, 0.0, 0.0], [0.137, -0.291, 0.413], [-0.377, 0.219, 0.081]])
ON_MESH = (1, 1, 3)            # band mode at this mesh's k-points reproduces the k-mesh result

# kmesh: the k-mesh of fisdf_eval_ao, or None for fisdf_eval_ao_band with kband "off3" (three
# off-mesh points, Gamma first), "off1" (one off-mesh point) or "mesh" (the points of ON_MESH)
Raw = namedtuple("Raw", "name shells tn rcut ng kmesh kband")
RAW_CASES = [
    Raw("each_l_gamma", "each_l", "box", RCUT, 37, (1, 1, 1), None),
    Raw("each_l_222", "each_l", "box", RCUT, 37, (2, 2, 2), None),
    Raw("each_l_113", "each_l", "box", RCUT, 37, (1, 1, 3), None),
    Raw("mixed_112", "mixed", "box", RCUT, 29, (1, 1, 2), None),
    Raw("mixed_312", "mixed", "box", RCUT, 29, (3, 1, 2), None),
    Raw("shuffled_222", "mixed", "shuffled", RCUT, 29, (2, 2, 2), None),
    Raw("shuffled_113", "mixed", "shuffled", RCUT, 29, (1, 1, 3), None),
    Raw("neg_222", "mixed", "neg", RCUT, 29, (2, 2, 2), None),
    Raw("neg_312", "mixed", "neg", RCUT, 29, (3, 1, 2), None),
    Raw("masked_222", "mixed", "box", RCUT_MASKED, 29, (2, 2, 2), None),
    Raw("allmasked_312", "mixed", "box", RCUT_NONE, 29, (3, 1, 2), None),
    Raw("nT0_222", "mixed", "none", RCUT, 29, (2, 2, 2), None),
    Raw("nT0_113", "mixed", "none", RCUT, 29, (1, 1, 3), None),
    Raw("ng0_112", "mixed", "box", RCUT, 0, (1, 1, 2), None),
    Raw("ng1_113", "mixed", "box", RCUT, 1, (1, 1, 3), None),
    Raw("ng1_gamma", "mixed", "box", RCUT, 1, (1, 1, 1), None),
    Raw("t255_222", "mixed", "box", RCUT, 15, (2, 2, 2), None),        # 15 x 17 = 256 - 1
    Raw("t513_113", "spd", "box", RCUT, 57, (1, 1, 3), None),          # 57 x 9 = 2 x 256 + 1
    Raw("band_many_off3", "mixed", "box", RCUT, 29, None, "off3"),
    Raw("band_neg_off1", "each_l", "neg", RCUT, 37, None, "off1"),
    Raw("band_one_off3", "mixed", "one", RCUT, 29, None, "off3"),
    Raw("band_one_off1", "mixed", "one", RCUT, 29, None, "off1"),
    Raw("band_nT0_off3", "mixed", "none", RCUT, 29, None, "off3"),
    Raw("band_nT0_off1", "mixed", "none", RCUT, 29, None, "off1"),
    Raw("band_shuffled_mesh", "mixed", "shuffled", RCUT, 29, None, "mesh"),
    Raw("band_masked_off3", "mixed", "box", RCUT_MASKED, 29, None, "off3"),
    Raw("band_allmasked_off1", "mixed", "box", RCUT_NONE, 29, None, "off1"),
    Raw("band_ng0_off3", "mixed", "box", RCUT, 0, None, "off3"),
    Raw("band_ng1_off3", "mixed", "box", RCUT, 1, None, "off3"),
    Raw("band_t255_off3", "mixed", "box", RCUT, 15, None, "off3"),
    Raw("band_t513_off1", "spd", "neg", RCUT, 57, None, "off1"),
]
RAW_BY_NAME = {c.name: c for c in RAW_CASES}
BAND_MESH_PAIR = ("band_shuffled_mesh", "shuffled_113")    # the same tables and points


def case_id(c):
    return c.name


def band_kpts(kind, a=LATTICE):
    if kind == "mesh":
        return mesh_kpts(a, ON_MESH)
    fr = BAND_FRAC if kind == "off3" else BAND_FRAC[1:2]
    return fr @ reciprocal(a)


def expect_zero(c):
    """an output that must be exactly zero: no translation, or none in range."""
    return c.tn == "none" or c.rcut == RCUT_NONE


# what a test needs of a case: tables, points, kband (None: k-mesh), the long-double chi, the
# float64 restatement's per-column error, the longest sum
Data = namedtuple("Data", "tab coords kband ref err64 nsum F F_err64")   # F: the folded images


def _data(tab, coords, kmesh, kband):
    if kband is None:
        wide, f64 = kmesh_sum(tab, coords, kmesh, True), kmesh_sum(tab, coords, kmesh, False)
    else:
        wide, f64 = band_sum(tab, coords, kband, True), band_sum(tab, coords, kband, False)
    F, Fe = (None, None) if wide.F is None else (wide.F, col_err(f64.F, wide.F))
    return Data(tab, coords, kband, wide.chi, col_err(f64.chi, wide.chi), wide.nsum, F, Fe)


@functools.lru_cache(maxsize=None)
def raw_data(name):
    c = RAW_BY_NAME[name]
    tab = raw_tables(c.shells, c.tn, c.rcut)
    coords = raw_points(c.ng, seed=5 + c.ng)
    return _data(tab, coords, c.kmesh, None if c.kband is None else band_kpts(c.kband))


# ---- real-cell cases ---------------------------------------------------------------------------
# (cell builder of fisdf.cell, FFT mesh, points, k-mesh or None, band k-points): the wrap-around
# grid of the mesh, or a block of 40 random points
Real = namedtuple("Real", "name cell mesh points kmesh kband")
REAL_CASES = [
    Real("toy_grid_222", "toy_cell", (5, 5, 5), "grid", (2, 2, 2), None),
    Real("toy_rand_113", "toy_cell", (5, 5, 5), "random", (1, 1, 3), None),
    Real("toy_grid_band", "toy_cell", (5, 5, 5), "grid", None, "off3"),
    Real("diamond_grid_112", "diamond_cell", (4, 4, 4), "grid", (1, 1, 2), None),
    Real("diamond_rand_312", "diamond_cell", (4, 4, 4), "random", (3, 1, 2), None),
    Real("diamond_rand_band", "diamond_cell", (4, 4, 4), "random", None, "off3"),
    Real("nio_grid_222", "nio_cell", (3, 3, 3), "grid", (2, 2, 2), None),
    Real("nio_rand_gamma", "nio_cell", (3, 3, 3), "random", (1, 1, 1), None),
    Real("nio_grid_band", "nio_cell", (3, 3, 3), "grid", None, "off1"),
]
REAL_BY_NAME = {c.name: c for c in REAL_CASES}


@functools.lru_cache(maxsize=None)
def real_cell(name, mesh):
    from fisdf import cell as C
    return getattr(C, name)(mesh=mesh)


def real_points(c):
    cell = real_cell(c.cell, c.mesh)
    if c.points == "grid":
        return cell.gen_uniform_grids(cell.mesh)
    fr = np.random.default_rng(len(c.name)).uniform(-0.5, 0.5, (40, 3))
    return fr @ cell.lattice_vectors()


def real_tables(cell, coords):
    """the tables of a fisdf.cell.Cell as the wrappers hand them over, but the coefficients from
    the raw basis table normalised by radial_norm, not the ones stored in cell.shells."""
    from fisdf import cell as C
    raw = []
    for sym, _ in cell.atoms:
        key = (sym, cell.basis) if (sym, cell.basis) in C.BASIS else ("X", "toy")
        raw.extend(C.BASIS[key])
    assert len(raw) == len(cell.shells)
    cld = []
    for (l, exps, coefs), (ia, l2, e2, c2, ao0) in zip(raw, cell.shells):
        assert l == l2 and np.array_equal(np.asarray(exps, float), e2)
        cld.extend(radial_norm(l, exps, coefs))
    cld = np.asarray(cld, LD)
    return Tables(cell.atom_coords(), np.array([s[0] for s in cell.shells], np.int32),
                  np.array([s[1] for s in cell.shells], np.int32),
                  np.array([len(s[2]) for s in cell.shells], np.int32),
                  np.concatenate([s[2] for s in cell.shells]), cld.astype(float),
                  np.ascontiguousarray(C.lattice_translations(cell, coords), np.int32),
                  np.asarray(cell.lattice_vectors(), float), C.cell_rcut(cell), cld)


@functools.lru_cache(maxsize=None)
def real_data(name):
    c = REAL_BY_NAME[name]
    cell = real_cell(c.cell, c.mesh)
    coords = real_points(c)
    tab = real_tables(cell, coords)
    kband = None if c.kband is None else band_kpts(c.kband, tab.a)
    return _data(tab, coords, c.kmesh, kband)
