"""Cases and references for the device functional and the fused RKS block: fisdf_xc_eval and
fisdf_nr_rks_block (csrc/func.hip, api.hip), fisdf.xc, ISDF.eval_xc and ISDF.nr_rks.  No tests and
no GPU here: tests/test_func_cases.py checks this file on the CPU, tests/test_gpu_nr_rks.py runs
the device against it.

The functional (atomic units, spin-unpolarised; n the density, sigma = |grad n|^2):
    e_x^LDA = -(3/4)(3/pi)^(1/3) n^(4/3),  rs = (3/(4 pi n))^(1/3)
    PW92 ("pw_mod"): A = (1 - ln 2)/pi^2, a1 = 0.21370, b1..b4 = 7.5957, 3.5876, 1.6382, 0.49294
    eps = -2A(1 + a1 rs) ln(1 + 1/(2A(b1 rs^(1/2) + b2 rs + b3 rs^(3/2) + b4 rs^2)))
    PBE: kappa = 0.804, beta = 0.06672455060314922, gamma = A, mu = beta pi^2/3
    kF = (3 pi^2 n)^(1/3), s^2 = sigma/(4 kF^2 n^2), F_x = 1 + kappa - kappa/(1 + mu s^2/kappa)
    ks^2 = 4 kF/pi, t^2 = sigma/(4 ks^2 n^2), A' = (beta/gamma)/(exp(-eps/gamma) - 1)
    H = gamma ln(1 + (beta/gamma) t^2 (1 + A' t^2)/(1 + A' t^2 + A'^2 t^4)), e_c = n (eps + H)
``naive_energy`` is that text, literally, in long double.  ``parts`` is the reference proper: the
energy and its analytic derivatives, exchange and correlation separately, with the correlation
written as eps + H = gamma log1p(-q/D), q = -expm1(eps/gamma), D = 1 + y + y^2, y = A' t^2 (the
two logarithms combined; nothing cancels at large t^2), or, where q/D > 1/2, as
gamma (log(D - q) - log(D)) with D - q = y + y^2 + exp(eps/gamma).  ``parts(..., dt=np.float64)``
is the same code in float64: it measures what float64 arithmetic alone costs at the points of a
case.

Error scale of an output at a point: |cx exchange part| + |cc correlation part| of that output,
times 2 |d_c n| for wv[1:4].  A device value may be factor_cases.bound(err64, 1) times that scale
from the long-double reference, err64 the float64 restatement's largest scaled error over the
case: 16 times what float64 itself costs, floored at eps.
"""
import functools
from collections import namedtuple

import numpy as np

import fft_cases as F
import xc_cases as X
from factor_cases import CLD, EPS, LD, bound  # noqa: F401

LDA, GGA = 0, 1
RHO_CUT = 1e-15
XC_THREADS = 256       # points per workgroup of the functional kernel (one per thread)

KAPPA = "0.804"
BETA = "0.06672455060314922"
PW = ("0.21370", "7.5957", "3.5876", "1.6382", "0.49294")


def _c(dt):
    """The constants in dt."""
    pi = dt(4) * np.arctan(dt(1))
    A = (dt(1) - np.log(dt(2))) / (pi * pi)
    beta = dt(LD(BETA))
    return dict(pi=pi, A=A, gamma=A, beta=beta, kappa=dt(LD(KAPPA)), mu=beta * pi * pi / dt(3),
                a1=dt(LD(PW[0])), b=[dt(LD(x)) for x in PW[1:]],
                cx=dt(3) / dt(4) * np.cbrt(dt(3) / pi), rs0=np.cbrt(dt(3) / (dt(4) * pi)),
                kf0=np.cbrt(dt(3) * pi * pi))


def eps_unif(rs, dt=LD):
    """(eps_c^unif, d eps / d rs)."""
    k = _c(dt)
    rs = np.asarray(rs, dt)
    sr = np.sqrt(rs)
    b1, b2, b3, b4 = k["b"]
    q0 = -2 * k["A"] * (1 + k["a1"] * rs)
    q1 = 2 * k["A"] * (b1 * sr + b2 * rs + b3 * rs * sr + b4 * rs * rs)
    dq1 = k["A"] * (b1 / sr + 2 * b2 + 3 * b3 * sr + 4 * b4 * rs)
    lg = np.log1p(1 / q1)
    return q0 * lg, -2 * k["A"] * k["a1"] * lg - q0 * dq1 / (q1 * q1 + q1)


def naive_energy(family, n, sigma):
    """(e_x, e_c) in long double, the formulas of the module text as they stand."""
    k = _c(LD)
    n, sigma = np.asarray(n, LD), np.asarray(sigma, LD)
    ex = -k["cx"] * n ** (LD(4) / 3)
    rs = (3 / (4 * k["pi"] * n)) ** (LD(1) / 3)
    b1, b2, b3, b4 = k["b"]
    eps = -2 * k["A"] * (1 + k["a1"] * rs) * np.log(
        1 + 1 / (2 * k["A"] * (b1 * rs ** LD(0.5) + b2 * rs + b3 * rs ** LD(1.5) + b4 * rs ** 2)))
    if family == LDA:
        return ex, n * eps
    kf = (3 * k["pi"] ** 2 * n) ** (LD(1) / 3)
    s2 = sigma / (4 * kf ** 2 * n ** 2)
    fx = 1 + k["kappa"] - k["kappa"] / (1 + k["mu"] * s2 / k["kappa"])
    t2 = sigma / (4 * (4 * kf / k["pi"]) * n ** 2)
    Ap = (k["beta"] / k["gamma"]) / (np.exp(-eps / k["gamma"]) - 1)
    H = k["gamma"] * np.log(1 + (k["beta"] / k["gamma"]) * t2 * (1 + Ap * t2)
                            / (1 + Ap * t2 + Ap ** 2 * t2 ** 2))
    return ex * fx, n * (eps + H)


Parts = namedtuple("Parts", "ex ec vnx vnc vsx vsc fx w")


def parts(family, n, sigma, dt=LD):
    """e, de/dn and de/dsigma of the exchange and of the correlation part at n > 0 (arrays), with
    F_x and eps + H (LDA: 1 and eps) for the limit checks."""
    k = _c(dt)
    n, sigma = np.asarray(n, dt), np.asarray(sigma, dt)
    c = np.cbrt(n)
    exl, dexl = -k["cx"] * n * c, -(dt(4) / 3) * k["cx"] * c
    rs = k["rs0"] / c
    eps, deps = eps_unif(rs, dt)
    neps = -(rs / 3) * deps
    zero = np.zeros_like(n)
    if family == LDA:
        return Parts(exl, n * eps, dexl, eps + neps, zero, zero, zero + 1, eps)
    kf = k["kf0"] * c
    cs = 1 / (4 * kf * kf * n * n)
    s2 = sigma * cs
    den = 1 + (k["mu"] / k["kappa"]) * s2
    fx = 1 + k["mu"] * s2 / den
    dfx = k["mu"] / (den * den)
    nct = k["pi"] / (16 * kf * n)
    t2 = sigma * (nct / n)
    q, p = -np.expm1(eps / k["gamma"]), np.exp(eps / k["gamma"])
    bg = k["beta"] / k["gamma"]
    A = bg * p / q
    dA = A * A / (k["beta"] * p)
    y = A * t2
    yy = y + y * y
    D = 1 + yy
    u, r = 1 / D, 1 / (yy + p)
    # q / D <= 1/2: log1p of it; else (high density, small y) the two logarithms apart, which is
    # log(p) = eps / gamma at y = 0 and cancels nothing while their difference is below log(1/2)
    z = q * u
    W = k["gamma"] * np.where(z <= 0.5, np.log1p(-np.minimum(z, 0.5)), np.log(yy + p) - np.log1p(yy))
    We = p * r
    Wy = k["gamma"] * q * ((1 + 2 * y) * u) * r
    return Parts(exl * fx, n * W, dexl * (fx - 2 * s2 * dfx),
                 W + We * neps + Wy * (t2 * dA * neps - (dt(7) / 3) * y),
                 exl * dfx * cs, nct * A * Wy, fx, W)


Func = namedtuple("Func", "e wv se sw")


def func_ref(family, cx, cc, cut, rho, dt=LD):
    """The kernel's outputs from rho (nset, 4, ng) real (LDA: (nset, ng)): e (nset, ng),
    wv (nset, 4 or 1, ng), and their error scales se, sw.  Points with n <= cut give zeros."""
    rho = np.asarray(rho, np.float64)
    if family == LDA:
        rho = rho[:, None]
    ncomp = 4 if family == GGA else 1
    n = rho[:, 0]
    live = n > cut
    nl = np.where(live, n, 1.0).astype(dt)
    g = rho[:, 1:].astype(dt)
    sigma = (g * g).sum(axis=1) if family == GGA else np.zeros_like(nl)
    P = parts(family, nl, sigma, dt)
    cx, cc = dt(cx), dt(cc)
    z = lambda a: np.where(live, a, dt(0))      # noqa: E731
    e, se = z(cx * P.ex + cc * P.ec), z(abs(cx * P.ex) + abs(cc * P.ec))
    wv = np.zeros((rho.shape[0], ncomp, rho.shape[2]), dt)
    sw = np.zeros_like(wv)
    wv[:, 0], sw[:, 0] = z(cx * P.vnx + cc * P.vnc), z(abs(cx * P.vnx) + abs(cc * P.vnc))
    if family == GGA:
        vs, ss = z(cx * P.vsx + cc * P.vsc), z(abs(cx * P.vsx) + abs(cc * P.vsc))
        wv[:, 1:] = 2 * vs[:, None] * g
        sw[:, 1:] = 2 * ss[:, None] * abs(g)
    return Func(e, wv, se, sw)


def scaled_err(x, ref, scale):
    """max |x - ref| / scale over the entries with scale > 0; an entry with scale 0 must be exactly
    0 in x (the reference is)."""
    x, ref, scale = np.asarray(x), np.asarray(ref), np.asarray(scale)
    dead = scale == 0
    assert not np.asarray(x)[dead].any(), "an output with zero scale is not exactly 0"
    if dead.all():
        return 0.0
    d = np.abs(x.astype(LD) - ref.astype(LD))[~dead] / scale[~dead].astype(LD)
    assert np.isfinite(d).all(), "a non-finite output"
    return float(d.max())


# ---- the point table ---------------------------------------------------------------------------
SPOT_EPS = [(1, "-0.05977368037840"), (2, "-0.04475949452353"), (5, "-0.02821623242871")]
# (n, sigma): e_x^PBE, e_c^PBE, e^LDA
SPOTS = [((0.1, 0.02), "-3.599231070380e-02", "-3.906133616133e-03", "-3.960595149945e-02"),
         ((1.0, 3.0), "-7.509973005640e-01", "-6.056602525347e-02", "-8.097588174955e-01"),
         ((1e-3, 1e-6), "-9.857529291179e-05", "-5.623857151898e-06", "-9.879195757772e-05"),
         ((2.5, 0.0), "-2.505946157947e+00", "-1.972928325928e-01", "-2.703238990540e+00")]
N_RANGE, G_RANGE = (-14.0, 3.0), (-12.0, 4.0)       # log10 of n and of |grad n|
S2_LARGE = (1e-3, 1e3)          # (n, |grad n|) with s^2 = 2.6e12


def special_points(cut):
    """(name, n, |grad n|) of the points every table with room for them starts with."""
    out = [("at_cut", cut, 1e-3), ("ulp_above_cut", np.nextafter(cut, np.inf), 1e-3),
           ("ulp_below_cut", np.nextafter(cut, -np.inf), 1e-3), ("n_zero", 0.0, 1e-3),
           ("n_negative", -0.3, 0.5), ("sigma_zero", 0.7, 0.0),
           ("s2_large", S2_LARGE[0], S2_LARGE[1])]
    out += [("spot%d" % i, s[0][0], float(np.sqrt(s[0][1]))) for i, s in enumerate(SPOTS)]
    return out


def point_table(ng, nset, cut=RHO_CUT, seed=0):
    """rho (nset, 4, ng) float64: n log-uniform in [1e-14, 1e3], |grad n| zero for one point in
    eight and log-uniform in [1e-12, 1e4] otherwise, its direction random; the special points
    first in every set where ng has room for them (the spot rows' sigma is the square of a rounded
    root: they are there as points, the CPU test checks their values from (n, sigma) directly)."""
    rng = np.random.default_rng(4000 + 17 * ng + nset + seed)
    n = 10.0 ** rng.uniform(*N_RANGE, (nset, ng))
    gn = 10.0 ** rng.uniform(*G_RANGE, (nset, ng))
    gn[rng.random((nset, ng)) < 0.125] = 0.0
    sp = special_points(cut)
    if ng >= len(sp):
        for i, (_, a, b) in enumerate(sp):
            n[:, i], gn[:, i] = a, b
    d = rng.standard_normal((nset, 3, ng))
    d /= np.sqrt((d * d).sum(axis=1, keepdims=True))
    rho = np.empty((nset, 4, ng))
    rho[:, 0] = n
    rho[:, 1:] = d * gn[:, None]
    return rho


def table_branches(rho, cut=RHO_CUT):
    """What a table reaches."""
    n = rho[:, 0]
    sigma = (rho[:, 1:].astype(LD) ** 2).sum(axis=1)
    out = set()
    if (n == cut).any():
        out.add("at_cut")
    if (n == np.nextafter(cut, np.inf)).any():
        out.add("ulp_above_cut")
    if (n == np.nextafter(cut, -np.inf)).any():
        out.add("ulp_below_cut")
    if (n == 0).any():
        out.add("n_zero")
    if (n < 0).any():
        out.add("n_negative")
    live = n > cut
    if (live & (sigma == 0)).any():
        out.add("sigma_zero")
    k = _c(LD)
    nl = np.where(live, n, 1.0).astype(LD)
    s2 = sigma / (4 * (k["kf0"] * np.cbrt(nl)) ** 2 * nl * nl)
    if (live & (s2 > 1e6)).any():
        out.add("s2_large")
    ng = rho.shape[2]
    out.add("one_workgroup" if ng <= XC_THREADS else "many_workgroups")
    out.add("workgroup_partial" if ng % XC_THREADS else "workgroup_full")
    return out


TABLE_BRANCHES = {"at_cut", "ulp_above_cut", "ulp_below_cut", "n_zero", "n_negative", "sigma_zero",
                  "s2_large", "one_workgroup", "many_workgroups", "workgroup_partial",
                  "workgroup_full"}

# ---- fisdf_xc_eval cases -------------------------------------------------------------------------
XcCase = namedtuple("XcCase", "family cx cc ng nset")
MIXES = [(1.0, 1.0), (0.75, 1.0), (1.0, 0.0), (0.0, 1.0)]
NGS = [1, 255, 256, 257, 1000]
XC_CASES = [XcCase(fam, cx, cc, ng, nset)
            for fam in (LDA, GGA) for ng in NGS for nset in (1, 3) for cx, cc in MIXES]
EPAD = 9           # extra elements between the sets of e
SPAD = 13          # extra elements between the sets of rho and of wv, beyond the components


def xc_id(c):
    return "%s-cx%g-cc%g-g%d-s%d" % ("gga" if c.family else "lda", c.cx, c.cc, c.ng, c.nset)


@functools.lru_cache(maxsize=None)
def xc_table(ng, nset):
    t = point_table(ng, nset)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def xc_data(c):
    """rho as the entry takes it ((nset, 4, ng), LDA (nset, ng)), the long-double reference and
    the float64 restatement's scaled errors (e, wv)."""
    rho = xc_table(c.ng, c.nset)
    rho = rho if c.family == GGA else rho[:, 0]
    ref = func_ref(c.family, c.cx, c.cc, RHO_CUT, rho, LD)
    f64 = func_ref(c.family, c.cx, c.cc, RHO_CUT, rho, np.float64)
    return rho, ref, (scaled_err(f64.e, ref.e, ref.se), scaled_err(f64.wv, ref.wv, ref.sw))


# ---- fused block cases ---------------------------------------------------------------------------
BlockCase = namedtuple("BlockCase", "nao ng nk nset acc")
BLOCK_CASES = [BlockCase(1, 1, 1, 1, 0), BlockCase(8, 65, 2, 3, 1), BlockCase(26, 997, 2, 4, 0),
               BlockCase(33, 65, 1, 5, 1), BlockCase(8, 2049, 1, 1, 0)]
BLOCK_SCALE = 0.37
BLOCK_MIX = (0.75, 1.0)


def block_id(c):
    return "nao%d-g%d-k%d-s%d-acc%d" % c


@functools.lru_cache(maxsize=None)
def block_inputs(c):
    """f4 (nk, 4, ng, nao), Hermitian D (nset, nk, nao, nao) = B B^H + I scaled to order one (the
    density f D f^H is then at least |f|^2 > 0 at every point), the Hermitian start of vxc
    (nset, nk, nao, nao) and the start of the sums (nset, 2)."""
    rng = np.random.default_rng(5000 * c.nao + c.ng + 7 * c.nk + c.nset)
    f4 = F.rnd(rng, c.nk, 4, c.ng, c.nao)
    B = F.rnd(rng, c.nset, c.nk, c.nao, c.nao)
    D = (B @ B.conj().swapaxes(-1, -2)) / c.nao + np.eye(c.nao)
    D = (D + D.conj().swapaxes(-1, -2)) / 2
    P = F.rnd(rng, c.nset, c.nk, c.nao, c.nao)
    return f4, D, P + P.conj().swapaxes(-1, -2), rng.standard_normal((c.nset, 2))


BlockRef = namedtuple("BlockRef", "rho vxc sums")


def block_pipeline(f4, D, family, cx, cc, cut, scale, wide=True):
    """rho (nset, 4, ng) real, V (nset, nk, nao, nao) and scale (sum n, sum e) (nset, 2) of the
    pipeline xc_cases.rho_gga_ref -> the functional -> xc_cases.gga_gram_ref / lda_gram_ref, in long
    double or, wide=False, in float64."""
    dt = LD if wide else np.float64
    rho = X.rho_gga_ref(f4, D, 1, wide).real
    if family == GGA:
        fr = _func_wide(GGA, cx, cc, cut, rho, dt)
        V = X.gga_gram_ref(f4, fr.wv, scale, wide)
    else:
        fr = _func_wide(LDA, cx, cc, cut, rho[:, 0], dt)
        V = X.lda_gram_ref(f4, fr.wv[:, 0], scale, wide)
    live = rho[:, 0] > cut
    sums = np.stack([np.where(live, rho[:, 0], 0).sum(axis=1), fr.e.sum(axis=1)], axis=1) * dt(scale)
    return BlockRef(rho, V, sums)


def _func_wide(family, cx, cc, cut, rho, dt):
    """func_ref on a density that is itself in dt (func_ref rounds its input to float64, which the
    device's input is; inside the pipeline the density keeps the pipeline's precision)."""
    rho = np.asarray(rho, dt)
    if family == LDA:
        rho = rho[:, None]
    n, g = rho[:, 0], rho[:, 1:]
    live = n > cut
    nl = np.where(live, n, dt(1))
    sigma = (g * g).sum(axis=1) if family == GGA else np.zeros_like(nl)
    P = parts(family, nl, sigma, dt)
    z = lambda a: np.where(live, a, dt(0))      # noqa: E731
    wv = np.zeros((rho.shape[0], 4 if family == GGA else 1, rho.shape[2]), dt)
    wv[:, 0] = z(dt(cx) * P.vnx + dt(cc) * P.vnc)
    if family == GGA:
        wv[:, 1:] = 2 * z(dt(cx) * P.vsx + dt(cc) * P.vsc)[:, None] * g
    return Func(z(dt(cx) * P.ex + dt(cc) * P.ec), wv, None, None)


@functools.lru_cache(maxsize=None)
def block_ref(c):
    f4, D, P, S0 = block_inputs(c)
    cx, cc = BLOCK_MIX
    w = block_pipeline(f4, D, GGA, cx, cc, RHO_CUT, BLOCK_SCALE, True)
    d = block_pipeline(f4, D, GGA, cx, cc, RHO_CUT, BLOCK_SCALE, False)
    return w, d


# ---- end to end ------------------------------------------------------------------------------------
E2E_XC = {"lda": (LDA, 1.0, 1.0), "pbe": (GGA, 1.0, 1.0), "pbe0": (GGA, 0.75, 1.0)}


E2E_TWO_SETS = ("toy_222", "toy_113")    # cells whose two-set matrices keep every point above the cut
TIE_CASES = ("toy_222", "toy_113")


def e2e_dm(name, nset=1):
    """xc_cases.e2e_dms of a cell, (nset, nk, nao, nao).  With one set the smallest density on the
    grid is 0.116 (toy_222), 0.028 (toy_113), 1.05e-3 (diamond_112); the second of two sets goes
    negative at a point of the diamond cell, so two sets are for the toy cells only."""
    c, d = X.E2E_BY_NAME[name], X.e2e_data(name)
    return X.e2e_dms(d.cell, c.kmesh, nset)


def tie_matrices(name):
    """The one-set D of a cell and a Hermitian perturbation on the 2^-20 grid (D + d, D - d and
    the halved perturbation are exact in float64)."""
    c, d = X.E2E_BY_NAME[name], X.e2e_data(name)
    D = e2e_dm(name)[0]
    rng = np.random.default_rng(9)
    dl = X.quantize(F.rnd(rng, *D.shape) * 0.02)
    return D, dl + dl.conj().swapaxes(-1, -2)


@functools.lru_cache(maxsize=None)
def e2e_ref(name, xc, nset=1):
    """The long-double and the float64 pipeline on the cell's whole grid with e2e_dm."""
    c, d = X.E2E_BY_NAME[name], X.e2e_data(name)
    D = e2e_dm(name, nset)
    fam, cx, cc = E2E_XC[xc]
    ngrid = len(d.coords)
    w = block_pipeline(d.f4, D, fam, cx, cc, RHO_CUT, LD(d.cell.vol) / ngrid, True)
    f = block_pipeline(d.f4_64, D, fam, cx, cc, RHO_CUT, d.cell.vol / ngrid, False)
    return w, f


# ---- the arena of the fused block, restated ------------------------------------------------------
def arena_plan(nk, ng, nao, nset):
    """(bytes per point, fixed bytes) of fisdf_nr_rks_plan: per point and set 64 B of rho, 32 B of
    wv and 8 B of e, and the gram's aow row; fixed the gram's matrix and split-K partials, the
    workgroup sums and 256 B of alignment for each of the seven pieces."""
    ks = X.gram_ksplit(ng)
    nm = nk * nao * nao
    split = ks * nm if ks > 1 else 0
    nblk = (ng + XC_THREADS - 1) // XC_THREADS
    return 104 * nset + 16 * nk * nao, 16 * (nm + split) + 16 * nset * nblk + 256 * 7
