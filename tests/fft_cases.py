"""Case tables, a long-double reference and a restatement of the dispatch rule of fft3d()
(csrc/fft.hip) for tests/test_gpu_fft_variants.py.  No tests here: tests/test_fft_cases.py checks,
without a GPU, that the tables reach every route, kernel instantiation and named branch, that the
reference agrees with numpy's fftn and that the paired inputs have the Hermitian identity.

Conventions of every GPU case: entries N(0,1) + i N(0,1) (N(0,1) for real rows); input rows at
in_ld = ngrid + 5 in a NaN-filled buffer (rows a gather does not name stay NaN); output rows at
out_ld = ngrid + 3 in a buffer filled with the sentinel 7 + 7j, whose padding must come back
bitwise; the gather is ROWIDX out of ROWS_IN rows (non-monotone, one repeat); the error is
max |out - ref| / max |ref| over the compared region, weight included, below TOL.
"""
import os
from collections import namedtuple

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
PI = 4 * np.arctan(LD(1))          # pi to long-double precision (np.pi is a double)

TOL = 1e-14                        # the suite's FFT bound (test_fft3d, test_fft3d_paired)
SENTINEL = 7.0 + 7.0j
PAD_IN, PAD_OUT = 5, 3
ROWS_IN, ROWIDX = 6, (4, 0, 4)
KD = (0.83, -1.91, 2.6)
IN_LD_UNUSED = 7                   # in_ld of a sliced call: the plane table replaces it

# ---- the dispatch rule of fft3d(), restated ----------------------------------------------------
LISTED = (8, 12, 13, 15, 16, 18, 20, 24, 25, 27, 30, 32, 36, 40, 45, 48)
MAXN, MAXST = 64, 8
REG, REG_HERM, PLANE, AXES, BIG = 0, 1, 2, 3, 16
PLANE_LDS_MAX = 96 * 1024
AXIS_LDS_MAX = 160 * 1024


def factorize(n):
    """Radix list of a line length (4 first, then 2, 3, 5, 7, 11, 13), or None when the library
    has no transform for it."""
    if not 1 <= n <= MAXN:
        return None
    st = []
    for r in (4, 2, 3, 5, 7, 11, 13):
        while n % r == 0:
            st.append(r)
            n //= r
    return st if n == 1 and len(st) <= MAXST else None


def needs_big(n):
    """Whether a line length runs the radix-7/11/13 instantiation of the Stockham kernels."""
    return any(r > 5 for r in factorize(n))


def reg_mesh(mesh):
    n0, n1, n2 = mesh
    return n1 == n2 and n1 in LISTED and n0 in LISTED


def plane_lds(mesh):
    """Dynamic LDS of fft_plane_kernel: four 64-entry tables and two images of the plane."""
    return 16 * (256 + 2 * mesh[1] * mesh[2])


def reads_slices(mesh):
    return reg_mesh(mesh) or plane_lds(mesh) <= PLANE_LDS_MAX


def herm_enabled():
    return os.environ.get("FISDF_FFT_HERM", "1")[:1] != "0"


AxisGeom = namedtuple("AxisGeom", "n inner outer contiguous TL tiles_per_row lds")


def _largest_divisor_le(x, cap):
    return max(d for d in range(1, min(x, cap) + 1) if x % d == 0)


def axis_geom(mesh, axis):
    """Tiling of one fft_axis_kernel pass (axis_geom of fft.hip): TL lines of n points per
    workgroup; None when the library refuses the pass."""
    n = mesh[axis]
    if factorize(n) is None:
        return None
    inner = int(np.prod(mesh[axis + 1:], dtype=np.int64))
    outer = int(np.prod(mesh[:axis], dtype=np.int64))
    if axis == 2:
        TL = max(1, min(64, 2048 // n))
        tiles = -(-outer // TL)
    else:
        TL = _largest_divisor_le(inner, 64)
        if TL < 16 and inner > 64:
            TL = _largest_divisor_le(inner, 128)
        tiles = outer * (inner // TL)
    lds = 16 * (MAXN + 2 * TL * n)
    if lds > AXIS_LDS_MAX:
        return None
    return AxisGeom(n, inner, outer, axis == 2, TL, tiles, lds)


def herm_prefix(n, m):
    """Lines i <= their partner (-i - m) mod n are a prefix [0, nH): nH."""
    return max(i for i in range(n) if i <= (-i - m) % n) + 1


half_prefix_planes = herm_prefix   # linalg.hip: the same rule on axis 0


HermLines = namedtuple("HermLines", "n1H lo hi sl0 sl1 ok")


def herm_lines(n1, m1):
    """Line pairing of fft_axis0_herm: stored lines [lo, hi) pair with skipped lines, sl0 / sl1
    are their own partners (-1: none); ok: every paired line's partner was skipped."""
    m1 %= n1
    n1H = herm_prefix(n1, m1)
    partner = lambda j: (-j - m1) % n1
    sl0 = 0 if partner(0) == 0 else -1
    sl1 = n1H - 1 if n1H - 1 > 0 and partner(n1H - 1) == n1H - 1 else -1
    lo, hi = (1 if sl0 >= 0 else 0), (n1H - 1 if sl1 >= 0 else n1H)
    return HermLines(n1H, lo, hi, sl0, sl1, all(partner(j) >= n1H for j in range(lo, hi)))


def base_route(mesh, m=None):
    if reg_mesh(mesh):
        return REG_HERM if m is not None and m[0] in (0, 1) and herm_enabled() else REG
    return PLANE if plane_lds(mesh) <= PLANE_LDS_MAX else AXES


def kernels(mesh, m=None):
    """The kernels fft3d() launches, in order, as (name, template argument) pairs."""
    n0, n1, n2 = mesh
    r = base_route(mesh, m)
    if r == REG:
        return [("plane_reg", n1), ("axis0_reg", n0)]
    if r == REG_HERM:
        return [("plane_reg", n1), ("axis0_herm", (n0, m[0]))]
    if r == PLANE:
        return [("plane", needs_big(n1) or needs_big(n2)), ("axis", needs_big(n0))]
    return [("axis", needs_big(n2)), ("axis", needs_big(n1)), ("axis", needs_big(n0))]


def route(mesh, m=None):
    """What fisdf_fft3d_ex reports in *h_path."""
    r = base_route(mesh, m)
    if r in (PLANE, AXES) and any(needs_big(n) for n in mesh):
        r |= BIG
    return r


def accepted(mesh, m=None, in_real=False, sliced=False, inplace=False, gather=False):
    """Whether fft3d() takes the call (every refusal is a host-side check)."""
    if in_real and (not reg_mesh(mesh) or sliced or inplace):
        return False
    if inplace and gather:
        return False
    if sliced and not reads_slices(mesh):
        return False
    r = base_route(mesh, m)
    if r == REG:
        return True
    if r == REG_HERM:
        return herm_lines(mesh[1], m[1]).ok
    if any(factorize(n) is None for n in mesh):
        return False
    return all(axis_geom(mesh, a) is not None for a in ((0,) if r == PLANE else (0, 1, 2)))


# ---- the reference: separable DFT in long double -----------------------------------------------
def fftfreq_ld(n):
    """numpy.fft.fftfreq(n) in long double: i / n below (n + 1) // 2, (i - n) / n from there."""
    i = np.arange(n)
    return np.where(i < (n + 1) // 2, i, i - n).astype(LD) / LD(n)


def _expi(theta):
    out = np.empty(np.shape(theta), dtype=CLD)
    out.real, out.imag = np.cos(theta), np.sin(theta)
    return out


def dft_matrix(n):
    """W[k, j] = exp(-2 pi i j k / n) as clongdouble (the exponent reduced mod n as integers)."""
    k = np.arange(n)
    return _expi(-2 * PI * (np.outer(k, k) % n).astype(LD) / LD(n))


def phase(mesh, kd):
    """exp(-i f.kd) on the mesh, f the fftfreq fractions, formed in long double."""
    th = [-(fftfreq_ld(n) * LD(k)) for n, k in zip(mesh, kd)]
    return _expi(th[0][:, None, None] + th[1][None, :, None] + th[2][None, None, :])


def ref_fft3d(x, mesh, kd=None, weight=None):
    """Forward unnormalised 3-D DFT (numpy sign) of the rows of x (rows, ngrid), real or complex,
    after the phase, times the weight: one tensordot with a clongdouble DFT matrix per axis."""
    a = np.asarray(x).astype(CLD).reshape(-1, *mesh)
    if kd is not None:
        a = a * phase(mesh, kd)
    for ax in range(3):
        a = np.moveaxis(np.tensordot(dft_matrix(mesh[ax]), a, axes=([1], [ax + 1])), 0, ax + 1)
    a = a.reshape(a.shape[0], -1)
    if weight is not None:
        a = a * np.asarray(weight).astype(LD)
    return a


def rel_err(out, ref):
    """max |out - ref| / max |ref| with the difference taken in long double (an all-zero
    reference, the one-point mesh under weight[0] = 0, leaves the absolute difference)."""
    num, den = abs(np.asarray(out).astype(CLD) - ref).max(), abs(ref).max()
    return float(num / den) if den > 0 else float(num)


# ---- inputs --------------------------------------------------------------------------------------
def rnd(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def make_weight(rng, ngrid):
    """A Coulomb-like weight: [0, 2), weight[0] = 0 (the G = 0 term) and about 1 % exact zeros."""
    w = rng.uniform(0.0, 2.0, ngrid)
    w[rng.random(ngrid) < 0.01] = 0.0
    w[0] = 0.0
    return w


def slice_planes(n0):
    """Plane counts of the 3 input slices of a sliced case (unequal, every plane once)."""
    a = max(1, n0 // 5)
    b = max(1, (n0 - a) // 2 + 1)
    assert n0 - a - b >= 1 and len({a, b, n0 - a - b}) == 3, n0
    return (a, b, n0 - a - b)


SLICE_PAD, SLICE_GAP = (2, 0, 4), 9


def slice_layout(mesh, rows_in):
    """Sliced input as the all-to-all pieces of a k-sharded build arrive (plane_table, api.hip):
    slice p holds its planes of every row, rows at its own ld; here the ld is padded and a gap
    lies between the slices.  Returns (plane base (n0), plane ld (n0), buffer size)."""
    n0, P = mesh[0], mesh[1] * mesh[2]
    base, ld, off, i0 = [], [], 0, 0
    for cnt, pad in zip(slice_planes(n0), SLICE_PAD):
        ldp = cnt * P + pad
        for j in range(cnt):
            base.append(off + j * P)
            ld.append(ldp)
        off += rows_in * ldp + SLICE_GAP
        i0 += cnt
    return np.array(base, dtype=np.int64), np.array(ld, dtype=np.int64), off


# ---- case tables -----------------------------------------------------------------------------------
# gather: rows ROWIDX of ROWS_IN; kd: None or 3 floats; weight / inplace / sliced: flags
Case = namedtuple("Case", "mesh rows gather kd weight inplace sliced")


def plain(mesh, rows=3):
    return Case(tuple(mesh), rows, False, None, False, False, False)


def every(mesh, rows=3):
    """rowidx + kd + weight together (the strides are padded in every case)."""
    return Case(tuple(mesh), rows, True, KD, True, False, False)


def cid(c):
    s = "x".join(map(str, c.mesh))
    for flag, tag in ((c.gather, "g"), (c.kd is not None, "k"), (c.weight, "w"), (c.inplace, "i"),
                      (c.sliced, "s")):
        if flag:
            s += "-" + tag
    return s


def _both(meshes):
    return [f(m) for m in meshes for f in (plain, every)]


# 1. register kernels: every listed size as a plane size and as an axis-0 size, mixed meshes
REG_MESHES = ([(8, N, N) for N in LISTED] + [(N, 8, 8) for N in LISTED if N != 8]
              + [(13, 16, 16), (12, 15, 15), (45, 12, 12)])
GROUP_REG = _both(REG_MESHES)

# 2. LDS plane kernel + axis-0 Stockham pass
LDS_SMALL = [(6, 10, 10), (8, 12, 16), (12, 9, 20), (7, 12, 12), (1, 12, 12), (8, 1, 8), (1, 1, 1)]
LDS_TAIL = [(3, 48, 60), (4, 50, 50)]             # planes above 2048 points: the tail load loop
LDS_BIG = [(6, 10, 14), (5, 7, 11), (4, 13, 26), (14, 16, 16)]
LDS_TILES = [(7, 13, 13), (9, 7, 11), (64, 7, 11)]  # axis-0 tile: TL 13; TL widened to 77; largest
GROUP_LDS = _both(LDS_SMALL + LDS_TAIL + LDS_BIG + LDS_TILES)

# 3. three axis passes (a plane beyond 96 KB)
# (7, 56, 56): the radix-7 instantiation in the strided axis-0 pass as well
AXES_MESHES = [(3, 56, 56), (2, 64, 48), (3, 50, 64), (2, 56, 55), (7, 56, 56)]
GROUP_AXES = [f(m, 2) for m in AXES_MESHES for f in (plain, every)]

# 4. each option alone and all together on every route, kd on an even and an odd mesh per route
OPTION_MESHES = {REG: [(8, 12, 12), (13, 15, 15)], PLANE: [(6, 10, 10), (5, 9, 15)],
                 AXES: [(2, 64, 48), (3, 55, 55)]}


def _options(mesh, rows):
    m = tuple(mesh)
    return [Case(m, rows, False, KD, False, False, False),
            Case(m, rows, False, None, True, False, False),
            Case(m, rows, True, None, False, False, False),
            Case(m, rows, False, None, False, True, False),
            Case(m, rows, True, KD, True, False, False),
            Case(m, rows, False, KD, True, True, False)]


GROUP_OPTIONS = [c for r, ms in OPTION_MESHES.items() for m in ms
                 for c in _options(m, 2 if r == AXES else 3)]

# 5. sliced input through a plane table, alone, with the gather, with everything
SLICED_MESHES = [(8, 12, 12), (13, 16, 16), (6, 10, 10), (6, 10, 14), (6, 50, 50)]
GROUP_SLICED = [Case(tuple(m), 3, g, kd, w, False, True) for m in SLICED_MESHES
                for (g, kd, w) in ((False, None, False), (True, None, False), (True, KD, True))]

# 6. Hermitian pairing: real rows times exp(-i f.kd), kd = pi m, every m in {0,1}^3
HERM_MESHES = [(8, 12, 12), (13, 16, 16), (15, 15, 15), (12, 13, 13), (16, 8, 8)]
HERM_M = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
GROUP_HERM = [(m, h) for m in HERM_MESHES for h in HERM_M]
# in_real, gather, weight, sliced: what each (mesh, m) runs on one reference
HermVariant = namedtuple("HermVariant", "in_real gather weight sliced")
HERM_VARIANTS = [HermVariant(0, 0, 0, 0), HermVariant(1, 0, 0, 0), HermVariant(0, 0, 1, 0),
                 HermVariant(1, 0, 1, 0), HermVariant(0, 1, 1, 0), HermVariant(1, 1, 0, 0),
                 HermVariant(0, 0, 0, 1), HermVariant(0, 1, 1, 1)]
# m on a mesh without register kernels: the full transform is written
HERM_FULL = [((6, 10, 10), (1, 0, 1)), ((5, 7, 11), (1, 1, 1)), ((3, 56, 56), (0, 1, 1))]

# 7. calls the library refuses (before it launches anything): keyword arguments of accepted()
Reject = namedtuple("Reject", "name mesh m in_real sliced inplace gather")
GROUP_REJECT = [
    Reject("dim17-axis0", (17, 8, 8), None, 0, 0, 0, 0),
    Reject("dim17-axis1", (8, 17, 8), None, 0, 0, 0, 0),
    Reject("dim17-axis2", (8, 8, 17), None, 0, 0, 0, 0),
    Reject("dim17-axes-route", (17, 56, 56), None, 0, 0, 0, 0),
    Reject("dim65-axis0", (65, 8, 8), None, 0, 0, 0, 0),
    Reject("dim65-axis1", (8, 65, 8), None, 0, 0, 0, 0),
    Reject("dim65-axis2", (8, 8, 65), None, 0, 0, 0, 0),
    Reject("tile-91x64", (64, 7, 13), None, 0, 0, 0, 0),
    Reject("real-nonreg", (6, 10, 10), None, 1, 0, 0, 0),
    Reject("real-nonreg-m", (6, 10, 10), (0, 0, 0), 1, 0, 0, 0),
    Reject("real-sliced", (8, 12, 12), (0, 0, 0), 1, 1, 0, 0),
    Reject("real-inplace", (8, 12, 12), (0, 0, 0), 1, 0, 1, 0),
    Reject("inplace-gather", (8, 12, 12), None, 0, 0, 1, 1),
    Reject("inplace-gather-lds", (6, 10, 10), None, 0, 0, 1, 1),
    Reject("sliced-axes-route", (3, 56, 56), None, 0, 1, 0, 0),
    Reject("line-pairing-m1-3", (8, 12, 12), (0, 3, 0), 0, 0, 0, 0),
]

GROUPS = {"1-reg": GROUP_REG, "2-lds": GROUP_LDS, "3-axes": GROUP_AXES, "4-options": GROUP_OPTIONS,
          "5-sliced": GROUP_SLICED}


def all_cases():
    return [c for g in GROUPS.values() for c in g]
