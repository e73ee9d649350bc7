"""Case tables, fp64 references and a restatement of the dispatch rule of zgemm() / herk()
(csrc/zgemm.hip, csrc/zgemm_wide.hip) for tests/test_gpu_gemm_variants.py.  No tests here:
tests/test_gemm_cases.py checks, without a GPU, that the tables reach every loop variant the
dispatch can choose and that the references agree with a longdouble einsum.

Conventions of every GPU case: entries N(0,1) + i N(0,1); |alpha|, |beta| <= 1; padded leading
dimensions and batch strides with a gap (lda = cols + 3, ldb = cols + 5, ldc = N + 7, stride =
rows * ld + 11); NaN in the padding of A and B, the sentinel 7 + 7j in the padding of C; with
beta = 0 the logical part of C starts as NaN (beta = 0 means C is not read).
"""
from collections import namedtuple

import numpy as np

# op codes (common.h Op): bit 0 transpose, bit 1 conjugate
OP_N, OP_T, OP_R, OP_C = 0, 1, 2, 3
OPS = [(a, b) for a in range(4) for b in range(4)]
# GemmMode bits / Epi codes of common.h
A_REAL, RE_ONLY, A_LOWER, A_UPPER = 1, 2, 4, 8
EPI_NONE, EPI_STREAM, EPI_CSQUARE, EPI_REAL, EPI_WSRHO = 0, 2, 4, 5, 6

BK = 8          # complex K elements per K-step
RING = 3        # LDS ring depth of the long-K loops
ALPHA = 0.7 - 0.3j
BETA = 0.2 + 0.5j
SENTINEL = 7.0 + 7.0j
PAD_A, PAD_B, PAD_C, GAP = 3, 5, 7, 11


def tol_abs(K):
    """The suite's GEMM bound (test_gpu_kernels.py): max |out - ref| < 1e-12 max(K, 16)."""
    return 1e-12 * max(K, 16)


TOL_REL = 1e-12  # squared / real / scaled epilogues: max |out - ref| / max |ref|


# ---- the dispatch rule, restated -------------------------------------------------------------
def supported(opA, opB, mode):
    """Which (opA, opB, mode) zgemm() accepts; every accepted one must launch a kernel."""
    if mode == 0:
        return True
    if mode in (1, 2, 3):
        return (opA, opB) in ((OP_N, OP_N), (OP_C, OP_N))
    if mode in (4, 5):
        return (opA, opB) == (OP_N, OP_N)
    if mode == 8:
        return (opA, opB) in ((OP_C, OP_N), (OP_C, OP_C))
    return False


def kchunk_of(K, ks):
    """K range of one split: ceil(K / ks) rounded up to whole K-steps (at least one)."""
    per_split = -(-K // max(ks, 1))
    return max(BK, -(-per_split // BK) * BK)


def splits_of(K, ks):
    """The K-steps each split runs (the last one may be short)."""
    kc = kchunk_of(K, ks)
    n = max(1, -(-K // kc))
    return [-(-(min(K, (s + 1) * kc) - s * kc) // BK) for s in range(n)]


def gemm_path(opA, opB, M, N, K, batch=1, ks=1, mode=0, epi=EPI_NONE):
    """Which loop zgemm() launches: 'wide' (64 x 128 tile), 'ring2' (2-deep ring, K-chunk <= 4
    K-steps), 'pipe' (software-pipelined 3-multiplication loop) or 'plain' (ring-3)."""
    ks = 1 if epi != EPI_NONE else max(ks, 1)
    if ((opA, opB) == (OP_N, OP_N) and batch == 1 and ks <= 1 and epi == EPI_NONE and K % BK == 0
            and N >= 512 and (mode & ~(A_REAL | A_LOWER)) == 0):
        return "wide"
    if kchunk_of(K, ks) <= 4 * BK:
        return "ring2"
    if mode in (0, A_LOWER, A_UPPER) and K % BK == 0:
        return "pipe"
    return "plain"


def herk_path(n, K, ks=1, mode=0):
    """The same for herk() / herk_batched() (never wide)."""
    if kchunk_of(K, ks) <= 4 * BK:
        return "ring2"
    if mode == 0 and K % BK == 0:
        return "pipe"
    return "plain"


def mode_paths(mode):
    """The loops a mode can land in on the 64 x 64 kernel."""
    return ("ring2", "pipe", "plain") if mode in (0, A_LOWER, A_UPPER) else ("ring2", "plain")


# ---- references (complex128 / float64 NumPy) --------------------------------------------------
def opmat(a, op):
    if op & 1:
        a = a.swapaxes(-1, -2)
    if op & 2:
        a = a.conj()
    return a


def ref_acc(A, B, opA, opB, mode=0):
    """op(A) op(B) as the mode defines it: A_REAL drops Im op(A), A_LOWER / A_UPPER take the
    triangle of op(A), RE_ONLY keeps the real part of the product."""
    a, b = opmat(A, opA), opmat(B, opB)
    if mode & A_REAL:
        a = a.real.astype(a.dtype)
    if mode & A_LOWER:
        a = np.tril(a)
    if mode & A_UPPER:
        a = np.triu(a)
    acc = a @ b
    if mode & RE_ONLY:
        acc = acc.real.astype(acc.dtype)
    return acc


def ref_gemm(A, B, opA, opB, alpha, beta=0.0, C0=None, mode=0):
    out = alpha * ref_acc(A, B, opA, opB, mode)
    if beta != 0:
        out = out + beta * C0
    return out


def ref_epilogue(acc, alpha, epi, aux=None):
    """(C, monitor) of a fused epilogue on acc = op(A) op(B): the monitor is max |Im(alpha acc)|
    (0 for EPI_STREAM, which has none)."""
    v = alpha * acc
    mon = float(abs(v.imag).max()) if v.size else 0.0
    if epi == EPI_STREAM:
        return v, 0.0
    if epi == EPI_CSQUARE:
        return v * v, mon
    if epi == EPI_REAL:
        return v.real.copy(), mon
    if epi == EPI_WSRHO:
        return (aux * v.real).astype(v.dtype), mon
    raise ValueError(epi)


def ref_herk(A, alpha, beta=0.0, C0=None, mode=0):
    """alpha A A^H (RE_ONLY: its real part) + beta C0."""
    acc = A @ A.conj().swapaxes(-1, -2)
    if mode & RE_ONLY:
        acc = acc.real.astype(acc.dtype)
    out = alpha * acc
    if beta != 0:
        out = out + beta * C0
    return out


# ---- padded operands --------------------------------------------------------------------------
def padded(batch, rows, cols, ld, fill, dtype=np.complex128):
    """A flat buffer of `batch` slabs (stride rows * ld + GAP) filled with `fill`, its logical
    (batch, rows, cols) view and the stride."""
    stride = rows * ld + GAP
    buf = np.full(max(batch, 1) * stride, fill, dtype=dtype)
    isz = buf.itemsize
    view = np.lib.stride_tricks.as_strided(buf, (batch, rows, cols),
                                           (stride * isz, ld * isz, isz))
    return buf, view, stride


def logical(buf, batch, rows, cols, ld):
    """The logical (batch, rows, cols) view of a flat buffer laid out by padded()."""
    stride = rows * ld + GAP
    isz = buf.itemsize
    return np.lib.stride_tricks.as_strided(buf, (batch, rows, cols), (stride * isz, ld * isz, isz))


def padding_mask(batch, rows, cols, ld):
    """True where a buffer laid out by padded() holds padding (not a logical element)."""
    m, v, _ = padded(batch, rows, cols, ld, True, dtype=bool)
    v[...] = False
    return m


def rnd(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def stored_shape(op, rows, K):
    """Stored shape of an operand whose op() is rows x K (A) — for B pass op ^ 1."""
    return (K, rows) if op & 1 else (rows, K)


# ---- case tables ------------------------------------------------------------------------------
# beta: 0 -> beta = 0 with a NaN C; 1 -> complex BETA with a random C
Gemm = namedtuple("Gemm", "opA opB M N K batch ks mode beta")


def gid(c):
    s = "%s%s-%dx%dx%d-b%d" % ("NTRC"[c.opA], "NTRC"[c.opB], c.M, c.N, c.K, c.batch)
    if c.ks > 1:
        s += "-ks%d" % c.ks
    if c.mode:
        s += "-m%d" % c.mode
    return s + ("-beta" if c.beta else "")


# 1. op matrix x loop variant: K = 20 ring-2, 37 plain, 40 / 48 / 56 pipelined with 5, 6, 7
# K-steps (the three phases of the 3-deep ring)
OPS_K = (20, 37, 40, 48, 56)
GROUP_OPS = [Gemm(a, b, 70, 45, K, 3, 1, 0, 1) for (a, b) in OPS for K in OPS_K]

# 2. split-K
SPLITK_SHAPES = [(33, 45, 20, 8),      # more splits asked for than K-steps
                 (70, 45, 77, 2),      # plain
                 (70, 45, 104, 3), (70, 45, 136, 4), (70, 45, 168, 5),  # last split 3, 2, 1 steps
                 (130, 70, 160, 2)]    # several tiles
SPLITK_OPS = [(OP_N, OP_N), (OP_C, OP_N), (OP_N, OP_C), (OP_T, OP_T), (OP_R, OP_T)]
GROUP_SPLITK = [Gemm(a, b, M, N, K, batch, ks, 0, beta)
                for (M, N, K, ks) in SPLITK_SHAPES for (a, b) in SPLITK_OPS
                for batch in (1, 2) for beta in (0, 1)]

# 3. real / triangular modes on the 64 x 64 kernel (N < 512)
REAL_OPS = [(OP_N, OP_N), (OP_C, OP_N)]
GROUP_REAL = [Gemm(a, b, 70, 45, K, 2, 1, mode, 0)
              for mode in (1, 2, 3) for (a, b) in REAL_OPS for K in (20, 37, 56)]
# (40, 24) is the one shape short enough for the 2-deep ring
LOWER_MK = [(64, 64), (72, 72), (130, 130), (200, 200), (200, 64), (64, 128), (40, 24)]
GROUP_LOWER = [Gemm(OP_N, OP_N, M, N, K, 2, 1, mode, 0)
               for mode in (4, 5) for N in (45, 200) for (M, K) in LOWER_MK]
UPPER_OPS = [(OP_C, OP_N), (OP_C, OP_C)]
GROUP_UPPER = [Gemm(a, b, r, N, r, batch, ks, 8, 0)
               for (a, b) in UPPER_OPS for r in (64, 72, 130, 200) for N in (45, 130)
               for ks in (1, 3) for batch in (1, 2)]

# 4. dispatch acceptance: every op pair x mode 0..9 at 16 x 16 x 16
GROUP_DISPATCH = [(a, b, mode) for mode in range(10) for (a, b) in OPS]

# 5. epilogues: (epi, opA, opB, M, N, K, batch, real_inputs)
Epi = namedtuple("Epi", "epi opA opB M N K batch real")
GROUP_EPI = (
    [Epi(EPI_CSQUARE, OP_R, OP_T, 45, 45, K, 2, False) for K in (20, 37, 56)]
    + [Epi(EPI_STREAM, OP_N, OP_C, 24, 130, K, 1, False) for K in (37, 40)]
    + [Epi(EPI_REAL, OP_N, OP_N, M, 600, K, 1, False) for M in (1, 8, 27) for K in (8, 36, 64)]
    + [Epi(EPI_WSRHO, OP_N, OP_T, 40, 70, 37, 1, False),
       Epi(EPI_WSRHO, OP_N, OP_N, 27, 130, 24, 1, False),
       # purely real inputs and a real alpha: the monitor must come back (nearly) zero
       Epi(EPI_CSQUARE, OP_R, OP_T, 45, 45, 56, 2, True),
       Epi(EPI_REAL, OP_N, OP_N, 27, 600, 36, 1, True)])


def eid(c):
    name = {EPI_STREAM: "stream", EPI_CSQUARE: "csquare", EPI_REAL: "real", EPI_WSRHO: "wsrho"}
    return "%s-%s%s-%dx%dx%d-b%d%s" % (name[c.epi], "NTRC"[c.opA], "NTRC"[c.opB], c.M, c.N, c.K,
                                       c.batch, "-realin" if c.real else "")


# 6. HERK: (n, K, ks, mode), alpha = -0.75; batched (n, K): batch 3, alpha = -1, beta = 1
HERK_ALPHA = -0.75
GROUP_HERK = [(n, K, ks, mode) for mode in (0, RE_ONLY) for n in (1, 24, 64, 88, 130)
              for K in (7, 37, 40) for ks in (1, 2)]
# with K in (7, 37, 40) a split never leaves the 2-deep ring: two longer K for the other loops
GROUP_HERK += [(n, K, 2, mode) for mode in (0, RE_ONLY) for n in (64, 130) for K in (96, 100)]
GROUP_HERK_BATCHED = [(n, K) for n in (24, 72, 130) for K in (37, 64)]

# 7. the wide kernel (NN, N >= 512, K % 8 == 0, batch 1) with padded views
GROUP_WIDE = ([Gemm(0, 0, M, N, K, 1, 1, mode, beta)
               for (M, N, K) in ((24, 512, 8), (70, 520, 40), (130, 777, 136))
               for mode in (0, 1) for beta in (0, 1)]
              + [Gemm(0, 0, M, N, K, 1, 1, mode, beta)
                 for (M, N, K) in ((72, 520, 72), (130, 777, 136))
                 for mode in (4, 5) for beta in (0, 1)])

# 8. degenerate sizes
GROUP_K0 = [Gemm(0, 0, 70, N, 0, 1, 1, 0, beta) for N in (45, 520) for beta in (0, 1)]
GROUP_EMPTY = [Gemm(0, 0, 0, 45, 20, 1, 1, 0, 1), Gemm(0, 0, 70, 0, 20, 1, 1, 0, 1),
               Gemm(0, 0, 70, 45, 20, 0, 1, 0, 1)]

GEMM_TABLES = {"ops": GROUP_OPS, "splitk": GROUP_SPLITK, "real": GROUP_REAL,
               "lower": GROUP_LOWER, "upper": GROUP_UPPER, "wide": GROUP_WIDE}


def all_gemm_cases():
    """Every Gemm case that runs a K loop (what the coverage assertions count)."""
    return [c for t in GEMM_TABLES.values() for c in t]


def make_operands(c, rng, real=False):
    """Logical A, B (stored shapes, batch first) of a Gemm / Epi case, as the mode wants them:
    A_REAL: Im A of magnitude 1e3 (must be ignored) unless the mode is also A_LOWER; A_LOWER: A
    lower triangular with garbage past each 64-row tile's last row; A_UPPER: A (K x M, op C)
    stored lower triangular with garbage above each 64-column tile's first row.  Returns
    (A_given, B, A_clean): the reference is formed from A_clean."""
    mode = getattr(c, "mode", 0)
    sa = (c.batch,) + stored_shape(c.opA, c.M, c.K)
    sb = (c.batch,) + stored_shape(c.opB ^ 1, c.N, c.K)
    if real:
        A = rng.standard_normal(sa) + 0j
        return A, rng.standard_normal(sb) + 0j, A
    A, B = rnd(rng, *sa), rnd(rng, *sb)
    clean = A
    if mode & A_LOWER:
        r, k = np.arange(c.M)[:, None], np.arange(c.K)[None, :]
        clean = np.tril(A)
        A = clean + np.where(k >= 64 * (r // 64 + 1), rnd(rng, *sa) * 1e3, 0)
    elif mode & A_UPPER:
        k, m = np.arange(c.K)[:, None], np.arange(c.M)[None, :]
        clean = np.tril(A)
        A = clean + np.where(k < 64 * (m // 64), rnd(rng, *sa) * 1e3, 0)
    elif mode & A_REAL:
        A = A.real + 1e3j * rng.choice([-1.0, 1.0], size=sa)
        clean = A
    return A, B, clean
