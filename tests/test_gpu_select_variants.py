"""The interpolation-point selection on the GPU, piece by piece, against the long-double references
of tests/select_cases.py: every pivot case through fisdf_select_pivots_ex with the kernel that ran
held to the plan (a refused kernel, a refused co-resident launch or a stalled step fails the test
instead of falling back in silence), twin rows, a tie with the batched kernel's bound, the default
rule on either side of 800 pivots, the selection Gram with its time-reversal fold and shards, the
composite entries and the point gather.

Inputs live between NaN guard regions, outputs inside sentinel-filled buffers whose padding and
guards are checked afterwards.  The Gram's bound is factor_cases.bound (16 times the float64
restatement's own error against long double, floored at n eps); pivots are compared exactly."""
import ctypes as C

import numpy as np
import pytest

import factor_cases as F
import select_cases as S

pytestmark = pytest.mark.gpu

GUARD, PAD = 64, 8
SENT = complex(-7.25e77, 3.5e66)
ISENT = -777
CNAN = complex(np.nan, np.nan)


@pytest.fixture(scope="module")
def env():
    import torch
    from fisdf import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ctx = _lib.Context(0, torch.cuda.current_stream().cuda_stream)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return torch, _lib, ctx, ncu


class Buf:
    """A device buffer of `count` complex elements between two guard regions, all `fill`."""

    def __init__(self, torch, count, fill):
        self.fill, self.count = fill, count
        self.flat = torch.full((count + 2 * GUARD,), fill, dtype=torch.complex128, device="cuda")
        self.ptr = C.c_void_p(self.flat.data_ptr() + GUARD * self.flat.element_size())

    def put(self, host):
        import torch
        host = np.ascontiguousarray(host, np.complex128).reshape(-1)
        assert host.size == self.count
        self.flat[GUARD:GUARD + self.count] = torch.from_numpy(host).cuda()
        return self

    def get(self):
        return self.flat[GUARD:GUARD + self.count].cpu().numpy()

    def guards_intact(self):
        g = np.concatenate([self.flat[:GUARD].cpu().numpy(),
                            self.flat[GUARD + self.count:].cpu().numpy()])
        return bool((np.isnan(g) if self.fill != self.fill else g == self.fill).all())


def run_pivots(env, x2, rmax, tol, mode, lds_cols=0, wgs=0):
    """fisdf_select_pivots_ex on x2 (n x n, complex): (pivots, npiv, full_rank, info[6]); the
    host buffer's padding and the pivots beyond npiv must be left alone, the input unchanged."""
    torch, L, ctx, _ = env
    n = x2.shape[0]
    dx2 = Buf(torch, n * n, CNAN).put(x2)
    perm = np.full(rmax + 2 * PAD, ISENT, np.int32)
    info = np.full(6 + 2 * PAD, ISENT, np.int32)
    npiv, full = C.c_int(ISENT), C.c_int(ISENT)
    at = lambda a: C.cast(a.ctypes.data + 4 * PAD, L._ip)
    ctx.call("fisdf_select_pivots_ex", dx2.ptr, S.NK, n, rmax, tol, mode, lds_cols, wgs, at(perm),
             C.byref(npiv), C.byref(full), at(info))
    assert dx2.guards_intact()
    assert (perm[:PAD] == ISENT).all() and (perm[PAD + rmax:] == ISENT).all()
    assert (info[:PAD] == ISENT).all() and (info[PAD + 6:] == ISENT).all()
    r = npiv.value
    assert 0 <= r <= rmax and (perm[PAD + r:] == ISENT).all(), "perm[npiv:] was written"
    return perm[PAD:PAD + r].copy(), r, full.value, tuple(int(v) for v in info[PAD:PAD + 6])


def check_ran(env, info, n, rmax, mode, lds_cols, wgs, expect=None):
    """The kernel and its sizes are the plan's for this device; one pass."""
    ncu = env[3]
    want = S.reached(n, rmax, ncu, mode, lds_cols, wgs)
    assert info[:5] == want, (f"ran {S.KERNEL_NAMES[info[0]]} {info[1:5]}, the plan says "
                              f"{S.KERNEL_NAMES[want[0]]} {want[1:]} on {ncu} CUs")
    assert info[5] == 1, "a stalled step: the selection was redone on the second pass"
    if expect is not None and ncu == 256:
        assert info[0] == expect


# ------------------------------------------------------------------ a. pivot cases
@pytest.mark.parametrize("name", [c.name for c in S.PIV_CASES])
def test_pivot_case(env, name):
    c = S.PIV_BY_NAME[name]
    re = S.case_real(c)
    ref = S.reference(re, c.rmax, c.tol)
    im = S.case_imag(c)
    x2 = re + 1j * im if im is not None else re.astype(np.complex128)
    piv, r, full, info = run_pivots(env, x2, c.rmax, c.tol, c.mode, c.lds_cols, c.wgs)
    same = int((piv[:min(r, ref.rank)] == ref.piv[:min(r, ref.rank)]).sum())
    print(f"{name}: {S.KERNEL_NAMES[info[0]]} G {info[1]} RW {info[2]} K {info[3]} tpr {info[4]}, "
          f"npiv {r} (reference {ref.rank}), identical pivots {same}/{ref.rank}, min gap "
          f"{ref.min_gap:.1e}")
    check_ran(env, info, c.n, c.rmax, c.mode, c.lds_cols, c.wgs, c.expect)
    assert r == ref.rank and np.array_equal(piv, ref.piv)
    assert full == (1 if ref.rank < c.rmax else 0)


@pytest.mark.parametrize("name", S.IMAG_CASES)
def test_imaginary_part_is_ignored(env, name):
    c = S.PIV_BY_NAME[name]
    a = run_pivots(env, S.case_x2(c), c.rmax, c.tol, c.mode, c.lds_cols, c.wgs)
    b = run_pivots(env, S.case_x2(c, other_imag=True), c.rmax, c.tol, c.mode, c.lds_cols, c.wgs)
    z = run_pivots(env, S.case_real(c).astype(np.complex128), c.rmax, c.tol, c.mode, c.lds_cols,
                   c.wgs)
    assert a[3][0] == c.expect or env[3] != 256
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], z[0]) and a[1:] == b[1:] == z[1:]


@pytest.mark.parametrize("family", sorted(S.CROSS))
def test_kernels_agree(env, family):
    """One input on the batched, the cooperative, the split and the panel kernels: one result."""
    c0 = S.PIV_BY_NAME[S.CROSS[family][0]]
    x2 = S.case_x2(c0)
    runs = []
    for name in S.CROSS[family]:
        c = S.PIV_BY_NAME[name]
        assert (c.n, c.rmax, c.tol, c.family, c.k, c.seed) == (c0.n, c0.rmax, c0.tol, c0.family,
                                                               c0.k, c0.seed)
        runs.append((c.mode, c.lds_cols))
    if family in S.CROSS_SPLIT_OF:
        runs.append((1, S.CROSS_SPLIT_OF[family][1]))
    out = {}
    for mode, lds_cols in runs:
        piv, r, full, info = run_pivots(env, x2, c0.rmax, c0.tol, mode, lds_cols)
        check_ran(env, info, c0.n, c0.rmax, mode, lds_cols, 0)
        out[info[0]] = (piv.tolist(), r, full)
    print(f"{family}: " + ", ".join(S.KERNEL_NAMES[k] for k in sorted(out)))
    if env[3] == 256:
        assert sorted(out) == [S.BATCH, S.COOP, S.COOP_SPLIT, S.PANEL]
    first = out[min(out)]
    assert all(v == first for v in out.values())


def test_default_mode(env):
    """mode -1 at n = 1030 starts at the cooperative kernel for 799 pivots and at the batched one
    for 800 (their pivots: test_pivot_case d1030_r799, d1030_r800)."""
    lo, hi = S.PIV_BY_NAME["d1030_r799"], S.PIV_BY_NAME["d1030_r800"]
    assert (lo.mode, hi.mode, lo.rmax, hi.rmax) == (-1, -1, 799, 800)
    x2 = S.case_x2(hi)
    ran = [run_pivots(env, x2, c.rmax, c.tol, -1)[3] for c in (lo, hi)]
    for c, info in zip((lo, hi), ran):
        check_ran(env, info, c.n, c.rmax, -1, 0, 0)
    assert [i[0] for i in ran] == [S.COOP, S.BATCH]


# ------------------------------------------------------------------ b. twins and the bound's tie
@pytest.mark.parametrize("mode,lds_cols", [(0, 0), (1, 0), (1, 16), (2, 0)])
@pytest.mark.parametrize("name", [c.name for c in S.TWIN_CASES])
def test_twin_rows(env, name, mode, lds_cols):
    c = S.TWIN_BY_NAME[name]
    _, expect = S.twin_reference(c)
    piv, r, full, info = run_pivots(env, S.twin_x2(c), c.rmax, -1.0, mode, lds_cols)
    check_ran(env, info, c.n, c.rmax, mode, lds_cols, 0)
    at = int(np.argmax(expect == c.a))
    print(f"twin {name} on {S.KERNEL_NAMES[info[0]]}: pair ({c.a}, {c.b}) met at step {at}, the "
          f"device took {piv[at] if r > at else None}")
    assert r == c.rmax and full == 0
    assert S.twin_ok(c, piv, expect), (piv, expect)


@pytest.mark.parametrize("mode,lds_cols", [(0, 0), (1, 0), (1, 16), (2, 0)])
def test_tie_with_the_bound(env, mode, lds_cols):
    """select_cases.tie_real: the best candidate equals the bound B and has the larger row; the
    tie is exact on every path, so the reference's order (the smaller row first) is required."""
    ref = S.reference(S.tie_real(), S.TIE_RMAX, -1.0)
    piv, r, full, info = run_pivots(env, S.tie_x2(), S.TIE_RMAX, -1.0, mode, lds_cols)
    check_ran(env, info, S.TIE_N, S.TIE_RMAX, mode, lds_cols, 0)
    print(f"bound tie on {S.KERNEL_NAMES[info[0]]}: steps 4, 5 = {piv[4:6]} (reference "
          f"{ref.piv[4:6]})")
    assert r == S.TIE_RMAX and np.array_equal(piv, ref.piv)


def test_ex_refuses_before_it_launches(env):
    torch, L, ctx, _ = env
    x2 = torch.zeros(64 * 64, dtype=torch.complex128, device="cuda")
    perm = np.full(8, ISENT, np.int32)
    info = np.full(6, ISENT, np.int32)
    npiv, full = C.c_int(ISENT), C.c_int(ISENT)
    p = lambda a: a.ctypes.data_as(L._ip)
    for nip, mode, lds_cols, wgs in ((65, 1, 0, 0), (0, 1, 0, 0), (8, 3, 0, 0), (8, -2, 0, 0),
                                     (8, 1, -1, 0), (8, 1, 0, -1)):
        with pytest.raises(L.FisdfError):
            ctx.call("fisdf_select_pivots_ex", L.ptr(x2), S.NK, 64, nip, -1.0, mode, lds_cols, wgs,
                     p(perm), C.byref(npiv), C.byref(full), p(info))
    with pytest.raises(L.FisdfError):
        ctx.call("fisdf_select_pivots_ex", L.ptr(x2), S.NK, 64, 8, -1.0, 1, 0, 0, p(perm),
                 C.byref(npiv), C.byref(full), None)
    assert (perm == ISENT).all() and (info == ISENT).all()
    assert npiv.value == ISENT and full.value == ISENT


# ------------------------------------------------------------------ c. the Gram
def run_gram(env, x0, q0, q1, km=None, fold=0, ex=True):
    """x2 (ng0 x ng0, complex) of fisdf_select_gram_ex, or of fisdf_select_gram; its info."""
    torch, L, ctx, _ = env
    nk, ng0, nao = x0.shape
    dx0 = Buf(torch, x0.size, CNAN).put(x0)
    dx2 = Buf(torch, ng0 * ng0, SENT)
    info = (C.c_int * 3)(ISENT, ISENT, ISENT)
    if ex:
        kmp = (C.c_int * 3)(*km) if km is not None else None
        ctx.call("fisdf_select_gram_ex", dx0.ptr, kmp, fold, nk, q0, q1, ng0, nao, dx2.ptr, info)
    else:
        ctx.call("fisdf_select_gram", dx0.ptr, nk, q0, q1, ng0, nao, dx2.ptr)
        torch.cuda.synchronize()
    assert dx0.guards_intact() and dx2.guards_intact()
    x2 = dx2.get().reshape(ng0, ng0)
    assert not x2.imag.any(), "Im x2 must be zero"
    assert np.array_equal(x2.real, x2.real.T), "Re x2 must be exactly symmetric"
    return x2.real, tuple(info)


@pytest.mark.parametrize("nao", S.GRAM_NAO)
@pytest.mark.parametrize("ng0", S.GRAM_NG0)
def test_gram_plain_and_shards(env, ng0, nao):
    nk = S.GRAM_PLAIN_NK
    x0 = S.gram_x0(nk, ng0, nao, 500 + 16 * ng0 + nao)
    ref, bound = S.gram_reference(x0)
    whole, info = run_gram(env, x0, 0, nk)
    assert info == S.gram_plan(None, 0, nk, ng0, nao)
    old, _ = run_gram(env, x0, 0, nk, ex=False)
    assert np.array_equal(old, whole)                    # one code path behind both entries
    parts = np.zeros_like(whole)
    for q0, q1 in S.GRAM_SHARDS:
        part, pinfo = run_gram(env, x0, q0, q1)
        assert pinfo == S.gram_plan(None, 0, q1 - q0, ng0, nao)
        pref, pbound = S.gram_reference(x0, range(q0, q1)) if q1 > q0 else (0 * ref, 0.0)
        if q1 == q0:
            assert not part.any()
        else:
            assert F.relerr(part, pref) <= pbound
            assert np.array_equal(run_gram(env, x0, q0, q1, ex=False)[0], part)
        parts += part
    e, es = F.relerr(whole, ref), F.relerr(parts, ref)
    print(f"gram ng0 {ng0} nao {nao}: whole {e:.1e}, shard sum {es:.1e} (bound {bound:.1e}, "
          f"{max(e, es) / bound:.2f} of it)")
    # the shard sum equals the whole: both meet the whole's reference within the one bound (a
    # direct comparison of the two device results could only ask for twice the bound, which this
    # implies)
    assert e <= bound and es <= bound


@pytest.mark.parametrize("g", S.GRAM_FOLD, ids=lambda g: "x".join(map(str, g.km)))
def test_gram_fold(env, g):
    nk = int(np.prod(g.km))
    reps, w = S.kmesh_reps(g.km)
    # (a) x0[-k] = conj(x0[k]): folded and plain against the plain sum over all k
    x0 = S.gram_x0(nk, g.ng0, g.nao, 300 + nk, g.km)
    ref, bound = S.gram_reference(x0)
    folded, fi = run_gram(env, x0, 0, nk, g.km, 1)
    plain, pi = run_gram(env, x0, 0, nk, g.km, 0)
    assert fi == (g.reps, g.launches, g.ks_fold) and pi == (nk, 1, g.ks_all)
    assert np.array_equal(run_gram(env, x0, 0, nk, ex=False)[0], plain)   # fisdf_select_gram
    ef, ep, ed = F.relerr(folded, ref), F.relerr(plain, ref), F.relerr(folded, plain.astype(F.LD))
    # (b) no symmetry: the fold is the weighted sum over the representatives
    y0 = S.gram_x0(nk, g.ng0, g.nao, 700 + nk)
    wref, wbound = S.gram_reference(y0, reps, w)
    ew = F.relerr(run_gram(env, y0, 0, nk, g.km, 1)[0], wref)
    print(f"gram fold {g.km}: {g.reps} representatives in {g.launches} launches, split-K "
          f"{g.ks_fold} / {g.ks_all}: folded {ef:.1e}, plain {ep:.1e}, folded - plain {ed:.1e} "
          f"(bound {bound:.1e}); weighted {ew:.1e} (bound {wbound:.1e}); worst "
          f"{max(ef / bound, ep / bound, ed / bound, ew / wbound):.2f} of its bound")
    assert ef <= bound and ep <= bound and ed <= bound
    assert ew <= wbound
    if len(reps) < nk:      # the weights matter: the plain sum over all k is another matrix
        assert F.relerr(_plain_sum(y0), wref) > 1e3 * wbound


def _plain_sum(x0):
    return S.gram_reference(x0)[0]


def test_gram_ex_refuses_before_it_launches(env):
    torch, L, ctx, _ = env
    x0 = torch.zeros(8 * 4 * 2, dtype=torch.complex128, device="cuda")
    dx2 = Buf(torch, 16, SENT)
    km = (C.c_int * 3)(2, 2, 2)
    info = (C.c_int * 3)(ISENT, ISENT, ISENT)
    for kmp, fold, nk, q0, q1 in ((None, 1, 8, 0, 8), (km, 1, 8, 0, 7), (km, 0, 9, 0, 9),
                                  (km, 0, 8, 3, 2)):
        with pytest.raises(L.FisdfError):
            ctx.call("fisdf_select_gram_ex", L.ptr(x0), kmp, fold, nk, q0, q1, 4, 2, dx2.ptr, info)
    torch.cuda.synchronize()
    assert (dx2.get() == SENT).all() and dx2.guards_intact() and tuple(info) == (ISENT,) * 3


# ------------------------------------------------------------------ d. composite entries
def test_select_points_entries(env):
    torch, L, ctx, _ = env
    x0, x4, ref = S.composite_input()
    nk, ng0, nao = x0.shape
    dx0 = Buf(torch, x0.size, CNAN).put(x0)
    km = (C.c_int * 3)(*S.COMP_KM)
    got = {}
    try:
        for what in ("points", "km_fold", "km_plain"):
            perm = np.full(S.COMP_NIP, ISENT, np.int32)
            npiv, full = C.c_int(ISENT), C.c_int(ISENT)
            if what == "points":
                ctx.call("fisdf_select_points", dx0.ptr, nk, ng0, nao, S.COMP_NIP, -1.0,
                         perm.ctypes.data_as(L._ip), C.byref(npiv), C.byref(full))
            else:
                ctx.call("fisdf_set_time_reversal", 1 if what == "km_fold" else 0)
                ctx.call("fisdf_select_points_km", dx0.ptr, km, ng0, nao, S.COMP_NIP, -1.0,
                         perm.ctypes.data_as(L._ip), C.byref(npiv), C.byref(full))
            got[what] = (perm, npiv.value, full.value)
    finally:
        ctx.call("fisdf_set_time_reversal", 0)
    assert dx0.guards_intact()
    for what, (perm, r, full) in got.items():
        print(f"select {what}: npiv {r}, identical pivots {int((perm == ref.piv).sum())}/{ref.rank}")
        assert r == ref.rank == S.COMP_NIP and full == 0 and np.array_equal(perm, ref.piv), what


@pytest.mark.parametrize("nk,ng0,nao,nip", [(3, 37, 5, 7), (3, 37, 5, 33), (1, 300, 1, 257)])
def test_gather_points(env, nk, ng0, nao, nip):
    torch, L, ctx, _ = env
    assert (nk * nip * nao) % 256 != 0
    rng = np.random.default_rng(900 + nip)
    x0 = rng.standard_normal((nk, ng0, nao)) + 1j * rng.standard_normal((nk, ng0, nao))
    perm = rng.integers(0, ng0, nip).astype(np.int32)
    perm[0] = perm[nip // 2] = ng0 - 1          # the last index, twice
    perm[-1] = perm[1]                          # a repeated index at the end
    dx0 = Buf(torch, x0.size, CNAN).put(x0)
    dX = Buf(torch, nk * nip * nao, SENT)
    ctx.call("fisdf_gather_points", dx0.ptr, nk, ng0, nao, perm.ctypes.data_as(L._ip), nip, dX.ptr)
    torch.cuda.synchronize()
    assert dX.guards_intact() and dx0.guards_intact()
    assert np.array_equal(dX.get().reshape(nk, nip, nao), x0[:, perm])
    bad = perm.copy()
    bad[3] = ng0
    with pytest.raises(L.FisdfError):
        ctx.call("fisdf_gather_points", dx0.ptr, nk, ng0, nao, bad.ctypes.data_as(L._ip), nip, dX.ptr)
