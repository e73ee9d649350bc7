"""The separable k-mesh transforms on the device, every path through its direct C-ABI entry against
a long-double DFT: the register, LDS and fused kernels of the y build (fisdf_kmesh_y_ex,
fisdf_y_fused_ex, fisdf_y_fused_stream_ex, fisdf_build_y), x4 (fisdf_build_x4), get_k's pair
(fisdf_k_wsrho_ex) and the Bloch AO's DFT (fisdf_bloch_dft_ex, fisdf_bloch_band_ex).

Cases, references, the restated launch rules and the conventions live in tests/kmesh_cases.py
(tests/test_kmesh_cases.py checks on the CPU that the tables reach every instantiation, tier and
branch).  Every input is a view into a buffer of NaN, with NaN in every row a kernel must not read;
every output a view into the sentinel 7 + 7j, and every element a call must not write has to come
back as the sentinel bit for bit.

Bound (tests/factor_cases.py's rule): the device may be 16 times as far from the long-double
result as the float64 restatement of the same sums is, floored at n eps (n the longest sum: nk for
the transforms, max(nao, nk) with the GEMM in front), in max-norm relative to max |ref|; the
monitor value (max |Im| of the s-space field) gets the same bound, its error relative to the
largest magnitude of that field (under time reversal the monitor itself is a rounding residue).
"""
import ctypes as C

import numpy as np
import pytest

import kmesh_cases as K

pytestmark = pytest.mark.gpu

NAN = complex(np.nan, np.nan)
KPAD = 13           # extra elements between the k blocks of f
WORST = {}          # family -> (largest error / bound, error, bound, cases)


@pytest.fixture(scope="module")
def env():
    import torch
    from fisdf import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ctx = _lib.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, _lib, ctx
    for fam, (ratio, err, tol, n) in sorted(WORST.items()):
        print(f"kmesh {fam}: {n} comparisons, largest error {err:.2e} (bound {tol:.2e}, "
              f"ratio {ratio:.2f})")


def note(fam, err, tol):
    r = err / tol
    old = WORST.get(fam, (-1.0, 0.0, 0.0, 0))
    WORST[fam] = (r, err, tol, old[3] + 1) if r > old[0] else old[:3] + (old[3] + 1,)
    assert err <= tol, (fam, err, tol)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan_view(torch, a):
    """a (flat) on the device inside NaN: (buffer, view of the logical part)."""
    a = np.asarray(a).ravel()
    buf = np.full(a.size + 2 * K.EDGE, NAN if np.iscomplexobj(a) else np.nan)
    buf[K.EDGE:K.EDGE + a.size] = a
    d = dev(torch, buf)
    return d, d[K.EDGE:K.EDGE + a.size]


def f_view(torch, f):
    """f (nk, m, nao) with its k blocks fks = m nao + KPAD apart in NaN: (buffer, view, fks)."""
    nk, m, nao = f.shape
    ks = m * nao + KPAD
    buf = np.full(nk * ks + 2 * K.EDGE, NAN)
    for k in range(nk):
        buf[K.EDGE + k * ks: K.EDGE + k * ks + m * nao] = f[k].ravel()
    d = dev(torch, buf)
    return d, d[K.EDGE:], ks


def out_view(torch, n):
    d = dev(torch, np.full(n + 2 * K.EDGE, K.SENTINEL))
    return d, d[K.EDGE:K.EDGE + n]


def untouched(d):
    return bool(np.all(d.cpu().numpy() == K.SENTINEL))


def km3(kmesh):
    return (C.c_int * 3)(*kmesh)


def lattice():
    return (C.c_double * 9)(*K.LATTICE.ravel())


class Layout:
    """yT[slot * qs + I * Is + goff + g] for the columns c = I * m + g of nq slots."""

    def __init__(self, nq, ncol, m, goff, pad):
        self.nq, self.ncol, self.m, self.goff = nq, ncol, m, goff
        self.Is = m + goff + pad
        self.qs = -(-ncol // m) * self.Is + pad
        c = np.arange(ncol)
        self.pos = (c // m) * self.Is + goff + c % m
        self.size = nq * self.qs

    def check(self, buf, view, ref, real_slots=()):
        """the written elements (nq, ncol), after asserting that all the others, the edges
        included, are the sentinel bit for bit.  real_slots: stored as doubles in the first half
        of the slot, whose second half stays the sentinel."""
        h = buf.cpu().numpy()
        flat = h.view(np.float64)
        want = np.ones(flat.size, bool)                      # True: must still be the sentinel
        got = np.empty((self.nq, self.ncol), complex)
        for s in range(self.nq):
            base = K.EDGE + s * self.qs
            if s in real_slots:
                idx = 2 * base + self.pos
                got[s] = flat[idx]
            else:
                idx = np.concatenate([2 * (base + self.pos), 2 * (base + self.pos) + 1])
                got[s] = h[base + self.pos]
            want[idx] = False
        assert np.all(flat[want] == 7.0), "an element outside the output was written"
        assert got.shape == np.shape(ref)
        return got


def run_kmesh_y(env, c, conj_out=0):
    torch, L, ctx = env
    d = K.y_data(c.kmesh, c.ncol, c.half, conj_out, c.qsel)
    lay = Layout(len(d.qs), c.ncol, c.m, c.goff, c.pad)
    fb, fv = nan_view(torch, d.fx)
    ob, ov = out_view(torch, lay.size)
    qa, qp = L.iarr(d.qs)
    mon, rt = C.c_double(-1.0), C.c_int(-2)
    ctx.call("fisdf_kmesh_y_ex", L.ptr(fv), c.ncol, km3(c.kmesh), qp, len(d.qs), c.m, L.ptr(ov),
             lay.qs, lay.Is, c.goff, c.half, conj_out, C.byref(mon), C.byref(rt))
    got = lay.check(ob, ov, d.ref)
    return d, got, mon.value, rt.value


# ---- register y transform ----------------------------------------------------------------------
@pytest.mark.parametrize("c", K.REG_Y_CASES + [K.REG_Y_BIT63, K.REG_Y_STRIDE], ids=K.case_id)
def test_register_y(env, c):
    d, got, mon, rt = run_kmesh_y(env, c, c.conj_out)
    assert rt == K.REG == K.route(c.kmesh, c.ncol)[0]
    err, tol = K.rel_err(got, d.ref), K.bound(d.err64, d.nsum)
    merr, mtol = abs(mon - d.mon) / d.scale, K.bound(d.mon64, d.nsum)
    print(f"register y {K.case_id(c)}: err {err:.2e} bound {tol:.2e}; monitor {merr:.2e} {mtol:.2e}")
    note("y register", err, tol)
    note("y register monitor", merr, mtol)


# ---- LDS y transform ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.LDS_Y_CASES + [K.LDS_Y_STRIDE], ids=K.case_id)
def test_lds_y(env, c):
    d, got, mon, rt = run_kmesh_y(env, c)
    assert rt == K.LDS == K.route(c.kmesh, c.ncol)[0]
    err, tol = K.rel_err(got, d.ref), K.bound(d.err64, d.nsum)
    merr, mtol = abs(mon - d.mon) / d.scale, K.bound(d.mon64, d.nsum)
    print(f"lds y {K.case_id(c)} CT {K.route(c.kmesh)[1]} lds {K.route(c.kmesh)[2]}: err {err:.2e} "
          f"bound {tol:.2e}; monitor {merr:.2e} {mtol:.2e}")
    note("y lds", err, tol)
    note("y lds monitor", merr, mtol)


def _refused(env, name, *args):
    torch, L, ctx = env
    rc = getattr(L.load(), name)(ctx.h, *args)
    assert rc != 0, name + " accepted a call it must refuse"
    return L.load().fisdf_last_error(ctx.h).decode()


def test_refused_calls_leave_the_output_untouched(env):
    """A k-mesh axis above 16, a tile above 160 KB of LDS, a q-list that is not ascending or
    leaves the k-mesh, conj_out off the register list: refused before anything is launched."""
    torch, L, ctx = env
    ncol, m = 20, 20
    mon, rt = C.c_double(), C.c_int()

    def call(kmesh, qs, conj_out=0):
        nk = K.nk_of(kmesh)
        fb, fv = nan_view(torch, np.zeros(nk * ncol, complex))
        ob, ov = out_view(torch, nk * ncol)
        qa, qp = L.iarr(qs)
        msg = _refused(env, "fisdf_kmesh_y_ex", L.ptr(fv), ncol, km3(kmesh), qp, len(qs), m,
                       L.ptr(ov), ncol, m, 0, 0, conj_out, C.byref(mon), C.byref(rt))
        ctx.call("fisdf_sync")
        assert untouched(ob) and rt.value == -1, (kmesh, qs)
        return msg

    assert "1..16" in call((17, 1, 1), [0])
    assert "too large" in call((16, 16, 5), [0])
    for km in ((2, 2, 2), (1, 1, 3)):
        assert "ascending" in call(km, [1, 0])
        assert "ascending" in call(km, [0, 0])
        assert "ascending" in call(km, [K.nk_of(km)])
    for km in ((1, 1, 3), (8, 8, 1)):
        assert "conj_out" in call(km, [0], conj_out=1)
    # the composite entries check the k-mesh on entry, before their first GEMM
    km, nip, nao, ng = (17, 1, 1), 3, 2, 5
    Xb, Xv = nan_view(torch, np.zeros(17 * nip * nao, complex))
    fb, fv = nan_view(torch, np.zeros(17 * ng * nao, complex))
    ob, ov = out_view(torch, 17 * nip * max(nip, ng))
    assert "1..16" in _refused(env, "fisdf_build_x4", L.ptr(Xv), nip, nao, km3(km), lattice(),
                               L.ptr(ov))
    assert "1..16" in _refused(env, "fisdf_build_y", L.ptr(fv), ng * nao, 0, ng, ng, L.ptr(Xv), nip,
                               nao, km3(km), lattice(), 0, 17, L.ptr(ov))
    ctx.call("fisdf_sync")
    assert untouched(ob)
    # the fused entry: the same q-list checks
    hd = C.c_int(-1)
    for qs in ([1, 0], [8]):
        qa, qp = L.iarr(qs)
        assert "ascending" in _refused(env, "fisdf_y_fused_ex", L.ptr(Xv), 3, 2, L.ptr(fv), 10, 5,
                                       km3((2, 2, 2)), qp, len(qs), L.ptr(ov), 15, 5, 0, 0,
                                       C.byref(hd))
    ctx.call("fisdf_sync")
    assert untouched(ob) and hd.value == 0


# ---- fused y -----------------------------------------------------------------------------------
def fused_q_and_mask(c):
    qs = K.q_lists(c.kmesh)[c.qsel]
    sc = [int(q) for q in K.self_conjugate(c.kmesh)]
    rmask = K.mask_of(sc) if c.real else 0
    return qs, rmask, [i for i, q in enumerate(qs) if c.real and q in sc]


def run_fused(env, c, d, qs, rmask, real_slots):
    torch, L, ctx = env
    lay = Layout(len(qs), c.nip * c.m, c.m, c.goff, c.pad)
    Xb, Xv = nan_view(torch, d.X)
    fb, fv, fks = f_view(torch, d.F)
    ob, ov = out_view(torch, lay.size)
    qa, qp = L.iarr(qs)
    hd = C.c_int(-1)
    ctx.call("fisdf_y_fused_ex", L.ptr(Xv), c.nip, c.nao, L.ptr(fv), fks, c.m, km3(c.kmesh), qp,
             len(qs), L.ptr(ov), lay.qs, lay.Is, c.goff, rmask, C.byref(hd))
    return lay, ob, ov, hd.value


@pytest.mark.parametrize("c", K.FUSED_CASES, ids=K.case_id)
def test_fused_y(env, c):
    d = K.fused_data(c.kmesh, c.nip, c.m, c.nao)
    qs, rmask, real_slots = fused_q_and_mask(c)
    lay, ob, ov, handled = run_fused(env, c, d, qs, rmask, real_slots)
    assert handled == 1
    ref = d.ref.reshape(len(d.ref), -1)[qs]
    got = lay.check(ob, ov, ref, real_slots)
    if c.real == 1:
        assert real_slots and len(real_slots) == len(K.self_conjugate(c.kmesh))
    for s in real_slots:                                      # y_q of a self-conjugate q is real
        assert abs(ref[s].imag).max() <= K.EPS * abs(ref).max()
    err, tol = K.rel_err(got, ref), K.bound(d.err64, d.nsum)
    print(f"fused y {K.case_id(c)}: err {err:.2e} bound {tol:.2e}")
    note("y fused", err, tol)


def _build_y(env, kmesh, X, F, nip, m, nao, tr):
    """fisdf_build_y over the whole grid of m points, every q: y (nk, nip * m)."""
    torch, L, ctx = env
    nk = K.nk_of(kmesh)
    lay = Layout(nk, nip * m, m, 0, 0)
    Xb, Xv = nan_view(torch, X)
    fb, fv, fks = f_view(torch, F)
    ob, ov = out_view(torch, lay.size)
    ctx.call("fisdf_set_time_reversal", tr)
    try:
        ctx.call("fisdf_build_y", L.ptr(fv), fks, 0, m, m, L.ptr(Xv), nip, nao, km3(kmesh),
                 lattice(), 0, nk, L.ptr(ov))
        ctx.call("fisdf_sync")
    finally:
        ctx.call("fisdf_set_time_reversal", 0)
    return lay, ob, ov


def test_fused_refuses_nao_129_and_build_y_takes_the_half_register_kernel(env):
    torch, L, ctx = env
    km, nip, m, nao = (2, 2, 2), 17, 19, K.FUSED_REFUSED_NAO
    d = K.fused_data(km, nip, m, nao)
    c = K.Fused(km, nip, m, nao, 0, 0, 0, 0)
    lay, ob, ov, handled = run_fused(env, c, d, list(range(8)), 0, [])
    ctx.call("fisdf_sync")
    assert handled == 0 and untouched(ob)
    # X and F hold NaN at the k time reversal must not read
    lay, ob, ov = _build_y(env, km, d.X, d.F, nip, m, nao, 1)
    ref = d.ref.reshape(8, -1)
    err, tol = K.rel_err(lay.check(ob, ov, ref), ref), K.bound(d.err64, d.nsum)
    print(f"build_y nao 129 (HALF register kernel): err {err:.2e} bound {tol:.2e}")
    note("build_y", err, tol)


@pytest.mark.parametrize("tr", [0, 1])
@pytest.mark.parametrize("km", K.UNRUN_BEFORE, ids=str)
def test_build_y_on_the_unrun_meshes(env, km, tr):
    nip, m, nao = 17, 19, 5
    d = K.fused_data(km, nip, m, nao)
    X, F = (d.X, d.F) if tr else (d.fullX, d.fullF)
    lay, ob, ov = _build_y(env, km, X, F, nip, m, nao, tr)
    ref = d.ref.reshape(len(d.ref), -1)
    err, tol = K.rel_err(lay.check(ob, ov, ref), ref), K.bound(d.err64, d.nsum)
    print(f"build_y {km} time_reversal={tr}: err {err:.2e} bound {tol:.2e}")
    note("build_y", err, tol)


@pytest.mark.parametrize("c", K.STREAMED_CASES, ids=K.case_id)
def test_fused_y_streamed(env, c):
    torch, L, ctx = env
    d = K.streamed_data(c.kmesh, c.nip, c.m, c.nao, c.ng0)
    nk = K.nk_of(c.kmesh)
    qs = list(range(nk))
    lay = Layout(nk, c.nip * c.m, c.m, 1, 2)
    xb, xv = nan_view(torch, d.x0)
    fb, fv, fks = f_view(torch, d.F)
    qa, qp = L.iarr(qs)
    pa, pp = L.iarr(d.piv)
    ob, ov = out_view(torch, lay.size)
    hd, er = C.c_int(-1), C.c_int(-1)
    ctx.call("fisdf_y_fused_stream_ex", L.ptr(xv), c.ng0, c.nao, pp, c.nip, c.rows, L.ptr(fv), fks,
             c.m, km3(c.kmesh), qp, nk, L.ptr(ov), lay.qs, lay.Is, 1, 0, c.two, C.byref(hd),
             C.byref(er))
    assert (hd.value, er.value) == (1, 0)
    ref = d.ref.reshape(nk, -1)
    got = lay.check(ob, ov, ref)
    # the unstreamed kernel on the gathered rows: the same bits
    Xb, Xv = nan_view(torch, d.x0[:, d.piv])
    o2b, o2v = out_view(torch, lay.size)
    ctx.call("fisdf_y_fused_ex", L.ptr(Xv), c.nip, c.nao, L.ptr(fv), fks, c.m, km3(c.kmesh), qp, nk,
             L.ptr(o2v), lay.qs, lay.Is, 1, 0, C.byref(hd))
    assert hd.value == 1 and np.array_equal(got, lay.check(o2b, o2v, ref))
    err, tol = K.rel_err(got, ref), K.bound(d.err64, d.nsum)
    print(f"streamed y {K.case_id(c)}: err {err:.2e} bound {tol:.2e}")
    note("y fused streamed", err, tol)


# ---- x4 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.X4_CASES, ids=K.case_id)
def test_x4(env, c, monkeypatch):
    torch, L, ctx = env
    d = K.x4_data(c.kmesh, c.nip, c.nao)
    nk = K.nk_of(c.kmesh)
    Xb, Xv = nan_view(torch, d.X)
    ob, ov = out_view(torch, nk * c.nip * c.nip)
    if c.dense:
        monkeypatch.setenv("FISDF_X4_DFT", "0")
    else:
        monkeypatch.delenv("FISDF_X4_DFT", raising=False)
    ctx.max_imag()
    ctx.call("fisdf_set_time_reversal", c.tr)
    try:
        ctx.call("fisdf_build_x4", L.ptr(Xv), c.nip, c.nao, km3(c.kmesh), lattice(), L.ptr(ov))
        ctx.call("fisdf_sync")
    finally:
        ctx.call("fisdf_set_time_reversal", 0)
    mon = ctx.max_imag()[0]
    h = ob.cpu().numpy()
    assert np.all(h[:K.EDGE] == K.SENTINEL) and np.all(h[-K.EDGE:] == K.SENTINEL)
    got = h[K.EDGE:-K.EDGE].reshape(d.ref.shape)
    lattice_phi = c.dense or (nk > 1 and K.route(c.kmesh)[0] != K.REG)
    err64 = d.err64_dense if lattice_phi else d.err64
    err, tol = K.rel_err(got, d.ref), K.bound(err64, d.nsum)
    mtol = K.bound(err64, d.nsum)
    print(f"x4 {K.case_id(c)}: err {err:.2e} bound {tol:.2e}; monitor {mon / d.scale:.2e} {mtol:.2e}")
    fam = "x4 dense" if lattice_phi else ("x4 gamma" if nk == 1 else "x4 register")
    note(fam, err, tol)
    note(fam + " monitor", abs(mon - d.mon) / d.scale, mtol)


# ---- get_k's pair ------------------------------------------------------------------------------
def run_wsrho(env, kmesh, ncol, use_reg):
    torch, L, ctx = env
    d = K.wsrho_data(kmesh, ncol)
    nk = K.nk_of(kmesh)
    ld = ncol + K.WSRHO_PAD
    ws = np.full((nk, ld), np.nan)
    ws[:, :ncol] = d.Ws
    wb, wv = nan_view(torch, ws)
    bb = dev(torch, np.concatenate([np.full(K.EDGE, K.SENTINEL), d.B.ravel(),
                                    np.full(K.EDGE, K.SENTINEL)]))
    bv = bb[K.EDGE:K.EDGE + nk * ncol]
    mon, hd = C.c_double(-1.0), C.c_int(-1)
    ctx.call("fisdf_k_wsrho_ex", L.ptr(bv), ncol, km3(kmesh), lattice(), L.ptr(wv), ld, use_reg,
             C.byref(mon), C.byref(hd))
    h = bb.cpu().numpy()
    assert np.all(h[:K.EDGE] == K.SENTINEL) and np.all(h[-K.EDGE:] == K.SENTINEL)
    return d, h[K.EDGE:-K.EDGE].reshape(nk, ncol), mon.value, hd.value


@pytest.mark.parametrize("ncol", K.WSRHO_NCOL)
@pytest.mark.parametrize("km", K.REG_MESHES, ids=str)
def test_get_k_pair(env, km, ncol):
    d, reg, mon, hd = run_wsrho(env, km, ncol, 1)
    assert hd == 1
    err, tol = K.rel_err(reg, d.ref), K.bound(d.err64, d.nsum)
    note("get_k pair register", err, tol)
    note("get_k pair register monitor", abs(mon - d.mon) / d.scale, K.bound(d.mon64, d.nsum))
    d, dense, mond, hd = run_wsrho(env, km, ncol, 0)
    assert hd == 0
    errd, told = K.rel_err(dense, d.ref), K.bound(d.err64_dense, d.nsum)
    print(f"get_k pair {km} ncol {ncol}: register {err:.2e} bound {tol:.2e}; dense {errd:.2e} "
          f"bound {told:.2e}")
    note("get_k pair dense", errd, told)
    note("get_k pair dense monitor", abs(mond - d.mon) / d.scale, told)
    assert abs(reg - dense).max() < K.WSRHO_PAIR_TOL * abs(dense).max()


def test_get_k_pair_off_the_list_is_not_handled(env):
    d, dense, mon, hd = run_wsrho(env, K.WSRHO_OFF_LIST, 65, 1)
    assert hd == 0
    note("get_k pair dense", K.rel_err(dense, d.ref), K.bound(d.err64_dense, d.nsum))


# ---- Bloch AO ----------------------------------------------------------------------------------
def run_bloch(env, kmesh, ncol, F):
    torch, L, ctx = env
    nk = K.nk_of(kmesh)
    fb, fv = nan_view(torch, F)
    ob, ov = out_view(torch, nk * ncol)
    rt = C.c_int(-2)
    ctx.call("fisdf_bloch_dft_ex", L.ptr(fv), ncol, km3(kmesh), L.ptr(ov), C.byref(rt))
    h = ob.cpu().numpy()
    assert np.all(h[:K.EDGE] == K.SENTINEL) and np.all(h[-K.EDGE:] == K.SENTINEL)
    return h[K.EDGE:-K.EDGE].reshape(nk, ncol), rt.value


@pytest.mark.parametrize("ncol", K.BLOCH_NCOL)
@pytest.mark.parametrize("km", K.REG_MESHES + K.BLOCH_GENERIC, ids=str)
def test_bloch_dft(env, km, ncol):
    d = K.bloch_data(km, ncol)
    got, rt = run_bloch(env, km, ncol, d.F)
    assert rt == K.route(km)[0]
    err, tol = K.rel_err(got, d.ref), K.bound(d.err64, d.nsum)
    print(f"bloch {km} ncol {ncol} route {rt}: err {err:.2e} bound {tol:.2e}")
    note("bloch register" if rt == K.REG else "bloch generic", err, tol)


def test_bloch_dft_grid_stride(env):
    km, ncol = K.BLOCH_STRIDE
    F = np.random.default_rng(2).standard_normal((1, ncol))
    got, rt = run_bloch(env, km, ncol, F)
    assert rt == K.REG and np.array_equal(got, F.astype(complex))   # one image: chi = F


@pytest.mark.parametrize("nkb", K.BAND_NKB)
@pytest.mark.parametrize("nT", K.BAND_NT)
@pytest.mark.parametrize("ncol", K.BLOCH_NCOL)
def test_bloch_band(env, ncol, nT, nkb):
    torch, L, ctx = env
    d = K.band_data(nT, nkb, ncol)
    fb, fv = nan_view(torch, d.F if nT else np.zeros(1))
    pb, pv = nan_view(torch, d.ph)
    ob, ov = out_view(torch, nkb * ncol)
    ctx.call("fisdf_bloch_band_ex", L.ptr(fv), ncol, nT, L.ptr(pv), nkb, L.ptr(ov))
    h = ob.cpu().numpy()
    assert np.all(h[:K.EDGE] == K.SENTINEL) and np.all(h[-K.EDGE:] == K.SENTINEL)
    got = h[K.EDGE:-K.EDGE].reshape(nkb, ncol)
    if nT == 0:
        assert np.all(got == 0)
        return
    err, tol = K.rel_err(got, d.ref), K.bound(d.err64, d.nsum)
    print(f"band nT {nT} nkb {nkb} ncol {ncol}: err {err:.2e} bound {tol:.2e}")
    note("bloch band", err, tol)
