"""The AO first derivatives and what is built on them, on the device against long-double
references: fisdf_eval_ao_deriv1 / fisdf_eval_ao_band_deriv1 (raw tables on a triclinic lattice),
fisdf_get_rho_gga and fisdf_gga_gram (random blocks), and ISDF.get_rho(xctype="GGA"), nr_vxc_mat
and get_kin end to end (the toy and diamond cells), tied together by the identity dE = tr(V dD)
of a polynomial functional.

Cases, references and conventions live in tests/xc_cases.py (tests/test_xc_cases.py checks them on
the CPU).  Inputs are views inside NaN with padded strides, outputs views inside the sentinel
7 + 7j, which has to come back intact; every entry runs twice and the two runs are compared bit
for bit.  A device result may be factor_cases.bound(err64, n) from the long-double reference: 16
times the float64 restatement's error, floored at n eps; the evaluator per AO column and component.

Component 0 of fisdf_get_rho_gga is fisdf_get_rho's sum in another order (eight column groups of
32 points where rho_grid has four waves of 64 or 128), so the two agree within the bound and not
bit for bit, except at nao = 1, where one thread adds the k-points in order in both kernels (the
two nao = 1 cases came out equal, the other ten 7e-15 to 4e-13 apart).
"""
import ctypes as C

import numpy as np
import pytest

import ao_cases as A
import kmesh_cases as K
import xc_cases as X

pytestmark = pytest.mark.gpu

SPARE = 40
NANC = complex(np.nan, np.nan)


@pytest.fixture(scope="module")
def env():
    import torch
    from fisdf import _lib
    from fisdf.isdf import _Device
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch, _lib, _Device()


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _dev(torch, host):
    return torch.from_numpy(np.ascontiguousarray(host)).cuda()


def _inside(torch, data, fill):
    """data (flattened) with EDGE elements of fill before and after: (buffer, view)."""
    flat = np.asarray(data).ravel()
    host = np.full(flat.size + 2 * X.EDGE, fill, dtype=flat.dtype)
    host[X.EDGE:X.EDGE + flat.size] = flat
    buf = _dev(torch, host)
    return buf, buf[X.EDGE:]


def _f4_buffer(torch, f4):
    """f4 (nk, 4, ng, nao) with padded strides inside NaN: (buffer, view, f_kstride, f_cstride)."""
    nk, _, ng, nao = f4.shape
    cs = ng * nao + X.CPAD
    ks = 4 * cs + X.KPAD
    host = np.full(nk * ks, NANC)
    for k in range(nk):
        for c in range(4):
            o = k * ks + c * cs
            host[o:o + ng * nao] = f4[k, c].ravel()
    buf, view = _inside(torch, host, NANC)
    return buf, view, ks, cs


# ================================================================ the evaluator
def ev_call(env, tab, coords, kmesh=None, kband=None, deriv=1, **over):
    """fisdf_eval_ao[_band][_deriv1] on raw tables; over replaces single arguments (the refusals).
    Returns (rc, message, output buffer, logical size)."""
    torch, L, device = env
    ng = len(np.reshape(coords, (-1, 3)))
    nao = A.nao_of(tab)
    nk = K.nk_of(kmesh) if kband is None else len(kband)
    nout = nk * (4 if deriv else 1) * ng * nao
    co = np.asarray(coords, float).ravel()
    cb = np.full(co.size + 2 * X.EDGE + 3, np.nan)
    cb[X.EDGE:X.EDGE + co.size] = co
    cb = _dev(torch, cb)
    ob = _dev(torch, np.full(nout + SPARE + 2 * X.EDGE, X.SENTINEL))
    k = dict(
        atoms=np.ascontiguousarray(tab.atoms, float), sh_atom=np.ascontiguousarray(tab.sh_atom, np.int32),
        sh_l=np.ascontiguousarray(tab.sh_l, np.int32), sh_np=np.ascontiguousarray(tab.sh_np, np.int32),
        exps=np.ascontiguousarray(tab.exps, float), coefs=np.ascontiguousarray(tab.coefs, float),
        tn=np.ascontiguousarray(np.reshape(tab.tn, (-1, 3)), np.int32),
        a=np.ascontiguousarray(tab.a, float).ravel(), ng=ng, nao=nao)
    k.update(over)
    head = (device.ctx.h, L.ptr(cb[X.EDGE:]), k["ng"], len(k["atoms"]), _dp(k["atoms"]), len(k["sh_l"]),
            _ip(k["sh_atom"]), _ip(k["sh_l"]), _ip(k["sh_np"]), _dp(k["exps"]), _dp(k["coefs"]),
            len(k["tn"]), _ip(k["tn"]))
    tail = (_dp(k["a"]), float(tab.rcut), k["nao"], L.ptr(ob[X.EDGE:]))
    lib = L.load()
    if kband is None:
        km = np.asarray(k.get("kmesh_arg", kmesh), np.int32)
        fn = lib.fisdf_eval_ao_deriv1 if deriv else lib.fisdf_eval_ao
        rc = fn(*head, _ip(km), *tail)
    else:
        kb = np.ascontiguousarray(kband, float)
        kp = None if k.get("null_kpts") else _dp(kb)
        fn = lib.fisdf_eval_ao_band_deriv1 if deriv else lib.fisdf_eval_ao_band
        rc = fn(*head, k.get("nkb", len(kb)), kp, *tail)
    msg = lib.fisdf_last_error(device.ctx.h).decode() if rc else ""
    device.ctx.call("fisdf_sync")
    return rc, msg, ob, nout


def _logical(ob, nout):
    h = ob.cpu().numpy()
    assert np.all(h[:X.EDGE] == X.SENTINEL) and np.all(h[X.EDGE + nout:] == X.SENTINEL), \
        "an element outside the output was written"
    return h[X.EDGE:X.EDGE + nout]


def ev_run(env, c, deriv=1):
    d = X.ev_data(c.name)
    rc, msg, ob, nout = ev_call(env, d.tab, d.coords, c.kmesh, d.kband, deriv=deriv)
    assert rc == 0, msg
    got = _logical(ob, nout)
    return d, got.reshape(d.ref.shape if deriv else d.ref[:, 0].shape)


@pytest.mark.parametrize("c", X.EV_CASES, ids=X.ev_id)
def test_evaluator(env, c):
    d, got = ev_run(env, c)
    _, again = ev_run(env, c)
    assert np.array_equal(got, again), "two runs differ"
    if c.ng == 0:
        assert got.size == 0            # _logical has seen the sentinel everywhere
        return
    # component 0 is fisdf_eval_ao's output bit for bit
    _, val = ev_run(env, c, deriv=0)
    assert np.array_equal(got[:, 0], val), "component 0 differs from fisdf_eval_ao"
    if c.tn == "none":
        assert not d.ref.any() and np.all(got == 0), "no translation: exact zeros"
        return
    err = X.col_err4(got, d.ref)
    tol = np.vectorize(lambda e: X.bound(e, d.nsum))(d.err64)
    i = np.unravel_index(np.argmax(err / tol), err.shape)
    print(f"{c.name}: err {err[i]:.2e} bound {tol[i]:.2e} at component {i[0]} column {i[1]} "
          f"{A.ao_labels(d.tab)[i[1]]}; float64 restatement {d.err64.max():.2e}, n {d.nsum}")
    assert np.all(err <= tol), (i, err[i], tol[i])
    if c.atom:      # the point on the atom alone: finite, and within the bound of its own scale
        assert np.all(np.isfinite(got[:, :, 0]))
        den = np.abs(d.ref).max(axis=(0, 2))
        e0 = np.asarray(np.abs(got[:, :, 0].astype(X.CLD) - d.ref[:, :, 0]).max(axis=0) / den, float)
        assert np.all(e0 <= tol)


def test_evaluator_refusals_leave_the_output_untouched(env):
    """Every refused argument set of fisdf_eval_ao / fisdf_eval_ao_band is refused by the deriv1
    entries on the host, the output stays the sentinel, and the next valid call gives the bits it
    gave before."""
    c, b = X.EV_BY_NAME["lds_113"], X.EV_BY_NAME["band_off3"]
    d, before = ev_run(env, c)
    db, before_band = ev_run(env, b)
    tab, nsh = d.tab, len(d.tab.sh_l)

    def with_(arr, i, v):
        out = np.array(arr, np.int32)
        out[i] = v
        return out

    refusals = [
        ("angular momentum", dict(sh_l=with_(tab.sh_l, 2, 4), nao=A.nao_of(tab) + 4)),
        ("angular momentum", dict(sh_l=with_(tab.sh_l, 0, -1), nao=A.nao_of(tab) - 8)),
        ("out of range", dict(sh_atom=with_(tab.sh_atom, 1, -1))),
        ("out of range", dict(sh_atom=with_(tab.sh_atom, nsh - 1, len(tab.atoms)))),
        ("nao does not match", dict(nao=A.nao_of(tab) + 1)),
        ("nao does not match", dict(nao=A.nao_of(tab) - 1)),
        ("at least one primitive", dict(sh_np=with_(tab.sh_np, 1, 0))),
        ("at least one primitive", dict(sh_np=with_(tab.sh_np, nsh - 1, -2))),
        ("bad sizes", dict(ng=-1)),
    ]
    kmesh_only = [("bad k-mesh", dict(kmesh_arg=(3, 0, 2))), ("bad k-mesh", dict(kmesh_arg=(0, 1, 1))),
                  ("bad k-mesh", dict(kmesh_arg=(3, 1, -2)))]
    band_only = [("no band k-points", dict(nkb=0)), ("no band k-points", dict(nkb=-1)),
                 ("no band k-points", dict(null_kpts=True))]
    n = 0
    for case, dd, extra in ((c, d, kmesh_only), (b, db, band_only)):
        for want, over in refusals + extra:
            rc, msg, ob, nout = ev_call(env, dd.tab, dd.coords, case.kmesh, dd.kband, **over)
            assert rc != 0, (case.name, over, "accepted a call it must refuse")
            assert want in msg, (case.name, over, msg)
            assert np.all(ob.cpu().numpy() == X.SENTINEL), (case.name, over)
            n += 1
    assert n == 2 * len(refusals) + 6
    assert np.array_equal(ev_run(env, c)[1], before)
    assert np.array_equal(ev_run(env, b)[1], before_band)


# ================================================================ fisdf_get_rho_gga
def rho_call(env, c, f4, D):
    torch, L, device = env
    fb, fv, ks, cs = _f4_buffer(torch, f4)
    Db, Dv = _inside(torch, D.astype(complex), NANC)
    rcs = c.ng + X.RPAD
    ob, ov = _inside(torch, np.full(c.nset * 4 * rcs, X.SENTINEL), X.SENTINEL)
    device.ctx.call("fisdf_get_rho_gga", L.ptr(fv), ks, cs, c.nk, c.ng, c.nao, L.ptr(Dv), c.nset,
                    c.hermi, L.ptr(ov), rcs)
    device.ctx.call("fisdf_sync")
    h = ob.cpu().numpy()
    rows = h[X.EDGE:X.EDGE + c.nset * 4 * rcs].reshape(c.nset, 4, rcs)
    assert np.all(h[:X.EDGE] == X.SENTINEL) and np.all(h[-X.EDGE:] == X.SENTINEL)
    assert np.all(rows[:, :, c.ng:] == X.SENTINEL), "an element between the rows was written"
    # fisdf_get_rho on the same buffer: component 0 of f4 is (nk, ng, nao) at k stride ks
    r0 = device.empty((c.nset, c.ng))
    device.ctx.call("fisdf_get_rho", L.ptr(fv), ks, c.nk, c.ng, c.nao, L.ptr(Dv), c.nset, L.ptr(r0))
    device.ctx.call("fisdf_sync")
    return rows[:, :, :c.ng].copy(), r0.cpu().numpy()


@pytest.mark.parametrize("c", X.RHO_CASES, ids=X.rho_id)
def test_rho_gga(env, c):
    f4, D = X.rho_inputs(c)
    got, rho0 = rho_call(env, c, f4, D)
    again, _ = rho_call(env, c, f4, D)
    assert np.array_equal(got, again), "two runs differ"
    ref, r64 = X.rho_gga_ref(f4, D, c.hermi, True), X.rho_gga_ref(f4, D, c.hermi, False)
    n = c.nk * c.nao * c.nao
    for comp in range(4):
        err, e64 = X.rel_err(got[:, comp], ref[:, comp]), X.rel_err(r64[:, comp], ref[:, comp])
        print(f"{X.rho_id(c)} component {comp}: err {err:.2e} bound {X.bound(e64, n):.2e} "
              f"(float64 restatement {e64:.2e})")
        assert err <= X.bound(e64, n), (comp, err, X.bound(e64, n))
    if c.hermi:
        assert not got[:, 1:].imag.any(), "hermi = 1: the gradient's imaginary part is exactly 0"
    # component 0 against fisdf_get_rho: the same sum in another order
    e0, e64 = X.rel_err(rho0, ref[:, 0]), X.rel_err(r64[:, 0], ref[:, 0])
    assert e0 <= X.bound(e64, n)
    same = np.array_equal(got[:, 0], rho0)
    print(f"{X.rho_id(c)}: component 0 {'equals' if same else 'differs from'} fisdf_get_rho bit for "
          f"bit (|diff| {np.abs(got[:, 0] - rho0).max():.2e})")
    assert X.rel_err(got[:, 0], rho0.astype(X.CLD)) <= 2 * X.bound(e64, n)


def test_rho_gga_refusals(env):
    torch, L, device = env
    c = X.RhoCase(8, 65, 2, 2, 1)
    f4, D = X.rho_inputs(c)
    fb, fv, ks, cs = _f4_buffer(torch, f4)
    Db, Dv = _inside(torch, D.astype(complex), NANC)
    rcs = c.ng + X.RPAD
    ob, ov = _inside(torch, np.full(c.nset * 4 * rcs, X.SENTINEL), X.SENTINEL)
    good = dict(ks=ks, cs=cs, nk=c.nk, ng=c.ng, nao=c.nao, nset=c.nset, hermi=1, rcs=rcs)
    for over in (dict(ng=0), dict(nk=0), dict(nao=0), dict(nset=0), dict(hermi=2), dict(hermi=-1),
                 dict(cs=c.ng * c.nao - 1), dict(ks=c.ng * c.nao - 1), dict(rcs=c.ng - 1)):
        a = dict(good, **over)
        rc = L.load().fisdf_get_rho_gga(device.ctx.h, L.ptr(fv), a["ks"], a["cs"], a["nk"], a["ng"],
                                        a["nao"], L.ptr(Dv), a["nset"], a["hermi"], L.ptr(ov), a["rcs"])
        device.ctx.call("fisdf_sync")
        assert rc != 0, over
        assert np.all(ob.cpu().numpy() == X.SENTINEL), over


# ================================================================ fisdf_gga_gram
SCALE = 0.37


def gram_call(env, c, f4, w, P):
    torch, L, device = env
    fb, fv, ks, cs = _f4_buffer(torch, f4)
    wcs = c.ng + X.WPAD
    wss = 4 * wcs + 3
    wh = np.full(c.nset * wss, np.nan)
    for s in range(c.nset):
        for comp in range(4):
            o = s * wss + comp * wcs
            wh[o:o + c.ng] = w[s, comp]
    wb, wv = _inside(torch, wh, np.nan)
    nout = c.nset * c.nk * c.nao * c.nao
    init = P.astype(complex).ravel() if c.acc else np.full(nout, X.SENTINEL)
    ob, ov = _inside(torch, init, X.SENTINEL)
    device.ctx.call("fisdf_gga_gram", L.ptr(fv), ks, cs, c.nk, c.ng, c.nao, L.ptr(wv), wss, wcs,
                    c.nset, SCALE, c.acc, L.ptr(ov))
    device.ctx.call("fisdf_sync")
    h = ob.cpu().numpy()
    assert np.all(h[:X.EDGE] == X.SENTINEL) and np.all(h[-X.EDGE:] == X.SENTINEL)
    return h[X.EDGE:X.EDGE + nout].reshape(c.nset, c.nk, c.nao, c.nao).copy()


@pytest.mark.parametrize("c", X.GRAM_CASES, ids=X.gram_id)
def test_gga_gram(env, c):
    f4, w, P = X.gram_inputs(c)
    got = gram_call(env, c, f4, w, P)
    assert np.array_equal(got, gram_call(env, c, f4, w, P)), "two runs differ"
    ref = X.gga_gram_ref(f4, w, SCALE, True) + (P.astype(X.CLD) if c.acc else 0)
    r64 = X.gga_gram_ref(f4, w, SCALE, False) + (P if c.acc else 0)
    n = 4 * c.ng
    err, e64 = X.rel_err(got, ref), X.rel_err(r64, ref)
    print(f"{X.gram_id(c)}: err {err:.2e} bound {X.bound(e64, n):.2e} (float64 restatement {e64:.2e})")
    assert err <= X.bound(e64, n)
    assert np.array_equal(got, got.conj().swapaxes(-1, -2)), "out != out^H bit for bit"
    assert not np.diagonal(got, axis1=-2, axis2=-1).imag.any()


def test_gga_gram_refusals(env):
    torch, L, device = env
    c = X.GramCase(8, 64, 2, 2, 0)
    f4, w, P = X.gram_inputs(c)
    fb, fv, ks, cs = _f4_buffer(torch, f4)
    wb, wv = _inside(torch, w.ravel(), np.nan)
    ob, ov = _inside(torch, np.full(c.nset * c.nk * c.nao * c.nao, X.SENTINEL), X.SENTINEL)
    good = dict(ks=ks, cs=cs, nk=c.nk, ng=c.ng, nao=c.nao, wss=4 * c.ng, wcs=c.ng, nset=c.nset)
    for over in (dict(ng=0), dict(nk=0), dict(nao=0), dict(nset=0), dict(cs=c.ng * c.nao - 1),
                 dict(ks=c.ng * c.nao - 1), dict(wcs=c.ng - 1), dict(wss=c.ng - 1)):
        a = dict(good, **over)
        rc = L.load().fisdf_gga_gram(device.ctx.h, L.ptr(fv), a["ks"], a["cs"], a["nk"], a["ng"],
                                     a["nao"], L.ptr(wv), a["wss"], a["wcs"], a["nset"], SCALE, 0,
                                     L.ptr(ov))
        device.ctx.call("fisdf_sync")
        assert rc != 0, over
        assert np.all(ob.cpu().numpy() == X.SENTINEL), over


# ================================================================ end to end
_DFS = {}


def df_of(name):
    from fisdf import ISDF
    if name not in _DFS:
        c, d = X.E2E_BY_NAME[name], X.e2e_data(name)
        df = ISDF(d.cell, d.cell.get_kpts(c.kmesh))
        df._kmesh()
        _DFS[name] = df
    return _DFS[name]


def small_budget(df):
    """a deriv_work_bytes whose block size is at least a quarter of the grid and does not divide it"""
    ngrid = int(np.prod(df.mesh))
    full = df.deriv_work_bytes
    try:
        for b in range(1 << 20, 1 << 26, 1 << 16):
            df.deriv_work_bytes = b
            try:
                nb = df.deriv_block_points()
            except ValueError:
                continue
            if ngrid // 4 <= nb < ngrid and ngrid % nb:
                return b, nb
    finally:
        df.deriv_work_bytes = full
    raise AssertionError("no budget found")


class budget:
    def __init__(self, df, b):
        self.df, self.b = df, b

    def __enter__(self):
        self.old = self.df.deriv_work_bytes
        self.df.deriv_work_bytes = self.b

    def __exit__(self, *a):
        self.df.deriv_work_bytes = self.old


@pytest.mark.parametrize("name", [c.name for c in X.E2E_CASES])
def test_get_rho_gga_end_to_end(env, name):
    c, d, df = X.E2E_BY_NAME[name], X.e2e_data(name), df_of(name)
    D = X.e2e_dms(d.cell, c.kmesh, 2)
    nk, nao = K.nk_of(c.kmesh), d.cell.nao_nr()
    ngrid = len(d.coords)
    got = df.get_rho(D, xctype="GGA")
    assert got.shape == (2, 4, ngrid) and got.dtype == np.float64
    assert np.array_equal(got, df.get_rho(D, xctype="GGA")), "two runs differ"
    ref, r64 = X.rho_gga_ref(d.f4, D, 1), X.rho_gga_ref(d.f4_64, D, 1, False)
    n = nk * nao * nao
    for comp in range(4):
        err, e64 = X.rel_err(got[:, comp], ref[:, comp].real), X.rel_err(r64[:, comp].real, ref[:, comp].real)
        print(f"{name} rho component {comp}: err {err:.2e} bound {X.bound(e64, n):.2e}")
        assert err <= X.bound(e64, n)
    one = df.get_rho(D[0], xctype="GGA")
    assert one.shape == (4, ngrid) and np.array_equal(one, got[0])
    gen = df.get_rho(D, hermi=0, xctype="GGA")
    assert gen.dtype == np.complex128 and X.rel_err(gen, ref) <= X.bound(X.rel_err(r64, ref), n)
    # rho is pointwise: it does not depend on the block size, bit for bit
    b, nb = small_budget(df)
    assert ngrid % nb and nb < ngrid
    with budget(df, b):
        assert np.array_equal(df.get_rho(D, xctype="GGA"), got)
        assert np.array_equal(df.get_rho(D, hermi=0, xctype="GGA"), gen)
    # xctype="LDA" is today's get_rho
    torch, L, device = env
    lda = df.get_rho(D)
    assert np.array_equal(df.get_rho(D, xctype="LDA"), lda) and lda.shape == (2, ngrid)
    f = df._grid_aos()
    r = df.device.empty((2, ngrid))
    df.device.ctx.call("fisdf_get_rho", L.ptr(f), ngrid * nao, nk, ngrid, nao,
                       L.ptr(df.device.to_dev(D.astype(complex))), 2, L.ptr(r))
    assert np.array_equal(lda, df.device.to_host(r).real)


@pytest.mark.parametrize("name", [c.name for c in X.E2E_CASES])
def test_nr_vxc_mat_and_get_kin_end_to_end(env, name):
    c, d, df = X.E2E_BY_NAME[name], X.e2e_data(name), df_of(name)
    nk, nao = K.nk_of(c.kmesh), d.cell.nao_nr()
    ngrid = len(d.coords)
    scale = X.LD(d.cell.vol) / ngrid
    rng = np.random.default_rng(17)
    wv = rng.standard_normal((2, 4, ngrid))
    worst = {}

    def close(tag, got, ref):
        e = float(np.abs(np.asarray(got, X.CLD) - ref).max())
        worst[tag] = max(worst.get(tag, 0.0), e)
        assert e <= X.JK_TOL, (tag, e)

    # GGA, two sets and one
    v = df.nr_vxc_mat(wv)
    assert v.shape == (2, nk, nao, nao)
    assert np.array_equal(v, df.nr_vxc_mat(wv)), "two runs differ"
    assert np.array_equal(v, v.conj().swapaxes(-1, -2))
    vref = X.gga_gram_ref(d.f4, wv, scale)
    close("V gga", v, vref)
    v1 = df.nr_vxc_mat(wv[1])
    assert v1.shape == (nk, nao, nao) and np.array_equal(v1, v[1])
    # LDA, two sets and one
    vl = df.nr_vxc_mat(wv[:, 0])
    assert vl.shape == (2, nk, nao, nao)
    close("V lda", vl, X.lda_gram_ref(d.f4, wv[:, 0], scale))
    assert np.array_equal(df.nr_vxc_mat(wv[0, 0]), vl[0])
    # the kinetic matrix
    t = df.get_kin()
    assert t.shape == (nk, nao, nao) and np.array_equal(t, df.get_kin())
    tref = X.kin_ref(d.f4, scale)
    close("T", t, tref)
    assert not t[0].imag.any(), "Gamma: the imaginary part is set to zero"
    # k-points of the mesh in another order, one k-point
    sel = [nk - 1, 0]
    close("V gga subset", df.nr_vxc_mat(wv, kpts=df.kpts[sel]), vref[:, sel])
    close("T subset", df.get_kin(kpts=df.kpts[sel]), tref[sel])
    assert df.get_kin(kpts=df.kpts[1]).shape == (nao, nao)
    assert df.nr_vxc_mat(wv, kpts=df.kpts[1]).shape == (2, nao, nao)
    # off the mesh: the band evaluator
    vb = df.nr_vxc_mat(wv, kpts=d.kband)
    assert vb.shape == (2, len(d.kband), nao, nao)
    close("V gga band", vb, X.gga_gram_ref(d.f4b, wv, scale))
    close("V lda band", df.nr_vxc_mat(wv[:, 0], kpts=d.kband), X.lda_gram_ref(d.f4b, wv[:, 0], scale))
    close("T band", df.get_kin(kpts=d.kband), X.kin_ref(d.f4b, scale))
    # another block size: block partials in block order, within the bound
    b, nb = small_budget(df)
    with budget(df, b):
        v2, t2 = df.nr_vxc_mat(wv), df.get_kin()
        assert np.array_equal(v2, df.nr_vxc_mat(wv)) and np.array_equal(t2, df.get_kin())
    v64 = X.gga_gram_ref(d.f4_64, wv, float(scale), False)
    t64 = X.kin_ref(d.f4_64, float(scale), False)
    assert X.rel_err(v2, vref) <= X.bound(X.rel_err(v64, vref), 4 * ngrid)
    assert X.rel_err(t2, tref) <= X.bound(X.rel_err(t64, tref), 3 * ngrid)
    assert X.rel_err(v, vref) <= X.bound(X.rel_err(v64, vref), 4 * ngrid)
    assert X.rel_err(t, tref) <= X.bound(X.rel_err(t64, tref), 3 * ngrid)
    close("V gga blocks", v2, vref)
    close("T blocks", t2, tref)
    print(f"{name} (blocks of {nb}): largest deviations " +
          ", ".join(f"{k} {e:.2e}" for k, e in worst.items()))


def test_errors(env):
    from fisdf import ISDF, kshard
    d = X.e2e_data("toy_113")
    df = df_of("toy_113")
    ngrid, nao = len(d.coords), d.cell.nao_nr()
    D = X.e2e_dms(d.cell, (1, 1, 3), 1)
    with pytest.raises(ValueError):
        df.get_rho(D, xctype="MGGA")
    for bad in (np.zeros((3, ngrid + 1)), np.zeros((2, 4, ngrid - 1)), np.zeros(ngrid + 1),
                np.zeros((2, 3, 4, ngrid)), np.zeros((4, ngrid), complex)):
        with pytest.raises(ValueError):
            df.nr_vxc_mat(bad)
    with pytest.raises(ValueError):
        df.nr_vxc_mat(np.zeros((4, ngrid)), xctype="mgga")
    # four LDA sets: the shape that reads as one GGA set unless told otherwise
    assert df.nr_vxc_mat(np.ones((4, ngrid)), xctype="LDA").shape == (4, 3, nao, nao)
    with budget(df, 1000):
        with pytest.raises(ValueError):
            df.get_kin()
    with pytest.raises(ValueError):
        list(df.aoR_loop(deriv=2))
    sh = ISDF(d.cell, d.cell.get_kpts((1, 1, 3)), comm=kshard.EmulatedGroup(0, 2))
    for call in (lambda: sh.get_rho(D, xctype="GGA"), lambda: sh.nr_vxc_mat(np.zeros((4, ngrid))),
                 lambda: sh.get_kin()):
        with pytest.raises(NotImplementedError):
            call()


def test_aor_loop_deriv1_and_the_pyscf_protocol(env):
    """aoR_loop(deriv=1) yields the (nk, 4, nb, nao) blocks; a cell without ``shells`` is asked
    for "GTOval_sph_deriv1" block by block and gives the same matrices."""
    name = "diamond_112"
    c, d, df = X.E2E_BY_NAME[name], X.e2e_data(name), df_of(name)
    nk, nao = K.nk_of(c.kmesh), d.cell.nao_nr()
    n = 0
    for (ao,), g0, g1 in df.aoR_loop(deriv=1, blksize=37):
        assert ao.shape == (nk, 4, g1 - g0, nao)
        err = X.col_err4(ao, d.f4[:, :, g0:g1])
        assert err.max() < 1e-12
        n += g1 - g0
    assert n == len(d.coords)

    class Proto:
        """PySCF's Cell protocol: no shells, pbc_eval_gto by name"""
        def __init__(self, cell):
            self._c = cell
            self.mesh, self.asked = cell.mesh, []
            self.vol = cell.vol

        def pbc_eval_gto(self, name, coords, kpts=None):
            self.asked.append((name, len(coords)))
            return self._c.pbc_eval_gto(name, coords, kpts=kpts)

        def __getattr__(self, k):
            if k == "shells":
                raise AttributeError(k)
            return getattr(self._c, k)

    from fisdf import ISDF
    p = Proto(d.cell)
    dfp = ISDF(p, d.cell.get_kpts(c.kmesh))
    dfp.blksize = 29
    t = dfp.get_kin()
    assert ("GTOval_sph_deriv1", 29) in p.asked
    assert np.abs(t - X.kin_ref(d.f4, X.LD(d.cell.vol) / len(d.coords))).max() <= X.JK_TOL


# ================================================================ the identity
def test_density_and_potential_agree_through_the_energy(env):
    """e(rho, sigma) = a rho^2 + b sigma makes E[D] quadratic in D, so the central difference with
    step 1 is exact up to rounding: (E[D + d] - E[D - d]) / 2 = (1/nk) sum_k Re tr(V_k d_k) with
    V = nr_vxc_mat([2 a rho, 2 b grad rho]).  Both sides from the device methods, against the same
    identity in long double; a wrong sign, factor 1/2 or index order between the density and the
    potential kernels breaks it."""
    name = "toy_222"
    c, d, df = X.E2E_BY_NAME[name], X.e2e_data(name), df_of(name)
    nk, ngrid, vol = K.nk_of(c.kmesh), len(d.coords), d.cell.vol
    Ds = X.e2e_dms(d.cell, c.kmesh, 2, seed=9)
    D, dl = Ds[0], Ds[1] - np.eye(d.cell.nao_nr())
    assert np.array_equal((D + dl) - (D - dl), 2 * dl)

    def sides(rho_of, vxc_of, tr_dt):
        ep, em = X.energy(rho_of(D + dl), vol), X.energy(rho_of(D - dl), vol)
        V = vxc_of(X.identity_wv(rho_of(D)))
        rhs = sum(np.trace(np.asarray(V[k], tr_dt) @ dl[k].astype(tr_dt)).real for k in range(nk)) / nk
        return (ep - em) / 2, rhs

    dev = sides(lambda m: df.get_rho(m, xctype="GGA"), lambda w: df.nr_vxc_mat(w), np.complex128)
    ref = sides(lambda m: X.rho_gga_ref(d.f4, m[None], 1)[0].real,
                lambda w: X.gga_gram_ref(d.f4, w[None], X.LD(vol) / ngrid)[0], X.CLD)
    f64 = sides(lambda m: X.rho_gga_ref(d.f4_64, m[None], 1, False)[0].real,
                lambda w: X.gga_gram_ref(d.f4_64, w[None], vol / ngrid, False)[0], np.complex128)
    assert abs(ref[0] - ref[1]) <= 1e-13 * abs(ref[0]), "the references do not satisfy the identity"
    den = abs(ref[0])
    tol = [X.bound(float(abs(f64[i] - ref[i]) / den), ngrid) for i in (0, 1)]
    err = [float(abs(X.LD(dev[i]) - ref[i]) / den) for i in (0, 1)]
    print(f"identity: lhs {float(dev[0]):.15e} rhs {float(dev[1]):.15e} reference {float(ref[0]):.15e}; "
          f"errors {err[0]:.2e} {err[1]:.2e}, bounds {tol[0]:.2e} {tol[1]:.2e}")
    assert err[0] <= tol[0] and err[1] <= tol[1]
    assert abs(dev[0] - dev[1]) / float(den) <= tol[0] + tol[1]
