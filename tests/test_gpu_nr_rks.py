"""The device functional and the fused RKS step against long-double references: fisdf_xc_eval on
the point tables, fisdf_nr_rks_block on random blocks, and ISDF.eval_xc / ISDF.nr_rks end to end
on the toy and diamond cells, tied to the density through the energy.

Cases, references and bounds live in tests/func_cases.py (tests/test_func_cases.py checks them on
the CPU).  Inputs are views inside NaN with padded strides, outputs views inside the sentinel
(7 + 7j, 7.0 for the real ones), which has to come back intact; every entry runs twice and the two
runs are compared bit for bit.  The functional's outputs may be factor_cases.bound(err64, 1) times
their scale from the reference (func_cases' module text); matrices and sums follow test_gpu_xc.py.

The end-to-end cases use one density matrix of xc_cases.e2e_dms per cell.  The two-set case runs
on the toy cells only, not on diamond_112: the second e2e_dms set has a negative density
(-2.0e-4) at one grid point of the diamond cell, and no end-to-end point may be at or below the
cut (func_cases.E2E_TWO_SETS; tests/test_func_cases.py checks the smallest densities).

Measured on one MI355X (largest error / bound; profiles/nr_rks/gpu_tests_figures.txt): fisdf_xc_eval
0.18 (e) and 0.32 (wv) for LDA, 0.16 and 0.10 for PBE, errors 1e-16 to 2.9e-15 of the scale; the
fused block 0.009 (vxc) and 0.06 (sums); end to end 0.016 at most, V within 3.7e-15 Ha; the energy
difference 6.5e-15 of its value (bound 3.8e-13).
"""
import numpy as np
import pytest

import func_cases as Fc
import kmesh_cases as K
import xc_cases as X

pytestmark = pytest.mark.gpu

NANC = complex(np.nan, np.nan)
RSENT = 7.0


@pytest.fixture(scope="module")
def env():
    import torch
    from fisdf import _lib
    from fisdf.isdf import _Device
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch, _lib, _Device()


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


def _strided(nset, ncomp, ng, ss, cs):
    """flat indices (nset, ncomp, ng) of the logical elements of a padded array"""
    return (np.arange(nset)[:, None, None] * ss + np.arange(ncomp)[None, :, None] * cs
            + np.arange(ng)[None, None, :])


def _unpack(buf, idx, total, fill):
    """the logical elements of a padded output; everything else must still be the sentinel"""
    h = buf.cpu().numpy()
    body = h[X.EDGE:X.EDGE + total]
    out = body[idx].copy()
    rest = np.ones(h.size, bool)
    rest[X.EDGE + idx.ravel()] = False
    assert np.all(h[rest] == fill), "an element outside the output was written"
    return out


# ================================================================ fisdf_xc_eval
def xc_strides(c):
    ncomp = 4 if c.family == Fc.GGA else 1
    rcs = c.ng + X.RPAD
    wcs = c.ng + X.WPAD
    return dict(ncomp=ncomp, rcs=rcs, rss=ncomp * rcs + Fc.SPAD, ess=c.ng + Fc.EPAD, wcs=wcs,
                wss=ncomp * wcs + Fc.SPAD)


def xc_call(env, c, rho, want_e=True, want_wv=True, nan_imag=False, cut=Fc.RHO_CUT, tight=False,
            **over):
    """fisdf_xc_eval on a padded rho; over replaces single arguments (the refusals).  Returns
    (rc, message, e or None, wv or None); refused calls check that both outputs are intact.
    tight: every stride at its minimum."""
    torch, L, device = env
    st = xc_strides(c)
    ncomp = st["ncomp"]
    if tight:
        st = dict(ncomp=ncomp, rcs=c.ng, rss=ncomp * c.ng, ess=c.ng, wcs=c.ng, wss=ncomp * c.ng)
    r = np.asarray(rho, float).reshape(c.nset, ncomp, c.ng)
    ridx = _strided(c.nset, ncomp, c.ng, st["rss"], st["rcs"])
    rtot = c.nset * st["rss"]
    rh = np.full(rtot, NANC)
    vals = r.astype(complex)
    if nan_imag:
        vals.imag = np.nan
    rh[ridx] = vals
    rb, rv = _inside(torch, rh, NANC)
    etot, wtot = c.nset * st["ess"], c.nset * st["wss"]
    eb, ev = _inside(torch, np.full(etot, RSENT), RSENT)
    wb, wv = _inside(torch, np.full(wtot, RSENT), RSENT)
    a = dict(family=c.family, cx=c.cx, cc=c.cc, cut=cut, ng=c.ng, nset=c.nset, **st)
    a.update(over)
    lib = L.load()
    rc = lib.fisdf_xc_eval(device.ctx.h, a["family"], a["cx"], a["cc"], a["cut"], L.ptr(rv), a["rss"],
                           a["rcs"], a["ng"], a["nset"], L.ptr(ev) if want_e else None, a["ess"],
                           L.ptr(wv) if want_wv else None, a["wss"], a["wcs"])
    msg = lib.fisdf_last_error(device.ctx.h).decode() if rc else ""
    device.ctx.call("fisdf_sync")
    eidx = _strided(c.nset, 1, c.ng, st["ess"], 0)[:, 0]
    widx = _strided(c.nset, ncomp, c.ng, st["wss"], st["wcs"])
    if rc or not want_e:
        assert np.all(eb.cpu().numpy() == RSENT), "e was written"
    if rc or not want_wv:
        assert np.all(wb.cpu().numpy() == RSENT), "wv was written"
    e = _unpack(eb, eidx, etot, RSENT) if want_e and not rc else None
    w = _unpack(wb, widx, wtot, RSENT) if want_wv and not rc else None
    return rc, msg, e, w


@pytest.mark.parametrize("c", Fc.XC_CASES, ids=Fc.xc_id)
def test_xc_eval(env, c):
    rho, ref, (e64, w64) = Fc.xc_data(c)
    rc, _, e, w = xc_call(env, c, rho)
    assert rc == 0
    rc2, _, e2, w2 = xc_call(env, c, rho)
    assert rc2 == 0 and np.array_equal(e, e2) and np.array_equal(w, w2), "two runs differ"
    assert np.isfinite(e).all() and np.isfinite(w).all()
    ee, ew = Fc.scaled_err(e, ref.e, ref.se), Fc.scaled_err(w, ref.wv, ref.sw)
    be, bw = Fc.bound(e64, 1), Fc.bound(w64, 1)
    print(f"{Fc.xc_id(c)}: e err {ee:.2e} bound {be:.2e} ratio {ee / be:.3f}; "
          f"wv err {ew:.2e} bound {bw:.2e} ratio {ew / bw:.3f}")
    assert ee <= be and ew <= bw
    # exact zeros at and below the cut (scaled_err has checked every entry of scale 0)
    n = np.asarray(rho).reshape(c.nset, -1, c.ng)[:, 0]
    dead = n <= Fc.RHO_CUT
    assert not e[dead].any() and not w.transpose(0, 2, 1)[dead].any()
    if c.ng >= 255:
        assert dead.sum() >= 4 * c.nset and (e[~dead] != 0).all()


def test_xc_eval_optional_outputs_and_imaginary_parts(env):
    for fam in (Fc.LDA, Fc.GGA):
        c = Fc.XcCase(fam, 0.75, 1.0, 257, 3)
        rho = Fc.xc_data(c)[0]
        _, _, e, w = xc_call(env, c, rho)
        rc, _, e1, w1 = xc_call(env, c, rho, want_wv=False)
        assert rc == 0 and w1 is None and np.array_equal(e1, e)
        rc, _, e1, w1 = xc_call(env, c, rho, want_e=False)
        assert rc == 0 and e1 is None and np.array_equal(w1, w)
        rc, _, e1, w1 = xc_call(env, c, rho, want_e=False, want_wv=False)
        assert rc == 0
        rc, _, e1, w1 = xc_call(env, c, rho, nan_imag=True)
        assert rc == 0 and np.array_equal(e1, e) and np.array_equal(w1, w), "Im rho was read"
        # the cut is an argument: a larger one zeroes more points, 0 keeps every positive one
        rc, _, e1, w1 = xc_call(env, c, rho, cut=1e-3)
        n = np.asarray(rho).reshape(3, -1, 257)[:, 0]
        assert rc == 0 and not e1[n <= 1e-3].any() and np.array_equal(e1[n > 1e-3], e[n > 1e-3])


def test_xc_eval_refusals(env):
    c = Fc.XcCase(Fc.GGA, 1.0, 1.0, 255, 3)
    rho = Fc.xc_data(c)[0]
    st = xc_strides(c)
    overs = [dict(family=2), dict(family=-1), dict(ng=0), dict(nset=0), dict(ng=-3),
             dict(rcs=c.ng - 1), dict(rss=3 * st["rcs"] + c.ng - 1), dict(ess=c.ng - 1),
             dict(wcs=c.ng - 1), dict(wss=3 * st["wcs"] + c.ng - 1), dict(cut=-1e-300),
             dict(cut=np.nan), dict(cx=np.inf), dict(cc=np.nan), dict(cx=-np.inf)]
    for over in overs:
        rc, msg, _, _ = xc_call(env, c, rho, **over)
        assert rc != 0 and msg, over
    cl = Fc.XcCase(Fc.LDA, 1.0, 1.0, 255, 3)
    for over in (dict(rss=cl.ng - 1), dict(wss=cl.ng - 1), dict(ess=cl.ng - 1)):
        rc, msg, _, _ = xc_call(env, cl, Fc.xc_data(cl)[0], **over)
        assert rc != 0 and msg, over
    # a stride at its minimum is taken
    for case in (c, cl):
        rho = Fc.xc_data(case)[0]
        rc, _, e, w = xc_call(env, case, rho, tight=True)
        _, _, e0, w0 = xc_call(env, case, rho)
        assert rc == 0 and np.array_equal(e, e0) and np.array_equal(w, w0)


# ================================================================ fisdf_nr_rks_block
def block_call(env, c, stages=False, **over):
    """fisdf_nr_rks_block (stages: the three entries one after another and no sums) on the case's
    padded block.  Returns (rc, message, vxc, sums)."""
    torch, L, device = env
    f4, D, P, S0 = Fc.block_inputs(c)
    cx, cc = Fc.BLOCK_MIX
    fb, fv, ks, cs = _f4_buffer(torch, f4)
    Db, Dv = _inside(torch, D.astype(complex), NANC)
    nout = c.nset * c.nk * c.nao * c.nao
    ob, ov = _inside(torch, P.astype(complex).ravel() if c.acc else np.full(nout, X.SENTINEL),
                     X.SENTINEL)
    sb, sv = _inside(torch, S0.ravel() if c.acc else np.full(2 * c.nset, RSENT), RSENT)
    a = dict(family=Fc.GGA, cx=cx, cc=cc, cut=Fc.RHO_CUT, ks=ks, cs=cs, nk=c.nk, ng=c.ng, nao=c.nao,
             nset=c.nset, scale=Fc.BLOCK_SCALE, acc=c.acc, null_sums=False, null_vxc=False)
    a.update(over)
    lib = L.load()
    if stages:
        rho = device.empty((c.nset, 4, c.ng))
        wv = device.empty((c.nset, 4, c.ng), "f64")
        device.ctx.call("fisdf_get_rho_gga", L.ptr(fv), ks, cs, c.nk, c.ng, c.nao, L.ptr(Dv), c.nset,
                        1, L.ptr(rho), c.ng)
        device.ctx.call("fisdf_xc_eval", Fc.GGA, cx, cc, Fc.RHO_CUT, L.ptr(rho), 4 * c.ng, c.ng, c.ng,
                        c.nset, None, c.ng, L.ptr(wv), 4 * c.ng, c.ng)
        device.ctx.call("fisdf_gga_gram", L.ptr(fv), ks, cs, c.nk, c.ng, c.nao, L.ptr(wv), 4 * c.ng,
                        c.ng, c.nset, Fc.BLOCK_SCALE, c.acc, L.ptr(ov))
        rc = 0
    else:
        rc = lib.fisdf_nr_rks_block(device.ctx.h, a["family"], a["cx"], a["cc"], a["cut"], L.ptr(fv),
                                    a["ks"], a["cs"], a["nk"], a["ng"], a["nao"], L.ptr(Dv), a["nset"],
                                    a["scale"], a["acc"], None if a["null_vxc"] else L.ptr(ov),
                                    None if a["null_sums"] else L.ptr(sv))
    msg = lib.fisdf_last_error(device.ctx.h).decode() if rc else ""
    device.ctx.call("fisdf_sync")
    h, hs = ob.cpu().numpy(), sb.cpu().numpy()
    assert np.all(h[:X.EDGE] == X.SENTINEL) and np.all(h[-X.EDGE:] == X.SENTINEL)
    assert np.all(hs[:X.EDGE] == RSENT) and np.all(hs[-X.EDGE:] == RSENT)
    return (rc, msg, h[X.EDGE:X.EDGE + nout].reshape(c.nset, c.nk, c.nao, c.nao).copy(),
            hs[X.EDGE:X.EDGE + 2 * c.nset].reshape(c.nset, 2).copy())


@pytest.mark.parametrize("c", Fc.BLOCK_CASES, ids=Fc.block_id)
def test_nr_rks_block(env, c):
    f4, D, P, S0 = Fc.block_inputs(c)
    rc, _, v, s = block_call(env, c)
    assert rc == 0
    rc2, _, v2, s2 = block_call(env, c)
    assert rc2 == 0 and np.array_equal(v, v2) and np.array_equal(s, s2), "two runs differ"
    w, d = Fc.block_ref(c)
    vref = w.vxc + (P.astype(X.CLD) if c.acc else 0)
    v64 = d.vxc + (P if c.acc else 0)
    err, e64 = X.rel_err(v, vref), X.rel_err(v64, vref)
    print(f"{Fc.block_id(c)}: vxc err {err:.2e} bound {X.bound(e64, 4 * c.ng):.2e} "
          f"ratio {err / X.bound(e64, 4 * c.ng):.3f}")
    assert err <= X.bound(e64, 4 * c.ng)
    sref = w.sums + (S0.astype(X.LD) if c.acc else 0)
    s64 = d.sums + (S0 if c.acc else 0)
    for j, tag in enumerate(("sum n", "sum e")):
        err, e64 = X.rel_err(s[:, j], sref[:, j]), X.rel_err(s64[:, j], sref[:, j])
        print(f"{Fc.block_id(c)}: {tag} err {err:.2e} bound {X.bound(e64, c.ng):.2e} "
              f"ratio {err / X.bound(e64, c.ng):.3f}")
        assert err <= X.bound(e64, c.ng)
    # the bits of the three entries called one after another
    _, _, v3, _ = block_call(env, c, stages=True)
    assert np.array_equal(v, v3), "the fused block differs from its three stages"
    assert np.array_equal(v, v.conj().swapaxes(-1, -2)), "out != out^H bit for bit"
    assert not np.diagonal(v, axis1=-2, axis2=-1).imag.any()


def test_nr_rks_block_refusals(env):
    for acc in (0, 1):
        c = Fc.BlockCase(8, 65, 2, 3, acc)
        f4, D, P, S0 = Fc.block_inputs(c)
        for over in (dict(family=Fc.LDA), dict(family=2), dict(ng=0), dict(nk=0), dict(nao=0),
                     dict(nset=0), dict(cs=c.ng * c.nao - 1), dict(ks=c.ng * c.nao - 1),
                     dict(cut=-1.0), dict(cut=np.nan), dict(cx=np.inf), dict(cc=np.nan),
                     dict(scale=np.nan), dict(null_sums=True), dict(null_vxc=True)):
            rc, msg, v, s = block_call(env, c, **over)
            assert rc != 0 and msg, over
            if acc:
                assert np.array_equal(v, P) and np.array_equal(s, S0), over
            else:
                assert np.all(v == X.SENTINEL) and np.all(s == RSENT), over


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


def small_budget(df, nset=1):
    """a deriv_work_bytes whose nr_rks block is at least a quarter of the grid and does not divide
    it"""
    ngrid = int(np.prod(df.mesh))
    full = df.deriv_work_bytes
    try:
        for b in range(1 << 20, 1 << 26, 1 << 16):
            df.deriv_work_bytes = b
            try:
                nb = df.nr_rks_block_points(nset)
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


def stitched(df, xc, D):
    """nr_vxc_mat(eval_xc(get_rho)): the route through the host"""
    fam = Fc.E2E_XC[xc][0]
    rho = df.get_rho(D, xctype="GGA" if fam == Fc.GGA else "LDA")
    e, wv = df.eval_xc(xc, rho)
    return df.nr_vxc_mat(wv, xctype="GGA" if fam == Fc.GGA else "LDA"), e, rho


def check_against(name, got, ref, f64, tag):
    """(nelec, exc, vxc) arrays over the sets against the long-double pipeline"""
    d = X.e2e_data(name)
    ngrid = len(d.coords)
    nelec, exc, vxc = got
    err, e64 = X.rel_err(vxc, ref.vxc), X.rel_err(f64.vxc, ref.vxc)
    dev = float(np.abs(np.asarray(vxc, X.CLD) - ref.vxc).max())
    out = [f"{tag}: vxc err {err:.2e} bound {X.bound(e64, 4 * ngrid):.2e} ratio "
           f"{err / X.bound(e64, 4 * ngrid):.3f} (largest deviation {dev:.2e} Ha)"]
    assert err <= X.bound(e64, 4 * ngrid) and dev <= X.JK_TOL
    for j, (x, what) in enumerate(((nelec, "nelec"), (exc, "exc"))):
        err, e64 = X.rel_err(np.atleast_1d(x), ref.sums[:, j]), X.rel_err(f64.sums[:, j], ref.sums[:, j])
        out.append(f"{what} err {err:.2e} bound {X.bound(e64, ngrid):.2e} ratio "
                   f"{err / X.bound(e64, ngrid):.3f}")
        assert err <= X.bound(e64, ngrid), what
    print("; ".join(out))


@pytest.mark.parametrize("xc", list(Fc.E2E_XC))
@pytest.mark.parametrize("name", [c.name for c in X.E2E_CASES])
def test_nr_rks_end_to_end(env, name, xc):
    c, d, df = X.E2E_BY_NAME[name], X.e2e_data(name), df_of(name)
    nk, nao, ngrid = K.nk_of(c.kmesh), d.cell.nao_nr(), len(d.coords)
    D = Fc.e2e_dm(name)[0]
    assert df.nr_rks_block_points() >= ngrid, "the default budget holds the grid in one block"
    nelec, exc, vxc = df.nr_rks(xc.upper(), D)
    assert isinstance(nelec, float) and isinstance(exc, float) and vxc.shape == (nk, nao, nao)
    again = df.nr_rks(xc, D)
    assert again[:2] == (nelec, exc) and np.array_equal(again[2], vxc), "two runs differ"
    ref, f64 = Fc.e2e_ref(name, xc)
    check_against(name, (nelec, exc, vxc[None]), ref, f64, f"{name} {xc}")
    fam = Fc.E2E_XC[xc][0]
    if fam == Fc.GGA:
        assert np.array_equal(vxc, vxc.conj().swapaxes(-1, -2)), "vxc != vxc^H bit for bit"
    else:
        assert np.abs(vxc - vxc.conj().swapaxes(-1, -2)).max() <= 4 * ngrid * X.EPS * np.abs(vxc).max()
    # nelec is the trace of D S on the same quadrature
    S = df.device.to_host(df.get_ovlp())
    tr = sum(np.trace(D[k].astype(X.CLD) @ S[k].astype(X.CLD)).real for k in range(nk)) / nk
    e64 = X.rel_err(f64.sums[:, 0], ref.sums[:, 0])
    assert abs(nelec - tr) / abs(tr) <= X.bound(e64, ngrid), (nelec, float(tr))
    # one block: the bits of the route through the host
    v_host, e_host, rho = stitched(df, xc, D)
    assert np.array_equal(vxc, v_host), "nr_rks differs from nr_vxc_mat(eval_xc(get_rho))"
    assert abs(d.cell.vol / ngrid * e_host.sum() - exc) <= ngrid * X.EPS * abs(exc)
    # a block that does not divide the grid: block partials in block order, equal to rounding
    b, nb = small_budget(df)
    with budget(df, b):
        assert df.nr_rks_block_points() == nb and ngrid % nb
        n2, x2, v2 = df.nr_rks(xc, D)
        again = df.nr_rks(xc, D)
        assert again[:2] == (n2, x2) and np.array_equal(again[2], v2)
    check_against(name, (n2, x2, v2[None]), ref, f64, f"{name} {xc} (blocks of {nb})")
    assert abs(n2 - nelec) <= ngrid * X.EPS * abs(nelec) and abs(x2 - exc) <= ngrid * X.EPS * abs(exc)
    if fam == Fc.GGA:
        assert np.array_equal(v2, v2.conj().swapaxes(-1, -2))
    else:
        assert np.array_equal(v2, vxc) and (n2, x2) == (nelec, exc), "LDA takes no derivative blocks"


@pytest.mark.parametrize("name", [c.name for c in X.E2E_CASES])
def test_pbe0_is_the_scaled_mix(env, name):
    from fisdf import hybrid_coeff, xc
    d, df = X.e2e_data(name), df_of(name)
    ngrid = len(d.coords)
    D = Fc.e2e_dm(name)[0]
    n0, e0, v0 = df.nr_rks("pbe0", D)
    nx, ex, vx = df.nr_rks(xc.Functional("GGA", 1, 0), D)
    nc, ec, vc = df.nr_rks(xc.Functional("GGA", 0, 1), D)
    scale = np.abs(vx).max() + np.abs(vc).max()
    assert np.abs(v0 - (0.75 * vx + vc)).max() <= 4 * ngrid * X.EPS * scale
    assert abs(e0 - (0.75 * ex + ec)) <= ngrid * X.EPS * (abs(ex) + abs(ec))
    assert n0 == nx == nc
    same = df.nr_rks(xc.Functional("GGA", 0.75, 1.0, 0.25), D)
    assert same[:2] == (n0, e0) and np.array_equal(same[2], v0)
    assert hybrid_coeff("pbe0") == 0.25
    # nothing local: zeros, and an object that has not touched the device still has not
    from fisdf import ISDF
    c = X.E2E_BY_NAME[name]
    fresh = ISDF(d.cell, d.cell.get_kpts(c.kmesh))
    nh, eh, vh = fresh.nr_rks("hf", D)
    assert (nh, eh) == (0.0, 0.0) and vh.shape == D.shape and not vh.any() and fresh._d is None
    nh, eh, vh = fresh.nr_rks("HF", D[None].repeat(2, axis=0))
    assert nh.shape == eh.shape == (2,) and vh.shape == (2,) + D.shape and fresh._d is None


@pytest.mark.parametrize("name", [c.name for c in X.E2E_CASES])
def test_callable_functional(env, name):
    d, df = X.e2e_data(name), df_of(name)
    ngrid, vol = len(d.coords), d.cell.vol
    D = Fc.e2e_dm(name)[0]
    calls = []

    def poly(rho):
        calls.append(rho.shape)
        a, b = X.IDENTITY_A, X.IDENTITY_B
        return a * rho[0] ** 2 + b * (rho[1:] ** 2).sum(axis=0), X.identity_wv(rho)

    rho = df.get_rho(D, xctype="GGA")
    want = df.nr_vxc_mat(X.identity_wv(rho))
    nelec, exc, vxc = df.nr_rks(poly, D)
    assert calls == [(4, ngrid)]
    assert np.array_equal(vxc, want), "the callable route differs from nr_vxc_mat(f(get_rho))"
    assert abs(exc - X.energy(rho, vol)) <= ngrid * X.EPS * abs(exc)
    assert abs(nelec - vol / ngrid * rho[0].sum()) <= ngrid * X.EPS * nelec
    # the device functional wrapped as a callable: the built-in route, under the same budget
    for b in (df.deriv_work_bytes, small_budget(df)[0]):
        with budget(df, b):
            n1, e1, v1 = df.nr_rks("pbe", D)
            n2, e2, v2 = df.nr_rks(lambda r: df.eval_xc("pbe", r), D)
        assert np.array_equal(v1, v2), "the callable route differs from the built-in one"
        assert abs(n1 - n2) <= ngrid * X.EPS * n1 and abs(e1 - e2) <= ngrid * X.EPS * abs(e1)
    with pytest.raises(ValueError):
        df.nr_rks(lambda r: (r[0], r[:1]), D)


@pytest.mark.parametrize("name", Fc.E2E_TWO_SETS)
def test_two_sets_are_two_single_sets(env, name):
    c, d, df = X.E2E_BY_NAME[name], X.e2e_data(name), df_of(name)
    nk, nao = K.nk_of(c.kmesh), d.cell.nao_nr()
    D = Fc.e2e_dm(name, 2)
    for xc in ("lda", "pbe"):
        nelec, exc, vxc = df.nr_rks(xc, D)
        assert nelec.shape == exc.shape == (2,) and vxc.shape == (2, nk, nao, nao)
        for s in range(2):
            n1, e1, v1 = df.nr_rks(xc, D[s])
            assert (n1, e1) == (nelec[s], exc[s]) and np.array_equal(v1, vxc[s]), (xc, s)
        ref, f64 = Fc.e2e_ref(name, xc, 2)
        check_against(name, (nelec, exc, vxc), ref, f64, f"{name} {xc} two sets")


# ================================================================ the energy tie
def test_energy_difference_against_long_double(env):
    """(exc[D + d] - exc[D - d]) / 2 from the device against the same expression in long double
    (tests/test_func_cases.py shows it approaching (1/nk) sum_k Re tr(V_k d_k) as d halves): the
    density, the functional and the block sums together, at the accuracy the difference leaves."""
    name = "toy_222"
    c, d, df = X.E2E_BY_NAME[name], X.e2e_data(name), df_of(name)
    nk, ngrid, vol = K.nk_of(c.kmesh), len(d.coords), d.cell.vol
    D, dl = Fc.tie_matrices(name)
    assert np.array_equal((D + dl) - (D - dl), 2 * dl)

    def diff(exc_of):
        return (exc_of(D + dl) - exc_of(D - dl)) / 2

    def pipeline(wide):
        f4, sc = (d.f4, X.LD(vol) / ngrid) if wide else (d.f4_64, vol / ngrid)
        return lambda m: Fc.block_pipeline(f4, m[None], Fc.GGA, 1.0, 1.0, Fc.RHO_CUT, sc, wide).sums[0, 1]

    dev = diff(lambda m: df.nr_rks("pbe", m)[1])
    ref, f64 = diff(pipeline(True)), diff(pipeline(False))
    V = df.nr_rks("pbe", D)[2]
    tr = sum(np.trace(V[k] @ dl[k]).real for k in range(nk)) / nk
    tol = X.bound(float(abs(f64 - ref) / abs(ref)), ngrid)
    err = float(abs(X.LD(dev) - ref) / abs(ref))
    print(f"energy tie: device {dev:.15e} reference {float(ref):.15e} tr(V d)/nk {tr:.15e}; "
          f"err {err:.2e} bound {tol:.2e} ratio {err / tol:.3f}")
    assert err <= tol
    assert abs(tr - dev) <= 1e-3 * abs(dev)      # the step's truncation error, 1.3e-5 at toy_113


# ================================================================ errors
def test_errors(env):
    from fisdf import ISDF, kshard
    name = "toy_113"
    d, df = X.e2e_data(name), df_of(name)
    ngrid, nao = len(d.coords), d.cell.nao_nr()
    D = Fc.e2e_dm(name)[0]
    fresh = ISDF(d.cell, d.cell.get_kpts((1, 1, 3)))
    for bad in ("svwn", "b3lyp", "hse06", "scan", 7):
        with pytest.raises(ValueError, match="pbe0"):
            fresh.nr_rks(bad, D)
        with pytest.raises(ValueError):
            fresh.eval_xc(bad, np.ones((4, 5)))
    assert fresh._d is None, "the name is checked before the device is touched"
    for hermi in (0, 2):
        with pytest.raises(ValueError):
            df.nr_rks("pbe", D, hermi=hermi)
    for xc, bad in (("pbe", np.ones(ngrid)), ("pbe", np.ones((3, ngrid))), ("pbe", np.ones((2, 3, 4, ngrid))),
                    ("pbe", np.ones((2, 5, ngrid))), ("lda", np.ones((2, 4, ngrid))), ("lda", np.ones(())),
                    ("pbe", np.ones((4, 0))), ("hf", np.ones(ngrid))):
        with pytest.raises(ValueError):
            df.eval_xc(xc, bad)
    # shapes of eval_xc: a block of any length, with and without the set axis
    e, wv = df.eval_xc("pbe", np.ones((4, 5)))
    assert e.shape == (5,) and wv.shape == (4, 5)
    e, wv = df.eval_xc("lda", np.ones((2, 5)))
    assert e.shape == (2, 5) and wv.shape == (2, 5)
    with budget(df, 1000):
        with pytest.raises(ValueError):
            df.nr_rks("pbe", D)
    sh = ISDF(d.cell, d.cell.get_kpts((1, 1, 3)), comm=kshard.EmulatedGroup(0, 2))
    for xc in ("pbe", "lda", lambda r: (r[0], r)):
        with pytest.raises(NotImplementedError):
            sh.nr_rks(xc, D)
