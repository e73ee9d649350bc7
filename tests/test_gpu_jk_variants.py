"""The layer that composes the factors into J, K and (ij|kl) on the device, every entry through the
C ABI against the long-double references of tests/jk_cases.py: fisdf_get_j_rows,
fisdf_get_j_band_rows, fisdf_get_k_rows, fisdf_get_k_rows_local, fisdf_get_j / fisdf_get_k,
fisdf_get_eri, the unsharded fisdf_get_jk, the same entries as the ISDF object drives them on a
real build, and fisdf_unpack_slices.

Inputs live in NaN-guarded buffers (test_gpu_factor_chain.Buf), outputs in buffers of NaN between
sentinel guards, so an element a call does not write, or a guard it does, fails the case.  Every
comparison is with a long-double reference under jk_cases' bound (per (set, k) block: 16 times
the float64 restatement's own error, floored at n eps scale) or a bitwise identity; the route of a
K case is asserted before its numbers are looked at; every refused call is followed by a valid one
on the same context that meets its bound.  The largest error / bound of each family is printed
when the module ends."""
import ctypes as C
import os

import numpy as np
import pytest

import jk_cases as J
from kmesh_cases import reps
from test_gpu_factor_chain import SENT, Buf, env  # noqa: F401  (env: the module's context fixture)

pytestmark = pytest.mark.gpu

NANC = complex(np.nan, np.nan)
J_REG_ROUTE = 0     # h_route[0] of fisdf_kmesh_plan: the k-mesh has register kernels
WORST = {}          # family -> (largest error / bound, comparisons, where)


@pytest.fixture(scope="module", autouse=True)
def figures():
    yield
    for fam, (r, n, where) in sorted(WORST.items()):
        print(f"jk {fam}: {n} comparisons, largest error / bound {r:.3f} at {where}")


@pytest.fixture(autouse=True)
def no_k_dft(monkeypatch):
    monkeypatch.delenv("FISDF_K_DFT", raising=False)


def note(fam, r, where):
    old = WORST.get(fam, (-1.0, 0, ""))
    WORST[fam] = (r, old[1] + 1, where) if r > old[0] else (old[0], old[1] + 1, old[2])
    assert r <= 1, (fam, where, r)


def compare(fam, where, got, ref, tol):
    r = J.worst_ratio(J.block_err(got, ref), tol)
    print(f"{fam} {where}: error / bound {r:.3f}")
    note(fam, r, where)


def in_buf(torch, a):
    a = np.ascontiguousarray(a)
    if np.iscomplexobj(a):
        return Buf(torch, a.size, NANC).put(a.astype(complex))
    return Buf(torch, a.size, float("nan"), torch.float64).put(a.astype(float))


def out_buf(torch, n, fill=NANC):
    """n elements of `fill` between sentinel guards."""
    return Buf(torch, n, SENT).put(np.full(n, fill))


def km3(kmesh):
    return (C.c_int * 3)(*kmesh)


def lattice():
    return (C.c_double * 9)(*J.LATTICE.ravel())


def plan_route(L, kmesh, ncol, nao, nip):
    route = (C.c_long * 3)()
    assert L.load().fisdf_kmesh_plan(km3(kmesh), ncol, nao, nip, 1, route, None, None, 0, None,
                                     None, None, None) == 0
    return route[0]


def refused(L, ctx, out, name, *args):
    """the call fails with a message and leaves the output as it was."""
    before = out.flat.cpu().numpy()
    with pytest.raises(L.FisdfError) as e:
        ctx.call(name, *args)
    assert "fisdf" in str(e.value)
    ctx.call("fisdf_sync")
    assert np.array_equal(out.flat.cpu().numpy(), before, equal_nan=True)


# ---- J -------------------------------------------------------------------------------------------
class JRun:
    def __init__(self, env, c):
        self.env, self.c = env, c
        torch = env[0]
        d = J.j_data(c)
        self.nk = J.nk_of(c.kmesh)
        self.nko = c.nkb or self.nk
        self.bX, self.bW, self.bD = in_buf(torch, d.X), in_buf(torch, d.W0), in_buf(torch, d.D)
        self.bXb = in_buf(torch, d.Xb) if c.nkb else None
        self.shape = (c.nset, self.nko, c.nao, c.nao)

    def args(self, i0, i1, out):
        c = self.c
        if c.nkb:
            return ("fisdf_get_j_band_rows", self.bX.ptr, self.bW.ptr, self.bD.ptr, c.nset, self.nk,
                    c.nip, c.nao, self.bXb.ptr, c.nkb, i0, i1, out.ptr)
        return ("fisdf_get_j_rows", self.bX.ptr, self.bW.ptr, self.bD.ptr, c.nset, self.nk, c.nip,
                c.nao, i0, i1, out.ptr)

    def finish(self, out):
        torch, L, ctx = self.env
        ctx.call("fisdf_sync")
        assert out.guards_intact()
        assert all(b.guards_intact() for b in (self.bX, self.bW, self.bD, self.bXb) if b)
        return out.get().reshape(self.shape)

    def rows(self, i0, i1):
        torch, L, ctx = self.env
        out = out_buf(torch, int(np.prod(self.shape)))
        ctx.call(*self.args(i0, i1, out))
        return self.finish(out)

    def whole(self):
        torch, L, ctx = self.env
        c = self.c
        out = out_buf(torch, int(np.prod(self.shape)))
        ctx.call("fisdf_get_j", self.bX.ptr, self.bW.ptr, self.bD.ptr, c.nset, self.nk, c.nip,
                 c.nao, out.ptr)
        return self.finish(out)

    def check(self, i0, i1):
        c = self.c
        ref, tol = J.j_expect(c, i0, i1)
        got = self.rows(i0, i1)
        if i0 == i1:
            assert (got == 0).all()                     # exact zeros over the NaN
        compare("J band" if c.nkb else "J", f"{J.case_id(c)} [{i0},{i1})", got, ref, tol)
        return got, tol


@pytest.mark.parametrize("c", J.J_CASES + J.J_BAND_CASES, ids=J.case_id)
def test_j_rows(env, c):
    run = JRun(env, c)
    full = None
    for i0, i1 in J.row_blocks(c.nip):
        got, _ = run.check(i0, i1)
        if (i0, i1) == (0, c.nip):
            full = got
    if not c.nkb:
        assert np.array_equal(run.whole(), full)        # fisdf_get_j is the [0, nip) row form
    total, tols = 0, 0
    for i0, i1 in J.partition(c.nip):
        got, tol = run.check(i0, i1)
        total, tols = total + got.astype(J.CLD), tols + tol
    ref, _ = J.j_expect(c, 0, c.nip)
    compare("J partition sum", J.case_id(c), total, ref, tols)


def test_j_refusals(env):
    torch, L, ctx = env
    c = J.JCase((2, 2, 2), 8, 37, 3, 0, 0)
    cb = J.JCase((2, 2, 2), 8, 37, 3, 0, 1)
    for case in (c, cb):
        run = JRun(env, case)
        out = out_buf(torch, int(np.prod(run.shape)))
        good = run.args(5, 20, out)
        null = C.c_void_p(None)
        last = len(good) - 1
        i0_at = last - 2
        bad = [{i0_at: -1}, {i0_at + 1: case.nip + 1}, {i0_at: 21}, {1: null}, {2: null}, {3: null},
               {last: null}, {4: 0}, {5: 0}, {6: 0}, {7: 0}, {4: -1}]
        if case.nkb:
            bad += [{9: 0}, {8: null}]
        for change in bad:
            a = list(good)
            for k, v in change.items():
                a[k] = v
            refused(L, ctx, out, *a)
            run.check(5, 20)


# ---- K -------------------------------------------------------------------------------------------
class KRun:
    def __init__(self, env, c):
        self.env, self.c = env, c
        torch = env[0]
        self.d = J.k_data(c)
        self.nk = J.nk_of(c.kmesh)
        self.bX, self.bD = in_buf(torch, self.d.X), in_buf(torch, self.d.D)
        self.shape = (c.nset, self.nk, c.nao, c.nao)

    def ws(self, i0, i1, local):
        """the compact rows, or the whole W_s with NaN in every row outside the block."""
        w = self.d.Ws
        if local:
            return in_buf(self.env[0], w[:, i0:i1])
        full = np.full_like(w, np.nan)
        full[:, i0:i1] = w[:, i0:i1]
        return in_buf(self.env[0], full)

    def args(self, i0, i1, out, bW, local):
        c = self.c
        return ("fisdf_get_k_rows_local" if local else "fisdf_get_k_rows", self.bX.ptr, bW.ptr,
                self.bD.ptr, c.nset, c.nip, c.nao, km3(c.kmesh), lattice(), i0, i1, out.ptr)

    def rows(self, i0, i1, local, entry=None):
        torch, L, ctx = self.env
        c = self.c
        bW = self.ws(i0, i1, local)
        out = out_buf(torch, int(np.prod(self.shape)))
        ctx.max_imag()                                  # reset the monitors
        if entry == "whole":
            ctx.call("fisdf_get_k", self.bX.ptr, bW.ptr, self.bD.ptr, c.nset, c.nip, c.nao,
                     km3(c.kmesh), lattice(), out.ptr)
        else:
            ctx.call(*self.args(i0, i1, out, bW, local))
        mi = ctx.max_imag()                             # synchronous
        assert out.guards_intact() and bW.guards_intact()
        assert self.bX.guards_intact() and self.bD.guards_intact()
        assert mi[0] == 0 and mi[1] == 0
        return out.get().reshape(self.shape), mi[2]

    def route_is_asserted(self, i0, i1):
        c, L = self.c, self.env[1]
        want = J.k_route(c)
        listed = plan_route(L, c.kmesh, max((i1 - i0) * c.nip, 1), c.nao, c.nip) == J_REG_ROUTE
        assert listed == (tuple(c.kmesh) in J.REG_MESHES)
        if want == "gamma":
            assert self.nk == 1
        elif want == "register":
            assert listed and "FISDF_K_DFT" not in os.environ
        else:
            assert self.nk > 1 and (not listed or os.environ.get("FISDF_K_DFT") == "0")
        return want

    def check(self, i0, i1):
        c = self.c
        where = f"{J.case_id(c)} [{i0},{i1})"
        fam = "K " + self.route_is_asserted(i0, i1)
        e = J.k_expect(c, i0, i1)
        got, mon = self.rows(i0, i1, False)
        loc, mon_l = self.rows(i0, i1, True)
        if i0 == i1:
            assert (got == 0).all() and (loc == 0).all()
        compare(fam, where, got, e.ref, e.tol)
        compare(fam + " compact rows", where, loc, e.ref, e.tol)
        # the same launches on the same numbers, only the stride between the W_s[R] differs: the
        # two forms agree bit for bit on every route
        assert np.array_equal(got, loc) and mon == mon_l
        if e.scale > 0:
            r = abs(mon - e.mon) / e.scale / e.mon_tol
            print(f"{fam} monitor {where}: {mon:.3e} (reference {e.mon:.3e}), error / bound {r:.3f}")
            note(fam + " monitor", r, where)
        else:
            assert mon == 0
        return got, e.tol


@pytest.mark.parametrize("c", J.K_CASES, ids=J.case_id)
def test_k_rows(env, c, monkeypatch):
    if c.kdft is not None:
        monkeypatch.setenv("FISDF_K_DFT", c.kdft)
    run = KRun(env, c)
    full = None
    for i0, i1 in J.row_blocks(c.nip):
        got, _ = run.check(i0, i1)
        if (i0, i1) == (0, c.nip):
            full = got
    whole, _ = run.rows(0, c.nip, False, "whole")
    assert np.array_equal(whole, full)                  # fisdf_get_k is the [0, nip) row form
    total, tols = 0, 0
    for i0, i1 in J.partition(c.nip):
        got, tol = run.check(i0, i1)
        total, tols = total + got.astype(J.CLD), tols + tol
    compare("K partition sum", J.case_id(c), total, J.k_expect(c, 0, c.nip).ref, tols)


def test_k_refusals(env):
    torch, L, ctx = env
    c = J.KCase((2, 2, 2), 9, 3, 2, 1, None)
    run = KRun(env, c)
    null = C.c_void_p(None)
    for local in (False, True):
        bW = run.ws(2, 7, local)
        out = out_buf(torch, int(np.prod(run.shape)))
        good = run.args(2, 7, out, bW, local)
        bad = [{9: -1}, {10: c.nip + 1}, {9: 8}, {1: null}, {2: null}, {3: null}, {11: null},
               {4: 0}, {5: 0}, {6: 0}, {7: km3((0, 2, 2))}, {7: km3((17, 1, 1))}, {7: None},
               {8: None}]
        for change in bad:
            a = list(good)
            for k, v in change.items():
                a[k] = v
            refused(L, ctx, out, *a)
            run.check(2, 7)


# ---- ERI -----------------------------------------------------------------------------------------
class ERun:
    def __init__(self, env, c):
        self.env, self.c = env, c
        torch = env[0]
        self.d = d = J.e_data(c)
        self.bX, self.bW = in_buf(torch, d.X), in_buf(torch, d.W)
        self.bC = [None if m is None else in_buf(torch, m) for m in d.Cs]
        self.n = [c.nao if m is None else m.shape[1] for m in d.Cs]
        self.kidx = (C.c_int * 4)(*d.kidx)
        self.nmo = (C.c_int * 4)(*[0 if m is None else m.shape[1] for m in d.Cs])
        self.ptrs = None if c.cs == "none" else \
            (C.c_void_p * 4)(*[None if b is None else b.ptr.value for b in self.bC])
        self.size = self.n[0] * self.n[1] * self.n[2] * self.n[3]

    def args(self, out):
        c = self.c
        return ("fisdf_get_eri", self.bX.ptr, c.nip, c.nao, self.kidx, self.bW.ptr, self.ptrs,
                self.nmo if self.ptrs is not None else None, out.ptr)

    def check(self):
        torch, L, ctx = self.env
        out = out_buf(torch, self.size)
        ctx.call(*self.args(out))
        ctx.call("fisdf_sync")
        assert out.guards_intact() and self.bX.guards_intact() and self.bW.guards_intact()
        assert all(b.guards_intact() for b in self.bC if b)
        got = out.get().reshape(self.d.ref.shape)
        compare("ERI", J.case_id(self.c), got, self.d.ref, self.d.tol)


@pytest.mark.parametrize("c", J.E_CASES, ids=J.case_id)
def test_eri(env, c):
    ERun(env, c).check()


def test_eri_refusals(env):
    torch, L, ctx = env
    run = ERun(env, J.ECase(37, 5, 0, "all"))
    out = out_buf(torch, run.size)
    good = run.args(out)
    null = C.c_void_p(None)
    huge = (C.c_int * 4)(50000, 50000, 2, 5)            # n1 n2 = 2.5e9: refused before any workspace
    huge34 = (C.c_int * 4)(3, 4, 50000, 50000)
    bad = [{1: null}, {5: null}, {8: null}, {2: 0}, {3: 0}, {2: -3}, {7: (C.c_int * 4)(3, 0, 2, 5)},
           {7: (C.c_int * 4)(3, 4, 2, -1)}, {7: huge}, {7: huge34}, {7: None}, {4: None}]
    for change in bad:
        a = list(good)
        for k, v in change.items():
            a[k] = v
        refused(L, ctx, out, *a)
        run.check()


# ---- the unsharded fisdf_get_jk ------------------------------------------------------------------
def test_unsharded_get_jk_is_the_row_entries(env):
    """with_j / with_k of (1,0), (0,1), (1,1) after a fisdf_build: the output not asked for keeps
    its sentinel, the one asked for equals the row entry called on fisdf_build_get's buffers."""
    from cases import inputs
    torch, L, _ = env
    ctx = L.Context(0, torch.cuda.current_stream().cuda_stream)
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs("toy222")
    nk, nao = J.nk_of(kmesh), cell.nao_nr()
    dx0, df = torch.from_numpy(x0).cuda(), torch.from_numpy(chi).cuda()
    opts = L.BuildOpts()
    L.load().fisdf_build_opts_default(C.byref(opts))
    opts.nip_max = nao * 6
    nip = C.c_int()
    ctx.call("fisdf_build", L.ptr(dx0), x0.shape[1], L.ptr(df), nao, km3(kmesh), km3(cell.mesh),
             (C.c_double * 9)(*np.asarray(cell.a, float).ravel()), C.byref(opts), C.byref(nip))
    r = ctx.build_result()
    assert (r.nk, r.nip, r.nao, r.shard_size) == (nk, nip.value, nao, 1)
    rng = np.random.default_rng(5)
    dms = np.concatenate([dm, J.rnd(rng, 1, nk, nao, nao)])
    bD = in_buf(torch, dms)
    n = dms.size
    a9 = (C.c_double * 9)(*np.asarray(cell.a, float).ravel())
    rj, rk = out_buf(torch, n), out_buf(torch, n)
    ctx.call("fisdf_get_j_rows", C.c_void_p(r.d_X), C.c_void_p(r.d_W0), bD.ptr, 2, nk, r.nip, nao,
             0, r.nip, rj.ptr)
    ctx.call("fisdf_get_k_rows", C.c_void_p(r.d_X), C.c_void_p(r.d_Ws), bD.ptr, 2, r.nip, nao,
             km3(kmesh), a9, 0, r.nip, rk.ptr)
    ctx.call("fisdf_sync")
    assert not np.isnan(rj.get()).any() and not np.isnan(rk.get()).any()
    for wj, wk in ((1, 0), (0, 1), (1, 1)):
        vj, vk = out_buf(torch, n, SENT), out_buf(torch, n, SENT)
        ctx.call("fisdf_get_jk", bD.ptr, 2, wj, wk, vj.ptr, vk.ptr)
        ctx.call("fisdf_sync")
        assert vj.guards_intact() and vk.guards_intact() and bD.guards_intact()
        assert np.array_equal(vj.get(), rj.get()) if wj else (vj.get() == SENT).all()
        assert np.array_equal(vk.get(), rk.get()) if wk else (vk.get() == SENT).all()
    # a missing output and no density matrices are refused
    vj = out_buf(torch, n, SENT)
    refused(L, ctx, vj, "fisdf_get_jk", bD.ptr, 2, 1, 1, vj.ptr, C.c_void_p(None))
    refused(L, ctx, vj, "fisdf_get_jk", bD.ptr, 0, 1, 0, vj.ptr, C.c_void_p(None))
    ctx.call("fisdf_build_release")
    ctx.close()


# ---- through the object ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def objs():
    """toy222 and toy331 built by the object itself (its own AO values and selection, no oracle, no
    injected points) with few points, and the factors it holds, downloaded."""
    from cases import CASES
    from fisdf import ISDF
    out = {}
    for name in ("toy222", "toy331"):
        make, kmesh, m0, _ = CASES[name]
        cell = make()
        df = ISDF(cell, cell.get_kpts(kmesh), m0=list(m0), c0=6.0)
        df.build()
        out[name] = (df, tuple(kmesh), df._x, df._w0, df._wq)
    return out


def obj_dms(df, kmesh, seed):
    """two sets: a Hermitian one and one that is not."""
    nao = df.cell.nao_nr()
    rng = np.random.default_rng(seed)
    herm = J.make_dm(rng, kmesh, 1, nao, True)
    return np.concatenate([herm, J.rnd(rng, 1, J.nk_of(kmesh), nao, nao)])


def obj_k(X, Wq, D, kmesh, extra=None, n_extra=0):
    """K from the downloaded factors, W_s = sqrt(nk) Re(Phi W_q): (reference, bound)."""
    nk, nip, nao = X.shape
    ref = J.k_rows(X, J.ws_from_wq(Wq, kmesh), D, kmesh, 0, nip)[0]
    r64 = J.k64(X, J.ws_from_wq(Wq, kmesh, wide=False), D, kmesh, 0, nip)[0]
    if extra is not None:
        ref, r64 = ref + extra(J.CLD), r64 + extra(complex)
    return ref, J.block_bound(r64, ref, J.k_chain(nk, nao, nip, nip) + nk + n_extra)


@pytest.mark.parametrize("name", ["toy222", "toy331"])
def test_object_get_jk(objs, name):
    df, kmesh, X, W0, Wq = objs[name]
    nk, nip, nao = X.shape
    print(f"{name}: nao {nao}, nip {nip}, {len(df.fit_qs)} of {nk} q fitted")
    # a real fit under time reversal: one q of each (q, -q) pair (all 8 of toy222, 5 of toy331's 9)
    assert nao < nip <= 6 * nao and len(df.fit_qs) == len(reps(kmesh))
    D = obj_dms(df, kmesh, 3)
    vj, vk = df.get_jk(D)
    ref = J.j_rows(X, W0, D, 0, nip)
    tol = J.block_bound(J.j_rows(X, W0, D, 0, nip, wide=False), ref, J.j_chain(nk, nao, nip, nip))
    compare("object J", name, vj, ref, tol)
    compare("object K", name, vk, *obj_k(X, Wq, D, kmesh))


def test_object_kpts_band(objs):
    from fisdf import isdf as I
    df, kmesh, X, W0, Wq = objs["toy222"]
    nk, nip, nao = X.shape
    D = obj_dms(df, kmesh, 4)
    rng = np.random.default_rng(6)
    off = rng.uniform(-0.5, 0.5, (3, 3)) @ df.cell.reciprocal_vectors()
    for what, kb in (("off the mesh", off), ("on the mesh", np.asarray(df.kpts)[[5, 0, 3]])):
        vj, _ = df.get_jk(D, kpts_band=kb, with_k=False)
        Xb = I._band_aos(df, np.asarray(kb, float)).cpu().numpy()   # the AOs the object contracts
        ref = J.j_rows(X, W0, D, 0, nip, Xb=Xb)
        tol = J.block_bound(J.j_rows(X, W0, D, 0, nip, Xb=Xb, wide=False), ref,
                            J.j_chain(nk, nao, nip, nip))
        compare("object J band", what, vj, ref, tol)


def test_object_exxdiv_ewald(objs):
    df, kmesh, X, W0, Wq = objs["toy222"]
    nk, nip, nao = X.shape
    D = obj_dms(df, kmesh, 7)
    _, vk = df.get_jk(D, with_j=False, exxdiv="ewald")
    S, mad = df.get_ovlp().cpu().numpy(), df.madelung()

    def sds(dt):
        s = S.astype(dt)
        return dt(mad) * (s[None] @ D.astype(dt) @ s[None])

    compare("object K ewald", "toy222", vk, *obj_k(X, Wq, D, kmesh, sds, 2 * nao))


def test_object_get_eri_and_ao2mo(objs):
    df, kmesh, X, W0, Wq = objs["toy331"]
    nk, nip, nao = X.shape
    kpts = np.asarray(df.kpts)
    fitted = set(int(q) for q in df.fit_qs)
    idx = np.arange(nk).reshape(kmesh)

    def kof(v):
        return int(idx[tuple(np.mod(v, kmesh))])

    ks = np.array(np.unravel_index(np.arange(nk), kmesh)).T
    seen = set()
    for k1, k2, k3 in [(1, 0, 0), (0, 1, 4), (5, 2, 7), (8, 3, 2)]:
        q, k4 = kof(ks[k2] - ks[k1]), kof(ks[k1] - ks[k2] + ks[k3])
        seen.add(q in fitted)
        kidx = (k1, k2, k3, k4)
        got = df.get_eri(kpts[list(kidx)])
        ref = J.eri(X, kidx, Wq[q])
        tol = J.block_bound(J.eri(X, kidx, Wq[q], wide=False), ref, J.eri_chain(nao, nip))
        compare("object ERI", f"k {kidx} q {q} fitted {q in fitted}", got, ref, tol)
    assert seen == {True, False}                        # a fitted q and a partner's conj(W)
    rng = np.random.default_rng(8)
    Cs = [None, J.rnd(rng, nao, 4), None, J.rnd(rng, nao, 2)]
    got = df.ao2mo(Cs, kpts[list(kidx)])
    ref = J.eri(X, kidx, Wq[q], Cs)
    tol = J.block_bound(J.eri(X, kidx, Wq[q], Cs, wide=False), ref, J.eri_chain(nao, nip))
    compare("object ao2mo", "C_2 and C_4 only", got, ref, tol)


# ---- fisdf_unpack_slices -------------------------------------------------------------------------
def test_unpack_slices(env):
    """unequal slices, out of order, one empty: yT exact, the sentinel wherever no slice lands; a
    slice past ngrid is refused and writes nothing."""
    torch, L, ctx = env
    nrows, ngrid = 7, 61
    g0, ng = [40, 3, 20, 50], [9, 13, 0, 11]           # [3,16), [40,49), [50,61); 20: empty
    rng = np.random.default_rng(9)
    parts = [J.rnd(rng, nrows, n) for n in ng]
    recv = in_buf(torch, np.concatenate([p.ravel() for p in parts]))
    larr = lambda v: (C.c_long * len(v))(*v)            # noqa: E731
    yT = out_buf(torch, nrows * ngrid, SENT)
    ctx.call("fisdf_unpack_slices", recv.ptr, nrows, len(ng), larr(g0), larr(ng), ngrid, yT.ptr)
    ctx.call("fisdf_sync")
    want = np.full((nrows, ngrid), SENT)
    for p, a, n in zip(parts, g0, ng):
        want[:, a:a + n] = p
    assert yT.guards_intact() and recv.guards_intact()
    assert np.array_equal(yT.get().reshape(nrows, ngrid), want)
    yT2 = out_buf(torch, nrows * ngrid, SENT)
    for g0b, ngb in (([40, 3, 20, 51], ng), ([40, -1, 20, 50], ng), (g0, [9, 13, -2, 11])):
        refused(L, ctx, yT2, "fisdf_unpack_slices", recv.ptr, nrows, len(ng), larr(g0b), larr(ngb),
                ngrid, yT2.ptr)
    assert (yT2.get() == SENT).all()
    ctx.call("fisdf_unpack_slices", recv.ptr, nrows, len(ng), larr(g0), larr(ng), ngrid, yT2.ptr)
    ctx.call("fisdf_sync")
    assert np.array_equal(yT2.get().reshape(nrows, ngrid), want)
