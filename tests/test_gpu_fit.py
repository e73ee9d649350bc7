"""The Coulomb fit on the GPU against the long-double references of tests/fit_cases.py: the
library's own composition fisdf_factor_x4_qs + fisdf_fit_coulomb_qs on every path (real and complex
factor, full and half grid, empty and long asymmetric lists, omega of either sign, 1 to 4 lanes,
the pipelined ring, W_PP in the lane and in the batched tail, minimum-norm / basic / zero-rank q,
the W_PP split, y contiguous, in plane slices and marked ready), its refusals, the Coulomb weights
and fisdf_build_ws_qs / _rows / _blocks.

Inputs live in NaN-guarded buffers, outputs in sentinel-filled buffers whose guards are checked.
Every case asserts fisdf_fit_report / fisdf_fit_info against fit_cases' prediction BEFORE it
compares numbers, so no path is compared with a fallback.  Every bound is the float64 host chain's
own error against long double times 16, floored at ngrid eps (nq eps for W_s); each comparison
prints the device's error next to it.

fisdf_set_y_slices defines a piece as the concatenation of (nip, ng_p) blocks, so strides and gaps
are not the caller's to choose; the slices here are unequal, out of plane order and, on n0 = 2,
one of them empty."""
import ctypes as C

import numpy as np
import pytest

import factor_cases as F
import fft_cases as FF
import fit_cases as T
from oracle import isdf_ref as R
from test_gpu_factor_chain import SENT, Buf

pytestmark = pytest.mark.gpu

NAN = complex(np.nan, np.nan)
DSENT = -7.25e77


@pytest.fixture(scope="module")
def env():
    import torch
    from fisdf import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ctx = _lib.Context(0, torch.cuda.current_stream().cuda_stream)
    yield torch, _lib, ctx
    ctx.close()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for var in ("FISDF_WPP_KSPLIT", "FISDF_LANE_WPP", "FISDF_FIT_LANES", "FISDF_FIT_PIPE",
                "FISDF_PIPE_DEPTH", "FISDF_HALF_G", "FISDF_FFT_HERM", "FISDF_PIVOTED_FIT"):
        monkeypatch.delenv(var, raising=False)


def _defaults(ctx):
    ctx.call("fisdf_set_fit_mode", T.LSTSQ)
    ctx.call("fisdf_set_half_grid", -1)
    ctx.call("fisdf_set_fit_lanes", 0)
    ctx.call("fisdf_set_fit_pipe", -1, 0)
    ctx.call("fisdf_set_omega", 0.0)


def y_slices(mesh):
    """(g0, ng) of the pieces' slices: three unequal runs of planes, the last planes first; on
    n0 = 2 one plane, an empty slice, one plane."""
    n0, P = mesh[0], mesh[1] * mesh[2]
    cnt = (1, 0, 1) if n0 == 2 else FF.slice_planes(n0)
    start = np.concatenate([[0], np.cumsum(cnt)])
    order = (2, 0, 1)
    return [(int(start[p]) * P, cnt[p] * P) for p in order]


def make_piece(y, slices):
    """One q's all-to-all piece: the (nip, ng_p) blocks of the slices one after the other."""
    return np.concatenate([y[:, g0:g0 + ng].reshape(-1) for g0, ng in slices])


class Fit:
    """One factored q-list on the device and the calls on it."""

    def __init__(self, env, run, omega=None, factor="qs"):
        """factor: "qs" = fisdf_factor_x4_qs; "async" = fisdf_factor_x4_async then _wait; "nowait"
        = _async alone (the fit waits by itself; wait() reads the ranks afterwards)."""
        self.env, self.run = env, run
        torch, L, ctx = env
        c = self.c = T.BY_NAME[run.case]
        self.nq, self.nip, self.ngrid = len(c.qs), c.nip, int(np.prod(c.mesh))
        nk = int(np.prod(c.kmesh))
        x4 = np.full((nk, c.nip, c.nip), NAN)
        x4[list(c.qs)] = T.device_x4(run.case, run.real)
        self.dx4 = Buf(torch, x4.size, NAN).put(x4)
        self.y = T.inputs(run.case)[1]
        self.dy = Buf(torch, self.y.size, NAN).put(self.y)
        self.qs, self.qs_p = L.iarr(c.qs)
        self.mesh, self.mesh_p = L.iarr(c.mesh)
        self.km, self.km_p = L.iarr(c.kmesh)
        self.a, self.a_p = L.darr(c.a.ravel())
        self.omega = c.omega if omega is None else omega
        self.pieces = []
        ctx.call("fisdf_set_fit_mode", run.mode)
        ctx.call("fisdf_set_half_grid", run.half)
        ctx.call("fisdf_set_fit_lanes", run.lanes)
        ctx.call("fisdf_set_fit_pipe", run.pipe, run.depth)
        ctx.call("fisdf_set_omega", self.omega)
        self.ranks = np.full(self.nq, -9, np.int32)
        kmp = self.km_p if run.real else None
        if factor == "qs":
            ctx.call("fisdf_factor_x4_qs", self.dx4.ptr, self.qs_p, self.nq, c.nip, T.FIT_TOL, kmp,
                     self.ranks.ctypes.data_as(L._ip))
        else:
            ctx.call("fisdf_factor_x4_async", self.dx4.ptr, self.qs_p, self.nq, c.nip, T.FIT_TOL,
                     kmp)
            if factor == "async":
                self.wait()
        assert self.dx4.guards_intact()

    def wait(self):
        torch, L, ctx = self.env
        ctx.call("fisdf_factor_x4_wait", self.ranks.ctypes.data_as(L._ip))
        return tuple(int(r) for r in self.ranks)

    def hand_over_y(self, j0, j1):
        """Marks or pieces for the q [j0, j1) of the next call; returns the d_yT to pass."""
        torch, L, ctx = self.env
        if self.run.y == "ready":
            for j in range(j1 - j0):
                ctx.call("fisdf_mark_y_ready", j)
        if self.run.y != "slices":
            return C.c_void_p(self.dy.ptr.value + 16 * j0 * self.nip * self.ngrid)
        sl = y_slices(self.c.mesh)
        g0 = (C.c_long * len(sl))(*[s[0] for s in sl])
        ng = (C.c_long * len(sl))(*[s[1] for s in sl])
        self.pieces = [Buf(torch, self.nip * self.ngrid, NAN).put(make_piece(self.y[j], sl))
                       for j in range(j0, j1)]
        for j, piece in enumerate(self.pieces):
            ctx.call("fisdf_set_y_slices", j, piece.ptr, len(sl), g0, ng)
        return None

    def fit(self, j0=0, j1=None, dy="auto", nip=None, qs=None):
        """fisdf_fit_coulomb_qs over the q [j0, j1) of the factored list (or an explicit list).
        Returns (rc, W (n, nip, nip), whether W is still all sentinel)."""
        torch, L, ctx = self.env
        j1 = self.nq if j1 is None else j1
        n = j1 - j0
        qs_arr, qs_p = L.iarr(self.c.qs[j0:j1] if qs is None else qs)
        n = len(qs_arr)
        dyp = self.hand_over_y(j0, j1) if dy == "auto" else dy
        dW = Buf(torch, n * self.nip * self.nip, SENT)
        rc = ctx.lib.fisdf_fit_coulomb_qs(ctx.h, qs_p, n, dyp, self.nip if nip is None else nip,
                                          self.mesh_p, self.km_p, self.a_p, dW.ptr)
        ctx.call("fisdf_sync")
        torch.cuda.synchronize()
        assert dW.guards_intact() and self.dy.guards_intact()
        assert all(p.guards_intact() for p in self.pieces)
        W = dW.get().reshape(n, self.nip, self.nip)
        return rc, W, bool((W == SENT).all())

    def info(self):
        torch, L, ctx = self.env
        lanes, depth, slots = C.c_int(-9), C.c_int(-9), C.c_int(-9)
        ctx.call("fisdf_fit_info", C.byref(lanes), C.byref(depth))
        ctx.call("fisdf_min_norm_info", C.byref(slots))
        return lanes.value, depth.value, slots.value

    def reports(self, n):
        torch, L, ctx = self.env
        out = []
        for j in range(n):
            info = np.full(12, -99, np.int32)
            ctx.call("fisdf_fit_report", j, info.ctypes.data_as(L._ip))
            out.append(T.Report(*[int(v) for v in info]))
        return out


def check_run(env, run, ksplit_env=T.WPP_KSPLIT_DEFAULT, omega=None, label=""):
    """One whole call of a run: ranks, report and lanes as predicted, then every W_q within its
    bound.  Returns W."""
    torch, L, ctx = env
    try:
        f = Fit(env, run, omega)
        c = f.c
        assert tuple(f.ranks) == T.run_ranks(run), (run, f.ranks)
        rc, W, untouched = f.fit()
        assert rc == 0, ctx.lib.fisdf_last_error(ctx.h)
        lanes, depth, slots = f.info()
        assert (lanes, depth) == T.run_lanes(run), (run, lanes, depth)
        want = T.run_reports(run, ksplit_env, omega)
        got = f.reports(f.nq)
        for j in range(f.nq):
            assert got[j] == want[j], (run, j, got[j], want[j])
        assert slots == sum(r.min_norm for r in want)
        rc = ctx.lib.fisdf_fit_report(ctx.h, f.nq, np.zeros(12, np.int32).ctypes.data_as(L._ip))
        assert rc != 0                                   # no such q in the last call
        for j, q in enumerate(c.qs):
            ref = T.wq_ld(run.case, j, run.mode, omega)
            if want[j].rank == 0:
                assert not W[j].any(), (run, q)          # exactly zero
                continue
            err, bnd = F.relerr(W[j], ref), T.wq_bound(run.case, j, omega)
            rep = want[j]
            print(f"{label}{run.case} q={q} real={rep.real} half={rep.half} herm={rep.herm} "
                  f"ncol={rep.ncol} nasym={rep.nasym} solve={rep.solve} wpp={rep.wpp} "
                  f"split={rep.split} lanes={lanes} ring={depth} mode={run.mode} y={run.y}: "
                  f"|W - W_ld| / |W| {err:.2e} (bound {bnd:.2e})")
            assert err <= bnd, (run, q, err, bnd)
        return W
    finally:
        _defaults(ctx)


# ------------------------------------------------------------------ weights
@pytest.mark.parametrize("mesh", sorted({c.mesh for c in T.CASES}))
def test_coulg_weights(env, mesh):
    """fisdf_coulg against get_coulG (rtol / atol of test_coulg, the atol scaled with the
    weights): plain and square-rooted, scale != 1, omega 0 and +-0.4, k = 0 and every k-point of
    (2, 2, 2) and (3, 1, 2); exact zeros at G = 0 and on the box edge stay exact zeros."""
    torch, L, ctx = env
    a = T.LATTICE
    scale = 0.37
    m, mp = L.iarr(mesh)
    aa, ap = L.darr(a.ravel())
    kpts = np.concatenate([R.get_kpts(a, km) for km in ((2, 2, 2), (3, 1, 2))])
    ngrid = int(np.prod(mesh))
    worst = 0.0
    try:
        for omega in (0.0, 0.4, -0.4):
            ctx.call("fisdf_set_omega", omega)
            for k in kpts:
                kk, kp = L.darr(k)
                ref = R.get_coulG(a, k, mesh, omega=omega) * scale
                for take_sqrt in (0, 1):
                    dw = Buf(torch, ngrid, DSENT, torch.float64)
                    ctx.call("fisdf_coulg", mp, ap, kp, scale, take_sqrt, dw.ptr)
                    w = dw.get()
                    assert dw.guards_intact()
                    want = np.sqrt(ref) if take_sqrt else ref
                    assert ((w == 0) == (want == 0)).all(), (mesh, omega, k, take_sqrt)
                    worst = max(worst, float(np.abs(w - want).max() / np.abs(want).max()))
                    np.testing.assert_allclose(w, want, rtol=1e-13, atol=1e-14 * scale)
    finally:
        _defaults(ctx)
    print(f"coulg mesh {mesh}: largest |w - ref| / max |ref| over omega, k, sqrt {worst:.2e} "
          f"(rtol 1e-13)")


# ------------------------------------------------------------------ W_q, every case
@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_wq_every_case(env, name):
    runs = [r for r in T.wq_runs() if r.case == name]
    assert len(runs) == 4
    W = {(r.real, r.half): check_run(env, r) for r in runs}
    # without the real factor the half-grid switch changes nothing
    assert np.array_equal(W[0, 0], W[0, 1])
    # and all four forms agree to twice the bound
    bnd = T.wq_bound(name)
    for key in ((1, 0), (1, 1)):
        assert max(F.relerr(W[key][j], W[0, 0][j]) for j in range(len(W[key]))) <= 2 * bnd


# ------------------------------------------------------------------ invariances
def test_wq_does_not_depend_on_lanes_pipe_or_ring(env):
    """Bit for bit across 1, 2, 3 and 4 lanes, pipe off and on, ring depths 1, 2 and nq (six q,
    so slots are reused)."""
    runs = T.invariance_runs()
    W0 = check_run(env, runs[0], label="lanes/pipe: ")
    for run in runs[1:]:
        W = check_run(env, run, label="lanes/pipe: ")
        assert np.array_equal(W, W0), run


def test_q_alone_equals_q_in_a_larger_call(env):
    """Each q's split-K comes from its own rank: one q fitted alone (one lane, no pipe, the
    batched tail of one) equals the same q inside the six-q call."""
    torch, L, ctx = env
    run = T.Run(T.INVARIANCE_CASE, 1, 1, 0, -1, 0, T.LSTSQ, "contig")
    try:
        f = Fit(env, run)
        rc, W, _ = f.fit()
        assert rc == 0
        for j in (0, 3, 5):
            rc, W1, _ = f.fit(j, j + 1)
            assert rc == 0 and f.info()[:2] == (1, 0) and f.reports(1)[0].lane == 0
            assert np.array_equal(W1[0], W[j]), j
    finally:
        _defaults(ctx)


@pytest.mark.parametrize("name", [T.INVARIANCE_CASE, "rank312_self_n70"])
def test_factor_async_equals_sync(env, name):
    """fisdf_factor_x4_async + _wait, and _async with the fit waiting by itself, give the ranks and
    the W_q of fisdf_factor_x4_qs bit for bit (a rank-deficient call included: its pivoted redo and
    its minimum-norm operators are built inside the wait)."""
    torch, L, ctx = env
    run = T.Run(name, 1, 1, 0, -1, 0, T.LSTSQ, "contig")
    try:
        f = Fit(env, run)
        rc, W, _ = f.fit()
        assert rc == 0 and tuple(f.ranks) == T.run_ranks(run)
        want = f.reports(f.nq)
        for how in ("async", "nowait"):
            g = Fit(env, run, factor=how)
            rc, Wa, _ = g.fit()
            assert rc == 0 and g.wait() == T.run_ranks(run), how
            assert g.reports(g.nq) == want and np.array_equal(Wa, W), how
    finally:
        _defaults(ctx)


def test_lane_wpp_equals_batched_tail(env):
    """The 12-q call forms W_PP in the lanes; the same q in two calls of six go through the
    batched tail: the same bits."""
    torch, L, ctx = env
    run = T.Run("k322_w0_n40", 1, 1, 0, -1, 0, T.LSTSQ, "contig")
    try:
        f = Fit(env, run)
        rc, W, _ = f.fit()
        assert rc == 0 and all(r.wpp == T.WPP_LANE for r in f.reports(12))
        for j0 in (0, 6):
            rc, Wh, _ = f.fit(j0, j0 + 6)
            assert rc == 0 and all(r.wpp == T.WPP_TAIL_GEMM for r in f.reports(6))
            assert np.array_equal(Wh, W[j0:j0 + 6]), j0
    finally:
        _defaults(ctx)


def test_weight_caches_are_keyed_by_omega(env):
    """omega 0 -> -0.4 -> 0 on one context: the first W_q comes back bit for bit, and the middle
    one is within the bound of its own reference."""
    name = "even222_w0_n40"
    run = T.Run(name, 1, 1, 0, -1, 0, T.LSTSQ, "contig")
    W0 = check_run(env, run, label="omega 0: ")
    Wm = check_run(env, run, omega=-0.4, label="omega -0.4: ")
    W1 = check_run(env, run, label="omega 0 again: ")
    assert np.array_equal(W0, W1) and not np.array_equal(W0, Wm)
    full = T.Run(name, 1, 0, 0, -1, 0, T.LSTSQ, "contig")
    Wf0 = check_run(env, full)
    check_run(env, full, omega=-0.4)
    assert np.array_equal(check_run(env, full), Wf0)


# ------------------------------------------------------------------ the W_PP split
def test_wpp_split_default_and_off(env, monkeypatch):
    """nip = 256: split-K of W_PP with the default FISDF_WPP_KSPLIT and with 1, both within the
    bound (the variable is read on every call)."""
    (run, _), (run1, env1) = T.split_runs()
    W = check_run(env, run, label="split default: ")
    monkeypatch.setenv("FISDF_WPP_KSPLIT", str(env1))
    W1 = check_run(env, run1, ksplit_env=env1, label="split off: ")
    assert F.relerr(W1[0], W[0]) <= 2 * T.wq_bound(run.case)


# ------------------------------------------------------------------ rank-deficient
@pytest.mark.parametrize("name", [c.name for c in T.RANK_CASES])
def test_rank_deficient_calls(env, name):
    """A full-rank q, a rank-r q and x4_q = 0 in one call under the three fit modes, on the full
    and on the half grid: ranks, minimum-norm slots and report as predicted, W of the rank-0 q
    exactly zero, the others within the bound of the mode's own reference."""
    runs = [r for r in T.rank_runs() if r.case == name]
    assert len(runs) == 6
    W = {(r.mode, r.half): check_run(env, r) for r in runs}
    c = T.BY_NAME[name]
    j = [i for i, r in enumerate(T.case_ranks(c)) if 0 < r < c.nip][0]
    # the minimum-norm and the basic solution are different operators (the test would not see a
    # mode switch that did nothing otherwise), LSTSQ and SVD the same one
    bnd = T.wq_bound(name)
    assert F.relerr(W[T.BASIC, 0][j], W[T.LSTSQ, 0][j]) > 1e3 * bnd
    assert F.relerr(W[T.SVD, 0][j], W[T.LSTSQ, 0][j]) <= 2 * bnd


# ------------------------------------------------------------------ y sources
def test_y_sources(env):
    """y read in place from plane slices (register mesh), unpacked first (axis-route mesh) and
    marked ready: within the same bound, and equal to the contiguous call bit for bit (the same
    kernels on the same numbers; marks and pieces cap the lanes, which changes no arithmetic)."""
    for run in T.y_runs():
        W = check_run(env, run, label="y source: ")
        Wc = check_run(env, run._replace(y="contig"))
        assert np.array_equal(W, Wc), run


# ------------------------------------------------------------------ refusals
def test_refusals_leave_w_untouched(env):
    torch, L, ctx = env
    run = T.Run(T.INVARIANCE_CASE, 1, 1, 4, 0, 0, T.LSTSQ, "contig")
    try:
        f = Fit(env, run)
        rc, W, _ = f.fit()
        assert rc == 0 and f.info()[:2] == (4, 0)

        def normal_call_succeeds():
            rc, Wn, _ = f.fit()
            assert rc == 0 and np.array_equal(Wn, W)
            # no mark of a failed call is left: a call in 'ready' mode has 3 lanes at the most
            assert f.info()[:2] == (4, 0)

        def refused(rc, untouched, what):
            assert rc != 0 and untouched, what
            msg = ctx.lib.fisdf_last_error(ctx.h).decode()
            print(f"refused ({what}): {msg}")
            return msg

        # a q-list that is not a contiguous run of the factored list
        rc, _, untouched = f.fit(qs=(f.c.qs[0], f.c.qs[2]), dy=f.dy.ptr)
        assert "contiguous run" in refused(rc, untouched, "gap in the q-list")
        normal_call_succeeds()
        # a run that starts inside the factored list and ends past it
        rc, _, untouched = f.fit(qs=(f.c.qs[-1], f.c.qs[-1] + 1), dy=f.dy.ptr)
        refused(rc, untouched, "a q-list past the factored one")
        normal_call_succeeds()
        # nip different from the factored one
        rc, _, untouched = f.fit(dy=f.dy.ptr, nip=f.nip - 1)
        assert "factor" in refused(rc, untouched, "another nip")
        normal_call_succeeds()
        # no y at all
        rc, _, untouched = f.fit(dy=None)
        assert "no y" in refused(rc, untouched, "no y")
        normal_call_succeeds()
        # only some q marked ready
        ctx.call("fisdf_mark_y_ready", 0)
        ctx.call("fisdf_mark_y_ready", 2)
        rc, _, untouched = f.fit(dy=f.dy.ptr)
        assert "ready" in refused(rc, untouched, "some q marked ready")
        normal_call_succeeds()
    finally:
        _defaults(ctx)


# ------------------------------------------------------------------ W_s
def _ws_call(env, entry, Wq, kmesh, qs, wt, nip, out_count, *tail):
    torch, L, ctx = env
    dWq = Buf(torch, Wq.size, NAN).put(Wq)
    dWs = Buf(torch, out_count, DSENT, torch.float64)
    qa, qp = L.iarr(qs)
    wa, wp = L.darr(wt if wt is not None else [])
    km, kmp = L.iarr(kmesh)
    aa, ap = L.darr(T.LATTICE.ravel())
    ctx.call(entry, dWq.ptr, qp if len(qa) else None, wp if wt is not None else None, len(qa),
             nip, kmp, ap, *tail, dWs.ptr)
    ctx.call("fisdf_sync")
    torch.cuda.synchronize()
    assert dWs.guards_intact() and dWq.guards_intact()
    return dWs.get()


@pytest.mark.parametrize("kmesh,nip", T.WS_CASES)
def test_build_ws(env, kmesh, nip):
    """fisdf_build_ws_qs, _rows and _blocks against the long-double W_s: every q with no weights,
    the time-reversal representatives with weights 1 and 2, a strict subset; row blocks of unequal
    size with an empty one, chunk larger than a block, the padding left at the sentinel; nq = 0."""
    nk = int(np.prod(kmesh))
    nn = nip * nip
    Wall = T.ws_inputs(kmesh, nip)
    reps, wt = T.tr_reps(kmesh)
    subset = [q for q in range(nk) if q % 3 != 1]
    paired = any(T.partner_q(kmesh, q) != q for q in range(nk))     # (2, 2, 2): every q its own
    assert 0 < len(subset) < nk and 1.0 in wt and (2.0 in wt) == paired
    assert paired or len(reps) == nk
    lists = [("all", list(range(nk)), None), ("reps", reps, wt),
             ("subset", subset, [1.0 + 0.5 * (i % 2) for i in range(len(subset))])]
    rows = [0, 2, 2, nip - 1, nip]                       # blocks of 2, 0, nip - 3 and 1 rows
    chunk = nk * (nip - 3) * nip + 6
    for tag, qs, w in lists:
        Wq = Wall[qs]
        ref, bnd = T.ws_bound(Wq, T.LATTICE, kmesh, qs, w if w is not None else np.ones(len(qs)))
        got = _ws_call(env, "fisdf_build_ws_qs", Wq, kmesh, qs, w, nip, nk * nn).reshape(nk, nip, nip)
        err = F.relerr(got, ref)
        print(f"W_s kmesh {kmesh} {tag} nq={len(qs)}: qs {err:.2e} (bound {bnd:.2e})")
        assert err <= bnd
        i0, i1 = 1, nip - 1
        part = _ws_call(env, "fisdf_build_ws_rows", Wq, kmesh, qs, w, nip, nk * (i1 - i0) * nip,
                        i0, i1).reshape(nk, i1 - i0, nip)
        assert np.array_equal(part, got[:, i0:i1])       # the same GEMM on fewer columns
        ra, rp = env[1].iarr(rows)
        flat = _ws_call(env, "fisdf_build_ws_blocks", Wq, kmesh, qs, w, nip, 4 * chunk, 4, rp,
                        chunk)
        for b in range(4):
            nb = rows[b + 1] - rows[b]
            blk = flat[b * chunk:(b + 1) * chunk]
            assert np.array_equal(blk[:nk * nb * nip].reshape(nk, nb, nip),
                                  got[:, rows[b]:rows[b + 1]]), (tag, b)
            assert (blk[nk * nb * nip:] == DSENT).all(), (tag, b)
    zero = _ws_call(env, "fisdf_build_ws_qs", Wall[:1], kmesh, [], None, nip, nk * nn)
    assert not zero.any()
    ra, rp = env[1].iarr(rows)
    zero = _ws_call(env, "fisdf_build_ws_blocks", Wall[:1], kmesh, [], None, nip, 4 * chunk, 4, rp,
                    chunk)
    for b in range(4):
        n = nk * (rows[b + 1] - rows[b]) * nip
        assert not zero[b * chunk:b * chunk + n].any()
        assert (zero[b * chunk + n:(b + 1) * chunk] == DSENT).all()
