"""The Bloch AO evaluator on the device against long-double lattice sums: ao_folded_kernel with
sph.h, the table building and translation grouping of eval_ao, through the C-ABI entries
fisdf_eval_ao and fisdf_eval_ao_band themselves (raw tables on a triclinic lattice) and through the
wrappers fisdf.ao.eval_ao_kpts_gpu / eval_ao_band_gpu (the toy, diamond and NiO cells).

Cases, references and conventions live in tests/ao_cases.py (tests/test_ao_cases.py checks them,
and the host restatement, on the CPU).  The references take no constant from fisdf.cell or sph.h:
harmonics from their definition, the radial normalisation restated, everything in long double.
The coordinates of a raw case are a view into a buffer of NaN, the output a view into the sentinel
7 + 7j, and every element outside the logical output has to come back as the sentinel bit for bit.

Bound (tests/factor_cases.py's rule), per AO column: the error is max over k and points of
|got - ref| over max |ref| of that column, so a small d or f component cannot hide under the s
functions; the device may be 16 times as far from the long-double sum as the float64 restatement
of the same sum is in that column, floored at n eps, n the longest sum of the case (the in-range
translations of one image times nprim, plus the images or translations of the DFT).  No case has a
(point, atom, T) triple within 1e-9 (relative, in r^2) of the cutoff, where the device's
(r - A) - T and the reference's r - (A + T) could fall on different sides.
"""
import ctypes as C

import numpy as np
import pytest

import ao_cases as A
import kmesh_cases as K

pytestmark = pytest.mark.gpu

WORST = {}          # family -> (largest error / bound, error, bound, float64's error, comparisons)
SPARE = 40          # sentinel elements behind the logical output, besides the edges


@pytest.fixture(scope="module")
def env():
    import torch
    from fisdf import _lib
    from fisdf.isdf import _Device
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    device = _Device()
    yield torch, _lib, device
    for fam, (ratio, err, tol, e64, n) in sorted(WORST.items()):
        print(f"ao {fam}: {n} comparisons, largest error {err:.2e} (bound {tol:.2e}, ratio "
              f"{ratio:.2f}; float64 restatement {e64:.2e})")


def note(fam, got, d):
    """got against the case's reference, column by column; keeps the family's worst ratio."""
    assert got.shape == d.ref.shape
    err = A.col_err(got, d.ref)
    tol = np.asarray([A.bound(e, d.nsum) for e in d.err64])
    j = int(np.argmax(err / tol))
    old = WORST.get(fam, (-1.0, 0.0, 0.0, 0.0, 0))
    new = (err[j] / tol[j], err[j], tol[j], d.err64[j])
    WORST[fam] = (new if new[0] > old[0] else old[:4]) + (old[4] + 1,)
    assert np.all(err <= tol), (fam, j, A.ao_labels(d.tab)[j], err[j], tol[j])
    return err[j], tol[j], j


def _buffers(torch, coords, nout):
    """coords inside NaN and an output of nout logical elements inside the sentinel."""
    co = np.asarray(coords, float).ravel()
    cb = np.full(co.size + 2 * A.EDGE + 3, np.nan)
    cb[A.EDGE:A.EDGE + co.size] = co
    cb = torch.from_numpy(cb).cuda()
    ob = torch.from_numpy(np.full(nout + SPARE + 2 * A.EDGE, A.SENTINEL)).cuda()
    return cb, cb[A.EDGE:], ob, ob[A.EDGE:]


def _logical(ob, nout):
    """the logical output, after asserting that everything around it is still the sentinel."""
    h = ob.cpu().numpy()
    assert np.all(h[:A.EDGE] == A.SENTINEL) and np.all(h[A.EDGE + nout:] == A.SENTINEL), \
        "an element outside the output was written"
    return h[A.EDGE:A.EDGE + nout]


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def call(env, tab, coords, kmesh=None, kband=None, **over):
    """fisdf_eval_ao (kmesh) or fisdf_eval_ao_band (kband) on raw tables; over replaces single
    arguments (the refusals).  Returns (rc, message, output buffer, logical size)."""
    torch, L, device = env
    ng = len(np.reshape(coords, (-1, 3)))
    nao = A.nao_of(tab)
    nk = K.nk_of(kmesh) if kband is None else len(kband)
    nout = nk * ng * nao
    cb, cv, ob, ov = _buffers(torch, coords, nout)
    keep = dict(
        atoms=np.ascontiguousarray(tab.atoms, float), sh_atom=np.ascontiguousarray(tab.sh_atom, np.int32),
        sh_l=np.ascontiguousarray(tab.sh_l, np.int32), sh_np=np.ascontiguousarray(tab.sh_np, np.int32),
        exps=np.ascontiguousarray(tab.exps, float), coefs=np.ascontiguousarray(tab.coefs, float),
        tn=np.ascontiguousarray(np.reshape(tab.tn, (-1, 3)), np.int32),
        a=np.ascontiguousarray(tab.a, float).ravel(), ng=ng, nao=nao)
    keep.update(over)
    k = keep
    head = (device.ctx.h, L.ptr(cv), k["ng"], len(k["atoms"]), _dp(k["atoms"]), len(k["sh_l"]),
            _ip(k["sh_atom"]), _ip(k["sh_l"]), _ip(k["sh_np"]), _dp(k["exps"]), _dp(k["coefs"]),
            len(k["tn"]), _ip(k["tn"]))
    tail = (_dp(k["a"]), float(tab.rcut), k["nao"], L.ptr(ov))
    if kband is None:
        km = np.asarray(k.get("kmesh_arg", kmesh), np.int32)
        rc = L.load().fisdf_eval_ao(*head, _ip(km), *tail)
    else:
        kb = np.ascontiguousarray(kband, float)
        kp = None if k.get("null_kpts") else _dp(kb)
        rc = L.load().fisdf_eval_ao_band(*head, k.get("nkb", len(kb)), kp, *tail)
    msg = L.load().fisdf_last_error(device.ctx.h).decode() if rc else ""
    device.ctx.call("fisdf_sync")
    return rc, msg, ob, nout


def run_raw(env, c):
    d = A.raw_data(c.name)
    rc, msg, ob, nout = call(env, d.tab, d.coords, c.kmesh, d.kband)
    assert rc == 0, msg
    got = _logical(ob, nout).reshape(d.ref.shape)
    return d, got


def family(c):
    if c.kmesh is None:
        return "raw band"
    if K.nk_of(c.kmesh) == 1:
        return "raw gamma"
    return "raw k-mesh register" if K.route(c.kmesh)[0] == K.REG else "raw k-mesh generic"


# ---- raw tables through the C-ABI --------------------------------------------------------------
@pytest.mark.parametrize("c", A.RAW_CASES, ids=A.case_id)
def test_raw_tables(env, c):
    d, got = run_raw(env, c)
    if c.ng == 0:                       # nothing to write: _logical has seen the sentinel everywhere
        assert got.size == 0
        return
    if A.expect_zero(c):
        assert not d.ref.any() and np.all(got == 0), "no translation in range: exact zeros"
        return
    err, tol, j = note(family(c), got, d)
    print(f"{c.name} ({family(c)}): err {err:.2e} bound {tol:.2e} at column {j} "
          f"{A.ao_labels(d.tab)[j]}; float64 restatement {d.err64.max():.2e}, n {d.nsum}")


def test_band_mode_on_the_mesh_reproduces_the_kmesh_result(env):
    (db, band), (dk, mesh) = (run_raw(env, A.RAW_BY_NAME[n]) for n in A.BAND_MESH_PAIR)
    tol = np.asarray([A.bound(e, db.nsum) + A.bound(f, dk.nsum) for e, f in zip(db.err64, dk.err64)])
    assert np.all(A.col_err(band, mesh) <= tol + A.col_err(db.ref, dk.ref))


# ---- the cells through the wrappers ------------------------------------------------------------
@pytest.mark.parametrize("c", A.REAL_CASES, ids=A.case_id)
def test_cells_through_the_wrappers(env, c):
    from fisdf.ao import eval_ao_band_gpu, eval_ao_kpts_gpu
    torch, L, device = env
    d = A.real_data(c.name)
    cell = A.real_cell(c.cell, c.mesh)
    if c.kmesh is None:
        got = eval_ao_band_gpu(device, cell, d.coords, d.kband).cpu().numpy()
    else:
        got = eval_ao_kpts_gpu(device, cell, d.coords, c.kmesh).cpu().numpy()
    fam = "cell band" if c.kmesh is None else "cell k-mesh"
    err, tol, j = note(fam, got, d)
    print(f"{c.name} ({fam}): err {err:.2e} bound {tol:.2e} at column {j} {A.ao_labels(d.tab)[j]}; "
          f"float64 restatement {d.err64.max():.2e}, n {d.nsum}")


# ---- refusals ----------------------------------------------------------------------------------
def test_refused_calls_leave_the_output_untouched_and_the_context_usable(env):
    """Every argument check of fisdf_eval_ao / fisdf_eval_ao_band / eval_ao runs on the host before
    the first copy or launch: the call returns nonzero with a message, the output stays the
    sentinel, and the next valid call on the same context gives the bits it gave before."""
    c = A.RAW_BY_NAME["mixed_312"]
    b = A.RAW_BY_NAME["band_many_off3"]
    d, before = run_raw(env, c)
    db, before_band = run_raw(env, b)
    tab, nsh = d.tab, len(d.tab.sh_l)

    def with_(arr, i, v):
        out = np.array(arr, np.int32)
        out[i] = v
        return out

    l4 = with_(tab.sh_l, 2, 4)                                   # the d shell becomes l = 4
    refusals = [
        ("angular momentum", dict(sh_l=l4, nao=A.nao_of(tab) + 4)),
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
            rc, msg, ob, nout = call(env, dd.tab, dd.coords, case.kmesh, dd.kband, **over)
            assert rc != 0, (case.name, over, "accepted a call it must refuse")
            assert want in msg, (case.name, over, msg)
            assert np.all(ob.cpu().numpy() == A.SENTINEL), (case.name, over)
            n += 1
    assert n == 2 * len(refusals) + 6
    d2, after = run_raw(env, c)
    d3, after_band = run_raw(env, b)
    assert np.array_equal(after, before) and np.array_equal(after_band, before_band)
    note(family(c), after, d)
    note(family(b), after_band, db)
