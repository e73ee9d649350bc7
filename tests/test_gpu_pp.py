"""The GTH pseudopotential matrices on the device: the stage entries fisdf_vloc_g,
fisdf_gth_projectors, fisdf_pp_overlap and fisdf_get_pp through the C-ABI against long-double
references, then ISDF.get_pp / get_nuc end to end.

Cases, references, the restated launch rules, the bounds and the conventions live in
tests/pp_cases.py (tests/test_pp_cases.py checks them on the CPU).  Every input is a view into a
buffer of NaN (the k blocks of f are f_kstride > ngrid * nao apart), every output a view into the
sentinel 7 + 7j, which must come back bitwise; two runs of an entry must agree bitwise.

Bound of the stage tests (tests/factor_cases.py's rule): the device may be 16 times as far from the
long-double result as the float64 restatement of the same sums is, floored at n eps, in max-norm
relative to max |ref|; n = natm + max |(k+G).R_a| for V_G and the projectors (no long sums, but a
phase whose float64 argument carries that rounding), n = ngrid for the overlap and fisdf_get_pp.
End to end: max |V - ref| < JK_TOL = 1e-8 Ha, the project's bar.
"""
import ctypes

import numpy as np
import pytest

import pp_cases as P

pytestmark = pytest.mark.gpu

NAN = complex(np.nan, np.nan)


@pytest.fixture(scope="module")
def env():
    import torch
    from fisdf import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ctx = _lib.Context(0, torch.cuda.current_stream().cuda_stream)
    return torch, _lib, ctx


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan_view(torch, a):
    a = np.asarray(a, complex).ravel()
    buf = np.full(a.size + 2 * P.EDGE, NAN)
    buf[P.EDGE:P.EDGE + a.size] = a
    d = dev(torch, buf)
    return d, d[P.EDGE:P.EDGE + a.size]


def f_view(torch, f):
    """f (nk, ngrid, nao) with its k blocks f_kstride apart in NaN: (buffer, view, f_kstride)."""
    nk, ngrid, nao = f.shape
    ks = ngrid * nao + P.KPAD
    buf = np.full(nk * ks + 2 * P.EDGE, NAN)
    for k in range(nk):
        buf[P.EDGE + k * ks: P.EDGE + k * ks + ngrid * nao] = f[k].ravel()
    d = dev(torch, buf)
    return d, d[P.EDGE:], ks


def out_view(torch, n):
    d = dev(torch, np.full(n + 2 * P.EDGE, P.SENTINEL))
    return d, d[P.EDGE:P.EDGE + n]


def edges_intact(d, n):
    h = d.cpu().numpy()
    return bool(np.all(h[:P.EDGE] == P.SENTINEL) and np.all(h[P.EDGE + n:] == P.SENTINEL))


def geometry(L, mesh):
    m = L.iarr(mesh)
    a = L.darr(P.LATTICE.ravel())
    return m, a


@pytest.mark.parametrize("nuc", (False, True), ids=("pp", "bare"))
@pytest.mark.parametrize("mesh", P.MESHES, ids=str)
def test_vloc_g(env, mesh, nuc):
    torch, L, ctx = env
    atoms = P.atoms_of(nuc=nuc)
    tab = P.pack(atoms, L)
    ref, err64 = P.vloc_g_refs(mesh, nuc)
    (mc, mp), (ac, ap) = geometry(L, mesh)
    n = P.ngrid_of(mesh)
    runs = []
    for _ in range(2):
        ob, ov = out_view(torch, n)
        ctx.call("fisdf_vloc_g", mp, ap, tab, len(atoms), L.ptr(ov))
        ctx.call("fisdf_sync")
        assert edges_intact(ob, n)
        runs.append(ov.cpu().numpy())
    assert np.array_equal(runs[0], runs[1])
    err, tol = P.rel_err(runs[0], ref), P.bound(err64, P.phase_floor(mesh, np.zeros(3), atoms))
    print(f"vloc_g {mesh} {'bare' if nuc else 'pp'}: err {err:.2e} float64 {err64:.2e} "
          f"bound {tol:.2e}")
    assert err <= tol


@pytest.mark.parametrize("ik", range(3), ids=("gamma", "half", "off"))
@pytest.mark.parametrize("mesh", P.MESHES, ids=str)
def test_gth_projectors(env, mesh, ik):
    torch, L, ctx = env
    atoms = P.atoms_of()
    tab = P.pack(atoms, L)
    ref, err64 = P.beta_refs(mesh, ik)
    (mc, mp), (ac, ap) = geometry(L, mesh)
    kc, kp = L.darr(P.KPTS[ik])
    ng, rows = P.ngrid_of(mesh), P.atom_rows(atoms)
    nproj = sum(rows)
    assert ctx.lib.fisdf_pp_nproj(tab, len(atoms)) == nproj == ref.shape[0]
    runs = []
    for _ in range(2):
        ob, ov = out_view(torch, nproj * ng)
        ctx.call("fisdf_gth_projectors", mp, ap, kp, tab, len(atoms), 0, len(atoms), L.ptr(ov))
        ctx.call("fisdf_sync")
        assert edges_intact(ob, nproj * ng)
        runs.append(ov.cpu().numpy().reshape(nproj, ng))
    assert np.array_equal(runs[0], runs[1])
    err, tol = P.rel_err(runs[0], ref), P.bound(err64, P.phase_floor(mesh, P.KPTS[ik], atoms))
    print(f"projectors {mesh} k{ik}: err {err:.2e} float64 {err64:.2e} bound {tol:.2e}")
    assert err <= tol
    # an atom range: the rows of those atoms, bitwise (what a chunk of fisdf_get_pp builds)
    ob, ov = out_view(torch, rows[1] * ng)
    ctx.call("fisdf_gth_projectors", mp, ap, kp, tab, len(atoms), 1, 2, L.ptr(ov))
    ctx.call("fisdf_sync")
    assert edges_intact(ob, rows[1] * ng)
    assert np.array_equal(ov.cpu().numpy().reshape(rows[1], ng), runs[0][rows[0]:rows[0] + rows[1]])


@pytest.mark.parametrize("c", P.OVERLAP_CASES, ids=P.case_id)
def test_pp_overlap(env, c):
    torch, L, ctx = env
    t, f = P.overlap_inputs(c)
    ref, err64 = P.overlap_refs(c)
    ng = P.ngrid_of(c.mesh)
    mc, mp = L.iarr(c.mesh)
    kd = None if c.kd is None else L.darr(c.kd)
    tb, tv = nan_view(torch, t)
    fb, fv = nan_view(torch, f)
    # the restated launch rule is the library's
    out = [ctypes.c_int() for _ in range(4)]
    assert ctx.lib.fisdf_pp_plan(c.nao, ng, 1, c.np, None, 0, 0, 0, *[ctypes.byref(o) for o in out],
                                 None, None, None) == 0
    assert (out[0].value, out[1].value) == P.overlap_split(ng)
    assert (out[2].value, out[3].value) == (-(-c.nao // P.MT), -(-c.np // P.PT))
    n = c.np * c.nao
    runs = []
    for _ in range(2):
        ob, ov = out_view(torch, n)
        ctx.call("fisdf_pp_overlap", L.ptr(tv), c.np, L.ptr(fv), c.nao, mp,
                 kd[1] if kd else None, 1.0 / ng, L.ptr(ov))
        ctx.call("fisdf_sync")
        assert edges_intact(ob, n)
        runs.append(ov.cpu().numpy().reshape(c.np, c.nao))
    assert np.array_equal(runs[0], runs[1])
    err, tol = P.rel_err(runs[0], ref), P.bound(err64, ng)
    print(f"overlap {P.case_id(c)}: err {err:.2e} float64 {err64:.2e} bound {tol:.2e}")
    assert err <= tol


def call_get_pp(env, f, mesh, kpts, atoms, with_nonlocal, work_bytes=0):
    """fisdf_get_pp on f (nk, ngrid, nao) inside NaN into the sentinel: the (nk, nao, nao) result."""
    torch, L, ctx = env
    nk, ng, nao = f.shape
    tab = P.pack(atoms, L)
    (mc, mp), (ac, ap) = geometry(L, mesh)
    kc, kp = L.darr(np.asarray(kpts).ravel())
    fb, fv, ks = f_view(torch, f)
    n = nk * nao * nao
    ob, ov = out_view(torch, n)
    ctx.call("fisdf_get_pp", L.ptr(fv), ks, nk, kp, mp, ap, nao, tab, len(atoms), with_nonlocal,
             work_bytes, L.ptr(ov))
    ctx.call("fisdf_sync")
    assert edges_intact(ob, n)
    return ov.cpu().numpy().reshape(nk, nao, nao)


@pytest.mark.parametrize("kind", ("pp", "local", "nuc"))
@pytest.mark.parametrize("c", P.PP_CASES, ids=P.case_id)
def test_get_pp_stage(env, c, kind):
    """The whole entry on random AOs at the three k-points in one call."""
    f = P.pp_inputs(c)
    nuc, nl = kind == "nuc", kind == "pp"
    atoms = P.atoms_of(nuc=nuc)
    ref, err64 = P.pp_refs(c, nl, nuc)
    runs = [call_get_pp(env, f, c.mesh, P.KPTS, atoms, int(nl)) for _ in range(2)]
    assert np.array_equal(runs[0], runs[1])
    err, tol = P.rel_err(runs[0], ref), P.bound(err64, P.ngrid_of(c.mesh))
    print(f"get_pp {P.case_id(c)} {kind}: err {err:.2e} float64 {err64:.2e} bound {tol:.2e}")
    assert err <= tol
    herm = abs(runs[0] - runs[0].conj().swapaxes(-1, -2)).max()
    assert herm <= 2 * tol * float(abs(ref).max())
    assert not runs[0][0].imag.any()                      # k = 0: the imaginary part is dropped


@pytest.mark.parametrize("c", (P.PP_CASES[1], P.PP_CASES[5]), ids=P.case_id)
def test_get_pp_chunked_bitwise(env, c):
    """A budget that splits the projector rows into chunks of whole atoms gives the same bits."""
    torch, L, ctx = env
    f = P.pp_inputs(c)
    atoms = P.atoms_of()
    rows, ng = P.atom_rows(atoms), P.ngrid_of(c.mesh)
    whole = call_get_pp(env, f, c.mesh, P.KPTS, atoms, 1)
    tab = P.pack(atoms, L)
    for budget in (21 * 16 * ng, 26 * 16 * ng, 47 * 16 * ng):
        want = P.chunks(rows, ng, budget)
        nch, crow = ctypes.c_int(), ctypes.c_int()
        assert ctx.lib.fisdf_pp_plan(c.nao, ng, 3, 0, tab, len(atoms), 1, budget, None, None, None,
                                     None, ctypes.byref(nch), ctypes.byref(crow), None) == 0
        assert nch.value == len(want)
        assert crow.value == max(sum(rows[a0:a1]) for a0, a1 in want)
        got = call_get_pp(env, f, c.mesh, P.KPTS, atoms, 1, budget)
        assert np.array_equal(got, whole), budget
    assert len(P.chunks(rows, ng, 21 * 16 * ng)) == 3 and len(P.chunks(rows, ng, 47 * 16 * ng)) == 1


def test_refusals_leave_the_output_untouched(env):
    """l > 3, n_l > 3, nexp > 4, a mesh the FFT refuses, a budget below one atom's rows, bad sizes:
    a negative return, a message, and d_out bitwise as it was."""
    torch, L, ctx = env
    c = P.PP_CASES[1]
    f = P.pp_inputs(c)
    atoms = P.atoms_of()
    nk, ng, nao = f.shape
    (mc, mp), (ac, ap) = geometry(L, c.mesh)
    kc, kp = L.darr(np.asarray(P.KPTS).ravel())
    fb, fv, ks = f_view(torch, f)
    ob, ov = out_view(torch, nk * nao * nao)
    before = ob.cpu().numpy().copy()

    def table(edit):
        tab = P.pack(atoms, L)
        edit(tab)
        return tab

    def set_nl(t):
        t[1].nl = 5

    def set_n(t):
        t[1].n[0] = 4

    def set_nexp(t):
        t[0].nexp = 5

    good = P.pack(atoms, L)
    rmesh = L.iarr(P.REFUSED_MESH)
    rng = int(np.prod(P.REFUSED_MESH))
    small = np.full(nk * (rng * nao + P.KPAD) + 2 * P.EDGE, NAN)
    sb = dev(torch, small)
    cases = [
        ("l > 3", (L.ptr(fv), ks, nk, kp, mp, ap, nao, table(set_nl), 4, 1, 0)),
        ("n_l > 3", (L.ptr(fv), ks, nk, kp, mp, ap, nao, table(set_n), 4, 1, 0)),
        ("nexp > 4", (L.ptr(fv), ks, nk, kp, mp, ap, nao, table(set_nexp), 4, 1, 0)),
        ("refused mesh", (L.ptr(sb[P.EDGE:]), rng * nao + P.KPAD, nk, kp, rmesh[1], ap, nao, good,
                          4, 1, 0)),
        ("budget below one atom", (L.ptr(fv), ks, nk, kp, mp, ap, nao, good, 4, 1, 21 * 16 * ng - 1)),
        ("f_kstride", (L.ptr(fv), ng * nao - 1, nk, kp, mp, ap, nao, good, 4, 1, 0)),
        ("nk", (L.ptr(fv), ks, 0, kp, mp, ap, nao, good, 4, 1, 0)),
        ("nao", (L.ptr(fv), ks, nk, kp, mp, ap, 0, good, 4, 1, 0)),
        ("no atoms", (L.ptr(fv), ks, nk, kp, mp, ap, nao, good, 0, 1, 0)),
    ]
    for name, args in cases:
        rc = ctx.lib.fisdf_get_pp(ctx.h, *args, L.ptr(ov))
        msg = ctx.lib.fisdf_last_error(ctx.h)
        ctx.call("fisdf_sync")
        assert rc < 0 and msg, name
        assert np.array_equal(ob.cpu().numpy().view(np.uint8), before.view(np.uint8)), name
    # the stage entries refuse the same tables
    vb, vv = out_view(torch, nk * 47 * ng)
    vbefore = vb.cpu().numpy().copy()
    for name, args in cases[:3]:
        tab = args[7]
        assert ctx.lib.fisdf_vloc_g(ctx.h, mp, ap, tab, 4, L.ptr(vv)) < 0, name
        assert ctx.lib.fisdf_gth_projectors(ctx.h, mp, ap, kp, tab, 4, 0, 4, L.ptr(vv)) < 0, name
        assert ctx.lib.fisdf_pp_nproj(tab, 4) < 0, name
    assert ctx.lib.fisdf_gth_projectors(ctx.h, mp, ap, kp, good, 4, 3, 4, L.ptr(vv)) < 0  # no rows
    ctx.call("fisdf_sync")
    assert np.array_equal(vb.cpu().numpy().view(np.uint8), vbefore.view(np.uint8))
    # and the entry still works afterwards
    ctx.call("fisdf_get_pp", L.ptr(fv), ks, nk, kp, mp, ap, nao, good, 4, 1, 0, L.ptr(ov))
    ctx.call("fisdf_sync")
    assert np.isfinite(ov.cpu().numpy()).all()


# ---- end to end ------------------------------------------------------------------------------------
def check_e2e(df, mesh, what="toy"):
    kmesh_kpts = df.cell.get_kpts(P.KMESH)
    assert abs(kmesh_kpts - np.asarray(P.KPTS[:2])).max() < 1e-12
    ref_pp, ref_nuc = P.toy_refs(mesh), P.toy_refs(mesh, nuc=True)
    for name, fn, ref in (("get_pp", df.get_pp, ref_pp), ("get_nuc", df.get_nuc, ref_nuc)):
        on = fn()                                   # kpts=None: the k-mesh, resident AOs
        assert on.shape == ref[:2].shape
        off = fn(np.asarray(P.KPTS[2]))             # (3,): one matrix, band AOs
        assert off.shape == ref[2].shape
        both = fn(np.asarray(P.KPTS))               # (n, 3) with an off-mesh point: band AOs
        assert both.shape == ref.shape
        one = fn(np.asarray(P.KPTS[1:2]))           # a subset of the mesh: gathered resident AOs
        assert one.shape == ref[1:2].shape and abs(one[0] - ref[1]).max() < P.JK_TOL
        errs = [float(abs(on - ref[:2]).max()), float(abs(off - ref[2]).max()),
                float(abs(both - ref).max())]
        print(f"{what} {name} {mesh}: max |d| mesh {errs[0]:.2e} off-mesh {errs[1]:.2e} "
              f"all {errs[2]:.2e} Ha")
        assert max(errs) < P.JK_TOL
        tol = P.bound(0.0, P.ngrid_of(mesh)) * float(abs(ref).max())
        assert abs(both - both.conj().swapaxes(-1, -2)).max() <= 2 * tol
        assert not on[0].imag.any() and not both[0].imag.any()       # Im == 0 at k = 0


@pytest.mark.parametrize("mesh", P.MESHES, ids=str)
def test_isdf_get_pp_get_nuc(mesh):
    from fisdf import ISDF
    cell = P.toy_cell(mesh)
    df = ISDF(cell, cell.get_kpts(P.KMESH))
    check_e2e(df, mesh)                            # no build()
    # get_nuc is get_pp of the same cell without pseudopotentials
    bare = P.toy_cell(mesh, pseudo={})
    dfb = ISDF(bare, bare.get_kpts(P.KMESH))
    assert np.array_equal(dfb.get_nuc(), dfb.get_pp())
    assert list(bare.atom_charges()) == [14, 28, 28, 6]


class PyscfLikeCell:
    """Only the PySCF Cell protocol, nothing of fisdf.cell's own: no ``shells``, ``rcut`` an
    attribute, AO values through ``pbc_eval_gto``, the pseudopotential in ``_pseudo``."""

    def __init__(self, inner):
        self._inner = inner
        self.mesh = tuple(inner.mesh)
        self.vol = float(inner.vol)
        self.rcut = float(inner.rcut())
        self.natm = inner.natm
        self.verbose = 0
        self.dimension = 3
        self._pseudo = dict(P.PSEUDO)

    def lattice_vectors(self):
        return self._inner.lattice_vectors()

    def reciprocal_vectors(self):
        return self._inner.reciprocal_vectors()

    def atom_coords(self):
        return self._inner.atom_coords()

    def atom_charges(self):
        return np.array([4, 18, 18, 6])

    def atom_symbol(self, ia):
        return P.SYMBOLS[ia]

    def nao_nr(self):
        return self._inner.nao_nr()

    def get_kpts(self, kmesh):
        from fisdf import cell as C
        return C.make_kpts(self._inner, kmesh)

    def gen_uniform_grids(self, mesh=None, wrap_around=True):
        return self._inner.gen_uniform_grids(mesh, wrap_around)

    def pbc_eval_gto(self, eval_name, coords, kpts=None):
        from fisdf import cell as C
        assert eval_name == "GTOval"
        k = np.zeros((1, 3)) if kpts is None else np.asarray(kpts, float).reshape(-1, 3)
        out = C.eval_ao_band(self._inner, np.asarray(coords), k)
        return out[0] if kpts is None else [out[i] for i in range(len(k))]


def test_pyscf_protocol_cell():
    from fisdf import ISDF
    mesh = P.MESHES[1]
    stub = PyscfLikeCell(P.toy_cell(mesh, pseudo={}))
    assert not hasattr(stub, "shells")
    df = ISDF(stub, stub.get_kpts(P.KMESH))
    check_e2e(df, mesh, what="PySCF-style cell")
