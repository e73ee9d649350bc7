"""Every route and option of fft3d() (csrc/fft.hip) through fisdf_fft3d_ex against a long-double
DFT: the register kernels at every listed size (as a plane size and as an axis-0 size, cubic or
not), both instantiations of the LDS plane kernel and of the Stockham axis kernel, the three-pass
route, and on each the row gather, the row strides, the phase exp(-i f.kd), the fused weight,
in-place operation, sliced input through a plane table, Hermitian pairing and real input rows.

Cases, the reference and the conventions live in tests/fft_cases.py (tests/test_fft_cases.py
checks on the CPU that the tables reach every route and branch).  Every buffer is a view: input
rows at in_ld = ngrid + 5 in NaN (rows the gather does not name are NaN too), output rows at
out_ld = ngrid + 3 in the sentinel 7 + 7j, which must come back bitwise; the route the library
reports must be the one the restated rule gives.  Bound: max |out - ref| / max |ref| < 1e-14, the
suite's own FFT bound (test_fft3d), about 25 x the error of numpy's fp64 fftn against the same
reference (2.5e-16 to 4.2e-16 on these meshes).
"""
import ctypes as C
import zlib

import numpy as np
import pytest

import fft_cases as F

pytestmark = pytest.mark.gpu

NAN = complex(np.nan, np.nan)
_lp = C.POINTER(C.c_long)


@pytest.fixture(scope="module")
def env():
    import torch
    from fisdf import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ctx = _lib.Context(0, torch.cuda.current_stream().cuda_stream)
    return torch, _lib, ctx


@pytest.fixture(scope="module")
def worst():
    """Cases run and largest error per family, printed when the module is done."""
    w = {}
    yield w
    for k in sorted(w):
        n, err, name = w[k]
        print(f"\nfft-variants {k}: {n} transforms, largest error {err:.3e} (bound {F.TOL:.0e}) at {name}")


def note(worst, group, err, name):
    n, e, nm = worst.get(group, (0, -1.0, ""))
    worst[group] = (n + 1, err, name) if err > e else (n + 1, e, nm)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def used_rows(rng, mesh, rows, real=False):
    """(all ROWS_IN input rows, the `rows` rows a transform sees): the gather names ROWIDX."""
    ngrid = int(np.prod(mesh))
    full = rng.standard_normal((F.ROWS_IN, ngrid)) if real else F.rnd(rng, F.ROWS_IN, ngrid)
    return full, full[list(F.ROWIDX[:rows])]


def transform(env, mesh, full, used, gather=False, kd=None, weight=None, inplace=False,
              sliced=False, m=None, in_real=False):
    """One fisdf_fft3d_ex call on padded views.  Returns (rc, reported route, logical output
    (rows, ngrid), flat output buffer, flat output buffer before the call)."""
    torch, L, ctx = env
    rows, ngrid = used.shape
    P = mesh[1] * mesh[2]
    out_ld = ngrid + F.PAD_OUT
    obuf = np.full(rows * out_ld, F.SENTINEL)
    oview = obuf.reshape(rows, out_ld)[:, :ngrid]
    src = full if gather else used            # the rows the input buffer holds
    named = set(F.ROWIDX[:rows]) if gather else set(range(rows))
    base = ld = None
    if inplace:
        assert not gather and not sliced and not in_real
        oview[...] = used
        in_ld = out_ld
    elif sliced:
        base, ld, size = F.slice_layout(mesh, len(src))
        ibuf = np.full(size, NAN)
        for r in named:
            for i0 in range(mesh[0]):
                ibuf[base[i0] + r * ld[i0]: base[i0] + r * ld[i0] + P] = src[r, i0 * P:(i0 + 1) * P]
        in_ld = F.IN_LD_UNUSED
    else:
        in_ld = ngrid + F.PAD_IN
        ibuf = np.full(len(src) * in_ld, np.nan if in_real else NAN)
        for r in named:
            ibuf[r * in_ld: r * in_ld + ngrid] = src[r]
    dout = dev(torch, obuf)
    din = dout if inplace else dev(torch, ibuf)
    drow = dev(torch, np.array(F.ROWIDX[:rows], dtype=np.int32)) if gather else None
    dw = dev(torch, weight) if weight is not None else None
    ma, mp = L.iarr(mesh)                     # the arrays stay alive as long as their pointers
    ka, kp = L.darr(kd) if kd is not None else (None, None)
    ha, hp = L.iarr(m) if m is not None else (None, None)
    path = C.c_int(-7)
    rc = ctx.lib.fisdf_fft3d_ex(
        ctx.h, L.ptr(din), in_ld, L.ptr(drow) if gather else None, L.ptr(dout), out_ld, rows, mp,
        kp, L.ptr(dw) if dw is not None else None,
        base.ctypes.data_as(_lp) if sliced else None, ld.ctypes.data_as(_lp) if sliced else None,
        hp, int(in_real), C.byref(path))
    ctx.call("fisdf_sync")
    flat = dout.cpu().numpy()
    return rc, path.value, flat.reshape(rows, out_ld)[:, :ngrid], flat, obuf


def check(env, worst, group, name, mesh, ref, rc, path, out, flat, m=None, ncol=None):
    """The route, the compared region within the bound, the row padding bitwise the sentinel."""
    torch, L, ctx = env
    assert rc == 0, ctx.lib.fisdf_last_error(ctx.h)
    assert path == F.route(mesh, m), (path, F.route(mesh, m))
    ngrid = int(np.prod(mesh))
    ncol = ngrid if ncol is None else ncol
    err = F.rel_err(out[:, :ncol], ref[:, :ncol])
    print(f"{group} {name}: route {path} err {err:.3e}")
    note(worst, group, err, name)
    pad = flat.reshape(out.shape[0], -1)[:, ngrid:]
    assert pad.tobytes() == np.full(pad.shape, F.SENTINEL).tobytes(), "the row padding was written"
    assert err < F.TOL, err
    return err


def run_case(env, worst, group, c):
    rng = np.random.default_rng(zlib.crc32(repr((group, tuple(c))).encode()))
    full, used = used_rows(rng, c.mesh, c.rows)
    w = F.make_weight(rng, used.shape[1]) if c.weight else None
    kd = np.array(c.kd) if c.kd is not None else None
    rc, path, out, flat, _ = transform(env, c.mesh, full, used, c.gather, kd, w, c.inplace, c.sliced)
    check(env, worst, group, F.cid(c), c.mesh, F.ref_fft3d(used, c.mesh, kd, w), rc, path, out, flat)


# ---- 1. register kernels ----------------------------------------------------------------------------
@pytest.mark.parametrize("c", F.GROUP_REG, ids=F.cid)
def test_register_sizes(env, worst, c):
    """fft_plane_reg<N> at (8, N, N) and fft_axis0_reg<N> at (N, 8, 8) for every listed N, and
    meshes with n0 != n1; bare, and with the gather, the phase, the weight and the strides."""
    run_case(env, worst, "1-reg", c)


# ---- 2. LDS plane kernel + axis-0 pass ----------------------------------------------------------------
@pytest.mark.parametrize("c", F.GROUP_LDS, ids=F.cid)
def test_lds_plane_route(env, worst, c):
    """fft_plane_kernel<false> and <true> (planes of one point up to 96256 bytes of LDS, the tail
    load loop above 2048 points) followed by fft_axis_kernel on axis 0 (narrow, widened and
    largest tile)."""
    run_case(env, worst, "2-lds", c)


# ---- 3. three axis passes --------------------------------------------------------------------------
@pytest.mark.parametrize("c", F.GROUP_AXES, ids=F.cid)
def test_three_axis_passes(env, worst, c):
    """Planes beyond 96 KB: fft_axis_kernel on axes 2, 1, 0, with a partial last tile in the
    contiguous pass and the radix-7/11 instantiation on each axis."""
    run_case(env, worst, "3-axes", c)


# ---- 4. options on every route ---------------------------------------------------------------------
@pytest.mark.parametrize("c", F.GROUP_OPTIONS, ids=F.cid)
def test_options_alone_and_together(env, worst, c):
    """The phase (generic kd, an even and an odd mesh: the fftfreq wrap is at (n + 1) / 2), the
    weight, the gather and in-place operation, each alone and together, on each route."""
    run_case(env, worst, "4-options", c)


# ---- 5. sliced input --------------------------------------------------------------------------------
@pytest.mark.parametrize("c", F.GROUP_SLICED, ids=F.cid)
def test_sliced_input(env, worst, c):
    """Input planes in 3 slices of unequal plane counts, each with its own row stride and NaN
    between them, read through the plane table (in_ld is unused and given a wrong value)."""
    run_case(env, worst, "5-sliced", c)


# ---- 6. Hermitian pairing ----------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,m", F.GROUP_HERM,
                         ids=["%s-m%d%d%d" % (("x".join(map(str, g)),) + h) for g, h in F.GROUP_HERM])
def test_hermitian_pairing(env, worst, mesh, m):
    """Real rows times exp(-i f.kd), kd = pi m: the plane pass stores the lines j1 < n1H, the
    axis-0 pass rebuilds their partners (conjugate, twiddle for m0 = 1, weight by the partner's own
    column) and writes the prefix planes; rows stored complex and as doubles, with the weight, the
    gather and the plane table."""
    rng = np.random.default_rng(sum(mesh) * 8 + m[0] * 4 + m[1] * 2 + m[2])
    full, used = used_rows(rng, mesh, 3, real=True)
    kd = np.pi * np.array(m, dtype=float)
    w = F.make_weight(rng, used.shape[1])
    ref = F.ref_fft3d(used, mesh, kd)
    refw = ref * w.astype(F.LD)
    ncol = F.half_prefix_planes(mesh[0], m[0]) * mesh[1] * mesh[2]
    for v in F.HERM_VARIANTS:
        src_full, src_used = (full, used) if v.in_real else (full + 0j, used + 0j)
        rc, path, out, flat, _ = transform(env, mesh, src_full, src_used, bool(v.gather), kd,
                                           w if v.weight else None, False, bool(v.sliced), m,
                                           bool(v.in_real))
        name = "%s-m%d%d%d-%s" % (("x".join(map(str, mesh)),) + m + ("".join(map(str, v)),))
        check(env, worst, "6-herm", name, mesh, refw if v.weight else ref, rc, path, out, flat, m,
              ncol)


@pytest.mark.parametrize("mesh,m", F.HERM_FULL)
def test_pairing_on_other_routes_writes_everything(env, worst, mesh, m):
    """m on a mesh without register kernels: the whole transform is written."""
    rng = np.random.default_rng(sum(mesh) + 100)
    full, used = used_rows(rng, mesh, 2, real=True)
    kd = np.pi * np.array(m, dtype=float)
    w = F.make_weight(rng, used.shape[1])
    rc, path, out, flat, _ = transform(env, mesh, full + 0j, used + 0j, True, kd, w, m=m)
    check(env, worst, "6-herm-full", "x".join(map(str, mesh)), mesh, F.ref_fft3d(used, mesh, kd, w),
          rc, path, out, flat, m)


# ---- 7. accept or fail ---------------------------------------------------------------------------------
@pytest.mark.parametrize("r", F.GROUP_REJECT, ids=[r.name for r in F.GROUP_REJECT])
def test_rejects_before_launching(env, r):
    """What fft3d() cannot do fails with a message, reports no route and leaves the output
    untouched: every check runs on the host before the first kernel."""
    torch, L, ctx = env
    rng = np.random.default_rng(17)
    rows, ngrid, P = 3, int(np.prod(r.mesh)), r.mesh[1] * r.mesh[2]
    obuf = np.full(rows * (ngrid + F.PAD_OUT), F.SENTINEL)
    ibuf = F.rnd(rng, F.ROWS_IN * (ngrid + F.PAD_IN))
    dout = dev(torch, obuf)
    din = dout if r.inplace else dev(torch, ibuf.view(np.float64) if r.in_real else ibuf)
    drow = dev(torch, np.array(F.ROWIDX, dtype=np.int32))
    base = np.arange(r.mesh[0], dtype=np.int64) * P   # the unsliced layout, as a plane table
    ld = np.full(r.mesh[0], ngrid + F.PAD_IN, dtype=np.int64)
    ma, mp = L.iarr(r.mesh)
    ha, hp = L.iarr(r.m) if r.m is not None else (None, None)
    path = C.c_int(-7)
    ld_io = ngrid + (F.PAD_OUT if r.inplace else F.PAD_IN)
    rc = ctx.lib.fisdf_fft3d_ex(
        ctx.h, L.ptr(din), ld_io, L.ptr(drow) if r.gather else None, L.ptr(dout),
        ngrid + F.PAD_OUT, rows, mp, None, None, base.ctypes.data_as(_lp) if r.sliced else None,
        ld.ctypes.data_as(_lp) if r.sliced else None, hp, r.in_real, C.byref(path))
    ctx.call("fisdf_sync")
    assert rc != 0 and len(ctx.lib.fisdf_last_error(ctx.h)) > 0, r.name
    assert path.value == -1
    assert dout.cpu().numpy().tobytes() == obuf.tobytes(), "a refused call wrote to the output"


@pytest.mark.parametrize("mesh", [(8, 12, 12), (6, 10, 10), (3, 56, 56)])
def test_zero_rows(env, mesh):
    """rows = 0 returns 0, runs nothing and writes nothing."""
    torch, L, ctx = env
    ngrid = int(np.prod(mesh))
    obuf = np.full(ngrid + F.PAD_OUT, F.SENTINEL)
    dout, din = dev(torch, obuf), dev(torch, np.full(ngrid + F.PAD_IN, NAN))
    ma, mp = L.iarr(mesh)
    path = C.c_int(-7)
    rc = ctx.lib.fisdf_fft3d_ex(ctx.h, L.ptr(din), ngrid + F.PAD_IN, None, L.ptr(dout),
                                ngrid + F.PAD_OUT, 0, mp, None, None, None, None, None, 0,
                                C.byref(path))
    ctx.call("fisdf_sync")
    assert rc == 0, ctx.lib.fisdf_last_error(ctx.h)
    assert path.value == -1
    assert dout.cpu().numpy().tobytes() == obuf.tobytes()
