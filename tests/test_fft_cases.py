"""CPU checks of tests/fft_cases.py: the case tables of test_gpu_fft_variants.py reach every route
of fft3d(), both instantiations of each Stockham kernel, every listed register size as a plane size
and as an axis-0 size and every branch the tables name (by the dispatch rule restated there); the
long-double reference agrees with numpy's fftn; the paired inputs have the Hermitian identity."""
import numpy as np
import pytest

import fft_cases as F


def test_dispatch_rule_examples():
    """The restated rule on the meshes whose landing place the case tables rely on."""
    assert F.route((8, 12, 12)) == F.REG and F.route((8, 12, 12), (1, 0, 1)) == F.REG_HERM
    assert F.route((13, 16, 16)) == F.REG and F.route((8, 12, 16)) == F.PLANE
    assert F.route((7, 12, 12)) == F.PLANE | F.BIG      # n0 not listed; its axis-0 pass is radix 7
    assert F.kernels((7, 12, 12)) == [("plane", False), ("axis", True)]
    assert F.kernels((14, 16, 16)) == [("plane", False), ("axis", True)]
    assert F.kernels((9, 7, 11)) == [("plane", True), ("axis", False)]
    assert F.route((6, 10, 10)) == F.PLANE and F.route((6, 10, 14)) == F.PLANE | F.BIG
    assert F.route((1, 1, 1)) == F.PLANE and F.factorize(1) == []
    # the 96 KiB limit of the plane kernel: 48 x 60 fits (96256 bytes), 56 x 56 does not
    assert F.plane_lds((3, 48, 60)) == 96256 <= F.PLANE_LDS_MAX < F.plane_lds((3, 56, 56))
    assert F.route((3, 48, 60)) == F.PLANE and F.route((4, 50, 50)) == F.PLANE
    assert F.route((3, 56, 56)) == F.AXES | F.BIG and F.route((2, 64, 48)) == F.AXES
    assert F.route((3, 50, 64)) == F.AXES and F.route((2, 56, 55)) == F.AXES | F.BIG
    # m on a mesh without register kernels does not change the route
    assert F.route((6, 10, 10), (1, 0, 1)) == F.PLANE
    # axis-0 tiles: 169 columns stay at TL 13, 77 columns widen to 77, 77 x 64 is the largest tile
    assert F.axis_geom((7, 13, 13), 0).TL == 13 and F.axis_geom((9, 7, 11), 0).TL == 77
    assert F.axis_geom((64, 7, 11), 0).lds == 158720 <= F.AXIS_LDS_MAX
    assert F.axis_geom((64, 7, 13), 0) is None          # 91 x 64: 187392 bytes
    # the contiguous pass of (3, 50, 64): 150 lines in tiles of 32, the last one partial
    g = F.axis_geom((3, 50, 64), 2)
    assert (g.TL, g.outer, g.tiles_per_row) == (32, 150, 5) and g.outer % g.TL == 22
    assert F.herm_prefix(12, 0) == 7 and F.herm_prefix(12, 1) == 6
    assert F.herm_prefix(13, 0) == 7 and F.herm_prefix(13, 1) == 7
    assert F.herm_lines(12, 0) == (7, 1, 6, 0, 6, True)
    assert F.herm_lines(12, 1) == (6, 0, 6, -1, -1, True)
    assert F.herm_lines(13, 0) == (7, 1, 7, 0, -1, True)
    assert F.herm_lines(13, 1) == (7, 0, 6, -1, 6, True)
    assert not F.herm_lines(12, 3).ok
    assert F.slice_planes(8) == (1, 4, 3)


def test_every_case_is_accepted_and_every_reject_is_not():
    for c in F.all_cases():
        assert F.accepted(c.mesh, None, False, c.sliced, c.inplace, c.gather), c
        assert max(c.mesh) <= 64 and int(np.prod(c.mesh)) <= 36 ** 3 and c.rows in (2, 3)
    for mesh, m in F.GROUP_HERM:
        for v in F.HERM_VARIANTS:
            assert F.accepted(mesh, m, v.in_real, v.sliced, False, v.gather)
    for mesh, m in F.HERM_FULL:
        assert F.accepted(mesh, m) and F.base_route(mesh, m) in (F.PLANE, F.AXES)
    for r in F.GROUP_REJECT:
        assert not F.accepted(r.mesh, r.m, r.in_real, r.sliced, r.inplace, r.gather), r.name
    assert len({r.name for r in F.GROUP_REJECT}) == len(F.GROUP_REJECT)
    for name, g in F.GROUPS.items():
        assert len({F.cid(c) for c in g}) == len(g), name


def test_tables_reach_every_route_and_kernel():
    cases = F.all_cases()
    routes = {F.route(c.mesh) for c in cases} | {F.route(m, h) for m, h in F.GROUP_HERM}
    assert routes == {F.REG, F.REG_HERM, F.PLANE, F.PLANE | F.BIG, F.AXES, F.AXES | F.BIG}
    ks = [k for c in cases for k in F.kernels(c.mesh)]
    # every listed size as a plane size and as an axis-0 size, bare and with every option
    for opts in (F.plain, F.every):
        got = [k for c in F.GROUP_REG if c == opts(c.mesh) for k in F.kernels(c.mesh)]
        assert {n for k, n in got if k == "plane_reg"} == set(F.LISTED)
        assert {n for k, n in got if k == "axis0_reg"} == set(F.LISTED)
    assert any(c.mesh[0] != c.mesh[1] for c in F.GROUP_REG)
    # the Hermitian axis-0 kernel at both m0, even and odd n0
    hk = {k[1] for mesh, m in F.GROUP_HERM for k in F.kernels(mesh, m) if k[0] == "axis0_herm"}
    assert hk == {(n0, m0) for n0 in (8, 13, 15, 12, 16) for m0 in (0, 1)}
    # both instantiations of the LDS plane kernel and of the axis kernel, the latter in both routes
    assert {b for k, b in ks if k == "plane"} == {False, True}
    for r in (F.PLANE, F.AXES):
        for axis_from_end in (1, 2, 3) if r == F.AXES else (1,):
            seen = {F.kernels(c.mesh)[-axis_from_end][1] for c in cases if F.base_route(c.mesh) == r}
            assert seen == {False, True}, (r, axis_from_end)


def test_tables_reach_every_named_branch():
    cases = F.all_cases()
    lds = [c for c in cases if F.base_route(c.mesh) == F.PLANE]
    # plane kernel: planes above 8 x 256 points (the tail load loop), in both instantiations of
    # the plain route and with a plane table; a mesh dimension of 1 on every axis
    big_planes = [c for c in lds if c.mesh[1] * c.mesh[2] > 2048]
    assert {c.sliced for c in big_planes} == {False, True}
    assert any(c.kd is not None for c in big_planes)
    for ax in range(3):
        assert any(c.mesh[ax] == 1 for c in lds)
    # axis-0 pass of the plane route: narrow tile kept, tile widened beyond 64, the largest LDS
    g0 = {c.mesh: F.axis_geom(c.mesh, 0) for c in lds}
    assert any(g.inner > 64 and g.TL < 16 for g in g0.values())
    assert any(g.TL > 64 for g in g0.values())
    assert max(g.lds for g in g0.values()) == 158720
    assert any(g.TL * g.n > 2048 for g in g0.values())   # the kernel's own tail load loop
    # three axis passes: a partial last tile in the contiguous pass, with the phase
    ax = [c for c in cases if F.base_route(c.mesh) == F.AXES]
    part = [c for c in ax if F.axis_geom(c.mesh, 2).outer % F.axis_geom(c.mesh, 2).TL]
    assert {c.kd is not None for c in part} == {False, True}
    # options: each alone and together on every route, kd on an even and an odd mesh of each
    for r, meshes in F.OPTION_MESHES.items():
        assert all(F.base_route(m) == r for m in meshes)
        assert [all(n % 2 == 0 for n in m) for m in meshes] == [True, False]
        assert any(all(n % 2 == 1 for n in m[1:]) and m[0] % 2 == 1 for m in meshes)
        for m in meshes:
            got = {(c.gather, c.kd is not None, c.weight, c.inplace)
                   for c in F.GROUP_OPTIONS if c.mesh == tuple(m)}
            assert got == {(0, 1, 0, 0), (0, 0, 1, 0), (1, 0, 0, 0), (0, 0, 0, 1), (1, 1, 1, 0),
                           (0, 1, 1, 1)}
    # sliced input on a register mesh and on both instantiations of the plane kernel
    sk = {F.kernels(c.mesh)[0] for c in F.GROUP_SLICED}
    assert {k for k, _ in sk} == {"plane_reg", "plane"} and ("plane", True) in sk
    assert {(c.gather, c.weight) for c in F.GROUP_SLICED} == {(0, 0), (1, 0), (1, 1)}
    # Hermitian pairing: all eight m; line pairings with and without each self-paired line; the
    # partner lanes' weight, the gather, real rows and the plane table each occur
    assert {h for _, h in F.GROUP_HERM} == set(F.HERM_M) and len(F.HERM_M) == 8
    pair = {(l.sl0 >= 0, l.sl1 >= 0) for mesh, m in F.GROUP_HERM
            for l in [F.herm_lines(mesh[1], m[1])]}
    assert pair == {(True, True), (False, False), (True, False), (False, True)}
    assert any(F.herm_prefix(mesh[0], m[0]) < mesh[0] // 2 + 1 for mesh, m in F.GROUP_HERM)
    v = F.HERM_VARIANTS
    assert {(x.in_real, x.weight) for x in v} >= {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert any(x.gather and x.in_real for x in v) and any(x.gather and x.weight for x in v)
    assert any(x.sliced and x.weight and x.gather for x in v)
    assert not any(x.sliced and x.in_real for x in v)


def test_weight_and_slices():
    rng = np.random.default_rng(1)
    w = F.make_weight(rng, 20000)
    assert w[0] == 0.0 and 0 <= w.min() and w.max() < 2.0 and 100 <= (w == 0).sum() <= 300
    for mesh in F.SLICED_MESHES + F.HERM_MESHES:
        cnt = F.slice_planes(mesh[0])
        assert sum(cnt) == mesh[0] and len(set(cnt)) == 3
        base, ld, size = F.slice_layout(mesh, F.ROWS_IN)
        P = mesh[1] * mesh[2]
        assert len(base) == len(ld) == mesh[0] and len(set(ld)) == 3
        # no two (row, plane) blocks overlap and all lie inside the buffer
        used = np.zeros(size, dtype=int)
        for r in range(F.ROWS_IN):
            for i0 in range(mesh[0]):
                used[base[i0] + r * ld[i0]: base[i0] + r * ld[i0] + P] += 1
        assert used.max() == 1 and used[-F.SLICE_GAP:].sum() == 0
        # a kernel that took IN_LD_UNUSED for the stride would still read inside the buffer
        assert (base + (F.ROWS_IN - 1) * F.IN_LD_UNUSED + P <= size).all()


@pytest.mark.parametrize("mesh", [(8, 12, 12), (5, 7, 11), (13, 15, 15), (3, 50, 64), (1, 1, 1)])
def test_reference_matches_numpy_fftn(mesh):
    rng = np.random.default_rng(sum(mesh))
    x = F.rnd(rng, 2, int(np.prod(mesh)))
    w = F.make_weight(rng, x.shape[1])
    f = [np.fft.fftfreq(n) for n in mesh]
    ph = np.exp(-1j * (f[0][:, None, None] * F.KD[0] + f[1][None, :, None] * F.KD[1]
                       + f[2][None, None, :] * F.KD[2]))
    for kd, wt in ((None, None), (F.KD, None), (F.KD, w)):
        y = x.reshape(2, *mesh) * (ph if kd else 1.0)
        out = np.fft.fftn(y, axes=(1, 2, 3)).reshape(2, -1) * (1.0 if wt is None else wt)
        ref = F.ref_fft3d(x, mesh, kd, wt)
        assert ref.dtype == F.CLD
        assert F.rel_err(out, ref) < 1e-14
    assert float(abs(F.fftfreq_ld(mesh[1]) - f[1]).max()) < 1e-16


def test_reference_is_a_long_double_dft():
    """The DFT matrix is accurate beyond fp64 (W W^H = n I to long-double rounding) and pi is a
    long double."""
    assert np.finfo(F.LD).eps < 1e-18, "long double is no wider than double here"
    assert float(abs(np.sin(F.PI))) < 1e-18
    for n in (7, 13, 45, 64):
        W = F.dft_matrix(n)
        assert float(abs(W @ W.conj().T - n * np.eye(n)).max()) < 1e-16 * n


@pytest.mark.parametrize("mesh", [(8, 12, 12), (12, 13, 13)])
@pytest.mark.parametrize("m", F.HERM_M)
def test_paired_inputs_have_the_hermitian_identity(mesh, m):
    """Real rows times exp(-i f.kd), kd = pi m: F(-j - m) = conj F(j)."""
    rng = np.random.default_rng(sum(mesh) + 7 * sum(m))
    y = rng.standard_normal((2, int(np.prod(mesh))))
    ref = F.ref_fft3d(y, mesh, np.pi * np.array(m, dtype=float)).reshape(2, *mesh)
    j = [(-np.arange(n) - mm) % n for n, mm in zip(mesh, m)]
    partner = ref[:, j[0][:, None, None], j[1][None, :, None], j[2][None, None, :]]
    assert float(abs(partner - ref.conj()).max() / abs(ref).max()) < 1e-14
    # the prefix planes and their partners cover the mesh
    nH = F.half_prefix_planes(mesh[0], m[0])
    assert set(range(nH)) | {int(j[0][i]) for i in range(nH)} == set(range(mesh[0]))
