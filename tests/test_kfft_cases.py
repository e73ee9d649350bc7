"""tests/kfft_cases.py checked on the CPU: the restated plan rule against fisdf_kfft_plan (the
host functions the launchers call), the reach of the case tables, and the references against the
oracle's exact_k and the golden file."""
import ctypes as C
import os

import numpy as np

import fft_cases as F
import kfft_cases as K
from cases import inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def lib_plan(lib, nao, ngrid, nset, work):
    mc, nch, rl, nr, tw, nn = (C.c_int() for _ in range(6))
    row, tot = C.c_long(), C.c_long()
    rc = lib.fisdf_kfft_plan(nao, ngrid, nset, work, C.byref(mc), C.byref(nch), C.byref(rl),
                             C.byref(nr), C.byref(tw), C.byref(nn), C.byref(row), C.byref(tot))
    assert rc == 0
    return K.Plan(mc.value, nch.value, rl.value, nr.value, tw.value, nn.value, row.value, tot.value)


def test_plan_rule_matches_library():
    from fisdf import _lib
    lib = _lib.load()
    n = 0
    for nao in range(1, 81):
        for ngrid in (1, 63, 64, 65, 512, 1000, 1728, 46656):
            for nset in range(1, 7):
                for work in K.budget_ladder(nao, ngrid):
                    if work < 0:
                        continue
                    got, want = lib_plan(lib, nao, ngrid, nset, work), K.plan(nao, ngrid, nset, work)
                    assert got == want, (nao, ngrid, nset, work, got, want)
                    n += 1
    assert n > 20000
    # beyond 128: still the four-tile instantiation; sizes whose products would not fit a long
    # are an error, not an overflow
    for nao in (128, 129, 130, 1000, K.MAX_NAO):
        for ngrid in (512, 2 ** 31 - 1):
            assert lib_plan(lib, nao, ngrid, 1, 0) == K.plan(nao, ngrid, 1, 0)
    assert K.plan(129, 512, 1, 0).exx_nn == 4 and K.plan(129, 512, 1, 0).mc == 129
    assert lib_plan(lib, K.MAX_NAO, 2 ** 31 - 1, K.MAX_SETS, 0) == K.plan(K.MAX_NAO, 2 ** 31 - 1,
                                                                         K.MAX_SETS, 0)
    for bad in ((0, 512, 1, 0), (K.MAX_NAO + 1, 512, 1, 0), (2 ** 31 - 1, 2 ** 31 - 1, 1, 0),
                (3, 512, K.MAX_SETS + 1, 0), (3, 2 ** 31, 1, 0), (3, 512, 1, -1)):
        assert lib.fisdf_kfft_plan(*bad, *([None] * 8)) < 0


def test_plan_edges():
    row = 16 * 13 * 512
    assert K.plan(13, 512, 1, row - 1).mc == 0                 # one byte short of a row m
    assert K.plan(13, 512, 1, row) [:2] == (1, 13)
    assert K.plan(13, 512, 1, 2 * row + 5)[:2] == (2, 7)       # a partial last chunk
    assert K.plan(13, 512, 1, 10 ** 12)[:2] == (13, 1)         # capped at nao
    assert K.plan(26, 46656, 1, 0)[:2] == (26, 1)              # the default holds C3 whole
    assert K.grid_split(46656) == (384, 122)
    assert K.grid_split(260) == (64, 5) and 260 % 64           # a partial last run
    assert K.grid_split(9216) == (128, 72)                     # two tiles per run


def test_tables_reach_every_path():
    tws = {K.plan(c.nao, c.ngrid, 1).pair_tw for c in K.PAIR_CASES}
    assert tws == set(K.PAIR_TWS)
    assert {c.same for c in K.PAIR_CASES} == {True, False}
    assert {(c.ngrid, c.nao) for c in K.PAIR_CASES} == {(g, n) for g in K.PAIR_NGRIDS
                                                        for n in K.PAIR_NAOS}
    for nao in K.PAIR_NAOS:
        r = K.row_ranges(nao)
        assert (0, nao) in r and all(0 <= a < b <= nao for a, b in r)
        if nao > 2:
            assert any(b - a == 1 for a, b in r) and len(r) == 3
    # the contraction: every mesh x nao, every set count and kd kind on every mesh
    seen = {(c.mesh, c.nao) for c in K.CONTRACT_CASES}
    assert seen >= {(m, n) for m in K.CONTRACT_MESHES for n in K.CONTRACT_NAOS}
    for m in K.CONTRACT_MESHES:
        assert {c.nset for c in K.CONTRACT_CASES if c.mesh == m} == set(K.CONTRACT_NSETS)
        assert {c.kd_kind for c in K.CONTRACT_CASES if c.mesh == m} == set(K.KD_KINDS)
    full = {(c.mesh, c.nao, c.nset) for c in K.CONTRACT_CASES}
    assert full >= {(m, n, s) for m in K.CONTRACT_MESHES for n in K.CONTRACT_NAOS
                    for s in K.CONTRACT_NSETS}
    for n in K.CONTRACT_NAOS:
        assert {c.kd_kind for c in K.CONTRACT_CASES if c.nao == n} == set(K.KD_KINDS)
    for s_ in K.CONTRACT_NSETS:
        assert {c.kd_kind for c in K.CONTRACT_CASES if c.nset == s_} == set(K.KD_KINDS)
    # every (sets, n-tiles) instantiation the launcher can pick, and more than one column group
    inst, groups = set(), set()
    for c in K.CONTRACT_CASES:
        i, g = K.exx_instantiations(c.nao, c.nset)
        inst |= i
        groups.add(g)
    assert inst == {(sc, nn) for sc in (1, 2, 3, 4) for nn in K.EXX_NNS}
    assert groups == {1, 2}
    assert K.WIDE_NAO % K.EXX_NT and K.WIDE_NAO % K.EXX_MT       # partial n-tile and m-tile
    assert any(c.nset > K.SET_CHUNK for c in K.CONTRACT_CASES)            # two set chunks
    splits = [K.grid_split(int(np.prod(c.mesh))) + (int(np.prod(c.mesh)),) for c in K.CONTRACT_CASES]
    assert any(g % rl for rl, nr, g in splits)                            # a partial last run
    assert any(rl > K.GT for rl, nr, g in splits)                         # more than one tile a run
    assert any(nr > 1 for rl, nr, g in splits)
    # get_k: mc = 1, a value not dividing nao, nao; every fft route the GPU cases use
    for c in K.GETK_CASES:
        ngrid = int(np.prod(c.mesh))
        mcs = [K.plan(c.nao, ngrid, c.nset, w).mc for w in K.getk_budgets(c)]
        assert mcs == [1, 2, c.nao] and c.nao % 2
        assert F.route(c.mesh) == K.GETK_ROUTES[c.mesh] and F.accepted(c.mesh, inplace=True)
    assert {F.route(c.mesh) for c in K.GETK_CASES} == set(K.GETK_ROUTES.values())
    assert not F.accepted(K.REFUSED_MESH)
    assert {c.kmesh for c in K.GETK_CASES} == {(1, 1, 1), (2, 1, 1), (1, 2, 3)}
    assert {c.omega for c in K.GETK_CASES} == {0.0, 0.4, -0.4}
    assert {c.nao for c in K.GETK_CASES} == {3, 13} and {c.nset for c in K.GETK_CASES} == {1, 2}
    assert {c.band for c in K.GETK_CASES} == {None, "off", "on"}


def test_exact_k64_is_the_oracle():
    from oracle.exact_ref import exact_k
    from oracle.isdf_ref import get_kpts
    cell, kmesh, m0, c0, x0, coords, chi, dm = inputs("toy222")
    kpts = get_kpts(cell.a, kmesh)
    mine = K.exact_k64(chi, chi, kpts, kpts, dm, cell.a, cell.mesh)
    ref = exact_k(chi, dm, cell.a, cell.mesh, kpts, coords)
    assert abs(mine - ref).max() <= 1e-12 * abs(ref).max()
    gold = np.load(os.path.join(GOLDEN, "toy222.npz"))["vk_exact"]
    assert abs(mine - gold).max() <= 1e-12 * abs(gold).max()


def test_long_double_reference_and_float64_agree():
    c = K.GETK_CASES[3]
    ref, err64 = K.getk_refs(c)
    assert ref.dtype == K.CLD and 0 < err64 < 1e-13
    c = next(c for c in K.CONTRACT_CASES if c.nao == 13 and c.nset == 2)
    Z, u, f1, vk0 = K.contract_inputs(c)
    a = K.contract_ref(Z, u, f1, c.mesh, K.contract_kd(c), 0, c.nao, 0.5)
    b = K.contract_ref(Z, u, f1, c.mesh, K.contract_kd(c), 0, c.nao, 0.5, wide=False)
    assert 0 < K.rel_err(b, a) < 1e-13
    # rows of a range are the rows of the whole
    part = K.contract_ref(Z[c.nao:2 * c.nao], u, f1, c.mesh, K.contract_kd(c), 1, 2, 0.5)
    assert np.array_equal(part[:, 0], a[:, 1])


def test_omega_variants():
    c = K.GETK_CASES[3]._replace(nset=1)
    f, D, kpts, _, _ = K.getk_inputs(c)
    k0 = K.exact_k64(f, f, kpts, kpts, D, K.LATTICE, c.mesh, 0.0)
    for w in (0.4, -0.4):
        kw = K.exact_k64(f, f, kpts, kpts, D, K.LATTICE, c.mesh, w)
        assert abs(kw - k0).max() > 1e-3 * abs(k0).max()
    # long range + short range = the full kernel wherever both are defined (not at k + G = 0,
    # where the full kernel drops the term and the short-range one has its finite limit)
    for q in (np.zeros(3), kpts[1] - kpts[0]):
        full, lr, sr = (K.coulG(K.LATTICE, q, c.mesh, w) for w in (0.0, 0.4, -0.4))
        keep = full > 0
        assert keep.sum() >= full.size - 1 - (abs(q).sum() > 0) * full.size // 2
        assert abs(lr + sr - full)[keep].max() <= 1e-13 * full.max()


def test_dms_are_not_hermitian():
    for c in K.GETK_CASES:
        f, D, kpts, kband, fb = K.getk_inputs(c)
        Dh = 0.5 * (D + D.conj().swapaxes(-1, -2))
        args = (f, f if fb is None else fb, kpts, kpts if kband is None else kband)
        a = K.exact_k64(*args, D, K.LATTICE, c.mesh, c.omega)
        b = K.exact_k64(*args, Dh, K.LATTICE, c.mesh, c.omega)
        assert abs(a - b).max() > 1e-3 * abs(a).max(), K.getk_id(c)
