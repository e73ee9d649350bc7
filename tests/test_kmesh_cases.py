"""CPU checks of tests/kmesh_cases.py: the restated rules equal the library's own host functions
(fisdf_kmesh_plan, host only) over a sweep; the case tables of test_gpu_kmesh_variants.py reach
every instantiation, tier, refusal and branch the rules name (these assertions stand where the
earlier test commits had a mutant table: code made wrong on purpose is not run); the fused kernel's
tile walk visits every tile once; the references agree with numpy's FFT and with the explicit Phi
of the lattice; every float64 restatement is a sane float64 computation (within 16 n eps of the
long-double reference)."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import kmesh_cases as K


def _plan_lib():
    from fisdf import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfisdf.so not built (run __graft_entry__.build())")
    return _lib.load()


def plan(lib, kmesh, ncol=1, nao=1, nip=1, m=1):
    km = (C.c_int * 3)(*kmesh)
    rt, fb = (C.c_long * 3)(), (C.c_long * 2)()
    half, nruns = C.c_int(), C.c_int()
    cap = K.nk_of(kmesh)
    runs = np.zeros((cap, 2), np.int32)
    fused, slots = (C.c_int * 4)(), (C.c_int * 48)()
    rc = lib.fisdf_kmesh_plan(km, ncol, nao, nip, m, rt, C.byref(half),
                              runs.ctypes.data_as(C.POINTER(C.c_int)), cap, C.byref(nruns), fused,
                              slots, fb)
    assert rc == 0, lib.fisdf_last_error(None)
    nA, nB = fused[1], fused[2]
    return dict(route=tuple(rt), half=half.value,
                runs=[tuple(int(v) for v in r) for r in runs[:nruns.value]],
                fused=K.FusedPlan(bool(fused[0]), nA, nB, tuple(slots[:nA]),
                                  tuple(slots[nA:nA + nB]), fb[0], fused[3]),
                slots_tail=list(slots[nA + nB:]), work=fb[1])


def test_route_and_time_reversal_equal_the_host_functions():
    """Every k-mesh with axes 1..17 and at most 1300 points (and the refused one just above the LDS
    cap): route, tile tier, LDS bytes, stored-k count and runs."""
    lib = _plan_lib()
    n = 0
    seen = set()
    meshes = [km for km in itertools.product(range(1, 18), repeat=3) if K.nk_of(km) <= 1300]
    for km in meshes:
        p = plan(lib, km, ncol=1000)
        assert p["route"] == K.route(km, 1000), km
        assert p["half"] == len(K.reps(km)) and p["runs"] == K.rep_runs(km), km
        seen.add((p["route"][0], p["route"][1]))
        n += 1
    assert n > 2000 and seen == {(K.REG, 0), (K.REFUSED, 0), (K.REFUSED, 8)} | {
        (K.LDS, ct) for ct in (64, 32, 16, 8)}
    for km in K.REG_MESHES:                       # a column count the register kernels' int cannot hold
        assert plan(lib, km, ncol=2 ** 31 - 1)["route"][0] == K.REG
        assert plan(lib, km, ncol=2 ** 31)["route"] == K.route(km, 2 ** 31)
        assert K.route(km, 2 ** 31)[0] == K.LDS
    assert plan(lib, (1, 1, 3), ncol=64 * 2 ** 31)["route"] == K.route((1, 1, 3), 64 * 2 ** 31)
    assert K.route((1, 1, 3), 64 * 2 ** 31 - 63)[0] == K.REFUSED
    assert K.route((1, 1, 3), 64 * 2 ** 31 - 64)[0] == K.LDS
    # the figures the launch rule is documented with
    assert K.route((7, 8, 8)) == (K.LDS, 8, 67072) and K.route((16, 16, 4)) == (K.LDS, 8, 152320)
    assert K.route((16, 16, 5))[0] == K.REFUSED and K.route((17, 1, 1)) == (K.REFUSED, 0, 0)
    assert len(K.reps((4, 4, 4))) == 36 and len(K.reps((6, 6, 6))) == 112


def test_fused_plan_equals_the_host_functions():
    """Every listed k-mesh x nao 1..130, and meshes off the list: whether the fused kernel
    applies, its slots in order, LDS bytes, K chunks and workspace."""
    lib = _plan_lib()
    for km in K.REG_MESHES:
        for nao in range(1, 131):
            p = plan(lib, km, nao=nao, nip=37, m=53)
            want = K.fused_plan(km, nao)
            assert p["fused"] == want, (km, nao)
            assert want.applies == (nao <= 128)
            assert set(p["slots_tail"]) == {-1}
            assert p["work"] == K.fused_workspace(km, 37, nao, 53), (km, nao)
            if want.applies:                      # the workspace holds the plan's slots
                assert p["work"] >= 16 * (want.nA + want.nB) * nao * (37 + 53)
    for km in [(1, 1, 3), (3, 1, 2), (5, 5, 5), (6, 6, 6), (8, 8, 1), (1, 4, 4), (17, 1, 1)]:
        p = plan(lib, km, nao=8, nip=37, m=53)
        assert p["fused"] == K.NO_FUSED == K.fused_plan(km, 8), km
        assert p["work"] == K.fused_workspace(km, 37, 8, 53), km
    for km, nao, nip, m in [((2, 2, 2), 8, 0, 5), ((2, 2, 2), 8, 5, 0)]:
        assert plan(lib, km, nao=nao, nip=nip, m=m)["work"] == 0 == K.fused_workspace(km, nip, nao, m)


@pytest.mark.parametrize("km", K.REG_MESHES + [(1, 1, 3), (5, 5, 5), (7, 8, 8)], ids=str)
def test_partner_slot_and_plan_are_consistent(km):
    p, slot, r = K.partner(km), K.rep_slot(km), K.reps(km)
    assert np.array_equal(p[p], np.arange(p.size))            # an involution
    assert np.array_equal(slot[r], np.arange(r.size))         # representatives in ascending rows
    assert sum(e - b for b, e in K.rep_runs(km)) == r.size
    assert set(K.self_conjugate(km)) <= set(r)
    x = K.rnd(np.random.default_rng(1), r.size, 3)
    full = K.extend_half(x, km)
    pair = p != np.arange(p.size)                             # a self-conjugate k is taken as given
    assert np.array_equal(full[r], x) and np.array_equal(full[p][pair], full.conj()[pair])
    fp = K.fused_plan(km, 5)
    if fp.applies:
        assert sorted(fp.kA + fp.kB) == list(r)               # the plan reads the representatives
        n0, n1, n2 = km
        P, ip, rank = n1 * n2, K.inplane_partner(n1, n2), K.inplane_rank(n1, n2)
        R = int((np.arange(P) <= ip).sum())
        for i, k in enumerate(fp.kB):                         # slot = plane index * R + in-plane rank
            a, bc = divmod(k, P)
            assert i == (0 if a == 0 else 1) * R + rank[bc] and bc <= ip[bc]
        assert fp.kA == tuple(range(P, 2 * P))[:fp.nA]


def test_tile_walk_visits_every_tile_once():
    for nIt in range(1, 6):
        for nGt in range(1, 71):
            w = K.tile_walk(nIt, nGt)
            tiles = [t for t in w if t is not None]
            assert len(w) % (8 * K.GPAIR) == 0 and len(w) < 2 ** 31
            assert sorted(tiles) == [(it, gt) for it in range(nIt) for gt in range(nGt)], (nIt, nGt)
            # an XCD's g-tiles: workgroup id & 7 == gt & 7
            assert all(t is None or t[1] % 8 == b % 8 for b, t in enumerate(w))


def test_tables_reach_every_register_instantiation():
    got = {(c.kmesh, c.half, c.conj_out) for c in K.REG_Y_CASES}
    assert got == set(itertools.product(K.REG_MESHES, (0, 1), (0, 1)))
    for km in K.REG_MESHES:
        assert K.route(km)[0] == K.REG
        cs = [c for c in K.REG_Y_CASES if c.kmesh == km]
        assert {c.ncol for c in cs} == {1, 63, 64, 65, 200}
        assert {c.qsel for c in cs} == set(range(len(K.q_lists(km))))
        assert any(c.ncol % c.m and c.m > 1 for c in cs) and any(c.m == c.ncol for c in cs)
        assert any(c.goff > 0 and c.pad > 0 for c in cs)
    assert set(K.UNRUN_BEFORE) < set(K.REG_MESHES)
    assert K.q_lists((4, 4, 4))[K.REG_Y_BIT63.qsel] == [63]
    c = K.REG_Y_STRIDE
    assert -(-c.ncol // 64) > K.REG_GRID_CAP and c.ncol % 64 and c.ncol % c.m
    # x4, get_k's pair and the Bloch DFT run on REG_MESHES themselves
    assert {c.kmesh for c in K.X4_CASES if not c.dense} >= set(K.REG_MESHES)
    assert {(c.kmesh, c.tr) for c in K.X4_CASES if not c.dense} >= set(
        itertools.product(K.REG_MESHES, (0, 1)))
    assert {c.kmesh for c in K.X4_CASES if c.dense} == set(K.X4_DENSE_MESHES)
    assert {(c.nip, c.nao) for c in K.X4_CASES} == set(K.X4_SHAPES)
    assert {c.nip for c in K.X4_CASES} == {1, 17, 65} and {c.nao for c in K.X4_CASES} == {3, 8}
    assert K.route(K.WSRHO_OFF_LIST)[0] == K.LDS
    assert all(K.route(km)[0] == K.LDS for km in K.BLOCH_GENERIC)
    km, ncol = K.BLOCH_STRIDE
    assert -(-ncol // 64) > K.BLOCH_GRID_CAP and ncol % 64 and K.route(km)[0] == K.REG


def test_tables_reach_every_lds_tier_and_refusal():
    for km, ct in K.LDS_MESHES.items():
        assert K.route(km)[:2] == (K.LDS, ct), km
        cs = [c for c in K.LDS_Y_CASES if c.kmesh == km]
        assert {c.half for c in cs} == {0, 1}
        assert {c.ncol for c in cs} == {1, ct - 1, ct + 1, 3 * ct + 5}
    assert set(K.LDS_MESHES.values()) == {64, 32, 16, 8}
    assert K.route(K.LDS_ABOVE_64K)[2] > 64 * 1024
    assert 150 * 1024 - 2000 < K.route(K.LDS_NEAR_CAP)[2] <= K.LDS_CAP
    assert any(16 in km for km in K.LDS_MESHES) and {(16, 1, 1), (1, 16, 1), (1, 1, 16)} <= set(
        K.LDS_MESHES)
    c = K.LDS_Y_STRIDE
    assert -(-c.ncol // K.route(c.kmesh)[1]) > K.LDS_GRID_CAP
    assert [K.route(km)[0] for km in K.REFUSED_MESHES] == [K.REFUSED, K.REFUSED]
    assert max(K.REFUSED_MESHES[0]) > K.KM_MAXN and max(K.REFUSED_MESHES[1]) <= K.KM_MAXN


def test_tables_reach_every_fused_branch():
    got = set()
    for c in K.FUSED_CASES:
        assert K.fused_plan(c.kmesh, c.nao).applies, c
        got |= K.fused_branches(c)
    assert got == K.FUSED_BRANCHES, K.FUSED_BRANCHES - got
    for km in ((2, 2, 2), (4, 4, 1)):
        assert {c.nao for c in K.FUSED_CASES if c.kmesh == km} >= set(K.FUSED_NAO)
    for km in ((2, 2, 1), (3, 3, 1)):
        assert {c.nip for c in K.FUSED_CASES if c.kmesh == km} >= set(K.FUSED_NIP)
        assert {c.m for c in K.FUSED_CASES if c.kmesh == km} >= set(K.FUSED_M)
    assert any(c.goff > 0 and c.pad > 0 for c in K.FUSED_CASES)
    assert {c.kmesh for c in K.FUSED_CASES if c.real == 1} == {(2, 2, 2), (4, 4, 4), (2, 2, 4),
                                                                (3, 3, 3)}
    assert list(K.self_conjugate((3, 3, 3))) == [0] and len(K.self_conjugate((2, 2, 2))) == 8
    # a bit of rmask outside the q-list, beside a real slot inside it
    c = [c for c in K.FUSED_CASES if c.real == 2 and c.kmesh == (2, 2, 2)][0]
    qs, sc = set(K.q_lists(c.kmesh)[c.qsel]), set(K.self_conjugate(c.kmesh))
    assert qs & sc and sc - qs
    assert not K.fused_plan((2, 2, 2), K.FUSED_REFUSED_NAO).applies
    assert K.fused_plan((2, 2, 2), K.FUSED_REFUSED_NAO - 1).applies
    # it0 > 0: every streamed case has several row blocks; one and two streams, both row sizes
    assert {(c.kmesh, c.rows, c.two) for c in K.STREAMED_CASES} == set(
        itertools.product([(2, 2, 2), (4, 4, 4)], (16, 48), (0, 1)))
    assert all(c.nip > c.rows and c.nip % c.rows and c.nip % 16 for c in K.STREAMED_CASES)


def test_references_agree_with_numpy_and_the_lattice_phase():
    rng = np.random.default_rng(3)
    for km in [(2, 2, 4), (3, 3, 3), (4, 4, 1), (1, 1, 3), (5, 5, 5), (2, 9, 13)]:
        nk = K.nk_of(km)
        x = K.rnd(rng, nk, 4)
        want = np.fft.ifftn(x.reshape(km + (4,)), axes=(0, 1, 2)).reshape(nk, 4) * nk
        assert K.rel_err(K.mesh_dft(x, km, scale=False), want.astype(K.CLD)) < 1e-14
        phi = K.lattice_phase64(km, K.LATTICE)
        assert K.rel_err(K.mesh_dft(x, km), (phi @ x).astype(K.CLD)) < 1e-13
        y, mon = K.y_ref(x, km)
        fs = phi @ x
        assert K.rel_err(y, (phi.T @ (fs.real ** 2)).astype(K.CLD)) < 1e-13
        assert abs(mon - abs(fs.imag).max()) < 1e-13
        yc = K.y_ref(x, km, qs=[nk - 1], conj_out=True)[0]
        assert np.array_equal(yc[0], y[nk - 1].conj())
    # the oracle's formulas for x4 (fftisdf.py:38-46): x2_k = conj(X) X^T, Phi x2, square, Phi^H
    km = (2, 2, 4)
    X = K.tr_symmetric(rng, km, 5, 3)
    phi = K.lattice_phase64(km, K.LATTICE)
    x2 = np.einsum("kim,kjm->kij", X.conj(), X).reshape(16, 25)
    x4 = phi.conj().T @ ((phi @ x2) ** 2)
    ref, mon = K.x4_ref(X, km)
    assert K.rel_err(ref.reshape(16, 25), x4.astype(K.CLD)) < 1e-13 and mon < 1e-17 * abs(x2).max()
    p = K.partner(km)
    assert np.array_equal(X[p], X.conj())


def _within(err64, n):
    return err64 <= K.BOUND_FACTOR * n * K.EPS


def test_float64_restatements_stay_within_their_bound():
    """Each restatement is 16 n eps from the long-double reference at the most (n the longest
    sum), on every table: what the device bound is built from is itself a float64 result."""
    worst = {}

    def note(fam, err, n):
        assert _within(err, n), (fam, err, n)
        worst[fam] = max(worst.get(fam, 0.0), err)

    for c in K.REG_Y_CASES + [K.REG_Y_BIT63]:
        d = K.y_data(c.kmesh, c.ncol, c.half, c.conj_out, c.qsel)
        note("y register", d.err64, d.nsum)
        note("y monitor", d.mon64, d.nsum)
    for c in K.LDS_Y_CASES:
        d = K.y_data(c.kmesh, c.ncol, c.half, 0, c.qsel)
        note("y lds", d.err64, d.nsum)
    for c in K.FUSED_CASES:
        d = K.fused_data(c.kmesh, c.nip, c.m, c.nao)
        note("y fused", d.err64, d.nsum)
    for c in K.X4_CASES:
        d = K.x4_data(c.kmesh, c.nip, c.nao)
        note("x4", d.err64, d.nsum)
        note("x4 dense", d.err64_dense, d.nsum)
    for c in K.STREAMED_CASES:
        d = K.streamed_data(c.kmesh, c.nip, c.m, c.nao, c.ng0)
        note("y fused streamed", d.err64, d.nsum)
    for km in K.REG_MESHES:
        for ncol in K.WSRHO_NCOL:
            d = K.wsrho_data(km, ncol)
            note("get_k pair", d.err64, d.nsum)
            note("get_k pair dense", d.err64_dense, d.nsum)
    for km in K.REG_MESHES + K.BLOCH_GENERIC:
        for ncol in K.BLOCH_NCOL:
            d = K.bloch_data(km, ncol)
            note("bloch", d.err64, d.nsum)
    for nT, nkb in itertools.product(K.BAND_NT, K.BAND_NKB):
        d = K.band_data(nT, nkb, 65)
        note("band", d.err64, d.nsum)
    print({k: "%.1e" % v for k, v in worst.items()})
