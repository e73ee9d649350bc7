"""CPU checks of tests/gemm_cases.py: the case tables of test_gpu_gemm_variants.py reach every
loop variant zgemm() / herk() can choose (by the dispatch rule restated there), and the reference
helpers agree with a plain longdouble einsum."""
import numpy as np
import pytest

import gemm_cases as G


def _paths(cases):
    seen = {}
    for c in cases:
        p = G.gemm_path(c.opA, c.opB, c.M, c.N, c.K, c.batch, c.ks, c.mode)
        seen.setdefault((c.opA, c.opB, c.mode), set()).add(p)
    return seen


def test_dispatch_rule_examples():
    """The restated rule on the shapes whose landing place the case tables rely on."""
    assert G.gemm_path(0, 0, 70, 45, 20) == "ring2"
    assert G.gemm_path(0, 0, 70, 45, 32) == "ring2"
    assert G.gemm_path(0, 0, 70, 45, 37) == "plain"
    assert [G.gemm_path(3, 1, 70, 45, K, batch=3) for K in (40, 48, 56)] == ["pipe"] * 3
    assert G.gemm_path(0, 0, 33, 45, 20, ks=8) == "ring2" and G.splits_of(20, 8) == [1, 1, 1]
    assert G.gemm_path(0, 0, 70, 45, 77, ks=2) == "plain"
    # pipelined split-K whose last split runs 3, 2 and 1 K-steps
    for K, ks, last in ((104, 3, 3), (136, 4, 2), (168, 5, 1)):
        assert G.gemm_path(1, 1, 70, 45, K, ks=ks) == "pipe"
        assert G.splits_of(K, ks)[-1] == last and G.splits_of(K, ks)[0] == 5
    assert G.gemm_path(0, 0, 70, 520, 40) == "wide"
    assert G.gemm_path(0, 0, 70, 520, 0) == "wide" and G.gemm_path(0, 0, 70, 45, 0) == "ring2"
    assert G.gemm_path(0, 0, 70, 520, 37) == "plain"
    assert G.gemm_path(0, 0, 70, 520, 40, batch=2) == "pipe"
    assert G.gemm_path(0, 0, 70, 520, 40, ks=2) == "ring2"
    assert G.gemm_path(0, 0, 70, 520, 40, mode=2) == "plain"
    assert G.gemm_path(0, 0, 27, 600, 64, epi=G.EPI_REAL) == "pipe"
    assert G.gemm_path(0, 0, 64, 45, 64, mode=4) == "pipe"
    assert G.gemm_path(0, 0, 64, 45, 64, mode=5) == "plain"
    assert G.gemm_path(3, 0, 72, 45, 72, mode=8) == "pipe"
    assert G.gemm_path(3, 0, 130, 45, 130, mode=8) == "plain"
    assert G.herk_path(64, 40) == "pipe" and G.herk_path(64, 40, mode=2) == "plain"
    assert G.herk_path(64, 40, ks=2) == "ring2" and G.herk_path(64, 37) == "plain"


def test_mode0_covers_every_op_pair_and_loop():
    seen = _paths(G.GROUP_OPS)
    for (a, b) in G.OPS:
        assert seen[(a, b, 0)] >= {"ring2", "pipe", "plain"}, (a, b, seen.get((a, b, 0)))
    # all three phases of the 3-deep ring: K-step counts 5, 6, 7
    steps = {c.K // G.BK % G.RING for c in G.GROUP_OPS if c.K % G.BK == 0}
    assert steps == {0, 1, 2}


def test_every_mode_covers_its_op_pairs_and_loops():
    seen = _paths(G.all_gemm_cases())
    for mode in range(10):
        for (a, b) in G.OPS:
            if not G.supported(a, b, mode):
                assert (a, b, mode) not in seen
                continue
            want = set(G.mode_paths(mode))
            if (a, b) == (0, 0) and mode in (0, 1, 4, 5):
                want.add("wide")
            assert seen.get((a, b, mode), set()) >= want, (a, b, mode, seen.get((a, b, mode)))
    # split-K: every op pair of the group in each loop, batch 1 and 2, beta zero and not
    sk = {}
    for c in G.GROUP_SPLITK:
        sk.setdefault((c.opA, c.opB), set()).add(
            (G.gemm_path(c.opA, c.opB, c.M, c.N, c.K, c.batch, c.ks), c.batch, c.beta))
    for ops in G.SPLITK_OPS:
        assert len(sk[ops]) == 3 * 2 * 2
    # the short last splits of the pipelined loop
    assert {G.splits_of(c.K, c.ks)[-1] for c in G.GROUP_SPLITK
            if G.gemm_path(c.opA, c.opB, c.M, c.N, c.K, c.batch, c.ks) == "pipe"} >= {1, 2, 3}
    # mode 8 with split-K in every loop
    assert {G.gemm_path(c.opA, c.opB, c.M, c.N, c.K, c.batch, c.ks, 8)
            for c in G.GROUP_UPPER if c.ks > 1} == {"ring2", "pipe", "plain"}
    # HERK: both modes in each loop they can take, with and without split-K
    hk = {(mode, G.herk_path(n, K, ks, mode), ks > 1) for (n, K, ks, mode) in G.GROUP_HERK}
    assert {(0, "pipe", False), (0, "plain", False), (0, "ring2", False), (0, "ring2", True),
            (0, "plain", True), (0, "pipe", True), (2, "plain", False), (2, "ring2", False),
            (2, "ring2", True), (2, "plain", True)} <= hk
    assert {G.herk_path(n, K) for (n, K) in G.GROUP_HERK_BATCHED} == {"pipe", "plain"}


def test_dispatch_table_is_complete():
    assert len(G.GROUP_DISPATCH) == 160 and len(set(G.GROUP_DISPATCH)) == 160
    assert sum(G.supported(a, b, m) for (a, b, m) in G.GROUP_DISPATCH) == 16 + 3 * 2 + 2 + 2


def _ld(x):
    return np.asarray(x).astype(np.clongdouble)


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(543)
    return rng


@pytest.mark.parametrize("opA,opB", G.OPS)
def test_ref_gemm_matches_longdouble_einsum(small, opA, opB):
    M, N, K = 5, 4, 3
    A = G.rnd(small, *G.stored_shape(opA, M, K))
    B = G.rnd(small, *G.stored_shape(opB ^ 1, N, K))
    C0 = G.rnd(small, M, N)
    a, b = _ld(A), _ld(B)
    a = a.T if opA & 1 else a
    a = a.conj() if opA & 2 else a
    b = b.T if opB & 1 else b
    b = b.conj() if opB & 2 else b
    acc = np.einsum("mk,kn->mn", a, b)
    ref = _ld(G.ALPHA) * acc + _ld(G.BETA) * _ld(C0)
    out = G.ref_gemm(A, B, opA, opB, G.ALPHA, G.BETA, C0)
    assert abs(out - ref).max() < 1e-14
    assert abs(G.ref_gemm(A, B, opA, opB, G.ALPHA) - _ld(G.ALPHA) * acc).max() < 1e-14
    # the modes, on the same operands (square case for the triangles)
    re = np.einsum("mk,kn->mn", _ld(a.real), b)
    assert abs(G.ref_acc(A, B, opA, opB, G.A_REAL) - re).max() < 1e-14
    assert abs(G.ref_acc(A, B, opA, opB, G.RE_ONLY) - _ld(acc.real)).max() < 1e-14
    assert abs(G.ref_acc(A, B, opA, opB, 3) - _ld(re.real)).max() < 1e-14


def test_ref_triangles_match_longdouble_einsum(small):
    M, N, K = 5, 4, 5
    A, B = G.rnd(small, M, K), G.rnd(small, K, N)
    low = np.einsum("mk,kn->mn", _ld(np.tril(A)), _ld(B))
    assert abs(G.ref_acc(A, B, 0, 0, G.A_LOWER) - low).max() < 1e-14
    lowre = np.einsum("mk,kn->mn", _ld(np.tril(A).real), _ld(B))
    assert abs(G.ref_acc(A, B, 0, 0, 5) - lowre).max() < 1e-14
    Bc = G.rnd(small, N, K)
    ah = _ld(np.triu(A.conj().T))
    assert abs(G.ref_acc(A, B, 3, 0, G.A_UPPER) - np.einsum("mk,kn->mn", ah, _ld(B))).max() < 1e-14
    assert abs(G.ref_acc(A, Bc, 3, 3, G.A_UPPER)
               - np.einsum("mk,nk->mn", ah, _ld(Bc).conj())).max() < 1e-14


def test_ref_herk_and_epilogues_match_longdouble_einsum(small):
    n, K = 5, 3
    A, C0 = G.rnd(small, n, K), G.rnd(small, n, n)
    acc = np.einsum("ik,jk->ij", _ld(A), _ld(A).conj())
    assert abs(G.ref_herk(A, -0.75) - (-0.75) * acc).max() < 1e-14
    assert abs(G.ref_herk(A, -0.75, mode=G.RE_ONLY) - (-0.75) * acc.real).max() < 1e-14
    assert (G.ref_herk(A, -0.75, mode=G.RE_ONLY).imag == 0).all()
    assert abs(G.ref_herk(A, -1.0, 1.0, C0) - (_ld(C0) - acc)).max() < 1e-14
    M, N = 5, 4
    P = G.rnd(small, M, N)
    aux = small.standard_normal((M, N))
    v = _ld(G.ALPHA) * _ld(P)
    mon = float(abs(v.imag).max())
    for epi, want in ((G.EPI_STREAM, v), (G.EPI_CSQUARE, v * v), (G.EPI_REAL, v.real),
                      (G.EPI_WSRHO, aux * v.real)):
        out, m = G.ref_epilogue(P, G.ALPHA, epi, aux)
        assert abs(out - want).max() < 1e-14
        assert abs(m - (0.0 if epi == G.EPI_STREAM else mon)) < 1e-14
    assert G.ref_epilogue(P.real + 0j, 0.5, G.EPI_CSQUARE)[1] == 0.0


def test_padded_layout(small):
    buf, view, stride = G.padded(3, 5, 4, 4 + G.PAD_C, G.SENTINEL)
    assert stride == 5 * 11 + G.GAP and buf.size == 3 * stride
    view[...] = G.rnd(small, 3, 5, 4)
    mask = G.padding_mask(3, 5, 4, 11)
    assert mask.sum() == buf.size - 60 and (buf[mask] == G.SENTINEL).all()
    assert np.array_equal(G.logical(buf, 3, 5, 4, 11), view)
    A, B, clean = G.make_operands(G.Gemm(3, 0, 130, 45, 130, 2, 1, 8, 0), small)
    assert A.shape == (2, 130, 130) and B.shape == (2, 130, 45)
    assert abs(A[:, 10, 70]).max() > 10 and (A[:, 64, 70] == 0).all() and (clean[:, 10, 70] == 0).all()
    A, B, clean = G.make_operands(G.Gemm(0, 0, 130, 45, 130, 2, 1, 4, 0), small)
    assert abs(A[:, 10, 70]).max() > 10 and (A[:, 10, 20] == 0).all() and (clean[:, 10, 70] == 0).all()
