"""The triangular GEMM's diagonal section (zgemm_wide.hip, GEMM_A_LOWER): in the last K-steps of
a 64-row M-tile — its diagonal 64 x 64 square of A — only the 16-row blocks that still hold
nonzeros issue MFMAs, and every wave of such a tile owns all its row blocks x 32 columns.

Every case goes through fisdf_zgemm_mode with N >= 512, so the 64 x 128-tile kernel runs.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from fisdf import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ctx = _lib.Context(0, torch.cuda.current_stream().cuda_stream)
    return torch, _lib, ctx


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rnd(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def gemm_mode(env, A, B, C0, beta, mode):
    """C = A B + beta C0 through fisdf_zgemm_mode (NN, one batch); returns C on the host."""
    torch, L, ctx = env
    (M, K), N = A.shape, B.shape[1]
    dA, dB, dC = dev(torch, A), dev(torch, B), dev(torch, C0)
    one, vb = np.array([1.0, 0.0]), np.array([float(beta), 0.0])
    ctx.call("fisdf_zgemm_mode", 0, 0, M, N, K, one.ctypes.data_as(L._dp), L.ptr(dA), K, 0,
             L.ptr(dB), N, 0, vb.ctypes.data_as(L._dp), L.ptr(dC), N, 0, 1, mode)
    return dC.cpu().numpy()


# (M, K): one full tile; M-edge tiles (<= 32 rows) with a diagonal section of 8 and of 24 columns
# (the latter is the last tile of nip = 600); a non-edge last tile with 40 rows; two and four
# tiles; nip = 600; K < M (tiles with no diagonal section); K > M; K % 8 != 0 (the unpipelined
# 64 x 64 kernel takes it and must stay correct)
SHAPES = [(64, 64), (72, 72), (88, 88), (104, 104), (128, 128), (200, 200), (600, 600),
          (200, 64), (64, 128), (129, 17)]
CASES = [(M, K, N, mode, 0) for (M, K) in SHAPES for N in (512, 777) for mode in (4, 5)]
CASES += [(200, 200, 777, 4, 1), (600, 600, 512, 5, 1)]


@pytest.mark.parametrize("M,K,N,mode,beta", CASES)
def test_tri_diag_matches_numpy(env, M, K, N, mode, beta):
    """tril(A) @ B (Re A for mode 5) against numpy at the tolerance of test_zgemm_modes_wide.
    Past each 64-row M-tile's last row A holds garbage that must never be read."""
    rng = np.random.default_rng(M * 7 + N + K + mode + beta)
    A, B = rnd(rng, M, K), rnd(rng, K, N)
    Aeff = A.real.astype(complex) if mode & 1 else A.copy()
    Aeff = np.tril(Aeff)
    beyond = np.arange(K)[None, :] >= 64 * (np.arange(M)[:, None] // 64 + 1)
    A = np.tril(A) + np.where(beyond, rnd(rng, M, K) * 1e3, 0)
    C0 = rnd(rng, M, N) if beta else np.zeros((M, N), complex)
    out = gemm_mode(env, A, B, C0, beta, mode)
    ref = Aeff @ B + beta * C0
    err = abs(out - ref).max()
    print(f"M={M} K={K} N={N} mode={mode} beta={beta}: err {err:.2e}")
    assert err < 1e-12 * max(K, 16), err


@pytest.mark.parametrize("N", [512, 777])
@pytest.mark.parametrize("M", [128, 600, 88])
@pytest.mark.parametrize("mode", [4, 5])
def test_tri_diag_equals_dense_mode(env, M, N, mode):
    """On the same tril(A) (exact zeros above the diagonal) and B, the lower-triangular mode
    equals the same kernel's dense mode (4 vs 0, 5 vs 1) as numbers: the dense mode multiplies
    the zeros the triangular mode skips, and every element of C is accumulated over ascending k
    by one lane either way.  K = M is a multiple of 8: both run the pipelined loop."""
    rng = np.random.default_rng(M + N + mode)
    A, B = np.tril(rnd(rng, M, M)), rnd(rng, M, N)
    C0 = np.zeros((M, N), complex)
    tri = gemm_mode(env, A, B, C0, 0, mode)
    dense = gemm_mode(env, A, B, C0, 0, mode & 1)
    assert np.array_equal(tri, dense), abs(tri - dense).max()
