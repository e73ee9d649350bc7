"""What the GPU modules of the exact FFT-grid K share (test_gpu_kfft.py, test_gpu_kfft_lr.py): the
device context and kfft_cases' buffer conventions.  Every input is a view into a buffer of NaN,
every output a view into the sentinel 7 + 7j, which must come back bitwise."""
import numpy as np
import pytest

import kfft_cases as K

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
    """a (flat) on the device inside NaN: (buffer, view of the logical part)."""
    a = np.asarray(a, complex).ravel()
    buf = np.full(a.size + 2 * K.EDGE, NAN)
    buf[K.EDGE:K.EDGE + a.size] = a
    d = dev(torch, buf)
    return d, d[K.EDGE:K.EDGE + a.size]


def f_view(torch, f):
    """f (nk, ngrid, nao) with its k blocks f_kstride apart in NaN: (buffer, view, f_kstride)."""
    nk, ngrid, nao = f.shape
    ks = ngrid * nao + K.KPAD
    buf = np.full(nk * ks + 2 * K.EDGE, NAN)
    for k in range(nk):
        buf[K.EDGE + k * ks: K.EDGE + k * ks + ngrid * nao] = f[k].ravel()
    d = dev(torch, buf)
    return d, d[K.EDGE:], ks


def out_view(torch, n, fill=None):
    """n output elements inside the sentinel, themselves the sentinel or `fill`."""
    buf = np.full(n + 2 * K.EDGE, K.SENTINEL)
    if fill is not None:
        buf[K.EDGE:K.EDGE + n] = np.asarray(fill).ravel()
    d = dev(torch, buf)
    return d, d[K.EDGE:K.EDGE + n]


def edges_intact(d, n):
    h = d.cpu().numpy()
    return bool(np.all(h[:K.EDGE] == K.SENTINEL) and np.all(h[K.EDGE + n:] == K.SENTINEL))
