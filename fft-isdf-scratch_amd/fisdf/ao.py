"""Bloch AO values on the GPU: the input layer PySCF's
``pbc_eval_gto('GTOval', coords, kpts)`` provides to ``fftisdf.py:72,367-370``.

``eval_ao_kpts_gpu`` returns the same array as ``cell.eval_ao_kpts`` (the host restatement),
computed by ``fisdf_eval_ao`` (csrc/ao.hip) and left resident on the device.  ``deriv=1`` adds the
first derivatives (``fisdf_eval_ao_deriv1``): (nk, 4, ng, nao), component 0 the value and 1..3
d/dx, d/dy, d/dz — PySCF's ``eval_ao_kpts(..., deriv=1)`` layout per k-point."""
from __future__ import annotations

import numpy as np

from . import _lib
from .cell import cell_rcut, lattice_translations


def _shell_tables(cell):
    sh_atom, sh_l, sh_np, exps, coefs = [], [], [], [], []
    for (ia, l, e, c, _ao0) in cell.shells:
        sh_atom.append(ia)
        sh_l.append(l)
        sh_np.append(len(e))
        exps.extend(np.asarray(e, float).tolist())
        coefs.extend(np.asarray(c, float).tolist())
    return (np.asarray(sh_atom, np.int32), np.asarray(sh_l, np.int32), np.asarray(sh_np, np.int32),
            np.asarray(exps, np.float64), np.asarray(coefs, np.float64))


def _check_deriv(deriv):
    if deriv not in (0, 1):
        raise ValueError(f"deriv must be 0 or 1, not {deriv!r}")


def eval_ao_band_gpu(device, cell, coords, kpts, deriv=0, tn=None):
    """chi_k(r) at arbitrary k-points ``kpts`` (nkb, 3) (``fisdf_eval_ao_band``; host
    restatement ``cell.eval_ao_band``): device tensor (nkb, ng, nao), or (nkb, 4, ng, nao) with
    ``deriv=1``.  tn: the lattice translations (default: those of ``coords``)."""
    _check_deriv(deriv)
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    kpts = np.ascontiguousarray(np.asarray(kpts, float).reshape(-1, 3))
    ng, nao = coords.shape[0], cell.nao_nr()
    tn = np.ascontiguousarray(lattice_translations(cell, coords) if tn is None else tn,
                              dtype=np.int32)
    sh_atom, sh_l, sh_np, exps, coefs = _shell_tables(cell)
    atoms = np.ascontiguousarray(cell.atom_coords(), dtype=np.float64)
    dcoords = device.torch.as_tensor(coords, device=device.dev)
    out = device.empty((len(kpts), 4, ng, nao) if deriv else (len(kpts), ng, nao))
    a, ap = _lib.darr(np.asarray(cell.lattice_vectors(), float).ravel())
    ip, dp = _lib._ip, _lib._dp
    device.ctx.call("fisdf_eval_ao_band_deriv1" if deriv else "fisdf_eval_ao_band", _lib.ptr(dcoords), ng, len(atoms),
                    atoms.ctypes.data_as(dp), len(sh_l), sh_atom.ctypes.data_as(ip),
                    sh_l.ctypes.data_as(ip), sh_np.ctypes.data_as(ip), exps.ctypes.data_as(dp),
                    coefs.ctypes.data_as(dp), len(tn), tn.ctypes.data_as(ip), len(kpts),
                    kpts.ctypes.data_as(dp), ap, cell_rcut(cell), nao, _lib.ptr(out))
    return out


def eval_ao_kpts_gpu(device, cell, coords, kmesh, deriv=0, tn=None):
    """chi_k(r) for the k-mesh ``kmesh`` at ``coords`` (ng, 3): device tensor (nk, ng, nao), or
    (nk, 4, ng, nao) with ``deriv=1``.  tn: the lattice translations (default: those of
    ``coords``)."""
    _check_deriv(deriv)
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    ng = coords.shape[0]
    kmesh = [int(k) for k in kmesh]
    nk = int(np.prod(kmesh))
    nao = cell.nao_nr()
    tn = np.ascontiguousarray(lattice_translations(cell, coords) if tn is None else tn,
                              dtype=np.int32)
    sh_atom, sh_l, sh_np, exps, coefs = _shell_tables(cell)
    atoms = np.ascontiguousarray(cell.atom_coords(), dtype=np.float64)
    torch = device.torch
    dcoords = torch.as_tensor(coords, device=device.dev)
    out = device.empty((nk, 4, ng, nao) if deriv else (nk, ng, nao))
    km, kmp = _lib.iarr(kmesh)
    a, ap = _lib.darr(np.asarray(cell.lattice_vectors(), float).ravel())
    ip, dp = _lib._ip, _lib._dp
    device.ctx.call("fisdf_eval_ao_deriv1" if deriv else "fisdf_eval_ao", _lib.ptr(dcoords), ng, len(atoms),
                    atoms.ctypes.data_as(dp), len(sh_l), sh_atom.ctypes.data_as(ip),
                    sh_l.ctypes.data_as(ip), sh_np.ctypes.data_as(ip), exps.ctypes.data_as(dp),
                    coefs.ctypes.data_as(dp), len(tn), tn.ctypes.data_as(ip), kmp, ap,
                    cell_rcut(cell), nao, _lib.ptr(out))
    return out
