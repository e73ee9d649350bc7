#!/usr/bin/env python
"""Times the stages of the exact FFT-grid K in the occupied-orbital form for one (k1, k2) block of
C3 shape (FFT mesh 36^3, nao 26) at I orbitals per k-point — the orbitals on the grid (two zgemm),
fisdf_pair_density_lr, the two fft3d calls over the nao I rows, fisdf_exx_contract_lr — the whole
block through fisdf_get_k_fft_lr at a 1x1x1 k-mesh, and the whole call at --nk beside the dm form
(fisdf_get_k_fft) on the same arrays, each repeat of the whole calls on its own.  Synthetic device
arrays; needs a GPU (no fallback).  tools/kfft_bench.py has the dm form's stages.

Beside every time stands the traffic model of DESIGN 3.11 — passes over the block's
B = nao I ngrid 16 bytes: pair 1 (write), each two-pass FFT 4, conjugation 2, contraction 1 (read);
the orbitals read f twice and write 2 I ngrid 16 — and the time those bytes take at 5.3 TB/s.
One JSON line per I.

  python tools/kfft_lr_bench.py [--mesh 36 36 36] [--nao 26] [--nk 2 2 2] [--ranks 4 26]
                                [--nset 1] [--reps 20] [--warmup 2] [--call-reps 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fft-isdf-scratch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

MODEL_TBPS = 5.3
PASSES = {"pair": 1, "fft_w": 4, "fft": 4, "contract": 1, "block": 12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nk", type=int, nargs=3, default=[2, 2, 2])
    ap.add_argument("--mesh", type=int, nargs=3, default=[36, 36, 36])
    ap.add_argument("--nao", type=int, default=26)
    ap.add_argument("--ranks", type=int, nargs="+", default=[4, 26], help="orbitals per set and k")
    ap.add_argument("--nset", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--call-reps", type=int, default=3, help="repeats of the whole calls")
    args = ap.parse_args()

    import torch
    from fisdf import _lib as L
    if not torch.cuda.is_available():
        raise SystemExit("kfft_lr_bench: no GPU visible")
    ctx = L.Context(0, torch.cuda.current_stream().cuda_stream)
    nk, ngrid, nao, nset = int(np.prod(args.nk)), int(np.prod(args.mesh)), args.nao, args.nset
    a = np.diag([10.26, 10.26, 10.26]).astype(float)
    km, kmp = L.iarr(args.nk)
    k1, k1p = L.iarr([1, 1, 1])
    ms, msp = L.iarr(args.mesh)
    aa, ap_ = L.darr(a.ravel())
    kd, kdp = L.darr([0.83, -1.91, 2.6])
    one, zero = np.array([1.0, 0.0]), np.zeros(2)
    onep, zerop = one.ctypes.data_as(L._dp), zero.ctypes.data_as(L._dp)
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*shape):
        return torch.randn(*shape, dtype=torch.complex128, device="cuda", generator=gen)

    def timed(call, reps, warmup):
        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    f = rnd(nk, ngrid, nao)
    w = torch.rand(ngrid, dtype=torch.float64, device="cuda", generator=gen)
    D = rnd(nset, nk, nao, nao)
    out = torch.zeros(nset, nk, nao, nao, dtype=torch.complex128, device="cuda")

    def dm_call():
        ctx.call("fisdf_get_k_fft", L.ptr(f), ngrid * nao, kmp, msp, ap_, nao, L.ptr(D), nset, 0.0,
                 None, None, 0, 0, L.ptr(out))

    dm_ms = [round(timed(dm_call, 1, 1 if i == 0 else 0), 3) for i in range(args.call_reps)]
    for r in args.ranks:
        ni = nset * r
        seg, segp = L.iarr([s * r for s in range(nset + 1)])
        rk, rkp = L.iarr([r] * (nset * nk))
        A, B = rnd(nset, nk, nao, r), rnd(nset, nk, nao, r)
        psi, u = rnd(ngrid, ni), rnd(ni, ngrid)
        rows = rnd(nao * ni, ngrid)
        o1 = torch.zeros(nset, nao, nao, dtype=torch.complex128, device="cuda")
        block_bytes = rows.numel() * 16

        def orbitals():
            for s in range(nset):
                ctx.call("fisdf_zgemm", 0, 0, ngrid, r, nao, onep, L.ptr(f[0]), nao, 0,
                         L.ptr(A[s, 0]), r, 0, zerop, L._vp(psi.data_ptr() + 16 * s * r), ni, 0,
                         1, 1)
                ctx.call("fisdf_zgemm", 3, 3, r, ngrid, nao, onep, L.ptr(B[s, 0]), r, 0,
                         L.ptr(f[0]), nao, 0, zerop, L.ptr(u[s * r:]), ngrid, 0, 1, 1)

        def lr_call(kmesh_p):
            return lambda: ctx.call("fisdf_get_k_fft_lr", L.ptr(f), ngrid * nao, kmesh_p, msp, ap_,
                                    nao, L.ptr(A), L.ptr(B), rkp, r, nset, 0.0, None, None, 0, 0,
                                    L.ptr(out))

        stages = {
            "orbitals": orbitals,
            "pair": lambda: ctx.call("fisdf_pair_density_lr", L.ptr(f[-1]), nao, L.ptr(psi), ni, ni,
                                     ngrid, 0, nao, L.ptr(rows)),
            "fft_w": lambda: ctx.call("fisdf_fft3d_ex", L.ptr(rows), ngrid, None, L.ptr(rows),
                                      ngrid, nao * ni, msp, kdp, L.ptr(w), None, None, None, 0,
                                      None),
            "fft": lambda: ctx.call("fisdf_fft3d_ex", L.ptr(rows), ngrid, None, L.ptr(rows), ngrid,
                                    nao * ni, msp, None, None, None, None, None, 0, None),
            "contract": lambda: ctx.call("fisdf_exx_contract_lr", L.ptr(rows), L.ptr(u),
                                         L.ptr(f[0]), msp, kdp, 0, nao, nao, ni, segp, nset, 1.0,
                                         L.ptr(o1)),
            "block": lr_call(k1p),
        }
        res = {"form": "lowrank", "nk": nk, "ngrid": ngrid, "nao": nao, "nset": nset, "rank": r,
               "I": ni, "block_bytes": block_bytes, "model_TBps": MODEL_TBPS, "reps": args.reps}
        for name, call in stages.items():
            ms_call = timed(call, args.reps, args.warmup)
            nbytes = (2 * 16 * ngrid * (nao + ni) if name == "orbitals"
                      else PASSES[name] * block_bytes)
            model_ms = nbytes / (MODEL_TBPS * 1e12) * 1e3
            res[name + "_ms"] = round(ms_call, 4)
            res[name + "_model_bytes"] = nbytes
            res[name + "_model_ms"] = round(model_ms, 4)
            res[name + "_x_model"] = round(ms_call / model_ms, 2)
        # the whole calls, every repeat on its own (the first after one warm-up call)
        call = lr_call(kmp)
        res["call_ms"] = [round(timed(call, 1, 1 if i == 0 else 0), 3)
                          for i in range(args.call_reps)]
        res["call_model_ms"] = round(PASSES["block"] * nk * nk * block_bytes
                                     / (MODEL_TBPS * 1e12) * 1e3, 3)
        res["dm_call_ms"] = dm_ms
        res["dm_call_model_ms"] = round(PASSES["block"] * nk * nk * nao * nao * ngrid * 16
                                        / (MODEL_TBPS * 1e12) * 1e3, 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
