#!/usr/bin/env python
"""Times the stages of the exact FFT-grid K (fisdf_pair_density, the two fft3d calls over the
block, fisdf_exx_contract) for one (k1, k2) block of C3 shape (FFT mesh 36^3, nao 26, all nao rows
m in one chunk), the whole block through fisdf_get_k_fft at a 1x1x1 k-mesh (the stages plus the
conjugation, u = D f^H and the Coulomb weight), and the whole call at a 2x2x2 k-mesh, on synthetic
device arrays.  Needs a GPU (no fallback).

Beside every time stands the traffic model of DESIGN 3.10 — passes over the block's
B = nao^2 ngrid 16 bytes: pair 1 (write), each two-pass FFT 4 (read + write per pass), conjugation
2, contraction 1 (read) — and the time those bytes take at the 5.3 TB/s of the FFT.
First measurements: no threshold.  One JSON line per nset.

  python tools/kfft_bench.py [--mesh 36 36 36] [--nao 26] [--nk 2 2 2] [--nsets 1 2]
                             [--reps 20] [--warmup 2] [--call-reps 3]
                             [--only pair|fft_w|fft|contract|block|call]
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
    ap.add_argument("--nsets", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--call-reps", type=int, default=3, help="repetitions of the whole call")
    ap.add_argument("--only", choices=list(PASSES) + ["call"], default=None)
    args = ap.parse_args()

    import torch
    from fisdf import _lib as L
    if not torch.cuda.is_available():
        raise SystemExit("kfft_bench: no GPU visible")
    ctx = L.Context(0, torch.cuda.current_stream().cuda_stream)
    nk, ngrid, nao = int(np.prod(args.nk)), int(np.prod(args.mesh)), args.nao
    a = np.diag([10.26, 10.26, 10.26]).astype(float)
    km, kmp = L.iarr(args.nk)
    k1, k1p = L.iarr([1, 1, 1])
    ms, msp = L.iarr(args.mesh)
    aa, ap_ = L.darr(a.ravel())
    kd, kdp = L.darr([0.83, -1.91, 2.6])
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*shape):
        return torch.randn(*shape, dtype=torch.complex128, device="cuda", generator=gen)

    f = rnd(nk, ngrid, nao)
    rows = rnd(nao * nao, ngrid)
    w = torch.rand(ngrid, dtype=torch.float64, device="cuda", generator=gen)
    block_bytes = rows.numel() * 16
    for nset in args.nsets:
        D = rnd(nset, nk, nao, nao)
        u = rnd(nset, nao, ngrid)
        out = torch.zeros(nset, nk, nao, nao, dtype=torch.complex128, device="cuda")
        stages = {
            "pair": lambda: ctx.call("fisdf_pair_density", L.ptr(f[0]), L.ptr(f[-1]), ngrid, nao,
                                     0, nao, L.ptr(rows)),
            "fft_w": lambda: ctx.call("fisdf_fft3d_ex", L.ptr(rows), ngrid, None, L.ptr(rows),
                                      ngrid, nao * nao, msp, kdp, L.ptr(w), None, None, None, 0,
                                      None),
            "fft": lambda: ctx.call("fisdf_fft3d_ex", L.ptr(rows), ngrid, None, L.ptr(rows), ngrid,
                                    nao * nao, msp, None, None, None, None, None, 0, None),
            "block": lambda: ctx.call("fisdf_get_k_fft", L.ptr(f), ngrid * nao, k1p, msp, ap_, nao,
                                      L.ptr(D), nset, 0.0, None, None, 0, 0, L.ptr(out)),
            "call": lambda: ctx.call("fisdf_get_k_fft", L.ptr(f), ngrid * nao, kmp, msp, ap_, nao,
                                     L.ptr(D), nset, 0.0, None, None, 0, 0, L.ptr(out)),
        }
        res = {"nk": nk, "ngrid": ngrid, "nao": nao, "nset": nset, "block_bytes": block_bytes,
               "model_TBps": MODEL_TBPS}
        # d_vk_k1 is (nset, nao, nao) contiguous
        o1 = torch.zeros(nset, nao, nao, dtype=torch.complex128, device="cuda")
        stages["contract"] = lambda: ctx.call("fisdf_exx_contract", L.ptr(rows), L.ptr(u),
                                              L.ptr(f[0]), msp, kdp, 0, nao, nao, nset, 1.0,
                                              L.ptr(o1))
        order = ["pair", "fft_w", "fft", "contract", "block", "call"]
        for name in order:
            call = stages[name]
            if args.only and name != args.only:
                continue
            # the whole call is nk^2 blocks: --call-reps of it after one warm-up call
            reps = args.call_reps if name == "call" else args.reps
            res[name + "_reps"] = reps
            for _ in range(args.warmup if name != "call" else 1):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            ms_call = e0.elapsed_time(e1) / reps
            res[name + "_ms"] = round(ms_call, 4)
            passes = PASSES["block"] * nk * nk if name == "call" else PASSES[name]
            model_ms = passes * block_bytes / (MODEL_TBPS * 1e12) * 1e3
            res[name + "_model_bytes"] = passes * block_bytes
            res[name + "_model_ms"] = round(model_ms, 4)
            res[name + "_x_model"] = round(ms_call / model_ms, 2)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
