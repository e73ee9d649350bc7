#!/usr/bin/env python
"""Times the stages of the exact FFT-grid four-index integrals (ISDF.eri_method = "fft") for one
(k1, k2) of C3 shape (FFT mesh 36^3, nao 26, all rows i in one chunk) on synthetic device arrays:
the B builder fisdf_pair34, the two fft3d calls over the row block, the (R, T) GEMM of the block
against B with the plan's split-K, and the whole fisdf_get_eri_fft at npair 1 and 8.  Needs a GPU
(no fallback).

Beside every time stands a model.  Traffic, as DESIGN 3.10 counts it for the exact K: passes over
the row block's n1 n2 ngrid 16 bytes — pair 1, each two-pass FFT 4, conjugation 2, the GEMM's read
1: 12 in all — plus B (npair n3 n4 ngrid 16 bytes) written once and read once by the GEMM, at the
5.3 TB/s of the FFT.  The GEMM is also given as a rate, 8 n1n2 n3n4 ngrid flop per
pair, beside the same product as an (N, C) GEMM, the shape tools/gemm_bench.py --herk-shapes times.
First measurements: no threshold.  One JSON line per npair.

  python tools/eri_bench.py [--mesh 36 36 36] [--nao 26] [--npairs 1 8] [--reps 10] [--warmup 2]
                            [--only pair34|fft_w|fft|gemm|gemm_nc|call] [--work-bytes W]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fft-isdf-scratch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

MODEL_TBPS = 5.3
STAGES = ["pair34", "fft_w", "fft", "gemm", "gemm_nc", "call"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, nargs=3, default=[36, 36, 36])
    ap.add_argument("--nao", type=int, default=26)
    ap.add_argument("--npairs", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=STAGES, default=None)
    ap.add_argument("--work-bytes", type=int, default=0,
                    help="fisdf_get_eri_fft's budget (0: the library's default)")
    args = ap.parse_args()

    import torch
    from fisdf import _lib as L
    if not torch.cuda.is_available():
        raise SystemExit("eri_bench: no GPU visible")
    ctx = L.Context(0, torch.cuda.current_stream().cuda_stream)
    ngrid, nao = int(np.prod(args.mesh)), args.nao
    nn = nao * nao
    a = np.diag([10.26, 10.26, 10.26]).astype(float)
    ms, msp = L.iarr(args.mesh)
    aa, ap_ = L.darr(a.ravel())
    kd, kdp = L.darr([0.83, -1.91, 2.6])
    q, qp = L.darr(np.linalg.solve(a, kd))
    one, zero = (C.c_double * 2)(1.0, 0.0), (C.c_double * 2)(0.0, 0.0)
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*shape):
        return torch.randn(*shape, dtype=torch.complex128, device="cuda", generator=gen)

    a1, a2 = rnd(ngrid, nao), rnd(ngrid, nao)
    rows = rnd(nn, ngrid)
    w = torch.rand(ngrid, dtype=torch.float64, device="cuda", generator=gen)
    block_bytes = rows.numel() * 16
    for npair in args.npairs:
        a3 = [rnd(ngrid, nao) for _ in range(npair)]
        a4 = [rnd(ngrid, nao) for _ in range(npair)]
        p3 = (L._vp * npair)(*[t.data_ptr() for t in a3])
        p4 = (L._vp * npair)(*[t.data_ptr() for t in a4])
        B = torch.empty(npair * nn, ngrid, dtype=torch.complex128, device="cuda")
        out = torch.empty(npair, nn, nn, dtype=torch.complex128, device="cuda")
        v = [C.c_int() for _ in range(7)]
        nbytes = C.c_long()
        assert ctx.lib.fisdf_eri_fft_plan(nao, nao, nao, nao, npair, ngrid, args.work_bytes,
                                          *[C.byref(x) for x in v], C.byref(nbytes)) == 0
        mc, nrc, bc, nbc, b_once, tw, ks = (x.value for x in v)
        b_bytes = B.numel() * 16

        def gemm(opb):
            # one GEMM per pair, as the driver runs them; (N, C) reads B as it lies too
            for p in range(npair):
                ctx.call("fisdf_zgemm", 2 if opb == 1 else 0, opb, nn, nn, ngrid, one, L.ptr(rows),
                         ngrid, 0, L.ptr(B[p * nn:]), ngrid, 0, zero, L.ptr(out[p]), nn, 0, 1, ks)

        stages = {
            "pair34": lambda: ctx.call("fisdf_pair34", p3, p4, npair, nao, nao, nao, nao, msp, kdp,
                                       0, npair * nao, L.ptr(B)),
            "fft_w": lambda: ctx.call("fisdf_fft3d_ex", L.ptr(rows), ngrid, None, L.ptr(rows),
                                      ngrid, nn, msp, kdp, L.ptr(w), None, None, None, 0, None),
            "fft": lambda: ctx.call("fisdf_fft3d_ex", L.ptr(rows), ngrid, None, L.ptr(rows), ngrid,
                                    nn, msp, None, None, None, None, None, 0, None),
            "gemm": lambda: gemm(1),
            "gemm_nc": lambda: gemm(3),
            "call": lambda: ctx.call("fisdf_get_eri_fft", msp, ap_, qp, 0.0, L.ptr(a1), nao,
                                     L.ptr(a2), nao, p3, p4, npair, nao, nao, args.work_bytes,
                                     L.ptr(out)),
        }
        model_bytes = {"pair34": b_bytes, "fft_w": 4 * block_bytes, "fft": 4 * block_bytes,
                       "gemm": block_bytes + b_bytes, "gemm_nc": block_bytes + b_bytes,
                       "call": 12 * block_bytes + 2 * b_bytes}
        res = {"ngrid": ngrid, "nao": nao, "npair": npair, "block_bytes": block_bytes,
               "b_bytes": b_bytes, "model_TBps": MODEL_TBPS, "mc": mc, "bc": bc, "b_once": b_once,
               "tw": tw, "ksplit": ks, "arena_bytes": nbytes.value, "work_bytes": args.work_bytes}
        for name in STAGES:
            if args.only and name != args.only:
                continue
            call = stages[name]
            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            ms_call = e0.elapsed_time(e1) / args.reps
            model_ms = model_bytes[name] / (MODEL_TBPS * 1e12) * 1e3
            res[name + "_ms"] = round(ms_call, 4)
            res[name + "_model_ms"] = round(model_ms, 4)
            res[name + "_x_model"] = round(ms_call / model_ms, 2)
            if name in ("gemm", "gemm_nc", "call"):
                res[name + "_gemm_TFps"] = round(8.0 * nn * nn * ngrid * npair / ms_call / 1e9, 2)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
