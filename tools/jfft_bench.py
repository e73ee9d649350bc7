#!/usr/bin/env python
"""Times the three stages of the exact FFT-grid J (fisdf_get_rho, fisdf_coulomb_potential,
fisdf_weighted_gram) and the composite fisdf_get_j_fft at C3 shapes (nk 64, FFT mesh 36^3, nao 26,
nset 1 and 2) on synthetic device arrays, and beside them the ISDF J (fisdf_get_j at --isdf-nip
interpolation points), so the price of exactness is on the same line.  Needs a GPU (no fallback).

Per stage: device events around `--reps` back-to-back calls after `--warmup` calls, the mean per
call, and for the two AO kernels the algorithmic traffic (the AO array once) over that time.
One JSON line per nset.

  python tools/jfft_bench.py [--nk 4 4 4] [--mesh 36 36 36] [--nao 26] [--nsets 1 2]
                             [--reps 100] [--warmup 3] [--only rho|potential|gram|j|isdf_j]
                             [--isdf-nip 600]

--only runs a single stage (for a counters-only profiler run around one kernel).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nk", type=int, nargs=3, default=[4, 4, 4])
    ap.add_argument("--mesh", type=int, nargs=3, default=[36, 36, 36])
    ap.add_argument("--nao", type=int, default=26)
    ap.add_argument("--nsets", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--isdf-nip", type=int, default=600,
                    help="interpolation points of the ISDF J timed beside it (fisdf_get_j; 0: skip)")
    ap.add_argument("--only", choices=["rho", "potential", "gram", "j", "isdf_j"], default=None)
    args = ap.parse_args()

    import torch
    from fisdf import _lib as L
    if not torch.cuda.is_available():
        raise SystemExit("jfft_bench: no GPU visible")
    ctx = L.Context(0, torch.cuda.current_stream().cuda_stream)
    nk, ngrid, nao = int(np.prod(args.nk)), int(np.prod(args.mesh)), args.nao
    a = np.diag([10.26, 10.26, 10.26]).astype(float)
    km, kmp = L.iarr(args.nk)
    ms, msp = L.iarr(args.mesh)
    aa, ap_ = L.darr(a.ravel())
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*shape):
        return torch.randn(*shape, dtype=torch.complex128, device="cuda", generator=gen)

    f = rnd(nk, ngrid, nao)
    ao_bytes = f.numel() * 16
    for nset in args.nsets:
        D = rnd(nset, nk, nao, nao)
        D = D + D.conj().transpose(-1, -2)
        rho, v = rnd(nset, ngrid), rnd(nset, ngrid)
        out = torch.empty_like(D)
        stages = {
            "rho": lambda: ctx.call("fisdf_get_rho", L.ptr(f), ngrid * nao, nk, ngrid, nao,
                                    L.ptr(D), nset, L.ptr(rho)),
            "potential": lambda: ctx.call("fisdf_coulomb_potential", L.ptr(rho), nset, msp, ap_,
                                          0.0, L.ptr(v)),
            "gram": lambda: ctx.call("fisdf_weighted_gram", L.ptr(f), ngrid * nao, nk, ngrid, nao,
                                     L.ptr(v), nset, 0, a[0, 0] ** 3 / ngrid, L.ptr(out)),
            "j": lambda: ctx.call("fisdf_get_j_fft", L.ptr(f), ngrid * nao, kmp, msp, ap_, nao,
                                  L.ptr(D), nset, 0.0, None, 0, L.ptr(out)),
        }
        if args.isdf_nip > 0:       # the fit's J on synthetic X, W_0: what j_method = "isdf" runs
            nip = args.isdf_nip
            X, W0 = rnd(nk, nip, nao), rnd(nip, nip)
            stages["isdf_j"] = lambda: ctx.call("fisdf_get_j", L.ptr(X), L.ptr(W0), L.ptr(D), nset,
                                                nk, nip, nao, L.ptr(out))
        res = {"nk": nk, "ngrid": ngrid, "nao": nao, "nset": nset, "reps": args.reps,
               "ao_bytes": ao_bytes}
        for name, call in stages.items():
            if args.only and name != args.only:
                continue
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
            res[name + "_ms"] = round(ms_call, 4)
            if name in ("rho", "gram"):
                res[name + "_ao_TBps"] = round(ao_bytes / (ms_call * 1e-3) / 1e12, 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
