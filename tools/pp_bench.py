#!/usr/bin/env python
"""Times the stages of the GTH pseudopotential matrices (fisdf_vloc_g, fisdf_gth_projectors, the
projector rows' fisdf_fft3d, fisdf_pp_overlap, fisdf_weighted_gram) and the composite fisdf_get_pp
with and without the non-local part, on synthetic device arrays.  Needs a GPU (no fallback).

Two shapes: "c3" (nk 64, FFT mesh 36^3, nao 26, 2 atoms of 1 projector each) and "nio" (nk 1, mesh
32^3, nao 76, 2 atoms of 13 projectors and 2 of 1).  The per-stage times are for one k-point; the
composites take all nk.  Per stage: device events around `--reps` back-to-back calls after
`--warmup` calls, the mean per call.  One JSON line per shape.

  python tools/pp_bench.py [--shapes c3 nio] [--reps 50] [--warmup 3] [--only STAGE]
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

# entries in PySCF's _pseudo format with the projector counts of GTH-PADE C (1 row), O (1 row) and
# Ni (s 2, p 2, d 1: 13 rows); the numbers are placeholders of the right size
PSEUDO = {
    "C": [[2, 2], 0.35, 2, [-8.5, 1.23], 1, [0.30, 1, [[9.5]]]],
    "O": [[2, 4], 0.25, 2, [-16.6, 2.4], 1, [0.22, 1, [[18.3]]]],
    "Ni": [[4, 6, 8], 0.35, 2, [2.1, 0.65], 3,
           [0.25, 2, [[12.2, -9.0], [-9.0, 11.6]]],
           [0.23, 2, [[-11.6, 12.4], [12.4, -14.8]]],
           [0.22, 1, [[-12.6]]]],
}
SHAPES = {
    "c3": dict(nk=(4, 4, 4), mesh=(36, 36, 36), nao=26, symbols=("C", "C"), a=6.74),
    "nio": dict(nk=(1, 1, 1), mesh=(32, 32, 32), nao=76, symbols=("Ni", "Ni", "O", "O"), a=7.88),
}


class _Atoms:
    """The protocol fisdf.pp.pack_atoms reads."""

    def __init__(self, symbols, a):
        self.symbols, self._pseudo, self.natm = symbols, PSEUDO, len(symbols)
        rng = np.random.default_rng(3)
        self._xyz = rng.uniform(0, 1, (self.natm, 3)) @ a

    def atom_coords(self):
        return self._xyz

    def atom_charges(self):
        return np.array([sum(PSEUDO[s][0]) for s in self.symbols])

    def atom_symbol(self, ia):
        return self.symbols[ia]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["c3", "nio"], choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()

    import torch
    from fisdf import _lib as L
    from fisdf.pp import pack_atoms
    if not torch.cuda.is_available():
        raise SystemExit("pp_bench: no GPU visible")
    ctx = L.Context(0, torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*shape):
        return torch.randn(*shape, dtype=torch.complex128, device="cuda", generator=gen)

    for name in args.shapes:
        s = SHAPES[name]
        nk, ngrid, nao = int(np.prod(s["nk"])), int(np.prod(s["mesh"])), s["nao"]
        a = (np.ones((3, 3)) - np.eye(3)) * s["a"] / 2
        b = 2 * np.pi * np.linalg.inv(a).T
        kfrac = np.stack(np.meshgrid(*[np.arange(n) / n for n in s["nk"]], indexing="ij"),
                         -1).reshape(-1, 3)
        kpts = kfrac @ b
        tab = pack_atoms(_Atoms(s["symbols"], a))
        natm = len(tab)
        nproj = ctx.lib.fisdf_pp_nproj(tab, natm)
        ms, msp = L.iarr(s["mesh"])
        aa, ap_ = L.darr(a.ravel())
        kc, kp = L.darr(kpts.ravel())
        k1c, k1p = L.darr(kpts[-1])
        kdc, kdp = L.darr(a @ kpts[-1])
        f = rnd(nk, ngrid, nao)
        vg, v = rnd(ngrid), rnd(1, ngrid)
        rows = rnd(nproj, ngrid)
        c = rnd(nproj, nao)
        out = rnd(nk, nao, nao)
        vol = abs(np.linalg.det(a))
        stages = {
            "vloc_g": lambda: ctx.call("fisdf_vloc_g", msp, ap_, tab, natm, L.ptr(vg)),
            "projectors": lambda: ctx.call("fisdf_gth_projectors", msp, ap_, k1p, tab, natm, 0,
                                           natm, L.ptr(rows)),
            "rows_fft": lambda: ctx.call("fisdf_fft3d", L.ptr(rows), L.ptr(rows), nproj, msp),
            "overlap": lambda: ctx.call("fisdf_pp_overlap", L.ptr(rows), nproj, L.ptr(f[-1]), nao,
                                        msp, kdp, 1.0 / ngrid, L.ptr(c)),
            "gram": lambda: ctx.call("fisdf_weighted_gram", L.ptr(f), ngrid * nao, nk, ngrid, nao,
                                     L.ptr(v), 1, 0, vol / ngrid, L.ptr(out)),
            "get_nuc": lambda: ctx.call("fisdf_get_pp", L.ptr(f), ngrid * nao, nk, kp, msp, ap_,
                                        nao, tab, natm, 0, 0, L.ptr(out)),
            "get_pp": lambda: ctx.call("fisdf_get_pp", L.ptr(f), ngrid * nao, nk, kp, msp, ap_,
                                       nao, tab, natm, 1, 0, L.ptr(out)),
        }
        res = {"shape": name, "nk": nk, "ngrid": ngrid, "nao": nao, "natm": natm, "nproj": nproj,
               "reps": args.reps}
        for st, call in stages.items():
            if args.only and st != args.only:
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
            res[st + "_ms"] = round(e0.elapsed_time(e1) / args.reps, 4)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
