#!/usr/bin/env python
"""Times the GGA layer at the C3 shape (nk 64 = 4x4x4, FFT mesh 36^3, nao 26) one grid block at a
time, as ISDF.get_rho(xctype="GGA") / nr_vxc_mat / get_kin walk the grid: the evaluator of the AO
values with first derivatives (fisdf_eval_ao_deriv1 on the diamond cell's tables), the density
with its gradient (fisdf_get_rho_gga, hermi 1 and 0, 1..4 sets) and the potential matrix
(fisdf_gga_gram) on synthetic device arrays — and beside them, in the same run and on the same
block of points, the yardsticks fisdf_eval_ao, fisdf_get_rho and fisdf_weighted_gram.  Needs a GPU
(no fallback).

Per stage: `--warmup` calls, then `--windows` windows of back-to-back calls between two device
events, each window long enough for about `--window-ms` of work; the mean per call of every window
is kept (their spread is the noise).  One JSON line: the times per block, the block size the
default deriv_work_bytes gives, the blocks of the grid, and the structural counts (bytes of AO
read, fused multiply-adds) the times are to be held against.

  python tools/xc_bench.py [--windows 3] [--window-ms 300] [--warmup 2] [--only STAGE]
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

KMESH, MESH = (4, 4, 4), (36, 36, 36)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()

    import torch
    from fisdf import ISDF, _lib as L, cell as C
    from fisdf.ao import eval_ao_kpts_gpu
    if not torch.cuda.is_available():
        raise SystemExit("xc_bench: no GPU visible")

    cell = C.diamond_cell(mesh=MESH)
    df = ISDF(cell, cell.get_kpts(KMESH))
    df._kmesh()
    d = df.device
    ctx = d.ctx
    nk, ngrid, nao = int(np.prod(KMESH)), int(np.prod(MESH)), cell.nao_nr()
    nb = min(df.deriv_block_points(), ngrid)
    nblocks = -(-ngrid // nb)
    coords = df.grids_coords()
    tn = C.lattice_translations(cell, coords)
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*shape):
        return torch.randn(*shape, dtype=torch.complex128, device="cuda", generator=gen)

    f4 = rnd(nk, 4, nb, nao)
    dms = rnd(4, nk, nao, nao)
    dms = dms + dms.conj().transpose(-1, -2)
    rho4, rho = rnd(4, 4, nb), rnd(4, nb)
    w4 = torch.randn(4, 4, nb, dtype=torch.float64, device="cuda", generator=gen)
    v = rnd(4, nb)
    out = rnd(4, nk, nao, nao)
    ks, cs = 4 * nb * nao, nb * nao
    vol = cell.vol

    stages = {
        "eval_ao_deriv1": lambda: eval_ao_kpts_gpu(d, cell, coords[:nb], KMESH, deriv=1, tn=tn),
        "eval_ao": lambda: eval_ao_kpts_gpu(d, cell, coords[:nb], KMESH, tn=tn),
    }
    for hermi in (1, 0):
        for nset in (1, 2, 3, 4):
            stages[f"get_rho_gga_h{hermi}_s{nset}"] = (
                lambda hermi=hermi, nset=nset: ctx.call(
                    "fisdf_get_rho_gga", L.ptr(f4), ks, cs, nk, nb, nao, L.ptr(dms), nset, hermi,
                    L.ptr(rho4), nb))
    for nset in (1, 2, 3, 4):
        # the yardstick on the same points: component 0 of every k-point, k stride ks
        stages[f"get_rho_s{nset}"] = (lambda nset=nset: ctx.call(
            "fisdf_get_rho", L.ptr(f4), ks, nk, nb, nao, L.ptr(dms), nset, L.ptr(rho)))
    for nset in (1, 4):
        stages[f"gga_gram_s{nset}"] = (lambda nset=nset: ctx.call(
            "fisdf_gga_gram", L.ptr(f4), ks, cs, nk, nb, nao, L.ptr(w4), 4 * nb, nb, nset,
            vol / ngrid, 1, L.ptr(out)))
        stages[f"weighted_gram_s{nset}"] = (lambda nset=nset: ctx.call(
            "fisdf_weighted_gram", L.ptr(f4), ks, nk, nb, nao, L.ptr(v), nset, 0, vol / ngrid,
            L.ptr(out)))

    def window(call, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    res = {"shape": "c3", "nk": nk, "ngrid": ngrid, "nao": nao, "block_points": nb,
           "blocks": nblocks, "deriv_work_bytes": int(df.deriv_work_bytes),
           # per block: bytes of AO the kernels read, fused multiply-adds (complex = 4) a set
           "ao_bytes_values": 16 * nk * nb * nao, "ao_bytes_deriv1": 64 * nk * nb * nao,
           "fma_get_rho": 4 * nk * nb * (nao * nao + nao),
           "fma_get_rho_gga_h1": 4 * nk * nb * (nao * nao + nao) + 2 * 3 * nk * nb * nao,
           "ms": {}}
    for st, call in stages.items():
        if args.only and st != args.only:
            continue
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        once = window(call, 2)
        reps = int(max(3, min(2000, args.window_ms / max(once, 1e-3))))
        res["ms"][st] = [round(window(call, reps), 4) for _ in range(args.windows)]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
