#!/usr/bin/env python
"""Times the fused RKS block and the whole ISDF.nr_rks step at the C3 shape (nk 64 = 4x4x4, FFT
mesh 36^3, nao 26).  Needs a GPU (no fallback).

Per block (the block of the default deriv_work_bytes, synthetic device arrays, 1 and 4 sets):
fisdf_nr_rks_block against its three stages called separately (fisdf_get_rho_gga hermi 1,
fisdf_xc_eval, fisdf_gga_gram), and fisdf_xc_eval alone.  `--warmup` calls, then `--windows`
windows of back-to-back calls between two device events, each about `--window-ms` long; the mean
per call of every window is kept (their spread is the noise).

Per whole grid (the diamond cell, one density matrix, host wall clock around calls that end with
their results on the host): ISDF.nr_rks("pbe") against the route through the host that needs no
device functional — get_rho(xctype="GGA"), a stand-in for the functional that costs nothing
(wv = rho), nr_vxc_mat — `--steps` alternated pairs.

One JSON line.  Nothing here is a pass mark.

  python tools/nr_rks_bench.py [--windows 3] [--window-ms 300] [--warmup 2] [--steps 3]
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()

    import torch
    from fisdf import ISDF, _lib as L, cell as C, xc
    if not torch.cuda.is_available():
        raise SystemExit("nr_rks_bench: no GPU visible")

    cell = C.diamond_cell(mesh=MESH)
    df = ISDF(cell, cell.get_kpts(KMESH))
    df._kmesh()
    d = df.device
    ctx = d.ctx
    nk, ngrid, nao = int(np.prod(KMESH)), int(np.prod(MESH)), cell.nao_nr()
    nb = min(df.deriv_block_points(), ngrid)
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*shape):
        return torch.randn(*shape, dtype=torch.complex128, device="cuda", generator=gen)

    f4 = rnd(nk, 4, nb, nao)
    # B B^H + 1: the density of the synthetic block is positive at every point
    B = rnd(4, nk, nao, nao)
    dms = (B @ B.conj().transpose(-1, -2) / nao + torch.eye(nao, device="cuda")).contiguous()
    rho4 = torch.empty(4, 4, nb, dtype=torch.complex128, device="cuda")
    w4 = torch.empty(4, 4, nb, dtype=torch.float64, device="cuda")
    e = torch.empty(4, nb, dtype=torch.float64, device="cuda")
    out = torch.zeros(4, nk, nao, nao, dtype=torch.complex128, device="cuda")
    sums = torch.zeros(4, 2, dtype=torch.float64, device="cuda")
    ks, cs = 4 * nb * nao, nb * nao
    scale, cut = cell.vol / ngrid, float(df.xc_rho_cut)

    def rho_stage(nset):
        ctx.call("fisdf_get_rho_gga", L.ptr(f4), ks, cs, nk, nb, nao, L.ptr(dms), nset, 1,
                 L.ptr(rho4), nb)

    def xc_stage(nset):
        ctx.call("fisdf_xc_eval", xc.GGA, 1.0, 1.0, cut, L.ptr(rho4), 4 * nb, nb, nb, nset,
                 L.ptr(e), nb, L.ptr(w4), 4 * nb, nb)

    def gram_stage(nset):
        ctx.call("fisdf_gga_gram", L.ptr(f4), ks, cs, nk, nb, nao, L.ptr(w4), 4 * nb, nb, nset,
                 scale, 0, L.ptr(out))

    def three(nset):
        rho_stage(nset)
        xc_stage(nset)
        gram_stage(nset)

    def fused(nset):
        ctx.call("fisdf_nr_rks_block", xc.GGA, 1.0, 1.0, cut, L.ptr(f4), ks, cs, nk, nb, nao,
                 L.ptr(dms), nset, scale, 0, L.ptr(out), L.ptr(sums))

    stages = {}
    for nset in (1, 4):
        stages[f"nr_rks_block_s{nset}"] = lambda nset=nset: fused(nset)
        stages[f"three_entries_s{nset}"] = lambda nset=nset: three(nset)
        stages[f"get_rho_gga_s{nset}"] = lambda nset=nset: rho_stage(nset)
        stages[f"xc_eval_s{nset}"] = lambda nset=nset: xc_stage(nset)
        stages[f"gga_gram_s{nset}"] = lambda nset=nset: gram_stage(nset)

    def window(call, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    res = {"shape": "c3", "nk": nk, "ngrid": ngrid, "nao": nao, "block_points": nb,
           "nr_rks_block_points": {s: df.nr_rks_block_points(s) for s in (1, 4)},
           "deriv_work_bytes": int(df.deriv_work_bytes), "ms": {}}
    for st, call in stages.items():
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        once = window(call, 2)
        reps = int(max(3, min(2000, args.window_ms / max(once, 1e-3))))
        res["ms"][st] = [round(window(call, reps), 4) for _ in range(args.windows)]

    # the whole grid, host wall clock
    rng = np.random.default_rng(3)
    D = rng.standard_normal((nk, nao, nao)) + 1j * rng.standard_normal((nk, nao, nao))
    D = 0.05 * (D + D.conj().swapaxes(-1, -2)) + np.eye(nao)

    def fused_step():
        return df.nr_rks("pbe", D)

    def host_step():
        rho = df.get_rho(D, xctype="GGA")
        return df.nr_vxc_mat(rho)           # the functional's stand-in: wv = rho

    def wall(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3, 3)

    for _ in range(max(1, args.warmup)):
        nelec = fused_step()[0]
        host_step()
    res["whole_grid_nelec"] = nelec
    res["whole_grid_ms"] = {"nr_rks_pbe": [], "get_rho_gga_plus_nr_vxc_mat": []}
    for _ in range(args.steps):
        res["whole_grid_ms"]["nr_rks_pbe"].append(wall(fused_step))
        res["whole_grid_ms"]["get_rho_gga_plus_nr_vxc_mat"].append(wall(host_step))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
