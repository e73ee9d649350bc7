"""Bits of the Coulomb fit for an A/B of two library builds: every run of fit_cases.all_runs()
(ranks, lanes, ring, the twelve report integers per q, sha256 of the W_q bytes), then the composite
build on the small toy cell, 1-GPU and 2-rank sharded (sha256 of W_q, W_s, X).
  FISDF_LIB_VARIANT=base python tools/fit_bits.py OUT.txt"""
import hashlib
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fft-isdf-scratch_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
for var in ("FISDF_WPP_KSPLIT", "FISDF_LANE_WPP", "FISDF_FIT_LANES", "FISDF_FIT_PIPE",
            "FISDF_PIPE_DEPTH", "FISDF_HALF_G", "FISDF_FFT_HERM", "FISDF_PIVOTED_FIT"):
    os.environ.pop(var, None)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def sha(x):
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def fit_runs(out):
    import fit_cases as T
    import test_gpu_fit as G
    from fisdf import _lib
    ctx = _lib.Context(0, torch.cuda.current_stream().cuda_stream)
    env = (torch, _lib, ctx)
    runs = [(r, None) for r in T.wq_runs() + T.invariance_runs() + T.rank_runs() + T.y_runs()]
    runs += T.split_runs()
    for run, ks in runs:
        if ks is None:
            os.environ.pop("FISDF_WPP_KSPLIT", None)
        else:
            os.environ["FISDF_WPP_KSPLIT"] = str(ks)
        try:
            f = G.Fit(env, run)
            rc, W, _ = f.fit()
            lanes, depth, slots = f.info()
            reps = [tuple(r) for r in f.reports(f.nq)]
            out.write(f"{tuple(run)} ksplit_env={ks} rc={rc} ranks={tuple(int(r) for r in f.ranks)} "
                      f"lanes={lanes} ring={depth} slots={slots} reports={reps} W={sha(W)}\n")
        finally:
            G._defaults(ctx)
        out.flush()
    os.environ.pop("FISDF_WPP_KSPLIT", None)
    ctx.close()


def composite(out):
    import test_gpu_shard_full as S
    from fisdf import ISDF, kshard
    from fisdf import cell as C
    cell = C.toy_cell(mesh=(12, 12, 12))
    kmesh, m0, c0 = (2, 2, 2), (9, 9, 9), 40.0
    x0 = C.eval_ao_kpts(cell, cell.gen_uniform_grids(m0), kmesh)
    chi = C.eval_ao_kpts(cell, cell.gen_uniform_grids(cell.mesh), kmesh)
    dm = C.make_dm(cell.nao_nr(), kmesh, cell, seed=1234)
    df1, vj1, vk1 = S._one_gpu(cell, kmesh, m0, c0, x0, chi, dm, "lstsq")
    ws1 = df1._dev_state["Ws"]
    out.write(f"composite 1-GPU nip={df1.nip} ranks={[int(r) for r in df1.ranks]} "
              f"Wq={sha(df1._wq)} Ws={sha(ws1)} X={sha(df1._dev_state['X'])} "
              f"vj={sha(vj1)} vk={sha(vk1)}\n")
    yall, fit_qs, partner = S._full_y(df1)
    n = 2
    real_q = np.array([partner[q] == q for q in fit_qs])
    chunks = kshard.assign_q(np.where(real_q, 0.6, 1.0), n)
    slices = kshard.grid_slices(cell.mesh, n)
    for R in range(n):
        grp = kshard.EmulatedGroup(R, n, kshard.emulated_pieces(yall, chunks, slices, R),
                                   w0=df1._dev_state["W0"], ws_src=ws1, keep_ws=True)
        df = ISDF(cell, cell.get_kpts(kmesh), m0=list(m0), c0=c0, comm=grp)
        df.fit = "lstsq"
        df._kmesh()
        df._ao_parent, df._ao_grid = df1._ao_parent, df1._ao_grid
        df.build()
        vj, vk = df.get_jk(dm)
        out.write(f"composite sharded rank {R}/{n} q={[int(q) for q in df.my_qs]} "
                  f"Wq={sha(df._dev_state['Wq'])} Ws_blocks={sha(grp.ws_blocks)} "
                  f"X={sha(df._dev_state['X'])} vj={sha(vj)} vk={sha(vk)}\n")
        del df, grp
    torch.cuda.synchronize()


if __name__ == "__main__":
    path = sys.argv[1]
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as out:
        fit_runs(out)
        try:
            composite(out)
        except Exception:
            out.write("composite FAILED\n" + traceback.format_exc())
            raise
