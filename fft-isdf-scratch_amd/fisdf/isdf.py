"""PySCF-style ISDF density-fitting object on MI355X (mirror of fftisdf.py).

Drop-in for ``InterpolativeSeparableDensityFitting`` / ``ISDF`` of the reference
(/root/reference/fftisdf.py:296-410): same constructor, attributes (``c0``, ``m0``,
``blksize``, ``_x``, ``_w0``, ``_wq``), ``build()``, ``aoR_loop()``,
``select_interpolation_points()``, ``get_jk()`` and the module functions ``build``,
``get_j_kpts`` and ``get_k_kpts`` — with every numerical stage executed by the HIP
kernels of libfisdf.so (no CPU fallback: missing library or GPU raises).

Differences from the reference, all deliberate:
* the zgelsy fit (fftisdf.py:108) is replaced by a pivoted-Cholesky factorisation of
  x4_q applied in factored order (tolerance ``fit_tol``); J/K agree with
  the gelsy oracle to < 1e-8 but W_q differs in the null space of x4_q;
* ``y`` stays resident in HBM (no HDF5 scratch, fftisdf.py:60-63);
* the bug of fftisdf.py:322 (global ``cell``) is not reproduced;
* optional k-point sharding over ranks of a torch.distributed group (``comm``).
"""
from __future__ import annotations

import logging
import os
import time

import numpy as np

from . import _lib, kshard
from . import xc as _xc
from .cell import bloch_ao, madelung, make_kpts

log = logging.getLogger("fisdf")


def _torch():
    import torch
    return torch


def kpts_to_kmesh(cell, kpts):
    """[pyscf] k2gamma.kpts_to_kmesh: number of distinct scaled coordinates per axis."""
    kpts = np.asarray(kpts, float).reshape(-1, 3)
    scaled = kpts @ cell.lattice_vectors().T / (2 * np.pi)
    kmesh = [len(np.unique(np.round(scaled[:, i], 6))) for i in range(3)]
    return np.asarray(kmesh)


def _format_dms(dm_kpts, nkpts):
    """[pyscf] df_jk._format_dms -> (nset, nk, nao, nao)."""
    dm = np.asarray(dm_kpts)
    nao = dm.shape[-1]
    return dm.reshape(-1, nkpts, nao, nao)


def _format_jks(v, dm_kpts):
    """[pyscf] df_jk._format_jks: result shaped like the input dm."""
    return v.reshape(np.shape(dm_kpts))


class _Device:
    """Per-process device state: torch device, fisdf context, k-point shard."""

    def __init__(self, device=None, comm=None):
        torch = _torch()
        if not torch.cuda.is_available():
            raise _lib.FisdfError("fisdf: no GPU visible (the HIP path has no CPU fallback)")
        if device is None:
            device = torch.cuda.current_device()
        self.torch = torch
        self.dev = torch.device("cuda", int(device))
        self.stream = torch.cuda.current_stream(self.dev)
        self.ctx = _lib.Context(int(device), self.stream.cuda_stream)
        self.comm = comm
        if isinstance(comm, kshard.EmulatedGroup):
            self.rank, self.size = comm.rank, comm.size
        elif comm is not None:
            import torch.distributed as dist
            self.rank = dist.get_rank(comm)
            self.size = dist.get_world_size(comm)
        else:
            self.rank, self.size = 0, 1

    def shard(self, nk):
        """Contiguous q-range of this rank."""
        return kshard.shard_range(nk, self.rank, self.size)

    def sharded(self, df_obj):
        """Whether this build takes the collective (k-sharded) code path."""
        if self.size > 1:
            return True
        if getattr(df_obj, "force_sharded", False):
            if self.comm is None:
                raise ValueError("ISDF.force_sharded needs a torch.distributed group (comm)")
            return True
        return False

    def empty(self, shape, dtype="c128"):
        t = self.torch
        dt = {"c128": t.complex128, "f64": t.float64, "i32": t.int32}[dtype]
        return t.empty(tuple(int(s) for s in shape), dtype=dt, device=self.dev)

    def to_dev(self, arr):
        t = self.torch
        a = np.ascontiguousarray(arr)
        return t.from_numpy(a).to(self.dev, non_blocking=False)

    def to_host(self, x):
        """Read back through pinned memory: the copy is enqueued right behind the kernels that
        produce x and the host then waits for the stream.  A pageable ``.cpu()`` first drains the
        stream and only then stages its copy — about 0.2 ms of idle GPU at the end of every
        get_jk (kernel trace, profiles/r05/prof_v2).  FISDF_PINNED_D2H=0: ``.cpu()``."""
        if os.environ.get("FISDF_PINNED_D2H", "1") == "0":
            return x.cpu().numpy()
        h = self.torch.empty(tuple(x.shape), dtype=x.dtype, pin_memory=True)
        # on the context's stream (the one the library produced x on and the one waited for
        # below), whatever stream the caller has made current
        with self.torch.cuda.stream(self.stream):
            h.copy_(x, non_blocking=True)
        self.stream.synchronize()
        return h.numpy()

    def to_dev_async(self, arr):
        """Upload through pinned memory without a host wait on the stream (small per-call inputs
        such as density matrices: the GPU keeps running the work already enqueued)."""
        t = self.torch
        h = t.from_numpy(np.ascontiguousarray(arr)).pin_memory()
        return h.to(self.dev, non_blocking=True)


class InterpolativeSeparableDensityFitting:
    """ISDF(cell, kpts, m0=None, c0=20.0) — fftisdf.py:296-306."""

    _x = None
    _w0 = None
    _wq = None
    blksize = 8000          # fftisdf.py:300
    fit_tol = 4.2e-15       # relative pivot cut of the x4_q factorisation: where
                            # its ranks reproduce gelsy's at rcond = eps (fftisdf.py:108)
    select_tol = -1.0       # dpstrf default tolerance (ng0*eps*max diag)
    y_streamed = False      # the last 1-GPU build formed y behind the selection
    # cap on the number of interpolation points; None -> int(nao * c0) (fftisdf.py:383);
    # the get_coul drivers set it directly (fftdf-with-k-lstsq.py:71, fftdf-with-k.py:64)
    nip_max = None
    # fit one q of each (q, -q) pair and take W_{-q} = conj(W_q) (y_s, x4_s real: :43,:81)
    time_reversal = True
    # q with 2 k_q in the reciprocal lattice (Gamma, all q of a 2x2x2 mesh): real x4_q and
    # W_q, fitted with real-factor / real-part GEMMs (half the MFMA work)
    real_self_conjugate = True
    # a self-conjugate q fitted over one member of each Hermitian G pair (fisdf_set_half_grid;
    # DESIGN §3.5): None = library default (FISDF_HALF_G, on), True / False force it
    half_grid = None
    # x4_q factorisation: None = library default (unpivoted blocked Cholesky when every x4_q
    # is numerically full rank, else the greedy pivoted one); True forces the pivoted path
    pivoted_fit = None
    # the solution the fit applies (fisdf_set_fit_mode): "lstsq" = scipy lstsq/gelsy semantics
    # (fftisdf.py:108; unique solution of a full-rank x4_q, minimum-norm one of a rank-deficient
    # x4_q), "svd" = the truncated pseudo-solve on every q (fftdf-with-k-svd.py:158-164 intent),
    # "basic" = the rank-revealing factor's basic solution (round-1 path)
    fit = "lstsq"
    # Bloch AO inputs evaluated on the GPU (fisdf_eval_ao) instead of the host restatement
    ao_on_gpu = True
    # multi-rank selection: False (default) replicates the 1-GPU Gram + pivots on every rank
    # (rank-count-invariant pivots); True k-shards the Gram and all-reduces it
    sharded_gram = False
    # run the sharded (collective) code path even in a one-rank group: grid-sliced y, the chunked
    # all-to-all, the W_s all-reduce and W_0 broadcast, the get_jk all-reduces — how the RCCL path
    # is exercised on a single GPU (tests/test_gpu_rccl.py); needs ``comm``
    force_sharded = False
    # where J comes from: "isdf" = the fit's W_0 (the reference, fftisdf.py:133-171); "fft" = the
    # exact FFT-grid J (PySCF fft_jk.get_j_kpts: the density on the FFT grid, one forward and one
    # inverse FFT, one weighted AO Gram over the resident Bloch AOs) — no fitting error, and
    # defined at any band k-point.
    j_method = "isdf"
    J_METHODS = ("isdf", "fft")
    # where K comes from: "isdf" = the fit's W_q (the reference, fftisdf.py:173-228); "fft" = the
    # exact FFT-grid K (PySCF fft_jk.get_k_kpts, the dm form: per (k1, k2) the nao^2 pair densities
    # transformed forth and back with coulG(k2 - k1) and contracted with D and the AOs) — no
    # fitting error, defined at any band k-point, and nk^2 nao^2 pairs of FFTs per call.
    k_method = "isdf"
    K_METHODS = ("isdf", "fft")
    # which form of the exact K (read only when k_method = "fft"): "dm" = all nao^2 pair densities
    # per (k1, k2); "lowrank" = the occupied-orbital form of fft_jk.get_k_kpts, D = A B^H with r
    # columns and nao r pair densities — the factors from the dm's mo_coeff / mo_occ tags
    # (tag_array; trusted, as PySCF trusts them) or else from a host SVD of every D[s][k] that
    # keeps sigma > k_rank_tol sigma_max(set s) (None: nao eps, numpy.linalg.matrix_rank's rule);
    # "auto" = "lowrank" when it has fewer transform rows, sum_k r_k < K_AUTO_ROW_RATIO nk nao.
    # k_form_used: what the last exact K took.
    k_form = "dm"
    K_FORMS = ("dm", "lowrank", "auto")
    k_rank_tol = None
    k_form_used = None
    # where get_eri / ao2mo / get_eri_many come from: "isdf" = the fit's W_q (the reference's ERI
    # loop, fftdf-with-k-lstsq.py:221-232); "fft" = the exact FFT-grid integrals (PySCF
    # FFTDF.get_eri / ao2mo: the pair densities of (k1, k2) transformed forth and back with
    # coulG(k2 - k1), then one GEMM against the pair densities of (k3, k4)) — no fitting error, no
    # build() needed, defined at any k-points that conserve momentum.
    eri_method = "isdf"
    ERI_METHODS = ("isdf", "fft")
    # byte budget of one grid block of the AO values with their first derivatives, (nk, 4, nb, nao)
    # complex plus the evaluator's folded workspace: get_rho(xctype="GGA"), nr_vxc_mat and get_kin
    # walk the FFT grid in blocks of nb points (the four-component array is never resident: 5 GB
    # at nk 64, 36^3, nao 26).  Below one point: ValueError
    deriv_work_bytes = 512 << 20
    XCTYPES = ("LDA", "GGA")
    # eval_xc / nr_rks: a grid point with rho <= xc_rho_cut contributes nothing (e = 0, wv = 0)
    xc_rho_cut = 1e-15

    def __init__(self, cell, kpts, m0=None, c0=20.0, device=None, comm=None):
        self.cell = cell
        self.kpts = np.asarray(kpts, float).reshape(-1, 3)
        self.m0 = m0 if m0 is not None else [15, 15, 15]
        self.c0 = c0
        self.mesh = tuple(cell.mesh)
        self.verbose = getattr(cell, "verbose", 0)
        self.kmesh = None
        self._device_id = device
        self._comm = comm
        self._d = None
        self._ao_grid = None      # device (nk, ngrid, nao) Bloch AOs on the FFT grid (cached)
        self._ao_parent = None    # device (nk, ng0, nao) Bloch AOs on the parent grid (cached)
        self._dev_state = None
        self.timings = {}
        self.nip = None
        self.ranks = None

    # ---- device plumbing --------------------------------------------------
    @property
    def device(self):
        if self._d is None:
            self._d = _Device(self._device_id, self._comm)
        return self._d

    def grids_coords(self):
        return self.cell.gen_uniform_grids(self.mesh)

    def _eval_ao(self, coords):
        """Bloch AOs (nk, ng, nao) at ``coords`` on the device, for the k-mesh of ``build``.

        A cell of ``fisdf.cell`` (explicit ``shells``) is evaluated by the GPU evaluator
        (``ao_on_gpu``, default; fisdf_eval_ao).  Any other cell is asked for its AO values the
        way the reference asks PySCF — ``cell.pbc_eval_gto("GTOval", coords, kpts=self.kpts)``
        (fftisdf.py:367-370; the FFT-grid values of ``aoR_loop``, :327-355, are the same
        function on ``grids.coords``) — block by block on the host (``blksize`` points at a
        time, so host memory stays at one block) and uploaded into one device array."""
        kmesh = self._kmesh()
        if self.ao_on_gpu and hasattr(self.cell, "shells"):
            from .ao import eval_ao_kpts_gpu
            return eval_ao_kpts_gpu(self.device, self.cell, coords, kmesh)
        coords = np.asarray(coords, float)
        ng, nk = coords.shape[0], len(self.kpts)
        out = self.device.empty((nk, ng, self.cell.nao_nr()))
        blk = max(1, int(self.blksize))
        for g0 in range(0, ng, blk):
            g1 = min(g0 + blk, ng)
            out[:, g0:g1] = self.device.to_dev(bloch_ao(self.cell, coords[g0:g1], self.kpts,
                                                        kmesh))
        return out

    def preload_ao(self):
        """Evaluate the AO inputs (PySCF's job in the reference) on the device before build."""
        if self._ao_parent is None:
            self._ao_parent = self._eval_ao(self.cell.gen_uniform_grids(self.m0))
        if self._ao_grid is None:
            self._ao_grid = self._eval_ao(self.grids_coords())
        return self

    def _kmesh(self):
        if self.kmesh is None:
            self.kmesh = kpts_to_kmesh(self.cell, self.kpts)
            self.kpts = make_kpts(self.cell, self.kmesh)        # fftisdf.py:317-322 (self.cell)
        return self.kmesh

    # ---- reference surface ----------------------------------------------
    def build(self):
        """fftisdf.py:308-325."""
        self._kmesh()
        return build(self)

    def aoR_loop(self, grids=None, kpts=None, deriv=0, blksize=None):
        """fftisdf.py:327-355: yields ((ao_k,), g0, g1) over blocks of the FFT grid (host);
        ao_k (nk, nb, nao), or with deriv=1 (nk, 4, nb, nao): the values and their x, y, z
        derivatives (PySCF's eval_ao_kpts(..., deriv=1) layout per k-point)."""
        if deriv not in (0, 1):
            raise ValueError(f"aoR_loop: deriv must be 0 or 1, not {deriv!r}")
        coords = self.grids_coords() if grids is None else np.asarray(getattr(grids, "coords", grids))
        blksize = self.blksize if blksize is None else blksize
        kmesh = self._kmesh()
        for g0 in range(0, coords.shape[0], blksize):
            g1 = min(g0 + blksize, coords.shape[0])
            yield (bloch_ao(self.cell, coords[g0:g1], self.kpts, kmesh, deriv=deriv),), g0, g1

    def select_interpolation_points(self, x0=None, phase=None):
        """fftisdf.py:357-388 on the GPU; returns X = x0[:, perm[:nip], :] as a host array."""
        self._select()
        return self._dev_state["X"].cpu().numpy()

    def _select(self, time_reversal=None):
        d = self.device
        if time_reversal is None:
            time_reversal = self.time_reversal
        kmesh = self._kmesh()
        nk = int(np.prod(kmesh))
        nao = self.cell.nao_nr()
        if self._ao_parent is None:
            self._ao_parent = self._eval_ao(self.cell.gen_uniform_grids(self.m0))
        x0 = self._ao_parent
        ng0 = x0.shape[1]
        cap = int(nao * self.c0) if self.nip_max is None else int(self.nip_max)
        nip_max = min(cap, ng0)
        perm = np.zeros(nip_max, np.int32)
        npiv = C_int()
        full = C_int()
        # time reversal (real AOs): the Gram over the representatives k <= -k only
        d.ctx.call("fisdf_set_time_reversal", 1 if time_reversal else 0)
        km_c, km_p = _lib.iarr(kmesh)
        if d.size == 1:
            d.ctx.call("fisdf_select_points_km", _lib.ptr(x0), km_p, ng0, nao, nip_max,
                       float(self.select_tol), perm.ctypes.data_as(_lib._ip), byref(npiv),
                       byref(full))
        elif self.sharded_gram:
            # k-sharded Gram (fftisdf.py:376-378) + all-reduce: the sum runs in another order
            # than the 1-GPU Gram, so near-tied pivots may differ from the 1-GPU selection
            q0, q1 = d.shard(nk)
            x2 = d.empty((ng0, ng0))
            d.ctx.call("fisdf_select_gram", _lib.ptr(x0), nk, q0, q1, ng0, nao, _lib.ptr(x2))
            kshard.allreduce_real_part(x2, d.comm)  # the Gram is Re(x2) + 0i
            d.ctx.call("fisdf_select_pivots", _lib.ptr(x2), nk, ng0, nip_max,
                       float(self.select_tol), perm.ctypes.data_as(_lib._ip), byref(npiv),
                       byref(full))
            del x2
        else:
            # replicated selection (default): every rank forms the whole Gram in the 1-GPU
            # order (0.4 ms at C3) — the pivots are those of the 1-GPU build on every rank,
            # with no collective
            d.ctx.call("fisdf_select_points_km", _lib.ptr(x0), km_p, ng0, nao, nip_max,
                       float(self.select_tol), perm.ctypes.data_as(_lib._ip), byref(npiv),
                       byref(full))
        nip = min(nip_max, npiv.value)                                  # fftisdf.py:383
        self.perm = perm[:nip].copy()
        X = d.empty((nk, nip, nao))
        d.ctx.call("fisdf_gather_points", _lib.ptr(x0), nk, ng0, nao,
                   self.perm.ctypes.data_as(_lib._ip), nip, _lib.ptr(X))
        log.info("Pivoted Cholesky: nip = %d (rank %s)", nip, "reached" if full.value else ">= nip")
        self._dev_state = dict(X=X)
        self.nip = nip
        return X

    def set_interpolation_points(self, perm):
        """Inject a selection (e.g. the oracle's pivots, SURVEY.md §7 hard part (b))."""
        d = self.device
        kmesh = self._kmesh()
        nk = int(np.prod(kmesh))
        nao = self.cell.nao_nr()
        if self._ao_parent is None:
            self._ao_parent = self._eval_ao(self.cell.gen_uniform_grids(self.m0))
        x0 = self._ao_parent
        self.perm = np.ascontiguousarray(perm, dtype=np.int32)
        nip = len(self.perm)
        X = d.empty((nk, nip, nao))
        d.ctx.call("fisdf_gather_points", _lib.ptr(x0), nk, x0.shape[1], nao,
                   self.perm.ctypes.data_as(_lib._ip), nip, _lib.ptr(X))
        self._dev_state = dict(X=X)
        self.nip = nip

    # ---- checkpoint (the reference keeps _x / _w0 / _wq in memory only) ---------
    _DUMP_VERSION = 1

    def dump(self, path):
        """Save what build() left resident — the interpolation points, X (``_x``), the fitted W_q
        (``_wq`` of the fitted q; the others are their time-reversal partners' conjugates) and
        W_s — to an ``.npz`` of plain arrays (no pickles), so that another process can call
        get_jk / get_eri on the same cell without building again (``load``).  A k-sharded build
        (W_q and the W_s rows distributed over the ranks) is not saved: NotImplementedError."""
        st = self._dev_state
        if st is None or "Ws" not in st:
            raise RuntimeError("ISDF.dump: call build() first")
        if self.device.sharded(self):
            raise NotImplementedError("ISDF.dump of a k-sharded build (W_q are distributed)")
        np.savez(path, version=self._DUMP_VERSION, kmesh=np.asarray(self.kmesh, np.int64),
                 mesh=np.asarray(self.mesh, np.int64),
                 a=np.asarray(self.cell.lattice_vectors(), float), nao=self.cell.nao_nr(),
                 perm=self.perm, fit_qs=self.fit_qs, q_partner=self.q_partner, ranks=self.ranks,
                 X=st["X"].cpu().numpy(), Wq=st["Wq"].cpu().numpy(), Ws=st["Ws"].cpu().numpy(),
                 time_reversal_used=bool(self.time_reversal_used),
                 min_norm_slots=int(self.min_norm_slots),
                 used_pivoted_fit=bool(self.used_pivoted_fit), tr_deviation=self.tr_deviation)

    def load(self, path):
        """Restore a ``dump`` into this object (the same lattice, FFT mesh, k-mesh and AO count,
        checked: ValueError otherwise); afterwards get_jk / get_eri / _x / _w0 / _wq behave as
        after the build that was saved.  Returns self."""
        z = np.load(path)                                     # plain arrays: allow_pickle off
        if int(z["version"]) != self._DUMP_VERSION:
            raise ValueError(f"ISDF.load: dump version {int(z['version'])}")
        kmesh = self._kmesh()
        if (tuple(int(v) for v in z["kmesh"]) != tuple(int(v) for v in kmesh)
                or tuple(int(v) for v in z["mesh"]) != tuple(int(v) for v in self.mesh)
                or int(z["nao"]) != self.cell.nao_nr()
                or not np.allclose(z["a"], np.asarray(self.cell.lattice_vectors(), float),
                                   rtol=0, atol=1e-12)):
            raise ValueError("ISDF.load: the dump is of another cell, FFT mesh or k-mesh")
        if self.device.sharded(self):
            raise NotImplementedError("ISDF.load into a k-sharded object")
        d = self.device
        Wq = d.to_dev(z["Wq"])
        self._dev_state = dict(X=d.to_dev(z["X"]), Wq=Wq, W0=Wq[0], Ws=d.to_dev(z["Ws"]))
        self.perm = np.asarray(z["perm"], np.int32)
        self.fit_qs = np.asarray(z["fit_qs"], np.int32)
        self.my_qs = self.fit_qs.copy()
        self.q_partner = np.asarray(z["q_partner"], np.int32)
        self.ranks = np.asarray(z["ranks"]).copy()
        self.nip = len(self.perm)
        self.time_reversal_used = bool(z["time_reversal_used"])
        self.min_norm_slots = int(z["min_norm_slots"])
        self.used_pivoted_fit = bool(z["used_pivoted_fit"])
        self.tr_deviation = float(z["tr_deviation"])
        return self

    def get_jk(self, dm, hermi=1, kpts=None, kpts_band=None, with_j=True, with_k=True,
               omega=None, exxdiv=None):
        """fftisdf.py:390-408."""
        _check_j_method(self)
        _check_k_method(self)
        if omega is not None and omega != 0:
            # range-separated kernel (PySCF get_coulG omega; the reference raises, :392-393):
            # W_q refitted once per omega with the attenuated weight, X and the AO inputs shared
            if exxdiv is not None:
                raise NotImplementedError("exxdiv with a range-separated kernel")
            if ((self.j_method == "fft" or not with_j)
                    and (self.k_method == "fft" or not with_k)):
                # the grid J and K take omega as an argument: no refit of W_q for them
                return self._get_jk(dm, kpts, kpts_band, with_j, with_k, None, float(omega))
            sub = self._omega_df(float(omega))
            sub.j_method = self.j_method     # the cached sub-object follows the parent's setting
            sub.k_method = self.k_method
            sub.k_form, sub.k_rank_tol = self.k_form, self.k_rank_tol
            out = sub._get_jk(dm, kpts, kpts_band, with_j, with_k, None, float(omega))
            self.k_form_used = sub.k_form_used
            return out
        if exxdiv is not None and exxdiv != "ewald":
            # the reference raises for every exxdiv (:395-396); 'ewald' is added here as
            # PySCF's FFTDF does it: K + madelung * S_k D_k S_k
            raise NotImplementedError
        return self._get_jk(dm, kpts, kpts_band, with_j, with_k, exxdiv,
                            float(getattr(self, "_fit_omega", 0.0)))

    def _get_jk(self, dm, kpts, kpts_band, with_j, with_k, exxdiv, j_omega):
        """get_jk on this object's fitted state; j_omega: the range-separation parameter of the
        grid J and K (j_method / k_method = "fft"), which take it as an argument rather than from
        the fit."""
        kpts = self.kpts if kpts is None else np.asarray(kpts)
        if kpts.ndim == 1:                                            # _check_kpts single kpt
            raise NotImplementedError
        band = _band_of(self, kpts, kpts_band)
        vj = vk = None
        # one upload of the density matrices, K then J enqueued back to back (:404-407), one
        # read-back each at the end: no host round trip between the two
        dms, ddms = _dms_to_dev(self, dm)
        if with_k:
            vk = _get_k_dev(self, ddms, exxdiv, band, j_omega, dm)
        if with_j:
            vj = _get_j_dev(self, ddms, band, j_omega)
        if vk is not None and vj is not None and vk.shape == vj.shape:
            # one device-to-host copy (and one synchronisation) for both
            vk, vj = self.device.to_host(self.device.torch.stack((vk, vj)))
        if vk is not None:
            vk = _format_band(vk if isinstance(vk, np.ndarray) else self.device.to_host(vk), dm,
                              kpts_band, kpts)
        if vj is not None:
            vj = _finish_j(vj, dm, kpts, kpts_band)
        return vj, vk

    def _omega_df(self, omega):
        """The ISDF state for a range-separated kernel (built on first use, cached per omega):
        same interpolation points, W_q / W_s fitted with coulG(omega)."""
        st = self._dev_state
        assert st is not None and "W0" in st, "call build() first"
        cache = self.__dict__.setdefault("_omega_dfs", {})
        if omega not in cache:
            import copy
            sub = copy.copy(self)
            sub._fit_omega = omega
            sub._dev_state = dict(X=st["X"])
            sub._omega_dfs = {}
            sub.timings = {}
            try:
                build(sub)
            finally:
                # the sub-object shares the device context: put its Coulomb kernel back to the
                # parent's, so later direct fisdf_coulg / fit calls do not see erf(w) weights
                self.device.ctx.call("fisdf_set_omega", float(getattr(self, "_fit_omega", 0.0)))
            cache[omega] = sub
        return cache[omega]

    def get_ovlp(self):
        """AO overlap S_k = (vol/ngrid) chi_k^H chi_k (nk, nao, nao) by the FFT-grid quadrature
        (the grid FFTDF's J/K use; PySCF's ``pbc_intor('int1e_ovlp')`` is analytic), one batched
        split-K GEMM over the resident Bloch AOs; cached on the device."""
        st = self._dev_state
        if st is not None and "S" in st:
            return st["S"]
        d = self.device
        if self._ao_grid is None:
            self._ao_grid = self._eval_ao(self.grids_coords())
        chi = self._ao_grid
        nk, ngrid, nao = chi.shape
        S = d.empty((nk, nao, nao))
        alpha = np.array([self.cell.vol / ngrid, 0.0])
        beta = np.zeros(2)
        d.ctx.call("fisdf_zgemm", 3, 0, nao, nao, ngrid, alpha.ctypes.data_as(_lib._dp),
                   _lib.ptr(chi), nao, ngrid * nao, _lib.ptr(chi), nao, ngrid * nao,
                   beta.ctypes.data_as(_lib._dp), _lib.ptr(S), nao, nao * nao, nk,
                   max(1, min(64, ngrid // 1024)))
        if st is not None:
            st["S"] = S
        return S

    def _grid_aos(self):
        """The Bloch AOs on the FFT grid, device (nk, ngrid, nao): what build() left resident,
        evaluated on first use otherwise (an object restored by ``load``)."""
        if self._ao_grid is None:
            self._ao_grid = self._eval_ao(self.grids_coords())
        return self._ao_grid

    def get_rho(self, dm, hermi=1, xctype="LDA"):
        """Electron density on the FFT grid, rho[g] = (1/nk) sum_k sum_mn chi_k[g,m] D_k[m,n]
        conj(chi_k[g,n]) (PySCF fft_jk.get_j_kpts' rhoR; integrates to the electron count with the
        weight vol/ngrid): (nset, ngrid), or (ngrid,) for a single dm (nk, nao, nao).  hermi=1:
        the dms are Hermitian, rho is returned real after checking max |Im| <= 1e-10 max |rho|;
        hermi=0: complex.

        xctype="GGA": the density with its gradient, (nset, 4, ngrid) or (4, ngrid) — component 0
        rho, 1..3 d rho / dx, dy, dz (PySCF ``eval_rho(..., xctype="GGA")``'s layout).  The AO
        values and derivatives are evaluated a grid block at a time (``deriv_work_bytes``) and
        consumed by fisdf_get_rho_gga; the result does not depend on the budget, bit for bit."""
        if xctype not in self.XCTYPES:
            raise ValueError(f"get_rho: xctype must be one of {list(self.XCTYPES)}, "
                             f"not {xctype!r}")
        d = self.device
        if d.sharded(self):
            raise NotImplementedError("get_rho on a k-sharded object")
        self._kmesh()
        dms, ddms = _dms_to_dev(self, dm)
        nset = ddms.shape[0]
        if xctype == "GGA":
            out = _get_rho_gga(self, ddms, nset, hermi)
            check = out[:, 0]
        else:
            f = self._grid_aos()
            nk, ngrid, nao = f.shape
            rho = d.empty((nset, ngrid))
            d.ctx.call("fisdf_get_rho", _lib.ptr(f), ngrid * nao, nk, ngrid, nao, _lib.ptr(ddms),
                       nset, _lib.ptr(rho))
            out = check = d.to_host(rho)
        if hermi == 1:
            if abs(check.imag).max() > 1e-10 * abs(check).max():
                raise ValueError("get_rho(hermi=1): the density is not real (max |Im rho| = "
                                 f"{abs(check.imag).max():.3e}); pass hermi=0 for general dms")
            out = np.ascontiguousarray(out.real)
        nd = np.ndim(dm)
        return out[0] if nd < 4 else out

    def deriv_block_points(self, kpts=None):
        """Grid points per block of the AO values with first derivatives that ``deriv_work_bytes``
        allows, for the k-mesh (None) or for ``kpts``."""
        self._kmesh()
        return _deriv_plan(self, kpts)[0]

    def nr_vxc_mat(self, wv, kpts=None, xctype=None):
        """The exchange-correlation potential matrices of a caller's functional derivatives on
        the FFT grid (PySCF ``KNumInt.nr_rks``' matrix step; the functional itself stays with the
        caller).  GGA: ``wv`` (4, ngrid) or (nset, 4, ngrid) real, wv[0] = de/drho and
        wv[1:4] = 2 de/dsigma grad rho, unweighted (the quadrature weight vol/ngrid is applied
        here):
          V_k[m,n] = (vol/ngrid) sum_g { wv_0 conj f[g,m] f[g,n]
                     + sum_c wv_c (conj d_c f[g,m] f[g,n] + conj f[g,m] d_c f[g,n]) }
        (``aow = 1/2 wv_0 f + sum_c wv_c d_c f; V = f^H aow + h.c.``), Hermitian by construction.
        LDA: ``wv`` (ngrid,) or (nset, ngrid), V = (vol/ngrid) f^H wv f over the resident AOs.
        A 2-D ``wv`` of shape (4, ngrid) is read as one GGA set unless xctype="LDA" says
        otherwise.  Returns (..., nk, nao, nao) on the host: at the k-mesh (kpts None), at (n, 3)
        ``kpts`` ((n, nao, nao)) or at one (3,) k-point ((nao, nao)); points off the mesh go
        through the band evaluator.  No build() needed."""
        return _nr_vxc_mat(self, wv, kpts, xctype)

    def get_kin(self, kpts=None):
        """The kinetic matrices by the FFT-grid quadrature,
          T_k[m,n] = 1/2 (vol/ngrid) sum_g sum_c conj d_c f_k[g,m] d_c f_k[g,n],
        the companion of ``get_ovlp``: the quadrature ``get_ovlp``, ``get_pp`` and the exact J
        use, so that ``get_pp() + get_kin()`` is a core Hamiltonian on one grid.  It is NOT
        PySCF's analytic ``pbc_intor('int1e_kin')``: it converges to it with the mesh, and a
        steep basis function needs a fine mesh.  Arguments and shapes as ``get_pp``; at Gamma
        the imaginary part is set to zero.  No build() needed."""
        return _get_kin(self, kpts)

    def eval_xc(self, xc, rho):
        """The functional ``xc`` (a name of ``fisdf.xc.FUNCTIONALS`` or a ``fisdf.xc.Functional``)
        at the points of ``rho`` as ``get_rho`` returns it — GGA: (4, n) or (nset, 4, n), LDA:
        (n,) or (nset, n), real (of a complex rho the real part is read); n is the grid or any
        block of it.  Returns ``(e, wv)`` on the host: e (..., n) the energy per unit volume
        (E_xc = vol/ngrid sum e), wv the unweighted ``wv`` of ``nr_vxc_mat`` ((..., 4, n) with
        wv[0] = de/dn, wv[1:4] = 2 de/dsigma grad n; LDA (..., n)).  Points with n <=
        ``xc_rho_cut`` give exact zeros.  fisdf_xc_eval; pointwise, so the result does not depend
        on how the grid is cut into calls.  ``nr_vxc_mat(eval_xc(xc, get_rho(dm, xctype="GGA"))[1],
        kpts=band)`` is V at band k-points."""
        return _eval_xc(self, xc, rho)

    def nr_rks_block_points(self, nset=1):
        """Grid points per block of ``nr_rks`` for a GGA with ``nset`` density matrices:
        ``deriv_work_bytes`` bounds the AO derivative block together with the arena of
        fisdf_nr_rks_block (fisdf_nr_rks_plan), so it is at most ``deriv_block_points()``."""
        self._kmesh()
        return _nr_rks_plan(self, int(nset))[0]

    def nr_rks(self, xc, dm, hermi=1):
        """PySCF ``KNumInt.nr_rks``' ``(nelec, exc, vxc)`` of closed-shell density matrices
        ``dm`` (nk, nao, nao) — floats and vxc (nk, nao, nao) — or (nset, nk, nao, nao), each set
        an independent density — arrays (nset,) and vxc (nset, nk, nao, nao).  ``xc``: a name of
        ``fisdf.xc.FUNCTIONALS`` ("lda", "pbe", "pbe0", "hf"), a ``fisdf.xc.Functional`` or a
        callable.  For a hybrid this is the local part; the step is
        ``vxc + vj - 0.5 * fisdf.hybrid_coeff(xc) * vk``.

        GGA: one walk over the grid in blocks of the AO values with first derivatives, and per
        block fisdf_nr_rks_block: the density with its gradient, the functional and the potential
        matrix without leaving the device.  rho is ``get_rho(xctype="GGA")``'s, bit for bit;
        nelec and exc add the block sums in block order: repeatable for a given
        ``deriv_work_bytes``, equal up to rounding across budgets, as vxc is.  vxc is Hermitian
        bit for bit.  LDA: the resident AOs, fisdf_get_rho, fisdf_xc_eval, fisdf_weighted_gram.
        "hf": zeros, the device is not touched.  A callable ``f(rho) -> (e, wv)`` on host arrays
        is treated as a GGA and called per block and set with rho (4, nb) real; it returns
        e (nb,) per unit volume and wv (4, nb) as ``nr_vxc_mat`` takes it; the walk is the same,
        with fisdf_get_rho_gga and fisdf_gga_gram around the call.  hermi must be 1.  No build()
        needed."""
        return _nr_rks(self, xc, dm, hermi)

    def get_pp(self, kpts=None):
        """``FFTDF.get_pp(kpts)`` [pyscf]: the GTH pseudopotential matrices V^loc + V^nl of
        ``cell._pseudo`` (an atom without an entry: a bare nucleus) at ``kpts`` — None: this
        object's k-mesh; a (3,) k-point: (nao, nao); (n, 3): (n, nao, nao).  The local part is
        the structure-factor sum in G space, one FFT and the AO Gram weighted by Re v(r); the
        non-local part the separable GTH projectors (fisdf_get_pp).  k-points of
        the mesh use the resident Bloch AOs, others the band AOs on the FFT grid.  No build()
        needed.  What ``KRHF.get_hcore`` calls for a cell with ``pseudo``."""
        return _get_pp(self, kpts, nuc=False)

    def get_nuc(self, kpts=None):
        """``FFTDF.get_nuc(kpts)`` [pyscf]: the nuclear attraction of the bare charges
        ``cell.atom_charges()`` — get_pp's local part with every atom a bare nucleus (the G = 0
        term dropped).  Arguments and shapes as ``get_pp``."""
        return _get_pp(self, kpts, nuc=True)

    def madelung(self):
        """``tools.pbc.madelung(cell, kpts)`` [pyscf] for this k-mesh (host scalar, cached)."""
        if getattr(self, "_madelung", None) is None:
            self._madelung = madelung(self.cell, self._kmesh())
        return self._madelung

    # ---- 4-index integrals (north-star get_eri / ao2mo surface; next-2 of SURVEY §8f) ----
    def _kidx(self, kpts):
        """Indices of k-points on the mesh (scaled coordinates modulo 1)."""
        kmesh = np.asarray(self._kmesh())
        scaled = np.asarray(kpts, float).reshape(-1, 3) @ self.cell.lattice_vectors().T / (2 * np.pi)
        v = np.rint(scaled * kmesh).astype(int) % kmesh
        if abs(scaled * kmesh - np.rint(scaled * kmesh)).max() > 1e-6:
            raise ValueError("k-points are not on the ISDF k-mesh")
        return ((v[:, 0] * kmesh[1] + v[:, 1]) * kmesh[2] + v[:, 2]).astype(np.int32), v

    def _w_of_q(self, q):
        """W_q on the device: a fitted q's own W (local or fetched from the host copy), or
        conj(W_{-q}) for the partner of a time-reversal representative."""
        st = self._dev_state
        d = self.device
        rep = q if q in set(int(x) for x in self.fit_qs) else int(self.q_partner[q])
        slot = np.nonzero(self.my_qs == rep)[0]
        if len(slot):
            W = st["Wq"][int(slot[0])]
        else:
            W = d.to_dev(self._wq[rep])
        return W.conj().resolve_conj() if rep != q else W

    def _eri_isdf(self, Cs, kpts, nmo):
        """The ISDF (ij|kl) of one k-quartet, complex (n1 n2, n3 n4) on the host (fisdf_get_eri)."""
        st = self._dev_state
        assert st is not None and "Wq" in st, "call build() first"
        d = self.device
        kidx, v = self._kidx(kpts)
        kmesh = np.asarray(self.kmesh)
        if np.any((v[0] - v[1] + v[2] - v[3]) % kmesh):
            raise ValueError("k-points violate momentum conservation k1 - k2 + k3 - k4 = G")
        qv = (v[1] - v[0]) % kmesh
        q = int((qv[0] * kmesh[1] + qv[1]) * kmesh[2] + qv[2])
        nao = self.cell.nao_nr()
        nip = st["X"].shape[1]
        W = self._w_of_q(q).contiguous()
        dC = [None if c is None else d.to_dev(np.asarray(c, dtype=np.complex128)) for c in Cs]
        ptrs = (_lib._vp * 4)(*[None if t is None else t.data_ptr() for t in dC])
        out = d.empty((nmo[0] * nmo[1], nmo[2] * nmo[3]))
        kk, kp = _lib.iarr(kidx)
        nn, np_ = _lib.iarr(nmo)
        d.ctx.call("fisdf_get_eri", _lib.ptr(st["X"]), nip, nao, kp, _lib.ptr(W), ptrs, np_,
                   _lib.ptr(out))
        return out.cpu().numpy()

    def _eri_coeffs(self, mo_coeffs):
        """(the four coefficient matrices or None each, the four widths)."""
        nao = self.cell.nao_nr()
        if mo_coeffs is None:
            Cs = [None] * 4
        elif isinstance(mo_coeffs, np.ndarray) and mo_coeffs.ndim == 2:
            Cs = [mo_coeffs] * 4
        else:
            Cs = list(mo_coeffs)
        return Cs, [nao if c is None else np.asarray(c).shape[1] for c in Cs]

    def ao2mo(self, mo_coeffs, kpts=None, compact=False, omega=None):
        """(ij|kl) for four k-points; mirrors FFTDF.ao2mo(mo_coeffs, kpts, compact) [pyscf];
        mo_coeffs None -> AO integrals.

        eri_method = "isdf": eri[ij, kl] = sum_IJ W_q[I,J] conj(XC1)[I,i] (XC2)[I,j]
        conj(XC3)[J,k] (XC4)[J,l], q = k2 - k1 (fftdf-with-k-lstsq.py:221-232), after build(); a
        non-zero omega takes the W_q of _omega_df(omega).  eri_method = "fft": the exact FFT-grid
        integrals (get_eri_many), no build() needed, at any k-points, with coulG(q, omega) (None:
        the omega this object was fitted with)."""
        _check_eri_method(self)
        kpts = np.zeros((4, 3)) if kpts is None else np.asarray(kpts, float).reshape(-1, 3)
        if kpts.shape[0] == 1:
            kpts = np.repeat(kpts, 4, axis=0)
        Cs, nmo = self._eri_coeffs(mo_coeffs)
        if self.eri_method == "fft":
            eri = self.get_eri_many(kpts[:2], kpts[None, 2:], Cs, omega)[0]
        elif omega is not None and omega != 0:
            return self._omega_df(float(omega)).ao2mo(mo_coeffs, kpts, compact)
        else:
            eri = self._eri_isdf(Cs, kpts, nmo)
        if abs(kpts).max() < 1e-9 and all(c is None or np.isrealobj(c) for c in Cs):
            eri = eri.real
            if compact and nmo[0] == nmo[1] and nmo[2] == nmo[3]:
                i0, i1 = np.tril_indices(nmo[0])
                k0, k1 = np.tril_indices(nmo[2])
                e4 = eri.reshape(nmo[0], nmo[1], nmo[2], nmo[3])
                eri = e4[i0, i1][:, k0, k1]
        return eri

    def get_eri(self, kpts=None, compact=False, omega=None):
        """AO ERIs for four k-points (FFTDF.get_eri surface [pyscf]): ISDF-factorised, or with
        eri_method = "fft" the exact FFT-grid ones."""
        return self.ao2mo(None, kpts, compact, omega)

    def get_eri_many(self, kpts12, kpts34, mo_coeffs=None, omega=None):
        """(ij|kl) for one (k1, k2) and npair (k3, k4): kpts12 (2, 3), kpts34 (npair, 2, 3) ->
        complex (npair, n1 n2, n3 n4) on the host.  eri_method = "fft": one fisdf_get_eri_fft, the
        transforms of the (k1, k2) pair densities paid once for all pairs; "isdf": a loop of
        fisdf_get_eri."""
        _check_eri_method(self)
        kpts12 = np.asarray(kpts12, float).reshape(2, 3)
        kpts34 = np.asarray(kpts34, float).reshape(-1, 2, 3)
        Cs, nmo = self._eri_coeffs(mo_coeffs)
        if self.eri_method == "fft":
            return _get_eri_fft_dev(self, kpts12, kpts34, Cs, nmo, omega)
        if omega is not None and omega != 0:
            return self._omega_df(float(omega)).get_eri_many(kpts12, kpts34, mo_coeffs)
        return np.stack([self._eri_isdf(Cs, np.concatenate([kpts12, k34]), nmo) for k34 in kpts34])

    get_ao_eri = get_eri

    # reference attributes, materialised on demand from HBM
    def __getattribute__(self, name):
        if name in ("_x", "_w0", "_wq"):
            st = object.__getattribute__(self, "_dev_state")
            if st is not None and "W0" in st:
                if name == "_x":
                    return st["X"].cpu().numpy()
                if name == "_w0":
                    return st["W0"].cpu().numpy()
                return object.__getattribute__(self, "_gather_wq")()
        return object.__getattribute__(self, name)

    def _gather_wq(self):
        """All W_q (nk, nip, nip) on the host: fitted q from every rank, partners by conj."""
        st = self._dev_state
        d = self.device
        nk = int(np.prod(self.kmesh))
        if d.size == 1 or isinstance(d.comm, kshard.EmulatedGroup):
            parts = [(self.my_qs, st["Wq"].cpu().numpy())]
        else:
            import torch.distributed as dist
            parts = [None] * d.size
            dist.all_gather_object(parts, (self.my_qs, st["Wq"].cpu().numpy()), group=d.comm)
        out = np.zeros((nk, self.nip, self.nip), complex)
        for qs, w in parts:
            out[np.asarray(qs, dtype=int)] = w
        for q in range(nk):
            p = int(self.q_partner[q])
            if p != q and q not in set(int(x) for x in self.fit_qs):
                out[q] = out[p].conj()
        return out


ISDF = InterpolativeSeparableDensityFitting

from ctypes import c_double as C_double, c_int as C_int, c_long as C_long, byref  # noqa: E402


class _TorchBuffers:
    """The composite build's device buffers (fisdf_set_allocator) taken from torch's caching
    allocator on the context's stream, so X, x4, W_q, W_s become torch tensors the rest of the
    mirror (get_jk, ERIs, the reference attributes) reads, and y returns to torch's cache as soon
    as the fit is enqueued."""

    def __init__(self, d):
        self.d = d
        self.live = {}
        self.alloc_cb = _lib.ALLOC_FN(self._alloc)
        self.free_cb = _lib.FREE_FN(self._free)
        d.ctx.call("fisdf_set_allocator", self.alloc_cb, self.free_cb, None)

    def _alloc(self, nbytes, user):
        # on the context's stream whatever stream is current when build() runs: the caching
        # allocator hands a freed block out again only to work ordered on the stream it was
        # allocated on, and fisdf.h's free_fn contract orders the buffer's last use on ctx.stream
        with self.d.torch.cuda.stream(self.d.stream):
            t = self.d.torch.empty(int(nbytes), dtype=self.d.torch.uint8, device=self.d.dev)
        self.live[t.data_ptr()] = t
        return t.data_ptr()

    def _free(self, ptr, user):
        self.live.pop(ptr, None)

    def tensor(self, ptr, shape, dtype="c128"):
        t = self.d.torch
        dt, size = {"c128": (t.complex128, 16), "f64": (t.float64, 8)}[dtype]
        n = int(np.prod(shape))
        return self.live[ptr][:n * size].view(dt).reshape(tuple(int(x) for x in shape))


def _build_one_gpu(df_obj):
    """The 1-GPU build through the library's composite entry fisdf_build (include/fisdf.h;
    fftisdf.py:22-128): selection (or the injected points), x4, y, factor + fit + FFT Coulomb of
    the fitted q, W_s — one C call; the result is adopted as torch tensors."""
    d = df_obj.device
    cell = df_obj.cell
    kmesh = np.asarray(df_obj._kmesh(), dtype=np.int32)
    nk = int(np.prod(kmesh))
    nao = cell.nao_nr()
    km_c, km_p = _lib.iarr(kmesh)
    a_c, a_p = _lib.darr(np.ascontiguousarray(cell.lattice_vectors(), dtype=np.float64).ravel())
    mesh_c, mesh_p = _lib.iarr(df_obj.mesh)
    if df_obj._ao_parent is None:
        df_obj._ao_parent = df_obj._eval_ao(cell.gen_uniform_grids(df_obj.m0))
    if df_obj._ao_grid is None:
        df_obj._ao_grid = df_obj._eval_ao(df_obj.grids_coords())
    x0, f = df_obj._ao_parent, df_obj._ao_grid
    ng0 = x0.shape[1]
    modes = {"lstsq": 0, "svd": 1, "basic": 2}
    if df_obj.fit not in modes:
        raise ValueError(f"ISDF.fit must be one of {sorted(modes)}, not {df_obj.fit!r}")
    o = _lib.BuildOpts()
    d.ctx.lib.fisdf_build_opts_default(byref(o))
    st = df_obj._dev_state
    if st is not None and "X" in st:            # points given (select_interpolation_points /
        perm_c = np.ascontiguousarray(df_obj.perm, dtype=np.int32)   # set_interpolation_points)
        o.perm, o.n_perm = perm_c.ctypes.data_as(_lib._ip), len(perm_c)
    else:
        cap = int(nao * df_obj.c0) if df_obj.nip_max is None else int(df_obj.nip_max)
        o.nip_max = max(1, min(cap, ng0))                              # fftisdf.py:383
    o.select_tol = float(df_obj.select_tol)
    o.fit_mode = modes[df_obj.fit]
    o.fit_tol = float(df_obj.fit_tol)
    o.pivoted_fit = -1 if df_obj.pivoted_fit is None else int(bool(df_obj.pivoted_fit))
    o.half_grid = -1 if df_obj.half_grid is None else int(bool(df_obj.half_grid))
    o.time_reversal = int(bool(df_obj.time_reversal))
    o.real_self_conjugate = int(bool(df_obj.real_self_conjugate))
    o.omega = float(getattr(df_obj, "_fit_omega", 0.0))
    if getattr(d, "bufs", None) is None:
        d.bufs = _TorchBuffers(d)
    nip_c = C_int()
    d.ctx.call("fisdf_build", _lib.ptr(x0), ng0, _lib.ptr(f), nao, km_p, mesh_p, a_p, byref(o),
               byref(nip_c))
    r = d.ctx.build_result()
    nip, nq = r.nip, r.nfit
    b = d.bufs
    Wq = b.tensor(r.d_Wq, (nq, nip, nip))
    df_obj._dev_state = dict(X=b.tensor(r.d_X, (nk, nip, nao)), x4=b.tensor(r.d_x4, (nk, nip, nip)),
                             Wq=Wq, W0=Wq[0], Ws=b.tensor(r.d_Ws, (nk, nip, nip), "f64"))
    df_obj.perm = np.ctypeslib.as_array(r.perm, (nip,)).copy()
    df_obj.fit_qs = np.ctypeslib.as_array(r.fit_qs, (nq,)).astype(np.int32)
    df_obj.q_partner = np.ctypeslib.as_array(r.partner, (nk,)).astype(np.int32)
    df_obj.my_qs = df_obj.fit_qs.copy()
    df_obj.ranks = np.ctypeslib.as_array(r.ranks, (nq,)).copy()
    df_obj.used_pivoted_fit = bool(r.used_pivoted_fit)
    df_obj.min_norm_slots = int(r.min_norm_slots)
    df_obj.time_reversal_used = bool(r.time_reversal)
    df_obj.tr_deviation = float(r.tr_deviation)
    df_obj.nip = nip
    ys = C_int()
    d.ctx.call("fisdf_build_y_streamed", byref(ys))
    df_obj.y_streamed = bool(ys.value)     # y formed behind the selection (fisdf_build_y_streamed)
    return df_obj


# relative tolerance of the time-reversal check (fisdf_build's kTrTol): rounding of the lattice
# phases is ~1e-15; a complex basis or a shifted k-mesh violates the symmetry at O(1)
TR_TOL = 1e-9


def _time_reversal_holds(df_obj, x0, f, kmesh):
    """x0_{-k} = conj(x0_k) and f_{-k} = conj(f_k) on the device (fisdf_check_time_reversal):
    what folding the selection Gram, x4 and y over k <= -k and W_{-q} = conj(W_q) rely on.
    The k-sharded build's counterpart of fisdf_build's own check; every rank
    holds the same inputs, so every rank reaches the same verdict.  The verdict is kept while the
    input tensors are unchanged (same storage, torch version counter and shape): a repeated
    build on resident inputs reads them once."""
    key = tuple((int(a.data_ptr()), int(a._version), tuple(a.shape)) for a in (x0, f))
    key += tuple(int(k) for k in kmesh)
    cached = getattr(df_obj, "_tr_cache", None)
    if cached is not None and cached[0] == key:
        df_obj.tr_deviation = cached[2]
        return cached[1]
    km_c, km_p = _lib.iarr(kmesh)
    out = (C_double * 2)()
    worst = 0.0
    for a in (x0, f):
        per_k = int(a.shape[1]) * int(a.shape[2])
        df_obj.device.ctx.call("fisdf_check_time_reversal", _lib.ptr(a), per_k, per_k, km_p, out)
        if out[1] > 0:
            worst = max(worst, out[0] / out[1])
    df_obj.tr_deviation = worst
    ok = worst <= TR_TOL
    df_obj._tr_cache = (key, ok, worst)
    if not ok:
        log.warning("AO inputs violate time reversal (max |a[-k] - conj(a[k])| / max |a| = "
                    "%.3e): every q fitted", worst)
    return ok


def build(df_obj):
    """fftisdf.py:22-128 on the GPU.  Leaves X, W_q (own shard), W_0, W_s resident.  One GPU:
    the library's composite fisdf_build; k-sharded: the stage entries with the collectives
    between them."""
    t0 = time.perf_counter()
    d = df_obj.device
    if not d.sharded(df_obj):
        df_obj._omega_dfs = {}                   # range-separated states of an earlier build
        _build_one_gpu(df_obj)
        df_obj.timings["build"] = time.perf_counter() - t0
        return df_obj
    torch = d.torch
    cell = df_obj.cell
    kmesh = np.asarray(df_obj._kmesh(), dtype=np.int32)
    nk = int(np.prod(kmesh))
    nao = cell.nao_nr()
    a = np.ascontiguousarray(cell.lattice_vectors(), dtype=np.float64)
    km_c, km_p = _lib.iarr(kmesh)
    a_c, a_p = _lib.darr(a.ravel())
    mesh_c, mesh_p = _lib.iarr(df_obj.mesh)
    ngrid = int(np.prod(df_obj.mesh))

    if df_obj._ao_parent is None:
        df_obj._ao_parent = df_obj._eval_ao(cell.gen_uniform_grids(df_obj.m0))
    if df_obj._ao_grid is None:
        df_obj._ao_grid = df_obj._eval_ao(df_obj.grids_coords())
    tr = bool(df_obj.time_reversal) and _time_reversal_holds(df_obj, df_obj._ao_parent,
                                                              df_obj._ao_grid, kmesh)
    df_obj.time_reversal_used = tr
    # y streamed behind the selection (fisdf_y_stream_arm): this rank's grid slice
    # of y for every fitted q is formed on a second stream as the replicated selection publishes
    # its pivots, at the point cap; kept when the selection reaches the cap.  Opt-in here
    # (FISDF_Y_STREAM_SHARDED=1): on an emulated 8-way C3 rank its 1/8-grid y hides under the
    # selection but slows it by as much (16.5-17.4 vs 17.0 ms, profiles/r06/lanes3/)
    ys_send = None
    sharded = d.sharded(df_obj)
    if df_obj._dev_state is None or "X" not in df_obj._dev_state:
        if sharded and tr and os.environ.get("FISDF_Y_STREAM_SHARDED", "0") == "1":
            ng0 = df_obj._ao_parent.shape[1]
            cap = int(nao * df_obj.c0) if df_obj.nip_max is None else int(df_obj.nip_max)
            nip_cap = max(1, min(cap, ng0))
            qs0 = np.ascontiguousarray(_fit_qset(df_obj, kmesh, tr)[0], dtype=np.int32)
            g0, ng = kshard.grid_slices(df_obj.mesh, d.size)[d.rank]
            if ng:
                send_pre = d.empty((len(qs0), nip_cap, ng))
                f = df_obj._ao_grid
                fptr = _lib._vp(f.data_ptr() + g0 * nao * f.element_size())
                d.ctx.call("fisdf_set_time_reversal", 1)
                armed = C_int()
                d.ctx.call("fisdf_y_stream_arm", _lib.ptr(df_obj._ao_parent), ng0, fptr,
                           ngrid * nao, ng, nao, nip_cap, km_p, qs0.ctypes.data_as(_lib._ip),
                           len(qs0), _lib.ptr(send_pre), byref(armed))
                if armed.value:
                    ys_send = send_pre
                del send_pre
        df_obj._select(time_reversal=tr)                                 # fftisdf.py:33
    X = df_obj._dev_state["X"]
    nip = X.shape[1]

    # X_{-k} = conj(X_k) for real AOs: x2_k (x4) and fx_k (y) formed for half the k-mesh (:38, :76)
    d.ctx.call("fisdf_set_time_reversal", 1 if tr else 0)
    x4 = d.empty((nk, nip, nip))
    d.ctx.call("fisdf_build_x4", _lib.ptr(X), nip, nao, km_p, a_p, _lib.ptr(x4))   # :38-48

    # q to fit: time-reversal representatives (W_{-q} = conj(W_q)) or every q, shared among the
    # ranks by cost: a self-conjugate q fitted with real arithmetic on its half
    # grid costs about 0.6 of a complex one; longest-first greedy (kshard.assign_q)
    fit_qs, partner, weight = _fit_qset(df_obj, kmesh, tr)
    real_q = np.array([bool(df_obj.real_self_conjugate and partner[q] == q) for q in fit_qs])
    parts = kshard.assign_q(np.where(real_q, 0.6, 1.0), d.size)
    mine = parts[d.rank]
    my_qs = np.ascontiguousarray(fit_qs[mine], dtype=np.int32)
    my_wt = np.ascontiguousarray(weight[mine], dtype=np.float64)
    nq = len(my_qs)
    qs_c = my_qs.ctypes.data_as(_lib._ip)
    f = df_obj._ao_grid
    # x4_q factorisation (replaces zgelsy's QRCP, :108) on the library's side stream,
    # overlapped with the y build enqueued next on the main stream
    d.ctx.call("fisdf_set_pivoted_fit", -1 if df_obj.pivoted_fit is None
               else (1 if df_obj.pivoted_fit else 0))
    modes = {"lstsq": 0, "svd": 1, "basic": 2}
    if df_obj.fit not in modes:
        raise ValueError(f"ISDF.fit must be one of {sorted(modes)}, not {df_obj.fit!r}")
    d.ctx.call("fisdf_set_fit_mode", modes[df_obj.fit])
    d.ctx.call("fisdf_set_half_grid", -1 if df_obj.half_grid is None else int(bool(df_obj.half_grid)))
    # the side stream starts from here (x4 built); the factor chain itself is enqueued after
    # the y build, since it reads ranks back to the host part-way (a blocking copy)
    # a k-shard's 1/N-grid y build is short, so its factor chain runs at the greatest priority
    d.ctx.call("fisdf_set_factor_priority", 1 if sharded else 0)
    if nq:
        d.ctx.call("fisdf_factor_x4_mark")
    y_streamed = False
    if ys_send is not None:
        # after the mark: the factor chain does not wait for the y stream, the exchange does
        got = C_int()
        d.ctx.call("fisdf_y_stream_finish", nip, byref(got))
        y_streamed = bool(got.value)
        if not y_streamed:
            ys_send = None
    df_obj.y_streamed = y_streamed

    def factor_async():
        if nq:
            d.ctx.call("fisdf_factor_x4_async", _lib.ptr(x4), qs_c, nq, nip,
                       float(df_obj.fit_tol), km_p if df_obj.real_self_conjugate else None)
    d.ctx.call("fisdf_set_omega", float(getattr(df_obj, "_fit_omega", 0.0)))
    df_obj._omega_dfs = {}                   # range-separated states of an earlier build
    if not sharded:
        yT = d.empty((nq, nip, ngrid))
        d.ctx.call("fisdf_build_y_qs", _lib.ptr(f), ngrid * nao, 0, ngrid, ngrid, _lib.ptr(X),
                   nip, nao, km_p, a_p, qs_c, nq, _lib.ptr(yT))                 # :67-87
        factor_async()
    else:
        # grid-sharded y (all fitted q on this rank's plane-aligned grid slice), then one
        # all-to-all hands every rank the y_q of its own q-chunk on the whole grid
        slices = kshard.grid_slices(df_obj.mesh, d.size)
        g0, ng = slices[d.rank]
        all_qs = np.ascontiguousarray(fit_qs, dtype=np.int32)
        if y_streamed:
            send = ys_send                      # formed behind the selection
        else:
            send = d.empty((len(all_qs), nip, ng))
        ys_send = None
        if ng and not y_streamed:
            fptr = _lib._vp(f.data_ptr() + g0 * nao * f.element_size())
            d.ctx.call("fisdf_build_y_qs", fptr, ngrid * nao, 0, ng, ng, _lib.ptr(X), nip, nao,
                       km_p, a_p, all_qs.ctypes.data_as(_lib._ip), len(all_qs), _lib.ptr(send))
        factor_async()
        # the all-to-all, split per local q, runs on the collective stream while this rank
        # factorises its x4_q and fits its earlier q
        pieces = kshard.exchange_y_chunked(send, nip, slices, d.rank, d.size, d.comm,
                                           parts)

    # the factor's verdict (ranks, which q the rank-revealing path redid) is read after the fit
    # call, which waits for it itself
    Wq = d.empty((nq, nip, nip))
    if not sharded:
        if nq:
            d.ctx.call("fisdf_fit_coulomb_qs", qs_c, nq, _lib.ptr(yT), nip, mesh_p, km_p, a_p,
                       _lib.ptr(Wq))
    else:
        g0s = (C_long * d.size)(*[s[0] for s in slices])
        ngs = (C_long * d.size)(*[s[1] for s in slices])
        for j, (recv, work) in enumerate(pieces):
            if work is not None:
                work.wait()               # stream-ordered: no host block with RCCL
            # the fit's FFT reads q j straight from its piece (plane-aligned grid slices); its
            # lanes wait for this point only
            d.ctx.call("fisdf_set_y_slices", j, _lib.ptr(recv), d.size, g0s, ngs)
        # one call over the whole shard: its lanes and pipelined FFT stream start each q as
        # soon as that q's piece has landed
        if nq:
            d.ctx.call("fisdf_fit_coulomb_qs", qs_c, nq, None, nip, mesh_p, km_p, a_p,
                       _lib.ptr(Wq))
        del send, pieces
        yT = None
    del yT
    ranks = np.zeros(nq, np.int32)
    if nq:
        d.ctx.call("fisdf_factor_x4_wait", ranks.ctypes.data_as(_lib._ip))
        used = C_int()
        d.ctx.call("fisdf_factor_info", byref(used))
        df_obj.used_pivoted_fit = bool(used.value)
        d.ctx.call("fisdf_min_norm_info", byref(used))
        df_obj.min_norm_slots = int(used.value)

    if sharded:
        # W_s = sqrt(nk) Re(sum_q Phi[R,q] W_q) (:204-207) mixes every rank's q; get_k on rank r
        # contracts only its interpolation-point rows, so each rank forms every rank's row block of
        # its partial sum and the blocks are reduce-scattered (W_s rows stay distributed)
        rows = [kshard.shard_range(nip, r, d.size) for r in range(d.size)]
        chunk = nk * max(b - a for a, b in rows) * nip
        Wsb = d.empty((chunk * d.size,), "f64")         # W_s is real (fftisdf.py:207)
        bounds = np.ascontiguousarray([a for a, _ in rows] + [rows[-1][1]], dtype=np.int32)
        assert all(rows[r][1] == bounds[r + 1] for r in range(d.size))
        d.ctx.call("fisdf_build_ws_blocks", _lib.ptr(Wq), qs_c, my_wt.ctypes.data_as(_lib._dp),
                   nq, nip, km_p, a_p, d.size, bounds.ctypes.data_as(_lib._ip), chunk,
                   _lib.ptr(Wsb))
        i0, i1 = rows[d.rank]
        Ws = kshard.reduce_scatter_rows(Wsb, chunk, nk * (i1 - i0) * nip, d.rank, d.size,
                                        d.comm, rows=(i0, i1)).reshape(nk, i1 - i0, nip)
        del Wsb
        owner0 = next(r for r, p in enumerate(parts) if 0 in p)          # fit_qs[0] == 0
        W0 = Wq[0].clone() if d.rank == owner0 else d.empty((nip, nip))
        kshard.broadcast_w0(W0, nk, d.comm, src_local=owner0)           # W_0 for get_j
    else:
        Ws = d.empty((nk, nip, nip), "f64")              # W_s is real (fftisdf.py:207)
        d.ctx.call("fisdf_build_ws_qs", _lib.ptr(Wq), qs_c, my_wt.ctypes.data_as(_lib._dp), nq,
                   nip, km_p, a_p, _lib.ptr(Ws))                                 # :204-207
        W0 = Wq[0]
    df_obj.fit_qs, df_obj.q_partner = fit_qs, partner
    df_obj.my_qs = my_qs
    df_obj._dev_state.update(x4=x4, Wq=Wq, W0=W0, Ws=Ws)
    df_obj.ranks = ranks
    df_obj.nip = nip
    df_obj.timings["build"] = time.perf_counter() - t0
    return df_obj


def _fit_qset(df_obj, kmesh, time_reversal=None):
    """(fit_qs, partner, weight): the q whose W_q is computed, the -q map and the W_s weights."""
    nk = int(np.prod(kmesh))
    if df_obj.time_reversal if time_reversal is None else time_reversal:
        return kshard.time_reversal_reps(kmesh)
    return (np.arange(nk, dtype=np.int32), np.arange(nk, dtype=np.int32), np.ones(nk))


def _dms_to_dev(df_obj, dm_kpts):
    nk = int(np.prod(df_obj.kmesh))
    dms = _format_dms(dm_kpts, nk).astype(np.complex128)
    return dms, df_obj.device.to_dev_async(dms)


def get_j_kpts(df_obj, dm_kpts, hermi=1, kpts=np.zeros((1, 3)), kpts_band=None, exxdiv=None):
    """fftisdf.py:133-171 (kpts_band: J at any band k-points, next-4)."""
    assert exxdiv is None
    _check_j_method(df_obj)
    dms, ddms = _dms_to_dev(df_obj, dm_kpts)
    band = _band_of(df_obj, np.asarray(kpts), kpts_band)
    return _finish_j(_get_j_dev(df_obj, ddms, band), dm_kpts, kpts, kpts_band)


def _band_of(df_obj, kpts, kpts_band):
    """kpts_band (fftisdf.py:162-164,194-196; the reference asserts nband == nkpt): None when the
    band k-points are the k-mesh itself, else the (nband, 3) array."""
    if kpts_band is None:
        return None
    kb = np.asarray(kpts_band, float).reshape(-1, 3)
    mesh_k = np.asarray(df_obj.kpts, float).reshape(-1, 3)
    if kb.shape == mesh_k.shape and abs(kb - mesh_k).max() < 1e-9:
        return None
    return kb


def _format_band(v, dm_kpts, kpts_band, kpts):
    """[pyscf] df_jk._format_jks with kpts_band: v (nset, nband, nao, nao) -> the caller's
    shape (band axis dropped for a 1-D band k-point; set axis dropped unless the dms carry one)."""
    if kpts_band is None:
        return _format_jks(v, dm_kpts)
    dm = np.asarray(dm_kpts)
    if np.ndim(kpts_band) == 1:
        v = v[:, 0]
    if dm.ndim < 3:
        return v[0]
    if dm.ndim == 3 and dm.shape[0] == np.asarray(kpts).reshape(-1, 3).shape[0]:
        return v[0]
    return v


def _band_aos(df_obj, kb):
    """AOs at the interpolation points for band k-points (device (nkb, nip, nao)), cached."""
    st = df_obj._dev_state
    cache = st.setdefault("band_aos", {})
    key = kb.round(12).tobytes()
    if key not in cache:
        pts = df_obj.cell.gen_uniform_grids(df_obj.m0)[df_obj.perm]
        if df_obj.ao_on_gpu and hasattr(df_obj.cell, "shells"):
            from .ao import eval_ao_band_gpu
            cache[key] = eval_ao_band_gpu(df_obj.device, df_obj.cell, pts, kb)
        else:                                   # a PySCF-protocol cell: pbc_eval_gto at kb
            cache[key] = df_obj.device.to_dev(bloch_ao(df_obj.cell, pts, kb))
    return cache[key]


def _check_j_method(df_obj):
    if df_obj.j_method not in df_obj.J_METHODS:
        raise ValueError(f"ISDF.j_method must be one of {list(df_obj.J_METHODS)}, "
                         f"not {df_obj.j_method!r}")


def _check_k_method(df_obj):
    if df_obj.k_method not in df_obj.K_METHODS:
        raise ValueError(f"ISDF.k_method must be one of {list(df_obj.K_METHODS)}, "
                         f"not {df_obj.k_method!r}")
    if df_obj.k_method == "fft" and df_obj.k_form not in df_obj.K_FORMS:
        raise ValueError(f"ISDF.k_form must be one of {list(df_obj.K_FORMS)}, "
                         f"not {df_obj.k_form!r}")


def _check_eri_method(df_obj):
    if df_obj.eri_method not in df_obj.ERI_METHODS:
        raise ValueError(f"ISDF.eri_method must be one of {list(df_obj.ERI_METHODS)}, "
                         f"not {df_obj.eri_method!r}")


class TaggedArray(np.ndarray):
    """An ndarray that carries attributes (PySCF's tagged-array convention: a density matrix with
    the ``mo_coeff`` and ``mo_occ`` it was made from).  ``np.asarray`` of it is the plain array."""

    def __array_finalize__(self, obj):
        if isinstance(obj, TaggedArray):
            self.__dict__.update(obj.__dict__)


def tag_array(a, **tags):
    """``a`` as a TaggedArray with ``tags`` as attributes, e.g. ``tag_array(dm, mo_coeff=C,
    mo_occ=n)`` (PySCF ``lib.tag_array``) — what k_form = "lowrank" reads its orbitals from."""
    t = np.asarray(a).view(TaggedArray)
    if isinstance(a, TaggedArray):
        t.__dict__.update(a.__dict__)
    t.__dict__.update(tags)
    return t


def lowrank_factors(dm, tol=None):
    """(A, B, ranks) with D[s][k] = A[s, k, :, :r] B[s, k, :, :r]^H, r = ranks[s, k]: A and B
    (nset, nk, nao, rmax) complex, zero beyond r, rmax = max(1, ranks.max()); ranks (nset, nk) int32.
    dm is (nk, nao, nao) or (nset, nk, nao, nao).

    A dm tagged with ``mo_coeff`` ((nk, nao, nmo), with a leading set axis where dm has one; a
    sequence per k-point will do) and ``mo_occ`` ((nk, nmo) likewise) gives the orbitals with
    occupation != 0: A = C occ, B = C.  The tags are trusted, dm itself is not read.  Otherwise an
    SVD of each D[s][k] — Hermitian or not, one code path: D = U S V^H, A = U S, B = V — keeping
    sigma > tol sigma_max(set s); tol None: nao eps, the rule of numpy.linalg.matrix_rank."""
    plain = np.asarray(dm)
    nao = plain.shape[-1]
    has_set = plain.ndim == 4
    shape = plain.shape if has_set else (1,) + plain.shape
    nset, nk = shape[:2]
    cols = [[None] * nk for _ in range(nset)]
    C, occ = getattr(dm, "mo_coeff", None), getattr(dm, "mo_occ", None)
    if C is not None and occ is not None:
        if not has_set:
            C, occ = [C], [occ]
        for s in range(nset):
            for k in range(nk):
                c, n = np.asarray(C[s][k], complex), np.asarray(occ[s][k], float)
                keep = n != 0
                cols[s][k] = (c[:, keep] * n[keep], c[:, keep])
    else:
        D = plain.reshape(shape).astype(complex)
        if tol is None:
            tol = nao * np.finfo(float).eps
        for s in range(nset):
            usv = [np.linalg.svd(D[s, k]) for k in range(nk)]
            smax = max(sv[0] for _, sv, _ in usv)
            for k, (U, sv, Vh) in enumerate(usv):
                r = int(np.count_nonzero(sv > tol * smax))
                cols[s][k] = (U[:, :r] * sv[:r], Vh[:r].conj().T)
    ranks = np.array([[cols[s][k][0].shape[1] for k in range(nk)] for s in range(nset)], np.int32)
    rmax = max(1, int(ranks.max()))
    A = np.zeros((nset, nk, nao, rmax), complex)
    B = np.zeros((nset, nk, nao, rmax), complex)
    for s in range(nset):
        for k in range(nk):
            A[s, k, :, :ranks[s, k]], B[s, k, :, :ranks[s, k]] = cols[s][k]
    return A, B, ranks


# device bytes of band AOs on the FFT grid evaluated at a time (J and K at off-mesh band k-points)
BAND_BLOCK_BYTES = 1 << 28
# byte budget of the exact K's transform rows (fisdf_get_k_fft work_bytes); 0 = the library's default
KFFT_WORK_BYTES = 0
# k_form = "auto" takes the low-rank form when sum_k r_k < K_AUTO_ROW_RATIO nk nao.  Both forms make
# the same passes over a transform row, so the row counts decide, but not at 1: at equal row counts
# (C3 shape, 2x2x2 k-mesh, rank 26 = nao) the low-rank call measured 85.49 ms against the dm form's
# 81.76 ms (its contraction is slower at full rank, and it forms the orbitals), a ratio of 0.956,
# rounded down
K_AUTO_ROW_RATIO = 0.95


def _band_grid_aos(df_obj, coords, kb):
    """Bloch AOs at the band k-points kb on the FFT grid, device (len(kb), ngrid, nao)."""
    cell = df_obj.cell
    if df_obj.ao_on_gpu and hasattr(cell, "shells"):
        from .ao import eval_ao_band_gpu
        return eval_ao_band_gpu(df_obj.device, cell, coords, kb)
    return df_obj.device.to_dev(bloch_ao(cell, coords, kb))   # a PySCF-protocol cell


def _mesh_index(df_obj, kp):
    """Indices of kp on the k-mesh, or None when a point is off the mesh (or a mesh point
    shifted by a reciprocal vector)."""
    try:
        idx, _ = df_obj._kidx(kp)
    except ValueError:
        return None
    if abs(np.asarray(df_obj.kpts)[idx] - kp).max() > 1e-9:
        return None
    return idx


def _deriv_plan(df_obj, kpts, arena=None):
    """(nb, kp, idx, tn) of a walk over the FFT grid in blocks of the AO values with first
    derivatives: nb points per block from ``deriv_work_bytes``, kp the k-points (None: the
    k-mesh), idx their k-mesh indices (None: off the mesh, band evaluator), tn the lattice
    translations of the whole grid (None for a cell evaluated on the host).  arena(nk, nao) ->
    (bytes per point, fixed bytes) of a consumer's own workspace the budget has to hold too."""
    cell = df_obj.cell
    nao = cell.nao_nr()
    kp = None if kpts is None else np.asarray(kpts, float).reshape(-1, 3)
    idx = None if kp is None else _mesh_index(df_obj, kp)
    mesh = kp is None or idx is not None
    nk = len(df_obj.kpts) if mesh else len(kp)
    tn = None
    per_point, fixed = 64 * nk * nao, 0
    if df_obj.ao_on_gpu and hasattr(cell, "shells"):
        from .cell import lattice_translations
        tn = lattice_translations(cell, df_obj.grids_coords())
        nimg = nk if mesh else max(len(tn), 1)
        per_point += 32 * nimg * nao                      # the folded images, four components
        fixed = (1 << 20) + 4096 + 24 * len(tn) + (0 if mesh else (16 * nk + 4) * len(tn))
    if arena is not None:
        ap, af = arena(nk, nao)
        per_point, fixed = per_point + ap, fixed + af
    nb = (int(df_obj.deriv_work_bytes) - fixed) // per_point
    if nb < 1:
        raise ValueError(f"deriv_work_bytes = {df_obj.deriv_work_bytes} is below one grid point "
                         f"of the AO derivative block ({per_point} bytes a point + {fixed})")
    return int(nb), kp, idx, tn


def _deriv_blocks(df_obj, plan):
    """Yield (g0, g1, f4) over the FFT grid: f4 the device block (nk, 4, g1 - g0, nao)."""
    nb, kp, idx, tn = plan
    cell, d = df_obj.cell, df_obj.device
    coords = df_obj.grids_coords()
    kmesh = df_obj._kmesh()
    mesh = kp is None or idx is not None
    on_gpu = df_obj.ao_on_gpu and hasattr(cell, "shells")
    sub = None
    if idx is not None and not (len(idx) == len(df_obj.kpts)
                                and np.array_equal(idx, np.arange(len(idx)))):
        sub = idx.astype(np.int64)
    for g0 in range(0, len(coords), nb):
        g1 = min(g0 + nb, len(coords))
        if on_gpu:
            from .ao import eval_ao_band_gpu, eval_ao_kpts_gpu
            if mesh:
                f4 = eval_ao_kpts_gpu(d, cell, coords[g0:g1], kmesh, deriv=1, tn=tn)
            else:
                f4 = eval_ao_band_gpu(d, cell, coords[g0:g1], kp, deriv=1, tn=tn)
        else:       # a PySCF-protocol cell: pbc_eval_gto("GTOval_sph_deriv1"), uploaded
            blk = max(1, int(df_obj.blksize))
            f4 = d.empty((len(df_obj.kpts) if mesh else len(kp), 4, g1 - g0, cell.nao_nr()))
            for h0 in range(g0, g1, blk):
                h1 = min(h0 + blk, g1)
                f4[:, :, h0 - g0:h1 - g0] = d.to_dev(
                    bloch_ao(cell, coords[h0:h1], df_obj.kpts if mesh else kp,
                             kmesh if mesh else None, deriv=1))
        if sub is not None:
            f4 = f4[d.torch.as_tensor(sub, device=f4.device)].contiguous()
        yield g0, g1, f4
        del f4


def _get_rho_gga(df_obj, ddms, nset, hermi):
    """rho and its gradient (nset, 4, ngrid) complex on the host (fisdf_get_rho_gga per block)."""
    if hermi not in (0, 1):
        raise ValueError(f"get_rho: hermi must be 0 or 1, not {hermi!r}")
    d = df_obj.device
    ngrid = int(np.prod(df_obj.mesh))
    rho = d.empty((nset, 4, ngrid))
    flat = rho.view(-1)
    for g0, g1, f4 in _deriv_blocks(df_obj, _deriv_plan(df_obj, None)):
        nk, _, nb, nao = f4.shape
        d.ctx.call("fisdf_get_rho_gga", _lib.ptr(f4), 4 * nb * nao, nb * nao, nk, nb, nao,
                   _lib.ptr(ddms), nset, int(hermi), _lib.ptr(flat[g0:]), ngrid)
    return d.to_host(rho)


def _nr_vxc_mat(df_obj, wv, kpts, xctype):
    d = df_obj.device
    if d.sharded(df_obj):
        raise NotImplementedError("nr_vxc_mat on a k-sharded object")
    df_obj._kmesh()
    cell = df_obj.cell
    ngrid = int(np.prod(df_obj.mesh))
    nao = cell.nao_nr()
    w = np.asarray(wv)
    if xctype is not None and xctype not in df_obj.XCTYPES:
        raise ValueError(f"nr_vxc_mat: xctype must be one of {list(df_obj.XCTYPES)} or None, "
                         f"not {xctype!r}")
    if np.iscomplexobj(w):
        raise ValueError("nr_vxc_mat: wv must be real")
    if xctype is None:
        xctype = "GGA" if w.ndim == 3 or (w.ndim == 2 and w.shape[0] == 4) else "LDA"
    gga = xctype == "GGA"
    want = ((4, ngrid), (None, 4, ngrid)) if gga else ((ngrid,), (None, ngrid))
    if not any(w.ndim == len(t) and all(a is None or a == b for a, b in zip(t, w.shape))
               for t in want) or w.size == 0:
        raise ValueError(f"nr_vxc_mat: wv of shape {w.shape} is neither {want[0]} nor "
                         f"(nset,) + {want[0]} for xctype {xctype}")
    has_set = w.ndim == len(want[1])
    w = np.ascontiguousarray(w.reshape((-1,) + want[0]), dtype=np.float64)
    nset = w.shape[0]
    single = kpts is not None and np.ndim(kpts) == 1
    scale = cell.vol / ngrid
    if gga:
        plan = _deriv_plan(df_obj, kpts)
        dw = d.torch.as_tensor(w, device=d.dev).view(-1)
        out = None
        for g0, g1, f4 in _deriv_blocks(df_obj, plan):
            nk, _, nb, _ = f4.shape
            if out is None:
                out = d.empty((nset, nk, nao, nao))
            d.ctx.call("fisdf_gga_gram", _lib.ptr(f4), 4 * nb * nao, nb * nao, nk, nb, nao,
                       _lib.ptr(dw[g0:]), 4 * ngrid, ngrid, nset, scale, 1 if g0 else 0,
                       _lib.ptr(out))
        v = d.to_host(out)
    else:
        kp = df_obj.kpts if kpts is None else np.asarray(kpts, float).reshape(-1, 3)
        idx = np.arange(len(kp)) if kpts is None else _mesh_index(df_obj, kp)
        dv = d.to_dev(w.astype(np.complex128))

        def run(f):
            o = d.empty((nset, f.shape[0], nao, nao))
            d.ctx.call("fisdf_weighted_gram", _lib.ptr(f), ngrid * nao, f.shape[0], ngrid, nao,
                       _lib.ptr(dv), nset, 0, scale, _lib.ptr(o))
            return d.to_host(o)

        if idx is not None:
            f = df_obj._grid_aos()
            if not (len(idx) == f.shape[0] and np.array_equal(idx, np.arange(f.shape[0]))):
                f = f[d.torch.as_tensor(idx.astype(np.int64), device=f.device)].contiguous()
            v = run(f)
        else:
            blk = max(1, int(BAND_BLOCK_BYTES // (16 * ngrid * nao)))
            coords = df_obj.grids_coords()
            v = np.empty((nset, len(kp), nao, nao), complex)
            for b0 in range(0, len(kp), blk):
                fb = _band_grid_aos(df_obj, coords, kp[b0:b0 + blk])
                v[:, b0:b0 + blk] = run(fb)
                del fb
    if single:
        v = v[:, 0]
    return v if has_set else v[0]


def _get_kin(df_obj, kpts):
    d = df_obj.device
    if d.sharded(df_obj):
        raise NotImplementedError("get_kin on a k-sharded object")
    df_obj._kmesh()
    cell = df_obj.cell
    ngrid = int(np.prod(df_obj.mesh))
    nao = cell.nao_nr()
    single = kpts is not None and np.ndim(kpts) == 1
    plan = _deriv_plan(df_obj, kpts)
    kp = df_obj.kpts if plan[1] is None else plan[1]
    alpha = np.array([0.5 * cell.vol / ngrid, 0.0])
    beta = np.array([1.0, 0.0])
    T = None
    for g0, g1, f4 in _deriv_blocks(df_obj, plan):
        nk, _, nb, _ = f4.shape
        if T is None:
            T = d.torch.zeros((nk, nao, nao), dtype=d.torch.complex128, device=f4.device)
        flat = f4.view(-1)
        for c in (1, 2, 3):     # T_k += 1/2 (vol/ngrid) (d_c f_k)^H (d_c f_k), in block order
            fc = _lib.ptr(flat[c * nb * nao:])
            d.ctx.call("fisdf_zgemm", 3, 0, nao, nao, nb, alpha.ctypes.data_as(_lib._dp), fc, nao,
                       4 * nb * nao, fc, nao, 4 * nb * nao, beta.ctypes.data_as(_lib._dp),
                       _lib.ptr(T), nao, nao * nao, nk, max(1, min(64, nb // 1024)))
    t = d.to_host(T)
    gamma = np.abs(kp).max(axis=1) < 1e-12
    t[gamma] = t[gamma].real
    return t[0] if single else t


def _xc_call(df_obj, fn, drho, nset, ng, want_e=True):
    """fisdf_xc_eval on a device density (nset, 4, ng) or (nset, ng) complex: device (e, wv),
    real."""
    d = df_obj.device
    gga = fn.code == _xc.GGA
    e = d.empty((nset, ng), "f64") if want_e else None
    wv = d.empty((nset, 4, ng) if gga else (nset, ng), "f64")
    d.ctx.call("fisdf_xc_eval", fn.code, fn.cx, fn.cc, float(df_obj.xc_rho_cut), _lib.ptr(drho),
               (4 if gga else 1) * ng, ng, ng, nset, _lib.ptr(e) if want_e else None, ng,
               _lib.ptr(wv), (4 if gga else 1) * ng, ng)
    return e, wv


def _eval_xc(df_obj, xc, rho):
    fn = _xc.parse_xc(xc)
    if fn.family is None:
        raise ValueError(f"eval_xc: {xc!r} has no local part")
    gga = fn.code == _xc.GGA
    r = np.asarray(rho)
    tail = 2 if gga else 1
    if r.ndim not in (tail, tail + 1) or (gga and r.shape[-2] != 4) or r.size == 0:
        want = "(4, n) or (nset, 4, n)" if gga else "(n,) or (nset, n)"
        raise ValueError(f"eval_xc: rho of shape {r.shape} is not {want} for a "
                         f"{fn.family} functional")
    has_set = r.ndim == tail + 1
    ng = r.shape[-1]
    r = np.ascontiguousarray(r.reshape((-1,) + r.shape[-tail:]), dtype=np.complex128)
    nset = r.shape[0]
    d = df_obj.device
    dr = d.to_dev(r)
    e, wv = _xc_call(df_obj, fn, dr, nset, ng)
    e, wv = d.to_host(e), d.to_host(wv)
    return (e, wv) if has_set else (e[0], wv[0])


def _nr_rks_plan(df_obj, nset):
    """_deriv_plan of the k-mesh with the arena of the fused block inside the budget.  The fixed
    part is taken at the whole grid: it does not decrease with the block."""
    ngrid = int(np.prod(df_obj.mesh))
    return _deriv_plan(df_obj, None,
                       arena=lambda nk, nao: _xc.nr_rks_arena(nk, ngrid, nao, nset))


def _nr_rks(df_obj, xc, dm, hermi):
    fn = xc if callable(xc) else _xc.parse_xc(xc)
    if hermi != 1:
        raise ValueError(f"nr_rks: hermi must be 1 (Hermitian density matrices), not {hermi!r}")
    df_obj._kmesh()
    nk = int(np.prod(df_obj.kmesh))
    single = np.ndim(dm) < 4

    def shaped(nelec, exc, vxc):
        return (float(nelec[0]), float(exc[0]), vxc[0]) if single else (nelec, exc, vxc)

    if not callable(fn) and not fn.local:       # nothing local: the device is not touched
        dms = _format_dms(dm, nk)
        return shaped(np.zeros(len(dms)), np.zeros(len(dms)), np.zeros(dms.shape, complex))
    d = df_obj.device
    if d.sharded(df_obj):
        raise NotImplementedError("nr_rks on a k-sharded object")
    dms, ddms = _dms_to_dev(df_obj, dm)
    nset, nao = dms.shape[0], dms.shape[-1]
    ngrid = int(np.prod(df_obj.mesh))
    scale = df_obj.cell.vol / ngrid
    cut = float(df_obj.xc_rho_cut)
    if not callable(fn) and fn.code == _xc.LDA:
        f = df_obj._grid_aos()
        rho = d.empty((nset, ngrid))
        d.ctx.call("fisdf_get_rho", _lib.ptr(f), ngrid * nao, nk, ngrid, nao, _lib.ptr(ddms), nset,
                   _lib.ptr(rho))
        e, wv = _xc_call(df_obj, fn, rho, nset, ngrid)
        vxc = d.empty((nset, nk, nao, nao))
        dv = wv.to(d.torch.complex128)
        d.ctx.call("fisdf_weighted_gram", _lib.ptr(f), ngrid * nao, nk, ngrid, nao,
                   _lib.ptr(dv), nset, 0, scale, _lib.ptr(vxc))
        n = d.to_host(rho).real
        nelec = scale * np.where(n > cut, n, 0.0).sum(axis=1)
        return shaped(nelec, scale * d.to_host(e).sum(axis=1), d.to_host(vxc))
    plan = _nr_rks_plan(df_obj, nset)
    vxc = d.empty((nset, nk, nao, nao))
    if not callable(fn):
        sums = d.empty((nset, 2), "f64")
        for g0, g1, f4 in _deriv_blocks(df_obj, plan):
            nb = g1 - g0
            d.ctx.call("fisdf_nr_rks_block", fn.code, fn.cx, fn.cc, cut, _lib.ptr(f4),
                       4 * nb * nao, nb * nao, nk, nb, nao, _lib.ptr(ddms), nset, scale,
                       1 if g0 else 0, _lib.ptr(vxc), _lib.ptr(sums))
        s = d.to_host(sums)
        return shaped(s[:, 0].copy(), s[:, 1].copy(), d.to_host(vxc))
    nelec, exc = np.zeros(nset), np.zeros(nset)
    for g0, g1, f4 in _deriv_blocks(df_obj, plan):
        nb = g1 - g0
        rho = d.empty((nset, 4, nb))
        d.ctx.call("fisdf_get_rho_gga", _lib.ptr(f4), 4 * nb * nao, nb * nao, nk, nb, nao,
                   _lib.ptr(ddms), nset, 1, _lib.ptr(rho), nb)
        rh = np.ascontiguousarray(d.to_host(rho).real)
        wv = np.empty((nset, 4, nb))
        for s in range(nset):
            e, w = fn(rh[s])
            e, w = np.asarray(e, float), np.asarray(w, float)
            if e.shape != (nb,) or w.shape != (4, nb):
                raise ValueError(f"nr_rks: the functional returned e {e.shape} and wv {w.shape} "
                                 f"for rho (4, {nb}); expected ({nb},) and (4, {nb})")
            wv[s] = w
            nelec[s] += scale * rh[s, 0].sum()
            exc[s] += scale * e.sum()
        dw = d.to_dev(wv)
        d.ctx.call("fisdf_gga_gram", _lib.ptr(f4), 4 * nb * nao, nb * nao, nk, nb, nao,
                   _lib.ptr(dw), 4 * nb, nb, nset, scale, 1 if g0 else 0, _lib.ptr(vxc))
    return shaped(nelec, exc, d.to_host(vxc))


def _get_pp(df_obj, kpts, nuc):
    """get_pp / get_nuc on the device (fisdf_get_pp): (n, nao, nao) on the host, or (nao, nao) for
    a (3,) k-point.  k-points that are all points of the k-mesh take the resident Bloch AOs (the
    whole mesh in place, a subset gathered); otherwise every point's AOs are evaluated on the FFT
    grid, a block of points at a time."""
    from .pp import pack_atoms
    d = df_obj.device
    if d.sharded(df_obj):
        raise NotImplementedError(("get_nuc" if nuc else "get_pp") + " on a k-sharded object")
    df_obj._kmesh()
    cell = df_obj.cell
    single = kpts is not None and np.ndim(kpts) == 1
    kp = df_obj.kpts if kpts is None else np.asarray(kpts, float).reshape(-1, 3)
    tab = pack_atoms(cell, bare=nuc)
    natm = len(tab)
    a = np.asarray(cell.lattice_vectors(), float)
    mesh_c, mesh_p = _lib.iarr(df_obj.mesh)
    a_c, a_p = _lib.darr(a.ravel())
    nao = cell.nao_nr()
    ngrid = int(np.prod(df_obj.mesh))
    idx = None
    try:
        idx, _ = df_obj._kidx(kp)
        if abs(np.asarray(df_obj.kpts)[idx] - kp).max() > 1e-9:
            idx = None      # a mesh point shifted by a reciprocal vector: other k + G
    except ValueError:
        idx = None

    def run(f, ks):
        ks_c, ks_p = _lib.darr(ks.ravel())
        out = d.empty((len(ks), nao, nao))
        d.ctx.call("fisdf_get_pp", _lib.ptr(f), ngrid * nao, len(ks), ks_p, mesh_p, a_p, nao,
                   tab, natm, 0 if nuc else 1, 0, _lib.ptr(out))
        return d.to_host(out)

    if idx is not None:
        f = df_obj._grid_aos()
        if not (len(idx) == f.shape[0] and np.array_equal(idx, np.arange(f.shape[0]))):
            f = f[d.torch.as_tensor(idx.astype(np.int64), device=f.device)].contiguous()
        v = run(f, kp)
    else:
        blk = max(1, int(BAND_BLOCK_BYTES // (16 * ngrid * nao)))
        coords = df_obj.grids_coords()
        v = np.empty((len(kp), nao, nao), complex)
        for b0 in range(0, len(kp), blk):
            fb = _band_grid_aos(df_obj, coords, kp[b0:b0 + blk])
            v[b0:b0 + blk] = run(fb, kp[b0:b0 + blk])
            del fb
    return v[0] if single else v


def _k_factors(df_obj, dm, ddms):
    """The factors of k_form "lowrank" / "auto" — (A, B, ranks) of lowrank_factors — or None for
    the dm form.  dm: what the caller gave (its tags are read), None: the device dms alone."""
    if df_obj.k_form == "dm":
        return None
    nk = ddms.shape[1]
    tagged = getattr(dm, "mo_coeff", None) is not None and getattr(dm, "mo_occ", None) is not None
    if tagged and (np.ndim(dm) == 4 or (np.ndim(dm) == 3 and np.shape(dm)[0] == nk)):
        src = dm
    else:
        src = ddms.cpu().numpy() if dm is None else _format_dms(dm, nk)
    A, B, ranks = lowrank_factors(src, df_obj.k_rank_tol)
    if df_obj.k_form == "auto" and not ranks.sum() < K_AUTO_ROW_RATIO * nk * ddms.shape[2]:
        return None
    return A, B, ranks


def _get_k_fft_dev(df_obj, ddms, exxdiv=None, band=None, omega=None, dm=None):
    """The exact FFT-grid K on the device (PySCF fft_jk.get_k_kpts), k_method = "fft", with the
    Coulomb kernel coulG(k2 - k1, omega) (None: the omega this object was fitted with): on the
    k-mesh one fisdf_get_k_fft over the resident Bloch AOs; at band k-points that are all on the
    mesh rows of that; otherwise the band AOs on the FFT grid, a block of band points at a time,
    as the output side of the same call.  exxdiv='ewald' adds madelung S D S on the mesh; off the
    mesh PySCF adds it only to the band points that are mesh members, which is refused here.
    k_form "lowrank" / "auto": the same calls to fisdf_get_k_fft_lr with the factors of _k_factors
    (dm: the caller's array, for its tags) in place of the dms; everything else is unchanged."""
    d = df_obj.device
    if d.sharded(df_obj):
        raise NotImplementedError('k_method = "fft" on a k-sharded object')
    on_mesh = None
    if band is not None:
        try:
            on_mesh, _ = df_obj._kidx(band)
        except ValueError:
            on_mesh = None
        if on_mesh is None and exxdiv == "ewald":
            raise NotImplementedError("exxdiv='ewald' at band k-points off the k-mesh")
    cell = df_obj.cell
    f = df_obj._grid_aos()
    nk, ngrid, nao = f.shape
    nset = ddms.shape[0]
    if omega is None:
        omega = getattr(df_obj, "_fit_omega", 0.0)
    omega = float(omega)
    km_c, km_p = _lib.iarr(df_obj._kmesh())
    mesh_c, mesh_p = _lib.iarr(df_obj.mesh)
    a_c, a_p = _lib.darr(np.asarray(cell.lattice_vectors(), float).ravel())
    work = int(KFFT_WORK_BYTES)
    fac = _k_factors(df_obj, dm, ddms)
    df_obj.k_form_used = "dm" if fac is None else "lowrank"
    if fac is None:
        def get_k(fb, kb_p, nb, out):
            d.ctx.call("fisdf_get_k_fft", _lib.ptr(f), ngrid * nao, km_p, mesh_p, a_p, nao,
                       _lib.ptr(ddms), nset, omega, fb, kb_p, nb, work, _lib.ptr(out))
    else:
        dA, dB = d.to_dev(fac[0]), d.to_dev(fac[1])
        rk_c, rk_p = _lib.iarr(fac[2].ravel())
        rmax = fac[0].shape[-1]

        def get_k(fb, kb_p, nb, out):
            d.ctx.call("fisdf_get_k_fft_lr", _lib.ptr(f), ngrid * nao, km_p, mesh_p, a_p, nao,
                       _lib.ptr(dA), _lib.ptr(dB), rk_p, rmax, nset, omega, fb, kb_p, nb, work,
                       _lib.ptr(out))
    if band is None or on_mesh is not None:
        vk = d.empty(ddms.shape)
        get_k(None, None, 0, vk)
        if exxdiv == "ewald":
            _ewald_exxdiv_for_G0(df_obj, ddms, vk)
        if on_mesh is not None:
            vk = vk[:, d.torch.as_tensor(on_mesh.astype(np.int64), device=vk.device)]
        return vk
    nb = len(band)
    vk = d.empty((nset, nb, nao, nao))
    blk = max(1, int(BAND_BLOCK_BYTES // (16 * ngrid * nao)))
    coords = df_obj.grids_coords()
    for b0 in range(0, nb, blk):
        b1 = min(nb, b0 + blk)
        fb = _band_grid_aos(df_obj, coords, band[b0:b1])
        kb_c, kb_p = _lib.darr(np.asarray(band[b0:b1], float).ravel())
        out = d.empty((nset, b1 - b0, nao, nao))
        get_k(_lib.ptr(fb), kb_p, b1 - b0, out)
        vk[:, b0:b1] = out
        del fb
    return vk


# byte budget of the exact ERI's transform rows and of its B operand, each (fisdf_get_eri_fft
# work_bytes); 0 = the library's default
ERI_FFT_WORK_BYTES = 0


def _eri_grid_aos(df_obj, kpts):
    """The Bloch AOs on the FFT grid, device (ngrid, nao) each, at the given k-points: the resident
    ones for points on the k-mesh, evaluated (_band_grid_aos) for any other."""
    f = df_obj._grid_aos()
    out, coords = [], None
    for k in np.asarray(kpts, float).reshape(-1, 3):
        try:
            idx, _ = df_obj._kidx(k[None])
            out.append(f[int(idx[0])])
        except ValueError:
            if coords is None:
                coords = df_obj.grids_coords()
            out.append(_band_grid_aos(df_obj, coords, k[None])[0].contiguous())
    return out


def _get_eri_fft_dev(df_obj, kpts12, kpts34, Cs, nmo, omega=None):
    """The exact FFT-grid (ij|kl) on the device (PySCF FFTDF.get_eri / ao2mo), eri_method = "fft":
    one fisdf_get_eri_fft for (k1, k2) and every (k3, k4) of kpts34, with coulG(k2 - k1, omega)
    (None: the omega this object was fitted with).  The MO coefficients are applied on the device,
    a_s = f_{k_s} C_s (fisdf_zgemm).  Host (npair, n1 n2, n3 n4)."""
    d = df_obj.device
    if d.sharded(df_obj):
        raise NotImplementedError('eri_method = "fft" on a k-sharded object')
    df_obj._kmesh()
    cell = df_obj.cell
    a = np.asarray(cell.lattice_vectors(), float)
    k1, k2 = kpts12
    for k3, k4 in kpts34:
        s = (k1 - k2 + k3 - k4) @ a.T / (2 * np.pi)
        if abs(s - np.rint(s)).max() > 1e-6:
            raise ValueError("k-points violate momentum conservation k1 - k2 + k3 - k4 = G")
    if omega is None:
        omega = getattr(df_obj, "_fit_omega", 0.0)
    npair = len(kpts34)
    one = np.array([1.0, 0.0])
    zero = np.zeros(2)

    def orbitals(f, C):
        if C is None:
            return f
        dC = d.to_dev(np.asarray(C, dtype=np.complex128))
        ngrid, nao = f.shape
        n = dC.shape[1]
        out = d.empty((ngrid, n))
        d.ctx.call("fisdf_zgemm", 0, 0, ngrid, n, nao, one.ctypes.data_as(_lib._dp), _lib.ptr(f),
                   nao, 0, _lib.ptr(dC), n, 0, zero.ctypes.data_as(_lib._dp), _lib.ptr(out), n, 0,
                   1, 1)
        return out

    f12 = _eri_grid_aos(df_obj, kpts12)
    a1, a2 = orbitals(f12[0], Cs[0]), orbitals(f12[1], Cs[1])
    f34 = _eri_grid_aos(df_obj, kpts34.reshape(-1, 3))
    a3 = [orbitals(f34[2 * p], Cs[2]) for p in range(npair)]
    a4 = [orbitals(f34[2 * p + 1], Cs[3]) for p in range(npair)]
    p3 = (_lib._vp * npair)(*[t.data_ptr() for t in a3])
    p4 = (_lib._vp * npair)(*[t.data_ptr() for t in a4])
    mesh_c, mesh_p = _lib.iarr(df_obj.mesh)
    a_c, a_p = _lib.darr(a.ravel())
    q_c, q_p = _lib.darr(k2 - k1)
    out = d.empty((npair, nmo[0] * nmo[1], nmo[2] * nmo[3]))
    d.ctx.call("fisdf_get_eri_fft", mesh_p, a_p, q_p, float(omega), _lib.ptr(a1), nmo[0],
               _lib.ptr(a2), nmo[1], p3, p4, npair, nmo[2], nmo[3], int(ERI_FFT_WORK_BYTES),
               _lib.ptr(out))
    return d.to_host(out)


def _get_j_fft_dev(df_obj, ddms, band=None, omega=None):
    """The exact FFT-grid J on the device (PySCF fft_jk.get_j_kpts), j_method = "fft", with the
    Coulomb kernel coulG(omega) (None: the omega this object was fitted with): on the
    k-mesh one fisdf_get_j_fft over the resident Bloch AOs; at band k-points that are all on the
    mesh rows of that; otherwise rho and v once, then the Gram of the band AOs on the full FFT
    grid weighted by v, a block of band points at a time.  A kpts_band that mixes on-mesh and
    off-mesh points takes the second route for all of them: the on-mesh ones are evaluated again
    on the grid rather than taken as rows of the k-mesh J (the same J to rounding)."""
    d = df_obj.device
    if d.sharded(df_obj):
        raise NotImplementedError('j_method = "fft" on a k-sharded object')
    cell = df_obj.cell
    f = df_obj._grid_aos()
    nk, ngrid, nao = f.shape
    nset = ddms.shape[0]
    if omega is None:
        omega = getattr(df_obj, "_fit_omega", 0.0)
    omega = float(omega)
    a = np.asarray(cell.lattice_vectors(), float)
    km_c, km_p = _lib.iarr(df_obj._kmesh())
    mesh_c, mesh_p = _lib.iarr(df_obj.mesh)
    a_c, a_p = _lib.darr(a.ravel())
    on_mesh = None
    if band is not None:
        try:
            on_mesh, _ = df_obj._kidx(band)
        except ValueError:
            on_mesh = None
    if band is None or on_mesh is not None:
        vj = d.empty(ddms.shape)
        d.ctx.call("fisdf_get_j_fft", _lib.ptr(f), ngrid * nao, km_p, mesh_p, a_p, nao,
                   _lib.ptr(ddms), nset, omega, None, 0, _lib.ptr(vj))
        if on_mesh is not None:
            vj = vj[:, d.torch.as_tensor(on_mesh.astype(np.int64), device=vj.device)]
        return vj
    rho = d.empty((nset, ngrid))
    v = d.empty((nset, ngrid))
    d.ctx.call("fisdf_get_rho", _lib.ptr(f), ngrid * nao, nk, ngrid, nao, _lib.ptr(ddms), nset,
               _lib.ptr(rho))
    d.ctx.call("fisdf_coulomb_potential", _lib.ptr(rho), nset, mesh_p, a_p, omega, _lib.ptr(v))
    nb = len(band)
    vj = d.empty((nset, nb, nao, nao))
    blk = max(1, int(BAND_BLOCK_BYTES // (16 * ngrid * nao)))
    coords = df_obj.grids_coords()
    scale = abs(np.linalg.det(a)) / ngrid
    for b0 in range(0, nb, blk):
        b1 = min(nb, b0 + blk)
        fb = _band_grid_aos(df_obj, coords, band[b0:b1])
        out = d.empty((nset, b1 - b0, nao, nao))
        d.ctx.call("fisdf_weighted_gram", _lib.ptr(fb), ngrid * nao, b1 - b0, ngrid, nao,
                   _lib.ptr(v), nset, 0, scale, _lib.ptr(out))
        vj[:, b0:b1] = out
        del fb
    return vj


def _get_j_dev(df_obj, ddms, band=None, omega=None):
    """vj on the device (fftisdf.py:150-166) for device dms (nset, nk, nao, nao); band: J at
    those k-points instead (nset, nband, nao, nao).  omega: see _get_j_fft_dev (the ISDF J's
    kernel is in the fitted W_0)."""
    if df_obj.j_method == "fft":
        return _get_j_fft_dev(df_obj, ddms, band, omega)
    st = df_obj._dev_state
    assert st is not None and "W0" in st, "call build() first"
    d = df_obj.device
    nset, nk, nao = ddms.shape[:3]
    nip = st["X"].shape[1]
    # sharded: each rank contracts its block of interpolation points, one all-reduce (:166)
    sharded = d.sharded(df_obj)
    i0, i1 = d.shard(nip) if sharded else (0, nip)
    if band is None:
        vj = d.empty(ddms.shape)
        d.ctx.call("fisdf_get_j_rows", _lib.ptr(st["X"]), _lib.ptr(st["W0"]), _lib.ptr(ddms),
                   nset, nk, nip, nao, i0, i1, _lib.ptr(vj))
    else:
        Xb = _band_aos(df_obj, band)
        vj = d.empty((nset, len(band), nao, nao))
        d.ctx.call("fisdf_get_j_band_rows", _lib.ptr(st["X"]), _lib.ptr(st["W0"]),
                   _lib.ptr(ddms), nset, nk, nip, nao, _lib.ptr(Xb), len(band), i0, i1,
                   _lib.ptr(vj))
    if sharded:  # the library runs on torch's current stream: the all-reduce is ordered
        kshard.allreduce_sum(vj, d.comm)
    return vj


def _finish_j(vj, dm_kpts, kpts, kpts_band):
    out = vj if isinstance(vj, np.ndarray) else vj.cpu().numpy()
    band = np.asarray(kpts if kpts_band is None else kpts_band)
    if abs(band).max() < 1e-9:                                           # :169-170
        out = out.real
    return _format_band(out, dm_kpts, kpts_band, kpts)


def get_k_kpts(df_obj, dm_kpts, hermi=1, kpts=np.zeros((1, 3)), kpts_band=None, exxdiv=None):
    """fftisdf.py:173-228 (+ exxdiv='ewald' and kpts_band on the k-mesh, next-4)."""
    assert exxdiv in (None, "ewald")
    _check_k_method(df_obj)
    dms, ddms = _dms_to_dev(df_obj, dm_kpts)
    band = _band_of(df_obj, np.asarray(kpts), kpts_band)
    return _format_band(_get_k_dev(df_obj, ddms, exxdiv, band, None, dm_kpts).cpu().numpy(),
                        dm_kpts, kpts_band, kpts)


def _get_k_dev(df_obj, ddms, exxdiv=None, band=None, omega=None, dm=None):
    """vk on the device (fftisdf.py:204-225) for device dms (nset, nk, nao, nao).  band: K at
    band k-points ON the k-mesh (rows of the k-mesh K); a band k' off the mesh needs W_q at the
    off-mesh q = k' - k, which the k-mesh fit does not produce (NotImplementedError under
    k_method = "isdf"; the exact K, k_method = "fft", has no such limit).  omega: see
    _get_k_fft_dev (the ISDF K's kernel is in the fitted W_q).  dm: the caller's array, whose
    tags the exact K's k_form = "lowrank" reads."""
    if df_obj.k_method == "fft":
        return _get_k_fft_dev(df_obj, ddms, exxdiv, band, omega, dm)
    if band is not None:
        try:
            kidx, _ = df_obj._kidx(band)
        except ValueError:
            raise NotImplementedError("K at band k-points off the ISDF k-mesh (W_q exists only "
                                      "for q on the mesh)") from None
        vk = _get_k_dev(df_obj, ddms, exxdiv)
        return vk[:, df_obj.device.torch.as_tensor(kidx.astype(np.int64), device=vk.device)]
    st = df_obj._dev_state
    assert st is not None and "Ws" in st, "call build() first"
    d = df_obj.device
    nset, nk, nao = ddms.shape[:3]
    nip = st["X"].shape[1]
    km_c, km_p = _lib.iarr(df_obj.kmesh)
    a_c, a_p = _lib.darr(np.asarray(df_obj.cell.lattice_vectors(), float).ravel())
    vk = d.empty(ddms.shape)
    # sharded: each rank contracts its block of interpolation points, one all-reduce (:225)
    sharded = d.sharded(df_obj)
    i0, i1 = d.shard(nip) if sharded else (0, nip)
    # sharded: the rank holds only its W_s rows (reduce-scattered by build)
    call = "fisdf_get_k_rows_local" if sharded else "fisdf_get_k_rows"
    d.ctx.call(call, _lib.ptr(st["X"]), _lib.ptr(st["Ws"]), _lib.ptr(ddms), nset, nip, nao, km_p,
               a_p, i0, i1, _lib.ptr(vk))
    if sharded:
        kshard.allreduce_sum(vk, d.comm)
    if exxdiv == "ewald":
        _ewald_exxdiv_for_G0(df_obj, ddms, vk)
    return vk


def _ewald_exxdiv_for_G0(df_obj, ddms, vk):
    """PySCF ``pbc.df.df_jk._ewald_exxdiv_for_G0`` (kpts_band = kpts): the G=0 exchange term left
    out by coulG(G=0) = 0, vk[x, k] += madelung * S_k D[x, k] S_k — two batched GEMMs per dm set
    on the device (T = D_k S_k, then vk += madelung * S_k T)."""
    d = df_obj.device
    S = df_obj.get_ovlp()
    nset, nk, nao = ddms.shape[:3]
    mad = df_obj.madelung()
    T = d.empty((nk, nao, nao))
    one, zero = np.array([1.0, 0.0]), np.zeros(2)
    amad = np.array([mad, 0.0])
    st = nao * nao
    for x in range(nset):
        d.ctx.call("fisdf_zgemm", 0, 0, nao, nao, nao, one.ctypes.data_as(_lib._dp),
                   _lib.ptr(ddms[x]), nao, st, _lib.ptr(S), nao, st,
                   zero.ctypes.data_as(_lib._dp), _lib.ptr(T), nao, st, nk, 1)
        d.ctx.call("fisdf_zgemm", 0, 0, nao, nao, nao, amad.ctypes.data_as(_lib._dp),
                   _lib.ptr(S), nao, st, _lib.ptr(T), nao, st, one.ctypes.data_as(_lib._dp),
                   _lib.ptr(vk[x]), nao, st, nk, 1)
