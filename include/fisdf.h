/*
 * fisdf — MI355X-native FFT-ISDF kernel library: the C-ABI drop-in boundary.
 *
 * The reference (yangjunjie0320/fft-isdf-scratch) has no native boundary: its hot
 * path is the Python module fftisdf.py calling NumPy/SciPy/PySCF.  Each entry point
 * below replaces one stage of that path; the Python mirror of the reference's
 * `ISDF` class (fft-isdf-scratch_amd/fisdf/isdf.py) binds them with ctypes
 * (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - complex arrays are complex128 (interleaved double re/im), C-contiguous.
 *  - pointers named d_* are DEVICE pointers (hipMalloc'ed, or from fisdf_malloc);
 *    pointers named h_* are host pointers.  Work is enqueued on the context's stream
 *    and is asynchronous unless the function says "synchronous".
 *  - every function returns 0 on success or a negative code; fisdf_last_error(ctx)
 *    returns the message of that context's last failure (fisdf_last_error(NULL): the last
 *    failure on the calling thread, e.g. of fisdf_create).
 *  - a context is not thread-safe; several contexts (devices) may be driven from one thread.
 *
 * Two layers: the composite entries (fisdf_build / fisdf_get_jk / fisdf_get_wq, the reference's
 * ISDF.build() and ISDF.get_jk(), fftisdf.py:308-325,390-408) drive the whole 1-GPU path; the
 * stage entries below them are what the composite entries run, exported for k-sharded callers
 * (which interleave collectives between the stages, fisdf/isdf.py) and for the tests.
 */
#ifndef FISDF_H
#define FISDF_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FISDF_ABI_VERSION 4

typedef struct fisdf_ctx fisdf_ctx;

/* stage ids for fisdf_timings */
enum {
  FISDF_ST_SELECT = 0, /* Gram + pivoted Cholesky (fftisdf.py:357-388)          */
  FISDF_ST_X4 = 1,     /* x2_k, x2_s, x4_s, x4_k (fftisdf.py:38-48)               */
  FISDF_ST_Y = 2,      /* y build (fftisdf.py:67-87)                              */
  FISDF_ST_FACTOR = 3, /* per-q factorisation of x4_q (replaces zgelsy QRCP :108) */
  FISDF_ST_FFT = 4,    /* fft(z_q * f_q) * coulG weight (fftisdf.py:113-115)      */
  FISDF_ST_TRSM = 5,   /* factored fit application (fftisdf.py:108)               */
  FISDF_ST_HERK = 6,   /* W_q = zeta z_q^H (fftisdf.py:118-121, Parseval HERK)   */
  FISDF_ST_SMALL = 7,  /* nip x nip back-substitutions + scatter                  */
  FISDF_ST_J = 8,      /* get_j_kpts (fftisdf.py:133-171)                         */
  FISDF_ST_K = 9,      /* get_k_kpts (fftisdf.py:173-228)                         */
  FISDF_ST_WS = 10,    /* W_s = Re(Phi W) sqrt(nk) (fftisdf.py:204-207)           */
  FISDF_ST_AO = 11,    /* Bloch AO values (input layer, fftisdf.py:72,367-370)    */
  FISDF_NSTAGES = 12
};

/* ---- context / memory ---------------------------------------------------- */
int fisdf_abi_version(void);
int fisdf_create(int device, void* hip_stream /* NULL: default (null) stream */, fisdf_ctx** out);
int fisdf_destroy(fisdf_ctx* ctx);
const char* fisdf_last_error(const fisdf_ctx* ctx /* NULL: the calling thread's last failure */);
int fisdf_sync(fisdf_ctx* ctx);
int fisdf_malloc(fisdf_ctx* ctx, size_t bytes, void** d_ptr);
int fisdf_free(fisdf_ctx* ctx, void* d_ptr);
int fisdf_memcpy_htod(fisdf_ctx* ctx, void* d_dst, const void* h_src, size_t bytes); /* synchronous */
int fisdf_memcpy_dtoh(fisdf_ctx* ctx, void* h_dst, const void* d_src, size_t bytes); /* synchronous */
int fisdf_set_timing(fisdf_ctx* ctx, int enable);
int fisdf_timings(fisdf_ctx* ctx, double* h_ms /* FISDF_NSTAGES */, int* h_calls); /* synchronous; resets */
/* reality invariants, max |Im| seen since the last call: [0] x2_s (fftisdf.py:43),
 * [1] fx_s (fftisdf.py:81), [2] rho_s (fftisdf.py:216).  synchronous; resets.
 * [2] covers what fisdf_get_k(_rows, _rows_local) transformed since the last call: for a row
 * block [i0, i1) the entries rho_s[R, J, I] with I in the block and every J, R and set (the ones
 * that enter the block's V_s), nothing for an empty block; an absolute value, to be judged against
 * max |rho_s|. */
int fisdf_max_imag(fisdf_ctx* ctx, double* h_out /* 3 */);

/* ---- composite entries: the whole 1-GPU build and get_jk ----------------
 * Replace InterpolativeSeparableDensityFitting.build() + get_jk() (fftisdf.py:308-325, 22-128,
 * 390-408): selection (:357-388), x4 (:38-48), y (:67-87), per-q fit + FFT Coulomb (:97-121),
 * W_s (:204-207) in one call, the results left resident on the device for fisdf_get_jk. */
typedef struct fisdf_build_opts {
  int nip_max;             /* cap on interpolation points, int(nao * c0) (fftisdf.py:383); <= 0: ng0 */
  double select_tol;       /* dpstrf tolerance of the selection; <= 0: ng0 * eps * max diag */
  const int* perm;         /* host, n_perm parent-grid indices: use these points, no selection */
  int n_perm;              /*   (ISDF.set_interpolation_points / a refit on the same points)     */
  int fit_mode;            /* FISDF_FIT_LSTSQ (gelsy semantics, default), _SVD, _BASIC */
  double fit_tol;          /* relative pivot cut of the x4_q factorisation (4.2e-15: gelsy's rank
                              decision at rcond = eps, fftisdf.py:108) */
  int pivoted_fit;         /* -1 default (fisdf_set_pivoted_fit), 0, 1 */
  int half_grid;           /* -1 default (fisdf_set_half_grid), 0, 1 */
  int time_reversal;       /* 1: fit one q of each (q, -q) pair, W_{-q} = conj(W_q) (default);
                              the build checks x0_{-k} = conj(x0_k), f_{-k} = conj(f_k) on the device
                              (relative 1e-9) and fits every q when they do not hold */
  int real_self_conjugate; /* 1: q with 2 k_q in the reciprocal lattice fitted in real arithmetic */
  double omega;            /* Coulomb kernel (fisdf_set_omega); 0 = 1/r */
} fisdf_build_opts;
void fisdf_build_opts_default(fisdf_build_opts* opts);

/* The build.  d_x0 (nk, ng0, nao) c128: Bloch AOs on the parent grid (:367-370); d_f (nk,
 * ngrid, nao): Bloch AOs on the FFT grid (:72); kmesh, mesh, a: k-mesh, FFT mesh, lattice rows
 * (bohr); opts may be NULL (defaults).  *h_nip = interpolation points.  Synchronous (returns
 * with the device work enqueued; the host waits only where the stages read ranks back).
 * Replaces the previous build's results; its buffers are released first. */
int fisdf_build(fisdf_ctx* ctx, const void* d_x0, int ng0, const void* d_f, int nao,
                const int kmesh[3], const int mesh[3], const double a[9],
                const fisdf_build_opts* opts, int* h_nip);
/* 1 in *h_streamed if the last fisdf_build formed y (:67-87) behind the selection: its fused y
 * kernel started on the first pivots the cooperative selection kernel published, on a second
 * stream, instead of after the selection (the selection's own points, time reversal, a k-mesh the
 * fused kernel covers; environment FISDF_Y_STREAM=0, read per build, turns it off).  The y,
 * hence every result, is the same either way. */
int fisdf_build_y_streamed(fisdf_ctx* ctx, int* h_streamed);
/* The same streamed y for a caller that drives the stages itself (the k-sharded mirror, one
 * process per GPU).  arm, before fisdf_select_points(_km) / fisdf_select_pivots: the arguments of
 * fisdf_build_y_qs (d_f at the first grid point of the m-point block, k stride f_kstride; y_q of
 * the ascending q-list h_qs into d_yT[slot][I][g], slot stride nip_max * m) with the point cap
 * nip_max in place of nip and d_x0 (nk, ng0, nao) in place of X; time reversal must be on
 * (fisdf_set_time_reversal) and the k-mesh one the fused y kernel covers, else *h_armed = 0 and
 * nothing streams.  The next selection then forms y on a second stream as its pivots appear.
 * finish, after the selection, with the nip it returned: *h_streamed = 1 if d_yT holds
 * fisdf_build_y_qs's result for those points (the caller skips it), 0 if not (the caller builds
 * y as usual, e.g. the selection stopped below the cap); either way the context stream is
 * ordered after the y stream.  Not synchronous for the device; finish waits for the y stream's
 * host-visible completion flag. */
int fisdf_y_stream_arm(fisdf_ctx* ctx, const void* d_x0, int ng0, const void* d_f, long f_kstride,
                       int m, int nao, int nip_max, const int kmesh[3], const int* h_qs, int nq,
                       void* d_yT, int* h_armed);
int fisdf_y_stream_finish(fisdf_ctx* ctx, int nip, int* h_streamed);

/* What the last build left resident.  Pointers stay valid until the next fisdf_build,
 * fisdf_build_release or fisdf_destroy on the context.  fisdf_build restores the context's stage
 * settings (time reversal, fit mode, pivoted fit, half grid, omega, factor priority) on return. */
typedef struct fisdf_build_result {
  int nk, nip, nao, nfit;     /* k-points, interpolation points, AOs, fitted q */
  int used_pivoted_fit;       /* 1: some x4_q needed the pivoted (rank-revealing) factorisation */
  int min_norm_slots;         /* q fitted through the minimum-norm operator */
  const int* perm;            /* host (nip): the interpolation points, parent-grid indices */
  const int* fit_qs;          /* host (nfit): fitted q, ascending (W_q slot i <-> q = fit_qs[i]) */
  const int* ranks;           /* host (nfit): numerical rank of each fitted x4_q (:122) */
  const int* partner;         /* host (nk): index of -q; W_q = conj(W_{partner[q]}) if not fitted */
  const void* d_X;            /* (nk, nip, nao) c128: x0 at the points (fftisdf.py:125, _x) */
  const void* d_x4;           /* (nk, nip, nip) c128 */
  const void* d_Wq;           /* (nfit, nip, nip) c128 */
  const void* d_Ws;           /* (nk, nip, nip) float64: W_s = Re(...) (fftisdf.py:207) */
  int time_reversal;          /* 1: one q of each (q, -q) pair fitted, W_{-q} = conj(W_q); 0: every
                                 q fitted (asked for, or the inputs failed the check below) */
  double tr_deviation;        /* max |a[-k] - conj(a[k])| / max |a| over x0 and f (0 unchecked) */
  /* k-sharded build (fisdf_build_sharded): this rank's share.  nfit / fit_qs / ranks / d_Wq are
   * the rank's own q; d_Ws holds only interpolation-point rows [row0, row1) of every W_s[R],
   * (nk, row1 - row0, nip) float64; d_W0 is W_0 (broadcast from its owner).  One GPU: rank 0 of
   * 1, rows [0, nip), d_W0 = slot 0 of d_Wq. */
  int shard_rank, shard_size;
  int row0, row1;
  const void* d_W0;           /* (nip, nip) c128 */
} fisdf_build_result;
int fisdf_build_get(fisdf_ctx* ctx, fisdf_build_result* out);
/* Time-reversal check of Bloch AO values d_a[k][per_k] (k stride k_stride elements, get_kpts
 * order over kmesh): h_out[0] = max |a[-k] - conj(a[k])| (2 |Im a| on a self-paired k), h_out[1] =
 * max |a|.  What the fold over k <= -k relies on (fisdf_set_time_reversal).  synchronous. */
int fisdf_check_time_reversal(fisdf_ctx* ctx, const void* d_a, long k_stride, long per_k,
                              const int kmesh[3], double* h_out);
int fisdf_build_release(fisdf_ctx* ctx);

/* ---- k-sharded composite build over several GPUs -----------------------------
 * One process (or thread) per GPU, each with its own context, all calling fisdf_build_sharded
 * with the same inputs and options (the Python mirror's torch.distributed build, fisdf/isdf.py
 * build(), in C).  The fitted q are shared by cost, longest first (a self-conjugate q 0.6 of a
 * complex one); the selection and x4 are replicated (identical pivots on every rank, no
 * collective); y is built on the rank's plane-aligned grid slice for every fitted q and
 * exchanged with one all-to-all per local q (each q's fit starts when its piece has landed);
 * W_s row blocks are reduce-scattered; W_0 is broadcast from the rank fitting q = 0.  W_q of a
 * rank equals the 1-GPU build's bit for bit.  fisdf_get_jk on a sharded build contracts the
 * rank's interpolation-point rows and all-reduces J and K (every rank gets the whole result).
 *
 * The collectives come from the caller (MPI, RCCL, a framework's process group) through
 * fisdf_comm; each is enqueued stream-ordered on `stream` (a hipStream_t): it may return before
 * the transfer is done, as long as work enqueued on `stream` afterwards sees the result.  Device
 * pointers throughout; zero-byte entries are allowed.  Return 0, or non-zero on failure. */
typedef struct fisdf_comm {
  int rank, size;
  void* user;
  /* send d_send[r] (send_bytes[r]) to rank r and receive d_recv[r] (recv_bytes[r]) from rank r,
   * for every r (self included) */
  int (*all_to_all)(void* user, const void* const* d_send, const size_t* send_bytes,
                    void* const* d_recv, const size_t* recv_bytes, void* stream);
  /* d_recv[i] = sum over ranks of d_send[rank * count + i], i < count */
  int (*reduce_scatter_f64)(void* user, const double* d_send, double* d_recv, size_t count,
                            void* stream);
  /* in place: d_buf[i] = sum over ranks of d_buf[i] */
  int (*allreduce_f64)(void* user, double* d_buf, size_t count, void* stream);
  /* in place: d_buf of rank `root` to every rank */
  int (*broadcast)(void* user, void* d_buf, size_t bytes, int root, void* stream);
} fisdf_comm;
/* The build of one rank.  `comm` must stay valid while the build's results are used
 * (fisdf_get_jk all-reduces through it).  Arguments otherwise as fisdf_build. */
int fisdf_build_sharded(fisdf_ctx* ctx, const fisdf_comm* comm, const void* d_x0, int ng0,
                        const void* d_f, int nao, const int kmesh[3], const int mesh[3],
                        const double a[9], const fisdf_build_opts* opts, int* h_nip);
/* A fisdf_comm over RCCL (librccl, loaded at run time): rank 0 makes the id, the caller hands it
 * to every rank (MPI_Bcast, a file, a TCP store), each rank then joins on its own GPU.  The
 * collectives run on the stream they are given, over xGMI within a node. */
#define FISDF_COMM_ID_BYTES 128
int fisdf_comm_rccl_unique_id(unsigned char h_id[FISDF_COMM_ID_BYTES]);
int fisdf_comm_rccl_init(const unsigned char h_id[FISDF_COMM_ID_BYTES], int rank, int size,
                         int device, fisdf_comm* out);
int fisdf_comm_rccl_destroy(fisdf_comm* comm);

/* ---- one process, several GPUs (SURVEY §8(b)'s fisdf_create(ndev, dev_ids)) -----------------
 * A group of n ranks, rank r on devices[r] with a context and a stream of its own, joined by
 * RCCL (FISDF_GROUP_RCCL: distinct devices) or by device copies between the ranks' buffers
 * (FISDF_GROUP_COPY: any devices, a device may repeat).  fisdf_group_build / _get_jk run
 * fisdf_build_sharded / fisdf_get_jk on every rank at once, one host thread per rank; the per-rank
 * arrays hold each rank's device pointers (the same AO values on every rank).  Results: through
 * fisdf_group_ctx(g, r) and the single-rank entries (fisdf_build_get, ...); every rank's J/K are
 * the full, all-reduced matrices.  On failure the message is fisdf_group_last_error(g). */
#define FISDF_GROUP_COPY 0
#define FISDF_GROUP_RCCL 1
typedef struct fisdf_group fisdf_group;
int fisdf_group_create(int n, const int* devices, int kind, fisdf_group** out);
int fisdf_group_destroy(fisdf_group* g);
fisdf_ctx* fisdf_group_ctx(fisdf_group* g, int rank);
const char* fisdf_group_last_error(fisdf_group* g);
int fisdf_group_build(fisdf_group* g, const void* const* d_x0, int ng0, const void* const* d_f,
                      int nao, const int kmesh[3], const int mesh[3], const double a[9],
                      const fisdf_build_opts* opts, int* h_nip);
int fisdf_group_get_jk(fisdf_group* g, const void* const* d_dms, int nset, int with_j,
                       int with_k, void* const* d_vj, void* const* d_vk);

/* Host copies of the reference's attributes (fftisdf.py:125-128): h_x (nk, nip, nao) = _x,
 * h_w0 (nip, nip) = _w0, h_wq (nk, nip, nip) = _wq (unfitted q filled as conj(W_{-q}); not on a
 * sharded build of several ranks, whose W_q are distributed: fisdf_build_get per rank).
 * synchronous. */
int fisdf_get_x(fisdf_ctx* ctx, void* h_x);
int fisdf_get_w0(fisdf_ctx* ctx, void* h_w0);
int fisdf_get_wq(fisdf_ctx* ctx, void* h_wq);

/* get_jk of the last build (fftisdf.py:390-408 -> get_k_kpts :173-228, then get_j_kpts
 * :133-171): d_dms (nset, nk, nao, nao) c128 device; d_vj / d_vk same shape (either may be NULL
 * when with_j / with_k is 0).  J is complex: a Gamma-only caller takes .real (:169-170).
 * After fisdf_build_sharded every rank calls it with the same d_dms: each contracts its own
 * interpolation-point rows and J / K are all-reduced through the build's fisdf_comm.
 * asynchronous. */
int fisdf_get_jk(fisdf_ctx* ctx, const void* d_dms, int nset, int with_j, int with_k, void* d_vj,
                 void* d_vk);

/* Device memory of the composite build's buffers (X, x4, y, W_q, W_s) from the caller, e.g. a
 * framework's caching allocator; alloc(NULL-safe) returns a device pointer of >= bytes or NULL.
 * The library returns each buffer through free_fn once it no longer uses it — the y buffer right
 * after the fit is enqueued, so free_fn must be stream-ordered on the context's stream (like
 * hipFreeAsync / a caching allocator bound to that stream); the rest at the next build or
 * fisdf_build_release (not at fisdf_destroy: the caller owns what it allocated).  NULL: library-
 * owned buffers, kept between builds of the same size (fisdf_build_release frees them). */
typedef void* (*fisdf_alloc_fn)(size_t bytes, void* user);
typedef void (*fisdf_free_fn)(void* d_ptr, void* user);
int fisdf_set_allocator(fisdf_ctx* ctx, fisdf_alloc_fn alloc, fisdf_free_fn release, void* user);

/* ---- input layer: Bloch AO values ------------------------
 * Replaces PySCF pbc_eval_gto('GTOval', coords, kpts) / KNumInt.block_loop as called at
 * fftisdf.py:72,327-355,367-370 (restated on the host by fisdf/cell.py eval_ao_kpts):
 *   chi_k(r_g)[nu] = sum_{T = n.a} exp(i k.T) phi_nu(r_g - T)
 * for contracted real-spherical Gaussian shells (l <= 3, cell.py's harmonics and order).
 * d_coords (ng, 3) f64 device; h_atoms (natm, 3); shells: atom, l, nprim, then the nprim
 * exponents / normalised coefficients of each shell in order; h_tn (nT, 3) the lattice
 * translations n to sum (T = n @ a, image R = n mod kmesh); terms with |r - T - atom| >= rcut
 * are dropped.  d_out (nk, ng, nao) c128, nk = prod(kmesh), kpts = make_kpts order.  nT = 0 gives
 * zeros, ng = 0 writes nothing.  Refused on the host, before anything is copied or launched and
 * with d_out untouched: ng or nT < 0, l outside 0..3, a shell atom outside [0, natm), nprim < 1,
 * nao other than sum (2 l + 1), a k-mesh axis < 1 (band entry: nkb < 1 or h_kpts NULL). */
int fisdf_eval_ao(fisdf_ctx* ctx, const void* d_coords, int ng, int natm, const double* h_atoms,
                  int nsh, const int* h_sh_atom, const int* h_sh_l, const int* h_sh_nprim,
                  const double* h_exps, const double* h_coefs, int nT, const int* h_tn,
                  const int kmesh[3], const double a[9], double rcut, int nao, void* d_out);

/* Same Bloch AO values at nkb arbitrary (band) k-points h_kpts (nkb, 3), cartesian 1/bohr —
 * the AOs at the interpolation points that get_jk(kpts_band=...) contracts.  d_out (nkb, ng, nao). */
int fisdf_eval_ao_band(fisdf_ctx* ctx, const void* d_coords, int ng, int natm, const double* h_atoms,
                       int nsh, const int* h_sh_atom, const int* h_sh_l, const int* h_sh_nprim,
                       const double* h_exps, const double* h_coefs, int nT, const int* h_tn,
                       int nkb, const double* h_kpts, const double a[9], double rcut, int nao,
                       void* d_out);

/* The values with their first derivatives: the arguments and the host checks of fisdf_eval_ao /
 * fisdf_eval_ao_band, d_out (nk, 4, ng, nao) c128 — per k-point component 0 the value, 1..3
 * d/dx, d/dy, d/dz (PySCF's eval_ao_kpts(..., deriv=1) layout):
 *   d_c chi_k(r) = sum_T e^{ik.T} d_c phi(r - T),   same mask |r - A - T|^2 < rcut^2,
 *   d_c [R(r^2) S_lm(d)] = R' 2 d_c S_lm + R d_c S_lm,   R' = -sum_p alpha_p c_p e^{-alpha_p r^2},
 * the gradients of the solid harmonics as polynomials (no division by r: a point on an atom gives
 * the finite p gradient and zeros for d and f).  One exponential per primitive serves the four
 * components, the translations of an image are summed in list order, and component 0 equals
 * fisdf_eval_ao's output bit for bit.  The four real components pass the k-mesh transform / band
 * tail of the value entries as 4 ng nao columns.  Workspace: the context's arena, four times the
 * value entries' folded images. */
int fisdf_eval_ao_deriv1(fisdf_ctx* ctx, const void* d_coords, int ng, int natm,
                         const double* h_atoms, int nsh, const int* h_sh_atom, const int* h_sh_l,
                         const int* h_sh_nprim, const double* h_exps, const double* h_coefs, int nT,
                         const int* h_tn, const int kmesh[3], const double a[9], double rcut,
                         int nao, void* d_out);
int fisdf_eval_ao_band_deriv1(fisdf_ctx* ctx, const void* d_coords, int ng, int natm,
                              const double* h_atoms, int nsh, const int* h_sh_atom,
                              const int* h_sh_l, const int* h_sh_nprim, const double* h_exps,
                              const double* h_coefs, int nT, const int* h_tn, int nkb,
                              const double* h_kpts, const double a[9], double rcut, int nao,
                              void* d_out);

/* ---- A1: interpolation-point selection ------------------------------------
 * Replaces InterpolativeSeparableDensityFitting.select_interpolation_points
 * (fftisdf.py:357-388): x2 = sum_q Re(x0_q^* x0_q^T); x4 = x2*x2/nk; greedy pivoted
 * Cholesky of x4 (LAPACK dpstrf semantics, tol <= 0 -> ng0*eps*max(diag)).
 * Produces the first min(nip_max, rank) pivots.  synchronous.
 *   d_x0 (nk, ng0, nao) c128;  h_perm (nip_max) int;  *h_npiv = pivots produced;
 *   *h_full_rank = 1 if the tolerance (not nip_max) stopped the factorisation. */
int fisdf_select_points(fisdf_ctx* ctx, const void* d_x0, int nk, int ng0, int nao, int nip_max,
                        double tol, int* h_perm, int* h_npiv, int* h_full_rank);
/* The same for a k-mesh (x0 in get_kpts order over kmesh[0]*kmesh[1]*kmesh[2] k-points): with
 * fisdf_set_time_reversal on (real AOs, x0_{-k} = conj(x0_k)) the Gram sums the representatives
 * k <= -k only, a paired one counted twice (36 of 64 k at 4x4x4). */
int fisdf_select_points_km(fisdf_ctx* ctx, const void* d_x0, const int kmesh[3], int ng0, int nao,
                           int nip_max, double tol, int* h_perm, int* h_npiv, int* h_full_rank);

/* The two halves of fisdf_select_points, for a k-point-sharded selection:
 * fisdf_select_gram: d_x2 (ng0, ng0) c128 = Re(sum_{q in [q0,q1)} x0_q x0_q^H) + 0i (the real
 *   part is fftisdf.py:376-378's x2, the only part :379 uses; shards are summed with an
 *   all-reduce);
 * fisdf_select_pivots: x4 = Re(x2)^2/nk and the greedy pivoted Cholesky (fftisdf.py:379-384);
 *   synchronous. */
int fisdf_select_gram(fisdf_ctx* ctx, const void* d_x0, int nk, int q0, int q1, int ng0, int nao,
                      void* d_x2);
int fisdf_select_pivots(fisdf_ctx* ctx, const void* d_x2, int nk, int ng0, int nip_max, double tol,
                        int* h_perm, int* h_npiv, int* h_full_rank);

/* Reassemble a k-shard's y after the grid-slice all-to-all: d_recv holds, for p = 0..nparts-1,
 * a (nrows, h_ng[p]) block of grid points [h_g0[p], h_g0[p]+h_ng[p]); d_yT is (nrows, ngrid). */
/* Every slice is checked before the first copy: a slice outside [0, ngrid) (or a negative count)
 * is refused with d_yT untouched.  Slices may come in any order and may be empty. */
int fisdf_unpack_slices(fisdf_ctx* ctx, const void* d_recv, int nrows, int nparts,
                        const long* h_g0, const long* h_ng, long ngrid, void* d_yT);

/* X[k, I, :] = x0[k, perm[I], :]  (fftisdf.py:388) */
int fisdf_gather_points(fisdf_ctx* ctx, const void* d_x0, int nk, int ng0, int nao,
                        const int* h_perm, int nip, void* d_X);

/* ---- A2: x4_k = Phi^H ((Phi x2_k)^2), x2_k = X_k^* X_k^T  (fftisdf.py:38-48) ----
 *   d_X (nk, nip, nao); d_x4 (nk, nip, nip); a: lattice (3x3 rows, bohr) */
int fisdf_build_x4(fisdf_ctx* ctx, const void* d_X, int nip, int nao, const int kmesh[3],
                   const double a[9], void* d_x4);

/* ---- A3: y build for one grid block (fftisdf.py:67-87) ---------------------
 * d_f: Bloch AOs of the block, element (k, g, m) at d_f[k*f_kstride + g*nao + m],
 * g in [0, nblk); writes y_q, q in [q0, q1) (a k-point shard), for grid points
 * [g0, g0+nblk) into the library's transposed layout d_yT[q-q0][I][g]
 * (q1-q0, nip, ngrid). */
int fisdf_build_y(fisdf_ctx* ctx, const void* d_f, long f_kstride, int g0, int nblk, int ngrid,
                  const void* d_X, int nip, int nao, const int kmesh[3], const double a[9],
                  int q0, int q1, void* d_yT);

/* Same for an explicit ascending q-list h_qs[0..nq) (e.g. the time-reversal representatives
 * of this rank, see fisdf_fit_coulomb_qs): y_q is written to d_yT[i] for q = h_qs[i]. */
int fisdf_build_y_qs(fisdf_ctx* ctx, const void* d_f, long f_kstride, int g0, int nblk, int ngrid,
                     const void* d_X, int nip, int nao, const int kmesh[3], const double a[9],
                     const int* h_qs, int nq, void* d_yT);

/* ---- A4: per-q factorisation of x4_q, q in [q0, q1) (replaces zgelsy's QRCP,
 * fftisdf.py:108).  Pivoted Cholesky with rank cut tol_rel*max(diag); factors stay in
 * the context.  d_x4: (nk, nip, nip) (all q).  synchronous: h_ranks (q1-q0) receives
 * the numerical ranks (logged at fftisdf.py:122). */
int fisdf_factor_x4(fisdf_ctx* ctx, const void* d_x4, int q0, int q1, int nip, double tol_rel,
                    int* h_ranks);
/* q-list form: factors x4_q for q = h_qs[i] (ascending); h_ranks (nq).  kmesh (may be NULL):
 * q that are their own time-reversal partner (2 k_q a reciprocal-lattice vector) have real
 * x4_q, y_q, z_q and W_q; with kmesh given they are factored as real and fitted with real-
 * factor / real-part GEMMs (half the MFMA work). */
int fisdf_factor_x4_qs(fisdf_ctx* ctx, const void* d_x4, const int* h_qs, int nq, int nip,
                       double tol_rel, const int* kmesh, int* h_ranks);
/* Asynchronous form: enqueues the factorisation on the context's side stream (after the work
 * already enqueued on the main stream, i.e. x4) and returns at once, so the y build enqueued
 * next overlaps it.  fisdf_factor_x4_wait (synchronous on the side stream) returns the ranks;
 * fisdf_fit_coulomb_qs waits by itself. */
int fisdf_factor_x4_async(fisdf_ctx* ctx, const void* d_x4, const int* h_qs, int nq, int nip,
                          double tol_rel, const int* kmesh);
int fisdf_factor_x4_wait(fisdf_ctx* ctx, int* h_ranks /* nq, may be NULL */);
/* Record the point on the main stream (x4 built) the next fisdf_factor_x4_async starts from, so
 * that the y build can be enqueued between the two calls: the factorisation reads its ranks back
 * to the host mid-chain, which can block the enqueueing thread until the side stream gets there. */
int fisdf_factor_x4_mark(fisdf_ctx* ctx);
/* Factorisation path.  Default (mode -1: unless FISDF_PIVOTED_FIT=1 in the environment): an
 * unpivoted blocked Cholesky, kept when every pivot exceeds tol_rel * max(diag) (the full-rank
 * verdict of the rank-revealing factorisation) and otherwise redone — for the whole batch —
 * by the greedy pivoted Cholesky; mode 1 forces the pivoted one, mode 0 the default.
 * fisdf_factor_info: 1 if the last factorisation used the pivoted path. */
int fisdf_set_pivoted_fit(fisdf_ctx* ctx, int mode);
int fisdf_factor_info(fisdf_ctx* ctx, int* h_used_pivoted);
/* Solution the fit applies (replaces scipy lstsq/gelsy, fftisdf.py:108, and the SVD
 * pseudo-solve of fftdf-with-k-svd.py:158-164):
 *  FISDF_FIT_LSTSQ (default): gelsy's semantics — the unique solution of a full-rank x4_q
 *    (blocked Cholesky, TRSM-first factored order) and, when the rank-revealing factor finds
 *    rank r < nip, the MINIMUM-NORM solution z = x4_r^+ y: A = P L (nip x r), thin QR A = Q R
 *    (shifted CholeskyQR3 on the device), z[P] = M^H M y[P] with M = A^+ = R^{-1} Q^H — the
 *    complete orthogonal step gelsy takes after its QRCP;
 *  FISDF_FIT_SVD: the truncated pseudo-solve on every q (rank-revealing factor with the
 *    relative cut tol_rel, then the same minimum-norm operator), the "SVD fit" configuration;
 *  FISDF_FIT_BASIC: the basic solution z[P1] = L11^-H L11^-1 y[P1] (round-1 behaviour).
 * fisdf_min_norm_info: number of q of the last factorisation fitted through M. */
#define FISDF_FIT_LSTSQ 0
#define FISDF_FIT_SVD 1
#define FISDF_FIT_BASIC 2
int fisdf_set_fit_mode(fisdf_ctx* ctx, int mode);
/* A self-conjugate q (real z_q: Zhat(G') = conj(Zhat(G)), G' = -G - 2 k_q) is fitted on half the
 * grid — one member of each pair G, G' with the pair's combined Coulomb weight, the asymmetric
 * pairs' Im(W) from a signed-weight GEMM — so its TRSM and HERK run over ~N/2 columns.
 * mode -1: environment FISDF_HALF_G (default on), 0 off (full grid), 1 on. */
int fisdf_set_half_grid(fisdf_ctx* ctx, int mode);
int fisdf_min_norm_info(fisdf_ctx* ctx, int* h_nslots);

/* ---- A4+A5: fit + FFT Coulomb for the factored shard q in [q0, q1) (fftisdf.py:97-121)
 * Needs fisdf_factor_x4 on the same range.  W_q = zeta_q z_q^H computed as
 * (vol/N^2) Zhat diag(coulG(k_q+G)) Zhat^H with Zhat = FFT(z_q * f_q), the
 * fit applied in factored order.  d_yT: (q1-q0, nip, ngrid) from fisdf_build_y;
 * d_Wq: (q1-q0, nip, nip). */
int fisdf_fit_coulomb(fisdf_ctx* ctx, int q0, int q1, const void* d_yT, int nip,
                      const int mesh[3], const int kmesh[3], const double a[9], void* d_Wq);
/* q-list form (the list given to fisdf_factor_x4_qs).  Time reversal: y_s and x4_s are real
 * (fftisdf.py:43,81), so y_{-q} = conj(y_q), x4_{-q} = conj(x4_q) and W_{-q} = conj(W_q);
 * callers may fit only one q of each (q, -q) pair and weight it 2 in fisdf_build_ws_qs. */
int fisdf_fit_coulomb_qs(fisdf_ctx* ctx, const int* h_qs, int nq, const void* d_yT, int nip,
                         const int mesh[3], const int kmesh[3], const double a[9], void* d_Wq);
/* Fit lanes: the q of one fisdf_fit_coulomb_qs call are spread round-robin over `lanes`
 * streams with private workspaces (one q's memory-bound FFT/HERK overlaps another's
 * MFMA-bound TRSM); 0 (default): FISDF_FIT_LANES from the environment, else 2.  Results do
 * not depend on it (same kernels, same per-q arithmetic). */
int fisdf_set_fit_lanes(fisdf_ctx* ctx, int lanes);
/* Stream priority of the x4_q factorisation chain (fisdf_factor_x4_async): 0 (default) = the
 * device's least priority (the 1-GPU build, where the chain hides behind the y build), 1 = the
 * greatest (a k-shard, whose 1/N-grid y build leaves the chain on the critical path). */
int fisdf_set_factor_priority(fisdf_ctx* ctx, int high);
/* Pipelined FFT stream of the fit (with >= 2 lanes): mode -1 = FISDF_FIT_PIPE from the
 * environment (default on), 0 off (the FFT runs in its lane), 1 on; the FFTs run ahead of the
 * lanes into a ring of `depth` Yhat slots (0: FISDF_PIPE_DEPTH or lanes + 2), i.e.
 * depth x rank x ngrid complex of workspace (C3: 448 MB per slot), whatever the number of q.
 * Falls back to the in-lane FFT when the device lacks the memory.  Results do not depend on it. */
int fisdf_set_fit_pipe(fisdf_ctx* ctx, int mode, int depth);
/* What the last fisdf_fit_coulomb_qs ran with: MFMA lanes and ring depth (0 = not pipelined). */
int fisdf_fit_info(fisdf_ctx* ctx, int* h_lanes, int* h_pipe_depth);
/* What the last fisdf_fit_coulomb_qs that passed its argument checks did for the j-th q of its
 * list (read-only, for tests of its dispatch).  info: [0] rank; [1] real factor; [2] half-grid
 * weights; [3] the FFT took its Hermitian-paired form (register meshes); [4] grid columns fitted;
 * [5] weight-asymmetric G listed (0 for a q without a real factor); [6] the solve that formed U:
 * 0 one lower-triangular GEMM with L^-1, 1 the minimum-norm operator, 2 the blocked substitution
 * (basic solution of a short rank), -1 none (rank 0); [7] minimum-norm slot; [8] lane; [9] W_PP:
 * 0 the batched tail's two triangular GEMMs, 1 in the lane, 2 the batched tail's blocked
 * substitution; [10] split-K of the W_PP GEMMs (1 where they did not run); [11] y read from:
 * 0 d_yT, 1 plane slices in place, 2 plane slices unpacked first. */
int fisdf_fit_report(fisdf_ctx* ctx, int j, int info[12]);
/* The fit's host-side rules for q of a k-mesh on a mesh, in a call of nq q with nip points (no
 * context, no device).  info: [0] q is its own time-reversal partner; [1..3] m = 2 k_q in
 * reciprocal-lattice units (0 otherwise); [4] the half grid's prefix planes (mesh[0] for a q
 * that is not self-conjugate); [5] its columns; [6] nq is large enough for W_PP in the lanes
 * (FISDF_LANE_WPP overrides); [7] split-K of the W_PP GEMMs (FISDF_WPP_KSPLIT, read per call). */
int fisdf_fit_plan(const int kmesh[3], const int mesh[3], int q, int nq, int nip, int info[8]);
/* Sharded build: record, on the context's stream, that y of the j-th q of the NEXT
 * fisdf_fit_coulomb_qs call has landed in d_yT (after its all-to-all piece is unpacked).  When
 * every q of that call is marked, the call runs its lanes on side streams and starts each q's
 * FFT as soon as its own piece is there (one call for the whole shard keeps the lanes and the
 * pipelined FFT stream; replaces one call per q).  Marks are consumed by the call. */
int fisdf_mark_y_ready(fisdf_ctx* ctx, int j);
/* The same, with the j-th q's y read IN PLACE from its all-to-all piece d_recv (replaces
 * fisdf_unpack_slices + fisdf_mark_y_ready): d_recv holds, for p = 0..nparts-1, the (nip,
 * h_ng[p]) block of grid points [h_g0[p], h_g0[p] + h_ng[p]), whole planes of the mesh; the fit's
 * FFT reads each plane where it lies.  Every piece of one call has the same layout; d_yT of that
 * call may then be NULL.  The piece must stay alive until the call's work is done. */
int fisdf_set_y_slices(fisdf_ctx* ctx, int j, const void* d_recv, int nparts, const long* h_g0,
                       const long* h_ng);
/* Grow the context's scratch arena to at least `bytes` now (pre-allocation; a failed growth
 * leaves an empty arena, never a stale one). */
int fisdf_reserve_workspace(fisdf_ctx* ctx, size_t bytes);
/* Coulomb kernel of the fit (and of fisdf_coulg): 0 = 1/r (default, fftisdf.py:114); omega > 0 the
 * long-range erf(omega r)/r, omega < 0 the short-range erfc(|omega| r)/r (PySCF get_coulG's
 * omega; the reference's get_jk raises for omega, fftisdf.py:392-393). */
int fisdf_set_omega(fisdf_ctx* ctx, double omega);
/* Time reversal of the inputs (real AOs, k-mesh closed under k -> -k): f_{-k} = conj(f_k)
 * and x_{-k} = conj(x_k), so fx_{-k} = conj(fx_k) (fftisdf.py:76) and fisdf_build_y(_qs)
 * computes fx_k only for the k-planes a <= kmesh[0]/2.  Default 0 (every k computed). */
int fisdf_set_time_reversal(fisdf_ctx* ctx, int on);

/* ---- A8 prep: W_s[R] = sqrt(nk) Re(sum_{q in [q0,q1)} Phi[R,q] W_q) (fftisdf.py:204-207)
 * d_Wq: (q1-q0, nip, nip) shard; d_Ws: (nimg, nip, nip) REAL float64 (the reference keeps
 * W_s = ws.real, :207; a partial sum for a q-shard, summed over the shards). */
int fisdf_build_ws(fisdf_ctx* ctx, const void* d_Wq, int q0, int q1, int nip,
                   const int kmesh[3], const double a[9], void* d_Ws);
/* q-list form: W_s[R] = sqrt(nk) Re(sum_i h_wt[i] Phi[R,q_i] W_{q_i}) (h_wt NULL: all 1;
 * 2 for a time-reversal representative whose partner -q is not listed).  synchronous. */
int fisdf_build_ws_qs(fisdf_ctx* ctx, const void* d_Wq, const int* h_qs, const double* h_wt,
                      int nq, int nip, const int kmesh[3], const double a[9], void* d_Ws);

/* Row block [i0, i1) of W_s for a q-list: d_Ws (nk, i1-i0, nip) float64 = rows i0..i1 of every W_s[R] of
 * fisdf_build_ws_qs.  A k-sharded build forms every rank's block of its partial sum and
 * REDUCE-SCATTERS them (each rank then holds the rows its get_k contracts, half the bytes of the
 * all-reduce of the whole W_s).  asynchronous. */
int fisdf_build_ws_rows(fisdf_ctx* ctx, const void* d_Wq, const int* h_qs, const double* h_wt,
                        int nq, int nip, const int kmesh[3], const double a[9], int i0, int i1,
                        void* d_Ws);
/* Every rank's row block in one call (the reduce-scatter input): block b = rows
 * [h_rows[b], h_rows[b+1]) written as (nk, rows, nip) float64 at d_Wsb + b * chunk doubles.
 * asynchronous. */
int fisdf_build_ws_blocks(fisdf_ctx* ctx, const void* d_Wq, const int* h_qs, const double* h_wt,
                          int nq, int nip, const int kmesh[3], const double a[9], int nblk,
                          const int* h_rows, long chunk, void* d_Wsb);

/* ---- A7: get_j_kpts (fftisdf.py:133-171) ------------------------------------
 * d_dms (nset, nk, nao, nao); d_vj same shape (complex; caller takes .real for Gamma). */
int fisdf_get_j(fisdf_ctx* ctx, const void* d_X, const void* d_W0, const void* d_dms, int nset,
                int nk, int nip, int nao, void* d_vj);

/* ---- A8: get_k_kpts (fftisdf.py:173-228) ------------------------------------
 * rho_k = X_k D_k X_k^H / nk; rho_s = Phi rho_k; V_s[R,I,J] = W_s[R,I,J] Re(rho_s[R,J,I]);
 * V_k = Phi^T V_s; K_k = X_k^H V_k X_k.  Only Re(rho_s) enters V_s (the reference asserts
 * |Im rho_s| < 1e-10 and drops it, :216-217): for density matrices without D_{-k} = conj(D_k), or
 * AOs without X_{-k} = conj(X_k), Im(rho_s) is not small, it is still dropped, and slot 2 of
 * fisdf_max_imag reports its size. */
int fisdf_get_k(fisdf_ctx* ctx, const void* d_X, const void* d_Ws, const void* d_dms, int nset,
                int nip, int nao, const int kmesh[3], const double a[9], void* d_vk);

/* Row-block forms: the contribution of the interpolation points I in [i0, i1) to J / K
 * (J_k = sum_I X_k[I]^H v_I X_k[I], K_k = sum_I X_k[I]^H (V_k[I,:] X_k)); the full result is
 * the sum over a partition of [0, nip) — a sharded caller all-reduces nset*nk*nao^2 values.
 * fisdf_get_j / fisdf_get_k are the [0, nip) cases (the same launches, bit for bit); an empty
 * block writes zeros.  Refused on the host, before anything is enqueued and with the output
 * untouched: a null X, W, density-matrix or output pointer (K: a null k-mesh or lattice), nset, nk,
 * nip or nao below 1, a row range outside 0 <= i0 <= i1 <= nip, a k-mesh axis outside 1..16, and
 * for the band form nkb < 1 or a null d_Xb. */
int fisdf_get_j_rows(fisdf_ctx* ctx, const void* d_X, const void* d_W0, const void* d_dms,
                     int nset, int nk, int nip, int nao, int i0, int i1, void* d_vj);
int fisdf_get_k_rows(fisdf_ctx* ctx, const void* d_X, const void* d_Ws, const void* d_dms,
                     int nset, int nip, int nao, const int kmesh[3], const double a[9], int i0,
                     int i1, void* d_vk);
/* the same with only this block's W_s rows at hand: d_Ws_rows (nk, i1-i0, nip) float64.  d_Ws
 * of fisdf_get_k / fisdf_get_k_rows is the real (nk, nip, nip) array of fisdf_build_ws_qs. */
int fisdf_get_k_rows_local(fisdf_ctx* ctx, const void* d_X, const void* d_Ws_rows,
                           const void* d_dms, int nset, int nip, int nao, const int kmesh[3],
                           const double a[9], int i0, int i1, void* d_vk);
/* J at band k-points (get_jk kpts_band; the reference asserts nband == nkpt, fftisdf.py:164):
 * rho and v = W0 rho from the k-mesh dms as fisdf_get_j, then J_k' = Xb_k'^H diag(v) Xb_k' with
 * d_Xb (nkb, nip, nao) the AOs at the interpolation points for the band k-points (the q = 0 pair
 * fit serves any k' on both sides).  d_vj (nset, nkb, nao, nao); rows [i0, i1) as above. */
int fisdf_get_j_band_rows(fisdf_ctx* ctx, const void* d_X, const void* d_W0, const void* d_dms,
                          int nset, int nk, int nip, int nao, const void* d_Xb, int nkb, int i0,
                          int i1, void* d_vj);

/* ---- exact FFT-grid J and electron density (PySCF fft_jk.get_j_kpts) ----------------------
 * J without the ISDF fit: the density of the Bloch AOs d_f (nk, ngrid, nao) c128 (k blocks
 * f_kstride >= ngrid * nao elements apart) on the FFT grid, its Coulomb potential by one forward
 * and one inverse 3-D FFT, and the AO Gram weighted by that potential.  Each of the two AO
 * kernels reads d_f once per 4 sets, forms no grid x nao temporary and sums in a fixed order
 * (repeated calls agree bit for bit).  Arguments are checked on the host and a refused call
 * leaves its output untouched; a mesh the FFT does not take is found when the transform is
 * reached, by which time earlier stages may have written the context's scratch arena, nothing
 * else.  Asynchronous.
 *
 * The density: d_rho[s][g] = (1/nk) sum_k sum_mn f_k[g,m] D[s][k][m,n] conj(f_k[g,n]); d_dms
 * (nset, nk, nao, nao), d_rho (nset, ngrid), complex (real up to rounding for Hermitian D). */
int fisdf_get_rho(fisdf_ctx* ctx, const void* d_f, long f_kstride, int nk, int ngrid, int nao,
                  const void* d_dms, int nset, void* d_rho);
/* d_v[s] = ifft(coulG(G, omega) fft(d_rho[s])) on `mesh` (both (nset, ngrid) c128; coulG at k = 0
 * with G = 0 dropped, omega as in fisdf_set_omega but given here, the context's setting is not
 * read).  The inverse transform is the forward one between two conjugations.  A mesh the FFT
 * does not take fails with d_v untouched. */
int fisdf_coulomb_potential(fisdf_ctx* ctx, const void* d_rho, int nset, const int mesh[3],
                            const double a[9], double omega, void* d_v);
/* d_out[s][k][m][n] = scale sum_g conj(f_k[g,m]) v_s[g] f_k[g,n], with conj(v_s[g]) when conj_v
 * is not 0; d_v (nset, ngrid), d_out (nset, nk, nao, nao).  The grid is split among workgroups
 * and the partial blocks are summed in split order. */
int fisdf_weighted_gram(fisdf_ctx* ctx, const void* d_f, long f_kstride, int nk, int ngrid,
                        int nao, const void* d_v, int nset, int conj_v, double scale, void* d_out);
/* ---- GGA density and potential matrix over a block of AO values with first derivatives ------
 * d_f4: component c (0 the value, 1..3 d/dx, d/dy, d/dz) of k-point k at d_f4 + k f_kstride +
 * c f_cstride, (ng, nao) c128 each, both strides >= ng * nao (fisdf_eval_ao_deriv1's output:
 * f_kstride = 4 ng nao, f_cstride = ng nao).  ng is a block of the grid: the four-component array
 * of a whole FFT grid is not meant to be resident.
 *
 * d_rho[(s 4 + c) rho_cstride + g], complex, rho_cstride >= ng (a block writes into a whole-grid
 * array (nset, 4, ngrid) through an offset pointer and rho_cstride = ngrid):
 *   rho_0   = (1/nk) sum_k sum_mn f[g,m] D[s][k][m,n] conj f[g,n]          (fisdf_get_rho's sum)
 *   d_c rho = (1/nk) sum_k sum_mn (d_c f[g,m] D[m,n] conj f[g,n] + f[g,m] D[m,n] conj d_c f[g,n])
 * hermi = 1 (D Hermitian): d_c rho = (2/nk) sum_k Re sum_n t[g,n] conj d_c f[g,n], t = f D the
 * row rho_0 forms anyway — three real dot products more per point, imaginary part exactly 0.
 * hermi = 0: both terms (a second row u[n] = sum_m f[g,m] conj D[n,m] stands for the first).
 * One pass over d_f4 serves up to 4 sets (2 for hermi = 0 with nao > 32).  No atomics, a fixed
 * summation order: repeated calls agree bit for bit, and a point's result does not depend on the
 * block it is in.  Refused on the host with d_rho untouched: a size < 1, a stride below its
 * minimum, hermi other than 0 or 1.  Asynchronous. */
int fisdf_get_rho_gga(fisdf_ctx* ctx, const void* d_f4, long f_kstride, long f_cstride, int nk,
                      int ng, int nao, const void* d_dms, int nset, int hermi, void* d_rho,
                      long rho_cstride);
/* d_out[s][k][m,n] (+)= scale sum_g { w_0 conj f[g,m] f[g,n]
 *                        + sum_c w_c (conj d_c f[g,m] f[g,n] + conj f[g,m] d_c f[g,n]) },
 * w real doubles, d_w[s w_sstride + c w_cstride + g] (both strides >= ng), d_out (nset, nk, nao,
 * nao); accumulate = 0 overwrites, else adds to what d_out holds.  PySCF's aow = 1/2 w_0 f +
 * sum_c w_c d_c f; M = f^H aow; V = M + M^H: aow by an elementwise kernel into the arena, M by
 * the batched split-K GEMM, then M + M^H.  Hermitian bit for bit (the diagonal exactly real) when
 * what it accumulates onto is, no atomics, repeated calls agree bit for bit.  The LDA case
 * (w (nset, ng)) is fisdf_weighted_gram.  Workspace: the context's arena.  Asynchronous. */
int fisdf_gga_gram(fisdf_ctx* ctx, const void* d_f4, long f_kstride, long f_cstride, int nk, int ng,
                   int nao, const void* d_w, long w_sstride, long w_cstride, int nset, double scale,
                   int accumulate, void* d_out);
/* ---- the spin-unpolarised functional at the points of a block, and the fused RKS block --------
 * LDA: Slater exchange + PW92 correlation (libxc's "pw_mod" parameters); GGA: PBE.  With
 * n = Re rho_0, d_c n = Re rho_c (imaginary parts are not read) and sigma = |grad n|^2:
 *   d_e[s e_sstride + g]                 = cx e_x + cc e_c, the energy per unit volume
 *                                          (E_xc = (vol/ngrid) sum_g e)
 *   d_wv[s w_sstride + g]                = d e / d n
 *   d_wv[s w_sstride + c w_cstride + g]  = 2 d e / d sigma  d_c n,  c = 1..3 (GGA only)
 * — the unweighted wv of fisdf_gga_gram (LDA: the v of fisdf_weighted_gram, as real doubles).
 * d_rho[s rho_sstride + c rho_cstride + g] complex: fisdf_get_rho_gga's layout is rho_sstride =
 * 4 rho_cstride (GGA), fisdf_get_rho's rho_sstride = ngrid (LDA, rho_cstride and w_cstride not
 * read).  Minimum strides: LDA every set stride >= ng; GGA component strides >= ng and set strides
 * >= 3 component strides + ng; e_sstride >= ng.  A point with n <= rho_cut (negative or NaN n
 * included) gets e = 0 and wv = 0 exactly.  d_e or d_wv may be NULL and is then skipped.  FP64,
 * analytic derivatives in s^2 and t^2 (sigma = 0 is no special case); one point per thread, no
 * reduction: repeated calls agree bit for bit.  Refused on the host with the outputs untouched:
 * an unknown family, ng or nset < 1, a stride below its minimum, rho_cut negative or NaN, cx or cc
 * not finite.  Asynchronous. */
#define FISDF_XC_LDA 0
#define FISDF_XC_GGA 1
int fisdf_xc_eval(fisdf_ctx* ctx, int family, double cx, double cc, double rho_cut,
                  const void* d_rho, long rho_sstride, long rho_cstride, int ng, int nset,
                  void* d_e, long e_sstride, void* d_wv, long w_sstride, long w_cstride);
/* One block of a Kohn-Sham XC step (PySCF KNumInt.nr_rks), three stages back to back on the
 * context's stream over one block d_f4 of fisdf_eval_ao_deriv1 output: fisdf_get_rho_gga with
 * hermi = 1 into the arena, the functional above, and fisdf_gga_gram of its wv into
 * d_vxc (nset, nk, nao, nao) — the bits of the three entries called one after another.  Also
 * d_sums[s] = scale (sum_g n, sum_g e), doubles (nset, 2): n as the functional saw it (points at
 * or below the cut add nothing to either), summed by a tree per 256 points and then over the
 * workgroups in a fixed order, no atomics.  accumulate = 0 overwrites d_vxc and d_sums, else adds
 * to what they hold.  family must be FISDF_XC_GGA.  The arena is carved once for all three stages
 * (fisdf_nr_rks_plan); the argument checks of all three stages (family, sizes, strides, cx, cc,
 * rho_cut, scale, null pointers) run before the first launch, and a call they refuse leaves d_vxc
 * and d_sums untouched.  Asynchronous. */
int fisdf_nr_rks_block(fisdf_ctx* ctx, int family, double cx, double cc, double rho_cut,
                       const void* d_f4, long f_kstride, long f_cstride, int nk, int ng, int nao,
                       const void* d_dms, int nset, double scale, int accumulate, void* d_vxc,
                       void* d_sums);
/* The arena of fisdf_nr_rks_block, no context needed: at most *h_point_bytes ng + *h_fixed_bytes
 * bytes.  Per point 64 B of rho, 32 B of wv and 8 B of e a set and the gram's 16 nk nao B; fixed:
 * the gram's matrix and split-K partials for this ng, the workgroup sums and the alignment of the
 * seven pieces.  *h_fixed_bytes does not decrease with ng. */
int fisdf_nr_rks_plan(int nk, int ng, int nao, int nset, long* h_point_bytes, long* h_fixed_bytes);
/* The three stages back to back with scale = vol / ngrid: d_vj (nset, nk, nao, nao) for the
 * k-mesh, or, with d_fband (nband, ngrid, nao) the AOs at band k-points on the same grid,
 * d_vj (nset, nband, nao, nao) at those (d_fband NULL: the k-mesh).  rho and v live in the
 * context's scratch arena. */
int fisdf_get_j_fft(fisdf_ctx* ctx, const void* d_f, long f_kstride, const int kmesh[3],
                    const int mesh[3], const double a[9], int nao, const void* d_dms, int nset,
                    double omega, const void* d_fband, int nband, void* d_vj);

/* ---- exact FFT-grid K (PySCF fft_jk.get_k_kpts, the dm form, exxdiv=None) ----------------------
 * For output k-points k1 (the k-mesh, or band points with their AOs f1 on the FFT grid), every k2
 * of the k-mesh, q = k2 - k1 and em[g] = exp(-i q.r_g):
 *   pair[m,l,g] = conj(f1[g,m]) f_k2[g,l] em[g]
 *   vR[m,l,g]   = ifft(coulG(q, omega) fft(pair[m,l,:]))[g] conj(em[g])
 *   u_s[l,g]    = sum_t D[s][k2][l,t] conj(f_k2[g,t])
 *   K[s][k1][m,n] += (vol/ngrid)/nk sum_g (sum_l vR[m,l,g] u_s[l,g]) f1[g,n]
 * D is any complex matrix, K is not symmetrised.  No atomics: repeated calls agree bit for bit,
 * and fisdf_get_k_fft's result does not depend on work_bytes.
 *
 * d_out[(m - m0) nao + l][g] = conj(f1[g,m]) f2[g,l] for m in [m0, m1): (m1 - m0) nao rows of
 * ngrid; d_f1, d_f2 (ngrid, nao), the same pointer or not. */
int fisdf_pair_density(fisdf_ctx* ctx, const void* d_f1, const void* d_f2, int ngrid, int nao,
                       int m0, int m1, void* d_out);
/* d_vk_k1[s][m][n] += scale sum_g t_s[m,g] f1[g,n] for m in [m0, m1), where
 * t_s[m,g] = conj(em[g]) sum_l conj(Z[(m - m0) nao + l][g]) u[s][l][g] and
 * conj(em[g]) = exp(+i frac(g).h_kd), frac the fftfreq fractions of the point's mesh indices
 * (h_kd NULL: no phase).  d_z (m1 - m0) nao rows of ngrid, d_u (nset, nao, ngrid), d_f1 (ngrid,
 * nao), d_vk_k1 (nset, nao, nao): rows outside [m0, m1) are left as they are.  The grid is split
 * into runs (fisdf_kfft_plan) whose partial blocks are summed in run order. */
int fisdf_exx_contract(fisdf_ctx* ctx, const void* d_z, const void* d_u, const void* d_f1,
                       const int mesh[3], const double* h_kd /*3 or NULL*/, int m0, int m1,
                       int nao, int nset, double scale, void* d_vk_k1);
/* The whole exact K: d_vk (nset, nk, nao, nao) for the k-mesh (d_fband NULL, nband 0), or with
 * d_fband (nband, ngrid, nao) the AOs at the nband band k-points h_kband (nband x 3, Cartesian,
 * 1/bohr, as fisdf_eval_ao_band takes them) d_vk (nset, nband, nao, nao) at those.  d_f (nk,
 * ngrid, nao) with k stride f_kstride, d_dms (nset, nk, nao, nao).  omega is an argument (the
 * context's setting is neither read nor changed).  work_bytes: the byte budget of the transform
 * rows, 0 = the default (512 MiB), never more than nao rows m are taken; below one row m (nao
 * rows of ngrid complex) is an error.  The argument checks come before the first launch; the FFT's
 * own checks of the mesh run when the first transform is reached, when only the arena has been
 * written.  Either way a refused call leaves d_vk untouched.  nao up to 32768, nset up to 1024.
 * Workspace: the context's arena (fisdf_kfft_plan's bytes).  Asynchronous on the context's
 * stream. */
int fisdf_get_k_fft(fisdf_ctx* ctx, const void* d_f, long f_kstride, const int kmesh[3],
                    const int mesh[3], const double a[9], int nao, const void* d_dms, int nset,
                    double omega, const void* d_fband, const double* h_kband, int nband,
                    long work_bytes, void* d_vk);
/* what fisdf_get_k_fft does for given sizes, from the host functions its launchers use (no
 * context, no device): rows m per chunk and chunks (both 0: the budget is below one row m), the
 * contraction's grid runs (points per run, runs), the pair kernel's AO tile width (8 or 32), the
 * contraction's n-tiles per thread (1, 2, 4; nao > 128 runs the last once per group of 128
 * columns, reading Z once per group), the bytes of one row m and the arena bytes of the call.
 * nao > 32768 or nset > 1024 is an error.  Any output may be NULL */
int fisdf_kfft_plan(int nao, long ngrid, int nset, long work_bytes, int* h_mc, int* h_nchunk,
                    int* h_run_len, int* h_nrun, int* h_pair_tw, int* h_exx_nn, long* h_row_bytes,
                    long* h_bytes);

/* ---- exact FFT-grid K, the occupied-orbital (low-rank) form ---------------------------------------
 * D[s][k2] = A B^H with A, B (nao, r), r = r[s][k2] (any dm has such factors: D = U S V^H gives
 * A = U S, B = V; occupied orbitals C with occupations n give A = C n, B = C).  With the orbitals on
 * the grid psiA_i(g) = sum_l f_k2[g,l] A[l,i], psiB_i(g) = sum_t f_k2[g,t] B[t,i], and em, q, coulG
 * and the output points k1 those of the dm form above:
 *   pair[m,i,g] = conj(f1[g,m]) psiA_i(g) em[g]
 *   vR[m,i,g]   = ifft(coulG(q, omega) fft(pair[m,i,:]))[g] conj(em[g])
 *   K[s][k1][m,n] += (vol/ngrid)/nk sum_g (sum_{i<r} vR[m,i,g] conj(psiB_i(g))) f1[g,n]
 * The transform rows of one k2 are the orbitals of all sets stacked, ni = sum_s r[s][k2] per row m
 * where the dm form has nao, set s owning the segment [seg[s], seg[s+1]).  No atomics: repeated
 * calls agree bit for bit, and fisdf_get_k_fft_lr's result does not depend on work_bytes.
 *
 * d_out[(m - m0) ni + i][g] = conj(f1[g,m]) psi[g,i] for m in [m0, m1): (m1 - m0) ni rows of
 * ngrid; d_f1 (ngrid, nao), d_psi (ngrid, ni) with leading dimension ld_psi >= ni. */
int fisdf_pair_density_lr(fisdf_ctx* ctx, const void* d_f1, int nao, const void* d_psi, int ni,
                          long ld_psi, int ngrid, int m0, int m1, void* d_out);
/* d_vk_k1[s][m][n] += scale sum_g t_s[m,g] f1[g,n] for m in [m0, m1), where
 * t_s[m,g] = conj(em[g]) sum_{i in [h_seg[s], h_seg[s+1])} conj(Z[(m - m0) ni + i][g]) u[i][g],
 * conj(em) as in fisdf_exx_contract.  d_z (m1 - m0) ni rows of ngrid, d_u (ni, ngrid) = conj(psiB)
 * transposed, d_f1 (ngrid, nao), d_vk_k1 (nset, nao, nao); h_seg nset + 1 offsets, h_seg[0] = 0,
 * not decreasing, h_seg[nset] = ni.  Every element of d_z is read once and meets one set; an
 * empty segment adds exact zeros.  Runs and their order as fisdf_exx_contract. */
int fisdf_exx_contract_lr(fisdf_ctx* ctx, const void* d_z, const void* d_u, const void* d_f1,
                          const int mesh[3], const double* h_kd /*3 or NULL*/, int m0, int m1,
                          int nao, int ni, const int* h_seg /*nset+1 offsets*/, int nset,
                          double scale, void* d_vk_k1);
/* The whole exact K from the factors: d_A, d_B (nset, nk, nao, rmax), of which only the first
 * h_rank[s nk + k] columns are ever read; every other argument, the output, the checks and the
 * workspace as fisdf_get_k_fft, with the transform rows of one row m now those of the fullest
 * k-point, imax = max_k sum_s h_rank[s nk + k] (work_bytes below imax rows of ngrid complex is an
 * error).  A rank below 0 or above rmax, or rmax < 1, is an error.  A k2 without orbitals launches
 * nothing: the first k2 that has some overwrites d_vk, and when no k2 has any d_vk is set to zero
 * (nothing is transformed then, so the mesh is not checked by the FFT). */
int fisdf_get_k_fft_lr(fisdf_ctx* ctx, const void* d_f, long f_kstride, const int kmesh[3],
                       const int mesh[3], const double a[9], int nao, const void* d_A,
                       const void* d_B, const int* h_rank /*nset*nk*/, int rmax, int nset,
                       double omega, const void* d_fband, const double* h_kband, int nband,
                       long work_bytes, void* d_vk);
/* what fisdf_get_k_fft_lr does for given sizes and imax >= 1 (host only): rows m per chunk =
 * min(nao, budget / (imax ngrid 16)) and chunks (both 0: the budget is below one row m), the
 * contraction's grid runs, the pair kernel's orbital tile width (8 or 32), the sets per launch of
 * the contraction (1 or 2: 32 or 16 rows m per workgroup) and its n-tiles per thread (1, 2, 4), the
 * bytes of one row m and the arena bytes of the call.  Any output may be NULL */
int fisdf_kfft_lr_plan(int nao, long ngrid, int nset, int imax, long work_bytes, int* h_mc,
                       int* h_nchunk, int* h_run_len, int* h_nrun, int* h_pair_tw, int* h_exx_sc,
                       int* h_exx_nn, long* h_row_bytes, long* h_bytes);

/* ---- exact FFT-grid four-index integrals (PySCF FFTDF.get_eri / ao2mo) ---------------------------
 * Orbitals on the FFT grid: a1 (ngrid, n1) at k1 and a2 (ngrid, n2) at k2, q = k2 - k1,
 * em[g] = exp(-i q.r_g), and npair pairs (a3_p (ngrid, n3), a4_p (ngrid, n4)):
 *   pair[i,j,g] = conj(a1[g,i]) a2[g,j] em[g]
 *   v[i,j,g]    = ifft(coulG(q, omega) fft(pair[i,j,:]))[g] conj(em[g])
 *   eri[p][i n2 + j][k n4 + l] = (vol/ngrid) sum_g v[i,j,g] conj(a3_p[g,k]) a4_p[g,l]
 * coulG drops G = 0 at q = 0, as in the exact K.  AO integrals are a_s = f_{k_s}, MO integrals
 * a_s = f_{k_s} C_s.  The transforms of (a1, a2) are paid once for all npair pairs (the (k3, k4)
 * that share (k1, k2)).  With Z the transformed rows as fisdf_get_k_fft forms them,
 * eri = (vol/ngrid) conj(Z) B^T with B[(p,k,l)][g] = conj(em[g]) conj(a3_p[g,k]) a4_p[g,l]: one
 * GEMM with deterministic split-K, no atomics; repeated calls agree bit for bit.
 *
 * d_out[((p n3 + k - r0) n4 + l)][g] = conj(em[g]) conj(a3_p[g,k]) a4_p[g,l] for the rows (p, k)
 * in [r0, r1) of the npair n3: (r1 - r0) n4 rows of ngrid.  h_d_a3, h_d_a4: host arrays of npair
 * device pointers, (ngrid, n3) and (ngrid, n4) at leading dimensions ld3 >= n3, ld4 >= n4 (only
 * the pairs the range meets are read).  conj(em[g]) = exp(+i frac(g).h_kd), frac the fftfreq
 * fractions of the point's mesh indices (h_kd NULL: no phase), formed in the kernel, not stored.
 * At most 8 pairs per launch, further launches beyond. */
int fisdf_pair34(fisdf_ctx* ctx, const void* const* h_d_a3, const void* const* h_d_a4, int npair,
                 int n3, int n4, long ld3, long ld4, const int mesh[3],
                 const double* h_kd /*3 or NULL*/, int r0, int r1, void* d_out);
/* The whole exact ERI: d_out (npair, n1 n2, n3 n4).  h_q = k2 - k1, Cartesian in 1/bohr (as
 * h_kband of fisdf_get_k_fft); d_a1 (ngrid, n1), d_a2 (ngrid, n2) and every pair's orbitals
 * contiguous.  omega is an argument (the context's setting is neither read nor changed).
 * work_bytes: the byte budget that holds for the transform rows and for B each, 0 = the default
 * (512 MiB); below one row i (n2 rows of ngrid complex) or one row (p, k) of B (n4 rows) is an
 * error.  The result does not depend on work_bytes or on how the pairs are grouped into calls
 * (the split-K depends on n1 n2, n3 n4 and ngrid alone).  The argument checks and the plan's
 * verdict come before the first launch; the FFT's own checks of the mesh run when the first
 * transform is reached, when only the arena has been written.  Either way a refused call leaves
 * d_out untouched.  n up to 32768, npair up to 65535, ngrid < 2^31.  Workspace: the context's
 * arena (fisdf_eri_fft_plan's bytes).  Asynchronous on the context's stream, no host
 * synchronisation inside. */
int fisdf_get_eri_fft(fisdf_ctx* ctx, const int mesh[3], const double a[9], const double h_q[3],
                      double omega, const void* d_a1, int n1, const void* d_a2, int n2,
                      const void* const* h_d_a3, const void* const* h_d_a4, int npair, int n3,
                      int n4, long work_bytes, void* d_out /* (npair, n1 n2, n3 n4) */);
/* what fisdf_get_eri_fft does for given sizes (host only, no context): rows i per chunk =
 * min(n1, W / (16 n2 ngrid)) and their chunks, rows (p, k) per B chunk = min(npair n3,
 * W / (16 n4 ngrid)) and their chunks (all four 0: the budget W is below one row of either kind),
 * whether B is built once before the row loop (one B chunk) or again inside every row chunk, the
 * builder's tile width (8 or 32, by n4), the GEMMs' split-K (doubled while tiles ks < 512 and
 * ngrid / (2 ks) >= 256, tiles those of the whole n1 n2 x n3 n4 product in 64 x 64) and the arena
 * bytes of the call.  A size out of range is an error.  Any output may be NULL */
int fisdf_eri_fft_plan(int n1, int n2, int n3, int n4, int npair, long ngrid, long work_bytes,
                       int* h_mc, int* h_nrow_chunks, int* h_bc, int* h_nb_chunks, int* h_b_once,
                       int* h_tw, int* h_ksplit, long* h_bytes);

/* ---- GTH pseudopotential and nuclear-attraction matrices (PySCF FFTDF.get_pp / get_nuc) ----------
 * With Omega the cell volume, N = ngrid, G the vectors of the mesh (fftfreq wrap), r_g the grid
 * points, f_k the Bloch AOs on the grid and SI_a(G) = exp(-i G.R_a):
 *   V_G = sum_a SI_a(G) v_a(|G|),  x = |G| rloc,
 *   v_a(G != 0) = -Z_a (4 pi / G^2) e^{-x^2/2} + (2 pi)^{3/2} rloc^3 e^{-x^2/2}
 *                 [c1 + c2 (3 - x^2) + c3 (15 - 10 x^2 + x^4) + c4 (105 - 105 x^2 + 21 x^4 - x^6)]
 *   v_a(G = 0)  = 2 pi Z_a rloc^2 + (2 pi)^{3/2} rloc^3 (c1 + 3 c2 + 15 c3 + 105 c4)
 *   (a bare nucleus: -Z_a 4 pi / G^2, and 0 at G = 0: the formulas above at rloc = 0)
 *   v(r_g) = (1/Omega) sum_G V_G e^{i G.r_g}
 *   Vloc_k[m,n] = (Omega/N) sum_g conj(f_k[g,m]) Re v(r_g) f_k[g,n]
 * and, for the projector p = (a, l, i, mm), i < n_l, K = k + G, x = |K| r_l:
 *   beta_p(G; k) = e^{-i K.R_a} P_i^l(|K|) S_{l,mm}(K)
 *   P_i^l(K) = q_{l,i}(x) pi^{5/4} r_l^{l + 3/2} e^{-x^2/2}   (q: the table of DESIGN 3.13)
 *   S_{l,mm}: the real solid harmonics |K|^l Y_{l,mm} of fisdf_eval_ao
 *   c[p,m] = sum_G conj(beta_p(G; k)) (1/N) sum_g e^{-i K.r_g} f_k[g,m]
 *   Vnl_k[m,n] = sum_{a,l,mm} sum_{ij} conj(c[(a,l,i,mm),m]) h_l[i,j] c[(a,l,j,mm),n]
 * c is formed as sum_g t_p(r_g) e^{-i k.r_g} f_k[g,m] with t_p = (1/N) fft3d(conj beta_p): the
 * projector rows are transformed, the AOs are read where they lie.  No atomics: repeated calls
 * agree bit for bit, and fisdf_get_pp's result does not depend on work_bytes.
 *
 * One atom of the table.  A bare nucleus (bare != 0) has charge z and nothing else is read. */
typedef struct fisdf_pp_atom {
  double r[3];      /* position, bohr */
  double z;         /* Z_ion of the pseudopotential, or the nuclear charge */
  double rloc;
  double c[4];      /* c1..c4, the first nexp are read */
  double rl[4];     /* r_l of channel l */
  double h[4][9];   /* h_l, row-major 3 x 3, the leading n[l] x n[l] block is read */
  int nexp;         /* <= 4 */
  int bare;
  int nl;           /* angular-momentum channels l = 0..nl-1, <= 4 */
  int n[4];         /* projectors of channel l, <= 3 (0: none) */
  int reserved;
} fisdf_pp_atom;
/* projector rows of the table: sum over atoms and channels of n[l] (2 l + 1); a bare atom has
 * none.  A negative value: the table is refused (nl > 4, n[l] > 3, nexp > 4 or a negative count,
 * rloc <= 0 or r_l <= 0 where read) */
int fisdf_pp_nproj(const fisdf_pp_atom* h_atoms, int natm);
/* d_vg[G] = V_G over the mesh (ngrid c128) */
int fisdf_vloc_g(fisdf_ctx* ctx, const int mesh[3], const double a[9],
                 const fisdf_pp_atom* h_atoms, int natm, void* d_vg);
/* d_rows[p][G] = conj(beta_p(G; k)) for the projectors of atoms [a0, a1) at the k-point h_k
 * (Cartesian, 1/bohr): rows in table order (atom, l, i, mm), each of ngrid */
int fisdf_gth_projectors(fisdf_ctx* ctx, const int mesh[3], const double a[9], const double h_k[3],
                         const fisdf_pp_atom* h_atoms, int natm, int a0, int a1, void* d_rows);
/* d_c[p][m] = scale sum_g d_t[p][g] exp(-i frac(g).h_kd) d_f[g][m]: d_t (np, ngrid), d_f (ngrid,
 * nao), d_c (np, nao); frac the fftfreq fractions of the point's mesh indices (h_kd NULL: no
 * phase), formed in the kernel.  The grid is split into runs (fisdf_pp_plan) whose partial blocks
 * are summed in run order; the runs depend on ngrid alone */
int fisdf_pp_overlap(fisdf_ctx* ctx, const void* d_t, int np, const void* d_f, int nao,
                     const int mesh[3], const double* h_kd /*3 or NULL*/, double scale, void* d_c);
/* d_out[k] (nao, nao) = Vloc_k (+ Vnl_k when with_nonlocal) for the nk k-points h_kpts (nk x 3,
 * Cartesian, 1/bohr) whose AOs on the grid are d_f (nk, ngrid, nao) with k stride f_kstride.
 * get_nuc is this with a table of bare nuclei and with_nonlocal = 0.  At a k-point with
 * sum |k_d| < 1e-9 the imaginary part is set to zero.  work_bytes: the byte budget of one
 * k-point's projector rows, 0 = the default (512 MiB); rows beyond it are taken in chunks of whole
 * atoms, and an atom whose own rows exceed it is an error.  Every check of the table, the sizes
 * and the mesh (the FFT's own rule included) comes before the first launch: a refused call leaves
 * d_out untouched.  Workspace: the context's arena (fisdf_pp_plan's bytes).  Asynchronous. */
int fisdf_get_pp(fisdf_ctx* ctx, const void* d_f, long f_kstride, int nk, const double* h_kpts,
                 const int mesh[3], const double a[9], int nao, const fisdf_pp_atom* h_atoms,
                 int natm, int with_nonlocal, long work_bytes, void* d_out);
/* what fisdf_pp_overlap and fisdf_get_pp do for given sizes (host only, no context): the grid runs
 * of the overlap (points per run, runs), its AO tiles (of 32) and, for np projector rows, its
 * projector tiles (of 16); the atom chunks of the table under work_bytes (0: no projectors, or an
 * atom beyond the budget; a refused table is an error) and the most rows of a chunk; the arena bytes of fisdf_get_pp with nk
 * k-points.  h_atoms may be NULL (natm 0): no chunks, np as given.  Any output may be NULL */
int fisdf_pp_plan(int nao, long ngrid, int nk, int np, const fisdf_pp_atom* h_atoms, int natm,
                  int with_nonlocal, long work_bytes, int* h_run_len, int* h_nrun, int* h_mtiles,
                  int* h_ptiles, int* h_nchunk, int* h_chunk_rows, long* h_bytes);

/* ---- ISDF 4-index integrals (get_eri / ao2mo surface) --------------------------
 * eri[i*n2+j][k*n4+l] = sum_IJ W_q[I,J] conj(A1[I,i]) A2[I,j] conj(A3[J,k]) A4[J,l] with
 * A_s = X_{kidx[s]} C_s, q = k2 - k1 (fftdf-with-k-lstsq.py:221-232).  d_Wq: the (nip,nip)
 * W of that q; h_dC: host array of 4 DEVICE pointers to (nao, nmo[s]) MO coefficients, or
 * NULL (or NULL entries) for AO integrals (nmo[s] is then not read).  d_out: (n1*n2, n3*n4) c128.
 * W_q is taken as given: any complex matrix, nothing Hermitian assumed.
 * kidx[s] selects X_{kidx[s]} inside d_X (nk, nip, nao).  The entry is not told nk, so it cannot
 * check the upper end: 0 <= kidx[s] < nk is the caller's responsibility (the mirror maps k-points
 * to indices and checks momentum conservation, isdf.py _kidx / _eri_isdf); a negative index is
 * refused.  Also refused on the host, before the workspace is asked for and with d_out untouched:
 * a null d_X, d_Wq, kidx or d_out, nip or nao below 1, a C_s given with nmo NULL or nmo[s] < 1,
 * n1*n2 or n3*n4 beyond INT_MAX (they are GEMM dimensions). */
int fisdf_get_eri(fisdf_ctx* ctx, const void* d_X, int nip, int nao, const int kidx[4],
                  const void* d_Wq, const void* const* h_dC, const int nmo[4], void* d_out);

/* ---- building blocks exported for tests / other callers -------------------- */
/* C[b] = alpha op(A[b]) op(B[b]) + beta C[b]; op: 0 N, 1 T, 2 conj, 3 conj-transpose */
int fisdf_zgemm(fisdf_ctx* ctx, int opA, int opB, int M, int N, int K, const double alpha[2],
                const void* d_A, long lda, long strideA, const void* d_B, long ldb, long strideB,
                const double beta[2], void* d_C, long ldc, long strideC, int batch, int ksplit);
/* the same with the fit's arithmetic modes (no split-K): 1 = Im op(A) taken as zero, 2 = only
 * Re C formed, 4 = op(A) lower triangular (op N), 8 = op(A) = A^H upper triangular (op C), 5 =
 * 4 | 1; NN products with N >= 512 run on the 64 x 128-tile kernel */
int fisdf_zgemm_mode(fisdf_ctx* ctx, int opA, int opB, int M, int N, int K, const double alpha[2],
                     const void* d_A, long lda, long strideA, const void* d_B, long ldb,
                     long strideB, const double beta[2], void* d_C, long ldc, long strideC,
                     int batch, int mode);
/* everything the library's GEMM takes, for tests of its dispatch: split-K (workspace from the
 * context's arena) together with a mode, and the fused epilogues: epi 0 none, 2 = C = alpha acc
 * with streaming stores, 4 = C = (alpha acc)^2 elementwise, 5 = C = Re(alpha acc) written as
 * doubles (d_C is a double*, ldc in doubles, one batch), 6 = C = d_aux * Re(alpha acc) + 0i with
 * d_aux real (doubles, row stride ldaux).  The epilogues take beta = 0 and no split-K.  h_mon
 * (host, may be NULL) receives max |Im(alpha acc)| of epilogues 4, 5, 6 (0 otherwise); it is kept
 * in a device word of its own, so what fisdf_max_imag reports does not change. */
int fisdf_zgemm_ex(fisdf_ctx* ctx, int opA, int opB, int M, int N, int K, const double alpha[2],
                   const void* d_A, long lda, long strideA, const void* d_B, long ldb,
                   long strideB, const double beta[2], void* d_C, long ldc, long strideC,
                   int batch, int ksplit, int mode, int epi, const void* d_aux, long ldaux,
                   double* h_mon);
/* C[b] = alpha A[b] A[b]^H + beta C[b] with real alpha, beta.  batch == 1 and beta == 0: the
 * HERK with split-K and mode 0 (full) or 2 (C = alpha Re(A A^H)); anything else: the batched
 * HERK (lower tiles + mirror of a Hermitian C), which has no split-K and mode 0 only (an error
 * otherwise) */
int fisdf_herk_ex(fisdf_ctx* ctx, int n, int K, double alpha, const void* d_A, long lda,
                  long strideA, double beta, void* d_C, long ldc, long strideC, int batch,
                  int ksplit, int mode);
/* C = alpha A A^H (A: n x K, lda; C: n x n, ldc), Hermitian: lower tiles + mirror */
int fisdf_herk(fisdf_ctx* ctx, int n, int K, double alpha, const void* d_A, long lda, void* d_C,
               long ldc, int ksplit);
/* forward 3-D FFT (numpy fftn sign, unnormalised) of `rows` rows of n0*n1*n2 points */
int fisdf_fft3d(fisdf_ctx* ctx, const void* d_in, void* d_out, int rows, const int mesh[3]);
/* the fit's transform of a self-conjugate q: rows pre-multiplied by exp(-i f.kd) (f: fftfreq
 * fractions; kd may be NULL), m (or NULL) = 2 k_q in mesh units: the input is real up to that
 * phase, out(j') = conj(out(j)) for j' = -j - m, and only the prefix planes
 * j0 < #{i0 : i0 <= (-i0 - m0) mod n0} of d_out are written (register meshes; other meshes
 * write every plane).  in_real: d_in holds rows of doubles (same strides), d_in != d_out,
 * register meshes only (an error otherwise) */
int fisdf_fft3d_paired(fisdf_ctx* ctx, const void* d_in, void* d_out, int rows, const int mesh[3],
                       const double kd[3], const int m[3], int in_real);
/* everything the library's FFT takes, for tests of its dispatch: rows of the input at stride in_ld
 * (complex elements; doubles with in_real), d_rowidx (device, `rows` ints, or NULL) the input row
 * each output row is gathered from, output rows at stride out_ld, h_kd (3, or NULL) the phase
 * exp(-i f.kd) applied before the transform, d_weight (device, n0*n1*n2 doubles, or NULL)
 * multiplied into the result, h_plane_base / h_plane_ld (n0 each, or both NULL) sliced input:
 * plane i0 of input row r at d_in + h_plane_base[i0] + r * h_plane_ld[i0] (in_ld unused; the
 * table is uploaded to a buffer of this call, which then waits for the stream before it frees
 * it), h_m / in_real as fisdf_fft3d_paired.  d_in == d_out (equal strides, no gather) transforms
 * in place.  *h_path (may be NULL) = the kernels that ran: 0 register kernels, 1 register kernels
 * with Hermitian pairing, 2 LDS plane kernel + axis-0 pass, 3 three axis passes, + 16 when a
 * pass ran as the radix-7/11/13 instantiation; -1 when nothing ran (rows = 0, or an error).  A
 * call the library cannot do fails before it launches anything. */
int fisdf_fft3d_ex(fisdf_ctx* ctx, const void* d_in, long in_ld, const int* d_rowidx, void* d_out,
                   long out_ld, int rows, const int mesh[3], const double* h_kd,
                   const double* d_weight, const long* h_plane_base, const long* h_plane_ld,
                   const int* h_m, int in_real, int* h_path);
/* sqrt(coulG(k+G) * scale) (or without sqrt), PySCF get_coulG(exxdiv=None) restated */
int fisdf_coulg(fisdf_ctx* ctx, const int mesh[3], const double a[9], const double k[3],
                double scale, int take_sqrt, double* d_w);
/* minimum-norm operator of one Hermitian PSD n x n matrix (the fit's FISDF_FIT_LSTSQ/SVD path):
 * rank-revealing pivoted Cholesky (cut tol_rel * max diag) then M = (P L)^+ (n x n, rows < rank
 * valid, columns in pivot order h_piv), so x4^+ ~ P M^H M P^T; d_Q (n x rank) and d_Rinv
 * (rank x rank), if not NULL, receive the thin QR factors P L = Q R; synchronous */
int fisdf_min_norm_operator(fisdf_ctx* ctx, const void* d_A, int n, double tol_rel, void* d_M,
                            void* d_Q, void* d_Rinv, int* h_piv /* n */, int* h_rank);
/* batched pivoted Cholesky (pivots + ranks to host; synchronous) */
int fisdf_pivoted_cholesky(fisdf_ctx* ctx, const void* d_A, int n, int batch, int rmax,
                           double tol_rel, int* h_piv /* batch*rmax */, int* h_rank /* batch */);
/* the fit's unpivoted blocked Cholesky of batch Hermitian PD n x n matrices, in place (lower
 * triangle = L on return; 64-column blocks, the diagonal blocks factored and inverted in LDS);
 * h_fail[b] = 1 when a pivot fell below tol_rel * max(diag) (the fit then refactors with
 * pivoting).  synchronous */
int fisdf_cholesky(fisdf_ctx* ctx, void* d_A, int n, int batch, double tol_rel, int* h_fail);
/* L^{-1} of batch lower-triangular n x n matrices by the factor stage's block-row substitution
 * (the operator the fit's triangular GEMM applies); a matrix's result does not depend on the
 * batch it is computed in */
int fisdf_tri_inverse(fisdf_ctx* ctx, const void* d_L, int n, int batch, void* d_Linv);

/* ---- the factor-and-solve chain piece by piece, for tests of its dispatch.  Every pointer named
 * d_ is device memory, every call is synchronous and fails before it launches anything when it
 * cannot run. ---- */
/* everything the pivoted Cholesky takes: batch Hermitian PSD n x n matrices at d_A (row stride
 * lda, batch stride sA >= n*lda, complex elements), at most rmax pivots per matrix, stop when the
 * largest residual diagonal is not above max(tol_rel > 0 ? tol_rel * m : n * eps * m, tol_abs),
 * m = max diag.  d_L (batch, n, rmax): column j = the factor's column of pivot j, rows in the
 * matrix's own order; columns >= rank unspecified.  d_piv (batch, rmax): entries >= rank are left
 * as they were.  d_rank (batch).  *h_path (may be NULL): 0 = panels of 32 pivots in one
 * workgroup's registers (n <= 1024), 1 = one step per pivot */
int fisdf_pivoted_cholesky_ex(fisdf_ctx* ctx, const void* d_A, long lda, long sA, int n, int batch,
                              int rmax, double tol_rel, double tol_abs, void* d_L, int* d_piv,
                              int* d_rank, int* h_path);
/* d_Lp[b] (rpad x rpad, rpad <= rmax) = the rows of d_L[b] (n x rmax) in pivot order, lower
 * triangle of the leading rank[b] x rank[b] block, the identity beyond the rank, zero elsewhere */
int fisdf_gather_lp(fisdf_ctx* ctx, const void* d_L, int n, int rmax, const int* d_piv,
                    const int* d_rank, int rpad, void* d_Lp, int batch);
/* X = L^{-1} B (lower = 1) or L^{-H} B (lower = 0) by the fit's blocked substitution (64-row
 * blocks, the diagonal-block inverses built here as the factor stage does).  L: the leading r x r
 * of d_Lp (row stride ldl, batch stride sL); d_B (r x ncol, ldb, sB) is overwritten; d_X (ldx,
 * sX).  a_real: Im L is taken as zero */
int fisdf_trsm_blocked_ex(fisdf_ctx* ctx, int lower, const void* d_Lp, long ldl, long sL, int r,
                          void* d_B, long ldb, long sB, void* d_X, long ldx, long sX, int ncol,
                          int batch, int a_real);
/* X <- L^{-1} X in place by the factor stage's merged block-row substitution: the block-row
 * operator of d_Lp (batch of r x r, row stride r, batch stride sL) is built, then applied to d_X
 * (r x ncol, row stride ld, batch stride sX).  lower_rhs: X is lower triangular (block row b is
 * computed for its columns < b1 only).  use_work: split-K with a workspace of work_elems complex
 * elements (batches that do not fit run in sub-batches; fewer than one matrix's partials is an
 * error and leaves d_X as it was).  h_rows (may be NULL; rows_cap >= (r + 63) / 64 rows of 6
 * ints): per block row b0, m, b1, columns, split-K, matrices per launch */
int fisdf_trsm_merged_ex(fisdf_ctx* ctx, const void* d_Lp, long sL, int r, void* d_X, long ld,
                         long sX, int ncol, int batch, int lower_rhs, int use_work,
                         long work_elems, int* h_rows, int rows_cap);
/* d_W[b] (nip x nip) = 0, then d_W[b][piv[s]][piv[t]] = d_Wpp[b][s][t] (row stride ldw, batch
 * stride sW) for s, t < rank[b] <= rmax; d_piv rows are nip apart (the factor stage's layout) */
int fisdf_scatter_w(fisdf_ctx* ctx, const void* d_Wpp, int ldw, long sW, int rmax,
                    const int* d_piv, const int* d_rank, void* d_W, int nip, int batch);
/* d_B[b] = d_A[b]^H for batch n x n matrices (row stride n, batch stride sA for both) */
int fisdf_conj_transpose(fisdf_ctx* ctx, const void* d_A, int n, long sA, void* d_B, int batch);
/* what the chain does for given sizes, from the host functions its launchers use (no context, no
 * device): the pivoted Cholesky's path and panel width for an n x n matrix; the merged
 * substitution's partition of n rows (h_nblk block rows, the first of *h_s0 rows) and, per block
 * row, 8 ints in h_rows (rows_cap rows; may be NULL): b0, m, b1, then split-K and matrices per
 * launch for a full right-hand side of ncol columns, then columns, split-K and matrices per launch
 * for a lower-triangular one, all for a batch of `batch` with a workspace of work_elems complex
 * elements (< 0: none; matrices per launch 0 = the workspace is too small); the workspace that
 * lets the whole batch run in one launch per row with n columns; the (rows per thread, pivots per
 * panel) of the real selection panel kernel for an n x n Gram (0, 0 beyond n = 4096).  Any output
 * may be NULL */
int fisdf_factor_plan(int n, int ncol, int batch, long work_elems, int* h_pchol_path,
                      int* h_pchol_nb, int* h_nblk, int* h_s0, int* h_rows, int rows_cap,
                      long* h_split_work_elems, int* h_sel_rpt, int* h_sel_nb);

/* ---- the separable k-mesh transforms piece by piece (the y build, x4, get_k's pair, the Bloch
 * AO), for tests of their dispatch.  Every pointer named d_ is device memory, every call with a
 * context is synchronous and fails before it launches or copies anything when it cannot run, its
 * output left as it was. ---- */
/* what the k-mesh transforms do for a k-mesh (axes >= 1), from the host functions their launchers
 * use (no context, no device).  h_route (3): the route of a transform over ncol columns (0 the
 * register kernels: a k-mesh of the compiled list, ncol < 2^31; 1 the LDS kernel; 2 refused: an
 * axis above 16, more than 160 KB of LDS or 2^31 tiles), then the LDS kernel's columns per tile
 * (64, 32, 16 or 8) and its dynamic LDS bytes (both 0 on route 0 or with an axis above 16).
 * *h_half_count: the k stored under time reversal (k <= -k); h_runs (runs_cap pairs) / *h_nruns:
 * those k as [begin, end) runs.  h_fused (4): whether the fused y kernel takes (kmesh, nao), its
 * chunk A and chunk B slot counts and its K chunks of 28 per slot (all 0 when it does not);
 * h_slots (48): the k of every slot, chunk A's then chunk B's, -1 beyond; h_fused_bytes (2): the
 * fused kernel's dynamic LDS bytes and the workspace bytes y_fused asks for (nip, nao, m).  Any
 * output may be NULL */
int fisdf_kmesh_plan(const int kmesh[3], long ncol, int nao, int nip, int m, long* h_route,
                     int* h_half_count, int* h_runs, int runs_cap, int* h_nruns, int* h_fused,
                     int* h_slots, long* h_fused_bytes);
/* y_q = Phi^T (Re(Phi FX))^2 for the ascending q-list h_qs (nq entries; uploaded by the call):
 * d_FX (nk rows of ncol columns; half: only the rows of the k <= -k, the others taken as
 * conj(FX[-k])), column c = I * m + g written to d_yT[slot * qs + I * Is + goff + g] (conj_out:
 * conjugated; register route only).  *h_mon = max |Im(Phi FX)|, *h_route as h_route[0] of
 * fisdf_kmesh_plan (-1: nothing ran) */
int fisdf_kmesh_y_ex(fisdf_ctx* ctx, const void* d_FX, long ncol, const int kmesh[3],
                     const int* h_qs, int nq, int m, void* d_yT, long qs, long Is, long goff,
                     int half, int conj_out, double* h_mon, int* h_route);
/* the fused y build under time reversal: d_X (nk, nip, nao), d_F (k stride fks, m rows of nao),
 * rmask: the q (bits) stored as doubles in the first half of their slot (bits outside the q-list
 * are ignored).  *h_handled = 0: the fused kernel does not take (kmesh, nao); nothing was written.
 * The workspace comes from the context */
int fisdf_y_fused_ex(fisdf_ctx* ctx, const void* d_X, int nip, int nao, const void* d_F, long fks,
                     int m, const int kmesh[3], const int* h_qs, int nq, void* d_yT, long qs,
                     long Is, long goff, unsigned long long rmask, int* h_handled);
/* the same, streamed: rows [0, nip) of y in blocks of `rows` (a multiple of 16, 16..1024), block
 * rows gathered from d_x0 (nk, ng0, nao) through h_piv (nip entries in [0, ng0)); two_streams: odd
 * blocks on a second stream.  The progress word is set to done on the context's stream before the
 * first launch.  *h_err: the device flag of a wait past its bound */
int fisdf_y_fused_stream_ex(fisdf_ctx* ctx, const void* d_x0, int ng0, int nao, const int* h_piv,
                            int nip, int rows, const void* d_F, long fks, int m,
                            const int kmesh[3], const int* h_qs, int nq, void* d_yT, long qs,
                            long Is, long goff, unsigned long long rmask, int two_streams,
                            int* h_handled, int* h_err);
/* get_k's pair in place on d_B (nk rows of ncol columns): rho_s = Phi rho_k, V_s = W_s Re(rho_s)
 * (d_Ws: doubles, row s at s * ws_Rstride), V_k = Phi^T V_s.  use_reg = 1: the register kernel
 * where the k-mesh has one (*h_handled = 1), else, and with use_reg = 0, the two dense Phi GEMMs
 * (Phi from the lattice h_a).  *h_mon = max |Im rho_s| */
int fisdf_k_wsrho_ex(fisdf_ctx* ctx, void* d_B, long ncol, const int kmesh[3], const double h_a[9],
                     const void* d_Ws, long ws_Rstride, int use_reg, double* h_mon,
                     int* h_handled);
/* the tail of fisdf_eval_ao: d_chi[k][c] = sum_R exp(2 pi i sum_a r_a k_a / n_a) d_F[R][c] (d_F
 * doubles, nk rows of ncol); *h_route: 0 the register kernel, 1 one thread per (k, column) */
int fisdf_bloch_dft_ex(fisdf_ctx* ctx, const void* d_F, long ncol, const int kmesh[3], void* d_chi,
                       int* h_route);
/* the tail of fisdf_eval_ao_band: d_chi[k][c] = sum_t d_ph[t * nkb + k] d_F[t][c], t < nT */
int fisdf_bloch_band_ex(fisdf_ctx* ctx, const void* d_F, long ncol, int nT, const void* d_ph,
                        int nkb, void* d_chi);

/* ---- the interpolation-point selection piece by piece, for tests of its dispatch.  Every pointer
 * named d_ is device memory, every call with a context is synchronous and fails before it launches
 * or copies anything when it cannot run, its outputs left as they were. ---- */
/* what the selection does for an n x n Gram and rmax pivots (1 <= rmax <= n) on a device of ncu
 * compute units, from the host functions its launchers use (no context, no device).  lds_cols and
 * wgs: 0 = the production values, else what FISDF_SEL_LDS_COLS and FISDF_SEL_WGS would set.
 * *h_mode: the kernel tried first when no switch is set (0 batch: from 800 pivots on, 1 coop); a
 * kernel that does not take the sizes hands on to the next: batch, coop, panel, then the generic
 * pivoted Cholesky.
 * h_batch (4): taken or not, the rule that refused it (0 none, 1 n < 64, 2 n > 4096, 3 rmax > 4096,
 *   4 more workgroups than ncu, 5 the owner's LDS above 150 KB, 6 the scratch beyond the n*n work
 *   area), the grid (owners + leader), rows per owner; *h_batch_lds: dynamic LDS bytes.
 * h_coop (7): taken or not, the rule that refused it (0 none, 1 n < 64, 2 no workgroup, 3 fewer
 *   than 16 columns of the split form fit, 4 LDS above 150 KB, 5 more than 64 rows per workgroup,
 *   6 the scratch beyond the work area), split form or not, G workgroups, RW rows per workgroup,
 *   K columns of the owned rows in LDS, tpr threads per row; *h_coop_lds: dynamic LDS bytes.
 *   Entries computed after the refusing rule are 0.
 * h_panel (2): rows per thread and pivots per panel of the register-panel kernel (0, 0 beyond
 *   n = 4096); *h_pchol_path: the generic path's (0 blocked, 1 per step).  Any output may be NULL */
int fisdf_select_plan(int n, int rmax, int ncu, int lds_cols, int wgs, int* h_mode, int* h_batch,
                      long* h_batch_lds, int* h_coop, long* h_coop_lds, int* h_panel,
                      int* h_pchol_path);
/* fisdf_select_pivots (nip_max <= ng0) with the switches as arguments.  mode: -1 as
 * fisdf_select_pivots (the default rule and FISDF_SEL_MODE), 0 start at the batch kernel, 1 at the
 * cooperative one, 2 the register panels only (FISDF_SEL_COOP then unread too); lds_cols, wgs as
 * above, FISDF_SEL_LDS_COLS and FISDF_SEL_WGS unread.  h_perm: entries from *h_npiv on are left as they were.  h_info (6): what
 * produced the pivots, which a refused kernel makes differ from the mode asked for: the kernel
 * (0 batch, 1 coop, 2 coop in its split form, 3 register panels, 4 generic blocked, 5 generic per
 * step), G, RW, K, tpr as in fisdf_select_plan (batch: the grid, 16, rmax, 0; panels: 1, rows per
 * thread, pivots per panel, 0; generic: 0, 0, panel width, 0), and the passes (2: the first one
 * reported a stalled step and the selection was redone without the co-resident kernels) */
int fisdf_select_pivots_ex(fisdf_ctx* ctx, const void* d_x2, int nk, int ng0, int nip_max,
                           double tol, int mode, int lds_cols, int wgs, int* h_perm, int* h_npiv,
                           int* h_full_rank, int* h_info);
/* fisdf_select_gram with an optional k-mesh (NULL, or axes whose product is nk) and the
 * time-reversal fold as an argument: fold = 1 (needs the k-mesh, q0 = 0, q1 = nk) sums the
 * representatives k <= -k, a paired one scaled by sqrt(2).  h_info (3, may be NULL): the k-points
 * summed, the permute launches (64 k each under the fold) and the HERK split-K.  The _plan form
 * gives h_info alone (no context, no device) */
int fisdf_select_gram_ex(fisdf_ctx* ctx, const void* d_x0, const int* kmesh, int fold, int nk,
                         int q0, int q1, int ng0, int nao, void* d_x2, int* h_info);
int fisdf_select_gram_plan(const int* kmesh, int fold, int nk, int q0, int q1, int ng0, int nao,
                           int* h_info);

#ifdef __cplusplus
}
#endif

#endif /* FISDF_H */
