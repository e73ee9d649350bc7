// C-ABI of libfisdf.so (include/fisdf.h): orchestration of the HIP kernels that
// replace the reference's fftisdf.py hot path.  Each entry cites the reference lines
// it stands in for.
#include "../../include/fisdf.h"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "common.h"
#include "linalg.h"

namespace fisdf {

static thread_local std::string g_last_error;
// the context the calling thread is working on (set by the entry points' guards): a failure is
// recorded in it too, so fisdf_last_error(ctx) reports that context's own last failure.  Only a
// context that is still alive is written (one destroyed on another thread must not
// be), and fisdf_create clears it, so its failures go to fisdf_last_error(NULL) only
static thread_local fisdf_ctx* t_cur_ctx = nullptr;
static std::mutex g_live_mu;
static std::set<const fisdf_ctx*> g_live;
void set_ctx_error(fisdf_ctx* c, const std::string& msg);
void set_error(const std::string& msg) {
  g_last_error = msg;
  if (!t_cur_ctx) return;
  std::lock_guard<std::mutex> lk(g_live_mu);
  if (g_live.count(t_cur_ctx)) set_ctx_error(t_cur_ctx, msg);
}

LaunchEvents& launch_events() {
  static thread_local LaunchEvents ev;
  return ev;
}

}  // namespace fisdf

using namespace fisdf;

// default relative pivot cut of the x4_q factorisation (fisdf_build_opts.fit_tol, the rank of a
// rank-deficient x4_q): 4.2e-15 ~ 19 eps is where the pivoted Cholesky's ranks reproduce gelsy's
// (fftisdf.py:108: QRCP + incremental condition estimate at rcond = eps) in the reference demo's
// regime (C2 at c0 = 1e4, every x4_q rank-deficient): per-q ranks 0-13 from gelsy's, J/K within
// 0.78 / 0.71 of gelsy's own rcond band; the round-4 cut 1e-14 sat 27-37 ranks below it, at
// 1.38 / 0.97 of the band (tests/experiments/rank_rule_c2.py, profiles/r05/rank_regime/)
constexpr double kFitTolDefault = 4.2e-15;

struct fisdf_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // grow-only scratch arena (sequential use on `stream`)
  void* arena = nullptr;
  size_t arena_size = 0;
  // phase matrices Phi (nimg x nk) keyed by kmesh + lattice
  std::map<std::vector<double>, cplx*> phase_cache;
  // per-q factors of x4_q (fisdf_factor_x4)
  std::vector<int> f_qs;  // the factored q (ascending), slot i <-> q = f_qs[i]
  std::vector<char> f_real;  // slot factored as real (self-conjugate q, kmesh given)
  // per (mesh, lattice, k_q): device list of G with asymmetric Coulomb weight (asym_list)
  struct Asym { int* idx = nullptr; int n = 0; double* f = nullptr; };
  std::map<std::vector<double>, Asym> asym_cache;
  // fisdf_set_half_grid: a self-conjugate q is fitted on half the G (its Hermitian pairs), -1:
  // environment FISDF_HALF_G (default on)
  int half_grid = -1;
  // per (mesh, k-mesh, lattice, q, omega): sqrt(coulG(k_q + G) vol / N^2) of the fit, computed
  // once (the timed steps of a repeated build reuse them)
  std::map<std::vector<double>, double*> wt_cache;
  int f_nk = 0, f_nip = 0, f_nb = 64;
  cplx* f_L = nullptr;      // (nk, nip, nip) raw left-looking factor (row order)
  cplx* f_Lp = nullptr;     // (nk, nip*nip) pivot-order factor, ld = rank_q
  cplx* f_Linv = nullptr;   // (nk, nblk*nb*nb)
  cplx* f_Q = nullptr;      // (nk, nip, nip) block-row operator of trsm_merged_batched (build_trsm_q)
  cplx* f_Li = nullptr;     // (nk, nip, nip) L^{-1} (pivot order) = trsm_merged_batched on the identity
  cplx* f_ksw = nullptr;    // split-K partials of that substitution (trsm_split_work_elems)
  long f_ksw_elems = 0;
  cplx* f_x4s = nullptr;    // (nk, nip, nip) staged x4_q of the factored slots
  int* f_fail_pinned = nullptr;  // unpivoted path: per-slot failure flags (host, pinned)
  int* f_qr_pinned = nullptr;    // factored q-list + real flags (2 nk ints, pinned) and device copy
  int* f_qr_dev = nullptr;
  double f_tol = kFitTolDefault;
  bool f_check_fail = false, f_used_pivoted = false;
  int f_cap_nk = 0, f_cap_nip = 0;  // shape the factor buffers were allocated for
  int force_pivoted = -1;  // fisdf_set_pivoted_fit; -1: environment FISDF_PIVOTED_FIT
  // fisdf_set_fit_mode: FISDF_FIT_LSTSQ (gelsy semantics: the unique solution of a full-rank
  // x4_q, the minimum-norm one of a rank-deficient x4_q), FISDF_FIT_SVD (rank-revealing factor
  // and the minimum-norm operator on every q), FISDF_FIT_BASIC (basic solution, round-1 path)
  int fit_mode = 0;
  cplx* f_M = nullptr;          // (nk, nip, nip) minimum-norm operators A^+ (rows < rank)
  std::vector<char> f_cod;      // slot fitted through its minimum-norm operator
  // the fit's pipelined-FFT ring (Yhat slots, nip rows each), a grow-only buffer of its own
  cplx* f_ring = nullptr;
  size_t f_ring_bytes = 0;
  // grow-only temporaries instead of the stream-ordered pool (hipMallocAsync): on the HIP 7.2
  // runtime a block freed on one stream was handed to another stream's allocation while the
  // first still used it (torch-free C-ABI build: the pivoted factor's ranks corrupted by the
  // Coulomb weights computed beside it on the FFT stream).  ws_main: the main stream's;
  // ws_side_a / ws_side_b: the factorisation's (side stream)
  struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
  } ws_main, ws_side_a, ws_side_b, ws_x4;  // ws_x4: x2_k of an x4 built on the side stream
  int* f_nip_dev = nullptr;     // device copy of nip (scatter of a full W_PP)
  int lanes = 0;           // fisdf_set_fit_lanes; 0: environment FISDF_FIT_LANES / default
  bool time_reversal = false;  // fisdf_set_time_reversal: fx_{-k} = conj(fx_k) in build_y
  double omega = 0.0;          // fisdf_set_omega: range-separated Coulomb kernel of the fit
  // extra streams of the fit lanes (fisdf_fit_coulomb_qs)
  hipStream_t aux[3] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
  // cross-stream ordering of buffers handed back to the caller's allocator: a
  // call that gives aux[i] work bumps aux_use[i]; joining aux[i] into `stream` (aux_join) sets
  // aux_joined[i] = aux_use[i].  build_return asserts every aux stream is joined, so a buffer
  // freed stream-ordered on `stream` has no reader left on another stream
  unsigned aux_use[3] = {0, 0, 0}, aux_joined[3] = {0, 0, 0};
  hipEvent_t ev_ybuf[4] = {nullptr, nullptr, nullptr, nullptr};  // y pipeline: fx ready / free
  std::vector<hipEvent_t> ev_q;  // FISDF_FIT_PIPE: Yhat of fitted q ready (FFT stream)
  std::vector<hipEvent_t> ev_free;  // FISDF_FIT_PIPE: Yhat ring slot read by its lane
  int pipe_mode = -1;   // fisdf_set_fit_pipe; -1: environment FISDF_FIT_PIPE (default on)
  int pipe_depth = 0;   // ring slots; 0: lanes + 2
  int last_fit_lanes = 0, last_fit_pipe = 0;  // what the last fisdf_fit_coulomb_qs ran with
  // fisdf_fit_report: what the last fisdf_fit_coulomb_qs did for each q of its list
  struct FitRec {
    int v[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  };
  std::vector<FitRec> fit_report;
  std::vector<hipEvent_t> ev_ready;  // fisdf_mark_y_ready: y of local q j landed (sharded fit)
  std::vector<char> ready_marked;
  // fisdf_set_y_slices: y of local q j read in place from its all-to-all piece (grid slices)
  std::vector<const cplx*> y_piece;
  // the composite 1-GPU build stores the self-conjugate q's y real (y_real_store, set around
  // its y build and fit); y_real_slot[i]: slot i of the last fisdf_build_y_qs holds doubles
  bool y_real_store = false;
  std::vector<char> y_real_slot;
  std::vector<long> y_slices;  // (g0, ng) pairs of the pieces' layout, shared by every piece
  std::map<std::vector<long>, PlaneRef*> plane_cache;  // device plane tables per (slices, mesh, rows)
  int* f_piv = nullptr;     // (nk, nip)
  int* f_rank_dev = nullptr;
  std::vector<int> f_rank;  // host copy
  // the factorisation runs on a side stream, overlapped with the y build on `stream`, at the
  // priority fisdf_set_factor_priority asked for (side_hi: the priority it was created with)
  hipStream_t side = nullptr;
  int factor_hi = 0, side_hi = -1;
  std::vector<hipStream_t> pad;  // FISDF_PAD_QUEUES (ensure_side)
  void* pad_buf = nullptr;
  hipEvent_t ev_x4 = nullptr, ev_fac = nullptr, ev_chol = nullptr;
  hipEvent_t ev_fac_early = nullptr;  // the first f_early slots' operators (factor_finish)
  int f_early = 0;
  bool f_fac_unjoined = false;  // ev_fac not yet waited on by the main stream (fit lanes do)
  bool f_pending = false;
  bool x4_marked = false;  // fisdf_factor_x4_mark recorded ev_x4 for the next factor_x4_async
  int* f_rank_pinned = nullptr;  // host (pinned) copy target, f_nk ints
  void* f_scratch = nullptr;     // device scratch of the factorisation
  size_t f_scratch_size = 0;
  // pinned staging of small host arrays copied asynchronously (q-lists)
  int* stage_pinned = nullptr;
  int* sel_pinned = nullptr;  // selection read-back {error flag, rank, pivots} (pinned)
  size_t sel_cap = 0;
  size_t stage_cap = 0;
  hipEvent_t ev_stage = nullptr;
  // reality-invariant monitors
  unsigned long long* maximag = nullptr;  // 3 slots
  // time-reversal check of the build's AO inputs (x0, f): {max dev, max |a|} x 2 on the device,
  // read back through tr_pinned when ev_tr completes
  unsigned long long* trmon = nullptr;
  unsigned long long* tr_pinned = nullptr;
  hipEvent_t ev_tr = nullptr;
  // timing
  bool timing = false;
  struct Ev { int stage; hipEvent_t a, b; int span; };
  std::vector<Ev> events;
  // kernel execution spans of the kernel-exact stages (StageTimer): 2 u64 per slot, all-ones
  // initialised, read and refilled by fisdf_timings
  unsigned long long* spans = nullptr;
  int span_used = 0;
  static constexpr int kSpanCap = 16384;
  std::string last_error;  // fisdf_last_error(ctx)
  // fisdf_build: the resident result of the last composite build (W_q, W_s, X, ... on the device)
  struct Build {
    bool valid = false;
    int nk = 0, nip = 0, nao = 0, ng0 = 0, nfit = 0, used_pivoted = 0, min_norm = 0;
    int time_reversal = 0;  // 1: one q of each (q, -q) pair fitted (the inputs passed the check)
    double tr_deviation = 0.0;
    int kmesh[3] = {0, 0, 0}, mesh[3] = {0, 0, 0};
    double a[9] = {0};
    std::vector<int> perm, fit_qs, partner, ranks;
    std::vector<double> wt;
    void *X = nullptr, *x4 = nullptr, *Wq = nullptr, *Ws = nullptr;
    // fisdf_build_sharded: this rank's share (W_s rows [row0, row1), W_0 broadcast) and the
    // caller's collectives (get_jk all-reduces through them)
    int shard_rank = 0, shard_size = 1, row0 = 0, row1 = 0;
    void* W0 = nullptr;
    bool sharded = false;
    bool y_streamed = false;  // y formed behind the selection (fisdf_build_y_streamed)
    fisdf_comm comm{};
  } bld;
  // stream of the sharded build's all-to-all (fisdf_build_sharded), forked from `stream`
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_comm = nullptr;
  // fisdf_set_allocator: device memory of the composite build's buffers from the caller (e.g. a
  // framework's caching allocator), else library-owned grow-only buffers
  fisdf_alloc_fn alloc_fn = nullptr;
  fisdf_free_fn free_fn = nullptr;
  void* alloc_user = nullptr;
  std::map<int, std::pair<void*, size_t>> owned;  // role -> library-owned buffer
  std::vector<void*> lent;                        // buffers from alloc_fn not yet returned
  // The y build streamed behind the selection (build_impl, FISDF_Y_STREAM): while the
  // cooperative selection runs on `stream`, aux[2] and aux[0] form y in blocks of pivots as the
  // kernel publishes them (pchol_select_coop's progress word).  ys_dev: {progress, spin error}
  // (device ints); ws_ypiv: the pivots, context-owned so that no later arena user
  // overwrites them under the y stream; ws_ystream: XT / FT of the fused kernel.  `ys` is the
  // build's request, armed around the first selection only; enqueued: the y stream received the
  // work.
  int* ys_dev = nullptr;
  int* ys_err_pinned = nullptr;
  hipEvent_t ev_yerr = nullptr;
  hipEvent_t ev_ysfork = nullptr;  // `stream` just before the selection kernel: the y stream's start
  hipEvent_t ev_ys2[2] = {nullptr, nullptr};  // the streamed y's second stream (FISDF_Y_STREAM_2S)
  DevBuf ws_ypiv, ws_ystream;
  struct YStream {
    bool armed = false, enqueued = false;
    bool stale = false;  // the kernel it followed failed (a stalled step): its pivots were redone
    int aux = 2;         // the aux stream it runs on
    const cplx* x0 = nullptr;
    const cplx* f = nullptr;
    int ng0 = 0, nao = 0, nip = 0, rows = 128;
    long m = 0, fks = 0;  // grid points of the y build (columns of yT), k stride of f
    int kmesh[3] = {0, 0, 0};
    std::vector<int> qs;
    cplx* yT = nullptr;
    unsigned long long rmask = 0;
  } ys;
};

namespace fisdf {
void set_ctx_error(fisdf_ctx* c, const std::string& msg) { c->last_error = msg; }
}  // namespace fisdf

namespace {

// a grow-only temporary (growth waits for the device: the old block may be in use on any stream)
static int devbuf_get(fisdf_ctx::DevBuf& w, size_t bytes, void** out) {
  bytes = std::max<size_t>(bytes, 256);
  if (bytes > w.n) {
    if (w.p) {
      FISDF_HIP(hipDeviceSynchronize());
      FISDF_HIP(hipFree(w.p));
    }
    w.p = nullptr;
    w.n = 0;
    FISDF_HIP(hipMalloc(&w.p, bytes));
    w.n = bytes;
  }
  *out = w.p;
  return 0;
}

int arena_get(fisdf_ctx* c, size_t bytes, void** out) {
  bytes = std::max<size_t>(bytes, 256);
  if (bytes > c->arena_size) {
    FISDF_HIP(hipStreamSynchronize(c->stream));
    if (c->arena) FISDF_HIP(hipFree(c->arena));
    c->arena = nullptr;
    c->arena_size = 0;  // a failed growth below must not leave a stale size behind a null base
    size_t sz = bytes + bytes / 8;
    if (hipMalloc(&c->arena, sz) != hipSuccess) {
      (void)hipGetLastError();
      c->arena = nullptr;
      FISDF_HIP(hipMalloc(&c->arena, bytes));  // without the growth slack, then give up
      sz = bytes;
    }
    c->arena_size = sz;
  }
  *out = c->arena;
  return 0;
}

// carve aligned sub-buffers from one arena request
struct Carver {
  size_t off = 0;
  size_t take(size_t bytes) {
    size_t o = off;
    off += (bytes + 255) / 256 * 256;
    return o;
  }
};

// Asynchronous upload of a small host int array: staged through a pinned buffer whose reuse
// waits for the previous copy (no host sync on the stream).
// host -> device through the context's pinned staging buffer, asynchronous on the main stream;
// the buffer is reused once the previous staged copy has completed (ev_stage)
int upload_bytes(fisdf_ctx* c, const void* h, size_t bytes, void* d) {
  if (bytes == 0) return 0;
  if (!c->ev_stage) FISDF_HIP(hipEventCreateWithFlags(&c->ev_stage, hipEventDisableTiming));
  FISDF_HIP(hipEventSynchronize(c->ev_stage));
  if (bytes > c->stage_cap) {
    if (c->stage_pinned) FISDF_HIP(hipHostFree(c->stage_pinned));
    c->stage_pinned = nullptr;
    c->stage_cap = 0;
    FISDF_HIP(hipHostMalloc((void**)&c->stage_pinned, bytes, hipHostMallocDefault));
    c->stage_cap = bytes;
  }
  std::memcpy(c->stage_pinned, h, bytes);
  FISDF_HIP(hipMemcpyAsync(d, c->stage_pinned, bytes, hipMemcpyHostToDevice, c->stream));
  FISDF_HIP(hipEventRecord(c->ev_stage, c->stream));
  return 0;
}

int upload_ints(fisdf_ctx* c, const int* h, int n, int* d) {
  return n <= 0 ? 0 : upload_bytes(c, h, sizeof(int) * (size_t)n, d);
}

// Stage timer on stream `st`: events recorded on the stream around the stage.  kernel_exact: the
// stage is ONE zgemm()/herk() call whose kernels also record their execution span on the device
// (launch_events); fisdf_timings then reports that span — the kernels' own begin to end, as
// rocprofv3's kernel trace times them — instead of the event interval, which beside the other fit
// lanes also counts the time the stream waits for free CUs (r02: ~10 % more than the trace).
struct StageTimer {
  fisdf_ctx* c;
  int stage;
  hipStream_t st;
  bool exact;
  hipEvent_t a = nullptr, b = nullptr;
  int span = -1;
  StageTimer(fisdf_ctx* c_, int stg, hipStream_t on = nullptr, bool kernel_exact = false)
      : c(c_), stage(stg), st(on ? on : c_->stream), exact(kernel_exact) {
    if (c->timing) {
      (void)hipEventCreate(&a);
      (void)hipEventCreate(&b);
      (void)hipEventRecord(a, st);
      if (exact && c->spans && c->span_used < fisdf_ctx::kSpanCap) {
        span = c->span_used++;
        LaunchEvents le;
        le.span = c->spans + 2 * span;
        launch_events() = le;
      }
    }
  }
  ~StageTimer() {
    if (c->timing) {
      (void)hipEventRecord(b, st);
      if (span >= 0) launch_events() = LaunchEvents();
      c->events.push_back({stage, a, b, span});
    }
  }
};

void lattice(const double a[9], CellGeom& g) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) g.a[i][j] = a[3 * i + j];
  // b = 2 pi inv(a)^T
  const double(*A)[3] = g.a;
  double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) -
               A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
               A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
  double inv[3][3];
  inv[0][0] = (A[1][1] * A[2][2] - A[1][2] * A[2][1]) / det;
  inv[0][1] = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) / det;
  inv[0][2] = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) / det;
  inv[1][0] = (A[1][2] * A[2][0] - A[1][0] * A[2][2]) / det;
  inv[1][1] = (A[0][0] * A[2][2] - A[0][2] * A[2][0]) / det;
  inv[1][2] = (A[0][2] * A[1][0] - A[0][0] * A[1][2]) / det;
  inv[2][0] = (A[1][0] * A[2][1] - A[1][1] * A[2][0]) / det;
  inv[2][1] = (A[0][1] * A[2][0] - A[0][0] * A[2][1]) / det;
  inv[2][2] = (A[0][0] * A[1][1] - A[0][1] * A[1][0]) / det;
  const double twopi = 6.283185307179586;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) g.b[i][j] = twopi * inv[j][i];
}

double cell_volume(const double a[9]) {
  return std::fabs(a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) +
                   a[2] * (a[3] * a[7] - a[4] * a[6]));
}

// k-point q of the mesh (get_kpts order, wrap_around=False): k = (i/n) . b
void kpoint(const int kmesh[3], const CellGeom& g, int q, double k[3]) {
  int i2 = q % kmesh[2], i1 = (q / kmesh[2]) % kmesh[1], i0 = q / (kmesh[1] * kmesh[2]);
  double f[3] = {(double)i0 / kmesh[0], (double)i1 / kmesh[1], (double)i2 / kmesh[2]};
  for (int c = 0; c < 3; ++c) k[c] = f[0] * g.b[0][c] + f[1] * g.b[1][c] + f[2] * g.b[2][c];
}

// Phi[R,k] = exp(i T_R . k)/sqrt(nk)  (k2gamma.get_phase, wrap_around=False)
int get_phase(fisdf_ctx* c, const int kmesh[3], const double a[9], const cplx** out) {
  std::vector<double> key = {(double)kmesh[0], (double)kmesh[1], (double)kmesh[2]};
  for (int i = 0; i < 9; ++i) key.push_back(a[i]);
  auto it = c->phase_cache.find(key);
  if (it != c->phase_cache.end()) { *out = it->second; return 0; }
  CellGeom g;
  lattice(a, g);
  int nk = kmesh[0] * kmesh[1] * kmesh[2];
  std::vector<cplx> h((size_t)nk * nk);
  for (int R = 0; R < nk; ++R) {
    int r2 = R % kmesh[2], r1 = (R / kmesh[2]) % kmesh[1], r0 = R / (kmesh[1] * kmesh[2]);
    double T[3];
    for (int cc = 0; cc < 3; ++cc) T[cc] = r0 * g.a[0][cc] + r1 * g.a[1][cc] + r2 * g.a[2][cc];
    for (int q = 0; q < nk; ++q) {
      double k[3];
      kpoint(kmesh, g, q, k);
      double th = T[0] * k[0] + T[1] * k[1] + T[2] * k[2];
      h[(size_t)R * nk + q] = cmk(std::cos(th) / std::sqrt((double)nk), std::sin(th) / std::sqrt((double)nk));
    }
  }
  cplx* d = nullptr;
  FISDF_HIP(hipMalloc(&d, sizeof(cplx) * h.size()));
  FISDF_HIP(hipMemcpy(d, h.data(), sizeof(cplx) * h.size(), hipMemcpyHostToDevice));
  c->phase_cache[key] = d;
  *out = d;
  return 0;
}

int device_guard(fisdf_ctx* c) {
  t_cur_ctx = c;
  FISDF_CHECK(c != nullptr, "null context");
  FISDF_HIP(hipSetDevice(c->device));
  return 0;
}

// the entry points that touch no device state: failures still go to the context's own message
int ctx_guard(fisdf_ctx* c) {
  t_cur_ctx = c;
  FISDF_CHECK(c != nullptr, "null context");
  return 0;
}

const cplx ONE = {1.0, 0.0}, ZERO = {0.0, 0.0};

int free_factors(fisdf_ctx* c) {
  if (c->f_L) FISDF_HIP(hipFree(c->f_L));
  if (c->f_Lp) FISDF_HIP(hipFree(c->f_Lp));
  if (c->f_Linv) FISDF_HIP(hipFree(c->f_Linv));
  if (c->f_Q) FISDF_HIP(hipFree(c->f_Q));
  c->f_Q = nullptr;
  if (c->f_Li) FISDF_HIP(hipFree(c->f_Li));
  c->f_Li = nullptr;
  if (c->f_ksw) FISDF_HIP(hipFree(c->f_ksw));
  c->f_ksw = nullptr;
  c->f_ksw_elems = 0;
  if (c->f_x4s) FISDF_HIP(hipFree(c->f_x4s));
  c->f_x4s = nullptr;
  if (c->f_M) FISDF_HIP(hipFree(c->f_M));
  c->f_M = nullptr;
  if (c->f_nip_dev) FISDF_HIP(hipFree(c->f_nip_dev));
  c->f_nip_dev = nullptr;
  c->f_cod.clear();
  if (c->f_fail_pinned) FISDF_HIP(hipHostFree(c->f_fail_pinned));
  c->f_fail_pinned = nullptr;
  if (c->f_qr_pinned) FISDF_HIP(hipHostFree(c->f_qr_pinned));
  c->f_qr_pinned = nullptr;
  if (c->f_qr_dev) FISDF_HIP(hipFree(c->f_qr_dev));
  c->f_qr_dev = nullptr;
  if (c->f_piv) FISDF_HIP(hipFree(c->f_piv));
  if (c->f_rank_dev) FISDF_HIP(hipFree(c->f_rank_dev));
  if (c->f_rank_pinned) FISDF_HIP(hipHostFree(c->f_rank_pinned));
  c->f_rank_pinned = nullptr;
  c->f_L = c->f_Lp = c->f_Linv = nullptr;
  c->f_piv = c->f_rank_dev = nullptr;
  c->f_rank.clear();
  c->f_qs.clear();
  c->f_real.clear();
  c->f_nk = c->f_nip = 0;
  c->f_cap_nk = c->f_cap_nip = 0;
  return 0;
}

// x2 = sum_{q in [q0,q1)} conj(x0_q) x0_q^T, via P = x0 permuted to (ng0, nq*nao) and the
// Hermitian update P P^H (only its real part is used: Re(P P^H) = Re(conj(P) P^T)).
// `tmp` must hold ng0*nq*nao complex.
// the HERK split-K of the selection Gram (n x n from K columns): more tiles in flight while the
// triangle alone leaves CUs idle and every part keeps 256 columns
int select_gram_ksplit(int ng0, int K) {
  int ks = 1;
  const long tiles = (long)((ng0 + 63) / 64) * ((ng0 + 63) / 64 + 1) / 2;
  while (tiles * ks < 512 && K / (ks * 2) >= 256) ks *= 2;
  return ks;
}

// info (nullable, 3 ints): the k-points summed (the representatives under the fold), the permute
// launches and the HERK split-K
void select_gram_plan(const int* kmesh, bool fold, int nq, int ng0, int nao, int* info) {
  int launches = nq > 0 ? 1 : 0;
  if (kmesh && fold) {
    std::vector<int> reps;
    std::vector<char> self;
    kmesh_reps(kmesh, &reps, &self);
    nq = (int)reps.size();
    launches = (nq + 63) / 64;
  }
  info[0] = nq;
  info[1] = launches;
  info[2] = nq > 0 ? select_gram_ksplit(ng0, nq * nao) : 0;
}

// fold: sum the time-reversal representatives of `kmesh` only (the whole mesh, q0 = 0, q1 = nk)
int select_gram(fisdf_ctx* c, const cplx* x0, int nk, int q0, int q1, int ng0, int nao, cplx* x2,
                cplx* tmp, const int* kmesh, bool fold) {
  int nq = q1 - q0;
  if (kmesh && fold && q0 == 0 && q1 == nk) {
    // time reversal (x0_{-q} = conj(x0_q)): Re(x0_{-q} x0_{-q}^H) = Re(x0_q x0_q^H), so the sum
    // over the k-mesh is the sum over the representatives q <= -q with a paired one counted
    // twice — its copy scaled by sqrt(2): 36 of 64 k at 4x4x4
    std::vector<int> reps;
    std::vector<char> self;
    kmesh_reps(kmesh, &reps, &self);
    std::vector<double> sc(reps.size());
    for (size_t j = 0; j < reps.size(); ++j) sc[j] = self[j] ? 1.0 : std::sqrt(2.0);
    nq = (int)reps.size();
    FISDF_TRY(permute_kgm_sel(c->stream, x0, reps.data(), sc.data(), nq, ng0, nao, tmp));
  } else {
    FISDF_TRY(permute_kgm(c->stream, x0 + (long)q0 * ng0 * nao, nq, ng0, nao, tmp));
  }
  const int K = nq * nao;
  const int ks = select_gram_ksplit(ng0, K);
  void* work = nullptr;
  if (ks > 1) FISDF_TRY(devbuf_get(c->ws_main, sizeof(cplx) * (size_t)ks * ng0 * ng0, &work));
  // only Re(x2) enters the selection (fftisdf.py:379): real-part HERK, imaginary part zero
  FISDF_TRY(herk(c->stream, ng0, K, 1.0, tmp, K, x2, ng0, ks, (cplx*)work, GEMM_RE_ONLY));
  (void)nk;
  return 0;
}

// q is its own time-reversal partner (2 k_q in the reciprocal lattice): Phi[:, q] is real, so
// x4_q, y_q and z_q are real and W_q = Zhat diag(c) Zhat^H is real (Hermitian-symmetric
// spectrum) — the fit runs with a real factor (GEMM_A_REAL) and a real-part HERK
bool self_conjugate(const int kmesh[3], int q) {
  const int i2 = q % kmesh[2], i1 = (q / kmesh[2]) % kmesh[1], i0 = q / (kmesh[1] * kmesh[2]);
  return (2 * i0) % kmesh[0] == 0 && (2 * i1) % kmesh[1] == 0 && (2 * i2) % kmesh[2] == 0;
}

// cached Coulomb weight of the fit for q (computed on `st` and waited for the first time, so
// every stream may read it afterwards)
// the reciprocal-lattice vector m.b = 2 k_q of a self-conjugate q
void self_conjugate_m(const int kmesh[3], int q, int m[3]) {
  const int i2 = q % kmesh[2], i1 = (q / kmesh[2]) % kmesh[1], i0 = q / (kmesh[1] * kmesh[2]);
  m[0] = 2 * i0 / kmesh[0];
  m[1] = 2 * i1 / kmesh[1];
  m[2] = 2 * i2 / kmesh[2];
}

// half: the self-conjugate q's half-grid weight sqrt(c_G + c_G') (sqrt(c_G) on a self-paired
// plane, 0 beyond the prefix planes), see linalg.h half_weight
int get_weight(fisdf_ctx* c, hipStream_t st, const int mesh[3], const int kmesh[3],
               const double a[9], int q, double scale, bool half, const double** out) {
  std::vector<double> key = {(double)mesh[0], (double)mesh[1], (double)mesh[2], (double)kmesh[0],
                             (double)kmesh[1], (double)kmesh[2], (double)q, c->omega, scale,
                             half ? 1.0 : 0.0};
  for (int i = 0; i < 9; ++i) key.push_back(a[i]);
  auto it = c->wt_cache.find(key);
  if (it == c->wt_cache.end()) {
    CellGeom g;
    lattice(a, g);
    double kq[3];
    kpoint(kmesh, g, q, kq);
    const size_t ng = (size_t)mesh[0] * mesh[1] * mesh[2];
    double* w = nullptr;
    FISDF_HIP(hipMalloc(&w, sizeof(double) * ng));
    if (!half) {
      FISDF_TRY(coulg_weight(st, mesh, g, kq, scale, 1, w, c->omega));
    } else {
      // a cache fill: plain allocations (no stream-ordered pool memory shared with other streams)
      double* cw = nullptr;
      FISDF_HIP(hipMalloc((void**)&cw, sizeof(double) * ng));
      FISDF_TRY(coulg_weight(st, mesh, g, kq, scale, 0, cw, c->omega));
      int m[3];
      self_conjugate_m(kmesh, q, m);
      FISDF_TRY(half_weight(st, w, cw, mesh, m));
      FISDF_HIP(hipStreamSynchronize(st));
      FISDF_HIP(hipFree(cw));
    }
    FISDF_HIP(hipStreamSynchronize(st));
    it = c->wt_cache.emplace(key, w).first;
  }
  *out = it->second;
  return 0;
}

// the half-grid asymmetric-weight list of a self-conjugate q with its Im factors (cached)
int get_asym_half(fisdf_ctx* c, hipStream_t st, const int mesh[3], const int kmesh[3],
                  const double a[9], int q, double scale, const fisdf_ctx::Asym** out) {
  std::vector<double> key = {(double)mesh[0], (double)mesh[1], (double)mesh[2], (double)kmesh[0],
                             (double)kmesh[1], (double)kmesh[2], (double)q, c->omega, scale, 1.0};
  for (int i = 0; i < 9; ++i) key.push_back(a[i]);
  auto it = c->asym_cache.find(key);
  if (it == c->asym_cache.end()) {
    CellGeom g;
    lattice(a, g);
    double kq[3];
    kpoint(kmesh, g, q, kq);
    const long ngrid = (long)mesh[0] * mesh[1] * mesh[2];
    fisdf_ctx::Asym as;
    double* cw = nullptr;
    FISDF_HIP(hipMalloc(&as.idx, sizeof(int) * (ngrid + 1)));
    FISDF_HIP(hipMalloc(&as.f, sizeof(double) * ngrid));
    FISDF_HIP(hipMalloc((void**)&cw, sizeof(double) * ngrid));  // a cache fill (see get_weight)
    FISDF_TRY(coulg_weight(st, mesh, g, kq, scale, 0, cw, c->omega));
    int m[3];
    self_conjugate_m(kmesh, q, m);
    FISDF_TRY(asym_half(st, cw, mesh, m, as.idx, as.f, as.idx + ngrid));
    FISDF_HIP(hipMemcpyAsync(&as.n, as.idx + ngrid, sizeof(int), hipMemcpyDeviceToHost, st));
    FISDF_HIP(hipStreamSynchronize(st));
    FISDF_HIP(hipFree(cw));
    it = c->asym_cache.emplace(key, as).first;
  }
  *out = &it->second;
  return 0;
}

// cached asym_list of a self-conjugate q (one synchronous count read the first time)
int get_asym(fisdf_ctx* c, hipStream_t st, const int mesh[3], const int kmesh[3],
             const double a[9], int q, const double* wt, const fisdf_ctx::Asym** out) {
  std::vector<double> key = {(double)mesh[0], (double)mesh[1], (double)mesh[2], (double)kmesh[0],
                             (double)kmesh[1], (double)kmesh[2], (double)q, c->omega};
  for (int i = 0; i < 9; ++i) key.push_back(a[i]);
  auto it = c->asym_cache.find(key);
  if (it == c->asym_cache.end()) {
    const int i2 = q % kmesh[2], i1 = (q / kmesh[2]) % kmesh[1], i0 = q / (kmesh[1] * kmesh[2]);
    const int m[3] = {2 * i0 / kmesh[0], 2 * i1 / kmesh[1], 2 * i2 / kmesh[2]};
    const long ngrid = (long)mesh[0] * mesh[1] * mesh[2];
    fisdf_ctx::Asym as;
    int* cnt = nullptr;
    FISDF_HIP(hipMalloc(&as.idx, sizeof(int) * (ngrid + 1)));
    cnt = as.idx + ngrid;
    FISDF_TRY(asym_list(st, wt, mesh, m, as.idx, cnt));
    FISDF_HIP(hipMemcpyAsync(&as.n, cnt, sizeof(int), hipMemcpyDeviceToHost, st));
    FISDF_HIP(hipStreamSynchronize(st));
    if (getenv("FISDF_VERBOSE")) fprintf(stderr, "fisdf: q %d: %d of %ld G with asymmetric weight\n", q, as.n, ngrid);
    it = c->asym_cache.emplace(key, as).first;
  }
  *out = &it->second;
  return 0;
}

int env_fit_lanes() {
  static const int n = [] {
    const char* e = getenv("FISDF_FIT_LANES");
    const int v = e ? atoi(e) : 2;
    return std::max(1, std::min(4, v));
  }();
  return n;
}

int env_fit_pipe() {
  static const int v = [] {
    const char* e = getenv("FISDF_FIT_PIPE");
    return (e && e[0] == '0') ? 0 : 1;
  }();
  return v;
}

int env_half_grid() {
  static const int v = [] {
    const char* e = getenv("FISDF_HALF_G");
    return (e && e[0] == '0') ? 0 : 1;
  }();
  return v;
}

// the FFT ring's depth when fisdf_set_fit_pipe gave none: FISDF_PIPE_DEPTH, else lanes + 2
int default_pipe_depth(int lanes) {
  static const int env = [] {
    const char* e = getenv("FISDF_PIPE_DEPTH");
    return e ? std::max(0, std::min(64, atoi(e))) : 0;
  }();
  return env > 0 ? env : lanes + 2;
}

int num_cus(int device) {
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n <= 0)
    n = 256;
  return n;
}

// The fit's extra streams: aux[0] and aux[1] are MFMA lanes, aux[2] the pipelined FFT stream (its
// priority below).  All three are created
// together and in this order: HIP maps a process's streams onto hardware queues by creation
// order, and leaving aux[1] uncreated when unused measured +4.5 ms/step (even with 8 queues).
int ensure_aux(fisdf_ctx* c) {
  if (c->ev_fork) return 0;
  FISDF_HIP(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  int least = 0, greatest = 0;
  FISDF_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
  // The FFT stream's priority depends on the HIP runtime the process runs: on the ROCm 7.0
  // runtime torch bundles the least priority is -0.45 ms/step (the lanes' MFMA kernels take the
  // CU slots first, r03), but the 7.2 runtime honours it more strictly and starves the FFTs the
  // lanes wait on: +4.2 ms/step (tools/capi_bench.py, profiles/r04/capi_vs_torch).  So: least
  // below 7.2, the default priority from 7.2 on.  FISDF_FFT_PRIO: 0 least, 1 default, 2 greatest.
  static const int fft_prio = [] {
    const char* e = getenv("FISDF_FFT_PRIO");
    if (e) return atoi(e);
    int v = 0;
    if (hipRuntimeGetVersion(&v) != hipSuccess) return 1;
    return (v / 10000000 > 7 || (v / 10000000 == 7 && (v / 100000) % 100 >= 2)) ? 1 : 0;
  }();
  // FISDF_FFT_CUS=n (experiment): the FFT stream confined to n CUs spread evenly over the device
  // (hipExtStreamCreateWithCUMask), so the HBM-bound FFTs stop taking workgroup slots on every CU
  static const int fft_cus = getenv("FISDF_FFT_CUS") ? atoi(getenv("FISDF_FFT_CUS")) : 0;
  for (int l = 0; l < 3; ++l) {
    if (l == 2 && fft_cus > 0) {
      const int ncu = num_cus(c->device);
      std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
      const int n = std::min(fft_cus, ncu);
      for (int i = 0; i < n; ++i) {
        const int cu = (int)((long)i * ncu / n);
        mask[cu / 32] |= 1u << (cu % 32);
      }
      FISDF_HIP(hipExtStreamCreateWithCUMask(&c->aux[l], (uint32_t)mask.size(), mask.data()));
    } else if (l == 2 && fft_prio != 1)
      FISDF_HIP(hipStreamCreateWithPriority(&c->aux[l], hipStreamNonBlocking,
                                            fft_prio == 2 ? greatest : least));
    else
      FISDF_HIP(hipStreamCreateWithFlags(&c->aux[l], hipStreamNonBlocking));
    FISDF_HIP(hipEventCreateWithFlags(&c->ev_join[l], hipEventDisableTiming));
  }
  for (int l = 0; l < 4; ++l) FISDF_HIP(hipEventCreateWithFlags(&c->ev_ybuf[l], hipEventDisableTiming));
  return 0;
}


std::vector<int> q_range(int q0, int q1) {
  std::vector<int> v;
  for (int q = q0; q < q1; ++q) v.push_back(q);
  return v;
}

// aux[i] is given work that may read a build buffer (fork side of the invariant above)
void aux_fork(fisdf_ctx* c, int i) { ++c->aux_use[i]; }

// join aux[i] into the main stream: later work (and frees) on `stream` are ordered after it
int aux_join(fisdf_ctx* c, int i) {
  FISDF_HIP(hipEventRecord(c->ev_join[i], c->aux[i]));
  FISDF_HIP(hipStreamWaitEvent(c->stream, c->ev_join[i], 0));
  c->aux_joined[i] = c->aux_use[i];
  return 0;
}

int check_aux_joined(fisdf_ctx* c, const char* what) {
  for (int i = 0; i < 3; ++i)
    FISDF_CHECK(c->aux_joined[i] == c->aux_use[i],
                std::string(what) + ": aux stream " + std::to_string(i) +
                    " not joined into the context stream (a buffer would be freed under a reader)");
  return 0;
}

int check_qlist(const int* qs, int nq, int nk, const char* who) {
  FISDF_CHECK(nq >= 0 && (nq == 0 || qs != nullptr), std::string(who) + ": bad q-list");
  for (int i = 0; i < nq; ++i)
    FISDF_CHECK(qs[i] >= 0 && qs[i] < nk && (i == 0 || qs[i] > qs[i - 1]),
                std::string(who) + ": q-list must be ascending and inside the k-mesh");
  return 0;
}

// K-split for a HERK of n x n over K: the lower-triangle tile count times ks is chosen just
// below a whole number of rounds of resident workgroups (3 per CU for the 64x64 ZGEMM tile),
// so the last round is not a nearly empty tail; each split keeps >= 2048 of K (the split
// partials cost 2 ks n^2 x 16 B of extra traffic).
int pick_ksplit_herk(int n, int K, int ncu) {
  const long nt = (n + 63) / 64, tiles = nt * (nt + 1) / 2;
  if (tiles == 0) return 1;  // n = 0: a rank-0 q beside others in one fit call
  const long slots = 3L * ncu;
  int best = 1;
  double best_eff = 0;
  for (int m = 1; m <= 4; ++m) {
    long ks = std::max(1L, (m * slots) / tiles);
    ks = std::min<long>(ks, std::max(1, K / 1024));  // C3 sweep (3M): ks 13 -> 41 is -5% HERK time
    const long T = tiles * ks;
    const double eff = (double)T / ((double)((T + slots - 1) / slots) * slots);
    if (eff > best_eff + 0.01 || (eff > best_eff - 0.01 && ks > best)) {
      if (eff > best_eff) best_eff = eff;
      best = (int)ks;
    }
  }
  return best;
}


int pick_ksplit(int M, int N, int K) {
  long tiles = (long)((M + 63) / 64) * ((N + 63) / 64);
  int ks = 1;
  while (tiles * ks < 1024 && K / (ks * 2) >= 512) ks *= 2;
  return ks;
}

// whether a fit call of nq q runs each q's W_PP in its lane (when every q is full rank and none
// is a minimum-norm slot; the batched tail otherwise).  FISDF_LANE_WPP: 0 never, 1 always
constexpr int kLaneWppMinQ = 12;
bool lane_wpp_wanted(int nq) {
  static const int lane_wpp_env = [] {
    const char* e = getenv("FISDF_LANE_WPP");
    return e ? atoi(e) : -1;
  }();
  return lane_wpp_env < 0 ? nq >= kLaneWppMinQ : lane_wpp_env != 0;
}

// split-K of the W_PP GEMMs: from nip alone.  FISDF_WPP_KSPLIT (read per call; 1 = off)
int wpp_ksplit(int nip) {
  const char* e = getenv("FISDF_WPP_KSPLIT");
  const int v = e ? atoi(e) : 4;
  return (nip >= 256 && v > 1) ? std::min(v, 16) : 1;
}

}  // namespace

// ---------------------------------------------------------------------------
extern "C" {

int fisdf_abi_version(void) { return FISDF_ABI_VERSION; }

const char* fisdf_last_error(const fisdf_ctx* c) {
  return c ? c->last_error.c_str() : g_last_error.c_str();
}

int fisdf_create(int device, void* stream, fisdf_ctx** out) {
  t_cur_ctx = nullptr;
  FISDF_CHECK(out != nullptr, "out is null");
  int ndev = 0;
  FISDF_HIP(hipGetDeviceCount(&ndev));
  FISDF_CHECK(device >= 0 && device < ndev, "device id out of range (no GPU visible?)");
  FISDF_HIP(hipSetDevice(device));
  fisdf_ctx* c = new fisdf_ctx();
  c->device = device;
  // NULL = the device's default (null) stream, which orders with torch's default stream
  c->stream = (hipStream_t)stream;
  c->own_stream = false;
  FISDF_HIP(hipMalloc(&c->maximag, 4 * sizeof(unsigned long long)));
  FISDF_HIP(hipMemsetAsync(c->maximag, 0, 4 * sizeof(unsigned long long), c->stream));
  {
    std::lock_guard<std::mutex> lk(g_live_mu);
    g_live.insert(c);
  }
  *out = c;
  return 0;
}

int fisdf_destroy(fisdf_ctx* c) {
  if (!c) return 0;
  {
    std::lock_guard<std::mutex> lk(g_live_mu);
    g_live.erase(c);
  }
  if (t_cur_ctx == c) t_cur_ctx = nullptr;
  FISDF_HIP(hipSetDevice(c->device));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  // buffers lent by the caller's allocator stay the caller's (fisdf_set_allocator)
  c->lent.clear();
  for (auto& kv : c->owned)
    if (kv.second.first) (void)hipFree(kv.second.first);
  c->owned.clear();
  for (auto& e : c->events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  for (auto& kv : c->phase_cache) (void)hipFree(kv.second);
  for (auto& kv : c->asym_cache) {
    (void)hipFree(kv.second.idx);
    if (kv.second.f) (void)hipFree(kv.second.f);
  }
  for (auto& kv : c->wt_cache) (void)hipFree(kv.second);
  if (c->f_pending) (void)hipEventSynchronize(c->ev_fac);
  free_factors(c);
  if (c->f_scratch) (void)hipFree(c->f_scratch);
  if (c->f_ring) (void)hipFree(c->f_ring);
  for (int l = 0; l < 3; ++l)  // the streamed y build's workspaces may still be in use there
    if (c->aux[l]) (void)hipStreamSynchronize(c->aux[l]);
  if (c->ys_dev) (void)hipFree(c->ys_dev);
  if (c->ys_err_pinned) (void)hipHostFree(c->ys_err_pinned);
  if (c->ev_yerr) (void)hipEventDestroy(c->ev_yerr);
  if (c->ev_ysfork) (void)hipEventDestroy(c->ev_ysfork);
  for (hipEvent_t e : c->ev_ys2)
    if (e) (void)hipEventDestroy(e);
  for (auto* w : {&c->ws_main, &c->ws_side_a, &c->ws_side_b, &c->ws_x4, &c->ws_ypiv, &c->ws_ystream})
    if (w->p) (void)hipFree(w->p);
  for (hipStream_t p : c->pad) (void)hipStreamDestroy(p);
  if (c->pad_buf) (void)hipFree(c->pad_buf);
  if (c->side) {
    (void)hipStreamSynchronize(c->side);
    (void)hipStreamDestroy(c->side);
    (void)hipEventDestroy(c->ev_x4);
    (void)hipEventDestroy(c->ev_fac);
    (void)hipEventDestroy(c->ev_fac_early);
    (void)hipEventDestroy(c->ev_chol);
  }
  if (c->ev_fork) {
    (void)hipEventDestroy(c->ev_fork);
    for (int l = 0; l < 3; ++l) {
      if (c->aux[l]) {
        (void)hipStreamSynchronize(c->aux[l]);
        (void)hipStreamDestroy(c->aux[l]);
        c->aux[l] = nullptr;
      }
      (void)hipEventDestroy(c->ev_join[l]);
    }
    for (int l = 0; l < 4; ++l) (void)hipEventDestroy(c->ev_ybuf[l]);
  }
  for (hipEvent_t e : c->ev_q) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->ev_free) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->ev_ready) (void)hipEventDestroy(e);
  if (c->comm_stream) {
    (void)hipStreamSynchronize(c->comm_stream);
    (void)hipStreamDestroy(c->comm_stream);
    (void)hipEventDestroy(c->ev_comm);
  }
  for (auto& kv : c->plane_cache) (void)hipFree(kv.second);
  if (c->arena) (void)hipFree(c->arena);
  if (c->ev_stage) (void)hipEventSynchronize(c->ev_stage), (void)hipEventDestroy(c->ev_stage);
  if (c->stage_pinned) (void)hipHostFree(c->stage_pinned);
  if (c->sel_pinned) (void)hipHostFree(c->sel_pinned);
  if (c->maximag) (void)hipFree(c->maximag);
  if (c->ev_tr) (void)hipEventSynchronize(c->ev_tr), (void)hipEventDestroy(c->ev_tr);
  if (c->trmon) (void)hipFree(c->trmon);
  if (c->tr_pinned) (void)hipHostFree(c->tr_pinned);
  if (c->spans) (void)hipFree(c->spans);
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return 0;
}

int fisdf_sync(fisdf_ctx* c) {
  FISDF_TRY(device_guard(c));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int fisdf_malloc(fisdf_ctx* c, size_t bytes, void** p) {
  FISDF_TRY(device_guard(c));
  FISDF_HIP(hipMalloc(p, std::max<size_t>(bytes, 1)));
  return 0;
}

int fisdf_free(fisdf_ctx* c, void* p) {
  FISDF_TRY(device_guard(c));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  FISDF_HIP(hipFree(p));
  return 0;
}

int fisdf_memcpy_htod(fisdf_ctx* c, void* d, const void* h, size_t bytes) {
  FISDF_TRY(device_guard(c));
  FISDF_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int fisdf_memcpy_dtoh(fisdf_ctx* c, void* h, const void* d, size_t bytes) {
  FISDF_TRY(device_guard(c));
  FISDF_HIP(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int fisdf_set_timing(fisdf_ctx* c, int enable) {
  FISDF_TRY(device_guard(c));
  c->timing = enable != 0;
  if (c->timing && !c->spans) {
    FISDF_HIP(hipMalloc(&c->spans, sizeof(unsigned long long) * 2 * fisdf_ctx::kSpanCap));
    FISDF_HIP(hipMemsetAsync(c->spans, 0xff, sizeof(unsigned long long) * 2 * fisdf_ctx::kSpanCap,
                             c->stream));
    FISDF_HIP(hipStreamSynchronize(c->stream));
    c->span_used = 0;
  }
  return 0;
}

int fisdf_timings(fisdf_ctx* c, double* ms, int* calls) {
  FISDF_TRY(device_guard(c));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  for (int i = 0; i < FISDF_NSTAGES; ++i) {
    if (ms) ms[i] = 0;
    if (calls) calls[i] = 0;
  }
  std::vector<unsigned long long> sp(2 * (size_t)c->span_used);
  if (c->span_used) {
    FISDF_HIP(hipDeviceSynchronize());  // the lanes' kernels too
    FISDF_HIP(hipMemcpy(sp.data(), c->spans, sizeof(unsigned long long) * sp.size(),
                        hipMemcpyDeviceToHost));
  }
  for (auto& e : c->events) {
    float t = 0;
    if (e.span >= 0) {
      // the kernels' own execution span: s_memrealtime runs at 100 MHz
      const unsigned long long t0 = sp[2 * e.span], t1 = ~sp[2 * e.span + 1];
      t = (t0 != ~0ull && sp[2 * e.span + 1] != ~0ull && t1 >= t0) ? (float)((t1 - t0) * 1e-5) : 0.f;
    } else {
      FISDF_HIP(hipEventElapsedTime(&t, e.a, e.b));
    }
    if (ms) ms[e.stage] += t;
    if (calls) calls[e.stage] += 1;
    (void)hipEventDestroy(e.a);
    (void)hipEventDestroy(e.b);
  }
  c->events.clear();
  if (c->span_used) {
    FISDF_HIP(hipMemsetAsync(c->spans, 0xff, sizeof(unsigned long long) * 2 * c->span_used, c->stream));
    FISDF_HIP(hipStreamSynchronize(c->stream));
    c->span_used = 0;
  }
  return 0;
}

int fisdf_max_imag(fisdf_ctx* c, double* out) {
  FISDF_TRY(device_guard(c));
  unsigned long long h[4];
  FISDF_HIP(hipMemcpyAsync(h, c->maximag, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  for (int i = 0; i < 3; ++i) {
    double v;
    std::memcpy(&v, &h[i], sizeof(double));
    out[i] = v;
  }
  FISDF_HIP(hipMemsetAsync(c->maximag, 0, 4 * sizeof(unsigned long long), c->stream));
  return 0;
}

// ---- building blocks -------------------------------------------------------
int fisdf_zgemm(fisdf_ctx* c, int opA, int opB, int M, int N, int K, const double alpha[2],
                const void* A, long lda, long sA, const void* B, long ldb, long sB,
                const double beta[2], void* C, long ldc, long sC, int batch, int ksplit) {
  FISDF_TRY(device_guard(c));
  cplx* work = nullptr;
  if (ksplit > 1) {
    void* w;
    FISDF_TRY(arena_get(c, sizeof(cplx) * (size_t)ksplit * M * N * batch, &w));
    work = (cplx*)w;
  }
  return zgemm(c->stream, opA, opB, M, N, K, cmk(alpha[0], alpha[1]), (const cplx*)A, lda, sA,
               (const cplx*)B, ldb, sB, cmk(beta[0], beta[1]), (cplx*)C, ldc, sC, batch,
               ksplit, work);
}

int fisdf_zgemm_mode(fisdf_ctx* c, int opA, int opB, int M, int N, int K, const double alpha[2],
                     const void* A, long lda, long sA, const void* B, long ldb, long sB,
                     const double beta[2], void* C, long ldc, long sC, int batch, int mode) {
  FISDF_TRY(device_guard(c));
  return zgemm(c->stream, opA, opB, M, N, K, cmk(alpha[0], alpha[1]), (const cplx*)A, lda, sA,
               (const cplx*)B, ldb, sB, cmk(beta[0], beta[1]), (cplx*)C, ldc, sC, batch, 1,
               nullptr, EPI_NONE, nullptr, mode);
}

int fisdf_herk(fisdf_ctx* c, int n, int K, double alpha, const void* A, long lda, void* Cm,
               long ldc, int ksplit) {
  FISDF_TRY(device_guard(c));
  cplx* work = nullptr;
  if (ksplit > 1) {
    void* w;
    FISDF_TRY(arena_get(c, sizeof(cplx) * (size_t)ksplit * n * n, &w));
    work = (cplx*)w;
  }
  return herk(c->stream, n, K, alpha, (const cplx*)A, lda, (cplx*)Cm, ldc, ksplit, work);
}

int fisdf_zgemm_ex(fisdf_ctx* c, int opA, int opB, int M, int N, int K, const double alpha[2],
                   const void* A, long lda, long sA, const void* B, long ldb, long sB,
                   const double beta[2], void* C, long ldc, long sC, int batch, int ksplit,
                   int mode, int epi, const void* aux, long ldaux, double* h_mon) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(epi == EPI_NONE || epi == EPI_STREAM || epi == EPI_CSQUARE || epi == EPI_REAL ||
                  epi == EPI_WSRHO,
              "zgemm_ex: unknown epilogue");
  FISDF_CHECK(epi == EPI_NONE || (beta[0] == 0.0 && beta[1] == 0.0),
              "zgemm_ex: the epilogues take beta = 0");
  FISDF_CHECK(epi != EPI_REAL || batch <= 1, "zgemm_ex: EPI_REAL takes one batch");
  FISDF_CHECK(epi != EPI_WSRHO || (aux != nullptr && ldaux >= N),
              "zgemm_ex: EPI_WSRHO needs the real aux matrix (ldaux >= N)");
  // the epilogue's max |Im| goes to the context's fourth monitor word: fisdf_max_imag reports
  // the first three (the product's), which this call leaves alone
  const bool monitored = epi == EPI_CSQUARE || epi == EPI_REAL || epi == EPI_WSRHO;
  unsigned long long* mon = monitored ? c->maximag + 3 : nullptr;
  if (mon) FISDF_HIP(hipMemsetAsync(mon, 0, sizeof(unsigned long long), c->stream));
  cplx* work = nullptr;
  if (epi == EPI_WSRHO) {
    work = (cplx*)const_cast<void*>(aux);
  } else if (epi == EPI_NONE && ksplit > 1 && M > 0 && N > 0 && batch > 0) {
    void* w;
    FISDF_TRY(arena_get(c, sizeof(cplx) * (size_t)ksplit * M * N * batch, &w));
    work = (cplx*)w;
  }
  FISDF_TRY(zgemm(c->stream, opA, opB, M, N, K, cmk(alpha[0], alpha[1]), (const cplx*)A, lda, sA,
                  (const cplx*)B, ldb, sB, cmk(beta[0], beta[1]), (cplx*)C, ldc, sC, batch, ksplit,
                  work, epi, mon, mode, ldaux));
  if (h_mon) {
    *h_mon = 0.0;
    if (mon) {
      unsigned long long h = 0;
      FISDF_HIP(hipMemcpyAsync(&h, mon, sizeof(h), hipMemcpyDeviceToHost, c->stream));
      FISDF_HIP(hipStreamSynchronize(c->stream));
      std::memcpy(h_mon, &h, sizeof(double));
    }
  }
  return 0;
}

int fisdf_herk_ex(fisdf_ctx* c, int n, int K, double alpha, const void* A, long lda, long sA,
                  double beta, void* Cm, long ldc, long sC, int batch, int ksplit, int mode) {
  FISDF_TRY(device_guard(c));
  if (batch == 1 && beta == 0.0) {
    cplx* work = nullptr;
    if (ksplit > 1 && n > 0) {
      void* w;
      FISDF_TRY(arena_get(c, sizeof(cplx) * (size_t)ksplit * n * n, &w));
      work = (cplx*)w;
    }
    return herk(c->stream, n, K, alpha, (const cplx*)A, lda, (cplx*)Cm, ldc, ksplit, work, mode);
  }
  FISDF_CHECK(ksplit <= 1, "herk_ex: the batched / beta != 0 HERK has no split-K");
  FISDF_CHECK(mode == GEMM_FULL, "herk_ex: the batched / beta != 0 HERK has mode FULL only");
  return herk_batched(c->stream, n, K, alpha, (const cplx*)A, lda, sA, beta, (cplx*)Cm, ldc, sC,
                      batch);
}

int fisdf_fft3d(fisdf_ctx* c, const void* in, void* out, int rows, const int mesh[3]) {
  FISDF_TRY(device_guard(c));
  long ng = (long)mesh[0] * mesh[1] * mesh[2];
  return fft3d(c->stream, (const cplx*)in, ng, nullptr, (cplx*)out, ng, rows, mesh[0], mesh[1],
               mesh[2], nullptr, nullptr, nullptr);
}

int fisdf_fft3d_paired(fisdf_ctx* c, const void* in, void* out, int rows, const int mesh[3],
                       const double kd[3], const int m[3], int in_real) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(in && out && mesh && rows >= 0, "fft3d_paired: bad arguments");
  FISDF_CHECK(!in_real || in != out, "fft3d_paired: real input needs an output buffer of its own");
  long ng = (long)mesh[0] * mesh[1] * mesh[2];
  return fft3d(c->stream, (const cplx*)in, ng, nullptr, (cplx*)out, ng, rows, mesh[0], mesh[1],
               mesh[2], kd, nullptr, nullptr, nullptr, m, in_real != 0);
}

int fisdf_fft3d_ex(fisdf_ctx* c, const void* in, long in_ld, const int* rowidx, void* out,
                   long out_ld, int rows, const int mesh[3], const double* h_kd,
                   const double* weight, const long* h_plane_base, const long* h_plane_ld,
                   const int* h_m, int in_real, int* h_path) {
  FISDF_TRY(device_guard(c));
  if (h_path) *h_path = -1;
  FISDF_CHECK(in && out && mesh && rows >= 0, "fft3d_ex: bad arguments");
  FISDF_CHECK(mesh[0] >= 1 && mesh[1] >= 1 && mesh[2] >= 1, "fft3d_ex: bad mesh");
  FISDF_CHECK((h_plane_base == nullptr) == (h_plane_ld == nullptr),
              "fft3d_ex: the plane table is two arrays (base and ld) or none");
  // the plane table lives in a device buffer of this call: freed after a stream sync
  PlaneRef* planes = nullptr;
  if (h_plane_base) {
    std::vector<PlaneRef> h(mesh[0]);
    for (int i0 = 0; i0 < mesh[0]; ++i0) h[i0] = PlaneRef{h_plane_base[i0], h_plane_ld[i0]};
    FISDF_HIP(hipMalloc(&planes, sizeof(PlaneRef) * mesh[0]));
    if (hipMemcpy(planes, h.data(), sizeof(PlaneRef) * mesh[0], hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(planes);
      FISDF_CHECK(false, "fft3d_ex: plane table upload failed");
    }
  }
  const int rc = fft3d(c->stream, (const cplx*)in, in_ld, rowidx, (cplx*)out, out_ld, rows, mesh[0],
                       mesh[1], mesh[2], h_kd, weight, nullptr, planes, h_m, in_real != 0);
  if (planes) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(planes);
  }
  if (rc == 0 && rows > 0 && h_path) *h_path = fft3d_route(mesh[0], mesh[1], mesh[2], h_m);
  return rc;
}

int fisdf_coulg(fisdf_ctx* c, const int mesh[3], const double a[9], const double k[3],
                double scale, int take_sqrt, double* w) {
  FISDF_TRY(device_guard(c));
  CellGeom g;
  lattice(a, g);
  return coulg_weight(c->stream, mesh, g, k, scale, take_sqrt, w, c->omega);
}

int fisdf_min_norm_operator(fisdf_ctx* c, const void* A, int n, double tol_rel, void* M,
                            void* Qo, void* Rio, int* h_piv, int* h_rank) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(n >= 1, "min_norm_operator: bad size");
  Carver cv;
  size_t oL = cv.take(sizeof(cplx) * (size_t)n * n);
  size_t oP = cv.take(sizeof(int) * (size_t)n);
  size_t oR = cv.take(sizeof(int));
  size_t oD = cv.take(sizeof(double) * (size_t)n);
  size_t oF = cv.take(sizeof(int) * 4);
  size_t oW = cv.take(sizeof(double) * (size_t)(1 + n));
  size_t oM = cv.take(min_norm_work_bytes(n, n));
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  char* b = (char*)base;
  void* trail = nullptr;
  FISDF_TRY(devbuf_get(c->ws_main, sizeof(cplx) * pchol_trail_elems(n, 1), &trail));
  FISDF_TRY(pchol(c->stream, (const cplx*)A, n, (long)n * n, n, 1, n, tol_rel, 0.0, (cplx*)(b + oL),
                  (int*)(b + oP), (int*)(b + oR), (double*)(b + oD), (int*)(b + oF),
                  (double*)(b + oW), (cplx*)trail));
  int r = 0;
  FISDF_HIP(hipMemcpyAsync(&r, b + oR, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  FISDF_CHECK(r >= 1, "min_norm_operator: zero matrix");
  FISDF_HIP(hipMemsetAsync(M, 0, sizeof(cplx) * (size_t)n * n, c->stream));
  FISDF_TRY(min_norm_operator(c->stream, (const cplx*)(b + oL), n, n, (int*)(b + oP), r, (cplx*)M, n,
                              b + oM, (int*)(b + oF), (cplx*)Qo, (cplx*)Rio));
  int fl[3] = {0, 0, 0};
  FISDF_HIP(hipMemcpyAsync(fl, b + oF, sizeof(fl), hipMemcpyDeviceToHost, c->stream));
  FISDF_HIP(hipMemcpyAsync(h_piv, b + oP, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  FISDF_CHECK(fl[0] == 0 && fl[1] == 0 && fl[2] == 0, "min_norm_operator: CholeskyQR breakdown");
  *h_rank = r;
  return 0;
}

int fisdf_pivoted_cholesky(fisdf_ctx* c, const void* A, int n, int batch, int rmax,
                           double tol_rel, int* h_piv, int* h_rank) {
  FISDF_TRY(device_guard(c));
  Carver cv;
  size_t oL = cv.take(sizeof(cplx) * (size_t)batch * n * rmax);
  size_t oP = cv.take(sizeof(int) * (size_t)batch * rmax);
  size_t oR = cv.take(sizeof(int) * batch);
  size_t oD = cv.take(sizeof(double) * (size_t)batch * n);
  size_t oF = cv.take(sizeof(int) * batch);
  size_t oW = cv.take(sizeof(double) * (size_t)batch * (1 + rmax));
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  char* b = (char*)base;
  void* trail = nullptr;
  FISDF_TRY(devbuf_get(c->ws_main, sizeof(cplx) * pchol_trail_elems(n, batch), &trail));
  FISDF_TRY(pchol(c->stream, (const cplx*)A, n, (long)n * n, n, batch, rmax, tol_rel, 0.0,
                  (cplx*)(b + oL), (int*)(b + oP), (int*)(b + oR), (double*)(b + oD),
                  (int*)(b + oF), (double*)(b + oW), (cplx*)trail));
  FISDF_HIP(hipMemcpyAsync(h_piv, b + oP, sizeof(int) * (size_t)batch * rmax,
                           hipMemcpyDeviceToHost, c->stream));
  FISDF_HIP(hipMemcpyAsync(h_rank, b + oR, sizeof(int) * batch, hipMemcpyDeviceToHost, c->stream));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int fisdf_cholesky(fisdf_ctx* c, void* A, int n, int batch, double tol_rel, int* h_fail) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(n >= 1 && batch >= 1, "cholesky: bad sizes");
  Carver cv;
  size_t oW = cv.take(sizeof(cplx) * (size_t)batch * 4096 + sizeof(double) * batch);
  size_t oP = cv.take(sizeof(int) * (size_t)batch * n);
  size_t oR = cv.take(sizeof(int) * batch);
  size_t oF = cv.take(sizeof(int) * batch);
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  char* b = (char*)base;
  FISDF_TRY(chol_unpivoted(c->stream, (cplx*)A, n, batch, tol_rel, (int*)(b + oP), (int*)(b + oR),
                           (int*)(b + oF), (cplx*)(b + oW)));
  FISDF_HIP(hipMemcpyAsync(h_fail, b + oF, sizeof(int) * batch, hipMemcpyDeviceToHost, c->stream));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int fisdf_tri_inverse(fisdf_ctx* c, const void* L, int n, int batch, void* Linv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(n >= 1 && batch >= 1, "tri_inverse: bad sizes");
  const long nn = (long)n * n, we = std::max(1L, trsm_split_work_elems(n, batch));
  Carver cv;
  size_t oQ = cv.take(sizeof(cplx) * (size_t)batch * nn);
  size_t oK = cv.take(sizeof(cplx) * (size_t)we);
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  cplx* Q = (cplx*)((char*)base + oQ);
  // the factor stage's own sequence (factor_finish): block-row operator, then the merged
  // substitution applied to the identity
  FISDF_TRY(build_trsm_q(c->stream, (const cplx*)L, n, nn, Q, batch, GEMM_FULL));
  FISDF_TRY(set_identity(c->stream, (cplx*)Linv, n, batch));
  FISDF_TRY(trsm_merged_batched(c->stream, Q, nn, n, (cplx*)Linv, n, nn, n, batch, true,
                                (cplx*)((char*)base + oK), we));
  return 0;
}

// ---- the factor-and-solve chain piece by piece, for tests of its dispatch (thin forwards) ----
int fisdf_pivoted_cholesky_ex(fisdf_ctx* c, const void* A, long lda, long sA, int n, int batch,
                              int rmax, double tol_rel, double tol_abs, void* Lf, int* d_piv,
                              int* d_rank, int* h_path) {
  FISDF_TRY(device_guard(c));
  if (h_path) *h_path = -1;
  FISDF_CHECK(A && Lf && d_piv && d_rank, "pivoted_cholesky_ex: null argument");
  FISDF_CHECK(n >= 1 && batch >= 1 && rmax >= 1 && rmax <= n, "pivoted_cholesky_ex: bad sizes");
  FISDF_CHECK(lda >= n && (batch == 1 || sA >= (long)(n - 1) * lda + n),
              "pivoted_cholesky_ex: lda / batch stride smaller than the matrix");
  Carver cv;
  size_t oD = cv.take(sizeof(double) * (size_t)batch * n);
  size_t oF = cv.take(sizeof(int) * batch);
  size_t oW = cv.take(sizeof(double) * (size_t)batch * (1 + rmax));
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  char* b = (char*)base;
  void* trail = nullptr;
  FISDF_TRY(devbuf_get(c->ws_main, sizeof(cplx) * pchol_trail_elems(n, batch), &trail));
  FISDF_TRY(pchol(c->stream, (const cplx*)A, lda, sA, n, batch, rmax, tol_rel, tol_abs, (cplx*)Lf,
                  d_piv, d_rank, (double*)(b + oD), (int*)(b + oF), (double*)(b + oW),
                  (cplx*)trail));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  if (h_path) *h_path = pchol_path(n);
  return 0;
}

int fisdf_gather_lp(fisdf_ctx* c, const void* Lf, int n, int rmax, const int* d_piv,
                    const int* d_rank, int rpad, void* Lp, int batch) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(n >= 1 && rmax >= 1 && rmax <= n && rpad >= 0 && rpad <= rmax && batch >= 0,
              "gather_lp: bad sizes");
  FISDF_TRY(gather_lp(c->stream, (const cplx*)Lf, n, rmax, d_piv, d_rank, rpad, (cplx*)Lp, batch));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int fisdf_trsm_blocked_ex(fisdf_ctx* c, int lower, const void* Lp, long ldl, long sL, int r,
                          void* B, long ldb, long sB, void* X, long ldx, long sX, int ncol,
                          int batch, int a_real) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(r >= 1 && ncol >= 1 && batch >= 1 && ldl >= r && ldb >= ncol && ldx >= ncol,
              "trsm_blocked_ex: bad sizes");
  const int nb = 64, nblk = (r + nb - 1) / nb;  // the product's block (f_nb)
  const long sLi = (long)nblk * nb * nb;
  void* base;
  FISDF_TRY(arena_get(c, sizeof(cplx) * (size_t)sLi * batch, &base));
  // the diagonal-block inverses as factor_finish builds them
  FISDF_TRY(trinv_blocks(c->stream, (const cplx*)Lp, r, (int)ldl, sL, nb, sLi, (cplx*)base, batch));
  FISDF_TRY(trsm_blocked(c->stream, lower, (const cplx*)Lp, ldl, sL, r, (const cplx*)base, sLi, nb,
                         (cplx*)B, ldb, sB, (cplx*)X, ldx, sX, ncol, batch, a_real));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int fisdf_trsm_merged_ex(fisdf_ctx* c, const void* Lp, long sL, int r, void* X, long ld, long sX,
                         int ncol, int batch, int lower_rhs, int use_work, long work_elems,
                         int* h_rows, int rows_cap) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(r >= 1 && ncol >= 1 && batch >= 1 && ld >= ncol && work_elems >= 0,
              "trsm_merged_ex: bad sizes");
  const int nblk = trsm_merged_blocks(r);
  FISDF_CHECK(!h_rows || rows_cap >= nblk, "trsm_merged_ex: h_rows too short");
  const long rr = (long)r * r;
  Carver cv;
  size_t oQ = cv.take(sizeof(cplx) * (size_t)batch * rr);
  size_t oK = cv.take(sizeof(cplx) * (size_t)std::max(1L, work_elems));
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  cplx* Q = (cplx*)((char*)base + oQ);
  cplx* work = use_work ? (cplx*)((char*)base + oK) : nullptr;
  if (h_rows)
    for (int b = 0; b < nblk; ++b) {
      TrsmRow row;
      trsm_merged_row(r, ncol, batch, lower_rhs != 0, use_work != 0, work_elems, b, &row);
      const int v[6] = {row.b0, row.m, row.b1, row.nc, row.ks, row.sub};
      std::memcpy(h_rows + 6 * b, v, sizeof(v));
    }
  FISDF_TRY(build_trsm_q(c->stream, (const cplx*)Lp, r, sL, Q, batch, GEMM_FULL));
  const int rc = trsm_merged_batched(c->stream, Q, rr, r, (cplx*)X, ld, sX, ncol, batch,
                                     lower_rhs != 0, work, use_work ? work_elems : 0);
  FISDF_HIP(hipStreamSynchronize(c->stream));
  return rc;
}

int fisdf_scatter_w(fisdf_ctx* c, const void* Wpp, int ldw, long sW, int rmax, const int* d_piv,
                    const int* d_rank, void* W, int nip, int batch) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(nip >= 1 && rmax >= 0 && rmax <= nip && ldw >= rmax && batch >= 0,
              "scatter_w: bad sizes");
  FISDF_TRY(scatter_w(c->stream, (const cplx*)Wpp, ldw, sW, rmax, d_piv, d_rank, (cplx*)W, nip,
                      batch));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int fisdf_conj_transpose(fisdf_ctx* c, const void* A, int n, long sA, void* B, int batch) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(n >= 1 && batch >= 0 && A != B, "conj_transpose: bad arguments");
  FISDF_TRY(conj_transpose(c->stream, (const cplx*)A, n, sA, (cplx*)B, batch));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int fisdf_factor_plan(int n, int ncol, int batch, long work_elems, int* h_pchol_path,
                      int* h_pchol_nb, int* h_nblk, int* h_s0, int* h_rows, int rows_cap,
                      long* h_split_work_elems, int* h_sel_rpt, int* h_sel_nb) {
  t_cur_ctx = nullptr;
  FISDF_CHECK(n >= 1 && ncol >= 1 && batch >= 1, "factor_plan: bad sizes");
  const int nblk = trsm_merged_blocks(n);
  FISDF_CHECK(!h_rows || rows_cap >= nblk, "factor_plan: h_rows too short");
  if (h_pchol_path) *h_pchol_path = pchol_path(n);
  if (h_pchol_nb) *h_pchol_nb = PCHOL_NB;
  if (h_nblk) *h_nblk = nblk;
  TrsmRow row;
  trsm_merged_row(n, ncol, batch, false, false, 0, 0, &row);
  if (h_s0) *h_s0 = row.m;
  if (h_rows)
    for (int b = 0; b < nblk; ++b) {
      TrsmRow full, low;
      trsm_merged_row(n, ncol, batch, false, work_elems >= 0, work_elems, b, &full);
      trsm_merged_row(n, ncol, batch, true, work_elems >= 0, work_elems, b, &low);
      const int v[8] = {full.b0, full.m, full.b1, full.ks, full.sub, low.nc, low.ks, low.sub};
      std::memcpy(h_rows + 8 * b, v, sizeof(v));
    }
  if (h_split_work_elems) *h_split_work_elems = trsm_split_work_elems(n, batch);
  int rpt = 0, nb = 0;
  pchol_real_variant(n, &rpt, &nb);
  if (h_sel_rpt) *h_sel_rpt = rpt;
  if (h_sel_nb) *h_sel_nb = nb;
  return 0;
}

// ---- A1 ---------------------------------------------------------------------
// The streamed y build's work on aux[2] and aux[0], enqueued right after the selection kernel (so
// it never precedes it on any queue): the fused y kernel block by block, each block's XT rows
// waiting on the kernel's progress word (y_fused_stream).  Ordered after everything on `stream`
// before the selection (the previous build's readers of the y buffer and workspaces included).
static int ensure_side(fisdf_ctx* c);

static int ystream_enqueue(fisdf_ctx* c, const int* piv) {
  fisdf_ctx::YStream& Y = c->ys;
  // the side stream first, then the aux streams: the order the unstreamed build creates them in
  // (the runtime places a process's streams on hardware queues in creation order, and the fit's
  // two lanes serialise when aux[0] lands elsewhere: C3 89 vs 81 ms/step, profiles/r06/lanes/)
  FISDF_TRY(ensure_side(c));
  FISDF_TRY(ensure_aux(c));
  const int nq = (int)Y.qs.size();
  const size_t yw = y_fused_workspace(Y.kmesh, Y.nip, Y.nao, (int)Y.m);
  FISDF_CHECK(yw > 0 && nq > 0, "streamed y: the fused kernel does not apply");
  void* wb = nullptr;
  FISDF_TRY(devbuf_get(c->ws_ystream, yw, &wb));
  // the aux stream that carries the streamed y: aux[2], the fit's FFT stream, whose FFTs then
  // follow y in stream order (C3 79.8 / 79.4 ms/step against 81.6 / 81.2 on aux[1] and 79.9 on
  // aux[0], profiles/r06/lanes2-3); FISDF_Y_STREAM_AUX (read per build) for A/B
  const int ia = [] {
    const char* e = getenv("FISDF_Y_STREAM_AUX");
    const int v = e ? atoi(e) : 2;
    return (v >= 0 && v <= 2) ? v : 2;
  }();
  c->ys.aux = ia;
  hipStream_t ys = c->aux[ia];
  aux_fork(c, ia);
  FISDF_HIP(hipStreamWaitEvent(ys, c->ev_ysfork, 0));
  // blocks alternate over aux[ia] and a second aux stream (one block's tail overlaps the next
  // one's start), ordered back into aux[ia] at the end, so joining aux[ia] joins both: C3 in one
  // process 79.05 / 79.30 against 79.52 / 79.59 ms/step on one stream (profiles/r06/ab11-12);
  // FISDF_Y_STREAM_2S=0 (read per build) keeps one stream
  const char* e2 = getenv("FISDF_Y_STREAM_2S");
  const int i2 = (e2 && e2[0] == '0') ? -1 : (ia == 0 ? 1 : 0);
  if (i2 >= 0 && !c->ev_ys2[0]) {
    FISDF_HIP(hipEventCreateWithFlags(&c->ev_ys2[0], hipEventDisableTiming));
    FISDF_HIP(hipEventCreateWithFlags(&c->ev_ys2[1], hipEventDisableTiming));
  }
  // (a round-6 experiment held the blocks after the first until x4 was done, on a device flag the
  // build set: x4 1.3 ms instead of 3.0, but the factor chain after it 5.2 instead of 4.1 ms and
  // the step 0.5-1 ms slower, profiles/r06/r06_gate.  Removed: a host-side device synchronisation
  // before the flag was set — a workspace growth, a hipFree — waited for the held blocks until
  // their bounded wait expired)
  bool handled = false;
  {
    StageTimer tm(c, FISDF_ST_Y, ys);
    FISDF_TRY(y_fused_stream(ys, Y.x0, Y.ng0, Y.nao, piv, c->ys_dev, c->ys_dev + 1, Y.nip, Y.rows,
                             Y.f, Y.fks, (int)Y.m, Y.kmesh, Y.qs.data(), nq, Y.yT,
                             (long)Y.nip * Y.m, Y.m, 0, (cplx*)wb, yw, Y.rmask, &handled,
                             i2 >= 0 ? c->aux[i2] : nullptr, c->ev_ys2[0], c->ev_ys2[1]));
  }
  // aux[i2]'s work is ordered before aux[ia]'s last command: joined with it (buffer-return
  // bookkeeping, check_aux_joined)
  if (i2 >= 0) {
    aux_fork(c, i2);
    c->aux_joined[i2] = c->aux_use[i2];
  }
  FISDF_CHECK(handled, "streamed y: nothing enqueued");
  Y.enqueued = true;
  return 0;
}

// after the selection: whether yT holds the y build of the selected points (the selection gave
// the cap's points, its first pass did not fail, the q-list is the armed one); the y stream's
// spin-error flag is queued for read-back (ev_yerr).  The caller joins the y stream (ystream_join).
static bool ystream_valid(fisdf_ctx* c, int nip, const int* qs, int nq) {
  const fisdf_ctx::YStream& Y = c->ys;
  return Y.enqueued && !Y.stale && nip == Y.nip && (int)Y.qs.size() == nq &&
         std::equal(Y.qs.begin(), Y.qs.end(), qs);
}

static int ystream_join(fisdf_ctx* c) {
  const int ia = c->ys.aux;
  if (!c->ys.enqueued || c->aux_joined[ia] == c->aux_use[ia]) return 0;
  FISDF_TRY(aux_join(c, ia));
  FISDF_HIP(hipMemcpyAsync(c->ys_err_pinned, c->ys_dev + 1, sizeof(int), hipMemcpyDeviceToHost,
                           c->stream));
  FISDF_HIP(hipEventRecord(c->ev_yerr, c->stream));
  return 0;
}

// the streamed y's bounded waits all met their pivots (call after ystream_join)
static int ystream_check(fisdf_ctx* c) {
  FISDF_HIP(hipEventSynchronize(c->ev_yerr));
  FISDF_CHECK(*c->ys_err_pinned == 0, "streamed y: the selection's progress never arrived");
  return 0;
}

// arm the streamed y for the next selection: y_q (q in qs, ascending) of rows [0, nip_max) on m
// grid points (f: k stride fks) into yT[slot][I][g], self-conjugate q in rmask stored real.
// *armed = false when the fused kernel does not cover the k-mesh (nothing will stream).
static int ystream_arm(fisdf_ctx* c, const void* x0, int ng0, const void* f, long fks, long m,
                       int nao, int nip_max, const int kmesh[3], const int* qs, int nq, void* yT,
                       unsigned long long rmask, bool* armed) {
  *armed = false;
  FISDF_TRY(ystream_join(c));  // a streamed y never finished (an error in between) is joined
  c->ys = fisdf_ctx::YStream();
  if (nip_max <= 0 || m <= 0 || nq <= 0 || !y_fused_applies(kmesh, nao)) return 0;
  FISDF_CHECK(x0 && f && yT && qs, "y_stream_arm: null argument");
  if (!c->ys_dev) {
    FISDF_HIP(hipMalloc((void**)&c->ys_dev, 4 * sizeof(int)));
    FISDF_HIP(hipHostMalloc((void**)&c->ys_err_pinned, sizeof(int), hipHostMallocDefault));
    FISDF_HIP(hipEventCreateWithFlags(&c->ev_yerr, hipEventDisableTiming));
    FISDF_HIP(hipEventCreateWithFlags(&c->ev_ysfork, hipEventDisableTiming));
  }
  fisdf_ctx::YStream& Y = c->ys;
  Y.x0 = (const cplx*)x0;
  Y.f = (const cplx*)f;
  Y.fks = fks;
  Y.m = m;
  Y.ng0 = ng0;
  Y.nao = nao;
  Y.nip = std::min(nip_max, ng0);
  for (int i = 0; i < 3; ++i) Y.kmesh[i] = kmesh[i];
  Y.qs.assign(qs, qs + nq);
  Y.yT = (cplx*)yT;
  Y.rmask = rmask;
  // pivots per block, FISDF_Y_STREAM_ROWS (a multiple of 16; read per build): 128 — C3 in one
  // process, 4 interleaved rounds: 64 rows 78.77, 128 78.29, 192 78.23, 256 78.45, unstreamed
  // 79.96 ms/step (profiles/r06/ab9_inproc.json); fewer, larger launches beat an earlier start
  const int rows_env = [] {
    const char* e = getenv("FISDF_Y_STREAM_ROWS");
    const int v = e ? atoi(e) : 128;
    return (v >= 16 && v % 16 == 0 && v <= 1024) ? v : 128;
  }();
  Y.rows = rows_env;
  Y.armed = true;
  *armed = true;
  return 0;
}

// The selection's work area: the n x n complex x4 of the generic path, which also holds the
// co-resident kernels' scratch (their plans check it against n*n doubles) and the register panels'
// n*n + 17 n + 1 doubles (pchol_select_real) — the larger below n = 18, where a work area of n*n
// complex let the panels' L panel and diagonal run over the pivots and the rank behind it
static size_t select_work_bytes(int n) {
  const size_t nn = (size_t)n * n;
  return std::max(sizeof(cplx) * nn, sizeof(double) * (nn + 17 * (size_t)n + 1));
}

// The selection's pivots on the device: the cooperative kernel, the blocked or the generic pivoted
// Cholesky (in that order of preference), then ONE pinned read-back of {error flag, rank, pivots}
// and one stream synchronisation (round 2 synchronised twice through pageable copies); a
// cooperative run that reports a stalled step is redone on the non-cooperative paths.
static int select_pivots_dev(fisdf_ctx* c, const cplx* X2, double scale, int ng0, int nip_max,
                             double tol, cplx* X4, int* piv, int* rank, cplx* L, double* d,
                             int* flags, double* w, int* h_perm, int* h_rank,
                             const SelOpts* opt = nullptr, int* h_info = nullptr) {
  const size_t nint = 2 + (size_t)nip_max;
  if (c->sel_cap < nint) {
    if (c->sel_pinned) FISDF_HIP(hipHostFree(c->sel_pinned));
    c->sel_pinned = nullptr;
    c->sel_cap = 0;
    FISDF_HIP(hipHostMalloc((void**)&c->sel_pinned, sizeof(int) * nint, hipHostMallocDefault));
    c->sel_cap = nint;
  }
  // an armed streamed y (build_impl, fisdf_y_stream_arm) is for this selection only
  const bool armed = c->ys.armed;
  c->ys.armed = false;
  for (int pass = 0; pass < 2; ++pass) {
    bool handled = false;
    const int* coop_err = nullptr;
    // a streamed y build reads the pivots while the kernel runs: the selection then writes them
    // to the context's own buffer and publishes its progress
    const bool stream_y = armed && pass == 0 && c->ys.nip == nip_max;
    int* progress = nullptr;
    if (stream_y) {
      void* pp = nullptr;
      FISDF_TRY(devbuf_get(c->ws_ypiv, sizeof(int) * (size_t)nip_max, &pp));
      piv = (int*)pp;
      progress = c->ys_dev;
      FISDF_HIP(hipMemsetAsync(c->ys_dev, 0, 2 * sizeof(int), c->stream));
      // the y stream starts from here, beside the kernel (not after it)
      FISDF_HIP(hipEventRecord(c->ev_ysfork, c->stream));
    }
    bool publishes = false;
    SelRan ran = {};
    FISDF_TRY(pchol_select_real(c->stream, X2, scale, ng0, nip_max, tol, piv, rank, (double*)X4,
                                flags, &handled, pass == 0, &coop_err, progress, &publishes, opt,
                                &ran));
    if (stream_y) {
      // whatever ran, consumers waiting on the progress word are released when it has ended
      FISDF_HIP(hipMemsetD32Async(c->ys_dev, kSelDone, 1, c->stream));
      if (handled && publishes) FISDF_TRY(ystream_enqueue(c, piv));
    }
    if (!handled) {
      FISDF_TRY(square_scale(c->stream, X2, scale, X4, (long)ng0 * ng0));
      void* trail = nullptr;
      FISDF_TRY(devbuf_get(c->ws_main, sizeof(cplx) * pchol_trail_elems(ng0, 1), &trail));
      FISDF_TRY(pchol(c->stream, X4, ng0, 0, ng0, 1, nip_max, tol, 0.0, L, piv, rank, d, flags, w,
                      (cplx*)trail));
      const bool blk = pchol_path(ng0) == PCHOL_BLOCKED;
      ran = SelRan{blk ? SEL_RAN_PCHOL_BLOCKED : SEL_RAN_PCHOL_STEP, 0, 0, blk ? PCHOL_NB : 0, 0};
    }
    int* hp = c->sel_pinned;
    hp[0] = 0;
    if (coop_err)
      FISDF_HIP(hipMemcpyAsync(hp, coop_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    FISDF_HIP(hipMemcpyAsync(hp + 1, rank, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    FISDF_HIP(hipMemcpyAsync(hp + 2, piv, sizeof(int) * nip_max, hipMemcpyDeviceToHost, c->stream));
    FISDF_HIP(hipStreamSynchronize(c->stream));
    if (stream_y && hp[0] != 0) c->ys.stale = true;
    if (hp[0] == 0) {
      *h_rank = hp[1];
      // the _ex entry (h_info) receives the rank's pivots only: what lies beyond is the caller's
      const int ncopy = h_info ? std::max(0, std::min(hp[1], nip_max)) : nip_max;
      std::memcpy(h_perm, hp + 2, sizeof(int) * ncopy);
      if (h_info) {
        const int v[6] = {ran.kernel, ran.G, ran.RW, ran.K, ran.tpr, pass + 1};
        std::memcpy(h_info, v, sizeof(v));
      }
      return 0;
    }
  }
  FISDF_CHECK(false, "select: pivoted Cholesky failed on every path");
  return 0;
}

static int select_points_impl(fisdf_ctx* c, const void* x0v, int nk, const int* kmesh, int ng0,
                              int nao, int nip_max, double tol, int* h_perm, int* h_npiv,
                              int* h_full_rank);

int fisdf_select_points(fisdf_ctx* c, const void* x0v, int nk, int ng0, int nao, int nip_max,
                        double tol, int* h_perm, int* h_npiv, int* h_full_rank) {
  FISDF_TRY(device_guard(c));
  return select_points_impl(c, x0v, nk, nullptr, ng0, nao, nip_max, tol, h_perm, h_npiv,
                            h_full_rank);
}

int fisdf_select_points_km(fisdf_ctx* c, const void* x0v, const int kmesh[3], int ng0, int nao,
                           int nip_max, double tol, int* h_perm, int* h_npiv, int* h_full_rank) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(kmesh && kmesh[0] > 0 && kmesh[1] > 0 && kmesh[2] > 0, "select_points: bad k-mesh");
  return select_points_impl(c, x0v, kmesh[0] * kmesh[1] * kmesh[2], kmesh, ng0, nao, nip_max, tol,
                            h_perm, h_npiv, h_full_rank);
}

static int select_points_impl(fisdf_ctx* c, const void* x0v, int nk, const int* kmesh, int ng0,
                              int nao, int nip_max, double tol, int* h_perm, int* h_npiv,
                              int* h_full_rank) {
  FISDF_CHECK(nk > 0 && ng0 > 0 && nao > 0 && nip_max > 0, "select_points: bad sizes");
  nip_max = std::min(nip_max, ng0);
  StageTimer tm(c, FISDF_ST_SELECT);
  const cplx* x0 = (const cplx*)x0v;
  Carver cv;
  size_t oX2 = cv.take(sizeof(cplx) * (size_t)ng0 * ng0);
  size_t oX4 = cv.take(select_work_bytes(ng0));
  size_t oPm = cv.take(sizeof(cplx) * (size_t)ng0 * nk * nao);
  size_t oL = cv.take(sizeof(cplx) * (size_t)ng0 * nip_max);
  size_t oP = cv.take(sizeof(int) * nip_max);
  size_t oR = cv.take(sizeof(int) * 4);
  size_t oD = cv.take(sizeof(double) * ng0);
  size_t oF = cv.take(sizeof(int) * 4);
  size_t oW = cv.take(sizeof(double) * (1 + nip_max));
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  char* b = (char*)base;
  cplx* X2 = (cplx*)(b + oX2);
  cplx* X4 = (cplx*)(b + oX4);
  // x2 = sum_q conj(x0_q) x0_q^T   (fftisdf.py:376-378; real part taken below) as one
  // K = nk*nao Hermitian rank-K update of the permuted x0
  FISDF_TRY(select_gram(c, x0, nk, 0, nk, ng0, nao, X2, (cplx*)(b + oPm), kmesh,
                        c->time_reversal != 0));
  // x4 = Re(x2)^2 / nk (:379) and the greedy pivoted Cholesky (:381-384), first nip_max
  // pivots: real blocked panels (X4's storage holds the real trailing matrix)
  int rank = 0;
  FISDF_TRY(select_pivots_dev(c, X2, 1.0 / nk, ng0, nip_max, tol, X4, (int*)(b + oP),
                              (int*)(b + oR), (cplx*)(b + oL), (double*)(b + oD), (int*)(b + oF),
                              (double*)(b + oW), h_perm, &rank));
  *h_npiv = rank;
  if (h_full_rank) *h_full_rank = rank < nip_max ? 1 : 0;
  return 0;
}

int fisdf_select_gram(fisdf_ctx* c, const void* x0, int nk, int q0, int q1, int ng0, int nao,
                      void* x2) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(0 <= q0 && q0 <= q1 && q1 <= nk && ng0 > 0 && nao > 0, "select_gram: bad sizes");
  StageTimer tm(c, FISDF_ST_SELECT);
  if (q1 == q0) {
    FISDF_HIP(hipMemsetAsync(x2, 0, sizeof(cplx) * (size_t)ng0 * ng0, c->stream));
    return 0;
  }
  void* base;
  FISDF_TRY(arena_get(c, sizeof(cplx) * (size_t)ng0 * (q1 - q0) * nao, &base));
  return select_gram(c, (const cplx*)x0, nk, q0, q1, ng0, nao, (cplx*)x2, (cplx*)base, nullptr,
                     false);
}

static int select_gram_plan_checked(const int* kmesh, int fold, int nk, int q0, int q1, int ng0,
                                    int nao, int* h_info) {
  FISDF_CHECK(h_info && nk > 0 && 0 <= q0 && q0 <= q1 && q1 <= nk && ng0 > 0 && nao > 0,
              "select_gram_plan: bad sizes");
  FISDF_CHECK(!kmesh || (kmesh[0] > 0 && kmesh[1] > 0 && kmesh[2] > 0 &&
                         (long)kmesh[0] * kmesh[1] * kmesh[2] == nk),
              "select_gram_plan: the k-mesh does not have nk points");
  FISDF_CHECK(!fold || (kmesh && q0 == 0 && q1 == nk),
              "select_gram_plan: the fold needs the k-mesh and the whole of it");
  select_gram_plan(kmesh, fold != 0, q1 - q0, ng0, nao, h_info);
  return 0;
}

int fisdf_select_gram_plan(const int* kmesh, int fold, int nk, int q0, int q1, int ng0, int nao,
                           int* h_info) {
  t_cur_ctx = nullptr;
  return select_gram_plan_checked(kmesh, fold, nk, q0, q1, ng0, nao, h_info);
}

int fisdf_select_gram_ex(fisdf_ctx* c, const void* x0, const int* kmesh, int fold, int nk, int q0,
                         int q1, int ng0, int nao, void* x2, int* h_info) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(x0 && x2, "select_gram_ex: null argument");
  int info[3];
  FISDF_TRY(select_gram_plan_checked(kmesh, fold, nk, q0, q1, ng0, nao, info));
  if (q1 == q0) {
    FISDF_HIP(hipMemsetAsync(x2, 0, sizeof(cplx) * (size_t)ng0 * ng0, c->stream));
  } else {
    void* base;
    FISDF_TRY(arena_get(c, sizeof(cplx) * (size_t)ng0 * (q1 - q0) * nao, &base));
    FISDF_TRY(select_gram(c, (const cplx*)x0, nk, q0, q1, ng0, nao, (cplx*)x2, (cplx*)base, kmesh,
                          fold != 0));
  }
  FISDF_HIP(hipStreamSynchronize(c->stream));
  if (h_info) std::memcpy(h_info, info, sizeof(info));
  return 0;
}

int fisdf_select_plan(int n, int rmax, int ncu, int lds_cols, int wgs, int* h_mode, int* h_batch,
                      long* h_batch_lds, int* h_coop, long* h_coop_lds, int* h_panel,
                      int* h_pchol_path) {
  t_cur_ctx = nullptr;
  FISDF_CHECK(n >= 1 && rmax >= 1 && rmax <= n && ncu >= 0 && lds_cols >= 0 && wgs >= 0,
              "select_plan: bad sizes");
  SelBatchPlan bp;
  SelCoopPlan cp;
  select_batch_plan(n, rmax, ncu, &bp);
  select_coop_plan(n, rmax, ncu, lds_cols, wgs, &cp);
  if (h_mode) *h_mode = select_default_mode(rmax);
  if (h_batch) {
    const int v[4] = {bp.ok, bp.why, bp.grid, bp.RW};
    std::memcpy(h_batch, v, sizeof(v));
  }
  if (h_batch_lds) *h_batch_lds = bp.lds;
  if (h_coop) {
    const int v[7] = {cp.ok, cp.why, cp.split, cp.G, cp.RW, cp.K, cp.tpr};
    std::memcpy(h_coop, v, sizeof(v));
  }
  if (h_coop_lds) *h_coop_lds = cp.lds;
  if (h_panel) pchol_real_variant(n, h_panel, h_panel + 1);
  if (h_pchol_path) *h_pchol_path = pchol_path(n);
  return 0;
}

int fisdf_select_pivots_ex(fisdf_ctx* c, const void* x2, int nk, int ng0, int nip_max, double tol,
                           int mode, int lds_cols, int wgs, int* h_perm, int* h_npiv,
                           int* h_full_rank, int* h_info) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(x2 && h_perm && h_npiv && h_info, "select_pivots_ex: null argument");
  FISDF_CHECK(nk > 0 && ng0 > 0 && nip_max > 0 && nip_max <= ng0, "select_pivots_ex: bad sizes");
  FISDF_CHECK(mode >= -1 && mode <= 2 && lds_cols >= 0 && wgs >= 0,
              "select_pivots_ex: mode is -1..2, lds_cols and wgs are 0 or positive");
  StageTimer tm(c, FISDF_ST_SELECT);
  Carver cv;
  size_t oX4 = cv.take(select_work_bytes(ng0));
  size_t oL = cv.take(sizeof(cplx) * (size_t)ng0 * nip_max);
  size_t oP = cv.take(sizeof(int) * nip_max);
  size_t oR = cv.take(sizeof(int) * 4);
  size_t oD = cv.take(sizeof(double) * ng0);
  size_t oF = cv.take(sizeof(int) * 4);
  size_t oW = cv.take(sizeof(double) * (1 + nip_max));
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  char* b = (char*)base;
  const SelOpts opt = {mode, lds_cols, wgs};
  int rank = 0;
  FISDF_TRY(select_pivots_dev(c, (const cplx*)x2, 1.0 / nk, ng0, nip_max, tol, (cplx*)(b + oX4),
                              (int*)(b + oP), (int*)(b + oR), (cplx*)(b + oL), (double*)(b + oD),
                              (int*)(b + oF), (double*)(b + oW), h_perm, &rank, &opt, h_info));
  *h_npiv = rank;
  if (h_full_rank) *h_full_rank = rank < nip_max ? 1 : 0;
  return 0;
}

int fisdf_select_pivots(fisdf_ctx* c, const void* x2, int nk, int ng0, int nip_max, double tol,
                        int* h_perm, int* h_npiv, int* h_full_rank) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(nk > 0 && ng0 > 0 && nip_max > 0, "select_pivots: bad sizes");
  nip_max = std::min(nip_max, ng0);
  StageTimer tm(c, FISDF_ST_SELECT);
  Carver cv;
  size_t oX4 = cv.take(select_work_bytes(ng0));
  size_t oL = cv.take(sizeof(cplx) * (size_t)ng0 * nip_max);
  size_t oP = cv.take(sizeof(int) * nip_max);
  size_t oR = cv.take(sizeof(int) * 4);
  size_t oD = cv.take(sizeof(double) * ng0);
  size_t oF = cv.take(sizeof(int) * 4);
  size_t oW = cv.take(sizeof(double) * (1 + nip_max));
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  char* b = (char*)base;
  cplx* X4 = (cplx*)(b + oX4);
  int rank = 0;  // x4 = Re(x2)^2/nk (:379) + pivoted Cholesky (:381-384)
  FISDF_TRY(select_pivots_dev(c, (const cplx*)x2, 1.0 / nk, ng0, nip_max, tol, X4, (int*)(b + oP),
                              (int*)(b + oR), (cplx*)(b + oL), (double*)(b + oD), (int*)(b + oF),
                              (double*)(b + oW), h_perm, &rank));
  *h_npiv = rank;
  if (h_full_rank) *h_full_rank = rank < nip_max ? 1 : 0;
  return 0;
}

int fisdf_unpack_slices(fisdf_ctx* c, const void* recv, int nrows, int nparts, const long* h_g0,
                        const long* h_ng, long ngrid, void* yT) {
  FISDF_TRY(device_guard(c));
  StageTimer tm(c, FISDF_ST_Y);
  FISDF_CHECK(nrows >= 0 && nparts >= 0 && (nparts == 0 || (h_g0 && h_ng)), "unpack: bad sizes");
  for (int p = 0; p < nparts; ++p)  // every slice before the first copy: a refused call writes nothing
    FISDF_CHECK(h_g0[p] >= 0 && h_ng[p] >= 0 && h_g0[p] + h_ng[p] <= ngrid, "unpack: bad slice");
  FISDF_CHECK(nrows == 0 || nparts == 0 || (recv && yT), "unpack: null buffer");
  const char* src = (const char*)recv;
  for (int p = 0; p < nparts; ++p) {
    if (h_ng[p] == 0 || nrows == 0) continue;
    FISDF_HIP(hipMemcpy2DAsync((char*)yT + sizeof(cplx) * h_g0[p], sizeof(cplx) * ngrid, src,
                               sizeof(cplx) * h_ng[p], sizeof(cplx) * h_ng[p], nrows,
                               hipMemcpyDeviceToDevice, c->stream));
    src += sizeof(cplx) * (size_t)h_ng[p] * nrows;
  }
  return 0;
}

// ---- input layer: Bloch AO values -------------------------------------
namespace {

// fisdf_eval_ao / fisdf_eval_ao_deriv1: ncomp = 1 values, 4 values and first derivatives
int eval_ao_entry(fisdf_ctx* c, const void* d_coords, int ng, int natm, const double* h_atoms,
                  int nsh, const int* h_sh_atom, const int* h_sh_l, const int* h_sh_nprim,
                  const double* h_exps, const double* h_coefs, int nT, const int* h_tn,
                  const int* kmesh, const double* a, double rcut, int nao, void* d_out, int deriv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(kmesh && kmesh[0] > 0 && kmesh[1] > 0 && kmesh[2] > 0, "eval_ao: bad k-mesh");
  FISDF_CHECK(ng >= 0 && nT >= 0, "eval_ao: bad sizes");  // before they size the workspace
  StageTimer tm(c, FISDF_ST_AO);
  int nao_sh = 0;
  for (int i = 0; i < nsh; ++i) nao_sh += 2 * h_sh_l[i] + 1;
  FISDF_CHECK(nao_sh == nao, "eval_ao: nao does not match the shells");
  const int nimg = kmesh[0] * kmesh[1] * kmesh[2];
  const size_t ncomp = deriv ? 4 : 1;
  Carver cv;
  const size_t oF = cv.take(sizeof(double) * ncomp * (size_t)nimg * ng * nao);
  const size_t tables = 1 << 20;
  const size_t oT = cv.take(tables + sizeof(double) * 3 * (size_t)std::max(nT, 1));
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  char* b = (char*)base;
  int nao_out = 0;
  FISDF_TRY(eval_ao(c->stream, (const double*)d_coords, ng, natm, h_atoms, nsh, h_sh_atom,
                    h_sh_l, h_sh_nprim, h_exps, h_coefs, nT, h_tn, kmesh, a, rcut,
                    (double*)(b + oF), b + oT, tables + sizeof(double) * 3 * (size_t)std::max(nT, 1),
                    (cplx*)d_out, &nao_out, 0, nullptr, deriv));
  return 0;
}

int eval_ao_band_entry(fisdf_ctx* c, const void* d_coords, int ng, int natm, const double* h_atoms,
                       int nsh, const int* h_sh_atom, const int* h_sh_l, const int* h_sh_nprim,
                       const double* h_exps, const double* h_coefs, int nT, const int* h_tn,
                       int nkb, const double* h_kpts, const double* a, double rcut, int nao,
                       void* d_out, int deriv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(nkb > 0 && h_kpts != nullptr, "eval_ao_band: no band k-points");
  FISDF_CHECK(ng >= 0 && nT >= 0, "eval_ao_band: bad sizes");  // before they size the workspace
  StageTimer tm(c, FISDF_ST_AO);
  int nao_sh = 0;
  for (int i = 0; i < nsh; ++i) nao_sh += 2 * h_sh_l[i] + 1;
  FISDF_CHECK(nao_sh == nao, "eval_ao_band: nao does not match the shells");
  const int one[3] = {1, 1, 1};
  const size_t ncomp = deriv ? 4 : 1;
  Carver cv;
  const size_t oF = cv.take(sizeof(double) * ncomp * (size_t)std::max(nT, 1) * ng * nao);
  const size_t tables = (1 << 20) + sizeof(double) * 3 * (size_t)std::max(nT, 1) +
                        sizeof(cplx) * (size_t)std::max(nT, 1) * nkb + sizeof(int) * (nT + 2);
  const size_t oT = cv.take(tables);
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  char* b = (char*)base;
  int nao_out = 0;
  FISDF_TRY(eval_ao(c->stream, (const double*)d_coords, ng, natm, h_atoms, nsh, h_sh_atom, h_sh_l,
                    h_sh_nprim, h_exps, h_coefs, nT, h_tn, one, a, rcut, (double*)(b + oF), b + oT,
                    tables, (cplx*)d_out, &nao_out, nkb, h_kpts, deriv));
  return 0;
}

}  // namespace

int fisdf_eval_ao(fisdf_ctx* c, const void* d_coords, int ng, int natm, const double* h_atoms,
                  int nsh, const int* h_sh_atom, const int* h_sh_l, const int* h_sh_nprim,
                  const double* h_exps, const double* h_coefs, int nT, const int* h_tn,
                  const int* kmesh, const double* a, double rcut, int nao, void* d_out) {
  return eval_ao_entry(c, d_coords, ng, natm, h_atoms, nsh, h_sh_atom, h_sh_l, h_sh_nprim, h_exps,
                       h_coefs, nT, h_tn, kmesh, a, rcut, nao, d_out, 0);
}

int fisdf_eval_ao_band(fisdf_ctx* c, const void* d_coords, int ng, int natm, const double* h_atoms,
                       int nsh, const int* h_sh_atom, const int* h_sh_l, const int* h_sh_nprim,
                       const double* h_exps, const double* h_coefs, int nT, const int* h_tn,
                       int nkb, const double* h_kpts, const double* a, double rcut, int nao,
                       void* d_out) {
  return eval_ao_band_entry(c, d_coords, ng, natm, h_atoms, nsh, h_sh_atom, h_sh_l, h_sh_nprim,
                            h_exps, h_coefs, nT, h_tn, nkb, h_kpts, a, rcut, nao, d_out, 0);
}

// ---- AO first derivatives: d_out (nk, 4, ng, nao) ---------------------------
int fisdf_eval_ao_deriv1(fisdf_ctx* c, const void* d_coords, int ng, int natm,
                         const double* h_atoms, int nsh, const int* h_sh_atom, const int* h_sh_l,
                         const int* h_sh_nprim, const double* h_exps, const double* h_coefs, int nT,
                         const int* h_tn, const int* kmesh, const double* a, double rcut, int nao,
                         void* d_out) {
  return eval_ao_entry(c, d_coords, ng, natm, h_atoms, nsh, h_sh_atom, h_sh_l, h_sh_nprim, h_exps,
                       h_coefs, nT, h_tn, kmesh, a, rcut, nao, d_out, 1);
}

int fisdf_eval_ao_band_deriv1(fisdf_ctx* c, const void* d_coords, int ng, int natm,
                              const double* h_atoms, int nsh, const int* h_sh_atom,
                              const int* h_sh_l, const int* h_sh_nprim, const double* h_exps,
                              const double* h_coefs, int nT, const int* h_tn, int nkb,
                              const double* h_kpts, const double* a, double rcut, int nao,
                              void* d_out) {
  return eval_ao_band_entry(c, d_coords, ng, natm, h_atoms, nsh, h_sh_atom, h_sh_l, h_sh_nprim,
                            h_exps, h_coefs, nT, h_tn, nkb, h_kpts, a, rcut, nao, d_out, 1);
}

int fisdf_gather_points(fisdf_ctx* c, const void* x0, int nk, int ng0, int nao, const int* h_perm,
                        int nip, void* X) {
  FISDF_TRY(device_guard(c));
  void* base;
  FISDF_TRY(arena_get(c, sizeof(int) * (size_t)nip, &base));
  for (int i = 0; i < nip; ++i) FISDF_CHECK(h_perm[i] >= 0 && h_perm[i] < ng0, "perm out of range");
  // through the pinned staging buffer, stream-ordered (the arena's next user is enqueued after
  // the gather on the same stream): no host synchronisation
  FISDF_TRY(upload_ints(c, h_perm, nip, (int*)base));
  FISDF_TRY(gather_points(c->stream, (const cplx*)x0, nk, ng0, nao, (const int*)base, nip, (cplx*)X));
  return 0;
}

// ---- A2 ---------------------------------------------------------------------
// FISDF_X4_DFT=0: the x4 build through the two dense Phi GEMMs (A/B on one box)
static bool x4_dft_enabled() {  // read per call (A/B in one process)
  const char* e = getenv("FISDF_X4_DFT");
  return !(e && e[0] == '0');
}

static int build_x4_on(fisdf_ctx* c, hipStream_t st, fisdf_ctx::DevBuf* wsb, const void* Xv,
                       int nip, int nao, const int kmesh[3], const double a[9], void* x4v);

int fisdf_build_x4(fisdf_ctx* c, const void* Xv, int nip, int nao, const int kmesh[3],
                   const double a[9], void* x4v) {
  FISDF_TRY(device_guard(c));
  return build_x4_on(c, c->stream, nullptr, Xv, nip, nao, kmesh, a, x4v);
}

// x4 on stream st; wsb (optional): the x2_k workspace of the register path from this grow-only
// buffer instead of the arena (whose users are ordered on c->stream only)
static int build_x4_on(fisdf_ctx* c, hipStream_t st, fisdf_ctx::DevBuf* wsb, const void* Xv,
                       int nip, int nao, const int kmesh[3], const double a[9], void* x4v) {
  // before anything is enqueued: a k-mesh no k-mesh transform takes (the y build would refuse it
  // only after its first GEMM)
  FISDF_TRY(kmesh_check(kmesh, "build_x4"));
  FISDF_CHECK(nip >= 1 && nao >= 1, "build_x4: bad sizes");
  StageTimer tm(c, FISDF_ST_X4, st);
  const int nk = kmesh[0] * kmesh[1] * kmesh[2];
  const cplx* phase;
  FISDF_TRY(get_phase(c, kmesh, a, &phase));
  const cplx* X = (const cplx*)Xv;
  const long nn = (long)nip * nip;
  if (nk == 1) {
    // Gamma only: Phi = 1, so x2_s = x2_k and x4 = x2_s^2 (:45) straight from the x2 GEMM's
    // epilogue with the reality monitor of :43 (the two Phi GEMMs would run with M = 1)
    FISDF_TRY(zgemm(st, OP_R, OP_T, nip, nip, nao, ONE, X, nao, 0, X, nao, 0, ZERO,
                    (cplx*)x4v, nip, 0, 1, 1, nullptr, EPI_CSQUARE, c->maximag + 0));
    return 0;
  }
  if (x4_dft_enabled() && kmesh_y_reg_applies(kmesh, nn)) {
    // the k-mesh DFT pair of :41-46 per (I, J) column in registers (the y build's kmesh_y with
    // conj output: x4_k = Phi^H x4_s, x4_s real) instead of two dense nk x nk Phi GEMMs; under
    // time reversal (X_{-k} = conj(X_k), so x2_{-k} = conj(x2_k)) x2_k only for the
    // representatives k <= -k
    const bool half = c->time_reversal;
    const int nks = half ? kmesh_half_count(kmesh) : nk;
    void* base;
    if (wsb)
      FISDF_TRY(devbuf_get(*wsb, sizeof(cplx) * (size_t)nks * nn, &base));
    else
      FISDF_TRY(arena_get(c, sizeof(cplx) * (size_t)nks * nn, &base));
    cplx* X2k = (cplx*)base;
    std::vector<int> runs = {0, nk};
    if (half) FISDF_TRY(kmesh_rep_runs(kmesh, &runs));
    // x2_k = X_k^* X_k^T  (:38), one batched GEMM per run of stored k
    for (size_t r = 0, slot = 0; r < runs.size(); r += 2) {
      const int k0 = runs[r], nb = runs[r + 1] - runs[r];
      FISDF_TRY(zgemm(st, OP_R, OP_T, nip, nip, nao, ONE, X + (long)k0 * nip * nao, nao,
                      (long)nip * nao, X + (long)k0 * nip * nao, nao, (long)nip * nao, ZERO,
                      X2k + (long)slot * nn, nip, nn, nb));
      slot += nb;
    }
    // x2_s = Phi x2_k (:41, real: max|Im| monitored, :43), x4_s = x2_s^2 (:45),
    // x4_k = Phi^H x4_s (:46) for every k
    std::vector<int> all(nk);
    for (int q = 0; q < nk; ++q) all[q] = q;
    FISDF_TRY(kmesh_y(st, X2k, nn, kmesh, all.data(), nullptr, nk, nip, (cplx*)x4v, nn, nip,
                      0, half, c->maximag + 0, true));
    return 0;
  }
  FISDF_CHECK(st == c->stream, "build_x4: the dense path runs on the context stream only");
  Carver cv;
  size_t o1 = cv.take(sizeof(cplx) * nk * nn);
  size_t o2 = cv.take(sizeof(cplx) * nk * nn);
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  cplx* X2k = (cplx*)((char*)base + o1);
  cplx* X2s = (cplx*)((char*)base + o2);
  // x2_k = X_k^* X_k^T  (:38)
  FISDF_TRY(zgemm(st, OP_R, OP_T, nip, nip, nao, ONE, X, nao, (long)nip * nao, X, nao,
                  (long)nip * nao, ZERO, X2k, nip, nn, nk));
  // x2_s = Phi x2_k  (:41), must be real (:43), squared in the GEMM's epilogue:
  // x4_s = x2_s * x2_s (:45), recording max|Im x2_s|
  FISDF_TRY(zgemm(st, OP_N, OP_N, nk, nn, nk, ONE, phase, nk, 0, X2k, nn, 0, ZERO, X2s, nn,
                  0, 1, 1, nullptr, EPI_CSQUARE, c->maximag + 0));
  // x4_k = Phi^H x4_s (:46)
  FISDF_TRY(zgemm(st, OP_C, OP_N, nk, nn, nk, ONE, phase, nk, 0, X2s, nn, 0, ZERO,
                  (cplx*)x4v, nn, 0, 1));
  return 0;
}

// ---- A3 ---------------------------------------------------------------------
int fisdf_build_y_qs(fisdf_ctx* c, const void* fv, long f_kstride, int g0, int nblk, int ngrid,
                     const void* Xv, int nip, int nao, const int kmesh[3], const double a[9],
                     const int* h_qs, int nq, void* yTv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(g0 >= 0 && nblk >= 0 && g0 + nblk <= ngrid, "build_y: block out of range");
  // kmesh_y's own k-mesh checks come only after the fx GEMM has been enqueued
  FISDF_TRY(kmesh_check(kmesh, "build_y"));
  StageTimer tm(c, FISDF_ST_Y);
  const int nk = kmesh[0] * kmesh[1] * kmesh[2];
  FISDF_TRY(check_qlist(h_qs, nq, nk, "build_y"));
  FISDF_CHECK(nq > 0, "build_y: empty q-list");
  const cplx* f = (const cplx*)fv;
  const cplx* X = (const cplx*)Xv;
  cplx* yT = (cplx*)yTv;
  // grid sub-blocks of ~2 GB of FX temporary (swept on MI355X at C3 after the half-k /
  // short-K changes: y 28.1 / 22.7 / 20.9 / 18.4 / 16.7 ms for 128 MB / 256 MB / 512 MB /
  // 1 GB / 2 GB — cache-sized blocks lose more to the smaller GEMM/DFT launches than they
  // gain from Infinity-Cache residency; bigger blocks slow the side-stream factorisation)
  constexpr long yblk_bytes = 2048L << 20;
  // time reversal (fisdf_set_time_reversal): fx_k only for the representatives k <= -k, the
  // others are conj(fx_{-k}) inside kmesh_y — 36 of 64 k at 4x4x4
  const bool half = c->time_reversal;
  c->y_real_slot.assign(nq, 0);
#ifdef FISDF_EXP_NOY  // timing experiment only (wrong results)
  return 0;
#endif
  if (half && nblk > 0) {
    // fused fx + k-mesh DFT where the k-mesh allows it: no fx round trip through HBM
    bool done = false;
    const size_t yw = y_fused_workspace(kmesh, nip, nao, nblk);
    // self-conjugate q stored real (half their bytes) when the caller's fit reads them so:
    // the composite build on the whole grid (c->y_real_store)
    // (a 64-bit mask of q: the fused kernel runs only for nk <= 64, so larger meshes keep it 0)
    unsigned long long rmask = 0;
    if (c->y_real_store && g0 == 0 && nblk == ngrid && nk <= 64)
      for (int i = 0; i < nq; ++i) {
        const int q = h_qs[i];
        const int i2 = q % kmesh[2], i1 = (q / kmesh[2]) % kmesh[1], i0 = q / (kmesh[1] * kmesh[2]);
        if ((2 * i0) % kmesh[0] == 0 && (2 * i1) % kmesh[1] == 0 && (2 * i2) % kmesh[2] == 0)
          rmask |= 1ull << q;
      }
    if (yw) {
      void* wb = nullptr;
      FISDF_TRY(arena_get(c, yw, &wb));
      FISDF_TRY(y_fused(c->stream, X, nip, nao, f, f_kstride, nblk, kmesh, h_qs, nq, yT,
                        (long)nip * ngrid, ngrid, g0, c->maximag + 1, (cplx*)wb, yw, rmask, &done));
    }
    if (done) {
      for (int i = 0; i < nq; ++i) c->y_real_slot[i] = (rmask >> h_qs[i]) & 1ull ? 1 : 0;
      return 0;
    }
  }
  const int nks = half ? kmesh_half_count(kmesh) : nk;
  std::vector<int> runs = {0, nk};
  if (half) FISDF_TRY(kmesh_rep_runs(kmesh, &runs));
  const long per_g = (long)nks * nip * sizeof(cplx);
  int gb = (int)std::max(64L, std::min<long>(nblk, yblk_bytes / std::max(per_g, 1L)));
  gb = std::min(gb, std::max(nblk, 1));
  // pipelined: the fx GEMM of block i+1 (main stream) runs beside the k-mesh DFT of block i
  // (aux stream) on two fx buffers — the GEMM is write/compute bound, the DFT read/write bound,
  // and neither alone saturates HBM
  const int nbuf = gb < nblk ? 2 : 1;
  Carver cv;
  size_t o1[2];
  for (int i = 0; i < nbuf; ++i) o1[i] = cv.take((size_t)per_g * gb);
  size_t oq = cv.take(sizeof(int) * (size_t)nq);
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  int* dq = (int*)((char*)base + oq);
  FISDF_TRY(upload_ints(c, h_qs, nq, dq));
  hipStream_t sk = c->stream;
  if (nbuf == 2) {
    FISDF_TRY(ensure_aux(c));
    sk = c->aux[0];
    aux_fork(c, 0);
    FISDF_HIP(hipEventRecord(c->ev_fork, c->stream));
    FISDF_HIP(hipStreamWaitEvent(sk, c->ev_fork, 0));
  }
  const int fx_epi = EPI_STREAM;  // fx is read back by the DFT only a block later
  int blk = 0;
  for (int s0 = 0; s0 < nblk; s0 += gb, ++blk) {
    const int m = std::min(gb, nblk - s0);
    const long nm = (long)nip * m;
    const int bi = blk % nbuf;
    cplx* FX = (cplx*)((char*)base + o1[bi]);
    // buffer bi is free once the DFT of block blk-2 has read it
    if (nbuf == 2 && blk >= 2) FISDF_HIP(hipStreamWaitEvent(c->stream, c->ev_ybuf[2 + bi], 0));
    // fx_k^T = X_k f_k^H  -> FX[slot(k)][I][g]   (:76, transposed layout), one batched GEMM
    // per run of consecutive stored k
    for (size_t r = 0, slot = 0; r < runs.size(); r += 2) {
      const int k0 = runs[r], nb = runs[r + 1] - runs[r];
      FISDF_TRY(zgemm(c->stream, OP_N, OP_C, nip, m, nao, ONE, X + (long)k0 * nip * nao, nao,
                      (long)nip * nao, f + (long)k0 * f_kstride + (long)s0 * nao, nao, f_kstride,
                      ZERO, FX + (long)slot * nm, m, nm, nb, 1, nullptr, fx_epi));
      slot += nb;
    }
    if (nbuf == 2) {
      FISDF_HIP(hipEventRecord(c->ev_ybuf[bi], c->stream));
      FISDF_HIP(hipStreamWaitEvent(sk, c->ev_ybuf[bi], 0));
    }
    // fx_s = Phi fx_k (:79, real :81), y_s = fx_s^2 (:83), y_k = Phi^T y_s (:84) for the
    // listed q, written into yT[slot][I][g0+s0+g] (:85): separable k-mesh DFTs
    FISDF_TRY(kmesh_y(sk, FX, nm, kmesh, h_qs, dq, nq, m, yT, (long)nip * ngrid, ngrid,
                      (long)g0 + s0, half, c->maximag + 1));
    if (nbuf == 2) FISDF_HIP(hipEventRecord(c->ev_ybuf[2 + bi], sk));
  }
  if (nbuf == 2) FISDF_TRY(aux_join(c, 0));  // later work on the main stream (the fit, the
                                             // arena's next user) sees y
  return 0;
}

int fisdf_build_y(fisdf_ctx* c, const void* fv, long f_kstride, int g0, int nblk, int ngrid,
                  const void* Xv, int nip, int nao, const int kmesh[3], const double a[9],
                  int q0, int q1, void* yTv) {
  t_cur_ctx = c;
  FISDF_CHECK(kmesh && kmesh[0] >= 1 && kmesh[1] >= 1 && kmesh[2] >= 1, "build_y: bad k-mesh");
  const int nk = kmesh[0] * kmesh[1] * kmesh[2];
  FISDF_CHECK(0 <= q0 && q0 < q1 && q1 <= nk, "build_y: bad q range");
  std::vector<int> qs = q_range(q0, q1);
  return fisdf_build_y_qs(c, fv, f_kstride, g0, nblk, ngrid, Xv, nip, nao, kmesh, a, qs.data(),
                          (int)qs.size(), yTv);
}

// ---- A4 ---------------------------------------------------------------------
// rank copies, pivot-order factor (identity-padded to nip so the small back-substitutions of
// all q run as one batch), diagonal-block inverses and the merged TRSM operator, on stream s
// need_linv: the diagonal-block inverses of Lp (trsm_blocked, used only when some rank < nip;
// the unpivoted path is full-rank by construction — a failing slot is refactored, and this
// rerun, by factor_pivoted_slots)
int factor_finish(fisdf_ctx* c, hipStream_t s, const int* rank_dev_src, bool need_linv) {
  const int nk = c->f_nk, nip = c->f_nip, nb = c->f_nb, nblk = (nip + nb - 1) / nb;
  const long nn = (long)nip * nip;
  FISDF_HIP(hipMemcpyAsync(c->f_rank_pinned, rank_dev_src, sizeof(int) * nk, hipMemcpyDeviceToHost, s));
  FISDF_HIP(hipMemcpyAsync(c->f_rank_dev, rank_dev_src, sizeof(int) * nk, hipMemcpyDeviceToDevice, s));
  // ranks and pivots are known here: fisdf_factor_x4_wait returns on this event, and the fit
  // starts its FFTs while the operators below are still being built (it waits on ev_fac
  // per lane before its first TRSM)
  FISDF_HIP(hipEventRecord(c->ev_chol, s));
  // the operators of slots [z0, z0 + nz): every kernel below works per slot (strides from the
  // batch index; split-K from the block row's shape only), so a slot's operators do not depend on
  // which slots share the launch
  const long sLi = (long)nblk * nb * nb;
  auto operators = [&](int z0, int nz) -> int {
    if (nz <= 0) return 0;
    FISDF_TRY(gather_lp(s, c->f_L + z0 * nn, nip, nip, c->f_piv + (long)z0 * nip,
                        c->f_rank_dev + z0, nip, c->f_Lp + z0 * nn, nz));
    if (need_linv)
      FISDF_TRY(trinv_blocks(s, c->f_Lp + z0 * nn, nip, nip, nn, nb, sLi, c->f_Linv + z0 * sLi,
                             nz));
    FISDF_TRY(build_trsm_q(s, c->f_Lp + z0 * nn, nip, nn, c->f_Q + z0 * nn, nz, GEMM_FULL));
    // L^{-1} by the same block-row substitution applied to the identity (the fit then applies it
    // as one lower-triangular GEMM over the grid; J/K within 2-3x of the TRSM's rounding,
    // tests/experiments/explicit_tri_inverse.py)
    FISDF_TRY(set_identity(s, c->f_Li + z0 * nn, nip, nz));
    FISDF_TRY(trsm_merged_batched(s, c->f_Q + z0 * nn, nn, nip, c->f_Li + z0 * nn, nip, nn, nip,
                                   nz, true, c->f_ksw, c->f_ksw_elems));
    return 0;
  };
  // the first fitted slots' operators first (ev_fac_early): their lanes start the fit while the
  // rest are still being built.  FISDF_FAC_EARLY (slots, read per call; 0 off)
  const int early = [&] {
    const char* e = getenv("FISDF_FAC_EARLY");
    const int v = e ? atoi(e) : 2;
    return (v > 0 && v < nk) ? v : 0;
  }();
  c->f_early = early;
  if (early) {
    FISDF_TRY(operators(0, early));
    FISDF_HIP(hipEventRecord(c->ev_fac_early, s));
  }
  FISDF_TRY(operators(early, nk - early));
  return 0;
}

bool pivoted_fit_forced() {
  static const bool on = [] {
    const char* e = getenv("FISDF_PIVOTED_FIT");
    return e && e[0] == '1';
  }();
  return on;
}

// the greedy pivoted (rank-revealing) factorisation of the staged x4 (fallback / forced)
int factor_pivoted(fisdf_ctx* c, hipStream_t s) {
  const int nk = c->f_nk, nip = c->f_nip;
  const long nn = (long)nip * nip;
  char* b = (char*)c->f_scratch;
  Carver cv;
  size_t oR = cv.take(sizeof(int) * nk);
  size_t oD = cv.take(sizeof(double) * (size_t)nk * nip);
  size_t oF = cv.take(sizeof(int) * nk);
  size_t oW = cv.take(sizeof(double) * (size_t)nk * (1 + nip));
  void* trail = nullptr;
  FISDF_TRY(devbuf_get(c->ws_side_b, sizeof(cplx) * pchol_trail_elems(nip, nk), &trail));
  FISDF_TRY(pchol(s, c->f_x4s, nip, nn, nip, nk, nip, c->f_tol, 0.0, c->f_L, c->f_piv,
                  (int*)(b + oR), (double*)(b + oD), (int*)(b + oF), (double*)(b + oW),
                  (cplx*)trail));
  c->f_used_pivoted = true;
  return factor_finish(c, s, (const int*)(b + oR), true);
}

// the greedy pivoted factorisation of only the listed slots (those whose unpivoted Cholesky
// failed the full-rank test): gathered into a contiguous batch, factored, scattered back, so a
// q's factor does not depend on which other q share the batch (1-GPU and sharded builds agree)
int factor_pivoted_slots(fisdf_ctx* c, hipStream_t s, const std::vector<int>& slots) {
  const int nk = c->f_nk, nip = c->f_nip, nf = (int)slots.size();
  const long nn = (long)nip * nip;
  char* b = (char*)c->f_scratch;
  Carver cv;
  size_t oR = cv.take(sizeof(int) * nk);
  size_t oD = cv.take(sizeof(double) * (size_t)nk * nip);
  size_t oF = cv.take(sizeof(int) * nk);
  size_t oW = cv.take(sizeof(double) * (size_t)nk * (1 + nip));
  size_t oU = cv.take(sizeof(int) * nk);  // the unpivoted path's per-slot ranks
  void* wa = nullptr;
  FISDF_TRY(devbuf_get(c->ws_side_a, sizeof(cplx) * 2 * nf * nn + sizeof(int) * (size_t)nf * nip, &wa));
  cplx* A = (cplx*)wa;
  cplx* L = A + nf * nn;
  int* P = (int*)(L + nf * nn);
  void* trail = nullptr;
  FISDF_TRY(devbuf_get(c->ws_side_b, sizeof(cplx) * pchol_trail_elems(nip, nf), &trail));
  for (int j = 0; j < nf; ++j)
    FISDF_HIP(hipMemcpyAsync(A + j * nn, c->f_x4s + slots[j] * nn, sizeof(cplx) * nn,
                             hipMemcpyDeviceToDevice, s));
  FISDF_TRY(pchol(s, A, nip, nn, nip, nf, nip, c->f_tol, 0.0, L, P, (int*)(b + oR),
                  (double*)(b + oD), (int*)(b + oF), (double*)(b + oW), (cplx*)trail));
  for (int j = 0; j < nf; ++j) {
    const int i = slots[j];
    FISDF_HIP(hipMemcpyAsync(c->f_L + i * nn, L + j * nn, sizeof(cplx) * nn, hipMemcpyDeviceToDevice, s));
    FISDF_HIP(hipMemcpyAsync(c->f_piv + (long)i * nip, P + (long)j * nip, sizeof(int) * nip,
                             hipMemcpyDeviceToDevice, s));
    FISDF_HIP(hipMemcpyAsync((int*)(b + oU) + i, (int*)(b + oR) + j, sizeof(int),
                             hipMemcpyDeviceToDevice, s));
  }
  c->f_used_pivoted = true;
  return factor_finish(c, s, (const int*)(b + oU), true);
}

static int ensure_side(fisdf_ctx* c) {
  // 1-GPU build: the factor chain (small latency-bound kernels) on the device's LEAST priority,
  // the y build and the fit go first and the chain fills the gaps (at normal priority the factor
  // ends 2 ms sooner but the C3 step is 5 ms slower).  A k-shard's y build is 1/N as long, so
  // there the chain is the critical path to the first TRSM and runs at the GREATEST priority
  // (fisdf_set_factor_priority).  One side stream at a time: an extra stream changes
  // how HIP maps the context's streams onto the process's hardware queues (4 here), and two
  // fit lanes sharing a queue serialise (C3 +5 ms/step measured with a second side stream)
  // One padding stream (given one small memset so the runtime maps it onto a hardware queue)
  // before the side stream, in the place the cooperative launch's own queue takes when the
  // selection is launched cooperatively: without it, with the plain launch, the fit's two lanes
  // serialise (C3 90.3 vs 81.3 ms/step; profiles/r06/lanes/).  FISDF_PAD_QUEUES=n overrides.
  static const int pad_env = getenv("FISDF_PAD_QUEUES") ? atoi(getenv("FISDF_PAD_QUEUES"))
                                                        : (coop_launch_enabled() ? 0 : 1);
  if (pad_env > 0 && c->pad.empty()) {
    if (!c->pad_buf) FISDF_HIP(hipMalloc(&c->pad_buf, 256));
    for (int i = 0; i < pad_env && i < 8; ++i) {
      hipStream_t p = nullptr;
      FISDF_HIP(hipStreamCreateWithFlags(&p, hipStreamNonBlocking));
      FISDF_HIP(hipMemsetAsync(c->pad_buf, 0, 256, p));
      FISDF_HIP(hipStreamSynchronize(p));
      c->pad.push_back(p);
    }
  }
  if (c->side && c->side_hi != c->factor_hi) {
    FISDF_HIP(hipStreamSynchronize(c->side));
    FISDF_HIP(hipStreamDestroy(c->side));
    c->side = nullptr;
  }
  if (!c->side) {
    int least = 0, greatest = 0;
    FISDF_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    FISDF_HIP(hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking,
                                          c->factor_hi ? greatest : least));
    c->side_hi = c->factor_hi;
  }
  if (!c->ev_x4) {
    FISDF_HIP(hipEventCreateWithFlags(&c->ev_x4, hipEventDisableTiming));
    FISDF_HIP(hipEventCreateWithFlags(&c->ev_fac, hipEventDisableTiming));
    FISDF_HIP(hipEventCreateWithFlags(&c->ev_fac_early, hipEventDisableTiming));
    FISDF_HIP(hipEventCreateWithFlags(&c->ev_chol, hipEventDisableTiming));
  }
  return 0;
}

int fisdf_set_factor_priority(fisdf_ctx* c, int high) {
  FISDF_TRY(ctx_guard(c));
  FISDF_CHECK(c != nullptr && (high == 0 || high == 1), "set_factor_priority: 0 or 1");
  c->factor_hi = high;
  return 0;
}

int fisdf_factor_x4_mark(fisdf_ctx* c) {
  FISDF_TRY(device_guard(c));
  if (c->f_pending) FISDF_TRY(fisdf_factor_x4_wait(c, nullptr));
  FISDF_TRY(ensure_side(c));
  FISDF_HIP(hipEventRecord(c->ev_x4, c->stream));
  c->x4_marked = true;
  return 0;
}

int fisdf_factor_x4_async(fisdf_ctx* c, const void* x4all, const int* h_qs, int nq, int nip,
                          double tol_rel, const int* kmesh) {
  FISDF_TRY(device_guard(c));
  const int nk = nq;
  FISDF_CHECK(nk > 0 && nip > 0, "factor_x4: bad sizes");
  FISDF_TRY(check_qlist(h_qs, nq, 1 << 30, "factor_x4"));
  if (c->f_pending) FISDF_TRY(fisdf_factor_x4_wait(c, nullptr));
  if (!c->x4_marked) FISDF_TRY(ensure_side(c));
  const int nb = c->f_nb;
  const int nblk = (nip + nb - 1) / nb;
  const long nn = (long)nip * nip;
  // the factor buffers are kept between builds of the same shape (hipFree synchronises the
  // device and the ~1.2 GB re-allocation cost ~2 ms of idle GPU per C3 step)
  if (c->f_L && c->f_cap_nip == nip && c->f_cap_nk >= nk) {
    c->f_rank.clear();
    c->f_qs.clear();
    c->f_real.clear();
  } else {
  FISDF_TRY(free_factors(c));
  c->f_cap_nk = nk;
  c->f_cap_nip = nip;
  FISDF_HIP(hipMalloc(&c->f_x4s, sizeof(cplx) * nk * nn));
  FISDF_HIP(hipMalloc(&c->f_L, sizeof(cplx) * nk * nn));
  FISDF_HIP(hipMalloc(&c->f_Lp, sizeof(cplx) * nk * nn));
  FISDF_HIP(hipMalloc(&c->f_Linv, sizeof(cplx) * (size_t)nk * nblk * nb * nb));
  FISDF_HIP(hipMalloc(&c->f_Q, sizeof(cplx) * nk * nn));
  FISDF_HIP(hipMalloc(&c->f_Li, sizeof(cplx) * nk * nn));
  // split-K partials of the L^{-1} substitution: the whole batch in one launch per block row when
  // that fits 16M elements (256 MB), else trsm_merged_batched runs sub-batches (a matrix's split
  // depends on its shape only, so its arithmetic is unchanged)
  c->f_ksw_elems = std::max({1L, trsm_split_work_elems(nip, 1),
                             std::min(trsm_split_work_elems(nip, nk), 16L << 20)});
  FISDF_HIP(hipMalloc(&c->f_ksw, sizeof(cplx) * c->f_ksw_elems));
  FISDF_HIP(hipMalloc(&c->f_piv, sizeof(int) * (size_t)nk * nip));
  FISDF_HIP(hipMalloc(&c->f_rank_dev, sizeof(int) * nk));
  FISDF_HIP(hipHostMalloc((void**)&c->f_rank_pinned, sizeof(int) * nk, hipHostMallocDefault));
  FISDF_HIP(hipHostMalloc((void**)&c->f_fail_pinned, sizeof(int) * nk, hipHostMallocDefault));
  FISDF_HIP(hipHostMalloc((void**)&c->f_qr_pinned, sizeof(int) * 2 * nk, hipHostMallocDefault));
  FISDF_HIP(hipMalloc(&c->f_qr_dev, sizeof(int) * 2 * nk));
  }
  // scratch: pivoted pchol work, or the unpivoted path's rank/fail flags + block inverses
  Carver cv;
  cv.take(sizeof(int) * nk);
  cv.take(sizeof(double) * (size_t)nk * nip);
  cv.take(sizeof(int) * nk);
  cv.take(sizeof(double) * (size_t)nk * (1 + nip));
  size_t oU = cv.take(sizeof(int) * nk);                                   // unpivoted rank
  size_t oFl = cv.take(sizeof(int) * nk);                                  // unpivoted fail
  size_t oWk = cv.take(sizeof(cplx) * (size_t)nk * 4096 + sizeof(double) * nk);
  if (cv.off > c->f_scratch_size) {
    if (c->f_scratch) FISDF_HIP(hipFree(c->f_scratch));
    FISDF_HIP(hipMalloc(&c->f_scratch, cv.off));
    c->f_scratch_size = cv.off;
  }
  char* b = (char*)c->f_scratch;
  c->f_qs.assign(h_qs, h_qs + nq);
  c->f_real.assign(nq, 0);
  for (int i = 0; kmesh && i < nq; ++i) c->f_real[i] = self_conjugate(kmesh, h_qs[i]) ? 1 : 0;
  c->f_nk = nk;
  c->f_nip = nip;
  c->f_tol = tol_rel;
  c->f_used_pivoted = false;
  // the side stream starts once everything enqueued on `stream` so far (x4) is done; work
  // enqueued on `stream` after this call (the y build) runs concurrently
  // (or at fisdf_factor_x4_mark, so that work enqueued between the two calls — the y build —
  // is not waited for, and the factor's host-blocking rank read-back cannot delay its launch)
  if (!c->x4_marked) FISDF_HIP(hipEventRecord(c->ev_x4, c->stream));
  c->x4_marked = false;
  FISDF_HIP(hipStreamWaitEvent(c->side, c->ev_x4, 0));
  StageTimer tm(c, FISDF_ST_FACTOR, c->side);
  hipStream_t s = c->side;
  // stage the listed x4_q in one pass (self-conjugate q: x4_q = Phi[:,q]^H x4_s is real up to
  // rounding); the unpivoted path factors its copy in f_L in place.  The pinned q-list is
  // rewritten only here, after the previous factorisation was waited for (f_pending)
  const bool pivoted = c->force_pivoted == 1 || (c->force_pivoted < 0 && pivoted_fit_forced()) ||
                       c->fit_mode == FISDF_FIT_SVD;
  for (int i = 0; i < nq; ++i) {
    c->f_qr_pinned[i] = h_qs[i];
    c->f_qr_pinned[nq + i] = c->f_real[i];
  }
  FISDF_HIP(hipMemcpyAsync(c->f_qr_dev, c->f_qr_pinned, sizeof(int) * 2 * nq, hipMemcpyHostToDevice, s));
  FISDF_TRY(stage_x4(s, (const cplx*)x4all, c->f_qr_dev, nq, nn, c->f_x4s, pivoted ? nullptr : c->f_L));
  if (pivoted) {
    FISDF_TRY(factor_pivoted(c, s));
    c->f_check_fail = false;
  } else {
    // full-rank fast path: unpivoted blocked Cholesky (all pivots > tol_rel * max diag is the
    // same full-rank verdict the rank-revealing pivoted factorisation gives); any matrix that
    // fails it is redone by the pivoted pchol in fisdf_factor_x4_wait
    FISDF_TRY(chol_unpivoted(s, c->f_L, nip, nk, tol_rel, c->f_piv, (int*)(b + oU),
                             (int*)(b + oFl), (cplx*)(b + oWk)));
    FISDF_HIP(hipMemcpyAsync(c->f_fail_pinned, b + oFl, sizeof(int) * nk, hipMemcpyDeviceToHost, s));
    FISDF_TRY(factor_finish(c, s, (const int*)(b + oU), false));
    c->f_check_fail = true;
  }
  FISDF_HIP(hipEventRecord(c->ev_fac, s));
  c->f_pending = true;
  return 0;
}

int fisdf_set_pivoted_fit(fisdf_ctx* c, int mode) {
  FISDF_TRY(ctx_guard(c));
  FISDF_CHECK(c != nullptr && mode >= -1 && mode <= 1, "set_pivoted_fit: bad mode");
  c->force_pivoted = mode;
  return 0;
}

int fisdf_set_half_grid(fisdf_ctx* c, int mode) {
  FISDF_TRY(ctx_guard(c));
  FISDF_CHECK(c != nullptr && mode >= -1 && mode <= 1, "set_half_grid: mode must be -1, 0 or 1");
  c->half_grid = mode;
  return 0;
}

int fisdf_set_fit_mode(fisdf_ctx* c, int mode) {
  FISDF_TRY(ctx_guard(c));
  FISDF_CHECK(c != nullptr && mode >= FISDF_FIT_LSTSQ && mode <= FISDF_FIT_BASIC,
              "set_fit_mode: mode must be FISDF_FIT_LSTSQ, FISDF_FIT_SVD or FISDF_FIT_BASIC");
  c->fit_mode = mode;
  return 0;
}

int fisdf_min_norm_info(fisdf_ctx* c, int* h_nslots) {
  FISDF_TRY(ctx_guard(c));
  FISDF_CHECK(c != nullptr, "null context");
  int n = 0;
  for (char v : c->f_cod) n += v ? 1 : 0;
  if (h_nslots) *h_nslots = n;
  return 0;
}

int fisdf_set_omega(fisdf_ctx* c, double omega) {
  FISDF_TRY(ctx_guard(c));
  FISDF_CHECK(c != nullptr && std::isfinite(omega), "set_omega: omega must be finite");
  c->omega = omega;
  return 0;
}

int fisdf_set_time_reversal(fisdf_ctx* c, int on) {
  FISDF_TRY(ctx_guard(c));
  FISDF_CHECK(c != nullptr && (on == 0 || on == 1), "set_time_reversal: on must be 0 or 1");
  c->time_reversal = on == 1;
  return 0;
}

int fisdf_set_fit_lanes(fisdf_ctx* c, int lanes) {
  FISDF_TRY(ctx_guard(c));
  FISDF_CHECK(c != nullptr && lanes >= 0 && lanes <= 4, "set_fit_lanes: lanes must be 0..4");
  c->lanes = lanes;
  return 0;
}

int fisdf_set_fit_pipe(fisdf_ctx* c, int mode, int depth) {
  FISDF_TRY(ctx_guard(c));
  FISDF_CHECK(c != nullptr && mode >= -1 && mode <= 1 && depth >= 0 && depth <= 64,
              "set_fit_pipe: mode must be -1..1, depth 0..64");
  c->pipe_mode = mode;
  c->pipe_depth = depth;
  return 0;
}

}  // extern "C"

namespace {
// grow a vector of untimed events to n
int grow_events(std::vector<hipEvent_t>& v, int n) {
  while ((int)v.size() < n) {
    hipEvent_t e;
    FISDF_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    v.push_back(e);
  }
  return 0;
}

// y of the next fit's j-th q has landed once the work enqueued so far on `st` is done
int mark_y_ready_on(fisdf_ctx* c, int j, hipStream_t st) {
  FISDF_CHECK(j >= 0 && j < 4096, "mark_y_ready: bad index");
  FISDF_TRY(grow_events(c->ev_ready, j + 1));
  if ((int)c->ready_marked.size() <= j) c->ready_marked.resize(j + 1, 0);
  FISDF_HIP(hipEventRecord(c->ev_ready[j], st));
  c->ready_marked[j] = 1;
  return 0;
}

int set_y_slices_on(fisdf_ctx* c, int j, const void* recv, int nparts, const long* h_g0,
                    const long* h_ng, hipStream_t st) {
  FISDF_CHECK(recv != nullptr && nparts >= 1 && nparts <= 4096, "set_y_slices: bad piece");
  std::vector<long> sl;
  for (int p = 0; p < nparts; ++p) {
    FISDF_CHECK(h_g0[p] >= 0 && h_ng[p] >= 0, "set_y_slices: bad slice");
    sl.push_back(h_g0[p]);
    sl.push_back(h_ng[p]);
  }
  bool any = false;
  for (const cplx* pc : c->y_piece) any = any || pc != nullptr;
  FISDF_CHECK(!any || sl == c->y_slices, "set_y_slices: every piece of a call has one layout");
  c->y_slices = sl;
  if ((int)c->y_piece.size() <= j) c->y_piece.resize(j + 1, nullptr);
  c->y_piece[j] = (const cplx*)recv;
  return mark_y_ready_on(c, j, st);
}
}  // namespace

extern "C" {

int fisdf_mark_y_ready(fisdf_ctx* c, int j) {
  FISDF_TRY(device_guard(c));
  return mark_y_ready_on(c, j, c->stream);
}

int fisdf_set_y_slices(fisdf_ctx* c, int j, const void* recv, int nparts, const long* h_g0,
                       const long* h_ng) {
  FISDF_TRY(device_guard(c));
  return set_y_slices_on(c, j, recv, nparts, h_g0, h_ng, c->stream);
}

int fisdf_fit_info(fisdf_ctx* c, int* h_lanes, int* h_pipe_depth) {
  FISDF_TRY(ctx_guard(c));
  FISDF_CHECK(c != nullptr, "null context");
  if (h_lanes) *h_lanes = c->last_fit_lanes;
  if (h_pipe_depth) *h_pipe_depth = c->last_fit_pipe;
  return 0;
}

int fisdf_fit_report(fisdf_ctx* c, int j, int info[12]) {
  FISDF_TRY(ctx_guard(c));
  FISDF_CHECK(c != nullptr && info != nullptr, "fit_report: null argument");
  FISDF_CHECK(j >= 0 && j < (int)c->fit_report.size(), "fit_report: no such q in the last fit");
  for (int i = 0; i < 12; ++i) info[i] = c->fit_report[j].v[i];
  return 0;
}

int fisdf_fit_plan(const int kmesh[3], const int mesh[3], int q, int nq, int nip, int info[8]) {
  FISDF_CHECK(kmesh && mesh && info, "fit_plan: null argument");
  FISDF_CHECK(kmesh[0] >= 1 && kmesh[1] >= 1 && kmesh[2] >= 1 && mesh[0] >= 1 && mesh[1] >= 1 &&
                  mesh[2] >= 1 && q >= 0 && q < kmesh[0] * kmesh[1] * kmesh[2],
              "fit_plan: bad sizes");
  const bool self = self_conjugate(kmesh, q);
  int m[3] = {0, 0, 0};
  if (self) self_conjugate_m(kmesh, q, m);
  info[0] = self ? 1 : 0;
  for (int d = 0; d < 3; ++d) info[1 + d] = m[d];
  info[4] = self ? half_prefix_planes(mesh[0], m[0]) : mesh[0];
  info[5] = info[4] * mesh[1] * mesh[2];
  info[6] = lane_wpp_wanted(nq) ? 1 : 0;
  info[7] = wpp_ksplit(nip);
  return 0;
}

int fisdf_reserve_workspace(fisdf_ctx* c, size_t bytes) {
  FISDF_TRY(device_guard(c));
  void* base;
  return arena_get(c, bytes, &base);
}

int fisdf_factor_info(fisdf_ctx* c, int* h_used_pivoted) {
  FISDF_TRY(ctx_guard(c));
  FISDF_CHECK(c != nullptr, "null context");
  if (h_used_pivoted) *h_used_pivoted = c->f_used_pivoted ? 1 : 0;
  return 0;
}

// Minimum-norm operators (fisdf_set_fit_mode) of the slots that need one, on the side stream
// once the ranks are known: a rank-deficient x4_q (FISDF_FIT_LSTSQ) or every q (FISDF_FIT_SVD).
// gelsy (fftisdf.py:108) returns the minimum-norm least-squares solution; the basic solution
// of the rank-revealing factor differs from it in the null space (tests/experiments/
// min_norm_fit.py).  Synchronous: the Cholesky breakdown flags of each CholeskyQR pass are read.
static int build_min_norm(fisdf_ctx* c, bool* built) {
  *built = false;
  const int nk = c->f_nk, nip = c->f_nip;
  const long nn = (long)nip * nip;
  c->f_cod.assign(nk, 0);
  int ncod = 0;
  for (int q = 0; q < nk; ++q) {
    const int r = c->f_rank[q];
    const bool cod = r > 0 && (c->fit_mode == FISDF_FIT_SVD || (c->fit_mode == FISDF_FIT_LSTSQ && r < nip));
    c->f_cod[q] = cod ? 1 : 0;
    ncod += cod ? 1 : 0;
  }
  if (ncod == 0) return 0;
  if (!c->f_M) FISDF_HIP(hipMalloc(&c->f_M, sizeof(cplx) * (size_t)c->f_cap_nk * nn));
  if (!c->f_nip_dev) FISDF_HIP(hipMalloc(&c->f_nip_dev, sizeof(int)));
  FISDF_HIP(hipMemcpy(c->f_nip_dev, &nip, sizeof(int), hipMemcpyHostToDevice));
  hipStream_t s = c->side;
  const size_t wb = (min_norm_work_bytes(nip, nip) + 255) / 256 * 256;
  void* wv = nullptr;
  FISDF_TRY(devbuf_get(c->ws_side_b, wb + sizeof(int) * 3 * (size_t)nk, &wv));
  char* work = (char*)wv;
  int* fail = (int*)(work + wb);
  for (int q = 0; q < nk; ++q)
    if (c->f_cod[q])
      FISDF_TRY(min_norm_operator(s, c->f_L + q * nn, nip, nip, c->f_piv + (long)q * nip,
                                  c->f_rank[q], c->f_M + q * nn, nip, work, fail + 3 * q));
  std::vector<int> hf(3 * (size_t)nk, 0);
  FISDF_HIP(hipMemcpyAsync(hf.data(), fail, sizeof(int) * 3 * nk, hipMemcpyDeviceToHost, s));
  FISDF_HIP(hipEventRecord(c->ev_fac, s));
  FISDF_HIP(hipEventSynchronize(c->ev_fac));
  for (int q = 0; q < nk; ++q)
    FISDF_CHECK(!c->f_cod[q] || (hf[3 * q] == 0 && hf[3 * q + 1] == 0 && hf[3 * q + 2] == 0),
                "min-norm fit: CholeskyQR breakdown of the rank-revealing factor");
  *built = true;
  return 0;
}

int fisdf_factor_x4_wait(fisdf_ctx* c, int* h_ranks) {
  FISDF_TRY(device_guard(c));
  if (c->f_pending) {
    // ranks, pivots and the full-rank verdict are ready at ev_chol; the operators built
    // after it (L^-1 etc.) are waited for on the device (ev_fac, by the fit)
    FISDF_HIP(hipEventSynchronize(c->ev_chol));
    bool redone = false;
    if (c->f_check_fail) {
      std::vector<int> failed;
      for (int q = 0; q < c->f_nk; ++q)
        if (c->f_fail_pinned[q] != 0) failed.push_back(q);
      c->f_check_fail = false;
      if (!failed.empty()) {  // not numerically full rank at tol: rank-revealing factorisation
        FISDF_TRY(factor_pivoted_slots(c, c->side, failed));
        FISDF_HIP(hipEventRecord(c->ev_fac, c->side));
        FISDF_HIP(hipEventSynchronize(c->ev_fac));
        redone = true;
      }
    }
    c->f_rank.assign(c->f_rank_pinned, c->f_rank_pinned + c->f_nk);
    if (redone) FISDF_HIP(hipStreamWaitEvent(c->stream, c->ev_fac, 0));
    c->f_fac_unjoined = !redone;
    c->f_pending = false;
    bool built = false;
    FISDF_TRY(build_min_norm(c, &built));
    if (built) c->f_fac_unjoined = true;  // ev_fac re-recorded after the operators
  }
  if (h_ranks)
    for (int q = 0; q < c->f_nk; ++q) h_ranks[q] = c->f_rank[q];
  return 0;
}

// the main stream waits for every factor operator (the fit joins per lane instead)
static int join_factors(fisdf_ctx* c) {
  if (c->f_fac_unjoined) {
    FISDF_HIP(hipStreamWaitEvent(c->stream, c->ev_fac, 0));
    c->f_fac_unjoined = false;
  }
  return 0;
}

int fisdf_factor_x4_qs(fisdf_ctx* c, const void* x4all, const int* h_qs, int nq, int nip,
                       double tol_rel, const int* kmesh, int* h_ranks) {
  FISDF_TRY(fisdf_factor_x4_async(c, x4all, h_qs, nq, nip, tol_rel, kmesh));
  FISDF_TRY(fisdf_factor_x4_wait(c, h_ranks));
  return join_factors(c);
}

int fisdf_factor_x4(fisdf_ctx* c, const void* x4v, int q0, int q1, int nip, double tol_rel,
                    int* h_ranks) {
  FISDF_CHECK(q0 >= 0 && q1 > q0, "factor_x4: bad sizes");
  std::vector<int> qs = q_range(q0, q1);
  return fisdf_factor_x4_qs(c, x4v, qs.data(), (int)qs.size(), nip, tol_rel, nullptr, h_ranks);
}

// device table of where each plane i0 of a row lives inside an all-to-all piece (the concat over
// slices p of (rows, ng_p) blocks of grid points [g0_p, g0_p + ng_p)); cached per layout
static int plane_table(fisdf_ctx* c, const int mesh[3], int rows, const PlaneRef** out) {
  const long P = (long)mesh[1] * mesh[2], n0 = mesh[0];
  FISDF_CHECK(fft3d_reads_slices(mesh[0], mesh[1], mesh[2]),
              "fit_coulomb: sliced y needs a mesh the plane FFT kernels take");
  std::vector<long> key = c->y_slices;
  key.insert(key.end(), {(long)mesh[0], (long)mesh[1], (long)mesh[2], (long)rows});
  auto it = c->plane_cache.find(key);
  if (it == c->plane_cache.end()) {
    std::vector<PlaneRef> h(n0, PlaneRef{-1, 0});
    long off = 0;
    for (size_t p = 0; p + 1 < c->y_slices.size(); p += 2) {
      const long g0 = c->y_slices[p], ng = c->y_slices[p + 1];
      FISDF_CHECK(g0 % P == 0 && ng % P == 0 && g0 + ng <= n0 * P,
                  "fit_coulomb: y slices must be whole planes of the mesh");
      for (long i0 = g0 / P; i0 < (g0 + ng) / P; ++i0) h[i0] = PlaneRef{off + (i0 * P - g0), ng};
      off += (long)rows * ng;
    }
    for (long i0 = 0; i0 < n0; ++i0) FISDF_CHECK(h[i0].base >= 0, "fit_coulomb: y slices leave a plane out");
    PlaneRef* d = nullptr;
    FISDF_HIP(hipMalloc(&d, sizeof(PlaneRef) * n0));
    FISDF_HIP(hipMemcpy(d, h.data(), sizeof(PlaneRef) * n0, hipMemcpyHostToDevice));
    it = c->plane_cache.emplace(key, d).first;
  }
  *out = it->second;
  return 0;
}

}  // extern "C"

// ---- A4 + A5: the Coulomb fit's plan, fork, steps and driver -------
namespace {

// What one fisdf_fit_coulomb_qs call does, decided on the host before anything is enqueued: plain
// arithmetic on what the call already knows, no HIP call.  The driver and its steps read every
// decision from here, and fit_report_fill copies them into the record fisdf_fit_report returns.
struct FitPlan {
  struct Q {
    int rank = 0, ks = 1, lane = 0;
    int solve = -1;  // fisdf_fit_report's [6]: 0 L^-1 GEMM, 1 minimum norm, 2 blocked, -1 rank 0
    long ncol = 0;   // grid columns fitted (the prefix planes of a half-grid q)
    bool real = false, half = false, cod = false;
  };
  int nq = 0, NL = 1, D = 0;  // q, MFMA lanes, ring slots (0: the FFT runs in its lane)
  bool pipe = false, ready = false, any_piece = false, unpack = false;
  int rmax = 0, rfmax = 0, ncod = 0;  // largest rank, most rows transformed, minimum-norm slots
  int ks = 1, wks = 1;                // largest HERK split (workspace), split of the W_PP GEMMs
  bool all_full = false, lane_wpp = false;
  std::vector<Q> q;
};

// How many lanes and ring slots the call gets, and how its y is read.
// q are processed on NL "lanes" (the main stream and aux streams), each with its own workspaces,
// so one q's HBM-bound FFT and memory-stalled HERK overlap another q's MFMA-bound TRSM on the
// same CUs.
// Pipelined FFTs (default with >= 2 lanes; fisdf_set_fit_pipe / FISDF_FIT_PIPE=0 turn it off):
// the HBM-bound FFTs run on their own stream into a ring of D Yhat slots, ahead of the MFMA
// lanes, which wait per q on its event — the FFTs then overlap TRSM/HERK work instead of meeting
// another lane's FFT.  A slot is reused once the lane that read it records its `free` event, so
// the working set is D x nip x ngrid (D = lanes + 2 by default) whatever nq is.  With a single
// MFMA lane it is slower (C3 107.8 vs 100.9 ms/step), so one lane keeps the FFT in-lane.
// Sharded build (fisdf_mark_y_ready): y of the call's j-th q lands at ev_ready[j] on the main
// stream (all-to-all piece + unpack); the lanes then run on the aux streams only and each q
// starts as soon as its own piece is there, one call for the whole shard.
// lanes, depth: as set (depth 0: default_pipe_depth); pipe_mode 0: off
void fit_plan_lanes(FitPlan& p, int nq, const int mesh[3], int lanes, int pipe_mode, int depth,
                    bool ready, bool any_piece) {
  p.nq = nq;
  p.ready = ready;
  p.any_piece = any_piece;
  p.NL = std::min(nq, lanes);
  p.pipe = pipe_mode != 0 && nq > 1 && p.NL > 1;
  if (p.pipe) p.NL = std::min(p.NL, ready ? 2 : 3);  // aux[2] is the FFT stream
  if (ready) p.NL = std::min(p.NL, 3);               // every lane on an aux stream
  p.D = p.pipe ? std::min(nq, depth > 0 ? depth : default_pipe_depth(p.NL)) : 0;
  // all-to-all pieces of a mesh whose first FFT pass cannot read plane slices in place (no
  // register kernel, plane too large for the LDS plane kernel): each FFT-issuing stream (the FFT
  // stream, or every lane) unpacks its q's piece into a (nip, ngrid) buffer of its own first
  p.unpack = any_piece && !fft3d_reads_slices(mesh[0], mesh[1], mesh[2]);
}

// What follows from the ranks (known once the factorisation has been waited for): the slots
// [s0, s0 + nq) of the factored list, their ranks, real flags and minimum-norm flags.
void fit_plan_ranks(FitPlan& p, int nip, const int mesh[3], const int kmesh[3], const int* h_qs,
                    int s0, const std::vector<int>& f_rank, const std::vector<char>& f_real,
                    const std::vector<char>& f_cod, bool half_on, int ncu) {
  const long ngrid = (long)mesh[0] * mesh[1] * mesh[2];
  p.q.assign(p.nq, FitPlan::Q{});
  p.rmax = p.ncod = 0;
  p.ks = 1;
  p.all_full = true;
  for (int lq = 0; lq < p.nq; ++lq) {
    FitPlan::Q& pq = p.q[lq];
    const int sl = s0 + lq, r = f_rank[sl];
    pq.rank = r;
    pq.lane = lq % p.NL;
    pq.real = f_real[sl] != 0;
    // a self-conjugate q is fitted on the prefix planes of its Hermitian G pairs (about half the
    // grid): Re W = sum over one member of each pair with the pair's combined weight
    pq.half = half_on && pq.real;
    pq.ncol = ngrid;
    if (pq.half) {
      int m[3];
      self_conjugate_m(kmesh, h_qs[lq], m);
      pq.ncol = (long)half_prefix_planes(mesh[0], m[0]) * mesh[1] * mesh[2];
    }
    // minimum-norm slots transform all nip rows of y (the operator A^+ mixes every row)
    pq.cod = sl < (int)f_cod.size() && f_cod[sl] != 0;
    pq.solve = r == 0 ? -1 : pq.cod ? 1 : r == nip ? 0 : 2;
    // split-K of each q's HERK from its own rank (not the call's largest), so a q's arithmetic
    // does not depend on which other q share the call (1-GPU vs sharded builds agree bitwise);
    // the workspace holds the largest split over the whole grid
    pq.ks = pick_ksplit_herk(r, (int)pq.ncol, ncu);
    p.ks = std::max(p.ks, pick_ksplit_herk(r, (int)ngrid, ncu));
    p.rmax = std::max(p.rmax, r);
    p.ncod += pq.cod ? 1 : 0;
    p.all_full = p.all_full && r == nip;
  }
  p.rfmax = p.ncod ? nip : p.rmax;
  // every q full rank (the production regime) and many q in the call: each q's W_PP =
  // L^-H G L^-1 and its scatter run in its lane right after its HERK, overlapped with the other
  // q's fit, instead of as a batched tail after the lanes join (the same kernel per output, batch
  // 1: W_q unchanged bit for bit).  C3 on one GPU (36 q): 79.89 vs 80.21 ms/step; a k-shard's 4-5
  // q: +0.6 ms per rank (the last q of each lane then waits for its own small GEMMs), so below
  // kLaneWppMinQ q the batched tail stays.  FISDF_LANE_WPP: 0 never, 1 always
  p.lane_wpp = lane_wpp_wanted(p.nq) && p.all_full && p.ncod == 0;
  // W_PP = L^-H G L^-1 (two upper-triangular nip^3 GEMMs per q) split over K: 100 output tiles
  // of 64 x 64 at C3 leave most CUs idle for ~180 us per GEMM, in every lane, for every q.  The
  // split depends on nip only, the same in the lanes and in the batched tail (W_q bitwise equal
  // between the 1-GPU and the k-sharded builds).  FISDF_WPP_KSPLIT (read per call; 1 = off)
  p.wks = wpp_ksplit(nip);
}

// the arena of one call, carved in this order
struct FitLayout {
  size_t oY[4] = {0, 0, 0, 0}, oU[4] = {0, 0, 0, 0}, oK[4] = {0, 0, 0, 0}, oTc[4] = {0, 0, 0, 0};
  size_t oP[4] = {0, 0, 0, 0};                            // unpack buffers (FFT stream 0, lane l -> l)
  size_t oWk = 0, oG = 0, oT = 0, oS = 0, oMS = 0, oMT = 0, total = 0;
};

FitLayout fit_layout(const FitPlan& p, int nip, long ngrid) {
  const long rr = (long)p.rmax * p.rmax, nn = (long)nip * nip;
  FitLayout o;
  Carver cv;
  for (int l = 0; l < p.NL; ++l) {
    if (!p.pipe) o.oY[l] = cv.take(sizeof(cplx) * p.rfmax * ngrid);
    o.oU[l] = cv.take(sizeof(cplx) * p.rmax * ngrid);
    o.oK[l] = cv.take(sizeof(cplx) * (size_t)p.ks * p.rmax * p.rmax);
    o.oTc[l] = cv.take(sizeof(cplx) * rr);
  }
  if (p.unpack)
    for (int l = 0; l < (p.pipe ? 1 : p.NL); ++l) o.oP[l] = cv.take(sizeof(cplx) * (size_t)nip * ngrid);
  if (p.wks > 1) o.oWk = cv.take(sizeof(cplx) * (size_t)p.NL * p.wks * rr);
  o.oG = cv.take(sizeof(cplx) * p.nq * rr);  // (nq, rmax, rmax): G_q in the leading r_q x r_q block
  o.oT = cv.take(sizeof(cplx) * p.nq * rr);
  o.oS = cv.take(sizeof(cplx) * p.nq * rr);
  if (p.ncod) {
    o.oMS = cv.take(sizeof(cplx) * (size_t)p.ncod * p.rmax * nip);  // G M per min-norm slot
    o.oMT = cv.take(sizeof(cplx) * nn);                              // M^H G M
  }
  o.total = cv.off;
  return o;
}

const cplx* fit_piece(const fisdf_ctx* c, int lq) {
  return lq < (int)c->y_piece.size() ? c->y_piece[lq] : nullptr;
}

// the record fisdf_fit_report reads (what the plan decides; the FFT form [3] and the asymmetric
// count [5] are filled in where they are found)
void fit_report_fill(fisdf_ctx* c, const FitPlan& p) {
  c->fit_report.assign(p.nq, fisdf_ctx::FitRec{});
  for (int lq = 0; lq < p.nq; ++lq) {
    const FitPlan::Q& pq = p.q[lq];
    int* v = c->fit_report[lq].v;
    v[0] = pq.rank;
    v[1] = pq.real ? 1 : 0;
    v[2] = pq.half ? 1 : 0;
    v[4] = (int)pq.ncol;
    v[6] = pq.solve;
    v[7] = pq.cod ? 1 : 0;
    v[8] = pq.lane;
    v[9] = p.lane_wpp ? 1 : p.all_full ? 0 : 2;
    v[10] = (p.lane_wpp || p.all_full) ? p.wks : 1;
    v[11] = fit_piece(c, lq) ? (p.unpack ? 2 : 1) : 0;
  }
}

// The ring outside the arena (nip rows per slot, whatever the ranks turn out to be) and the events
// of the pipelined mode; without the memory for the ring, the in-lane FFT.
int fit_ring(fisdf_ctx* c, FitPlan& p, int nip, long ngrid) {
  if (!p.pipe) return 0;
  const size_t rb = sizeof(cplx) * (size_t)p.D * nip * ngrid;
  if (rb > c->f_ring_bytes) {
    if (c->f_ring) FISDF_HIP(hipFree(c->f_ring));
    c->f_ring = nullptr;
    c->f_ring_bytes = 0;
    if (hipMalloc(&c->f_ring, rb) == hipSuccess) {
      c->f_ring_bytes = rb;
    } else {
      // only pipe and D are cleared: NL keeps the cap (2 ready, else 3) it got while pipe was
      // still true, so such a call runs fewer lanes than one that asked for no pipe
      (void)hipGetLastError();
      c->f_ring = nullptr;
      p.pipe = false;
      p.D = 0;
      return 0;
    }
  }
  FISDF_TRY(grow_events(c->ev_q, p.nq));
  return grow_events(c->ev_free, p.D);
}

// one call's state, shared by its steps
struct FitCall {
  fisdf_ctx* c = nullptr;
  FitPlan p;
  FitLayout o;
  // the arguments
  const int* h_qs = nullptr;
  int nip = 0;
  const int *mesh = nullptr, *kmesh = nullptr;
  const double* a = nullptr;
  const cplx* yT = nullptr;
  cplx* Wq = nullptr;
  int s0 = 0, nb = 0;                 // first factor slot, block of the blocked substitution
  long ngrid = 0, nn = 0, rr = 0, sLi = 0;
  char* b = nullptr;                  // the arena
  cplx *G = nullptr, *T = nullptr, *S = nullptr;
  hipStream_t lane_st[4] = {nullptr, nullptr, nullptr, nullptr};
  hipStream_t fst = nullptr;          // the FFT stream of the pipelined mode
  bool aux_used[3] = {false, false, false};
  const PlaneRef* planes = nullptr;
  CellGeom g;
  double wscale = 0;  // sqrt(coulG(k_q+G) vol/N^2)  (:114-115 and the Parseval 1/N of :118)
};

// Which stream lane l runs on: aux[ready ? l : l - 1], lane 0 of a call that is not ready on the
// context's stream; the FFT stream of the pipelined mode is aux[2].  A ready call's lanes first
// wait for ev_ready[0]: everything enqueued before the first piece landed (the y build, the
// arena's previous users) is complete there.  G is zeroed on lane 0 and the other streams start
// behind that (ev_fork).  A one-lane, in-lane-FFT call that is not ready touches no aux stream.
int fit_fork(FitCall& f) {
  fisdf_ctx* c = f.c;
  const FitPlan& p = f.p;
  const bool forked = p.ready || p.NL > 1 || p.pipe;
  if (forked) FISDF_TRY(ensure_aux(c));
  f.lane_st[0] = c->stream;
  for (int l = p.ready ? 0 : 1; l < p.NL; ++l) {
    const int i = p.ready ? l : l - 1;
    f.lane_st[l] = c->aux[i];
    f.aux_used[i] = true;
    aux_fork(c, i);
    if (p.ready) FISDF_HIP(hipStreamWaitEvent(f.lane_st[l], c->ev_ready[0], 0));
  }
  FISDF_HIP(hipMemsetAsync(f.G, 0, sizeof(cplx) * p.nq * f.rr, f.lane_st[0]));
  if (!forked) return 0;
  FISDF_HIP(hipEventRecord(c->ev_fork, f.lane_st[0]));
  for (int l = 1; l < p.NL; ++l) FISDF_HIP(hipStreamWaitEvent(f.lane_st[l], c->ev_fork, 0));
  if (p.pipe) {
    f.fst = c->aux[2];
    f.aux_used[2] = true;
    aux_fork(c, 2);
    FISDF_HIP(hipStreamWaitEvent(f.fst, c->ev_fork, 0));
  }
  return 0;
}

// join the lanes (and the FFT stream: that keeps the arena reuse ordered) before the batched
// small stage on the main stream
// (this join is what makes fisdf_build's build_return(c, yT) right after this call safe: every
// FFT / lane read of y is ordered before the caller's stream-ordered free on c->stream)
int fit_join(FitCall& f) {
  for (int i = 0; i < 3; ++i)
    if (f.aux_used[i]) FISDF_TRY(aux_join(f.c, i));
  return join_factors(f.c);
}

// the weights of q lq, cached per q
int fit_weight(FitCall& f, hipStream_t st, int lq, const double** w) {
  return get_weight(f.c, st, f.mesh, f.kmesh, f.a, f.h_qs[lq], f.wscale, f.p.q[lq].half, w);
}

cplx* fit_slot(const FitCall& f, int lq) {
  return f.c->f_ring + (long)(lq % f.p.D) * f.nip * f.ngrid;
}

// Yhat_q = FFT(y_q[:, piv] * f_q) * w_q   (:99, :113-115, :118; rows in pivot order); the
// sharded build reads q in place from their all-to-all pieces (fisdf_set_y_slices) through a
// per-plane address table (plane-aligned slices)
// ub: the stream's unpack buffer (FFT stream 0, lane l -> l)
int fit_fft(FitCall& f, hipStream_t st, int lq, cplx* Yh, int ub) {
  fisdf_ctx* c = f.c;
  const FitPlan::Q& pq = f.p.q[lq];
  const int* mesh = f.mesh;
  const int nip = f.nip, sl = f.s0 + lq;
  const long ngrid = f.ngrid;
  const int r = pq.cod ? nip : pq.rank;
  double kq[3], kd[3];
  kpoint(f.kmesh, f.g, f.h_qs[lq], kq);
  for (int i = 0; i < 3; ++i) kd[i] = f.g.a[i][0] * kq[0] + f.g.a[i][1] * kq[1] + f.g.a[i][2] * kq[2];
  const double* wt = nullptr;
  FISDF_TRY(fit_weight(f, st, lq, &wt));
  // a half-grid q: its transform pairs G with -G - m (m = 2 k_q, the phase exp(-i k_q.r) times
  // a real input), so the FFT writes the prefix planes only and moves half of its intermediate
  // (fft3d herm); m from the phase actually applied must match the pairing the weights use
  int herm_m[3];
  bool herm = pq.half;
  if (herm) {
    int m[3];
    self_conjugate_m(f.kmesh, f.h_qs[lq], m);
    for (int d = 0; d < 3; ++d) {
      const double t = kd[d] / M_PI;
      const long tm2 = std::lround(t);
      herm = herm && std::fabs(t - (double)tm2) < 1e-9 &&
             ((tm2 % mesh[d]) + mesh[d]) % mesh[d] == m[d] % mesh[d];
      herm_m[d] = m[d];
    }
  }
  const int* hm = herm ? herm_m : nullptr;
  c->fit_report[lq].v[3] = fft3d_route(mesh[0], mesh[1], mesh[2], hm) == FFT_REG_HERM ? 1 : 0;
  // y of this q stored real by the composite build's y kernel (fisdf_build_y_qs)
  const bool y_real = f.yT != nullptr && lq < (int)c->y_real_slot.size() && c->y_real_slot[lq];
  StageTimer tm(c, FISDF_ST_FFT, st);
  const cplx* pc = fit_piece(c, lq);
  FISDF_CHECK(pc || f.yT, "fit_coulomb: q without y");
#ifdef FISDF_EXP_NOFFT  // timing experiment only (wrong results)
  return 0;
#endif
  if (pc && f.p.unpack) {  // piece -> (nip, ngrid) rows, stream-ordered before the FFT reads them
    cplx* yb = (cplx*)(f.b + f.o.oP[ub]);
    const char* src = (const char*)pc;
    for (size_t p = 0; p + 1 < c->y_slices.size(); p += 2) {
      const long g0 = c->y_slices[p], ng = c->y_slices[p + 1];
      FISDF_CHECK(g0 + ng <= ngrid, "fit_coulomb: y slice out of the mesh");
      if (ng == 0) continue;
      FISDF_HIP(hipMemcpy2DAsync(yb + g0, sizeof(cplx) * ngrid, src, sizeof(cplx) * ng,
                                 sizeof(cplx) * ng, nip, hipMemcpyDeviceToDevice, st));
      src += sizeof(cplx) * (size_t)ng * nip;
    }
    FISDF_TRY(fft3d(st, yb, ngrid, c->f_piv + (long)sl * nip, Yh, ngrid, r, mesh[0], mesh[1],
                    mesh[2], kd, wt, nullptr, nullptr, hm));
    return 0;
  }
  FISDF_CHECK(!(pc && y_real), "fit_coulomb: a real y slot with a y piece");
  FISDF_TRY(fft3d(st, pc ? pc : f.yT + (long)lq * nip * ngrid, ngrid, c->f_piv + (long)sl * nip, Yh,
                  ngrid, r, mesh[0], mesh[1], mesh[2], kd, wt, nullptr, pc ? f.planes : nullptr,
                  hm, y_real));
  return 0;
}

// FFT of q lq into its ring slot, after the lane that read the slot's previous q is done
int fit_enqueue_fft(FitCall& f, int lq) {
  fisdf_ctx* c = f.c;
  const FitPlan& p = f.p;
  if (lq >= p.nq || p.q[lq].rank == 0) return 0;
  if (lq >= p.D) FISDF_HIP(hipStreamWaitEvent(f.fst, c->ev_free[lq % p.D], 0));
  if (p.ready) FISDF_HIP(hipStreamWaitEvent(f.fst, c->ev_ready[lq], 0));
  FISDF_TRY(fit_fft(f, f.fst, lq, fit_slot(f, lq), 0));
  FISDF_HIP(hipEventRecord(c->ev_q[lq], f.fst));
  return 0;
}

// U = L^{-1} Yh   (fit, factored order; (x4_q)_PP = L L^H): one GEMM (timed kernel-exact) on a
// full-rank q and on a minimum-norm q; the basic solution of a rank-deficient q
// (FISDF_FIT_BASIC) substitutes block by block
int fit_solve(FitCall& f, int lq, cplx* Yh, cplx* U) {
  fisdf_ctx* c = f.c;
  const FitPlan::Q& pq = f.p.q[lq];
  hipStream_t st = f.lane_st[pq.lane];
  const int nip = f.nip, sl = f.s0 + lq, r = pq.rank, ncol = (int)pq.ncol;
  const long ngrid = f.ngrid, nn = f.nn;
  const bool real_q = pq.real;
  StageTimer tm(c, FISDF_ST_TRSM, st, pq.solve != 2);
  if (pq.solve == 1) {  // U = A^+ Yh[P]: the minimum-norm operator over all nip rows
    FISDF_TRY(zgemm(st, OP_N, OP_N, r, ncol, nip, ONE, c->f_M + (long)sl * nn, nip, 0, Yh, ngrid, 0,
                    ZERO, U, ngrid, 0, 1, 1, nullptr, EPI_NONE, nullptr,
                    real_q ? GEMM_A_REAL : GEMM_FULL));
  } else if (pq.solve == 0) {  // one lower-triangular GEMM with L^{-1}
#ifdef FISDF_EXP_NOREALTRSM  // timing experiment only (wrong results)
    if (real_q) return 0;
#endif
    FISDF_TRY(zgemm(st, OP_N, OP_N, nip, ncol, nip, ONE, c->f_Li + (long)sl * nn, nip, 0, Yh, ngrid,
                    0, ZERO, U, ngrid, 0, 1, 1, nullptr, EPI_NONE, nullptr,
                    GEMM_A_LOWER | (real_q ? GEMM_A_REAL : GEMM_FULL)));
  } else {
    FISDF_TRY(trsm_blocked(st, 1, c->f_Lp + (long)sl * nn, nip, 0, r, c->f_Linv + (long)sl * f.sLi,
                           0, f.nb, Yh, ngrid, 0, U, ngrid, 0, ncol, 1, real_q ? 1 : 0));
  }
  return 0;
}

// G = U U^H  (:121 by Parseval); of a real-factor q the HERK forms Re G only, and Im G comes from
// the weight-asymmetric G alone: every other (G, G') pair cancels.  scratch: r x ngrid (Yhat of
// this q, no longer needed)
int fit_gram(FitCall& f, int lq, const cplx* U, cplx* scratch) {
  fisdf_ctx* c = f.c;
  const FitPlan::Q& pq = f.p.q[lq];
  hipStream_t st = f.lane_st[pq.lane];
  const int r = pq.rank, ncol = (int)pq.ncol, rmax = f.p.rmax, q = f.h_qs[lq];
  const long ngrid = f.ngrid;
  cplx* kw = (cplx*)(f.b + f.o.oK[pq.lane]);
  cplx* Tc = (cplx*)(f.b + f.o.oTc[pq.lane]);
  cplx* Gq = f.G + lq * f.rr;
  {
    StageTimer tm(c, FISDF_ST_HERK, st, true);
    FISDF_TRY(herk(st, r, ncol, 1.0, U, ngrid, Gq, rmax, pq.ks, kw,
                   pq.real ? GEMM_RE_ONLY : GEMM_FULL));
  }
  if (!pq.real) return 0;
  StageTimer tm(c, FISDF_ST_SMALL, st);
  const fisdf_ctx::Asym* as = nullptr;
  if (pq.half) {
    // half grid: one member of each asymmetric pair, Im W = Im(U_A diag(f) U_A^H)
    FISDF_TRY(get_asym_half(c, st, f.mesh, f.kmesh, f.a, q, f.wscale, &as));
    c->fit_report[lq].v[5] = as->n;
    // scratch holds r x ngrid: the plain and the scaled copy of at most ngrid / 2 listed
    // columns at a time (one pass unless more than half the grid is listed, which takes a
    // mesh whose planes are all self-paired, n0 <= 2)
    const int cap = (int)std::max(1L, ngrid / 2);
    for (int o = 0; o < as->n; o += cap) {
      const int na = std::min(cap, as->n - o);
      cplx* plain = scratch;
      cplx* scaled = scratch + (long)r * na;
      FISDF_TRY(gather_cols_scaled(st, U, ngrid, r, as->idx + o, nullptr, na, plain));
      FISDF_TRY(gather_cols_scaled(st, U, ngrid, r, as->idx + o, as->f + o, na, scaled));
      FISDF_TRY(zgemm(st, OP_N, OP_C, r, r, na, ONE, scaled, na, 0, plain, na, 0, ZERO, Tc, rmax, 0,
                      1, std::min(pq.ks, std::max(1, na / 256)), kw));
      FISDF_TRY(add_imag(st, Gq, rmax, Tc, rmax, r));
    }
  } else {
    const double* wt = nullptr;
    FISDF_TRY(fit_weight(f, st, lq, &wt));
    FISDF_TRY(get_asym(c, st, f.mesh, f.kmesh, f.a, q, wt, &as));
    c->fit_report[lq].v[5] = as->n;
    if (as->n > 0) {
      FISDF_TRY(gather_cols(st, U, ngrid, r, as->idx, as->n, scratch));
      FISDF_TRY(herk(st, r, as->n, 1.0, scratch, as->n, Tc, rmax,
                     std::min(pq.ks, std::max(1, as->n / 256)), kw));
      FISDF_TRY(add_imag(st, Gq, rmax, Tc, rmax, r));
    }
  }
  return 0;
}

// W_PP = L^-H G L^-1 of this q in its lane (S = L^-H G, W_PP = L^-H S^H), scattered
int fit_wpp_lane(FitCall& f, int lq) {
  fisdf_ctx* c = f.c;
  const FitPlan& p = f.p;
  const int nip = f.nip, sl = f.s0 + lq, ln = p.q[lq].lane, rmax = p.rmax, wks = p.wks;
  const long rr = f.rr;
  hipStream_t st = f.lane_st[ln];
  StageTimer tm(c, FISDF_ST_SMALL, st);
  const cplx* Lf = c->f_Li + (long)sl * f.nn;
  cplx* wk = wks > 1 ? (cplx*)(f.b + f.o.oWk) + (long)ln * wks * rr : nullptr;
  FISDF_TRY(zgemm(st, OP_C, OP_N, nip, nip, nip, ONE, Lf, nip, 0, f.G + lq * rr, rmax, 0, ZERO,
                  f.S + lq * rr, rmax, 0, 1, wks, wk, EPI_NONE, nullptr, GEMM_A_UPPER));
  FISDF_TRY(zgemm(st, OP_C, OP_C, nip, nip, nip, ONE, Lf, nip, 0, f.S + lq * rr, rmax, 0, ZERO,
                  f.T + lq * rr, rmax, 0, 1, wks, wk, EPI_NONE, nullptr, GEMM_A_UPPER));
  FISDF_TRY(scatter_w(st, f.T + lq * rr, rmax, rr, rmax, c->f_piv + (long)sl * nip,
                      c->f_rank_dev + sl, f.Wq + lq * f.nn, nip, 1));
  return 0;
}

// What one q enqueues on its lane, in order: the wait for its Yhat (its ring slot's event, or its
// own ready mark and the FFT in the lane), the wait for its factor, the solve, the Gram, the
// ring slot handed back with the FFT D q ahead enqueued, and W_PP when it runs in the lane.
int fit_q(FitCall& f, int lq) {
  fisdf_ctx* c = f.c;
  const FitPlan& p = f.p;
  const FitPlan::Q& pq = p.q[lq];
  if (pq.rank == 0) return p.pipe ? fit_enqueue_fft(f, lq + p.D) : 0;
  const int sl = f.s0 + lq;  // factor slot
  hipStream_t st = f.lane_st[pq.lane];
  cplx* Yh = p.pipe ? fit_slot(f, lq) : (cplx*)(f.b + f.o.oY[pq.lane]);
  cplx* U = (cplx*)(f.b + f.o.oU[pq.lane]);  // where L^{-1} Yh lands
  if (p.pipe) {
    FISDF_HIP(hipStreamWaitEvent(st, c->ev_q[lq], 0));
  } else {
    if (p.ready) FISDF_HIP(hipStreamWaitEvent(st, c->ev_ready[lq], 0));
    FISDF_TRY(fit_fft(f, st, lq, Yh, pq.lane));
  }
  // L^-1, Q, ...: the slots built first need only their own (ev_fac_early); a lane's later q
  // wait for all of them
  if (c->f_fac_unjoined)
    FISDF_HIP(hipStreamWaitEvent(st, (sl < c->f_early && !pq.cod) ? c->ev_fac_early : c->ev_fac, 0));
  FISDF_TRY(fit_solve(f, lq, Yh, U));
  FISDF_TRY(fit_gram(f, lq, U, Yh));
  if (p.pipe) {  // this lane is done with the ring slot: the FFT D q ahead may overwrite it
    FISDF_HIP(hipEventRecord(c->ev_free[lq % p.D], st));
    FISDF_TRY(fit_enqueue_fft(f, lq + p.D));
  }
  if (p.lane_wpp) FISDF_TRY(fit_wpp_lane(f, lq));
  return 0;
}

// W_PP = L^{-H} G L^{-1} for all q of the shard at once on the main stream (L padded with
// identity, G with zeros beyond each rank):  T = L^{-H} G ; S = L^{-H} T^H ; W_PP = S^H ; scatter
// by pivots
int fit_tail(FitCall& f) {
  fisdf_ctx* c = f.c;
  const FitPlan& p = f.p;
  const int nip = f.nip, nq = p.nq, s0 = f.s0, rmax = p.rmax, NL = p.NL, wks = p.wks, nb = f.nb;
  const long nn = f.nn, rr = f.rr, sLi = f.sLi;
  cplx *G = f.G, *T = f.T, *S = f.S;
  StageTimer tm(c, FISDF_ST_SMALL);
  const cplx* Lp0 = c->f_Lp + (long)s0 * nn;
  const cplx* Li0 = c->f_Linv + (long)s0 * sLi;
  // minimum-norm slots: G M first (the batched back-substitutions below overwrite G)
  for (int lq = 0, j = 0; lq < nq && p.ncod; ++lq) {
    const int sl = s0 + lq, r = p.q[lq].rank;
    if (!p.q[lq].cod) continue;
    FISDF_TRY(zgemm(c->stream, OP_N, OP_N, r, nip, r, ONE, G + lq * rr, rmax, 0,
                    c->f_M + (long)sl * nn, nip, 0, ZERO, (cplx*)(f.b + f.o.oMS) + (long)j++ * rmax * nip,
                    nip, 0, 1));
  }
  if (p.all_full) {
    // with L^{-1} at hand, two batched GEMMs whose A = L^{-H} is upper triangular (each
    // M-tile starts its K loop at its own row: half the flops of dense GEMMs):
    //   S = L^{-H} G,  W_PP = L^{-H} S^H  (= L^{-H} G L^{-1}, G Hermitian)
    const cplx* Lf = c->f_Li + (long)s0 * nn;
    if (wks > 1) {
      // the lanes' split workspace, NL q at a time (per-q arithmetic as in the lanes)
      cplx* wk = (cplx*)(f.b + f.o.oWk);
      for (int z0 = 0; z0 < nq; z0 += NL) {
        const int nz = std::min(NL, nq - z0);
        FISDF_TRY(zgemm(c->stream, OP_C, OP_N, nip, nip, nip, ONE, Lf + (long)z0 * nn, nip, nn,
                        G + z0 * rr, rmax, rr, ZERO, S + z0 * rr, rmax, rr, nz, wks, wk, EPI_NONE,
                        nullptr, GEMM_A_UPPER));
        FISDF_TRY(zgemm(c->stream, OP_C, OP_C, nip, nip, nip, ONE, Lf + (long)z0 * nn, nip, nn,
                        S + z0 * rr, rmax, rr, ZERO, T + z0 * rr, rmax, rr, nz, wks, wk, EPI_NONE,
                        nullptr, GEMM_A_UPPER));
      }
    } else {
      FISDF_TRY(zgemm(c->stream, OP_C, OP_N, nip, nip, nip, ONE, Lf, nip, nn, G, rmax, rr, ZERO,
                      S, rmax, rr, nq, 1, nullptr, EPI_NONE, nullptr, GEMM_A_UPPER));
      FISDF_TRY(zgemm(c->stream, OP_C, OP_C, nip, nip, nip, ONE, Lf, nip, nn, S, rmax, rr, ZERO,
                      T, rmax, rr, nq, 1, nullptr, EPI_NONE, nullptr, GEMM_A_UPPER));
    }
  } else {
    FISDF_TRY(trsm_blocked(c->stream, 0, Lp0, nip, nn, rmax, Li0, sLi, nb, G, rmax, rr,
                           T, rmax, rr, rmax, nq));
    FISDF_TRY(conj_transpose(c->stream, T, rmax, rr, G, nq));
    FISDF_TRY(trsm_blocked(c->stream, 0, Lp0, nip, nn, rmax, Li0, sLi, nb, G, rmax, rr,
                           S, rmax, rr, rmax, nq));
    FISDF_TRY(conj_transpose(c->stream, S, rmax, rr, T, nq));
  }
  FISDF_TRY(scatter_w(c->stream, T, rmax, rr, rmax, c->f_piv + (long)s0 * nip,
                      c->f_rank_dev + s0, f.Wq, nip, nq));
  // minimum-norm slots: W_PP = M^H (G M) (nip x nip: z[P] = M^H U) replaces the above
  for (int lq = 0, j = 0; lq < nq && p.ncod; ++lq) {
    const int sl = s0 + lq, r = p.q[lq].rank;
    if (!p.q[lq].cod) continue;
    const cplx* MS = (cplx*)(f.b + f.o.oMS) + (long)j++ * rmax * nip;
    cplx* MT = (cplx*)(f.b + f.o.oMT);
    const cplx* Mq = c->f_M + (long)sl * nn;
    FISDF_TRY(zgemm(c->stream, OP_C, OP_N, nip, nip, r, ONE, Mq, nip, 0, MS, nip, 0, ZERO, MT,
                    nip, 0, 1));
    FISDF_TRY(scatter_w(c->stream, MT, nip, 0, nip, c->f_piv + (long)sl * nip, c->f_nip_dev,
                        f.Wq + lq * nn, nip, 1));
  }
  return 0;
}

}  // namespace

extern "C" {

int fisdf_fit_coulomb_qs(fisdf_ctx* c, const int* h_qs, int nq, const void* yTv, int nip,
                         const int mesh[3], const int kmesh[3], const double a[9], void* Wqv) {
  FISDF_TRY(device_guard(c));
  // the marks belong to this call: cleared on every return, error returns included, so a failed
  // call cannot leave the next one running in 'ready' mode against stale events
  struct ClearMarks {
    fisdf_ctx* c;
    ~ClearMarks() {
      c->ready_marked.assign(c->ready_marked.size(), 0);
      c->y_piece.clear();
    }
  } clear_marks{c};
  const int nk = kmesh[0] * kmesh[1] * kmesh[2];
  FISDF_TRY(check_qlist(h_qs, nq, nk, "fit_coulomb"));
  // the listed q must be a contiguous run of the factored q-list (slots s0 .. s0+nq-1): the
  // whole shard at once, or one q at a time as its y arrives (overlapped all-to-all)
  FISDF_CHECK(c->f_nip == nip && nq >= 1, "fit_coulomb: call fisdf_factor_x4 first");
  const auto it0 = std::find(c->f_qs.begin(), c->f_qs.end(), h_qs[0]);
  FISDF_CHECK(it0 != c->f_qs.end() && (it0 - c->f_qs.begin()) + nq <= (long)c->f_qs.size() &&
                  std::equal(h_qs, h_qs + nq, it0),
              "fit_coulomb: the q-list must be a contiguous run of the factored q-list");
  FitCall f;
  FitPlan& p = f.p;
  f.c = c;
  f.h_qs = h_qs;
  f.nip = nip;
  f.mesh = mesh;
  f.kmesh = kmesh;
  f.a = a;
  f.yT = (const cplx*)yTv;
  f.Wq = (cplx*)Wqv;
  f.s0 = (int)(it0 - c->f_qs.begin());
  f.nb = c->f_nb;
  f.ngrid = (long)mesh[0] * mesh[1] * mesh[2];
  f.nn = (long)nip * nip;
  f.sLi = (long)((nip + f.nb - 1) / f.nb) * f.nb * f.nb;
  lattice(a, f.g);
  f.wscale = cell_volume(a) / ((double)f.ngrid * f.ngrid);
  int nready = 0;
  bool any_piece = false;
  for (int lq = 0; lq < nq; ++lq) {
    nready += (lq < (int)c->ready_marked.size() && c->ready_marked[lq]) ? 1 : 0;
    any_piece = any_piece || fit_piece(c, lq) != nullptr;
  }
  FISDF_CHECK(nready == 0 || nready == nq, "fit_coulomb: mark every q of the call ready, or none");
  fit_plan_lanes(p, nq, mesh, c->lanes > 0 ? c->lanes : env_fit_lanes(),
                 c->pipe_mode >= 0 ? c->pipe_mode : env_fit_pipe(), c->pipe_depth, nready > 0,
                 any_piece);
  FISDF_TRY(fit_ring(c, p, nip, f.ngrid));
  if (any_piece && !p.unpack) FISDF_TRY(plane_table(c, mesh, nip, &f.planes));
  FISDF_CHECK(f.yT != nullptr || any_piece, "fit_coulomb: no y");
  const bool half_on = (c->half_grid >= 0 ? c->half_grid : env_half_grid()) != 0;
  FISDF_TRY(fisdf_factor_x4_wait(c, nullptr));
  fit_plan_ranks(p, nip, mesh, kmesh, h_qs, f.s0, c->f_rank, c->f_real, c->f_cod, half_on,
                 num_cus(c->device));
  f.o = fit_layout(p, nip, f.ngrid);
  f.rr = (long)p.rmax * p.rmax;
  c->last_fit_lanes = p.NL;
  c->last_fit_pipe = p.D;
  fit_report_fill(c, p);
  void* base;
  FISDF_TRY(arena_get(c, f.o.total, &base));
  f.b = (char*)base;
  f.G = (cplx*)(f.b + f.o.oG);
  f.T = (cplx*)(f.b + f.o.oT);
  f.S = (cplx*)(f.b + f.o.oS);
  if (p.rmax == 0) {
    FISDF_TRY(join_factors(c));
    FISDF_HIP(hipMemsetAsync(f.Wq, 0, sizeof(cplx) * nq * f.nn, c->stream));
    return 0;
  }
  FISDF_TRY(fit_fork(f));
  if (p.pipe)
    for (int lq = 0; lq < p.D; ++lq) FISDF_TRY(fit_enqueue_fft(f, lq));
  for (int lq = 0; lq < nq; ++lq) FISDF_TRY(fit_q(f, lq));
  FISDF_TRY(fit_join(f));
  if (!p.lane_wpp) FISDF_TRY(fit_tail(f));
  return 0;
}

int fisdf_fit_coulomb(fisdf_ctx* c, int q0, int q1, const void* yTv, int nip, const int mesh[3],
                      const int kmesh[3], const double a[9], void* Wqv) {
  const int nk = kmesh[0] * kmesh[1] * kmesh[2];
  FISDF_CHECK(0 <= q0 && q0 <= q1 && q1 <= nk, "fit_coulomb: bad q range");
  std::vector<int> qs = q_range(q0, q1);
  return fisdf_fit_coulomb_qs(c, qs.data(), (int)qs.size(), yTv, nip, mesh, kmesh, a, Wqv);
}

// ---- A8 prep ------------------------------------------------------------------
int fisdf_build_ws_qs(fisdf_ctx* c, const void* Wqv, const int* h_qs, const double* h_wt, int nq,
                      int nip, const int kmesh[3], const double a[9], void* Wsv) {
  FISDF_TRY(device_guard(c));
  StageTimer tm(c, FISDF_ST_WS);
  const int nk = kmesh[0] * kmesh[1] * kmesh[2];
  FISDF_TRY(check_qlist(h_qs, nq, nk, "build_ws"));
  const long nn = (long)nip * nip;
  if (nq == 0) {
    FISDF_HIP(hipMemsetAsync(Wsv, 0, sizeof(double) * nk * nn, c->stream));
    return 0;
  }
  // Phi_sel[R, i] = wt_i Phi[R, q_i]  (host; nk x nq)
  CellGeom g;
  lattice(a, g);
  std::vector<cplx> ph((size_t)nk * nq);
  for (int R = 0; R < nk; ++R) {
    int r2 = R % kmesh[2], r1 = (R / kmesh[2]) % kmesh[1], r0 = R / (kmesh[1] * kmesh[2]);
    double T[3];
    for (int cc = 0; cc < 3; ++cc) T[cc] = r0 * g.a[0][cc] + r1 * g.a[1][cc] + r2 * g.a[2][cc];
    for (int i = 0; i < nq; ++i) {
      double k[3];
      kpoint(kmesh, g, h_qs[i], k);
      const double th = T[0] * k[0] + T[1] * k[1] + T[2] * k[2];
      const double w = (h_wt ? h_wt[i] : 1.0) / std::sqrt((double)nk);
      ph[(size_t)R * nq + i] = cmk(w * std::cos(th), w * std::sin(th));
    }
  }
  Carver cv;
  size_t oP = cv.take(sizeof(cplx) * ph.size());
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  cplx* dph = (cplx*)((char*)base + oP);
  FISDF_TRY(upload_bytes(c, ph.data(), sizeof(cplx) * ph.size(), dph));
  // ws = Phi W (:205), real part * sqrt(nk) (:207) in the GEMM's epilogue, stored real (the
  // reference keeps W_s = ws.real, a real array).  With time-reversal representatives the
  // partner -q contributes conj(Phi[R,q] W_q), so Re(.) of the pair is 2 Re(Phi[R,q] W_q): wt = 2.
  FISDF_TRY(zgemm(c->stream, OP_N, OP_N, nk, nn, nq, cmk(std::sqrt((double)nk), 0), dph, nq, 0,
                  (const cplx*)Wqv, nn, 0, ZERO, (cplx*)Wsv, nn, 0, 1, 1, nullptr, EPI_REAL,
                  nullptr));
  return 0;
}

// W_s row blocks [rows[b], rows[b+1]) of a q-list's partial sum, block b at Wsb + b * chunk
// doubles (chunk 0: one block): the phase table uploaded once, one GEMM per block
static int ws_row_blocks(fisdf_ctx* c, const void* Wqv, const int* h_qs, const double* h_wt, int nq,
                         int nip, const int kmesh[3], const double a[9], int nblk,
                         const int* rows, long chunk, void* Wsv) {
  StageTimer tm(c, FISDF_ST_WS);
  const int nk = kmesh[0] * kmesh[1] * kmesh[2];
  FISDF_TRY(check_qlist(h_qs, nq, nk, "build_ws_rows"));
  FISDF_CHECK(nblk >= 1, "build_ws_rows: no blocks");
  for (int b = 0; b < nblk; ++b)
    FISDF_CHECK(0 <= rows[b] && rows[b] <= rows[b + 1] && rows[b + 1] <= nip &&
                    (nblk == 1 || (long)nk * (rows[b + 1] - rows[b]) * nip <= chunk),
                "build_ws_rows: bad row range");
  const long nn = (long)nip * nip;
  double* Ws = (double*)Wsv;
  if (nq == 0) {
    for (int b = 0; b < nblk; ++b)
      FISDF_HIP(hipMemsetAsync(Ws + b * chunk, 0,
                               sizeof(double) * nk * (rows[b + 1] - rows[b]) * nip, c->stream));
    return 0;
  }
  CellGeom g;
  lattice(a, g);
  std::vector<cplx> ph((size_t)nk * nq);
  for (int R = 0; R < nk; ++R) {
    int r2 = R % kmesh[2], r1 = (R / kmesh[2]) % kmesh[1], r0 = R / (kmesh[1] * kmesh[2]);
    double T[3];
    for (int cc = 0; cc < 3; ++cc) T[cc] = r0 * g.a[0][cc] + r1 * g.a[1][cc] + r2 * g.a[2][cc];
    for (int i = 0; i < nq; ++i) {
      double k[3];
      kpoint(kmesh, g, h_qs[i], k);
      const double th = T[0] * k[0] + T[1] * k[1] + T[2] * k[2];
      const double w = (h_wt ? h_wt[i] : 1.0) / std::sqrt((double)nk);
      ph[(size_t)R * nq + i] = cmk(w * std::cos(th), w * std::sin(th));
    }
  }
  Carver cv;
  size_t oP = cv.take(sizeof(cplx) * ph.size());
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  cplx* dph = (cplx*)((char*)base + oP);
  FISDF_TRY(upload_bytes(c, ph.data(), sizeof(cplx) * ph.size(), dph));
  // W_s[R][i0:i1] = sqrt(nk) Re(sum_i Phi_sel[R,i] W_{q_i}[i0:i1]) (fftisdf.py:205-207): the same
  // GEMM as fisdf_build_ws_qs on the row block (B = W_q rows i0..i1, ld nip^2), written (nk, nb, nip)
  for (int b = 0; b < nblk; ++b) {
    const long nb = rows[b + 1] - rows[b];
    if (nb == 0) continue;
    FISDF_TRY(zgemm(c->stream, OP_N, OP_N, nk, (int)(nb * nip), nq, cmk(std::sqrt((double)nk), 0),
                    dph, nq, 0, (const cplx*)Wqv + (long)rows[b] * nip, nn, 0, ZERO,
                    (cplx*)(Ws + b * chunk), nb * nip, 0, 1, 1, nullptr, EPI_REAL, nullptr));
  }
  return 0;
}

int fisdf_build_ws_rows(fisdf_ctx* c, const void* Wqv, const int* h_qs, const double* h_wt, int nq,
                        int nip, const int kmesh[3], const double a[9], int i0, int i1,
                        void* Wsv) {
  FISDF_TRY(device_guard(c));
  const int rows[2] = {i0, i1};
  return ws_row_blocks(c, Wqv, h_qs, h_wt, nq, nip, kmesh, a, 1, rows, 0, Wsv);
}

int fisdf_build_ws_blocks(fisdf_ctx* c, const void* Wqv, const int* h_qs, const double* h_wt,
                          int nq, int nip, const int kmesh[3], const double a[9], int nblk,
                          const int* h_rows, long chunk, void* Wsbv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(h_rows != nullptr && chunk >= 0, "build_ws_blocks: bad arguments");
  return ws_row_blocks(c, Wqv, h_qs, h_wt, nq, nip, kmesh, a, nblk, h_rows, chunk, Wsbv);
}

int fisdf_build_ws(fisdf_ctx* c, const void* Wqv, int q0, int q1, int nip, const int kmesh[3],
                   const double a[9], void* Wsv) {
  const int nk = kmesh[0] * kmesh[1] * kmesh[2];
  FISDF_CHECK(0 <= q0 && q0 <= q1 && q1 <= nk, "build_ws: bad q range");
  std::vector<int> qs = q_range(q0, q1);
  return fisdf_build_ws_qs(c, Wqv, qs.data(), nullptr, (int)qs.size(), nip, kmesh, a, Wsv);
}

// ---- next-2: ISDF ERIs / ao2mo --------------------------------------------------
// eri[i*n2+j][k*n4+l] = sum_IJ W_q[I,J] conj(A1[I,i]) A2[I,j] conj(A3[J,k]) A4[J,l],
// A_s = X_{k_s} C_s (C_s = identity when d_C[s] is null -> AO integrals), q = k2 - k1
// (identity of fftdf-with-k-lstsq.py:221-232).
int fisdf_get_eri(fisdf_ctx* c, const void* Xv, int nip, int nao, const int kidx[4],
                  const void* Wqv, const void* const* Cv, const int nmo[4], void* outv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(Xv && Wqv && outv && kidx, "get_eri: null X, W, index list or output");
  FISDF_CHECK(nip >= 1 && nao >= 1, "get_eri: nip and nao must be at least 1");
  const cplx* X = (const cplx*)Xv;
  int n[4];
  for (int s = 0; s < 4; ++s) {
    FISDF_CHECK(kidx[s] >= 0, "get_eri: negative k index");
    FISDF_CHECK(!(Cv && Cv[s]) || (nmo && nmo[s] >= 1), "get_eri: C_s given with nmo[s] < 1");
    n[s] = Cv && Cv[s] ? nmo[s] : nao;
  }
  // the pair counts are GEMM dimensions (int), checked before the arena is asked for anything
  const long p12 = (long)n[0] * n[1], p34 = (long)n[2] * n[3];
  FISDF_CHECK(p12 <= INT_MAX && p34 <= INT_MAX, "get_eri: n1*n2 or n3*n4 beyond int range");
  Carver cv;
  size_t oA[4];
  for (int s = 0; s < 4; ++s) oA[s] = cv.take(sizeof(cplx) * (size_t)nip * n[s]);
  size_t oP12 = cv.take(sizeof(cplx) * nip * p12);
  size_t oP34 = cv.take(sizeof(cplx) * nip * p34);
  size_t oT = cv.take(sizeof(cplx) * nip * p34);
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  char* b = (char*)base;
  const cplx* A[4];
  for (int s = 0; s < 4; ++s) {
    const cplx* Xk = X + (long)kidx[s] * nip * nao;
    if (Cv && Cv[s]) {
      cplx* As = (cplx*)(b + oA[s]);
      FISDF_TRY(zgemm(c->stream, OP_N, OP_N, nip, n[s], nao, ONE, Xk, nao, 0,
                      (const cplx*)Cv[s], n[s], 0, ZERO, As, n[s], 0, 1));
      A[s] = As;
    } else {
      A[s] = Xk;
    }
  }
  cplx* P12 = (cplx*)(b + oP12);
  cplx* P34 = (cplx*)(b + oP34);
  cplx* T = (cplx*)(b + oT);
  FISDF_TRY(pair_product(c->stream, A[0], n[0], A[1], n[1], nip, P12));
  FISDF_TRY(pair_product(c->stream, A[2], n[2], A[3], n[3], nip, P34));
  FISDF_TRY(zgemm(c->stream, OP_N, OP_N, nip, (int)p34, nip, ONE, (const cplx*)Wqv, nip, 0, P34,
                  p34, 0, ZERO, T, p34, 0, 1));
  FISDF_TRY(zgemm(c->stream, OP_T, OP_N, (int)p12, (int)p34, nip, ONE, P12, p12, 0, T, p34, 0,
                  ZERO, (cplx*)outv, p34, 0, 1));
  return 0;
}

// ---- A7 -----------------------------------------------------------------------
int fisdf_get_j_rows(fisdf_ctx* c, const void* Xv, const void* W0, const void* dmsv, int nset,
                     int nk, int nip, int nao, int i0, int i1, void* vjv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(Xv && W0 && dmsv && vjv, "get_j: null X, W0, density matrices or output");
  FISDF_CHECK(nset >= 1 && nk >= 1 && nip >= 1 && nao >= 1, "get_j: a size below 1");
  FISDF_CHECK(0 <= i0 && i0 <= i1 && i1 <= nip, "get_j: bad row range");
  StageTimer tm(c, FISDF_ST_J);
  const cplx* X = (const cplx*)Xv;
  const cplx* dms = (const cplx*)dmsv;
  cplx* vj = (cplx*)vjv;
  const int nb = i1 - i0;
  const long xs = (long)nip * nao, ds = (long)nao * nao;
  if (nb == 0) {
    FISDF_HIP(hipMemsetAsync(vj, 0, sizeof(cplx) * nset * nk * ds, c->stream));
    return 0;
  }
  Carver cv;
  size_t oT = cv.take(sizeof(cplx) * nset * nk * xs);
  size_t oR = cv.take(sizeof(cplx) * nset * nip);
  size_t oV = cv.take(sizeof(cplx) * nset * nb);
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  cplx* T = (cplx*)((char*)base + oT);
  cplx* rho = (cplx*)((char*)base + oR);
  cplx* v = (cplx*)((char*)base + oV);
  // T = X_k D_k
  for (int x = 0; x < nset; ++x)
    FISDF_TRY(zgemm(c->stream, OP_N, OP_N, nip, nao, nao, ONE, X, nao, xs, dms + (long)x * nk * ds,
                    nao, ds, ZERO, T + (long)x * nk * xs, nao, xs, nk));
  // rho_I = sum_k X_k[I,m] D_k[m,n] X_k*[I,n] / nk  (:155-156), every I
  FISDF_TRY(rho_diag(c->stream, T, X, nset, nk, nip, nao, 1.0 / nk, rho));
  // v_I = (W0 rho)_I for the rows of the block  (:159)
  FISDF_TRY(zgemm(c->stream, OP_N, OP_N, nb, 1, nip, ONE, (const cplx*)W0 + (long)i0 * nip, nip, 0,
                  rho, 1, nip, ZERO, v, 1, nb, nset));
  // J_k (block part) = X_k[I]^H diag(v_I) X_k[I]  (:166)
  FISDF_TRY(scale_rows(c->stream, X, v, nset, nk, nip, i0, nb, nao, T));
  for (int x = 0; x < nset; ++x)
    FISDF_TRY(zgemm(c->stream, OP_C, OP_N, nao, nao, nb, ONE, X + (long)i0 * nao, nao, xs,
                    T + (long)x * nk * nb * nao, nao, (long)nb * nao, ZERO,
                    vj + (long)x * nk * ds, nao, ds, nk));
  return 0;
}

int fisdf_get_j_band_rows(fisdf_ctx* c, const void* Xv, const void* W0, const void* dmsv, int nset,
                          int nk, int nip, int nao, const void* Xbv, int nkb, int i0, int i1,
                          void* vjv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(Xv && W0 && dmsv && Xbv && vjv,
              "get_j_band: null X, W0, density matrices, band AOs or output");
  FISDF_CHECK(nset >= 1 && nk >= 1 && nip >= 1 && nao >= 1, "get_j_band: a size below 1");
  FISDF_CHECK(0 <= i0 && i0 <= i1 && i1 <= nip && nkb > 0, "get_j_band: bad sizes");
  StageTimer tm(c, FISDF_ST_J);
  const cplx* X = (const cplx*)Xv;
  const cplx* Xb = (const cplx*)Xbv;
  const cplx* dms = (const cplx*)dmsv;
  cplx* vj = (cplx*)vjv;
  const int nb = i1 - i0;
  const long xs = (long)nip * nao, ds = (long)nao * nao;
  if (nb == 0) {
    FISDF_HIP(hipMemsetAsync(vj, 0, sizeof(cplx) * nset * nkb * ds, c->stream));
    return 0;
  }
  Carver cv;
  size_t oT = cv.take(sizeof(cplx) * nset * (size_t)std::max(nk, nkb) * xs);
  size_t oR = cv.take(sizeof(cplx) * nset * nip);
  size_t oV = cv.take(sizeof(cplx) * nset * nb);
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  cplx* T = (cplx*)((char*)base + oT);
  cplx* rho = (cplx*)((char*)base + oR);
  cplx* v = (cplx*)((char*)base + oV);
  // rho_I from the k-mesh density matrices and v = W0 rho (fftisdf.py:155-159), as get_j
  for (int x = 0; x < nset; ++x)
    FISDF_TRY(zgemm(c->stream, OP_N, OP_N, nip, nao, nao, ONE, X, nao, xs, dms + (long)x * nk * ds,
                    nao, ds, ZERO, T + (long)x * nk * xs, nao, xs, nk));
  FISDF_TRY(rho_diag(c->stream, T, X, nset, nk, nip, nao, 1.0 / nk, rho));
  FISDF_TRY(zgemm(c->stream, OP_N, OP_N, nb, 1, nip, ONE, (const cplx*)W0 + (long)i0 * nip, nip, 0,
                  rho, 1, nip, ZERO, v, 1, nb, nset));
  // J_k' = Xb_k'[I]^H diag(v_I) Xb_k'[I] at the band k-points (fftisdf.py:166 with kpts_band)
  FISDF_TRY(scale_rows(c->stream, Xb, v, nset, nkb, nip, i0, nb, nao, T));
  for (int x = 0; x < nset; ++x)
    FISDF_TRY(zgemm(c->stream, OP_C, OP_N, nao, nao, nb, ONE, Xb + (long)i0 * nao, nao, xs,
                    T + (long)x * nkb * nb * nao, nao, (long)nb * nao, ZERO,
                    vj + (long)x * nkb * ds, nao, ds, nkb));
  return 0;
}

int fisdf_get_j(fisdf_ctx* c, const void* Xv, const void* W0, const void* dmsv, int nset, int nk,
                int nip, int nao, void* vjv) {
  return fisdf_get_j_rows(c, Xv, W0, dmsv, nset, nk, nip, nao, 0, nip, vjv);
}

// ---- exact FFT-grid J (PySCF fft_jk.get_j_kpts; the kernels are in jfft.hip) ------------------
}  // extern "C"

namespace {

// the host-side checks of a potential on `mesh` other than the FFT's own (fft3d makes those
// when it is reached; until then only scratch is written)
int potential_check(const int mesh[3], const double a[9], int nset, long* ngrid) {
  FISDF_CHECK(mesh && a, "coulomb_potential: null mesh or lattice");
  FISDF_CHECK(nset >= 1, "coulomb_potential: nset must be >= 1");
  FISDF_CHECK(mesh[0] >= 1 && mesh[1] >= 1 && mesh[2] >= 1, "coulomb_potential: bad mesh");
  FISDF_CHECK(cell_volume(a) > 0, "coulomb_potential: singular lattice");
  *ngrid = (long)mesh[0] * mesh[1] * mesh[2];
  FISDF_CHECK(*ngrid < (1L << 31), "coulomb_potential: mesh too large");
  return 0;
}

// v_s = ifft(coulG(k = 0, omega) fft(rho_s)) with the forward fft3d only: t = fft(rho) coulG / N
// (the weight of the transform's last pass), then v = conj(fft(conj(t))).  w (ngrid doubles) and
// t (nset * ngrid) are scratch.  final_conj = false leaves conj(v) in v (weighted_gram's conj_v
// takes it from there).  fft3d runs all its checks before its first launch, and nothing before it
// writes v: a refused mesh leaves v untouched.
int potential_enqueue(fisdf_ctx* c, const cplx* rho, int nset, const int mesh[3],
                      const double a[9], double omega, double* w, cplx* t, cplx* v,
                      bool final_conj) {
  const long ngrid = (long)mesh[0] * mesh[1] * mesh[2];
  CellGeom g;
  lattice(a, g);
  const double k0[3] = {0, 0, 0};
  FISDF_TRY(coulg_weight(c->stream, mesh, g, k0, 1.0 / ngrid, 0, w, omega));
  FISDF_TRY(fft3d(c->stream, rho, ngrid, nullptr, t, ngrid, nset, mesh[0], mesh[1], mesh[2],
                  nullptr, w, nullptr));
  FISDF_TRY(conj_inplace(c->stream, t, nset * ngrid));
  FISDF_TRY(fft3d(c->stream, t, ngrid, nullptr, v, ngrid, nset, mesh[0], mesh[1], mesh[2], nullptr,
                  nullptr, nullptr));
  if (final_conj) FISDF_TRY(conj_inplace(c->stream, v, nset * ngrid));
  return 0;
}

}  // namespace

extern "C" {

int fisdf_get_rho(fisdf_ctx* c, const void* fv, long f_kstride, int nk, int ngrid, int nao,
                  const void* dmsv, int nset, void* rhov) {
  FISDF_TRY(device_guard(c));
  StageTimer tm(c, FISDF_ST_J);
  return rho_grid(c->stream, (const cplx*)fv, f_kstride, nk, ngrid, nao, (const cplx*)dmsv, nset,
                  (cplx*)rhov);
}

int fisdf_get_rho_gga(fisdf_ctx* c, const void* f4v, long f_kstride, long f_cstride, int nk, int ng,
                      int nao, const void* dmsv, int nset, int hermi, void* rhov,
                      long rho_cstride) {
  FISDF_TRY(device_guard(c));
  StageTimer tm(c, FISDF_ST_J);
  return rho_grid_gga(c->stream, (const cplx*)f4v, f_kstride, f_cstride, nk, ng, nao,
                      (const cplx*)dmsv, nset, hermi, (cplx*)rhov, rho_cstride);
}

int fisdf_gga_gram(fisdf_ctx* c, const void* f4v, long f_kstride, long f_cstride, int nk, int ng,
                   int nao, const void* wv, long w_sstride, long w_cstride, int nset, double scale,
                   int accumulate, void* outv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(nk >= 1 && ng >= 1 && nao >= 1 && nset >= 1, "gga_gram: sizes must be >= 1");
  StageTimer tm(c, FISDF_ST_J);
  size_t na, nm, ns;
  gga_gram_work(nk, ng, nao, &na, &nm, &ns);
  Carver cv;
  const size_t oA = cv.take(sizeof(cplx) * na), oM = cv.take(sizeof(cplx) * nm),
               oS = cv.take(sizeof(cplx) * ns);
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  char* b = (char*)base;
  return gga_gram(c->stream, (const cplx*)f4v, f_kstride, f_cstride, nk, ng, nao,
                  (const double*)wv, w_sstride, w_cstride, nset, scale, accumulate, (cplx*)outv,
                  (cplx*)(b + oA), (cplx*)(b + oM), ns ? (cplx*)(b + oS) : nullptr);
}

int fisdf_xc_eval(fisdf_ctx* c, int family, double cx, double cc, double rho_cut, const void* rhov,
                  long rho_sstride, long rho_cstride, int ng, int nset, void* ev, long e_sstride,
                  void* wv, long w_sstride, long w_cstride) {
  FISDF_TRY(device_guard(c));
  StageTimer tm(c, FISDF_ST_J);
  return xc_eval(c->stream, family, cx, cc, rho_cut, (const cplx*)rhov, rho_sstride, rho_cstride,
                 ng, nset, (double*)ev, e_sstride, (double*)wv, w_sstride, w_cstride, nullptr);
}

}  // extern "C"

namespace {

// the arena of one fused block, carved in this order; bytes() <= per_point ng + fixed of
// fisdf_nr_rks_plan (each of the seven pieces is rounded up to 256 bytes)
struct NrRksArena {
  size_t oRho, oW, oE, oPart, oAow, oM, oSplit, bytes;
  size_t nsplit;
};

constexpr int kNrRksPieces = 7;

void nr_rks_arena(int nk, int ng, int nao, int nset, NrRksArena* a) {
  size_t na, nm, ns;
  gga_gram_work(nk, ng, nao, &na, &nm, &ns);
  Carver cv;
  a->oRho = cv.take(sizeof(cplx) * (size_t)nset * 4 * ng);
  a->oW = cv.take(sizeof(double) * (size_t)nset * 4 * ng);
  a->oE = cv.take(sizeof(double) * (size_t)nset * ng);
  a->oPart = cv.take(sizeof(double) * 2 * (size_t)nset * xc_blocks(ng));
  a->oAow = cv.take(sizeof(cplx) * na);
  a->oM = cv.take(sizeof(cplx) * nm);
  a->oSplit = cv.take(sizeof(cplx) * ns);
  a->nsplit = ns;
  a->bytes = cv.off;
}

}  // namespace

extern "C" {

int fisdf_nr_rks_plan(int nk, int ng, int nao, int nset, long* h_point_bytes, long* h_fixed_bytes) {
  t_cur_ctx = nullptr;
  FISDF_CHECK(nk >= 1 && ng >= 1 && nao >= 1 && nset >= 1, "nr_rks_plan: sizes must be >= 1");
  FISDF_CHECK((long)nao * nao * nk < (1L << 31), "nr_rks_plan: matrices too large");
  size_t na, nm, ns;
  gga_gram_work(nk, ng, nao, &na, &nm, &ns);
  // per point: rho 64 B, wv 32 B and e 8 B a set, and the gram's aow row of every k-point
  if (h_point_bytes) *h_point_bytes = 104L * nset + 16L * nk * nao;
  if (h_fixed_bytes)
    *h_fixed_bytes = (long)(sizeof(cplx) * (nm + ns)) + 16L * nset * xc_blocks(ng) +
                     256L * kNrRksPieces;
  return 0;
}

int fisdf_nr_rks_block(fisdf_ctx* c, int family, double cx, double cc, double rho_cut,
                       const void* f4v, long f_kstride, long f_cstride, int nk, int ng, int nao,
                       const void* dmsv, int nset, double scale, int accumulate, void* vxcv,
                       void* sumsv) {
  FISDF_TRY(device_guard(c));
  // every check of the three stages, before the first launch
  FISDF_CHECK(family == 1, "nr_rks_block: family must be FISDF_XC_GGA (the LDA step takes the "
                           "resident AOs: fisdf_get_rho, fisdf_xc_eval, fisdf_weighted_gram)");
  FISDF_CHECK(f4v && dmsv && vxcv && sumsv, "nr_rks_block: null pointer");
  FISDF_CHECK(nk >= 1 && ng >= 1 && nao >= 1 && nset >= 1, "nr_rks_block: sizes must be >= 1");
  FISDF_CHECK(f_cstride >= (long)ng * nao, "nr_rks_block: f_cstride below ng * nao");
  FISDF_CHECK(f_kstride >= (long)ng * nao, "nr_rks_block: f_kstride below ng * nao");
  FISDF_CHECK((long)nao * nao * nk < (1L << 31), "nr_rks_block: density matrices too large");
  FISDF_CHECK(((long)ng * nao * nk + 255) / 256 < (1L << 31), "nr_rks_block: block too large");
  FISDF_CHECK((long)nset * 4 * ng < (1L << 40), "nr_rks_block: block too large");
  FISDF_CHECK(std::isfinite(scale), "nr_rks_block: scale must be finite");
  FISDF_TRY(xc_check(family, cx, cc, rho_cut, ng, nset, 4L * ng, ng, ng, 4L * ng, ng, true, true));
  StageTimer tm(c, FISDF_ST_J);
  NrRksArena a;
  nr_rks_arena(nk, ng, nao, nset, &a);
  void* base;
  FISDF_TRY(arena_get(c, a.bytes, &base));
  char* b = (char*)base;
  cplx* rho = (cplx*)(b + a.oRho);
  double *w = (double*)(b + a.oW), *e = (double*)(b + a.oE), *part = (double*)(b + a.oPart);
  FISDF_TRY(rho_grid_gga(c->stream, (const cplx*)f4v, f_kstride, f_cstride, nk, ng, nao,
                         (const cplx*)dmsv, nset, 1, rho, ng));
  FISDF_TRY(xc_eval(c->stream, family, cx, cc, rho_cut, rho, 4L * ng, ng, ng, nset, e, ng, w,
                    4L * ng, ng, part));
  FISDF_TRY(gga_gram(c->stream, (const cplx*)f4v, f_kstride, f_cstride, nk, ng, nao, w, 4L * ng,
                     ng, nset, scale, accumulate, (cplx*)vxcv, (cplx*)(b + a.oAow),
                     (cplx*)(b + a.oM), a.nsplit ? (cplx*)(b + a.oSplit) : nullptr));
  return xc_sums(c->stream, part, xc_blocks(ng), nset, scale, accumulate, (double*)sumsv);
}

int fisdf_coulomb_potential(fisdf_ctx* c, const void* rhov, int nset, const int mesh[3],
                            const double a[9], double omega, void* vv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(rhov && vv, "coulomb_potential: null pointer");
  long ngrid = 0;
  FISDF_TRY(potential_check(mesh, a, nset, &ngrid));
  StageTimer tm(c, FISDF_ST_J);
  Carver cv;
  size_t oW = cv.take(sizeof(double) * ngrid);
  size_t oT = cv.take(sizeof(cplx) * nset * ngrid);
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  return potential_enqueue(c, (const cplx*)rhov, nset, mesh, a, omega,
                           (double*)((char*)base + oW), (cplx*)((char*)base + oT), (cplx*)vv, true);
}

int fisdf_weighted_gram(fisdf_ctx* c, const void* fv, long f_kstride, int nk, int ngrid, int nao,
                        const void* vv, int nset, int conj_v, double scale, void* outv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(nk >= 1 && ngrid >= 1 && nao >= 1 && nset >= 1,
              "weighted_gram: sizes must be >= 1");
  StageTimer tm(c, FISDF_ST_J);
  const long we = weighted_gram_work_elems(nk, ngrid, nao, nset);
  void* base;
  FISDF_TRY(arena_get(c, sizeof(cplx) * we, &base));
  return weighted_gram(c->stream, (const cplx*)fv, f_kstride, nk, ngrid, nao, (const cplx*)vv,
                       nset, conj_v, scale, (cplx*)outv, (cplx*)base, we);
}

int fisdf_get_j_fft(fisdf_ctx* c, const void* fv, long f_kstride, const int kmesh[3],
                    const int mesh[3], const double a[9], int nao, const void* dmsv, int nset,
                    double omega, const void* fbandv, int nband, void* vjv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(fv && dmsv && vjv && kmesh, "get_j_fft: null pointer");
  FISDF_CHECK(kmesh[0] >= 1 && kmesh[1] >= 1 && kmesh[2] >= 1, "get_j_fft: bad k-mesh");
  FISDF_CHECK(nao >= 1, "get_j_fft: nao must be >= 1");
  FISDF_CHECK(fbandv == nullptr || nband >= 1, "get_j_fft: band AOs without band k-points");
  long ngl = 0;
  FISDF_TRY(potential_check(mesh, a, nset, &ngl));
  const long nkl = (long)kmesh[0] * kmesh[1] * kmesh[2];
  FISDF_CHECK(nkl <= 65535, "get_j_fft: more than 65535 k-points");
  FISDF_CHECK(f_kstride >= ngl * nao, "get_j_fft: f_kstride below ngrid * nao");
  const int nk = (int)nkl, ngrid = (int)ngl;
  // J at the k-mesh from f itself, or at the band k-points from their AOs on the same grid
  const cplx* fo = fbandv ? (const cplx*)fbandv : (const cplx*)fv;
  const long fo_ks = fbandv ? ngl * nao : f_kstride;
  const int no = fbandv ? nband : nk;
  StageTimer tm(c, FISDF_ST_J);
  const long we = weighted_gram_work_elems(no, ngrid, nao, nset);
  Carver cv;
  size_t oW = cv.take(sizeof(double) * ngl);
  size_t oR = cv.take(sizeof(cplx) * nset * ngl);
  size_t oT = cv.take(sizeof(cplx) * nset * ngl);
  size_t oV = cv.take(sizeof(cplx) * nset * ngl);
  size_t oP = cv.take(sizeof(cplx) * we);
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  double* w = (double*)((char*)base + oW);
  cplx* rho = (cplx*)((char*)base + oR);
  cplx* t = (cplx*)((char*)base + oT);
  cplx* v = (cplx*)((char*)base + oV);
  FISDF_TRY(rho_grid(c->stream, (const cplx*)fv, f_kstride, nk, ngrid, nao, (const cplx*)dmsv,
                     nset, rho));
  // conj(v) is left in v: the Gram reads it conjugated
  FISDF_TRY(potential_enqueue(c, rho, nset, mesh, a, omega, w, t, v, false));
  return weighted_gram(c->stream, fo, fo_ks, no, ngrid, nao, v, nset, 1,
                       cell_volume(a) / (double)ngl, (cplx*)vjv, (cplx*)((char*)base + oP), we);
}

// ---- exact FFT-grid K (PySCF fft_jk.get_k_kpts) in the dm form and the occupied-orbital form; the
// kernels and the plan are in kfft.hip ------------------------------------------------------------
static void kfft_plan_report(const KfftPlan& p, int* h_mc, int* h_nchunk, int* h_run_len,
                             int* h_nrun, int* h_pair_tw, int* h_exx_sc, int* h_exx_nn,
                             long* h_row_bytes, long* h_bytes) {
  if (h_mc) *h_mc = p.ok ? p.mc : 0;
  if (h_nchunk) *h_nchunk = p.ok ? p.nchunk : 0;
  if (h_run_len) *h_run_len = p.run_len;
  if (h_nrun) *h_nrun = p.nrun;
  if (h_pair_tw) *h_pair_tw = p.pair_tw;
  if (h_exx_sc) *h_exx_sc = p.exx_sc;
  if (h_exx_nn) *h_exx_nn = p.exx_nn;
  if (h_row_bytes) *h_row_bytes = p.row_bytes;
  if (h_bytes) *h_bytes = p.ok ? p.bytes : 0;
}

int fisdf_kfft_plan(int nao, long ngrid, int nset, long work_bytes, int* h_mc, int* h_nchunk,
                    int* h_run_len, int* h_nrun, int* h_pair_tw, int* h_exx_nn, long* h_row_bytes,
                    long* h_bytes) {
  t_cur_ctx = nullptr;
  FISDF_CHECK(nao >= 1 && nao <= kKfftMaxNao && ngrid >= 1 && ngrid < (1L << 31) && nset >= 1 &&
                  nset <= kKfftMaxSets && work_bytes >= 0,
              "kfft_plan: bad sizes");
  KfftPlan p;
  kfft_plan(nao, ngrid, nset, nao, false, work_bytes, &p);
  kfft_plan_report(p, h_mc, h_nchunk, h_run_len, h_nrun, h_pair_tw, nullptr, h_exx_nn, h_row_bytes,
                   h_bytes);
  return 0;
}

int fisdf_kfft_lr_plan(int nao, long ngrid, int nset, int imax, long work_bytes, int* h_mc,
                       int* h_nchunk, int* h_run_len, int* h_nrun, int* h_pair_tw, int* h_exx_sc,
                       int* h_exx_nn, long* h_row_bytes, long* h_bytes) {
  t_cur_ctx = nullptr;
  FISDF_CHECK(nao >= 1 && nao <= kKfftMaxNao && ngrid >= 1 && ngrid < (1L << 31) && nset >= 1 &&
                  nset <= kKfftMaxSets && imax >= 1 && imax <= kKfftMaxNao && work_bytes >= 0,
              "kfft_lr_plan: bad sizes");
  KfftPlan p;
  kfft_plan(nao, ngrid, nset, imax, true, work_bytes, &p);
  kfft_plan_report(p, h_mc, h_nchunk, h_run_len, h_nrun, h_pair_tw, h_exx_sc, h_exx_nn, h_row_bytes,
                   h_bytes);
  return 0;
}

int fisdf_pair_density(fisdf_ctx* c, const void* f1v, const void* f2v, int ngrid, int nao, int m0,
                       int m1, void* outv) {
  FISDF_TRY(device_guard(c));
  StageTimer tm(c, FISDF_ST_K);
  return pair_density(c->stream, (const cplx*)f1v, (const cplx*)f2v, ngrid, nao, m0, m1,
                      (cplx*)outv);
}

int fisdf_exx_contract(fisdf_ctx* c, const void* zv, const void* uv, const void* f1v,
                       const int mesh[3], const double* h_kd, int m0, int m1, int nao, int nset,
                       double scale, void* vkv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(mesh && mesh[0] >= 1 && mesh[1] >= 1 && mesh[2] >= 1, "exx_contract: bad mesh");
  const long ngl = (long)mesh[0] * mesh[1] * mesh[2];
  FISDF_CHECK(ngl < (1L << 31), "exx_contract: mesh too large");
  FISDF_CHECK(nao >= 1 && nset >= 1, "exx_contract: sizes must be >= 1");
  FISDF_CHECK(0 <= m0 && m0 < m1 && m1 <= nao, "exx_contract: bad row range");
  StageTimer tm(c, FISDF_ST_K);
  const long we = exx_contract_work_elems((int)ngl, nao, nset, m1 - m0, kJfftSetChunk);
  void* base;
  FISDF_TRY(arena_get(c, sizeof(cplx) * we, &base));
  return exx_contract(c->stream, (const cplx*)zv, (const cplx*)uv, (const cplx*)f1v, mesh, h_kd,
                      m0, m1, nao, nset, scale, 1, (cplx*)vkv, (long)nao * nao, (cplx*)base, we);
}

int fisdf_pair_density_lr(fisdf_ctx* c, const void* f1v, int nao, const void* psiv, int ni,
                          long ld_psi, int ngrid, int m0, int m1, void* outv) {
  FISDF_TRY(device_guard(c));
  StageTimer tm(c, FISDF_ST_K);
  return pair_density_lr(c->stream, (const cplx*)f1v, nao, (const cplx*)psiv, ni, ld_psi, ngrid,
                         m0, m1, (cplx*)outv);
}

int fisdf_exx_contract_lr(fisdf_ctx* c, const void* zv, const void* uv, const void* f1v,
                          const int mesh[3], const double* h_kd, int m0, int m1, int nao, int ni,
                          const int* h_seg, int nset, double scale, void* vkv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(mesh && mesh[0] >= 1 && mesh[1] >= 1 && mesh[2] >= 1, "exx_contract_lr: bad mesh");
  const long ngl = (long)mesh[0] * mesh[1] * mesh[2];
  FISDF_CHECK(ngl < (1L << 31), "exx_contract_lr: mesh too large");
  FISDF_CHECK(nao >= 1 && nset >= 1 && ni >= 1, "exx_contract_lr: sizes must be >= 1");
  FISDF_CHECK(0 <= m0 && m0 < m1 && m1 <= nao, "exx_contract_lr: bad row range");
  StageTimer tm(c, FISDF_ST_K);
  const long we = exx_contract_work_elems((int)ngl, nao, nset, m1 - m0, kLrSetChunk);
  void* base;
  FISDF_TRY(arena_get(c, sizeof(cplx) * we, &base));
  return exx_contract_lr(c->stream, (const cplx*)zv, (const cplx*)uv, (const cplx*)f1v, mesh, h_kd,
                         m0, m1, nao, ni, h_seg, nset, scale, 1, (cplx*)vkv, (long)nao * nao,
                         (cplx*)base, we);
}

// What the driver hands a form's steps: the sizes it has checked and the arena it has carved
struct KfftWork {
  int nk = 0, ngrid = 0;
  double scale = 0;  // of the contraction: cell volume / ngrid / nk
  long vk_set = 0;   // set stride of d_vk
  cplx *rows = nullptr, *psi = nullptr, *u = nullptr, *part = nullptr;
  long part_elems = 0;
};
// What a form of the exact K gives the driver; every step returns 0 or an error code
struct KfftForm {
  const char* name;   // the entry's name, the prefix of the driver's messages
  const char* row_m;  // what one row m holds, for the plan's refusal
  bool lowrank;       // kfft_plan's form
  // the entry's checks that need nk; *rows_max = the most rows per row m of any k2 (0: K = 0)
  std::function<int(int nk, int* rows_max)> sizes;
  // enqueues what the blocks of k2 share (w.u, w.psi); *rows = its rows per row m (0: no work)
  std::function<int(const KfftWork& w, int k2, const cplx* f2, int* rows)> prepare;
  // the pair densities of the rows [m0, m1) into w.rows, (m1 - m0) rows transform rows
  std::function<int(const KfftWork& w, const cplx* f1, int m0, int m1, int rows)> pair;
  // the transformed w.rows into the rows [m0, m1) of vk_k1
  std::function<int(const KfftWork& w, int rows, const cplx* f1, const double* kd, int m0, int m1,
                    int accumulate, cplx* vk_k1)> contract;
};

// fisdf_get_k_fft and fisdf_get_k_fft_lr behind their own argument checks: K[s][k1] = (1/nk) sum_k2
// of the blocks (k2, k1), each block in chunks of plan.mc rows m as pair densities, the transform
// pair between two conjugations, and the contraction.  The first k2 that has work overwrites d_vk,
// the later ones add; when no k2 has any, K = 0 is written and nothing else is read.
static int get_k_fft_run(fisdf_ctx* c, const KfftForm& form, const void* fv, long f_kstride,
                         const int kmesh[3], const int mesh[3], const double a[9], int nao,
                         int nset, double omega, const void* fbandv, const double* h_kband,
                         int nband, long work_bytes, void* vkv) {
  const std::string nm = std::string(form.name) + ": ";
  FISDF_CHECK(kmesh[0] >= 1 && kmesh[1] >= 1 && kmesh[2] >= 1, nm + "bad k-mesh");
  FISDF_CHECK(nao >= 1 && nao <= kKfftMaxNao, nm + "nao must be in [1, 32768]");
  FISDF_CHECK(nset <= kKfftMaxSets, nm + "more than 1024 sets");
  FISDF_CHECK(nband >= 0 && work_bytes >= 0 && std::isfinite(omega), nm + "bad arguments");
  FISDF_CHECK((fbandv != nullptr) == (nband > 0) && (fbandv == nullptr || h_kband != nullptr),
              nm + "band AOs, band k-points and nband go together");
  long ngl = 0;
  FISDF_TRY(potential_check(mesh, a, nset, &ngl));
  const long nkl = (long)kmesh[0] * kmesh[1] * kmesh[2];
  FISDF_CHECK(nkl <= 65535, nm + "more than 65535 k-points");
  FISDF_CHECK(f_kstride >= ngl * nao, nm + "f_kstride below ngrid * nao");
  const int nk = (int)nkl, ngrid = (int)ngl;
  int rows_max = 0;
  FISDF_TRY(form.sizes(nk, &rows_max));
  const cplx* f = (const cplx*)fv;
  cplx* vk = (cplx*)vkv;
  // K at the k-mesh from f itself, or at the band k-points from their AOs on the same grid
  const cplx* fo = fbandv ? (const cplx*)fbandv : f;
  const long fo_ks = fbandv ? ngl * nao : f_kstride;
  const int no = fbandv ? nband : nk;
  const long nn = (long)nao * nao;
  if (rows_max == 0) {  // nothing is transformed, the mesh is not read
    StageTimer tm(c, FISDF_ST_K);
    FISDF_HIP(hipMemsetAsync(vk, 0, sizeof(cplx) * (size_t)nset * no * nn, c->stream));
    return 0;
  }
  KfftPlan p;
  kfft_plan(nao, ngl, nset, rows_max, form.lowrank, work_bytes, &p);
  FISDF_CHECK(p.ok, nm + "work_bytes below one row of m (" + form.row_m + ")");
  // fft3d makes its own checks of the mesh when the first transform is reached: until then only
  // the arena is written, and d_vk is first written behind both transforms of the first block
  CellGeom g;
  lattice(a, g);
  StageTimer tm(c, FISDF_ST_K);
  void* base;
  FISDF_TRY(arena_get(c, (size_t)p.bytes, &base));
  KfftWork w;
  w.nk = nk;
  w.ngrid = ngrid;
  w.scale = cell_volume(a) / (double)ngl / (double)nk;
  w.vk_set = (long)no * nn;
  w.rows = (cplx*)((char*)base + p.off_rows);
  w.psi = (cplx*)((char*)base + p.off_psi);
  w.u = (cplx*)((char*)base + p.off_u);
  w.part = (cplx*)((char*)base + p.off_part);
  w.part_elems = p.part_elems;
  double* wt = (double*)((char*)base + p.off_w);
  bool first = true;  // no k2 has written d_vk yet
  for (int k2 = 0; k2 < nk; ++k2) {
    int rows = 0;
    FISDF_TRY(form.prepare(w, k2, f + (long)k2 * f_kstride, &rows));
    if (rows == 0) continue;
    double kq2[3];
    kpoint(kmesh, g, k2, kq2);
    for (int k1 = 0; k1 < no; ++k1) {
      const cplx* f1 = fo + (long)k1 * fo_ks;
      double kq1[3], q[3], kd[3];
      if (fbandv)
        for (int d = 0; d < 3; ++d) kq1[d] = h_kband[3 * k1 + d];
      else
        kpoint(kmesh, g, k1, kq1);
      for (int d = 0; d < 3; ++d) q[d] = kq2[d] - kq1[d];
      for (int d = 0; d < 3; ++d) kd[d] = g.a[d][0] * q[0] + g.a[d][1] * q[1] + g.a[d][2] * q[2];
      FISDF_TRY(coulg_weight(c->stream, mesh, g, q, 1.0 / (double)ngl, 0, wt, omega));
      for (int m0 = 0; m0 < nao; m0 += p.mc) {
        const int m1 = std::min(nao, m0 + p.mc);
        const int R = (m1 - m0) * rows;
        FISDF_TRY(form.pair(w, f1, m0, m1, rows));
        // vR conj(em)^-1 = ifft(coulG fft(pair em)) by the forward transform between conjugations;
        // the second conjugation and conj(em) are the contraction's
        FISDF_TRY(fft3d(c->stream, w.rows, ngl, nullptr, w.rows, ngl, R, mesh[0], mesh[1], mesh[2],
                        kd, wt, nullptr));
        FISDF_TRY(conj_inplace(c->stream, w.rows, (long)R * ngl));
        FISDF_TRY(fft3d(c->stream, w.rows, ngl, nullptr, w.rows, ngl, R, mesh[0], mesh[1], mesh[2],
                        nullptr, nullptr, nullptr));
        FISDF_TRY(form.contract(w, rows, f1, kd, m0, m1, first ? 0 : 1, vk + (long)k1 * nn));
      }
    }
    first = false;
  }
  return 0;
}

int fisdf_get_k_fft(fisdf_ctx* c, const void* fv, long f_kstride, const int kmesh[3],
                    const int mesh[3], const double a[9], int nao, const void* dmsv, int nset,
                    double omega, const void* fbandv, const double* h_kband, int nband,
                    long work_bytes, void* vkv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(fv && dmsv && vkv && kmesh, "get_k_fft: null pointer");
  const cplx* dms = (const cplx*)dmsv;
  const long nn = (long)nao * nao;
  const cplx* f2 = nullptr;  // of the k2 prepared last
  KfftForm form;
  form.name = "get_k_fft";
  form.row_m = "nao transform rows of the grid";
  form.lowrank = false;
  form.sizes = [&](int, int* rows_max) {
    *rows_max = nao;
    return 0;
  };
  // u_s = D[s][k2] f_k2^H, (nset, nao, ngrid): every k2 has work
  form.prepare = [&](const KfftWork& w, int k2, const cplx* fk2, int* rows) {
    f2 = fk2;
    *rows = nao;
    return zgemm(c->stream, OP_N, OP_C, nao, w.ngrid, nao, ONE, dms + (long)k2 * nn, nao,
                 (long)w.nk * nn, f2, nao, 0, ZERO, w.u, w.ngrid, (long)nao * w.ngrid, nset);
  };
  form.pair = [&](const KfftWork& w, const cplx* f1, int m0, int m1, int) {
    return pair_density(c->stream, f1, f2, w.ngrid, nao, m0, m1, w.rows);
  };
  form.contract = [&](const KfftWork& w, int, const cplx* f1, const double* kd, int m0, int m1,
                      int accumulate, cplx* vk_k1) {
    return exx_contract(c->stream, w.rows, w.u, f1, mesh, kd, m0, m1, nao, nset, w.scale,
                        accumulate, vk_k1, w.vk_set, w.part, w.part_elems);
  };
  return get_k_fft_run(c, form, fv, f_kstride, kmesh, mesh, a, nao, nset, omega, fbandv, h_kband,
                       nband, work_bytes, vkv);
}

int fisdf_get_k_fft_lr(fisdf_ctx* c, const void* fv, long f_kstride, const int kmesh[3],
                       const int mesh[3], const double a[9], int nao, const void* Av,
                       const void* Bv, const int* h_rank, int rmax, int nset, double omega,
                       const void* fbandv, const double* h_kband, int nband, long work_bytes,
                       void* vkv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(fv && Av && Bv && h_rank && vkv && kmesh, "get_k_fft_lr: null pointer");
  FISDF_CHECK(rmax >= 1 && rmax <= kKfftMaxNao, "get_k_fft_lr: rmax must be in [1, 32768]");
  const cplx* A = (const cplx*)Av;
  const cplx* B = (const cplx*)Bv;
  const long nr = (long)nao * rmax;
  std::vector<int> seg;  // of the k2 prepared last: set s owns the rows [seg[s], seg[s + 1])
  KfftForm form;
  form.name = "get_k_fft_lr";
  form.row_m = "the transform rows of the orbitals of the fullest k-point";
  form.lowrank = true;
  form.sizes = [&](int nk, int* rows_max) {
    long imax = 0;
    for (int k = 0; k < nk; ++k) {
      long ik = 0;
      for (int s = 0; s < nset; ++s) {
        const int r = h_rank[(long)s * nk + k];
        FISDF_CHECK(r >= 0 && r <= rmax, "get_k_fft_lr: rank outside [0, rmax]");
        ik += r;
      }
      imax = std::max(imax, ik);
    }
    FISDF_CHECK(imax <= kKfftMaxNao, "get_k_fft_lr: more than 32768 orbitals at one k-point");
    *rows_max = (int)imax;
    seg.resize(nset + 1);
    return 0;
  };
  // the orbitals of every set on the grid: psi[:, segment s] = f_k2 A[s][k2][:, :r_s], (ngrid,
  // ni), and u[segment s] = (B[s][k2][:, :r_s])^H f_k2^H = conj(psiB)^T, (ni, ngrid)
  form.prepare = [&](const KfftWork& w, int k2, const cplx* f2, int* rows) {
    seg[0] = 0;
    for (int s = 0; s < nset; ++s) seg[s + 1] = seg[s] + h_rank[(long)s * w.nk + k2];
    const int ni = *rows = seg[nset];
    for (int s = 0; s < nset; ++s) {
      const int r = seg[s + 1] - seg[s];
      if (r == 0) continue;
      const long sk = ((long)s * w.nk + k2) * nr;
      FISDF_TRY(zgemm(c->stream, OP_N, OP_N, w.ngrid, r, nao, ONE, f2, nao, 0, A + sk, rmax, 0,
                      ZERO, w.psi + seg[s], ni, 0, 1));
      FISDF_TRY(zgemm(c->stream, OP_C, OP_C, r, w.ngrid, nao, ONE, B + sk, rmax, 0, f2, nao, 0,
                      ZERO, w.u + (long)seg[s] * w.ngrid, w.ngrid, 0, 1));
    }
    return 0;
  };
  form.pair = [&](const KfftWork& w, const cplx* f1, int m0, int m1, int ni) {
    return pair_density_lr(c->stream, f1, nao, w.psi, ni, ni, w.ngrid, m0, m1, w.rows);
  };
  form.contract = [&](const KfftWork& w, int ni, const cplx* f1, const double* kd, int m0, int m1,
                      int accumulate, cplx* vk_k1) {
    return exx_contract_lr(c->stream, w.rows, w.u, f1, mesh, kd, m0, m1, nao, ni, seg.data(), nset,
                           w.scale, accumulate, vk_k1, w.vk_set, w.part, w.part_elems);
  };
  return get_k_fft_run(c, form, fv, f_kstride, kmesh, mesh, a, nao, nset, omega, fbandv, h_kband,
                       nband, work_bytes, vkv);
}

// ---- exact FFT-grid four-index integrals (PySCF FFTDF.get_eri / ao2mo); the B builder and the
// plan are in erifft.hip ---------------------------------------------------------------------------
int fisdf_eri_fft_plan(int n1, int n2, int n3, int n4, int npair, long ngrid, long work_bytes,
                       int* h_mc, int* h_nrow_chunks, int* h_bc, int* h_nb_chunks, int* h_b_once,
                       int* h_tw, int* h_ksplit, long* h_bytes) {
  t_cur_ctx = nullptr;
  FISDF_CHECK(n1 >= 1 && n2 >= 1 && n3 >= 1 && n4 >= 1 && n1 <= kKfftMaxNao &&
                  n2 <= kKfftMaxNao && n3 <= kKfftMaxNao && n4 <= kKfftMaxNao && npair >= 1 &&
                  npair <= kEriMaxPairs && ngrid >= 1 && ngrid < (1L << 31) && work_bytes >= 0,
              "eri_fft_plan: bad sizes");
  EriFftPlan p;
  eri_fft_plan(n1, n2, n3, n4, npair, ngrid, work_bytes, &p);
  if (h_mc) *h_mc = p.mc;
  if (h_nrow_chunks) *h_nrow_chunks = p.nrow_chunks;
  if (h_bc) *h_bc = p.bc;
  if (h_nb_chunks) *h_nb_chunks = p.nb_chunks;
  if (h_b_once) *h_b_once = p.b_once;
  if (h_tw) *h_tw = p.tw;
  if (h_ksplit) *h_ksplit = p.ksplit;
  if (h_bytes) *h_bytes = p.bytes;
  return 0;
}

int fisdf_pair34(fisdf_ctx* c, const void* const* a3v, const void* const* a4v, int npair, int n3,
                 int n4, long ld3, long ld4, const int mesh[3], const double* h_kd, int r0, int r1,
                 void* outv) {
  FISDF_TRY(device_guard(c));
  StageTimer tm(c, FISDF_ST_K);
  return pair34(c->stream, (const cplx* const*)a3v, (const cplx* const*)a4v, npair, n3, n4, ld3,
                ld4, mesh, h_kd, r0, r1, (cplx*)outv);
}

// eri[p] = (vol/ngrid) conj(Z) B_p^T in chunks of plan.mc rows i: the pair densities of (a1, a2),
// the transform pair between two conjugations as in get_k_fft_run, then one GEMM per (B chunk,
// pair) straight into d_out — conj(Z) is the GEMM's op, conj(em) is in B
int fisdf_get_eri_fft(fisdf_ctx* c, const int mesh[3], const double a[9], const double h_q[3],
                      double omega, const void* a1v, int n1, const void* a2v, int n2,
                      const void* const* a3v, const void* const* a4v, int npair, int n3, int n4,
                      long work_bytes, void* outv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(mesh && a && h_q && a1v && a2v && a3v && a4v && outv, "get_eri_fft: null pointer");
  FISDF_CHECK(n1 >= 1 && n2 >= 1 && n3 >= 1 && n4 >= 1 && npair >= 1,
              "get_eri_fft: sizes must be >= 1");
  FISDF_CHECK(n1 <= kKfftMaxNao && n2 <= kKfftMaxNao && n3 <= kKfftMaxNao && n4 <= kKfftMaxNao,
              "get_eri_fft: more than 32768 orbitals");
  FISDF_CHECK(npair <= kEriMaxPairs, "get_eri_fft: more than 65535 pairs");
  FISDF_CHECK(work_bytes >= 0 && std::isfinite(omega) && std::isfinite(h_q[0]) &&
                  std::isfinite(h_q[1]) && std::isfinite(h_q[2]),
              "get_eri_fft: bad arguments");
  const cplx* const* a3 = (const cplx* const*)a3v;
  const cplx* const* a4 = (const cplx* const*)a4v;
  for (int p = 0; p < npair; ++p) FISDF_CHECK(a3[p] && a4[p], "get_eri_fft: null pair pointer");
  long ngl = 0;
  FISDF_TRY(potential_check(mesh, a, 1, &ngl));
  EriFftPlan p;
  eri_fft_plan(n1, n2, n3, n4, npair, ngl, work_bytes, &p);
  FISDF_CHECK(p.ok, "get_eri_fft: work_bytes below one row (n2 transform rows or n4 rows of B)");
  // fft3d makes its own checks of the mesh when the first transform is reached: until then only
  // the arena is written, and d_out is first written behind both transforms of the first chunk
  CellGeom g;
  lattice(a, g);
  StageTimer tm(c, FISDF_ST_K);
  void* base;
  FISDF_TRY(arena_get(c, (size_t)p.bytes, &base));
  cplx* rows = (cplx*)((char*)base + p.off_rows);
  cplx* B = (cplx*)((char*)base + p.off_b);
  double* wt = (double*)((char*)base + p.off_w);
  cplx* work = p.ksplit > 1 ? (cplx*)((char*)base + p.off_work) : nullptr;
  const int ngrid = (int)ngl;
  double kd[3];
  for (int d = 0; d < 3; ++d) kd[d] = g.a[d][0] * h_q[0] + g.a[d][1] * h_q[1] + g.a[d][2] * h_q[2];
  // q = 0: em = 1, neither the transform nor B carries a phase
  const double* kdp = h_q[0] == 0 && h_q[1] == 0 && h_q[2] == 0 ? nullptr : kd;
  const long n34 = (long)n3 * n4, n12 = (long)n1 * n2;
  const int nrow34 = npair * n3;
  cplx* out = (cplx*)outv;
  const cplx alpha = cmk(cell_volume(a) / (double)ngl, 0);
  FISDF_TRY(coulg_weight(c->stream, mesh, g, h_q, 1.0 / (double)ngl, 0, wt, omega));
  if (p.b_once)
    FISDF_TRY(pair34(c->stream, a3, a4, npair, n3, n4, n3, n4, mesh, kdp, 0, nrow34, B));
  for (int i0 = 0; i0 < n1; i0 += p.mc) {
    const int i1 = std::min(n1, i0 + p.mc);
    const int R = (i1 - i0) * n2;
    FISDF_TRY(pair_density_lr(c->stream, (const cplx*)a1v, n1, (const cplx*)a2v, n2, n2, ngrid, i0,
                              i1, rows));
    FISDF_TRY(fft3d(c->stream, rows, ngl, nullptr, rows, ngl, R, mesh[0], mesh[1], mesh[2], kdp, wt,
                    nullptr));
    FISDF_TRY(conj_inplace(c->stream, rows, (long)R * ngl));
    FISDF_TRY(fft3d(c->stream, rows, ngl, nullptr, rows, ngl, R, mesh[0], mesh[1], mesh[2], nullptr,
                    nullptr, nullptr));
    for (int b0 = 0; b0 < nrow34; b0 += p.bc) {
      const int b1 = std::min(nrow34, b0 + p.bc);
      if (!p.b_once)
        FISDF_TRY(pair34(c->stream, a3, a4, npair, n3, n4, n3, n4, mesh, kdp, b0, b1, B));
      for (int pr = b0 / n3; pr <= (b1 - 1) / n3; ++pr) {
        const int ka = std::max(b0 - pr * n3, 0), kb = std::min(b1 - pr * n3, n3);
        FISDF_TRY(zgemm(c->stream, OP_R, OP_T, R, (kb - ka) * n4, ngrid, alpha, rows, ngl, 0,
                        B + (long)(pr * n3 + ka - b0) * n4 * ngl, ngl, 0, ZERO,
                        out + pr * n12 * n34 + (long)i0 * n2 * n34 + (long)ka * n4, n34, 0, 1,
                        p.ksplit, work));
      }
    }
  }
  return 0;
}

// ---- GTH pseudopotential and nuclear-attraction matrices (PySCF FFTDF.get_pp / get_nuc); the
// kernels and the plan are in pp.hip -----------------------------------------------------------------
int fisdf_pp_nproj(const fisdf_pp_atom* atoms, int natm) {
  if (pp_check_table(atoms, natm, "pp_nproj") != 0) return -1;
  const long rows = pp_rows(atoms, 0, natm);
  return rows < (1L << 31) ? (int)rows : -1;
}

int fisdf_pp_plan(int nao, long ngrid, int nk, int np, const fisdf_pp_atom* atoms, int natm,
                  int with_nonlocal, long work_bytes, int* h_run_len, int* h_nrun, int* h_mtiles,
                  int* h_ptiles, int* h_nchunk, int* h_chunk_rows, long* h_bytes) {
  FISDF_CHECK(atoms == nullptr || pp_check_table(atoms, natm, "pp_plan") == 0,
              "pp_plan: the atom table is refused");
  PpPlan p;
  pp_plan(nao, ngrid, nk, atoms, atoms ? natm : 0, with_nonlocal, work_bytes, &p);
  FISDF_CHECK(p.run_len > 0, "pp_plan: a size is out of range");
  if (h_run_len) *h_run_len = p.run_len;
  if (h_nrun) *h_nrun = p.nrun;
  if (h_mtiles) *h_mtiles = p.mtiles;
  if (h_ptiles) *h_ptiles = ((atoms ? p.nproj : np) + kPpPT - 1) / kPpPT;
  if (h_nchunk) *h_nchunk = p.ok ? p.nchunk : 0;
  if (h_chunk_rows) *h_chunk_rows = p.ok ? p.chunk_rows : 0;
  if (h_bytes) *h_bytes = p.ok ? p.bytes : 0;
  return 0;
}

int fisdf_vloc_g(fisdf_ctx* c, const int mesh[3], const double a[9], const fisdf_pp_atom* atoms,
                 int natm, void* vgv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(vgv, "vloc_g: null pointer");
  long ngl = 0;
  FISDF_TRY(potential_check(mesh, a, 1, &ngl));
  FISDF_TRY(pp_check_table(atoms, natm, "vloc_g"));
  CellGeom g;
  lattice(a, g);
  std::vector<double> tab;
  pp_vloc_table(atoms, natm, &tab);
  void* base;
  FISDF_TRY(arena_get(c, sizeof(double) * tab.size(), &base));
  FISDF_TRY(upload_bytes(c, tab.data(), sizeof(double) * tab.size(), base));
  return vloc_g(c->stream, mesh, g, (const double*)base, natm, 1.0, 0, (cplx*)vgv);
}

int fisdf_gth_projectors(fisdf_ctx* c, const int mesh[3], const double a[9], const double h_k[3],
                         const fisdf_pp_atom* atoms, int natm, int a0, int a1, void* rowsv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(rowsv && h_k, "gth_projectors: null pointer");
  FISDF_CHECK(std::isfinite(h_k[0]) && std::isfinite(h_k[1]) && std::isfinite(h_k[2]),
              "gth_projectors: bad k-point");
  long ngl = 0;
  FISDF_TRY(potential_check(mesh, a, 1, &ngl));
  FISDF_TRY(pp_check_table(atoms, natm, "gth_projectors"));
  FISDF_CHECK(0 <= a0 && a0 < a1 && a1 <= natm, "gth_projectors: bad atom range");
  std::vector<PpBlock> blk;
  pp_blocks(atoms, a0, a1, &blk);
  FISDF_CHECK(!blk.empty(), "gth_projectors: the atoms have no projectors");
  CellGeom g;
  lattice(a, g);
  void* base;
  FISDF_TRY(arena_get(c, sizeof(PpBlock) * blk.size(), &base));
  FISDF_TRY(upload_bytes(c, blk.data(), sizeof(PpBlock) * blk.size(), base));
  return gth_projectors(c->stream, mesh, g, h_k, (const PpBlock*)base, (int)blk.size(),
                        (cplx*)rowsv);
}

int fisdf_pp_overlap(fisdf_ctx* c, const void* tv, int np, const void* fv, int nao,
                     const int mesh[3], const double* h_kd, double scale, void* cv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(tv && fv && cv && mesh, "pp_overlap: null pointer");
  FISDF_CHECK(np >= 1 && nao >= 1 && nao <= kKfftMaxNao, "pp_overlap: sizes out of range");
  FISDF_CHECK(mesh[0] >= 1 && mesh[1] >= 1 && mesh[2] >= 1, "pp_overlap: bad mesh");
  const long ngl = (long)mesh[0] * mesh[1] * mesh[2];
  FISDF_CHECK(ngl < (1L << 31), "pp_overlap: mesh too large");
  int run_len = 0, nrun = 0;
  pp_overlap_split(ngl, &run_len, &nrun);
  void* base;
  FISDF_TRY(arena_get(c, sizeof(cplx) * (size_t)nrun * np * nao, &base));
  return pp_overlap(c->stream, (const cplx*)tv, np, (const cplx*)fv, nao, mesh, h_kd, scale,
                    (cplx*)cv, (cplx*)base);
}

int fisdf_get_pp(fisdf_ctx* c, const void* fv, long f_kstride, int nk, const double* h_kpts,
                 const int mesh[3], const double a[9], int nao, const fisdf_pp_atom* atoms,
                 int natm, int with_nonlocal, long work_bytes, void* outv) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(fv && h_kpts && outv, "get_pp: null pointer");
  FISDF_CHECK(nk >= 1 && nk <= 65535, "get_pp: 1 to 65535 k-points");
  FISDF_CHECK(nao >= 1 && nao <= kKfftMaxNao, "get_pp: nao must be in [1, 32768]");
  FISDF_CHECK(work_bytes >= 0, "get_pp: negative work_bytes");
  for (int i = 0; i < 3 * nk; ++i) FISDF_CHECK(std::isfinite(h_kpts[i]), "get_pp: bad k-point");
  long ngl = 0;
  FISDF_TRY(potential_check(mesh, a, 1, &ngl));
  FISDF_CHECK(f_kstride >= ngl * nao, "get_pp: f_kstride below ngrid * nao");
  FISDF_TRY(pp_check_table(atoms, natm, "get_pp"));
  PpPlan p;
  pp_plan(nao, ngl, nk, atoms, natm, with_nonlocal, work_bytes, &p);
  FISDF_CHECK(p.ok, "get_pp: work_bytes below the projector rows of one atom");
  // the FFT's own checks of the mesh, for the potential's row and for the largest chunk
  FISDF_TRY(fft3d_check(std::max(1, p.chunk_rows), mesh[0], mesh[1], mesh[2]));
  CellGeom g;
  lattice(a, g);
  const double vol = cell_volume(a);
  const int ngrid = (int)ngl;
  void* base;
  FISDF_TRY(arena_get(c, (size_t)p.bytes, &base));
  auto at = [&](long off) { return (char*)base + off; };
  cplx* v = (cplx*)at(p.off_v);
  cplx* rows = (cplx*)at(p.off_rows);
  cplx* part = (cplx*)at(p.off_part);
  cplx* cc = (cplx*)at(p.off_c);
  double* tab = (double*)at(p.off_tab);
  PpBlock* dblk = (PpBlock*)at(p.off_blk);
  cplx* out = (cplx*)outv;
  // the local part: conj(V_G) / vol, one forward transform = conj(v), its real part, the Gram
  std::vector<double> htab;
  pp_vloc_table(atoms, natm, &htab);
  FISDF_TRY(upload_bytes(c, htab.data(), sizeof(double) * htab.size(), tab));
  FISDF_TRY(vloc_g(c->stream, mesh, g, tab, natm, 1.0 / vol, 1, v));
  FISDF_TRY(fft3d(c->stream, v, ngl, nullptr, v, ngl, 1, mesh[0], mesh[1], mesh[2], nullptr, nullptr,
                  nullptr));
  FISDF_TRY(zero_imag(c->stream, v, ngl));
  FISDF_TRY(weighted_gram(c->stream, (const cplx*)fv, f_kstride, nk, ngrid, nao, v, 1, 0,
                          vol / (double)ngl, out, (cplx*)at(p.off_gram), p.gram_elems));
  // the non-local part, k by k and chunk by chunk: every chunk's channels lie one behind the other
  std::vector<int> blk0(p.nchunk + 1, 0);
  for (int ch = 0; ch < p.nchunk; ++ch) {
    std::vector<PpBlock> blk;
    pp_blocks(atoms, p.chunk_a[ch], p.chunk_a[ch + 1], &blk);
    FISDF_TRY(upload_bytes(c, blk.data(), sizeof(PpBlock) * blk.size(), dblk + blk0[ch]));
    blk0[ch + 1] = blk0[ch] + (int)blk.size();
  }
  for (int k = 0; k < nk; ++k) {
    const double* kp = h_kpts + 3 * k;
    double kd[3];
    for (int d = 0; d < 3; ++d) kd[d] = g.a[d][0] * kp[0] + g.a[d][1] * kp[1] + g.a[d][2] * kp[2];
    const bool gamma = std::fabs(kp[0]) + std::fabs(kp[1]) + std::fabs(kp[2]) < 1e-9;
    cplx* out_k = out + (long)k * nao * nao;
    for (int ch = 0; ch < p.nchunk; ++ch) {
      const int nb = blk0[ch + 1] - blk0[ch];
      const int np = (int)pp_rows(atoms, p.chunk_a[ch], p.chunk_a[ch + 1]);
      if (nb == 0) continue;
      FISDF_TRY(gth_projectors(c->stream, mesh, g, kp, dblk + blk0[ch], nb, rows));
      FISDF_TRY(fft3d(c->stream, rows, ngl, nullptr, rows, ngl, np, mesh[0], mesh[1], mesh[2],
                      nullptr, nullptr, nullptr));
      FISDF_TRY(pp_overlap(c->stream, rows, np, (const cplx*)fv + (long)k * f_kstride, nao, mesh,
                           gamma ? nullptr : kd, 1.0 / (double)ngl, cc, part));
      FISDF_TRY(pp_vnl(c->stream, cc, nao, dblk + blk0[ch], nb, out_k));
    }
    if (gamma) FISDF_TRY(zero_imag(c->stream, out_k, (long)nao * nao));
  }
  return 0;
}

// ---- A8 -----------------------------------------------------------------------
static int get_k_block(fisdf_ctx* c, const void* Xv, const double* Ws_rows, long ws_Rstride,
                       const void* dmsv, int nset, int nip, int nao, const int kmesh[3],
                       const double a[9], int i0, int i1, void* vkv);

// the host checks of both row forms, made before anything is enqueued
static int get_k_check(const void* Xv, const void* Wsv, const void* dmsv, int nset, int nip,
                       int nao, const int kmesh[3], const double a[9], int i0, int i1,
                       const void* vkv) {
  FISDF_CHECK(Xv && Wsv && dmsv && vkv && kmesh && a,
              "get_k: null X, W_s, density matrices, k-mesh, lattice or output");
  FISDF_CHECK(nset >= 1 && nip >= 1 && nao >= 1, "get_k: a size below 1");
  FISDF_TRY(kmesh_check(kmesh, "get_k"));
  FISDF_CHECK(0 <= i0 && i0 <= i1 && i1 <= nip, "get_k: bad row range");
  return 0;
}

int fisdf_get_k_rows(fisdf_ctx* c, const void* Xv, const void* Wsv, const void* dmsv, int nset,
                     int nip, int nao, const int kmesh[3], const double a[9], int i0, int i1,
                     void* vkv) {
  FISDF_TRY(device_guard(c));
  FISDF_TRY(get_k_check(Xv, Wsv, dmsv, nset, nip, nao, kmesh, a, i0, i1, vkv));
  // rows i0.. of W_s[R] inside the full (nk, nip, nip) array
  return get_k_block(c, Xv, (const double*)Wsv + (long)i0 * nip, (long)nip * nip, dmsv, nset, nip,
                     nao, kmesh, a, i0, i1, vkv);
}

int fisdf_get_k_rows_local(fisdf_ctx* c, const void* Xv, const void* Ws_rows, const void* dmsv,
                           int nset, int nip, int nao, const int kmesh[3], const double a[9],
                           int i0, int i1, void* vkv) {
  FISDF_TRY(device_guard(c));
  FISDF_TRY(get_k_check(Xv, Ws_rows, dmsv, nset, nip, nao, kmesh, a, i0, i1, vkv));
  // this rank's rows only: (nk, i1 - i0, nip) from fisdf_build_ws_rows + a reduce-scatter
  return get_k_block(c, Xv, (const double*)Ws_rows, (long)(i1 - i0) * nip, dmsv, nset, nip, nao,
                     kmesh, a, i0, i1, vkv);
}

// get_k's transform pair in place on B1 (nk rows of bn columns; B2 a buffer of the same size):
// rho_s = Phi rho_k (:215), V_s = W_s * Re(rho_s) (:219), V_k = Phi^T V_s (:222).  use_reg: one
// register pass per column where the k-mesh has one (round 6, C3: 0.50 -> ~0.2 ms; *reg_ran);
// otherwise two dense Phi GEMMs
static int k_wsrho_pair(fisdf_ctx* c, const int kmesh[3], const cplx* phase, cplx* B1, cplx* B2,
                        long bn, const double* Ws_rows, long ws_Rstride, bool use_reg,
                        unsigned long long* mon, bool* reg_ran) {
  const int nk = kmesh[0] * kmesh[1] * kmesh[2];
  *reg_ran = false;
  if (use_reg) FISDF_TRY(k_wsrho_reg(c->stream, B1, bn, kmesh, Ws_rows, ws_Rstride, mon, reg_ran));
  if (*reg_ran) return 0;
  // rho_s = Phi rho_k (:215), real (:216), and V_s = W_s * rho_s^T (:219) for the block
  // rows, both in the GEMM's epilogue (EPI_WSRHO: Re(W_s) Re(.), max |Im rho_s| recorded)
  FISDF_TRY(zgemm(c->stream, OP_N, OP_N, nk, bn, nk, ONE, phase, nk, 0, B1, bn, 0, ZERO, B2, bn, 0,
                  1, 1, (cplx*)(void*)Ws_rows, EPI_WSRHO, mon, GEMM_FULL, ws_Rstride));
  // V_k = Phi^T V_s (:222)
  FISDF_TRY(zgemm(c->stream, OP_T, OP_N, nk, bn, nk, ONE, phase, nk, 0, B2, bn, 0, ZERO, B1, bn, 0,
                  1));
  return 0;
}

static int get_k_block(fisdf_ctx* c, const void* Xv, const double* Ws_rows, long ws_Rstride,
                       const void* dmsv, int nset, int nip, int nao, const int kmesh[3],
                       const double a[9], int i0, int i1, void* vkv) {
  StageTimer tm(c, FISDF_ST_K);
  const int nk = kmesh[0] * kmesh[1] * kmesh[2];
  const cplx* phase;
  FISDF_TRY(get_phase(c, kmesh, a, &phase));
  const cplx* X = (const cplx*)Xv;
  const cplx* dms = (const cplx*)dmsv;
  cplx* vk = (cplx*)vkv;
  const int nb = i1 - i0;
  const long xs = (long)nip * nao, ds = (long)nao * nao, bn = (long)nb * nip, ba = (long)nb * nao;
  if (nb == 0) {
    FISDF_HIP(hipMemsetAsync(vk, 0, sizeof(cplx) * nset * nk * ds, c->stream));
    return 0;
  }
  Carver cv;
  size_t oT = cv.take(sizeof(cplx) * nk * ba);
  size_t o1 = cv.take(sizeof(cplx) * nk * bn);
  size_t o2 = cv.take(sizeof(cplx) * nk * bn);
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  cplx* T = (cplx*)((char*)base + oT);
  cplx* B1 = (cplx*)((char*)base + o1);
  cplx* B2 = (cplx*)((char*)base + o2);
  const cplx* Xb = X + (long)i0 * nao;
  for (int x = 0; x < nset; ++x) {
    const cplx* dm = dms + (long)x * nk * ds;
    // rho_k^T[I, J] = rho_k[J, I] = (conj(X_k[I]) D_k^T X_k^T)[I, J] / nk for the block rows
    // (:211-212, transposed at the source so :219's product is element-wise)
    FISDF_TRY(zgemm(c->stream, OP_R, OP_T, nb, nao, nao, cmk(1.0 / nk, 0), Xb, nao, xs, dm, nao, ds,
                    ZERO, T, nao, ba, nk));
    if (nk == 1) {
      // Gamma only (Phi = 1): rho_s = Re(rho_k) (:215-216) and V = W_s * rho_s^T (:219) in this
      // GEMM's epilogue; V_k = V_s (:222)
      FISDF_TRY(zgemm(c->stream, OP_N, OP_T, nb, nip, nao, ONE, T, nao, ba, X, nao, xs, ZERO, B1,
                      nip, bn, 1, 1, (cplx*)(void*)Ws_rows, EPI_WSRHO, c->maximag + 2, GEMM_FULL,
                      (long)nip));
    } else {
      FISDF_TRY(zgemm(c->stream, OP_N, OP_T, nb, nip, nao, ONE, T, nao, ba, X, nao, xs, ZERO, B1,
                      nip, bn, nk));
      // FISDF_K_DFT=0 (read per call: the GPU tests compare) keeps the GEMMs
      const char* kd = getenv("FISDF_K_DFT");
      bool reg = false;
      FISDF_TRY(k_wsrho_pair(c, kmesh, phase, B1, B2, bn, Ws_rows, ws_Rstride,
                             !(kd && kd[0] == '0'), c->maximag + 2, &reg));
    }
    // K_k (block part) = X_k[I]^H (V_k[I, :] X_k)  (:225)
    FISDF_TRY(zgemm(c->stream, OP_N, OP_N, nb, nao, nip, ONE, B1, nip, bn, X, nao, xs, ZERO, T,
                    nao, ba, nk));
    FISDF_TRY(zgemm(c->stream, OP_C, OP_N, nao, nao, nb, ONE, Xb, nao, xs, T, nao, ba, ZERO,
                    vk + (long)x * nk * ds, nao, ds, nk));
  }
  return 0;
}

int fisdf_get_k(fisdf_ctx* c, const void* Xv, const void* Wsv, const void* dmsv, int nset, int nip,
                int nao, const int kmesh[3], const double a[9], void* vkv) {
  return fisdf_get_k_rows(c, Xv, Wsv, dmsv, nset, nip, nao, kmesh, a, 0, nip, vkv);
}

// ---- the separable k-mesh transforms piece by piece, for tests of their dispatch --------------
int fisdf_kmesh_plan(const int kmesh[3], long ncol, int nao, int nip, int m, long* h_route,
                     int* h_half_count, int* h_runs, int runs_cap, int* h_nruns, int* h_fused,
                     int* h_slots, long* h_fused_bytes) {
  t_cur_ctx = nullptr;
  FISDF_CHECK(kmesh && kmesh[0] >= 1 && kmesh[1] >= 1 && kmesh[2] >= 1 && ncol >= 0,
              "kmesh_plan: bad sizes");
  const KmeshPlan kp = kmesh_route(kmesh, ncol);
  if (h_route) {
    h_route[0] = kp.route;
    h_route[1] = kp.CT;
    h_route[2] = (long)kp.lds;
  }
  if (h_half_count) *h_half_count = kmesh_half_count(kmesh);
  if (h_runs || h_nruns) {
    std::vector<int> runs;
    FISDF_TRY(kmesh_rep_runs(kmesh, &runs));
    const int nr = (int)runs.size() / 2;
    FISDF_CHECK(!h_runs || runs_cap >= nr, "kmesh_plan: h_runs too short");
    if (h_nruns) *h_nruns = nr;
    if (h_runs) std::memcpy(h_runs, runs.data(), sizeof(int) * runs.size());
  }
  YFusedPlan yp;
  y_fused_plan(kmesh, nao, &yp);
  if (h_fused) {
    h_fused[0] = yp.applies ? 1 : 0;
    h_fused[1] = yp.nA;
    h_fused[2] = yp.nB;
    h_fused[3] = yp.nkc;
  }
  if (h_slots)
    for (int i = 0; i < 48; ++i) h_slots[i] = i < yp.nA ? yp.kA[i] : (i - yp.nA < yp.nB ? yp.kB[i - yp.nA] : -1);
  if (h_fused_bytes) {
    h_fused_bytes[0] = (long)yp.lds;
    h_fused_bytes[1] = (long)y_fused_workspace(kmesh, nip, nao, m);
  }
  return 0;
}

// a device monitor word and a device q-list in the arena behind `extra` bytes of workspace
static int kmesh_test_scratch(fisdf_ctx* c, size_t extra, const int* h_qs, int nq, char** work,
                              unsigned long long** mon, int** dq) {
  Carver cv;
  const size_t oW = cv.take(extra), oM = cv.take(sizeof(unsigned long long)),
               oQ = cv.take(sizeof(int) * (size_t)std::max(nq, 1));
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  *work = (char*)base + oW;
  *mon = (unsigned long long*)((char*)base + oM);
  *dq = (int*)((char*)base + oQ);
  FISDF_HIP(hipMemsetAsync(*mon, 0, sizeof(unsigned long long), c->stream));
  FISDF_TRY(upload_ints(c, h_qs, nq, *dq));
  return 0;
}

static int kmesh_test_monitor(fisdf_ctx* c, const unsigned long long* mon, double* h_mon) {
  unsigned long long bits = 0;
  FISDF_HIP(hipMemcpyAsync(&bits, mon, sizeof(bits), hipMemcpyDeviceToHost, c->stream));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  if (h_mon) std::memcpy(h_mon, &bits, sizeof(double));
  return 0;
}

int fisdf_kmesh_y_ex(fisdf_ctx* c, const void* FX, long ncol, const int kmesh[3], const int* h_qs,
                     int nq, int m, void* yT, long qs, long Is, long goff, int half, int conj_out,
                     double* h_mon, int* h_route) {
  FISDF_TRY(device_guard(c));
  if (h_route) *h_route = -1;
  FISDF_CHECK(FX && yT && kmesh && ncol >= 0 && m >= 1 && qs >= 0 && Is >= 0 && goff >= 0,
              "kmesh_y_ex: bad arguments");
  FISDF_TRY(kmesh_check(kmesh, "kmesh_y_ex"));
  FISDF_TRY(check_qlist(h_qs, nq, kmesh[0] * kmesh[1] * kmesh[2], "kmesh_y_ex"));
  const KmeshPlan kp = kmesh_route(kmesh, ncol);
  FISDF_CHECK(kp.route != KM_REFUSED, "kmesh_y_ex: too many columns");
  FISDF_CHECK(!conj_out || kp.route == KM_REG,
              "kmesh_y_ex: conj_out needs the register kernel's k-mesh");
  char* work;
  unsigned long long* mon;
  int* dq;
  FISDF_TRY(kmesh_test_scratch(c, 0, h_qs, nq, &work, &mon, &dq));
  FISDF_TRY(kmesh_y(c->stream, (const cplx*)FX, ncol, kmesh, h_qs, dq, nq, m, (cplx*)yT, qs, Is,
                    goff, half != 0, mon, conj_out != 0));
  FISDF_TRY(kmesh_test_monitor(c, mon, h_mon));
  if (h_route && ncol > 0) *h_route = kp.route;
  return 0;
}

int fisdf_y_fused_ex(fisdf_ctx* c, const void* X, int nip, int nao, const void* F, long fks, int m,
                     const int kmesh[3], const int* h_qs, int nq, void* yT, long qs, long Is,
                     long goff, unsigned long long rmask, int* h_handled) {
  FISDF_TRY(device_guard(c));
  if (h_handled) *h_handled = 0;
  FISDF_CHECK(X && F && yT && kmesh && nip >= 1 && nao >= 1 && m >= 1 && fks >= 0 && qs >= 0 &&
                  Is >= 0 && goff >= 0,
              "y_fused_ex: bad arguments");
  FISDF_TRY(kmesh_check(kmesh, "y_fused_ex"));
  FISDF_TRY(check_qlist(h_qs, nq, kmesh[0] * kmesh[1] * kmesh[2], "y_fused_ex"));
  if (!y_fused_applies(kmesh, nao)) return 0;
  const size_t yw = y_fused_workspace(kmesh, nip, nao, m);
  FISDF_CHECK(yw > 0, "y_fused_ex: no workspace for a k-mesh the fused kernel takes");
  char* work;
  unsigned long long* mon;
  int* dq;
  FISDF_TRY(kmesh_test_scratch(c, yw, h_qs, nq, &work, &mon, &dq));
  bool done = false;
  FISDF_TRY(y_fused(c->stream, (const cplx*)X, nip, nao, (const cplx*)F, fks, m, kmesh, h_qs, nq,
                    (cplx*)yT, qs, Is, goff, mon, (cplx*)work, yw, rmask, &done));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  if (h_handled) *h_handled = done ? 1 : 0;
  return 0;
}

int fisdf_y_fused_stream_ex(fisdf_ctx* c, const void* x0, int ng0, int nao, const int* h_piv,
                            int nip, int rows, const void* F, long fks, int m, const int kmesh[3],
                            const int* h_qs, int nq, void* yT, long qs, long Is, long goff,
                            unsigned long long rmask, int two_streams, int* h_handled,
                            int* h_err) {
  FISDF_TRY(device_guard(c));
  if (h_handled) *h_handled = 0;
  if (h_err) *h_err = 0;
  FISDF_CHECK(x0 && F && yT && kmesh && h_piv && ng0 >= 1 && nip >= 1 && nao >= 1 && m >= 1 &&
                  fks >= 0 && qs >= 0 && Is >= 0 && goff >= 0,
              "y_fused_stream_ex: bad arguments");
  FISDF_CHECK(rows >= 16 && rows % 16 == 0 && rows <= 64 * 16, "y_fused_stream_ex: bad row block");
  for (int i = 0; i < nip; ++i)
    FISDF_CHECK(h_piv[i] >= 0 && h_piv[i] < ng0, "y_fused_stream_ex: pivot out of range");
  FISDF_TRY(kmesh_check(kmesh, "y_fused_stream_ex"));
  FISDF_TRY(check_qlist(h_qs, nq, kmesh[0] * kmesh[1] * kmesh[2], "y_fused_stream_ex"));
  if (!y_fused_applies(kmesh, nao)) return 0;
  const size_t yw = y_fused_workspace(kmesh, nip, nao, m);
  FISDF_CHECK(yw > 0, "y_fused_stream_ex: no workspace for a k-mesh the fused kernel takes");
  // behind the workspace: the pivots, then the progress word (already "done": the bounded wait of
  // the XT kernel never spins) and the error flag
  Carver cv;
  const size_t oW = cv.take(yw), oP = cv.take(sizeof(int) * ((size_t)nip + 2));
  void* base;
  FISDF_TRY(arena_get(c, cv.off, &base));
  int* dpiv = (int*)((char*)base + oP);
  std::vector<int> h(h_piv, h_piv + nip);
  h.push_back(kSelDone);
  h.push_back(0);
  FISDF_TRY(upload_ints(c, h.data(), nip + 2, dpiv));
  hipStream_t s2 = nullptr;
  hipEvent_t ea = nullptr, eb = nullptr;
  int rc = 0;
  bool done = false;
  if (two_streams) {
    if (hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ea, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&eb, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      set_error("fisdf: y_fused_stream_ex: could not create the second stream");
      rc = -2;
    }
  }
  if (rc == 0)
    rc = y_fused_stream(c->stream, (const cplx*)x0, ng0, nao, dpiv, dpiv + nip, dpiv + nip + 1, nip,
                        rows, (const cplx*)F, fks, m, kmesh, h_qs, nq, (cplx*)yT, qs, Is, goff,
                        (cplx*)((char*)base + oW), yw, rmask, &done, s2, ea, eb);
  int err = 0;
  if (s2) (void)hipStreamSynchronize(s2);
  if (rc == 0 && hipMemcpyAsync(&err, dpiv + nip + 1, sizeof(int), hipMemcpyDeviceToHost,
                                c->stream) != hipSuccess) {
    (void)hipGetLastError();
    set_error("fisdf: y_fused_stream_ex: reading the error flag failed");
    rc = -2;
  }
  (void)hipStreamSynchronize(c->stream);
  if (ea) (void)hipEventDestroy(ea);
  if (eb) (void)hipEventDestroy(eb);
  if (s2) (void)hipStreamDestroy(s2);
  if (rc != 0) return rc;
  if (h_handled) *h_handled = done ? 1 : 0;
  if (h_err) *h_err = err;
  return 0;
}

int fisdf_k_wsrho_ex(fisdf_ctx* c, void* B, long ncol, const int kmesh[3], const double a[9],
                     const void* Ws, long ws_Rstride, int use_reg, double* h_mon,
                     int* h_handled) {
  FISDF_TRY(device_guard(c));
  if (h_handled) *h_handled = 0;
  FISDF_CHECK(B && Ws && kmesh && a && ncol >= 1 && ncol < (1L << 31) && ws_Rstride >= ncol,
              "k_wsrho_ex: bad arguments");
  FISDF_TRY(kmesh_check(kmesh, "k_wsrho_ex"));
  const int nk = kmesh[0] * kmesh[1] * kmesh[2];
  const cplx* phase;
  FISDF_TRY(get_phase(c, kmesh, a, &phase));
  char* work;
  unsigned long long* mon;
  int* dq;
  FISDF_TRY(kmesh_test_scratch(c, sizeof(cplx) * (size_t)nk * ncol, nullptr, 0, &work, &mon, &dq));
  bool reg = false;
  FISDF_TRY(k_wsrho_pair(c, kmesh, phase, (cplx*)B, (cplx*)work, ncol, (const double*)Ws,
                         ws_Rstride, use_reg != 0, mon, &reg));
  FISDF_TRY(kmesh_test_monitor(c, mon, h_mon));
  if (h_handled) *h_handled = reg ? 1 : 0;
  return 0;
}

int fisdf_bloch_dft_ex(fisdf_ctx* c, const void* F, long ncol, const int kmesh[3], void* chi,
                       int* h_route) {
  FISDF_TRY(device_guard(c));
  if (h_route) *h_route = -1;
  FISDF_CHECK(F && chi && kmesh && ncol >= 0, "bloch_dft_ex: bad arguments");
  int route = -1;
  FISDF_TRY(bloch_dft(c->stream, (const double*)F, ncol, kmesh, (cplx*)chi, &route));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  if (h_route && ncol > 0) *h_route = route;
  return 0;
}

int fisdf_bloch_band_ex(fisdf_ctx* c, const void* F, long ncol, int nT, const void* ph, int nkb,
                        void* chi) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(F && ph && chi, "bloch_band_ex: bad arguments");
  FISDF_TRY(bloch_band(c->stream, (const double*)F, ncol, nT, (const cplx*)ph, nkb, (cplx*)chi));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

// ---- composite entries --------------------------------------------------------
}  // extern "C"

namespace {

enum BuildRole { BR_X = 0, BR_X4 = 1, BR_Y = 2, BR_WQ = 3, BR_WS = 4, BR_SEND = 5, BR_WSB = 6,
                 BR_W0 = 7 };

// a buffer of the composite build: the caller's allocator, or a library-owned grow-only buffer
int build_alloc(fisdf_ctx* c, int role, size_t bytes, void** out) {
  bytes = std::max<size_t>(bytes, 256);
  if (c->alloc_fn) {
    void* p = c->alloc_fn(bytes, c->alloc_user);
    FISDF_CHECK(p != nullptr, "build: the caller's allocator returned NULL");
    c->lent.push_back(p);
    *out = p;
    return 0;
  }
  auto& o = c->owned[role];
  if (o.second < bytes) {
    if (o.first) {
      FISDF_HIP(hipStreamSynchronize(c->stream));
      FISDF_HIP(hipFree(o.first));
    }
    o = {nullptr, 0};
    FISDF_HIP(hipMalloc(&o.first, bytes));
    o.second = bytes;
  }
  *out = o.first;
  return 0;
}

// hand one lent buffer back (stream-ordered: its last use is enqueued on c->stream, and every
// aux stream that read it has been joined into c->stream — checked)
int build_return(fisdf_ctx* c, void* p) {
  if (!c->alloc_fn || !p) return 0;
  auto it = std::find(c->lent.begin(), c->lent.end(), p);
  if (it == c->lent.end()) return 0;
  FISDF_TRY(check_aux_joined(c, "build_return"));
  c->lent.erase(it);
  if (c->free_fn) c->free_fn(p, c->alloc_user);
  return 0;
}

void build_return_all(fisdf_ctx* c) {
  // an earlier call that failed between a fork and its join may have left an aux stream with
  // work: drain it before the caller's allocator gets the buffers back (likewise the sharded
  // build's collective stream, whose exchange reads and writes the build's y buffers)
  for (int i = 0; i < 3; ++i)
    if (c->aux_joined[i] != c->aux_use[i]) {
      if (c->aux[i]) (void)hipStreamSynchronize(c->aux[i]);
      c->aux_joined[i] = c->aux_use[i];
    }
  if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
  // y-readiness marks left by a build that failed before its fit consumed them
  c->ready_marked.assign(c->ready_marked.size(), 0);
  c->y_piece.clear();
  std::vector<void*> l;
  l.swap(c->lent);
  if (c->free_fn)
    for (void* p : l) c->free_fn(p, c->alloc_user);
  c->bld = fisdf_ctx::Build();
}

// time-reversal classes of the q-mesh (get_kpts order): partner[q] = index of -q, the fitted
// representatives (smaller index of each pair) and their W_s weights (2 unless self-paired)
void tr_classes(const int km[3], bool on, std::vector<int>& reps, std::vector<int>& partner,
                std::vector<double>& wt) {
  const int nk = km[0] * km[1] * km[2];
  partner.resize(nk);
  reps.clear();
  wt.clear();
  for (int q = 0; q < nk; ++q) {
    const int i2 = q % km[2], i1 = (q / km[2]) % km[1], i0 = q / (km[1] * km[2]);
    partner[q] = (((km[0] - i0) % km[0]) * km[1] + (km[1] - i1) % km[1]) * km[2] + (km[2] - i2) % km[2];
  }
  for (int q = 0; q < nk; ++q) {
    if (!on) {  // every q fitted on its own (W_s weights 1)
      partner[q] = q;
      reps.push_back(q);
      wt.push_back(1.0);
    } else if (partner[q] >= q) {
      reps.push_back(q);
      wt.push_back(partner[q] == q ? 1.0 : 2.0);
    }
  }
}

// time reversal of the AO inputs (what the fold over k <= -k of the selection Gram, x4 and y, and
// W_{-q} = conj(W_q), rely on): a[-k] = conj(a[k]) holds for real basis functions on a k-mesh
// containing -k (get_kpts order, no shift).  The check reads all of x0 (the selection's input,
// 45 MB at C3) and every 61st grid point of f (x0 and f come from one basis: the whole 1.24 GB of
// f cost 0.7 ms/step beside the selection and the y build, profiles/r05/tr_check/) on stream `st`
// and lands in tr_pinned behind ev_tr; tr_verdict waits for it.
int tr_alloc(fisdf_ctx* c) {
  if (c->trmon) return 0;
  FISDF_HIP(hipMalloc(&c->trmon, 4 * sizeof(unsigned long long)));
  FISDF_HIP(hipHostMalloc((void**)&c->tr_pinned, 4 * sizeof(unsigned long long),
                          hipHostMallocDefault));
  FISDF_HIP(hipEventCreateWithFlags(&c->ev_tr, hipEventDisableTiming));
  FISDF_HIP(hipEventRecord(c->ev_tr, c->stream));
  return 0;
}

constexpr long kTrFStride = 61;  // grid-point sampling of f in the composite build's check

int tr_check_enqueue(fisdf_ctx* c, hipStream_t st, const cplx* x0, long ng0, const cplx* f,
                     long ngrid, int nao, const int kmesh[3]) {
  FISDF_TRY(tr_alloc(c));
  FISDF_HIP(hipEventSynchronize(c->ev_tr));  // the pinned words are rewritten below
  FISDF_HIP(hipMemsetAsync(c->trmon, 0, 4 * sizeof(unsigned long long), st));
  FISDF_TRY(tr_check(st, x0, ng0 * nao, ng0, nao, 1, kmesh, c->trmon));
  if (f) FISDF_TRY(tr_check(st, f, ngrid * nao, ngrid, nao, kTrFStride, kmesh, c->trmon + 2));
  FISDF_HIP(hipMemcpyAsync(c->tr_pinned, c->trmon, 4 * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, st));
  FISDF_HIP(hipEventRecord(c->ev_tr, st));
  return 0;
}

// the largest relative violation max |a[-k] - conj(a[k])| / max |a| of the last check
int tr_verdict(fisdf_ctx* c, double* rel) {
  FISDF_HIP(hipEventSynchronize(c->ev_tr));
  double v[4];
  for (int i = 0; i < 4; ++i) v[i] = __builtin_bit_cast(double, c->tr_pinned[i]);
  *rel = 0.0;
  for (int i = 0; i < 2; ++i)
    if (v[2 * i + 1] > 0.0) *rel = std::max(*rel, v[2 * i] / v[2 * i + 1]);
  return 0;
}

// tolerance of the check: rounding of the lattice phases e^{ik.T} is ~1e-15 relative; a complex
// basis or a shifted k-mesh violates the symmetry at O(1)
constexpr double kTrTol = 1e-9;

// the composite build's context-wide stage settings, restored when fisdf_build returns (ADVICE
// r04: a stage-API caller on the same context must not inherit them)
struct StageSettings {
  fisdf_ctx* c;
  bool time_reversal;
  int force_pivoted, fit_mode, half_grid, factor_hi;
  double omega;
  explicit StageSettings(fisdf_ctx* cc)
      : c(cc), time_reversal(cc->time_reversal), force_pivoted(cc->force_pivoted),
        fit_mode(cc->fit_mode), half_grid(cc->half_grid), factor_hi(cc->factor_hi),
        omega(cc->omega) {}
  ~StageSettings() {
    c->time_reversal = time_reversal;
    c->force_pivoted = force_pivoted;
    c->fit_mode = fit_mode;
    c->half_grid = half_grid;
    c->factor_hi = factor_hi;
    c->omega = omega;
  }
};

}  // namespace

extern "C" {

int fisdf_check_time_reversal(fisdf_ctx* c, const void* d_a, long k_stride, long per_k,
                              const int kmesh[3], double* h_out) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(d_a && kmesh && h_out, "check_time_reversal: null argument");
  FISDF_CHECK(kmesh[0] > 0 && kmesh[1] > 0 && kmesh[2] > 0, "check_time_reversal: bad k-mesh");
  FISDF_CHECK(per_k > 0 && k_stride >= per_k, "check_time_reversal: bad sizes");
  FISDF_TRY(tr_alloc(c));
  FISDF_HIP(hipEventSynchronize(c->ev_tr));
  FISDF_HIP(hipMemsetAsync(c->trmon, 0, 4 * sizeof(unsigned long long), c->stream));
  FISDF_TRY(tr_check(c->stream, (const cplx*)d_a, k_stride, per_k, 1, 1, kmesh, c->trmon));
  unsigned long long h[2];
  FISDF_HIP(hipMemcpyAsync(h, c->trmon, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  h_out[0] = __builtin_bit_cast(double, h[0]);
  h_out[1] = __builtin_bit_cast(double, h[1]);
  return 0;
}

void fisdf_build_opts_default(fisdf_build_opts* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->nip_max = 0;
  o->select_tol = -1.0;
  o->perm = nullptr;
  o->n_perm = 0;
  o->fit_mode = FISDF_FIT_LSTSQ;
  o->fit_tol = kFitTolDefault;
  o->pivoted_fit = -1;
  o->half_grid = -1;
  o->time_reversal = 1;
  o->real_self_conjugate = 1;
  o->omega = 0.0;
}

int fisdf_set_allocator(fisdf_ctx* c, fisdf_alloc_fn alloc, fisdf_free_fn release, void* user) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK((alloc == nullptr) == (release == nullptr), "set_allocator: give both functions or neither");
  FISDF_TRY(fisdf_build_release(c));
  c->alloc_fn = alloc;
  c->free_fn = release;
  c->alloc_user = user;
  return 0;
}

int fisdf_build_release(fisdf_ctx* c) {
  FISDF_TRY(device_guard(c));
  if (c->f_pending) FISDF_TRY(fisdf_factor_x4_wait(c, nullptr));
  build_return_all(c);
  if (!c->owned.empty()) {
    FISDF_HIP(hipStreamSynchronize(c->stream));
    for (auto& kv : c->owned)
      if (kv.second.first) FISDF_HIP(hipFree(kv.second.first));
    c->owned.clear();
  }
  return 0;
}

}  // extern "C"

namespace {

// kshard.assign_q: longest-processing-time greedy over the fit positions (most expensive first,
// each to the least loaded rank, ties to the lower rank), each rank's positions ascending
std::vector<std::vector<int>> assign_q(const std::vector<double>& cost, int size) {
  std::vector<int> order(cost.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cost[x] > cost[y]; });
  std::vector<double> load(size, 0.0);
  std::vector<std::vector<int>> parts(size);
  for (int i : order) {
    int r = 0;
    for (int t = 1; t < size; ++t)
      if (load[t] < load[r]) r = t;
    parts[r].push_back(i);
    load[r] += cost[i];
  }
  for (auto& p : parts) std::sort(p.begin(), p.end());
  return parts;
}

// kshard.shard_range: contiguous balanced [lo, hi) of `rank` among `size`
void shard_range(long n, int rank, int size, long* lo, long* hi) {
  const long base = n / size, rem = n % size;
  *lo = rank * base + std::min<long>(rank, rem);
  *hi = *lo + base + (rank < rem ? 1 : 0);
}

int comm_check(int rc, const char* what) {
  FISDF_CHECK(rc == 0, std::string("build_sharded: the caller's ") + what + " failed");
  return 0;
}

// fisdf_build (comm NULL) and fisdf_build_sharded: ISDF.build() (fftisdf.py:308-325 ->
// build(df_obj), :22-128), the same stage sequence as the Python mirror's build (fisdf/isdf.py
// build(): its unsharded branch, and its k-sharded branch with the caller's collectives)
// FISDF_HOST_TRACE=1 (diagnosis): host timestamps (CLOCK_MONOTONIC, the clock of Python's
// time.perf_counter) of the composite build's hand-offs, to stderr — where the host holds the
// device idle between a step's last kernel and the next step's first
static void host_mark(const char* what) {
  static const bool on = getenv("FISDF_HOST_TRACE") != nullptr;
  if (!on) return;
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  fprintf(stderr, "fisdf-host %.6f %s\n", ts.tv_sec + 1e-9 * ts.tv_nsec, what);
}

int build_impl(fisdf_ctx* c, const fisdf_comm* comm, const void* x0, int ng0, const void* f,
               int nao, const int kmesh[3], const int mesh[3], const double a[9],
               const fisdf_build_opts* opts_in, int* h_nip) {
  host_mark("build enter");
  fisdf_build_opts o;
  fisdf_build_opts_default(&o);
  if (opts_in) o = *opts_in;
  FISDF_CHECK(x0 && f && kmesh && mesh && a && ng0 > 0 && nao > 0, "build: bad arguments");
  FISDF_CHECK(kmesh[0] > 0 && kmesh[1] > 0 && kmesh[2] > 0 && mesh[0] > 0 && mesh[1] > 0 && mesh[2] > 0,
              "build: bad k-mesh or mesh");
  FISDF_CHECK(o.fit_mode >= FISDF_FIT_LSTSQ && o.fit_mode <= FISDF_FIT_BASIC, "build: bad fit_mode");
  FISDF_CHECK(o.perm == nullptr || o.n_perm > 0, "build: perm given without n_perm");
  // the previous build's factor chain may still read x4: wait for it before anything else
  if (c->f_pending) FISDF_TRY(fisdf_factor_x4_wait(c, nullptr));
  StageSettings keep(c);
  fisdf_ctx::Build& B = c->bld;
  const int nk = kmesh[0] * kmesh[1] * kmesh[2];
  const long ngrid = (long)mesh[0] * mesh[1] * mesh[2];
  FISDF_CHECK(ngrid < (1L << 31), "build: mesh too large");
  const int NR = comm ? comm->size : 1, RK = comm ? comm->rank : 0;
  if (comm)
    FISDF_CHECK(NR >= 1 && RK >= 0 && RK < NR && comm->all_to_all && comm->reduce_scatter_f64 &&
                    comm->allreduce_f64 && comm->broadcast,
                "build_sharded: incomplete fisdf_comm");
  // a k-shard's 1/N-grid y build is short, so its factor chain runs at the greatest priority
  // FISDF_FACTOR_PRIO=0/1 (A/B) overrides: 1-GPU least, k-shard greatest
  const char* fpe = getenv("FISDF_FACTOR_PRIO");
  FISDF_TRY(fisdf_set_factor_priority(c, fpe ? (fpe[0] == '1' ? 1 : 0) : (NR > 1 ? 1 : 0)));
  // time reversal (X_{-k} = conj(X_k), real AOs): the selection Gram, x2_k (x4) and fx_k (y)
  // are formed for the representatives k <= -k only.  The inputs are checked on the side
  // stream beside the selection; a violation (complex basis, shifted k-mesh) is found when the
  // selection returns, and the build then starts over with every q fitted
  bool tr = o.time_reversal != 0;
  double tr_dev = 0.0;
  // FISDF_TR_CHECK=0 trusts the inputs (A/B of the check's cost only)
  static const bool tr_check_on = [] {
    const char* e = getenv("FISDF_TR_CHECK");
    return !(e && e[0] == '0');
  }();
  // the check (~25 us) runs on the main stream ahead of the selection, whose read-back brings
  // the verdict along; a violation redoes the selection without the fold and fits every q
  const bool check_tr = tr && tr_check_on;
  if (check_tr) {
    FISDF_TRY(tr_alloc(c));
    FISDF_TRY(tr_check_enqueue(c, c->stream, (const cplx*)x0, ng0, (const cplx*)f, ngrid, nao,
                               kmesh));
  }
  // the previous build's buffers go back to the caller's allocator now, while the check runs
  // (in the mirror each is a Python callback: done first, they left the GPU idle between steps)
  host_mark("tr check enqueued");
  build_return_all(c);
  host_mark("previous buffers returned");
  // X and x4 at their upper bound (the point cap) taken now, while the check runs: the caller's
  // allocator (a Python callback in the mirror, ~40 us each) then no longer sits in the idle gap
  // between the selection's read-back and the gather
  const int nip_ub = o.perm ? o.n_perm : (o.nip_max > 0 ? std::min(o.nip_max, ng0) : 0);
  void *X = nullptr, *x4 = nullptr;
  if (nip_ub > 0) {
    FISDF_TRY(build_alloc(c, BR_X, sizeof(cplx) * (size_t)nk * nip_ub * nao, &X));
    FISDF_TRY(build_alloc(c, BR_X4, sizeof(cplx) * (size_t)nk * nip_ub * nip_ub, &x4));
  }
  // The y build streamed behind the selection (1-GPU composite build, time reversal, a k-mesh
  // the fused kernel covers; FISDF_Y_STREAM=0: off): y is formed at the point cap nip_ub on
  // aux[0] while the selection runs, and is kept when the selection returns exactly nip_ub
  // points with time reversal confirmed — else it is discarded and built the usual way.
  // read per build: the GPU tests compare the two paths in one process (FISDF_Y_STREAM=0: off)
  const bool y_stream_env = [] {
    const char* e = getenv("FISDF_Y_STREAM");
    return !(e && e[0] == '0');
  }();
  static const bool y_real_env = [] {  // the self-conjugate q's y real; FISDF_Y_REAL=0: off
    const char* e = getenv("FISDF_Y_REAL");
    return !(e && e[0] == '0');
  }();
  struct YsScope {  // the request is this build's only: cleared on every exit
    fisdf_ctx* c;
    ~YsScope() {
      // an error between the enqueue and the join leaves the y stream joined all the same, so
      // the buffers it writes are not handed back under it
      (void)ystream_join(c);
      c->ys = fisdf_ctx::YStream();
    }
  } ys_scope{c};
  void* yT_pre = nullptr;  // the y buffer taken before the selection (streamed y)
  std::vector<int> ys_qs, ys_partner;
  std::vector<double> ys_wt;
  if (y_stream_env && !comm && !o.perm && tr && nip_ub > 0 && y_fused_applies(kmesh, nao)) {
    tr_classes(kmesh, true, ys_qs, ys_partner, ys_wt);
    FISDF_TRY(build_alloc(c, BR_Y, sizeof(cplx) * (size_t)ys_qs.size() * nip_ub * ngrid, &yT_pre));
    unsigned long long rmask = 0;
    if (y_real_env && o.real_self_conjugate && fft3d_reads_real(mesh[0], mesh[1], mesh[2]))
      for (int q : ys_qs) {
        const int i2 = q % kmesh[2], i1 = (q / kmesh[2]) % kmesh[1], i0 = q / (kmesh[1] * kmesh[2]);
        if ((2 * i0) % kmesh[0] == 0 && (2 * i1) % kmesh[1] == 0 && (2 * i2) % kmesh[2] == 0)
          rmask |= 1ull << q;
      }
    bool armed = false;
    FISDF_TRY(ystream_arm(c, x0, ng0, f, ngrid * nao, ngrid, nao, nip_ub, kmesh, ys_qs.data(),
                          (int)ys_qs.size(), yT_pre, rmask, &armed));
  }
  host_mark("allocations + y stream armed");
  // interpolation points (:33 -> :357-388), or the caller's
  std::vector<int> perm;
  for (int attempt = 0;; ++attempt) {
    FISDF_TRY(fisdf_set_time_reversal(c, tr ? 1 : 0));
    if (o.perm) {
      perm.assign(o.perm, o.perm + o.n_perm);
    } else {
      const int cap = o.nip_max > 0 ? std::min(o.nip_max, ng0) : ng0;
      perm.assign(cap, 0);
      int npiv = 0, full = 0;
      FISDF_TRY(fisdf_select_points_km(c, x0, kmesh, ng0, nao, cap, o.select_tol, perm.data(),
                                       &npiv, &full));
      c->ys.armed = false;  // a second selection (time reversal refuted) streams nothing
      perm.resize(std::min(cap, npiv));                                           // :383
    }
    if (!check_tr || attempt > 0) break;
    FISDF_TRY(tr_verdict(c, &tr_dev));
    if (tr_dev <= kTrTol) break;
    if (getenv("FISDF_VERBOSE"))
      fprintf(stderr, "fisdf: build: AO inputs violate time reversal (max |a[-k] - conj(a[k])| / "
                      "max |a| = %.3e): every q fitted\n", tr_dev);
    tr = false;
  }
  host_mark("selection read back");
  const int nip = (int)perm.size();
  FISDF_CHECK(nip > 0, "build: no interpolation points");
  const long nn = (long)nip * nip;
  FISDF_CHECK(nip_ub == 0 || nip <= nip_ub, "build: more points than the cap");
  if (!X) FISDF_TRY(build_alloc(c, BR_X, sizeof(cplx) * (size_t)nk * nip * nao, &X));
  FISDF_TRY(fisdf_gather_points(c, x0, nk, ng0, nao, perm.data(), nip, X));        // :388
  if (!x4) FISDF_TRY(build_alloc(c, BR_X4, sizeof(cplx) * (size_t)nk * nn, &x4));
  // FISDF_X4_SIDE=1 (experiment, read per build): with y streamed, x4 on the side stream at the
  // head of the factor chain it feeds.  Beside the streamed y its 0.2 ms DFT kernel stretches to
  // 2.6 ms on either stream and the chain after it to 4 ms; measured +0.3 ms/step on the side
  // stream, and no better at the greatest priority (profiles/r06/r06_x4side)
  const char* x4e = getenv("FISDF_X4_SIDE");
  const bool x4_side = !comm && (x4e && x4e[0] == '1') && c->ys.enqueued && !c->ys.stale && tr &&
                       nip == c->ys.nip;
  if (!x4_side) FISDF_TRY(fisdf_build_x4(c, X, nip, nao, kmesh, a, x4));           // :38-48
  std::vector<int> qs, partner;
  std::vector<double> wt;
  tr_classes(kmesh, tr, qs, partner, wt);
  const int nq = (int)qs.size();
  FISDF_TRY(fisdf_set_pivoted_fit(c, o.pivoted_fit));
  FISDF_TRY(fisdf_set_fit_mode(c, o.fit_mode));
  FISDF_TRY(fisdf_set_half_grid(c, o.half_grid));
  FISDF_TRY(fisdf_set_omega(c, o.omega));
  // this rank's q: the fitted q shared by cost, longest first (one GPU: all of them)
  std::vector<double> cost(nq);
  for (int i = 0; i < nq; ++i)
    cost[i] = (o.real_self_conjugate && partner[qs[i]] == qs[i]) ? 0.6 : 1.0;
  const std::vector<std::vector<int>> parts = assign_q(cost, NR);
  std::vector<int> my_qs;
  std::vector<double> my_wt;
  for (int i : parts[RK]) my_qs.push_back(qs[i]), my_wt.push_back(wt[i]);
  const int nmine = (int)my_qs.size();
  void *Wq, *Ws, *W0;
  std::vector<int> ranks(nmine, 0);
  int used = 0, ncod = 0;
  long row0 = 0, row1 = nip;
  // the streamed y is this build's y when the selection gave the cap's points under time
  // reversal (the q-list it was formed for) and the y stream met no stalled wait
  const bool y_streamed = tr && ystream_valid(c, nip, qs.data(), nq);
  // a discarded streamed y: its stream joins before its buffer goes back (the usual build may be
  // handed the same memory)
  if (c->ys.enqueued && !y_streamed) FISDF_TRY(ystream_join(c));
  if (yT_pre && !y_streamed) {
    FISDF_TRY(build_return(c, yT_pre));
    yT_pre = nullptr;
  }
  FISDF_CHECK(!x4_side || y_streamed, "build: x4 on the side stream without the streamed y");
  if (!comm) {
    // the factorisation (replaces zgelsy's QRCP, :108) on the side stream, overlapped with y
    FISDF_TRY(fisdf_factor_x4_mark(c));
    if (x4_side) {  // X gathered (ev_x4) -> x4 -> the factor chain, all on the side stream
      FISDF_HIP(hipStreamWaitEvent(c->side, c->ev_x4, 0));
      FISDF_TRY(build_x4_on(c, c->side, &c->ws_x4, X, nip, nao, kmesh, a, x4));  // :38-48
    }
    void* yT = yT_pre;
    if (!yT) FISDF_TRY(build_alloc(c, BR_Y, sizeof(cplx) * (size_t)nq * nip * ngrid, &yT));
    // the self-conjugate q's y real (half their y writes and FFT reads); FISDF_Y_REAL=0: off
    struct YRealScope {  // the mode is this build's only: reset on every exit
      fisdf_ctx* c;
      ~YRealScope() { c->y_real_store = false; c->y_real_slot.clear(); }
    } y_real_scope{c};
    c->y_real_store = y_real_env && o.real_self_conjugate && fft3d_reads_real(mesh[0], mesh[1], mesh[2]);
    if (y_streamed) {
      // the fit comes after the y stream; joined only now, after x4 has been marked for the
      // factor chain, so the side stream does not wait for y
      FISDF_TRY(ystream_join(c));
      // what fisdf_build_y_qs records for the fit: the slots stored real
      c->y_real_slot.assign(nq, 0);
      for (int i = 0; i < nq; ++i) c->y_real_slot[i] = (c->ys.rmask >> qs[i]) & 1ull ? 1 : 0;
    } else {
      FISDF_TRY(fisdf_build_y_qs(c, f, ngrid * nao, 0, (int)ngrid, (int)ngrid, X, nip, nao, kmesh,
                                 a, qs.data(), nq, yT));                           // :67-87
    }
    FISDF_TRY(fisdf_factor_x4_async(c, x4, qs.data(), nq, nip, o.fit_tol,
                                    o.real_self_conjugate ? kmesh : nullptr));
    FISDF_TRY(build_alloc(c, BR_WQ, sizeof(cplx) * (size_t)nq * nn, &Wq));
    // the fit waits for the factor's verdict itself
    FISDF_TRY(fisdf_fit_coulomb_qs(c, qs.data(), nq, yT, nip, mesh, kmesh, a, Wq)); // :97-121
    host_mark("fit enqueued");
    FISDF_TRY(fisdf_factor_x4_wait(c, ranks.data()));
    host_mark("factor ranks read back");
    FISDF_TRY(fisdf_factor_info(c, &used));
    FISDF_TRY(fisdf_min_norm_info(c, &ncod));
    // a block that waited past its bound built y from unfinished pivots
    if (y_streamed) FISDF_TRY(ystream_check(c));
    // y is dead once the fit is enqueued: fit_coulomb_qs joined its lanes and FFT stream into
    // c->stream (aux_join, checked by build_return), so a stream-ordered free cannot overtake a
    // reader
    FISDF_TRY(build_return(c, yT));
    FISDF_TRY(build_alloc(c, BR_WS, sizeof(double) * (size_t)nk * nn, &Ws));
    FISDF_TRY(fisdf_build_ws_qs(c, Wq, qs.data(), wt.data(), nq, nip, kmesh, a, Ws)); // :204-207
    W0 = Wq;  // q = 0 is slot 0 (the smallest representative)
  } else {
    // y on this rank's plane-aligned grid slice for every fitted q (y_k = Phi^T (Phi fx_k)^2
    // mixes all k at each grid point, :79-84), then one all-to-all per local q hands every rank
    // its own q on the whole grid (kshard.exchange_y_chunked)
    std::vector<long> g0s(NR), ngs(NR);
    const long plane = (long)mesh[1] * mesh[2];
    for (int r = 0; r < NR; ++r) {
      long p0, p1;
      shard_range(mesh[0], r, NR, &p0, &p1);
      g0s[r] = p0 * plane;
      ngs[r] = (p1 - p0) * plane;
    }
    const long ngme = ngs[RK];
    if (nmine) FISDF_TRY(fisdf_factor_x4_mark(c));
    void *send, *recv;
    FISDF_TRY(build_alloc(c, BR_SEND, sizeof(cplx) * (size_t)nq * nip * std::max(ngme, 1L), &send));
    if (ngme)
      FISDF_TRY(fisdf_build_y_qs(c, (const cplx*)f + g0s[RK] * nao, ngrid * nao, 0, (int)ngme,
                                 (int)ngme, X, nip, nao, kmesh, a, qs.data(), nq, send));
    if (nmine)
      FISDF_TRY(fisdf_factor_x4_async(c, x4, my_qs.data(), nmine, nip, o.fit_tol,
                                      o.real_self_conjugate ? kmesh : nullptr));
    FISDF_TRY(build_alloc(c, BR_Y, sizeof(cplx) * (size_t)std::max(nmine, 1) * nip * ngrid, &recv));
    // the exchange runs on its own stream while this rank factorises and fits its earlier q
    if (!c->comm_stream) {
      FISDF_HIP(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
      FISDF_HIP(hipEventCreateWithFlags(&c->ev_comm, hipEventDisableTiming));
    }
    FISDF_HIP(hipEventRecord(c->ev_comm, c->stream));
    FISDF_HIP(hipStreamWaitEvent(c->comm_stream, c->ev_comm, 0));
    size_t nmax = 0;
    for (const auto& p : parts) nmax = std::max(nmax, p.size());
    std::vector<const void*> sp(NR);
    std::vector<void*> rp(NR);
    std::vector<size_t> sb(NR), rb(NR);
    for (size_t j = 0; j < nmax; ++j) {
      const bool mine = j < (size_t)nmine;
      cplx* rj = (cplx*)recv + (long)j * nip * ngrid;
      for (int r = 0; r < NR; ++r) {
        const bool to_r = j < parts[r].size();
        sp[r] = to_r ? (const cplx*)send + (long)parts[r][j] * nip * ngme : nullptr;
        sb[r] = to_r ? sizeof(cplx) * (size_t)nip * ngme : 0;
        // piece j = concat over ranks p of the (nip, ng_p) blocks: p's block at nip * g0_p
        rp[r] = mine ? rj + (long)nip * g0s[r] : nullptr;
        rb[r] = mine ? sizeof(cplx) * (size_t)nip * ngs[r] : 0;
      }
      FISDF_TRY(comm_check(comm->all_to_all(comm->user, sp.data(), sb.data(), rp.data(), rb.data(),
                                            c->comm_stream), "all_to_all"));
      if (mine)
        FISDF_TRY(set_y_slices_on(c, (int)j, rj, NR, g0s.data(), ngs.data(), c->comm_stream));
    }
    FISDF_HIP(hipEventRecord(c->ev_comm, c->comm_stream));
    FISDF_TRY(build_alloc(c, BR_WQ, sizeof(cplx) * (size_t)std::max(nmine, 1) * nn, &Wq));
    if (nmine) {
      // one call over the whole shard: its lanes start each q when that q's piece has landed
      FISDF_TRY(fisdf_fit_coulomb_qs(c, my_qs.data(), nmine, nullptr, nip, mesh, kmesh, a, Wq));
      FISDF_TRY(fisdf_factor_x4_wait(c, ranks.data()));
      FISDF_TRY(fisdf_factor_info(c, &used));
      FISDF_TRY(fisdf_min_norm_info(c, &ncod));
    }
    // the send and receive buffers stay the build's until the exchange is done
    FISDF_HIP(hipStreamWaitEvent(c->stream, c->ev_comm, 0));
    FISDF_TRY(build_return(c, recv));
    FISDF_TRY(build_return(c, send));
    // W_s = sqrt(nk) Re(sum_q Phi[R,q] W_q) (:204-207) mixes every rank's q: each rank forms every
    // rank's interpolation-point row block of its partial sum, reduce-scattered by rows
    std::vector<int> bounds(NR + 1);
    long rmax = 0;
    for (int r = 0; r < NR; ++r) {
      long lo, hi;
      shard_range(nip, r, NR, &lo, &hi);
      bounds[r] = (int)lo;
      bounds[r + 1] = (int)hi;
      rmax = std::max(rmax, hi - lo);
      if (r == RK) row0 = lo, row1 = hi;
    }
    const long chunk = (long)nk * std::max(rmax, 1L) * nip;
    void* Wsb;
    FISDF_TRY(build_alloc(c, BR_WSB, sizeof(double) * (size_t)chunk * NR, &Wsb));
    FISDF_HIP(hipMemsetAsync(Wsb, 0, sizeof(double) * (size_t)chunk * NR, c->stream));
    FISDF_TRY(fisdf_build_ws_blocks(c, Wq, my_qs.data(), my_wt.data(), nmine, nip, kmesh, a, NR,
                                    bounds.data(), chunk, Wsb));
    FISDF_TRY(build_alloc(c, BR_WS, sizeof(double) * (size_t)chunk, &Ws));
    FISDF_TRY(comm_check(comm->reduce_scatter_f64(comm->user, (const double*)Wsb, (double*)Ws,
                                                  (size_t)chunk, c->stream), "reduce_scatter_f64"));
    FISDF_TRY(build_return(c, Wsb));
    // W_0 for get_j (:159) from the rank fitting q = 0 (position 0 of the fit order, its slot 0)
    int owner0 = 0;
    for (int r = 0; r < NR; ++r)
      if (!parts[r].empty() && parts[r][0] == 0) owner0 = r;
    FISDF_TRY(build_alloc(c, BR_W0, sizeof(cplx) * (size_t)nn, &W0));
    if (RK == owner0)
      FISDF_HIP(hipMemcpyAsync(W0, Wq, sizeof(cplx) * nn, hipMemcpyDeviceToDevice, c->stream));
    FISDF_TRY(comm_check(comm->broadcast(comm->user, W0, sizeof(cplx) * nn, owner0, c->stream),
                         "broadcast"));
  }
  B.valid = true;
  B.nk = nk;
  B.nip = nip;
  B.nao = nao;
  B.ng0 = ng0;
  B.nfit = nmine;
  B.used_pivoted = used;
  B.min_norm = ncod;
  B.time_reversal = tr ? 1 : 0;
  B.tr_deviation = tr_dev;
  for (int i = 0; i < 3; ++i) B.kmesh[i] = kmesh[i], B.mesh[i] = mesh[i];
  for (int i = 0; i < 9; ++i) B.a[i] = a[i];
  B.perm = perm;
  B.fit_qs = my_qs;
  B.partner = partner;
  B.ranks = ranks;
  B.wt = my_wt;
  B.X = X;
  B.x4 = x4;
  B.Wq = Wq;
  B.Ws = Ws;
  B.W0 = W0;
  B.sharded = comm != nullptr;
  B.y_streamed = y_streamed;
  if (comm) B.comm = *comm;
  B.shard_rank = RK;
  B.shard_size = NR;
  B.row0 = (int)row0;
  B.row1 = (int)row1;
  if (h_nip) *h_nip = nip;
  host_mark("build return");
  return 0;
}

}  // namespace

extern "C" {

int fisdf_build(fisdf_ctx* c, const void* x0, int ng0, const void* f, int nao, const int kmesh[3],
                const int mesh[3], const double a[9], const fisdf_build_opts* opts, int* h_nip) {
  FISDF_TRY(device_guard(c));
  return build_impl(c, nullptr, x0, ng0, f, nao, kmesh, mesh, a, opts, h_nip);
}

int fisdf_build_sharded(fisdf_ctx* c, const fisdf_comm* comm, const void* x0, int ng0,
                        const void* f, int nao, const int kmesh[3], const int mesh[3],
                        const double a[9], const fisdf_build_opts* opts, int* h_nip) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(comm != nullptr, "build_sharded: comm is null (fisdf_build is the 1-GPU build)");
  return build_impl(c, comm, x0, ng0, f, nao, kmesh, mesh, a, opts, h_nip);
}

int fisdf_y_stream_arm(fisdf_ctx* c, const void* x0, int ng0, const void* f, long f_kstride,
                       int m, int nao, int nip_max, const int kmesh[3], const int* h_qs, int nq,
                       void* yT, int* h_armed) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(kmesh && h_armed && ng0 > 0 && nao > 0, "y_stream_arm: bad arguments");
  FISDF_TRY(check_qlist(h_qs, nq, kmesh[0] * kmesh[1] * kmesh[2], "y_stream_arm"));
  FISDF_CHECK(c->ys.enqueued == false, "y_stream_arm: the previous streamed y is not finished");
  bool armed = false;
  if (c->time_reversal)  // the fused kernel folds fx over k <= -k
    FISDF_TRY(ystream_arm(c, x0, ng0, f, f_kstride, m, nao, nip_max, kmesh, h_qs, nq, yT, 0,
                          &armed));
  *h_armed = armed ? 1 : 0;
  return 0;
}

int fisdf_y_stream_finish(fisdf_ctx* c, int nip, int* h_streamed) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(h_streamed, "y_stream_finish: null output");
  const bool ok = c->ys.enqueued && ystream_valid(c, nip, c->ys.qs.data(), (int)c->ys.qs.size());
  const bool had = c->ys.enqueued;
  FISDF_TRY(ystream_join(c));
  if (had) FISDF_TRY(ystream_check(c));
  *h_streamed = ok ? 1 : 0;
  c->ys = fisdf_ctx::YStream();
  return 0;
}

int fisdf_build_y_streamed(fisdf_ctx* c, int* h_streamed) {
  FISDF_TRY(ctx_guard(c));
  FISDF_CHECK(h_streamed, "build_y_streamed: null output");
  *h_streamed = c->bld.valid && c->bld.y_streamed ? 1 : 0;
  return 0;
}

int fisdf_build_get(fisdf_ctx* c, fisdf_build_result* out) {
  FISDF_TRY(ctx_guard(c));
  FISDF_CHECK(out != nullptr, "build_get: out is null");
  const fisdf_ctx::Build& B = c->bld;
  FISDF_CHECK(B.valid, "build_get: no build (call fisdf_build first)");
  out->nk = B.nk;
  out->nip = B.nip;
  out->nao = B.nao;
  out->nfit = B.nfit;
  out->used_pivoted_fit = B.used_pivoted;
  out->min_norm_slots = B.min_norm;
  out->perm = B.perm.data();
  out->fit_qs = B.fit_qs.data();
  out->ranks = B.ranks.data();
  out->partner = B.partner.data();
  out->d_X = B.X;
  out->d_x4 = B.x4;
  out->d_Wq = B.Wq;
  out->d_Ws = B.Ws;
  out->time_reversal = B.time_reversal;
  out->tr_deviation = B.tr_deviation;
  out->shard_rank = B.shard_rank;
  out->shard_size = B.shard_size;
  out->row0 = B.row0;
  out->row1 = B.row1;
  out->d_W0 = B.W0;
  return 0;
}

int fisdf_get_x(fisdf_ctx* c, void* h_x) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(c->bld.valid && h_x, "get_x: no build or null output");
  const auto& B = c->bld;
  return fisdf_memcpy_dtoh(c, h_x, B.X, sizeof(cplx) * (size_t)B.nk * B.nip * B.nao);
}

int fisdf_get_w0(fisdf_ctx* c, void* h_w0) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(c->bld.valid && h_w0, "get_w0: no build or null output");
  const auto& B = c->bld;  // q = 0 is always fitted (slot 0: the smallest representative)
  return fisdf_memcpy_dtoh(c, h_w0, B.W0, sizeof(cplx) * (size_t)B.nip * B.nip);
}

int fisdf_get_wq(fisdf_ctx* c, void* h_wq) {
  FISDF_TRY(device_guard(c));
  FISDF_CHECK(c->bld.valid && h_wq, "get_wq: no build or null output");
  const auto& B = c->bld;
  FISDF_CHECK(B.shard_size == 1, "get_wq: the W_q of a sharded build are distributed over the "
                                 "ranks (fisdf_build_get: this rank's fit_qs and d_Wq)");
  const size_t nn = (size_t)B.nip * B.nip;
  cplx* h = (cplx*)h_wq;
  std::vector<int> slot(B.nk, -1);
  for (int i = 0; i < B.nfit; ++i) slot[B.fit_qs[i]] = i;
  for (int i = 0; i < B.nfit; ++i)
    FISDF_HIP(hipMemcpyAsync(h + (size_t)B.fit_qs[i] * nn, (const cplx*)B.Wq + i * nn,
                             sizeof(cplx) * nn, hipMemcpyDeviceToHost, c->stream));
  FISDF_HIP(hipStreamSynchronize(c->stream));
  for (int q = 0; q < B.nk; ++q) {  // W_{-q} = conj(W_q) (x4_s, y_s real: fftisdf.py:43,81)
    if (slot[q] >= 0) continue;
    const int p = B.partner[q];
    FISDF_CHECK(p >= 0 && p < B.nk && slot[p] >= 0, "get_wq: q neither fitted nor a partner");
    for (size_t e = 0; e < nn; ++e) h[(size_t)q * nn + e] = cconj(h[(size_t)p * nn + e]);
  }
  return 0;
}

// fftisdf.py:390-408: K (get_k_kpts, :173-228) enqueued before J (get_j_kpts, :133-171)
int fisdf_get_jk(fisdf_ctx* c, const void* dms, int nset, int with_j, int with_k, void* vj, void* vk) {
  FISDF_TRY(device_guard(c));
  const auto& B = c->bld;
  FISDF_CHECK(B.valid, "get_jk: no build (call fisdf_build first)");
  FISDF_CHECK(dms && nset > 0, "get_jk: no density matrices");
  FISDF_CHECK((!with_j || vj) && (!with_k || vk), "get_jk: missing output");
  if (!B.sharded) {
    if (with_k)
      FISDF_TRY(fisdf_get_k_rows(c, B.X, B.Ws, dms, nset, B.nip, B.nao, B.kmesh, B.a, 0, B.nip, vk));
    if (with_j)
      FISDF_TRY(fisdf_get_j_rows(c, B.X, B.W0, dms, nset, B.nk, B.nip, B.nao, 0, B.nip, vj));
    return 0;
  }
  // sharded: this rank's interpolation-point rows (its W_s rows), then the sums over the ranks
  // (fftisdf.py:166,225 contract over all points)
  const size_t nv = 2 * (size_t)nset * B.nk * B.nao * B.nao;
  if (with_k) {
    FISDF_TRY(fisdf_get_k_rows_local(c, B.X, B.Ws, dms, nset, B.nip, B.nao, B.kmesh, B.a, B.row0,
                                     B.row1, vk));
    FISDF_TRY(comm_check(B.comm.allreduce_f64(B.comm.user, (double*)vk, nv, c->stream),
                         "allreduce_f64"));
  }
  if (with_j) {
    FISDF_TRY(fisdf_get_j_rows(c, B.X, B.W0, dms, nset, B.nk, B.nip, B.nao, B.row0, B.row1, vj));
    FISDF_TRY(comm_check(B.comm.allreduce_f64(B.comm.user, (double*)vj, nv, c->stream),
                         "allreduce_f64"));
  }
  return 0;
}

}  // extern "C"
