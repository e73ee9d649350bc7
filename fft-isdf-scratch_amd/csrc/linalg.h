#pragma once
#include "common.h"

#include <vector>

struct fisdf_pp_atom;  // include/fisdf.h

namespace fisdf {

struct CellGeom {
  double a[3][3];  // lattice vectors (rows), bohr
  double b[3][3];  // reciprocal vectors (rows), 2*pi*inv(a)^T
};

int gather_lp(hipStream_t s, const cplx* L, int n, int rmax, const int* piv, const int* rank,
              int rpad, cplx* Lp, int batch);
int trinv_blocks(hipStream_t s, const cplx* Lp, int r, int ldl, long sL, int nb, long sLi,
                 cplx* Linv, int batch);
int build_trsm_q(hipStream_t s, const cplx* Lp, int r, long sL, cplx* Q, int batch, int mode);
int trsm_merged_batched(hipStream_t s, const cplx* Q, long sQ, int r, cplx* X, long ld, long sX,
                        int ncol, int batch, bool lower_rhs = false, cplx* work = nullptr,
                        long work_elems = 0);
// split-K of one block row of trsm_merged_batched (from its shape only) and the workspace
// (complex elements) that lets a batch of `batch` r x r matrices run in one launch per row
int trsm_split_k(int nc, int b1);
long trsm_split_work_elems(int r, int batch);
// the partition of trsm_merged_batched (the partial block first) and what it does per block row
struct TrsmRow {
  int b0, m, b1;  // rows [b0, b0 + m), K = b1 = b0 + m
  int nc;         // columns computed
  int ks;         // split-K
  int sub;        // matrices per launch (sub-batches when the workspace is short)
};
int trsm_merged_blocks(int r);
bool trsm_merged_row(int r, int ncol, int batch, bool lower_rhs, bool have_work, long work_elems,
                     int b, TrsmRow* row);
int set_identity(hipStream_t s, cplx* X, int n, int batch);
// out[g][j*nao + m] = h_sc[j] * x0[h_k[j]][g][m] for the nsel listed k (any nsel)
int permute_kgm_sel(hipStream_t s, const cplx* x0, const int* h_k, const double* h_sc, int nsel,
                    int ng, int nao, cplx* out);
// time-reversal check of Bloch AO values a[k][row][nao] (k stride ks elements, get_kpts order) on
// every rstride-th row: atomically maxes mon[0] with max |a[-k] - conj(a[k])| and mon[1] with
// max |a[k]| (double bits)
int tr_check(hipStream_t s, const cplx* a, long ks, long rows, int nao, long rstride,
             const int kmesh[3], unsigned long long* mon);
// the time-reversal representatives k <= -k (ascending) and whether each is self-paired
void kmesh_reps(const int kmesh[3], std::vector<int>* reps, std::vector<char>* self);
int trsm_blocked(hipStream_t s, int lower, const cplx* Lp, long ldl, long sL, int r,
                 const cplx* Linv, long sLi, int nb, cplx* B, long ldb, long sB, cplx* X, long ldx,
                 long sX, int ncol, int batch, int a_real = 0);
// G indices whose Coulomb weight differs from that of G' = -G - m.b (ascending) -> idx, *count
int asym_list(hipStream_t s, const double* w, const int mesh[3], const int m[3], int* idx,
              int* count);
int gather_cols(hipStream_t s, const cplx* A, long ld, int r, const int* idx, int n, cplx* out);
// self-conjugate q on half the G: the prefix planes i0 < nH hold one member of every Hermitian
// pair G' = -G - m.b (both members on a self-paired plane); half_weight: w = sqrt of the pair's
// combined weight (c = coulG*scale, not rooted) on the prefix, 0 beyond; asym_half: the prefix G
// of unequal pair weights with f = (c - c')/(c + c') (1 on a self-paired plane), ascending
int half_prefix_planes(int n0, int m0);
int half_weight(hipStream_t s, double* w, const double* c, const int mesh[3], const int m[3]);
int asym_half(hipStream_t s, const double* c, const int mesh[3], const int m[3], int* idx,
              double* f, int* count);
int gather_cols_scaled(hipStream_t s, const cplx* A, long ld, int r, const int* idx,
                       const double* f, int n, cplx* out);
int add_imag(hipStream_t s, cplx* G, int ldg, const cplx* H, int ldh, int n);
// zero the imaginary parts of n complex elements
int zero_imag(hipStream_t s, cplx* a, long n);
// x4s[i] = x4all[qr[i]] (imag zeroed where qr[nq + i] != 0), also into L if not null
int stage_x4(hipStream_t s, const cplx* x4all, const int* qr, int nq, long nn, cplx* x4s, cplx* L);
// Minimum-norm operator of a rank-deficient x4_q from its rank-revealing pivoted Cholesky
// x4[P,P] ~ L L^H (L: rows of f_L, row order; piv: the pivot order; r = rank): A = P L (n x r),
// thin QR A = Q R by shifted CholeskyQR3, M = A^+ = R^{-1} Q^H (r x n, ld ldm; columns in pivot
// order) so that z[P] = M^H M y[P] is the minimum-norm solution (gelsy's complete orthogonal
// step).  Completes piv[r..n) with the rows outside the first r pivots (ascending).
// q_out (n x r) / rinv_out (r x r), if given, receive Q and R^{-1}.  work: min_norm_work_bytes(n, r); fail: 3 device ints (Cholesky breakdown per pass).
int min_norm_operator(hipStream_t s, const cplx* L, int n, int rmax, int* piv, int r,
                      cplx* M, long ldm, void* work, int* fail, cplx* q_out = nullptr,
                      cplx* rinv_out = nullptr);
size_t min_norm_work_bytes(int n, int r);
int scatter_w(hipStream_t s, const cplx* Wpp, int ldw, long sW, int rmax, const int* piv,
              const int* rank, cplx* W, int nip, int batch);
int conj_transpose(hipStream_t s, const cplx* A, int n, long sA, cplx* B, int batch);
int coulg_weight(hipStream_t s, const int mesh[3], const CellGeom& g, const double k[3],
                 double scale, int take_sqrt, double* w, double omega = 0.0);
int square_real(hipStream_t s, const cplx* in, cplx* out, long n, unsigned long long* maximag);
int csquare(hipStream_t s, cplx* a, long n, unsigned long long* maximag);
int rho_diag(hipStream_t s, const cplx* T, const cplx* X, int nset, int nk, int nip, int nao,
             double scale, cplx* rho);
int scale_rows(hipStream_t s, const cplx* X, const cplx* v, int nset, int nk, int nip, int i0,
               int nb, int nao, cplx* Xv);
int gather_points(hipStream_t s, const cplx* x0, int nk, int ng0, int nao, const int* perm,
                  int nip, cplx* X);
int square_scale(hipStream_t s, const cplx* in, double sc, cplx* out, long n);
int permute_kgm(hipStream_t s, const cplx* x0, int nq, int ng, int nao, cplx* out);
int pair_product(hipStream_t s, const cplx* A, int n1, const cplx* B, int n2, int nip, cplx* P);
// y_q = Phi^T (Re(Phi FX))^2 for the ascending q-list (h_qs on the host; d_qs a device copy,
// needed only when the k-mesh has more than 64 points), written to yT[slot][I][goff + g].
// half: FX holds only the kmesh_half_count(kmesh) representatives k <= -k (ascending k, 36 of
// 64 at 4x4x4); the others are conj(FX[-k]) (time reversal).  kmesh_rep_runs: the
// representatives as [begin, end) runs of consecutive k (pairs appended to runs)
int kmesh_half_count(const int kmesh[3]);
// Fused y build (time reversal, register k-meshes): fx_k = X_k f_k^H on MFMA for the
// representative k, staged per 16 x 16 (I, g) tile in LDS, then the kmesh_y DFTs — no fx in
// HBM.  X (nk, nip, nao); F = f + g0*nao with k stride fks (g rows of nao); writes
// yT[slot][I][goff + g] for g < m.  *handled = false (nothing enqueued) for other k-meshes
// or nk > 64 (the two-kernel path then runs).
// workspace bytes of y_fused for this shape (0: the fused kernel does not apply)
size_t y_fused_workspace(const int kmesh[3], int nip, int nao, int m);
// rmask: q (bits) stored real, as doubles in the first half of their slot (self-conjugate q)
int y_fused(hipStream_t s, const cplx* X, int nip, int nao, const cplx* F, long fks, int m,
            const int kmesh[3], const int* h_qs, int nq, cplx* yT, long qs, long Is, long goff,
            unsigned long long* mon, cplx* work, size_t work_bytes, unsigned long long rmask,
            bool* handled);
// whether the fused kernel covers this k-mesh (time reversal assumed)
bool y_fused_applies(const int kmesh[3], int nao);
// The same y build streamed behind a running selection (api.hip build_impl): rows [0, nip) of
// y in blocks of `rows` (a multiple of 16); block [lo, hi) forms its XT rows straight from x0
// through piv[lo..hi) once the selection's progress word (device) reaches hi, then runs the
// fused kernel on its I-tiles.  X is never read; work holds XT (nip rows) and FT as for
// y_fused.  *err (device) is set if a block waited past the bound.  *handled as for y_fused.
int y_fused_stream(hipStream_t s, const cplx* x0, int ng0, int nao, const int* piv,
                   const int* progress, int* err, int nip, int rows, const cplx* F, long fks,
                   int m, const int kmesh[3], const int* h_qs, int nq, cplx* yT, long qs, long Is,
                   long goff, cplx* work, size_t work_bytes, unsigned long long rmask,
                   bool* handled, hipStream_t s2 = nullptr, hipEvent_t ev_a = nullptr,
                   hipEvent_t ev_b = nullptr);
int kmesh_rep_runs(const int kmesh[3], std::vector<int>* runs);
// Bloch AO values (ao.hip): F (nimg, ng, nao) f64 workspace, scratch for the small tables;
// nkb > 0: at the nkb band k-points h_kband (any k) instead of the k-mesh, F (nT, ng, nao)
int eval_ao(hipStream_t s, const double* d_coords, int ng, int natm, const double* h_atoms, int nsh,
            const int* h_sh_atom, const int* h_sh_l, const int* h_sh_nprim, const double* h_exps,
            const double* h_coefs, int nT, const int* h_tn, const int kmesh[3], const double a[9],
            double rcut, double* F, void* scratch, size_t scratch_size, cplx* chi, int* h_nao,
            int nkb = 0, const double* h_kband = nullptr, int deriv = 0);
// conj_out: store conj(y_q) — the x4 build's Phi^H x4_s (fftisdf.py:46; x4_s real) where the y
// build has Phi^T y_s (:84)
int kmesh_y(hipStream_t s, const cplx* FX, long ncol, const int kmesh[3], const int* h_qs,
            const int* d_qs, int nq, int m, cplx* yT, long qs, long Is, long goff, bool half,
            unsigned long long* mon, bool conj_out = false);
// the k-meshes with compile-time instantiations of the register kernels (kmesh_y_reg_kernel,
// y_fused_kernel, k_wsrho_reg_kernel, bloch_dft_reg_kernel): the one list every dispatch expands
#define FISDF_KM_REG_MESHES(X)                                                                 \
  X(1, 1, 1) X(1, 1, 2) X(2, 2, 2) X(3, 3, 1) X(3, 3, 3) X(4, 4, 4) X(2, 2, 1) X(1, 2, 2)       \
  X(4, 4, 1) X(2, 2, 4)
// Which kernel a separable k-mesh transform over ncol columns runs; kmesh_y(),
// kmesh_y_reg_applies(), k_wsrho_reg() and bloch_dft() branch on it.  KM_REG: a listed k-mesh
// (at most 64 points) and ncol < 2^31.  KM_LDS: kmesh_y_kernel on tiles of CT columns (64, halved
// down to 8 until the nk x (CT + 1) tile and the twiddles fit 64 KB) with `lds` bytes of dynamic
// LDS (the tile, the twiddles and the nk-entry source table).  KM_REFUSED: an axis outside 1..16,
// more than 160 KB of LDS, or 2^31 tiles; CT and lds are still those of the LDS rule when the
// axes are in range.
enum KmeshRoute { KM_REG = 0, KM_LDS = 1, KM_REFUSED = 2 };
struct KmeshPlan {
  int route;
  int CT;
  size_t lds;
};
KmeshPlan kmesh_route(const int kmesh[3], long ncol);
// 0 when some kmesh_route of this k-mesh runs, else the error a transform over it would raise
int kmesh_check(const int kmesh[3], const char* who);
// whether kmesh_y runs its register kernel for this k-mesh and column count (no device q-list)
bool kmesh_y_reg_applies(const int kmesh[3], long ncol);
// the fused kernel's plan for a k-mesh and nao: whether it applies, the k of its chunk A / chunk B
// slots in slot order, its dynamic LDS bytes and the K chunks (of 28) per slot
struct YFusedPlan {
  bool applies;
  int nA, nB;
  int kA[16], kB[32];
  size_t lds;
  int nkc;
};
void y_fused_plan(const int kmesh[3], int nao, YFusedPlan* out);
// chi[k][col] = sum_R exp(+2 pi i sum_a r_a k_a / n_a) F[R][col] over the k-mesh (the tail of
// eval_ao): the register kernel on a KM_REG route, else one thread per (k, column); *route (may
// be null) tells which.  bloch_band: chi[k][col] = sum_t ph[t][k] F[t][col] for nkb band k-points
int bloch_dft(hipStream_t s, const double* F, long ncol, const int kmesh[3], cplx* chi,
              int* route = nullptr);
int bloch_band(hipStream_t s, const double* F, long ncol, int nT, const cplx* ph, int nkb,
               cplx* chi);
// get_k's rho_s = Phi rho_k, V_s = W_s * Re(rho_s), V_k = Phi^T V_s in place on B (nk rows of
// ncol columns; W_s row s at Ws + s * ws_Rstride) for the register k-meshes; *handled = false
// (nothing enqueued) otherwise.  max |Im rho_s| into *mon
int k_wsrho_reg(hipStream_t s, cplx* B, long ncol, const int kmesh[3], const double* Ws,
                long ws_Rstride, unsigned long long* mon, bool* handled);

// ---- exact FFT-grid J (jfft.hip; PySCF fft_jk.get_j_kpts) ----
// both kernels take at most kJfftSetChunk sets per pass over f (one launch per chunk)
constexpr int kJfftSetChunk = 4;
// rho[s][g] = (1/nk) sum_k sum_mn f_k[g,m] D[s][k][m,n] conj(f_k[g,n]); f (nk, ngrid, nao) with k
// stride fks; no workspace.  rho_grid_tiled: D_sk is staged in 32 x 32 tiles (nao > 32)
int rho_grid(hipStream_t s, const cplx* f, long fks, int nk, int ngrid, int nao, const cplx* D,
             int nset, cplx* rho);
bool rho_grid_tiled(int nao);
// out[s][k][m][n] = scale sum_g conj(f_k[g,m]) v_s[g] f_k[g,n] (conj_v: conj(v_s[g])), the grid
// split into *nsplit runs of *chunk points (weighted_gram_split, from the shape only) whose
// partial blocks are summed in split order; work: weighted_gram_work_elems complex elements
constexpr long kGramWgs = 1024;
void weighted_gram_split(int nk, int ngrid, int nao, int* chunk, int* nsplit);
long weighted_gram_work_elems(int nk, int ngrid, int nao, int nset);
int weighted_gram(hipStream_t s, const cplx* f, long fks, int nk, int ngrid, int nao,
                  const cplx* v, int nset, int conj_v, double scale, cplx* out, cplx* work,
                  long work_elems);
// a[e] = conj(a[e]): ifft(x) = conj(fft(conj(x))) / N around the forward fft3d
int conj_inplace(hipStream_t s, cplx* a, long n);

// ---- GGA density and potential matrix over the four-component AO block (xc.hip) ---------------
// f4: component c of k-point k at f4 + k fks + c fcs, (ngrid, nao) each.
// rho[(s 4 + c) rcs + g]: c = 0 the density of rho_grid, c = 1..3 its gradient; hermi = 1 takes
// D Hermitian (gradient 2 Re(t conj d_c f), imaginary part exactly 0), hermi = 0 both terms.
// rho_gga_set_chunk sets per pass over f4 (4; 2 for hermi = 0 with D tiled, nao > 32); no workspace
int rho_grid_gga(hipStream_t s, const cplx* f4, long fks, long fcs, int nk, int ngrid, int nao,
                 const cplx* D, int nset, int hermi, cplx* rho, long rcs);
bool rho_gga_tiled(int nao);
int rho_gga_set_chunk(int nao, int hermi);
size_t rho_gga_lds_bytes(int nao, int sc, int hermi);
// out[s][k] (+)= scale (M + M^H), M = f_k^H aow_k, aow = 1/2 w_0 f + sum_c w_c d_c f; w real,
// w[s wss + c wcs + g].  Workspaces in complex elements from gga_gram_work (split: 0 = none)
void gga_gram_work(int nk, int ng, int nao, size_t* aow, size_t* m, size_t* split);
int gga_gram(hipStream_t s, const cplx* f4, long fks, long fcs, int nk, int ng, int nao,
             const double* w, long wss, long wcs, int nset, double scale, int accumulate, cplx* out,
             cplx* aow, cplx* M, cplx* split);

// ---- the functional at the grid points of a block (func.hip) -----------------------------------
// family 0 LDA (Slater + PW92), 1 GGA (PBE); rho[s rss + c rcs + g] complex, the real parts read;
// e[s ess + g], wv[s wss + c wcs + g] real, either may be null.  part (optional): xc_blocks(ng)
// pairs (sum n, sum e) per set, which xc_sums adds in a fixed order into sums[s][2].  xc_check
// is xc_eval's argument check alone (for callers that must refuse before their first launch)
int xc_blocks(int ng);
int xc_check(int family, double cx, double cc, double rho_cut, int ng, int nset, long rss, long rcs,
             long ess, long wss, long wcs, bool has_e, bool has_wv);
int xc_eval(hipStream_t s, int family, double cx, double cc, double rho_cut, const cplx* rho,
            long rss, long rcs, int ng, int nset, double* e, long ess, double* wv, long wss,
            long wcs, double* part);
int xc_sums(hipStream_t s, const double* part, int nblk, int nset, double scale, int accumulate,
            double* sums);

// ---- exact FFT-grid K (kfft.hip; PySCF fft_jk.get_k_kpts) in its two forms: the dm form, nao
// transform rows per row m, and the occupied-orbital (low-rank) form below ----
constexpr int kKfftGT = 64;        // grid points per tile of the kernels (one per lane)
constexpr int kExxMT = 8;          // rows m per workgroup of the contraction
constexpr int kExxNT = 32;         // output columns per n-tile of the contraction
constexpr long kExxRuns = 128;     // grid runs the contraction aims at
constexpr long kKfftWorkBytes = 1L << 29;  // default budget of the transform rows
constexpr int kKfftMaxNao = 1 << 15, kKfftMaxSets = 1 << 10;  // kfft_plan's arithmetic fits a long
// P[(m - m0) nao + l][g] = conj(f1[g,m]) f2[g,l] for m in [m0, m1): (m1 - m0) nao rows of ngrid,
// f1 and f2 (ngrid, nao): pair_density_lr with psi = f2, ni = ld = nao.  pair_density_variant: the
// tile width of the instantiation (8, 32) for ni rows per row m
int pair_density(hipStream_t s, const cplx* f1, const cplx* f2, int ngrid, int nao, int m0, int m1,
                 cplx* P);
int pair_density_variant(int ni);
// vk[s][m][n] (+)= scale sum_g t_s[m,g] f1[g,n] for m in [m0, m1), with
// t_s[m,g] = exp(+i frac(g).kd) sum_l conj(Z[(m - m0) nao + l][g]) u[s][l][g] (kd null: no phase;
// frac the fftfreq fractions of fft3d's phase); Z (m1 - m0) nao rows of ngrid, u (nset, nao,
// ngrid), vk set stride vk_set.  The grid is split into *nrun runs of *run_len points
// (exx_grid_split, from the shape only) whose partial blocks are summed in run order; at most
// kJfftSetChunk sets per pass over Z.  accumulate = 0 overwrites the rows.  work:
// exx_contract_work_elems complex elements (set_chunk: the sets per launch of the form, this one's
// kJfftSetChunk).  exx_contract_variant: the n-tiles per thread of the
// instantiation (1, 2, 4); nao > 128 runs the last once per group of 128 columns, each of which
// reads Z again
int exx_contract(hipStream_t s, const cplx* Z, const cplx* u, const cplx* f1, const int mesh[3],
                 const double* kd, int m0, int m1, int nao, int nset, double scale, int accumulate,
                 cplx* vk, long vk_set, cplx* work, long work_elems);
int exx_contract_variant(int nao);
void exx_grid_split(int ngrid, int nao, int nset, int* run_len, int* nrun);
long exx_contract_work_elems(int ngrid, int nao, int nset, int mc, int set_chunk);

// The occupied-orbital (low-rank) form: D[s][k2] = A B^H with r_s columns, the orbitals of all
// sets stacked, ni = sum_s r_s rows per row m where the dm form has nao, set s owning the segment
// [seg[s], seg[s + 1]).
constexpr int kLrRows = 32;     // rows (set, m) per workgroup of the segmented contraction
constexpr int kLrSetChunk = 2;  // sets per launch: 32 rows m per workgroup for one set, 16 for two
// P[(m - m0) ni + i][g] = conj(f1[g,m]) psi[g,i] for m in [m0, m1): f1 (ngrid, nao), psi (ngrid,
// ni) at leading dimension ld.  The tile width is pair_density_variant(ni)
int pair_density_lr(hipStream_t s, const cplx* f1, int nao, const cplx* psi, int ni, long ld,
                    int ngrid, int m0, int m1, cplx* P);
// vk[s][m][n] (+)= scale sum_g t_s[m,g] f1[g,n] for m in [m0, m1), with
// t_s[m,g] = exp(+i frac(g).kd) sum_{i in segment s} conj(Z[(m - m0) ni + i][g]) u[i][g]; Z
// (m1 - m0) ni rows of ngrid, u (ni, ngrid), seg nset + 1 host offsets from 0 to ni (an empty
// segment gives zeros).  Runs, reduction, accumulate and vk_set as exx_contract; at most
// kLrSetChunk sets per launch, each launch reading only its sets' rows of Z.  work:
// exx_contract_work_elems complex elements at set_chunk = kLrSetChunk.  The n-tiles per thread are
// exx_contract_variant's
int exx_contract_lr(hipStream_t s, const cplx* Z, const cplx* u, const cplx* f1, const int mesh[3],
                    const double* kd, int m0, int m1, int nao, int ni, const int* seg, int nset,
                    double scale, int accumulate, cplx* vk, long vk_set, cplx* work,
                    long work_elems);

// What fisdf_get_k_fft (rows = nao, lowrank = false) and fisdf_get_k_fft_lr (rows = imax, the
// largest ni of a k2, lowrank = true) do for given sizes and a byte budget for the transform rows
// (0: the default kKfftWorkBytes; never more than nao rows m): ok = 0 when the budget is below one
// row m (row_bytes = its `rows` transform rows; mc, nchunk and bytes are then 0) or a size is out
// of range (nao or rows > kKfftMaxNao, nset > kKfftMaxSets, ngrid >= 2^31).  mc rows m per chunk,
// nchunk chunks; exx_sc the most sets per contraction launch (the form's set chunk); the arena's
// layout (byte offsets) and total.  The dm form's u is (nset, nao, ngrid) and it has no psi (its
// slot is empty); the low-rank form's psi and u hold the orbitals on the grid, `rows` rows each.
struct KfftPlan {
  int ok = 0;
  int mc = 0, nchunk = 0;
  int run_len = 0, nrun = 0;
  int pair_tw = 0, exx_sc = 0, exx_nn = 0;
  long row_bytes = 0, part_elems = 0;
  long off_rows = 0, off_psi = 0, off_u = 0, off_w = 0, off_part = 0, bytes = 0;
};
void kfft_plan(int nao, long ngrid, int nset, int rows, bool lowrank, long work_bytes,
               KfftPlan* p);

// ---- exact FFT-grid four-index integrals (erifft.hip; PySCF FFTDF.get_eri / ao2mo): the exact K's
// pair densities and transform pair, then one GEMM of the transformed rows against B ----
constexpr int kPair34Cap = 8;          // pairs per launch of the B builder
constexpr int kEriMaxPairs = 65535;    // npair n3 stays inside an int
// B[(p n3 + k - r0) n4 + l][g] = exp(+i frac(g).kd) conj(a3_p[g,k]) a4_p[g,l] for the rows (p, k)
// in [r0, r1) of the npair n3 (kd null: no phase; frac the fftfreq fractions of fft3d's phase);
// a3, a4 host arrays of npair device pointers, (ngrid, n3) and (ngrid, n4) at leading dimensions
// ld3, ld4.  At most kPair34Cap pairs per launch; the tile width is pair_density_variant(n4)
int pair34(hipStream_t s, const cplx* const* a3, const cplx* const* a4, int npair, int n3, int n4,
           long ld3, long ld4, const int mesh[3], const double* kd, int r0, int r1, cplx* B);
// the split-K of the driver's GEMMs: the selection Gram's rule (select_gram_ksplit) with the tiles
// of the whole n1 n2 x n3 n4 problem, so that it depends on neither the budget nor npair
int eri_gemm_ksplit(long n12, long n34, long ngrid);
// What fisdf_get_eri_fft does for given sizes and a byte budget W (0: kKfftWorkBytes) that holds
// for the transform rows and for B each: mc = min(n1, W / (16 n2 ngrid)) rows i per chunk,
// bc = min(npair n3, W / (16 n4 ngrid)) rows (p, k) per B chunk; ok = 0 when either is below 1 or
// a size is out of range (mc = bc = bytes = 0 then).  b_once: B is one chunk, built before the row
// loop; otherwise it is rebuilt inside each row chunk.  The arena's layout (byte offsets) and
// total; work_elems the split-K workspace of the largest GEMM (0 at ksplit 1).
struct EriFftPlan {
  int ok = 0;
  int mc = 0, nrow_chunks = 0, bc = 0, nb_chunks = 0, b_once = 0;
  int tw = 0, ksplit = 0;
  long work_elems = 0;
  long off_rows = 0, off_b = 0, off_w = 0, off_work = 0, bytes = 0;
};
void eri_fft_plan(int n1, int n2, int n3, int n4, int npair, long ngrid, long work_bytes,
                  EriFftPlan* p);

// ---- GTH pseudopotential matrices (pp.hip; PySCF FFTDF.get_pp / get_nuc): the local part's V_G,
// the separable projectors of one k-point, their overlaps with the Bloch AOs, c^H h c ----
constexpr int kPpGT = 64;        // grid points per step of the overlap kernel
constexpr int kPpMT = 32;        // AO columns per workgroup of the overlap
constexpr int kPpPT = 16;        // projector rows per workgroup of the overlap (two per thread)
constexpr long kPpRuns = 256;    // grid runs the overlap aims at
constexpr int kPpVlocCols = 9;   // doubles per atom of the local table: R, Z, rloc, c1..c4
// One (atom, l) channel of the table: its n (2 l + 1) projector rows start at row0 of the rows
// in hand (a chunk of whole atoms), row = row0 + i (2 l + 1) + mm
struct PpBlock {
  double R[3], rl;
  double h[9];
  int l, n, row0, pad;
};
// the table's checks (nl <= 4, n[l] <= 3, nexp <= 4, counts >= 0, rloc and the r_l read > 0) as an
// error naming `who`; pp_rows: the projector rows of atoms [a0, a1) of a checked table
int pp_check_table(const fisdf_pp_atom* atoms, int natm, const char* who);
long pp_rows(const fisdf_pp_atom* atoms, int a0, int a1);
// the host tables: kPpVlocCols doubles per atom (a bare nucleus: rloc = 0, c = 0, for which the
// pseudopotential's formulas give -4 pi Z / G^2 and 0 at G = 0); the channels of atoms [a0, a1)
void pp_vloc_table(const fisdf_pp_atom* atoms, int natm, std::vector<double>* tab);
void pp_blocks(const fisdf_pp_atom* atoms, int a0, int a1, std::vector<PpBlock>* blocks);
// out[G] = scale V_G (conj_out: conjugated) over the mesh; tab: device, pp_vloc_table's
int vloc_g(hipStream_t s, const int mesh[3], const CellGeom& g, const double* tab, int natm,
           double scale, int conj_out, cplx* out);
// rows[row][G] = conj(beta_row(G; k)) for the channels blocks[0..nblocks) (device)
int gth_projectors(hipStream_t s, const int mesh[3], const CellGeom& g, const double k[3],
                   const PpBlock* blocks, int nblocks, cplx* rows);
// c[p][m] = scale sum_g t[p][g] exp(-i frac(g).kd) f[g][m] (kd null: no phase); the grid in
// *nrun runs of *run_len points (pp_overlap_split, from ngrid alone) whose partial blocks are
// summed in run order; part: nrun np nao complex elements
void pp_overlap_split(long ngrid, int* run_len, int* nrun);
int pp_overlap(hipStream_t s, const cplx* t, int np, const cplx* f, int nao, const int mesh[3],
               const double* kd, double scale, cplx* c, cplx* part);
// out[m][n] += sum over the channels, mm, i, j of conj(c[(i, mm)][m]) h[i][j] c[(j, mm)][n], the
// terms added to out's value one by one in table order (so the result does not depend on how the
// channels are spread over calls)
int pp_vnl(hipStream_t s, const cplx* c, int nao, const PpBlock* blocks, int nblocks, cplx* out);
// What fisdf_get_pp does for given sizes and a byte budget for one k-point's projector rows (0:
// kKfftWorkBytes): chunks of whole atoms [chunk_a[i], chunk_a[i + 1]) of at most chunk_rows rows;
// ok = 0 when an atom's own rows exceed the budget or a size is out of range.  The arena's layout
// (byte offsets) and total.
struct PpPlan {
  int ok = 0;
  int run_len = 0, nrun = 0, mtiles = 0;
  int nproj = 0, nchunk = 0, chunk_rows = 0, max_blocks = 0;
  std::vector<int> chunk_a;
  long gram_elems = 0;
  long off_v = 0, off_gram = 0, off_rows = 0, off_part = 0, off_c = 0, off_tab = 0, off_blk = 0;
  long bytes = 0;
};
void pp_plan(int nao, long ngrid, int nk, const fisdf_pp_atom* atoms, int natm, int with_nonlocal,
             long work_bytes, PpPlan* p);

}  // namespace fisdf
