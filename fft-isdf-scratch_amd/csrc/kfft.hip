// Exact FFT-grid exchange (PySCF fft_jk.get_k_kpts restated) in both forms: the dm form, nao
// transform rows per row m, and the occupied-orbital (low-rank) form, D[s][k2] = A B^H with r_s
// columns, the orbitals of all sets stacked into I = sum_s r_s transform rows per row m.  The
// kernels around the transforms of the pair densities — the pair builder, which turns the [g][m]
// AO layout into grid-contiguous transform rows, and the two contractions of the transformed rows
// back to nao x nao: exx_contract_kernel gives every set all of Z, exx_contract_lr_kernel is
// segmented, every transformed row meeting the u of the one set that owns it — with the host
// arithmetic of their launchers (kfft_plan).  Deterministic: no atomics, partial sums are combined
// in a fixed order, and a row m's sums do not depend on the chunk it is in.
#include "common.h"
#include "linalg.h"

#include <algorithm>

namespace fisdf {

namespace {

// the fftfreq fraction of index i on an axis of n points
__device__ __forceinline__ double kfft_freq(int i, int n) {
  return (double)(i < (n + 1) / 2 ? i : i - n) / (double)n;
}

// ---- P[(m - m0) ni + i][g] = conj(f1[g,m]) psi[g,i], m in [m0, m1) -----------------------------
// psi has ni columns at leading dimension ld, f1 its nao (the dm form: psi = f2, ni = ld = nao).
// Workgroup (grid tile of kKfftGT points, i-tile, m-tile): the points' psi columns of the i-tile
// (TW wide) and f1 columns of the m-tile (TW / 2 wide, at least 8) are read as runs of contiguous
// columns per point and staged in LDS at a pitch odd in 16-byte units, so that the lanes of a
// wave — consecutive grid points of one column — meet no bank twice; wave j then writes the
// rows (m, i), i = j + 4 t, of the tile, each a run of 64 consecutive grid points.
template <int TW>
__global__ __launch_bounds__(256) void pair_density_kernel(const cplx* __restrict__ f1, int nao,
                                                           const cplx* __restrict__ psi, int ni,
                                                           long ld, int ngrid, int m0, int m1,
                                                           cplx* __restrict__ P) {
  constexpr int MW = TW >= 16 ? TW / 2 : TW;
  constexpr int PL = TW | 1, PM = MW | 1;
  __shared__ cplx sl[kKfftGT * PL];
  __shared__ cplx sm[kKfftGT * PM];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long g0 = (long)blockIdx.x * kKfftGT;
  const int rows = (int)min((long)kKfftGT, ngrid - g0);
  const int it0 = blockIdx.y * TW, ic = min(TW, ni - it0);
  const int mt0 = m0 + blockIdx.z * MW, mcn = min(MW, m1 - mt0);
  for (int e = tid; e < kKfftGT * TW; e += 256) {
    const int g = e / TW, c = e - g * TW;
    sl[g * PL + c] = g < rows && c < ic ? psi[(g0 + g) * ld + it0 + c] : cmk(0, 0);
  }
  for (int e = tid; e < kKfftGT * MW; e += 256) {
    const int g = e / MW, c = e - g * MW;
    sm[g * PM + c] = g < rows && c < mcn ? f1[(g0 + g) * nao + mt0 + c] : cmk(0, 0);
  }
  __syncthreads();
  if (lane >= rows) return;
  for (int mi = 0; mi < mcn; ++mi) {
    const cplx a = cconj(sm[lane * PM + mi]);
    cplx* row = P + ((long)(mt0 - m0 + mi) * ni + it0) * ngrid + g0 + lane;
    for (int ii = wv; ii < ic; ii += 4) row[(long)ii * ngrid] = cmul(a, sl[lane * PL + ii]);
  }
}

// too_many: the entry's message for a launch grid beyond 65535 tiles
template <int TW>
int pair_launch(hipStream_t st, const cplx* f1, int nao, const cplx* psi, int ni, long ld,
                int ngrid, int m0, int m1, cplx* P, const char* too_many) {
  constexpr int MW = TW >= 16 ? TW / 2 : TW;
  const long gt = ((long)ngrid + kKfftGT - 1) / kKfftGT;
  const int it = (ni + TW - 1) / TW, mt = (m1 - m0 + MW - 1) / MW;
  FISDF_CHECK(it <= 65535 && mt <= 65535, too_many);
  hipLaunchKernelGGL(pair_density_kernel<TW>, dim3((unsigned)gt, it, mt), dim3(256), 0, st, f1, nao,
                     psi, ni, ld, ngrid, m0, m1, P);
  FISDF_HIP(hipGetLastError());
  return 0;
}

// the arguments are the entry's to check
int pair_build(hipStream_t st, const cplx* f1, int nao, const cplx* psi, int ni, long ld, int ngrid,
               int m0, int m1, cplx* P, const char* too_many) {
  return pair_density_variant(ni) == 8
             ? pair_launch<8>(st, f1, nao, psi, ni, ld, ngrid, m0, m1, P, too_many)
             : pair_launch<32>(st, f1, nao, psi, ni, ld, ngrid, m0, m1, P, too_many);
}

// ---- the tail of both contractions -----------------------------------------------------------
// ts holds the t rows of one tile of kKfftGT points, row (s, m) at s MT + (m - mt0) with MT rows m
// per set.  Thread (orow, on) of the 8 x 32 output tile owns the Q rows orow + 8 q of ts and one
// column of each of the NN n-tiles: acc[t][q] += ts[orow + 8 q][g] f1[g, n] over the tile's points,
// g ascending, f1's 32 columns staged per n-tile in fs.  The dm form has MT = 8, so q is the set.
template <int NN, int Q>
__device__ __forceinline__ void exx_tile_add(const cplx (*ts)[kKfftGT], cplx (*fs)[kExxNT],
                                             const cplx* __restrict__ f1, int nao, int nbase,
                                             long g0, long gend, int tid, cplx (&acc)[NN][Q]) {
  const int orow = tid >> 5, on = tid & 31;
#pragma unroll
  for (int t = 0; t < NN; ++t) {
    const int nt0 = nbase + t * kExxNT;
    if (nt0 < nao) {  // uniform over the workgroup
      __syncthreads();  // ts written (t = 0) / the previous n-tile's readers of fs are done
      for (int e = tid; e < kKfftGT * kExxNT; e += 256) {
        const int gg = e / kExxNT, c = e - gg * kExxNT;
        fs[gg][c] = g0 + gg < gend && nt0 + c < nao ? f1[(g0 + gg) * nao + nt0 + c] : cmk(0, 0);
      }
      __syncthreads();
#pragma unroll 4
      for (int gg = 0; gg < kKfftGT; ++gg) {
        const cplx b = fs[gg][on];
#pragma unroll
        for (int q = 0; q < Q; ++q) cfma(acc[t][q], ts[orow + 8 * q][gg], b);
      }
    }
  }
}

// part[run][s][m - m0][n] = acc of the thread's rows (s, m) and columns n
template <int NN, int Q, int MT>
__device__ __forceinline__ void exx_tile_store(const cplx (&acc)[NN][Q], int run, int mt0, int m0,
                                               int m1, int nao, int nbase, int tid,
                                               cplx* __restrict__ part) {
  constexpr int SC = 8 * Q / MT;  // sets of the launch
  const int orow = tid >> 5, on = tid & 31, mc = m1 - m0;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int r = orow + 8 * q, s = r / MT, m = mt0 + r % MT;
    if (m < m1) {
#pragma unroll
      for (int t = 0; t < NN; ++t) {
        const int n = nbase + t * kExxNT + on;
        if (n < nao) part[(((long)run * SC + s) * mc + (m - m0)) * nao + n] = acc[t][q];
      }
    }
  }
}

// ---- part[run][s][m - m0][n] = sum_{g in run} t_s[m,g] f1[g,n],
//      t_s[m,g] = conj(em[g]) sum_l conj(Z[(m - m0) nao + l][g]) u_s[l][g] ------------------------
// Workgroup (run, m-tile of kExxMT rows).  Per tile of kKfftGT grid points: lane g of wave j forms
// t_s for the rows m = j and j + 4 of the m-tile, l ascending — every Z element is read from HBM
// once, a run of 64 consecutive points per wave, and meets the SC sets' u in registers — and
// leaves them in LDS; then thread (m, n) of the 8 x 32 output tile adds t_s[m, g] f1[g, n] over
// the tile's points, g ascending, for each of the NN n-tiles (f1's 32 columns staged per n-tile).
// NN kExxNT columns are one column group; nao beyond 4 n-tiles takes further groups as
// blockIdx.z of the NN = 4 instantiation, each of which forms t_s again (Z is then read once per
// group).
// conj(em[g]) = exp(+i sum_d frac_d(g) kd_d) comes from the point's mesh indices (fft3d's
// separable phase, conjugated).
template <int SC, int NN>
__global__ __launch_bounds__(256) void exx_contract_kernel(
    const cplx* __restrict__ Z, const cplx* __restrict__ u, const cplx* __restrict__ f1, int ngrid,
    int nao, int n1, int n2, int n0, double kd0, double kd1, double kd2, int use_phase, int m0,
    int m1, int run_len, cplx* __restrict__ part) {
  __shared__ cplx ts[SC * kExxMT][kKfftGT];
  __shared__ cplx fs[kKfftGT][kExxNT];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int run = blockIdx.x;
  const int mt0 = m0 + blockIdx.y * kExxMT;
  const int nbase = blockIdx.z * NN * kExxNT;  // this workgroup's column group
  const long gbeg = (long)run * run_len, gend = min((long)ngrid, gbeg + run_len);
  const long uset = (long)nao * ngrid;
  cplx acc[NN][SC];
#pragma unroll
  for (int t = 0; t < NN; ++t)
#pragma unroll
    for (int s = 0; s < SC; ++s) acc[t][s] = cmk(0, 0);

  for (long g0 = gbeg; g0 < gend; g0 += kKfftGT) {
    const long g = g0 + lane;
    const bool in = g < gend;
    // rows wv and wv + 4 of the m-tile (a row past m1 reads row wv, its sums are dropped)
    const int ma = mt0 + wv, mb = mt0 + wv + 4;
    const bool va = ma < m1, vb = mb < m1;
    cplx ta[SC], tb[SC];
#pragma unroll
    for (int s = 0; s < SC; ++s) ta[s] = tb[s] = cmk(0, 0);
    if (in && va) {
      const cplx* za = Z + (long)(ma - m0) * nao * ngrid + g;
      const cplx* zb = Z + (long)((vb ? mb : ma) - m0) * nao * ngrid + g;
      const cplx* ug = u + g;
#pragma unroll 2
      for (int l = 0; l < nao; ++l) {
        const cplx a = za[(long)l * ngrid], b = zb[(long)l * ngrid];
#pragma unroll
        for (int s = 0; s < SC; ++s) {
          const cplx w = ug[s * uset + (long)l * ngrid];
          cfma_conj(ta[s], a, w);
          cfma_conj(tb[s], b, w);
        }
      }
      if (use_phase) {
        const int i2 = (int)(g % n2), i1 = (int)((g / n2) % n1), i0 = (int)(g / ((long)n1 * n2));
        const double th =
            kfft_freq(i0, n0) * kd0 + kfft_freq(i1, n1) * kd1 + kfft_freq(i2, n2) * kd2;
        double sn, cs;
        sincos(th, &sn, &cs);
        const cplx ph = cmk(cs, sn);
#pragma unroll
        for (int s = 0; s < SC; ++s) {
          ta[s] = cmul(ph, ta[s]);
          tb[s] = cmul(ph, tb[s]);
        }
      }
    }
    __syncthreads();  // the previous tile's readers of ts are done
#pragma unroll
    for (int s = 0; s < SC; ++s) {
      ts[s * kExxMT + wv][lane] = ta[s];
      ts[s * kExxMT + wv + 4][lane] = vb && in ? tb[s] : cmk(0, 0);
    }
    exx_tile_add<NN, SC>(ts, fs, f1, nao, nbase, g0, gend, tid, acc);
  }
  exx_tile_store<NN, SC, kExxMT>(acc, run, mt0, m0, m1, nao, nbase, tid, part);
}

// the segments of the sets of one launch: set s owns the rows i in [o[s], o[s + 1])
struct LrSegs {
  int o[kLrSetChunk + 1];
};

// ---- part[run][s][m - m0][n] = sum_{g in run} t_s[m,g] f1[g,n],
//      t_s[m,g] = conj(em[g]) sum_{i in segment s} conj(Z[(m - m0) ni + i][g]) u[i][g] -----------
// Workgroup (run, m-tile of MT = kLrRows / SC rows m, column group): the kLrRows = 32 rows (s, m)
// of ts take the LDS that exx_contract_kernel gives to 4 sets x 8 rows, so one set has 32 rows m
// per workgroup and f1 is read nao / 32 times where the dm form reads it nao / 8 times — with
// ni rows per m the read of Z is nao ni ngrid elements, and at small ni the re-read of f1 would
// otherwise be as large.  Per tile of kKfftGT grid points: lane g of wave j forms t_s for the
// rows m = j + 4 q of the m-tile, q < MT / 4, i ascending over the segment — u[i][g] is loaded
// once for the MT / 4 rows, and every Z element is read once, by the one set whose segment holds
// its row — multiplies by conj(em[g]) and leaves them in LDS; then thread (r, n) of the 8 x 32
// output tile adds ts[r + 8 q][g] f1[g, n], q < 4, over the tile's points, g ascending, for each
// of the NN n-tiles (f1's 32 columns staged per n-tile).  Column groups as in the dm form.
template <int SC, int NN>
__global__ __launch_bounds__(256) void exx_contract_lr_kernel(
    const cplx* __restrict__ Z, const cplx* __restrict__ u, const cplx* __restrict__ f1, int ngrid,
    int nao, int ni, LrSegs seg, int n1, int n2, int n0, double kd0, double kd1, double kd2,
    int use_phase, int m0, int m1, int run_len, cplx* __restrict__ part) {
  constexpr int MT = kLrRows / SC;  // rows m per workgroup
  constexpr int JR = MT / 4;        // rows m per wave and set
  constexpr int QR = kLrRows / 8;   // rows (s, m) per thread of the output tile
  __shared__ cplx ts[kLrRows][kKfftGT];
  __shared__ cplx fs[kKfftGT][kExxNT];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int run = blockIdx.x;
  const int mt0 = m0 + blockIdx.y * MT;
  const int nbase = blockIdx.z * NN * kExxNT;  // this workgroup's column group
  const long gbeg = (long)run * run_len, gend = min((long)ngrid, gbeg + run_len);
  cplx acc[NN][QR];
#pragma unroll
  for (int t = 0; t < NN; ++t)
#pragma unroll
    for (int q = 0; q < QR; ++q) acc[t][q] = cmk(0, 0);

  for (long g0 = gbeg; g0 < gend; g0 += kKfftGT) {
    const long g = g0 + lane;
    const bool in = g < gend;
    cplx ph = cmk(1, 0);
    if (use_phase && in) {
      const int i2 = (int)(g % n2), i1 = (int)((g / n2) % n1), i0 = (int)(g / ((long)n1 * n2));
      const double th =
          kfft_freq(i0, n0) * kd0 + kfft_freq(i1, n1) * kd1 + kfft_freq(i2, n2) * kd2;
      double sn, cs;
      sincos(th, &sn, &cs);
      ph = cmk(cs, sn);
    }
    __syncthreads();  // the previous tile's readers of ts are done
#pragma unroll
    for (int s = 0; s < SC; ++s) {
      cplx t[JR];
      const cplx* zr[JR];
#pragma unroll
      for (int q = 0; q < JR; ++q) {
        t[q] = cmk(0, 0);
        // a row past m1 reads the tile's first row, its sums are dropped
        const int m = mt0 + wv + 4 * q;
        zr[q] = Z + (long)((m < m1 ? m : mt0) - m0) * ni * ngrid + g;
      }
      if (in) {
        for (int i = seg.o[s]; i < seg.o[s + 1]; ++i) {
          const cplx w = u[(long)i * ngrid + g];
#pragma unroll
          for (int q = 0; q < JR; ++q) cfma_conj(t[q], zr[q][(long)i * ngrid], w);
        }
      }
#pragma unroll
      for (int q = 0; q < JR; ++q) {
        const bool v = in && mt0 + wv + 4 * q < m1;
        ts[s * MT + wv + 4 * q][lane] = v ? (use_phase ? cmul(ph, t[q]) : t[q]) : cmk(0, 0);
      }
    }
    exx_tile_add<NN, QR>(ts, fs, f1, nao, nbase, g0, gend, tid, acc);
  }
  exx_tile_store<NN, QR, MT>(acc, run, mt0, m0, m1, nao, nbase, tid, part);
}

// vk[s][m][n] (+)= scale (part[0] + part[1] + ...), m in [m0, m1): the runs in order
__global__ void exx_reduce_kernel(const cplx* __restrict__ part, int nrun, int sc, int mc, int nao,
                                  int m0, double scale, int accumulate, cplx* __restrict__ vk,
                                  long vk_set) {
  const long n = (long)sc * mc * nao;
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (e >= n) return;
  cplx r = part[e];
  for (int q = 1; q < nrun; ++q) r = cadd(r, part[(long)q * n + e]);
  const int s = (int)(e / ((long)mc * nao));
  const long mn = e - (long)s * mc * nao;
  cplx* o = vk + s * vk_set + (long)m0 * nao + mn;
  const cplx v = cscale(r, scale);
  *o = accumulate ? cadd(*o, v) : v;
}

// the sc sets of one contraction launch, from its partial blocks into vk (vk at the first of them)
int exx_reduce(hipStream_t st, const cplx* part, int nrun, int sc, int mc, int nao, int m0,
               double scale, int accumulate, cplx* vk, long vk_set) {
  const long n = (long)sc * mc * nao;
  hipLaunchKernelGGL(exx_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part,
                     nrun, sc, mc, nao, m0, scale, accumulate, vk, vk_set);
  FISDF_HIP(hipGetLastError());
  return 0;
}

template <int SC, int NN>
int exx_launch(hipStream_t st, const cplx* Z, const cplx* u, const cplx* f1, int ngrid, int nao,
               const int mesh[3], const double* kd, int m0, int m1, int run_len, int nrun,
               cplx* part) {
  const int mt = (m1 - m0 + kExxMT - 1) / kExxMT;
  const int ng = (nao + NN * kExxNT - 1) / (NN * kExxNT);  // column groups (1 unless nao > 128)
  FISDF_CHECK(mt <= 65535 && ng <= 65535, "exx_contract: too many tiles");
  hipLaunchKernelGGL((exx_contract_kernel<SC, NN>), dim3(nrun, mt, ng), dim3(256), 0, st, Z, u, f1,
                     ngrid, nao, mesh[1], mesh[2], mesh[0], kd ? kd[0] : 0.0, kd ? kd[1] : 0.0,
                     kd ? kd[2] : 0.0, kd ? 1 : 0, m0, m1, run_len, part);
  FISDF_HIP(hipGetLastError());
  return 0;
}

template <int SC, int NN>
int exx_lr_launch(hipStream_t st, const cplx* Z, const cplx* u, const cplx* f1, int ngrid, int nao,
                  int ni, const LrSegs& seg, const int mesh[3], const double* kd, int m0, int m1,
                  int run_len, int nrun, cplx* part) {
  constexpr int MT = kLrRows / SC;
  const int mt = (m1 - m0 + MT - 1) / MT;
  const int ng = (nao + NN * kExxNT - 1) / (NN * kExxNT);  // column groups (1 unless nao > 128)
  FISDF_CHECK(mt <= 65535 && ng <= 65535, "exx_contract_lr: too many tiles");
  hipLaunchKernelGGL((exx_contract_lr_kernel<SC, NN>), dim3(nrun, mt, ng), dim3(256), 0, st, Z, u,
                     f1, ngrid, nao, ni, seg, mesh[1], mesh[2], mesh[0], kd ? kd[0] : 0.0,
                     kd ? kd[1] : 0.0, kd ? kd[2] : 0.0, kd ? 1 : 0, m0, m1, run_len, part);
  FISDF_HIP(hipGetLastError());
  return 0;
}

}  // namespace

int pair_density_variant(int ni) { return ni <= 8 ? 8 : 32; }

int exx_contract_variant(int nao) {
  const int nt = (nao + kExxNT - 1) / kExxNT;
  return nt <= 1 ? 1 : nt <= 2 ? 2 : 4;
}

void exx_grid_split(int ngrid, int nao, int nset, int* run_len, int* nrun) {
  (void)nao;
  (void)nset;
  const long tiles = ((long)ngrid + kKfftGT - 1) / kKfftGT;
  const long want = std::min(tiles, kExxRuns);
  const long per = (tiles + want - 1) / want;
  *run_len = (int)(per * kKfftGT);
  *nrun = (int)(((long)ngrid + *run_len - 1) / *run_len);
}

long exx_contract_work_elems(int ngrid, int nao, int nset, int mc, int set_chunk) {
  int run_len, nrun;
  exx_grid_split(ngrid, nao, nset, &run_len, &nrun);
  return (long)nrun * std::min(nset, set_chunk) * mc * nao;
}

void kfft_plan(int nao, long ngrid, int nset, int rows, bool lowrank, long work_bytes,
               KfftPlan* p) {
  *p = KfftPlan();
  // the size limits keep every product below inside a long
  if (nao < 1 || nao > kKfftMaxNao || ngrid < 1 || ngrid >= (1L << 31) || nset < 1 ||
      nset > kKfftMaxSets || rows < 1 || rows > kKfftMaxNao || work_bytes < 0)
    return;
  const int set_chunk = lowrank ? kLrSetChunk : kJfftSetChunk;
  p->row_bytes = (long)sizeof(cplx) * rows * ngrid;  // the transform rows of one row m
  const long budget = work_bytes ? work_bytes : kKfftWorkBytes;
  p->pair_tw = pair_density_variant(rows);
  p->exx_sc = std::min(nset, set_chunk);
  p->exx_nn = exx_contract_variant(nao);
  exx_grid_split((int)ngrid, nao, nset, &p->run_len, &p->nrun);
  p->mc = (int)std::min<long>(nao, budget / p->row_bytes);  // mc <= nao
  if (p->mc < 1) return;
  p->nchunk = (nao + p->mc - 1) / p->mc;
  auto al = [](long b) { return (b + 255) / 256 * 256; };
  p->off_rows = 0;
  p->off_psi = p->off_rows + al(p->row_bytes * p->mc);
  // the dm form has no psi (the pair builder reads f2) and every set's u over the nao rows
  p->off_u = p->off_psi + (lowrank ? al(p->row_bytes) : 0);
  p->off_w = p->off_u + al(lowrank ? p->row_bytes : nset * p->row_bytes);
  p->off_part = p->off_w + al((long)sizeof(double) * ngrid);
  p->part_elems = exx_contract_work_elems((int)ngrid, nao, nset, p->mc, set_chunk);
  p->bytes = p->off_part + al((long)sizeof(cplx) * p->part_elems);
  p->ok = 1;
}

int pair_density(hipStream_t st, const cplx* f1, const cplx* f2, int ngrid, int nao, int m0, int m1,
                 cplx* P) {
  FISDF_CHECK(f1 && f2 && P, "pair_density: null pointer");
  FISDF_CHECK(ngrid >= 1 && nao >= 1, "pair_density: sizes must be >= 1");
  FISDF_CHECK(0 <= m0 && m0 < m1 && m1 <= nao, "pair_density: bad row range");
  return pair_build(st, f1, nao, f2, nao, nao, ngrid, m0, m1, P,
                    "pair_density: too many AO tiles");
}

int pair_density_lr(hipStream_t st, const cplx* f1, int nao, const cplx* psi, int ni, long ld,
                    int ngrid, int m0, int m1, cplx* P) {
  FISDF_CHECK(f1 && psi && P, "pair_density_lr: null pointer");
  FISDF_CHECK(ngrid >= 1 && nao >= 1 && ni >= 1, "pair_density_lr: sizes must be >= 1");
  FISDF_CHECK(ld >= ni, "pair_density_lr: ld_psi below ni");
  FISDF_CHECK(0 <= m0 && m0 < m1 && m1 <= nao, "pair_density_lr: bad row range");
  return pair_build(st, f1, nao, psi, ni, ld, ngrid, m0, m1, P, "pair_density_lr: too many tiles");
}

int exx_contract(hipStream_t st, const cplx* Z, const cplx* u, const cplx* f1, const int mesh[3],
                 const double* kd, int m0, int m1, int nao, int nset, double scale, int accumulate,
                 cplx* vk, long vk_set, cplx* work, long work_elems) {
  FISDF_CHECK(Z && u && f1 && vk && work && mesh, "exx_contract: null pointer");
  FISDF_CHECK(mesh[0] >= 1 && mesh[1] >= 1 && mesh[2] >= 1, "exx_contract: bad mesh");
  const long ngl = (long)mesh[0] * mesh[1] * mesh[2];
  FISDF_CHECK(ngl < (1L << 31), "exx_contract: mesh too large");
  FISDF_CHECK(nao >= 1 && nset >= 1, "exx_contract: sizes must be >= 1");
  FISDF_CHECK(0 <= m0 && m0 < m1 && m1 <= nao, "exx_contract: bad row range");
  const int nn = exx_contract_variant(nao);
  const int ngrid = (int)ngl, mc = m1 - m0;
  FISDF_CHECK(work_elems >= exx_contract_work_elems(ngrid, nao, nset, mc, kJfftSetChunk),
              "exx_contract: workspace too small");
  int run_len, nrun;
  exx_grid_split(ngrid, nao, nset, &run_len, &nrun);
  // at most kJfftSetChunk sets per pass over Z
  for (int s0 = 0; s0 < nset; s0 += kJfftSetChunk) {
    const int sc = std::min(kJfftSetChunk, nset - s0);
    const cplx* uc = u + (long)s0 * nao * ngrid;
    int rc = -1;
#define FISDF_EXX(SC, NN)       \
  if (sc == SC && nn == NN)     \
    rc = exx_launch<SC, NN>(st, Z, uc, f1, ngrid, nao, mesh, kd, m0, m1, run_len, nrun, work);
#define FISDF_EXX_N(SC) FISDF_EXX(SC, 1) FISDF_EXX(SC, 2) FISDF_EXX(SC, 4)
    FISDF_EXX_N(1) FISDF_EXX_N(2) FISDF_EXX_N(3) FISDF_EXX_N(4)
#undef FISDF_EXX_N
#undef FISDF_EXX
    FISDF_TRY(rc);
    FISDF_TRY(exx_reduce(st, work, nrun, sc, mc, nao, m0, scale, accumulate, vk + s0 * vk_set,
                         vk_set));
  }
  return 0;
}

int exx_contract_lr(hipStream_t st, const cplx* Z, const cplx* u, const cplx* f1, const int mesh[3],
                    const double* kd, int m0, int m1, int nao, int ni, const int* seg, int nset,
                    double scale, int accumulate, cplx* vk, long vk_set, cplx* work,
                    long work_elems) {
  FISDF_CHECK(Z && u && f1 && vk && work && mesh && seg, "exx_contract_lr: null pointer");
  FISDF_CHECK(mesh[0] >= 1 && mesh[1] >= 1 && mesh[2] >= 1, "exx_contract_lr: bad mesh");
  const long ngl = (long)mesh[0] * mesh[1] * mesh[2];
  FISDF_CHECK(ngl < (1L << 31), "exx_contract_lr: mesh too large");
  FISDF_CHECK(nao >= 1 && nset >= 1 && ni >= 1, "exx_contract_lr: sizes must be >= 1");
  FISDF_CHECK(0 <= m0 && m0 < m1 && m1 <= nao, "exx_contract_lr: bad row range");
  FISDF_CHECK(seg[0] == 0 && seg[nset] == ni, "exx_contract_lr: segments must cover [0, ni)");
  for (int s = 0; s < nset; ++s)
    FISDF_CHECK(seg[s] <= seg[s + 1], "exx_contract_lr: segment offsets must not decrease");
  const int nn = exx_contract_variant(nao);
  const int ngrid = (int)ngl, mc = m1 - m0;
  FISDF_CHECK(work_elems >= exx_contract_work_elems(ngrid, nao, nset, mc, kLrSetChunk),
              "exx_contract_lr: workspace too small");
  int run_len, nrun;
  exx_grid_split(ngrid, nao, nset, &run_len, &nrun);
  // at most kLrSetChunk sets per launch; the launches read disjoint rows of Z
  for (int s0 = 0; s0 < nset; s0 += kLrSetChunk) {
    const int sc = std::min(kLrSetChunk, nset - s0);
    LrSegs sg;
    for (int s = 0; s <= kLrSetChunk; ++s) sg.o[s] = seg[s0 + std::min(s, sc)];
    int rc = -1;
#define FISDF_EXX_LR(SC, NN)                                                                  \
  if (sc == SC && nn == NN)                                                                   \
    rc = exx_lr_launch<SC, NN>(st, Z, u, f1, ngrid, nao, ni, sg, mesh, kd, m0, m1, run_len, \
                               nrun, work);
#define FISDF_EXX_LR_N(SC) FISDF_EXX_LR(SC, 1) FISDF_EXX_LR(SC, 2) FISDF_EXX_LR(SC, 4)
    FISDF_EXX_LR_N(1) FISDF_EXX_LR_N(2)
#undef FISDF_EXX_LR_N
#undef FISDF_EXX_LR
    FISDF_TRY(rc);
    FISDF_TRY(exx_reduce(st, work, nrun, sc, mc, nao, m0, scale, accumulate, vk + s0 * vk_set,
                         vk_set));
  }
  return 0;
}

}  // namespace fisdf
