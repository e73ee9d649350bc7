// Exact FFT-grid exchange in the occupied-orbital (low-rank) form: D[s][k2] = A B^H with r_s
// columns, the orbitals of all sets stacked into I = sum_s r_s transform rows per row m (kfft.hip
// is the dm form, nao rows per row m).  The pair builder against the orbitals on the grid, the
// segmented contraction — every transformed row meets the u of the one set that owns it — and the
// host arithmetic of their launchers (kfft_lr_plan).  Deterministic: no atomics, partial sums are
// combined in a fixed order, and a row m's sums do not depend on the chunk it is in.
#include "common.h"
#include "linalg.h"

#include <algorithm>

namespace fisdf {

namespace {

// the complex FMAs and the mesh fraction of kfft.hip, restated (that file is kept as it is)
__device__ __forceinline__ void cfma(cplx& acc, cplx a, cplx b) {
  acc.x = fma(a.x, b.x, acc.x);
  acc.x = fma(-a.y, b.y, acc.x);
  acc.y = fma(a.x, b.y, acc.y);
  acc.y = fma(a.y, b.x, acc.y);
}

// acc += conj(a) b
__device__ __forceinline__ void cfma_conj(cplx& acc, cplx a, cplx b) {
  acc.x = fma(a.x, b.x, acc.x);
  acc.x = fma(a.y, b.y, acc.x);
  acc.y = fma(a.x, b.y, acc.y);
  acc.y = fma(-a.y, b.x, acc.y);
}

__device__ __forceinline__ double lr_freq(int i, int n) {
  return (double)(i < (n + 1) / 2 ? i : i - n) / (double)n;
}

// ---- P[(m - m0) ni + i][g] = conj(f1[g,m]) psi[g,i], m in [m0, m1) -----------------------------
// pair_density_kernel's staging with the tile of the second operand over the ni orbitals: psi has
// ni columns at leading dimension ld, f1 its nao.  Workgroup (grid tile of kKfftGT points, i-tile
// of TW, m-tile of MW); both operands are staged in LDS at a pitch odd in 16-byte units; wave j
// writes the rows (m, i), i = j + 4 t, of the tile, each a run of 64 consecutive grid points.
template <int TW>
__global__ __launch_bounds__(256) void pair_density_lr_kernel(const cplx* __restrict__ f1, int nao,
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

template <int TW>
int pair_lr_launch(hipStream_t st, const cplx* f1, int nao, const cplx* psi, int ni, long ld,
                   int ngrid, int m0, int m1, cplx* P) {
  constexpr int MW = TW >= 16 ? TW / 2 : TW;
  const long gt = ((long)ngrid + kKfftGT - 1) / kKfftGT;
  const int it = (ni + TW - 1) / TW, mt = (m1 - m0 + MW - 1) / MW;
  FISDF_CHECK(it <= 65535 && mt <= 65535, "pair_density_lr: too many tiles");
  hipLaunchKernelGGL(pair_density_lr_kernel<TW>, dim3((unsigned)gt, it, mt), dim3(256), 0, st, f1,
                     nao, psi, ni, ld, ngrid, m0, m1, P);
  FISDF_HIP(hipGetLastError());
  return 0;
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
  const int orow = tid >> 5, on = tid & 31;  // this thread's rows orow + 8 q and column
  const int run = blockIdx.x;
  const int mt0 = m0 + blockIdx.y * MT;
  const int nbase = blockIdx.z * NN * kExxNT;  // this workgroup's column group
  const int mc = m1 - m0;
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
      const double th = lr_freq(i0, n0) * kd0 + lr_freq(i1, n1) * kd1 + lr_freq(i2, n2) * kd2;
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
          for (int q = 0; q < QR; ++q) cfma(acc[t][q], ts[orow + 8 * q][gg], b);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < QR; ++q) {
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

// vk[s][m][n] (+)= scale (part[0] + part[1] + ...), m in [m0, m1): the runs in order;
// kfft.hip's exx_reduce_kernel restated (that file is kept as it is)
__global__ void exx_reduce_lr_kernel(const cplx* __restrict__ part, int nrun, int sc, int mc,
                                     int nao, int m0, double scale, int accumulate,
                                     cplx* __restrict__ vk, long vk_set) {
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

int pair_density_lr_variant(int ni) { return ni <= 8 ? 8 : 32; }

long exx_contract_lr_work_elems(int ngrid, int nao, int nset, int mc) {
  int run_len, nrun;
  exx_grid_split(ngrid, nao, nset, &run_len, &nrun);
  return (long)nrun * std::min(nset, kLrSetChunk) * mc * nao;
}

void kfft_lr_plan(int nao, long ngrid, int nset, int imax, long work_bytes, KfftLrPlan* p) {
  *p = KfftLrPlan();
  // the size limits keep every product below inside a long
  if (nao < 1 || nao > kKfftMaxNao || ngrid < 1 || ngrid >= (1L << 31) || nset < 1 ||
      nset > kKfftMaxSets || imax < 1 || imax > kKfftMaxNao || work_bytes < 0)
    return;
  p->row_bytes = (long)sizeof(cplx) * imax * ngrid;  // the imax transform rows of one row m
  const long budget = work_bytes ? work_bytes : kKfftWorkBytes;
  p->pair_tw = pair_density_lr_variant(imax);
  p->exx_sc = std::min(nset, kLrSetChunk);
  p->exx_nn = exx_contract_variant(nao);
  exx_grid_split((int)ngrid, nao, nset, &p->run_len, &p->nrun);
  p->mc = (int)std::min<long>(nao, budget / p->row_bytes);  // mc <= nao
  if (p->mc < 1) return;
  p->nchunk = (nao + p->mc - 1) / p->mc;
  auto al = [](long b) { return (b + 255) / 256 * 256; };
  p->off_rows = 0;
  p->off_psi = p->off_rows + al(p->row_bytes * p->mc);
  p->off_u = p->off_psi + al(p->row_bytes);
  p->off_w = p->off_u + al(p->row_bytes);
  p->off_part = p->off_w + al((long)sizeof(double) * ngrid);
  p->bytes = p->off_part +
             al((long)sizeof(cplx) * exx_contract_lr_work_elems((int)ngrid, nao, nset, p->mc));
  p->ok = 1;
}

int pair_density_lr(hipStream_t st, const cplx* f1, int nao, const cplx* psi, int ni, long ld,
                    int ngrid, int m0, int m1, cplx* P) {
  FISDF_CHECK(f1 && psi && P, "pair_density_lr: null pointer");
  FISDF_CHECK(ngrid >= 1 && nao >= 1 && ni >= 1, "pair_density_lr: sizes must be >= 1");
  FISDF_CHECK(ld >= ni, "pair_density_lr: ld_psi below ni");
  FISDF_CHECK(0 <= m0 && m0 < m1 && m1 <= nao, "pair_density_lr: bad row range");
  return pair_density_lr_variant(ni) == 8
             ? pair_lr_launch<8>(st, f1, nao, psi, ni, ld, ngrid, m0, m1, P)
             : pair_lr_launch<32>(st, f1, nao, psi, ni, ld, ngrid, m0, m1, P);
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
  FISDF_CHECK(work_elems >= exx_contract_lr_work_elems(ngrid, nao, nset, mc),
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
    const long n = (long)sc * mc * nao;
    hipLaunchKernelGGL(exx_reduce_lr_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                       work, nrun, sc, mc, nao, m0, scale, accumulate, vk + s0 * vk_set, vk_set);
    FISDF_HIP(hipGetLastError());
  }
  return 0;
}

}  // namespace fisdf
