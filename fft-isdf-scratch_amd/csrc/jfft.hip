// Exact FFT-grid J (PySCF fft_jk.get_j_kpts restated): the two kernels that stream the Bloch-AO
// array f[k][g][m] — the electron density on the FFT grid and the AO Gram weighted by a potential
// on the grid — and the elementwise conjugate that turns the forward fft3d into the inverse.
// Neither kernel forms a grid x nao temporary; both are deterministic (no floating-point atomics:
// partial sums are combined in a fixed order).
#include "common.h"
#include "linalg.h"

#include <algorithm>

namespace fisdf {

namespace {

// ---- rho[s][g] = (1/nk) sum_k sum_mn f_k[g,m] D_sk[m,n] conj(f_k[g,n]) ----------------------
// A workgroup of 256 threads owns PG * 64 grid points and loops over k.  Per k it stages the
// points' f rows (row pitch odd in 16-byte units: the rows are nao * 16 B apart, so lanes of
// consecutive points would otherwise meet on one bank) and D_sk of the set chunk in LDS.  Lane
// g of wave j forms t_s = sum_m f[g,m] D_s[m,n] for the columns n = j, j + 4, ... and adds
// t_s conj(f[g,n]); the four waves' sums are combined through LDS in wave order.
// nao <= kRhoNT: D_sk whole; one set takes PG = 2 points per lane, more sets PG = 1 (registers).
// Beyond it D is tiled kRhoNT x kRhoNT, the m-tile and the n-tile of f are staged side by side
// and PG = 1 (the n-tiles are read again per m-tile, by the same workgroup: cache hits).
// The (k, m-tile, n-tile) steps are software-pipelined: the next step's f and D elements are
// loaded into registers before the current step's arithmetic and stored to LDS after it.
constexpr int kRhoNT = 32;

template <int SC, int PG, bool TILED>
__global__ __launch_bounds__(256) void rho_grid_kernel(const cplx* __restrict__ f, long fks, int nk,
                                                       int ngrid, int nao,
                                                       const cplx* __restrict__ D, double inv_nk,
                                                       cplx* __restrict__ rho) {
  extern __shared__ cplx smem[];
  constexpr int PT = 64 * PG;
  constexpr int RF = PT * kRhoNT / 256;            // f elements per thread and tile
  constexpr int RD = SC * kRhoNT * kRhoNT / 256;   // D elements per thread and step
  constexpr int NB = PG * SC <= 2 ? 2 : 1;         // columns of D per pass over a tile's rows
  const int ntile = TILED ? (nao + kRhoNT - 1) / kRhoNT : 1;
  const int nta = TILED ? kRhoNT : nao;
  const int pitch = nta | 1;
  cplx* fm = smem;
  cplx* fn = TILED ? fm + PT * pitch : fm;
  cplx* Ds = fn + PT * pitch;
  const int tid = threadIdx.x, gl = tid & 63, j = tid >> 6;
  const long g0 = (long)blockIdx.x * PT;
  const int rows = (int)min((long)PT, ngrid - g0);  // grid points of this tile (the rest: zeros)
  const long dset = (long)nk * nao * nao;
  const int nsteps = nk * ntile * ntile;
  cplx acc[PG][SC];
#pragma unroll
  for (int p = 0; p < PG; ++p)
#pragma unroll
    for (int s = 0; s < SC; ++s) acc[p][s] = cmk(0, 0);
  cplx rm[RF], rn[RF], rd[RD];

  // step t = (k, mt, nt), nt fastest
  auto tile_of = [&](int t, int& k, int& m0, int& mc, int& n0, int& nc, bool& new_m) {
    if (TILED) {
      const int nt = t % ntile, q = t / ntile, mt = q % ntile;
      k = q / ntile;
      m0 = mt * kRhoNT;
      n0 = nt * kRhoNT;
      mc = min(kRhoNT, nao - m0);
      nc = min(kRhoNT, nao - n0);
      new_m = nt == 0;
    } else {
      k = t;
      m0 = n0 = 0;
      mc = nc = nao;
      new_m = true;
    }
  };
  // element e = tid + 256 i of a tile: tiled, row e / 32 and column e % 32 of the 32-wide tile;
  // untiled, the tile is one contiguous run of f (whole rows) and of D_sk
  auto fetch = [&](int t) {
    int k, m0, mc, n0, nc;
    bool new_m;
    tile_of(t, k, m0, mc, n0, nc, new_m);
    const cplx* fk = f + (long)k * fks + g0 * nao;
    const cplx* Dk = D + (long)k * nao * nao;
    if (new_m) {
#pragma unroll
      for (int i = 0; i < RF; ++i) {
        const int e = tid + 256 * i;
        if constexpr (TILED) {
          const int g = e / kRhoNT, c = e % kRhoNT;
          rm[i] = g < rows && c < mc ? fk[(long)g * nao + m0 + c] : cmk(0, 0);
        } else {
          rm[i] = e < rows * nao ? fk[e] : cmk(0, 0);
        }
      }
    }
    if constexpr (TILED) {
#pragma unroll
      for (int i = 0; i < RF; ++i) {
        const int e = tid + 256 * i, g = e / kRhoNT, c = e % kRhoNT;
        rn[i] = g < rows && c < nc ? fk[(long)g * nao + n0 + c] : cmk(0, 0);
      }
    }
#pragma unroll
    for (int s = 0; s < SC; ++s)
#pragma unroll
      for (int i = 0; i < RD / SC; ++i) {
        const int r = tid + 256 * i;
        if constexpr (TILED) {
          const int m = r / kRhoNT, n = r % kRhoNT;
          rd[s * (RD / SC) + i] =
              m < mc && n < nc ? Dk[s * dset + (long)(m0 + m) * nao + n0 + n] : cmk(0, 0);
        } else {
          rd[s * (RD / SC) + i] = r < nao * nao ? Dk[s * dset + r] : cmk(0, 0);
        }
      }
  };
  auto stash = [&](int t) {
    int k, m0, mc, n0, nc;
    bool new_m;
    tile_of(t, k, m0, mc, n0, nc, new_m);
    if (new_m) {
#pragma unroll
      for (int i = 0; i < RF; ++i) {
        const int e = tid + 256 * i;
        const int g = TILED ? e / kRhoNT : e / nao, c = TILED ? e % kRhoNT : e - g * nao;
        if (g < PT) fm[g * pitch + c] = rm[i];
      }
    }
    if constexpr (TILED) {
#pragma unroll
      for (int i = 0; i < RF; ++i) {
        const int e = tid + 256 * i, g = e / kRhoNT, c = e % kRhoNT;
        fn[g * pitch + c] = rn[i];
      }
    }
#pragma unroll
    for (int s = 0; s < SC; ++s)
#pragma unroll
      for (int i = 0; i < RD / SC; ++i) {
        const int r = tid + 256 * i;
        if (r < nta * nta) Ds[s * nta * nta + r] = rd[s * (RD / SC) + i];
      }
  };

  fetch(0);
  for (int t = 0; t < nsteps; ++t) {
    __syncthreads();  // the previous step's readers are done
    stash(t);
    __syncthreads();
    if (t + 1 < nsteps) fetch(t + 1);
    int k, m0, mc, n0, nc;
    bool new_m;
    tile_of(t, k, m0, mc, n0, nc, new_m);
    // NB columns at a time (n, n + 4, ...): each f element read from LDS meets NB entries of D
    for (int n = j; n < nc; n += 4 * NB) {
      cplx tt[NB][PG][SC];
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int p = 0; p < PG; ++p)
#pragma unroll
          for (int s = 0; s < SC; ++s) tt[b][p][s] = cmk(0, 0);
#pragma unroll 2
      for (int m = 0; m < mc; ++m) {
        cplx a[PG];
#pragma unroll
        for (int p = 0; p < PG; ++p) a[p] = fm[(gl + 64 * p) * pitch + m];
#pragma unroll
        for (int s = 0; s < SC; ++s)
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            // a column past nc reads the slack behind Ds; its sum is dropped below
            const cplx d = Ds[(s * nta + m) * nta + n + 4 * b];
#pragma unroll
            for (int p = 0; p < PG; ++p) cfma(tt[b][p][s], a[p], d);
          }
      }
#pragma unroll
      for (int b = 0; b < NB; ++b)
        if (n + 4 * b < nc) {
#pragma unroll
          for (int p = 0; p < PG; ++p) {
            const cplx c = cconj(fn[(gl + 64 * p) * pitch + n + 4 * b]);
#pragma unroll
            for (int s = 0; s < SC; ++s) cfma(acc[p][s], tt[b][p][s], c);
          }
        }
    }
  }
  // the four waves' column shares, summed in wave order
  __syncthreads();
  cplx* red = smem;  // [4][SC][PT]
#pragma unroll
  for (int p = 0; p < PG; ++p)
#pragma unroll
    for (int s = 0; s < SC; ++s) red[(j * SC + s) * PT + gl + 64 * p] = acc[p][s];
  __syncthreads();
  for (int e = tid; e < SC * PT; e += 256) {
    const int s = e / PT, g = e - s * PT;
    if (g >= rows) continue;
    cplx r = red[s * PT + g];
    for (int w = 1; w < 4; ++w) r = cadd(r, red[(w * SC + s) * PT + g]);
    rho[(long)s * ngrid + g0 + g] = cscale(r, inv_nk);
  }
}

size_t rho_lds_bytes(int nao, int sc, int pg) {
  const int ntile = (nao + kRhoNT - 1) / kRhoNT;
  const int nta = std::min(nao, kRhoNT), pitch = nta | 1;
  const int pt = 64 * pg;
  // + 4: the slack a second column past the tile's last may read (rho_grid_kernel, NB)
  const size_t tiles = (size_t)(ntile > 1 ? 2 : 1) * pt * pitch + (size_t)sc * nta * nta + 4;
  return sizeof(cplx) * std::max(tiles, (size_t)4 * sc * pt);
}

template <int SC, int PG, bool TILED>
int rho_launch(hipStream_t st, const cplx* f, long fks, int nk, int ngrid, int nao, const cplx* D,
               cplx* rho) {
  const size_t lds = rho_lds_bytes(nao, SC, PG);
  FISDF_CHECK(lds <= 160 * 1024, "rho_grid: LDS tile too large");
  FISDF_TRY(func_max_lds((const void*)rho_grid_kernel<SC, PG, TILED>, (int)lds));
  const long blocks = ((long)ngrid + 64 * PG - 1) / (64 * PG);
  hipLaunchKernelGGL((rho_grid_kernel<SC, PG, TILED>), dim3((unsigned)blocks), dim3(256), lds, st, f, fks,
                     nk, ngrid, nao, D, 1.0 / nk, rho);
  FISDF_HIP(hipGetLastError());
  return 0;
}

// ---- out[s][k][m][n] = scale sum_g conj(f_k[g,m]) v_s[g] f_k[g,n] ---------------------------
// Workgroup (tile pair, grid split, k): a 32 x 32 block of the output over the split's grid
// points, kGramGT at a time: the two f column tiles and v_s (conjugated on request) staged in
// LDS, thread (tm, tn) holding the 2 x 2 elements (tm + 16 i, tn + 16 j) of every set.  The
// splits' blocks go to `part` and gram_reduce_kernel sums them in split order.
constexpr int kGramNT = 32, kGramGT = 32;

template <int SC>
__global__ __launch_bounds__(256) void gram_kernel(const cplx* __restrict__ f, long fks, int ngrid,
                                                   int nao, const cplx* __restrict__ v, int conj_v,
                                                   int chunk, cplx* __restrict__ part) {
  __shared__ cplx fm[kGramGT][kGramNT];
  __shared__ cplx fn[kGramGT][kGramNT];
  __shared__ cplx vs[SC][kGramGT];
  const int ntile = (nao + kGramNT - 1) / kGramNT;
  const int mt = blockIdx.x / ntile, nt = blockIdx.x - mt * ntile;
  const int split = blockIdx.y, k = blockIdx.z, nk = gridDim.z;
  const int m0 = mt * kGramNT, n0 = nt * kGramNT;
  const int mc = min(kGramNT, nao - m0), nc = min(kGramNT, nao - n0);
  const int tid = threadIdx.x, tn = tid & 15, tm = tid >> 4;
  const cplx* fk = f + (long)k * fks;
  const long gbeg = (long)split * chunk, gend = min((long)ngrid, gbeg + chunk);
  cplx acc[SC][2][2];
#pragma unroll
  for (int s = 0; s < SC; ++s)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) acc[s][i][jj] = cmk(0, 0);

  // the next step's elements wait in registers while this step's are multiplied
  constexpr int RT = kGramGT * kGramNT / 256;
  cplx ra[RT], rb[RT], rv = cmk(0, 0);
  auto fetch = [&](long g0) {
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const int e = tid + 256 * i, g = e / kGramNT, c = e - g * kGramNT;
      const bool in = g0 + g < gend;
      ra[i] = in && c < mc ? fk[(g0 + g) * nao + m0 + c] : cmk(0, 0);
      rb[i] = in && c < nc ? fk[(g0 + g) * nao + n0 + c] : cmk(0, 0);
    }
    if (tid < SC * kGramGT) {
      const int s = tid / kGramGT, g = tid - s * kGramGT;
      const cplx x = g0 + g < gend ? v[(long)s * ngrid + g0 + g] : cmk(0, 0);
      rv = conj_v ? cconj(x) : x;
    }
  };
  fetch(gbeg);
  for (long g0 = gbeg; g0 < gend; g0 += kGramGT) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const int e = tid + 256 * i, g = e / kGramNT, c = e - g * kGramNT;
      fm[g][c] = ra[i];
      fn[g][c] = rb[i];
    }
    if (tid < SC * kGramGT) vs[tid / kGramGT][tid % kGramGT] = rv;
    __syncthreads();
    if (g0 + kGramGT < gend) fetch(g0 + kGramGT);
#pragma unroll 4
    for (int g = 0; g < kGramGT; ++g) {
      const cplx a0 = cconj(fm[g][tm]), a1 = cconj(fm[g][tm + 16]);
      const cplx b0 = fn[g][tn], b1 = fn[g][tn + 16];
      if (SC <= 2) {  // v folded into the right factor: 8 + 16 operations per set
#pragma unroll
        for (int s = 0; s < SC; ++s) {
          const cplx w = vs[s][g];
          const cplx c0 = cmul(w, b0), c1 = cmul(w, b1);
          cfma(acc[s][0][0], a0, c0);
          cfma(acc[s][0][1], a0, c1);
          cfma(acc[s][1][0], a1, c0);
          cfma(acc[s][1][1], a1, c1);
        }
      } else {        // the products once, then v per set: 16 + 16 SC operations
        const cplx p00 = cmul(a0, b0), p01 = cmul(a0, b1), p10 = cmul(a1, b0), p11 = cmul(a1, b1);
#pragma unroll
        for (int s = 0; s < SC; ++s) {
          const cplx w = vs[s][g];
          cfma(acc[s][0][0], w, p00);
          cfma(acc[s][0][1], w, p01);
          cfma(acc[s][1][0], w, p10);
          cfma(acc[s][1][1], w, p11);
        }
      }
    }
  }
  const long nn = (long)nao * nao;
#pragma unroll
  for (int s = 0; s < SC; ++s) {
    cplx* o = part + (((long)split * SC + s) * nk + k) * nn;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int m = tm + 16 * i, n = tn + 16 * jj;
        if (m < mc && n < nc) o[(long)(m0 + m) * nao + n0 + n] = acc[s][i][jj];
      }
  }
}

// out[e] = scale * (part[0][e] + part[1][e] + ...), e over the chunk's sc * nk * nao * nao
__global__ void gram_reduce_kernel(const cplx* __restrict__ part, int nsplit, long n, double scale,
                                   cplx* __restrict__ out) {
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (e >= n) return;
  cplx r = part[e];
  for (int sp = 1; sp < nsplit; ++sp) r = cadd(r, part[(long)sp * n + e]);
  out[e] = cscale(r, scale);
}

__global__ void conj_kernel(cplx* __restrict__ a, long n) {
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (e < n) a[e].y = -a[e].y;
}

template <int SC>
int gram_launch(hipStream_t st, const cplx* f, long fks, int nk, int ngrid, int nao, const cplx* v,
                int conj_v, double scale, cplx* out, cplx* part) {
  int chunk, nsplit;
  weighted_gram_split(nk, ngrid, nao, &chunk, &nsplit);
  const int ntile = (nao + kGramNT - 1) / kGramNT;
  hipLaunchKernelGGL(gram_kernel<SC>, dim3(ntile * ntile, nsplit, nk), dim3(256), 0, st, f, fks,
                     ngrid, nao, v, conj_v, chunk, part);
  FISDF_HIP(hipGetLastError());
  const long n = (long)SC * nk * nao * nao;
  hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part,
                     nsplit, n, scale, out);
  FISDF_HIP(hipGetLastError());
  return 0;
}

}  // namespace

bool rho_grid_tiled(int nao) { return nao > kRhoNT; }

int rho_grid(hipStream_t st, const cplx* f, long fks, int nk, int ngrid, int nao, const cplx* D,
             int nset, cplx* rho) {
  FISDF_CHECK(f && D && rho, "rho_grid: null pointer");
  FISDF_CHECK(nk >= 1 && ngrid >= 1 && nao >= 1 && nset >= 1, "rho_grid: sizes must be >= 1");
  FISDF_CHECK(fks >= (long)ngrid * nao, "rho_grid: f_kstride below ngrid * nao");
  FISDF_CHECK((long)nao * nao * nk < (1L << 31), "rho_grid: density matrices too large");
  const bool tiled = rho_grid_tiled(nao);
  const long dset = (long)nk * nao * nao;
  // at most kJfftSetChunk sets per pass over f
  for (int s0 = 0; s0 < nset; s0 += kJfftSetChunk) {
    const int sc = std::min(kJfftSetChunk, nset - s0);
    const cplx* Dc = D + s0 * dset;
    cplx* rc = rho + (long)s0 * ngrid;
    int rc_ = 0;
#define FISDF_RHO(SC)                                                                  \
  if (sc == SC)                                                                        \
    rc_ = tiled ? rho_launch<SC, 1, true>(st, f, fks, nk, ngrid, nao, Dc, rc)          \
                : rho_launch<SC, (SC == 1 ? 2 : 1), false>(st, f, fks, nk, ngrid, nao, Dc, rc);
    FISDF_RHO(1) FISDF_RHO(2) FISDF_RHO(3) FISDF_RHO(4)
#undef FISDF_RHO
    FISDF_TRY(rc_);
  }
  return 0;
}

void weighted_gram_split(int nk, int ngrid, int nao, int* chunk, int* nsplit) {
  const int ntile = (nao + kGramNT - 1) / kGramNT;
  const long wgs = (long)nk * ntile * ntile;
  // about kGramWgs workgroups in all, at least four grid tiles per split
  long want = std::max(1L, (kGramWgs + wgs - 1) / wgs);
  want = std::min(want, std::max(1L, ((long)ngrid + 4 * kGramGT - 1) / (4 * kGramGT)));
  long c = ((long)ngrid + want - 1) / want;
  c = (c + kGramGT - 1) / kGramGT * kGramGT;
  *chunk = (int)c;
  *nsplit = (int)(((long)ngrid + c - 1) / c);
}

long weighted_gram_work_elems(int nk, int ngrid, int nao, int nset) {
  int chunk, nsplit;
  weighted_gram_split(nk, ngrid, nao, &chunk, &nsplit);
  return (long)nsplit * std::min(nset, kJfftSetChunk) * nk * nao * nao;
}

int weighted_gram(hipStream_t st, const cplx* f, long fks, int nk, int ngrid, int nao,
                  const cplx* v, int nset, int conj_v, double scale, cplx* out, cplx* work,
                  long work_elems) {
  FISDF_CHECK(f && v && out && work, "weighted_gram: null pointer");
  FISDF_CHECK(nk >= 1 && ngrid >= 1 && nao >= 1 && nset >= 1, "weighted_gram: sizes must be >= 1");
  FISDF_CHECK(nk <= 65535, "weighted_gram: more than 65535 k-points");
  FISDF_CHECK(fks >= (long)ngrid * nao, "weighted_gram: f_kstride below ngrid * nao");
  FISDF_CHECK(work_elems >= weighted_gram_work_elems(nk, ngrid, nao, nset),
              "weighted_gram: workspace too small");
  const long oset = (long)nk * nao * nao;
  for (int s0 = 0; s0 < nset; s0 += kJfftSetChunk) {
    const int sc = std::min(kJfftSetChunk, nset - s0);
    const cplx* vc = v + (long)s0 * ngrid;
    cplx* oc = out + s0 * oset;
    int rc_ = 0;
#define FISDF_GRAM(SC) \
  if (sc == SC) rc_ = gram_launch<SC>(st, f, fks, nk, ngrid, nao, vc, conj_v, scale, oc, work);
    FISDF_GRAM(1) FISDF_GRAM(2) FISDF_GRAM(3) FISDF_GRAM(4)
#undef FISDF_GRAM
    FISDF_TRY(rc_);
  }
  return 0;
}

int conj_inplace(hipStream_t st, cplx* a, long n) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(conj_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, n);
  FISDF_HIP(hipGetLastError());
  return 0;
}

}  // namespace fisdf
