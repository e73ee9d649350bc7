// The grid side of a GGA step over the four-component Bloch-AO block f4[k][c][g][m] (c = 0 the
// value, 1..3 its x, y, z derivatives; fisdf_eval_ao_deriv1): the density with its gradient, and
// the potential matrix of a caller's wv.  Deterministic: no floating-point atomics, partial sums
// are combined in a fixed order.
#include "common.h"
#include "linalg.h"

#include <algorithm>

namespace fisdf {

namespace {

// ---- rho_c[s][g], c = 0..3 ---------------------------------------------------------------------
//   rho_0  = (1/nk) sum_k sum_mn f[g,m] D[m,n] conj f[g,n]
//   d_c rho = (1/nk) sum_k sum_mn (d_c f[g,m] D[m,n] conj f[g,n] + f[g,m] D[m,n] conj d_c f[g,n])
// rho_grid_kernel's structure (jfft.hip) with the n-side rows in four components: a workgroup of
// 256 threads owns kXcPT = 32 grid points (half of rho_grid's 64: the four-component rows of nao
// 26 then take 55 KB and two workgroups share a CU) and loops over the (k, m-tile, n-tile) steps,
// the next step's elements fetched into registers before the current step's arithmetic.  Thread
// (point gl, column group j of 8) forms t_s = sum_m f[g,m] D_s[m,n] for n = j, j + 8, ... and
//   hermi: d_c rho += 2 Re(t conj d_c f[g,n])         (three real dot products more than rho_0)
//   else:  d_c rho += t conj d_c f[g,n] + conj(u) d_c f[g,n],  u[n] = sum_m f[g,m] conj D[n,m]
// (the first term of the definition, written with the value rows on the m side: only the n side
// is staged in four components).  Tiled, u needs the tile D[n-tile][m-tile] beside D[m-tile]
// [n-tile], which halves the sets per pass there.  The eight groups' sums are combined through
// LDS in group order.
constexpr int kXcNT = 32, kXcPT = 32, kXcGroups = 8;

template <int SC, bool HERMI, bool TILED>
__global__ __launch_bounds__(256) void rho_gga_kernel(const cplx* __restrict__ f4, long fks,
                                                      long fcs, int nk, int ngrid, int nao,
                                                      const cplx* __restrict__ D, double inv_nk,
                                                      cplx* __restrict__ rho, long rcs) {
  extern __shared__ cplx smem[];
  constexpr int PT = kXcPT, NT = kXcNT;
  constexpr int RF = PT * NT / 256;   // f elements per thread, component and tile
  constexpr int RD = NT * NT / 256;   // D elements per thread, set and tile
  constexpr bool DT = TILED && !HERMI;
  const int ntile = TILED ? (nao + NT - 1) / NT : 1;
  const int W = TILED ? NT : nao;     // width of a staged tile
  const int pitch = W | 1;
  cplx* fn = smem;                                   // [4][PT][pitch]
  cplx* fm = TILED ? fn + 4 * PT * pitch : fn;       // [PT][pitch]; untiled: component 0 of fn
  cplx* Ds = smem + (TILED ? 5 : 4) * PT * pitch;    // [SC][W][W]
  cplx* Du = DT ? Ds + SC * W * W : Ds;              // D[n-tile][m-tile]
  const int tid = threadIdx.x, gl = tid & (PT - 1), j = tid / PT;
  const long g0 = (long)blockIdx.x * PT;
  const int rows = (int)min((long)PT, ngrid - g0);
  const long dset = (long)nk * nao * nao;
  const int nsteps = nk * ntile * ntile;
  cplx acc0[SC], accg[3][SC];   // hermi: accg[c][s].x holds Re, .y stays 0
#pragma unroll
  for (int s = 0; s < SC; ++s) {
    acc0[s] = cmk(0, 0);
#pragma unroll
    for (int c = 0; c < 3; ++c) accg[c][s] = cmk(0, 0);
  }
  cplx rn[4][RF], rm[RF], rd[SC][RD], rt[DT ? SC : 1][RD];

  auto tile_of = [&](int t, int& k, int& m0, int& mc, int& n0, int& nc) {
    if (TILED) {
      const int nt = t % ntile, q = t / ntile, mt = q % ntile;
      k = q / ntile;
      m0 = mt * NT;
      n0 = nt * NT;
      mc = min(NT, nao - m0);
      nc = min(NT, nao - n0);
    } else {
      k = t;
      m0 = n0 = 0;
      mc = nc = nao;
    }
  };
  auto fetch = [&](int t) {
    int k, m0, mc, n0, nc;
    tile_of(t, k, m0, mc, n0, nc);
    const cplx* fk = f4 + (long)k * fks + g0 * nao;
    const cplx* Dk = D + (long)k * nao * nao;
#pragma unroll
    for (int i = 0; i < RF; ++i) {
      const int e = tid + 256 * i, g = e / W, cc = e - g * W;
      const bool in = g < rows;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        rn[c][i] = in && cc < nc ? fk[c * fcs + (long)g * nao + n0 + cc] : cmk(0, 0);
      if constexpr (TILED) rm[i] = in && cc < mc ? fk[(long)g * nao + m0 + cc] : cmk(0, 0);
    }
#pragma unroll
    for (int s = 0; s < SC; ++s)
#pragma unroll
      for (int i = 0; i < RD; ++i) {
        const int r = tid + 256 * i, m = r / W, n = r - m * W;
        rd[s][i] = m < mc && n < nc ? Dk[s * dset + (long)(m0 + m) * nao + n0 + n] : cmk(0, 0);
        if constexpr (DT)
          rt[s][i] = m < nc && n < mc ? Dk[s * dset + (long)(n0 + m) * nao + m0 + n] : cmk(0, 0);
      }
  };
  auto stash = [&]() {
#pragma unroll
    for (int i = 0; i < RF; ++i) {
      const int e = tid + 256 * i, g = e / W, cc = e - g * W;
      if (g < PT) {
#pragma unroll
        for (int c = 0; c < 4; ++c) fn[(c * PT + g) * pitch + cc] = rn[c][i];
        if constexpr (TILED) fm[g * pitch + cc] = rm[i];
      }
    }
#pragma unroll
    for (int s = 0; s < SC; ++s)
#pragma unroll
      for (int i = 0; i < RD; ++i) {
        const int r = tid + 256 * i;
        if (r < W * W) {
          Ds[s * W * W + r] = rd[s][i];
          if constexpr (DT) Du[s * W * W + r] = rt[s][i];
        }
      }
  };

  fetch(0);
  for (int t = 0; t < nsteps; ++t) {
    __syncthreads();  // the previous step's readers are done
    stash();
    __syncthreads();
    if (t + 1 < nsteps) fetch(t + 1);
    int k, m0, mc, n0, nc;
    tile_of(t, k, m0, mc, n0, nc);
    for (int n = j; n < nc; n += kXcGroups) {
      cplx tt[SC], uu[SC];
#pragma unroll
      for (int s = 0; s < SC; ++s) tt[s] = uu[s] = cmk(0, 0);
#pragma unroll 2
      for (int m = 0; m < mc; ++m) {
        const cplx a = fm[gl * pitch + m];
#pragma unroll
        for (int s = 0; s < SC; ++s) {
          cfma(tt[s], a, Ds[(s * W + m) * W + n]);
          if constexpr (!HERMI) cfma(uu[s], a, cconj(Du[(s * W + n) * W + m]));
        }
      }
      const cplx c0 = cconj(fn[gl * pitch + n]);
#pragma unroll
      for (int s = 0; s < SC; ++s) cfma(acc0[s], tt[s], c0);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const cplx d = fn[((c + 1) * PT + gl) * pitch + n];
#pragma unroll
        for (int s = 0; s < SC; ++s) {
          if constexpr (HERMI) {
            accg[c][s].x = fma(tt[s].x, d.x, accg[c][s].x);
            accg[c][s].x = fma(tt[s].y, d.y, accg[c][s].x);
          } else {
            cfma(accg[c][s], tt[s], cconj(d));
            cfma(accg[c][s], cconj(uu[s]), d);
          }
        }
      }
    }
  }
  // the eight groups' column shares, summed in group order
  __syncthreads();
  cplx* red = smem;  // [kXcGroups][4][SC][PT]
#pragma unroll
  for (int s = 0; s < SC; ++s) {
    red[((j * 4 + 0) * SC + s) * PT + gl] = acc0[s];
#pragma unroll
    for (int c = 0; c < 3; ++c) red[((j * 4 + c + 1) * SC + s) * PT + gl] = accg[c][s];
  }
  __syncthreads();
  for (int e = tid; e < 4 * SC * PT; e += 256) {
    const int g = e % PT, cs = e / PT, s = cs % SC, c = cs / SC;
    if (g >= rows) continue;
    cplx r = red[(c * SC + s) * PT + g];
    for (int w = 1; w < kXcGroups; ++w) r = cadd(r, red[((w * 4 + c) * SC + s) * PT + g]);
    // hermi: the gradient is 2 Re of the sum, its imaginary part exactly 0
    const double sc = HERMI && c > 0 ? 2.0 * inv_nk : inv_nk;
    rho[((long)s * 4 + c) * rcs + g0 + g] = cscale(r, sc);
  }
}

template <int SC, bool HERMI, bool TILED>
int rho_gga_launch(hipStream_t st, const cplx* f4, long fks, long fcs, int nk, int ngrid, int nao,
                   const cplx* D, cplx* rho, long rcs) {
  const size_t lds = rho_gga_lds_bytes(nao, SC, HERMI);
  FISDF_CHECK(lds <= 160 * 1024, "rho_grid_gga: LDS tile too large");
  FISDF_TRY(func_max_lds((const void*)rho_gga_kernel<SC, HERMI, TILED>, (int)lds));
  const long blocks = ((long)ngrid + kXcPT - 1) / kXcPT;
  hipLaunchKernelGGL((rho_gga_kernel<SC, HERMI, TILED>), dim3((unsigned)blocks), dim3(256), lds, st,
                     f4, fks, fcs, nk, ngrid, nao, D, 1.0 / nk, rho, rcs);
  FISDF_HIP(hipGetLastError());
  return 0;
}

// ---- aow[k][g][n] = 1/2 w_0[g] f[g,n] + sum_c w_c[g] d_c f[g,n] -------------------------------
__global__ void gga_aow_kernel(const cplx* __restrict__ f4, long fks, long fcs, long per_k, int nao,
                               long total, const double* __restrict__ w, long wcs, int ng,
                               cplx* __restrict__ aow) {
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (e >= total) return;
  const long k = e / per_k, r = e - k * per_k;
  const int g = (int)(r / nao);
  const cplx* p = f4 + k * fks + r;
  const double w0 = 0.5 * w[g];
  cplx a = cscale(p[0], w0);
#pragma unroll
  for (int c = 1; c < 4; ++c) {
    const double wc = w[c * wcs + g];
    const cplx d = p[c * fcs];
    a.x = fma(wc, d.x, a.x);
    a.y = fma(wc, d.y, a.y);
  }
  aow[e] = a;
}

// out[k][m][n] (+)= scale (M[k][m][n] + conj M[k][n][m]): Hermitian bit for bit, diagonal real
__global__ void herm_sum_kernel(const cplx* __restrict__ M, int nao, long total, double scale,
                                int accumulate, cplx* __restrict__ out) {
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (e >= total) return;
  const long nn = (long)nao * nao, k = e / nn, r = e - k * nn;
  const int m = (int)(r / nao), n = (int)(r - (long)m * nao);
  const cplx a = M[e], b = M[k * nn + (long)n * nao + m];
  const cplx v = cmk(scale * (a.x + b.x), scale * (a.y - b.y));
  out[e] = accumulate ? cadd(out[e], v) : v;
}

}  // namespace

bool rho_gga_tiled(int nao) { return nao > kXcNT; }

int rho_gga_set_chunk(int nao, int hermi) { return rho_gga_tiled(nao) && !hermi ? 2 : 4; }

size_t rho_gga_lds_bytes(int nao, int sc, int hermi) {
  const bool tiled = rho_gga_tiled(nao);
  const int w = tiled ? kXcNT : nao, pitch = w | 1;
  const size_t tiles = (size_t)(tiled ? 5 : 4) * kXcPT * pitch +
                       (size_t)sc * w * w * (tiled && !hermi ? 2 : 1);
  return sizeof(cplx) * std::max(tiles, (size_t)kXcGroups * 4 * sc * kXcPT);
}

int rho_grid_gga(hipStream_t st, const cplx* f4, long fks, long fcs, int nk, int ngrid, int nao,
                 const cplx* D, int nset, int hermi, cplx* rho, long rcs) {
  FISDF_CHECK(f4 && D && rho, "rho_grid_gga: null pointer");
  FISDF_CHECK(nk >= 1 && ngrid >= 1 && nao >= 1 && nset >= 1, "rho_grid_gga: sizes must be >= 1");
  FISDF_CHECK(hermi == 0 || hermi == 1, "rho_grid_gga: hermi must be 0 or 1");
  FISDF_CHECK(fcs >= (long)ngrid * nao, "rho_grid_gga: f_cstride below ngrid * nao");
  FISDF_CHECK(fks >= (long)ngrid * nao, "rho_grid_gga: f_kstride below ngrid * nao");
  FISDF_CHECK(rcs >= ngrid, "rho_grid_gga: rho_cstride below ngrid");
  FISDF_CHECK((long)nao * nao * nk < (1L << 31), "rho_grid_gga: density matrices too large");
  const bool tiled = rho_gga_tiled(nao);
  const long dset = (long)nk * nao * nao;
  const int chunk = rho_gga_set_chunk(nao, hermi);
  for (int s0 = 0; s0 < nset; s0 += chunk) {
    const int sc = std::min(chunk, nset - s0);
    const cplx* Dc = D + s0 * dset;
    cplx* rc = rho + (long)s0 * 4 * rcs;
    int rc_ = 0;
#define FISDF_XC_RHO(SC, H, T)                   \
  if (sc == SC && (hermi != 0) == H && tiled == T) \
    rc_ = rho_gga_launch<SC, H, T>(st, f4, fks, fcs, nk, ngrid, nao, Dc, rc, rcs);
    FISDF_XC_RHO(1, true, false) FISDF_XC_RHO(2, true, false) FISDF_XC_RHO(3, true, false)
    FISDF_XC_RHO(4, true, false) FISDF_XC_RHO(1, true, true) FISDF_XC_RHO(2, true, true)
    FISDF_XC_RHO(3, true, true) FISDF_XC_RHO(4, true, true) FISDF_XC_RHO(1, false, false)
    FISDF_XC_RHO(2, false, false) FISDF_XC_RHO(3, false, false) FISDF_XC_RHO(4, false, false)
    FISDF_XC_RHO(1, false, true) FISDF_XC_RHO(2, false, true)
#undef FISDF_XC_RHO
    FISDF_TRY(rc_);
  }
  return 0;
}

int gga_gram_ksplit(int ng) { return std::max(1, std::min(64, ng / 1024)); }

void gga_gram_work(int nk, int ng, int nao, size_t* aow, size_t* m, size_t* split) {
  *aow = (size_t)nk * ng * nao;
  *m = (size_t)nk * nao * nao;
  const int ks = gga_gram_ksplit(ng);
  *split = ks > 1 ? (size_t)ks * nk * nao * nao : 0;
}

int gga_gram(hipStream_t st, const cplx* f4, long fks, long fcs, int nk, int ng, int nao,
             const double* w, long wss, long wcs, int nset, double scale, int accumulate, cplx* out,
             cplx* aow, cplx* M, cplx* split) {
  FISDF_CHECK(f4 && w && out && aow && M, "gga_gram: null pointer");
  FISDF_CHECK(nk >= 1 && ng >= 1 && nao >= 1 && nset >= 1, "gga_gram: sizes must be >= 1");
  FISDF_CHECK(fcs >= (long)ng * nao, "gga_gram: f_cstride below ng * nao");
  FISDF_CHECK(fks >= (long)ng * nao, "gga_gram: f_kstride below ng * nao");
  FISDF_CHECK(wcs >= ng && wss >= ng, "gga_gram: a stride of w below ng");
  const long per_k = (long)ng * nao, total = per_k * nk, nn = (long)nao * nao * nk;
  FISDF_CHECK((total + 255) / 256 < (1L << 31), "gga_gram: block too large");
  const int ks = gga_gram_ksplit(ng);
  for (int s = 0; s < nset; ++s) {
    hipLaunchKernelGGL(gga_aow_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, f4,
                       fks, fcs, per_k, nao, total, w + s * wss, wcs, ng, aow);
    FISDF_HIP(hipGetLastError());
    // M_k = f_k^H aow_k on the FP64 MFMA GEMM, split over the grid points
    FISDF_TRY(zgemm(st, OP_C, OP_N, nao, nao, ng, cmk(1, 0), f4, nao, fks, aow, nao, per_k,
                    cmk(0, 0), M, nao, (long)nao * nao, nk, ks, ks > 1 ? split : nullptr));
    hipLaunchKernelGGL(herm_sum_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, M,
                       nao, nn, scale, accumulate, out + s * nn);
    FISDF_HIP(hipGetLastError());
  }
  return 0;
}

}  // namespace fisdf
