// GTH pseudopotential and nuclear-attraction matrices (PySCF FFTDF.get_pp / get_nuc restated; the
// definitions are in include/fisdf.h and DESIGN 3.13).  The local part is a structure-factor sum
// over the atoms in G space (vloc_g_kernel), one transform and the weighted AO Gram of the exact J;
// the non-local part the separable projectors of one k-point, contiguous along G
// (gth_projector_kernel), transformed by the plain forward fft3d, their overlaps with the Bloch
// AOs read where they lie (pp_overlap_kernel) and c^H h c (pp_vnl_kernel).  Vector stores only, no
// atomics; every sum has a fixed order.
#include "common.h"
#include "linalg.h"
#include "sph.h"

#include <algorithm>

#include "fisdf.h"

namespace fisdf {

namespace {

struct Recip {
  double b[3][3];
};

// the fftfreq integer of index i on an axis of n points
__device__ __forceinline__ int pp_freq(int i, int n) { return i < (n + 1) / 2 ? i : i - n; }

// G = (fftfreq integers of the flat index g) . b
__device__ __forceinline__ void pp_gvec(long g, int n0, int n1, int n2, const Recip& rb, int f[3],
                                        double G[3]) {
  const int i2 = (int)(g % n2), i1 = (int)((g / n2) % n1), i0 = (int)(g / ((long)n1 * n2));
  f[0] = pp_freq(i0, n0), f[1] = pp_freq(i1, n1), f[2] = pp_freq(i2, n2);
#pragma unroll
  for (int c = 0; c < 3; ++c) G[c] = f[0] * rb.b[0][c] + f[1] * rb.b[1][c] + f[2] * rb.b[2][c];
}

// ---- out[G] = scale sum_a SI_a(G) v_a(|G|) ---------------------------------------------------------
// One thread per G, the atoms in table order.  A bare nucleus is rloc = 0, c = 0 in the table: the
// pseudopotential's own formulas then give -4 pi Z / G^2, and 0 at G = 0.
__global__ __launch_bounds__(256) void vloc_g_kernel(const double* __restrict__ tab, int natm,
                                                     int n0, int n1, int n2, Recip rb, double scale,
                                                     int conj_out, cplx* __restrict__ out) {
  const long ngrid = (long)n0 * n1 * n2;
  const long g = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (g >= ngrid) return;
  int f[3];
  double G[3];
  pp_gvec(g, n0, n1, n2, rb, f, G);
  const double G2 = G[0] * G[0] + G[1] * G[1] + G[2] * G[2];
  const bool zero = f[0] == 0 && f[1] == 0 && f[2] == 0;
  const double fourpi = 12.566370614359172, twopi = 6.283185307179586;
  const double twopi32 = 15.749609945722419;  // (2 pi)^(3/2)
  cplx acc = cmk(0, 0);
  for (int a = 0; a < natm; ++a) {
    const double* t = tab + (long)kPpVlocCols * a;
    const double Z = t[3], rloc = t[4], c1 = t[5], c2 = t[6], c3 = t[7], c4 = t[8];
    const double rl2 = rloc * rloc, rl3 = rl2 * rloc;
    if (zero) {
      acc.x += twopi * Z * rl2 + twopi32 * rl3 * (c1 + 3 * c2 + 15 * c3 + 105 * c4);
      continue;
    }
    const double x2 = G2 * rl2, x4 = x2 * x2;
    const double e = exp(-0.5 * x2);
    const double poly = c1 + c2 * (3 - x2) + c3 * (15 - 10 * x2 + x4) +
                        c4 * (105 - 105 * x2 + 21 * x4 - x4 * x2);
    const double v = e * (-Z * fourpi / G2 + twopi32 * rl3 * poly);
    double sn, cs;
    sincos(G[0] * t[0] + G[1] * t[1] + G[2] * t[2], &sn, &cs);
    acc.x += v * cs;
    acc.y -= v * sn;
  }
  out[g] = cmk(scale * acc.x, conj_out ? -scale * acc.y : scale * acc.y);
}

// q_{l,i}(x) of the closed form P_i^l = q pi^{5/4} r_l^{l + 3/2} e^{-x^2/2}, i = 0, 1, 2
__device__ __forceinline__ double pp_q(int l, int i, double x2) {
  const double x4 = x2 * x2;
  switch (l) {
    case 0:
      if (i == 0) return 4.0 * sqrt(2.0);
      if (i == 1) return 8.0 * sqrt(2.0 / 15.0) * (3 - x2);
      return 16.0 / 3.0 * sqrt(2.0 / 105.0) * (15 - 10 * x2 + x4);
    case 1:
      if (i == 0) return 8.0 / sqrt(3.0);
      if (i == 1) return 16.0 / sqrt(105.0) * (5 - x2);
      return 32.0 / 3.0 / sqrt(1155.0) * (35 - 14 * x2 + x4);
    case 2:
      if (i == 0) return 8.0 * sqrt(2.0 / 15.0);
      if (i == 1) return 16.0 / 3.0 * sqrt(2.0 / 105.0) * (7 - x2);
      return 32.0 / 3.0 * sqrt(2.0 / 15015.0) * (63 - 18 * x2 + x4);
    default:
      if (i == 0) return 16.0 / sqrt(105.0);
      if (i == 1) return 32.0 / 3.0 / sqrt(1155.0) * (9 - x2);
      return 64.0 / 45.0 / sqrt(1001.0) * (99 - 22 * x2 + x4);
  }
}

// ---- rows[row0 + i (2 l + 1) + mm][G] = conj(beta(G; k)) of one (atom, l) channel per blockIdx.y ---
// One thread per (G, channel): the phase e^{+i K.R}, e^{-x^2/2} and r_l^{l + 3/2} once, shared by
// the channel's n (2 l + 1) rows; consecutive threads write consecutive G of a row.
__global__ __launch_bounds__(256) void gth_projector_kernel(const PpBlock* __restrict__ blocks,
                                                            int n0, int n1, int n2, Recip rb,
                                                            double k0, double k1, double k2,
                                                            cplx* __restrict__ rows) {
  const long ngrid = (long)n0 * n1 * n2;
  const long g = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (g >= ngrid) return;
  const PpBlock B = blocks[blockIdx.y];
  int f[3];
  double K[3];
  pp_gvec(g, n0, n1, n2, rb, f, K);
  K[0] += k0, K[1] += k1, K[2] += k2;
  const double K2 = K[0] * K[0] + K[1] * K[1] + K[2] * K[2];
  double sn, cs;
  sincos(K[0] * B.R[0] + K[1] * B.R[1] + K[2] * B.R[2], &sn, &cs);
  const double x2 = K2 * B.rl * B.rl;
  double base = 4.182513398379599 * B.rl * sqrt(B.rl) * exp(-0.5 * x2);  // pi^(5/4) r^(3/2) e
  for (int j = 0; j < B.l; ++j) base *= B.rl;
  const int nm = 2 * B.l + 1;
  double P[3];
  for (int i = 0; i < B.n; ++i) P[i] = pp_q(B.l, i, x2) * base;
  for (int mm = 0; mm < nm; ++mm) {
    const double S = real_sph(B.l, mm, K[0], K[1], K[2]);
    for (int i = 0; i < B.n; ++i) {
      const double r = P[i] * S;
      rows[(long)(B.row0 + i * nm + mm) * ngrid + g] = cmk(r * cs, r * sn);
    }
  }
}

// ---- part[run][p][m] = sum_{g in run} t[p][g] exp(-i frac(g).kd) f[g][m] ---------------------------
// Workgroup (run, AO tile of kPpMT, projector tile of kPpPT).  Per step of kPpGT points: the
// points' AO columns of the tile are staged in LDS as they lie (runs of contiguous columns), the
// projector rows times the phase beside them; thread (m, pg) then sums the points in order for
// the rows pg and pg + 8.  The phase comes from the point's mesh indices (fft3d's separable
// phase), one sincos per point and step, by the first wave.  Points and rows beyond the ends are
// staged as zeros.
__global__ __launch_bounds__(256) void pp_overlap_kernel(const cplx* __restrict__ t, int np,
                                                         const cplx* __restrict__ f, int nao,
                                                         int ngrid, int run_len, int n0, int n1,
                                                         int n2, double kd0, double kd1, double kd2,
                                                         int use_phase, cplx* __restrict__ part) {
  __shared__ cplx sf[kPpGT * kPpMT];
  __shared__ cplx st[kPpPT * kPpGT];
  __shared__ cplx sp[kPpGT];
  const int tid = threadIdx.x, mu = tid & (kPpMT - 1), pg = tid / kPpMT;
  const int run = blockIdx.x, m0 = blockIdx.y * kPpMT, p0 = blockIdx.z * kPpPT;
  const long gbeg = (long)run * run_len, gend = min((long)ngrid, gbeg + run_len);
  cplx acc0 = cmk(0, 0), acc1 = cmk(0, 0);
  for (long g0 = gbeg; g0 < gend; g0 += kPpGT) {
    const int rows = (int)min((long)kPpGT, gend - g0);
    if (tid < kPpGT) {
      cplx ph = cmk(1, 0);
      if (use_phase && tid < rows) {
        const long g = g0 + tid;
        const int i2 = (int)(g % n2), i1 = (int)((g / n2) % n1), i0 = (int)(g / ((long)n1 * n2));
        const double th = (double)pp_freq(i0, n0) / n0 * kd0 + (double)pp_freq(i1, n1) / n1 * kd1 +
                          (double)pp_freq(i2, n2) / n2 * kd2;
        double sn, cs;
        sincos(th, &sn, &cs);
        ph = cmk(cs, -sn);
      }
      sp[tid] = ph;
    }
    for (int e = tid; e < kPpGT * kPpMT; e += 256) {
      const int g = e / kPpMT, c = e - g * kPpMT;
      sf[e] = g < rows && m0 + c < nao ? f[(g0 + g) * nao + m0 + c] : cmk(0, 0);
    }
    __syncthreads();
    for (int e = tid; e < kPpPT * kPpGT; e += 256) {
      const int p = e / kPpGT, g = e - p * kPpGT;
      st[e] = g < rows && p0 + p < np ? cmul(t[(long)(p0 + p) * ngrid + g0 + g], sp[g]) : cmk(0, 0);
    }
    __syncthreads();
    for (int g = 0; g < kPpGT; ++g) {
      const cplx a = sf[g * kPpMT + mu];
      cfma(acc0, st[pg * kPpGT + g], a);
      cfma(acc1, st[(pg + 8) * kPpGT + g], a);
    }
    __syncthreads();
  }
  if (m0 + mu < nao) {
    if (p0 + pg < np) part[((long)run * np + p0 + pg) * nao + m0 + mu] = acc0;
    if (p0 + pg + 8 < np) part[((long)run * np + p0 + pg + 8) * nao + m0 + mu] = acc1;
  }
}

// c[e] = scale sum_run part[run][e], in run order
__global__ void pp_reduce_kernel(const cplx* __restrict__ part, long n, int nrun, double scale,
                                 cplx* __restrict__ c) {
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (e >= n) return;
  cplx acc = part[e];
  for (int r = 1; r < nrun; ++r) acc = cadd(acc, part[(long)r * n + e]);
  c[e] = cscale(acc, scale);
}

// out[m][n] += sum over channels, mm, i, j of conj(c[(i, mm)][m]) h[i][j] c[(j, mm)][n]: one thread
// per element, every term added to the element's running value in table order
__global__ void pp_vnl_kernel(const cplx* __restrict__ c, int nao, const PpBlock* __restrict__ blocks,
                              int nblocks, cplx* __restrict__ out) {
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (e >= (long)nao * nao) return;
  const int m = (int)(e / nao), n = (int)(e - (long)m * nao);
  cplx acc = out[e];
  for (int b = 0; b < nblocks; ++b) {
    const PpBlock& B = blocks[b];
    const int nm = 2 * B.l + 1;
    for (int mm = 0; mm < nm; ++mm)
      for (int i = 0; i < B.n; ++i) {
        const cplx ci = cconj(c[(long)(B.row0 + i * nm + mm) * nao + m]);
        for (int j = 0; j < B.n; ++j)
          acc = cadd(acc, cmul(ci, cscale(c[(long)(B.row0 + j * nm + mm) * nao + n], B.h[3 * i + j])));
      }
  }
  out[e] = acc;
}

Recip recip_of(const CellGeom& g) {
  Recip r;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r.b[i][j] = g.b[i][j];
  return r;
}

int pp_mesh_check(const int mesh[3], long* ngrid, const char* who) {
  FISDF_CHECK(mesh && mesh[0] >= 1 && mesh[1] >= 1 && mesh[2] >= 1, std::string(who) + ": bad mesh");
  *ngrid = (long)mesh[0] * mesh[1] * mesh[2];
  FISDF_CHECK(*ngrid < (1L << 31), std::string(who) + ": mesh too large");
  return 0;
}

}  // namespace

int pp_check_table(const fisdf_pp_atom* atoms, int natm, const char* who) {
  const std::string w(who);
  FISDF_CHECK(atoms && natm >= 1, w + ": the atom table is empty");
  for (int a = 0; a < natm; ++a) {
    const fisdf_pp_atom& A = atoms[a];
    if (A.bare) continue;
    FISDF_CHECK(A.nexp >= 0 && A.nexp <= 4, w + ": nexp must be in [0, 4]");
    FISDF_CHECK(A.rloc > 0, w + ": rloc must be > 0");
    FISDF_CHECK(A.nl >= 0 && A.nl <= 4, w + ": angular momentum must be <= 3");
    for (int l = 0; l < A.nl; ++l) {
      FISDF_CHECK(A.n[l] >= 0 && A.n[l] <= 3, w + ": at most 3 projectors per channel");
      FISDF_CHECK(A.n[l] == 0 || A.rl[l] > 0, w + ": r_l must be > 0");
    }
  }
  return 0;
}

long pp_rows(const fisdf_pp_atom* atoms, int a0, int a1) {
  long rows = 0;
  for (int a = a0; a < a1; ++a)
    if (!atoms[a].bare)
      for (int l = 0; l < atoms[a].nl; ++l) rows += (long)atoms[a].n[l] * (2 * l + 1);
  return rows;
}

void pp_vloc_table(const fisdf_pp_atom* atoms, int natm, std::vector<double>* tab) {
  tab->assign((size_t)kPpVlocCols * natm, 0.0);
  for (int a = 0; a < natm; ++a) {
    double* t = tab->data() + (size_t)kPpVlocCols * a;
    for (int d = 0; d < 3; ++d) t[d] = atoms[a].r[d];
    t[3] = atoms[a].z;
    if (atoms[a].bare) continue;
    t[4] = atoms[a].rloc;
    for (int j = 0; j < atoms[a].nexp; ++j) t[5 + j] = atoms[a].c[j];
  }
}

void pp_blocks(const fisdf_pp_atom* atoms, int a0, int a1, std::vector<PpBlock>* blocks) {
  blocks->clear();
  int row = 0;
  for (int a = a0; a < a1; ++a) {
    if (atoms[a].bare) continue;
    for (int l = 0; l < atoms[a].nl; ++l) {
      if (atoms[a].n[l] == 0) continue;
      PpBlock B;
      for (int d = 0; d < 3; ++d) B.R[d] = atoms[a].r[d];
      B.rl = atoms[a].rl[l];
      for (int j = 0; j < 9; ++j) B.h[j] = atoms[a].h[l][j];
      B.l = l, B.n = atoms[a].n[l], B.row0 = row, B.pad = 0;
      row += B.n * (2 * l + 1);
      blocks->push_back(B);
    }
  }
}

int vloc_g(hipStream_t s, const int mesh[3], const CellGeom& g, const double* tab, int natm,
           double scale, int conj_out, cplx* out) {
  long ngrid = 0;
  FISDF_TRY(pp_mesh_check(mesh, &ngrid, "vloc_g"));
  FISDF_CHECK(tab && out && natm >= 1, "vloc_g: null pointer or no atoms");
  hipLaunchKernelGGL(vloc_g_kernel, dim3((unsigned)((ngrid + 255) / 256)), dim3(256), 0, s, tab, natm,
                     mesh[0], mesh[1], mesh[2], recip_of(g), scale, conj_out, out);
  FISDF_HIP(hipGetLastError());
  return 0;
}

int gth_projectors(hipStream_t s, const int mesh[3], const CellGeom& g, const double k[3],
                   const PpBlock* blocks, int nblocks, cplx* rows) {
  long ngrid = 0;
  FISDF_TRY(pp_mesh_check(mesh, &ngrid, "gth_projectors"));
  FISDF_CHECK(blocks && rows && k, "gth_projectors: null pointer");
  FISDF_CHECK(nblocks >= 1 && nblocks <= 65535, "gth_projectors: 1 to 65535 channels per launch");
  hipLaunchKernelGGL(gth_projector_kernel, dim3((unsigned)((ngrid + 255) / 256), nblocks), dim3(256),
                     0, s, blocks, mesh[0], mesh[1], mesh[2], recip_of(g), k[0], k[1], k[2], rows);
  FISDF_HIP(hipGetLastError());
  return 0;
}

void pp_overlap_split(long ngrid, int* run_len, int* nrun) {
  const long steps = (ngrid + kPpGT - 1) / kPpGT;
  const long per = std::max<long>(1, (steps + kPpRuns - 1) / kPpRuns);
  *run_len = (int)(per * kPpGT);
  *nrun = (int)std::max<long>(1, (ngrid + *run_len - 1) / *run_len);
}

int pp_overlap(hipStream_t s, const cplx* t, int np, const cplx* f, int nao, const int mesh[3],
               const double* kd, double scale, cplx* c, cplx* part) {
  long ngrid = 0;
  FISDF_TRY(pp_mesh_check(mesh, &ngrid, "pp_overlap"));
  FISDF_CHECK(t && f && c && part, "pp_overlap: null pointer");
  FISDF_CHECK(np >= 1 && nao >= 1, "pp_overlap: sizes must be >= 1");
  const int mt = (nao + kPpMT - 1) / kPpMT, pt = (np + kPpPT - 1) / kPpPT;
  FISDF_CHECK(mt <= 65535 && pt <= 65535, "pp_overlap: too many tiles");
  int run_len = 0, nrun = 0;
  pp_overlap_split(ngrid, &run_len, &nrun);
  hipLaunchKernelGGL(pp_overlap_kernel, dim3(nrun, mt, pt), dim3(256), 0, s, t, np, f, nao,
                     (int)ngrid, run_len, mesh[0], mesh[1], mesh[2], kd ? kd[0] : 0.0,
                     kd ? kd[1] : 0.0, kd ? kd[2] : 0.0, kd ? 1 : 0, part);
  FISDF_HIP(hipGetLastError());
  const long n = (long)np * nao;
  hipLaunchKernelGGL(pp_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, n,
                     nrun, scale, c);
  FISDF_HIP(hipGetLastError());
  return 0;
}

int pp_vnl(hipStream_t s, const cplx* c, int nao, const PpBlock* blocks, int nblocks, cplx* out) {
  FISDF_CHECK(c && blocks && out && nao >= 1 && nblocks >= 1, "pp_vnl: bad arguments");
  const long n = (long)nao * nao;
  hipLaunchKernelGGL(pp_vnl_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c, nao,
                     blocks, nblocks, out);
  FISDF_HIP(hipGetLastError());
  return 0;
}

void pp_plan(int nao, long ngrid, int nk, const fisdf_pp_atom* atoms, int natm, int with_nonlocal,
             long work_bytes, PpPlan* p) {
  *p = PpPlan();
  if (nao < 1 || nao > kKfftMaxNao || ngrid < 1 || ngrid >= (1L << 31) || nk < 1 || nk > 65535 ||
      natm < 0 || work_bytes < 0)
    return;
  pp_overlap_split(ngrid, &p->run_len, &p->nrun);
  p->mtiles = (nao + kPpMT - 1) / kPpMT;
  const long budget = work_bytes ? work_bytes : kKfftWorkBytes;
  const long row_bytes = (long)sizeof(cplx) * ngrid;
  p->chunk_a.push_back(0);
  if (with_nonlocal && atoms) {
    p->nproj = (int)pp_rows(atoms, 0, natm);
    // whole atoms while their rows fit the budget; atoms without projectors ride along
    long rows = 0;
    std::vector<PpBlock> blk;
    for (int a = 0; a < natm && p->nproj > 0; ++a) {
      const long ra = pp_rows(atoms, a, a + 1);
      if (ra * row_bytes > budget) return;  // an atom's own rows exceed the budget
      if (rows > 0 && (rows + ra) * row_bytes > budget) {
        p->chunk_a.push_back(a);
        rows = 0;
      }
      rows += ra;
      p->chunk_rows = (int)std::max<long>(p->chunk_rows, rows);
    }
    if (p->nproj > 0) {
      p->chunk_a.push_back(natm);
      p->nchunk = (int)p->chunk_a.size() - 1;
      pp_blocks(atoms, 0, natm, &blk);
      p->max_blocks = (int)blk.size();
    }
  }
  auto al = [](long b) { return (b + 255) / 256 * 256; };
  p->gram_elems = weighted_gram_work_elems(nk, (int)ngrid, nao, 1);
  p->off_v = 0;
  p->off_gram = p->off_v + al(row_bytes);
  p->off_rows = p->off_gram + al((long)sizeof(cplx) * p->gram_elems);
  p->off_part = p->off_rows + al(row_bytes * p->chunk_rows);
  p->off_c = p->off_part + al((long)sizeof(cplx) * p->nrun * p->chunk_rows * nao);
  p->off_tab = p->off_c + al((long)sizeof(cplx) * p->chunk_rows * nao);
  p->off_blk = p->off_tab + al((long)sizeof(double) * kPpVlocCols * std::max(natm, 1));
  p->bytes = p->off_blk + al((long)sizeof(PpBlock) * std::max(p->max_blocks, 1));
  p->ok = 1;
}

}  // namespace fisdf
