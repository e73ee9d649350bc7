// Exact FFT-grid four-index integrals (PySCF FFTDF.get_eri / ao2mo restated): what the exact K's
// chain — pair densities, the transform pair between two conjugations — needs beside it.  The
// transformed rows Z of (a1, a2) meet a second set of pair densities in one GEMM,
//   eri (R x N) = (vol/ngrid) conj(Z) B^T,   B[(p,k,l)][g] = conj(em[g]) conj(a3_p[g,k]) a4_p[g,l],
// so the tail is the B builder below and the host arithmetic of the driver (eri_fft_plan).  No
// atomics; an element's sum over the grid does not depend on the chunk it is in.
#include "common.h"
#include "linalg.h"

#include <algorithm>
#include <climits>

namespace fisdf {

namespace {

// the fftfreq fraction of index i on an axis of n points
__device__ __forceinline__ double eri_freq(int i, int n) {
  return (double)(i < (n + 1) / 2 ? i : i - n) / (double)n;
}

// The pairs of one launch: pair j has the rows k in [k0[j], k1[j]) of its n3, the first of them
// output row orow[j], and owns the k-tiles [t0[j], t0[j + 1]) of blockIdx.z (an unused slot:
// t0 = INT_MAX)
struct Pair34Segs {
  const cplx* a3[kPair34Cap];
  const cplx* a4[kPair34Cap];
  int k0[kPair34Cap], k1[kPair34Cap], orow[kPair34Cap];
  int t0[kPair34Cap + 1];
};

// ---- B[(orow + k - k0) n4 + l][g] = conj(em[g]) conj(a3_p[g,k]) a4_p[g,l] ------------------------
// pair_density_kernel's tile scheme.  Workgroup (grid tile of kKfftGT points, l-tile, (p, k-tile)):
// the points' a4 columns of the l-tile (TW wide) and a3 columns of the k-tile (TW / 2 wide, at
// least 8) are read as runs of contiguous columns per point and staged in LDS at a pitch odd in
// 16-byte units, so that the lanes of a wave — consecutive grid points of one column — meet no
// bank twice; wave j then writes the rows (k, l), l = j + 4 t, of the tile, each a run of 64
// consecutive grid points.  conj(em[g]) = exp(+i sum_d frac_d(g) kd_d) comes from the point's mesh
// indices (fft3d's separable phase, conjugated), one sincos per point and workgroup, by the first
// wave; it multiplies conj(a3) once per row k (use_phase = 0: one product per element).
template <int TW>
__global__ __launch_bounds__(256) void pair34_kernel(Pair34Segs sg, int n3, int n4, long ld3,
                                                     long ld4, int ngrid, int n1, int n2, int n0,
                                                     double kd0, double kd1, double kd2,
                                                     int use_phase, cplx* __restrict__ B) {
  constexpr int MW = TW >= 16 ? TW / 2 : TW;
  constexpr int PL = TW | 1, PM = MW | 1;
  __shared__ cplx sl[kKfftGT * PL];
  __shared__ cplx sm[kKfftGT * PM];
  __shared__ cplx sp[kKfftGT];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long g0 = (long)blockIdx.x * kKfftGT;
  const int rows = (int)min((long)kKfftGT, ngrid - g0);
  // the pair of this k-tile (uniform; compile-time slots, so the struct stays in the arguments)
  const int z = blockIdx.z;
  const cplx* __restrict__ a3 = sg.a3[0];
  const cplx* __restrict__ a4 = sg.a4[0];
  int k0 = sg.k0[0], k1 = sg.k1[0], orow = sg.orow[0], t0 = sg.t0[0];
#pragma unroll
  for (int j = 1; j < kPair34Cap; ++j)
    if (z >= sg.t0[j]) {
      a3 = sg.a3[j], a4 = sg.a4[j];
      k0 = sg.k0[j], k1 = sg.k1[j], orow = sg.orow[j], t0 = sg.t0[j];
    }
  const int it0 = blockIdx.y * TW, ic = min(TW, n4 - it0);
  const int kt0 = k0 + (z - t0) * MW, kc = min(MW, k1 - kt0);
  if (tid < kKfftGT) {
    cplx ph = cmk(1, 0);
    if (use_phase && tid < rows) {
      const long g = g0 + tid;
      const int i2 = (int)(g % n2), i1 = (int)((g / n2) % n1), i0 = (int)(g / ((long)n1 * n2));
      const double th = eri_freq(i0, n0) * kd0 + eri_freq(i1, n1) * kd1 + eri_freq(i2, n2) * kd2;
      double sn, cs;
      sincos(th, &sn, &cs);
      ph = cmk(cs, sn);
    }
    sp[tid] = ph;
  }
  for (int e = tid; e < kKfftGT * TW; e += 256) {
    const int g = e / TW, c = e - g * TW;
    sl[g * PL + c] = g < rows && c < ic ? a4[(g0 + g) * ld4 + it0 + c] : cmk(0, 0);
  }
  for (int e = tid; e < kKfftGT * MW; e += 256) {
    const int g = e / MW, c = e - g * MW;
    sm[g * PM + c] = g < rows && c < kc ? a3[(g0 + g) * ld3 + kt0 + c] : cmk(0, 0);
  }
  __syncthreads();
  if (lane >= rows) return;
  const cplx ph = sp[lane];
  for (int ki = 0; ki < kc; ++ki) {
    cplx a = cconj(sm[lane * PM + ki]);
    if (use_phase) a = cmul(ph, a);
    cplx* row = B + ((long)(orow + kt0 - k0 + ki) * n4 + it0) * ngrid + g0 + lane;
    for (int ii = wv; ii < ic; ii += 4) row[(long)ii * ngrid] = cmul(a, sl[lane * PL + ii]);
  }
}

template <int TW>
int pair34_launch(hipStream_t st, const Pair34Segs& sg, int ktiles, int n3, int n4, long ld3,
                  long ld4, int ngrid, const int mesh[3], const double* kd, cplx* B) {
  const long gt = ((long)ngrid + kKfftGT - 1) / kKfftGT;
  const int it = (n4 + TW - 1) / TW;
  FISDF_CHECK(it <= 65535 && ktiles <= 65535, "pair34: too many tiles");
  hipLaunchKernelGGL(pair34_kernel<TW>, dim3((unsigned)gt, it, ktiles), dim3(256), 0, st, sg, n3, n4,
                     ld3, ld4, ngrid, mesh[1], mesh[2], mesh[0], kd ? kd[0] : 0.0,
                     kd ? kd[1] : 0.0, kd ? kd[2] : 0.0, kd ? 1 : 0, B);
  FISDF_HIP(hipGetLastError());
  return 0;
}

}  // namespace

int pair34(hipStream_t st, const cplx* const* a3, const cplx* const* a4, int npair, int n3, int n4,
           long ld3, long ld4, const int mesh[3], const double* kd, int r0, int r1, cplx* B) {
  FISDF_CHECK(a3 && a4 && mesh && B, "pair34: null pointer");
  FISDF_CHECK(npair >= 1 && n3 >= 1 && n4 >= 1, "pair34: sizes must be >= 1");
  FISDF_CHECK(n3 <= kKfftMaxNao && n4 <= kKfftMaxNao && npair <= kEriMaxPairs,
              "pair34: n3, n4 must be <= 32768 and npair <= 65535");
  FISDF_CHECK(ld3 >= n3 && ld4 >= n4, "pair34: leading dimension below the columns");
  FISDF_CHECK(mesh[0] >= 1 && mesh[1] >= 1 && mesh[2] >= 1, "pair34: bad mesh");
  const long ngl = (long)mesh[0] * mesh[1] * mesh[2];
  FISDF_CHECK(ngl < (1L << 31), "pair34: mesh too large");
  FISDF_CHECK(0 <= r0 && r0 < r1 && (long)r1 <= (long)npair * n3, "pair34: bad row range");
  const int p0 = r0 / n3, p1 = (r1 - 1) / n3;
  for (int p = p0; p <= p1; ++p) FISDF_CHECK(a3[p] && a4[p], "pair34: null pair pointer");
  const int tw = pair_density_variant(n4), mw = tw >= 16 ? tw / 2 : tw;
  // at most kPair34Cap pairs per launch
  for (int q0 = p0; q0 <= p1; q0 += kPair34Cap) {
    const int nq = std::min(kPair34Cap, p1 - q0 + 1);
    Pair34Segs sg;
    int tiles = 0;
    for (int j = 0; j < kPair34Cap; ++j) {
      const int p = q0 + std::min(j, nq - 1);
      sg.a3[j] = a3[p];
      sg.a4[j] = a4[p];
      sg.k0[j] = std::max(r0 - p * n3, 0);
      sg.k1[j] = (int)std::min<long>((long)r1 - (long)p * n3, n3);
      sg.orow[j] = p * n3 + sg.k0[j] - r0;
      sg.t0[j] = j < nq ? tiles : INT_MAX;
      if (j < nq) tiles += (sg.k1[j] - sg.k0[j] + mw - 1) / mw;
    }
    sg.t0[kPair34Cap] = INT_MAX;
    if (tw == 8)
      FISDF_TRY(pair34_launch<8>(st, sg, tiles, n3, n4, ld3, ld4, (int)ngl, mesh, kd, B));
    else
      FISDF_TRY(pair34_launch<32>(st, sg, tiles, n3, n4, ld3, ld4, (int)ngl, mesh, kd, B));
  }
  return 0;
}

int eri_gemm_ksplit(long n12, long n34, long ngrid) {
  const long tiles = ((n12 + 63) / 64) * ((n34 + 63) / 64);
  int ks = 1;
  while (tiles * ks < 512 && ngrid / (ks * 2) >= 256) ks *= 2;
  return ks;
}

void eri_fft_plan(int n1, int n2, int n3, int n4, int npair, long ngrid, long work_bytes,
                  EriFftPlan* p) {
  *p = EriFftPlan();
  // the size limits keep every product below inside a long
  if (n1 < 1 || n2 < 1 || n3 < 1 || n4 < 1 || n1 > kKfftMaxNao || n2 > kKfftMaxNao ||
      n3 > kKfftMaxNao || n4 > kKfftMaxNao || npair < 1 || npair > kEriMaxPairs || ngrid < 1 ||
      ngrid >= (1L << 31) || work_bytes < 0)
    return;
  const long budget = work_bytes ? work_bytes : kKfftWorkBytes;
  const long row12 = (long)sizeof(cplx) * n2 * ngrid;  // the transform rows of one row i
  const long row34 = (long)sizeof(cplx) * n4 * ngrid;  // the B rows of one row (p, k)
  p->tw = pair_density_variant(n4);
  p->ksplit = eri_gemm_ksplit((long)n1 * n2, (long)n3 * n4, ngrid);
  p->mc = (int)std::min<long>(n1, budget / row12);
  p->bc = (int)std::min<long>((long)npair * n3, budget / row34);
  if (p->mc < 1 || p->bc < 1) {
    p->mc = p->bc = 0;
    return;
  }
  p->nrow_chunks = (n1 + p->mc - 1) / p->mc;
  p->nb_chunks = (int)(((long)npair * n3 + p->bc - 1) / p->bc);
  p->b_once = p->nb_chunks == 1;
  auto al = [](long b) { return (b + 255) / 256 * 256; };
  p->off_rows = 0;
  p->off_b = p->off_rows + al(row12 * p->mc);
  p->off_w = p->off_b + al(row34 * p->bc);
  p->off_work = p->off_w + al((long)sizeof(double) * ngrid);
  // one GEMM per (B chunk, pair): at most mc n2 rows by min(bc, n3) n4 columns
  p->work_elems =
      p->ksplit > 1 ? (long)p->ksplit * p->mc * n2 * std::min(p->bc, n3) * n4 : 0;
  p->bytes = p->off_work + al((long)sizeof(cplx) * p->work_elems);
  p->ok = 1;
}

}  // namespace fisdf
