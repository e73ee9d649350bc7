// The spin-unpolarised exchange-correlation functional at the grid points of a block: Slater
// exchange + PW92 correlation (libxc's "pw_mod" parameters) for LDA, PBE for GGA, the exchange
// and correlation parts scaled by cx and cc.  Inputs n = Re rho_0 and d_c n = Re rho_c from the
// complex layout of fisdf_get_rho / fisdf_get_rho_gga; outputs the energy per volume e and
// wv = [de/dn, 2 de/dsigma d_c n], the unweighted wv of fisdf_gga_gram.  FP64 throughout,
// analytic derivatives.  Everything is written in s^2, t^2 and y = A t^2: sigma = 0 is no special
// case and nothing divides by sigma.  The PBE correlation uses
//   eps + H = gamma log1p(-q / D),  q = -expm1(eps / gamma),  D = 1 + y + y^2,
// which is gamma ln(1 + (beta/gamma) t^2 (1 + y) / D) + eps with the two logarithms combined
// (1 + E = 1 / (1 - q), E = expm1(-eps / gamma)): nothing cancels where eps + H -> 0.  Where
// q / D > 1/2 the same number is gamma (log(D - q) - log(D)), D - q = y + y^2 + exp(eps / gamma).
// The optional per-workgroup sums of n and e are reduced in a fixed order; no atomics.
#include "common.h"
#include "linalg.h"

#include <cmath>

namespace fisdf {

namespace {

constexpr int kXcThreads = 256;

constexpr double kPi = 3.14159265358979323846264338327950288;
constexpr double kCx = 0.73855876638202240588;      // (3/4) (3/pi)^(1/3)
constexpr double kRs0 = 0.62035049089940001667;     // (3/(4 pi))^(1/3)
constexpr double kKf0 = 3.09366772628013593097;     // (3 pi^2)^(1/3)
constexpr double kPwA = 0.03109069086965489503;     // (1 - ln 2) / pi^2
constexpr double kPwA1 = 0.21370;
constexpr double kPwB1 = 7.5957, kPwB2 = 3.5876, kPwB3 = 1.6382, kPwB4 = 0.49294;
constexpr double kKappa = 0.804;
constexpr double kBeta = 0.06672455060314922;
constexpr double kGamma = kPwA;
constexpr double kMu = kBeta * kPi * kPi / 3.0;

// eps_c^unif(rs) and its derivative with respect to rs
__device__ inline void pw92(double rs, double& eps, double& deps) {
  const double sr = sqrt(rs);
  const double q0 = -2.0 * kPwA * (1.0 + kPwA1 * rs);
  const double q1 = 2.0 * kPwA * (sr * (kPwB1 + sr * (kPwB2 + sr * (kPwB3 + sr * kPwB4))));
  const double dq1 = kPwA * (kPwB1 / sr + 2.0 * kPwB2 + sr * (3.0 * kPwB3 + 4.0 * kPwB4 * sr));
  const double lg = log1p(1.0 / q1);
  eps = q0 * lg;
  deps = -2.0 * kPwA * kPwA1 * lg - q0 * dq1 / (q1 * q1 + q1);
}

// e, de/dn and de/dsigma at a point with n above the cut
template <bool GGA>
__device__ inline void xc_point(double n, double sigma, double cx, double cc, double& e,
                                double& vn, double& vs) {
  const double c = cbrt(n);
  [[maybe_unused]] const double kf = kKf0 * c;   // the GGA parts only
  e = vn = vs = 0.0;
  if (cx != 0.0) {
    const double ex = -kCx * n * c;               // e_x^LDA
    const double dex = -(4.0 / 3.0) * kCx * c;    // its derivative
    if constexpr (GGA) {
      const double cs = 1.0 / (4.0 * kf * kf * n * n);   // d s^2 / d sigma
      const double s2 = sigma * cs;
      const double den = 1.0 + (kMu / kKappa) * s2;
      const double fx = 1.0 + kMu * s2 / den;
      const double dfx = kMu / (den * den);
      e += cx * ex * fx;
      vn += cx * dex * (fx - 2.0 * s2 * dfx);
      vs += cx * ex * dfx * cs;
    } else {
      e += cx * ex;
      vn += cx * dex;
    }
  }
  if (cc != 0.0) {
    const double rs = kRs0 / c;
    double eps, deps;
    pw92(rs, eps, deps);
    const double neps_n = -(rs / 3.0) * deps;     // n d eps / d n
    if constexpr (GGA) {
      const double nct = kPi / (16.0 * kf * n);   // n d t^2 / d sigma
      const double t2 = sigma * (nct / n);
      const double q = -expm1(eps / kGamma);      // E / (1 + E), in (0, 1)
      const double p = exp(eps / kGamma);         // 1 - q, without the cancellation at high n
      const double A = (kBeta / kGamma) * p / q;
      const double dA = A * A / (kBeta * p);              // d A / d eps
      const double y = A * t2;
      const double yy = y + y * y, D = 1.0 + yy;
      const double u = 1.0 / D, r = 1.0 / (yy + p);       // 1 / (D - q)
      // eps + H.  q / D <= 1/2: log1p of it; else (high density, small y) the two logarithms
      // apart: log(p) = eps / gamma at y = 0, and nothing cancels while the result is below
      // log(1/2)
      const double z = q * u;
      const double W = kGamma * (z <= 0.5 ? log1p(-z) : log(yy + p) - log1p(yy));
      const double We = p * r;                            // dW/d eps at fixed y
      const double Wy = kGamma * q * ((1.0 + 2.0 * y) * u) * r;
      e += cc * n * W;
      vn += cc * (W + We * neps_n + Wy * (t2 * dA * neps_n - (7.0 / 3.0) * y));
      vs += cc * nct * A * Wy;
    } else {
      e += cc * n * eps;
      vn += cc * (eps + neps_n);
    }
  }
}

// one point per thread, blockIdx.y the set.  part (optional): part[(s nblk + b) 2 + {0, 1}] the
// workgroup's sums of n and e over the points above the cut, by a tree in LDS
template <bool GGA>
__global__ __launch_bounds__(kXcThreads) void xc_kernel(const cplx* __restrict__ rho, long rss,
                                                        long rcs, int ng, double cx, double cc,
                                                        double cut, double* __restrict__ e,
                                                        long ess, double* __restrict__ wv, long wss,
                                                        long wcs, double* __restrict__ part) {
  __shared__ double red[2][kXcThreads];
  const int s = blockIdx.y, tid = threadIdx.x;
  const long g = (long)blockIdx.x * kXcThreads + tid;
  double nn = 0.0, ee = 0.0;
  if (g < ng) {
    const cplx* p = rho + s * rss + g;
    const double n = p[0].x;
    double gx = 0.0, gy = 0.0, gz = 0.0, vn = 0.0, vs = 0.0;
    if (n > cut) {   // false for NaN as well
      if constexpr (GGA) {
        gx = p[rcs].x;
        gy = p[2 * rcs].x;
        gz = p[3 * rcs].x;
      }
      xc_point<GGA>(n, gx * gx + gy * gy + gz * gz, cx, cc, ee, vn, vs);
      nn = n;
    }
    if (e) e[s * ess + g] = ee;
    if (wv) {
      double* w = wv + s * wss + g;
      w[0] = vn;
      if constexpr (GGA) {
        const double v2 = 2.0 * vs;
        w[wcs] = v2 * gx;
        w[2 * wcs] = v2 * gy;
        w[3 * wcs] = v2 * gz;
      }
    }
  }
  if (!part) return;
  red[0][tid] = nn;
  red[1][tid] = ee;
  __syncthreads();
  for (int h = kXcThreads / 2; h > 0; h >>= 1) {
    if (tid < h) {
      red[0][tid] += red[0][tid + h];
      red[1][tid] += red[1][tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* o = part + ((long)s * gridDim.x + blockIdx.x) * 2;
    o[0] = red[0][0];
    o[1] = red[1][0];
  }
}

// sums[s][j] (+)= scale sum_b part[s][b][j]: thread t adds blocks t, t + 256, ... in order, then
// the tree; one workgroup per set
__global__ __launch_bounds__(kXcThreads) void xc_sums_kernel(const double* __restrict__ part,
                                                             int nblk, double scale, int accumulate,
                                                             double* __restrict__ sums) {
  __shared__ double red[2][kXcThreads];
  const int s = blockIdx.x, tid = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int i = tid; i < nblk; i += kXcThreads) {
    a += part[((long)s * nblk + i) * 2];
    b += part[((long)s * nblk + i) * 2 + 1];
  }
  red[0][tid] = a;
  red[1][tid] = b;
  __syncthreads();
  for (int h = kXcThreads / 2; h > 0; h >>= 1) {
    if (tid < h) {
      red[0][tid] += red[0][tid + h];
      red[1][tid] += red[1][tid + h];
    }
    __syncthreads();
  }
  if (tid < 2) {
    const double v = scale * red[tid][0];
    sums[s * 2 + tid] = accumulate ? sums[s * 2 + tid] + v : v;
  }
}

}  // namespace

int xc_blocks(int ng) { return (ng + kXcThreads - 1) / kXcThreads; }

int xc_check(int family, double cx, double cc, double rho_cut, int ng, int nset, long rss, long rcs,
             long ess, long wss, long wcs, bool has_e, bool has_wv) {
  FISDF_CHECK(family == 0 || family == 1, "xc_eval: unknown family (0 LDA, 1 GGA)");
  FISDF_CHECK(ng >= 1 && nset >= 1, "xc_eval: sizes must be >= 1");
  FISDF_CHECK(nset <= 65535, "xc_eval: too many sets");
  FISDF_CHECK(std::isfinite(cx) && std::isfinite(cc), "xc_eval: cx and cc must be finite");
  FISDF_CHECK(rho_cut >= 0.0, "xc_eval: rho_cut must be >= 0 (and not NaN)");
  if (family == 1) {
    FISDF_CHECK(rcs >= ng && rss >= 3 * rcs + ng, "xc_eval: a stride of rho below its minimum");
    FISDF_CHECK(!has_wv || (wcs >= ng && wss >= 3 * wcs + ng),
                "xc_eval: a stride of wv below its minimum");
  } else {
    FISDF_CHECK(rss >= ng, "xc_eval: rho_sstride below ng");
    FISDF_CHECK(!has_wv || wss >= ng, "xc_eval: w_sstride below ng");
  }
  FISDF_CHECK(!has_e || ess >= ng, "xc_eval: e_sstride below ng");
  return 0;
}

int xc_eval(hipStream_t st, int family, double cx, double cc, double rho_cut, const cplx* rho,
            long rss, long rcs, int ng, int nset, double* e, long ess, double* wv, long wss,
            long wcs, double* part) {
  FISDF_CHECK(rho != nullptr, "xc_eval: null rho");
  FISDF_TRY(xc_check(family, cx, cc, rho_cut, ng, nset, rss, rcs, ess, wss, wcs, e != nullptr,
                     wv != nullptr));
  if (!e && !wv && !part) return 0;
  const dim3 grid((unsigned)xc_blocks(ng), (unsigned)nset);
  if (family == 1)
    hipLaunchKernelGGL(xc_kernel<true>, grid, dim3(kXcThreads), 0, st, rho, rss, rcs, ng, cx, cc,
                       rho_cut, e, ess, wv, wss, wcs, part);
  else
    hipLaunchKernelGGL(xc_kernel<false>, grid, dim3(kXcThreads), 0, st, rho, rss, rcs, ng, cx, cc,
                       rho_cut, e, ess, wv, wss, wcs, part);
  FISDF_HIP(hipGetLastError());
  return 0;
}

int xc_sums(hipStream_t st, const double* part, int nblk, int nset, double scale, int accumulate,
            double* sums) {
  hipLaunchKernelGGL(xc_sums_kernel, dim3((unsigned)nset), dim3(kXcThreads), 0, st, part, nblk,
                     scale, accumulate, sums);
  FISDF_HIP(hipGetLastError());
  return 0;
}

}  // namespace fisdf
