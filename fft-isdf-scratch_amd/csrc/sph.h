// The real solid harmonics of the Bloch AO evaluator (ao.hip) and of the GTH projectors (pp.hip).
#pragma once
#include "common.h"

namespace fisdf {

// real solid harmonics r^l Y_lm, cell.py::_real_sph order and constants
__device__ __forceinline__ double real_sph(int l, int m, double x, double y, double z) {
  if (l == 0) return 0.28209479177387814;
  if (l == 1) return 0.4886025119029199 * (m == 0 ? x : (m == 1 ? y : z));
  const double r2 = x * x + y * y + z * z;
  if (l == 2) {
    switch (m) {
      case 0: return 1.0925484305920792 * x * y;
      case 1: return 1.0925484305920792 * y * z;
      case 2: return 0.31539156525252005 * (3 * z * z - r2);
      case 3: return 1.0925484305920792 * x * z;
      default: return 0.5462742152960396 * (x * x - y * y);
    }
  }
  switch (m) {  // l == 3
    case 0: return 0.5900435899266435 * y * (3 * x * x - y * y);
    case 1: return 2.890611442640554 * x * y * z;
    case 2: return 0.4570457994644658 * y * (5 * z * z - r2);
    case 3: return 0.3731763325901154 * z * (5 * z * z - 3 * r2);
    case 4: return 0.4570457994644658 * x * (5 * z * z - r2);
    case 5: return 1.445305721320277 * z * (x * x - y * y);
    default: return 0.5900435899266435 * x * (x * x - 3 * y * y);
  }
}

// gradient of real_sph(l, m, .): polynomials of degree l - 1, no division by r (the p gradients
// are constants, the d and f gradients vanish at the origin)
__device__ __forceinline__ void real_sph_grad(int l, int m, double x, double y, double z,
                                              double& gx, double& gy, double& gz) {
  gx = gy = gz = 0.0;
  if (l == 0) return;
  if (l == 1) {
    const double c = 0.4886025119029199;
    if (m == 0) gx = c;
    else if (m == 1) gy = c;
    else gz = c;
    return;
  }
  if (l == 2) {
    const double c = 1.0925484305920792, c2 = 0.31539156525252005, c4 = 0.5462742152960396;
    switch (m) {
      case 0: gx = c * y; gy = c * x; return;
      case 1: gy = c * z; gz = c * y; return;
      case 2: gx = c2 * (-2 * x); gy = c2 * (-2 * y); gz = c2 * (4 * z); return;
      case 3: gx = c * z; gz = c * x; return;
      default: gx = c4 * (2 * x); gy = c4 * (-2 * y); return;
    }
  }
  const double xx = x * x, yy = y * y, zz = z * z;  // l == 3
  const double a = 0.5900435899266435, b = 2.890611442640554, c = 0.4570457994644658,
               d = 0.3731763325901154, e = 1.445305721320277;
  switch (m) {
    case 0: gx = a * (6 * x * y); gy = a * (3 * xx - 3 * yy); return;
    case 1: gx = b * (y * z); gy = b * (x * z); gz = b * (x * y); return;
    case 2: gx = c * (-2 * x * y); gy = c * (4 * zz - xx - 3 * yy); gz = c * (8 * y * z); return;
    case 3:
      gx = d * (-6 * x * z); gy = d * (-6 * y * z); gz = d * (6 * zz - 3 * xx - 3 * yy);
      return;
    case 4: gx = c * (4 * zz - 3 * xx - yy); gy = c * (-2 * x * y); gz = c * (8 * x * z); return;
    case 5: gx = e * (2 * x * z); gy = e * (-2 * y * z); gz = e * (xx - yy); return;
    default: gx = a * (3 * xx - 3 * yy); gy = a * (-6 * x * y); return;
  }
}

}  // namespace fisdf
