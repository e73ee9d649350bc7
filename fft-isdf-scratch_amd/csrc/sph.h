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

}  // namespace fisdf
