// icp_exp.h -- exp(a) for a <= 0 in float64 by plain IEEE operations: ONE definition for the moving least squares weights on the
// device (icp_mls.hip: mls_fit_kernel) and on the host.  No libm exp and no fused multiply-add (the tree builds with
// -ffp-contract=off), so its expressions are part of that rule (include/icpgpu.h "moving least squares", EXP_NEG):
// tests/mls_restated.py (exp_neg) takes the same steps and gets the same bits.  rint and ldexp are exact operations.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

namespace icpgpu {

// NaN stays NaN; a < -708 gives 0 (the result stays a normal number above that).  Otherwise a = k ln2 + r with |r| <= ln2 / 2 (ln2 in
// two parts: k times the first is exact), exp(r) by its Taylor polynomial of degree 13 in Horner form, the coefficients the doubles
// nearest 1 / n!, and the result scaled by 2^k.  Within 1 ulp of a correctly rounded exp on [-708, 0] (tests/test_mls_host.py).
__host__ __device__ __forceinline__ double exp_neg(double a) {
  if (a != a) return a;
  if (a < -708.0) return 0.0;
  const double k = rint(a * 0x1.71547652b82fep+0);
  const double r = (a - k * 0x1.62e42feep-1) - k * 0x1.a39ef35793c76p-33;
  double p = 0x1.6124613a86d09p-33;  // 1 / 13!
  p = p * r + 0x1.1eed8eff8d898p-29;
  p = p * r + 0x1.ae64567f544e4p-26;
  p = p * r + 0x1.27e4fb7789f5cp-22;
  p = p * r + 0x1.71de3a556c734p-19;
  p = p * r + 0x1.a01a01a01a01ap-16;
  p = p * r + 0x1.a01a01a01a01ap-13;
  p = p * r + 0x1.6c16c16c16c17p-10;
  p = p * r + 0x1.1111111111111p-7;
  p = p * r + 0x1.5555555555555p-5;
  p = p * r + 0x1.5555555555555p-3;
  p = p * r + 0x1.0000000000000p-1;
  p = p * r + 1.0;
  p = p * r + 1.0;
  return ldexp(p, (int)k);
}

}  // namespace icpgpu
