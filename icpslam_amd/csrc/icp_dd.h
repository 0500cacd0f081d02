// icp_dd.h -- double-double accumulation for the sums whose rule is "the EXACT sum rounded once" (the statistical outlier filter's sum
// and sq_sum, icp_outlier.hip; the plane refinement's nine sums, icp_sac.hip; the ISS scatter's six, icp_iss.hip): the high parts by TwoSum, the low parts in plain
// float64, as icp_gicp.hip has it.
#pragma once

#include <hip/hip_runtime.h>

namespace icpgpu {

struct DD {
  double hi, lo;
};
__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}
__device__ __forceinline__ void dd_add_term(DD& a, double t) {
  double s, e;
  two_sum(a.hi, t, s, e);
  a.hi = s;
  a.lo += e;
}
__device__ __forceinline__ DD dd_add(const DD& a, const DD& b) {
  DD r;
  double e;
  two_sum(a.hi, b.hi, r.hi, e);
  r.lo = (a.lo + b.lo) + e;
  return r;
}

}  // namespace icpgpu
