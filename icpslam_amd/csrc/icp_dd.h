// icp_dd.h -- double-double accumulation for the sums whose rule is "the EXACT sum rounded once" (the sums of a GICP evaluation,
// icp_gicp_device.h; the statistical outlier filter's sum and sq_sum, icp_outlier.hip; the plane refinement's nine sums,
// icp_sac.hip; the ISS scatter's six, icp_iss.hip): the high parts by TwoSum, the low parts in plain float64.
// (icp_gicp_quadratic.h's host-side DD has other operations -- split products, a renormalisation -- and its own namespace.)
#pragma once

#include <hip/hip_runtime.h>

namespace icpgpu {
namespace {

struct DD {
  double hi, lo;
};
__host__ __device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}
__host__ __device__ __forceinline__ void dd_add_term(DD& a, double t) {  // a += t, error-free in (hi, lo) up to lo's rounding
  double s, e;
  two_sum(a.hi, t, s, e);
  a.hi = s;
  a.lo += e;
}
__host__ __device__ __forceinline__ DD dd_add(const DD& a, const DD& b) {
  // cascaded: the high parts by TwoSum (error-free), everything small in plain float64 -- the low part stays ~1e-16 of the
  // running magnitudes, so its own rounding is ~1e-32 of them (the accurate double-double addition with two
  // renormalisations costs three times as much and buys nothing here)
  DD r;
  double e;
  two_sum(a.hi, b.hi, r.hi, e);
  r.lo = (a.lo + b.lo) + e;
  return r;
}

}  // namespace
}  // namespace icpgpu
