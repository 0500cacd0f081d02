// icp_angle.h -- the folded angle of the segmentation from normals (include/icpgpu.h "segmentation from normals", THE ANGLE): the
// angle in [0, pi/2] between two directions m and g from y = |m x g| and x = |m . g|, both float32 and not negative -- atan2(y, x)
// without a libm call, so that the device, the host and tests/sac_normals_restated.py compute the same bits.  Plain float32 IEEE
// operations and explicit fused multiply-adds only (the unit is built with -ffp-contract=off): one division for the range
// reduction, then a fixed polynomial.
//     y == 0 (x == 0 included: a zero direction)    0
//     y <= x    t = y / x,  angle = P(t)
//     y >  x    t = x / y,  angle = ANGLE_HALF_PI - P(t)       (x == 0: t = 0, P = 0: exactly the float32 image of pi / 2)
//     P(t) = fmaf(t * s, R(s), t),  s = t * t,  R by Horner's rule with fmaf from ANGLE_C[8] down to ANGLE_C[0]
// A NaN argument gives NaN, and so does inf / inf.  The coefficients are a least-squares fit of (atan(t) / t - 1) / s on [0, 1]
// rounded to float32; the polynomial itself is within 5.5e-9 of atan, the rest of the error is float32 rounding.
// Bound: |angle - atan2(y, x)| <= 2^-22 (2 ulp of pi / 2) for finite arguments that are not both 0 --
// tests/test_sac_normals_host.py asserts it over a dense sweep (measured there: 1.56e-7, 1.31 ulp of pi / 2).
#pragma once

#ifndef __host__
#define __host__
#define __device__
#endif

namespace icpgpu {

constexpr float ANGLE_HALF_PI = 1.57079637050628662109375f;  // the float32 image of pi / 2
constexpr float ANGLE_C[9] = {-0x1.55551ep-2f, 0x1.998bbcp-3f, -0x1.23e71cp-3f, 0x1.be6df6p-4f, -0x1.525702p-4f,
                              0x1.c7f87cp-5f,  -0x1.db5118p-6f, 0x1.414704p-7f, -0x1.97ba58p-10f};

__host__ __device__ inline float angle_poly(float t) {
  const float s = t * t;
  float r = ANGLE_C[8];
  r = __builtin_fmaf(r, s, ANGLE_C[7]);
  r = __builtin_fmaf(r, s, ANGLE_C[6]);
  r = __builtin_fmaf(r, s, ANGLE_C[5]);
  r = __builtin_fmaf(r, s, ANGLE_C[4]);
  r = __builtin_fmaf(r, s, ANGLE_C[3]);
  r = __builtin_fmaf(r, s, ANGLE_C[2]);
  r = __builtin_fmaf(r, s, ANGLE_C[1]);
  r = __builtin_fmaf(r, s, ANGLE_C[0]);
  return __builtin_fmaf(t * s, r, t);
}

// y = |m x g| >= 0, x = |m . g| >= 0
__host__ __device__ inline float folded_angle(float y, float x) {
  if (y == 0.f) return 0.f;
  if (y <= x) return angle_poly(y / x);
  if (y > x) return ANGLE_HALF_PI - angle_poly(x / y);
  return y + x;  // (a NaN argument)
}

}  // namespace icpgpu
