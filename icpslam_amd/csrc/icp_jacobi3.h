// icp_jacobi3.h -- the cyclic Jacobi eigen-decomposition of a symmetric 3x3 in float64: ONE definition for the NDT cells
// (icp_ndt.hip: ndt_cell_kernel), the surface normals (icp_normals.hip: normals_from_rows_kernel), the ISS scatter matrices
// (icp_iss.hip: iss_scatter_kernel) and, on the host, the plane refinement (icpgpu_sac.cpp).  Its expressions are part of
// those rules: tests/ndt_restated.py (_jacobi3) and tests/normals_restated.py (jacobi3) run the same sweeps with the same expressions.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#include "icp_kernels.h"

namespace icpgpu {

// Cyclic Jacobi on a symmetric 3x3 (a[i][j], double): on return a's diagonal holds the eigenvalues, v's columns the eigenvectors.
// A rotation is skipped when its off-diagonal entry is exactly zero (an axis-aligned degenerate cell keeps exact zeros).  The
// NumPy restatement (tests/ndt_restated.py) runs the same sweeps with the same expressions.
__host__ __device__ __forceinline__ void jacobi3(double (&a)[3][3], double (&v)[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kNdtJacobiSweeps; ++sweep) {
#pragma unroll
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      const double apq = a[p][q];
      if (apq == 0.0) continue;
      const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
      const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
      const int r = 3 - p - q;
      const double arp = a[r][p], arq = a[r][q];
      a[p][p] = a[p][p] - t * apq;
      a[q][q] = a[q][q] + t * apq;
      a[p][q] = a[q][p] = 0.0;
      a[r][p] = a[p][r] = c * arp - s * arq;
      a[r][q] = a[q][r] = s * arp + c * arq;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double vkp = v[k][p], vkq = v[k][q];
        v[k][p] = c * vkp - s * vkq;
        v[k][q] = s * vkp + c * vkq;
      }
    }
  }
}

}  // namespace icpgpu
