// icp_boundary.hip -- pcl::BoundaryEstimation: which points lie on a surface's rim, from the neighbour rows of the search cloud and
// the queries' normals (rules: include/icpgpu.h "boundary estimation"; host: icpgpu_boundary.cpp; ISS's border estimation calls the
// same kernel from icpgpu_iss.cpp).
//
// The rows are the neighbour search's (icp_search.hip), still in device memory, read as normals_from_rows_kernel reads them: dense
// rows of stride k with n_found, or CSR rows with row_start.  boundary_from_rows_kernel gives a query a wave:
//   * every lane builds the tangent frame (u, v) from the query's normal -- the same few float32 operations in all 64 lanes;
//   * the row is cut into tiles of 64 entries.  A lane turns its entry of a tile into a direction (x, y) = (u . d, v . d); a skipped
//     entry (a coincident point, a non-finite or zero projection) becomes (NaN, NaN), which lies in no sector and owns none;
//   * for a tile of candidates a -- a lane each, carrying xa, ya and c2 * na in float64 -- the wave streams the row's tiles of b past
//     them: the b's of a tile are handed round by lane reads (v_readlane with a wave-uniform lane number; no LDS, so no fence
//     between the lanes and no limit on occupancy from it), and the sector test of the header runs in float64 on exact products;
//   * a lane's a dies at the first b in its sector, and -- once a survivor is known -- so does every a whose cloud index is not
//     below the survivor's: it cannot lower the witness.  The wave leaves a pass, wave-uniformly, when no a is alive;
//   * the witness is a wave minimum over the survivors' cloud indices.
// An interior point costs a fraction of m^2 pair tests, a boundary point m^2 for its survivors only.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include "icp_device.h"
#include "icp_grid_device.h"
#include "icp_kernels.h"

namespace icpgpu {
namespace {

constexpr int BD_BLOCK = 256, BD_WAVES = BD_BLOCK / 64;

__device__ __forceinline__ float lane_float(float v, int lane) {  // (lane: wave-uniform)
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// b in a's sector: the counter-clockwise angle from a to b lies in (0, theta]; cneg: cos(theta) < 0.  Every product is exact in
// float64 (24 x 24 bits), every sum rounded once (-ffp-contract=off).
__device__ __forceinline__ bool in_sector(double xa, double ya, double c2na, double xb, double yb, bool cneg) {
  const double cr = xa * yb - ya * xb;
  const double dt = xa * xb + ya * yb;
  const double nb = xb * xb + yb * yb;
  const double lhs = dt * dt, rhs = c2na * nb;
  const bool cone = cneg ? (dt >= 0.0 || lhs <= rhs) : (dt >= 0.0 && lhs >= rhs);
  return cr >= 0.0 && !(cr == 0.0 && dt > 0.0) && cone;  // (a NaN fails cr >= 0)
}

// rows: n_found != null: row i = idx[i * k, i * k + n_found[i]); else row i = idx[row_start[i], row_start[i + 1]).
// A row counts when it has at least min_row entries (>= 3).  boundary (bytes) and flag32 (ints) receive the same 0 / 1; each of the
// four outputs may be null.
__global__ __launch_bounds__(BD_BLOCK) void boundary_from_rows_kernel(const float4* __restrict__ queries, int n_q, const float4* __restrict__ normals,
                                                                      const float4* __restrict__ cloud, int n, const int32_t* __restrict__ idx,
                                                                      const int32_t* __restrict__ n_found, int k, const int* __restrict__ row_start,
                                                                      int min_row, double c2, int cneg, uint8_t* __restrict__ boundary,
                                                                      int32_t* __restrict__ flag32, int32_t* __restrict__ n_directions,
                                                                      int32_t* __restrict__ witness) {
  const int lane = (int)(threadIdx.x & 63u);
  const int i = blockIdx.x * BD_WAVES + (int)(threadIdx.x >> 6);
  if (i >= n_q) return;  // (wave-uniform)
  size_t base;
  int m;
  if (n_found) {
    base = (size_t)i * (size_t)k;
    m = min(n_found[i], k);
  } else {
    base = (size_t)row_start[i];
    m = row_start[i + 1] - row_start[i];
  }
  m = __builtin_amdgcn_readfirstlane(m);
  const float4 p = queries[i];
  int n_dir = 0, wit = INT_MAX;
  if (m >= min_row && n > 0 && finite3(p.x, p.y, p.z)) {  // (wave-uniform)
    // the frame: PCL's getCoordinateSystemOnPlane with Eigen's unitOrthogonal, float32, every operation rounded on its own
    const float4 nn = normals[i];
    const float nx = nn.x, ny = nn.y, nz = nn.z;
    const float lim = 1e-5f * fabsf(nz);
    const bool near = fabsf(nx) <= lim && fabsf(ny) <= lim;
    float vx, vy, vz;
    if (!near) {
      const float inv = 1.f / sqrtf(nx * nx + ny * ny);
      vx = -ny * inv, vy = nx * inv, vz = 0.f;
    } else {
      const float inv = 1.f / sqrtf(ny * ny + nz * nz);
      vx = 0.f, vy = -nz * inv, vz = ny * inv;
    }
    const float ux = ny * vz - nz * vy, uy = nz * vx - nx * vz, uz = nx * vy - ny * vx;
    const float nan = __builtin_nanf("");
    // entry t of the row -> its direction and cloud index; (NaN, NaN) for a skipped entry and beyond the row's end
    auto direction = [&](int t, float& x, float& y, int& j) {
      x = y = nan;
      j = INT_MAX;
      if (t < m) {
        j = min(max(idx[base + (size_t)t], 0), n - 1);  // (a row names cloud points)
        const float4 q = cloud[j];
        const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
        const float xx = (ux * dx + uy * dy) + uz * dz, yy = (vx * dx + vy * dy) + vz * dz;
        const bool skip = (dx == 0.f && dy == 0.f && dz == 0.f) || !isfinite(xx) || !isfinite(yy) || (xx == 0.f && yy == 0.f);
        if (!skip) x = xx, y = yy;
      }
    };
    for (int a0 = 0; a0 < m; a0 += 64) {
      float fxa, fya;
      int ja;
      direction(a0 + lane, fxa, fya, ja);
      bool alive = fxa == fxa;  // (not a skipped entry)
      n_dir += __popcll(__ballot(alive));
      alive = alive && ja < wit;
      const double xa = (double)fxa, ya = (double)fya;
      const double c2na = c2 * (xa * xa + ya * ya);
      for (int b0 = 0; b0 < m && __ballot(alive) != 0ull; b0 += 64) {
        float fxb = fxa, fyb = fya;
        if (b0 != a0) {  // (wave-uniform)
          int jb;
          direction(b0 + lane, fxb, fyb, jb);
        }
        const int cnt = min(64, m - b0);
        for (int t = 0; t < cnt; ++t) {
          const double xb = (double)lane_float(fxb, t), yb = (double)lane_float(fyb, t);
          if (alive && in_sector(xa, ya, c2na, xb, yb, cneg != 0)) alive = false;
          if (__ballot(alive) == 0ull) break;  // (wave-uniform)
        }
      }
      int w = alive ? ja : INT_MAX;  // the survivors' lowest cloud index
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) w = min(w, __shfl_xor(w, s, 64));
      wit = min(wit, w);
    }
  }
  if (lane != 0) return;
  const int flag = wit != INT_MAX ? 1 : 0;
  if (boundary) boundary[i] = (uint8_t)flag;
  if (flag32) flag32[i] = flag;
  if (n_directions) n_directions[i] = n_dir;
  if (witness) witness[i] = flag ? wit : -1;
}

}  // namespace

hipError_t launch_boundary_from_rows(const float4* queries, int n_q, const float4* normals, const float4* cloud, int n, const int32_t* idx,
                                     const int32_t* n_found, int k, const int* row_start, int min_row, double cos_threshold, uint8_t* boundary,
                                     int32_t* flag32, int32_t* n_directions, int32_t* witness, hipStream_t stream) {
  if (n_q <= 0) return hipSuccess;
  if ((n_found == nullptr) == (row_start == nullptr)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(boundary_from_rows_kernel, dim3((n_q + BD_WAVES - 1) / BD_WAVES), dim3(BD_BLOCK), 0, stream, queries, n_q, normals, cloud, n, idx,
                     n_found, k, row_start, min_row < 3 ? 3 : min_row, cos_threshold * cos_threshold, cos_threshold < 0.0 ? 1 : 0, boundary, flag32,
                     n_directions, witness);
  return hipGetLastError();
}

}  // namespace icpgpu
