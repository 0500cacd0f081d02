// icp_morph.hip -- the ground filter's kernels (pcl::applyMorphologicalOperator, pcl::ProgressiveMorphologicalFilter; rules:
// include/icpgpu.h "ground filter"; host side: icpgpu_pmf.cpp; design and what was not built: DESIGN.md section 5).
//
// The hot path is "the extremum of a value array over every active point's xy box".  PCL answers it with a box query per point and
// pass; here the active points are binned per pass into a 2-D cell table of side window / 8 (counting sort, cell-row-major, so the
// cells a box spans in one cell row are ONE contiguous run of points) and every cell keeps its extremum as an ordered integer key.
// A WAVE then takes one point: its lanes read the extremum of the cells strictly inside the box's cell range -- whole cells, no point
// is looked at -- and test the points of the rim's cells with the rule's four comparisons.  cell() is monotone non-decreasing in the
// coordinate and is the same function for binning and for the box's bounds, so (lo <= q <= hi per axis) implies cell(lo) <= cell(q)
// <= cell(hi), and cell(lo) < cell(q) < cell(hi) implies lo < q < hi: the interior cells hold members only, everything else that
// can be a member sits in the rim.  The extremum is order-free, so no step depends on the order atomics arrive in.
//
// Extrema are taken on k'(v) = key(v) for a maximum and ~key(v) for a minimum, key = the float's bits with the sign flipped
// (negatives: all bits), so that one unsigned max serves both and 0 -- below every finite float's k' -- means "nothing yet".
#include <hip/hip_runtime.h>

#include "icp_kernels.h"

namespace icpgpu {
namespace {

__device__ __forceinline__ unsigned int morph_key(float v) {
  const unsigned int b = __float_as_uint(v);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float morph_value(unsigned int k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ __forceinline__ unsigned int morph_ordered(float v, bool is_max) { return is_max ? morph_key(v) : ~morph_key(v); }
__device__ __forceinline__ float morph_unordered(unsigned int k, bool is_max) { return morph_value(is_max ? k : ~k); }

// the cell of coordinate x along an axis of n cells: monotone non-decreasing in x (a subtraction, a product with a constant >= 0, a
// truncation and a clamp are), total (a NaN product -- inf * 0 in a one-cell grid -- lands in cell 0 like everything else there)
__device__ __forceinline__ int morph_cell(float x, float o, float inv, int n) {
  const float t = (x - o) * inv;
  if (!(t > 0.f)) return 0;
  if (t >= (float)(n - 1)) return n - 1;
  return (int)t;
}

__device__ __forceinline__ unsigned int wave_max(unsigned int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned int o = (unsigned int)__shfl_xor((int)v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(256) void morph_init_kernel(const float4* __restrict__ cloud, int n, int* __restrict__ flags, int32_t* __restrict__ removed_at,
                                                         float* __restrict__ out_z, unsigned int* __restrict__ bbox4) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  unsigned int k[4] = {0u, 0u, 0u, 0u};  // ~key(x), ~key(y), key(x), key(y): maxima of these are the box
  if (i < n) {
    const float4 p = cloud[i];
    const bool fin = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
    flags[i] = fin ? 1 : 0;
    if (removed_at) removed_at[i] = fin ? -1 : -2;
    if (out_z) out_z[i] = p.z;
    if (fin) k[0] = ~morph_key(p.x), k[1] = ~morph_key(p.y), k[2] = morph_key(p.x), k[3] = morph_key(p.y);
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {  // one atomic per wave and bound
    const unsigned int m = wave_max(k[a]);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(&bbox4[a], m);
  }
}

__global__ void morph_grid_kernel(const unsigned int* __restrict__ bbox4, float window, MorphGrid* __restrict__ grid) {
  MorphGrid g;
  g.ox = g.oy = g.inv = 0.f;
  g.nx = g.ny = 1;  // (no finite point, or a box no cell side can be derived from: one cell, every point a rim point)
  if (bbox4[2]) {
    const float x0 = morph_value(~bbox4[0]), y0 = morph_value(~bbox4[1]), x1 = morph_value(bbox4[2]), y1 = morph_value(bbox4[3]);
    const float ex = x1 - x0, ey = y1 - y0, ext = ex > ey ? ex : ey;
    float side = window / (float)kMorphCellsPerWindow;
    const float cap_side = ext / (float)kMorphAxisCells;
    if (cap_side > side) side = cap_side;
    const float inv = 1.f / side;
    if (inv > 0.f && isfinite(inv)) {
      g.ox = x0, g.oy = y0, g.inv = inv;
      const float tx = ex * inv, ty = ey * inv;
      g.nx = !(tx > 0.f) ? 1 : (tx >= (float)(kMorphAxisCells - 1) ? kMorphAxisCells : (int)tx + 1);
      g.ny = !(ty > 0.f) ? 1 : (ty >= (float)(kMorphAxisCells - 1) ? kMorphAxisCells : (int)ty + 1);
    }
  }
  *grid = g;
}

__global__ __launch_bounds__(256) void morph_count_kernel(const float4* __restrict__ cloud, const int* __restrict__ act, const int* __restrict__ d_count,
                                                          const MorphGrid* __restrict__ grid, int* __restrict__ counts, int* __restrict__ cellid) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= *d_count) return;
  const MorphGrid g = *grid;
  const float4 p = cloud[act[t]];
  const int cell = morph_cell(p.y, g.oy, g.inv, g.ny) * g.nx + morph_cell(p.x, g.ox, g.inv, g.nx);
  cellid[t] = cell;
  atomicAdd(&counts[cell], 1);
}

__global__ __launch_bounds__(256) void morph_scatter_kernel(const float4* __restrict__ cloud, const int* __restrict__ act, const int* __restrict__ d_count,
                                                            const int* __restrict__ cellid, const int* __restrict__ cell_start, int* __restrict__ fill,
                                                            unsigned int* __restrict__ ext, bool is_max, float2* __restrict__ sxy,
                                                            float* __restrict__ sval, int* __restrict__ sidx, int* __restrict__ scell) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= *d_count) return;
  const int i = act[t], cell = cellid[t];
  const float4 p = cloud[i];
  const int at = cell_start[cell] + atomicAdd(&fill[cell], 1);  // (the order inside a cell is free: every reader takes an extremum)
  sxy[at] = make_float2(p.x, p.y);
  sval[at] = p.z;
  sidx[at] = i;
  scell[at] = cell;
  atomicMax(&ext[cell], morph_ordered(p.z, is_max));
}

// a wave per sorted point
__global__ __launch_bounds__(256) void morph_box_kernel(const int* __restrict__ d_count, const MorphGrid* __restrict__ grid, float h,
                                                        const float2* __restrict__ sxy, const int* __restrict__ cell_start, const int* __restrict__ scell,
                                                        const float* __restrict__ in_val, const unsigned int* __restrict__ in_ext, bool is_max,
                                                        unsigned int* __restrict__ next_ext, float* __restrict__ out_val,
                                                        unsigned long long* __restrict__ tests) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= *d_count) return;  // (wave-uniform)
  const MorphGrid g = *grid;
  const float2 c = sxy[p];
  const float lox = c.x - h, hix = c.x + h, loy = c.y - h, hiy = c.y + h;
  const int cxl = morph_cell(lox, g.ox, g.inv, g.nx), cxh = morph_cell(hix, g.ox, g.inv, g.nx);
  const int cyl = morph_cell(loy, g.oy, g.inv, g.ny), cyh = morph_cell(hiy, g.oy, g.inv, g.ny);
  const int iw = cxh - cxl - 1, ih = cyh - cyl - 1;  // the strictly interior cells: iw x ih of them when both are positive
  unsigned int best = 0u;
  if (iw > 0 && ih > 0)
    for (int k = lane; k < iw * ih; k += 64) {
      const unsigned int e = in_ext[(cyl + 1 + k / iw) * g.nx + (cxl + 1 + k % iw)];
      best = e > best ? e : best;
    }
  unsigned int tested = 0u;
  auto scan_run = [&](int a, int b) {
    for (int q = a + lane; q < b; q += 64) {
      const float2 s = sxy[q];
      ++tested;
      if (lox <= s.x && s.x <= hix && loy <= s.y && s.y <= hiy) {
        const unsigned int e = morph_ordered(in_val[q], is_max);
        best = e > best ? e : best;
      }
    }
  };
  for (int cy = cyl; cy <= cyh; ++cy) {
    const int row = cy * g.nx;
    if (cy == cyl || cy == cyh || iw <= 0) {
      scan_run(cell_start[row + cxl], cell_start[row + cxh + 1]);  // a row of the rim, or a range without interior columns: one run
    } else {
      scan_run(cell_start[row + cxl], cell_start[row + cxl + 1]);
      scan_run(cell_start[row + cxh], cell_start[row + cxh + 1]);
    }
  }
  best = wave_max(best);
  if (tests) {
    unsigned int total = tested;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) total += (unsigned int)__shfl_xor((int)total, off, 64);
    if (lane == 0) atomicAdd(&tests[(p & (kMorphTestSlots - 1)) * kMorphTestStride], (unsigned long long)total);  // (spread over cache lines)
  }
  if (lane == 0) {
    const float v = morph_unordered(best, is_max);  // (never "nothing": a point is in its own box)
    out_val[p] = v;
    if (next_ext) atomicMax(&next_ext[scell[p]], morph_ordered(v, !is_max));
  }
}

__global__ __launch_bounds__(256) void morph_judge_kernel(const int* __restrict__ d_count, const float* __restrict__ sval, const float* __restrict__ opened,
                                                          const int* __restrict__ sidx, float thr, int pass, int* __restrict__ flags,
                                                          int32_t* __restrict__ removed_at) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= *d_count) return;
  const int i = sidx[p];
  const float diff = sval[p] - opened[p];
  const bool stays = diff < thr;
  flags[i] = stays ? 1 : 0;
  if (!stays) removed_at[i] = pass;
}

__global__ __launch_bounds__(256) void morph_unsort_kernel(const int* __restrict__ d_count, const float* __restrict__ val, const int* __restrict__ sidx,
                                                           float* __restrict__ out_z) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= *d_count) return;
  out_z[sidx[p]] = val[p];
}

__global__ __launch_bounds__(64) void morph_tests_total_kernel(const unsigned long long* __restrict__ tests, unsigned long long* __restrict__ total) {
  unsigned long long v = tests[threadIdx.x * kMorphTestStride];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if (threadIdx.x == 0) *total = v;
}

__global__ __launch_bounds__(256) void pmf_flags_kernel(const int32_t* __restrict__ removed_at, int n, bool invert, int* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  flags[i] = ((removed_at[i] == -1) != invert) ? 1 : 0;
}

}  // namespace

hipError_t launch_morph_init(const float4* cloud, int n, int* flags, int32_t* removed_at, float* out_z, unsigned int* bbox4, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(bbox4, 0, 4 * sizeof(unsigned int), stream);
  if (e != hipSuccess) return e;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(morph_init_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, cloud, n, flags, removed_at, out_z, bbox4);
  return hipGetLastError();
}

hipError_t launch_morph_bin(const float4* cloud, int n, const int* act, const int* d_count, const unsigned int* bbox4, float window, MorphGrid* grid,
                            int* table, int* cell_start, int* scan_scratch, int* cellid, float2* sxy, float* sval, int* sidx, int* scell, bool is_max,
                            hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(table, 0, kMorphTableInts * sizeof(int), stream);
  if (e != hipSuccess) return e;
  int* counts = table;
  int* fill = table + kMorphMaxCells + 1;
  unsigned int* ext = reinterpret_cast<unsigned int*>(fill + kMorphMaxCells);
  const dim3 grid_n((n + 255) / 256);
  hipLaunchKernelGGL(morph_grid_kernel, dim3(1), dim3(1), 0, stream, bbox4, window, grid);
  hipLaunchKernelGGL(morph_count_kernel, grid_n, dim3(256), 0, stream, cloud, act, d_count, grid, counts, cellid);
  e = launch_exclusive_scan(counts, cell_start, kMorphMaxCells + 1, scan_scratch, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(morph_scatter_kernel, grid_n, dim3(256), 0, stream, cloud, act, d_count, cellid, cell_start, fill, ext, is_max, sxy, sval, sidx,
                     scell);
  return hipGetLastError();
}

hipError_t launch_morph_box(int n, const int* d_count, const MorphGrid* grid, float window, const float2* sxy, const int* cell_start, const int* scell,
                            const float* in_val, int* table, int phase, bool is_max, bool feed_next, float* out_val, unsigned long long* tests,
                            hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  unsigned int* ext0 = reinterpret_cast<unsigned int*>(table + 2 * (size_t)kMorphMaxCells + 1);
  unsigned int* in_ext = ext0 + (size_t)phase * kMorphMaxCells;
  unsigned int* next_ext = feed_next ? ext0 + (size_t)(1 - phase) * kMorphMaxCells : nullptr;
  const float h = window / 2.0f;
  hipLaunchKernelGGL(morph_box_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, d_count, grid, h, sxy, cell_start, scell, in_val, in_ext, is_max,
                     next_ext, out_val, tests);
  return hipGetLastError();
}

hipError_t launch_morph_judge(int n, const int* d_count, const float* sval, const float* opened, const int* sidx, float thr, int pass, int* flags,
                              int32_t* removed_at, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(morph_judge_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_count, sval, opened, sidx, thr, pass, flags, removed_at);
  return hipGetLastError();
}

hipError_t launch_morph_unsort(int n, const int* d_count, const float* val, const int* sidx, float* out_z, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(morph_unsort_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_count, val, sidx, out_z);
  return hipGetLastError();
}

hipError_t launch_morph_tests_total(const unsigned long long* tests, unsigned long long* total, hipStream_t stream) {
  hipLaunchKernelGGL(morph_tests_total_kernel, dim3(1), dim3(64), 0, stream, tests, total);
  return hipGetLastError();
}

hipError_t launch_pmf_flags(const int32_t* removed_at, int n, bool invert, int* flags, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(pmf_flags_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, removed_at, n, invert, flags);
  return hipGetLastError();
}

}  // namespace icpgpu
