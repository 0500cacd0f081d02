// icp_region.hip -- pcl::RegionGrowing over a context's search cloud by an ORDER-FREE rule (rules: include/icpgpu.h "region growing",
// DESIGN.md section 3).
//
// PCL grows a region from a seed queue, and which region a point lands in depends on the order the points are visited in.  Here
// every decision is a property of the cloud, the normals and the arguments alone:
//   * region_kind_kernel, a thread per point: a finite point with four finite normal floats is a PARTICIPANT; one whose curvature
//     is not above the threshold is a CORE (kind 2, parent[i] = i), the others wait as kind 0 with parent[i] = -1; a point that is
//     no participant is kind -1 and is never looked at again.  border_key[i] = all ones, sizes[i] = 0.
//   * region_link_kernel and region_hook_kernel, a wave64 per core i and a lane per entry j of i's k-nearest row (k <= 64): the
//     lane gathers j's normal and tests smooth(i, j) = |(nx nx' + ny ny') + nz nz'| >= smoothness_cos, every product and sum
//     rounded on its own, so that the test is exactly symmetric.  A smooth CORE neighbour is an edge of the core graph -- j in
//     row(i) or i in row(j): the row's owner handles it, whichever of the two that is.  The link launch puts i under its lowest such
//     neighbour below itself with a plain store (nobody else writes parent[i] in that launch; measured: the hooks behind it are a
//     sixth cheaper, profiles/region.txt); the hook launch puts every such pair into the union-find of icp_unionfind_device.h as
//     cluster_hook_kernel's candidates go: the wave takes the minimum root of the batch first.  A smooth neighbour that is a
//     participant but no core gets, in the link launch, one 64-bit atomicMin of (bits of row(i)'s d2 for j) << 32 | i on
//     border_key[j]: it ends with its nearest listing core, the lowest index among equals.  A minimum and the hooks are both
//     order-free, and the links are a function of the rows, so the answer is the same from run to run.
//   * region_resolve_kernel, a launch later and a thread per point: region[i] = find(i) for a core; for the others the key says
//     whether a core claimed them (kind 1, anchor = that core, region = its root) or not (kind 0, a region of their own); the
//     regions' sizes are counted with integer atomics.
// The regions are then a partition stated as clustering states its components -- region[name] == name, sizes[name] -- and
// launch_cluster_tail (icp_cluster.hip) ranks and lists them.  Nothing iterates over the graph's diameter.
#include <hip/hip_runtime.h>

#include "icp_device.h"
#include "icp_grid_device.h"
#include "icp_kernels.h"
#include "icp_unionfind_device.h"

namespace icpgpu {
namespace {

constexpr int RG_BLOCK = 256, RG_WAVES = RG_BLOCK / 64;
constexpr unsigned long long kNoKey = ~0ull;

__global__ __launch_bounds__(RG_BLOCK) void region_kind_kernel(const float4* __restrict__ cloud, const float4* __restrict__ normals, int n,
                                                               float curvature_threshold, int* __restrict__ kind, int* __restrict__ parent,
                                                               int* __restrict__ sizes, unsigned long long* __restrict__ border_key) {
  const int i = blockIdx.x * RG_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float4 p = cloud[i], nc = normals[i];
  const bool participant = finite3(p.x, p.y, p.z) && finite3(nc.x, nc.y, nc.z) && isfinite(nc.w);
  const bool core = participant && !(nc.w > curvature_threshold);
  kind[i] = core ? 2 : participant ? 0 : -1;
  parent[i] = core ? i : -1;
  sizes[i] = 0;
  border_key[i] = kNoKey;
}

// LINK: the launch in front of the hooks (region_link_kernel below); otherwise the hooks themselves
template <bool LINK>
__device__ __forceinline__ void region_row(const float4* __restrict__ normals, const int* __restrict__ kind, int n,
                                           const int32_t* __restrict__ rows_idx, const float* __restrict__ rows_d2,
                                           const int32_t* __restrict__ rows_found, int k, float smoothness_cos, int* parent,
                                           unsigned long long* border_key) {
  const int lane = (int)(threadIdx.x & 63u);
  const int i = blockIdx.x * RG_WAVES + (int)(threadIdx.x >> 6);
  if (i >= n) return;         // (wave-uniform)
  if (kind[i] != 2) return;   // (wave-uniform)
  const float4 ni = normals[i];
  const int found = min(rows_found[i], k);
  int j = -1, kj = -1;
  float d2 = 0.f;
  if (lane < found) {
    j = rows_idx[(size_t)i * (size_t)k + (size_t)lane];
    d2 = rows_d2[(size_t)i * (size_t)k + (size_t)lane];
  }
  const bool listed = j >= 0 && j < n && j != i;
  bool smooth = false;
  if (listed) {
    kj = kind[j];
    if (kj >= 0) {
      const float4 nj = normals[j];
      const float dot = (ni.x * nj.x + ni.y * nj.y) + ni.z * nj.z;
      smooth = fabsf(dot) >= smoothness_cos;
    }
  }
  const bool in = smooth && kj == 2;
  if (LINK) {
    if (smooth && kj != 2) atomicMin(border_key + j, ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)(unsigned int)i);
    const int lowest = (int)wave_min_u32(in ? (unsigned int)j : (unsigned int)kNoRoot);
    if (lane == 0 && lowest < i) parent[i] = lowest;  // (i is a root and nobody else writes parent[i] in this launch)
    return;
  }
  if (__ballot(in) == 0ull) return;
  const int r = in ? cluster_find(parent, j) : kNoRoot;
  const int m = min((int)wave_min_u32((unsigned int)r), i);
  if (in && r != m) cluster_unite(parent, r, m);
  if (lane == 0 && i != m) cluster_unite(parent, i, m);
}

// the borders' keys, and every core under its lowest smooth core neighbour when that is below itself: a link is an edge of the core
// graph, parent[i] < i keeps the forest a forest, and nothing is contended -- most cores are attached before the first hook
__global__ __launch_bounds__(RG_BLOCK) void region_link_kernel(const float4* __restrict__ normals, const int* __restrict__ kind, int n,
                                                               const int32_t* __restrict__ rows_idx, const float* __restrict__ rows_d2,
                                                               const int32_t* __restrict__ rows_found, int k, float smoothness_cos, int* parent,
                                                               unsigned long long* border_key) {
  region_row<true>(normals, kind, n, rows_idx, rows_d2, rows_found, k, smoothness_cos, parent, border_key);
}

__global__ __launch_bounds__(RG_BLOCK) void region_hook_kernel(const float4* __restrict__ normals, const int* __restrict__ kind, int n,
                                                               const int32_t* __restrict__ rows_idx, const float* __restrict__ rows_d2,
                                                               const int32_t* __restrict__ rows_found, int k, float smoothness_cos, int* parent,
                                                               unsigned long long* border_key) {
  region_row<false>(normals, kind, n, rows_idx, rows_d2, rows_found, k, smoothness_cos, parent, border_key);
}

__global__ __launch_bounds__(RG_BLOCK) void region_resolve_kernel(int* parent, int n, const unsigned long long* __restrict__ border_key,
                                                                  int* __restrict__ kind, int* __restrict__ region, int* __restrict__ anchor,
                                                                  int* sizes) {
  const int i = blockIdx.x * RG_BLOCK + threadIdx.x;
  int root = -1;
  if (i < n) {
    const int kd = kind[i];
    int a = -1;
    if (kd == 2) {
      root = cluster_find(parent, i);
    } else if (kd == 0) {
      const unsigned long long key = border_key[i];
      if (key != kNoKey) {
        a = (int)(unsigned int)key;
        root = cluster_find(parent, a);
        kind[i] = 1;
      } else {
        root = i;
      }
    }
    region[i] = root;
    anchor[i] = a;
  }
  cluster_count_root(sizes, root);
}

}  // namespace

hipError_t launch_region_growing(const float4* cloud, const float4* normals, int n, bool any_finite, const int32_t* rows_idx, const float* rows_d2,
                                 const int32_t* rows_found, int k, float smoothness_cos, float curvature_threshold, int min_size, int max_size,
                                 int* kind, unsigned long long* border_key, int* anchor, int* parent, int* sizes, int* region, int* labels,
                                 int* rank_of, int* csize, int* cstart, long long* cstart64, int* keys, int* vals, int* scratch, int* counts,
                                 hipStream_t stream) {
  if (n > 0) {
    const dim3 per_point((n + RG_BLOCK - 1) / RG_BLOCK), block(RG_BLOCK);
    hipLaunchKernelGGL(region_kind_kernel, per_point, block, 0, stream, cloud, normals, n, curvature_threshold, kind, parent, sizes, border_key);
    if (any_finite) {
      const dim3 per_row((n + RG_WAVES - 1) / RG_WAVES);
      hipLaunchKernelGGL(region_link_kernel, per_row, block, 0, stream, normals, kind, n, rows_idx, rows_d2, rows_found, k, smoothness_cos, parent,
                         border_key);
      hipLaunchKernelGGL(region_hook_kernel, per_row, block, 0, stream, normals, kind, n, rows_idx, rows_d2, rows_found, k, smoothness_cos, parent,
                         border_key);
    }
    hipLaunchKernelGGL(region_resolve_kernel, per_point, block, 0, stream, parent, n, border_key, kind, region, anchor, sizes);
  }
  return launch_cluster_tail(region, sizes, n, min_size, max_size, labels, rank_of, csize, cstart, cstart64, keys, vals, scratch, counts, stream);
}

}  // namespace icpgpu
