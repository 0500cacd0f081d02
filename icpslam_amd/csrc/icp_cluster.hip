// icp_cluster.hip -- pcl::EuclideanClusterExtraction over a context's search cloud (rules: include/icpgpu.h "euclidean clustering",
// DESIGN.md section 3).
//
// The graph is implicit: points i != j are joined iff d2(i, j) < r2, the radius search's rule, and nobody writes its rows down.  Its
// connected components come from a lock-free union-find over ONE array, parent[n]:
//   * parent[i] = i for a finite point, -1 for the others (which are never looked at again);
//   * cluster_hook_kernel: one wave64 per point i walks i's ball exactly as search_radius_count_kernel does (icp_search_device.h)
//     and takes the pairs (i, j) with j < i, so that every edge is handled once.  Per batch of 64 candidates every lane finds the
//     root of its own j, the wave takes the minimum m of those roots and of the smallest root it knows for i, and every lane whose
//     root is not m hooks it under m: in a dense cloud most candidates already share a root and the batch costs finds only;
//   (the find / hook / path-halving functions themselves: icp_unionfind_device.h, shared with icp_region.hip)
//   * a hook puts the LARGER root under the SMALLER with one atomicCAS(parent[larger], larger, smaller).  parent[x] <= x always, and
//     a value only ever decreases, so a find walks a strictly decreasing chain, and when everything is hooked the root of a
//     component is its lowest index whatever order the hooks arrived in: the answer is the same from run to run;
//   * a failed CAS means another hook of that root succeeded: the loop goes on from the value the CAS returned, which is smaller.
//     That is the only retry.  Nothing here waits for another wave: every loop ends after at most (index of its start) steps.
//   * every load of parent[] inside those loops is a relaxed agent-scope atomic load -- a plain load could be hoisted out of the loop;
//   * finds halve their paths with atomicMin(parent[x], grandparent): an ancestor, and smaller than what was there.
// cluster_flatten_kernel, a launch later, names every point's component (its root) and counts the roots' sizes with integer atomics.
// The order -- size descending, lowest name first among equals, ascending indices inside a cluster -- is two stable radix sorts
// (icp_scan.hip) over all n points: by n - size of the emitted roots (every other point carries the key n and lands behind them), which
// ranks the clusters, then by rank (n for a point in no cluster), which lists the clusters' points one after the other in ascending
// order.  Every launch count is fixed by n's bit length alone: nothing iterates over the graph's diameter.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "icp_device.h"
#include "icp_grid_device.h"
#include "icp_kernels.h"
#include "icp_search_device.h"
#include "icp_unionfind_device.h"

namespace icpgpu {
namespace {

constexpr int CL_BLOCK = 256, CL_WAVES = CL_BLOCK / 64;

__global__ __launch_bounds__(CL_BLOCK) void cluster_init_kernel(const float4* __restrict__ cloud, int n, int* __restrict__ parent,
                                                                int* __restrict__ sizes) {
  const int i = blockIdx.x * CL_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float4 p = cloud[i];
  parent[i] = finite3(p.x, p.y, p.z) ? i : -1;
  sizes[i] = 0;
}

__global__ __launch_bounds__(CL_BLOCK) void cluster_hook_kernel(const float4* __restrict__ cloud, int n, const float4* __restrict__ sorted,
                                                                const int* __restrict__ cell_start, GridDesc g, int R, float r2, int* parent) {
  const unsigned int lane = threadIdx.x & 63u;
  const int i = blockIdx.x * CL_WAVES + (int)(threadIdx.x >> 6);
  if (i >= n) return;  // (wave-uniform)
  const float4 p = cloud[i];
  if (!finite3(p.x, p.y, p.z)) return;
  int cur = i;  // (wave-uniform) the smallest root seen for i's set
  ball_batches(cloud, n, sorted, cell_start, g, R, p, lane, [&](u64 key) {
    const int j = (int)(unsigned int)key;
    const bool in = key_in_ball(key, r2) && j < i;
    if (__ballot(in) == 0ull) return;
    const int r = in ? cluster_find(parent, j) : kNoRoot;
    const int m = min((int)wave_min_u32((unsigned int)r), cur);
    if (in && r != m) cluster_unite(parent, r, m);
    if (lane == 0u && cur != m) cluster_unite(parent, cur, m);
    cur = m;
  });
}

__global__ __launch_bounds__(CL_BLOCK) void cluster_flatten_kernel(int* parent, int n, int* __restrict__ component, int* sizes) {
  const int i = blockIdx.x * CL_BLOCK + threadIdx.x;
  int root = -1;
  if (i < n && parent_load(parent, i) >= 0) root = cluster_find(parent, i);
  if (i < n) component[i] = root;
  cluster_count_root(sizes, root);
}

// per point: the first sort's pair.  An emitted root carries n - size (0 .. n - 1), every other point n.
__global__ __launch_bounds__(CL_BLOCK) void cluster_root_keys_kernel(const int* __restrict__ component, const int* __restrict__ sizes, int n,
                                                                     int min_size, int max_size, int* __restrict__ keys, int* __restrict__ vals,
                                                                     int* __restrict__ rank_of) {
  const int i = blockIdx.x * CL_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int s = sizes[i];
  const bool emitted = component[i] == i && min_size <= s && s <= max_size;
  keys[i] = emitted ? n - s : n;
  vals[i] = i;
  rank_of[i] = -1;
}

// per position r of the first sort's result: rank_of[root] = r and csize[r] = the cluster's size for an emitted root, 0 behind them
__global__ __launch_bounds__(CL_BLOCK) void cluster_rank_kernel(const int* __restrict__ keys, const int* __restrict__ vals, int n,
                                                                int* __restrict__ rank_of, int* __restrict__ csize) {
  const int r = blockIdx.x * CL_BLOCK + threadIdx.x;
  if (r > n) return;
  int s = 0;
  if (r < n) {
    const int key = keys[r];
    if (key < n) {
      s = n - key;
      rank_of[vals[r]] = r;
    }
  }
  csize[r] = s;
}

// per point: its label and the second sort's pair; per position r: cstart64[r]; counts = {clusters, clustered points} (zero before)
__global__ __launch_bounds__(CL_BLOCK) void cluster_label_kernel(const int* __restrict__ component, const int* __restrict__ rank_of,
                                                                 const int* __restrict__ sorted_keys, const int* __restrict__ cstart, int n,
                                                                 int* __restrict__ labels, int* __restrict__ keys, int* __restrict__ vals,
                                                                 long long* __restrict__ cstart64, int* __restrict__ counts) {
  const int i = blockIdx.x * CL_BLOCK + threadIdx.x;
  if (i > n) return;
  cstart64[i] = (long long)cstart[i];
  if (i == n) return;
  const int comp = component[i];
  const int label = comp >= 0 ? rank_of[comp] : -1;
  labels[i] = label;
  keys[i] = label >= 0 ? label : n;
  vals[i] = i;
  if (sorted_keys[i] < n && (i == n - 1 || sorted_keys[i + 1] >= n)) {  // the last emitted root
    counts[0] = i + 1;
    counts[1] = cstart[i + 1];
  }
}

unsigned int bit_length(int n) {
  unsigned int b = 0;
  while (b < 31 && (n >> b) != 0) ++b;
  return b;
}

}  // namespace

size_t cluster_scratch_ints(int n) { return std::max(radix_sort_scratch_ints(n), exclusive_scan_scratch_ints(n + 1)); }

// the tail after the components are named and counted: the emitted roots' ranks, every point's label, the two stable sorts
hipError_t launch_cluster_tail(const int* component, const int* sizes, int n, int min_size, int max_size, int* labels, int* rank_of, int* csize,
                               int* cstart, long long* cstart64, int* keys, int* vals, int* scratch, int* counts, hipStream_t stream) {
  hipError_t e;
  if ((e = hipMemsetAsync(counts, 0, 2 * sizeof(int), stream)) != hipSuccess) return e;
  if (n <= 0) return hipMemsetAsync(cstart64, 0, sizeof(long long), stream);
  const dim3 per_point((n + CL_BLOCK - 1) / CL_BLOCK), per_slot((n + 1 + CL_BLOCK - 1) / CL_BLOCK), block(CL_BLOCK);
  const unsigned int end_bit = bit_length(n);  // the keys of both sorts are 0 .. n
  hipLaunchKernelGGL(cluster_root_keys_kernel, per_point, block, 0, stream, component, sizes, n, min_size, max_size, keys, vals, rank_of);
  if ((e = launch_radix_sort_pairs(keys, vals, n, end_bit, scratch, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(cluster_rank_kernel, per_slot, block, 0, stream, keys + n, vals + n, n, rank_of, csize);
  if ((e = launch_exclusive_scan(csize, cstart, n + 1, scratch, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(cluster_label_kernel, per_slot, block, 0, stream, component, rank_of, keys + n, cstart, n, labels, keys, vals, cstart64, counts);
  if ((e = launch_radix_sort_pairs(keys, vals, n, end_bit, scratch, stream)) != hipSuccess) return e;
  return hipGetLastError();
}

hipError_t launch_cluster_extract(const float4* cloud, int n, bool any_finite, const float4* sorted, const int* cell_start, const GridDesc& g,
                                  int shells, float r2, int min_size, int max_size, int* parent, int* sizes, int* component, int* labels,
                                  int* rank_of, int* csize, int* cstart, long long* cstart64, int* keys, int* vals, int* scratch, int* counts,
                                  hipStream_t stream) {
  if (n > 0) {
    const dim3 per_point((n + CL_BLOCK - 1) / CL_BLOCK), block(CL_BLOCK);
    hipLaunchKernelGGL(cluster_init_kernel, per_point, block, 0, stream, cloud, n, parent, sizes);
    if (any_finite && r2 > 0.f)  // (r2 == 0: no d2 is below it)
      hipLaunchKernelGGL(cluster_hook_kernel, dim3((n + CL_WAVES - 1) / CL_WAVES), block, 0, stream, cloud, n, sorted, cell_start, g, shells, r2, parent);
    hipLaunchKernelGGL(cluster_flatten_kernel, per_point, block, 0, stream, parent, n, component, sizes);
  }
  return launch_cluster_tail(component, sizes, n, min_size, max_size, labels, rank_of, csize, cstart, cstart64, keys, vals, scratch, counts, stream);
}

}  // namespace icpgpu
