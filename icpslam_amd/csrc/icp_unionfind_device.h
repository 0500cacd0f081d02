// icp_unionfind_device.h -- the lock-free union-find over ONE array, parent[n], that icp_cluster.hip (euclidean clustering) and
// icp_region.hip (region growing) hook their graphs' edges into (internal).  The rules are stated at the head of icp_cluster.hip:
// parent[x] <= x always, a value only ever decreases, a hook puts the LARGER root under the SMALLER with one atomicCAS, and when
// everything is hooked the root of a component is its lowest index whatever order the hooks arrived in.
#pragma once

#include <hip/hip_runtime.h>

namespace icpgpu {
namespace {

constexpr int kNoRoot = 0x7FFFFFFF;

__device__ __forceinline__ int parent_load(const int* parent, int x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x (x is a vertex's index).  Ends: every step moves to a strictly smaller index.
__device__ __forceinline__ int cluster_find(int* parent, int x) {
  int p = parent_load(parent, x);
  while (p != x) {
    const int gp = parent_load(parent, p);
    if (gp != p) __hip_atomic_fetch_min(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // path halving
    x = p;
    p = gp;
  }
  return x;
}

// joins the sets of a and b.  Ends: a failed CAS hands back a smaller parent of `hi`, and the pair of roots only ever decreases.
__device__ __forceinline__ void cluster_unite(int* parent, int a, int b) {
  for (;;) {
    a = cluster_find(parent, a);
    b = cluster_find(parent, b);
    if (a == b) return;
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    a = old;  // hi is no root any more: go on from what it was hooked under
    b = lo;
  }
}

// sizes[root] += 1 for every lane with root >= 0: one atomic for the lanes that share the first lane's root (neighbouring indices
// mostly do), one each for the others.  Every lane of the wave calls it.
__device__ __forceinline__ void cluster_count_root(int* sizes, int root) {
  const int first = __builtin_amdgcn_readfirstlane(root);
  const unsigned long long same = __ballot(root == first);
  if (root == first) {
    if (first >= 0 && (threadIdx.x & 63u) == (unsigned int)(__ffsll((long long)same) - 1)) atomicAdd(sizes + first, __popcll(same));
  } else if (root >= 0) {
    atomicAdd(sizes + root, 1);
  }
}

}  // namespace
}  // namespace icpgpu
