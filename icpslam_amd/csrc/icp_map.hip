// icp_map.hip -- the mapper's one-point-per-voxel map on the GPU.
//
// Reference behaviour (/root/reference/src/icpslam/octree_mapper.cpp):
//   :55-59  resetMap()          pcl::octree::OctreePointCloudSearch<PointXYZ>(octree_resolution_ = 0.5 m), empty cloud
//   :62-69  addPointsToMap()    for every point IN ORDER: if its octree voxel is not occupied, append it to map_cloud_
//   :72-90  approxNearestNeighbors()  for every scan point the nearest map point -> "nn cloud", the ICP target
// The octree itself is PCL's; what the reference relies on is (i) one point per leaf voxel, the FIRST one to arrive,
// (ii) PCL's leaf keys: trunc((p - min) / resolution) in double under the bounding box in force when the point is tested
// (OctreePointCloud::genOctreeKeyforPoint), the box starting at the first point +- resolution (p +- res/2 widened by
// getKeyBitSize) and doubling towards every point outside it -- such a point is always added, isVoxelOccupiedAtPoint() being
// false outside the box; keys are kept in the first box's frame (ApproxHistory in icp_kernels.h).  The minimum moves by
// whole side lengths, but each move rounds in double, so for a resolution that is not a power of two a point on a voxel face
// can key one voxel off floor((p - first minimum) / res) (until this was found the map keyed that lattice; powers of two
// round exactly and were never affected).  (iii) a nearest-neighbour query per scan point.  (iii) is approximate in PCL
// (approxNearestSearch descends by voxel centre); here it is EXACT by default, which is what SURVEY.md 8(f4) asks for.
//
// MI355X design: the octree becomes an open-addressing hash set keyed by the packed voxel coordinates (64-bit keys,
// linear probing, load factor <= 1/2).  "First point in input order wins" is made deterministic under parallel
// insertion with a per-slot atomicMin over the input index, followed by an order-preserving compaction (prefix sum) so
// that the map cloud is bit-for-bit the sequential one.  All HBM-bound integer work: coalesced 16-B point reads, one
// random 8-B probe per point.
#include "icp_kernels.h"

#include <cstring>

#include "icp_device.h"

namespace icpgpu {
namespace {

constexpr unsigned long long kEmptySlot = 0xFFFFFFFFFFFFFFFFull;
constexpr int kNoPoint = 0x7FFFFFFF;
constexpr long long kVoxelBias = 1ll << 20;  // voxel coordinates are stored biased, 21 bits per axis

__device__ __forceinline__ unsigned long long hash_key(unsigned long long k) {  // murmur3 finaliser
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// PCL's key of a point inside box version v (genOctreeKeyforPoint: truncation), in the first box's frame; false beyond the reach
__device__ __forceinline__ bool pcl_key(const ApproxHistory& h, int v, double res, float x, float y, float z, unsigned long long& key) {
  const long long kx = (long long)(((double)x - h.min[v][0]) / res) - h.shift[v][0];
  const long long ky = (long long)(((double)y - h.min[v][1]) / res) - h.shift[v][1];
  const long long kz = (long long)(((double)z - h.min[v][2]) / res) - h.shift[v][2];
  if (kx < -kMapKeyReach || kx > kMapKeyReach || ky < -kMapKeyReach || ky > kMapKeyReach || kz < -kMapKeyReach || kz > kMapKeyReach)
    return false;
  const unsigned long long ux = (unsigned long long)(kx + kVoxelBias), uy = (unsigned long long)(ky + kVoxelBias),
                           uz = (unsigned long long)(kz + kVoxelBias);
  key = (uz << 42) | (uy << 21) | ux;
  return true;
}

// find the slot holding `key`, or claim an empty one for it; -1 only if the table is full (never: load <= 1/2)
__device__ __forceinline__ int find_or_claim(unsigned long long* __restrict__ keys, unsigned int mask, unsigned long long key) {
  unsigned int s = (unsigned int)hash_key(key) & mask;
  for (unsigned int probe = 0; probe <= mask; ++probe) {
    unsigned long long cur = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == key) return (int)s;
    if (cur == kEmptySlot) {
      const unsigned long long prev = atomicCAS(&keys[s], kEmptySlot, key);
      if (prev == kEmptySlot || prev == key) return (int)s;
    }
    s = (s + 1) & mask;
  }
  return -1;
}

__global__ __launch_bounds__(256) void map_fill_kernel(unsigned long long* __restrict__ keys, int* __restrict__ vals,
                                                       int* __restrict__ first, unsigned int cap) {
  const unsigned int i = blockIdx.x * 256 + threadIdx.x;
  if (i < cap) {
    keys[i] = kEmptySlot;
    vals[i] = -1;
    first[i] = kNoPoint;
  }
}

// re-insert the existing map points after the table has grown, from their stored keys
__global__ __launch_bounds__(256) void map_rehash_kernel(const unsigned long long* __restrict__ pkeys, int n_map,
                                                         unsigned long long* __restrict__ keys, int* __restrict__ vals,
                                                         unsigned int mask) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_map) return;
  const int s = find_or_claim(keys, mask, pkeys[i]);
  if (s >= 0) vals[s] = i;
}

__global__ __launch_bounds__(256) void map_xform_kernel(const float4* __restrict__ in, int n, Xform T, float4* __restrict__ moved) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 s = in[i];
  float4 p;
  xform_point(T, s.x, s.y, s.z, p.x, p.y, p.z);
  p.w = 1.0f;
  moved[i] = p;
}

constexpr int kGrewBox = 1 << 30;  // slot_of flag: the point grew the box (slots < 2^30: cap <= 2^30)

// pass 1: key the point under its box version, locate / claim the voxel, and bid for it with the input index (lowest wins);
// a point that grew the box is appended whatever the voxel holds (it still bids, so that later points find the voxel taken)
__global__ __launch_bounds__(256) void map_claim_kernel(const float4* __restrict__ moved, int n, ApproxHistory h, double res,
                                                        unsigned long long* __restrict__ keys,
                                                        const int* __restrict__ vals, int* __restrict__ first,
                                                        unsigned int mask, int* __restrict__ slot_of) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = moved[i];
  int v = -1;
  for (int k = 0; k < h.n; ++k)
    if (h.first[k] <= i) v = k;
  int slot = -1;
  unsigned long long key;
  if (v >= 0 && isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
    const bool grew = h.first[v] == i;
    const double x = p.x, y = p.y, z = p.z;
    // a point outside its box that did not grow it was beyond the reach (icpgpu_map.cpp, map_replay_box): dropped
    const bool inside = !(x < h.min[v][0] || y < h.min[v][1] || z < h.min[v][2] || x >= h.max[v][0] || y >= h.max[v][1] ||
                          z >= h.max[v][2]);
    if ((grew || inside) && pcl_key(h, v, res, p.x, p.y, p.z, key)) {
      slot = find_or_claim(keys, mask, key);
      if (slot >= 0) {
        if (!grew && vals[slot] >= 0) slot = -1;  // voxel occupied by an earlier call: isVoxelOccupiedAtPoint() == true
        else {
          atomicMin(&first[slot], i);
          if (grew) slot |= kGrewBox;
        }
      }
    }
  }
  slot_of[i] = slot;
}

__global__ __launch_bounds__(256) void map_flag_kernel(const int* __restrict__ slot_of, const int* __restrict__ first, int n,
                                                       int* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int s = slot_of[i];
  flags[i] = (s >= 0 && ((s & kGrewBox) || first[s] == i)) ? 1 : 0;
}

// pass 2: the winners append themselves at base + rank (input order preserved) and seal their voxel
__global__ __launch_bounds__(256) void map_commit_kernel(const float4* __restrict__ moved, const int* __restrict__ slot_of,
                                                         const int* __restrict__ flags, const int* __restrict__ rank,
                                                         int n, int base, float4* __restrict__ map_pts,
                                                         unsigned long long* __restrict__ pkeys,
                                                         const unsigned long long* __restrict__ keys,
                                                         int* __restrict__ vals, int* __restrict__ first,
                                                         int* __restrict__ n_added) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (flags[i]) {
    const int s = slot_of[i] & ~kGrewBox, idx = base + rank[i];
    map_pts[idx] = moved[i];
    pkeys[idx] = keys[s];
    vals[s] = idx;  // (two points share a slot only if one of them grew the box: either index marks it occupied)
    first[s] = kNoPoint;
  }
  if (i == n - 1) *n_added = rank[i] + flags[i];
}

// nn cloud: out[rank] = T_out * map[index of the key], empty keys (non-finite queries) dropped, order preserved
__global__ __launch_bounds__(256) void map_nn_flag_kernel(const unsigned long long* __restrict__ keys, int n,
                                                          int* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) flags[i] = keys[i] != kEmptyKey ? 1 : 0;
}

__global__ __launch_bounds__(256) void map_nn_gather_kernel(const unsigned long long* __restrict__ keys,
                                                            const int* __restrict__ flags, const int* __restrict__ rank,
                                                            int n, const float4* __restrict__ map_pts, Xform T_out,
                                                            float4* __restrict__ out, int* __restrict__ n_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (flags[i]) {
    const float4 q = map_pts[(unsigned int)keys[i]];
    float4 o;
    xform_point(T_out, q.x, q.y, q.z, o.x, o.y, o.z);
    o.w = 1.0f;
    out[rank[i]] = o;
  }
  if (i == n - 1) *n_out = rank[i] + flags[i];
}

// distinct points of the nn cloud: a map point's first user (lowest scan index) represents it
__global__ __launch_bounds__(256) void map_first_user_kernel(const unsigned long long* __restrict__ keys,
                                                             const int* __restrict__ flags, int n,
                                                             int* __restrict__ first_user) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && flags[i]) atomicMin(&first_user[(unsigned int)keys[i]], i);
}

__global__ __launch_bounds__(256) void map_unique_flag_kernel(const unsigned long long* __restrict__ keys,
                                                              const int* __restrict__ flags, int n,
                                                              const int* __restrict__ first_user,
                                                              int* __restrict__ uflags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) uflags[i] = (flags[i] && first_user[(unsigned int)keys[i]] == i) ? 1 : 0;
}

__global__ __launch_bounds__(256) void map_unique_gather_kernel(const int* __restrict__ uflags, const int* __restrict__ urank,
                                                                const int* __restrict__ rank, int n,
                                                                const float4* __restrict__ nn_cloud,
                                                                float4* __restrict__ uniq, int* __restrict__ uniq_index,
                                                                int* __restrict__ n_uniq) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (uflags[i]) {
    const int pos = rank[i];  // position of scan point i's neighbour in the nn cloud
    uniq[urank[i]] = nn_cloud[pos];
    uniq_index[urank[i]] = pos;
  }
  if (i == n - 1) *n_uniq = urank[i] + uflags[i];
}

// ---- PCL's approxNearestSearch, faithfully (octree_mapper.cpp:84) ------------------------------------------------------
// The exact search above is what SURVEY.md 8(f4) asks for; THIS is what the reference literally calls:
// OctreePointCloudSearch::approxNearestSearch descends from the root to the EXISTING child whose voxel centre is nearest to
// the query (float squared distance, the first child in index order x*4 + y*2 + z on ties) and returns the point of the leaf
// it ends in.  The octree is PCL's (not under /root/reference: restated from PCL 1.8's octree_pointcloud.hpp /
// octree_search.hpp, as oracle/map_oracle.c's orc_octree_* restate it -- PARITY UNPINNED); its geometry is the bounding box
// PCL grows point by point (ApproxBox: the host replays adoptBoundingBoxToPoint over every insertion batch in input order, the
// device only finds the next point outside the box), and its leaf keys are the map's own (stored per map point).  The tree
// itself becomes a hash set of occupied nodes keyed by (level, node key = leaf key >> (depth - level)); a leaf entry heads the
// chain of its map points (more than one only where a point that grew the box landed in an occupied leaf).
constexpr int kApproxMaxDepth = 19;  // 19 bits per axis + 5 bits of level in a 64-bit key
__device__ __forceinline__ unsigned long long node_key(int level, long long kx, long long ky, long long kz) {
  return ((unsigned long long)level << 57) | ((unsigned long long)kx << 38) | ((unsigned long long)ky << 19) | (unsigned long long)kz;
}
// first point of pts[0..n) (index order) that is finite, not far from the first box and outside the box -- with no box yet,
// the first finite point: *first = min index (INT_MAX: none)
__global__ __launch_bounds__(256) void approx_first_outside_kernel(const float4* __restrict__ pts, int n, ApproxBox b, bool defined,
                                                                   int* __restrict__ first) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool out = false;
  if (i < n) {
    const float4 p = pts[i];
    const double x = p.x, y = p.y, z = p.z;
    out = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
    if (out && defined) {
      const bool far = !(fabs((x - b.origin[0]) / b.res) <= kMapFar && fabs((y - b.origin[1]) / b.res) <= kMapFar &&
                         fabs((z - b.origin[2]) / b.res) <= kMapFar);
      out = !far && (x < b.min[0] || y < b.min[1] || z < b.min[2] || x >= b.max[0] || y >= b.max[1] || z >= b.max[2]);
    }
  }
  const unsigned long long m = __ballot(out);
  if (m && (threadIdx.x & 63) == 0) atomicMin(first, i + (__ffsll((long long)m) - 1));
}

__global__ __launch_bounds__(256) void approx_fill_kernel(unsigned long long* __restrict__ keys, int* __restrict__ vals, unsigned int cap) {
  const unsigned int i = blockIdx.x * 256 + threadIdx.x;
  if (i < cap) {
    keys[i] = kEmptySlot;
    vals[i] = -1;
  }
}

// the nodes on the path root -> leaf of map points [lo, hi): the stored key (first box's frame) moved by the whole voxels the
// minimum has moved since; each leaf heads a chain of its points (leaf_next; order irrelevant: the descent takes the nearest,
// the lowest index on ties, which is PCL's first in insertion order)
__global__ __launch_bounds__(256) void approx_insert_kernel(const unsigned long long* __restrict__ pkeys, int lo, int hi, ApproxBox b,
                                                            unsigned long long* __restrict__ keys, int* __restrict__ vals,
                                                            int* __restrict__ leaf_next, unsigned int mask) {
  const int i = lo + blockIdx.x * 256 + threadIdx.x;
  if (i >= hi) return;
  const unsigned long long pk = pkeys[i];
  const long long kx = (long long)(pk & 0x1FFFFFull) - kVoxelBias + b.shift[0];
  const long long ky = (long long)((pk >> 21) & 0x1FFFFFull) - kVoxelBias + b.shift[1];
  const long long kz = (long long)((pk >> 42) & 0x1FFFFFull) - kVoxelBias + b.shift[2];
  for (int d = 1; d <= b.depth; ++d) {
    const int sh = b.depth - d;
    const int s = find_or_claim(keys, mask, node_key(d, kx >> sh, ky >> sh, kz >> sh));
    if (s >= 0 && d == b.depth) leaf_next[i] = atomicExch(&vals[s], i);
  }
}

__device__ __forceinline__ int approx_lookup(const unsigned long long* __restrict__ keys, unsigned int mask, unsigned long long key) {
  unsigned int s = (unsigned int)hash_key(key) & mask;
  for (unsigned int probe = 0; probe <= mask; ++probe) {
    const unsigned long long cur = keys[s];
    if (cur == key) return (int)s;
    if (cur == kEmptySlot) return -1;
    s = (s + 1) & mask;
  }
  return -1;
}

// approxNearestSearchRecursive for q = T * query[i]; out[i] = (0 << 32 | map index) or the empty key for a non-finite query
__global__ __launch_bounds__(256) void approx_descend_kernel(const float4* __restrict__ queries, int n, Xform T, ApproxBox b,
                                                             const unsigned long long* __restrict__ keys,
                                                             const int* __restrict__ vals, const int* __restrict__ leaf_next,
                                                             const float4* __restrict__ map_pts, unsigned int mask,
                                                             unsigned long long* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 s = queries[i];
  float qx, qy, qz;
  xform_point(T, s.x, s.y, s.z, qx, qy, qz);
  if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) {
    out[i] = kEmptySlot;
    return;
  }
  long long kx = 0, ky = 0, kz = 0;
  int leaf_slot = -1;
  for (int d = 1; d <= b.depth; ++d) {
    const double size = b.res * (double)(1ll << (b.depth - d));
    float best = 0.f;
    long long bx = 0, by = 0, bz = 0;
    int best_slot = -1;
#pragma unroll
    for (int child = 0; child < 8; ++child) {
      const long long nx = 2 * kx + ((child >> 2) & 1), ny = 2 * ky + ((child >> 1) & 1), nz = 2 * kz + (child & 1);
      const int slot = approx_lookup(keys, mask, node_key(d, nx, ny, nz));
      if (slot < 0) continue;
      // genVoxelCenterFromOctreeKey: float((key + 0.5) * side + min); pointSquaredDist: float, (dx^2 + dy^2) + dz^2
      const float cx = (float)(((double)nx + 0.5) * size + b.min[0]), cy = (float)(((double)ny + 0.5) * size + b.min[1]),
                  cz = (float)(((double)nz + 0.5) * size + b.min[2]);
      const float dx = cx - qx, dy = cy - qy, dz = cz - qz;
      const float dist = (dx * dx + dy * dy) + dz * dz;
      if (best_slot < 0 || dist < best) {
        best = dist;
        best_slot = slot;
        bx = nx;
        by = ny;
        bz = nz;
      }
    }
    if (best_slot < 0) {  // (cannot happen: every inner node has a child)
      out[i] = kEmptySlot;
      return;
    }
    kx = bx;
    ky = by;
    kz = bz;
    leaf_slot = best_slot;
  }
  // the leaf: the nearest of its points (pointSquaredDist, candidate - query), the first in insertion order on ties
  int idx = 0;  // depth 0: the box is one voxel, the map one point
  if (b.depth > 0) {
    float best = 0.f;
    idx = -1;
    for (int j = vals[leaf_slot]; j >= 0; j = leaf_next[j]) {
      const float4 c = map_pts[j];
      const float dx = c.x - qx, dy = c.y - qy, dz = c.z - qz;
      const float dist = (dx * dx + dy * dy) + dz * dz;
      if (idx < 0 || dist < best || (dist == best && j < idx)) {
        best = dist;
        idx = j;
      }
    }
  }
  out[i] = idx < 0 ? kEmptySlot : (unsigned long long)(unsigned int)idx;  // (an empty leaf cannot happen: every leaf has a point)
}

}  // namespace

size_t map_scan_temp_bytes(int n) { return exclusive_scan_scratch_ints(n) * sizeof(int); }

hipError_t launch_map_fill(unsigned long long* keys, int* vals, int* first, unsigned int cap, hipStream_t stream) {
  hipLaunchKernelGGL(map_fill_kernel, dim3((cap + 255) / 256), dim3(256), 0, stream, keys, vals, first, cap);
  return hipGetLastError();
}

hipError_t launch_map_rehash(const unsigned long long* pkeys, int n_map, unsigned long long* keys, int* vals, unsigned int cap,
                             hipStream_t stream) {
  if (n_map <= 0) return hipSuccess;
  hipLaunchKernelGGL(map_rehash_kernel, dim3((n_map + 255) / 256), dim3(256), 0, stream, pkeys, n_map, keys, vals, cap - 1);
  return hipGetLastError();
}

hipError_t launch_map_xform(const float4* in, int n, const Xform& T, float4* moved, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(map_xform_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, in, n, T, moved);
  return hipGetLastError();
}

hipError_t launch_map_insert(const float4* moved, int n, const ApproxHistory& h, double res, unsigned long long* keys, int* vals,
                             int* first, unsigned int cap, int* slot_of, int* flags, int* rank, void* temp, size_t temp_bytes,
                             int base, float4* map_pts, unsigned long long* pkeys, int* d_n_added, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const dim3 grid((n + 255) / 256), block(256);
  hipLaunchKernelGGL(map_claim_kernel, grid, block, 0, stream, moved, n, h, res, keys, vals, first, cap - 1, slot_of);
  hipLaunchKernelGGL(map_flag_kernel, grid, block, 0, stream, slot_of, first, n, flags);
  hipError_t e = launch_exclusive_scan(flags, rank, n, static_cast<int*>(temp), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(map_commit_kernel, grid, block, 0, stream, moved, slot_of, flags, rank, n, base, map_pts, pkeys, keys, vals,
                     first, d_n_added);
  return hipGetLastError();
}

hipError_t launch_map_nn_gather(const unsigned long long* keys, int n, const float4* map_pts, const Xform& T_out, int* flags,
                                int* rank, void* temp, size_t temp_bytes, float4* out, int* d_n_out, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const dim3 grid((n + 255) / 256), block(256);
  hipLaunchKernelGGL(map_nn_flag_kernel, grid, block, 0, stream, keys, n, flags);
  hipError_t e = launch_exclusive_scan(flags, rank, n, static_cast<int*>(temp), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(map_nn_gather_kernel, grid, block, 0, stream, keys, flags, rank, n, map_pts, T_out, out, d_n_out);
  return hipGetLastError();
}

hipError_t launch_map_nn_unique(const unsigned long long* keys, const int* flags, const int* rank, int n, const float4* nn_cloud,
                                int n_map, int* first_user, int* uflags, int* urank, void* temp, size_t temp_bytes,
                                float4* uniq, int* uniq_index, int* d_n_uniq, hipStream_t stream) {
  if (n <= 0 || n_map <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(first_user, 0x7F, (size_t)n_map * sizeof(int), stream);  // 0x7F7F7F7F: larger than any index
  if (e != hipSuccess) return e;
  const dim3 grid((n + 255) / 256), block(256);
  hipLaunchKernelGGL(map_first_user_kernel, grid, block, 0, stream, keys, flags, n, first_user);
  hipLaunchKernelGGL(map_unique_flag_kernel, grid, block, 0, stream, keys, flags, n, first_user, uflags);
  e = launch_exclusive_scan(uflags, urank, n, static_cast<int*>(temp), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(map_unique_gather_kernel, grid, block, 0, stream, uflags, urank, rank, n, nn_cloud, uniq, uniq_index,
                     d_n_uniq);
  return hipGetLastError();
}

}  // namespace icpgpu

namespace icpgpu {
hipError_t launch_approx_first_outside(const float4* pts, int n, const ApproxBox& b, bool defined, int* d_first, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(d_first, 0x7F, sizeof(int), stream);  // 0x7F7F7F7F: larger than any index
  if (e != hipSuccess || n <= 0) return e;
  hipLaunchKernelGGL(approx_first_outside_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, pts, n, b, defined, d_first);
  return hipGetLastError();
}
hipError_t launch_approx_fill(unsigned long long* keys, int* vals, unsigned int cap, hipStream_t stream) {
  hipLaunchKernelGGL(approx_fill_kernel, dim3((cap + 255) / 256), dim3(256), 0, stream, keys, vals, cap);
  return hipGetLastError();
}
hipError_t launch_approx_insert(const unsigned long long* pkeys, int lo, int hi, const ApproxBox& b, unsigned long long* keys,
                                int* vals, int* leaf_next, unsigned int cap, hipStream_t stream) {
  if (hi <= lo || b.depth == 0) return hipSuccess;
  hipLaunchKernelGGL(approx_insert_kernel, dim3((hi - lo + 255) / 256), dim3(256), 0, stream, pkeys, lo, hi, b, keys, vals, leaf_next,
                     cap - 1);
  return hipGetLastError();
}
hipError_t launch_approx_descend(const float4* queries, int n, const Xform& T, const ApproxBox& b, const unsigned long long* keys,
                                 const int* vals, const int* leaf_next, const float4* map_pts, unsigned int cap,
                                 unsigned long long* out, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(approx_descend_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, queries, n, T, b, keys, vals, leaf_next,
                     map_pts, cap - 1, out);
  return hipGetLastError();
}
int approx_max_depth() { return kApproxMaxDepth; }
}  // namespace icpgpu
