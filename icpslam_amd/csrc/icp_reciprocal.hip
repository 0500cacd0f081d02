// icp_reciprocal.hip -- device side of reciprocal correspondences (pcl::registration::CorrespondenceEstimation::
// determineReciprocalCorrespondences, PCL 1.8, as setUseReciprocalCorrespondences(true) makes IterativeClosestPoint call it): a
// stage between the gated key-writing search and the rejector chain that REWRITES KEYS, like the chain's own stages (icp_reject.hip).
//
// The rule: with x_i = T * source[i] (xform_point, as every search rounds it) and j = nn(x_i) in the target, the pair (i, j) stays
// iff the nearest of ALL x_* to target[j] is x_i -- distances by dist2(target[j], x_k), the search's own expression, so that the
// reverse distance of k = i is the pair's forward d2 bit for bit; equal distances go to the lowest source index.
//
// Two observations make the reverse search cheap:
//   * Only the ONE-TO-ONE WINNER of a target point can be reciprocal.  Every pair that chose j is a candidate for nn(target[j]);
//     the packed minimum (d2 bits << 32 | source index) over them -- recip_winner_kernel, the 64-bit atomicMin of one-to-one --
//     beats all the others in exactly the order the rule asks for.  So the kept set is a subset of one-to-one's.
//   * For the winner i the reverse search is an EXISTENCE test inside a known ball: is there any x_k with
//     (d2(target[j], x_k), k) < (d2_i, i)?  Such an x_k lies within sqrt(d2_i) <= the gate of target[j].  The test needs no
//     minimum, ends at the first hit, and does not care in which order a cell's points are visited.
//
// Grid flavour (the target has a usable grid): the transformed source is binned into the TARGET GRID'S OWN lattice (same GridDesc:
// no bounding box, no cell-size rule, no host round trip) -- count (fused with the winner pass), the generic exclusive scan of
// icp_scan.hip, scatter.  A point outside the box goes to the nearest edge cell when it is within `reach` cells of the box and is
// dropped otherwise (reach covers the gate, so a dropped point is farther than the gate from every target point); non-finite points
// are dropped: nobody's neighbour.  recip_grid_apply_kernel then walks, per winner, the cell rows that the ball's bounding box
// touches, sized as grow_cubes sizes its ball (3 % + grid_slack against the float binning), eight candidates per step.  There is no
// cell population cap: a
// crowded cell costs the winners near it a longer walk, never a wrong answer, so nothing has to be detected or handed to another
// kernel.
// Brute flavour (no usable grid, nn_mode = BRUTE): recip_brute_apply_kernel offers every winner all of x_* through LDS tiles of 256;
// a workgroup leaves as soon as none of its winners is still unbeaten.
//
// Per iteration and n_s source, n_t target points: 8 B per target winner set and 8 B per gated pair updated; 16 B read + 8 B
// (cell, rank) written per source point counted, 24 B read + 16 B written per point scattered, 4 B per cell cleared and 12 B
// scanned; the apply pass reads 8 B per key, 8 + 16 B per gated pair (winner, target point) and 16 B per candidate visited, and
// writes 8 B per rejected pair.  The statistics {pairs past the gate, pairs kept} stay in device memory until the host asks.
#include "icp_grid_device.h"

namespace icpgpu {
namespace {

constexpr int RC_BLOCK = 256;
constexpr int RC_UNROLL = 8;  // candidates a lane of the grid flavour's apply pass loads per step

__device__ __forceinline__ bool key_alive(unsigned long long key, float thr) {
  return (unsigned int)key != 0xFFFFFFFFu && __uint_as_float((unsigned int)(key >> 32)) <= thr;
}

// the cell a transformed source point is binned into: -1 = dropped (not finite, or more than `reach` cells outside the box)
__device__ __forceinline__ int bin_of(const GridDesc& g, int reach, float x, float y, float z) {
  if (!finite3(x, y, z)) return -1;
  int cx, cy, cz;
  cell_of(g, x, y, z, cx, cy, cz);
  if (cx < -reach || cx >= g.nx + reach || cy < -reach || cy >= g.ny + reach || cz < -reach || cz >= g.nz + reach) return -1;
  cx = min(max(cx, 0), g.nx - 1);
  cy = min(max(cy, 0), g.ny - 1);
  cz = min(max(cz, 0), g.nz - 1);
  return cz * g.sz + cy * g.sy + cx;
}

// One thread per source point: the winner of every chosen target point and, BIN, the point's cell and its rank in it.
template <bool BIN>
__global__ __launch_bounds__(RC_BLOCK) void recip_winner_kernel(const float4* __restrict__ src, const unsigned long long* __restrict__ keys,
                                                                int n_s, Xform T, float thr, int n_t, GridDesc g, int reach,
                                                                unsigned long long* __restrict__ winners, int* __restrict__ counts,
                                                                int* __restrict__ cell_of_point, int* __restrict__ rank,
                                                                unsigned int* __restrict__ state) {
  const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
  unsigned int alive = 0;
  if (i < n_s) {
    const unsigned long long key = keys[i];
    const unsigned int j = (unsigned int)key;
    if (key_alive(key, thr) && j < (unsigned int)n_t) {
      alive = 1;
      atomicMin(&winners[j], (key & 0xFFFFFFFF00000000ull) | (unsigned long long)(unsigned int)i);
    }
    if (BIN) {
      const float4 p = src[i];
      float x, y, z;
      xform_point(T, p.x, p.y, p.z, x, y, z);
      const int c = bin_of(g, reach, x, y, z);
      cell_of_point[i] = c;
      rank[i] = c >= 0 ? atomicAdd(&counts[c], 1) : 0;
    }
  }
  block_count_add(alive, state + 0);
}

__global__ __launch_bounds__(RC_BLOCK) void recip_scatter_kernel(const float4* __restrict__ src, int n_s, Xform T,
                                                                 const int* __restrict__ cell_of_point, const int* __restrict__ rank,
                                                                 const int* __restrict__ cell_start, float4* __restrict__ binned) {
  const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
  if (i >= n_s) return;
  const int c = cell_of_point[i];
  if (c < 0) return;
  const float4 p = src[i];
  float x, y, z;
  xform_point(T, p.x, p.y, p.z, x, y, z);
  binned[cell_start[c] + rank[i]] = make_float4(x, y, z, __uint_as_float((unsigned int)i));
}

// what a thread's pair is: not alive (nothing to do), alive but not its target's winner (rejected), or the winner (to be tested)
enum { kPairDead = 0, kPairLost = 1, kPairWinner = 2 };
__device__ __forceinline__ int classify(unsigned long long key, int i, float thr, int n_t, const unsigned long long* __restrict__ winners,
                                        unsigned long long& mine) {
  if (!key_alive(key, thr)) return kPairDead;
  const unsigned int j = (unsigned int)key;
  mine = (key & 0xFFFFFFFF00000000ull) | (unsigned long long)(unsigned int)i;
  return (j < (unsigned int)n_t && winners[j] == mine) ? kPairWinner : kPairLost;
}

__global__ __launch_bounds__(RC_BLOCK) void recip_grid_apply_kernel(unsigned long long* __restrict__ keys, int n_s, float thr, int n_t,
                                                                    const float4* __restrict__ tgt, const unsigned long long* __restrict__ winners,
                                                                    GridDesc g, const int* __restrict__ cell_start,
                                                                    const float4* __restrict__ binned, unsigned int* __restrict__ state) {
  const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
  unsigned int kept = 0;
  if (i < n_s) {
    const unsigned long long key = keys[i];
    unsigned long long mine = 0;
    int what = classify(key, i, thr, n_t, winners, mine);
    if (what == kPairWinner) {
      const float4 t = tgt[(unsigned int)key];
      // the ball of radius sqrt(d2) around the target point in cell units, inflated as grow_cubes inflates its own
      const float ux = (t.x - g.ox) * g.inv_h, uy = (t.y - g.oy) * g.inv_h, uz = (t.z - g.oz) * g.inv_h;
      const float w = fast_sqrt(__uint_as_float((unsigned int)(key >> 32))) * g.inv_h * 1.03125f + grid_slack(g);
      const int xa = (int)fmaxf(floorf(ux - w), 0.f), xb = (int)fminf(floorf(ux + w), (float)(g.nx - 1));
      const int ya = (int)fmaxf(floorf(uy - w), 0.f), yb = (int)fminf(floorf(uy + w), (float)(g.ny - 1));
      const int za = (int)fmaxf(floorf(uz - w), 0.f), zb = (int)fminf(floorf(uz + w), (float)(g.nz - 1));
      for (int zz = za; zz <= zb && what == kPairWinner; ++zz)
        for (int yy = ya; yy <= yb && what == kPairWinner; ++yy) {
          if (xa > xb) break;
          const int row = zz * g.sz + yy * g.sy;
          const int lo = cell_start[row + xa], hi = cell_start[row + xb + 1];
          // RC_UNROLL candidates per step, their loads in flight together (a lane's walk is a chain of memory latencies: one
          // candidate per step with an exit test behind every load was 338 us at 200k x 200k).  Past the end of the row the last
          // entry is read again: testing a point twice cannot change an existence test.
          for (int p = lo; p < hi && what == kPairWinner; p += RC_UNROLL) {
            float4 q[RC_UNROLL];
#pragma unroll
            for (int u = 0; u < RC_UNROLL; ++u) q[u] = binned[min(p + u, hi - 1)];
            unsigned long long least = kEmptyKey;
#pragma unroll
            for (int u = 0; u < RC_UNROLL; ++u) {
              const float d = dist2(t.x, t.y, t.z, q[u].x, q[u].y, q[u].z);
              const unsigned long long other = ((unsigned long long)__float_as_uint(d) << 32) | __float_as_uint(q[u].w);
              least = other < least ? other : least;
            }
            if (least < mine) what = kPairLost;
          }
        }
    }
    if (what == kPairWinner) kept = 1;
    else if (what == kPairLost) keys[i] = kEmptyKey;
  }
  block_count_add(kept, state + 1);
}

__global__ __launch_bounds__(RC_BLOCK) void recip_brute_apply_kernel(unsigned long long* __restrict__ keys, int n_s, float thr, int n_t,
                                                                     const float4* __restrict__ src, Xform T, const float4* __restrict__ tgt,
                                                                     const unsigned long long* __restrict__ winners,
                                                                     unsigned int* __restrict__ state) {
  __shared__ float4 tile[RC_BLOCK];
  const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
  int what = kPairDead;
  unsigned long long mine = 0;
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < n_s) {
    const unsigned long long key = keys[i];
    what = classify(key, i, thr, n_t, winners, mine);
    if (what == kPairWinner) t = tgt[(unsigned int)key];
  }
  for (int base = 0; base < n_s; base += RC_BLOCK) {
    if (!__syncthreads_or(what == kPairWinner)) break;  // (also: the tile is free to be overwritten)
    const int k = base + (int)threadIdx.x;
    float x = __builtin_nanf(""), y = x, z = x;  // past the end, or not finite: a NaN distance, whose bits exceed every d2 <= thr
    if (k < n_s) {
      const float4 p = src[k];
      float px, py, pz;
      xform_point(T, p.x, p.y, p.z, px, py, pz);
      if (finite3(px, py, pz)) {
        x = px;
        y = py;
        z = pz;
      }
    }
    tile[threadIdx.x] = make_float4(x, y, z, __uint_as_float((unsigned int)k));
    __syncthreads();
    if (what == kPairWinner) {
      for (int m = 0; m < RC_BLOCK; ++m) {
        const float4 q = tile[m];
        const float d = dist2(t.x, t.y, t.z, q.x, q.y, q.z);
        const unsigned long long other = ((unsigned long long)__float_as_uint(d) << 32) | __float_as_uint(q.w);
        if (other < mine) what = kPairLost;
      }
    }
  }
  unsigned int kept = 0;
  if (what == kPairWinner) kept = 1;
  else if (what == kPairLost) keys[i] = kEmptyKey;
  block_count_add(kept, state + 1);
}

}  // namespace

size_t reciprocal_cells(const GridDesc& g) { return (size_t)g.nx * (size_t)g.ny * (size_t)g.nz; }

hipError_t launch_reciprocal_grid(const float4* src, int n_s, const float4* tgt, int n_t, const Xform& T, float thr,
                                  unsigned long long* keys, const GridDesc& g, int* counts, int* cell_start, int* scan_scratch,
                                  int* cell_of_point, int* rank, float4* binned, unsigned long long* winners, unsigned int* state,
                                  hipStream_t stream) {
  if (n_s <= 0 || n_t <= 0) return hipSuccess;
  const size_t ncells = reciprocal_cells(g);
  hipError_t e = hipMemsetAsync(winners, 0xFF, (size_t)n_t * sizeof(unsigned long long), stream);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(counts, 0, (ncells + 1) * sizeof(int), stream)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(state, 0, kRecipStateInts * sizeof(unsigned int), stream)) != hipSuccess) return e;
  // a transformed point farther than this many cells from the box is farther than the gate from every target point: the gate is at
  // most r_max cells / kGridSafety, and the apply pass's ball 3 % + slack more than that
  const int reach = g.r_max + g.r_max / 8 + 2;
  const dim3 grid((n_s + RC_BLOCK - 1) / RC_BLOCK), block(RC_BLOCK);
  hipLaunchKernelGGL(recip_winner_kernel<true>, grid, block, 0, stream, src, keys, n_s, T, thr, n_t, g, reach, winners, counts,
                     cell_of_point, rank, state);
  if ((e = launch_exclusive_scan(counts, cell_start, (int)(ncells + 1), scan_scratch, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(recip_scatter_kernel, grid, block, 0, stream, src, n_s, T, cell_of_point, rank, cell_start, binned);
  hipLaunchKernelGGL(recip_grid_apply_kernel, grid, block, 0, stream, keys, n_s, thr, n_t, tgt, winners, g, cell_start, binned, state);
  return hipGetLastError();
}

hipError_t launch_reciprocal_brute(const float4* src, int n_s, const float4* tgt, int n_t, const Xform& T, float thr,
                                   unsigned long long* keys, unsigned long long* winners, unsigned int* state, hipStream_t stream) {
  if (n_s <= 0 || n_t <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(winners, 0xFF, (size_t)n_t * sizeof(unsigned long long), stream);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(state, 0, kRecipStateInts * sizeof(unsigned int), stream)) != hipSuccess) return e;
  const dim3 grid((n_s + RC_BLOCK - 1) / RC_BLOCK), block(RC_BLOCK);
  hipLaunchKernelGGL(recip_winner_kernel<false>, grid, block, 0, stream, src, keys, n_s, T, thr, n_t, GridDesc{}, 0, winners,
                     (int*)nullptr, (int*)nullptr, (int*)nullptr, state);
  hipLaunchKernelGGL(recip_brute_apply_kernel, grid, block, 0, stream, keys, n_s, thr, n_t, src, T, tgt, winners, state);
  return hipGetLastError();
}

}  // namespace icpgpu
