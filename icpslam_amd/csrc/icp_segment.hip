// icp_segment.hip -- per-segment moments, boxes and principal axes over CSR segments of a context's search cloud (rules:
// include/icpgpu.h "segment moments"; the float64 finish: icp_segment.h; design and what was not built: DESIGN.md section 5).
//
// A segmented reduction over rows whose lengths run from 1 to the cloud's size.  The LIST -- every segment's entries, one after the
// other -- is cut into chunks of kSegmentChunk = 64 entries, whatever the rows are: a wave takes a chunk and a lane an entry, so a
// launch is sized by what the host knows (the number of listed entries), never by a row's length, and its work per wave is the same
// for one ground segment of 10 000 points and for hundreds of 5-point clusters.  Of every segment with entries in its chunk the wave
// holds a PIECE, a run of neighbouring lanes: a long row is many pieces in many waves, short rows lie packed in one wave, as many
// as fit.  All pieces of a wave are reduced AT ONCE by a segmented ladder (SEGMENT_LADDER): six rounds d = 1, 2, .. 32 in which a
// lane takes in lane + d's value when that lane belongs to the same piece; the piece's first lane ends with its sum.  A piece's
// partial goes to slot chunk + segment -- unique, because a later segment lies in the same or a later chunk -- and a wave per
// segment folds its pieces in a fixed order (lane l the pieces l, l + 64, .. ascending, then a tree): no floating-point atomic anywhere.
//   * segment_first_kernel, a thread per entry: the entry's segment by a binary search over the row bounds, kept in seg_of[] for
//     the two passes; the ladder's minimum of the finite entries' list positions and one integer atomicMin per piece on first[].
//   * segment_sums_kernel: K = the entry at first[segment]; the nine terms exact in float64 as double-doubles (icp_dd.h), the
//     finite count and the float32 box as ordered keys, all through the ladder; the pieces' first lanes store their slots.
//   * segment_fold_kernel, a wave per segment: the pieces' partials into one per segment.
//   * segment_finish_kernel, a thread per segment: rounds each sum once, runs segment_finish (icp_segment.h).
//   * segment_box_kernel: the second pass over the points -- their coordinates along the axes the finish wrote, extents by 64-bit
//     ordered keys through the ladder into the pieces' slots.
//   * segment_box_fold_kernel, a wave per segment, and segment_box_finish_kernel, a thread per segment: segment_finish_box.
// Every store is an ordinary vector store.
#include <hip/hip_runtime.h>

#include "icp_dd.h"
#include "icp_device.h"
#include "icp_kernels.h"
#include "icp_segment.h"
#include "icp_wave.h"

namespace icpgpu {
namespace {

constexpr int SEG_BLOCK = 256;
constexpr unsigned int kNoFirst = 0xFFFFFFFFu;
static_assert(kSegmentChunk == 64 && kSegmentChunk == ICPGPU_SEGMENT_CHUNK, "a chunk is a wave's 64 lanes; include/icpgpu.h states it");

__device__ __forceinline__ unsigned long long shfl_down_u64(unsigned long long v, int d) {
  const unsigned int lo = (unsigned int)__shfl_down((int)(unsigned int)v, d, 64), hi = (unsigned int)__shfl_down((int)(unsigned int)(v >> 32), d, 64);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ double shfl_down_f64(double v, int d) {
  return __longlong_as_double((long long)shfl_down_u64((unsigned long long)__double_as_longlong(v), d));
}

// The segmented ladder.  seg: the lane's segment (-1 past the list's end); a wave's lanes hold neighbouring list positions, so the
// lanes of a segment are a run.  In round d lane l takes in lane l + d iff that lane exists and has the same segment; STEP(d, take)
// does the round's shuffles and combines where `take`.  After the six rounds the first lane of every run holds the run's result.
#define SEGMENT_LADDER(seg, lane, STEP)                                       \
  _Pragma("unroll") for (int d_ = 1; d_ < 64; d_ <<= 1) {                     \
    const int other_ = __shfl_down(seg, d_, 64);                              \
    const bool take_ = (lane) + d_ < 64 && other_ == (seg);                   \
    STEP(d_, take_)                                                           \
  }

// the entry's segment: the last s with start[s] <= e (it is not empty: start[s + 1] > e, as start[n_segments] = total > e)
__device__ __forceinline__ int segment_of_entry(const int* __restrict__ start, int n_segments, int e) {
  int lo = 0, hi = n_segments - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (start[mid] <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ float4 listed_point(const float4* __restrict__ cloud, int n, const int* __restrict__ list, int e) {
  return cloud[min(max(list[e], 0), n - 1)];  // (the list names cloud points)
}

// a piece's first lane: the wave's first lane, or a lane whose left neighbour has another segment
__device__ __forceinline__ bool piece_head(int seg, int lane) {
  const int left = __shfl_up(seg, 1, 64);
  return seg >= 0 && (lane == 0 || left != seg);
}

__global__ __launch_bounds__(SEG_BLOCK) void segment_first_kernel(const float4* __restrict__ cloud, int n, const int* __restrict__ start,
                                                                  const int* __restrict__ list, int n_segments, int total,
                                                                  int* __restrict__ seg_of, unsigned int* __restrict__ first) {
  const int lane = (int)(threadIdx.x & 63u);
  const long long el = (long long)blockIdx.x * SEG_BLOCK + (long long)threadIdx.x;  // (SEG_BLOCK is a multiple of the chunk: a wave is a chunk)
  const int e = el < (long long)total ? (int)el : -1;
  int seg = -1;
  unsigned int at = kNoFirst;
  if (e >= 0) {
    seg = segment_of_entry(start, n_segments, e);
    seg_of[e] = seg;
    const float4 q = listed_point(cloud, n, list, e);
    if (finite3(q.x, q.y, q.z)) at = (unsigned int)e;
  }
#define FIRST_STEP(d, take)                                           \
  {                                                                   \
    const unsigned int o_ = (unsigned int)__shfl_down((int)at, d, 64); \
    if (take) at = min(at, o_);                                       \
  }
  SEGMENT_LADDER(seg, lane, FIRST_STEP)
#undef FIRST_STEP
  if (piece_head(seg, lane) && at != kNoFirst) atomicMin(first + seg, at);
}

__global__ __launch_bounds__(SEG_BLOCK) void segment_sums_kernel(const float4* __restrict__ cloud, int n, const int* __restrict__ list, int total,
                                                                 const int* __restrict__ seg_of, const unsigned int* __restrict__ first,
                                                                 SegmentPartial* __restrict__ partials) {
  const int lane = (int)(threadIdx.x & 63u);
  const long long el = (long long)blockIdx.x * SEG_BLOCK + (long long)threadIdx.x;
  const int e = el < (long long)total ? (int)el : -1;
  const int seg = e >= 0 ? seg_of[e] : -1;
  DD acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t].hi = acc[t].lo = 0.0;
  unsigned int kmin[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, kmax[3] = {0u, 0u, 0u};
  int count = 0;
  if (seg >= 0) {
    const unsigned int at = first[seg];
    const float4 q = listed_point(cloud, n, list, e);
    if (at != kNoFirst && finite3(q.x, q.y, q.z)) {
      const float4 K = listed_point(cloud, n, list, (int)at);
      const double dx = (double)(q.x - K.x), dy = (double)(q.y - K.y), dz = (double)(q.z - K.z);
      acc[0].hi = dx * dx;  // (24 x 24 bits: exact)
      acc[1].hi = dx * dy;
      acc[2].hi = dx * dz;
      acc[3].hi = dy * dy;
      acc[4].hi = dy * dz;
      acc[5].hi = dz * dz;
      acc[6].hi = dx;
      acc[7].hi = dy;
      acc[8].hi = dz;
      kmin[0] = kmax[0] = segment_order_key(__float_as_uint(q.x));
      kmin[1] = kmax[1] = segment_order_key(__float_as_uint(q.y));
      kmin[2] = kmax[2] = segment_order_key(__float_as_uint(q.z));
      count = 1;
    }
  }
#define SUMS_STEP(d, take)                                                                \
  {                                                                                       \
    _Pragma("unroll") for (int t = 0; t < 9; ++t) {                                       \
      DD o_;                                                                              \
      o_.hi = shfl_down_f64(acc[t].hi, d), o_.lo = shfl_down_f64(acc[t].lo, d);           \
      if (take) acc[t] = dd_add(acc[t], o_);                                              \
    }                                                                                     \
    _Pragma("unroll") for (int a = 0; a < 3; ++a) {                                       \
      const unsigned int lo_ = (unsigned int)__shfl_down((int)kmin[a], d, 64);            \
      const unsigned int hi_ = (unsigned int)__shfl_down((int)kmax[a], d, 64);            \
      if (take) kmin[a] = min(kmin[a], lo_), kmax[a] = max(kmax[a], hi_);                 \
    }                                                                                     \
    const int c_ = __shfl_down(count, d, 64);                                             \
    if (take) count += c_;                                                                \
  }
  SEGMENT_LADDER(seg, lane, SUMS_STEP)
#undef SUMS_STEP
  if (piece_head(seg, lane)) {
    SegmentPartial& p = partials[e / kSegmentChunk + seg];
#pragma unroll
    for (int t = 0; t < 9; ++t) p.hi[t] = acc[t].hi, p.lo[t] = acc[t].lo;
#pragma unroll
    for (int a = 0; a < 3; ++a) p.box_min[a] = kmin[a], p.box_max[a] = kmax[a];
    p.count = count;
    p.pad = 0;
  }
}

// A wave per segment folds the segment's pieces, chunks b / 64 .. (e - 1) / 64 at slots chunk + s: lane l takes the pieces l, l + 64, ...
// in ascending order, then six rounds d = 32 .. 1 in which lane l < d takes in lane l + d; lane 0 stores the segment's folded partial.
__global__ __launch_bounds__(SEG_BLOCK) void segment_fold_kernel(const int* __restrict__ start, int n_segments, const unsigned int* __restrict__ first,
                                                                 const SegmentPartial* __restrict__ partials, SegmentPartial* __restrict__ folded) {
  const int lane = (int)(threadIdx.x & 63u);
  const int s = blockIdx.x * (SEG_BLOCK / 64) + (int)(threadIdx.x >> 6);
  if (s >= n_segments) return;          // (wave-uniform)
  if (first[s] == kNoFirst) return;     // (wave-uniform: the finish writes an EMPTY record without reading a partial)
  const int b = start[s], e = start[s + 1];
  const int g0 = b / kSegmentChunk, pieces = (e - 1) / kSegmentChunk - g0 + 1;
  DD acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t].hi = acc[t].lo = 0.0;
  unsigned int kmin[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, kmax[3] = {0u, 0u, 0u};
  int count = 0;
  for (int k = lane; k < pieces; k += 64) {
    const SegmentPartial& p = partials[g0 + k + s];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      DD other;
      other.hi = p.hi[t], other.lo = p.lo[t];
      acc[t] = dd_add(acc[t], other);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) kmin[a] = min(kmin[a], p.box_min[a]), kmax[a] = max(kmax[a], p.box_max[a]);
    count += p.count;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      DD other;
      other.hi = shfl_down_f64(acc[t].hi, d), other.lo = shfl_down_f64(acc[t].lo, d);
      acc[t] = dd_add(acc[t], other);  // (lanes at and above d hold values nobody reads)
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      kmin[a] = min(kmin[a], (unsigned int)__shfl_down((int)kmin[a], d, 64));
      kmax[a] = max(kmax[a], (unsigned int)__shfl_down((int)kmax[a], d, 64));
    }
    count += __shfl_down(count, d, 64);
  }
  if (lane == 0) {
    SegmentPartial& p = folded[s];
#pragma unroll
    for (int t = 0; t < 9; ++t) p.hi[t] = acc[t].hi, p.lo[t] = acc[t].lo;
#pragma unroll
    for (int a = 0; a < 3; ++a) p.box_min[a] = kmin[a], p.box_max[a] = kmax[a];
    p.count = count;
    p.pad = 0;
  }
}

// ... and its extents along the axes: a minimum and a maximum, whatever the order
__global__ __launch_bounds__(SEG_BLOCK) void segment_box_fold_kernel(const int* __restrict__ start, int n_segments, const unsigned int* __restrict__ first,
                                                                     const SegmentBoxPartial* __restrict__ box_partials,
                                                                     SegmentBoxPartial* __restrict__ box_folded) {
  const int lane = (int)(threadIdx.x & 63u);
  const int s = blockIdx.x * (SEG_BLOCK / 64) + (int)(threadIdx.x >> 6);
  if (s >= n_segments) return;          // (wave-uniform)
  if (first[s] == kNoFirst) return;     // (wave-uniform)
  const int b = start[s], e = start[s + 1];
  const int g0 = b / kSegmentChunk, pieces = (e - 1) / kSegmentChunk - g0 + 1;
  unsigned long long klo[3] = {~0ull, ~0ull, ~0ull}, khi[3] = {0ull, 0ull, 0ull};
  for (int k = lane; k < pieces; k += 64) {
    const SegmentBoxPartial& p = box_partials[g0 + k + s];
#pragma unroll
    for (int a = 0; a < 3; ++a) klo[a] = min(klo[a], p.lo[a]), khi[a] = max(khi[a], p.hi[a]);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) klo[a] = min(klo[a], shfl_down_u64(klo[a], d)), khi[a] = max(khi[a], shfl_down_u64(khi[a], d));
  }
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) box_folded[s].lo[a] = klo[a], box_folded[s].hi[a] = khi[a];
  }
}

__global__ __launch_bounds__(SEG_BLOCK) void segment_finish_kernel(const float4* __restrict__ cloud, int n, const int* __restrict__ start,
                                                                   const int* __restrict__ list, int n_segments,
                                                                   const unsigned int* __restrict__ first,
                                                                   const SegmentPartial* __restrict__ folded,
                                                                   icpgpu_segment_record* __restrict__ records) {
  const int s = blockIdx.x * SEG_BLOCK + threadIdx.x;
  if (s >= n_segments) return;
  icpgpu_segment_record r = {};
  const unsigned int at = first[s];
  if (at == kNoFirst) {
    r.status = ICPGPU_SEGMENT_EMPTY;
    records[s] = r;
    return;
  }
  const SegmentPartial& p = folded[s];
  const int ki = min(max(list[at], 0), n - 1);
  const float4 K4 = cloud[ki];
  const float K[3] = {K4.x, K4.y, K4.z};
  double S[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) S[t] = p.hi[t] + p.lo[t];  // the one rounding of each sum
  r.count = p.count;
  r.first = ki;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    r.aabb_min[a] = __uint_as_float(segment_order_unkey(p.box_min[a]));
    r.aabb_max[a] = __uint_as_float(segment_order_unkey(p.box_max[a]));
  }
  segment_finish(r, K, S);
  records[s] = r;
}

__global__ __launch_bounds__(SEG_BLOCK) void segment_box_kernel(const float4* __restrict__ cloud, int n, const int* __restrict__ list, int total,
                                                                const int* __restrict__ seg_of,
                                                                const icpgpu_segment_record* __restrict__ records,
                                                                SegmentBoxPartial* __restrict__ box_partials) {
  const int lane = (int)(threadIdx.x & 63u);
  const long long el = (long long)blockIdx.x * SEG_BLOCK + (long long)threadIdx.x;
  const int e = el < (long long)total ? (int)el : -1;
  const int seg = e >= 0 ? seg_of[e] : -1;
  unsigned long long klo[3] = {~0ull, ~0ull, ~0ull}, khi[3] = {0ull, 0ull, 0ull};
  if (seg >= 0) {
    const icpgpu_segment_record& r = records[seg];
    const float4 q = listed_point(cloud, n, list, e);
    if (r.status == ICPGPU_SEGMENT_OK && finite3(q.x, q.y, q.z)) {
      double axes[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) axes[t] = r.axes[t];
      const float K[3] = {(float)r.K[0], (float)r.K[1], (float)r.K[2]};  // (float32 values, widened by the finish)
      double u[3];
      segment_project(axes, K, q.x, q.y, q.z, u);
#pragma unroll
      for (int a = 0; a < 3; ++a) klo[a] = khi[a] = segment_order_key64((unsigned long long)__double_as_longlong(u[a]));
    }
  }
#define BOX_STEP(d, take)                                                  \
  {                                                                        \
    _Pragma("unroll") for (int a = 0; a < 3; ++a) {                        \
      const unsigned long long lo_ = shfl_down_u64(klo[a], d);             \
      const unsigned long long hi_ = shfl_down_u64(khi[a], d);             \
      if (take) klo[a] = min(klo[a], lo_), khi[a] = max(khi[a], hi_);      \
    }                                                                      \
  }
  SEGMENT_LADDER(seg, lane, BOX_STEP)
#undef BOX_STEP
  if (piece_head(seg, lane)) {
    SegmentBoxPartial& p = box_partials[e / kSegmentChunk + seg];
#pragma unroll
    for (int a = 0; a < 3; ++a) p.lo[a] = klo[a], p.hi[a] = khi[a];
  }
}

__global__ __launch_bounds__(SEG_BLOCK) void segment_box_finish_kernel(int n_segments, const SegmentBoxPartial* __restrict__ box_folded,
                                                                       icpgpu_segment_record* __restrict__ records) {
  const int s = blockIdx.x * SEG_BLOCK + threadIdx.x;
  if (s >= n_segments) return;
  if (records[s].status != ICPGPU_SEGMENT_OK) return;  // (EMPTY: the finish left zeros)
  double lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = __longlong_as_double((long long)segment_order_unkey64(box_folded[s].lo[a]));
    hi[a] = __longlong_as_double((long long)segment_order_unkey64(box_folded[s].hi[a]));
  }
  icpgpu_segment_record r;
#pragma unroll
  for (int t = 0; t < 9; ++t) r.axes[t] = records[s].axes[t];
#pragma unroll
  for (int a = 0; a < 3; ++a) r.K[a] = records[s].K[a];
  segment_finish_box(r, lo, hi);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    records[s].obb_lo[a] = r.obb_lo[a];
    records[s].obb_hi[a] = r.obb_hi[a];
    records[s].obb_position[a] = r.obb_position[a];
    records[s].obb_dims[a] = r.obb_dims[a];
  }
}

}  // namespace

hipError_t launch_segment_moments(const float4* cloud, int n, const int* start, const int* list, int n_segments, int total, int* seg_of,
                                  unsigned int* first, SegmentPartial* partials, SegmentBoxPartial* box_partials, void* records, hipStream_t stream) {
  if (n_segments <= 0) return hipSuccess;
  if (total > 0 && n <= 0) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(first, 0xFF, (size_t)n_segments * sizeof(unsigned int), stream);
  if (e != hipSuccess) return e;
  icpgpu_segment_record* rec = static_cast<icpgpu_segment_record*>(records);
  const dim3 block(SEG_BLOCK), per_entry((unsigned int)(((size_t)total + SEG_BLOCK - 1) / SEG_BLOCK)),
      per_segment((unsigned int)((n_segments + SEG_BLOCK - 1) / SEG_BLOCK)),
      wave_per_segment((unsigned int)(((size_t)n_segments + SEG_BLOCK / 64 - 1) / (SEG_BLOCK / 64)));
  // the segments' folded partials lie behind the pieces' slots
  SegmentPartial* folded = partials + segment_slots((size_t)n_segments, (size_t)total);
  SegmentBoxPartial* box_folded = box_partials + segment_slots((size_t)n_segments, (size_t)total);
  if (total > 0) {
    hipLaunchKernelGGL(segment_first_kernel, per_entry, block, 0, stream, cloud, n, start, list, n_segments, total, seg_of, first);
    hipLaunchKernelGGL(segment_sums_kernel, per_entry, block, 0, stream, cloud, n, list, total, seg_of, first, partials);
    hipLaunchKernelGGL(segment_fold_kernel, wave_per_segment, block, 0, stream, start, n_segments, first, partials, folded);
  }
  hipLaunchKernelGGL(segment_finish_kernel, per_segment, block, 0, stream, cloud, n, start, list, n_segments, first, folded, rec);
  if (total > 0) {
    hipLaunchKernelGGL(segment_box_kernel, per_entry, block, 0, stream, cloud, n, list, total, seg_of, rec, box_partials);
    hipLaunchKernelGGL(segment_box_fold_kernel, wave_per_segment, block, 0, stream, start, n_segments, first, box_partials, box_folded);
    hipLaunchKernelGGL(segment_box_finish_kernel, per_segment, block, 0, stream, n_segments, box_folded, rec);
  }
  return hipGetLastError();
}

}  // namespace icpgpu
