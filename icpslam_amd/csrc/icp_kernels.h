// icp_kernels.h -- launch wrappers for the gfx950 kernels of the ICP hot path (internal).
//
// Rows of SURVEY.md §8(a) implemented here:
//   a2  nearest-neighbour correspondence search   -> launch_nn_brute()
//   a3  outlier rejection (d2 <= r^2 predicate)   -> fused into launch_reduce()
//   a4  centroid / cross-covariance reduction     -> launch_reduce()
//   a6  point-set transform                       -> fused into a2/a4 loads; launch_transform() for the output cloud
//   a9  fitness score                             -> a2 + launch_reduce() with an open threshold
// Reference call sites these replace: /root/reference/src/icpslam/icp_odometer.cpp:198-201,
// /root/reference/src/icpslam/octree_mapper.cpp:114-117 (the arithmetic itself lives in PCL).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icp_brute_plan.h"

namespace icpgpu {

// Rigid transform as 12 floats (row-major 3x4) so that it travels in SGPRs as a kernel argument.
// ---- the result mailbox's pairs --------------------------------------------------------------------------------------------
// Every value the host (or another workgroup) waits for travels as a 16-byte pair {value bits, tag}, tag = the number of the
// sweep / evaluation it belongs to and a 24-bit checksum of the value's bits.  The pair leaves the device as ONE 16-byte
// write-through store (icp_device.h: store_pair_system) and has never been seen half-written on gfx950; but the reader does
// not rely on that: it accepts a pair only if the tag carries the number it waits for AND the checksum of the bits it read --
// a torn observation (new tag, old value, or the other way round) fails the check and is simply read again.  So a pair is
// valid or recognisably not, in whatever order its halves become visible (until round 4 correctness rested on the pair
// never being seen torn: VERDICT r3).  ICPGPU_MAILBOX=release (or a torn pair seen by the start-up self-test) selects the
// slower classic form on the device side -- value, system-scope release fence, tag -- signalled to the kernels by
// kMailboxReleaseBit in the number they are handed; the reader is the same.
#if defined(__HIPCC__)
#define ICPGPU_HD __host__ __device__
#else
#define ICPGPU_HD
#endif
static constexpr unsigned long long kMailboxReleaseBit = 1ull << 62;
ICPGPU_HD inline unsigned long long mailbox_tag(unsigned long long seq, unsigned long long bits) {  // seq < 2^38
  return (seq << 24) | ((bits ^ (bits >> 24) ^ (bits >> 48)) & 0xFFFFFFull);
}
// host side: true and the value bits if the pair carries number seq and its own checksum
inline bool mailbox_read(const volatile unsigned long long* pair, unsigned long long seq, unsigned long long* bits_out) {
  const unsigned long long tag = pair[1], bits = pair[0];
  if (tag != mailbox_tag(seq, bits)) return false;
  *bits_out = bits;
  return true;
}

struct Xform {
  float m[12];
};

// 64-bit correspondence key: (float bits of d2) << 32 | target index. For d2 >= 0 the unsigned order of
// the key is (d2, index) lexicographic, so a u64 min merges partial searches and breaks ties on the lowest index.
static constexpr int kGridStatInts = 6;
static constexpr unsigned long long kEmptyKey = 0xFFFFFFFFFFFFFFFFull;
static constexpr unsigned int kNoPrev = 0xFFFFFFFFu;  // previous-neighbour position: none (launch_nn_grid_search)

static constexpr int kReduceTerms = 17;   // n, Sp(3), Sq(3), Sqp(9), Sd2
static constexpr int kMaxReduceBlocks = 1024;

struct NnPlan {
  int variant;        // 0 LDS-tiled, 1 scalar-load, 2 LDS + packed f32; +10 = 8 points per lane (tuning knob)
  int splits;         // target splits (grid.y)
  int tgt_per_split;  // multiple of the LDS tile
  int grid_x;
};

NnPlan plan_nn_brute(int n_s, int n_t, int variant, int num_cus);

// The launch shape of a matrix-core brute-force sweep (MatrixNnPlan and its arithmetic: icp_brute_plan.h), with each unit's
// development switches applied.  The launchers launch what these say; nn_keys_brute prints it under ICPGPU_DEBUG.
MatrixNnPlan plan_nn_brute_mfma(int n_q, int n_t, int num_cus);
MatrixNnPlan plan_nn_brute_bf16(int n_q, int n_t, int num_cus, bool check);
// ICPGPU_MFMA_NO_EXACT (a timing experiment: the exact path is skipped, results are WRONG), read and warned about once per process
int matrix_nn_no_exact();
// the launch line of both launchers: `kernel` over the plan's grid with the arguments the two kernels share, then `extra`
template <typename Kernel, typename... Extra>
void launch_matrix_nn(Kernel kernel, const MatrixNnPlan& plan, hipStream_t stream, const float4* src_sorted, int n_q, const float4* tgt,
                      int n_t, const Xform& T, unsigned long long* keys, const unsigned long long* seed, Extra... extra) {
  hipLaunchKernelGGL(kernel, dim3(plan.grid_x, plan.splits), dim3(plan.block), 0, stream, src_sorted, n_q, tgt, n_t, T,
                     plan.tgt_per_split, plan.splits, keys, seed, matrix_nn_no_exact(), extra...);
}
// (the plain kernel's shape for the same line: NN_TILE, NN_BLOCK, source points per lane)
void nn_brute_shape(const NnPlan& plan, int* tile, int* block, int* per_lane);

// keys[i] = min over target of (d2, j) for p = T*src[i]. When plan.splits > 1 keys must be pre-filled with kEmptyKey.
hipError_t launch_nn_brute(const float4* src, int n_s, const float4* tgt, int n_t, const Xform& T, const NnPlan& plan,
                           unsigned long long* keys, hipStream_t stream);

// partials: [blocks][17] doubles, sums_out: 17 doubles (device). Deterministic (fixed order) two-stage reduction.
// The same keys from the matrix cores (icp_brute_mfma.hip).  src_sorted: the source in cell order, ORIGINAL index in .w (a
// grid's sorted copy); keys are written at the original indices and must be pre-filled with kEmptyKey.
// seed (nullable): n_s keys of an earlier sweep of the same source over the SAME target array -- each source's old neighbour
// bounds its search from the first tile on.
hipError_t launch_nn_brute_mfma(const float4* src_sorted, int n_q, const float4* tgt, int n_t, const Xform& T, int num_cus,
                                unsigned long long* keys, const unsigned long long* seed, hipStream_t stream);

// The same keys again with the lower bound on the bf16 matrix path (icp_brute_bf16.hip: split operands, one K = 16 MFMA per
// 32 x 32 pairs, vector work overlapped).  src_morton: launch_morton_order's output.  check (nullable): 2 x u64 zeroed by the
// caller -- the test mode's counters (pairs whose bound was too high; worst excess as float bits in the low half of [1]).
struct GridDesc;
size_t morton_order_work_ints(int n);
hipError_t launch_morton_order(const float4* sorted, int n, const GridDesc& g, int* work, float4* out, hipStream_t stream);
hipError_t launch_nn_brute_bf16(const float4* src_morton, int n_q, const float4* tgt, int n_t, const Xform& T, int num_cus,
                                unsigned long long* keys, const unsigned long long* seed, unsigned long long* check,
                                hipStream_t stream);

// The grid search on the matrix cores (icp_tile.hip): keys[orig source index] = exact NN within sqrt(thr) (else left empty:
// pre-fill with kEmptyKey), found by offering every workgroup of 256 Morton-ordered sources the target points of the grid cells
// their search balls touch, through the bf16 lower-bound filter.  seed (nullable): the previous sweep's keys.
hipError_t launch_nn_tile_search(const float4* src_morton, int n_q, const Xform& T, const float4* sorted, const int* cell_start,
                                 const GridDesc& g, const float4* tgt, int n_t, float thr, const unsigned long long* seed,
                                 float4* prev, bool use_prev, unsigned long long* keys, unsigned long long* stats,
                                 hipStream_t stream);

hipError_t launch_reduce(const float4* src, int n_s, const float4* tgt, const unsigned long long* keys, const Xform& T,
                         float d2_threshold, double* partials, double* sums_out, unsigned long long* flags,
                         unsigned long long seq, hipStream_t stream);

// flags (nullable; 34 64-bit words, host-mapped, 16-byte aligned): term k's workgroup stores the pair {sum bits, seq} at
// words 2k, 2k + 1 in ONE 16-byte write-through store, so the host can poll instead of synchronising the stream and never
// sees a sum without its number; sums_out is then left alone.  Without flags the sums go to sums_out (device memory).
// term_major: partials are laid out [term][block] (what launch_nn_grid_search writes) instead of [block][term].
hipError_t launch_mailbox_selftest(unsigned long long* pair_dev, int rounds, hipStream_t stream);
// n <= 32 ints of device memory as result pairs {value, tag(number)} into mapped host memory (the host polls them)
hipError_t launch_post_ints(const int* d_src, int n, unsigned long long* pairs_dev, unsigned long long number, hipStream_t stream);
hipError_t launch_reduce_final(const double* partials, int n_blocks, bool term_major, double* sums_out,
                               unsigned long long* flags, unsigned long long seq, hipStream_t stream);

hipError_t launch_transform(const float4* src, int n_s, const Xform& T, float4* out, hipStream_t stream);

hipError_t launch_fill_keys(unsigned long long* keys, int n, hipStream_t stream);

// Content fingerprint of a cloud (icpgpu_set_target's recognition of the previous source): the SUM over the points of a
// 64-bit mix of (bits of the point, its index), plus a mix of n -- an order-independent sum, so the host (a loop) and the
// device (any grid) compute the same number.  Two different clouds collide with probability ~2^-64.
ICPGPU_HD inline unsigned long long fp_mix(unsigned long long x) {  // splitmix64's finaliser
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}
ICPGPU_HD inline unsigned long long fp_point(unsigned long long w0, unsigned long long w1, unsigned long long i) {
  return fp_mix(w0 + 0x9e3779b97f4a7c15ull * (2ull * i + 1ull)) + fp_mix(w1 ^ (0xd6e8feb86659fd93ull * (2ull * i + 2ull)));
}
ICPGPU_HD inline unsigned long long fp_finish(unsigned long long sum, unsigned long long n) { return sum + fp_mix(n ^ 0xa5a5a5a5a5a5a5a5ull); }
// *d_acc (zeroed by the launcher) receives the sum of fp_point over pts[0..n)
hipError_t launch_fingerprint(const float4* pts, int n, unsigned long long* d_acc, hipStream_t stream);

// pts[0 .. min(d_counts[0] + d_counts[1], cap)) into host-mapped memory with 16-byte stores, *d_acc (ZERO before: the voxel
// filter's last kernel clears it) += the sum of fp_point over them (the voxel filter's result on its way to the caller: icpgpu_voxel_grid_view); n_most sizes the launch
hipError_t launch_publish_cloud(const float4* pts, const int* d_counts, int n_most, int cap, float4* host_out, unsigned long long* d_acc,
                                hipStream_t stream);

// keys -> (idx, d2) arrays for the kernel-level C-ABI entry point.
hipError_t launch_unpack_keys(const unsigned long long* keys, int n, int32_t* idx, float* d2, hipStream_t stream);

// ---- uniform-grid accelerated exact NN (icp_grid.hip) -------------------------------------------------------
// Target points are counting-sorted by cell (x fastest) into `sorted` (xyz + original index bits in w); a query
// searches the 3x3x3 block of cells around it, then cubes of growing Chebyshev radius, and stops as soon as the
// best squared distance is provably smaller than anything outside the searched cube.
struct GridDesc {
  float ox, oy, oz;  // origin (min corner)
  float h, inv_h;    // cell size
  int nx, ny, nz;
  int sy, sz;        // cell index = cz * sz + cy * sy + cx: x is always the fastest axis (a cell row = one x run); the
                     // thinner of y / z comes next, so that the layers of a flat scene stay close together in memory
  int r_max;         // last cube radius searched: r_max * h * kGridSafety >= cutoff distance
};
static constexpr float kGridSafety = 0.984375f;  // 63/64: covers the rounding of the float binning
static constexpr int kScanItems = 4096;           // elements per block of the cell-count scan

// encoded min/max (6 ints, see decode_bbox) of the finite points of a cloud
hipError_t launch_bbox(const float4* pts, int n, int* d_minmax6, hipStream_t stream, bool init = true);  // init = false: d_minmax6 holds the initial values already
void decode_bbox(const int enc[6], float lo[3], float hi[3]);  // host

// Produces cell_start (exclusive scan of the per-cell counts, ncells+1 entries, in place in counts_then_start),
// sorted[n_valid], d_stats2 = {n_valid, max cell population}.
// Two halves so that the host can look at the occupancy statistics (and pick another cell size) before paying for the
// scan and the scatter.  d_stats (kGridStatInts ints): [0] binned points (valid after finish), [1] largest cell
// population, [2..3] u64 sum of squared populations, [4] binned points (valid after count).
hipError_t launch_grid_count(const float4* pts, int n, const GridDesc& g, int* cell_of_point, int* rank_in_cell,
                             int* counts_then_start, int* block_sums, int* d_stats, hipStream_t stream);
// orig_index (nullable): sorted[].w carries orig_index[i] instead of i (see icpgpu_map_nn_target)
hipError_t launch_grid_finish(const float4* pts, int n, const GridDesc& g, const int* cell_of_point,
                              const int* rank_in_cell, int* counts_then_start, int* block_sums, int* d_stats,
                              const int* orig_index, float4* sorted, hipStream_t stream);

// Exact NN of T*src[i] among the grid's points, guaranteed whenever the NN lies within the cutoff the grid was built
// for; otherwise the point is reported unmatched (empty key).  nn_quad_kernel / nn_wave_kernel (see icp_grid.hip).
//   keys      : optional (nullptr to skip) 8-byte keys with ORIGINAL target indices
//   partials  : optional fused a3+a4 reduction: 17 x grid_search_blocks(n_s) doubles, TERM-major (partials[k * blocks + b])
//   unmatched : optional compaction of unmatched source indices (count at unmatched_count[0], pre-zeroed)
// flags: kGridSrcInCellOrder (XCD-contiguous workgroup mapping), kGridPackShortRows (sparse targets: four short rows per
// step in the cube search), kGridOver4GiB (2^28 or more binned points: nn_quad_kernel's 32-bit byte offsets do not reach,
// nn_wave_kernel takes over)
static constexpr int kGridSrcInCellOrder = 1, kGridPackShortRows = 2, kGridOver4GiB = 4;
// ---- lock-step sweeps over several independent pairs (icpgpu_align_batch) -------------------------------------------
constexpr int kBatchMax = 16;
struct BatchPair {  // what stays the same for a pair from sweep to sweep (a table in device memory)
  const float4* src;
  const float4* sorted;
  const int* cell_start;
  double* partials;
  unsigned int* prev_nn;      // the pair's previous-neighbour positions (below)
  unsigned long long* flags;  // the pair's result mailbox (device alias of pinned host memory)
  unsigned long long* keys;   // ungated (getFitnessScore) sweep: the pair's key array, its list of unmatched points + counter
  int* unmatched;
  int* unmatched_count;
  int r_max_open;             // ... and how far its cubes may grow (nn_keys_grid)
  GridDesc g;
  float accept_thr;
  int n_s, qpw, xcd_map, blocks;
};
struct BatchStep {  // what changes: passed by value with every launch (kernel arguments)
  Xform T[kBatchMax];
  unsigned long long seq[kBatchMax];
  unsigned char slot[kBatchMax];  // blockIdx.y -> row of the table
  unsigned int use_prev_mask;     // bit y: the pair's previous-neighbour buffer holds its last sweep
};
bool grid_search_batchable(int n_s, int flags);
int grid_search_qpw(int n_s);
hipError_t launch_nn_grid_search_batch(const BatchPair* d_pairs, const BatchStep& step, int n_active, int max_blocks, bool pack,
                                       bool open_range, hipStream_t stream);
hipError_t launch_reduce_final_batch(const BatchPair* d_pairs, const BatchStep& step, int n_active, hipStream_t stream);

hipError_t launch_nn_grid_search(const float4* src, int n_s, int flags, const Xform& T, const float4* sorted,
                                 const int* cell_start, const GridDesc& g, float accept_thr, unsigned long long* keys,
                                 double* partials, int* unmatched, int* unmatched_count, hipStream_t stream,
                                 unsigned int* prev_nn = nullptr, bool use_prev = false);
int grid_search_blocks(int n_s);
// Counting runs only (process-wide, not thread-safe): every nn_quad_kernel launch adds the number of target points it
// evaluates to *device_counter; nullptr switches the counting off again.
void grid_count_candidates(unsigned long long* device_counter);
// prev_nn (optional, n_s x 4 bytes): where in `sorted` (byte offset; kNoPrev: nowhere) the neighbour each point found sits,
// written by every sweep of nn_quad_kernel and, with
// use_prev, read back by the next one as an upper bound that prunes its search (valid for ANY transform, but only against
// the same target points and the same src array).  True when launch_nn_grid_search would use it for this size.
bool grid_search_keeps_prev(int n_s, int flags);

// brute force for a list of source indices (fallback for points the grid could not match); keys pre-filled empty.
// the same for at most kFewQueries listed queries, whose number may live in device memory (count_ptr, else n_list): the
// kernel then does nothing for 0 or more than kFewQueries of them and reports the number in *count_out (device-visible)
static constexpr int kFewQueries = 64;
hipError_t launch_nn_brute_few(const float4* src, const int* list, const int* count_ptr, int n_list, const float4* tgt, int n_t,
                               const Xform& T, unsigned long long* keys, int* count_out, hipStream_t stream);
hipError_t launch_nn_brute_list(const float4* src, const int* list, int n_list, const float4* tgt, int n_t,
                                const Xform& T, int num_cus, unsigned long long* keys, hipStream_t stream);

// ---- GICP mode (icp_gicp_cov.hip, icp_gicp.hip, icp_gicp_solve*.hip), SURVEY.md 8(f1) ----------------------------------------------------------------
static constexpr int kGicpK = 20;              // PCL k_correspondences_
static constexpr double kGicpEpsilon = 1e-3;   // PCL gicp_epsilon_
struct Rot3d {
  double m[9];  // row-major
};
static constexpr int kGicpCovFarMost = 1 << 16;  // clouds up to this size: the far-field kernel (a workgroup over the whole cloud per point)
// the covariances of a cloud that has no grid (n <= kGicpCovFarMost): every point through the far-field kernel; list as below
hipError_t launch_gicp_covariances_brute(const float4* cloud, int n, double* cov6, hipStream_t stream, int* list, bool list_counters_zero,
                                         float4* normals = nullptr);
// cov6[i] = upper triangle (xx, xy, xz, yy, yz, zz) of the regularised covariance of point i's 20 nearest neighbours
// normals (optional, n float4): the point-to-plane mode's surface normals instead (gicp_normal_finish_kernel): cov6 is then left
// holding the RAW covariances, scratch for the caller
hipError_t launch_gicp_covariances(const float4* cloud, int n, const float4* sorted, const int* cell_start,
                                   const GridDesc& g, double* cov6, hipStream_t stream, int* list = nullptr, bool list_counters_zero = false,
                                   float4* normals = nullptr);
// (list: 2 n + 2 ints of scratch -- the points the selecting kernel hands to the far-field and the streaming kernel; icp_gicp_cov.hip.
//  list_counters_zero: list[0] and list[1] are zero -- true from the second cloud on the same buffer: the last kernel leaves them so)
// maha6[i] = upper triangle of (C_t[j] + R C_s[i] R^T)^-1 for every source point whose key passes d2 < thr
hipError_t launch_gicp_mahalanobis(int n_s, const unsigned long long* keys, float thr, const Rot3d& R, const double* cov_s,
                                   const double* cov_t, double* maha6, hipStream_t stream);
// One BFGS function/gradient evaluation: at most kGicpDirectBlocks workgroups, each stores its partial sums straight into
// host-mapped memory (host_partials[block * kGicpPartialStride + ...]: [0] = m, [1..13] = high parts of sum r^T M r, sum M r
// (3), sum (base p)(M r)^T (9), [14] = sum d2, [16..28] = the 13 low parts -- the sums are double-double, see icp_gicp_device.h)
// followed by host_flags[block] = seq; the host adds the partials in block order.  blocks = gicp_direct_blocks(n_s, share).
// Since round 2 every value travels WITH its sequence number: entry e of a block is the 16-byte pair {value, tag} at doubles
// [2e, 2e + 1], written by ONE 16-byte store -- a pair is never seen half-written, so no flag and no system-scope release
// (a write-back + a wait for the earlier stores' acknowledgements, 1-1.5 us) stands between the sums and the host; the host
// takes a block's entry when its tag equals the evaluation's number.
// Since round 5 a workgroup's answer is four ANSWER LINES of 64 bytes instead of 28 pairs: line L = doubles [8 L, 8 L + 8) of the
// block's stride, seven values (numbers 7 L .. 7 L + 6 of: m, the 13 high parts, sum d2, the 13 low parts) and, in its last word,
// the tag (evaluation number << 24) | XOR of the 24-bit folds of the seven values' bits -- written by ONE store instruction,
// four 64-byte requests instead of seven; the host takes a block's lines when all four tags carry the evaluation's number and
// their checksums (gicp_line_read).
static constexpr int kGicpPartialStride = 64;
static constexpr int kGicpLines = 4;
inline unsigned long long gicp_line_fold(unsigned long long bits) { return (bits ^ (bits >> 24) ^ (bits >> 48)) & 0xFFFFFFull; }
// host side: value number s (0 = m, 1..13 high parts, 14 = sum d2, 15..27 low parts) of a block whose lines have been validated
inline double gicp_line_value(const volatile double* block, int s) { return block[8 * (s / 7) + (s % 7)]; }
static constexpr int kGicpDirectBlocks = 256;  // capacity of the mailbox; gicp_direct_blocks() may use fewer
int gicp_direct_blocks(int n_s, int most = kGicpDirectBlocks);
hipError_t launch_gicp_cost_direct(int blocks, const float4* src, int n_s, const float4* tgt, const unsigned long long* keys, float thr,
                                   const Xform& T, const Xform& base, const double* maha6, double* host_partials,
                                   unsigned long long* host_flags, unsigned long long seq, hipStream_t stream);

// Resident variant for a whole BFGS run (icp_gicp.hip): the kernel waits for commands in a line of fine-grained device
// memory the host writes through the BAR (cmd: 12 floats of T, then the sequence number), evaluates, answers through
// host_partials / host_flags like the direct kernel (flag = seq_hi << 32 | sequence number) and leaves on sequence number
// kGicpServerExit (acknowledged by host_flags[0] = ~0) or after 50 ms without a command.
// The device solver (icp_gicp_solve_device.h: gicp_solve_kernel): the whole BFGS run of an outer iteration inside one resident kernel.
// slots: gicp_solve_slot_bytes(blocks) of FINE-GRAINED device memory; host_out: gicp_solve_out_granules() granules (16 B each) of
// the host mailbox -- granule 0 the status (gicp::Status), 1..6 the state, 7 m, 8 sum d2, 9 f at the start, 10 evaluations --
// each carrying number seq0 and a checksum (gicp_granule_read).  Evaluation e of the run uses number seq0 + e.
size_t gicp_solve_slot_bytes(int blocks);
int gicp_solve_out_granules();
hipError_t launch_gicp_solve(int blocks, const float4* src, int n_s, const float4* tgt, const unsigned long long* keys, float thr,
                             const Xform& base, const float guess[16], const double* maha6, const double x0[6],
                             unsigned long long* slots, unsigned long long* host_out, unsigned long long seq0, int max_inner,
                             double gradient_tol, hipStream_t stream, unsigned long long* local_slots = nullptr,
                             unsigned long long* owner = nullptr, int xcc_want = 0);
// one-XCD variant (local_slots / owner given, <= gicp_solve_local_blocks() workgroups, correspondences resident): ordinary device
// memory (gicp_solve_slot_bytes) for the granules, kGicpDirectBlocks words for the worker claims
int gicp_solve_local_blocks();
// Several runs' device solvers in one launch (gicp_solve_batch_kernel): every item a RESIDENT run (blocks x 1024 >= n_s) with its
// own slots / host_out / numbers, as launch_gicp_solve takes them (seq0 may carry kMailboxReleaseBit); any placement.
constexpr int kGicpSolveBatchMax = 8;
struct GicpSolveItem {
  const float4* src;
  int n_s;
  const float4* tgt;
  const unsigned long long* keys;
  float thr;
  Xform base;
  float guess[16];
  const double* maha6;
  double x0[6];
  unsigned long long* slots;
  unsigned long long* host_out;
  unsigned long long seq0;
  int blocks;
};
hipError_t launch_gicp_solve_batch(const GicpSolveItem* items, int n, int max_inner, double gradient_tol, hipStream_t stream);
bool gicp_granule_read(const volatile unsigned long long* g, unsigned long long seq, double* value);
// The quadratic form of an outer iteration (icp_gicp_quadratic.h, icp_gicp.hip: gicp_quadratic_kernel): kGicpQuadSums
// double-double sums over the correspondences whose key passes d2 < thr, Mahalanobis matrices computed on the way (R: the rotation
// launch_gicp_mahalanobis takes).  partials: gicp_quadratic_blocks(n_s) x kGicpQuadSums x 2 doubles of device memory, done: a zeroed
// device word; host_out: 2 x kGicpQuadSums result pairs (16 B each) numbered seq -- pair 2 n the high part of sum n, 2 n + 1 its low
// part (gicp_granule_read).
static constexpr int kGicpQuadSums = 75;
static constexpr int kGicpQuadBlocks = 256;
int gicp_quadratic_blocks(int n_s);
hipError_t launch_gicp_quadratic(const float4* src, int n_s, const float4* tgt, const unsigned long long* keys, float thr,
                                 const Rot3d& R, const double* cov_s, const double* cov_t, double* partials, unsigned int* done,
                                 unsigned long long* host_out, unsigned long long seq, hipStream_t stream);
static constexpr unsigned int kGicpServerExit = 0xFFFFFFFFu;
hipError_t launch_gicp_server(int blocks, const float4* src, int n_s, const float4* tgt, const unsigned long long* keys, float thr,
                              const Xform& base, const double* maha6, double* host_partials, unsigned long long* host_flags,
                              unsigned int* cmd, unsigned int first_seq, unsigned int seq_hi, hipStream_t stream);

// ---- point-to-plane mode (icp_p2plane.hip): pcl::IterativeClosestPointWithNormals + TransformationEstimationPointToPlaneLLS --
// sums[29] over the pairs of a key sweep whose d2 <= thr (the point-to-point accept rule): [0] n, [1] sum d2, [2..22] the upper
// triangle of A^T A over (a, b, c, nx, ny, nz) row by row, [23..28] A^T r -- pairs whose target normal is not finite count in [0]
// and [1] only.  partials: p2plane_blocks(n_s) x kP2planeTerms doubles of device memory.  Like launch_reduce: with flags the 29
// sums go to the host mailbox as result pairs numbered seq (words 2k, 2k + 1), otherwise to sums_out (device memory).
static constexpr int kP2planeTerms = 29;
int p2plane_blocks(int n_s);
hipError_t launch_p2plane_reduce(const float4* src, int n_s, const float4* tgt, const float4* normals, const unsigned long long* keys,
                                 const Xform& T, float thr, double* partials, double* sums_out, unsigned long long* flags,
                                 unsigned long long seq, hipStream_t stream);
// the symmetric objective's sums in the same layout (TransformationEstimationSymmetricPointToPlaneLLS): src_normals = the source's
// normals as stored (n_s float4; the kernel rotates them by T), v = ((p + q) x n, n), r = (q - p) . n with n = n1 + n2, or n1 - n2
// where enforce is set and !(n1 . n2 >= 0); a pair whose n is not finite counts in [0] and [1] only.  Same partials, same final kernel.
hipError_t launch_p2plane_sym_reduce(const float4* src, const float4* src_normals, int n_s, const float4* tgt, const float4* normals,
                                     const unsigned long long* keys, const Xform& T, float thr, bool enforce, double* partials,
                                     double* sums_out, unsigned long long* flags, unsigned long long seq, hipStream_t stream);
// the p2plane final kernel alone: partials (n_blocks x 29 doubles, block-major) -> the first n_terms of the 29 sums, fixed order
// (NDT's derivative and trial passes)
hipError_t launch_terms29_final(const double* partials, int n_blocks, double* sums_out, unsigned long long* flags, unsigned long long seq,
                                hipStream_t stream, int n_terms = 29);

// ---- correspondence rejectors (icp_reject.hip): stages between a key-writing search and a keys reduction ---------------------
// A stage rewrites the keys of the pairs it rejects to kEmptyKey; a pair is alive when its key names a target and its d2 <= thr.
static constexpr int kRejectMedian = 1, kRejectTrimmed = 2, kRejectOneToOne = 3, kRejectSurfaceNormal = 4;  // = icpgpu_rejector_kind
static constexpr int kRejectSampleConsensus = 5;  // (a stage of the HOST's: icpgpu_reject_sac.cpp; launch_reject_chain refuses it)
static constexpr int kRejectMaxStages = 4;
struct RejectStage {
  int kind;
  unsigned int min_corr;  // trimmed
  float ratio;            // trimmed: overlap ratio (float, as PCL holds it)
  double factor;          // median: the factor; surface normal: the threshold (cosine of the largest accepted angle)
};
// per stage, unsigned ints of device memory: the radix select's three histograms (digits of 11, 11, 10 bits), then the statistics
// {pairs in, pairs out, bits of the cut (float d2; 0 where a stage has none), 0}
static constexpr int kRejectHist0 = 0, kRejectHist1 = 2048, kRejectHist2 = 4096, kRejectStats = 5120, kRejectStateInts = 5128;
// state: n_stages x kRejectStateInts ints; winners: n_t 64-bit words (one-to-one stages only, else may be null); src_normals
// (n_s float4, as stored), tgt_normals (n_t float4) and T (the iteration's transform: it rotates the source's normals): surface-normal
// stages only
hipError_t launch_reject_chain(unsigned long long* keys, int n_s, int n_t, float thr, const RejectStage* stages, int n_stages,
                               unsigned int* state, unsigned long long* winners, hipStream_t stream, const float4* src_normals = nullptr,
                               const float4* tgt_normals = nullptr, const Xform* T = nullptr);
// keys -> (idx, d2) for icpgpu_correspondences: idx = -1, d2 = +inf for a pair that is not alive
hipError_t launch_reject_unpack(const unsigned long long* keys, int n, float thr, int32_t* idx, float* d2, hipStream_t stream);

// ---- reciprocal correspondences (icp_reciprocal.hip): a stage in front of the rejector chain ---------------------------------
// Empties the key of every alive pair (i, j) for which x_i = T * src[i] is not the nearest of all x_* to tgt[j] (dist2(tgt[j], x_k),
// lowest k among equals).  state: kRecipStateInts unsigned ints of device memory = {pairs alive before, pairs kept, 0, 0};
// winners: n_t 64-bit words of scratch.
static constexpr int kRecipStateInts = 4;
// grid flavour: x_* binned into the lattice g of the target's grid.  counts, cell_start: reciprocal_cells(g) + 1 ints each;
// scan_scratch: exclusive_scan_scratch_ints(reciprocal_cells(g) + 1) ints; cell_of_point, rank: n_s ints each; binned: n_s float4
size_t reciprocal_cells(const GridDesc& g);
hipError_t launch_reciprocal_grid(const float4* src, int n_s, const float4* tgt, int n_t, const Xform& T, float thr,
                                  unsigned long long* keys, const GridDesc& g, int* counts, int* cell_start, int* scan_scratch,
                                  int* cell_of_point, int* rank, float4* binned, unsigned long long* winners, unsigned int* state,
                                  hipStream_t stream);
// brute flavour: every winner against all of x_* (no grid needed)
hipError_t launch_reciprocal_brute(const float4* src, int n_s, const float4* tgt, int n_t, const Xform& T, float thr,
                                   unsigned long long* keys, unsigned long long* winners, unsigned int* state, hipStream_t stream);

// ---- NDT (icp_ndt.hip): pcl::NormalDistributionsTransform's target cells and derivative pass ----------------------------
static constexpr int kNdtTerms = 29;         // pairs, score, gradient (6), Hessian upper triangle row by row (21)
static constexpr int kNdtGradTerms = 8;      // the trial pass's: pairs, score, gradient (6) -- the first 8 of the 29
static constexpr int kNdtGaussDoubles = 10;  // per valid cell: mean (3), icov xx xy xz yy yz zz (6), pad
static constexpr int kNdtMinPoints = 6;      // VoxelGridCovariance's min_points_per_voxel_
static constexpr double kNdtEigRatio = 0.01; // VoxelGridCovariance's min_covar_eigvalue_mult_
static constexpr int kNdtJacobiSweeps = 8;   // cyclic Jacobi sweeps of a cell's 3x3 covariance (converged well before)
// the cell lattice: the voxel filter's min_b / div_b at leaf = resolution (key = ix + iy mul_y + iz mul_z, ix .. relative to minb)
struct NdtLattice {
  int minb[3], divb[3];
  int mul_y, mul_z;
  float inv_leaf_f;  // 1.0f / (float)resolution, as PCL's inverse_leaf_size_
  double inv_leaf;   // the same value in double
};
// what an evaluation needs besides the clouds: radius, stencil widening, Gauss constants, the host's angle terms (PCL's j_ang_a.._h
// and h_ang_a2 .. f3, in that order)
struct NdtPass {
  double r_wide;   // resolution * (1 + 1e-6): bounds |c - q| per axis for every pair the float radius test accepts
  double excess;   // the cells' largest centroid excursion outside their own cell (cell units; ndt_stats_kernel)
  double d1, d2;   // gauss_d1_, gauss_d2_
  float r2f;       // float(resolution^2)
  double j_ang[8][3];
  double h_ang[15][3];
};
// keys / vals: 2 n ints each (sorted halves second); temp: radix_sort_scratch_ints(n) and exclusive_scan_scratch_ints(n) ints
hipError_t launch_ndt_keys(const float4* pts, int n, const NdtLattice& L, int* keys, int* vals, int* temp, hipStream_t stream);
// every cell of the sorted points -> per-cell records (n-sized scratch), the valid ones compacted into out_* in key order;
// stats = {valid cells, largest excess as double bits (2 ints)}
hipError_t launch_ndt_cells(const float4* pts, int n, const NdtLattice& L, const int* sorted_keys, const int* sorted_vals, int* flags,
                            int* slots, int* temp, int* valid, int* vslots, int* ckey, float4* cent, double* gauss, int* npts,
                            double* excess, int* out_key, float4* out_cent, double* out_gauss, int* out_n, int* stats,
                            hipStream_t stream);
int ndt_blocks(int n_s);
// one evaluation: partials = ndt_blocks(n_s) x 29 doubles; with flags the sums go into the mailbox, else to sums_out (device).
// hessian: the 29 sums (ndt_deriv_kernel); else the first 8 only (ndt_grad_kernel), the same bits as the 29-term pass's first 8
hipError_t launch_ndt_derivatives(const float4* src, int n_s, const Xform& T, const NdtLattice& L, const NdtPass& P, const int* ckey,
                                  const float4* cent, const double* gauss, int n_cells, double* partials, double* sums_out,
                                  unsigned long long* flags, unsigned long long seq, hipStream_t stream, bool hessian = true);


// ---- the mapper's one-point-per-voxel map (icp_map.hip), SURVEY.md 8(f4) --------------------------------------------
struct MapDesc {
  double res;  // voxel size (octree_resolution_, 0.5 m); the voxel keys come from the octree's box (ApproxBox / ApproxHistory)
};
// PCL's octree geometry (OctreePointCloud, octree_pointcloud.hpp): the bounding box as adoptBoundingBoxToPoint has grown it, in
// double; depth = levels below the root (side = 2^depth voxels); shift = whole voxels the minimum has moved since the first
// box; origin = the first box's minimum
struct ApproxBox {
  double min[3], max[3];
  double origin[3];
  long long shift[3];
  double res;
  int depth;
};
// PCL keys a point ONCE, from the bounding box in force when the point is tested (genOctreeKeyforPoint), and re-roots the tree
// when the box doubles -- a stored key then moves by whole voxels with the minimum; it is never recomputed from the new minimum
// (which could round the other way for a point on a voxel face; a resolution that is not a power of two makes the minimum
// round as it moves).  Map keys are therefore kept in the first box's frame: trunc((p - min[v]) / res) - shift[v] under the box
// version v in force for the point.  The versions of one insertion batch: version k is in force from batch index first[k] on
// (first = -1: carried over from earlier batches); the point AT first[k] grew the box (or was the first point of the map) and
// is appended whatever its key holds, isVoxelOccupiedAtPoint() being false outside the box.
constexpr int kApproxMaxVersions = 24;
struct ApproxHistory {
  int n;
  int first[kApproxMaxVersions];
  double min[kApproxMaxVersions][3], max[kApproxMaxVersions][3];
  long long shift[kApproxMaxVersions][3];
};
constexpr long long kMapKeyReach = (1ll << 20) - 1;  // voxels a map key may lie from the first box's minimum (21 bits per axis)
// a point farther than this (in voxels) from the first box's minimum can never get a key in reach: a key and the point's
// offset / res differ by less than one voxel plus the rounding of the minimum's moves
constexpr double kMapFar = 1048576.0 + 2.0;
// first point of pts[0..n) (index order) that is finite, not far, and outside the box (any finite one: box undefined)
hipError_t launch_approx_first_outside(const float4* pts, int n, const ApproxBox& b, bool defined, int* d_first, hipStream_t stream);
hipError_t launch_approx_fill(unsigned long long* keys, int* vals, unsigned int cap, hipStream_t stream);
// the node paths of map points [lo, hi) from their stored keys; leaves chain their points through leaf_next
hipError_t launch_approx_insert(const unsigned long long* pkeys, int lo, int hi, const ApproxBox& b, unsigned long long* keys,
                                int* vals, int* leaf_next, unsigned int cap, hipStream_t stream);
hipError_t launch_approx_descend(const float4* queries, int n, const Xform& T, const ApproxBox& b, const unsigned long long* keys,
                                 const int* vals, const int* leaf_next, const float4* map_pts, unsigned int cap,
                                 unsigned long long* out, hipStream_t stream);
int approx_max_depth();
// generic primitives (icp_scan.hip): exclusive prefix sum of int32 (scratch: exclusive_scan_scratch_ints(n) ints) and a stable
// LSD radix sort of (key, value) int32 pairs from the first halves of keys / vals (2 n ints each) into the second halves
size_t exclusive_scan_scratch_ints(int n);
hipError_t launch_exclusive_scan(const int* in, int* out, int n, int* scratch, hipStream_t stream);
// Order-preserving compaction: the indices i with flags[i] != 0 (0 / 1 flags), ascending, into kept and their number into *n_kept;
// with cloud and points both given, cloud[i] of those into points (device-visible memory) in the same order.  flags, pos, kept
// (and points): n of room each; scan_scratch: exclusive_scan_scratch_ints(n) ints.  n <= 0 writes nothing.  Every `flags, pos,
// scan_scratch` below is this launcher's.
hipError_t launch_compact(const int* flags, int n, int* pos, int* scan_scratch, int* kept, int* n_kept, const float4* cloud, float4* points,
                          hipStream_t stream);
size_t radix_sort_scratch_ints(int n);
hipError_t launch_radix_sort_pairs(int* keys, int* vals, int n, unsigned int end_bit, int* scratch, hipStream_t stream);
size_t map_scan_temp_bytes(int n);
// hash set: keys (packed voxel coordinates, all-ones = empty), vals (map index, -1 = claimed this call), first (bids)
hipError_t launch_map_fill(unsigned long long* keys, int* vals, int* first, unsigned int cap, hipStream_t stream);
hipError_t launch_map_rehash(const unsigned long long* pkeys, int n_map, unsigned long long* keys, int* vals, unsigned int cap,
                             hipStream_t stream);
// moved[i] = T * in[i] (w = 1)
hipError_t launch_map_xform(const float4* in, int n, const Xform& T, float4* moved, hipStream_t stream);
// addPointsToMap() for moved[0..n): every point keyed under the box version h gives it; the first point (lowest i) of every
// unoccupied voxel, and every point that grew the box, is appended to map_pts at base + (its rank among the appended), input
// order preserved, its key to pkeys; *d_n_added = number appended.  cap is a power of two.
hipError_t launch_map_insert(const float4* moved, int n, const ApproxHistory& h, double res, unsigned long long* keys, int* vals,
                             int* first, unsigned int cap, int* slot_of, int* flags, int* rank, void* temp, size_t temp_bytes,
                             int base, float4* map_pts, unsigned long long* pkeys, int* d_n_added, hipStream_t stream);
// nn cloud: out = T_out * map[index(keys[i])] for every non-empty key, order preserved; *d_n_out = points written
hipError_t launch_map_nn_gather(const unsigned long long* keys, int n, const float4* map_pts, const Xform& T_out, int* flags,
                                int* rank, void* temp, size_t temp_bytes, float4* out, int* d_n_out, hipStream_t stream);
// The nn cloud repeats every map point once per scan point that chose it.  uniq / uniq_index receive its DISTINCT points
// (first occurrences, in nn-cloud order) and their positions in the nn cloud; first_user is n_map ints of scratch,
// uflags / urank n ints each.  flags / rank are the arrays launch_map_nn_gather left behind.
hipError_t launch_map_nn_unique(const unsigned long long* keys, const int* flags, const int* rank, int n, const float4* nn_cloud,
                                int n_map, int* first_user, int* uflags, int* urank, void* temp, size_t temp_bytes,
                                float4* uniq, int* uniq_index, int* d_n_uniq, hipStream_t stream);

// ---- voxel-grid down-sampling (icp_voxel.hip), SURVEY.md 8(f2) -------------------------------------------------
size_t voxel_temp_bytes(int n);
// keys/vals: 2*n ints each, flags/slots: n ints each, d_n_out: 2 ints whose sum is the number of cells written to `out`.
// minb / divb / wraps: voxel_grid_plan's (icp_voxel_plan.h), wraps = its verdict was kVoxelPlanWrap.
hipError_t launch_voxel_grid(const float4* pts, int n, float inv_leaf, const int minb[3], const int divb[3], bool wraps, int* keys,
                             int* vals, int* flags, int* slots, void* temp, size_t temp_bytes, float4* out, int* d_n_out,
                             hipStream_t stream);

// The same filter without the library sort (one distribution pass + a sort in LDS; icp_voxel.hip): bins =
// voxel_direct_scratch_ints(n) ints, all zero before the first call; published = voxel_direct_groups(n) 64-bit words used for
// nothing else, zero before the first call; keys, relpos n ints each; comp n 64-bit words;
// *status != 0 when a voxel bucket exceeded the LDS capacity -- nothing usable was written, run launch_voxel_grid instead.
size_t voxel_direct_scratch_ints(int n);
int voxel_direct_groups(int n);
hipError_t launch_voxel_grid_direct(const float4* pts, int n, float inv_leaf, const int minb[3], const int divb[3], int* bins,
                                    unsigned long long* published, int* keys, int* relpos, unsigned long long* comp, float4* out,
                                    int* d_n_out, int* status, hipStream_t stream, unsigned long long* clear_word = nullptr,
                                    int* d_bbox6 = nullptr, int* d_plan = nullptr);
// (d_plan, 14 ints, with d_bbox6 = launch_bbox's result queued in front: the device derives minb / divb / the buckets itself and the
// host need not have seen the box; plan[7] = 0 the filter ran, 1 no finite point, 2 PCL's pass-through, 3 the sort path's cloud;
// plan[8..13] = the box, d_bbox6 itself is left as bbox_init_kernel leaves it: the next launch_bbox on it may skip its init)
// (clear_word, optional: a 64-bit word of device memory the last kernel sets to zero -- launch_publish_cloud's accumulator)

// ---- outlier removal (icp_outlier.hip): pcl::StatisticalOutlierRemoval / pcl::RadiusOutlierRemoval -----------------------------
// (sorted, cell_start, g, n_binned: the cloud's own grid, or sorted == null when it has none)
// dist[i] = PCL's mean distance to the mean_k nearest neighbours (0 for a non-finite point); far: n_binned + 2 ints of scratch.
// Without a grid every point takes the whole-cloud kernel: the caller caps n (kGicpCovFarMost).
hipError_t launch_sor_distances(const float4* cloud, int n, const float4* sorted, const int* cell_start, const GridDesc& g, int n_binned,
                                int mean_k, float* dist, int* far, hipStream_t stream);
// stats (4 doubles) = mean, stddev, threshold, n_valid over dist[]; flags[i] = 1 where point i is kept
hipError_t launch_sor_flags(const float4* cloud, const float* dist, int n, double stddev_mult, int negative, double* stats, int* flags,
                            hipStream_t stream);
// measure[i] = (float)(finite points j with d2(i, j) < r2) and flags[i]; brute: no grid, every point against the whole cloud
hipError_t launch_ror_counts(const float4* cloud, int n, const float4* sorted, const int* cell_start, const GridDesc& g, int n_binned, float r2,
                             int min_pts, int negative, bool brute, float* measure, int* flags, hipStream_t stream);
// (the kept points: launch_compact over flags)

// ---- neighbour search (icp_search.hip): pcl::search::KdTree's nearestKSearch / radiusSearch ------------------------------------
// (cloud, n: the search cloud; sorted, cell_start, g: its k-NN grid, or sorted == null when it has none -- the caller caps n then)
// Row q of idx / d2 (k entries each, k <= 64) = the k smallest keys (d2 bits << 32 | index) of queries[q] over the finite cloud
// points, ascending, padded with -1 / +inf; n_found[q] = how many there are.  far: n_q + 2 ints of scratch.
hipError_t launch_search_knn(const float4* queries, int n_q, const float4* cloud, int n, const float4* sorted, const int* cell_start,
                             const GridDesc& g, int k, int32_t* idx, float* d2, int32_t* n_found, int* far, hipStream_t stream);
// Radius search, first half: per query the number of finite cloud points with d2 < r2, cut at max_nn when max_nn > 0, and its
// exclusive scan row_start (n_q + 1 ints; row_start64: the same as int64).  shells: the cube of that many cells around a query's
// cell contains its ball (< 0: sweep the whole cloud instead).  counts, longs, scratch_start: n_q + 1 ints each; scan_scratch:
// exclusive_scan_scratch_ints(n_q + 1); totals: [0] the rows' total length, [1] the 64-bit words of scratch the second half needs
// -- 64-bit sums: a total that does not fit an int32 makes row_start meaningless and the caller must stop there.
static constexpr int kSearchRadiusShells = 8;  // a ball of more cells than this (17^3 in the cube) is searched without the grid
hipError_t launch_search_radius_count(const float4* queries, int n_q, const float4* cloud, int n, const float4* sorted, const int* cell_start,
                                      const GridDesc& g, int shells, float r2, int max_nn, int* counts, int* longs, int* row_start,
                                      int* scratch_start, int* scan_scratch, unsigned long long* totals, long long* row_start64,
                                      hipStream_t stream);
// ... second half: row q of idx / d2 = [row_start[q], row_start[q + 1]), ascending by key
hipError_t launch_search_radius_fill(const float4* queries, int n_q, const float4* cloud, int n, const float4* sorted, const int* cell_start,
                                     const GridDesc& g, int shells, float r2, const int* row_start, const int* scratch_start,
                                     unsigned long long* scratch, int32_t* idx, float* d2, hipStream_t stream);

// ---- euclidean clustering (icp_cluster.hip): pcl::EuclideanClusterExtraction over the search cloud ------------------------------
// The connected components of the graph "d2(i, j) < r2" over the cloud's finite points (shells, r2: as for the radius search;
// any_finite: the cloud has a finite point), the components of min_size .. max_size points as clusters by size descending, the
// lowest component name first among equal sizes.  component, labels: n ints (-1: none); cstart64: the clusters' starts, n + 1 entries
// of which the first counts[0] + 1 count; vals[n .. n + counts[1]): the clusters' points, ascending inside a cluster; counts: 2 ints.
// parent, sizes, rank_of: n ints each; csize, cstart: n + 1 ints; keys, vals: 2 n ints; scratch: cluster_scratch_ints(n) ints.
// n = 0 writes counts and cstart64[0] alone.  The number of launches depends on n's bit length only.
size_t cluster_scratch_ints(int n);
hipError_t launch_cluster_extract(const float4* cloud, int n, bool any_finite, const float4* sorted, const int* cell_start, const GridDesc& g,
                                  int shells, float r2, int min_size, int max_size, int* parent, int* sizes, int* component, int* labels,
                                  int* rank_of, int* csize, int* cstart, long long* cstart64, int* keys, int* vals, int* scratch, int* counts,
                                  hipStream_t stream);
// ... its tail alone, for any partition stated the same way (region growing's): component[i] = the name of i's set (the set's lowest
// member that names itself: component[name] == name) or -1, sizes[name] = the set's size.  Writes everything above but parent,
// sizes and component.
hipError_t launch_cluster_tail(const int* component, const int* sizes, int n, int min_size, int max_size, int* labels, int* rank_of, int* csize,
                               int* cstart, long long* cstart64, int* keys, int* vals, int* scratch, int* counts, hipStream_t stream);

// ---- region growing (icp_region.hip): pcl::RegionGrowing over the search cloud, the order-free rule of include/icpgpu.h ---------
// normals: n float4 {nx, ny, nz, curvature}; rows_idx / rows_d2 / rows_found: the cloud's own k-nearest rows (launch_search_knn with
// the cloud as queries, stride k), not read when any_finite is false.  kind (2 core, 1 border, 0 single, -1 none), anchor, region
// (the region's name, -1: none): n ints; border_key: n 64-bit words; the rest as launch_cluster_extract's, whose tail orders the
// regions.  The number of launches depends on n's bit length only.
hipError_t launch_region_growing(const float4* cloud, const float4* normals, int n, bool any_finite, const int32_t* rows_idx, const float* rows_d2,
                                 const int32_t* rows_found, int k, float smoothness_cos, float curvature_threshold, int min_size, int max_size,
                                 int* kind, unsigned long long* border_key, int* anchor, int* parent, int* sizes, int* region, int* labels,
                                 int* rank_of, int* csize, int* cstart, long long* cstart64, int* keys, int* vals, int* scratch, int* counts,
                                 hipStream_t stream);

// ---- segment moments (icp_segment.hip): per-segment sums, boxes and axes over CSR segments of the search cloud -----------------
// The list -- all segments' entries, one after the other, `total` of them -- is cut into chunks of kSegmentChunk entries; a wave
// takes a chunk, a lane an entry, and every segment that has entries in the chunk has one PIECE there.  Piece (segment s, chunk g) owns slot g + s of the two
// partial arrays (segment_partials(n_segments, total) of each): no two pieces share a slot, since a later segment lies in a later or
// the same chunk.  start: n_segments + 1 ints, non-decreasing from 0 to total; list: total cloud indices (clamped to the cloud).
static constexpr int kSegmentChunk = 64;  // = ICPGPU_SEGMENT_CHUNK: a wave
struct SegmentPartial {  // a piece's nine double-double sums about K, its finite entries and their float32 box as ordered keys
  double hi[9], lo[9];
  unsigned int box_min[3], box_max[3];
  int count, pad;
};
struct SegmentBoxPartial {  // a piece's extents along the segment's axes as ordered 64-bit keys
  unsigned long long lo[3], hi[3];
};
inline size_t segment_chunks(size_t total) { return (total + kSegmentChunk - 1) / kSegmentChunk; }
inline size_t segment_slots(size_t n_segments, size_t total) { return segment_chunks(total) + n_segments; }
// ... and behind the slots one folded partial per segment: what the two partial arrays hold
inline size_t segment_partials(size_t n_segments, size_t total) { return segment_slots(n_segments, total) + n_segments; }
// seg_of (total ints): every entry's segment.  first (n_segments words): the list position of each segment's first finite entry, all
// ones where it has none.  records: n_segments icpgpu_segment_record (void*: this header does not know the public one).  Seven
// launches and a memset, whatever the rows' lengths.
hipError_t launch_segment_moments(const float4* cloud, int n, const int* start, const int* list, int n_segments, int total, int* seg_of,
                                  unsigned int* first, SegmentPartial* partials, SegmentBoxPartial* box_partials, void* records, hipStream_t stream);

// ---- ISS keypoints (icp_iss.hip): pcl::ISSKeypoint3D over the search cloud ------------------------------------------------------------
// Per point of `cloud` (sorted, cell_start, g, shells_*: as launch_search_radius_count, one `shells` per radius; any_finite: the cloud
// has a finite point): n_salient (n), scatter6 (n x 6), eig3 (n x 3, descending) and saliency (n) from the salient ball, then the
// 0 / 1 keypoint flags from the non-max ball, the keypoints' indices ascending into kept, their points into points and their number
// into *n_kept (launch_compact).  n = 0 writes *n_kept alone.
// border (n ints, or null: no border estimation): a point with border[i] != 0 keeps its n_salient and has zeros otherwise.
hipError_t launch_iss_keypoints(const float4* cloud, int n, bool any_finite, const float4* sorted, const int* cell_start, const GridDesc& g,
                                int shells_salient, float r2_salient, int shells_non_max, float r2_non_max, int min_neighbors, double gamma_21,
                                double gamma_32, const int32_t* border, int32_t* n_salient, double* scatter6, double* eig3, double* saliency,
                                int* flags, int* pos, int* scan_scratch, float4* points, int* kept, int* n_kept, hipStream_t stream);
// border[i] = 1 iff point i is finite and a point j of its ball (shells, r2: as above; itself included) has edge[j] != 0, else 0
hipError_t launch_iss_border(const float4* cloud, int n, const float4* sorted, const int* cell_start, const GridDesc& g, int shells, float r2,
                             const int32_t* edge, int32_t* border, hipStream_t stream);

// ---- moving least squares (icp_mls.hip): pcl::MovingLeastSquares over the search cloud's radius rows ---------------------------------
// Per query, from its CSR row (idx by row_start, as launch_search_radius_fill leaves it): n_neighbours, status, plane7 (n_q x 7),
// coeff10 (n_q x 10), the projected point and the normal with the curvature (points / normals, n_q float4 each); the kept queries
// (status != 0) in query order: their indices into kept, their points and normals into out_points / out_normals, their number into
// *n_kept (launch_compact).  order: 0 .. 3; s: the weights' squared Gaussian parameter.  sums9 (n_q x 9), frame12 (n_q x 12) and
// fit (n_q x mls_fit_doubles(order)) are scratch.  n_q = 0 writes *n_kept alone.
size_t mls_fit_doubles(int order);
hipError_t launch_mls(const float4* queries, int n_q, const float4* cloud, int n, const int32_t* idx, const int* row_start, int order, double s,
                      int32_t* n_neighbours, double* sums9, double* frame12, double* fit, int32_t* status, double* plane7, double* coeff10,
                      float4* points, float4* normals, int* flags, int* pos, int* scan_scratch, int* kept, int* n_kept, float4* out_points,
                      float4* out_normals, hipStream_t stream);

// ---- plane segmentation (icp_sac.hip): pcl::SACSegmentation's RANSAC over the search cloud ---------------------------------------
// A batch of kSacBatch hypotheses t0 .. t0 + 63 (hypothesis t0 + h is lane h's): the model kernel fills plane / sample and sets
// count to 0, or to -1 for an INVALID hypothesis (and for t >= max_iterations), the counting kernel adds the inliers.  thr: the
// smallest float32 not below the double threshold.  The counting grid is capped at kSacGridCap workgroups of kSacBlockPoints points
// a step.  n > 0.
static constexpr int kSacBatch = 64, kSacBlockPoints = 512, kSacGridCap = 1024;
struct SacBatch {
  int count[kSacBatch];
  float4 plane[kSacBatch];
  int sample[kSacBatch][3];
};
hipError_t launch_sac_batch(const float4* cloud, int n, unsigned long long seed, int t0, int max_iterations, bool use_axis, const double axis[3],
                            double cos_eps, float thr, SacBatch* batch, hipStream_t stream);
// flags[i] = 1 where point i is an inlier of `plane` (nowhere when !found), the other way round with `invert`
hipError_t launch_sac_flags(const float4* cloud, int n, const float plane[4], float thr, bool found, bool invert, int* flags, hipStream_t stream);
// the inliers of `plane` in ascending order into inliers, their number into *n_inliers (launch_compact)
hipError_t launch_sac_select(const float4* cloud, int n, const float plane[4], float thr, int* flags, int* pos, int* scan_scratch, int* inliers,
                             int* n_inliers, hipStream_t stream);
// sums12[0 .. 9): the exact sums, rounded once, of dx dx, dx dy, dx dz, dy dy, dy dz, dz dz, dx, dy, dz over the m > 0 listed points
// about K = cloud[k_index] (d = q - K in float32); sums12[9 .. 12): K.  One workgroup, a fixed order.
hipError_t launch_sac_sums(const float4* cloud, int n, const int* inliers, int m, int k_index, double* sums12, hipStream_t stream);

// ---- segmentation from normals (icp_sac_normals.hip): pcl::SACSegmentationFromNormals' RANSAC over the search cloud ---------------
// The plane segmentation's scheme with the cloud's normals (n float4: nx, ny, nz, curvature) beside it.  model: kSacnPlane or
// kSacnCylinder (icp_sac_normals.h).  A record holds the coefficients in rec[0 .. 7) (4 for a plane) and, for a cylinder, the band
// of squared axis distances that can hold inliers in rec[8], rec[9] and its first sample point in rec[12 .. 15); NaN for an INVALID hypothesis.  weight: the float32 image of
// normal_distance_weight.  The counting grid is capped at kSacnGridCap workgroups of kSacnBlockPoints points a step.  n > 0.
static constexpr int kSacnRecord = 16, kSacnBlockPoints = 512, kSacnGridCap = 1024;
struct SacnBatch {
  int count[kSacBatch];
  float rec[kSacBatch][kSacnRecord];
  int sample[kSacBatch][3];
};
hipError_t launch_sacn_batch(const float4* cloud, const float4* normals, int n, int model, unsigned long long seed, int t0, int max_iterations,
                             bool use_axis, const double axis[3], double cos_eps, double radius_min, double radius_max, float thr, float weight,
                             SacnBatch* batch, hipStream_t stream);
// the inliers of the model in ascending order into inliers, their number into *n_inliers (launch_compact)
hipError_t launch_sacn_select(const float4* cloud, const float4* normals, int n, int model, const float coeff7[7], float thr, float weight, int* flags,
                              int* pos, int* scan_scratch, int* inliers, int* n_inliers, hipStream_t stream);
// sums21: the sums of sacn_cyl_terms (icp_sac_normals.h) over the m > 0 listed points for the axis P + s D, the chart coordinates
// ia < ib and the radius r, each the double-double sum of its terms rounded once.  One workgroup, a fixed order.
hipError_t launch_sacn_cyl_sums(const float4* cloud, int n, const int* inliers, int m, const double P[3], const double D[3], int ia, int ib, double r,
                                double* sums21, hipStream_t stream);
// flags[i] = 1 where i is among the m listed indices, the other way round with `invert`
hipError_t launch_sacn_list_flags(const int* list, int m, int n, bool invert, int* flags, hipStream_t stream);

// ---- sample-consensus rejector (icp_reject_sac.hip): pcl::registration::CorrespondenceRejectorSampleConsensus over m pairs --------
// The pairs live in arrays of the stage's own: P, Q (m float4 each) and rank (m ints: the source index of pair r in the chain, r in
// the call of its own).  A batch is kSacBatch hypotheses t0 .. t0 + 63 (hypothesis t0 + h is lane h's); the counting grid is capped
// as the plane segmentation's (kSacGridCap workgroups of kSacBlockPoints pairs a step).
static constexpr int kRsacDraws = 16;  // = ICPGPU_RSAC_DRAWS
struct RsacModels {  // what the model kernel hands the host: the 17 sums of a good draw's three pairs, its ranks (-1: no good draw)
  double sums[kSacBatch][kReduceTerms];
  int ranks[kSacBatch][3];
  int good[kSacBatch];
};
struct RsacBatch {  // what the host hands the counting kernel: count = 0 and the float transform, or -1 and NaN for an INVALID one
  int count[kSacBatch];
  Xform T[kSacBatch];
};
// the chain's gather: flags of the alive pairs (d2 <= thr, a target index below n_t), their ascending source ranks and number
// (launch_compact: flags, pos, scan_scratch are its scratch over n_s entries), then P_r = T * src[rank[r]], Q_r = tgt[index].  n_s, n_t > 0.
hipError_t launch_rsac_gather_keys(const float4* src, int n_s, const float4* tgt, int n_t, const unsigned long long* keys, float thr, const Xform& T,
                                   int* flags, int* pos, int* scan_scratch, int* rank, int* m_dev, float4* P, float4* Q, hipStream_t stream);
// the call's gather: P_r = source[iq[r]], Q_r = target[im[r]], rank[r] = r (every index inside its cloud; m, n_s, n_t > 0)
hipError_t launch_rsac_gather_index(const float4* source, int n_s, const float4* target, int n_t, const int32_t* iq, const int32_t* im, int m,
                                    float4* P, float4* Q, int* rank, hipStream_t stream);
// out14[0 .. 9): the exact sums, rounded once, of dx dx, dx dy, dx dz, dy dy, dy dz, dz dz, dx, dy, dz over the finite P_r about
// K = the first finite P (d = P_r - K in float32); out14[9 .. 12): K; out14[12]: the finite P_r; out14[13]: m = *m_dev, or m_host
// with m_dev == null, capped at m_cap.  One workgroup, a fixed order.
hipError_t launch_rsac_moments(const float4* P, int m_host, const int* m_dev, int m_cap, double* out14, hipStream_t stream);
hipError_t launch_rsac_models(const float4* P, const float4* Q, int m, unsigned long long seed, int t0, int max_iterations, double sample_d2,
                              RsacModels* models, hipStream_t stream);
// batch->count[h] += the pairs with d2(T_h P_r, Q_r) < thr (thr: the smallest float32 not below the double threshold squared)
hipError_t launch_rsac_count(const float4* P, const float4* Q, int m, float thr, RsacBatch* batch, hipStream_t stream);
// flags[r] (or null) = pair r stays: an inlier of T, or every pair with keep_all; keys (or null): kEmptyKey into keys[rank[r]] of a
// pair that does not.  The pairs that stay are ADDED to *n_kept, or with stats (a chain stage's kRejectStats words, zeroed) to
// stats[1], and stats[0] = m.
hipError_t launch_rsac_flags(const float4* P, const float4* Q, const int* rank, int m, const Xform& T, float thr, bool keep_all, int* flags,
                             unsigned long long* keys, int n_s, unsigned int* n_kept, unsigned int* stats, hipStream_t stream);

// ---- normal estimation (icp_normals.hip): pcl::NormalEstimation over neighbour rows still in device memory --------------------
// out[i] = {nx, ny, nz, curvature} of query i from its row of cloud indices (ascending by key, as the launchers above leave them):
// dense rows of stride k with n_found (row_start == null), or CSR rows with row_start (n_found == null).  moments (optional):
// n_q x {xx, xy, xz, yy, yz, zz, cx, cy, cz}.  Rows shorter than 3 give NaN.
hipError_t launch_normals_from_rows(const float4* queries, int n_q, const float4* cloud, int n, const int32_t* idx, const int32_t* n_found, int k,
                                    const int* row_start, const float viewpoint[3], float4* out, float* moments, hipStream_t stream);

// ---- boundary estimation (icp_boundary.hip): pcl::BoundaryEstimation over neighbour rows still in device memory ---------------
// Rows as for launch_normals_from_rows.  normals: the QUERIES' normals (float4, the fourth float ignored).  A row of at least
// max(min_row, 3) entries of a finite query is tested against cos_threshold = cos(angle_threshold); boundary (n_q bytes) and flag32
// (n_q ints) receive the same 0 / 1, n_directions the row's directions, witness the lowest cloud index among the directions with an
// empty sector, or -1.  Each of the four may be null.
hipError_t launch_boundary_from_rows(const float4* queries, int n_q, const float4* normals, const float4* cloud, int n, const int32_t* idx,
                                     const int32_t* n_found, int k, const int* row_start, int min_row, double cos_threshold, uint8_t* boundary,
                                     int32_t* flag32, int32_t* n_directions, int32_t* witness, hipStream_t stream);

// ---- fast point feature histograms (icp_fpfh.hip): pcl::FPFHEstimation over neighbour rows still in device memory -------------
// Rows as for launch_normals_from_rows (dense with n_found, or CSR with row_start).  spfh[p] (n x 33): the simplified histogram of
// cloud point p from ITS row over the cloud and the cloud's normals (float4, the fourth float ignored); rows shorter than 2 give
// zeros.  out[q] (n_q x 33): the queries' rows (idx with their d2) weighted over spfh; a non-finite query gives NaN.
hipError_t launch_spfh_from_rows(const float4* cloud, int n, const float4* normals, const int32_t* idx, const int32_t* n_found, int k,
                                 const int* row_start, float* spfh, hipStream_t stream);
hipError_t launch_fpfh_from_rows(const float4* queries, int n_q, int n, const float* spfh, const int32_t* idx, const float* d2, const int32_t* n_found,
                                 int k, const int* row_start, float* out, hipStream_t stream);

// ---- feature-space k-nearest (icp_feature.hip): pcl::KdTreeFLANN<FPFHSignature33>::nearestKSearch -----------------------------------
// Row q of idx / d2 (k entries each, k <= 64) = the k smallest keys (d2 bits << 32 | target row) of query row q over the target rows
// whose 33 components are all finite, ascending, padded with -1 / +inf; n_found[q] = how many there are (0 for a query row with a
// non-finite component).  d2 is the 33-term fma chain of include/icpgpu.h.  target_finite: n_t ints of scratch (written first).
static constexpr int kFeatureBins = 33;   // = ICPGPU_FPFH_BINS
static constexpr int kFeatureTile = 256;  // target rows a workgroup stages at a time (the tests' tile edge)
hipError_t launch_feature_knn(const float* target, int n_t, const float* query, int n_q, int k, int* target_finite, int32_t* idx, float* d2,
                              int32_t* n_found, hipStream_t stream);

// ---- sample-consensus alignment with pre-rejection (icp_feature.hip): pcl::SampleConsensusPrerejective ------------------------------
static constexpr int kScpChunk = 65536;     // = ICPGPU_SCP_CHUNK: hypotheses sampled per launch (and per host wait)
static constexpr int kScpBatch = 64;        // surviving hypotheses per evaluation launch
static constexpr int kScpMaxSamples = 8;    // = ICPGPU_SCP_MAX_SAMPLES
static constexpr int kScpBlockPoints = 64;  // source points per workgroup of the evaluation
static constexpr int kScpInvalid = 0, kScpPrerejected = 1, kScpNoTransform = 2, kScpEvaluated = 3;  // = ICPGPU_SCP_*
struct ScpBox {  // the target's box grown by the correspondence distance: an image outside it is no inlier (use = 0: no box known)
  float lo[3], hi[3];
  int use;
};
struct ScpPartial {
  long long count;
  double hi, lo;
};
struct ScpResult {
  long long count;
  double sum;
};
// hypotheses t0 .. t0 + m - 1 (m <= kScpChunk): status[e] (kScpEvaluated = survived the pre-rejection), the nr source and target indices
// (-1 where there is none), and for a survivor the 17 sums of solve_umeyama over its pairs (sum d2 = 0).  rows / found: the source's
// feature rows (kc entries each) over the target's descriptors.
hipError_t launch_scp_sample(const float4* source, int n_s, const float4* cloud, int n, const int32_t* rows, const int32_t* found, int kc,
                             unsigned long long seed, int t0, int m, int nr, float sim2, int32_t* status, int32_t* sidx, int32_t* tidx, double* sums,
                             hipStream_t stream);
// results[h] = {inliers, the exact sum of their d2 rounded once} of xforms[h], h < n_h <= kScpBatch, over the search cloud (cloud, n,
// sorted, cell_start, g, shells: as launch_search_radius_count).  partials: scp_eval_blocks(n_s) x kScpBatch.
int scp_eval_blocks(int n_s);
hipError_t launch_scp_eval(const float4* source, int n_s, const Xform* xforms, int n_h, const float4* cloud, int n, const float4* sorted,
                           const int* cell_start, const GridDesc& g, int shells, const ScpBox& box, float r2, ScpPartial* partials, ScpResult* results,
                           hipStream_t stream);
// the inliers of T, ascending, and their number (launch_compact over n_s flags)
hipError_t launch_scp_select(const float4* source, int n_s, const Xform& T, const float4* cloud, int n, const float4* sorted, const int* cell_start,
                             const GridDesc& g, int shells, const ScpBox& box, float r2, int* flags, int* pos, int* scan_scratch, int* inliers,
                             int* n_inliers, hipStream_t stream);

// ---- ground filter (icp_morph.hip): pcl::applyMorphologicalOperator / pcl::ProgressiveMorphologicalFilter over the search cloud ----
// "The extremum of a value array over every active point's xy box" (rule: include/icpgpu.h "ground filter"), over a 2-D cell table
// of the active points whose cell side the DEVICE derives from the cloud's finite xy box and the window: window / kMorphCellsPerWindow,
// coarsened until no axis has more than kMorphAxisCells cells.  Every count below is read from device memory (*d_count): launches
// are sized by n and no step needs the host.
static constexpr int kMorphCellsPerWindow = 8;
static constexpr int kMorphAxisCells = 512;
static constexpr int kMorphMaxCells = kMorphAxisCells * kMorphAxisCells;
// ints of the cell tables (counts: kMorphMaxCells + 1; fill, the two extremum tables: kMorphMaxCells each), zeroed before every binning
static constexpr size_t kMorphTableInts = 4 * (size_t)kMorphMaxCells + 1;
struct MorphGrid {  // cell(x) = clamp((int)((x - ox) * inv), 0, nx - 1), likewise y: the ONE cell function of binning and of box bounds
  float ox, oy, inv;
  int nx, ny;
};
// flags[i] = 1 for a finite point (x, y, z), else 0; removed_at[i] = -1 / -2 and out_z[i] = the point's own z where given; bbox4 (zeroed
// by the launcher) receives the finite points' xy box as ordered keys
hipError_t launch_morph_init(const float4* cloud, int n, int* flags, int32_t* removed_at, float* out_z, unsigned int* bbox4, hipStream_t stream);
// One binning of the active points act[0 .. *d_count) for `window`: the grid from bbox4, the counting sort into cell-row-major order
// (sxy, sval = z, sidx = cloud index, scell = cell; n of room each; cellid: n ints of scratch) with cell_start (kMorphMaxCells + 1
// ints) and, in the first extremum table of `table` (kMorphTableInts ints), every cell's extremum of z (is_max: max, else min).
hipError_t launch_morph_bin(const float4* cloud, int n, const int* act, const int* d_count, const unsigned int* bbox4, float window, MorphGrid* grid,
                            int* table, int* cell_start, int* scan_scratch, int* cellid, float2* sxy, float* sval, int* sidx, int* scell, bool is_max,
                            hipStream_t stream);
// out_val[p] = the extremum (is_max) of in_val over the box of sorted point p, a wave per point: the cells strictly inside the box's cell
// range through extremum table `phase` (0 / 1) of `table`, the rim's cells point by point with the rule's four comparisons.  With
// feed_next the OPPOSITE extremum of out_val per cell goes into table 1 - phase (what the second half of OPEN / CLOSE reads).
// tests (optional, kMorphTestSlots * kMorphTestStride counters, one per cache line in use): the number of exact point tests is added;
// launch_morph_tests_total sums the counters into *total.
static constexpr int kMorphTestSlots = 64, kMorphTestStride = 16;
hipError_t launch_morph_tests_total(const unsigned long long* tests, unsigned long long* total, hipStream_t stream);
hipError_t launch_morph_box(int n, const int* d_count, const MorphGrid* grid, float window, const float2* sxy, const int* cell_start, const int* scell,
                            const float* in_val, int* table, int phase, bool is_max, bool feed_next, float* out_val, unsigned long long* tests,
                            hipStream_t stream);
// the filter's verdict: sorted point p stays iff sval[p] - opened[p] < thr; flags[sidx[p]] = that, removed_at[sidx[p]] = pass where not
hipError_t launch_morph_judge(int n, const int* d_count, const float* sval, const float* opened, const int* sidx, float thr, int pass, int* flags,
                              int32_t* removed_at, hipStream_t stream);
// out_z[sidx[p]] = val[p]
hipError_t launch_morph_unsort(int n, const int* d_count, const float* val, const int* sidx, float* out_z, hipStream_t stream);
// flags[i] = 1 where removed_at[i] == -1 (ground), the other way round with `invert`
hipError_t launch_pmf_flags(const int32_t* removed_at, int n, bool invert, int* flags, hipStream_t stream);

// ---- cropping and sampling filters (icp_sampling.hip): pcl::PassThrough, CropBox, UniformSampling, FarthestPointSampling -------------
// (arithmetic: icp_sampling.h; every filter ends in flags for launch_compact or in a list of kept rows for launch_subset_gather)
struct CropRule {  // box = 0: PassThrough over `field` (-1: none) with lo[0] .. hi[0]; box = 1: CropBox over T * p (has_T) or p
  int box, field, negative, has_T;
  float lo[3], hi[3];
  Xform T;
};
hipError_t launch_crop_flags(const float4* cloud, int n, const CropRule& rule, int* flags, hipStream_t stream);
// UniformSampling over the plan's lattice (icp_voxel_plan.h: kVoxelPlanDirect): flags[i] = 1 for the row with the smallest (d2 bits,
// index) key of its cell, d2_of[i] = the row's d2 to its cell's centre (0 for a non-finite row).  cells (ints), best (64-bit words):
// uniform_table_slots(n) each; slot_of, d2_of: n.  Three launches whatever the cloud.  n <= kUniformMaxRows.
struct UniformLattice {
  float inv, leaf;
  int minb[3], divb[3];
};
static constexpr int kUniformMaxRows = 1 << 30;
unsigned int uniform_table_slots(int n);
hipError_t launch_uniform_flags(const float4* cloud, int n, const UniformLattice& L, int* cells, unsigned long long* best, unsigned int* slot_of,
                                float* d2_of, int* flags, hipStream_t stream);
// for j < count (*d_count when given, else count_most; the launch is sized by count_most): points[j] = cloud[kept[j]] and
// measure_out[j] = measure_in[kept[j]], each where given; *n_out = count where given
hipError_t launch_subset_gather(const int* kept, const int* d_count, int count_most, const float4* cloud, float4* points, const float* measure_in,
                                float* measure_out, int* n_out, hipStream_t stream);
// flags[i] = 1 for the n rows except kept[0 .. n_kept): what launch_compact turns into the removed indices
hipError_t launch_subset_removed_flags(const int* kept, int n_kept, int n, int* flags, hipStream_t stream);
// FarthestPointSampling from row `first` (finite, inside the cloud; n_samples <= the finite rows: the caller checks both): the
// selected rows in selection order into kept, each one's d2 to the set selected before it into measure (+inf for the first).
// launch_fps_one: n <= kFpsOneMax, ONE workgroup and one launch.  launch_fps_many: any n; m (n floats) and slots (2 x
// kFpsManyBlocksMax 64-bit words) are scratch; 1 + n_samples launches (*launches) over fps_many_blocks(n) workgroups.
static constexpr int kFpsOneMax = 16384;       // ICPGPU_FPS_ONE_WORKGROUP_MAX: 1024 lanes x 16 rows in registers
static constexpr int kFpsManyBlocksMax = 1024;  // the many-workgroup shape's grid cap: beyond 2^20 rows a workgroup makes several trips
int fps_many_blocks(int n);
hipError_t launch_fps_one(const float4* cloud, int n, int n_samples, int first, int* kept, float* measure, hipStream_t stream);
hipError_t launch_fps_many(const float4* cloud, int n, int n_samples, int first, float* m, unsigned long long* slots, int* kept, float* measure,
                           int* launches, hipStream_t stream);

}  // namespace icpgpu
