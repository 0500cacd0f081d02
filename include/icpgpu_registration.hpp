// icpgpu_registration.hpp -- header-only C++ shim: the PCL `Registration` protocol on top of the icpgpu C-ABI.
//
// The reference drives exactly this protocol at two call sites
//   /root/reference/src/icpslam/icp_odometer.cpp:188-201   and   src/icpslam/octree_mapper.cpp:104-117
// so switching it to the MI355X path is a one-type-name change:
//
//   - pcl::GeneralizedIterativeClosestPoint<pcl::PointXYZ, pcl::PointXYZ> icp;
//   + icpgpu::GeneralizedIterativeClosestPoint<pcl::PointCloud<pcl::PointXYZ>> icp;   // the same solver (GICP)
//
// icpgpu::IterativeClosestPoint<Cloud> is pcl::IterativeClosestPoint's counterpart (point-to-point, SVD): the solver
// BASELINE.json's north_star specifies kernel by kernel.  Each class keeps the semantics of the PCL class it is named after.
//
// CloudT is any type with a contiguous `points` container of 16-byte {x, y, z, pad} structs, `size()` and
// `resize()`: pcl::PointCloud<pcl::PointXYZ> qualifies (PointXYZ is 16 B, 16-byte aligned).
// The smart-pointer flavour (boost::shared_ptr in PCL <= 1.10, std::shared_ptr later) is a template parameter of
// the setters.  getFinalTransformation() returns Eigen::Matrix4f when Eigen is available, otherwise a POD with
// the same column-major layout.
//
// Behaviour kept from PCL: no exceptions on the data path; failure is hasConverged() == false.  The only throw
// is at construction when no gfx950 device / libicpgpu is usable (there is no CPU fallback to hide that).
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "icpgpu.h"

// -DICPGPU_SHIM_TIMING (development): wall time of the phases of align() -- 1 the uploads / recognitions, 2 icpgpu_align_view,
// 3 filling `output` -- summed in icpgpu::detail::shim_us[] (not thread-safe: for harnesses that run one callback at a time)
#if defined(ICPGPU_SHIM_TIMING)
#include <chrono>
namespace icpgpu { namespace detail {
inline double* shim_us_array() { static double v[8] = {0, 0, 0, 0, 0, 0, 0, 0}; return v; }
inline void shim_mark(int k) {
  static std::chrono::steady_clock::time_point t;
  const auto now = std::chrono::steady_clock::now();
  if (k > 0) shim_us_array()[k] += std::chrono::duration<double, std::micro>(now - t).count();
  t = now;
}
} }
#define ICPGPU_SHIM_MARK(k) ::icpgpu::detail::shim_mark(k)
#else
#define ICPGPU_SHIM_MARK(k) ((void)0)
#endif

#if defined(__has_include)
#if __has_include(<Eigen/Core>)
#include <Eigen/Core>
#define ICPGPU_HAVE_EIGEN 1
#endif
#endif

namespace icpgpu {

#ifdef ICPGPU_HAVE_EIGEN
using Matrix4 = Eigen::Matrix4f;
inline Matrix4 make_matrix4(const float* colmajor) { return Eigen::Map<const Eigen::Matrix4f>(colmajor); }
#else
struct Matrix4 {  // column-major like Eigen::Matrix4f
  float m[16];
  float operator()(int r, int c) const { return m[c * 4 + r]; }
  float& operator()(int r, int c) { return m[c * 4 + r]; }
  const float* data() const { return m; }
  static Matrix4 Identity() {
    Matrix4 I;
    for (int i = 0; i < 16; ++i) I.m[i] = (i % 5 == 0) ? 1.f : 0.f;
    return I;
  }
};
inline Matrix4 make_matrix4(const float* colmajor) {
  Matrix4 M;
  std::memcpy(M.m, colmajor, sizeof(M.m));
  return M;
}
#endif

namespace detail {
// The reference constructs its registration object on the stack for every scan (icp_odometer.cpp:188), and its callbacks
// run on whichever of the ROS AsyncSpinner(4) threads is free (icpslam_node.cpp:9).  The device context (stream, scratch,
// the clouds, grids and covariances in HBM) therefore lives in a per-process POOL, not in the object and not in the
// thread: an object leases a context for its lifetime and hands it back; the next object -- on any thread -- gets the most
// recently returned one, or, at align(), the idle one whose source cloud has the size of the target it is about to set
// (the odometer's previous scan: icpgpu_set_target then recognises the content and keeps cloud, grid and covariances).
// Two objects alive at once (the odometer's callback and the mapper's main loop, or two objects on one thread) hold two
// different contexts.  Contexts are never destroyed behind the caller's back: the pool is leaked at process end (no static
// destructor may run after the HIP runtime's own), release_cached_contexts() frees the idle ones on request.
struct Slot {
  icpgpu_ctx* ctx = nullptr;
  int device = 0;
  unsigned long long generation = 0;  // bumped whenever the context's clouds are replaced (only the lease holder writes it)
};
struct Pool {
  std::mutex m;
  std::vector<Slot*> idle;  // most recently returned last
};
inline Pool& pool() {
  static Pool* p = new Pool;
  return *p;
}
using ContextPtr = std::shared_ptr<Slot>;
inline void give_back(Slot* s) {
  std::lock_guard<std::mutex> g(pool().m);
  pool().idle.push_back(s);
}
// idle context of `device`: the one whose source cloud has want_source_n points if there is one, else the most recently
// returned one; nullptr if none is idle
inline Slot* take_idle(int device, std::size_t want_source_n) {
  Pool& P = pool();
  std::lock_guard<std::mutex> g(P.m);
  std::size_t pick = P.idle.size();
  for (std::size_t i = P.idle.size(); i-- > 0;) {
    if (P.idle[i]->device != device) continue;
    if (pick == P.idle.size()) pick = i;
    if (want_source_n == static_cast<std::size_t>(-1)) break;
    std::size_t ns = 0;
    icpgpu_cloud_sizes(P.idle[i]->ctx, &ns, nullptr);
    if (ns == want_source_n) {
      pick = i;
      break;
    }
  }
  if (pick == P.idle.size()) return nullptr;
  Slot* s = P.idle[pick];
  P.idle.erase(P.idle.begin() + static_cast<std::ptrdiff_t>(pick));
  return s;
}
inline ContextPtr acquire_context(int device, std::size_t want_source_n = static_cast<std::size_t>(-1)) {
  Slot* s = take_idle(device, want_source_n);
  if (!s) {
    icpgpu_ctx* raw = nullptr;
    const int rc = icpgpu_create(&raw, device);
    if (rc != ICPGPU_OK)
      throw std::runtime_error(std::string("icpgpu_create failed: ") + icpgpu_last_error(nullptr));
    s = new Slot;
    s->ctx = raw;
    s->device = device;
  }
  return ContextPtr(s, give_back);
}
// a better-matching idle context for an object about to set a target of n points; keeps `have` when there is none
inline ContextPtr rebind_for_target(const ContextPtr& have, std::size_t n_target) {
  std::size_t ns = 0;
  icpgpu_cloud_sizes(have->ctx, &ns, nullptr);
  if (ns == n_target) return have;
  Slot* s = take_idle(have->device, n_target);
  if (!s) return have;
  std::size_t ns2 = 0;
  icpgpu_cloud_sizes(s->ctx, &ns2, nullptr);
  if (ns2 != n_target) {  // just the most recently returned one: no better than what we hold
    give_back(s);
    return have;
  }
  return ContextPtr(s, give_back);
}
// the context of the OctreeMap that last built an nn cloud on this thread (setInputTargetFromMap() without an argument).
// A WEAK reference: it neither keeps the map's lease alive (the context goes back to the pool when the map dies, on whatever
// thread) nor can it hand a dead map's context to a registration object (lock() fails once the lease is over).
inline std::weak_ptr<Slot>& last_map_context() {
  static thread_local std::weak_ptr<Slot> p;
  return p;
}

// pcl::PointCloud keeps width / height / is_dense beside `points` (pcl::toROSMsg asserts width * height == size): set
// them when the cloud type has them
template <class C>
auto set_cloud_shape(C& c, std::size_t n, int) -> decltype(c.width = 0, c.height = 0, c.is_dense = true, void()) {
  c.width = static_cast<decltype(c.width)>(n);
  c.height = 1;
  c.is_dense = true;
}
template <class C>
void set_cloud_shape(C&, std::size_t, long) {}
}  // namespace detail

// destroys the pool's idle contexts (their HBM); contexts leased by live objects are untouched
inline void release_cached_contexts() {
  std::vector<detail::Slot*> idle;
  {
    std::lock_guard<std::mutex> g(detail::pool().m);
    idle.swap(detail::pool().idle);
  }
  for (detail::Slot* s : idle) {
    icpgpu_destroy(s->ctx);
    delete s;
  }
}

// pcl::Correspondence, as far as the sample-consensus rejector reads and writes it
struct Correspondence {
  int index_query, index_match;
  float distance;
};
typedef std::vector<Correspondence> Correspondences;

// --- pcl::registration::CorrespondenceRejector and the five rejectors a registration object's chain may hold (PCL 1.8's names;
// include/icpgpu.h, "correspondence rejectors", states the rules and the two deviations).  The objects carry parameters: the
// stages run on the device inside align(), which also leaves the last iteration's median in the median rejector.
namespace registration {
class CorrespondenceRejector {
 public:
  typedef std::shared_ptr<CorrespondenceRejector> Ptr;
  typedef std::shared_ptr<const CorrespondenceRejector> ConstPtr;
  virtual ~CorrespondenceRejector() {}
  const std::string& getClassName() const { return rejection_name_; }
  virtual icpgpu_rejector entry() const = 0;            // (no PCL counterpart: what the C-ABI takes)
  virtual void takeCut(float /*d2*/) {}
  virtual void takeBestTransformation(const float* /*colmajor16*/) {}  // (the sample-consensus rejector's: as takeCut hands over the median)

 protected:
  std::string rejection_name_;
};
class CorrespondenceRejectorMedianDistance : public CorrespondenceRejector {
 public:
  typedef std::shared_ptr<CorrespondenceRejectorMedianDistance> Ptr;
  CorrespondenceRejectorMedianDistance() : median_distance_(0), factor_(1.0) { rejection_name_ = "CorrespondenceRejectorMedianDistance"; }
  void setMedianFactor(double factor) { factor_ = factor; }
  double getMedianFactor() const { return factor_; }
  double getMedianDistance() const { return median_distance_; }
  icpgpu_rejector entry() const override { return icpgpu_rejector{ICPGPU_REJECT_MEDIAN_DISTANCE, 0, factor_}; }
  void takeCut(float d2) override { median_distance_ = d2; }

 private:
  double median_distance_, factor_;
};
class CorrespondenceRejectorTrimmed : public CorrespondenceRejector {
 public:
  typedef std::shared_ptr<CorrespondenceRejectorTrimmed> Ptr;
  CorrespondenceRejectorTrimmed() : overlap_ratio_(0.5f), nr_min_correspondences_(0) { rejection_name_ = "CorrespondenceRejectorTrimmed"; }
  void setOverlapRatio(float ratio) { overlap_ratio_ = std::min(1.0f, std::max(0.0f, ratio)); }
  float getOverlapRatio() const { return overlap_ratio_; }
  void setMinCorrespondences(unsigned int min_correspondences) { nr_min_correspondences_ = min_correspondences; }
  unsigned int getMinCorrespondences() const { return nr_min_correspondences_; }
  icpgpu_rejector entry() const override { return icpgpu_rejector{ICPGPU_REJECT_TRIMMED, (int32_t)nr_min_correspondences_, (double)overlap_ratio_}; }

 private:
  float overlap_ratio_;
  unsigned int nr_min_correspondences_;
};
class CorrespondenceRejectorOneToOne : public CorrespondenceRejector {
 public:
  typedef std::shared_ptr<CorrespondenceRejectorOneToOne> Ptr;
  CorrespondenceRejectorOneToOne() { rejection_name_ = "CorrespondenceRejectorOneToOne"; }
  icpgpu_rejector entry() const override { return icpgpu_rejector{ICPGPU_REJECT_ONE_TO_ONE, 0, 0.0}; }
};
// a pair stays iff the dot of the source's normal (rotated by the iteration's transform) and the target's is above the threshold,
// the cosine of the largest accepted angle.  The normals are the registration object's (setSourceNormals / setTargetNormals: PCL
// reads them from PointNormal clouds) or estimated on the device.
class CorrespondenceRejectorSurfaceNormal : public CorrespondenceRejector {
 public:
  typedef std::shared_ptr<CorrespondenceRejectorSurfaceNormal> Ptr;
  CorrespondenceRejectorSurfaceNormal() : threshold_(1.0) { rejection_name_ = "CorrespondenceRejectorSurfaceNormal"; }
  void setThreshold(double threshold) { threshold_ = threshold; }
  double getThreshold() const { return threshold_; }
  icpgpu_rejector entry() const override { return icpgpu_rejector{ICPGPU_REJECT_SURFACE_NORMAL, 0, threshold_}; }

 private:
  double threshold_;
};
// RANSAC over the pairs with a rigid transform as the model (include/icpgpu.h, "sample-consensus rejector").  In a registration
// object's chain it carries its two parameters, the stage runs inside align() -- and WAITS ON THE HOST there -- and align() leaves
// the last iteration's best transform here.  Alone (setInputSource, setInputTarget, setInputCorrespondences,
// getRemainingCorrespondences / getCorrespondences) it filters a pair list on a context of its own, taken at the first such call.
class CorrespondenceRejectorSampleConsensus : public CorrespondenceRejector {
 public:
  typedef std::shared_ptr<CorrespondenceRejectorSampleConsensus> Ptr;
  explicit CorrespondenceRejectorSampleConsensus(int device = 0) : device_(device) {
    rejection_name_ = "CorrespondenceRejectorSampleConsensus";
    for (int i = 0; i < 16; ++i) best_T_[i] = (i % 5 == 0) ? 1.f : 0.f;
  }
  void setInlierThreshold(double threshold) { inlier_threshold_ = threshold; }
  double getInlierThreshold() const { return inlier_threshold_; }
  void setMaximumIterations(int max_iterations) { max_iterations_ = std::max(max_iterations, 0); }  // (0: the call alone; a chain refuses it)
  int getMaximumIterations() const { return max_iterations_; }
  void setRefineModel(bool refine) {
    if (refine) throw std::invalid_argument("CorrespondenceRejectorSampleConsensus: setRefineModel(true) is not provided");
  }
  bool getRefineModel() const { return false; }
  void setSeed(uint64_t seed) { seed_ = seed; }  // no PCL counterpart: the call's seed (PCL's non-random RandomSampleConsensus: 12345)
  icpgpu_rejector entry() const override { return icpgpu_rejector{ICPGPU_REJECT_SAMPLE_CONSENSUS, (int32_t)max_iterations_, inlier_threshold_}; }
  void takeBestTransformation(const float* colmajor16) override { std::memcpy(best_T_, colmajor16, sizeof best_T_); }
  Matrix4 getBestTransformation() const { return make_matrix4(best_T_); }

  // --- the rejector alone: clouds of 16-byte points, valid until getRemainingCorrespondences() returns
  template <class CloudPtr>
  void setInputSource(const CloudPtr& cloud) {
    static_assert(sizeof(cloud->points[0]) == 16, "point type must be the 16-byte pcl::PointXYZ layout");
    source_ = cloud->points.empty() ? nullptr : reinterpret_cast<const float*>(&cloud->points[0]);
    n_source_ = cloud->points.size();
  }
  template <class CloudPtr>
  void setInputTarget(const CloudPtr& cloud) {
    static_assert(sizeof(cloud->points[0]) == 16, "point type must be the 16-byte pcl::PointXYZ layout");
    target_ = cloud->points.empty() ? nullptr : reinterpret_cast<const float*>(&cloud->points[0]);
    n_target_ = cloud->points.size();
  }
  void setInputCorrespondences(const std::shared_ptr<const Correspondences>& correspondences) { input_ = correspondences; }
  void setInputCorrespondences(const std::shared_ptr<Correspondences>& correspondences) { input_ = correspondences; }
  // the pairs of `original` that stay, in their order; false (and `remaining` empty) when the library refuses the call
  bool getRemainingCorrespondences(const Correspondences& original, Correspondences& remaining) {
    remaining.clear();
    if (!ctx_holder_) ctx_holder_ = detail::acquire_context(device_);
    std::vector<int32_t> iq(original.size()), im(original.size()), kept(original.size());
    for (std::size_t r = 0; r < original.size(); ++r) iq[r] = original[r].index_query, im[r] = original[r].index_match;
    std::size_t n_kept = 0;
    if (icpgpu_correspondence_rejector_sample_consensus(ctx_holder_->ctx, source_, n_source_, target_, n_target_, iq.data(), im.data(), original.size(),
                                                        inlier_threshold_, max_iterations_, seed_, kept.data(), &n_kept, best_T_) != ICPGPU_OK)
      return false;
    remaining.reserve(n_kept);
    for (std::size_t r = 0; r < original.size(); ++r)
      if (kept[r]) remaining.push_back(original[r]);
    return true;
  }
  void getCorrespondences(Correspondences& correspondences) {
    if (input_) getRemainingCorrespondences(*input_, correspondences);
    else correspondences.clear();
  }
  const char* lastError() const { return ctx_holder_ ? icpgpu_last_error(ctx_holder_->ctx) : ""; }

 private:
  int device_;
  double inlier_threshold_ = 0.05;
  int max_iterations_ = 1000;
  uint64_t seed_ = 12345;
  float best_T_[16];
  const float *source_ = nullptr, *target_ = nullptr;
  std::size_t n_source_ = 0, n_target_ = 0;
  std::shared_ptr<const Correspondences> input_;
  detail::ContextPtr ctx_holder_;
};
}  // namespace registration

template <class CloudT>
class IterativeClosestPoint {
 public:
  typedef registration::CorrespondenceRejector::Ptr CorrespondenceRejectorPtr;
  // pcl::Registration's rejector chain (at most ICPGPU_MAX_REJECTORS; GICP and NDT ignore it, as PCL's classes do)
  void addCorrespondenceRejector(const CorrespondenceRejectorPtr& rejector) { correspondence_rejectors_.push_back(rejector); }
  std::vector<CorrespondenceRejectorPtr> getCorrespondenceRejectors() { return correspondence_rejectors_; }
  bool removeCorrespondenceRejector(unsigned int i) {
    if (i >= correspondence_rejectors_.size()) return false;
    correspondence_rejectors_.erase(correspondence_rejectors_.begin() + i);
    return true;
  }
  void clearCorrespondenceRejectors() { correspondence_rejectors_.clear(); }
  // pcl::Registration::setUseReciprocalCorrespondences (include/icpgpu.h, "reciprocal correspondences": the rule and its tie
  // deviation).  Read by IterativeClosestPoint and IterativeClosestPointWithNormals; on GeneralizedIterativeClosestPoint and
  // NormalDistributionsTransform the flag is stored and changes nothing, as in PCL.
  void setUseReciprocalCorrespondences(bool use_reciprocal_correspondence) { use_reciprocal_correspondence_ = use_reciprocal_correspondence; }
  bool getUseReciprocalCorrespondences() const { return use_reciprocal_correspondence_; }

  explicit IterativeClosestPoint(int device = 0, icpgpu_method method = ICPGPU_P2P_SVD)
      : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx) {
    icpgpu_default_params(&params_);
    params_.method = method;
    std::memset(&result_, 0, sizeof(result_));
    for (int i = 0; i < 16; ++i) result_.T[i] = (i % 5 == 0) ? 1.f : 0.f;
  }

  // --- the setters the reference calls (icp_odometer.cpp:189-194, octree_mapper.cpp:105-110) -------------------
  void setMaximumIterations(int n) { params_.max_iterations = n; }
  void setTransformationEpsilon(double eps) { params_.transformation_epsilon = eps; }
  void setMaxCorrespondenceDistance(double d) { params_.max_correspondence_distance = d; }
  void setEuclideanFitnessEpsilon(double eps) { params_.euclidean_fitness_epsilon = eps; }
  void setRANSACIterations(int n) { ransac_iterations_ = n; }  // the reference always passes 0 (no RANSAC rejector)
  template <class CloudPtr>
  void setInputSource(const CloudPtr& cloud) { source_ = &*cloud; }
  template <class CloudPtr>
  void setInputTarget(const CloudPtr& cloud) {
    target_ = &*cloud;
    target_from_map_ = false;
  }
  // the target is the nn cloud OctreeMap::approxNearestNeighbors just left in HBM (skips one host round trip): this
  // object then works on the MAP's context -- the one given, or the one of the map that last built an nn cloud on this thread
  // (no live map on this thread / a null context: there is no target -- align() then leaves hasConverged() false, like PCL's
  // initCompute() without a target)
  void setInputTargetFromMap() { setInputTargetFromMap(detail::last_map_context().lock()); }
  void setInputTargetFromMap(const detail::ContextPtr& map_context) {
    target_ = nullptr;
    target_from_map_ = static_cast<bool>(map_context);
    if (map_context) {
      ctx_holder_ = map_context;
      ctx_ = ctx_holder_->ctx;
    }
  }

  // NOT PCL methods (PCL reads normal_x/y/z of PointNormal clouds): n float4 {nx, ny, nz, pad}, n == the cloud's size, valid until
  // align() returns; nullptr goes back to the estimated normals.  The surface-normal rejector reads both on any registration
  // object; IterativeClosestPointWithNormals reads the target's, and the source's for the symmetric objective.
  void setSourceNormals(const float* nxyzw, std::size_t n) {
    source_normals_ = nxyzw;
    n_source_normals_ = nxyzw ? n : 0;
  }
  void setTargetNormals(const float* nxyzw, std::size_t n) {
    target_normals_ = nxyzw;
    n_target_normals_ = nxyzw ? n : 0;
  }

  void setFitnessWithAlign(bool on) { fitness_with_align_ = on; }  // no PCL counterpart
  int getMaximumIterations() const { return params_.max_iterations; }
  double getTransformationEpsilon() const { return params_.transformation_epsilon; }
  double getMaxCorrespondenceDistance() const { return params_.max_correspondence_distance; }

  // --- align(out) (icp_odometer.cpp:198, octree_mapper.cpp:114) -------------------------------------------------
  void align(CloudT& output) { align_impl(output, nullptr); }
  void align(CloudT& output, const Matrix4& guess) { align_impl(output, guess.data()); }

  Matrix4 getFinalTransformation() const { return make_matrix4(result_.T); }  // icp_odometer.cpp:199
  bool hasConverged() const { return result_.converged != 0; }                // icp_odometer.cpp:201
  double getFitnessScore(double max_range = DBL_MAX) {                        // icp_odometer.cpp:201
    double f = DBL_MAX;
    if (!aligned_) return DBL_MAX;
    // Something else may have replaced the context's clouds since (a map's context is shared with its OctreeMap, whose
    // next approxNearestNeighbors call does): put this object's clouds and transform back first.
    if (ctx_holder_->generation != generation_) {
      if (target_from_map_ || !source_ || !target_ || !upload()) return DBL_MAX;
      double sums[17];
      std::size_t n = source_->points.size();
      if (n == 0) return DBL_MAX;
      // mean squared distance of the neighbours within max_range under THIS object's transform (kernel-level entry points)
      if (fitness_sums_at(result_.T, max_range, sums) != ICPGPU_OK) return DBL_MAX;
      return sums[0] > 0.0 ? sums[16] / sums[0] : DBL_MAX;
    }
    if (fitness_with_align_ && max_range == DBL_MAX && result_.fitness == result_.fitness) return result_.fitness;
    if (icpgpu_fitness(ctx_, max_range, &f) != ICPGPU_OK) return DBL_MAX;
    return f;
  }
  const icpgpu_result& getResult() const { return result_; }
  const char* lastError() const { return icpgpu_last_error(ctx_); }

 private:
  using PointT = typename std::remove_reference<decltype(std::declval<CloudT>().points[0])>::type;
  static_assert(sizeof(PointT) == 16, "point type must be the 16-byte pcl::PointXYZ layout");

  std::vector<CorrespondenceRejectorPtr> correspondence_rejectors_;
  bool use_reciprocal_correspondence_ = false;
  bool apply_rejectors() {  // (always: an object without rejectors clears what another one left on a shared context; the flag likewise)
    std::vector<icpgpu_rejector> chain;
    for (const auto& r : correspondence_rejectors_) chain.push_back(r->entry());
    if (icpgpu_set_reciprocal_correspondences(ctx_, use_reciprocal_correspondence_ ? 1 : 0) != ICPGPU_OK) return false;
    return icpgpu_set_correspondence_rejectors(ctx_, chain.empty() ? nullptr : chain.data(), chain.size()) == ICPGPU_OK;
  }
  void take_rejector_stats() {
    float cut[ICPGPU_MAX_REJECTORS] = {0, 0, 0, 0};
    std::size_t n = 0;
    if (correspondence_rejectors_.empty() || icpgpu_rejector_stats(ctx_, ICPGPU_MAX_REJECTORS, nullptr, nullptr, cut, &n) != ICPGPU_OK) return;
    for (std::size_t s = 0; s < n && s < correspondence_rejectors_.size(); ++s) correspondence_rejectors_[s]->takeCut(cut[s]);
    // the last iteration's best transform goes to the sample-consensus rejector (the last one, when the chain holds several)
    for (std::size_t s = correspondence_rejectors_.size(); s-- > 0;) {
      if (correspondence_rejectors_[s]->entry().kind != ICPGPU_REJECT_SAMPLE_CONSENSUS) continue;
      float T[16];
      if (icpgpu_rejector_sac_fetch(ctx_, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, T, nullptr, nullptr) == ICPGPU_OK)
        correspondence_rejectors_[s]->takeBestTransformation(T);
      break;
    }
  }

  bool apply_ndt() {
    return icpgpu_set_ndt_params(ctx_, ndt_[0], ndt_[1], ndt_[2]) == ICPGPU_OK &&
           icpgpu_set_ndt_line_search(ctx_, ndt_line_search_) == ICPGPU_OK;
  }

  bool upload() {
    // the TARGET first: it is usually the cloud the context still holds as the previous scan's source
    // (`*prev_cloud_ = *curr_cloud_`, icp_odometer.cpp:209), which icpgpu_set_target recognises -- no upload, the grid
    // and the GICP covariances stay -- but only as long as set_source has not replaced it
    if (!target_from_map_) {
      const std::size_t nt = target_->points.size();
      if (!bound_) {
        detail::ContextPtr better = detail::rebind_for_target(ctx_holder_, nt);
        if (better != ctx_holder_) {
          ctx_holder_ = better;
          ctx_ = ctx_holder_->ctx;
        }
        bound_ = true;
      }
      if (icpgpu_set_params(ctx_, &params_) != ICPGPU_OK) return false;
      if (params_.method == ICPGPU_NDT && !apply_ndt()) return false;
      if (icpgpu_set_target(ctx_, nt ? reinterpret_cast<const float*>(&target_->points[0]) : nullptr, nt) != ICPGPU_OK) return false;
      // (after set_target, which drops the normals a target had: setTargetNormals)
      if (target_normals_ && icpgpu_set_target_normals(ctx_, target_normals_, n_target_normals_) != ICPGPU_OK) return false;
    } else if (icpgpu_set_params(ctx_, &params_) != ICPGPU_OK ||
               (params_.method == ICPGPU_NDT && !apply_ndt())) {
      return false;
    }
    if (!apply_rejectors()) return false;
    if (icpgpu_set_p2plane_symmetric(ctx_, p2plane_symmetric_ ? 1 : 0, enforce_same_direction_normals_ ? 1 : 0) != ICPGPU_OK) return false;
    const std::size_t ns = source_->points.size();
    if (icpgpu_set_source(ctx_, ns ? reinterpret_cast<const float*>(&source_->points[0]) : nullptr, ns) != ICPGPU_OK) return false;
    return !source_normals_ || icpgpu_set_source_normals(ctx_, source_normals_, n_source_normals_) == ICPGPU_OK;
  }

  // fitness through the kernel-level entry points, for a transform that is not the context's last one
  int fitness_sums_at(const float* T, double max_range, double sums[17]) {
    const std::size_t n = source_->points.size();
    std::unique_ptr<int32_t[]> idx(new int32_t[n]);
    std::unique_ptr<float[]> d2(new float[n]);
    int rc = icpgpu_nn(ctx_, T, idx.get(), d2.get());
    if (rc != ICPGPU_OK) return rc;
    // PCL compares SQUARED distances with max_range; icpgpu_reduce takes the distance
    return icpgpu_reduce(ctx_, T, max_range >= 1e36 ? 1e18 : std::sqrt(max_range), sums);
  }

  void align_impl(CloudT& output, const float* guess) {
    aligned_ = false;
    result_.converged = 0;
    if (!source_ || (!target_ && !target_from_map_)) return;  // PCL: initCompute() fails, align returns, converged_ stays false
    ICPGPU_SHIM_MARK(-1);
    if (!upload()) return;
    const std::size_t ns = source_->points.size();
    generation_ = ++ctx_holder_->generation;
    // getFitnessScore() nearly always follows (icp_odometer.cpp:201): evaluated inside align it is one more sweep queued behind
    // the last iteration instead of a call of its own (setFitnessWithAlign(false) for callers that never ask: octree_mapper.cpp:117).
    // The aligned cloud comes as a view of the context's pinned staging buffer (the transform kernel writes it there while the
    // fitness sweep is still to run): `assign` fills `output` in one pass -- resize() + a copy would touch it twice.
    const float* view = nullptr;
    std::size_t nv = 0;
    ICPGPU_SHIM_MARK(1);
    if (icpgpu_align_view(ctx_, guess, fitness_with_align_ ? 1 : 0, &result_, &view, &nv) != ICPGPU_OK || nv != ns) {
      result_.converged = 0;
      output.points.resize(ns);  // (PCL sizes the output before it computes anything)
      detail::set_cloud_shape(output, ns, 0);
      return;
    }
    ICPGPU_SHIM_MARK(2);
    const PointT* first = reinterpret_cast<const PointT*>(view);
    output.points.assign(first, first + nv);
    detail::set_cloud_shape(output, ns, 0);
    aligned_ = true;
    take_rejector_stats();
    ICPGPU_SHIM_MARK(3);
  }

  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  unsigned long long generation_ = 0;

 protected:
  icpgpu_params params_;  // (GeneralizedIterativeClosestPoint sets its solver options here)
  bool p2plane_symmetric_ = false, enforce_same_direction_normals_ = true;  // (IterativeClosestPointWithNormals::setUseSymmetricObjective)
  double ndt_[3] = {1.0, 0.1, 0.55};  // (NormalDistributionsTransform: resolution, step size, outlier ratio)
  int ndt_line_search_ = ICPGPU_NDT_LINE_SEARCH_PCL18;  // (NormalDistributionsTransform::setMoreThuenteLineSearch)
  icpgpu_ctx* context() const { return ctx_; }

 private:
  icpgpu_result result_;
  const CloudT* source_ = nullptr;
  const CloudT* target_ = nullptr;
  int ransac_iterations_ = 0;
  bool aligned_ = false;
  bool target_from_map_ = false;
  bool fitness_with_align_ = true;
  const float* source_normals_ = nullptr;  // the caller's normals, n float4 each (setSourceNormals / setTargetNormals)
  const float* target_normals_ = nullptr;
  std::size_t n_source_normals_ = 0, n_target_normals_ = 0;
  bool bound_ = false;  // the pool has been asked once for the context that suits this object's target
};

// pcl::GeneralizedIterativeClosestPoint<PointXYZ, PointXYZ>'s counterpart -- the class the reference instantiates at
// icp_odometer.cpp:188 and octree_mapper.cpp:104: same protocol, method = ICPGPU_GICP (plane-to-plane cost, BFGS inner solver,
// PCL's constructor defaults: 20 neighbours, gicp_epsilon 1e-3, rotation_epsilon 2e-3, 20 inner iterations).
template <class CloudT>
class GeneralizedIterativeClosestPoint : public IterativeClosestPoint<CloudT> {
 public:
  explicit GeneralizedIterativeClosestPoint(int device = 0) : IterativeClosestPoint<CloudT>(device, ICPGPU_GICP) {}
  // NOT a PCL method: the inner minimisation on the quadratic form of an outer iteration (icpgpu.h: icpgpu_gicp_inner) -- 2-3x the
  // scans/s of the reference's pipeline, results within the stated tolerance of the default's instead of on its bits.  An
  // unchanged call site opts in with ICPGPU_GICP_INNER=quadratic in the environment.
  void setQuadraticInnerSolver(bool on) { this->params_.gicp_inner = on ? ICPGPU_GICP_INNER_QUADRATIC : ICPGPU_GICP_INNER_EXACT; }
};

// pcl::IterativeClosestPointWithNormals<PointNormal, PointNormal>'s counterpart (TransformationEstimationPointToPlaneLLS): same
// protocol, method = ICPGPU_P2PLANE -- the point-to-point loop with the linearised point-to-plane solve (the alternative the reference
// names at icp_odometer.cpp:187).  The clouds stay 16-byte points; a PointNormal cloud's normals come separately through
// setTargetNormals / setSourceNormals (n float4 {nx, ny, nz, pad}, n == the cloud's size, valid until align() returns).  Without them the target's normals are
// estimated on the device: GICP's plane, not pcl::NormalEstimation's solve (include/icpgpu.h, ICPGPU_P2PLANE).  icpgpu::NormalEstimation
// below computes pcl::NormalEstimation's normals (k or radius, viewpoint, curvature); its getNormalsXYZC() is what setTargetNormals takes.
template <class CloudT>
class IterativeClosestPointWithNormals : public IterativeClosestPoint<CloudT> {
 public:
  explicit IterativeClosestPointWithNormals(int device = 0) : IterativeClosestPoint<CloudT>(device, ICPGPU_P2PLANE) {}
  // (setTargetNormals / setSourceNormals: the base class's)
  // TransformationEstimationSymmetricPointToPlaneLLS in place of ...PointToPlaneLLS (PCL >= 1.10; include/icpgpu.h, "symmetric
  // objective"): it reads the source's normals too -- setSourceNormals, else estimated like the target's
  void setUseSymmetricObjective(bool use_symmetric_objective) { this->p2plane_symmetric_ = use_symmetric_objective; }
  bool getUseSymmetricObjective() const { return this->p2plane_symmetric_; }
  void setEnforceSameDirectionNormals(bool enforce_same_direction_normals) { this->enforce_same_direction_normals_ = enforce_same_direction_normals; }
  bool getEnforceSameDirectionNormals() const { return this->enforce_same_direction_normals_; }
};

// pcl::NormalDistributionsTransform<PointXYZ, PointXYZ>'s counterpart: same protocol, method = ICPGPU_NDT -- the target's points in
// cells of `resolution` with one Gaussian each, a Newton loop on the Gauss-fitted score (include/icpgpu.h, ICPGPU_NDT).  PCL's
// constructor defaults: resolution 1.0, step size 0.1, outlier ratio 0.55, 35 iterations, transformation epsilon 0.1.  The
// reference's call sites swap the one type; their setMaxCorrespondenceDistance is accepted and not used by NDT.
template <class CloudT>
class NormalDistributionsTransform : public IterativeClosestPoint<CloudT> {
 public:
  explicit NormalDistributionsTransform(int device = 0) : IterativeClosestPoint<CloudT>(device, ICPGPU_NDT) {
    this->params_.max_iterations = 35;
    this->params_.transformation_epsilon = 0.1;
  }
  void setResolution(float resolution) { this->ndt_[0] = resolution; }
  float getResolution() const { return static_cast<float>(this->ndt_[0]); }
  void setStepSize(double step_size) { this->ndt_[1] = step_size; }
  double getStepSize() const { return this->ndt_[1]; }
  void setOulierRatio(double outlier_ratio) { this->ndt_[2] = outlier_ratio; }  // (PCL's spelling)
  double getOulierRatio() const { return this->ndt_[2]; }
  // NOT a PCL method: the More-Thuente line search with its loop running instead of PCL 1.8's clamped Newton step
  // (icpgpu_set_ndt_line_search; include/icpgpu.h)
  void setMoreThuenteLineSearch(bool on) {
    this->ndt_line_search_ = on ? ICPGPU_NDT_LINE_SEARCH_MORE_THUENTE : ICPGPU_NDT_LINE_SEARCH_PCL18;
  }
  bool getMoreThuenteLineSearch() const { return this->ndt_line_search_ == ICPGPU_NDT_LINE_SEARCH_MORE_THUENTE; }
  void align(CloudT& output) {
    IterativeClosestPoint<CloudT>::align(output);
    fetch_probability();
  }
  void align(CloudT& output, const Matrix4& guess) {
    IterativeClosestPoint<CloudT>::align(output, guess);
    fetch_probability();
  }
  double getTransformationProbability() const { return probability_; }
  int getFinalNumIteration() const { return this->getResult().iterations; }

 private:
  void fetch_probability() {
    probability_ = 0.0;
    if (icpgpu_ndt_transformation_probability(this->context(), &probability_) != ICPGPU_OK) probability_ = 0.0;
  }
  double probability_ = 0.0;
};

// pcl::VoxelGrid<PointT>-shaped front end for the odometer's pre-step
// (/root/reference/src/icpslam/icp_odometer.cpp:96-101):
//   pcl::VoxelGrid<pcl::PointXYZ> voxel_filter;  ->  icpgpu::VoxelGrid<pcl::PointCloud<pcl::PointXYZ>> voxel_filter;
//   voxel_filter.setInputCloud(in); voxel_filter.setLeafSize(l, l, l); voxel_filter.filter(out);
template <class CloudT>
class VoxelGrid {
 public:
  explicit VoxelGrid(int device = 0) : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx) {}
  template <class CloudPtr>
  void setInputCloud(const CloudPtr& cloud) { input_ = &*cloud; }
  void setLeafSize(float lx, float ly, float lz) {
    if (lx != ly || ly != lz) throw std::invalid_argument("icpgpu::VoxelGrid: only cubic leaves (the reference passes one size)");
    leaf_ = lx;
  }
  void filter(CloudT& output) {
    if (!input_) return;
    const std::size_t n = input_->points.size();
    std::size_t m = 0;
    // the result as a view of the context's pinned staging buffer (the points arrive there in front of the voxel count the call
    // waits for): `assign` sizes and fills `output` in one pass -- sizing it for the worst case first would value-initialise n points
    // (3.2 MB for a raw 200k-point scan) to receive a tenth of them, and a fetch of its own is a second round trip to the device
    typedef typename std::remove_reference<decltype(output.points[0])>::type PointT;
    static_assert(sizeof(PointT) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
    const float* view = nullptr;
    const int rc = icpgpu_voxel_grid_view(ctx_, n ? reinterpret_cast<const float*>(&input_->points[0]) : nullptr, n, leaf_, &view, &m);
    if (rc == ICPGPU_OK && m) {
      const PointT* first = reinterpret_cast<const PointT*>(view);
      output.points.assign(first, first + m);
    } else {
      output.points.resize(0);
    }
    detail::set_cloud_shape(output, output.points.size(), 0);
  }

 private:
  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  const CloudT* input_ = nullptr;
  float leaf_ = 0.1f;
};

// What pcl::StatisticalOutlierRemoval and pcl::RadiusOutlierRemoval share (the filters a front end puts between VoxelGrid and the
// registration): the input cloud, `negative`, filter(output) from the view, getRemovedIndices().  Rules and deviations:
// include/icpgpu.h, "outlier removal".  A refused call leaves `output` empty, as PCL's error path does.
template <class CloudT, class Derived>
class OutlierFilterBase {
 public:
  explicit OutlierFilterBase(int device = 0) : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx) {}
  template <class CloudPtr>
  void setInputCloud(const CloudPtr& cloud) { input_ = &*cloud; }
  void setNegative(bool negative) { negative_ = negative; }
  bool getNegative() const { return negative_; }
  // the indices of the points the last filter() removed, ascending (PCL: extract_removed_indices = true, then getRemovedIndices())
  const std::vector<int>& getRemovedIndices() const { return removed_; }
  void filter(CloudT& output) {
    removed_.clear();
    if (!input_) return;
    typedef typename std::remove_reference<decltype(output.points[0])>::type PointT;
    static_assert(sizeof(PointT) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
    const std::size_t n = input_->points.size();
    std::size_t m = 0;
    const float* view = nullptr;
    const int rc = static_cast<Derived*>(this)->run(ctx_, n ? reinterpret_cast<const float*>(&input_->points[0]) : nullptr, n, &view, &m);
    if (rc == ICPGPU_OK && m) {
      const PointT* first = reinterpret_cast<const PointT*>(view);
      output.points.assign(first, first + m);
    } else {
      output.points.resize(0);
    }
    detail::set_cloud_shape(output, output.points.size(), 0);
    if (rc != ICPGPU_OK || n == 0) return;
    std::vector<int32_t> kept(m);
    std::size_t n_in = 0, n_kept = 0;
    if (icpgpu_outlier_fetch(ctx_, n, nullptr, m ? &kept[0] : nullptr, &n_in, &n_kept) != ICPGPU_OK) return;
    removed_.reserve(n - m);
    std::size_t k = 0;
    for (std::size_t i = 0; i < n; ++i) {
      if (k < m && (std::size_t)kept[k] == i) ++k;
      else removed_.push_back((int)i);
    }
  }

 protected:
  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  const CloudT* input_ = nullptr;
  bool negative_ = false;
  std::vector<int> removed_;
};

//   pcl::StatisticalOutlierRemoval<pcl::PointXYZ> sor;  ->  icpgpu::StatisticalOutlierRemoval<pcl::PointCloud<pcl::PointXYZ>> sor;
//   sor.setInputCloud(in); sor.setMeanK(50); sor.setStddevMulThresh(1.0); sor.filter(out);
template <class CloudT>
class StatisticalOutlierRemoval : public OutlierFilterBase<CloudT, StatisticalOutlierRemoval<CloudT>> {
 public:
  explicit StatisticalOutlierRemoval(int device = 0) : OutlierFilterBase<CloudT, StatisticalOutlierRemoval<CloudT>>(device) {}
  void setMeanK(int k) { mean_k_ = k; }
  int getMeanK() const { return mean_k_; }
  void setStddevMulThresh(double m) { stddev_mult_ = m; }
  double getStddevMulThresh() const { return stddev_mult_; }
  int run(icpgpu_ctx* ctx, const float* xyzw, std::size_t n, const float** view, std::size_t* m) {
    return icpgpu_statistical_outlier_removal_view(ctx, xyzw, n, mean_k_, stddev_mult_, this->negative_ ? 1 : 0, view, m);
  }

 private:
  int mean_k_ = 1;  // (PCL's constructor defaults)
  double stddev_mult_ = 0.0;
};

//   pcl::RadiusOutlierRemoval<pcl::PointXYZ> ror;  ->  icpgpu::RadiusOutlierRemoval<pcl::PointCloud<pcl::PointXYZ>> ror;
//   ror.setInputCloud(in); ror.setRadiusSearch(0.3); ror.setMinNeighborsInRadius(5); ror.filter(out);
template <class CloudT>
class RadiusOutlierRemoval : public OutlierFilterBase<CloudT, RadiusOutlierRemoval<CloudT>> {
 public:
  explicit RadiusOutlierRemoval(int device = 0) : OutlierFilterBase<CloudT, RadiusOutlierRemoval<CloudT>>(device) {}
  void setRadiusSearch(double r) { radius_ = r; }
  double getRadiusSearch() const { return radius_; }
  void setMinNeighborsInRadius(int n) { min_pts_ = n; }
  int getMinNeighborsInRadius() const { return min_pts_; }
  int run(icpgpu_ctx* ctx, const float* xyzw, std::size_t n, const float** view, std::size_t* m) {
    return icpgpu_radius_outlier_removal_view(ctx, xyzw, n, radius_, min_pts_, this->negative_ ? 1 : 0, view, m);
  }

 private:
  double radius_ = 0.0;  // (PCL's constructor defaults)
  int min_pts_ = 1;
};

// What pcl::PassThrough, pcl::CropBox, pcl::UniformSampling and pcl::FarthestPointSampling share (the filters that keep a subset of
// the input rows): the input cloud, filter(output) from the view, filter(indices) -- the kept rows' indices -- and
// getRemovedIndices().  Rules and deviations: include/icpgpu.h, "cropping and sampling filters".  A refused call leaves the output
// empty, as PCL's error path does.  Not provided: setKeepOrganized / setUserFilterValue, setIndices.
template <class CloudT, class Derived>
class SubsetFilterBase {
 public:
  explicit SubsetFilterBase(int device = 0) : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx) {}
  template <class CloudPtr>
  void setInputCloud(const CloudPtr& cloud) { input_ = &*cloud; }
  // the indices of the rows the last filter() removed, ascending
  const std::vector<int>& getRemovedIndices() const { return removed_; }
  void filter(CloudT& output) {
    typedef typename std::remove_reference<decltype(output.points[0])>::type PointT;
    static_assert(sizeof(PointT) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
    const float* view = nullptr;
    const std::size_t m = call(&view);
    if (m) {
      const PointT* first = reinterpret_cast<const PointT*>(view);
      output.points.assign(first, first + m);
    } else {
      output.points.resize(0);
    }
    detail::set_cloud_shape(output, output.points.size(), 0);
    observe(nullptr);
  }
  // the kept rows' indices: ascending, or in selection order for FarthestPointSampling
  void filter(std::vector<int>& indices) {
    const float* view = nullptr;
    call(&view);
    observe(&indices);
  }

 protected:
  std::size_t call(const float** view) {
    removed_.clear();
    ok_ = false;
    if (!input_) return 0;
    const std::size_t n = input_->points.size();
    std::size_t m = 0;
    ok_ = static_cast<Derived*>(this)->run(ctx_, n ? reinterpret_cast<const float*>(&input_->points[0]) : nullptr, n, view, &m) == ICPGPU_OK;
    return ok_ ? m : 0;
  }
  void observe(std::vector<int>* indices) {
    if (indices) indices->clear();
    if (!ok_) return;
    std::size_t n_in = 0, n_kept = 0, n_removed = 0;
    if (icpgpu_subset_fetch(ctx_, 0, nullptr, nullptr, &n_in, &n_kept) != ICPGPU_OK) return;
    static_assert(sizeof(int) == sizeof(int32_t), "icpgpu: 32-bit int");
    if (indices && n_kept) {
      indices->resize(n_kept);
      if (icpgpu_subset_fetch(ctx_, n_kept, reinterpret_cast<int32_t*>(&(*indices)[0]), nullptr, &n_in, &n_kept) != ICPGPU_OK) indices->clear();
    }
    removed_.resize(n_in - n_kept);
    if (!removed_.empty() && icpgpu_subset_removed(ctx_, removed_.size(), reinterpret_cast<int32_t*>(&removed_[0]), &n_removed) != ICPGPU_OK)
      removed_.clear();
  }
  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  const CloudT* input_ = nullptr;
  bool ok_ = false;
  std::vector<int> removed_;
};

//   pcl::PassThrough<pcl::PointXYZ> pass;  ->  icpgpu::PassThrough<pcl::PointCloud<pcl::PointXYZ>> pass;
//   pass.setInputCloud(in); pass.setFilterFieldName("z"); pass.setFilterLimits(-1.5, 3.0); pass.filter(out);
template <class CloudT>
class PassThrough : public SubsetFilterBase<CloudT, PassThrough<CloudT>> {
 public:
  explicit PassThrough(int device = 0) : SubsetFilterBase<CloudT, PassThrough<CloudT>>(device) {}
  void setFilterFieldName(const std::string& name) {
    if (name != "x" && name != "y" && name != "z") throw std::invalid_argument("icpgpu::PassThrough: the field is one of x, y, z");
    field_ = name[0] - 'x';
  }
  std::string getFilterFieldName() const { return field_ < 0 ? std::string() : std::string(1, (char)('x' + field_)); }
  void setFilterLimits(float lo, float hi) { lo_ = lo, hi_ = hi; }
  void getFilterLimits(float& lo, float& hi) const { lo = lo_, hi = hi_; }
  void setNegative(bool negative) { negative_ = negative; }
  bool getNegative() const { return negative_; }
  int run(icpgpu_ctx* ctx, const float* xyzw, std::size_t n, const float** view, std::size_t* m) {
    return icpgpu_pass_through_view(ctx, xyzw, n, field_, lo_, hi_, negative_ ? 1 : 0, view, m);
  }

 private:
  int field_ = -1;  // (PCL's constructor defaults: no field, FLT_MIN .. FLT_MAX)
  float lo_ = std::numeric_limits<float>::min(), hi_ = std::numeric_limits<float>::max();
  bool negative_ = false;
};

//   pcl::CropBox<pcl::PointXYZ> crop;  ->  icpgpu::CropBox<pcl::PointCloud<pcl::PointXYZ>> crop;
//   crop.setInputCloud(in); crop.setMin(Eigen::Vector4f(...)); crop.setMax(...); crop.setNegative(true); crop.filter(out);
// setMin / setMax / setTranslation / setRotation read v[0], v[1], v[2]; setTransform reads t(r, c) for r, c < 4 (Eigen::Affine3f,
// Eigen::Matrix4f).  The three poses are composed into one matrix by icpgpu_crop_box_matrix.
template <class CloudT>
class CropBox : public SubsetFilterBase<CloudT, CropBox<CloudT>> {
 public:
  explicit CropBox(int device = 0) : SubsetFilterBase<CloudT, CropBox<CloudT>>(device) {}
  template <class Vec>
  void setMin(const Vec& v) { for (int a = 0; a < 3; ++a) min_[a] = (float)v[a]; }
  template <class Vec>
  void setMax(const Vec& v) { for (int a = 0; a < 3; ++a) max_[a] = (float)v[a]; }
  template <class Vec>
  void setTranslation(const Vec& v) { for (int a = 0; a < 3; ++a) translation_[a] = (float)v[a]; posed_ = true; }
  template <class Vec>
  void setRotation(const Vec& v) { for (int a = 0; a < 3; ++a) rotation_[a] = (float)v[a]; posed_ = true; }
  template <class TransformT>
  void setTransform(const TransformT& t) {
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) transform_[4 * c + r] = (float)t(r, c);
    posed_ = true;
  }
  void setNegative(bool negative) { negative_ = negative; }
  bool getNegative() const { return negative_; }
  int run(icpgpu_ctx* ctx, const float* xyzw, std::size_t n, const float** view, std::size_t* m) {
    float T[16];
    if (posed_ && icpgpu_crop_box_matrix(transform_, translation_, rotation_, T) != ICPGPU_OK) return ICPGPU_ERR_INVALID_ARG;
    return icpgpu_crop_box_view(ctx, xyzw, n, min_, max_, posed_ ? T : nullptr, negative_ ? 1 : 0, view, m);
  }

 private:
  float min_[3] = {-1.f, -1.f, -1.f}, max_[3] = {1.f, 1.f, 1.f};  // (PCL's constructor defaults)
  float translation_[3] = {0.f, 0.f, 0.f}, rotation_[3] = {0.f, 0.f, 0.f};
  float transform_[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  bool posed_ = false, negative_ = false;
};

//   pcl::UniformSampling<pcl::PointXYZ> us;  ->  icpgpu::UniformSampling<pcl::PointCloud<pcl::PointXYZ>> us;
//   us.setInputCloud(in); us.setRadiusSearch(0.5); us.filter(keypoints);      (filter(indices): the rows to compute descriptors at)
template <class CloudT>
class UniformSampling : public SubsetFilterBase<CloudT, UniformSampling<CloudT>> {
 public:
  explicit UniformSampling(int device = 0) : SubsetFilterBase<CloudT, UniformSampling<CloudT>>(device) {}
  void setRadiusSearch(double radius) { leaf_ = (float)radius; }
  double getRadiusSearch() const { return leaf_; }
  int run(icpgpu_ctx* ctx, const float* xyzw, std::size_t n, const float** view, std::size_t* m) {
    return icpgpu_uniform_sampling_view(ctx, xyzw, n, leaf_, view, m);
  }

 private:
  float leaf_ = 0.f;
};

//   pcl::FarthestPointSampling<pcl::PointXYZ> fps;  ->  icpgpu::FarthestPointSampling<pcl::PointCloud<pcl::PointXYZ>> fps;
//   fps.setInputCloud(in); fps.setSample(1024); fps.setSeed(7); fps.filter(out);
// The first row is the plane segmentation's generator (hypothesis 0, sample 0) over the cloud's rows, advanced cyclically to the
// next finite row -- not mt19937's draw; the rows come in selection order.
template <class CloudT>
class FarthestPointSampling : public SubsetFilterBase<CloudT, FarthestPointSampling<CloudT>> {
 public:
  explicit FarthestPointSampling(int device = 0) : SubsetFilterBase<CloudT, FarthestPointSampling<CloudT>>(device) {}
  void setSample(std::size_t sample) { sample_ = sample; }
  std::size_t getSample() const { return sample_; }
  void setSeed(unsigned int seed) { seed_ = seed; }
  unsigned int getSeed() const { return seed_; }
  int run(icpgpu_ctx* ctx, const float* xyzw, std::size_t n, const float** view, std::size_t* m) {
    int64_t first = -1;
    if (n) {
      unsigned long long z = (unsigned long long)seed_ + 0x9E3779B97F4A7C15ull;  // splitmix64 of the rule's counter 3 t + c + 1 = 1
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      z ^= z >> 31;
      const std::size_t start = (std::size_t)(((z >> 32) * (unsigned long long)n) >> 32);
      for (std::size_t step = 0; step < n && first < 0; ++step) {
        const float* p = xyzw + 4 * ((start + step) % n);
        if (std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2])) first = (int64_t)((start + step) % n);
      }
    }
    return icpgpu_farthest_point_sampling_view(ctx, xyzw, n, sample_, first, view, m);
  }

 private:
  std::size_t sample_ = 0;
  unsigned int seed_ = 0;
};

// pcl::search::KdTree<PointT> / pcl::KdTreeFLANN<PointT>-shaped front end of the neighbour search (rules and deviations:
// include/icpgpu.h, "neighbour search": exact, results ascending by (squared distance, index)):
//   pcl::search::KdTree<pcl::PointXYZ> tree;  ->  icpgpu::search::KdTree<pcl::PointCloud<pcl::PointXYZ>> tree;
//   tree.setInputCloud(cloud); tree.nearestKSearch(p, k, indices, sqr_distances); tree.radiusSearch(p, r, indices, sqr_distances);
// Every call returns the number of neighbours found, as PCL does (0 when the library refuses the call).  A single-point call is a
// whole round trip to the device: code that queries many points should use the batched forms, which take a query cloud and
// return rows.
namespace search {
template <class CloudT>
class KdTree {
 public:
  typedef std::shared_ptr<KdTree> Ptr;
  typedef std::shared_ptr<const KdTree> ConstPtr;
  explicit KdTree(int device = 0) : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx) {}
  template <class CloudPtr>
  void setInputCloud(const CloudPtr& cloud) {
    input_ = &*cloud;
    const std::size_t n = input_->points.size();
    static_assert(sizeof(input_->points[0]) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
    ready_ = icpgpu_search_set_input(ctx_, n ? reinterpret_cast<const float*>(&input_->points[0]) : nullptr, n) == ICPGPU_OK;
  }
  template <class PointT>
  int nearestKSearch(const PointT& point, int k, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances) {
    const float q[4] = {point.x, point.y, point.z, 1.0f};
    return knn_one(q, k, k_indices, k_sqr_distances);
  }
  int nearestKSearch(int index, int k, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances) {
    if (!input_ || index < 0 || (std::size_t)index >= input_->points.size()) return clear(k_indices, k_sqr_distances);
    return knn_one(reinterpret_cast<const float*>(&input_->points[index]), k, k_indices, k_sqr_distances);
  }
  template <class PointT>
  int radiusSearch(const PointT& point, double radius, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances, unsigned int max_nn = 0) {
    const float q[4] = {point.x, point.y, point.z, 1.0f};
    return radius_one(q, radius, max_nn, k_indices, k_sqr_distances);
  }
  int radiusSearch(int index, double radius, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances, unsigned int max_nn = 0) {
    if (!input_ || index < 0 || (std::size_t)index >= input_->points.size()) return clear(k_indices, k_sqr_distances);
    return radius_one(reinterpret_cast<const float*>(&input_->points[index]), radius, max_nn, k_indices, k_sqr_distances);
  }
  // Batched forms (not PCL's): every point of `queries` in one call.  Row i of k_indices / k_sqr_distances has k entries, the
  // first n_found[i] of them neighbours (the rest -1 / +inf); returns the number of queries answered.
  int nearestKSearch(const CloudT& queries, int k, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances, std::vector<int>& n_found) {
    const std::size_t nq = queries.points.size();
    k_indices.assign(k > 0 ? nq * (std::size_t)k : 0, -1);
    k_sqr_distances.resize(k_indices.size());
    n_found.assign(nq, 0);
    if (!ready_ || nq == 0 || k <= 0) return 0;
    static_assert(sizeof(int) == sizeof(int32_t), "icpgpu: 32-bit int");
    const int rc = icpgpu_search_knn(ctx_, reinterpret_cast<const float*>(&queries.points[0]), nq, k, reinterpret_cast<int32_t*>(&k_indices[0]),
                                     &k_sqr_distances[0], reinterpret_cast<int32_t*>(&n_found[0]));
    if (rc != ICPGPU_OK) {
      k_indices.clear(), k_sqr_distances.clear(), n_found.assign(nq, 0);
      return 0;
    }
    return (int)nq;
  }
  // Row i is k_indices / k_sqr_distances [row_start[i], row_start[i + 1]); returns the number of queries answered.
  int radiusSearch(const CloudT& queries, double radius, std::vector<long long>& row_start, std::vector<int>& k_indices,
                   std::vector<float>& k_sqr_distances, unsigned int max_nn = 0) {
    const std::size_t nq = queries.points.size();
    return radius_rows(nq ? reinterpret_cast<const float*>(&queries.points[0]) : nullptr, nq, radius, max_nn, row_start, k_indices, k_sqr_distances)
               ? (int)nq : 0;
  }

 private:
  static int clear(std::vector<int>& a, std::vector<float>& b) {
    a.clear(), b.clear();
    return 0;
  }
  int knn_one(const float* q, int k, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances) {
    if (!ready_ || k <= 0) return clear(k_indices, k_sqr_distances);
    k_indices.resize((std::size_t)k), k_sqr_distances.resize((std::size_t)k);
    int32_t found = 0;
    if (icpgpu_search_knn(ctx_, q, 1, k, reinterpret_cast<int32_t*>(&k_indices[0]), &k_sqr_distances[0], &found) != ICPGPU_OK)
      return clear(k_indices, k_sqr_distances);
    k_indices.resize((std::size_t)found), k_sqr_distances.resize((std::size_t)found);  // (PCL returns a short list too)
    return (int)found;
  }
  // the two-call protocol of icpgpu_search_radius: the first call sizes the arrays
  bool radius_rows(const float* q, std::size_t nq, double radius, unsigned int max_nn, std::vector<long long>& row_start, std::vector<int>& k_indices,
                   std::vector<float>& k_sqr_distances) {
    static_assert(sizeof(long long) == sizeof(int64_t), "icpgpu: 64-bit long long");
    row_start.assign(nq + 1, 0);
    clear(k_indices, k_sqr_distances);
    if (!ready_ || nq == 0 || max_nn > 0x7FFFFFFFu) return false;
    std::size_t total = 0;
    int rc = icpgpu_search_radius(ctx_, q, nq, radius, (int)max_nn, 0, reinterpret_cast<int64_t*>(&row_start[0]), nullptr, nullptr, &total);
    if (rc == ICPGPU_OK) return true;  // (nothing found)
    if (rc != ICPGPU_ERR_INVALID_ARG || total == 0) return false;
    k_indices.resize(total), k_sqr_distances.resize(total);
    rc = icpgpu_search_radius(ctx_, q, nq, radius, (int)max_nn, total, reinterpret_cast<int64_t*>(&row_start[0]),
                              reinterpret_cast<int32_t*>(&k_indices[0]), &k_sqr_distances[0], &total);
    if (rc == ICPGPU_OK) return true;
    row_start.assign(nq + 1, 0);
    clear(k_indices, k_sqr_distances);
    return false;
  }
  int radius_one(const float* q, double radius, unsigned int max_nn, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances) {
    std::vector<long long> row_start;
    radius_rows(q, 1, radius, max_nn, row_start, k_indices, k_sqr_distances);
    return (int)k_indices.size();
  }

  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  const CloudT* input_ = nullptr;
  bool ready_ = false;
};
}  // namespace search
template <class CloudT>
using KdTreeFLANN = search::KdTree<CloudT>;

// pcl::NormalEstimation<PointInT, PointOutT>-shaped front end (rules and deviations: include/icpgpu.h, "normal estimation"):
//   pcl::NormalEstimation<pcl::PointXYZ, pcl::Normal> ne;
//     ->  icpgpu::NormalEstimation<pcl::PointCloud<pcl::PointXYZ>, pcl::PointCloud<pcl::Normal>> ne;
//   ne.setInputCloud(cloud); ne.setSearchSurface(raw); ne.setKSearch(20) or ne.setRadiusSearch(0.5); ne.setViewPoint(x, y, z);
//   ne.compute(normals);
// The output point type only needs normal_x, normal_y, normal_z and curvature (pcl::Normal, pcl::PointNormal).  A point without a
// normal (fewer than three neighbours, a non-finite point) gets NaN in all four and clears is_dense, as in PCL; a refused call
// (both or neither of k and radius set, ...) leaves the output empty.  getNormalsXYZC() is what
// IterativeClosestPointWithNormals::setTargetNormals takes: the chain VoxelGrid -> StatisticalOutlierRemoval -> NormalEstimation ->
// IterativeClosestPointWithNormals stays on the device's rules end to end.
template <class CloudInT, class CloudOutT>
class NormalEstimation {
 public:
  explicit NormalEstimation(int device = 0) : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx) {}
  template <class CloudPtr>
  void setInputCloud(const CloudPtr& cloud) { input_ = &*cloud; }
  // the cloud the neighbours are taken from (PCL: a denser cloud than the input); without it the input cloud itself
  template <class CloudPtr>
  void setSearchSurface(const CloudPtr& cloud) { surface_ = &*cloud; }
  template <class TreePtr>
  void setSearchMethod(const TreePtr&) {}  // accepted and ignored: the search is the library's own (exact)
  void setKSearch(int k) { k_ = k; }
  int getKSearch() const { return k_; }
  void setRadiusSearch(double radius) { radius_ = radius; }
  double getRadiusSearch() const { return radius_; }
  void setViewPoint(float vpx, float vpy, float vpz) { vp_[0] = vpx, vp_[1] = vpy, vp_[2] = vpz; }
  void getViewPoint(float& vpx, float& vpy, float& vpz) const { vpx = vp_[0], vpy = vp_[1], vpz = vp_[2]; }
  void compute(CloudOutT& output) {
    normals_.clear();
    output.points.resize(0);
    detail::set_cloud_shape(output, 0, 0);
    if (!input_) return;
    static_assert(sizeof(input_->points[0]) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
    const CloudInT* surface = surface_ ? surface_ : input_;
    const std::size_t n = input_->points.size(), ns = surface->points.size();
    if (icpgpu_search_set_input(ctx_, ns ? reinterpret_cast<const float*>(&surface->points[0]) : nullptr, ns) != ICPGPU_OK) return;
    normals_.resize(4 * n);
    const float* queries = surface == input_ ? nullptr : (n ? reinterpret_cast<const float*>(&input_->points[0]) : nullptr);
    if (surface != input_ && n == 0) return;  // (null queries would mean the surface's own points)
    if (icpgpu_normal_estimation(ctx_, queries, n, k_, radius_, vp_, n ? &normals_[0] : nullptr, nullptr, nullptr) != ICPGPU_OK) {
      normals_.clear();
      return;
    }
    output.points.resize(n);
    detail::set_cloud_shape(output, n, 0);
    bool dense = true;
    for (std::size_t i = 0; i < n; ++i) {
      const float* v = &normals_[4 * i];
      output.points[i].normal_x = v[0];
      output.points[i].normal_y = v[1];
      output.points[i].normal_z = v[2];
      output.points[i].curvature = v[3];
      dense = dense && v[0] == v[0] && v[1] == v[1] && v[2] == v[2] && v[3] == v[3];
    }
    set_dense(output, dense, 0);
  }
  // NOT a PCL method: the last compute()'s normals as n float4 {nx, ny, nz, curvature} (empty after a refused call)
  const std::vector<float>& getNormalsXYZC() const { return normals_; }

 private:
  template <class C>
  static auto set_dense(C& c, bool dense, int) -> decltype(c.is_dense = true, void()) { c.is_dense = dense; }
  template <class C>
  static void set_dense(C&, bool, long) {}

  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  const CloudInT* input_ = nullptr;
  const CloudInT* surface_ = nullptr;
  int k_ = 0;
  double radius_ = 0.0;
  float vp_[3] = {0.f, 0.f, 0.f};
  std::vector<float> normals_;
};

// pcl::FPFHSignature33 and the pcl::FPFHEstimation<PointInT, PointNT, PointOutT>-shaped front end (rules and deviations:
// include/icpgpu.h, "fast point feature histograms"):
//   pcl::FPFHEstimation<pcl::PointXYZ, pcl::Normal, pcl::FPFHSignature33> fpfh;
//     ->  icpgpu::FPFHEstimation<pcl::PointCloud<pcl::PointXYZ>, pcl::PointCloud<pcl::Normal>, pcl::PointCloud<pcl::FPFHSignature33>> fpfh;
//   fpfh.setInputCloud(keypoints); fpfh.setSearchSurface(cloud); fpfh.setInputNormals(normals); fpfh.setKSearch(10) or
//   fpfh.setRadiusSearch(0.5); fpfh.compute(signatures);
// The normals are the search surface's -- the input cloud's when no surface is set -- one per point, as in PCL; the class takes
// icpgpu::NormalEstimation's output cloud directly (any point type with normal_x, normal_y, normal_z).  The output point type only
// needs float histogram[33] (pcl::FPFHSignature33, icpgpu::FPFHSignature33).  A non-finite input point gets 33 NaN and clears
// is_dense; a refused call (both or neither of k and radius set, normals that do not match the surface, ...) leaves the output empty.
struct FPFHSignature33 {
  float histogram[ICPGPU_FPFH_BINS];
  static int descriptorSize() { return ICPGPU_FPFH_BINS; }
};

template <class CloudInT, class CloudNT, class CloudOutT>
class FPFHEstimation {
 public:
  explicit FPFHEstimation(int device = 0) : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx) {}
  template <class CloudPtr>
  void setInputCloud(const CloudPtr& cloud) { input_ = &*cloud; }
  template <class NormalsPtr>
  void setInputNormals(const NormalsPtr& normals) { normals_ = &*normals; }
  // the cloud the neighbours and their normals are taken from (PCL: a denser cloud than the input); without it the input cloud itself
  template <class CloudPtr>
  void setSearchSurface(const CloudPtr& cloud) { surface_ = &*cloud; }
  template <class TreePtr>
  void setSearchMethod(const TreePtr&) {}  // accepted and ignored: the search is the library's own (exact)
  void setKSearch(int k) { k_ = k; }
  int getKSearch() const { return k_; }
  void setRadiusSearch(double radius) { radius_ = radius; }
  double getRadiusSearch() const { return radius_; }
  void compute(CloudOutT& output) {
    output.points.resize(0);
    detail::set_cloud_shape(output, 0, 0);
    if (!input_ || !normals_) return;
    static_assert(sizeof(input_->points[0]) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
    static_assert(sizeof(output.points[0].histogram) == ICPGPU_FPFH_BINS * sizeof(float), "icpgpu: float histogram[33] (pcl::FPFHSignature33)");
    const CloudInT* surface = surface_ ? surface_ : input_;
    const std::size_t n = input_->points.size(), ns = surface->points.size();
    if (normals_->points.size() != ns) return;  // (PCL refuses normals that do not match the surface as well)
    if (surface != input_ && n == 0) return;    // (null queries would mean the surface's own points)
    if (icpgpu_search_set_input(ctx_, ns ? reinterpret_cast<const float*>(&surface->points[0]) : nullptr, ns) != ICPGPU_OK) return;
    std::vector<float> nxyzc(4 * ns), hist(static_cast<std::size_t>(ICPGPU_FPFH_BINS) * n);
    for (std::size_t i = 0; i < ns; ++i) {
      nxyzc[4 * i] = normals_->points[i].normal_x;
      nxyzc[4 * i + 1] = normals_->points[i].normal_y;
      nxyzc[4 * i + 2] = normals_->points[i].normal_z;
      nxyzc[4 * i + 3] = 0.f;
    }
    const float* queries = surface == input_ ? nullptr : reinterpret_cast<const float*>(&input_->points[0]);
    if (icpgpu_fpfh_estimation(ctx_, ns ? &nxyzc[0] : nullptr, queries, n, k_, radius_, n ? &hist[0] : nullptr, nullptr, nullptr) != ICPGPU_OK) return;
    output.points.resize(n);
    detail::set_cloud_shape(output, n, 0);
    bool dense = true;
    for (std::size_t i = 0; i < n; ++i) {
      for (int b = 0; b < ICPGPU_FPFH_BINS; ++b) {
        const float v = hist[static_cast<std::size_t>(ICPGPU_FPFH_BINS) * i + b];
        output.points[i].histogram[b] = v;
        dense = dense && v == v;
      }
    }
    set_dense(output, dense, 0);
  }

 private:
  template <class C>
  static auto set_dense(C& c, bool dense, int) -> decltype(c.is_dense = true, void()) { c.is_dense = dense; }
  template <class C>
  static void set_dense(C&, bool, long) {}

  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  const CloudInT* input_ = nullptr;
  const CloudNT* normals_ = nullptr;
  const CloudInT* surface_ = nullptr;
  int k_ = 0;
  double radius_ = 0.0;
};

// pcl::Boundary and pcl::BoundaryEstimation<PointInT, PointNT, pcl::Boundary>-shaped front end (rules and deviations:
// include/icpgpu.h, "boundary estimation") -- which points lie on the rim of the sampled surface:
//   pcl::BoundaryEstimation<pcl::PointXYZ, pcl::Normal, pcl::Boundary> be;
//     ->  icpgpu::BoundaryEstimation<pcl::PointCloud<pcl::PointXYZ>, pcl::PointCloud<pcl::Normal>> be;
//   be.setInputCloud(cloud); be.setInputNormals(normals); be.setSearchSurface(surface); be.setKSearch(30) or be.setRadiusSearch(0.5);
//   be.setAngleThreshold(M_PI / 2); be.compute(boundaries);
// The normals are the INPUT cloud's, one per point, as in PCL (any point type with normal_x, normal_y, normal_z).  The output point
// type only needs boundary_point (pcl::Boundary, icpgpu::Boundary).  A refused call (both or neither of k and radius set, normals
// that do not match the input, a threshold outside (0, pi], ...) leaves the output empty.
struct Boundary {
  uint8_t boundary_point;
};

template <class CloudInT, class CloudNT>
class BoundaryEstimation {
 public:
  explicit BoundaryEstimation(int device = 0) : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx) {}
  template <class CloudPtr>
  void setInputCloud(const CloudPtr& cloud) { input_ = &*cloud; }
  template <class NormalsPtr>
  void setInputNormals(const NormalsPtr& normals) { normals_ = &*normals; }
  // the cloud the neighbours are taken from; without it the input cloud itself
  template <class CloudPtr>
  void setSearchSurface(const CloudPtr& cloud) { surface_ = &*cloud; }
  template <class TreePtr>
  void setSearchMethod(const TreePtr&) {}  // accepted and ignored: the search is the library's own (exact)
  void setKSearch(int k) { k_ = k; }
  int getKSearch() const { return k_; }
  void setRadiusSearch(double radius) { radius_ = radius; }
  double getRadiusSearch() const { return radius_; }
  void setAngleThreshold(float angle) { angle_ = angle; }
  float getAngleThreshold() const { return angle_; }
  template <class CloudOutT>
  void compute(CloudOutT& output) {
    output.points.resize(0);
    detail::set_cloud_shape(output, 0, 0);
    if (!input_ || !normals_) return;
    static_assert(sizeof(input_->points[0]) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
    const CloudInT* surface = surface_ ? surface_ : input_;
    const std::size_t n = input_->points.size(), ns = surface->points.size();
    if (normals_->points.size() != n) return;  // (PCL refuses normals that do not match the input as well)
    if (n == 0) return;
    if (icpgpu_search_set_input(ctx_, ns ? reinterpret_cast<const float*>(&surface->points[0]) : nullptr, ns) != ICPGPU_OK) return;
    std::vector<float> nxyzc(4 * n);
    std::vector<uint8_t> flags(n);
    for (std::size_t i = 0; i < n; ++i) {
      nxyzc[4 * i] = normals_->points[i].normal_x;
      nxyzc[4 * i + 1] = normals_->points[i].normal_y;
      nxyzc[4 * i + 2] = normals_->points[i].normal_z;
      nxyzc[4 * i + 3] = 0.f;
    }
    const float* queries = surface == input_ ? nullptr : reinterpret_cast<const float*>(&input_->points[0]);
    // (float -> double: PCL keeps the threshold as a float; M_PI as a float lies above pi, which the library refuses)
    const double angle = angle_ == static_cast<float>(3.14159265358979323846) ? 3.14159265358979323846 : static_cast<double>(angle_);
    if (icpgpu_boundary_estimation(ctx_, &nxyzc[0], queries, n, k_, radius_, angle, &flags[0], nullptr, nullptr, nullptr) != ICPGPU_OK) return;
    output.points.resize(n);
    detail::set_cloud_shape(output, n, 0);
    for (std::size_t i = 0; i < n; ++i) output.points[i].boundary_point = flags[i];
  }

 private:
  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  const CloudInT* input_ = nullptr;
  const CloudNT* normals_ = nullptr;
  const CloudInT* surface_ = nullptr;
  int k_ = 0;
  double radius_ = 0.0;
  float angle_ = 1.57079632679489661923f;  // PCL's default: M_PI / 2
};

// pcl::PointIndices and pcl::EuclideanClusterExtraction<PointT>-shaped front end (rules and deviations: include/icpgpu.h,
// "euclidean clustering"):
//   pcl::EuclideanClusterExtraction<pcl::PointXYZ> ec;  ->  icpgpu::EuclideanClusterExtraction<pcl::PointCloud<pcl::PointXYZ>> ec;
//   ec.setClusterTolerance(0.5); ec.setMinClusterSize(10); ec.setMaxClusterSize(25000); ec.setSearchMethod(tree);
//   ec.setInputCloud(cloud); std::vector<icpgpu::PointIndices> clusters; ec.extract(clusters);
// The clusters come out by size descending (the lowest index first among equal sizes), the indices ascending inside each; the
// defaults are PCL's constructor's (0, 1, INT_MAX).  A refused call leaves `clusters` empty.  setIndices is not provided.
struct PointIndices {
  typedef std::shared_ptr<PointIndices> Ptr;
  typedef std::shared_ptr<const PointIndices> ConstPtr;
  std::vector<int> indices;
};

template <class CloudT>
class EuclideanClusterExtraction {
 public:
  explicit EuclideanClusterExtraction(int device = 0) : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx) {}
  template <class CloudPtr>
  void setInputCloud(const CloudPtr& cloud) { input_ = &*cloud; }
  template <class TreePtr>
  void setSearchMethod(const TreePtr&) {}  // accepted and ignored: the search is the library's own (exact)
  void setClusterTolerance(double tolerance) { tolerance_ = tolerance; }
  double getClusterTolerance() const { return tolerance_; }
  void setMinClusterSize(int min_cluster_size) { min_ = min_cluster_size; }
  int getMinClusterSize() const { return min_; }
  void setMaxClusterSize(int max_cluster_size) { max_ = max_cluster_size; }
  int getMaxClusterSize() const { return max_; }
  void extract(std::vector<PointIndices>& clusters) {
    clusters.clear();
    labels_.clear();
    have_ = false;
    if (!input_) return;
    static_assert(sizeof(input_->points[0]) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
    static_assert(sizeof(int) == sizeof(int32_t) && sizeof(long long) == sizeof(int64_t), "icpgpu: 32-bit int, 64-bit long long");
    const std::size_t n = input_->points.size();
    if (icpgpu_search_set_input(ctx_, n ? reinterpret_cast<const float*>(&input_->points[0]) : nullptr, n) != ICPGPU_OK) return;
    std::size_t n_clusters = 0, n_clustered = 0;
    if (icpgpu_euclidean_cluster_extraction(ctx_, tolerance_, min_, max_, &n_clusters, &n_clustered) != ICPGPU_OK) return;
    have_ = true, n_emitted_ = n_clusters;
    std::vector<long long> start(n_clusters + 1, 0);
    std::vector<int> indices(n_clustered);
    labels_.assign(n, -1);
    if (icpgpu_cluster_fetch(ctx_, n_clusters, n_clustered, reinterpret_cast<int64_t*>(&start[0]),
                             n_clustered ? reinterpret_cast<int32_t*>(&indices[0]) : nullptr, n ? reinterpret_cast<int32_t*>(&labels_[0]) : nullptr,
                             nullptr) != ICPGPU_OK) {
      labels_.clear();
      return;
    }
    clusters.resize(n_clusters);
    for (std::size_t r = 0; r < n_clusters; ++r) clusters[r].indices.assign(indices.begin() + start[r], indices.begin() + start[r + 1]);
  }
  // NOT a PCL method: the last extract()'s cluster rank of every input point, -1 where it is in none (empty after a refused call)
  const std::vector<int>& getLabels() const { return labels_; }
  // NOT PCL methods: the context that holds the last extract()'s result on the device, and whether and how many clusters it holds
  // (what MomentOfInertiaEstimation::computeClusters reads)
  icpgpu_ctx* context() const { return ctx_; }
  bool hasResult() const { return have_; }
  std::size_t getNumberOfSegments() const { return n_emitted_; }

 private:
  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  const CloudT* input_ = nullptr;
  double tolerance_ = 0.0;
  int min_ = 1, max_ = 0x7FFFFFFF;
  bool have_ = false;
  std::size_t n_emitted_ = 0;
  std::vector<int> labels_;
};

// pcl::RegionGrowing<PointT, NormalT>-shaped front end (rules and deviations: include/icpgpu.h, "region growing" -- an ORDER-FREE
// rule, not PCL's seed queue: regions agree with PCL's on smooth surfaces and differ where PCL's depend on its visiting order):
//   pcl::RegionGrowing<pcl::PointXYZ, pcl::Normal> reg;
//     ->  icpgpu::RegionGrowing<pcl::PointCloud<pcl::PointXYZ>, pcl::PointCloud<pcl::Normal>> reg;
//   reg.setMinClusterSize(50); reg.setMaxClusterSize(1000000); reg.setSearchMethod(tree); reg.setNumberOfNeighbours(30);
//   reg.setInputCloud(cloud); reg.setInputNormals(normals); reg.setSmoothnessThreshold(3.0 / 180.0 * M_PI);
//   reg.setCurvatureThreshold(1.0); std::vector<icpgpu::PointIndices> clusters; reg.extract(clusters);
// The normals are one per input point (any point type with normal_x, normal_y, normal_z and curvature: icpgpu::NormalEstimation's
// output cloud as it is).  The regions come out by size descending (the lowest name first among equal sizes), the indices ascending
// inside each; the defaults are PCL's constructor's (30 neighbours, 30 degrees, curvature 0.05, sizes 1 .. INT_MAX, smooth mode and
// the curvature test on, the residual test off).  A refused call (no normals, normals that do not match the cloud, ...) leaves
// `clusters` empty.  setIndices is not provided; setSmoothModeFlag(false) and setResidualTestFlag(true) throw.
template <class CloudT, class NormalCloudT>
class RegionGrowing {
 public:
  explicit RegionGrowing(int device = 0) : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx) {}
  template <class CloudPtr>
  void setInputCloud(const CloudPtr& cloud) { input_ = &*cloud, have_ = false; }
  template <class NormalsPtr>
  void setInputNormals(const NormalsPtr& normals) { normals_ = &*normals, have_ = false; }
  template <class TreePtr>
  void setSearchMethod(const TreePtr&) {}  // accepted and ignored: the search is the library's own (exact)
  void setNumberOfNeighbours(unsigned int neighbour_number) { k_ = (int)neighbour_number; }
  unsigned int getNumberOfNeighbours() const { return (unsigned int)k_; }
  void setSmoothnessThreshold(float theta) { theta_ = theta; }  // radians
  float getSmoothnessThreshold() const { return theta_; }
  void setCurvatureThreshold(float curvature) { curvature_ = curvature; }
  float getCurvatureThreshold() const { return curvature_; }
  void setCurvatureTestFlag(bool value) { curvature_test_ = value; }
  bool getCurvatureTestFlag() const { return curvature_test_; }
  void setSmoothModeFlag(bool value) {
    if (!value) throw std::invalid_argument("icpgpu::RegionGrowing: setSmoothModeFlag(false) is not provided");
  }
  bool getSmoothModeFlag() const { return true; }
  void setResidualTestFlag(bool value) {
    if (value) throw std::invalid_argument("icpgpu::RegionGrowing: setResidualTestFlag(true) is not provided");
  }
  bool getResidualTestFlag() const { return false; }
  void setMinClusterSize(int min_cluster_size) { min_ = min_cluster_size; }
  int getMinClusterSize() const { return min_; }
  void setMaxClusterSize(int max_cluster_size) { max_ = max_cluster_size; }
  int getMaxClusterSize() const { return max_; }
  void extract(std::vector<PointIndices>& clusters) {
    clusters.clear();
    clusters_.clear();
    labels_.clear();
    have_ = false;
    if (!input_ || !normals_) return;
    static_assert(sizeof(input_->points[0]) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
    static_assert(sizeof(int) == sizeof(int32_t) && sizeof(long long) == sizeof(int64_t), "icpgpu: 32-bit int, 64-bit long long");
    const std::size_t n = input_->points.size();
    if (normals_->points.size() != n) return;
    std::vector<float> nxyzc(4 * n);
    for (std::size_t i = 0; i < n; ++i) {
      nxyzc[4 * i] = normals_->points[i].normal_x;
      nxyzc[4 * i + 1] = normals_->points[i].normal_y;
      nxyzc[4 * i + 2] = normals_->points[i].normal_z;
      nxyzc[4 * i + 3] = normals_->points[i].curvature;
    }
    if (icpgpu_search_set_input(ctx_, n ? reinterpret_cast<const float*>(&input_->points[0]) : nullptr, n) != ICPGPU_OK) return;
    const float smoothness_cos = (float)std::cos((double)theta_);
    const float threshold = curvature_test_ ? curvature_ : std::numeric_limits<float>::infinity();
    std::size_t n_regions = 0, n_in = 0;
    if (icpgpu_region_growing(ctx_, n ? &nxyzc[0] : nullptr, k_, smoothness_cos, threshold, min_, max_, &n_regions, &n_in) != ICPGPU_OK) return;
    std::vector<long long> start(n_regions + 1, 0);
    std::vector<int> indices(n_in);
    labels_.assign(n, -1);
    if (icpgpu_region_fetch(ctx_, n_regions, n_in, reinterpret_cast<int64_t*>(&start[0]), n_in ? reinterpret_cast<int32_t*>(&indices[0]) : nullptr,
                            n ? reinterpret_cast<int32_t*>(&labels_[0]) : nullptr, nullptr, nullptr, nullptr) != ICPGPU_OK) {
      labels_.clear();
      return;
    }
    clusters_.resize(n_regions);
    for (std::size_t r = 0; r < n_regions; ++r) clusters_[r].indices.assign(indices.begin() + start[r], indices.begin() + start[r + 1]);
    clusters = clusters_;
    have_ = true;
  }
  // the emitted region the point lies in (extract() runs first if it has not), empty when it lies in none or the index is outside
  void getSegmentFromPoint(int index, PointIndices& cluster) {
    cluster.indices.clear();
    if (!have_) {
      std::vector<PointIndices> clusters;
      extract(clusters);
    }
    if (!have_ || index < 0 || (std::size_t)index >= labels_.size() || labels_[index] < 0) return;
    cluster = clusters_[labels_[index]];
  }
  // NOT a PCL method: the last extract()'s region rank of every input point, -1 where it is in none (empty after a refused call)
  const std::vector<int>& getLabels() const { return labels_; }
  // NOT PCL methods: the context that holds the last extract()'s result on the device, and whether and how many regions it holds
  // (what MomentOfInertiaEstimation::computeRegions reads)
  icpgpu_ctx* context() const { return ctx_; }
  bool hasResult() const { return have_; }
  std::size_t getNumberOfSegments() const { return clusters_.size(); }

 private:
  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  const CloudT* input_ = nullptr;
  const NormalCloudT* normals_ = nullptr;
  int k_ = 30;
  float theta_ = 30.0f / 180.0f * 3.14159265358979323846f;  // PCL's default
  float curvature_ = 0.05f;
  bool curvature_test_ = true, have_ = false;
  int min_ = 1, max_ = 0x7FFFFFFF;
  std::vector<int> labels_;
  std::vector<PointIndices> clusters_;
};

// pcl::MomentOfInertiaEstimation<PointT>-shaped front end (rules and deviations: include/icpgpu.h, "segment moments"):
//   pcl::MomentOfInertiaEstimation<pcl::PointXYZ> fe;  ->  icpgpu::MomentOfInertiaEstimation<pcl::PointCloud<pcl::PointXYZ>> fe;
//   fe.setInputCloud(cloud); fe.setIndices(indices); fe.compute();
//   fe.getAABB(min, max); fe.getOBB(min, max, position, rotation); fe.getEigenValues(major, middle, minor);
//   fe.getEigenVectors(major, middle, minor); fe.getMassCenter(centre);
// The points are anything with x, y, z; the vectors anything with operator[]; the rotation anything with operator()(row, column)
// (Eigen's or this header's).  As in PCL the oriented box's min and max are relative to its centre `position` and the rotation's
// COLUMNS are the major, middle and minor axis.  The getters return false before a successful compute and for an EMPTY segment.
// Beyond PCL, every segment of a segmentation in ONE call: compute(segments) over a vector of PointIndices, computeClusters(ec) and
// computeRegions(reg) over the result the extractor's last extract() left ON THE DEVICE (no indices travel); getRecords() then
// holds one icpgpu_segment_record per segment and the getters describe the first.  getMomentOfInertia, getEccentricity,
// setAngleStep and setIndices on top of a segment list throw.
template <class CloudT>
class MomentOfInertiaEstimation {
 public:
  explicit MomentOfInertiaEstimation(int device = 0) : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx) {}
  template <class CloudPtr>
  void setInputCloud(const CloudPtr& cloud) { input_ = &*cloud, records_.clear(); }
  template <class IndicesPtr>
  void setIndices(const IndicesPtr& indices) { indices_ = indices->indices, have_indices_ = true, records_.clear(); }
  void setAngleStep(float) { throw std::invalid_argument("icpgpu::MomentOfInertiaEstimation: the moment-of-inertia sweep is not provided"); }
  bool getMomentOfInertia(std::vector<float>&) const { throw std::invalid_argument("icpgpu::MomentOfInertiaEstimation: getMomentOfInertia is not provided"); }
  bool getEccentricity(std::vector<float>&) const { throw std::invalid_argument("icpgpu::MomentOfInertiaEstimation: getEccentricity is not provided"); }
  // one segment: the indices, or the whole cloud
  void compute() {
    records_.clear();
    if (!input_) return;
    std::vector<PointIndices> one(1);
    if (have_indices_) {
      one[0].indices = indices_;
    } else {
      one[0].indices.resize(input_->points.size());
      for (std::size_t i = 0; i < one[0].indices.size(); ++i) one[0].indices[i] = (int)i;
    }
    run_host(one);
  }
  // NOT PCL methods: every segment in one call
  void compute(const std::vector<PointIndices>& segments) {
    if (have_indices_) throw std::invalid_argument("icpgpu::MomentOfInertiaEstimation: setIndices on top of a segment list is not provided");
    records_.clear();
    if (input_) run_host(segments);
  }
  template <class ExtractorT>
  void computeClusters(const ExtractorT& ec) { run_device(ec, ICPGPU_SEGMENTS_CLUSTERS); }
  template <class ExtractorT>
  void computeRegions(const ExtractorT& reg) { run_device(reg, ICPGPU_SEGMENTS_REGIONS); }
  const std::vector<icpgpu_segment_record>& getRecords() const { return records_; }

  template <class PointT>
  bool getAABB(PointT& min_point, PointT& max_point) const {
    if (!usable()) return false;
    const icpgpu_segment_record& r = records_[0];
    min_point.x = r.aabb_min[0], min_point.y = r.aabb_min[1], min_point.z = r.aabb_min[2];
    max_point.x = r.aabb_max[0], max_point.y = r.aabb_max[1], max_point.z = r.aabb_max[2];
    return true;
  }
  template <class PointT, class Matrix3T>
  bool getOBB(PointT& min_point, PointT& max_point, PointT& position, Matrix3T& rotational_matrix) const {
    if (!usable()) return false;
    const icpgpu_segment_record& r = records_[0];
    max_point.x = (float)(r.obb_dims[0] / 2.0), max_point.y = (float)(r.obb_dims[1] / 2.0), max_point.z = (float)(r.obb_dims[2] / 2.0);
    min_point.x = -max_point.x, min_point.y = -max_point.y, min_point.z = -max_point.z;
    position.x = (float)r.obb_position[0], position.y = (float)r.obb_position[1], position.z = (float)r.obb_position[2];
    for (int a = 0; a < 3; ++a)
      for (int k = 0; k < 3; ++k) rotational_matrix(k, a) = (float)r.axes[3 * a + k];
    return true;
  }
  bool getEigenValues(float& major, float& middle, float& minor) const {
    if (!usable()) return false;
    major = (float)records_[0].eigenvalues[0], middle = (float)records_[0].eigenvalues[1], minor = (float)records_[0].eigenvalues[2];
    return true;
  }
  template <class Vector3T>
  bool getEigenVectors(Vector3T& major, Vector3T& middle, Vector3T& minor) const {
    if (!usable()) return false;
    for (int k = 0; k < 3; ++k) major[k] = (float)records_[0].axes[k], middle[k] = (float)records_[0].axes[3 + k], minor[k] = (float)records_[0].axes[6 + k];
    return true;
  }
  template <class Vector3T>
  bool getMassCenter(Vector3T& mass_center) const {
    if (!usable()) return false;
    for (int k = 0; k < 3; ++k) mass_center[k] = (float)records_[0].centroid[k];
    return true;
  }

 private:
  bool usable() const { return !records_.empty() && records_[0].status == ICPGPU_SEGMENT_OK; }
  void run_host(const std::vector<PointIndices>& segments) {
    static_assert(sizeof(input_->points[0]) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
    static_assert(sizeof(int) == sizeof(int32_t), "icpgpu: 32-bit int");
    const std::size_t n = input_->points.size();
    std::vector<int64_t> start(segments.size() + 1, 0);
    for (std::size_t r = 0; r < segments.size(); ++r) start[r + 1] = start[r] + (int64_t)segments[r].indices.size();
    std::vector<int32_t> flat;
    flat.reserve((std::size_t)start.back());
    for (const PointIndices& s : segments) flat.insert(flat.end(), s.indices.begin(), s.indices.end());
    if (icpgpu_search_set_input(ctx_, n ? reinterpret_cast<const float*>(&input_->points[0]) : nullptr, n) != ICPGPU_OK) return;
    records_.resize(segments.size());
    if (icpgpu_segment_moments(ctx_, ICPGPU_SEGMENTS_HOST, segments.size(), &start[0], flat.empty() ? nullptr : &flat[0], sizeof(icpgpu_segment_record),
                               records_.empty() ? nullptr : &records_[0]) != ICPGPU_OK)
      records_.clear();
  }
  template <class ExtractorT>
  void run_device(const ExtractorT& extractor, int source) {
    if (have_indices_) throw std::invalid_argument("icpgpu::MomentOfInertiaEstimation: setIndices on top of a segment list is not provided");
    records_.clear();
    if (!extractor.hasResult()) return;
    records_.resize(extractor.getNumberOfSegments());
    if (icpgpu_segment_moments(extractor.context(), source, records_.size(), nullptr, nullptr, sizeof(icpgpu_segment_record),
                               records_.empty() ? nullptr : &records_[0]) != ICPGPU_OK)
      records_.clear();
  }

  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  const CloudT* input_ = nullptr;
  std::vector<int> indices_;
  bool have_indices_ = false;
  std::vector<icpgpu_segment_record> records_;
};

// pcl::getMinMax3D, pcl::compute3DCentroid and pcl::computeMeanAndCovarianceMatrix over a cloud and an index list, as one-segment
// calls of the same rule ("segment moments": the NORMALISED covariance, as PCL's).  min_pt / max_pt / centroid: anything with
// operator[] and four entries (the fourth is set to 0 for the extremes and to 1 for the centroid, as PCL does); covariance_matrix:
// anything with operator()(row, column).  The two counting functions return the number of finite listed points, 0 on a refusal.
namespace detail {
template <class CloudT>
inline bool one_segment(const CloudT& cloud, const std::vector<int>& indices, icpgpu_segment_record& r) {
  static_assert(sizeof(cloud.points[0]) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
  ContextPtr holder = acquire_context(0);
  const std::size_t n = cloud.points.size();
  const int64_t start[2] = {0, (int64_t)indices.size()};
  if (icpgpu_search_set_input(holder->ctx, n ? reinterpret_cast<const float*>(&cloud.points[0]) : nullptr, n) != ICPGPU_OK) return false;
  return icpgpu_segment_moments(holder->ctx, ICPGPU_SEGMENTS_HOST, 1, start, indices.empty() ? nullptr : reinterpret_cast<const int32_t*>(&indices[0]),
                                sizeof r, &r) == ICPGPU_OK && r.status == ICPGPU_SEGMENT_OK;
}
}  // namespace detail

template <class CloudT, class Vector4T>
inline void getMinMax3D(const CloudT& cloud, const std::vector<int>& indices, Vector4T& min_pt, Vector4T& max_pt) {
  icpgpu_segment_record r;
  if (!detail::one_segment(cloud, indices, r)) return;
  for (int k = 0; k < 3; ++k) min_pt[k] = r.aabb_min[k], max_pt[k] = r.aabb_max[k];
  min_pt[3] = 0, max_pt[3] = 0;
}
template <class CloudT, class Vector4T>
inline unsigned int compute3DCentroid(const CloudT& cloud, const std::vector<int>& indices, Vector4T& centroid) {
  icpgpu_segment_record r;
  if (!detail::one_segment(cloud, indices, r)) return 0;
  for (int k = 0; k < 3; ++k) centroid[k] = (typename std::decay<decltype(centroid[0])>::type)r.centroid[k];
  centroid[3] = 1;
  return (unsigned int)r.count;
}
template <class CloudT, class Matrix3T, class Vector4T>
inline unsigned int computeMeanAndCovarianceMatrix(const CloudT& cloud, const std::vector<int>& indices, Matrix3T& covariance_matrix, Vector4T& centroid) {
  icpgpu_segment_record r;
  if (!detail::one_segment(cloud, indices, r)) return 0;
  const int at[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
  for (int a = 0; a < 3; ++a) {
    centroid[a] = (typename std::decay<decltype(centroid[0])>::type)r.centroid[a];
    for (int b = 0; b < 3; ++b) covariance_matrix(a, b) = (typename std::decay<decltype(covariance_matrix(0, 0))>::type)r.cov[at[a][b]];
  }
  centroid[3] = 1;
  return (unsigned int)r.count;
}

// pcl::ISSKeypoint3D<PointT, PointT>-shaped front end (rules and deviations: include/icpgpu.h, "ISS keypoints") -- the keypoints at
// which FPFHEstimation computes its descriptors (fpfh.setInputCloud(keypoints); fpfh.setSearchSurface(cloud)):
//   pcl::ISSKeypoint3D<pcl::PointXYZ, pcl::PointXYZ> iss;  ->  icpgpu::ISSKeypoint3D<pcl::PointCloud<pcl::PointXYZ>> iss;
//   iss.setSalientRadius(1.2); iss.setNonMaxRadius(0.8); iss.setThreshold21(0.975); iss.setThreshold32(0.975); iss.setMinNeighbors(5);
//   iss.setInputCloud(cloud); iss.compute(keypoints); iss.getKeypointsIndices();
// The defaults are PCL's constructor's (radii 0, gammas 0.975, 5 neighbours): compute() leaves the output empty until both radii are
// set, and after any refused call.  The keypoints come out in the input's order.  Border estimation is
// ISSKeypoint3DBorder's, below: on this class setBorderRadius with a radius above 0 throws; setNormalRadius and setNumberOfThreads
// are stored and have no effect.  setIndices and a search surface other than the input are not provided.
template <class CloudT>
class ISSKeypoint3D {
 public:
  explicit ISSKeypoint3D(int device = 0) : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx), indices_(new PointIndices) {}
  template <class CloudPtr>
  void setInputCloud(const CloudPtr& cloud) { input_ = &*cloud; }
  template <class TreePtr>
  void setSearchMethod(const TreePtr&) {}  // accepted and ignored: the search is the library's own (exact)
  void setSalientRadius(double salient_radius) { salient_ = salient_radius; }
  void setNonMaxRadius(double non_max_radius) { non_max_ = non_max_radius; }
  void setThreshold21(double gamma_21) { gamma_21_ = gamma_21; }
  void setThreshold32(double gamma_32) { gamma_32_ = gamma_32; }
  void setMinNeighbors(int min_neighbors) { min_neighbors_ = min_neighbors; }
  void setBorderRadius(double border_radius) {
    if (border_radius > 0.0) throw std::invalid_argument("icpgpu::ISSKeypoint3D: border estimation is not provided");
    border_ = border_radius;
  }
  void setNormalRadius(double normal_radius) { normal_radius_ = normal_radius; }  // stored: without border estimation it has no effect
  void setNumberOfThreads(unsigned int nr_threads = 0) { threads_ = nr_threads; }  // stored: the kernels' parallelism is the device's
  void compute(CloudT& output) {
    output.points.resize(0);
    detail::set_cloud_shape(output, 0, 0);
    indices_.reset(new PointIndices);
    if (!input_) return;
    typedef typename std::remove_reference<decltype(input_->points[0])>::type PointT;
    static_assert(sizeof(PointT) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
    static_assert(sizeof(int) == sizeof(int32_t), "icpgpu: 32-bit int");
    const std::size_t n = input_->points.size();
    if (icpgpu_search_set_input(ctx_, n ? reinterpret_cast<const float*>(&input_->points[0]) : nullptr, n) != ICPGPU_OK) return;
    std::size_t m = 0;
    if (icpgpu_iss_keypoints(ctx_, salient_, non_max_, gamma_21_, gamma_32_, min_neighbors_, &m) != ICPGPU_OK || m == 0) return;
    indices_->indices.resize(m);
    output.points.resize(m);
    if (icpgpu_iss_fetch(ctx_, m, reinterpret_cast<int32_t*>(&indices_->indices[0]), reinterpret_cast<float*>(&output.points[0]), nullptr, nullptr,
                         nullptr, nullptr) != ICPGPU_OK) {
      indices_->indices.clear();
      output.points.resize(0);
      return;
    }
    detail::set_cloud_shape(output, m, 0);
  }
  // the last compute()'s keypoints as ascending indices into the input cloud
  PointIndices::ConstPtr getKeypointsIndices() const { return indices_; }

 protected:  // (ISSKeypoint3DBorder below)
  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  const CloudT* input_ = nullptr;
  double salient_ = 0.0, non_max_ = 0.0, gamma_21_ = 0.975, gamma_32_ = 0.975, border_ = 0.0, normal_radius_ = 0.0;
  int min_neighbors_ = 5;
  unsigned int threads_ = 0;
  PointIndices::Ptr indices_;
};

// pcl::MovingLeastSquares<PointInT, PointOutT>-shaped front end (rules and deviations: include/icpgpu.h, "moving least squares") -- the
// smoothing in front of NormalEstimation on a scan with range noise:
//   pcl::MovingLeastSquares<pcl::PointXYZ, pcl::PointNormal> mls;
//     ->  icpgpu::MovingLeastSquares<pcl::PointCloud<pcl::PointXYZ>, pcl::PointCloud<pcl::PointNormal>> mls;
//   mls.setInputCloud(cloud); mls.setSearchRadius(0.45); mls.setPolynomialOrder(2); mls.setComputeNormals(true);
//   mls.process(smoothed); mls.getCorrespondingIndices();
// The defaults are PCL's constructor's (radius 0, order 2, the squared Gaussian parameter the radius squared, no normals): process()
// leaves the output empty until a radius is set, and after any refused call.  The output holds the kept points in the input's
// order: x, y, z and -- where the output point type has them and setComputeNormals(true) was called -- normal_x, normal_y, normal_z
// and curvature (not normalised: PCL 1.8).  setPolynomialFit(false) is order 0.  setUpsamplingMethod takes NONE alone; the other
// methods, setDilation*, setIndices and getMLSResults are not provided.
template <class CloudInT, class CloudOutT>
class MovingLeastSquares {
 public:
  enum UpsamplingMethod { NONE, DISTINCT_CLOUD, SAMPLE_LOCAL_PLANE, RANDOM_UNIFORM_DENSITY, VOXEL_GRID_DILATION };
  explicit MovingLeastSquares(int device = 0) : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx), indices_(new PointIndices) {}
  template <class CloudPtr>
  void setInputCloud(const CloudPtr& cloud) { input_ = &*cloud; }
  template <class TreePtr>
  void setSearchMethod(const TreePtr&) {}  // accepted and ignored: the search is the library's own (exact)
  void setSearchRadius(double radius) { radius_ = radius; }
  double getSearchRadius() const { return radius_; }
  void setPolynomialOrder(int order) { order_ = order; }
  int getPolynomialOrder() const { return order_; }
  void setPolynomialFit(bool polynomial_fit) { polynomial_fit_ = polynomial_fit; }
  bool getPolynomialFit() const { return polynomial_fit_; }
  void setSqrGaussParam(double sqr_gauss_param) { sqr_gauss_param_ = sqr_gauss_param; }
  double getSqrGaussParam() const { return sqr_gauss_param_ == 0.0 ? radius_ * radius_ : sqr_gauss_param_; }
  void setComputeNormals(bool compute_normals) { compute_normals_ = compute_normals; }
  void setUpsamplingMethod(UpsamplingMethod method) {
    if (method != NONE) throw std::invalid_argument("icpgpu::MovingLeastSquares: upsampling is not provided");
  }
  void process(CloudOutT& output) {
    output.points.resize(0);
    detail::set_cloud_shape(output, 0, 0);
    indices_.reset(new PointIndices);
    if (!input_) return;
    static_assert(sizeof(input_->points[0]) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
    static_assert(sizeof(int) == sizeof(int32_t), "icpgpu: 32-bit int");
    const std::size_t n = input_->points.size();
    if (icpgpu_search_set_input(ctx_, n ? reinterpret_cast<const float*>(&input_->points[0]) : nullptr, n) != ICPGPU_OK) return;
    std::vector<float> xyzw(4 * n), nxyzc(compute_normals_ ? 4 * n : 0);
    indices_->indices.resize(n);
    std::size_t m = 0;
    if (icpgpu_moving_least_squares(ctx_, nullptr, n, radius_, polynomial_fit_ ? order_ : 0, sqr_gauss_param_, n ? &xyzw[0] : nullptr,
                                    compute_normals_ && n ? &nxyzc[0] : nullptr, n ? reinterpret_cast<int32_t*>(&indices_->indices[0]) : nullptr,
                                    &m) != ICPGPU_OK) {
      indices_->indices.clear();
      return;
    }
    indices_->indices.resize(m);
    output.points.resize(m);
    detail::set_cloud_shape(output, m, 0);
    for (std::size_t i = 0; i < m; ++i) {
      output.points[i].x = xyzw[4 * i];
      output.points[i].y = xyzw[4 * i + 1];
      output.points[i].z = xyzw[4 * i + 2];
      if (compute_normals_) set_normal(output.points[i], &nxyzc[4 * i], 0);
    }
  }
  // the last process()'s kept points as ascending indices into the input cloud (PCL's corresponding_input_indices)
  PointIndices::ConstPtr getCorrespondingIndices() const { return indices_; }

 private:
  template <class P>
  static auto set_normal(P& p, const float* v, int) -> decltype(p.normal_x = 0.f, p.normal_y = 0.f, p.normal_z = 0.f, p.curvature = 0.f, void()) {
    p.normal_x = v[0], p.normal_y = v[1], p.normal_z = v[2], p.curvature = v[3];
  }
  template <class P>
  static void set_normal(P&, const float*, long) {}

  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  const CloudInT* input_ = nullptr;
  double radius_ = 0.0, sqr_gauss_param_ = 0.0;
  int order_ = 2;
  bool polynomial_fit_ = true, compute_normals_ = false;
  PointIndices::Ptr indices_;
};

// ISSKeypoint3D with PCL's border estimation (include/icpgpu.h, "ISS keypoints", BORDER ESTIMATION): setBorderRadius,
// setNormalRadius, setNormals and setAngleThreshold work as in pcl::ISSKeypoint3D, and compute() refuses every keypoint within the
// border radius of a boundary point of the cloud.  Beyond PCL: getEdgePoints() and getBorderPoints().  NormalCloudT: any cloud
// whose points have normal_x, normal_y, normal_z (icpgpu::NormalEstimation's output).  It is a class of its own, and not
// ISSKeypoint3D itself, because the tests of the change that added ISSKeypoint3D pin that its setBorderRadius(r > 0) throws;
// folding the two is left to a change that may edit them.
template <class CloudT, class NormalCloudT>
class ISSKeypoint3DBorder : public ISSKeypoint3D<CloudT> {
  typedef ISSKeypoint3D<CloudT> Base;

 public:
  explicit ISSKeypoint3DBorder(int device = 0) : Base(device), edge_(new PointIndices), border_points_(new PointIndices) {}
  void setBorderRadius(double border_radius) { this->border_ = border_radius; }
  void setNormalRadius(double normal_radius) { this->normal_radius_ = normal_radius; }
  template <class NormalsPtr>
  void setNormals(const NormalsPtr& normals) { normals_ = &*normals; }
  void setAngleThreshold(float angle) { angle_ = angle; }
  void compute(CloudT& output) {
    output.points.resize(0);
    detail::set_cloud_shape(output, 0, 0);
    this->indices_.reset(new PointIndices);
    edge_.reset(new PointIndices);
    border_points_.reset(new PointIndices);
    if (!this->input_) return;
    static_assert(sizeof(this->input_->points[0]) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
    static_assert(sizeof(int) == sizeof(int32_t), "icpgpu: 32-bit int");
    const std::size_t n = this->input_->points.size();
    if (normals_ && normals_->points.size() != n) return;
    if (icpgpu_search_set_input(this->ctx_, n ? reinterpret_cast<const float*>(&this->input_->points[0]) : nullptr, n) != ICPGPU_OK) return;
    std::vector<float> nxyzc(normals_ ? 4 * n : 0);
    for (std::size_t i = 0; i < nxyzc.size() / 4; ++i) {
      nxyzc[4 * i] = normals_->points[i].normal_x;
      nxyzc[4 * i + 1] = normals_->points[i].normal_y;
      nxyzc[4 * i + 2] = normals_->points[i].normal_z;
      nxyzc[4 * i + 3] = 0.f;
    }
    const double angle = angle_ == static_cast<float>(3.14159265358979323846) ? 3.14159265358979323846 : static_cast<double>(angle_);
    std::size_t m = 0;
    if (icpgpu_iss_keypoints_border(this->ctx_, this->salient_, this->non_max_, this->gamma_21_, this->gamma_32_, this->min_neighbors_, this->border_,
                                    angle, nxyzc.empty() ? nullptr : &nxyzc[0], this->normal_radius_, &m) != ICPGPU_OK)
      return;
    std::vector<int32_t> edge(n), border(n);
    if (n && icpgpu_iss_fetch_border(this->ctx_, &edge[0], &border[0]) != ICPGPU_OK) return;
    for (std::size_t i = 0; i < n; ++i) {
      if (edge[i]) edge_->indices.push_back(static_cast<int>(i));
      if (border[i]) border_points_->indices.push_back(static_cast<int>(i));
    }
    if (m == 0) return;
    this->indices_->indices.resize(m);
    output.points.resize(m);
    if (icpgpu_iss_fetch(this->ctx_, m, reinterpret_cast<int32_t*>(&this->indices_->indices[0]), reinterpret_cast<float*>(&output.points[0]), nullptr,
                         nullptr, nullptr, nullptr) != ICPGPU_OK) {
      this->indices_->indices.clear();
      output.points.resize(0);
      return;
    }
    detail::set_cloud_shape(output, m, 0);
  }
  // the last compute()'s boundary points, and the points it skipped for lying within the border radius of one (ascending indices)
  PointIndices::ConstPtr getEdgePoints() const { return edge_; }
  PointIndices::ConstPtr getBorderPoints() const { return border_points_; }

 private:
  const NormalCloudT* normals_ = nullptr;
  float angle_ = 1.57079632679489661923f;  // PCL's default: M_PI / 2
  PointIndices::Ptr edge_, border_points_;
};

// pcl::ModelCoefficients, pcl::SACSegmentation<PointT> and pcl::ExtractIndices<PointT>-shaped front ends (rules and deviations:
// include/icpgpu.h, "plane segmentation") -- the ground removal in front of EuclideanClusterExtraction:
//   pcl::SACSegmentation<pcl::PointXYZ> seg;  ->  icpgpu::SACSegmentation<pcl::PointCloud<pcl::PointXYZ>> seg;
//   seg.setOptimizeCoefficients(true); seg.setModelType(icpgpu::SACMODEL_PLANE); seg.setMethodType(icpgpu::SAC_RANSAC);
//   seg.setMaxIterations(100); seg.setDistanceThreshold(0.2); seg.setInputCloud(cloud); seg.segment(*inliers, *coefficients);
//   pcl::ExtractIndices<pcl::PointXYZ> extract;  ->  icpgpu::ExtractIndices<pcl::PointCloud<pcl::PointXYZ>> extract;
//   extract.setInputCloud(cloud); extract.setIndices(inliers); extract.setNegative(true); extract.filter(*objects);
// The defaults are PCL's (threshold 0, 50 iterations, probability 0.99, optimize true).  No model, or a refused call, leaves the
// inliers and the coefficients empty, as PCL does.  setSeed is ours: the samples come from a counter-based generator.
enum SacModel { SACMODEL_PLANE = 0, SACMODEL_PERPENDICULAR_PLANE = 15 };  // (pcl::SacModel's values)
enum { SAC_RANSAC = 0 };                                                  // (pcl's method_types.h)

struct ModelCoefficients {
  typedef std::shared_ptr<ModelCoefficients> Ptr;
  std::vector<float> values;
};

template <class CloudT>
class SACSegmentation {
 public:
  explicit SACSegmentation(int device = 0) : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx) {}
  template <class CloudPtr>
  void setInputCloud(const CloudPtr& cloud) { input_ = &*cloud; }
  void setModelType(int model) {
    if (model != SACMODEL_PLANE && model != SACMODEL_PERPENDICULAR_PLANE) throw std::invalid_argument("icpgpu::SACSegmentation: plane models only");
    model_ = model;
  }
  int getModelType() const { return model_; }
  void setMethodType(int method) {
    if (method != SAC_RANSAC) throw std::invalid_argument("icpgpu::SACSegmentation: SAC_RANSAC is the only method");
  }
  int getMethodType() const { return SAC_RANSAC; }
  void setDistanceThreshold(double threshold) { threshold_ = threshold; }
  double getDistanceThreshold() const { return threshold_; }
  void setMaxIterations(int max_iterations) { max_iterations_ = max_iterations; }
  int getMaxIterations() const { return max_iterations_; }
  void setProbability(double probability) { probability_ = probability; }
  double getProbability() const { return probability_; }
  void setOptimizeCoefficients(bool optimize) { optimize_ = optimize; }
  bool getOptimizeCoefficients() const { return optimize_; }
  template <class Vec3>
  void setAxis(const Vec3& axis) { axis_[0] = axis[0], axis_[1] = axis[1], axis_[2] = axis[2]; }  // (Eigen::Vector3f, or any [] of three)
  void setEpsAngle(double eps_angle) { eps_angle_ = eps_angle; }
  double getEpsAngle() const { return eps_angle_; }
  void setSeed(uint64_t seed) { seed_ = seed; }  // NOT a PCL method
  int getIterations() const { return iterations_; }   // NOT a PCL method: the iterations of the last segment()
  void segment(PointIndices& inliers, ModelCoefficients& coefficients) {
    inliers.indices.clear();
    coefficients.values.clear();
    iterations_ = 0;
    if (!input_) return;
    static_assert(sizeof(input_->points[0]) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
    static_assert(sizeof(int) == sizeof(int32_t), "icpgpu: 32-bit int");
    const std::size_t n = input_->points.size();
    if (icpgpu_search_set_input(ctx_, n ? reinterpret_cast<const float*>(&input_->points[0]) : nullptr, n) != ICPGPU_OK) return;
    float coeff[4];
    std::size_t n_inliers = 0;
    int32_t iterations = 0, found = 0;
    if (icpgpu_sac_plane_segmentation(ctx_, threshold_, max_iterations_, probability_, seed_, optimize_ ? 1 : 0,
                                      model_ == SACMODEL_PERPENDICULAR_PLANE ? axis_ : nullptr, eps_angle_, coeff, &n_inliers, &iterations,
                                      &found) != ICPGPU_OK)
      return;
    iterations_ = iterations;
    if (!found) return;
    std::vector<int> indices(n_inliers);
    if (icpgpu_sac_fetch(ctx_, n_inliers, 0, n_inliers ? reinterpret_cast<int32_t*>(&indices[0]) : nullptr, nullptr, nullptr, nullptr, nullptr,
                         nullptr, nullptr) != ICPGPU_OK)
      return;
    inliers.indices.swap(indices);
    coefficients.values.assign(coeff, coeff + 4);
  }

 private:
  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  const CloudT* input_ = nullptr;
  int model_ = SACMODEL_PLANE, max_iterations_ = 50, iterations_ = 0;
  double threshold_ = 0.0, probability_ = 0.99, eps_angle_ = 0.0;
  double axis_[3] = {0.0, 0.0, 0.0};
  bool optimize_ = true;
  uint64_t seed_ = 0;
};

// pcl::SACSegmentationFromNormals<PointT, PointNT>-shaped front end (rules and deviations: include/icpgpu.h, "segmentation from
// normals") -- the normal-aware ground plane, then the poles and pipes of what remains:
//   pcl::SACSegmentationFromNormals<pcl::PointXYZ, pcl::Normal> seg;
//     ->  icpgpu::SACSegmentationFromNormals<pcl::PointCloud<pcl::PointXYZ>, pcl::PointCloud<pcl::Normal>> seg;
//   seg.setModelType(icpgpu::SACMODEL_CYLINDER); seg.setMethodType(icpgpu::SAC_RANSAC); seg.setNormalDistanceWeight(0.1);
//   seg.setMaxIterations(10000); seg.setDistanceThreshold(0.05); seg.setRadiusLimits(0, 0.1); seg.setInputCloud(cloud);
//   seg.setInputNormals(normals); seg.segment(*inliers, *coefficients);
// The normals are the input cloud's, one per point (any point type with normal_x, normal_y, normal_z, curvature: NormalEstimation's
// output).  The defaults are PCL's (weight 0.1, limits 0 / 0); an axis of zero length, the default, means none.  The coefficients
// hold 4 (NORMAL_PLANE) or 7 (CYLINDER: point on the axis, direction, radius) values.
enum SacModelFromNormals { SACMODEL_CYLINDER = ICPGPU_SACMODEL_CYLINDER, SACMODEL_NORMAL_PLANE = ICPGPU_SACMODEL_NORMAL_PLANE };

template <class CloudT, class NormalCloudT>
class SACSegmentationFromNormals {
 public:
  explicit SACSegmentationFromNormals(int device = 0) : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx) {}
  template <class CloudPtr>
  void setInputCloud(const CloudPtr& cloud) { input_ = &*cloud; }
  template <class NormalsPtr>
  void setInputNormals(const NormalsPtr& normals) { normals_ = &*normals; }
  void setModelType(int model) {
    if (model != SACMODEL_NORMAL_PLANE && model != SACMODEL_CYLINDER)
      throw std::invalid_argument("icpgpu::SACSegmentationFromNormals: SACMODEL_NORMAL_PLANE or SACMODEL_CYLINDER");
    model_ = model;
  }
  int getModelType() const { return model_; }
  void setMethodType(int method) {
    if (method != SAC_RANSAC) throw std::invalid_argument("icpgpu::SACSegmentationFromNormals: SAC_RANSAC is the only method");
  }
  int getMethodType() const { return SAC_RANSAC; }
  void setDistanceThreshold(double threshold) { threshold_ = threshold; }
  double getDistanceThreshold() const { return threshold_; }
  void setNormalDistanceWeight(double weight) { weight_ = weight; }
  double getNormalDistanceWeight() const { return weight_; }
  void setRadiusLimits(double radius_min, double radius_max) { radius_min_ = radius_min, radius_max_ = radius_max; }
  void getRadiusLimits(double& radius_min, double& radius_max) const { radius_min = radius_min_, radius_max = radius_max_; }
  void setMaxIterations(int max_iterations) { max_iterations_ = max_iterations; }
  int getMaxIterations() const { return max_iterations_; }
  void setProbability(double probability) { probability_ = probability; }
  double getProbability() const { return probability_; }
  void setOptimizeCoefficients(bool optimize) { optimize_ = optimize; }
  bool getOptimizeCoefficients() const { return optimize_; }
  template <class Vec3>
  void setAxis(const Vec3& axis) { axis_[0] = axis[0], axis_[1] = axis[1], axis_[2] = axis[2]; }  // (Eigen::Vector3f, or any [] of three)
  void setEpsAngle(double eps_angle) { eps_angle_ = eps_angle; }
  double getEpsAngle() const { return eps_angle_; }
  void setSeed(uint64_t seed) { seed_ = seed; }  // NOT a PCL method
  int getIterations() const { return iterations_; }   // NOT a PCL method: the iterations of the last segment()
  void segment(PointIndices& inliers, ModelCoefficients& coefficients) {
    inliers.indices.clear();
    coefficients.values.clear();
    iterations_ = 0;
    if (!input_ || !normals_) return;
    static_assert(sizeof(input_->points[0]) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
    static_assert(sizeof(int) == sizeof(int32_t), "icpgpu: 32-bit int");
    const std::size_t n = input_->points.size();
    if (normals_->points.size() != n) return;
    if (icpgpu_search_set_input(ctx_, n ? reinterpret_cast<const float*>(&input_->points[0]) : nullptr, n) != ICPGPU_OK) return;
    std::vector<float> nxyzc(4 * n + 4);
    for (std::size_t i = 0; i < n; ++i) {
      nxyzc[4 * i] = normals_->points[i].normal_x;
      nxyzc[4 * i + 1] = normals_->points[i].normal_y;
      nxyzc[4 * i + 2] = normals_->points[i].normal_z;
      nxyzc[4 * i + 3] = normals_->points[i].curvature;
    }
    const bool axis = model_ == SACMODEL_CYLINDER && (axis_[0] != 0.0 || axis_[1] != 0.0 || axis_[2] != 0.0);
    float coeff[7];
    std::size_t n_inliers = 0;
    int32_t n_coeff = 0, iterations = 0, found = 0;
    if (icpgpu_sac_segmentation_from_normals(ctx_, model_, &nxyzc[0], threshold_, weight_, radius_min_, radius_max_, max_iterations_, probability_, seed_,
                                             optimize_ ? 1 : 0, axis ? axis_ : nullptr, eps_angle_, coeff, &n_coeff, &n_inliers, &iterations,
                                             &found) != ICPGPU_OK)
      return;
    iterations_ = iterations;
    if (!found) return;
    std::vector<int> indices(n_inliers);
    if (icpgpu_sac_normals_fetch(ctx_, n_inliers, 0, n_inliers ? reinterpret_cast<int32_t*>(&indices[0]) : nullptr, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, nullptr, nullptr) != ICPGPU_OK)
      return;
    inliers.indices.swap(indices);
    coefficients.values.assign(coeff, coeff + n_coeff);
  }

 private:
  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  const CloudT* input_ = nullptr;
  const NormalCloudT* normals_ = nullptr;
  int model_ = SACMODEL_NORMAL_PLANE, max_iterations_ = 50, iterations_ = 0;
  double threshold_ = 0.0, weight_ = 0.1, radius_min_ = 0.0, radius_max_ = 0.0, probability_ = 0.99, eps_angle_ = 0.0;
  double axis_[3] = {0.0, 0.0, 0.0};
  bool optimize_ = true;
  uint64_t seed_ = 0;
};

// (a plain host loop over the caller's indices: nothing here needs the device)
template <class CloudT>
class ExtractIndices {
 public:
  template <class CloudPtr>
  void setInputCloud(const CloudPtr& cloud) { input_ = &*cloud; }
  template <class IndicesPtr>
  void setIndices(const IndicesPtr& indices) { indices_ = &indices->indices; }  // (a pointer to pcl::PointIndices, as PCL takes it)
  void setNegative(bool negative) { negative_ = negative; }
  bool getNegative() const { return negative_; }
  void filter(CloudT& output) {
    output.points.resize(0);
    if (input_) {
      const std::size_t n = input_->points.size();
      std::vector<char> in(n, 0);
      if (indices_)
        for (std::size_t k = 0; k < indices_->size(); ++k)
          if ((*indices_)[k] >= 0 && (std::size_t)(*indices_)[k] < n) in[(std::size_t)(*indices_)[k]] = 1;
      for (std::size_t i = 0; i < n; ++i)
        if ((in[i] != 0) != negative_) output.points.push_back(input_->points[i]);
    }
    detail::set_cloud_shape(output, output.points.size(), 0);
  }

 private:
  const CloudT* input_ = nullptr;
  const std::vector<int>* indices_ = nullptr;
  bool negative_ = false;
};

// pcl::ProgressiveMorphologicalFilter<PointXYZ> and pcl::applyMorphologicalOperator-shaped front ends (rules and deviations:
// include/icpgpu.h, "ground filter") -- the ground of a scan whose ground is no plane:
//   pcl::ProgressiveMorphologicalFilter<pcl::PointXYZ> pmf;  ->  icpgpu::ProgressiveMorphologicalFilter<pcl::PointCloud<pcl::PointXYZ>> pmf;
//   pmf.setInputCloud(cloud); pmf.setMaxWindowSize(33); pmf.setSlope(0.7f); pmf.setInitialDistance(0.15f); pmf.setMaxDistance(10.0f);
//   pmf.setCellSize(1.0f); pmf.setBase(2.0f); pmf.setExponential(true); pmf.extract(ground->indices);
//   pcl::applyMorphologicalOperator<pcl::PointXYZ>(cloud, resolution, pcl::MORPH_OPEN, out)  ->  icpgpu::applyMorphologicalOperator(...)
// The defaults are PCL's.  A refused call leaves the ground empty (and the output cloud of the operator empty).  Non-finite points are
// never ground (PCL keeps their indices).  setIndices is not provided.
enum MorphologicalOperators { MORPH_OPEN, MORPH_CLOSE, MORPH_DILATE, MORPH_ERODE };  // (pcl's order, not icpgpu_morph_op's)

template <class CloudT>
class ProgressiveMorphologicalFilter {
 public:
  explicit ProgressiveMorphologicalFilter(int device = 0) : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx) {}
  template <class CloudPtr>
  void setInputCloud(const CloudPtr& cloud) { input_ = &*cloud; }
  void setMaxWindowSize(int max_window_size) { max_window_size_ = max_window_size; }
  int getMaxWindowSize() const { return max_window_size_; }
  void setSlope(float slope) { slope_ = slope; }
  float getSlope() const { return slope_; }
  void setMaxDistance(float max_distance) { max_distance_ = max_distance; }
  float getMaxDistance() const { return max_distance_; }
  void setInitialDistance(float initial_distance) { initial_distance_ = initial_distance; }
  float getInitialDistance() const { return initial_distance_; }
  void setCellSize(float cell_size) { cell_size_ = cell_size; }
  float getCellSize() const { return cell_size_; }
  void setBase(float base) { base_ = base; }
  float getBase() const { return base_; }
  void setExponential(bool exponential) { exponential_ = exponential; }
  bool getExponential() const { return exponential_; }
  int getPasses() const { return passes_; }  // NOT a PCL method: the schedule's length at the last extract()
  void extract(std::vector<int>& ground) {
    ground.clear();
    passes_ = 0;
    if (!input_) return;
    static_assert(sizeof(input_->points[0]) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
    static_assert(sizeof(int) == sizeof(int32_t), "icpgpu: 32-bit int");
    const std::size_t n = input_->points.size();
    if (icpgpu_search_set_input(ctx_, n ? reinterpret_cast<const float*>(&input_->points[0]) : nullptr, n) != ICPGPU_OK) return;
    std::size_t n_ground = 0;
    int32_t n_passes = 0;
    if (icpgpu_progressive_morphological_filter(ctx_, max_window_size_, slope_, initial_distance_, max_distance_, cell_size_, base_,
                                                exponential_ ? 1 : 0, &n_ground, &n_passes) != ICPGPU_OK)
      return;
    std::vector<int> indices(n_ground);
    if (icpgpu_pmf_fetch(ctx_, n_ground, (std::size_t)n_passes, n_ground ? reinterpret_cast<int32_t*>(&indices[0]) : nullptr, nullptr, nullptr,
                         nullptr, nullptr) != ICPGPU_OK)
      return;
    passes_ = n_passes;
    ground.swap(indices);
  }

 private:
  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  const CloudT* input_ = nullptr;
  int max_window_size_ = 33, passes_ = 0;
  float slope_ = 0.7f, max_distance_ = 10.0f, initial_distance_ = 0.15f, cell_size_ = 1.0f, base_ = 2.0f;
  bool exponential_ = true;
};

// cloud_out = cloud_in with every finite point's z replaced by the operator's (non-finite points keep theirs)
template <class CloudPtr, class CloudT>
void applyMorphologicalOperator(const CloudPtr& cloud_in, float resolution, int morphological_operator, CloudT& cloud_out, int device = 0) {
  cloud_out.points.resize(0);
  const int op = morphological_operator == MORPH_OPEN    ? ICPGPU_MORPH_OPEN
                 : morphological_operator == MORPH_CLOSE  ? ICPGPU_MORPH_CLOSE
                 : morphological_operator == MORPH_DILATE ? ICPGPU_MORPH_DILATE
                 : morphological_operator == MORPH_ERODE  ? ICPGPU_MORPH_ERODE
                                                          : -1;
  const std::size_t n = cloud_in->points.size();
  static_assert(sizeof(cloud_in->points[0]) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
  detail::ContextPtr holder = detail::acquire_context(device);
  std::vector<float> z(n);
  float none = 0.f;  // (an empty cloud still hands over a valid pointer)
  if (icpgpu_search_set_input(holder->ctx, n ? reinterpret_cast<const float*>(&cloud_in->points[0]) : nullptr, n) == ICPGPU_OK &&
      icpgpu_morphological_operator(holder->ctx, resolution, op, n ? &z[0] : &none) == ICPGPU_OK) {
    cloud_out.points = cloud_in->points;
    for (std::size_t i = 0; i < n; ++i) cloud_out.points[i].z = z[i];
  }
  detail::set_cloud_shape(cloud_out, cloud_out.points.size(), 0);
}

// pcl::KdTreeFLANN<pcl::FPFHSignature33> and pcl::SampleConsensusPrerejective<PointSource, PointTarget, FeatureT>-shaped front ends
// (rules and deviations: include/icpgpu.h, "feature-space k-nearest" and "sample-consensus alignment") -- the pose of a cloud in
// another WITHOUT a guess, the end of the chain VoxelGrid -> NormalEstimation -> FPFHEstimation and the start ICP needs:
//   pcl::KdTreeFLANN<pcl::FPFHSignature33> tree;  ->  icpgpu::FeatureKdTree<pcl::PointCloud<pcl::FPFHSignature33>> tree;
//   tree.setInputCloud(features); tree.nearestKSearch(features->points[i], k, indices, sqr_distances);
//   pcl::SampleConsensusPrerejective<pcl::PointXYZ, pcl::PointXYZ, pcl::FPFHSignature33> align;
//     ->  icpgpu::SampleConsensusPrerejective<pcl::PointCloud<pcl::PointXYZ>, pcl::PointCloud<pcl::FPFHSignature33>> align;
//   align.setInputSource(object); align.setSourceFeatures(object_features); align.setInputTarget(scene);
//   align.setTargetFeatures(scene_features); align.setMaximumIterations(50000); align.setNumberOfSamples(3);
//   align.setCorrespondenceRandomness(5); align.setSimilarityThreshold(0.9f); align.setMaxCorrespondenceDistance(0.5);
//   align.setInlierFraction(0.25f); align.align(aligned); align.hasConverged(); align.getFinalTransformation(); align.getInliers();
// (the shim's KdTreeFLANN is an alias over POINT clouds, which cannot be specialised for a feature type: the feature tree is a named
// class.)  The feature point type only needs float histogram[33].  The defaults are PCL's (3 samples, randomness 2, similarity 0.9,
// inlier fraction 0) except the two PCL inherits from Registration: 1000 iterations instead of 10, and a correspondence distance of
// 1 m instead of sqrt(DBL_MAX), whose square is not a float.  A refused call leaves the output empty and hasConverged() false.
// setSeed is ours: the samples come from a counter-based generator.  A guess is not provided.
template <class FeatureCloudT>
class FeatureKdTree {
 public:
  typedef std::shared_ptr<FeatureKdTree> Ptr;
  typedef std::shared_ptr<const FeatureKdTree> ConstPtr;
  explicit FeatureKdTree(int device = 0) : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx) {}
  template <class CloudPtr>
  void setInputCloud(const CloudPtr& features) {
    input_ = &*features;
    static_assert(sizeof(input_->points[0]) == ICPGPU_FPFH_BINS * sizeof(float), "icpgpu: float histogram[33] and nothing else (pcl::FPFHSignature33)");
  }
  template <class FeatureT>
  int nearestKSearch(const FeatureT& feature, int k, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances) {
    static_assert(sizeof(feature.histogram) == ICPGPU_FPFH_BINS * sizeof(float), "icpgpu: float histogram[33] (pcl::FPFHSignature33)");
    return knn(feature.histogram, 1, k, k_indices, k_sqr_distances, nullptr) ? (int)k_indices.size() : 0;
  }
  int nearestKSearch(int index, int k, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances) {
    if (!input_ || index < 0 || (std::size_t)index >= input_->points.size()) return (k_indices.clear(), k_sqr_distances.clear(), 0);
    return nearestKSearch(input_->points[index], k, k_indices, k_sqr_distances);
  }
  // Batched form (not PCL's): every row of `queries` in one call.  Row i of k_indices / k_sqr_distances has k entries, the first
  // n_found[i] of them neighbours (the rest -1 / +inf); returns the number of queries answered.
  int nearestKSearch(const FeatureCloudT& queries, int k, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances, std::vector<int>& n_found) {
    const std::size_t nq = queries.points.size();
    n_found.assign(nq, 0);
    if (nq == 0) return (k_indices.clear(), k_sqr_distances.clear(), 0);
    return knn(queries.points[0].histogram, nq, k, k_indices, k_sqr_distances, &n_found) ? (int)nq : 0;
  }

 private:
  bool knn(const float* rows, std::size_t nq, int k, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances, std::vector<int>* n_found) {
    static_assert(sizeof(int) == sizeof(int32_t), "icpgpu: 32-bit int");
    k_indices.clear(), k_sqr_distances.clear();
    if (!input_ || k <= 0) return false;
    const std::size_t n = input_->points.size();
    k_indices.assign(nq * (std::size_t)k, -1), k_sqr_distances.resize(nq * (std::size_t)k);
    int32_t found = 0;
    const int rc = icpgpu_feature_knn(ctx_, n ? input_->points[0].histogram : nullptr, n, rows, nq, k, reinterpret_cast<int32_t*>(&k_indices[0]),
                                      &k_sqr_distances[0], n_found ? reinterpret_cast<int32_t*>(&(*n_found)[0]) : &found);
    if (rc != ICPGPU_OK) {
      k_indices.clear(), k_sqr_distances.clear();
      return false;
    }
    if (!n_found) k_indices.resize((std::size_t)found), k_sqr_distances.resize((std::size_t)found);  // (PCL returns a short list too)
    return true;
  }
  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  const FeatureCloudT* input_ = nullptr;
};

template <class CloudT, class FeatureCloudT>
class SampleConsensusPrerejective {
 public:
  explicit SampleConsensusPrerejective(int device = 0) : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx) {
    const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(T_, eye, sizeof T_);
  }
  template <class CloudPtr>
  void setInputSource(const CloudPtr& cloud) { source_ = &*cloud; }
  template <class CloudPtr>
  void setInputTarget(const CloudPtr& cloud) { target_ = &*cloud; }
  template <class FeaturesPtr>
  void setSourceFeatures(const FeaturesPtr& features) { source_features_ = &*features; }
  template <class FeaturesPtr>
  void setTargetFeatures(const FeaturesPtr& features) { target_features_ = &*features; }
  void setNumberOfSamples(int nr_samples) { nr_samples_ = nr_samples; }
  int getNumberOfSamples() const { return nr_samples_; }
  void setCorrespondenceRandomness(int k) { k_correspondences_ = k; }
  int getCorrespondenceRandomness() const { return k_correspondences_; }
  void setSimilarityThreshold(float similarity_threshold) { similarity_ = similarity_threshold; }
  float getSimilarityThreshold() const { return similarity_; }
  void setMaxCorrespondenceDistance(double distance) { distance_ = distance; }
  double getMaxCorrespondenceDistance() const { return distance_; }
  void setInlierFraction(float inlier_fraction) { inlier_fraction_ = inlier_fraction; }
  float getInlierFraction() const { return inlier_fraction_; }
  void setMaximumIterations(int max_iterations) { max_iterations_ = max_iterations; }
  int getMaximumIterations() const { return max_iterations_; }
  void setSeed(uint64_t seed) { seed_ = seed; }  // NOT a PCL method
  void align(CloudT& output) {
    const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(T_, eye, sizeof T_);
    converged_ = false;
    fitness_ = FLT_MAX;
    inliers_.clear();
    output.points.resize(0);
    detail::set_cloud_shape(output, 0, 0);
    if (!source_ || !target_ || !source_features_ || !target_features_) return;
    static_assert(sizeof(source_->points[0]) == 16, "icpgpu: 16-byte points (pcl::PointXYZ)");
    static_assert(sizeof(source_features_->points[0]) == ICPGPU_FPFH_BINS * sizeof(float), "icpgpu: float histogram[33] and nothing else (pcl::FPFHSignature33)");
    static_assert(sizeof(int) == sizeof(int32_t), "icpgpu: 32-bit int");
    const std::size_t ns = source_->points.size(), n = target_->points.size();
    if (source_features_->points.size() != ns || target_features_->points.size() != n) return;  // (PCL refuses features that do not match as well)
    if (icpgpu_search_set_input(ctx_, n ? reinterpret_cast<const float*>(&target_->points[0]) : nullptr, n) != ICPGPU_OK) return;
    output.points.resize(ns);
    std::size_t n_inliers = 0;
    int32_t converged = 0;
    if (icpgpu_scp_align(ctx_, ns ? reinterpret_cast<const float*>(&source_->points[0]) : nullptr, ns, ns ? source_features_->points[0].histogram : nullptr,
                         n ? target_features_->points[0].histogram : nullptr, nr_samples_, k_correspondences_, (double)similarity_, distance_,
                         (double)inlier_fraction_, max_iterations_, seed_, T_, &n_inliers, &fitness_, &converged,
                         ns ? reinterpret_cast<float*>(&output.points[0]) : nullptr) != ICPGPU_OK) {
      output.points.resize(0);
      return;
    }
    detail::set_cloud_shape(output, ns, 0);
    std::vector<int> inliers(n_inliers);
    if (n_inliers && icpgpu_scp_fetch(ctx_, 0, n_inliers, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                      reinterpret_cast<int32_t*>(&inliers[0])) != ICPGPU_OK)
      return;
    inliers_.swap(inliers);
    converged_ = converged != 0;
  }
  bool hasConverged() const { return converged_; }
  Matrix4 getFinalTransformation() const { return make_matrix4(T_); }
  const std::vector<int>& getInliers() const { return inliers_; }
  double getFitnessScore() const { return (double)fitness_; }  // the inliers' mean squared distance (FLT_MAX without a pose)

 private:
  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  const CloudT *source_ = nullptr, *target_ = nullptr;
  const FeatureCloudT *source_features_ = nullptr, *target_features_ = nullptr;
  int nr_samples_ = 3, k_correspondences_ = 2, max_iterations_ = 1000;
  float similarity_ = 0.9f, inlier_fraction_ = 0.0f, fitness_ = FLT_MAX;
  double distance_ = 1.0;
  uint64_t seed_ = 0;
  bool converged_ = false;
  float T_[16];
  std::vector<int> inliers_;
};

// The mapper's map (/root/reference/src/icpslam/octree_mapper.cpp:55-90): replaces the pair
//   pcl::octree::OctreePointCloudSearch<pcl::PointXYZ>::Ptr map_octree_;  pcl::PointCloud<pcl::PointXYZ>::Ptr map_cloud_;
// Poses are the float 4x4 that pcl_ros::transformPointCloud applies (icpgpu_pose_to_matrix gives it for a Pose6DOF);
// the transform of transformCloudToPoseFrame is fused into both calls, so the mapper passes the scan in the robot frame.
template <class CloudT>
class OctreeMap {
 public:
  explicit OctreeMap(double resolution, int device = 0)
      : ctx_holder_(detail::acquire_context(device)), ctx_(ctx_holder_->ctx), resolution_(resolution) { resetMap(); }
  const detail::ContextPtr& context() const { return ctx_holder_; }  // for IterativeClosestPoint::setInputTargetFromMap(map.context())
  // :55-59.  The context comes from the pool and may have served another map before: the search mode is THIS object's
  // (exact unless setPclApproximateSearch(true) was called on it), re-applied with every reset.
  void resetMap() {
    icpgpu_map_reset(ctx_, resolution_);
    icpgpu_map_set_search(ctx_, pcl_approx_ ? ICPGPU_MAP_SEARCH_PCL_APPROX : ICPGPU_MAP_SEARCH_EXACT);
  }
  // which neighbour approxNearestNeighbors collects: false (default) = the EXACT nearest map point; true = a restatement of
  // PCL's approxNearestSearch heuristic (icpgpu.h: icpgpu_map_set_search; unpinned against a PCL build like the rest)
  void setPclApproximateSearch(bool on) {
    pcl_approx_ = on;
    icpgpu_map_set_search(ctx_, on ? ICPGPU_MAP_SEARCH_PCL_APPROX : ICPGPU_MAP_SEARCH_EXACT);
  }
  std::size_t addPointsToMap(const CloudT& cloud, const Matrix4& pose) {                         // :62-69 (+ :135, :152)
    std::size_t added = 0;
    const std::size_t n = cloud.points.size();
    icpgpu_map_add_points(ctx_, n ? reinterpret_cast<const float*>(&cloud.points[0]) : nullptr, n, pose.data(), &added);
    return added;
  }
  // :72-90 followed by the transform back at :146.  nearest_neighbors receives the nn cloud; it also stays in HBM as
  // the registration target (IterativeClosestPoint::setInputTargetFromMap).  Exact nearest neighbours unless
  // setPclApproximateSearch(true).
  bool approxNearestNeighbors(const CloudT& cloud, const Matrix4& pose, const Matrix4& pose_inv, CloudT& nearest_neighbors) {
    const std::size_t n = cloud.points.size();
    nearest_neighbors.points.resize(n);
    std::size_t m = 0;
    if (icpgpu_set_source(ctx_, n ? reinterpret_cast<const float*>(&cloud.points[0]) : nullptr, n) != ICPGPU_OK ||
        icpgpu_map_nn_target(ctx_, pose.data(), pose_inv.data(), n ? reinterpret_cast<float*>(&nearest_neighbors.points[0]) : nullptr,
                             &m) != ICPGPU_OK)
      m = 0;
    nearest_neighbors.points.resize(m);
    detail::set_cloud_shape(nearest_neighbors, m, 0);
    ++ctx_holder_->generation;  // the context's source / target are the map's now
    detail::last_map_context() = ctx_holder_;
    return m > 0;
  }
  std::size_t size() const {
    std::size_t n = 0;
    icpgpu_map_size(ctx_, &n);
    return n;
  }
  void getMapCloud(CloudT& out) const {  // map_cloud_ for the publisher at :155
    std::size_t n = size(), m = 0;
    out.points.resize(n);
    if (icpgpu_map_get_points(ctx_, n ? reinterpret_cast<float*>(&out.points[0]) : nullptr, n, &m) != ICPGPU_OK) out.points.resize(0);
    detail::set_cloud_shape(out, out.points.size(), 0);
  }

 private:
  detail::ContextPtr ctx_holder_;
  icpgpu_ctx* ctx_;
  double resolution_;
  bool pcl_approx_ = false;
};

}  // namespace icpgpu
