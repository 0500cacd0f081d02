// icpgpu_segment.cpp -- host side of the segment moments over the search cloud (pcl::MomentOfInertiaEstimation and the per-cluster
// centroid / box / covariance calls, for every segment of a segmentation at once; rules: include/icpgpu.h "segment moments"; kernels:
// icp_segment.hip).  A HOST source's CSR is validated here in one loop over its entries and copied into buffers of the call's own; a
// CLUSTERS / REGIONS source is read where the clustering or region growing call left it -- cstart and the second half of vals of
// c->cluster / c->region -- and nothing of it is written.  Every launch is sized by what the host knows: the number of segments and
// of listed entries.  The call keeps nothing.  One wait (deliver): the records.
#include "icp_ctx.h"

extern "C" {

int icpgpu_segment_moments(icpgpu_ctx* c, int source, size_t n_segments, const int64_t* segment_start, const int32_t* indices, size_t sizeof_record,
                           icpgpu_segment_record* out) {
  ENTER(c);
  auto& S = c->search;
  auto& G = c->segment;
  G.waits = 0;
  if (!S.set) return fail(c, ICPGPU_ERR_INVALID_ARG, "segment_moments: no search cloud (icpgpu_search_set_input)");
  if (sizeof_record != sizeof(icpgpu_segment_record))
    return fail(c, ICPGPU_ERR_INVALID_ARG, "segment_moments: sizeof_record %zu, no 1.x header has a record of that size (%zu)", sizeof_record,
                sizeof(icpgpu_segment_record));
  if (n_segments && !out) return fail(c, ICPGPU_ERR_INVALID_ARG, "segment_moments: null out for %zu segments", n_segments);
  const size_t n = S.n;
  size_t total = 0;
  const int* d_start = nullptr;
  const int* d_list = nullptr;
  std::vector<int> start32;
  if (source == ICPGPU_SEGMENTS_HOST) {
    if (!segment_start) return fail(c, ICPGPU_ERR_INVALID_ARG, "segment_moments: null segment_start");
    if (segment_start[0] != 0) return fail(c, ICPGPU_ERR_INVALID_ARG, "segment_moments: segment_start[0] is %lld, not 0", (long long)segment_start[0]);
    for (size_t r = 0; r < n_segments; ++r)
      if (segment_start[r + 1] < segment_start[r])
        return fail(c, ICPGPU_ERR_INVALID_ARG, "segment_moments: segment_start decreases at segment %zu", r);
    total = (size_t)segment_start[n_segments];
    if (total && !indices) return fail(c, ICPGPU_ERR_INVALID_ARG, "segment_moments: null indices for %zu listed entries", total);
    for (size_t e = 0; e < total; ++e)
      if (indices[e] < 0 || (size_t)indices[e] >= n)
        return fail(c, ICPGPU_ERR_INVALID_ARG, "segment_moments: index %d at entry %zu outside the search cloud's %zu points", indices[e], e, n);
  } else if (source == ICPGPU_SEGMENTS_CLUSTERS || source == ICPGPU_SEGMENTS_REGIONS) {
    const bool clusters = source == ICPGPU_SEGMENTS_CLUSTERS;
    const char* what = clusters ? "clustering" : "region growing";
    const bool have = clusters ? c->cluster.have : c->region.have;
    if (!have) return fail(c, ICPGPU_ERR_INVALID_ARG, "segment_moments: no %s result over this search cloud", what);
    if (segment_start || indices) return fail(c, ICPGPU_ERR_INVALID_ARG, "segment_moments: segment_start and indices must be NULL for a %s source", what);
    const size_t have_segments = clusters ? c->cluster.n_clusters : c->region.n_regions;
    if (n_segments != have_segments)
      return fail(c, ICPGPU_ERR_INVALID_ARG, "segment_moments: n_segments %zu, the %s result has %zu", n_segments, what, have_segments);
    total = clusters ? c->cluster.n_clustered : c->region.n_in_regions;
    const size_t n_of = clusters ? c->cluster.n : c->region.n;
    d_start = clusters ? c->cluster.cstart.as<const int>() : c->region.cstart.as<const int>();
    d_list = (clusters ? c->cluster.vals.as<const int>() : c->region.vals.as<const int>()) + n_of;
  } else {
    return fail(c, ICPGPU_ERR_INVALID_ARG, "segment_moments: unknown source %d", source);
  }
  if (n_segments == 0) return ICPGPU_OK;
  if (n_segments > (size_t)INT32_MAX || total > (size_t)INT32_MAX)
    return fail(c, ICPGPU_ERR_UNSUPPORTED, "segment_moments: %zu segments of %zu entries, more than 2^31 - 1", n_segments, total);
  const size_t slots = icpgpu::segment_partials(n_segments, total);
  int rc;
  if ((rc = ensure(c, G.first, n_segments * sizeof(unsigned int)))) return rc;
  if ((rc = ensure(c, G.seg_of, std::max<size_t>(total, 1) * sizeof(int)))) return rc;
  if ((rc = ensure(c, G.partials, slots * sizeof(icpgpu::SegmentPartial)))) return rc;
  if ((rc = ensure(c, G.box_partials, slots * sizeof(icpgpu::SegmentBoxPartial)))) return rc;
  if ((rc = ensure(c, G.records, n_segments * sizeof(icpgpu_segment_record)))) return rc;
  if (source == ICPGPU_SEGMENTS_HOST) {
    if ((rc = ensure(c, G.start, (n_segments + 1) * sizeof(int)))) return rc;
    if ((rc = ensure(c, G.list, std::max<size_t>(total, 1) * sizeof(int)))) return rc;
    start32.resize(n_segments + 1);
    for (size_t r = 0; r <= n_segments; ++r) start32[r] = (int)segment_start[r];
    HIP_TRY(c, hipMemcpyAsync(G.start.ptr, start32.data(), start32.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (total) HIP_TRY(c, hipMemcpyAsync(G.list.ptr, indices, total * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    d_start = G.start.as<const int>();
    d_list = G.list.as<const int>();
  }
  const SearchView v = view_of(c);
  HIP_TRY(c, launch_segment_moments(v.cloud, v.n, d_start, d_list, (int)n_segments, (int)total, G.seg_of.as<int>(), G.first.as<unsigned int>(),
                                    G.partials.as<icpgpu::SegmentPartial>(), G.box_partials.as<icpgpu::SegmentBoxPartial>(), G.records.ptr, c->stream));
  const Delivery parts[1] = {{out, G.records.ptr, n_segments * sizeof(icpgpu_segment_record)}};
  if ((rc = deliver(c, parts, 1))) return rc;
  G.waits = 1;
  if (std::getenv("ICPGPU_DEBUG"))
    fprintf(stderr, "[icpgpu] segment source=%d segments=%zu entries=%zu chunks=%zu waits=%d\n", source, n_segments, total,
            icpgpu::segment_chunks(total), G.waits);
  return ICPGPU_OK;
}

int icpgpu_segment_stats(const icpgpu_ctx* c, int32_t* host_waits) {
  if (!c) return ICPGPU_ERR_INVALID_ARG;
  if (host_waits) *host_waits = c->segment.waits;
  return ICPGPU_OK;
}

}  // extern "C"
