// icpgpu_region.cpp -- host side of region growing over the search cloud (pcl::RegionGrowing by an order-free rule; rules:
// include/icpgpu.h "region growing"; kernels: icp_region.hip, whose tail is clustering's, icp_cluster.hip).  The k-nearest rows never
// leave the device: knn_rows_on_device queues them into the search state's buffers without a wait and region_hook_kernel reads them
// there, on the same stream.  Everything the call keeps -- the caller's normals included -- lives in the region state's own buffers:
// a later search, normal, clustering, segmentation, ground filter, ISS or moving least squares call never meets it, nor it theirs.
// One wait (deliver): the two counts.
#include "icp_ctx.h"

extern "C" {

int icpgpu_region_growing(icpgpu_ctx* c, const float* normals_nxyzc, int k, float smoothness_cos, float curvature_threshold, int min_size,
                          int max_size, size_t* n_regions, size_t* n_in_regions) {
  ENTER(c);
  auto& S = c->search;
  auto& R = c->region;
  R.have = false;
  R.waits = 0;
  if (n_regions) *n_regions = 0;
  if (n_in_regions) *n_in_regions = 0;
  if (!S.set) return fail(c, ICPGPU_ERR_INVALID_ARG, "region_growing: no search cloud (icpgpu_search_set_input)");
  const size_t n = S.n;
  if (n && !normals_nxyzc) return fail(c, ICPGPU_ERR_INVALID_ARG, "region_growing: null normals for a search cloud of %zu points", n);
  if (k < 1 || k > ICPGPU_SEARCH_MAX_K) return fail(c, ICPGPU_ERR_INVALID_ARG, "region_growing: k %d outside 1..%d", k, ICPGPU_SEARCH_MAX_K);
  if (std::isnan(smoothness_cos) || std::isnan(curvature_threshold))
    return fail(c, ICPGPU_ERR_INVALID_ARG, "region_growing: smoothness_cos and curvature_threshold must not be NaN");
  if (!n_regions || !n_in_regions) return fail(c, ICPGPU_ERR_INVALID_ARG, "region_growing: null n_regions or n_in_regions");
  const size_t ints = std::max<size_t>(n, 1) * sizeof(int);
  int rc;
  if ((rc = ensure(c, R.normals, std::max<size_t>(n, 1) * sizeof(float4)))) return rc;
  if ((rc = ensure(c, R.border_key, std::max<size_t>(n, 1) * sizeof(unsigned long long)))) return rc;
  for (DeviceBuf* b : {&R.kind, &R.anchor, &R.parent, &R.sizes, &R.region, &R.labels, &R.rank_of})
    if ((rc = ensure(c, *b, ints))) return rc;
  for (DeviceBuf* b : {&R.csize, &R.cstart})
    if ((rc = ensure(c, *b, (n + 1) * sizeof(int)))) return rc;
  for (DeviceBuf* b : {&R.keys, &R.vals})
    if ((rc = ensure(c, *b, 2 * ints))) return rc;
  if ((rc = ensure(c, R.cstart64, (n + 1) * sizeof(long long)))) return rc;
  if ((rc = ensure(c, R.scratch, cluster_scratch_ints((int)n) * sizeof(int)))) return rc;
  if ((rc = ensure(c, R.counts, 2 * sizeof(int)))) return rc;
  if (n) HIP_TRY(c, hipMemcpyAsync(R.normals.ptr, normals_nxyzc, n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
  const SearchView v = view_of(c);
  const bool any_finite = v.n_eval > 0;
  if (any_finite && (rc = knn_rows_on_device(c, v.cloud, n, k))) return rc;  // (a cloud the grid refuses: the search's own whole-cloud kernel)
  HIP_TRY(c, launch_region_growing(v.cloud, R.normals.as<const float4>(), v.n, any_finite, S.idx.as<const int32_t>(), S.d2.as<const float>(),
                                   S.n_found.as<const int32_t>(), k, smoothness_cos, curvature_threshold, min_size, max_size, R.kind.as<int>(),
                                   R.border_key.as<unsigned long long>(), R.anchor.as<int>(), R.parent.as<int>(), R.sizes.as<int>(),
                                   R.region.as<int>(), R.labels.as<int>(), R.rank_of.as<int>(), R.csize.as<int>(), R.cstart.as<int>(),
                                   R.cstart64.as<long long>(), R.keys.as<int>(), R.vals.as<int>(), R.scratch.as<int>(), R.counts.as<int>(),
                                   c->stream));
  int counts[2] = {0, 0};
  const Delivery out[1] = {{counts, R.counts.ptr, sizeof counts}};
  if ((rc = deliver(c, out, 1))) return rc;
  R.waits = 1;
  R.n = n;
  R.n_regions = (size_t)counts[0];
  R.n_in_regions = (size_t)counts[1];
  R.have = true;
  *n_regions = R.n_regions;
  *n_in_regions = R.n_in_regions;
  if (std::getenv("ICPGPU_DEBUG"))
    fprintf(stderr, "[icpgpu] region n=%zu k=%d regions=%zu in_regions=%zu waits=%d\n", n, k, R.n_regions, R.n_in_regions, R.waits);
  return ICPGPU_OK;
}

int icpgpu_region_fetch(icpgpu_ctx* c, size_t capacity_regions, size_t capacity_indices, int64_t* region_start, int32_t* indices, int32_t* labels,
                        int32_t* region, int32_t* kind, int32_t* anchor) {
  ENTER(c);
  const auto& R = c->region;
  if (!R.have) return fail(c, ICPGPU_ERR_INVALID_ARG, "region_fetch: no result (icpgpu_region_growing)");
  if (!region_start) return fail(c, ICPGPU_ERR_INVALID_ARG, "region_fetch: null region_start");
  if (R.n_regions > capacity_regions || R.n_in_regions > capacity_indices || (R.n_in_regions && !indices))
    return fail(c, ICPGPU_ERR_INVALID_ARG, "region_fetch: %zu regions of %zu points, room for %zu and %zu", R.n_regions, R.n_in_regions,
                capacity_regions, indices ? capacity_indices : (size_t)0);
  const size_t per_point = R.n * sizeof(int32_t);
  const Delivery out[6] = {{region_start, R.cstart64.ptr, (R.n_regions + 1) * sizeof(int64_t)},
                           {indices, R.vals.as<const int>() + R.n, R.n_in_regions * sizeof(int32_t)},
                           {labels, R.labels.ptr, labels ? per_point : 0},
                           {region, R.region.ptr, region ? per_point : 0},
                           {kind, R.kind.ptr, kind ? per_point : 0},
                           {anchor, R.anchor.ptr, anchor ? per_point : 0}};
  return deliver(c, out, 6);
}

}  // extern "C"
