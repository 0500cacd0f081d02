"""An independent NumPy restatement of region growing (include/icpgpu.h, "region growing"), built on the neighbour search's
restatement (tests/search_restated.py: knn) and float32 NumPy.  It never calls the library.

    participant  a finite point whose four normal floats are finite; the others: kind = region = label = -1
    row(i)       search_restated.knn(cloud, None, k)'s row of point i
    smooth(i,j)  fabs((nx_i nx_j + ny_i ny_j) + nz_i nz_j) >= smoothness_cos, float32, every product and sum rounded on its own
    core         a participant with not (curvature > curvature_threshold)                              kind 2
    core graph   cores i != j joined iff smooth(i, j) and (j in row(i) or i in row(j)); a region's cores are a connected
                 component, its name the lowest core index
    border       a non-core participant j listed by a core i with smooth(i, j): it takes the core with the smallest key
                 (bits of row(i)'s d2 for j) << 32 | i and joins that core's region; anchor[j] = i       kind 1
    single       a non-core participant no core claims: a region of its own, named by its index           kind 0
    emission     clustering's (tests/cluster_restated.py: from_components)

Three functions beside each other: grow, the rule vectorised; grow_literal, the same rule as a per-point, per-neighbour Python loop;
pcl_literal, PCL 1.8's applySmoothRegionGrowingAlgorithm / growRegion / validatePoint transcribed (smooth mode on, curvature test
on, residual test off) over the same rows and with the same smooth(), in PCL's own order.
"""
from __future__ import annotations

import math

import numpy as np

import cluster_restated as CR
import search_restated as S

F32 = np.float32
INT_MAX = 2**31 - 1
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
NAMES = ("region_start", "indices", "labels", "region", "kind", "anchor")


class Refused(ValueError):
    """The library answers ICPGPU_ERR_INVALID_ARG."""


def smoothness_cos(theta: float) -> np.float32:
    """What the shims hand the library for PCL's theta (radians): (float)cos((double)theta)."""
    return F32(math.cos(float(theta)))


def _inputs(cloud, normals, k, cos, threshold):
    cloud = np.asarray(cloud, F32).reshape(-1, 4)
    n = cloud.shape[0]
    if normals is None:
        if n:
            raise Refused("null normals")
        normals = np.zeros((0, 4), F32)
    normals = np.asarray(normals, F32).reshape(-1, 4)
    if normals.shape[0] != n:
        raise ValueError("one normal per point")
    if not 1 <= k <= S.SEARCH_MAX_K:
        raise Refused(f"k {k}")
    cos, threshold = F32(cos), F32(threshold)          # (the C-ABI takes floats)
    if np.isnan(cos) or np.isnan(threshold):
        raise Refused("NaN")
    return cloud, normals, cos, threshold


def participants(cloud, normals) -> np.ndarray:
    return S.finite_mask(cloud) & np.isfinite(normals).all(axis=1)


def rows_of(cloud, k):
    """(idx (n, k) int32, d2 (n, k) float32, n_found (n,)): every point's k-nearest row over the cloud itself."""
    if cloud.shape[0] == 0:
        return np.zeros((0, k), np.int32), np.zeros((0, k), F32), np.zeros(0, np.int32)
    return S.knn(cloud, None, k)


def smooth_pairs(normals, i, j, cos):
    """smooth(i, j) element by element (i, j: index arrays of one shape)."""
    a, b = normals[i], normals[j]
    with np.errstate(invalid="ignore", over="ignore"):
        dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
        return np.abs(dot) >= cos


def partition(cloud, normals, k: int, cos, threshold, rows=None):
    """(region, kind, anchor), (n,) int32 each: the rule, vectorised.  rows: what rows_of(cloud, k) returned, when the caller has it."""
    cloud, normals, cos, threshold = _inputs(cloud, normals, k, cos, threshold)
    n = cloud.shape[0]
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    idx, d2, _ = rows if rows is not None else rows_of(cloud, k)
    part = participants(cloud, normals)
    with np.errstate(invalid="ignore"):
        core = part & ~(normals[:, 3] > threshold)
    owner = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], idx.shape)
    listed = (idx >= 0) & (idx != owner) & core[owner]
    i, j, dd = owner[listed], idx[listed].astype(np.int64), d2[listed]
    ok = part[j] & smooth_pairs(normals, i, j, cos)
    i, j, dd = i[ok], j[ok], dd[ok]
    # the core graph's components, named by their lowest index
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    e = core[j]
    _, comp = connected_components(coo_matrix((np.ones(int(e.sum()), np.int8), (i[e], j[e])), shape=(n, n)), directed=False)
    lowest = np.full(n, n, np.int64)
    np.minimum.at(lowest, comp, np.arange(n))
    region = np.where(core, lowest[comp], -1).astype(np.int64)
    # the borders: the smallest key among the cores that list them
    key = np.full(n, NO_KEY, np.uint64)
    b = ~e
    np.minimum.at(key, j[b], (S._bits(dd[b]).astype(np.uint64) << np.uint64(32)) | i[b].astype(np.uint64))
    claimed = part & ~core & (key != NO_KEY)
    single = part & ~core & (key == NO_KEY)
    anchor = np.where(claimed, (key & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    region[claimed] = region[anchor[claimed]]
    region[single] = np.flatnonzero(single)
    kind = np.where(core, 2, np.where(claimed, 1, np.where(single, 0, -1)))
    return region.astype(np.int32), kind.astype(np.int32), anchor.astype(np.int32)


def partition_literal(cloud, normals, k: int, cos, threshold, rows=None):
    """partition's answer by a per-point, per-neighbour loop with float32 scalars and a plain union-find."""
    cloud, normals, cos, threshold = _inputs(cloud, normals, k, cos, threshold)
    n = cloud.shape[0]
    idx, d2, _ = rows if rows is not None else rows_of(cloud, k)
    part = [bool(all(math.isfinite(float(v)) for v in cloud[p, :3]) and all(math.isfinite(float(v)) for v in normals[p])) for p in range(n)]
    core = [part[p] and not (normals[p, 3] > threshold) for p in range(n)]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def smooth(a, b):
        with np.errstate(invalid="ignore", over="ignore"):
            dot = F32(F32(F32(normals[a, 0] * normals[b, 0]) + F32(normals[a, 1] * normals[b, 1])) + F32(normals[a, 2] * normals[b, 2]))
            return bool(abs(dot) >= cos)

    best = [None] * n
    for i in range(n):
        if not core[i]:
            continue
        for s in range(idx.shape[1]):
            j = int(idx[i, s])
            if j < 0 or j == i or not part[j] or not smooth(i, j):
                continue
            if core[j]:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
            else:
                key = (int(np.asarray(d2[i, s], F32).view(np.uint32)) << 32) | i
                if best[j] is None or key < best[j]:
                    best[j] = key
    region, kind, anchor = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    for p in range(n):
        if core[p]:
            region[p], kind[p] = find(p), 2
        elif part[p] and best[p] is not None:
            anchor[p] = best[p] & 0xFFFFFFFF
            region[p], kind[p] = find(int(anchor[p])), 1
        elif part[p]:
            region[p], kind[p] = p, 0
    return region, kind, anchor


def emit(region, kind, anchor, min_size: int = 1, max_size: int = INT_MAX):
    """(region_start int64, indices int32, labels int32, region, kind, anchor): clustering's emission and order over the regions."""
    start, indices, labels, region = CR.from_components(region, min_size, max_size)
    return start, indices, labels, region, kind, anchor


def grow(cloud, normals, k: int = 30, cos=None, threshold=0.05, min_size: int = 1, max_size: int = INT_MAX, rows=None):
    """The library's answer: (region_start (n_regions + 1,) int64, indices int32, labels, region, kind, anchor (n,) int32 each).
    cos: the smoothness cosine (default: PCL's 30 degrees)."""
    cos = smoothness_cos(math.radians(30.0)) if cos is None else cos
    return emit(*partition(cloud, normals, k, cos, threshold, rows), min_size, max_size)


def grow_literal(cloud, normals, k: int = 30, cos=None, threshold=0.05, min_size: int = 1, max_size: int = INT_MAX, rows=None):
    cos = smoothness_cos(math.radians(30.0)) if cos is None else cos
    return emit(*partition_literal(cloud, normals, k, cos, threshold, rows), min_size, max_size)


def pcl_literal(cloud, normals, k: int = 30, cos=None, threshold=0.05, min_size: int = 1, max_size: int = INT_MAX, rows=None):
    """PCL 1.8 region_growing.hpp over every PARTICIPANT (PCL asserts on the others): (clusters, seeds) -- the regions in the order
    PCL grows them, each in the order its points were labelled, filtered by the size window as assembleRegions does, and every grown
    region's initial seed (before the filter: seeds[r] belongs to all_regions[r], returned third).  The curvature sort is
    std::sort in PCL (order among equals unspecified); here it is stable."""
    cos = smoothness_cos(math.radians(30.0)) if cos is None else cos
    cloud, normals, cos, threshold = _inputs(cloud, normals, k, cos, threshold)
    n = cloud.shape[0]
    idx, _, n_found = rows if rows is not None else rows_of(cloud, k)
    part = participants(cloud, normals)
    indices = np.flatnonzero(part)                                     # indices_
    num_of_pts = indices.size
    point_labels = [-1] * n
    # applySmoothRegionGrowingAlgorithm: point_residual = (curvature, index), sorted by curvature
    order = indices[np.argsort(normals[indices, 3], kind="stable")].tolist()

    def validate_point(point, nghbr):                                  # smooth_mode_flag_: the CURRENT seed's normal
        if not smooth_pairs(normals, np.int64(point), np.int64(nghbr), cos):
            return False, False                                        # "if (dot_product < cosine_threshold) return (false);"
        is_a_seed = not (normals[nghbr, 3] > threshold)                # curvature_flag_ && curvature > threshold: no seed
        return True, is_a_seed                                         # (residual_flag_ is off)

    def grow_region(initial_seed, segment_number):
        seeds = [initial_seed]
        head = 0
        point_labels[initial_seed] = segment_number
        members = [initial_seed]
        while head < len(seeds):
            curr_seed = seeds[head]
            head += 1
            i_nghbr = 0
            while i_nghbr < k and i_nghbr < int(n_found[curr_seed]):
                index = int(idx[curr_seed, i_nghbr])
                i_nghbr += 1
                if point_labels[index] != -1 or not part[index]:
                    continue
                belongs, is_a_seed = validate_point(curr_seed, index)
                if not belongs:
                    continue
                point_labels[index] = segment_number
                members.append(index)
                if is_a_seed:
                    seeds.append(index)
        return members

    all_regions, seeds_of = [], []
    if num_of_pts:
        seed_counter, seed = 0, order[0]
        segmented = 0
        while segmented < num_of_pts:
            members = grow_region(seed, len(all_regions))
            segmented += len(members)
            all_regions.append(members)
            seeds_of.append(seed)
            for i_seed in range(seed_counter + 1, num_of_pts):
                if point_labels[order[i_seed]] == -1:
                    seed, seed_counter = order[i_seed], i_seed
                    break
    clusters = [m for m in all_regions if min_size <= len(m) <= max_size]
    return clusters, seeds_of, all_regions


def agreement(a_regions, b_label, min_size: int = 50) -> float:
    """Of the points in the regions of a_regions (lists of indices) with min_size or more points, the fraction that falls in their
    region's majority region under b_label ((n,) ints, one name per point; negative: none)."""
    total = hit = 0
    for members in a_regions:
        if len(members) < min_size:
            continue
        names = b_label[np.asarray(members)]
        names = names[names >= 0]
        total += len(members)
        if names.size:
            hit += int(np.unique(names, return_counts=True)[1].max())
    return hit / total if total else 1.0
