"""An independent NumPy restatement of euclidean clustering (include/icpgpu.h, "euclidean clustering"), built on the neighbour
search's restatement (tests/search_restated.py: radius).  It never calls the library.

    graph      the finite points; i != j joined iff d2(i, j) < (float32)(tolerance * tolerance), strict -- the radius rows
    component  a connected component (a plain union-find over the rows); its name is its lowest index; -1 for a non-finite point
    cluster    a component with min_size <= size <= max_size
    order      size descending, the lowest name first among equals; indices ascending inside a cluster
    labels     the rank of the point's cluster in that order, -1 where it is in none

pcl_literal is PCL 1.8's extractEuclideanClusters transcribed -- the processed flags, the seed queue, the size test -- over the same
radius rows; it gives the same clusters as sets (tests/test_cluster_host.py), in PCL's own order.
"""
from __future__ import annotations

import math

import numpy as np

import search_restated as S

INT_MAX = 2**31 - 1
_WINDOWED_FROM, _WINDOW_CHUNK = 4096, 1024


class Refused(ValueError):
    """The library answers ICPGPU_ERR_INVALID_ARG."""


def radius_rows(cloud, tolerance: float):
    """(cloud (n, 4) float32, row_start, idx): every point's radius row over the cloud itself -- the graph's adjacency lists."""
    if not math.isfinite(tolerance) or tolerance < 0:
        raise Refused("tolerance")
    cloud = np.asarray(cloud, np.float32).reshape(-1, 4)
    n = cloud.shape[0]
    if n <= _WINDOWED_FROM:
        start, idx, _ = S.radius(cloud, None, float(tolerance))
        return cloud, start, idx
    # A large cloud (the restatement is quadratic): the same rows from S.radius, asked chunk by chunk in x order against only the
    # points whose x lies within the chunk's range widened by 1.01 tolerances.  Nothing is decided here: a point left out has
    # |dx| > 1.01 tolerance, so fl(dx * dx) > r2 and d2 >= fl(dx * dx) (rounding is monotone); the subset keeps the cloud's index
    # order, so S.radius orders equal distances as it would over the whole cloud.
    x = cloud[:, 0].astype(np.float64)
    by_x = np.argsort(np.where(np.isfinite(x), x, np.inf), kind="stable")
    margin = 1.01 * float(tolerance) + 1e-30
    counts, rows_idx = np.zeros(n, np.int64), [None] * n
    for a in range(0, n, _WINDOW_CHUNK):
        chunk = by_x[a:a + _WINDOW_CHUNK]
        xs = x[chunk][np.isfinite(x[chunk])]
        if xs.size == 0:
            continue
        near = np.flatnonzero((x >= xs.min() - margin) & (x <= xs.max() + margin))   # ascending: the cloud's index order
        st, ix, _ = S.radius(cloud[near], cloud[chunk], float(tolerance))
        for k, q in enumerate(chunk.tolist()):
            rows_idx[q] = near[ix[st[k]:st[k + 1]]]
            counts[q] = st[k + 1] - st[k]
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    filled = [r for r in rows_idx if r is not None and r.size]
    idx = np.concatenate(filled).astype(np.int32) if filled else np.zeros(0, np.int32)
    return cloud, start, idx


def components(cloud, tolerance: float, rows=None) -> np.ndarray:
    """component (n,) int32: the lowest index of every finite point's connected component, -1 for the others.  (rows: what
    radius_rows(cloud, tolerance) returned, when the caller has it already.)"""
    cloud, start, idx = rows if rows is not None else radius_rows(cloud, tolerance)
    n = cloud.shape[0]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    rows = np.repeat(np.arange(n), np.diff(start))
    once = idx < rows                                # d2 is symmetric: every edge is in both rows, one of them is enough
    for i, j in zip(rows[once].tolist(), idx[once].tolist()):
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    comp = np.array([find(i) for i in range(n)], np.int32).reshape(n)
    comp[~S.finite_mask(cloud)] = -1
    return comp


def from_components(comp: np.ndarray, min_size: int = 1, max_size: int = INT_MAX):
    """(cluster_start int64, indices int32, labels int32, component int32) from the components' names."""
    comp = np.asarray(comp, np.int32)
    n = comp.shape[0]
    names, sizes = np.unique(comp[comp >= 0], return_counts=True)
    emitted = (sizes >= min_size) & (sizes <= max_size)
    names, sizes = names[emitted], sizes[emitted]
    order = np.lexsort((names, -sizes))            # size descending, the lowest name first among equals
    names, sizes = names[order], sizes[order]
    rank_of = np.full(n + 1, -1, np.int32)          # (slot n: what comp = -1 reads)
    rank_of[names] = np.arange(names.size, dtype=np.int32)
    labels = rank_of[np.where(comp >= 0, comp, n)].astype(np.int32)
    members = np.flatnonzero(labels >= 0)
    indices = members[np.argsort(labels[members], kind="stable")].astype(np.int32)   # ascending inside a cluster
    cluster_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return cluster_start, indices, labels, comp


def extract(cloud, tolerance: float, min_size: int = 1, max_size: int = INT_MAX):
    """(cluster_start (n_clusters + 1,) int64, indices (n_clustered,) int32, labels (n,) int32, component (n,) int32)."""
    return from_components(components(cloud, tolerance), min_size, max_size)


def as_sets(cluster_start, indices) -> set:
    return {frozenset(indices[a:b].tolist()) for a, b in zip(cluster_start[:-1], cluster_start[1:])}


def pcl_literal(cloud, tolerance: float, min_size: int = 1, max_size: int = INT_MAX, rows=None) -> list:
    """PCL 1.8 extractEuclideanClusters (segmentation/extract_clusters.hpp) over every FINITE point as a seed, clusters in the order
    PCL finds them, each in seed-queue order.  (A non-finite seed is skipped: PCL asserts there.)  rows: as for components."""
    cloud, start, idx = rows if rows is not None else radius_rows(cloud, tolerance)
    n = cloud.shape[0]
    finite = S.finite_mask(cloud)
    processed = [False] * n
    clusters = []
    for i in range(n):
        if processed[i] or not finite[i]:
            continue
        seed_queue = [i]
        sq_idx = 0
        processed[i] = True
        while sq_idx < len(seed_queue):
            q = seed_queue[sq_idx]
            nn = idx[start[q]:start[q + 1]]           # radiusSearch(q, tolerance): q itself first, then the others
            if nn.size == 0:                          # "if (!tree->radiusSearch(...)) { sq_idx++; continue; }"
                sq_idx += 1
                continue
            for j in nn[1:].tolist():                 # "for (size_t j = nn_start_idx; ...)" with nn_start_idx = 1 (sorted results)
                if processed[j]:
                    continue
                seed_queue.append(j)
                processed[j] = True
            sq_idx += 1
        if min_size <= len(seed_queue) <= max_size:
            clusters.append(seed_queue)
    return clusters
