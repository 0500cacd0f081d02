"""An independent NumPy restatement of ISS with border estimation (include/icpgpu.h, "ISS keypoints", BORDER ESTIMATION), on top of
tests/iss_restated.py, tests/boundary_restated.py and tests/normals_restated.py.  It never calls the library.

    normals   the given rows, or normals_restated.estimate(cloud, None, 0, normal_radius) with the viewpoint at the origin
    edge      point i is finite, its border ball holds >= min_neighbors points and the boundary rule on that row with n_i says 1
    border    point i is finite and some j of its border ball, itself included, is an edge point
    skip      a border point has scatter6, eigenvalues3 and saliency 0; n_salient is still its salient ball's size
    the rest  iss_restated's: selection, non-maxima suppression, the keypoints ascending
"""
from __future__ import annotations

import math

import numpy as np

import boundary_restated as B
import iss_restated as R
import normals_restated as N
import search_restated as S

F32, F64 = np.float32, np.float64
Refused = S.Refused
FIELDS = R.FIELDS + ("edge", "border")


def keypoints_border(cloud, salient_radius: float, non_max_radius: float, gamma_21: float = 0.975, gamma_32: float = 0.975,
                     min_neighbors: int = 5, border_radius: float = 0.0, angle_threshold: float = math.pi / 2, normals=None,
                     normal_radius: float = 0.0):
    """iss_restated.keypoints' dict plus edge and border (n,) int32."""
    R.check_arguments(salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors)
    if not (math.isfinite(border_radius) and border_radius >= 0):
        raise Refused("border_radius")
    cloud = np.ascontiguousarray(cloud, F32).reshape(-1, 4)
    n = cloud.shape[0]
    if border_radius == 0:
        out = R.keypoints(cloud, salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors)
        out["edge"], out["border"] = np.zeros(n, np.int32), np.zeros(n, np.int32)
        return out
    B.check_threshold(angle_threshold)
    if normals is None:
        if not (math.isfinite(normal_radius) and normal_radius > 0):
            raise Refused("normals")
        normals = N.estimate(cloud, None, 0, normal_radius)[0] if n else np.zeros((0, 4), F32)
    finite = S.finite_mask(cloud)
    bstart, bidx, _ = S.radius(cloud, None, border_radius, 0)
    edge = B.from_rows(cloud, None, normals, bstart, bidx, angle_threshold, min_row=min_neighbors)["boundary"].astype(np.int32)
    border = np.zeros(n, np.int32)
    for i in np.flatnonzero(finite):
        border[i] = int(edge[bidx[bstart[i]:bstart[i + 1]]].any())
    on = border.astype(bool)
    start, idx, _ = S.radius(cloud, None, salient_radius, 0)
    n_salient, scatter6 = R.scatter(cloud, start, idx, min_neighbors)
    scatter6[on] = 0.0
    eig = R.eigenvalues(scatter6, n_salient, min_neighbors, finite & ~on)
    saliency = R.select(eig, n_salient, gamma_21, gamma_32, min_neighbors)
    saliency[~finite | on] = 0.0
    start2, idx2, _ = S.radius(cloud, None, non_max_radius, 0)
    index = np.flatnonzero(R.suppress(saliency, start2, idx2, min_neighbors)).astype(np.int32)
    return {"n_keypoints": int(index.size), "keypoint_index": index, "keypoints": cloud[index].copy(), "n_salient": n_salient,
            "scatter6": scatter6, "eigenvalues3": eig, "saliency": saliency, "edge": edge, "border": border}


def same_bits(a: dict, b: dict) -> list:
    bad = [] if a["n_keypoints"] == b["n_keypoints"] else ["n_keypoints"]
    for f in FIELDS:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(f)
    return bad
