"""The C++ shim's segment moments (include/icpgpu_registration.hpp: icpgpu::MomentOfInertiaEstimation, getMinMax3D, compute3DCentroid,
computeMeanAndCovarianceMatrix) with PCL's spelling of every call: tests/cpp/segment_demo.cpp runs VoxelGrid ->
ProgressiveMorphologicalFilter -> ExtractIndices(negative) -> EuclideanClusterExtraction -> MomentOfInertiaEstimation::computeClusters on
a street scene with five boxes of 0.8 m x 1.6 m x 2.4 m at five yaws.  The five records must be the restatement's on the demo's own
cloud, and every box's oriented dimensions and major axis must agree with its construction."""
import math
import os
import subprocess

import numpy as np
import pytest

import cluster_restated as CR
import oracle
import pmf_restated as P
import segment_restated as R
from icpslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJECTS = ((-6.0, -5.0, 0.0), (-1.0, 4.0, 20.0), (4.0, -4.0, 45.0), (7.0, 5.0, 70.0), (0.5, -7.5, 110.0))   # centre x, y; yaw in degrees
DIMS = (2.4, 1.6, 0.8)            # major (the height), middle, minor: distinct, so no tie rule decides an axis
SIGMA_FACE, SIGMA_GROUND = 0.005, 0.002
LEAF, INITIAL_DISTANCE, TOLERANCE, MIN_SIZE = 0.15, 0.03, 0.5, 20
# a face's points lie within 4 sigma of it (1 in 16 000 does not; 36 000 box points) and the voxel filter's centroids lie inside their
# voxels, so a box's outermost centroid is at most a leaf inside its face and at most 4 sigma outside: per face, and a dimension has two
DIMS_BOUND = 2.0 * (LEAF + 4.0 * SIGMA_FACE)
# the major axis against the vertical and the middle axis against the box's long side: measured with the restatement on the CPU chain
# below for this seed (test_restatement_...), the worst of the five boxes and the two axes; asserted at twice that
ANGLE_MEASURED_DEG = 3.14
ANGLE_BOUND_DEG = 2.0 * ANGLE_MEASURED_DEG


def street_scene(seed=4) -> np.ndarray:
    """A flat 24 m x 24 m patch of ground (2 mm of noise) and the SURFACES of five boxes standing on it: 0.8 m x 1.6 m footprints,
    2.4 m high, yawed by 0, 20, 45, 70 and 110 degrees, four sides and the top each within half a centimetre."""
    r = np.random.default_rng(seed)
    parts = [np.concatenate([r.uniform(-12, 12, (12000, 2)), r.normal(0, SIGMA_GROUND, (12000, 1))], axis=1)]
    hx, hy, hz = DIMS[1] / 2, DIMS[2] / 2, DIMS[0]          # the box frame: x along the 1.6 m side, y along the 0.8 m side
    for cx, cy, yaw in OBJECTS:
        local = []
        for axis, half, other in ((0, hx, hy), (1, hy, hx)):
            for sign in (-1.0, 1.0):
                p = np.zeros((1500, 3))
                p[:, axis] = sign * half + r.normal(0, SIGMA_FACE, 1500)
                p[:, 1 - axis] = r.uniform(-other, other, 1500)
                p[:, 2] = r.uniform(0.0, hz, 1500)
                local.append(p)
        local.append(np.concatenate([r.uniform(-1, 1, (1200, 2)) * (hx, hy), hz + r.normal(0, SIGMA_FACE, (1200, 1))], axis=1))
        local = np.concatenate(local)
        a = math.radians(yaw)
        world = local.copy()
        world[:, 0] = cx + math.cos(a) * local[:, 0] - math.sin(a) * local[:, 1]
        world[:, 1] = cy + math.sin(a) * local[:, 0] + math.cos(a) * local[:, 1]
        parts.append(world)
    cloud = np.ones((sum(len(p) for p in parts), 4), np.float32)
    cloud[:, :3] = r.permutation(np.concatenate(parts)).astype(np.float32)
    return cloud


def judge(objects, start, idx, records):
    """Five clusters, one per box; each record's dims and position against the construction.  Returns the worst angle, in degrees, of a
    major axis from the vertical or of a middle axis from its box's long side."""
    assert len(records) == len(OBJECTS) == len(start) - 1
    seen, worst = set(), 0.0
    for r in records:
        near = [j for j, (cx, cy, _) in enumerate(OBJECTS) if math.hypot(r["centroid"][0] - cx, r["centroid"][1] - cy) < 0.2]
        assert len(near) == 1 and r["status"] == R.OK and r["count"] >= MIN_SIZE
        seen.add(near[0])
        yaw = math.radians(OBJECTS[near[0]][2])
        assert np.abs(r["obb_dims"] - DIMS).max() <= DIMS_BOUND, (near, r["obb_dims"])
        assert np.abs(r["obb_position"] - [OBJECTS[near[0]][0], OBJECTS[near[0]][1], DIMS[0] / 2]).max() <= DIMS_BOUND / 2
        major, middle = r["axes"][:3], r["axes"][3:6]
        angle = math.degrees(math.acos(min(1.0, abs(major[2]))))
        worst = max(worst, angle)
        assert major[2] > 0                                              # the sign rule: the largest component is positive
        along = abs(middle[0] * math.cos(yaw) + middle[1] * math.sin(yaw))   # the middle axis against the 1.6 m side's direction
        worst = max(worst, math.degrees(math.acos(min(1.0, along))))
    assert seen == set(range(len(OBJECTS)))
    return worst


def test_restatement_on_the_scene_through_the_cpu_chain():
    """The chain on the CPU -- the oracle's voxel filter, the ground filter's, the clustering's and the segment moments' restatements --
    is where the angle bound comes from: the worst major axis is 2.342 degrees from the vertical and the worst middle axis 3.133 degrees
    from its box's long side for this seed -- a box has a top and no bottom, and the voxel centroids sample its faces unevenly; the GPU
    test asserts twice the worst, 6.28.  The dims are asserted against
    DIMS_BOUND = 2 (leaf + 4 sigma) = 0.34 m here as there."""
    raw = street_scene()
    filtered = oracle.voxel_grid(raw, LEAF)
    ground = P.run(filtered, initial_distance=INITIAL_DISTANCE)["ground"]
    objects = P.extract(filtered, ground, negative=True)
    start, idx, _, _ = CR.extract(objects, TOLERANCE, MIN_SIZE)
    records = R.records(objects, start, idx)
    worst = judge(objects, start, idx, records)
    print(f"worst axis angle {worst:.3f} degrees; dims errors {[np.abs(r['obb_dims'] - DIMS).max().round(3) for r in records]}")
    assert worst <= ANGLE_MEASURED_DEG < ANGLE_BOUND_DEG


def _build(tmp_path):
    exe = tmp_path / "segment_demo"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "segment_demo.cpp"), "-o", str(exe), "-L", libdir, "-licpgpu",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_demo_compiles_with_pcl_spelling(built, tmp_path):
    assert _build(tmp_path).exists()


def floats(line):
    words = line.split()
    return np.array([int(w, 16) for w in words[1:]], np.uint32).view(np.float32).reshape(int(words[0]), 4)


@pytest.mark.gpu
def test_demo_describes_the_five_boxes(built, ctx, tmp_path):
    """Worst axis angle measured on the CPU chain: 3.133 degrees (major axes alone: 2.342); asserted here: 6.28 degrees."""
    exe = _build(tmp_path)
    raw = street_scene()
    a = tmp_path / "cloud.bin"
    raw.tofile(a)
    r = subprocess.run([str(exe), str(a), str(len(raw)), str(LEAF), str(INITIAL_DISTANCE), str(TOLERANCE), str(MIN_SIZE), str(len(OBJECTS))],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr, r.stdout[-400:])
    lines = r.stdout.split("\n")
    objects = floats(lines[0])
    n_clusters = int(lines[1])
    assert n_clusters == len(OBJECTS)
    segments = [[int(v) for v in lines[2 + q].split()] for q in range(n_clusters)]
    start, idx = R.csr(segments)
    got = np.frombuffer(np.array([int(w, 16) for q in range(n_clusters) for w in lines[2 + n_clusters + q].split()], np.uint32).tobytes(), R.RECORD)
    assert R.same_records(got, R.records(objects, start, idx)) == []
    worst = judge(objects, start, idx, got)
    print(f"worst axis angle {worst:.3f} degrees")
    assert worst <= ANGLE_BOUND_DEG
    assert lines[2 + 2 * n_clusters] == "one-segment calls agree"
