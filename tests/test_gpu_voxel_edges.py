"""The voxel filter where its suite never went, bit for bit against oracle.voxel_grid: the edges of the plan (PCL's "leaf size is
too small" pass-through for every box and leaf: icp_voxel_plan.h, tests/voxel_edge_cases.py), the sort path run on its own
(ICPGPU_VOXEL_SORT=1, development flavour) across the tile sizes of the radix sort and the scan it stands on (icp_scan.hip), and
the one way a user reaches the sort path: a cloud of more than 2^21 points."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from icpslam_amd import synth

import voxel_edge_cases as vx

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same(got, ref):
    return got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref))


# ---- the overflow edge ---------------------------------------------------------------------------------------------------------
def edge_cases():
    """(name, cloud, leaf, verdict): the boundary table as clouds -- the box's corners and up to 3000 points inside, pad 7 so that a
    returned input is told from a filtered cloud, non-finite points mixed into every third -- and the finding's seven rows."""
    out = []
    for k, (name, lo, hi, leaf, want) in enumerate(vx.boundary_boxes()):
        if want == vx.NO_FINITE:
            cloud = np.full((300, 4), np.nan, F32)
        else:
            cloud = vx.cloud_in_box(lo, hi, (0, 5, 700, 3000)[k % 4], seed=k, bad=40 if k % 3 == 0 else 0, pad=7.0)
        out.append((name, cloud, leaf, want))
    for k, (name, cloud, leaf) in enumerate(vx.finding_rows()):
        c = cloud.copy()
        if k % 2:
            c[5::97, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
        out.append((name, c, leaf, vx.PASS_THROUGH))
    return out


@pytest.fixture(scope="module")
def edges():
    cases = edge_cases()
    refs = [oracle.voxel_grid(c, leaf) for _, c, leaf, _ in cases]
    ordinary = synth.make_pair(20000, 10, seed=3)[0]
    return cases, refs, ordinary, oracle.voxel_grid(ordinary, 0.2)


def _digest(rows):
    h = hashlib.sha256()
    for r in rows:
        h.update(np.ascontiguousarray(r, F32).tobytes())
        h.update(b"|%d|" % len(r))
    return h.hexdigest()


def test_overflow_edge_against_the_oracle(ctx, edges):
    """Every case through icpgpu_voxel_grid, icpgpu_voxel_grid_view and icpgpu_set_source_voxel_filtered (followed by a 3-iteration
    alignment, which builds its grids from the handed-over box); each pass-through followed by an ordinary cloud on the same context:
    the histogram, the published counts and the kept bounding box stayed clean."""
    cases, refs, ordinary, ordinary_ref = edges
    target = ordinary_ref
    n_pass = 0
    for (name, cloud, leaf, want), ref in zip(cases, refs):
        returned = _same(ref, cloud)
        assert returned == (want == vx.PASS_THROUGH), name                     # the oracle and the table agree
        if want == vx.NO_FINITE:
            assert len(ref) == 0, name
        for fn in (ctx.voxel_grid, ctx.voxel_grid_view):
            got = fn(cloud, leaf)
            assert _same(got, ref), (name, fn.__name__, got.shape, ref.shape)
        ctx.set_params(max_iterations=3)
        assert ctx.set_source_voxel_filtered(cloud, leaf) == len(ref), name
        if len(ref):
            ctx.set_target(target)
            got = ctx.align()
            want_a = oracle.icp_align(ref, target, oracle.default_params(max_iterations=3))
            print(name, "align:", got["iterations"], got["n_corr"], got["converged"], "| oracle:", want_a["iterations"], want_a["n_corr"],
                  want_a["converged"])
            assert (got["iterations"], got["n_corr"], got["converged"]) == (want_a["iterations"], want_a["n_corr"], want_a["converged"]), name
        if returned:
            n_pass += 1
            assert _same(ctx.voxel_grid(ordinary, 0.2), ordinary_ref), name
            assert _same(ctx.voxel_grid_view(ordinary, 0.2), ordinary_ref), name
    assert n_pass >= 30
    ctx.set_params(ctx.default_params())


_EDGE_CHILD = (
    "import sys, numpy as np\n"
    "sys.path.insert(0, sys.argv[2])\n"
    "from icpslam_amd import Context\n"
    "import test_gpu_voxel_edges as t\n"
    "with Context(0) as c:\n"
    "    rows = []\n"
    "    for name, cloud, leaf, want in t.edge_cases():\n"
    "        rows += [c.voxel_grid(cloud, leaf), c.voxel_grid_view(cloud, leaf)]\n"
    "        rows.append(np.full((1, 4), c.set_source_voxel_filtered(cloud, leaf), np.float32))\n"
    "print('digest', t._digest(rows), len(rows))\n")


def test_overflow_edge_waiting_for_the_box_gives_the_same_bytes(ctx, edges):
    """The development flavour with ICPGPU_VOXEL_PLANNED=0 derives the plan on the host from the box it waited for; the release
    flavour takes the device's verdict.  One function, so: identical bytes for every case and every entry point."""
    cases, refs, _, _ = edges
    rows = []
    for (name, cloud, leaf, want), ref in zip(cases, refs):
        rows += [ctx.voxel_grid(cloud, leaf), ctx.voxel_grid_view(cloud, leaf)]
        rows.append(np.full((1, 4), ctx.set_source_voxel_filtered(cloud, leaf), F32))
    env = dict(os.environ, ICPGPU_FLAVOUR="dev", ICPGPU_VOXEL_PLANNED="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _EDGE_CHILD, "-", os.path.join(ROOT, "tests")], env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[-3:] == ["digest", _digest(rows), str(len(rows))], r.stdout[-500:]
    assert _digest(rows) == _digest([x for ref in refs for x in (ref, ref, np.full((1, 4), len(ref), F32))])


# ---- the sort path on its own --------------------------------------------------------------------------------------------------
def _uniform(n, seed, half=8.0):
    c = np.ones((n, 4), F32)
    c[:, :3] = np.random.default_rng(seed).uniform(-half, half, (n, 3)).astype(F32)
    return c


def sort_path_clouds():
    """(name, cloud, leaf).  The clouds of three direct-path tests (test_gpu_voxel.py) and the wrapped-index seed; n around the radix
    sort's tile (2048), the scan's (4096) and the second tile of the sort's histogram scan (16 * tiles > 4096: n > 524 288); one
    voxel (all keys equal); keys strictly descending in input order; keys with bit 31 set (the wrapped index: negative keys)."""
    out = []
    rng = np.random.default_rng(9)
    for n in (2, 63, 64, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 8191):   # ...around_the_group_quantum
        c = np.ones((n, 4), F32)
        c[:, :3] = rng.uniform(-8, 8, (n, 3)).astype(F32)
        out += [(f"quantum {n}", c, 0.1), (f"quantum {n}", c, 1.5)]
    rng = np.random.default_rng(21)                                                                      # ...narrow_and_wide_sort_words
    tight = np.ones((60000, 4), F32)
    tight[:, :3] = rng.normal(0, 1.5, (60000, 3)).astype(F32)
    mixed = tight.copy()
    mixed[::7, :3] = rng.uniform(-400, 400, (len(mixed[::7]), 3)).astype(F32)
    dup = np.ones((3000, 4), F32)
    dup[:, :3] = F32(0.123)
    dup[1500:, :3] = rng.uniform(-3, 3, (1500, 3)).astype(F32)
    out += [(nm, c, leaf) for nm, c in (("tight", tight), ("mixed", mixed), ("dup", dup)) for leaf in (0.2, 0.35)]
    scene = synth.make_scene(31)                                                                         # ...raw_scan_dense_voxels
    out += [(f"scan {n}", synth.scan(scene, np.eye(4), n, seed=n), leaf) for n in (5000, 70000) for leaf in (0.2, 0.5, 2.0)]
    rng = np.random.default_rng(9000 + 2864)                                                             # the wrapped-index seed
    n = int(rng.integers(1, 120000))
    leaf = float(rng.choice([0.03, 0.1, 0.2, 0.35, 0.77, 2.0, 5.0]))
    wrap = np.ones((n, 4), F32)
    wrap[:, :3] = rng.normal(0, float(rng.choice([2.0, 30.0, 300.0])), (n, 3)).astype(F32)
    out.append(("wrapped index (keys with bit 31 set)", wrap, leaf))
    for n in (2047, 2048, 2049, 4095, 4096, 4097):
        out.append((f"tile {n}", _uniform(n, n), 0.7))
    for n in (524287, 524288, 524289):
        out.append((f"tile {n}", _uniform(n, n, 40.0), 0.5))
    one = np.ones((5000, 4), F32)
    one[:, :3] = np.random.default_rng(1).uniform(0.01, 0.19, (5000, 3)).astype(F32)
    out.append(("one voxel", one, 0.2))
    desc = _uniform(9001, 77, 30.0)
    inv = F32(1.0) / F32(0.5)
    cell = np.floor(desc[:, :3] * inv).astype(np.int64)
    desc = desc[np.lexsort((-cell[:, 0], -cell[:, 1], -cell[:, 2]))]
    _, first = np.unique(np.floor(desc[:, :3] * inv).astype(np.int64), axis=0, return_index=True)
    out.append(("strictly descending keys", np.ascontiguousarray(desc[np.sort(first)]), 0.5))
    return out


@pytest.fixture(scope="module")
def sort_cases():
    cases = sort_path_clouds()
    return cases, [oracle.voxel_grid(c, leaf) for _, c, leaf in cases]


def test_direct_path_on_the_sort_paths_clouds(ctx, sort_cases):
    """The switch off (release flavour): the same clouds, the same oracle bits -- so the two paths' bits are each other's."""
    cases, refs = sort_cases
    name, desc, leaf = cases[-1]
    keys = np.floor(desc[:, :3] * (F32(1.0) / F32(leaf))).astype(np.int64)
    lin = (keys - keys.min(0)) @ np.array([1, 1000, 1000000])
    assert name.startswith("strictly descending") and len(desc) > 4096 and (np.diff(lin) < 0).all()
    for (name, cloud, leaf), ref in zip(cases, refs):
        assert _same(ctx.voxel_grid(cloud, leaf), ref), name
    assert refs[-2].shape == (1, 4)                                            # "one voxel" is one


def test_sort_path_on_its_own(dev_flavour, sort_cases):
    """ICPGPU_VOXEL_SORT=1: every cloud goes down launch_voxel_grid -- the radix sort and the exclusive scan of icp_scan.hip, which
    also carry NDT's cell sort, the bf16 brute force's Morton order, the map's compactions and the reciprocal search's cell table."""
    os.environ["ICPGPU_VOXEL_SORT"] = "1"          # (read once, at the process's first filter: the delegated run is this test alone)
    if dev_flavour.delegated:
        del os.environ["ICPGPU_VOXEL_SORT"]
        return
    from icpslam_amd import Context
    cases, refs = sort_cases
    with Context(0) as c:
        c.profile_reset()
        for (name, cloud, leaf), ref in zip(cases, refs):
            assert _same(c.voxel_grid(cloud, leaf), ref), name
        for k in (0, 40, len(cases) - 1):
            assert _same(c.voxel_grid_view(cases[k][1], cases[k][2]), refs[k]), cases[k][0]
        assert c.profile().voxel_views_direct == 0                             # the switch took: nothing went the direct way


# ---- by size: the sort path as a user reaches it ---------------------------------------------------------------------------------
def test_two_million_points_take_the_sort_path(ctx, capsys):
    """2^21 points are the direct path's last size, 2^21 + 1 the sort path's first (release flavour).  A 262 145-point scan, eight
    times over with a few millimetres between the copies: dense near-field voxels of hundreds of points, as in a raw scan."""
    base = synth.scan(synth.make_scene(3), np.eye(4), (1 << 18) + 1, seed=4)
    big = np.concatenate([base + np.array([0.013 * k, -0.007 * k, 0.003 * k, 0], F32) for k in range(8)])[:(1 << 21) + 1]
    big = np.ascontiguousarray(big, F32)
    for n in (1 << 21, (1 << 21) + 1):
        cloud = big[:n]
        ref = oracle.voxel_grid(cloud, 0.2)
        ctx.profile_reset()
        got = ctx.voxel_grid(cloud, 0.2)
        p = ctx.profile()
        with capsys.disabled():
            print(f"\n[voxel by size] n = {n}: {'direct' if n <= 1 << 21 else 'sort'} path, {p.voxel_ms:.3f} ms on the device, {len(ref)} voxels")
        assert _same(got, ref), n
        assert 0 < len(ref) < n // 8
