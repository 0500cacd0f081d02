"""The segment moments on the device (icpgpu_segment_moments / icpgpu_segment_stats; icp_segment.hip) against the NumPy restatement
(tests/segment_restated.py): every field of every record bit for bit, a NaN matching any NaN.  There is no tolerance anywhere."""
import functools
import math
import os
import re

import numpy as np
import pytest

import segment_cases as K
import segment_restated as R
from icpslam_amd import SEGMENT_RECORD, Context, EuclideanClusterExtraction, IcpGpuError, MomentOfInertiaEstimation, _lib, synth
from test_segment_host import refusal_cases

pytestmark = pytest.mark.gpu

F32 = np.float32
CHUNK = R.CHUNK
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_f", "segment_2k.npz")
UNTOUCHED = b"\xab"


@functools.lru_cache(maxsize=None)
def scan(n: int = 3000, seed: int = 5) -> np.ndarray:
    cloud = synth.scan(synth.make_scene(3), np.eye(4), n, seed).copy()
    cloud[n // 3, 1] = np.nan                        # (one non-finite row among the listed ones)
    cloud.setflags(write=False)
    return cloud


def check(ctx, cloud, segments, what=""):
    """One call with a HOST source over the search cloud in place against the restatement; the wait count."""
    start, idx = R.csr(segments)
    want = R.records(cloud, start, idx)
    got = ctx.segment_moments(start, idx)
    assert got.dtype == SEGMENT_RECORD == R.RECORD
    assert R.same_records(got, want) == [], what
    if len(segments):
        assert ctx.segment_stats() == {"host_waits": 1}
    return got


def rows_of_lengths(lengths, n: int, seed: int):
    """Segments of the given lengths whose indices are drawn from range(n) with a fixed seed (repeats across segments are fine)."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, n, m).tolist() for m in lengths]


# ---- segment counts and row lengths -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_segments", [0, 1, 63, 64, 65, 257])
def test_segment_counts(ctx, n_segments):
    cloud = scan()
    ctx.search_set_input(cloud)
    lengths = np.random.default_rng(n_segments).integers(0, 40, n_segments).tolist()
    got = check(ctx, cloud, rows_of_lengths(lengths, len(cloud), 100 + n_segments), f"{n_segments} segments")
    assert got.shape == (n_segments,)


LENGTHS = (1, 2, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 255, 256, 257, 513)      # the chunk (a wave) and the workgroup of 256


@pytest.mark.parametrize("lead", [0, 1, CHUNK - 1, 255])
def test_row_lengths_at_every_edge(ctx, lead):
    """Rows of every length at which the kernel takes another path -- below, at and above the chunk (a wave's 64) and the workgroup's
    256 -- one after the other in both orders, behind a leading row that shifts where the chunk's multiples cut them."""
    cloud = scan()
    ctx.search_set_input(cloud)
    for order, lengths in enumerate((LENGTHS, LENGTHS[::-1])):
        lengths = ([lead] if lead else []) + list(lengths)
        check(ctx, cloud, rows_of_lengths(lengths, len(cloud), 7 * lead + order), f"lead {lead} lengths {lengths}")


@pytest.mark.parametrize("length", LENGTHS)
def test_one_row_alone(ctx, length):
    cloud = scan()
    ctx.search_set_input(cloud)
    check(ctx, cloud, rows_of_lengths([length], len(cloud), length))


def test_one_long_row_among_hundreds_of_short_ones(ctx):
    """The case the kernel is shaped for: one row of 20 000 entries in the middle of 500 rows of 3 -- 313 chunks hold the long row's
    pieces, the short rows lie packed 21 to a chunk."""
    cloud = scan(21000, 6)
    ctx.search_set_input(cloud)
    short = rows_of_lengths([3] * 500, len(cloud), 1)
    long_row = np.random.default_rng(2).permutation(len(cloud))[:20000].tolist()
    got = check(ctx, cloud, short[:250] + [long_row] + short[250:])
    assert got["count"][250] in (19999, 20000) and len(got) == 501                 # (the cloud's one NaN row may be listed)


def test_empty_rows_at_the_start_middle_and_end(ctx):
    cloud = scan()
    ctx.search_set_input(cloud)
    rows = rows_of_lengths([5, 300, 7, 64], len(cloud), 3)
    got = check(ctx, cloud, [[], []] + rows[:2] + [[], [], []] + rows[2:] + [[]])
    assert got["status"].tolist() == [1, 1, 0, 0, 1, 1, 1, 0, 0, 1]
    got = check(ctx, cloud, [[], [], []])
    assert got["status"].tolist() == [1, 1, 1] and not got["count"].any()


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_hand_clouds(ctx, name):
    case = K.CASES[name]
    ctx.search_set_input(case.cloud)
    check(ctx, case.cloud, case.segments, name)


def test_one_sum_whose_terms_span_fourteen_decades(ctx):
    case = K.wide_sum()
    ctx.search_set_input(case.cloud)
    got = check(ctx, case.cloud, case.segments)
    x = case.cloud[:, 0].astype(np.float64)
    assert got[0]["moments"][0] == math.fsum((x * x).tolist())


def clustered(n: int, seed: int) -> np.ndarray:
    """The cloud test_sor_cloud_the_grid_refuses builds: tight clusters (4 centres, sigma 0.3) in a wide sparse volume."""
    r = np.random.default_rng(seed)
    centres = r.uniform(-50, 50, (4, 3))
    c = np.ones((n, 4), F32)
    c[:, :3] = (centres[r.integers(0, 4, n)] + r.normal(0, 0.3, (n, 3))).astype(F32)
    c[::11, :3] = r.uniform(-200, 200, (len(c[::11]), 3)).astype(F32)
    return c


def test_cloud_the_grid_refuses(ctx, monkeypatch, capfd):
    """22 000 points whose densest cell holds more than 4 096: the grid refuses the cloud (ASSERTED, from the library's debug line).
    The call needs no grid."""
    cloud = clustered(22000, 1)
    cloud[7, 1] = np.nan
    monkeypatch.setenv("ICPGPU_DEBUG", "1")
    capfd.readouterr()
    ctx.search_set_input(cloud)
    found = re.findall(r"\[icpgpu\] grid n=22000 .* max=(\d+) ", capfd.readouterr().err)
    assert found and int(found[-1]) > 4096
    check(ctx, cloud, rows_of_lengths([1, 7, 5000, 300, 2], len(cloud), 4) + [[7]])
    assert re.search(r"\[icpgpu\] segment source=0 segments=6 entries=5311 chunks=83 waits=1", capfd.readouterr().err)


@pytest.mark.parametrize("leaf", [0.4])
def test_voxel_filtered_scan_through_all_three_sources(ctx, leaf):
    """The chain a user runs.  CLUSTERS / REGIONS records equal the HOST source's fed the fetched CSR, byte for byte, and the restatement's;
    afterwards the cluster or region result still fetches unchanged."""
    raw = synth.scan(synth.make_scene(3), np.eye(4), 20000, 7)
    cloud = ctx.voxel_grid(raw, leaf)
    ctx.search_set_input(cloud)
    normals, _ = ctx.normal_estimation(None, k=30)
    rc, n_clusters, n_clustered = ctx.cluster_extract_raw(0.5, 3, 2**31 - 1)
    rc2, n_regions, n_in = ctx.region_growing_raw(normals, 30, np.float32(math.cos(math.radians(30))), 0.05, 5, 2**31 - 1)
    assert rc == rc2 == 0 and n_clusters > 5 and n_regions > 5
    for source, count, size, fetch in (("clusters", n_clusters, n_clustered, ctx.cluster_fetch_raw), ("regions", n_regions, n_in, ctx.region_fetch_raw)):
        rc, start, idx, *rest = fetch(count, size)
        assert rc == 0
        got = ctx.segment_moments(source=source, n_segments=count)
        assert ctx.segment_stats() == {"host_waits": 1}
        assert R.same_records(got, R.records(cloud, start, idx)) == [], source
        assert ctx.segment_moments(start, idx).tobytes() == got.tobytes(), source
        rc, *again = fetch(count, size)                       # the result it read is as it was
        assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(again, [start, idx] + rest))
        assert ctx.segment_moments(source=source, n_segments=count).tobytes() == got.tobytes()
        print(f"{source}: {count} segments of {size} entries, sizes {np.diff(start)[:3]} .. {np.diff(start)[-3:]}")


def test_pcl_shaped_class(ctx):
    cloud = K.box_lattice().cloud
    moi = MomentOfInertiaEstimation()
    moi.setInputCloud(cloud)
    moi.compute()
    lo, hi = moi.getAABB()
    assert lo.tolist() == [1.0, -2.0, 0.5] and hi.tolist() == [7.0, 7.0, 15.5]
    omin, omax, position, rotation = moi.getOBB()
    assert omax.tolist() == [7.5, 4.5, 3.0] and omin.tolist() == [-7.5, -4.5, -3.0] and position.tolist() == list(K.BOX_CENTRE)
    assert rotation.tolist() == [[0, 0, -1], [0, 1, 0], [1, 0, 0]] and moi.getEigenValues() == (31.25, 11.25, 5.0)
    assert moi.getMassCenter().tolist() == list(K.BOX_CENTRE) and moi.getEigenVectors()[2].tolist() == [-1, 0, 0]
    moi.setIndices([0, 1, 2, 3])
    moi.compute()
    assert moi.getAABB()[1].tolist() == [1.0, -2.0, 15.5]
    ece = EuclideanClusterExtraction()
    ece.setInputCloud(scan())
    ece.setClusterTolerance(0.6)
    ece.setMinClusterSize(5)
    both = MomentOfInertiaEstimation()
    records = both.compute_clusters(ece)
    start, idx = R.csr(ece.extract())
    assert len(records) > 10 and R.same_records(records, R.records(scan(), start, idx)) == []


# ---- behaviour ------------------------------------------------------------------------------------------------------------------
def test_every_refusal_writes_nothing():
    """Every case of tests/test_segment_host.py's list on a context of its own.  Where a case speaks of a clustering or region growing
    result, the context gets a real one -- one cluster of all eight points, eight regions of one (k = 1) -- and the case's counts are
    taken relative to it."""
    n = 8
    cloud = scan()[:n].copy()
    normals = np.tile(np.array([0, 0, 1, 0], F32), (n, 1))
    for name, args, refused in refusal_cases(n):
        with Context(0) as c:
            if args.get("search_set", True):
                c.search_set_input(cloud)
            hc = hr = None
            if args.get("have_clusters") is not None:
                rc, hc, _ = c.cluster_extract_raw(1000.0, 1, 2**31 - 1)
                assert (rc, hc) == (0, 1)
            if args.get("have_regions") is not None:
                rc, hr, _ = c.region_growing_raw(normals, 1, 0.5, 0.05, 1, 2**31 - 1)
                assert (rc, hr) == (0, n)
            if args["source"] == 1 and hc is not None:
                args = dict(args, n_segments=hc + args["n_segments"] - args["have_clusters"])
            elif args["source"] == 2 and hr is not None:
                args = dict(args, n_segments=hc)
            args = dict(args, have_clusters=hc, have_regions=hr)
            assert R.validate(**args) == refused, name
            rc, records = c.segment_moments_raw(args["source"], args["n_segments"], args["segment_start"], args["indices"],
                                                sizeof_record=args.get("sizeof_record"), null_out=args.get("null_out", False))
            assert (rc == _lib.ERR_INVALID_ARG) == refused and rc in (0, _lib.ERR_INVALID_ARG), (name, rc)
            if refused:
                assert records.tobytes() == UNTOUCHED * records.nbytes, name
                assert c.segment_stats() == {"host_waits": 0}
            elif not args.get("null_out"):
                assert UNTOUCHED * 8 not in records.tobytes(), name


def test_device_sources_without_a_result_and_with_a_stale_one(ctx):
    cloud = scan()
    ctx.search_set_input(cloud)                        # a search cloud, no result over it (any earlier one is dropped)
    for code in (_lib.SEGMENTS_CLUSTERS, _lib.SEGMENTS_REGIONS):
        assert ctx.segment_moments_raw(code, 0)[0] == _lib.ERR_INVALID_ARG
    rc, n_clusters, _ = ctx.cluster_extract_raw(0.6, 5, 2**31 - 1)
    assert rc == 0 and n_clusters > 3
    assert ctx.segment_moments_raw(_lib.SEGMENTS_CLUSTERS, n_clusters)[0] == 0
    assert ctx.segment_moments_raw(_lib.SEGMENTS_REGIONS, n_clusters)[0] == _lib.ERR_INVALID_ARG
    assert ctx.segment_moments_raw(_lib.SEGMENTS_CLUSTERS, n_clusters + 1)[0] == _lib.ERR_INVALID_ARG
    ctx.search_set_input(cloud)                        # the same cloud again: the result is stale
    rc, records = ctx.segment_moments_raw(_lib.SEGMENTS_CLUSTERS, n_clusters)
    assert rc == _lib.ERR_INVALID_ARG and records.tobytes() == UNTOUCHED * records.nbytes
    with pytest.raises(IcpGpuError):
        ctx.segment_moments(source="clusters", n_segments=n_clusters)


def test_five_identical_runs(ctx):
    cloud = scan(21000, 6)
    ctx.search_set_input(cloud)
    start, idx = R.csr(rows_of_lengths([3] * 100 + [15000] + [70, 300, 1] * 30, len(cloud), 9))
    runs = {ctx.segment_moments(start, idx).tobytes() for _ in range(5)}
    assert len(runs) == 1


def test_golden_fixture(ctx):
    g = np.load(GOLDEN)
    ctx.search_set_input(g["cloud"])
    got = ctx.segment_moments(g["segment_start"], g["indices"])
    assert R.same_records(got, g["records"]) == []
