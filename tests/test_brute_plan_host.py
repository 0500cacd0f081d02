"""icpslam_amd/csrc/icp_brute_plan.h -- the one statement of the matrix-core brute-force kernels' launch arithmetic -- built for the
host (tests/cpp/brute_plan_check.cpp) and held, row by row, to the restatement in Python integers (tests/brute_edge_cases.py:
plan_mfma, plan_bf16 as shipped and in its bound-check shape), at the edges of the workgroup and of the tile.  No GPU."""
import functools
import itertools
import os
import subprocess

import pytest

import brute_edge_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256
PLANS = {"mfma": B.plan_mfma, "bf16": B.plan_bf16, "bf16-check": functools.partial(B.plan_bf16, check=True)}
# sizes at which every shape's splits hold exactly two tiles (65 537 sources, 256 CUs), the second one of 33 rows
TWO_TILES = {name: B.multi_tile_targets(fn, CUS, 33) for name, fn in PLANS.items()}
N_Q = (1, 255, 256, 257, 511, 512, 513, 8193, 65537)
N_T = (1, 511, 512, 513, 1023, 1024, 1025, 2047, 2049) + tuple(sorted(set(TWO_TILES.values())))
NUM_CUS = (1, 64, 256, 304)


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("brute_plan") / "brute_plan_check")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "icpslam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "brute_plan_check.cpp"), "-o", exe])
    table = "".join(f"{q} {t} {c}\n" for q, t, c in itertools.product(N_Q, N_T, NUM_CUS))
    out = subprocess.run([exe], input=table, capture_output=True, text=True, check=True).stdout
    return [ln.split() for ln in out.splitlines()]


def test_the_header_equals_the_restated_plans(rows):
    assert len(rows) == 3 * len(N_Q) * len(N_T) * len(NUM_CUS)
    seen = set()
    for name, *v in rows:
        n_q, n_t, cus, g, tile, block, grid_x, splits, per = (int(x) for x in v)
        want = PLANS[name](n_q, n_t, cus)
        assert (name, g, tile, block, grid_x, splits, per) == (want.kernel, want.g, want.tile, want.block, want.grid_x, want.splits, want.per), (name, n_q, n_t, cus)
        seen.add((name, n_q, n_t, cus))
    assert len(seen) == len(rows)


def test_the_table_holds_two_tiles_per_split_for_every_shape(rows):
    for name, n_t in TWO_TILES.items():
        hit = [r for r in rows if r[0] == name and (int(r[1]), int(r[2]), int(r[3])) == (B.MULTI_TILE_SOURCES, n_t, CUS)]
        assert len(hit) == 1 and int(hit[0][9]) == 2 * int(hit[0][5]) and int(hit[0][8]) > 1, (name, n_t, hit)
