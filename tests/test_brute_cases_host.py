"""tests/brute_edge_cases.py checked for itself, without a GPU: the restated launch plans against values worked by hand, and the
clouds under oracle.nn -- the ties are ties and the lower row wins, every non-finite target row has a real neighbour in its
step and half-wave, the sizes of the multi-tile cases reach the shape they are meant to reach on 64 to 304 CUs."""
import functools

import numpy as np
import pytest

import brute_edge_cases as B
import oracle


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_restated_plans_equal_values_worked_by_hand():
    # 200 000 x 200 000 on 256 CUs.  valu: 1024 sources a workgroup -> 196; 2048 workgroups wanted -> ceil(2048 / 196) = 11 splits;
    # ceil(200000 / 11) = 18182 -> 18 tiles of 1024 = 18432; ceil(200000 / 18432) = 11.
    assert B.plan_valu(200000, 200000, 256) == B.Plan("valu", 4, 1024, 256, 196, 11, 18432)
    # mfma: 256 sources a workgroup -> 782; 256 * 32 = 8192 wanted -> ceil(8192 / 782) = 11; as above
    assert B.plan_mfma(200000, 200000, 256) == B.Plan("mfma", 2, 1024, 256, 782, 11, 18432)
    # bf16 as shipped: 512 sources a workgroup -> 391; 256 * 32 * 4 / 8 = 4096 wanted -> ceil(4096 / 391) = 11
    assert B.plan_bf16(200000, 200000, 256) == B.Plan("bf16", 2, 1024, 512, 391, 11, 18432)
    # its check shape: 256 sources -> 782; 256 * 32 * 4 / 4 = 8192 -> 11; 18182 -> 36 tiles of 512 = 18432
    assert B.plan_bf16(200000, 200000, 256, check=True) == B.Plan("bf16-check", 2, 512, 256, 782, 11, 18432)
    # 304 CUs: 2432 / 196 -> 13, ceil(200000 / 13) = 15385 -> 16384, ceil(200000 / 16384) = 13; 9728 / 782 -> 13
    assert B.plan_valu(200000, 200000, 304) == B.Plan("valu", 4, 1024, 256, 196, 13, 16384)
    assert B.plan_mfma(200000, 200000, 304) == B.Plan("mfma", 2, 1024, 256, 782, 13, 16384)
    # one source, 8225 targets: as many splits as tiles (9 of 1024, 17 of 512), one tile each
    assert B.plan_bf16(1, 8225, 256) == B.Plan("bf16", 2, 1024, 512, 1, 9, 1024)
    assert B.plan_mfma(1, 8225, 256) == B.Plan("mfma", 2, 1024, 256, 1, 9, 1024)
    assert B.plan_bf16(1, 8225, 256, check=True) == B.Plan("bf16-check", 2, 512, 256, 1, 17, 512)
    assert B.plan_valu(8192, 8225, 256) == B.Plan("valu", 4, 1024, 256, 8, 9, 1024)
    # 65 537 x 64 513: 129 workgroups, ceil(4096 / 129) = 32 splits, ceil(64513 / 32) = 2017 -> 2048: two tiles a split
    assert B.plan_bf16(65537, 64513, 256) == B.Plan("bf16", 2, 1024, 512, 129, 32, 2048)
    # no targets: the plain kernel's plan still names one split of one tile
    assert B.plan_valu(100, 0, 256) == B.Plan("valu", 4, 1024, 256, 1, 1, 1024)


def test_debug_line_round_trip():
    p = B.plan_bf16(33, 8225, 256)
    text = ("[icpgpu] grid n=8192 binned=33 h=0.1 dims=3x3x3 pop=1.0 max=1 attempt=0\n"
            "[icpgpu] brute kernel=bf16 n_q=33 n_s=8192 n_t=8225 num_cus=256 G=2 TILE=1024 BLOCK=512 grid_x=1 splits=9 per=1024 seeded=1\n")
    assert B.parse_lines(text) == [B.line_of(p, 33, 8192, 8225, 256, 1)]
    assert set(B.LINE_FIELDS) | {"kernel"} == set(B.parse_lines(text)[0])


@pytest.mark.parametrize("num_cus", [64, 128, 256, 304])
def test_multi_tile_sizes_reach_their_shape(num_cus):
    for fn in (B.plan_bf16, B.plan_mfma, functools.partial(B.plan_bf16, check=True)):
        tile = fn(1, 1, 1).tile
        for lim in B.MULTI_TILE_LIMS[tile]:
            n_t = B.multi_tile_targets(fn, num_cus, lim)
            p = fn(B.MULTI_TILE_SOURCES, n_t, num_cus)
            assert p.per >= 2 * tile and p.splits >= 3, (num_cus, p)
            assert p.last_tiles(n_t) >= 2 and p.last_lim(n_t) == lim, (num_cus, p, n_t)
            assert B.MULTI_TILE_SOURCES * n_t < 6e9          # (a few 10^9 pairs: milliseconds)


def test_padding_rows_are_spread_not_appended():
    for c in B.source_shape_cases():
        ok = np.isfinite(c.src[:, :3]).all(axis=1)
        n_bad = int((~ok).sum())
        if n_bad >= 2:
            assert not ok[0] and not ok[-1], c.name
        if n_bad >= 260:
            assert not ok[63:8192:64].any() and not ok[64:8192:64].any(), c.name
        if ok.sum() >= 31 and n_bad > 300:     # finite rows in every quarter of the cloud, the last one too
            assert all(q.any() for q in np.array_split(ok, 4)), c.name
    kinds = B.bad_rows(9)[:, :3]
    assert np.isnan(kinds).sum() == 3 and np.isposinf(kinds).sum() == 3 and np.isneginf(kinds).sum() == 3
    assert all((~np.isfinite(kinds[:, a])).sum() == 3 for a in range(3))      # each of NaN, +inf, -inf in x, in y and in z


def test_sizes_and_expected_kernels():
    names = set()
    counts = []
    for group in B.GROUPS.values():
        for c in group():
            assert c.name not in names
            names.add(c.name)
            n_s, n_t = c.src.shape[0], c.tgt.shape[0]
            assert n_s <= 8193 and n_t <= 9217 or c.name.startswith("e: lattice"), c.name
            if n_s < B.MIN_MATRIX or n_t < B.MIN_MATRIX:
                assert not c.matrix, c.name
            assert B.expected_plan(c, 1, 256).kernel == "valu"
            assert B.expected_plan(c, 0, 256).kernel == ("bf16" if c.matrix else "valu")
            assert B.expected_plan(c, 2, 256).kernel == ("mfma" if c.matrix else "valu")
            assert B.expected_plan(c, 0, 256, check=True).kernel == ("bf16-check" if c.matrix else "valu")
            if c.name.startswith("a: ") and c.matrix:
                counts.append(B.finite_rows(c.src))
    assert tuple(counts) == B.SOURCE_COUNTS
    assert [c.tgt.shape[0] for c in B.target_shape_cases(33)] == list(B.TARGET_COUNTS)


def _check_ties(c):
    idx, d2 = oracle.nn(c.src, c.tgt, c.T)
    assert c.ties
    for s, lo, hi in c.ties:
        assert lo < hi and np.array_equal(c.tgt[lo], c.tgt[hi])
        assert idx[s] == lo, (c.name, s, lo, hi, idx[s])
        _, d_lo = oracle.nn(c.src[s:s + 1], c.tgt[lo:lo + 1], c.T)
        _, d_hi = oracle.nn(c.src[s:s + 1], c.tgt[hi:hi + 1], c.T)
        assert _bits(d_lo)[0] == _bits(d_hi)[0] == _bits(d2)[s], (c.name, s)
    return idx


def test_ties_are_ties_and_the_lower_row_is_the_oracles():
    cases = list(B.tie_cases())
    idx = _check_ties(cases[0])
    assert {(lo, hi) for _, lo, hi in cases[0].ties} == {(lo, hi) for _, lo, hi in B.seam_pairs(cases[0].tgt.shape[0])}
    assert np.any(_bits(oracle.nn(cases[0].src, cases[0].tgt, cases[0].T)[1])[[s for s, _, _ in cases[0].ties]] == 0)   # sources exactly on a pair
    idx, _ = oracle.nn(cases[1].src, cases[1].tgt, cases[1].T)
    ok = np.isfinite(cases[1].src[:, :3]).all(axis=1)
    assert (idx[ok] == 0).all() and (idx[~ok] == -1).all()


def test_lattice_shift_leaves_seeds_tied_but_not_lowest():
    c = B.lattice_case()
    old, _ = oracle.nn(c.src, c.tgt, c.T)
    new, d_new = oracle.nn(c.src, c.tgt, B.lattice_shift())
    moved = B.cloud(c.src[:, :3] + B.lattice_shift()[:3, 3])
    d_old = np.array([np.sum((moved[i, :3].astype(np.float64) - c.tgt[old[i], :3]) ** 2) for i in range(len(old))])
    tied_not_lowest = (d_old == d_new.astype(np.float64)) & (old > new)
    assert tied_not_lowest.mean() > 0.9, tied_not_lowest.mean()


def test_every_non_finite_target_row_has_a_neighbour_in_its_step_and_half():
    residues = set()
    for c in B.nonfinite_slot_cases():
        idx, _ = oracle.nn(c.src, c.tgt, c.T)
        assert c.bad
        for row, sources in c.bad:
            assert not np.isfinite(c.tgt[row, :3]).all()
            hit = [s for s in sources if idx[s] // 32 == row // 32 and (idx[s] ^ row) & 4 == 0 and idx[s] != row]
            assert len(hit) >= 1 and len(hit) == len(sources), (c.name, row, len(hit), len(sources))
            assert (row // 32) % 16 != 0
        if "whole tiles" in c.name:
            assert sorted(row % 32 for row, _ in c.bad) == list(range(32))
            assert all(row < 8192 for row, _ in c.bad)
        else:
            assert all(row >= 8192 for row, _ in c.bad)
            residues |= {row % 32 for row, _ in c.bad}
        # nothing but those rows is near the sources: every other target is 50 m away
        near = np.linalg.norm(c.tgt[:, :3], axis=1) < 1.0
        assert near.sum() == sum(len(s) for _, s in c.bad)
    assert residues >= set(range(32)) - {15}, residues
    kinds = np.concatenate([c.tgt[[r for r, _ in c.bad], :3] for c in B.nonfinite_slot_cases()])
    assert np.isnan(kinds).any() and np.isposinf(kinds).any() and np.isneginf(kinds).any()


def test_multi_tile_case_under_the_oracle():
    for fn, lim in ((B.plan_bf16, 33), (functools.partial(B.plan_bf16, check=True), 1)):
        c = B.multi_tile_case(fn, 256, lim)
        n_t = c.tgt.shape[0]
        p = fn(B.MULTI_TILE_SOURCES, n_t, 256)
        idx = _check_ties(c)
        los = {lo for _, lo, _ in c.ties}
        assert los == {p.tile - 1, 7, p.per + 40, 0}
        if lim > 1:
            assert c.tail and (idx[c.tail] >= n_t - lim).all()
        else:
            assert (n_t - 1) in {hi for _, _, hi in c.ties}     # the one row of the last tile: the copy of row 0


def test_degenerate_cases_are_what_they_say():
    cases = {c.name: c for c in B.degenerate_cases()}
    c = cases["f: 512 coincident sources, targets on and beside the centre"]
    idx, d2 = oracle.nn(c.src, c.tgt, c.T)
    ok = np.isfinite(c.src[:, :3]).all(axis=1)
    assert ok.sum() == 512 and (idx[ok] == 40).all() and (d2[ok] == 0).all()
    c = cases["f: 512 coincident sources, nearest targets a hair away"]
    idx, d2 = oracle.nn(c.src, c.tgt, c.T)
    assert (idx[ok] == 41).all() and (d2[ok] > 0).all() and (d2[ok] < 1e-18).all()
    c = cases["f: 512 coincident sources off the origin"]
    idx, d2 = oracle.nn(c.src, c.tgt, c.T)
    ok = np.isfinite(c.src[:, :3]).all(axis=1)
    assert (idx[ok] == 90).all()
    c = cases["f: 4096 coincident sources and 4096 spread"]
    _, counts = np.unique(c.src[:, :3], axis=0, return_counts=True)
    assert counts.max() == 4096
    c = cases["f: 8192 coincident sources (the grid refuses)"]
    assert len(np.unique(c.src, axis=0)) == 1 and not c.matrix
    c = cases["f: every target non-finite but one"]
    idx, _ = oracle.nn(c.src, c.tgt, c.T)
    assert (idx == 4321).all()
    c = cases["f: every target non-finite"]
    idx, _ = oracle.nn(c.src, c.tgt, c.T)
    assert (idx == -1).all()


def test_seeded_subset_and_far_pose():
    cases = list(B.seeded_cases())
    assert len(cases) >= 12
    T0, T3 = B.pose().astype(np.float64), B.far_pose().astype(np.float64)
    assert np.linalg.norm(T3[:3, 3] - T0[:3, 3]) == pytest.approx(5.0, abs=1e-5)
    R = T3[:3, :3] @ T0[:3, :3].T
    assert np.arccos((np.trace(R) - 1) / 2) == pytest.approx(0.5, abs=1e-3)
    assert cases[-1][0].name.startswith("e: lattice") and np.array_equal(cases[-1][1], B.lattice_shift())
