"""The history harness (tests/history_model.py) must be able to SEE a stale cache -- shown here on the host, never with a wrong GPU build
(a stale buffer of another size can fault the device).  `FakeContext` has `Context`'s Python interface; its answers are digests of
exactly the state an observation depends on, read THROUGH caches that mirror the version-keyed structure of
icpslam_amd/csrc/icp_ctx.h (two independent version counters, re-stamping on promote, recognition, adoption).  The very scenarios,
walks and seeds of tests/test_gpu_history.py pass against the correct fake; each injectable fault -- one invalidation skipped -- is
flagged by at least one scenario and one walk seed; and every (mutation, observation) pair of history_model.DEPENDS is exercised."""
import hashlib
import types

import numpy as np
import pytest

import history_model as hm
from icpslam_amd import IcpGpuError, _lib

FAULTS = (
    "normals_kept_across_promote",
    "supplied_normals_kept_across_recognised_set_target",
    "ndt_cells_kept_across_resolution_change",
    "ndt_cells_kept_across_equal_size_target_change",
    "prev_kept_across_target_change",
    "brute_seed_kept_across_set_target_device",
    "old_targets_covariance_grid_taken_for_new_source",
    "adopted_source_from_wrong_filter_result",
    "chain_statistics_kept_after_run_without_chain",
    "map_nn_grid_kept_after_set_target",
)


def D(*parts) -> str:
    h = hashlib.sha256()
    for p in parts:
        h.update(p.tobytes() if isinstance(p, np.ndarray) else repr(p).encode())
        h.update(b"|")
    return h.hexdigest()


def arr(digest, dtype=np.float32, n=8):
    raw = np.frombuffer(hashlib.sha256((digest + str(dtype)).encode()).digest() * 4, np.uint8)[: n * 4].copy()
    return (raw.view(np.uint32) % 1000003).astype(dtype)


def num(digest) -> float:
    return int(digest[:12], 16) / float(1 << 48)


def fake_filter(a, leaf):
    return np.ascontiguousarray(a[:: 2 if leaf == 0.2 else 3], dtype=np.float32).copy()


class Cache:
    """A cached product: the version (and key) it was made for, and what it was made FROM."""

    def __init__(self):
        self.version, self.key, self.content = 0, None, None

    def ok(self, version, key=None):
        return self.version == version and self.version != 0 and self.key == key

    def fill(self, version, content, key=None):
        self.version, self.key, self.content = version, key, content

    def drop(self):
        self.version = 0


class FakeContext:
    def __init__(self, faults=(), registry=None):
        self.faults = frozenset(faults)
        self.registry = registry if registry is not None else {}
        self.p = dict(method=0, max_iterations=10, transformation_epsilon=1e-6, max_correspondence_distance=1.0, euclidean_fitness_epsilon=-1.0,
                      min_correspondences=3, force_iterations=0, nn_mode=0, brute_variant=0, gicp_inner=0)
        self.ndt_p, self.ls, self.chain = (1.0, 0.1, 0.55), 0, []
        self.src = self.tgt = None                   # content digests
        self.src_ext = self.tgt_ext = False
        self.n_source = self.n_target = 0
        self.src_version = self.tgt_version = 1      # two independent sequences that both start at 1
        self.grid, self.src_grid = Cache(), Cache()
        self.grid_uniq = False
        self.prev, self.seed = Cache(), Cache()
        self.cov_src, self.cov_tgt, self.cov_grid_src, self.cov_grid_tgt = Cache(), Cache(), Cache(), Cache()
        self.nrm_src, self.nrm_tgt, self.nrm_user, self.nrm_supplied = Cache(), Cache(), None, False
        self.cells = Cache()
        self.vox_fp, self.vox_content, self.vox_n = None, None, 0
        self.stats_n, self.stats = 0, ""
        self.final = None
        self.keys = None
        self.last_ndt = ""
        self.map_res, self.map_mode, self.map_ins = None, False, []
        self.prof = types.SimpleNamespace(sources_adopted=0, targets_recognised=0)

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def _need(self, src=False, tgt=False):
        if (src and self.src is None) or (tgt and self.tgt is None):
            raise IcpGpuError(_lib.ERR_NO_INPUT, "cloud not set")

    # parameters
    def default_params(self):
        return types.SimpleNamespace(**FakeContext().p)

    def get_params(self):
        return types.SimpleNamespace(**self.p)

    def set_params(self, p=None, **kw):
        new = dict(vars(p)) if p is not None else dict(self.p)
        new.update(kw)
        self.p = new

    def set_ndt_params(self, resolution=1.0, step_size=0.1, outlier_ratio=0.55, line_search=None):
        self.ndt_p = (float(resolution), float(step_size), float(outlier_ratio))

    def set_ndt_line_search(self, mode):
        self.ls = int(mode)

    def set_correspondence_rejectors(self, chain=()):
        self.chain = [tuple(r) for r in chain]

    def profile(self):
        return types.SimpleNamespace(**vars(self.prof))

    # clouds
    def set_source(self, a):
        a = np.ascontiguousarray(a, np.float32)
        fp = D(a)
        self.src_version += 1
        self.src_ext = False
        if self.vox_fp is not None and fp == self.vox_fp and a.shape[0] > 0:
            self.src = self.vox_content              # the device copy of the filter's result
            self.prof.sources_adopted += 1
        else:
            self.src = fp
        self.n_source = a.shape[0]

    def _target_uploaded(self):
        old = self.tgt_version
        self.tgt_version += 1
        if "prev_kept_across_target_change" in self.faults and self.prev.version == old:
            self.prev.version = self.tgt_version
        if "map_nn_grid_kept_after_set_target" in self.faults and self.grid_uniq and self.grid.version == old:
            self.grid.version = self.tgt_version

    def set_target(self, a):
        a = np.ascontiguousarray(a, np.float32)
        fp = D(a)
        recognised = self.tgt is not None and not self.tgt_ext and fp == self.tgt and a.shape[0] > 0
        if not (recognised and "supplied_normals_kept_across_recognised_set_target" in self.faults):
            self.nrm_supplied = False
        if recognised:
            self.prof.targets_recognised += 1
            return
        if self.src is not None and not self.src_ext and fp == self.src and a.shape[0] > 0:
            self.prof.targets_recognised += 1
            n = self.n_source
            self._promote()
            self.src, self.n_source, self.src_ext = self.tgt, n, False     # put back as a copy; its caches moved on with the target
            return
        self._target_uploaded()
        self.tgt, self.tgt_ext, self.n_target = fp, False, a.shape[0]

    def set_source_device(self, ptr, n):
        self.src_version += 1
        self.src, self.src_ext, self.n_source = D(self.registry[ptr]), True, n

    def set_target_device(self, ptr, n):
        self.nrm_supplied = False
        old = self.tgt_version
        self._target_uploaded()
        if "brute_seed_kept_across_set_target_device" in self.faults and self.seed.version == old:
            self.seed.version = self.tgt_version
        self.tgt, self.tgt_ext, self.n_target = D(self.registry[ptr]), True, n

    def promote_source_to_target(self):
        self._promote()

    def _promote(self):                              # promote_internal, cache by cache
        if self.src is None:
            raise IcpGpuError(_lib.ERR_NO_INPUT, "no source")
        self.nrm_supplied = False
        old_sv, old_tv = self.src_version, self.tgt_version
        self.src, self.tgt = self.tgt, self.src
        self.src_ext, self.tgt_ext = self.tgt_ext, self.src_ext
        self.cov_src, self.cov_tgt = self.cov_tgt, self.cov_src
        self.cov_grid_src, self.cov_grid_tgt = self.cov_grid_tgt, self.cov_grid_src
        self.grid, self.src_grid = self.src_grid, self.grid
        self.grid_uniq = False
        self.tgt_version += 1
        for c in (self.grid, self.cov_tgt, self.cov_grid_tgt):   # what followed the cloud is re-stamped for its new counter
            if c.version == old_sv and c.version != 0:
                c.version = self.tgt_version
            else:
                c.drop()
        self.src_grid.drop()
        self.cov_src.drop()
        if "old_targets_covariance_grid_taken_for_new_source" not in self.faults:
            self.cov_grid_src.drop()
        if "normals_kept_across_promote" in self.faults and self.nrm_tgt.version == old_tv:
            self.nrm_tgt.version = self.tgt_version
        self.src_version += 1
        self.n_target, self.n_source = self.n_source, 0
        self.src, self.src_ext = None, False
        self.final = None

    # the voxel filter
    def voxel_grid(self, a, leaf):
        out = fake_filter(a, leaf)
        if not ("adopted_source_from_wrong_filter_result" in self.faults and self.vox_fp is not None):
            self.vox_fp = D(out)
        self.vox_content, self.vox_n = D(out), out.shape[0]
        return out

    voxel_grid_view = voxel_grid

    def set_source_voxel_filtered(self, a, leaf):
        out = fake_filter(a, leaf)
        self.src_version += 1
        self.src, self.src_ext, self.n_source = D(out), False, out.shape[0]
        return self.n_source

    # caches
    def _gate(self):
        return self.p["max_correspondence_distance"]

    def _grid(self):
        if not self.grid.ok(self.tgt_version, self._gate()):
            self.grid.fill(self.tgt_version, self.tgt, self._gate())
            self.grid_uniq = False
        return self.grid.content

    def _search(self, fresh_bounds=False):
        """What a correspondence search reads: the grid (or the cloud), and the last sweep's bounds when they are this pair's."""
        brute = self.p["nn_mode"] == _lib.NN_BRUTE
        field = self.tgt if brute else self._grid()
        bound = self.seed if brute else self.prev
        if fresh_bounds:
            bound.drop()
        key = self.src_version
        used = bound.content if bound.ok(self.tgt_version, key) else self.tgt
        bound.fill(self.tgt_version, self.tgt, key)
        return D(field, used, self.p["brute_variant"] if brute else 0)

    def _covariances(self, of_target):
        cloud, version = (self.tgt, self.tgt_version) if of_target else (self.src, self.src_version)
        cov, grid = (self.cov_tgt, self.cov_grid_tgt) if of_target else (self.cov_src, self.cov_grid_src)
        if not cov.ok(version):
            if not grid.ok(version):
                grid.fill(version, cloud)
            cov.fill(version, D("cov", cloud, grid.content))
        return cov.content

    def _normals(self, of_target):
        if of_target and self.nrm_supplied:
            return self.nrm_user
        cloud, version = (self.tgt, self.tgt_version) if of_target else (self.src, self.src_version)
        c = self.nrm_tgt if of_target else self.nrm_src
        if not c.ok(version):
            c.fill(version, D("normals", cloud))
        return c.content

    def _cells(self):
        res = self.ndt_p[0]
        if "ndt_cells_kept_across_resolution_change" in self.faults:
            ok = self.cells.version == self.tgt_version and self.cells.version != 0
        elif "ndt_cells_kept_across_equal_size_target_change" in self.faults:
            ok = self.cells.key == (res, self.n_target)
        else:
            ok = self.cells.ok(self.tgt_version, (res, self.n_target))
        if not ok:
            self.cells.fill(self.tgt_version, D("cells", self.tgt, res), (res, self.n_target))
        return self.cells.content

    # the hot path
    def align(self, guess=None, want_cloud=False, want_fitness=False):
        self._need(src=True, tgt=True)
        m, p = self.p["method"], self.p
        g = None if guess is None else np.asarray(guess, np.float32)
        base = [m, p["max_iterations"], self._gate(), self.src, g]
        if m in (hm.P2P, hm.P2PLANE):
            base += [self._search(fresh_bounds=True), self.chain] + ([self._normals(True)] if m == hm.P2PLANE else [])
        elif m == hm.GICP:
            base += [self._search(fresh_bounds=True), self._covariances(False), self._covariances(True), p["gicp_inner"]]
        else:
            base += [self._cells(), self.ndt_p, self.ls]
            self.prev.drop()
        d = D(*base)
        if m in (hm.P2P, hm.P2PLANE) and (self.chain or "chain_statistics_kept_after_run_without_chain" not in self.faults):
            self.stats_n, self.stats = len(self.chain), D("stats", d)
        if m == hm.NDT:
            self.last_ndt = d
        self.final = d
        self.keys = d
        fit = num(D("fit", d, self.tgt)) if want_fitness else float("nan")
        return dict(T=arr(d, n=16).reshape(4, 4), converged=True, iterations=int(d[:2], 16), state=1, n_corr=int(d[2:6], 16), mse=num(d),
                    fitness=fit, cloud=arr(D("cloud", d)))

    def align_view(self, guess=None, want_fitness=False):
        return self.align(guess, True, want_fitness)

    def fitness(self, max_range=1e308):
        self._need(src=True, tgt=True)
        return num(D("fitness", self.final, self.src, self._grid(), max_range))

    def align_batch(self, sources, targets, want_fitness=False):
        return [dict(T=arr(D("batch", s, t, self.p["method"], self.p["max_iterations"]), n=16), converged=True, iterations=1, state=1,
                     n_corr=1, mse=0.0) for s, t in zip(sources, targets)]

    def nn(self, T=np.eye(4)):
        self._need(src=True, tgt=True)
        d = D("nn", self.src, self._search(), np.asarray(T, np.float32))
        self.keys = d
        return arr(d, np.int32), arr(D(d, "d2"))

    def correspondences(self, T=np.eye(4)):
        self._need(src=True, tgt=True)
        d = D("corr", self.src, self._search(fresh_bounds=True), np.asarray(T, np.float32), self._gate(), self.chain)
        self.keys = d
        self.stats_n, self.stats = len(self.chain), D("stats", d)
        return arr(d, np.int32), arr(D(d, "d2"))

    def rejector_stats(self):
        return [dict(pairs_in=int(D(self.stats, s)[:6], 16), pairs_out=int(D(self.stats, s)[6:12], 16), cut=np.float32(num(D(self.stats, s))))
                for s in range(self.stats_n)]

    def reduce(self, T, max_dist):
        return arr(D("reduce", self.keys, self.src, self.tgt, np.asarray(T, np.float32), max_dist), np.float64, 17)

    def reduce_point_to_plane(self, T, max_dist):
        return arr(D("reduce29", self.keys, self.src, self.tgt, self._normals(True), np.asarray(T, np.float32), max_dist), np.float64, 29)

    def transform(self, T):
        self._need(src=True)
        return arr(D("transform", self.src, np.asarray(T, np.float32)))

    def set_target_normals(self, normals):
        self._need(tgt=True)
        if np.asarray(normals).shape[0] != self.n_target:
            raise IcpGpuError(_lib.ERR_INVALID_ARG, "normals of another size")
        self.nrm_user, self.nrm_supplied = D(np.ascontiguousarray(normals, np.float32)), True

    def normals(self, of_target=True):
        self._need(src=not of_target, tgt=bool(of_target))
        return arr(self._normals(of_target))

    def gicp_covariances(self, of_target=False):
        self._need(src=not of_target, tgt=bool(of_target))
        return arr(self._covariances(of_target), np.float64)

    def ndt_cells(self):
        self._need(tgt=True)
        d = self._cells()
        return dict(centroid=arr(d), mean=arr(D(d, 1), np.float64), icov=arr(D(d, 2), np.float64), n_points=arr(D(d, 3), np.int32))

    def ndt_derivatives(self, p):
        self._need(src=True, tgt=True)
        return arr(D("ndt29", self.src, self._cells(), tuple(p), self.ndt_p[2]), np.float64, 29)

    def ndt_gradient(self, p):
        return self.ndt_derivatives(p)[:8].copy()

    def ndt_transformation_probability(self):
        return num(D("prob", self.last_ndt))

    def ndt_line_search_trace(self):
        d = D("trace", self.last_ndt, self.ls)
        return dict(iteration=arr(d, np.int32, 2 * self.ls), step=arr(D(d, 1), np.float64, 2 * self.ls), phi=arr(D(d, 2), np.float64, 2 * self.ls),
                    d_phi=arr(D(d, 3), np.float64, 2 * self.ls))

    # the map
    def map_reset(self, resolution=0.5):
        self.map_res, self.map_ins = float(resolution), []

    def map_set_search(self, approx):
        self.map_mode = bool(approx)

    def map_add_points(self, a, pose=None):
        self.map_ins.append((D(np.ascontiguousarray(a, np.float32)), None if pose is None else D(np.asarray(pose, np.float32))))
        return 1

    def map_add_source(self, pose=None):
        self._need(src=True)
        self.map_ins.append((self.src, None if pose is None else D(np.asarray(pose, np.float32))))
        return 1

    def map_nn_target(self, pose, pose_inv, want_cloud=True):
        self._need(src=True)
        d = D("map_nn", self.map_res, self.map_mode, self.map_ins, self.src, np.asarray(pose, np.float32))
        out = np.random.default_rng(int(d[:16], 16)).random((self.n_source, 4), np.float32)
        self.nrm_supplied = False
        self.tgt_version += 1
        self.tgt, self.tgt_ext, self.n_target = D(out), False, out.shape[0]
        self.final = None
        if self.p["nn_mode"] != _lib.NN_BRUTE:       # the grid of the coming alignment, built from the nn cloud's distinct points
            self.grid.fill(self.tgt_version, self.tgt, self._gate())
            self.grid_uniq = True
        return out


class FakeBackend:
    def __init__(self, faults=()):
        self.faults = tuple(faults)
        self.registry = {}

    def new_context(self):
        return FakeContext(self.faults, self.registry)

    def device(self, a):
        ptr = 0x1000 + 16 * len(self.registry)
        self.registry[ptr] = np.array(a, copy=True)
        return ptr, None

    def filtered(self, spec, leaf):
        return fake_filter(hm.cloud(spec), leaf)


@pytest.fixture(autouse=True)
def small_clouds(monkeypatch):
    """The fake digests bytes: the operation lists stay the committed ones, the clouds behind their names are 1/50 of the size."""
    def tiny(spec):
        kind, n, seed = spec
        rng = np.random.default_rng((n, seed, kind == "src"))
        return rng.normal(size=(max(40, n // 50), 4)).astype(np.float32)
    cache = {}
    monkeypatch.setattr(hm, "cloud", lambda spec: cache.setdefault(spec, tiny(spec)))


def run(ops, faults=(), seed=None):
    with hm.Walk(FakeBackend(faults), seed=seed) as w:
        w.run(ops)
        return w.n_obs


def flagged(ops, fault) -> bool:
    try:
        run(ops, (fault,))
    except hm.HistoryDivergence:
        return True
    return False


ALL_SEEDS = hm.WALK_SEEDS + hm.LARGE_WALK_SEEDS


@pytest.mark.parametrize("name", sorted(hm.SCENARIOS))
def test_scenarios_pass_against_the_correct_fake(name):
    assert run(hm.SCENARIOS[name]()) >= 5


@pytest.mark.parametrize("seed", ALL_SEEDS)
def test_walks_pass_against_the_correct_fake(seed):
    assert run(hm.gen_walk(seed), seed=seed) >= 3


def test_walks_are_deterministic_lists_of_literals():
    for seed in ALL_SEEDS:
        ops = hm.gen_walk(seed)
        assert ops == hm.gen_walk(seed) and eval(repr(ops)) == ops      # a failure's log can be pasted back


@pytest.mark.parametrize("fault", FAULTS)
def test_every_fault_is_flagged_by_a_scenario_and_by_a_walk(fault):
    by_scenario = [n for n in sorted(hm.SCENARIOS) if flagged(hm.SCENARIOS[n](), fault)]
    by_walk = [s for s in ALL_SEEDS if flagged(hm.gen_walk(s), fault)]
    print(fault, by_scenario, by_walk)
    assert by_scenario and by_walk, (fault, by_scenario, by_walk)


def test_a_failure_names_the_seed_the_observation_and_a_replayable_log():
    fault, ops = "ndt_cells_kept_across_resolution_change", hm.SCENARIOS["ndt_cells"]()
    with pytest.raises(hm.HistoryDivergence) as e:
        run(ops, (fault,), seed=4711)
    text = str(e.value)
    assert "seed = 4711" in text and "first diverging observation = #" in text
    log = eval(text.split("log = ", 1)[1])
    assert log == ops[: len(log)] and log[-1][0] == "obs"              # stopped AT the divergence, nothing ran after it
    assert flagged(log, fault) and not flagged(log[:-1], fault)


def test_an_error_of_the_library_stops_the_walk_at_once():
    class Dies(FakeContext):
        def nn(self, T=np.eye(4)):
            raise IcpGpuError(_lib.ERR_HIP, "wait for the device timed out")
    b = FakeBackend()
    b.new_context = lambda: Dies((), b.registry)
    ops = [("set_target", hm.B), ("set_source", hm.A), hm.OBS("nn"), hm.OBS("align")]
    with pytest.raises(hm.HistoryDivergence, match="IcpGpuError -3") as e:
        hm.Walk(b).run(ops)
    assert "('obs', 'align'" not in str(e.value)


def greedy_seed_cover(candidates=range(100, 400)):
    """How history_model.WALK_SEEDS was chosen, to be run again (inside the `small_clouds` fixture's patch, as the test below does)
    after a change to the vocabulary, to gen_walk or to the faults: beside the large walks, the fewest small-walk seeds found
    greedily that together flag every fault and exercise every pair of DEPENDS.  Returns (seeds, what no candidate reaches)."""
    want = {(m, o) for o, ms in hm.DEPENDS.items() for m in ms}

    def reach(seed):
        ops = hm.gen_walk(seed, large=seed in hm.LARGE_WALK_SEEDS)
        run(ops, seed=seed)                                    # (a candidate must pass against the correct fake)
        return (hm.covered_pairs([ops]) & want) | {f for f in FAULTS if flagged(ops, f)}

    have = set().union(*[reach(s) for s in hm.LARGE_WALK_SEEDS])
    reached = {s: reach(s) for s in candidates}
    chosen, todo = [], (want | set(FAULTS)) - have
    while todo:
        best = max(reached, key=lambda s: len(reached[s] & todo))
        if not reached[best] & todo:
            break
        chosen.append(best)
        todo -= reached[best]
    return tuple(sorted(chosen)), todo


def test_the_committed_seeds_are_what_the_greedy_cover_gives():
    seeds, unreached = greedy_seed_cover()
    assert not unreached and seeds == hm.WALK_SEEDS, (seeds, unreached)


def test_every_dependence_pair_is_exercised_by_the_committed_walks():
    seen = hm.covered_pairs([hm.gen_walk(s) for s in ALL_SEEDS])
    want = {(m, o) for o, ms in hm.DEPENDS.items() for m in ms}
    missing = sorted(want - seen)
    assert not missing, missing


def test_the_fitness_rule_is_the_documented_one():
    got, want = dict(fitness=1.0 + 2e-13, T=np.eye(4)), dict(fitness=1.0, T=np.eye(4))
    assert hm.differences(got, want, n_source=99999) == ["fitness"]          # bit for bit below 100k source points
    assert hm.differences(got, want, n_source=100000) == []                  # 1e-12 relative from there on
    assert hm.differences(dict(got, fitness=1.0 + 2e-12), want, n_source=100000) == ["fitness"]
    assert hm.differences(dict(got, T=np.eye(4) + 1e-7), want, n_source=100000) == ["T"]
    assert hm.FITNESS_RTOL == 1e-12 and hm.ORDERED_SOURCE_MIN == 100000
