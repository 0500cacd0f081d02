"""History independence of a context ("History independence"): an operation vocabulary over `Context`, a model of
what a context LOGICALLY holds according to include/icpgpu.h, and the check -- whatever a context did before, an observation
returns what a new context returns that was given only the model's state by the shortest call sequence.

Not a conftest: a helper the GPU test (tests/test_gpu_history.py, real contexts) and the host test
(tests/test_history_model_host.py, a fake context with injectable stale caches) both drive with the SAME scenarios, walks and seeds.

An operation is a tuple (name, *args) of Python literals; clouds are named by generator and seed, never dumped:
    ("src" | "tgt", n, seed)    synth.make_pair(n, n, seed)[0 | 1]
so that a failing log can be pasted into `Walk(backend).run(log)`.
"""
from __future__ import annotations

import functools
import pprint

import numpy as np

from icpslam_amd import IcpGpuError, _lib, synth

P2P, GICP, P2PLANE, NDT = _lib.P2P_SVD, _lib.GICP, _lib.P2PLANE, _lib.NDT
METHOD_TAG = {P2P: "p2p", GICP: "gicp", P2PLANE: "p2plane", NDT: "ndt"}
ORDERED_SOURCE_MIN = 100000      # from here on the source is searched in cell order (atomic ranks inside a cell): `fitness` may move
FITNESS_RTOL = 1e-12             # ... in its last bit from run to run -- the bound tests/test_gpu_recognition.py uses for it
FITNESS_KEYS = ("fitness", "fitness_again")
DEFAULT_NDT = (1.0, 0.1, 0.55)


@functools.lru_cache(maxsize=24)
def _pair(n, seed):
    s, t, _ = synth.make_pair(n, n, seed=seed)
    s.setflags(write=False)
    t.setflags(write=False)
    return s, t


def cloud(spec) -> np.ndarray:
    kind, n, seed = spec
    return _pair(n, seed)[0 if kind == "src" else 1]


def variant(a: np.ndarray, kind: str) -> np.ndarray:
    """The recognition's near misses (tests/test_gpu_recognition.py): the same bytes in a new buffer, one bit flipped in a point the
    256-point sample holds (n / 2) or in one only the full fingerprint sees (n / 2 + 1), one point fewer."""
    a = np.array(a, dtype=np.float32, copy=True)
    n = a.shape[0]
    if kind == "flip_in":
        a.view(np.uint32)[n // 2, 1] ^= 1
    elif kind == "flip_out":
        a.view(np.uint32)[n // 2 + 1, 2] ^= 1
    elif kind == "short":
        a = a[:-1].copy()
    elif kind != "same":
        raise ValueError(kind)
    return a


def pose(p6) -> np.ndarray:
    return np.eye(4) if p6 is None else synth.pose_matrix(*p6)


def unit_normals(n, seed) -> np.ndarray:
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    out = np.zeros((n, 4), np.float32)
    out[:, :3] = v.astype(np.float32)
    return out


class Model:
    """What the context logically holds, by the contracts of include/icpgpu.h -- no caches, no versions."""

    def __init__(self):
        self.source = None
        self.target = None
        self.normals = None            # the caller's target normals
        self.params = {}               # icpgpu_params fields that differ from icpgpu_default_params
        self.ndt = DEFAULT_NDT
        self.line_search = 0
        self.chain = []
        self.map_resolution = None
        self.map_search = False
        self.map_insertions = []       # (cloud, pose 6-tuple or None), in order

    @property
    def method(self):
        return self.params.get("method", P2P)

    # the contracts, as icpgpu.h words them
    def set_target(self, a):           # "in force until the target changes (icpgpu_set_target -- recognised or not -- ...)"
        self.target = a
        self.normals = None

    def set_source(self, a):
        self.source = a

    def promote(self):                 # "make the current source the next target"; the source is unset afterwards
        self.target, self.source, self.normals = self.source, None, None


class HistoryDivergence(AssertionError):
    pass


# ---- observations ---------------------------------------------------------------------------------------------------------------
def _stats(ctx):
    st = ctx.rejector_stats()
    return dict(stats_n=len(st), stats_in=np.array([s["pairs_in"] for s in st], np.uint32),
                stats_out=np.array([s["pairs_out"] for s in st], np.uint32), stats_cut=np.array([s["cut"] for s in st], np.float32))


def _align(ctx, a):
    g = None if a.get("guess") is None else pose(a["guess"])
    if a.get("view"):
        r = ctx.align_view(guess=g, want_fitness=bool(a.get("fitness")))
    else:
        r = ctx.align(guess=g, want_cloud=True, want_fitness=bool(a.get("fitness")))
    out = {k: r[k] for k in ("T", "converged", "iterations", "state", "n_corr", "mse", "fitness", "cloud")}
    method = ctx.get_params().method
    if method in (P2P, P2PLANE):
        out.update(_stats(ctx))
    if method == NDT:
        out["ndt_probability"] = ctx.ndt_transformation_probability()
        out.update({"trace_" + k: v for k, v in ctx.ndt_line_search_trace().items()})
    return out


def observe(ctx, kind, a):
    """One self-contained observation on a context whose logical state is in place -> {name: array or scalar}."""
    if kind == "align":
        return _align(ctx, a)
    if kind == "align_fitness":       # icpgpu_fitness reads the last alignment's transform: observed together with it
        out = _align(ctx, a)
        out["fitness_again"] = ctx.fitness(a["max_range"]) if "max_range" in a else ctx.fitness()
        return out
    if kind == "align_corr":          # icpgpu_correspondences right after an alignment, whose neighbour bounds are still there
        out = _align(ctx, a)
        out["idx"], out["d2"] = ctx.correspondences(out["T"])
        out.update({"after_" + k: v for k, v in _stats(ctx).items()})
        return out
    if kind == "nn":
        idx, d2 = ctx.nn(pose(a.get("T")))
        return dict(idx=idx, d2=d2)
    if kind == "nn_reduce":
        T = pose(a.get("T"))
        idx, d2 = ctx.nn(T)
        return dict(idx=idx, d2=d2, sums=ctx.reduce(T, a["max_dist"]))
    if kind == "nn_reduce_p2plane":
        T = pose(a.get("T"))
        idx, d2 = ctx.nn(T)
        return dict(idx=idx, d2=d2, sums=ctx.reduce_point_to_plane(T, a["max_dist"]))
    if kind == "corr":
        idx, d2 = ctx.correspondences(pose(a.get("T")))
        return dict(idx=idx, d2=d2, **_stats(ctx))
    if kind == "normals":
        return dict(normals=ctx.normals(of_target=bool(a["of_target"])))
    if kind == "cov":
        return dict(cov=ctx.gicp_covariances(of_target=bool(a["of_target"])))
    if kind == "ndt_cells":
        return dict(ctx.ndt_cells())
    if kind == "ndt_derivatives":
        return dict(sums=ctx.ndt_derivatives(a["p"]))
    if kind == "ndt_gradient":
        return dict(sums=ctx.ndt_gradient(a["p"]))
    if kind == "transform":
        return dict(cloud=ctx.transform(pose(a.get("T"))))
    if kind == "align_batch":
        s, t = cloud(("src", a["n"], a["seed"])), cloud(("tgt", a["n"], a["seed"]))
        rs = ctx.align_batch([s] * a["k"], [t] * a["k"], want_fitness=False)
        return {f"{k}{i}": r[k] for i, r in enumerate(rs) for k in ("T", "converged", "iterations", "state", "n_corr", "mse")}
    if kind == "map_nn_target":
        P = pose(a.get("pose"))
        return dict(nn_cloud=ctx.map_nn_target(P, np.linalg.inv(P)))
    raise ValueError(kind)


def setup_fresh(ctx, model, with_map=False):
    """The model's logical state into a new context by the shortest call sequence: params, target, normals, source, chain."""
    ctx.set_params(ctx.default_params(), **model.params)
    if model.ndt != DEFAULT_NDT:
        ctx.set_ndt_params(*model.ndt)
    if model.line_search:
        ctx.set_ndt_line_search(model.line_search)
    if model.target is not None:
        ctx.set_target(model.target)
    if model.normals is not None:
        ctx.set_target_normals(model.normals)
    if model.source is not None:
        ctx.set_source(model.source)
    if model.chain:
        ctx.set_correspondence_rejectors(model.chain)
    if with_map:
        ctx.map_reset(model.map_resolution)
        if model.map_search:
            ctx.map_set_search(True)
        for c, p6 in model.map_insertions:
            ctx.map_add_points(c, None if p6 is None else pose(p6))


def replay_fresh(backend, model, kind, a):
    with backend.new_context() as f:
        setup_fresh(f, model, with_map=kind == "map_nn_target")
        return observe(f, kind, a)


def _bits(v):
    if isinstance(v, np.ndarray):
        return (v.dtype.str, v.shape, v.tobytes())
    if isinstance(v, (float, np.floating)):
        return np.float64(v).tobytes()
    return v


def differences(got, want, n_source):
    """Names whose values differ: bit for bit, but `fitness` of a source of >= ORDERED_SOURCE_MIN points at FITNESS_RTOL."""
    bad = [k for k in sorted(set(got) | set(want)) if k not in got or k not in want]
    for k in sorted(set(got) & set(want)):
        if k in FITNESS_KEYS and n_source >= ORDERED_SOURCE_MIN:
            g, w = float(got[k]), float(want[k])
            if not (abs(g - w) <= FITNESS_RTOL * abs(w) or (np.isnan(g) and np.isnan(w))):
                bad.append(k)
        elif _bits(got[k]) != _bits(want[k]):
            bad.append(k)
    return bad


# ---- the walk: every operation goes to a live context and to the model together --------------------------------------------------
class Walk:
    def __init__(self, backend, seed=None):
        self.b = backend
        self.seed = seed
        self.ctx = backend.new_context()
        self.model = Model()
        self.log = []
        self.n_obs = 0
        self.slots = {}
        self._keep = []                # device buffers the context refers to (zero copy: must stay alive)

    def close(self):
        self.ctx.close()
        self._keep = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def fail(self, what):
        raise HistoryDivergence(f"{what}\nseed = {self.seed!r}; first diverging observation = #{self.n_obs} (operation {len(self.log) - 1})\n"
                                f"log = {pprint.pformat(self.log, width=150)}")

    def run(self, ops):
        for op in ops:
            self.step(op)
        return self

    def step(self, op):
        self.log.append(op)
        try:
            getattr(self, "op_" + op[0])(*op[1:])
        except IcpGpuError as e:       # (a HIP or timeout code included: the walk stops here, nothing more is started)
            self.fail(f"IcpGpuError {e.code}: {e}")

    # clouds
    def op_set_source(self, spec):
        a = cloud(spec)
        self.ctx.set_source(a)
        self.model.set_source(a)

    def _set_target(self, a, expect, what):
        """expect: None, "recognised" or "upload" -- the path icpgpu_set_target took, read from profile().targets_recognised."""
        before = self.ctx.profile().targets_recognised
        self.ctx.set_target(a)
        moved = self.ctx.profile().targets_recognised - before
        if expect is not None and moved != (1 if expect == "recognised" else 0):
            self.fail(f"{what}: expected {expect}, targets_recognised moved by {moved}")
        self.model.set_target(a)

    def op_set_target(self, spec, expect=None):
        self._set_target(cloud(spec), expect, f"set_target {spec}")

    def op_set_target_variant(self, kind, expect=None):     # of the CURRENT target: "same" is the rejected scan's unchanged target
        self._set_target(variant(self.model.target, kind), expect, f"set_target of the current target's bytes ({kind})")

    def op_set_target_from_source(self, expect=None):       # the odometer's `*prev_cloud_ = *curr_cloud_`: the promote path inside set_target
        self._set_target(variant(self.model.source, "same"), expect, "set_target of the current source's bytes")   # (the source stays set)

    def op_set_source_variant(self, kind):
        a = variant(self.model.source, kind)
        self.ctx.set_source(a)
        self.model.set_source(a)

    def op_set_source_device(self, spec):
        a = cloud(spec)
        ptr, keep = self.b.device(a)
        self._keep.append(keep)
        self.ctx.set_source_device(ptr, a.shape[0])
        self.model.set_source(a)

    def op_set_target_device(self, spec):
        a = cloud(spec)
        ptr, keep = self.b.device(a)
        self._keep.append(keep)
        self.ctx.set_target_device(ptr, a.shape[0])
        self.model.set_target(a)

    def op_promote(self):
        self.ctx.promote_source_to_target()
        self.model.promote()

    # the voxel filter and the adoption of its result
    def op_voxel_grid(self, spec, leaf, slot, view=False):
        a = cloud(spec)
        got = self.ctx.voxel_grid_view(a, leaf) if view else self.ctx.voxel_grid(a, leaf)
        want = self.b.filtered(spec, leaf)
        if _bits(got) != _bits(want):
            self.fail(f"voxel_grid{'_view' if view else ''}: not a new context's result")
        self.slots[slot] = got

    def op_set_source_slot(self, slot, kind="same", expect=None):
        a = variant(self.slots[slot], kind)
        before = self.ctx.profile().sources_adopted
        self.ctx.set_source(a)
        adopted = self.ctx.profile().sources_adopted - before
        if expect is not None and adopted != (1 if expect == "adopt" else 0):
            self.fail(f"set_source of filter result {slot!r} ({kind}): expected {expect}, sources_adopted moved by {adopted}")
        self.model.set_source(a)

    def op_set_source_voxel_filtered(self, spec, leaf):
        n = self.ctx.set_source_voxel_filtered(cloud(spec), leaf)
        a = self.b.filtered(spec, leaf)
        if n != a.shape[0]:
            self.fail("set_source_voxel_filtered: not a new context's point count")
        self.model.set_source(a)

    # parameters
    def op_set_target_normals(self, seed):
        nrm = unit_normals(self.model.target.shape[0], seed)
        self.ctx.set_target_normals(nrm)
        self.model.normals = nrm

    def op_set_params(self, kw):
        self.ctx.set_params(**kw)
        self.model.params.update(kw)

    def op_set_ndt_params(self, resolution, step_size, outlier_ratio):
        self.ctx.set_ndt_params(resolution, step_size, outlier_ratio)
        self.model.ndt = (resolution, step_size, outlier_ratio)

    def op_set_ndt_line_search(self, mode):
        self.ctx.set_ndt_line_search(mode)
        self.model.line_search = mode

    def op_set_rejectors(self, chain):
        self.ctx.set_correspondence_rejectors(chain)
        self.model.chain = [tuple(r) for r in chain]

    # the map
    def op_map_reset(self, resolution):
        self.ctx.map_reset(resolution)
        self.model.map_resolution, self.model.map_insertions = resolution, []

    def op_map_set_search(self, approx):
        self.ctx.map_set_search(approx)
        self.model.map_search = bool(approx)

    def op_map_add_points(self, spec, p6=None):
        self.ctx.map_add_points(cloud(spec), None if p6 is None else pose(p6))
        self.model.map_insertions.append((cloud(spec), p6))

    def op_map_add_source(self, p6=None):
        self.ctx.map_add_source(None if p6 is None else pose(p6))
        self.model.map_insertions.append((self.model.source, p6))

    def op_map_nn_target(self, p6=None):       # a mutation AND an observation: the nn cloud becomes the target
        got = self.op_obs("map_nn_target", dict(pose=p6))
        self.model.set_target(got["nn_cloud"])

    # observations
    def op_obs(self, kind, a=None):
        a = a or {}
        n_source = 0 if self.model.source is None else self.model.source.shape[0]
        got = observe(self.ctx, kind, a)
        want = replay_fresh(self.b, self.model, kind, a)
        bad = differences(got, want, n_source)
        if bad:
            self.fail(f"observation {kind} {a}: {bad} differ from a new context's")
        self.n_obs += 1
        return got


class GpuBackend:
    """Real contexts; device buffers are torch tensors."""

    def __init__(self):
        self._filtered = {}

    def new_context(self):
        from icpslam_amd import Context
        return Context(0)

    def device(self, a):
        import torch
        t = torch.from_numpy(np.array(a, dtype=np.float32, copy=True)).to("cuda")
        torch.cuda.synchronize()
        return t.data_ptr(), t

    def filtered(self, spec, leaf):            # the voxel filter's result as a context WITHOUT history gives it
        key = (spec, leaf)
        if key not in self._filtered:
            with self.new_context() as f:
                self._filtered[key] = f.voxel_grid(cloud(spec), leaf)
        return self._filtered[key]


# ---- named scenarios: one per cache crossing read from icp_ctx.h / the units (DESIGN.md lists which) -----------------------------
def P(**kw):
    return ("set_params", kw)


def OBS(kind, **a):
    return ("obs", kind, a)


A, B, C3, D4 = ("src", 3000, 31), ("tgt", 3000, 31), ("src", 3000, 32), ("tgt", 3000, 32)      # below the AUTO grid's 4096 ...
E, F, G6 = ("src", 6000, 33), ("tgt", 6000, 33), ("src", 6000, 34)                               # ... and above it
P6 = (0.05, -0.03, 0.01, 0.002, -0.001, 0.01)
GUESS = (0.1, 0.05, 0.0, 0.0, 0.0, 0.02)
CHAIN = [(_lib.REJECT_MEDIAN_DISTANCE, 2.0), (_lib.REJECT_ONE_TO_ONE,)]
TRIM = [(_lib.REJECT_TRIMMED, 0.7, 10)]
ALIGN = OBS("align")
ALIGNS_EVERY_METHOD = [P(method=P2P), ALIGN, P(method=P2PLANE), ALIGN, P(method=GICP), ALIGN, P(method=NDT), ALIGN]


def _orders(items):
    import itertools
    return list(itertools.permutations(items))


def scenario_p2plane_promote_recognition():
    ops = [P(method=P2PLANE, max_iterations=4), ("set_target", B), ("set_source", A), ALIGN,
           OBS("normals", of_target=0), OBS("normals", of_target=1), OBS("normals", of_target=0),      # one normals grid, both clouds
           ("set_target_from_source",), OBS("normals", of_target=1), ("set_source", C3), ALIGN,       # the source's normals are not the target's
           ("promote",), OBS("normals", of_target=1), ("set_source", A), OBS("normals", of_target=0), OBS("align", guess=GUESS),
           ("set_target_normals", 7), ALIGN, OBS("nn_reduce_p2plane", T=P6, max_dist=1.0),
           ("set_target_variant", "same"), OBS("normals", of_target=1), ALIGN,                        # recognised: the caller's normals go all the same
           ("set_target_normals", 8), ("promote",), ("set_source", C3), ALIGN,
           ("set_target_normals", 9), ("set_target_variant", "flip_out"), ALIGN, OBS("normals", of_target=1)]
    return ops


def scenario_ndt_cells():
    ops = [P(method=NDT, max_iterations=5), ("set_target", B), ("set_source", A), ALIGN, OBS("ndt_cells"),
           ("set_ndt_params", 2.0, 0.1, 0.55), OBS("ndt_cells"), ALIGN, ("set_ndt_params", 1.0, 0.1, 0.55), OBS("ndt_cells"),
           OBS("ndt_derivatives", p=P6), ("set_target", D4), OBS("ndt_cells"), OBS("ndt_gradient", p=P6), ALIGN,   # another target, equal size
           ("set_ndt_line_search", 1), OBS("align", guess=GUESS), ("set_ndt_line_search", 0),
           ("promote",), OBS("ndt_cells"), ("set_source", C3), ALIGN, OBS("ndt_derivatives", p=P6),
           ("set_target_variant", "same"), OBS("ndt_cells"), ("set_target_variant", "flip_in"), OBS("ndt_cells"), ALIGN]
    return ops


def scenario_three_methods_all_orders():
    ops = [P(max_iterations=3), ("set_target", B), ("set_source", A)]
    for order in _orders((GICP, NDT, P2PLANE)):
        for m in order:
            ops += [P(method=m), ALIGN]
    return ops


def scenario_rejector_chain():
    ops = [P(method=P2P, max_iterations=4), ("set_target", F), ("set_source", E), ("set_rejectors", CHAIN), ALIGN,
           ("set_rejectors", []), ALIGN,                                        # a run without a chain: no stage may outlive it
           ("set_rejectors", CHAIN), ALIGN, P(method=GICP), ALIGN, P(method=NDT), ALIGN,      # these ignore the chain
           P(method=P2PLANE), ALIGN, OBS("align_corr"), ("set_rejectors", TRIM), OBS("corr", T=P6), OBS("align_corr", guess=GUESS),
           P(method=P2P), OBS("align_corr"), ("set_rejectors", []), OBS("align_corr"), OBS("corr", T=P6),
           ("set_rejectors", CHAIN), ("set_target", ("tgt", 6000, 34)), OBS("corr"), ALIGN]
    return ops


def scenario_gate_and_nn_mode(n):
    s, t = ("src", n, 35), ("tgt", n, 35)
    poses = [None, P6, GUESS]
    ops = [P(max_iterations=4), ("set_target", t), ("set_source", s), ALIGN]
    for kw in (dict(max_correspondence_distance=0.3), dict(nn_mode=_lib.NN_BRUTE), dict(brute_variant=1), dict(brute_variant=2),
               dict(nn_mode=_lib.NN_GRID, max_correspondence_distance=2.5), dict(nn_mode=_lib.NN_AUTO, brute_variant=0),
               dict(max_correspondence_distance=1.0)):
        ops += [P(**kw), OBS("nn", T=poses[len(ops) % 3]), OBS("align", fitness=True), OBS("nn", T=poses[(len(ops) + 1) % 3]),
                OBS("nn_reduce", T=P6, max_dist=kw.get("max_correspondence_distance", 1.0))]
    ops += [P(method=GICP), ALIGN, OBS("nn", T=P6), P(method=P2P), OBS("align_fitness")]
    return ops


def scenario_device_buffers():
    ops = [P(max_iterations=4), ("set_target_device", F), ("set_source_device", E), ALIGN, OBS("nn", T=P6),
           ("set_target", ("tgt", 6000, 34), "upload"), ALIGN,                 # host cloud of the external one's size: never recognised
           ("set_target_device", F), ("set_target_variant", "same", "upload"), ALIGN,    # ... not even with its very bytes
           ("set_target_variant", "same", "recognised"),                       # (the host copy just uploaded is recognised)
           ("set_source_device", G6), ("set_target", G6, "upload"), ALIGN,     # an external SOURCE's bytes as the target: uploaded as well
           ("promote",), ("set_source_device", E), ALIGN,                      # an external source promoted
           ("set_target_device", ("tgt", 6000, 34)), OBS("nn"), P(nn_mode=_lib.NN_BRUTE), OBS("nn"), ("set_target_device", F), OBS("nn"),
           ALIGN, P(nn_mode=_lib.NN_AUTO, method=GICP), ALIGN, ("set_source", E), ("set_target_from_source", "recognised"), ALIGN]
    return ops


def scenario_adoption():
    ra, rb = ("src", 6000, 36), ("tgt", 6000, 36)
    ops = [P(max_iterations=4), ("voxel_grid", rb, 0.2, "b"), ("set_target", F), ("voxel_grid", ra, 0.2, "a"), ("voxel_grid", rb, 0.2, "b"),
           ("set_source_slot", "a", "same", "upload"), ALIGN, ("set_source_slot", "b", "same", "adopt")]
    ops += ALIGNS_EVERY_METHOD + [OBS("normals", of_target=0), OBS("cov", of_target=0)]     # grids over a containing box bin every point
    ops += [("set_target_from_source",), ("voxel_grid", ra, 0.2, "a", True), ("set_source_slot", "a", "same", "adopt"), P(method=P2P), ALIGN,
            ("set_source_slot", "a", "flip_in", "upload"), ALIGN, ("set_source_slot", "a", "short", "upload"), OBS("nn"),
            ("set_source_voxel_filtered", rb, 0.2), P(method=GICP), ALIGN, ("voxel_grid", ra, 0.3, "c"), ("set_source_slot", "a", "same", "upload"),
            ALIGN]
    return ops


def scenario_map():
    ops = [P(max_iterations=4), ("map_reset", 0.5), ("map_add_points", F), ("set_source", E), ("map_add_source", P6),
           ("set_target", F), ("set_target_normals", 3), ("map_nn_target", None), P(method=P2PLANE), ALIGN, OBS("normals", of_target=1),
           P(method=P2P), ALIGN, ("map_set_search", True), ("map_nn_target", P6), ALIGN, ("map_set_search", False), ("map_nn_target", P6),
           OBS("nn"), ("set_target", F), OBS("nn"), ALIGN, P(method=NDT), ALIGN,                  # nothing of the map's distinct-point grid survives
           ("map_nn_target", None), P(method=P2P, max_correspondence_distance=0.4), OBS("nn", T=P6), ALIGN,   # the gate changes under the map's grid
           ("map_reset", 1.0), ("map_add_points", ("tgt", 6000, 34)), ("map_nn_target", None), P(method=GICP), ALIGN]
    return ops


def scenario_covariances_across_promote():
    """The version counters of the two clouds are independent sequences: after three targets and one source, the old target's
    covariance grid carries the number the next source gets."""
    ops = [P(method=GICP, max_iterations=3), ("set_target", B), ("set_target", D4), ("set_target", B), ("set_source", A), ALIGN,
           ("promote",), ("set_source", C3), OBS("cov", of_target=0), OBS("cov", of_target=1), ALIGN,
           P(gicp_inner=_lib.GICP_INNER_QUADRATIC), ALIGN, ("set_target_from_source",), ("set_source", A), ALIGN, P(gicp_inner=0), ALIGN]
    return ops


def scenario_odometer_loop():
    ops = [P(max_iterations=4)]
    methods = [P2P, GICP, P2PLANE, NDT]
    seeds = [31, 32, 37, 38]
    ops += [("set_target", ("tgt", 3000, 31)), ("set_source", ("src", 3000, 31)), ALIGN]
    for k in range(40):
        method = methods[(k // 4) % 4]
        if k % 4 == 0:
            ops.append(P(method=method))
        if k == 22:                                           # a batch in the middle of GICP's turn, which goes on after it
            ops += [OBS("align_batch", k=3, n=2000, seed=39)]
        if k % 3 == 2:
            ops.append(("set_target_variant", "same", "recognised"))      # a rejected scan: prev_cloud_ stays, and is recognised
        else:
            ops.append(("set_target_from_source", "recognised"))         # `*prev_cloud_ = *curr_cloud_`: the promote path
        ops.append(("set_source", ("src" if k % 2 else "tgt", 3000, seeds[k % 4])))
        ops.append(OBS("align", fitness=k % 5 == 0, view=k % 7 == 0))
    return ops


SCENARIOS = {
    "p2plane_promote_recognition": scenario_p2plane_promote_recognition,
    "ndt_cells": scenario_ndt_cells,
    "three_methods_all_orders": scenario_three_methods_all_orders,
    "rejector_chain": scenario_rejector_chain,
    "gate_and_nn_mode_9000": lambda: scenario_gate_and_nn_mode(9000),          # the matrix-core brute force and its Morton order
    "gate_and_nn_mode_33000": lambda: scenario_gate_and_nn_mode(33000),        # nn_quad_kernel
    "gate_and_nn_mode_120000": lambda: scenario_gate_and_nn_mode(120000),      # the cell-ordered source
    "device_buffers": scenario_device_buffers,
    "adoption": scenario_adoption,
    "map": scenario_map,
    "covariances_across_promote": scenario_covariances_across_promote,
    "odometer_loop": scenario_odometer_loop,
}

# ---- seeded random walks over the vocabulary -------------------------------------------------------------------------------------
# small clouds (2k .. 6k points).  The seeds are a greedy cover computed on the host by greedy_seed_cover() of
# tests/test_history_model_host.py (run it again after a change to the vocabulary or to gen_walk): together they flag every
# injectable fault of the fake context and exercise every pair of DEPENDS below.  The faults are flagged mostly through gen_walk's
# motif() sequences, each written for one cache crossing and placed at a random point of a random history; the plain random
# steps alone reach only some of them
WALK_SEEDS = (112, 113, 124, 125, 192, 197, 200, 208, 233, 239, 255, 269, 278, 295, 298, 341, 366)
LARGE_WALK_SEEDS = (900, 901)                # a fixed minority at the sizes the grid kernels and the cell-ordered source need
WALK_LENGTH, LARGE_WALK_LENGTH = 40, 14
GATES = (0.3, 1.0, 2.5)
CHAINS = ([], CHAIN, TRIM)


def gen_walk(seed, length=None, large=None):
    """A deterministic operation list: needs no context (it tracks only which clouds are set), so the host test and the GPU test
    walk the very same lists."""
    large = (seed in LARGE_WALK_SEEDS) if large is None else large
    length = (LARGE_WALK_LENGTH if large else WALK_LENGTH) if length is None else length
    rng = np.random.default_rng(seed)
    sizes = (33000, 120000) if large else tuple(int(x) for x in rng.choice((2000, 3000, 4500, 6000), 2, replace=False))
    pool = [(k, n, s) for n in sizes for s in (41 + seed % 3, 45) for k in ("src", "tgt")]
    pick = lambda seq: seq[int(rng.integers(len(seq)))]                       # noqa: E731
    st = dict(src=False, tgt=False, map=False, map_pts=False, slots=[], method=P2P, chain=False, n_tgt=0)
    ops = [P(max_iterations=3), ("set_target", pick(pool)), ("set_source", pick(pool))]
    st["src"] = st["tgt"] = True

    def p6():
        return tuple(round(float(x), 4) for x in rng.uniform(-1, 1, 6) * (0.2, 0.2, 0.02, 0.005, 0.005, 0.03))

    def mutation():
        cands = ["set_source", "set_target", "set_source_device", "set_target_device", "voxel_grid", "set_source_voxel_filtered", "set_params",
                 "set_params", "set_ndt_params", "set_ndt_line_search", "set_rejectors", "map_reset"]
        if st["tgt"]:
            cands += ["set_target_variant", "set_target_variant", "set_target_normals"]
        if st["src"]:
            cands += ["promote", "set_target_from_source", "set_target_from_source", "set_source_variant"]
        if st["slots"]:
            cands += ["set_source_slot", "set_source_slot"]
        if st["map"]:
            cands += ["map_add_points", "map_set_search"] + (["map_add_source"] if st["src"] else [])
        if st["map_pts"] and st["src"]:
            cands += ["map_nn_target", "map_nn_target"]
        name = pick(cands)
        if name in ("set_source", "set_source_device"):
            st["src"] = True
            return (name, pick(pool))
        if name in ("set_target", "set_target_device"):
            st["tgt"] = True
            return (name, pick(pool))
        if name == "set_target_variant":
            return (name, pick(("same", "same", "flip_in", "flip_out", "short")))
        if name == "set_source_variant":
            return (name, pick(("same", "flip_in", "flip_out", "short")))
        if name == "set_target_from_source":
            st["tgt"] = True
            return (name,)
        if name == "promote":
            st["src"], st["tgt"] = False, True
            return (name,)
        if name == "voxel_grid":
            slot = pick(("a", "b"))
            if slot not in st["slots"]:
                st["slots"].append(slot)
            return (name, pick(pool), 0.2, slot, bool(rng.integers(2)))
        if name == "set_source_slot":
            st["src"] = True
            return (name, pick(st["slots"]), pick(("same", "same", "same", "flip_out")))
        if name == "set_source_voxel_filtered":
            st["src"] = True
            return (name, pick(pool), 0.2)
        if name == "set_target_normals":
            return (name, int(rng.integers(1000)))
        if name == "set_params":
            field = pick(("method", "method", "method", "nn_mode", "brute_variant", "max_correspondence_distance", "max_iterations", "gicp_inner"))
            if field == "method":
                st["method"] = int(pick((P2P, GICP, P2PLANE, NDT)))
                return P(method=st["method"])
            if field == "max_correspondence_distance":
                return P(max_correspondence_distance=pick(GATES))
            if field == "max_iterations":
                return P(max_iterations=int(pick((2, 3, 5))))
            return P(**{field: int(rng.integers(3 if field != "gicp_inner" else 2))})
        if name == "set_ndt_params":
            return (name, pick((1.0, 2.0, 1.5)), 0.1, 0.55)
        if name == "set_ndt_line_search":
            return (name, int(rng.integers(2)))
        if name == "set_rejectors":
            chain = pick(CHAINS)
            st["chain"] = bool(chain)
            return (name, list(chain))
        if name == "map_reset":
            st["map"], st["map_pts"] = True, False
            return (name, pick((0.5, 1.0)))
        if name == "map_add_points":
            st["map_pts"] = True
            return (name, pick(pool), pick((None, p6())))
        if name == "map_add_source":
            st["map_pts"] = True
            return (name, pick((None, p6())))
        if name == "map_set_search":
            return (name, bool(rng.integers(2)))
        if name == "map_nn_target":
            st["tgt"] = True
            return (name, pick((None, p6())))
        raise AssertionError(name)

    def emit_observation(after=()):
        """An observation the state allows -- mostly one that DEPENDS names for the mutations just made -- with the method it needs."""
        both = st["src"] and st["tgt"]
        feasible = []
        for tag in DEPENDS:
            kind = tag.split(":")[0]
            if tag == "map_nn_target":
                continue
            if tag in ("normals:target", "cov:target", "ndt_cells"):
                ok = st["tgt"]
            elif tag in ("normals:source", "cov:source", "transform"):
                ok = st["src"]
            else:
                ok = both
            if ok:
                feasible += [tag] * (4 if kind == "align" else 1)
        if both and not large and not st["chain"]:
            feasible.append("align_batch")
        if not feasible:
            return
        related = [t for t in feasible if any(m in DEPENDS.get(t, ()) for m in after)]
        tag = pick(related) if related and rng.random() < 0.7 else pick(feasible)
        kind = tag.split(":")[0]
        want = None
        if kind == "align":
            want = {v: k for k, v in METHOD_TAG.items()}[tag.split(":")[1]]
        elif kind == "align_corr" and st["method"] not in (P2P, P2PLANE):
            want = int(pick((P2P, P2PLANE)))
        elif kind == "align_batch" and st["method"] not in (P2P, GICP):
            want = int(pick((P2P, GICP)))
        if want is not None and want != st["method"]:
            st["method"] = want
            ops.append(P(method=want))
        if kind in ("align", "align_fitness", "align_corr"):
            a = dict(guess=pick((None, None, p6())))
            if kind == "align":
                a.update(fitness=bool(rng.integers(2)), view=bool(rng.integers(2)))
            ops.append(OBS(kind, **a))
        elif kind in ("nn", "corr", "transform"):
            ops.append(OBS(kind, T=pick((None, p6()))))
        elif kind in ("nn_reduce", "nn_reduce_p2plane"):
            ops.append(OBS(kind, T=p6(), max_dist=pick(GATES)))
        elif kind in ("ndt_derivatives", "ndt_gradient"):
            ops.append(OBS(kind, p=p6()))
        elif kind == "align_batch":
            ops.append(OBS(kind, k=2, n=2000, seed=39))
        elif kind == "ndt_cells":
            ops.append(OBS(kind))
        else:
            ops.append(OBS(kind, of_target=int(tag.endswith("target"))))

    def motif():
        """Short crossings of one cache each, at a random place in a random history."""
        which = pick(("normals_recognised", "brute_seed", "covariance_grid", "chain_off", "map", "map", "two_filters", "promote_normals"))
        if which == "normals_recognised" and st["tgt"]:
            return [("set_target_normals", int(rng.integers(1000))), ("set_target_variant", "same")]
        if which == "brute_seed" and st["src"]:
            st["tgt"] = True
            return [P(nn_mode=_lib.NN_BRUTE), ("set_target_device", pick(pool)), OBS("nn", T=p6()), ("set_target_device", pick(pool))]
        if which == "covariance_grid" and st["src"] and st["tgt"]:
            st["method"] = GICP
            return ([("set_target_variant", pick(("flip_in", "flip_out")))] * int(rng.integers(4))
                    + [P(method=GICP), OBS("align"), ("promote",), ("set_source", pick(pool)), OBS("cov", of_target=0)])
        if which == "chain_off" and st["src"] and st["tgt"]:
            st["method"], st["chain"] = P2P, False
            return [P(method=P2P), ("set_rejectors", list(pick((CHAIN, TRIM)))), OBS("align"), ("set_rejectors", [])]
        if which == "map" and st["src"]:
            st["map"] = st["map_pts"] = st["tgt"] = True
            return [("map_reset", pick((0.5, 1.0))), ("map_add_points", pick(pool), None), ("map_add_source", pick((None, p6()))),
                    ("map_nn_target", pick((None, p6())))]
        if which == "promote_normals" and st["src"] and st["tgt"]:
            st["method"] = P2PLANE
            return [P(method=P2PLANE), OBS("align"), ("promote",), ("set_source", pick(pool)), OBS("normals", of_target=1)]
        if which == "two_filters":
            st["src"] = True
            st["slots"] = sorted(set(st["slots"]) | {"a", "b"})
            return [("voxel_grid", pick(pool[:4]), 0.2, "a", False), ("voxel_grid", pick(pool[4:]), 0.2, "b", True),
                    ("set_source_slot", pick(("a", "b")), "same")]
        return [mutation()]

    while len(ops) < length:
        made = motif() if rng.random() < 0.25 else [mutation()]
        if rng.random() < 0.3:
            made.append(mutation())
        ops += made
        after = [m for op in made for m in _writes(op)[0]]
        for _ in range(3 if "map_nn_target" in after else int(rng.integers(1, 3))):
            emit_observation(after)
    return ops


# ---- which mutation each observation depends on (checked on the host: every pair is exercised by the committed walks) --------------
SRC_OPS = ["set_source", "set_source_device", "set_source_slot", "set_source_variant", "set_source_voxel_filtered"]
TGT_OPS = ["set_target", "set_target_variant", "set_target_from_source", "set_target_device", "promote", "map_nn_target"]
CLOUDS = SRC_OPS + TGT_OPS
SEARCH = ["set_params:nn_mode", "set_params:brute_variant", "set_params:max_correspondence_distance"]
DEPENDS = {
    "align:p2p": CLOUDS + SEARCH + ["set_params:method", "set_params:max_iterations", "set_rejectors", "obs:align_batch"],
    "align:p2plane": CLOUDS + SEARCH + ["set_params:method", "set_target_normals", "set_rejectors"],
    "align:gicp": CLOUDS + SEARCH + ["set_params:method", "set_params:gicp_inner", "set_rejectors", "obs:align_batch"],
    "align:ndt": CLOUDS + ["set_params:method", "set_ndt_params", "set_ndt_line_search", "set_rejectors"],
    "align_fitness": CLOUDS + ["set_params:max_correspondence_distance"],
    "align_corr": CLOUDS + ["set_rejectors"],
    "nn": CLOUDS + SEARCH,
    "nn_reduce": CLOUDS,
    "nn_reduce_p2plane": CLOUDS + ["set_target_normals"],
    "corr": CLOUDS + SEARCH + ["set_rejectors"],
    "normals:target": TGT_OPS + ["set_target_normals"],
    "normals:source": SRC_OPS + ["promote"],
    "cov:target": TGT_OPS,
    "cov:source": SRC_OPS + ["promote"],
    "ndt_cells": TGT_OPS + ["set_ndt_params"],
    "ndt_derivatives": CLOUDS + ["set_ndt_params"],
    "ndt_gradient": CLOUDS + ["set_ndt_params"],
    "transform": SRC_OPS,
    "map_nn_target": SRC_OPS + ["map_reset", "map_add_points", "map_add_source", "map_set_search", "set_params:max_correspondence_distance",
                                "set_params:nn_mode"],
}
# an operation between the two that writes the same piece of state again resets the pair
_PIECE = {**{m: "source" for m in SRC_OPS}, **{m: "target" for m in TGT_OPS}, "set_target_normals": "normals", "set_ndt_params": "ndt",
          "set_ndt_line_search": "line_search", "set_rejectors": "chain", "map_reset": "map", "map_add_points": "map:points", "map_add_source": "map:source",
          "map_set_search": "map_search", "obs:align_batch": "batch"}


def _writes(op):
    """(mutation names, pieces of state written) of one logged operation."""
    name = op[0]
    if name == "set_params":
        tags = ["set_params:" + k for k in op[1]]
        return tags, tags
    if name == "obs":
        return (["obs:align_batch"], []) if op[1] == "align_batch" else ([], [])
    pieces = [_PIECE[name]] if name in _PIECE else []
    if name in TGT_OPS:
        pieces.append("normals")
    if name == "promote":
        pieces.append("source!")       # (unset, not rewritten: the pair promote -> normals:source needs the set_source in between)
    if name == "map_reset":
        pieces += ["map:points", "map:source"]       # (insertions accumulate: only a reset takes them away)
    return [name], pieces


def _obs_tag(op, method):
    kind, a = op[1], op[2]
    if kind == "align":
        return "align:" + METHOD_TAG[method]
    if kind in ("normals", "cov"):
        return f"{kind}:{'target' if a['of_target'] else 'source'}"
    return kind


def covered_pairs(logs):
    """{(mutation, observation tag)} over the logs: mutation first, observation after, the mutation's piece not rewritten between."""
    seen = set()
    for ops in logs:
        live = {}                     # mutation name -> pieces it wrote, still in force
        method = P2P
        for op in ops:
            if op[0] == "set_params" and "method" in op[1]:
                method = op[1]["method"]
            if op[0] == "obs" or op[0] == "map_nn_target":
                tag = "map_nn_target" if op[0] == "map_nn_target" else _obs_tag(op, method)
                seen.update((m, tag) for m in live)
            names, pieces = _writes(op)
            if pieces:
                for m in [m for m, ps in live.items() if set(ps) & set(pieces)]:
                    del live[m]
            for m in names:
                live[m] = [_PIECE.get(m, m)]          # its own piece (what it writes besides only resets others)
    return seen
