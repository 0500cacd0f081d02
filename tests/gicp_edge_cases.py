"""GICP alignment at its edges: ONE table of cases shared by tests/test_gicp_edges_host.py (CPU oracle) and
tests/test_gpu_gicp_edges.py (every GPU path).  A plain module, like tests/rejectors_restated.py.

Each case is (name, src, tgt, guess, params, exit):
  guess   None, or a 4x4 matrix (float32 or float64: both sides round it to float, the C ABI's type);
  params  what differs from the defaults, for oracle.default_params and Context.set_params alike;
  exit    the RECORDED end of the registration -- state, converged, and iterations / n_corr where they are the point of the case;
          refused = True: a cloud of fewer than 20 finite points (not converged, T = I, 0 iterations, 0 correspondences).
The inputs come from synth and NumPy only and are deterministic.  The ends were printed by the oracle when the table was written
(python tests/gicp_edge_cases.py prints them again) and are asserted by both test files, so a case cannot quietly stop hitting
what it was built to hit.

The launch boundaries behind the source sizes (icpslam_amd/csrc): the evaluation server gives one workgroup per 512 sources,
the device solver one per 1024; up to 32 workgroups (32 768) run the one-XCD variant; up to 64 x 1024 sources stay resident,
more are streamed.
"""
from __future__ import annotations

import functools
import os
import sys
from collections import namedtuple

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:   # (run as a script, or imported by a child process of a test)
    sys.path.insert(0, _ROOT)

from icpslam_amd import synth

Case = namedtuple("Case", "name src tgt guess params exit")

NOT_CONVERGED, ITERATIONS, TRANSFORM, NO_CORRESPONDENCES = 0, 1, 2, 5
SIZES = (20, 21, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 32767, 32768, 32769, 65535, 65536, 65537)
SMALL = 1025                      # "the small cases": what the slow restatement and the forced-streaming flavour take
COMMON = dict(max_iterations=3)   # wherever convergence is not the point (one parameter set: these cases share a batch call)
REFUSED = dict(state=NOT_CONVERGED, converged=False, iterations=0, n_corr=0, refused=True)
f32 = np.float32


def _cloud(xyz) -> np.ndarray:
    out = np.ones((len(xyz), 4), f32)
    out[:, :3] = np.asarray(xyz, f32)
    return out


def _moved(cloud, T) -> np.ndarray:
    out = cloud.copy()
    out[:, :3] = (cloud[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(f32)
    return out


# ---- the gate --------------------------------------------------------------------------------------------------------------
# A lone target point L = (0, 0, 100) high above the scene and source points (dx, dy, 100): with the identity as guess and one forced
# iteration the first search sees the coordinates unchanged, the differences are (dx, dy, 0) exactly and
# d2 = fma(dz, dz, fma(dy, dy, dx * dx)) = float(dy * dy + float(dx * dx)).
GATE_Z = 100.0


def _d2(dx, dy) -> np.float32:
    """The search's float d2 of the difference (dx, dy, 0).  dy * dy is exact in float64; the sum is then rounded once to float64
    and once to float -- _offsets_for only accepts sums whose float64 rounding cannot have moved a float tie."""
    xx = np.float64(f32(np.float64(dx) * np.float64(dx)))
    return f32(np.float64(dy) * np.float64(dy) + xx)


def _offsets_for(t: np.float32):
    """(dx, dy) floats with _d2(dx, dy) == t exactly: dx the largest float whose square does not exceed t, dy fills the rest."""
    dx = f32(np.sqrt(np.float64(t)))
    while _d2(dx, 0.0) > t:
        dx = np.nextafter(dx, f32(0))
    if _d2(dx, 0.0) == t:
        return dx, f32(0)
    rest = np.float64(t) - np.float64(_d2(dx, 0.0))
    dy = f32(np.sqrt(rest))
    for _ in range(64):
        got = _d2(dx, dy)
        if got == t:
            s = np.float64(dy) * np.float64(dy) + np.float64(_d2(dx, 0.0))
            lo, hi = np.float64(np.nextafter(t, f32(0))), np.float64(np.nextafter(t, f32(np.inf)))
            assert abs(s - np.float64(t)) < 0.25 * min(np.float64(t) - lo, hi - np.float64(t)), "too close to a tie"
            return dx, dy
        dy = np.nextafter(dy, f32(np.inf) if got < t else f32(0))
    raise AssertionError("no offsets for %r" % t)


def gate_points(r: float):
    """dict(inside, on, outside: (k, 2) float32 offsets (dx, dy), wide: a gate that lets `on` in and nothing else, d2: name -> the
    float d2 of the group).  r * r exact in float: `on` sits at d2 == r^2 (rejected: the test is strict), `inside` / `outside` one
    float below / above.  Otherwise no float equals r^2: `inside` is the largest float below it, `on` the smallest float above it --
    the pair threshold_from and its nextafterf have to separate -- and `outside` the next one."""
    r2 = np.float64(r) * np.float64(r)
    exact = np.float64(f32(r2)) == r2
    if exact:
        t_on = f32(r2)
    else:
        t_on = f32(r2)
        if np.float64(t_on) < r2:
            t_on = np.nextafter(t_on, f32(np.inf))
    t_in, t_out = np.nextafter(t_on, f32(0)), np.nextafter(t_on, f32(np.inf))
    assert np.float64(t_in) < r2 <= np.float64(t_on) < np.float64(t_out)

    def ring(t, signs):
        dx, dy = _offsets_for(t)
        return np.array([(sx * dx, sy * dy) if not swap else (sy * dy, sx * dx) for sx, sy, swap in signs], f32)

    out = dict(inside=ring(t_in, [(1, 1, False), (-1, 1, True)]), on=ring(t_on, [(1, -1, False), (-1, -1, False), (1, 1, True)]),
               outside=ring(t_out, [(-1, 1, False), (1, -1, True)]), d2=dict(inside=t_in, on=t_on, outside=t_out), exact=bool(exact))
    wide = np.sqrt(np.float64(t_on))
    while not (wide * wide > np.float64(t_on)):
        wide = np.nextafter(wide, np.inf)
    assert wide * wide < np.float64(t_out)
    out["wide"] = float(wide)
    return out


def _gate_pair(r: float):
    base_s, base_t, _ = synth.make_pair(1500, 1500, seed=21)
    g = gate_points(r)
    offs = np.concatenate([g["inside"], g["on"], g["outside"]])
    extra = np.column_stack([offs, np.full(len(offs), GATE_Z, f32)])
    src = np.concatenate([base_s, _cloud(extra)])
    tgt = np.concatenate([base_t, _cloud([(0.0, 0.0, GATE_Z)])])
    return src, tgt, g


# ---- the table --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, src, tgt, guess=None, params=None, **exit_):
        out.append(Case(name, np.ascontiguousarray(src, f32), np.ascontiguousarray(tgt, f32), guess, dict(COMMON if params is None else params), exit_))

    # -- source sizes on the launch boundaries (a scan's points come in random order: a prefix is a sample of the whole scene)
    big_s, tgt4k, _ = synth.make_pair(SIZES[-1], 4000, seed=7)
    for n in SIZES:
        add("ns_%d" % n, big_s[:n], tgt4k, state=ITERATIONS, converged=True, iterations=3)
    add("nt_20", big_s[:500], tgt4k[:20], **RECORDED["nt_20"])

    # -- an initial guess (want_cloud: see wants_cloud)
    gs, gt, _ = synth.make_pair(3000, 3000, seed=2)
    small = synth.pose_matrix(0.2, -0.1, 0.05, 0.01, -0.02, 0.03)
    dflt = dict()  # PCL's defaults: these cases are about where the registration ends
    add("guess_small", gs, gt, small.astype(f32), dflt, state=TRANSFORM, converged=True, iterations=2, n_corr=2776)
    add("guess_small_f64", gs, gt, small, dflt, state=TRANSFORM, converged=True, iterations=2, n_corr=2776)
    yaw = synth.pose_matrix(0.3, -0.2, 0.0, 0.0, 0.0, 1.0)
    add("guess_yaw_1rad", _moved(gs, np.linalg.inv(yaw)), gt, yaw, dflt, **RECORDED["guess_yaw_1rad"])
    ks, kt, T_gt = synth.make_known_answer_pair(3000, seed=5)
    add("guess_exact", ks, kt, T_gt, dflt, **RECORDED["guess_exact"])
    add("guess_far", gs, gt, synth.pose_matrix(500.0, 0.0, 0.0, 0.0, 0.0, 0.3), dflt, state=NO_CORRESPONDENCES, converged=False,
        iterations=0, n_corr=0)

    # -- pairs on the gate
    one = dict(max_iterations=1, force_iterations=1)
    for r in (1.0, 0.5, 0.3):
        src, tgt, g = _gate_pair(r)
        for tag, gate in (("", r), ("_wide", g["wide"])):
            add("gate_%g%s" % (r, tag), src, tgt, np.eye(4, dtype=f32), dict(one, max_correspondence_distance=gate), state=ITERATIONS,
                converged=True, iterations=1, n_corr=RECORDED_GATE[r] + (len(g["on"]) if tag else 0))

    # -- the correspondence minimum: k sources near the target, the rest of a 28-point source 500 m above it
    ms, mt, _ = synth.make_pair(40, 3000, seed=9)
    for k in (3, 4, 5):
        near = mt[100:100 + k].copy()
        near[:, :3] += f32(0.05)
        far = ms[:25].copy()
        far[:, 2] += f32(500.0)
        add("min_%d" % k, np.concatenate([far[:11], near, far[11:]]), mt, **RECORDED["min_%d" % k])

    # -- non-finite points
    ns, nt, _ = synth.make_pair(3000, 3000, seed=11)

    def poisoned(cloud, start):
        c = cloud.copy()
        for j, (axis, v) in enumerate([(0, np.nan), (1, np.inf), (2, -np.inf), (0, np.inf), (2, np.nan), (1, -np.inf)]):
            c[start + 97 * j, axis] = v
        return c
    add("nonfinite_src", poisoned(ns, 5), nt, **RECORDED["nonfinite_src"])
    add("nonfinite_tgt", ns, poisoned(nt, 11), **RECORDED["nonfinite_tgt"])
    add("nonfinite_both", poisoned(ns, 5), poisoned(nt, 11), **RECORDED["nonfinite_both"])
    last = big_s[:1025].copy()
    last[-1, 1] = np.nan
    add("nonfinite_last_of_1025", last, tgt4k, state=ITERATIONS, converged=True, iterations=3)
    thirty = mt[200:230].copy()
    thirty[:, :3] += f32(0.03)
    legal = thirty.copy()
    legal[::3, 0] = np.nan           # 10 of 30: exactly 20 finite points, the smallest legal cloud
    add("finite_20_of_30", legal, mt, **RECORDED["finite_20_of_30"])
    few = legal.copy()
    few[1, 2] = np.inf               # 19 finite points: too small, as a source and as a target
    add("finite_19_of_30_src", few, mt, **REFUSED)
    add("finite_19_of_30_tgt", ns, few, **REFUSED)
    probe = thirty.copy()
    probe[:12, 1] = np.nan           # 18 of 30: the cloud that crashed the oracle's covariances
    add("finite_18_of_30_src", probe, mt, **REFUSED)

    # -- degenerate but legal
    add("identical", nt, nt.copy(), state=TRANSFORM, converged=True, iterations=1, n_corr=3000)
    shift = np.array([3000.0, 0.0, 0.0, 0.0], f32)
    add("shifted_3km", ns + shift, nt + shift, **RECORDED["shifted_3km"])
    plane = synth.plane_through_origin(3000, seed=1)
    add("planar_target", _moved(synth.plane_through_origin(3000, seed=2), synth.pose_matrix(0.05, -0.03, 0.02, 0.004, -0.003, 0.01)), plane,
        **RECORDED["planar_target"])
    add("duplicate_targets", ns, np.concatenate([nt[:2700], nt[:300]]), **RECORDED["duplicate_targets"])
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


# What the oracle printed when the table was written (python tests/gicp_edge_cases.py); gates: n_corr at the nominal gate.
def _end(state, iterations, n_corr=None):
    e = dict(state=state, converged=state in (ITERATIONS, TRANSFORM), iterations=iterations)
    if n_corr is not None:
        e["n_corr"] = n_corr
    return e


RECORDED = {
    "nt_20": _end(ITERATIONS, 3),
    "guess_yaw_1rad": _end(TRANSFORM, 2, 2881),
    "guess_exact": _end(TRANSFORM, 1, 3000),
    "min_3": _end(NO_CORRESPONDENCES, 0, 3),      # NotEnoughPoints: m < 4
    "min_4": _end(ITERATIONS, 3, 4),
    "min_5": _end(ITERATIONS, 3, 5),
    "nonfinite_src": _end(ITERATIONS, 3, 2856),
    "nonfinite_tgt": _end(ITERATIONS, 3, 2862),
    "nonfinite_both": _end(ITERATIONS, 3, 2856),
    "finite_20_of_30": _end(ITERATIONS, 3, 20),
    "shifted_3km": _end(TRANSFORM, 2),
    "planar_target": _end(ITERATIONS, 3, 3000),
    "duplicate_targets": _end(ITERATIONS, 3),
}
RECORDED_GATE = {1.0: 1431, 0.5: 1344, 0.3: 1160}


def wants_cloud(case) -> bool:
    """the guess cases ask for the aligned cloud (and are therefore no batch material)"""
    return case.name.startswith("guess_")


def by_name(name):
    return next(c for c in cases() if c.name == name)


def is_small(case) -> bool:
    return case.src.shape[0] <= SMALL and case.tgt.shape[0] <= 4000 and bool(np.isfinite(case.src).all()) and bool(np.isfinite(case.tgt).all())


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's answer for a case (computed once, shared by every test that needs it; treat as read-only)."""
    import oracle
    c = by_name(name)
    return oracle.icp_align(c.src, c.tgt, oracle.default_params(method=oracle.GICP, **c.params), guess=c.guess,
                            want_cloud=wants_cloud(c), want_fitness=True)


def check_exit(case, got):
    """the recorded end of the case holds for `got` (an oracle or a library result)"""
    e = case.exit
    assert got["state"] == e["state"] and got["converged"] == e["converged"], (case.name, got["state"], got["converged"], e)
    for k in ("iterations", "n_corr"):
        if k in e:
            assert got[k] == e[k], (case.name, k, got[k], e[k])
    if e.get("refused"):
        assert np.array_equal(got["T"], np.eye(4, dtype=f32)), case.name


# ---- running the table on the library (tests/test_gpu_gicp_edges.py: in the test's process and in its child processes) ------------
AFTER_REFUSED = "ns_257"   # the ordinary pair that follows every refused cloud on the same context


def run_case(ctx, case):
    """one case on `ctx` -> the result dict + the profile's device / host solve counts of this alignment"""
    from icpslam_amd import GICP
    ctx.set_params(ctx.default_params(), method=GICP, **case.params)
    ctx.set_source(case.src)
    ctx.set_target(case.tgt)
    ctx.profile_reset()
    r = ctx.align(guess=case.guess, want_cloud=wants_cloud(case), want_fitness=True)
    p = ctx.profile()
    r["device_solves"], r["host_solves"] = int(p.gicp_device_solves), int(p.gicp_host_solves)
    return r


def run_table(ctx, names):
    """{name: result} for `names` in table order on ONE context; "after:<name>": AFTER_REFUSED right after a refused cloud"""
    out = {}
    for c in cases():
        if c.name not in names:
            continue
        out[c.name] = run_case(ctx, c)
        if c.exit.get("refused"):
            out["after:" + c.name] = run_case(ctx, by_name(AFTER_REFUSED))
    return out


def save_results(path, results):
    flat = {}
    for name, r in results.items():
        flat["T:" + name] = r["T"]
        flat["m:" + name] = np.array([r["converged"], r["iterations"], r["state"], r["n_corr"], r["device_solves"], r["host_solves"]], np.int64)
        flat["f:" + name] = np.array([r["mse"], r["fitness"]], np.float64)
        if r.get("cloud") is not None:
            flat["c:" + name] = r["cloud"]
    np.savez(path, **flat)


def load_results(path):
    z = np.load(path)
    out = {}
    for key in z.files:
        if key.startswith("T:"):
            name = key[2:]
            m, f = z["m:" + name], z["f:" + name]
            out[name] = dict(T=z[key], converged=bool(m[0]), iterations=int(m[1]), state=int(m[2]), n_corr=int(m[3]), device_solves=int(m[4]),
                             host_solves=int(m[5]), mse=float(f[0]), fitness=float(f[1]), cloud=z["c:" + name] if "c:" + name in z.files else None)
    return out


def child_main(path, which):
    """a child process of the test: the whole table (which = all) or its small cases (which = small) on one fresh context"""
    from icpslam_amd import Context
    names = {c.name for c in cases() if which == "all" or is_small(c)}
    with Context(0) as ctx:
        save_results(path, run_table(ctx, names))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child_main(sys.argv[2], sys.argv[3])
        sys.exit(0)
    for c in cases():
        r = reference(c.name)
        print("%-26s n_s=%-6d n_t=%-5d state=%d converged=%d iterations=%d n_corr=%d" % (
            c.name, c.src.shape[0], c.tgt.shape[0], r["state"], r["converged"], r["iterations"], r["n_corr"]))
