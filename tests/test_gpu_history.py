"""A context's answers do not depend on what it did before ("History independence"): every observation on a context with
history returns the bytes and counts of a new context that was given only the logical state (tests/history_model.py: the model, the
vocabulary, the named scenarios -- one per cache crossing of icpslam_amd/csrc/icp_ctx.h -- and the seeded walks; the same lists run
against a fake context with injectable stale caches in tests/test_history_model_host.py).  Bit for bit, except `fitness` of a source
of >= 100k points at the 1e-12 relative that tests/test_gpu_recognition.py documents.  Nothing is shrunk or retried here: a walk
stops at its first divergence or library error and prints seed, observation index and the replayable log."""
import numpy as np
import pytest

import history_model as hm

pytestmark = pytest.mark.gpu

FRESH_KINDS = [
    ("align", dict(fitness=True), dict(method=hm.P2P)), ("align", dict(view=True, guess=hm.GUESS), dict(method=hm.P2PLANE)),
    ("align", dict(fitness=True), dict(method=hm.GICP)), ("align", dict(), dict(method=hm.GICP, gicp_inner=1)),
    ("align", dict(fitness=True), dict(method=hm.NDT)), ("align", dict(line_search=1), dict(method=hm.NDT)),
    ("align_fitness", dict(), {}), ("align_corr", dict(), dict(method=hm.P2PLANE)), ("nn", dict(T=hm.P6), {}),
    ("nn", dict(T=hm.P6), dict(nn_mode=1)), ("nn_reduce", dict(T=hm.P6, max_dist=1.0), {}), ("nn_reduce_p2plane", dict(T=hm.P6, max_dist=1.0), {}),
    ("corr", dict(T=hm.P6), {}), ("normals", dict(of_target=0), {}), ("normals", dict(of_target=1), {}), ("cov", dict(of_target=0), {}),
    ("cov", dict(of_target=1), {}), ("ndt_cells", dict(), {}), ("ndt_derivatives", dict(p=hm.P6), {}), ("ndt_gradient", dict(p=hm.P6), {}),
    ("transform", dict(T=hm.P6), {}), ("align_batch", dict(k=2, n=2000, seed=39), {}), ("map_nn_target", dict(pose=hm.P6), {}),
]


@pytest.fixture(scope="module")
def backend(built):
    return hm.GpuBackend()


@pytest.mark.parametrize("n", [6000, 33000, 120000])
def test_two_new_contexts_agree_on_every_observation_kind(backend, n):
    """The rule the history tests apply, first between two contexts WITHOUT history: whatever fails here is not reproducible at all."""
    bad = []
    for kind, a, params in FRESH_KINDS:
        if kind == "align_batch" and n != 6000:
            continue
        a = dict(a)
        m = hm.Model()
        m.params = dict(max_iterations=4, **params)
        m.line_search = a.pop("line_search", 0)
        m.source, m.target = hm.cloud(("src", n, 35)), hm.cloud(("tgt", n, 35))
        m.chain = [] if kind == "align_batch" else list(hm.CHAIN)      # (a chain has no batch path)
        m.map_resolution, m.map_insertions = 0.5, [(m.target, None)]
        one, two = hm.replay_fresh(backend, m, kind, a), hm.replay_fresh(backend, m, kind, a)
        diff = hm.differences(one, two, n)
        print(n, kind, a, params, "differ:", diff)
        if diff:
            bad.append((kind, a, params, diff))
    assert not bad, bad


@pytest.mark.parametrize("name", list(hm.SCENARIOS))
def test_scenario(backend, name):
    with hm.Walk(backend, seed=name) as w:
        w.run(hm.SCENARIOS[name]())
        print(name, "operations", len(w.log), "observations", w.n_obs)


@pytest.mark.parametrize("seed", hm.WALK_SEEDS + hm.LARGE_WALK_SEEDS)
def test_walk(backend, seed):
    with hm.Walk(backend, seed=seed) as w:
        w.run(hm.gen_walk(seed))
        print(seed, "operations", len(w.log), "observations", w.n_obs)


def test_rejector_statistics_do_not_outlive_a_run_without_a_chain(backend):
    """Found by the rejector scenario, reduced by hand: the stages of an earlier alignment's chain were still reported after an
    alignment that ran without one (icpgpu_rejector_stats: "the last iteration of the context's last ... alignment")."""
    with hm.Walk(backend, seed="reduced") as w:
        w.run([hm.P(max_iterations=3), ("set_target", hm.B), ("set_source", hm.A), ("set_rejectors", hm.CHAIN), hm.ALIGN,
               ("set_rejectors", []), hm.ALIGN, hm.P(method=hm.P2PLANE), ("set_rejectors", hm.TRIM), hm.ALIGN, ("set_rejectors", []), hm.ALIGN])
        assert w.ctx.rejector_stats() == []
