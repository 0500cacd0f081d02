"""NumPy restatement of the NDT More-Thuente step rule (icpgpu_set_ndt_line_search(ctx, ICPGPU_NDT_LINE_SEARCH_MORE_THUENTE); the
contract is DESIGN.md f6, "More-Thuente step rule"), written from that text and never calling the library.

`search` runs PCL's computeStepLengthMT with its loop running on any phi(a) and records, for every decision it takes (the Wolfe
tests, the closing of the interval, the trial-value case and its choices, the interval update, the clamps), how far the decision
was from its threshold.  A test pins a GPU result to this restatement only where every margin is clear, so that a flipped decision
means a bug and not rounding.  `align_mt` is NormalDistributionsTransform::computeTransformation under that rule, on top of
tests/ndt_restated.py's derivatives."""
import math

import numpy as np

import ndt_restated as nr

MU, NU, MAX_LOOP_TRIALS = 1e-4, 0.9, 10
TRIAL, WOLFE, INTERVAL, TRIAL_CAP, NAN_STEP, NON_FINITE = range(6)
EXIT_NAMES = {TRIAL: "trial", WOLFE: "wolfe", INTERVAL: "interval", TRIAL_CAP: "cap", NAN_STEP: "nan step", NON_FINITE: "non-finite"}


class Log:
    """Decisions of one search: (name, margin) with the margin in units of the quantity's scale (phi, phi' or the step range)."""

    def __init__(self, phi_scale, dphi_scale, step_scale):
        self.phi_scale, self.dphi_scale, self.step_scale = phi_scale, dphi_scale, step_scale
        self.decisions = []
        self.cases = []      # trial-value cases taken: 1 .. 4
        self.updates = []    # interval updates: "U1", "U2", "U3", "converged"
        self.clamps = []     # "max" / "min" when a candidate was clamped
        self.mute = False    # (comparisons of a trial with an interval end at the same step: the same pose, equal on any
                             #  deterministic evaluation, so a tie there is exact and no margin is kept)

    def _add(self, name, diff, scale):
        if diff != diff or self.mute:  # (a comparison with a NaN is false whatever the rounding: no margin to keep)
            return
        self.decisions.append((name, abs(diff) / scale if scale > 0 else math.inf))

    def f(self, name, x, y):     # a comparison of two phi / psi values
        self._add(name, x - y, self.phi_scale)

    def g(self, name, x, y):     # of two phi' / psi' values
        self._add(name, x - y, self.dphi_scale)

    def a(self, name, x, y):     # of two steps
        self._add(name, x - y, self.step_scale)

    def min_margin(self):
        return min((m for _, m in self.decisions), default=math.inf)


def _cubic(a_l, f_l, g_l, a_t, f_t, g_t):
    z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l
    w = np.sqrt(z * z - g_t * g_l)
    return a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w)


def _secant(a_l, g_l, a_t, g_t):
    return a_l - (a_l - a_t) / (g_l - g_t) * g_l


def trial_value(log, a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t):
    """trialValueSelectionMT: the next trial's step from the interval ends (l, u) and the last trial (t), in IEEE double (NumPy
    scalars: a division by zero or the square root of a negative number gives an infinity or a NaN, as in C)."""
    a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t = map(np.float64, (a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t))
    log.mute = a_t == a_l
    try:
        return _trial_value(log, a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t)
    finally:
        log.mute = False


def _trial_value(log, a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t):
    log.f("case1: f_t > f_l", f_t, f_l)
    if f_t > f_l:
        log.cases.append(1)
        a_c = _cubic(a_l, f_l, g_l, a_t, f_t, g_t)
        a_q = a_l - 0.5 * (a_l - a_t) * g_l / (g_l - (f_l - f_t) / (a_l - a_t))
        log.a("case1 choice", abs(a_c - a_l), abs(a_q - a_l))
        return a_c if abs(a_c - a_l) < abs(a_q - a_l) else 0.5 * (a_q + a_c)
    log.g("case2: g_t (a_l - a_t) > 0", g_t, 0.0)
    if g_t * (a_l - a_t) > 0:
        log.cases.append(2)
        a_c = _cubic(a_l, f_l, g_l, a_t, f_t, g_t)
        a_s = _secant(a_l, g_l, a_t, g_t)
        log.a("case2 choice", abs(a_c - a_t), abs(a_s - a_t))
        return a_c if abs(a_c - a_t) >= abs(a_s - a_t) else a_s
    log.g("case3: |g_t| <= |g_l|", abs(g_t), abs(g_l))
    if abs(g_t) <= abs(g_l):
        log.cases.append(3)
        a_c = _cubic(a_l, f_l, g_l, a_t, f_t, g_t)
        a_s = _secant(a_l, g_l, a_t, g_t)
        log.a("case3 choice", abs(a_c - a_t), abs(a_s - a_t))
        nxt = a_c if abs(a_c - a_t) < abs(a_s - a_t) else a_s
        guard = a_t + 0.66 * (a_u - a_t)
        log.a("case3 safeguard", guard, nxt)
        return min(guard, nxt) if a_t > a_l else max(guard, nxt)
    log.cases.append(4)
    return _cubic(a_u, f_u, g_u, a_t, f_t, g_t)


def update_interval(log, ends, a_t, f_t, g_t):
    """updateIntervalMT on ends = [a_l, f_l, g_l, a_u, f_u, g_u] (in place) -> True when the interval has converged."""
    log.mute = a_t == ends[0]
    try:
        return _update_interval(log, ends, a_t, f_t, g_t)
    finally:
        log.mute = False


def _update_interval(log, ends, a_t, f_t, g_t):
    a_l, f_l, g_l = ends[:3]
    log.f("update U1: f_t > f_l", f_t, f_l)
    if f_t > f_l:
        log.updates.append("U1")
        ends[3:] = [a_t, f_t, g_t]
        return False
    log.g("update U2/U3: sign of g_t (a_l - a_t)", g_t, 0.0)
    s = g_t * (a_l - a_t)
    if s > 0:
        log.updates.append("U2")
        ends[:3] = [a_t, f_t, g_t]
        return False
    if s < 0:
        log.updates.append("U3")
        ends[3:] = [a_l, f_l, g_l]
        ends[:3] = [a_t, f_t, g_t]
        return False
    log.updates.append("converged")
    return True


def _clamp(log, a, step_max, step_min):
    if not math.isnan(a):
        if a != step_max:            # (a candidate exactly on a bound gives the bound either way)
            log.a("clamp max", a, step_max)
        if min(a, step_max) != step_min:
            log.a("clamp min", min(a, step_max), step_min)
        if a > step_max:
            log.clamps.append("max")
        elif a < step_min:
            log.clamps.append("min")
    b = step_max if step_max < a else a        # std::min(a, step_max)
    return step_min if b < step_min else b     # std::max(b, step_min)


def search(fn, phi_0, d_phi_0, step_init, step_max, step_min, phi_scale=None, dphi_scale=None):
    """computeStepLengthMT with its loop running.  fn(a) -> (phi(a), phi'(a)) (any extra items are kept per trial); d_phi_0 < 0.
    -> dict(step, final (index of the accepted trial), exit, steps, phi, d_phi, extra, log)."""
    assert d_phi_0 < 0
    log = Log(phi_scale or max(abs(phi_0), 1.0), dphi_scale or abs(d_phi_0), max(step_max - step_min, step_max, 1e-300))
    psi = lambda a, f: f - phi_0 - MU * d_phi_0 * a      # noqa: E731
    dpsi = lambda g: g - MU * d_phi_0                     # noqa: E731
    ends = [0.0, psi(0.0, phi_0), dpsi(d_phi_0), 0.0, psi(0.0, phi_0), dpsi(d_phi_0)]
    is_open = True
    converged = (step_max - step_min) < 0
    steps, phis, dphis, extra = [], [], [], []
    a_t = _clamp(log, step_init, step_max, step_min)
    loop = 0
    while True:
        out = fn(a_t)
        phi_t, d_phi_t = float(out[0]), float(out[1])
        steps.append(a_t)
        phis.append(phi_t)
        dphis.append(d_phi_t)
        extra.append(out[2:])
        k = len(steps) - 1
        if not (math.isfinite(phi_t) and math.isfinite(d_phi_t)):
            final = 0 if k == 0 else k - 1
            return dict(step=steps[final], final=final, exit=NON_FINITE, steps=steps, phi=phis, d_phi=dphis, extra=extra, log=log)
        psi_t, dpsi_t = psi(a_t, phi_t), dpsi(d_phi_t)
        if k > 0:
            if is_open:
                log.f("close: psi_t <= 0", psi_t, 0.0)
                log.g("close: dpsi_t >= 0", dpsi_t, 0.0)
            if is_open and psi_t <= 0 and dpsi_t >= 0:
                is_open = False
                ends[1] = ends[1] + phi_0 - MU * d_phi_0 * ends[0]
                ends[2] = ends[2] + MU * d_phi_0
                ends[4] = ends[4] + phi_0 - MU * d_phi_0 * ends[3]
                ends[5] = ends[5] + MU * d_phi_0
            converged = update_interval(log, ends, a_t, *((psi_t, dpsi_t) if is_open else (phi_t, d_phi_t)))
            loop += 1
        log.f("wolfe: psi_t <= 0", psi_t, 0.0)
        log.g("wolfe: d_phi_t <= -nu d_phi_0", d_phi_t, -NU * d_phi_0)
        ex = None
        if psi_t <= 0 and d_phi_t <= -NU * d_phi_0:
            ex = WOLFE
        elif converged:
            ex = INTERVAL
        elif loop >= MAX_LOOP_TRIALS:
            ex = TRIAL_CAP
        else:
            with np.errstate(all="ignore"):
                nxt = trial_value(log, *ends, a_t, *((psi_t, dpsi_t) if is_open else (phi_t, d_phi_t)))
            nxt = _clamp(log, float(nxt), step_max, step_min)
            if math.isnan(nxt):
                ex = NAN_STEP
            else:
                a_t = nxt
        if ex is not None:
            return dict(step=a_t, final=k, exit=ex, steps=steps, phi=phis, d_phi=dphis, extra=extra, log=log)


# ---- NDT with the More-Thuente rule ---------------------------------------------------------------------------------------------
def direction(sums):
    """The Newton direction of the loop (ndt_restated.step's): -> (status, d (descending, unit), |delta|, d_phi_0 < 0 or 0)."""
    g = np.asarray(sums[2:8], np.float64)
    H = nr.symmetric(sums)
    if not (np.isfinite(H).all() and np.isfinite(g).all()):
        return nr.NAN, None, math.nan, 0.0
    U, S, Vt = np.linalg.svd(H)
    thr = max(S[0] * 6 * 2.0**-52, np.finfo(np.float64).tiny)
    keep = S > thr
    delta = Vt[keep].T @ ((U[:, keep].T @ -g) / S[keep])
    norm = math.sqrt(float(np.sum(delta * delta)))
    if norm == 0.0:
        return nr.ZERO, None, 0.0, 0.0
    if norm != norm:
        return nr.NAN, None, norm, 0.0
    d = delta / norm
    d_phi_0 = -float(g @ d)
    if d_phi_0 > 0:
        d, d_phi_0 = -d, -d_phi_0
    return nr.STEP, d, norm, d_phi_0


def align_mt(tg, src, max_iterations=35, transformation_epsilon=0.1, step_size=0.1, guess=None):
    """computeTransformation under the More-Thuente rule -> nr.align's dict plus trace (iteration, step, phi, d_phi per trial),
    trials, min_margin (the least margin of any line-search decision) and searches (the per-search results)."""
    src = np.asarray(src, np.float32)
    eps = transformation_epsilon
    Tf = np.eye(4, dtype=np.float32) if guess is None else np.asarray(guess, np.float32).copy()
    p = nr.initial_pose(guess)
    sums = nr.derivatives(tg, src, Tf, p)
    it, state, converged = 0, nr.NOT_CONVERGED, False
    trace, searches = [], []
    if sums[0] == 0:
        converged, state = True, nr.CONV_NO_CORRESPONDENCES
    else:
        while True:
            st, d, norm, d_phi_0 = direction(sums)
            if st == nr.ZERO:
                converged, state = True, nr.CONV_TRANSFORM
                break
            if st == nr.NAN:
                converged, state = False, nr.NOT_CONVERGED
                break
            a = 0.0
            if d_phi_0 != 0.0:
                x0 = p

                def fn(a_t, x0=x0, d=d):
                    x = x0 + d * a_t
                    T = nr.transform_float(x)
                    s = nr.derivatives(tg, src, T, x)
                    return -s[1], -float(s[2:8] @ d), x, T, s

                gscale = float(np.abs(sums[2:8]).sum())
                r = search(fn, -sums[1], d_phi_0, norm, step_size, eps / 2.0, dphi_scale=max(gscale, abs(d_phi_0)))
                searches.append(r)
                trace += [(it, r["steps"][i], r["phi"][i], r["d_phi"][i]) for i in range(len(r["steps"]))]
                p, Tf, sums = r["extra"][r["final"]]
                a = r["step"]
            cap = it > max_iterations
            if cap or (it and abs(a) < eps):
                converged, state = True, (nr.CONV_ITERATIONS if cap else nr.CONV_TRANSFORM)
                it += 1
                break
            it += 1
    margin = min((r["log"].min_margin() for r in searches), default=math.inf)
    return dict(T=Tf, iterations=it, state=state, converged=converged, n_corr=int(sums[0]), probability=sums[1] / len(src), p=p,
                trace=trace, trials=len(trace), min_margin=margin, searches=searches)


# ---- More & Thuente's (1994) test functions ---------------------------------------------------------------------------------------
def mt_function(k, beta=None):
    """phi(a) and phi'(a) of test functions 1, 2 and 4 of More & Thuente (1994, section 5; beta 2 and 0.004 as there) -> fn(a) ->
    (phi, phi')."""
    if beta is None:
        beta = {1: 2.0, 2: 0.004}.get(k)
    if k == 1:
        return lambda a: (-a / (a * a + beta), (a * a - beta) / (a * a + beta) ** 2)
    if k == 2:
        return lambda a: ((a + beta) ** 5 - 2 * (a + beta) ** 4, 5 * (a + beta) ** 4 - 8 * (a + beta) ** 3)
    if k == 4:  # phi0 of their family with l = 39, beta = 0.01 (the interval [1 - beta, 1 + beta] is where psi's minimum lies)
        b, l = 0.01, 39

        def f(a):
            if a <= 1 - b:
                p0, dp0 = 1 - a, -1.0
            elif a >= 1 + b:
                p0, dp0 = a - 1, 1.0
            else:
                p0, dp0 = (a - 1) ** 2 / (2 * b) + b / 2, (a - 1) / b
            s = 2 * (1 - b) / (l * math.pi) * math.sin(l * math.pi / 2 * a)
            ds = (1 - b) * math.cos(l * math.pi / 2 * a)
            return p0 + s, dp0 + ds
        return f
    raise ValueError(k)
