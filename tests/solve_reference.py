"""An exact statement of what the point-to-point solve owes its caller, from the 17 sums alone.  numpy and fractions only: nothing here
is shared with icpslam_amd/csrc/icp_solver.cpp or oracle/.

For sums = {n, sum p, sum q, sum q p^T (row = q), sum d2} the solve returns T = [R t; 0 1] with q ~ R p + t.  Umeyama's rule: R maximises
tr(R^T Sigma) over SO(3), Sigma = M / n - mu_q mu_p^T, and the maximum is opt = s0 + s1 + sign(det Sigma) s2 over Sigma's singular values;
t = mu_q - R mu_p.  Optimality holds for EVERY input: where the rotation is not determined (planar, collinear, tied singular values) any
maximiser passes, so no case has to be left out.

  Sigma, mag, sign(det Sigma), the trace and the translation bound are exact (fractions.Fraction over the doubles' values);
  s comes from numpy.linalg.svd of Sigma rounded once to double and scaled by a power of two (its error, below 4 u s0, is in the budget).

The caps come from the solver's structure (64 sweeps of 3 plane rotations, each orthogonal to 2 u, one completion step), not from its output:
  ORTH     = 512 u                   max |R^T R - I|
  DEFICIT  = (27 + 4 + 3 * 512) u -> 1600 u, in units of mag = max_ab |M_ab / n| + |mu_q,a mu_p,b| (the size of what Sigma subtracts):
             forming Sigma in double moves each entry by 3 u mag_ab (27 u mag in the trace), numpy's s adds 4 u, a nearly orthogonal R
             3 ORTH mag.
  t        within 4 u (|mu_q| + |R| |mu_p|) per component: two roundings of the means, three of the product, one of the difference.
A float32 transform (what an alignment, SCP or RSAC returns) is the double one rounded once per entry, u32 = 2^-24:
  ORTH32    = 8 u32
  DEFICIT32 = 9 u32                  first order: each of the nine entries of R is rounded once
  t         one float32 ulp of t, plus the double bound, plus sum_b ulp32(R_ab) / 2 |mu_p,b|: t was formed from the DOUBLE rotation, and the
            check can only rebuild mu_q - R mu_p from the rounded one -- the same nine roundings DEFICIT32 allows for."""
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
U32 = Fraction(1, 2 ** 24)
ORTH = 512 * U
DEFICIT = 1600 * U
ORTH32 = 8 * U32
DEFICIT32 = 9 * U32


def _det3(m):
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def _exponent(x: Fraction) -> int:
    """e with x / 2^e in (1/2, 2)."""
    return x.numerator.bit_length() - x.denominator.bit_length()


def scaled(x: Fraction, e: int) -> Fraction:
    return x / (1 << e) if e >= 0 else x * (1 << -e)


def singular_values(sigma):
    """numpy's singular values (descending, as Fractions) of an exact 3x3: rounded once to double after an exact power-of-two scaling."""
    amax = max(abs(x) for row in sigma for x in row)
    if amax == 0:
        return [Fraction(0)] * 3
    e = _exponent(amax)
    a = np.array([[float(scaled(x, e)) for x in row] for row in sigma], np.float64)
    return [scaled(Fraction(float(v)), -e) for v in np.linalg.svd(a, compute_uv=False)]


def _ulp32(x) -> Fraction:
    return Fraction(float(np.spacing(np.float32(abs(float(x))))))


def exact(sums) -> dict:
    """The exact quantities of a sums record (17 finite doubles, n >= 1)."""
    F = [Fraction(float(x)) for x in sums]
    n = F[0]
    mu_p = [F[1 + a] / n for a in range(3)]
    mu_q = [F[4 + a] / n for a in range(3)]
    M = [[F[7 + 3 * a + b] / n for b in range(3)] for a in range(3)]
    sigma = [[M[a][b] - mu_q[a] * mu_p[b] for b in range(3)] for a in range(3)]
    mag = max(abs(M[a][b]) + abs(mu_q[a] * mu_p[b]) for a in range(3) for b in range(3))
    det = _det3(sigma)
    sign = (det > 0) - (det < 0)
    s = singular_values(sigma)
    return dict(n=n, mu_p=mu_p, mu_q=mu_q, sigma=sigma, mag=mag, sign=sign, s=s, opt=s[0] + s[1] + sign * s[2])


def check(sums, T, f32: bool = False, extra_deficit=0, extra_t=(0, 0, 0), ex=None) -> dict:
    """Assert that the 4x4 transform T (row r, column c) is a solve of `sums`: to the double caps, or with f32=True to those of a double
    solve rounded to float32.  extra_deficit (in units of mag) and extra_t (per component) widen the two bounds for a caller whose T went
    through more roundings than one cast and who says which.  Returns what was measured: deficit (in u mag; u32 mag for float32), orth
    (in u), t (worst ratio to its bound)."""
    T = np.asarray(T)
    assert T.shape == (4, 4) and T.dtype in (np.float32, np.float64) and (f32 or T.dtype == np.float64), (T.shape, T.dtype)
    assert np.isfinite(T).all(), T
    assert T[3].tolist() == [0.0, 0.0, 0.0, 1.0], T[3]
    ex = ex or exact(sums)
    u, orth_cap, deficit_cap = (U32, ORTH32, DEFICIT32) if f32 else (U, ORTH, DEFICIT)
    R = [[Fraction(float(T[r, c])) for c in range(3)] for r in range(3)]
    t = [Fraction(float(T[r, 3])) for r in range(3)]

    orth = max(abs(sum(R[k][i] * R[k][j] for k in range(3)) - (i == j)) for i in range(3) for j in range(3))
    assert orth <= orth_cap, ("R^T R - I", float(orth / u), "u")
    assert _det3(R) > 0, ("det R", float(_det3(R)))

    trace = sum(R[a][b] * ex["sigma"][a][b] for a in range(3) for b in range(3))
    miss = abs(ex["opt"] - trace)
    assert miss <= (deficit_cap + extra_deficit) * ex["mag"], ("deficit", float(miss / (u * ex["mag"])) if ex["mag"] else float(miss), "u mag")

    worst_t = Fraction(0)
    for a in range(3):
        want = ex["mu_q"][a] - sum(R[a][b] * ex["mu_p"][b] for b in range(3))
        bound = 4 * U * (abs(ex["mu_q"][a]) + sum(abs(R[a][b]) * abs(ex["mu_p"][b]) for b in range(3))) + extra_t[a]
        if f32:
            bound += _ulp32(T[a, 3]) + sum(_ulp32(T[a, b]) / 2 * abs(ex["mu_p"][b]) for b in range(3))
        err = abs(t[a] - want)
        assert err <= bound, ("t", a, float(err), float(bound))
        if bound:
            worst_t = max(worst_t, err / bound)
    return dict(deficit=float(miss / (u * ex["mag"])) if ex["mag"] else 0.0, orth=float(orth / u), t=float(worst_t))


def check32(sums, T, **kw) -> dict:
    T = np.asarray(T)
    assert T.dtype == np.float32, T.dtype
    return check(sums, T, f32=True, **kw)
