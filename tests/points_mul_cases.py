"""Case sets for dvp_points_mul (no GPU): the scalar set S, a plain-python width-w tau-NAF restated from the definition
(Solinas, "Efficient arithmetic on Koblitz curves", 2000, for mu = -1: tau^2 = -tau - 2), and lambda, the scalar tau acts as.
The recoder here CHOOSES cases (which digit values a scalar set reaches); results are checked against the integer
double-and-add of the C oracle, which shares nothing with any of it."""
import random

import pyref as o
import util

R = o.P  # the group order r (= the scalar field's modulus)
WIDTHS = (3, 4, 5)


# ---- Z[tau], elements as (a, b) = a + b tau -----------------------------------------------------------------------
def zt_mul(x, y):
    a, b = x
    c, d = y
    return (a * c - 2 * b * d, a * d + b * c - b * d)  # tau^2 = -tau - 2


def zt_norm(x):
    a, b = x
    return a * a - a * b + 2 * b * b  # N(a + b tau) = a^2 + mu a b + 2 b^2 with mu = -1


def zt_pow_tau(w):
    x = (1, 0)
    for _ in range(w):
        x = zt_mul(x, (0, 1))
    return x


def zt_div_tau(x):
    a, b = x
    assert a % 2 == 0
    h = a // 2
    return (b - h, -h)  # tau (c + d tau) = -2 d + (c - d) tau


def t_w(w):
    """the integer with tau = t_w (mod tau^w), i.e. t_w^2 + t_w + 2 = 0 (mod 2^w), t_w even: found by search (two roots, one even)"""
    roots = [t for t in range(1 << w) if (t * t + t + 2) % (1 << w) == 0 and t % 2 == 0]
    assert len(roots) == 1, roots
    return roots[0]


def alpha_table(w):
    """alpha_u = u mods tau^w for the odd u < 2^(w-1): the element of u + tau^w Z[tau] of least norm (ties: the lexicographically
    smallest (|beta|, |gamma|, beta, gamma) -- the identity checks hold for any representative)"""
    tw = zt_pow_tau(w)
    out = {}
    for u in range(1, 1 << (w - 1), 2):
        best = None
        for q0 in range(-4, 5):
            for q1 in range(-4, 5):
                m = zt_mul((q0, q1), tw)
                c = (u - m[0], -m[1])
                key = (zt_norm(c), abs(c[0]), abs(c[1]), c[0], c[1])
                if best is None or key < best:
                    best = key
        out[u] = (best[3], best[4])
    return out


def partial_reduce(k):
    """rho = k (mod delta) by exact rounding of k / delta in Z[tau] (any representative of the class is a valid input to the recoding)"""
    d0, d1 = util.TAU_D0, util.TAU_D1
    # k / delta = k conj(delta) / r, conj(delta) = (d0 - d1) - d1 tau
    c0, c1 = d0 - d1, -d1
    q0 = (2 * k * c0 + R) // (2 * R)
    q1 = (2 * k * c1 + R) // (2 * R)
    m = zt_mul((q0, q1), (d0, d1))
    return (k - m[0], -m[1])


def tnaf_w(k, w, alpha=None):
    """width-w tau-NAF of k mod delta: list of signed odd digits (0 for none), least significant first"""
    alpha = alpha or alpha_table(w)
    tw = t_w(w)
    r0, r1 = partial_reduce(k % R)
    digits = []
    while (r0, r1) != (0, 0):
        if r0 & 1:
            u = (r0 + r1 * tw) % (1 << w)
            if u >= 1 << (w - 1):
                u -= 1 << w
            s = 1 if u > 0 else -1
            b, g = alpha[abs(u)]
            r0 -= s * b
            r1 -= s * g
        else:
            u = 0
        digits.append(u)
        r0, r1 = zt_div_tau((r0, r1))
        assert len(digits) < 400
    return digits


def evaluate(digits, alpha, lam):
    """sum_j sign_j (beta_u + gamma_u lambda) lambda^j mod r"""
    acc = 0
    for d in reversed(digits):
        acc = acc * lam % R
        if d:
            b, g = alpha[abs(d)]
            acc = (acc + (1 if d > 0 else -1) * (b + g * lam)) % R
    return acc


_LAMBDA = None


def lam():
    """the root of x^2 + x + 2 mod r with lambda G = tau(G) = (Gx^2, Gy^2)"""
    global _LAMBDA
    if _LAMBDA is None:
        l0 = (-util.TAU_D0 * pow(util.TAU_D1, -1, R)) % R
        cands = [l0, (-1 - l0) % R]
        want = (o.gf_sqr(o.G_STD[0]), o.gf_sqr(o.G_STD[1]))
        hits = [l for l in cands if (l * l + l + 2) % R == 0 and o.k233_mul(l, o.G_STD) == want]
        assert len(hits) == 1, hits
        _LAMBDA = hits[0]
    return _LAMBDA


def scalar_cases(seed=2024):
    s = list(range(34))
    s += [R - 1, R - 2, R - 3, (R + 1) // 2, (R - 1) // 2]
    for k in (31, 32, 33, 63, 64, 65, 127, 128, 231):
        s += [1 << k, (1 << k) - 1]
    s += util.tau_adversarial_scalars()
    rnd = random.Random(seed)
    s += [rnd.randrange(R) for _ in range(64)]
    assert all(0 <= v < R for v in s)
    return s


def digit_values_seen(scalars, w):
    seen = set()
    a = alpha_table(w)
    for k in scalars:
        seen.update(d for d in tnaf_w(k, w, a) if d)
    return seen
