"""float64 restatement of manifold_gp_amd/spectral_laplace.py (docs/kernels/spectral_laplace.md): the site formulas by way of
the node fits' restatements, what mgp_spectral_site leaves, the weight-space Newton iteration, and -- as an independent formula
-- the dense function-space Laplace fit and evidence on K = s Z_obs Z_obs^T (Rasmussen & Williams, algorithm 3.1).  Test
infrastructure, sized for a few thousand rows.

A problem is a dict d: family, a, b (what the kernel reads: float32 values held as float64; b None: zeros), obs (bool [n]),
mean, r (the dispersion or None), const (the sum of the likelihood's f-independent terms over the observed rows)."""
import numpy as np
from scipy.special import expit, gammaln

import _counts_ref as cref
import _laplace_ref as lref
import _nb_ref as nref
import _ordinal_ref as oref

FAMILIES = ["bernoulli", "poisson", "binomial", "negative_binomial", "ordinal"]
CODES = {f: i for i, f in enumerate(FAMILIES)}
EPS = 2.0 ** -52
# max |d sigma' / dx| = 1 / (6 sqrt 3): the Lipschitz constant of h = sigma (1 - sigma)
H_LIP = 1.0 / (6.0 * np.sqrt(3.0))


def site(d, f):
    """(l, g, h) per row in float64 at the latent values f (without the mean); 0 at unobserved rows"""
    fam, obs, mean = d["family"], d["obs"], d["mean"]
    f = np.asarray(f, np.float64)
    if fam == "bernoulli":
        t = np.where(obs, np.nan_to_num(d["a"]) > 0.5, False).astype(np.float64)
        return lref.site(f + mean, None, t, obs)
    if fam == "ordinal":
        return oref.site(f + mean, d["a"], d["b"], obs)
    if fam == "negative_binomial":
        return nref.site(f, d["a"], d["b"], obs, mean, d["r"])[:3]
    return cref.site(fam, f, d["a"], d["b"], obs, mean)[:3]


def h_prime_bound(d, f):
    """an upper bound of |dh / df| per row near f (0 at unobserved rows): the Lipschitz constant of the curvature"""
    fam, obs = d["family"], d["obs"]
    h = site(d, f)[2]
    y = np.where(obs, np.nan_to_num(d["a"]), 0.0)
    if fam == "poisson":
        lip = h                                                          # h' = mu = h
    elif fam == "binomial":
        lip = np.where(obs, np.nan_to_num(d["b"]), 0.0) * H_LIP
    elif fam == "negative_binomial":
        lip = (y + d["r"]) * H_LIP
    elif fam == "ordinal":
        lip = np.full(h.shape, 2.0 * H_LIP)
    else:
        lip = np.full(h.shape, H_LIP)
    return np.where(obs, lip, 0.0)


def site_outputs(Z, w, d):
    """What mgp_spectral_site leaves from the float32 Z (held as float64) and the float64 w: f, grad, hess, sums, and the sum of
    the absolute terms of each (the scale of its rounding): |z_ij w_j| per row, |g_i z_ij| per column, h_i |z_ij z_ik| per entry,
    sum |l_i|."""
    Z = np.asarray(Z, np.float64)
    f = Z @ w
    l, g, h = site(d, f)
    grad = Z.T @ g
    hess = Z.T @ (h[:, None] * Z)
    sums = np.array([l.sum(), np.abs(f).max()])
    aZ = np.abs(Z)
    scale = dict(f=aZ @ np.abs(w), grad=aZ.T @ np.abs(g), hess=aZ.T @ (h[:, None] * aZ), lp=np.abs(l).sum())
    return f, grad, hess, sums, scale


# ------------------------------------------------------------------------------------------------ weight space
def psi(Z, d, s, w):
    return site(d, Z @ w)[0].sum() - 0.5 * (w @ w) / s


def gradient(Z, d, s, w):
    return Z.T @ site(d, Z @ w)[1] - w / s


def hessian(Z, d, s, w):
    h = site(d, Z @ w)[2]
    return Z.T @ (h[:, None] * Z) + np.eye(Z.shape[1]) / s


def gradient_rounding(Z, d, s, w):
    """the rounding of an evaluated gradient in the 2-norm: 2^-52 times the norm of the sums of its absolute terms, times the
    log2 of their number (pairwise or blocked summation)"""
    g = site(d, Z @ w)[1]
    terms = np.abs(Z).T @ np.abs(g) + np.abs(w) / s
    return EPS * np.ceil(np.log2(Z.shape[0] + 2)) * np.linalg.norm(terms)


def newton(Z, d, s, rtol=1e-12, max_steps=100, w0=None):
    """The weight-space Newton iteration with step halving on psi, until max |grad| <= rtol times its value at w = 0.
    Returns (w, grad at w, trace): one (psi, relative gradient, step) per step."""
    Z = np.asarray(Z, np.float64)
    m = Z.shape[1]
    g0 = np.abs(gradient(Z, d, s, np.zeros(m))).max()
    w = np.zeros(m) if w0 is None else np.array(w0, np.float64)
    trace = []
    for _ in range(max_steps):
        g = gradient(Z, d, s, w)
        if np.abs(g).max() <= rtol * g0:
            break
        delta = np.linalg.solve(hessian(Z, d, s, w), g)
        cur, step = psi(Z, d, s, w), 1.0
        while psi(Z, d, s, w + step * delta) < cur - 1e-13 * abs(cur) and step > 2.0 ** -40:
            step *= 0.5
        w = w + step * delta
        trace.append((psi(Z, d, s, w), np.abs(gradient(Z, d, s, w)).max() / g0, step))
    return w, gradient(Z, d, s, w), trace


def weight_bound(s, grads, roundings=()):
    """|w_1 - w_2|_2 <= s (|grad psi(w_1)|_2 + |grad psi(w_2)|_2): psi is strongly concave with modulus 1 / s (A >= I / s), so
    |w - w_hat|_2 <= s |grad psi(w)|_2 for each; an evaluated gradient carries its rounding on top."""
    return s * (sum(np.linalg.norm(g) for g in grads) + sum(roundings))


def log_z(Z, d, s, w):
    """(log Z, scale): sum l + const - w.w / (2 s) - 1/2 logdet(s A) at w, and |sum l| + w.w / (2 s) + |logdet|"""
    ll = site(d, Z @ w)[0].sum()
    quad = 0.5 * (w @ w) / s
    sign, logdet = np.linalg.slogdet(s * hessian(Z, d, s, w))
    assert sign > 0
    return ll + d["const"] - quad - 0.5 * logdet, abs(ll) + quad + abs(logdet)


def latent(Zs, d, s, Z, w):
    """(eta, var) at the feature rows Zs: z* . w + mean and z*^T A^-1 z*"""
    Zs = np.asarray(Zs, np.float64)
    A = hessian(Z, d, s, w)
    return Zs @ w + d["mean"], np.einsum("ij,ij->i", Zs, np.linalg.solve(A, Zs.T).T)


# ------------------------------------------------------------------------------------------------ function space
def _restrict(d):
    obs = d["obs"]
    out = dict(d, a=np.asarray(d["a"])[obs], obs=np.ones(int(obs.sum()), bool))
    out["b"] = None if d["b"] is None else np.asarray(d["b"])[obs]
    return out


def dense_fit(Z, d, s, rtol=1e-12, max_steps=200):
    """The function-space Laplace fit on the observed rows alone: K = s Z_o Z_o^T (n_o x n_o, rank <= m), f = K a, Newton by
    algorithm 3.1 (B = I + W^1/2 K W^1/2, never K^-1) with step halving on psi(a) = sum l(K a) - a.K a / 2, until the weight-space
    gradient Z_o^T (g - a) is below rtol times its value at 0 in the max norm.  Returns dict(w = s Z_o^T a, grad, log_z, scale,
    a, f)."""
    Zo = np.asarray(Z, np.float64)[d["obs"]]
    do = _restrict(d)
    K = s * (Zo @ Zo.T)
    no = K.shape[0]

    def psi_a(a):
        f = K @ a
        return site(do, f)[0].sum() - 0.5 * (a @ f)

    a = np.zeros(no)
    g0 = np.abs(Zo.T @ site(do, np.zeros(no))[1]).max()
    for _ in range(max_steps):
        f = K @ a
        _, g, h = site(do, f)
        if np.abs(Zo.T @ (g - a)).max() <= rtol * g0:
            break
        sw = np.sqrt(h)
        B = np.eye(no) + sw[:, None] * K * sw[None, :]
        b = h * f + g
        a_new = b - sw * np.linalg.solve(B, sw * (K @ b))
        cur, step = psi_a(a), 1.0
        while psi_a(a + step * (a_new - a)) < cur - 1e-13 * abs(cur) and step > 2.0 ** -40:
            step *= 0.5
        a = a + step * (a_new - a)
    f = K @ a
    l, g, h = site(do, f)
    sw = np.sqrt(h)
    sign, logdet = np.linalg.slogdet(np.eye(no) + sw[:, None] * K * sw[None, :])
    assert sign > 0
    quad = 0.5 * (a @ f)
    return dict(w=s * (Zo.T @ a), grad=Zo.T @ (g - a), log_z=l.sum() + d["const"] - quad - 0.5 * logdet,
                scale=abs(l.sum()) + quad + abs(logdet), a=a, f=f)


# ------------------------------------------------------------------------------------------------ problems
def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def constant(family, a, b, obs, r=None, cuts=None, labels=None):
    if family == "bernoulli":
        return 0.0
    if family == "ordinal":
        return float(oref.log_widths(cuts)[labels][obs].sum())
    if family == "negative_binomial":
        return nref.constant(a, obs, r)
    if family == "poisson":
        return float(-gammaln(a[obs] + 1.0).sum())
    return float((gammaln(b[obs] + 1.0) - gammaln(a[obs] + 1.0) - gammaln(b[obs] - a[obs] + 1.0)).sum())


def problem(family, ftrue, obs, seed, mean=0.0, r=1.7, K=4):
    """Data of one family simulated from the latent values ftrue [n] with a seed, as the kernel reads them, and what the public
    fit takes: d plus y (labels / counts / categories), exposure, trials, cutpoints, num_categories (None where not used)."""
    rng = np.random.default_rng(seed)
    n = ftrue.shape[0]
    d = dict(family=family, obs=obs, mean=mean, r=None, b=None)
    pub = dict(y=None, exposure=None, trials=None, cutpoints=None, num_categories=None, dispersion=None)
    if family == "bernoulli":
        y = (rng.random(n) < expit(ftrue + mean)).astype(np.float64)
        d.update(a=y, const=0.0)
    elif family == "poisson":
        E = rng.uniform(0.5, 20.0, n)
        y = rng.poisson(E * np.exp(np.minimum(ftrue + mean, 4.0))).astype(np.float64)
        d.update(a=y, b=f32(np.log(E)), const=constant(family, y, None, obs))
        pub["exposure"] = E
    elif family == "binomial":
        N = rng.integers(1, 40, n).astype(np.float64)
        y = rng.binomial(N.astype(np.int64), expit(ftrue + mean)).astype(np.float64)
        d.update(a=y, b=N, const=constant(family, y, N, obs))
        pub["trials"] = N
    elif family == "negative_binomial":
        E = rng.uniform(0.5, 20.0, n)
        mu = E * np.exp(np.minimum(ftrue + mean, 4.0))
        y = rng.poisson(rng.gamma(r, mu / r)).astype(np.float64)
        d.update(a=y, b=f32(np.log(E)), r=r, const=constant(family, y, None, obs, r=r))
        pub.update(exposure=E, dispersion=r)
    else:
        s = ftrue + mean + rng.logistic(size=n)
        y = np.searchsorted(np.quantile(s, np.arange(1, K) / K), s).astype(np.int64)
        cuts = oref.cutpoints(y, K, obs)
        lo, hi = oref.intervals(y, cuts)
        d.update(a=lo.astype(np.float64), b=hi.astype(np.float64), const=constant(family, None, None, obs, cuts=cuts, labels=y))
        pub.update(cutpoints=cuts, num_categories=K)
    pub["y"] = y
    return d, pub
