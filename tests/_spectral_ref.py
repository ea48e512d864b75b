"""float64 restatement of the spectral-feature kernels of csrc/features.hip, with the rounding bound of each entry.

Every function takes the kernel's own float32 inputs (arrays and scalars: a scalar is rounded to float32 first, as the C ABI
does), upcasts them and returns (want, bound), both float64.  Nothing here reads device output.

The bound.  With u = 2^-24 an fp32 sum of L terms, in any order, is within L u of the sum S of the terms' magnitudes (first
order); the 16 extra units pay for the handful of roundings outside the sums (products, divisions, square roots, the scalar
prefactors).  So

    bound = (L + 16) u S

where L counts every term that enters the entry -- the terms of its own sum and those of each normalising sum it is divided
by (the column norm, the spectral-density total, the test degree, the row sum of the extension weights) -- and S is the float64
sum of the entry's terms in magnitude.  A factor that passes through expf or powf is weighted by (1 + |argument|): the argument
is itself an fp32 number, and rounding it moves exp by |argument| u (powf(x, -nu) by nu u).  For a normalising sum of
exponentials the argument is the sum's weighted mean argument (that is what a rounding of every argument moves the sum by).

`exact_inputs` makes integer / dyadic operands for which every fp32 partial sum is exact whatever the order: the expected output
then follows from a few correctly rounded operations, and the long-n cases compare at 2 ulp (`ulp2`).
"""
import numpy as np

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126


def f32(x):
    """The float64 value of x after rounding to float32 (what a `float` parameter of the C ABI receives)."""
    return float(np.float32(x))


def _a(x):
    return np.asarray(x, dtype=np.float64)


def ulp2(want):
    """Two units in the last place of float32 at |want| (for a zero: 0, the result must be exact)."""
    w = np.abs(_a(want)).astype(np.float32)
    return np.where(w > 0, 2.0 * np.spacing(w).astype(np.float64), 0.0)


# ------------------------------------------------------------------------------ eigenvector post-processing
def postprocess(V, deg):
    """V[r, c] deg[r]^-1/2 / max(||column||_2, 1e-12).  L = n + 1: the n squares of the column norm and the entry itself."""
    V, deg = _a(V), _a(deg)
    W = V * (deg ** -0.5)[:, None]
    nrm = np.sqrt((W * W).sum(0))
    want = W / np.maximum(nrm, 1e-12)[None, :]
    return want, (V.shape[0] + 1 + 16) * U * np.abs(want)


# ------------------------------------------------------------------------------ spectral density
def _sqrt_density(evals, nu, kappa, n, eps_oos=None):
    """sqrt(n s_j / sum s) and its weight: (1 + nu) for the entry's own powf, (1 + nu) for the total's."""
    lam = _a(evals)
    kappa = f32(kappa)
    s = (2.0 * nu / (kappa * kappa) + lam) ** (-float(nu))
    if eps_oos is not None:
        e = f32(eps_oos)
        s = s / (1.0 - e * e * lam) ** 2
    return np.sqrt(s / s.sum() * n), s, (1.0 + nu) * (1.0 + nu)


def insample(evals, V, nu, kappa):
    """oracle.spectral.features_insample.  L = m + 1 (the m densities of the total, the entry)."""
    V = _a(V)
    n, m = V.shape
    sq, _, wgt = _sqrt_density(evals, nu, kappa, n)
    want = sq[None, :] * V
    return want, (m + 1 + 16) * U * wgt * np.abs(want)


def oos_weights(dtil, deg, d2, idx, eps, normalization):
    """The Nystrom extension weights c[T, k] (oracle.laplacian.out_of_sample), and per row the weight of their exponentials:
    (1 + arg_l) per term [T, k], times (1 + mean arg) for each of the two normalising sums [T]."""
    dtil, deg, d2 = _a(dtil), _a(deg), _a(d2)
    idx = np.asarray(idx, np.int64)
    e = f32(eps)
    arg = d2 / (4.0 * e * e)
    w = np.exp(-arg)
    dsum = w.sum(1)
    a = w / (dtil[idx] * dsum[:, None])
    s2 = a.sum(1)
    if normalization == 0:
        c = a / (np.sqrt(deg[idx]) * np.sqrt(s2)[:, None])
    else:
        c = a / s2[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_w = (w * arg).sum(1) / dsum
        mean_a = (a * arg).sum(1) / s2
    return c, (1.0 + arg), (1.0 + mean_w) * (1.0 + mean_a)


def bump(d2_first, eps, bump_scale, bump_decay):
    """torch_utils.bump_function at x = sqrt(d2_first) and its weight (1 + |b1|)(1 + |b2|) for the two exponentials."""
    d2_first = _a(d2_first)
    alpha = f32(bump_scale) * f32(eps)
    beta = f32(bump_decay)
    a2 = alpha * alpha
    b1 = beta / (d2_first - a2)
    b2 = -beta / a2
    return np.exp(b1) / np.exp(b2), (1.0 + np.abs(b1)) * (1.0 + np.abs(b2))


def support_f32(d2, eps, bump_scale):
    """The in-support decision as the kernel takes it: float32 sqrt(d2[:, 0]) < float32(bump_scale * eps)."""
    d2 = np.asarray(d2, np.float32)
    return np.sqrt(d2[:, 0]) < np.float32(bump_scale) * np.float32(eps)


def support_f64(d2, eps, bump_scale):
    return np.sqrt(_a(d2)[:, 0]) < f32(bump_scale) * f32(eps)


def oos(evals, V, nu, kappa, eps, normalization, dtil, deg, d2, idx, bump_scale, bump_decay, inside):
    """oracle.spectral.features_oos on the rows `inside` (bool [T], the caller's float32 support decision), 0 elsewhere.
    L = 3 k + m + 1: the k terms of the entry, of the test degree and of the weights' row sum, the m densities, the entry."""
    V = _a(V)
    n, m = V.shape
    idx = np.asarray(idx, np.int64)
    T, k = idx.shape
    inside = np.asarray(inside, bool)
    sq, _, wgt_s = _sqrt_density(evals, nu, kappa, n, eps)
    want = np.zeros((T, m))
    bound = np.zeros((T, m))
    rows = np.nonzero(inside)[0]
    if rows.size == 0:
        return want, bound
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c, wgt_t, wgt_r = oos_weights(dtil, deg, _a(d2)[rows], idx[rows], eps, normalization)
        b, wgt_b = bump(_a(d2)[rows, 0], eps, bump_scale, bump_decay)
        step = max(1, (1 << 22) // (k * m))
        for r0 in range(0, rows.size, step):
            sl = slice(r0, r0 + step)
            Vg = V[idx[rows[sl]]]                                   # [t, k, m]
            acc = np.einsum("tk,tkm->tm", c[sl], Vg)
            mag = np.einsum("tk,tkm->tm", np.abs(c[sl]) * wgt_t[sl], np.abs(Vg))
            want[rows[sl]] = sq[None, :] * acc * b[sl, None]
            S = sq[None, :] * mag * (b[sl] * wgt_b[sl] * wgt_r[sl])[:, None] * wgt_s
            bound[rows[sl]] = (3 * k + m + 1 + 16) * U * S
    return want, bound


def oos_nan_pattern_f32(evals, V, nu, kappa, eps, normalization, dtil, deg, d2, idx, bump_scale, bump_decay):
    """Where a float32 evaluation of the same formula (numpy float32 arithmetic, the reference's own precision) gives NaN: an
    in-support row whose k weights all underflow has test degree 0 and 0 / 0 weights."""
    f = np.float32
    V, d2 = np.asarray(V, f), np.asarray(d2, f)
    idx = np.asarray(idx, np.int64)
    n, m = V.shape
    e, kap = f(eps), f(kappa)
    lam = np.asarray(evals, f)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        s = np.power(f(2.0) * f(nu) / (kap * kap) + lam, -f(nu)) / (f(1.0) - e * e * lam) ** 2
        sq = np.sqrt(s / s.sum(dtype=f) * f(n))
        w = np.exp(d2 / (f(-4.0) * e * e))
        dsum = w.sum(1, dtype=f)
        a = w / (np.asarray(dtil, f)[idx] * dsum[:, None])
        s2 = a.sum(1, dtype=f)
        if normalization == 0:
            c = a / (np.sqrt(np.asarray(deg, f))[idx] * np.sqrt(s2)[:, None])
        else:
            c = a / s2[:, None]
        d1 = np.sqrt(d2[:, 0])
        alpha = f(bump_scale) * e
        a2 = alpha * alpha
        b = np.exp(f(bump_decay) / (d1 * d1 - a2)) / np.exp(-f(bump_decay) / a2)
        Z = sq[None, :] * (c[:, :, None] * V[idx]).sum(1, dtype=f) * b[:, None]
    Z[~(d1 < alpha)] = 0.0
    return np.isnan(Z)


# ------------------------------------------------------------------------------ the dense products
def kernel_diag(Z1, Z2, scale):
    """scale sum_j Z1[r, j] Z2[r, j].  L = m + 1."""
    p = _a(Z1) * _a(Z2)
    s = f32(scale)
    return s * p.sum(1), (p.shape[1] + 1 + 16) * U * abs(s) * np.abs(p).sum(1)


def lowrank_apply(Z, X, alpha, beta):
    """alpha Z (Z^T X) + beta X.  L = n + m + 2: the n terms of each t = Z^T X entry, the m terms of the row sum, the two
    scaled addends; S carries |Z|^T |X| for t, so that the error of t is counted at its own term magnitudes."""
    Z, X = _a(Z), _a(X)
    n, m = Z.shape
    a, b = f32(alpha), f32(beta)
    want = a * (Z @ (Z.T @ X)) + b * X
    S = abs(a) * (np.abs(Z) @ (np.abs(Z).T @ np.abs(X))) + abs(b) * np.abs(X)
    return want, (n + m + 2 + 16) * U * S


def lowrank_residual(Z, T, V, scale):
    """scale (V - Z T) with T float64: one fp32 rounding of the result plus the double-precision row sum,
    u |want| + (m + 4) 2^-53 |scale| sum_j |z_j t_j|."""
    Z, T, V = _a(Z), _a(T), _a(V)
    m = Z.shape[1]
    want = scale * (V - Z @ T)
    return want, U * np.abs(want) + (m + 4) * 2.0 ** -53 * abs(scale) * (np.abs(Z) @ np.abs(T))


# ------------------------------------------------------------------------------ exact inputs
def exact_inputs(kind, shape, seed):
    """Integer / dyadic float32 operands for which every fp32 partial sum of the kernel is exact in any order (all partial sums
    are integers, or multiples of 1/16, below 2^24 units).  Returns a dict of arrays and scalars.

      postprocess  (n, m)      V in {-1, 0, 1}, deg in {1, 4, 16}: the scaled entries are multiples of 1/4, their squares of 1/16
      kernel_diag  (n, m)      Z1 = (i % 17) - 5, Z2 in {-1, 0, 1}, scale 3
      apply        (n, m, C)   Z, X in {-1, 0, 1}: t = Z^T X are integers of at most n, the row sums of at most m n; alpha 1/2,
                               beta 2
      residual     (n, m, C)   Z in {-1, 0, 1}, T integers in [-3, 3] (float64), V = (i % 17) - 5, scale 1/2
    """
    rng = np.random.default_rng(seed)
    tri = lambda *s: rng.integers(-1, 2, size=s).astype(np.float32)           # noqa: E731
    ramp = lambda *s: ((np.arange(int(np.prod(s))) % 17) - 5.0).astype(np.float32).reshape(s)   # noqa: E731
    if kind == "postprocess":
        n, m = shape
        return dict(V=tri(n, m), deg=rng.choice(np.array([1.0, 4.0, 16.0], np.float32), size=n))
    if kind == "kernel_diag":
        n, m = shape
        return dict(Z1=ramp(n, m), Z2=tri(n, m), scale=3.0)
    if kind == "apply":
        n, m, C = shape
        return dict(Z=tri(n, m), X=tri(n, C), alpha=0.5, beta=2.0)
    if kind == "residual":
        n, m, C = shape
        return dict(Z=tri(n, m), T=rng.integers(-3, 4, size=(m, C)).astype(np.float64), V=ramp(n, C), scale=0.5)
    raise ValueError(kind)


def _two_orders(terms, axis):
    """float32 running sums of `terms` along `axis`, front to back and back to front: the last of each."""
    t = np.asarray(terms, np.float32)
    fwd = np.cumsum(t, axis=axis, dtype=np.float32)
    bwd = np.cumsum(np.flip(t, axis), axis=axis, dtype=np.float32)
    return np.take(fwd, -1, axis=axis), np.take(bwd, -1, axis=axis)


def exact_sums(kind, inp):
    """The sums the kernel forms on `exact_inputs` data, each as (float32 front to back, float32 back to front, float64):
    a list of such triples.  They are exact when all three are bit-equal (tests/test_spectral_kernels_cpu.py)."""
    f = np.float32
    out = []
    if kind == "postprocess":
        W = inp["V"] * (f(1.0) / np.sqrt(inp["deg"]))[:, None]
        assert np.array_equal(W.astype(np.float64), _a(inp["V"]) * (_a(inp["deg"]) ** -0.5)[:, None])
        sq = W * W
        out.append(_two_orders(sq, 0) + ((_a(W) ** 2).sum(0),))
    elif kind == "kernel_diag":
        p = inp["Z1"] * inp["Z2"]
        out.append(_two_orders(p, 1) + ((_a(inp["Z1"]) * _a(inp["Z2"])).sum(1),))
    elif kind == "apply":
        Z, X = inp["Z"], inp["X"]
        t64 = _a(Z).T @ _a(X)
        for c in range(X.shape[1]):
            out.append(_two_orders(Z * X[:, c:c + 1], 0) + (t64[:, c],))
            # the row sums of Z t: the largest partial sum is bounded by sum_j |t_j|
            out.append(_two_orders(Z * t64[:, c].astype(f)[None, :], 1) + (_a(Z) @ t64[:, c],))
    elif kind == "residual":
        Z, T = _a(inp["Z"]), inp["T"]
        for c in range(T.shape[1]):
            out.append(_two_orders(inp["Z"] * T[:, c].astype(f)[None, :], 1) + (Z @ T[:, c],))
    else:
        raise ValueError(kind)
    return out


# ------------------------------------------------------------------------------ the input sets of the GPU tests
# Built here so that tests/test_spectral_kernels_cpu.py can check, without a GPU, the properties the bounds rest on (the
# support decision is the same in float32 and float64, no normalising sum leaves the normal range, exact inputs are exact).
EPS_IN = 0.05                       # in-sample eigenvalues run up to 4 / eps^2 = 1600
INSAMPLE_M = (1, 3, 255, 256, 257, 1024)
INSAMPLE_NU = (1, 2, 3)
INSAMPLE_KAPPA = (0.05, 0.5, 20.0)

# (n, m, T, k): every k of {1, 2, 10, 255, 256, 257, 1024}, T of {1, 2, 257}, m of {1, 3, 100, 257, 1024}
OOS_SHAPES = ((1037, 1, 2, 1), (1037, 3, 2, 2), (300, 100, 257, 10), (1037, 257, 2, 255), (1037, 1024, 1, 256),
              (1037, 3, 2, 257), (1037, 1024, 2, 1024), (64, 257, 257, 2))

STRUCTURE = (("postprocess", (263_001, 5)), ("kernel_diag", (65_553, 3)), ("apply", (131_381, 3, 2)),
             ("apply", (65_553, 3, 2)), ("residual", (70_001, 3, 31)))


def eigenvalues(m, top):
    """lambda_0 = 0, the rest ascending (quadratically spaced) up to `top`; float32."""
    j = np.arange(m, dtype=np.float64)
    return (top * (j / max(m - 1, 1)) ** 2).astype(np.float32)


def insample_inputs(n, m, seed=0):
    rng = np.random.default_rng([seed, n, m])
    return dict(evals=eigenvalues(m, 4.0 / EPS_IN ** 2), V=rng.standard_normal((n, m)).astype(np.float32))


def neighbour_lists(n, T, k, rng):
    """[T, k] distinct node ids per row, including 0 and n - 1 (k = 1: one of the two, alternating by row)."""
    idx = np.empty((T, k), np.int32)
    for t in range(T):
        if k == 1:
            idx[t, 0] = 0 if t % 2 == 0 else n - 1
            continue
        mid = rng.choice(np.arange(1, n - 1), size=k - 2, replace=False) if k > 2 else np.empty(0, np.int64)
        row = np.concatenate([[0], mid, [n - 1]])
        idx[t] = row[rng.permutation(k)] if t % 2 else row
    return idx


def oos_inputs(n, m, T, k, seed=0, eps=0.5, bump_scale=4.0, bump_decay=1.0):
    """Random eigenvectors and degree arrays, hand-built neighbour lists, d2 ascending with sqrt(d2) <= alpha / 2 (so every
    row is in the support, the bump's argument is at most 4/3 beta / alpha^2 in magnitude and no weight is below e^-1);
    eigenvalues up to 1 / (4 eps^2), so that 1 - eps^2 lambda stays in [3/4, 1]."""
    rng = np.random.default_rng([seed, n, m, T, k])
    alpha = bump_scale * eps
    d2 = np.sort(rng.uniform(0.01, 1.0, size=(T, k)), axis=1) * (0.25 * alpha * alpha)
    return dict(evals=eigenvalues(m, 0.25 / eps ** 2), V=rng.standard_normal((n, m)).astype(np.float32),
                dtil=rng.uniform(1.0, 3.0, n).astype(np.float32), deg=rng.uniform(0.2, 2.0, n).astype(np.float32),
                d2=d2.astype(np.float32), idx=neighbour_lists(n, T, k, rng), eps=eps, bump_scale=bump_scale,
                bump_decay=bump_decay)


def oos_edge_inputs(seed=0):
    """The support edge: eps = 0.5, bump scale 4, alpha = 2, all representable.  Row 0 sits on a node (d2 = 0), row 1 at
    alpha / 2, row 2 exactly at alpha (d2 = 4), row 3 far outside with weights exp(-2500) and below.  k = 5, m = 7, n = 50."""
    inp = oos_inputs(50, 7, 4, 5, seed=seed)
    d2 = inp["d2"].copy()
    d2[0] = [0.0, 0.125, 0.25, 0.5, 0.75]
    d2[1] = [1.0, 1.25, 1.5, 2.0, 3.0]
    d2[2] = [4.0, 4.0, 5.0, 6.0, 7.0]
    d2[3] = [2500.0, 2600.0, 2700.0, 2800.0, 1.0e4]
    inp["d2"] = d2
    return inp


def oos_underflow_inputs(seed=0):
    """One in-support row whose weights all underflow float32: eps = 0.5, bump scale 32 (alpha = 16), d2 from 150 (sqrt
    12.2 < 16; exp(-150) = 7e-66 is 0 in float32), next to an ordinary row."""
    inp = oos_inputs(50, 7, 2, 5, seed=seed, bump_scale=32.0)
    d2 = inp["d2"].copy()
    d2[0] = [0.5, 1.0, 1.5, 2.0, 3.0]
    d2[1] = [150.0, 151.0, 152.0, 155.0, 160.0]
    inp["d2"] = d2
    return inp


def all_oos_inputs():
    """(name, inputs) of every features_oos input set the GPU file uses."""
    for shape in OOS_SHAPES:
        yield "oos%r" % (shape,), oos_inputs(*shape)
    yield "edge", oos_edge_inputs()
