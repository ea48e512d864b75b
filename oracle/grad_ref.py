"""CPU ORACLE (test infrastructure) -- float64 reference of the hyper-parameter gradient path.

The HIP gradient chain (csrc/laplacian.hip `lap_tangent_pass`, the fused SpMM on the tangent CSR, `mgp_spmm_backward_sums`,
autograd._FusedSpmm / _NodeVector, the wrappers) is checked against plain torch CPU float64 ops over the edge list, written the
way oracle/ref_torch.py::dense_model_precision writes the reference's cached properties (graph_laplacian_operator.py:52-106)
but sparse (gather / index_add: O(nnz C)), so that the same oracle runs on the 1.5k-node fixtures and on 150k-node graphs.

  laplacian_f64           the Laplacian's node vectors and per-edge values, differentiable in eps (real or complex eps)
  laplacian_tangent_f64   d/d eps of the same six arrays by forward-mode AD (torch.func.jvp) -- no hand-written derivative,
                          so it shares no derivation with the kernel -- plus a per-entry term scale that sizes tolerances
  laplacian_value_scale_f64   the same per-entry term scale and floor for the VALUES of the build (and the per-edge W, A, S)
  model_apply_f64         L, Q, Q2 or Q3 = Noise(Scale(Precision(L))) applied to a block V, differentiable in everything
"""
import torch

FLT_MIN = 2.0 ** -126          # smallest normal float32: an fp32 exponential below it is flushed or subnormal

NAMES = ("degree_unnorm", "degree", "diag", "dsqrt", "dinvsqrt", "triu")


def _edges(val, idx, eps):
    dt = eps.dtype if torch.is_tensor(eps) else torch.float64
    rdt = torch.float64
    val = torch.as_tensor(val).to(rdt)
    idx = torch.as_tensor(idx).to(torch.int64)
    return val, idx, dt


def laplacian_f64(val, idx, n, eps, self_loops=True):
    """graph_laplacian_operator.py:52-106 over the edge list (val [M] squared distances, idx [2, M] with idx[0] < idx[1]):
    dict of degree_unnorm D~, degree D, diag, dsqrt = sqrt(D), dinvsqrt = 1 / sqrt(D) [n] and triu = S [M] (the off-diagonal
    entries of L_sym, stored positive).  eps: 0-d float64 or complex128 tensor (may require grad / carry a tangent)."""
    val, idx, dt = _edges(val, idx, eps)
    r, c = idx[0], idx[1]
    w = torch.exp(-val.to(dt) / (4.0 * eps * eps))
    base = torch.ones(n, dtype=dt) if self_loops else torch.zeros(n, dtype=dt)
    dtil = base.index_add(0, r, w).index_add(0, c, w)
    a = w / (dtil[r] * dtil[c])
    self_a = dtil.pow(-2) if self_loops else torch.zeros(n, dtype=dt)
    deg = self_a.index_add(0, r, a).index_add(0, c, a)
    diag = (1.0 - self_a / deg) / (eps * eps) if self_loops else torch.ones(n, dtype=dt) / (eps * eps)
    dsqrt = deg.sqrt()
    return dict(degree_unnorm=dtil, degree=deg, diag=diag, dsqrt=dsqrt, dinvsqrt=1.0 / dsqrt,
                triu=a / (dsqrt[r] * dsqrt[c]) / (eps * eps))


def _term_scale(val, idx, n, eps, self_loops, lap, wmag, constants):
    """Per-entry sum of the magnitudes of the terms of the formula at the head of lap_tangent_pass, with |W| replaced by
    `wmag` (per edge) and the W-free terms included only when `constants`."""
    r, c = idx[0], idx[1]
    dt_, d_ = lap["degree_unnorm"], lap["degree"]
    e2 = eps * eps
    dw = wmag * val / (2.0 * e2 * eps)                                         # dW = W d2 / (2 eps^3)
    s_ddt = torch.zeros(n, dtype=torch.float64).index_add(0, r, dw).index_add(0, c, dw)
    am = wmag / (dt_[r] * dt_[c])
    s_da = dw / (dt_[r] * dt_[c]) + am * (s_ddt[r] / dt_[r] + s_ddt[c] / dt_[c])
    s_dd = torch.zeros(n, dtype=torch.float64).index_add(0, r, s_da).index_add(0, c, s_da)
    if self_loops:
        s_dd = s_dd + 2.0 * dt_.pow(-3) * s_ddt
    sq = torch.sqrt(d_[r] * d_[c])
    s_ds = (s_da + am * (0.5 * s_dd[r] / d_[r] + 0.5 * s_dd[c] / d_[c])) / (sq * e2) + 2.0 * am / (sq * e2) / eps
    if self_loops:
        s_diag = (2.0 * dt_.pow(-3) * s_ddt / d_ + dt_.pow(-2) * s_dd / (d_ * d_)) / e2
        if constants:
            s_diag = s_diag + 2.0 * (1.0 + dt_.pow(-2) / d_) / (e2 * eps)        # diag = (1 - D~^-2 / D) / eps^2
    else:
        s_diag = torch.full((n,), 2.0 / (e2 * eps) if constants else 0.0, dtype=torch.float64)
    return dict(degree_unnorm=s_ddt, degree=s_dd, diag=s_diag, dsqrt=0.5 * s_dd / d_.sqrt(),
                dinvsqrt=0.5 * s_dd / (d_ * d_.sqrt()), triu=s_ds)


VALUE_NAMES = NAMES + ("w", "a")


def _value_scale(val, idx, n, eps, self_loops, lap, wmag, constants):
    """The counterpart of _term_scale for the VALUES of mgp_laplacian_build (lap_pass) and mgp_edge_values: per entry, the sum of
    the magnitudes of the terms the entry is made of, each term counted with everything it is divided by -- a quantity q =
    f(D~, D, W) is moved by a perturbation of its inputs by sum |df/dx| s_x, with s_x the term scale of x -- with |W| replaced
    by `wmag` (per edge) and the W-free terms (the self loop's 1 in D~, D~^-2 in D, the two terms of diag) only when
    `constants`.  Keys: NAMES plus "w" (the weights W) and "a" (A = W / (D~_i D~_j)), the two per-edge arrays mgp_edge_values
    returns besides S."""
    r, c = idx[0], idx[1]
    dt_, d_ = lap["degree_unnorm"], lap["degree"]
    e2 = eps * eps
    base = 1.0 if (self_loops and constants) else 0.0
    s_dt = torch.full((n,), base, dtype=torch.float64).index_add(0, r, wmag).index_add(0, c, wmag)
    am = wmag / (dt_[r] * dt_[c])
    s_a = am * (1.0 + s_dt[r] / dt_[r] + s_dt[c] / dt_[c])                     # A = W / (D~_i D~_j)
    s_d = torch.zeros(n, dtype=torch.float64).index_add(0, r, s_a).index_add(0, c, s_a)
    if self_loops:
        s_d = s_d + dt_.pow(-2) * (base + 2.0 * s_dt / dt_)                    # D = D~^-2 + sum A
    sq = torch.sqrt(d_[r] * d_[c])
    s_s = (s_a + am * (0.5 * s_d[r] / d_[r] + 0.5 * s_d[c] / d_[c])) / (sq * e2)   # S = A / (sqrt(D_i D_j) eps^2)
    if self_loops:
        s_diag = (2.0 * dt_.pow(-3) * s_dt / d_ + dt_.pow(-2) * s_d / (d_ * d_)) / e2
        if constants:
            s_diag = s_diag + (1.0 + dt_.pow(-2) / d_) / e2                     # diag = (1 - D~^-2 / D) / eps^2
    else:
        s_diag = torch.full((n,), 1.0 / e2 if constants else 0.0, dtype=torch.float64)
    return dict(degree_unnorm=s_dt, degree=s_d, diag=s_diag, dsqrt=0.5 * s_d / d_.sqrt(), dinvsqrt=0.5 * s_d / (d_ * d_.sqrt()),
                triu=s_s, w=wmag, a=s_a)


def laplacian_value_scale_f64(val, idx, n, eps, self_loops=True):
    """(value, scale, floor) over VALUE_NAMES for the values of the Laplacian build, the way laplacian_tangent_f64 returns them for
    its tangent: the float64 arrays of laplacian_f64 (plus the weights "w" and the adjacency "a"), the per-entry term scale with
    a weight W = exp(-d2 / (4 eps^2)) counted as W (1 + d2 / (4 eps^2)), and the floor over the weights float32 holds only as
    subnormals or zero (W < 2^-126), each counted at 2^-126 (1 + d2 / (4 eps^2)).  eps: python / numpy scalar."""
    val, idx, _ = _edges(val, idx, torch.tensor(0.0, dtype=torch.float64))
    e = torch.tensor(float(eps), dtype=torch.float64)
    value = dict(laplacian_f64(val, idx, n, e, self_loops))
    arg = val / (4.0 * e * e)
    w = torch.exp(-arg)
    value["w"] = w
    value["a"] = w / (value["degree_unnorm"][idx[0]] * value["degree_unnorm"][idx[1]])
    normal = w >= FLT_MIN
    scale = _value_scale(val, idx, n, e, self_loops, value, torch.where(normal, w, torch.zeros_like(w)) * (1.0 + arg), True)
    floor = _value_scale(val, idx, n, e, self_loops, value, torch.where(normal, torch.zeros_like(w), torch.full_like(w, FLT_MIN))
                         * (1.0 + arg), False)
    return value, scale, floor


def laplacian_tangent_f64(val, idx, n, eps, self_loops=True):
    """(value, tangent, scale, floor): dicts over NAMES of the float64 Laplacian at eps, its derivative wrt eps by forward-mode
    AD (torch.func.jvp of laplacian_f64), and two per-entry magnitudes that size an fp32 kernel's tolerance:

      scale  the sum of the magnitudes of the terms of lap_tangent_pass's formula, where a weight W = exp(-d2 / (4 eps^2))
             counts as W (1 + d2 / (4 eps^2)) -- an fp32 exponential amplifies the rounding of its argument by the argument --
             and diag = (1 - D~^-2 / D) / eps^2 by its two terms;
      floor  the same terms over the weights that float32 holds only as subnormals or zero (W < 2^-126), each counted at
             2^-126 (1 + d2 / (4 eps^2)): the float64 value of such a weight is below what the kernel can represent.

    eps: python / numpy scalar (evaluated at float64(eps))."""
    val, idx, _ = _edges(val, idx, torch.tensor(0.0, dtype=torch.float64))
    e = torch.tensor(float(eps), dtype=torch.float64)

    def f(x):
        d = laplacian_f64(val, idx, n, x, self_loops)
        return tuple(d[k] for k in NAMES)
    value, tangent = torch.func.jvp(f, (e,), (torch.ones((), dtype=torch.float64),))
    value, tangent = dict(zip(NAMES, value)), dict(zip(NAMES, tangent))
    arg = val / (4.0 * e * e)
    w = torch.exp(-arg)
    normal = w >= FLT_MIN
    scale = _term_scale(val, idx, n, e, self_loops, value, torch.where(normal, w, torch.zeros_like(w)) * (1.0 + arg), True)
    floor = _term_scale(val, idx, n, e, self_loops, value, torch.where(normal, torch.zeros_like(w), torch.full_like(w, FLT_MIN))
                        * (1.0 + arg), False)
    return value, tangent, scale, floor


def underflow_eps(val, median_arg=100.0):
    """A bandwidth at which the median weight exp(-d2 / (4 eps^2)) is exp(-median_arg): with the default, most weights are
    below the smallest normal float32 (2^-126 = exp(-87.3)); with self loops every D~ is still >= 1."""
    v = torch.as_tensor(val).to(torch.float64)
    return float(torch.sqrt(v.median() / (4.0 * median_arg)))


def laplacian_apply_f64(lap, idx, V, normalization="symmetric", transposed=False):
    """L V for the Laplacian arrays `lap` (laplacian_f64): L_sym = diag - S - S^T; random walk L = D^-1/2 L_sym D^1/2, its
    transpose D^1/2 L_sym D^-1/2 (graph_laplacian_operator.py:108-124)."""
    idx = torch.as_tensor(idx).to(torch.int64)
    r, c = idx[0], idx[1]
    s = lap["triu"].view(-1, 1)

    def lsym(X):
        out = lap["diag"].view(-1, 1) * X
        out = out - torch.zeros_like(X).index_add(0, r, s * X[c]) - torch.zeros_like(X).index_add(0, c, s * X[r])
        return out
    if normalization == "symmetric":
        return lsym(V)
    sq, isq = lap["dsqrt"].view(-1, 1), lap["dinvsqrt"].view(-1, 1)
    return sq * lsym(V * isq) if transposed else isq * lsym(V * sq)


def model_apply_f64(val, idx, n, eps, kappa, outputscale, noise, nu, normalization="randomwalk", self_loops=True, V=None,
                    transposed=False, stop="Q3"):
    """Q3 V with Q3 = Q2 - noise Q2^2 + noise^2 Q2^3, Q2 = outputscale Q, Q = (2 nu / kappa^2 I + L)^nu (x D for random walk):
    riemann_gp.py:32-39 / precision_matern_operator.py:26-37 / scale_wrapper_operator.py:27 / noise_wrapper_operator.py:22 --
    what dense_model_precision builds densely -- applied to V [n, C] through the edge list, differentiable in eps, kappa,
    outputscale, noise (0-d float64 tensors) and V.  transposed: L^T in place of L (random walk).  stop: "L", "Q", "Q2" or
    "Q3" (the product that is returned)."""
    lap = laplacian_f64(val, idx, n, eps, self_loops)
    V = torch.as_tensor(V).to(torch.float64)
    squeeze = V.dim() == 1
    V = V.view(-1, 1) if squeeze else V

    def lapply(X):
        return laplacian_apply_f64(lap, idx, X, normalization, transposed)

    def q(X):
        tau = 2.0 * nu / (kappa * kappa)
        out = X
        for _ in range(int(nu)):
            out = tau * out + lapply(out)
        return lap["degree"].view(-1, 1) * out if normalization == "randomwalk" else out

    if stop == "L":
        out = lapply(V)
    elif stop == "Q":
        out = q(V)
    else:
        def q2(X):
            return outputscale * q(X)
        out = q2(V) if stop == "Q2" else q2(V - noise * q2(V - noise * q2(V)))
        if stop not in ("Q2", "Q3"):
            raise ValueError("stop must be L, Q, Q2 or Q3")
    return out.view(-1) if squeeze else out


def bilinear_grads_f64(val, idx, n, theta, nu, normalization, self_loops, V, W, transposed=False, stop="Q3", chunk=64):
    """d<W, A V>/d theta for theta = (eps, kappa, outputscale, noise) and A = model_apply_f64(..., stop), by forward mode: the
    tangent T of A V along each hyper-parameter gives both the gradient <W, T> and the magnitude sum_i |W_i| |T_i| that sizes an
    fp32 evaluation's tolerance.  Returns (grads [4], scales [4]) as float64 numpy; columns in chunks of `chunk`."""
    import numpy as np
    base = [torch.tensor(float(t), dtype=torch.float64) for t in theta]
    V = torch.as_tensor(V).to(torch.float64)
    W = torch.as_tensor(W).to(torch.float64)
    V, W = (V.view(-1, 1), W.view(-1, 1)) if V.dim() == 1 else (V, W)
    grads, scales = np.zeros(4), np.zeros(4)
    for c0 in range(0, V.shape[1], chunk):
        Vc, Wc = V[:, c0:c0 + chunk], W[:, c0:c0 + chunk]
        for k in range(4):
            def f(x):
                th = list(base)
                th[k] = x
                return model_apply_f64(val, idx, n, *th, nu, normalization, self_loops, Vc, transposed=transposed, stop=stop)
            _, tan = torch.func.jvp(f, (base[k],), (torch.ones((), dtype=torch.float64),))
            grads[k] += float((Wc * tan).sum())
            scales[k] += float((Wc.abs() * tan.abs()).sum())
    return grads, scales


def wrapped_schur_quadform_f64(precision, v, mask, scale, noise):
    """<v, Noise(Scale(Schur(Q))) v> in closed form with T = scale * S (S the Schur complement on the labelled nodes `mask`,
    symmetric): f = <v, T v> - noise <v, T^2 v> + noise^2 <v, T^3 v>, and its derivatives wrt scale and noise.  `precision`: an
    oracle/sparse.py::SparsePrecision (converged float64 Schur matvecs).  Returns (f, df/dscale, df/dnoise) as floats."""
    import numpy as np
    v = np.asarray(v, np.float64)
    y1 = precision.schur_matmul(v, mask)
    y2 = precision.schur_matmul(y1, mask)
    q1, q2, q3 = float(v @ y1), float(y1 @ y1), float(y1 @ y2)
    s, z = float(scale), float(noise)
    f = s * q1 - z * s * s * q2 + z * z * s ** 3 * q3
    return f, q1 - 2.0 * z * s * q2 + 3.0 * z * z * s * s * q3, -s * s * q2 + 2.0 * z * s ** 3 * q3
