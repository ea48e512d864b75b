"""float64 restatement of the dispersion gradient of the negative-binomial Laplace evidence (docs/kernels/counts.md, "Learning
the dispersion"; mgp_nb_dispersion_sums in csrc/laplace.hip): psi(y + r) - psi(r) operation by operation, the three rows with
the sums of their absolute terms, the dense gradient at the float64 mode and the float64 training loops the device's are
compared with.  Test infrastructure on top of _nb_ref.py, sized for the dumbbell fixtures.

    d log Z / dr =   sum_obs [ psi(y + r) - psi(r) + log(1 - pi) + pi - y (1 - pi) / r ]        row 0
                   - 1/2 sum_eff v [ pi (1 - pi) - h' / r ]                                       row 1: dh / dr at fixed f
                   - 1/2 sum_eff u [ h / r - pi ]                                                 row 2: dg / dr = h / r - pi
    v = diag(A^-1),  u = A^-1 (v o h'),  A = Q + H,  eff: observed and h >= H_FLOOR."""
import math

import numpy as np
import torch

import _evidence_ref as eref
import _nb_ref as nb

LIFT = 32                       # psi_diff: the sum of reciprocals up to here, the asymptotic series at arguments from here
# worst |psi_diff - mpmath at 50 digits| in units of 2^-53 |result| on the table of
# test_nb_dispersion_cpu.py::test_psi_diff_against_mpmath (at y = 32, r = 0.37: the 32-term sum), measured and printed there;
# the device bar of test_gpu_nb_dispersion.py is 4 x this constant
MEASURED_PSI_ULP = 3.7                  # (3.60)
DEVICE_PSI_ULP = 4 * MEASURED_PSI_ULP
# float64 Adam on the dense evidence of the fixture (test_nb_dispersion_cpu.py prints both): log Z gained by learn() from r = 16 in
# 30 steps at lr 0.1, and by train() in 10 epochs on (length scale, output scale, dispersion) from r = 16.  The device tests ask for
# half of each.
LEARN_GAIN = 43.05
TRAIN_GAIN = 33.69


def psi_tail(x):
    """log x - 1 / (2 x) - psi(x) for x >= 32, the Horner form of the device"""
    x2 = 1.0 / (x * x)
    return x2 * (1.0 / 12 - x2 * (1.0 / 120 - x2 * (1.0 / 252 - x2 * (1.0 / 240 - x2 * (1.0 / 132 - x2 * (691.0 / 32760))))))


def psi_diff(y, r):
    """psi(y + r) - psi(r) with the operations of the device's psi_diff: y an array of integers in 0 .. 2^24, r a scalar in
    [2^-10, 2^20].  y <= 32: sum_{j < y} 1 / (r + j), j ascending; beyond it sum_{j < k} 1 / (r + j) + log1p((y - k) / b) +
    (y - k) / (2 a b) + (t(b) - t(a)) with k = 32 for r < 32 and 0 otherwise, b = r + k, a = y + r."""
    y = np.asarray(y, np.float64)
    r = float(r)
    small = np.zeros(y.shape)
    for j in range(LIFT):
        small = np.where(y > j, small + 1.0 / (r + j), small)
    lift = 0.0
    k = LIFT if r < LIFT else 0
    for j in range(k):
        lift = lift + 1.0 / (r + j)
    b = r + k
    yy = np.maximum(y, LIFT + 1.0)                      # (the branch not taken stays in range)
    d = yy - k
    a = yy + r
    big = lift + np.log1p(d / b) + d / (2.0 * a * b) + (psi_tail(b) - psi_tail(a))
    return np.where(y <= LIFT, small, big)


def node_terms(f, y, aux, obs, mean, r, h_floor=eref.H_FLOOR):
    """dict of the per-node pieces in float64 (0 at unobserved nodes): psi, lse = log(1 - pi), pi, ypr = y (1 - pi) / r, pq =
    pi (1 - pi), h, hp, eff -- with the operations of DispersionNode"""
    f = np.asarray(f, np.float64)
    obs = np.ones(f.shape, bool) if obs is None else np.asarray(obs, bool)
    y = np.where(obs, np.nan_to_num(np.asarray(y, np.float64)), 0.0)
    a = np.zeros_like(f) if aux is None else np.where(obs, np.nan_to_num(np.asarray(aux, np.float64)), 0.0)
    z = f + mean + a - nb.log_r(r)
    az = np.abs(z)
    e = np.exp(-az)
    d = 1.0 + e
    pi = np.where(z >= 0, 1.0 / d, e / d)
    pib = np.where(z >= 0, e / d, 1.0 / d)
    lse = -(np.maximum(z, 0.0) + np.log1p(e))
    pq = e / (d * d)
    h = (y + r) * pq
    gap = -np.expm1(-az) / d
    hp = h * np.where(z >= 0, -gap, gap)
    zero = np.zeros_like(f)
    t = dict(psi=psi_diff(y, r), lse=lse, pi=pi, ypr=y * pib / r, pq=pq, h=h, hp=hp)
    t = {k: np.where(obs, v, zero) for k, v in t.items()}
    t["eff"] = obs & (h >= h_floor)
    return t


def dispersion_sums(f, y, aux, obs, var, u, mean, r, h_floor=eref.H_FLOOR):
    """(rows [3], scale [3]): the three rows of mgp_nb_dispersion_sums and the sums of the absolute values of the terms each is
    made of.  var, u: float64 [n] or None (the row is 0); entries at unobserved nodes are not read."""
    t = node_terms(f, y, aux, obs, mean, r, h_floor)
    eff = t["eff"]
    rows, scale = np.zeros(3), np.zeros(3)
    rows[0] = (((t["psi"] + t["lse"]) + t["pi"]) - t["ypr"]).sum()
    scale[0] = (np.abs(t["psi"]) + np.abs(t["lse"]) + np.abs(t["pi"]) + np.abs(t["ypr"])).sum()
    if var is not None:
        v = np.where(eff, np.nan_to_num(np.asarray(var, np.float64)), 0.0)
        rows[1] = (-0.5 * (v * np.where(eff, t["pq"] - t["hp"] / r, 0.0))).sum()
        scale[1] = (0.5 * np.abs(v) * np.where(eff, t["pq"] + np.abs(t["hp"]) / r, 0.0)).sum()
    if u is not None:
        w = np.where(eff, np.nan_to_num(np.asarray(u, np.float64)), 0.0)
        rows[2] = (-0.5 * (w * np.where(eff, t["h"] / r - t["pi"], 0.0))).sum()
        scale[2] = (0.5 * np.abs(w) * np.where(eff, t["h"] / r + t["pi"], 0.0)).sum()
    return rows, scale


def dispersion_gradient(Q, d, f0=None):
    """dict(rows [3], scale [3], total, f, v, u, log_z) of d log Z / dr at the dense float64 mode of the problem d (_nb_ref.data)"""
    f, z = nb.mode_log_z(Q, d, f0=f0)
    _, _, h, hp, _ = nb.site(f, d["y"], d["aux"], d["obs"], d["mean"], d["r"])
    Ainv = np.linalg.inv(Q + np.diag(h))
    v = np.diag(Ainv).copy()
    eff = d["obs"] & (h >= eref.H_FLOOR)
    u = Ainv @ np.where(eff, v * hp, 0.0)
    rows, scale = dispersion_sums(f, d["y"], d["aux"], d["obs"], v, u, d["mean"], d["r"])
    return dict(rows=rows, scale=scale, total=float(rows.sum()), f=f, v=v, u=u, log_z=z["value"])


def raw_dispersion(r):
    """rho = log r of counts.DispersionParameter"""
    return math.log(r)


def dispersion_of(rho, r0):
    """counts.DispersionParameter.forward on the float64 tensor rho started at log r0: r0 exp(rho - log r0), which is r0 itself
    until rho moves"""
    return (r0 * torch.exp(rho.clamp(math.log(nb.R_MIN), math.log(nb.R_MAX)) - math.log(r0))).clamp(nb.R_MIN, nb.R_MAX)


# the two training runs the device is compared with: learn_dispersion with the kernel fixed, and laplace_train on (length scale,
# output scale, dispersion) from the fixture's length scale at the output scale of a prior marginal variance of 1
LEARN = dict(r0=16.0, steps=30, lr=0.1)
TRAIN = dict(kappa0=0.5, scale0=9 * eref.TRAIN["scale0"], r0=16.0, steps=10, lr=0.1)


def learn(Q, c, r0, steps, lr):
    """counts.learn_dispersion in float64 with exact gradients: Adam(lr) on rho = log r from r0, Q fixed, loss -log Z / m, the mode
    re-fitted (warm-started) every step.  c: _nb_ref.nb_counts.  Returns the list of (r, dense log Z), one per step and one for
    the final dispersion."""
    rho = torch.tensor(raw_dispersion(r0), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([rho], lr=lr)
    f, trace = None, []
    for step in range(steps + 1):
        rt = dispersion_of(rho, r0)
        d = nb.data(c, float(rt))
        g = dispersion_gradient(Q, d, f0=f)
        f = g["f"]
        trace.append((d["r"], g["log_z"]))
        if step == steps:
            break
        m = int((d["obs"] & (nb.curvature(f, d) >= eref.H_FLOOR)).sum())
        opt.zero_grad()
        (-(g["total"] * rt) / m).backward()
        opt.step()
    return trace


def train(g, norm, nu, c, kappa0, scale0, r0, steps, lr):
    """_evidence_ref.train_f64 with the dispersion trained along: Adam(lr) on the raw length scale, the raw output scale and
    rho = log r together.  Returns the list of (kappa, scale, r, dense log Z), one per step and one for the final parameters."""
    raw = [torch.tensor(eref.softplus_inverse(v), dtype=torch.float64, requires_grad=True) for v in (kappa0, scale0)]
    rho = torch.tensor(raw_dispersion(r0), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam(raw + [rho], lr=lr)
    eps, f, trace = float(g["eps"]), None, []
    for step in range(steps + 1):
        kappa, scale = (torch.nn.functional.softplus(x) for x in raw)
        rt = dispersion_of(rho, r0)
        d = nb.data(c, float(rt))
        Qt = eref.dense_q(g, norm, nu, eps, kappa, scale)
        Q = Qt.detach().numpy()
        Q = 0.5 * (Q + Q.T)
        f = nb.newton(Q, d, f0=f)[0]
        z = nb.log_z(Q, f, d)
        trace.append((kappa.item(), scale.item(), d["r"], z["value"]))
        if step == steps:
            break
        _, _, h, hp, _ = nb.site(f, d["y"], d["aux"], d["obs"], d["mean"], d["r"])
        Ai, Qi = np.linalg.inv(Q + np.diag(h)), np.linalg.inv(Q)
        v = np.diag(Ai).copy()
        u = Ai @ np.where(d["obs"] & (h >= eref.H_FLOOR), v * hp, 0.0)
        G = float(dispersion_sums(f, d["y"], d["aux"], d["obs"], v, u, d["mean"], d["r"])[0].sum())
        ft, ut, M = torch.from_numpy(f), torch.from_numpy(u), torch.from_numpy(Qi - Ai)
        sur = 0.5 * ((ut - ft) @ (Qt @ ft)) + 0.5 * (M * Qt).sum() + G * rt
        opt.zero_grad()
        (-sur / z["m"]).backward()
        opt.step()
    return trace
