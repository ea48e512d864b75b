"""The likelihood families of the Laplace fits, each stated once: TABLE holds one record per family, and the node fits
(classification.py, counts.py, ordinal.py), their evidence (evidence.py), the spectral fit (spectral_laplace.py) and the model's
dispatch (RiemannGP.laplace_evidence, utils.laplace_train) read it.  Host code only: checks, float64 formulas, names.

A record says which code the family has in each of the three code spaces of the C ABI (include/mgp_hip.h: mgp_count_*,
mgp_laplace_evidence_site, mgp_spectral_site; None where it has none) and whether it has entry points of its own; what its data
are (`data`), its per-node auxiliary (`aux`) and its extra parameter (`extra`); the f-independent constant of its log-likelihood
(`constant`) and its float64 (g, h) (`gh`); and how a node fit of it is made and what its evidence needs (`fitter`, `forwards`,
`needs`, `live`, `evidence_of`: names, resolved when they are called for -- the modules they name import this one).
docs/scope.md, "Adding a likelihood family", lists what a new record goes with."""
import importlib
import inspect
import math

import torch

from ._lib import lib
from ._sites import _node_vector, _real, check_mask, picker

DISPERSION_MIN, DISPERSION_MAX = 2.0 ** -10, 2.0 ** 20
MAX_COUNT = 2 ** 24          # counts and trials are float32 on the device: integers are exact up to here
ETA_MAX = 700.0              # mu = exp(min(eta, ETA_MAX)) stays finite in float64
SPACES = ("count", "evidence", "spectral")


# ------------------------------------------------------------------------------------------------ the float64 formulas
def _sig(x):
    """(sigma(x), sigma(-x), sigma(x) sigma(-x)) in the dtype of x from one e = exp(-|x|), x = +-inf included"""
    e = torch.exp(-x.abs())
    d = 1.0 + e
    up = x >= 0
    return torch.where(up, 1.0 / d, e / d), torch.where(up, e / d, 1.0 / d), e / (d * d)


def _widths(b):
    """c_k = 1 - exp(-(b_{k+1} - b_k)) for the K categories of the cutpoints b [K - 1] (float64), 1 at the two ends"""
    one = torch.ones(1, dtype=b.dtype, device=b.device)
    return torch.cat([one, -torch.expm1(-(b[1:] - b[:-1])), one])


_STIRLING = (1.0 / 12, -1.0 / 360, 1.0 / 1260, -1.0 / 1680, 1.0 / 1188, -691.0 / 360360)


def _stirling_s(x):
    zi = 1.0 / x
    z2 = zi * zi
    s = _STIRLING[5]
    for c in _STIRLING[4::-1]:
        s = c + z2 * s
    return zi * s


def nb_log_constant(k, r):
    """c(k, r) = lgamma(k + r) - lgamma(r) - lgamma(k + 1) of a float64 tensor of counts k and the scalar dispersion r, in the
    form of the device's nb_const (csrc/count_predict.hip): sum_{j < k} log((r + j) / (j + 1)) for k < 32, Stirling differences
    beyond it -- no term is larger than the result's scale, where lgamma(k + r) and lgamma(r) are 1.3e7 each at r = 2^20."""
    k = k.to(torch.float64)
    r = float(r)
    small = torch.zeros_like(k)
    for j in range(31):
        small = small + torch.where(k > j, torch.full_like(k, math.log((r + j) / (j + 1.0))), torch.zeros_like(k))
    kk = k.clamp_min(32.0)                                # (the branch not taken stays finite)
    x = kk + r
    if r >= 33.0:
        big_r = (x - 0.5) * torch.log1p(kk / r) + kk * math.log(r) - kk + (_stirling_s(x) - _stirling_s(r)) - torch.lgamma(kk + 1.0)
    else:
        big_r = torch.zeros_like(k)
    y, d = kk + 1.0, r - 1.0
    big_k = (x - 0.5) * torch.log1p(d / y) + d * torch.log(y) - d + (_stirling_s(x) - _stirling_s(y)) - math.lgamma(r)
    return torch.where(k < 32.0, small, torch.where(kk + 1.0 <= r, big_r, big_k))


# (g, h) = (d l / d eta, -d2 l / d eta2) in float64 with the formulas of the site kernels: gh(eta, a, b, param) with eta the
# linear predictor (the mean and the log-exposure in it), a the labels, the counts or the lower ends of the intervals, b the
# trials or the upper ends, param the dispersion
def _bernoulli_gh(f, y, b, param):
    e = torch.exp(-f.abs())
    h = e / (1.0 + e) ** 2
    t = (torch.nan_to_num(y.double(), nan=0.0) > 0.5).double()
    return t - torch.where(f >= 0, 1.0 / (1.0 + e), e / (1.0 + e)), h


def _poisson_gh(eta, y, b, param):
    mu = torch.exp(eta.clamp_max(ETA_MAX))
    return y - mu, mu


def _logit_gh(eta, y, fail, total):
    """y successes and `fail` failures of `total` at the logit eta"""
    e = torch.exp(-eta.abs())
    d = 1.0 + e
    pi = torch.where(eta >= 0, 1.0 / d, e / d)
    pib = torch.where(eta >= 0, e / d, 1.0 / d)
    return y * pib - fail * pi, total * e / (d * d)


def _ordinal_gh(f, lo, hi, param):
    _, sig_mu, hu = _sig(hi - f)
    sig_l, _, hl = _sig(lo - f)
    return sig_l - sig_mu, hu + hl


# ------------------------------------------------------------------------------------------------ the table
class Family:
    """One row of TABLE (module docstring).  count, evidence, spectral: the family's code in that space of the C ABI or None;
    own: the stem of its own entry points (mgp_<own>_*) or None."""

    def __init__(self, data, fitter, aux=None, extra=None, count=None, evidence=None, spectral=None, own=None, constant=None,
                 gh=None, forwards=None, needs=None, live=None, evidence_of="evidence.laplace_evidence"):
        self.name = None
        self.data, self.aux, self.extra = data, aux, extra
        self.count, self.evidence, self.spectral, self.own = count, evidence, spectral, own
        self.constant, self.gh = constant, gh
        self.fitter, self.forwards, self.needs, self.live, self.evidence_of = fitter, forwards, needs, live, evidence_of

    def code(self, space):
        """The family's code in `space` ("count", "evidence", "spectral"); a family without one raises."""
        value = getattr(self, space) if space in SPACES else None
        if value is None:
            raise ValueError("the %s family has no %s code" % (self.name, space))
        return value


_COUNT_FIT = dict(fitter="counts.fit_counts", forwards="counts.laplace_fit_counts")
# constant(a, b, param): the per-node constant of the log-likelihood in float64, with a the counts (the labels of the ordinal
# family), b the trials and param the dispersion or the cutpoints [K - 1]
TABLE = {
    "bernoulli": Family("labels", "classification.laplace_fit", evidence=2, spectral=0, gh=_bernoulli_gh),
    "poisson": Family("counts", aux="exposure", count=0, evidence=0, spectral=1, gh=_poisson_gh,
                      constant=lambda y, b, param: -torch.lgamma(y + 1.0), **_COUNT_FIT),
    "binomial": Family("counts", aux="trials", count=1, evidence=1, spectral=2,
                       gh=lambda eta, y, N, param: _logit_gh(eta, y, N - y, N), **_COUNT_FIT,
                       constant=lambda y, N, param: torch.lgamma(N + 1.0) - torch.lgamma(y + 1.0) - torch.lgamma(N - y + 1.0)),
    # y + r trials, r failures at z = eta - log r
    "negative_binomial": Family("counts", aux="exposure", extra="dispersion", count=2, evidence=3, spectral=3, own="nb",
                                gh=lambda eta, y, b, r: _logit_gh(eta - math.log(r), y, r, y + r),
                                constant=lambda y, b, r: nb_log_constant(y, r), live="counts._live_dispersion", **_COUNT_FIT),
    "ordinal": Family("categories", "ordinal.laplace_fit_ordinal", aux="interval", extra="cutpoints", spectral=4, own="ordinal",
                      gh=_ordinal_gh, constant=lambda labels, b, cuts: torch.log(_widths(cuts))[labels], needs="num_categories",
                      live="ordinal._live_cutpoints"),
    # names and dispatch only: the softmax solver, site and evidence code are classification.py's and evidence.py's
    "multiclass": Family("classes", "classification.laplace_fit_multiclass", own="softmax", needs="num_classes",
                         evidence_of="evidence.softmax_evidence"),
}
for _name, _rec in TABLE.items():
    _rec.name = _name


def codes(space, own=True):
    """{name: code} of the families with a code in `space`; own=False: without those that have entry points of their own"""
    return {name: rec.code(space) for name, rec in TABLE.items() if getattr(rec, space) is not None and (own or rec.own is None)}


def with_own(own):
    """The name of the family whose entry points are mgp_<own>_*"""
    return next(name for name, rec in TABLE.items() if rec.own == own)


def _family(family, space):
    """The record of `family`, which must have a code in `space`"""
    rec = TABLE.get(family)
    if rec is None or getattr(rec, space) is None:
        raise ValueError("family must be one of %s, got %r" % (sorted(codes(space)), family))
    return rec


def fit_family(family):
    """The record of a family that has a node fit: every one of TABLE.  An unknown name gets the refusal of the evidence space,
    whose four names the message of RiemannGP.laplace_evidence and laplace_train has listed since before the other two had fits."""
    return TABLE[family] if family in TABLE else _family(family, "evidence")     # (never returns: the name is in no space)


# ------------------------------------------------------------------------------------------------ the kernel stages
_STAGES = {"site": ("mgp_count_site", "count"), "evidence_site": ("mgp_laplace_evidence_site", "evidence"),
           "predict_pmf": ("mgp_count_predict_pmf", "count"), "predict_logpmf": ("mgp_count_predict_logpmf", "count")}


def stage(rec, name, dispersion=None):
    """(entry point, its name, its workspace function or None, its family argument) of a stage of _STAGES: the family's own
    entry point with its dispersion where it has one (mgp_nb_*), the shared one with the family's code of that space otherwise."""
    shared, space = _STAGES[name]
    entry, arg = ("mgp_%s_%s" % (rec.own, name), dispersion) if rec.own else (shared, rec.code(space))
    return getattr(lib(), entry), entry, getattr(lib(), entry + "_workspace_bytes", None), arg


# ------------------------------------------------------------------------------------------------ the data and their checks
def check_dispersion(rec, dispersion):
    """float(dispersion) for a family that has one (required: a finite scalar in [2^-10, 2^20]); None for the others, which take
    none"""
    if rec.extra != "dispersion":
        if dispersion is not None:
            raise ValueError("dispersion belongs to the negative_binomial family")
        return None
    if dispersion is None:
        raise ValueError("the negative_binomial family needs dispersion=")
    r = _real(dispersion, "dispersion")
    if not DISPERSION_MIN <= r <= DISPERSION_MAX:            # (NaN fails the comparison)
        raise ValueError("dispersion must be a finite scalar in [2^-10, 2^20], got %r" % (dispersion,))
    return r


def check_labels(y, observed, n):
    """0/1 labels at the observed nodes: (y [n], observed [n] bool or None), on whatever device they came"""
    if not torch.is_tensor(y) or y.numel() != n:
        raise ValueError("y must be a tensor of %d labels, got %s" % (n, tuple(y.shape) if torch.is_tensor(y) else type(y)))
    y = y.reshape(-1)
    if check_mask(observed, n) is not None:
        observed = observed.to(y.device)
    seen = y if observed is None else y[observed]
    if not bool(((seen == 0) | (seen == 1)).all()):
        raise ValueError("labels at the observed nodes must all be 0 or 1")
    return y, observed


def check_aux(rec, n, exposure, trials, observed=None, training=False):
    """The exposure or the trials of a count family as float64 [n], None where none is given.  training=True: the nodes of a fit,
    the values checked at the observed ones and the messages saying so; False: test rows, all checked, in the spectral fit's words."""
    pick, where = picker(observed), " at the observed nodes" if training else ""
    if rec.aux != "trials":
        if trials is not None:
            raise ValueError("trials belong to the binomial family; the Poisson %s exposure"
                             % ("family takes" if training and rec.extra is None else "and negative_binomial families take"))
        extra = None if exposure is None else _node_vector(exposure, n, "exposure")
        if extra is not None and not bool((torch.isfinite(pick(extra)) & (pick(extra) > 0)).all()):
            raise ValueError("exposure%s must be finite and positive" % where)
        return extra
    if exposure is not None:
        raise ValueError("exposure belongs to the Poisson family; the binomial family takes trials")
    if trials is None:
        return None
    extra = _node_vector(trials, n, "trials")
    N = pick(extra)
    if not bool(((N >= 1) & (N <= MAX_COUNT) & (N == N.round())).all()):
        raise ValueError("trials%s must all be integers in [1, 2^24]" % where)
    return extra


def check_counts(rec, n, y, observed, exposure, trials):
    """Counts at the observed nodes with their exposure or trials: (y, observed, extra) with y and extra (None: none given)
    float64 [n] on the device they came on"""
    y = _node_vector(y, n, "y")
    if check_mask(observed, n) is not None:
        observed = observed.to(y.device)
    seen = picker(observed)(y)
    if not bool(((seen >= 0) & (seen <= MAX_COUNT) & (seen == seen.round())).all()):
        raise ValueError("counts at the observed nodes must all be integers in [0, 2^24]")
    extra = check_aux(rec, n, exposure, trials, observed, training=True)
    if rec.aux == "trials":
        if extra is None:
            raise ValueError("the binomial family needs trials")
        if not bool((picker(observed)(extra) >= seen.to(extra.device)).all()):
            raise ValueError("trials must be at least the counts at the observed nodes")
    return y, observed, extra


def count_moments(rec, eta, v, extra, dispersion=None, points=129):
    """(mean, var) of a new count of a count family, float64: eta the linear predictor at the mode and v its latent variance;
    extra the exposure (None: it is in eta already) or the trials.
    Poisson, in closed form (the rate is log-normal): m = E exp(eta + v / 2), var = m + m^2 (e^v - 1); the negative binomial adds
    m^2 e^v / r (E[mu^2] / r).  Binomial: p = int sigma(eta) N(eta; eta_hat, v) d eta by the trapezoid rule of bernoulli_predict
    (eta as float32, the kernel's input format), mean = N p, var = N p (1 - p): the variance of a draw with the success
    probability p."""
    if rec.aux == "trials":
        from .classification import bernoulli_predict
        p = bernoulli_predict(eta.float(), v, points)
        return extra * p, extra * p * (1.0 - p)
    m = torch.exp(eta + 0.5 * v)
    if extra is not None:
        m = extra * m
    var = m + m * m * torch.expm1(v)
    if rec.extra == "dispersion":
        var = var + m * m * torch.exp(v) / dispersion
    return m, var


# ------------------------------------------------------------------------------------------------ fits and their evidence
def _named(path):
    module, name = path.split(".")
    return getattr(importlib.import_module("." + module, __package__), name)


def fitter(rec):
    """The node fit of the family: fit(desc, y, observed=, **keywords)"""
    fit = _named(rec.fitter)
    if rec.count is None:
        return fit
    return lambda desc, y, **kw: fit(desc, y, family=rec.name, **kw)


def fit_keywords(rec):
    """The names of the fit's parameters, those of the function it forwards its **kw to included (and no **kw itself)"""
    paths = (rec.fitter,) if rec.forwards is None else (rec.fitter, rec.forwards)
    return {k for path in paths for k, p in inspect.signature(_named(path)).parameters.items() if p.kind is not p.VAR_KEYWORD}


def check_needs(rec, kw):
    if rec.needs is not None and rec.needs not in kw:
        raise ValueError("family %r needs %s" % (rec.name, rec.needs))


def split_live(rec, fit_kw):
    """(fit_kw with the family's extra parameter as the values a fit takes, {its name: the live tensor} or {}): a parameter given
    as a module or as a tensor that requires grad is what the evidence differentiates."""
    if rec.live is None:
        return fit_kw, {}
    fit_kw, live = _named(rec.live)(fit_kw)
    return fit_kw, ({} if live is None else {rec.extra: live})


def evidence_of(rec):
    """The evidence function of the family's fits"""
    return _named(rec.evidence_of)
