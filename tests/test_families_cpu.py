"""The table of likelihood families (manifold_gp_amd/families.py) is the single source of the family names, their codes in the
three code spaces of the C ABI, their data checks, the constant of their log-likelihood and the moments of a new count.  Host
code only: every check runs before the first device call, which a CPU tensor then refuses ("no CPU path")."""
import math
import types

import mpmath
import pytest
import torch

NAMES = ("bernoulli", "poisson", "binomial", "negative_binomial", "ordinal", "multiclass")
COUNT = {"poisson": 0, "binomial": 1, "negative_binomial": 2}
EVIDENCE = {"poisson": 0, "binomial": 1, "bernoulli": 2, "negative_binomial": 3}
SPECTRAL = {"bernoulli": 0, "poisson": 1, "binomial": 2, "negative_binomial": 3, "ordinal": 4}
UNKNOWN = ("softmax", "gaussian", "negative-binomial", "")
N = 6


def _fake_desc(n=N):
    from manifold_gp_amd.operators._descriptor import Descriptor
    sq = torch.ones(n)
    data = types.SimpleNamespace(dsqrt=sq, dinvsqrt=sq, graph=types.SimpleNamespace(n=n, device=torch.device("cpu")))
    return Descriptor(data=data, nu=2, kappa=1.0, form=0, noise=0.0)


def _model():
    from manifold_gp_amd.models import RiemannGP
    return RiemannGP.__new__(RiemannGP)                        # the dispatch alone: no kernel, no data


def _fronts():
    """{front: (the names the table says it takes, name -> the call, the sorted names its refusal lists)}"""
    from manifold_gp_amd import counts as ct, evidence as ev, families, spectral_laplace as sl
    from manifold_gp_amd.models import RiemannGP
    from manifold_gp_amd.utils import laplace_train
    d, y, f, Z = _fake_desc(), torch.zeros(N), torch.zeros(N), torch.ones(N, 2)
    node = set(families.TABLE)
    return {
        "fit_counts": (set(families.codes("count")), lambda name: ct.fit_counts(d, y, family=name), sorted(COUNT)),
        "evidence_site": (set(families.codes("evidence")), lambda name: ev.evidence_site(f, y, None, None, None, 0.0, name), sorted(EVIDENCE)),
        "spectral_site": (set(families.codes("spectral")), lambda name: sl.spectral_site(Z, torch.zeros(2), name, y), sorted(SPECTRAL)),
        "spectral_laplace_fit": (set(families.codes("spectral")), lambda name: sl.spectral_laplace_fit(Z, y, family=name), sorted(SPECTRAL)),
        "RiemannGP.laplace_evidence": (node, lambda name: RiemannGP.laplace_evidence(_model(), family=name), sorted(EVIDENCE)),
        "laplace_train": (node, lambda name: laplace_train(_model(), None, family=name), sorted(EVIDENCE)),
    }


def _refused_by_name(call, name):
    """the message when the front refuses the family's NAME, None when it gets past the name check (any later refusal -- a missing
    argument, the device -- comes after it)"""
    try:
        call(name)
    except ValueError as err:
        return str(err) if str(err).startswith("family must be one of") else None
    except Exception:
        return None
    return None


def test_the_table_holds_the_six_families():
    from manifold_gp_amd import families
    assert tuple(families.TABLE) == NAMES and all(rec.name == name for name, rec in families.TABLE.items())


@pytest.mark.parametrize("front", ["fit_counts", "evidence_site", "spectral_site", "spectral_laplace_fit", "RiemannGP.laplace_evidence",
                                   "laplace_train"])
def test_every_front_takes_the_names_the_table_gives_it(front):
    supported, call, listed = _fronts()[front]
    accepted = {name for name in NAMES if _refused_by_name(call, name) is None}
    assert accepted == supported, front
    for name in UNKNOWN:
        assert _refused_by_name(call, name) == "family must be one of %s, got %r" % (listed, name), (front, name)
        with pytest.raises(ValueError, match="family must be one of"):
            call(name)


def test_the_codes_of_the_three_spaces():
    from manifold_gp_amd import counts as ct, evidence as ev, families, spectral_laplace as sl
    assert families.codes("count") == COUNT and families.codes("evidence") == EVIDENCE and families.codes("spectral") == SPECTRAL
    for space, table in (("count", COUNT), ("evidence", EVIDENCE), ("spectral", SPECTRAL)):
        for name, rec in families.TABLE.items():
            if name in table:
                assert getattr(rec, space) == table[name] == rec.code(space) and type(rec.code(space)) is int
            else:
                assert getattr(rec, space) is None
                with pytest.raises(ValueError, match="has no %s code" % space):
                    rec.code(space)
    with pytest.raises(ValueError, match="has no"):
        families.TABLE["poisson"].code("name")
    # the constants that are read from outside are the table's
    assert ct.FAMILIES == COUNT and ct.NB == 2
    assert ev.FAMILIES == {"poisson": 0, "binomial": 1, "bernoulli": 2} and (ev.NB_FAMILY, ev.NB) == ("negative_binomial", 3)
    assert (ev.ORDINAL_FAMILY, ev.MULTICLASS_FAMILY) == ("ordinal", "multiclass")
    assert sl.FAMILIES == SPECTRAL and sl.COUNT_FAMILIES == ("poisson", "binomial", "negative_binomial")
    # entry points of their own
    assert {name: rec.own for name, rec in families.TABLE.items() if rec.own} == {"negative_binomial": "nb", "ordinal": "ordinal",
                                                                                  "multiclass": "softmax"}
    # every fit object names its row
    from manifold_gp_amd.classification import LaplaceFit, MulticlassLaplaceFit
    from manifold_gp_amd.ordinal import OrdinalLaplaceFit
    assert (LaplaceFit.family, OrdinalLaplaceFit.family, MulticlassLaplaceFit.family) == ("bernoulli", "ordinal", "multiclass")


# ------------------------------------------------------------------------------------------------ node fit and spectral fit alike
def _base(family):
    """valid data of N = 6 rows: (y, keywords both fits take)"""
    if family == "bernoulli":
        return torch.tensor([0.0, 1.0, 1.0, 0.0, 1.0, 0.0]), {}
    if family == "ordinal":
        return torch.tensor([0.0, 1.0, 3.0, 2.0, 1.0, 0.0]), dict(num_categories=4, cutpoints=torch.tensor([-1.0, 0.0, 1.5]))
    y = torch.tensor([0.0, 3.0, 1.0, 7.0, 2.0, 5.0])
    if family == "binomial":
        return y, dict(trials=torch.tensor([1.0, 3.0, 4.0, 9.0, 2.0, 8.0]))
    kw = dict(exposure=torch.tensor([1.0, 0.5, 2.0, 4.0, 1.0, 3.0]))
    return y, dict(kw, dispersion=2.0) if family == "negative_binomial" else kw


def _bad_inputs(family):
    """(label, y, observed, keywords) of one bad input each"""
    y, kw = _base(family)

    def at(i, v):
        z = y.clone()
        z[i] = v
        return z
    cases = [("a mask that is not bool", y, torch.ones(N), kw), ("a mask of the wrong length", y, torch.ones(N - 1, dtype=torch.bool), kw),
             ("an empty mask", y, torch.zeros(N, dtype=torch.bool), kw),
             ("out of range", at(2, {"bernoulli": 2.0, "ordinal": 4.0}.get(family, -1.0)), None, kw),
             ("out of range behind a mask", at(2, {"bernoulli": -1.0, "ordinal": -1.0}.get(family, 2.0 ** 25)),
              torch.tensor([False, True, True, True, False, True]), kw)]
    if family in COUNT:
        cases.append(("a count that is no integer", at(1, 2.5), None, kw))
    if family == "binomial":
        cases += [("trials below the count", at(1, 4.0), None, kw),
                  ("exposure given to the binomial", y, None, dict(kw, exposure=torch.ones(N))),
                  ("trials missing", y, None, {})]
    if family in ("poisson", "negative_binomial"):
        cases += [("exposure of zero", y, None, dict(kw, exposure=torch.tensor([1.0, 0.0, 2.0, 4.0, 1.0, 3.0]))),
                  ("exposure negative", y, None, dict(kw, exposure=-kw["exposure"])),
                  ("trials given", y, None, dict(kw, trials=torch.full((N,), 9.0)))]
    if family == "negative_binomial":
        cases.append(("dispersion missing", y, None, {k: v for k, v in kw.items() if k != "dispersion"}))
    if family == "ordinal":
        cases += [("cutpoints that do not increase", y, None, dict(kw, cutpoints=torch.tensor([-1.0, 0.5, 0.5]))),
                  ("cutpoints that decrease", y, None, dict(kw, cutpoints=torch.tensor([1.0, 0.0, -1.0])))]
    return cases


def _both_fits(family, y, observed, kw):
    """the exceptions the node fit and the spectral fit raise"""
    from manifold_gp_amd import classification as cl, counts as ct, ordinal as od, spectral_laplace as sl
    d, Z = _fake_desc(), torch.ones(N, 2)
    if family == "bernoulli":
        node = lambda: cl.laplace_fit(d, y, observed)
    elif family == "ordinal":
        node = lambda: od.laplace_fit_ordinal(d, y, kw["num_categories"], kw["cutpoints"], observed)
    else:
        node = lambda: ct.fit_counts(d, y, observed, family=family, **kw)
    raised = []
    for fit in (node, lambda: sl.spectral_laplace_fit(Z, y, observed, family, **kw)):
        with pytest.raises((ValueError, RuntimeError)) as err:
            fit()
        raised.append(err.value)
    return raised


@pytest.mark.parametrize("family", ["bernoulli", "poisson", "binomial", "negative_binomial", "ordinal"])
def test_node_fit_and_spectral_fit_refuse_the_same_bad_input_alike(family):
    y, kw = _base(family)
    for err in _both_fits(family, y, None, kw):                 # valid data pass every check: the device refuses
        assert type(err) is RuntimeError and "no CPU path" in str(err), err
    for label, y, observed, kw in _bad_inputs(family):
        a, b = _both_fits(family, y, observed, kw)
        assert type(a) is type(b) is ValueError, (family, label, a, b)
        assert str(a) == str(b), (family, label)


# ------------------------------------------------------------------------------------------------ the constant and the moments
U = 2.0 ** -53
R_ENDS = (2.0 ** -10, 2.0 ** 20)


def _lg(x):
    return mpmath.loggamma(mpmath.mpf(x))


def test_the_constant_of_the_log_likelihood_against_mpmath():
    """Per node, in float64, against mpmath at 30 digits, and against the plain math.lgamma statement of the same formula.  The bar
    is the one tests/test_nb_cpu.py holds nb_log_constant to: 8 * 2^-53 (1 + |c| + k |log r| + k), the term with r absent for the
    families without one.  Rows: y = 0, y = trials, and the dispersion at both ends of [2^-10, 2^20]."""
    from manifold_gp_amd.families import TABLE
    mpmath.mp.dps = 30
    y = [0.0, 1.0, 5.0, 12.0, 40.0]
    trials = [7.0, 1.0, 12.0, 12.0, 40.0]                      # y = trials at three rows, y = 0 at the first
    yt, Nt = torch.tensor(y, dtype=torch.float64), torch.tensor(trials, dtype=torch.float64)

    def held(got, want, k, r=1.0):
        bar = 8.0 * U * (1.0 + abs(float(want)) + k * abs(math.log(r)) + k)
        return abs(float(mpmath.mpf(float(got)) - want)) <= bar

    got = TABLE["poisson"].constant(yt, None, None)
    assert got.dtype == torch.float64
    for k, c in zip(y, got.tolist()):
        assert held(c, -_lg(k + 1), k) and abs(c + math.lgamma(k + 1.0)) <= 8.0 * U * (1.0 + abs(c) + k), ("poisson", k)
    got = TABLE["binomial"].constant(yt, Nt, None)
    for k, n, c in zip(y, trials, got.tolist()):
        assert held(c, _lg(n + 1) - _lg(k + 1) - _lg(n - k + 1), k), ("binomial", k, n)
        assert abs(c - (math.lgamma(n + 1.0) - math.lgamma(k + 1.0) - math.lgamma(n - k + 1.0))) <= 8.0 * U * (1.0 + abs(c) + k)
    assert got[0] == 0.0 and got[3] == 0.0 and got[4] == 0.0    # C(N, 0) = C(N, N) = 1 exactly
    for r in R_ENDS + (1.5,):
        got = TABLE["negative_binomial"].constant(yt, None, r)
        for k, c in zip(y, got.tolist()):
            assert held(c, _lg(k + r) - _lg(r) - _lg(k + 1), k, r), ("negative_binomial", k, r)
        assert got[0] == 0.0
    cuts = torch.tensor([-1.5, -1.5 + 2.0 ** -20, 0.25, 3.0], dtype=torch.float64)
    labels = torch.tensor([0, 1, 2, 3, 4, 2])
    got = TABLE["ordinal"].constant(labels, None, cuts)
    gaps = [None, 2.0 ** -20, 1.75 - 2.0 ** -20, 2.75, None]
    for k, c in zip(labels.tolist(), got.tolist()):
        want = mpmath.mpf(0) if gaps[k] is None else mpmath.log(-mpmath.expm1(-mpmath.mpf(gaps[k])))
        assert held(c, want, 0.0), ("ordinal", k)
    assert TABLE["bernoulli"].constant is None and TABLE["multiclass"].constant is None


def test_the_moments_of_a_new_count_against_mpmath():
    """m = E exp(eta + v / 2), var = m + m^2 (e^v - 1) [+ m^2 e^v / r] in float64 against mpmath at 30 digits, with the exposure
    given and with its logarithm already in eta (the two ways the fits call it).  The bar is that of the constant,
    8 * 2^-53 (1 + |value|).  Rows: v = 0, a negative and a positive predictor, r at both ends of [2^-10, 2^20].
    The binomial moments N p, N p (1 - p) take p from the device quadrature (bernoulli_predict), which no CPU test reaches: they are
    held to their float64 restatement by tests/test_gpu_counts.py and tests/test_gpu_spectral_laplace.py (predict_mean)."""
    from manifold_gp_amd.families import TABLE, count_moments
    mpmath.mp.dps = 30
    eta = [0.0, -0.75, 0.5, 0.25, -0.125]
    v = [0.0, 0.5, 0.25, 1.0, 0.0625]
    E = [1.0, 0.5, 3.0, 2.0, 7.0]
    et, vt, Et = (torch.tensor(a, dtype=torch.float64) for a in (eta, v, E))
    for family, rs in (("poisson", (None,)), ("negative_binomial", R_ENDS + (1.5,))):
        for r in rs:
            for exposure, predictor in ((Et, et), (None, et + Et.log())):
                m, var = count_moments(TABLE[family], predictor, vt, exposure, r)
                assert m.dtype == var.dtype == torch.float64
                for i in range(len(eta)):
                    arg = mpmath.mpf(eta[i]) + mpmath.mpf(v[i]) / 2
                    wm = mpmath.mpf(E[i]) * mpmath.exp(arg)
                    wv = wm + wm * wm * mpmath.expm1(mpmath.mpf(v[i]))
                    if r is not None:
                        wv += wm * wm * mpmath.exp(mpmath.mpf(v[i])) / mpmath.mpf(r)
                    for got, want in ((m[i], wm), (var[i], wv)):
                        err = abs(float(mpmath.mpf(float(got)) - want))
                        assert err <= 8.0 * U * (1.0 + abs(float(want))), (family, r, i, err)
    # v = 0 and r = 2^20: the Poisson variance but for m^2 / r
    m, var = count_moments(TABLE["poisson"], et[:1], vt[:1], Et[:1])
    assert float(m) == 1.0 and float(var) == 1.0
