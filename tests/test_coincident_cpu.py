"""Conditions on the coincident-point fixtures (tests/_coincident.py): they carry the self edges they claim, and the float64
matrix the reference applies on them is the well-defined, positive semi-definite one every GPU stage is compared with
(tests/test_gpu_coincident.py).  No GPU."""
import numpy as np
import pytest

import _coincident as co

LOOPS = (True, False)


@pytest.fixture(scope="module", params=sorted(co.FIXTURES))
def fx(request):
    return co.FIXTURES[request.param]()


def test_cloud300_self_edges():
    g = co.cloud300()
    assert g["self_nodes"].tolist() == [40, 41, 151, 299]
    I = g["knn_I"]
    assert I[41, :3].tolist() == [7, 40, 41] and I[299, :2].tolist() == [0, 299]       # the triple; first and last node


def test_dumbbell_dup_self_edges_and_tiles():
    g = co.dumbbell_dup()
    assert g["n"] == 1546 and int(g["k"]) == 10 and len(co.DUP_DST) == 12
    assert not set(co.DUP_DST) & set(co.DUP_SRC)
    assert g["self_nodes"].tolist() == sorted(co.DUP_DST)                            # every copy has a lower-indexed twin
    x = g["train_x"]
    pairs = [(s, d) for s, d in zip(co.DUP_SRC, co.DUP_DST) if np.array_equal(x[s], x[d])]
    assert len(pairs) == 12
    assert any(s // 16 == d // 16 for s, d in pairs)                                 # a pair inside one 16-row tile
    assert any(s // 64 != d // 64 and abs(s - d) < 64 for s, d in pairs)             # a pair across a 64-row tile boundary


def test_coo_self_edge_list():
    g = co.coo_self()
    idx, val = g["edge_index"], g["edge_value"]
    assert g["n"] == 65 and g["self_nodes"].tolist() == [0, 63, 64]
    assert (val[idx[0] == idx[1]] > 0).all()                                        # self edges with non-zero distance
    assert ((idx[0] == 64) | (idx[1] == 64)).sum() == 1                             # node 64: its self edge and nothing else
    assert (idx[0] <= idx[1]).all() and (np.diff(idx[0] * 65 + idx[1]) > 0).all()   # sorted, unique
    deg = np.bincount(np.concatenate([idx[0], idx[1]])[np.concatenate([idx[0] != idx[1]] * 2)], minlength=65)
    assert (deg[:64] == 2).all()                                                    # the ring


@pytest.mark.parametrize("name", co.KNN_FIXTURES)
def test_knn_fixtures_have_self_edges(name):
    g = co.FIXTURES[name]()
    n = g["n"]
    assert len(g["self_nodes"]) >= 3
    I, D = g["knn_I"], g["knn_D"]
    off = np.flatnonzero(I[:, 0] != np.arange(n))                                   # rows whose column 0 is not the row itself
    assert len(off) >= 3 and (D[off, 0] == 0).all()
    assert set(off.tolist()) == set(g["self_nodes"].tolist())
    idx, val = g["edge_index"], g["edge_value"]
    assert (val[idx[0] == idx[1]] == 0).all()                                       # coincident: squared distance 0
    assert (idx[0] <= idx[1]).all() and (np.diff(idx[0] * n + idx[1]) > 0).all()


@pytest.mark.parametrize("loops", LOOPS)
def test_dense_matrix_is_symmetric_psd(fx, loops):
    L = fx["dense"][("symmetric", loops)]
    assert np.abs(L - L.T).max() == 0.0
    w = np.linalg.eigvalsh(L)
    print("min eig %.2e max eig %.2e" % (w[0], w[-1]))
    assert w[0] >= -1e-12 * w[-1]


@pytest.mark.parametrize("loops", LOOPS)
def test_randomwalk_rows_sum_to_zero(fx, loops):
    """Within 1e-13 at eps = 0.5 (cloud300, coo_self: entries of 1 / eps^2 = 4).  The dumbbell's entries are 1 / eps^2 = 400, of
    which 1e-13 is less than two ulps: there the same bound relative to the entries, 1e-13 / 4 in units of 1 / eps^2."""
    L = fx["dense"][("randomwalk", loops)]
    worst = np.abs(L.sum(1)).max()
    bound = 1e-13 * max(1.0, 0.25 / float(fx["eps"]) ** 2)
    print("worst row sum %.2e (bound %.2e)" % (worst, bound))
    assert worst <= bound


@pytest.mark.parametrize("norm", co.NORMS)
@pytest.mark.parametrize("loops", LOOPS)
def test_diagonal_differs_from_diag_by_twice_the_self_value(fx, norm, loops):
    """diag(L) = diag_i - 2 S_ii at the self-edge nodes and diag_i everywhere else (to the rounding of (d - s) - s and of the
    random walk's scaling by sqrt(D) / sqrt(D): two ulps of the diagonal)."""
    lo = co.oracle(fx, norm, loops)
    nodes, s = co.self_values(fx, loops)
    assert np.array_equal(np.sort(nodes), fx["self_nodes"]) and (s > 0).all()
    want = lo.diag.copy()
    want[nodes] -= 2.0 * s
    got = np.diag(fx["dense"][(norm, loops)])
    assert np.abs(got - want).max() <= 2 * np.finfo(np.float64).eps * np.abs(lo.diag).max()
    other = np.setdiff1d(np.arange(fx["n"]), nodes)
    if norm == "symmetric":
        assert np.array_equal(got[other], lo.diag[other])
    assert (2.0 * s > 1e-3 * lo.diag[nodes]).all()                                   # a difference no tolerance hides
