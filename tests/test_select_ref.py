"""CPU: the fp64 oracle of the memory-selection kernels (tests/select_ref.py) against the textbook definitions and its own
properties, the margin condition tests/test_gpu_select.py's exact-pick fixtures rest on, and the importable surface."""
import numpy as np
import pytest

from tests.select_ref import EXACT_FIXTURES, HERDING, KCENTER, fixture, greedy, literal

MODES = [HERDING, KCENTER]


def _mean(X):
    return X.astype(np.float64).mean(axis=0)


def test_surface():
    import inspect
    import mafed_amd
    from mafed_amd import AGEM, ER, FeatureDistillation, MemorySelection, select_rows  # noqa: F401
    from mafed_amd.methods import CLMethod
    assert mafed_amd.selection.MemorySelection is MemorySelection
    sel = MemorySelection()
    assert (sel.method, sel.feature_space, sel.layer, sel.normalize, sel.batch_size) == ("herding", "both", -1, True, 32)
    for bad in (dict(method="random"), dict(features="audio")):
        with pytest.raises(ValueError):
            MemorySelection(**bad)
    for cls in (ER, FeatureDistillation):
        assert inspect.signature(cls.__init__).parameters["memory_selection"].default is None
    assert issubclass(AGEM, ER)
    assert len(CLMethod) == 4


@pytest.mark.parametrize("mode", MODES)
def test_greedy_equals_literal(mode):
    X = fixture(0, 8, 3)
    picks, values, _, _ = greedy(X, _mean(X), 8, mode)
    assert picks.tolist() == literal(X, 8, mode).tolist()
    assert sorted(picks.tolist()) == list(range(8)) and np.isfinite(values).all()


def test_herding_mean_beats_random_subsets():
    n, d, k = 1000, 64, 100
    X = fixture(1, n, d)
    mu = _mean(X)
    picks, _, _, _ = greedy(X, mu, k, HERDING)
    herd = np.linalg.norm(X[picks].astype(np.float64).mean(axis=0) - mu)
    rng = np.random.default_rng(7)
    rand = [np.linalg.norm(X[rng.choice(n, k, replace=False)].astype(np.float64).mean(axis=0) - mu) for _ in range(20)]
    assert herd < np.mean(rand) and herd < min(rand)


def test_kcenter_radius_is_non_increasing():
    X = fixture(2, 300, 16)
    _, values, last, _ = greedy(X, _mean(X), 60, KCENTER)
    assert (np.diff(values[1:]) <= 0).all()
    assert last.shape == (300,) and (last >= 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_duplicated_rows_lower_index_first(mode):
    X = fixture(3, 50, 5)
    X[47] = X[3]
    picks, _, _, _ = greedy(X, _mean(X), 50, mode)
    order = picks.tolist()
    assert order.index(3) < order.index(47)


@pytest.mark.parametrize("mode", MODES)
def test_nan_rows_are_never_picked(mode):
    X = fixture(4, 20, 4)
    mu = _mean(X)
    X[[2, 9, 19], 1] = np.nan
    picks, values, _, _ = greedy(X, mu, 20, mode)
    assert picks[-3:].tolist() == [-1, -1, -1] and np.isnan(values[-3:]).all()
    assert sorted(picks[:-3].tolist()) == [i for i in range(20) if i not in (2, 9, 19)]


@pytest.mark.parametrize("mode,seed,n,d,k", EXACT_FIXTURES)
def test_exact_pick_fixtures_have_margin(mode, seed, n, d, k):
    """Every pick of these fixtures beats its runner-up by a relative margin of at least 1e-3: four times the worst-case fp32 error
    (d + 3) 2^-23 of a score at d = 2048, so fp32 scores cannot reorder them and the GPU test may ask for the oracle's picks."""
    X = fixture(seed, n, d)
    picks, _, _, margins = greedy(X, _mean(X), k, mode)
    assert (picks >= 0).all()
    print("min margin", margins.min())
    assert margins.min() >= 1e-3
    assert 1e-3 >= 4 * (2048 + 3) * 2.0 ** -23
