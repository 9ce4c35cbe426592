"""CPU tests of the classifier's host side: the exported symbols, the label reader,
the metrics, the L-BFGS driver on the numpy restatement tests/clf_ref.py, and the fixture
tests/golden/clf_golden.npz (tests/golden/make_clf_golden.py).  No GPU, no scikit-learn."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import clf_ref as R  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "clf_golden.npz")))


@pytest.fixture(scope="module")
def objective(gold):
    y = gold["labels"][gold["train"]]

    def F(wb, dtype=np.float64):
        return R.objective_grad(gold["table"], gold["train"], y, gold["lo"], gold["scale"], wb, float(gold["l2"]), dtype)
    return F


def test_symbols_are_exported():
    from dynamicgraphrepresentationlearning_amd import _lib as L
    for name in ("wharf_clf_minmax", "wharf_clf_loss_grad", "wharf_clf_predict"):
        assert name in L.SIGNATURES and getattr(L.lib, name) is not None
    header = open(os.path.join(os.path.dirname(HERE), "include", "wharf_gpu.h")).read()
    for name in ("wharf_clf_minmax(", "wharf_clf_loss_grad(", "wharf_clf_predict(", "wharf_clf_params"):
        assert name in header


def test_read_labels_wiki():
    from dynamicgraphrepresentationlearning_amd import read_labels
    ids, y, classes = read_labels(os.path.join(GOLDEN, "wiki_labels.txt"))
    assert ids.dtype == np.uint32 and y.dtype == np.uint32
    np.testing.assert_array_equal(ids, np.arange(2405))
    assert len(classes) == 17 and (np.diff(classes) > 0).all()
    assert y.max() == 16 and np.bincount(y).min() == 9


def test_read_labels_remaps_in_ascending_label_value(tmp_path):
    from dynamicgraphrepresentationlearning_amd import read_labels
    p = tmp_path / "labels"
    p.write_text("7 40\n3 -2\n9 40\n1 5\n")
    ids, y, classes = read_labels(str(p))
    np.testing.assert_array_equal(ids, [7, 3, 9, 1])
    np.testing.assert_array_equal(classes, [-2, 5, 40])
    np.testing.assert_array_equal(y, [2, 0, 2, 1])


def test_metrics_match_sklearn_values(gold):
    from dynamicgraphrepresentationlearning_amd import metrics
    C = int(gold["m_classes"])
    cm = R.confusion(gold["m_true"], gold["m_pred"], C)
    assert cm[5].sum() > 0 and cm[:, 5].sum() == 0          # a class that is never predicted
    assert cm[6].sum() == 0 and cm[:, 6].sum() == 0          # a class in neither
    for m in (metrics(cm), R.metrics(cm)):
        got = [m["accuracy"], m["f1_macro"], m["f1_micro"], m["f1_weighted"]]
        np.testing.assert_allclose(got, gold["m_values"], rtol=0, atol=1e-12)


def test_metrics_zero_denominator():
    from dynamicgraphrepresentationlearning_amd import metrics
    m = metrics(np.array([[0, 2], [0, 0]]))   # class 0 never predicted, class 1 never true: both F1 are 0
    assert m == {"accuracy": 0.0, "f1_macro": 0.0, "f1_micro": 0.0, "f1_weighted": 0.0}


def test_fixture_optimum_is_at_least_as_stationary_as_the_recipe(gold, objective):
    f_opt, g_opt = objective(gold["W_opt"])
    f_rec, g_rec = objective(gold["W_recipe"])
    print(f"max|grad| at W_opt {np.abs(g_opt).max():.3e}, at W_recipe {np.abs(g_rec).max():.3e}")
    assert np.abs(g_opt).max() <= np.abs(g_rec).max()
    assert f_opt == pytest.approx(float(gold["F_opt"]), abs=1e-9) and f_rec == pytest.approx(float(gold["F_recipe"]), abs=1e-9)
    assert f_opt <= f_rec


def test_restatement_gradient_is_the_derivative(gold, objective):
    rng = np.random.default_rng(3)
    wb = rng.normal(0, 0.3, gold["W_opt"].shape)
    d = rng.normal(0, 1, wb.shape)
    _, g = objective(wb)
    h = 1e-6
    num = (objective(wb + h * d)[0] - objective(wb - h * d)[0]) / (2 * h)
    assert num == pytest.approx(float((g * d).sum()), rel=1e-6)


def test_lbfgs_float64_reaches_the_recipe(gold, objective):
    from dynamicgraphrepresentationlearning_amd import lbfgs
    wb, f, it = lbfgs(lambda w: objective(w.numpy()), gold["W_opt"].shape)
    print(f"lbfgs float64: {it} iterations, F {f:.9f}; F_recipe {float(gold['F_recipe']):.9f}, F_opt {float(gold['F_opt']):.9f}")
    assert f == pytest.approx(float(objective(wb.numpy())[0]), abs=0)
    assert f <= float(gold["F_recipe"])
    assert f >= float(gold["F_opt"]) - 1e-9
