"""CPU: the host side of the error-unit objective (Lotter's L_0 / L_all) -- train.combine_terms against
hand-computed values and the Python-side argument checks.  Its entry points and kernel instantiations are checked with all the
others in tests/test_train_host.py."""
import numpy as np
import pytest


def test_combine_terms_against_hand_computed_values():
    from evolutionary_illusion_generator_amd.train import combine_terms
    table = np.array([[0.5, 2.0, 8.0], [0.25, 4.0, 16.0], [1.0, 1.0, 1.0]])
    # L_0 is the default: the mean of column 0
    assert combine_terms(table) == (0.5 + 0.25 + 1.0) / 3
    assert combine_terms(table, [1.0, 0.0, 0.0]) == combine_terms(table)
    # L_all-like weights (binary fractions: every product and sum below is exact)
    lam = [1.0, 0.5, 0.25]
    rows = [0.5 + 1.0 + 2.0, 0.25 + 2.0 + 4.0, 1.0 + 0.5 + 0.25]
    assert combine_terms(table, lam) == sum(rows) / 3
    # step weights, zeros among them: a zero-weight step counts neither above nor below the line
    assert combine_terms(table, lam, [0.0, 2.0, 0.5]) == (2.0 * rows[1] + 0.5 * rows[2]) / 2.5
    assert combine_terms(table, None, [0.0, 0.0, 4.0]) == 1.0
    assert combine_terms(table, [0.0, 0.0, 2.0], [1.0, 1.0, 0.0]) == (16.0 + 32.0) / 2
    # one layer, and no term at all (a one-frame call)
    assert combine_terms(np.array([[0.125], [0.375]])) == 0.25
    assert combine_terms(np.zeros((0, 3))) == 0.0
    # a non-binary case, in the stated order: (step, layer), then one division
    t2 = np.array([[0.1, 0.7], [0.3, 0.9]])
    want = (0.2 * (1.0 * 0.1 + 0.1 * 0.7) + 0.6 * (1.0 * 0.3 + 0.1 * 0.9)) / (0.2 + 0.6)
    assert combine_terms(t2, [1.0, 0.1], [0.2, 0.6]) == want
    assert isinstance(combine_terms(t2), float)


def test_combine_terms_rejects_what_the_library_rejects():
    from evolutionary_illusion_generator_amd.train import combine_terms
    table = np.ones((3, 2))
    for lam in ([1.0], [1.0, 0.1, 0.1], [0.0, 0.0], [1.0, -0.1], [1.0, float("nan")], [float("inf"), 1.0]):
        with pytest.raises(ValueError):
            combine_terms(table, lam)
    for w in ([1.0, 1.0], [0.0, 0.0, 0.0], [1.0, -1.0, 1.0], [1.0, float("nan"), 1.0]):
        with pytest.raises(ValueError):
            combine_terms(table, None, w)
    with pytest.raises(ValueError):
        combine_terms(np.ones(3))


def test_layer_weights_of_the_wrong_length_are_a_value_error():
    """The length is checked in Python, ahead of any device work (tests/test_gpu_train_obj.py checks it through the trainer)."""
    import inspect
    from evolutionary_illusion_generator_amd import train
    assert train.check_layer_weights(None, 3) is None
    lam = train.check_layer_weights([1, 0.1, 0.1], 3)
    assert lam.dtype == np.float64 and lam.flags["C_CONTIGUOUS"] and lam.tolist() == [1.0, 0.1, 0.1]
    for bad in ([1.0, 0.1], [1.0, 0.1, 0.1, 0.1], [[1.0, 0.1, 0.1]], 1.0):
        with pytest.raises(ValueError):
            train.check_layer_weights(bad, 3)
    fb = inspect.signature(train.PredNetTrainer.forward_backward).parameters
    assert fb["objective"].default == "mse" and fb["layer_weights"].default is None and fb["layer_errors"].default is False
    st = inspect.signature(train.PredNetTrainer.step).parameters
    assert st["objective"].default == "mse" and st["layer_weights"].default is None
    assert inspect.signature(train.PredNetTrainer.evaluate).parameters["layer_errors"].default is False
    # nothing about the objective is trainer state: the hyper-parameter set is what it was
    assert train.HYPER == ("alpha", "beta1", "beta2", "eps")
