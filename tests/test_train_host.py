"""CPU: the training layer's host side -- the chainer npz round trip, the whole eigen_trainer_* C ABI surface,
and the register metadata of the training kernels (no scratch, no VGPR spills), read from the built library as
tests/test_isa_stats.py does (list and check: tests/train_support.py).  tests/test_train_ext_host.py holds the kernels of self-fed steps
and the per-step reductions beside the checkpoint layout; tests/test_train_obj_host.py holds the objective's host side."""
import os
import re

import numpy as np
import pytest

from tests.train_support import GRADIENT_KERNELS, check_no_scratch_and_no_spills

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAINER_API = ["eigen_trainer_create", "eigen_trainer_destroy", "eigen_trainer_set_weights", "eigen_trainer_get_weights",
               "eigen_trainer_loss_grad", "eigen_trainer_get_grads", "eigen_trainer_adam", "eigen_trainer_tape_bytes",
               "eigen_trainer_loss_grad_ext", "eigen_trainer_evaluate", "eigen_trainer_get_state", "eigen_trainer_set_state",
               "eigen_trainer_loss_grad_obj", "eigen_trainer_evaluate_err"]


def test_chainer_npz_round_trip_is_exact(tmp_path):
    from evolutionary_illusion_generator_amd import weights
    ch, w, h = [3, 4, 6], 16, 12
    wt = weights.synthetic_prednet_weights(ch, w, h, seed=3)
    path = str(tmp_path / "model.npz")
    weights.save_chainer_npz(wt, path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted("predictor/" + k for k in wt)
    back = weights.load_chainer_npz(path, ch, w, h)
    assert sorted(back) == sorted(wt)
    for k in wt:
        assert back[k].dtype == np.float32 and back[k].shape == wt[k].shape
        assert np.array_equal(back[k], wt[k]), k


def test_trainer_entry_points_are_declared_exported_and_listed():
    import __graft_entry__ as ge
    from evolutionary_illusion_generator_amd import engine
    assert "prednet_train.hip" in ge.HIP_UNITS and "flow_stage.hip" in ge.HIP_UNITS
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    declared = set(re.findall(r"\b(eigen_[a-z_0-9]+)\s*\(", header))
    assert "#define EIGEN_ABI_VERSION 4" in header
    assert re.search(r"EIGEN_OBJ_MSE\s*=\s*0\b", header) and re.search(r"EIGEN_OBJ_ERROR\s*=\s*1\b", header)
    for name in TRAINER_API:
        assert name in declared, name
        assert name in engine.EXPORTS, name
    if os.path.exists(engine.LIB_PATH):
        lib = engine.load_library()
        assert lib.eigen_abi_version() == 4
        for name in TRAINER_API:
            assert hasattr(lib, name), name


@pytest.mark.parametrize("kernel", GRADIENT_KERNELS)
def test_training_kernels_have_no_scratch_and_no_spills(kernel):
    check_no_scratch_and_no_spills(kernel)
