"""CPU: the training layer's host side -- chainer npz round trip, the eigen_trainer_* C ABI surface, and the register metadata of
every training kernel (no scratch, no VGPR spills), read from the built library as tests/test_isa_stats.py does."""
import os
import re

import numpy as np
import pytest

from tests import test_isa_stats as isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAINER_API = ["eigen_trainer_create", "eigen_trainer_destroy", "eigen_trainer_set_weights", "eigen_trainer_get_weights",
               "eigen_trainer_loss_grad", "eigen_trainer_get_grads", "eigen_trainer_adam", "eigen_trainer_tape_bytes"]
# every __global__ of csrc/train_kernels.h (the templates in each instantiation prednet_train.hip launches)
TRAIN_KERNELS = ["tconv3x3_kernel", "twgrad_kernel", "tsum_slabs_kernel", "tbias_grad_kernel", "terr_fwd_kernel", "terr_bwd_kernel",
                 "tlstm_fwd_kernel", "tlstm_bwd_kernel", "tpeep_grad_kernel", "tpact_fwd_kernel", "tpact_bwd_kernel",
                 "tloss_partial_kernel", "tloss_final_kernel", "tadam_kernel"]


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
    assert "prednet_train.hip" in ge.HIP_UNITS
    header = open(os.path.join(ROOT, "include", "eigen_engine.h")).read()
    declared = set(re.findall(r"\b(eigen_[a-z_0-9]+)\s*\(", header))
    assert "#define EIGEN_ABI_VERSION 4" in header
    for name in TRAINER_API:
        assert name in declared, name
        assert name in engine.EXPORTS, name
    if os.path.exists(engine.LIB_PATH):
        lib = engine.load_library()
        for name in TRAINER_API:
            assert hasattr(lib, name), name


@pytest.fixture(scope="module")
def stats():
    if not os.path.exists(isa.LIB):
        pytest.skip("libeigen_hip.so not built")
    if not os.path.exists(isa.READELF):
        pytest.skip("llvm-readelf not found")
    return isa._kernel_stats()


@pytest.mark.parametrize("kernel", TRAIN_KERNELS)
def test_training_kernels_have_no_scratch_and_no_spills(stats, kernel):
    names = [n for n in stats if re.match(r"_ZN4eigt\d+%s" % kernel, n)]
    assert names, "%s not in the library" % kernel
    for n in names:
        for s in stats[n]:
            assert s["private_segment_fixed_size"] == 0, (n, s)
            assert s["vgpr_spill_count"] == 0, (n, s)
            assert s["sgpr_spill_count"] == 0, (n, s)
