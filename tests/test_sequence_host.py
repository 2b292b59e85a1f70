"""Host-side pieces of the frame-sequence API (no GPU): shape validation and the buffer-size rule of Engine.prednet_sequence."""
import numpy as np
import pytest

from evolutionary_illusion_generator_amd import fitness
from evolutionary_illusion_generator_amd.engine import EXPORTS, Engine


def test_sequence_frames_shape_is_checked():
    fitness._check_sequence_frames(np.zeros((2, 3, 1, 8, 16), np.uint8), [1, 4], 16, 8)
    for bad in [(2, 3, 1, 16, 8), (2, 0, 1, 8, 16), (3, 1, 8, 16), (2, 3, 3, 8, 16)]:
        with pytest.raises(ValueError):
            fitness._check_sequence_frames(np.zeros(bad, np.uint8), [1, 4], 16, 8)


def test_buffer_bytes_sees_the_storage_behind_a_view():
    import torch
    a = np.zeros((2, 5, 3), np.uint8)
    assert Engine._buffer_bytes(a) == 30
    assert Engine._buffer_bytes(a[:, :2]) is None          # not contiguous: left to the caller
    t = torch.zeros((2, 5, 3), dtype=torch.uint8)
    assert Engine._buffer_bytes(t) == 30
    assert Engine._buffer_bytes(t[:, 2:]) == 30 - 6          # a strided view reaches the rest of its storage
    assert Engine._buffer_bytes(torch.zeros(4, dtype=torch.float32)) == 16
    assert Engine._buffer_bytes(12345) is None


def test_sequence_entry_point_is_bound():
    assert "eigen_prednet_sequence" in EXPORTS


def test_sequence_flow_of_single_frames_is_empty():
    assert fitness.sequence_flow(np.zeros((3, 1, 1, 8, 8), np.uint8)) == [[], [], []]
