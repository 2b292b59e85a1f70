"""The shortest K-runs of the F(4x4) kernel's rotated K loop (csrc/conv_wino4.h: khead / ktail / run), bit for bit against the C oracle.

The loop over the K-blocks of one kind is rotated by chunk 0: chunk 0 of K-block kb + 1 is issued at the end of the body of kb, also across the boundary between two
runs (full source -> unpooled source -> full source) and in front of the last K-block of all.  What can go wrong there shows at the smallest runs the operator rule
admits, so: a roll-out of 3 steps, batch 3, at 64 x 32 with channels [3, 16, 8] -- layer 1 is a fused Winograd ConvLSTM over E_1 (8 K-blocks), the unpooled R_2
(2 K-blocks: a run whose steady-state loop does not execute once) and h_1 (4 K-blocks) -- and the same with channels [3, 16, 24] (6 unpooled K-blocks).  oracle.wino_form
takes layer 1 of both shapes as a fused Winograd ConvLSTM (checked here on the CPU, before any launch); layer 2 (8 / 24 channels) stays direct.
Settings, each in a fresh child process because the switches are read once per process: the default (a launch this small runs on half blocks), EIGEN_W4_PARTS=1 (the
walk forced), and, so that the full-block wide and tall kernels certainly run these shapes, EIGEN_W4_HALF=0 and EIGEN_W4_TALL=1."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, B, STEPS = 64, 32, 3, 3
SHAPES = [[3, 16, 8], [3, 16, 24]]

_SCRIPT = r"""
import sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
import oracle
from evolutionary_illusion_generator_amd import weights
from evolutionary_illusion_generator_amd.engine import Engine
w, h, B, T = %(w)d, %(h)d, %(B)d, %(T)d
ok = True
for ch in %(shapes)r:
    rng = np.random.default_rng(23)
    img = rng.integers(0, 256, (B, ch[0], h, w), dtype=np.uint8)
    wts = weights.synthetic_prednet_weights(ch, w, h, seed=7)
    e = Engine(w, h, ch, B, n_repeat=T - 1, n_ext=1)
    e.set_weights(wts)
    fr = torch.zeros((B, T, ch[0], h, w), dtype=torch.uint8, device="cuda")
    e.conv_profile(True)
    e.prednet_rollout(torch.from_numpy(img).cuda(), B, T, 0, fr)
    torch.cuda.synchronize()
    got = fr.cpu().numpy()
    took = sorted({(r["epi"], r["layer"]) for r in e.conv_profile(False) if r["wino"] and r["launches"]})
    ref, _ = oracle.PredNetC(wts, ch, w, h, order="canonical").rollout(img, n_repeat=T - 1, n_ext=1)
    same = np.array_equal(got, ref)
    print("KRUN", ch, "bit-exact" if same else "MISMATCH %%d bytes" %% int((got != ref).sum()), "| Winograd operators:", took)
    ok = ok and same and ("lstm", 1) in took
    e.close()
print("KRUN_OK" if ok else "KRUN_FAIL")
"""

_SETTINGS = {"default": {}, "parts=1": {"EIGEN_W4_PARTS": "1"}, "half=0": {"EIGEN_W4_HALF": "0"}, "tall=1": {"EIGEN_W4_TALL": "1"}}


def test_oracle_takes_layer_1_as_a_fused_winograd_convlstm(oracle_lib):
    for ch in SHAPES:
        assert oracle_lib.wino_form(oracle_lib.WINO_AUTO, 0, 1, ch, W, H) == (True, True), ch


@pytest.mark.parametrize("setting", sorted(_SETTINGS))
def test_short_k_runs_frames_bit_exact(cuda, oracle_lib, setting):
    for ch in SHAPES:
        assert oracle_lib.wino_form(oracle_lib.WINO_AUTO, 0, 1, ch, W, H) == (True, True), ch
    env = dict(os.environ)
    for k in ("EIGEN_WINOGRAD", "EIGEN_WINO_FUSEUP", "EIGEN_W4_PARTS", "EIGEN_W4_TALL", "EIGEN_W4_HALF", "EIGEN_W4_PACK"):
        env.pop(k, None)
    env.update(_SETTINGS[setting])
    r = subprocess.run([sys.executable, "-c", _SCRIPT % {"root": ROOT, "w": W, "h": H, "B": B, "T": STEPS, "shapes": SHAPES}], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    print(r.stdout[-2000:])
    assert "KRUN_OK" in r.stdout, r.stdout[-2000:]
