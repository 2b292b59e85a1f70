"""CPU, reference only: the gradient comparisons of tests/test_gpu_train*.py and tests/test_gpu_frame_grad.py compare something.
Every case of the one list they parametrize over (tests/train_support.py ALL_CASES) has live reference gradients or is declared
dead; the wide shapes reach every tile configuration the table TILE_PROPERTIES names, by a Python restatement of the selection
arithmetic of conv() and wgrad(); and the gradient rule `_check_grads` rejects the errors it is there to catch."""
import os
import re

import numpy as np
import pytest
import torch

from tests import train_support as ts
from tests.frame_grad_support import check_frame_grads, run_frames, target_path, zero_steps
from tests.train_support import (ALL_CASES, ALL_GRAD_CASES, TILE_PROPERTIES, WIDE_CALLS, WIDE_SHAPES, SHAPES, _check_grads, case_frames, case_id,
                                 case_reference, cases, is_all_zero, is_clamped, is_dead, launches)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _saturated(pred):
    """the share of P0, over every step, that sits at the clamp"""
    return float(((pred <= 0) | (pred >= 1)).mean())


def test_the_list_holds_every_kind_of_case_at_every_shape():
    assert len(set(ALL_CASES)) == len(ALL_CASES) and len(set(map(case_id, ALL_CASES))) == len(ALL_CASES)
    for group in ("teacher_forced", "self_fed", "error_objective", "frames"):
        for w, h, ch in SHAPES:
            assert [c for c in cases(group, wide=False) if (c.w, c.h, list(c.ch)) == (w, h, ch)], (group, w, h, ch)
        for w, h, ch, B in WIDE_SHAPES:
            here = [c for c in cases(group, wide=True) if (c.w, c.h, list(c.ch), c.B) == (w, h, ch, B)]
            assert sorted((c.T,) + c.room for c in here) == sorted(WIDE_CALLS), (group, w, h, ch)
    # the dead cases are the random set at the two gray shapes, and nothing at a wide shape
    assert {(c.w, c.h) for c in ALL_CASES if is_dead(c)} == {(12, 8), (24, 16)}
    assert all(c.wset == "random" for c in ALL_CASES if is_dead(c))


@pytest.mark.parametrize("c", ALL_GRAD_CASES, ids=case_id)
def test_every_weight_gradient_case_is_live_or_declared_all_zero(c):
    r = case_reference(c)
    G = np.sqrt(sum(float((g ** 2).sum()) for g in r.grads.values()))
    if is_all_zero(c):
        assert _saturated(r.pred) == 1.0
        assert G == 0.0 and all(not g.any() for g in r.grads.values())
        return
    assert not is_dead(c)      # no weight-gradient case runs the dead weights under an objective that reaches past the clamp
    assert G > 0
    dead = [k for k, g in r.grads.items() if not g.any()]
    assert not dead, ("the reference gradient of these tensors is zero: the case compares nothing there", dead)
    assert 0.5 < _saturated(r.pred) < 0.75 if is_clamped(c) else _saturated(r.pred) <= 0.5, _saturated(r.pred)


@pytest.mark.parametrize("c", cases("frames"), ids=case_id)
def test_every_frame_gradient_case_is_live_or_declared_dead(c):
    """What tests/test_gpu_frame_grad.py compares is the frame gradient: every step outside `zero_steps` has a non-zero reference,
    and outside the dead cases the input path (the gradient less its analytic target path) is there."""
    r = case_reference(c, run=run_frames)
    g = r.frame_grad
    assert np.linalg.norm(g.ravel()) > 0
    zero = zero_steps(c.T, c.n_fed, c.sw, dead=is_all_zero(c))
    for t in range(c.T):
        assert bool(g[:, t].any()) == (t not in zero), (t, zero)
    inp = g - target_path(case_frames(c), r.pred, c.objective, c.sw, c.lam)
    fed = c.T if c.n_fed is None else c.n_fed
    if is_dead(c):
        assert _saturated(r.pred) == 1.0
        if c.objective == "mse":
            assert np.abs(inp).max() <= 1e-12 * np.abs(g).max()
    else:
        assert 0.5 < _saturated(r.pred) < 0.75 if is_clamped(c) else _saturated(r.pred) <= 0.5, _saturated(r.pred)
        assert np.abs(inp[:, :fed]).max() > 1e-6 * np.abs(g).max()


# ---- the tiles
def test_the_restated_selection_reads_the_constants_of_the_source():
    src = open(os.path.join(ROOT, "evolutionary_illusion_generator_amd", "csrc", "prednet_train.hip")).read()
    const = lambda name: re.search(r"constexpr\s+(?:long long|int)\s+%s\s*=\s*([^;]+);" % name, src).group(1).strip()
    assert const("WGRAD_WAVES") == str(ts.WGRAD_WAVES) and const("BIAS_SLICES") == str(ts.BIAS_SLICES)
    assert const("SLAB_FLOATS") == "16ll << 20" and ts.SLAB_FLOATS == 16 << 20
    # the thresholds of conv() and of wgrad(), and wgrad's split arithmetic, as the restatement has them
    assert "if (cout <= 16) launch_conv_mt<1>(a, st);" in src and "else if (cout <= 32) launch_conv_mt<2>(a, st);" in src
    assert "const int MT = cout <= 16 ? 1 : cout <= 32 ? 2 : 4;" in src
    for line in ("long long ns = WGRAD_WAVES / (long long)(gx * gy);", "ns = std::min<long long>(ns, t->slab_floats / (cout * K));",
                 "ns = std::min<long long>(ns, (P + 255) / 256);", "chunk = (chunk + 3) & ~3ll;", "ns = (P + chunk - 1) / chunk;"):
        assert line in src, line


def test_the_restated_selection_on_known_launches():
    # 48 x 32 colour, channels (3, 48, 96, 192), B = 4, T = 8: the real channel counts
    q = {(x["kind"], x["name"]): x for x in launches(48, 32, [3, 48, 96, 192], 4, 8)}
    f = q["forward", "ConvLSTM1/x0+h"]
    assert (f["MT"], f["gx"], f["gy"]) == (4, 4 * 16 * 24 // 64, 3)
    g = q["wgrad", "ConvLSTM3/h"]               # cout 768, K 1728, P = 32 * 4 * 6 = 768
    assert (g["MT"], g["gx"], g["gy"], g["nsplit"], g["chunk"], g["last"]) == (4, 27, 12, 3, 256, 256)
    g = q["wgrad", "ConvP0"]                    # cout 3, K 27, P = 32 * 1536: nsplit capped by the pixel count
    assert (g["MT"], g["gx"], g["gy"], g["nsplit"], g["chunk"]) == (1, 1, 1, 192, 256)


def test_the_wide_shapes_reach_every_tile_property():
    qs = [q for w, h, ch, B in WIDE_SHAPES for T, db, dT in WIDE_CALLS for q in launches(w, h, ch, B, T, (db, dT))]
    for name, hit in TILE_PROPERTIES:
        assert any(hit(q) for q in qs), "no launch of WIDE_SHAPES x WIDE_CALLS reaches: " + name
    # and SHAPES alone reach none of the MT = 4 rows: the wide shapes are what brings them in
    small = [q for w, h, ch in SHAPES for q in launches(w, h, ch, 2, 5)]
    assert all(q["MT"] < 4 and q["gy"] == 1 and q["P"] % 4 == 0 for q in small)


# ---- the rule
# the synthetic set: ten of its tensors lie below 1e-6 of G at this shape
WIDE_CASE = next(c for c in cases("teacher_forced", wide=True) if list(c.ch) == [3, 12, 20] and c.wset == "synthetic")


def _old_rule(got, ref):
    """the rule this one replaced: err_k <= 1e-3 |r_k| + 1e-6 G"""
    G = np.sqrt(sum(float((r ** 2).sum()) for r in ref.values()))
    return all(np.linalg.norm((got[k] - r).ravel()) <= 1e-3 * np.linalg.norm(r.ravel()) + 1e-6 * G for k, r in ref.items())


def _rejects(got, ref):
    try:
        _check_grads(got, ref)
    except AssertionError as e:
        return str(e)
    return None


def test_the_rule_rejects_what_it_is_there_to_catch():
    """Reference gradients of one wide case, perturbed four ways; the rule must reject each.  The tensor is ConvLSTM2/x_c0/W,
    [20, 40, 3, 3], the upper-layer conv gradient of the LARGEST norm here (3.7e-4 of G).  The rule this one replaced
    (1e-3 |r_k| + 1e-6 G) accepted (a), one element off by 1 % of the tensor's maximum; (c), a tensor below 1e-6 G returned all
    zero (ten tensors of this case); and, on this tensor, (d), a scale of 1.002, since 0.002 |r_k| < 1e-6 G; it rejected (b) here,
    and accepted (b) too on the gate weights below 1e-6 G (ConvLSTM2/h_i/W, 3.2e-8 of G).  Asserted below, so the record stays true."""
    ref = case_reference(WIDE_CASE).grads
    G = np.sqrt(sum(float((r ** 2).sum()) for r in ref.values()))
    assert _rejects(ref, ref) is None
    copy = lambda: {k: v.copy() for k, v in ref.items()}
    k = "ConvLSTM2/x_c0/W"
    assert ref[k].shape == (20, 40, 3, 3)
    # (a) one element off by 1 % of the tensor's maximum
    got = copy()
    got[k][7, 5, 1, 2] += 0.01 * np.abs(ref[k]).max()
    msg = _rejects(got, ref)
    assert msg and "%s[7, 5, 1, 2]" % k in msg, msg           # the report names the element
    assert _old_rule(got, ref)
    # (b) one 16-channel output block of a conv weight gradient zeroed
    for name, old_accepted in ((k, False), ("ConvLSTM2/h_i/W", True)):
        got = copy()
        got[name][:16] = 0
        assert _rejects(got, ref), name
        assert _old_rule(got, ref) == old_accepted, name
    # (c) a tensor with |r_k| < 1e-6 G zeroed entirely
    small = [n for n, r in ref.items() if 0 < np.linalg.norm(r.ravel()) < 1e-6 * G]
    assert len(small) == 10, small
    for n in small:
        got = copy()
        got[n][...] = 0
        assert _rejects(got, ref), n
        assert _old_rule(got, ref), n
    # (d) a tensor scaled by 1.002
    got = copy()
    got[k] = got[k] * 1.002
    assert _rejects(got, ref)
    assert _old_rule(got, ref)
    got = copy()
    got["ConvP0/W"] = got["ConvP0/W"] * 1.002                   # a tensor of large norm: both rules reject
    assert _rejects(got, ref) and not _old_rule(got, ref)
    # an undeclared zero reference compares nothing and fails; a declared one holds got to zero
    zeros = {n: np.zeros_like(v) for n, v in ref.items()}
    assert _rejects(zeros, zeros) and _check_grads(zeros, zeros, zero_allowed=True) == (0.0, 0.0)
    got = copy()
    for n in got:
        got[n][...] = 0
    got[k][0, 0, 0, 0] = 1e-30
    with pytest.raises(AssertionError):
        _check_grads(got, zeros, zero_allowed=True)


# one case of every group at every wide shape and at the colour shape: a sample of the measurement behind ELEMENT_BOUND
F32_SAMPLE = [c for c in ALL_GRAD_CASES if c in cases(c.group, wide=True) or ((c.w, c.h) == (16, 12) and c.wset == "live" and c.sw is None)]


def float32_deviation(c):
    """{tensor or step: (norm deviation / own norm, element-wise deviation / largest element, own norm / G)} of the float32 run of
    the reference against its float64 run, both fed the bytes of the float32 run's predictions: the measurement behind ELEMENT_BOUND.
    `python -m tests.test_train_cases_host` prints its worst over ALL_CASES (a minute on a CPU)."""
    run = run_frames if c.group == "frames" else None
    g32 = case_reference(c, dtype=torch.float32, run=run)
    r = case_reference(c, pred=g32.pred.astype(np.float32) if c.requant else None, run=run)
    if c.group == "frames":
        parts = {"t=%d" % t: (g32.frame_grad[:, t], r.frame_grad[:, t]) for t in range(c.T)}
        parts["tied"] = (g32.frame_grad.sum(1), r.frame_grad.sum(1))
    else:
        parts = {k: (g32.grads[k], r.grads[k]) for k in r.grads}
    G = np.sqrt(sum(float((b ** 2).sum()) for _, b in parts.values()))
    out = {}
    for k, (a, b) in parts.items():
        if b.any():
            out[k] = (np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()), np.abs(a - b).max() / np.abs(b).max(), np.linalg.norm(b.ravel()) / G)
        else:
            assert not a.any(), (case_id(c), k)
    return g32, r, out


@pytest.mark.parametrize("c", F32_SAMPLE, ids=case_id)
def test_the_float32_restatement_passes_the_rule(c):
    """The reference itself in float32 (no code of the trainer) against its float64 run: it passes the rule, by two orders in norm,
    and element-wise stays under the tenth of the bound that the bound was set from."""
    g32, r, dev = float32_deviation(c)
    norm, elem = _check_grads(g32.grads, r.grads, what=case_id(c))
    print("%s: float32 restatement at %.4f of the norm bound, %.4f of the element-wise bound" % (case_id(c), norm, elem))
    assert max(d[1] for d in dev.values()) <= ts.ELEMENT_BOUND / 10


def test_the_frame_rule_rejects_a_dead_step_and_a_local_error():
    c = next(x for x in cases("frames", wide=True) if list(x.ch) == [3, 12, 20] and x.objective == "mse")
    g = case_reference(c, run=run_frames).frame_grad
    assert check_frame_grads(g, g) == 0.0
    bad = g.copy()
    bad[1, 2, 0, 3, 4] += 0.01 * np.abs(g[:, 2]).max()
    with pytest.raises(AssertionError, match=r"t=2\[1, 0, 3, 4\]"):
        check_frame_grads(bad, g)
    bad = g.copy()
    bad[:, 0] = 0
    with pytest.raises(AssertionError):
        check_frame_grads(bad, g)
    with pytest.raises(AssertionError, match="not declared"):
        check_frame_grads(bad, bad)                      # a zero reference step outside `zero`
    check_frame_grads(bad, bad, zero={0})


if __name__ == "__main__":
    worst = {"norm": (0.0, None), "element": (0.0, None)}
    for case in ALL_CASES:
        for name, (dn, de, share) in float32_deviation(case)[2].items():
            for key, d in (("norm", dn), ("element", de)):
                if d > worst[key][0]:
                    worst[key] = (d, "%s %s (%.1e of G)" % (case_id(case), name, share))
                    print("%s: %.3e %s" % (key, d, worst[key][1]))
    print("%d cases; worst deviation in norm %.3e, element-wise %.3e; ELEMENT_BOUND = %.1e" % (len(ALL_CASES), worst["norm"][0], worst["element"][0], ts.ELEMENT_BOUND))
