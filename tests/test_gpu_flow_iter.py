"""The flow objective through the pyramidal, iterated solve on the GPU (eigen_trainer_flow_term_iter, eigen_trainer_loss_grad_flow_iter,
``FlowObjective.solved``; DESIGN.md section 13, "The iterated solve's gradient").  The field is compared bit for bit with the numpy
restatement of tests/dense_pyr_support.py and with the dense fitness's own field; the seed and the reference gradient, float32 out of
float64 arithmetic, are compared tensor by tensor with the float64 autograd statement of tests/flow_iter_support.py under
max |got - ref| <= 2^-23 max |ref|; tests/test_flow_iter_host.py keeps that statement's own reordering under 2^-30."""
import functools
import hashlib

import numpy as np
import pytest

from evolutionary_illusion_generator_amd import train
from evolutionary_illusion_generator_amd.train import CornerMembers, FlowObjective, PredictionFlow, PredNetTrainer
from tests import dense_pyr_support as dp
from tests import flow_iter_support as fi
from tests import flow_pair_support as ps
from tests.frame_grad_support import check_frame_grads
from tests.train_support import _check_grads, _grads_differ

pytestmark = pytest.mark.gpu

SCALE = 0.75
WORST = {"stage": 0.0}


def _trainer(name, batch=None):
    """a trainer for the stage alone on a case's image: two layers where the image halves, one where it is odd"""
    _, w, h, C, _, _, _, seeds, _ = fi.stage_case(name)
    ch = [C, 4] if w % 2 == 0 and h % 2 == 0 else [C]
    return PredNetTrainer("synthetic", ch, w, h, batch or len(seeds), 2)


@functools.lru_cache(maxsize=None)
def _field(name):
    _, _, _, _, levels, iters, r, _, _ = fi.stage_case(name)
    img0, img1 = fi.stage_images(name)
    return dp.dense_pyr_ref(img0, img1, r, fi.EPS, levels, iters)


def _check_tensor(got, ref64, what):
    err, bound = fi.within(got, ref64)
    assert bound > 0, what
    WORST["stage"] = max(WORST["stage"], err / bound)
    print("%s: max |got - ref| %.3e, bound %.3e (ratio %.3f, worst so far %.3f)" % (what, err, bound, err / bound, WORST["stage"]))
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("mode", fi.MODES)
@pytest.mark.parametrize("name", fi.STAGE_NAMES)
def test_the_stage_alone_meets_the_autograd_statement(cuda, name, mode):
    """`flow_term` (byte reference) and `flow_term_pair` (the same bytes as floats) with reference_grad=True under a real solve: the field
    is `dense_pyr_ref`'s bit for bit, the value is within 1e-10, the seed and the reference gradient are within 2^-23 of their tensor's
    maximum of float64 autograd; both entries and a second run return the same bytes."""
    _, w, h, C, levels, iters, r, _, _ = fi.stage_case(name)
    img0, img1 = fi.stage_images(name)
    pred, prev = fi.as_floats(img1), fi.as_floats(img0)
    ref = fi.stage_reference(name)[mode]
    flow = fi.make_objective(mode, w, h, r, levels, iters)
    with _trainer(name) as tr:
        assert tr.debug_flow_iter() == 0
        a = tr.flow_term(pred, img0, flow, scale=SCALE, reference_grad=True)
        held = tr.debug_flow_iter()
        b = tr.flow_term_pair(pred, prev, flow, scale=SCALE, reference_grad=True)
        again = tr.flow_term(pred, img0, flow, scale=SCALE, reference_grad=True)
        assert held > 0 and tr.debug_flow_iter() == held
    for x, y, z in zip(a[1:], b[1:], again[1:]):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert a[0] == b[0] == again[0]
    value, u, seed, rg = a
    assert np.array_equal(u, _field(name)), np.abs(u - _field(name)).max()
    assert abs(value - ref.value) <= 1e-10 * max(1.0, abs(ref.value)), (value, ref.value)
    assert seed.dtype == np.float32 and rg.dtype == np.float32 and np.abs(rg).max() > 0
    _check_tensor(seed, SCALE * ref.seed64, "%s %s seed" % (name, mode))
    _check_tensor(rg, SCALE * ref.ref64, "%s %s reference gradient" % (name, mode))


def test_the_field_is_the_dense_fitness_field_on_the_same_bytes(cuda):
    """48 x 32, 2 levels x 3 iterations: the trainer stage's u on (float)byte / 255.0f is `Engine.dense_score`'s d_flow bit for bit"""
    import torch
    from evolutionary_illusion_generator_amd.engine import Engine
    name = "48x32"
    _, w, h, C, levels, iters, r, _, _ = fi.stage_case(name)
    img0, img1 = fi.stage_images(name)
    dense = dp.dense_for(1, r, 8.0, levels, iters)
    B, per = len(img0), C * h * w
    eng = Engine(w, h, [C, 4], B)
    try:
        _, _, d_flow = eng.dense_score(torch.from_numpy(img0).to(cuda), per, torch.from_numpy(img1).to(cuda), per, B, dense, stats=True, flow=True)
    finally:
        eng.close()
    with _trainer(name) as tr:
        u = tr.flow_term(fi.as_floats(img1), img0, fi.make_objective("circles", w, h, r, levels, iters))[1]
    assert np.array_equal(u, np.asarray(d_flow).reshape(u.shape))


@pytest.mark.parametrize("mode", ["energy", "circles"])
def test_a_slice_of_the_batch_equals_the_batch(cuda, mode):
    """48 x 32, a batch of 3 whose third sample moves by 5.5 pixels: the slices [0, 2) and [2, 3) return the bytes of the batch's field and
    (under the energy mode, whose kappa a slice's scale can restate exactly) of its seed and reference gradient"""
    name = "48x32"
    _, w, h, C, levels, iters, r, _, _ = fi.stage_case(name)
    img0, img1 = fi.stage_images(name)
    pred = fi.as_floats(img1)
    flow = fi.make_objective(mode, w, h, r, levels, iters)
    with _trainer(name) as tr:
        whole = tr.flow_term(pred, img0, flow, scale=3.0, reference_grad=True)
        parts = [tr.flow_term(pred[s], img0[s], flow, scale=float(s.stop - s.start), reference_grad=True) for s in (slice(0, 2), slice(2, 3))]
    for k in (1, 2, 3):      # kappa = scale / (B N_m) or scale / B: 3 / 3, 2 / 2 and 1 / 1 are the same factor
        assert np.concatenate([p[k] for p in parts]).tobytes() == whole[k].tobytes(), k


def test_a_per_sample_mask_and_corner_members_follow_their_planes(cuda):
    """20 x 15 r 7 under the Circles score: a per-sample [n, H, W] mask returns, sample by sample, the bytes of a batch-of-one call under
    that plane as a shared mask, which meets the autograd statement; `CornerMembers` returns the bytes of the per-sample mask of the
    planes `flow_members` reports."""
    name = "20x15r7"
    _, w, h, C, levels, iters, r, _, _ = fi.stage_case(name)
    img0, img1 = fi.stage_images(name)
    pred = fi.as_floats(img1)
    B = len(img0)
    rng = np.random.default_rng(5)
    masks = (rng.random((B, h, w)) < 0.7).astype(np.uint8)
    members = CornerMembers(max_corners=60, quality_level=0.02, min_distance=2.0, block_size=3)
    with _trainer(name) as tr:
        batch = tr.flow_term(pred, img0, fi.make_objective("circles", w, h, r, levels, iters, mask=masks), scale=float(B), reference_grad=True)
        for b in range(B):
            one = tr.flow_term(pred[b:b + 1], img0[b:b + 1], fi.make_objective("circles", w, h, r, levels, iters, mask=masks[b]), scale=1.0, reference_grad=True)
            for k in (1, 2, 3):
                assert one[k].tobytes() == batch[k][b:b + 1].tobytes(), (b, k)
            ref = fi.stage_grads(pred[b:b + 1], fi.as_floats(img0[b:b + 1]), r, fi.EPS, levels, iters, ("circles",), h, w, mask=masks[b])["circles"]
            _check_tensor(one[2], ref.seed64, "masked sample %d seed" % b)
            _check_tensor(one[3], ref.ref64, "masked sample %d reference gradient" % b)
        planes, counts = tr.flow_members(img0, members)
        assert (planes.reshape(B, -1).sum(1) >= 4).all(), counts
        by_corners = tr.flow_term(pred, img0, fi.make_objective("circles", w, h, r, levels, iters, members=members), scale=SCALE, reference_grad=True)
        by_planes = tr.flow_term(pred, img0, fi.make_objective("circles", w, h, r, levels, iters, mask=planes), scale=SCALE, reference_grad=True)
    assert by_corners[0] == by_planes[0] and all(x.tobytes() == y.tobytes() for x, y in zip(by_corners[1:], by_planes[1:]))
    assert np.abs(by_corners[2]).max() > 0 and np.abs(by_corners[3]).max() > 0


def test_one_level_one_iteration_is_the_namesake_and_allocates_nothing(cuda):
    """16 x 12: an objective `.solved(1, 1)` returns the bytes of the objective without a solve under every mode and leaves the handle
    without an iterated workspace; forced through the new stage and its backward, the same call meets the bound against today's seed and
    reference gradient, and its field is today's bit for bit."""
    name = "16x12"
    _, w, h, C, _, _, r, _, _ = fi.stage_case(name)
    img0, img1 = fi.stage_images(name)
    pred = fi.as_floats(img1)
    with _trainer(name) as tr:
        today = {}
        for mode in fi.MODES:
            direction, score = fi.mode_objects(mode, w, h)
            plain = FlowObjective(r, fi.EPS, direction, score=score)
            assert plain.solve is None
            today[mode] = tr.flow_term(pred, img0, plain, scale=SCALE, reference_grad=True)
            same = tr.flow_term(pred, img0, fi.make_objective(mode, w, h, r, 1, 1), scale=SCALE, reference_grad=True)
            assert today[mode][0] == same[0] and all(x.tobytes() == y.tobytes() for x, y in zip(today[mode][1:], same[1:])), mode
        assert tr.debug_flow_iter() == 0
        tr.debug_flow_iter(True)
        for mode in fi.MODES:
            direction, score = fi.mode_objects(mode, w, h)
            forced = tr.flow_term(pred, img0, FlowObjective(r, fi.EPS, direction, score=score), scale=SCALE, reference_grad=True)
            assert np.array_equal(forced[1], today[mode][1]), mode
            assert abs(forced[0] - today[mode][0]) <= 1e-10 * max(1.0, abs(today[mode][0]))
            # today's float32 tensors are themselves one rounding from their float64 values: both sides round once, 2^-23 of the maximum
            _check_tensor(forced[2], today[mode][2].astype(np.float64), "forced 1 x 1 %s seed" % mode)
            _check_tensor(forced[3], today[mode][3].astype(np.float64), "forced 1 x 1 %s reference gradient" % mode)
        assert tr.debug_flow_iter(False) > 0


def test_refusals_leave_the_handle_training(cuda):
    """a coarsest level below 4 pixels is a ValueError before any call; the library refuses levels and iters outside eigen_dense_solve's
    values in that struct's words, before any allocation; the handle then still runs an iterated and a single-step call"""
    import ctypes
    from evolutionary_illusion_generator_amd.engine import DenseSolveC, _ptr
    name = "16x12"
    _, w, h, C, _, _, r, _, _ = fi.stage_case(name)
    img0, img1 = fi.stage_images(name)
    pred = fi.as_floats(img1)
    with _trainer(name) as tr:
        with pytest.raises(ValueError, match="the coarsest level of a 16 x 12 image is 2 x 2, below 4 pixels"):
            tr.flow_term(pred, img0, FlowObjective(r, fi.EPS).solved(4, 2))
        import torch
        p, x = torch.from_numpy(pred).to(cuda), torch.from_numpy(img0).to(cuda)
        per, n = C * h * w, len(img0)
        cfg = FlowObjective(r, fi.EPS).settings(stage_alone=True)
        for levels, iters, words in ((0, 1, "dense solve levels 0 outside 1 .. 6"), (7, 1, "dense solve levels 7 outside 1 .. 6"),
                                     (1, 0, "dense solve iters 0 outside 1 .. 32"), (1, 33, "dense solve iters 33 outside 1 .. 32"),
                                     (4, 1, "the coarsest level of a 16 x 12 image is 2 x 2, below 4 pixels")):
            solve = DenseSolveC(levels, iters)
            rc = tr.lib.eigen_trainer_flow_term_iter(tr._h, _ptr(p), ctypes.c_int64(per), _ptr(x), None, ctypes.c_int64(per), ctypes.c_int32(n), ctypes.byref(cfg),
                                                     None, None, None, None, ctypes.c_double(1.0), None, None, None, None, ctypes.c_int64(0), None, ctypes.c_int64(0),
                                                     None, None, ctypes.byref(solve))
            assert rc == -1 and words in tr.lib.eigen_last_error().decode(), (levels, iters, tr.lib.eigen_last_error())
        assert tr.debug_flow_iter() == 0
        a = tr.flow_term(pred, img0, FlowObjective(r, fi.EPS).solved(1, 5))
        b = tr.flow_term(pred, img0, FlowObjective(r, fi.EPS))
        assert np.array_equal(a[1], _field(name)) and np.isfinite(b[2]).all()


def _sha(*arrays):
    m = hashlib.sha256()
    for a in arrays:
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()


def test_other_paths_keep_their_bits_around_an_iterated_call(cuda):
    """16 x 12 [3, 4, 6]: an "mse", an "error" and a single-step "flow" training call return the same SHA-256 of loss, gradients and frame
    gradient before and after an iterated call on the same handle, and on a fresh handle"""
    c = ps.PairCase(16, 12, (3, 4, 6), "live", "energy", 7, "drifting")
    frames, wts = ps.pair_case_frames(c), ps.pair_case_weights(c)
    B, T = frames.shape[:2]

    def calls(tr):
        out = []
        for kw in (dict(objective="mse"), dict(objective="error"), dict(objective="flow", flow=PredictionFlow(7, 1e-2))):
            loss, g = tr.forward_backward(frames, frame_grads="frames", **kw)
            grads = tr.grads()
            out.append(_sha(np.float64(loss), g, *[grads[k] for k in sorted(grads)]))
        return out

    with PredNetTrainer(wts, list(c.ch), c.w, c.h, B, T) as tr:
        before = calls(tr)
        loss = tr.forward_backward(frames, objective="flow", flow=PredictionFlow(7, 1e-2).solved(2, 2))
        assert np.isfinite(loss) and tr.debug_flow_iter() > 0
        after = calls(tr)
    with PredNetTrainer(wts, list(c.ch), c.w, c.h, B, T) as tr:
        fresh = calls(tr)
        assert tr.debug_flow_iter() == 0
    assert before == after == fresh


# ---- training calls against the autograd statement (the cases of tests/flow_iter_support.py, which tests/test_flow_iter_host.py keeps under
# the float32 yardstick)
@functools.lru_cache(maxsize=None)
def _train_gpu_and_refs(c):
    from tests.train_support import _fed_from
    frames, wts, call = ps.pair_case_frames(c), fi.train_case_weights(c), ps.pair_case_call(c)
    flow = fi.train_case_flow(c)
    B, T = frames.shape[:2]
    with PredNetTrainer(wts, list(c.ch), c.w, c.h, B, T) as tr:
        loss, pred, per, terms = tr.forward_backward(frames, pred=True, frame_grads="frames", flow_terms=True, objective="flow", flow=flow, **call)
        grads = tr.grads()
        again = tr.forward_backward(frames, frame_grads="frames", objective="flow", flow=flow, **call)
        assert again[0] == loss and again[1].tobytes() == per.tobytes()
    # with requant both sides read the bytes of the GPU's own float32 predictions, as tests/test_gpu_flow_pair.py does
    fed = _fed_from(pred) if call["requant"] else None
    return (loss, pred, per, terms, grads), fi.train_case_reference(c, fed), fi.train_case_reference(c, fed, detach_prev=True), fi.train_case_reference(c, fed, single=True)


@pytest.mark.parametrize("c", fi.TRAIN_CASES, ids=fi.train_case_id)
def test_a_training_call_matches_float64_autograd_through_the_solve(cuda, c):
    """Prediction pairing, 2 levels x 2 iterations: loss and terms within 1e-5 of their un-cancelled scale (the bound of
    tests/test_gpu_flow_pair.py), every weight gradient within `_check_grads`, the per-frame gradient within `check_frame_grads`, both
    unchanged; the reference with every previous prediction detached and the single step's reference are outside `_check_grads`."""
    (loss, pred, per, terms, grads), r, detached, single = _train_gpu_and_refs(c)
    what = ps.pair_case_id(c)
    T = per.shape[1]
    assert np.abs(pred - r.pred).max() <= 1e-5
    assert r.scale > 0 and abs(loss - r.loss) <= 1e-5 * r.scale, (loss, r.loss, r.scale)
    assert (np.abs(terms - r.terms) <= 1e-5 * r.term_scales).all(), (terms, r.terms)
    norm, element = _check_grads(grads, r.grads, what=what)
    n_fed = ps.pair_case_call(c)["n_fed"] or T
    zero = {t for t in range(T) if t >= n_fed or t == T - 1}
    ratio = check_frame_grads(per, r.frame_grad, what, zero=zero)
    assert _grads_differ(detached.grads, grads), "the path through the previous prediction has vanished"
    assert _grads_differ(single.grads, grads), "the gradient is the single step's"
    print("iterated %s: error / bound norm %.4f element %.4f frames %.4f" % (what, norm, element, ratio))


def test_a_moving_frame_reference_reaches_the_frame_gradient(cuda):
    """16 x 12 colour, frame pairing with reference="moving", 2 x 2: the frame gradient holds every term's reference path (within
    `check_frame_grads` of autograd with the frames in the graph) and differs from the constant reference's"""
    from tests import flow_obj_support as fs
    c = ps.PairCase(16, 12, (3, 4, 6), "live", "energy", 3, "drifting")
    frames, wts, call = ps.pair_case_frames(c), ps.pair_case_weights(c), ps.pair_case_call(c)
    B, T = frames.shape[:2]
    with PredNetTrainer(wts, list(c.ch), c.w, c.h, B, T) as tr:
        out = {ref: tr.forward_backward(frames, frame_grads="frames", objective="flow", flow=FlowObjective(c.r, 1e-2, reference=ref).solved(2, 2), **call)
               for ref in ("moving", "constant")}
        grads = tr.grads()
    term = fi.IterTerm(None, c.r, 1e-2, 2, 2, pairing="frame", moving=True)
    r = fs.run_flow(wts, list(c.ch), frames, term=term, leaf="frames", **call)
    assert out["moving"][0] == out["constant"][0] and abs(out["moving"][0] - r.loss) <= 1e-5 * r.scale
    _check_grads(grads, r.grads, what="moving")
    check_frame_grads(out["moving"][1], r.frame_grad, "moving", zero=set())
    assert np.abs(out["moving"][1] - out["constant"][1]).max() > 0


def test_refine_stills_climbs_the_solved_score_as_the_reference_does(cuda):
    """`refine_stills` with `DenseFitness.solve_objective()` (Circles, 2 levels x 2 iterations) at the settings of
    tests/flow_iter_support.py `refine_reference`: reproducible, the kept columns untouched, no byte moves by more than 16, the first
    term is the reference's, and the term moves in the direction it moves on the float64 reference (tests/test_flow_iter_host.py records
    which that is; whether a score rises under this step rule is a property of the case)."""
    from tests import flow_ref_support as rs
    from tests.frame_grad_support import case_inputs
    w, h, ch = fi.REFINE_SHAPE
    frames, sets = case_inputs(w, h, tuple(ch), 2, 5)
    stills = np.ascontiguousarray(frames[:, 0])
    flow = fi.refine_fitness().solve_objective()
    assert flow.solve == (fi.REFINE_LEVELS, fi.REFINE_ITERS) and train._entry_key(flow) == "iter"
    kw = dict(requant=False, objective="flow", flow=flow, mask=rs.refine_mask(w, h), **rs.REFINE)
    with PredNetTrainer(sets["live"], list(ch), w, h, 2, 6) as tr:
        out, hist = train.refine_stills(tr, stills, **kw)
        out2, hist2 = train.refine_stills(tr, stills, **kw)
    _, ref_hist = fi.refine_reference()
    print("refine through the solve: %s (reference: %s)" % (" ".join("%.5e" % v for v in hist), " ".join("%.5e" % v for v in ref_hist)))
    assert np.array_equal(out, out2) and np.array_equal(hist, hist2) and np.isfinite(hist).all()
    assert np.array_equal(out[..., :w // 4], stills[..., :w // 4]) and (out != stills).any()
    assert np.abs(out.astype(np.int32) - stills).max() <= 8 * 2
    assert abs(hist[0] - ref_hist[0]) <= 1e-5 * max(abs(ref_hist[0]), 1e-30)
    if abs(ref_hist[-1] - ref_hist[0]) > 1e-3 * abs(ref_hist[0]):
        assert (hist[-1] > hist[0]) == (ref_hist[-1] > ref_hist[0]), (hist, ref_hist)


def test_refine_genomes_climbs_the_solved_score_as_the_reference_does(cuda):
    """`refine_genomes` with `DenseFitness.solve_objective()` (Circles, 2 levels x 2 iterations, r 3) at the setting of
    tests/cppn_grad_support.py, the path `examples/evolve_illusion.py --refine-solve fitness` takes: render, the trainer through the new
    entry, the CPPN's parameter gradients, the update.  Reproducible, the inputs untouched, the genomes move and differently than under
    the single step, the last entry of the history is the loss a direct call gives for the returned images, the first term is the
    simulation's of tests/flow_iter_support.py `refine_genomes_reference`, and the term moves in the direction it moves there (it rises,
    0.2542 -> 0.2704)."""
    from tests import cppn_grad_support as S
    from tests.train_support import _weight_sets
    SIM = S.SIM
    w, h, ch = SIM["w"], SIM["h"], list(SIM["ch"])
    n_repeat, n_ext = SIM["n_repeat"], SIM["n_ext"]
    dense = fi.refine_fitness()
    flow, single = dense.solve_objective(), dense.flow_objective()
    assert train._entry_key(flow) == "iter" and train._entry_key(single) == "score"
    kw = dict(n_repeat=n_repeat, n_ext=n_ext, iters=SIM["iters"], lr=SIM["lr"], requant=False, objective="flow")
    cfg, genomes = S.sim_genomes()
    params = lambda g: ({k: (n.bias, n.response) for k, n in g.nodes.items()}, {k: c.weight for k, c in g.connections.items()})
    before = [params(g) for g in genomes]
    with PredNetTrainer(dict(_weight_sets(ch, w, h))["live"], ch, w, h, batch=len(genomes), max_steps=n_repeat + n_ext) as tr:
        out, history, images = train.refine_genomes(tr, genomes, cfg, SIM["structure"], flow=flow, **kw)
        assert tr.debug_flow_iter() > 0
        out2, history2, images2 = train.refine_genomes(tr, genomes, cfg, SIM["structure"], flow=flow, **kw)
        out_s, history_s, _ = train.refine_genomes(tr, genomes, cfg, SIM["structure"], flow=single, **kw)
        frames = np.ascontiguousarray(np.broadcast_to(images[:, None], (len(genomes), n_repeat + n_ext) + images.shape[1:]))
        direct = tr.forward_backward(frames, n_fed=n_repeat, requant=False, step_weights=[0.0] * n_repeat + [1.0] * (n_ext - 1), objective="flow", flow=flow)
    _, ref_hist = fi.refine_genomes_reference()
    print("refine_genomes through the solve: %s (reference: %s)" % (" ".join("%.5e" % v for v in history), " ".join("%.5e" % v for v in ref_hist)))
    assert np.isfinite(history).all() and history.tobytes() == history2.tobytes() and images.tobytes() == images2.tobytes()
    assert [params(g) for g in out] == [params(g) for g in out2] and [params(g) for g in genomes] == before
    assert any(params(a) != b for a, b in zip(out, before)) and any(params(a) != params(b) for a, b in zip(out, out_s))
    assert history[0] != history_s[0] and history[-1] == direct
    assert abs(history[0] - ref_hist[0]) <= 1e-5 * abs(ref_hist[0])
    assert ref_hist[-1] > ref_hist[0] and history[-1] > history[0], (history, ref_hist)


def _raw_iter_term(tr, cuda, pred, ref, flow, solve, scale):
    """eigen_trainer_flow_term_iter called directly: ref uint8 or float32 [n, C, H, W]; solve None (NULL) or (levels, iters).
    -> (value, u, seed, reference gradient, records)"""
    import ctypes
    import torch
    from evolutionary_illusion_generator_amd.engine import DenseSolveC, _ptr
    n, C, h, w = pred.shape
    per = C * h * w
    p, r = torch.from_numpy(pred).to(cuda), torch.from_numpy(ref).to(cuda)
    float_ref = ref.dtype == np.float32
    d_dir, d_mask = flow.on_device(torch, tr.device, h, w)
    cfg = flow.settings(stage_alone=True)
    sc = flow.score.settings(h) if flow.score is not None else None
    by_circles = isinstance(flow.score, train.FlowScore)
    mem = flow.members_settings(n, h, w) if flow.score is not None else None
    by = lambda x: None if x is None else ctypes.byref(x)
    value, rec = ctypes.c_double(), np.zeros((n, 10), np.float64)
    u = torch.empty((n, 2, h, w), dtype=torch.float64, device=cuda)
    seed, rg = (torch.empty((n, C, h, w), dtype=torch.float32, device=cuda) for _ in range(2))
    s = None if solve is None else DenseSolveC(*solve)
    rc = tr.lib.eigen_trainer_flow_term_iter(tr._h, _ptr(p), ctypes.c_int64(per), None if float_ref else _ptr(r), _ptr(r) if float_ref else None, ctypes.c_int64(per),
                                             ctypes.c_int32(n), ctypes.byref(cfg), _ptr(d_mask), by(sc if by_circles else None), by(None if by_circles else sc), by(mem),
                                             ctypes.c_double(scale), ctypes.byref(value), _ptr(rec), _ptr(u), _ptr(seed), ctypes.c_int64(per), _ptr(rg), ctypes.c_int64(per),
                                             None, _ptr(d_dir), by(s))
    assert rc == 0, tr.lib.eigen_last_error()
    return value.value, u.cpu().numpy(), seed.cpu().numpy(), rg.cpu().numpy(), rec


def test_the_stage_entry_with_no_solve_is_its_namesake(cuda):
    """`eigen_trainer_flow_term_iter` itself with solve NULL and {1, 1}, 20 x 15 colour: under every mode with a byte reference, under the
    displacement modes with a float reference, and under a per-sample mask it returns the bytes of `flow_term` / `flow_term_pair` on the
    objective without a solve (eigen_trainer_flow_term_ref, _pair, _score, _structure, _members), the records included, and the handle
    holds no iterated workspace afterwards."""
    name = "20x15r3"
    _, w, h, C, _, _, r, _, _ = fi.stage_case(name)
    img0, img1 = fi.stage_images(name)
    pred, prev = fi.as_floats(img1), fi.as_floats(img0)
    rng = np.random.default_rng(11)
    masks = (rng.random((len(img0), h, w)) < 0.8).astype(np.uint8)
    cases = [(mode, img0, None) for mode in fi.MODES] + [("energy", prev, None), ("horizontal", prev, None), ("circles", img0, masks), ("free", prev, masks)]
    with _trainer(name) as tr:
        for mode, ref, mask in cases:
            direction, score = fi.mode_objects(mode, w, h)
            flow = FlowObjective(r, fi.EPS, direction, mask, score=score)
            if ref.dtype == np.uint8:
                want = tr.flow_term(pred, ref, flow, scale=SCALE, reference_grad=True)
            else:
                want = tr.flow_term_pair(pred, ref, flow, scale=SCALE, reference_grad=True)
            want_rec = tr.last_flow_stats
            for solve in (None, (1, 1)):
                got = _raw_iter_term(tr, cuda, pred, ref, flow, solve, SCALE)
                what = (mode, str(ref.dtype), mask is not None, solve)
                assert got[0] == want[0], what
                assert all(x.tobytes() == y.tobytes() for x, y in zip(got[1:4], want[1:4])), what
                assert (want_rec is None and not got[4].any()) or got[4].tobytes() == want_rec.tobytes(), what
                assert np.abs(got[2]).max() > 0 and np.abs(got[3]).max() > 0, what
        assert tr.debug_flow_iter() == 0


def _raw_iter_loss_grad(tr, cuda, frames, flow, solve):
    """eigen_trainer_loss_grad_flow_iter called directly: one reset, teacher-forced call with per-frame frame gradients.
    -> (loss, terms, frame gradient [B, T, C, H, W], records or None)"""
    import ctypes
    import torch
    from evolutionary_illusion_generator_amd.engine import DenseSolveC, _ptr
    B, T, C, h, w = frames.shape
    per = C * h * w
    d = torch.from_numpy(frames).to(cuda)
    d_dir, d_mask = flow.on_device(torch, tr.device, h, w)
    cfg = flow.settings()
    sc = flow.score.settings(h) if flow.score is not None else None
    by_circles = isinstance(flow.score, train.FlowScore)
    mem = flow.members_settings(B, h, w) if flow.score is not None else None
    by = lambda x: None if x is None else ctypes.byref(x)
    loss, terms = ctypes.c_double(), np.zeros(T - 1, np.float64)
    stats = np.zeros((T - 1, B, 10), np.float64) if mem is not None else None
    buf = torch.empty((B, T, C, h, w), dtype=torch.float32, device=cuda)
    s = None if solve is None else DenseSolveC(*solve)
    rc = tr.lib.eigen_trainer_loss_grad_flow_iter(tr._h, _ptr(d), ctypes.c_int64(T * per), ctypes.c_int32(B), ctypes.c_int32(T), ctypes.c_int32(T), ctypes.c_int32(0),
                                                  ctypes.c_int32(1), None, ctypes.c_int32(2), None, ctypes.byref(loss), None, None, _ptr(buf), ctypes.c_int64(T * per),
                                                  ctypes.c_int64(per), ctypes.byref(cfg), _ptr(d_dir), _ptr(d_mask), _ptr(terms), ctypes.c_int32(train.FLOW_PAIRINGS[flow.pairing]),
                                                  by(sc if by_circles else None), by(None if by_circles else sc), by(mem), _ptr(stats), None, by(s))
    assert rc == 0, tr.lib.eigen_last_error()
    return loss.value, terms, buf.cpu().numpy(), stats


def test_the_training_entry_with_no_solve_is_its_namesake(cuda):
    """`eigen_trainer_loss_grad_flow_iter` itself with solve NULL and {1, 1}, 16 x 12 [3, 4, 6], T = 5: loss, terms, every weight gradient,
    the frame gradient and the records are the bytes of `forward_backward` on the objective without a solve, under the prediction
    pairing (energy), the frame pairing with a direction field, the moving reference under the Circles score and a per-sample mask under
    the Bands score; the handle holds no iterated workspace afterwards."""
    c = ps.PairCase(16, 12, (3, 4, 6), "live", "energy", 7, "drifting")
    frames, wts = ps.pair_case_frames(c), ps.pair_case_weights(c)
    B, T = frames.shape[:2]
    rng = np.random.default_rng(12)
    masks = (rng.random((B, c.h, c.w)) < 0.8).astype(np.uint8)
    flows = [PredictionFlow(7, 1e-2), FlowObjective(3, 1e-2, train.flow_direction("horizontal", c.w, c.h)),
             FlowObjective(7, 1e-2, score=train.FlowScore(max_norm=2.0, min_count=4), reference="moving"),
             PredictionFlow(3, 1e-2, mask=masks).scored(train.BandsScore(max_norm=2.0))]
    sha = lambda g: _sha(*[g[k] for k in sorted(g)])
    with PredNetTrainer(wts, list(c.ch), c.w, c.h, B, T) as tr:
        for flow in flows:
            tr.last_flow_stats = None
            loss, per, terms = tr.forward_backward(frames, frame_grads="frames", flow_terms=True, objective="flow", flow=flow)
            want_g, want_stats = sha(tr.grads()), tr.last_flow_stats
            for solve in (None, (1, 1)):
                got = _raw_iter_loss_grad(tr, cuda, frames, flow, solve)
                what = (train._entry_key(flow), solve)
                assert got[0] == loss and got[1].tobytes() == terms.tobytes() and got[2].tobytes() == per.tobytes() and sha(tr.grads()) == want_g, what
                assert (got[3] is None) == (want_stats is None) and (got[3] is None or got[3].tobytes() == want_stats.tobytes()), what
            assert loss != 0 and np.abs(per).max() > 0
        assert tr.debug_flow_iter() == 0


@pytest.mark.parametrize("mode", ["circles", "bands", "free"])
def test_the_records_under_a_solve_meet_the_dense_fitness_bounds(cuda, mode):
    """48 x 32, 2 levels x 3 iterations, `flow_term(stats=True)`: the records [n, 10] of the samples meet `check_records` of
    tests/test_gpu_dense_fitness.py against the restatement's score on `dense_pyr_ref`'s field (N exact, every record sum within
    N 2^-53 sum |terms|, S_b within 1e-10), the value is the mean of the S_b, and `last_flow_stats` holds the same records"""
    from tests.test_gpu_dense_fitness import check_records
    name = "48x32"
    _, w, h, C, levels, iters, r, _, _ = fi.stage_case(name)
    img0, img1 = fi.stage_images(name)
    flow = fi.make_objective(mode, w, h, r, levels, iters)
    sc = fi.support_score(flow.score, h)
    with _trainer(name) as tr:
        value, u, seed, rec = tr.flow_term(fi.as_floats(img1), img0, flow, stats=True)
        assert tr.last_flow_stats.tobytes() == rec.tobytes()
    check_records(rec, np.ascontiguousarray(rec[:, 8]), dp.Want(_field(name), sc), sc)
    assert (rec[:, 0] >= 4).all() and value == (rec[0, 8] + rec[1, 8] + rec[2, 8]) / 3.0


def test_a_training_call_under_a_solve_keeps_the_records_of_its_terms(cuda):
    """16 x 12 [3, 4, 6], T = 5, prediction pairing, the Circles score under a per-sample mask, 2 x 2, weights [0, 0, 1, 1]:
    `last_flow_stats` [T - 1, n, 10] holds zeros for the terms that are not computed and, for term s, the bytes of the records the stage
    alone leaves on the call's own predictions P0_s against P0_{s-1}"""
    c = ps.PairCase(16, 12, (3, 4, 6), "live", "energy", 3, "drifting")
    frames, wts = ps.pair_case_frames(c), ps.pair_case_weights(c)
    B, T = frames.shape[:2]
    rng = np.random.default_rng(13)
    masks = (rng.random((B, c.h, c.w)) < 0.8).astype(np.uint8)
    flow = PredictionFlow(3, 1e-2, mask=masks).scored(train.FlowScore(max_norm=2.0, min_count=4)).solved(2, 2)
    with PredNetTrainer(wts, list(c.ch), c.w, c.h, B, T) as tr:
        loss, pred = tr.forward_backward(frames, pred=True, objective="flow", flow=flow, step_weights=[0.0, 0.0, 1.0, 1.0])
        stats = tr.last_flow_stats
        assert stats.shape == (T - 1, B, 10) and not stats[:2].any()
        for s in (2, 3):
            tr.flow_term_pair(np.ascontiguousarray(pred[:, s]), np.ascontiguousarray(pred[:, s - 1]), flow)
            assert tr.last_flow_stats.tobytes() == stats[s].tobytes() and (stats[s][:, 0] >= 4).all(), s
        assert abs(loss - (stats[2][:, 8].mean() + stats[3][:, 8].mean()) / 2.0) <= 1e-15       # the loss is the weighted mean of the terms, a term the mean of its S_b
