"""GPU tests of the score kernels (csrc/score_kernels.h) on degenerate vectors: the hand-built sets of tests/flow_config_support.py -- an
exactly zero displacement, norms on both float32 neighbours of the plausibility limits, 24 / 25 vectors AFTER the filter, fewer than two
vectors inside the Circles radius, a point on the image centre, y == lim1 and y == middle in Bands with h / 4 fractional, 14 / 15 / 16
vectors in Free, pairs nearer than, at and beyond 100 px, counts above K, K = 128 and K = 1 -- at four geometries, all four structures and the
inside_outside scorer, against oracle/scores.py.  NaN must appear on both sides or on neither; the finite scores agree within the tolerance
of test_scores_match_oracle (rel 1e-9, abs 1e-12: sequential device sums against numpy's pairwise ones, two acos implementations).
tests/test_flow_config_host.py checks with the oracle alone that every branch the sets are built for is taken."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from evolutionary_illusion_generator_amd.engine import Engine
from tests import flow_config_support as fc

INSIDE_OUTSIDE = 4


def _run(cuda, w, h, K, structure, cases):
    import torch
    B = len(cases)
    vec = np.zeros((B, K, 4), np.float32)
    cnt = np.zeros(B, np.int32)
    for b, (_, v, n) in enumerate(cases):
        vec[b, :len(v)] = v
        cnt[b] = n
    e = Engine(w, h, [1, 4], B, max_corners=K)
    assert e.K == K
    df = torch.full((B,), 12345.0, dtype=torch.float64, device=cuda)
    e.score(structure, torch.from_numpy(vec).to(cuda), torch.from_numpy(cnt).to(cuda), B, df)
    torch.cuda.synchronize()
    got = df.cpu().numpy()
    e.close()
    return got


def _compare(got, ref, cases, what):
    worst = 0.0
    for b, (name, _, _) in enumerate(cases):
        assert np.isnan(got[b]) == np.isnan(ref[b]), "%s, case %s: %r vs oracle %r" % (what, name, got[b], ref[b])
        if not np.isnan(ref[b]):
            if ref[b] != 0:
                worst = max(worst, abs(got[b] - ref[b]) / abs(ref[b]))
    print("SCORE_DEV %s: worst relative deviation %.3g over %d cases (%d NaN, %d zero)" % (
        what, worst, len(cases), int(np.isnan(ref).sum()), int((ref == 0).sum())))
    for b, (name, _, _) in enumerate(cases):
        if not np.isnan(ref[b]):
            assert got[b] == pytest.approx(ref[b], rel=1e-9, abs=1e-12), "%s, case %s: %r vs oracle %r" % (what, name, got[b], ref[b])


@pytest.mark.parametrize("structure", [0, 1, 2, 3])
@pytest.mark.parametrize("w,h,K", fc.SCORE_GEOMETRIES)
def test_score_edge_cases_match_oracle(cuda, w, h, K, structure):
    from oracle import scores
    cases = fc.score_cases(w, h, K)
    got = _run(cuda, w, h, K, structure, cases)
    ref = np.array([scores.fitness_from_vectors(structure, v[:min(n, K)].astype(np.float64), w, h) for _, v, n in cases])
    _compare(got, ref, cases, "%dx%d K=%d structure %d" % (w, h, K, structure))


@pytest.mark.parametrize("w,h,K", fc.SCORE_GEOMETRIES)
def test_inside_outside_edge_cases_match_oracle(cuda, w, h, K):
    from oracle import scores
    cases = fc.io_cases(w, h, K)
    got = _run(cuda, w, h, K, INSIDE_OUTSIDE, cases)
    ref = np.array([scores.inside_outside_score(v[:min(n, K)].astype(np.float64), w, h) for _, v, n in cases])
    assert np.isfinite(ref).all()
    _compare(got, ref, cases, "%dx%d K=%d inside_outside" % (w, h, K))


def test_score_edge_census():
    """over the whole file: every listed branch taken (by the oracle's intermediate counts), >= 3 NaN, >= 3 exact zeros, at least half finite and non-zero"""
    n_nan, n_zero, n_live = fc.check_score_census(fc.score_table())
    print("census: %d NaN, %d zero, %d finite and non-zero" % (n_nan, n_zero, n_live))
