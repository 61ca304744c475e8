"""CPU: the test-owned tracker tree (tests/tracker_layout.py) against what the REFERENCE's own BaseTrackerPredictor returned (fixture G28,
tools/make_golden_g28.py): same parameter layout, and with the same deterministic fill the same correlation samples, per-iteration coordinates,
visibility and confidence, to 1e-4 of the maximum."""
import pytest
import torch

import tracker_layout as TL


@pytest.mark.parametrize("case", list(TL.CASES))
def test_layout_reproduces_the_reference_tracker(golden, case):
    g = golden("g28_vggt_tracker")
    trk = TL.make_tracker(case)
    assert TL.param_layout(trk) == g[f"{case}_param_layout"]
    q, fmaps = TL.seeded_inputs(case)
    taps = {}
    with torch.no_grad():
        coords, vis, conf = trk(q, fmaps, iters=TL.ITERS, taps=taps)
    c = TL.CASES[case]
    assert len(coords) == TL.ITERS and coords[0].shape == (c["B"], c["S"], c["N"], 2) and vis.shape == conf.shape == (c["B"], c["S"], c["N"])
    for name, got in (("corr", taps["corr"]), ("coords", torch.stack(coords)), ("vis", vis), ("conf", conf)):
        want = g[f"{case}_{name}"]
        assert got.shape == want.shape, name
        assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max()), name


def test_prepare_iterate_finish_are_forward_cut_at_the_iteration():
    trk = TL.make_tracker("c")
    q, fmaps = TL.seeded_inputs("c")
    with torch.no_grad():
        coords, vis, feats, qfeat, conf = trk(q, fmaps, iters=2, return_feat=True, down_ratio=2, apply_sigmoid=False)
        st = trk.prepare(q, fmaps, down_ratio=2)
        steps = [trk.iterate(st) for _ in range(2)]
        v2, c2 = trk.finish(st, apply_sigmoid=False)
    assert all(torch.equal(a, b) for a, b in zip(coords, steps)) and torch.equal(vis, v2) and torch.equal(conf, c2)
    assert torch.equal(feats, st["feats"]) and torch.equal(qfeat, st["query_feat"])
    assert torch.equal(coords[-1][:, 0], q.expand_as(coords[-1][:, 0]))           # frame 0 stays the query, back at image scale


def test_cached_position_table_changes_nothing():
    q, fmaps = TL.seeded_inputs("c")
    with torch.no_grad():
        a = TL.make_tracker("c")(q, fmaps, iters=2)
        b = TL.make_tracker("c", cache_pos_embed=True)(q, fmaps, iters=2)
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and torch.equal(a[1], b[1])
