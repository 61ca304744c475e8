"""CPU: the test-owned dense-prediction head (tests/dpt_layout.py) against fixture G26 — what the REFERENCE's own DPTHead returned on the three
tiny cases with the deterministic weights of `fill_params` (tools/make_golden_g26.py) — and its separable position tables against the tables the
reference's `_apply_pos_embed` arithmetic gave."""
import pytest
import torch

import dpt_layout as DL
from conftest import load_golden
from test_teacher_runner_ref import fill_params


@pytest.mark.parametrize("case", list(DL.CASES))
def test_layout_reproduces_the_reference_head(case):
    g = load_golden("g26_dpt_head")
    m = DL.make_head(case)
    assert DL.param_layout(m) == g[f"{case}_param_layout"]            # the name order fill_params depends on
    fill_params(m)
    toks, img = DL.seeded_inputs(case)
    for i, t in enumerate(toks):
        assert torch.equal(t, g[f"{case}_tokens_{i}"])                # inputs bit-equal
    assert list(img.shape[-2:]) == g[f"{case}_image_hw"].tolist()
    taps = {}
    with torch.no_grad():
        res = m(toks, img, DL.PREFIX, taps=taps)
    got = {"features": res} if torch.is_tensor(res) else {"preds": res[0], "conf": res[1]}
    got["pre"] = taps["pre"]
    for name, t in got.items():
        want = g[f"{case}_{name}"]
        e, bound = float((t - want).abs().max()), 1e-4 * float(want.abs().max())
        print(f"case {case} {name}: max abs err {e:.3e} (bound {bound:.3e})")
        assert t.shape == want.shape and e <= bound, name
    if case == "c":
        assert got["features"].shape == (1, DL.FRAMES, 16, 21, 35)


def test_layout_position_tables_equal_the_reference_embedding():
    g = load_golden("g26_dpt_head")
    H, W = g["a_image_hw"].tolist()
    px, py = DL.pos_tables(W, H, DL.FEATURES // 2, W / H)
    assert px.shape == g["a_px"].shape == (W, DL.FEATURES // 4) and py.shape == g["a_py"].shape == (H, DL.FEATURES // 4)
    assert torch.equal(px, g["a_px"]) and torch.equal(py, g["a_py"])


def test_chunking_does_not_change_the_layout():
    m = DL.make_head("a")
    fill_params(m)
    toks, img = DL.seeded_inputs("a")
    with torch.no_grad():
        a, b = m(toks, img, DL.PREFIX), m(toks, img, DL.PREFIX, frames_chunk_size=1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
