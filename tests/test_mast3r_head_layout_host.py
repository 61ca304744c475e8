"""CPU: the test-owned MASt3R head (tests/mast3r_head_layout.py) against fixture G27 — what the REFERENCE's own Cat_MLP_LocalFeatures_DPT_Pts3d
returned on the tiny cases with the deterministic weights of `fill_params` (tools/make_golden_g27.py)."""
import pytest
import torch

import mast3r_head_layout as ML
from conftest import load_golden
from test_teacher_runner_ref import fill_params


@pytest.mark.parametrize("case", list(ML.CASES))
def test_layout_reproduces_the_reference_head(case):
    g = load_golden("g27_mast3r_head")
    cfg = ML.CASES[case]
    m = ML.make_head(case)
    assert ML.param_layout(m) == g[f"{case}_param_layout"]            # the name order fill_params depends on
    fill_params(m)
    decout, (H, W) = ML.seeded_inputs(case)
    for hook in ML.HOOKS:
        assert torch.equal(decout[hook], g[f"{case}_tokens_{hook}"])  # inputs bit-equal
    assert [H, W] == g[f"{case}_image_hw"].tolist() == [cfg["grid"][0] * ML.PATCH, cfg["grid"][1] * ML.PATCH]
    taps = {}
    with torch.no_grad():
        got = m(decout, (H, W), taps=taps)
    assert set(got) == {"pts3d", "desc", "desc_conf"} | ({"conf"} if cfg["has_conf"] else set())
    assert f"{case}_conf" in g or not cfg["has_conf"]
    got["pre"] = taps["pre"]
    for name, t in got.items():
        want = g[f"{case}_{name}"]
        e, bound = float((t - want).abs().max()), 1e-4 * float(want.abs().max())
        print(f"case {case} {name}: max abs err {e:.3e} (bound {bound:.3e})")
        assert t.shape == want.shape and e <= bound, name
    D = cfg["local_feat_dim"]
    assert got["pre"].shape == (1, 3 + cfg["has_conf"] + D + cfg["two_confs"], H, W) and got["desc"].shape == (1, H, W, D)
    assert float((got["desc"].norm(dim=-1) - 1).abs().max()) <= 1e-6
    if not cfg["two_confs"]:
        assert torch.equal(got["desc_conf"], got["conf"])


def test_cases_cover_what_the_fused_head_must_serve():
    grids = [c["grid"] for c in ML.CASES.values()]
    assert (3, 5) in grids and (2, 4) in grids and (1, 2) in grids
    assert {c["two_confs"] for c in ML.CASES.values()} == {True, False} and any(not c["has_conf"] for c in ML.CASES.values())
    assert max(c["local_feat_dim"] for c in ML.CASES.values()) == 24
