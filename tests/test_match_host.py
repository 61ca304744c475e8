"""CPU: host side of the correspondence evaluation (gd_amd.evaluate) — the transfer field's geometry, the reference's patch-14
query mapping at 640, the PCK formula, and the argument checks that fire before any kernel runs."""
import pytest
import torch
import torch.nn.functional as F

import gd_amd  # noqa: F401
import gd_oracle as O
from gd_amd import ops
from gd_amd._lib import GdHipError, SIGNATURES


def test_transfer_geometry_at_p16_640():
    from gd_amd.evaluate import transfer_geometry
    g = transfer_geometry(640, 640, 16, 16)
    # src/evaluate_timm.py:469-471, 531-538: ph = 1 + (640 - 16) // 16, ds = ((640 - 16) // 16) * 16 + 1, pads 8 / 640 - 625 - 8
    assert (g["gh"], g["gw"]) == (40, 40)
    assert (g["ds_h"], g["ds_w"]) == (625, 625)
    assert (g["top"], g["left"], g["bottom"], g["right"]) == (8, 8, 7, 7)
    assert g["top"] + g["ds_h"] + g["bottom"] == 640


def test_transfer_geometry_other_backbones():
    from gd_amd.evaluate import transfer_geometry
    g = transfer_geometry(640, 640, 14, 7)
    assert (g["gh"], g["ds_h"], g["top"], g["bottom"]) == (90, 624, 7, 9)
    g = transfer_geometry(480, 640, 16, 16)
    assert (g["gh"], g["gw"], g["ds_h"], g["ds_w"]) == (30, 40, 465, 625)
    assert (g["top"], g["bottom"], g["left"], g["right"]) == (8, 7, 8, 7)
    # the padded field is the image, and F.pad's replicate form gives it that size
    up = F.interpolate(torch.zeros(1, 1, g["gh"], g["gw"]), size=(g["ds_h"], g["ds_w"]), mode="bilinear", align_corners=True)
    assert F.pad(up, (g["left"], g["right"], g["top"], g["bottom"]), mode="replicate").shape[-2:] == (480, 640)


def test_query_mapping_is_the_patch14_default_at_640():
    from gd_amd.evaluate import keypoint_grid_coords
    pts = torch.tensor([[7.0, 7.0], [623.0, 623.0], [315.0, 7.0], [0.0, 639.0]])
    g = keypoint_grid_coords(pts, 640, 640)
    assert torch.allclose(g[0], torch.tensor([-1.0, -1.0]), atol=1e-6)
    assert torch.allclose(g[1], torch.tensor([1.0, 1.0]), atol=1e-6)
    assert abs(float(g[2, 0])) < 1e-6
    assert torch.equal(g, O.keypoint_grid_coords(pts[None], 640, 640, 14, 14)[0])     # the oracle's restatement of utils/functions.py
    # the same positions on the patch-16 mapping are NOT the reference's (8 -> -1, 632 -> +1)
    g16 = keypoint_grid_coords(pts, 640, 640, 16, 16)
    assert not torch.allclose(g16, g)


def test_pck_hand_computed():
    from gd_amd.evaluate import pck
    gt = torch.tensor([[100.0, 100.0], [200.0, 50.0], [10.0, 10.0], [300.0, 300.0]])
    pred = torch.tensor([[100, 130], [200, 50], [10, 90], [350, 300]])      # errors 30, 0, 80, 50
    # thresholds at 640: 64 (0.10), 32 (0.05), 96 (0.15)
    r = pck(pred, gt, 640)
    assert r.dtype == torch.float32
    assert torch.equal(r, torch.tensor([3 / 4, 2 / 4, 4 / 4]))
    # strict inequality: an error of exactly alpha * img_size is not correct
    r = pck(torch.tensor([[64, 0]]), torch.tensor([[0.0, 0.0]]), 640, alphas=(0.10,))
    assert float(r[0]) == 0.0


def test_argument_errors():
    from gd_amd import evaluate as E
    with pytest.raises(GdHipError, match="multiple of 8"):
        ops.match_argmax(torch.zeros(4, 12), torch.zeros(5, 12))
    with pytest.raises(GdHipError, match="widths differ"):
        ops.match_argmax(torch.zeros(4, 16), torch.zeros(5, 24))
    with pytest.raises(GdHipError, match="precision"):
        ops.match_argmax(torch.zeros(4, 16), torch.zeros(5, 16), precision="tf32")
    with pytest.raises(GdHipError, match="both directions"):
        ops.match_argmax(torch.zeros(4, 16), torch.zeros(5, 16), both=False, want_mutual=True)
    with pytest.raises(GdHipError, match="does not match"):
        ops.transfer_argmax(torch.zeros(3, 39, 40), (640, 640), 16, 16)       # 640 at p16/s16 is a 40 x 40 grid
    with pytest.raises(GdHipError, match="needs"):
        E.transfer_keypoints_from_tokens(torch.zeros(41 * 40, 32), torch.zeros(40 * 40, 32), torch.zeros(3, 3))
    with pytest.raises(GdHipError):
        E.token_grid(10, 640, 16, 16)


def test_new_entry_points_are_bound():
    for name in ("gd_match_argmax", "gd_match_argmax_workspace_bytes", "gd_transfer_argmax", "gd_transfer_argmax_workspace_bytes"):
        assert name in SIGNATURES


def test_workspace_queries():
    from gd_amd._lib import MATCH_COLS, lib
    L = lib()
    assert L.gd_match_argmax_workspace_bytes(1000, 120000, 0) >= 8 * 1000
    assert L.gd_match_argmax_workspace_bytes(1000, 120000, MATCH_COLS) >= 8 * (1000 + 120000)
    assert L.gd_match_argmax_workspace_bytes(0, 10, MATCH_COLS) == 0
    assert L.gd_transfer_argmax_workspace_bytes(20) >= 160
