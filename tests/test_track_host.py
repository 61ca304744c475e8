"""CPU: host side of the TAP-Vid tracking evaluation (gd_amd.evaluate) — grid coordinates and disc sizes, the sampling map, the
lower-median rule, the metric restatement against the reference's recorded metrics (G24), the argument checks of
gd_track_points that fire before any HIP call, and the fp64 restatement of the tracker (tests/track_ref64.py) against the
reference's own fp64 run (G24)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gd_amd  # noqa: F401
import track_ref64 as R64
from gd_amd import evaluate as E
from gd_amd import ops
from gd_amd._lib import GdHipError, SIGNATURES

G24 = os.path.join(os.path.dirname(__file__), "golden", "g24_tapvid_tracking.npz")
TAGS = ("p16", "p14")


def _g24():
    return np.load(G24, allow_pickle=False)


def _bench(z, tag):
    bh, bw = (int(v) for v in z[f"{tag}.bench.hw"])
    frames = [int(f) for f in z[f"{tag}.bench.frames"]]
    cfg = {"video_idx": 0, "h": bh, "w": bw, "query_points": {}, "target_points": {}, "occluded": {}}
    for f in frames:
        cfg["query_points"][f] = z[f"{tag}.bench.q{f}"]
        cfg["target_points"][f] = z[f"{tag}.bench.t{f}"]
        cfg["occluded"][f] = z[f"{tag}.bench.o{f}"]
    return cfg, frames


def test_grid_coordinates_and_disc_sizes():
    g = E.track_geometry(464, 848, 16, 8)                          # DAVIS at p16 / s8: 476x854 floored to 464x848
    assert g == (464, 848, 16, 8, 57, 105, 105)
    xy = E.grid_xy(g)
    assert xy.shape == (57 * 105, 2)
    assert xy[0].tolist() == [8.0, 8.0] and xy[105 + 2].tolist() == [8.0 + 16, 8.0 + 8]
    assert xy[-1].tolist() == [8.0 + 104 * 8, 8.0 + 56 * 8]
    # an interior cell: (8 dx)^2 + (8 dy)^2 <= 35^2  <=>  dx^2 + dy^2 <= 19 -> 61 lattice points; bounded by (2 ceil(r / s) + 1)^2
    inner = 30 * 105 + 50
    assert len(E.disc_cells(g, 35, inner)) == 61 <= (2 * 5 + 1) ** 2
    assert len(E.disc_cells(g, 35, 0)) == sum(1 for dx in range(0, 6) for dy in range(0, 6) if dx * dx + dy * dy <= 19)
    g14 = E.track_geometry(476, 854, 14, 7)
    assert g14[4:6] == (67, 121)
    assert len(E.disc_cells(g14, 35, 30 * 121 + 60)) == sum(1 for dx in range(-5, 6) for dy in range(-5, 6) if dx * dx + dy * dy <= 25)
    # the integer rule equals the fp32 norm rule of the reference for integer radius
    d = (E.grid_xy(g).float() - E.grid_xy(g).float()[inner]).norm(dim=-1) <= 35
    assert sorted(d.nonzero().reshape(-1).tolist()) == E.disc_cells(g, 35, inner)
    assert torch.equal(R64.disc_mask(16, 8, 57, 105, 35, inner).nonzero().reshape(-1), torch.tensor(E.disc_cells(g, 35, inner)))


def test_sampling_map_is_keypoint_grid_coords():
    pts = torch.rand(200, 2, generator=torch.Generator().manual_seed(0)) * torch.tensor([848.0, 464.0])
    for (H, W, p, s) in ((464, 848, 16, 8), (476, 854, 14, 7), (96, 128, 16, 8)):
        lh = ((H - p) // s) * s + p / 2
        lw = ((W - p) // s) * s + p / 2
        a = torch.tensor([[2 / (lw - p / 2), 2 / (lh - p / 2), 1]])            # normalize_points_for_sampling (x, y, t)
        b = torch.tensor([[1 - lw * 2 / (lw - p / 2), 1 - lh * 2 / (lh - p / 2), 0]])
        p3 = torch.cat([pts, torch.zeros(200, 1)], 1)
        want = (a * p3 + b)[:, :2]
        assert torch.equal(E.keypoint_grid_coords(pts, H, W, p, s), want)


def test_lower_median_rule():
    g = torch.Generator().manual_seed(1)
    for n in (1, 2, 3, 4, 7, 10):
        x = torch.randn(n, 13, generator=g)
        assert torch.equal(E.lower_median(x, 0), torch.median(x, dim=0).values)
        assert torch.equal(R64.lower_median(x.double(), 0), torch.median(x.double(), dim=0).values)
    x = torch.tensor([[1.0], [4.0], [2.0], [3.0]])
    assert float(E.lower_median(x, 0)) == 2.0                                   # even count: the lower middle value


@pytest.mark.parametrize("tag", TAGS)
def test_metrics_equal_the_reference(tag):
    z = _g24()
    cfg, frames = _bench(z, tag)
    qp, tr32, oc32 = torch.from_numpy(z[f"{tag}.qp"]), z[f"{tag}.tr32"], z[f"{tag}.oc32"]
    H, W = (int(v) for v in z[f"{tag}.geom"][:2])
    trd = {f: tr32[(qp[:, 2] == f).numpy()] for f in frames}
    ocd = {f: oc32[(qp[:, 2] == f).numpy()] for f in frames}
    got = E.compute_tapvid_metrics_for_video(trd, ocd, {"videos": [cfg]}, 0, pred_video_sizes=[W, H])
    names, vals = [str(n) for n in z[f"{tag}.metric_names"]], z[f"{tag}.metric_values"]
    assert sorted(got) == names
    for n, v in zip(names, vals):
        assert abs(got[n] - float(v)) <= 1e-12, n
    # the :203-204 rescale quirk (column 2 from the overwritten column 1) has no effect: only the frame column is read
    cfg2 = dict(cfg, query_points={f: np.asarray(q)[:, ::-1] * 3.0 + 17.0 for f, q in cfg["query_points"].items()})
    got2 = E.compute_tapvid_metrics_for_video(trd, ocd, {"videos": [cfg2]}, 0, pred_video_sizes=[W, H])
    assert got2 == got


def test_metrics_query_modes():
    qp = np.array([[[0, 5, 5], [2, 5, 5]]], dtype=np.float32)
    gt = np.zeros((1, 2, 3, 2), np.float32)
    occ = np.zeros((1, 2, 3), bool)
    pred = gt + np.array([0.5, 0.0], np.float32)
    m = E.compute_tapvid_metrics(qp, occ, gt, occ, pred, "strided")
    assert float(m["pts_within_1"][0]) == 1.0 and float(m["occlusion_accuracy"][0]) == 1.0
    m = E.compute_tapvid_metrics(qp, occ, gt, occ, pred + np.array([1.0, 0.0], np.float32), "first")
    assert float(m["pts_within_1"][0]) == 0.0 and float(m["pts_within_2"][0]) == 1.0
    with pytest.raises(ValueError):
        E.compute_tapvid_metrics(qp, occ, gt, occ, pred, "all")


def _call(**kw):
    from gd_amd._lib import lib
    a = dict(E=1 << 20, F=1 << 20, Es=1 << 20, Fs=1 << 20, dtype=0, src=0, rows=256, T=4, gh=57, gw=105, pitch=106, D=768,
             img_h=464, img_w=848, patch=16, stride=8, radius=35, tiles=[[0, 0, 128, 0]], n_out=256)
    a.update(kw)
    t = np.ascontiguousarray(np.asarray(a["tiles"], dtype=np.int32).reshape(-1, 4))
    rc = lib().gd_track_points(a["E"], a["F"], a["Es"], a["Fs"], a["dtype"], a["src"], a["rows"], a["T"], a["gh"], a["gw"], a["pitch"],
                               a["D"], a["img_h"], a["img_w"], a["patch"], a["stride"], a["radius"], 1 << 20, 1 << 20, None, None,
                               t.ctypes.data_as(ctypes.c_void_p), t.shape[0], a["n_out"], 1 << 20, None, 1 << 20, None)
    return rc, lib().gd_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(gh=56), "grid"),
    (dict(gw=104, pitch=104), "grid"),
    (dict(pitch=104), "pitch"),
    (dict(D=12), "multiple of 8"),
    (dict(tiles=[[0, 0, 129, 0]]), "rows"),
    (dict(tiles=[[4, 0, 16, 0]]), "frame"),
    (dict(tiles=[[-1, 0, 16, 0]]), "frame"),
    (dict(tiles=[[0, 200, 100, 0]]), "outside E"),
    (dict(tiles=[[0, 0, 100, 200]]), "outside"),
    (dict(T=1 << 15, gh=1 << 10, img_h=8 + 8 * ((1 << 10) - 1) + 8), "2^31"),
    (dict(dtype=3, src=1), "recompute"),
    (dict(Es=2 << 20), "own recompute"),
    (dict(E=(1 << 20) + 8, Es=(1 << 20) + 8), "aligned"),
    (dict(patch=0), "geometry"),
])
def test_argument_checks_fire_before_any_hip_call(kw, msg):
    rc, err = _call(**kw)
    assert rc == -1 and msg in err, err


def test_python_argument_checks():
    with pytest.raises(GdHipError, match="precision"):
        ops.TrackFeatures(torch.zeros(2, 6, 16), precision="tf32")
    with pytest.raises(GdHipError, match="CUDA"):
        ops.TrackFeatures(torch.zeros(2, 6, 16), precision="f32")
    with pytest.raises(GdHipError):
        E.track_geometry(10, 848, 16, 8)
    o, t = ops.track_tiles(torch.tensor([3, 1, 3, 1, 1] + [2] * 130))
    assert t.tolist()[:2] == [[1, 0, 3, 0], [2, 3, 128, 3]] and t.tolist()[2:] == [[2, 131, 2, 131], [3, 133, 2, 133]]
    assert o[:3].tolist() == [1, 3, 4]


def test_new_entry_points_are_bound():
    for name in ("gd_track_points", "gd_track_points_workspace_bytes", "gd_track_row_norms"):
        assert name in SIGNATURES
    from gd_amd._lib import lib
    L = lib()
    assert L.gd_track_points_workspace_bytes(10) >= 160
    assert L.gd_track_points_workspace_bytes(0) == 0


@pytest.mark.parametrize("tag", TAGS)
def test_fp64_restatement_reproduces_the_reference(tag):
    z = _g24()
    H, W, p, s, gh, gw = (int(v) for v in z[f"{tag}.geom"])
    feats = torch.from_numpy(z[f"{tag}.feats"]).permute(0, 2, 3, 1).double()
    qp = torch.from_numpy(z[f"{tag}.qp"])
    r = R64.infer(feats, (H, W, p, s, gh, gw), qp)
    assert float((r["tracks"] - torch.from_numpy(z[f"{tag}.tr64"])).abs().max()) <= 1e-9
    assert torch.equal(r["occ"], torch.from_numpy(z[f"{tag}.oc64"]))
    assert float((r["cos"] - torch.from_numpy(z[f"{tag}.cos64"])).abs().max()) <= 1e-12
    # the fixture's conditions: anchors non-empty, 25-75 % visible, the fp32 and fp64 reference runs agree on every flag
    assert all(a.numel() > 0 for a in r["anchors"].values())
    assert 0.25 <= 1 - float(r["occ"].float().mean()) <= 0.75
    assert np.array_equal(z[f"{tag}.oc32"], z[f"{tag}.oc64"])
    assert float(z[f"{tag}.ref_dev_px"]) < 1e-3
