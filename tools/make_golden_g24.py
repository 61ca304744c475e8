"""G24 (TAP-Vid tracking evaluation): the reference's own tracker (utils/tracking_model.py Tracker + ModelInference.infer,
batch_size=None) and metrics (utils/tracking_metrics.py compute_tapvid_metrics_for_video) on synthetic features, on the CPU —
build container only.  The one patch: RangeNormalizer's default device 'cuda' -> 'cpu'.

Writes tests/golden/g24_tapvid_tracking.npz: per geometry (p16/s8 and p14/s7) the features [T, C, gh, gw] (a 3x3-smoothed random
field drifting one cell per frame, plus noise), the query points, the reference's tracks / occlusions / cosines from an fp32 and
an fp64 run (torch.set_default_dtype), a synthetic benchmark entry and the reference's metric dict.  Asserts the fixture's
conditions: non-empty anchor sets, 25-75 % visible predictions, fp32 and fp64 runs agreeing on every argmax cell and flag, every
deciding quantity at least 1e-3 (cosines) / 1e-2 px (median distances) from its threshold."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import ref_import as R  # noqa: E402
import track_ref64 as T64  # noqa: E402

R.install()
import utils.tracking_model as TM  # noqa: E402
import utils.tracking_metrics as TMM  # noqa: E402

TM.RangeNormalizer.__init__.__defaults__ = ("cpu",)
OUT = os.path.join(HERE, "..", "tests", "golden", "g24_tapvid_tracking.npz")
GEOMS = {"p16": (96, 128, 16, 8), "p14": (84, 112, 14, 7)}
T_, C, NQ, NOISE = 10, 64, 8, 0.08


def features(gh, gw, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(1, C, gh + 2, gw + T_ + 2, generator=g)
    base = F.avg_pool2d(base, 3, stride=1)                                   # 3x3-smoothed field [C, gh, gw + T]
    fr = torch.stack([base[0, :, :, t:t + gw] for t in range(T_)])          # content moves one cell left per frame
    return (fr + NOISE * torch.randn(fr.shape, generator=g)).contiguous()


def run_ref(feats, geom, qp, dtype):
    H, W, p, s = geom
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        tr = TM.Tracker(feats.to(dtype), torch.zeros(T_, 3, H, W, dtype=dtype), dino_patch_size=p, stride=s, device="cpu")
        mi = TM.ModelInference(model=tr, range_normalizer=tr.range_normalizer, anchor_cosine_similarity_threshold=0.7,
                               cosine_similarity_threshold=0.6)
        with torch.no_grad():
            trajs, occ = mi.infer(query_points=qp, batch_size=None)
            t3 = mi.compute_trajectories(qp)
            cos = mi.compute_trajectory_cos_sims(t3, qp)
    finally:
        torch.set_default_dtype(old)
    return trajs[..., :2].double(), occ.bool(), cos.double()


def one(tag, geom, seed):
    H, W, p, s = geom
    gh, gw = 1 + (H - p) // s, 1 + (W - p) // s
    feats = features(gh, gw, seed)
    g = torch.Generator().manual_seed(seed + 1)
    qx = (torch.rand(NQ, generator=g) * (W - 2 * p) + p).float()
    qy = (torch.rand(NQ, generator=g) * (H - 2 * p) + p).float()
    qt = torch.randint(0, T_, (NQ,), generator=g).float()
    qp = torch.stack([qx, qy, qt], 1)
    tr32, oc32, cos32 = run_ref(feats, geom, qp, torch.float32)
    tr64, oc64, cos64 = run_ref(feats, geom, qp, torch.float64)
    # the restatement (fp64) on the same inputs, for the cells and the margins
    rs = T64.infer(feats.permute(0, 2, 3, 1).double(), (H, W, p, s, gh, gw), qp)
    dev = float((tr32 - tr64).abs().max())
    vis = 1 - float(oc64.float().mean())
    cm = min(float((cos64 - 0.7).abs().min()), float((cos64 - 0.6).abs().min()))
    mm = min(float((med - th).abs()[(med - th).abs() > 0].min()) if bool(((med - th).abs() > 0).any()) else 1e9
             for med, th in rs["meds"].values())
    ok = (dev < 1e-3 and torch.equal(oc32, oc64) and all(a.numel() > 0 for a in rs["anchors"].values()) and 0.25 <= vis <= 0.75
          and cm >= 1e-3 and mm >= 1e-2 and torch.equal(rs["occ"], oc64)
          and float((rs["tracks"] - tr64).abs().max()) < 1e-9)
    # dev < 1e-3 px: the fp32 run picked the fp64 run's argmax cell everywhere (another disc centre moves a point by >= 1 px)
    print(f"{tag} seed {seed}: visible {vis:.2f}  cos margin {cm:.2e}  median margin {mm:.2e}  fp32-fp64 {dev:.2e} px  "
          f"restatement {float((rs['tracks'] - tr64).abs().max()):.1e}  anchors {[a.numel() for a in rs['anchors'].values()]}  ok {ok}")
    if not ok:
        return None
    # benchmark entry: benchmark resolution 2x the frames', ground truth = the fp64 tracks moved by up to 6 px, 20 % occluded
    bh, bw = 2 * H, 2 * W
    qf = sorted(set(int(t) for t in qt.tolist()))
    cfg = {"video_idx": 0, "h": bh, "w": bw, "query_points": {}, "target_points": {}, "occluded": {}}
    tr_d, oc_d = {}, {}
    for f in qf:
        sel = (qt == f).nonzero().reshape(-1)
        cfg["query_points"][f] = (qp[sel, :2].double() * torch.tensor([bw / W, bh / H], dtype=torch.float64)).numpy()
        gt = tr64[sel] * torch.tensor([bw / W, bh / H], dtype=torch.float64) + 6 * torch.rand(len(sel), T_, 2, generator=g) - 3
        cfg["target_points"][f] = gt.numpy()
        cfg["occluded"][f] = (torch.rand(len(sel), T_, generator=g) < 0.2).numpy()
        tr_d[f], oc_d[f] = tr32[sel].float().numpy(), oc32[sel].numpy()
    met = TMM.compute_tapvid_metrics_for_video(tr_d, oc_d, {"videos": [cfg]}, 0, pred_video_sizes=[W, H])
    arr = {f"{tag}.geom": np.array([H, W, p, s, gh, gw]), f"{tag}.feats": feats.numpy(), f"{tag}.qp": qp.numpy(),
           f"{tag}.tr32": tr32.float().numpy(), f"{tag}.tr64": tr64.numpy(), f"{tag}.oc32": oc32.numpy(), f"{tag}.oc64": oc64.numpy(),
           f"{tag}.cos32": cos32.float().numpy(), f"{tag}.cos64": cos64.numpy(), f"{tag}.ref_dev_px": np.array(dev),
           f"{tag}.bench.frames": np.array(qf), f"{tag}.metric_names": np.array(sorted(met)),
           f"{tag}.metric_values": np.array([met[k] for k in sorted(met)])}
    for f in qf:
        arr[f"{tag}.bench.q{f}"] = cfg["query_points"][f]
        arr[f"{tag}.bench.t{f}"] = cfg["target_points"][f]
        arr[f"{tag}.bench.o{f}"] = cfg["occluded"][f]
    arr[f"{tag}.bench.hw"] = np.array([bh, bw])
    print("  metrics", met)
    return arr


arrs = {}
for tag, geom in GEOMS.items():
    for seed in range(240, 290):
        a = one(tag, geom, seed)
        if a is not None:
            arrs.update(a)
            arrs[f"{tag}.seed"] = np.array(seed)
            break
    else:
        raise SystemExit(f"no seed for {tag} met the fixture's conditions")
np.savez_compressed(OUT, **arrs)
print(os.path.getsize(OUT) / 1e6, "MB")
assert os.path.getsize(OUT) < 1e6
