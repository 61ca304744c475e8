"""TAP-Vid tracking evaluation timings -> profiles/bench_track.json (or the path given as the first argument).

DAVIS-sized synthetic workload: T = 64 frames of 464x848 at patch 16 / stride 8 (57 x 105 grid, pitch 106 after the refine conv),
D = 768, N = 256 queries.  Stage 1 (trajectories): every query embedding against every frame.  Stage 2 (anchors): every trajectory
sample against every anchor frame, ~50 % anchors per query.  Per precision: gd_track_points (fused), and the same stages in a torch
form on the GPU (a chunked per-frame matmul with the score map materialised, then relu / argmax / disc sums).  For the record, the
reference's einsum form (all T + 1 maps per call, one kept; restated here in torch) on a reduced shape, and one whole synthetic
video through gd_amd.evaluate.tapvid_video_metrics (forward included).  Median of 5 timed runs after 2 warm-ups."""
import hashlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gd_amd  # noqa: E402,F401
from gd_amd import _lib, ops  # noqa: E402
from gd_amd import evaluate as E  # noqa: E402
from bench import PEAK_TFLOPS  # noqa: E402

T, H, W, P, S, D, N, RADIUS = 64, 464, 848, 16, 8, 768, 256, 35
GEOM = E.track_geometry(H, W, P, S, pitch=106)
GH, GW, PITCH = GEOM[4:]


def timed(fn, warm=2, iters=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    t.sort()
    return {"median_ms": round(t[len(t) // 2], 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3)}


def torch_head(E_rows, fmap, frames, dtype, chunk=512):
    """The tracker head in torch, per target frame: S = E F^T materialised, cosine, relu, argmax, disc soft-argmax."""
    xy = torch.arange(GH * GW, device=fmap.device)
    cx = (xy % GW).float() * S + P // 2
    cy = (xy // GW).float() * S + P // 2
    Fv = fmap.view(T, GH, PITCH, D)[:, :, :GW].reshape(T, GH * GW, D)
    fn = Fv.norm(dim=-1)
    en = E_rows.norm(dim=-1)
    out = torch.empty(E_rows.shape[0], 2, device=fmap.device)
    for t in torch.unique(frames).tolist():
        idx = (frames == t).nonzero().reshape(-1)
        Ft = Fv[t].to(dtype)
        for i in range(0, len(idx), chunk):
            r = idx[i:i + chunk]
            c = (E_rows[r].to(dtype) @ Ft.T).float() / torch.clamp(en[r, None] * fn[t][None], min=1e-8)
            c = torch.relu(c)
            g = c.argmax(1)
            m = (cx[None] - cx[g][:, None]) ** 2 + (cy[None] - cy[g][:, None]) ** 2 <= RADIUS * RADIUS
            w = torch.exp(c) * m
            sw = w.sum(1)
            out[r] = torch.stack([(w * cx).sum(1) / sw, (w * cy).sum(1) / sw], 1)
    return out


def reference_einsum_form(emb, fmap_nchw, frames_set):
    """tracking_model.py:292-303 restated: every row's map against every frame of the set, one kept per row."""
    maps = torch.einsum("bc,nchw->bnhw", emb, fmap_nchw)
    return maps[torch.arange(emb.shape[0]), frames_set]


def main():
    torch.manual_seed(0)
    dev = "cuda"
    res = {"library_sha256_16": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16], "device": torch.cuda.get_device_name(0),
           "workload": {"T": T, "img": [H, W], "patch": P, "stride": S, "grid": [GH, GW], "pitch": PITCH, "D": D, "N": N, "radius": RADIUS}}
    fmap = torch.randn(T, GH * PITCH, D, device=dev)
    emb = torch.randn(N, D, device=dev)
    # stage 1: N rows per frame; stage 2: ~50 % anchors per query, every trajectory sample (T rows per query) against each
    f1 = torch.arange(T).repeat_interleave(N)
    rows1 = emb.repeat(T, 1)
    g = torch.Generator().manual_seed(1)
    anchors = torch.rand(N, T, generator=g) < 0.5
    nn_, aa = anchors.nonzero(as_tuple=True)
    f2 = aa[:, None].expand(-1, T).reshape(-1)
    samp = torch.randn(N * T, D, device=dev)
    rows2 = samp.view(N, T, D)[nn_.to(dev)].reshape(-1, D)
    stages = {"stage1": (rows1, f1), "stage2": (rows2, f2)}
    res["rows"] = {k: int(v[0].shape[0]) for k, v in stages.items()}
    res["anchor_fraction"] = round(float(anchors.float().mean()), 4)
    for prec in ("f16", "f32"):
        tf = ops.TrackFeatures(fmap, prec)
        peak = PEAK_TFLOPS["tf32h" if prec == "f16" else "f32"]
        for st, (rows, fr) in stages.items():
            order, tiles = ops.track_tiles(fr)
            ro = rows[order.to(dev)].contiguous()
            flop = 2.0 * ro.shape[0] * GH * PITCH * D
            r = timed(lambda: ops.track_points(ro, tf, geometry=GEOM, radius=RADIUS, precision=prec, tiles=tiles))
            r["tflops"] = round(flop / r["median_ms"] / 1e9, 1)
            r["frac_of_peak"] = round(r["tflops"] / peak, 4)
            res[f"fused_{prec}_{st}"] = r
            dt = torch.float16 if prec == "f16" else torch.float32
            frd = fr.to(dev)
            q = timed(lambda: torch_head(rows, fmap, frd, dt), warm=1, iters=3 if st == "stage2" else 5)
            q["speedup_fused"] = round(q["median_ms"] / r["median_ms"], 2)
            res[f"torch_{prec}_{st}"] = q
            print(st, prec, res[f"fused_{prec}_{st}"], res[f"torch_{prec}_{st}"], flush=True)
    # the reference's einsum form on a reduced shape (T = 8 frames, 16 queries), for the record
    Tr, Nr = 8, 16
    fm_r = fmap[:Tr].view(Tr, GH, PITCH, D)[:, :, :GW].permute(0, 3, 1, 2).contiguous()
    e_r = emb[:Nr]
    fs = torch.arange(Tr, device=dev).repeat_interleave(Nr)
    res["reference_einsum_reduced"] = dict(timed(lambda: reference_einsum_form(e_r.repeat(Tr, 1), fm_r, fs)), T=Tr, N=Nr,
                                           maps_computed=Tr * Nr * Tr, maps_kept=Tr * Nr)
    tfr = ops.TrackFeatures(fmap[:Tr].contiguous(), "f32")
    res["fused_f32_reduced"] = timed(lambda: ops.track_points(e_r.repeat(Tr, 1), tfr, frames=fs.cpu(), geometry=GEOM, radius=RADIUS,
                                                              precision="f32"))
    # one whole synthetic video: the tiny test ViT at 464x848 / stride 8, 16 frames, 32 queries, forward included
    from gd_amd.finetune import FinetuneGD
    eng = FinetuneGD(r=4, backbone="vit_tiny_test", patch_size=16, img_size=H, variant="vggt", geometry="shared", dtype="f32",
                     lora_b_std=0.05, vit_kwargs=dict(init_values=1.0), teacher_patch=16).cuda().eval()
    Tv = 16
    frames = torch.rand(Tv, 3, H, W, device=dev)
    q = torch.rand(32, 2, generator=g) * torch.tensor([W - 40.0, H - 40.0]) + 20
    cfg = {"video_idx": 0, "h": H, "w": W, "query_points": {0: q[:16].numpy(), 5: q[16:].numpy()},
           "target_points": {0: q[:16, None].expand(-1, Tv, -1).numpy(), 5: q[16:, None].expand(-1, Tv, -1).numpy()},
           "occluded": {0: torch.zeros(16, Tv, dtype=torch.bool).numpy(), 5: torch.zeros(16, Tv, dtype=torch.bool).numpy()}}
    walls = []
    for i in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            E.tapvid_video_metrics(eng, frames, cfg)
        except _lib.GdHipError as e:          # a random video may leave a query without anchors; timing is what is recorded
            res["video_note"] = str(e)[:120]
        torch.cuda.synchronize()
        if i >= 1:
            walls.append((time.perf_counter() - t0) * 1e3)
    walls.sort()
    res["video_wall_ms"] = {"median_ms": round(walls[1], 1), "frames": Tv, "queries": 32, "img": [H, W], "backbone": "vit_tiny_test"}
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_track.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
