"""Teacher block-stack timings on one GPU, VGGT and MASt3R (not the training benchmark: bench.py stays the yardstick of the step).

  python3 tools/bench_teacher.py [--out profiles/bench_teacher.json] [--iters 5] [--warm 2] [--depth 24] [--sections vggt,mast3r,heads,heads_share,mast3r_heads,mast3r_heads_share,tracker,tracker_share,updateformer,patch_embed,patch_embed_share,camera_head,camera_head_share,tokens_linear]

1. The aggregator's block stack at VGGT-1B size — width 1024, 16 heads, 24 frame + 24 global blocks, S = 2 views of P = 1374 tokens
   (518^2 at patch 14 + 5 prefix tokens), random weights, bf16: `VGGTTeacherRunner.aggregate` with fused_blocks (the HIP kernels,
   teacher_blocks.FusedAggregatorBlocks) against the same call on the torch modules under bf16 autocast with the q/k hooks (the default
   path).  Both include the aggregator's own pre-block part (patch embedding, tokens, position grid).  The modules are
   tests/test_teacher_runner_ref.AggregatorLayout: the aggregator's parameter names and call pattern, not the user's vggt package.
2. The fused block's kernels one by one at that size (time per call x calls per pair), and gd_qk_norm_rope's bytes per second against
   its algorithmic bytes — a read and a write of two thirds of qkv — at the pair's size (the tensor fits the Infinity Cache) and on
   a 64-pair tensor that does not.
3. "parity": the bf16 pair e_ref / e_hip of tests/test_gpu_teacher_blocks.py (max abs error against the fp64 run of the torch modules under
   autocast, and of the fused bf16 path), on fixture G22's weights and image.
4. "mast3r_block_stack": the MASt3R teacher's transformer at its size — ViT-L encoder 24 x 1024 / 16 heads, decoder 12 + 12 x 768 / 12 heads, two views
   of 768 tokens (24 x 32), B = 2 (the symmetrised pair), random weights: encoder blocks, `enc_norm`, decoder and target map through
   teacher_blocks.FusedCroCoBlocks (f32 and bf16) against the torch modules of tests/croco_layout.py (f32, and under bf16 autocast) in the same
   process, alternating.  "cross_attention_kernel": gd_cross_attention_fwd alone at (B, Nq, Nk, H) = (2, 768, 768, 12) per element type, from device
   events around 20 back-to-back calls, with the achieved TFLOP/s of its 4 B H Nq Nk 64 operations.  "parity" / "mast3r": the measured values of
   tests/test_gpu_mast3r_blocks.py (f32 stack against fixture G25 with the measured bound of the target map; the bf16 pair e_ref / e_hip).
5. "vggt_dpt_heads" (--sections heads): ONE dense-prediction head at VGGT-1B size — dim_in 2048, 256 features, out_channels [256, 512, 1024, 1024], two
   frames of 518^2, random weights: teacher_heads.FusedDPTHead (f32 and bf16 operands) against the torch module of tests/dpt_layout.py (f32, and
   under bf16 autocast) in the same process, alternating; the fused path's GEMM FLOP (counted by ops.GemmProfiler), its peak workspace (the
   allocator's peak above what was resident before the call) and the agreement of the f32 paths on the map before the activations.
   "vggt_dpt_heads_share_of_targets" (--sections heads_share): a VGGT-shaped random-weight teacher (the aggregator at --depth / --width with fused_blocks, depth and
   point heads, a track head whose feature extractor is a 128-feature head at down_ratio 2 around a stub tracker): the three heads' time, on the
   modules and fused, beside `aggregate` and the whole `targets()` call.
6. "mast3r_heads" (--sections mast3r_heads): ONE head of the MASt3R teacher at its size — encoder width 1024, decoder width 768, 256 features,
   last_dim 128, 24 descriptor channels, two_confs, two frames of 384 x 512 (a 24 x 32 token grid), random weights: teacher_heads.FusedMASt3RHead
   (f32 and bf16 operands) against the torch module of tests/mast3r_head_layout.py (f32, and under bf16 autocast), measured as section 5 is.
   "mast3r_heads_share" (--sections mast3r_heads_share): a MASt3R-shaped random-weight teacher (the transformer of section 4 with fused_blocks in
   bf16, a linear patch embedding, two such heads): `targets()` of one pair and the two heads alone, on the modules and with fused_heads (f32, bf16).
7. "vggt_tracker" (--sections tracker): the tracker tail at teacher size — a 259 x 259 x 128 feature map, S = 2 frames, N = 300 points, 7 pyramid levels, radius 4,
   4 iterations, hidden size 384, depth 6, random weights: the torch module of tests/tracker_layout.py as it stands (the position table rebuilt on the host in
   every iteration, as the reference does), the same with the table cached on the device, and teacher_tracker.FusedTracker (NCHW and channel-last input);
   gd_corr_sample alone with the bytes per second of the in-map window cells it gathers; the update transformer's share of the fused time.
   "vggt_tracker_share_of_targets" (--sections tracker_share): the teacher of heads_share with a real tracker behind the 128-feature head, fused_blocks
   and fused_heads on: `targets()` and the tracker call alone with fused_tracker off and on, and with fused_updateformer on top.
8. "vggt_updateformer" (--sections updateformer): the tracker's update transformer alone at teacher size — B = 1, N = 300 points + 64 virtual tracks, S = 2, hidden
   384, depth 6 + 6, 8 heads, random weights: the torch module of tests/tracker_layout.py against teacher_tracker.FusedUpdateFormer, alternating, each twice;
   the launches of one fused call; gd_attention_small_fwd alone for the four shapes it is called with (device events around 50 back-to-back calls); every GEMM
   of one fused call by shape, from device events around each launch; one LayerNorm over all rows.  "vggt_tracker" also times FusedTracker with
   fused_updateformer (alternating with the plain fused tracker).
9. "vggt_patch_embed" (--sections patch_embed): the aggregator's DINOv2 patch embedder alone at teacher size — ViT-L/14, 24 blocks of width 1024, 16 heads, 4
   registers, two frames of 518^2 (1374 tokens each), random weights: teacher_blocks.FusedDinoEmbed (f32 and bf16 operands) against the torch module of
   tests/dino_layout.py (f32, and under bf16 autocast), alternating, each path twice; the agreement of every path with the f32 module.
   "vggt_patch_embed_share" (--sections patch_embed_share): the teacher of tracker_share built around that embedder instead of the stub convolution, everything
   else fused: the embedder alone, `aggregate` and `targets()` with fused_patch_embed off and on.
10. "vggt_camera_head" (--sections camera_head): the camera head alone at teacher size — dim_in 2048, 4 trunk blocks, 16 heads (head dimension 128), B = 1,
   S = 2 camera rows, 4 iterations: teacher_heads.FusedCameraHead with fp32 and with bf16 weights against the torch module of tests/camera_layout.py in
   fp32 (as the reference runs it, outside autocast), alternating, each path twice; launches and weight bytes per call, the fused call's achieved TB/s; and
   gd_rows_linear alone at the head's five shapes (M = 2) against gd_gemm_nt on the same operands, interleaved, three rounds, every call on another copy
   of the weights (a pool above 512 MB, so that no call finds its weights in the 256 MB last-level cache — as in the head, which cycles through 864 MB),
   also as a fraction of the bandwidth gd_cost_volume_teacher_stats reaches on a stream of the same size.
   "vggt_camera_head_share" (--sections camera_head_share): the teacher of tracker_share with that camera head in place of the stub, every other switch
   fused, with fused_camera_head off and on: the head's time, targets(), and the head's share of it.
11. "tokens_linear" (--sections tokens_linear): gd_tokens_linear against gd_gemm_nt on the same operands, alternating in one run, each with its epilogue
   (+ bias, + residual), device events around 20 back-to-back calls (the new kernel through its C entry point, so that the host keeps ahead of it): the update transformer's products — M in {728, 600, 128} x (K, N) in {(384, 1152),
   (384, 768), (384, 384), (384, 1536), (1536, 384), (388, 384), (384, 132)} — and the tracker's own three at M = 600: microseconds, TFLOP/s and the ratio to
   the f32 MFMA floor 2 M N K / 157.3 TFLOP/s.  "vggt_updateformer" also times FusedUpdateFormer(linear="tokens") ("fused_tokens") with its launches and its
   per-kernel split; "vggt_tracker" and "vggt_tracker_share_of_targets" also run FusedTracker / the runner with the transformer fused on "tokens".
Prints one JSON object (also written to --out; sections that were not run keep what the file held)."""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import gd_amd  # noqa: E402,F401
from gd_amd import _lib, ops  # noqa: E402
from gd_amd.teacher_runner import VGGTTeacherRunner  # noqa: E402
from bench import PEAK_HBM_GBS, PEAK_TFLOPS  # noqa: E402
import croco_layout as CL  # noqa: E402
import test_gpu_mast3r_blocks as TM  # noqa: E402
import test_gpu_teacher_blocks as T  # noqa: E402
from test_teacher_runner_ref import AggregatorLayout  # noqa: E402

HBM_TBS = PEAK_HBM_GBS / 1000.0


def timed(fn, warm, iters, reps=1):
    """ms per call: device events around `reps` back-to-back calls (a kernel of a few microseconds needs several inside one window),
    `iters` windows after `warm` warm-up calls."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    singles = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        singles.append(e0.elapsed_time(e1) / reps)
    singles.sort()
    return {"median_ms": round(singles[len(singles) // 2], 4), "min_ms": round(singles[0], 4), "max_ms": round(singles[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--img", type=int, default=518)
    ap.add_argument("--sections", default="vggt,mast3r")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {}
    if a.out and os.path.exists(a.out):
        res = json.load(open(a.out))
    res.pop("library_sha256_16", None)          # (files of earlier runs: one hash for the whole file; it is kept per section now)
    res["device"] = torch.cuda.get_device_name(0)
    sections = a.sections.split(",")
    if "vggt" in sections:
        vggt_sections(res, a, dev)
    if "mast3r" in sections:
        mast3r_sections(res, a, dev)
    if "heads" in sections:
        dpt_head_section(res, a, dev)
    if "heads_share" in sections:
        dpt_share_section(res, a, dev)
    if "mast3r_heads" in sections:
        mast3r_head_section(res, a, dev)
    if "mast3r_heads_share" in sections:
        mast3r_share_section(res, a, dev)
    if "tracker" in sections:
        tracker_section(res, a, dev)
    if "tracker_share" in sections:
        tracker_share_section(res, a, dev)
    if "updateformer" in sections:
        updateformer_section(res, a, dev)
    if "patch_embed" in sections:
        patch_embed_section(res, a, dev)
    if "patch_embed_share" in sections:
        patch_embed_share_section(res, a, dev)
    if "camera_head" in sections:
        camera_head_section(res, a, dev)
    if "camera_head_share" in sections:
        camera_head_share_section(res, a, dev)
    if "tokens_linear" in sections:
        tokens_linear_section(res, a, dev)
    # every section that ran in this call carries the library it ran on; sections that were not run keep what the file held
    lib_hash = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    ran = {"vggt": ["block_stack", "fused_kernels_at_vggt_size", "qk_norm_rope_bandwidth"], "mast3r": ["mast3r_block_stack", "cross_attention_kernel"],
           "heads": ["vggt_dpt_heads"], "heads_share": ["vggt_dpt_heads_share_of_targets"], "mast3r_heads": ["mast3r_heads"],
           "mast3r_heads_share": ["mast3r_heads_share"], "tracker": ["vggt_tracker"], "tracker_share": ["vggt_tracker_share_of_targets"],
           "updateformer": ["vggt_updateformer"], "patch_embed": ["vggt_patch_embed"], "patch_embed_share": ["vggt_patch_embed_share"],
           "camera_head": ["vggt_camera_head"], "camera_head_share": ["vggt_camera_head_share"], "tokens_linear": ["tokens_linear"]}
    for sec in sections:
        for key in ran.get(sec, []):
            if key in res:
                res[key]["library_sha256_16"] = lib_hash
    txt = json.dumps(res)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


VGGT_HEAD = dict(dim_in=2048, features=256, out_channels=[256, 512, 1024, 1024])


def dpt_head_section(res, a, dev):
    import dpt_layout as DL
    from gd_amd.teacher_heads import FusedDPTHead
    S, P = 2, (a.img // 14) ** 2 + 5
    with torch.device(dev):
        m = DL.DPTLayout(output_dim=2, activation="exp", conf_activation="expp1", **VGGT_HEAD).eval()
    toks = [torch.randn(1, S, P, VGGT_HEAD["dim_in"], device=dev) for _ in range(4)]
    img = torch.rand(1, S, 3, (a.img // 14) * 14, (a.img // 14) * 14, device=dev)
    f32, bf = FusedDPTHead(m, dtype=torch.float32), FusedDPTHead(m, dtype=torch.bfloat16)

    def module_run(autocast, taps=None):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            return m(toks, img, 5, taps=taps)
    paths = {"fused_f32": lambda: f32.forward(toks, img, 5), "module_f32": lambda: module_run(False), "fused_bf16": lambda: bf.forward(toks, img, 5),
             "module_bf16_autocast": lambda: module_run(True)}
    out = dict(VGGT_HEAD, frames=S, image=list(img.shape[-2:]), patch_grid=[a.img // 14, a.img // 14])
    prof = ops.GemmProfiler()
    ops.set_gemm_profiler(prof)
    f32.forward(toks, img, 5)
    ops.set_gemm_profiler(None)
    flop, _, launches = prof.totals()
    out["fused_gemm_flop"], out["fused_gemm_launches"] = flop, launches
    for name in ("fused_f32", "fused_bf16", "module_f32", "module_bf16_autocast"):
        paths[name]()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        paths[name]()
        torch.cuda.synchronize()
        out[name + "_peak_workspace_MB"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    # each path twice, interleaved: other work shares the machine
    for name, fn in paths.items():
        out[name] = timed(fn, a.warm, a.iters)
    for name, fn in paths.items():
        out[name + "_again"] = timed(fn, 1, a.iters)
    best = lambda k: min(out[k]["median_ms"], out[k + "_again"]["median_ms"])
    out["speedup_fused_f32_vs_module_f32"] = round(best("module_f32") / best("fused_f32"), 3)
    out["speedup_fused_bf16_vs_module_bf16_autocast"] = round(best("module_bf16_autocast") / best("fused_bf16"), 3)
    out["fused_f32_tflops"] = round(flop / best("fused_f32") * 1e-9, 1)
    out["fused_bf16_tflops"] = round(flop / best("fused_bf16") * 1e-9, 1)
    tf, tm, tb, ta = {}, {}, {}, {}
    f32.forward(toks, img, 5, taps=tf), module_run(False, tm), bf.forward(toks, img, 5, taps=tb), module_run(True, ta)
    rel = lambda x, y: float((x.float() - y).abs().max() / y.abs().max())
    out["pre_activation_rel_diff_vs_module_f32"] = {"fused_f32": rel(tf["pre"], tm["pre"]), "fused_bf16": rel(tb["pre"], tm["pre"]),
                                                    "module_bf16_autocast": rel(ta["pre"], tm["pre"])}
    res["vggt_dpt_heads"] = out


def dpt_share_section(res, a, dev):
    import dpt_layout as DL
    C, S = a.width, 2
    idx = [a.depth // 6, a.depth // 2 - 1, 3 * a.depth // 4 - 1, a.depth - 1]          # [4, 11, 17, 23] at depth 24
    with torch.device(dev):
        agg = AggregatorLayout(img_size=a.img, patch_size=14, embed_dim=C, depth=a.depth, num_heads=C // 64, num_register_tokens=4,
                               attn_indices=[a.depth // 2, a.depth - 1], temperature=0.8).eval()
        head = lambda **kw: DL.DPTLayout(**dict(dict(VGGT_HEAD, dim_in=2 * C), intermediate_layer_idx=idx, **kw)).eval()
        track = DL.TinyTrackHead(2 * C)
        track.feature_extractor = head(features=128, feature_only=True, down_ratio=2)
        depth_head, point_head = head(output_dim=2, activation="exp"), head(output_dim=4, activation="inv_log")
    rope = T.DeviceRope2D()
    agg.rope = rope
    for b in list(agg.frame_blocks) + list(agg.global_blocks):
        b.attn.rope = rope
        torch.nn.init.constant_(b.ls1.gamma, 0.2)
        torch.nn.init.constant_(b.ls2.gamma, 0.2)
    teacher = type("Teacher", (), {"aggregator": agg, "depth_head": depth_head, "point_head": point_head,
                                   "track_head": track.eval(), "camera_head": lambda self, toks: [torch.zeros(1, 2, 9, device=dev)]})()
    img = torch.rand(1, S, 3, (a.img // 14) * 14, (a.img // 14) * 14, device=dev)
    out = {"width": C, "depth": a.depth, "intermediate_layer_idx": idx, "aggregator": "fused_blocks bf16", "track_feature_extractor": "128 features, down_ratio 2"}
    for tag, fused_heads in (("module_heads_f32", False), ("fused_heads_f32", True)):
        r = VGGTTeacherRunner(teacher, dtype=torch.bfloat16, pose_decoder=DL.tiny_pose_decoder, fused_blocks=True, fused_heads=fused_heads)
        toks, ps, _ = r.aggregate(img)
        hs = r.heads or {"depth_head": teacher.depth_head, "point_head": teacher.point_head, "track_head.feature_extractor": track.feature_extractor}

        def heads_run():
            with torch.no_grad():
                for h in hs.values():
                    h(toks, img, ps)
        got = r.targets(img)
        out[tag] = {"aggregate": timed(lambda: r.aggregate(img), 1, a.iters), "three_heads": timed(heads_run, a.warm, a.iters),
                    "targets": timed(lambda: r.targets(img), 1, a.iters), "targets_returned_none": got is None}
        out[tag]["heads_share_of_targets"] = round(out[tag]["three_heads"]["median_ms"] / out[tag]["targets"]["median_ms"], 3)
        del r
    res["vggt_dpt_heads_share_of_targets"] = out


TRACKER = dict(H=259, W=259, S=2, N=300, levels=7, radius=4, iters=4, hidden_size=384, depth=6)


def teacher_size_tracker(dev, **kw):
    import tracker_layout as TL
    with torch.device(dev):
        return TL.TrackerLayout(stride=2, corr_levels=TRACKER["levels"], corr_radius=TRACKER["radius"], hidden_size=TRACKER["hidden_size"],
                                depth=TRACKER["depth"], **kw).eval()


def tracker_section(res, a, dev):
    from gd_amd.teacher_tracker import FusedTracker
    t = TRACKER
    H, W, S, N, iters = t["H"], t["W"], t["S"], t["N"], t["iters"]
    trk = teacher_size_tracker(dev)
    cached = teacher_size_tracker(dev, cache_pos_embed=True)
    cached.load_state_dict(trk.state_dict())
    fused, fused_uf = FusedTracker(trk), FusedTracker(trk, fused_updateformer=True)
    fused_tok = FusedTracker(trk, fused_updateformer=True, linear="tokens")
    fmaps = torch.randn(1, S, 128, H, W, device=dev)
    cl = fmaps.permute(0, 1, 3, 4, 2).contiguous()
    q = torch.rand(1, N, 2, device=dev) * torch.tensor([2.0 * (W - 1), 2.0 * (H - 1)], device=dev)

    def module_run(m):
        with torch.no_grad():
            return m(q, fmaps, iters=iters)
    out = dict(t, updateformer="the torch module in every path but fused_updateformer*", dtype="float32")
    want, got = module_run(cached)[0][-1], fused(q, fmaps, iters=iters)[0][-1]
    out["fused_vs_module_final_coords_max_abs_px"] = float((want - got).abs().max())       # random unit-scale weights: the loop amplifies rounding
    # the host-built table costs seconds per call: fewer windows for that path
    out["module_host_table"] = timed(lambda: module_run(trk), 1, min(a.iters, 3))
    for name, fn in (("module_cached_table", lambda: module_run(cached)), ("fused", lambda: fused(q, fmaps, iters=iters)),
                     ("fused_channel_last", lambda: fused(q, iters=iters, fmaps_cl=cl)), ("fused_updateformer", lambda: fused_uf(q, fmaps, iters=iters)),
                     ("fused_updateformer_tokens", lambda: fused_tok(q, fmaps, iters=iters)),
                     ("fused_again", lambda: fused(q, fmaps, iters=iters)), ("fused_updateformer_again", lambda: fused_uf(q, fmaps, iters=iters)),
                     ("fused_updateformer_tokens_again", lambda: fused_tok(q, fmaps, iters=iters))):
        out[name] = timed(fn, a.warm, a.iters)
    out["fused_updateformer_tokens_vs_module_final_coords_max_abs_px"] = float((want - fused_tok(q, fmaps, iters=iters)[0][-1]).abs().max())
    out["speedup_fused_updateformer_tokens_vs_fused"] = round(min(out["fused"]["median_ms"], out["fused_again"]["median_ms"]) /
                                                              min(out["fused_updateformer_tokens"]["median_ms"], out["fused_updateformer_tokens_again"]["median_ms"]), 3)
    out["fused_updateformer_vs_module_final_coords_max_abs_px"] = float((want - fused_uf(q, fmaps, iters=iters)[0][-1]).abs().max())
    out["speedup_fused_updateformer_vs_fused"] = round(min(out["fused"]["median_ms"], out["fused_again"]["median_ms"]) /
                                                       min(out["fused_updateformer"]["median_ms"], out["fused_updateformer_again"]["median_ms"]), 3)
    st = fused.begin(q, fmaps)
    out["corr_sample"] = timed(lambda: ops.corr_sample(st.pyramid, st.feats, st.coords, fused.radius, ld=fused.kpad), a.warm, a.iters, reps=20)
    cells = 0                                   # the in-map cells of every (2r+2)^2 window: what the kernel's dot products read (512 B each)
    for l, (_m, h, w, _p) in enumerate(st.pyramid):
        c0 = (st.coords / 2 ** l).floor().long() - fused.radius
        k = torch.arange(2 * fused.radius + 2, device=dev)
        nx = ((c0[..., 0:1] + k >= 0) & (c0[..., 0:1] + k < w)).sum(-1)
        ny = ((c0[..., 1:2] + k >= 0) & (c0[..., 1:2] + k < h)).sum(-1)
        cells += int((nx * ny).sum())
    out["corr_sample"]["gathered_MB"] = round(cells * 512 / 1e6, 1)
    out["corr_sample"]["gathered_GBps"] = round(cells * 512 / 1e9 / (out["corr_sample"]["median_ms"] * 1e-3), 1)
    x = torch.randn(1, N, S, fused.D, device=dev)

    def former():
        with torch.no_grad():
            trk.updateformer(x)
    out["updateformer_one_call"] = timed(former, a.warm, a.iters)
    out["updateformer_share_of_fused"] = round(iters * out["updateformer_one_call"]["median_ms"] / out["fused"]["median_ms"], 3)
    res["vggt_tracker"] = out


def vggt_shaped_teacher(a, dev, make_aggregator=AggregatorLayout, **agg_kw):
    """-> (teacher, track head, image pair): the aggregator at --depth / --width, depth and point heads, and a track head with a 128-feature extractor at
    down_ratio 2 around a teacher-size tracker, random weights."""
    import dpt_layout as DL
    import tracker_layout as TL
    C, S = a.width, 2
    idx = [a.depth // 6, a.depth // 2 - 1, 3 * a.depth // 4 - 1, a.depth - 1]
    with torch.device(dev):
        agg = make_aggregator(img_size=a.img, patch_size=14, embed_dim=C, depth=a.depth, num_heads=C // 64, num_register_tokens=4,
                              attn_indices=[a.depth // 2, a.depth - 1], temperature=0.8, **agg_kw).eval()
        head = lambda **kw: DL.DPTLayout(**dict(dict(VGGT_HEAD, dim_in=2 * C), intermediate_layer_idx=idx, **kw)).eval()
        track = TL.TrackHeadLayout(2 * C, levels=TRACKER["levels"], iters=TRACKER["iters"])
        track.feature_extractor = head(features=128, feature_only=True, down_ratio=2)
        depth_head, point_head = head(output_dim=2, activation="exp"), head(output_dim=4, activation="inv_log")
    track.tracker = teacher_size_tracker(dev)
    rope = T.DeviceRope2D()
    agg.rope = rope
    for b in list(agg.frame_blocks) + list(agg.global_blocks):
        b.attn.rope = rope
        torch.nn.init.constant_(b.ls1.gamma, 0.2)
        torch.nn.init.constant_(b.ls2.gamma, 0.2)
    teacher = type("Teacher", (), {"aggregator": agg, "depth_head": depth_head, "point_head": point_head,
                                   "track_head": track.eval(), "camera_head": lambda self, toks: [torch.zeros(1, 2, 9, device=dev)]})()
    img = torch.rand(1, S, 3, (a.img // 14) * 14, (a.img // 14) * 14, device=dev)
    return teacher, track, img


def tracker_share_section(res, a, dev):
    import dpt_layout as DL
    C = a.width
    teacher, track, img = vggt_shaped_teacher(a, dev)
    out = dict(TRACKER, width=C, depth=a.depth, aggregator="fused_blocks bf16", heads="fused_heads f32")
    for tag, on, uf, lin in (("module_tracker", False, False, "gemm_nt"), ("fused_tracker", True, False, "gemm_nt"),
                             ("fused_tracker_fused_updateformer", True, True, "gemm_nt"), ("fused_tracker_fused_updateformer_tokens", True, True, "tokens"),
                             ("fused_tracker_again", True, False, "gemm_nt")):
        r = VGGTTeacherRunner(teacher, dtype=torch.bfloat16, pose_decoder=DL.tiny_pose_decoder, fused_blocks=True, fused_heads=True, fused_tracker=on,
                              fused_updateformer=uf, tracker_linear=lin)
        toks, ps, _ = r.aggregate(img)
        fm, pitch = r.heads["track_head.feature_extractor"](toks, img, ps, channel_last=True)
        nchw = fm.permute(0, 1, 4, 2, 3)
        q = torch.rand(1, TRACKER["N"], 2, device=dev) * (img.shape[-1] - 1)

        def tracker_run():
            with torch.no_grad():
                return r.tracker(q, iters=track.iters, fmaps_cl=fm, pitch=pitch) if on else track.tracker(query_points=q, fmaps=nchw, iters=track.iters)
        got = r.targets(img)
        out[tag] = {"tracker": timed(tracker_run, 1, min(a.iters, 3)), "targets": timed(lambda: r.targets(img), 1, min(a.iters, 3)),
                    "targets_returned_none": got is None, "keypoints": 0 if got is None else int(got["kp_1"].shape[0])}
        out[tag]["tracker_share_of_targets"] = round(out[tag]["tracker"]["median_ms"] / out[tag]["targets"]["median_ms"], 3)
        del r
    res["vggt_tracker_share_of_targets"] = out


DINO = dict(patch_size=14, embed_dim=1024, depth=24, num_heads=16, num_register_tokens=4)          # dinov2_vitl14_reg


def dino_at_teacher_size(a, dev):
    import dino_layout as DY
    with torch.device(dev):
        m = DY.DinoLayout(img_size=a.img, **DINO).eval()
    for b in m.blocks:                              # random weights: LayerScale below 1 keeps 24 blocks' residual stream in range
        torch.nn.init.constant_(b.ls1.gamma, 0.2)
        torch.nn.init.constant_(b.ls2.gamma, 0.2)
    torch.nn.init.normal_(m.pos_embed, std=0.02)
    return m


def patch_embed_section(res, a, dev):
    """The DINOv2 patch embedder alone at teacher size: teacher_blocks.FusedDinoEmbed (f32 and bf16 operands) against the torch module of
    tests/dino_layout.py (f32, and under bf16 autocast; its attention is F.scaled_dot_product_attention), alternating, each path twice."""
    from gd_amd.teacher_blocks import FusedDinoEmbed
    m = dino_at_teacher_size(a, dev)
    side = (a.img // 14) * 14
    img = torch.randn(2, 3, side, side, device=dev)
    f32, b16 = FusedDinoEmbed(m, dtype=torch.float32), FusedDinoEmbed(m, dtype=torch.bfloat16)

    def module(autocast, sdpa=True):
        for b in m.blocks:
            b.attn.sdpa = sdpa
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            return m(img)
    Nt = 1 + DINO["num_register_tokens"] + (side // 14) ** 2
    D, L = DINO["embed_dim"], DINO["depth"]
    out = dict(DINO, img=side, frames=2, tokens_per_frame=Nt,
               counted_TFLOP=round(2 * L * (2 * Nt * 12 * D * D + 4 * Nt * Nt * D) / 1e12, 3))          # 12 D^2 per token in the four GEMMs, 4 N D in attention
    want = module(False, sdpa=False)
    for k in ("x_prenorm", "x_norm_patchtokens"):
        out[f"max_abs_{k}"] = {"scale": float(want[k].abs().max()), "fused_f32": T.max_abs(f32.forward(img)[k], want[k]),
                               "fused_bf16": T.max_abs(b16.forward(img)[k], want[k]), "module_autocast_bf16": T.max_abs(module(True)[k], want[k])}
    # module_*: attention through F.scaled_dot_product_attention; module_explicit_*: the [B, H, N, N] softmax the reference forms without xformers
    paths = (("module_f32", lambda: module(False)), ("fused_f32", lambda: f32.forward(img)), ("module_autocast_bf16", lambda: module(True)),
             ("fused_bf16", lambda: b16.forward(img)), ("module_explicit_f32", lambda: module(False, sdpa=False)),
             ("module_explicit_autocast_bf16", lambda: module(True, sdpa=False)))
    for suffix in ("", "_again"):
        for name, fn in paths:
            out[name + suffix] = timed(fn, a.warm, a.iters)
    best = lambda n: min(out[n]["median_ms"], out[n + "_again"]["median_ms"])
    out["speedup_fused_f32_vs_module_f32"] = round(best("module_f32") / best("fused_f32"), 3)
    out["speedup_fused_bf16_vs_module_autocast_bf16"] = round(best("module_autocast_bf16") / best("fused_bf16"), 3)
    out["speedup_fused_bf16_vs_module_explicit_autocast_bf16"] = round(best("module_explicit_autocast_bf16") / best("fused_bf16"), 3)
    out["fused_bf16_TFLOPs"] = round(out["counted_TFLOP"] / (best("fused_bf16") * 1e-3), 1)
    res["vggt_patch_embed"] = out


def patch_embed_share_section(res, a, dev):
    """The embedder's share of `aggregate` and of `targets()`: the VGGT-shaped teacher of tracker_share built around the DINO embedder instead of the
    stub convolution, fused_blocks / fused_heads / fused_tracker on, with fused_patch_embed off and on."""
    import dino_layout as DY
    import dpt_layout as DL
    teacher, track, img = vggt_shaped_teacher(a, dev, DY.DinoAggregatorLayout, dino_depth=DINO["depth"], dino_heads=DINO["num_heads"])
    emb = teacher.aggregator.patch_embed
    for b in emb.blocks:
        b.attn.sdpa = True
        torch.nn.init.constant_(b.ls1.gamma, 0.2)
        torch.nn.init.constant_(b.ls2.gamma, 0.2)
    torch.nn.init.normal_(emb.pos_embed, std=0.02)
    out = dict(width=a.width, depth=a.depth, embedder=DINO, aggregator="fused_blocks bf16", heads="fused_heads f32", tracker="fused_tracker")
    frames = ((img - teacher.aggregator._resnet_mean) / teacher.aggregator._resnet_std)[0]
    for tag, on in (("module_patch_embed", False), ("fused_patch_embed", True)):
        r = VGGTTeacherRunner(teacher, dtype=torch.bfloat16, pose_decoder=DL.tiny_pose_decoder, fused_blocks=True, fused_heads=True, fused_tracker=True,
                              fused_patch_embed=on)

        def embed_run():
            if on:
                return r.embed.forward(frames)
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                return emb(frames)
        got = r.targets(img)
        out[tag] = {"patch_embed": timed(embed_run, a.warm, a.iters), "aggregate": timed(lambda: r.aggregate(img), 1, a.iters),
                    "targets": timed(lambda: r.targets(img), 1, min(a.iters, 3)), "targets_returned_none": got is None}
        out[tag]["patch_embed_share_of_aggregate"] = round(out[tag]["patch_embed"]["median_ms"] / out[tag]["aggregate"]["median_ms"], 3)
        out[tag]["patch_embed_share_of_targets"] = round(out[tag]["patch_embed"]["median_ms"] / out[tag]["targets"]["median_ms"], 3)
        del r
    out["speedup_aggregate"] = round(out["module_patch_embed"]["aggregate"]["median_ms"] / out["fused_patch_embed"]["aggregate"]["median_ms"], 3)
    out["speedup_targets"] = round(out["module_patch_embed"]["targets"]["median_ms"] / out["fused_patch_embed"]["targets"]["median_ms"], 3)
    res["vggt_patch_embed_share"] = out


CAMERA = dict(dim_in=2048, trunk_depth=4, num_heads=16)
CAMERA_SHAPES = [(2048, 6144), (2048, 2048), (2048, 8192), (8192, 2048), (2048, 1024)]          # (K, N): qkv / modulation, proj, fc1, fc2, pose_branch.fc1


def camera_head_at_teacher_size(dev, dim_in=CAMERA["dim_in"]):
    """The layout's camera head with torch's default initialisation, the pose branch conditioned as tests/camera_layout.fill_head does (a unit
    quaternion part and fields of view inside (0, pi) in every iteration), LayerScale and the empty pose token away from their zero-ish defaults."""
    import camera_layout as CAM
    with torch.device(dev):
        m = CAM.CameraHeadLayout(**dict(CAMERA, dim_in=dim_in)).eval()
    with torch.no_grad():
        for b in m.trunk:
            torch.nn.init.constant_(b.ls1.gamma, 0.2)
            torch.nn.init.constant_(b.ls2.gamma, 0.2)
        torch.nn.init.normal_(m.empty_pose_tokens, std=0.5)
        m.pose_branch.fc2.weight.mul_(0.1)
        m.pose_branch.fc2.bias[6] += 1.0
        m.pose_branch.fc2.bias[7:] += 0.4
    return m


def camera_head_section(res, a, dev):
    from gd_amd.teacher_heads import FusedCameraHead
    m = camera_head_at_teacher_size(dev)
    D, S, iters = CAMERA["dim_in"], 2, 4
    toks = [torch.randn(1, S, 1 + 4 + 37 * 37, D, device=dev)]
    f32, b16 = FusedCameraHead(m, dtype=torch.float32), FusedCameraHead(m, dtype=torch.bfloat16)

    def module():
        with torch.no_grad():
            return m(toks)
    want = module()[-1]
    out = dict(CAMERA, B=1, S=S, iterations=iters, max_abs_last_encoding={"scale": float(want.abs().max()), "fused_f32": T.max_abs(f32.forward(toks)[-1], want),
                                                                          "fused_bf16_weights": T.max_abs(b16.forward(toks)[-1], want)})
    for f, tag in ((f32, "fused_f32"), (b16, "fused_bf16_weights")):
        f.launches = 0
        f.forward(toks)
        out[f"launches_per_call_{tag}"] = f.launches
        out[f"weight_bytes_per_call_{tag}"] = f.weight_bytes * iters
    # the module's launches, counted as the aten operators one forward dispatches that are not views (each is at least one kernel)
    from torch.utils._python_dispatch import TorchDispatchMode
    views = ("view", "reshape", "permute", "transpose", "expand", "unbind", "chunk", "split", "select", "slice", "detach", "squeeze", "alias", "aten.t.")

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            Count.n += not any(v in str(func) for v in views)
            return func(*args, **(kwargs or {}))
    with Count():
        module()
    out["launches_per_call_module_f32"] = int(Count.n)
    paths = (("module_f32", module), ("fused_f32", lambda: f32.forward(toks)), ("fused_bf16_weights", lambda: b16.forward(toks)))
    for suffix in ("", "_again"):
        for name, fn in paths:
            out[name + suffix] = timed(fn, a.warm, a.iters)
    best = lambda n: min(out[n]["median_ms"], out[n + "_again"]["median_ms"])
    for tag in ("fused_f32", "fused_bf16_weights"):
        out[f"speedup_{tag}_vs_module_f32"] = round(best("module_f32") / best(tag), 3)
        out[f"achieved_TBs_{tag}"] = round(out[f"weight_bytes_per_call_{tag}"] / (best(tag) * 1e-3) / 1e12, 3)
        out[f"fraction_of_peak_HBM_{tag}"] = round(out[f"achieved_TBs_{tag}"] / HBM_TBS, 3)
    del f32, b16, m
    torch.cuda.empty_cache()
    # gd_rows_linear alone against gd_gemm_nt, M = 2, interleaved, three rounds; every call streams another copy of the weights
    shapes = {}
    for K, N in CAMERA_SHAPES:
        nbytes = N * K * 4
        copies = max(3, -(-(512 << 20) // nbytes))
        pool = [torch.randn(N, K, device=dev) * K ** -0.5 for _ in range(copies)]
        x, bias = torch.randn(2, K, device=dev), torch.randn(N, device=dev)
        y = torch.empty(2, N, device=dev)
        hw = 1024
        P = max(1, round(nbytes / (2 * hw * hw * 4)))
        maps = [(torch.rand(P, hw, hw, device=dev), torch.rand(P, hw, hw, device=dev)) for _ in range(max(3, -(-(512 << 20) // (2 * P * hw * hw * 4))))]
        L, st = _lib.lib(), _lib.stream()
        rl_args = [(x.data_ptr(), w.data_ptr(), _lib.F32, y.data_ptr(), 2, N, K, K, K, N, bias.data_ptr(), None, 0, None, 0, 0, st) for w in pool]
        tstats = torch.empty(P, 2, hw, 4, device=dev)
        ts_args = [(t1.data_ptr(), t2.data_ptr(), P, hw, hw, tstats.data_ptr(), st) for t1, t2 in maps]
        assert L.gd_rows_linear(*rl_args[0]) == 0 and L.gd_cost_volume_teacher_stats(*ts_args[0]) == 0
        state = {"i": 0}

        def nxt(lst):
            state["i"] = (state["i"] + 1) % len(lst)
            return lst[state["i"]]
        entry = {"K": K, "N": N, "weight_MB": round(nbytes / 2 ** 20, 1), "weight_copies": copies, "stream_MB": round(2 * P * hw * hw * 4 / 2 ** 20, 1), "rounds": []}
        for _ in range(3):
            # the two streaming kernels run 10 to 20 us: they are called at the C ABI with prepared arguments (as FusedCameraHead calls them), the
            # tensor wrappers' checks alone cost about as much on the host; gd_gemm_nt goes through its wrapper
            r = {"rows_linear": timed(lambda: L.gd_rows_linear(*nxt(rl_args)), a.warm, a.iters, reps=copies),
                 "gemm_nt": timed(lambda: ops.gemm_nt(x, nxt(pool), out=y, bias=bias), a.warm, a.iters, reps=copies),
                 "teacher_stats_stream": timed(lambda: L.gd_cost_volume_teacher_stats(*nxt(ts_args)), a.warm, a.iters, reps=len(maps))}
            entry["rounds"].append(r)
        med = lambda k: sorted(r[k]["median_ms"] for r in entry["rounds"])
        rl, gm, ts = med("rows_linear"), med("gemm_nt"), med("teacher_stats_stream")
        entry["rows_linear_ms"], entry["gemm_nt_ms"] = rl, gm
        entry["faster_beyond_the_spread"] = bool(rl[-1] < gm[0])                # the slowest rows_linear round against the fastest gemm_nt round
        entry["speedup_vs_gemm_nt"] = round(gm[1] / rl[1], 2)
        entry["rows_linear_TBs"] = round(nbytes / (rl[1] * 1e-3) / 1e12, 3)
        entry["teacher_stats_TBs"] = round(2 * P * hw * hw * 4 / (ts[1] * 1e-3) / 1e12, 3)
        entry["fraction_of_teacher_stats_bandwidth"] = round(entry["rows_linear_TBs"] / entry["teacher_stats_TBs"], 3)
        shapes[f"{K}->{N}"] = entry
        del pool, maps
        torch.cuda.empty_cache()
    out["rows_linear_M2"] = shapes
    res["vggt_camera_head"] = out


def camera_head_share_section(res, a, dev):
    """The camera head's share of `targets()`: the VGGT-shaped teacher of tracker_share with a real camera head, every other switch fused (patch
    embedder excepted: that teacher has the stub convolution), with fused_camera_head off and on."""
    import camera_layout as CAM
    teacher, track, img = vggt_shaped_teacher(a, dev)
    head = camera_head_at_teacher_size(dev, 2 * a.width)
    teacher.camera_head = head
    out = dict(CAMERA, dim_in=2 * a.width, width=a.width, depth=a.depth, aggregator="fused_blocks bf16", heads="fused_heads f32",
               tracker="fused_tracker + fused_updateformer")
    for tag, on in (("module_camera_head", False), ("fused_camera_head", True)):
        r = VGGTTeacherRunner(teacher, dtype=torch.bfloat16, pose_decoder=None if on else CAM.decode_pose, fused_blocks=True, fused_heads=True,
                              fused_updateformer=True, fused_camera_head=on, fused_tracker=True)
        toks, _, _ = r.aggregate(img)
        got = r.targets(img)
        out[tag] = {"cameras": timed(lambda: r.cameras(toks, img.shape[-2:]), a.warm, a.iters), "targets": timed(lambda: r.targets(img), 1, min(a.iters, 3)),
                    "targets_returned_none": got is None, "keypoints": 0 if got is None else int(got["kp_1"].shape[0]), "token_dtype": str(toks[-1].dtype)}
        out[tag]["camera_share_of_targets"] = round(out[tag]["cameras"]["median_ms"] / out[tag]["targets"]["median_ms"], 3)
        del r
    out["speedup_cameras"] = round(out["module_camera_head"]["cameras"]["median_ms"] / out["fused_camera_head"]["cameras"]["median_ms"], 3)
    out["speedup_targets"] = round(out["module_camera_head"]["targets"]["median_ms"] / out["fused_camera_head"]["targets"]["median_ms"], 3)
    res["vggt_camera_head_share"] = out


def updateformer_section(res, a, dev):
    """The tracker's update transformer alone at teacher size with random weights: the user's module against FusedUpdateFormer (alternating, each
    twice), gd_attention_small_fwd alone for the four shapes the transformer calls it with, and the per-kernel split of one fused call."""
    import tracker_layout as TL
    from gd_amd.teacher_tracker import FusedUpdateFormer
    t = TRACKER
    S, N, D, depth, H = t["S"], t["N"], t["hidden_size"], t["depth"], 8
    with torch.device(dev):
        m = TL.UpdateFormerLayout(depth, depth, 3 * 128 + 4, D, 130, num_heads=H).eval()
    fused, fused_tok = FusedUpdateFormer(m), FusedUpdateFormer(m, linear="tokens")
    x = torch.randn(1, N, S, 388, device=dev)

    def module_run():
        with torch.no_grad():
            return m(x)[0]
    out = dict(B=1, N=N, S=S, hidden=D, depth=depth, heads=H, virtual_tracks=fused.nv, dtype="float32")
    want, got = module_run(), fused(x)[0]
    out["max_abs_diff_vs_module"], out["max_abs_module"] = float((want - got).abs().max()), float(want.abs().max())
    out["launches_per_call"] = fused.launches
    out["fused_tokens_max_abs_diff_vs_module"] = float((want - fused_tok(x)[0]).abs().max())
    out["fused_tokens_launches_per_call"] = fused_tok.launches
    paths = {"module": module_run, "fused": lambda: fused(x), "fused_tokens": lambda: fused_tok(x)}
    for name, fn in paths.items():
        out[name] = timed(fn, a.warm, a.iters)
    for name, fn in paths.items():
        out[name + "_again"] = timed(fn, 1, a.iters)
    best = lambda k: min(out[k]["median_ms"], out[k + "_again"]["median_ms"])
    out["speedup_fused_vs_module"] = round(best("module") / best("fused"), 3)
    out["speedup_fused_tokens_vs_module"] = round(best("module") / best("fused_tokens"), 3)
    # the attention kernel alone, on the views the transformer hands it
    n, nv = N + fused.nv, fused.nv
    qkv, q1, kv = torch.randn(n * S, 3 * D, device=dev), torch.randn(n * S, D, device=dev), torch.randn(n * S, 2 * D, device=dev)
    o = torch.empty(n * S, D, device=dev)
    view = lambda tns, c0, r0, G0, G1, L, a0, a1, al: torch.as_strided(tns, (G0, G1, L, D), (a0 * tns.stride(0), a1 * tns.stride(0), al * tns.stride(0), 1),
                                                                      r0 * tns.stride(0) + c0)
    shapes = {
        "time": ((qkv, 0, 0, n, 1, S, S, 0, 1), (qkv, D, 0, n, 1, S, S, 0, 1), (qkv, 2 * D, 0, n, 1, S, S, 0, 1), (o, 0, 0, n, 1, S, S, 0, 1)),
        "virtual2point": ((q1, 0, N * S, 1, S, nv, 0, 1, S), (kv, 0, 0, 1, S, N, 0, 1, S), (kv, D, 0, 1, S, N, 0, 1, S), (o, 0, N * S, 1, S, nv, 0, 1, S)),
        "virtual": ((qkv, 0, N * S, 1, S, nv, 0, 1, S), (qkv, D, N * S, 1, S, nv, 0, 1, S), (qkv, 2 * D, N * S, 1, S, nv, 0, 1, S), (o, 0, N * S, 1, S, nv, 0, 1, S)),
        "point2virtual": ((q1, 0, 0, 1, S, N, 0, 1, S), (kv, 0, N * S, 1, S, nv, 0, 1, S), (kv, D, N * S, 1, S, nv, 0, 1, S), (o, 0, 0, 1, S, N, 0, 1, S)),
    }
    out["attention_small"] = {}
    for name, (aq, ak, av, ao) in shapes.items():
        vq, vk, vv, vo = view(*aq), view(*ak), view(*av), view(*ao)
        G0, G1, Lq, Lk = vq.shape[0], vq.shape[1], vq.shape[2], vk.shape[2]
        r = timed(lambda: ops.attention_small_fwd(vq, vk, vv, G0, G1, Lq, Lk, H, out=vo), a.warm, a.iters, reps=50)
        r.update(G0=G0, G1=G1, Nq=Lq, Nk=Lk, calls_per_transformer=depth, flop=4 * G0 * G1 * Lq * Lk * D)
        out["attention_small"][name] = r
    out["attention_small_us_per_transformer_call"] = round(sum(v["median_ms"] * depth for v in out["attention_small"].values()) * 1e3, 1)
    # the per-kernel split of one fused call: device events around every GEMM (ops.GemmProfiler), LayerNorm and attention by their own timing
    # (ops.tokens_linear honours the same profiler; its records' epilogue tags start with "t")
    for key, f in (("fused_gemm", fused), ("fused_tokens_linear", fused_tok)):
        prof = ops.GemmProfiler()
        ops.set_gemm_profiler(prof)
        f(x)
        ops.set_gemm_profiler(None)
        torch.cuda.synchronize()
        flop, _, launches = prof.totals()
        by = {}
        for e0, e1, fl, tag in prof.records:
            k = f"M={tag[0]} N={tag[1]} K={tag[2]} {tag[4]}"
            d = by.setdefault(k, {"calls": 0, "ms": 0.0})
            d["calls"] += 1
            d["ms"] = round(d["ms"] + e0.elapsed_time(e1), 4)
        out[key] = {"flop": flop, "launches": launches, "event_ms_total": round(sum(d["ms"] for d in by.values()), 3), "by_shape": by}
    xn = torch.randn(n * S, D, device=dev)
    g, b = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    out["layernorm_all_rows"] = timed(lambda: ops.layernorm_fwd(xn, g, b, 1e-5, save_stats=False), a.warm, a.iters, reps=50)
    res["vggt_updateformer"] = out


F32_MFMA_TFLOPS = 157.3          # the f32 MFMA peak of one MI355X: 256 CUs x 256 FLOP / clk x 2.4 GHz


def tokens_linear_section(res, a, dev):
    """gd_tokens_linear against gd_gemm_nt, alternating, on the update transformer's products and the tracker's own (each with + bias, + residual)."""
    from gd_amd.teacher_tracker import FusedTracker
    trk =FusedTracker(teacher_size_tracker(dev))
    kpad, hidden = trk.kpad, trk.corr_mlp[0].shape[0]
    shapes = [(M, K, N, "updateformer") for M in (728, 600, 128) for K, N in ((384, 1152), (384, 768), (384, 384), (384, 1536), (1536, 384), (388, 384), (384, 132))]
    shapes += [(600, kpad, hidden, "corr_mlp.fc1"), (600, hidden, 128, "corr_mlp.fc2"), (600, 128, 128, "ffeat_updater")]
    out = {"reps_per_window": 20, "epilogue": "+ bias + residual", "mfma_floor_tflops": F32_MFMA_TFLOPS, "shapes": {}}
    for M, K, N, what in shapes:
        x, w, b, r = torch.randn(M, K, device=dev), torch.randn(N, K, device=dev), torch.randn(N, device=dev), torch.randn(M, N, device=dev)
        y1, y2 = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
        # the new kernel through the C entry point: the Python of ops.tokens_linear (16 us per call) costs more than the kernel; gd_gemm_nt's launches
        # take longer than its wrapper
        targs = (_lib.ptr(x), _lib.ptr(w), _lib.ptr(y1), M, N, K, K, K, N, _lib.ptr(b), 0, _lib.ptr(r), N, 0, _lib.stream())
        fns = {"tokens_linear": lambda: _lib.lib().gd_tokens_linear(*targs), "gemm_nt": lambda: ops.gemm_nt(x, w, y2, bias=b, residual=r)}
        e = {"what": what, "max_abs_diff": float((ops.tokens_linear(x, w, b, out=y1, residual=r) - fns["gemm_nt"]()).abs().max())}
        t = {k: [] for k in fns}
        for _ in range(3):                                                         # alternating: three rounds of each
            for k, fn in fns.items():
                t[k].append(timed(fn, a.warm, a.iters, reps=20)["median_ms"])
        floor_us = 2.0 * M * N * K / (F32_MFMA_TFLOPS * 1e12) * 1e6
        for k in fns:
            us = min(t[k]) * 1e3
            e[k] = {"us": round(us, 2), "tflops": round(2.0 * M * N * K / us / 1e6, 2), "over_mfma_floor": round(us / floor_us, 2)}
        e["mfma_floor_us"] = round(floor_us, 2)
        e["speedup_vs_gemm_nt"] = round(e["gemm_nt"]["us"] / e["tokens_linear"]["us"], 2)
        out["shapes"][f"M={M} K={K} N={N}"] = e
    res["tokens_linear"] = out


MAST3R_HEAD = dict(enc_dim=1024, dec_dim=768, feature_dim=256, last_dim=128, local_feat_dim=24, two_confs=True)
MAST3R_IMG = (384, 512)


def mast3r_head_section(res, a, dev):
    import mast3r_head_layout as ML
    from gd_amd.teacher_heads import FusedMASt3RHead
    B, (H, W) = 2, MAST3R_IMG
    N = (H // 16) * (W // 16)
    with torch.device(dev):
        m = ML.MASt3RHeadLayout(**MAST3R_HEAD).eval()
    decout = [torch.randn(B, N, MAST3R_HEAD["enc_dim"] if i == 0 else MAST3R_HEAD["dec_dim"], device=dev) for i in range(ML.DEC_DEPTH + 1)]
    f32, bf = FusedMASt3RHead(m, dtype=torch.float32), FusedMASt3RHead(m, dtype=torch.bfloat16)

    def module_run(autocast, taps=None):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            return m(decout, (H, W), taps=taps)
    paths = {"fused_f32": lambda: f32(decout, (H, W)), "module_f32": lambda: module_run(False), "fused_bf16": lambda: bf(decout, (H, W)),
             "module_bf16_autocast": lambda: module_run(True)}
    out = dict(MAST3R_HEAD, frames=B, image=[H, W], patch_grid=[H // 16, W // 16], hooks=ML.HOOKS, layer_dims=list(ML.LAYER_DIMS))
    prof = ops.GemmProfiler()
    ops.set_gemm_profiler(prof)
    f32(decout, (H, W))
    ops.set_gemm_profiler(None)
    flop, _, launches = prof.totals()
    mlp = prof.totals(keep=lambda tag: tag[1] in (m.head_local_features.fc1.out_features, m.head_local_features.fc2.out_features) and tag[0] == B * N)[0]
    out["fused_gemm_flop"], out["fused_gemm_launches"], out["fused_gemm_flop_mlp"] = flop, launches, mlp
    for name in ("fused_f32", "fused_bf16", "module_f32", "module_bf16_autocast"):
        paths[name]()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        paths[name]()
        torch.cuda.synchronize()
        out[name + "_peak_workspace_MB"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    # each path twice, interleaved: other work shares the machine
    for name, fn in paths.items():
        out[name] = timed(fn, a.warm, a.iters)
    for name, fn in paths.items():
        out[name + "_again"] = timed(fn, 1, a.iters)
    best = lambda k: min(out[k]["median_ms"], out[k + "_again"]["median_ms"])
    out["speedup_fused_f32_vs_module_f32"] = round(best("module_f32") / best("fused_f32"), 3)
    out["speedup_fused_bf16_vs_module_bf16_autocast"] = round(best("module_bf16_autocast") / best("fused_bf16"), 3)
    out["fused_f32_tflops"] = round(flop / best("fused_f32") * 1e-9, 1)
    out["fused_bf16_tflops"] = round(flop / best("fused_bf16") * 1e-9, 1)
    tf, tm, tb, ta = {}, {}, {}, {}
    f32(decout, (H, W), taps=tf), module_run(False, tm), bf(decout, (H, W), taps=tb), module_run(True, ta)
    rel = lambda x, y: float((x.float() - y).abs().max() / y.abs().max())
    out["pre_activation_rel_diff_vs_module_f32"] = {"fused_f32": rel(tf["pre"], tm["pre"]), "fused_bf16": rel(tb["pre"], tm["pre"]),
                                                    "module_bf16_autocast": rel(ta["pre"], tm["pre"])}
    res["mast3r_heads"] = out


def mast3r_share_section(res, a, dev):
    import mast3r_head_layout as ML
    from gd_amd.teacher_runner import MASt3RTeacherRunner
    (H, W), B = MAST3R_IMG, 2
    cfg = dict(enc_dim=1024, enc_heads=16, enc_depth=a.depth, dec_dim=768, dec_heads=12, dec_depth=a.depth // 2, temperature=3.0, reciprocity=True)
    head_kw = {k: v for k, v in MAST3R_HEAD.items() if k not in ("enc_dim", "dec_dim")}
    with torch.device(dev):
        m = ML.tiny_matcher(cfg, (H, W), dict(head_kw, layer_dims=ML.LAYER_DIMS), fill=False)
    img1, img2 = torch.rand(1, 3, H, W, device=dev), torch.rand(1, 3, H, W, device=dev)
    depth = torch.rand(H, W, device=dev) + 1.0
    N = (H // 16) * (W // 16)
    decout = [torch.randn(B, N, cfg["enc_dim"] if i == 0 else cfg["dec_dim"], device=dev) for i in range(cfg["dec_depth"] + 1)]
    out = dict(cfg, image=[H, W], blocks="fused_blocks bf16", head=head_kw)
    runs = {}
    for tag, kw in (("module_heads_f32", {}), ("fused_heads_f32", dict(fused_heads=True)), ("fused_heads_bf16", dict(fused_heads=True, heads_dtype=torch.bfloat16))):
        r = MASt3RTeacherRunner(m, inference=ML.inference, make_pairs=ML.make_pairs, min_conf_thr=0, fused_blocks=True, dtype=torch.bfloat16, **kw)
        hs = list(r.heads.values()) if r.heads else [m.downstream_head1, m.downstream_head2]

        def heads_run(hs=hs):
            with torch.no_grad():
                for h in hs:
                    h(decout, (H, W))
        runs[tag] = (lambda r=r: r.targets(img1, img2, depth_1=depth, depth_2=depth), heads_run)
        out[tag] = {"targets_returned_none": runs[tag][0]() is None}
    # each path twice, alternating: other work shares the machine
    for again in ("", "_again"):
        for tag, (targets, heads_run) in runs.items():
            out[tag]["targets" + again] = timed(targets, 1, a.iters)
            out[tag]["two_heads" + again] = timed(heads_run, 1, a.iters)
    for tag in runs:
        best = lambda k: min(out[tag][k]["median_ms"], out[tag][k + "_again"]["median_ms"])
        out[tag]["heads_share_of_targets"] = round(best("two_heads") / best("targets"), 3)
    res["mast3r_heads_share"] = out


def mast3r_sections(res, a, dev):
    from gd_amd import teacher_glue as tg
    from gd_amd.teacher_blocks import FusedCroCoBlocks
    B, grid = 2, (24, 32)
    N = grid[0] * grid[1]
    cfg = dict(enc_dim=1024, enc_heads=16, enc_depth=a.depth, dec_dim=768, dec_heads=12, dec_depth=a.depth // 2, temperature=3.0, reciprocity=True)
    with torch.device(dev):
        m = CL.CrocoLayout(**cfg).eval()
    x1, x2 = torch.randn(B, N, cfg["enc_dim"], device=dev), torch.randn(B, N, cfg["enc_dim"], device=dev)
    pos = CL.grid_positions(B, *grid).to(dev)
    Ce, Cd, Le, Ld = cfg["enc_dim"], cfg["dec_dim"], cfg["enc_depth"], cfg["dec_depth"]
    M = 2 * B * N                                            # token rows of both views
    # encoder: 12 C^2 weights per block + QK^T and PV; decoder block: 4 C^2 (self) + 4 C^2 (cross: q, k, v, proj) + 8 C^2 (MLP) + two attention products
    # + the head-mean score GEMM; decoder_embed
    flop = (Le * (24.0 * M * Ce * Ce + 4.0 * M * N * Ce) + 2.0 * M * Ce * Cd + Ld * (32.0 * M * Cd * Cd + 8.0 * M * N * Cd + 2.0 * M * N * Cd))
    stack = dict(cfg, B=B, tokens_per_view=N, flop_per_pair=flop)

    def fused_run(f):
        e1, e2 = f.encode(x1, pos), f.encode(x2, pos)
        outs, c1, c2 = f.decode(m.enc_norm(e1), pos, m.enc_norm(e2), pos)
        return outs, tg.mast3r_tgt_attn_map(c1, c2, m.temperature)

    def module_run(autocast):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            e1, e2 = m.encode_blocks(x1, pos), m.encode_blocks(x2, pos)
            return m.target(m.enc_norm(e1), pos, m.enc_norm(e2), pos)
    f32, bf = FusedCroCoBlocks(m, dtype=torch.float32), FusedCroCoBlocks(m, dtype=torch.bfloat16)
    paths = {"fused_f32": lambda: fused_run(f32), "module_f32": lambda: module_run(False), "fused_bf16": lambda: fused_run(bf),
             "module_bf16_autocast": lambda: module_run(True)}
    # each path twice, interleaved: other work shares the machine
    for name, fn in paths.items():
        stack[name] = timed(fn, a.warm, a.iters)
    for name, fn in paths.items():
        stack[name + "_again"] = timed(fn, 1, a.iters)
    best = lambda k: min(stack[k]["median_ms"], stack[k + "_again"]["median_ms"])
    stack["speedup_fused_f32_vs_module_f32"] = round(best("module_f32") / best("fused_f32"), 3)
    stack["speedup_fused_bf16_vs_module_bf16_autocast"] = round(best("module_bf16_autocast") / best("fused_bf16"), 3)
    stack["fused_f32_tflops"] = round(flop / best("fused_f32") * 1e-9, 1)
    stack["fused_bf16_tflops"] = round(flop / best("fused_bf16") * 1e-9, 1)
    # agreement of the paths at this size (random weights): last decoder output relative to its largest value, and the target map
    (of, tf_), (om, tm) = fused_run(f32), module_run(False)
    stack["f32_last_output_rel_diff_fused_vs_module"] = float((of[0][-1] - om[0][-1]).abs().max() / om[0][-1].abs().max())
    stack["f32_tgt_attn_map_max_abs_diff_fused_vs_module"] = float((tf_ - tm).abs().max())
    (ob, tb), (oa, ta) = fused_run(bf), module_run(True)
    stack["bf16_last_output_rel_diff_vs_module_f32"] = {"fused": float((ob[0][-1] - om[0][-1]).abs().max() / om[0][-1].abs().max()),
                                                        "module_autocast": float((oa[0][-1].float() - om[0][-1]).abs().max() / om[0][-1].abs().max())}
    res["mast3r_block_stack"] = stack
    del f32, bf, m
    torch.cuda.empty_cache()

    H = 12
    kflop = 4.0 * B * H * N * N * 64
    kern = {"shape_B_Nq_Nk_H": [B, N, N, H], "flop": kflop}
    for name, dt, x3, peak in (("f32", torch.float32, False, "f32"), ("bf16", torch.bfloat16, False, "bf16"), ("f16", torch.float16, False, "bf16"),
                               ("f32x3", torch.float32, True, "bf16")):
        q, kv = torch.randn(B * N, H * 64, device=dev).to(dt), torch.randn(B * N, 2 * H * 64, device=dev).to(dt)
        t = timed(lambda: ops.cross_attention_fwd(q, kv, B, N, N, H, x3=x3), a.warm, max(a.iters, 5), reps=20)
        kern[name] = dict(t, tflops=round(kflop / t["median_ms"] * 1e-9, 1))
        if peak in PEAK_TFLOPS and name != "f32x3":
            kern[name]["frac_of_peak"] = round(kflop / t["median_ms"] * 1e-9 / PEAK_TFLOPS[peak], 4)
    res["cross_attention_kernel"] = kern

    g, enc, outs, c1, c2, tgt, e32 = TM.f32_parity()
    named = [("enc_1", enc[0]), ("enc_2", enc[1])] + [(f"out{v + 1}_{i}", t) for v in range(2) for i, t in enumerate(outs[v])]
    named += [(f"camap1_{l}", t) for l, t in enumerate(c1)] + [(f"camap2_{l}", t) for l, t in enumerate(c2)]
    par = {"f32_vs_g25_worst_e_over_max": max(TM.max_abs(t, g[n]) / float(g[n].abs().max()) for n, t in named), "f32_tokens_bound_e_over_max": 1e-4,
           "f32_tgt_attn_map_e": TM.max_abs(tgt, g["tgt_attn_map"]), "e32_layout_f32_vs_f64": e32, "f32_tgt_attn_map_bound": max(TM.TGT_TOL, 4 * e32)}
    for k, v in TM.bf16_parity_pair().items():
        par["bf16_" + k] = {"e_ref_torch_autocast": v[0], "e_hip_fused": v[1], "ratio": round(v[1] / v[0], 3)}
    res.setdefault("parity", {})["mast3r"] = par


def vggt_sections(res, a, dev):
    C, H, S = a.width, a.width // 64, 2
    P = (a.img // 14) ** 2 + 5
    with torch.device(dev):
        agg = AggregatorLayout(img_size=a.img, patch_size=14, embed_dim=C, depth=a.depth, num_heads=H, num_register_tokens=4,
                               attn_indices=[a.depth // 2, a.depth - 1], temperature=0.8).eval()
    rope = T.DeviceRope2D()
    agg.rope = rope
    for b in list(agg.frame_blocks) + list(agg.global_blocks):
        b.attn.rope = rope
        torch.nn.init.constant_(b.ls1.gamma, 0.2)       # a LayerScale that keeps 2 x depth random blocks' residual stream at O(1)
        torch.nn.init.constant_(b.ls2.gamma, 0.2)
    teacher = type("Teacher", (), {"aggregator": agg})()
    img = torch.rand(1, S, 3, a.img, a.img, device=dev)
    M = S * P
    flop = 2 * a.depth * (24.0 * M * C * C + 4.0 * M * (P + M) / 2 * C)        # 12 C^2 weights per block; QK^T and PV over N = P (frame) / S P (global)
    stack = {"width": C, "heads": H, "depth": a.depth, "views": S, "tokens_per_view": P, "flop_per_pair": flop, "dtype": "bf16"}
    fused = VGGTTeacherRunner(teacher, dtype=torch.bfloat16, fused_blocks=True)
    hooks = VGGTTeacherRunner(teacher, dtype=torch.bfloat16)
    # each path twice, interleaved: other work shares the machine
    stack["fused_aggregate"] = timed(lambda: fused.aggregate(img), a.warm, a.iters)
    stack["module_aggregate"] = timed(lambda: hooks.aggregate(img), a.warm, a.iters)
    stack["fused_aggregate_again"] = timed(lambda: fused.aggregate(img), 1, a.iters)
    stack["module_aggregate_again"] = timed(lambda: hooks.aggregate(img), 1, a.iters)
    tokens, pos = fused._block_inputs(img)
    stack["fused_blocks_only"] = timed(lambda: fused.fused.forward(tokens, pos, 1, S), a.warm, a.iters)
    f_ms = min(stack["fused_aggregate"]["median_ms"], stack["fused_aggregate_again"]["median_ms"])
    m_ms = min(stack["module_aggregate"]["median_ms"], stack["module_aggregate_again"]["median_ms"])
    stack["speedup_fused_vs_module"] = round(m_ms / f_ms, 3)
    stack["fused_blocks_tflops"] = round(flop / stack["fused_blocks_only"]["median_ms"] * 1e-9, 1)
    stack["fused_blocks_frac_of_bf16_peak"] = round(flop / stack["fused_blocks_only"]["median_ms"] * 1e-9 / PEAK_TFLOPS["bf16"], 4)
    # agreement of the two paths at this size (random weights, bf16 both): relative to the largest token value
    tf, _, maps_f = fused.aggregate(img)
    th, _, qk = hooks.aggregate(img)
    stack["tokens_rel_diff_fused_vs_module"] = round(max(float((x - y.float()).abs().max() / y.float().abs().max()) for x, y in zip(tf, th)), 5)
    res["block_stack"] = stack

    # one fused block's kernels at this size
    p = fused.fused.frame[0]
    bf = torch.bfloat16
    x32 = torch.randn(M, C, device=dev)
    y16 = torch.randn(M, C, device=dev).to(bf)
    h16 = torch.randn(M, 4 * C, device=dev).to(bf)
    qkv = torch.randn(M, 3 * C, device=dev).to(bf)
    posf = pos.to(dev).reshape(M, 2).long().contiguous()
    per_block = {
        "layernorm_f32_to_bf16": (2, lambda: ops.layernorm_fwd(x32, p.n1[0], p.n1[1], p.n1[2], save_stats=False, out_dtype=bf)),
        "gemm_qkv_bias": (1, lambda: ops.gemm_nt(y16, p.wqkv, bias=p.bqkv)),
        "qk_norm_rope": (1, lambda: ops.qk_norm_rope(qkv, 1, M, H, posf, *p.qk, p.qk_eps, p.base)),
        "attention_frame": (0.5, lambda: ops.attention_fwd(qkv, S, P, H)),
        "attention_global": (0.5, lambda: ops.attention_fwd(qkv, 1, M, H)),
        "gemm_proj_bias_residual_f32": (1, lambda: ops.gemm_nt(y16, p.wproj, out_dtype=torch.float32, bias=p.bproj, residual=x32)),
        "gemm_fc1_bias_gelu": (1, lambda: ops.gemm_nt(y16, p.w1, bias=p.b1, act=1)),
        "gemm_fc2_bias_residual_f32": (1, lambda: ops.gemm_nt(h16, p.w2, out_dtype=torch.float32, bias=p.b2, residual=x32)),
    }
    kern, total = {}, 0.0
    for name, (per, fn) in per_block.items():
        t = timed(fn, a.warm, a.iters, reps=20)
        calls = per * 2 * a.depth
        kern[name] = {"median_ms": t["median_ms"], "calls_per_pair": calls, "ms_per_pair": round(t["median_ms"] * calls, 3)}
        total += t["median_ms"] * calls
    kern["sum_ms_per_pair"] = round(total, 3)
    res["fused_kernels_at_vggt_size"] = kern

    # gd_qk_norm_rope against its algorithmic bytes
    band = {"hbm_peak_TBs": HBM_TBS}
    for tag, Bq in (("one_pair", 1), ("64_pairs", 64)):
        for dt, es in ((bf, 2), (torch.float32, 4)):
            t_ = torch.randn(Bq * M, 3 * C, device=dev).to(dt)
            pp = posf.repeat(Bq, 1).contiguous()
            ms = timed(lambda: ops.qk_norm_rope(t_, Bq, M, H, pp, *p.qk, p.qk_eps, p.base), a.warm, a.iters, reps=20 if Bq == 1 else 3)["median_ms"]
            nbytes = 2.0 * (2.0 / 3.0) * t_.numel() * es
            band[f"{tag}_{'bf16' if es == 2 else 'f32'}"] = {"tensor_bytes": t_.numel() * es, "algorithmic_bytes": nbytes, "median_ms": ms,
                                                             "TBs": round(nbytes / ms * 1e-9, 3), "frac_of_hbm_peak": round(nbytes / ms * 1e-9 / HBM_TBS, 3)}
            del t_
    res["qk_norm_rope_bandwidth"] = band
    del agg, fused, hooks
    torch.cuda.empty_cache()

    pair = T.bf16_parity_pair()
    res.setdefault("parity", {}).update({k: {"e_ref_torch_autocast": v[0], "e_hip_fused": v[1], "ratio": round(v[1] / v[0], 3)} for k, v in pair.items()})


if __name__ == "__main__":
    main()
