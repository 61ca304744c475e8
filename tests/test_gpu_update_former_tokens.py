"""GPU: the tracker's update transformer and the tracker's own linear layers on gd_tokens_linear (FusedUpdateFormer(linear="tokens"),
FusedTracker(fused_updateformer=True, linear="tokens"), VGGTTeacherRunner(fused_tracker=True, fused_updateformer=True, tracker_linear="tokens")), on the
layouts, truths and bounds of tests/test_gpu_update_former.py and tests/test_gpu_vggt_tracker.py: the truth is tracker_layout.UpdateFormerLayout in fp64
and a result's error against it is at most 4 max(the fp32 torch layout's error on the GPU, its error on the CPU, one ulp of the largest value).
Every figure is printed before it is asserted."""
import pytest
import torch

import tracker_layout as TL
from conftest import load_golden
from test_gpu_update_former import DIN, ULP, gen, judged, make_former
from test_gpu_vggt_tracker import Recording, run_errors, truth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("space_depth,time_depth,hidden,B,N,S", [
    (2, 2, 96, 1, 40, 2),        # case a's sizes
    (2, 2, 96, 2, 5, 3),         # case c's: batch and frame indexing, nv = 64 > N
    (2, 2, 384, 1, 40, 2),       # the teacher's width: head dimension 48
    (2, 4, 96, 2, 5, 3),         # a space stage every second block, the last time block without one
    (0, 2, 96, 2, 5, 3),         # no space attention: no virtual tracks
])
def test_whole_transformer_on_tokens_linear(space_depth, time_depth, hidden, B, N, S):
    from gd_amd.teacher_tracker import FusedUpdateFormer
    x = torch.randn(B, N, S, DIN, generator=gen(N + S))
    mk = lambda: make_former(space_depth, time_depth, hidden)
    fused, plain = FusedUpdateFormer(mk().cuda(), linear="tokens"), FusedUpdateFormer(mk().cuda())
    with torch.no_grad():
        t64 = mk().double()(x.double())[0]
        cpu, gpu = mk()(x)[0], mk().cuda()(x.cuda())[0]
    delta, none = fused(x.cuda())
    assert none is None and delta.stride(-1) == 1
    judged(f"update transformer on tokens_linear: space {space_depth} time {time_depth} hidden {hidden} B={B} N={N} S={S} ({fused.launches} launches)",
           delta, t64, cpu, gpu)
    assert torch.equal(fused(x.cuda())[0], delta)                               # two calls: the same bits
    plain(x.cuda())
    assert fused.launches == plain.launches                                     # launches count as before
    late = FusedUpdateFormer(mk(), linear="tokens")                             # a transformer read on the host follows its input to the GPU
    assert torch.equal(late(x.cuda())[0], delta)


@pytest.mark.parametrize("case", list(TL.CASES))
def test_teacher_forced_step_on_tokens_linear(case):
    """As test_gpu_vggt_tracker.test_teacher_forced_step, under its bound max(2 max(e_torch_gpu, e_torch_cpu), 4 ulp of the largest value)."""
    from gd_amd.teacher_tracker import FusedTracker
    states, _, _, _ = truth(case)
    q, fmaps = TL.seeded_inputs(case)
    trk64, trk_cpu, trk_gpu = TL.make_tracker(case).double(), TL.make_tracker(case), TL.make_tracker(case).cuda()
    fused = FusedTracker(trk_gpu, fused_updateformer=True, linear="tokens")
    with torch.no_grad():
        base = {"f64": trk64.prepare(q.double(), fmaps.double()), "cpu": trk_cpu.prepare(q, fmaps), "gpu": trk_gpu.prepare(q.cuda(), fmaps.cuda())}
        hip = fused.begin(q.cuda(), fmaps.cuda())
    for i, (c64, f64) in enumerate(states):
        c32, f32 = c64.float(), f64.float()
        out = {}
        with torch.no_grad():
            for name, trk, dev, dt in (("f64", trk64, "cpu", torch.float64), ("cpu", trk_cpu, "cpu", torch.float32), ("gpu", trk_gpu, "cuda", torch.float32)):
                st = dict(base[name], coords=c32.to(dev, dt), feats=f32.to(dev, dt))
                pred = trk.iterate(st)
                out[name] = (pred.cpu().double(), st["feats"].cpu().double())
            hip.load(c32.cuda(), f32.cuda())
            pred = fused.step(hip)
            out["hip"] = (pred.cpu().double(), hip.feats_bsn.cpu().double())
        for k, what in enumerate(("coords (px)", "track_feats")):
            e = {n: float((out[n][k] - out["f64"][k]).abs().max()) for n in ("cpu", "gpu", "hip")}
            floor = 4 * ULP * float(out["f64"][k].abs().max())
            bound = max(2 * max(e["gpu"], e["cpu"]), floor)
            print(f"tokens: case {case} iteration {i + 1} {what}: e_hip {e['hip']:.3e}, e_torch_gpu {e['gpu']:.3e}, e_torch_cpu {e['cpu']:.3e}, floor {floor:.3e}")
            assert e["hip"] <= bound, (what, i)


@pytest.mark.parametrize("case", list(TL.CASES))
def test_whole_run_on_tokens_linear(case):
    """As test_gpu_vggt_tracker.test_whole_run_against_fixture_and_fp64: per iteration against the layout in fp64, and against fixture G28; two runs
    give the same bits."""
    from gd_amd.teacher_tracker import FusedTracker, FusedUpdateFormer
    g = load_golden("g28_vggt_tracker")
    q, fmaps = TL.seeded_inputs(case)
    fused = FusedTracker(TL.make_tracker(case).cuda(), fused_updateformer=True, linear="tokens")
    assert isinstance(fused.updateformer, FusedUpdateFormer) and fused.updateformer.linear == "tokens"
    preds, vis, conf = fused(q.cuda(), fmaps.cuda(), iters=TL.ITERS)
    c = TL.CASES[case]
    assert len(preds) == TL.ITERS and preds[0].shape == (c["B"], c["S"], c["N"], 2) and vis.shape == conf.shape == (c["B"], c["S"], c["N"])
    rows, _, _ = run_errors(case, preds, vis, conf)
    for row in rows:
        print(f"tokens: case {case} {row[0]}: e_hip {row[1]:.3e}, e_torch_cpu {row[3]:.3e}, e_torch_gpu {row[4]:.3e}, bound 4 max(e_torch_gpu, e_torch_cpu, ulp) = {row[2]:.3e}")
    for row in rows:
        assert row[1] <= row[2], row[0]
    _, p64, v64, c64 = truth(case)
    for name, got, want, t64, bound in (("coords", torch.stack(preds), g[f"{case}_coords"], torch.stack(p64), rows[TL.ITERS - 1][2]),
                                        ("vis", vis, g[f"{case}_vis"], v64, rows[TL.ITERS][2]), ("conf", conf, g[f"{case}_conf"], c64, rows[TL.ITERS + 1][2])):
        e, e_ref = float((got.cpu() - want).abs().max()), float((want.double() - t64).abs().max())
        print(f"tokens: case {case} {name}: against the reference's fp32 run (G28) {e:.3e}; that run is {e_ref:.3e} from fp64")
        assert e <= bound + e_ref, name
    again = fused(q.cuda(), fmaps.cuda(), iters=TL.ITERS)
    assert all(torch.equal(u, v) for u, v in zip(list(again[0]) + [again[1], again[2]], list(preds) + [vis, conf]))
    # the tracker's own linear layers alone on the new kernel, around the user's module
    own = FusedTracker(TL.make_tracker(case).cuda(), linear="tokens")
    rows_own, _, _ = run_errors(case, *own(q.cuda(), fmaps.cuda(), iters=TL.ITERS))
    for row in rows_own:
        print(f"tokens (module transformer): case {case} {row[0]}: e_hip {row[1]:.3e}, bound {row[2]:.3e}")
        assert row[1] <= row[2], row[0]


class Replayable(Recording):
    """Recording that also keeps the call's arguments, so that the call can be made again on the same bits."""

    def __call__(self, *a, **k):
        keep = lambda v: v.detach().clone() if torch.is_tensor(v) else v
        self.args, self.kwargs = tuple(keep(v) for v in a), {n: keep(v) for n, v in k.items()}
        return super().__call__(*a, **k)


def test_runner_tracker_linear_tokens_against_gemm_nt():
    """As test_gpu_update_former.test_runner_fused_updateformer_off_and_on: the runner with tracker_linear "gemm_nt" and "tokens" (fused_tracker and
    fused_updateformer on) against the default path: same keys, shapes, masks, kp_1 and integer kp_2; the float tracks within
    4 max(e_torch_gpu, e_torch_cpu, ulp) of the layout in fp64; the runner's tracker call, made twice more on the arguments the runner handed it (the
    torch heads in front of it are not reproducible run to run), gives the recorded bits both times."""
    import dpt_layout as DL
    from gd_amd.teacher_runner import VGGTTeacherRunner
    from test_gpu_teacher_blocks import DeviceRope2D
    teacher = TL.make_tiny_vggt()
    rope = DeviceRope2D()
    teacher.aggregator.rope = rope
    for blk in list(teacher.aggregator.frame_blocks) + list(teacher.aggregator.global_blocks):
        blk.attn.rope = rope
    teacher = teacher.cuda()
    img = torch.rand(1, 2, 3, DL.TinyVGGT.IMG[0], DL.TinyVGGT.IMG[1], generator=gen(240)).cuda()
    seen = {}
    def keep(key, value):                                                      # the first call's: the default path's (a hook returns None)
        if key not in seen:
            seen[key] = value.detach().clone()
    hooks = [teacher.track_head.feature_extractor.register_forward_hook(lambda m, a, out: keep("fmaps", out)),
             teacher.track_head.register_forward_hook(lambda m, a, out: keep("tracks", out[0][-1])),
             teacher.track_head.register_forward_pre_hook(lambda m, a, k: keep("query", k["query_points"]), with_kwargs=True)]
    runs, tracks = {}, {}
    both = dict(fused_tracker=True, fused_updateformer=True)
    for name, kw in (("default", dict()), ("gemm_nt", dict(both, tracker_linear="gemm_nt")), ("tokens", dict(both, tracker_linear="tokens"))):
        r = VGGTTeacherRunner(teacher, dtype=torch.float32, pose_decoder=DL.tiny_pose_decoder, **kw)
        if name != "default":
            assert r.tracker.linear == r.tracker.updateformer.linear == kw["tracker_linear"]
            r.tracker = Replayable(r.tracker)
        runs[name] = r.targets(img, num_keypoints=50, min_distance=3, generator=torch.Generator(device="cuda").manual_seed(1))
        if name != "default":
            tracks[name] = r.tracker.last
            for _ in range(2):
                again = r.tracker.inner(*r.tracker.args, **r.tracker.kwargs)
                assert torch.equal(again[0][-1], tracks[name]), name
    for h in hooks:
        h.remove()
    a = runs["default"]
    assert a is not None and a["kp_1"].shape[0] > 0
    q, fm = seen["query"].float().cpu(), seen["fmaps"].float().cpu()
    with torch.no_grad():
        t64 = TL.make_tiny_vggt().track_head.tracker.double()(q.double(), fm.double(), iters=TL.ITERS)[0][-1]
        t_cpu = TL.make_tiny_vggt().track_head.tracker(q, fm, iters=TL.ITERS)[0][-1]
    e_gpu, e_cpu = float((seen["tracks"].cpu().double() - t64).abs().max()), float((t_cpu.double() - t64).abs().max())
    bound = 4 * max(e_gpu, e_cpu, ULP * float(t64.abs().max()))
    tr = seen["tracks"][0, 1].double()
    margin = float(torch.minimum(tr - tr.floor(), tr.ceil() - tr).min())
    for name in ("gemm_nt", "tokens"):
        b = runs[name]
        assert b is not None and set(a) == set(b)
        for k in a:
            assert a[k].shape == b[k].shape, (name, k)
        assert torch.equal(a["kp_1"], b["kp_1"]) and torch.equal(a["mask_1"], b["mask_1"]) and torch.equal(a["mask_2"], b["mask_2"]), name
        e_hip = float((tracks[name].cpu().double() - t64).abs().max())
        print(f"runner tracker_linear={name}: float tracks e_hip {e_hip:.3e}, e_torch_gpu {e_gpu:.3e}, e_torch_cpu {e_cpu:.3e}, bound {bound:.3e}; "
              f"the default path's tracks keep {margin:.3e} px from the nearest integer")
        assert e_hip <= bound, name
        assert margin > bound + e_gpu
        assert torch.equal(a["kp_2"], b["kp_2"]), name
