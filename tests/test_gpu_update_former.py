"""GPU: the tracker's update transformer on the HIP kernels (gd_amd.teacher_tracker.FusedUpdateFormer, FusedTracker(fused_updateformer=True),
VGGTTeacherRunner(fused_tracker=True, fused_updateformer=True)).  The truth is tracker_layout.UpdateFormerLayout in fp64, which fixture G28 pins to
the reference's module (tests/test_tracker_layout_host.py); a result is judged as tests/test_gpu_vggt_tracker.py judges a step: its error against fp64
is at most 4 max(the fp32 torch layout's error on the GPU, its error on the CPU, one ulp of the largest value).
  1. one self block and one cross block alone, through the class's own block routines;
  2. the whole transformer on five layouts;
  3. FusedTracker with the fused transformer inside: teacher-forced steps and whole runs of the fixture cases, under test_gpu_vggt_tracker's bounds;
  4. the runner with `fused_updateformer` off and on, for both settings of `fused_heads`.
Every figure is printed before it is asserted."""
import pytest
import torch

import tracker_layout as TL
from conftest import load_golden
from test_gpu_vggt_tracker import Recording, run_errors, truth

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
DIN, DOUT = 3 * TL.LATENT + 4, TL.LATENT + 2


def gen(seed):
    return torch.Generator().manual_seed(seed)


def make_former(space_depth, time_depth, hidden, seed=31):
    from test_teacher_runner_ref import fill_params
    m = TL.UpdateFormerLayout(space_depth, time_depth, DIN, hidden, DOUT)
    fill_params(m, seed=seed)
    return m.eval()


def judged(name, got, t64, cpu, gpu):
    e = [float((t.detach().cpu().double() - t64).abs().max()) for t in (got, cpu, gpu)]
    bound = 4 * max(e[1], e[2], ULP * float(t64.abs().max()))
    print(f"{name}: e_hip {e[0]:.3e}, e_torch_cpu {e[1]:.3e}, e_torch_gpu {e[2]:.3e}, bound 4 max(e_torch_gpu, e_torch_cpu, ulp) = {bound:.3e}")
    assert tuple(got.shape) == tuple(t64.shape) and e[0] <= bound, name


# ---------------------------------------------------------------------------------------------------------------------------------- 1. blocks
def test_self_block_and_cross_block_alone():
    """Tokens [2, 7, 3, 96] (b, n, s).  The self block runs as a time block (sequences of S consecutive rows), the cross block as `point2virtual` of a
    space stage (4 points attend to 3 virtual rows per frame, tokens S rows apart).  The teacher's blocks keep norm1(x), not x, as the residual."""
    from gd_amd.teacher_tracker import FusedUpdateFormer
    B, n, S, D, N = 2, 7, 3, TL.HIDDEN, 4
    m = make_former(2, 2, D)
    fused = FusedUpdateFormer(make_former(2, 2, D).cuda())
    tok = torch.randn(B, n, S, D, generator=gen(7)) * 2 + 0.5
    with torch.no_grad():
        # self
        blk = m.time_blocks[1]
        ref = {k: mod(tok.to(dev, dt).reshape(B * n, S, D)).reshape(B, n, S, D)
               for k, mod, dev, dt in (("f64", make_former(2, 2, D).double().time_blocks[1], "cpu", torch.float64), ("cpu", blk, "cpu", torch.float32),
                                       ("gpu", make_former(2, 2, D).cuda().time_blocks[1], "cuda", torch.float32))}
        x = tok.cuda().clone()
        out = fused.self_block(fused.time_blocks[1], x.view(B * n * S, D), (B * n, 1, S, S, 0, 1))
        assert out.data_ptr() == x.data_ptr()                                # written back in place
        judged("self block (time layout)", x, ref["f64"], ref["cpu"], ref["gpu"])
        b64, t64 = make_former(2, 2, D).double().time_blocks[1], tok.double().reshape(B * n, S, D)
        xn = b64.norm1(t64)
        x1 = t64 + b64.attn(xn, xn, xn)[0]                                   # the usual pre-norm block: the block INPUT as the residual
        pre_norm = (x1 + b64.mlp(b64.norm2(x1))).reshape(B, n, S, D)
        print(f"self block: the pre-norm residual form is {float((pre_norm - ref['f64']).abs().max()):.3e} from the teacher's form")
        # cross: per batch entry, points = tokens[:, :N], context = tokens[:, N:], per frame
        def cross(mod, t):
            sp = t.permute(0, 2, 1, 3).reshape(B * S, n, D)
            return mod(sp[:, :N], sp[:, N:]).view(B, S, N, D).permute(0, 2, 1, 3)
        ref = {k: cross(f.space_point2virtual_blocks[0], tok.to(dev, dt))
               for k, f, dev, dt in (("f64", make_former(2, 2, D).double(), "cpu", torch.float64), ("cpu", m, "cpu", torch.float32),
                                     ("gpu", make_former(2, 2, D).cuda(), "cuda", torch.float32))}
        x = tok.cuda().clone()
        rows = x.view(B, n * S, D)
        for b in range(B):
            fused.cross_block(fused.space_point2virtual_blocks[0], rows[b, :N * S], rows[b, N * S:], (1, S, N, 0, 1, S), (1, S, n - N, 0, 1, S))
        judged("cross block (space layout)", x[:, :N], ref["f64"], ref["cpu"], ref["gpu"])
        assert torch.equal(x[:, N:].cpu(), tok[:, N:])                       # the context rows are read only


# ---------------------------------------------------------------------------------------------------------------------------------- 2. the transformer
@pytest.mark.parametrize("space_depth,time_depth,hidden,B,N,S", [
    (2, 2, 96, 1, 40, 2),        # case a's sizes
    (2, 2, 96, 2, 5, 3),         # case c's: batch and frame indexing, nv = 64 > N
    (2, 2, 384, 1, 40, 2),       # the teacher's width: head dimension 48
    (2, 4, 96, 2, 5, 3),         # a space stage every second block, the last time block without one
    (0, 2, 96, 2, 5, 3),         # no space attention: no virtual tracks
])
def test_whole_transformer(space_depth, time_depth, hidden, B, N, S):
    from gd_amd.teacher_tracker import FusedUpdateFormer
    x = torch.randn(B, N, S, DIN, generator=gen(N + S))
    mk = lambda: make_former(space_depth, time_depth, hidden)
    fused = FusedUpdateFormer(mk().cuda())
    with torch.no_grad():
        t64 = mk().double()(x.double())[0]
        cpu, gpu = mk()(x)[0], mk().cuda()(x.cuda())[0]
    delta, none = fused(x.cuda())
    assert none is None and delta.stride(-1) == 1
    judged(f"update transformer space {space_depth} time {time_depth} hidden {hidden} B={B} N={N} S={S} ({fused.launches} launches)", delta, t64, cpu, gpu)
    again = fused(x.cuda())[0]
    assert torch.equal(again, delta)
    # a transformer read on the host follows its input to the GPU
    late = FusedUpdateFormer(mk())
    assert torch.equal(late(x.cuda())[0], delta)


# ---------------------------------------------------------------------------------------------------------------------------------- 3. inside the tracker
@pytest.mark.parametrize("case", list(TL.CASES))
def test_teacher_forced_step_with_the_fused_transformer(case):
    """As test_gpu_vggt_tracker.test_teacher_forced_step, under its bound max(2 max(e_torch_gpu, e_torch_cpu), 4 ulp of the largest value)."""
    from gd_amd.teacher_tracker import FusedTracker
    states, _, _, _ = truth(case)
    q, fmaps = TL.seeded_inputs(case)
    trk64, trk_cpu, trk_gpu = TL.make_tracker(case).double(), TL.make_tracker(case), TL.make_tracker(case).cuda()
    fused = FusedTracker(trk_gpu, fused_updateformer=True)
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
            print(f"case {case} iteration {i + 1} {what}: e_hip {e['hip']:.3e}, e_torch_gpu {e['gpu']:.3e}, e_torch_cpu {e['cpu']:.3e}, floor {floor:.3e}")
            assert e["hip"] <= bound, (what, i)


@pytest.mark.parametrize("case", list(TL.CASES))
def test_whole_run_with_the_fused_transformer(case):
    """As test_gpu_vggt_tracker.test_whole_run_against_fixture_and_fp64: per iteration against the layout in fp64, and against fixture G28."""
    from gd_amd.teacher_tracker import FusedTracker, FusedUpdateFormer
    g = load_golden("g28_vggt_tracker")
    q, fmaps = TL.seeded_inputs(case)
    fused = FusedTracker(TL.make_tracker(case).cuda(), fused_updateformer=True)
    assert isinstance(fused.updateformer, FusedUpdateFormer)
    preds, vis, conf = fused(q.cuda(), fmaps.cuda(), iters=TL.ITERS)
    c = TL.CASES[case]
    assert len(preds) == TL.ITERS and preds[0].shape == (c["B"], c["S"], c["N"], 2) and vis.shape == conf.shape == (c["B"], c["S"], c["N"])
    rows, _, _ = run_errors(case, preds, vis, conf)
    for row in rows:
        print(f"case {case} {row[0]}: e_hip {row[1]:.3e}, e_torch_cpu {row[3]:.3e}, e_torch_gpu {row[4]:.3e}, bound 4 max(e_torch_gpu, e_torch_cpu, ulp) = {row[2]:.3e}")
    for row in rows:
        assert row[1] <= row[2], row[0]
    _, p64, v64, c64 = truth(case)
    for name, got, want, t64, bound in (("coords", torch.stack(preds), g[f"{case}_coords"], torch.stack(p64), rows[TL.ITERS - 1][2]),
                                        ("vis", vis, g[f"{case}_vis"], v64, rows[TL.ITERS][2]), ("conf", conf, g[f"{case}_conf"], c64, rows[TL.ITERS + 1][2])):
        e, e_ref = float((got.cpu() - want).abs().max()), float((want.double() - t64).abs().max())
        print(f"case {case} {name}: against the reference's fp32 run (G28) {e:.3e}; that run is {e_ref:.3e} from fp64")
        assert e <= bound + e_ref, name


def test_forward_returns_the_same_structure_with_return_feat_on_and_off():
    from gd_amd.teacher_tracker import FusedTracker
    case = "c"
    q, fmaps = TL.seeded_inputs(case)
    trk = TL.make_tracker(case).cuda()
    plain, fused = FusedTracker(trk), FusedTracker(trk, fused_updateformer=True)
    for kw in (dict(), dict(return_feat=True), dict(return_feat=True, down_ratio=2, apply_sigmoid=False)):
        a, b = plain(q.cuda(), fmaps.cuda(), iters=2, **kw), fused(q.cuda(), fmaps.cuda(), iters=2, **kw)
        assert len(a) == len(b) == (5 if kw.get("return_feat") else 3) and len(a[0]) == len(b[0]) == 2
        for u, v in zip(list(a[0]) + list(a[1:]), list(b[0]) + list(b[1:])):
            assert (u is None and v is None) or (u.shape == v.shape and u.dtype == v.dtype and bool(torch.isfinite(v).all()))


# ---------------------------------------------------------------------------------------------------------------------------------- 4. the runner
@pytest.mark.parametrize("fused_heads", [False, True])
def test_runner_fused_updateformer_off_and_on(fused_heads):
    """As test_gpu_vggt_tracker.test_runner_fused_tracker_against_default_path, with a third runner: same keys, shapes, masks and kp_1; the float tracks
    within 4 max(e_torch_gpu, e_torch_cpu, ulp) of the layout in fp64, and kp_2 equal because the default path's tracks keep more than that from every
    integer."""
    import dpt_layout as DL
    from gd_amd.teacher_runner import VGGTTeacherRunner
    from gd_amd.teacher_tracker import FusedUpdateFormer
    from test_gpu_teacher_blocks import DeviceRope2D
    teacher = TL.make_tiny_vggt()
    rope = DeviceRope2D()
    teacher.aggregator.rope = rope
    for blk in list(teacher.aggregator.frame_blocks) + list(teacher.aggregator.global_blocks):
        blk.attn.rope = rope
    teacher = teacher.cuda()
    own = lambda: {n: set(vars(m)) for n, m in teacher.named_modules() if n.startswith("track_head")}
    before = own()
    img = torch.rand(1, 2, 3, DL.TinyVGGT.IMG[0], DL.TinyVGGT.IMG[1], generator=gen(240)).cuda()
    seen = {}
    def keep(key, value):                                                      # the first call's: the default path's (a hook returns None)
        if key not in seen:
            seen[key] = value.detach().clone()
    hooks = [teacher.track_head.feature_extractor.register_forward_hook(lambda m, a, out: keep("fmaps", out)),
             teacher.track_head.register_forward_hook(lambda m, a, out: keep("tracks", out[0][-1])),
             teacher.track_head.register_forward_pre_hook(lambda m, a, k: keep("query", k["query_points"]), with_kwargs=True)]
    runs, tracks = {}, {}
    for name, kw in (("default", dict()), ("tracker", dict(fused_tracker=True)), ("former", dict(fused_tracker=True, fused_updateformer=True))):
        r = VGGTTeacherRunner(teacher, dtype=torch.float32, pose_decoder=DL.tiny_pose_decoder, fused_heads=fused_heads, **kw)
        if name != "default":
            assert isinstance(r.tracker.updateformer, FusedUpdateFormer) == (name == "former")
            r.tracker = Recording(r.tracker)
        runs[name] = r.targets(img, num_keypoints=50, min_distance=3, generator=torch.Generator(device="cuda").manual_seed(1))
        if name != "default":
            tracks[name] = r.tracker.last
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
    for name in ("tracker", "former"):
        b = runs[name]
        assert b is not None and set(a) == set(b)
        for k in a:
            assert a[k].shape == b[k].shape, (name, k)
        assert torch.equal(a["kp_1"], b["kp_1"]) and torch.equal(a["mask_1"], b["mask_1"]) and torch.equal(a["mask_2"], b["mask_2"]), name
        e_hip = float((tracks[name].cpu().double() - t64).abs().max())
        print(f"runner fused_heads={fused_heads} {name}: float tracks e_hip {e_hip:.3e}, e_torch_gpu {e_gpu:.3e}, e_torch_cpu {e_cpu:.3e}, bound {bound:.3e}; "
              f"the default path's tracks keep {margin:.3e} px from the nearest integer")
        assert e_hip <= bound, name
        assert margin > bound + e_gpu
        assert torch.equal(a["kp_2"], b["kp_2"]), name
    assert own() == before
