"""GPU: the VGGT tracker tail on the HIP kernels (csrc/vggt_track.hip, gd_amd.teacher_tracker.FusedTracker, VGGTTeacherRunner(fused_tracker=True)).
  1. gd_avgpool2_cl per element against fp64;
  2. gd_corr_sample per element against the fp64 restatement of the fused formulation (tests/track_corr_ref64.py) on the same fp32 inputs;
  3. gd_points_bilinear, gd_track_pos_embed, gd_track_assemble per element against fp64;
  4. one teacher-forced FusedTracker.step per iteration against the layout (tests/tracker_layout.py) in fp64 stepping from the same state,
     judged by the fp32 torch layout's own single-step error on the GPU and on the CPU;
  5. the whole run against fixture G28 (the reference's tracker) and the layout in fp64, judged the same way per iteration;
  6. the runner with `fused_tracker` off and on, for both settings of `fused_heads`.
Every bound is derived in track_corr_ref64.py or stated where it is used; every figure is printed before it is asserted."""
import functools

import pytest
import torch

import track_corr_ref64 as R64
import tracker_layout as TL
from conftest import load_golden

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23


def gen(seed):
    return torch.Generator().manual_seed(seed)


def worst(err, bound):
    """(largest err / bound, its err, its bound) over the elements."""
    ratio = err / bound
    i = int(ratio.argmax())
    return float(ratio.reshape(-1)[i]), float(err.reshape(-1)[i]), float(bound.reshape(-1)[i])


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. pooling
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,H,W", [(2, 7, 9), (1, 8, 6), (3, 2, 2), (1, 131, 139)])
@pytest.mark.parametrize("sep", [0, 1])
def test_avgpool2_cl_per_element(F, H, W, sep):
    from gd_amd import ops
    m = torch.randn(F, H, W, 128, generator=gen(H * W)) * torch.rand(F, H, W, 1, generator=gen(7)) * 4
    src = (R64.pitched(m) if sep else m).cuda()
    got = ops.avgpool2_cl(src, W, pitch_out=W // 2 + sep)
    assert got.shape == (F, H // 2, W // 2 + sep, 128)
    want, bound = R64.pool2_64(m), R64.pool2_bound(m)
    r, e, b = worst((got[:, :, :W // 2].cpu().double() - want).abs(), bound.clamp_min(R64.TINY))
    print(f"avgpool2_cl {F}x{H}x{W} sep={sep}: worst err / bound {r:.2f} (err {e:.2e}, bound 3 U mean|inputs| = {b:.2e})")
    assert r <= 1.0
    if sep:
        assert float(got[:, :, W // 2:].abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. correlation window sampling
# ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corr_case(case):
    """fp32 inputs of the first iteration (frames s > 0 moved off the query) and the fp64 restatement's (out, A) on exactly those."""
    from test_teacher_tracker_host import first_iteration
    pyr, targets, coords = first_iteration(case, torch.float32)
    levels = R64.pyramid32(R64.nchw_to_cl(pyr.maps[0]), TL.CASES[case]["levels"])
    want, A = R64.corr_sample64(levels, targets, coords, TL.RADIUS)
    return levels, targets, coords, want, A


@pytest.mark.parametrize("case", list(TL.CASES))
@pytest.mark.parametrize("sep", [0, 1])
def test_corr_sample_per_element(case, sep):
    from gd_amd import ops
    levels, targets, coords, want, A = corr_case(case)
    B, S, N, C = targets.shape
    n = want.shape[-1]
    ld = n if not sep else (n + 31) // 32 * 32 + 32
    pyramid = [((R64.pitched(m) if sep else m).cuda(), m.shape[1], m.shape[2], m.shape[2] + sep) for m in levels]
    junk = torch.full((B * S, N, ld), float("nan"), device="cuda")          # the block the output is about to be carved from: stale NaNs
    del junk
    got = ops.corr_sample(pyramid, targets.permute(0, 2, 1, 3).contiguous().cuda(), coords.permute(0, 2, 1, 3).contiguous().cuda(), TL.RADIUS, ld=ld)
    assert got.shape == (B * S, N, ld)
    got = got.cpu().view(B, S, N, ld)
    assert float(got[..., n:].abs().max()) == 0.0 if ld > n else True       # pad columns: exactly 0 (and not NaN)
    got = got[..., :n].double()
    r, e, b = worst((got - want).abs(), R64.corr_bound(A))
    zero = A == 0
    print(f"corr_sample case {case} pitch=W+{sep}: worst err / bound {r:.3f} (err {e:.2e}, bound (C + 8) U A = {b:.2e}); "
          f"{int(zero.sum())} of {zero.numel()} entries expected 0")
    assert bool(torch.isfinite(got).all()) and r <= 1.0
    assert bool((got[zero] == 0).all())


def test_corr_sample_far_and_non_finite_points_give_zeros():
    from gd_amd import ops
    m = torch.randn(1, 8, 8, 128, generator=gen(3)).cuda()
    coords = torch.tensor([[1e12, 3.0], [float("nan"), 2.0], [3.0, float("-inf")], [-2e9, -2e9]]).view(1, 4, 1, 2).cuda()
    got = ops.corr_sample([(m, 8, 8, 8)], torch.randn(1, 4, 1, 128, generator=gen(4)).cuda(), coords, 4)
    assert float(got.abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. point sampling, position embedding, input assembly
# ----------------------------------------------------------------------------------------------------------------------------------
def planted_points(B, N, H, W, seed):
    p = torch.rand(B, N, 2, generator=gen(seed)) * torch.tensor([W + 6.0, H + 6.0]) - 3.0
    p[:, :5] = torch.tensor([[0.0, 0.0], [W - 1.0, H - 1.0], [3.0, 2.0], [2.5, 1.5], [-7.25, H + 9.0]])
    return p


@pytest.mark.parametrize("B,S,H,W,sep", [(2, 3, 9, 11, 0), (2, 3, 9, 11, 1), (1, 2, 21, 35, 1)])
def test_points_bilinear_per_element(B, S, H, W, sep):
    from gd_amd import ops
    m = torch.randn(B * S, H, W, 128, generator=gen(W))
    pts = planted_points(B, 40, H, W, 11)
    got = ops.points_bilinear((R64.pitched(m) if sep else m).cuda(), W, pts.cuda(), frame_step=S).cpu().double()
    want, mag = R64.points_bilinear64(m[0::S], pts)
    r, e, b = worst((got - want).abs(), 4 * ULP * mag + R64.TINY)
    print(f"points_bilinear {B}x{S}x{H}x{W} sep={sep}: worst err / bound {r:.3f} (err {e:.2e}, bound 4 ulp of the blended magnitude = {b:.2e})")
    assert r <= 1.0


@pytest.mark.parametrize("H,W", [(9, 11), (259, 259)])
def test_track_pos_embed_per_element(H, W):
    from gd_amd import ops
    pts = planted_points(1, 60, H, W, 12)[0]
    got = ops.track_pos_embed(pts.cuda(), H, W, 388).cpu().double()
    want, bound = R64.pos_embed64(pts, H, W, 388)
    r, e, b = worst((got - want).abs(), bound)
    print(f"track_pos_embed {H}x{W}: worst err / bound {r:.3f} (err {e:.2e}, bound {b:.2e})")
    assert got.shape == (60, 388) and r <= 1.0
    # and it is the bilinear sample of the table the layout builds on the host
    table = TL.sample_points(TL.position_table(388, H, W, torch.float64), pts[None].double())[0]
    assert float((want - table).abs().max()) <= 1e-12


@pytest.mark.parametrize("B,S,N", [(1, 2, 40), (2, 3, 5)])
def test_track_assemble_per_element(B, S, N):
    from gd_amd import ops
    g = gen(13)
    coords = torch.rand(B, N, S, 2, generator=g) * 40 - 5            # flows up to ~45 cells: arguments to 4e4
    corr, feats = torch.randn(B, S, N, 128, generator=g), torch.randn(B, N, S, 128, generator=g)
    pos, tok = torch.randn(B * N, 388, generator=g), torch.randn(2, 388, generator=g)
    got = ops.track_assemble(coords.cuda(), corr.cuda(), feats.cuda(), pos.cuda(), tok.cuda(), 518).cpu().double()
    want, bound = R64.assemble64(coords, corr, feats, pos, tok, 518.0)
    r, e, b = worst((got - want).abs(), bound)
    print(f"track_assemble B={B} S={S} N={N}: worst err / bound {r:.3f} (err {e:.2e}, bound {b:.2e})")
    assert got.shape == (B, N, S, 388) and r <= 1.0


def test_track_update_is_exact():
    from gd_amd import ops
    g = gen(14)
    B, N, S = 2, 5, 3
    delta, coords = torch.randn(B, N, S, 130, generator=g), torch.rand(B, N, S, 2, generator=g) * 30
    c = coords.clone().cuda()
    pred, dfeat = ops.track_update(delta.cuda(), c, 2.0, 3.0)
    want = coords + delta[..., :2]
    want[:, :, 0] = coords[:, :, 0]
    assert torch.equal(c.cpu(), want) and torch.equal(dfeat.cpu(), delta[..., 2:].reshape(-1, 128))
    assert torch.equal(pred.cpu(), (want * 2.0 * 3.0).permute(0, 2, 1, 3))


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. / 5. the loop
# ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def truth(case):
    """The layout in fp64: per iteration the state BEFORE it (coords, feats), and the run's results."""
    trk = TL.make_tracker(case).double()
    q, fmaps = TL.seeded_inputs(case)
    states, preds = [], []
    with torch.no_grad():
        st = trk.prepare(q.double(), fmaps.double())
        for _ in range(TL.ITERS):
            states.append((st["coords"].clone(), st["feats"].clone()))
            preds.append(trk.iterate(st))
        vis, conf = trk.finish(st)
    return states, preds, vis, conf


def layout_run(case, device, **kw):
    trk = TL.make_tracker(case).to(device)
    q, fmaps = TL.seeded_inputs(case)
    with torch.no_grad():
        return trk(q.to(device), fmaps.to(device), iters=TL.ITERS, **kw)


@pytest.mark.parametrize("case", ["a", "b"])
def test_teacher_forced_step(case):
    from gd_amd.teacher_tracker import FusedTracker
    states, _, _, _ = truth(case)
    q, fmaps = TL.seeded_inputs(case)
    trk64, trk_cpu, trk_gpu = TL.make_tracker(case).double(), TL.make_tracker(case), TL.make_tracker(case).cuda()
    fused = FusedTracker(trk_gpu)
    with torch.no_grad():
        base = {"f64": trk64.prepare(q.double(), fmaps.double()), "cpu": trk_cpu.prepare(q, fmaps), "gpu": trk_gpu.prepare(q.cuda(), fmaps.cuda())}
        hip = fused.begin(q.cuda(), fmaps.cuda())
    for i, (c64, f64) in enumerate(states):
        c32, f32 = c64.float(), f64.float()                       # the state every path steps from
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


def run_errors(case, got_preds, got_vis, got_conf):
    """Per iteration e_hip against the layout in fp64 and the bound 4 max(e_torch_gpu, e_torch_cpu, 2^-23 max|coords|); the same for vis / conf (floor:
    2^-23, they are at most 1)."""
    _, p64, v64, c64 = truth(case)
    cpu, gpu = layout_run(case, "cpu"), layout_run(case, "cuda")
    rows = []
    for i in range(TL.ITERS):
        e = [float((t[0][i].cpu().double() - p64[i]).abs().max()) for t in ((got_preds,), cpu, gpu)]
        rows.append((f"coords after iteration {i + 1} (px)", e[0], 4 * max(e[1], e[2], ULP * float(p64[i].abs().max())), e[1], e[2]))
    for name, k, t64, got in (("vis", 1, v64, got_vis), ("conf", 2, c64, got_conf)):
        e = [float((t.cpu().double() - t64).abs().max()) for t in (got, cpu[k], gpu[k])]
        rows.append((name, e[0], 4 * max(e[1], e[2], ULP), e[1], e[2]))
    return rows, cpu, gpu


@pytest.mark.parametrize("case", list(TL.CASES))
def test_whole_run_against_fixture_and_fp64(case):
    from gd_amd.teacher_tracker import FusedTracker
    g = load_golden("g28_vggt_tracker")
    q, fmaps = TL.seeded_inputs(case)
    fused = FusedTracker(TL.make_tracker(case).cuda())
    preds, vis, conf = fused(q.cuda(), fmaps.cuda(), iters=TL.ITERS)
    c = TL.CASES[case]
    assert len(preds) == TL.ITERS and preds[0].shape == (c["B"], c["S"], c["N"], 2) and vis.shape == conf.shape == (c["B"], c["S"], c["N"])
    rows, cpu, gpu = run_errors(case, preds, vis, conf)
    for row in rows:
        print(f"case {case} {row[0]}: e_hip {row[1]:.3e}, e_torch_cpu {row[3]:.3e}, e_torch_gpu {row[4]:.3e}, bound 4 max(e_torch_gpu, e_torch_cpu, ulp) = {row[2]:.3e}")
    for row in rows:
        assert row[1] <= row[2], row[0]
    # the reference's own fp32 run (G28) is one of the torch paths' kind: the fused run sits within its own bound plus that run's error of it
    _, p64, v64, c64 = truth(case)
    for name, got, want, t64, bound in (("coords", torch.stack(preds), g[f"{case}_coords"], torch.stack(p64), rows[TL.ITERS - 1][2]),
                                        ("vis", vis, g[f"{case}_vis"], v64, rows[TL.ITERS][2]), ("conf", conf, g[f"{case}_conf"], c64, rows[TL.ITERS + 1][2])):
        e, e_ref = float((got.cpu() - want).abs().max()), float((want.double() - t64).abs().max())
        print(f"case {case} {name}: against the reference's fp32 run (G28) {e:.3e}; that run is {e_ref:.3e} from fp64")
        assert e <= bound + e_ref, name
    # the first iteration's window samples against the reference's own
    st = fused.begin(q.cuda(), fmaps.cuda())
    fused.step(st)
    n = g[f"{case}_corr"].shape[-1]
    e = float((st.corr.view(c["B"], c["S"], c["N"], -1)[..., :n].cpu() - g[f"{case}_corr"]).abs().max()) / float(g[f"{case}_corr"].abs().max())
    print(f"case {case} corr of iteration 1 against the reference's: {e:.3e} of the maximum (the reference's fp32 volume form is ~1e-5 from fp64)")
    assert e <= 1e-4


def test_whole_run_options_and_channel_last_input():
    from gd_amd.teacher_tracker import FusedTracker
    case = "a"
    q, fmaps = TL.seeded_inputs(case)
    fused = FusedTracker(TL.make_tracker(case).cuda())
    kw = dict(iters=TL.ITERS, return_feat=True, down_ratio=2, apply_sigmoid=False)
    preds, vis, feats, qfeat, conf = fused(q.cuda(), fmaps.cuda(), **kw)
    runs = {}
    for name, dev, dt in (("f64", "cpu", torch.float64), ("cpu", "cpu", torch.float32), ("gpu", "cuda", torch.float32)):
        with torch.no_grad():
            runs[name] = TL.make_tracker(case).to(dev, dt)(q.to(dev, dt), fmaps.to(dev, dt), **kw)
    flat = lambda r: [r[0][-1], r[1], r[2], r[3], r[4]]
    t64 = flat(runs["f64"])
    for name, got, w64, c32, g32 in zip(("coords", "vis (logits)", "track_feats", "query_track_feat", "conf (logits)"), flat((preds, vis, feats, qfeat, conf)),
                                        t64, flat(runs["cpu"]), flat(runs["gpu"])):
        e = [float((t.cpu().double() - w64).abs().max()) for t in (got, c32, g32)]
        bound = 4 * max(e[1], e[2], ULP * float(w64.abs().max()))
        print(f"options run, {name}: e_hip {e[0]:.3e}, e_torch_cpu {e[1]:.3e}, e_torch_gpu {e[2]:.3e}, bound {bound:.3e}")
        assert got.shape == w64.shape and e[0] <= bound, name
    # down_ratio scales the prediction: frame 0 is the query at image scale
    assert float((preds[-1][:, 0].cpu() - q).abs().max()) <= 4 * ULP * float(q.abs().max())
    # the channel-last inputs, dense and pitched with a poisoned separator column, give the same numbers as NCHW
    B, S, C, H, W = fmaps.shape
    cl = fmaps.permute(0, 1, 3, 4, 2).contiguous().cuda()
    buf = R64.pitched(cl.view(B * S, H, W, C)).view(B, S, H, W + 1, C)
    odd = torch.as_strided(cl, cl.shape, (7,) + cl.stride()[1:])             # B = 1: the batch stride is arbitrary
    for name, t, pitch in (("dense", cl, None), ("pitched", buf[:, :, :, :W], W + 1), ("pitched, pitch from the strides", buf[:, :, :, :W], None),
                           ("dense, arbitrary stride on the size-1 batch dimension", odd, None)):
        p2, v2, f2, q2, c2 = fused(q.cuda(), iters=TL.ITERS, return_feat=True, down_ratio=2, apply_sigmoid=False, fmaps_cl=t, pitch=pitch)
        assert all(torch.equal(a, b) for a, b in zip(p2, preds)) and torch.equal(v2, vis) and torch.equal(c2, conf) and torch.equal(f2, feats) and torch.equal(q2, qfeat), name
    # a tracker read while the module was still on the host follows the feature map to the GPU on its first call
    host = TL.make_tracker(case)
    late = FusedTracker(host)
    host.cuda()
    p3, v3, c3 = late(q.cuda(), fmaps.cuda(), iters=TL.ITERS, down_ratio=2, apply_sigmoid=False)
    assert all(torch.equal(a, b) for a, b in zip(p3, preds)) and torch.equal(v3, vis) and torch.equal(c3, conf)
    from gd_amd._lib import GdHipError
    with pytest.raises(GdHipError, match="not both"):
        fused(q.cuda(), fmaps.cuda(), fmaps_cl=cl)
    with pytest.raises(GdHipError, match="level 1 of a 3 x 35 map is 1 x 17"):
        fused(q.cuda(), fmaps[:, :, :, :3].cuda())


# ----------------------------------------------------------------------------------------------------------------------------------
# 6. the runner
# ----------------------------------------------------------------------------------------------------------------------------------
class Recording:
    """Stands in for runner.tracker: keeps the float tracks of the last call."""

    def __init__(self, inner):
        self.inner, self.last = inner, None

    def __call__(self, *a, **k):
        out = self.inner(*a, **k)
        self.last = out[0][-1].detach().clone()
        return out


@pytest.mark.parametrize("fused_heads", [False, True])
def test_runner_fused_tracker_against_default_path(fused_heads):
    import dpt_layout as DL
    from gd_amd.teacher_runner import VGGTTeacherRunner
    from test_gpu_teacher_blocks import DeviceRope2D
    teacher = TL.make_tiny_vggt()
    rope = DeviceRope2D()
    teacher.aggregator.rope = rope
    for blk in list(teacher.aggregator.frame_blocks) + list(teacher.aggregator.global_blocks):
        blk.attn.rope = rope
    teacher = teacher.cuda()
    own = lambda: {n: set(vars(m)) for n, m in teacher.named_modules() if n.startswith("track_head")}
    before = own()
    # the image seed is chosen for the default path's margin from the integer thresholds, asserted below (seeds 230 .. 249 measured 2.4e-4 .. 2.0e-2 px)
    img = torch.rand(1, 2, 3, DL.TinyVGGT.IMG[0], DL.TinyVGGT.IMG[1], generator=gen(240)).cuda()
    seen = {}
    hooks = [teacher.track_head.feature_extractor.register_forward_hook(lambda m, a, out: seen.__setitem__("fmaps", out.detach().clone())),
             teacher.track_head.register_forward_hook(lambda m, a, out: seen.__setitem__("tracks", out[0][-1].detach().clone())),
             teacher.track_head.register_forward_pre_hook(lambda m, a, k: seen.__setitem__("query", k["query_points"].detach().clone()), with_kwargs=True)]
    runs = {}
    for on in (False, True):
        r = VGGTTeacherRunner(teacher, dtype=torch.float32, pose_decoder=DL.tiny_pose_decoder, fused_heads=fused_heads, fused_tracker=on)
        assert (r.tracker is not None) == on
        if on:
            r.tracker = Recording(r.tracker)
        runs[on] = r.targets(img, num_keypoints=50, min_distance=3, generator=torch.Generator(device="cuda").manual_seed(1))
        if on:
            seen["fused_tracks"] = r.tracker.last
    for h in hooks:
        h.remove()
    a, b = runs[False], runs[True]
    assert a is not None and b is not None and set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape, k
    assert torch.equal(a["kp_1"], b["kp_1"]) and a["kp_1"].shape[0] > 0
    assert torch.equal(a["mask_1"], b["mask_1"]) and torch.equal(a["mask_2"], b["mask_2"])
    # the float tracks of both paths against the layout in fp64 on the default path's own feature map and query points
    trk = teacher.track_head.tracker
    q, fm = seen["query"].float().cpu(), seen["fmaps"].float().cpu()
    with torch.no_grad():
        t64 = TL.make_tiny_vggt().track_head.tracker.double()(q.double(), fm.double(), iters=TL.ITERS)[0][-1]
        t_cpu = TL.make_tiny_vggt().track_head.tracker(q, fm, iters=TL.ITERS)[0][-1]
    assert trk.corr_levels == 3 and fm.shape[-2:] == (21, 35)
    e_gpu, e_cpu = float((seen["tracks"].cpu().double() - t64).abs().max()), float((t_cpu.double() - t64).abs().max())
    e_hip = float((seen["fused_tracks"].cpu().double() - t64).abs().max())
    bound = 4 * max(e_gpu, e_cpu, ULP * float(t64.abs().max()))
    print(f"runner fused_heads={fused_heads}: float tracks e_hip {e_hip:.3e}, e_torch_gpu {e_gpu:.3e}, e_torch_cpu {e_cpu:.3e}, bound {bound:.3e}")
    assert e_hip <= bound
    # the target extraction truncates the tracks to integers and compares them with integer borders: equal whenever the default path's tracks keep
    # more than both paths' distance from every integer
    tr = seen["tracks"][0, 1].double()
    margin = float(torch.minimum(tr - tr.floor(), tr.ceil() - tr).min())
    print(f"runner fused_heads={fused_heads}: the default path's tracks keep {margin:.3e} px from the nearest integer against e_hip + e_torch_gpu = {e_hip + e_gpu:.3e}")
    assert margin > bound + e_gpu
    assert torch.equal(a["kp_2"], b["kp_2"])
    # nothing is left on the user's modules
    assert own() == before
