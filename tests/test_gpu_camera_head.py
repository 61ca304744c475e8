"""GPU: the camera head on the few-row kernels.  gd_rows_attention, gd_adaln_modulate and gd_pose_update per element against the fp64 restatement
and its derived bounds (tests/rows_ref64.py; tests/test_rows_ref_host.py shows on the CPU that each mutant breaks them); teacher_heads.
FusedCameraHead — both tiny configurations, both (B, S), every iteration — against the layout (tests/camera_layout.py) run in fp64 on the same weights,
held to 4 x the error of the layout's own fp32 CPU run (measured here, per output tensor: the factor covers another summation order in about 20
chained linears), and against fixture G30 (the reference's own module) at the tolerance of the G29 whole-embedder test; the bf16-weight mode under the
same rule against the layout with bf16-rounded weights; the runner's switch.  With GD_CAMERA_ERRORS=<file> the measured values are appended there
(profiles/camera_head_errors.txt)."""
import copy
import os

import pytest
import torch

import camera_layout as CL
import dpt_layout as DL
import rows_ref64 as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

G30_TOL = 1e-4                  # of the fixture tensor's largest magnitude: tests/test_gpu_dino_embed.py's whole-embedder tolerance
_LINES = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("GD_CAMERA_ERRORS")
    if path and _LINES:
        with open(path, "a") as f:
            f.write("# tests/test_gpu_camera_head.py\n" + "".join(l + "\n" for l in _LINES))


def note(line):
    print(line)
    _LINES.append(line)


def worst(got, want, bound):
    return float(((got.double().cpu() - want.double()).abs() / bound).max())


def canaried(t, pad=4, rows_around=1):
    """t [R, C] inside a NaN-filled device buffer [R + 2, C + pad] -> (buffer, view)."""
    R_, C = t.shape
    buf = torch.full((R_ + 2 * rows_around, C + pad), float("nan"), device="cuda")
    view = buf[rows_around:rows_around + R_, :C]
    view.copy_(t)
    return buf, view


def only_view_written(buf, view_rows, view_cols):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[1:1 + view_rows, :view_cols] = False
    return bool(torch.isnan(buf[mask]).all())


# ---------------------------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("B,S,H,hd", R.ATTENTION_CASES)
@pytest.mark.parametrize("huge", [False, True], ids=["plain", "huge_keys_in_the_last_entry"])
def test_rows_attention_per_element_against_fp64(B, S, H, hd, huge):
    from gd_amd import ops
    W = H * hd
    qkv = R.attention_inputs(B, S, H, hd, pad=0, huge_entry=B - 1 if huge else None)
    want, bound = R.attention64(qkv, B, S, H, hd)
    qbuf, q = canaried(qkv, pad=8)                                            # a row stride above 3 H hd
    obuf, o = canaried(torch.zeros(B * S, W), pad=4)
    o.fill_(float("nan"))
    before = qbuf.view(torch.int32).clone()
    got = ops.rows_attention(q, B, S, H, out=o)
    torch.cuda.synchronize()
    r = worst(got, want, bound)
    note(f"{r:8.4f}  rows_attention[B{B}-S{S}-H{H}-hd{hd}{'-huge' if huge else ''}] worst err / bound")
    assert r <= 1.0 and torch.equal(qbuf.view(torch.int32), before) and only_view_written(obuf, B * S, W)
    if B > 1 and huge:
        # the probe: with the last entry's keys 64 x as large, an output row of another entry that had seen them would be that entry's v
        crossed, _ = R.attention64(qkv, B, S, H, hd, mutant="attention_across_entries")
        assert worst(crossed[:S], want[:S], bound[:S]) >= 4.0
    assert torch.equal(ops.rows_attention(q, B, S, H), got)                   # a new contiguous output: the same bits


@pytest.mark.parametrize("M,D", R.ADALN_CASES)
def test_adaln_modulate_per_element_against_fp64(M, D):
    from gd_amd import ops
    x, mod = R.adaln_inputs(M, D)
    want, bound = R.adaln64(x, mod)
    xbuf, xv = canaried(x)
    mbuf, mv = canaried(mod)
    obuf, o = canaried(torch.zeros(M, D))
    o.fill_(float("nan"))
    before = (xbuf.view(torch.int32).clone(), mbuf.view(torch.int32).clone())
    got = ops.adaln_modulate(xv, mv, 1e-6, out=o)
    torch.cuda.synchronize()
    r = worst(got, want, bound)
    note(f"{r:8.4f}  adaln_modulate[M{M}-D{D}] worst err / bound")
    assert r <= 1.0 and only_view_written(obuf, M, D)
    assert torch.equal(xbuf.view(torch.int32), before[0]) and torch.equal(mbuf.view(torch.int32), before[1])


def test_adaln_modulate_at_the_widest_row():
    from gd_amd import ops
    x, mod = R.adaln_inputs(1, 8192)
    want, bound = R.adaln64(x, mod)
    r = worst(ops.adaln_modulate(x.cuda(), mod.cuda()), want, bound)
    note(f"{r:8.4f}  adaln_modulate[M1-D8192] worst err / bound")
    assert r <= 1.0


@pytest.mark.parametrize("first,acts", R.POSE_CASES, ids=lambda v: "-".join(v) if isinstance(v, tuple) else ("first" if v else "later"))
def test_pose_update_against_fp64(first, acts):
    from gd_amd import ops
    delta, raw = R.pose_inputs(first, acts)
    want = R.pose64(delta, raw, first, acts, R.POSE_HW)
    M = delta.shape[0]
    dbuf, dv = canaried(delta, pad=3)                                         # delta as the pose branch leaves it: 9 columns in rows of 12
    rawd = raw.cuda() if not first else torch.full((M, 12), float("nan"), device="cuda")      # a first iteration reads nothing of raw
    enc, E, K = ops.pose_update(dv, rawd, first, acts, R.POSE_HW)
    torch.cuda.synchronize()
    got = dict(raw=rawd.cpu(), enc=enc.cpu(), extrinsic=E.cpu(), intrinsic=K.cpu())
    r = R.pose_ratio(got, want)
    note(f"{r:8.4f}  pose_update[{'first' if first else 'later'}-{'-'.join(acts)}] worst err / bound (fx, fy: {R.FOCAL_REL / R.U:.0f} u relative)")
    assert r <= 1.0
    assert float(got["raw"][:, 9:].abs().max()) == 0.0                        # the pad columns stay 0
    assert not bool(torch.isnan(got["intrinsic"]).any()) and not bool(torch.isnan(got["extrinsic"]).any())
    if acts[2] == "relu":                                                     # row 0's raw fov_h is negative: an exact 0, +inf as the restatement's
        assert float(got["raw"][0, 7]) < 0 and float(got["enc"][0, 7]) == 0.0
        assert bool(torch.isposinf(got["intrinsic"][0, 1, 1])) and bool(torch.isposinf(want["intrinsic"][0, 1, 1]))
    # without the matrices: the same encoding, nothing else
    raw2 = raw.cuda() if not first else torch.zeros(M, 12, device="cuda")
    assert torch.equal(ops.pose_update(dv, raw2, first, acts).cpu(), got["enc"]) and torch.equal(raw2.cpu(), got["raw"])


# ---------------------------------------------------------------------------------------------------------------------------------- the whole head
@pytest.fixture(scope="module")
def g30():
    return load_golden("g30_camera_head")


def max_abs(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def layout_outputs(head, toks):
    """Every iteration's (enc, extrinsic, intrinsic) of a layout module, in its own dtype, on the host."""
    with torch.no_grad():
        encs = head(toks)
    return [(e,) + CL.decode_pose(e, CL.IMAGE_HW) for e in encs]


def fused_outputs(fused, toks):
    """The same from FusedCameraHead: the matrices of iteration k are those of a k-iteration call; its encodings are the 4-iteration call's, bit for bit."""
    dev = [t.cuda() for t in toks]
    encs = fused.forward(dev)
    out = []
    for k in range(1, 5):
        e, E, K = fused.poses(dev, CL.IMAGE_HW, num_iterations=k)
        assert len(e) == k and all(torch.equal(a, b) for a, b in zip(e, encs))
        out.append((encs[k - 1], E, K))
    return out


def bf16_rounded(head):
    """The layout with the weights FusedCameraHead(dtype=bfloat16) narrows — the trunk's and the modulation's linears — rounded to bf16."""
    m = copy.deepcopy(head)
    with torch.no_grad():
        for lin in [m.poseLN_modulation[1]] + [l for b in m.trunk for l in (b.attn.qkv, b.attn.proj, b.mlp.fc1, b.mlp.fc2)]:
            lin.weight.copy_(lin.weight.bfloat16().float())
    return m


@pytest.mark.parametrize("cfg", list(CL.CONFIGS))
@pytest.mark.parametrize("B,S", CL.SHAPES)
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_whole_head_against_the_layout_in_fp64(g30, cfg, B, S, mode):
    from gd_amd.teacher_heads import FusedCameraHead
    head = CL.make_head(cfg)
    toks = CL.seeded_tokens(cfg, B, S)
    yard = head if mode == "f32" else bf16_rounded(head)
    want = layout_outputs(copy.deepcopy(yard).double(), [t.double() for t in toks])
    cpu32 = layout_outputs(yard, toks)
    fused = FusedCameraHead(head, dtype=torch.float32 if mode == "f32" else torch.bfloat16)
    got = fused_outputs(fused, toks)
    ref32 = layout_outputs(copy.deepcopy(head).double(), [t.double() for t in toks]) if mode == "bf16" else None
    bad = []
    for it in range(4):
        for j, what in enumerate(("enc", "extrinsic", "intrinsic")):
            assert got[it][j].shape == want[it][j].shape and got[it][j].dtype == torch.float32 and bool(torch.isfinite(got[it][j]).all())
            e_hip, e_cpu = max_abs(got[it][j], want[it][j]), max_abs(cpu32[it][j], want[it][j])
            line = f"whole head {cfg} {B}x{S} {mode} iteration {it} {what}: fused vs fp64 {e_hip:.3e}, layout fp32 CPU vs fp64 {e_cpu:.3e}, ratio {e_hip / max(e_cpu, 1e-300):.2f}"
            if mode == "bf16":
                line += f", distance from the fp32-weight layout (fp64) {max_abs(got[it][j], ref32[it][j]):.3e} of {float(ref32[it][j].abs().max()):.3e}"
            note(line)
            if e_hip > 4 * e_cpu:
                bad.append((it, what, e_hip, e_cpu))
            if mode == "f32":
                ref = g30[f"{cfg}_{B}x{S}_{what}_{it}"]
                e, bound = max_abs(got[it][j], ref), G30_TOL * float(ref.abs().max())
                note(f"whole head {cfg} {B}x{S} f32 iteration {it} {what}: against G30 {e:.3e}, bound {bound:.3e}")
                assert e <= bound, (it, what)
    assert not bad, bad
    # launches: one token_norm, then 7 + 7 depth per iteration
    depth = CL.CONFIGS[cfg]["trunk_depth"]
    fused.launches = 0
    fused.forward([t.cuda() for t in toks])
    assert fused.launches == 1 + 4 * (7 + 7 * depth)


def test_whole_head_reads_bf16_and_strided_tokens_in_place_and_reuses_its_workspace():
    from gd_amd._lib import GdHipError
    from gd_amd.teacher_heads import FusedCameraHead
    head = CL.make_head("d64")
    fused = FusedCameraHead(head)
    toks = CL.seeded_tokens("d64", 2, 3)[-1]
    want = fused.forward([toks.cuda()])
    ws = fused._ws[6]
    wide = torch.full((2, 3, 4, 72), float("nan"), device="cuda")            # the same tokens as a view of wider rows
    wide[..., :64] = toks.cuda()
    again = fused.forward([wide[..., :64]])
    assert all(torch.equal(a, b) for a, b in zip(again, want)) and fused._ws[6] is ws and again[0].data_ptr() != want[0].data_ptr()
    low = fused.forward([toks.bfloat16().cuda()])
    exact = fused.forward([toks.bfloat16().float().cuda()])
    assert all(torch.equal(a, b) for a, b in zip(low, exact))                # bf16 tokens are widened by the token norm's load, nothing else
    with pytest.raises(GdHipError, match="B \\* S = 3 \\* 3 = 9 camera rows"):
        fused.poses([torch.zeros(3, 3, 2, 64, device="cuda")], CL.IMAGE_HW)
    with pytest.raises(GdHipError, match="one row stride"):
        fused.forward([wide[:, :, :, 1:65]])


# ---------------------------------------------------------------------------------------------------------------------------------- the runner
@pytest.fixture(scope="module")
def teacher():
    from test_gpu_teacher_blocks import DeviceRope2D
    t = DL.TinyVGGT()
    rope = DeviceRope2D()
    t.aggregator.rope = rope
    for blk in list(t.aggregator.frame_blocks) + list(t.aggregator.global_blocks):
        blk.attn.rope = rope
    t = t.cuda()
    return CL.attach_camera_head(t, CL.make_head("d256").cuda())


def _img():
    return torch.rand(1, 2, 3, DL.TinyVGGT.IMG[0], DL.TinyVGGT.IMG[1], generator=torch.Generator().manual_seed(234)).cuda()


def test_runner_cameras_fused_against_the_default_runner(teacher, monkeypatch):
    import gd_amd  # noqa: F401
    from gd_amd import teacher_heads
    from gd_amd.teacher_runner import VGGTTeacherRunner
    img, hw = _img(), DL.TinyVGGT.IMG
    head = teacher.camera_head
    built, calls, decoded = [], [], []
    init = teacher_heads.FusedCameraHead.__init__
    monkeypatch.setattr(teacher_heads.FusedCameraHead, "__init__", lambda self, *a, **k: built.append(1) or init(self, *a, **k))
    hook = head.register_forward_hook(lambda mod, a, out: calls.append(1))

    def dec(enc, image_hw):
        decoded.append(enc)
        return CL.decode_pose(enc, image_hw)
    try:
        off = VGGTTeacherRunner(teacher, dtype=torch.float32, pose_decoder=dec)
        tokens_list, _, _ = off.aggregate(img)
        E0, K0 = off.cameras(tokens_list, hw)
        assert calls == [1] and built == [] and len(decoded) == 1 and off.camera is None     # the module ran once, no fused head was built
        on = VGGTTeacherRunner(teacher, dtype=torch.float32, fused_camera_head=True)
        E1, K1 = on.cameras(tokens_list, hw)
        assert calls == [1] and built == [1] and len(decoded) == 1                            # neither the module nor a decoder ran
        user = VGGTTeacherRunner(teacher, dtype=torch.float32, fused_camera_head=True, pose_decoder=dec)
        E2, K2 = user.cameras(tokens_list, hw)
        assert calls == [1] and len(decoded) == 2                                             # the user's decoder is honoured, on the fused encoding
        assert torch.equal(decoded[1], on.camera.forward(tokens_list)[-1])
    finally:
        hook.remove()
    toks = [tokens_list[-1].float().cpu()]
    cpu = copy.deepcopy(head).cpu()
    want = layout_outputs(copy.deepcopy(cpu).double(), [t.double() for t in toks])[-1]
    cpu32 = layout_outputs(cpu, toks)[-1]
    for what, w, c, default, fused, through in (("extrinsic", want[1], cpu32[1], E0, E1, E2), ("intrinsic", want[2], cpu32[2], K0, K1, K2)):
        e_hip, e_cpu, e_def, e_dec = max_abs(fused, w), max_abs(c, w), max_abs(default, w), max_abs(through, w)
        note(f"runner cameras() {what}: fused vs fp64 {e_hip:.3e}, through the user's decoder {e_dec:.3e}, layout fp32 CPU vs fp64 {e_cpu:.3e}, "
             f"default runner (torch on the GPU) vs fp64 {e_def:.3e}")
        assert fused.shape == default.shape == w.shape and fused.dtype == torch.float32
        assert e_hip <= 4 * e_cpu and e_dec <= 4 * e_cpu, what


def test_runner_targets_with_the_switch_on_has_the_keys_and_shapes_of_the_default(teacher):
    import gd_amd  # noqa: F401
    from gd_amd.teacher_runner import VGGTTeacherRunner
    img = _img()
    calls = []
    hook = teacher.camera_head.register_forward_hook(lambda mod, a, out: calls.append(1))
    try:
        runs = {}
        for fused in (False, True):
            r = VGGTTeacherRunner(teacher, dtype=torch.float32, pose_decoder=None if fused else CL.decode_pose, fused_camera_head=fused)
            runs[fused] = r.targets(img, num_keypoints=50, min_distance=3, generator=torch.Generator(device="cuda").manual_seed(1))
            assert len(calls) == 1                                            # once with the switch off, never with it on
    finally:
        hook.remove()
    a, b = runs[False], runs[True]
    assert a is not None and b is not None and set(a) == set(b)
    per_keypoint = ("kp_1", "kp_2", "pts3d_1", "pts3d_2")                      # the keypoint choice is discrete: only the rows may differ in number
    for k in a:
        assert a[k].dtype == b[k].dtype and (a[k].shape[1:] == b[k].shape[1:] if k in per_keypoint else a[k].shape == b[k].shape), k
    assert a["kp_1"].shape[0] > 0 and b["kp_1"].shape[0] > 0
