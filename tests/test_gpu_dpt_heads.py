"""GPU: the VGGT teacher's dense-prediction heads on the HIP kernels — the kernels of csrc/dpt.hip against fp64, teacher_heads.FusedDPTHead against
fixture G26 (what the reference's own DPTHead returned) and against the module tree of tests/dpt_layout.py, and VGGTTeacherRunner with fused_heads
against its own default path.

Every test prints its measured error beside the bound before it asserts.

Measured on an MI355X (rel. to max |want|): whole head f32 against G26 6.7e-7 .. 1.2e-6 on every output and pre-activation map (bound 1e-4); bf16 operands 2.6e-3 .. 1.8e-2 against 5.6e-3 .. 3.1e-2 for the same modules under
torch.autocast(bfloat16), e_hip / e_ref 0.32 .. 0.56 (rule: at most 2); runner, fused against default heads: depth, tracker features and point_conf
within 1e-6, keypoints equal at an NMS margin of 1.1e-3 against the 4.8e-4 the bound asks for."""
import functools

import pytest
import torch
import torch.nn.functional as F

import dpt_layout as DL
from conftest import load_golden, rel_err
from test_teacher_runner_ref import fill_params

pytestmark = pytest.mark.gpu

KERNEL_TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2}          # the project's kernel bounds per output type (tests/test_gpu_rope.py, test_gpu_mast3r_blocks.py)
HEAD_TOL = 1e-4                                                   # test_whole_stack_f32_against_reference_fixture's bound, relative to max |want|
C = 8                                                             # the narrowest row a bf16 operand allows (16 bytes)


def pitched(x, dtype=torch.float32):
    """x [frames, h, w, c] (host) -> the separator-column grid [frames*h*(w+1), c] on the device; separators hold NaN: a kernel that reads one shows it."""
    f, h, w, c = x.shape
    g = torch.full((f, h, w + 1, c), float("nan"))
    g[:, :, :w] = x
    return g.reshape(f * h * (w + 1), c).to(dtype).cuda()


def unpitched(g, f, h, w):
    """device grid -> (pixels [f, h, w, c], separators [f, h, c]) on the host."""
    g = g.float().cpu().view(f, h, w + 1, -1)
    return g[:, :, :w], g[:, :, w]


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. gd_grid_resample
# ----------------------------------------------------------------------------------------------------------------------------------
RESAMPLE = {"2x3->3x5": ((2, 3), (3, 5), False), "3x5->3x5": ((3, 5), (3, 5), False), "12x20->21x35+tables+addend": ((12, 20), (21, 35), True),
            "1x4->1x7": ((1, 4), (1, 7), False)}


@pytest.mark.parametrize("src_dtype", [torch.float32, torch.bfloat16], ids=["src_f32", "src_bf16"])
@pytest.mark.parametrize("case", list(RESAMPLE))
def test_grid_resample_against_fp64(case, src_dtype):
    from gd_amd import ops
    (sh, sw), (dh, dw), extras = RESAMPLE[case]
    x = randn(2, sh, sw, C, seed=sh * 100 + sw).to(src_dtype).float()            # two frames of different content, exactly representable in the source type
    add = px = py = None
    want = F.interpolate(x.double().permute(0, 3, 1, 2), size=(dh, dw), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    if extras:
        add, px, py = randn(2, dh, dw, C, seed=1), randn(dw, C // 2, seed=2), randn(dh, C // 2, seed=3)
        want = want + add.double()
        want[..., :C // 2] += px.double()[None, None]
        want[..., C // 2:] += py.double()[None, :, None]
    kw = dict(addend=pitched(add) if extras else None, px=px.cuda() if extras else None, py=py.cuda() if extras else None)
    src = pitched(x, src_dtype)
    plain = ops.grid_resample(src, 2, sh, sw, dh, dw, C, **kw)
    got, sep = unpitched(plain, 2, dh, dw)
    e = rel_err(got, want)
    print(f"grid_resample {case} {src_dtype}: rel err {e:.3e} (bound {KERNEL_TOL[torch.float32]:.0e})")
    assert plain.dtype == torch.float32 and e <= KERNEL_TOL[torch.float32]
    assert torch.count_nonzero(sep) == 0                                          # separators written as zero (and no NaN read from the source's)
    if (sh, sw) == (dh, dw) and not extras:
        assert torch.equal(got, x)                                                # the identity is a copy, bit for bit
    rows = 2 * dh * (dw + 1)
    st32 = ops.grid_resample(src, 2, sh, sw, dh, dw, C, stacked=torch.float32, **kw)
    assert torch.equal(st32, ops.stack3_rows(plain, 2, dh, dw, C, dh * (dw + 1) * C, 0, dw + 1, torch.float32))       # the stacked form: bit-equal in f32
    st16 = ops.grid_resample(src, 2, sh, sw, dh, dw, C, stacked=torch.bfloat16, **kw)
    e16 = rel_err(st16, st32)
    print(f"   stacked bf16 against stacked f32: rel err {e16:.3e} (bound {KERNEL_TOL[torch.bfloat16]:.0e})")
    assert st16.shape == (rows + 2, 3 * C) and e16 <= KERNEL_TOL[torch.bfloat16]
    assert not st16[st32 == 0].any() and not st16[0].any() and not st16[-1].any()          # zeros at separators, outside the image and in the guard rows


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_relu_operand_equals_stack3_of_relu(dt):
    from gd_amd import ops
    h, w = 5, 7
    x = randn(2, h, w, C, seed=9)
    grid = pitched(x)
    got = ops.grid_resample(grid, 2, h, w, h, w, C, relu=True, stacked=dt)
    want = ops.stack3_rows(pitched(F.relu(x)), 2, h, w, C, h * (w + 1) * C, 0, w + 1, dt)
    assert bool((x < 0).any()) and torch.equal(got, want)


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. the transposed convolutions and the stride-2 convolution
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("src_pitch_extra", [0, 1], ids=["token_rows", "pitched_rows"])
@pytest.mark.parametrize("k", [4, 2])
def test_deconv_scatter_against_fp64(k, src_pitch_extra, dt):
    from gd_amd import ops
    h, w, cin, cout = 3, 5, 8, 16
    x = randn(2, h, w, cin, seed=k).to(dt).float()
    wt = (randn(cin, cout, k, k, seed=20 + k) / cin ** 0.5).to(dt).float()
    bias = randn(cout, seed=30)
    want = F.conv_transpose2d(x.double().permute(0, 3, 1, 2), wt.double(), bias.double(), stride=k).permute(0, 2, 3, 1)
    a = (pitched(x, dt) if src_pitch_extra else x.reshape(-1, cin).to(dt).cuda())
    a = torch.nan_to_num(a)                                                       # (separator rows enter the GEMM as rows like any other; their outputs are dropped)
    g = ops.gemm_nt(a, wt.permute(2, 3, 1, 0).reshape(k * k * cout, cin).to(dt).cuda().contiguous(), out_dtype=torch.float32)
    out = ops.deconv_scatter(g, bias.cuda(), 2, h, w, w + src_pitch_extra, k, cout)
    got, sep = unpitched(out, 2, h * k, w * k)
    e = rel_err(got, want)
    print(f"deconv_scatter k={k} pitch+{src_pitch_extra} {dt}: rel err {e:.3e} (bound {KERNEL_TOL[torch.float32]:.0e}: exact products of the rounded operands)")
    assert e <= KERNEL_TOL[torch.float32] and torch.count_nonzero(sep) == 0


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("grid", [(3, 5), (4, 4)], ids=["3x5", "4x4"])
def test_stride2_convolution_against_fp64(grid, dt):
    """resize_layers[3]: the full-resolution stacked GEMM, then gd_grid_resample(step=2) — rows and columns 0, 2, 4, ..."""
    from gd_amd import ops
    (h, w), cin, cout = grid, 8, 16
    x = randn(2, h, w, cin, seed=h).to(dt).float()
    wt = (randn(cout, cin, 3, 3, seed=40) / (9 * cin) ** 0.5).to(dt).float()
    bias = randn(cout, seed=41)
    want = F.conv2d(x.double().permute(0, 3, 1, 2), wt.double(), bias.double(), stride=2, padding=1).permute(0, 2, 3, 1)
    oh, ow = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    assert want.shape == (2, oh, ow, cout)
    buf = ops.stack3_rows(x.reshape(2, h * w, cin).cuda(), 2, h, w, cin, h * w * cin, 0, w, dt)        # from token rows, as the head does
    full = ops.gemm_nt(ops.conv_view(buf, 2 * h * (w + 1), cin), wt.permute(0, 3, 2, 1).reshape(cout, 9 * cin).to(dt).cuda().contiguous(),
                       out_dtype=torch.float32, bias=bias.cuda())
    got, sep = unpitched(ops.grid_resample(full, 2, h, w, oh, ow, cout, step=2), 2, oh, ow)
    e = rel_err(got, want)
    print(f"stride-2 conv {h}x{w} {dt}: rel err {e:.3e} (bound {KERNEL_TOL[torch.float32]:.0e}: exact products of the rounded operands)")
    assert e <= KERNEL_TOL[torch.float32] and torch.count_nonzero(sep) == 0
    st = ops.grid_resample(full, 2, h, w, oh, ow, cout, step=2, stacked=torch.float32)
    assert torch.equal(st, ops.stack3_rows(pitched(got), 2, oh, ow, cout, oh * (ow + 1) * cout, 0, ow + 1, torch.float32))


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. gd_dpt_head_out
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conf_act", ["expp1", "expp0", "sigmoid"])
@pytest.mark.parametrize("act", ["exp", "inv_log", "linear", "relu", "sigmoid"])
def test_dpt_head_out_against_fp64(act, conf_act):
    from gd_amd import ops
    f, h, w, cin, od = 2, 9, 13, 32, 2 if act == "exp" else 4
    x = F.relu(randn(f, h, w, cin, seed=5))
    wt, bias = randn(od, cin, seed=6), randn(od, seed=7)
    y = x.double() @ wt.double().T + bias.double()
    s = 4.0 / float(y.abs().max())                                                # logits in [-4, 4]
    wt, bias = (wt.double() * s).float(), (bias.double() * s).float()
    y = x.double() @ wt.double().T + bias.double()
    want_v, want_c = DL.activate(y, act, conf_act)
    preds, conf = ops.dpt_head_out(pitched(x), wt.cuda(), bias.cuda(), f, h, w, act, conf_act)
    assert preds.shape == (f, h, w, od - 1) and conf.shape == (f, h, w) and preds.dtype == conf.dtype == torch.float32
    for what, got, want in (("values", preds, want_v), ("confidence", conf, want_c)):
        e = float(((got.double().cpu() - want).abs() / want.abs().clamp_min(1.0)).max())
        print(f"dpt_head_out {act}/{conf_act} {what}: worst element error {e:.3e} relative (absolute below 1), bound 1e-5")
        assert e <= 1e-5
    if conf_act == "expp1":
        assert float(conf.min()) >= 1.0


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. the whole head
# ----------------------------------------------------------------------------------------------------------------------------------
def outputs(res):
    return {"features": res} if torch.is_tensor(res) else {"preds": res[0], "conf": res[1]}


@functools.lru_cache(maxsize=None)
def layout64(case, inplace=True):
    """The layout's own fp64 run of a fixture case: ({output name: tensor}, pre-activation map), computed once."""
    m = DL.make_head(case, inplace_relu=inplace)
    fill_params(m)
    toks, img = DL.seeded_inputs(case)
    taps = {}
    with torch.no_grad():
        res = m.double()([t.double() for t in toks], img.double(), DL.PREFIX, taps=taps)
    return outputs(res), taps["pre"]


def fused_run(case, dtype, chunk=None, inplace=True):
    from gd_amd.teacher_heads import FusedDPTHead
    m = DL.make_head(case, inplace_relu=inplace)
    fill_params(m)
    toks, img = DL.seeded_inputs(case)
    taps = {}
    res = FusedDPTHead(m.cuda(), dtype=dtype).forward([t.cuda() for t in toks], img.cuda(), DL.PREFIX, frames_chunk_size=chunk, taps=taps)
    return outputs(res), taps["pre"]


@pytest.mark.parametrize("case", list(DL.CASES))
def test_whole_head_f32_against_reference_fixture(case):
    g = load_golden("g26_dpt_head")
    got, pre = fused_run(case, torch.float32)
    for name, t in list(got.items()) + [("pre", pre)]:
        want = g[f"{case}_{name}"]
        e = rel_err(t, want)
        print(f"case {case} {name}: rel err {e:.3e} against the reference's head (bound {HEAD_TOL:.0e})")
        assert t.shape == want.shape and t.dtype == want.dtype == torch.float32 and t.is_cuda
        assert e <= HEAD_TOL
    one, pre1 = fused_run(case, torch.float32, chunk=1)
    assert all(torch.equal(one[k], got[k]) for k in got) and torch.equal(pre1, pre)          # chunking over frames changes nothing


def test_whole_head_f32_out_of_place_relu():
    """Residual units whose ReLU is NOT in place keep the un-rectified input for the skip: the ReLU then rides in the operand producer."""
    want, want_pre = layout64("a", inplace=False)
    base, _ = layout64("a")
    got, pre = fused_run("a", torch.float32, inplace=False)
    assert rel_err(base["preds"], want["preds"]) > 1e-2                                      # the two variants are different functions
    for name, t, w in [(k, got[k], want[k]) for k in got] + [("pre", pre, want_pre)]:
        e = rel_err(t, w)
        print(f"out-of-place ReLU, {name}: rel err {e:.3e} against the layout in fp64 (bound {HEAD_TOL:.0e})")
        assert e <= HEAD_TOL


@pytest.mark.parametrize("case", list(DL.CASES))
def test_whole_head_bf16_in_the_precision_class_of_autocast(case):
    want, want_pre = layout64(case)
    got, pre = fused_run(case, torch.bfloat16)
    m = DL.make_head(case)
    fill_params(m)
    toks, img = DL.seeded_inputs(case)
    taps = {}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ref = outputs(m.cuda()([t.cuda() for t in toks], img.cuda(), DL.PREFIX, taps=taps))
    pairs = {name: (rel_err(ref[name].float(), want[name]), rel_err(got[name], want[name])) for name in want}
    pairs["pre"] = (rel_err(taps["pre"].float(), want_pre), rel_err(pre, want_pre))
    for name, (e_ref, e_hip) in pairs.items():
        print(f"bf16 case {case} {name}: e_ref (torch autocast) {e_ref:.4e}, e_hip (fused) {e_hip:.4e}")
    for name, (e_ref, e_hip) in pairs.items():
        assert e_hip <= 2 * e_ref, name


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. the runner
# ----------------------------------------------------------------------------------------------------------------------------------
def nms_margin(conf, mask, r):
    """How far the confidence map is from changing its set of masked local maxima: for a maximum the gap to the runner-up of its window, for every
    other pixel the gap to its window's maximum; the smallest over the masked pixels."""
    s = torch.where(mask, conf, torch.zeros_like(conf))[None, None]
    k = 2 * r + 1
    win = F.unfold(F.pad(s, (r, r, r, r), value=float("-inf")), k).view(k * k, -1)              # [window, pixels]
    top = win.topk(2, dim=0).values
    flat = s.reshape(-1)
    gap = torch.where(flat >= top[0], top[0] - top[1], top[0] - flat)
    return float(gap[mask.reshape(-1)].min())


def test_runner_fused_heads_against_default_path():
    import gd_amd  # noqa: F401
    from gd_amd.teacher_runner import VGGTTeacherRunner
    from test_gpu_teacher_blocks import DeviceRope2D
    teacher = DL.TinyVGGT()
    rope = DeviceRope2D()                    # (the layout's own RoPE module builds its table on the host)
    teacher.aggregator.rope = rope
    for blk in list(teacher.aggregator.frame_blocks) + list(teacher.aggregator.global_blocks):
        blk.attn.rope = rope
    teacher = teacher.cuda()
    # the image seed is chosen for the default path's NMS margin, asserted below
    img = torch.rand(1, 2, 3, DL.TinyVGGT.IMG[0], DL.TinyVGGT.IMG[1], generator=torch.Generator().manual_seed(234)).cuda()
    runs = {}
    for fused in (False, True):
        r = VGGTTeacherRunner(teacher, dtype=torch.float32, pose_decoder=DL.tiny_pose_decoder, fused_heads=fused)
        assert (r.heads is not None) == fused
        runs[fused] = (r.targets(img, num_keypoints=50, min_distance=3, generator=torch.Generator(device="cuda").manual_seed(1)),
                       teacher.track_head.last_features)
        assert "forward" not in vars(teacher.track_head.feature_extractor)
    (a, fa), (b, fb) = runs[False], runs[True]
    assert a is not None and b is not None and set(a) == set(b)
    for k in ("depth_1", "depth_2"):
        e = rel_err(b[k], a[k])
        print(f"runner {k}: fused against default rel err {e:.3e} (bound {HEAD_TOL:.0e})")
        assert b[k].shape == a[k].shape and e <= HEAD_TOL
    e = rel_err(fb, fa)
    print(f"runner tracker features: rel err {e:.3e} (bound {HEAD_TOL:.0e})")
    assert fb.shape == fa.shape and e <= HEAD_TOL
    # the keypoints follow the confidence ranking: equal whenever the default path's ranking has a margin above the bound
    tokens_list, ps_idx, _ = r.aggregate(img)
    with torch.no_grad():
        conf_a, conf_b = teacher.point_head(tokens_list, img, ps_idx)[1], r.heads["point_head"](tokens_list, img, ps_idx)[1]
    e = rel_err(conf_b, conf_a)
    margin = nms_margin(conf_a[0, 0], a["mask_1"], 3)
    print(f"runner point_conf: rel err {e:.3e} (bound {HEAD_TOL:.0e}); NMS margin of the default path {margin:.3e} against 2 x bound x max = "
          f"{2 * HEAD_TOL * float(conf_a.abs().max()):.3e}")
    assert e <= HEAD_TOL
    assert margin > 2 * HEAD_TOL * float(conf_a.abs().max())
    assert torch.equal(a["mask_1"], b["mask_1"]) and torch.equal(a["mask_2"], b["mask_2"])
    for k in a:
        assert a[k].shape == b[k].shape, k
    assert torch.equal(a["kp_1"], b["kp_1"]) and torch.equal(a["kp_2"], b["kp_2"]) and a["kp_1"].shape[0] > 0
