"""GPU: the MASt3R teacher's heads on the HIP kernels — gd_mast3r_head_out against fp64 and, bit for bit, against F.pixel_shuffle;
teacher_heads.FusedMASt3RHead against fixture G27 (what the reference's own Cat_MLP_LocalFeatures_DPT_Pts3d returned) and against the module tree of
tests/mast3r_head_layout.py; and MASt3RTeacherRunner with fused_heads against its own default heads.

Every test prints its measured error beside the bound before it asserts.

Measured on an MI355X: the kernel at most 0.056 of its derived bound (1 - 2 ulp where only the activation's rounding counts); the shuffle bit-exact; whole head f32
against G27 5.3e-7 .. 2.9e-6 of max |want| on every output and on the map before the postprocess (bound 1e-4); bf16 operands e_hip / e_ref 0.25 .. 0.94 (rule: at
most 2) at e_hip 3.3e-3 .. 2.6e-2; runner, fused against default heads: keypoints equal, gathered points within 4.6e-6, cost maps equal."""
import functools

import pytest
import torch
import torch.nn.functional as F

import mast3r_head_layout as ML
from conftest import load_golden, rel_err
from test_gpu_dpt_heads import pitched, randn
from test_teacher_runner_ref import fill_params

pytestmark = pytest.mark.gpu

INF = float("inf")
HEAD_TOL = 1e-4             # the project's bound for a whole head against the reference's fixture, relative to max |want| (tests/test_gpu_dpt_heads.py)
LIN_TOL = 1e-5              # gd_dpt_head_out's bound for the 1x1 convolution: per element, relative, absolute below 1 (tests/test_gpu_dpt_heads.py)
ULP = 2.0 ** -23
TGT_TOL = 2e-6              # tests/test_gpu_mast3r_blocks.py: the bound of the target maps, which the heads do not touch

# ----------------------------------------------------------------------------------------------------------------------------------
# 1. gd_mast3r_head_out against fp64
# ----------------------------------------------------------------------------------------------------------------------------------
# (H, W, P), Cin, od, D, two_confs, pts mode, conf mode, desc_conf mode
SIZES = {"16x32p16": (16, 32, 16), "8x24p8": (8, 24, 8)}
KERNEL_CASES = {
    "teacher": ("16x32p16", 128, 4, 24, 1, "exp", ("exp", 1.0, INF), ("exp", 0.0, INF)),
    "teacher_small_patch": ("8x24p8", 128, 4, 24, 1, "exp", ("exp", 1.0, INF), ("exp", 0.0, INF)),
    "narrow_map": ("16x32p16", 8, 4, 24, 1, "square", ("sigmoid", 0.0, 5.0), ("sigmoid", 1.0, 3.0)),
    "clipped_exp": ("8x24p8", 8, 4, 16, 1, "exp", ("exp", 1.0, 3.0), ("exp", 0.0, 2.0)),
    "one_conf": ("16x32p16", 128, 4, 16, 0, "linear", ("exp", 1.0, INF), ("exp", 0.0, INF)),
    "one_conf_sigmoid": ("8x24p8", 8, 4, 24, 0, "square", ("sigmoid", 0.0, 5.0), ("exp", 0.0, INF)),
    "no_conf": ("8x24p8", 128, 3, 24, 1, "exp", ("exp", 1.0, INF), ("sigmoid", 0.0, 1.0)),
    "no_conf_narrow": ("16x32p16", 8, 3, 16, 1, "linear", ("exp", 1.0, INF), ("exp", 0.0, 20.0)),
    "one_channel": ("16x32p16", 128, 4, 1, 1, "square", ("exp", 0.0, INF), ("exp", 0.0, INF)),
    "one_channel_one_conf": ("8x24p8", 8, 4, 1, 0, "exp", ("exp", 1.0, INF), ("exp", 1.0, INF)),
    "pts_only": ("16x32p16", 128, 4, None, 0, "exp", ("exp", 1.0, INF), None),
    "pts_only_no_conf": ("8x24p8", 8, 3, None, 0, "square", ("exp", 1.0, INF), None),
}


def conf64(y, mode, dy):
    """(value, bound) of a confidence in fp64: f(y) and |f'(y)| dy.  exp: f = vmin + min(e^y, vmax - vmin), Lipschitz with e^y;  sigmoid:
    f' = (vmax - vmin) s (1 - s)."""
    kind, vmin, vmax = mode
    if kind == "exp":
        return vmin + y.exp().clamp(max=vmax - vmin), y.exp() * dy
    s = torch.sigmoid(y)
    return (vmax - vmin) * s + vmin, (vmax - vmin) * s * (1 - s) * dy


def pts64(xyz, mode, dxyz):
    """(value, bound): r = xyz g(d) / d with d = |xyz|, g = d (linear), d^2 (square), expm1(d) (exp).  The Jacobian has the radial eigenvalue g'(d)
    and the tangential one g(d) / d <= g'(d), so |dr|_2 <= g'(d) |dxyz|_2 with g' = 1, 2 d, e^d; every component is held to that."""
    if mode == "linear":
        return xyz, dxyz
    d = xyz.norm(dim=-1, keepdim=True)
    n2 = dxyz.norm(dim=-1, keepdim=True)
    u = xyz / d.clamp(min=1e-8)
    return (u * d.square(), 2 * d * n2) if mode == "square" else (u * torch.expm1(d), d.exp() * n2)


@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_head_out_against_fp64(case):
    """The bound.  The 1x1 convolution's logits y are held as gd_dpt_head_out's are: |dy| <= 1e-5 max(|y|, 1) (LIN_TOL; logits scaled into [-4, 4]).
    An output f(y) is then held to |f'(y)| |dy|, the first-order propagation (functions `conf64`, `pts64`; dy <= 4e-5, so the second-order term
    is below 1e-4 of the first and is covered by the factor 1.01), plus the rounding of evaluating f in float: 16 ulp of |f(y)| (expf, expm1f and the
    division are each within 2 ulp; the rest are a handful of float operations).  The local-feature values reach the kernel as exact floats (no
    linear part), so `desc_conf` carries only that rounding term, and `desc` = v / |v| the rounding of a D-term sum of squares, a square root and
    a division: (D + 16) ulp of |desc|.  A confidence clipped at vmax - vmin is exact there and 1-Lipschitz-continued, so the same bound holds
    across the clip."""
    from gd_amd import ops
    size, cin, od, D, tc, pmode, cmode, dmode = KERNEL_CASES[case]
    (H, W, P), f = SIZES[size], 2
    x = F.relu(randn(f, H, W, cin, seed=cin + od))
    wt, bias = randn(od, cin, seed=6), randn(od, seed=7)
    s = 4.0 / float((x.double() @ wt.double().T + bias.double()).abs().max())                  # logits in [-4, 4]
    wt, bias = (wt.double() * s).float(), (bias.double() * s).float()
    y = x.double() @ wt.double().T + bias.double()
    dy = 1.01 * LIN_TOL * y.abs().clamp_min(1.0)
    want = {"pts3d": pts64(y[..., :3], pmode, dy[..., :3])}
    if od == 4:
        want["conf"] = conf64(y[..., 3], cmode, dy[..., 3])
    lf = None
    if D is not None:
        n, gh, gw = D + tc, H // P, W // P
        lf = 2.0 * randn(f * gh * gw, P * P * n, seed=D + tc)                                   # token rows, columns (i, j, c)
        px = lf.double().view(f, gh, gw, P, P, n).permute(0, 1, 3, 2, 4, 5).reshape(f, H, W, n)
        v = px[..., :D]
        want["desc"] = (v / v.norm(dim=-1, keepdim=True), torch.zeros_like(v))
        want["desc_conf"] = conf64(px[..., D], dmode, torch.zeros(f, H, W, dtype=torch.float64)) if tc else want["conf"]
    got = ops.mast3r_head_out(pitched(x), wt.cuda(), bias.cuda(), None if lf is None else lf.cuda(), f, H, W, patch=P, desc_dim=D or 0, two_confs=bool(tc),
                              pts_mode=pmode, conf_mode=cmode, desc_conf_mode=dmode or ("raw", 0.0, 0.0))
    got = dict(zip(("pts3d", "conf", "desc", "desc_conf"), got))
    assert {k for k, t in got.items() if t is not None} == set(want)
    for name, (w, prop) in want.items():
        g = got[name]
        bound = prop + ((D + 16) if name == "desc" else 16) * ULP * w.abs()
        err = (g.double().cpu() - w).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"head_out {case} {name}: worst |err| {float(err.max()):.3e}, worst err / bound {worst:.3f} (max |want| {float(w.abs().max()):.3g})")
        assert g.dtype == torch.float32 and g.shape == w.shape and torch.isfinite(g).all()
        assert worst <= 1.0, name
    if D is not None and not tc:
        assert torch.equal(got["desc_conf"], got["conf"])                                       # a copy
    if od == 4 and cmode[0] == "exp" and cmode[2] < INF:
        assert float(got["conf"].max()) == cmode[2] and float(got["conf"].min()) > cmode[1]     # the clip is reached, exactly


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. the pixel shuffle is addressing alone
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 2, 3, 16, 24, 1), (2, 3, 2, 8, 16, 1), (3, 3, 5, 2, 32, 1), (2, 1, 2, 16, 16, 0), (2, 2, 2, 1, 7, 1)],
                         ids=["3f_2x3_p16_d24+1", "2f_3x2_p8_d16+1", "3f_3x5_p2_d32+1", "2f_1x2_p16_d16", "2f_2x2_p1_d7+1"])
def test_pixel_shuffle_by_addressing_is_bit_exact(shape):
    """Raw modes.  In the module's order, channel (c P^2 + i P + j) of token (frame, ty, tx) holds a number that encodes all six indices (below 2^24:
    exact in float); F.pixel_shuffle places it at channel c of pixel (ty P + i, tx P + j).  The kernel reads the same numbers from token rows packed
    (i, j, c) and must put every one in the same place — the last frame, token row and token column included."""
    from gd_amd import ops
    from gd_amd.teacher_heads import pack_pixel_shuffle
    f, gh, gw, P, D, tc = shape
    n, H, W = D + tc, gh * P, gw * P
    code = torch.arange(f * gh * gw * n * P * P, dtype=torch.float32).view(f, gh * gw, n * P * P) + 1.0        # [frames, tokens, module-order channels]
    assert code.max() < 2 ** 24
    want = F.pixel_shuffle(code.transpose(-1, -2).reshape(f, n * P * P, gh, gw), P).permute(0, 2, 3, 1)        # [f, H, W, n], as the module shuffles
    rows = pack_pixel_shuffle(code.view(-1, n * P * P).T.contiguous(), P).T.contiguous()                       # the columns in the packed order
    cin = 8
    x, wt, bias = F.relu(randn(f, H, W, cin, seed=1)), randn(4, cin, seed=2), randn(4, seed=3)
    pts, conf, desc, dconf = ops.mast3r_head_out(pitched(x), wt.cuda(), bias.cuda(), rows.cuda(), f, H, W, patch=P, desc_dim=D, two_confs=bool(tc),
                                                 desc_mode="raw")
    assert torch.equal(desc.cpu(), want[..., :D])
    assert torch.equal(dconf.cpu(), want[..., D]) if tc else torch.equal(dconf, conf)
    lin = x.double() @ wt.double().T + bias.double()
    e = float(((torch.cat([pts, conf[..., None]], -1).double().cpu() - lin).abs() / lin.abs().clamp_min(1.0)).max())
    print(f"shuffle {shape}: every local-feature value in place; the raw 1x1 convolution is within {e:.2e} of fp64 (bound {LIN_TOL:.0e})")
    assert e <= LIN_TOL


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. the whole head
# ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layout64(case):
    """The layout's own fp64 run of a fixture case: (outputs, pre-activation map), computed once."""
    m = ML.make_head(case)
    fill_params(m)
    decout, hw = ML.seeded_inputs(case)
    taps = {}
    with torch.no_grad():
        res = m.double()([t.double() for t in decout], hw, taps=taps)
    return res, taps["pre"]


def fused_run(case, dtype):
    from gd_amd.teacher_heads import FusedMASt3RHead
    m = ML.make_head(case)
    fill_params(m)
    decout, hw = ML.seeded_inputs(case)
    taps = {}
    res = FusedMASt3RHead(m.cuda(), dtype=dtype)([t.cuda() for t in decout], hw, taps=taps)
    return res, taps["pre"]


@pytest.mark.parametrize("case", list(ML.CASES))
def test_whole_head_f32_against_reference_fixture(case):
    """Every output and the map before the postprocess against what the reference's head returned, at the project's bound for a whole head,
    1e-4 of max |want| — not widened for the exp-type outputs (measured: the module docstring and DESIGN.md 6d)."""
    g = load_golden("g27_mast3r_head")
    got, pre = fused_run(case, torch.float32)
    assert set(got) == {"pts3d", "desc", "desc_conf"} | ({"conf"} if ML.CASES[case]["has_conf"] else set())
    worst = 0.0
    for name, t in list(got.items()) + [("pre", pre)]:
        want = g[f"{case}_{name}"]
        e = rel_err(t, want)
        worst = max(worst, e)
        print(f"case {case} {name}: rel err {e:.3e} against the reference's head (bound {HEAD_TOL:.0e})")
        assert t.shape == want.shape and t.dtype == want.dtype == torch.float32 and t.is_cuda
        assert e <= HEAD_TOL, name
    print(f"case {case}: worst {worst:.3e}")


def test_frames_of_a_batch_are_independent():
    """Two different frames in one call give what each gives alone (the heads run all frames of a call together)."""
    from gd_amd.teacher_heads import FusedMASt3RHead
    m = ML.make_head("a")
    fill_params(m)
    h = FusedMASt3RHead(m.cuda())
    d0, hw = ML.seeded_inputs("a")
    d1 = [t.flip(1) * 0.5 for t in d0]
    both = h([torch.cat([a, b]).cuda() for a, b in zip(d0, d1)], hw)
    for i, d in enumerate((d0, d1)):
        one = h([t.cuda() for t in d], hw)
        for k in one:
            e = rel_err(both[k][i:i + 1], one[k])
            print(f"frame {i} {k}: in a batch of two against alone, rel err {e:.3e} (bound {HEAD_TOL:.0e})")
            assert both[k].shape[0] == 2 and e <= HEAD_TOL


@pytest.mark.parametrize("case", list(ML.CASES))
def test_whole_head_bf16_in_the_precision_class_of_autocast(case):
    want, want_pre = layout64(case)
    got, pre = fused_run(case, torch.bfloat16)
    m = ML.make_head(case)
    fill_params(m)
    decout, hw = ML.seeded_inputs(case)
    taps = {}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ref = m.cuda()([t.cuda() for t in decout], hw, taps=taps)
    pairs = {name: (rel_err(ref[name].float(), want[name]), rel_err(got[name], want[name])) for name in want}
    pairs["pre"] = (rel_err(taps["pre"].float(), want_pre), rel_err(pre, want_pre))
    for name, (e_ref, e_hip) in pairs.items():
        print(f"bf16 case {case} {name}: e_ref (torch autocast) {e_ref:.4e}, e_hip (fused) {e_hip:.4e}")
    for name, (e_ref, e_hip) in pairs.items():
        assert e_hip <= 2 * e_ref, name


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. the runner
# ----------------------------------------------------------------------------------------------------------------------------------
def _shadows(m):
    return [n for n in ("downstream_head1", "downstream_head2") if "forward" in vars(getattr(m, n))]


@pytest.mark.parametrize("fused_blocks", [False, True], ids=["torch_blocks", "fused_blocks"])
def test_runner_fused_heads_against_default_heads(fused_blocks):
    """The same runner with and without fused heads.  The pair is one image twice and the matcher's two sides carry the same weights
    (mast3r_head_layout.tiny_matcher), so every pixel's reciprocal nearest neighbour is its twin whatever the last bits of the descriptors: the
    keypoints must be equal, the gathered points within the whole-head bound, and the cost maps — which no head touches — the same."""
    from gd_amd.teacher_runner import MASt3RTeacherRunner
    m = ML.tiny_matcher().cuda()
    g = torch.Generator().manual_seed(9)
    img = torch.rand(1, 3, ML.IMG_H, ML.IMG_W, generator=g)
    depth = (torch.rand(ML.IMG_H, ML.IMG_W, generator=g) + 1.0).cuda()
    kw = dict(inference=ML.inference, make_pairs=ML.make_pairs, min_conf_thr=0, subsample=8, fused_blocks=fused_blocks)
    args = dict(temperature=3.0, depth_1=depth, depth_2=depth)
    plain = MASt3RTeacherRunner(m, **kw).targets(img, img, **args)
    runner = MASt3RTeacherRunner(m, fused_heads=True, **kw)
    assert runner.heads is not None and (runner.fused is not None) == fused_blocks
    fused = runner.targets(img, img, **args)
    assert _shadows(m) == [] and all(h.forward.__func__ is ML.MASt3RHeadLayout.forward for h in (m.downstream_head1, m.downstream_head2))
    assert plain is not None and fused is not None and set(plain) == set(fused) and plain["kp_1"].shape[0] > 0
    assert torch.equal(plain["kp_1"], plain["kp_2"])                                           # the twins
    assert torch.equal(plain["kp_1"], fused["kp_1"]) and torch.equal(plain["kp_2"], fused["kp_2"])
    for k in ("pts3d_1", "pts3d_2"):
        e = rel_err(fused[k], plain[k])
        print(f"runner {k} ({plain[k].shape[0]} keypoints): fused against default heads rel err {e:.3e} (bound {HEAD_TOL:.0e})")
        assert fused[k].shape == plain[k].shape and e <= HEAD_TOL
    for k in ("cost_1", "cost_2", "depth_1", "depth_2"):
        e = float((fused[k].double() - plain[k].double()).abs().max())
        print(f"runner {k}: max abs difference {e:.3e} (bound {TGT_TOL:.0e})")
        assert fused[k].shape == plain[k].shape and e <= TGT_TOL, k
