"""GPU: the VGGT teacher's DINOv2 patch embedder on the HIP kernels — the two new kernels of csrc/norm.hip (gd_dino_assemble_tokens bit for bit,
gd_vggt_tokens_from_dino per element against fp64 within tests/rowwise_ref64.ln_fwd_bound), teacher_blocks.FusedDinoEmbed against fixture G29 (what the
reference's own DinoVisionTransformer returned, tools/make_golden_g29.py) and against the layout module under autocast, and the runner's
`fused_patch_embed` switch against the default runner.

Every test prints its measured error beside the bound before it asserts."""
import pytest
import torch

import rowwise_ref64 as R64
from conftest import load_golden
from dino_layout import DINO_CFG, DINO_SIZES, DinoAggregatorLayout, DinoLayout
from test_gpu_teacher_blocks import MAPS_TOL, DeviceRope2D, max_abs
from test_teacher_runner_ref import CFG, fill_params

pytestmark = pytest.mark.gpu

PAD = 64            # elements of surround on either side of an output (a multiple of 16 bytes in fp32 and in int64)
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def surrounded(shape, dtype, fill):
    """-> (buf, view): `view` a contiguous tensor of `shape` inside `buf`, PAD cells of `fill` on either side."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device="cuda")
    return buf, buf[PAD:PAD + n].view(shape)


def untouched(buf, fill):
    edge = torch.cat([buf[:PAD], buf[-PAD:]])
    return bool(edge.isnan().all()) if fill != fill else bool((edge == fill).all())


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. gd_dino_assemble_tokens: every element one fp32 addition or a copy
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("BS,Np,R,D", [(2, 15, 4, 128), (3, 4, 0, 136), (2, 16, 4, 1024)])
def test_dino_assemble_tokens_bit_exact(BS, Np, R, D, dtype):
    from gd_amd import ops
    g = torch.Generator().manual_seed(BS * 1000 + Np * 10 + R)
    patch = torch.randn(BS * Np, D, generator=g).to(dtype).cuda()
    cls, pos = torch.randn(D, generator=g).cuda(), torch.randn(1 + Np, D, generator=g).cuda()
    reg = torch.randn(R, D, generator=g).cuda() if R else None
    buf, out = surrounded((BS, 1 + R + Np, D), torch.float32, float("nan"))
    got = ops.dino_assemble_tokens(patch, cls, reg, pos, BS, Np, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(got[:, 0], (cls + pos[0]).expand(BS, D))
    if R:
        assert torch.equal(got[:, 1:1 + R], reg.expand(BS, R, D))
    assert torch.equal(got[:, 1 + R:], patch.float().view(BS, Np, D) + pos[1:])
    assert untouched(buf, float("nan"))
    assert torch.equal(ops.dino_assemble_tokens(patch, cls, reg, pos, BS, Np), got)          # the wrapper's own output buffer


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. gd_vggt_tokens_from_dino: final norm on the patch rows + the aggregator's token and position assembly
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,gh,gw,R,Rg,D", [(1, 2, 3, 5, 4, 4, 128), (2, 3, 2, 2, 0, 4, 128), (1, 2, 4, 4, 4, 0, 1024), (1, 1, 2, 3, 4, 4, 2048)])
def test_vggt_tokens_from_dino_against_fp64(B, S, gh, gw, R, Rg, D):
    from gd_amd import ops
    g = torch.Generator().manual_seed(D + 7 * gh + S)
    BS, Np, eps = B * S, gh * gw, 1e-6
    x = torch.randn(BS, 1 + R + Np, D, generator=g)
    x[:, 1 + R::2] = 3.0 + 0.5 * x[:, 1 + R::2]                      # every other patch row: mean 3, std 0.5 (the bound's conditioning term)
    x[:, :1 + R] = float("nan")                                      # the embedder's cls and register rows must not be read
    gamma, beta = 1.0 + 0.3 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g)
    camera = torch.randn(2, D, generator=g)
    regs = torch.randn(2, Rg, D, generator=g) if Rg else None
    P = 1 + Rg + Np
    tbuf, tokens = surrounded((BS, P, D), torch.float32, float("nan"))
    pbuf, pos = surrounded((BS, P, 2), torch.int64, -7)
    dev = lambda t: None if t is None else t.cuda()
    got_t, got_p = ops.vggt_tokens_from_dino(x.cuda(), gamma.cuda(), beta.cuda(), eps, dev(camera), dev(regs), B, S, gh, gw, R, tokens=tokens, pos=pos)
    assert got_t.data_ptr() == tokens.data_ptr() and got_p.data_ptr() == pos.data_ptr()
    got_t, got_p = got_t.cpu(), got_p.cpu()
    assert bool(got_t.isfinite().all())
    # camera / register rows: bit-exact copies, slot 0 for the first frame of every batch entry, slot 1 for the others
    for f in range(BS):
        slot = 0 if f % S == 0 else 1
        assert torch.equal(got_t[f, 0], camera[slot]), f
        if Rg:
            assert torch.equal(got_t[f, 1:1 + Rg], regs[slot]), f
    # normalised rows: per element against fp64
    rows = x[:, 1 + R:].reshape(BS * Np, D)
    want, _, _ = R64.ln_fwd64(rows, gamma, beta, eps)
    bound, _, _ = R64.ln_fwd_bound(rows, gamma, beta, eps, torch.float32)
    err = (got_t[:, 1 + Rg:].reshape(BS * Np, D).double() - want).abs()
    ratio = float((err / bound).max())
    print(f"vggt_tokens_from_dino {(B, S, gh, gw, R, Rg, D)}: worst |err| / bound {ratio:.3f} (max err {float(err.max()):.3e})")
    assert ratio <= 1.0
    # positions: exact
    grid = torch.cartesian_prod(torch.arange(gh), torch.arange(gw)) + 1
    want_p = torch.cat([torch.zeros(1 + Rg, 2, dtype=torch.int64), grid]).expand(BS, -1, -1)
    assert torch.equal(got_p, want_p)
    assert untouched(tbuf, float("nan")) and untouched(pbuf, -7)


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. - 4. the whole embedder
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def layout():
    m = DinoLayout(**DINO_CFG).eval()
    fill_params(m)
    return m.cuda()


@pytest.fixture(scope="module")
def g29():
    return load_golden("g29_dino_embed")


@pytest.mark.parametrize("H,W", DINO_SIZES)
def test_whole_embedder_f32_against_reference_fixture(layout, g29, H, W):
    from gd_amd.teacher_blocks import FusedDinoEmbed
    fused = FusedDinoEmbed(layout, dtype=torch.float32)
    img = g29[f"img_{H}x{W}"].cuda()
    x = fused.features(img)
    out = fused.forward(img)
    for what, got, want in (("x_prenorm", x, g29[f"x_prenorm_{H}x{W}"]), ("x_norm_patchtokens", out["x_norm_patchtokens"], g29[f"x_norm_patchtokens_{H}x{W}"])):
        e, bound = max_abs(got, want), 1e-4 * float(want.abs().max())
        print(f"{H}x{W} {what}: e {e:.3e}, bound {bound:.3e}")
        assert got.shape == want.shape and got.dtype == torch.float32 and e <= bound, what
    assert set(out) == {"x_norm_clstoken", "x_norm_regtokens", "x_norm_patchtokens", "x_prenorm", "masks"} and out["masks"] is None
    assert out["x_norm_clstoken"].shape == (2, 128) and out["x_norm_regtokens"].shape == (2, 4, 128) and torch.equal(out["x_prenorm"], x)


def test_normalisation_inside_im2col_equals_a_normalised_image(layout):
    from gd_amd.teacher_blocks import FusedDinoEmbed
    fused = FusedDinoEmbed(layout, dtype=torch.float32)
    img01 = torch.rand(2, 3, 42, 70, generator=torch.Generator().manual_seed(31)).cuda()
    mean, std = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1), torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    want = fused.features((img01 - mean) / std)
    got = fused.features(img01, MEAN, STD)
    e, bound = max_abs(got, want), 1e-4 * float(want.abs().max())
    print(f"features(img01, mean, std) vs features((img01 - mean) / std): e {e:.3e}, bound {bound:.3e}")
    assert e <= bound


def test_whole_embedder_bf16_in_the_precision_class_of_autocast(layout, g29):
    from gd_amd.teacher_blocks import FusedDinoEmbed
    img = g29["img_42x70"].cuda()
    with torch.no_grad():
        want = layout(img)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ref = layout(img)
    hip = FusedDinoEmbed(layout, dtype=torch.bfloat16).forward(img)
    pairs = {k: (max_abs(ref[k], want[k]), max_abs(hip[k], want[k])) for k in ("x_prenorm", "x_norm_patchtokens")}
    for k, (e_ref, e_hip) in pairs.items():
        print(f"bf16 {k}: e_ref (torch autocast) {e_ref:.4e}, e_hip (fused) {e_hip:.4e}")
    for k, (e_ref, e_hip) in pairs.items():
        assert e_hip <= 2 * e_ref, k


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. the runner's switch
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def teacher():
    """A teacher holding the aggregator layout (width 128, 2 heads) around the DINO layout, its shared RoPE module able to run on the GPU."""
    agg = DinoAggregatorLayout(**CFG, dino_depth=3, dino_heads=2).eval()
    fill_params(agg)
    rope = DeviceRope2D()
    agg.rope = rope
    for b in list(agg.frame_blocks) + list(agg.global_blocks):
        b.attn.rope = rope
    return type("T", (), {"aggregator": agg.cuda()})()


def _maps(third, fused_blocks):
    """The cross-view maps of an `aggregate` result: the finished maps (fused blocks) or built from the hooks' (q, k)."""
    from gd_amd import teacher_glue as tg
    if fused_blocks:
        return third
    maps = None
    for i, (q, k) in enumerate(third):
        maps = tg.cross_view_attention_maps(q, k, 64 ** -0.5, 0.8, 5, out=maps, weight=1.0 / (q.shape[1] * len(third)), accumulate=i > 0)
    return maps


@pytest.mark.parametrize("H,W", [(56, 56), (42, 70)])
@pytest.mark.parametrize("fused_blocks", [False, True], ids=["modules", "fused_blocks"])
def test_runner_fused_patch_embed_against_the_default_runner(teacher, fused_blocks, H, W):
    from gd_amd.teacher_runner import VGGTTeacherRunner
    agg = teacher.aggregator
    img = torch.rand(1, 2, 3, H, W, generator=torch.Generator().manual_seed(H + W)).cuda()
    want_tok, want_ps, want_third = VGGTTeacherRunner(teacher, dtype=torch.float32, fused_blocks=fused_blocks).aggregate(img)
    calls = []
    hook = agg.patch_embed.register_forward_hook(lambda mod, a, out: calls.append(1))
    try:
        got_tok, got_ps, got_third = VGGTTeacherRunner(teacher, dtype=torch.float32, fused_blocks=fused_blocks, fused_patch_embed=True).aggregate(img)
    finally:
        hook.remove()
    assert "forward" not in vars(agg.patch_embed)
    assert got_ps == want_ps == 5 and len(got_tok) == len(want_tok) == 3
    if fused_blocks:
        assert len(calls) == 0                                      # neither the aggregator's forward nor the embedder module ran
    for i, (a, b) in enumerate(zip(got_tok, want_tok)):
        e, bound = max_abs(a, b), 1e-4 * float(b.abs().max())
        print(f"{H}x{W} fused_blocks={fused_blocks} tokens_{i}: e {e:.3e}, bound {bound:.3e}")
        assert a.shape == b.shape and e <= bound, i
    e = max_abs(_maps(got_third, fused_blocks), _maps(want_third, fused_blocks))
    print(f"{H}x{W} fused_blocks={fused_blocks} maps: e {e:.3e}, bound {MAPS_TOL:g}")
    assert e < MAPS_TOL


@pytest.mark.parametrize("fused_blocks", [False, True], ids=["modules", "fused_blocks"])
def test_runner_restores_the_embedder_after_a_refused_image(teacher, fused_blocks):
    from gd_amd._lib import GdHipError
    from gd_amd.teacher_runner import VGGTTeacherRunner
    agg = teacher.aggregator
    runner = VGGTTeacherRunner(teacher, dtype=torch.float32, fused_blocks=fused_blocks, fused_patch_embed=True)
    with pytest.raises(GdHipError, match="patch_size"):             # a host refusal: the height is not a multiple of the patch
        runner.aggregate(torch.rand(1, 2, 3, 50, 56, device="cuda"))
    assert "forward" not in vars(agg.patch_embed)
    runner.aggregate(torch.rand(1, 2, 3, 56, 56, device="cuda"))   # and the runner still works
    assert "forward" not in vars(agg.patch_embed)


def test_runner_with_the_switch_off_is_the_previous_path(teacher):
    """Default arguments: `_block_inputs` (the aggregator's own forward up to the first frame block) still feeds the fused blocks, and the module path
    is the aggregator's forward — bit for bit."""
    from gd_amd.teacher_blocks import FusedAggregatorBlocks
    from gd_amd.teacher_runner import QKCapture, VGGTTeacherRunner, _no_attention_maps
    agg = teacher.aggregator
    img = torch.rand(1, 2, 3, 42, 70, generator=torch.Generator().manual_seed(3)).cuda()
    runner = VGGTTeacherRunner(teacher, dtype=torch.float32, fused_blocks=True)
    assert runner.embed is None
    used, inner = [], runner._block_inputs
    runner._block_inputs = lambda rgb: used.append(1) or inner(rgb)
    got_tok, ps, got_maps = runner.aggregate(img)
    assert used == [1] and ps == 5
    want_tok, want_maps = FusedAggregatorBlocks(agg, dtype=torch.float32).forward(*inner(img), 1, 2)
    assert all(torch.equal(a, b) for a, b in zip(got_tok, want_tok)) and torch.equal(got_maps, want_maps)
    runner = VGGTTeacherRunner(teacher, dtype=torch.float32)
    got_tok, ps, qk = runner.aggregate(img)
    with torch.no_grad(), QKCapture(runner.sel) as cap, _no_attention_maps(runner.sel):
        want_tok, _, _ = agg(img)
    assert all(torch.equal(a, b) for a, b in zip(got_tok, want_tok))
    assert all(torch.equal(q, q2) and torch.equal(k, k2) for (q, k), (q2, k2) in zip(qk, cap.pairs()))
