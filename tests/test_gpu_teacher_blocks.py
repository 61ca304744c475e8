"""GPU: the VGGT teacher's attention blocks on the HIP kernels (gd_qk_norm_rope, teacher_blocks.FusedAggregatorBlocks, the runner's
`fused_blocks` path) against fp64, against the torch module tree with the aggregator's layout (tests/test_teacher_runner_ref.py) and
against fixture G22 (what the reference's own Aggregator returned).

Every test prints its measured error beside the bound before it asserts; tools/bench_teacher.py records the bf16 pair under "parity"."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import gd_oracle as O
from conftest import load_golden, rel_err
from test_teacher_runner_ref import CFG, AggregatorLayout, fill_params

pytestmark = pytest.mark.gpu

ROPE_TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2}      # tests/test_gpu_rope.py, gd_rope_2d at that dtype (rel_err: max abs / max |want|)
MAPS_TOL = 2e-6                                              # tests/test_gpu_teacher_glue.py, gd_cross_view_attn in f32 against its fixture


class DeviceRope2D(nn.Module):
    """gd_oracle.rope_2d's arithmetic on [B, H, N, D] with the frequency table on the tokens' device (the oracle builds it on the host, so
    the layout's own RoPE module cannot run on the GPU); on the host it IS the oracle's function."""

    def forward(self, tokens, positions):
        if not tokens.is_cuda:
            return O.rope_2d(tokens.transpose(1, 2), positions).transpose(1, 2)
        Q, positions = tokens.shape[-1] // 4, positions.to(tokens.device)             # (the layout builds its position grid on the host)
        inv = 1.0 / (100.0 ** (torch.arange(Q, dtype=torch.float32, device=tokens.device) / Q))
        out = tokens.clone()
        for ax in range(2):
            th = positions[..., ax].float().unsqueeze(-1) * inv                       # [B, N, Q]
            c, s = torch.cos(th).unsqueeze(1), torch.sin(th).unsqueeze(1)
            u, v = tokens[..., 2 * ax * Q:(2 * ax + 1) * Q], tokens[..., (2 * ax + 1) * Q:(2 * ax + 2) * Q]
            out[..., 2 * ax * Q:(2 * ax + 1) * Q] = u * c - v * s
            out[..., (2 * ax + 1) * Q:(2 * ax + 2) * Q] = v * c + u * s
        return out


def make_layout(**over):
    """The aggregator-shaped module tree with the fixture's deterministic weights, its shared RoPE module able to run on either device."""
    agg = AggregatorLayout(**dict(CFG, **over)).eval()
    fill_params(agg)
    rope = DeviceRope2D()
    agg.rope = rope
    for b in list(agg.frame_blocks) + list(agg.global_blocks):
        b.attn.rope = rope
    return agg


def block_inputs(agg, img):
    from gd_amd.teacher_runner import VGGTTeacherRunner
    return VGGTTeacherRunner(type("T", (), {"aggregator": agg})(), dtype=torch.float32)._block_inputs(img)


def max_abs(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against fp64
# ----------------------------------------------------------------------------------------------------------------------------------
def _qk_case(B, N, H, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + 131 * N + H)
    qkv = (1.5 * torch.randn(B * N, 3 * H * 64, generator=g) + 0.3).to(dtype)
    pos = torch.randint(0, 38, (B, N, 2), generator=g)
    pos[:, :5] = 0                                   # the prefix tokens
    pos[0, 5], pos[-1, -1] = torch.tensor([37, 1]), torch.tensor([2, 37])
    gb = [(1.0 if i % 2 == 0 else 0.0) + 0.3 * torch.randn(64, generator=g) for i in range(4)]      # gq, bq, gk, bk
    return qkv, pos.reshape(B * N, 2), gb


def _qk_ref64(qkv, B, N, H, pos, gb, eps):
    """fp64: (q, k) [B, N, H, 64] after LayerNorm_64 (none when gb is None) and rope_2d."""
    x = qkv.double().reshape(B, N, 3, H, 64)
    out = []
    for i in range(2):
        t = x[:, :, i]
        if gb is not None:
            t = F.layer_norm(t, (64,), gb[2 * i].double(), gb[2 * i + 1].double(), eps)
        out.append(O.rope_2d(t, pos.reshape(B, N, 2), 100.0, 1.0))
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,N,H", [(2, 21, 2), (1, 42, 2), (1, 130, 3)])
def test_qk_norm_rope_against_fp64(B, N, H, dtype):
    from gd_amd import ops
    from gd_amd.rope import rope_2d
    eps, tol = 1e-5, ROPE_TOL[dtype]
    qkv, pos, gb = _qk_case(B, N, H, dtype)
    dev_gb = [t.cuda() for t in gb]
    buf = qkv.cuda()
    q_out, k_out = ops.qk_norm_rope(buf, B, N, H, pos.cuda(), *dev_gb, eps, 100.0, want_qk=True)
    got = buf.cpu().reshape(B, N, 3, H, 64)
    want_q, want_k = _qk_ref64(qkv, B, N, H, pos, gb, eps)
    eq, ek = rel_err(got[:, :, 0], want_q), rel_err(got[:, :, 1], want_k)
    print(f"qk_norm_rope {(B, N, H)} {dtype}: rel err q {eq:.3e} k {ek:.3e} (tolerance {tol:g})")
    assert eq < tol and ek < tol
    assert torch.equal(got[:, :, 2], qkv.reshape(B, N, 3, H, 64)[:, :, 2])                                   # v: bit-identical
    assert torch.equal(q_out.cpu(), got[:, :, 0].permute(0, 2, 1, 3)) and torch.equal(k_out.cpu(), got[:, :, 1].permute(0, 2, 1, 3))
    # without the optional outputs: the same in-place result, nothing returned
    buf2 = qkv.cuda()
    assert ops.qk_norm_rope(buf2, B, N, H, pos.cuda(), *dev_gb, eps, 100.0) is None and torch.equal(buf2, buf)
    # null gamma / beta: plain RoPE of q and k — the oracle's, and gd_rope_2d's on the same data
    buf3 = qkv.cuda()
    ops.qk_norm_rope(buf3, B, N, H, pos.cuda(), None, None, None, None, eps, 100.0)
    got3 = buf3.cpu().reshape(B, N, 3, H, 64)
    plain_q, plain_k = _qk_ref64(qkv, B, N, H, pos, None, eps)
    assert rel_err(got3[:, :, 0], plain_q) < tol and rel_err(got3[:, :, 1], plain_k) < tol
    assert torch.equal(got3[:, :, 2], qkv.reshape(B, N, 3, H, 64)[:, :, 2])
    twin = qkv.cuda().reshape(B, N, 3 * H, 64)
    rope_2d(twin[:, :, :2 * H], pos.cuda().reshape(B, N, 2), 100.0, 1.0)
    assert rel_err(buf3.reshape(B, N, 3 * H, 64)[:, :, :2 * H], twin[:, :, :2 * H]) < tol


def test_qk_norm_rope_argument_checks():
    from gd_amd import ops
    from gd_amd._lib import GdHipError, lib
    qkv = torch.zeros(8, 3 * 2 * 64, device="cuda")
    pos = torch.zeros(8, 2, dtype=torch.long, device="cuda")
    g = torch.ones(64, device="cuda")
    with pytest.raises(GdHipError):
        ops.qk_norm_rope(qkv, 1, 8, 2, pos, g, g, None, None, 1e-5, 100.0)                 # some of gamma / beta missing
    with pytest.raises(GdHipError):
        ops.qk_norm_rope(qkv, 1, 9, 2, pos, g, g, g, g, 1e-5, 100.0)                       # shape does not match B * N
    rc = lib().gd_qk_norm_rope(qkv.data_ptr(), pos.data_ptr(), None, None, None, None, None, None, 1, 8, 4, 32, 1e-5, 100.0, 0, None)
    assert rc != 0 and b"head_dim" in lib().gd_last_error()


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. - 6. blocks, the whole stack, the runner
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g22():
    """Fixture G22's image through the fused f32 stack, once: (golden, outputs, maps)."""
    from gd_amd.teacher_blocks import FusedAggregatorBlocks
    g = load_golden("g22_vggt_aggregator")
    agg = make_layout().cuda()
    tokens, pos = block_inputs(agg, g["img"].cuda())
    outputs, maps = FusedAggregatorBlocks(agg, dtype=torch.float32).forward(tokens, pos, 1, 2)
    return g, outputs, maps


def test_one_frame_block_and_one_global_block_f32():
    from gd_amd.teacher_blocks import FusedAggregatorBlocks
    agg = make_layout()
    ref = copy.deepcopy(agg).double()
    fused = FusedAggregatorBlocks(agg.cuda(), dtype=torch.float32)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 21, 128, generator=g)
    grid = torch.cartesian_prod(torch.arange(4), torch.arange(4)) + 1
    pos = torch.cat([torch.zeros(5, 2, dtype=torch.long), grid]).expand(2, -1, -1).contiguous()
    with torch.no_grad():
        want_f = ref.frame_blocks[0](x.double(), pos=pos)
        want_g, _ = ref.global_blocks[1](x.double().reshape(1, 42, 128), pos=pos.reshape(1, 42, 2), return_attn=True, temperature=0.8)
    got_f, none = fused._block(fused.frame[0], x.reshape(42, 128).cuda(), pos.reshape(42, 2).cuda(), 2, 21)
    got_g, qk = fused._block(fused.glob[1], x.reshape(42, 128).cuda(), pos.reshape(42, 2).cuda(), 1, 42, want_qk=True)
    ef, eg = max_abs(got_f, want_f.reshape(42, 128)), max_abs(got_g, want_g.reshape(42, 128))
    print(f"frame block e {ef:.3e} (max {float(want_f.abs().max()):.3f}), global block e {eg:.3e} (max {float(want_g.abs().max()):.3f})")
    assert ef <= 1e-4 * float(want_f.abs().max()) and eg <= 1e-4 * float(want_g.abs().max())
    assert none is None and qk[0].shape == (1, 2, 42, 64) and qk[1].shape == (1, 2, 42, 64)


def test_whole_stack_f32_against_reference_fixture(g22):
    g, outputs, maps = g22
    assert len(outputs) == 3 and outputs[0].shape == (1, 2, 21, 256) and maps.shape == (2, 16, 16)
    for i, t in enumerate(outputs):
        want = g[f"tokens_{i}"]
        e = max_abs(t, want)
        print(f"tokens_{i}: e {e:.3e}, bound {1e-4 * float(want.abs().max()):.3e}")
        assert e <= 1e-4 * float(want.abs().max()), i
    want = g["attn_mean"].mean(dim=1)
    e = max_abs(maps, want)
    print(f"maps: e {e:.3e}, bound {MAPS_TOL:g}")
    assert e < MAPS_TOL


def bf16_parity_pair(img=None):
    """-> {"tokens": (e_ref, e_hip), "maps": (e_ref, e_hip)}: on the fixture's weights and image, the max abs error against the module tree's
    fp64 run of (e_ref) the same modules under torch.autocast(bfloat16) and (e_hip) the fused bf16 path."""
    from gd_amd.teacher_runner import VGGTTeacherRunner
    agg = make_layout()
    img = load_golden("g22_vggt_aggregator")["img"] if img is None else img
    with torch.no_grad():
        tok64, _, attn64 = copy.deepcopy(agg).double()(img.double())
    agg = agg.cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        tok_ref, _, attn_ref = agg(img.cuda())
    # the runner's fused path: the aggregator's pre-block part under the same autocast, then the blocks on the kernels
    tok_hip, _, maps_hip = VGGTTeacherRunner(type("T", (), {"aggregator": agg})(), dtype=torch.bfloat16, fused_blocks=True).aggregate(img.cuda())
    return {"tokens": (max(max_abs(a, b) for a, b in zip(tok_ref, tok64)), max(max_abs(a, b) for a, b in zip(tok_hip, tok64))),
            "maps": (max_abs(attn_ref.float().mean(dim=1), attn64.mean(dim=1)), max_abs(maps_hip, attn64.mean(dim=1)))}


def test_whole_stack_bf16_in_the_precision_class_of_autocast():
    pair = bf16_parity_pair()
    for what, (e_ref, e_hip) in pair.items():
        print(f"bf16 {what}: e_ref (torch autocast) {e_ref:.4e}, e_hip (fused) {e_hip:.4e}")
    for what, (e_ref, e_hip) in pair.items():
        assert e_hip <= 2 * e_ref, what


def test_second_geometry_non_square_f32():
    """126 x 70 at patch 14: 9 x 5 + 5 = 50 tokens per view, 100 global tokens, y and x positions of different range."""
    from gd_amd.teacher_blocks import FusedAggregatorBlocks
    agg = make_layout()
    img = torch.rand(1, 2, 3, 126, 70, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        want_tok, _, want_attn = copy.deepcopy(agg).double()(img.double())
    agg = agg.cuda()
    tokens, pos = block_inputs(agg, img.cuda())
    assert tokens.shape == (2, 50, 128) and int(pos[..., 0].max()) == 9 and int(pos[..., 1].max()) == 5
    outputs, maps = FusedAggregatorBlocks(agg, dtype=torch.float32).forward(tokens, pos, 1, 2)
    for i, (t, w) in enumerate(zip(outputs, want_tok)):
        e = max_abs(t, w)
        print(f"126x70 tokens_{i}: e {e:.3e}, bound {1e-4 * float(w.abs().max()):.3e}")
        assert e <= 1e-4 * float(w.abs().max()), i
    e = max_abs(maps, want_attn.mean(dim=1))
    print(f"126x70 maps: e {e:.3e}, bound {MAPS_TOL:g}")
    assert maps.shape == (2, 45, 45) and e < MAPS_TOL


def test_runner_aggregate_fused_against_hooks(g22):
    from gd_amd import teacher_glue as tg
    from gd_amd.teacher_runner import VGGTTeacherRunner
    g = g22[0]
    agg = make_layout().cuda()
    teacher = type("T", (), {"aggregator": agg})()
    img = g["img"].cuda()
    tok_f, ps_f, maps_f = VGGTTeacherRunner(teacher, dtype=torch.float32, fused_blocks=True).aggregate(img)
    tok_h, ps_h, qk = VGGTTeacherRunner(teacher, dtype=torch.float32).aggregate(img)
    assert ps_f == ps_h == 5 and len(tok_f) == len(tok_h) == 3 and len(qk) == 2
    for i, (a, b) in enumerate(zip(tok_f, tok_h)):
        assert max_abs(a, b) <= 1e-4 * float(b.abs().max()), i
    maps_h = None
    for i, (q, k) in enumerate(qk):
        maps_h = tg.cross_view_attention_maps(q, k, 64 ** -0.5, 0.8, 5, out=maps_h, weight=1.0 / (q.shape[1] * len(qk)), accumulate=i > 0)
    e = max_abs(maps_f, maps_h)
    print(f"runner maps fused vs hooks: e {e:.3e}, bound {MAPS_TOL:g}")
    assert e < MAPS_TOL
    assert max_abs(maps_f, g22[2]) < MAPS_TOL            # the runner's fused path is the class's forward on the aggregator's own inputs
