"""CPU: the VGGT teacher's DINOv2 patch embedder without a device — the test layouts (tests/dino_layout.py) against fixture G29 (what the reference's own
DinoVisionTransformer and Aggregator returned, tools/make_golden_g29.py), every refusal of teacher_blocks.FusedDinoEmbed, and the argument checks of the
two new C entry points (they fail before any launch)."""
import ctypes

import pytest
import torch
import torch.nn as nn

from dino_layout import AGG_CFG, AGG_DINO, DINO_CFG, DINO_SIZES, DinoAggregatorLayout, DinoLayout, param_layout
from test_teacher_runner_ref import CFG, AggregatorLayout, fill_params


def dino(**over):
    m = DinoLayout(**dict(DINO_CFG, **over)).eval()
    fill_params(m)
    return m


def agg_layout(**over):
    cfg = dict(CFG, dino_depth=2, dino_heads=2)
    cfg.update(over)
    a = DinoAggregatorLayout(**cfg).eval()
    fill_params(a)
    return a


def test_dino_layout_reproduces_the_reference_embedder(golden):
    g = golden("g29_dino_embed")
    m = dino()
    assert param_layout(m) == g["param_layout"]
    for H, W in DINO_SIZES:
        with torch.no_grad():
            out = m(g[f"img_{H}x{W}"])
        for k in ("x_prenorm", "x_norm_patchtokens"):
            want = g[f"{k}_{H}x{W}"]
            e = float((out[k] - want).abs().max())
            print(f"{H}x{W} {k}: e {e:.3e}, bound {1e-6 * float(want.abs().max()):.3e}")
            assert out[k].shape == want.shape and e <= 1e-6 * float(want.abs().max()), (H, W, k)


def test_aggregator_layout_reproduces_the_reference_aggregator(golden):
    g = golden("g29_dino_embed")
    a = DinoAggregatorLayout(**AGG_CFG, dino_depth=AGG_DINO["depth"], dino_heads=AGG_DINO["num_heads"]).eval()
    fill_params(a)
    with torch.no_grad():
        tokens, ps_idx, _ = a(g["agg_img"])
    assert ps_idx == g["agg_ps_idx"] == 5 and len(tokens) == 2
    assert isinstance(a.patch_embed, DinoLayout)                       # the forward's stand-in is gone again
    for i, t in enumerate(tokens):
        want = g[f"agg_tokens_{i}"]
        e = float((t - want).abs().max())
        print(f"agg tokens_{i}: e {e:.3e}, bound {1e-4 * float(want.abs().max()):.3e}")
        assert t.shape == want.shape and e <= 1e-4 * float(want.abs().max()), i


# ----------------------------------------------------------------------------------------------------------------------------------
# refusals: at construction (or at the call, before anything touches a device), naming the attribute
# ----------------------------------------------------------------------------------------------------------------------------------
class _SwiGLU(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.w12, self.w3 = nn.Linear(dim, 2 * dim), nn.Linear(dim, dim)


def _set(path, value):
    def edit(m):
        obj, names = m, path.split(".")
        for n in names[:-1]:
            obj = obj[int(n)] if n.isdigit() else getattr(obj, n)
        setattr(obj, names[-1], value)
    return edit


REFUSALS = [
    ("blocks", lambda: nn.Conv2d(3, 128, 14, 14), None),                                              # the "conv" patch embedder
    ("chunked_blocks", dino, _set("chunked_blocks", True)),
    ("head dim", lambda: dino(num_heads=4), None),
    ("attn.scale", dino, _set("blocks.1.attn.scale", 0.2)),
    ("q_norm", dino, _set("blocks.0.attn.q_norm", nn.LayerNorm(64))),
    ("k_norm", dino, _set("blocks.0.attn.k_norm", nn.LayerNorm(64))),
    ("attn.rope", dino, _set("blocks.2.attn.rope", nn.Identity())),
    ("fc1", dino, _set("blocks.0.mlp", _SwiGLU(128))),                                                 # vit_giant2's SwiGLU
    ("mlp.act", dino, _set("blocks.0.mlp.act", nn.GELU(approximate="tanh"))),
    ("mlp.act", dino, _set("blocks.0.mlp.act", nn.SiLU())),
    (".norm is not an affine", dino, _set("norm", nn.Identity())),
    ("norm2", dino, _set("blocks.1.norm2", nn.LayerNorm(128, elementwise_affine=False))),
    ("norm1", dino, _set("blocks.1.norm1", nn.LayerNorm(64))),
    ("patch_embed.proj", dino, _set("patch_embed.proj", nn.Conv2d(3, 128, 14, 7))),
    ("patch_embed.proj", dino, _set("patch_embed.proj", nn.Linear(588, 128))),
    ("register_tokens", dino, _set("register_tokens", None)),
    ("register_tokens", dino, _set("num_register_tokens", 2)),
    ("pos_embed", lambda: dino(embed_dim=132, depth=0), None),                                         # D % 8 != 0
    ("pos_embed", lambda: dino(embed_dim=2112, depth=0), None),                                        # D > 2048
]


@pytest.mark.parametrize("case", range(len(REFUSALS)), ids=[f"{i}-{r[0].split()[0]}" for i, r in enumerate(REFUSALS)])
def test_refusals_at_construction_name_the_attribute(case):
    import gd_amd  # noqa: F401
    from gd_amd._lib import GdHipError
    from gd_amd.teacher_blocks import FusedDinoEmbed
    named, make, edit = REFUSALS[case]
    m = make()
    if edit is not None:
        edit(m)
    with pytest.raises(GdHipError) as ei:
        FusedDinoEmbed(m, dtype=torch.float32)
    print(ei.value)
    assert named in str(ei.value) and "aggregator.patch_embed" in str(ei.value)


def test_served_embedder_constructs_without_a_device():
    import gd_amd  # noqa: F401
    from gd_amd.teacher_blocks import FusedDinoEmbed
    f = FusedDinoEmbed(dino(), dtype=torch.bfloat16)
    assert (f.D, f.P, f.R, f.Kp, len(f.blocks)) == (128, 14, 4, 640, 3)
    assert f.wpe.dtype == torch.bfloat16 and f.blocks[0].wqkv.dtype == torch.bfloat16 and f.blocks[0].bqkv.dtype == torch.float32
    # LayerScale is folded: proj' = diag(gamma) proj
    m = dino()
    f32 = FusedDinoEmbed(m, dtype=torch.float32)
    assert torch.equal(f32.blocks[1].wproj, m.blocks[1].ls1.gamma.detach()[:, None] * m.blocks[1].attn.proj.weight.detach())
    # the position table: the parameter itself at its own grid, the module's own resampling (cached) elsewhere
    assert torch.equal(f32._pos(56, 56, 4, 4), m.pos_embed.detach()[0])
    with torch.no_grad():
        want = m.interpolate_pos_encoding(torch.empty(1, 16, 128), 42, 70)[0]
    assert torch.equal(f32._pos(42, 70, 3, 5), want) and f32._pos(42, 70, 3, 5) is f32._pos(42, 70, 3, 5)


def test_refusals_at_the_call_and_in_the_runner():
    import gd_amd  # noqa: F401
    from gd_amd._lib import GdHipError
    from gd_amd.teacher_blocks import FusedDinoEmbed
    from gd_amd.teacher_runner import VGGTTeacherRunner
    f = FusedDinoEmbed(dino(), dtype=torch.float32)
    for shape in [(2, 3, 50, 56), (2, 3, 56, 60)]:                      # H, then W, not a multiple of the patch: refused before any device work
        with pytest.raises(GdHipError, match="patch_size"):
            f.features(torch.zeros(shape))
    with pytest.raises(GdHipError, match="patch_size"):
        f.forward(torch.zeros(1, 3, 57, 56))
    a = agg_layout()
    f2 = FusedDinoEmbed(a.patch_embed, dtype=torch.float32)
    camera, regs, prefix = f2.check_aggregator(a)
    assert camera.shape == (2, 128) and regs.shape == (2, 4, 128) and prefix == 5
    a.patch_start_idx = 0
    with pytest.raises(GdHipError, match="patch_start_idx"):
        f2.check_aggregator(a)
    with pytest.raises(GdHipError, match="patch_start_idx"):
        VGGTTeacherRunner(type("T", (), {"aggregator": a})(), dtype=torch.float32, fused_patch_embed=True)
    a.patch_start_idx = 5
    wide = FusedDinoEmbed(dino(embed_dim=192, num_heads=3, depth=1), dtype=torch.float32)
    with pytest.raises(GdHipError, match="camera_token"):                 # an aggregator of another width
        wide.check_aggregator(a)
    # the runner refuses in __init__, not in targets(): the "conv" embedder, and an embedder the class does not serve
    conv = AggregatorLayout(**CFG).eval()
    with pytest.raises(GdHipError, match="blocks"):
        VGGTTeacherRunner(type("T", (), {"aggregator": conv})(), fused_patch_embed=True)
    a.patch_embed.blocks[0].attn.rope = nn.Identity()
    with pytest.raises(GdHipError, match="attn.rope"):
        VGGTTeacherRunner(type("T", (), {"aggregator": a})(), fused_patch_embed=True)
    # the switch is keyword-only and off by default
    with pytest.raises(TypeError):
        VGGTTeacherRunner(type("T", (), {"aggregator": conv})(), torch.float32, 5, None, False, False, torch.float32, False, False, True)
    assert VGGTTeacherRunner(type("T", (), {"aggregator": conv})()).embed is None


# ----------------------------------------------------------------------------------------------------------------------------------
# the C entry points: arguments outside the contract fail before any launch, with a message
# ----------------------------------------------------------------------------------------------------------------------------------
A = 0x10000          # a 16-byte aligned address that is never dereferenced: every call below fails its checks first


def _assemble(L, D, patch=A, out=A):
    return L.gd_dino_assemble_tokens(patch, 0, A, A, A, out, 2, 16, 4, D, None)


def _from_dino(L, D, x=A, tokens=A, pos=A):
    return L.gd_vggt_tokens_from_dino(x, A, A, ctypes.c_float(1e-6), A, A, tokens, pos, 1, 2, 4, 4, 4, 4, D, None)


@pytest.mark.parametrize("D", [12, 2052])
def test_entry_points_refuse_a_width_outside_the_contract(D):
    import gd_amd  # noqa: F401
    from gd_amd import _lib
    L = _lib.lib()
    for name, call in (("gd_dino_assemble_tokens", _assemble), ("gd_vggt_tokens_from_dino", _from_dino)):
        rc = call(L, D)
        msg = L.gd_last_error()
        print(name, D, rc, msg)
        assert rc != 0 and name.encode() in msg and f"D={D}".encode() in msg


def test_entry_points_refuse_a_misaligned_pointer():
    import gd_amd  # noqa: F401
    from gd_amd import _lib
    L = _lib.lib()
    for kw in ({"patch": A + 4}, {"out": A + 8}):
        rc = _assemble(L, 128, **kw)
        assert rc != 0 and b"gd_dino_assemble_tokens" in L.gd_last_error() and b"16-byte aligned" in L.gd_last_error(), kw
    for kw in ({"x": A + 4}, {"tokens": A + 8}, {"pos": A + 8}):
        rc = _from_dino(L, 128, **kw)
        assert rc != 0 and b"gd_vggt_tokens_from_dino" in L.gd_last_error() and b"16-byte aligned" in L.gd_last_error(), kw
    # null pointers, a bad dtype and a bad shape are refused as well
    assert L.gd_dino_assemble_tokens(None, 0, A, A, A, A, 2, 16, 4, 128, None) != 0 and b"null" in L.gd_last_error()
    assert L.gd_dino_assemble_tokens(A, 0, A, None, A, A, 2, 16, 4, 128, None) != 0 and b"null" in L.gd_last_error()      # reg may be null only when R = 0
    assert L.gd_dino_assemble_tokens(A, 3, A, A, A, A, 2, 16, 4, 128, None) != 0 and b"patch_dtype" in L.gd_last_error()
    assert L.gd_vggt_tokens_from_dino(A, A, A, ctypes.c_float(1e-6), A, None, A, A, 1, 2, 4, 4, 4, 4, 128, None) != 0 and b"null" in L.gd_last_error()
    assert L.gd_vggt_tokens_from_dino(A, A, A, ctypes.c_float(1e-6), A, A, A, A, 1, 0, 4, 4, 4, 4, 128, None) != 0 and b"bad shape" in L.gd_last_error()
