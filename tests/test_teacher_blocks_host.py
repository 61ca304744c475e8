"""CPU: the host side of teacher_blocks.FusedAggregatorBlocks — LayerScale folding, the refusals (each names its block), and the runner's
default, which builds nothing new.  The kernels themselves: tests/test_gpu_teacher_blocks.py."""
import pytest
import torch
import torch.nn as nn

from test_teacher_runner_ref import CFG, AggregatorLayout, fill_params


def _layout(**over):
    agg = AggregatorLayout(**dict(CFG, **over)).eval()
    fill_params(agg)
    return agg


def test_layer_scale_folds_into_the_linear():
    import gd_amd  # noqa: F401
    from gd_amd.teacher_blocks import fold_layer_scale
    agg = _layout().double()
    blk = agg.global_blocks[1]
    x = torch.randn(7, CFG["embed_dim"], dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    for lin, ls, inp in ((blk.attn.proj, blk.ls1, x), (blk.mlp.fc2, blk.ls2, torch.cat([x] * 4, 1))):
        W, b = fold_layer_scale(lin, ls)
        want = ls(lin(inp)).detach()
        assert float((inp @ W.t() + b - want).abs().max()) < 1e-12
    # nothing to fold: the module's own tensors, no copy
    W, b = fold_layer_scale(blk.attn.proj, nn.Identity())
    assert W.data_ptr() == blk.attn.proj.weight.data_ptr() and b.data_ptr() == blk.attn.proj.bias.data_ptr()
    nobias = nn.Linear(8, 8, bias=False).double()
    W, b = fold_layer_scale(nobias, blk.ls1.__class__(8).double())
    assert b is None and torch.equal(W, nobias.weight)


def test_unsupported_modules_are_refused_by_block_name():
    import gd_amd  # noqa: F401
    from gd_amd._lib import GdHipError
    from gd_amd.teacher_blocks import FusedAggregatorBlocks
    with pytest.raises(GdHipError, match=r"frame_blocks\[0\].*head dim 32"):
        FusedAggregatorBlocks(_layout(num_heads=4), dtype=torch.float32)                  # 128 / 4 = 32 channels per head
    agg = _layout()
    agg.global_blocks[2].attn.q_norm = nn.BatchNorm1d(64)
    with pytest.raises(GdHipError, match=r"global_blocks\[2\].*q_norm.*BatchNorm1d"):
        FusedAggregatorBlocks(agg, dtype=torch.float32)
    agg = _layout()
    agg.frame_blocks[1].mlp.act = nn.GELU(approximate="tanh")
    with pytest.raises(GdHipError, match=r"frame_blocks\[1\].*GELU"):
        FusedAggregatorBlocks(agg, dtype=torch.float32)
    # an odd global token count (S = 1 view of 5 + 16 tokens) cannot be cut into two views: refused before any kernel runs
    fused = FusedAggregatorBlocks(_layout(), dtype=torch.float32)
    with pytest.raises(GdHipError, match=r"global_blocks\[1\].*odd global token count 21"):
        fused.forward(torch.zeros(1, 21, 128), torch.zeros(1, 21, 2, dtype=torch.long), 1, 1)
    # Identity q/k-norm (a teacher built with qk_norm off) is served: nothing to refuse
    agg = _layout()
    for b in list(agg.frame_blocks) + list(agg.global_blocks):
        b.attn.q_norm, b.attn.k_norm = nn.Identity(), nn.Identity()
    assert FusedAggregatorBlocks(agg, dtype=torch.float32).glob[0].qk == (None, None, None, None)


def _edit(path, value):
    def edit(m):
        obj, names = m, path.split(".")
        for n in names[:-1]:
            obj = obj[int(n)] if n.isdigit() else getattr(obj, n)
        setattr(obj, names[-1], value)
    return edit


def _drop(path):
    def edit(m):
        obj, names = m, path.split(".")
        for n in names[:-1]:
            obj = obj[int(n)] if n.isdigit() else getattr(obj, n)
        delattr(obj, names[-1])
    return edit


AGGREGATOR_REFUSALS = [
    (_edit("global_blocks.0.attn.k_norm", nn.Identity()), r"global_blocks\[0\].*q_norm.*LayerNorm.*Identity"),
    (_edit("frame_blocks.1.attn.q_norm", nn.Identity()), r"frame_blocks\[1\].*q_norm.*Identity.*LayerNorm"),
    (_edit("frame_blocks.2.attn.k_norm", nn.LayerNorm(64, eps=1e-6)), r"frame_blocks\[2\].*q_norm.*k_norm.*eps"),
    (_edit("global_blocks.1.attn.q_norm", nn.LayerNorm(64, elementwise_affine=False)), r"global_blocks\[1\].*q_norm"),
    (_edit("frame_blocks.0.attn.rope", None), r"frame_blocks\[0\].*attn\.rope"),
    (_edit("frame_blocks.0.attn.scale", 0.25), r"frame_blocks\[0\].*attn\.scale"),
    (_edit("global_blocks.1.norm2", nn.LayerNorm(128, elementwise_affine=False)), r"global_blocks\[1\].*norm2"),
    (_edit("frame_blocks.2.norm1", nn.LayerNorm(64)), r"frame_blocks\[2\].*norm1"),
    (_drop("global_blocks.2.attn"), r"global_blocks\[2\].*attn"),
    (_drop("frame_blocks.1.mlp"), r"frame_blocks\[1\].*mlp"),
    (_drop("frame_blocks.0.mlp.fc2"), r"frame_blocks\[0\].*fc2"),
    (_drop("global_blocks.0.attn.proj"), r"global_blocks\[0\].*proj"),
    (_drop("global_blocks.0.norm1"), r"global_blocks\[0\].*norm1"),
    (_edit("aa_order", ["global", "frame"]), r"aa_order"),
    (lambda a: setattr(a, "global_blocks", a.global_blocks[:2]), r"3 frame / 2 global blocks"),
    (_edit("aa_block_size", 2), r"3 frame / 3 global blocks.*groups of 2"),
    (_drop("frame_blocks"), r"frame_blocks"),
    (_drop("patch_start_idx"), r"patch_start_idx"),
]


@pytest.mark.parametrize("case", range(len(AGGREGATOR_REFUSALS)))
def test_aggregator_refusals_name_the_block_and_the_attribute(case):
    """One case per refusal branch of the aggregator's block reader: construction only, no device."""
    import gd_amd  # noqa: F401
    from gd_amd._lib import GdHipError
    from gd_amd.teacher_blocks import FusedAggregatorBlocks
    edit, match = AGGREGATOR_REFUSALS[case]
    agg = _layout()
    FusedAggregatorBlocks(agg, dtype=torch.float32)                                       # accepted as it stands
    edit(agg)
    with pytest.raises(GdHipError, match=match) as e:
        FusedAggregatorBlocks(agg, dtype=torch.float32)
    print(e.value)
    assert str(e.value).startswith("FusedAggregatorBlocks: ")


@pytest.mark.parametrize("path", ["frame_blocks.0.norm1", "global_blocks.1.norm2", "frame_blocks.1.attn.k_norm"])
def test_a_layer_norm_without_bias_is_refused(path):
    """The kernels read beta wherever they read gamma, so LayerNorm(bias=False) is refused at construction (before the one reader it was
    packed with a null beta)."""
    import gd_amd  # noqa: F401
    from gd_amd._lib import GdHipError
    from gd_amd.teacher_blocks import FusedAggregatorBlocks
    agg = _layout()
    _edit(path, nn.LayerNorm(64 if path.endswith("k_norm") else 128, bias=False))(agg)
    blk, attr = path.split(".", 2)[0] + rf"\[{path.split('.')[1]}\]", path.split(".", 2)[2]
    with pytest.raises(GdHipError, match=blk + r"\." + attr.replace(".", r"\.") + r": .*with a bias"):
        FusedAggregatorBlocks(agg, dtype=torch.float32)


def test_aggregator_accepts_a_layout_without_mlp_act_and_without_layer_scale():
    import gd_amd  # noqa: F401
    from gd_amd.teacher_blocks import FusedAggregatorBlocks
    agg = _layout()
    for b in agg.frame_blocks:
        del b.ls1, b.ls2                                                                  # no LayerScale attribute: the module's own tensors
    assert not hasattr(agg.frame_blocks[0].mlp, "act")                                     # the layout's Mlp calls F.gelu itself
    f = FusedAggregatorBlocks(agg, dtype=torch.float32)
    assert f.frame[0].wproj.data_ptr() == agg.frame_blocks[0].attn.proj.weight.data_ptr()
    assert f.frame[0].qk_eps == agg.frame_blocks[0].attn.q_norm.eps and f.frame[0].base == 100.0 and f.per == 1


def test_runner_default_builds_no_fused_blocks(monkeypatch):
    import gd_amd  # noqa: F401
    from gd_amd import teacher_blocks
    from gd_amd.teacher_runner import VGGTTeacherRunner
    built = []
    orig = teacher_blocks.FusedAggregatorBlocks.__init__
    monkeypatch.setattr(teacher_blocks.FusedAggregatorBlocks, "__init__", lambda self, *a, **k: (built.append(1), orig(self, *a, **k))[1])
    teacher = type("T", (), {"aggregator": _layout()})()
    assert VGGTTeacherRunner(teacher).fused is None and VGGTTeacherRunner(teacher, fused_blocks=False).fused is None and not built
    r = VGGTTeacherRunner(teacher, dtype=torch.float32, fused_blocks=True)
    assert isinstance(r.fused, teacher_blocks.FusedAggregatorBlocks) and built == [1]
