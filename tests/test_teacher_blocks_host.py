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
