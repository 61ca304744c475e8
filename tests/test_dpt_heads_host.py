"""CPU: teacher_heads.FusedDPTHead's host side — the position tables against fixture G26, every refusal (raised while the module is read, before any
HIP call, naming the attribute), and the runner's `fused_heads` switch: off by default, a refused head raises at construction, and the instance
attribute that shadows the track head's feature extractor is gone after a failing `targets()`."""
import pytest
import torch
import torch.nn as nn

import dpt_layout as DL
from conftest import load_golden
from test_teacher_runner_ref import fill_params

import gd_amd  # noqa: F401
from gd_amd import _lib, ops, teacher_heads, teacher_runner
from gd_amd._lib import GdHipError


@pytest.fixture
def no_hip(monkeypatch):
    """Any call into the library fails the test: what runs under this fixture is host logic only."""
    def boom():
        raise AssertionError("a HIP entry point was reached")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(ops, "lib", boom)


def test_host_position_tables_equal_the_fixture():
    g = load_golden("g26_dpt_head")
    H, W = g["a_image_hw"].tolist()
    px, py = teacher_heads.pos_tables(W, H, DL.FEATURES // 2, W / H)
    assert px.dtype == py.dtype == torch.float32 and px.shape == g["a_px"].shape and py.shape == g["a_py"].shape
    assert torch.equal(px, g["a_px"]) and torch.equal(py, g["a_py"])
    # the aspect ratio is the IMAGE's: the same grid at another aspect gives other tables
    assert float((teacher_heads.pos_tables(W, H, DL.FEATURES // 2, 1.0)[0] - px).abs().max()) > 1e-3


def _set(path, value):
    def mutate(m):
        obj, parts = m, path.split(".")
        for p in parts[:-1]:
            obj = obj[int(p)] if p.isdigit() else getattr(obj, p)
        if parts[-1].isdigit():
            obj[int(parts[-1])] = value
        else:
            setattr(obj, parts[-1], value)
    return mutate


REFUSALS = {
    "groups": (_set("scratch.refinenet2.resConfUnit1.conv1", nn.Conv2d(16, 16, 3, padding=1, groups=2)), {}, "scratch.refinenet2.resConfUnit1.conv1", "groups"),
    "block_groups": (_set("scratch.refinenet2.groups", 2), {}, "scratch.refinenet2.groups", "groups"),
    "batch_norm": (_set("scratch.refinenet3.resConfUnit2.bn", True), {}, "scratch.refinenet3.resConfUnit2.bn", "batch-norm"),
    "norm_layer": (_set("scratch.refinenet1.resConfUnit1.norm1", nn.BatchNorm2d(16)), {}, "scratch.refinenet1.resConfUnit1.bn", "batch-norm"),
    "deconv_block": (_set("scratch.refinenet1.deconv", True), {}, "scratch.refinenet1.deconv", "not served"),
    "expand_block": (_set("scratch.refinenet2.expand", True), {}, "scratch.refinenet2.expand", "not served"),
    "align_corners": (_set("scratch.refinenet4.align_corners", False), {}, "scratch.refinenet4.align_corners", "align_corners=True"),
    "features_not_8": (None, dict(features=12), "scratch.layer1_rn", "multiples of 8"),
    "out_channels_not_8": (None, dict(out_channels=[12, 32, 64, 64]), "projects[0]", "multiples of 8"),
    "activation": (None, dict(activation="norm_exp"), "activation", "norm_exp"),
    "conf_activation": (None, dict(conf_activation="softplus"), "conf_activation", "softplus"),
    "resize_kind": (_set("resize_layers.2", nn.Upsample(scale_factor=2)), {}, "resize_layers[2]", "Upsample"),
    "resize_deconv_stride": (_set("resize_layers.0", nn.ConvTranspose2d(16, 16, 4, stride=2, padding=1)), {}, "resize_layers[0]", "kernel = stride"),
    "resize_conv_stride": (_set("resize_layers.3", nn.Conv2d(64, 64, 3, stride=1, padding=1)), {}, "resize_layers[3]", "stride 2"),
    "unit_activation": (_set("scratch.refinenet2.resConfUnit2.activation", nn.GELU()), {}, "scratch.refinenet2.resConfUnit2.activation", "ReLU"),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals_name_the_attribute(what, dtype, no_hip):
    mutate, over, attr, word = REFUSALS[what]
    m = DL.make_head("a", **over)
    if mutate is not None:
        mutate(m)
    with pytest.raises(GdHipError) as e:
        teacher_heads.FusedDPTHead(m, dtype=dtype, name="depth_head")
    print(e.value)
    assert f"depth_head.{attr}:" in str(e.value) and word in str(e.value)


@pytest.mark.parametrize("attr", ["pos_embed", "feature_only", "down_ratio"])
def test_a_present_none_attribute_is_the_modules_own_value_not_a_missing_one(attr, no_hip):
    """Only an absent attribute is missing: None stands for False in the two flags, and down_ratio is not read before the first call."""
    m = DL.make_head("a")
    setattr(m, attr, None)
    h = teacher_heads.FusedDPTHead(m, name="depth_head")
    assert getattr(h, attr) in (False, None)
    m = DL.make_head("a")
    m.__dict__.pop(attr, None)
    if not hasattr(m, attr):
        with pytest.raises(GdHipError, match=rf"depth_head\.{attr}: missing"):
            teacher_heads.FusedDPTHead(m, name="depth_head")


def test_served_heads_construct_without_a_hip_call(no_hip):
    for case in DL.CASES:
        for dtype in (torch.float32, torch.bfloat16):
            h = teacher_heads.FusedDPTHead(DL.make_head(case), dtype=dtype)
            assert h.feature_only == DL.CASES[case]["feature_only"] and h.rn[0][0].dtype == dtype
    with pytest.raises(GdHipError):
        teacher_heads.FusedDPTHead(DL.make_head("a"), dtype=torch.float16)


def test_weights_are_packed_into_the_operand_layout():
    m = DL.make_head("a")
    fill_params(m)
    h = teacher_heads.FusedDPTHead(m)
    w = m.scratch.layer2_rn.weight                                   # [n, c, ky, kx] -> [n, (kx, ky, c)]
    assert h.rn[1][0].shape == (16, 9 * 32) and h.rn[1][0][3, (2 * 3 + 0) * 32 + 5] == w[3, 5, 0, 2]
    wd = m.resize_layers[0].weight                                   # [c, n, ky, kx] -> [(ky, kx, n), c]
    kind, cout, k, packed, bias = h.resize[0]
    assert (kind, cout, k) == ("deconv", 16, 4) and packed.shape == (16 * 16, 16) and packed[(1 * 4 + 3) * 16 + 7, 2] == wd[2, 7, 1, 3]
    assert all(u.inplace for blk in h.fusion for u in blk[:2] if u is not None)
    assert not teacher_heads.FusedDPTHead(DL.make_head("a", inplace_relu=False)).fusion[0][1].inplace


def test_fused_heads_is_off_by_default_and_then_constructs_nothing(monkeypatch):
    class Boom:
        def __init__(self, *a, **k):
            raise AssertionError("FusedDPTHead was constructed")
    monkeypatch.setattr(teacher_heads, "FusedDPTHead", Boom)
    teacher = DL.TinyVGGT()
    r = teacher_runner.VGGTTeacherRunner(teacher, dtype=torch.float32, pose_decoder=DL.tiny_pose_decoder)
    assert r.heads is None and r.fused is None
    with pytest.raises(AssertionError):
        teacher_runner.VGGTTeacherRunner(teacher, dtype=torch.float32, pose_decoder=DL.tiny_pose_decoder, fused_heads=True)


def test_a_refused_head_raises_when_the_runner_is_built(no_hip):
    teacher = DL.TinyVGGT()
    teacher.point_head.activation = "norm_exp"
    with pytest.raises(GdHipError) as e:
        teacher_runner.VGGTTeacherRunner(teacher, dtype=torch.float32, pose_decoder=DL.tiny_pose_decoder, fused_heads=True)
    assert "point_head.activation" in str(e.value)
    teacher.point_head.activation = "inv_log"
    teacher.track_head.feature_extractor.scratch.refinenet1.expand = True
    with pytest.raises(GdHipError) as e:
        teacher_runner.VGGTTeacherRunner(teacher, dtype=torch.float32, pose_decoder=DL.tiny_pose_decoder, fused_heads=True)
    assert "track_head.feature_extractor.scratch.refinenet1.expand" in str(e.value)


def test_feature_extractor_shadow_is_removed_when_the_track_head_raises(monkeypatch, no_hip):
    teacher = DL.TinyVGGT()
    r = teacher_runner.VGGTTeacherRunner(teacher, dtype=torch.float32, pose_decoder=DL.tiny_pose_decoder, fused_heads=True)
    H, W = DL.TinyVGGT.IMG
    # host stand-ins for everything that would reach the GPU: the aggregator's outputs, the two map heads, and the glue (which calls the tracker)
    monkeypatch.setattr(r, "aggregate", lambda rgb: ([torch.zeros(1, 2, 20, 256)] * 4, 5, [(torch.zeros(1, 2, 40, 64),) * 2]))
    r.heads["depth_head"] = lambda toks, img, ps: (torch.ones(1, 2, H, W, 1), torch.ones(1, 2, H, W))
    r.heads["point_head"] = lambda toks, img, ps: (torch.ones(1, 2, H, W, 3), torch.ones(1, 2, H, W))
    monkeypatch.setattr(teacher_runner.tg, "extract_vggt_targets", lambda qk, depth, conf, E, K, track_fn, **kw: track_fn(torch.zeros(3, 2, dtype=torch.int32)))
    fe = teacher.track_head.feature_extractor
    teacher.track_head.fail = True
    with pytest.raises(RuntimeError, match="stub track head failure"):
        r.targets(torch.rand(1, 2, 3, H, W))
    assert teacher.track_head.saw_shadow is True                     # the fused forward was in place while the track head ran
    assert "forward" not in vars(fe) and fe.forward.__func__ is DL.DPTLayout.forward
