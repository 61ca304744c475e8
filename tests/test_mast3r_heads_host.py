"""CPU: teacher_heads.FusedMASt3RHead's host side — every refusal (raised while the module is read, before any HIP call, naming the attribute), the
packed order of the local-feature MLP's last layer against F.pixel_shuffle, the C entry point's guards, and MASt3RTeacherRunner's `fused_heads`
switch: off by default, a refused head raises at construction, and the instance attributes that shadow the two heads' `forward` are gone after
`targets()`, also when the teacher's forward raises."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mast3r_head_layout as ML
from test_dpt_heads_host import _set
from test_teacher_runner_ref import fill_params

import gd_amd  # noqa: F401
from gd_amd import _lib, ops, teacher_heads, teacher_runner
from gd_amd._lib import GdHipError

INF = float("inf")


@pytest.fixture
def no_hip(monkeypatch):
    """Any call into the library fails the test: what runs under this fixture is host logic only."""
    def boom():
        raise AssertionError("a HIP entry point was reached")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(ops, "lib", boom)


REFUSALS = {
    "width_ratio": (_set("dpt.scratch.refinenet2.width_ratio", 2), {}, "dpt.scratch.refinenet2.width_ratio", "served is 1"),
    "batch_norm": (_set("dpt.scratch.refinenet3.resConfUnit2.bn", True), {}, "dpt.scratch.refinenet3.resConfUnit2.bn", "batch-norm"),
    "unit_activation": (_set("dpt.scratch.refinenet1.resConfUnit1.activation", nn.GELU()), {}, "dpt.scratch.refinenet1.resConfUnit1.activation", "ReLU"),
    "postprocess_three_layers": (_set("dpt.act_postprocess.2", nn.Sequential(nn.Conv2d(48, 384, 1), nn.ReLU(), nn.Conv2d(384, 384, 1))), {},
                                 "dpt.act_postprocess[2]", "Sequential(Conv2d 1x1"),
    "postprocess_not_1x1": (_set("dpt.act_postprocess.2", nn.Sequential(nn.Conv2d(48, 384, 3, padding=1))), {}, "dpt.act_postprocess[2][0]", "kernel 1"),
    "postprocess_deconv_stride": (_set("dpt.act_postprocess.0.1", nn.ConvTranspose2d(96, 96, 4, stride=2, padding=1)), {}, "dpt.act_postprocess[0][1]",
                                  "kernel = stride"),
    "postprocess_conv_stride": (_set("dpt.act_postprocess.3.1", nn.Conv2d(768, 768, 3, stride=1, padding=1)), {}, "dpt.act_postprocess[3][1]", "stride 2"),
    "postprocess_kind": (_set("dpt.act_postprocess.1.1", nn.Upsample(scale_factor=2)), {}, "dpt.act_postprocess[1][1]", "Upsample"),
    "layer_dims_not_8": (None, dict(layer_dims=(12, 192, 384, 768)), "dpt.act_postprocess[0][0]", "multiples of 8"),
    "features_not_8": (None, dict(feature_dim=24), "dpt.head[0]", "multiples of 8"),
    "last_dim_not_8": (None, dict(last_dim=12), "dpt.head[2]", "multiples of 8"),
    "bounded_depth": (None, dict(depth_mode=("exp", -INF, 100.0)), "depth_mode", "bounded"),
    "depth_kind": (None, dict(depth_mode=("cube", -INF, INF)), "depth_mode", "cube"),
    "no_postprocess": (_set("postprocess", None), {}, "postprocess", "missing"),
    "conf_kind": (None, dict(conf_mode=("softplus", 0, INF)), "conf_mode", "softplus"),
    "desc_mode": (None, dict(desc_mode="raw"), "desc_mode", "norm"),
    "one_conf_without_conf": (None, dict(has_conf=False, conf_mode=None, two_confs=False), "two_confs", "does not have"),
    "channels_against_conf_mode": (None, dict(has_conf=False), "dpt.head[4]", "3 output channels"),
    "interpolate": (_set("dpt.head.1", ML.Interpolate(2, "nearest", None)), {}, "dpt.head", "Interpolate(scale_factor=2"),
    "gelu_form": (_set("head_local_features.act", nn.GELU(approximate="tanh")), {}, "head_local_features.act", "erf"),
    "fc2_width": (_set("head_local_features.fc2", nn.Linear(448, 24 * 256)), {}, "head_local_features.fc2", "patch_size^2"),
    "hooks": (_set("dpt.hooks", [0, 6, 12]), {}, "dpt.hooks", "four levels"),
    "semseg": (_set("dpt.head_type", "semseg"), {}, "dpt.head_type", "regression"),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals_name_the_attribute(what, dtype, no_hip):
    mutate, over, attr, word = REFUSALS[what]
    m = ML.make_head("a", **dict(dict(local_feat_dim=24), **over))
    if mutate is not None:
        mutate(m)
    with pytest.raises(GdHipError) as e:
        teacher_heads.FusedMASt3RHead(m, dtype=dtype, name="downstream_head1")
    print(e.value)
    assert f"FusedMASt3RHead: downstream_head1.{attr}:" in str(e.value) and word in str(e.value)


def test_served_heads_construct_without_a_hip_call(no_hip):
    for case, cfg in ML.CASES.items():
        for dtype in (torch.float32, torch.bfloat16):
            h = teacher_heads.FusedMASt3RHead(ML.make_head(case), dtype=dtype)
            assert (h.od, h.D, h.two_confs, h.pts_mode) == (3 + cfg["has_conf"], cfg["local_feat_dim"], cfg["two_confs"], cfg["depth_mode"][0])
            assert h.rn[0][0].dtype == h.fc1[0].dtype == h.fc2[0].dtype == dtype and h.fc2[1].dtype == h.w_last.dtype == torch.float32
            assert [r[0] for r in h.resize] == ["deconv", "deconv", "identity", "conv_s2"] and h.hooks == ML.HOOKS
            # refinenet4's resConfUnit1 exists in the module and is ignored; every unit rectifies out of place
            assert h.fusion[3][0] is None and all(u is not None and not u.inplace for blk in h.fusion[:3] for u in blk[:2])
    assert teacher_heads.FusedMASt3RHead(ML.make_head("b")).desc_conf_mode == ("sigmoid", 0.0, 5.0)          # None: the confidence's own mode
    with pytest.raises(GdHipError):
        teacher_heads.FusedMASt3RHead(ML.make_head("a"), dtype=torch.float16)


@pytest.mark.parametrize("patch,n", [(16, 25), (2, 3), (1, 4)])
def test_packed_last_layer_realises_pixel_shuffle_by_addressing(patch, n):
    """fc2's rows in the order (i, j, c): element ((i * P + j) * n + c) of token (ty, tx)'s packed output is what F.pixel_shuffle puts at channel c of
    pixel (ty * P + i, tx * P + j)."""
    B, gh, gw, K = 2, 2, 3, 8
    g = torch.Generator().manual_seed(patch)
    fc2 = nn.Linear(K, n * patch * patch)
    x = torch.randn(B, gh * gw, K, generator=g)
    with torch.no_grad():
        want = F.pixel_shuffle(fc2(x).transpose(-1, -2).reshape(B, -1, gh, gw), patch)                 # [B, n, H, W], as the module computes it
        w, b = teacher_heads.pack_pixel_shuffle(fc2.weight, patch), teacher_heads.pack_pixel_shuffle(fc2.bias, patch)
        rows = x.reshape(B * gh * gw, K) @ w.T + b                                                     # token rows, columns (i, j, c)
    got = rows.reshape(B, gh, gw, patch, patch, n).permute(0, 5, 1, 3, 2, 4).reshape(B, n, gh * patch, gw * patch)
    assert w.shape == fc2.weight.shape and b.shape == fc2.bias.shape and torch.allclose(got, want, atol=1e-6, rtol=0)
    assert torch.equal(w[(1 % patch * patch + 0) * n + (n - 1)], fc2.weight[(n - 1) * patch * patch + (1 % patch) * patch])
    m = ML.make_head("c")
    fill_params(m)
    h = teacher_heads.FusedMASt3RHead(m)
    assert torch.equal(h.fc2[0][(3 * 16 + 5) * 25 + 7], m.head_local_features.fc2.weight[7 * 256 + 3 * 16 + 5])
    assert h.fc2[1][(3 * 16 + 5) * 25 + 7] == m.head_local_features.fc2.bias[7 * 256 + 3 * 16 + 5]


def test_entry_point_guards_fail_loudly_without_touching_the_device():
    L = _lib.lib()
    f = ctypes.c_float
    lf = ctypes.c_void_p(64)            # never dereferenced: every call below is refused before the launch

    def call(Cin=128, od=4, P=16, D=24, tc=1, H=32, W=32, frames=1, lf=lf, pts=2, conf=0, desc=0, dconf=0):
        return L.gd_mast3r_head_out(None, None, None, lf, None, None, None, None, frames, H, W, Cin, od, P, D, tc, pts, conf, f(1), f(INF), desc, dconf,
                                    f(0), f(INF), None)
    for kw, word in ((dict(Cin=12), b"multiple of 8"), (dict(od=5), b"output channels"), (dict(od=2), b"output channels"), (dict(P=0), b"patch size"),
                     (dict(P=32), b"patch size"), (dict(D=0), b"descriptor channels"), (dict(D=33), b"descriptor channels"), (dict(tc=2), b"two_confs"),
                     (dict(H=24), b"whole number"), (dict(frames=0), b"bad shape"), (dict(H=46352, W=46352), b"2^31"), (dict(pts=3), b"pts3d mode"),
                     (dict(conf=3), b"confidence mode"), (dict(desc=2), b"descriptor mode"), (dict(dconf=-1), b"desc_conf mode"),
                     (dict(od=3, tc=0), b"does not have"), (dict(), b"null pointer"), (dict(lf=None, P=0, D=0), b"null pointer")):
        assert call(**kw) != 0 and word in L.gd_last_error(), (kw, L.gd_last_error())


# ----------------------------------------------------------------------------------------------------------------------------------
# the runner
# ----------------------------------------------------------------------------------------------------------------------------------
KW = dict(inference=ML.inference, make_pairs=ML.make_pairs)


def test_fused_heads_is_off_by_default_and_then_constructs_nothing(monkeypatch):
    class Boom:
        def __init__(self, *a, **k):
            raise AssertionError("FusedMASt3RHead was constructed")
    monkeypatch.setattr(teacher_heads, "FusedMASt3RHead", Boom)
    m = ML.tiny_matcher()
    r = teacher_runner.MASt3RTeacherRunner(m, **KW)
    assert r.heads is None and r.fused is None
    with pytest.raises(AssertionError):
        teacher_runner.MASt3RTeacherRunner(m, fused_heads=True, **KW)


def test_a_refused_head_raises_when_the_runner_is_built(no_hip):
    m = ML.tiny_matcher()
    m.downstream_head2.dpt.scratch.refinenet1.width_ratio = 1.5
    with pytest.raises(GdHipError) as e:
        teacher_runner.MASt3RTeacherRunner(m, fused_heads=True, **KW)
    assert "downstream_head2.dpt.scratch.refinenet1.width_ratio" in str(e.value)
    m.downstream_head2.dpt.scratch.refinenet1.width_ratio = 1
    r = teacher_runner.MASt3RTeacherRunner(m, fused_heads=True, heads_dtype=torch.bfloat16, **KW)
    assert sorted(r.heads) == ["downstream_head1", "downstream_head2"] and r.heads["downstream_head2"].dtype == torch.bfloat16 and r.fused is None


def test_head_shadows_drive_the_users_forward_and_are_removed(monkeypatch, no_hip):
    m = ML.tiny_matcher()
    r = teacher_runner.MASt3RTeacherRunner(m, fused_heads=True, min_conf_thr=0, subsample=8, **KW)
    calls = []

    class HostHead:
        """a host stand-in for the fused head: the module's own forward, noting that it was reached through the shadow"""
        def __init__(self, name):
            self.name = name

        def forward(self, decout, img_shape):
            mod = getattr(m, self.name)
            calls.append((self.name, "forward" in vars(mod)))
            return type(mod).forward(mod, decout, img_shape)
    for n in r.heads:
        r.heads[n] = HostHead(n)
    seen = {}
    monkeypatch.setattr(teacher_runner.tg, "extract_mast3r_targets", lambda *a, **k: seen.update(desc=a[0], k=k) or "targets")
    img = torch.rand(1, 3, ML.IMG_H, ML.IMG_W, generator=torch.Generator().manual_seed(1))
    assert r.targets(img, img, device="cpu") == "targets"
    assert calls == [("downstream_head1", True), ("downstream_head2", True)] and seen["desc"].shape == (ML.IMG_H, ML.IMG_W, 24)
    heads = (m.downstream_head1, m.downstream_head2)
    assert all("forward" not in vars(h) and h.forward.__func__ is ML.MASt3RHeadLayout.forward for h in heads)
    # the teacher's forward raises: the shadows were in place while it ran, and are gone afterwards
    m.fail = True
    with pytest.raises(RuntimeError, match="stub matcher failure"):
        r.targets(img, img, device="cpu")
    assert m.saw_shadow == [True, True]
    assert all("forward" not in vars(h) and h.forward.__func__ is ML.MASt3RHeadLayout.forward for h in heads)
