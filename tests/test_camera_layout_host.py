"""Host: the camera-head layout (tests/camera_layout.py) against fixture G30 (what the reference's own CameraHead and pose decoding returned,
tools/make_golden_g30.py); FusedCameraHead's acceptance and refusals, at construction, with no device; the runner's new keywords; the four entry
points' argument errors, which fail before any device call."""
import ctypes
import inspect

import pytest
import torch

import camera_layout as CL
from conftest import load_golden


@pytest.fixture(scope="module")
def g30():
    return load_golden("g30_camera_head")


@pytest.mark.parametrize("cfg", list(CL.CONFIGS))
@pytest.mark.parametrize("B,S", CL.SHAPES)
def test_layout_against_reference_fixture(g30, cfg, B, S):
    head = CL.make_head(cfg)
    assert CL.param_layout(head) == g30[f"{cfg}_param_layout"]
    toks = CL.seeded_tokens(cfg, B, S)
    assert torch.equal(toks[-1], g30[f"{cfg}_{B}x{S}_tokens"])
    with torch.no_grad():
        encs = head(toks)
    assert len(encs) == 4
    for it, enc in enumerate(encs):
        E, K = CL.decode_pose(enc, CL.IMAGE_HW)
        for what, got in (("enc", enc), ("extrinsic", E), ("intrinsic", K)):
            want = g30[f"{cfg}_{B}x{S}_{what}_{it}"]
            e, bound = float((got - want).abs().max()), 1e-5 * float(want.abs().max())
            print(f"{cfg} {B}x{S} iteration {it} {what}: e {e:.3e}, bound {bound:.3e}")
            assert got.shape == want.shape and e <= bound, (what, it)
    assert float(head.empty_pose_tokens.detach().abs().min()) > 0 and float(head.trunk[0].ls1.gamma.detach().abs().min()) > 0


# ---------------------------------------------------------------------------------------------------------------------------------- refusals
def _fused(m, **kw):
    import gd_amd  # noqa: F401
    from gd_amd.teacher_heads import FusedCameraHead
    return FusedCameraHead(m, **kw)


@pytest.mark.parametrize("cfg", list(CL.CONFIGS))
def test_fused_head_accepts_the_layout_and_packs_once(cfg):
    m = CL.make_head(cfg)
    D, depth = CL.CONFIGS[cfg]["dim_in"], CL.CONFIGS[cfg]["trunk_depth"]
    f = _fused(m)
    assert f.D == D and len(f.blocks) == depth and f.acts == ["linear", "linear", "relu"]
    assert f.embed[0].shape == (D, 12) and float(f.embed[0][:, 9:].abs().max()) == 0.0 and torch.equal(f.embed[0][:, :9], m.embed_pose.weight)
    assert f.empty.shape == (1, 12) and torch.equal(f.empty[0, :9], m.empty_pose_tokens.reshape(9)) and float(f.empty[0, 9:].abs().max()) == 0.0
    assert f.blocks[0]["H"] == CL.CONFIGS[cfg]["num_heads"] and f.blocks[0]["qkv"][0].dtype == torch.float32
    weights = 12 * D + 3 * D * D + depth * 12 * D * D + D * D // 2 + 9 * (D // 2)
    assert f.weight_bytes == 4 * weights
    h = _fused(m, dtype=torch.bfloat16)
    assert h.blocks[0]["fc2"][0].dtype == torch.bfloat16 and h.modulation[0].dtype == torch.bfloat16 and h.pb1[0].dtype == torch.float32
    assert torch.equal(h.blocks[0]["fc1"][0], m.trunk[0].mlp.fc1.weight.bfloat16()) and h.weight_bytes < f.weight_bytes
    m.trunk[0].ls1 = torch.nn.Identity()                                    # a block without LayerScale is served: gamma = None
    assert _fused(m).blocks[0]["ls1"] is None


class _Rope(torch.nn.Module):
    def forward(self, x, pos):
        return x


def _set(name, value):
    def mutate(m):
        obj, parts = m, name.split(".")
        for p in parts[:-1]:
            obj = obj[int(p)] if p.isdigit() else getattr(obj, p)
        setattr(obj, parts[-1], value)
    return mutate


@pytest.mark.parametrize("mutate,match", [
    (_set("trunk.1.attn.rope", _Rope()), r"camera_head\.trunk\[1\]\.attn\.rope"),
    (_set("trunk.0.attn.q_norm", torch.nn.LayerNorm(16)), r"camera_head\.trunk\[0\]\.attn\.q_norm"),
    (_set("trunk.0.attn.k_norm", torch.nn.LayerNorm(16)), r"camera_head\.trunk\[0\]\.attn\.k_norm"),
    (_set("trunk.1.mlp.act", torch.nn.ReLU()), r"camera_head\.trunk\[1\]\.mlp\.act"),
    (_set("trunk.0.mlp.act", torch.nn.GELU(approximate="tanh")), r"camera_head\.trunk\[0\]\.mlp\.act"),
    (_set("pose_branch.act", torch.nn.ReLU()), r"camera_head\.pose_branch\.act"),
    (_set("target_dim", 8), r"camera_head\.target_dim: 8"),
    (_set("fl_act", "softplus"), r"camera_head\.fl_act: 'softplus'"),
    (_set("trans_act", "tanh"), r"camera_head\.trans_act: 'tanh'"),
    (_set("trunk.0.norm1", torch.nn.LayerNorm(64, elementwise_affine=False)), r"camera_head\.trunk\[0\]\.norm1"),
    (_set("trunk_norm", torch.nn.Identity()), r"camera_head\.trunk_norm"),
    (_set("adaln_norm", torch.nn.LayerNorm(64)), r"camera_head\.adaln_norm"),
    (_set("trunk.0.attn.num_heads", 32), r"camera_head\.trunk\[0\]\.attn\.num_heads: 32: head dimension 2"),
    (_set("trunk.0.attn.num_heads", 7), r"camera_head\.trunk\[0\]\.attn\.num_heads: 7"),
])
def test_fused_head_refuses_what_the_kernels_do_not_serve(mutate, match):
    from gd_amd._lib import GdHipError
    m = CL.make_head("d64")
    _fused(m)                                                                 # accepted as it stands
    mutate(m)
    with pytest.raises(GdHipError, match=match):
        _fused(m)


def test_fused_head_refuses_dropout_only_in_training_mode_and_a_wide_head():
    from gd_amd._lib import GdHipError
    m = CL.make_head("d64")
    m.trunk[0].attn.proj_drop = torch.nn.Dropout(0.1)
    _fused(m.eval())                                                          # eval mode: dropout is the identity
    m.train()
    with pytest.raises(GdHipError, match=r"trunk\[0\]\.attn\.proj_drop: p = 0\.1"):
        _fused(m)
    wide = CL.CameraHeadLayout(dim_in=520, num_heads=1, trunk_depth=1).eval()     # head dimension 520
    with pytest.raises(GdHipError, match=r"trunk\[0\]\.attn\.num_heads: 1: head dimension 520"):
        _fused(wide)
    with pytest.raises(GdHipError, match="dtype"):
        _fused(CL.make_head("d64"), dtype=torch.float16)


def test_fused_head_refuses_host_tokens_and_more_than_eight_rows():
    from gd_amd._lib import GdHipError
    f = _fused(CL.make_head("d64"))
    with pytest.raises(GdHipError, match=r"tokens_list\[-1\] must be a CUDA"):
        f.forward(CL.seeded_tokens("d64", 1, 2))
    with pytest.raises(GdHipError, match=r"tokens_list\[-1\] must be a CUDA"):
        f.poses(CL.seeded_tokens("d64", 3, 3), CL.IMAGE_HW)


# ---------------------------------------------------------------------------------------------------------------------------------- the runner
def test_runner_keywords_and_defaults():
    import gd_amd  # noqa: F401
    from gd_amd._lib import GdHipError
    from gd_amd.teacher_heads import FusedCameraHead
    from gd_amd.teacher_runner import VGGTTeacherRunner
    import dpt_layout as DL
    params = inspect.signature(VGGTTeacherRunner.__init__).parameters
    names = list(params)
    assert params["fused_camera_head"].default is False and params["camera_dtype"].default is torch.float32
    assert params["fused_camera_head"].kind is inspect.Parameter.KEYWORD_ONLY and params["camera_dtype"].kind is inspect.Parameter.KEYWORD_ONLY
    assert names[-1] == "fused_tracker" and names.index("fused_patch_embed") < names.index("fused_camera_head") < names.index("camera_dtype") < names.index("fused_tracker")
    assert inspect.signature(FusedCameraHead.__init__).parameters["dtype"].default is torch.float32
    assert list(inspect.signature(VGGTTeacherRunner.cameras).parameters) == ["self", "tokens_list", "image_hw"]
    vggt = DL.TinyVGGT()
    assert VGGTTeacherRunner(vggt).camera is None                            # the stub camera head is never looked at with the switch off
    CL.attach_camera_head(vggt, CL.CameraHeadLayout(dim_in=256, num_heads=2, trunk_depth=1).eval())
    r = VGGTTeacherRunner(vggt, fused_camera_head=True, camera_dtype=torch.bfloat16)
    assert isinstance(r.camera, FusedCameraHead) and r.camera.dtype == torch.bfloat16 and r.camera.name == "camera_head"
    vggt.camera_head.trunk[0].attn.rope = _Rope()
    VGGTTeacherRunner(vggt)
    with pytest.raises(GdHipError, match=r"camera_head\.trunk\[0\]\.attn\.rope"):    # in the constructor, not in targets()
        VGGTTeacherRunner(vggt, fused_camera_head=True)


def test_runner_cameras_with_the_switch_off_is_the_module_then_the_decoder():
    import gd_amd  # noqa: F401
    from gd_amd.teacher_runner import VGGTTeacherRunner
    import dpt_layout as DL
    vggt = DL.TinyVGGT()
    CL.attach_camera_head(vggt, CL.make_head("d256"))
    toks, calls = CL.seeded_tokens("d256", 1, 2), []
    hook = vggt.camera_head.register_forward_hook(lambda mod, a, out: calls.append(1))
    seen = []

    def dec(enc, hw):
        seen.append((enc, tuple(hw)))
        return CL.decode_pose(enc, hw)
    E, K = VGGTTeacherRunner(vggt, pose_decoder=dec).cameras(toks, CL.IMAGE_HW)
    hook.remove()
    with torch.no_grad():
        want = vggt.camera_head(toks)[-1]
    assert calls == [1] and len(seen) == 1 and torch.equal(seen[0][0], want) and seen[0][1] == CL.IMAGE_HW
    We, Wk = CL.decode_pose(want, CL.IMAGE_HW)
    assert torch.equal(E, We) and torch.equal(K, Wk)


# ---------------------------------------------------------------------------------------------------------------------------------- entry points
@pytest.fixture(scope="module")
def L():
    import gd_amd  # noqa: F401
    from gd_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def arena():
    buf = ctypes.create_string_buffer(1 << 21)                                # never dereferenced: every call below is refused before a launch
    return buf, (ctypes.addressof(buf) + 4095) & ~4095


def test_rows_linear_checks_its_arguments_before_any_device_call(L, arena):
    from gd_amd._lib import BF16, F32
    _, a = arena
    err = lambda: L.gd_last_error().decode()
    x, w, y, r = a, a + (1 << 16), a + (1 << 20), a + (1 << 20) + (1 << 16)

    def call(x=x, w=w, wt=F32, y=y, M=2, N=8, K=16, ldx=16, ldw=16, ldy=8, bias=None, res=None, ldr=0, gamma=None, pro=0, act=0):
        return L.gd_rows_linear(x, w, wt, y, M, N, K, ldx, ldw, ldy, bias, res, ldr, gamma, pro, act, None)
    assert call(M=9) != 0 and "M = 9" in err()
    assert call(M=0) != 0 and "M = 0" in err()
    assert call(N=0) != 0 and "N = 0" in err()
    assert call(K=6, ldx=8, ldw=8) != 0 and "K = 6" in err() and "multiple of 4" in err()
    assert call(wt=BF16, K=12, ldx=12, ldw=16) != 0 and "K = 12" in err() and "multiple of 8 for bf16" in err()
    assert call(wt=2) != 0 and "w_dtype 2" in err()
    assert call(ldw=12) != 0 and "ldw = 12" in err() and ">= K = 16" in err()
    assert call(ldx=18, K=16) != 0 and "ldx = 18" in err()
    assert call(ldy=4) != 0 and "ldy = 4" in err() and ">= N = 8" in err()
    assert call(M=8, K=2052, ldx=2052, ldw=2052) != 0 and "M * K = 8 * 2052 = 16416" in err()
    assert call(M=2, K=8196, ldx=8196, ldw=8196) != 0 and "16392" in err()
    assert call(x=x + 4) != 0 and "x " in err() and "16-byte aligned" in err()
    assert call(w=w + 8) != 0 and "w " in err() and "16-byte aligned" in err()
    assert call(y=y + 4) != 0 and "y " in err() and "16-byte aligned" in err()
    assert call(y=x) != 0 and "overlaps x" in err()
    assert call(y=x + 48, M=1) != 0 and "overlaps x" in err()                 # y's 8 floats start inside x's one row of 16
    assert call(y=w + 16 * 4 * 7) != 0 and "overlaps w" in err()              # inside w's last row
    assert call(res=y + 16, ldr=8) != 0 and "overlaps residual" in err()      # shifted by four columns: neither disjoint nor in place
    assert call(res=y, ldr=12) != 0 and "overlaps residual" in err()          # the same pointer, another stride
    assert call(gamma=r) != 0 and "gamma is given without a residual" in err()
    assert call(x=None) != 0 and "required" in err()
    assert call(pro=2) != 0 and "prologue 2" in err()
    assert call(act=3) != 0 and "activation 3" in err()


def test_rows_attention_adaln_and_pose_check_their_arguments_before_any_device_call(L, arena):
    _, a = arena
    err = lambda: L.gd_last_error().decode()
    q, o = a, a + (1 << 20)
    f = ctypes.c_float

    def attn(q=q, o=o, B=1, S=2, H=2, hd=8, ld=48, ldo=16):
        return L.gd_rows_attention(q, o, B, S, H, hd, ld, ldo, f(0.5), None)
    assert attn(S=9) != 0 and "S = 9" in err()
    assert attn(S=0) != 0 and "S = 0" in err()
    for hd in (260, 0, 6):
        assert attn(hd=hd, ld=3 * 2 * 260, ldo=2 * 260) != 0 and f"head_dim {hd}" in err()
    assert attn(ld=44) != 0 and "ld = 44" in err()
    assert attn(ldo=12) != 0 and "ldo = 12" in err()
    assert attn(q=q + 4) != 0 and "16-byte aligned" in err()
    assert attn(o=q + 4 * 48) != 0 and "o overlaps qkv" in err()
    assert attn(q=None) != 0 and "required" in err()

    def adaln(x=q, mod=a + (1 << 16), out=o, M=2, D=8, ldx=8, ldm=24, ldo=8):
        return L.gd_adaln_modulate(x, mod, out, M, D, ldx, ldm, ldo, f(1e-6), None)
    assert adaln(D=6) != 0 and "D = 6" in err()
    assert adaln(D=8196, ldx=8196, ldm=3 * 8196, ldo=8196) != 0 and "D = 8196" in err()
    assert adaln(ldm=20) != 0 and "ldm = 20" in err()
    assert adaln(out=q + 16) != 0 and "out overlaps x" in err()                # four columns in: neither disjoint nor x itself
    assert adaln(out=a + (1 << 16)) != 0 and "out overlaps mod" in err()
    assert adaln(x=q + 4) != 0 and "16-byte aligned" in err()
    assert adaln(M=0) != 0 and "M = 0" in err()

    def pose(delta=q, ldd=12, raw=a + (1 << 16), enc=o, E=None, K=None, M=2, first=1, acts=(0, 0, 3), H=0, W=0):
        return L.gd_pose_update(delta, ldd, raw, enc, E, K, M, first, *acts, H, W, None)
    assert pose(ldd=8) != 0 and "ldd = 8" in err()
    assert pose(acts=(0, 4, 3)) != 0 and "quat_act = 4" in err()
    assert pose(acts=(0, 0, -1)) != 0 and "fl_act = -1" in err()
    assert pose(E=o + 4096) != 0 and "both extrinsic and intrinsic" in err()
    assert pose(E=o + 4096, K=o + 8192, H=0, W=70) != 0 and "H = 0" in err()
    assert pose(M=0) != 0 and "M = 0" in err()
    assert pose(raw=None) != 0 and "required" in err()
    assert pose(delta=q + 2) != 0 and "4-byte aligned" in err()


def test_wrappers_refuse_host_tensors_and_bad_views():
    import gd_amd  # noqa: F401
    from gd_amd import ops
    from gd_amd._lib import GdHipError
    x, w = torch.zeros(2, 16), torch.zeros(8, 16)
    with pytest.raises(GdHipError, match="rows_linear: x must be a CUDA fp32 view"):
        ops.rows_linear(x, w)
    with pytest.raises(GdHipError, match="rows_linear: x must be a CUDA fp32 view"):
        ops.rows_linear(x.T, w)
    with pytest.raises(GdHipError, match="rows_attention: qkv must be a CUDA fp32 view"):
        ops.rows_attention(torch.zeros(2, 48), 1, 2, 2)
    with pytest.raises(GdHipError, match="adaln_modulate: x must be a CUDA fp32 view"):
        ops.adaln_modulate(x, torch.zeros(2, 48))
    with pytest.raises(GdHipError, match="pose_update: delta must be a CUDA fp32 view"):
        ops.pose_update(torch.zeros(2, 9), torch.zeros(2, 12), True)
    assert ops.ROWS_MAX_M == 8 and ops.ROWS_LDS_FLOATS == 16384 and ops.POSE_ACTS == {"linear": 0, "inv_log": 1, "exp": 2, "relu": 3}
