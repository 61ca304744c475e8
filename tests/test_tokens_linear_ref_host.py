"""Host: the fp64 restatement of gd_tokens_linear (tests/tokens_linear_ref64.py).  On every case of the table the GPU test uses, (a) the same
expression evaluated in fp32 on the CPU stays inside the derived bound — the bound is not tighter than fp32 arithmetic itself, whatever the summation
order — and (b) each deliberate mistake (MUTANTS) breaks the bound by a factor of at least 4 on every case it applies to, and applies to at least one.
Then the entry point's argument checks (no device is touched: every call fails before its launch) and the new keywords of the three constructors."""
import ctypes
import inspect

import pytest
import torch

import tokens_linear_ref64 as R


def worst(got, want, bound):
    return float(((got.double() - want.double()).abs() / bound).max())


def lin(c, mutant=None, dtype=torch.float64):
    i = R.inputs(c)
    return R.linear64(i["x"], i["w"], i["bias"], i["residual"], i["y0"], c["gelu"], c["accumulate"], mutant=mutant, dtype=dtype)


@pytest.mark.parametrize("c", R.CASES, ids=R.IDS)
def test_fp32_evaluation_is_inside_the_bound(c):
    want, bound = lin(c)
    got, _ = lin(c, dtype=torch.float32)
    r = worst(got, want, bound)
    print(f"tokens_linear fp32 CPU vs fp64: worst err / bound {r:.3f}")
    assert got.dtype == torch.float32 and r <= 1.0


@pytest.mark.parametrize("c", R.CASES, ids=R.IDS)
def test_mutants_break_the_bound(c):
    want, bound = lin(c)
    for m in R.MUTANTS:
        if R.mutant_applies(c, m):
            r = worst(lin(c, m)[0], want, bound)
            print(f"tokens_linear mutant {m}: worst err / bound {r:.1f}")
            assert r >= 4.0, m
        else:
            assert torch.equal(lin(c, m)[0], want), m


def test_every_mutant_every_epilogue_and_every_constant_is_in_the_table():
    for m in R.MUTANTS:
        assert any(R.mutant_applies(c, m) for c in R.CASES), m
    assert len(R.MUTANTS) == 7
    forms = {(c["bias"], c["gelu"], c["residual"], c["accumulate"]) for c in R.CASES}
    # qkv / q / kv / input_transform / flow_head; fc1; out_proj and fc2; fc2 of a last block; ffeat_updater
    assert {(True, False, False, False), (True, True, False, False), (True, False, True, False), (True, False, True, True), (True, True, True, False)} <= forms
    shapes = {(c["M"], c["N"], c["K"]) for c in R.CASES}
    assert {(1, 1, 4), (9, 36, 12), (31, 31, 16), (32, 32, 60), (33, 33, 64), (65, 4, 68), (40, 130, 388), (128, 96, 384), (50, 96, 1536), (600, 128, 128)} <= shapes
    assert any(R.tall_tiles(c) for c in R.CASES) and not all(R.tall_tiles(c) for c in R.CASES)
    assert sum(1 for c in R.CASES if any(c["pads"])) >= 4
    assert all(c["K"] % 4 == 0 for c in R.CASES)


# ---------------------------------------------------------------------------------------------------------------------------------- argument checks
X, W, Y, RES, BIAS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000        # never dereferenced: every call below fails before its launch


def _call(**kw):
    import gd_amd  # noqa: F401
    from gd_amd import _lib
    a = dict(x=X, w=W, y=Y, M=40, N=36, K=24, ldx=24, ldw=24, ldy=36, bias=BIAS, gelu=0, residual=RES, ldr=36, accumulate=0)
    a.update(kw)
    L = _lib.lib()
    rc = L.gd_tokens_linear(a["x"], a["w"], a["y"], a["M"], a["N"], a["K"], a["ldx"], a["ldw"], a["ldy"], a["bias"], a["gelu"], a["residual"], a["ldr"],
                            a["accumulate"], None)
    return rc, L.gd_last_error().decode()


@pytest.mark.parametrize("kw,name", [
    (dict(x=None), "x is null"), (dict(w=None), "w is null"), (dict(y=None), "y is null"),
    (dict(M=0), "M = 0"), (dict(N=0), "N = 0"), (dict(N=-3), "N = -3"),
    (dict(K=0), "K = 0"), (dict(K=22, ldx=24), "K = 22"), (dict(K=2), "K = 2"),
    (dict(x=X + 4), "x 0x"), (dict(w=W + 8), "w 0x"), (dict(y=Y + 4), "y 0x"), (dict(bias=BIAS + 4), "bias 0x"), (dict(residual=RES + 8), "residual 0x"),
    (dict(ldx=20), "ldx = 20"), (dict(ldx=26), "ldx = 26"), (dict(ldw=20), "ldw = 20"), (dict(ldw=30), "ldw = 30"),
    (dict(ldy=32), "ldy = 32"), (dict(ldy=38), "ldy = 38"), (dict(ldr=32), "ldr = 32"), (dict(ldr=38), "ldr = 38"),
    (dict(y=X + 16 * 24), "overlaps x"), (dict(x=Y + 39 * 36 * 4), "overlaps x"), (dict(y=W + 35 * 24 * 4 + 80), "overlaps w"),
    (dict(residual=Y + 16), "overlaps residual"), (dict(residual=Y, ldr=40), "overlaps residual"),
    (dict(gelu=2), "gelu 2"), (dict(accumulate=-1), "accumulate -1"),
])
def test_argument_checks_name_the_argument_without_touching_the_device(kw, name):
    rc, msg = _call(**kw)
    print(f"{kw}: rc {rc}, {msg!r}")
    assert rc != 0 and msg.startswith("gd_tokens_linear: ") and name in msg, (kw, msg)


def test_wrapper_refuses_before_the_library_is_called():
    import gd_amd  # noqa: F401
    from gd_amd import ops
    from gd_amd._lib import GdHipError
    with pytest.raises(GdHipError, match="tokens_linear: x must be a CUDA fp32"):
        ops.tokens_linear(torch.zeros(4, 8), torch.zeros(4, 8))


# ---------------------------------------------------------------------------------------------------------------------------------- the switches
def test_constructor_keywords_and_defaults():
    import gd_amd  # noqa: F401
    import dpt_layout as DL
    import tracker_layout as TL
    from gd_amd._lib import GdHipError
    from gd_amd.teacher_runner import VGGTTeacherRunner
    from gd_amd.teacher_tracker import FusedTracker, FusedUpdateFormer
    for cls, kw in ((FusedUpdateFormer, "linear"), (FusedTracker, "linear"), (VGGTTeacherRunner, "tracker_linear")):
        p = inspect.signature(cls.__init__).parameters[kw]
        assert p.default == "gemm_nt" and p.kind is inspect.Parameter.KEYWORD_ONLY, cls.__name__
    names = list(inspect.signature(VGGTTeacherRunner.__init__).parameters)
    assert names[-1] == "fused_tracker" and names.index("fused_patch_embed") < names.index("fused_camera_head") < names.index("camera_dtype") < \
        names.index("tracker_linear") < names.index("fused_tracker")
    assert list(inspect.signature(FusedUpdateFormer.__init__).parameters)[:3] == ["self", "former", "name"]
    assert list(inspect.signature(FusedTracker.__init__).parameters)[:4] == ["self", "tracker", "name", "fused_updateformer"]
    trk = TL.make_tracker("a")
    assert FusedUpdateFormer(trk.updateformer).linear == "gemm_nt" and FusedUpdateFormer(trk.updateformer, linear="tokens").linear == "tokens"
    plain, both = FusedTracker(trk), FusedTracker(trk, fused_updateformer=True, linear="tokens")
    assert plain.linear == "gemm_nt" and both.linear == "tokens" and both.updateformer.linear == "tokens"
    assert FusedTracker(trk, linear="tokens").updateformer is trk.updateformer          # the user's module stays unless fused_updateformer
    assert FusedTracker(trk, fused_updateformer=True).updateformer.linear == "gemm_nt"
    for make in (lambda: FusedUpdateFormer(trk.updateformer, linear="rocblas"), lambda: FusedTracker(trk, linear="split_k"),
                 lambda: FusedTracker(trk, fused_updateformer=True, linear=None)):
        with pytest.raises(GdHipError, match="linear = "):
            make()
    vggt = TL.make_tiny_vggt()
    r = VGGTTeacherRunner(vggt, pose_decoder=DL.tiny_pose_decoder, fused_updateformer=True, tracker_linear="tokens", fused_tracker=True)
    assert r.tracker.linear == "tokens" and r.tracker.updateformer.linear == "tokens"
    assert VGGTTeacherRunner(vggt, pose_decoder=DL.tiny_pose_decoder, fused_tracker=True).tracker.linear == "gemm_nt"
    with pytest.raises(GdHipError, match="tracker_linear='tokens' needs fused_tracker=True"):
        VGGTTeacherRunner(vggt, pose_decoder=DL.tiny_pose_decoder, tracker_linear="tokens")
    with pytest.raises(GdHipError, match="linear = 'other'"):
        VGGTTeacherRunner(vggt, pose_decoder=DL.tiny_pose_decoder, tracker_linear="other", fused_tracker=True)
