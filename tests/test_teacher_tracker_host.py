"""CPU: the host side of the fused tracker (gd_amd.teacher_tracker, csrc/vggt_track.hip's argument checks) and the fp64 restatement the GPU tests use.
  * tests/track_corr_ref64.py (integer window, zero mask, shared fraction, transposed order) against the layout's correlation class — the reference's
    form, full volume + grid_sample — in fp64: 1e-12 relative (measured 4e-15 to 3e-14);
  * the restatement's expected output covers what it is meant to check: every window offset is non-zero somewhere, at least half of all entries are;
  * FusedTracker refuses by attribute name what the kernels do not serve, and a pyramid level with a side of 1;
  * the runner's and the head's new keywords default to off;
  * the new entry points' argument checks fail without touching the device."""
import ctypes
import inspect

import pytest
import torch

import track_corr_ref64 as R64
import tracker_layout as TL


def first_iteration(case, dtype=torch.float64):
    """(pyramid maps channel-last [levels] x [B*S, H_l, W_l, C], targets [B, S, N, C], coords [B, S, N, 2]) as the first iteration sees them;
    frames s > 0 are moved off the query by a seeded sub-cell offset so that the frames differ."""
    trk = TL.make_tracker(case).to(dtype)
    q, fmaps = TL.seeded_inputs(case)
    with torch.no_grad():
        st = trk.prepare(q.to(dtype), fmaps.to(dtype))
    coords = st["coords"].clone()
    coords[:, 1:] += torch.rand(coords[:, 1:].shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64).to(dtype) * 2 - 1
    return st["pyramid"], st["feats"], coords


@pytest.mark.parametrize("case", list(TL.CASES))
def test_restatement_matches_the_volume_form_in_fp64(case):
    pyr, targets, coords = first_iteration(case)
    want = pyr.sample(targets, coords)
    got, A = R64.corr_sample64([R64.nchw_to_cl(m) for m in pyr.maps], targets, coords, TL.RADIUS)
    assert got.shape == want.shape == A.shape
    e = float((got - want).abs().max()) / float(want.abs().max())
    print(f"{case}: fused formulation vs volume + grid_sample in fp64: {e:.1e} relative")
    assert e <= 1e-12
    assert bool((A >= got.abs() * (1 - 1e-12)).all())


def test_restatement_pools_as_avg_pool2d_does_and_level_sizes_agree():
    """The truth the GPU pooling test relies on (R64.pool2_64 / pyramid32) against F.avg_pool2d, and teacher_tracker.level_sizes — what the size-1
    refusal is decided from — against the sizes that pooling really produces."""
    import gd_amd  # noqa: F401
    from gd_amd.teacher_tracker import level_sizes
    m = torch.randn(2, 7, 9, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    want = torch.nn.functional.avg_pool2d(m.permute(0, 3, 1, 2), 2, stride=2).permute(0, 2, 3, 1)
    assert R64.pool2_64(m).shape == (2, 3, 4, 4) and float((R64.pool2_64(m) - want).abs().max()) <= 1e-15
    pyr = R64.pyramid32(m.float(), 3)
    assert [tuple(p.shape[1:3]) for p in pyr] == [(7, 9), (3, 4), (1, 2)] and all(p.dtype == torch.float32 for p in pyr)
    assert level_sizes(7, 9, 3) == [tuple(p.shape[1:3]) for p in pyr]
    big = R64.pyramid32(torch.zeros(1, 131, 139, 1), 7)
    assert level_sizes(131, 139, 7) == [tuple(p.shape[1:3]) for p in big]


@pytest.mark.parametrize("case", ["a", "b"])
def test_expected_output_covers_every_window_offset(case):
    pyr, targets, coords = first_iteration(case)
    want, _ = R64.corr_sample64([R64.nchw_to_cl(m) for m in pyr.maps], targets, coords, TL.RADIUS)
    win = (2 * TL.RADIUS + 1) ** 2
    nz = want.reshape(-1, len(pyr.maps), win) != 0
    for l, m in enumerate(pyr.maps):
        if min(m.shape[-2:]) >= 2 * TL.RADIUS + 1:
            assert bool(nz[:, l].any(0).all()), f"level {l}: a window offset is zero for every point"
    share = float(nz.double().mean())
    print(f"{case}: {100 * share:.0f} % of the expected entries are non-zero")
    assert share >= 0.5
    assert bool((~nz).any())            # and the zero mask is exercised too


# ---------------------------------------------------------------------------------------------------------------------------------- refusals
def _refused(mutate, match):
    import gd_amd  # noqa: F401
    from gd_amd._lib import GdHipError
    from gd_amd.teacher_tracker import FusedTracker
    trk = TL.make_tracker("a")
    mutate(trk)
    with pytest.raises(GdHipError, match=match):
        FusedTracker(trk)


def _del(name):
    def f(t):
        if name in t._parameters:
            t._parameters[name] = None
        else:
            t._modules[name] = None
    return f


@pytest.mark.parametrize("mutate,match", [
    (lambda t: setattr(t, "latent_dim", 64), r"tracker\.latent_dim"),
    (lambda t: setattr(t, "corr_radius", 5), r"tracker\.corr_radius"),
    (lambda t: setattr(t, "corr_levels", 9), r"tracker\.corr_levels"),
    (lambda t: setattr(t, "fmap_norm", torch.nn.LayerNorm(128, elementwise_affine=False)), r"tracker\.fmap_norm"),
    (lambda t: setattr(t, "fmap_norm", torch.nn.LayerNorm(64)), r"tracker\.fmap_norm"),
    (lambda t: setattr(t, "ffeat_norm", torch.nn.GroupNorm(1, 128, affine=False)), r"tracker\.ffeat_norm"),
    (lambda t: setattr(t, "ffeat_norm", torch.nn.GroupNorm(2, 128)), r"tracker\.ffeat_norm"),
    (lambda t: setattr(t.corr_mlp, "act", torch.nn.GELU(approximate="tanh")), r"tracker\.corr_mlp\.act"),
    (lambda t: setattr(t.corr_mlp, "act", torch.nn.ReLU()), r"tracker\.corr_mlp\.act"),
    (lambda t: t.ffeat_updater.__setitem__(1, torch.nn.ReLU()), r"tracker\.ffeat_updater\[1\]"),
    (lambda t: setattr(t.corr_mlp, "fc1", torch.nn.Linear(100, TL.HIDDEN)), r"tracker\.corr_mlp"),
    (_del("updateformer"), r"tracker\.updateformer"),
    (_del("query_ref_token"), r"tracker\.query_ref_token"),
    (_del("vis_predictor"), r"tracker\.vis_predictor"),
    (_del("conf_predictor"), r"tracker\.conf_predictor"),
])
def test_fused_tracker_refuses_by_attribute_name(mutate, match):
    _refused(mutate, match)


def test_channel_last_pitch_ignores_strides_of_size_one_dimensions():
    """B = 1 (or S = 1) leaves that dimension's stride arbitrary: a valid map must not be refused for it; a wrong stride elsewhere is."""
    import gd_amd  # noqa: F401
    from gd_amd._lib import GdHipError
    from gd_amd.teacher_tracker import FusedTracker
    buf = torch.zeros(1, 2, 5, 7, 128)
    assert FusedTracker.pitch_of(buf) == 7 and FusedTracker.pitch_of(buf[:, :, :, :6]) == 7 and FusedTracker.pitch_of(buf[:, :, :, :6], 7) == 7
    odd = torch.as_strided(buf, (1, 2, 5, 6, 128), (12345,) + buf.stride()[1:])
    assert FusedTracker.pitch_of(odd) == 7
    one_frame = torch.as_strided(buf, (1, 1, 5, 6, 128), (3, 11) + buf.stride()[2:])
    assert FusedTracker.pitch_of(one_frame) == 7
    with pytest.raises(GdHipError, match="strides"):
        FusedTracker.pitch_of(buf[:, :, :, :6], 6)
    with pytest.raises(GdHipError, match="strides"):
        FusedTracker.pitch_of(buf[:, :, ::2, :6])
    with pytest.raises(GdHipError, match="strides"):
        FusedTracker.pitch_of(buf.permute(1, 0, 2, 3, 4)[:, :, :, :6].expand(2, 2, 5, 6, 128))


def test_fused_tracker_accepts_the_layout_and_pads_k():
    import gd_amd  # noqa: F401
    from gd_amd.teacher_tracker import FusedTracker
    ft = FusedTracker(TL.make_tracker("b"))
    assert ft.levels == 7 and ft.radius == 4 and ft.kpad == 576 and ft.corr_mlp[0].shape == (TL.HIDDEN, 576)
    assert float(ft.corr_mlp[0][:, 567:].abs().max()) == 0.0 and ft.predictors[0].shape == (8, 128)
    no_conf = TL.make_tracker("a", predict_conf=False)
    assert FusedTracker(no_conf).predict_conf is False


def test_level_with_a_side_of_one_is_refused_with_level_and_size():
    import gd_amd  # noqa: F401
    from gd_amd._lib import GdHipError
    from gd_amd.teacher_tracker import check_levels, level_sizes
    assert level_sizes(131, 139, 7)[-1] == (2, 2)
    check_levels(131, 139, 7)
    check_levels(128, 128, 7)
    for H, W in ((69, 83), (64, 64), (127, 300)):
        with pytest.raises(GdHipError, match=r"level 6 of a \d+ x \d+ map is 1 x \d"):
            check_levels(H, W, 7)


def test_new_keywords_default_to_off_and_come_last():
    import gd_amd  # noqa: F401
    from gd_amd.teacher_heads import FusedDPTHead
    from gd_amd.teacher_runner import VGGTTeacherRunner
    from gd_amd.teacher_tracker import FusedTracker
    p = list(inspect.signature(VGGTTeacherRunner.__init__).parameters.values())
    assert p[-1].name == "fused_tracker" and p[-1].default is False
    p = list(inspect.signature(FusedDPTHead.forward).parameters.values())
    assert p[-1].name == "channel_last" and p[-1].default is False
    p = inspect.signature(FusedTracker.forward).parameters
    assert list(p)[1:] == ["query_points", "fmaps", "iters", "return_feat", "down_ratio", "apply_sigmoid", "fmaps_cl", "pitch"]
    assert p["fmaps_cl"].kind is inspect.Parameter.KEYWORD_ONLY and p["iters"].default == 6
    vggt = TL.make_tiny_vggt()
    assert VGGTTeacherRunner(vggt).tracker is None
    assert VGGTTeacherRunner(vggt, fused_tracker=True).tracker.levels == 3


def test_a_refused_tracker_raises_in_the_runner_constructor():
    import gd_amd  # noqa: F401
    from gd_amd._lib import GdHipError
    from gd_amd.teacher_runner import VGGTTeacherRunner
    vggt = TL.make_tiny_vggt()
    vggt.track_head.tracker.corr_radius = 6
    VGGTTeacherRunner(vggt)
    with pytest.raises(GdHipError, match=r"track_head\.tracker\.corr_radius"):
        VGGTTeacherRunner(vggt, fused_tracker=True)


# ---------------------------------------------------------------------------------------------------------------------------------- entry points
def test_entry_points_check_their_arguments_before_any_device_call():
    import gd_amd  # noqa: F401
    from gd_amd import _lib
    L = _lib.lib()
    f = ctypes.c_float
    err = lambda: L.gd_last_error().decode()
    maps, dims = (ctypes.c_void_p * 8)(), (ctypes.c_int * 24)(*([64, 64, 64] * 8))
    assert L.gd_corr_sample(maps, dims, 1, 4, None, None, 1, 2, 4, 64, None, 81, None) != 0 and "C = 64" in err()
    assert L.gd_corr_sample(maps, dims, 9, 4, None, None, 1, 2, 4, 128, None, 729, None) != 0 and "9 levels" in err()
    assert L.gd_corr_sample(maps, dims, 1, 5, None, None, 1, 2, 4, 128, None, 121, None) != 0 and "radius 5" in err()
    buf = ctypes.create_string_buffer(64)
    a = (ctypes.addressof(buf) + 15) & ~15
    assert L.gd_corr_sample(maps, dims, 2, 4, a, a, 1, 2, 4, 128, a, 100, None) != 0 and "ld 100" in err()
    one = (ctypes.c_int * 6)(8, 8, 8, 4, 1, 1)
    two = (ctypes.c_void_p * 2)(a, a)
    assert L.gd_corr_sample(two, one, 2, 4, a, a, 1, 2, 4, 128, a, 162, None) != 0 and "level 1 is 4 x 1" in err()
    assert L.gd_avgpool2_cl(None, None, 1, 8, 8, 8, 4, 32, None) != 0 and "C = 32" in err()
    assert L.gd_avgpool2_cl(a, a, 1, 8, 8, 7, 4, 128, None) != 0 and "pitch_in 7" in err()
    assert L.gd_avgpool2_cl(a, a, 1, 1, 8, 8, 4, 128, None) != 0 and "2 x 2" in err()
    assert L.gd_points_bilinear(None, None, None, 1, 4, 8, 8, 8, 96, 1, None) != 0 and "C = 96" in err()
    assert L.gd_points_bilinear(a, a, a, 1, 4, 8, 8, 7, 128, 1, None) != 0 and "pitch" in err()
    assert L.gd_track_pos_embed(a, a, a, 4, 8, 8, 390, None) != 0 and "multiple of 4" in err()
    assert L.gd_track_pos_embed(None, a, a, 4, 8, 8, 388, None) != 0 and "required" in err()
    assert L.gd_track_assemble(a, a, a, a, a, a, 1, 2, 4, 64, f(518.0), None) != 0 and "C = 64" in err()
    assert L.gd_track_assemble(a, a, a, a, a, a, 1, 0, 4, 128, f(518.0), None) != 0 and "S=0" in err()
    assert L.gd_track_update(a, 100, a, a, a, 1, 2, 4, 128, f(1.0), f(1.0), None) != 0 and "ldd 100" in err()
    assert L.gd_track_update(a, 130, a, a, a + 4, 1, 2, 4, 128, f(1.0), f(1.0), None) != 0 and "aligned" in err()


def test_tensor_wrappers_refuse_host_tensors_and_bad_shapes():
    import gd_amd  # noqa: F401
    from gd_amd import ops
    from gd_amd._lib import GdHipError
    m = torch.zeros(2, 8, 8, 128)
    with pytest.raises(GdHipError, match="avgpool2_cl: src"):
        ops.avgpool2_cl(m)
    with pytest.raises(GdHipError, match="corr_sample: targets"):
        ops.corr_sample([(m, 8, 8, 8)], torch.zeros(1, 4, 2, 128), torch.zeros(1, 4, 2, 2), 4)
    with pytest.raises(GdHipError, match="points_bilinear: fmap"):
        ops.points_bilinear(m, 8, torch.zeros(2, 4, 2))
    with pytest.raises(GdHipError, match="track_pos_embed: points"):
        ops.track_pos_embed(torch.zeros(4, 2), 8, 8, 388)
    with pytest.raises(GdHipError, match="track_assemble: coords"):
        ops.track_assemble(torch.zeros(1, 4, 2, 2), torch.zeros(1, 2, 4, 128), torch.zeros(1, 4, 2, 128), torch.zeros(4, 388), torch.zeros(2, 388), 518)
    with pytest.raises(GdHipError, match="track_update: coords"):
        ops.track_update(torch.zeros(1, 4, 2, 130), torch.zeros(1, 4, 2, 2))
