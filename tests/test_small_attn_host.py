"""Host: the fp64 restatement of gd_attention_small_fwd (tests/small_attn_ref64.py) against torch.nn.MultiheadAttention and against a
permuted-and-contiguous evaluation; FusedUpdateFormer's refusals, at construction, with no device; the entry point's argument errors, which fail
before any device call."""
import ctypes

import pytest
import torch

import small_attn_ref64 as A64
import tracker_layout as TL


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("Lq,Lk,hd,H,cross", [(2, 2, 48, 8, False), (17, 65, 12, 3, True), (5, 9, 4, 1, True), (7, 7, 64, 2, False)])
def test_restatement_is_multihead_attention_between_its_projections(Lq, Lk, hd, H, cross):
    """nn.MultiheadAttention in fp64 with identity input / output projections and no biases IS softmax(q k^T / sqrt(hd)) v per head."""
    D, Bt = H * hd, 3
    mha = torch.nn.MultiheadAttention(D, H, batch_first=True, bias=False).double()
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(D, dtype=torch.float64).repeat(3, 1))
        mha.out_proj.weight.copy_(torch.eye(D, dtype=torch.float64))
    q = torch.randn(Bt, Lq, D, generator=gen(Lq), dtype=torch.float64)
    k = torch.randn(Bt, Lk, D, generator=gen(Lk + 100), dtype=torch.float64) if cross else q
    v = torch.randn(Bt, Lk, D, generator=gen(Lk + 200), dtype=torch.float64) if cross else q
    with torch.no_grad():
        want = mha(q, k, v, need_weights=False)[0]
    got, bound = A64.attention64(q[:, None], k[:, None], v[:, None], H)
    rel = float((got[:, 0] - want).abs().max() / want.abs().max())
    print(f"restatement against nn.MultiheadAttention (fp64) Lq={Lq} Lk={Lk} hd={hd} H={H}: {rel:.2e} relative")
    assert rel <= 1e-13 and bool((bound > 0).all())


def test_restatement_with_the_modules_own_projections():
    """A whole _SelfBlock / _CrossBlock attention: in_proj, the restatement, out_proj, against the module in fp64."""
    D, H = 96, 8
    mha = torch.nn.MultiheadAttention(D, H, batch_first=True).double()
    x, c = torch.randn(2, 5, D, generator=gen(1), dtype=torch.float64), torch.randn(2, 9, D, generator=gen(2), dtype=torch.float64)
    w, b = mha.in_proj_weight, mha.in_proj_bias
    with torch.no_grad():
        for ctx in (x, c):
            want = mha(x, ctx, ctx, need_weights=False)[0]
            q, k, v = x @ w[:D].T + b[:D], ctx @ w[D:2 * D].T + b[D:2 * D], ctx @ w[2 * D:].T + b[2 * D:]
            o = A64.attention64(q[:, None], k[:, None], v[:, None], H)[0][:, 0]
            got = o @ mha.out_proj.weight.T + mha.out_proj.bias
            assert float((got - want).abs().max() / want.abs().max()) <= 1e-13


def space_layout(B, S, N, nv, D, ld):
    """(offsets, strides) of the update transformer's space stage in a [B, N + nv, S, ld] buffer: point rows from 0, virtual rows from N * S * ld."""
    return dict(points=0, virtual=N * S * ld, s0=(N + nv) * S * ld, s1=ld, ldrow=S * ld)


def test_strided_addressing_is_the_permuted_contiguous_evaluation():
    B, S, N, nv, H, hd = 2, 3, 5, 4, 8, 12
    D = H * hd
    ld = D + 8
    L = space_layout(B, S, N, nv, D, ld)
    buf = torch.randn(B, N + nv, S, ld, generator=gen(5), dtype=torch.float64)
    flat = buf.reshape(-1)
    # q = the virtual rows, k = v = the point rows, per frame (b, s): what virtual2point addresses
    got, _ = A64.attention_strided64(flat, flat, flat, (L["virtual"], L["points"], L["points"]), B, S, nv, N, H, hd, (L["ldrow"],) * 3, ((L["s0"], L["s1"]),) * 3)
    sp = buf[..., :D].permute(0, 2, 1, 3).contiguous()                       # [B, S, N + nv, D]: the reference's permute().contiguous()
    want, _ = A64.attention64(sp[:, :, N:], sp[:, :, :N], sp[:, :, :N], H)
    assert torch.equal(got, want)
    # the time stage: q | k | v column blocks of one packed [rows, 3 D] tensor, sequences of S consecutive rows
    rows = B * (N + nv)
    packed = torch.randn(rows * S, 3 * D, generator=gen(6), dtype=torch.float64)
    got, _ = A64.attention_strided64(*(packed.reshape(-1),) * 3, (0, D, 2 * D), rows, 1, S, S, H, hd, (3 * D,) * 3, ((S * 3 * D, 0),) * 3)
    p4 = packed.view(rows, 1, S, 3 * D)
    want, _ = A64.attention64(p4[..., :D].contiguous(), p4[..., D:2 * D].contiguous(), p4[..., 2 * D:].contiguous(), H)
    assert torch.equal(got, want)
    # and the cells an output of that layout covers are distinct and inside the buffer
    c = A64.cells(L["virtual"], B, S, nv, D, L["s0"], L["s1"], L["ldrow"])
    assert c.unique().numel() == c.numel() == B * S * nv * D and int(c.max()) < flat.numel()


# ---------------------------------------------------------------------------------------------------------------------------------- refusals
def former(space_depth=2, time_depth=2, hidden=TL.HIDDEN, heads=8):
    torch.manual_seed(0)
    return TL.UpdateFormerLayout(space_depth, time_depth, 3 * TL.LATENT + 4, hidden, TL.LATENT + 2, num_heads=heads).eval()


def _refused(mutate, match, **kw):
    import gd_amd  # noqa: F401
    from gd_amd._lib import GdHipError
    from gd_amd.teacher_tracker import FusedUpdateFormer
    m = former(**kw)
    FusedUpdateFormer(m)                                                      # accepted as it stands
    mutate(m)
    with pytest.raises(GdHipError, match=match):
        FusedUpdateFormer(m)


class _NotMHA(torch.nn.Module):
    def forward(self, q, k, v):
        return q, None


def _mha(**kw):
    return torch.nn.MultiheadAttention(TL.HIDDEN, 8, **dict(dict(batch_first=True), **kw))


@pytest.mark.parametrize("mutate,match", [
    (lambda m: setattr(m.time_blocks[1], "attn", _NotMHA()), r"updateformer\.time_blocks\[1\]\.attn: _NotMHA"),
    (lambda m: setattr(m.space_virtual_blocks[0], "attn", _mha(batch_first=False)), r"space_virtual_blocks\[0\]\.attn\.batch_first"),
    (lambda m: setattr(m.space_point2virtual_blocks[1], "cross_attn", _mha(kdim=64, vdim=64)), r"space_point2virtual_blocks\[1\]\.cross_attn\._qkv_same_embed_dim"),
    (lambda m: setattr(m.time_blocks[0], "attn", _mha(dropout=0.1)), r"time_blocks\[0\]\.attn\.dropout"),
    (lambda m: setattr(m.space_virtual2point_blocks[0], "cross_attn", _mha(add_bias_kv=True)), r"space_virtual2point_blocks\[0\]\.cross_attn\.bias_k"),
    (lambda m: setattr(m.time_blocks[0], "attn", _mha(add_zero_attn=True)), r"time_blocks\[0\]\.attn\.add_zero_attn"),
])
def test_refuses_an_attention_module_the_kernel_does_not_serve(mutate, match):
    _refused(mutate, match)


def test_refuses_heads_that_do_not_divide_the_width_or_leave_the_contract():
    _refused(lambda m: setattr(m.time_blocks[0].attn, "num_heads", 7), r"time_blocks\[0\]\.attn\.num_heads: 7 does not divide embed_dim 96")
    # 96 / 16 = 6: not a multiple of 4; 96 / 1 = 96: above 64; 96 / 48 = 2: below 4
    for heads, hd in ((16, 6), (1, 96), (48, 2)):
        _refused(lambda m: setattr(m.space_virtual_blocks[1], "attn", torch.nn.MultiheadAttention(TL.HIDDEN, heads, batch_first=True)),
                 rf"space_virtual_blocks\[1\]\.attn\.num_heads: {heads}: head dimension {hd}")


def test_refuses_an_activation_that_is_not_exact_gelu():
    _refused(lambda m: setattr(m.time_blocks[1].mlp, "act", torch.nn.GELU(approximate="tanh")), r"time_blocks\[1\]\.mlp\.act")
    _refused(lambda m: setattr(m.space_point2virtual_blocks[0].mlp, "act", torch.nn.ReLU()), r"space_point2virtual_blocks\[0\]\.mlp\.act")


def test_refuses_a_layernorm_that_is_not_affine():
    plain = lambda: torch.nn.LayerNorm(TL.HIDDEN, elementwise_affine=False)
    _refused(lambda m: setattr(m.time_blocks[0], "norm1", plain()), r"time_blocks\[0\]\.norm1")
    _refused(lambda m: setattr(m.space_virtual2point_blocks[1], "norm_context", plain()), r"space_virtual2point_blocks\[1\]\.norm_context")
    _refused(lambda m: setattr(m.space_virtual_blocks[0], "norm2", plain()), r"space_virtual_blocks\[0\]\.norm2")
    _refused(lambda m: setattr(m, "output_norm", plain()), r"updateformer\.output_norm")
    _refused(lambda m: setattr(m, "input_norm", torch.nn.LayerNorm(3 * TL.LATENT + 4, elementwise_affine=False)), r"updateformer\.input_norm")


def test_refuses_depths_whose_loop_would_index_past_the_space_blocks():
    """blocks.py:122: a stage after time block i when i % (time // space) == 0.  6 / 4 -> every block: 6 stages for 4 space blocks; 5 / 2 -> i = 0, 2, 4:
    3 stages for 2.  4 / 2 (stages at 0 and 2) and 6 / 6 are served."""
    import gd_amd  # noqa: F401
    from gd_amd._lib import GdHipError
    from gd_amd.teacher_tracker import FusedUpdateFormer
    for t, s, last in ((6, 4, 5), (5, 2, 2)):
        with pytest.raises(GdHipError, match=rf"space_virtual_blocks: time depth {t} / space depth {s}.*space block {last} of {s}"):
            FusedUpdateFormer(former(space_depth=s, time_depth=t))
    assert FusedUpdateFormer(former(space_depth=2, time_depth=4)).every == 2
    f = FusedUpdateFormer(former(space_depth=3, time_depth=3))
    assert f.every == 1 and f.nv == 64 and f.D == TL.HIDDEN and f.ldo == 132 and f.flow_head[0].shape == (132, TL.HIDDEN)
    assert float(f.flow_head[0][130:].abs().max()) == 0.0
    assert FusedUpdateFormer(former(space_depth=0, time_depth=2)).nv == 0


def test_a_mask_is_refused_and_the_switches_default_to_off():
    import inspect
    import gd_amd  # noqa: F401
    from gd_amd._lib import GdHipError
    from gd_amd.teacher_runner import VGGTTeacherRunner
    from gd_amd.teacher_tracker import FusedTracker, FusedUpdateFormer
    with pytest.raises(GdHipError, match="mask"):
        FusedUpdateFormer(former())(torch.zeros(1, 2, 2, 388), mask=torch.ones(1))
    assert inspect.signature(FusedTracker.__init__).parameters["fused_updateformer"].default is False
    assert inspect.signature(VGGTTeacherRunner.__init__).parameters["fused_updateformer"].default is False
    trk = TL.make_tracker("a")
    assert FusedTracker(trk).updateformer is trk.updateformer
    assert isinstance(FusedTracker(trk, fused_updateformer=True).updateformer, FusedUpdateFormer)
    vggt = TL.make_tiny_vggt()
    with pytest.raises(GdHipError, match="fused_updateformer=True needs fused_tracker=True"):
        VGGTTeacherRunner(vggt, fused_updateformer=True)
    r = VGGTTeacherRunner(vggt, fused_tracker=True, fused_updateformer=True)
    assert isinstance(r.tracker.updateformer, FusedUpdateFormer)
    assert VGGTTeacherRunner(vggt, fused_tracker=True).tracker.updateformer is vggt.track_head.tracker.updateformer
    vggt.track_head.tracker.updateformer.time_blocks[0].mlp.act = torch.nn.ReLU()
    VGGTTeacherRunner(vggt, fused_tracker=True)
    with pytest.raises(GdHipError, match=r"track_head\.tracker\.updateformer\.time_blocks\[0\]\.mlp\.act"):
        VGGTTeacherRunner(vggt, fused_tracker=True, fused_updateformer=True)


# ---------------------------------------------------------------------------------------------------------------------------------- entry point
def test_entry_point_checks_its_arguments_before_any_device_call():
    import gd_amd  # noqa: F401
    from gd_amd import _lib
    L = _lib.lib()
    err = lambda: L.gd_last_error().decode()
    buf = ctypes.create_string_buffer(1 << 16)
    a = (ctypes.addressof(buf) + 15) & ~15
    q, k, v, o = a, a + 4096, a + 8192, a + 12288                             # 1024 floats apart: never dereferenced

    def call(q=q, k=k, v=v, o=o, G0=1, G1=1, Nq=2, Nk=2, H=2, hd=8, ld=(16, 16, 16, 16), st=(32, 32) * 4):
        return L.gd_attention_small_fwd(q, k, v, o, G0, G1, Nq, Nk, H, hd, *ld, *st, ctypes.c_float(0.5), None)
    for hd in (5, 0, 68):
        assert call(hd=hd) != 0 and f"head_dim {hd}" in err()
    assert call(Nk=0) != 0 and "Nk=0" in err()
    assert call(ld=(16, 18, 16, 16)) != 0 and "ldk = 18" in err() and "multiple of 4" in err()
    assert call(st=(32, 32, 32, 32, 32, 30, 32, 32)) != 0 and "sv1 = 30" in err()
    assert call(ld=(16, 16, 16, 12)) != 0 and "below H * head_dim = 16" in err()
    assert call(k=k + 4) != 0 and "16-byte aligned" in err()
    assert call(q=None) != 0 and "required" in err()
    assert call(o=q) != 0 and "o overlaps q" in err()
    assert call(o=v + 64) != 0 and "o overlaps v" in err()                   # two rows in: the ranges intersect
    assert call(G0=3, G1=2, o=k - 4 * 32) != 0 and "o overlaps k" in err()   # o's last cells reach into k


def test_wrapper_refuses_host_tensors_and_bad_views():
    import gd_amd  # noqa: F401
    from gd_amd import ops
    from gd_amd._lib import GdHipError
    t = torch.zeros(1, 1, 2, 16)
    with pytest.raises(GdHipError, match="attention_small_fwd: q"):
        ops.attention_small_fwd(t, t, t, 1, 1, 2, 2, 2)
