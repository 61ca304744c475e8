"""GPU: the MASt3R teacher's blocks on the HIP kernels — gd_cross_attention_fwd against fp64, teacher_blocks.FusedCroCoBlocks against the module
tree of tests/croco_layout.py (fp64) and against fixture G25 (what the reference's own blocks returned), and MASt3RTeacherRunner with
fused_blocks against its own default path.

Every test prints its measured error beside the bound before it asserts; tools/bench_teacher.py records the parity values."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

import croco_layout as CL
from conftest import load_golden, rel_err
from test_teacher_runner_ref import fill_params

pytestmark = pytest.mark.gpu

TGT_TOL = 2e-6            # tests/test_gpu_teacher_glue.py: gd_mast3r_attn_target in f32 against fixture G17
# (o, lse) bounds of tests/test_gpu_attention.py for the same arithmetic; f32x3: o as a relative Frobenius norm
KERNEL_TOL = {"f32": (1e-5, 1e-5), "bf16": (2e-2, 1e-2), "f16": (3e-3, 1e-2), "f32x3": (3e-5, 1e-5)}
TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f32x3": torch.float32}
SHAPES = [(1, 1, 1, 1), (1, 17, 70, 1), (2, 130, 64, 2), (1, 64, 17, 3), (2, 200, 257, 2), (2, 768, 768, 12)]


def max_abs(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def make_layout(norm_mem_off=None, **over):
    """The MASt3R-shaped module tree with deterministic weights.  norm_mem_off: index of a `dec_blocks` entry built with norm_mem=False."""
    m = CL.CrocoLayout(**dict(CL.CFG, **over)).eval()
    if norm_mem_off is not None:
        m.dec_blocks[norm_mem_off] = CL.CrocoDecoderBlock(CL.CFG["dec_dim"], CL.CFG["dec_heads"], m.rope, norm_mem=False).eval()
    fill_params(m)
    return m


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against fp64
# ----------------------------------------------------------------------------------------------------------------------------------
def _ref64(q, kv, B, Nq, Nk, H):
    """fp64 on the device: o [B*Nq, H*64], lse [B, H, Nq] of the (already rounded) operands."""
    qd = q.double().reshape(B, Nq, H, 64).transpose(1, 2)
    k, v = kv.double().reshape(B, Nk, 2, H, 64).permute(2, 0, 3, 1, 4).unbind(0)
    s = qd @ k.transpose(-1, -2) * 64 ** -0.5
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * Nq, H * 64), torch.logsumexp(s, -1)


@functools.lru_cache(maxsize=None)
def _case(shape, dt):
    """(q, kv, o64, lse64) for one shape and element type, computed once and shared by the layout variants."""
    B, Nq, Nk, H = shape
    g = torch.Generator().manual_seed(1000 * Nq + Nk)            # (a host generator: the inputs do not depend on the device's RNG)
    q = torch.randn(B * Nq, H * 64, generator=g)
    kv = torch.randn(B * Nk, 2 * H * 64, generator=g)
    if Nk == 1:
        # One key: lse IS the one score, a 64-term dot product.  With independent signs its terms cancel (sum |q_i k_i| / 8 ~ 5 against a result of
        # ~0.5), and a RELATIVE bound on that one number would measure the conditioning of the sum, not the kernel: the split-precision products
        # carry ~2^-17 of each TERM whatever the sum comes to.  The key's signs follow the query's, so the score is the sum of its terms' sizes.
        kv[:, :H * 64] = kv[:, :H * 64].abs() * torch.sign(q[:1].expand(B * Nk, -1))
    q, kv = q.to(TORCH_DTYPE[dt]).cuda(), kv.to(TORCH_DTYPE[dt]).cuda()
    return (q, kv) + _ref64(q, kv, B, Nq, Nk, H)


def _check_kernel(o, lse, o64, lse64, dt, what):
    otol, ltol = KERNEL_TOL[dt]
    eo = float((o.double() - o64).norm() / o64.norm()) if dt == "f32x3" else rel_err(o, o64)
    el = rel_err(lse, lse64)
    print(f"cross_attention {what} {dt}: o {eo:.3e} (bound {otol:g}), lse {el:.3e} (bound {ltol:g})")
    assert bool(torch.isfinite(o.float()).all()) and eo < otol and el < ltol


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16", "f32x3"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cross_attention_against_fp64(shape, dt):
    from gd_amd import ops
    B, Nq, Nk, H = shape
    q, kv, o64, lse64 = _case(shape, dt)
    x3 = dt == "f32x3"
    o, lse = ops.cross_attention_fwd(q, kv, B, Nq, Nk, H, want_lse=True, x3=x3)
    assert o.shape == (B * Nq, H * 64) and lse.shape == (B, H, Nq)
    _check_kernel(o, lse, o64, lse64, dt, f"{shape} contiguous")
    o2, none = ops.cross_attention_fwd(q, kv, B, Nq, Nk, H, x3=x3)              # lse = NULL
    assert none is None and torch.equal(o2, o)
    # padded row strides, the pad columns NaN: nothing outside the operands is read
    qp = torch.full((B * Nq, H * 64 + 64), float("nan"), dtype=q.dtype, device="cuda")
    kvp = torch.full((B * Nk, 2 * H * 64 + 128), float("nan"), dtype=q.dtype, device="cuda")
    qp[:, :H * 64], kvp[:, :2 * H * 64] = q, kv
    o3, lse3 = ops.cross_attention_fwd(qp[:, :H * 64], kvp[:, :2 * H * 64], B, Nq, Nk, H, want_lse=True, x3=x3)
    _check_kernel(o3, lse3, o64, lse64, dt, f"{shape} padded strides")
    assert torch.equal(o3, o) and torch.equal(lse3, lse)


@pytest.mark.parametrize("N", [17, 257])
def test_cross_attention_on_a_packed_qkv_buffer_equals_self_attention(N):
    """q and kv as the two column slices of one packed [B*N, 3*H*64] buffer (ldq = ldkv = 3*H*64): self-attention."""
    from gd_amd import ops
    B, H = 2, 2
    qkv = torch.randn(B * N, 3 * H * 64, generator=torch.Generator(device="cuda").manual_seed(N), device="cuda")
    want, want_lse = ops.attention_fwd(qkv, B, N, H)
    o, lse = ops.cross_attention_fwd(qkv[:, :H * 64], qkv[:, H * 64:], B, N, N, H, want_lse=True)
    eo, el = rel_err(o, want), rel_err(lse, want_lse)
    print(f"packed qkv N={N}: o {eo:.3e}, lse {el:.3e} (bound 1e-5 each); bit-identical to attention_fwd: o {torch.equal(o, want)}, "
          f"lse {torch.equal(lse, want_lse)}")
    assert eo < 1e-5 and el < 1e-5


@pytest.mark.parametrize("dt,tol,lse_tol", [("f16", 4 * 3e-3, 2e-2), ("bf16", 2e-2, 0.15)])
def test_cross_attention_reference_point_moves(dt, tol, lse_tol):
    """"rising": the keys of the third 64-key tile score ~29 log2 units (> ATT_THR = 8) above everything before them, so the lagged reference
    point is raised there and o / l are rescaled; Nk = 200 ends in a partial tile.  Tolerances: the "rising" case of
    tests/test_gpu_attention.py::test_attention_reference_point_moves (the score offset comes from ONE coordinate shared by every query,
    so its 16-bit rounding is coherent: see there)."""
    from gd_amd import ops
    B, Nq, Nk, H = 2, 70, 200, 2
    g = torch.Generator(device="cuda").manual_seed(7)
    q = torch.randn(B, Nq, H, 64, generator=g, device="cuda")
    kv = torch.randn(B, Nk, 2, H, 64, generator=g, device="cuda")
    q[..., 0] = 8.0
    kv[:, :, 0, :, 0] = 0.0
    kv[:, 128:192, 0, :, 0] = 20.0                          # + 8 * 20 / 8 = 20 on the score (28.9 in log2 units)
    q, kv = q.reshape(B * Nq, H * 64).to(TORCH_DTYPE[dt]), kv.reshape(B * Nk, 2 * H * 64).to(TORCH_DTYPE[dt])
    o, lse = ops.cross_attention_fwd(q, kv, B, Nq, Nk, H, want_lse=True)
    o64, lse64 = _ref64(q, kv, B, Nq, Nk, H)
    eo, el = rel_err(o, o64), max_abs(lse, lse64)
    print(f"rising {dt}: o {eo:.3e} (bound {tol:g}), lse max abs {el:.3e} (bound {lse_tol:g})")
    assert bool(torch.isfinite(o.float()).all()) and eo < tol and el < lse_tol


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. one block of each kind, f32, against the layout in fp64
# ----------------------------------------------------------------------------------------------------------------------------------
def test_one_encoder_block_and_one_decoder_block_f32():
    from gd_amd.teacher_blocks import FusedCroCoBlocks
    m = make_layout(norm_mem_off=1)
    assert isinstance(m.dec_blocks[1].norm_y, nn.Identity)
    ref = copy.deepcopy(m).double()
    fused = FusedCroCoBlocks(m.cuda(), dtype=torch.float32)
    x1, pos1, x2, pos2 = CL.seeded_inputs(seed=5)
    g = torch.Generator().manual_seed(6)
    d1, d2 = torch.randn(CL.B, 21, 128, generator=g), torch.randn(CL.B, 20, 128, generator=g)
    with torch.no_grad():
        want_e = ref.enc_blocks[1](x2.double(), pos2)
        want = [blk(d1.double(), d2.double(), pos1, pos2) for blk in (ref.dec_blocks[0], ref.dec_blocks[1])]
        want_r, _, want_rs = ref.dec_blocks2[0](d2.double(), d1.double(), pos2, pos1)
    dev = lambda t, n: t.reshape(CL.B * n, -1).cuda()
    got_e = fused._enc_block(fused.enc[1], dev(x2, 20), dev(pos2, 20), CL.B, 20)
    e, bound = max_abs(got_e, want_e.reshape(-1, 192)), 1e-4 * float(want_e.abs().max())
    print(f"encoder block: e {e:.3e}, bound {bound:.3e}")
    assert e <= bound
    for name, p, (wx, _, ws) in (("decoder block", fused.dec1[0], want[0]), ("decoder block, norm_mem=False", fused.dec1[1], want[1])):
        got, camap = fused._dec_block(p, dev(d1, 21), dev(d2, 20), dev(pos1, 21), dev(pos2, 20), CL.B, 21, 20)
        e, bound = max_abs(got, wx.reshape(-1, 128)), 1e-4 * float(wx.abs().max())
        wm = ws.mean(dim=1, keepdim=True)
        em, mbound = max_abs(camap, wm), 1e-4 * float(wm.abs().max())
        print(f"{name}: e {e:.3e}, bound {bound:.3e}; head-mean scores e {em:.3e}, bound {mbound:.3e}")
        assert camap.shape == (CL.B, 1, 21, 20) and e <= bound and em <= mbound
    got, camap = fused._dec_block(fused.dec2[0], dev(d2, 20), dev(d1, 21), dev(pos2, 20), dev(pos1, 21), CL.B, 20, 21)      # Nq < Nk
    e, bound = max_abs(got, want_r.reshape(-1, 128)), 1e-4 * float(want_r.abs().max())
    print(f"decoder block of the other side: e {e:.3e}, bound {bound:.3e}")
    assert camap.shape == (CL.B, 1, 20, 21) and e <= bound and max_abs(camap, want_rs.mean(dim=1, keepdim=True)) <= 1e-4 * float(want_rs.abs().max())


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. the whole stack
# ----------------------------------------------------------------------------------------------------------------------------------
def fused_stack(m, dtype, x1, pos1, x2, pos2):
    """The layout's path with its blocks on the kernels: encode -> the module's own enc_norm -> decode -> teacher_glue's target.
    -> (encoder-block outputs, decoder outputs, camaps1, camaps2, tgt_attn_map)"""
    from gd_amd import teacher_glue as tg
    from gd_amd.teacher_blocks import FusedCroCoBlocks
    fused = FusedCroCoBlocks(m, dtype=dtype)
    enc = [fused.encode(x1.cuda(), pos1.cuda()), fused.encode(x2.cuda(), pos2.cuda())]
    with torch.no_grad():
        f1, f2 = m.enc_norm(enc[0]), m.enc_norm(enc[1])
    outs, c1, c2 = fused.decode(f1, pos1.cuda(), f2, pos2.cuda())
    return enc, outs, c1, c2, tg.mast3r_tgt_attn_map(c1, c2, m.temperature)


def layout_stack(m, x1, pos1, x2, pos2):
    """The same through the modules: (encoder-block outputs, decoder outputs, tgt_attn_map)"""
    with torch.no_grad():
        enc = [m.encode_blocks(x1, pos1), m.encode_blocks(x2, pos2)]
        outs, tgt = m.target(m.enc_norm(enc[0]), pos1, m.enc_norm(enc[1]), pos2)
    return enc, outs, tgt


def stack_tokens(enc, outs):
    return list(enc) + [t for v in outs for t in v]


@functools.lru_cache(maxsize=None)
def layout_fp64():
    """The layout's fp64 run on the fixture's inputs, once: (inputs, tokens, tgt_attn_map, e32 = max abs error of its float32 run's target)."""
    m = make_layout()
    inp = CL.seeded_inputs()
    x1, pos1, x2, pos2 = inp
    enc, outs, tgt = layout_stack(copy.deepcopy(m).double(), x1.double(), pos1, x2.double(), pos2)
    _, _, tgt32 = layout_stack(m, *inp)
    return inp, stack_tokens(enc, outs), tgt, max_abs(tgt32, tgt)


def f32_parity():
    """-> dict of the measured f32 values of the whole stack against fixture G25 (also recorded by tools/bench_teacher.py)."""
    g = load_golden("g25_mast3r_blocks")
    inp, _, _, e32 = layout_fp64()
    assert all(torch.equal(a, g[k]) for a, k in zip(inp, ("x1", "pos1", "x2", "pos2")))
    enc, outs, c1, c2, tgt = fused_stack(make_layout().cuda(), torch.float32, *inp)
    return g, enc, outs, c1, c2, tgt, e32


def test_whole_stack_f32_against_reference_fixture():
    g, enc, outs, c1, c2, tgt, e32 = f32_parity()
    assert len(outs) == 2 and len(outs[0]) == len(outs[1]) == 3 and len(c1) == len(c2) == 2
    named = [("enc_1", enc[0]), ("enc_2", enc[1])] + [(f"out{v + 1}_{i}", t) for v in range(2) for i, t in enumerate(outs[v])]
    named += [(f"camap1_{l}", t) for l, t in enumerate(c1)] + [(f"camap2_{l}", t) for l, t in enumerate(c2)]
    for name, t in named:
        want = g[name]
        e, bound = max_abs(t, want), 1e-4 * float(want.abs().max())
        print(f"{name}: e {e:.3e}, bound {bound:.3e}")
        assert t.dtype == torch.float32 and tuple(t.shape) == tuple(want.shape) and e <= bound, name
    assert c1[0].shape == (2, 1, 21, 20) and c2[0].shape == (2, 1, 20, 21)
    e, bound = max_abs(tgt, g["tgt_attn_map"]), max(TGT_TOL, 4 * e32)
    print(f"tgt_attn_map: e {e:.3e}, bound max(2e-6, 4 * e32) = {bound:.3e} (e32 {e32:.3e})")
    assert tgt.shape == (2, 21, 20) and e <= bound


def bf16_parity_pair():
    """-> {"tokens": (e_ref, e_hip), "tgt_attn_map": (e_ref, e_hip)}: max abs error against the layout's fp64 run of (e_ref) the same modules on
    the GPU under torch.autocast(bfloat16) and (e_hip) the fused bf16 path."""
    inp, tok64, tgt64, _ = layout_fp64()
    m = make_layout().cuda()
    cu = [t.cuda() for t in inp]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        enc_r, outs_r, tgt_r = layout_stack(m, *cu)
    enc_h, outs_h, _, _, tgt_h = fused_stack(m, torch.bfloat16, *inp)
    worst = lambda toks: max(max_abs(a, b) for a, b in zip(toks, tok64))
    return {"tokens": (worst(stack_tokens(enc_r, outs_r)), worst(stack_tokens(enc_h, outs_h))),
            "tgt_attn_map": (max_abs(tgt_r, tgt64), max_abs(tgt_h, tgt64))}


def test_whole_stack_bf16_in_the_precision_class_of_autocast():
    pair = bf16_parity_pair()
    for what, (e_ref, e_hip) in pair.items():
        print(f"bf16 {what}: e_ref (torch autocast) {e_ref:.4e}, e_hip (fused) {e_hip:.4e}")
    for what, (e_ref, e_hip) in pair.items():
        assert e_hip <= 2 * e_ref, what


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. the runner
# ----------------------------------------------------------------------------------------------------------------------------------
PATCH, IMG_H, IMG_W = 16, 48, 80         # 3 x 5 = 15 tokens per view


class TinyMatcher(CL.CrocoLayout):
    """A matcher shaped like the teacher around the layout's blocks: a small patch embedding, `_encode_image`-style loops over `enc_blocks`,
    `_decoder`, and stub heads (desc / conf / pts3d per pixel: a fixed unit-norm code per pixel, so that reciprocal matching finds every pixel's
    twin, plus a small term read off the decoder tokens)."""

    def __init__(self):
        super().__init__(**CL.CFG)
        self.patch_embed = nn.Linear(3 * PATCH * PATCH, CL.CFG["enc_dim"])
        self.head = nn.Linear(CL.CFG["dec_dim"], 24 + 1 + 3)
        code = torch.randn(IMG_H, IMG_W, 24, generator=torch.Generator().manual_seed(3))
        self.register_buffer("code", code / code.norm(dim=-1, keepdim=True))
        self.fail_once = False

    def _encode_image(self, img):
        b = img.shape[0]
        gh, gw = IMG_H // PATCH, IMG_W // PATCH
        x = self.patch_embed(img.reshape(b, 3, gh, PATCH, gw, PATCH).permute(0, 2, 4, 1, 3, 5).reshape(b, gh * gw, -1))
        pos = CL.grid_positions(b, gh, gw).to(img.device)
        for blk in self.enc_blocks:
            x = blk(x, pos)
        return self.enc_norm(x), pos

    def _head(self, toks):
        if self.fail_once:
            self.fail_once = False
            raise RuntimeError("stub head failure")
        b, gh, gw = toks[-1].shape[0], IMG_H // PATCH, IMG_W // PATCH
        px = self.head(toks[-1].to(self.head.weight.dtype)).reshape(b, gh, gw, -1).repeat_interleave(PATCH, dim=1).repeat_interleave(PATCH, dim=2)
        return {"desc": self.code + 1e-3 * px[..., :24], "conf": 1.0 + px[..., 24].abs(), "pts3d": px[..., 25:]}

    def forward(self, view1, view2):
        (f1, pos1), (f2, pos2) = self._encode_image(view1["img"]), self._encode_image(view2["img"])
        dec, maps1, maps2 = self._decoder(f1, pos1, f2, pos2)
        res1, res2 = self._head(dec[0]), self._head(dec[1])
        res2["pts3d_in_other_view"] = res2.pop("pts3d")
        res2["tgt_attn_map"] = self.target_from_maps(maps1, maps2)
        return res1, res2


def _make_pairs(imgs, scene_graph="complete", prefilter=None, symmetrize=True):
    return [(imgs[0], imgs[1]), (imgs[1], imgs[0])]


def _inference(pairs, model, device, verbose=False):
    v1 = {"img": torch.cat([a for a, _ in pairs]).to(device)}
    v2 = {"img": torch.cat([b for _, b in pairs]).to(device)}
    p1, p2 = model(v1, v2)
    return {"view1": v1, "view2": v2, "pred1": p1, "pred2": p2}


def _shadows(m):
    return [n for n in ("_decoder",) if n in vars(m)] + [f"enc_blocks[{i}].forward" for i, b in enumerate(m.enc_blocks) if "forward" in vars(b)]


def test_runner_fused_blocks_against_the_plain_runner():
    from gd_amd.teacher_runner import MASt3RTeacherRunner
    m = TinyMatcher().eval()
    fill_params(m, seed=26)
    g = torch.Generator().manual_seed(8)
    im1, im2 = torch.rand(1, 3, IMG_H, IMG_W, generator=g), torch.rand(1, 3, IMG_H, IMG_W, generator=g)
    depth = torch.rand(IMG_H, IMG_W, generator=g) + 1.0
    # e32: the float32 error of this matcher's own target against its fp64 run (both on the host)
    with torch.no_grad():
        m.temperature = 3.0
        t32 = _inference(_make_pairs([im1, im2]), m, "cpu")["pred2"]["tgt_attn_map"]
        t64 = _inference(_make_pairs([im1.double(), im2.double()]), copy.deepcopy(m).double(), "cpu")["pred2"]["tgt_attn_map"]
    e32 = max_abs(t32, t64)
    m = m.cuda()
    kw = dict(inference=_inference, make_pairs=_make_pairs, keep_logits=True)
    args = dict(temperature=3.0, depth_1=depth.cuda(), depth_2=depth.cuda())
    plain = MASt3RTeacherRunner(m, **kw).targets(im1, im2, **args)
    assert _shadows(m) == []
    runner = MASt3RTeacherRunner(m, fused_blocks=True, **kw)
    fused = runner.targets(im1, im2, **args)
    assert _shadows(m) == []
    assert plain is not None and fused is not None and plain["kp_1"].shape[0] > 0
    assert torch.equal(plain["kp_1"], fused["kp_1"]) and torch.equal(plain["kp_2"], fused["kp_2"])
    bound = max(TGT_TOL, 4 * e32)
    for k in ("cost_1", "cost_2"):
        e = max_abs(fused[k], plain[k])
        print(f"runner {k}: fused vs plain e {e:.3e}, bound max(2e-6, 4 * e32) = {bound:.3e}")
        assert fused[k].shape == plain[k].shape == (15, 15) and e <= bound, k
    e, rb = max_abs(fused["cost_recip"], plain["cost_recip"]), 1e-4 * float(plain["cost_recip"].abs().max())
    print(f"runner cost_recip: fused vs plain e {e:.3e}, bound {rb:.3e}")
    assert fused["cost_recip"].shape == plain["cost_recip"].shape == (2, 2, 15, 15) and e <= rb
    # without keep_logits the shadowed decoder is the fused one itself; and nothing is left behind when the user's forward raises
    nolog = MASt3RTeacherRunner(m, inference=_inference, make_pairs=_make_pairs, fused_blocks=True).targets(im1, im2, **args)
    assert "cost_recip" not in nolog and torch.equal(nolog["cost_1"], fused["cost_1"]) and _shadows(m) == []
    m.fail_once = True
    with pytest.raises(RuntimeError, match="stub head failure"):
        runner.targets(im1, im2, **args)
    assert _shadows(m) == []
    assert m._decoder.__func__ is CL.CrocoLayout._decoder and all(b.forward.__func__ is CL.CrocoBlock.forward for b in m.enc_blocks)


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. refusals (construction only: no device launch)
# ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_block():
    from gd_amd._lib import GdHipError
    from gd_amd.teacher_blocks import FusedCroCoBlocks

    def refused(m, *words):
        with pytest.raises(GdHipError) as ei:
            FusedCroCoBlocks(m)
        assert all(w in str(ei.value) for w in words), str(ei.value)
    m = make_layout()
    m.enc_blocks[1] = CL.CrocoBlock(192, 6, m.rope)                        # head dim 32
    refused(m, "enc_blocks[1]", "head dim 32")
    m = make_layout()
    m.dec_blocks2[1].cross_attn.rope = None
    refused(m, "dec_blocks2[1]", "cross_attn.rope is None")
    m = make_layout()
    m.dec_blocks[0].attn.rope = None
    refused(m, "dec_blocks[0]", "rope is None")
    m = make_layout()
    m.dec_blocks[1].mlp.act = nn.GELU(approximate="tanh")
    refused(m, "dec_blocks[1]", "GELU")
    m = make_layout()
    m.dec_blocks[0].attn.scale = 0.1
    refused(m, "dec_blocks[0]", "scale")
    m = make_layout()
    m.enc_blocks[0].norm2 = nn.LayerNorm(192, elementwise_affine=False)
    refused(m, "enc_blocks[0]", "norm2")
    m = make_layout()
    del m.dec_blocks[0].cross_attn.projk
    refused(m, "dec_blocks[0]", "projk")
    refused(make_layout(dec_depth2=1), "dec_blocks", "dec_blocks2", "differ in length")
    with pytest.raises(GdHipError):
        FusedCroCoBlocks(make_layout(), dtype=torch.float16)
